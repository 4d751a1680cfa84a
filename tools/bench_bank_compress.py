#!/usr/bin/env python3
"""Filling a compressed passage bank from embeddings on the device: PassageBank.add_compress (rr_bank_add_compress) against the
path a user composes without it, in the same process, on the same device tensors.

Shape: `--passages` passages (512) padded to Lc 180 with lengths U[64, 180], li_dim 128, nbits 8, `--centroids` centroids (65 536).
Rows are centroids plus a small residual, renormalised, handed over as fp16 (what a retriever's `.half()` gives).

  add_compress   one call from the padded device tensors with the host's lengths, and the synchronisation behind it;
  composed       on the kept rows, as the reference's ResidualCodec.compress does it on a GPU: float32 `centroids @ rows.T` in
                 chunks of (1 << 29) // centroids rows with `.max(0)`, the float32 residual, torch.bucketize, the bit packing by
                 shifts and a weighted sum, then PassageBank.add_compressed through the host.
  add_fp16       PassageBank.add (rr_bank_add) of the same tensors into an fp16 bank of the same capacity, timed the same way in
                 rounds of its own.

Wall-clock ms per call (median of `--iters` calls, the two taking turns, `--rounds` times; the bank is cleared between calls), the
device time of add_compress between two events, the same with rr_set_tuning("compress_stop_after") = 0: the row map and the
assignment kernel alone, and that kernel's TFLOP/s (2 * rows * centroids * li_dim) beside the 155 the f32 matrix core gives and
the 54 li_scores_kernel reaches.  The two paths' codes are compared on the first passages (the composed path sums in another
order: rows whose two best centroids lie within rounding of each other may differ).  For scale beside the compress time: the
build of the bank's inverted file over the passages just compressed (PassageBank.build_ivf, rr_bank_build_ivf: the median of three
builds, synchronisation included).  One JSON line to stdout and to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passages", type=int, default=512)
    ap.add_argument("--centroids", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/bank_compress_bench.json.log")
    args = ap.parse_args()

    import torch
    import rmr_amd
    from rmr_amd import _lib as L

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    P, Lc, nbits, Cn = args.passages, 180, 8, args.centroids
    arch = rmr_amd.make_arch(dict(cross_encoder_num_hidden_layers=3, cross_encoder_max_position_embeddings=750, loss_fn="BCE",
                                  pos_weight=None), model_kind="interaction", has_vision=0)
    D = arch["li_dim"]
    eng = rmr_amd.RerankEngine(arch, dev)                  # a handle is all the calls need (no weights)
    lib = eng.lib
    g = torch.Generator(device=dev).manual_seed(2025)
    cen = torch.nn.functional.normalize(torch.randn(Cn, D, generator=g, device=dev), dim=-1).half()
    lens_t = torch.randint(64, Lc + 1, (P,), generator=g, device=dev)
    lens = lens_t.tolist()
    R = sum(lens)
    pick = torch.randint(0, Cn, (P, Lc), generator=g, device=dev)
    li = torch.nn.functional.normalize(cen[pick].float() + 0.35 * torch.randn(P, Lc, D, generator=g, device=dev) / D ** 0.5, dim=-1).half()
    keep = torch.arange(Lc, device=dev)[None, :] < lens_t[:, None]
    cm = keep.float()
    resid = (li.float() - cen[pick].float())[keep].flatten()[:1 << 22].cpu()
    nb = 1 << nbits
    cutoffs = resid.quantile(torch.arange(1, nb) / nb).float()
    weights = resid.quantile((torch.arange(0, nb) + 0.5) / nb).float()
    codec = rmr_amd.PlaidCodec(cen, weights, nbits, bucket_cutoffs=cutoffs)
    bank = eng.create_bank(R, P, codec=codec)
    plain = eng.create_bank(R, P)
    ids = list(range(P))
    cen32, cut_d = cen.float(), cutoffs.to(dev)
    shifts = torch.arange(nbits, device=dev, dtype=torch.int32)
    place = (2 ** torch.arange(7, -1, -1, device=dev)).to(torch.int32)
    last = {}

    def fused():
        bank.clear()
        bank.add_compress(ids, li, cm, lengths=lens)

    def add_fp16():
        plain.clear()
        plain.add(ids, li, cm, lengths=lens)

    def composed():
        bank.clear()
        rows = li[keep]                                    # [R, D] fp16
        codes = torch.cat([(cen32 @ b.T.float()).max(dim=0).indices for b in rows.split((1 << 29) // Cn)])
        r = rows.float() - cen32[codes]
        bits = (torch.bucketize(r, cut_d).to(torch.int32).unsqueeze(-1) >> shifts) & 1
        packed = (bits.reshape(R, D * nbits // 8, 8) * place).sum(-1).to(torch.uint8)
        last["codes"], last["res"] = codes.to(torch.int32).cpu(), packed.cpu()
        bank.add_compressed(ids, last["codes"], last["res"], lens)

    def wall(fns):
        for _ in range(args.warmup):
            for fn in fns:
                fn()
        torch.cuda.synchronize()
        out = [[] for _ in fns]
        for _ in range(args.iters):
            for i, fn in enumerate(fns):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                out[i].append((time.perf_counter() - t0) * 1e3)
        return out

    def device_ms(fn, n=5):
        t = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            t.append(a.elapsed_time(b))
        return statistics.median(t)

    per = dict(add_compress=[], composed=[], add_fp16=[])
    for _ in range(args.rounds):
        for key, x in zip(("add_compress", "composed"), wall([fused, composed])):
            per[key].append(round(statistics.median(x), 3))
    for _ in range(args.rounds):
        per["add_fp16"].append(round(statistics.median(wall([add_fp16])[0]), 3))
    mid = {k: statistics.median(v) for k, v in per.items()}
    composed()
    want_codes, want_res = last["codes"], last["res"]
    fused()
    n_cmp = min(P, 64)
    same_code = same_rows = rows_cmp = 0
    o = 0
    for i in range(n_cmp):
        c, r, _ = bank.read_compressed(i)
        eq = c == want_codes[o:o + lens[i]]
        same_code += int(eq.sum())
        same_rows += int((eq & (r == want_res[o:o + lens[i]]).all(1)).sum())
        rows_cmp += lens[i]
        o += lens[i]
    ivf_ms = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ivf = bank.build_ivf()                             # synchronises
        ivf_ms.append((time.perf_counter() - t0) * 1e3)
    call_dev = device_ms(fused)
    L.check(lib.rr_set_tuning(b"compress_stop_after", 0), None, "rr_set_tuning")
    try:
        assign_dev = device_ms(fused)
    finally:
        L.check(lib.rr_set_tuning(b"compress_stop_after", 1), None, "rr_set_tuning")
    flop = 2.0 * R * Cn * D
    res = dict(device=torch.cuda.get_device_name(0), passages=P, Lc=Lc, lengths=[64, Lc], rows=R, D=D, nbits=nbits, centroids=Cn,
               iters=args.iters, warmup=args.warmup, rounds=args.rounds, round_medians_ms=per,
               add_compress_ms=round(mid["add_compress"], 3), composed_ms=round(mid["composed"], 3),
               add_compress_over_composed=round(mid["add_compress"] / mid["composed"], 4), add_fp16_ms=round(mid["add_fp16"], 3),
               add_compress_device_ms=round(call_dev, 3), assign_kernel_ms=round(assign_dev, 3),
               assign_tflops=round(flop / (assign_dev * 1e-3) / 1e12, 2), f32_matrix_core_tflops=155, li_scores_kernel_tflops=54,
               compared_rows=rows_cmp, codes_equal=same_code, rows_equal_where_codes_equal=same_rows,
               ivf_build_ms=round(statistics.median(ivf_ms), 3), ivf_postings=ivf["postings"], ivf_longest_list=ivf["longest_list"])
    line = json.dumps(res)
    out = args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
