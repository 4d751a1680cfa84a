#!/usr/bin/env python3
"""The interaction rerankers fed from a device-resident passage bank, against the explicit packed call, on an MI355X.

    python tools/bench_interaction_bank.py [--queries 8 --K 100 --Lq 113 --Lc 512 --iters 16 --warmup 4 --rounds 5
                                            --model-kind interaction|mores --compute-dtype fp16 --profile]
    python tools/bench_interaction_bank.py --plaid NBITS [--centroids 16384 --out profiles/interaction_bank_plaid_bench.json.log ...]

int_base geometry (Lq 113, Lc 512, D 128, 3 cross-encoder layers), `queries` x `K` candidates, unit-norm retriever embeddings
with context lengths U[64, Lc].  Three lines, pairs/s each:
  (a) RerankEngine.forward_interaction_bank: the passages are in a PassageBank (fp16 rows at their own length), the call names
      them; lengths come from the bank's host table;
  (b) RerankEngine.forward_interaction_packed with the float32 [N, Lc, D] tensors resident on the device and `lengths=` given:
      the call a caller without a bank makes when its tensors are on the device already — the yardstick;
  (c) the same with context_li / context_mask starting in pinned host memory every step: what a caller without a bank pays per
      query batch.
One process; the three take turns inside an iteration, HIP events around every call; `rounds` repeats of the whole measurement
give (b)'s own spread, against which (a) is judged.  A host clock around `iters` back-to-back calls ending in a synchronise
gives the sustained rate of each line.  `bytes` are the context-side bytes every line moves before the first GEMM, computed
from the shapes.  Prints ONE JSON line.

--plaid NBITS: the same shape from a COMPRESSED bank (PlaidCodec of `--centroids` random unit centroids, random residual codes at
the same lengths) against an fp16 bank that holds its decoded rows: line (a) as above, line (p) the compressed bank, taking turns
in one process.  The yardstick is (a) in the same run and the margin twice (a)'s own spread over the rounds.  The JSON line is
also written to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_ms(fns, iters, warmup):
    """ms of every call of each fn in `fns`, the fns taking turns (one after the other inside an iteration)."""
    import torch
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    marks = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            marks[i].append((a, b))
    torch.cuda.synchronize()
    return [[a.elapsed_time(b) for a, b in m] for m in marks]


def wall_ms(fn, iters):
    """Host ms per call of `iters` back-to-back calls, the last one waited for."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def plaid_main(args):
    import torch
    import rmr_amd

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    Bq, K, Lq, Lc, nbits = args.queries, args.K, args.Lq, args.Lc, args.plaid
    N = Bq * K
    arch = rmr_amd.make_arch(dict(cross_encoder_num_hidden_layers=3, cross_encoder_max_position_embeddings=750, loss_fn="BCE",
                                  pos_weight=None, compute_dtype=args.compute_dtype), model_kind=args.model_kind, has_vision=0)
    D = arch["li_dim"]
    eng = rmr_amd.RerankEngine(arch, dev)
    eng.load_state_dict(rmr_amd.synthetic_state_dict(arch, seed=0))
    g = torch.Generator().manual_seed(2022)
    q = torch.nn.functional.normalize(torch.randn(Bq, Lq, D, generator=g), dim=-1).to(dev)
    clen = torch.randint(64, Lc + 1, (N,), generator=g)
    lens, rows = clen.tolist(), int(clen.sum())
    qm = torch.ones(Bq, Lq, device=dev)
    codec = rmr_amd.PlaidCodec(torch.nn.functional.normalize(torch.randn(args.centroids, D, generator=g), dim=-1),
                               torch.randn(1 << nbits, generator=g) * (0.5 / D ** 0.5), nbits)
    codes = torch.randint(0, args.centroids, (rows,), generator=g, dtype=torch.int32)
    resid = torch.randint(0, 256, (rows, codec.residual_bytes), generator=g, dtype=torch.uint8)
    ids = list(range(N))
    comp = eng.create_bank(rows, N, codec=codec)
    comp.add_compressed(ids, codes, resid, lens)
    li, cm = torch.zeros(N, Lc, D, dtype=torch.float16), torch.zeros(N, Lc)
    for i, ln in enumerate(lens):                      # the fp16 bank holds what the compressed one decodes to
        li[i, :ln], cm[i, :ln] = comp.read(i)[0], 1.0
    bank = eng.create_bank(rows, N)
    bank.add(ids, li, cm, lengths=lens)
    del li

    kw = dict(want_order=True, granule=args.granule, padded_len=Lc)
    line_a = lambda: eng.forward_interaction_bank(bank, q, qm, ids, Bq, K, **kw)                       # noqa: E731
    line_p = lambda: eng.forward_interaction_bank(comp, q, qm, ids, Bq, K, **kw)                       # noqa: E731
    ra, rp = line_a(), line_p()
    torch.cuda.synchronize()
    same = torch.equal(ra["logits"], rp["logits"]) and torch.equal(ra["order"], rp["order"])
    C = int(ra["packed_rows"])
    ia, ip = bank.format(), comp.format()
    res = dict(device=torch.cuda.get_device_name(0), model_kind=args.model_kind, Bq=Bq, K=K, Lq=Lq, Lc=Lc, D=D, iters=args.iters,
               warmup=args.warmup, rounds=args.rounds, granule=args.granule, compute_dtype=args.compute_dtype, nbits=nbits,
               centroids=args.centroids, centroid_table_bytes=args.centroids * D * 2, packed_rows=C,
               packed_segments=int(ra["packed_segments"]), passage_rows=rows, logits_identical_a_p=bool(same),
               bytes_per_row=dict(a=ia["bytes_per_row"], p=ip["bytes_per_row"]),
               bank_bytes=dict(a=rows * ia["bytes_per_row"], p=rows * ip["bytes_per_row"]))
    # context-side bytes before the first GEMM: what the gather reads per bank row that exists (p: code, residual bytes, mask byte
    # from memory, and the 2 D bytes of the centroid row, which come from the table) and the 16-bit rows and float masks it writes
    res["bytes"] = dict(a=dict(device=rows * (2 * D + 1) + C * (2 * D + 4)),
                        p=dict(device=rows * ip["bytes_per_row"] + C * (2 * D + 4), centroid_table_reads=rows * 2 * D))
    rounds = []
    for _ in range(args.rounds):
        ev = event_ms([line_a, line_p], args.iters, args.warmup)
        med = [statistics.median(x) for x in ev]
        wall = [wall_ms(fn, args.iters) for fn in (line_a, line_p)]
        rounds.append(dict(event_median_ms=dict(zip("ap", (round(x, 4) for x in med))),
                           wall_ms_per_call=dict(zip("ap", (round(x, 4) for x in wall)))))
    res["rounds_detail"] = rounds
    for key in ("event_median_ms", "wall_ms_per_call"):
        per = {k: [r[key][k] for r in rounds] for k in "ap"}
        mid = {k: statistics.median(v) for k, v in per.items()}
        spread = max(per["a"]) - min(per["a"])
        res[key] = dict(median={k: round(v, 4) for k, v in mid.items()}, a_spread=[min(per["a"]), max(per["a"])],
                        a_spread_percent=round(100.0 * spread / mid["a"], 3),
                        pairs_per_s={k: round(N / (v * 1e-3), 1) for k, v in mid.items()},
                        p_over_a=round(mid["a"] / mid["p"], 4),                                      # ratio of pairs/s
                        p_minus_a_percent=round(100.0 * (mid["p"] - mid["a"]) / mid["a"], 3),
                        p_within_twice_a_spread=bool(mid["p"] <= mid["a"] + 2.0 * spread))
    if args.profile:
        eng.set_profiling(True)
        res["profile_ms"] = {}
        for name, fn in (("a", line_a), ("p", line_p)):
            eng.get_profile(reset=True)
            fn()
            p = eng.get_profile(reset=True)
            res["profile_ms"][name] = {k: round(v["ms"], 4) for k, v in p.items() if v["launches"]}
        eng.set_profiling(False)
    line = json.dumps(res)
    out = args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=8)
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--Lq", type=int, default=113)
    ap.add_argument("--Lc", type=int, default=512)
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--granule", type=int, default=16)
    ap.add_argument("--model-kind", default="interaction", choices=["interaction", "mores"])
    ap.add_argument("--compute-dtype", default="fp16", choices=["bf16", "fp16"])
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--plaid", type=int, default=0, choices=[0, 1, 2, 4, 8], help="compressed bank of NBITS against the fp16 bank of its decoded rows")
    ap.add_argument("--centroids", type=int, default=16384, help="--plaid: centroids of the codec (16384 x 128 fp16 = 4 MiB)")
    ap.add_argument("--out", default="profiles/interaction_bank_plaid_bench.json.log", help="--plaid: where the JSON line is written")
    args = ap.parse_args()
    if args.plaid:
        return plaid_main(args)

    import torch
    import rmr_amd

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    Bq, K, Lq, Lc = args.queries, args.K, args.Lq, args.Lc
    N = Bq * K
    arch = rmr_amd.make_arch(dict(cross_encoder_num_hidden_layers=3, cross_encoder_max_position_embeddings=750, loss_fn="BCE",
                                  pos_weight=None, compute_dtype=args.compute_dtype), model_kind=args.model_kind, has_vision=0)
    D = arch["li_dim"]
    eng = rmr_amd.RerankEngine(arch, dev)
    eng.load_state_dict(rmr_amd.synthetic_state_dict(arch, seed=0))
    g = torch.Generator().manual_seed(2022)
    q = torch.nn.functional.normalize(torch.randn(Bq, Lq, D, generator=g), dim=-1).to(dev)
    c_host = torch.nn.functional.normalize(torch.randn(N, Lc, D, generator=g), dim=-1).pin_memory()
    clen = torch.randint(64, Lc + 1, (N,), generator=g)
    cm_host = (torch.arange(Lc)[None, :] < clen[:, None]).float().pin_memory()
    lens = clen.tolist()
    qm = torch.ones(Bq, Lq, device=dev)
    c, cm = c_host.to(dev), cm_host.to(dev)
    ids = list(range(N))
    bank = eng.create_bank(int(clen.sum()), N)
    bank.add(ids, c, cm, lengths=lens)

    kw = dict(want_order=True, granule=args.granule)
    line_a = lambda: eng.forward_interaction_bank(bank, q, qm, ids, Bq, K, **kw)                       # noqa: E731
    line_b = lambda: eng.forward_interaction_packed(q, c, qm, cm, Bq, K, lengths=lens, **kw)           # noqa: E731
    line_c = lambda: eng.forward_interaction_packed(q, c_host.to(dev, non_blocking=True), qm,          # noqa: E731
                                                    cm_host.to(dev, non_blocking=True), Bq, K, lengths=lens, **kw)
    ra, rb = line_a(), line_b()
    torch.cuda.synchronize()
    same = torch.equal(ra["logits"], rb["logits"]) and torch.equal(ra["order"], rb["order"])
    C = int(ra["packed_rows"])                 # context rows computed (the same segments in all three lines)
    rows = int(clen.sum())
    res = dict(device=torch.cuda.get_device_name(0), model_kind=args.model_kind, Bq=Bq, K=K, Lq=Lq, Lc=Lc, D=D, iters=args.iters,
               warmup=args.warmup, rounds=args.rounds, granule=args.granule, compute_dtype=args.compute_dtype,
               packed_rows=C, packed_segments=int(ra["packed_segments"]), passage_rows=rows,
               logits_identical_a_b=bool(same))
    # context-side bytes before the first GEMM.  (a): the gather reads the bank rows and mask bytes that exist and writes the
    # 16-bit rows and float masks of the segments; the per-pair descriptors (16 bytes each) are all that is uploaded.  (b): pack_rows
    # is index_select over the padded tensor (read + write [N, Lc, D] float32), then slice + cat per segment (read + write the C rows),
    # then the conversion (read float32, write 16 bits); masks alike.  (c): (b) plus the upload of both padded tensors.
    dev_a = rows * (2 * D + 1) + C * (2 * D + 4)
    dev_b = 2 * N * Lc * (4 * D + 4) + 2 * C * (4 * D + 4) + C * (4 * D + 2 * D + 4)
    res["bytes"] = dict(a=dict(host_to_device=16 * N, device=dev_a), b=dict(host_to_device=0, device=dev_b),
                        c=dict(host_to_device=N * Lc * (4 * D + 4), device=dev_b))

    rounds = []
    for _ in range(args.rounds):
        ev = event_ms([line_a, line_b, line_c], args.iters, args.warmup)
        med = [statistics.median(x) for x in ev]
        wall = [wall_ms(fn, args.iters) for fn in (line_a, line_b, line_c)]
        rounds.append(dict(event_median_ms=dict(zip("abc", (round(x, 4) for x in med))),
                           wall_ms_per_call=dict(zip("abc", (round(x, 4) for x in wall)))))
    res["rounds_detail"] = rounds
    for key in ("event_median_ms", "wall_ms_per_call"):
        per = {k: [r[key][k] for r in rounds] for k in "abc"}
        mid = {k: statistics.median(v) for k, v in per.items()}
        res[key] = dict(median={k: round(v, 4) for k, v in mid.items()},
                        b_spread=[min(per["b"]), max(per["b"])],
                        pairs_per_s={k: round(N / (v * 1e-3), 1) for k, v in mid.items()},
                        a_over_b=round(mid["b"] / mid["a"], 4), a_over_c=round(mid["c"] / mid["a"], 4),     # ratios of pairs/s
                        a_slower_than_b_spread=bool(mid["a"] > max(per["b"])))
    if args.profile:
        eng.set_profiling(True)
        res["profile_ms"] = {}
        for name, fn in (("a", line_a), ("b", line_b)):
            eng.get_profile(reset=True)
            fn()
            p = eng.get_profile(reset=True)
            res["profile_ms"][name] = {k: round(v["ms"], 4) for k, v in p.items() if v["launches"]}
        eng.set_profiling(False)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
