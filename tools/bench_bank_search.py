#!/usr/bin/env python3
"""Exact top-k search over a passage bank (rr_bank_search) against what the library offered for the same answer before it:
rr_bank_li_scores over the full (query, passage) pair list, then torch.topk.

Bank: `--passages` passages (default 100 000) with lengths U[64, 180] at the handle's li_dim (128), once as PLAID residual codes
at nbits 8 and once as the fp16 bank of the decoded rows.  Queries: Lq 32, n_queries 1 and 16, k = 100.

Per (bank, n_queries): leg (s) = RerankEngine.bank_search; leg (c) = rr_bank_li_scores with MaxSim only over all n_queries x
passages pairs (the host pair arrays are built once, outside the timed call) followed by torch.topk.  The two must agree on the
indices (and on the scores, bit for bit).  Times are wall-clock per call including the synchronisation behind it, the median of
`--iters` calls, the legs taking turns, `--rounds` times; `kernel_ms` is the device time of the call's launches from the
handle's profile.  (s) at other `search_chunk` values is timed too: what the chunk length in bank_search.hip rests on.
One JSON line to stdout and to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wall_ms(fns, iters, warmup):
    import torch
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out[i].append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passages", type=int, default=100000)
    ap.add_argument("--Lq", type=int, default=32)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--centroids", type=int, default=16384)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunks", type=int, nargs="*", default=[8, 32, 64, 128], help="other search_chunk values to time leg (s) at")
    ap.add_argument("--out", default="profiles/bank_search_bench.json.log")
    args = ap.parse_args()

    import numpy as np
    import torch
    import rmr_amd
    from rmr_amd import _lib as L

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    P, Lq, k, nbits, Lc = args.passages, args.Lq, args.k, 8, 180
    arch = rmr_amd.make_arch(dict(cross_encoder_num_hidden_layers=3, cross_encoder_max_position_embeddings=750, loss_fn="BCE",
                                  pos_weight=None), model_kind="interaction", has_vision=0)
    D = arch["li_dim"]
    eng = rmr_amd.RerankEngine(arch, dev)                  # a handle is all the calls need (no weights)
    lib, st = eng.lib, torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator().manual_seed(2024)
    clen = torch.randint(64, Lc + 1, (P,), generator=g)
    lens, rows = clen.tolist(), int(clen.sum())
    codec = rmr_amd.PlaidCodec(torch.nn.functional.normalize(torch.randn(args.centroids, D, generator=g), dim=-1),
                               torch.randn(1 << nbits, generator=g) * (0.5 / D ** 0.5), nbits)
    codes = torch.randint(0, args.centroids, (rows,), generator=g, dtype=torch.int32)
    resid = torch.randint(0, 256, (rows, codec.residual_bytes), generator=g, dtype=torch.uint8)
    ids = list(range(P))
    comp = eng.create_bank(rows, P, codec=codec)
    comp.add_compressed(ids, codes, resid, lens)
    # the fp16 bank holds what the compressed one decodes to: decoded on the device by the bank's own decoder
    dec = torch.empty((rows, D), dtype=torch.float16, device=dev)
    cen, w, cd, rd = codec.centroids.to(dev), codec.bucket_weights.to(dev), codes.to(dev), resid.to(dev)
    L.check(lib.rr_op_plaid_decode_rows(L.ptr(cen), args.centroids, L.ptr(w), nbits, D, L.ptr(cd), L.ptr(rd), 0, rows, L.ptr(dec), st),
            None, "rr_op_plaid_decode_rows")
    torch.cuda.synchronize()
    del cd, rd, codes, resid
    bank = eng.create_bank(rows, P)
    first = torch.cat([torch.zeros(1, dtype=torch.int64), clen.cumsum(0)[:-1]]).to(dev)
    clen_d, t = clen.to(dev), torch.arange(Lc, device=dev)
    for a in range(0, P, 4000):
        b = min(P, a + 4000)
        keep = t[None, :] < clen_d[a:b, None]
        idx = (first[a:b, None] + t[None, :]).clamp(max=rows - 1)
        bank.add(ids[a:b], dec[idx] * keep[:, :, None], keep.float(), lengths=lens[a:b])
    torch.cuda.synchronize()
    del dec

    res = dict(device=torch.cuda.get_device_name(0), passages=P, passage_rows=rows, lengths=[64, Lc], D=D, Lq=Lq, k=k, nbits=nbits,
               centroids=args.centroids, iters=args.iters, warmup=args.warmup, rounds=args.rounds, configs={})
    found = {}
    for nq in args.queries:
        q = torch.nn.functional.normalize(torch.randn(nq, Lq, D, generator=g), dim=-1).to(dev)
        pp = np.ascontiguousarray(np.tile(np.arange(P, dtype=np.int32), nq))
        pq = np.ascontiguousarray(np.repeat(np.arange(nq, dtype=np.int32), P))
        ms = torch.empty(nq * P, device=dev, dtype=torch.float32)
        flops = 2.0 * nq * rows * Lq * D
        for name, b in (("fp16", bank), ("nbits8", comp)):
            keep = {}

            def search():
                keep["s"] = eng.bank_search(b, q, k)

            def composed():
                L.check(lib.rr_bank_li_scores(eng.h, b.h, L.ptr(q), nq, Lq, pp.ctypes.data, pq.ctypes.data, nq * P, Lc, None, L.ptr(ms), st),
                        eng.h, "rr_bank_li_scores")
                keep["c"] = torch.topk(ms.view(nq, P), k, dim=1)

            search()
            composed()
            torch.cuda.synchronize()
            same_i = bool(torch.equal(keep["s"]["indices"].long(), keep["c"].indices))
            same_s = bool(torch.equal(keep["s"]["scores"], keep["c"].values))
            assert same_i, f"{name} nq {nq}: bank_search and bank_li_scores + topk disagree on the indices"
            found[(name, nq)] = keep["s"]["indices"].clone()
            per = dict(s=[], c=[])
            for _ in range(args.rounds):
                for key, x in zip(("s", "c"), wall_ms([search, composed], args.iters, args.warmup)):
                    per[key].append(round(statistics.median(x), 4))
            mid = {key: statistics.median(v) for key, v in per.items()}
            eng.set_profiling(True)
            kernel = {}
            for key, fn in (("s", search), ("c", composed)):
                eng.get_profile(reset=True)
                fn()
                kernel[key] = round(eng.get_profile(reset=True)["tail"]["ms"], 4)
            eng.set_profiling(False)
            chunk_ms = {}
            for ch in args.chunks:
                L.check(lib.rr_set_tuning(b"search_chunk", ch), None, "rr_set_tuning")
                chunk_ms[str(ch)] = round(statistics.median(wall_ms([search], args.iters, args.warmup)[0]), 4)
                assert torch.equal(keep["s"]["indices"], found[(name, nq)])
            L.check(lib.rr_set_tuning(b"search_chunk", 16), None, "rr_set_tuning")
            res["configs"][f"{name}_nq{nq}"] = dict(
                indices_agree=same_i, scores_bit_identical=same_s, round_medians_ms=per,
                search_ms=round(mid["s"], 4), composed_ms=round(mid["c"], 4), search_over_composed=round(mid["s"] / mid["c"], 4),
                kernel_ms=kernel, kernel_search_over_composed_scoring=round(kernel["s"] / kernel["c"], 4), search_tflops=round(flops / (kernel["s"] * 1e-3) / 1e12, 2),
                composed_scoring_tflops=round(flops / (kernel["c"] * 1e-3) / 1e12, 2), search_ms_at_chunk=chunk_ms)
        assert torch.equal(found[("fp16", nq)], found[("nbits8", nq)]), "the compressed bank and its fp16 twin disagree"
    res["search_faster_everywhere"] = all(c["search_over_composed"] < 0.975 for c in res["configs"].values())
    line = json.dumps(res)
    out = args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
