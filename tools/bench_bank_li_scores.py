#!/usr/bin/env python3
"""The retriever's scores straight from a passage bank (rr_bank_li_scores) against rr_li_scores on resident padded tensors, on an
MI355X.

    python tools/bench_bank_li_scores.py [--queries 8 --K 100 --Lq 113 --Lc 512 --nbits 8 --centroids 16384 --iters 64
                                          --warmup 16 --rounds 5 --sorted --out profiles/bank_li_scores_bench.json.log]

`queries` x `K` pairs, li_dim 128, unit-norm query rows, passage lengths U[64, Lc] (seeded).  Three legs over the SAME rows:
  (a) rr_bank_li_scores on an fp16 bank;
  (p) rr_bank_li_scores on the compressed bank (`nbits`, `centroids` random unit centroids, random residual codes) whose decoded
      rows the fp16 bank holds;
  (c) rr_li_scores on the resident padded float32 [N, Lc, D] tensor and float mask of the same pairs: what a caller without this
      call does today, and the yardstick.
Each leg in two forms: MaxSim only, and with the [N, Lc, Lq] score block.  Before anything is timed the tool asserts that the
three give the same bits.  One process; the raw C calls with every buffer allocated beforehand (a host-side lookup of 800 ids
would outweigh a 0.2 ms kernel), the legs taking turns inside an iteration, HIP events around every call, `warmup` untimed
iterations first; `rounds` repeats of the whole measurement give each leg's spread, and (a) / (p) are judged against (c)'s.
Leg (pw) is (p) under rr_set_tuning("li_lds_kb", 150): the widest column block (JT 8 at `Lq` above 64) at one workgroup per CU
and one decode per tile, against (p)'s default of two workgroups per CU, which at D 128 means JT 4, two column blocks and two
decodes per tile.  The events bracket a whole C call, which for the bank legs includes the host's descriptor loop, the wait for
the staging slot and the upload; `kernel_ms` is the `tail` class of rr_get_profile for one call of each leg (events directly
around the launch), so kernel time and call time can be told apart.
`--sorted` adds legs (as) / (ps): the same calls with the caller's pair list ordered by descending passage length.  The call
orders its workgroups that way itself (one workgroup per pair, the longest start first), so these legs show whether the caller's
order still matters; profiles/bank_li_scores_bench_call_order.json.log is this tool's record of the form that launched in call
order.  Bytes and FLOPs are the algorithm's, computed from the shapes: (a) and (p) read the rows that
exist (p: code, residual bytes and the centroid row, which comes from the 4 MiB table), (c) reads every padded row, and only (c)
multiplies pad rows.  Prints ONE JSON line and writes it to --out."""
import argparse
import json
import os
import statistics
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=8)
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--Lq", type=int, default=113)
    ap.add_argument("--Lc", type=int, default=512)
    ap.add_argument("--nbits", type=int, default=8, choices=[1, 2, 4, 8])
    ap.add_argument("--centroids", type=int, default=16384)
    ap.add_argument("--iters", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sorted", action="store_true", help="add the legs with the pair list ordered by descending length")
    ap.add_argument("--out", default="profiles/bank_li_scores_bench.json.log")
    args = ap.parse_args()

    import numpy as np
    import torch
    import rmr_amd
    from rmr_amd import _lib as L

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    Bq, K, Lq, Lc, nbits = args.queries, args.K, args.Lq, args.Lc, args.nbits
    N = Bq * K
    arch = rmr_amd.make_arch(dict(cross_encoder_num_hidden_layers=3, cross_encoder_max_position_embeddings=750, loss_fn="BCE",
                                  pos_weight=None), model_kind="interaction", has_vision=0)
    D = arch["li_dim"]
    eng = rmr_amd.RerankEngine(arch, dev)                  # a handle is all the score calls need (no weights)
    lib, st = eng.lib, torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator().manual_seed(2022)
    q = torch.nn.functional.normalize(torch.randn(Bq, Lq, D, generator=g), dim=-1).to(dev)
    clen = torch.randint(64, Lc + 1, (N,), generator=g)
    lens, rows = clen.tolist(), int(clen.sum())
    codec = rmr_amd.PlaidCodec(torch.nn.functional.normalize(torch.randn(args.centroids, D, generator=g), dim=-1),
                               torch.randn(1 << nbits, generator=g) * (0.5 / D ** 0.5), nbits)
    codes = torch.randint(0, args.centroids, (rows,), generator=g, dtype=torch.int32)
    resid = torch.randint(0, 256, (rows, codec.residual_bytes), generator=g, dtype=torch.uint8)
    ids = list(range(N))
    comp = eng.create_bank(rows, N, codec=codec)
    comp.add_compressed(ids, codes, resid, lens)
    li, cm = torch.zeros(N, Lc, D, dtype=torch.float16), torch.zeros(N, Lc)
    for i, ln in enumerate(lens):                          # the fp16 bank holds what the compressed one decodes to
        li[i, :ln], cm[i, :ln] = comp.read(i)[0], 1.0
    bank = eng.create_bank(rows, N)
    bank.add(ids, li, cm, lengths=lens)
    c32, cm32 = li.float().to(dev), cm.to(dev)             # leg (c): the padded float32 tensors, resident
    del li

    f32 = dict(device=dev, dtype=torch.float32)
    pp = np.arange(N, dtype=np.int32)
    pq = (np.arange(N) // K).astype(np.int32)
    order = np.argsort(-np.asarray(lens), kind="stable").astype(np.int32)
    pps, pqs = np.ascontiguousarray(pp[order]), np.ascontiguousarray(pq[order])
    names = ["a", "p", "c", "pw"] + (["as", "ps"] if args.sorted else [])
    sc = {k: torch.empty((N, Lc, Lq), **f32) for k in names}
    ms = {k: torch.empty(N, **f32) for k in names}

    def bank_call(b, k, with_scores, p_idx=pp, q_idx=pq, lds_kb=72):
        def fn():
            L.check(lib.rr_set_tuning(b"li_lds_kb", lds_kb), None, "rr_set_tuning")
            L.check(lib.rr_bank_li_scores(eng.h, b.h, L.ptr(q), Bq, Lq, p_idx.ctypes.data, q_idx.ctypes.data, N, Lc,
                                          L.ptr(sc[k]) if with_scores else None, L.ptr(ms[k]), st), eng.h, "rr_bank_li_scores")
        return fn

    def padded_call(with_scores):
        def fn():
            L.check(lib.rr_set_tuning(b"li_lds_kb", 72), None, "rr_set_tuning")
            L.check(lib.rr_li_scores(eng.h, L.ptr(q), L.ptr(c32), L.ptr(cm32), Bq, K, Lq, Lc, 0, N,
                                     L.ptr(sc["c"]) if with_scores else None, L.ptr(ms["c"]), st), eng.h, "rr_li_scores")
        return fn

    def legs(with_scores):
        out = [bank_call(bank, "a", with_scores), bank_call(comp, "p", with_scores), padded_call(with_scores),
               bank_call(comp, "pw", with_scores, lds_kb=150)]
        if args.sorted:
            out += [bank_call(bank, "as", with_scores, pps, pqs), bank_call(comp, "ps", with_scores, pps, pqs)]
        return out

    # equality first: with the score block, then MaxSim only (it must not depend on the block)
    for fn in legs(True):
        fn()
    torch.cuda.synchronize()
    full = {k: ms[k].clone() for k in names}
    same = all(torch.equal(sc[k], sc["c"]) and torch.equal(ms[k], ms["c"]) for k in ("a", "p", "pw"))
    if args.sorted:
        o = torch.from_numpy(order.astype(np.int64)).to(dev)
        same = same and all(torch.equal(sc[k], sc["c"][o]) and torch.equal(ms[k], ms["c"][o]) for k in ("as", "ps"))
    for k in names:
        ms[k].fill_(0.0)
    for fn in legs(False):
        fn()
    torch.cuda.synchronize()
    same = same and all(torch.equal(ms[k], full[k]) for k in names)
    assert same, "legs (a), (p) and (c) must give the same bits"

    row_bytes = dict(a=2 * D + 1, p=4 + codec.residual_bytes + 2 * D + 1)
    flops = dict(a=2.0 * rows * Lq * D, p=2.0 * rows * Lq * D, c=2.0 * N * Lc * Lq * D)
    res = dict(device=torch.cuda.get_device_name(0), Bq=Bq, K=K, Lq=Lq, Lc=Lc, D=D, nbits=nbits, centroids=args.centroids,
               iters=args.iters, warmup=args.warmup, rounds=args.rounds, passage_rows=rows, padded_rows=N * Lc,
               identical_a_p_c=bool(same), gflop={k: round(v / 1e9, 3) for k, v in flops.items()})
    for form, with_scores in (("maxsim_only", False), ("with_scores", True)):
        out_bytes = 4.0 * N + (4.0 * N * Lc * Lq if with_scores else 0.0)
        qbytes = 4.0 * N * Lq * D                           # every workgroup stages its query block (from L2 after the first)
        nbytes = dict(a=rows * row_bytes["a"] + 16.0 * N + qbytes + out_bytes, p=rows * row_bytes["p"] + 16.0 * N + qbytes + out_bytes,
                      c=N * Lc * (4.0 * D + 4.0) + qbytes + out_bytes)
        fns = legs(with_scores)
        per = {k: [] for k in names}
        for _ in range(args.rounds):
            for k, x in zip(names, event_ms(fns, args.iters, args.warmup)):
                per[k].append(round(statistics.median(x), 4))
        mid = {k: statistics.median(v) for k, v in per.items()}
        eng.set_profiling(True)                             # one call per leg: the launch alone
        kernel = {}
        for k, fn in zip(names, fns):
            eng.get_profile(reset=True)
            fn()
            kernel[k] = round(eng.get_profile(reset=True)["tail"]["ms"], 4)
        eng.set_profiling(False)
        base = {"as": "a", "ps": "p", "pw": "p"}
        c_spread = max(per["c"]) - min(per["c"])
        res[form] = dict(
            round_medians_ms=per, median_ms={k: round(v, 4) for k, v in mid.items()}, kernel_ms=kernel,
            kernel_time_over_c={k: round(kernel[k] / kernel["c"], 4) for k in names if k != "c"},
            spread_ms={k: [min(v), max(v)] for k, v in per.items()},
            c_spread_percent=round(100.0 * c_spread / mid["c"], 2),
            time_over_c={k: round(mid[k] / mid["c"], 4) for k in names if k != "c"},
            behind_c_by_more_than_its_spread={k: bool(mid[k] > mid["c"] + c_spread) for k in names if k != "c"},
            bytes={k: nbytes[base.get(k, k)] for k in names},
            gb_per_s={k: round(nbytes[base.get(k, k)] / (mid[k] * 1e-3) / 1e9, 1) for k in names},
            tflops={k: round(flops[base.get(k, k)] / (mid[k] * 1e-3) / 1e12, 2) for k in names})
    lib.rr_set_tuning(b"li_lds_kb", 72)
    line = json.dumps(res)
    out = args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
