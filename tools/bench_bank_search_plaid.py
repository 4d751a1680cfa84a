#!/usr/bin/env python3
"""PLAID-pruned search over a compressed passage bank (rr_bank_search_plaid) against the exhaustive search (rr_bank_search) in the
same process, on the same bank.

Bank: `--passages` passages (default 100 000) with lengths U[64, 180] at the handle's li_dim (128), PLAID residual codes at nbits
8 over `--centroids` centroids (16 384), WITH cluster structure so that pruning prunes: a passage draws its codes from
`--topics` centroids of its own (8) and its rows are those centroids plus a small residual.  Queries: Lq 32, drawn near stored
passages (the decoded rows of a random passage plus noise, renormalised), n_queries 1 and 16.  Configuration: the reference's
defaults for k = 100 (PlaidSearch.defaults: ncells 2, threshold 0.45, ndocs 1024).

Per n_queries: wall-clock ms per call of both searches including the synchronisation behind it (the median of `--iters` calls,
the two taking turns, `--rounds` times), the device time of each call's launches from the handle's profile, the device time of
every stage of the pruned call (the profile with rr_set_tuning("plaid_stop_after") at 0 .. 7, by difference), the candidates per
query (the entries of the dense A1 row that are not -inf) and overlap@k of the pruned result with the exhaustive one.

`--ivf` adds the search from the bank's inverted file (rr_bank_build_ivf, rr_bank_search_plaid_ivf) as a third leg of the same
turns, with the same queries: its wall-clock and device time, its own stage table (rr_set_tuning("plaid_ivf_stop_after") at
0 .. 8: `candidates`, `score_listed` and `select_ndocs` stand where `scan` and `select_ndocs` stand in the other), whether its
result equals the scan path's bytes, and the build time of the inverted file (the median of three builds, synchronised) with what
rr_bank_ivf_info says.  `--passages` takes several bank sizes, run one after the other in the one process: a bank above the
default is given shorter passages (the lengths are scaled so that the rows stay at the default bank's 12.2 M), so that two sizes
show how each path grows with the passages at equal rows.  With one size the record has the layout it always had; with more,
`banks` holds one such record per size.
One JSON line to stdout and to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ["centroid_scores", "cells", "bitmaps", "scan", "select_ndocs", "select_quarter", "exact_list", "select_k"]
IVF_STAGES = ["centroid_scores", "cells", "bitmaps", "candidates", "score_listed", "select_ndocs", "select_quarter", "exact_list", "select_k"]
DEFAULT_ROWS = 100000 * 122                                 # the rows of the default bank (lengths U[64, 180])


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
    ap.add_argument("--passages", type=int, nargs="+", default=[100000])
    ap.add_argument("--ivf", action="store_true")
    ap.add_argument("--Lq", type=int, default=32)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--centroids", type=int, default=16384)
    ap.add_argument("--topics", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/bank_search_plaid_bench.json.log")
    args = ap.parse_args()

    import torch
    import rmr_amd
    from rmr_amd import _lib as L

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    arch = rmr_amd.make_arch(dict(cross_encoder_num_hidden_layers=3, cross_encoder_max_position_embeddings=750, loss_fn="BCE",
                                  pos_weight=None), model_kind="interaction", has_vision=0)
    D = arch["li_dim"]
    eng = rmr_amd.RerankEngine(arch, dev)                  # a handle is all the calls need (no weights)
    banks = [run_bank(args, eng, D, P) for P in args.passages]
    res = banks[0] if len(banks) == 1 else dict(device=banks[0]["device"], banks=banks)
    line = json.dumps(res)
    out = args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    print(line)


def stage_table(eng, key, names, fn):
    """Device ms of every stage of `fn`, by difference of the profile's tail class with the stop-after switch `key` at 0, 1, ..."""
    from rmr_amd import _lib as L
    upto = []
    for s in range(len(names)):
        L.check(eng.lib.rr_set_tuning(key, s), None, "rr_set_tuning")
        t = []
        for _ in range(5):
            eng.get_profile(reset=True)
            fn()
            t.append(eng.get_profile(reset=True)["tail"]["ms"])
        upto.append(statistics.median(t))
    L.check(eng.lib.rr_set_tuning(key, len(names) - 1), None, "rr_set_tuning")
    return {name: round(upto[i] - (upto[i - 1] if i else 0.0), 4) for i, name in enumerate(names)}


def run_bank(args, eng, D, P):
    import torch
    import rmr_amd
    dev = eng.device
    Lq, k, nbits, C = args.Lq, args.k, 8, args.centroids
    scale = min(1.0, DEFAULT_ROWS / (P * 122.0))           # a larger bank: shorter passages, the same rows
    Lmin, Lc = max(1, int(64 * scale)), max(1, int(180 * scale))
    g = torch.Generator().manual_seed(2025)
    clen = torch.randint(Lmin, Lc + 1, (P,), generator=g)
    lens, rows = clen.tolist(), int(clen.sum())
    codec = rmr_amd.PlaidCodec(torch.nn.functional.normalize(torch.randn(C, D, generator=g), dim=-1),
                               torch.randn(1 << nbits, generator=g) * (0.25 / D ** 0.5), nbits)
    topics = torch.randint(0, C, (P, args.topics), generator=g)
    pid = torch.repeat_interleave(torch.arange(P), clen)
    codes = topics[pid, torch.randint(0, args.topics, (rows,), generator=g)].to(torch.int32)
    resid = torch.randint(0, 256, (rows, codec.residual_bytes), generator=g, dtype=torch.uint8)
    first = torch.cat([torch.zeros(1, dtype=torch.int64), clen.cumsum(0)[:-1]])
    bank = eng.create_bank(rows, P, codec=codec)
    bank.add_compressed(list(range(P)), codes, resid, lens)
    print(f"bank: {P} passages, {rows} rows", file=sys.stderr, flush=True)
    plaid = rmr_amd.PlaidSearch.defaults(k)
    kw = dict(ncells=plaid.ncells, centroid_score_threshold=plaid.centroid_score_threshold, ndocs=plaid.ndocs)

    res = dict(device=torch.cuda.get_device_name(0), passages=P, passage_rows=rows, lengths=[Lmin, Lc], D=D, Lq=Lq, k=k, nbits=nbits,
               centroids=C, topics=args.topics, plaid=dict(kw), iters=args.iters, warmup=args.warmup, rounds=args.rounds, configs={})
    if args.ivf:
        t = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info = bank.build_ivf()                        # synchronises
            t.append((time.perf_counter() - t0) * 1e3)
        res["ivf"] = dict(build_ms=round(statistics.median(t), 3), build_ms_runs=[round(x, 3) for x in t], **info,
                          device_bytes=8 * (C + 1) + 4 * info["postings"])
    for nq in args.queries:
        qs, targets = [], torch.randint(0, P, (nq,), generator=g).tolist()
        for t in targets:                                  # a query near passage t: Lq of its decoded rows plus noise
            r = first[t] + torch.randint(0, lens[t], (Lq,), generator=g)
            near = codec.decode(codes[r], resid[r]).float()
            qs.append(torch.nn.functional.normalize(near + 0.3 * torch.randn(Lq, D, generator=g) / D ** 0.5, dim=-1))
        q = torch.stack(qs).to(dev)
        keep = {}

        def exhaustive():
            keep["e"] = eng.bank_search(bank, q, k)

        def pruned():
            keep["p"] = eng.bank_search_plaid(bank, q, k, **kw)

        def from_ivf():
            keep["i"] = eng.bank_search_plaid_ivf(bank, q, k, **kw)

        legs = [("exhaustive", exhaustive), ("pruned", pruned)] + ([("ivf", from_ivf)] if args.ivf else [])
        for _, fn in legs:
            fn()
        torch.cuda.synchronize()
        pruned()                                           # the tap below reads the last scan call's block
        torch.cuda.synchronize()
        cand = (torch.from_numpy(eng.bank_search_plaid_tap("a1")).view(nq, P) != float("-inf")).sum(1).tolist()
        e_idx, p_idx, counts = keep["e"]["indices"].tolist(), keep["p"]["indices"].tolist(), keep["p"]["counts"].tolist()
        overlap = [len(set(e_idx[i]) & set(p_idx[i][:counts[i]])) / k for i in range(nq)]
        target_rank = [p_idx[i].index(targets[i]) if targets[i] in p_idx[i] else -1 for i in range(nq)]
        per = {key: [] for key, _ in legs}
        for _ in range(args.rounds):
            for key, x in zip(per, wall_ms([fn for _, fn in legs], args.iters, args.warmup)):
                per[key].append(round(statistics.median(x), 4))
        mid = {key: statistics.median(v) for key, v in per.items()}
        eng.set_profiling(True)
        kernel = {}
        for key, fn in legs:
            eng.get_profile(reset=True)
            fn()
            kernel[key] = round(eng.get_profile(reset=True)["tail"]["ms"], 4)
        stage_ms = stage_table(eng, b"plaid_stop_after", STAGES, pruned)
        extra = {}
        if args.ivf:
            same = all(torch.equal(keep["i"][key].view(torch.int32), keep["p"][key].view(torch.int32)) for key in ("indices", "scores", "counts"))
            extra = dict(ivf_ms=round(mid["ivf"], 4), ivf_over_pruned=round(mid["ivf"] / mid["pruned"], 4),
                         kernel_ivf_over_pruned=round(kernel["ivf"] / kernel["pruned"], 4),
                         ivf_stage_ms=stage_table(eng, b"plaid_ivf_stop_after", IVF_STAGES, from_ivf), ivf_equals_pruned=bool(same))
            cut = lambda tab, names: round(sum(tab[n] for n in names), 4)
            extra["scan_plus_select_ms"] = cut(stage_ms, ("scan", "select_ndocs"))
            extra["ivf_candidates_score_select_ms"] = cut(extra["ivf_stage_ms"], ("candidates", "score_listed", "select_ndocs"))
        eng.set_profiling(False)
        print(f"  n_queries {nq} done", file=sys.stderr, flush=True)
        res["configs"][f"nq{nq}"] = dict(
            **extra, round_medians_ms=per, exhaustive_ms=round(mid["exhaustive"], 4), pruned_ms=round(mid["pruned"], 4),
            pruned_over_exhaustive=round(mid["pruned"] / mid["exhaustive"], 4), kernel_ms=kernel,
            kernel_pruned_over_exhaustive=round(kernel["pruned"] / kernel["exhaustive"], 4), pruned_stage_ms=stage_ms,
            candidates_per_query=dict(min=min(cand), mean=round(sum(cand) / nq, 1), max=max(cand)), returned_per_query=dict(min=min(counts), max=max(counts)),
            overlap_at_k=dict(min=round(min(overlap), 4), mean=round(sum(overlap) / nq, 4)),
            top1_agrees=sum(e_idx[i][0] == p_idx[i][0] for i in range(nq)), query_source_passage_found=sum(r >= 0 for r in target_rank))
    bank.close()
    return res


if __name__ == "__main__":
    main()
