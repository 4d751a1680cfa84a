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
    P, Lq, k, nbits, Lc, C = args.passages, args.Lq, args.k, 8, 180, args.centroids
    arch = rmr_amd.make_arch(dict(cross_encoder_num_hidden_layers=3, cross_encoder_max_position_embeddings=750, loss_fn="BCE",
                                  pos_weight=None), model_kind="interaction", has_vision=0)
    D = arch["li_dim"]
    eng = rmr_amd.RerankEngine(arch, dev)                  # a handle is all the calls need (no weights)
    lib = eng.lib
    g = torch.Generator().manual_seed(2025)
    clen = torch.randint(64, Lc + 1, (P,), generator=g)
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
    plaid = rmr_amd.PlaidSearch.defaults(k)
    kw = dict(ncells=plaid.ncells, centroid_score_threshold=plaid.centroid_score_threshold, ndocs=plaid.ndocs)

    res = dict(device=torch.cuda.get_device_name(0), passages=P, passage_rows=rows, lengths=[64, Lc], D=D, Lq=Lq, k=k, nbits=nbits,
               centroids=C, topics=args.topics, plaid=dict(kw), iters=args.iters, warmup=args.warmup, rounds=args.rounds, configs={})
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

        exhaustive()
        pruned()
        torch.cuda.synchronize()
        cand = (torch.from_numpy(eng.bank_search_plaid_tap("a1")).view(nq, P) != float("-inf")).sum(1).tolist()
        e_idx, p_idx, counts = keep["e"]["indices"].tolist(), keep["p"]["indices"].tolist(), keep["p"]["counts"].tolist()
        overlap = [len(set(e_idx[i]) & set(p_idx[i][:counts[i]])) / k for i in range(nq)]
        target_rank = [p_idx[i].index(targets[i]) if targets[i] in p_idx[i] else -1 for i in range(nq)]
        per = dict(exhaustive=[], pruned=[])
        for _ in range(args.rounds):
            for key, x in zip(("exhaustive", "pruned"), wall_ms([exhaustive, pruned], args.iters, args.warmup)):
                per[key].append(round(statistics.median(x), 4))
        mid = {key: statistics.median(v) for key, v in per.items()}
        eng.set_profiling(True)
        kernel, upto = {}, []
        for key, fn in (("exhaustive", exhaustive), ("pruned", pruned)):
            eng.get_profile(reset=True)
            fn()
            kernel[key] = round(eng.get_profile(reset=True)["tail"]["ms"], 4)
        for s in range(len(STAGES)):
            L.check(lib.rr_set_tuning(b"plaid_stop_after", s), None, "rr_set_tuning")
            t = []
            for _ in range(5):
                eng.get_profile(reset=True)
                pruned()
                t.append(eng.get_profile(reset=True)["tail"]["ms"])
            upto.append(statistics.median(t))
        L.check(lib.rr_set_tuning(b"plaid_stop_after", len(STAGES) - 1), None, "rr_set_tuning")
        eng.set_profiling(False)
        stage_ms = {name: round(upto[i] - (upto[i - 1] if i else 0.0), 4) for i, name in enumerate(STAGES)}
        res["configs"][f"nq{nq}"] = dict(
            round_medians_ms=per, exhaustive_ms=round(mid["exhaustive"], 4), pruned_ms=round(mid["pruned"], 4),
            pruned_over_exhaustive=round(mid["pruned"] / mid["exhaustive"], 4), kernel_ms=kernel,
            kernel_pruned_over_exhaustive=round(kernel["pruned"] / kernel["exhaustive"], 4), pruned_stage_ms=stage_ms,
            candidates_per_query=dict(min=min(cand), mean=round(sum(cand) / nq, 1), max=max(cand)), returned_per_query=dict(min=min(counts), max=max(counts)),
            overlap_at_k=dict(min=round(min(overlap), 4), mean=round(sum(overlap) / nq, 4)),
            top1_agrees=sum(e_idx[i][0] == p_idx[i][0] for i in range(nq)), query_source_passage_found=sum(r >= 0 for r in target_rank))
    line = json.dumps(res)
    out = args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
