#!/usr/bin/env python3
"""The three bank searches under a candidate filter (rr_bank_search_filtered, rr_bank_search_plaid_filtered,
rr_bank_search_plaid_ivf_filtered) against their unfiltered entries in the same process, on the bank of
tools/bench_bank_search_plaid.py: 100 000 passages of U[64, 180] rows at the handle's li_dim (128), nbits 8 over 16 384 centroids
with cluster structure, Lq 32, k 100, PlaidSearch.defaults(k); the same generator and seed, so the same bank and queries.

Per n_queries (1 and 16) and per density (1.0, 0.5, 0.1, 0.01 of the passages, one shared random row; at 1.0 every bit is set) and
for each of the three searches: wall-clock ms per call of the filtered and of the unfiltered entry including the synchronisation
behind it, the two taking turns (the median of `--iters` calls, `--rounds` times; the record keeps every round's median), their
ratio, the fraction of passages the filter allows, and the unfiltered entry's own spread over the rounds ((max - min) / median of
its round medians), beside which a ratio is to be read.  At density 1.0 the filtered result must equal the unfiltered bytes; the
record says whether it did.  Nothing here is a gate.

`--sparse` measures the exact search only, and its list-driven form (rr_bank_search_filtered_sparse): per bank (`--sparse-passages`:
100 000 passages, and the 800 000-passage bank of tools/bench_bank_search_plaid.py --ivf, the same rows in shorter passages), per
n_queries (1 and 16), with one shared filter row and with one row per query, at the densities 1.0, 0.5, 0.1, 0.01, 0.001 and 0.0
(an all-clear filter: the floor of a call whose workgroups all return at once), three legs take turns in one process: `sparse`;
`dense`, rr_bank_search_filtered; `composed`, bank_li_scores over the explicit (query, passage) pairs and torch.topk per query (up
to `--composed-max-pairs` pairs: the route is meant for a few thousand).  Wall-clock ms per call with the synchronisation inside
the span, the median of `--iters` calls `--rounds` times, every round's median kept; sparse / dense and sparse / composed beside
the dense leg's own spread over its rounds.  Before anything is timed the sparse and the dense result are asserted equal as bytes.
With `--profile` (a run of its own: profiling serialises the launches) the record holds device ms instead: the dense call, and the
sparse call stage by stage (compaction, scoring, selection) from the handle's profile with rr_set_tuning("sparse_stop_after") at
0, 1, 2, by difference.  The default --out becomes profiles/bank_search_sparse_bench.json.log; `--profile` puts its record under the
key "profile" of the record --out holds already, so that the file stays one line.
One JSON line to stdout and to --out."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

DEFAULT_ROWS = 100000 * 122


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passages", type=int, default=100000)
    ap.add_argument("--Lq", type=int, default=32)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--densities", type=float, nargs="+", default=[1.0, 0.5, 0.1, 0.01])
    ap.add_argument("--centroids", type=int, default=16384)
    ap.add_argument("--topics", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sparse", action="store_true")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--sparse-passages", type=int, nargs="+", default=[100000, 800000])
    ap.add_argument("--sparse-densities", type=float, nargs="+", default=[1.0, 0.5, 0.1, 0.01, 0.001, 0.0])
    ap.add_argument("--composed-max-pairs", type=int, default=200000)
    args = ap.parse_args()
    if args.profile and not args.sparse:
        ap.error("--profile goes with --sparse")
    if args.out is None:
        args.out = "profiles/bank_search_sparse_bench.json.log" if args.sparse else "profiles/bank_search_filter_bench.json.log"
    if args.sparse:
        return sparse_main(args)

    import numpy as np
    import torch
    import rmr_amd
    from bench_bank_search_plaid import wall_ms

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    arch = rmr_amd.make_arch(dict(cross_encoder_num_hidden_layers=3, cross_encoder_max_position_embeddings=750, loss_fn="BCE",
                                  pos_weight=None), model_kind="interaction", has_vision=0)
    D = arch["li_dim"]
    eng = rmr_amd.RerankEngine(arch, dev)
    P, Lq, k, nbits, C = args.passages, args.Lq, args.k, 8, args.centroids
    # the bank of bench_bank_search_plaid.py's run_bank, draw for draw
    scale = min(1.0, DEFAULT_ROWS / (P * 122.0))
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
    info = bank.build_ivf()
    print(f"bank: {P} passages, {rows} rows", file=sys.stderr, flush=True)
    plaid = rmr_amd.PlaidSearch.defaults(k)
    kw = dict(ncells=plaid.ncells, centroid_score_threshold=plaid.centroid_score_threshold, ndocs=plaid.ndocs)
    rng = np.random.default_rng(2025)
    filters = {}
    for d in args.densities:
        allowed = list(range(P)) if d >= 1.0 else np.flatnonzero(rng.random(P) < d).tolist()
        filters[d] = (bank.filter(allowed=allowed), len(allowed) / P)

    res = dict(device=torch.cuda.get_device_name(0), passages=P, passage_rows=rows, D=D, Lq=Lq, k=k, nbits=nbits, centroids=C,
               topics=args.topics, plaid=dict(kw), ivf=info, iters=args.iters, warmup=args.warmup, rounds=args.rounds, configs={})
    searches = dict(
        exact=(lambda q: eng.bank_search(bank, q, k), lambda q, f: eng.bank_search_filtered(bank, q, k, f)),
        plaid=(lambda q: eng.bank_search_plaid(bank, q, k, **kw), lambda q, f: eng.bank_search_plaid_filtered(bank, q, k, f, **kw)),
        plaid_ivf=(lambda q: eng.bank_search_plaid_ivf(bank, q, k, **kw), lambda q, f: eng.bank_search_plaid_ivf_filtered(bank, q, k, f, **kw)))
    for nq in args.queries:
        qs, targets = [], torch.randint(0, P, (nq,), generator=g).tolist()
        for t in targets:
            r = first[t] + torch.randint(0, lens[t], (Lq,), generator=g)
            near = codec.decode(codes[r], resid[r]).float()
            qs.append(torch.nn.functional.normalize(near + 0.3 * torch.randn(Lq, D, generator=g) / D ** 0.5, dim=-1))
        q = torch.stack(qs).to(dev)
        cfg = {}
        for name, (plain, filtered) in searches.items():
            per_density = {}
            for d, (f, frac) in filters.items():
                keep = {}

                def run_plain():
                    keep["u"] = plain(q)

                def run_filtered():
                    keep["f"] = filtered(q, f)

                rounds = {"unfiltered": [], "filtered": []}
                for _ in range(args.rounds):
                    for key, x in zip(rounds, wall_ms([run_plain, run_filtered], args.iters, args.warmup)):
                        rounds[key].append(round(statistics.median(x), 4))
                u, fl = statistics.median(rounds["unfiltered"]), statistics.median(rounds["filtered"])
                rec = dict(allowed_fraction=round(frac, 5), unfiltered_ms=round(u, 4), filtered_ms=round(fl, 4),
                           filtered_over_unfiltered=round(fl / u, 4),
                           unfiltered_spread=round((max(rounds["unfiltered"]) - min(rounds["unfiltered"])) / u, 4), round_medians_ms=rounds,
                           returned_per_query=dict(min=int(keep["f"]["counts"].min()), max=int(keep["f"]["counts"].max())))
                if d >= 1.0:
                    rec["equals_unfiltered"] = all(torch.equal(keep["f"][key].view(torch.int32), keep["u"][key].view(torch.int32))
                                                   for key in keep["u"])
                per_density[str(d)] = rec
            cfg[name] = per_density
            print(f"  n_queries {nq} {name} done", file=sys.stderr, flush=True)
        res["configs"][f"nq{nq}"] = cfg
    bank.close()
    line = json.dumps(res)
    out = args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    print(line)


def _bank(args, eng, rmr_amd, torch, P, D):
    """The bank of bench_bank_search_plaid.py's run_bank, draw for draw, and what the queries are drawn from."""
    nbits, C = 8, args.centroids
    scale = min(1.0, DEFAULT_ROWS / (P * 122.0))
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
    return bank, rows, [Lmin, Lc], g, codec, codes, resid, first, lens


def sparse_main(args):
    import numpy as np
    import torch
    import rmr_amd
    from rmr_amd import _lib as L
    from bench_bank_search_plaid import wall_ms

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    arch = rmr_amd.make_arch(dict(cross_encoder_num_hidden_layers=3, cross_encoder_max_position_embeddings=750, loss_fn="BCE",
                                  pos_weight=None), model_kind="interaction", has_vision=0)
    D = arch["li_dim"]
    eng = rmr_amd.RerankEngine(arch, dev)
    Lq, k = args.Lq, args.k
    res = dict(device=torch.cuda.get_device_name(0), mode="profile" if args.profile else "wall", D=D, Lq=Lq, k=k, nbits=8,
               centroids=args.centroids, topics=args.topics, iters=args.iters, warmup=args.warmup, rounds=args.rounds,
               composed_max_pairs=args.composed_max_pairs, banks=[])
    for P in args.sparse_passages:
        bank, rows, lengths, g, codec, codes, resid, first, lens = _bank(args, eng, rmr_amd, torch, P, D)
        print(f"bank: {P} passages, {rows} rows", file=sys.stderr, flush=True)
        rng = np.random.default_rng(2025)
        rec_bank = dict(passages=P, passage_rows=rows, lengths=lengths, configs={})
        for nq in args.queries:
            qs, targets = [], torch.randint(0, P, (nq,), generator=g).tolist()
            for t in targets:
                r = first[t] + torch.randint(0, lens[t], (Lq,), generator=g)
                near = codec.decode(codes[r], resid[r]).float()
                qs.append(torch.nn.functional.normalize(near + 0.3 * torch.randn(Lq, D, generator=g) / D ** 0.5, dim=-1))
            q = torch.stack(qs).to(dev)
            for rows_kind in (["shared"] if nq == 1 else ["shared", "per_query"]):
                nrows = 1 if rows_kind == "shared" else nq
                per_density = {}
                for d in args.sparse_densities:
                    # the bitmap packed here (bit i & 31 of word i >> 5 = passage i), not through bank.filter: sixteen rows of 800 000
                    # ids would spend their time in the id table
                    on = np.ones((nrows, P), dtype=bool) if d >= 1.0 else rng.random((nrows, P)) < d
                    words = (P + 31) // 32
                    padded = np.zeros((nrows, words * 32), dtype=bool)
                    padded[:, :P] = on
                    packed = np.packbits(padded.reshape(nrows, words, 32), axis=2, bitorder="little").view("<u4").reshape(nrows, words)
                    f = rmr_amd.BankFilter(torch.from_numpy(packed.view(np.int32)).to(dev), nrows, P, bank.generation)
                    lists = [np.flatnonzero(r).tolist() for r in on]
                    sizes = [len(lists[0 if nrows == 1 else i]) for i in range(nq)]
                    pairs = sum(sizes)
                    keep = {}

                    def sparse():
                        keep["s"] = eng.bank_search_filtered_sparse(bank, q, k, f)

                    def dense():
                        keep["d"] = eng.bank_search_filtered(bank, q, k, f)

                    flat = [p for i in range(nq) for p in lists[0 if nrows == 1 else i]] if 0 < pairs <= args.composed_max_pairs else []

                    def composed():
                        ms = eng.bank_li_scores(bank, q, flat, list_sizes=sizes)["maxsim"]
                        keep["c"] = [torch.topk(part, min(k, part.numel())) for part in torch.split(ms, sizes) if part.numel()]

                    sparse()
                    dense()
                    torch.cuda.synchronize()
                    for key in ("indices", "scores", "counts"):      # equal bytes before anything is timed
                        assert torch.equal(keep["s"][key].view(torch.int32), keep["d"][key].view(torch.int32)), (P, nq, rows_kind, d, key)
                    rec = dict(allowed_fraction=round(pairs / (nq * P), 6), allowed_per_query=dict(min=min(sizes), max=max(sizes)),
                               returned_per_query=dict(min=int(keep["s"]["counts"].min()), max=int(keep["s"]["counts"].max())),
                               sparse_equals_dense=True)
                    if args.profile:
                        rec = dict(allowed_per_query=rec["allowed_per_query"])      # the wall-clock record beside it holds the rest
                        eng.set_profiling(True)

                        def tail(fn):
                            t = []
                            for _ in range(5):
                                eng.get_profile(reset=True)
                                fn()
                                t.append(eng.get_profile(reset=True)["tail"]["ms"])
                            return statistics.median(t)
                        upto = []
                        for stage in range(3):
                            L.check(eng.lib.rr_set_tuning(b"sparse_stop_after", stage), None, "rr_set_tuning")
                            upto.append(tail(sparse))
                        rec.update(dense_device_ms=round(tail(dense), 4), sparse_device_ms=round(upto[2], 4),
                                   sparse_stage_ms=dict(compaction=round(upto[0], 4), scoring=round(upto[1] - upto[0], 4),
                                                        selection=round(upto[2] - upto[1], 4)))
                        eng.set_profiling(False)
                    else:
                        legs = [("sparse", sparse), ("dense", dense)] + ([("composed", composed)] if 0 < pairs <= args.composed_max_pairs else [])
                        rounds = {key: [] for key, _ in legs}
                        for _ in range(args.rounds):
                            for key, x in zip(rounds, wall_ms([fn for _, fn in legs], args.iters, args.warmup)):
                                rounds[key].append(round(statistics.median(x), 4))
                        mid = {key: statistics.median(v) for key, v in rounds.items()}
                        rec.update(sparse_ms=round(mid["sparse"], 4), dense_ms=round(mid["dense"], 4),
                                   sparse_over_dense=round(mid["sparse"] / mid["dense"], 4),
                                   dense_spread=round((max(rounds["dense"]) - min(rounds["dense"])) / mid["dense"], 4),
                                   composed_ms=round(mid["composed"], 4) if "composed" in mid else None,
                                   sparse_over_composed=round(mid["sparse"] / mid["composed"], 4) if "composed" in mid else None,
                                   round_medians_ms=rounds)
                    per_density[str(d)] = rec
                rec_bank["configs"][f"nq{nq}_{rows_kind}"] = per_density
                print(f"  {P} passages, n_queries {nq}, {rows_kind} done", file=sys.stderr, flush=True)
        res["banks"].append(rec_bank)
        bank.close()
    out = args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if args.profile and os.path.exists(out):                  # beside the wall-clock record of an earlier run
        res = dict(json.loads([l for l in open(out) if l.startswith("{")][-1]), profile=res)
    line = json.dumps(res)
    with open(out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
