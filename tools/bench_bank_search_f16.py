#!/usr/bin/env python3
"""The exhaustive bank search whose first pass runs on the fp16 matrix core (rr_bank_search_f16) against the exact exhaustive search
(rr_bank_search) and the two pruned searches, over the same rows, in one process.

Banks: the two coded fp16 banks of tools/bench_bank_search_coded.py, one after the other: 100 000 passages of 64 .. 180 rows and
800 000 passages of 8 .. 22 rows (about 12.2 M rows each, D 128, rows near 8 of 16 384 centroids per passage).  Queries: Lq 32, near
stored passages; n_queries 1, 16 and 64; ndocs 1024, k 100; PlaidSearch.defaults(k) for the pruned legs.
The legs take turns in one process (exhaustive, f16, pruned, inverted-file), `--iters` calls each behind `--warmup` unmeasured
rounds, `--rounds` times; reported: the median of the round medians and the round medians, wall-clock ms per call with the
synchronisation.  Device ms per stage of the f16 call through rr_set_tuning("f16_stop_after"), by difference of the profile's tail
class ("scores_f16" is the scoring launch alone), and the device ms of the whole exhaustive call.  certified: the share of the
queries the f16 call certifies at the default slack; overlap@k: the share of the exhaustive top k that each other leg returns; for
certified queries the f16 result must be the exhaustive call's bytes (asserted).
One JSON line to stdout and to --out."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_bank_search_plaid import DEFAULT_ROWS, stage_table, wall_ms  # noqa: E402

CHUNK = 2048                                                # passages per add
F16_STAGES = ["scores_f16", "select_ndocs", "exact_list", "select_k_certify"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passages", type=int, nargs="+", default=[100000, 800000])
    ap.add_argument("--Lq", type=int, default=32)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--ndocs", type=int, default=1024)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--centroids", type=int, default=16384)
    ap.add_argument("--topics", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/bank_search_f16_bench.json.log")
    args = ap.parse_args()

    import torch
    import rmr_amd

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    arch = rmr_amd.make_arch(dict(cross_encoder_num_hidden_layers=3, cross_encoder_max_position_embeddings=750, loss_fn="BCE",
                                  pos_weight=None), model_kind="interaction", has_vision=0)
    eng = rmr_amd.RerankEngine(arch, dev)                  # a handle is all the calls need (no weights)
    banks = [run_bank(args, eng, arch["li_dim"], P) for P in args.passages]
    line = json.dumps(dict(device=torch.cuda.get_device_name(0), banks=banks))
    out = args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    print(line)


def run_bank(args, eng, D, P):
    import torch
    import rmr_amd
    dev = eng.device
    Lq, k, C, ndocs = args.Lq, args.k, args.centroids, args.ndocs
    scale = min(1.0, DEFAULT_ROWS / (P * 122.0))           # a larger bank: shorter passages, the same rows
    Lmin, Lc = max(1, int(64 * scale)), max(1, int(180 * scale))
    g = torch.Generator().manual_seed(2025)
    clen = torch.randint(Lmin, Lc + 1, (P,), generator=g)
    lens, rows = clen.tolist(), int(clen.sum())
    cen = torch.nn.functional.normalize(torch.randn(C, D, generator=g), dim=-1).half()
    topics = torch.randint(0, C, (P, args.topics), generator=g).to(dev)
    cen_d = cen.float().to(dev)
    F = eng.create_bank(rows, P, centroids=cen)
    dg = torch.Generator(device=dev).manual_seed(7)
    for c0 in range(0, P, CHUNK):
        n = min(CHUNK, P - c0)
        pick = topics[c0:c0 + n].gather(1, torch.randint(0, args.topics, (n, Lc), generator=dg, device=dev))
        x = torch.nn.functional.normalize(cen_d[pick] + 0.5 * torch.randn(n, Lc, D, generator=dg, device=dev) / D ** 0.5, dim=-1).half()
        m = (torch.arange(Lc, device=dev)[None, :] < clen[c0:c0 + n].to(dev)[:, None]).float()
        F.add(list(range(c0, c0 + n)), x, m, lengths=lens[c0:c0 + n])
    F.build_ivf()
    print(f"bank: {P} passages, {rows} rows", file=sys.stderr, flush=True)
    plaid = rmr_amd.PlaidSearch.defaults(k)
    kw = dict(ncells=plaid.ncells, centroid_score_threshold=plaid.centroid_score_threshold, ndocs=plaid.ndocs)
    res = dict(passages=P, passage_rows=rows, lengths=[Lmin, Lc], D=D, Lq=Lq, k=k, ndocs=ndocs, centroids=C, topics=args.topics, plaid=dict(kw),
               configs={})
    for nq in args.queries:
        qs, targets = [], torch.randint(0, P, (nq,), generator=g).tolist()
        for t_ in targets:                                 # a query near passage t: Lq of its rows plus noise
            rws, _ = F.read(t_)
            near = rws.float()[torch.randint(0, lens[t_], (Lq,), generator=g)]
            qs.append(torch.nn.functional.normalize(near + 0.3 * torch.randn(Lq, D, generator=g) / D ** 0.5, dim=-1))
        q = torch.stack(qs).to(dev)
        slack = rmr_amd.F16Search(ndocs).slack_for(q)       # once: the legs time the call, not the reduction before it
        keep = {}
        legs = [("exhaustive", lambda: keep.__setitem__("e", eng.bank_search(F, q, k))),
                ("f16", lambda: keep.__setitem__("f", eng.bank_search_f16(F, q, k, ndocs, slack=slack))),
                ("coded_pruned", lambda: keep.__setitem__("p", eng.bank_search_plaid(F, q, k, **kw))),
                ("coded_ivf", lambda: keep.__setitem__("i", eng.bank_search_plaid_ivf(F, q, k, **kw)))]
        fns = dict(legs)
        for _, fn in legs:
            fn()
        torch.cuda.synchronize()
        cert = keep["f"]["certified"].bool()
        assert torch.equal(keep["f"]["indices"][cert], keep["e"]["indices"][cert]) and torch.equal(keep["f"]["scores"][cert], keep["e"]["scores"][cert]), \
            "a certified query's result is the exhaustive search's"
        e_idx = keep["e"]["indices"].tolist()

        def overlap(r):
            idx = r["indices"].tolist()
            cnt = r["counts"].tolist() if "counts" in r else [k] * nq
            o = [len(set(e_idx[i]) & set(idx[i][:cnt[i]])) / k for i in range(nq)]
            return dict(min=round(min(o), 4), mean=round(sum(o) / nq, 4))

        per = {key: [] for key, _ in legs}
        for _ in range(args.rounds):
            for key, x in zip(per, wall_ms([fn for _, fn in legs], args.iters, args.warmup)):
                per[key].append(round(statistics.median(x), 4))
        mid = {key: round(statistics.median(v), 4) for key, v in per.items()}
        eng.set_profiling(True)
        stage = stage_table(eng, b"f16_stop_after", F16_STAGES, fns["f16"])
        t = []
        for _ in range(5):
            eng.get_profile(reset=True)
            fns["exhaustive"]()
            t.append(eng.get_profile(reset=True)["tail"]["ms"])
        eng.set_profiling(False)
        print(f"  n_queries {nq} done", file=sys.stderr, flush=True)
        res["configs"][f"nq{nq}"] = dict(
            ms_per_call=mid, round_medians_ms=per, f16_stage_device_ms=stage, exhaustive_device_ms=round(statistics.median(t), 4),
            default_slack=round(slack, 6), certified_share=round(float(cert.float().mean()), 4),
            f16_over_exhaustive=round(mid["f16"] / mid["exhaustive"], 4),
            overlap_at_k={key: overlap(keep[s]) for key, s in (("f16", "f"), ("coded_pruned", "p"), ("coded_ivf", "i"))})
    F.close()
    return res


if __name__ == "__main__":
    main()
