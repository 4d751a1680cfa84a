#!/usr/bin/env python3
"""An fp16 passage bank with a centroid table (rr_bank_set_centroids) under the pruned searches, against the exhaustive search over
the same rows and against a compressed bank of the same centroids, in one process.

Bank: `--passages` passages (100 000 and 800 000, one size after the other; the larger bank has shorter passages so that both hold
about 12.2 M rows) at the handle's li_dim (128), WITH cluster structure: a passage draws `--topics` centroids (8) of `--centroids`
(16 384) and its rows are unit vectors near them.  The same padded tensors, made on the device chunk by chunk, fill three banks:
  F  an fp16 bank with the centroid table (rr_bank_add assigns the codes),
  P  a compressed bank, nbits 8, of the same table (rr_bank_add_compress),
  N  a plain fp16 bank.
The fill is timed per chunk on F and on N (rr_bank_add with and without a table, each with the synchronisation behind it), and
rr_bank_set_centroids over the full bank afterwards (it assigns every row again).
Queries: Lq 32, near stored passages; n_queries 1 and 16; PlaidSearch.defaults(k = 100).
Equal bits first: the exhaustive search on F is N's; the inverted-file search equals the scan form on F and on P; F and P keep the
same stage-2 survivors (the tap of the scan form).  Then the legs take turns (exhaustive on N, pruned and IVF on F, pruned and IVF
on P), `--iters` calls each, `--rounds` times, the median of the round medians is reported, wall-clock with the synchronisation.
Device ms per stage through rr_set_tuning("plaid_stop_after" / "plaid_ivf_stop_after"), by difference.  Recall: the overlap of
the pruned result on F with the exhaustive top k on the fp16 rows.
One JSON line to stdout and to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_bank_search_plaid import DEFAULT_ROWS, IVF_STAGES, STAGES, stage_table, wall_ms  # noqa: E402

CHUNK = 2048                                                # passages per add


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passages", type=int, nargs="+", default=[100000, 800000])
    ap.add_argument("--Lq", type=int, default=32)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--centroids", type=int, default=16384)
    ap.add_argument("--topics", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/bank_search_coded_bench.json.log")
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


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def same_bytes(a, b):
    import torch
    return all(torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)) for key in a if key in b)


def run_bank(args, eng, D, P):
    import torch
    import rmr_amd
    dev = eng.device
    Lq, k, C = args.Lq, args.k, args.centroids
    scale = min(1.0, DEFAULT_ROWS / (P * 122.0))           # a larger bank: shorter passages, the same rows
    Lmin, Lc = max(1, int(64 * scale)), max(1, int(180 * scale))
    g = torch.Generator().manual_seed(2025)
    clen = torch.randint(Lmin, Lc + 1, (P,), generator=g)
    lens, rows = clen.tolist(), int(clen.sum())
    cen = torch.nn.functional.normalize(torch.randn(C, D, generator=g), dim=-1).half()
    codec = rmr_amd.PlaidCodec(cen, torch.linspace(-0.1, 0.1, 256), 8, bucket_cutoffs=torch.linspace(-0.1, 0.1, 255) + 2.0 ** -26)
    topics = torch.randint(0, C, (P, args.topics), generator=g).to(dev)
    cen_d = cen.float().to(dev)
    F = eng.create_bank(rows, P, centroids=cen)
    Pb = eng.create_bank(rows, P, codec=codec)
    N = eng.create_bank(rows, P)
    dg = torch.Generator(device=dev).manual_seed(7)
    add_ms = dict(with_table=[], without=[], compress=[])
    keep_chunk = None
    for c0 in range(0, P, CHUNK):
        n = min(CHUNK, P - c0)
        pick = topics[c0:c0 + n].gather(1, torch.randint(0, args.topics, (n, Lc), generator=dg, device=dev))
        x = torch.nn.functional.normalize(cen_d[pick] + 0.5 * torch.randn(n, Lc, D, generator=dg, device=dev) / D ** 0.5, dim=-1).half()
        ln = lens[c0:c0 + n]
        m = (torch.arange(Lc, device=dev)[None, :] < clen[c0:c0 + n].to(dev)[:, None]).float()
        ids = list(range(c0, c0 + n))
        # N and F take turns at being first, so that neither always pays for the chunk's first touch
        order = (("without", N.add), ("with_table", F.add)) if (c0 // CHUNK) % 2 == 0 else (("with_table", F.add), ("without", N.add))
        for key, add in order:
            add_ms[key].append(timed(lambda: add(ids, x, m, lengths=ln)))
        add_ms["compress"].append(timed(lambda: Pb.add_compress(ids, x, m, lengths=ln)))
        if c0 == 0:
            keep_chunk = (x[:4].float().cpu(), ln[:4])
    print(f"banks: {P} passages, {rows} rows", file=sys.stderr, flush=True)
    full = slice(1, -1) if len(add_ms["without"]) > 2 else slice(None)      # the first chunk grows the scratch, the last is short
    res = dict(passages=P, passage_rows=rows, lengths=[Lmin, Lc], D=D, Lq=Lq, k=k, centroids=C, topics=args.topics, chunk_passages=CHUNK,
               add_ms_per_chunk={key: round(statistics.median(v[full]), 3) for key, v in add_ms.items()}, configs={})
    res["add_with_table_over_without"] = round(res["add_ms_per_chunk"]["with_table"] / res["add_ms_per_chunk"]["without"], 3)
    t = [timed(lambda: F.set_centroids(cen)) for _ in range(3)]
    res["set_centroids_ms"] = dict(median=round(statistics.median(t), 2), runs=[round(v, 2) for v in t])
    res["bytes_per_row"] = dict(coded=F.format()["bytes_per_row"], compressed=Pb.format()["bytes_per_row"], plain=N.format()["bytes_per_row"])
    t = [timed(F.build_ivf) for _ in range(3)]
    Pb.build_ivf()
    res["ivf"] = dict(build_ms=round(statistics.median(t), 3), **F.ivf_info())
    assert F.ivf_info() == Pb.ivf_info()
    plaid = rmr_amd.PlaidSearch.defaults(k)
    kw = dict(ncells=plaid.ncells, centroid_score_threshold=plaid.centroid_score_threshold, ndocs=plaid.ndocs)
    res["plaid"] = dict(kw)
    for nq in args.queries:
        qs, targets = [], torch.randint(0, P, (nq,), generator=g).tolist()
        for t_ in targets:                                 # a query near passage t: Lq of its rows plus noise
            rws, _ = F.read(t_)
            near = rws.float()[torch.randint(0, lens[t_], (Lq,), generator=g)]
            qs.append(torch.nn.functional.normalize(near + 0.3 * torch.randn(Lq, D, generator=g) / D ** 0.5, dim=-1))
        q = torch.stack(qs).to(dev)
        keep = {}
        legs = [("exhaustive", lambda: keep.__setitem__("e", eng.bank_search(N, q, k))),
                ("coded_pruned", lambda: keep.__setitem__("fp", eng.bank_search_plaid(F, q, k, **kw))),
                ("coded_ivf", lambda: keep.__setitem__("fi", eng.bank_search_plaid_ivf(F, q, k, **kw))),
                ("nbits8_pruned", lambda: keep.__setitem__("pp", eng.bank_search_plaid(Pb, q, k, **kw))),
                ("nbits8_ivf", lambda: keep.__setitem__("pi", eng.bank_search_plaid_ivf(Pb, q, k, **kw)))]
        fns = dict(legs)
        # equal bits first
        for _, fn in legs:
            fn()
        torch.cuda.synchronize()
        assert same_bytes(eng.bank_search(F, q, k), keep["e"]), "the exhaustive search on the coded bank is the plain bank's"
        assert same_bytes(keep["fi"], keep["fp"]) and same_bytes(keep["pi"], keep["pp"]), "the inverted file gives the scan's bytes"
        fns["nbits8_pruned"]()
        torch.cuda.synchronize()
        l2p = eng.bank_search_plaid_tap("list2")
        fns["coded_pruned"]()
        torch.cuda.synchronize()
        l2f = eng.bank_search_plaid_tap("list2")
        assert (l2p == l2f).all(), "both banks keep the same stage-2 survivors"
        cand = (torch.from_numpy(eng.bank_search_plaid_tap("a1")).view(nq, P) != float("-inf")).sum(1).tolist()
        e_idx, p_idx, counts = keep["e"]["indices"].tolist(), keep["fp"]["indices"].tolist(), keep["fp"]["counts"].tolist()
        recall = [len(set(e_idx[i]) & set(p_idx[i][:counts[i]])) / k for i in range(nq)]
        per = {key: [] for key, _ in legs}
        for _ in range(args.rounds):
            for key, x in zip(per, wall_ms([fn for _, fn in legs], args.iters, args.warmup)):
                per[key].append(round(statistics.median(x), 4))
        mid = {key: round(statistics.median(v), 4) for key, v in per.items()}
        eng.set_profiling(True)
        stage = dict(coded_pruned=stage_table(eng, b"plaid_stop_after", STAGES, fns["coded_pruned"]),
                     coded_ivf=stage_table(eng, b"plaid_ivf_stop_after", IVF_STAGES, fns["coded_ivf"]),
                     nbits8_pruned=stage_table(eng, b"plaid_stop_after", STAGES, fns["nbits8_pruned"]),
                     nbits8_ivf=stage_table(eng, b"plaid_ivf_stop_after", IVF_STAGES, fns["nbits8_ivf"]))
        eng.set_profiling(False)
        print(f"  n_queries {nq} done", file=sys.stderr, flush=True)
        res["configs"][f"nq{nq}"] = dict(
            ms_per_call=mid, round_medians_ms=per, stage_ms=stage,
            coded_ivf_over_exhaustive=round(mid["coded_ivf"] / mid["exhaustive"], 4),
            coded_pruned_over_exhaustive=round(mid["coded_pruned"] / mid["exhaustive"], 4),
            coded_ivf_over_nbits8_ivf=round(mid["coded_ivf"] / mid["nbits8_ivf"], 4),
            stage3_fp16_over_nbits8=dict(scan=round(stage["coded_pruned"]["exact_list"] / stage["nbits8_pruned"]["exact_list"], 4),
                                         ivf=round(stage["coded_ivf"]["exact_list"] / stage["nbits8_ivf"]["exact_list"], 4)),
            candidates_per_query=dict(min=min(cand), mean=round(sum(cand) / nq, 1), max=max(cand)),
            returned_per_query=dict(min=min(counts), max=max(counts)),
            recall_at_k=dict(min=round(min(recall), 4), mean=round(sum(recall) / nq, 4)))
    # the codes of the first passages (assigned by the adds, then again by set_centroids) against the host definition
    x64, ln64 = keep_chunk                                  # (four passages: the host definition walks every centroid per row)
    want = torch.cat([codec.compress(x64[i, :l])[0] for i, l in enumerate(ln64)])
    got = torch.cat([F.codes(i) for i in range(len(ln64))])
    res["codes_equal_host_definition_rows"] = int(want.numel()) if torch.equal(want, got) else -1
    for b in (F, Pb, N):
        b.close()
    return res


if __name__ == "__main__":
    main()
