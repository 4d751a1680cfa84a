#!/usr/bin/env python3
"""The exhaustive search of a COMPRESSED bank whose first pass runs on the fp16 matrix core (rr_bank_search_f16_plaid) against the
exact exhaustive search of the same bank (rr_bank_search: the only exact search such a bank had), the two pruned searches, and a
yardstick built from parts that exist, in one process.

Banks: the two banks of tools/bench_bank_search_f16.py's record in the compressed format of tools/bench_bank_search_plaid.py, one
after the other: 100 000 passages of 64 .. 180 rows and 800 000 passages of 8 .. 22 rows (about 12.2 M rows each, D 128, nbits 8, rows
near 8 of 16 384 centroids per passage).  Queries: Lq 32, near stored passages; n_queries 1, 16 and 64; ndocs 1024, k 100;
PlaidSearch.defaults(k) for the pruned legs.
Legs, taking turns in one process, `--iters` calls each behind `--warmup` unmeasured rounds, `--rounds` times (reported: the median
of the round medians and the round medians, wall-clock ms per call with the synchronisation):
  exhaustive      rr_bank_search on the compressed bank (every row decoded once per query);
  f16_plaid       rr_bank_search_f16_plaid (every row decoded once per query block);
  pruned, ivf     rr_bank_search_plaid and rr_bank_search_plaid_ivf;
  decode_then_f16 THE YARDSTICK: rr_op_plaid_decode_rows of every row of the bank into a scratch buffer, then rr_bank_search_f16 on
                  the fp16 bank that holds the decoded rows: what a decode-once-per-CALL design would cost (its first pass reads
                  the buffer the decode wrote: 2 D bytes per row written and read again, against D + 5 read per query block).
Device ms per stage of the f16_plaid call through rr_set_tuning("f16_stop_after"), by difference of the profile's tail class.
certified_share: the queries the call certifies at the default slack; overlap_at_k: the share of the exhaustive top k each other
leg returns.  Before any timing, a certified query's result must be the exhaustive call's bytes, and the whole f16_plaid result the
yardstick's bytes (asserted).  `bar`: whether f16_plaid lies below exhaustive by more than the spread of the round medians of either leg.
One JSON line to stdout and to --out."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_bank_search_f16 import CHUNK, F16_STAGES  # noqa: E402
from bench_bank_search_plaid import DEFAULT_ROWS, stage_table, wall_ms  # noqa: E402


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
    ap.add_argument("--out", default="profiles/bank_search_f16_plaid_bench.json.log")
    args = ap.parse_args()

    import torch
    import rmr_amd

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    arch = rmr_amd.make_arch(dict(cross_encoder_num_hidden_layers=3, cross_encoder_max_position_embeddings=750, loss_fn="BCE",
                                  pos_weight=None), model_kind="interaction", has_vision=0)
    eng = rmr_amd.RerankEngine(arch, dev)                  # a handle is all the calls need (no weights)
    banks = [run_bank(args, eng, arch["li_dim"], P) for P in args.passages]
    line = json.dumps(dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, rounds=args.rounds, banks=banks))
    out = args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    print(line)


def run_bank(args, eng, D, P):
    import torch
    import rmr_amd
    from rmr_amd import _lib as L
    dev = eng.device
    Lq, k, nbits, C, ndocs = args.Lq, args.k, 8, args.centroids, args.ndocs
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
    bank.build_ivf()
    # the yardstick's parts: the compressed rows as loose device arrays, the scratch buffer of the decode, the fp16 twin
    codes_d, resid_d = codes.to(dev), resid.to(dev)
    cen_d, w_d = codec.centroids.to(dev), codec.bucket_weights.to(dev)
    scratch = torch.empty((rows, D), dtype=torch.float16, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def decode_all():
        L.check(eng.lib.rr_op_plaid_decode_rows(L.ptr(cen_d), C, L.ptr(w_d), nbits, D, L.ptr(codes_d), L.ptr(resid_d), 0, rows, L.ptr(scratch), st),
                None, "rr_op_plaid_decode_rows")

    decode_all()
    twin = eng.create_bank(rows, P)
    first_d, clen_d = first.to(dev), clen.to(dev)
    for c0 in range(0, P, CHUNK):
        n = min(CHUNK, P - c0)
        at = (first_d[c0:c0 + n, None] + torch.arange(Lc, device=dev)[None, :]).clamp_(max=rows - 1)
        m = (torch.arange(Lc, device=dev)[None, :] < clen_d[c0:c0 + n, None]).float()
        twin.add(list(range(c0, c0 + n)), scratch[at], m, lengths=lens[c0:c0 + n])
    print(f"bank: {P} passages, {rows} rows", file=sys.stderr, flush=True)
    plaid = rmr_amd.PlaidSearch.defaults(k)
    kw = dict(ncells=plaid.ncells, centroid_score_threshold=plaid.centroid_score_threshold, ndocs=plaid.ndocs)
    res = dict(passages=P, passage_rows=rows, lengths=[Lmin, Lc], D=D, Lq=Lq, k=k, ndocs=ndocs, nbits=nbits, centroids=C, topics=args.topics,
               plaid=dict(kw), configs={})
    for nq in args.queries:
        qs, targets = [], torch.randint(0, P, (nq,), generator=g).tolist()
        for t_ in targets:                                 # a query near passage t: Lq of its decoded rows plus noise
            r = first[t_] + torch.randint(0, lens[t_], (Lq,), generator=g)
            near = codec.decode(codes[r], resid[r]).float()
            qs.append(torch.nn.functional.normalize(near + 0.3 * torch.randn(Lq, D, generator=g) / D ** 0.5, dim=-1))
        q = torch.stack(qs).to(dev)
        slack = rmr_amd.F16Search(ndocs).slack_for(q)       # once: the legs time the call, not the reduction before it
        keep = {}

        def yardstick():
            decode_all()
            keep["y"] = eng.bank_search_f16(twin, q, k, ndocs, slack=slack)

        legs = [("exhaustive", lambda: keep.__setitem__("e", eng.bank_search(bank, q, k))),
                ("f16_plaid", lambda: keep.__setitem__("f", eng.bank_search_f16_plaid(bank, q, k, ndocs, slack=slack))),
                ("pruned", lambda: keep.__setitem__("p", eng.bank_search_plaid(bank, q, k, **kw))),
                ("ivf", lambda: keep.__setitem__("i", eng.bank_search_plaid_ivf(bank, q, k, **kw))),
                ("decode_then_f16", yardstick)]
        fns = dict(legs)
        for _, fn in legs:
            fn()
        torch.cuda.synchronize()
        cert = keep["f"]["certified"].bool()
        assert torch.equal(keep["f"]["indices"][cert], keep["e"]["indices"][cert]) and torch.equal(keep["f"]["scores"][cert], keep["e"]["scores"][cert]), \
            "a certified query's result is the exhaustive search's"
        assert all(torch.equal(keep["f"][key], keep["y"][key]) for key in ("indices", "scores", "certified")), \
            "the call's result is rr_bank_search_f16's on the fp16 bank of the decoded rows"
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
        spread = {key: round(max(v) - min(v), 4) for key, v in per.items()}
        eng.set_profiling(True)
        stage = stage_table(eng, b"f16_stop_after", F16_STAGES, fns["f16_plaid"])
        t = []
        for _ in range(5):
            eng.get_profile(reset=True)
            fns["exhaustive"]()
            t.append(eng.get_profile(reset=True)["tail"]["ms"])
        eng.set_profiling(False)
        print(f"  n_queries {nq} done", file=sys.stderr, flush=True)
        gap = round(mid["exhaustive"] - mid["f16_plaid"], 4)
        res["configs"][f"nq{nq}"] = dict(
            ms_per_call=mid, round_medians_ms=per, round_median_spread_ms=spread, f16_plaid_stage_device_ms=stage,
            exhaustive_device_ms=round(statistics.median(t), 4), default_slack=round(slack, 6),
            certified_share=round(float(cert.float().mean()), 4), f16_plaid_over_exhaustive=round(mid["f16_plaid"] / mid["exhaustive"], 4),
            f16_plaid_over_decode_then_f16=round(mid["f16_plaid"] / mid["decode_then_f16"], 4),
            bar=dict(exhaustive_minus_f16_plaid_ms=gap, larger_spread_ms=max(spread["exhaustive"], spread["f16_plaid"]),
                     met=bool(gap > max(spread["exhaustive"], spread["f16_plaid"]))),
            overlap_at_k={key: overlap(keep[s]) for key, s in (("f16_plaid", "f"), ("pruned", "p"), ("ivf", "i"))})
    bank.close()
    twin.close()
    return res


if __name__ == "__main__":
    main()
