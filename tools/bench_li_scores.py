#!/usr/bin/env python3
"""The late-interaction score operator and the from-li attention fusion on an MI355X.

    python tools/bench_li_scores.py [--queries 8 --K 100 --Lq 113 --Lc 512 --iters 64 --warmup 16 --compute-dtype fp16]

One process, HIP events around every call, warm-up / iteration counts as tools/bench_strings_to_records.py uses them (16 / 64):
  (a) RerankEngine.li_scores alone at [Bq x K pairs, Lq, Lc, D = li_dim]: scores + maxsim, and maxsim only; GB/s of the first
      from the algorithmic traffic (context_li and query_li read once, the score block written once);
  (b) InteractionRerankModel NORMAL on the int_base geometry (3 cross-encoder layers), unit-norm retriever embeddings with
      context lengths U[64, Lc]: forward_interaction(fusion_from_li=True) against forward_interaction(preflmr_scores = the
      resident tensor li_scores produced), alternating, after rr_reserve(with_fusion = 2); both give the same logits.  With
      --profile the per-class device time of one forward of each form (rr_get_profile) is added.
Prints ONE JSON line (median and mean ms per call)."""
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


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 4), mean_ms=round(statistics.fmean(ms), 4), min_ms=round(min(ms), 4),
                max_ms=round(max(ms), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=8)
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--Lq", type=int, default=113)
    ap.add_argument("--Lc", type=int, default=512)
    ap.add_argument("--iters", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--compute-dtype", default="fp16", choices=["bf16", "fp16"])
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()

    import torch
    import rmr_amd

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    Bq, K, Lq, Lc = args.queries, args.K, args.Lq, args.Lc
    N = Bq * K
    arch = rmr_amd.make_arch(dict(cross_encoder_num_hidden_layers=3, cross_encoder_max_position_embeddings=750, loss_fn="BCE",
                                  pos_weight=None, compute_dtype=args.compute_dtype), model_kind="interaction", has_vision=0)
    D = arch["li_dim"]
    eng = rmr_amd.RerankEngine(arch, dev)
    eng.load_state_dict(rmr_amd.synthetic_state_dict(arch, seed=0))
    g = torch.Generator().manual_seed(2022)
    q = torch.nn.functional.normalize(torch.randn(Bq, Lq, D, generator=g), dim=-1).to(dev)
    c = torch.nn.functional.normalize(torch.randn(N, Lc, D, generator=g), dim=-1).to(dev)
    clen = torch.randint(64, Lc + 1, (N,), generator=g)
    cm = (torch.arange(Lc)[None, :] < clen[:, None]).float().to(dev)
    qm = torch.ones(Bq, Lq, device=dev)
    res = dict(device=torch.cuda.get_device_name(0), Bq=Bq, K=K, Lq=Lq, Lc=Lc, D=D, iters=args.iters, warmup=args.warmup,
               compute_dtype=args.compute_dtype)

    # (a) the operator alone
    both, only = event_ms([lambda: eng.li_scores(q, c, cm, Bq, K), lambda: eng.li_scores(q, c, cm, Bq, K, want_scores=False)],
                          args.iters, args.warmup)
    traffic = 4.0 * (N * Lc * D + Bq * Lq * D + N * Lc * Lq + N * Lc + N)
    res["li_scores"] = dict(scores_and_maxsim=stats(both), maxsim_only=stats(only), bytes=traffic,
                            gb_per_s=round(traffic / (statistics.median(both) * 1e-3) / 1e9, 1),
                            gflop=round(2.0 * N * Lc * Lq * D / 1e9, 3),
                            tflops=round(2.0 * N * Lc * Lq * D / (statistics.median(both) * 1e-3) / 1e12, 2))

    # (b) the forward: scores from the call's own tensors against a resident score tensor
    eng.reserve(N, Bq, Lq, Lc, with_fusion=2)
    resident = eng.li_scores(q, c, cm, Bq, K, want_maxsim=False)["scores"]
    kw = dict(want_scores=True, want_order=True, fusion_multiplier=1.0)
    explicit = lambda: eng.forward_interaction(q, c, qm, cm, Bq, K, preflmr_scores=resident, **kw)      # noqa: E731
    from_li = lambda: eng.forward_interaction(q, c, qm, cm, Bq, K, fusion_from_li=True, **kw)          # noqa: E731
    same = torch.equal(explicit()["logits"], from_li()["logits"])
    ex_ms, li_ms = event_ms([explicit, from_li], args.iters, args.warmup)
    res["forward_interaction"] = dict(explicit_scores=stats(ex_ms), fusion_from_li=stats(li_ms), logits_identical=bool(same),
                                      from_li_over_explicit=round(statistics.median(li_ms) / statistics.median(ex_ms), 4))
    if args.profile:
        eng.set_profiling(True)
        for name, fn in (("explicit_scores", explicit), ("fusion_from_li", from_li)):
            eng.get_profile(reset=True)
            fn()
            p = eng.get_profile(reset=True)
            res["forward_interaction"][name]["profile_ms"] = {k: round(v["ms"], 4) for k, v in p.items() if v["launches"]}
        eng.set_profiling(False)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
