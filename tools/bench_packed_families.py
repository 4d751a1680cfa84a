#!/usr/bin/env python3
"""Padded against packed forwards of the joint and interaction reranker families on an MI355X.

    python tools/bench_packed_families.py [--steps 10 --warmup 3 --queries 8 --K 100 --granule 16 --only joint,mores]

Workloads (seeded; 8 queries x 100 candidates by default, pair lengths U[64, 512]):
  joint, joint_fusion   RerankModel (2H_BCE) on the c3 geometry: bert-base text encoder over the [query 32 | context] joint
                        sequence of S = 512, 81 vision tokens, one cross-encoder layer (RerankEngine.forward_joint against
                        forward_joint_packed); _fusion with PreFLMR attention-fusion scores [N, 512, 113].
  normal, normal_fusion InteractionRerankModel NORMAL on the int_base geometry (Lq = 113, Lc = 512, 3 cross-encoder layers;
                        forward_interaction against forward_interaction_packed); context lengths U[64, 512].
  mores                 InteractionRerankModel MORES (5 layers), the same inputs.
A step is one forward with the head (order + scores); the packed form gets the pair lengths as host data (the tokenizer / the
retriever knows them), as bench.py --packed does.  Timing: W warm-up steps, then K steps between device synchronisations.
Prints ONE JSON line: per workload ms per step of both forms, the speed-up, rows computed and segments."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--queries", type=int, default=8)
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--granule", type=int, default=16)
    ap.add_argument("--compute-dtype", default="fp16", choices=["bf16", "fp16"])
    ap.add_argument("--only", default="", help="comma-separated subset of joint,joint_fusion,normal,normal_fusion,mores")
    args = ap.parse_args()

    import torch
    import rmr_amd
    from rmr_amd.pair_inputs import pair_lengths
    from rmr_amd.synthetic import image_features, pair_batch

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    Bq, K = args.queries, args.K
    N = Bq * K
    only = set(filter(None, args.only.split(",")))
    res = {}

    def record(name, pad_ms, pk_ms, pad_out, pk_out, padded_rows):
        d = (pad_out["logits"] - pk_out["logits"]).abs().max().item()
        res[name] = dict(padded_ms=round(pad_ms, 3), packed_ms=round(pk_ms, 3), speedup=round(pad_ms / pk_ms, 3),
                         padded_rows=padded_rows, packed_rows=int(pk_out["packed_rows"]), segments=int(pk_out["packed_segments"]),
                         max_abs_dlogit=d, same_order=bool(torch.equal(pad_out["order"], pk_out["order"])))

    # ---- joint (RerankModel) on the c3 geometry
    if not only or only & {"joint", "joint_fusion"}:
        arch = rmr_amd.make_arch(dict(cross_encoder_num_hidden_layers=1, cross_encoder_max_position_embeddings=750,
                                      loss_fn="2H_BCE", pos_weight=None, compute_dtype=args.compute_dtype))
        eng = rmr_amd.RerankEngine(arch, dev)
        eng.load_state_dict(rmr_amd.synthetic_state_dict(arch, seed=0))
        S, ql = 512, 32
        P = arch["prefix_len"] + arch["n_patches"]
        ids, am, _ = pair_batch(arch["vocab_size"], Bq, K, S, seed=2022, regime="realistic", q_len=ql)
        lens = pair_lengths(ids, am).numpy()
        ids, am = ids.to(dev), am.to(dev)
        cls, pat = [t.to(dev) for t in image_features(Bq, arch["n_patches"], arch["vision_hidden"])]
        eng.reserve(N, N, S, with_fusion=True)
        for name in ("joint", "joint_fusion"):
            if only and name not in only:
                continue
            kw = dict(want_scores=True, want_order=True)
            if name == "joint_fusion":
                g = torch.Generator().manual_seed(3)
                kw.update(preflmr_scores=torch.randn(N, S, ql + P, generator=g).to(dev), fusion_multiplier=5.0)
            pad_ms, pad_out = timed(lambda: eng.forward_joint(ids, am, Bq, K, ql, cls, pat, None, **kw), args.steps, args.warmup)
            pk_ms, pk_out = timed(lambda: eng.forward_joint_packed(ids, am, Bq, K, ql, cls, pat, None, granule=args.granule,
                                                                   lengths=lens, **kw), args.steps, args.warmup)
            record(name, pad_ms, pk_ms, pad_out, pk_out, N * S)
        del eng

    # ---- interaction NORMAL / MORES on the int_base geometry
    if not only or only & {"normal", "normal_fusion", "mores"}:
        Lq, Lc, D = 113, 512, 128
        g = torch.Generator().manual_seed(2022)
        q = torch.randn(Bq, Lq, D, generator=g)
        c = torch.randn(N, Lc, D, generator=g)
        qm = torch.ones(Bq, Lq)
        qm[:, 94:] = 0
        clen = torch.randint(64, Lc + 1, (N,), generator=g)
        cm = (torch.arange(Lc)[None, :] < clen[:, None]).float()
        lens = clen.numpy()
        ps = torch.randn(N, Lc, Lq, generator=g)
        q, c, qm, cm, ps = q.to(dev), c.to(dev), qm.to(dev), cm.to(dev), ps.to(dev)
        for kind, layers, names in (("interaction", 3, ("normal", "normal_fusion")), ("mores", 5, ("mores",))):
            names = [n for n in names if not only or n in only]
            if not names:
                continue
            arch = rmr_amd.make_arch(dict(cross_encoder_num_hidden_layers=layers, cross_encoder_max_position_embeddings=750,
                                          loss_fn="BCE", pos_weight=None, compute_dtype=args.compute_dtype),
                                     model_kind=kind, has_vision=0)
            eng = rmr_amd.RerankEngine(arch, dev)
            eng.load_state_dict(rmr_amd.synthetic_state_dict(arch, seed=0))
            eng.reserve(N, N, Lq, Lc, with_fusion=kind == "interaction")
            for name in names:
                kw = dict(want_scores=True, want_order=True)
                if name == "normal_fusion":
                    kw.update(preflmr_scores=ps, fusion_multiplier=5.0)
                pad_ms, pad_out = timed(lambda: eng.forward_interaction(q, c, qm, cm, Bq, K, **kw), args.steps, args.warmup)
                pk_ms, pk_out = timed(lambda: eng.forward_interaction_packed(q, c, qm, cm, Bq, K, granule=args.granule,
                                                                             lengths=lens, **kw), args.steps, args.warmup)
                record(name, pad_ms, pk_ms, pad_out, pk_out, N * Lc)
            del eng

    print(json.dumps({"bench": "packed_families", "pairs": N, "lengths": "U[64, 512]", "granule": args.granule,
                      "compute_dtype": args.compute_dtype, "steps": args.steps, "warmup": args.warmup,
                      "device": torch.cuda.get_device_name(dev), "results": res}))


if __name__ == "__main__":
    main()
