#!/usr/bin/env python3
"""Training a PLAID codec's centroids on the device: rr_plaid_kmeans (THE TRAINED CENTROIDS, include/rerank_mi355.h) against the same
Lloyd iteration composed from torch, in the same process, on the same device tensor.

Shape: `--rows` rows (262 144) of li_dim 128 around `--centroids` directions (4 096), handed over as fp16, `--niters` iterations (4),
the first `--centroids` rows as the initial table.

  kmeans     one rr_plaid_kmeans call between two events.  Per iteration: (the call at niters - the call at 0 iterations) / niters,
             so the staging of the initial rows, its synchronisation, the initial table and the normalisation cancel.  The same with
             rr_set_tuning("kmeans_stop_after") = 0 (assignment alone) and 1 (assignment + accumulation) gives the three kernels of
             an iteration by difference.
  composed   per iteration: float32 `rows @ table.T` in chunks of (1 << 29) // centroids rows plus the bias, `argmax`, `index_add_`
             of the float32 rows and of ones, the division; empty clusters keep their row.

Reported: ms per iteration of both, the three device times, the assignment's TFLOP/s (2 * rows * centroids * li_dim) beside the
101.9 bank_compress.hip reports for the same kernel without bias, the 64-bit atomic byte rate of the accumulation (rows * li_dim * 8
bytes added / its time; it also reads the rows and the keys), the share of accumulation + update in an iteration, and how many of
the rows the two paths assign alike after the last iteration (they round differently).  No threshold.  One JSON line to stdout and
to --out."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--centroids", type=int, default=4096)
    ap.add_argument("--niters", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="profiles/plaid_train_bench.json.log")
    args = ap.parse_args()

    import torch
    import rmr_amd
    from rmr_amd import _lib as L

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    R, Cn, niters = args.rows, args.centroids, args.niters
    arch = rmr_amd.make_arch(dict(cross_encoder_num_hidden_layers=3, cross_encoder_max_position_embeddings=750, loss_fn="BCE",
                                  pos_weight=None), model_kind="interaction", has_vision=0)
    D = arch["li_dim"]
    eng = rmr_amd.RerankEngine(arch, dev)                  # a handle is all the calls need (no weights)
    lib = eng.lib
    g = torch.Generator(device=dev).manual_seed(2026)
    planted = torch.nn.functional.normalize(torch.randn(Cn, D, generator=g, device=dev), dim=-1)
    pick = torch.randint(0, Cn, (R,), generator=g, device=dev)
    rows = torch.nn.functional.normalize(planted[pick] + 0.35 * torch.randn(R, D, generator=g, device=dev) / D ** 0.5, dim=-1).half()
    init = torch.arange(Cn, dtype=torch.int32)
    cen = torch.empty((Cn, D), dtype=torch.float16, device=dev)
    counts = torch.empty(Cn, dtype=torch.int32, device=dev)
    stats = torch.zeros((max(niters, 1), 2), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def kmeans(n):
        L.check(lib.rr_plaid_kmeans(eng.h, L.ptr(rows), L.RR_F16, R, init.data_ptr(), Cn, n, 123, L.ptr(cen), L.ptr(counts), L.ptr(stats),
                                    st), eng.h, "rr_plaid_kmeans")

    rows32 = rows.float()
    ones = torch.ones(R, device=dev)
    state = {}

    def composed(n):
        t = rows32[:Cn].clone()
        for _ in range(n):
            h = -0.5 * (t * t).sum(1)
            code = torch.cat([(b @ t.T + h).argmax(1) for b in rows32.split((1 << 29) // Cn)])
            s = torch.zeros_like(t).index_add_(0, code, rows32)
            cnt = torch.zeros(Cn, device=dev).index_add_(0, code, ones)
            t = torch.where(cnt[:, None] > 0, s / cnt.clamp(min=1)[:, None], t)
            state["code"] = code
        state["table"] = t

    def device_ms(fn):
        t = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            t.append(a.elapsed_time(b))
        return statistics.median(t)

    def per_iter(fn):
        fn(niters)                                         # warm-up: scratch grown, kernels loaded
        return (device_ms(lambda: fn(niters)) - device_ms(lambda: fn(0))) / niters

    stage = {}
    try:
        for stop in (0, 1, 2):
            L.check(lib.rr_set_tuning(b"kmeans_stop_after", stop), None, "rr_set_tuning")
            stage[stop] = per_iter(kmeans)
    finally:
        L.check(lib.rr_set_tuning(b"kmeans_stop_after", 2), None, "rr_set_tuning")
    kmeans(niters)
    torch.cuda.synchronize()
    moved = stats[:niters, 0].tolist()
    reseeded = stats[:niters, 1].tolist()
    composed_ms = per_iter(composed)
    composed(niters)                                       # the timing's last call ran 0 iterations
    # rows the two finished tables assign alike
    c16 = cen.float()
    mine = torch.cat([(b @ c16.T).argmax(1) for b in rows32.split((1 << 29) // Cn)])
    tn = torch.nn.functional.normalize(state["table"], dim=-1)
    theirs = torch.cat([(b @ tn.T).argmax(1) for b in rows32.split((1 << 29) // Cn)])
    mse = lambda table, code: float(((rows32 - table[code]) ** 2).sum(1).mean())      # noqa: E731
    assign, accumulate, update = stage[0], stage[1] - stage[0], stage[2] - stage[1]
    res = dict(device=torch.cuda.get_device_name(0), rows=R, D=D, centroids=Cn, niters=niters, repeats=args.repeats,
               kmeans_ms_per_iter=round(stage[2], 4), composed_ms_per_iter=round(composed_ms, 4),
               kmeans_over_composed=round(stage[2] / composed_ms, 4), assign_ms=round(assign, 4), accumulate_ms=round(accumulate, 4),
               update_ms=round(update, 4), assign_tflops=round(2.0 * R * Cn * D / (assign * 1e-3) / 1e12, 2),
               compress_assign_tflops_reported=101.9, f32_matrix_core_tflops=155,
               atomic64_bytes=R * D * 8, atomic64_gb_per_s=round(R * D * 8 / (accumulate * 1e-3) / 1e9, 2),
               accumulate_plus_update_share=round((accumulate + update) / stage[2], 4), rows_moved=moved, clusters_reseeded=reseeded,
               rows_assigned_alike=int((mine == theirs).sum()), mse_kmeans=round(mse(c16, mine), 6),
               mse_composed=round(mse(tn, theirs), 6))
    line = json.dumps(res)
    out = args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
