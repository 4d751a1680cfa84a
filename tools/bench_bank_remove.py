#!/usr/bin/env python3
"""Removing passages from a bank in place (rr_bank_remove, PassageBank.remove) against what the library offered before:
clear(), add the survivors again from tensors that are resident on the device, build_ivf().

Bank: `--passages` passages (100 000) of U[64, 512] rows at the handle's li_dim 128; once as fp16 rows, once compressed at nbits 8
(`--centroids` centroids, compressed on the device by add_compress) with an inverted file.  The padded source tensors
[passages, 512, 128] fp16 stay on the device for the whole run, and the survivors of a pattern are gathered into their add
batches (`--batch` passages) BEFORE anything is timed: leg (b) pays the library's work alone.

Patterns: 1 % and 10 % of the passages at random, the oldest 10 % (a front block: every survivor moves), the newest 10 % (nothing
moves).  Per pattern the legs take turns in one process, after `--warmup` untimed turns, `--iters` times:
  fill (untimed): clear(), add everything, build_ivf() on the compressed bank
  (r) PassageBank.remove(ids): host clock around the call, which synchronises; `lib_ms` is the rr_bank_remove call inside it
  (b) clear(), add the survivors batch by batch, build_ivf() on the compressed bank, torch.cuda.synchronize()
Reported per pattern: the medians of both legs and their ratio; the bytes the plan moves (moved rows times the bytes of a row over
all arrays of the bank, from the shapes); `move_GBps`: the traffic of the move (every moved byte is read and written twice: into
the staging block and out of it) over lib_ms less the inverted file's rebuild, beside the HBM rates of MI355X_MICROARCH.md; and
`ivf_share`: a build_ivf over the survivors, timed on its own behind (r), over lib_ms.
Then the staging block: `bank_move_kb` at 16, 64 and 256 MiB on the oldest-10 % pattern of the fp16 bank, `--sweep-iters` removals
each in turn, the spread (max - min over the median) of the repeated legs, and `default_MiB_by_rule`: the smallest block whose
median lies inside the range the repeats of the largest cover, which is how the shipped default is chosen.
One JSON line to stdout and to --out.  Needs an MI355X: without a device it fails."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_TBPS, HBM_MEASURED_TBPS = 8.0, 6.29          # MI355X_MICROARCH.md: spec; measured float4 copy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passages", type=int, default=100000)
    ap.add_argument("--centroids", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=10000)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sweep-iters", type=int, default=9)
    ap.add_argument("--kinds", default="fp16,plaid8")
    ap.add_argument("--out", default="profiles/bank_remove_bench.json.log")
    args = ap.parse_args()

    import numpy as np
    import torch
    import rmr_amd

    if not torch.cuda.is_available():
        raise SystemExit("bench_bank_remove: no GPU (the figures are not measured without an MI355X)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    arch = rmr_amd.make_arch(dict(cross_encoder_num_hidden_layers=3, cross_encoder_max_position_embeddings=750, loss_fn="BCE",
                                  pos_weight=None), model_kind="interaction", has_vision=0)
    D, P, Lc = arch["li_dim"], args.passages, 512
    eng = rmr_amd.RerankEngine(arch, dev)                  # a handle is all the calls need (no weights)
    g = torch.Generator().manual_seed(2026)
    clen = torch.randint(64, Lc + 1, (P,), generator=g)
    lens = clen.tolist()
    rows = int(clen.sum())
    first = np.concatenate([[0], np.cumsum(lens)])
    gd = torch.Generator(device=dev).manual_seed(7)
    src = torch.randn(P, Lc, D, device=dev, dtype=torch.float16, generator=gd) * (1.0 / D ** 0.5)
    ones = torch.ones(args.batch, Lc, device=dev)
    print(f"bank: {P} passages, {rows} rows", file=sys.stderr, flush=True)
    res = dict(device=torch.cuda.get_device_name(0), passages=P, rows=rows, D=D, lengths="U[64, 512]", batch=args.batch, iters=args.iters,
               warmup=args.warmup, hbm_peak_TBps=HBM_PEAK_TBPS, hbm_measured_copy_TBps=HBM_MEASURED_TBPS,
               bank_move_kb_default=262144, kinds={})
    rng = np.random.default_rng(5)
    patterns = {"random_1pct": np.sort(rng.choice(P, P // 100, replace=False)), "random_10pct": np.sort(rng.choice(P, P // 10, replace=False)),
                "oldest_10pct": np.arange(P // 10), "newest_10pct": np.arange(P - P // 10, P)}

    def make_bank(kind):
        if kind == "fp16":
            return eng.create_bank(rows, P), 2 * D + 1
        nbits = 8
        codec = rmr_amd.PlaidCodec(torch.nn.functional.normalize(torch.randn(args.centroids, D, generator=g), dim=-1),
                                   torch.randn(1 << nbits, generator=g) * (0.25 / D ** 0.5), nbits,
                                   bucket_cutoffs=torch.linspace(-0.25, 0.25, (1 << nbits) - 1))
        return eng.create_bank(rows, P, codec=codec), codec.residual_bytes + 4 + 1

    def add(bank, ids, li, ln):
        (bank.add_compress if bank.codec is not None else bank.add)(ids, li, ones[:len(ids)], lengths=ln)

    def fill(bank):
        bank.clear()
        for f in range(0, P, args.batch):
            e = min(P, f + args.batch)
            add(bank, list(range(f, e)), src[f:e], lens[f:e])
        if bank.codec is not None:
            bank.build_ivf()
        torch.cuda.synchronize()

    def timed_remove(bank, ids):
        """(ms of PassageBank.remove, ms of the rr_bank_remove call inside it)"""
        inner = []
        real = bank.lib.rr_bank_remove

        class Timed:
            def __getattr__(self, name):
                return getattr(bank_lib, name)

            def rr_bank_remove(self, *a):
                t = time.perf_counter()
                rc = real(*a)
                inner.append((time.perf_counter() - t) * 1e3)
                return rc
        bank_lib = bank.lib
        bank.lib = Timed()
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bank.remove(ids)
            ms = (time.perf_counter() - t0) * 1e3
        finally:
            bank.lib = bank_lib
        return ms, inner[0]

    def moved_bytes(gone, bytes_per_row):
        g0 = int(gone.min())
        kept_behind = rows - int(first[g0]) - int(sum(lens[p] for p in gone.tolist()))
        return kept_behind * bytes_per_row

    out_path = args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    for kind in args.kinds.split(","):
        bank, bpr = make_bank(kind)
        out = {}
        for name, gone in patterns.items():
            keep = np.setdiff1d(np.arange(P), gone)
            batches = []                                    # the survivors' add batches, resident before anything is timed
            for f in range(0, len(keep), args.batch):
                idx = keep[f:f + args.batch]
                batches.append((idx.tolist(), src[torch.from_numpy(idx).to(dev)], [lens[p] for p in idx.tolist()]))
            torch.cuda.synchronize()

            def rebuild():
                bank.clear()
                for ids, li, ln in batches:
                    add(bank, ids, li, ln)
                if bank.codec is not None:
                    bank.build_ivf()
                torch.cuda.synchronize()
            t = dict(r=[], lib=[], b=[], ivf=[])
            for it in range(args.warmup + args.iters):
                fill(bank)
                r_ms, lib_ms = timed_remove(bank, gone.tolist())
                ivf_ms = 0.0
                if bank.codec is not None:
                    t0 = time.perf_counter()
                    bank.build_ivf()
                    ivf_ms = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                rebuild()
                b_ms = (time.perf_counter() - t0) * 1e3
                if it >= args.warmup:
                    t["r"].append(round(r_ms, 3)), t["lib"].append(round(lib_ms, 3)), t["b"].append(round(b_ms, 3)), t["ivf"].append(round(ivf_ms, 3))
            med = {k: statistics.median(v) for k, v in t.items()}
            nbytes = moved_bytes(gone, bpr)
            move_ms = max(med["lib"] - med["ivf"], 1e-6)
            out[name] = dict(removed=len(gone), remove_ms=med["r"], remove_lib_ms=med["lib"], readd_ms=med["b"],
                             readd_over_remove=round(med["b"] / med["r"], 2), bytes_moved=nbytes, move_ms=round(move_ms, 3),
                             move_GBps=round(4 * nbytes / move_ms / 1e6, 1) if nbytes else None,
                             move_share_of_hbm_peak=round(4 * nbytes / move_ms / 1e9 / HBM_PEAK_TBPS, 3) if nbytes else None,
                             ivf_rebuild_ms=med["ivf"], ivf_share=round(med["ivf"] / med["lib"], 3), turns=t)
            del batches
            print(f"  {kind} {name}: remove {med['r']:.1f} ms, re-add {med['b']:.1f} ms", file=sys.stderr, flush=True)
        res["kinds"][kind] = dict(bytes_per_row=bpr, patterns=out)
        if kind == "fp16":                                  # the staging block, on the pattern that moves everything
            gone = patterns["oldest_10pct"].tolist()
            sweep = {16: [], 64: [], 256: []}
            try:
                for it in range(1 + args.sweep_iters):
                    for mib in sweep:
                        fill(bank)
                        assert eng.lib.rr_set_tuning(b"bank_move_kb", mib * 1024) == 0
                        ms = timed_remove(bank, gone)[1]
                        if it:
                            sweep[mib].append(round(ms, 3))
            finally:
                assert eng.lib.rr_set_tuning(b"bank_move_kb", 262144) == 0
            med = {m: statistics.median(v) for m, v in sweep.items()}
            res["bank_move_kb_sweep"] = dict(pattern="oldest_10pct", kind="fp16", lib_ms={f"{m}MiB": v for m, v in sweep.items()},
                                             median_ms={f"{m}MiB": v for m, v in med.items()},
                                             spread_of_64MiB=round((max(sweep[64]) - min(sweep[64])) / med[64], 4),
                                             spread_of_256MiB=round((max(sweep[256]) - min(sweep[256])) / med[256], 4),
                                             # the rule for the shipped default: the smallest block whose median lies inside the
                                             # range the repeats of the largest cover
                                             default_MiB_by_rule=min(m for m in sweep if min(sweep[256]) <= med[m] <= max(sweep[256])))
        bank.close()
        torch.cuda.empty_cache()
        line = json.dumps(res)                              # the record so far: a later kind that fails leaves the earlier ones
        with open(out_path, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
