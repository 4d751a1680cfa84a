#!/usr/bin/env python3
"""Extending a bank's inverted file over added passages (rr_bank_extend_ivf, PassageBank.extend_ivf) against building it again
over everything (rr_bank_build_ivf), in one process, for the same final state.

Bank: `--passages` passages (100 000) with lengths U[64, 180], PLAID codes over `--centroids` centroids (16 384) with the cluster
structure of tools/bench_bank_search_plaid.py: a passage draws its codes from `--topics` centroids of its own (8).  The inverted
file reads codes and mask bytes only, so the residual bytes are kept short (nbits 2) to spare the uploads.  Then 1 %, 10 % and
100 % more passages of the same kind are added (`--grow`, per cent).

Per proportion, `--warmup` untimed and `--iters` timed turns, each on a FRESH bank (created, filled with the base passages, file
built over them, the new passages added, device idle):
  (e) rr_bank_extend_ivf: host clock around the C call, which synchronises its stream itself
  (b) rr_bank_build_ivf on the grown bank, the same way: the file it leaves is the one (e) left (compared, byte for byte, in the
      first turn: `equal_bytes`)
(e) has to run first: after (b) there is nothing to extend.  So (b) finds codes and mask that (e) has just read; the order favours
the rebuild, never the extend.  Reported per proportion: the medians, every turn, build_over_extend = median (b) / median (e), and
what rr_bank_ivf_info says before and after.  A row where the extend does not beat the rebuild stays in the record with
beats_rebuild false.
One JSON line to stdout and to --out.  Needs an MI355X: without a device it fails."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passages", type=int, default=100000)
    ap.add_argument("--centroids", type=int, default=16384)
    ap.add_argument("--topics", type=int, default=8)
    ap.add_argument("--grow", type=int, nargs="+", default=[1, 10, 100])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="profiles/bank_ivf_extend_bench.json.log")
    args = ap.parse_args()

    import numpy as np
    import torch
    import rmr_amd

    if not torch.cuda.is_available():
        raise SystemExit("bench_bank_ivf_extend: no GPU (the figures are not measured without an MI355X)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    arch = rmr_amd.make_arch(dict(cross_encoder_num_hidden_layers=3, cross_encoder_max_position_embeddings=750, loss_fn="BCE",
                                  pos_weight=None), model_kind="interaction", has_vision=0)
    D, P0, C, nbits = arch["li_dim"], args.passages, args.centroids, 2
    eng = rmr_amd.RerankEngine(arch, dev)                  # a handle is all the calls need (no weights)
    Pmax = P0 + P0 * max(args.grow) // 100
    g = torch.Generator().manual_seed(2025)
    clen = torch.randint(64, 181, (Pmax,), generator=g)
    lens, first = clen.tolist(), np.concatenate([[0], np.cumsum(clen.numpy())])
    rows = int(first[-1])
    codec = rmr_amd.PlaidCodec(torch.nn.functional.normalize(torch.randn(C, D, generator=g), dim=-1),
                               torch.randn(1 << nbits, generator=g) * (0.25 / D ** 0.5), nbits)
    topics = torch.randint(0, C, (Pmax, args.topics), generator=g)
    pid = torch.repeat_interleave(torch.arange(Pmax), clen)
    codes = topics[pid, torch.randint(0, args.topics, (rows,), generator=g)].to(torch.int32).numpy()
    resid = torch.randint(0, 256, (rows, codec.residual_bytes), generator=g, dtype=torch.uint8).numpy()
    print(f"source: {Pmax} passages, {rows} rows", file=sys.stderr, flush=True)

    def add(bank, a, b):
        r = slice(int(first[a]), int(first[b]))
        bank.add_compressed(range(a, b), codes[r], resid[r], lens[a:b])

    def timed(entry, bank):
        torch.cuda.synchronize()
        st = torch.cuda.current_stream(dev).cuda_stream
        t0 = time.perf_counter()
        rc = entry(bank.h, st)                              # synchronises st before it returns
        ms = (time.perf_counter() - t0) * 1e3
        assert rc == 0, bank.lib.rr_bank_last_error(bank.h)
        return ms

    res = dict(device=torch.cuda.get_device_name(0), passages=P0, lengths=[64, 180], centroids=C, topics=args.topics, nbits=nbits,
               iters=args.iters, warmup=args.warmup, order="extend, then build, on one fresh bank per turn", grow={})
    for pct in args.grow:
        P = P0 + P0 * pct // 100
        t = dict(extend=[], build=[])
        before = after = equal = None
        for it in range(args.warmup + args.iters):
            bank = eng.create_bank(int(first[P]), P, codec=codec)
            add(bank, 0, P0)
            before = bank.build_ivf()
            add(bank, P0, P)
            e_ms = timed(bank.lib.rr_bank_extend_ivf, bank)
            if it == 0:
                ext_pids, ext_lengths = bank.ivf()
            b_ms = timed(bank.lib.rr_bank_build_ivf, bank)
            after = bank.ivf_info()
            if it == 0:
                pids, lengths = bank.ivf()
                equal = bool(torch.equal(pids, ext_pids) and torch.equal(lengths, ext_lengths))
                del pids, lengths, ext_pids, ext_lengths
            if it >= args.warmup:
                t["extend"].append(round(e_ms, 3)), t["build"].append(round(b_ms, 3))
            bank.close()
            torch.cuda.empty_cache()
        med = {k: statistics.median(v) for k, v in t.items()}
        res["grow"][f"{pct}pct"] = dict(added=P - P0, passages_after=P, rows_added=int(first[P] - first[P0]), extend_ms=med["extend"],
                                        build_ms=med["build"], build_over_extend=round(med["build"] / med["extend"], 2),
                                        beats_rebuild=bool(med["extend"] < med["build"]), equal_bytes=equal, ivf_before=before,
                                        ivf_after=after, turns=t)
        print(f"  +{pct} %: extend {med['extend']:.2f} ms, build {med['build']:.2f} ms", file=sys.stderr, flush=True)
    line = json.dumps(res)
    out = args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
