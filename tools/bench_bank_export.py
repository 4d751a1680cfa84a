#!/usr/bin/env python3
"""Export of a compressed passage bank (rr_bank_export_plaid), saving it as a PLAID index and loading it back with its inverted file.

Bank: that of tools/bench_bank_search_plaid.py (`--passages` passages, default 100 000, of U[64, 180] rows at the handle's li_dim
128, nbits 8, `--centroids` centroids, codes drawn from 8 topics per passage), with 10 % of the rows masked at random (the first
row of every passage stays).

1. `export`: wall-clock of PassageBank.export_compressed over the whole bank in chunks of `--chunk` passages (25 000), the
   synchronisation behind every call included, with and without the copy of every chunk to the host.  The comparison is the only
   route the library had before: a PassageBank.read_compressed loop (one synchronisation and three copies per passage), timed on the
   first `--sample` passages (2 000) and SCALED to the bank by passages (`read_loop_ms_scaled`; `read_loop_scaled` says so).
2. `move`: the move kernel.  rr_bank_export_plaid as an export call and as a sizing call take turns on one chunk; the sizing call
   runs the count, the scan and the read-back, the export call the same and the move (plus one launch), so the difference of the
   medians is the move kernel's time as the host sees it (`move_ms_by_difference`).  Where torch's profiler traces the process's
   kernels, `move_kernel_ms_traced` is the device duration of export_move_kernel itself, from a pass of its own.  The yardstick is
   a hipMemcpyDtoDAsync of the same byte count (R * (residual bytes + 4)), timed by device events in the same process, the legs
   taking turns: `move_GBps` and `copy_GBps` count the bytes once (a copy of n bytes reads n and writes n).
3. `index`: PassageBank.save_plaid_index into a temporary directory, then load_plaid_index(ivf=True) (the file is verified against
   a fresh build) beside load_plaid_index + build_ivf and beside load_plaid_index + load_ivf(verify=False), each into a new bank,
   end to end, `--index-rounds` times.
One JSON line to stdout and to --out."""
import argparse
import ctypes
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passages", type=int, default=100000)
    ap.add_argument("--centroids", type=int, default=16384)
    ap.add_argument("--topics", type=int, default=8)
    ap.add_argument("--chunk", type=int, default=25000)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--masked", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--index-rounds", type=int, default=2)
    ap.add_argument("--out", default="profiles/bank_export_bench.json.log")
    args = ap.parse_args()

    import numpy as np
    import torch
    import rmr_amd

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    arch = rmr_amd.make_arch(dict(cross_encoder_num_hidden_layers=3, cross_encoder_max_position_embeddings=750, loss_fn="BCE",
                                  pos_weight=None), model_kind="interaction", has_vision=0)
    D, nbits, P, C = arch["li_dim"], 8, args.passages, args.centroids
    eng = rmr_amd.RerankEngine(arch, dev)                  # a handle is all the calls need (no weights)
    g = torch.Generator().manual_seed(2025)
    clen = torch.randint(64, 181, (P,), generator=g)
    lens, rows = clen.tolist(), int(clen.sum())
    codec = rmr_amd.PlaidCodec(torch.nn.functional.normalize(torch.randn(C, D, generator=g), dim=-1),
                               torch.randn(1 << nbits, generator=g) * (0.25 / D ** 0.5), nbits,
                               bucket_cutoffs=torch.linspace(-0.25, 0.25, (1 << nbits) - 1))
    rb = codec.residual_bytes
    topics = torch.randint(0, C, (P, args.topics), generator=g)
    pid = torch.repeat_interleave(torch.arange(P), clen)
    codes = topics[pid, torch.randint(0, args.topics, (rows,), generator=g)].to(torch.int32)
    resid = torch.randint(0, 256, (rows, rb), generator=g, dtype=torch.uint8)
    mask = (torch.rand(rows, generator=g) >= args.masked).to(torch.uint8)
    mask[torch.cat([torch.zeros(1, dtype=torch.int64), clen.cumsum(0)[:-1]])] = 1
    bank = eng.create_bank(rows, P, codec=codec)
    bank.add_compressed(list(range(P)), codes, resid, lens, mask=mask)
    kept = int(mask.sum())
    del codes, resid, pid, topics
    print(f"bank: {P} passages, {rows} rows, {kept} unmasked", file=sys.stderr, flush=True)
    res = dict(device=torch.cuda.get_device_name(0), passages=P, passage_rows=rows, unmasked_rows=kept, D=D, nbits=nbits, residual_bytes=rb,
               centroids=C, chunk_passages=args.chunk, iters=args.iters, warmup=args.warmup, rounds=args.rounds)
    ranges = [(f, min(args.chunk, P - f)) for f in range(0, P, args.chunk)]

    # ---- 1. export_compressed over the bank against the read_compressed loop ----
    def export_device():
        return [bank.export_compressed(f, n) for f, n in ranges]

    def export_host():
        out = []
        for f, n in ranges:
            c, r, d = bank.export_compressed(f, n)
            out.append((c.cpu(), r.cpu(), d))
        return out

    def read_loop():
        return [bank.read_compressed(i) for i in range(min(args.sample, P))]
    for fn in (export_device, export_host, read_loop):
        fn()
    per = dict(device=[], host=[], read=[])
    for _ in range(args.rounds):
        for key, fn in (("device", export_device), ("host", export_host), ("read", read_loop)):
            per[key].append(round(timed(fn)[0], 3))
    sample = min(args.sample, P)
    got = export_host()
    want = read_loop()
    row = 0
    same = True
    for (c1, r1, m1), d in zip(want, got[0][2]):                  # the sample lies in the first chunk
        k = m1 != 0
        same = same and d == int(k.sum()) and torch.equal(got[0][0][row:row + d], c1[k]) and torch.equal(got[0][1][row:row + d], r1[k])
        row += d
    read_ms = statistics.median(per["read"])
    res["export"] = dict(round_ms=per, export_ms=statistics.median(per["device"]), export_to_host_ms=statistics.median(per["host"]),
                         read_loop_sample_passages=sample, read_loop_sample_ms=read_ms, read_loop_scaled=True,
                         read_loop_ms_scaled=round(read_ms * P / sample, 1),
                         read_loop_scaled_over_export_to_host=round(read_ms * P / sample / statistics.median(per["host"]), 1),
                         rows_exported=sum(int(c.numel()) for c, _, _ in got), sample_equals_read_compressed=bool(same))
    del got, want
    print("  export done", file=sys.stderr, flush=True)

    # ---- 2. the move kernel beside a device-to-device copy of its bytes ----
    f0, n0 = ranges[0]
    doclens, R = bank._export_sizes(f0, n0)
    co = torch.empty(R, device=dev, dtype=torch.int32)
    ro = torch.empty((R, rb), device=dev, dtype=torch.uint8)
    dl = np.empty(n0, dtype=np.int32)
    got_rows = ctypes.c_int64(0)
    st = torch.cuda.current_stream().cuda_stream
    nbytes = R * (rb + 4)
    src = torch.empty(nbytes, device=dev, dtype=torch.uint8).random_(0, 256)
    dst = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    with open("/proc/self/maps") as f:                     # the HIP runtime this process runs on already (torch's), not a second copy
        hip_path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    hip = ctypes.CDLL(hip_path)
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]

    def sizing():
        assert bank.lib.rr_bank_export_plaid(bank.h, f0, n0, dl.ctypes.data, None, None, 0, ctypes.byref(got_rows), st) == 0

    def export():
        assert bank.lib.rr_bank_export_plaid(bank.h, f0, n0, dl.ctypes.data, co.data_ptr(), ro.data_ptr(), R, ctypes.byref(got_rows), st) == 0

    def copy():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        assert hip.hipMemcpyDtoDAsync(dst.data_ptr(), src.data_ptr(), nbytes, st) == 0
        b.record()
        b.synchronize()
        return a.elapsed_time(b)
    for _ in range(args.warmup):
        sizing(), export(), copy()
    t = dict(sizing=[], export=[], copy=[])
    for _ in range(args.rounds * args.iters):
        t["sizing"].append(timed(sizing)[0])
        t["export"].append(timed(export)[0])
        t["copy"].append(copy())
    med = {k: statistics.median(v) for k, v in t.items()}
    move_ms = med["export"] - med["sizing"]
    traced = None
    try:                                                    # the kernel's own device duration, where the profiler sees this process's kernels
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(5):
                export()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if "export_move_kernel" in e.name]
        dur = [getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0) for e in ev]
        if dur and min(dur) > 0:
            traced = round(statistics.median(dur) / 1e3, 4)
    except Exception as e:                                  # not measured: the difference above stands alone
        print(f"  kernel trace unavailable: {type(e).__name__}: {e}", file=sys.stderr, flush=True)
    best = traced if traced else move_ms
    res["move"] = dict(chunk_passages=n0, rows=R, bytes=nbytes, sizing_call_ms=round(med["sizing"], 4), export_call_ms=round(med["export"], 4),
                       move_ms_by_difference=round(move_ms, 4), move_kernel_ms_traced=traced, copy_dtod_ms=round(med["copy"], 4),
                       move_GBps=round(nbytes / best / 1e6, 1), copy_GBps=round(nbytes / med["copy"] / 1e6, 1),
                       move_over_copy_rate=round(med["copy"] / best, 3), move_time_from="trace" if traced else "difference")
    del src, dst, co, ro
    print("  move done", file=sys.stderr, flush=True)

    # ---- 3. the index directory, end to end ----
    tmp = tempfile.mkdtemp(prefix="rr_plaid_index_")
    try:
        idx = dict(save_ms=[], load_with_ivf_ms=[], load_then_build_ms=[], load_then_trusted_ivf_ms=[])
        for r in range(args.index_rounds):
            d = os.path.join(tmp, f"index{r}")
            idx["save_ms"].append(round(timed(lambda: bank.save_plaid_index(d, chunk_passages=args.chunk))[0], 1))
            print(f"  index round {r}: save_ms {idx['save_ms'][-1]}", file=sys.stderr, flush=True)
            codec2, _ = rmr_amd.read_plaid_index(d)
            infos = []
            for key in ("load_with_ivf_ms", "load_then_build_ms", "load_then_trusted_ivf_ms"):
                b2 = eng.create_bank(kept, P, codec=codec2)

                def load():
                    if key == "load_with_ivf_ms":
                        b2.load_plaid_index(d, ivf=True)
                    elif key == "load_then_build_ms":
                        b2.load_plaid_index(d)
                        b2.build_ivf()
                    else:
                        b2.load_plaid_index(d)
                        b2.load_ivf(d, verify=False)
                idx[key].append(round(timed(load)[0], 1))
                print(f"  index round {r}: {key} {idx[key][-1]}", file=sys.stderr, flush=True)
                infos.append(b2.ivf_info())
                b2.close()
            assert infos[0] == infos[1] == infos[2] == bank.ivf_info()
            size = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
            shutil.rmtree(d)
        res["index"] = dict(rounds=idx, **{k: statistics.median(v) for k, v in idx.items()}, directory_bytes=size, ivf=bank.ivf_info())
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    bank.close()
    line = json.dumps(res)
    out = args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
