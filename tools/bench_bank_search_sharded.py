#!/usr/bin/env python3
"""A passage bank held as several banks: the merge of their k-lists (rr_bank_merge_topk) and search_banks end to end.

Bank: the compressed bank of tools/bench_bank_search.py (`--passages` passages, default 100 000, lengths U[64, 180] at li_dim 128,
nbits 8), held as 1, 2, 4 and 8 banks in one process (the corpus cut into equal slices in corpus order).  Queries: Lq 32, n_queries
1 and 16; k 100 and 1024.

Per (banks, n_queries, k):
  merge     RerankEngine.bank_merge_topk over the stacked per-bank results (computed once, outside the timed call), against the
            COMPOSED route a caller has today: torch.cat of the global indices and of the scores, a stable descending sort, the first
            k.  Where no two scores of a merged list tie, the two must give the same indices (asserted before anything is timed).
            Wall-clock per call including the synchronisation behind it, the legs taking turns; `kernel_ms`: the device time of the
            one launch from the handle's profile.
  search    passage_bank.search_banks end to end (every bank searched, the merge, the ids from the tables), wall-clock per call, the
            bank counts taking turns.
`--rehearse-one-gpu N` (N <= 4): sharding.ShardedBank.search with N processes over gloo on ONE card, each holding its slice of a
smaller corpus (`--rehearse-passages`), as bench.py rehearses its collective: what it times is the host staging, not a fabric.
One JSON line to stdout and to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wall_ms(fns, iters, warmup):
    import torch
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out[i].append((time.perf_counter() - t0) * 1e3)
    return out


def make_engine(dev):
    import rmr_amd
    arch = rmr_amd.make_arch(dict(cross_encoder_num_hidden_layers=3, cross_encoder_max_position_embeddings=750, loss_fn="BCE",
                                  pos_weight=None), model_kind="interaction", has_vision=0)
    return rmr_amd.RerankEngine(arch, dev), arch["li_dim"]


def make_corpus(P, D, centroids, seed=2024):
    """(codec, lengths, codes, residual bytes) of the benchmark corpus, on the host."""
    import torch
    import rmr_amd
    g = torch.Generator().manual_seed(seed)
    clen = torch.randint(64, 181, (P,), generator=g)
    rows = int(clen.sum())
    codec = rmr_amd.PlaidCodec(torch.nn.functional.normalize(torch.randn(centroids, D, generator=g), dim=-1),
                               torch.randn(256, generator=g) * (0.5 / D ** 0.5), 8)
    codes = torch.randint(0, centroids, (rows,), generator=g, dtype=torch.int32)
    resid = torch.randint(0, 256, (rows, codec.residual_bytes), generator=g, dtype=torch.uint8)
    return codec, clen, codes, resid


def slice_bank(eng, corpus, a, b):
    """The passages [a, b) of the corpus as a compressed bank under their corpus numbers."""
    import torch
    codec, clen, codes, resid = corpus
    first = torch.cat([torch.zeros(1, dtype=torch.int64), clen.cumsum(0)])
    r0, r1 = int(first[a]), int(first[b])
    bank = eng.create_bank(max(r1 - r0, 1), max(b - a, 1), codec=codec)
    if b > a:
        bank.add_compressed(list(range(a, b)), codes[r0:r1], resid[r0:r1], clen[a:b].tolist())
    return bank


def _rehearse_worker(rank, world, port, args, q):
    import datetime

    import torch
    import torch.distributed as dist
    from rmr_amd.sharding import ShardedBank, shard_range
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=300))
    try:
        dev = torch.device("cuda:0")
        torch.cuda.set_device(dev)
        eng, D = make_engine(dev)
        corpus = make_corpus(args.rehearse_passages, D, args.centroids)
        a, b = shard_range(args.rehearse_passages, rank, world)
        shard = ShardedBank(slice_bank(eng, corpus, a, b))
        shard.refresh()
        g = torch.Generator().manual_seed(7)
        out = {}
        for nq in args.queries:
            qs = torch.nn.functional.normalize(torch.randn(nq, args.Lq, D, generator=g), dim=-1).to(dev)
            for k in args.k:
                keep = {}

                def search():
                    keep["r"] = shard.search(eng, qs, k)
                t = wall_ms([search], args.iters, args.warmup)[0]
                out[f"nq{nq}_k{k}"] = dict(search_ms=round(statistics.median(t), 4), first_ids=keep["r"][0][0][:5])
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def rehearse(args):
    import socket

    import torch.multiprocessing as mp
    world = args.rehearse_one_gpu
    assert 1 <= world <= 4, "--rehearse-one-gpu takes at most 4 processes on the one card"
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_rehearse_worker, args=(r, world, port, args, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = sorted((q.get(timeout=900) for _ in ps), key=lambda t: t[0])
    for p in ps:
        p.join(timeout=60)
    assert all(r[1] == res[0][1] or all(r[1][c]["first_ids"] == res[0][1][c]["first_ids"] for c in r[1]) for r in res), \
        "the ranks disagree on the merged result"
    return dict(world=world, backend="gloo, staged through pinned host memory", passages=args.rehearse_passages, per_rank=[r[1] for r in res])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passages", type=int, default=100000)
    ap.add_argument("--Lq", type=int, default=32)
    ap.add_argument("--k", type=int, nargs="+", default=[100, 1024])
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--banks", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--centroids", type=int, default=16384)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rehearse-one-gpu", type=int, default=0, metavar="N")
    ap.add_argument("--rehearse-passages", type=int, default=20000)
    ap.add_argument("--out", default="profiles/bank_merge_bench.json.log")
    args = ap.parse_args()

    import torch
    from rmr_amd.passage_bank import search_bank_part, search_banks
    from rmr_amd.sharding import shard_range

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    eng, D = make_engine(dev)
    P = args.passages
    corpus = make_corpus(P, D, args.centroids)
    held = {n: [slice_bank(eng, corpus, *shard_range(P, r, n)) for r in range(n)] for n in args.banks}
    res = dict(device=torch.cuda.get_device_name(0), passages=P, passage_rows=int(corpus[1].sum()), D=D, Lq=args.Lq, nbits=8,
               centroids=args.centroids, iters=args.iters, warmup=args.warmup, configs={})
    g = torch.Generator().manual_seed(11)
    for nq in args.queries:
        q = torch.nn.functional.normalize(torch.randn(nq, args.Lq, D, generator=g), dim=-1).to(dev)
        for k in args.k:
            cfg = {}
            for n, banks in held.items():
                parts = [search_bank_part(eng, b, q, k) for b in banks]
                idx, sc, cnt = (torch.stack([p[key] for p in parts]) for key in ("indices", "scores", "counts"))
                off = [0]
                for b in banks:
                    off.append(off[-1] + len(b))
                off_d = torch.tensor(off[:-1], device=dev, dtype=torch.int32)
                keep = {}

                def merge():
                    keep["m"] = eng.bank_merge_topk(idx, sc, cnt, off, k)

                def composed():
                    gi = torch.where(idx >= 0, idx + off_d[:, None, None], idx).permute(1, 0, 2).reshape(nq, n * k)
                    gs = sc.permute(1, 0, 2).reshape(nq, n * k)
                    s, o = torch.sort(gs, dim=1, descending=True, stable=True)
                    keep["c"] = (torch.gather(gi, 1, o[:, :k]), s[:, :k])

                merge()
                composed()
                torch.cuda.synchronize()
                ms = keep["m"]["scores"]
                untied = bool((ms[:, 1:] != ms[:, :-1]).all())
                if untied:
                    assert torch.equal(keep["m"]["indices"], keep["c"][0]), f"{n} banks, nq {nq}, k {k}: the merge and cat + sort disagree"
                tm, tc = wall_ms([merge, composed], args.iters, args.warmup)
                eng.set_profiling(True)
                eng.get_profile(reset=True)
                merge()
                kernel = round(eng.get_profile(reset=True)["tail"]["ms"], 4)
                eng.set_profiling(False)
                cfg[f"banks{n}"] = dict(no_score_ties=untied, indices_agree=untied or None, merge_ms=round(statistics.median(tm), 4),
                                        composed_ms=round(statistics.median(tc), 4), merge_kernel_ms=kernel,
                                        merge_over_composed=round(statistics.median(tm) / statistics.median(tc), 4))
            fns = [(lambda banks=banks: search_banks(eng, banks, q, k)) for banks in held.values()]
            for n, t in zip(held, wall_ms(fns, args.iters, args.warmup)):
                cfg[f"banks{n}"]["search_banks_ms"] = round(statistics.median(t), 4)
            first = search_banks(eng, held[args.banks[0]], q, k)[0]
            assert all(search_banks(eng, banks, q, k)[0] == first for banks in held.values()), "the bank counts disagree on the ids"
            res["configs"][f"nq{nq}_k{k}"] = cfg
    if args.rehearse_one_gpu:
        del held
        torch.cuda.empty_cache()
        res["rehearse_one_gpu"] = rehearse(args)
    line = json.dumps(res)
    out = args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
