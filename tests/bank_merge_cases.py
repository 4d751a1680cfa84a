"""Inputs for rr_bank_merge_topk ("THE MERGED LIST", include/rerank_mi355.h), shared by tests/test_bank_merge_cpu.py and
tests/test_gpu_bank_merge.py, and a numpy restatement of the definition that calls nothing of the library.

A case is a dict: the three input arrays as views into ONE int32 block laid out as an all-gather delivers it
([P][ indices | score bits | counts | pad ]) or, for `packed`, as three tight arrays; the strides in 4-byte words; the host
offsets; (P, nq, k_in, k).  Scores come from a SMALL set of values so that ties across parts, +0 / -0, NaN, +-inf and -inf
inside a count all occur; local indices are drawn with repetition (an index listed twice within a part) and some fall below 0
or beyond the part.
"""
import numpy as np

NEG0 = np.float32(-0.0)
VALUES = np.array([0.0, -0.0, 1.5, 1.5, -2.25, 3.0, np.inf, -np.inf, np.nan, 7.0, 7.0, 1e-30, -1e-30], dtype=np.float32)
INT32_MAX = (1 << 31) - 1


def merge_reference(idx, sc, cnt, offsets, k):
    """idx int32 / sc float32 [P, nq, k_in] (any strides), cnt int32 [P, nq] or None, offsets [P + 1], k ->
    (indices [nq, k], score bits uint32 [nq, k], counts [nq], parts [nq, k]) by a stable lexsort on (NaN flag, score with
    -0 -> +0 descending, global index ascending) over the real entries taken part by part."""
    P, nq, k_in = idx.shape
    off = np.asarray(offsets, dtype=np.int64)
    out_i = np.full((nq, k), -1, dtype=np.int32)
    out_s = np.full((nq, k), -np.inf, dtype=np.float32)
    out_p = np.full((nq, k), -1, dtype=np.int32)
    out_c = np.zeros(nq, dtype=np.int32)
    for q in range(nq):
        g, s, part = [], [], []
        for p in range(P):
            c = k_in if cnt is None else int(np.clip(cnt[p, q], 0, k_in))
            li = idx[p, q, :c].astype(np.int64)
            real = (li >= 0) & (li < off[p + 1] - off[p])
            g.append(off[p] + li[real])
            s.append(sc[p, q, :c][real])
            part.append(np.full(int(real.sum()), p, dtype=np.int32))
        g, s, part = np.concatenate(g), np.concatenate(s), np.concatenate(part)
        nan = np.isnan(s)
        mag = np.where(nan, np.float32(0.0), s) + np.float32(0.0)          # -0 + +0 = +0
        order = np.lexsort((g, -mag.astype(np.float64), ~nan))             # the last key is the primary one; lexsort is stable
        n = min(k, order.size)
        sel = order[:n]
        out_i[q, :n], out_s[q, :n], out_p[q, :n], out_c[q] = g[sel], s[sel], part[sel], n
    return out_i, out_s.view(np.uint32), out_c, out_p


def make_case(name, P, k_in, k, nq, seed, sizes=None, packed=False, with_counts=True, reach_int32_max=False, spread=False):
    rng = np.random.default_rng(seed)
    if sizes is None:
        sizes = rng.integers(1, 4 * k_in + 2, size=P)
        if P >= 3:
            sizes[1] = 0                                                   # an empty part
    sizes = np.asarray(sizes, dtype=np.int64)
    offsets = np.zeros(P + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(sizes)
    if reach_int32_max:                                                    # the last part ends at 2^31 - 1
        offsets += INT32_MAX - offsets[-1]
    words = nq * k_in
    if packed:
        block = np.zeros(P * (2 * words + nq), dtype=np.int32)
        idx = block[:P * words].reshape(P, nq, k_in)
        sc = block[P * words:2 * P * words].view(np.float32).reshape(P, nq, k_in)
        cnt = block[2 * P * words:].reshape(P, nq)
        part_stride, count_stride = words, nq
    else:
        stride = 2 * words + nq + 3                                        # a status word and two words of slack
        block = np.full(P * stride, 0x5a5a5a5a, dtype=np.int32).reshape(P, stride)
        idx = block[:, :words].reshape(P, nq, k_in)
        sc = block[:, words:2 * words].view(np.float32).reshape(P, nq, k_in)
        cnt = block[:, 2 * words:2 * words + nq]
        part_stride = count_stride = stride
    real_sizes = offsets[1:] - offsets[:-1]
    for p in range(P):
        n = int(real_sizes[p])
        idx[p] = rng.integers(-2, n + 3, size=(nq, k_in)) if n else rng.integers(-2, 3, size=(nq, k_in))
    if spread:                                                             # distinct finite scores with a few of the special ones
        vals = rng.standard_normal((P, nq, k_in)).astype(np.float32)
        mask = rng.random((P, nq, k_in)) < 0.02
        vals[mask] = VALUES[rng.integers(0, VALUES.size, size=int(mask.sum()))]
        sc[...] = vals
    else:
        sc[...] = VALUES[rng.integers(0, VALUES.size, size=(P, nq, k_in))]
    cnt[...] = rng.integers(max(k_in - 3, 0), k_in + 1, size=(P, nq))
    cnt[0, :] = 0 if P > 1 else cnt[0, :]                                  # count 0 for one part
    if P > 1:
        cnt[P - 1, 0] = -3                                                 # negative
        cnt[P - 1, nq - 1] = k_in + 7 if nq > 1 else cnt[P - 1, 0]         # above k_in
    if nq > 2:
        cnt[:, 1] = 0                                                      # count 0 for every part of a query
    return dict(name=name, P=P, nq=nq, k_in=k_in, k=k, block=block, idx=idx, sc=sc, cnt=cnt if with_counts else None,
                part_stride=part_stride, count_stride=count_stride, offsets=offsets.astype(np.int32))


def cases(nq):
    """The cases of the issue at `nq` queries: P * k_in = 1, 2, 3 * 5, 8 * 1024."""
    return [
        make_case("one entry", 1, 1, 1, nq, 1, sizes=[4]),
        make_case("one entry, no counts, packed", 1, 1, 1, nq, 2, sizes=[2], packed=True, with_counts=False),
        make_case("two parts of one", 2, 1, 1, nq, 3),
        make_case("one part of two", 1, 2, 2, nq, 4, sizes=[3], reach_int32_max=True),
        make_case("3 x 5, k 5", 3, 5, 5, nq, 5),
        make_case("3 x 5, k 3, up to 2^31 - 1", 3, 5, 3, nq, 6, reach_int32_max=True),
        make_case("3 x 5, no counts", 3, 5, 4, nq, 7, with_counts=False, packed=True),
        make_case("3 x 5, every part empty but one", 3, 5, 5, nq, 8, sizes=[0, 0, 9]),
        make_case("8 x 1024, ties", 8, 1024, 1024, nq, 9, sizes=[3000, 0, 17, 2500, 1024, 4000, 1, 3333]),
        make_case("8 x 1024, spread, k 100", 8, 1024, 100, nq, 10, sizes=[3000, 5000, 17, 2500, 1024, 4000, 900, 3333], spread=True,
                  reach_int32_max=True),
    ]


def expected(case):
    return merge_reference(case["idx"], case["sc"], case["cnt"], case["offsets"], case["k"])
