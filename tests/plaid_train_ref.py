"""THE TRAINED CENTROIDS (include/rerank_mi355.h, rr_plaid_kmeans), restated from the header's text alone in plain Python / numpy:
the fp16 rounding, the biased score (the fmaf chain of tests/plaid_compress_ref.py plus one float32 add), the rank order of the code,
the exact fixed-point sum in int64, the mean in float64, the splitmix64 re-seed row and the norm in the order of the decoded row.
Slow by design: small inputs only."""
import numpy as np

import plaid_compress_ref as P

M64 = (1 << 64) - 1


def sumsq(row):
    """float32 sum of squares of a float32 row of D = 8 * 2^k values: per chunk of 8 an fmaf chain from zero, then the pairwise tree over
    neighbours."""
    q = []
    for c8 in range(len(row) // 8):
        acc = 0.0
        for k in range(8):
            v = float(row[8 * c8 + k])
            acc = P._libm.fmaf(v, v, acc)
        q.append(np.float32(acc))
    with np.errstate(all="ignore"):
        while len(q) > 1:
            q = [np.float32(q[2 * i] + q[2 * i + 1]) for i in range(len(q) // 2)]
    return q[0]


def fix(x):
    """clamp(v, -256, 256) * 2^24 as int64; NaN -> 0.  x: float32 array holding fp16 values."""
    with np.errstate(all="ignore"):
        v = np.where(np.isnan(x), np.float32(0), np.clip(x, np.float32(-256), np.float32(256))).astype(np.float64)
    return (v * float(1 << 24)).astype(np.int64)


def reseed_row(seed, i, c, R):
    z = (seed ^ ((i << 32) | c)) & M64
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z % R


def kmeans(rows, init_rows, niters, seed):
    """(centroids float16 [C, D], counts int32 [C], stats int32 [niters, 2], codes int32 [R]) of rows [R, D] (float32 or float16)."""
    x16 = np.asarray(rows).astype(np.float16)
    x = x16.astype(np.float32)
    R, D = x.shape
    C = len(init_rows)
    T = x16[np.asarray(init_rows, dtype=np.int64)].copy()                     # fp16 table
    neg_half = np.float32(-0.5)

    def bias(T):
        with np.errstate(all="ignore"):
            return np.array([neg_half * sumsq(T[c].astype(np.float32)) for c in range(C)], dtype=np.float32)

    h = bias(T)
    codes = np.full(R, -1, dtype=np.int32)
    counts = np.zeros(C, dtype=np.int32)
    stats = np.zeros((niters, 2), dtype=np.int32)
    for i in range(niters):
        Tf = T.astype(np.float32)
        new = np.zeros(R, dtype=np.int32)
        with np.errstate(all="ignore"):
            for r in range(R):
                best = None
                for c in range(C):
                    s = np.float32(P.score(Tf[c], x[r]) + h[c])
                    if best is None or P.ranks_before(s, c, best[0], best[1]):
                        best = (s, c)
                new[r] = best[1]
        stats[i, 0] = int((new != codes).sum())
        codes = new
        A = np.zeros((C, D), dtype=np.int64)
        np.add.at(A, codes, fix(x))
        counts = np.bincount(codes, minlength=C).astype(np.int32)
        for c in range(C):
            if counts[c] == 0:
                T[c] = x16[reseed_row(seed, i, c, R)]
                stats[i, 1] += 1
            else:
                mean = A[c].astype(np.float64) / np.float64(int(counts[c]) << 24)
                with np.errstate(all="ignore"):
                    T[c] = mean.astype(np.float32).astype(np.float16)
        h = bias(T)
    out = np.zeros((C, D), dtype=np.float16)
    with np.errstate(all="ignore"):
        for c in range(C):
            t = T[c].astype(np.float32)
            d = np.fmax(np.sqrt(sumsq(t), dtype=np.float32), np.float32(1e-12))     # fmaxf: a NaN norm gives 1e-12
            out[c] = (t / d).astype(np.float32).astype(np.float16)
    return out, counts, stats, codes
