"""The fixtures of the fp16-matrix-core bank search (rr_bank_search_f16, include/rerank_mi355.h) and its definition in float64 numpy:
A (the MaxSim with the query rounded once to fp16), E (the exact MaxSim), the survivors and the certificate.  No device, no library.

A fixture is a dict: rows float32 [R, D] (every value exact in fp16), mask uint8 [R], lens (one per passage, rows back to back), q
float32 [nq, Lq, D].  `padded(fx)` gives what PassageBank.add takes.
"""
import numpy as np

MASKED = -9999.0


def first_rows(lens):
    return np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)


def fp16_rne(x):
    """float32 -> the nearest fp16 (ties to even), back as float32: what the kernel does to the query."""
    return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def maxsim64(q, fx, first=0, count=None):
    """float64 [nq, n]: sum over the query's tokens of the largest product with an unmasked row of the passage (a masked row counts
    -9999); q float32 [nq, Lq, D] taken as it is."""
    lens, rows, mask = fx["lens"], fx["rows"].astype(np.float64), fx["mask"]
    fr = first_rows(lens)
    n = len(lens) - first if count is None else count
    out = np.empty((q.shape[0], n))
    q64 = q.astype(np.float64)
    for p in range(n):
        a, ln = fr[first + p], lens[first + p]
        s = np.einsum("rd,qjd->qrj", rows[a:a + ln], q64)                 # [nq, len, Lq]
        s[:, mask[a:a + ln] == 0, :] = MASKED
        out[:, p] = s.max(axis=1).sum(axis=1)
    return out


def approx64(fx, **kw):
    """A in float64: the query rounded to fp16, the products and sums exact."""
    return maxsim64(fp16_rne(fx["q"]), fx, **kw)


def exact64(fx, **kw):
    return maxsim64(fx["q"], fx, **kw)


def rank_order(scores):
    """the one total order over a row of scores without NaN: higher first, equal scores by ascending index"""
    return np.argsort(-np.asarray(scores), kind="stable")


def survivors(A, ndocs):
    """[nq, m] the first m = min(ndocs, n) passages of every row of A in rank order"""
    m = min(ndocs, A.shape[1])
    return np.stack([rank_order(r)[:m] for r in A])


def search_f16(A, E, ndocs, k, slack, first=0):
    """rr_bank_search_f16 from its definition, on given A and E [nq, n] (float32 from the device, or float64): (indices [nq, k] bank
    indices, scores [nq, k], certified [nq]); the certificate's sum a* + slack is a float32 sum when A is float32."""
    surv = survivors(A, ndocs)
    nq, n = A.shape
    idx, sc, cert = np.empty((nq, k), np.int64), np.empty((nq, k), E.dtype), np.empty(nq, np.int32)
    for qi in range(nq):
        s = np.sort(surv[qi])                                             # ties among the survivors go by bank index
        top = s[rank_order(E[qi, s])[:k]]
        idx[qi], sc[qi] = top + first, E[qi, top]
        a_star = A[qi, surv[qi, -1]]
        cert[qi] = 1 if surv.shape[1] == n else int(sc[qi, k - 1] > a_star + A.dtype.type(slack))
    return idx, sc, cert


def default_slack(q, D):
    """passage_bank.f16_default_slack for the queries q [nq, Lq, D], restated"""
    s = np.linalg.norm(q.astype(np.float64), axis=-1).sum(axis=-1).max()
    sr = s * (1.0 + 2.0 ** -10)
    return sr * (2.0 ** -11 + D * 2.0 ** -22) + q.shape[1] * 2.0 ** -22 * sr


def _masks(lens, rng, fully_masked):
    """every row kept, but an interior row of every seventh passage of three rows or more, and every row of `fully_masked`"""
    mask = np.ones(int(np.sum(lens)), np.uint8)
    fr = first_rows(lens)
    for p, ln in enumerate(lens):
        if ln >= 3 and p % 7 == 3:
            mask[fr[p] + 1 + rng.integers(0, ln - 2)] = 0
    mask[fr[fully_masked]:fr[fully_masked] + lens[fully_masked]] = 0
    return mask


def exact_fixture(kind, D, nq, Lq, seed):
    """Entries are multiples of 2^-3 in [-2, 2]: every product is a multiple of 2^-6 below 4 and every partial sum of a dot product
    or of a column sum is exact in float32 in any order, and the query is exact in fp16: A == E bit for bit, whatever the order.
    kind "mixed": 300 passages of 1 .. 40 rows; "short": 4200 passages of 1 .. 3 rows (the selection crosses a 4096 slice)."""
    rng = np.random.default_rng(seed)
    if kind == "mixed":
        lens = [int(v) for v in rng.integers(1, 41, 300)]
        lens[0], lens[1], lens[150], lens[299], lens[17] = 1, 40, 1, 1, 33
    else:
        lens = [p % 3 + 1 for p in range(4200)]
    R = int(np.sum(lens))
    rows = (rng.integers(-16, 17, (R, D)) / 8.0).astype(np.float32)
    q = (rng.integers(-16, 17, (nq, Lq, D)) / 8.0).astype(np.float32)
    return dict(rows=rows, mask=_masks(lens, rng, fully_masked=5), lens=lens, q=q, D=D)


PLANTED = 16          # the passages per query that hold its tokens


def random_fixture(D, nq, Lq, seed):
    """300 passages of 1 .. 40 random unit rows (rounded to fp16), nq queries of Lq random unit tokens.  Passage 16 i + j (i < nq, j <
    16) is PLANTED for query i: 40 - j rows, the first min(40 - j, Lq) of them noisy copies of the query's tokens, so that it scores
    near min(40 - j, Lq) where a random passage scores near 0.3 Lq: the k = 16 best of a query stand far above its 65th best, the
    gap the certificate needs (tests/test_bank_f16_cpu.py shows it in float64).  The other passages: random, 1 .. 28 rows, with
    one-row passages, interior masked rows and one fully masked passage."""
    assert nq * PLANTED <= 272
    rng = np.random.default_rng(seed)
    lens = [40 - p % PLANTED for p in range(272)] + [p + 1 for p in range(28)]
    lens[273], lens[299] = 1, 1
    R = int(np.sum(lens))
    unit = lambda x: x / np.linalg.norm(x, axis=-1, keepdims=True)
    rows = unit(rng.standard_normal((R, D)))
    q = unit(rng.standard_normal((nq, Lq, D))).astype(np.float32)
    fr = first_rows(lens)
    for i in range(nq):
        for j in range(PLANTED):
            p, c = PLANTED * i + j, min(40 - j, Lq)
            rows[fr[p]:fr[p] + c] = unit(q[i, :c] + 0.02 * (j + 1) / np.sqrt(D) * rng.standard_normal((c, D)))
    mask = _masks(lens, rng, fully_masked=280)
    for i in range(nq):                     # a masked interior row must not be a planted copy of a short query
        for j in range(PLANTED):
            p = PLANTED * i + j
            mask[fr[p]:fr[p] + lens[p]] = 1
    mask[fr[1] + 36] = 0                    # ... but interior masked rows behind the copies are there
    return dict(rows=fp16_rne(rows), mask=mask, lens=lens, q=q, D=D)


def adversarial_fixture(D, ndocs):
    """One nonzero product per score, so no accumulation order matters.  Lq 1, the query token (1 + 2^-12) e1 + (1 - 2^-13) e2: both
    elements round to 1.0 in fp16.  ndocs + 8 one-row passages e2 at the low indices, one passage e1 at the highest.  Exactly the e1
    passage scores 1 + 2^-12 and wins; in A every passage scores 1.0, the tie goes by index and the e1 passage is not among the
    ndocs survivors: rr_bank_search_f16 cannot return it, and must not certify."""
    n = ndocs + 9
    rows = np.zeros((n, D), np.float32)
    rows[:n - 1, 1] = 1.0
    rows[n - 1, 0] = 1.0
    q = np.zeros((1, 1, D), np.float32)
    q[0, 0, 0], q[0, 0, 1] = 1.0 + 2.0 ** -12, 1.0 - 2.0 ** -13
    return dict(rows=rows, mask=np.ones(n, np.uint8), lens=[1] * n, q=q, D=D)


def padded(fx, lo=0, hi=None):
    """(context_li float32 [n, Lc, D], context_mask float32 [n, Lc], lengths) of the passages lo .. hi - 1, as PassageBank.add takes them"""
    lens = fx["lens"][lo:hi]
    fr = first_rows(fx["lens"])[lo:hi]
    Lc = max(lens)
    li = np.zeros((len(lens), Lc, fx["D"]), np.float32)
    cm = np.zeros((len(lens), Lc), np.float32)
    for p, (a, ln) in enumerate(zip(fr, lens)):
        li[p, :ln] = fx["rows"][a:a + ln]
        cm[p, :ln] = fx["mask"][a:a + ln]
    return li, cm, list(lens)
