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
    with np.errstate(over="ignore"):                                      # 65520 and above: infinity, as on the device
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
        with np.errstate(invalid="ignore"):                               # -inf + inf: NaN, and no comparison with NaN holds
            cert[qi] = 1 if surv.shape[1] == n else int(sc[qi, k - 1] > a_star + A.dtype.type(slack))
    return idx, sc, cert


def old_default_slack(q, D):
    """The default slack as it was before the absolute term: the 2^-11 of the query's rounding taken as relative for EVERY element.
    Kept to show what it certified (tests/test_bank_f16_forms_cpu.py)."""
    s = np.linalg.norm(q.astype(np.float64), axis=-1).sum(axis=-1).max()
    sr = s * (1.0 + 2.0 ** -10)
    return sr * (2.0 ** -11 + D * 2.0 ** -22) + q.shape[1] * 2.0 ** -22 * sr


def default_slack(q, D):
    """F16Search(ndocs).slack_for(q) for the queries q [nq, Lq, D], restated: passage_bank.f16_default_slack, whose term Lq sqrt(D)
    2^-25 R covers the elements below fp16's normal range (their rounding error is absolute, at most 2^-25), and +inf when an
    element is infinite or rounds to infinity in fp16 (magnitude >= 65520)."""
    if (np.abs(q.astype(np.float64)) >= 65520.0).any():
        return np.inf
    return old_default_slack(q, D) + q.shape[1] * np.sqrt(D) * 2.0 ** -25 * (1.0 + 2.0 ** -10)


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
    kind "mixed": 300 passages of 1 .. 40 rows; "short": 4200 passages of 1 .. 3 rows (the selection crosses a 4096 slice); "long":
    long_lens / long_masks below.
    THE CONDITION, asserted: a product is a multiple of 2^-6 and a column sum stays below 4 D Lq in magnitude, so every partial sum
    is a multiple of 2^-6 below 2^18 = 2^(24 - 6), exact in float32, iff D Lq <= 65536 (a fully masked passage scores Lq * -9999, an
    integer below 2^24)."""
    assert D * Lq <= 65536, f"exact_fixture: D {D} x Lq {Lq} = {D * Lq} > 65536: a partial sum may need more than 24 bits"
    rng = np.random.default_rng(seed)
    if kind == "mixed":
        lens = [int(v) for v in rng.integers(1, 41, 300)]
        lens[0], lens[1], lens[150], lens[299], lens[17] = 1, 40, 1, 1, 33
    elif kind == "long":
        lens = long_lens(rng)
    else:
        assert kind == "short", kind
        lens = [p % 3 + 1 for p in range(4200)]
    R = int(np.sum(lens))
    rows = (rng.integers(-16, 17, (R, D)) / 8.0).astype(np.float32)
    q = (rng.integers(-16, 17, (nq, Lq, D)) / 8.0).astype(np.float32)
    mask = long_masks(lens, rng) if kind == "long" else _masks(lens, rng, fully_masked=5)
    return dict(rows=rows, mask=mask, lens=lens, q=q, D=D)


# The "long" passages: 71 of them (two chunks of 32 and a partial one of 7: the four waves of the last workgroup get 2, 2, 2 and 1
# passages).  The first seventeen end on, just before and just behind a 16-row tile after zero to eight two-tile steps of the
# kernel's row loop; the rest are random in 1 .. 130.
LONG_EDGES = [1, 15, 16, 17, 31, 32, 33, 47, 48, 64, 65, 80, 96, 97, 128, 129, 257]
LONG_PASSAGES = 71
LONG_FULLY_MASKED, LONG_ROW0_MASKED, LONG_LAST_MASKED, LONG_ONLY_LAST_KEPT, LONG_TILE_EDGES_MASKED = 3, 5, 8, 13, 16


def long_lens(rng):
    lens = LONG_EDGES + [int(v) for v in rng.integers(1, 131, LONG_PASSAGES - len(LONG_EDGES))]
    assert len(lens) % 32 and max(lens) == 257
    return lens


def long_masks(lens, rng):
    """_masks (an interior row of every seventh passage, passage 3 of 17 rows fully masked) and: row 0 of passage 5 (32 rows), the
    last row of passage 8 (48 rows), every row but row 96 of passage 13 (97 rows: the one kept row is alone in the tail tile behind
    three two-tile steps), rows 15, 16, 31, 32, 63, 64 of passage 16 (257 rows: both sides of a tile edge and of a step edge)."""
    mask = _masks(lens, rng, fully_masked=LONG_FULLY_MASKED)
    fr = first_rows(lens)
    assert (lens[LONG_FULLY_MASKED], lens[LONG_ROW0_MASKED], lens[LONG_LAST_MASKED], lens[LONG_ONLY_LAST_KEPT], lens[LONG_TILE_EDGES_MASKED]) == \
        (17, 32, 48, 97, 257)
    mask[fr[LONG_ROW0_MASKED]] = 0
    mask[fr[LONG_LAST_MASKED] + 47] = 0
    mask[fr[LONG_ONLY_LAST_KEPT]:fr[LONG_ONLY_LAST_KEPT] + 96] = 0
    mask[fr[LONG_ONLY_LAST_KEPT] + 96] = 1
    mask[fr[LONG_TILE_EDGES_MASKED] + np.array([15, 16, 31, 32, 63, 64])] = 0
    return mask


# (D, n_queries, Lq) of tests/test_bank_f16_forms_cpu.py and tests/test_gpu_bank_f16_forms.py: every (NT, TP) of the two launchers,
# one, two and three or more passes at every cap of the block, a padded tile count, a last pass of fewer tokens than a tile, a query
# block whose last slot is empty in a wide form ((3, 49) at (8, 4), (3, 130) at (8, 8)).  The CPU test asserts the coverage.
_NQ_LQ_AT_64_128 = [(1, 16), (2, 9), (1, 17), (4, 16), (2, 32), (1, 33), (1, 48), (5, 1), (3, 31), (2, 64), (3, 49), (1, 65), (2, 128), (1, 129),
                    (3, 130), (1, 257)]
FORM_SHAPES = [(D, nq, Lq) for D in (64, 128) for nq, Lq in _NQ_LQ_AT_64_128] + \
    [(256, 1, 64), (256, 2, 65), (256, 1, 200), (512, 1, 32), (512, 2, 33), (512, 1, 100), (1024, 1, 16), (1024, 2, 17), (1024, 1, 40),
     (32, 3, 20), (96, 3, 20)]


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


def random_fixture_long(D, nq, Lq, seed):
    """random_fixture over the "long" passages (long_lens, long_masks): random unit rows rounded to fp16, nq (<= 3) queries of Lq
    random unit tokens.  Passage 17 + 16 i + j (j < 16) is PLANTED for query i: its first min(length, Lq) rows are noisy copies of
    the query's tokens and none of its rows is masked.  With 71 passages of 1 .. 257 rows the 65th best of a query is one of its
    seven worst, a short or masked passage: the certificate's gap at k 16, ndocs 64 is wide (tests/test_bank_f16_forms_cpu.py
    shows twice the default slack in float64)."""
    assert nq * PLANTED <= LONG_PASSAGES - len(LONG_EDGES)
    rng = np.random.default_rng(seed)
    lens = long_lens(rng)
    R = int(np.sum(lens))
    unit = lambda x: x / np.linalg.norm(x, axis=-1, keepdims=True)
    rows = unit(rng.standard_normal((R, D)))
    q = unit(rng.standard_normal((nq, Lq, D))).astype(np.float32)
    mask = long_masks(lens, rng)
    fr = first_rows(lens)
    for i in range(nq):
        for j in range(PLANTED):
            p = len(LONG_EDGES) + PLANTED * i + j
            c = min(lens[p], Lq)
            rows[fr[p]:fr[p] + c] = unit(q[i, :c] + 0.02 * (j + 1) / np.sqrt(D) * rng.standard_normal((c, D)))
            mask[fr[p]:fr[p] + lens[p]] = 1
    return dict(rows=fp16_rne(rows), mask=mask, lens=lens, q=q, D=D)


def _e1_fixture(D, ndocs, q0, low, high):
    """adversarial_fixture's layout with everything on e1: Lq 1, the query q0 e1, ndocs + 8 one-row passages low e1 at the low
    indices and one passage high e1 at the highest"""
    n = ndocs + 9
    rows = np.zeros((n, D), np.float32)
    rows[:n - 1, 0] = low
    rows[n - 1, 0] = high
    q = np.zeros((1, 1, D), np.float32)
    q[0, 0, 0] = q0
    return dict(rows=rows, mask=np.ones(n, np.uint8), lens=[1] * n, q=q, D=D)


def overflow_fixture(D, ndocs):
    """The query 70000 e1 is +inf in fp16.  Rows -2^-10 e1, the last one -2^-14 e1: every A is -inf, the tie goes by index and the
    last passage is no survivor, yet its exact score -4.27 beats the others' -68.4.  No finite slack bounds |A - E| here."""
    return _e1_fixture(D, ndocs, 70000.0, -2.0 ** -10, -2.0 ** -14)


def underflow_fixture(D, ndocs):
    """The query 2^-26 e1 is 0 in fp16 (a quarter of the smallest subnormal, 2^-24).  Rows 0.5 e1, the last one 1.0 e1: every A
    is 0, the last passage is no survivor, and its exact score 2^-26 is twice the others'.  |A - E| = 2^-26 is ABSOLUTE: a slack
    that takes the rounding as 2^-11 of the query's norm (7.5e-12 here) does not bound it."""
    return _e1_fixture(D, ndocs, 2.0 ** -26, 0.5, 1.0)


def subnormal_mix_fixture(D, seed):
    """40 passages of 1 .. 5 random unit rows; 2 queries of 3 tokens, each a unit vector on the first half of the dimensions with
    elements drawn from (0, 2^-14) on the second half: below fp16's normal range, where the rounding error of an element is absolute
    (up to 2^-25) beside the relative 2^-11 of the unit part."""
    rng = np.random.default_rng(seed)
    lens = [int(v) for v in rng.integers(1, 6, 40)]
    unit = lambda x: x / np.linalg.norm(x, axis=-1, keepdims=True)
    rows = fp16_rne(unit(rng.standard_normal((int(np.sum(lens)), D))))
    q = np.zeros((2, 3, D))
    q[..., :D // 2] = unit(rng.standard_normal((2, 3, D // 2)))
    q[..., D // 2:] = rng.uniform(0.0, 2.0 ** -14, (2, 3, D - D // 2))
    q = q.astype(np.float32)
    assert (q[..., D // 2:] > 0).all() and (q[..., D // 2:] < 2.0 ** -14).all()
    return dict(rows=rows, mask=np.ones(int(np.sum(lens)), np.uint8), lens=lens, q=q, D=D)


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
