"""Cases of rr_plaid_kmeans, rr_plaid_residuals and rr_op_plaid_compress_rows (include/rerank_mi355.h, THE TRAINED CENTROIDS and THE
COMPRESSED ROW) at real centroid counts on which the assignment is EXACT arithmetic, and an oracle in vectorised numpy that calls
nothing of the library.  Helper of tests/test_plaid_train_exact_cases_cpu.py and tests/test_gpu_plaid_train_scale.py.

Why exact: rows are multiples of GRID = 1/16 (planted centres with six entries of k/8, members a centre plus three entries of +-1/8 or
+-1/16, "lines" of members along one coordinate), the table holds fp16 values, so every term T[c][e] * x[r][e] of a score is a multiple
of u = (the smallest fp16 lsb among the table's non-zero values) * GRID, and the largest sum of |terms| stays below 2^24 u: every
partial sum of the float32 fmaf chain, in any order, is representable, and a float64 T @ x.T (BLAS, chunked over C) is every bit of
it.  _assert_exact ASSERTS that on the table of every iteration.  What is order-faithful and not exact — the bias h[c] and the final
norm — comes from tests/plaid_train_ref.py's sumsq, row by row; the rest of the definition is restated here in numpy: one float32
add of the bias, the rank maximum (np.argmax: a NaN is the largest, the first of equal values wins), the int64 sums of
plaid_train_ref.fix, the float64 mean rounded to float32 and to fp16, plaid_train_ref.reseed_row, the float32 division of the output.

So that the cases BITE, the builder also asserts: pairs of equal initial rows at centroid-index distances 16 (the next wave's tile),
64 (the same wave's next tile), 256, 1024, 4096 and C / 2 (those below C; whatever split boundaries the plan picks) whose rows the
tie decides — the LOWER index wins, the upper cluster is empty and is re-seeded; 0 < changed < R in at least two iterations; cluster
sizes that are no powers of two (the mean really rounds); winners in every quarter of the index range.  The float32 sources hold
values that are no fp16 values and round to the grid rows (offsets of a quarter of an fp16 ulp, +-1e-30 for the zeros, so the fp16
rows hold both zeros)."""
import numpy as np

import plaid_ref
import plaid_train_ref as T

GRID = 1.0 / 16
SEED = 0x5EED0123456789AB
TIE_DISTANCES = (16, 64, 256, 1024, 4096)              # and C / 2
LINE_T = (0, 1, 2, 3, 4, 5, 6)                         # a line's members: centre + t / 8 along one coordinate; the first two are initial rows

# name: D, C, R, iterations, lines (groups of two initial centroids at one end of len(LINE_T) members: the boundary moves a member an
# iteration), extra pairs of equal initial rows (each an empty cluster: the re-seeds keep codes changing), seed
KM = {
    "km4096": dict(D=128, C=4096, R=8192, niters=4, lines=256, dupes=8, seed=0),      # the automatic plan: 16 splits of 256
    "km512d": dict(D=512, C=1024, R=2049, niters=3, lines=64, dupes=8, seed=1),       # jt 2, lpr 64, 8 accumulate trips
    "km256d": dict(D=256, C=512, R=1100, niters=3, lines=32, dupes=8, seed=2),
    "km32d":  dict(D=32, C=600, R=2051, niters=3, lines=40, dupes=8, seed=3),         # two rows a wave instruction; R no multiple of 32
    "km64d":  dict(D=64, C=4096, R=4100, niters=3, lines=0, dupes=64, seed=4),
    "km16d":  dict(D=16, C=4096, R=5000, niters=3, lines=100, dupes=16, seed=5),
    "tiny":   dict(D=16, C=8, R=64, niters=3, lines=1, dupes=1, seed=6),              # what the slow restatement can follow
}
# name: D, C, R, nbits, seed
CP = {
    "cp65536":  dict(D=128, C=65536, R=300, nbits=(8, 2), seed=7),                    # the automatic plan: 64 splits of 1024
    "cp262144": dict(D=64, C=262144, R=130, nbits=(1,), seed=8),
}


def tie_distances(C):
    return sorted({d for d in TIE_DISTANCES + (C // 2,) if 0 < d < C})


def cutoffs_of(nbits):
    """Non-decreasing cutoffs among which lie values a residual takes (multiples of 1/16): the STRICT count decides those."""
    n = (1 << nbits) - 1
    step = {1: 1.0, 2: 1.0 / 16, 4: 1.0 / 32, 8: 1.0 / 64}[nbits]
    return ((np.arange(n) - n // 2) * step).astype(np.float32)


def _centres(n, D, rng, kmax=4):
    """[n, D] float64: up to six non-zero entries of +-k / 8, k in 1 .. kmax."""
    cen = np.zeros((n, D))
    pos = rng.integers(0, D, size=(n, 6))
    val = rng.integers(1, kmax + 1, size=(n, 6)) * rng.choice([-1.0, 1.0], size=(n, 6)) / 8.0
    cen[np.arange(n)[:, None], pos] = val
    return cen


def _perturb(rows, rng, entries=3):
    """rows + `entries` entries of +-1/8 or +-1/16 each."""
    n, D = rows.shape
    pos = rng.integers(0, D, size=(n, entries))
    val = rng.choice([-0.125, -0.0625, 0.0625, 0.125], size=(n, entries))
    out = rows.copy()
    np.add.at(out, (np.arange(n)[:, None], pos), val)
    return out


def float32_source(x, rng):
    """float32 values that are NO fp16 values and round to x: a quarter of an fp16 ulp off, +-1e-30 where x is 0."""
    x16 = x.astype(np.float16)
    assert (x16.astype(np.float64) == x).all()
    sign = rng.choice([-1.0, 1.0], size=x.shape)
    off = np.where(x == 0, 1e-30, np.spacing(np.abs(x16)).astype(np.float64) / 4) * sign
    x32 = (x + off).astype(np.float32)
    assert (x32.astype(np.float16).astype(np.float32) != x32).all()
    assert (x32.astype(np.float16).astype(np.float64) == x).all()
    return x32


def _assert_exact(T16, x):
    """Every term of T16 @ x.T a multiple of u, every sum of |terms| below 2^24 u; (bound, limit).  The bound's own matmul is in
    float32: a sum of D non-negative terms, at most D 2^-24 of itself too small, which the factor 1.001 more than covers."""
    assert (x / GRID == np.round(x / GRID)).all(), "a row is off the grid"
    nz = T16[T16 != 0]
    assert nz.size and np.isfinite(nz).all()
    u = float(np.spacing(np.abs(nz)).min()) * GRID
    a, b = np.abs(T16).astype(np.float32), np.abs(x).astype(np.float32)
    bound = max(float((a[c:c + 8192] @ b.T).max()) for c in range(0, len(a), 8192)) * 1.001
    assert bound < 2.0 ** 24 * u, f"sum of |terms| {bound} reaches 2^24 u = {2.0 ** 24 * u}"
    return bound, 2.0 ** 24 * u


def assign(T16, x, h=None, chunk=1024):
    """code int32 [R]: the rank maximum over c of float32(T16[c] . x[r]) (+ h[c], one float32 add).  x [R, D] float64."""
    best = code = None
    xt = np.ascontiguousarray(x.T)
    with np.errstate(all="ignore"):
        for c0 in range(0, len(T16), chunk):
            S64 = T16[c0:c0 + chunk].astype(np.float64) @ xt
            S = S64.astype(np.float32)
            assert (S.astype(np.float64) == S64).all(), "a score is no float32"
            if h is not None:
                S = S + h[c0:c0 + chunk, None]
            am = np.argmax(S, axis=0)                        # a NaN is the largest; the first of equal values (+0 == -0)
            v = S[am, np.arange(S.shape[1])]
            if best is None:
                best, code = v, am.astype(np.int32)
            else:
                up = (v > best) | (np.isnan(v) & ~np.isnan(best))      # equal scores stay with the lower index
                best = np.where(up, v, best)
                code = np.where(up, am + c0, code).astype(np.int32)
    return code


_SUMSQ = {}


def _sumsq_rows(T16):
    """float32 [C]: plaid_train_ref.sumsq of every table row (remembered by the row's bytes: most rows outlive an iteration)."""
    out = np.empty(len(T16), dtype=np.float32)
    Tf = T16.astype(np.float32)
    for c in range(len(T16)):
        k = T16[c].tobytes()
        if k not in _SUMSQ:
            _SUMSQ[k] = T.sumsq(Tf[c])
        out[c] = _SUMSQ[k]
    return out


def kmeans(rows, init_rows, niters, seed):
    """THE TRAINED CENTROIDS: dict(centroids fp16 [C, D], counts int32 [C], stats int32 [niters, 2], codes [niters][R], tables
    [niters + 1] (the fp16 table each assignment saw, and the last), bounds [(bound, limit)] of every assignment)."""
    x16 = np.asarray(rows).astype(np.float16)
    x = x16.astype(np.float64)
    R, C = len(x), len(init_rows)
    T16 = x16[np.asarray(init_rows, dtype=np.int64)].copy()
    fixed = T.fix(x16.astype(np.float32))
    prev = np.full(R, -1, dtype=np.int32)
    counts = np.zeros(C, dtype=np.int32)
    stats = np.zeros((niters, 2), dtype=np.int32)
    codes, tables, bounds = [], [T16.copy()], []
    for i in range(niters):
        bounds.append(_assert_exact(T16, x))
        h = (np.float32(-0.5) * _sumsq_rows(T16)).astype(np.float32)
        code = assign(T16, x, h)
        stats[i, 0] = int((code != prev).sum())
        prev = code
        codes.append(code)
        A = np.zeros((C, x.shape[1]), dtype=np.int64)
        np.add.at(A, code, fixed)
        counts = np.bincount(code, minlength=C).astype(np.int32)
        with np.errstate(all="ignore"):
            mean = A.astype(np.float64) / (np.maximum(counts, 1).astype(np.int64) << 24).astype(np.float64)[:, None]
            T16 = mean.astype(np.float32).astype(np.float16)
        for c in np.flatnonzero(counts == 0):
            T16[c] = x16[T.reseed_row(seed, i, int(c), R)]
            stats[i, 1] += 1
        tables.append(T16.copy())
    t = T16.astype(np.float32)
    with np.errstate(all="ignore"):
        d = np.fmax(np.sqrt(_sumsq_rows(T16), dtype=np.float32), np.float32(1e-12))
        out = (t / d[:, None]).astype(np.float32).astype(np.float16)
    return dict(centroids=out, counts=counts, stats=stats, codes=codes, tables=tables, bounds=bounds)


def residuals(rows, cen16):
    """(codes int32 [R], float32 residuals [R, D]) of THE COMPRESSED ROW steps 1 - 4 without the buckets."""
    x16 = np.asarray(rows).astype(np.float16)
    code = assign(np.asarray(cen16, dtype=np.float16), x16.astype(np.float64))
    with np.errstate(all="ignore"):
        res = x16.astype(np.float32) - np.asarray(cen16).astype(np.float32)[code]
    return code, res


def pack(res, cutoffs, nbits):
    """(buckets [R, D], packed bytes): bucket = the cutoffs STRICTLY below the residual (a NaN: 0), bit j of element e at position
    e * nbits + j of a bit stream that fills bytes from the most significant end (tests/plaid_compress_ref.py's rule)."""
    with np.errstate(invalid="ignore"):
        buckets = (np.asarray(cutoffs, dtype=np.float32)[None, None, :] < res[:, :, None]).sum(axis=2)
    return buckets, plaid_ref.pack_buckets(buckets, nbits)


def _slots(C, n_pairs_extra, rng):
    """(source slot, copy slot) pairs: one a tie distance, then n_pairs_extra at other distances; no slot twice."""
    used, pairs = set(), []
    for d in tie_distances(C) + [None] * n_pairs_extra:
        for _ in range(10000):
            s = int(rng.integers(0, C - (d or 1)))
            t = s + d if d else int(rng.integers(s + 1, C))
            if s not in used and t not in used:
                break
        else:
            raise AssertionError("no free slots for a pair")
        used |= {s, t}
        pairs.append((s, t))
    return pairs


def build_km(name):
    """The k-means case `name`: rows (fp16 and float32 sources of the same values), init_rows, pairs (slot, slot, row, row), the
    oracle's result under "want"."""
    p = dict(KM[name])
    D, C, R, niters, lines = p["D"], p["C"], p["R"], p["niters"], p["lines"]
    rng = np.random.default_rng(p["seed"])
    pairs = _slots(C, p["dupes"], rng)
    n_clusters = C - 2 * lines - len(pairs)                  # plain clusters: one initial row each, the pairs' among them twice
    extra = R - C - (len(LINE_T) - 2) * lines                # members that are no initial rows
    assert n_clusters >= len(pairs) and extra >= 2
    cen = _centres(n_clusters + lines, D, rng)
    rows, inits = [], []                                     # inits: row indices in slot-free order, filled into the free slots below
    first = _perturb(cen[:n_clusters], rng)                  # every plain cluster's initial row
    rows.append(first)
    inits += list(range(n_clusters))
    n = n_clusters
    owner = np.sort(rng.integers(0, n_clusters, size=extra))
    owner[1] = owner[0]                                      # one cluster of at least three members
    rows.append(_perturb(cen[owner], rng))
    n += extra
    line_rows = []
    for g in range(lines):
        c = cen[n_clusters + g]
        free = np.flatnonzero(c == 0)
        k = int(free[rng.integers(0, len(free))])
        m = np.tile(c, (len(LINE_T), 1))
        m[:, k] += np.array(LINE_T) / 8.0
        m = _perturb(m, rng, entries=1)
        m[:, k] = c[k] + np.array(LINE_T) / 8.0               # the line's coordinate itself stays unperturbed
        line_rows.append(m)
        inits += [n, n + 1]
        n += len(LINE_T)
    if lines:
        rows.append(np.concatenate(line_rows))
    copies = first[:len(pairs)].copy()                       # plain cluster i < len(pairs): its initial row a second time
    rows.append(copies)
    pair_rows = [(i, n + i) for i in range(len(pairs))]
    n += len(pairs)
    x = np.concatenate(rows)
    assert x.shape == (R, D) and n == R
    order = rng.permutation(R)                               # row index order tells nothing
    where = np.empty(R, dtype=np.int64)
    where[order] = np.arange(R)
    x = x[order]
    init_rows = np.full(C, -1, dtype=np.int64)
    for (s, t), (a, b) in zip(pairs, pair_rows):
        init_rows[s], init_rows[t] = where[a], where[b]
    rest = [where[r] for r in inits if r >= len(pairs)]
    free_slots = rng.permutation(np.flatnonzero(init_rows < 0))
    assert len(rest) == len(free_slots)
    init_rows[free_slots] = rest
    assert len(set(init_rows.tolist())) == C and init_rows.min() >= 0
    x32 = float32_source(x, rng)
    x16 = x32.astype(np.float16)                             # the grid rows, zeros of both signs
    want = kmeans(x16, init_rows, niters, SEED)
    pairs = [(s, t, int(where[a]), int(where[b])) for (s, t), (a, b) in zip(pairs, pair_rows)]
    p.update(name=name, rows16=x16, rows32=x32, init_rows=init_rows.astype(np.int32), pairs=pairs, seed=SEED, want=want)
    _assert_bites_km(p)
    return p


def km_facts(p):
    """What the oracle's run of a k-means case has."""
    w, C, R = p["want"], p["C"], p["R"]
    sizes = set(np.concatenate([np.bincount(c, minlength=C) for c in w["codes"]]).tolist())
    return dict(reseeds=w["stats"][:, 1].tolist(), changed=w["stats"][:, 0].tolist(),
                odd_sizes=sorted(s for s in sizes if s & (s - 1)),
                quarters=[sorted(set((c.astype(np.int64) * 4 // C).tolist())) for c in w["codes"]],
                ties=[(t - s, int(w["codes"][0][a]), int(w["codes"][0][b])) for s, t, a, b in p["pairs"]],
                bounds=w["bounds"], max_size=max(sizes))


def _assert_bites_km(p):
    w, C, R = p["want"], p["C"], p["R"]
    f = km_facts(p)
    assert f["changed"][0] == R and sum(0 < ch < R for ch in f["changed"]) >= min(2, p["niters"] - 1), f["changed"]
    assert f["reseeds"][0] >= len(p["pairs"]) >= 1, f["reseeds"]
    assert f["odd_sizes"], "every cluster size is a power of two"
    assert all(q == [0, 1, 2, 3] for q in f["quarters"]) or C < 16
    t0 = w["tables"][0]
    have = set()
    for s, t, a, b in p["pairs"]:                            # equal table rows (a zero may differ in sign: the products and the
        assert s < t and (t0[s] == t0[t]).all()              # squares do not): the scores tie bit for bit, and they are the rows' best
        assert w["codes"][0][a] == s and w["codes"][0][b] == s, "a tie's rows do not have their maximum on the repeated value"
        have.add(t - s)
    assert have >= set(tie_distances(C))
    assert int(np.bincount(w["codes"][0], minlength=C)[[t for _, t, _, _ in p["pairs"]]].sum()) == 0


def build_cp(name):
    """The compression case `name`: centroids fp16 [C, D] with rows repeated at the tie distances, rows (both sources), per nbits the
    cutoffs, and the oracle's codes, residuals, buckets and packed bytes."""
    p = dict(CP[name])
    D, C, R = p["D"], p["C"], p["R"]
    rng = np.random.default_rng(p["seed"])
    cen = _centres(C, D, rng)
    pairs = _slots(C, 0, rng)
    for s, t in pairs:                                       # a repeated row: six entries of +-1/2 at six places, the largest norm there is
        cen[s] = 0.0
        cen[s, rng.permutation(D)[:6]] = rng.choice([-0.5, 0.5], size=6)
        cen[t] = cen[s]
    flat = [c for st in pairs for c in st]
    pick = np.concatenate([flat, flat, rng.integers(0, C, size=R - 2 * len(flat))]).astype(np.int64)
    x = cen[pick].copy()
    x[len(flat):] = _perturb(x[len(flat):], rng)             # the first rows ARE the repeated rows; the next lie near them
    order = rng.permutation(R)
    x, pick = x[order], pick[order]
    x32 = float32_source(x, rng)
    x16 = x32.astype(np.float16)
    cen16 = cen.astype(np.float16)
    assert (cen16.astype(np.float64) == cen).all()
    bound = _assert_exact(cen16, x)
    code, res = residuals(x16, cen16)
    packed = {}
    for nbits in p["nbits"]:
        cut = cutoffs_of(nbits)
        buckets, by = pack(res, cut, nbits)
        assert by.shape == (R, D // 8 * nbits) and np.array_equal(plaid_ref.buckets_of(by, nbits, D), buckets)
        packed[nbits] = dict(cutoffs=cut, buckets=buckets, bytes=by)
    p.update(name=name, centroids=cen16, rows16=x16, rows32=x32, pairs=pairs, pick=pick, codes=code, residuals=res, packed=packed,
             bound=bound)
    _assert_bites_cp(p)
    return p


def _assert_bites_cp(p):
    C, code, pick, cen = p["C"], p["codes"], p["pick"], p["centroids"]
    assert sorted(set((code.astype(np.int64) * 4 // C).tolist())) == [0, 1, 2, 3]
    assert {t - s for s, t in p["pairs"]} >= set(tie_distances(C))
    for s, t in p["pairs"]:                                  # rows drawn from either copy go to the lower one: the tie decided
        assert np.array_equal(cen[s].view(np.uint16), cen[t].view(np.uint16))
        assert (code[pick == s] == s).all() and (code[pick == t] == s).all() and (pick == t).sum() >= 2 and (pick == s).sum() >= 2
    if C > 65536:
        assert (code > 65535).sum() >= 16
    for nbits, q in p["packed"].items():
        hit = np.isin(p["residuals"], q["cutoffs"])          # residuals ON a cutoff: the strict count decides their bucket
        assert hit.any() and len(np.unique(q["buckets"])) >= min(1 << nbits, 5)


_BUILT = {}


def get(name):
    """The case `name` of KM or CP with its oracle, built once a process; shared, so left unchanged by whoever takes it."""
    if name not in _BUILT:
        _BUILT[name] = build_km(name) if name in KM else build_cp(name)
    return _BUILT[name]
