"""Cases of rr_bank_search_plaid (include/rerank_mi355.h) on which the whole search is EXACT arithmetic, and an oracle in float64
numpy that calls nothing of the library.  Helper of tests/test_plaid_exact_cases_cpu.py and tests/test_gpu_bank_search_plaid_scale.py.

Why exact: centroids hold a few entries of {+-0.25, +-0.5, +-1}, query tokens are multiples of 1/8 in [-1, 1], so every product of
S = centroids @ query.T is a multiple of 2^-5 and a row's sum of |products| stays far below 2^19: any order of float32 partial
sums gives the float64 value.  Bucket weights and residual bytes are chosen so that a decoded row (centroid + weight, divided by
its norm, rounded to fp16: csrc/plaid_decode.h) has a sum of squares of exactly 0.25, 1 or 4: the division is by a power of two,
the row is a multiple of 1/8, differs from its centroid, and the exact MaxSim is exact as well (products: multiples of 2^-6).
The builder ASSERTS all of that.  Such inputs have ties in every column of S; centroid rows repeated at chosen indices make whole
rows of S tie where the kernels of csrc/bank_search_plaid.hip split their work (the 256-stride of the cell search, the 256-centroid
workgroups and 32-bit words of the bitmaps).  The centroid-only stages come from tests/plaid_search_ref.py (the contract in numpy:
A1 / A2 are float32 chains in a DEFINED order and need not be exact); S and the exact scores come from float64."""
import numpy as np

import plaid_ref
import plaid_search_ref as ref

LEN_CYCLE = [1, 15, 16, 17, 40, 63, 64, 65, 130]       # tests/test_gpu_bank_search_plaid.py's: around the 16-row tile and the 64-code step
N_TOPICS = 4
N_POOL = 48                                            # centroids the passages draw their codes from
POOL_DIMS = 16                                         # the pool's rows live in the first dimensions: they overlap one another
SUMSQ_OK = (0.25, 1.0, 4.0)
THRESHOLD = 0.5

# name: C, D, nbits, Lq, Lqc, ncells, ndocs, k, nq, n_base (passages before the duplicates; every dupe_step-th, default 9th, is
# stored twice), seed
CASES = {
    "c257":    dict(C=257, D=64, nbits=1, Lq=32, Lqc=20, ncells=3, ndocs=32, k=8, nq=3, n_base=270, seed=0),
    "c300":    dict(C=300, D=64, nbits=4, Lq=130, Lqc=70, ncells=4, ndocs=9, k=2, nq=2, n_base=270, seed=3),
    "c1000":   dict(C=1000, D=64, nbits=1, Lq=32, Lqc=20, ncells=16, ndocs=64, k=8, nq=3, n_base=270, seed=0),
    "c16384":  dict(C=16384, D=64, nbits=8, Lq=32, Lqc=20, ncells=2, ndocs=32, k=8, nq=3, n_base=270, seed=4),
    "c16384w": dict(C=16384, D=128, nbits=2, Lq=32, Lqc=32, ncells=2, ndocs=1024, k=8, nq=2, n_base=27, dupe_step=2, seed=3),
    "c262144": dict(C=262144, D=64, nbits=1, Lq=4, Lqc=2, ncells=1, ndocs=32, k=8, nq=2, n_base=270, seed=1),
}


def weights_of(nbits):
    """Bucket weights, multiples of 0.5 with 0 at bucket 0: [0, 0.5] at nbits 1, a cycle through {0, 0.5, 1, -1, -0.5} above."""
    b = np.arange(1 << nbits)
    return (0.5 * ((b + 2) % 5 - 2)).astype(np.float32)


def repeats_of(C):
    """(source, copy) centroid indices: row `copy` is made equal to row `source`.  0 / 256: one residue of the cell search's
    256-stride, two workgroups of the bitmap kernel, either side of 255 | 256.  7 / 200: one workgroup, two residues, two words.
    5 / C - 1: either side of the start of the last 32-bit word (at C = 257 the pair 0 / 256 is that pair)."""
    assert C > 256
    rep = [(0, 256), (7, 200)]
    if C - 1 != 256:
        rep.append((5, C - 1))
    last_word = 32 * ((C - 1) // 32)
    assert any(s < last_word <= d for s, d in rep)
    return rep


def _centroids(C, D, rng):
    """fp16-exact [C, D] float64: four non-zero entries a row.  Pool rows are written over these later."""
    pos = np.argsort(rng.random((C, D)), axis=1)[:, :4]
    mags = np.array([[0.5, 0.5, 0.5, 0.5], [0.5, 0.5, 0.25, 0.25], [1.0, 0.25, 0.25, 0.25]])[rng.integers(0, 3, size=C)]
    cen = np.zeros((C, D))
    np.put_along_axis(cen, pos, mags * rng.choice([-1.0, 1.0], size=(C, 4)), axis=1)
    return cen


def _pool(C, rng):
    must = {0, 5, 7, 200, 255, 256, C - 2, C - 1, 32 * ((C - 1) // 32) - 1}    # C - 2: in the last word, no copy of a lower row
    if C > 600:
        must |= {263, 519, C - 300}                   # further workgroups of the bitmap kernel, 263 in the residue of 7
    rest = [int(i) for i in rng.permutation(C)[:4 * N_POOL] if int(i) not in must]
    return sorted(must) + sorted(rest[:N_POOL - len(must)])


def _patterns(row, weights, nbits, rng, want=4, trials=4000):
    """Up to `want` bucket rows [D] for the centroid `row` whose decoded row is exact and differs from the centroid."""
    D = len(row)
    zero_b = np.flatnonzero(weights == 0)
    other_b = np.flatnonzero(weights != 0)
    m = rng.choice([2, 3, 4, 6, 12], size=trials)
    bias = rng.choice([-0.6, 0.0, 2.0], size=trials)
    rank = np.argsort(np.argsort(rng.random((trials, D)) + bias[:, None] * (row != 0)[None, :], axis=1), axis=1)
    changed = rank < m[:, None]
    buckets = np.where(changed, rng.choice(other_b, size=(trials, D)), rng.choice(zero_b, size=(trials, D)))
    s = row[None, :] + weights.astype(np.float64)[buckets]
    sumsq = (s * s).sum(axis=1)
    ok = np.isin(sumsq, SUMSQ_OK)
    ok &= (s / np.sqrt(np.where(ok, sumsq, 1.0))[:, None] != row[None, :]).any(axis=1)
    found, seen = [], set()
    for t in np.flatnonzero(ok):                      # one of each sum of squares first, then whatever else is valid
        if sumsq[t] not in seen:
            seen.add(sumsq[t])
            found.append(t)
    found += [t for t in np.flatnonzero(ok) if t not in found]
    assert found, "no exact residual pattern for a pool centroid"
    return buckets[found[:want]]


def decode64(cen, weights, buckets, codes):
    """The decoded rows in float64 from bucket indices, every step asserted exact: sum of squares 0.25, 1 or 4."""
    s = cen[codes] + weights.astype(np.float64)[buckets]
    sumsq = (s * s).sum(axis=1)
    assert np.isin(sumsq, SUMSQ_OK).all(), "a decoded row's sum of squares is not 0.25, 1 or 4"
    dec = s / np.sqrt(sumsq)[:, None]
    assert (dec.astype(np.float16).astype(np.float64) == dec).all() and (dec * 8 == np.round(dec * 8)).all()
    return dec


def _assert_exact(a, b, g, what):
    """a [n, D] . b [m, D]: every product a multiple of 2^-g, every row's sum of |products| below 2^(24 - g)."""
    ga = g - 3                                        # a: multiples of 2^-(g - 3), b: multiples of 2^-3, so a product: of 2^-g
    assert (a * 2 ** ga == np.round(a * 2 ** ga)).all() and (b * 8 == np.round(b * 8)).all(), f"{what}: a product is no multiple of 2^-{g}"
    bound = (np.abs(a) @ np.abs(b).T).max()           # itself exact: a sum of such products
    assert bound < 2.0 ** (24 - g), f"{what}: a row's sum of |products| reaches 2^{24 - g}"


def build(name, seed=None):
    """The case `name` of CASES as a dict: the codec's tables, the bank's rows, the queries and the float64 oracle's S / exact."""
    return build_from(CASES[name], name, seed)


def build_from(params, name, seed=None):
    """`build` for parameters of the form of a CASES entry that need not be one (tests/coded_exact_cases.py derives cases)."""
    p = dict(params)
    C, D, nbits, Lq, nq = p["C"], p["D"], p["nbits"], p["Lq"], p["nq"]
    rng = np.random.default_rng(p["seed"] if seed is None else seed)
    weights = weights_of(nbits)
    cen = _centroids(C, D, rng)
    pool = _pool(C, rng)
    for c in pool:                                    # pool rows: four +-0.5 (every sixth: two) within the first POOL_DIMS dimensions
        n = 2 if c % 6 == 3 else 4
        cen[c] = 0.0
        cen[c, rng.permutation(POOL_DIMS)[:n]] = rng.choice([-0.5, 0.5], size=n)
    for src, dst in repeats_of(C):
        assert src in pool and dst in pool
        cen[dst] = cen[src]
    assert (cen.astype(np.float16).astype(np.float64) == cen).all()
    patterns = {c: _patterns(cen[c], weights, nbits, rng) for c in pool}

    # passages: LEN_CYCLE lengths, codes from N_TOPICS pool centroids each, interior masked rows, one fully masked, duplicates
    n_base = p["n_base"]
    dupes = list(range(5, n_base, 9)) if "dupe_step" not in p else list(range(1, n_base, p["dupe_step"]))
    fully_masked = 13
    base = [LEN_CYCLE[i % len(LEN_CYCLE)] for i in range(n_base)]
    codes, buckets, masks = [], [], []
    for i, ln in enumerate(base):
        topics = rng.permutation(len(pool))[:N_TOPICS]
        cs = np.array(pool)[topics[rng.integers(0, N_TOPICS, size=ln)]]
        codes.append(cs)
        buckets.append(np.stack([patterns[int(c)][rng.integers(0, len(patterns[int(c)]))] for c in cs]))
        m = np.ones(ln, dtype=np.uint8)
        if i % 2:
            m[2::3] = 0
        if i == fully_masked:
            m[:] = 0
        masks.append(m)
    lens = base + [base[i] for i in dupes]
    codes = np.concatenate(codes + [codes[i] for i in dupes]).astype(np.int32)
    buckets = np.concatenate(buckets + [buckets[i] for i in dupes])
    mask = np.concatenate(masks + [masks[i] for i in dupes])
    decoded = decode64(cen, weights, buckets, codes)
    residuals = plaid_ref.pack_buckets(buckets, nbits)
    assert residuals.shape == (len(codes), D // 8 * nbits)
    assert np.array_equal(plaid_ref.buckets_of(residuals, nbits, D), buckets)

    # queries: tokens near a handful of pool centroids (sources and copies of the repeated rows among them) plus a sparse
    # perturbation, multiples of 1/8 clipped to [-1, 1]
    rep = repeats_of(C)
    q = np.zeros((nq, Lq, D))
    for qi in range(nq):
        src, dst = rep[qi % len(rep)]
        near = [src, dst if qi % 2 else src] + [pool[int(i)] for i in rng.permutation(len(pool))[:3]]
        pick = np.array(near)[rng.integers(0, len(near), size=Lq)]
        pick[0] = src
        if qi == 0 and Lq > 1:
            pick[1] = C - 2
        tok = cen[pick].copy()
        for j in range(Lq):
            at = rng.permutation(D)[:3]
            tok[j, at] += rng.integers(-4, 5, size=3) / 8.0
        q[qi] = np.clip(tok, -1.0, 1.0)
    assert (q * 8 == np.round(q * 8)).all() and np.abs(q).max() <= 1.0

    flat = q.reshape(nq * Lq, D)
    _assert_exact(cen, flat, 5, "S")
    _assert_exact(decoded, flat, 6, "exact score")
    S = scores64(cen, q)
    exact = exact_scores(decoded, mask, lens, q)
    p.update(name=name, centroids=cen.astype(np.float16), weights=weights, pool=pool, repeats=rep, codes=codes, buckets=buckets,
             residuals=residuals, mask=mask, lens=lens, decoded=decoded.astype(np.float16), queries=q.astype(np.float32), S=S, exact=exact,
             dupes=dupes, fully_masked=fully_masked, threshold=THRESHOLD)
    return p


_BUILT = {}


def get(name):
    """(case, oracle(case)) of CASES[name], built once a process; shared, so left unchanged by whoever takes it."""
    if name not in _BUILT:
        case = build(name)
        _BUILT[name] = (case, oracle(case))
    return _BUILT[name]


def exact_scores(decoded, mask, lens, q):
    """float32 [nq, P]: sum over ALL Lq columns of max(-9999, max over the passage's unmasked decoded rows of row . token), in float64,
    asserted to be a float32 (so any float32 order of the sum gives it)."""
    nq, Lq, _ = q.shape
    out = np.empty((nq, len(lens)))
    first = np.concatenate([[0], np.cumsum(lens)])
    for qi in range(nq):
        dots = decoded.astype(np.float64) @ q[qi].astype(np.float64).T      # [rows, Lq]
        for pi in range(len(lens)):
            live = dots[first[pi]:first[pi + 1]][mask[first[pi]:first[pi + 1]].astype(bool)]
            col = np.full(Lq, -9999.0) if not len(live) else np.maximum(-9999.0, live.max(axis=0))
            out[qi, pi] = col.sum()
    f = out.astype(np.float32)
    empty = out == -9999.0 * Lq                       # no unmasked row: a sum of integers, exact below 2^24
    assert (f.astype(np.float64) == out).all() and np.abs(out[~empty]).max() < 2.0 ** 18 and 9999.0 * Lq < 2.0 ** 24
    return f


def scores64(cen, q, by_element=False):
    """S [nq, C, Lq] = centroids @ query.T in float64, asserted to be float32 values where finite.  by_element: the sum over D
    written out (no BLAS between a NaN or an inf and its place in S: 0 * inf = NaN, whatever the order)."""
    cen, q = np.asarray(cen, dtype=np.float64), np.asarray(q, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if by_element:
            S64 = np.stack([(cen[:, None, :] * q[qi][None, :, :]).sum(axis=2) for qi in range(len(q))])
        else:
            S64 = np.stack([cen @ q[qi].T for qi in range(len(q))])
        S = S64.astype(np.float32)
    fin = np.isfinite(S64)
    assert (S.astype(np.float64)[fin] == S64[fin]).all()
    return S


def oracle(case, first=0, count=None, S=None, exact=None):
    """Per query dict(cells, keep, a1, a2, list1, list2, final) over the passages [first, first + count), indices range-relative."""
    lens = case["lens"]
    count = len(lens) - first if count is None else count
    row0 = int(np.sum(lens[:first]))
    rows = int(np.sum(lens[first:first + count]))
    S = case["S"] if S is None else S
    exact = case["exact"] if exact is None else exact
    out = []
    for qi in range(S.shape[0]):
        w = ref.prune(S[qi][:, :case["Lqc"]], case["codes"][row0:row0 + rows], case["mask"][row0:row0 + rows], lens[first:first + count],
                      case["ncells"], case["threshold"], case["ndocs"])
        w["final"] = ref.final(w["list2"], exact[qi][first:first + count], case["k"])
        out.append(w)
    return out
