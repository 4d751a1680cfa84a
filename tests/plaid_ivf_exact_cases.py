"""THE INVERTED FILE (include/rerank_mi355.h) restated for real sizes, the candidate definition of rr_bank_search_plaid_ivf in numpy,
and banks on which csrc/bank_ivf.hip and the inverted-file form of csrc/bank_search_plaid.hip take the paths the benchmark takes.
Helper of tests/test_plaid_ivf_exact_cases_cpu.py and tests/test_gpu_bank_ivf_scale.py.  Calls nothing of the library.

ivf_fast: np.unique over the (clamped code, passage) pairs of the unmasked rows and a bincount for the offsets: usable at 262 144
centroids and a million rows, where tests/test_bank_ivf_cpu.py's ivf_numpy (a full compare per centroid) is not.
candidates: the sorted union of the lists of a query's cells, cut to a range.  It equals {p : a1[p] != -inf} of
plaid_search_ref.prune, which is what lets the inverted-file form be held to the float64 oracle of the scan form.

The search cases follow the construction of tests/plaid_exact_cases.py (its builders and asserts are used as they are): inputs on
the 1/8 grid, S and the exact MaxSim exact in float32 in any order of the sums.  With E = Lq_coarse * ncells cell entries a query
and `longest` the bank's longest list, the plan's compact score rows hold cap = max(1, min(n, E * longest)) entries.
  BIG    16 384 centroids, 40 007 short passages (1 .. 4 rows, one of 130), 256 pool centroids.  Four HOT centroids sit in every
         17th passage each (about 2 200 with the row unmasked, disjoint but for a few RICH passages holding all four), every other list is far
         shorter.  Used by three cases:
           wide     E 16: cap < n, cap > ndocs, a query with more than 4 096 candidates (two selection slices over a compact row), a
                    query whose candidates all lie at passage 32 768 and above (words >= 1024 of its bitmap: ivf_compact_kernel's
                    second round alone), queries with candidates on both sides;
           strided  E 4, a query whose cells are the four hot centroids: 8 192 < cap < n and more than 8 192 candidates
                    (plaid_score_listed_kernel's second trip), rich passages behind place 8 192 among the survivors;
           control  E 32 with the same queries: cap == n.
  NARROW 16 384 centroids, 301 passages of 1 .. 2 rows whose longest list has 3 entries, E 2: cap 6 < ndocs / 4, and k above cap.
edges (build only, nothing exact needed): 1 500 centroids, 33 500 passages, lists of exactly 0, 1, 2, 3, 255, 256, 257, 4 095,
4 096, 4 097, 9 000 and 5 000 entries at chosen centroids, 0 and C - 1 among them.
million (build and one search call): 1 052 673 passages of one centroid, every 257th also holding a second."""
import numpy as np

import plaid_exact_cases as X
import plaid_ref
import plaid_search_ref as ref

IVF_SORT_MAX = 4096            # entries ivf_sort_kernel sorts in LDS; a longer list is rebuilt through a bitmap
COMPACT_WORDS = 1024           # bitmap words ivf_compact_kernel takes a round: 32 768 passages
LISTED_TRIP = 8192             # candidates of a query plaid_score_listed_kernel takes in its first trip (2 048 groups of 4)


def ivf_fast(codes, mask, lengths, C):
    """(offsets int64 [C + 1], pids int32): the definition, vectorised.  Passages lie back to back in codes / mask."""
    lengths = np.asarray(lengths, dtype=np.int64)
    P = len(lengths)
    codes = np.clip(np.asarray(codes, dtype=np.int64), 0, C - 1)
    pid = np.repeat(np.arange(P, dtype=np.int64), lengths)
    assert len(pid) == len(codes)
    if mask is not None:
        live = np.asarray(mask) != 0
        codes, pid = codes[live], pid[live]
    pair = np.unique(codes * P + pid)                              # ascending by (code, passage), every pair once
    offsets = np.concatenate([[0], np.cumsum(np.bincount(pair // P, minlength=C))]).astype(np.int64)
    return offsets, (pair % P).astype(np.int32)


def candidates(offsets, pids, cells, first=0, n=None):
    """Range-relative, ascending: the union of the lists of the centroids set in `cells` (bool [C]), cut to [first, first + n)."""
    parts = [pids[offsets[c]:offsets[c + 1]] for c in np.flatnonzero(cells)]
    u = np.unique(np.concatenate(parts)) if parts else np.zeros(0, dtype=np.int32)
    if n is not None:
        u = u[(u >= first) & (u < first + n)]
    return (u - first).astype(np.int64)


def cap_of(case, longest, n=None):
    """The plan's pitch of the compact rows (rr_plaid_search_plan, csrc/bank_search_plaid.hip)."""
    n = len(case["lens"]) if n is None else n
    return max(1, min(n, case["Lqc"] * case["ncells"] * int(longest)))


# ---- the exact banks -----------------------------------------------------------------------------------------------------------------
P_BIG, N_POOL_BIG, N_DUPES, LONG_PASSAGE, FULLY_MASKED = 40007, 256, 150, 77, 13
RICH = [100, 20000, 33000] + list(range(38500, 38510)) + [39800]      # the last eleven: behind place 8 192 of the strided query
BANKS = {
    "big":    dict(C=16384, D=64, nbits=2, Lq=16, n_pool=N_POOL_BIG, seed=11),
    "narrow": dict(C=16384, D=64, nbits=2, Lq=4, n_pool=N_POOL_BIG, seed=12),
}
# name: bank, Lqc, ncells, ndocs, k, the queries it takes of the bank's
CASES = {
    "wide":    dict(bank="big", Lqc=8, ncells=2, ndocs=64, k=16, queries=[0, 1, 2, 3]),
    "strided": dict(bank="big", Lqc=2, ncells=2, ndocs=64, k=16, queries=[4, 1]),
    "control": dict(bank="big", Lqc=16, ncells=2, ndocs=64, k=16, queries=[4, 1]),
    "narrow":  dict(bank="narrow", Lqc=2, ncells=1, ndocs=32, k=2, queries=[0, 1, 2]),
    "narrow_k": dict(bank="narrow", Lqc=2, ncells=1, ndocs=32, k=8, queries=[0, 1, 2]),
}


def _table(p, rng):
    """Centroids (float64, fp16-exact), the pool and an exact residual pattern table per pool centroid, as X.build makes them."""
    C, D, nbits = p["C"], p["D"], p["nbits"]
    weights = X.weights_of(nbits)
    cen = X._centroids(C, D, rng)
    must = {0, 5, 7, 200, 255, 256, C - 2, C - 1, 32 * ((C - 1) // 32) - 1, 263, 519, 1023, 1024, C - 300}
    rest = [int(i) for i in rng.permutation(C)[:4 * p["n_pool"]] if int(i) not in must]
    pool = sorted(must) + sorted(rest[:p["n_pool"] - len(must)])
    for c in pool:
        n = 2 if c % 6 == 3 else 4
        cen[c] = 0.0
        cen[c, rng.permutation(X.POOL_DIMS)[:n]] = rng.choice([-0.5, 0.5], size=n)
    for src, dst in X.repeats_of(C):
        cen[dst] = cen[src]
    assert (cen.astype(np.float16).astype(np.float64) == cen).all()
    patterns = {c: X._patterns(cen[c], weights, nbits, rng, want=2, trials=1000) for c in pool}
    return cen, weights, pool, patterns


def _query(cen, near, Lq, rng):
    """Tokens near the centroids `near` (the first len(near) columns take them in turn) plus a sparse perturbation: multiples of 1/8."""
    D = cen.shape[1]
    pick = np.array(near)[rng.integers(0, len(near), size=Lq)]
    pick[:min(len(near), Lq)] = near[:Lq]
    tok = cen[pick].copy()
    for j in range(Lq):
        at = rng.permutation(D)[:3]
        tok[j, at] += rng.integers(-2, 3, size=3) / 8.0
    return np.clip(tok, -1.0, 1.0)


def _cells(cen, q, Lqc, ncells):
    S = X.scores64(cen, q[None])[0]
    return ref.cells_of(S[:, :Lqc], ncells)


def _rows_of(pool_codes, patterns, rng):
    return np.stack([patterns[int(c)][rng.integers(0, len(patterns[int(c)]))] for c in pool_codes])


def _finish(p, cen, weights, pool, lens, codes, buckets, mask, queries):
    codes = np.concatenate(codes).astype(np.int32)
    buckets = np.concatenate(buckets)
    mask = np.concatenate(mask)
    decoded = X.decode64(cen, weights, buckets, codes)
    residuals = plaid_ref.pack_buckets(buckets, p["nbits"])
    assert np.array_equal(plaid_ref.buckets_of(residuals, p["nbits"], p["D"]), buckets)
    q = np.stack(queries)
    assert (q * 8 == np.round(q * 8)).all() and np.abs(q).max() <= 1.0
    flat = q.reshape(-1, p["D"])
    X._assert_exact(cen, flat, 5, "S")
    X._assert_exact(decoded, flat, 6, "exact score")
    out = dict(p)
    out.update(centroids=cen.astype(np.float16), weights=weights, pool=pool, codes=codes, buckets=buckets, residuals=residuals, mask=mask,
               lens=[int(x) for x in lens], decoded=decoded.astype(np.float16), queries=q.astype(np.float32), S=X.scores64(cen, q),
               exact=X.exact_scores(decoded, mask, lens, q), threshold=X.THRESHOLD, fully_masked=FULLY_MASKED)
    return out


def _build_big():
    p = dict(BANKS["big"])
    rng = np.random.default_rng(p["seed"])
    cen, weights, pool, patterns = _table(p, rng)
    C, Lq = p["C"], p["Lq"]
    inpool = np.zeros(C, dtype=bool)
    inpool[pool] = True
    free = [c for c in pool if c not in (0, 256, 7, 200, 5, C - 1)]             # not a repeated row: its cell is its own
    wide, strided = CASES["wide"], CASES["strided"]

    # query 4 (strided): its first two columns open four distinct pool centroids and nothing else: the HOT centroids
    for _ in range(200):
        near = [int(c) for c in rng.choice(free, size=2, replace=False)]
        q4 = _query(cen, near, Lq, rng)
        hot = np.flatnonzero(_cells(cen, q4, strided["Lqc"], strided["ncells"]))
        if len(hot) == 4 and inpool[hot].all():
            break
    else:
        raise AssertionError("no query with four pool cells")
    hot = [int(c) for c in hot]
    # query 0 (late): none of its cells is hot; its pool cells are the LATE centroids, held by passages from 32 768 on only
    for _ in range(200):
        near = [int(c) for c in rng.choice([c for c in free if c not in hot], size=5, replace=False)]
        q0 = _query(cen, near, Lq, rng)
        c0 = np.flatnonzero(_cells(cen, q0, wide["Lqc"], wide["ncells"]))
        if not set(c0) & set(hot) and inpool[c0].any():
            break
    else:
        raise AssertionError("no query without a hot cell")
    late = [int(c) for c in c0 if inpool[c]]
    others = [c for c in pool if c not in hot and c not in late]
    # query 1: near two hot centroids and three others (more than 4 096 candidates on both sides); 2, 3 and 5 .. 19: anywhere
    queries = [q0, _query(cen, hot[:2] + [int(c) for c in rng.choice(others, size=3, replace=False)], Lq, rng)]
    queries += [_query(cen, [int(c) for c in rng.choice(others, size=5, replace=False)], Lq, rng) for _ in range(2)]
    queries.append(q4)
    queries += [_query(cen, [int(c) for c in rng.choice(pool, size=5, replace=False)], Lq, rng) for _ in range(15)]

    n_base = P_BIG - N_DUPES
    cycle = [1, 2, 3, 4, 2, 1, 4, 3, 3, 1, 2]
    early_from, late_from = np.array(others), np.array(others + late * 12)
    ten = np.array(others[:10])
    lens, codes, masks = [], [], []
    for i in range(n_base):
        ln = 130 if i == LONG_PASSAGE else 4 if i in RICH else cycle[i % len(cycle)]
        src = late_from if i >= 32768 else early_from
        cs = src[rng.integers(0, len(src), size=ln)]
        if i == LONG_PASSAGE:
            cs = ten[np.arange(ln) % 10]
        r = i % 17
        if r in (1, 5, 9, 13):
            cs[rng.integers(0, ln)] = hot[(r - 1) // 4]
        if i in RICH:
            cs = np.array(hot)[rng.permutation(4)]
        m = np.ones(ln, dtype=np.uint8)
        if ln >= 3 and i % 2:
            m[1] = 0                                               # an interior masked row
        if i == LONG_PASSAGE:
            m[5::7] = 0
        if i == FULLY_MASKED:
            m[:] = 0
        lens.append(ln); codes.append(cs); masks.append(m)
    buckets = [_rows_of(cs, patterns, rng) for cs in codes]
    dupes = [40 + 211 * j for j in range(N_DUPES - 2)] + RICH[:2]  # stored again at the end of the bank: ties far apart
    assert max(dupes) < 32768 and len(set(dupes)) == N_DUPES
    lens += [lens[i] for i in dupes]
    codes += [codes[i] for i in dupes]
    buckets += [buckets[i] for i in dupes]
    masks += [masks[i] for i in dupes]
    out = _finish(p, cen, weights, pool, lens, codes, buckets, masks, queries)
    out.update(hot=hot, late=late, dupes=dupes, n_base=n_base)
    return out


def _build_narrow():
    p = dict(BANKS["narrow"])
    rng = np.random.default_rng(p["seed"])
    cen, weights, pool, patterns = _table(p, rng)
    P = 301
    lens = [1 + i % 2 for i in range(P)]
    rows = int(np.sum(lens))
    assert rows <= 2 * len(pool)
    deck = np.array(pool * 2)[rng.permutation(2 * len(pool))][:rows]            # every pool centroid at most twice ...
    first = np.concatenate([[0], np.cumsum(lens)])
    codes = [deck[first[i]:first[i + 1]].copy() for i in range(P)]
    three = int(codes[0][0])
    holders = [i for i in range(P) if three in codes[i]]
    extra = next(i for i in range(150, P) if lens[i] == 2 and three not in codes[i])
    codes[extra][1] = three                                                     # ... and one of them a third time
    masks = [np.ones(ln, dtype=np.uint8) for ln in lens]
    masks[FULLY_MASKED][:] = 0
    for i in (21, 45):
        masks[i][0] = 0                                                         # a masked first row
    buckets = [_rows_of(cs, patterns, rng) for cs in codes]
    held = [int(codes[i][j]) for i in range(P) for j in range(lens[i]) if masks[i][j]]
    # query 0 opens the centroid of three passages and another held one, 1 and 2 two held centroids each
    near = [[three, held[7]], [held[100], held[200]], [held[300], held[17]]]
    queries = [_query(cen, nr, p["Lq"], rng) for nr in near]
    out = _finish(p, cen, weights, pool, lens, codes, buckets, masks, queries)
    out.update(three=three, holders=sorted(holders + [extra]))
    return out


_BUILT = {}


def bank(name):
    """The bank `name` of BANKS, built once a process and left unchanged by whoever takes it."""
    if name not in _BUILT:
        _BUILT[name] = {"big": _build_big, "narrow": _build_narrow}[name]()
    return _BUILT[name]


def get(name):
    """(case, oracle) of CASES[name]: the bank's arrays with the case's parameters and queries, in the form X.oracle takes."""
    key = ("case", name)
    if key not in _BUILT:
        c = CASES[name]
        case = dict(bank(c["bank"]))
        qs = c["queries"]
        case.update(name=name, Lqc=c["Lqc"], ncells=c["ncells"], ndocs=c["ndocs"], k=c["k"], nq=len(qs), queries=case["queries"][qs],
                    S=case["S"][qs], exact=case["exact"][qs])
        _BUILT[key] = (case, X.oracle(case))
    return _BUILT[key]


def sixteen_queries():
    """Sixteen queries of the big bank for one call against sixteen (no oracle: the calls are compared with one another)."""
    return bank("big")["queries"][4:20]


# ---- the build-only banks ------------------------------------------------------------------------------------------------------------
C_EDGES, P_EDGES = 1500, 33500
# centroid: entries of its list.  0 and C - 1 among them; three lists above one sort slice, met by the rebuild loop in the order
# 0, 700, C - 1; 1: only under masked rows; 300 .. 699 take the passages nothing else holds
EDGE_LISTS = {0: 4097, 1: 0, 2: 1, 3: 2, 5: 3, 255: 255, 256: 256, 257: 257, 1023: 4095, 1024: 4096, 1025: 3, 700: 9000, C_EDGES - 1: 5000}


def edges():
    """(codes, mask, lens, C) of the edges bank: every centroid of EDGE_LISTS holds exactly that many passages, drawn from the whole
    bank (so from both sides of passage 32 768); rows of a passage in shuffled order, some codes twice, masked rows between."""
    if "edges" not in _BUILT:
        rng = np.random.default_rng(21)
        member = [[] for _ in range(P_EDGES)]
        for c, cnt in EDGE_LISTS.items():
            for p in rng.permutation(P_EDGES)[:cnt]:
                member[int(p)].append(c)
        lens, codes, mask = [], [], []
        for p in range(P_EDGES):
            cs = list(member[p]) or [int(rng.integers(300, 700))]
            ms = [1] * len(cs)
            if p % 3 == 0:
                cs.append(cs[0]); ms.append(1)                                  # a code twice in a passage
            if p % 5 == 0:
                cs.append(1); ms.append(0)                                      # centroid 1 only under masked rows
            if p % 7 == 0:
                cs.append(int(rng.choice(list(EDGE_LISTS)))); ms.append(0)      # a masked row with a counted code
            o = rng.permutation(len(cs))
            codes.append(np.array(cs)[o]); mask.append(np.array(ms, dtype=np.uint8)[o]); lens.append(len(cs))
        _BUILT["edges"] = (np.concatenate(codes).astype(np.int32), np.concatenate(mask), lens, C_EDGES)
    return _BUILT["edges"]


P_MILLION, C_MILLION, EVERYWHERE, SOMETIMES = 1048576 + 4097, 1030, 1029, 3


def million():
    """(codes, mask None, lens, C): P_MILLION passages whose first row holds EVERYWHERE; every 257th has a second row of SOMETIMES."""
    lens = np.ones(P_MILLION, dtype=np.int32)
    lens[::257] = 2
    first = np.concatenate([[0], np.cumsum(lens)])
    codes = np.full(first[-1], EVERYWHERE, dtype=np.int32)
    codes[first[:-1][::257] + 1] = SOMETIMES
    return codes, None, lens, C_MILLION
