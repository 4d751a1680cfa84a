"""The contract of rr_bank_search_plaid (include/rerank_mi355.h) restated in numpy from a given S: cells, candidates, the two
centroid-only pruning stages and the final cut.  Written from the definition: float32 scalars, maxima in which a NaN sticks,
columns summed one after the other from 0.0f, and ONE order everywhere: NaN first, then higher score, then lower index
(+0 == -0).  -inf marks "absent".  Helper of tests/test_plaid_search_cpu.py, tests/test_gpu_bank_search_plaid.py
and tests/plaid_exact_cases.py."""
import numpy as np

MASKED = np.float32(-9999.0)
NEG_INF = np.float32(-np.inf)


def order(scores, idx=None):
    """`idx` (default 0 .. n-1, ascending) in rank order by scores[idx]: NaN first, higher first, equal scores by lower index."""
    idx = list(range(len(scores))) if idx is None else sorted(int(i) for i in idx)
    def key(i):
        s = float(scores[i])
        return (0, 0.0) if s != s else (1, -s)                  # -(+0.0) == -(-0.0): equal; sorted() is stable
    return sorted(idx, key=key)


def cells_of(S, ncells):
    """bool [C]: the union over the columns of S [C, Lq_coarse] of each column's first ncells centroids in rank order."""
    C, Lqc = S.shape
    cell = np.zeros(C, dtype=bool)
    for j in range(Lqc):
        cell[order(S[:, j])[:ncells]] = True
    return cell


def keep_of(S, threshold):
    """bool [C]: max_j S[c][j] >= threshold; a NaN in the row makes the maximum NaN and the comparison false."""
    with np.errstate(invalid="ignore"):
        return np.max(S, axis=1) >= np.float32(threshold)


def _chain(v):
    s = np.float32(0.0)
    for x in v:
        s = np.float32(s + np.float32(x))
    return s


def approx_score(S, codes, keep=None):
    """sum_j max(-9999, max over the rows `codes` (those with keep[code], if given) of S[code][j]), columns in sequence."""
    rows = codes if keep is None else codes[keep[codes]]
    m = np.full(S.shape[1], MASKED, dtype=np.float32)
    if len(rows):
        with np.errstate(invalid="ignore"):
            m = np.maximum(m, np.max(S[rows], axis=0))          # np.max / np.maximum: a NaN sticks
    return _chain(m)


def prune(S, codes, mask, lengths, ncells, threshold, ndocs):
    """One query.  S float32 [C, Lq_coarse]; codes / mask over the rows of the passages back to back (mask None: all ones).
    dict(cells bool [C], keep bool [C], a1, a2 float32 [n] (-inf: no candidate), list1, list2: passage indices in order)."""
    S = np.asarray(S, dtype=np.float32)
    codes = np.asarray(codes, dtype=np.int64)
    mask = np.ones(len(codes), dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    n = len(lengths)
    cell, keep = cells_of(S, ncells), keep_of(S, threshold)
    a1 = np.full(n, NEG_INF, dtype=np.float32)
    a2 = np.full(n, NEG_INF, dtype=np.float32)
    row0 = 0
    for p, ln in enumerate(lengths):
        live = codes[row0:row0 + ln][mask[row0:row0 + ln]]      # masked rows contribute nothing at any stage
        row0 += ln
        if len(live) and cell[live].any():
            a1[p] = approx_score(S, live, keep)
            a2[p] = approx_score(S, live)
    list1 = order(a1, [p for p in range(n) if a1[p] != NEG_INF])[:ndocs]
    list2 = order(a2, [p for p in list1 if a2[p] != NEG_INF])[:ndocs // 4]
    return dict(cells=cell, keep=keep, a1=a1, a2=a2, list1=list1, list2=list2)


def final(list2, exact, k):
    """The first k of the stage-2 survivors by their exact score (exact: float32 [n], indexed by passage); -inf is absent."""
    return order(exact, [p for p in list2 if exact[p] != NEG_INF])[:k]
