"""The candidate filter of the bank searches ("CANDIDATE FILTERS", include/rerank_mi355.h) restated in numpy: the bitmap
rr_bank_filter_fill / rr_util_bank_filter_bits write, and the order rr_bank_search_filtered returns from exact scores and a
bitmap.  No device, no library."""
import numpy as np


def words(passages: int) -> int:
    return (passages + 31) // 32


def pack_bits(rows, passages: int, exclude: bool, ld=None) -> np.ndarray:
    """uint32 [len(rows), ld]: bit i & 31 of word i >> 5 of row r is set iff (i in rows[r]) != exclude and i < passages."""
    ld = words(passages) if ld is None else ld
    out = np.zeros((len(rows), ld), dtype=np.uint32)
    for r, lst in enumerate(rows):
        on = np.full(passages, bool(exclude))
        on[np.asarray(lst, dtype=np.int64)] = not exclude
        padded = np.zeros(ld * 32, dtype=bool)
        padded[:passages] = on
        out[r] = np.packbits(padded.reshape(ld, 32), axis=1, bitorder="little").view("<u4").reshape(ld)
    return out


def bit_rows(bits: np.ndarray, passages: int) -> np.ndarray:
    """bool [rows, passages] from a packed bitmap."""
    b = np.unpackbits(np.ascontiguousarray(bits).view(np.uint8).reshape(bits.shape[0], -1), axis=1, bitorder="little")
    return b[:, :passages].astype(bool)


def rank_order(scores: np.ndarray) -> np.ndarray:
    """The one rank order over a row of float32 scores: NaN first, higher score first, equal scores (+0 == -0) by ascending index."""
    s = np.asarray(scores, dtype=np.float32)
    nan = np.isnan(s)
    key = np.where(nan, np.inf, s.astype(np.float64))
    return np.lexsort((np.arange(len(s)), -key, ~nan))


def filtered_topk(scores: np.ndarray, allowed: np.ndarray, k: int, first: int = 0):
    """rr_bank_search_filtered from its definition.  scores float32 [nq, n]: the exact score of every passage of the range;
    allowed bool [1 or nq, n]: the filter's bits of the range.  The competitors of a query are its allowed passages whose score is
    not -inf, in rank order; the first k: (indices int32 [nq, k] + first, -1 behind the count; scores float32 [nq, k], -inf there;
    counts int32 [nq])."""
    nq, n = scores.shape
    idx = np.full((nq, k), -1, dtype=np.int32)
    sc = np.full((nq, k), -np.inf, dtype=np.float32)
    cnt = np.zeros(nq, dtype=np.int32)
    for q in range(nq):
        a = allowed[0 if allowed.shape[0] == 1 else q]
        order = [int(p) for p in rank_order(scores[q]) if a[p] and not np.isneginf(scores[q, p])][:k]
        cnt[q] = len(order)
        idx[q, :len(order)] = np.asarray(order, dtype=np.int32) + first
        sc[q, :len(order)] = scores[q, order]
    return idx, sc, cnt
