"""CPU: the host side of the candidate filters of the bank searches ("CANDIDATE FILTERS", include/rerank_mi355.h): the bitmap
rr_bank_filter_fill writes, through its host restatement rr_util_bank_filter_bits, against a numpy packing
(tests/bank_filter_ref.py); PassageBank.filter_lists / filter / search(filter=) and InteractionRerankModel.retrieve on host tables
and stub engines; the numpy restatement of the filtered exact order on crafted scores.  No device."""
import numpy as np
import pytest
import torch

import bank_filter_ref as ref
from rmr_amd import BankFilter, BankTable, InteractionRerankModel, PassageBank, _lib as L

POISON = np.uint32(0xDEADBEEF)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return L.load()


def _host_bits(lib, rows, passages, exclude, ld=None, extra=2):
    """rr_util_bank_filter_bits into a poisoned buffer with `extra` words more than it may write: (rc, bits [rows, ld], tail)."""
    ld = ref.words(passages) if ld is None else ld
    idx = np.ascontiguousarray(np.concatenate([np.asarray(r, dtype=np.int32) for r in rows]) if rows else np.zeros(0, np.int32))
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    out = np.full(len(rows) * ld + extra, POISON, dtype=np.uint32)
    rc = lib.rr_util_bank_filter_bits(idx.ctypes.data if idx.size else None, off.ctypes.data, len(rows), int(exclude), passages,
                                      out.ctypes.data, ld)
    return rc, out[:len(rows) * ld].reshape(len(rows), ld), out[len(rows) * ld:]


@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("nrows", [1, 3])
@pytest.mark.parametrize("passages", [1, 31, 32, 33, 4097])
def test_host_bitmap_equals_the_numpy_packing(lib, passages, nrows, exclude):
    rng = np.random.default_rng(1000 * passages + 10 * nrows + exclude)
    rows = [rng.integers(0, passages, size=max(1, passages // 3)).tolist() for _ in range(nrows)]      # (with repeats)
    rows[0] = rows[0] + rows[0][:2] + [passages - 1, 0]           # duplicates, the last and the first passage
    if nrows == 3:
        rows[1] = []                                              # an empty row: nothing allowed / nothing excluded
    for ld in (ref.words(passages), ref.words(passages) + 3):     # a wider pitch: the words behind the bank are written as zeros
        rc, bits, tail = _host_bits(lib, rows, passages, exclude, ld)
        assert rc == 0 and (tail == POISON).all()
        want = ref.pack_bits(rows, passages, exclude, ld)
        assert np.array_equal(bits, want), np.argwhere(bits != want)[:4].tolist()
        on = ref.bit_rows(bits, ld * 32)
        assert not on[:, passages:].any(), "bits at or beyond the passage count are zero in both modes"
        for r, lst in enumerate(rows):
            assert on[r, :passages].sum() == (passages - len(set(lst)) if exclude else len(set(lst)))


def test_host_bitmap_refusals_write_nothing(lib):
    def refused(rows, passages, exclude=0, ld=None, offsets=None):
        ld = ref.words(max(passages, 1)) if ld is None else ld
        idx = np.ascontiguousarray(np.concatenate([np.asarray(r, dtype=np.int32) for r in rows]))
        off = np.asarray(offsets if offsets is not None else np.concatenate([[0], np.cumsum([len(r) for r in rows])]), dtype=np.int64)
        out = np.full(64, POISON, dtype=np.uint32)
        rc = lib.rr_util_bank_filter_bits(idx.ctypes.data, off.ctypes.data, len(off) - 1, exclude, passages, out.ctypes.data, ld)
        assert (out == POISON).all(), "a refused call writes nothing"
        return rc
    for exclude in (0, 1):
        assert refused([[0, 40]], 40, exclude) == L.RR_ERR_BAD_SHAPE              # an index at the passage count
        assert refused([[3], [-1]], 40, exclude) == L.RR_ERR_BAD_SHAPE            # a negative index, in the second row
        assert refused([[1, 2, 3]], 40, exclude, offsets=[0, 2, 1, 3]) == L.RR_ERR_BAD_SHAPE      # offsets descend
        assert refused([[1, 2, 3]], 40, exclude, offsets=[1, 3]) == L.RR_ERR_BAD_SHAPE            # offsets do not start at 0
        assert refused([[1]], 33, exclude, ld=1) == L.RR_ERR_BAD_SHAPE            # 33 passages take two words
        assert refused([[0]], 0, exclude) == L.RR_ERR_BAD_SHAPE
    off = np.zeros(2, dtype=np.int64)
    assert lib.rr_util_bank_filter_bits(None, off.ctypes.data, 1, 0, 8, None, 1) == L.RR_ERR_BAD_ARG
    assert lib.rr_util_bank_filter_bits(None, None, 1, 0, 8, off.ctypes.data, 1) == L.RR_ERR_BAD_ARG


def _bank(ids):
    bank = PassageBank.__new__(PassageBank)                       # the host table alone: no device store behind it
    bank.table = BankTable()
    bank.table.append(ids, [1] * len(ids))
    return bank


def test_filter_arguments_flat_and_nested(lib):
    bank = _bank(["a", ("c", 3), 7, "e", "f"])
    for kw in ({}, dict(allowed=["a"], excluded=["e"])):
        with pytest.raises(ValueError, match="exactly one"):
            bank.filter_lists(**kw)
        with pytest.raises(ValueError, match="exactly one"):
            bank.filter(**kw)                                     # refused before anything touches the device
    with pytest.raises(KeyError, match="'zz'"):
        bank.filter_lists(allowed=["a", "zz"])
    with pytest.raises(KeyError, match="'zz'"):
        bank.filter(excluded=[["a"], ["zz"]])
    idx, off, exclude = bank.filter_lists(allowed=["e", ("c", 3), "e"])          # flat: one row; a tuple is an id
    assert idx.dtype == np.int32 and off.dtype == np.int64 and (idx.tolist(), off.tolist(), exclude) == ([3, 1, 3], [0, 3], False)
    idx, off, exclude = bank.filter_lists(excluded=[["a"], [], [7, ("c", 3)]])   # nested: a row per query, one of them empty
    assert (idx.tolist(), off.tolist(), exclude) == ([0, 2, 1], [0, 1, 1, 3], True)
    idx, off, exclude = bank.filter_lists(allowed=[])                            # nothing allowed: one empty row
    assert (idx.tolist(), off.tolist(), exclude) == ([], [0, 0], False)
    # the lists are what the library takes: through the host restatement they give the bitmap of the ids
    idx, off, exclude = bank.filter_lists(excluded=[["a"], [], [7, ("c", 3)]])
    out = np.zeros((3, 1), dtype=np.uint32)
    assert lib.rr_util_bank_filter_bits(idx.ctypes.data, off.ctypes.data, 3, int(exclude), len(bank.table), out.ctypes.data, 1) == 0
    assert out[:, 0].tolist() == [0b11110, 0b11111, 0b11001]


class _Recorder:
    """An engine whose filtered searches return given results and record what they were asked."""

    def __init__(self, indices, counts):
        self.indices, self.counts, self.calls = torch.tensor(indices, dtype=torch.int32), torch.tensor(counts, dtype=torch.int32), []

    def _result(self, name, bank, k, filter, **kw):
        self.calls.append((name, k, filter, kw))
        return dict(indices=self.indices, scores=torch.zeros(self.indices.shape), counts=self.counts)

    def bank_search(self, *a, **kw):
        raise AssertionError("the unfiltered search was called")

    def bank_search_filtered(self, bank, q, k, filter, **kw):
        return self._result("exact", bank, k, filter, **kw)

    def bank_search_plaid_filtered(self, bank, q, k, filter, **kw):
        return self._result("plaid", bank, k, filter, **kw)

    def bank_search_plaid_ivf_filtered(self, bank, q, k, filter, **kw):
        return self._result("ivf", bank, k, filter, **kw)


def test_search_with_a_filter_refuses_a_stale_one_and_returns_true_lengths():
    from rmr_amd import PlaidSearch
    bank = _bank(["a", "b", "c", "d", "e"])
    eng = _Recorder([[3, 0, -1], [-1, -1, -1]], [2, 0])
    q = torch.zeros(2, 5, 64)
    stale = BankFilter(None, 1, 4)                                # built when the bank held four passages
    with pytest.raises(ValueError, match="built for 4 passages"):
        bank.search(eng, q, 3, filter=stale)
    with pytest.raises(ValueError, match="built for 4 passages"):
        bank.search(eng, q, 3, first=2, count=3, filter=stale)
    assert eng.calls == []
    ids, _ = bank.search(eng, q, 3, first=1, count=3, filter=stale)              # a range the old filter still covers
    assert ids == [["d", "a"], []], "a query's list has its true length on the exact path too"
    fresh = BankFilter(None, 1, 5)
    bank.search(eng, q, 3, filter=fresh)
    bank.search(eng, q, 3, filter=fresh, plaid=PlaidSearch(2, 0.4, 16))
    bank.search(eng, q, 3, filter=fresh, plaid=PlaidSearch(2, 0.4, 16, ivf=True))
    assert [c[0] for c in eng.calls] == ["exact", "exact", "plaid", "ivf"] and all(c[2] is fresh for c in eng.calls[1:])
    assert eng.calls[2][3] == dict(ncells=2, centroid_score_threshold=0.4, ndocs=16, coarse_tokens=None, first=0, count=None)


def test_retrieve_takes_a_filter_and_rerank_refuses_an_empty_list():
    m = InteractionRerankModel.__new__(InteractionRerankModel)
    torch.nn.Module.__init__(m)
    m.bank = _bank(["a", "b", "c", "d"])
    m.engine = _Recorder([[2, 0, -1], [3, -1, -1]], [2, 1])
    f = BankFilter(None, 2, 4)
    q, qm = torch.zeros(2, 5, 64), torch.ones(2, 5)
    with pytest.raises(ValueError, match="not both"):
        m.retrieve(q, 3, allowed=["a"], filter=f)
    ids, _ = m.retrieve(q, 3, filter=f)
    assert ids == [["c", "a"], ["d"]] and m.engine.calls[-1][2] is f
    seen = {}

    def forward_passages(q, qm, passage_ids, num_negative_examples, **kw):
        seen.update(ids=passage_ids, neg=num_negative_examples, kw=kw)
        return "output"
    m.forward_passages = forward_passages
    got_ids, out = m.retrieve_and_rerank(q, qm, 3, filter=f)
    assert got_ids == ids and out == "output" and seen == dict(ids=["c", "a", "d"], neg=2, kw=dict(candidates_per_query=[2, 1]))
    m.engine = _Recorder([[2, 0, -1], [-1, -1, -1]], [2, 0])
    with pytest.raises(ValueError, match="query 1 found no candidate"):
        m.retrieve_and_rerank(q, qm, 3, filter=f)


def test_the_numpy_restatement_of_the_filtered_order():
    inf, nan = np.inf, np.nan
    s = np.array([[1.0, nan, 3.0, 3.0, -inf, 0.0, -0.0, 2.0],
                  [5.0, 4.0, nan, nan, 1.0, 1.0, -inf, inf]], dtype=np.float32)
    assert ref.rank_order(s[0]).tolist() == [1, 2, 3, 7, 0, 5, 6, 4]             # NaN first, ties (+0 == -0) by index, -inf last
    assert ref.rank_order(s[1]).tolist() == [2, 3, 7, 0, 1, 4, 5, 6]
    every = np.ones((1, 8), dtype=bool)
    idx, sc, cnt = ref.filtered_topk(s, every, 8, first=10)
    assert idx.tolist() == [[11, 12, 13, 17, 10, 15, 16, -1], [12, 13, 17, 10, 11, 14, 15, -1]] and cnt.tolist() == [7, 7]
    assert np.isneginf(sc[:, 7]).all() and np.isnan(sc[0, 0]), "a genuine -inf counts as absent"
    per_query = np.array([[0, 0, 1, 1, 1, 0, 1, 0], [0] * 8], dtype=bool)
    idx, sc, cnt = ref.filtered_topk(s, per_query, 3)
    assert idx.tolist() == [[2, 3, 6], [-1, -1, -1]] and cnt.tolist() == [3, 0] and np.isneginf(sc[1]).all()
    idx, sc, cnt = ref.filtered_topk(s, per_query[:1], 5)                        # one shared row, k above what it allows
    assert idx.tolist() == [[2, 3, 6, -1, -1], [2, 3, 4, -1, -1]] and cnt.tolist() == [3, 3]
    assert sc[1, 2] == 1.0 and np.isnan(sc[1, :2]).all()
