"""CPU: THE INVERTED FILE of a compressed bank (include/rerank_mi355.h) in the library's host code, rr_util_plaid_ivf, against a
numpy restatement written here: per centroid, np.unique of the passages of the unmasked rows with that code.  Exact equality.
Fixtures: a passage holding one code in every row; a passage whose rows are all masked (it appears in no list); a centroid no row
uses (an empty list, equal neighbouring offsets); codes at 0 and C - 1; one centroid present in every passage.  Then the Python
surface on stubs: PlaidSearch(ivf=True) takes the new entry, the default the old one.  No device."""
import numpy as np
import pytest

from rmr_amd import BankTable, PassageBank, PlaidSearch
from rmr_amd import _lib as L


def ivf_numpy(codes, mask, lengths, C):
    """(offsets int64 [C + 1], pids int32): the definition, restated."""
    codes = np.clip(np.asarray(codes, dtype=np.int64), 0, C - 1)
    pid = np.repeat(np.arange(len(lengths)), lengths)
    live = np.ones(len(codes), dtype=bool) if mask is None else np.asarray(mask) != 0
    lists = [np.unique(pid[live & (codes == c)]) for c in range(C)]
    offsets = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    return offsets, (np.concatenate(lists) if offsets[-1] else np.zeros(0)).astype(np.int32)


def ivf_lib(codes, mask, lengths, C):
    """rr_util_plaid_ivf: first sized with pids_out NULL, then filled."""
    lib = L.load()
    import ctypes
    codes = np.ascontiguousarray(codes, dtype=np.int32)
    lens = np.ascontiguousarray(lengths, dtype=np.int32)
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    mp = None if m is None else m.ctypes.data
    offsets = np.full(C + 1, -7, dtype=np.int64)
    total = ctypes.c_int64(-1)
    assert lib.rr_util_plaid_ivf(codes.ctypes.data, mp, lens.ctypes.data, len(lens), C, offsets.ctypes.data, None, 0, ctypes.byref(total)) == 0
    assert total.value == offsets[C] >= 0
    pids = np.full(total.value + 3, -7, dtype=np.int32)
    again = np.full(C + 1, -7, dtype=np.int64)
    assert lib.rr_util_plaid_ivf(codes.ctypes.data, mp, lens.ctypes.data, len(lens), C, again.ctypes.data, pids.ctypes.data, total.value,
                                 None) == 0
    assert np.array_equal(again, offsets) and (pids[total.value:] == -7).all(), "nothing is written behind the postings"
    if total.value:                                                       # too small a buffer is refused and left alone
        small = np.full(total.value, -7, dtype=np.int32)
        assert lib.rr_util_plaid_ivf(codes.ctypes.data, mp, lens.ctypes.data, len(lens), C, again.ctypes.data, small.ctypes.data,
                                     total.value - 1, None) == L.RR_ERR_BAD_SHAPE
        assert (small == -7).all()
    return offsets, pids[:total.value]


def fixture_bank(seed=0, C=11, n=30, max_len=9):
    """The fixtures in one bank.  Passage 2 holds code 4 in every row; passage 3 is fully masked; centroid 5 is used by no row;
    passage 0 has codes 0 and C - 1; centroid 4 is present in every passage (its last row; in passage 3 under a masked row)."""
    rng = np.random.default_rng(seed)
    usable = np.array([c for c in range(C) if c != 5])
    lens, codes, mask = [], [], []
    for p in range(n):
        ln = int(rng.integers(3, max_len + 1))
        c = usable[rng.integers(0, len(usable), size=ln)]
        m = np.ones(ln, dtype=np.uint8)
        if p % 2:
            m[1::3] = 0                                                   # interior masked rows
        if p == 0:
            c[0], c[1] = 0, C - 1
        if p == 2:
            c[:] = 4
        c[-1] = 4
        m[-1] = 1
        if p == 3:
            m[:] = 0
        lens.append(ln); codes.append(c); mask.append(m)
    return np.concatenate(codes), np.concatenate(mask), lens, C


@pytest.mark.parametrize("seed", range(4))
def test_the_host_definition_equals_the_numpy_restatement(seed):
    codes, mask, lens, C = fixture_bank(seed)
    offsets, pids = ivf_lib(codes, mask, lens, C)
    want_off, want_pids = ivf_numpy(codes, mask, lens, C)
    assert np.array_equal(offsets, want_off) and np.array_equal(pids, want_pids)
    n = len(lens)
    lst = lambda c: pids[offsets[c]:offsets[c + 1]].tolist()
    assert offsets[5] == offsets[6], "a centroid no row uses: an empty list"
    assert 3 not in pids.tolist(), "a fully masked passage appears in no list"
    assert lst(4) == [p for p in range(n) if p != 3], "one centroid in every passage with an unmasked row"
    assert [c for c in range(C) if 2 in lst(c)] == [4], "one code in every row: one list"
    assert 0 in lst(0) and 0 in lst(C - 1)
    for c in range(C):
        assert lst(c) == sorted(set(lst(c))), f"list {c} ascending, every passage once"


def test_no_mask_counts_every_row_and_codes_are_clamped():
    codes, mask, lens, C = fixture_bank(5)
    offsets, pids = ivf_lib(codes, None, lens, C)
    want_off, want_pids = ivf_numpy(codes, None, lens, C)
    assert np.array_equal(offsets, want_off) and np.array_equal(pids, want_pids) and 3 in pids.tolist()
    wild = codes.copy()
    wild[::4] = -3
    wild[1::4] = C + 9
    offsets, pids = ivf_lib(wild, mask, lens, C)
    want_off, want_pids = ivf_numpy(wild, mask, lens, C)
    assert np.array_equal(offsets, want_off) and np.array_equal(pids, want_pids)


def test_one_passage_one_row_and_everything_masked():
    offsets, pids = ivf_lib([2], None, [1], 4)
    assert offsets.tolist() == [0, 0, 0, 1, 1] and pids.tolist() == [0]
    offsets, pids = ivf_lib([2, 1, 1], [0, 0, 0], [1, 2], 4)
    assert offsets.tolist() == [0, 0, 0, 0, 0] and pids.size == 0
    lib = L.load()
    off = np.zeros(5, dtype=np.int64)
    bad = np.array([0], dtype=np.int32)
    one = np.array([1], dtype=np.int32)
    assert lib.rr_util_plaid_ivf(one.ctypes.data, None, bad.ctypes.data, 1, 4, off.ctypes.data, None, 0, None) == L.RR_ERR_BAD_SHAPE
    assert lib.rr_util_plaid_ivf(None, None, one.ctypes.data, 1, 4, off.ctypes.data, None, 0, None) == L.RR_ERR_BAD_ARG


class _StubEngine:
    def __init__(self):
        self.calls = []

    def _result(self, name, nq, k, kw):
        import torch
        self.calls.append((name, kw))
        return dict(indices=torch.tensor([[1, 0, -1]] * nq, dtype=torch.int32)[:, :k], scores=torch.zeros(nq, k),
                    counts=torch.tensor([2] * nq, dtype=torch.int32))

    def bank_search_plaid(self, bank, q, k, **kw):
        return self._result("scan", q.shape[0], k, kw)

    def bank_search_plaid_ivf(self, bank, q, k, **kw):
        return self._result("ivf", q.shape[0], k, kw)


def test_plaid_search_ivf_flag_picks_the_entry_and_the_default_is_the_scan():
    import torch
    bank = PassageBank.__new__(PassageBank)
    bank.table = BankTable()
    bank.table.append(["a", "b"], [3, 4])
    bank.h = None
    eng, q = _StubEngine(), torch.zeros(2, 4, 8)
    assert PlaidSearch(2, 0.4, 16).ivf is False and PlaidSearch.defaults(10).ivf is False
    assert PlaidSearch.defaults(10, ivf=True).ivf is True and "ivf=True" in repr(PlaidSearch(2, 0.4, 16, ivf=True))
    assert "ivf" not in repr(PlaidSearch(2, 0.4, 16))
    ids, _ = bank.search(eng, q, 3, plaid=PlaidSearch(2, 0.4, 16, coarse_tokens=3))
    ids2, _ = bank.search(eng, q, 3, plaid=PlaidSearch(2, 0.4, 16, coarse_tokens=3, ivf=True), first=0, count=2)
    assert ids == ids2 == [["b", "a"], ["b", "a"]]
    assert [c[0] for c in eng.calls] == ["scan", "ivf"]
    assert eng.calls[0][1] == dict(ncells=2, centroid_score_threshold=0.4, ndocs=16, coarse_tokens=3, first=0, count=None)
    assert eng.calls[1][1] == dict(ncells=2, centroid_score_threshold=0.4, ndocs=16, coarse_tokens=3, first=0, count=2)
