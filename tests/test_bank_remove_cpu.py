"""CPU: the plan of rr_bank_remove in the library's host code, rr_util_bank_remove_plan (include/rerank_mi355_diag.h; the function
rr_bank_remove itself calls), replayed in numpy on an array of row ids: the result is the survivors' rows back to back, no window
exceeds the staging block, a window's destination ends below every source of every later window, and the passages in front of
the first removed one give no move.  Then the refusals, and the host table (BankTable.remove).  Exact equality; no device."""
import ctypes

import numpy as np
import pytest

from bank_remove_cases import REMOVAL_SETS, plan, removal_set, replay, survivors_rows
from rmr_amd import BankTable
from rmr_amd import _lib as L

LENGTHS = (1, 2, 3, 17, 64, 130)
WINDOWS = (1, 7, 64, 10**9)


def length_lists():
    rng = np.random.default_rng(20)
    counts = [1, 2, 3, 5, 8, 13, 21, 34, 47, 60]
    return [rng.choice(LENGTHS, size=n).astype(np.int32) for n in counts]


@pytest.mark.parametrize("window_rows", WINDOWS)
@pytest.mark.parametrize("which", REMOVAL_SETS)
def test_the_plan_replayed_gives_the_survivors_back_to_back(which, window_rows):
    for lengths in length_lists():
        n = len(lengths)
        remove = removal_set(which, n)
        rc, new_index, moves = plan(lengths, remove, window_rows)
        assert rc == 0
        gone = set(remove)
        want_index = np.full(n, -1, dtype=np.int32)
        want_index[[p for p in range(n) if p not in gone]] = np.arange(n - len(gone))
        assert np.array_equal(new_index, want_index)
        want = survivors_rows(lengths, remove)
        got = replay(lengths, moves, window_rows)
        assert np.array_equal(got[:len(want)], want)
        first = np.concatenate([[0], np.cumsum(lengths)])
        prefix_rows = int(first[min(gone)]) if gone else int(first[-1])
        assert len(moves) == 0 or int(moves[:, 2].min()) == prefix_rows, "the unmoved prefix gives no move; the first move starts behind it"
        assert int(moves[:, 3].sum()) == len(want) - min(prefix_rows, len(want)), "every surviving row behind the prefix moves once"
        if moves.shape[0] > 1:
            shift = moves[:, 1] - moves[:, 2]
            assert (np.diff(shift) >= 0).all(), "the shift never decreases"
        if which == "none" or which == "last":
            assert len(moves) == 0


def test_runs_are_maximal_at_an_unbounded_window():
    """One window: the moves are the runs, one per block of adjacent survivors behind the first removed passage."""
    lengths = np.array([3, 1, 2, 17, 64, 2, 1, 130, 3], dtype=np.int32)
    rc, new_index, moves = plan(lengths, [1, 5, 6], 10**9)
    assert rc == 0 and new_index.tolist() == [0, -1, 1, 2, 3, -1, -1, 4, 5]
    assert moves.tolist() == [[0, 4, 3, 83], [0, 90, 86, 133]]
    rc, _, moves = plan(lengths, [1, 5, 6], 50)
    assert rc == 0 and moves.tolist() == [[0, 4, 3, 50], [1, 54, 53, 33], [1, 90, 86, 17], [2, 107, 103, 50], [3, 157, 153, 50], [4, 207, 203, 16]]


def test_refusals_write_nothing():
    lengths = np.array([3, 1, 2, 17], dtype=np.int32)
    for bad in ([1, 1], [-1], [4], [0, 2, 0]):
        assert plan(lengths, bad, 7)[0] == L.RR_ERR_BAD_SHAPE
    assert plan(lengths, [1], 0)[0] == L.RR_ERR_BAD_SHAPE
    assert plan(np.array([3, 0, 2], dtype=np.int32), [0], 7)[0] == L.RR_ERR_BAD_SHAPE
    lib = L.load()
    rc, new_index, moves = plan(lengths, [0], 2)
    assert rc == 0 and len(moves) == 10
    rem = np.array([0], dtype=np.int32)
    idx = np.full(4, -7, dtype=np.int32)
    out = np.full((10, 4), -7, dtype=np.int64)
    count = ctypes.c_int64(-7)
    assert lib.rr_util_bank_remove_plan(lengths.ctypes.data, 4, rem.ctypes.data, 1, 2, idx.ctypes.data, out.ctypes.data, 9,
                                        ctypes.byref(count)) == L.RR_ERR_BAD_SHAPE
    assert (idx == -7).all() and (out == -7).all() and count.value == -7, "too small a move buffer: nothing is written"
    assert lib.rr_util_bank_remove_plan(None, 4, rem.ctypes.data, 1, 2, None, None, 0, None) == L.RR_ERR_BAD_ARG


def test_bank_table_remove():
    t = BankTable()
    t.append(["a", "b", ("c", 1), "d", "e"], [3, 1, 2, 17, 5])
    with pytest.raises(KeyError, match="'zz'"):
        t.check_remove(["a", "zz"])
    with pytest.raises(ValueError, match="twice"):
        t.check_remove(["d", "a", "d"])
    with pytest.raises(ValueError):
        t.remove([1, 1])
    with pytest.raises(IndexError):
        t.remove([5])
    assert t.ids == ["a", "b", ("c", 1), "d", "e"] and len(t) == 5, "a refusal changes nothing"
    assert t.check_remove(["d", "b"]) == [3, 1]
    assert t.remove([3, 1]) == [0, -1, 1, -1, 2]
    assert t.ids == ["a", ("c", 1), "e"] and t.lengths == [3, 2, 5] and len(t) == 3
    assert "b" not in t and "d" not in t and "e" in t
    idx, lens = t.lookup(["e", ("c", 1)])
    assert idx.tolist() == [2, 1] and lens.tolist() == [5, 2]
    with pytest.raises(KeyError, match="'b'"):
        t.lookup(["b"])
    assert t.append(["b", "f"], [4, 1]) == 3, "a removed id may be added again"
    assert t.lookup(["b"])[0].tolist() == [3] and t.ids == ["a", ("c", 1), "e", "b", "f"]
    assert t.remove([]) == [0, 1, 2, 3, 4]
    assert t.remove([0, 1, 2, 3, 4]) == [-1] * 5 and len(t) == 0 and t.index_of == {}


def test_filter_and_bank_carry_a_generation():
    from rmr_amd import BankFilter, PassageBank
    assert BankFilter(None, 1, 5).generation == 0 and BankFilter(None, 1, 5, 3).generation == 3
    assert callable(PassageBank.remove)
