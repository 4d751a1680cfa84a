"""What the removal tests share (tests/test_bank_remove_cpu.py, tests/test_gpu_bank_remove.py): the removal sets, the library's plan
(rr_util_bank_remove_plan) behind a sizing call, and a numpy replay of its moves through a staging array."""
import ctypes

import numpy as np

from rmr_amd import _lib as L

REMOVAL_SETS = ("first", "last", "every_other", "middle_block", "all_but_one", "all", "none")
GPU_LENGTHS = [1, 3, 17, 64, 2, 130, 5, 33]
# on the device also the second and the third passage alone: with GPU_LENGTHS everything behind them shifts by 3 and by 17 rows
GPU_REMOVAL_SETS = REMOVAL_SETS + ("second", "third")


def removal_set(name: str, n: int) -> list:
    """The dense indices of removal set `name` for n passages (some in descending order: the call takes any order)."""
    if name == "first":
        return [0]
    if name == "last":
        return [n - 1]
    if name == "second":
        return [1]
    if name == "third":
        return [2]
    if name == "every_other":
        return list(range(0, n, 2))[::-1]
    if name == "middle_block":
        return list(range(n // 3, max(n // 3 + 1, 2 * n // 3)))
    if name == "all_but_one":
        return [i for i in range(n) if i != n // 2]
    if name == "all":
        return list(range(n - 1, -1, -1))
    if name == "none":
        return []
    raise KeyError(name)


def plan(lengths, remove, window_rows):
    """(rc, new_index int32 [n], moves int64 [n_moves, 4]) of rr_util_bank_remove_plan: sized with moves_out NULL, then filled."""
    lib = L.load()
    lens = np.ascontiguousarray(lengths, dtype=np.int32)
    rem = np.ascontiguousarray(remove, dtype=np.int32)
    n, m = len(lens), len(rem)
    new_index = np.full(n, -7, dtype=np.int32)
    n_moves = ctypes.c_int64(-7)
    rc = lib.rr_util_bank_remove_plan(lens.ctypes.data if n else None, n, rem.ctypes.data if m else None, m, int(window_rows),
                                      new_index.ctypes.data if n else None, None, 0, ctypes.byref(n_moves))
    if rc != 0:
        assert (new_index == -7).all() and n_moves.value == -7, "a refused plan writes nothing"
        return rc, None, None
    moves = np.full((n_moves.value + 1, 4), -7, dtype=np.int64)
    again = np.full(n, -7, dtype=np.int32)
    count = ctypes.c_int64(-7)
    assert lib.rr_util_bank_remove_plan(lens.ctypes.data if n else None, n, rem.ctypes.data if m else None, m, int(window_rows),
                                        again.ctypes.data if n else None, moves.ctypes.data, n_moves.value, ctypes.byref(count)) == 0
    assert count.value == n_moves.value and np.array_equal(again, new_index) and (moves[n_moves.value] == -7).all()
    return 0, new_index, moves[:n_moves.value]


def replay(lengths, moves, window_rows):
    """The moves carried out in numpy on an array of row ids, window by window through a staging array of window_rows rows, with the
    properties of the plan asserted on the way.  Returns the array (the rows behind the survivors are whatever was left there)."""
    rows = np.arange(int(np.sum(lengths)), dtype=np.int64)
    staging = np.full(min(int(window_rows), len(rows) + 1), -1, dtype=np.int64)
    windows = sorted(set(moves[:, 0].tolist()))
    assert windows == list(range(len(windows))), "windows are numbered from 0 without a gap"
    assert (np.diff(moves[:, 0]) >= 0).all(), "the moves come window by window"
    lo = np.searchsorted(moves[:, 0], windows, side="left")
    hi = np.searchsorted(moves[:, 0], windows, side="right")
    ends = []
    for w in windows:
        mv = moves[lo[w]:hi[w]]
        total = int(mv[:, 3].sum())
        assert 1 <= total <= window_rows, f"window {w} holds {total} rows, the staging block {window_rows}"
        d0 = int(mv[0, 2])
        at = 0
        for _, src, dst, cnt in mv.tolist():
            assert cnt >= 1 and dst < src and dst == d0 + at, "a move goes down, and a window's moves lie side by side"
            staging[at:at + cnt] = rows[src:src + cnt]
            at += cnt
        rows[d0:d0 + total] = staging[:total]
        ends.append((d0, d0 + total, int(mv[:, 1].min())))
    later_src = np.inf                                   # the lowest source row of every later window
    for i in range(len(ends) - 1, -1, -1):
        d0, d1, src_min = ends[i]
        assert i == 0 or d0 == ends[i - 1][1], "the windows tile the moved rows"
        assert d1 <= later_src, "a window's destination ends below every source of every later window"
        later_src = min(later_src, src_min)
    return rows


def survivors_rows(lengths, remove):
    """The row ids of the surviving passages back to back."""
    first = np.concatenate([[0], np.cumsum(lengths)])
    gone = set(remove)
    keep = [np.arange(first[p], first[p + 1]) for p in range(len(lengths)) if p not in gone]
    return np.concatenate(keep).astype(np.int64) if keep else np.zeros(0, dtype=np.int64)
