"""CPU: the host side of the passage bank (passage_bank.BankTable, plan_bank_batch): ids -> indices, lengths -> segments, the
packed pair order and the per-pair query index, for uniform and unequal lists.  No device, no library call."""
import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

from rmr_amd.passage_bank import BankTable, plan_bank_batch


def _table(lengths):
    t = BankTable()
    first = t.append([f"p{i}" for i in range(len(lengths))], lengths)
    assert first == 0 and len(t) == len(lengths)
    return t


def _check_plan(plan, table, ids, owner, padded_len, granule):
    N = len(ids)
    idx = np.array([table.index_of[i] for i in ids])
    lens = np.array([table.lengths[j] for j in idx])
    assert plan["indices"].tolist() == idx.tolist() and plan["lengths"].tolist() == lens.tolist()
    assert plan["owner"].tolist() == list(owner)
    order = np.asarray(plan["order"])
    assert sorted(order.tolist()) == list(range(N)), "every pair appears once in the packed order"
    seg_n, seg_len = plan["seg_n"], plan["seg_len"]
    assert sum(seg_n) == N and all(n >= 1 for n in seg_n) and 1 <= len(seg_n) <= 64
    assert all(0 < s <= padded_len for s in seg_len) and seg_len == sorted(seg_len)
    assert plan["pair_passage"].dtype == np.int32 and plan["pair_query"].dtype == np.int32
    assert plan["pair_passage"].tolist() == idx[order].tolist()
    assert plan["pair_query"].tolist() == np.asarray(owner)[order].tolist()
    o = 0
    for n, s in zip(seg_n, seg_len):
        seg = lens[order[o:o + n]]
        assert (seg <= s).all(), "every passage fits its segment"
        # the smallest multiple of the granule (capped at the padded length) that holds it: no pair pads more than a granule
        assert (s - seg < granule).all() or s == padded_len
        assert order[o:o + n].tolist() == sorted(order[o:o + n].tolist()), "input order kept inside a segment"
        o += n


@settings(max_examples=60, deadline=None)
@given(st.lists(st.integers(1, 64), min_size=1, max_size=40), st.integers(1, 4), st.integers(1, 5), st.sampled_from([1, 8, 16]),
       st.randoms(use_true_random=False))
def test_uniform_lists(bank_lengths, Bq, K, granule, rnd):
    table = _table(bank_lengths)
    ids = [f"p{rnd.randrange(len(bank_lengths))}" for _ in range(Bq * K)]           # passages repeat, in any order
    plan = plan_bank_batch(table, ids, K, None, 64, granule)
    _check_plan(plan, table, ids, [p // K for p in range(Bq * K)], 64, granule)


@settings(max_examples=60, deadline=None)
@given(st.lists(st.integers(1, 64), min_size=1, max_size=40), st.lists(st.integers(1, 6), min_size=1, max_size=5),
       st.sampled_from([1, 8, 16]), st.randoms(use_true_random=False))
def test_unequal_lists(bank_lengths, sizes, granule, rnd):
    table = _table(bank_lengths)
    ids = [f"p{rnd.randrange(len(bank_lengths))}" for _ in range(sum(sizes))]
    plan = plan_bank_batch(table, ids, None, sizes, 64, granule)
    owner = [q for q, k in enumerate(sizes) for _ in range(k)]
    _check_plan(plan, table, ids, owner, 64, granule)


def test_a_known_batch():
    table = _table([5, 17, 33])
    plan = plan_bank_batch(table, ["p2", "p0", "p1", "p0"], 2, None, 40, 16)
    assert plan["order"].tolist() == [1, 3, 2, 0] and plan["seg_n"] == [2, 1, 1] and plan["seg_len"] == [16, 32, 40]
    assert plan["pair_passage"].tolist() == [0, 0, 1, 2] and plan["pair_query"].tolist() == [0, 1, 1, 0]
    lists = plan_bank_batch(table, ["p2", "p0", "p1", "p0"], None, [1, 3], 40, 16)
    assert lists["order"].tolist() == [1, 3, 2, 0] and lists["pair_query"].tolist() == [1, 1, 1, 0]


def test_segment_cost_merges_neighbouring_lengths():
    table = _table([3, 9, 17, 25])
    ids = ["p0", "p1", "p2", "p3"]
    fine = plan_bank_batch(table, ids, 4, None, 32, 8)
    merged = plan_bank_batch(table, ids, 4, None, 32, 8, segment_cost_rows=1000)
    assert len(fine["seg_n"]) == 4 and merged["seg_n"] == [4] and merged["seg_len"] == [32]
    _check_plan(merged, table, ids, [0] * 4, 32, 32)


def test_unknown_and_duplicate_ids():
    table = _table([4, 6])
    with pytest.raises(KeyError, match="'nope'"):
        plan_bank_batch(table, ["p0", "nope"], 2, None, 16, 8)
    with pytest.raises(KeyError, match="'nope'"):
        table.lookup(["nope"])
    with pytest.raises(ValueError, match="'p1'"):
        table.append(["p7", "p1"], [3, 3])
    with pytest.raises(ValueError, match="'p8'"):
        table.append(["p8", "p8"], [3, 3])                      # twice in one call
    assert len(table) == 2 and "p7" not in table and "p8" not in table, "a refused append changes nothing"
    assert table.append(["p7"], [3]) == 2 and table.lookup(["p7"])[0].tolist() == [2]


def test_shape_errors():
    table = _table([4, 6, 40])
    with pytest.raises(AssertionError):
        plan_bank_batch(table, ["p0", "p1", "p0"], 2, None, 16, 8)            # 3 passages are not lists of 2
    with pytest.raises(AssertionError):
        plan_bank_batch(table, ["p0", "p1"], None, [1, 0, 1], 16, 8)          # an empty list
    with pytest.raises(AssertionError):
        plan_bank_batch(table, ["p2"], 1, None, 16, 8)                        # longer than the padded context length
    table.clear()
    assert len(table) == 0 and "p0" not in table
