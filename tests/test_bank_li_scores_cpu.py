"""CPU: the host planning of a retriever-score call on a passage bank (passage_bank.plan_bank_scores, the host side of
rr_bank_li_scores / RerankEngine.bank_li_scores): passage ids -> bank indices, the three ways to say which query a pair belongs
to, the default padded length, and what it refuses.  No device, no library call.  (That the symbol is declared, exported and
bound is tests/test_abi_cpu.py's table comparison.)"""
import numpy as np
import pytest

import rmr_amd
from rmr_amd import BankTable, plan_bank_scores


def _table():
    t = BankTable()
    t.append(["a", "b", ("c", 3), 7, "e"], [5, 17, 1, 64, 40])
    return t


def test_ids_become_indices_in_pair_order_with_repeats():
    t = _table()
    ids = [7, "a", 7, ("c", 3), "e", 7]
    p = plan_bank_scores(t, ids, 1, K=6)
    assert p["indices"].tolist() == [3, 0, 3, 2, 4, 3] and p["lengths"].tolist() == [64, 5, 64, 1, 40, 64]
    assert p["pair_passage"].dtype == np.int32 and p["pair_passage"].tolist() == [3, 0, 3, 2, 4, 3]
    assert p["pair_query"].dtype == np.int32 and p["pair_query"].tolist() == [0] * 6
    assert p["padded_len"] == 64                                   # the longest passage OF THE CALL ...
    assert plan_bank_scores(t, ["a", ("c", 3), "a"], 1, K=3)["padded_len"] == 5   # ... not of the bank
    assert plan_bank_scores(t, ["a", "b"], 1, K=2, padded_len=70)["padded_len"] == 70
    assert plan_bank_scores(t, ["b"], 1, K=1, padded_len=17)["padded_len"] == 17


def test_the_three_ways_to_name_the_query_of_a_pair():
    t = _table()
    ids = ["a", "b", "e", "a", 7, "b"]
    assert plan_bank_scores(t, ids, 2, K=3)["pair_query"].tolist() == [0, 0, 0, 1, 1, 1]             # as plan_bank_batch's owner
    assert plan_bank_scores(t, ids, 3, K=2)["pair_query"].tolist() == [0, 0, 1, 1, 2, 2]
    assert plan_bank_scores(t, ids, 3, list_sizes=[1, 4, 1])["pair_query"].tolist() == [0, 1, 1, 1, 1, 2]
    assert plan_bank_scores(t, ids, 5, list_sizes=[6])["pair_query"].tolist() == [0] * 6             # queries may go unused
    pq = [2, 0, 2, 1, 0, 0]                                                                           # explicit: any order
    p = plan_bank_scores(t, ids, 3, pair_query=pq)
    assert p["pair_query"].tolist() == pq and p["pair_passage"].tolist() == [0, 1, 4, 0, 3, 1]
    assert plan_bank_scores(t, ids, 3, pair_query=np.array(pq, dtype=np.int64))["pair_query"].tolist() == pq
    same = rmr_amd.plan_bank_batch(t, ids, 3, None, 64)
    assert plan_bank_scores(t, ids, 2, K=3)["pair_query"].tolist() == same["owner"].tolist()
    assert plan_bank_scores(t, ids, 2, K=3)["pair_passage"].tolist() == same["indices"].tolist()     # ... but never reordered


def test_an_unknown_id_is_a_key_error_that_names_it():
    t = _table()
    with pytest.raises(KeyError, match="'nope'"):
        plan_bank_scores(t, ["a", "nope", "b"], 1, K=3)
    with pytest.raises(KeyError, match="8"):
        plan_bank_scores(t, [7, 8], 1, K=2)


def test_what_the_planning_refuses():
    t = _table()
    ids = ["a", "b", "e", 7]
    with pytest.raises(AssertionError):
        plan_bank_scores(t, [], 1, K=1)
    with pytest.raises(AssertionError):
        plan_bank_scores(t, ids, 2)                                 # nothing says which query
    with pytest.raises(AssertionError):
        plan_bank_scores(t, ids, 2, K=2, list_sizes=[2, 2])         # two of the three
    with pytest.raises(AssertionError):
        plan_bank_scores(t, ids, 2, K=3)                            # 4 passages are not lists of 3
    with pytest.raises(AssertionError):
        plan_bank_scores(t, ids, 1, K=2)                            # lists of 2 need two queries
    with pytest.raises(AssertionError):
        plan_bank_scores(t, ids, 2, list_sizes=[3, 2])
    with pytest.raises(AssertionError):
        plan_bank_scores(t, ids, 2, list_sizes=[4, 0])
    with pytest.raises(AssertionError):
        plan_bank_scores(t, ids, 2, pair_query=[0, 1, 0])           # one index per pair
    with pytest.raises(AssertionError):
        plan_bank_scores(t, ids, 2, pair_query=[0, 1, 2, 0])        # query 2 of 2
    with pytest.raises(AssertionError):
        plan_bank_scores(t, ids, 2, pair_query=[0, -1, 1, 0])
    with pytest.raises(AssertionError):
        plan_bank_scores(t, ids, 2, K=2, padded_len=63)             # passage 7 holds 64 rows
