"""CPU: the host side of the list-driven filtered exact search (rr_bank_search_filtered_sparse; "CANDIDATE FILTERS",
include/rerank_mi355.h): the entry and its two diagnostic operators are exported and bound, and `sparse=True` on
PassageBank.search / search_bank_part / search_banks / InteractionRerankModel.retrieve / retrieve_and_rerank reaches
RerankEngine.bank_search_filtered_sparse while the default reaches bank_search_filtered with the keywords it always had.  Stub
engines, as in tests/test_bank_filter_cpu.py.  No device."""
import ctypes as C

import pytest
import torch

from rmr_amd import BankFilter, InteractionRerankModel, PlaidSearch, _lib as L
from rmr_amd.passage_bank import search_bank_part, search_banks
from test_bank_filter_cpu import _Recorder, _bank


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return L.load()


def test_the_entry_and_its_operators_are_exported_and_bound(lib):
    P = C.c_void_p
    want = {
        "rr_bank_search_filtered_sparse": [P, P, P, C.c_int, C.c_int, C.c_int32, C.c_int32, C.c_int, P, C.c_int, C.c_int64, P, P, P, P],
        "rr_op_filter_compact": [P, C.c_int, C.c_int64, C.c_int32, C.c_int32, P, P, P],
        "rr_op_topk_select_counted": [P, C.c_int, C.c_int, P, P, C.c_int, C.c_int, C.c_int32, P, P, P, P],
    }
    for name, args in want.items():
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == args, name
    # the sparse entry takes what the dense entry takes, argument for argument
    assert list(lib.rr_bank_search_filtered_sparse.argtypes) == list(lib.rr_bank_search_filtered.argtypes)
    # no handle, no operand: refused on the host before a device is looked at
    assert lib.rr_bank_search_filtered_sparse(None, None, None, 1, 1, 0, 1, 1, None, 1, 1, None, None, None, None) == L.RR_ERR_BAD_ARG
    assert lib.rr_op_filter_compact(None, 1, 1, 0, 1, None, None, None) == L.RR_ERR_BAD_ARG
    assert lib.rr_op_topk_select_counted(None, 1, 1, None, None, 1, 1, 0, None, None, None, None) == L.RR_ERR_BAD_ARG


class _Both(_Recorder):
    """_Recorder with the list-driven entry beside the dense one."""

    def bank_search_filtered_sparse(self, bank, q, k, filter, **kw):
        return self._result("sparse", bank, k, filter, **kw)


def test_sparse_reaches_the_list_driven_entry_and_the_default_the_dense_one():
    bank = _bank(["a", "b", "c", "d", "e"])
    eng = _Both([[3, 0, -1], [-1, -1, -1]], [2, 0])
    q = torch.zeros(2, 5, 64)
    f = BankFilter(None, 1, 5)
    ids, _ = bank.search(eng, q, 3, first=1, count=3, filter=f, sparse=True)
    assert ids == [["d", "a"], []], "true list lengths, as on the dense path"
    assert eng.calls == [("sparse", 3, f, dict(first=1, count=3))]
    bank.search(eng, q, 3, first=1, count=3, filter=f)
    bank.search(eng, q, 3, filter=f, sparse=False)
    assert eng.calls[1:] == [("exact", 3, f, dict(first=1, count=3)), ("exact", 3, f, dict(first=0, count=None))], "today's keywords only"


def test_sparse_without_a_filter_or_with_plaid_raises_and_calls_nothing():
    class _Nothing:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was reached")
    bank = _bank(["a", "b", "c", "d", "e"])
    eng, q, f = _Nothing(), torch.zeros(2, 5, 64), BankFilter(None, 1, 5)
    plaid = PlaidSearch(2, 0.4, 16)
    with pytest.raises(ValueError, match="sparse=True needs a filter"):
        bank.search(eng, q, 3, sparse=True)
    with pytest.raises(ValueError, match="sparse=True with plaid"):
        bank.search(eng, q, 3, filter=f, plaid=plaid, sparse=True)
    with pytest.raises(ValueError, match="sparse=True needs a filter"):
        search_bank_part(eng, bank, q, 3, sparse=True)
    with pytest.raises(ValueError, match="sparse=True with plaid"):
        search_bank_part(eng, bank, q, 3, plaid, f, sparse=True)
    with pytest.raises(ValueError, match="sparse=True needs a filter"):
        search_banks(eng, [bank, bank], q, 3, sparse=True)
    with pytest.raises(ValueError, match="sparse=True needs a filter"):
        search_banks(eng, [bank, bank], q, 3, filters=[f, None], sparse=True)
    with pytest.raises(ValueError, match="sparse=True with plaid"):
        search_banks(eng, [bank, bank], q, 3, plaid=plaid, filters=[f, f], sparse=True)
    m = InteractionRerankModel.__new__(InteractionRerankModel)
    torch.nn.Module.__init__(m)
    m.bank, m.engine = bank, eng
    qm = torch.ones(2, 5)
    with pytest.raises(ValueError, match="sparse=True needs"):
        m.retrieve(q, 3, sparse=True)
    with pytest.raises(ValueError, match="sparse=True with plaid"):
        m.retrieve(q, 3, filter=f, plaid=plaid, sparse=True)
    with pytest.raises(ValueError, match="sparse=True needs"):
        m.retrieve_and_rerank(q, qm, 3, sparse=True)
    with pytest.raises(ValueError, match="sparse=True needs"):
        m.retrieve_and_rerank(q, qm, 3, filter=f, plaid=plaid, sparse=True)


def test_a_stale_filter_raises_on_the_sparse_path_as_on_the_dense_one():
    bank = _bank(["a", "b", "c", "d", "e"])
    bank.generation = 2
    eng = _Both([[3, 0, -1], [-1, -1, -1]], [2, 0])
    q = torch.zeros(2, 5, 64)
    for sparse in (False, True):
        with pytest.raises(ValueError, match="built for 4 passages"):
            bank.search(eng, q, 3, filter=BankFilter(None, 1, 4, 2), sparse=sparse)
        with pytest.raises(ValueError, match="built at generation 1"):
            bank.search(eng, q, 3, filter=BankFilter(None, 1, 5, 1), sparse=sparse)
    assert eng.calls == []
    bank.search(eng, q, 3, first=1, count=3, filter=BankFilter(None, 1, 4, 2), sparse=True)      # a range the old filter still covers
    assert [c[0] for c in eng.calls] == ["sparse"]


def test_search_bank_part_takes_sparse_and_keeps_its_default_call():
    bank = _bank(["a", "b", "c"])
    eng = _Both([[2, 0, -1], [1, -1, -1]], [2, 1])
    eng.device = torch.device("cpu")
    q, f = torch.zeros(2, 5, 64), BankFilter(None, 1, 3)
    r = search_bank_part(eng, bank, q, 3, None, f, sparse=True)
    assert r["counts"].tolist() == [2, 1]
    search_bank_part(eng, bank, q, 3, None, f)
    assert eng.calls == [("sparse", 3, f, {}), ("exact", 3, f, {})]


def test_retrieve_and_rerank_sparse_hands_on_true_list_lengths():
    m = InteractionRerankModel.__new__(InteractionRerankModel)
    torch.nn.Module.__init__(m)
    m.bank = _bank(["a", "b", "c", "d"])
    m.engine = _Both([[2, 0, -1], [3, -1, -1]], [2, 1])
    f = BankFilter(None, 2, 4)
    q, qm = torch.zeros(2, 5, 64), torch.ones(2, 5)
    ids, _ = m.retrieve(q, 3, filter=f, sparse=True)
    assert ids == [["c", "a"], ["d"]] and m.engine.calls == [("sparse", 3, f, dict(first=0, count=None))]
    m.retrieve(q, 3, filter=f)
    assert m.engine.calls[-1] == ("exact", 3, f, dict(first=0, count=None))
    seen = {}

    def forward_passages(q, qm, passage_ids, num_negative_examples, **kw):
        seen.update(ids=passage_ids, neg=num_negative_examples, kw=kw)
        return "output"
    m.forward_passages = forward_passages
    got_ids, out = m.retrieve_and_rerank(q, qm, 3, filter=f, sparse=True)
    assert m.engine.calls[-1][0] == "sparse"
    assert got_ids == ids and out == "output" and seen == dict(ids=["c", "a", "d"], neg=2, kw=dict(candidates_per_query=[2, 1]))
    m.engine = _Both([[2, 0, -1], [-1, -1, -1]], [2, 0])
    with pytest.raises(ValueError, match="query 1 found no candidate"):
        m.retrieve_and_rerank(q, qm, 3, filter=f, sparse=True)
