"""CPU: the host side of the bank search (rr_bank_search): BankTable.ids (dense index -> passage id) through append and clear,
what RerankEngine.bank_search refuses before it calls the library, and the id mapping of PassageBank.search /
InteractionRerankModel.retrieve / retrieve_and_rerank on stub engines.  No device, no library call.  (That the symbols are
declared, exported and bound is tests/test_abi_cpu.py's table comparison.)"""
import pytest
import torch

from rmr_amd import BankTable, InteractionRerankModel, PassageBank, RerankEngine


def test_bank_table_ids_follow_append_and_clear():
    t = BankTable()
    assert t.ids == []
    assert t.append(["a", ("c", 3)], [5, 1]) == 0
    assert t.append([7], [64]) == 2
    assert t.ids == ["a", ("c", 3), 7] and [t.index_of[p] for p in t.ids] == [0, 1, 2] and len(t.ids) == len(t)
    with pytest.raises(ValueError):
        t.append(["b", "a"], [1, 1])                              # refused as a whole: "b" is not registered either
    assert t.ids == ["a", ("c", 3), 7] and "b" not in t
    t.clear()
    assert t.ids == [] and len(t) == 0
    assert t.append([7, "a"], [2, 3]) == 0 and t.ids == [7, "a"]


class _StubBank:
    def __init__(self, n):
        self.table = BankTable()
        self.table.append([f"id{i}" for i in range(n)], [1] * n)
        self.h = None

    def __len__(self):
        return len(self.table)


class _StubEngine:
    """bank_search's checks run before the first library call: a stub without a library shows that they refuse on their own."""
    arch = {"li_dim": 64}
    device = "cpu"
    bank_search = RerankEngine.bank_search

    @property
    def lib(self):
        raise AssertionError("the call reached the library")


def test_python_argument_checks_refuse_before_the_library():
    eng, bank = _StubEngine(), _StubBank(2000)
    q = torch.zeros(2, 5, 64)
    for bad_q in (torch.zeros(2, 5, 32), torch.zeros(5, 64), torch.zeros(0, 5, 64), torch.zeros(2, 0, 64)):
        with pytest.raises(ValueError):
            eng.bank_search(bank, bad_q, 1)
    for k in (0, -1, 2001):
        with pytest.raises(ValueError, match="k ="):
            eng.bank_search(bank, q, k)
    with pytest.raises(ValueError, match="k = 11"):
        eng.bank_search(bank, q, 11, first=5, count=10)           # k is held against the range, not the bank
    with pytest.raises(NotImplementedError, match="1024"):
        eng.bank_search(bank, q, 1025)
    for first, count in ((-1, None), (2000, None), (0, 0), (1, 2000), (1999, 2), (0, -1)):
        with pytest.raises(ValueError, match="holds 2000"):
            eng.bank_search(bank, q, 1, first=first, count=count)
    with pytest.raises(AssertionError, match="reached the library"):
        eng.bank_search(bank, q, 1024, first=976)                 # what is right goes on to the library


class _Recorder:
    """An engine whose bank_search returns given indices and records what it was asked."""

    def __init__(self, indices):
        self.indices, self.calls = torch.tensor(indices, dtype=torch.int32), []

    def bank_search(self, bank, query_li, k, first=0, count=None):
        self.calls.append((bank, k, first, count))
        return dict(indices=self.indices, scores=torch.arange(self.indices.numel(), dtype=torch.float32).reshape(self.indices.shape))


def _bank(ids):
    bank = PassageBank.__new__(PassageBank)                       # the host table alone: no device store behind it
    bank.table = BankTable()
    bank.table.append(ids, [1] * len(ids))
    return bank


def test_search_maps_indices_to_the_callers_ids():
    bank = _bank(["a", ("c", 3), 7, "e"])
    eng = _Recorder([[3, 0], [1, 2]])
    q = torch.zeros(2, 5, 64)
    ids, scores = bank.search(eng, q, 2, first=0, count=4)
    assert ids == [["e", "a"], [("c", 3), 7]] and scores.tolist() == [[0.0, 1.0], [2.0, 3.0]]
    assert eng.calls == [(bank, 2, 0, 4)]
    bank.search(eng, q, 2)
    assert eng.calls[-1] == (bank, 2, 0, None)


def test_retrieve_and_rerank_hand_the_found_ids_to_forward_passages():
    m = InteractionRerankModel.__new__(InteractionRerankModel)   # no engine, no device: the two methods and a host table
    torch.nn.Module.__init__(m)
    m.bank = None
    with pytest.raises(RuntimeError, match="create_bank"):
        m.retrieve(torch.zeros(1, 5, 64), 1)
    m.bank = _bank(["a", "b", "c", "d"])
    m.engine = _Recorder([[2, 0, 1], [3, 1, 0]])
    seen = {}

    def forward_passages(q, qm, passage_ids, num_negative_examples, **kw):
        seen.update(ids=passage_ids, neg=num_negative_examples, kw=kw)
        return "output"
    m.forward_passages = forward_passages
    q, qm = torch.zeros(2, 5, 64), torch.ones(2, 5)
    ids, scores = m.retrieve(q, 3)
    assert ids == [["c", "a", "b"], ["d", "b", "a"]] and scores.shape == (2, 3)
    got_ids, out = m.retrieve_and_rerank(q, qm, 3, fusion_from_li=True)
    assert got_ids == ids and out == "output"
    assert seen == dict(ids=["c", "a", "b", "d", "b", "a"], neg=2, kw=dict(fusion_from_li=True))      # labels: forward_passages' default
