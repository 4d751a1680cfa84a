"""CPU: the host side of the PLAID-pruned bank search (rr_bank_search_plaid, include/rerank_mi355.h).

1. rr_util_plaid_prune, the contract's cells / candidates / stage 1 / stage 2 in the library's host code, equals
   tests/plaid_search_ref.py (the same contract in numpy) EXACTLY on crafted inputs: few distinct scores so that ties sit at
   every cut, duplicate passages, masked rows, a fully masked passage, a passage whose codes all lie below the threshold, fewer
   candidates than ndocs / ndocs // 4, ndocs no multiple of 4, ncells 1 and ncells = n_centroids, NaN and -inf in S.
2. plaid_search_ref against what the reference's own get_cells / colbert_score_reduce gave (tests/golden/plaid_search_ref.npz,
   made by tests/golden/make_plaid_search_fixture.py): sets exactly, scores within 1e-4 (the reference's .sum may add in another
   order; the maker asserts that no cut is decided within 1e-3).
3. The Python surface on stub engines: argument checks before the library, counts / -1 handling, id mapping, PlaidSearch
   defaults, retrieve_and_rerank handing unequal lists to forward_passages, and plaid=None calling exactly what it called before.
No device."""
import os

import numpy as np
import pytest
import torch

import plaid_search_ref as ref
from rmr_amd import BankTable, InteractionRerankModel, PassageBank, PlaidSearch, RerankEngine
from rmr_amd import _lib as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plaid_search_ref.npz")


def _prune_lib(S, codes, mask, lengths, ncells, thr, ndocs):
    lib = L.load()
    S = np.ascontiguousarray(S, dtype=np.float32)
    C, Lqc = S.shape
    n = len(lengths)
    codes = np.ascontiguousarray(codes, dtype=np.int32)
    lens = np.ascontiguousarray(lengths, dtype=np.int32)
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    cells = np.full(C, 7, dtype=np.uint8)
    a1, a2 = np.full(n, 5.5, dtype=np.float32), np.full(n, 5.5, dtype=np.float32)
    l1, l2 = np.full(min(ndocs, n), -7, dtype=np.int32), np.full(min(ndocs // 4, n), -7, dtype=np.int32)
    n1, n2 = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    rc = lib.rr_util_plaid_prune(S.ctypes.data, C, Lqc, codes.ctypes.data, None if m is None else m.ctypes.data, lens.ctypes.data, n,
                                 ncells, thr, ndocs, cells.ctypes.data, a1.ctypes.data, a2.ctypes.data, l1.ctypes.data, n1.ctypes.data,
                                 l2.ctypes.data, n2.ctypes.data)
    assert rc == 0, rc
    assert (l1[int(n1[0]):] == -7).all() and (l2[int(n2[0]):] == -7).all(), "nothing is written behind a list's length"
    return dict(cells=cells.astype(bool), a1=a1, a2=a2, list1=l1[:int(n1[0])].tolist(), list2=l2[:int(n2[0])].tolist())


def _same(S, codes, mask, lengths, ncells, thr, ndocs):
    got = _prune_lib(S, codes, mask, lengths, ncells, thr, ndocs)
    want = ref.prune(S, codes, mask, lengths, ncells, thr, ndocs)
    assert np.array_equal(got["cells"], want["cells"])
    for k in ("a1", "a2"):
        assert np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), f"{k}: {got[k]} for {want[k]}"
    assert got["list1"] == want["list1"] and got["list2"] == want["list2"]
    return want


def _crafted(seed, C=12, Lqc=5, n=40, max_len=9):
    """S on a grid of 0.25 (ties in every column and between passages), passages of 1 .. max_len rows from few codes, every
    third passage stored twice, interior masked rows, passage 3 fully masked."""
    rng = np.random.default_rng(seed)
    S = (rng.integers(-2, 4, size=(C, Lqc)) * 0.25).astype(np.float32)
    lens, codes, mask = [], [], []
    for p in range(n):
        if p % 3 == 2:                                           # a duplicate of the passage before it: an exact tie, other index
            lens.append(lens[-1]); codes.append(codes[-1].copy()); mask.append(mask[-1].copy())
            continue
        ln = int(rng.integers(1, max_len + 1))
        lens.append(ln)
        codes.append(rng.integers(0, C, size=ln))
        m = np.ones(ln, dtype=np.uint8)
        m[2::3] = 0
        if p == 3:
            m[:] = 0
        mask.append(m)
    return S, np.concatenate(codes), np.concatenate(mask), lens


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("ncells,thr,ndocs", [(1, 0.5, 8), (2, 0.25, 10), (3, 0.75, 16), (12, -1.0, 1024), (1, 0.5, 4), (2, 2.0, 9)])
def test_prune_equals_the_numpy_restatement_exactly(seed, ncells, thr, ndocs):
    S, codes, mask, lens = _crafted(seed)
    w = _same(S, codes, mask, lens, ncells, thr, ndocs)
    assert np.isneginf(w["a1"][3]) and 3 not in w["list1"], "a fully masked passage is never a candidate"
    if ncells == 12:                                             # every centroid is a cell: every passage with an unmasked row
        assert int(np.isfinite(w["a1"]).sum()) == len(lens) - 1 and len(w["list1"]) == len(lens) - 1
        assert len(w["list2"]) == len(lens) - 1                  # fewer candidates than ndocs and than ndocs // 4
    if thr == 2.0:                                               # no centroid reaches the threshold
        cand = np.isfinite(w["a1"])
        assert cand.any() and (w["a1"][cand] == np.float32(S.shape[1] * -9999.0)).all()
        assert w["list1"] == sorted(w["list1"]), "all-equal scores keep index order"
    _same(S, codes, None, lens, ncells, thr, ndocs)              # mask NULL = all ones


def test_the_crafted_cases_have_ties_at_the_cuts():
    """What makes the comparison above bite: at both cuts the last kept and the first dropped passage tie, so that only the index
    decides, in at least one crafted case each; and duplicates sit next to each other in the lists."""
    cut1 = cut2 = dup = 0
    for seed in range(6):
        S, codes, mask, lens = _crafted(seed)
        for ncells, thr, ndocs in [(1, 0.5, 8), (2, 0.25, 10), (3, 0.75, 16), (1, 0.5, 4)]:
            w = ref.prune(S, codes, mask, lens, ncells, thr, ndocs)
            full1 = ref.order(w["a1"], [p for p in range(len(lens)) if w["a1"][p] != ref.NEG_INF])
            if len(full1) > ndocs and w["a1"][full1[ndocs - 1]] == w["a1"][full1[ndocs]]:
                cut1 += 1
            full2 = ref.order(w["a2"], w["list1"])
            if len(full2) > ndocs // 4 and w["a2"][full2[ndocs // 4 - 1]] == w["a2"][full2[ndocs // 4]]:
                cut2 += 1
            for i, p in enumerate(w["list1"][:-1]):
                if p % 3 == 1 and w["list1"][i + 1] == p + 1:
                    dup += 1
    assert cut1 and cut2 and dup, (cut1, cut2, dup)


def test_below_threshold_passage_nan_and_inf():
    # centroid 2 tops column 0 with 0.5 (a cell at ncells 1) but lies below the threshold 0.75; centroid 0 passes it
    S = np.array([[0.25, 1.0, 0.0], [0.0, 0.5, 0.25], [0.5, 0.0, 0.0], [0.0, 0.0, 0.75]], dtype=np.float32)
    lens = [2, 1, 3, 1]
    codes = [2, 2, 1, 0, 2, 3, 3]                                # passage 0: only the below-threshold code; 1: code 1 (no cell at 0.75?)
    w = _same(S, codes, None, lens, 1, 0.75, 4)
    assert w["cells"].tolist() == [True, False, True, True]      # column tops: 2, 0, 3
    assert w["a1"][0] == np.float32(3 * -9999.0) and w["a2"][0] == np.float32(0.5)
    assert np.isneginf(w["a1"][1]) and np.isneginf(w["a2"][1])   # code 1 lies in no cell
    assert w["list1"] == [2, 3, 0] and w["list2"] == [2]         # ndocs // 4 = 1
    # a NaN ranks first in its column and sticks in a maximum; a row of S with a NaN is not kept; -inf A1 means absent
    S2 = S.copy()
    S2[1, 2] = np.nan
    w = _same(S2, codes, None, lens, 1, 0.25, 8)
    assert w["cells"][1] and not w["keep"][1] and np.isnan(w["a2"][1]) and w["list2"][0] == 1
    S3 = np.full((4, 3), -np.inf, dtype=np.float32)
    w = _same(S3, codes, None, lens, 4, 0.0, 8)
    assert (w["a1"] == np.float32(3 * -9999.0)).all() and w["list1"] == [0, 1, 2, 3]
    lib = L.load()
    bad = np.array([4], dtype=np.int32)
    one = np.array([1], dtype=np.int32)
    assert lib.rr_util_plaid_prune(S.ctypes.data, 4, 3, bad.ctypes.data, None, one.ctypes.data, 1, 1, 0.0, 4, *([None] * 7)) == L.RR_ERR_BAD_SHAPE
    assert lib.rr_util_plaid_prune(S.ctypes.data, 4, 3, one.ctypes.data, None, one.ctypes.data, 1, 5, 0.0, 4, *([None] * 7)) == L.RR_ERR_BAD_SHAPE


# ---- 2. the numpy restatement against the reference's own numbers --------------------------------------------------------------
def test_restatement_against_the_recorded_reference():
    z = np.load(GOLDEN)
    codes, lens = z["codes"], z["doclens"].tolist()
    assert z["centroids"].shape == (64, 64) and z["Q"].shape == (32, 64) and len(lens) == 60 and min(lens) == 1 and max(lens) == 70
    for ci, (ncells, thr, ndocs) in enumerate(z["configs"].tolist()):
        ncells, ndocs = int(ncells), int(ndocs)
        S = z[f"c{ci}/S"]
        assert np.allclose(S, z["centroids"].astype(np.float32) @ z["Q"].T, atol=1e-6)
        w = ref.prune(S, codes, None, lens, ncells, thr, ndocs)
        assert np.flatnonzero(w["cells"]).tolist() == z[f"c{ci}/cells"].tolist()
        cand = z[f"c{ci}/candidates"]
        assert np.flatnonzero(w["a1"] != ref.NEG_INF).tolist() == cand.tolist() and 0 < len(cand) < len(lens)
        for k in ("a1", "a2"):
            err = np.abs(w[k][cand].astype(np.float64) - z[f"c{ci}/{k}"].astype(np.float64)).max()
            print(f"config {ci} {k}: max |difference| {err:.3e}")
            assert err <= 1e-4, (ci, k, err)
        assert sorted(w["list1"]) == z[f"c{ci}/survivors1"].tolist() and len(w["list1"]) == ndocs < len(cand)
        assert sorted(w["list2"]) == z[f"c{ci}/survivors2"].tolist() and len(w["list2"]) == ndocs // 4


# ---- 3. the Python surface -------------------------------------------------------------------------------------------------------
class _StubBank:
    def __init__(self, n, n_centroids=64):
        self.table = BankTable()
        self.table.append([f"id{i}" for i in range(n)], [1] * n)
        self.h = None
        self.codec = None if n_centroids is None else type("Codec", (), {"n_centroids": n_centroids})()

    def __len__(self):
        return len(self.table)


class _StubEngine:
    arch = {"li_dim": 64}
    device = "cpu"
    bank_search_plaid = RerankEngine.bank_search_plaid

    @property
    def lib(self):
        raise AssertionError("the call reached the library")


def test_python_argument_checks_refuse_before_the_library():
    eng, bank = _StubEngine(), _StubBank(2000)
    q = torch.zeros(2, 8, 64)
    ok = dict(ncells=2, centroid_score_threshold=0.45, ndocs=1024)
    for bad_q in (torch.zeros(2, 8, 32), torch.zeros(8, 64), torch.zeros(0, 8, 64), torch.zeros(2, 0, 64)):
        with pytest.raises(ValueError):
            eng.bank_search_plaid(bank, bad_q, 1, **ok)
    with pytest.raises(NotImplementedError, match="fp16 bank"):
        eng.bank_search_plaid(_StubBank(10, None), q, 1, **ok)
    for k in (0, -1, 257):
        with pytest.raises(ValueError, match="k ="):
            eng.bank_search_plaid(bank, q, k, **ok)
    with pytest.raises(ValueError, match="k = 11"):
        eng.bank_search_plaid(bank, q, 11, first=5, count=10, **ok)
    with pytest.raises(ValueError, match="k = 3"):
        eng.bank_search_plaid(bank, q, 3, ncells=1, centroid_score_threshold=0.0, ndocs=11)      # 11 // 4 = 2
    for ndocs, exc in ((3, ValueError), (0, ValueError), (1025, NotImplementedError)):
        with pytest.raises(exc, match="ndocs"):
            eng.bank_search_plaid(bank, q, 1, ncells=1, centroid_score_threshold=0.0, ndocs=ndocs)
    for ncells, exc in ((0, ValueError), (65, ValueError), (17, NotImplementedError)):
        with pytest.raises(exc, match="ncells"):
            eng.bank_search_plaid(bank, q, 1, ncells=ncells, centroid_score_threshold=0.0, ndocs=64)
    with pytest.raises(ValueError, match="ncells = 9"):
        eng.bank_search_plaid(_StubBank(10, 8), q, 1, ncells=9, centroid_score_threshold=0.0, ndocs=64)
    for coarse in (0, 9):
        with pytest.raises(ValueError, match="coarse_tokens"):
            eng.bank_search_plaid(bank, q, 1, coarse_tokens=coarse, **ok)
    for first, count in ((-1, None), (2000, None), (0, 0), (1, 2000)):
        with pytest.raises(ValueError, match="holds 2000"):
            eng.bank_search_plaid(bank, q, 1, first=first, count=count, **ok)
    with pytest.raises(AssertionError, match="reached the library"):
        eng.bank_search_plaid(bank, q, 256, coarse_tokens=8, **ok)                               # what is right goes on


def test_plaid_search_defaults_follow_the_reference():
    for k in (1, 10, 100):
        p = PlaidSearch.defaults(k)
        assert (p.ncells, p.centroid_score_threshold, p.ndocs, p.coarse_tokens) == (2, 0.45, 1024, None)
    assert PlaidSearch.defaults(50, coarse_tokens=32).coarse_tokens == 32
    with pytest.raises(NotImplementedError, match="4096"):
        PlaidSearch.defaults(101)
    with pytest.raises(ValueError):
        PlaidSearch.defaults(0)


class _Recorder:
    """An engine whose two searches return given results and record what they were asked."""

    def __init__(self, indices, counts=None):
        self.indices, self.calls = torch.tensor(indices, dtype=torch.int32), []
        self.counts = None if counts is None else torch.tensor(counts, dtype=torch.int32)

    def _scores(self):
        return torch.arange(self.indices.numel(), dtype=torch.float32).reshape(self.indices.shape)

    def bank_search(self, bank, query_li, k, first=0, count=None):
        self.calls.append(("exact", bank, k, first, count))
        return dict(indices=self.indices, scores=self._scores())

    def bank_search_plaid(self, bank, query_li, k, **kw):
        self.calls.append(("plaid", bank, k, kw))
        return dict(indices=self.indices, scores=self._scores(), counts=self.counts)


def _bank(ids):
    bank = PassageBank.__new__(PassageBank)
    bank.table = BankTable()
    bank.table.append(ids, [1] * len(ids))
    return bank


def test_search_with_plaid_maps_ids_and_cuts_at_the_counts():
    bank = _bank(["a", ("c", 3), 7, "e"])
    q = torch.zeros(3, 5, 64)
    eng = _Recorder([[3, 0, 1], [1, -1, -1], [-1, -1, -1]], [3, 1, 0])
    plaid = PlaidSearch(2, 0.45, 16, coarse_tokens=4)
    ids, scores = bank.search(eng, q, 3, first=0, count=4, plaid=plaid)
    assert ids == [["e", "a", ("c", 3)], [("c", 3)], []] and scores.shape == (3, 3)
    assert eng.calls == [("plaid", bank, 3, dict(ncells=2, centroid_score_threshold=0.45, ndocs=16, coarse_tokens=4, first=0, count=4))]
    exact = _Recorder([[3, 0], [1, 2], [0, 1]])
    bank.search(exact, q, 2)                                     # plaid=None: exactly the call it made before
    bank.search(exact, q, 2, plaid=None, first=1, count=2)
    assert exact.calls == [("exact", bank, 2, 0, None), ("exact", bank, 2, 1, 2)]


def test_retrieve_and_rerank_hand_unequal_lists_to_forward_passages():
    m = InteractionRerankModel.__new__(InteractionRerankModel)
    torch.nn.Module.__init__(m)
    m.bank = _bank(["a", "b", "c", "d"])
    seen = {}

    def forward_passages(q, qm, passage_ids, num_negative_examples, **kw):
        seen.clear()
        seen.update(ids=passage_ids, neg=num_negative_examples, kw=kw)
        return "output"
    m.forward_passages = forward_passages
    q, qm = torch.zeros(2, 5, 64), torch.ones(2, 5)
    plaid = PlaidSearch(1, 0.5, 12)
    m.engine = _Recorder([[2, 0, 1], [3, -1, -1]], [3, 1])
    ids, scores = m.retrieve(q, 3, plaid=plaid)
    assert ids == [["c", "a", "b"], ["d"]] and m.engine.calls[-1][0] == "plaid"
    got, out = m.retrieve_and_rerank(q, qm, 3, plaid=plaid, fusion_from_li=True)
    assert got == ids and out == "output"
    assert seen == dict(ids=["c", "a", "b", "d"], neg=2, kw=dict(candidates_per_query=[3, 1], fusion_from_li=True))
    m.engine = _Recorder([[2, 0, 1], [-1, -1, -1]], [3, 0])
    with pytest.raises(ValueError, match="query 1 found no candidate"):
        m.retrieve_and_rerank(q, qm, 3, plaid=plaid)
    m.engine = _Recorder([[2, 0, 1], [3, 1, 0]])
    ids, _ = m.retrieve(q, 3)                                    # plaid=None: the exhaustive search, called as before
    got, _ = m.retrieve_and_rerank(q, qm, 3, plaid=None, fusion_from_li=True)
    assert got == ids == [["c", "a", "b"], ["d", "b", "a"]]
    assert [c[0] for c in m.engine.calls] == ["exact", "exact"] and m.engine.calls[0][2:] == (3, 0, None)
    assert seen == dict(ids=["c", "a", "b", "d", "b", "a"], neg=2, kw=dict(fusion_from_li=True))
    m.bank = None
    with pytest.raises(RuntimeError, match="create_bank"):
        m.retrieve(q, 1, plaid=plaid)
