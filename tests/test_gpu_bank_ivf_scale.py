"""GPU: the inverted file (rr_bank_build_ivf, csrc/bank_ivf.hip) and the search that reads it (rr_bank_search_plaid_ivf, the
inverted-file form of csrc/bank_search_plaid.hip) at the bank and centroid sizes the benchmark runs, against float64.

tests/test_gpu_bank_ivf.py holds the file to its definition on a bank of 5 000 passages and 400 centroids, and the search to the scan
form where the longest list times Lq_coarse * ncells reaches the range, so that both forms share their row layout (cap == n).  Here:
  the six cases of tests/plaid_exact_cases.py   257 .. 262 144 centroids: ivf_scan_kernel at 1, 16 and 256 centroids a thread and at
           counts no multiple of 1024, ivf_sort_kernel as a grid of 262 144 workgroups, 280 cell entries a query
  wide     cap < n: compact rows whose pitch is not the range and whose entries are places; 40 007 passages: ivf_compact_kernel's
           second round, alone (a query whose candidates all lie from passage 32 768 on) and after the first; a range; 16 queries
  narrow   cap below ndocs / 4 and below k
  strided  more than 8 192 candidates in rows of 8 192 < cap < n: plaid_score_listed_kernel's second trip; control: cap == n
  edges    lists of 0, 1, 2, 3, 255, 256, 257, 4 095, 4 096, 4 097, 9 000 and 5 000 entries; three rebuilt lists on one bitmap
  million  a list above 4096 x 256 entries: ivf_list_bits_kernel's grid stride; 33 rounds of the compaction
The file read back equals the numpy restatement of tests/plaid_ivf_exact_cases.py, two builds give equal bytes.  The search equals
the float64 oracle's final list and exact scores AND rr_bank_search_plaid bit for bit, poisoned outputs included, and in the same
test the scan form's taps are held to the oracle, so a disagreement says which form is wrong.  The cap conditions are asserted here
from rr_bank_ivf_info, so a fixture that stops biting fails.  tests/test_plaid_ivf_exact_cases_cpu.py shows the rest on the oracle
alone.  No tolerance anywhere."""
import numpy as np
import pytest
import torch

import plaid_exact_cases as X
import plaid_ivf_exact_cases as V
from test_gpu_bank_ivf import _both, _outputs, _raw, _read_raw
from test_gpu_bank_search_plaid import _check_result, _codec
from test_gpu_bank_search_plaid_scale import _bank as _exact_bank
from test_gpu_bank_search_plaid_scale import _run_and_check
from test_gpu_li_scores import _engine as _bare_engine

pytestmark = pytest.mark.gpu

_BANKS = {}


def _bank(name):
    """(engine, bank) of a bank of V.BANKS, built once."""
    if name not in _BANKS:
        from rmr_amd import PlaidCodec
        b = V.bank(name)
        eng = _bare_engine(b["D"])
        lens = b["lens"]
        bank = eng.create_bank(sum(lens) + 4, len(lens) + 1, codec=PlaidCodec(b["centroids"], b["weights"], b["nbits"]))
        bank.add_compressed(range(len(lens)), b["codes"], b["residuals"], lens, mask=b["mask"])
        _BANKS[name] = (eng, bank)
    return _BANKS[name]


def _plain_bank(name, D=64):
    """(engine, bank, (codes, mask, lens, C)) of a build-only bank of V: any codec, residual bytes of zero."""
    if name not in _BANKS:
        codes, mask, lens, C = getattr(V, name)()
        eng = _bare_engine(D)
        codec = _codec(D, 1, C)
        bank = eng.create_bank(len(codes) + 4, len(lens) + 1, codec=codec)
        bank.add_compressed(range(len(lens)), codes, np.zeros((len(codes), codec.residual_bytes), dtype=np.uint8), lens, mask=mask)
        _BANKS[name] = (eng, bank, (codes, mask, lens, C))
    return _BANKS[name]


def _check_file(bank, codes, mask, lens, C):
    """Build twice; the file read back into poisoned buffers, and what rr_bank_ivf_info says, against the restatement."""
    want_off, want_pids = V.ivf_fast(codes, mask, lens, C)
    lengths = np.diff(want_off)
    info = bank.build_ivf()
    off, pids, raw_info = _read_raw(bank)
    bad = np.flatnonzero(off != want_off)
    assert bad.size == 0, f"offsets differ at {bad[:5].tolist()}: {off[bad[:5]].tolist()} for {want_off[bad[:5]].tolist()}"
    assert pids.shape == want_pids.shape
    bad = np.flatnonzero(pids != want_pids)
    lists = np.unique(np.searchsorted(want_off, bad, side="right") - 1)
    assert bad.size == 0, (f"{bad.size} pids differ, first at {bad[:5].tolist()}: {pids[bad[:5]].tolist()} for {want_pids[bad[:5]].tolist()}; "
                           f"lists {lists[:8].tolist()} of lengths {lengths[lists[:8]].tolist()}")
    assert info == raw_info == dict(passages_covered=len(lens), postings=int(want_off[-1]), longest_list=int(lengths.max()))
    bank.build_ivf()
    again_off, again_pids, again_info = _read_raw(bank)
    assert np.array_equal(again_off, off) and np.array_equal(again_pids, pids) and again_info == raw_info, "two builds"
    return info


def _search(case, want, eng, bank, first=0, count=None):
    """The scan form's taps and result against the oracle; the inverted-file form equal to the scan form bit for bit on poisoned
    outputs, and to the oracle's final list and the float64 exact scores."""
    n = len(case["lens"]) - first if count is None else count
    q = torch.from_numpy(case["queries"]).cuda()
    exact = case["exact"][:, first:first + n]
    _run_and_check(eng, bank, case, q, want, case["S"], exact, first=first, count=n)
    gi, gs, gc = _both(eng, bank, q, case["k"], Lqc=case["Lqc"], ncells=case["ncells"], thr=case["threshold"], ndocs=case["ndocs"],
                       first=first, n=n)
    _check_result(dict(indices=gi, scores=gs, counts=gc), want, exact, case["k"], add=first)
    return gi, gs, gc


# ---- the six exact cases of the scan form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(X.CASES))
def test_the_file_and_the_search_on_the_exact_cases_of_the_scan_form(name):
    case, want = X.get(name)
    eng, bank = _exact_bank(name)
    info = _check_file(bank, case["codes"], case["mask"], case["lens"], case["C"])
    cap, n = V.cap_of(case, info["longest_list"]), len(case["lens"])
    assert cap < n if name == "c262144" else cap == n, "c262144 alone (2 cell entries a query) has compact rows below the range"
    _search(case, want, eng, bank)


def test_a_range_on_an_exact_case_of_the_scan_form():
    name, first = "c1000", 6
    case, _ = X.get(name)
    count = len(case["lens"]) - first - 5
    eng, bank = _exact_bank(name)
    bank.build_ivf()
    gi, _, _ = _search(case, X.oracle(case, first, count), eng, bank, first, count)
    assert int(gi.min()) >= first and int(gi.max()) < first + count


# ---- cap < n ---------------------------------------------------------------------------------------------------------------------------
def test_the_file_of_the_big_bank():
    b = V.bank("big")
    info = _check_file(_bank("big")[1], b["codes"], b["mask"], b["lens"], b["C"])
    assert info["longest_list"] <= V.IVF_SORT_MAX, "every list of this bank is sorted in LDS"


def test_wide_compact_rows_narrower_than_the_range():
    case, want = V.get("wide")
    eng, bank = _bank("big")
    n, cap = len(case["lens"]), V.cap_of(case, bank.build_ivf()["longest_list"])
    assert case["ndocs"] < cap < n and n > 32 * V.COMPACT_WORDS and n % 32
    assert max(int((w["a1"] != -np.inf).sum()) for w in want) > 4096
    _search(case, want, eng, bank)


def test_wide_over_a_range_off_the_bitmap_words():
    first, count = 37, 39901
    case, _ = V.get("wide")
    eng, bank = _bank("big")
    cap = V.cap_of(case, bank.build_ivf()["longest_list"], count)
    assert case["ndocs"] < cap < count and first % 32 and count % 32 and count > 32 * V.COMPACT_WORDS
    gi, _, _ = _search(case, X.oracle(case, first, count), eng, bank, first, count)
    assert int(gi.min()) >= first and int(gi.max()) < first + count


def test_wide_sixteen_queries_in_one_call_equal_sixteen_calls():
    case, _ = V.get("wide")
    eng, bank = _bank("big")
    bank.build_ivf()
    q = torch.from_numpy(V.sixteen_queries()).cuda()
    k = case["k"]
    kw = dict(Lqc=case["Lqc"], ncells=case["ncells"], thr=case["threshold"], ndocs=case["ndocs"])
    gi, gs, gc = _both(eng, bank, q, k, **kw)
    assert gc.tolist() == [k] * 16
    for qi in range(16):
        one = _outputs(1, k)
        assert _raw("rr_bank_search_plaid_ivf", eng, bank, q[qi:qi + 1], one, k, **kw) == 0
        torch.cuda.synchronize()
        assert torch.equal(one[0][0], gi[qi]) and torch.equal(one[1][0].view(torch.int32), gs[qi].view(torch.int32)) and one[2][0] == gc[qi]


@pytest.mark.parametrize("name", ["strided", "control"])
def test_strided_more_candidates_than_one_trip_of_the_listed_scores(name):
    case, want = V.get(name)
    eng, bank = _bank("big")
    n, cap = len(case["lens"]), V.cap_of(case, bank.build_ivf()["longest_list"])
    assert int((want[0]["a1"] != -np.inf).sum()) > V.LISTED_TRIP
    assert V.LISTED_TRIP < cap < n if name == "strided" else cap == n
    _search(case, want, eng, bank)


@pytest.mark.parametrize("name", ["narrow", "narrow_k"])
def test_narrow_compact_rows_shorter_than_the_lists_of_the_later_stages(name):
    case, want = V.get(name)
    eng, bank = _bank("narrow")
    b = V.bank("narrow")
    info = _check_file(bank, b["codes"], b["mask"], b["lens"], b["C"])
    cap = V.cap_of(case, info["longest_list"])
    assert cap < case["ndocs"] // 4 < len(case["lens"]) and (cap < case["k"]) == (name == "narrow_k")
    _, _, gc = _search(case, want, eng, bank)
    if name == "narrow_k":
        assert int(gc.max()) < case["k"]


# ---- the build alone -------------------------------------------------------------------------------------------------------------------
def test_edges_list_lengths_around_every_boundary_of_the_build():
    _, bank, (codes, mask, lens, C) = _plain_bank("edges")
    info = _check_file(bank, codes, mask, lens, C)
    assert info["longest_list"] == max(V.EDGE_LISTS.values()) > 2 * V.IVF_SORT_MAX
    _, lengths = bank.ivf()
    assert {c: int(lengths[c]) for c in V.EDGE_LISTS} == V.EDGE_LISTS


def test_million_a_list_longer_than_one_pass_of_its_bitmap_kernel():
    eng, bank, (codes, mask, lens, C) = _plain_bank("million")
    info = _check_file(bank, codes, mask, lens, C)
    assert info["longest_list"] == V.P_MILLION > 4096 * 256
    cen = bank.codec.centroids[V.EVERYWHERE].float()
    gen = torch.Generator().manual_seed(5)
    q = torch.nn.functional.normalize(cen[None, None] + 0.3 * torch.randn(1, 4, cen.shape[0], generator=gen) / 8.0, dim=-1).cuda()
    gi, gs, gc = _both(eng, bank, q, 16, Lqc=2, ncells=1, thr=0.3, ndocs=64)
    assert gc.tolist() == [16] and int(gi.max()) < V.P_MILLION
