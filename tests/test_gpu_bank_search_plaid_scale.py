"""GPU: rr_bank_search_plaid (include/rerank_mi355.h, csrc/bank_search_plaid.hip) at real centroid counts, against float64.

tests/test_gpu_bank_search_plaid.py compares every stage bit for bit, at 16 and 64 centroids, on random unit vectors, with S and the
exact scores taken from the library's own kernels.  Here the inputs are the exact cases of tests/plaid_exact_cases.py: S and the
exact MaxSim are exact in float32 whatever the order of the sums, so a float64 numpy computation that calls nothing of the library
predicts every bit, and every column of S holds ties.  What only these cases reach:
  c257     a second workgroup of plaid_bitmaps_kernel that holds one centroid; 9 bitmap words, the last of 1 bit
  c300     Lq_coarse * ncells = 280 > 256 (the cell loop's second trip); C no multiple of 32 or 64; ndocs no multiple of 4
  c1000    ncells 16; 4 bitmap workgroups; a short last pseudo-passage of stage 0
  c16384   the benchmark's count; 512 bitmap words: the second trip of the scan's bitmap load
  c16384w  D 128; ndocs and ndocs / 4 above the passage count
  c262144  the accepted maximum: 64 KB of LDS in the scan, 1024 bitmap workgroups
and, on all of them, the "lower index wins" rule of plaid_cells_kernel across its 256-stride, its lanes and its waves (centroid rows
repeated at chosen indices), a range, the refusal one centroid above the maximum, and NaN / +-inf in S on the device.
tests/test_plaid_exact_cases_cpu.py shows on the oracle alone that the cases bite.  No tolerance anywhere."""
import numpy as np
import pytest
import torch

import plaid_exact_cases as X
import plaid_search_ref as ref
from test_gpu_bank_li_scores import POISON
from test_gpu_bank_search import IPOISON
from test_gpu_bank_search_plaid import LEN_CYCLE, _check_result, _exact_all, _padded, _raw
from test_gpu_li_scores import _engine as _bare_engine

pytestmark = pytest.mark.gpu

_BANKS = {}


def _bank(name):
    """(engine, bank) holding the rows of case `name`, built once."""
    if name not in _BANKS:
        from rmr_amd import PlaidCodec
        case, _ = X.get(name)
        eng = _bare_engine(case["D"])
        codec = PlaidCodec(case["centroids"], case["weights"], case["nbits"])
        lens = case["lens"]
        bank = eng.create_bank(sum(lens) + 4, len(lens) + 1, codec=codec)
        bank.add_compressed([f"p{i}" for i in range(len(lens))], case["codes"], case["residuals"], lens, mask=case["mask"])
        _BANKS[name] = (eng, bank)
    return _BANKS[name]


def _same_bits(got, want, what):
    """Bitwise, except that a NaN equals a NaN whatever its payload."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, f"{what}: {got.shape} for {want.shape}"
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN positions differ"
    bad = np.argwhere((got.view(np.int32) != want.view(np.int32)) & ~nan)
    assert bad.size == 0, f"{what} differs at {bad[:4].tolist()}: {got[tuple(bad[0])]} for {want[tuple(bad[0])]}"


def _run_and_check(eng, bank, case, q, want, S, exact, first=0, count=None):
    """One call through the handle; every tap and the result against `want` (the oracle of the range), bit for bit."""
    C, Lqc, ndocs, k, nq = case["C"], case["Lqc"], case["ndocs"], case["k"], q.shape[0]
    n = len(case["lens"]) - first if count is None else count
    k1, k2 = min(ndocs, n), min(ndocs // 4, n)
    got = eng.bank_search_plaid(bank, q, k, ncells=case["ncells"], centroid_score_threshold=case["threshold"], ndocs=ndocs, coarse_tokens=Lqc,
                                first=first, count=n)
    torch.cuda.synchronize()
    _same_bits(eng.bank_search_plaid_tap("S").reshape(nq, C, Lqc), S[:, :, :Lqc], "S")
    for key in ("cells", "keep"):
        t = eng.bank_search_plaid_tap(key).reshape(nq, C).astype(bool)
        bad = np.argwhere(t != np.stack([w[key] for w in want]))
        assert bad.size == 0, f"{key} differs at (query, centroid) {bad[:6].tolist()}"
    _same_bits(eng.bank_search_plaid_tap("a1").reshape(nq, n), np.stack([w["a1"] for w in want]), "A1")
    l1, l2 = eng.bank_search_plaid_tap("list1").reshape(nq, k1), eng.bank_search_plaid_tap("list2").reshape(nq, k2)
    w1, w2 = _padded([w["list1"] for w in want], k1), _padded([w["list2"] for w in want], k2)
    assert np.array_equal(l1, w1), f"stage-1 list: {l1.tolist()} for {w1.tolist()}"
    assert np.array_equal(l2, w2), f"stage-2 list: {l2.tolist()} for {w2.tolist()}"
    _check_result(got, want, exact, k, add=first)
    return got


@pytest.mark.parametrize("name", list(X.CASES))
def test_every_stage_against_float64(name):
    case, want = X.get(name)
    assert X.LEN_CYCLE == LEN_CYCLE
    eng, bank = _bank(name)
    _run_and_check(eng, bank, case, torch.from_numpy(case["queries"]).cuda(), want, case["S"], case["exact"])


def test_a_range_with_a_duplicate_on_each_side_of_its_start():
    name, first = "c1000", 6
    case, whole = X.get(name)
    P = len(case["lens"])
    count = P - first - 5
    d0 = case["dupes"][0]
    assert d0 < first <= case["dupes"][1] and case["n_base"] + 1 < first + count     # passage 5 lies before the range, its copy
    want = X.oracle(case, first, count)                                              # (270) and both of the pair 14 / 271 in it
    assert any(w["list1"] != [p - first for p in v["list1"]] for w, v in zip(want, whole)), "the range changes nothing"
    assert any(case["n_base"] - first in w["list1"] for w in want), "the copy of the passage before the range survives nowhere"
    eng, bank = _bank(name)
    got = _run_and_check(eng, bank, case, torch.from_numpy(case["queries"]).cuda(), want, case["S"], case["exact"][:, first:first + count],
                         first=first, count=count)
    idx = got["indices"].cpu().numpy()
    assert idx.min() >= first and idx.max() < first + count


def test_one_centroid_above_the_maximum_is_refused_and_nothing_is_written():
    from rmr_amd import PlaidCodec
    from rmr_amd import _lib as L
    D, C = 64, 262145
    eng = _bare_engine(D)
    cen = torch.zeros(C, D, dtype=torch.float16)
    cen[:, 0] = 1.0
    bank = eng.create_bank(64, 8, codec=PlaidCodec(cen, X.weights_of(1), 1))
    lens = [3, 1, 5, 2]
    bank.add_compressed(list("abcd"), np.arange(sum(lens), dtype=np.int32) * 20000, np.zeros((sum(lens), D // 8), dtype=np.uint8), lens)
    q = torch.zeros(2, 4, D, device="cuda")
    gi = torch.full((2, 2), IPOISON, device="cuda", dtype=torch.int32)
    gs = torch.full((2, 2), POISON, device="cuda")
    gc = torch.full((2,), IPOISON, device="cuda", dtype=torch.int32)
    assert _raw(eng, bank, q, gi, gs, gc, k=1) == L.RR_ERR_UNSUPPORTED
    assert b"262144" in eng.lib.rr_last_error(eng.h), eng.lib.rr_last_error(eng.h)
    with pytest.raises(NotImplementedError, match="262144"):
        eng.bank_search_plaid(bank, q, 1, ncells=1, centroid_score_threshold=0.3, ndocs=16)
    torch.cuda.synchronize()
    assert (gi == IPOISON).all() and (gs == POISON).all() and (gc == IPOISON).all()


def test_nan_and_inf_in_the_queries_reach_every_stage_as_the_contract_says():
    """Query 0: a NaN component in coarse token 3, so column 3 of S is NaN for every centroid: no row of S is kept, A1 is Lq_coarse
    times -9999 for every candidate (stage 1 is decided by the index alone), A2 and the exact score are NaN.  Query 1: +inf at a
    component where some centroids are 0 (NaN), some positive (+inf) and some negative (-inf), in coarse token 5.  Query 2: query 0
    as it was.  S .. list2 against the numpy oracle (a NaN is a NaN in any order of the sum); the exact scores of the two
    non-finite queries from rr_bank_search over the whole bank, as tests/test_gpu_bank_search_plaid.py takes them."""
    name = "c300"
    case, finite = X.get(name)
    C, Lqc, ncells, ndocs = case["C"], case["Lqc"], case["ncells"], case["ndocs"]
    cen = case["centroids"].astype(np.float64)
    q = np.stack([case["queries"][0], case["queries"][1], case["queries"][0]]).copy()
    nan_col, inf_col = 3, 5
    inf_at = next(d for d in range(case["D"]) if (cen[:, d] == 0).any() and (cen[:, d] > 0).any() and (cen[:, d] < 0).any())
    q[0, nan_col, 17] = np.nan
    q[1, inf_col, inf_at] = np.inf
    S = X.scores64(cen, q, by_element=True)
    assert np.isnan(S[0, :, nan_col]).all() and np.isfinite(np.delete(S[0], nan_col, axis=1)).all()
    col = S[1, :, inf_col]
    assert np.isnan(col).any() and np.isposinf(col).any() and np.isneginf(col).any() and np.isfinite(np.delete(S[1], inf_col, axis=1)).all()
    assert np.array_equal(S[2], case["S"][0])

    eng, bank = _bank(name)
    qd = torch.from_numpy(q).cuda()
    exact, _ = _exact_all(eng, bank, qd)
    live = np.ones(len(case["lens"]), dtype=bool)
    live[case["fully_masked"]] = False
    assert np.isnan(exact[0][live]).all(), "every passage with an unmasked row scores NaN against a query with a NaN column"
    assert np.array_equal(exact[2].view(np.int32), case["exact"][0].view(np.int32)), "the control query's exact scores: float64"
    want = X.oracle(case, S=S, exact=exact)

    w = want[0]                                                   # on the oracle alone
    assert ref.order(S[0, :, nan_col])[:ncells] == list(range(ncells)), "a NaN column's cells: the lowest indices"
    assert not w["keep"].any()
    cand = [p for p in range(len(case["lens"])) if w["a1"][p] != ref.NEG_INF]
    chain = ref._chain([ref.MASKED] * Lqc)
    assert len(cand) > ndocs and (w["a1"][cand] == chain).all() and w["list1"] == cand[:ndocs]
    assert np.isnan(w["a2"][cand]).all() and np.isnan(w["a2"][w["list2"][0]])
    w = want[1]
    assert np.isnan(w["a2"][w["list2"][0]]) and w["keep"].any() and not w["keep"][np.isnan(col)].any()
    assert np.isposinf(w["a1"]).any() or np.isnan(w["a1"]).any()
    assert want[2]["list1"] == finite[0]["list1"] and want[2]["final"] == finite[0]["final"]

    _run_and_check(eng, bank, case, qd, want, S, exact)
