"""CPU: the exact cases of tests/plaid_exact_cases.py (what tests/test_gpu_bank_search_plaid_scale.py runs on the device).

1. Every case BITES, on the float64 / numpy oracle alone: the candidate set selects, both centroid-only stages cut, ties sit at the
   ncells cut of a column and at the stage-1 cut of every case that cuts, at the stage-2 and the final cut somewhere in the table,
   cells fall into the last bitmap word and into a 256-centroid block other than the first, and the exact scores reorder the
   stage-2 list.
2. rr_util_plaid_prune (the library's host code) equals the numpy restatement exactly on each case's S: centroid counts the CPU
   suite has not had (above 256, no multiple of 32, 2^18).
3. rr_util_plaid_decode_rows (host code) gives exactly the rows the builder intended from the case's codes and packed residuals.
No device."""
import numpy as np
import pytest

import plaid_exact_cases as X
import plaid_search_ref as ref
from test_plaid_search_cpu import _same

CUTS = [n for n in X.CASES if n != "c16384w"]              # c16384w: ndocs above the passage count, no cut before the final one

_case = X.get


def _tie_at(scores, full, cut):
    return len(full) > cut and scores[full[cut - 1]] == scores[full[cut]]


def _bite(case, want):
    """What the oracle's result of each query has: a list of dicts of facts."""
    P, C, Lqc, ncells, ndocs, k = len(case["lens"]), case["C"], case["Lqc"], case["ncells"], case["ndocs"], case["k"]
    facts = []
    for qi, w in enumerate(want):
        S = case["S"][qi][:, :Lqc]
        cand = [p for p in range(P) if w["a1"][p] != ref.NEG_INF]
        col_ties = 0
        for j in range(Lqc):
            o = ref.order(S[:, j])
            col_ties += bool(S[o[ncells - 1], j] == S[o[ncells], j])
        cells = np.flatnonzero(w["cells"])
        full2 = ref.order(w["a2"], w["list1"])
        fullf = ref.order(case["exact"][qi], w["list2"])
        facts.append(dict(cand=len(cand), keep=int(w["keep"].sum()), col_ties=col_ties,
                          tie1=_tie_at(w["a1"], ref.order(w["a1"], cand), ndocs), tie2=_tie_at(w["a2"], full2, ndocs // 4),
                          tief=_tie_at(case["exact"][qi], fullf, k), last_word=bool((cells >= 32 * ((C - 1) // 32)).any()),
                          far_block=bool((cells >= 256).any()), reordered=w["final"] != w["list2"][:k],
                          n1=len(w["list1"]), n2=len(w["list2"]), nf=len(w["final"])))
    return facts


@pytest.mark.parametrize("name", list(X.CASES))
def test_the_case_bites_on_the_oracle_alone(name):
    case, want = _case(name)
    P, C, ndocs, k = len(case["lens"]), case["C"], case["ndocs"], case["k"]
    facts = _bite(case, want)
    print(name, facts)
    assert any(0 < f["cand"] < P - 1 for f in facts)
    assert any(0 < f["keep"] < C for f in facts)
    assert any(f["col_ties"] for f in facts), "no column ties at the ncells cut"
    assert any(f["last_word"] for f in facts) and any(f["far_block"] for f in facts)
    assert any(f["reordered"] for f in facts), "the exact scores leave the stage-2 order as it is"
    for w in want:
        assert np.isneginf(w["a1"][case["fully_masked"]])
    if name in CUTS:
        assert any(f["cand"] > ndocs and f["n1"] == ndocs and f["n2"] == ndocs // 4 for f in facts)
        assert any(f["tie1"] for f in facts), "no tie at the stage-1 cut"
    else:
        assert ndocs > P and ndocs // 4 > P and all(f["n1"] == f["cand"] == f["n2"] for f in facts)
    assert all(f["nf"] == min(k, f["n2"]) for f in facts)


def test_ties_at_the_stage_2_and_the_final_cut_somewhere_in_the_table():
    tie2 = tief = 0
    for name in X.CASES:
        case, want = _case(name)
        for f in _bite(case, want):
            tie2 += f["tie2"]
            tief += f["tief"]
    assert tie2 >= 1 and tief >= 1, (tie2, tief)


@pytest.mark.parametrize("name", list(X.CASES))
def test_the_repeated_centroid_rows_tie_whole_rows_of_S(name):
    case, _ = _case(name)
    C, last_word = case["C"], 32 * ((case["C"] - 1) // 32)
    rep = case["repeats"]
    for src, dst in rep:
        assert np.array_equal(case["S"][:, src], case["S"][:, dst]) and src < dst < C
    assert any(s % 256 == d % 256 for s, d in rep) and any(s % 256 != d % 256 for s, d in rep)      # the cell search's stride
    assert any(s >> 8 == d >> 8 for s, d in rep) and any(s >> 8 != d >> 8 for s, d in rep)          # the bitmap kernel's workgroups
    assert any(s <= 255 < d for s, d in rep) and any(s < last_word <= d for s, d in rep)
    assert len(np.unique(case["S"])) < 200, "S is meant to hold few distinct values: ties in every column"


@pytest.mark.parametrize("name", list(X.CASES))
def test_host_prune_equals_the_numpy_restatement_on_the_case(name):
    case, want = _case(name)
    for qi in range(case["nq"]):
        w = _same(case["S"][qi][:, :case["Lqc"]], case["codes"], case["mask"], case["lens"], case["ncells"], case["threshold"], case["ndocs"])
        assert w["list1"] == want[qi]["list1"] and w["list2"] == want[qi]["list2"]


@pytest.mark.parametrize("name", list(X.CASES))
def test_host_decode_gives_the_rows_the_builder_intended(name):
    from rmr_amd import PlaidCodec
    case, _ = _case(name)
    codec = PlaidCodec(case["centroids"], case["weights"], case["nbits"])
    got = codec.decode(case["codes"], case["residuals"]).numpy()
    assert np.array_equal(got.view(np.uint16), case["decoded"].view(np.uint16))
    cen = case["centroids"][case["codes"]]
    assert (got != cen).any(axis=1).all(), "every decoded row differs from its centroid"
    assert set(np.unique(case["buckets"])) == set(range(1 << case["nbits"])) or case["nbits"] == 8
