"""CPU: the restatement, the candidate definition and the banks of tests/plaid_ivf_exact_cases.py (what
tests/test_gpu_bank_ivf_scale.py runs on the device).

1. ivf_fast equals tests/test_bank_ivf_cpu.py's ivf_numpy on that file's fixtures and on the 5 000-passage layout of
   tests/test_gpu_bank_ivf.py, and equals rr_util_plaid_ivf (the library's host code) on every bank used here: the six cases of
   tests/plaid_exact_cases.py (257 .. 262 144 centroids), big, narrow, edges, million.
2. On every search case the sorted union of the lists of a query's cells, cut to the range, is {p : a1[p] != -inf} of the oracle.
3. Every case BITES, on the oracle and the restatement alone: the cap conditions, the bitmap rounds, the list lengths.
No device."""
import numpy as np
import pytest

import plaid_exact_cases as X
import plaid_ivf_exact_cases as V
import plaid_search_ref as ref
from test_bank_ivf_cpu import fixture_bank, ivf_lib, ivf_numpy

_FILES = {}


def _file(name):
    """(offsets, pids) of a bank by the restatement, once."""
    if name not in _FILES:
        if name in X.CASES:
            b = X.get(name)[0]
            args = (b["codes"], b["mask"], b["lens"], b["C"])
        elif name in V.BANKS:
            b = V.bank(name)
            args = (b["codes"], b["mask"], b["lens"], b["C"])
        else:
            args = getattr(V, name)()
        _FILES[name] = (args, V.ivf_fast(*args))
    return _FILES[name]


def _bank5k_layout():
    """The codes, mask and lengths of tests/test_gpu_bank_ivf.py's _bank5k, made without an engine."""
    import torch
    from test_gpu_bank_ivf import ALL_MASKED, C5K, EVERYWHERE, LONG, LONG_ROWS, P5K, UNUSED
    from test_gpu_bank_search_plaid import _topic_rows

    class Codec:
        n_centroids, residual_bytes = C5K, 16

    lens = (torch.arange(P5K) * 3 % 5 + 1).tolist()
    lens[LONG] = LONG_ROWS
    codes, _ = _topic_rows(Codec, lens, seed=P5K, topics_from=[c for c in range(C5K) if c not in (EVERYWHERE, UNUSED)])
    first = np.concatenate([[0], np.cumsum(lens)])
    mask = torch.ones(len(codes), dtype=torch.uint8)
    ten = torch.tensor([0, C5K - 1, 11, 12, 13, 200, 255, 256, 257, 300], dtype=torch.int32)
    codes[first[LONG]:first[LONG + 1]] = ten[torch.arange(LONG_ROWS) % 10]
    mask[first[LONG] + 5:first[LONG + 1]:7] = 0
    for p in range(0, P5K, 3):
        if lens[p] >= 3:
            mask[first[p] + 1] = 0
    codes[first[:-1]] = EVERYWHERE
    mask[first[:-1]] = 1
    mask[first[ALL_MASKED]:first[ALL_MASKED + 1]] = 0
    return codes.numpy(), mask.numpy(), lens, C5K


# ---- 1. the restatement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_the_fast_restatement_equals_ivf_numpy_on_the_fixture_banks(seed):
    codes, mask, lens, C = fixture_bank(seed)
    wild = codes.copy()
    wild[::4] = -3
    wild[1::4] = C + 9
    for cs, m in ((codes, mask), (codes, None), (wild, mask)):
        off, pids = V.ivf_fast(cs, m, lens, C)
        want_off, want_pids = ivf_numpy(cs, m, lens, C)
        assert off.dtype == np.int64 and pids.dtype == np.int32
        assert np.array_equal(off, want_off) and np.array_equal(pids, want_pids)


def test_the_fast_restatement_equals_ivf_numpy_on_the_5000_passage_layout():
    from test_gpu_bank_ivf import ALL_MASKED, EVERYWHERE, P5K, UNUSED
    codes, mask, lens, C = _bank5k_layout()
    off, pids = V.ivf_fast(codes, mask, lens, C)
    want_off, want_pids = ivf_numpy(codes, mask, lens, C)
    assert np.array_equal(off, want_off) and np.array_equal(pids, want_pids)
    lengths = np.diff(off)
    assert lengths[EVERYWHERE] == P5K - 1 and lengths[UNUSED] == 0 and ALL_MASKED not in pids.tolist()


ALL_BANKS = list(X.CASES) + list(V.BANKS) + ["edges", "million"]


@pytest.mark.parametrize("name", ALL_BANKS)
def test_the_host_definition_equals_the_fast_restatement(name):
    (codes, mask, lens, C), (off, pids) = _file(name)
    host_off, host_pids = ivf_lib(codes, mask, lens, C)
    assert np.array_equal(host_off, off), "offsets"
    bad = np.flatnonzero(host_pids != pids)
    assert bad.size == 0, f"pids differ at {bad[:5].tolist()}"
    lengths = np.diff(off)
    for c in np.flatnonzero(lengths > 1)[:2000]:
        assert (np.diff(pids[off[c]:off[c + 1]]) > 0).all(), f"list {c} ascending, every passage once"


# ---- 2. the candidate definition -----------------------------------------------------------------------------------------------------
def _candidates_are_the_oracles(case, want, off, pids, first=0, n=None):
    n = len(case["lens"]) - first if n is None else n
    out = []
    for qi, w in enumerate(want):
        cells = ref.cells_of(case["S"][qi][:, :case["Lqc"]], case["ncells"])
        assert np.array_equal(cells, w["cells"])
        cand = V.candidates(off, pids, cells, first, n)
        assert np.array_equal(cand, np.flatnonzero(w["a1"] != ref.NEG_INF)), f"query {qi}: the union of the lists is not the oracle's set"
        assert len(cand) <= case["Lqc"] * case["ncells"] * np.diff(off).max()
        out.append(cand)
    return out


@pytest.mark.parametrize("name", list(X.CASES))
def test_candidates_from_the_lists_are_the_oracles_on_the_six_exact_cases(name):
    case, want = X.get(name)
    _, (off, pids) = _file(name)
    cands = _candidates_are_the_oracles(case, want, off, pids)
    assert any(0 < len(c) < len(case["lens"]) for c in cands)
    cap, n = V.cap_of(case, np.diff(off).max()), len(case["lens"])
    assert cap < n if name == "c262144" else cap == n, "c262144 alone (2 cell entries a query) has compact rows below the range"
    if name == "c300":
        assert case["Lqc"] * case["ncells"] == 280
    if name == "c1000":                                        # the range of tests/test_gpu_bank_search_plaid_scale.py
        first, count = 6, len(case["lens"]) - 11
        _candidates_are_the_oracles(case, X.oracle(case, first, count), off, pids, first, count)


def _places(cand, passages):
    at = np.searchsorted(cand, passages)
    assert np.array_equal(cand[at], passages)
    return at


def test_wide_bites():
    case, want = V.get("wide")
    _, (off, pids) = _file("big")
    n, C, ndocs, k = len(case["lens"]), case["C"], case["ndocs"], case["k"]
    longest = int(np.diff(off).max())
    cap = V.cap_of(case, longest)
    assert C == 16384 and n > 32 * V.COMPACT_WORDS and n % 32 and n % 1024
    assert ndocs < cap < n and cap == case["Lqc"] * case["ncells"] * longest
    cands = _candidates_are_the_oracles(case, want, off, pids)
    print("wide: longest", longest, "cap", cap, "candidates", [len(c) for c in cands])
    assert max(len(c) for c in cands) > 4096, "two selection slices over a compact row"
    assert all(len(c) > ndocs for c in cands) and all(len(w["final"]) == k for w in want)
    assert len(cands[0]) and cands[0].min() >= 32 * V.COMPACT_WORDS, "query 0: the first round of the compaction finds nothing"
    assert any(c.min() < 32 * V.COMPACT_WORDS <= c.max() for c in cands[1:])
    for w, c in zip(want, cands):                                 # a place is not a passage
        assert (_places(c, np.array(w["list1"])) != np.array(w["list1"])).any()
    b = V.bank("big")
    assert np.isneginf(want[1]["a1"][V.FULLY_MASKED]) and b["lens"][V.LONG_PASSAGE] == 130 and set(b["lens"]) == {1, 2, 3, 4, 130}
    assert any(want[1]["a1"][d] == want[1]["a1"][b["n_base"] + j] != ref.NEG_INF for j, d in enumerate(b["dupes"])), "no tie far apart"
    assert any(any(p >= b["n_base"] for p in w["list1"]) for w in want)


@pytest.mark.parametrize("first,count", [(37, 39901)])
def test_wide_over_a_range_bites(first, count):
    case, _ = V.get("wide")
    _, (off, pids) = _file("big")
    assert first % 32 and count % 32 and count > 32 * V.COMPACT_WORDS and first + count < len(case["lens"])
    want = X.oracle(case, first, count)
    cands = _candidates_are_the_oracles(case, want, off, pids, first, count)
    cap = V.cap_of(case, np.diff(off).max(), count)
    assert case["ndocs"] < cap < count and max(len(c) for c in cands) > 4096
    whole = V.get("wide")[1]
    assert any(w["final"] != [p - first for p in v["final"]] for w, v in zip(want, whole)), "the range changes nothing"


def test_strided_and_its_control_bite():
    _, (off, pids) = _file("big")
    longest = int(np.diff(off).max())
    case, want = V.get("strided")
    n = len(case["lens"])
    cap = V.cap_of(case, longest)
    assert case["Lqc"] * case["ncells"] == 4 and longest > V.LISTED_TRIP // 4 and V.LISTED_TRIP < cap < n
    cands = _candidates_are_the_oracles(case, want, off, pids)
    print("strided: longest", longest, "cap", cap, "candidates", [len(c) for c in cands])
    assert V.LISTED_TRIP < len(cands[0]) <= cap, "the second trip of the listed scores"
    assert sorted(np.flatnonzero(want[0]["cells"]).tolist()) == sorted(V.bank("big")["hot"])
    # what the second trip scores decides the result: survivors of every stage sit behind place 8 192
    for key in ("list1", "list2", "final"):
        assert (_places(cands[0], np.array(want[0][key])) >= V.LISTED_TRIP).any(), key
    assert set(want[0]["final"]) & set(V.RICH[-11:])
    control, cwant = V.get("control")
    assert V.cap_of(control, longest) == n and control["Lqc"] * control["ncells"] == 32
    _candidates_are_the_oracles(control, cwant, off, pids)
    assert np.array_equal(control["queries"], case["queries"])


def test_narrow_bites():
    _, (off, pids) = _file("narrow")
    longest = int(np.diff(off).max())
    b = V.bank("narrow")
    assert longest == 3 and pids[off[b["three"]]:off[b["three"] + 1]].tolist() == b["holders"]
    for name in ("narrow", "narrow_k"):
        case, want = V.get(name)
        cap = V.cap_of(case, longest)
        assert case["Lqc"] * case["ncells"] == 2 and cap == 6 < case["ndocs"] // 4 < len(case["lens"])
        cands = _candidates_are_the_oracles(case, want, off, pids)
        print(name, "candidates", [c.tolist() for c in cands], "final", [w["final"] for w in want])
        assert all(0 < len(c) <= cap for c in cands) and max(len(c) for c in cands) >= 3
        assert all(w["list1"] and len(w["list1"]) == len(w["list2"]) == len(c) for w, c in zip(want, cands)), "nothing cuts before k"
        if name == "narrow_k":
            assert cap < case["k"] <= case["ndocs"] // 4
            assert all(len(w["final"]) == len(c) < case["k"] for w, c in zip(want, cands)), "counts below k"
        else:
            assert case["k"] < cap and any(len(c) > case["k"] for c in cands) and all(len(w["final"]) == case["k"] for w in want)


def test_edges_bites():
    (codes, mask, lens, C), (off, pids) = _file("edges")
    lengths = np.diff(off)
    P = len(lens)
    assert C > 1024 and C % 1024 and P > 32 * V.COMPACT_WORDS
    assert {c: int(lengths[c]) for c in V.EDGE_LISTS} == V.EDGE_LISTS and 0 in V.EDGE_LISTS and C - 1 in V.EDGE_LISTS
    for want in (0, 1, 2, 3, 255, 256, 257, V.IVF_SORT_MAX - 1, V.IVF_SORT_MAX, V.IVF_SORT_MAX + 1):
        assert want in V.EDGE_LISTS.values()
    assert max(V.EDGE_LISTS.values()) > 2 * V.IVF_SORT_MAX
    assert (mask[codes == 1] == 0).all() and (codes == 1).sum() > 1000, "centroid 1 lies under masked rows only"
    rebuilt = [int(c) for c in np.flatnonzero(lengths > V.IVF_SORT_MAX)]
    assert len(rebuilt) >= 3 and lengths[rebuilt[-1]] < lengths[rebuilt[-2]], "the last rebuilt list is shorter than the one before"
    lists = [set(pids[off[c]:off[c + 1]].tolist()) for c in rebuilt]
    for i in range(1, len(lists)):                                # a bitmap left from an earlier list adds passages below the last
        stale = set().union(*lists[:i]) - lists[i]
        assert stale and min(stale) < max(lists[i]), "a later rebuilt list holds all of an earlier one"
    far = pids >= 32 * V.COMPACT_WORDS
    for c in V.EDGE_LISTS:
        if lengths[c] >= 255:
            assert far[off[c]:off[c + 1]].any() and not far[off[c]:off[c + 1]].all(), f"list {c} on one side of passage 32 768"
    short = np.flatnonzero((lengths > 1) & (lengths < 255))
    assert sum(far[off[c]:off[c + 1]].any() for c in short) > 100, "short lists with passages from 32 768 on"
    assert 1 < np.median(lengths[300:700]) < 255
    first = np.concatenate([[0], np.cumsum(lens)])
    unsorted = sum((np.diff(codes[first[p]:first[p + 1]]) < 0).any() for p in range(0, P, 10))
    assert unsorted > 200, "rows of a passage in code order"


def test_million_bites():
    (codes, mask, lens, C), (off, pids) = _file("million")
    lengths = np.diff(off)
    P = len(lens)
    assert P == V.P_MILLION and lengths[V.EVERYWHERE] == P > 4096 * 256, "the grid stride of the list's bitmap kernel"
    assert lengths[V.SOMETIMES] == (P + 256) // 257 == V.IVF_SORT_MAX + 1 and lengths.sum() == P + 4097
    assert np.array_equal(pids[off[V.SOMETIMES]:off[V.SOMETIMES + 1]], np.arange(0, P, 257))
    assert C > 1024 and C % 1024
