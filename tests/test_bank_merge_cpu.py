"""CPU: rr_util_bank_merge_topk, THE MERGED LIST of include/rerank_mi355.h in host code, against a numpy restatement that calls
nothing of the library (tests/bank_merge_cases.py: a stable lexsort on (NaN flag, score with -0 -> +0, global index)), and every
refusal of the entry's table with the outputs left untouched."""
import numpy as np
import pytest

import bank_merge_cases as MC

POISON = 0x7b7b7b7b


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from rmr_amd import _lib
    return _lib.load()


def _ptr(a):
    return 0 if a is None else a.ctypes.data


def run_util(lib, case, k=None, scores=True, parts=True):
    k = case["k"] if k is None else k
    nq = case["nq"]
    out = dict(indices=np.full((nq, k), POISON, dtype=np.int32), scores=np.full((nq, k), POISON, dtype=np.int32) if scores else None,
               counts=np.full(nq, POISON, dtype=np.int32), parts=np.full((nq, k), POISON, dtype=np.int32) if parts else None)
    rc = lib.rr_util_bank_merge_topk(case["idx"].ctypes.data, case["sc"].ctypes.data, _ptr(case["cnt"]), case["part_stride"],
                                     case["count_stride"], case["P"], case["offsets"].ctypes.data, nq, case["k_in"], k,
                                     _ptr(out["indices"]), _ptr(out["scores"]), _ptr(out["counts"]), _ptr(out["parts"]))
    return rc, out


def check_against_reference(case, out, what):
    wi, ws, wc, wp = MC.expected(case)
    assert np.array_equal(out["counts"], wc), f"{what}: counts"
    assert np.array_equal(out["indices"], wi), f"{what}: indices"
    if out.get("scores") is not None:
        assert np.array_equal(np.asarray(out["scores"]).view(np.uint32), ws), f"{what}: score bits"
    if out.get("parts") is not None:
        assert np.array_equal(out["parts"], wp), f"{what}: parts"


@pytest.mark.parametrize("nq", [1, 3])
def test_host_definition_equals_the_numpy_restatement(lib, nq):
    for case in MC.cases(nq):
        before = case["block"].copy()
        rc, out = run_util(lib, case)
        assert rc == 0, case["name"]
        check_against_reference(case, out, case["name"])
        assert np.array_equal(case["block"], before), "the inputs are read only"


def test_the_cases_hold_what_they_are_meant_to(lib):
    """The inputs themselves: ties across parts, both zeros, NaN, both infinities, -inf inside a count, an index twice within a
    part, indices outside their part, an empty part, offsets up to 2^31 - 1, counts 0 / negative / above k_in."""
    cs = MC.cases(3)
    c = next(x for x in cs if x["name"] == "8 x 1024, ties")
    sc, idx, cnt = c["sc"], c["idx"], c["cnt"]
    bits = sc.view(np.uint32)
    assert (bits == 0x80000000).any() and (bits == 0).any() and np.isnan(sc).any() and np.isposinf(sc).any() and np.isneginf(sc).any()
    assert np.isneginf(sc[3, 0, :max(int(cnt[3, 0]), 0)]).any()
    assert (idx < 0).any() and (idx[3] >= 2500).any()
    assert len(np.unique(idx[2, 0])) < idx.shape[2]
    assert (cnt[0] == 0).all() and (cnt[:, 1] == 0).all() and (cnt < 0).any() and (cnt > c["k_in"]).any()
    assert c["offsets"][1] == c["offsets"][2]
    wi, ws, wc, wp = MC.expected(c)
    assert wc[1] == 0 and wc[0] == c["k"] and len(set(wp[0].tolist())) > 1
    top = ws[0, :wc[0]]
    assert (top == 0x40e00000).sum() > 1                      # 7.0 from more than one part: ties across parts, by global index
    assert any(int(x["offsets"][-1]) == MC.INT32_MAX for x in cs)


def test_null_scores_out_and_parts_out(lib):
    case = MC.cases(3)[4]
    rc, out = run_util(lib, case, scores=False, parts=False)
    assert rc == 0
    check_against_reference(case, out, "no scores, no parts")


def test_k_below_k_in_is_a_prefix(lib):
    case = MC.cases(3)[8]
    _, full = run_util(lib, case)
    rc, out = run_util(lib, case, k=37)
    assert rc == 0
    assert np.array_equal(out["indices"], full["indices"][:, :37]) and np.array_equal(out["scores"], full["scores"][:, :37])
    assert np.array_equal(out["counts"], np.minimum(full["counts"], 37))


def refusals(case):
    """(what, status, the arguments that differ from a good call): every row of the entry's table that needs no device."""
    from rmr_amd import _lib as L
    P, nq, k_in = case["P"], case["nq"], case["k_in"]
    down = case["offsets"].copy()
    down[2] = down[1] - 1
    neg = case["offsets"].copy()
    neg[0] = -1
    big = np.zeros(66, dtype=np.int32)
    return [
        ("null indices_in", L.RR_ERR_BAD_ARG, dict(indices_in=0)),
        ("null scores_in", L.RR_ERR_BAD_ARG, dict(scores_in=0)),
        ("null part_offsets", L.RR_ERR_BAD_ARG, dict(offsets=0)),
        ("null indices_out", L.RR_ERR_BAD_ARG, dict(indices_out=0)),
        ("null counts_out", L.RR_ERR_BAD_ARG, dict(counts_out=0)),
        ("misaligned indices_in", L.RR_ERR_BAD_ARG, dict(indices_in=case["idx"].ctypes.data + 2)),
        ("misaligned counts_in", L.RR_ERR_BAD_ARG, dict(counts_in=case["cnt"].ctypes.data + 1)),
        ("misaligned scores_out", L.RR_ERR_BAD_ARG, dict(scores_out_shift=2)),
        ("n_parts 0", L.RR_ERR_BAD_SHAPE, dict(P=0)),
        ("n_queries 0", L.RR_ERR_BAD_SHAPE, dict(nq=0)),
        ("k_in -1", L.RR_ERR_BAD_SHAPE, dict(k_in=-1)),
        ("k 0", L.RR_ERR_BAD_SHAPE, dict(k=0)),
        ("k above k_in", L.RR_ERR_BAD_SHAPE, dict(k=k_in + 1)),
        ("part_stride below n_queries * k_in", L.RR_ERR_BAD_SHAPE, dict(part_stride=nq * k_in - 1)),
        ("count_stride below n_queries", L.RR_ERR_BAD_SHAPE, dict(count_stride=nq - 1)),
        ("part_offsets[0] negative", L.RR_ERR_BAD_SHAPE, dict(offsets=neg.ctypes.data, keep=neg)),
        ("a descending offset", L.RR_ERR_BAD_SHAPE, dict(offsets=down.ctypes.data, keep=down)),
        ("n_parts 65", L.RR_ERR_UNSUPPORTED, dict(P=65, k_in=1, k=1, offsets=big.ctypes.data, keep=big, part_stride=1 << 20, count_stride=1 << 20)),
        ("n_queries 65536", L.RR_ERR_UNSUPPORTED, dict(nq=65536, part_stride=1 << 30, count_stride=1 << 30)),
        ("3 x 2731 = 8193 entries", L.RR_ERR_UNSUPPORTED, dict(k_in=2731, k=1, part_stride=1 << 30)),
    ]


def call_with(fn, case, out, over, lead=(), tail=()):
    a = dict(indices_in=case["idx"].ctypes.data, scores_in=case["sc"].ctypes.data, counts_in=case["cnt"].ctypes.data,
             part_stride=case["part_stride"], count_stride=case["count_stride"], P=case["P"], offsets=case["offsets"].ctypes.data,
             nq=case["nq"], k_in=case["k_in"], k=case["k"], indices_out=out["indices"], scores_out=out["scores"],
             counts_out=out["counts"], parts_out=out["parts"])
    a.update({n: v for n, v in over.items() if n in a})
    a["scores_out"] += over.get("scores_out_shift", 0)
    return fn(*lead, a["indices_in"], a["scores_in"], a["counts_in"], a["part_stride"], a["count_stride"], a["P"], a["offsets"], a["nq"],
              a["k_in"], a["k"], a["indices_out"], a["scores_out"], a["counts_out"], a["parts_out"], *tail)


def test_every_refusal_leaves_the_outputs_untouched(lib):
    case = MC.make_case("3 x 5", 3, 5, 5, 3, 11)
    for what, status, over in refusals(case):
        outs = {n: np.full(64, POISON, dtype=np.int32) for n in ("indices", "scores", "counts", "parts")}
        rc = call_with(lib.rr_util_bank_merge_topk, case, {n: v.ctypes.data for n, v in outs.items()}, over)
        assert rc == status, f"{what}: status {rc}"
        assert all((v == POISON).all() for v in outs.values()), f"{what}: an output was written"
    outs = {n: np.full(64, POISON, dtype=np.int32) for n in ("indices", "scores", "counts", "parts")}
    assert call_with(lib.rr_util_bank_merge_topk, case, {n: v.ctypes.data for n, v in outs.items()}, {}) == 0
    from rmr_amd import _lib as L
    assert call_with(lib.rr_bank_merge_topk, case, {n: v.ctypes.data for n, v in outs.items()}, {}, lead=(None,), tail=(None,)) == L.RR_ERR_BAD_ARG


def test_the_largest_call_is_taken_and_one_more_entry_is_not(lib):
    from rmr_amd import _lib as L
    case = MC.make_case("8 x 1024", 8, 1024, 1024, 1, 12)
    assert run_util(lib, case)[0] == 0
    case = MC.make_case("3 x 2731", 3, 2731, 1, 1, 13)
    assert run_util(lib, case)[0] == L.RR_ERR_UNSUPPORTED
