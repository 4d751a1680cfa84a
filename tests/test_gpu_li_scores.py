"""rr_li_scores on the device (csrc/li_scores.hip): the retriever's late-interaction score matrix and MaxSim, against the
formula of the reference's colbert_score (flmr_utils.py:22-48; tests/li_scores_ref.py, pinned to the reference's own arrays by
tests/test_li_scores_cpu.py) evaluated in float64 on the same float32 inputs.

Bounds (unit-norm rows, u = 2^-23): an unmasked entry is a length-D float32 dot product, |d| <= D * u * |q| * |c| = D * 2^-23;
MaxSim adds Lq such entries in float32, |d| <= Lq * D * 2^-23 + Lq^2 * 2^-24 (Lq - 1 additions of partial sums below Lq, half
an ulp each).  Masked rows are -9999 exactly.  The measured maxima go to the margins file (helpers.record_margin;
profiles/li_scores_margins.json holds the run that was committed)."""
import ctypes as C

import pytest
import torch

from helpers import O, arch_from_cfg, record_margin
from li_scores_ref import MASKED, li_scores_formula, load_li_scores_ref, retriever_inputs

pytestmark = pytest.mark.gpu

POISON = 12345.5
_ENGINES = {}


def _engine(D, kind="interaction"):
    """A handle is all rr_li_scores needs (no weights); any model kind."""
    import rmr_amd
    if (D, kind) not in _ENGINES:
        cfg = O.OracleConfig(li_dim=D)
        arch = arch_from_cfg(cfg, kind == "full_context")
        arch["model_kind"] = kind
        _ENGINES[(D, kind)] = rmr_amd.RerankEngine(arch)
    return _ENGINES[(D, kind)]


def _bounds(D, Lq):
    return D * 2.0 ** -23, Lq * D * 2.0 ** -23 + Lq ** 2 * 2.0 ** -24


def _raw(eng, q, c, cm, Bq, K, pb, pe, scores, maxsim):
    from rmr_amd import _lib as L
    return eng.lib.rr_li_scores(eng.h, L.ptr(q), L.ptr(c), L.ptr(cm), Bq, K, q.shape[1], c.shape[1], pb, pe, L.ptr(scores),
                                L.ptr(maxsim), torch.cuda.current_stream().cuda_stream)


SHAPES = [(D, Lq, Lc) for D in (64, 128) for Lq in (1, 9, 113, 130) for Lc in (1, 40, 512, 515)]


@pytest.mark.parametrize("D,Lq,Lc", SHAPES)
def test_scores_and_maxsim_against_float64(D, Lq, Lc):
    i = SHAPES.index((D, Lq, Lc))
    K = (1, 3, 100)[(i + i // 4) % 3]                 # every K meets every Lq and every Lc over the two D
    Bq = 2 if K == 100 else 3
    N = Bq * K
    q, c, cm = retriever_inputs(Bq, K, Lq, Lc, D, seed=100 + i, full_mask_pair=N - 2)
    m64, s64 = li_scores_formula(q, c, cm, K, torch.float64)
    eng = _engine(D)
    qd, cd, cmd = q.cuda(), c.cuda(), cm.cuda()
    r = eng.li_scores(qd, cd, cmd, Bq, K)
    again = eng.li_scores(qd, cd, cmd, Bq, K)
    only = eng.li_scores(qd, cd, cmd, Bq, K, want_scores=False)
    torch.cuda.synchronize()
    sc, ms = r["scores"].cpu(), r["maxsim"].cpu()
    keep = cm.bool()
    assert (sc[~keep] == MASKED).all(), "masked rows must be -9999 exactly"
    d_s = (sc.double() - s64)[keep].abs().max().item() if keep.any() else 0.0
    d_m = (ms.double() - m64).abs().max().item()
    b_s, b_m = _bounds(D, Lq)
    print(f"[D {D} Lq {Lq} Lc {Lc} K {K}] scores |d| {d_s:.3e} (bound {b_s:.3e}), maxsim |d| {d_m:.3e} (bound {b_m:.3e})")
    record_margin(f"li_scores/D{D}_Lq{Lq}_Lc{Lc}_K{K}", scores_max_abs=d_s, scores_bound=b_s, maxsim_max_abs=d_m, maxsim_bound=b_m)
    assert d_s <= b_s and d_m <= b_m
    assert ms[N - 2].item() == MASKED * Lq                                   # fully masked pair: integers below 2^24
    assert "scores" not in only and torch.equal(only["maxsim"], r["maxsim"])  # the same bits without the score block
    assert torch.equal(again["maxsim"], r["maxsim"]) and torch.equal(again["scores"], r["scores"])

    # a slice that starts and ends inside a query (K > 1) writes its rows only, with the full call's bits
    pb, pe = K // 2, N - max(1, K // 3)
    ps = torch.full((N, Lc, Lq), POISON, device="cuda")
    pm = torch.full((N,), POISON, device="cuda")
    assert _raw(eng, qd, cd, cmd, Bq, K, pb, pe, ps, pm) == 0
    torch.cuda.synchronize()
    assert torch.equal(ps[pb:pe], r["scores"][pb:pe]) and torch.equal(pm[pb:pe], r["maxsim"][pb:pe])
    assert (ps[:pb] == POISON).all() and (ps[pe:] == POISON).all() and (pm[:pb] == POISON).all() and (pm[pe:] == POISON).all()


@pytest.mark.parametrize("kind", ["interaction", "mores", "full_context"])
def test_reference_fixture_on_every_model_kind(kind):
    """tests/golden/li_scores_ref.npz: what the reference's own colbert_score returned (holes, one fully masked pair)."""
    g = load_li_scores_ref()
    eng = _engine(g["D"], kind)
    r = eng.li_scores(g["query_li"].cuda(), g["context_li"].cuda(), g["context_mask"].cuda(), g["Bq"], g["K"])
    torch.cuda.synchronize()
    sc, ms = r["scores"].cpu(), r["maxsim"].cpu()
    keep = g["context_mask"].bool()
    b_s, b_m = _bounds(g["D"], g["Lq"])
    d_s, d_m = (sc - g["scores"])[keep].abs().max().item(), (ms - g["maxsim"]).abs().max().item()
    print(f"[li_scores_ref/{kind}] vs the reference's arrays: scores {d_s:.3e}, maxsim {d_m:.3e}")
    record_margin(f"li_scores/reference_fixture_{kind}", scores_max_abs=d_s, maxsim_max_abs=d_m)
    assert torch.equal(sc[~keep], g["scores"][~keep])
    assert d_s <= 2 * b_s and d_m <= 2 * b_m              # two float32 evaluations, each within the bound of the exact value
    assert ms[4].item() == g["maxsim"][4].item() == MASKED * g["Lq"]


def test_non_finite_rows():
    D, Lq, Lc, Bq, K = 64, 9, 40, 2, 3
    q, c, cm = retriever_inputs(Bq, K, Lq, Lc, D, seed=7, holes=False)
    cm[:, :8] = 1
    cm[1, 5] = 0                                           # a hole ...
    c[1, 5] = float("nan")                                 # ... whose embedding is NaN, and one with inf
    cm[2, 6] = 0
    c[2, 6, 3] = float("inf")
    c[3, 2, 1] = float("nan")                              # an unmasked NaN in pair 3
    eng = _engine(D)
    r = eng.li_scores(q.cuda(), c.cuda(), cm.cuda(), Bq, K)
    only = eng.li_scores(q.cuda(), c.cuda(), cm.cuda(), Bq, K, want_scores=False)
    torch.cuda.synchronize()
    sc, ms = r["scores"].cpu(), r["maxsim"].cpu()
    assert (sc[1, 5] == MASKED).all() and (sc[2, 6] == MASKED).all()
    assert torch.isnan(sc[3, 2]).all()
    others = torch.ones(Bq * K, Lc, dtype=torch.bool)
    others[3, 2] = False
    assert torch.isfinite(sc[others]).all(), "a NaN row must not leak into other rows"
    assert torch.isnan(ms[3]) and torch.isfinite(ms[[0, 1, 2, 4, 5]]).all()
    assert torch.isnan(only["maxsim"][3]) and torch.equal(only["maxsim"].cpu()[[0, 1, 2, 4, 5]], ms[[0, 1, 2, 4, 5]])
    c[3, 2] = 0.0                                          # the same batch without the NaN: the other pairs' bits are unchanged
    clean = eng.li_scores(q.cuda(), c.cuda(), cm.cuda(), Bq, K)
    torch.cuda.synchronize()
    assert torch.equal(clean["maxsim"].cpu()[[0, 1, 2, 4, 5]], ms[[0, 1, 2, 4, 5]])


def test_refusals_write_nothing():
    D, Lq, Lc, Bq, K = 64, 9, 40, 2, 3
    N = Bq * K
    q, c, cm = (t.cuda() for t in retriever_inputs(Bq, K, Lq, Lc, D, seed=9))
    eng = _engine(D)
    ps = torch.full((N, Lc, Lq), POISON, device="cuda")
    pm = torch.full((N,), POISON, device="cuda")
    from rmr_amd import _lib as L
    st = torch.cuda.current_stream().cuda_stream
    call = eng.lib.rr_li_scores
    args = (L.ptr(q), L.ptr(c), L.ptr(cm))
    assert call(eng.h, *args, Bq, K, Lq, Lc, 0, N, None, None, st) == L.RR_ERR_BAD_ARG          # no output at all
    assert b"both null" in eng.lib.rr_last_error(eng.h)
    for bad in ((None, args[1], args[2]), (args[0], None, args[2]), (args[0], args[1], None)):
        assert call(eng.h, *bad, Bq, K, Lq, Lc, 0, N, L.ptr(ps), L.ptr(pm), st) == L.RR_ERR_BAD_ARG
    assert call(None, *args, Bq, K, Lq, Lc, 0, N, L.ptr(ps), L.ptr(pm), st) == L.RR_ERR_BAD_ARG
    for shape in ((0, K, Lq, Lc), (Bq, 0, Lq, Lc), (Bq, K, 0, Lc), (Bq, K, Lq, -1)):
        assert call(eng.h, *args, *shape, 0, N, L.ptr(ps), L.ptr(pm), st) == L.RR_ERR_BAD_SHAPE
    for pb, pe in ((0, N + 1), (-1, N), (3, 3), (4, 2)):
        assert call(eng.h, *args, Bq, K, Lq, Lc, pb, pe, L.ptr(ps), L.ptr(pm), st) == L.RR_ERR_BAD_SHAPE
    assert call(eng.h, args[0] + 4, args[1], args[2], Bq, K, Lq, Lc, 0, N, L.ptr(ps), L.ptr(pm), st) == L.RR_ERR_BAD_ARG   # alignment
    torch.cuda.synchronize()
    assert (ps == POISON).all() and (pm == POISON).all()
    with pytest.raises(ValueError):
        eng.li_scores(q, c, cm, Bq, K, want_scores=False, want_maxsim=False)
    with pytest.raises(AssertionError):
        eng.li_scores(q, c, cm, Bq, K, pair_range=(0, N + 1))
    with pytest.raises(AssertionError):
        eng.li_scores(q, c, cm, Bq, K + 1)


def test_profile_books_the_operator_as_tail():
    D, Lq, Lc, Bq, K = 128, 113, 512, 1, 6
    q, c, cm = (t.cuda() for t in retriever_inputs(Bq, K, Lq, Lc, D, seed=3))
    eng = _engine(D)
    eng.set_profiling(True)
    try:
        eng.get_profile(reset=True)
        eng.li_scores(q, c, cm, Bq, K)
        p = eng.get_profile(reset=True)
    finally:
        eng.set_profiling(False)
    assert p["tail"]["launches"] == 1 and p["tail"]["flops"] == 2.0 * Bq * K * Lc * Lq * D and p["tail"]["ms"] > 0
    assert sum(v["launches"] for v in p.values()) == 1
