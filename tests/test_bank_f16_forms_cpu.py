"""CPU: what tests/test_gpu_bank_f16_forms.py stands on, shown without a device.

THE LAUNCH FORMS.  rr_op_bank_scores_f16_form (include/rerank_mi355_diag.h) reads out the host function the two first-pass launchers
call: the block's column tiles nt, the tiles of one query in a pass tp (the kernel instantiated is <nt, tp>) and the passes over a
query.  Over bank_f16_cases.FORM_SHAPES it must report every one of the ten instantiations, one, two and three or more passes at a
full-width block for each cap of the block (8, 4, 2, 1 as D grows), a padded tile count and a last pass shorter than a tile: "every
form is covered" is an assertion here, and a launcher retuned away from the table fails it.  The library is loaded (it loads
without a device); nothing is launched.
THE DEFAULT SLACK.  Two queries outside fp16's normal range that the default slack used to certify although the exact winner is not
among the results, on the host definition (bank_f16_cases.search_f16 over approx64 / exact64): the old formula certifies both, the
corrected default neither, and the corrected bound holds where the query's rounding error is absolute.
THE FLOAT64 MARGINS of the long random fixture: twice the default slack, as tests/test_bank_f16_cpu.py shows for the short one.
"""
import ctypes

import numpy as np
import pytest

import bank_f16_cases as C
from rmr_amd import F16Search, f16_default_slack

NDOCS, K = 64, 16
ALL_FORMS = {(1, 1), (2, 1), (2, 2), (4, 1), (4, 2), (4, 4), (8, 1), (8, 2), (8, 4), (8, 8)}
# (n_queries, Lq) -> (nt, tp, passes) wherever the block may be 8 tiles wide (both launchers at D 32 .. 128)
FORMS_AT_CAP_8 = {(1, 16): (1, 1, 1), (2, 9): (2, 1, 1), (1, 17): (2, 2, 1), (4, 16): (4, 1, 1), (2, 32): (4, 2, 1), (1, 33): (4, 4, 1),
                  (1, 48): (4, 4, 1), (5, 1): (8, 1, 1), (3, 31): (8, 2, 1), (2, 64): (8, 4, 1), (3, 49): (8, 4, 1), (1, 65): (8, 8, 1),
                  (2, 128): (8, 8, 1), (1, 129): (8, 8, 2), (3, 130): (8, 8, 2), (1, 257): (8, 8, 3), (3, 20): (8, 2, 1)}
FORMS_ABOVE_128 = {(256, 1, 64): (4, 4, 1), (256, 2, 65): (4, 4, 2), (256, 1, 200): (4, 4, 4), (512, 1, 32): (2, 2, 1), (512, 2, 33): (2, 2, 2),
                   (512, 1, 100): (2, 2, 4), (1024, 1, 16): (1, 1, 1), (1024, 2, 17): (1, 1, 2), (1024, 1, 40): (1, 1, 3)}
CAPS = {32: 8, 64: 8, 96: 8, 128: 8, 256: 4, 512: 2, 1024: 1}


def _form(nq, Lq, D, plaid):
    """(status, nt, tp, passes) of rr_op_bank_scores_f16_form; the outputs start at -7 and must stay there when it refuses"""
    from rmr_amd import _lib as L
    lib = L.load()
    out = [ctypes.c_int(-7) for _ in range(3)]
    rc = lib.rr_op_bank_scores_f16_form(nq, Lq, D, int(plaid), *[ctypes.byref(o) for o in out])
    return (rc,) + tuple(o.value for o in out)


def test_form_shapes_cover_every_form_of_the_fp16_launcher():
    assert len(set(C.FORM_SHAPES)) == len(C.FORM_SHAPES) == 2 * 16 + 9 + 2
    forms = {}
    for D, nq, Lq in C.FORM_SHAPES:
        rc, nt, tp, passes = _form(nq, Lq, D, plaid=False)
        assert rc == 0, (D, nq, Lq, rc)
        tiles = -(-Lq // 16)
        assert tp <= nt <= CAPS[D] and tp & (tp - 1) == 0 and nt % tp == 0 and passes == -(-tiles // tp) and (passes == 1 or tp == nt == CAPS[D])
        forms[(D, nq, Lq)] = (nt, tp, passes)
    want = {(D, nq, Lq): f for (nq, Lq), f in FORMS_AT_CAP_8.items() for D in (32, 64, 96, 128) if (D, nq, Lq) in forms}
    want.update(FORMS_ABOVE_128)
    assert forms == want, {s: (forms.get(s), want.get(s)) for s in set(forms) | set(want) if forms.get(s) != want.get(s)}
    for D in (64, 128):                                                    # all ten instantiations, at both engine dimensions
        assert {f[:2] for s, f in forms.items() if s[0] == D} == ALL_FORMS, D
    for cap in (8, 4, 2, 1):                                               # 1, 2 and >= 3 passes at a full-width block, per cap
        seen = {min(f[2], 3) for s, f in forms.items() if CAPS[s[0]] == cap and f[0] == cap and f[1] == cap}
        assert seen == {1, 2, 3}, (cap, seen)
    assert _form(64, 4096, 64, False)[1:] == (8, 8, 32)                    # ... and the caps are the launcher's, not this file's
    for D, cap in CAPS.items():
        assert _form(64, 4096, D, False)[1] == cap, D
    padded = [s for s, f in forms.items() if -(-s[2] // 16) < f[1] * f[2]]                       # tiles behind Lq in the last pass
    assert {(64, 1, 33), (128, 1, 129), (128, 3, 130), (256, 2, 65), (512, 2, 33)} <= set(padded)
    short_last = [s for s, f in forms.items() if f[2] > 1 and s[2] - (f[2] - 1) * f[1] * 16 < 16]   # (Lq - j0) < 16 in the last pass
    assert {(64, 1, 129), (128, 3, 130), (128, 1, 257), (256, 2, 65), (512, 2, 33), (1024, 2, 17), (1024, 1, 40)} <= set(short_last)
    empty_slot = [s for s, f in forms.items() if s[1] % (f[0] // f[1])]                           # the q < nq guard, in a wide form
    assert {(64, 3, 49), (128, 3, 49), (64, 5, 1), (128, 3, 31)} <= set(empty_slot)


def test_form_shapes_cover_every_form_of_the_plaid_launcher():
    """D 64 and 128: all ten instantiations (the block is 8 tiles wide beside the decoded tiles: 72 KB of LDS at D 128).  D 256: the
    block is capped at 4 tiles (NT_MAX 4 of the launch) and FORM_SHAPES runs it at one, two and four passes.  D 32 at (8, 2)."""
    from rmr_amd import _lib as L
    forms = {}
    for D, nq, Lq in C.FORM_SHAPES:
        rc, nt, tp, passes = _form(nq, Lq, D, plaid=True)
        if D in (512, 1024, 96):
            assert (rc, nt, tp, passes) == (L.RR_ERR_UNSUPPORTED, -7, -7, -7), (D, rc)          # refused, nothing written ...
            assert _form(nq, Lq, D, plaid=False)[0] == 0                                       # ... and accepted for fp16 rows
        else:
            assert rc == 0, (D, nq, Lq, rc)
            forms[(D, nq, Lq)] = (nt, tp, passes)
    want = {(D, nq, Lq): f for (nq, Lq), f in FORMS_AT_CAP_8.items() for D in (32, 64, 128) if (D, nq, Lq) in forms}
    want.update({s: f for s, f in FORMS_ABOVE_128.items() if s[0] == 256})
    assert forms == want, {s: (forms.get(s), want.get(s)) for s in set(forms) | set(want) if forms.get(s) != want.get(s)}
    for D in (64, 128):
        assert {f[:2] for s, f in forms.items() if s[0] == D} == ALL_FORMS, D
    assert {f for s, f in forms.items() if s[0] == 256} == {(4, 4, 1), (4, 4, 2), (4, 4, 4)}
    assert [_form(64, 4096, D, True)[1] for D in (32, 64, 128, 256)] == [8, 8, 8, 4]
    assert forms[(32, 3, 20)] == (8, 2, 1)


def test_the_form_entry_refuses_what_the_operators_refuse():
    from rmr_amd import _lib as L
    untouched = (-7, -7, -7)
    for plaid in (False, True):
        for D in (0, -32, 48, 16):
            assert _form(1, 16, D, plaid) == (L.RR_ERR_UNSUPPORTED,) + untouched, (plaid, D)
        for nq, Lq in ((0, 16), (-1, 16), (65536, 16), (1, 0), (1, -5)):
            assert _form(nq, Lq, 64, plaid) == (L.RR_ERR_BAD_SHAPE,) + untouched, (plaid, nq, Lq)
        assert _form(65535, 1, 64, plaid) == (0, 8, 1, 1)
    assert _form(1, 16, 96, True)[0] == L.RR_ERR_UNSUPPORTED and _form(1, 16, 96, False) == (0, 1, 1, 1)
    # the narrowest block [16][D + 16] fp16 must fit 150 KB of LDS: D 4768 does, D 4800 does not (the launch itself refuses)
    assert _form(1, 16, 4768, False) == (0, 1, 1, 1) and _form(1, 16, 4800, False) == (L.RR_ERR_HIP,) + untouched
    lib = L.load()
    assert lib.rr_op_bank_scores_f16_form(1, 16, 64, 0, None, None, None) == L.RR_ERR_BAD_ARG


def test_exact_fixture_states_its_condition_and_the_long_kind_its_edges():
    for D, nq, Lq in C.FORM_SHAPES:
        assert D * Lq <= 65536
    assert max(D * Lq for D, nq, Lq in C.FORM_SHAPES) == 256 * 200
    with pytest.raises(AssertionError, match="65536"):
        C.exact_fixture("mixed", 1024, 1, 65, seed=0)
    fx = C.exact_fixture("long", 64, 1, 16, seed=1)
    lens, mask, fr = fx["lens"], fx["mask"], C.first_rows(fx["lens"])
    assert len(lens) == C.LONG_PASSAGES == 71 and lens[:17] == C.LONG_EDGES and all(1 <= v <= 130 for v in lens[17:])
    assert np.abs(fx["rows"]).max() <= 2.0 and np.array_equal(fx["rows"] * 8, np.round(fx["rows"] * 8))
    kept = lambda p: mask[fr[p]:fr[p] + lens[p]]
    assert not kept(C.LONG_FULLY_MASKED).any()
    assert kept(C.LONG_ROW0_MASKED).tolist() == [0] + [1] * 31 and kept(C.LONG_LAST_MASKED).tolist() == [1] * 47 + [0]
    assert kept(C.LONG_ONLY_LAST_KEPT).tolist() == [0] * 96 + [1]
    assert np.flatnonzero(kept(C.LONG_TILE_EDGES_MASKED) == 0).tolist() == [15, 16, 31, 32, 63, 64]
    E = C.exact64(fx)
    assert (E[:, C.LONG_FULLY_MASKED] == 16 * C.MASKED).all() and np.array_equal(E.astype(np.float32).astype(np.float64), E)
    p, a = C.LONG_ONLY_LAST_KEPT, fr[C.LONG_ONLY_LAST_KEPT]
    assert E[0, p] == (fx["q"][0].astype(np.float64) @ fx["rows"][a + 96].astype(np.float64)).sum()      # the one kept row decides alone


def _certified(fx, slack):
    A, E = C.approx64(fx), C.exact64(fx)
    return A, E, C.search_f16(A, E, NDOCS, K, slack)


def test_the_old_default_slack_certified_two_wrong_results_and_the_new_one_does_not():
    D = 64
    over, under = C.overflow_fixture(D, NDOCS), C.underflow_fixture(D, NDOCS)
    n = NDOCS + 9
    # overflow: every A is -inf, the exact winner (the last passage, -4.27 against -68.4) is no survivor
    old = C.old_default_slack(over["q"], D)
    A, E, (idx, sc, cert) = _certified(over, old)
    assert np.isneginf(A).all() and C.rank_order(E[0])[0] == n - 1 and E[0, n - 1] == -70000.0 * 2.0 ** -14 and E[0, 0] == -70000.0 * 2.0 ** -10
    assert old == pytest.approx(35.3, rel=1e-2) and idx[0].tolist() == list(range(K)) and n - 1 not in idx[0]
    assert cert.tolist() == [1], "the old formula no longer shows the false certificate it is kept here to show"
    new = C.default_slack(over["q"], D)
    assert new == np.inf and _certified(over, new)[2][2].tolist() == [0]
    assert _certified(over, 1e30)[2][2].tolist() == [1]                    # no finite slack helps: -inf + slack is -inf
    # underflow: every A is 0, the exact winner (the last passage, 2^-26 against 2^-27) is no survivor
    old = C.old_default_slack(under["q"], D)
    A, E, (idx, sc, cert) = _certified(under, old)
    assert (A == 0.0).all() and C.rank_order(E[0])[0] == n - 1 and E[0, n - 1] == 2.0 ** -26 and (sc == 2.0 ** -27).all()
    assert old == pytest.approx(7.5e-12, rel=1e-2) and n - 1 not in idx[0]
    assert cert.tolist() == [1], "the old formula no longer shows the false certificate it is kept here to show"
    assert np.abs(A - E).max() > old                                       # ... because it is no bound on |A - E| here
    new = C.default_slack(under["q"], D)
    assert np.abs(A - E).max() <= new and _certified(under, new)[2][2].tolist() == [0]
    assert new == pytest.approx(old + np.sqrt(D) * 2.0 ** -25 * (1 + 2.0 ** -10), rel=1e-12)


@pytest.mark.parametrize("D", [64, 128])
def test_the_default_slack_bounds_the_rounding_of_elements_below_the_normal_range(D):
    fx = C.subnormal_mix_fixture(D, seed=D)
    A, E = C.approx64(fx), C.exact64(fx)
    err = np.abs(C.fp16_rne(fx["q"]).astype(np.float64) - fx["q"].astype(np.float64))
    assert err[..., D // 2:].max() <= 2.0 ** -25 and err[..., D // 2:].max() > 2.0 ** -11 * fx["q"][..., D // 2:].min()      # absolute, not relative
    assert (err <= np.maximum(2.0 ** -11 * np.abs(fx["q"]), 2.0 ** -25)).all()                    # the per-element statement of the bound
    assert np.abs(A - E).max() <= C.default_slack(fx["q"], D)


def test_python_default_is_the_restated_one():
    """F16Search.slack_for (torch, on whatever device the query lies) against bank_f16_cases.default_slack, on every fixture above"""
    import torch
    D = 64
    cases = [C.overflow_fixture(D, NDOCS), C.underflow_fixture(D, NDOCS), C.subnormal_mix_fixture(D, seed=D), C.adversarial_fixture(D, NDOCS),
             C.random_fixture_long(D, 2, 49, seed=D + 49)]
    for fx in cases:
        got, want = F16Search(NDOCS).slack_for(torch.from_numpy(fx["q"])), C.default_slack(fx["q"], D)
        assert got == want if np.isinf(want) else got == pytest.approx(want, rel=1e-12)
    q = torch.zeros(2, 3, D)
    q[1, 2, 5] = -65519.0
    assert np.isfinite(F16Search(8).slack_for(q))
    for v in (65520.0, -65520.0, float("inf"), -float("inf")):
        q[1, 2, 5] = v
        assert F16Search(8).slack_for(q) == float("inf"), v
    q[0, 0, 0] = float("nan")                                             # a NaN query keeps a NaN slack: the entries refuse it
    assert np.isnan(F16Search(8).slack_for(q))
    assert F16Search(8, 0.5).slack_for(q) == 0.5
    assert float(np.float16(np.float32(65519.99))) == 65504.0 and np.isinf(C.fp16_rne(65520.0))


@pytest.mark.parametrize("D,nq,Lq", [(128, 3, 130), (64, 2, 49)])
def test_long_random_fixture_leaves_the_certificate_twice_the_default_slack(D, nq, Lq):
    """tests/test_bank_f16_cpu.py's statement for random_fixture_long, the fixture of the accumulation measurements over long
    passages: in float64 the k-th exact score stands at least 2 x the default slack above the (ndocs + 1)-th best."""
    fx = C.random_fixture_long(D, nq, Lq, seed=D + Lq)
    assert NDOCS < len(fx["lens"])
    E = C.exact64(fx)
    slack = C.default_slack(fx["q"], D)
    assert slack == pytest.approx(f16_default_slack(np.linalg.norm(fx["q"].astype(np.float64), axis=-1).sum(axis=-1).max(), D, Lq), rel=1e-12)
    assert np.linalg.norm(fx["rows"].astype(np.float64), axis=-1).max() <= 1.0 + 2.0 ** -10
    for qi in range(nq):
        s = E[qi, C.rank_order(E[qi])]
        assert s[K - 1] - s[NDOCS] >= 2.0 * slack, (qi, s[K - 1], s[NDOCS], slack)
    assert np.abs(C.approx64(fx) - E).max() <= slack                      # the query's rounding alone stays inside it
    assert (C.search_f16(C.approx64(fx), E, NDOCS, K, slack)[2] == 1).all()
