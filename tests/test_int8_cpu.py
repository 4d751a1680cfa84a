"""CPU: the host side of the int8 (W8A8) form of rr_config.fp8 ("q8_format" = 1) — the outlier smoothing folded at
rr_finalize_weights and the per-channel weight quantiser (pure host code in the library, no GPU), against the emulation the GPU
tests use (tests/int8_emulation.py)."""
import numpy as np
import torch

from helpers import ROOT  # noqa: F401
from int8_emulation import quant_rows_i8, smooth_scales

OUTLIERS = ((7, 50.0), (300, 50.0), (555, 300.0))       # the dimensions and factors of tests/test_gpu_outliers.py


def _lib():
    from rmr_amd import _lib
    return _lib.load()


def _ln_affine(n, seed, outliers=()):
    g = np.random.default_rng(seed)
    gamma = (1.0 + 0.1 * g.standard_normal(n)).astype(np.float32)
    beta = (0.05 * g.standard_normal(n)).astype(np.float32)
    for d, s in outliers:
        gamma[d] *= s
        beta[d] += 0.02 * s
    return gamma, beta


def _lib_smooth(gamma, beta):
    out = np.zeros(gamma.size, dtype=np.float32)
    assert _lib().rr_util_smooth_scales(gamma.ctypes.data, beta.ctypes.data, gamma.size, out.ctypes.data) == 0
    return out


def test_smoothing_rule_library_equals_emulation():
    for seed, outl in ((0, ()), (1, OUTLIERS), (2, ((3, 2000.0), (4, 0.5), (5, 1.45)))):
        gamma, beta = _ln_affine(1024, seed, outl)
        s = _lib_smooth(gamma, beta)
        np.testing.assert_array_equal(s, smooth_scales(gamma, beta))
        e = np.log2(s)
        assert (e == np.round(e)).all() and s.min() >= 1.0 and s.max() <= 1024.0       # powers of two in [1, 2^10]
        for d, f in outl:
            if f >= 2.0:
                assert s[d] == 2.0 ** min(10, round(np.log2(max(abs(gamma[d]), abs(beta[d])) / np.median(np.maximum(abs(gamma), abs(beta))))))
    gamma, beta = _ln_affine(1024, 1, OUTLIERS)
    s = _lib_smooth(gamma, beta)
    assert s[7] == 64.0 and s[300] == 64.0 and s[555] == 256.0        # x50 -> 2^6, x300 -> 2^8 (round(log2 300) = 8)
    assert (np.delete(s, [7, 300, 555]) == 1.0).all()                   # ordinary channels are left alone
    z = np.zeros(256, dtype=np.float32)
    assert (_lib_smooth(z, z) == 1.0).all()                             # degenerate LayerNorm: nothing to migrate


def test_the_fold_is_exact_in_fp32():
    """(x * gamma / s + beta / s) . (W * s)^T equals (x * gamma + beta) . W^T bit for bit in fp32: s is a power of two, so every
    scaled factor is exact and every product of the matrix product is the same number."""
    for seed, outl in ((3, ()), (4, OUTLIERS)):
        gamma, beta = _ln_affine(1024, seed, outl)
        s = smooth_scales(gamma, beta)
        g = np.random.default_rng(seed + 10)
        x = g.standard_normal((64, 1024)).astype(np.float32)            # normalised rows (x - mean) * rstd
        W = (0.03 * g.standard_normal((384, 1024))).astype(np.float32)
        for d, f in outl:
            W[:, d] /= f                                                 # the compensated columns of a trained model
        y = x * gamma
        y = y + beta
        ys = x * (gamma / s)
        ys = ys + beta / s
        np.testing.assert_array_equal(ys * s, y)                         # the LayerNorm output, exactly divided by s
        Ws = W * s[None, :]
        np.testing.assert_array_equal(Ws / s[None, :], W)
        ref = torch.from_numpy(y) @ torch.from_numpy(W).t()
        got = torch.from_numpy(ys) @ torch.from_numpy(Ws).t()
        assert torch.equal(got, ref)


def _lib_quant(W):
    W = np.ascontiguousarray(W, dtype=np.float32)
    q = np.zeros(W.shape, dtype=np.int8)
    sc = np.zeros(W.shape[0], dtype=np.float32)
    assert _lib().rr_util_quantize_rows_i8(W.ctypes.data, W.shape[0], W.shape[1], q.ctypes.data, sc.ctypes.data) == 0
    return q, sc


def test_host_int8_quantiser_equals_emulation():
    g = np.random.default_rng(5)
    W = (g.standard_normal((300, 768)) * g.uniform(0.01, 3.0, (300, 1))).astype(np.float32)
    W[17] = 0.0
    W[40, 5] = 40.0                                                      # one outlier element sets its row's scale
    q, sc = _lib_quant(W)
    qe, se = quant_rows_i8(torch.from_numpy(W))
    np.testing.assert_array_equal(sc, se.numpy().reshape(-1))
    np.testing.assert_array_equal(q.astype(np.float32), qe.numpy())
    deq = q.astype(np.float32) * sc[:, None]
    assert (np.abs(deq - W) <= 0.5 * sc[:, None] * (1 + 1e-6)).all()   # half a code step


def test_quantiser_edge_cases():
    # amax 127 -> scale exactly 1: halves are ties, rounded to even; the row's minimum -127 stays -127
    row = np.array([127.0, 2.5, 3.5, -2.5, 0.5, 1.5, -0.5, -127.0], dtype=np.float32)
    q, sc = _lib_quant(row[None, :].repeat(2, 0))
    assert sc[0] == 1.0
    assert q[0].tolist() == [127, 2, 4, -2, 0, 2, 0, -127]
    # the clamp: -amax maps to -127 (never -128), whatever the rounding of amax / 127 * (127 / amax)
    g = np.random.default_rng(6)
    W = g.standard_normal((1000, 64)).astype(np.float32) * 7.3
    W[:, 0] = -np.abs(W).max(1) - 1e-3                                   # every row's extreme element is negative
    q, sc = _lib_quant(W)
    assert q.min() >= -127 and q.max() <= 127
    assert (q[:, 0] == -127).all()
    # a zero row: scale 1, codes 0
    q, sc = _lib_quant(np.zeros((3, 128), dtype=np.float32))
    assert (sc == 1.0).all() and (q == 0).all()
    qe, se = quant_rows_i8(torch.zeros(3, 128))
    assert (se == 1.0).all() and (qe == 0).all()
    # the emulation rounds ties to even too
    qe, _ = quant_rows_i8(torch.from_numpy(row)[None, :])
    assert qe[0].tolist() == [127, 2, 4, -2, 0, 2, 0, -127]


def test_a_nan_or_inf_in_a_weight_row_makes_its_scale_non_finite():
    """fmaxf drops a NaN from the row maximum and fminf(fmaxf(v, -127), 127) turns one into -127: the row (0.5, NaN, -0.25, 0.1)
    used to pack as scale 0.5 / 127, codes 127, -127, -64, 25 — the most negative code under a finite scale.  The scale multiplies
    the whole output column in the GEMM epilogue, so a row that holds a NaN or an inf gets a NaN scale (the column is then
    non-finite and the range guard sees it); every other row packs exactly as before."""
    q, sc = _lib_quant(np.array([[0.5, np.nan, -0.25, 0.1], [0.5, 0.25, -0.25, 0.1]], dtype=np.float32))
    assert not np.isfinite(sc[0]) and sc[1] == np.float32(0.5) * np.float32(1.0 / 127.0)
    assert q[1].tolist() == [127, 64, -64, 25]
    g = np.random.default_rng(9)
    W = (g.standard_normal((64, 256)) * g.uniform(0.01, 3.0, (64, 1))).astype(np.float32)
    bad = W.copy()
    bad[3, 0], bad[10, 255], bad[20, 7], bad[33, 100], bad[33, 101] = np.nan, np.nan, np.inf, -np.inf, np.nan
    rows = [3, 10, 20, 33]
    q0, s0 = _lib_quant(W)
    q1, s1 = _lib_quant(bad)
    assert not np.isfinite(s1[rows]).any()
    keep = np.setdiff1d(np.arange(64), rows)
    np.testing.assert_array_equal(s1[keep].view(np.int32), s0[keep].view(np.int32))      # bit for bit
    np.testing.assert_array_equal(q1[keep], q0[keep])
    qe, se = quant_rows_i8(torch.from_numpy(W))
    np.testing.assert_array_equal(s1[keep], se.numpy().reshape(-1)[keep])
    np.testing.assert_array_equal(q1[keep].astype(np.float32), qe.numpy()[keep])
