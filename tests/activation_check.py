"""The judge of the GEMM epilogues' activation functions (tests/test_gpu_activations.py) and the fp32 emulations that prove it
can fail (tests/test_activation_bounds_cpu.py).  Not a test module.

A 16-bit output `got` of a function f at the exactly known fp32 pre-activation x is accepted when
    |got - f(x)| <= ulp16(f(x)) / 2 + E_f(x),
f in float64, ulp16 the spacing of the output type at f(x) (fp16: 2^-24 below 2^-14; bf16: 2^-133 below 2^-126): half an ulp is
what the round-to-nearest cast of an exact value may cost, E_f is what the fp32 evaluation in the kernel may cost:
  * erf-GELU   E = 7.5e-7, and where |f| >= 1e-3 the smaller of that and 3.0e-4 |f|: the bounds csrc/rr_common.h states for the
               degree-5 fit (6.4e-7 absolute over [-12, 12], 2.8e-4 relative where |gelu| >= 1e-3) plus 1e-7 for the hardware exp2
               (one ulp of 2^p moves z Phi(-z) by at most max z Phi(-z) * 2^-23 = 2.0e-8: five ulp);
  * tanh       E = 6e-7: 1 - 2 / (exp(2x) + 1) in fp32 with correctly rounded exp and division is 1.8e-7 off on the grid; a 1-ulp
               rcp adds at most 2.4e-7, a 1-ulp exp2 with its rounded argument at most 0.9e-7;
  * quick-GELU E = 3e-6 |f|: x / (1 + exp(-1.702 x)) in fp32 is 1.13e-6 relative off on the grid, plus up to 1.4e-6 from the
               argument rounding of exp(-1.702 x) at |x| = 12 and the rcp ulp.
The grid: x = k + j / 4096, k = -12 .. 12, j = 0 .. 4095 (102 400 values, each exact in fp32)."""
import math
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reranking-multimodal-retrievers_amd", "csrc")

# csrc/rr_common.h gelu_erf_fast, RR_GELU_DEGREE 5, highest power first — DATA here; test_activation_bounds_cpu.py reads the
# source text and compares, so that the two cannot drift apart
GELU5_COEFFS = (-4.733084352e-04, 7.084545679e-03, -5.182733759e-02, -4.599924982e-01, -1.150787830e+00, -1.000037670e+00)
GELU_CLAMP = 5.7
QGELU_SLOPE = 1.702

KS = list(range(-12, 13))
NFRAC = 4096
FUNCTIONS = {1: "gelu", 3: "tanh", 5: "qgelu"}      # epilogue codes of rr_op_gemm_bf16


def grid_x():
    """[25, 4096] float64: x[m, n] = k_m + n / 4096."""
    return torch.tensor(KS, dtype=torch.float64)[:, None] + torch.arange(NFRAC, dtype=torch.float64)[None, :] / NFRAC


def f64(fn, x):
    x = x.double()
    if fn == "gelu":
        return 0.5 * x * torch.erfc(-x / math.sqrt(2.0))       # x Phi(x); erfc keeps the negative tail's digits
    if fn == "tanh":
        return torch.tanh(x)
    if fn == "qgelu":
        return x * torch.sigmoid(QGELU_SLOPE * x)
    raise KeyError(fn)


def ulp16(f, dtype):
    """Spacing of `dtype` (torch.bfloat16 / torch.float16) at the float64 values f."""
    mant, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    _, e = torch.frexp(f.abs().clamp_min(2.0 ** -200))         # |f| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(f), (e - 1).clamp_min(emin) - mant)


def allowance(fn, f):
    """E_f at the float64 function values f."""
    a = f.abs()
    if fn == "gelu":
        return torch.where(a >= 1e-3, torch.minimum(torch.full_like(a, 7.5e-7), 3.0e-4 * a), torch.full_like(a, 7.5e-7))
    if fn == "tanh":
        return torch.full_like(a, 6e-7)
    if fn == "qgelu":
        return 3e-6 * a
    raise KeyError(fn)


def judge(fn, x, got, dtype):
    """x: float64 pre-activations (finite); got: the 16-bit outputs (any float tensor holding them exactly), same shape.
    Returns a dict: ok (bool), worst = max |err| / bound, where = x at that maximum, max_abs = max |got - f|,
    max_rel = max |got - f| / |f| over |f| >= 1e-3."""
    x = x.double()
    f = f64(fn, x)
    g = got.double()
    err = (g - f).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, float("inf")))
    ratio = err / (ulp16(f, dtype) / 2 + allowance(fn, f))
    i = int(ratio.argmax())
    big = f.abs() >= 1e-3
    return dict(ok=bool((ratio <= 1.0).all()), worst=float(ratio.flatten()[i]), where=float(x.flatten()[i]),
                max_abs=float(err.max()), max_rel=float((err[big] / f[big].abs()).max()) if bool(big.any()) else 0.0)


def _e4m3_round(v):
    """float64 v -> the nearest e4m3fn value (ties to even), saturating at +-448, as float64."""
    v = v.clamp(-448.0, 448.0)
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -200))
    step = torch.ldexp(torch.ones_like(v), (e - 1).clamp_min(-6) - 3)
    return torch.round(v / step) * step                        # torch.round: half to even


def judge_e4m3(x, got_bytes, out_mul=8.0):
    """erf-GELU written as e4m3 bytes of clamp(out_mul * gelu(x), +-448): the byte is the round-to-nearest code of out_mul f(x) or
    differs from it only where out_mul (f(x) +- E) straddles a rounding boundary (then it is a neighbouring code).  Values are
    compared, so +0 and -0 are one code.  Returns ok, the number of outputs that differ from the nearest code, and the first x
    that fails."""
    x = x.double()
    f = f64("gelu", x)
    E = allowance("gelu", f)
    got = got_bytes.view(torch.float8_e4m3fn).double()
    mid, lo, hi = _e4m3_round(out_mul * f), _e4m3_round(out_mul * (f - E)), _e4m3_round(out_mul * (f + E))
    ok = (got == mid) | (got == lo) | (got == hi)
    bad = (~ok).nonzero()
    return dict(ok=bool(ok.all()), off_nearest=int((got != mid).sum()), n_bad=int((~ok).sum()),
                first_bad=float(x.flatten()[int((~ok).flatten().nonzero()[0])]) if len(bad) else None)


# ---- fp32 emulations of the kernels' formulas (numpy; a fused multiply-add is the float64 product and sum rounded once to fp32:
# the product of two fp32 values is exact in float64) ----
def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32)


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate_gelu(x, coeffs=GELU5_COEFFS, clamp=GELU_CLAMP, exp2_ulps=0):
    """csrc/rr_common.h gelu_erf_fast in fp32: z = min(|x|, clamp), p = Horner(coeffs, z) with FMAs, max(x, 0) - z exp2(p)."""
    x = _f32(x)
    z = np.minimum(np.abs(x), np.float32(clamp))
    p = np.full_like(z, np.float32(coeffs[0]))
    for c in coeffs[1:]:
        p = _fma(p, z, np.full_like(z, np.float32(c)))
    e = np.exp2(p.astype(np.float64)).astype(np.float32)
    if exp2_ulps:
        e = (e.view(np.int32) + np.int32(exp2_ulps)).view(np.float32)
    return _fma(-z, e, np.maximum(x, np.float32(0)))


def emulate_tanh(x, arg_scale=2.0):
    """csrc/gemm_bf16.hip tanh_fast: 1 - 2 / (exp(2 x) + 1)."""
    x = _f32(x)
    t = _f32(np.float32(arg_scale).astype(np.float64) * x)
    e = np.exp(t.astype(np.float64)).astype(np.float32)
    r = (1.0 / (e.astype(np.float64) + 1.0).astype(np.float32).astype(np.float64)).astype(np.float32)
    return _fma(np.full_like(r, np.float32(-2.0)), r, np.ones_like(r))


def emulate_qgelu(x, slope=QGELU_SLOPE):
    """csrc/gemm_bf16.hip qgelu_fast: x / (1 + exp(-slope x))."""
    x = _f32(x)
    t = _f32(np.float32(-slope).astype(np.float64) * x)
    e = np.exp(t.astype(np.float64)).astype(np.float32)
    r = (1.0 / (1.0 + e.astype(np.float64)).astype(np.float32).astype(np.float64)).astype(np.float32)
    return _f32(x.astype(np.float64) * r)


def to16(y, dtype):
    """fp32 numpy values -> torch 16-bit tensor, round to nearest even (torch's cast)."""
    return torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).to(dtype)


# ---- the constants as the source text has them ----
def source_gelu_constants():
    """(coefficients highest power first, clamp) of gelu_erf_fast and of gelu_erf_fast2 (RR_GELU_DEGREE 5 branches)."""
    with open(os.path.join(CSRC, "rr_common.h")) as fh:
        src = fh.read()
    num = r"(-?\d+\.\d+(?:e[+-]?\d+)?)f"
    a = src.index("float gelu_erf_fast(float x)")
    b = src.index("f32x2 gelu_erf_fast2(f32x2 x)")
    scalar, packed = src[a:b], src[b:src.index("return __builtin_elementwise_fma(-z, e, m)")]
    out = []
    for body, first, step in ((scalar, r"float p = " + num, r"fmaf\(p, z, " + num + r"\)"),
                              (packed, r"f32x2 p = \{" + num, r"__builtin_elementwise_fma\(p, z, f32x2\{" + num)):
        deg5 = body[body.index("#else"):body.index("#endif")]
        co = [float(re.search(first, deg5).group(1))] + [float(m) for m in re.findall(step, deg5)]
        clamps = {float(m) for m in re.findall(r"fminf\(fabsf\(x(?:\.[xy])?\), " + num + r"\)", body)}
        assert len(clamps) == 1, clamps
        out.append((tuple(co), clamps.pop()))
    return out


def source_exp_constants():
    """(argument scale of tanh_fast's exp, slope of qgelu_fast) from csrc/gemm_bf16.hip."""
    with open(os.path.join(CSRC, "gemm_bf16.hip")) as fh:
        src = fh.read()
    t = re.search(r"float tanh_fast\(float x\) \{ return 1\.0f - 2\.0f \* __builtin_amdgcn_rcpf\(__expf\((\d+\.\d+)f \* x\) \+ 1\.0f\); \}", src)
    q = re.search(r"float qgelu_fast\(float x\) \{ return x \* __builtin_amdgcn_rcpf\(1\.0f \+ __expf\(-(\d+\.\d+)f \* x\)\); \}", src)
    return float(t.group(1)), float(q.group(1))
