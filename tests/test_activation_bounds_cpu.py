"""The judge of tests/test_gpu_activations.py (activation_check.judge) can fail: it accepts fp32 emulations of the kernels' own
formulas and rejects each of them with one constant changed in its fourth significant digit — for bf16 and for fp16 outputs, where
half a 16-bit ulp of rounding is three orders above the fp32 error being judged (the dense grid finds the values whose rounding
flips).  Runs without a GPU."""
import numpy as np
import pytest
import torch

import activation_check as AC

DTYPES = [torch.bfloat16, torch.float16]


def _x():
    return AC.grid_x()


def _verdict(fn, y32, dtype):
    x = _x()
    return AC.judge(fn, x, AC.to16(y32.reshape(x.shape), dtype), dtype)


def test_grid_is_exact_in_fp32():
    x = _x()
    assert x.numel() == 102_400 and torch.equal(x.float().double(), x)
    k = torch.tensor(AC.KS, dtype=torch.float32)[:, None] + (torch.arange(AC.NFRAC) % 4096).float()[None, :] / 4096
    assert torch.equal(k.double(), x)                      # the fp32 sum k + j / 4096 a kernel forms is that value


def test_constants_match_the_source_text():
    (scalar, clamp1), (packed, clamp2) = AC.source_gelu_constants()
    assert scalar == AC.GELU5_COEFFS and packed == AC.GELU5_COEFFS
    assert clamp1 == AC.GELU_CLAMP and clamp2 == AC.GELU_CLAMP
    assert AC.source_exp_constants() == (2.0, AC.QGELU_SLOPE)


@pytest.mark.parametrize("dtype", DTYPES)
def test_judge_accepts_the_kernels_formulas(dtype):
    x = _x().numpy()
    for ulps in (0, 4, -4):                                # a hardware exp2 a few ulp off is still inside
        v = _verdict("gelu", AC.emulate_gelu(x, exp2_ulps=ulps), dtype)
        assert v["ok"] and v["worst"] > 0.9, v              # > 0.9: the bound is tight, an output may sit half an ulp off
    for fn, y in (("tanh", AC.emulate_tanh(x)), ("qgelu", AC.emulate_qgelu(x))):
        v = _verdict(fn, y, dtype)
        assert v["ok"] and v["worst"] > 0.9, (fn, v)


def test_fp32_error_of_the_degree5_chain_is_inside_the_stated_bound():
    x = _x()
    y = torch.from_numpy(AC.emulate_gelu(x.numpy())).double()
    f = AC.f64("gelu", x)
    err = (y - f).abs()
    assert err.max().item() <= 6.4e-7                      # csrc/rr_common.h
    big = f.abs() >= 1e-3
    assert (err[big] / f[big].abs()).max().item() <= 2.8e-4


def _mutated(i, value):
    c = list(AC.GELU5_COEFFS)
    assert abs(c[i] - value) < 5e-4 * abs(c[i]) and c[i] != value
    c[i] = value
    return tuple(c)


MUTANTS = [
    ("gelu", "coefficient 4 up", lambda x: AC.emulate_gelu(x, coeffs=_mutated(3, -0.4601))),
    ("gelu", "coefficient 4 down", lambda x: AC.emulate_gelu(x, coeffs=_mutated(3, -0.4598))),
    ("gelu", "clamp 5.0", lambda x: AC.emulate_gelu(x, clamp=5.0)),
    ("qgelu", "slope 1.700", lambda x: AC.emulate_qgelu(x, slope=1.700)),
    ("tanh", "exp(2.001 x)", lambda x: AC.emulate_tanh(x, arg_scale=2.001)),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fn,what,mutant", MUTANTS, ids=[m[1].replace(" ", "_") for m in MUTANTS])
def test_judge_rejects_a_constant_off_in_its_fourth_digit(fn, what, mutant, dtype):
    v = _verdict(fn, mutant(_x().numpy()), dtype)
    assert not v["ok"] and v["worst"] > 1.0, (what, v)


def test_judge_rejects_a_nan_and_a_wrong_function_on_one_lane():
    x = _x()
    for dtype in DTYPES:
        good = AC.to16(AC.emulate_gelu(x.numpy()).reshape(x.shape), dtype)
        bad = good.clone()
        bad[3, 17] = float("nan")
        assert not AC.judge("gelu", x, bad, dtype)["ok"]
        bad = good.clone()
        bad[:, 5::64] = AC.to16(AC.emulate_qgelu(x.numpy()).reshape(x.shape), dtype)[:, 5::64]   # one lane's column
        assert not AC.judge("gelu", x, bad, dtype)["ok"]


def test_e4m3_judge_accepts_the_formula_and_rejects_the_mutants():
    x = _x()

    def codes(y32):
        v = torch.from_numpy(np.ascontiguousarray(y32.reshape(x.shape))) * 8.0
        return v.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)

    v = AC.judge_e4m3(x, codes(AC.emulate_gelu(x.numpy())))
    assert v["ok"], v
    # (the clamp mutant moves gelu by 1e-6 at most, where the e4m3 step is 2^-9 / 8: no grid value flips; the 16-bit outputs catch it)
    for what, co in (("up", _mutated(3, -0.4601)), ("down", _mutated(3, -0.4598))):
        assert not AC.judge_e4m3(x, codes(AC.emulate_gelu(x.numpy(), coeffs=co)))["ok"], what
    off = codes(AC.emulate_gelu(x.numpy())).clone()
    off[7, 100] += 1                                       # a neighbouring code away from a boundary
    assert not AC.judge_e4m3(x, off)["ok"]
