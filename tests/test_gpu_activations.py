"""GPU: the FUNCTION every GEMM epilogue applies after the product (erf-GELU, tanh, quick-GELU), on pre-activations the test knows
to the bit.  A[m, 0] = k_m (the integers -12 .. 12 in turn), W[n, 0] = 1, every other operand element 0 and bias[n] = (n mod
4096) / 4096 make A W^T + b = k_m + j_n / 4096 exactly in fp32 whatever the summation order and the operand type (bf16, fp16,
e4m3, int8: small integers are exact in all four; scales are 1 / NULL), so every kernel is handed the same 102 400 fp32 numbers
and its 16-bit outputs are judged against the float64 function with activation_check.judge (half an output ulp + the fp32
allowance of the formula, derived there; tests/test_activation_bounds_cpu.py shows the judge rejecting a constant that is off in
its fourth digit).  Because the input is exact, all kernels must also agree with each other to the bit, and a row's values may not
depend on where the row lies in a tile.  A second bias holds the special values (signed zeros, the clamp 5.7 and its neighbours,
overflow ranges, infinities, NaN, the smallest normal and a subnormal)."""
import math

import pytest
import torch

import activation_check as AC
from helpers import record_margin

pytestmark = pytest.mark.gpu

N, K = 4096, 128
M_SMALL = 300              # 25 x 12: two row tiles of 256, the last one ragged
M_RING = 8200              # 25 x 328: 33 x 16 = 528 tiles of 256 x 256 (>= 512: the 8-bit ring; >= 128: the 16-bit one), ragged
T16 = {0: torch.bfloat16, 1: torch.float16}
TNAME = {0: "bf16", 1: "fp16"}
# rr_set_gemm_variant codes per operand type (gemm_bf16.hip rr_launch_gemm_fold: the fp16 instantiations are the production
# configurations only, 1 and 3 answer RR_ERR_BAD_SHAPE there)
VARIANTS = {0: [0, 1, 2, 3, 10, 11, 12, 14], 1: [0, 2, 10, 11, 12, 14]}


@pytest.fixture(scope="module")
def lib():
    import rmr_amd  # noqa: F401
    from rmr_amd import _lib
    return _lib.load()       # raises if librerank_mi355.so is missing: no fallback


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _operands(M, kind, zero_rows=False):
    """A [M, K] with A[m, 0] = KS[m % 25] (0 when zero_rows), W [N, K] with W[n, 0] = 1, in the operand type `kind`."""
    k = torch.tensor(AC.KS, dtype=torch.float32)[torch.arange(M) % 25]
    A = torch.zeros(M, K)
    if not zero_rows:
        A[:, 0] = k
    W = torch.zeros(N, K)
    W[:, 0] = 1.0
    if kind == "e4m3":
        A, W = A.to(torch.float8_e4m3fn), W.to(torch.float8_e4m3fn)
        assert torch.equal(A.float()[:, 0], torch.zeros(M) if zero_rows else k)
        return A.view(torch.uint8).cuda(), W.view(torch.uint8).cuda()
    if kind == "i8":
        return A.to(torch.int8).cuda(), W.to(torch.int8).cuda()
    return A.to(kind).cuda(), W.to(kind).cuda()


def _grid_bias():
    return ((torch.arange(N) % AC.NFRAC).float() / AC.NFRAC).cuda()


def _rows_repeat(out, what):
    """Rows with the same k_m are identical within the launch: the value may not depend on the row's place in a tile or lane."""
    M = out.shape[0]
    assert M % 25 == 0
    v = out.view(torch.int16) if out.dtype != torch.uint8 else out
    assert bool((v.view(M // 25, 25, -1) == v[:25][None]).all()), f"{what}: rows of one k differ within a launch"
    return out[:25]


_JUDGED = {}       # (fn, dt) -> the 16-bit [25, N] block every kernel must reproduce to the bit


def _judge_and_compare(fn, dt, out, what):
    """Assertion 1 (accuracy on the grid) and 2 (same bits as every other kernel, rows independent of their place)."""
    blk = _rows_repeat(out, what)
    v = AC.judge(fn, AC.grid_x(), blk.cpu(), T16[dt])
    print(f"{what}: worst err / bound {v['worst']:.5f} at x = {v['where']!r}, max |err| {v['max_abs']:.3e}, "
          f"max rel (|f| >= 1e-3) {v['max_rel']:.3e}")
    assert v["ok"], (what, v)
    ref = _JUDGED.setdefault((fn, dt), blk.clone())
    same = ref.view(torch.int16) == blk.view(torch.int16)
    assert bool(same.all()), f"{what}: {int((~same).sum())} of {same.numel()} outputs differ in their bits from the first kernel judged"
    return v


def _gemm16(lib, A, W, bias, M, epi, dt):
    out = torch.full((M, N), float("nan"), device="cuda", dtype=T16[dt])
    rc = lib.rr_op_gemm_bf16(A.data_ptr(), W.data_ptr(), bias.data_ptr(), M, N, K, epi, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("epi", [1, 3, 5])
@pytest.mark.parametrize("dt", [0, 1])
def test_gemm16_every_variant_on_the_grid(lib, dt, epi):
    """rr_op_gemm_bf16: the five textual copies of the activation switch (two-stage direct 0 / 1 / 2 / 3 and LDS-staged 10, half-tile
    ring direct 11 and staged 12, persistent ring 14 with the packed GELU chain) and the shape heuristic at a ring-sized M.
    Measured on an MI355X, every variant giving the same bits — worst error over bound (1 = the bound; half an output ulp alone is
    up to ~0.998 of it): erf-GELU 0.99998 [`profiles/activations_parity_margins.json` "activations/gelu/bf16" "worst_err_over_bound"]
    (bf16) and 0.99981 [`profiles/activations_parity_margins.json` "activations/gelu/fp16" "worst_err_over_bound"] (fp16), tanh
    0.99965 [`profiles/activations_parity_margins.json` "activations/tanh/bf16" "worst_err_over_bound"] and
    0.99807 [`profiles/activations_parity_margins.json` "activations/tanh/fp16" "worst_err_over_bound"], quick-GELU
    0.99918 [`profiles/activations_parity_margins.json` "activations/qgelu/bf16" "worst_err_over_bound"] and
    0.99996 [`profiles/activations_parity_margins.json` "activations/qgelu/fp16" "worst_err_over_bound"]: the derived tanh and
    quick-GELU allowances hold on the hardware.  -inf gives NaN in both GELUs ("activations/minus_inf/..." in the same record)."""
    fn = AC.FUNCTIONS[epi]
    bias = _grid_bias()
    assert lib.rr_set_op_dtype(dt) == 0
    try:
        worst = None
        for variant, M in [(v, M_SMALL) for v in VARIANTS[dt]] + [(-1, M_RING), (-1, M_SMALL)]:
            A, W = _operands(M, T16[dt])
            assert lib.rr_set_gemm_variant(variant) == 0
            rc, out = _gemm16(lib, A, W, bias, M, epi, dt)
            assert rc == 0, (variant, M)
            v = _judge_and_compare(fn, dt, out, f"gemm16 {TNAME[dt]} {fn} variant {variant} M {M}")
            worst = v if worst is None or v["worst"] > worst["worst"] else worst
        record_margin(f"activations/{fn}/{TNAME[dt]}", max_abs=worst["max_abs"], max_rel_where_absf_ge_0p001=worst["max_rel"],
                      worst_err_over_bound=worst["worst"], at_x=worst["where"], bits_equal_across_variants=True)
        for variant in sorted(set(VARIANTS[0]) - set(VARIANTS[dt])):     # not built for this operand type: an error, not a fallback
            assert lib.rr_set_gemm_variant(variant) == 0
            A, W = _operands(25, T16[dt])
            assert _gemm16(lib, A, W, bias, 25, epi, dt)[0] != 0
    finally:
        lib.rr_set_gemm_variant(-1)
        lib.rr_set_op_dtype(0)


@pytest.mark.parametrize("dt", [0, 1])
def test_lnfold_gelu_on_the_grid(lib, dt):
    """rr_op_gemm_lnfold epilogue 1 with stats = (0, 1): rstd (acc - mean csum) + dvec = acc + dvec exactly; the two-stage kernel and
    the persistent ring's folded instantiation."""
    bias = _grid_bias()
    csum = torch.full((N,), 3.25, device="cuda")
    assert lib.rr_set_op_dtype(dt) == 0
    try:
        for M in (M_SMALL, M_RING):
            A, W = _operands(M, T16[dt])
            stats = torch.tensor([0.0, 1.0]).repeat(M, 1).contiguous().cuda()
            out = torch.full((M, N), float("nan"), device="cuda", dtype=T16[dt])
            assert lib.rr_op_gemm_lnfold(A.data_ptr(), W.data_ptr(), bias.data_ptr(), csum.data_ptr(), stats.data_ptr(), M, N, K, 1,
                                         out.data_ptr(), _stream()) == 0
            torch.cuda.synchronize()
            _judge_and_compare("gelu", dt, out, f"lnfold {TNAME[dt]} M {M}")
    finally:
        lib.rr_set_op_dtype(0)


def _gemm8(lib, entry, A, W, bias, M, dt):
    out = torch.full((M, N), float("nan"), device="cuda", dtype=T16[dt])
    if entry == "fp8":
        rc = lib.rr_op_gemm_fp8(A.data_ptr(), W.data_ptr(), bias.data_ptr(), 1.0, M, N, K, 1, out.data_ptr(), _stream())
    elif entry == "fp8_rc":
        rc = lib.rr_op_gemm_fp8_rc(A.data_ptr(), W.data_ptr(), bias.data_ptr(), 0, 0, M, N, K, 1, out.data_ptr(), _stream())
    else:
        ones_m, ones_n = torch.ones(M, device="cuda"), torch.ones(N, device="cuda")        # scale vectors given, all 1
        rc = lib.rr_op_gemm_i8_rc(A.data_ptr(), W.data_ptr(), bias.data_ptr(), ones_m.data_ptr(), ones_n.data_ptr(), M, N, K, 1,
                                  out.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("entry", ["fp8", "fp8_rc", "i8_rc"])
@pytest.mark.parametrize("dt", [0, 1])
def test_gemm8_gelu_on_the_grid(lib, dt, entry):
    """The e4m3 and int8 GEMMs' erf-GELU -> 16 bit, two-stage kernel (small M) and persistent ring (528 tiles)."""
    bias = _grid_bias()
    assert lib.rr_set_op_dtype(dt) == 0
    try:
        for M in (M_SMALL, M_RING):
            A, W = _operands(M, "i8" if entry == "i8_rc" else "e4m3")
            rc, out = _gemm8(lib, entry, A, W, bias, M, dt)
            assert rc == 0
            _judge_and_compare("gelu", dt, out, f"{entry} {TNAME[dt]} M {M}")
    finally:
        lib.rr_set_op_dtype(0)


def test_gelu_to_e4m3_on_the_grid(lib):
    """rr_op_gemm_fp8_gelu_e4m3 (ring only) under out_mul 8: the byte is the nearest e4m3 code of 8 gelu(x), or the neighbouring one
    where 8 (gelu(x) +- E) straddles a rounding boundary."""
    A, W = _operands(M_RING, "e4m3")
    bias = _grid_bias()
    out = torch.full((M_RING, N), 0x7f, device="cuda", dtype=torch.uint8)
    assert lib.rr_op_gemm_fp8_gelu_e4m3(A.data_ptr(), W.data_ptr(), bias.data_ptr(), 0, 0, 8.0, M_RING, N, K, out.data_ptr(),
                                        _stream()) == 0
    torch.cuda.synchronize()
    blk = _rows_repeat(out, "gelu -> e4m3")
    v = AC.judge_e4m3(AC.grid_x(), blk.cpu(), 8.0)
    print("gelu -> e4m3:", v)
    record_margin("activations/gelu/e4m3_out_mul_8", off_nearest_code=v["off_nearest"], outside_allowance=v["n_bad"], n=blk.numel())
    assert v["ok"], v


# ---- special values ----
def _specials():
    f = torch.float32
    c = torch.tensor(5.7, dtype=f)
    near = [torch.nextafter(c, torch.tensor(math.inf, dtype=f)).item(), torch.nextafter(c, torch.tensor(0.0, dtype=f)).item()]
    vals = [0.0, -0.0, c.item(), -c.item(), near[0], near[1], -near[0], -near[1], 20.0, -20.0, 88.0, -88.0, 1e4, -1e4, 7e4, -1e30,
            math.inf, -math.inf, math.nan, 2.0 ** -126, 2.0 ** -130]
    return torch.tensor(vals, dtype=f)


def _special_bias():
    s = _specials()
    return s[torch.arange(N) % s.numel()].cuda(), s.numel()


def _check_specials(fn, dtype, out, what, minus_inf_key=None):
    """out [M, N] 16-bit, every row the activation of the special bias.  NaN -> NaN; +inf -> +inf (tanh: 1); -inf -> -1 (tanh), the
    limit 0 or NaN (the GELUs); a finite x whose float64 value overflows the output type -> that infinity; every other finite x
    inside the grid's bound."""
    s = _specials().cuda()
    ns = s.numel()
    got_all = out.float()
    first = got_all[0]
    same = (got_all == first) | (torch.isnan(got_all) & torch.isnan(first))
    assert bool(same.all()), f"{what}: rows differ"
    got = first.view(-1)[: (N // ns) * ns].view(N // ns, ns)
    same = (got == got[0]) | (torch.isnan(got) & torch.isnan(got[0]))
    assert bool(same.all()), f"{what}: the same special gives different results in different columns"
    got = got[0].double().cpu()
    s = s.cpu()
    for i in range(ns):
        x, g = s[i].item(), got[i].item()
        tag = f"{what}: f({x!r}) = {g!r}"
        if math.isnan(x):
            assert math.isnan(g), tag
        elif x == math.inf:
            assert g == (1.0 if fn == "tanh" else math.inf), tag
        elif x == -math.inf:
            if fn == "tanh":
                assert g == -1.0, tag
            else:
                assert math.isnan(g) or g == 0.0, tag
                if minus_inf_key:
                    record_margin(minus_inf_key, value="NaN" if math.isnan(g) else repr(g))
        else:
            xs = torch.tensor([x], dtype=torch.float64)
            want = AC.f64(fn, xs).to(dtype)
            if not bool(torch.isfinite(want).all()):
                assert g == want.item(), tag
            else:
                assert AC.judge(fn, xs, torch.tensor([g], dtype=torch.float64), dtype)["ok"], tag


@pytest.mark.parametrize("epi", [1, 3, 5])
@pytest.mark.parametrize("dt", [0, 1])
def test_gemm16_specials(lib, dt, epi):
    fn = AC.FUNCTIONS[epi]
    bias, _ = _special_bias()
    assert lib.rr_set_op_dtype(dt) == 0
    try:
        for variant, M in [(v, 50) for v in VARIANTS[dt]] + [(-1, M_RING)]:
            A, W = _operands(M, T16[dt], zero_rows=True)
            assert lib.rr_set_gemm_variant(variant) == 0
            rc, out = _gemm16(lib, A, W, bias, M, epi, dt)
            assert rc == 0, (variant, M)
            _check_specials(fn, T16[dt], out, f"gemm16 {TNAME[dt]} {fn} variant {variant} M {M}",
                            minus_inf_key=f"activations/minus_inf/{fn}/{TNAME[dt]}" if variant == 0 else None)
    finally:
        lib.rr_set_gemm_variant(-1)
        lib.rr_set_op_dtype(0)


@pytest.mark.parametrize("dt", [0, 1])
def test_lnfold_and_gemm8_specials(lib, dt):
    bias, _ = _special_bias()
    csum = torch.full((N,), 3.25, device="cuda")
    assert lib.rr_set_op_dtype(dt) == 0
    try:
        for M in (50, M_RING):
            A, W = _operands(M, T16[dt], zero_rows=True)
            stats = torch.tensor([0.0, 1.0]).repeat(M, 1).contiguous().cuda()
            out = torch.full((M, N), float("nan"), device="cuda", dtype=T16[dt])
            assert lib.rr_op_gemm_lnfold(A.data_ptr(), W.data_ptr(), bias.data_ptr(), csum.data_ptr(), stats.data_ptr(), M, N, K, 1,
                                         out.data_ptr(), _stream()) == 0
            torch.cuda.synchronize()
            _check_specials("gelu", T16[dt], out, f"lnfold {TNAME[dt]} M {M}")
            for entry in ("fp8", "fp8_rc", "i8_rc"):
                A8, W8 = _operands(M, "i8" if entry == "i8_rc" else "e4m3", zero_rows=True)
                rc, out = _gemm8(lib, entry, A8, W8, bias, M, dt)
                assert rc == 0
                _check_specials("gelu", T16[dt], out, f"{entry} {TNAME[dt]} M {M}")
    finally:
        lib.rr_set_op_dtype(0)


def test_gelu_to_e4m3_specials(lib):
    """e4m3 has no infinity and the epilogue saturates: +inf and 7e4 -> 448; NaN -> the NaN code; -inf -> NaN or 0."""
    bias, ns = _special_bias()
    A, W = _operands(M_RING, "e4m3", zero_rows=True)
    out = torch.zeros((M_RING, N), device="cuda", dtype=torch.uint8)
    assert lib.rr_op_gemm_fp8_gelu_e4m3(A.data_ptr(), W.data_ptr(), bias.data_ptr(), 0, 0, 8.0, M_RING, N, K, out.data_ptr(),
                                        _stream()) == 0
    torch.cuda.synchronize()
    val = out.view(torch.float8_e4m3fn).float()
    same = (val == val[0]) | (torch.isnan(val) & torch.isnan(val[0]))
    assert bool(same.all()), "rows differ"
    s = _specials()
    got_b = out[0, :ns].cpu()
    got = val[0, :ns].double().cpu()
    for i in range(ns):
        x, g = s[i].item(), got[i].item()
        tag = f"gelu -> e4m3: f({x!r}) = {g!r}"
        if math.isnan(x):
            assert math.isnan(g), tag
        elif x == math.inf:
            assert g == 448.0, tag
        elif x == -math.inf:
            assert math.isnan(g) or g == 0.0, tag
        else:
            assert AC.judge_e4m3(torch.tensor([x], dtype=torch.float64), got_b[i:i + 1], 8.0)["ok"], tag
