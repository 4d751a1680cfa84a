"""Addressing of every kernel family once a buffer no longer fits 32 bits (more than 2^32 bytes, or 2^31 16-bit elements): the
regime of a forward over more than ~1 000 pairs at S = 512.

Audit (read before the first run): every expression of csrc/*.hip that forms an address or an element count from a row / pair /
sequence index, its width, and what bounds it.  "64" = size_t / long long arithmetic (wraps beyond any memory).

  gemm_bf16.hip, gemm_fp8.hip (all kernels)
    tile origin A + (size_t) m0 * lda, W + (size_t) n0 * ldw, + (size_t) tk * BK           64 (scalar base of the LDS-DMA)
    in-tile byte offsets a_off / w_off / so_a* / so_b* = min(r, M-1-m0) * ld (+ chunk)     uint32; r < 256, so < 2^32 while a row
                                                                                            is shorter than 16 MiB (ld < 2^23 el.)
    epilogue rows C / resid / x16 / lo / r_hi / r_lo at (size_t) gm * ld + col             64
    lo8_pair_offset(r, col, ld) (rr_common.h), part[(size_t) gm * nparts + grp], stats[gm] 64; gm is an int row index
    m0, gm, tiles_m * tiles_n (nwg), tile ids                                              int: wrap beyond 2^31 rows / tiles
  attention_bf16.hip
    q / k / v / out origins ((size_t) b * Tq + row) * stride, (size_t) b * Tk * kv_stride   64
    key_bias[(size_t) b * Tk + key], dense_bias + ((size_t) b * Tq + row) * dense_ld        64
    in-sequence LDS-DMA offsets ro0 / ro1 = min(key, Tk-1) * kv_stride * 2                  uint32; the host refuses
                                                                                            Tk * kv_stride * 2 >= 2^32 (both launchers)
    segments: r0 * stride with r0 = seg_row0 (long long), host and device                  64
    nblk, blk0[], flags[blockIdx.x]                                                         int; the host refuses nblk > 2^31 - 1
  elementwise.hip
    row kernels (layernorm*, embed_ln, ce_embed_ln, vit_embed_ln, li_normalize, cls_heads): (size_t) row * cols,
      ((size_t) p * T + t) * D, (size_t) p * T * cols                                       64; row = blockIdx.x * 4 + wave is an int
    fusion_adj*: (size_t) b * (Tq + Tc) * ld, t.off[] long long                             64
    cast16, gather_rows, split_residual_value, quant_e4m3, amax, vit_im2col: size_t i = (size_t) blockIdx.x * blockDim.x + tid
                                                                                            64; grid = (unsigned)(total / 256): the
                                                                                            runtime refuses grids beyond 2^32 threads
    key_bias_kernel, interaction_bias_kernel: int i < n * T; li_normalize: int r < n_pairs * rows_per_batch
                                                                                            int: wrapped beyond 2^31 elements / rows;
                                                                                            the launchers now refuse that (guard below)
  head.hip: (size_t) qi * K + i, (size_t) base + i                                          64
  rr_api.hip
    layout(): every size (size_t) n * S|T * width                                           64
    run_layer: int rows = batch * Tseq, rows = (int) r (packed); rr_forward: int R, RT      int: wrapped beyond 2^31 rows; packed calls
                                                                                            were refused beyond 2^30 rows, padded calls
                                                                                            and rr_reserve now are too (check_rows)

Nothing wraps at a size a card can hold; the int row counts want a guard, not a test (2^30 rows of 768 are 1.6 TB of 16-bit
rows alone): test_calls_beyond_2_30_rows_are_refused_before_any_launch sees RR_ERR_BAD_SHAPE and no launch.

Pattern (tests/test_gpu_ops.py::test_gemm_operand_beyond_4_gib, generalised): the big buffer is filled on the device in row chunks,
every chunk from a generator seeded by (case, chunk) so that no two row blocks hold the same data; every output is pre-filled
with NaN; the op runs ONCE; then row blocks of BLK rows — the first, one in the middle, the one that ends at the 2^32-byte
boundary of the buffer under test, the one that starts on it (its first row straddles the boundary when the row size does not
divide 2^32) and the last, partial tile — are compared with a float64 / float32 torch reference of those rows alone, under the
tolerance of the small-shape test of the same op (named at each use), and must be finite everywhere.  Where an existing test
proves that a row's bits do not depend on its place (test_gemm_rows_do_not_depend_on_where_their_tile_lies, its int8 twin, the
row kernels: one wave per row), the block behind the boundary must ALSO be bit-equal to the same op on a copy of just those rows
with the kernel pinned.

Why a truncated index fails these checks (one argument per family; nothing here runs a broken kernel):

* GEMM operand / residual / row-kernel INPUT (read at base + r * row_bytes): with the offset reduced mod 2^32 row r >= edge
  (edge = 2^32 // row_bytes) would be read from byte (r - edge) * row_bytes + (edge * row_bytes - 2^32), i.e. from rows
  r - edge - 1 .. r - edge of the first block.  The block at `edge` would then be computed from the data of rows 0 .. BLK, which
  come from another seed: independent N(0, 1) operands give an error of the order of the result itself (|ref| ~ 1, tolerance
  1.2e-2 (1 + |ref|) at most), and the bit-equality with the run on the copied rows fails outright.
* GEMM / row-kernel OUTPUT (written at base + r * row_bytes): the rows behind the boundary would land on rows 0 .. of the output;
  the block at `edge` keeps its NaN pre-fill (the finiteness assertion fails) and block 0 holds the results of other rows (its
  tolerance check fails), whichever is written last.
* 8-bit GEMMs: the same two arguments with row_bytes = K (operands), 2 N / N / 4 N (16-bit, e4m3, fp32 outputs); the per-row
  scales are indexed by the row alone (4 M bytes: they cross only beyond 2^30 rows, out of scope).
* Attention: sequence b starts at (size_t) b * Tk * kv_stride elements; truncated to 32 bits, the sequences from the one that
  straddles element 2^31 on would read K / V (and write O at b * Tq * out_stride) of sequences b - 1 820.., whose keys are
  other random data: the float64 softmax reference of the inspected sequences differs by O(1).  The dense bias likewise at
  (size_t) b * Tq * dense_ld floats.  A segment's seg_row0 * stride is 64-bit on the host and in the kernel (long long).
* Forward: 2 400 (2 200) pairs are 24 (11) COPIES of one golden list; a wrapped row origin in any of the ~300 launches of the
  stack makes the copies behind the wrap read or overwrite rows of the first copies, and then their logits are not bit-equal
  to copy 0's (nor copy 0's to the 100-pair call's): the copies hold the same data, but a wrap shifts by edge * row_bytes - 2^32
  bytes, which is not a whole number of pairs for any buffer of layout() (2^32 is not a multiple of 512 * 768 * k bytes ... for
  S = 512, H = 768: 2^32 / (512 * 768 * 2) = 5461.33), so a wrapped read lands inside ANOTHER ROW POSITION of a pair.

Cases left out, and why: rr_op_key_bias / rr_op_joint_masks / rr_op_interaction_bias / the head
(4 or 8 bytes per token or pair: 2^29 tokens to cross = 2^20 pairs of 512, beyond the workspace of any card; the launchers
refuse n * T > INT_MAX); rr_op_vit_* (the ViT runs per query image: 50 to 257 rows each, 2^32 bytes at 10 000+ images per call).

Memory and time: every test states what it allocates and skips below that much free memory (never on an idle card: the largest
case, the 2 400-pair forward, holds a 40 GB workspace); seconds and peak bytes of each test (torch's allocations; a forward's
workspace is the library's own and is recorded beside it) go to the margins file (helpers.record_margin, keys large_index/*)."""
import ctypes as C
import math
import time

import numpy as np
import pytest
import torch

import test_gpu_attention_forms as AF
import test_gpu_ops as OPS
import test_gpu_row_kernels as RK
from helpers import O, arch_from_cfg, load_fullsize, record_margin
from int8_emulation import quant_rows_i8

pytestmark = pytest.mark.gpu

GIB4 = 1 << 32
BLK = 300
T16 = {0: torch.bfloat16, 1: torch.float16}
RR_ERR_BAD_SHAPE = -2


@pytest.fixture(scope="module")
def lib():
    import rmr_amd  # noqa: F401
    from rmr_amd import _lib
    return _lib.load()


@pytest.fixture(autouse=True)
def _cost(request):
    """Seconds and peak device bytes of every test of this module -> the margins file (profiles/large_index_tests.json)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    record_margin(f"large_index/{request.node.name}", seconds=round(time.time() - t0, 3), peak_bytes=int(torch.cuda.max_memory_allocated()))
    torch.cuda.empty_cache()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return t.data_ptr() if t is not None else 0


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _need(nbytes):
    """Skip (with the figure) when the card has less free memory than the test allocates plus 2 GiB of slack."""
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes + (2 << 30):
        pytest.skip(f"needs {nbytes / 2 ** 30:.1f} GiB of device memory, {free / 2 ** 30:.1f} GiB free")


def _chunks(M, cols, elems=1 << 27):
    """(chunk index, first row, rows) of row chunks of about `elems` elements: the fp32 temporary of a fill stays at 512 MiB."""
    step = max(1, elems // cols)
    return [(i, r0, min(step, M - r0)) for i, r0 in enumerate(range(0, M, step))]


def _randn_chunk(case, i, shape):
    g = torch.Generator(device="cuda").manual_seed(case * 1_000_003 + i)      # one seed per (case, chunk): no two blocks alike
    return torch.randn(shape, device="cuda", generator=g)


def _fill(t, case, scale=1.0, shift=0.0):
    """t [M, ...] <- N(shift, scale) in t's type, chunk by chunk."""
    cols = t[0].numel()
    for i, r0, n in _chunks(t.shape[0], cols):
        x = _randn_chunk(case, i, (n,) + tuple(t.shape[1:]))
        if scale != 1.0:
            x *= scale
        if shift != 0.0:
            x += shift
        t[r0:r0 + n] = x.to(t.dtype)
    return t


def _blocks(M, row_bytes):
    """First rows of the inspected blocks: start, middle, up to the 2^32-byte boundary, from it on, the last (partial) tile."""
    edge = GIB4 // row_bytes
    assert M * row_bytes > GIB4 and edge + BLK <= M - BLK and M % 256 != 0, (M, row_bytes)
    return edge, [0, edge // 2, edge - BLK, edge, M - BLK]


def _variant(lib, v):
    assert lib.rr_set_gemm_variant(v) == 0


def _small_variant(v):
    """The kernel the heuristic picks for the big problem, pinned for the run on the copied rows: -1 -> 14 (persistent ring)."""
    return 14 if v < 0 else v


def _gelu(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def _weights(case, N, K, t16, scale=0.05):
    g = torch.Generator(device="cuda").manual_seed(case)
    W = (torch.randn(N, K, device="cuda", generator=g) * scale).to(t16)
    b = torch.randn(N, device="cuda", generator=g)
    return W, b, g


def _close(got, ref, tol, what):
    got = got.double()
    assert torch.isfinite(got).all(), f"{what}: a value was left unwritten (NaN pre-fill) or is not finite"
    err = (got - ref).abs()
    bad = err > tol * (1 + ref.abs())
    assert not bad.any(), f"{what}: {int(bad.sum())} beyond tolerance, max err {err.max().item():.3e}"


# ================================================================================================ 1. 16-bit GEMM outputs
@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("variant", [-1, 0])     # -1: the production heuristic (persistent ring), 0: the 128 x 128 kernel
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_gemm_output_beyond_4_gib(lib, epi, variant, dt):
    """rr_op_gemm_bf16 writing 4.3 GB: 16-bit [700 003, 3072] (epilogues 0, 1) and fp32 [1 400 003, 768] (epilogue 2), K = 64.
    Tolerances of test_gemm_epilogues (1.2e-2 / 2e-4 times 1 + |ref|); the block behind the boundary bit-equal to the pinned
    kernel on a copy of its rows (test_gemm_rows_do_not_depend_on_where_their_tile_lies)."""
    M, N, K, es = (1_400_003, 768, 64, 4) if epi == 2 else (700_003, 3072, 64, 2)
    _need(M * N * es + M * K * 2 + (1 << 30))
    t16 = T16[dt]
    assert lib.rr_set_op_dtype(dt) == 0
    try:
        A = _fill(torch.empty(M, K, dtype=t16, device="cuda"), 100 + epi)
        W, b, _ = _weights(11 + epi, N, K, t16)
        out = torch.full((M, N), float("nan"), device="cuda", dtype=torch.float32 if epi == 2 else t16)
        _variant(lib, variant)
        assert lib.rr_op_gemm_bf16(_p(A), _p(W), _p(b), M, N, K, epi, _p(out), _stream()) == 0
        torch.cuda.synchronize()
        edge, blocks = _blocks(M, N * es)
        for r0 in blocks:
            ref = A[r0:r0 + BLK].double() @ W.double().t() + b.double()
            _close(out[r0:r0 + BLK], _gelu(ref) if epi == 1 else ref, 2e-4 if epi == 2 else 1.2e-2, f"rows {r0}")
        sub = A[edge:edge + BLK].contiguous()
        small = torch.full((BLK, N), float("nan"), device="cuda", dtype=out.dtype)
        _variant(lib, _small_variant(variant))
        assert lib.rr_op_gemm_bf16(_p(sub), _p(W), _p(b), BLK, N, K, epi, _p(small), _stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(out[edge:edge + BLK]), _bits(small)), "rows behind the boundary differ from the run on their copy"
    finally:
        lib.rr_set_gemm_variant(-1)
        lib.rr_set_op_dtype(0)


# ================================================================================================ 2. fp32 residual epilogues
@pytest.mark.parametrize("variant", [-1, 0])
@pytest.mark.parametrize("kind", ["resid", "ln_resid"])
def test_residual_gemm_rows_beyond_4_gib(lib, kind, variant):
    """rr_op_gemm_resid_f32 (resid and out fp32 [1 400 003, 768], 4.3 GB each) and rr_op_gemm_ln_resid_f32 (x likewise, the
    residual recomputed from stats [M, 2] that rr_op_layernorm_stats wrote over the same rows).  fp32 rule of
    test_ring_kernels_ragged_multi_tile: 2e-4 (1 + |ref|); statistics as test_ln_residual_gemm_is_reproducible...: 1e-5."""
    M, N, K, eps = 1_400_003, 768, 64, 1e-12
    _need(2 * M * N * 4 + M * N * 2 + (1 << 30))
    A = _fill(torch.empty(M, K, dtype=torch.bfloat16, device="cuda"), 200)
    W, b, g = _weights(21, N, K, torch.bfloat16)
    X = _fill(torch.empty(M, N, device="cuda"), 201, 1.5, 0.3)
    gam = 1 + 0.1 * torch.randn(N, device="cuda", generator=g)
    bet = 0.05 * torch.randn(N, device="cuda", generator=g)
    out = torch.full((M, N), float("nan"), device="cuda")
    stats = torch.full((M, 2), float("nan"), device="cuda")
    edge, blocks = _blocks(M, N * 4)

    def run(a, x, st, o, m):
        if kind == "resid":
            return lib.rr_op_gemm_resid_f32(_p(a), _p(W), _p(b), _p(x), m, N, K, _p(o), _stream())
        return lib.rr_op_gemm_ln_resid_f32(_p(a), _p(W), _p(b), _p(x), _p(st), _p(gam), _p(bet), m, N, K, _p(o), _stream())

    try:
        if kind == "ln_resid":
            ln16 = torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16)
            assert lib.rr_op_layernorm_stats(_p(X), _p(gam), _p(bet), eps, M, N, 0, _p(ln16), _p(stats), _stream()) == 0
        _variant(lib, variant)
        assert run(A, X, stats, out, M) == 0
        torch.cuda.synchronize()
        for r0 in blocks:
            x = X[r0:r0 + BLK].double()
            res = x
            if kind == "ln_resid":
                mean, rstd = x.mean(1, keepdim=True), torch.rsqrt(x.var(1, unbiased=False, keepdim=True) + eps)
                st = stats[r0:r0 + BLK].double()
                assert torch.allclose(st, torch.cat([mean, rstd], 1), atol=1e-5, rtol=1e-5), f"stats of rows {r0}"
                res = (x - mean) * rstd * gam.double() + bet.double()
                _close(ln16[r0:r0 + BLK], res, 1.2e-2, f"16-bit LayerNorm rows {r0}")
            _close(out[r0:r0 + BLK], A[r0:r0 + BLK].double() @ W.double().t() + b.double() + res, 2e-4, f"rows {r0}")
        small = torch.full((BLK, N), float("nan"), device="cuda")
        _variant(lib, _small_variant(variant))
        assert run(A[edge:edge + BLK].contiguous(), X[edge:edge + BLK].contiguous(), stats[edge:edge + BLK].contiguous(), small, BLK) == 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(out[edge:edge + BLK]), _bits(small))
    finally:
        lib.rr_set_gemm_variant(-1)


# ================================================================================================ 3. folded LayerNorm chain
@pytest.mark.parametrize("dt", [0, 1])
def test_folded_producer_outputs_beyond_4_gib(lib, dt):
    """rr_op_gemm_resid_lnprep over [1 400 003, 768]: resid and out_f32 cross the boundary (fp32), x16_out and the partials
    [M, 6, 2] lie below it at this M and are checked on the same blocks; rr_op_ln_finalize stand-alone over the partials must
    reproduce stats_out bit for bit.  Rules of test_folded_layernorm_halves."""
    M, N, K, eps = 1_400_003, 768, 64, 1e-12
    _need(2 * M * N * 4 + M * N * 2 + (1 << 30))
    t16 = T16[dt]
    assert lib.rr_set_op_dtype(dt) == 0
    try:
        A = _fill(torch.empty(M, K, dtype=t16, device="cuda"), 300)
        W, b, _ = _weights(31, N, K, t16, 0.03)
        R = _fill(torch.empty(M, N, device="cuda"), 301, 2.0, 0.7)
        nparts = (N + 127) // 128

        def run(a, r, m):
            out = torch.full((m, N), float("nan"), device="cuda")
            x16 = torch.full((m, N), float("nan"), device="cuda", dtype=t16)
            stats, part = torch.full((m, 2), float("nan"), device="cuda"), torch.full((m, nparts, 2), float("nan"), device="cuda")
            assert lib.rr_op_gemm_resid_lnprep(_p(a), _p(W), _p(b), _p(r), m, N, K, eps, _p(out), _p(x16), _p(stats), _p(part), _stream()) == 0
            torch.cuda.synchronize()
            return out, x16, stats, part

        out, x16, stats, part = run(A, R, M)
        stats2 = torch.full((M, 2), float("nan"), device="cuda")
        assert lib.rr_op_ln_finalize(_p(part), nparts, N, eps, M, _p(stats2), 0, float("inf"), _stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(stats2), _bits(stats))
        edge, blocks = _blocks(M, N * 4)
        for r0 in blocks:
            rows = slice(r0, r0 + BLK)
            ref = A[rows].float() @ W.float().t() + b + R[rows]
            assert torch.isfinite(out[rows]).all() and torch.allclose(out[rows], ref, atol=5e-4, rtol=1e-4), f"rows {r0}"
            assert torch.equal(_bits(x16[rows]), _bits(out[rows].to(t16))), f"x16 rows {r0}"
            o = out[rows].double()
            assert torch.allclose(stats[rows, 0].double(), o.mean(1), atol=2e-6, rtol=1e-6)
            assert torch.allclose(stats[rows, 1].double(), 1 / torch.sqrt(o.var(1, unbiased=False) + eps), rtol=2e-6)
        _variant(lib, 14)
        s_out, s_x16, s_stats, _ = run(A[edge:edge + BLK].contiguous(), R[edge:edge + BLK].contiguous(), BLK)
        assert torch.equal(_bits(out[edge:edge + BLK]), _bits(s_out)) and torch.equal(_bits(x16[edge:edge + BLK]), _bits(s_x16))
        assert torch.equal(_bits(stats[edge:edge + BLK]), _bits(s_stats))
    finally:
        lib.rr_set_gemm_variant(-1)
        lib.rr_set_op_dtype(0)


@pytest.mark.parametrize("variant", [-1, 0])
@pytest.mark.parametrize("shape", ["operand", "output"])
def test_folded_consumer_beyond_4_gib(lib, shape, variant):
    """rr_op_gemm_lnfold: "operand" = A_raw [2 100 003, 1024] (4.3 GB) into N = 128 fp32 columns; "output" = 16-bit
    [530 003, 4096] (4.3 GB) from K = 64, epilogues 0 and 1.  Expectation and tolerances of test_folded_layernorm_halves
    (exact arithmetic on the same operands: rstd (x16 Wf^T - mean csum) + d; 3e-4 fp32, 1.2e-2 16-bit, times 1 + |want|)."""
    M, N, K, epis = (2_100_003, 128, 1024, (2,)) if shape == "operand" else (530_003, 4096, 64, (0, 1))
    _need(M * K * 2 + M * N * (4 if shape == "operand" else 2) + (1 << 30))
    t16 = torch.bfloat16
    A = _fill(torch.empty(M, K, dtype=t16, device="cuda"), 310 + K)
    Wf, dvec, g = _weights(32 + K, N, K, t16, 0.03)
    csum = Wf.double().sum(1).float()
    stats = torch.stack([0.2 * torch.randn(M, device="cuda", generator=g), 0.5 + torch.rand(M, device="cuda", generator=g)], 1).contiguous()
    try:
        for epi in epis:
            out = torch.full((M, N), float("nan"), device="cuda", dtype=torch.float32 if epi == 2 else t16)
            _variant(lib, variant)
            assert lib.rr_op_gemm_lnfold(_p(A), _p(Wf), _p(dvec), _p(csum), _p(stats), M, N, K, epi, _p(out), _stream()) == 0
            torch.cuda.synchronize()
            edge, blocks = _blocks(M, K * 2 if shape == "operand" else N * 2)
            for r0 in blocks:
                rows = slice(r0, r0 + BLK)
                st = stats[rows].double()
                want = st[:, 1:2] * (A[rows].double() @ Wf.double().t() - st[:, 0:1] * csum.double()[None]) + dvec.double()
                _close(out[rows], _gelu(want) if epi == 1 else want, 3e-4 if epi == 2 else 1.2e-2, f"epi {epi} rows {r0}")
            small = torch.full((BLK, N), float("nan"), device="cuda", dtype=out.dtype)
            _variant(lib, _small_variant(variant))
            assert lib.rr_op_gemm_lnfold(_p(A[edge:edge + BLK].contiguous()), _p(Wf), _p(dvec), _p(csum), _p(stats[edge:edge + BLK].contiguous()),
                                         BLK, N, K, epi, _p(small), _stream()) == 0
            torch.cuda.synchronize()
            assert torch.equal(_bits(out[edge:edge + BLK]), _bits(small)), f"epi {epi}"
            del out
    finally:
        lib.rr_set_gemm_variant(-1)


# ================================================================================================ 4. split residual stream
@pytest.mark.parametrize("with_ln", [False, True])
def test_split_stream_rows_beyond_4_gib(lib, with_ln):
    """rr_op_gemm_resid_split in place over hi (bf16) and lo (fp16) [2 800 003, 768], 4.3 GB each.  The expectation is built as
    test_production_split_epilogue_is_bit_exact builds it, per row block: rr_op_split_residual_value on a copy of the block's
    (hi, lo, stats) taken BEFORE the in-place run, rr_op_gemm_resid_lnprep (persistent ring pinned) on those fp32 rows, and the
    exact roundings hi = 16 bits of it, lo = fp16(x - hi): bit for bit; statistics to 1e-6 as there."""
    M, N, K, eps = 2_800_003, 768, 64, 1e-12
    _need(2 * M * N * 2 + (2 << 30))
    t16 = torch.bfloat16
    assert lib.rr_set_op_dtype(0) == 0 and lib.rr_set_tuning(b"resid_lo8", 0) == 0
    try:
        A = _fill(torch.empty(M, K, dtype=t16, device="cuda"), 400)
        W, b, g = _weights(41, N, K, t16)
        gam = 1 + 0.1 * torch.randn(N, device="cuda", generator=g)
        bet = 0.05 * torch.randn(N, device="cuda", generator=g)
        hi, lo = torch.empty(M, N, dtype=t16, device="cuda"), torch.empty(M, N, dtype=torch.float16, device="cuda")
        st_in = torch.empty(M, 2, device="cuda")
        for i, r0, n in _chunks(M, N):
            x = _randn_chunk(401, i, (n, N)) * 3 + 0.5
            h = x.to(t16)
            l = (x - h.float()).half()
            xs = h.double() + l.double()
            hi[r0:r0 + n], lo[r0:r0 + n] = h, l
            st_in[r0:r0 + n] = torch.stack([xs.mean(1), 1 / torch.sqrt(xs.var(1, unbiased=False) + eps)], 1).float()
            del x, h, l, xs
        edge, blocks = _blocks(M, N * 2)
        before = {r0: (hi[r0:r0 + BLK].clone(), lo[r0:r0 + BLK].clone(), st_in[r0:r0 + BLK].clone()) for r0 in blocks}
        nparts = (N + 127) // 128
        stats, part = torch.full((M, 2), float("nan"), device="cuda"), torch.empty(M, nparts, 2, device="cuda")
        assert lib.rr_op_gemm_resid_split(_p(A), _p(W), _p(b), _p(hi), _p(lo), _p(st_in) if with_ln else 0, _p(gam) if with_ln else 0,
                                          _p(bet) if with_ln else 0, M, N, K, eps, _p(hi), _p(lo), _p(stats), _p(part), _stream()) == 0
        torch.cuda.synchronize()
        _variant(lib, 14)
        for r0 in blocks:
            h0, l0, s0 = before[r0]
            R, out32 = torch.empty(BLK, N, device="cuda"), torch.full((BLK, N), float("nan"), device="cuda")
            assert lib.rr_op_split_residual_value(_p(h0), _p(l0), _p(s0) if with_ln else 0, _p(gam) if with_ln else 0,
                                                  _p(bet) if with_ln else 0, BLK, N, _p(R), _stream()) == 0
            x16_f, st_ref, pt = torch.empty(BLK, N, device="cuda", dtype=t16), torch.empty(BLK, 2, device="cuda"), torch.empty(BLK, nparts, 2, device="cuda")
            assert lib.rr_op_gemm_resid_lnprep(_p(A[r0:r0 + BLK].contiguous()), _p(W), _p(b), _p(R), BLK, N, K, eps, _p(out32), _p(x16_f),
                                               _p(st_ref), _p(pt), _stream()) == 0
            torch.cuda.synchronize()
            want_hi = out32.to(t16)
            want_lo = (out32 - want_hi.float()).half()
            assert torch.isfinite(out32).all()
            assert torch.equal(_bits(hi[r0:r0 + BLK]), _bits(want_hi)), f"hi rows {r0}"
            assert torch.equal(_bits(lo[r0:r0 + BLK]), _bits(want_lo)), f"lo rows {r0}"
            assert torch.allclose(stats[r0:r0 + BLK], st_ref, rtol=1e-6, atol=1e-6), f"stats rows {r0}"
    finally:
        lib.rr_set_gemm_variant(-1)
        lib.rr_set_tuning(b"resid_lo8", -1)


def test_split_stream_e5m2_lo_beyond_4_gib(lib):
    """The 8-bit lo half ("resid_lo8", the fp16 handles' default): e5m2 bytes in the paired-row layout of rr_common.h
    lo8_pair_offset, ceil(M / 32) * 32 rows of N bytes — 5 600 003 rows of 768 to pass 2^32 bytes (the fp16 hi rows, 8.6 GB, pass
    it twice).  In place, with the LayerNorm recompute, expectation per 32-row-aligned block as
    test_production_split_epilogue_is_bit_exact builds it for lo8 = 1: hi and the stored bytes bit for bit."""
    M, N, K, eps, G = 5_600_003, 768, 64, 1e-12, 320
    R = (M + 31) // 32 * 32
    _need(M * N * 2 + R * N + (3 << 30))
    assert R * N > GIB4
    t16 = torch.float16
    assert lib.rr_set_op_dtype(1) == 0 and lib.rr_set_tuning(b"resid_lo8", 1) == 0
    try:
        A = _fill(torch.empty(M, K, dtype=t16, device="cuda"), 450)
        W, b, g = _weights(45, N, K, t16)
        gam = 1 + 0.1 * torch.randn(N, device="cuda", generator=g)
        bet = 0.05 * torch.randn(N, device="cuda", generator=g)
        hi, lo8 = torch.empty(M, N, dtype=t16, device="cuda"), torch.zeros(R * N, dtype=torch.uint8, device="cuda")
        st_in = torch.empty(M, 2, device="cuda")
        step = (1 << 26) // N // 32 * 32
        for i, r0 in enumerate(range(0, M, step)):
            n = min(step, M - r0)
            x = _randn_chunk(451, i, (n, N)) * 3 + 0.5
            h = x.to(t16)
            l8 = OPS._lo8_encode(x - h.float())
            xs = h.double() + OPS._lo8_decode(l8).double()
            hi[r0:r0 + n] = h
            st_in[r0:r0 + n] = torch.stack([xs.mean(1), 1 / torch.sqrt(xs.var(1, unbiased=False) + eps)], 1).float()
            packed = OPS._lo8_to_device_layout(l8)
            lo8[r0 * N:r0 * N + packed.numel()] = packed
            del x, h, l8, xs, packed
        edge = GIB4 // N // 32 * 32                                 # the 32-row group whose bytes straddle 2^32
        blocks = [0, edge // 2 // 32 * 32, edge - G, edge, edge + G, M // 32 * 32 - G + 32]

        def lo_rows(r0):                                            # the e5m2 rows of a block, out of the device layout
            nb = min(G, M - r0)
            return OPS._lo8_from_device_layout(lo8[r0 * N:(r0 + (nb + 31) // 32 * 32) * N], nb, N)

        before = {r0: (hi[r0:r0 + G].clone(), OPS._lo8_decode(lo_rows(r0)).half(), st_in[r0:r0 + G].clone()) for r0 in blocks}
        nparts = (N + 127) // 128
        stats, part = torch.full((M, 2), float("nan"), device="cuda"), torch.empty(M, nparts, 2, device="cuda")
        assert lib.rr_op_gemm_resid_split(_p(A), _p(W), _p(b), _p(hi), _p(lo8), _p(st_in), _p(gam), _p(bet), M, N, K, eps, _p(hi), _p(lo8),
                                          _p(stats), _p(part), _stream()) == 0
        torch.cuda.synchronize()
        _variant(lib, 14)
        for r0 in blocks:
            h0, l0, s0 = before[r0]
            nb = h0.shape[0]
            Rv, out32 = torch.empty(nb, N, device="cuda"), torch.full((nb, N), float("nan"), device="cuda")
            assert lib.rr_op_split_residual_value(_p(h0), _p(l0), _p(s0), _p(gam), _p(bet), nb, N, _p(Rv), _stream()) == 0
            x16_f, st_ref, pt = torch.empty(nb, N, device="cuda", dtype=t16), torch.empty(nb, 2, device="cuda"), torch.empty(nb, nparts, 2, device="cuda")
            assert lib.rr_op_gemm_resid_lnprep(_p(A[r0:r0 + nb].contiguous()), _p(W), _p(b), _p(Rv), nb, N, K, eps, _p(out32), _p(x16_f),
                                               _p(st_ref), _p(pt), _stream()) == 0
            torch.cuda.synchronize()
            want_hi = out32.to(t16)
            want_lo = OPS._lo8_encode(out32 - want_hi.float()).view(torch.uint8)
            assert torch.isfinite(out32).all()
            assert torch.equal(_bits(hi[r0:r0 + nb]), _bits(want_hi)), f"hi rows {r0}"
            assert torch.equal(lo_rows(r0).view(torch.uint8), want_lo), f"lo rows {r0}"
            assert torch.allclose(stats[r0:r0 + nb], st_ref, rtol=1e-6, atol=1e-6), f"stats rows {r0}"
    finally:
        lib.rr_set_gemm_variant(-1)
        lib.rr_set_tuning(b"resid_lo8", -1)
        lib.rr_set_op_dtype(0)


# ================================================================================================ 5. 8-bit GEMMs and quantising LayerNorms
def _rowscaled(case, i, n, K):
    g = torch.Generator(device="cuda").manual_seed(case * 1_000_003 + i)
    return torch.randn(n, K, device="cuda", generator=g) * (0.2 + 3.0 * torch.rand(n, 1, device="cuda", generator=g))


def _operands8(case, M, N, K, fmt):
    """Per-row quantised A [M, K] (chunked) and per-channel W [N, K], as _e4m3_operands / _i8_operands of the small tests."""
    t8 = torch.float8_e4m3fn if fmt == "fp8" else torch.int8
    a8, sa = torch.empty(M, K, dtype=t8, device="cuda"), torch.empty(M, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(case)
    w = torch.randn(N, K, device="cuda", generator=g) * (0.01 + 0.08 * torch.rand(N, 1, device="cuda", generator=g))
    bias = torch.randn(N, device="cuda", generator=g) * 0.1

    def quant(x):
        if fmt == "fp8":
            s = x.abs().amax(1) / 448.0
            return (x / s[:, None]).to(t8), s
        q, s = quant_rows_i8(x)
        return q.to(t8), s.reshape(-1)

    for i, r0, n in _chunks(M, K):
        a8[r0:r0 + n], sa[r0:r0 + n] = quant(_rowscaled(case, i, n, K))
    w8, sw = quant(w)
    return a8, sa, w8.contiguous(), sw.contiguous(), bias, g


@pytest.mark.parametrize("fmt", ["fp8", "i8"])
def test_eight_bit_gemm_operand_and_output_beyond_4_gib(lib, fmt):
    """rr_op_gemm_fp8_rc / rr_op_gemm_i8_rc: A8 [1 100 003, 4096] (4.5 GB) and the 16-bit output [M, 2048] (4.5 GB) both cross.
    Rules: test_gemm_fp8_row_and_channel_scales (1e-4 of the magnitude sum + 2^-8 |ref|); test_gemm_i8_matches_the_exact_product
    (exact product, 2^-7 |ref|), and — int8 only, test_gemm_i8_rows_do_not_depend_on_where_their_tile_lies — the blocks behind
    both boundaries bit-equal to the run on their copy."""
    M, N, K = 1_100_003, 2048, 4096
    _need(M * K + M * N * 2 + (2 << 30))
    a8, sa, w8, sw, bias, _ = _operands8(500, M, N, K, fmt)
    op = lib.rr_op_gemm_fp8_rc if fmt == "fp8" else lib.rr_op_gemm_i8_rc
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device="cuda")
    assert op(_p(a8), _p(w8), _p(bias), _p(sa), _p(sw), M, N, K, 0, _p(out), _stream()) == 0
    torch.cuda.synchronize()
    e_in, b_in = _blocks(M, K)
    e_out, b_out = _blocks(M, N * 2)
    for r0 in sorted(set(b_in + b_out)):
        rows = slice(r0, r0 + BLK)
        got = out[rows].double()
        assert torch.isfinite(got).all(), f"rows {r0}"
        if fmt == "fp8":
            af, wf = a8[rows].float(), w8.float()
            ref = (af @ wf.T) * sa[rows, None] * sw[None, :] + bias
            mag = (af.abs() @ wf.abs().T) * sa[rows, None] * sw[None, :] + bias.abs()
            bad = (got - ref).abs() > 1e-4 * mag + 2.0 ** -8 * ref.abs() + 1e-6
        else:
            acc = (a8[rows].double() @ w8.double().t()).float().double()
            ref = acc * (sa[rows, None] * sw[None, :]).double() + bias.double()
            bad = (got - ref).abs() > 2.0 ** -7 * ref.abs() + 1e-30
        assert not bad.any(), f"rows {r0}: {int(bad.sum())} beyond tolerance, max |d| {(got - ref).abs().max().item():.3e}"
    if fmt == "i8":
        for e in sorted({e_in, e_out}):
            small = torch.full((BLK, N), float("nan"), dtype=torch.bfloat16, device="cuda")
            assert op(_p(a8[e:e + BLK].contiguous()), _p(w8), _p(bias), _p(sa[e:e + BLK].contiguous()), _p(sw), BLK, N, K, 0, _p(small), _stream()) == 0
            torch.cuda.synchronize()
            assert torch.equal(_bits(out[e:e + BLK]), _bits(small))


def test_fp8_gelu_e4m3_output_beyond_4_gib(lib):
    """rr_op_gemm_fp8_gelu_e4m3: out8 [1 100 003, 4096] e4m3 bytes (4.5 GB), K = 128.  Rule of test_gemm_fp8_gelu_to_e4m3_epilogue:
    torch's e4m3 rounding of the same fp32 value, byte for byte except rare one-step differences (< 2e-3 of the bytes)."""
    M, N, K, mul = 1_100_003, 4096, 128, 8.0
    _need(M * N + M * K + (2 << 30))
    a8, sa, w8, sw, bias, _ = _operands8(510, M, N, K, "fp8")
    out = torch.full((M, N), 0x7F, dtype=torch.uint8, device="cuda")                  # 0x7f: the e4m3 NaN
    assert lib.rr_op_gemm_fp8_gelu_e4m3(_p(a8), _p(w8), _p(bias), _p(sa), _p(sw), C.c_float(mul), M, N, K, _p(out), _stream()) == 0
    torch.cuda.synchronize()
    _, blocks = _blocks(M, N)
    for r0 in blocks:
        rows = slice(r0, r0 + BLK)
        pre = (a8[rows].float() @ w8.float().T) * sa[rows, None] * sw[None, :] + bias
        want = (torch.nn.functional.gelu(pre) * mul).clamp(-448, 448).to(torch.float8_e4m3fn)
        got = out[rows].view(torch.float8_e4m3fn)
        differ = got.view(torch.uint8) != want.view(torch.uint8)
        wf, gf = want.float(), got.float()
        assert torch.isfinite(gf).all(), f"rows {r0}"
        assert ((gf - wf).abs() <= torch.maximum(wf.abs(), gf.abs()) * 2.0 ** -3 + 2.0 ** -9)[differ].all(), f"rows {r0}"
        assert differ.float().mean().item() < 2e-3, f"rows {r0}"


@pytest.mark.parametrize("with_stats", [False, True])
def test_fp8_residual_rows_beyond_4_gib(lib, with_stats):
    """rr_op_gemm_fp8_resid: fp32 resid and out [1 400 003, 768] (4.3 GB each), with and without the (mean, rstd) recompute.
    Rule of test_gemm_fp8_residual_epilogue: 1e-4 of the magnitude sum."""
    M, N, K, scale = 1_400_003, 768, 128, 0.125
    _need(2 * M * N * 4 + (2 << 30))
    a8, _, w8, sw, bias, g = _operands8(520, M, N, K, "fp8")
    X = _fill(torch.empty(M, N, device="cuda"), 521, 2.0, 0.3)
    gamma = 1.0 + 0.1 * torch.randn(N, device="cuda", generator=g)
    beta = 0.05 * torch.randn(N, device="cuda", generator=g)
    stats = torch.empty(M, 2, device="cuda")
    for _, r0, n in _chunks(M, N):
        x = X[r0:r0 + n]
        stats[r0:r0 + n] = torch.stack([x.mean(1), torch.rsqrt(x.var(1, unbiased=False) + 1e-12)], 1)
    out = torch.full((M, N), float("nan"), device="cuda")
    assert lib.rr_op_gemm_fp8_resid(_p(a8), _p(w8), _p(bias), C.c_float(scale), _p(sw), _p(X), _p(stats) if with_stats else 0,
                                    _p(gamma) if with_stats else 0, _p(beta) if with_stats else 0, M, N, K, _p(out), _stream()) == 0
    torch.cuda.synchronize()
    _, blocks = _blocks(M, N * 4)
    for r0 in blocks:
        rows = slice(r0, r0 + BLK)
        af, wf = a8[rows].float(), w8.float()
        res = ((X[rows] - stats[rows, 0:1]) * stats[rows, 1:2] * gamma + beta) if with_stats else X[rows]
        ref = (af @ wf.T) * scale * sw[None, :] + bias + res
        mag = (af.abs() @ wf.abs().T) * scale * sw[None, :] + bias.abs() + res.abs()
        assert torch.isfinite(out[rows]).all(), f"rows {r0}"
        bad = (out[rows] - ref).abs() > 1e-4 * mag + 1e-6
        assert not bad.any(), f"rows {r0}: {int(bad.sum())} beyond tolerance, max |d| {(out[rows] - ref).abs().max().item():.3e}"


@pytest.mark.parametrize("fmt", ["fp8", "i8"])
def test_quantising_layernorm_rows_beyond_4_gib(lib, fmt):
    """rr_op_layernorm_q8 / rr_op_layernorm_i8 over [4 200 003, 1024]: the fp32 input (17 GB) crosses 2^32 bytes four times, the
    codes (4.3 GB) once; row_scale and stats [M] / [M, 2] stay below.  Rules of test_layernorm_q8_matches_torch /
    test_layernorm_i8_matches_the_emulation on blocks around every crossing; one wave per row, so the block behind the codes'
    boundary is bit-equal to the run on its copy."""
    M, cols, eps = 4_200_003, 1024, 1e-12
    _need(M * cols * 5 + (2 << 30))
    X = _fill(torch.empty(M, cols, device="cuda"), 530, 1.3, 0.4)
    g = torch.Generator(device="cuda").manual_seed(53)
    gamma, beta = 1 + 0.2 * torch.randn(cols, device="cuda", generator=g), 0.1 * torch.randn(cols, device="cuda", generator=g)
    op = lib.rr_op_layernorm_q8 if fmt == "fp8" else lib.rr_op_layernorm_i8

    def run(x, m):
        out = torch.full((m, cols), 0x7F if fmt == "fp8" else -128, dtype=torch.uint8 if fmt == "fp8" else torch.int8, device="cuda")
        sc, st = torch.full((m,), float("nan"), device="cuda"), torch.full((m, 2), float("nan"), device="cuda")
        assert op(_p(x), _p(gamma), _p(beta), eps, m, cols, _p(out), _p(sc), _p(st), _stream()) == 0
        torch.cuda.synchronize()
        return out, sc, st

    out, sc, st = run(X, M)
    e_out, b_out = _blocks(M, cols)
    starts = set(b_out)
    for k in (1, 2, 3):
        e = k * GIB4 // (cols * 4)
        starts |= {e - BLK, e}
    for r0 in sorted(starts):
        rows = slice(r0, r0 + BLK)
        x = X[rows]
        y = torch.nn.functional.layer_norm(x, (cols,), gamma, beta, eps)
        assert torch.allclose(st[rows, 0], x.mean(1), atol=1e-5), f"rows {r0}"
        assert torch.allclose(st[rows, 1], 1 / torch.sqrt(x.var(1, unbiased=False) + eps), rtol=1e-4), f"rows {r0}"
        if fmt == "fp8":
            assert torch.allclose(sc[rows], y.abs().amax(1) / 448.0, rtol=3e-6, atol=0), f"rows {r0}"
            deq = out[rows].view(torch.float8_e4m3fn).float() * sc[rows, None]
            assert ((deq - y).abs() <= 0.0626 * y.abs() + sc[rows, None] * 2.0 ** -10 + 1e-7).all(), f"rows {r0}"
            want = (y / sc[rows, None]).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
            assert (out[rows] != want).float().mean().item() < 2e-3, f"rows {r0}"
        else:
            q, s = quant_rows_i8(y)
            assert torch.allclose(sc[rows], s.reshape(-1), rtol=3e-6, atol=0), f"rows {r0}"
            d = (out[rows].float() - q).abs()
            near_tie = (((y / s).abs() % 1.0) - 0.5).abs() < 2e-3
            assert d.max().item() <= 1 and not (d > 0)[~near_tie].any() and (d > 0).float().mean().item() < 2e-3, f"rows {r0}"
    s_out, s_sc, s_st = run(X[e_out:e_out + BLK].contiguous(), BLK)
    assert torch.equal(_bits(out[e_out:e_out + BLK]), _bits(s_out)) and torch.equal(_bits(sc[e_out:e_out + BLK]), _bits(s_sc))
    assert torch.equal(_bits(st[e_out:e_out + BLK]), _bits(s_st))


# ================================================================================================ 6. attention
def _tail_bias(case, B, T, lo):
    g = torch.Generator(device="cuda").manual_seed(case)
    lens = torch.randint(lo, T + 1, (B, 1), device="cuda", generator=g)
    return torch.where(torch.arange(T, device="cuda")[None] < lens, 0.0, -1e30).float().contiguous()


def _fused_qkv(case, B, T, H, t16):
    qkv = torch.empty(B * T, 3 * H, dtype=t16, device="cuda")
    for i, r0, n in _chunks(B * T, 3 * H):
        x = _randn_chunk(case, i, (n, 3 * H))
        x[:, :H] *= 0.25
        qkv[r0:r0 + n] = x.to(t16)
    return qkv


def _qkv_of(qkv, sel, T, H):
    v = qkv.view(-1, T, 3 * H)[sel]
    return v[..., :H].contiguous(), v[..., H:2 * H].contiguous(), v[..., 2 * H:].contiguous()


@pytest.mark.parametrize("dt", [0, 1])
def test_attention_on_a_fused_qkv_buffer_beyond_4_gib(lib, dt):
    """rr_op_attention_ex on the forward's layout: 1 850 sequences of Tq = Tk = 512, 12 heads, q / k / v at columns 0 / 768 /
    1536 of one [B * 512, 2304] buffer (4.36 GB; element 2^31 lies inside sequence 1 820), tail-padded key bias.  The schedules
    fixed_mode 1, 2 (fixed reference, 32 / 64 rows per wave) and 0 (online); sequences 0, 1 819 .. 1 821 and the last against the
    float64 softmax reference and the rounding emulation under the gates of tests/test_gpu_attention_forms.py; the three
    sequences around the boundary bit-equal to the same schedule (schedule_blocks = the big call's grid) on a copy of them.
    Then rr_op_attention_segs over the same buffer, three segments whose seg_row0 lie before, across and behind the boundary,
    against one rr_op_attention_ex per segment (bit for bit, test_segments_one_launch_equals_per_segment_launches) and the
    references; rows of no segment keep their NaN."""
    B, T, heads = 1850, 512, 12
    H = heads * 64
    _need(B * T * 3 * H * 2 + 2 * B * T * H * 2 + (2 << 30))
    stats = []
    with AF._op_dtype(lib, dt) as t16:
        qkv = _fused_qkv(600 + dt, B, T, H, t16)
        bias = _tail_bias(60, B, T, 64)
        sb = (GIB4 // 2) // (T * 3 * H)
        assert 0 < sb - 1 and sb + 1 < B - 1 and sb * T * 3 * H < GIB4 // 2 < (sb + 1) * T * 3 * H
        sel = torch.tensor([0, sb - 1, sb, sb + 1, B - 1], device="cuda")
        sched = ((B * heads + 7) // 8) * 8 * ((T + 127) // 128)
        for mode in (1, 2, 0):
            out = torch.full((B * T, H), float("nan"), dtype=t16, device="cuda")
            assert lib.rr_op_attention_ex(_p(qkv), _p(qkv) + H * 2, _p(qkv) + 2 * H * 2, 3 * H, 3 * H, _p(bias), B, heads, T, T, 1, 0,
                                          _p(out), H, 0, 0, 0, mode, _stream()) == 0
            torch.cuda.synchronize()
            q, k, v = _qkv_of(qkv, sel, T, H)
            stats.append(AF._check(f"large.fused_qkv.mode{mode}", out.view(B, T, H)[sel], q, k, v, bias[sel], heads))
            near = slice(sb - 1, sb + 2)
            q, k, v = _qkv_of(qkv, near, T, H)
            small = AF._attn(lib, q, k, v, bias[near].contiguous(), heads, sched=sched, mode=mode)
            assert torch.equal(_bits(out.view(B, T, H)[near]), _bits(small)), f"fixed_mode {mode}"
            del out
        # segments: (n sequences, rows each, first row) before, across and behind the boundary
        segs = [(3, 512, 0), (4, 300, (sb - 1) * T + 77), (2, 512, (B - 2) * T)]
        rowbias = _tail_bias(61, B, T, 64).view(-1)
        rowbias[segs[1][2]:segs[1][2] + 4 * 300] = _tail_bias(62, 4, 300, 40).view(-1)
        sn, sl = np.array([s[0] for s in segs], np.int32), np.array([s[1] for s in segs], np.int32)
        sr = np.array([s[2] for s in segs], np.int64)
        for mode in (2, 0):
            out = torch.full((B * T, H), float("nan"), dtype=t16, device="cuda")
            assert lib.rr_op_attention_segs(_p(qkv), 3 * H, _p(qkv) + H * 2, _p(qkv) + 2 * H * 2, 3 * H, _p(rowbias), heads, 3, sn.ctypes.data,
                                            sl.ctypes.data, sr.ctypes.data, _p(out), H, 1 << 20, mode, _stream()) == 0
            torch.cuda.synchronize()
            written = torch.zeros(B * T, dtype=torch.bool, device="cuda")
            for n, L, r0 in segs:
                rows = slice(r0, r0 + n * L)
                written[rows] = True
                x = qkv[rows].view(n, L, 3 * H)
                q, k, v = x[..., :H].contiguous(), x[..., H:2 * H].contiguous(), x[..., 2 * H:].contiguous()
                kb = rowbias[rows].view(n, L).contiguous()
                per = AF._attn(lib, q, k, v, kb, heads, sched=1 << 20, mode=mode)
                assert torch.equal(_bits(out[rows].view(n, L, H)), _bits(per)), f"segment at row {r0}, fixed_mode {mode}"
                stats.append(AF._check(f"large.segs.row{r0}.mode{mode}", out[rows].view(n, L, H), q, k, v, kb, heads))
            assert torch.isnan(out[~written].float()).all(), "a row of no segment was written"
            del out
    AF._gate(stats, "large_fused_qkv")


@pytest.mark.parametrize("dt", [0, 1])
def test_dense_bias_beyond_4_gib(lib, dt):
    """The dense (attention-fusion) bias [2 900][593][640] fp32 = 4.40 GB read by the online kernel (Tq = Tk = 593, 2 heads);
    the 47 slack columns hold 1e3, which must not leak.  Sequences 0, the one whose bias straddles the boundary, its neighbours
    and the last, against the references and gates of test_dense_bias_online_kernel."""
    B, T, ld, heads = 2900, 593, 640, 2
    H = heads * 64
    _need(B * T * ld * 4 + 4 * B * T * H * 2 + (2 << 30))
    with AF._op_dtype(lib, dt) as t16:
        dense = torch.empty(B, T, ld, device="cuda")
        for i, r0, n in _chunks(B, T * ld):
            x = _randn_chunk(610, i, (n, T, ld)) * 2.0
            x[:, :, T:] = 1e3
            dense[r0:r0 + n] = x
        q = _fill(torch.empty(B, T, H, dtype=t16, device="cuda"), 611, 0.25)
        k = _fill(torch.empty(B, T, H, dtype=t16, device="cuda"), 612)
        v = _fill(torch.empty(B, T, H, dtype=t16, device="cuda"), 613)
        bias = _tail_bias(63, B, T, 64)
        sb = GIB4 // (T * ld * 4)
        assert sb + 1 < B - 1
        sel = torch.tensor([0, sb - 1, sb, sb + 1, B - 1], device="cuda")
        out = AF._attn(lib, q, k, v, bias, heads, dense=dense)
        st = AF._check("large.dense", out[sel], q[sel], k[sel], v[sel], bias[sel], heads, dense=dense[sel][:, :, :T].contiguous())
    AF._gate([st], "large_dense")


def test_fusion_adj_output_beyond_4_gib(lib):
    """rr_op_fusion_adj writing 4.3 GB of adj: [39 000][145][192] fp32 from scores [39 000][64][81] (interaction form, row0 = 0):
    the pairs around the boundary, the first and the last against the oracle adjacency (FUSION_GATE per unit of the
    multiplier), padding columns exactly 0, nothing behind the last pair.  Tq = 81, Tc = 64 is a shape of
    test_fusion_bias_builders.  The geometry is not the cross-encoder's [593][640] because that gate (1e-6, measured on 6 pairs up
    to Tc = 200) is a statement about rounding that does not hold for longer columns or more data: the column softmax adds its Tc
    terms one after the other in fp32, and PAIR 0 — nothing to do with addressing — sat 1.9e-6 from float64 at Tc = 512 and
    1.3e-6 at Tc = 200 with this module's data.  The same number of bytes is written here with more, smaller pairs."""
    n, Tq, Tc, ld, mult = 39_000, 81, 64, 192, 20.0
    T = Tq + Tc
    _need(n * T * ld * 4 + n * Tc * Tq * 4 + (2 << 30))
    scores = _fill(torch.empty(n, Tc, Tq, device="cuda"), 620, 3.0)
    out = torch.full((n * T * ld + 64,), float("nan"), device="cuda")
    assert lib.rr_op_fusion_adj(_p(scores), Tc, Tq, Tc, C.c_float(mult), 0, n, _p(out), ld, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out[n * T * ld:]).all()
    adj = out[:n * T * ld].view(n, T, ld)
    sb = GIB4 // (T * ld * 4)
    for p in (0, sb - 1, sb, sb + 1, n - 1):
        a = adj[p].cpu()
        assert torch.isfinite(a).all() and (a[:, T:] == 0).all(), f"pair {p}"
        ref = AF._adj_ref(scores[p:p + 1].cpu(), "interaction", Tq, Tc, mult)[0]
        err = (a[:, :T].double() - ref).abs().max().item() / mult
        assert err <= AF.FUSION_GATE, (p, err)


# ================================================================================================ 7. row kernels
@pytest.mark.parametrize("dt", [0, 1])
def test_layernorm_rows_beyond_4_gib(lib, dt):
    """rr_op_layernorm and rr_op_layernorm_stats over fp32 [1 400 003, 768] in and out (4.3 GB each) plus the 16-bit rows.
    LN_UNITS of tests/test_gpu_row_kernels.py against float64; the 16-bit rows are the fp32 rows rounded; the two ops and the run
    on a copy of the block behind the boundary agree bit for bit (one wave per row)."""
    M, cols, eps = 1_400_003, 768, 1e-12
    _need(2 * M * cols * 4 + M * cols * 2 + (1 << 30))
    X = _fill(torch.empty(M, cols, device="cuda"), 700, 1.3, 0.4)
    _, gamma, beta = RK._params(cols, 70)
    gd, bd = gamma.cuda(), beta.cuda()
    edge, blocks = _blocks(M, cols * 4)
    with RK._op_dtype(lib, dt) as t16:
        def run(x, m, with_stats):
            o32, o16 = torch.full((m, cols), float("nan"), device="cuda"), RK._filled16((m, cols), t16)
            st = torch.full((m, 2), float("nan"), device="cuda")
            if with_stats:
                assert lib.rr_op_layernorm_stats(_p(x), _p(gd), _p(bd), eps, m, cols, _p(o32), _p(o16), _p(st), _stream()) == 0
            else:
                assert lib.rr_op_layernorm(_p(x), _p(gd), _p(bd), eps, m, cols, _p(o32), _p(o16), _stream()) == 0
            torch.cuda.synchronize()
            return o32, o16, st

        o32, o16, _ = run(X, M, False)
        for r0 in blocks:
            rows = slice(r0, r0 + BLK)
            ref, unit = RK._ln_ref(X[rows].cpu().double(), gamma.double(), beta.double(), eps)
            RK._check_ln(f"large.layernorm.dt{dt}.rows{r0}", o32[rows], o16[rows], ref, unit, t16)
        s32, s16, _ = run(X[edge:edge + BLK].contiguous(), BLK, False)
        assert torch.equal(_bits(o32[edge:edge + BLK]), _bits(s32)) and torch.equal(_bits(o16[edge:edge + BLK]), _bits(s16))
        keep = {r0: (o32[r0:r0 + BLK].clone(), o16[r0:r0 + BLK].clone()) for r0 in blocks}
        del o32, o16
        o32, o16, st = run(X, M, True)
        for r0 in blocks:
            rows = slice(r0, r0 + BLK)
            assert torch.equal(_bits(o32[rows]), _bits(keep[r0][0])) and torch.equal(_bits(o16[rows]), _bits(keep[r0][1]))
            x = X[rows].double()
            assert torch.allclose(st[rows].double(), torch.stack([x.mean(1), torch.rsqrt(x.var(1, unbiased=False) + eps)], 1), atol=1e-5, rtol=1e-5)


def test_embed_ln_rows_beyond_4_gib(lib):
    """rr_op_embed_ln: 2 735 sequences of 512 tokens, 768 columns: fp32 rows 4.3 GB, 16-bit rows 2.15 GB, ids / token types
    int64 [rows].  Distinct position and type rows (a wrong row index is O(1)); LN_UNITS against float64."""
    n, S, cols, vocab, tv, eps = 2735, 512, 768, 1000, 2, 1e-12
    rows_n = n * S
    _need(rows_n * cols * 6 + (1 << 30))
    g, gamma, beta = RK._params(cols, 71)
    word, pos, typ = torch.randn(vocab, cols, generator=g), 2 * torch.randn(S, cols, generator=g), 2 * torch.randn(tv, cols, generator=g)
    gd = torch.Generator(device="cuda").manual_seed(710)
    ids = torch.randint(0, vocab, (rows_n,), device="cuda", generator=gd)
    tts = torch.randint(0, tv, (rows_n,), device="cuda", generator=gd)
    with RK._op_dtype(lib, 0) as t16:
        o32, o16 = RK._embed(lib, ids, tts, word.cuda(), pos.cuda(), typ.cuda(), gamma.cuda(), beta.cuda(), eps, S, vocab, tv, t16)
    assert rows_n % 256 == 0            # (a row count of whole sequences: the partial last tile is the GEMMs' and LayerNorm's case)
    edge = GIB4 // (cols * 4)
    for r0 in (0, edge // 2, edge - BLK, edge, rows_n - BLK):
        r = torch.arange(r0, r0 + BLK)
        x64 = (word[ids[r0:r0 + BLK].cpu()] + typ[tts[r0:r0 + BLK].cpu()] + pos[r % S]).double()
        ref, unit = RK._ln_ref(x64, gamma.double(), beta.double(), eps)
        RK._check_ln(f"large.embed_ln.rows{r0}", o32[r0:r0 + BLK], o16[r0:r0 + BLK], ref, unit, t16)


def test_ce_embed_ln_rows_beyond_4_gib(lib):
    """rr_op_ce_embed_ln over 2 361 pairs of T = 593 rows x 768 (fp32 in and out 4.3 GB each), bucketed positions (text rows at t,
    vision rows from 520); cls32: fp32 written for the rows t == 0 alone, bit-equal to the full call, NaN elsewhere."""
    n, T, cols, s_text, vis0, eps = 2361, 593, 768, 512, 520, 1e-12
    rows_n = n * T
    _need(2 * rows_n * cols * 4 + rows_n * cols * 2 + (1 << 30))
    g, gamma, beta = RK._params(cols, 72)
    pt = torch.tensor(RK._ce_positions(T, s_text, vis0))
    pos, typ0 = 2 * torch.randn(int(pt.max()) + 1, cols, generator=g), torch.randn(cols, generator=g)
    X = _fill(torch.empty(rows_n, cols, device="cuda"), 720)
    dev = [t.cuda() for t in (pos, typ0, gamma, beta)]
    edge, blocks = _blocks(rows_n, cols * 4)
    with RK._op_dtype(lib, 1) as t16:
        res = {}
        for cls32 in (0, 1):
            o32, o16 = torch.full((rows_n, cols), float("nan"), device="cuda"), RK._filled16((rows_n, cols), t16)
            assert lib.rr_op_ce_embed_ln(_p(X), *[_p(t) for t in dev], eps, rows_n, T, cols, _p(o32), _p(o16), s_text, vis0, cls32, _stream()) == 0
            torch.cuda.synchronize()
            for r0 in blocks:
                r = torch.arange(r0, r0 + BLK)
                if cls32 == 0:
                    x64 = (X[r0:r0 + BLK].cpu() + typ0 + pos[pt[r % T]]).double()
                    ref, unit = RK._ln_ref(x64, gamma.double(), beta.double(), eps)
                    RK._check_ln(f"large.ce_embed_ln.rows{r0}", o32[r0:r0 + BLK], o16[r0:r0 + BLK], ref, unit, t16)
                    res[r0] = (o32[r0:r0 + BLK].clone(), o16[r0:r0 + BLK].clone())
                    cls_full = o32[::T].clone()
                else:
                    is_cls = ((r % T) == 0).cuda()
                    assert torch.isnan(o32[r0:r0 + BLK][~is_cls]).all(), f"cls32 wrote a non-CLS fp32 row near {r0}"
                    assert torch.equal(_bits(o32[r0:r0 + BLK][is_cls]), _bits(res[r0][0][is_cls]))
                    assert torch.equal(_bits(o16[r0:r0 + BLK]), _bits(res[r0][1]))
            if cls32:
                # every pair's CLS row, the ones behind the boundary included (a block of 300 rows may hold none)
                assert torch.isfinite(o32[::T]).all() and torch.equal(_bits(o32[::T]), _bits(cls_full))
            del o32, o16


def test_li_normalize_rows_beyond_4_gib(lib):
    """rr_op_li_normalize: 28 400 pairs x 512 text rows x 128 (fp32 source 7.4 GB, crossing at pair 16 384) into the 16-bit
    [pairs][593][128] buffer (4.3 GB, crossing at pair 28 292), ids mask, L2-normalised.  Nearest-16-bit rule of
    test_li_normalize_ids_mask; the 81 rows of every inspected pair that are not destinations keep their NaN."""
    n, S, T, D = 28_400, 512, 593, 128
    _need(n * S * D * 4 + n * T * D * 2 + n * S * 8 + (1 << 30))
    src = _fill(torch.empty(n * S, D, device="cuda"), 730)
    g = torch.Generator(device="cuda").manual_seed(73)
    ids = torch.randint(1, 100, (n, S), device="cuda", generator=g)
    ids[:, -3:] = 0
    with RK._op_dtype(lib, 0) as t16:
        dst = RK._li(lib, src, (n, T, D), t16, ids=ids, ids_stride=S, n_pairs=n, rpb=S, D=D, T=T)
    e_src, e_dst = GIB4 // (S * D * 4), GIB4 // (T * D * 2)
    assert e_src * S * D * 4 == GIB4 and e_dst + 2 < n
    for p in (0, e_src - 1, e_src, e_dst - 1, e_dst, e_dst + 1, n - 1):
        expect = RK._li_expect(src.view(n, S, D)[p:p + 1].cpu(), (ids[p:p + 1] != 0).double().cpu(), 1, 0, 1, 0, 1)
        RK._check_li(f"large.li_normalize.pair{p}", dst[p:p + 1], expect, list(range(S)), 1, t16)


def test_gather_rows_beyond_4_gib(lib):
    """rr_op_gather_rows: the CLS gather out of a [2 361][593][768] fp32 source (4.3 GB) and the query broadcast into a
    [45 000][32][768] fp32 destination (4.4 GB): bit-exact copies, checked whole (the gather) and on the pairs around the
    boundary (the broadcast)."""
    n, T, H = 2361, 593, 768
    _need(n * T * H * 4 + (1 << 30))
    src = _fill(torch.empty(n, T, H, device="cuda"), 740)
    dst = torch.full((n, H), float("nan"), device="cuda")
    assert lib.rr_op_gather_rows(_p(src), _p(dst), n, 1, T, H * 4, 0, 1, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert GIB4 // (T * H * 4) + 1 < n and torch.equal(_bits(dst), _bits(src[:, 0]))
    del src, dst
    n, Lq, K, off, q_lo = 45_000, 32, 100, 7, 0
    nq = (n - 1 + off) // K - q_lo + 1
    q = _fill(torch.empty(nq, Lq, H, device="cuda"), 741)
    dst = torch.full((n, Lq, H), float("nan"), device="cuda")
    assert lib.rr_op_gather_rows(_p(q), _p(dst), n, Lq, Lq, H * 4, off, K, q_lo, _stream()) == 0
    torch.cuda.synchronize()
    e = GIB4 // (Lq * H * 4)
    assert e + 50 < n
    for p0 in (0, e - 50, e, n - 50):
        p = torch.arange(p0, p0 + 50, device="cuda")
        assert torch.equal(_bits(dst[p0:p0 + 50]), _bits(q[(p + off) // K - q_lo])), f"pairs {p0}"


def test_cast16_beyond_2_31_elements(lib):
    """rr_op_cast16 over 2^31 + 4 000 floats (8.6 GB in, 4.3 GB out): torch's rounding, bit for bit, on blocks at the start, at
    elements 2^30 (byte 2^32 of the input), 2^31 (byte 2^33 of the input, byte 2^32 of the output) and the end."""
    n = (1 << 31) + 4000
    _need(n * 6 + (1 << 30))
    x = _fill(torch.empty(n // 8, 8, device="cuda"), 750).view(-1)
    y = RK._filled16((n,), torch.bfloat16)
    assert lib.rr_op_cast16(_p(x), _p(y), n, _stream()) == 0
    torch.cuda.synchronize()
    m = 1 << 16
    for i0 in (0, (1 << 30) - m, 1 << 30, (1 << 31) - m, 1 << 31, n - 4000):
        assert torch.equal(_bits(y[i0:i0 + m]), _bits(x[i0:i0 + m].bfloat16())), f"elements from {i0}"


def test_cls_heads_beyond_4_gib(lib):
    """rr_op_cls_heads reading the CLS rows of h32 [2 361][593][768] fp32 (pair p at p * T * cols: 4.3 GB): every pair against
    float64 under DOT_UNITS; the other rows hold NaN (only the CLS rows may be read)."""
    n, T, cols = 2361, 593, 768
    _need(n * T * cols * 4 + (1 << 30))
    h = torch.full((n, T, cols), float("nan"), device="cuda")
    h[:, 0] = _fill(torch.empty(n, cols, device="cuda"), 760, 2.0)
    g = torch.Generator().manual_seed(76)
    w1, w2 = torch.randn(cols, generator=g) * 0.05, torch.randn(cols, generator=g) * 0.05
    b1, b2 = torch.tensor([0.25]), torch.tensor([-1.5])
    o1, o2 = torch.full((n,), float("nan"), device="cuda"), torch.full((n,), float("nan"), device="cuda")
    dev = [t.cuda() for t in (w1, b1, w2, b2)]
    assert lib.rr_op_cls_heads(_p(h), T, cols, n, *[_p(t) for t in dev], _p(o1), _p(o2), _stream()) == 0
    torch.cuda.synchronize()
    assert GIB4 // (T * cols * 4) + 1 < n
    h0 = h[:, 0].cpu().double()
    for o, w, b in ((o1, w1, b1), (o2, w2, b2)):
        ref = h0 @ w.double() + float(b)
        unit = RK.U * ((h0 * w.double()).abs().sum(-1) + abs(float(b)))
        assert float(((o.cpu().double() - ref) / unit).abs().max()) <= RK.DOT_UNITS


def test_split_residual_value_beyond_4_gib(lib):
    """rr_op_split_residual_value over hi (bf16) / lo (fp16) [2 800 003, 768] (4.3 GB each) -> fp32 (8.6 GB, two crossings), with
    statistics: the kernel's expression (x = hi + lo; (x - mean) * rstd * gamma + beta) in float64 on the same inputs.  Bound: the
    kernel rounds five times in fp32 (the sum, the difference, two products, the last sum), each by at most 2^-24 of a magnitude
    that is at most (|x| + |mean|) * rstd * |gamma| + |beta| once carried to the result: 5 x 2^-24 of that."""
    M, N = 2_800_003, 768
    _need(M * N * 8 + (1 << 30))
    hi = _fill(torch.empty(M, N, dtype=torch.bfloat16, device="cuda"), 770, 3.0, 0.5)
    lo = _fill(torch.empty(M, N, dtype=torch.float16, device="cuda"), 771, 2.0 ** -9)
    g = torch.Generator(device="cuda").manual_seed(77)
    stats = torch.stack([0.5 + 0.1 * torch.randn(M, device="cuda", generator=g), 0.3 + 0.1 * torch.rand(M, device="cuda", generator=g)], 1).contiguous()
    gamma, beta = 1 + 0.1 * torch.randn(N, device="cuda", generator=g), 0.05 * torch.randn(N, device="cuda", generator=g)
    out = torch.full((M, N), float("nan"), device="cuda")
    assert lib.rr_op_split_residual_value(_p(hi), _p(lo), _p(stats), _p(gamma), _p(beta), M, N, _p(out), _stream()) == 0
    torch.cuda.synchronize()
    starts = set(_blocks(M, N * 2)[1])
    for k in (1, 2):
        e = k * GIB4 // (N * 4)
        starts |= {e - BLK, e}
    for r0 in sorted(starts):
        rows = slice(r0, r0 + BLK)
        x = hi[rows].double() + lo[rows].double()
        st = stats[rows].double()
        ref = (x - st[:, 0:1]) * st[:, 1:2] * gamma.double() + beta.double()
        mag = ((x.abs() + st[:, 0:1].abs()) * st[:, 1:2] * gamma.double().abs() + beta.double().abs())
        got = out[rows].double()
        assert torch.isfinite(got).all() and ((got - ref).abs() <= 5.01 * 2.0 ** -24 * mag).all(), f"rows {r0}"


def test_quantize_and_amax_beyond_2_32_elements(lib):
    """rr_op_quantize_fp8 / rr_op_amax over 2^32 + 8 000 bf16 values (8.6 GB in, 4.3 GB of codes out): the element INDEX no longer
    fits 32 bits (the fp32 input form shares the kernel and its size_t index; 17 GB more for it were not spent).  Codes byte for
    byte torch's e4m3 rounding of x * (1 / scale), the rule of test_quantize_and_amax_match_torch, on blocks at the start, around
    elements 2^31 and 2^32 and at the end; the maximum sits in the last 8 elements, which a truncated count never visits."""
    n = (1 << 32) + 8000
    _need(n * 3 + (2 << 30))
    x = _fill(torch.empty(n // 8, 8, dtype=torch.bfloat16, device="cuda"), 780).view(-1)
    x[-3] = -77.0
    amax = torch.full((1,), float("nan"), device="cuda")
    assert lib.rr_op_amax(_p(x), 0, n, _p(amax), _stream()) == 0
    torch.cuda.synchronize()
    assert amax.item() == 77.0
    scale = 77.0 / 448.0                                        # 11 / 64: exact, so 1 / scale rounds the same way on host and device
    out = torch.full((n,), 0x7F, dtype=torch.uint8, device="cuda")
    assert lib.rr_op_quantize_fp8(_p(x), 0, scale, _p(out), n, _stream()) == 0
    torch.cuda.synchronize()
    m = 1 << 16
    for i0 in (0, (1 << 31) - m, 1 << 31, (1 << 32) - m, 1 << 32, n - 8000):
        want = (x[i0:i0 + m].float() * (1.0 / scale)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
        diff = out[i0:i0 + m] != want
        assert not diff.any(), f"elements from {i0}: {int(diff.sum())} bytes differ"


# ================================================================================================ host guards (the audit above)
def test_calls_beyond_2_30_rows_are_refused_before_any_launch(lib):
    """Row counts are ints inside a forward (run_layer's rows, the row kernels' grids): rr_forward and rr_reserve refuse more than
    2^30 rows per call with RR_ERR_BAD_SHAPE before they allocate or launch — the outputs keep their NaN and the device memory in
    use does not move —, and the row-kernel launchers refuse a row or element count beyond INT_MAX."""
    import rmr_amd
    cfg = O.OracleConfig(vocab_size=100, hidden=64, layers=1, heads=1, intermediate=128, max_pos=512, ce_hidden=64, ce_heads=1,
                         ce_intermediate=128, ce_layers=1, ce_max_pos=512, li_dim=64)
    cfg.loss_fn = "BCE"
    eng = rmr_amd.RerankEngine(arch_from_cfg(cfg, False, "fp16"))
    eng.load_state_dict(O.make_weights(cfg, seed=0, vision=False))
    S, n = 512, (1 << 21) + 1                                    # n * S = 2^30 + 512 rows
    dummy = torch.zeros(S, dtype=torch.int64, device="cuda")
    logits = torch.full((2, 16), float("nan"), device="cuda")
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    rc = lib.rr_forward(eng.h, _p(dummy), _p(dummy), 0, 0, 0, n, 1, S, 0, 0, n, _p(logits[0]), _p(logits[1]), 0, 0, 0, _stream())
    assert rc == RR_ERR_BAD_SHAPE and b"rows" in lib.rr_last_error(eng.h)
    assert lib.rr_reserve(eng.h, n, 1, S, 0, 0, _stream()) == RR_ERR_BAD_SHAPE
    torch.cuda.synchronize()
    assert torch.isnan(logits).all() and torch.cuda.mem_get_info()[0] >= free0 - (64 << 20)
    x = torch.zeros(64, device="cuda")
    y = RK._filled16((64,), torch.bfloat16)
    assert lib.rr_op_li_normalize(_p(x), 0, 0, 1 << 20, 1 << 12, 4, 1 << 12, 0, 0, 1, 0, _p(y), 1, 0, 1 << 30, 0, _stream()) == RR_ERR_BAD_SHAPE
    torch.cuda.synchronize()
    assert (_bits(y) == 0x7fff).all()


# ================================================================================================ forward level
_FULL = {}


def _fullsize(name):
    if name not in _FULL:
        _FULL[name] = load_fullsize(name)
    return _FULL[name]


def _gate_of(q, dt):
    """The gate of test_full_size_logits_match_the_fp32_goldens: 1e-3 in fp16, max(1e-3, 1.5 x the reference's autocast drift)."""
    return 1e-3 if dt == "fp16" else max(1e-3, 1.5 * (q["autocast"] - q["fp32"]).abs().max().item())


def _copies_case(name, copies, dt, arch_extra=(), options=(), late_options=(), golden_gate=True):
    """`copies` queries, each the golden list of `name`, in ONE forward_ids call, against the plain one-list call on the same
    handle.  Every copy's logits bit-equal to copy 0's and to the one-list call's; copy 0 within the golden gate; the order of
    every query the stable descending sort of its logits; the loss EQUAL to the one-list call's: the per-query partials
    (loss sum, weight) are identical floats p, w; head_reduce_kernel adds them in a fixed order in double, where copies * p and
    copies * w are exact (24 + 5 bits), and (copies * p) / (copies * w) is the same real number as p / w, hence the same
    correctly rounded double and the same float — the bound on the difference is 0."""
    import rmr_amd
    cfg, w, vision, qs = _fullsize(name)
    q = qs[0]
    K, S = q["ids"].shape
    arch = arch_from_cfg(cfg, vision, dt)
    arch.update(dict(arch_extra))
    eng = rmr_amd.RerankEngine(arch)
    for k, v in options:
        eng.set_option(k, v)
    eng.load_state_dict(w)
    for k, v in late_options:
        eng.set_option(k, v)
    n = copies * K
    ws = eng.workspace_bytes(n, S)
    _need(ws + 3 * n * S * 8 + (1 << 30))
    eng.reserve(n, copies, S)
    ids, am, tt = (x.cuda().repeat(copies, 1) for x in (q["ids"], q["am"], q["tt"]))
    cls, pat = (None, None) if not vision else tuple(x.cuda().repeat(copies, *([1] * (x.dim() - 1))) for x in q["img"])
    labels = torch.zeros(n, device="cuda")
    labels[::K] = 1.0
    one = eng.forward_ids(ids[:K], am[:K], tt[:K], 1, K, None if cls is None else cls[:1], None if pat is None else pat[:1],
                          labels[:K], want_order=True)
    big = eng.forward_ids(ids, am, tt, copies, K, cls, pat, labels, want_order=True)
    torch.cuda.synchronize()
    lg = big["logits"].view(copies, K)
    assert torch.isfinite(lg).all()
    differ = (_bits(lg) != _bits(lg[0:1])).any(1).nonzero().flatten().tolist()
    assert not differ, f"copies {differ[:8]} of {copies} differ from copy 0 (max |d| {(lg - lg[0:1]).abs().max().item():.3e})"
    assert torch.equal(_bits(lg[0]), _bits(one["logits"].view(-1))), \
        f"copy 0 differs from the {K}-pair call by {(lg[0] - one['logits'].view(-1)).abs().max().item():.3e}"
    d = (lg[0].cpu() - q["fp32"]).abs().max().item()
    record_margin(f"large_index/{name}/{dt}/{copies}x{K}" + "".join(f"/{k}={v}" for k, v in tuple(arch_extra) + tuple(late_options)),
                  vs_fp32_golden=d, workspace_bytes=ws, pairs=n)
    if golden_gate:
        assert d <= _gate_of(q, dt), (d, _gate_of(q, dt))
    order = big["order"].cpu().tolist()
    rows = lg.cpu().tolist()
    for c in range(copies):
        assert order[c] == O.rank_descending_stable(rows[c]), f"query {c}"
    assert big["loss"].item() == one["loss"].item()
    return eng, (ids, am, tt, cls, pat), big


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_forward_2400_pairs_c3(dt):
    """c3_full's list (K = 100, S = 512, 81 vision tokens) 24 times in one call: 2 400 pairs, w.mid (n >= 1 179), w.qkv
    (n >= 1 572) and the fp32 rows (n >= 2 358) all beyond 2^32 bytes; the image features repeated per query.  Then the same
    2 400 pairs as eight pair_range slices of 300: they compose to the whole call (test_pair_slices_compose_to_full_forward)."""
    eng, (ids, am, tt, cls, pat), big = _copies_case("c3_full", 24, dt)
    parts = torch.full_like(big["logits"], float("nan"))
    for b in range(0, 2400, 300):
        r = eng.forward_ids(ids, am, tt, 24, 100, cls, pat, None, pair_range=(b, b + 300), want_loss=False)
        parts[b:b + 300] = r["logits"][b:b + 300]
    torch.cuda.synchronize()
    assert torch.equal(_bits(parts), _bits(big["logits"]))
    del eng
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_forward_2200_pairs_c5(dt):
    """c5_full's list (bert-large, K = 200, S = 512, text only) 11 times: 2 200 pairs (w.mid from 1 024, w.qkv from 1 366, the
    fp32 rows from 2 048)."""
    eng, _, _ = _copies_case("c5_full", 11, dt)
    del eng
    torch.cuda.empty_cache()


@pytest.mark.parametrize("form", ["fp8_ffn_down", "int8"])
def test_forward_2200_pairs_c5_eight_bit(form):
    """The 8-bit configuration over the whole stack (fp8_first_layer = 0) at 2 200 pairs: e4m3 with the e4m3 FFN-down operand
    (w.mid as bytes: crossing from 2 048 pairs) and int8 ("q8_format" 1), each bit-equal to the same handle's 200-pair call.  The
    distance to the fp32 golden is recorded, its gates are those of tests/test_gpu_fp8.py / test_gpu_int8.py at K = 200."""
    if form == "int8":
        eng, _, _ = _copies_case("c5_full", 11, "fp16", arch_extra=(("fp8", 1), ("q8_format", 1)), options=(("fp8_first_layer", 0),),
                                 golden_gate=False)
    else:
        eng, _, _ = _copies_case("c5_full", 11, "fp16", arch_extra=(("fp8", 1),), options=(("fp8_first_layer", 0),),
                                 late_options=(("fp8_ffn_down", 1),), golden_gate=False)
    del eng
    torch.cuda.empty_cache()


def test_packed_forward_2400_pairs():
    """forward_ids_packed (granule 64) over 2 400 pairs with the length mix of test_packed_forward_at_the_bench_size (24 queries x
    100 candidates, S = 512, pair lengths U[64, 512], text only, fp16), against the padded call as that test compares them: every
    logit and every order bit-equal, a second packed call bit-equal to the first."""
    import rmr_amd
    from rmr_amd.synthetic import pair_batch
    arch = rmr_amd.make_arch(dict(cross_encoder_num_hidden_layers=1, cross_encoder_max_position_embeddings=750, loss_fn="BCE"),
                             has_vision=0, compute_dtype="fp16")
    eng = rmr_amd.RerankEngine(arch)
    eng.load_state_dict(rmr_amd.synthetic_state_dict(arch, 0, True))
    Bq, K, S = 24, 100, 512
    _need(eng.workspace_bytes(Bq * K, S) + 6 * Bq * K * S * 8 + (1 << 30))
    ids, am, tt = [t.cuda() for t in pair_batch(arch["vocab_size"], Bq, K, S, regime="realistic")]
    ref = eng.forward_ids(ids, am, tt, Bq, K, None, None, want_order=True)
    got = eng.forward_ids_packed(ids, am, tt, Bq, K, None, None, granule=64, want_order=True)
    again = eng.forward_ids_packed(ids, am, tt, Bq, K, None, None, granule=64, want_order=True)
    torch.cuda.synchronize()
    assert got["packed_rows"] < 0.7 * Bq * K * S
    assert torch.equal(got["logits"], again["logits"])
    assert not eng.activation_range_exceeded()
    assert torch.isfinite(ref["logits"]).all()
    assert (got["logits"] - ref["logits"]).abs().max().item() == 0.0 and torch.equal(got["order"], ref["order"])
    del eng
    torch.cuda.empty_cache()
