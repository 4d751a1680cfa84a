"""GPU: codec training and compression (rr_plaid_kmeans, rr_plaid_residuals, rr_op_plaid_compress_rows; csrc/plaid_train.hip,
csrc/bank_compress.hip, csrc/plaid_assign.h) at real centroid counts, against an oracle that calls nothing of the library.

tests/test_gpu_plaid_train.py and tests/test_gpu_plaid_compress.py stop at 272 and 200 centroids and hold the device to the library's
own host code, which shares train_fix, rank_key and the norm with the kernels.  Here the inputs are the exact cases of
tests/plaid_train_exact_cases.py: every score is exact in float32 whatever the order of its sum, so a float64 numpy matmul predicts
every code, and the rest of the definition is restated there in numpy.  What only these cases reach:
  km4096    the automatic split plan at 16 splits of 256 centroids; 64 tiles a wave; bias loads up to entry 4095
  km512d    D 512: the halved column block (jt 2) under the bias, 64 lanes a table row, 8 trips of the accumulate loop
  km256d    D 256: 4 trips        km32d  D 32: two rows side by side in a wave instruction, R no multiple of 32
  km64d     D 64, as many centroids as rows (nearly)        km16d  D 16 at 4096 centroids
  cp65536   64 splits of 1024 centroids, nbits 8 and 2      cp262144  codes beyond 65 535, 64 splits of 4096, nbits 1
and, on all of them, equal table rows at index distances 16, 64, 256, 1024, 4096 and C / 2 whose tie the LOWER index must win, across
tiles, waves and splits.  km4096 and km32d run again at "compress_chunk" 16 and at the largest chunk that leaves two splits.
Beside the scale cases: D = 32, 64, 256 and 512 on ordinary unit rows against the host definition (tests/test_gpu_plaid_train.py has
16 and 128), and clamped, infinite, NaN, subnormal and float32-only values (65 519 rounds to 65 504, 65 520 to +inf) as members and
as initial centroids, against the host definition AND the restatement of tests/plaid_train_ref.py.
tests/test_plaid_train_exact_cases_cpu.py shows on the oracle alone that the cases bite.  No tolerance anywhere."""
import numpy as np
import pytest
import torch

import plaid_compress_ref as P
import plaid_train_exact_cases as X
import plaid_train_ref as T
from test_gpu_passage_bank import _engine
from test_gpu_plaid_train import _chunk, _dev, _dt, _host, _L, _rows, _same, _st
from test_plaid_train_cpu import _bits
from test_plaid_train_cpu import _rows as _cpu_rows

pytestmark = pytest.mark.gpu

ENGINE_OF = {64: "int_tiny", 128: "int_base"}                # the li_dim of the fixtures of test_gpu_passage_bank._engine
KM_CASES = [n for n in X.KM if n != "tiny"]


def _handle(D):
    return _engine(ENGINE_OF[D])[0].h if D in ENGINE_OF else None


def _held(got, want, what):
    """Device (torch, host) against the oracle's dict: table bits, counts, statistics."""
    assert np.array_equal(_bits(got[0].numpy()), _bits(want["centroids"])), ("centroids", what)
    assert np.array_equal(got[1].numpy(), want["counts"]), ("counts", what)
    assert np.array_equal(got[2].numpy(), want["stats"]), ("stats", what, got[2].tolist(), want["stats"].tolist())


# ---- 1. k-means at scale against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", KM_CASES)
def test_kmeans_equals_the_oracle(name):
    p = X.get(name)
    init = torch.from_numpy(p["init_rows"])
    h = _handle(p["D"])
    for src in ("rows16", "rows32"):
        rows_d = torch.from_numpy(p[src]).cuda()
        _held(_dev(rows_d, init, p["niters"], p["seed"]), p["want"], (name, src, "operator"))
        if h is not None:
            _held(_dev(rows_d, init, p["niters"], p["seed"], handle=h), p["want"], (name, src, "handle"))


@pytest.mark.parametrize("name", ["km4096", "km32d"])
def test_kmeans_in_forced_splits_equals_the_oracle(name):
    p = X.get(name)
    C = p["C"]
    init = torch.from_numpy(p["init_rows"])
    rows_d = torch.from_numpy(p["rows32"]).cuda()
    two = (C + 15) // 16 * 16 - 16                           # the largest chunk that leaves two splits
    assert two < C <= 2 * two
    try:
        for chunk in (16, two):
            _chunk(chunk)
            _held(_dev(rows_d, init, p["niters"], p["seed"]), p["want"], (name, "compress_chunk", chunk))
    finally:
        _chunk(0)


# ---- 2. compression and residuals at scale against the oracle ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(X.CP))
def test_compress_and_residuals_equal_the_oracle(name):
    L, lib = _L()
    p = X.get(name)
    R, D, C = p["R"], p["D"], p["C"]
    cen_d = torch.from_numpy(p["centroids"]).cuda()
    h = _handle(D)
    for src in ("rows16", "rows32"):
        rows_d = torch.from_numpy(p[src]).cuda()
        for nbits, q in p["packed"].items():
            codes = torch.full((R,), -7, dtype=torch.int32, device="cuda")
            by = torch.full((R, D // 8 * nbits), 0xA5, dtype=torch.uint8, device="cuda")
            cut_d = torch.from_numpy(q["cutoffs"]).cuda()
            assert lib.rr_op_plaid_compress_rows(L.ptr(rows_d), _dt(L, rows_d), R, D, L.ptr(cen_d), C, L.ptr(cut_d), nbits, L.ptr(codes),
                                                 L.ptr(by), _st()) == L.RR_OK
            torch.cuda.synchronize()
            assert np.array_equal(codes.cpu().numpy(), p["codes"]), (name, src, nbits, "codes")
            assert np.array_equal(by.cpu().numpy(), q["bytes"]), (name, src, nbits, "bytes")
        for handle in (None, h) if h is not None else (None,):
            codes = torch.full((R,), -7, dtype=torch.int32, device="cuda")
            res = torch.full((R, D), 9.0, dtype=torch.float32, device="cuda")
            if handle is None:
                rc = lib.rr_op_plaid_residuals(L.ptr(rows_d), _dt(L, rows_d), R, D, L.ptr(cen_d), C, L.ptr(codes), L.ptr(res), _st())
            else:
                rc = lib.rr_plaid_residuals(handle, L.ptr(rows_d), _dt(L, rows_d), R, L.ptr(cen_d), C, L.ptr(codes), L.ptr(res), _st())
            assert rc == L.RR_OK
            torch.cuda.synchronize()
            assert np.array_equal(codes.cpu().numpy(), p["codes"]), (name, src, "residual codes", handle is not None)
            assert np.array_equal(res.cpu().numpy().view(np.int32), p["residuals"].view(np.int32)), (name, src, "residuals")


# ---- 3. the dimensions the sibling file leaves out, against the host definition ----------------------------------------------------------
@pytest.mark.parametrize("D", [32, 64, 256, 512])
@pytest.mark.parametrize("R,Cn", [(1, 1), (130, 40), (1000, 272)])
def test_kmeans_equals_the_host_definition_at_the_other_dimensions(D, R, Cn):
    rows32 = _rows(D, R)
    init = torch.arange(Cn, dtype=torch.int32)               # rows 0 and 1 are equal: cluster 1 starts empty
    for rows in (rows32, rows32.half()):
        rows_d = rows.cuda()
        for niters in (0, 1, 4):
            want = _host(rows, init, niters)
            _same(_dev(rows_d, init, niters), want, (D, R, Cn, rows.dtype, niters))
            if niters and Cn > 1:
                assert int(want[2][0, 0]) == R and int(want[2][0, 1]) >= 1


# ---- 4. specials on the device ------------------------------------------------------------------------------------------------------
def _special_rows(D):
    """The rows of tests/test_plaid_train_cpu.py's test_clamped_values_a_nan_and_the_smallest_subnormal, plus values only a float32
    source holds."""
    rows = _cpu_rows(D, 50, 2)
    rows[3, 0], rows[3, 1] = 255.875, -255.875               # inside the clamp: summed as they are
    rows[4, 2], rows[5, 2] = 300.0, -np.inf                  # clamped to 256 and -256
    rows[6, 5] = np.nan                                      # fix(NaN) = 0
    rows[8, 7] = 2.0 ** -24                                  # one unit of the fixed point
    rows[9, 7] = -(2.0 ** -24)
    rows[12, 3] = 65519.0                                    # rounds to 65504, the largest fp16
    rows[13, 4] = 65520.0                                    # rounds to +inf
    rows[14, 6] = 1e6                                        # +inf
    rows[15, 8] = 1e-30                                      # 0
    return rows


SPECIAL_INITS = ([0, 1, 2, 10, 11], [3, 4, 5, 6, 8], [9, 12, 13, 14, 15])      # the special rows as members, and as centroids


@pytest.mark.parametrize("D", [16, 128])
def test_specials_equal_the_host_definition_and_the_restatement(D):
    rows = _special_rows(D)
    with np.errstate(over="ignore"):
        x16 = rows.astype(np.float16)
    assert x16[12, 3] == 65504.0 and np.isposinf(x16[13, 4]) and np.isposinf(x16[14, 6]) and x16[15, 8] == 0 and rows[15, 8] != 0
    fixed = T.fix(x16.astype(np.float32))
    assert fixed[3, 0] == int(255.875 * 2 ** 24) and fixed[4, 2] == 2 ** 32 and fixed[5, 2] == -2 ** 32 and fixed[6, 5] == 0
    assert fixed[8, 7] == 1 and fixed[9, 7] == -1 and fixed[12, 3] == 2 ** 32 and fixed[13, 4] == 2 ** 32
    h = _handle(D)
    nan_tables = 0
    for ini in SPECIAL_INITS:
        init = torch.tensor(ini, dtype=torch.int32)
        for src in (rows, x16):
            t = torch.from_numpy(src)
            t_d = t.cuda()
            for niters in (0, 3):                            # 0: the initial table through the norm alone
                with np.errstate(over="ignore"):       # 65 520 and 1e6 overflow to +inf in fp16: meant
                    want = T.kmeans(src, np.array(ini), niters, X.SEED)
                runs = [(_host(t, init, niters), "host"), (_dev(t_d, init, niters), "operator")]
                if h is not None:
                    runs.append((_dev(t_d, init, niters, handle=h), "handle"))
                for got, what in runs:
                    assert np.array_equal(_bits(got[0].numpy()), _bits(want[0])), ("centroids", what, D, ini, src.dtype, niters)
                    assert np.array_equal(got[1].numpy(), want[1]), ("counts", what, D, ini, src.dtype, niters)
                    assert np.array_equal(got[2].numpy(), want[2]), ("stats", what, D, ini, src.dtype, niters)
                nan_tables += bool(np.isnan(want[0].astype(np.float32)).any())
    assert nan_tables >= 4                                   # a NaN row's norm is NaN, an infinite row divides to NaN


def _canon32(a):
    """float32 bits with every NaN made one value."""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).copy()
    b[(b & 0x7fffffff) > 0x7f800000] = 0x7fc00000
    return b


@pytest.mark.parametrize("D", [16, 128])
def test_residuals_of_the_specials_equal_the_restatement(D):
    L, lib = _L()
    rows = _special_rows(D)
    with np.errstate(over="ignore"):
        x16 = rows.astype(np.float16)
    table = x16[[0, 4, 5, 6, 12]].copy()                      # a table with 300, -inf, a NaN and 65504 in it
    cut = np.zeros(1, dtype=np.float32)
    with np.errstate(over="ignore"):
        want_codes, _, _ = P.compress(rows, table, cut, 1)
    assert len(set(want_codes.tolist())) >= 3
    with np.errstate(all="ignore"):
        want_res = x16.astype(np.float32) - table.astype(np.float32)[want_codes]
    assert np.isnan(want_res).any() and np.isinf(want_res).any()
    cen_d = torch.from_numpy(table).cuda()
    h = _handle(D)
    for src in (rows, x16):
        host_codes = np.full(50, -7, dtype=np.int32)
        scrap = np.zeros((50, D // 8), dtype=np.uint8)
        assert lib.rr_util_plaid_compress_rows(src.ctypes.data, L.RR_F16 if src.dtype == np.float16 else L.RR_F32, 50, D, table.ctypes.data, 5,
                                               cut.ctypes.data, 1, host_codes.ctypes.data, scrap.ctypes.data) == L.RR_OK
        assert np.array_equal(host_codes, want_codes)
        rows_d = torch.from_numpy(src).cuda()
        for handle in (None, h) if h is not None else (None,):
            codes = torch.full((50,), -7, dtype=torch.int32, device="cuda")
            res = torch.full((50, D), 9.0, dtype=torch.float32, device="cuda")
            if handle is None:
                rc = lib.rr_op_plaid_residuals(L.ptr(rows_d), _dt(L, rows_d), 50, D, L.ptr(cen_d), 5, L.ptr(codes), L.ptr(res), _st())
            else:
                rc = lib.rr_plaid_residuals(handle, L.ptr(rows_d), _dt(L, rows_d), 50, L.ptr(cen_d), 5, L.ptr(codes), L.ptr(res), _st())
            assert rc == L.RR_OK
            torch.cuda.synchronize()
            assert np.array_equal(codes.cpu().numpy(), want_codes), (D, src.dtype, handle is not None)
            assert np.array_equal(_canon32(res.cpu().numpy()), _canon32(want_res)), (D, src.dtype, handle is not None)
