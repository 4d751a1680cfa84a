"""CPU: training a PLAID codec (rr_util_plaid_kmeans, PlaidCodec.bucket_statistics / save, plaid_num_partitions).  The host
definition of THE TRAINED CENTROIDS (include/rerank_mi355.h, rr_plaid_kmeans) against a numpy restatement of the header's text
(tests/plaid_train_ref.py) bit for bit — table, counts and statistics — on the cases the definition settles by rule: equal initial
rows (the tie, the empty cluster, the re-seed), clamped values, a NaN, the smallest fp16 subnormal; the refusals of the entry; the
quantile stage against what the reference's _compute_avg_residual gave (tests/golden/plaid_train_ref.npz, made by
tests/golden/make_plaid_train_fixture.py); the codec written and read back as an index.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch

import plaid_train_ref as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plaid_train_ref.npz")
SEED = 0xC0FFEE1234567


def _lib():
    from rmr_amd import _lib as L
    return L, L.load()


def _host(rows, init, niters, seed=SEED, D=None, Cn=None, R=None, dtype=None):
    """rr_util_plaid_kmeans on numpy arrays -> (rc, centroids uint16 [C, D], counts, stats [niters, 2])."""
    L, lib = _lib()
    rows = np.ascontiguousarray(rows)
    init = np.ascontiguousarray(init, dtype=np.int32)
    R = rows.shape[0] if R is None else R
    D = rows.shape[1] if D is None else D
    Cn = init.size if Cn is None else Cn
    cen = np.full((max(Cn, 1), D), 0x1234, dtype=np.uint16)
    cnt = np.full(max(Cn, 1), -1, dtype=np.int32)
    stats = np.full((max(niters, 1), 2), -1, dtype=np.int32)
    if dtype is None:
        dtype = L.RR_F16 if rows.dtype == np.float16 else L.RR_F32
    rc = lib.rr_util_plaid_kmeans(rows.ctypes.data, dtype, R, D, init.ctypes.data, Cn, niters, seed, cen.ctypes.data, cnt.ctypes.data,
                                  stats.ctypes.data)
    return rc, cen, cnt, stats[:max(niters, 0)]


def _bits(h):
    """fp16 bits with every NaN made one value: a NaN's sign and payload are not part of the definition."""
    h = np.asarray(h).view(np.uint16).copy()
    h[(h & 0x7fff) > 0x7c00] = 0x7e00
    return h


def _check(rows, init, niters, seed=SEED):
    rc, cen, cnt, stats = _host(rows, init, niters, seed)
    assert rc == 0
    want = T.kmeans(rows, init, niters, seed)
    assert np.array_equal(_bits(cen), _bits(want[0])), "centroids"
    assert np.array_equal(cnt, want[1]), (cnt.tolist(), want[1].tolist())
    assert np.array_equal(stats, want[2]), (stats.tolist(), want[2].tolist())
    return cen.view(np.float16), cnt, stats


def _rows(D, R, seed):
    rng = np.random.default_rng(1000 * D + R + seed)
    cen = rng.standard_normal((max(R // 10, 2), D))
    rows = cen[rng.integers(0, cen.shape[0], R)] + 0.4 * rng.standard_normal((R, D))
    return (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("D,Cn,R,niters", [(16, 5, 60, 3), (16, 16, 200, 1), (16, 40, 200, 3), (64, 5, 40, 0), (64, 16, 120, 3),
                                           (64, 40, 90, 1), (16, 40, 40, 0)])
@pytest.mark.parametrize("half", [False, True])
def test_host_kmeans_equals_the_restatement(D, Cn, R, niters, half):
    rows = _rows(D, R, 0)
    assert not np.array_equal(rows.astype(np.float16).astype(np.float32), rows)        # float32 values that fp16 rounds
    init = np.random.default_rng(5).permutation(R)[:Cn]
    cen, cnt, stats = _check(rows.astype(np.float16) if half else rows, init, niters)
    if niters:
        assert int(cnt.sum()) == R and int(stats[0, 0]) == R
    else:
        assert not cnt.any() and stats.shape == (0, 2)


def test_equal_initial_rows_tie_low_and_reseed():
    rows = _rows(16, 60, 1)
    rows[7] = rows[2]
    init = np.array([2, 11, 7, 30, 41])                      # clusters 0 and 2 start equal: every tie goes to 0, 2 is empty
    _, _, stats = _check(rows, init, 3)
    assert int(stats[0, 1]) >= 1
    _, cnt, _ = _check(rows, init, 1)
    assert cnt[2] == 0 and cnt[0] >= 2                       # rows 2 and 7 both went to cluster 0
    _check(rows, init, 3, seed=SEED ^ 1)                     # another seed, another re-seed row
    assert T.reseed_row(SEED, 0, 2, 60) != T.reseed_row(SEED ^ 1, 0, 2, 60)


def test_clamped_values_a_nan_and_the_smallest_subnormal():
    rows = _rows(16, 50, 2)
    rows[3, 0], rows[3, 1] = 255.875, -255.875               # inside the clamp: summed as they are
    rows[4, 2], rows[5, 2] = 300.0, -np.inf                  # clamped to 256 and -256
    rows[6, 5] = np.nan                                      # fix(NaN) = 0
    rows[8, 7] = 2.0 ** -24                                  # one unit of the fixed point
    rows[9, 7] = -(2.0 ** -24)
    for init in (np.array([0, 1, 2, 10, 11]), np.array([3, 4, 5, 6, 8])):      # the special rows as members, and as centroids
        for half in (False, True):
            _check(rows.astype(np.float16) if half else rows, init, 3)
    # the sum itself: one cluster holds everything, its mean is the fixed-point sum over R
    fixed = T.fix(rows.astype(np.float16).astype(np.float32))
    assert fixed[3, 0] == int(255.875 * 2 ** 24) and fixed[4, 2] == 2 ** 32 and fixed[5, 2] == -2 ** 32 and fixed[6, 5] == 0
    assert fixed[8, 7] == 1 and fixed[9, 7] == -1


def test_refusals():
    L, _ = _lib()
    rows = _rows(16, 40, 3)
    init = np.arange(5)
    assert _host(rows, init, 1)[0] == L.RR_OK
    assert _host(rows, init, 1, Cn=0)[0] == L.RR_ERR_BAD_SHAPE
    assert _host(rows, np.arange(41) % 40, 1, Cn=41)[0] == L.RR_ERR_BAD_SHAPE          # C > R
    assert _host(rows, np.array([0, 1, 40, 3, 4]), 1)[0] == L.RR_ERR_BAD_SHAPE         # out of range
    assert _host(rows, np.array([0, 1, -1, 3, 4]), 1)[0] == L.RR_ERR_BAD_SHAPE
    assert _host(rows, np.array([0, 1, 3, 3, 4]), 1)[0] == L.RR_ERR_BAD_SHAPE          # repeated
    assert _host(rows, init, -1)[0] == L.RR_ERR_BAD_SHAPE
    assert _host(rows, init, 1, dtype=L.RR_BF16)[0] == L.RR_ERR_BAD_DTYPE
    assert _host(rows, init, 1, R=(1 << 30) + 1)[0] == L.RR_ERR_UNSUPPORTED            # refused before a row is read
    for D in (8, 24, 48, 1024):
        assert _host(np.zeros((40, D), np.float32), init, 1)[0] == L.RR_ERR_UNSUPPORTED
    lib = _lib()[1]
    assert lib.rr_util_plaid_kmeans(None, L.RR_F32, 40, 16, init.astype(np.int32).ctypes.data, 5, 1, 0, None, None, None) == L.RR_ERR_BAD_ARG


def test_the_quantile_stage_equals_the_reference():
    """The fixture's residuals through PlaidCodec.bucket_statistics: cutoffs, weights and avg_residual of the reference's
    _compute_avg_residual (CPU branch) bit for bit.  The fixture's rows have a best centroid more than 1e-3 ahead of the second, so
    the reference's matmul and the library's chain choose the same code and the residuals are the same float32 subtractions."""
    import rmr_amd
    z = np.load(GOLDEN)
    rows, cen, nbits = z["rows"], z["centroids"], int(z["nbits"])
    assert rows.dtype == np.float16 and rows.shape == (256, 16) and cen.dtype == np.float16 and cen.shape == (8, 16) and nbits == 2
    assert float(z["min_margin"]) > 1e-3
    codec = rmr_amd.PlaidCodec(torch.from_numpy(cen), torch.zeros(4), nbits, bucket_cutoffs=torch.zeros(3))
    codes, _ = codec.compress(torch.from_numpy(rows))
    assert np.array_equal(codes.numpy(), z["codes"])
    res = torch.from_numpy(rows).float() - torch.from_numpy(cen).float()[codes.long()]
    cut, w, avg = rmr_amd.PlaidCodec.bucket_statistics(res, nbits)
    assert np.array_equal(cut.numpy().view(np.int32), z["cutoffs"].view(np.int32))
    assert np.array_equal(w.numpy().view(np.int32), z["weights"].view(np.int32))
    assert np.float32(avg).view(np.int32) == z["avg_residual"].astype(np.float32).view(np.int32)
    with pytest.raises(ValueError):
        rmr_amd.PlaidCodec.bucket_statistics(res[:0], nbits)
    with pytest.raises(ValueError):
        rmr_amd.PlaidCodec.bucket_statistics(torch.zeros(1).expand((1 << 16) + 1, 256), nbits)


def test_save_then_read_plaid_index(tmp_path):
    import rmr_amd
    gen = torch.Generator().manual_seed(4)
    codec = rmr_amd.PlaidCodec(torch.randn(24, 64, generator=gen), torch.randn(16, generator=gen).sort().values, 4,
                               bucket_cutoffs=torch.randn(15, generator=gen).sort().values)
    codec.avg_residual = 0.03125
    path = str(tmp_path / "index")
    codec.save(path)
    with open(os.path.join(path, "metadata.json"), "w") as f:
        json.dump({"config": {"nbits": 4, "dim": 64}, "num_chunks": 0}, f)
    back, chunks = rmr_amd.read_plaid_index(path)
    assert list(chunks) == [] and back.nbits == 4
    assert torch.equal(back.centroids.view(torch.int16), codec.centroids.view(torch.int16))
    assert torch.equal(back.bucket_cutoffs, codec.bucket_cutoffs) and torch.equal(back.bucket_weights, codec.bucket_weights)
    assert float(torch.load(os.path.join(path, "avg_residual.pt"))) == 0.03125
    with pytest.raises(ValueError):
        rmr_amd.PlaidCodec(codec.centroids, codec.bucket_weights, 4).save(path)


def test_plaid_num_partitions():
    import rmr_amd
    f = rmr_amd.plaid_num_partitions
    assert [f(n) for n in (1, 4, 255, 256, 257, 1023, 1024, 10 ** 6, 10 ** 8)] == [16, 32, 128, 256, 256, 256, 512, 8192, 131072]
    with pytest.raises(ValueError):
        f(0)
