"""GPU: training a PLAID codec on the device (rr_plaid_kmeans, rr_plaid_residuals, PlaidCodec.train; THE TRAINED CENTROIDS of
include/rerank_mi355.h).  The device is held to the host definition (rr_util_plaid_kmeans, itself held to a restatement of the
header's text by tests/test_plaid_train_cpu.py): table, counts and statistics, every equality torch.equal.  The sums are exact
integers added with atomics, so neither the split of the centroid range ("compress_chunk") nor contention (every row in one
cluster) nor a second run may change a bit.  A handle's li_dim is a multiple of 64: D = 16 runs through the handle-free operators
(rr_op_plaid_kmeans, rr_op_plaid_residuals: the same kernels and checks).
End to end the trained table's mean squared row-to-centroid distance is held to 1.01 times that of a float64 numpy Lloyd from the same
initial rows; measured on an MI355X: 1.0000003 [`profiles/plaid_train_parity_margins.json` "plaid_train/end_to_end_N4096_D128_C64" "mse_ratio_device_over_float64"]."""
import functools

import numpy as np
import pytest
import torch

from helpers import record_margin
from test_gpu_passage_bank import _engine

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789AB


def _L():
    from rmr_amd import _lib as L
    return L, L.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dt(L, t):
    return L.RR_F16 if t.dtype == torch.float16 else L.RR_F32


@functools.lru_cache(maxsize=None)
def _rows(D, R, seed=0):
    """Unit rows around R // 12 + 1 directions, float32 values that fp16 rounds; rows 1 and 0 are equal (the first two initial rows:
    the tie goes to cluster 0, cluster 1 is empty in iteration 0 and is re-seeded)."""
    gen = torch.Generator().manual_seed(7919 * D + R + seed)
    cen = torch.nn.functional.normalize(torch.randn(R // 12 + 1, D, generator=gen), dim=-1)
    pick = torch.randint(0, cen.shape[0], (R,), generator=gen)
    rows = torch.nn.functional.normalize(cen[pick] + 0.5 * torch.randn(R, D, generator=gen) / D ** 0.5, dim=-1)
    if R > 1:
        rows[1] = rows[0]
    return rows.contiguous()


def _host(rows, init, niters, seed=SEED):
    """rr_util_plaid_kmeans on host tensors -> (centroids fp16 [C, D], counts [C], stats [niters, 2])."""
    L, lib = _L()
    R, D = rows.shape
    Cn = init.numel()
    cen = torch.zeros((Cn, D), dtype=torch.float16)
    cnt = torch.full((Cn,), -1, dtype=torch.int32)
    stats = torch.full((max(niters, 1), 2), -1, dtype=torch.int32)
    rc = lib.rr_util_plaid_kmeans(rows.data_ptr(), _dt(L, rows), R, D, init.data_ptr(), Cn, niters, seed, cen.data_ptr(), cnt.data_ptr(),
                                  stats.data_ptr())
    assert rc == L.RR_OK, rc
    return cen, cnt, stats[:niters]


def _dev(rows_d, init, niters, seed=SEED, handle=None):
    """rr_op_plaid_kmeans (handle None) or rr_plaid_kmeans on device rows; the outputs start poisoned and come back on the host."""
    L, lib = _L()
    R, D = rows_d.shape
    Cn = init.numel()
    cen = torch.full((Cn, D), 7.0, dtype=torch.float16, device="cuda")
    cnt = torch.full((Cn,), -1, dtype=torch.int32, device="cuda")
    stats = torch.full((max(niters, 1), 2), -1, dtype=torch.int32, device="cuda")
    if handle is None:
        rc = lib.rr_op_plaid_kmeans(L.ptr(rows_d), _dt(L, rows_d), R, D, init.data_ptr(), Cn, niters, seed, L.ptr(cen), L.ptr(cnt),
                                    L.ptr(stats), _st())
    else:
        rc = lib.rr_plaid_kmeans(handle, L.ptr(rows_d), _dt(L, rows_d), R, init.data_ptr(), Cn, niters, seed, L.ptr(cen), L.ptr(cnt),
                                 L.ptr(stats), _st())
    assert rc == L.RR_OK, (rc, lib.rr_last_error(handle).decode() if handle is not None else "")
    torch.cuda.synchronize()
    return cen.cpu(), cnt.cpu(), stats[:niters].cpu()


def _same(got, want, what):
    assert torch.equal(got[0].view(torch.int16), want[0].view(torch.int16)), ("centroids", what)
    assert torch.equal(got[1], want[1]), ("counts", what, got[1].tolist(), want[1].tolist())
    assert torch.equal(got[2], want[2]), ("stats", what, got[2].tolist(), want[2].tolist())


def _chunk(value):
    L, lib = _L()
    assert lib.rr_set_tuning(b"compress_chunk", value) == L.RR_OK


# ---- 1. the device against the host definition ------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [16, 128])
@pytest.mark.parametrize("R,Cn", [(1, 1), (130, 16), (130, 40), (1000, 40), (1000, 272)])
def test_kmeans_equals_the_host_definition(D, R, Cn):
    rows32 = _rows(D, R)
    init = torch.arange(Cn, dtype=torch.int32)               # rows 0 and 1 are equal: cluster 1 starts empty
    for rows in (rows32, rows32.half()):
        rows_d = rows.cuda()
        for niters in (0, 1, 4):
            want = _host(rows, init, niters)
            _same(_dev(rows_d, init, niters), want, (D, R, Cn, rows.dtype, niters))
            if niters:
                assert int(want[2][0, 0]) == R and int(want[1].sum()) == R
                if Cn > 1:
                    assert int(want[2][0, 1]) >= 1           # the equal initial rows: the re-seed rule ran
            else:
                assert not want[1].any()


def test_kmeans_through_a_handle_and_scattered_initial_rows():
    eng, _ = _engine("int_base")                             # li_dim 128
    rows = _rows(128, 1000, seed=1)
    init = torch.randperm(1000, generator=torch.Generator().manual_seed(3))[:272].to(torch.int32).contiguous()
    want = _host(rows, init, 4)
    got = _dev(rows.cuda(), init, 4, handle=eng.h)
    _same(got, want, "handle")
    _same(_dev(rows.cuda(), init, 4, handle=eng.h), got, "second run through the grown block")
    # NULL counts and stats: the table alone
    L, lib = _L()
    cen = torch.empty((272, 128), dtype=torch.float16, device="cuda")
    assert lib.rr_plaid_kmeans(eng.h, L.ptr(rows.cuda()), L.RR_F32, 1000, init.data_ptr(), 272, 4, SEED, L.ptr(cen), None, None, _st()) == L.RR_OK
    torch.cuda.synchronize()
    assert torch.equal(cen.cpu().view(torch.int16), want[0].view(torch.int16))


# ---- 2. the centroid range in splits ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,Cn", [(128, 40), (128, 272), (16, 40)])
def test_splits_give_the_unsplit_bits(D, Cn):
    rows = _rows(D, 1000)
    init = torch.arange(Cn, dtype=torch.int32)
    want = _host(rows, init, 4)
    rows_d = rows.cuda()
    try:
        _chunk(0)
        _same(_dev(rows_d, init, 4), want, "one split")
        _chunk(16)                                           # 3 splits (the last of 8 centroids) and 17
        _same(_dev(rows_d, init, 4), want, "compress_chunk 16")
    finally:
        _chunk(0)


# ---- 3. contention: every add of an iteration lands in one table row ----------------------------------------------------------------
def test_equal_rows_sum_exactly_under_contention():
    D, R, Cn = 128, 4096, 16
    row = _rows(D, 130)[5]
    rows = row[None, :].repeat(R, 1).contiguous()
    init = torch.arange(Cn, dtype=torch.int32)
    rows_d = rows.cuda()
    a = _dev(rows_d, init, 3)
    b = _dev(rows_d, init, 3)
    _same(a, b, "two runs")
    _same(a, _host(rows, init, 3), "host")
    assert a[1].tolist() == [R] + [0] * (Cn - 1) and a[2].tolist() == [[R, Cn - 1], [0, Cn - 1], [0, Cn - 1]]
    # the mean of 4096 equal rows is the row: the table row is what the row alone gives (niters 0 normalises the initial table)
    alone = _host(rows[:1], init[:1], 0)[0]
    assert torch.equal(a[0].view(torch.int16), alone.view(torch.int16).expand(Cn, D))


# ---- 4. residuals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [16, 128])
def test_residuals_equal_the_compressed_rows_codes_and_a_float32_subtraction(D):
    L, lib = _L()
    R, Cn = 1000, 272
    rows32 = _rows(D, R, seed=2)
    cen = _host(rows32, torch.arange(Cn, dtype=torch.int32), 2)[0].contiguous()
    cut = torch.zeros(1)
    eng = _engine("int_base")[0] if D == 128 else None
    for rows in (rows32, rows32.half()):
        want_codes = torch.empty(R, dtype=torch.int32)
        scrap = torch.empty((R, D // 8), dtype=torch.uint8)
        assert lib.rr_util_plaid_compress_rows(rows.data_ptr(), _dt(L, rows), R, D, cen.data_ptr(), Cn, cut.data_ptr(), 1,
                                               want_codes.data_ptr(), scrap.data_ptr()) == L.RR_OK
        x = rows.half().float().numpy()
        want_res = x - cen.float().numpy()[want_codes.numpy()]
        rows_d, cen_d = rows.cuda(), cen.cuda()
        for chunk in (0, 16):
            codes = torch.full((R,), -7, dtype=torch.int32, device="cuda")
            res = torch.full((R, D), 9.0, dtype=torch.float32, device="cuda")
            try:
                _chunk(chunk)
                if eng is None:
                    rc = lib.rr_op_plaid_residuals(L.ptr(rows_d), _dt(L, rows), R, D, L.ptr(cen_d), Cn, L.ptr(codes), L.ptr(res), _st())
                else:
                    rc = lib.rr_plaid_residuals(eng.h, L.ptr(rows_d), _dt(L, rows), R, L.ptr(cen_d), Cn, L.ptr(codes), L.ptr(res), _st())
            finally:
                _chunk(0)
            assert rc == L.RR_OK
            torch.cuda.synchronize()
            assert torch.equal(codes.cpu(), want_codes), (D, rows.dtype, chunk)
            assert np.array_equal(res.cpu().numpy().view(np.int32), want_res.view(np.int32)), (D, rows.dtype, chunk)
        assert len(set(want_codes.tolist())) > Cn // 2


# ---- 5. end to end: train, create a bank from the codec, compress, read back --------------------------------------------------------
def _lloyd64(x, Cn, niters, seed):
    """Lloyd in float64 numpy from the first Cn rows, the re-seed rule of the definition; (normalised table, clusters re-seeded)."""
    import plaid_train_ref as T
    t = x[:Cn].copy()
    reseeded = 0
    for i in range(niters):
        code = (((x * x).sum(1))[:, None] - 2.0 * x @ t.T + (t * t).sum(1)[None, :]).argmin(1)
        n = np.bincount(code, minlength=Cn)
        for c in range(Cn):
            if n[c]:
                t[c] = x[code == c].mean(0)
            else:
                t[c] = x[T.reseed_row(seed, i, c, x.shape[0])]
                reseeded += 1
    return t / np.linalg.norm(t, axis=1, keepdims=True), reseeded


def _mse(x, table):
    d2 = ((x * x).sum(1))[:, None] - 2.0 * x @ table.T + (table * table).sum(1)[None, :]
    return float(d2.min(1).mean())


def test_train_compress_read_end_to_end():
    import rmr_amd
    eng, _ = _engine("int_base")
    N, D, Cn, nbits, niters, seed = 4096, 128, 64, 2, 8, 123
    gen = torch.Generator().manual_seed(99)
    planted = torch.nn.functional.normalize(torch.randn(Cn, D, generator=gen), dim=-1)
    # the shuffle PlaidCodec.train makes: its first Cn rows, the initial centroids, are given one planted direction each
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(seed))
    label = torch.randint(0, Cn, (N,), generator=gen)
    label[perm[:Cn]] = torch.arange(Cn)
    emb = torch.nn.functional.normalize(planted[label] + 0.25 * torch.randn(N, D, generator=gen) / D ** 0.5, dim=-1).half()
    codec = rmr_amd.PlaidCodec.train(eng, emb.cuda(), nbits, Cn, niters=niters, seed=seed)
    n_held = int(min(0.05 * N, 50_000))
    assert codec.n_centroids == Cn and codec.bucket_cutoffs is not None and codec.train_stats["n_heldout"] == n_held
    assert codec.train_stats["n_train"] == N - n_held and int(codec.train_stats["counts"].sum()) == N - n_held
    assert not codec.train_stats["stats"][:, 1].any() and codec.avg_residual > 0
    x = emb[perm][:N - n_held].double().numpy()
    ref, reseeded = _lloyd64(x, Cn, niters, seed)
    assert reseeded == 0
    ratio = _mse(x, codec.centroids.double().numpy()) / _mse(x, ref)
    record_margin("plaid_train/end_to_end_N4096_D128_C64", mse_ratio_device_over_float64=ratio, gate=1.01)
    print(f"plaid_train end to end: mse ratio {ratio:.8f}")
    assert ratio <= 1.01, ratio
    bank = eng.create_bank(N, N // 64, codec=codec)
    ids = list(range(N // 64))
    bank.add_compress(ids, emb.view(N // 64, 64, D).cuda(), torch.ones(N // 64, 64).cuda(), lengths=[64] * (N // 64))
    back = torch.cat([bank.read(i)[0] for i in ids]).float()
    cos = torch.nn.functional.cosine_similarity(back, emb.float(), dim=-1)
    print(f"plaid_train end to end: min cosine {float(cos.min()):.4f}")
    assert float(cos.min()) >= 0.9, float(cos.min())


# ---- 6. the refusals that need a device ---------------------------------------------------------------------------------------------
def test_refusals_on_the_device():
    L, lib = _L()
    eng, _ = _engine("int_base")
    rows = _rows(128, 130).cuda()
    init = torch.arange(16, dtype=torch.int32)
    cen = torch.full((16, 128), 7.0, dtype=torch.float16, device="cuda")
    codes = torch.empty(130, dtype=torch.int32, device="cuda")
    res = torch.empty((130, 128), dtype=torch.float32, device="cuda")

    def kmeans(h=eng.h, r=rows, dtype=L.RR_F32, R=130, ini=init, Cn=16, niters=1, out=cen, stream=None):
        return lib.rr_plaid_kmeans(h, L.ptr(r) if torch.is_tensor(r) else r, dtype, R, ini.data_ptr(), Cn, niters, SEED,
                                   L.ptr(out) if torch.is_tensor(out) else out, None, None, _st() if stream is None else stream)

    def err():
        return lib.rr_last_error(eng.h).decode()
    assert kmeans(Cn=0) == L.RR_ERR_BAD_SHAPE and kmeans(Cn=131, ini=torch.arange(131, dtype=torch.int32)) == L.RR_ERR_BAD_SHAPE
    assert "centroids of 130 rows" in err()
    bad = init.clone()
    bad[3] = 130
    assert kmeans(ini=bad) == L.RR_ERR_BAD_SHAPE and "outside [0, 130)" in err()
    bad[3] = 2
    assert kmeans(ini=bad) == L.RR_ERR_BAD_SHAPE and "initial row 2 is named twice" in err()
    assert kmeans(dtype=L.RR_BF16) == L.RR_ERR_BAD_DTYPE
    assert kmeans(r=rows.data_ptr() + 4) == L.RR_ERR_BAD_ARG and "16-byte aligned" in err()
    assert kmeans(out=cen.data_ptr() + 2) == L.RR_ERR_BAD_ARG
    assert kmeans(R=(1 << 30) + 1) == L.RR_ERR_UNSUPPORTED and "2^30" in err()
    assert kmeans(niters=-1) == L.RR_ERR_BAD_SHAPE
    assert kmeans(r=None) == L.RR_ERR_BAD_ARG and kmeans(h=None) == L.RR_ERR_BAD_ARG
    probe = torch.zeros(1, device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            probe.add_(1.0)                                  # the graph holds this node alone
            rc = kmeans()
            msg = err()
            rc2 = lib.rr_plaid_residuals(eng.h, L.ptr(rows), L.RR_F32, 130, L.ptr(cen), 16, L.ptr(codes), L.ptr(res), _st())
    assert rc == L.RR_ERR_BAD_ARG and msg == "rr_plaid_kmeans cannot be captured into a graph (it stages its descriptors from the host)"
    assert rc2 == L.RR_ERR_BAD_ARG and "rr_plaid_residuals cannot be captured" in err()
    torch.cuda.synchronize()
    assert bool((cen == 7.0).all())                          # nothing was enqueued by any refused call
    if torch.cuda.device_count() >= 2:
        other = _rows(128, 130).to("cuda:1")
        assert kmeans(r=other) == L.RR_ERR_BAD_ARG and "rows live on device 1" in err()
    assert kmeans() == L.RR_OK
    torch.cuda.synchronize()
    assert not bool((cen == 7.0).all())
    # PlaidCodec.train: an empty held-out block, and one torch.quantile does not take (more than 2^24 elements)
    import rmr_amd
    with pytest.raises(ValueError, match="held-out block is empty"):
        rmr_amd.PlaidCodec.train(eng, rows[:16], 2, 4)
    big = torch.zeros(((1 << 17) + 1, 128), dtype=torch.float16, device="cuda")
    with pytest.raises(ValueError, match="torch.quantile takes at most"):
        rmr_amd.PlaidCodec.train(eng, big, 2, 64, heldout_fraction=1.0, heldout_max=1 << 30)
    with pytest.raises(ValueError, match="device tensor"):
        rmr_amd.PlaidCodec.train(eng, rows.cpu(), 2, 4)
