"""GPU: compressing embeddings into a compressed passage bank on the device (rr_bank_add_compress, rr_op_plaid_compress_rows;
the compressed row of include/rerank_mi355.h).  The device is held to the host definition (rr_util_plaid_compress_rows /
PlaidCodec.compress, itself held to the reference's ResidualCodec.compress by tests/test_plaid_compress_cpu.py): codes and packed
bytes, every equality torch.equal.  A code is one maximum over 64-bit rank keys, so it may not depend on how the centroid range is
divided: the "compress_chunk" cases force several splits at a small C and ask for the unsplit result."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import plaid_compress_ref as P
from test_gpu_passage_bank import _engine

pytestmark = pytest.mark.gpu

C_SIZES = (1, 16, 17, 80, 200)
R_SIZES = (1, 15, 16, 17, 130)
R_MAX = max(R_SIZES)


def _L():
    from rmr_amd import _lib as L
    return L, L.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _tables(D, nbits, Cn, seed=0):
    """fp16 unit centroids, non-decreasing cutoffs of residual size (two equal neighbours at nbits >= 2), unit rows around them."""
    gen = torch.Generator().manual_seed(1000 * D + 10 * nbits + Cn + seed)
    cen = torch.nn.functional.normalize(torch.randn(Cn, D, generator=gen), dim=-1).half()
    cut = (torch.randn((1 << nbits) - 1, generator=gen) * (0.6 / D ** 0.5)).sort().values
    if cut.numel() > 2:
        cut[2] = cut[1]
    pick = torch.randint(0, Cn, (R_MAX,), generator=gen)
    rows = torch.nn.functional.normalize(cen[pick].float() + 0.8 * torch.randn(R_MAX, D, generator=gen) / D ** 0.5, dim=-1)
    rows[R_MAX // 2:] = torch.nn.functional.normalize(torch.randn(R_MAX - R_MAX // 2, D, generator=gen), dim=-1)
    return cen.contiguous(), cut.float().contiguous(), rows.contiguous()


def _host(rows, cen, cut, nbits):
    """rr_util_plaid_compress_rows on host tensors (rows float32 or float16)."""
    L, lib = _L()
    R, D = rows.shape
    codes = torch.empty(R, dtype=torch.int32)
    res = torch.empty((R, D // 8 * nbits), dtype=torch.uint8)
    rc = lib.rr_util_plaid_compress_rows(rows.data_ptr(), L.RR_F16 if rows.dtype == torch.float16 else L.RR_F32, R, D, cen.data_ptr(),
                                         cen.shape[0], cut.data_ptr(), nbits, codes.data_ptr(), res.data_ptr())
    assert rc == L.RR_OK
    return codes, res


def _dev(rows_d, cen_d, cut_d, nbits):
    """rr_op_plaid_compress_rows on device tensors; the outputs start poisoned and come back on the host."""
    L, lib = _L()
    R, D = rows_d.shape
    codes = torch.full((R,), -7, dtype=torch.int32, device="cuda")
    res = torch.full((R, D // 8 * nbits), 0xA5, dtype=torch.uint8, device="cuda")
    rc = lib.rr_op_plaid_compress_rows(L.ptr(rows_d), L.RR_F16 if rows_d.dtype == torch.float16 else L.RR_F32, R, D, L.ptr(cen_d),
                                       cen_d.shape[0], L.ptr(cut_d), nbits, L.ptr(codes), L.ptr(res), _st())
    assert rc == L.RR_OK, rc
    return codes.cpu(), res.cpu()


def _chunk(value):
    L, lib = _L()
    assert lib.rr_set_tuning(b"compress_chunk", value) == L.RR_OK


# ---- 1. the operator against the host definition ----------------------------------------------------------------------------
@pytest.mark.parametrize("D", [16, 64, 128, 512])            # 512: the column block is halved (twice) by the LDS limit
def test_operator_equals_the_host_definition(D):
    for nbits in (1, 2, 4, 8):
        if D % (8 * nbits):
            continue
        for Cn in C_SIZES:
            cen, cut, rows32 = _tables(D, nbits, Cn)
            assert not torch.equal(rows32.half().float(), rows32)          # float32 values that fp16 rounds
            cen_d, cut_d = cen.cuda(), cut.cuda()
            for rows in (rows32, rows32.half()):
                want_c, want_r = _host(rows, cen, cut, nbits)              # rows are independent: R rows = the first R of these
                rows_d = rows.cuda()
                for R in R_SIZES:
                    got_c, got_r = _dev(rows_d[:R].contiguous(), cen_d, cut_d, nbits)
                    assert torch.equal(got_c, want_c[:R]), (D, nbits, Cn, R, rows.dtype)
                    assert torch.equal(got_r, want_r[:R]), (D, nbits, Cn, R, rows.dtype)
            if Cn > 1:
                assert len(set(want_c.tolist())) > 1


# ---- 2. the centroid range in splits ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,nbits", [(64, 8), (128, 2), (16, 1)])
def test_splits_give_the_unsplit_codes(D, nbits):
    cen, cut, rows = _tables(D, nbits, 200, seed=1)
    cen_d, cut_d, rows_d = cen.cuda(), cut.cuda(), rows.cuda()
    want = _host(rows, cen, cut, nbits)
    try:
        _chunk(0)
        whole = _dev(rows_d, cen_d, cut_d, nbits)                          # 200 centroids: one split
        for chunk in (64, 48, 16):                                         # 4, 5 and 13 splits
            _chunk(chunk)
            got = _dev(rows_d, cen_d, cut_d, nbits)
            assert torch.equal(got[0], whole[0]) and torch.equal(got[1], whole[1]), chunk
    finally:
        _chunk(0)
    assert torch.equal(whole[0], want[0]) and torch.equal(whole[1], want[1])


# ---- 3. ties and specials -------------------------------------------------------------------------------------------------------
def test_ties_and_specials_on_the_device():
    D, nbits, Cn = 64, 4, 200
    cen, cut, rows = _tables(D, nbits, Cn, seed=2)
    # tiles of 16 centroids, tile t walked by wave t % 4; at compress_chunk 64 split s holds centroids 64 s .. 64 s + 63
    cen[67] = cen[3]                                 # the same wave's next tile
    cen[21] = cen[5]                                 # another wave's tile
    cen[135] = cen[7]                                # another split
    cen[150] = cen[149]                              # neighbours in one tile
    rows = rows[:16].clone()
    for r, c in enumerate((3, 5, 7, 149)):
        rows[r] = 4.0 * cen[c].float()
    rows[4] = 0.0                                    # the zero row: every score an exact 0
    rows[5, 9] = float("nan")                        # every score NaN
    rows[6] = 0.0
    rows[6, 11] = float("inf")                       # +-inf scores, NaN where the centroid holds a 0 there
    cen[:, 11] = torch.where(cen[:, 11] == 0, torch.tensor(0.01, dtype=torch.float16), cen[:, 11])
    cen[140, 11], cen[180, 11] = 0.0, 0.0
    want = _host(rows, cen, cut, nbits)
    assert want[0][:7].tolist() == [3, 5, 7, 149, 0, 0, 140]
    cen_d, cut_d, rows_d = cen.cuda(), cut.cuda(), rows.cuda()
    try:
        for chunk in (0, 64, 16):
            _chunk(chunk)
            got = _dev(rows_d, cen_d, cut_d, nbits)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), chunk
    finally:
        _chunk(0)
    # zero scores from +0 and -0 operands are equal: the lowest index wins.  (A chain that starts at +0 ends at -0 for no input —
    # (+0) + (-0) is +0 — so both scores are +0 here; that a -0 score would rank as +0 is rank_key's own property.)
    cen0 = torch.zeros(40, 16, dtype=torch.float16)
    cen0[:, 0] = -1.0
    cen0[17, 0], cen0[33, 0] = 0.0, -0.0
    rows0 = torch.zeros(3, 16)
    rows0[1, 0] = -0.0
    rows0[2, 0] = 1.0                                # scores -1 everywhere but +0 at 17 and -0 at 33: 17
    cut0 = torch.zeros(1)
    want0 = _host(rows0, cen0, cut0, 1)
    assert want0[0].tolist() == [0, 0, 17]
    got0 = _dev(rows0.cuda(), cen0.cuda(), cut0.cuda(), 1)
    assert torch.equal(got0[0], want0[0]) and torch.equal(got0[1], want0[1])


# ---- 4. the search's arithmetic -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [16, 128])
def test_codes_are_the_rank_maximum_of_li_scores(D):
    L, lib = _L()
    Cn, R, nbits = 200, 130, 2
    cen, cut, rows = _tables(D, nbits, Cn, seed=3)
    cen[190] = cen[2]
    rows[0] = 3.0 * cen[2].float()
    rows[1] = 0.0
    rows[2, 1] = float("nan")
    x = rows.half().float().cuda().contiguous()                            # the query columns: [1, R, D]
    ctx = cen.float().cuda().contiguous()                                  # one padded context of C rows
    ones = torch.ones(1, Cn, device="cuda")
    S = torch.full((1, Cn, R), -1.0, device="cuda")
    assert lib.rr_op_li_scores(L.ptr(x), L.ptr(ctx), L.ptr(ones), 1, 1, R, Cn, D, L.ptr(S), None, _st()) == L.RR_OK
    torch.cuda.synchronize()
    # np.argmax is the rank order's maximum: a NaN is the largest, the first occurrence of equal values (+0 == -0) wins
    want = np.argmax(S[0].cpu().numpy(), axis=0).astype(np.int32)
    assert want[0] == 2 and want[1] == 0 and want[2] == 0
    got = _dev(rows.cuda(), cen.cuda(), cut.cuda(), nbits)[0]
    assert np.array_equal(got.numpy(), want)


# ---- 5. the reference's own results ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,nbits", P.CASES)
def test_fixture_cases_on_the_device(dim, nbits):
    case = P.load_case(dim, nbits)
    cen, cut = torch.from_numpy(case["centroids"]).cuda(), torch.from_numpy(case["cutoffs"]).cuda()
    for rows in (torch.from_numpy(case["rows"]), torch.from_numpy(case["rows"]).float()):
        codes, res = _dev(rows.cuda(), cen, cut, nbits)
        assert np.array_equal(codes.numpy(), case["codes"]) and np.array_equal(res.numpy(), case["residuals"])


# ---- 6. through the bank ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture_codec(D, nbits):
    from rmr_amd import PlaidCodec
    case = P.load_case(D, nbits)
    return PlaidCodec(torch.from_numpy(case["centroids"]), torch.from_numpy(case["weights"]), nbits,
                      bucket_cutoffs=torch.from_numpy(case["cutoffs"]))


def _passages(codec, seed):
    """Two calls' padded tensors: ragged lengths, Lc padding behind the longest, interior mask zeros, a passage without a token."""
    gen = torch.Generator().manual_seed(seed)
    D, cen = codec.dim, codec.centroids.float()
    calls = []
    for Lc, lens in ((40, (33, 1, 17, 40 - 4)), (24, (24, 9, 1))):
        n = len(lens)
        pick = torch.randint(0, cen.shape[0], (n, Lc), generator=gen)
        x = torch.nn.functional.normalize(cen[pick] + 0.5 * torch.randn(n, Lc, D, generator=gen) / D ** 0.5, dim=-1)
        x[0, 2] = 0.0                                                    # a zero row inside a passage
        m = torch.zeros(n, Lc)
        for i, ln in enumerate(lens):
            m[i, :ln] = 1.0
        m[0, 3], m[0, 5], m[2, 0] = 0.0, 0.0, 2.5                         # interior zeros stay; any non-zero value is 1
        if Lc == 24:
            m[2] = 0.0                                                    # no unmasked token: length 1
        calls.append((x, m, list(lens)))
    return calls


@pytest.mark.parametrize("name,nbits", [("int_tiny", 8), ("int_tiny", 1), ("int_base", 8), ("int_base", 2)])      # li_dim 64 and 128
def test_add_compress_through_the_bank(name, nbits):
    from rmr_amd import PlaidSearch
    eng, _ = _engine(name)
    D = int(eng.arch["li_dim"])
    codec = _fixture_codec(D, nbits)
    calls = _passages(codec, seed=40 + nbits)
    total = sum(sum(lens) for _, _, lens in calls)
    n_all = sum(len(lens) for _, _, lens in calls)
    bank = eng.create_bank(total + 3, n_all + 1, codec=codec)
    twin = eng.create_bank(total + 3, n_all + 1, codec=codec)
    o = 0
    for k, (x, m, lens) in enumerate(calls):
        ids = [f"c{k}/{i}" for i in range(len(lens))]
        # the first call: host float32 tensors and derived lengths; the second: device fp16 tensors and the host's lengths
        first = bank.add_compress(ids, x, m) if k == 0 else bank.add_compress(ids, x.half().cuda(), m.cuda(), lengths=lens)
        assert first == o and bank.lookup(ids)[1].tolist() == lens
        o += len(ids)
        kept = torch.cat([x[i, :ln] for i, ln in enumerate(lens)])
        codes, res = codec.compress(kept)
        mask = torch.cat([(m[i, :ln] != 0).to(torch.uint8) for i, ln in enumerate(lens)])
        assert twin.add_compressed(ids, codes, res, lens, mask=mask) == first
        r0 = 0
        for i, ln in enumerate(lens):
            gc, gr, gm = bank.read_compressed(ids[i])
            assert torch.equal(gc, codes[r0:r0 + ln]) and torch.equal(gr, res[r0:r0 + ln]) and torch.equal(gm, mask[r0:r0 + ln]), ids[i]
            rows, rmask = bank.read(ids[i])
            assert torch.equal(rows.view(torch.int16), codec.decode(codes[r0:r0 + ln], res[r0:r0 + ln]).view(torch.int16))
            assert torch.equal(rmask, gm)
            r0 += ln
    assert bank.info() == twin.info() and bank.info()["rows_used"] == total and bank.padded_len == 40
    gen = torch.Generator().manual_seed(9)
    q = torch.nn.functional.normalize(torch.randn(2, 8, D, generator=gen), dim=-1).cuda()
    ids = list(bank.table.ids)
    a = bank.maxsim(eng, q, ids + ids, K=len(ids))
    b = twin.maxsim(eng, q, ids + ids, K=len(ids))
    assert torch.equal(a, b)
    ps = PlaidSearch(ncells=4, centroid_score_threshold=0.2, ndocs=32)
    (ia, sa), (ib, sb) = bank.search(eng, q, 4, plaid=ps), twin.search(eng, q, 4, plaid=ps)
    assert ia == ib and len(ia[0]) > 0 and torch.equal(sa, sb)
    (ia, sa), (ib, sb) = bank.search(eng, q, 5), twin.search(eng, q, 5)
    assert ia == ib and torch.equal(sa, sb)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_bank_unchanged():
    L, lib = _L()
    eng, _ = _engine("int_tiny")
    D = int(eng.arch["li_dim"])
    codec = _fixture_codec(D, 4)
    (x, m, lens), _ = _passages(codec, seed=5)
    bank = eng.create_bank(sum(lens) + 5, len(lens) + 2, codec=codec)
    ids = [f"p{i}" for i in range(len(lens))]
    bank.add_compress(ids, x, m, lengths=lens)
    before = [bank.read_compressed(i) for i in ids]
    info0 = bank.info()
    st = _st()
    y, ones = torch.randn(3, 8, D).cuda(), torch.ones(3, 8).cuda()

    def raw(b, li, dtype, ln, n=None, Lc=8):
        ln = np.ascontiguousarray(ln, dtype=np.int32)
        first = C.c_int32(-7)
        rc = lib.rr_bank_add_compress(b.h, li, dtype, ones.data_ptr(), ln.ctypes.data, len(ln) if n is None else n, Lc, C.byref(first), st)
        assert rc != 0 and first.value == -7
        return rc

    def unchanged():
        same = bank.info() == info0 and len(bank) == len(ids)
        for i, (c0, r0, m0) in zip(ids, before):
            c1, r1, m1 = bank.read_compressed(i)
            same = same and torch.equal(c0, c1) and torch.equal(r0, r1) and torch.equal(m0, m1)
        return same
    # an fp16 bank
    plain = eng.create_bank(16, 2)
    assert raw(plain, y.data_ptr(), L.RR_F32, [8]) == L.RR_ERR_UNSUPPORTED and b"rr_bank_add" in lib.rr_bank_last_error(plain.h)
    with pytest.raises(NotImplementedError):
        plain.add_compress(["x"], y[:1], ones[:1])
    with pytest.raises(NotImplementedError):
        plain.read_compressed("x")
    cut = np.zeros(15, dtype=np.float32)
    assert lib.rr_bank_set_plaid_cutoffs(plain.h, cut.ctypes.data) == L.RR_ERR_UNSUPPORTED
    assert plain.info() == dict(passages=0, rows_used=0, capacity_rows=16)
    # no cutoffs
    from rmr_amd import PlaidCodec
    bare = eng.create_bank(64, 2, codec=PlaidCodec(codec.centroids, codec.bucket_weights, 4))
    assert raw(bare, y.data_ptr(), L.RR_F32, [8]) == L.RR_ERR_UNSUPPORTED and b"cutoffs" in lib.rr_bank_last_error(bare.h)
    with pytest.raises(NotImplementedError):
        bare.add_compress(["x"], y[:1], ones[:1])
    assert bare.info()["passages"] == 0 and bare.info()["rows_used"] == 0
    # cutoffs that are no cutoffs; then the real ones, and the bank compresses
    cut[3] = np.nan
    assert lib.rr_bank_set_plaid_cutoffs(bare.h, cut.ctypes.data) == L.RR_ERR_BAD_SHAPE
    cut[3], cut[7] = 0.0, -1.0
    assert lib.rr_bank_set_plaid_cutoffs(bare.h, cut.ctypes.data) == L.RR_ERR_BAD_SHAPE
    assert raw(bare, y.data_ptr(), L.RR_F32, [8]) == L.RR_ERR_UNSUPPORTED
    assert lib.rr_bank_set_plaid_cutoffs(bare.h, codec.bucket_cutoffs.data_ptr()) == L.RR_OK
    assert bare.add_compress(["x"], x[:1], m[:1], lengths=lens[:1]) == 0
    got = bare.read_compressed("x")
    assert all(torch.equal(a, b) for a, b in zip(got, before[0]))
    # a length outside [1, Lc]
    assert raw(bank, y.data_ptr(), L.RR_F32, [8, 0]) == L.RR_ERR_BAD_SHAPE
    assert raw(bank, y.data_ptr(), L.RR_F32, [9]) == L.RR_ERR_BAD_SHAPE
    with pytest.raises(ValueError):
        bank.add_compress(["x", "y"], y[:2], ones[:2], lengths=[8, 0])
    assert unchanged()
    # rows (5 are free), then slots (2 are free)
    assert raw(bank, y.data_ptr(), L.RR_F32, [6]) == L.RR_ERR_OOM
    with pytest.raises(MemoryError):
        bank.add_compress(["x"], y[:1], ones[:1], lengths=[6])
    assert raw(bank, y.data_ptr(), L.RR_F32, [1, 1, 1]) == L.RR_ERR_OOM
    with pytest.raises(MemoryError):
        bank.add_compress(["x", "y", "z"], y, ones, lengths=[1, 1, 1])
    assert unchanged()
    # a misaligned pointer, a bad dtype, an id added twice
    assert raw(bank, y.data_ptr() + 4, L.RR_F32, [2]) == L.RR_ERR_BAD_ARG
    assert raw(bank, y.data_ptr(), L.RR_BF16, [2]) == L.RR_ERR_BAD_DTYPE
    with pytest.raises(ValueError):
        bank.add_compress(["p1"], y[:1], ones[:1], lengths=[2])
    assert unchanged() and "x" not in bank
    # rr_bank_add still refuses a compressed bank, and what fits is still taken
    with pytest.raises(NotImplementedError):
        bank.add(["x"], y[:1], ones[:1])
    assert bank.add_compress(["x"], y[:1], ones[:1], lengths=[5]) == len(ids)
    c, r, mk = bank.read_compressed("x")
    want = codec.compress(y[0, :5].cpu())
    assert torch.equal(c, want[0]) and torch.equal(r, want[1]) and mk.tolist() == [1] * 5


# ---- 8. what rr_bank_add and rr_bank_add_compress share: admission, the two staging slots, the append ---------------------------------
def _bank_pair(eng, cap_rows, slots):
    """An fp16 bank and an nbits = 2 bank of 32 centroids (li_dim 64) of the same capacity."""
    from rmr_amd import PlaidCodec
    cen, cut, _ = _tables(64, 2, 32)
    codec = PlaidCodec(cen, torch.tensor([-0.06, -0.02, 0.02, 0.06]), 2, bucket_cutoffs=cut)
    return codec, eng.create_bank(cap_rows, slots), eng.create_bank(cap_rows, slots, codec=codec)


def _holds(plain, bank, codec, pid, x, m, ln):
    """Passage `pid` is rows 0 .. ln - 1 of the padded x [Lc, D] / m [Lc] (host): `x.half()` and (m != 0) in the fp16 bank, the host
    definition's codes and bytes of the same rows in the compressed one."""
    want_mask = (m[:ln] != 0).to(torch.uint8)
    rows, mask = plain.read(pid)
    assert rows.shape == (ln, x.shape[1]) and torch.equal(rows.view(torch.int16), x[:ln].half().view(torch.int16)), pid
    assert torch.equal(mask, want_mask), pid
    codes, res = _host(x[:ln].contiguous(), codec.centroids, codec.bucket_cutoffs, codec.nbits)
    gc, gr, gm = bank.read_compressed(pid)
    assert torch.equal(gc, codes) and torch.equal(gr, res) and torch.equal(gm, want_mask), pid


def test_three_adds_back_to_back_reuse_a_staging_slot():
    """A bank stages its (first row, length) slots through two buffers taking turns: the third add is the first that overwrites one,
    and must wait for the first add's launch.  Device tensors and host lengths: nothing synchronises between the calls."""
    eng, _ = _engine("int_tiny")
    D, Lc = int(eng.arch["li_dim"]), 5
    assert D == 64
    calls = ([5, 2], [1, 4], [3, 3])
    total = sum(map(sum, calls))
    codec, plain, bank = _bank_pair(eng, total + 1, 2 * len(calls) + 1)
    gen = torch.Generator().manual_seed(61)
    host, dev = [], []
    for k, lens in enumerate(calls):
        x = torch.nn.functional.normalize(torch.randn(2, Lc, D, generator=gen), dim=-1)
        x = x.half() if k == 1 else x                                    # an fp16 source between two float32 ones
        m = (torch.arange(Lc)[None, :] < torch.tensor(lens)[:, None]).float()
        i = max(range(2), key=lambda j: lens[j])
        m[i, 1] = 0.0                                                    # one interior zero, in the longer passage
        host.append((x, m))
        dev.append((x.cuda(), m.cuda()))
    torch.cuda.synchronize()
    for b, add in ((plain, plain.add), (bank, bank.add_compress)):
        for k, lens in enumerate(calls):
            assert add([f"{k}/0", f"{k}/1"], *dev[k], lengths=lens) == 2 * k
        assert b.info()["passages"] == 2 * len(calls) and b.info()["rows_used"] == total and b.padded_len == Lc
    for k, lens in enumerate(calls):
        for i, ln in enumerate(lens):
            _holds(plain, bank, codec, f"{k}/{i}", host[k][0][i], host[k][1][i], ln)


def test_one_add_of_more_passages_than_a_staging_slot_starts_with():
    """1025 passages of one row: one descriptor more than the 1024 a staging slot starts with.  Two small adds first give both slots
    that size, so that the slot grows inside the call."""
    eng, _ = _engine("int_tiny")
    D, n = int(eng.arch["li_dim"]), 1025
    codec, plain, bank = _bank_pair(eng, n, n)
    gen = torch.Generator().manual_seed(62)
    x = torch.nn.functional.normalize(torch.randn(n, 1, D, generator=gen), dim=-1)
    m = torch.ones(n, 1)
    m[1023] = 0.0                                                        # no unmasked token: still one row, its mask byte 0
    xd, md = x.cuda(), m.cuda()
    ids = list(range(n))
    for b, add in ((plain, plain.add), (bank, bank.add_compress)):
        for warm in ("a", "b"):
            add([warm], xd[:1], md[:1], lengths=[1])
        b.clear()
        assert add(ids, xd, md, lengths=[1] * n) == 0
        assert b.info()["passages"] == n and b.info()["rows_used"] == n and len(b) == n
    for i in (0, 1023, 1024):
        _holds(plain, bank, codec, i, x[i], m[i], 1)
