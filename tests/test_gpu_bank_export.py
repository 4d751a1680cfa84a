"""GPU: a compressed bank written to disk as a PLAID index and read back, inverted file included: rr_bank_export_plaid /
rr_op_bank_export_plaid (the unmasked rows of a range of passages back to back, compacted on the device), PassageBank.save_plaid_index /
load_plaid_index(ivf=True), rr_bank_load_ivf (include/rerank_mi355.h).

1. Op level, rr_op_bank_export_plaid over loose pointers: outputs pre-filled with a poison value, the expectation is numpy boolean
   indexing over the inputs, bytes compared exactly, every case run twice with equal bytes.  Passage lengths 1, 2, 63, 64, 65, 127,
   128, 129, 200 (both sides of one and of two 64-row steps) each under every mask shape that fits it, at 1, 4, 16, 128 and 512
   residual bytes per row (one lane per row below 16; 16-byte units above, 1, 8 and 32 per row), from table entry 0 and 3, over a
   table that lies in row order and over one whose passages lie out of order with gaps; capacity exactly R, more than R (poison
   behind R stays) and R - 1 (refused, nothing written); and three passages around byte 2^32 of a residual array of 2^32 + 2^20
   bytes (64-bit source offsets).
2. Bank level: 300 passages of 1 .. 180 rows with interior masked rows saved in 5 chunks and loaded into a second bank: the stored
   rows, the whole-bank export, the exact and the pruned search, the written and the loaded inverted file, all equal byte for byte.
3. Refusals of the export, of the save and of rr_bank_load_ivf (the previous file kept).
Exact equality everywhere; no tolerance."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from test_gpu_li_scores import _engine as _bare_engine

pytestmark = pytest.mark.gpu

BPOISON, IPOISON = 0xA5, -123456789
LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 200)


def _masks(ln, gen):
    """Every mask shape a passage of ln rows can take: (name, uint8 [ln])."""
    z, o = np.zeros(ln, dtype=np.uint8), np.ones(ln, dtype=np.uint8)

    def single(r):
        m = z.copy()
        m[r] = 1
        return m
    out = [("ones", o), ("zero", z), ("row0", single(0)), ("last", single(ln - 1)), ("alternating", (np.arange(ln) % 2 == 0).astype(np.uint8)),
           ("random", (torch.rand(ln, generator=gen) < 0.5).numpy().astype(np.uint8))]
    if ln >= 64:
        out.append(("row63", single(63)))
    if ln >= 65:
        out.append(("row64", single(64)))
    if ln >= 129:
        m = o.copy()
        m[64:128] = 0                                            # a zero run of exactly one whole step between kept rows
        out.append(("zero_step", m))
    return out


def _slots(first_rows, lens):
    a = np.zeros(len(lens), dtype=np.dtype([("first", "<i8"), ("len", "<i4"), ("unused", "<i4")]))
    a["first"], a["len"] = first_rows, lens
    return torch.from_numpy(a.view(np.uint8).copy()).cuda()


_OP = {}


def _op_case(rb, scattered):
    """The passages of LENGTHS x _masks in one table; scattered: the passages lie in a shuffled order with gaps of 0 .. 70 rows between
    them (and rows in front of the first), the gaps holding unmasked garbage that must not travel."""
    if (rb, scattered) not in _OP:
        gen = torch.Generator().manual_seed(1000 * rb + scattered)
        lens, masks = [], []
        for ln in LENGTHS:
            for _, m in _masks(ln, gen):
                lens.append(ln)
                masks.append(m)
        n = len(lens)
        if scattered:
            order = torch.randperm(n, generator=gen).tolist()
            gaps = torch.randint(0, 71, (n,), generator=gen).tolist()
            first = [0] * n
            row = 5
            for p in order:
                first[p] = row
                row += lens[p] + gaps[p]
            total = row + 3
        else:
            first = np.concatenate([[0], np.cumsum(lens)[:-1]]).tolist()
            total = sum(lens)
        codes = torch.randint(0, 1 << 20, (total,), generator=gen, dtype=torch.int32).numpy()
        res = torch.randint(0, 256, (total, rb), generator=gen, dtype=torch.uint8).numpy()
        mask = np.ones(total, dtype=np.uint8)
        for f, ln, m in zip(first, lens, masks):
            mask[f:f + ln] = m
        _OP[(rb, scattered)] = dict(first=first, lens=lens, codes=codes, res=res, mask=mask, table=_slots(first, lens),
                                    d_codes=torch.from_numpy(codes).cuda(), d_res=torch.from_numpy(res).cuda(), d_mask=torch.from_numpy(mask).cuda())
    return _OP[(rb, scattered)]


def _expect(c, first_passage, n):
    keep = [np.arange(f, f + ln)[c["mask"][f:f + ln] != 0] for f, ln in zip(c["first"][first_passage:first_passage + n], c["lens"][first_passage:first_passage + n])]
    rows = np.concatenate(keep)
    doclens = np.array([len(k) for k in keep], dtype=np.int32)
    return doclens, np.concatenate([[0], np.cumsum(doclens)]).astype(np.int64), c["codes"][rows], c["res"][rows]


def _op(c, rb, first_passage, n, capacity, rows_allocated, sizing=False, offsets=True):
    """One rr_op_bank_export_plaid call on poisoned outputs: (rc, doclens, offsets, codes, residuals) as numpy."""
    from rmr_amd import _lib as L
    lib = L.load()
    dl = torch.full((n + 2,), IPOISON, device="cuda", dtype=torch.int32)
    of = torch.full((n + 3,), IPOISON, device="cuda", dtype=torch.int64)
    co = torch.full((rows_allocated,), IPOISON, device="cuda", dtype=torch.int32)
    ro = torch.full((rows_allocated, rb), BPOISON, device="cuda", dtype=torch.uint8)
    rc = lib.rr_op_bank_export_plaid(L.ptr(c["table"]), first_passage, n, L.ptr(c["d_mask"]), L.ptr(c["d_codes"]), L.ptr(c["d_res"]), rb, L.ptr(dl),
                                     L.ptr(of) if offsets else None, None if sizing else L.ptr(co), None if sizing else L.ptr(ro), capacity,
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, dl.cpu().numpy(), of.cpu().numpy(), co.cpu().numpy(), ro.cpu().numpy()


@pytest.mark.parametrize("first_passage", [0, 3])
@pytest.mark.parametrize("scattered", [0, 1])
@pytest.mark.parametrize("rb", [1, 4, 16, 128, 512])
def test_op_export_equals_boolean_indexing(rb, scattered, first_passage):
    c = _op_case(rb, scattered)
    n = len(c["lens"]) - first_passage
    doclens, offsets, codes, res = _expect(c, first_passage, n)
    R = int(offsets[-1])
    assert 0 in doclens.tolist() and n > 60 and R > 1500, "the fixture holds passages of doclen 0 and more than one block of waves"
    runs = []
    for capacity, allocated in ((R, R + 7), (R + 5, R + 7)):      # exactly R; more than R: the rows behind R keep the poison
        for _ in range(2):
            rc, dl, of, co, ro = _op(c, rb, first_passage, n, capacity, allocated)
            assert rc == 0
            assert np.array_equal(dl[:n], doclens) and (dl[n:] == IPOISON).all(), "doclens"
            assert np.array_equal(of[:n + 1], offsets) and (of[n + 1:] == IPOISON).all(), "offsets"
            bad = np.flatnonzero(co[:R] != codes)
            assert bad.size == 0, f"codes differ at rows {bad[:5].tolist()}"
            bad = np.flatnonzero((ro[:R] != res).any(axis=1))
            assert bad.size == 0, f"residual bytes differ at rows {bad[:5].tolist()}"
            assert (co[R:] == IPOISON).all() and (ro[R:] == BPOISON).all(), "nothing is written behind R"
            runs.append((dl.tobytes(), of.tobytes(), co.tobytes(), ro.tobytes()))
    assert runs[0] == runs[1] and runs[2] == runs[3], "two runs give equal bytes"


@pytest.mark.parametrize("rb", [4, 128])
def test_op_sizing_call_and_short_capacity(rb):
    from rmr_amd import _lib as L
    c = _op_case(rb, 1)
    n = len(c["lens"])
    doclens, offsets, _, _ = _expect(c, 0, n)
    R = int(offsets[-1])
    rc, dl, of, co, ro = _op(c, rb, 0, n, 0, 4, sizing=True)
    assert rc == 0 and np.array_equal(dl[:n], doclens) and np.array_equal(of[:n + 1], offsets)
    assert (co == IPOISON).all() and (ro == BPOISON).all()
    rc, dl, of, co, ro = _op(c, rb, 0, n, 0, 4, sizing=True, offsets=False)
    assert rc == 0 and np.array_equal(dl[:n], doclens) and (of == IPOISON).all()
    rc, dl, of, co, ro = _op(c, rb, 0, n, R - 1, R + 7)
    assert rc == L.RR_ERR_BAD_SHAPE
    assert (dl == IPOISON).all() and (of == IPOISON).all() and (co == IPOISON).all() and (ro == BPOISON).all(), "a refused call writes nothing"
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    dl_d = torch.zeros(n, device="cuda", dtype=torch.int32)
    co_d = torch.zeros(R, device="cuda", dtype=torch.int32)
    ro_d = torch.zeros((R, rb), device="cuda", dtype=torch.uint8)
    args = (L.ptr(c["table"]), 0, n, L.ptr(c["d_mask"]), L.ptr(c["d_codes"]), L.ptr(c["d_res"]))
    assert lib.rr_op_bank_export_plaid(*args, rb, L.ptr(dl_d), None, L.ptr(co_d), None, R, st) == L.RR_ERR_BAD_ARG       # one of the two
    assert lib.rr_op_bank_export_plaid(*args, rb, L.ptr(dl_d), None, None, L.ptr(ro_d), R, st) == L.RR_ERR_BAD_ARG
    assert lib.rr_op_bank_export_plaid(*args, 3, L.ptr(dl_d), None, L.ptr(co_d), L.ptr(ro_d), R, st) == L.RR_ERR_UNSUPPORTED
    assert lib.rr_op_bank_export_plaid(*args, 1024, L.ptr(dl_d), None, L.ptr(co_d), L.ptr(ro_d), R, st) == L.RR_ERR_UNSUPPORTED
    assert lib.rr_op_bank_export_plaid(*args[:2], 0, *args[3:], rb, L.ptr(dl_d), None, L.ptr(co_d), L.ptr(ro_d), R, st) == L.RR_ERR_BAD_SHAPE
    torch.cuda.synchronize()
    assert not co_d.any() and not ro_d.any() and not dl_d.any()


def test_op_source_offsets_are_64_bit():
    """Three passages whose rows lie just before, across and just after byte 2^32 of an uninitialised residual array of 2^32 + 2^20
    bytes at 512 bytes per row: row 2^23 starts at byte 2^32."""
    rb, edge = 512, 1 << 23
    total = edge + (1 << 20) // rb
    gen = torch.Generator().manual_seed(4)
    res = torch.empty((total, rb), device="cuda", dtype=torch.uint8)
    assert res.numel() == (1 << 32) + (1 << 20)
    codes = torch.empty(total, device="cuda", dtype=torch.int32)
    mask = torch.zeros(total, device="cuda", dtype=torch.uint8)
    first, lens = [edge - 70, edge - 3, edge + 8], [64, 10, 70]
    want_codes, want_res, doclens = [], [], []
    for f, ln in zip(first, lens):
        r = torch.randint(0, 256, (ln, rb), generator=gen, dtype=torch.uint8)
        cd = torch.randint(0, 1 << 20, (ln,), generator=gen, dtype=torch.int32)
        m = (torch.rand(ln, generator=gen) < 0.7).to(torch.uint8)
        m[0] = m[-1] = 1
        res[f:f + ln] = r.cuda()
        codes[f:f + ln] = cd.cuda()
        mask[f:f + ln] = m.cuda()
        want_codes.append(cd[m != 0])
        want_res.append(r[m != 0])
        doclens.append(int(m.sum()))
    c = dict(table=_slots(first, lens), d_mask=mask, d_codes=codes, d_res=res)
    R = sum(doclens)
    runs = []
    for _ in range(2):
        rc, dl, of, co, ro = _op(c, rb, 0, 3, R, R + 2)
        assert rc == 0 and dl[:3].tolist() == doclens and of[3] == R
        assert np.array_equal(co[:R], torch.cat(want_codes).numpy()) and np.array_equal(ro[:R], torch.cat(want_res).numpy())
        assert (co[R:] == IPOISON).all() and (ro[R:] == BPOISON).all()
        runs.append((co.tobytes(), ro.tobytes()))
    assert runs[0] == runs[1]


# ---- 2. bank level -------------------------------------------------------------------------------------------------------------------
D, NBITS, C, P = 64, 8, 64, 300
_BANK = {}


def _codec():
    from rmr_amd import PlaidCodec
    gen = torch.Generator().manual_seed(77)
    cen = torch.nn.functional.normalize(torch.randn(C, D, generator=gen), dim=-1)
    cut = torch.linspace(-0.3, 0.3, (1 << NBITS) - 1)
    w = torch.linspace(-0.31, 0.31, 1 << NBITS)
    return PlaidCodec(cen, w, NBITS, bucket_cutoffs=cut)


def _queries(codec, nq, Lq, seed):
    gen = torch.Generator().manual_seed(seed)
    qs = []
    for _ in range(nq):
        pick = torch.randperm(C, generator=gen)[:5][torch.randint(0, 5, (Lq,), generator=gen)]
        qs.append(torch.nn.functional.normalize(codec.centroids[pick].float() + 0.9 * torch.randn(Lq, D, generator=gen) / D ** 0.5, dim=-1))
    return torch.stack(qs).cuda()


def _bank():
    """300 passages of U[1, 180] rows, each drawn from four centroids, with random interior masked rows and at least one unmasked."""
    if not _BANK:
        eng, codec = _bare_engine(D), _codec()
        gen = torch.Generator().manual_seed(300)
        lens = torch.randint(1, 181, (P,), generator=gen).tolist()
        codes, masks = [], []
        for ln in lens:
            t = torch.randperm(C, generator=gen)[:4]
            codes.append(t[torch.randint(0, 4, (ln,), generator=gen)])
            m = (torch.rand(ln, generator=gen) < 0.8).to(torch.uint8)
            m[int(torch.randint(0, ln, (1,), generator=gen))] = 1
            masks.append(m)
        codes, mask = torch.cat(codes).to(torch.int32), torch.cat(masks)
        res = torch.randint(0, 256, (len(codes), codec.residual_bytes), generator=gen, dtype=torch.uint8)
        bank = eng.create_bank(sum(lens) + 4, P + 1, codec=codec)
        ids = [f"p{i}" for i in range(P)]
        bank.add_compressed(ids, codes, res, lens, mask=mask)
        _BANK.update(eng=eng, codec=codec, bank=bank, ids=ids, lens=lens, codes=codes, res=res, mask=mask)
    return _BANK


def _saved(tmp_path_factory):
    """The bank saved once (5 chunks) and loaded into a second bank with its inverted file."""
    from rmr_amd import read_plaid_index
    b = _bank()
    if "dir" not in b:
        d = str(tmp_path_factory.mktemp("plaid_index"))
        b["meta"] = b["bank"].save_plaid_index(d, chunk_passages=64, config={"query_maxlen": 32})
        codec2, _ = read_plaid_index(d)
        bank2 = b["eng"].create_bank(int(b["mask"].sum()) + 4, P + 1, codec=codec2)
        assert bank2.load_plaid_index(d, ivf=True) == P
        b.update(dir=d, bank2=bank2)
    return b


def test_save_writes_five_chunks_and_the_loaded_bank_holds_the_unmasked_rows(tmp_path_factory):
    b = _saved(tmp_path_factory)
    bank, bank2, d, mask = b["bank"], b["bank2"], b["dir"], b["mask"]
    files = set(os.listdir(d))
    assert {f"{i}.codes.pt" for i in range(5)} <= files and "5.codes.pt" not in files
    assert {"metadata.json", "ivf.pid.pt", "passage_ids.json", "centroids.pt", "buckets.pt", "avg_residual.pt"} <= files and "plan.json" not in files
    with open(os.path.join(d, "doclens.4.json")) as f:
        assert len(json.load(f)) == P - 4 * 64, "the last chunk is partial"
    assert b["meta"]["num_chunks"] == 5 and b["meta"]["num_embeddings"] == int(mask.sum()) and b["meta"]["num_partitions"] == C
    assert b["meta"]["config"] == {"dim": D, "nbits": NBITS, "query_maxlen": 32}
    assert bank2.table.ids == b["ids"], "the ids come from passage_ids.json"
    assert bank2.info()["rows_used"] == int(mask.sum())
    all_codes, all_res, row = [], [], 0
    for pid, ln in zip(b["ids"], b["lens"]):
        c0, r0, m0 = bank.read_compressed(pid)
        assert torch.equal(c0, b["codes"][row:row + ln]) and torch.equal(r0, b["res"][row:row + ln]) and torch.equal(m0, mask[row:row + ln])
        c1, r1, m1 = bank2.read_compressed(pid)
        keep = m0 != 0
        assert torch.equal(c1, c0[keep]) and torch.equal(r1, r0[keep]) and bool(m1.all()), pid
        all_codes.append(c0[keep])
        all_res.append(r0[keep])
        row += ln
    for bk in (bank, bank2):
        codes, res, doclens = bk.export_compressed()
        assert codes.is_cuda and res.is_cuda and codes.dtype == torch.int32 and res.dtype == torch.uint8
        assert doclens == [int(x.numel()) for x in all_codes]
        assert torch.equal(codes.cpu(), torch.cat(all_codes)) and torch.equal(res.cpu(), torch.cat(all_res))
    codes, res, doclens = b["eng"].bank_export_plaid(bank, 37, 100)
    assert doclens == [int(x.numel()) for x in all_codes[37:137]]
    assert torch.equal(codes.cpu(), torch.cat(all_codes[37:137])) and torch.equal(res.cpu(), torch.cat(all_res[37:137]))


def test_both_banks_search_alike(tmp_path_factory):
    from rmr_amd import PlaidSearch
    b = _saved(tmp_path_factory)
    eng, bank, bank2 = b["eng"], b["bank"], b["bank2"]
    q = _queries(b["codec"], 3, 16, seed=5)
    a, c = eng.bank_search(bank, q, 10), eng.bank_search(bank2, q, 10)
    torch.cuda.synchronize()
    assert torch.equal(a["indices"], c["indices"]) and torch.equal(a["scores"].view(torch.int32), c["scores"].view(torch.int32))
    kw = dict(ncells=2, centroid_score_threshold=0.3, ndocs=64)
    a, c = eng.bank_search_plaid(bank, q, 10, **kw), eng.bank_search_plaid(bank2, q, 10, **kw)
    torch.cuda.synchronize()
    assert int(a["counts"].min()) >= 1, "the queries find candidates"
    for name in ("indices", "scores", "counts"):
        assert torch.equal(a[name].view(torch.int32), c[name].view(torch.int32)), name
    scan, ivf = PlaidSearch(2, 0.3, 64), PlaidSearch(2, 0.3, 64, ivf=True)
    want_ids, want_scores = bank.search(eng, q, 10, plaid=scan)
    for bk in (bank, bank2):                                      # bank: the file save_plaid_index built; bank2: the file it loaded
        got_ids, got_scores = bk.search(eng, q, 10, plaid=ivf)
        assert got_ids == want_ids and torch.equal(got_scores.view(torch.int32), want_scores.view(torch.int32))


def test_the_written_and_the_loaded_inverted_file_equal_a_build(tmp_path_factory):
    b = _saved(tmp_path_factory)
    eng, bank, bank2, d = b["eng"], b["bank"], b["bank2"], b["dir"]
    pids, lengths = bank.ivf()
    on_disk = torch.load(os.path.join(d, "ivf.pid.pt"), map_location="cpu", weights_only=True)
    assert on_disk[0].dtype == torch.int32 and on_disk[1].dtype == torch.int64
    assert torch.equal(on_disk[0], pids) and torch.equal(on_disk[1], lengths)
    loaded_info, loaded = bank2.ivf_info(), bank2.ivf()
    assert loaded_info == bank.ivf_info() and loaded_info["passages_covered"] == P
    built_info = bank2.build_ivf()
    built = bank2.ivf()
    assert built_info == loaded_info
    for got in (loaded, built):
        assert torch.equal(got[0], pids) and torch.equal(got[1], lengths)
    assert eng.bank_load_ivf(bank2, (pids, lengths)) == loaded_info                # the pair itself
    assert bank2.load_ivf(os.path.join(d, "ivf.pid.pt"), verify=False) == loaded_info  # the file; unverified
    assert torch.equal(bank2.ivf()[0], pids)


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------
def _small_bank(eng, codec, fully_masked=None, n=6):
    gen = torch.Generator().manual_seed(8)
    lens = [3, 70, 1, 9, 64, 5][:n]
    R = sum(lens)
    codes = torch.randint(0, C, (R,), generator=gen, dtype=torch.int32)
    res = torch.randint(0, 256, (R, codec.residual_bytes), generator=gen, dtype=torch.uint8)
    mask = torch.ones(R, dtype=torch.uint8)
    mask[4] = 0
    if fully_masked is not None:
        f = sum(lens[:fully_masked])
        mask[f:f + lens[fully_masked]] = 0
    bank = eng.create_bank(R + 4, n + 1, codec=codec)
    bank.add_compressed([f"s{i}" for i in range(n)], codes, res, lens, mask=mask)
    return bank, int(mask.sum())


def test_save_and_export_refusals(tmp_path):
    from rmr_amd import PlaidCodec
    from rmr_amd import _lib as L
    eng, codec = _bare_engine(D), _codec()
    bank, _ = _small_bank(eng, codec, fully_masked=3)
    d = str(tmp_path / "masked")
    with pytest.raises(ValueError, match=r"no unmasked row.*'s3'"):
        bank.save_plaid_index(d, chunk_passages=4)
    assert not os.path.exists(d) or not os.listdir(d), "nothing is written"
    assert bank.export_compressed()[2][3] == 0, "the export itself reports the doclen 0"
    plain = eng.create_bank(64, 4)
    plain.add(["a", "b"], torch.nn.functional.normalize(torch.randn(2, 8, D), dim=-1), torch.ones(2, 8), lengths=[8, 3])
    with pytest.raises(NotImplementedError):
        plain.save_plaid_index(str(tmp_path / "fp16"))
    with pytest.raises(NotImplementedError):
        plain.export_compressed()
    assert not os.path.exists(str(tmp_path / "fp16"))
    no_cut = PlaidCodec(codec.centroids, codec.bucket_weights, NBITS)
    bare, _ = _small_bank(eng, no_cut)
    with pytest.raises(ValueError, match="bucket_cutoffs"):
        bare.save_plaid_index(str(tmp_path / "no_cutoffs"))
    assert not os.path.exists(str(tmp_path / "no_cutoffs"))
    # the C entry
    bank, R = _small_bank(eng, codec)
    n, rb, st = len(bank), codec.residual_bytes, torch.cuda.current_stream().cuda_stream
    dl = np.full(n + 1, IPOISON, dtype=np.int32)
    rows = ctypes.c_int64(IPOISON)
    co = torch.full((R + 3,), IPOISON, device="cuda", dtype=torch.int32)
    ro = torch.full((R + 3, rb), BPOISON, device="cuda", dtype=torch.uint8)

    def call(b, first, cnt, codes_out, res_out, cap):
        return b.lib.rr_bank_export_plaid(b.h, first, cnt, dl.ctypes.data, codes_out, res_out, cap, ctypes.byref(rows), st)
    assert call(bank, 0, n, co.data_ptr(), None, R) == L.RR_ERR_BAD_ARG
    assert call(bank, 0, n, None, ro.data_ptr(), R) == L.RR_ERR_BAD_ARG
    assert call(plain, 0, 2, co.data_ptr(), ro.data_ptr(), R) == L.RR_ERR_UNSUPPORTED
    for first, cnt in ((0, 0), (0, n + 1), (-1, 2), (n, 1), (2, n - 1)):
        assert call(bank, first, cnt, co.data_ptr(), ro.data_ptr(), R) == L.RR_ERR_BAD_SHAPE, (first, cnt)
    assert call(bank, 0, n, co.data_ptr(), ro.data_ptr(), R - 1) == L.RR_ERR_BAD_SHAPE
    assert str(R).encode() in bank.lib.rr_bank_last_error(bank.h), "the message names R"
    torch.cuda.synchronize()
    assert (dl == IPOISON).all() and rows.value == IPOISON and (co == IPOISON).all() and (ro == BPOISON).all(), "a refused call writes nothing"
    assert call(bank, 0, n, None, None, 0) == 0 and rows.value == R and dl[n] == IPOISON and int(dl[:n].sum()) == R      # the sizing call
    assert (co == IPOISON).all() and (ro == BPOISON).all()
    assert call(bank, 0, n, co.data_ptr(), ro.data_ptr(), R) == 0 and rows.value == R
    torch.cuda.synchronize()
    assert (co[:R] != IPOISON).all() and (co[R:] == IPOISON).all() and (ro[R:] == BPOISON).all()
    # under stream capture
    probe = torch.zeros(1, device="cuda")
    co.fill_(IPOISON)
    off = np.zeros(C + 1, dtype=np.int64)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            probe.add_(1.0)
            cs = torch.cuda.current_stream().cuda_stream
            rc = bank.lib.rr_bank_export_plaid(bank.h, 0, n, dl.ctypes.data, co.data_ptr(), ro.data_ptr(), R, ctypes.byref(rows), cs)
            msg = bank.lib.rr_bank_last_error(bank.h)
            rc_load = bank.lib.rr_bank_load_ivf(bank.h, off.ctypes.data, None, 0, cs)
            msg_load = bank.lib.rr_bank_last_error(bank.h)
        graph.replay()
        torch.cuda.synchronize()
    assert rc == L.RR_ERR_BAD_ARG and b"captured" in msg and rc_load == L.RR_ERR_BAD_ARG and b"captured" in msg_load
    assert probe.item() == 1.0 and (co == IPOISON).all() and bank.ivf_info()["passages_covered"] == 0


def test_load_ivf_refusals_keep_the_previous_file():
    from rmr_amd import _lib as L
    eng, codec = _bare_engine(D), _codec()
    bank, _ = _small_bank(eng, codec)
    n = len(bank)
    info = bank.build_ivf()
    pids, lengths = bank.ivf()
    offsets = np.concatenate([[0], np.cumsum(lengths.numpy())]).astype(np.int64)
    good = pids.numpy().copy()
    st = torch.cuda.current_stream().cuda_stream

    def raw(off, pid, verify=1):
        off, pid = np.ascontiguousarray(off, dtype=np.int64), np.ascontiguousarray(pid, dtype=np.int32)
        return bank.lib.rr_bank_load_ivf(bank.h, off.ctypes.data, pid.ctypes.data, verify, st), bank.lib.rr_bank_last_error(bank.h)

    def unchanged():
        got = bank.ivf()
        return bank.ivf_info() == info and torch.equal(got[0], pids) and torch.equal(got[1], lengths)
    two = int(np.flatnonzero(np.diff(offsets) >= 2)[0])                 # a list of two entries or more
    i = int(offsets[two])
    for name, off, pid, word in (("a descending pair", offsets, np.concatenate([good[:i], good[i:i + 2][::-1], good[i + 2:]]), b"ascend"),
                                 ("a duplicate", offsets, np.concatenate([good[:i + 1], good[i:i + 1], good[i + 2:]]), b"ascend"),
                                 ("a pid equal to the passage count", offsets, np.concatenate([good[:i + 1], [n], good[i + 2:]]), b"names passage"),
                                 ("offsets[0] = 1", np.concatenate([[1], offsets[1:]]), good, b"offsets[0]"),
                                 ("a decreasing offset", np.concatenate([offsets[:two + 1], [offsets[two] - 1], offsets[two + 2:]]), good, b"decrease")):
        for verify in (1, 0):
            rc, msg = raw(off, pid, verify)
            assert rc == L.RR_ERR_BAD_SHAPE and word in msg, (name, verify, rc, msg)
            assert unchanged(), name
    assert f"list {two}".encode() in raw(offsets, np.concatenate([good[:i + 1], good[i:i + 1], good[i + 2:]]))[1], "the offending list is named"
    # one pid replaced by another valid one: a well-formed file of another index
    single = [c for c in range(C) if lengths[c] == 1 and int(good[offsets[c]]) != (int(good[offsets[c]]) + 1) % n]
    other = good.copy()
    other[offsets[single[0]]] = (other[offsets[single[0]]] + 1) % n
    rc, msg = raw(offsets, other, 1)
    assert rc == L.RR_ERR_BAD_SHAPE and b"another index" in msg and unchanged()
    with pytest.raises(ValueError, match="another index"):
        bank.load_ivf((torch.from_numpy(other), lengths))
    assert unchanged()
    assert bank.load_ivf((torch.from_numpy(other), lengths), verify=False)["postings"] == info["postings"]
    assert torch.equal(bank.ivf()[0], torch.from_numpy(other)), "verify=False trusts the caller"
    assert bank.load_ivf((pids, lengths)) == info and unchanged()
    # the Python side's own refusals, an fp16 bank and an empty bank
    with pytest.raises(ValueError):
        bank.load_ivf((pids, lengths[:-1]))
    with pytest.raises(ValueError):
        bank.load_ivf((pids[:-1], lengths))
    assert unchanged()
    plain = eng.create_bank(64, 4)
    plain.add(["a"], torch.nn.functional.normalize(torch.randn(1, 8, D), dim=-1), torch.ones(1, 8), lengths=[8])
    with pytest.raises(NotImplementedError):
        plain.load_ivf((pids, lengths))
    assert plain.lib.rr_bank_load_ivf(plain.h, offsets.ctypes.data, good.ctypes.data, 1, st) == L.RR_ERR_UNSUPPORTED
    empty = eng.create_bank(64, 4, codec=codec)
    assert empty.lib.rr_bank_load_ivf(empty.h, offsets.ctypes.data, good.ctypes.data, 1, st) == L.RR_ERR_BAD_SHAPE
    # passages added after a load are not covered, as after a build
    bank.add_compressed(["late"], torch.zeros(2, dtype=torch.int32), torch.zeros((2, codec.residual_bytes), dtype=torch.uint8), [2])
    assert bank.ivf_info()["passages_covered"] == n
    rc, msg = raw(offsets, good, 1)
    assert rc == L.RR_ERR_BAD_SHAPE and b"another index" in msg, "the file no longer covers the bank"
