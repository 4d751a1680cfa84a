"""GPU: the compressed (PLAID residual) passage bank — rr_bank_create_plaid / rr_bank_add_plaid / rr_bank_format,
rr_op_plaid_decode_rows, and rr_bank_read / rr_forward_interaction_bank on a compressed bank, through PassageBank.add_compressed,
RerankEngine.forward_interaction_bank and rerank_dataset_pipelined.

Contract (include/rerank_mi355.h, rr_bank_create_plaid): the device decodes a row to exactly the fp16 bits of the host decoder
rr_util_plaid_decode_rows, and a compressed bank is bit for bit an fp16 bank that holds the decoded rows — on fp16 and bf16
handles and in the float32 copies of the attention fusion.  Every equality below is torch.equal; no tolerance anywhere
("resid_split" = 0 as in tests/test_gpu_passage_bank.py, whose engines this module shares)."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_packed_families import _int_args
from test_gpu_passage_bank import _engine, _model

pytestmark = pytest.mark.gpu

N_CENTROIDS = 16


def _codec(D, nbits, seed=0):
    """Random tables: unit centroids with row 0 all zero, weights of residual size with an exact 0 for bucket 0."""
    from rmr_amd import PlaidCodec
    gen = torch.Generator().manual_seed(100 * D + 10 * nbits + seed)
    cen = torch.nn.functional.normalize(torch.randn(N_CENTROIDS, D, generator=gen), dim=-1)
    cen[0] = 0.0
    w = torch.randn(1 << nbits, generator=gen) * (0.5 / D ** 0.5)
    w[0] = 0.0
    return PlaidCodec(cen, w, nbits)


def _rows(codec, n, seed):
    """n random rows (codes int32, residual bytes uint8); row 0 is the zero-norm row (zero centroid, every bucket 0)."""
    gen = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, N_CENTROIDS, (n,), generator=gen, dtype=torch.int32)
    res = torch.randint(0, 256, (n, codec.residual_bytes), generator=gen, dtype=torch.uint8)
    codes[0], res[0] = 0, 0
    return codes, res


def _fill(eng, codec, lens_a, lens_b, seed=3, spare_rows=0, spare_slots=0):
    """A compressed bank filled by two add_compressed calls, passages "p0", "p1", ...; the first call's mask has interior zeros,
    the second is all ones (None).  Returns (bank, codes, residuals, mask, lengths) over all rows."""
    lens = list(lens_a) + list(lens_b)
    codes, res = _rows(codec, sum(lens), seed)
    bank = eng.create_bank(sum(lens) + spare_rows, len(lens) + spare_slots, codec=codec)
    ra = sum(lens_a)
    mask = torch.ones(sum(lens), dtype=torch.uint8)
    mask[torch.arange(2, ra, 3)] = 0
    assert bank.add_compressed([f"p{i}" for i in range(len(lens_a))], codes[:ra], res[:ra], lens_a, mask=mask[:ra]) == 0
    assert bank.add_compressed([f"p{i}" for i in range(len(lens_a), len(lens))], codes[ra:].numpy(), res[ra:].numpy(), lens_b) == len(lens_a)
    return bank, codes, res, mask, lens


def _fp16_twin(eng, bank, lens, Lc):
    """An fp16 bank under the same ids filled with read()'s rows and masks."""
    D = bank.li_dim
    li = torch.zeros(len(lens), Lc, D, dtype=torch.float16)
    cm = torch.zeros(len(lens), Lc)
    for i, ln in enumerate(lens):
        rows, mask = bank.read(f"p{i}")
        li[i, :ln], cm[i, :ln] = rows, mask.float()
    twin = eng.create_bank(sum(lens) + 1, len(lens) + 1)
    twin.add([f"p{i}" for i in range(len(lens))], li, cm, lengths=lens)
    assert twin.padded_len == Lc
    return twin


def _equal(a, b, keys):
    for k in keys:
        assert a[k] is not None and b[k] is not None and torch.equal(a[k], b[k]), \
            f"{k} differs: {(a[k].float() - b[k].float()).abs().max().item():.3e}"


# ---- 1. decode ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["int_tiny", "int_base"])             # li_dim 64 (8 rows per wave) and 128 (4 rows per wave)
@pytest.mark.parametrize("nbits", [1, 2, 4, 8])
def test_read_equals_the_host_decoder_bit_for_bit(name, nbits):
    eng, g = _engine(name)
    D, Lc = int(eng.arch["li_dim"]), int(g["Lc"])
    codec = _codec(D, nbits)
    bank, codes, res, mask, lens = _fill(eng, codec, [1, 7, 33], [Lc, 33, 7, 1])
    info = bank.info()
    assert info == dict(passages=7, rows_used=sum(lens), capacity_rows=sum(lens), nbits=nbits, bytes_per_row=4 + D * nbits // 8 + 1)
    assert bank.padded_len == Lc and bank.lookup([f"p{i}" for i in range(7)])[1].tolist() == lens
    want = codec.decode(codes, res)                                     # rr_util_plaid_decode_rows, host code
    assert not bool(want[0].view(torch.int16).any()), "row 0 has norm zero"
    assert bool(torch.isfinite(want.float()).all()) and float(want.float().abs().max()) <= 1.0
    o = 0
    for i, ln in enumerate(lens):
        rows, m = bank.read(f"p{i}")
        assert rows.shape == (ln, D) and rows.dtype == torch.float16
        diff = rows.view(torch.int16) != want[o:o + ln].view(torch.int16)
        assert not bool(diff.any()), f"passage {i} (rows {o}..{o + ln}): {int(diff.sum())} of {diff.numel()} values differ, first at " \
                                     f"{diff.nonzero()[0].tolist()}"
        assert torch.equal(m, mask[o:o + ln])
        o += ln
    bank.clear()
    assert bank.info()["rows_used"] == 0 and len(bank) == 0 and bank.info()["nbits"] == nbits
    assert bank.add_compressed(["again"], codes[:5], res[:5], [5]) == 0
    assert torch.equal(bank.read("again")[0].view(torch.int16), want[:5].view(torch.int16))
    assert bank.format() == dict(nbits=nbits, n_centroids=N_CENTROIDS, bytes_per_row=4 + D * nbits // 8 + 1)
    plain = eng.create_bank(8, 2)                                       # an fp16 bank: info() as before, format() says nbits 0
    assert plain.info() == dict(passages=0, rows_used=0, capacity_rows=8)
    assert plain.format() == dict(nbits=0, n_centroids=0, bytes_per_row=2 * D + 1)


# ---- 2. forward == the fp16 bank of the decoded rows ---------------------------------------------------------------------------
def _two_queries(g):
    """Two queries of the fixture's geometry (int_base has one: its reversal is the second)."""
    q, _, qm, _ = _int_args(g)
    if q.shape[0] == 1:
        q, qm = torch.cat([q, q.flip(1)]), torch.cat([qm, qm])
    return q[:2].contiguous(), qm[:2].contiguous()


@pytest.mark.parametrize("name,dtype,fusion", [
    ("int_tiny", "fp16", False), ("int_tiny", "fp16", True), ("int_tiny", "bf16", False), ("int_tiny", "bf16", True),
    ("int_base", "fp16", False), ("int_base", "fp16", True), ("int_base", "bf16", False), ("int_base", "bf16", True),
    ("mores_tiny", "fp16", False), ("mores_tiny", "bf16", False)])
@pytest.mark.parametrize("nbits", [8, 2])
def test_forward_equals_the_fp16_bank_of_decoded_rows(name, dtype, fusion, nbits):
    eng, g = _engine(name, dtype)
    D, Lc = int(eng.arch["li_dim"]), int(g["Lc"])
    bank, _, _, _, lens = _fill(eng, _codec(D, nbits), [1, 7, 33], [Lc, 12, 20], seed=11)
    twin = _fp16_twin(eng, bank, lens, Lc)
    q, qm = _two_queries(g)
    sel = [2, 0, 2, 3, 2, 1]                                            # p2 in three pairs, under both queries; p4, p5 unused
    ids = [f"p{i}" for i in sel]
    kw = dict(granule=8, want_order=True, padded_len=Lc)
    if fusion:
        kw.update(fusion_from_li=True, fusion_multiplier=5.0, want_maxsim=True)
    got = eng.forward_interaction_bank(bank, q, qm, ids, 2, 3, **kw)
    ref = eng.forward_interaction_bank(twin, q, qm, ids, 2, 3, **kw)
    torch.cuda.synchronize()
    assert got["packed_segments"] == ref["packed_segments"] >= 2, "segments of different length"
    assert bool(torch.isfinite(got["logits"]).all())
    _equal(got, ref, ("logits", "logits2", "order") + (("maxsim",) if fusion else ()))
    if name == "mores_tiny":
        with pytest.raises(NotImplementedError):                       # mores_model.py:72-73, as on an fp16 bank
            eng.forward_interaction_bank(bank, q, qm, ids, 2, 3, fusion_from_li=True, padded_len=Lc)


# ---- 3. refusals leave the bank unchanged ---------------------------------------------------------------------------------------
def test_refused_calls_leave_the_bank_unchanged():
    from rmr_amd import _lib as L
    eng, g = _engine("int_tiny")
    D, Lc = int(eng.arch["li_dim"]), int(g["Lc"])
    codec = _codec(D, 4)
    bank, codes, res, _, lens = _fill(eng, codec, [1, 7, 33], [Lc, 12], spare_rows=5, spare_slots=3)
    twin = _fp16_twin(eng, bank, lens, Lc)
    q, qm = _two_queries(g)
    ids = ["p2", "p0", "p3", "p1", "p4", "p2"]
    st = torch.cuda.current_stream().cuda_stream

    def state(b):
        r = eng.forward_interaction_bank(b, q, qm, ids, 2, 3, granule=8, padded_len=Lc)
        torch.cuda.synchronize()
        return b.info(), r["logits"].clone(), len(b)
    info0, logits0, n0 = state(bank)
    tinfo0, tlogits0, tn0 = state(twin)

    def unchanged():
        i, l, n = state(bank)
        ti, tl, tn = state(twin)
        return i == info0 and torch.equal(l, logits0) and n == n0 and ti == tinfo0 and torch.equal(tl, tlogits0) and tn == tn0

    def raw_add(b, cd, rs, ln):
        cd, ln = np.ascontiguousarray(cd, dtype=np.int32), np.ascontiguousarray(ln, dtype=np.int32)
        rs = np.ascontiguousarray(rs, dtype=np.uint8)
        first = C.c_int32(-7)
        rc = eng.lib.rr_bank_add_plaid(b.h, cd.ctypes.data, rs.ctypes.data, None, ln.ctypes.data, len(ln), C.byref(first), st)
        assert rc != 0 and first.value == -7
        return rc
    c5, r5 = codes[:5].numpy().copy(), res[:5].numpy()
    bad = c5.copy()
    bad[4] = N_CENTROIDS                                                # a code equal to C
    assert raw_add(bank, bad, r5, [2, 3]) == L.RR_ERR_BAD_SHAPE and b"centroid code" in eng.lib.rr_bank_last_error(bank.h)
    with pytest.raises(ValueError):
        bank.add_compressed(["x", "y"], bad, r5, [2, 3])
    assert unchanged()
    bad[4] = -1
    assert raw_add(bank, bad, r5, [2, 3]) == L.RR_ERR_BAD_SHAPE and unchanged()
    assert raw_add(bank, c5, r5, [5, 0]) == L.RR_ERR_BAD_SHAPE           # a length of 0
    with pytest.raises(ValueError):
        bank.add_compressed(["x", "y"], c5, r5, [5, 0])
    assert unchanged()
    c6, r6 = codes[:6].numpy(), res[:6].numpy()                         # one row too many: 5 are free
    assert raw_add(bank, c6, r6, [6]) == L.RR_ERR_OOM
    with pytest.raises(MemoryError):
        bank.add_compressed(["x"], c6, r6, [6])
    assert unchanged()
    with pytest.raises(MemoryError):
        bank.add_compressed(["a", "b", "c", "d"], c5[:4], r5[:4], [1, 1, 1, 1])     # 4 passages, 3 slots are free
    with pytest.raises(ValueError):
        bank.add_compressed(["p1"], c5, r5, [5])                        # an id is added once
    with pytest.raises(ValueError):
        bank.add_compressed(["x"], c5, r5[:, :-1], [5])                 # residual rows of the wrong width
    assert unchanged() and "x" not in bank and "a" not in bank
    # the two formats do not mix
    li, ones = torch.randn(1, 8, D), torch.ones(1, 8)
    with pytest.raises(NotImplementedError):
        bank.add(["x"], li, ones)
    lic, onesc, one = li.cuda(), ones.cuda(), np.array([5], dtype=np.int32)
    assert eng.lib.rr_bank_add(bank.h, lic.data_ptr(), L.RR_F32, onesc.data_ptr(), one.ctypes.data, 1, 8, None, st) == L.RR_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError):
        twin.add_compressed(["x"], c5, r5, [5])
    assert raw_add(twin, c5, r5, [5]) == L.RR_ERR_UNSUPPORTED
    assert unchanged() and "x" not in twin
    # and what fits is still taken
    assert bank.add_compressed(["x"], c5, r5, [5]) == n0
    assert torch.equal(bank.read("x")[0].view(torch.int16), codec.decode(c5, r5).view(torch.int16))
    # a codec of another width, an engine that does not take it
    with pytest.raises(ValueError):
        eng.create_bank(8, 2, codec=_codec(128, 4))
    h = C.c_void_p()
    cen, w = np.zeros((4, D), np.float16), np.zeros(8, np.float32)
    assert eng.lib.rr_bank_create_plaid(eng.h, 8, 2, 3, 4, cen.ctypes.data, w.ctypes.data, C.byref(h)) == L.RR_ERR_UNSUPPORTED and not h.value


# ---- 4. the pipelined loop ------------------------------------------------------------------------------------------------------
def test_pipelined_records_equal_those_of_the_fp16_bank():
    import rmr_amd
    m, g = _model("int_tiny")
    Lq, D, Lc = int(g["Lq"]), g["query_li"].shape[2], int(g["Lc"])
    gen = torch.Generator().manual_seed(41)
    lens = [int(x) for x in torch.randint(1, Lc, (9,), generator=gen)] + [Lc]
    codec = _codec(D, 8)
    codes, res = _rows(codec, sum(lens), seed=43)
    comp = m.create_bank(sum(lens), len(lens), codec=codec)
    assert m.bank is comp
    comp.add_compressed([f"p{i}" for i in range(10)], codes, res, lens)
    twin = _fp16_twin(m.engine, comp, lens, Lc)
    queries = []
    for qi in range(4):
        docs = [int(x) for x in torch.randperm(10, generator=gen)[:5]]
        qmask = torch.ones(Lq)
        qmask[Lq - 1 - qi % 3:] = 0
        queries.append(dict(question_id=f"q{qi}", query_late_interaction=torch.randn(Lq, D, generator=gen), query_mask=qmask,
                            retrieved_docs=[dict(passage_id=f"p{d}", content=f"text {d}") for d in docs], pos_item_ids=[f"p{docs[2]}"]))
    Ks = [1, 3]
    a = rmr_amd.rerank_dataset_pipelined(queries, m, 2, Ks)
    m.bank = twin
    b = rmr_amd.rerank_dataset_pipelined(queries, m, 2, Ks)
    assert len(a["output"]) == 4 and all(len(r["top_ranking_passages"]) == 5 for r in a["output"])
    assert a["output"] == b["output"] and a["metrics"] == b["metrics"]


# ---- 5. past 4 GiB -----------------------------------------------------------------------------------------------------------------
def test_decode_rows_past_4_gib_of_residuals():
    """rr_op_plaid_decode_rows over a residual buffer of 2^32 bytes + 64 rows (li_dim 128, nbits 8: 128 bytes per row): the 50 rows
    from row 2^25 + 8 on start 1 024 bytes behind byte 2^32.  A row offset cut to 32 bits would read rows 8.. of the buffer, which
    hold other data."""
    from rmr_amd import _lib as L
    from test_gpu_large_index import _need
    lib = L.load()
    D, nbits, rb = 128, 8, 128
    total = (1 << 32) // rb + 64
    _need(total * rb + total * 4 + (1 << 26))
    codec = _codec(D, nbits)
    first, n = (1 << 25) + 8, 50
    assert first * rb > 1 << 32 and first + n <= total
    codes_d = torch.empty(total, dtype=torch.int32, device="cuda")
    res_d = torch.empty(total, rb, dtype=torch.uint8, device="cuda")
    assert res_d.numel() > 1 << 32
    codes, res = _rows(codec, 64, seed=51)
    alias_c, alias_r = _rows(codec, 64, seed=52)
    codes_d[:64], res_d[:64] = alias_c.cuda(), alias_r.cuda()           # where a wrapped offset would land
    codes_d[total - 64:], res_d[total - 64:] = codes.cuda(), res.cuda()
    cen_d, w_d = codec.centroids.cuda(), codec.bucket_weights.cuda()
    out = torch.full((n + 6, D), float("nan"), dtype=torch.float16, device="cuda")
    rc = lib.rr_op_plaid_decode_rows(cen_d.data_ptr(), N_CENTROIDS, w_d.data_ptr(), nbits, D, codes_d.data_ptr(), res_d.data_ptr(), first, n,
                                     out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    k = first - (total - 64)
    want = codec.decode(codes[k:k + n], res[k:k + n])
    assert torch.equal(out[:n].cpu().view(torch.int16), want.view(torch.int16))
    assert bool(torch.isnan(out[n:]).all()), "nothing is written behind the n rows"
    del codes_d, res_d
    torch.cuda.empty_cache()
