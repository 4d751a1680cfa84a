"""GPU: the device-resident passage-embedding bank of the interaction rerankers — rr_bank_* and rr_forward_interaction_bank
through PassageBank, RerankEngine.forward_interaction_bank, InteractionRerankModel.forward_passages and
pipeline.InteractionStages.

Contract (include/rerank_mi355.h): the bank holds `context_li.half()` and (mask != 0) at every passage's own length, and a bank
forward's logits are bit for bit those of the explicit packed call on float32(bank rows) and the bank's masks; on an fp16 handle
also those of the call on the original float32 tensors.  Every equality below is torch.equal ("resid_split" = 0, as
tests/test_gpu_packed_families.py sets it for its exact cases)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from helpers import O, arch_from_cfg
from test_gpu_packed_families import GATE, _cfg, _int_args, _int_engine, _labels, _npz

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


@functools.lru_cache(maxsize=None)
def _engine(name, dtype="fp16"):
    """One engine per (fixture, operand type) for the whole module, "resid_split" = 0."""
    return _int_engine(name, dtype)


def _lengths(cm):
    """1 + index of the last unmasked token, at least 1 (host list)."""
    cols = torch.arange(1, cm.shape[1] + 1, device=cm.device)
    return ((cm != 0) * cols).amax(1).clamp(min=1).cpu().tolist()


def _banked(c, cm, lens=None):
    """What the explicit call takes in the bank's place: float32(bank rows), zero beyond a passage's length, and the bank's mask
    bytes as floats."""
    lens = _lengths(cm) if lens is None else lens
    keep = torch.arange(c.shape[1], device=c.device)[None, :] < torch.tensor(lens, device=c.device)[:, None]
    return c.half().float() * keep[:, :, None], ((cm != 0) & keep).float(), lens


def _same(a, b, keys):
    for k in keys:
        assert a[k] is not None and torch.equal(a[k], b[k]), f"{k} differs: {(a[k].float() - b[k].float()).abs().max().item():.3e}"


# ---- 1. ingest -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["int_tiny", "int_base"])             # li_dim 64 and 128
@pytest.mark.parametrize("src", [torch.float32, torch.float16])
def test_ingest_round_trip_and_refusals(name, src):
    eng, g = _engine(name)
    D = int(eng.arch["li_dim"])
    gen = torch.Generator().manual_seed(17)
    parts = []
    for Lc, n in ((40, 3), (64, 3)):                                    # two separate add calls
        x = (torch.randn(n, Lc, D, generator=gen) * 3.0).to(src)
        # the largest fp16, a value that rounds to a subnormal, the smallest normal's neighbourhood, two ties (1 + 2^-11 goes down
        # to the even 1, 1 + 3 * 2^-11 up to the even 1 + 2^-9)
        x[0, 0, :5] = torch.tensor([65504.0, -1e-7, 6.1e-5, 1.00048828125, 1.00146484375]).to(src)
        m = torch.zeros(n, Lc)
        for i, ln in enumerate((Lc, Lc // 2 + 1, 7)[:n]):
            m[i, :ln] = 1.0
        m[0, 3], m[0, 5] = 0.0, 0.0                                     # interior zeros (skiplist punctuation) stay where they are
        m[1, 1], m[1, 2] = 2.0, -1.0                                    # any non-zero value is 1
        if Lc == 64:
            m[2] = 0.0                                                  # no unmasked token: length 1
        parts.append((x, m))
    want_len = [_lengths(m) for _, m in parts]
    assert want_len[1][2] == 1
    used = sum(sum(w) for w in want_len)
    bank = eng.create_bank(used + 5, 7)
    o = 0
    for (x, m), wl in zip(parts, want_len):
        ids = [f"{x.shape[1]}/{i}" for i in range(x.shape[0])]
        first = bank.add(ids, x.cuda() if x.shape[1] == 40 else x, m)   # device and host tensors
        assert first == o and bank.lookup(ids)[1].tolist() == wl
        o += len(ids)
    info = bank.info()
    assert info == dict(passages=6, rows_used=used, capacity_rows=used + 5) and bank.padded_len == 64
    for (x, m), wl in zip(parts, want_len):
        for i, ln in enumerate(wl):
            rows, mask = bank.read(f"{x.shape[1]}/{i}")
            assert rows.shape == (ln, D) and torch.equal(rows.view(torch.int16), x[i, :ln].half().view(torch.int16))
            assert torch.equal(mask, (m[i, :ln] != 0).to(torch.uint8))
    # three refusals, each before anything is enqueued: the bank is unchanged
    y, ones = torch.randn(2, 8, D, generator=gen).to(src), torch.ones(2, 8)
    with pytest.raises(MemoryError):
        bank.add(["r0"], y[:1], ones[:1], lengths=[6])                  # 6 rows, 5 are free
    with pytest.raises(MemoryError):
        bank.add(["s0", "s1"], y, ones, lengths=[1, 1])                 # 2 passages, 1 slot is free
    with pytest.raises(ValueError):
        bank.add(["z0"], y[:1], ones[:1], lengths=[0])
    with pytest.raises(ValueError):
        bank.add(["40/1"], y[:1], ones[:1])                             # an id is added once
    assert bank.info() == info and len(bank) == 6 and "r0" not in bank and "s0" not in bank and "z0" not in bank
    assert bank.add(["r0"], y[:1], ones[:1], lengths=[5]) == 6          # and it still takes what fits
    rows, _ = bank.read("r0")
    assert torch.equal(rows.view(torch.int16), y[0, :5].half().view(torch.int16))
    with pytest.raises(KeyError, match="'nope'"):
        bank.lookup(["40/0", "nope"])


# ---- 2. forward == the explicit packed call ----------------------------------------------------------------------------------
def _fixture_bank(eng, g, extra=0, seed=23):
    """A bank holding the fixture's passages as "d0".."d5", between `extra` filler passages before and after them, with room
    for one more."""
    q, c, qm, cm = _int_args(g)
    n, Lc, D = c.shape
    bank = eng.create_bank((n + 2 * extra + 1) * Lc, n + 2 * extra + 1)
    gen = torch.Generator().manual_seed(seed)

    def filler(tag):
        if extra:
            ln = torch.randint(1, Lc + 1, (extra,), generator=gen)
            m = (torch.arange(Lc)[None, :] < ln[:, None]).float()
            bank.add([f"{tag}{i}" for i in range(extra)], torch.randn(extra, Lc, D, generator=gen), m, lengths=ln.tolist())
    filler("a")
    bank.add([f"d{i}" for i in range(n)], c, cm)
    filler("b")
    return bank, (q, c, qm, cm)


@pytest.mark.parametrize("name", ["int_tiny", "mores_tiny", "int_base"])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("granule", [8, 16])
def test_forward_equals_the_explicit_packed_call(name, dtype, granule):
    eng, g = _engine(name, dtype)
    Bq, K = int(g["Bq"]), int(g["K"])
    bank, (q, c, qm, cm) = _fixture_bank(eng, g)
    ids = [f"d{i}" for i in range(Bq * K)]
    c16, cmb, lens = _banked(c, cm)
    kw = dict(granule=granule, want_order=True, want_scores=True)
    ref = eng.forward_interaction_packed(q, c16, qm, cmb, Bq, K, _labels(g), lengths=lens, **kw)
    got = eng.forward_interaction_bank(bank, q, qm, ids, Bq, K, _labels(g), **kw)
    torch.cuda.synchronize()
    assert got["packed_segments"] == ref["packed_segments"] >= 2 and got["packed_rows"] == ref["packed_rows"]
    _same(got, ref, ("logits", "logits2", "loss", "order", "scores"))
    orig = eng.forward_interaction_packed(q, c, qm, cm, Bq, K, _labels(g), lengths=lens, **kw)
    torch.cuda.synchronize()
    d = (got["logits"] - orig["logits"]).abs().max().item()
    dg = (got["logits"].cpu() - torch.from_numpy(g["logits"]).reshape(-1)).abs().max().item()
    print(f"[{name} {dtype} granule {granule}] bank vs the original float32 tensors {d:.3e}; vs the fp32 golden {dg:.3e}")
    if dtype == "fp16":               # float32 -> fp16 happens once either way
        _same(got, orig, ("logits", "logits2", "loss", "order"))
        assert dg <= GATE


# ---- 3. reuse and order --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["int_tiny", "mores_tiny"])
def test_passages_are_reused_in_any_order(name):
    eng, g = _engine(name)
    Bq, K = int(g["Bq"]), int(g["K"])
    bank, (q, c, qm, cm) = _fixture_bank(eng, g, extra=6)               # 18 passages, 4 of them used
    assert len(bank) == 3 * c.shape[0]
    sel = [3, 0, 3, 5, 3, 1]                                            # d3 in three pairs, under both queries
    c16, cmb, lens = _banked(c, cm)
    idx = torch.tensor(sel, device="cuda")
    kw = dict(granule=8, want_order=True)
    ref = eng.forward_interaction_packed(q, c16[idx], qm, cmb[idx], Bq, K, _labels(g), lengths=[lens[i] for i in sel], **kw)
    got = eng.forward_interaction_bank(bank, q, qm, [f"d{i}" for i in sel], Bq, K, _labels(g), **kw)
    torch.cuda.synchronize()
    _same(got, ref, ("logits", "logits2", "loss", "order"))
    assert bank.lookup(["d3"])[0].tolist() == [6 + 3]


# ---- 4. unequal lists ------------------------------------------------------------------------------------------------------------
def test_unequal_lists_equal_the_packed_list_call():
    eng, g = _engine("int_tiny")
    bank, (q, c, qm, cm) = _fixture_bank(eng, g)
    sizes = [1, 5, 3]
    q3 = torch.cat([q, q[:1].flip(1)])                                  # a third query
    qm3 = torch.cat([qm, qm[:1].flip(1)])
    sel = [4, 0, 1, 2, 3, 5, 2, 4, 0]
    c16, cmb, lens = _banked(c, cm)
    idx = torch.tensor(sel, device="cuda")
    labels = torch.tensor([1.0, 0, 1, 0, 0, 0, 0, 0, 1], device="cuda")
    kw = dict(list_sizes=sizes, granule=8, want_order=True, want_scores=True)
    ref = eng.forward_interaction_packed(q3, c16[idx], qm3, cmb[idx], None, None, labels, lengths=[lens[i] for i in sel], **kw)
    got = eng.forward_interaction_bank(bank, q3, qm3, [f"d{i}" for i in sel], None, None, labels, **kw)
    torch.cuda.synchronize()
    _same(got, ref, ("logits", "loss", "list_loss", "order", "scores"))
    assert got["list_loss"].shape == (3,) and got["order"].shape == (9,)
    with pytest.raises(ValueError):
        eng.forward_interaction_bank(bank, q3, qm3, [f"d{i}" for i in sel], None, None, labels, pair_range=(0, 4), **kw)


# ---- 5. fusion -----------------------------------------------------------------------------------------------------------------
def _raw(eng, bank_h, q, qm, pp, pq, seg_n, seg_len, Lc, fusion, outs):
    """rr_forward_interaction_bank itself, on caller-held outputs."""
    pp, pq = np.asarray(pp, dtype=np.int32), np.asarray(pq, dtype=np.int32)
    return eng.lib.rr_forward_interaction_bank(eng.h, bank_h, q.data_ptr(), qm.data_ptr(), q.shape[0], q.shape[1], pp.ctypes.data,
                                               pq.ctypes.data, len(seg_n), (C.c_int32 * len(seg_n))(*seg_n),
                                               (C.c_int32 * len(seg_len))(*seg_len), Lc, int(fusion), 5.0, outs[0].data_ptr(),
                                               outs[1].data_ptr(), outs[2].data_ptr() if fusion else None,
                                               torch.cuda.current_stream().cuda_stream)


def _sentinels(n):
    return [torch.full((n,), SENTINEL, device="cuda") for _ in range(3)]


def _untouched(outs):
    torch.cuda.synchronize()
    return all(bool((t == SENTINEL).all()) for t in outs)


def test_fusion_from_li_equals_the_explicit_call_and_mores_refuses():
    eng, g = _engine("int_tiny")
    Bq, K = int(g["Bq"]), int(g["K"])
    bank, (q, c, qm, cm) = _fixture_bank(eng, g)
    Lq, Lc = q.shape[1], c.shape[1]
    gen = torch.Generator().manual_seed(5)
    dark = torch.randn(1, Lc, c.shape[2], generator=gen).cuda()         # a passage without an unmasked token
    bank.add(["dark"], dark, torch.zeros(1, Lc))
    sel = ["d0", "dark", "d2", "d3", "d4", "d1"]
    call = torch.cat([c, dark])[torch.tensor([0, 6, 2, 3, 4, 1], device="cuda")]
    cmall = torch.cat([cm, torch.zeros(1, Lc, device="cuda")])[torch.tensor([0, 6, 2, 3, 4, 1], device="cuda")]
    c16, cmb, lens = _banked(call, cmall)
    assert lens[1] == 1
    kw = dict(granule=8, fusion_from_li=True, fusion_multiplier=5.0, want_maxsim=True, want_order=True)
    ref = eng.forward_interaction_packed(q, c16, qm, cmb, Bq, K, _labels(g), lengths=lens, **kw)
    got = eng.forward_interaction_bank(bank, q, qm, sel, Bq, K, _labels(g), **kw)
    plain = eng.forward_interaction_bank(bank, q, qm, sel, Bq, K, _labels(g), granule=8)
    torch.cuda.synchronize()
    _same(got, ref, ("logits", "logits2", "loss", "order", "maxsim"))
    assert got["maxsim"][1].item() == -9999.0 * Lq
    assert not torch.equal(got["logits"], plain["logits"]), "the fusion bias changes the logits"
    with pytest.raises(ValueError):
        eng.forward_interaction_bank(bank, q, qm, sel, Bq, K, want_maxsim=True)

    em, gm = _engine("mores_tiny")
    qmo, _, qmm, _ = _int_args(gm)
    with pytest.raises(NotImplementedError):                           # mores_model.py:72-73
        em.forward_interaction_bank(bank, qmo, qmm, sel, Bq, K, fusion_from_li=True)
    outs = _sentinels(6)
    from rmr_amd import _lib as L
    rc = _raw(em, bank.h, qmo, qmm, [0, 1, 2, 3, 4, 5], [0, 0, 0, 1, 1, 1], [6], [Lc], Lc, True, outs)
    assert rc == L.RR_ERR_UNSUPPORTED and _untouched(outs)
    # the same bank serves the MORES handle without fusion
    r = em.forward_interaction_bank(bank, qmo, qmm, sel, Bq, K)
    torch.cuda.synchronize()
    assert torch.isfinite(r["logits"]).all()


# ---- 6. refusals write nothing ---------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing():
    from rmr_amd import _lib as L
    eng, g = _engine("int_tiny")
    bank, (q, c, qm, cm) = _fixture_bank(eng, g)
    Lc, lens = c.shape[1], _lengths(cm)                                 # [12, 25, 22, 32, 37, 12]
    pp, pq, seg = [0, 1, 2, 3, 4, 5], [0, 0, 0, 1, 1, 1], ([6], [Lc])
    outs = _sentinels(65)
    call = lambda pp=pp, pq=pq, seg=seg, b=bank.h, e=eng: _raw(e, b, q, qm, pp, pq, seg[0], seg[1], Lc, False, outs)
    assert call(pp=[0, 1, 6, 3, 4, 5]) == L.RR_ERR_BAD_SHAPE and _untouched(outs)          # index outside the bank
    assert call(pp=[0, 1, -1, 3, 4, 5]) == L.RR_ERR_BAD_SHAPE and _untouched(outs)
    assert lens[1] > 24
    assert call(seg=([6], [24])) == L.RR_ERR_BAD_SHAPE and _untouched(outs)                # passage 1 is longer than its segment
    assert call(pp=[0] * 65, pq=[0] * 65, seg=([1] * 65, [16] * 65)) == L.RR_ERR_BAD_SHAPE and _untouched(outs)   # 65 segments
    assert call(pq=[0, 0, 0, 1, 1, 2]) == L.RR_ERR_BAD_SHAPE and _untouched(outs)          # query index out of range
    assert call(seg=([6], [Lc + 1])) == L.RR_ERR_BAD_SHAPE and _untouched(outs)            # above the padded length
    wide, _ = _engine("int_base")                                                           # li_dim 128
    other = wide.create_bank(64, 4)
    assert call(b=other.h) == L.RR_ERR_BAD_SHAPE and _untouched(outs)
    assert b"li_dim" in eng.lib.rr_last_error(eng.h)
    # and the call that is fine runs
    assert call() == 0
    torch.cuda.synchronize()
    ref = eng.forward_interaction_bank(bank, q, qm, [f"d{i}" for i in range(6)], 2, 3, granule=Lc)
    torch.cuda.synchronize()
    assert torch.equal(outs[0][:6], ref["logits"]) and bool((outs[0][6:] == SENTINEL).all())


# ---- 7. past 4 GiB ---------------------------------------------------------------------------------------------------------------
def test_bank_rows_past_4_gib():
    """17 000 passages of 1 024 rows of 128 fp16 values fill 4.46 GB: the int_base passages added behind them lie beyond byte
    2^32 (element 2^31) of the bank, and the forward over them is case 2's."""
    from test_gpu_large_index import _need
    eng, g = _engine("int_base")
    n0, L0, D = 17000, 1024, 128
    big = n0 * L0 * D * 2
    _need(2 * big + n0 * L0 * 5 + (1 << 28))
    q, c, qm, cm = _int_args(g)
    Bq, K = int(g["Bq"]), int(g["K"])
    bank = eng.create_bank(n0 * L0 + c.shape[0] * c.shape[1], n0 + c.shape[0])
    zeros = torch.zeros([n0, L0, D], dtype=torch.float16, device="cuda")
    bank.add(range(n0), zeros, torch.ones(n0, L0, device="cuda"), lengths=[L0] * n0)
    del zeros
    ids = [f"d{i}" for i in range(c.shape[0])]
    assert bank.add(ids, c, cm) == n0 and bank.info()["rows_used"] * D * 2 > 1 << 32
    c16, cmb, lens = _banked(c, cm)
    rows, mask = bank.read("d5")
    assert torch.equal(rows.view(torch.int16), c[5, :lens[5]].half().cpu().view(torch.int16)) and bool(mask.all())
    kw = dict(granule=16, want_order=True, padded_len=c.shape[1])
    ref = eng.forward_interaction_packed(q, c16, qm, cmb, Bq, K, _labels(g), lengths=lens, granule=16, want_order=True)
    got = eng.forward_interaction_bank(bank, q, qm, ids, Bq, K, _labels(g), **kw)
    torch.cuda.synchronize()
    _same(got, ref, ("logits", "logits2", "loss", "order"))
    rows0, _ = bank.read(n0 - 1)
    assert rows0.shape == (L0, D) and not bool(rows0.view(torch.int16).any())
    bank.close()
    torch.cuda.empty_cache()


# ---- 8. pipeline / 9. drop-in class ------------------------------------------------------------------------------------------------
def _model(name, dtype="fp16"):
    import rmr_amd
    g = _npz(name)
    cfg = _cfg(g, str(g["loss_fn"]))
    mores = bool(g["mores"])
    conf = dict(cross_encoder_num_hidden_layers=cfg.ce_layers, cross_encoder_max_position_embeddings=cfg.ce_max_pos,
                loss_fn=cfg.loss_fn, interaction_type="MORES" if mores else "NORMAL", arch=arch_from_cfg(cfg, False, dtype))
    m = rmr_amd.InteractionRerankModel(conf, state_dict=O.make_interaction_weights(cfg, mores, seed=0))
    m.engine.set_option("resid_split", 0)
    return m, g


@pytest.mark.parametrize("name", ["int_tiny", "mores_tiny"])
def test_forward_passages_gives_what_forward_gives(name):
    m, g = _model(name)
    q, c, qm, cm = _int_args(g)
    K = int(g["K"])
    lab = [float(x) for x in g["labels"]] if g["labels"].size else None
    with pytest.raises(RuntimeError):
        m.forward_passages(q, qm, ["d0"] * 6, K - 1)
    bank = m.create_bank(c.shape[0] * c.shape[1], 16)
    ids = [f"d{i}" for i in range(c.shape[0])]
    bank.add(ids, c.cpu(), cm.cpu())
    want = m(q, c, K - 1, qm, cm, labels=lab, want_order=True)
    got = m.forward_passages(q, qm, ids, K - 1, labels=lab, want_order=True)
    torch.cuda.synchronize()
    assert got.logits.shape == want.logits.shape
    assert torch.equal(got.logits, want.logits) and torch.equal(got.loss, want.loss) and torch.equal(got.order, want.order)
    lists = m.forward_passages(q, qm, ids, None, labels=lab, candidates_per_query=[2, 4])
    torch.cuda.synchronize()
    assert lists.order.shape == (6,) and lists.list_loss.shape == (2,)


@pytest.mark.parametrize("name", ["int_tiny", "mores_tiny"])
def test_pipeline_records_equal_the_serial_loop(name):
    import rmr_amd
    from rmr_amd.pipeline import InteractionStages
    m, g = _model(name)
    Lq, D, Lc = int(g["Lq"]), g["query_li"].shape[2], int(g["Lc"])
    gen = torch.Generator().manual_seed(31)
    n_pass = 10
    ln = torch.randint(1, Lc + 1, (n_pass,), generator=gen)
    cm = (torch.arange(Lc)[None, :] < ln[:, None]).float()
    bank = m.create_bank(int(ln.sum()), n_pass)
    bank.add([f"doc{i}" for i in range(n_pass)], torch.randn(n_pass, Lc, D, generator=gen), cm)
    sizes = [3, 1, 4, 2, 3]
    queries = []
    for qi, k in enumerate(sizes):
        docs = [int(x) for x in torch.randperm(n_pass, generator=gen)[:k]]
        qmask = torch.ones(Lq)
        qmask[Lq - 1 - qi % 3:] = 0
        queries.append(dict(question_id=f"q{qi}", query_late_interaction=torch.randn(Lq, D, generator=gen), query_mask=qmask,
                            retrieved_docs=[dict(passage_id=f"doc{d}", content=f"text {d}") for d in docs],
                            pos_item_ids=[f"doc{docs[-1]}"]))
    pointwise = m.engine.arch["loss_fn"] != "negative_sampling"

    def forward_batch(batch):
        ids = [d["passage_id"] for q in batch for d in q["retrieved_docs"]]
        lab = [1.0 if d["passage_id"] in q["pos_item_ids"] else 0.0 for q in batch for d in q["retrieved_docs"]] if pointwise else None
        out = m.forward_passages(torch.stack([q["query_late_interaction"] for q in batch]).cuda(),
                                 torch.stack([q["query_mask"] for q in batch]).cuda(), ids, None, labels=lab,
                                 candidates_per_query=[len(q["retrieved_docs"]) for q in batch], want_order=True)
        return dict(logits=out.logits.reshape(-1), order=out.order, loss=out.loss, list_loss=out.list_loss)

    Ks = [1, 2]
    serial = rmr_amd.rerank_dataset(queries, forward_batch, 2, Ks, ragged=True)
    stats = {}
    piped = rmr_amd.rerank_dataset_pipelined(queries, m, 2, Ks, ragged=True, stats=stats)
    assert stats["batches"] == 3
    assert piped["output"] == serial["output"] and piped["metrics"] == serial["metrics"]
    assert all(f"pos_item_ids_recall_at_{k}" in piped["metrics"] for k in Ks)
    assert len(piped["output"]) == 5 and [len(r["top_ranking_passages"]) for r in piped["output"]] == sizes
    # uniform lists through the same stages
    uni = [dict(q, retrieved_docs=(q["retrieved_docs"] * 4)[:2]) for q in queries]
    a = rmr_amd.rerank_dataset_pipelined(uni, m, 2, Ks, stages=InteractionStages(m, 2, 2, uni[0], granule=8))

    def forward_uniform(batch):
        lab = [1.0 if d["passage_id"] in q["pos_item_ids"] else 0.0 for q in batch for d in q["retrieved_docs"]] if pointwise else None
        o = m.forward_passages(torch.stack([q["query_late_interaction"] for q in batch]).cuda(),
                               torch.stack([q["query_mask"] for q in batch]).cuda(),
                               [d["passage_id"] for q in batch for d in q["retrieved_docs"]], 1, labels=lab, want_order=True, granule=8)
        return dict(logits=o.logits.reshape(len(batch), 2), order=o.order, loss=o.loss)
    b = rmr_amd.rerank_dataset(uni, forward_uniform, 2, Ks)
    assert a["output"] == b["output"] and a["metrics"] == b["metrics"]
    # a passage the bank does not hold
    bad = [dict(q) for q in queries]
    bad[3] = dict(bad[3], retrieved_docs=bad[3]["retrieved_docs"] + [dict(passage_id="doc-missing", content="")])
    with pytest.raises(KeyError, match="doc-missing"):
        rmr_amd.rerank_dataset_pipelined(bad, m, 2, Ks, ragged=True)
    m.bank = None
    with pytest.raises(ValueError):
        rmr_amd.rerank_dataset_pipelined(queries, m, 2, Ks, ragged=True)
