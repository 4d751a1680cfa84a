"""GPU: the joint family (RerankModel) from compact tokens.  rr_assemble_joint against the padded joint rows of
RerankModel.forward packed by pack_rows, its refusal of bad descriptors, RerankEngine.forward_joint_tokens_packed against
RerankModel.forward (packed rows: bit for bit; padded: the fp16 parity gate), and rerank_dataset_pipelined(queries, RerankModel)
against rerank_dataset driven by RerankModel.forward over the reference's padded inputs."""
import ctypes as C
import dataclasses
import json
import random
import threading

import numpy as np
import pytest
import torch

from helpers import O
from test_gpu_pipeline import WORDS, _hf_tokenizer
from test_gpu_vision import _arch, _load

pytestmark = pytest.mark.gpu

S = 512          # max_decoder_source_length = the text encoder's max_pos


def _cfg():
    return dataclasses.replace(_load("vit_tiny")["cfg"], max_pos=S, ce_max_pos=S + 48, loss_fn="2H_BCE")


def _model(hf, packed=True, vit=True, instr=None):
    import rmr_amd
    cfg = _cfg()
    w = O.make_weights(cfg, seed=0, vision=True)
    arch = _arch(cfg, "fp16")
    fn = None
    if vit:
        w.update(O.make_vit_weights(cfg, seed=5))
    else:
        arch["vit_layers"] = 0
        Vh, P = cfg.vision_hidden, cfg.n_patches

        def fn(px):          # a stand-in for the reference-side vision encoder; exact in fp32, so host and device agree
            x = torch.as_tensor(px, dtype=torch.float32).reshape(px.shape[0], -1)
            return x[:, :Vh] * 0.5, (x[:, Vh:Vh + P * Vh] * 0.25).reshape(-1, P, Vh)
    conf = dict(cross_encoder_num_hidden_layers=cfg.ce_layers, cross_encoder_max_position_embeddings=cfg.ce_max_pos,
                loss_fn="2H_BCE", pos_weight=None, arch=arch, decoder_tokenizer=hf, max_decoder_source_length=S,
                packed_rows=packed, instruction_token_id=instr, image_feature_fn=fn)
    return rmr_amd.RerankModel(conf, state_dict=w), cfg


def _text(rng, n):
    return " ".join(rng.choice(WORDS) + rng.choice(["", "", "s", "ing", ",", "."]) for _ in range(n))


def _queries(n, K, ql, seed, cfg, instr=None):
    rng = random.Random(seed)
    px = O.make_pixel_values(cfg, n, seed=seed)
    out = []
    for i in range(n):
        real = rng.randint(4, ql)
        body = [rng.randint(110, 1999) for _ in range(real - 2)]
        if instr is not None:
            body[rng.randrange(len(body))] = instr
        q_ids = [101] + body + [102] + [0] * (ql - real)
        docs = [{"passage_id": f"p{i}_{k}", "content": _text(rng, rng.choice([0, 5, rng.randint(20, 200), rng.randint(300, 700)]))}
                for k in range(K)]
        out.append({"question_id": f"q{i}", "query_input_ids": torch.tensor(q_ids),
                    "query_attention_mask": torch.tensor([1] * real + [0] * (ql - real)), "pixel_values": px[i],
                    "retrieved_docs": docs, "pos_item_ids": [d["passage_id"] for d in rng.sample(docs, min(2, K))]})
    return out


def _padded(hf, batch, K):
    """The reference's inputs of RerankModel.forward: query ids / mask as the dataset gives them, contexts through
    tokenize_retrieved_docs (FLMRContextEncoderTokenizer)."""
    from rmr_amd.pair_inputs import flmr_context_inputs
    enc = flmr_context_inputs([d["content"] for q in batch for d in q["retrieved_docs"]], hf, S)
    return (torch.stack([q["query_input_ids"] for q in batch]), torch.stack([q["query_attention_mask"] for q in batch]),
            enc["input_ids"], enc["attention_mask"])


def _joint_rows(q_ids, q_am, c_ids, c_am, K):
    ql = q_ids.shape[1]
    return (torch.cat([q_ids.repeat_interleave(K, 0), c_ids[:, 2:2 - ql]], 1).long(),
            torch.cat([q_am.repeat_interleave(K, 0), c_am[:, 2:2 - ql]], 1).long())


@pytest.fixture(scope="module")
def hf(tmp_path_factory):
    return _hf_tokenizer(tmp_path_factory.mktemp("vocab"))


@pytest.fixture(scope="module")
def joint_case(hf):
    from rmr_amd.pair_inputs import NativePairTokenizer
    from rmr_amd.pipeline import joint_compact_batch
    tok = NativePairTokenizer(hf, n_threads=4)
    K, ql = 40, 16
    batch = _queries(4, K, ql, 3, _cfg())
    pool, desc = joint_compact_batch(tok, batch, [d["content"] for q in batch for d in q["retrieved_docs"]], K, ql, S)
    ids, am = _joint_rows(*_padded(hf, batch, K), K)
    lengths = ql + np.minimum(desc[:, 2].astype(np.int64) + 1, S - ql)
    return dict(tok=tok, batch=batch, K=K, ql=ql, pool=pool, desc=desc, ids=ids, am=am, lengths=lengths, N=len(batch) * K)


def _tables(case, lengths, ql):
    from rmr_amd.pair_inputs import group_pairs_by_length
    N, floor = len(lengths), max(ql + 1, 32)
    if case == "padded":
        return np.arange(N), [N], [S]
    if case == "granule16":
        return group_pairs_by_length(lengths, S, 16, floor)
    if case == "merged":
        return group_pairs_by_length(lengths, S, 16, floor, 4096)
    if case in ("max64", "exact"):               # 64 segments (the maximum), each as long as its longest pair (or the floor)
        order = np.argsort(lengths, kind="stable")
        parts = np.array_split(order, 64 if case == "max64" else 8)
        return order, [len(p) for p in parts], [max(floor, int(lengths[p].max())) for p in parts]
    raise ValueError(case)


@pytest.mark.parametrize("case", ["padded", "granule16", "merged", "max64", "exact"])
def test_assemble_joint_equals_the_padded_rows_packed(joint_case, case):
    import rmr_amd
    from rmr_amd.pair_inputs import pack_rows, pair_lengths
    c = joint_case
    eng = rmr_amd.RerankEngine(_arch(_cfg(), "fp16"))
    assert c["lengths"].tolist() == pair_lengths(c["ids"], c["am"]).tolist()      # the lengths forward_joint_packed derives
    assert (c["lengths"] == S).any() and (c["lengths"] < 64).any()
    order, seg_n, seg_len = _tables(case, c["lengths"], c["ql"])
    ids, am = eng.assemble_joint(c["pool"].cuda(), c["desc"], order, seg_n, seg_len, c["ql"], S, c["tok"].special_ids)
    torch.cuda.synchronize()
    o = torch.from_numpy(np.asarray(order, dtype=np.int64))
    assert torch.equal(ids.cpu(), pack_rows(c["ids"], o, seg_n, seg_len).reshape(-1)), case
    assert torch.equal(am.cpu(), pack_rows(c["am"], o, seg_n, seg_len).reshape(-1)), case


def test_assemble_joint_refuses_bad_descriptors_and_writes_nothing(joint_case):
    import rmr_amd
    from rmr_amd import _lib as L
    c = joint_case
    eng = rmr_amd.RerankEngine(_arch(_cfg(), "fp16"))
    N, ql = c["N"], c["ql"]
    _, sep, pad = c["tok"].special_ids
    pool_d = c["pool"].cuda()
    order, seg_n, seg_len = _tables("granule16", c["lengths"], ql)
    rows = sum(n * s for n, s in zip(seg_n, seg_len))
    outs = [torch.full((rows,), -3, dtype=torch.int64, device="cuda") for _ in range(2)]
    stream = torch.cuda.current_stream().cuda_stream
    o32 = np.ascontiguousarray(order, dtype=np.int32)
    good = c["desc"]

    def call(d, o=o32, sn=seg_n, sl=seg_len):
        return eng.lib.rr_assemble_joint(eng.h, pool_d.data_ptr(), pool_d.numel(), d.ctypes.data, N, o.ctypes.data, len(sn),
                                         (C.c_int32 * len(sn))(*sn), (C.c_int32 * len(sn))(*sl), ql, S, sep, pad,
                                         outs[0].data_ptr(), outs[1].data_ptr(), stream)
    bad = []
    d = good.copy()
    d[3, 1], d[3, 2] = pool_d.numel() - 1, max(2, int(d[3, 2]))      # a context run past the end of the pool
    bad.append(d)
    d = good.copy()
    d[5, 0] = pool_d.numel() - ql                                       # the query's mask past the end of the pool
    bad.append(d)
    d = good.copy()
    d[7, 1] = -1                                                        # a negative offset
    bad.append(d)
    d = good.copy()
    shortest = int(np.argmin(c["lengths"]))
    d[shortest, 2] += 64                                                # a pair longer than its segment
    bad.append(d)
    for d in bad:
        assert call(d) == L.RR_ERR_BAD_SHAPE
        with pytest.raises(ValueError):
            eng.assemble_joint(pool_d, d, order, seg_n, seg_len, ql, S, c["tok"].special_ids)
    bad_order = o32.copy()
    bad_order[0] = bad_order[1]                                         # not a permutation
    assert call(good, o=bad_order) == L.RR_ERR_BAD_SHAPE
    short = np.argsort(c["lengths"], kind="stable").astype(np.int32)
    assert call(good, o=short, sn=[1, N - 1], sl=[ql, S]) == L.RR_ERR_BAD_SHAPE          # seg_len <= query_len
    assert call(good, o=short, sn=[1, N - 1], sl=[ql + 1, S]) == L.RR_ERR_BAD_SHAPE      # below the cross-attention window
    assert call(good, o=short, sn=[N], sl=[S + 16]) == L.RR_ERR_BAD_SHAPE                # above the padded length
    torch.cuda.synchronize()
    assert all((t == -3).all().item() for t in outs)
    assert call(good) == 0                                             # the same buffers, a good call
    torch.cuda.synchronize()
    assert not (outs[0] == -3).any().item()


def test_forward_joint_tokens_packed_equals_the_drop_in(hf):
    from rmr_amd.pipeline import joint_compact_batch
    m_pk, cfg = _model(hf, packed=True)
    m_pad, _ = _model(hf, packed=False)
    K, ql, instr = 30, 16, 777
    batch = _queries(3, K, ql, 9, cfg, instr=instr)
    for m in (m_pk, m_pad):
        m.instruction_token_id = instr
    q_ids, q_am, c_ids, c_am = _padded(hf, batch, K)
    cls, pat = m_pk.engine.encode_image(torch.stack([q["pixel_values"] for q in batch]).cuda())
    ref = m_pk(q_ids, q_am, None, c_ids, c_am, K - 1, image_features=(cls, pat), want_order=True)
    pad = m_pad(q_ids, q_am, None, c_ids, c_am, K - 1, image_features=(cls, pat), want_order=True)
    pool, desc = joint_compact_batch(m_pk.native_tokenizer, batch, [d["content"] for q in batch for d in q["retrieved_docs"]], K,
                                     ql, S)
    got = m_pk.engine.forward_joint_tokens_packed(pool.cuda(), desc, len(batch), K, ql, cls, pat, instr, want_order=True,
                                                  padded_len=S, special_ids=m_pk.native_tokenizer.special_ids)
    torch.cuda.synchronize()
    assert got["packed_segments"] > 1
    assert torch.equal(got["logits"].view(-1, 1), ref.logits)
    assert torch.equal(got["logits2"], ref.logits2) and torch.equal(got["order"], ref.order)
    assert got["loss"].item() == ref.loss.item()
    d = (got["logits"].view(-1, 1) - pad.logits).abs().max().item()
    print(f"forward_joint_tokens_packed vs the padded RerankModel.forward: |dlogit| {d:.2e}")
    assert d <= 1e-3
    with pytest.raises(NotImplementedError):
        m_pk.engine.forward_joint_tokens_packed(pool.cuda(), desc, len(batch), K, ql, None, None, padded_len=S)


def _serial(m, hf, K):
    from rmr_amd import rank_descending_stable

    def fwd(batch):
        q_ids, q_am, c_ids, c_am = _padded(hf, batch, K)
        px = torch.stack([q["pixel_values"] for q in batch]) if all("pixel_values" in q for q in batch) else None
        r = m(q_ids, q_am, px, c_ids, c_am, K - 1)
        logits = r.logits.view(len(batch), K).tolist()
        return {"logits": logits, "order": [rank_descending_stable(x) for x in logits], "loss": r.loss.item()}
    return fwd


@pytest.mark.parametrize("vit,instr,K,n,B", [(True, None, 100, 7, 3), (False, 777, 1, 10, 4), (True, 777, 6, 9, 2),
                                             (False, None, 12, 5, 5)])
def test_pipelined_joint_loop_equals_the_serial_loop(hf, tmp_path, vit, instr, K, n, B):
    import rmr_amd
    m, cfg = _model(hf, packed=True, vit=vit, instr=instr)
    qs = _queries(n, K, 16, 100 + K, cfg, instr=instr)
    Ks = sorted({1, min(5, K), K})
    want = rmr_amd.rerank_dataset(qs, _serial(m, hf, K), B, Ks, docs_to_rerank=K)
    before = set(threading.enumerate())
    stats = {}
    got = rmr_amd.rerank_dataset_pipelined(qs, m, B, Ks, docs_to_rerank=K, out_path=str(tmp_path / "pred.json"), stats=stats)
    assert set(threading.enumerate()) == before
    assert stats["batches"] == -(-n // B) and len(got["output"]) == n
    assert json.dumps(got["output"]) == json.dumps(want["output"])
    assert got["metrics"] == want["metrics"]
    assert json.load(open(tmp_path / "pred.json")) == {"output": want["output"]}


def test_pipelined_joint_loop_raises_like_the_serial_loop(hf):
    import rmr_amd
    m, cfg = _model(hf, packed=True)
    K = 5
    qs = _queries(12, K, 16, 3, cfg)
    qs[9]["retrieved_docs"] = qs[9]["retrieved_docs"][:-1]               # batch 4 (of 2 queries) has a query with K - 1 docs
    with pytest.raises(AssertionError):
        rmr_amd.rerank_dataset(qs, _serial(m, hf, K), 2, [K], docs_to_rerank=K)
    before = set(threading.enumerate())
    with pytest.raises(AssertionError):
        rmr_amd.rerank_dataset_pipelined(qs, m, 2, [K], docs_to_rerank=K)
    assert set(threading.enumerate()) == before
    qs = _queries(6, K, 16, 4, cfg)
    del qs[3]["pixel_values"]                                            # text_only (rerank_model.py:184-185)
    with pytest.raises(NotImplementedError):
        rmr_amd.rerank_dataset(qs, _serial(m, hf, K), 2, [K], docs_to_rerank=K)
    with pytest.raises(NotImplementedError):
        rmr_amd.rerank_dataset_pipelined(qs, m, 2, [K], docs_to_rerank=K)
    assert set(threading.enumerate()) == before
    # the handle is fine afterwards
    out = rmr_amd.rerank_dataset_pipelined(qs[:2], m, 2, [K], docs_to_rerank=K)
    assert len(out["output"]) == 2
