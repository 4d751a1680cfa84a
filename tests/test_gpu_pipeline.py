"""GPU: rr_assemble_pairs (the pair rows built on the device from compact tokens) against rr_tok_prepare_pairs + pack_rows,
its refusal of bad descriptors, RerankEngine.forward_tokens_packed against FullContextRerankModel.forward with the native
tokenizer and packed rows, and rerank_dataset_pipelined against rerank_dataset driven by that forward."""
import ctypes as C
import json
import random
import threading

import numpy as np
import pytest
import torch

from helpers import arch_from_cfg, load_golden
from oracle import rerank_oracle as O
from test_pipeline_cpu import bench_vocab

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    import rmr_amd
    g = load_golden("tiny")
    eng = rmr_amd.RerankEngine(arch_from_cfg(g["cfg"], False))
    eng.load_state_dict(O.make_weights(g["cfg"], 0, False))
    return eng


@pytest.fixture(scope="module")
def compact():
    from rmr_amd.pair_inputs import NativePairTokenizer
    vocab, text = bench_vocab()
    tok = NativePairTokenizer(vocab, n_threads=4)
    rng = random.Random(5)
    nq, K, S = 4, 40, 512
    q = [text(rng.randint(3, 40)) + "?" for _ in range(nq)]
    c = [text(rng.randint(0, 420)) for _ in range(nq * K)]
    c[5] = ""
    padded = tok.prepare_full_context_inputs(q, c, 32, S - 36, S, K)
    pool, desc, lengths = tok.prepare_compact(q, c, 32, S - 36, S, K)
    return dict(tok=tok, padded=padded, pool=pool, desc=desc, lengths=lengths, N=nq * K, S=S, K=K, q=q, c=c)


def _tables(case, lengths, S):
    from rmr_amd.pair_inputs import group_pairs_by_length
    N = len(lengths)
    if case == "padded":
        return np.arange(N), [N], [S]
    if case == "granule16":
        return group_pairs_by_length(lengths, S, 16)
    if case == "merged":
        return group_pairs_by_length(lengths, S, 16, 1, 4096)
    if case == "single":
        order = np.argsort(lengths, kind="stable")
        return order, [N], [int(lengths.max())]
    if case in ("max64", "exact"):                 # 64 segments (the maximum), each as long as its longest pair exactly
        order = np.argsort(lengths, kind="stable")
        parts = np.array_split(order, 64 if case == "max64" else 8)
        return order, [len(p) for p in parts], [int(lengths[p].max()) for p in parts]
    raise ValueError(case)


@pytest.mark.parametrize("case", ["padded", "granule16", "merged", "single", "max64", "exact"])
def test_assembly_equals_tokenizer_rows_packed(engine, compact, case):
    from rmr_amd.pair_inputs import pack_rows
    tok, S = compact["tok"], compact["S"]
    order, seg_n, seg_len = _tables(case, compact["lengths"], S)
    if case == "max64":
        assert len(seg_n) == 64
    if case == "exact":
        assert all(int(compact["lengths"][order[sum(seg_n[:s + 1]) - 1]]) == seg_len[s] for s in range(len(seg_n)))
    pool_d = compact["pool"].cuda()
    ids, am, tt = engine.assemble_pairs(pool_d, compact["desc"], order, seg_n, seg_len, tok.special_ids)
    torch.cuda.synchronize()
    o = torch.from_numpy(np.asarray(order, dtype=np.int64))
    for got, k in zip((ids, am, tt), ("input_ids", "attention_mask", "token_type_ids")):
        want = pack_rows(compact["padded"][k], o, seg_n, seg_len).reshape(-1)
        assert torch.equal(got.cpu(), want), (case, k)


def test_assembly_refuses_bad_descriptors_and_writes_nothing(engine, compact):
    from rmr_amd import _lib as L
    tok, S, N = compact["tok"], compact["S"], compact["N"]
    order, seg_n, seg_len = _tables("granule16", compact["lengths"], S)
    pool_d = compact["pool"].cuda()
    rows = sum(n * s for n, s in zip(seg_n, seg_len))
    cls, sep, pad = tok.special_ids
    good = compact["desc"]
    longest = int(np.argmax(compact["lengths"]))
    bad_cases = []
    d = good.copy()
    d[longest, 3] += 16                              # a pair longer than its segment
    bad_cases.append(d)
    d = good.copy()
    d[3, 2] = pool_d.numel() - 1                     # a context run past the end of the pool
    bad_cases.append(d)
    d = good.copy()
    d[7, 0] = pool_d.numel() + 5                     # a query offset past the pool
    bad_cases.append(d)
    d = good.copy()
    d[2, 1] = -1                                     # a negative length
    bad_cases.append(d)
    outs = [torch.full((rows,), -3, dtype=torch.int64, device="cuda") for _ in range(3)]
    sn, sl = (C.c_int32 * len(seg_n))(*seg_n), (C.c_int32 * len(seg_n))(*seg_len)
    o32 = np.ascontiguousarray(order, dtype=np.int32)
    stream = torch.cuda.current_stream().cuda_stream
    for d in bad_cases:
        rc = engine.lib.rr_assemble_pairs(engine.h, pool_d.data_ptr(), pool_d.numel(), d.ctypes.data, N, o32.ctypes.data,
                                          len(seg_n), sn, sl, cls, sep, pad, *[t.data_ptr() for t in outs], stream)
        assert rc == L.RR_ERR_BAD_SHAPE
        with pytest.raises(ValueError):
            engine.assemble_pairs(pool_d, d, order, seg_n, seg_len, tok.special_ids)
    bad_order = o32.copy()
    bad_order[0] = bad_order[1]                      # not a permutation
    rc = engine.lib.rr_assemble_pairs(engine.h, pool_d.data_ptr(), pool_d.numel(), good.ctypes.data, N, bad_order.ctypes.data,
                                      len(seg_n), sn, sl, cls, sep, pad, *[t.data_ptr() for t in outs], stream)
    assert rc == L.RR_ERR_BAD_SHAPE
    torch.cuda.synchronize()
    assert all((t == -3).all().item() for t in outs)
    # the same buffers are written by a good call
    rc = engine.lib.rr_assemble_pairs(engine.h, pool_d.data_ptr(), pool_d.numel(), good.ctypes.data, N, o32.ctypes.data,
                                      len(seg_n), sn, sl, cls, sep, pad, *[t.data_ptr() for t in outs], stream)
    torch.cuda.synchronize()
    assert rc == 0 and not (outs[0] == -3).any().item()


# ---- model level -------------------------------------------------------------------------------------------------------

WORDS = ["what", "is", "the", "color", "of", "this", "bus", "red", "a", "big", "city", "street", "in", "london", "double",
         "decker", "buses", "are", "usually", "image", "query", "train", "station", "river", "bridge", "tower", "old", "new",
         "green", "blue", "park", "museum", "people", "walk", "near", "over", "under", "with", "from", "and"]


def _vocab():
    return ["[PAD]"] + [f"[unused{i}]" for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"] + WORDS + \
        ["##s", "##es", "##ing", "##ed", ".", ",", "?"]


def _hf_tokenizer(tmp_path):
    import os
    from transformers import BertTokenizer
    f = os.path.join(tmp_path, "vocab.txt")
    with open(f, "w") as fh:
        fh.write("\n".join(_vocab()) + "\n")
    return BertTokenizer(f, do_lower_case=True)


def _text(rng, n):
    return " ".join(rng.choice(WORDS) + rng.choice(["", "", "s", "ing", ",", "."]) for _ in range(n))


def _queries(n, K, seed, pixels=None):
    rng = random.Random(seed)
    out = []
    for i in range(n):
        docs = [{"passage_id": f"p{i}_{k}", "content": _text(rng, rng.randint(0, 70))} for k in range(K)]
        q = {"question_id": f"q{i}", "question": _text(rng, rng.randint(2, 12)) + "?", "retrieved_docs": docs,
             "pos_item_ids": [d["passage_id"] for d in rng.sample(docs, 2)], "neg_item_ids": []}
        if pixels is not None:
            q["pixel_values"] = pixels[i]
        out.append(q)
    return out


def _models(tmp_path, vision, loss_fn):
    import rmr_amd
    tok = _hf_tokenizer(tmp_path)
    if vision:
        from test_gpu_vision import _arch, _load
        cfg = _load("vit_tiny")["cfg"]
        w = O.make_weights(cfg, seed=0, vision=True)
        w.update(O.make_vit_weights(cfg, seed=5))
        arch = _arch(cfg, "bf16")
    else:
        cfg = load_golden("tiny")["cfg"]
        w = O.make_weights(cfg, 0, False)
        arch = arch_from_cfg(cfg, False)
    arch["loss_fn"] = loss_fn
    conf = dict(cross_encoder_num_hidden_layers=cfg.ce_layers, cross_encoder_max_position_embeddings=cfg.ce_max_pos,
                loss_fn=loss_fn, pos_weight=None, max_query_length=8, max_decoder_source_length=cfg.max_pos, text_only=not vision,
                arch=arch, tokenizer=tok, native_tokenizer=True, packed_rows=True)
    return rmr_amd.FullContextRerankModel(conf, state_dict=w), cfg


def test_forward_tokens_packed_equals_the_string_forward(tmp_path):
    m, cfg = _models(tmp_path, False, "BCE")
    K = 9
    qs = _queries(3, K, seed=1)
    q = [x["question"] for x in qs]
    c = [d["content"] for x in qs for d in x["retrieved_docs"]]
    labels = [float(i % 3 == 0) for i in range(len(c))]
    ref = m(q, None, c, K - 1, labels=labels)
    tok = m.native_tokenizer
    pool, desc, _ = tok.prepare_compact(q, c, m.max_query_length, m.max_context_length, m.max_decoder_source_length, K)
    got = m.engine.forward_tokens_packed(pool.cuda(), desc, len(q), K, labels=torch.tensor(labels).cuda(), want_order=True,
                                         padded_len=m.max_decoder_source_length, special_ids=tok.special_ids)
    torch.cuda.synchronize()
    assert torch.equal(got["logits"].view(-1, 1), ref.logits)
    assert got["loss"].item() == ref.loss.item()


def test_forward_tokens_packed_with_vision_tokens(tmp_path):
    m, cfg = _models(tmp_path, True, "BCE")
    K = 6
    qs = _queries(2, K, seed=2)
    q = [x["question"] for x in qs]
    c = [d["content"] for x in qs for d in x["retrieved_docs"]]
    px = O.make_pixel_values(cfg, len(q), seed=9)
    ref = m(q, px, c, K - 1)
    cls, pat = m.engine.encode_image(px.cuda())
    tok = m.native_tokenizer
    pool, desc, _ = tok.prepare_compact(q, c, m.max_query_length, m.max_context_length, m.max_decoder_source_length, K)
    got = m.engine.forward_tokens_packed(pool.cuda(), desc, len(q), K, cls, pat, padded_len=m.max_decoder_source_length,
                                         special_ids=tok.special_ids)
    torch.cuda.synchronize()
    d = (got["logits"].view(-1, 1) - ref.logits).abs().max().item()
    print(f"forward_tokens_packed with vision tokens: |dlogit| {d:.2e}")
    assert d < 5e-5


def _serial(m, K):
    from rmr_amd import rank_descending_stable

    def fwd(batch):
        q = [x["question"] for x in batch]
        c = [d["content"] for x in batch for d in x["retrieved_docs"]]
        px = torch.stack([x["pixel_values"] for x in batch]) if "pixel_values" in batch[0] else None
        labels = None
        if m.engine.arch["loss_fn"] != "negative_sampling":
            labels = [1.0 if d["passage_id"] in x["pos_item_ids"] else 0.0 for x in batch for d in x["retrieved_docs"]]
        r = m(q, px, c, K - 1, labels=labels)
        logits = r.logits.view(len(batch), K).tolist()
        return {"logits": logits, "order": [rank_descending_stable(x) for x in logits], "loss": r.loss.item()}
    return fwd


@pytest.mark.parametrize("vision,loss_fn", [(False, "BCE"), (False, "negative_sampling"), (True, "BCE"),
                                            (True, "negative_sampling")])
def test_pipelined_loop_equals_the_serial_loop(tmp_path, vision, loss_fn):
    import rmr_amd
    m, cfg = _models(tmp_path, vision, loss_fn)
    K, B, n = 10, 3, 17                                  # 5 full batches and a partial one
    px = O.make_pixel_values(cfg, n, seed=4) if vision else None
    qs = _queries(n, K, seed=7, pixels=px)
    Ks = [1, 5, 10]
    want = rmr_amd.rerank_dataset(qs, _serial(m, K), B, Ks, docs_to_rerank=K)
    before = set(threading.enumerate())
    stats = {}
    got = rmr_amd.rerank_dataset_pipelined(qs, m, B, Ks, docs_to_rerank=K, out_path=str(tmp_path / "pred.json"), stats=stats)
    assert set(threading.enumerate()) == before
    assert stats["batches"] == 6 and len(got["output"]) == n
    assert json.dumps(got["output"]) == json.dumps(want["output"])
    assert got["metrics"] == want["metrics"]
    assert json.load(open(tmp_path / "pred.json")) == {"output": want["output"]}


def test_pipelined_loop_raises_like_the_serial_loop(tmp_path):
    import rmr_amd
    m, _ = _models(tmp_path, False, "BCE")
    K = 5
    qs = _queries(12, K, seed=3)
    qs[9]["retrieved_docs"] = qs[9]["retrieved_docs"][:-1]          # batch 3 (of 2 queries) has a query with K - 1 docs
    with pytest.raises(AssertionError):
        rmr_amd.rerank_dataset(qs, _serial(m, K), 2, [K], docs_to_rerank=K)
    before = set(threading.enumerate())
    with pytest.raises(AssertionError):
        rmr_amd.rerank_dataset_pipelined(qs, m, 2, [K], docs_to_rerank=K)
    assert set(threading.enumerate()) == before
    # the handle is fine afterwards
    out = rmr_amd.rerank_dataset_pipelined(qs[:4], m, 2, [K], docs_to_rerank=K)
    assert len(out["output"]) == 4
