"""CPU: the joint family's compact inputs.  rr_tok_prepare_contexts_compact plus the FLMR post-processing equals the reference's
context encoding (HF BertTokenizer on ". " + text, ids[:, 1] = [unused1]); the compact batch of JointStages, expanded on the host
as rr_assemble_joint expands it, equals the joint rows RerankModel.forward builds with cat(q, ctx[:, 2 : 2 - ql]), padded and
packed; the pool-size report; and rerank_dataset_pipelined's ordering and failure logic through JointStages with a fake device."""
import ctypes as C
import os
import random
import threading

import numpy as np
import pytest
import torch

from helpers import ROOT  # noqa: F401  (puts the repo root on sys.path)
from test_pair_tokenizer_cpu import corpus, make_vocab


def _hf(tmp_path, vocab):
    from transformers import BertTokenizer
    f = os.path.join(tmp_path, "vocab.txt")
    with open(f, "w", encoding="utf-8") as fh:
        fh.write("\n".join(vocab) + "\n")
    return BertTokenizer(f, do_lower_case=True)


def reference_contexts(hf, texts, S):
    """FLMRContextEncoderTokenizer.__call__ (tokenization_flmr.py:120-150) as tokenize_retrieved_docs calls it."""
    enc = hf([". " + t for t in texts], padding="max_length", max_length=S, truncation=True, return_tensors="pt")
    ids = enc["input_ids"].clone()
    ids[:, 1] = hf.convert_tokens_to_ids("[unused1]")
    return ids.long(), enc["attention_mask"].long()


def expand_contexts(pool, offsets, lengths, S, cls, d_marker, sep, pad):
    pool = np.asarray(pool)
    ids, am = [], []
    for o, m in zip(offsets.tolist(), lengths.tolist()):
        row = [cls, d_marker] + pool[o:o + m].tolist() + [sep]
        assert len(row) <= S
        ids.append(row + [pad] * (S - len(row)))
        am.append([1] * len(row) + [0] * (S - len(row)))
    return torch.tensor(ids, dtype=torch.int64), torch.tensor(am, dtype=torch.int64)


def expand_joint(pool, desc, order, seg_n, seg_len, ql, S, sep, pad):
    """Host restatement of rr_assemble_joint: the packed joint (ids, mask) rows from the compact form."""
    pool = np.asarray(pool)
    ids, am = [], []
    i = 0
    for n, L in zip(seg_n, seg_len):
        for p in order[i:i + n]:
            qo, co, m = (int(x) for x in desc[p])
            ctx = pool[co:co + m].tolist() + [sep] + [pad] * S
            cm = [1] * (m + 1) + [0] * S
            row = pool[qo:qo + ql].tolist() + ctx[:S - ql]
            mask = pool[qo + ql:qo + 2 * ql].tolist() + cm[:S - ql]
            assert ql + min(m + 1, S - ql) <= L
            ids += row[:L]
            am += mask[:L]
        i += n
    return torch.tensor(ids, dtype=torch.int64), torch.tensor(am, dtype=torch.int64)


def lengths_of(ids, am):
    used = (ids != 0) | (am != 0)
    return (used * torch.arange(1, ids.shape[1] + 1)).amax(1).clamp(min=1)


@pytest.fixture(scope="module")
def native():
    from rmr_amd.pair_inputs import NativePairTokenizer
    return NativePairTokenizer(make_vocab(), do_lower_case=True, n_threads=4)


def test_context_encoding_equals_the_flmr_context_tokenizer(native, tmp_path):
    from rmr_amd.pair_inputs import flmr_context_inputs
    hf = _hf(tmp_path, make_vocab())
    S = 512
    # the unicode corpus (without the final sigma and NUL, where the installed Rust tokenizer and the pinned slow one part)
    texts = corpus(60, seed=11, avoid=("Σ", "\x00"))
    for n in (0, 508, 509, 510, 1100):                            # exact token counts around the cut, and far over it
        texts.append(" ".join(random.Random(n).choice(["bus", "red", "city", "street", "london"]) for _ in range(n)))
    texts += ["", ".", "[SEP] bus", "  leading spaces", "́accent first"]
    pool, off, ln = native.prepare_contexts_compact(texts, S - 3, pin_memory=False)
    assert pool.dtype == torch.int32 and off.dtype == np.int32 and ln.dtype == np.int32
    assert [int(x) for x in ln[60:65]] == [0, 508, 509, 509, 509]
    vocab = make_vocab()
    idx = {t: i for i, t in enumerate(vocab)}
    got = expand_contexts(pool, off, ln, S, idx["[CLS]"], idx["[unused1]"], idx["[SEP]"], idx["[PAD]"])
    want = reference_contexts(hf, texts, S)
    for i in range(len(texts)):
        assert torch.equal(got[0][i], want[0][i]), (i, texts[i][:80])
        assert torch.equal(got[1][i], want[1][i]), i
    lib = flmr_context_inputs(texts, hf, S)
    assert torch.equal(lib["input_ids"], want[0]) and torch.equal(lib["attention_mask"], want[1])
    # every run is stored once, back to back, in context order
    assert off[0] == 0 and (off[1:] == off[:-1] + ln[:-1]).all() and pool.numel() == int(ln.sum())


def _joint_queries(n, K, ql, vocab, seed):
    rng = random.Random(seed)
    words = [w for w in vocab if w.isalpha() and w.islower()]
    out = []
    for i in range(n):
        real = rng.randint(3, ql)
        q_ids = [101] + [rng.randint(110, len(vocab) - 1) for _ in range(real - 2)] + [102] + [0] * (ql - real)
        q_am = [1] * real + [0] * (ql - real)
        docs = [{"passage_id": f"p{i}_{k}", "content": " ".join(rng.choice(words) for _ in range(rng.choice([0, 3, 40, 200, 600])))}
                for k in range(K)]
        out.append({"question_id": f"q{i}", "query_input_ids": torch.tensor(q_ids), "query_attention_mask": torch.tensor(q_am),
                    "retrieved_docs": docs, "pos_item_ids": [docs[0]["passage_id"]], "pixel_values": torch.zeros(3, 4, 4)})
    return out


def _padded_joint(hf, batch, K, ql, S):
    """RerankModel.forward's joint rows (rerank_model.py:191-222) on the reference's padded inputs."""
    ids, am = reference_contexts(hf, [d["content"] for q in batch for d in q["retrieved_docs"]], S)
    q_ids = torch.stack([q["query_input_ids"] for q in batch]).repeat_interleave(K, 0)
    q_am = torch.stack([q["query_attention_mask"] for q in batch]).repeat_interleave(K, 0)
    return torch.cat([q_ids, ids[:, 2:2 - ql]], 1), torch.cat([q_am, am[:, 2:2 - ql]], 1)


@pytest.mark.parametrize("ql", [16, 32])
def test_joint_descriptors_expand_to_the_reference_rows(native, tmp_path, ql):
    from rmr_amd.pair_inputs import group_pairs_by_length, pack_rows
    from rmr_amd.pipeline import joint_compact_batch
    vocab = make_vocab()
    hf = _hf(tmp_path, vocab)
    S, K = 512, 7
    batch = _joint_queries(4, K, ql, vocab, seed=ql)
    contexts = [d["content"] for q in batch for d in q["retrieved_docs"]]
    pool, desc = joint_compact_batch(native, batch, contexts, K, ql, S)
    assert desc.shape == (4 * K, 3) and desc.dtype == np.int32
    want_ids, want_am = _padded_joint(hf, batch, K, ql, S)
    idx = {t: i for i, t in enumerate(vocab)}
    sep, pad = idx["[SEP]"], idx["[PAD]"]
    N = 4 * K
    got = expand_joint(pool, desc, np.arange(N), [N], [S], ql, S, sep, pad)
    assert torch.equal(got[0], want_ids.reshape(-1)) and torch.equal(got[1], want_am.reshape(-1))
    # the descriptors' lengths are the ones forward_joint_packed derives from the padded rows
    lengths = ql + np.minimum(desc[:, 2].astype(np.int64) + 1, S - ql)
    assert lengths.tolist() == lengths_of(want_ids, want_am).tolist()
    assert (lengths == S).any() and (lengths < S).any()         # some passages fill the window and lose their [SEP]
    for granule, cost in ((16, 0), (16, 4096), (1, 0)):
        order, seg_n, seg_len = group_pairs_by_length(lengths, S, granule, max(ql + 1, 32), cost)
        got = expand_joint(pool, desc, order, seg_n, seg_len, ql, S, sep, pad)
        o = torch.from_numpy(order)
        assert torch.equal(got[0], pack_rows(want_ids, o, seg_n, seg_len).reshape(-1)), (granule, cost)
        assert torch.equal(got[1], pack_rows(want_am, o, seg_n, seg_len).reshape(-1)), (granule, cost)


def test_contexts_compact_reports_the_pool_size_it_needs(native):
    from rmr_amd import _lib as L
    texts = corpus(9, seed=2, avoid=("\x00",)) + ["bus " * 700]
    pool, off, ln = native.prepare_contexts_compact(texts, 509, pin_memory=False)
    need = pool.numel()
    arr = (C.c_char_p * len(texts))(*[t.encode() for t in texts])
    small = torch.full((need - 1,), -7, dtype=torch.int32)
    o, n = np.full(len(texts), -7, dtype=np.int32), np.full(len(texts), -7, dtype=np.int32)
    got = C.c_int64(0)
    rc = native.lib.rr_tok_prepare_contexts_compact(native.h, arr, len(texts), 509, 2, small.data_ptr(), small.numel(),
                                                    C.byref(got), o.ctypes.data, n.ctypes.data)
    assert rc == L.RR_ERR_BAD_SHAPE and got.value == need
    assert (small == -7).all() and (o == -7).all() and (n == -7).all()      # nothing written
    exact = torch.empty(need, dtype=torch.int32)
    rc = native.lib.rr_tok_prepare_contexts_compact(native.h, arr, len(texts), 509, 2, exact.data_ptr(), exact.numel(),
                                                    C.byref(got), o.ctypes.data, n.ctypes.data)
    assert rc == 0 and torch.equal(exact, pool) and (o == off).all() and (n == ln).all()
    assert int(ln[-1]) == 509
    # the Python binding grows a buffer that is too small and tokenises again
    p2, o2, n2 = native.prepare_contexts_compact(texts, 509, out=torch.empty(3, dtype=torch.int32), pin_memory=False)
    assert torch.equal(p2, pool) and (o2 == off).all() and (n2 == ln).all()
    assert native.lib.rr_tok_prepare_contexts_compact(native.h, arr, 0, 509, 2, exact.data_ptr(), exact.numel(), C.byref(got),
                                                      o.ctypes.data, n.ctypes.data) == L.RR_ERR_BAD_SHAPE


# ---- the loop through JointStages, with a fake device --------------------------------------------------------------------

class _Engine:
    device = torch.device("cpu")
    arch = {"loss_fn": "2H_BCE"}


class _Model:
    """What JointStages reads of a RerankModel, without a device."""

    def __init__(self, tok, S):
        self.engine, self.native_tokenizer, self.decoder_tokenizer = _Engine(), tok, None
        self.max_decoder_source_length, self.instruction_token_id, self.image_feature_fn = S, None, None


def _fake_logits(ids, am, n, K):
    w = torch.arange(1, ids.shape[1] + 1, dtype=torch.float64)
    return (((ids.double() * w).sum(1) + am.double().sum(1)) % 1009 / 1009.0).reshape(n, K).tolist()


def _fake_forward(rows_of):
    from rmr_amd import rank_descending_stable

    def fwd(batch, rows):
        logits = _fake_logits(*rows, len(batch), len(batch[0]["retrieved_docs"]))
        return {"logits": logits, "order": [rank_descending_stable(r) for r in logits], "loss": sum(map(sum, logits))}
    return fwd


def _joint_stages(tok, K, S, first, fail_at=None):
    from rmr_amd.pipeline import JointStages
    idx = {t: i for i, t in enumerate(tok.vocab)}
    fwd = _fake_forward(None)

    class FakeJointStages(JointStages):
        """The real JointStages host side (prepare: tokenisation and the compact batch); the device replaced by a host
        expansion of the descriptors (what rr_assemble_joint writes) and a fake forward over the rows."""
        events = []

        def new_slot(self):
            return super().new_slot(pin_memory=False)

        def submit(self, batch, item):
            if fail_at is not None and len(self.events) == fail_at:
                raise RuntimeError("fake forward failure")
            N = item["n"] * self.K
            ids, am = expand_joint(item["pool"], item["desc"], np.arange(N), [N], [self.S], self.ql, self.S, idx["[SEP]"],
                                   idx["[PAD]"])
            self.events.append(("submit", len(self.events)))
            return fwd(batch, (ids.view(N, self.S), am.view(N, self.S)))

        def release(self, pending):
            pass

        def collect(self, pending):
            return pending["logits"], pending["order"], pending["loss"]

    return FakeJointStages(_Model(tok, S), 3, K, first)


def test_joint_stages_loop_equals_the_serial_loop(native, tmp_path):
    import json
    from rmr_amd import rerank_dataset, rerank_dataset_pipelined
    vocab = make_vocab()
    hf = _hf(tmp_path, vocab)
    K, S, ql, Ks = 6, 512, 16, [1, 3, 6]
    qs = _joint_queries(11, K, ql, vocab, seed=5)                 # 3 full batches of 3 and a partial one of 2
    fwd = _fake_forward(None)
    want = rerank_dataset(qs, lambda b: fwd(b, _padded_joint(hf, b, K, ql, S)), 3, Ks, docs_to_rerank=K)
    before = set(threading.enumerate())
    st = _joint_stages(native, K, S, qs[0])
    stats = {}
    got = rerank_dataset_pipelined(qs, None, 3, Ks, docs_to_rerank=K, stages=st, stats=stats)
    assert set(threading.enumerate()) == before
    assert stats["batches"] == 4 and len(got["output"]) == 11
    assert json.dumps(got) == json.dumps(want)


def test_joint_stages_failures_reach_the_caller(native):
    from rmr_amd import rerank_dataset_pipelined
    vocab = make_vocab()
    K, S, ql = 4, 512, 16
    before = set(threading.enumerate())
    qs = _joint_queries(10, K, ql, vocab, seed=8)
    qs[7]["retrieved_docs"] = qs[7]["retrieved_docs"][:-1]        # a wrong doc count in batch 2
    with pytest.raises(AssertionError):
        rerank_dataset_pipelined(qs, None, 3, [K], stages=_joint_stages(native, K, S, qs[0]))
    qs = _joint_queries(10, K, ql, vocab, seed=8)
    del qs[4]["pixel_values"]                                     # text_only: not implemented, as RerankModel.forward
    with pytest.raises(NotImplementedError):
        rerank_dataset_pipelined(qs, None, 3, [K], stages=_joint_stages(native, K, S, qs[0]))
    qs = _joint_queries(10, K, ql, vocab, seed=8)
    with pytest.raises(RuntimeError, match="fake"):
        rerank_dataset_pipelined(qs, None, 3, [K], stages=_joint_stages(native, K, S, qs[0], fail_at=2))
    qs[2]["query_input_ids"] = qs[2]["query_input_ids"][:-1]      # a query of another length
    with pytest.raises(AssertionError):
        rerank_dataset_pipelined(qs, None, 3, [K], stages=_joint_stages(native, K, S, qs[0]))
    assert set(threading.enumerate()) == before
