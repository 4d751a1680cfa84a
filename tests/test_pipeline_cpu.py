"""CPU: the compact pair tokenisation (rr_tok_prepare_compact) expanded on the host equals rr_tok_prepare_pairs bit for bit, in
the padded layout and in packed segment tables; and the ordering / failure logic of rerank_dataset_pipelined, driven by a fake
device stage, gives rerank_dataset's records and metrics."""
import ctypes as C
import random
import threading

import numpy as np
import pytest
import torch

from helpers import ROOT  # noqa: F401  (puts the repo root on sys.path)
from test_pair_tokenizer_cpu import corpus, make_vocab


def bench_vocab():
    """The synthetic WordPiece vocabulary of tools/bench_tokenizer.py."""
    rng = random.Random(0)
    syll = ["ka", "to", "mi", "ra", "ne", "so", "lu", "vi", "en", "or", "th", "st", "ing", "ed", "er", "al", "pre", "con"]
    words = sorted({"".join(rng.choice(syll) for _ in range(rng.randint(1, 3))) for _ in range(4000)})
    vocab = ["[PAD]"] + [f"[unused{i}]" for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"] + words + \
        ["##" + s for s in syll] + list(".,?!'-")
    text = lambda n: " ".join(rng.choice(words) + rng.choice(["", "", "", ",", "."]) for _ in range(n))
    return vocab, text


def expand(pool, desc, order, seg_n, seg_len, special):
    """Host restatement of rr_assemble_pairs: the packed (ids, mask, types) rows from the compact form."""
    cls, sep, pad = special
    pool = np.asarray(pool)
    ids, am, tt = [], [], []
    i = 0
    for n, S in zip(seg_n, seg_len):
        for p in order[i:i + n]:
            qo, la, co, lb = (int(x) for x in desc[p])
            row = [cls] + pool[qo:qo + la].tolist() + [sep] + pool[co:co + lb].tolist() + [sep]
            typ = [0] * (la + 2) + [1] * (lb + 1)
            assert len(row) <= S
            ids += row + [pad] * (S - len(row))
            am += [1] * len(row) + [0] * (S - len(row))
            tt += typ + [0] * (S - len(row))
        i += n
    return [torch.tensor(x, dtype=torch.int64) for x in (ids, am, tt)]


def check_equal(tok, q, c, mq, mc, L, K, granules=(16,)):
    from rmr_amd.pair_inputs import group_pairs_by_length, pack_rows
    want = tok.prepare_full_context_inputs(q, c, mq, mc, L, K)
    pool, desc, lengths = tok.prepare_compact(q, c, mq, mc, L, K, pin_memory=False)
    N = len(c)
    assert desc.shape == (N, 4) and desc.dtype == np.int32 and pool.dtype == torch.int32
    # the compact lengths are the padded rows' lengths
    used = (want["input_ids"] != 0) | (want["attention_mask"] != 0)
    assert lengths.tolist() == (used * torch.arange(1, L + 1)).amax(1).tolist()
    # padded layout: one segment of length L, identity order
    got = expand(pool, desc, np.arange(N), [N], [L], tok.special_ids)
    for g, k in zip(got, ("input_ids", "attention_mask", "token_type_ids")):
        assert torch.equal(g, want[k].reshape(-1)), k
    # packed segment tables, as forward_ids_packed builds them
    for granule in granules:
        for cost in (0, 4096):
            order, seg_n, seg_len = group_pairs_by_length(lengths, L, granule, 1, cost)
            got = expand(pool, desc, order, seg_n, seg_len, tok.special_ids)
            o = torch.from_numpy(order)
            for g, k in zip(got, ("input_ids", "attention_mask", "token_type_ids")):
                assert torch.equal(g, pack_rows(want[k], o, seg_n, seg_len).reshape(-1)), (k, granule, cost)
    return pool, desc


@pytest.fixture(scope="module")
def native():
    from rmr_amd.pair_inputs import NativePairTokenizer
    return NativePairTokenizer(make_vocab(), do_lower_case=True, n_threads=4)


def test_compact_equals_padded_on_unicode_corpus(native):
    nq, K = 5, 7
    q = [t.replace("\x00", "") for t in corpus(nq, seed=3)]
    c = [t.replace("\x00", "") for t in corpus(nq * K, seed=4)]
    c[3] = ""                                                     # an empty context
    for (mq, mc, L) in [(8, 20, 32), (32, 476, 512), (0, 3, 8), (4, 0, 16)]:
        check_equal(native, q, c, mq, mc, L, K, granules=(1, 16))


def test_compact_equals_padded_on_bench_vocabulary():
    from rmr_amd.pair_inputs import NativePairTokenizer
    vocab, text = bench_vocab()
    tok = NativePairTokenizer(vocab, n_threads=3)
    nq, K = 3, 20
    q = [text(12) + "?", text(60) + "?", text(5)]                 # the second query is over 32 tokens
    c = [text(random.Random(i).randint(0, 400)) for i in range(nq * K)]
    c[7] = ""
    assert len(tok.encode(q[1])) > 32
    check_equal(tok, q, c, 32, 476, 512, K, granules=(16, 64))
    check_equal(tok, q, c, 64, 476, 512, K)                       # the long query kept whole
    # max_length so small that LONGEST_FIRST cuts the query as well as the contexts
    pool, desc = check_equal(tok, q, c, 64, 476, 24, K)
    full_q = tok.prepare_compact(q, c, 64, 476, 512, K, pin_memory=False)[1][K, 1]
    assert desc[K, 1] < full_q and (desc[:, 1] + desc[:, 3] + 3 <= 24).all()


def test_compact_reports_the_pool_size_it_needs():
    from rmr_amd import _lib as L
    from rmr_amd.pair_inputs import NativePairTokenizer
    vocab, text = bench_vocab()
    tok = NativePairTokenizer(vocab, n_threads=2)
    nq, K = 2, 4
    q, c = [text(10), text(3)], [text(50 + 20 * i) for i in range(nq * K)]
    pool, desc, _ = tok.prepare_compact(q, c, 32, 476, 512, K, pin_memory=False)
    need = pool.numel()
    qa = (C.c_char_p * nq)(*[t.encode() for t in q])
    ca = (C.c_char_p * (nq * K))(*[t.encode() for t in c])
    small = torch.full((need - 1,), -7, dtype=torch.int32)
    d = np.full((nq * K, 4), -7, dtype=np.int32)
    got = C.c_int64(0)
    rc = tok.lib.rr_tok_prepare_compact(tok.h, qa, nq, ca, K, 32, 476, 512, 2, small.data_ptr(), small.numel(), C.byref(got),
                                        d.ctypes.data)
    assert rc == L.RR_ERR_BAD_SHAPE and got.value == need
    assert (small == -7).all() and (d == -7).all()                # nothing written
    exact = torch.empty(need, dtype=torch.int32)
    rc = tok.lib.rr_tok_prepare_compact(tok.h, qa, nq, ca, K, 32, 476, 512, 2, exact.data_ptr(), exact.numel(), C.byref(got),
                                        d.ctypes.data)
    assert rc == 0 and torch.equal(exact, pool) and (d == desc).all()
    # the Python binding grows a buffer that is too small and tokenises again
    p2, d2, _ = tok.prepare_compact(q, c, 32, 476, 512, K, out=torch.empty(3, dtype=torch.int32), pin_memory=False)
    assert torch.equal(p2, pool) and (d2 == desc).all()


def test_host_threads_follow_affinity_and_omp(monkeypatch):
    import os
    from rmr_amd.pair_inputs import host_threads
    n = len(os.sched_getaffinity(0))
    monkeypatch.setenv("OMP_NUM_THREADS", "1")
    assert host_threads() == 1
    monkeypatch.delenv("OMP_NUM_THREADS")
    assert host_threads() == n


# ---- the loop, with a fake device stage --------------------------------------------------------------------------------

def make_queries(n, K, seed=0):
    rng = random.Random(seed)
    out = []
    for i in range(n):
        docs = [{"passage_id": f"p{i}_{k}", "content": f"doc {k} of {i}"} for k in range(K)]
        out.append({"question_id": f"q{i}", "question": f"question {i}", "retrieved_docs": docs,
                    "pos_item_ids": [d["passage_id"] for d in rng.sample(docs, 2)], "neg_item_ids": []})
    return out


def fake_logit(q, d):
    return float((hash((q["question_id"], d["passage_id"])) % 1000) / 997.0 - 0.5)


class FakeStages:
    """Host-only stand-in for DeviceStages: logits from the ids, an optional failure at a given batch and stage."""

    def __init__(self, K, fail_at=None, fail_in="submit"):
        self.K, self.fail_at, self.fail_in = K, fail_at, fail_in
        self.prepared = self.submitted = self.collected = 0
        self.events = []

    def new_slot(self):
        return {"id": object()}

    def prepare(self, batch, slot):
        if self.fail_in == "prepare" and self.prepared == self.fail_at:
            raise AssertionError("fake tokenizer failure")
        for q in batch:
            assert len(q["retrieved_docs"]) == self.K
        self.prepared += 1
        return [[fake_logit(q, d) for d in q["retrieved_docs"]] for q in batch]

    def submit(self, batch, item):
        if self.fail_in == "submit" and self.submitted == self.fail_at:
            raise RuntimeError("fake forward failure")
        self.events.append(("submit", self.submitted))
        self.submitted += 1
        from rmr_amd import rank_descending_stable
        return {"logits": item, "order": [rank_descending_stable(r) for r in item], "loss": 0.25 * len(item), "i": self.submitted - 1}

    def release(self, pending):
        pass

    def collect(self, pending):
        self.events.append(("collect", pending["i"]))
        self.collected += 1
        return pending["logits"], pending["order"], pending["loss"]


def serial(queries, K, Ks):
    from rmr_amd import rank_descending_stable, rerank_dataset

    def fwd(batch):
        logits = [[fake_logit(q, d) for d in q["retrieved_docs"]] for q in batch]
        return {"logits": logits, "order": [rank_descending_stable(r) for r in logits], "loss": 0.25 * len(batch)}
    return rerank_dataset(queries, fwd, 4, Ks, docs_to_rerank=K)


def test_fake_loop_equals_serial_and_flushes_the_last_batch(tmp_path):
    import json
    from rmr_amd import rerank_dataset_pipelined
    K, Ks = 10, [1, 5, 10]
    qs = make_queries(22, K)                                      # 5 full batches of 4 and a partial one of 2
    st = FakeStages(K)
    stats = {}
    got = rerank_dataset_pipelined(iter(qs), None, 4, Ks, docs_to_rerank=K, out_path=str(tmp_path / "p.json"), stages=st,
                                   stats=stats)
    want = serial(qs, K, Ks)
    assert json.dumps(got) == json.dumps(want)
    assert len(got["output"]) == 22 and st.submitted == st.collected == 6 and stats["batches"] == 6
    # batch i - 1's records are built after batch i has been submitted
    assert st.events[:4] == [("submit", 0), ("submit", 1), ("collect", 0), ("submit", 2)]
    assert json.load(open(tmp_path / "p.json")) == {"output": want["output"]}
    assert rerank_dataset_pipelined([], None, 4, Ks, stages=st)["output"] == []


@pytest.mark.parametrize("fail_in", ["submit", "prepare"])
def test_fake_loop_failure_reaches_the_caller_and_leaves_no_thread(fail_in):
    from rmr_amd import rerank_dataset_pipelined
    K = 6
    before = set(threading.enumerate())
    st = FakeStages(K, fail_at=3, fail_in=fail_in)
    exc = RuntimeError if fail_in == "submit" else AssertionError
    with pytest.raises(exc, match="fake"):
        rerank_dataset_pipelined(make_queries(40, K), None, 4, [K], stages=st)
    assert set(threading.enumerate()) == before
    assert not [t for t in threading.enumerate() if t.name == "rmr_amd-tokenize"]


def test_fake_loop_wrong_doc_count_raises_like_the_serial_loop():
    from rmr_amd import rerank_dataset_pipelined
    K = 5
    qs = make_queries(9, K)
    qs[6]["retrieved_docs"] = qs[6]["retrieved_docs"][:-1]
    before = set(threading.enumerate())
    with pytest.raises(AssertionError):
        rerank_dataset_pipelined(qs, None, 2, [K], stages=FakeStages(K))
    assert set(threading.enumerate()) == before
