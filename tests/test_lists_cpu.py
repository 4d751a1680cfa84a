"""CPU: lists of unequal length in one batch.  The C ABI of rr_head_lists (header, library, ctypes table agree), and the ordering /
failure logic of rerank_dataset_pipelined(ragged=True) driven by a device-free stages object: records, their order, the ranked
passage ids and the metrics are those of the serial loop run one query per forward, which is what the reference executor does
(src/executors/Reranker_base_executor.py:807-976 of the reference)."""
import ctypes as C
import json
import os
import random
import re
import threading

import pytest

from helpers import ROOT  # noqa: F401  (puts the repo root on sys.path)

SIZES = [5, 1, 3, 5, 2, 4, 5]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------

def _prototype(name):
    src = open(os.path.join(ROOT, "include", "rerank_mi355.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/rerank_mi355.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def _ctype(decl):
    if "*" in decl or decl.startswith("rr_handle"):
        return C.c_void_p
    return {"int": C.c_int, "float": C.c_float, "int64_t": C.c_int64}[decl.rsplit(" ", 1)[0].replace("const ", "")]


def test_head_lists_is_declared_exported_and_bound():
    import __graft_entry__ as g
    g.build()
    from rmr_amd import _lib
    args = _prototype("rr_head_lists")
    names = [a.rsplit(" ", 1)[1].lstrip("*") for a in args]
    assert names == ["h", "logits", "logits2", "labels", "n_lists", "list_offsets", "gather", "joint", "loss_out", "list_loss_out",
                     "scores_out", "order_out", "hip_stream"]
    assert "rr_head_lists" in _lib.EXPORTED
    res, bound = _lib._SIGS["rr_head_lists"]
    assert res is C.c_int and bound == [_ctype(a) for a in args]
    lib = _lib.load()
    assert hasattr(lib, "rr_head_lists") and lib.rr_head_lists.argtypes == bound
    # a null handle is refused before anything else is looked at
    assert lib.rr_head_lists(None, None, None, None, 1, None, None, 0, None, None, None, None, None) == _lib.RR_ERR_BAD_ARG


# ---- the loop, with a device-free stages object ---------------------------------------------------------------------------

def make_queries(sizes, seed=0):
    rng = random.Random(seed)
    out = []
    for i, k in enumerate(sizes):
        docs = [{"passage_id": f"p{i}_{j}", "content": f"doc {j} of {i}"} for j in range(k)]
        out.append({"question_id": f"q{i}", "question": f"question {i}", "retrieved_docs": docs,
                    "pos_item_ids": [d["passage_id"] for d in rng.sample(docs, min(2, k))], "neg_item_ids": []})
    return out


def fake_logit(q, d):
    x = sum(ord(c) * (i + 1) for i, c in enumerate(q["question_id"] + "|" + d["passage_id"]))
    return float((x * 2654435761 % 1000) // 50) / 7.0 - 1.0           # few distinct values: ties inside a list are common


def fake_loss(q):
    return sum(fake_logit(q, d) for d in q["retrieved_docs"]) / len(q["retrieved_docs"])


class RaggedFakeStages:
    """Host-only stand-in for DeviceStages(ragged=True): logits from the ids, one row and one loss per query, an optional
    failure at a given batch and stage."""

    def __init__(self, most, fail_at=None, fail_in="submit"):
        self.most, self.fail_at, self.fail_in = most, fail_at, fail_in
        self.prepared = self.submitted = self.collected = 0
        self.batch_sizes = []

    def new_slot(self):
        return {"id": object()}

    def prepare(self, batch, slot):
        if self.fail_in == "prepare" and self.prepared == self.fail_at:
            raise AssertionError("fake tokenizer failure")
        for q in batch:
            assert 1 <= len(q["retrieved_docs"]) <= self.most
        self.prepared += 1
        return [[fake_logit(q, d) for d in q["retrieved_docs"]] for q in batch]

    def submit(self, batch, item):
        if self.fail_in == "submit" and self.submitted == self.fail_at:
            raise RuntimeError("fake forward failure")
        self.submitted += 1
        self.batch_sizes.append([len(r) for r in item])
        from rmr_amd import rank_descending_stable
        return {"logits": item, "order": [rank_descending_stable(r) for r in item], "loss": [fake_loss(q) for q in batch]}

    def release(self, pending):
        pass

    def collect(self, pending):
        self.collected += 1
        return pending["logits"], pending["order"], pending["loss"]


def one_query_per_forward(queries, Ks, most=None):
    """The reference executor's loop: one query per forward, its own loss in its record."""
    from rmr_amd import rank_descending_stable, rerank_dataset

    def fwd(batch):
        (q,) = batch
        row = [fake_logit(q, d) for d in q["retrieved_docs"]]
        return {"logits": [row], "order": [rank_descending_stable(row)], "loss": fake_loss(q)}
    return rerank_dataset(queries, fwd, 1, Ks, docs_to_rerank=most, ragged=True)


def test_ragged_fake_loop_equals_one_query_per_forward(tmp_path):
    from rmr_amd import rerank_dataset_pipelined
    Ks = [1, 3, 5]
    qs = make_queries(SIZES)                                        # batches of 3, 3 and a last one of 1
    st = RaggedFakeStages(5)
    stats = {}
    got = rerank_dataset_pipelined(iter(qs), None, 3, Ks, docs_to_rerank=5, out_path=str(tmp_path / "p.json"), stages=st,
                                   stats=stats, ragged=True)
    want = one_query_per_forward(qs, Ks, 5)
    assert json.dumps(got) == json.dumps(want)
    assert [r["question_id"] for r in got["output"]] == [q["question_id"] for q in qs]
    assert [len(r["top_ranking_passages"]) for r in got["output"]] == SIZES
    assert st.batch_sizes == [[5, 1, 3], [5, 2, 4], [5]] and st.submitted == st.collected == 3 and stats["batches"] == 3
    for q, r in zip(qs, got["output"]):                             # the rank, and each record's own loss
        row = [fake_logit(q, d) for d in q["retrieved_docs"]]
        ids = [d["passage_id"] for _, d in sorted(zip(row, q["retrieved_docs"]), key=lambda t: t[0], reverse=True)]
        assert [p["passage_id"] for p in r["top_ranking_passages"]] == ids
        assert r["loss"] == fake_loss(q)
    assert len({r["loss"] for r in got["output"]}) > 1
    assert json.load(open(tmp_path / "p.json")) == {"output": want["output"]}


def test_ragged_loop_cuts_long_lists_and_keeps_the_callers_queries():
    from rmr_amd import rerank_dataset_pipelined
    qs = make_queries([6, 2, 9, 4], seed=1)
    got = rerank_dataset_pipelined(qs, None, 2, [1, 4], docs_to_rerank=4, stages=RaggedFakeStages(4), ragged=True)
    assert [len(r["top_ranking_passages"]) for r in got["output"]] == [4, 2, 4, 4]
    assert [len(r["raw_top_ranking_passages"]) for r in got["output"]] == [4, 2, 4, 4]
    assert [len(q["retrieved_docs"]) for q in qs] == [6, 2, 9, 4]                 # the caller's dicts are untouched
    want = one_query_per_forward(qs, [1, 4], 4)
    assert json.dumps(got) == json.dumps(want)


def test_ragged_serial_loop_takes_flat_outputs():
    """rerank_dataset(ragged=True) with a forward that answers as the drop-in classes do with candidates_per_query: flat
    logits ([N, 1] for the pointwise losses), a flat order local to each list, list_loss."""
    from rmr_amd import rank_descending_stable, rerank_dataset
    qs = make_queries(SIZES, seed=2)

    def fwd(batch):
        rows = [[fake_logit(q, d) for d in q["retrieved_docs"]] for q in batch]
        return {"logits": [[x] for r in rows for x in r], "order": [i for r in rows for i in rank_descending_stable(r)],
                "loss": 0.0, "list_loss": [fake_loss(q) for q in batch]}
    got = rerank_dataset(qs, fwd, 3, [1, 5], ragged=True)
    assert json.dumps(got) == json.dumps(one_query_per_forward(qs, [1, 5]))


@pytest.mark.parametrize("fail_in", ["submit", "prepare"])
def test_ragged_loop_failure_reaches_the_caller_and_leaves_no_thread(fail_in):
    from rmr_amd import rerank_dataset_pipelined
    before = set(threading.enumerate())
    st = RaggedFakeStages(5, fail_at=2, fail_in=fail_in)
    exc = RuntimeError if fail_in == "submit" else AssertionError
    with pytest.raises(exc, match="fake"):
        rerank_dataset_pipelined(make_queries(SIZES * 4), None, 3, [5], stages=st, ragged=True)
    assert set(threading.enumerate()) == before
    assert not [t for t in threading.enumerate() if t.name == "rmr_amd-tokenize"]
    with pytest.raises(AssertionError):                             # an empty list is refused
        qs = make_queries(SIZES)
        qs[4]["retrieved_docs"] = []
        rerank_dataset_pipelined(qs, None, 3, [5], stages=RaggedFakeStages(5), ragged=True)
    assert set(threading.enumerate()) == before


def test_default_path_still_refuses_an_odd_list():
    from rmr_amd import rerank_dataset_pipelined
    from test_pipeline_cpu import FakeStages
    from test_pipeline_cpu import make_queries as uniform_queries
    K = 5
    qs = uniform_queries(9, K)
    qs[6]["retrieved_docs"] = qs[6]["retrieved_docs"][:-1]
    before = set(threading.enumerate())
    with pytest.raises(AssertionError):
        rerank_dataset_pipelined(qs, None, 2, [K], stages=FakeStages(K))
    with pytest.raises(AssertionError):
        rerank_dataset_pipelined(qs, None, 2, [K], stages=FakeStages(K), ragged=False)
    assert set(threading.enumerate()) == before


def test_records_take_one_loss_per_query():
    from rmr_amd import build_records
    from rmr_amd.evaluate import split_lists
    qs = make_queries([2, 3])
    recs = build_records(qs, [[0.1, 0.2], [0.3, 0.1, 0.2]], [[1, 0], [0, 2, 1]], [0.5, 0.25])
    assert [r["loss"] for r in recs] == [0.5, 0.25]
    assert [r["loss"] for r in build_records(qs, [[0.1, 0.2], [0.3, 0.1, 0.2]], [[1, 0], [0, 2, 1]], 0.75)] == [0.75, 0.75]
    with pytest.raises(AssertionError):
        build_records(qs, [[0.1, 0.2], [0.3, 0.1, 0.2]], [[1, 0], [0, 2, 1]], [0.5])
    assert split_lists([1, 2, 3, 4, 5, 6], [1, 3, 2]) == [[1], [2, 3, 4], [5, 6]]
    with pytest.raises(AssertionError):
        split_lists([1, 2, 3], [1, 1])
