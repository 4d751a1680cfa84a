"""Strings -> prediction records with the device kept busy (rerank_dataset_pipelined).

`evaluate.rerank_dataset` runs each batch in series: tokenise, upload, forward, a blocking read-back, records.  Here the
three overlap.  A producer thread tokenises batch i + 1 (rr_tok_prepare_compact: host work only, ctypes releases the GIL)
into one of two pinned slots while batch i runs; the calling thread uploads a slot's compact tokens on a copy stream,
assembles the pair rows on the device (rr_assemble_pairs), runs the forward and the head, queues non-blocking copies of the
logits, order and loss into pinned buffers, and only then builds batch i - 1's records.  Every HIP call is made from the calling
thread (the engine's handle is not thread-safe).  Records and metrics are those of rerank_dataset driven by
FullContextRerankModel.forward with `native_tokenizer` and `packed_rows` (the reference executor's loop,
src/executors/Reranker_base_executor.py:807-976 of the reference).

For the two-head RerankModel (the joint family) JointStages does the same from what the executor has for a query
(Reranker_base_executor.py:866-873): the dataset's query ids and mask, the query image and the retrieved passages, which the
producer tokenises as the executor's `tokenize_retrieved_docs` does (rr_tok_prepare_contexts_compact, the context encoder's
tokens); rr_assemble_joint builds the joint rows on the device and RerankEngine.forward_joint_tokens_packed runs
rr_forward_joint_packed and rr_head_joint.  Records and metrics are those of rerank_dataset driven by RerankModel.forward
with `packed_rows` over the reference's padded inputs.

The device side is a `stages` object (DeviceStages for a FullContextRerankModel, JointStages for a RerankModel) with
  new_slot() -> slot                     (calling thread; pinned host buffers)
  prepare(batch, slot) -> item           (producer thread; host work only)
  submit(batch, item) -> pending         (calling thread; enqueues everything, blocks on nothing)
  release(pending)                       (calling thread; returns once the slot's upload has completed)
  collect(pending) -> (logits, order, loss)   (calling thread; waits for the batch's read-back)
so the ordering and failure logic can be driven without a device.
"""
from __future__ import annotations

import itertools
import json
import queue
import threading
import time
from typing import Iterable, List, Optional, Sequence

from .evaluate import build_records, compute_rerank_scores


class DeviceStages:
    """The device side of rerank_dataset_pipelined for a `FullContextRerankModel` (native tokenizer, packed rows)."""

    def __init__(self, model, batch_queries: int, K: int, first_query: dict):
        import torch
        from .pair_inputs import NativePairTokenizer
        self.torch = torch
        self.model, self.engine = model, model.engine
        self.K, self.batch_queries = int(K), int(batch_queries)
        tok = model.native_tokenizer
        if tok is None:
            if model.query_tokenizer is None:
                raise RuntimeError("rerank_dataset_pipelined needs config.tokenizer (an HF-style BERT tokenizer)")
            tok = NativePairTokenizer(model.query_tokenizer, do_lower_case=getattr(model.query_tokenizer, "do_lower_case", True))
        self.tok = tok
        self.special = tok.special_ids
        self.pointwise = self.engine.arch["loss_fn"] != "negative_sampling"
        px = first_query.get("pixel_values")
        self.pixel_shape = tuple(px.shape) if px is not None else None
        self.device = self.engine.device
        self.copy_stream = torch.cuda.Stream(self.device)

    def new_slot(self) -> dict:
        torch, N, nq = self.torch, self.batch_queries * self.K, self.batch_queries
        m = self.model
        return dict(pool=torch.empty(nq * 2 * max(1, m.max_query_length) + N * m.max_decoder_source_length, dtype=torch.int32,
                                     pin_memory=True),
                    labels=torch.empty(N, dtype=torch.float32, pin_memory=True),
                    pixels=torch.empty((nq,) + self.pixel_shape, dtype=torch.float32, pin_memory=True)
                    if self.pixel_shape is not None else None)

    def prepare(self, batch: List[dict], slot: dict) -> dict:
        torch, K, m = self.torch, self.K, self.model
        contexts, labels = [], []
        for q in batch:
            docs = q["retrieved_docs"]
            assert len(docs) == K, f"query {q.get('question_id')}: {len(docs)} retrieved docs, the loop reranks {K}"
            contexts += [d["content"] for d in docs]
            if self.pointwise:                       # Reranker_base_executor.py:830-833
                pos = q["pos_item_ids"]
                labels += [1.0 if d["passage_id"] in pos else 0.0 for d in docs]
        n = len(batch)
        has_px = [q.get("pixel_values") is not None for q in batch]
        assert all(has_px) or not any(has_px), "every query of a batch carries pixel_values, or none does"
        pixels = None
        if has_px[0]:
            assert slot["pixels"] is not None, "pixel_values appear after a first query without them"
            pixels = slot["pixels"][:n]
            torch.stack([torch.as_tensor(q["pixel_values"], dtype=torch.float32).reshape(self.pixel_shape) for q in batch],
                        out=pixels)
        lab = None
        if self.pointwise:
            lab = slot["labels"][:n * K]
            lab.copy_(torch.tensor(labels, dtype=torch.float32))
        pool, desc, _ = self.tok.prepare_compact([q["question"] for q in batch], contexts, m.max_query_length, m.max_context_length,
                                                 m.max_decoder_source_length, K, out=slot["pool"], pin_memory=False)
        return dict(n=n, pool=pool, desc=desc, labels=lab, pixels=pixels)

    def submit(self, batch: List[dict], item: dict) -> dict:
        torch, eng, m, dev = self.torch, self.engine, self.model, self.device
        n, K = item["n"], self.K
        cs = torch.cuda.current_stream(dev)
        with torch.cuda.stream(self.copy_stream):       # allocated and filled on the copy stream, used on the compute stream
            up = [torch.empty(t.shape, dtype=t.dtype, device=dev).copy_(t, non_blocking=True) if t is not None else None
                  for t in (item["pool"], item["labels"], item["pixels"])]
            uploaded = torch.cuda.Event()
            uploaded.record(self.copy_stream)
        cs.wait_event(uploaded)
        for t in up:
            if t is not None:
                t.record_stream(cs)
        pool_d, labels_d, px_d = up
        cls = patches = None
        if px_d is not None:
            if m.image_feature_fn is not None:
                cls, patches = m.image_feature_fn(px_d)
            elif eng.arch.get("vit_layers", 0) > 0:
                cls, patches = eng.encode_image(px_d)
            else:
                raise NotImplementedError("pixel_values given but neither config.vision_encoder nor config.image_feature_fn "
                                          "(CLIP ViT) is set")
        r = eng.forward_tokens_packed(pool_d, item["desc"], n, K, cls, patches, labels_d, want_order=True,
                                      padded_len=m.max_decoder_source_length, special_ids=self.special)
        host = dict(logits=torch.empty((n, K), dtype=torch.float32, pin_memory=True),
                    order=torch.empty((n, K), dtype=torch.int32, pin_memory=True),
                    loss=torch.empty((), dtype=torch.float32, pin_memory=True))
        host["logits"].copy_(r["logits"].view(n, K), non_blocking=True)
        host["order"].copy_(r["order"], non_blocking=True)
        host["loss"].copy_(r["loss"], non_blocking=True)
        done = torch.cuda.Event()
        done.record(cs)
        # the batch's device buffers stay referenced here until `done` has been waited for
        return dict(uploaded=uploaded, done=done, host=host, keep=(up, cls, patches, r))

    def release(self, pending: dict) -> None:
        pending["uploaded"].synchronize()

    def collect(self, pending: dict):
        pending["done"].synchronize()
        h = pending["host"]
        out = h["logits"].tolist(), h["order"].tolist(), float(h["loss"])
        pending.clear()
        return out


def joint_compact_batch(tok, batch: List[dict], contexts: List[str], K: int, query_len: int, padded_len: int, out=None):
    """Host side of JointStages.prepare: the compact inputs of rr_assemble_joint for one batch.  Returns (pool, desc): `pool`
    an int32 host tensor (a view of `out` when it is large enough) with every query's `query_len` ids then its `query_len` mask
    values (query order), then every context's t[0:m], m <= padded_len - 3 (tok.prepare_contexts_compact, pair order); `desc`
    an int32 numpy [len(batch) * K, 3] of (query offset, context offset, m)."""
    import numpy as np
    import torch
    n, ql = len(batch), int(query_len)
    rows = [torch.cat([torch.as_tensor(q["query_input_ids"]).reshape(-1).long(),
                       torch.as_tensor(q["query_attention_mask"]).reshape(-1).long()]) for q in batch]
    assert all(r.numel() == 2 * ql for r in rows), f"query_input_ids / query_attention_mask must hold {ql} entries each"
    qpart = torch.stack(rows)
    assert int(qpart.min()) >= 0 and int(qpart.max()) <= 2**31 - 1, "query ids outside the int32 range"
    base = n * 2 * ql
    if out is None or out.numel() < base:
        out = torch.empty(base + len(contexts) * max(1, int(padded_len) - 3), dtype=torch.int32)
    out[:base].copy_(qpart.reshape(-1))
    ctx_out = out[base:]
    cpool, off, ln = tok.prepare_contexts_compact(contexts, int(padded_len) - 3, out=ctx_out, pin_memory=out.is_pinned())
    if cpool.numel() and cpool.data_ptr() != ctx_out.data_ptr():              # the tokenizer grew a buffer of its own
        pool = torch.cat([out[:base], cpool])
        pool = pool.pin_memory() if out.is_pinned() else pool
    else:
        pool = out[:base + cpool.numel()]
    desc = np.empty((n * K, 3), dtype=np.int32)
    desc[:, 0] = (np.arange(n * K) // K) * 2 * ql
    desc[:, 1] = off + base
    desc[:, 2] = ln
    return pool, desc


class JointStages(DeviceStages):
    """The device side of rerank_dataset_pipelined for a `RerankModel` (native context tokenizer, packed joint rows)."""

    def __init__(self, model, batch_queries: int, K: int, first_query: dict):
        import torch
        from .pair_inputs import NativePairTokenizer
        self.torch = torch
        self.model, self.engine = model, model.engine
        self.K, self.batch_queries = int(K), int(batch_queries)
        tok = model.native_tokenizer
        if tok is None:
            if model.decoder_tokenizer is None:
                raise RuntimeError("rerank_dataset_pipelined needs config.decoder_tokenizer (an HF-style BERT tokenizer)")
            tok = NativePairTokenizer(model.decoder_tokenizer,
                                      do_lower_case=getattr(model.decoder_tokenizer, "do_lower_case", True))
        self.tok = tok
        self.special = tok.special_ids
        self.S = int(model.max_decoder_source_length)
        self.ql = int(torch.as_tensor(first_query["query_input_ids"]).numel())
        assert 0 < self.ql < self.S, f"query length {self.ql} must lie in (0, {self.S})"
        px = first_query.get("pixel_values")
        self.pixel_shape = tuple(px.shape) if px is not None else None
        self.device = self.engine.device
        self.copy_stream = None                         # created by the first submit (the calling thread)

    def new_slot(self, pin_memory: bool = True) -> dict:
        torch, nq = self.torch, self.batch_queries
        return dict(pool=torch.empty(nq * 2 * self.ql + nq * self.K * (self.S - 3), dtype=torch.int32, pin_memory=pin_memory),
                    pixels=torch.empty((nq,) + self.pixel_shape, dtype=torch.float32, pin_memory=pin_memory)
                    if self.pixel_shape is not None else None)

    def prepare(self, batch: List[dict], slot: dict) -> dict:
        torch, K, ql = self.torch, self.K, self.ql
        contexts = []
        for q in batch:
            docs = q["retrieved_docs"]
            assert len(docs) == K, f"query {q.get('question_id')}: {len(docs)} retrieved docs, the loop reranks {K}"
            contexts += [d["content"] for d in docs]
        n = len(batch)
        if any(q.get("pixel_values") is None for q in batch):
            raise NotImplementedError("text_only is not implemented for this model")        # rerank_model.py:184-185
        assert slot["pixels"] is not None, "pixel_values appear after a first query without them"
        pixels = slot["pixels"][:n]
        torch.stack([torch.as_tensor(q["pixel_values"], dtype=torch.float32).reshape(self.pixel_shape) for q in batch], out=pixels)
        pool, desc = joint_compact_batch(self.tok, batch, contexts, K, ql, self.S, out=slot["pool"])
        return dict(n=n, pool=pool, desc=desc, pixels=pixels)

    def submit(self, batch: List[dict], item: dict) -> dict:
        torch, eng, m, dev = self.torch, self.engine, self.model, self.device
        n, K = item["n"], self.K
        if self.copy_stream is None:
            self.copy_stream = torch.cuda.Stream(dev)
        cs = torch.cuda.current_stream(dev)
        with torch.cuda.stream(self.copy_stream):       # allocated and filled on the copy stream, used on the compute stream
            up = [torch.empty(t.shape, dtype=t.dtype, device=dev).copy_(t, non_blocking=True) for t in (item["pool"], item["pixels"])]
            uploaded = torch.cuda.Event()
            uploaded.record(self.copy_stream)
        cs.wait_event(uploaded)
        for t in up:
            t.record_stream(cs)
        pool_d, px_d = up
        if m.image_feature_fn is not None:
            cls, patches = m.image_feature_fn(px_d)
        elif eng.arch.get("vit_layers", 0) > 0:
            cls, patches = eng.encode_image(px_d)
        else:
            raise NotImplementedError("query_pixel_values given but neither config.vision_encoder nor config.image_feature_fn "
                                      "(CLIP ViT) is set")
        r = eng.forward_joint_tokens_packed(pool_d, item["desc"], n, K, self.ql, cls, patches, m.instruction_token_id,
                                            want_order=True, padded_len=self.S, special_ids=self.special)
        host = dict(logits=torch.empty((n, K), dtype=torch.float32, pin_memory=True),
                    order=torch.empty((n, K), dtype=torch.int32, pin_memory=True),
                    loss=torch.empty((), dtype=torch.float32, pin_memory=True))
        host["logits"].copy_(r["logits"].view(n, K), non_blocking=True)
        host["order"].copy_(r["order"], non_blocking=True)
        host["loss"].copy_(r["loss"], non_blocking=True)
        done = torch.cuda.Event()
        done.record(cs)
        # the batch's device buffers stay referenced here until `done` has been waited for
        return dict(uploaded=uploaded, done=done, host=host, keep=(up, cls, patches, r))


def rerank_dataset_pipelined(queries: Iterable[dict], model, batch_queries: int, Ks: Sequence[int],
                             docs_to_rerank: Optional[int] = None, out_path: Optional[str] = None, stages=None,
                             stats: Optional[dict] = None) -> dict:
    """`evaluate.rerank_dataset` for a `FullContextRerankModel` or a `RerankModel`, from strings, pipelined (module
    docstring).  A query dict has the fields rerank_dataset reads and, for a FullContextRerankModel, "question" (the query
    text) and optionally "pixel_values" [3, 224, 224] (the model's image path); labels follow the reference executor: 1 where
    a retrieved passage is in pos_item_ids for pointwise losses, none for negative_sampling.  For a RerankModel it has
    "query_input_ids" / "query_attention_mask" (max_query_length entries each, as the dataset gives them) and "pixel_values"
    (mandatory: a query without it raises NotImplementedError, as RerankModel.forward does); its loss reads no labels.
    K = docs_to_rerank, else the first query's retrieved-doc count; a query with another count raises AssertionError.
    Returns {"metrics", "output"} and writes `out_path` as rerank_dataset does.  `stages`: the device side (default
    JointStages(model, ...) for a RerankModel, else DeviceStages(model, ...)).  `stats`, when given, receives batches, tokenise_ms (producer time in `prepare`) and
    records_ms (calling-thread time building records)."""
    if docs_to_rerank is not None:
        assert docs_to_rerank == max(Ks), "The number of retrieved documents must be equal to the maximum K."   # :806-808
    records: List[dict] = []
    it = iter(queries)
    first = next(it, None)
    st = dict(batches=0, tokenise_ms=0.0, records_ms=0.0)
    if first is not None:
        if stages is None:
            K = docs_to_rerank if docs_to_rerank is not None else len(first["retrieved_docs"])
            from .model import RerankModel
            stages = (JointStages if isinstance(model, RerankModel) else DeviceStages)(model, batch_queries, K, first)
        _run(itertools.chain([first], it), stages, batch_queries, records, st)
    if stats is not None:
        stats.update(st)
    metrics = compute_rerank_scores(records, Ks)
    metrics["loss"] = sum(r["loss"] for r in records) / max(1, len(records))                      # :1022-1026
    result = {"metrics": metrics, "output": records}
    if out_path:
        with open(out_path, "w") as f:
            json.dump({"output": records}, f, indent=4)
    return result


_END, _ERROR, _BATCH = range(3)


def _run(source, stages, batch_queries: int, records: List[dict], st: dict) -> None:
    free: "queue.Queue" = queue.Queue()
    ready: "queue.Queue" = queue.Queue()
    stop = threading.Event()
    for _ in range(2):
        free.put(stages.new_slot())

    def emit(batch) -> bool:
        while True:                                 # a free slot, unless the calling thread has given up
            if stop.is_set():
                return False
            try:
                slot = free.get(timeout=0.05)
                break
            except queue.Empty:
                pass
        t0 = time.perf_counter()
        item = stages.prepare(batch, slot)
        st["tokenise_ms"] += (time.perf_counter() - t0) * 1e3
        ready.put((_BATCH, (batch, slot, item)))
        return True

    def producer():
        try:
            batch: List[dict] = []
            for q in source:
                batch.append(q)
                if len(batch) == batch_queries:
                    if not emit(batch):
                        return
                    batch = []
            if batch and not emit(batch):           # the last, partial batch
                return
            ready.put((_END, None))
        except BaseException as e:                  # reaches the caller as it is
            ready.put((_ERROR, e))

    def finish(batch, pending):
        logits, order, loss = stages.collect(pending)
        t0 = time.perf_counter()
        records.extend(build_records(batch, logits, order, loss))
        st["records_ms"] += (time.perf_counter() - t0) * 1e3
        st["batches"] += 1

    th = threading.Thread(target=producer, name="rmr_amd-tokenize", daemon=True)
    th.start()
    prev = None
    try:
        while True:
            kind, val = ready.get()
            if kind == _ERROR:
                raise val
            if kind == _END:
                break
            batch, slot, item = val
            pending = stages.submit(batch, item)
            stages.release(pending)                 # the slot's upload has completed: it may be refilled
            free.put(slot)
            if prev is not None:                    # batch i - 1's records while batch i runs
                finish(*prev)
            prev = (batch, pending)
        if prev is not None:
            p, prev = prev, None
            finish(*p)
    finally:
        stop.set()
        th.join()
