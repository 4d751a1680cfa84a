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

For the interaction rerankers (NORMAL, MORES) InteractionStages runs the loop from the frozen retriever's embeddings: the query's
late-interaction tensors travel with the query, the passages' are in the model's device-resident bank (passage_bank.PassageBank)
and are named by id.  Records and metrics are those of rerank_dataset driven by InteractionRerankModel.forward_passages.

The device side is a `stages` object (DeviceStages for a FullContextRerankModel, JointStages for a RerankModel,
InteractionStages for an InteractionRerankModel) with
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

from .evaluate import build_records, compute_rerank_scores, cut_lists, split_lists


class DeviceStages:
    """The device side of rerank_dataset_pipelined for a `FullContextRerankModel` (native tokenizer, packed rows)."""

    def __init__(self, model, batch_queries: int, K: int, first_query: dict, ragged: bool = False):
        """`ragged`: K is the most a query's list may hold (the pinned slots are sized for batch_queries * K pairs), a batch's
        lists may differ in length, and the host buffers are flat over the batch's pairs, beside the list sizes."""
        import torch
        from .pair_inputs import NativePairTokenizer
        self.torch = torch
        self.model, self.engine = model, model.engine
        self.K, self.batch_queries, self.ragged = int(K), int(batch_queries), bool(ragged)
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
            if self.ragged:
                assert 1 <= len(docs) <= K, f"query {q.get('question_id')}: {len(docs)} retrieved docs, the slots hold 1..{K}"
            else:
                assert len(docs) == K, f"query {q.get('question_id')}: {len(docs)} retrieved docs, the loop reranks {K}"
            contexts += [d["content"] for d in docs]
            if self.pointwise:                       # Reranker_base_executor.py:830-833
                pos = q["pos_item_ids"]
                labels += [1.0 if d["passage_id"] in pos else 0.0 for d in docs]
        n = len(batch)
        sizes = [len(q["retrieved_docs"]) for q in batch] if self.ragged else None
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
            lab = slot["labels"][:len(labels)]
            lab.copy_(torch.tensor(labels, dtype=torch.float32))
        if sizes is not None:
            pool, desc = self._prepare_lists(batch, contexts, sizes, slot["pool"])
            return dict(n=n, pool=pool, desc=desc, labels=lab, pixels=pixels, sizes=sizes)
        pool, desc, _ = self.tok.prepare_compact([q["question"] for q in batch], contexts, m.max_query_length, m.max_context_length,
                                                 m.max_decoder_source_length, K, out=slot["pool"], pin_memory=False)
        return dict(n=n, pool=pool, desc=desc, labels=lab, pixels=pixels)

    def _prepare_lists(self, batch: List[dict], contexts: List[str], sizes: List[int], out):
        """prepare_compact for lists of unequal length: the tokenizer takes one candidate count per call, so every query is
        tokenised with its own list into the next part of the slot's pool, and its descriptors are moved to that part."""
        import numpy as np
        torch, m = self.torch, self.model
        descs, pools, used, o, in_place = [], [], 0, 0, True
        for q, k in zip(batch, sizes):
            pool, desc, _ = self.tok.prepare_compact([q["question"]], contexts[o:o + k], m.max_query_length, m.max_context_length,
                                                     m.max_decoder_source_length, k, out=out[used:], pin_memory=False)
            in_place = in_place and pool.numel() > 0 and pool.data_ptr() == out[used:].data_ptr()
            desc = desc.copy()
            desc[:, 0] += used
            desc[:, 2] += used
            descs.append(desc)
            pools.append(pool)
            used += pool.numel()
            o += k
        pool = out[:used] if in_place else torch.cat(pools)      # (a pool the tokenizer had to grow is not in the slot)
        return pool, np.concatenate(descs)

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
        if self.ragged:
            r = eng.forward_tokens_packed(pool_d, item["desc"], None, None, cls, patches, labels_d, want_order=True,
                                          padded_len=m.max_decoder_source_length, special_ids=self.special,
                                          list_sizes=item["sizes"])
        else:
            r = eng.forward_tokens_packed(pool_d, item["desc"], n, K, cls, patches, labels_d, want_order=True,
                                          padded_len=m.max_decoder_source_length, special_ids=self.special)
        host, done = self._read_back(r, n, item.get("sizes"), cs)
        # the batch's device buffers stay referenced here until `done` has been waited for
        return dict(uploaded=uploaded, done=done, host=host, keep=(up, cls, patches, r), sizes=item.get("sizes"))

    def _read_back(self, r: dict, n: int, sizes, cs):
        """Non-blocking copies of a batch's logits, order and loss into pinned memory, and the event behind them.  Uniform:
        [n, K] logits and order, the batch loss.  Ragged: flat [N] logits and order, one loss per list."""
        torch, K = self.torch, self.K
        if sizes is None:
            host = dict(logits=torch.empty((n, K), dtype=torch.float32, pin_memory=True),
                        order=torch.empty((n, K), dtype=torch.int32, pin_memory=True),
                        loss=torch.empty((), dtype=torch.float32, pin_memory=True))
            host["logits"].copy_(r["logits"].view(n, K), non_blocking=True)
            host["loss"].copy_(r["loss"], non_blocking=True)
        else:
            N = sum(sizes)
            host = dict(logits=torch.empty(N, dtype=torch.float32, pin_memory=True),
                        order=torch.empty(N, dtype=torch.int32, pin_memory=True),
                        loss=torch.empty(n, dtype=torch.float32, pin_memory=True))
            host["logits"].copy_(r["logits"], non_blocking=True)
            host["loss"].copy_(r["list_loss"], non_blocking=True)
        host["order"].copy_(r["order"], non_blocking=True)
        done = torch.cuda.Event()
        done.record(cs)
        return host, done

    def release(self, pending: dict) -> None:
        pending["uploaded"].synchronize()

    def collect(self, pending: dict):
        pending["done"].synchronize()
        h, sizes = pending["host"], pending.get("sizes")
        if sizes is None:
            out = h["logits"].tolist(), h["order"].tolist(), float(h["loss"])
        else:                                           # one row per list, one loss per list
            out = split_lists(h["logits"].tolist(), sizes), split_lists(h["order"].tolist(), sizes), h["loss"].tolist()
        pending.clear()
        return out


def joint_compact_batch(tok, batch: List[dict], contexts: List[str], K: int, query_len: int, padded_len: int, out=None,
                        sizes: Optional[Sequence[int]] = None):
    """Host side of JointStages.prepare: the compact inputs of rr_assemble_joint for one batch.  Returns (pool, desc): `pool`
    an int32 host tensor (a view of `out` when it is large enough) with every query's `query_len` ids then its `query_len` mask
    values (query order), then every context's t[0:m], m <= padded_len - 3 (tok.prepare_contexts_compact, pair order); `desc`
    an int32 numpy [len(batch) * K, 3] of (query offset, context offset, m).  `sizes`: the queries' list lengths in place of one K
    (desc then has sum(sizes) rows)."""
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
    owner = np.arange(n * K) // K if sizes is None else np.repeat(np.arange(n), np.asarray(sizes, dtype=np.int64))
    assert owner.size == len(contexts), "one context per pair"
    desc = np.empty((owner.size, 3), dtype=np.int32)
    desc[:, 0] = owner * 2 * ql
    desc[:, 1] = off + base
    desc[:, 2] = ln
    return pool, desc


class JointStages(DeviceStages):
    """The device side of rerank_dataset_pipelined for a `RerankModel` (native context tokenizer, packed joint rows)."""

    def __init__(self, model, batch_queries: int, K: int, first_query: dict, ragged: bool = False):
        import torch
        from .pair_inputs import NativePairTokenizer
        self.torch = torch
        self.model, self.engine = model, model.engine
        self.K, self.batch_queries, self.ragged = int(K), int(batch_queries), bool(ragged)
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
            if self.ragged:
                assert 1 <= len(docs) <= K, f"query {q.get('question_id')}: {len(docs)} retrieved docs, the slots hold 1..{K}"
            else:
                assert len(docs) == K, f"query {q.get('question_id')}: {len(docs)} retrieved docs, the loop reranks {K}"
            contexts += [d["content"] for d in docs]
        n = len(batch)
        sizes = [len(q["retrieved_docs"]) for q in batch] if self.ragged else None
        if any(q.get("pixel_values") is None for q in batch):
            raise NotImplementedError("text_only is not implemented for this model")        # rerank_model.py:184-185
        assert slot["pixels"] is not None, "pixel_values appear after a first query without them"
        pixels = slot["pixels"][:n]
        torch.stack([torch.as_tensor(q["pixel_values"], dtype=torch.float32).reshape(self.pixel_shape) for q in batch], out=pixels)
        pool, desc = joint_compact_batch(self.tok, batch, contexts, K, ql, self.S, out=slot["pool"], sizes=sizes)
        return dict(n=n, pool=pool, desc=desc, pixels=pixels, sizes=sizes)

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
        if self.ragged:
            r = eng.forward_joint_tokens_packed(pool_d, item["desc"], None, None, self.ql, cls, patches, m.instruction_token_id,
                                                want_order=True, padded_len=self.S, special_ids=self.special,
                                                list_sizes=item["sizes"])
        else:
            r = eng.forward_joint_tokens_packed(pool_d, item["desc"], n, K, self.ql, cls, patches, m.instruction_token_id,
                                                want_order=True, padded_len=self.S, special_ids=self.special)
        host, done = self._read_back(r, n, item.get("sizes"), cs)
        # the batch's device buffers stay referenced here until `done` has been waited for
        return dict(uploaded=uploaded, done=done, host=host, keep=(up, cls, patches, r), sizes=item.get("sizes"))


class InteractionStages(DeviceStages):
    """The device side of rerank_dataset_pipelined for an `InteractionRerankModel` with a passage bank (model.bank): a query
    carries its own late-interaction tensors "query_late_interaction" [Lq, D] and "query_mask" [Lq] and names its candidates
    by "passage_id"; their embeddings are in the bank.  The producer thread fills a pinned slot with the batch's query tensors,
    looks the passages up (an id the bank does not hold raises KeyError naming it, which reaches the caller), groups the pairs
    into segments (passage_bank.plan_bank_batch) and builds the labels; the calling thread uploads the slot and runs
    RerankEngine.forward_interaction_bank.  `granule` / `segment_cost_rows` as that call takes them."""

    def __init__(self, model, batch_queries: int, K: int, first_query: dict, ragged: bool = False, granule: int = 16,
                 segment_cost_rows: int = 0):
        import torch
        self.torch = torch
        self.model, self.engine = model, model.engine
        if getattr(model, "bank", None) is None:
            raise ValueError("rerank_dataset_pipelined needs model.bank (InteractionRerankModel.create_bank) for an interaction model")
        self.bank = model.bank
        self.K, self.batch_queries, self.ragged = int(K), int(batch_queries), bool(ragged)
        self.granule, self.segment_cost_rows = int(granule), int(segment_cost_rows)
        q = torch.as_tensor(first_query["query_late_interaction"])
        assert q.dim() == 2 and q.shape[1] == self.bank.li_dim, f"query_late_interaction must be [Lq, {self.bank.li_dim}]"
        self.Lq, self.D = int(q.shape[0]), int(q.shape[1])
        self.pointwise = self.engine.arch["loss_fn"] != "negative_sampling"
        self.device = self.engine.device
        self.copy_stream = None                         # created by the first submit (the calling thread)

    def new_slot(self, pin_memory: bool = True) -> dict:
        torch, nq = self.torch, self.batch_queries
        return dict(q=torch.empty((nq, self.Lq, self.D), dtype=torch.float32, pin_memory=pin_memory),
                    qm=torch.empty((nq, self.Lq), dtype=torch.float32, pin_memory=pin_memory),
                    labels=torch.empty(nq * self.K, dtype=torch.float32, pin_memory=pin_memory))

    def prepare(self, batch: List[dict], slot: dict) -> dict:
        from .passage_bank import plan_bank_batch
        torch, K = self.torch, self.K
        ids, labels = [], []
        for q in batch:
            docs = q["retrieved_docs"]
            if self.ragged:
                assert 1 <= len(docs) <= K, f"query {q.get('question_id')}: {len(docs)} retrieved docs, the slots hold 1..{K}"
            else:
                assert len(docs) == K, f"query {q.get('question_id')}: {len(docs)} retrieved docs, the loop reranks {K}"
            ids += [d["passage_id"] for d in docs]
            if self.pointwise:                       # Reranker_base_executor.py:829-832
                pos = q["pos_item_ids"]
                labels += [1.0 if d["passage_id"] in pos else 0.0 for d in docs]
        n = len(batch)
        sizes = [len(q["retrieved_docs"]) for q in batch] if self.ragged else None
        qs, qms = slot["q"][:n], slot["qm"][:n]
        for i, q in enumerate(batch):
            qs[i].copy_(torch.as_tensor(q["query_late_interaction"], dtype=torch.float32).reshape(self.Lq, self.D))
            qms[i].copy_(torch.as_tensor(q["query_mask"], dtype=torch.float32).reshape(self.Lq))
        lab = None
        if self.pointwise:
            lab = slot["labels"][:len(labels)]
            lab.copy_(torch.tensor(labels, dtype=torch.float32))
        plan = plan_bank_batch(self.bank.table, ids, None if self.ragged else K, sizes, self.bank.padded_len, self.granule,
                               self.segment_cost_rows)
        return dict(n=n, q=qs, qm=qms, labels=lab, plan=plan, sizes=sizes)

    def submit(self, batch: List[dict], item: dict) -> dict:
        torch, eng, dev = self.torch, self.engine, self.device
        n, K = item["n"], self.K
        if self.copy_stream is None:
            self.copy_stream = torch.cuda.Stream(dev)
        cs = torch.cuda.current_stream(dev)
        with torch.cuda.stream(self.copy_stream):       # allocated and filled on the copy stream, used on the compute stream
            up = [torch.empty(t.shape, dtype=t.dtype, device=dev).copy_(t, non_blocking=True) if t is not None else None
                  for t in (item["q"], item["qm"], item["labels"])]
            uploaded = torch.cuda.Event()
            uploaded.record(self.copy_stream)
        cs.wait_event(uploaded)
        for t in up:
            if t is not None:
                t.record_stream(cs)
        q_d, qm_d, labels_d = up
        kw = dict(want_order=True, granule=self.granule, segment_cost_rows=self.segment_cost_rows, plan=item["plan"])
        if self.ragged:
            r = eng.forward_interaction_bank(self.bank, q_d, qm_d, None, None, None, labels_d, list_sizes=item["sizes"], **kw)
        else:
            r = eng.forward_interaction_bank(self.bank, q_d, qm_d, None, n, K, labels_d, **kw)
        host, done = self._read_back(r, n, item.get("sizes"), cs)
        # the batch's device buffers stay referenced here until `done` has been waited for
        return dict(uploaded=uploaded, done=done, host=host, keep=(up, r), sizes=item.get("sizes"))


def rerank_dataset_pipelined(queries: Iterable[dict], model, batch_queries: int, Ks: Sequence[int],
                             docs_to_rerank: Optional[int] = None, out_path: Optional[str] = None, stages=None,
                             stats: Optional[dict] = None, ragged: bool = False) -> dict:
    """`evaluate.rerank_dataset` for a `FullContextRerankModel` or a `RerankModel`, from strings, pipelined (module
    docstring).  A query dict has the fields rerank_dataset reads and, for a FullContextRerankModel, "question" (the query
    text) and optionally "pixel_values" [3, 224, 224] (the model's image path); labels follow the reference executor: 1 where
    a retrieved passage is in pos_item_ids for pointwise losses, none for negative_sampling.  For a RerankModel it has
    "query_input_ids" / "query_attention_mask" (max_query_length entries each, as the dataset gives them) and "pixel_values"
    (mandatory: a query without it raises NotImplementedError, as RerankModel.forward does); its loss reads no labels.
    For an InteractionRerankModel with a passage bank (model.bank) it has "query_late_interaction" [Lq, D] and "query_mask" [Lq],
    the retrieved passages are looked up in the bank by "passage_id" (KeyError for one it does not hold), labels as above.
    K = docs_to_rerank, else the first query's retrieved-doc count; a query with another count raises AssertionError.
    Returns {"metrics", "output"} and writes `out_path` as rerank_dataset does.  `stages`: the device side (default
    JointStages(model, ...) for a RerankModel, InteractionStages(model, ...) for an InteractionRerankModel, else
    DeviceStages(model, ...)).  `stats`, when given, receives batches, tokenise_ms (producer time in `prepare`) and
    records_ms (calling-thread time building records).
    `ragged`: a batch is the next `batch_queries` queries whatever the lengths of their retrieved lists (1 or more docs each);
    `docs_to_rerank`, if given, is the most a list may hold and longer lists are cut to it, else the longest list sizes the
    pinned slots (the queries are then read once before the loop starts); `collect` returns one row of logits and of order
    per query and one loss per query, so each record carries its own list's loss, as the reference's one-query loop does."""
    if ragged:
        queries = cut_lists(queries, docs_to_rerank)
    if docs_to_rerank is not None:
        assert docs_to_rerank == max(Ks), "The number of retrieved documents must be equal to the maximum K."   # :806-808
    records: List[dict] = []
    it = iter(queries)
    first = next(it, None)
    st = dict(batches=0, tokenise_ms=0.0, records_ms=0.0)
    if first is not None:
        if stages is None:
            K = docs_to_rerank if docs_to_rerank is not None else len(first["retrieved_docs"])
            from .model import InteractionRerankModel, RerankModel
            kind = JointStages if isinstance(model, RerankModel) else \
                InteractionStages if isinstance(model, InteractionRerankModel) else DeviceStages
            if ragged:
                if docs_to_rerank is None:           # the longest list sizes the slots
                    rest = list(it)
                    K, it = max(len(q["retrieved_docs"]) for q in [first] + rest), iter(rest)
                stages = kind(model, batch_queries, K, first, ragged=True)
            else:
                stages = kind(model, batch_queries, K, first)
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
