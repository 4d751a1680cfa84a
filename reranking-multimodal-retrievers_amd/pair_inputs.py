"""Pair-input assembly for the full-context reranker (host side, CPU string work).

Restates `prepare_full_context_inputs` (/root/reference/src/models/rerank/utils.py:129-167): truncate the
query to `max_query_length` tokens and every context to `max_context_length` tokens by an
encode->decode round trip (no special tokens), pair them query-major, then `batch_encode_plus` the
(query, context) pairs with special tokens, padded/truncated to `max_decoder_source_length` — which yields
input_ids, attention_mask and pair-encoding token_type_ids.  Any HF-style tokenizer object works; the build
environment has no vocab file, so tests use a small locally generated WordPiece vocab.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch


def truncate_and_pair(query_text_sequences: List[str], context_text_sequences: List[str], tokenizer, max_query_length: int,
                      max_context_length: int, docs_per_query: int) -> List[tuple]:
    """utils.py:131-153: queries / contexts cut to their token budgets by an encode -> decode round trip (no special tokens),
    then paired query-major.  Pinned to the reference's own loop executed from source (tests/golden/reference_fn.npz `pfc.*`)."""
    def clip(text: str, n: int) -> str:
        return tokenizer.decode(tokenizer.encode(text, add_special_tokens=False, max_length=n, truncation=True))

    queries = [clip(t, max_query_length) for t in query_text_sequences]
    contexts = [clip(t, max_context_length) for t in context_text_sequences]
    return [(q, contexts[i * docs_per_query + j]) for i, q in enumerate(queries) for j in range(docs_per_query)]


def prepare_full_context_inputs(query_text_sequences: List[str], context_text_sequences: List[str], tokenizer,
                                max_query_length: int, max_context_length: int, max_decoder_source_length: int,
                                docs_per_query: int) -> Dict[str, torch.Tensor]:
    pairs = truncate_and_pair(query_text_sequences, context_text_sequences, tokenizer, max_query_length, max_context_length,
                              docs_per_query)
    kw = dict(add_special_tokens=True, return_tensors="pt", padding="max_length", truncation=True,
              max_length=max_decoder_source_length, return_attention_mask=True, return_token_type_ids=True)
    if hasattr(tokenizer, "batch_encode_plus"):          # transformers 4.x (the reference pins 4.38.2)
        enc = tokenizer.batch_encode_plus(pairs, **kw)
    else:                                                # transformers 5.x dropped it; __call__ is equivalent
        enc = tokenizer([q for q, _ in pairs], [c for _, c in pairs], **kw)
    return {"input_ids": enc["input_ids"].to(torch.int64), "attention_mask": enc["attention_mask"].to(torch.int64),
            "token_type_ids": enc["token_type_ids"].to(torch.int64)}


class NativePairTokenizer:
    """The same assembly in native code (csrc/pair_tokenizer.cpp behind `rr_tok_*`): multi-threaded WordPiece +
    truncate-by-round-trip + pair encoding straight into pinned int64 host tensors, no Python per text.

    `vocab` is the id-ordered token list (the lines of vocab.txt) or an HF tokenizer exposing `.vocab` / `get_vocab()`.
    Semantics: transformers 4.38.2 slow `BertTokenizer` (what the reference pins), see the C++ file's header."""

    def __init__(self, vocab, do_lower_case: bool = True, n_threads: int = 0):
        import ctypes as C
        from . import _lib as L
        self._C, self._L = C, L
        self.lib = L.load()
        if not isinstance(vocab, (list, tuple)):
            v = vocab.get_vocab() if hasattr(vocab, "get_vocab") else vocab.vocab
            vocab = [t for t, _ in sorted(v.items(), key=lambda kv: kv[1])]
        self.vocab = list(vocab)
        arr = (C.c_char_p * len(self.vocab))(*[t.encode("utf-8") for t in self.vocab])
        h = C.c_void_p()
        L.check(self.lib.rr_tok_create(arr, len(self.vocab), int(do_lower_case), C.byref(h)), None, "rr_tok_create")
        self.h, self.n_threads = h, int(n_threads)

    def __del__(self):
        h = getattr(self, "h", None)
        if h:
            try:
                self.lib.rr_tok_destroy(h)
            except Exception:
                pass
            self.h = None

    def encode(self, text: str, max_length: int = -1) -> List[int]:
        C = self._C
        raw = text.encode("utf-8", "replace")
        cap = len(raw) + 8                                    # every id consumes at least one input byte
        buf = (C.c_int32 * cap)()
        n = self.lib.rr_tok_encode(self.h, raw, int(max_length), buf, cap)
        if n < 0:
            raise ValueError(f"rr_tok_encode failed ({n})")
        return list(buf[:n])

    def decode(self, ids) -> str:
        C = self._C
        ids = list(ids)
        arr = (C.c_int32 * max(1, len(ids)))(*ids)
        cap = 16 + sum(len(self.vocab[i].encode("utf-8")) + 1 for i in ids)
        out = C.create_string_buffer(cap)
        n = self.lib.rr_tok_decode(self.h, arr, len(ids), out, cap)
        if n < 0:
            raise ValueError(f"rr_tok_decode failed ({n})")
        return out.raw[:n].decode("utf-8")

    def prepare_full_context_inputs(self, query_text_sequences: List[str], context_text_sequences: List[str],
                                    max_query_length: int, max_context_length: int, max_decoder_source_length: int,
                                    docs_per_query: int, pin_memory: bool = False) -> Dict[str, torch.Tensor]:
        C = self._C
        nq = len(query_text_sequences)
        N = nq * docs_per_query
        assert N == len(context_text_sequences), "expanded batch size must be batch_size * docs_per_query"   # :527
        q = (C.c_char_p * nq)(*[t.encode("utf-8", "replace") for t in query_text_sequences])
        c = (C.c_char_p * N)(*[t.encode("utf-8", "replace") for t in context_text_sequences])
        out = [torch.empty((N, max_decoder_source_length), dtype=torch.int64, pin_memory=pin_memory) for _ in range(3)]
        rc = self.lib.rr_tok_prepare_pairs(self.h, q, nq, c, docs_per_query, max_query_length, max_context_length,
                                           max_decoder_source_length, self.n_threads, out[0].data_ptr(), out[1].data_ptr(),
                                           out[2].data_ptr())
        if rc != 0:
            raise ValueError(f"rr_tok_prepare_pairs failed ({rc})")
        return {"input_ids": out[0], "attention_mask": out[1], "token_type_ids": out[2]}


    @property
    def special_ids(self):
        """(cls, sep, pad) ids of the vocabulary (a repeated token keeps its last index, as rr_tok_create)."""
        idx = {t: i for i, t in enumerate(self.vocab)}
        return idx["[CLS]"], idx["[SEP]"], idx["[PAD]"]

    def prepare_compact(self, query_text_sequences: List[str], context_text_sequences: List[str], max_query_length: int,
                        max_context_length: int, max_decoder_source_length: int, docs_per_query: int,
                        out: Optional[torch.Tensor] = None, pin_memory: bool = True):
        """rr_tok_prepare_compact: the pairs of `prepare_full_context_inputs` without padded rows.  Returns (pool, desc,
        lengths): `pool` an int32 host tensor (a view of `out` when it is large enough, else of a new buffer, pinned when
        `pin_memory`) with every query's round-tripped ids once, then every pair's kept context ids; `desc` an int32 numpy
        [N, 4] of (query offset, la, context offset, lb); `lengths` the int64 numpy token counts la + lb + 3, which is
        what `pair_lengths` gives for the padded rows.  All host values: grouping needs no device -> host copy."""
        import numpy as np
        C = self._C
        nq = len(query_text_sequences)
        N = nq * docs_per_query
        assert N == len(context_text_sequences), "expanded batch size must be batch_size * docs_per_query"   # :527
        q = (C.c_char_p * nq)(*[t.encode("utf-8", "replace") for t in query_text_sequences])
        c = (C.c_char_p * N)(*[t.encode("utf-8", "replace") for t in context_text_sequences])
        desc = np.empty((N, 4), dtype=np.int32)
        need = C.c_int64(0)
        threads = self.n_threads if self.n_threads > 0 else host_threads()
        buf = out if out is not None else torch.empty(nq * 2 * max(1, max_query_length) + N * max_decoder_source_length,
                                                      dtype=torch.int32, pin_memory=pin_memory)
        for _ in range(2):
            assert buf.dtype == torch.int32 and buf.is_contiguous()
            rc = self.lib.rr_tok_prepare_compact(self.h, q, nq, c, docs_per_query, max_query_length, max_context_length,
                                                 max_decoder_source_length, threads, buf.data_ptr(), buf.numel(), C.byref(need),
                                                 desc.ctypes.data)
            if rc == 0:
                lengths = desc[:, 1].astype(np.int64) + desc[:, 3] + 3
                return buf[:need.value], desc, lengths
            if rc != self._L.RR_ERR_BAD_SHAPE or need.value <= buf.numel():
                break
            buf = torch.empty(need.value + need.value // 4, dtype=torch.int32, pin_memory=pin_memory)   # grow, tokenise again
        raise ValueError(f"rr_tok_prepare_compact failed ({rc}, pool needs {need.value})")

    def prepare_contexts_compact(self, context_text_sequences: List[str], max_tokens: int, out: Optional[torch.Tensor] = None,
                                 pin_memory: bool = True):
        """rr_tok_prepare_contexts_compact: the context encoder's tokens (FLMRContextEncoderTokenizer, see
        flmr_context_inputs) without padded rows.  Returns (pool, offsets, lengths): `pool` an int32 host tensor (a view of
        `out` when it is large enough, else of a new buffer, pinned when `pin_memory`) holding every context's
        t[0:min(len(t), max_tokens)] once, in context order; `offsets` / `lengths` int32 numpy [n] into it.  With max_tokens =
        max_length - 3 the reference's padded row of context i is [CLS] [unused1] t[0:lengths[i]] [SEP] [PAD]..."""
        import numpy as np
        C = self._C
        n = len(context_text_sequences)
        c = (C.c_char_p * n)(*[t.encode("utf-8", "replace") for t in context_text_sequences])
        offsets, lengths = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        need = C.c_int64(0)
        threads = self.n_threads if self.n_threads > 0 else host_threads()
        buf = out if out is not None else torch.empty(max(1, n * int(max_tokens)), dtype=torch.int32, pin_memory=pin_memory)
        for _ in range(2):
            assert buf.dtype == torch.int32 and buf.is_contiguous()
            rc = self.lib.rr_tok_prepare_contexts_compact(self.h, c, n, int(max_tokens), threads, buf.data_ptr(), buf.numel(),
                                                          C.byref(need), offsets.ctypes.data, lengths.ctypes.data)
            if rc == 0:
                return buf[:need.value], offsets, lengths
            if rc != self._L.RR_ERR_BAD_SHAPE or need.value <= buf.numel():
                break
            buf = torch.empty(need.value + need.value // 4, dtype=torch.int32, pin_memory=pin_memory)   # grow, tokenise again
        raise ValueError(f"rr_tok_prepare_contexts_compact failed ({rc}, pool needs {need.value})")


def flmr_context_inputs(context_text_sequences: List[str], tokenizer, max_length: int = 512) -> Dict[str, torch.Tensor]:
    """What the reference executor's `tokenize_retrieved_docs` (Reranker_base_executor.py:1056-1066) gets from its
    `decoder_tokenizer`, FLMRContextEncoderTokenizer.__call__ (tokenization_flmr.py:120-150), on any HF-style BERT tokenizer:
    ". " + text, padded and truncated to `max_length`, then ids[:, 1] = [unused1] (the [D] marker).  int64 [N, max_length]
    input_ids / attention_mask: the serial path's context inputs of RerankModel.forward."""
    enc = tokenizer([". " + t for t in context_text_sequences], padding="max_length", max_length=max_length, truncation=True,
                    return_tensors="pt")
    ids, mask = enc["input_ids"].to(torch.int64), enc["attention_mask"].to(torch.int64)
    ids[:, 1] = tokenizer.convert_tokens_to_ids("[unused1]")
    return {"input_ids": ids, "attention_mask": mask}


def host_threads() -> int:
    """CPU threads for host-side tokenisation: the CPUs this process may run on (not os.cpu_count(), the machine's), capped by
    OMP_NUM_THREADS when that is set."""
    import os
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        cap = int(os.environ.get("OMP_NUM_THREADS", "0"))
    except ValueError:
        cap = 0
    return max(1, min(n, cap) if cap > 0 else n)


def group_pairs_by_length(lengths, padded_len: int, granule: int, min_len: int = 1, segment_cost_rows: int = 0):
    """Host side of the packed forward (rr_forward_packed): pairs -> segments of equal row length.
    `lengths[i]` = token count of pair i (1 + index of its last non-pad position, as the tokenizer knows it), clipped to
    [1, padded_len]; a pair goes to the smallest multiple of `granule` (at least `min_len`: the mapping network's
    cross-attention window when image features are present; at most `padded_len`) that holds it.
    Returns (order, seg_pairs, seg_len): `order` lists the pair indices segment after segment (ascending length, input order
    kept inside a segment: a stable sort), seg_pairs / seg_len one entry per NON-EMPTY segment.  The reference pads every
    pair to padded_len (utils.py:157-165): one segment of that length.
    `segment_cost_rows` > 0: every segment costs the forward a fixed number of small launches (embeddings, masks, gathers, the
    CLS attention: ~140 us on an MI355X), so neighbouring lengths are MERGED where that is cheaper than the rows the merge pads:
    the segmentation of the sorted lengths that minimises (rows computed + segment_cost_rows x segments), by dynamic
    programming over the <= padded_len / granule distinct lengths.  Any grouping computes the same logits (a pair only has to
    fit its segment's length)."""
    import numpy as np
    if granule <= 0 or padded_len <= 0:
        raise ValueError("granule and padded_len must be positive")
    ln = np.clip(np.asarray(lengths, dtype=np.int64).reshape(-1), 1, padded_len)
    sizes = np.asarray(sorted({min(padded_len, max(int(min_len), g)) for g in range(granule, padded_len + granule, granule)}), dtype=np.int64)
    which = np.searchsorted(sizes, ln, side="left")               # smallest segment length >= len
    order = np.argsort(which, kind="stable")
    counts = np.bincount(which, minlength=len(sizes))
    keep = counts > 0
    cnt, szs = counts[keep].tolist(), sizes[keep].tolist()
    if segment_cost_rows > 0 and len(cnt) > 1:
        m = len(cnt)
        pre = [0]
        for c in cnt:
            pre.append(pre[-1] + c)
        best = [0.0] + [float("inf")] * m          # best[j] = cheapest segmentation of the first j lengths
        cut = [0] * (m + 1)
        for j in range(1, m + 1):
            for i in range(j):                        # last segment = lengths i .. j-1, run at length szs[j-1]
                c = best[i] + (pre[j] - pre[i]) * szs[j - 1] + segment_cost_rows
                if c < best[j]:
                    best[j], cut[j] = c, i
        segs, j = [], m
        while j > 0:
            segs.append((cut[j], j))
            j = cut[j]
        segs.reverse()
        cnt, szs = [pre[j] - pre[i] for i, j in segs], [szs[j - 1] for i, j in segs]
    return order, cnt, szs


def pair_lengths(*rows) -> torch.Tensor:
    """Length of every pair for the packed forwards: 1 + index of the last non-zero entry over the union of the given [N, S]
    tensors (ids / attention masks of the full-context and joint sequences, the context mask of the interaction rerankers),
    at least 1.  Stays on the tensors' device."""
    used = None
    for t in rows:
        nz = t.reshape(t.shape[0], -1) != 0
        used = nz if used is None else used | nz
    cols = torch.arange(1, used.shape[1] + 1, device=used.device)
    return (used * cols).amax(1).clamp_(min=1)


def pack_rows(t: torch.Tensor, order: torch.Tensor, seg_n, seg_len) -> torch.Tensor:
    """Packed layout of a per-pair tensor t [N, S, ...] for the rr_forward_*_packed calls: segment after segment, inside a
    segment pair after pair (`order`, as group_pairs_by_length returns it), the first seg_len[i] positions of every pair:
    [sum_i seg_n[i] * seg_len[i], ...].  Index plumbing only (index_select + slicing)."""
    parts, o = [], 0
    for n, sl in zip(seg_n, seg_len):
        parts.append(t.index_select(0, order[o: o + n])[:, :sl].reshape(n * sl, *t.shape[2:]))
        o += n
    return torch.cat(parts).contiguous()


def scatter_packed(values: torch.Tensor, order: torch.Tensor) -> torch.Tensor:
    """Inverse of the packed pair order: out[order[i]] = values[i] (logits come back from the packed calls in packed order)."""
    return torch.empty_like(values).index_copy_(0, order, values)


def pack_fusion_scores(scores: torch.Tensor, order: torch.Tensor, row0: int = 0, rows: int = -1) -> torch.Tensor:
    """PreFLMR fusion scores of a packed call: rows row0 .. row0 + rows of every pair's context axis (the joint sequence's context
    tokens sit at score rows 2 .. 2 + S - query_len, rerank_model.py:276-284; the interaction scores [N, Lc, Lq] are all context)
    in packed pair order — still PADDED along that axis: the reference's softmax over the context tokens runs over all of it."""
    rows = scores.shape[1] - row0 if rows < 0 else rows
    return scores[:, row0:row0 + rows].index_select(0, order).contiguous()
