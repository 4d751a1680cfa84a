"""Device-resident passage-embedding bank of the interaction rerankers (rr_bank_*, include/rerank_mi355.h).

The interaction families rerank from the frozen retriever's token embeddings, which the reference hands over in fp16
(`D = D.half()`, src/models/flmr/models/flmr/modeling_flmr.py:1554-1555 of the reference).  A `PassageBank` keeps them on the
device in that form, every passage at its own length, under the caller's passage ids; a forward then names passages
(RerankEngine.forward_interaction_bank, InteractionRerankModel.forward_passages, pipeline.InteractionStages) instead of
uploading and packing a padded float32 [N, Lc, D] tensor per query.

`BankTable` and `plan_bank_batch` are the host side (ids -> indices and lengths -> segments and the packed pair order): pure
Python / numpy, usable and tested without a device.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

from .pair_inputs import group_pairs_by_length


class BankTable:
    """The host table of a bank: passage id -> dense index, and every passage's length in rows."""

    def __init__(self):
        self.index_of: dict = {}
        self.lengths: list = []

    def __len__(self) -> int:
        return len(self.lengths)

    def __contains__(self, passage_id) -> bool:
        return passage_id in self.index_of

    def check_new(self, passage_ids: Sequence) -> None:
        """ValueError when an id is in the table already or appears twice in `passage_ids`; nothing is changed."""
        seen = set()
        for pid in passage_ids:
            if pid in self.index_of or pid in seen:
                raise ValueError(f"passage id {pid!r} is in the bank already: an id is added once")
            seen.add(pid)

    def append(self, passage_ids: Sequence, lengths: Sequence[int], first_index: Optional[int] = None) -> int:
        """Register ids with their lengths under the next dense indices; returns the first of them."""
        assert len(passage_ids) == len(lengths), "one length per passage id"
        self.check_new(passage_ids)
        first = len(self.lengths)
        assert first_index is None or first_index == first, f"the bank's indices continue at {first_index}, the table's at {first}"
        for pid, ln in zip(passage_ids, lengths):
            assert int(ln) >= 1, f"passage {pid!r}: length {ln}"
            self.index_of[pid] = len(self.lengths)
            self.lengths.append(int(ln))
        return first

    def lookup(self, passage_ids: Sequence):
        """(indices, lengths) of `passage_ids` as int64 numpy arrays; an id the table does not hold raises a KeyError naming it."""
        import numpy as np
        idx = np.empty(len(passage_ids), dtype=np.int64)
        lens = np.empty(len(passage_ids), dtype=np.int64)
        for i, pid in enumerate(passage_ids):
            try:
                j = self.index_of[pid]
            except KeyError:
                raise KeyError(f"passage id {pid!r} is not in the bank") from None
            idx[i], lens[i] = j, self.lengths[j]
        return idx, lens

    def clear(self) -> None:
        self.index_of.clear()
        self.lengths.clear()


def plan_bank_batch(table: BankTable, passage_ids: Sequence, K: Optional[int], list_sizes: Optional[Sequence[int]], padded_len: int,
                    granule: int = 16, segment_cost_rows: int = 0) -> dict:
    """Host side of one rr_forward_interaction_bank call.  `passage_ids`: the candidates in pair order, K per query, or
    `list_sizes[q]` for query q (K is None then).  Returns
      indices, lengths : bank index and length of every pair, pair order
      owner            : the query of every pair, pair order
      order, seg_n, seg_len : the packed pair order and the segment table (pair_inputs.group_pairs_by_length over the lengths)
      pair_passage, pair_query : int32, `indices` / `owner` in packed order — what the C call takes.
    Every pair appears once in `order` and every passage fits its segment; an unknown id raises KeyError naming it."""
    import numpy as np
    idx, lens = table.lookup(passage_ids)
    N = int(idx.size)
    assert N >= 1, "no passages"
    if list_sizes is None:
        assert K is not None and K >= 1 and N % K == 0, f"{N} passages are not lists of {K}"
        owner = np.arange(N, dtype=np.int64) // K
    else:
        sizes = np.asarray(list_sizes, dtype=np.int64).reshape(-1)
        assert sizes.size > 0 and int(sizes.min()) >= 1 and int(sizes.sum()) == N, \
            f"list_sizes {sizes.tolist()} do not partition {N} passages into non-empty lists"
        owner = np.repeat(np.arange(sizes.size, dtype=np.int64), sizes)
    assert int(lens.max()) <= padded_len, f"a passage of {int(lens.max())} rows exceeds the padded context length {padded_len}"
    order, seg_n, seg_len = group_pairs_by_length(lens, int(padded_len), int(granule), 1, int(segment_cost_rows))
    return dict(indices=idx, lengths=lens, owner=owner, order=order, seg_n=seg_n, seg_len=seg_len,
                pair_passage=idx[order].astype(np.int32), pair_query=owner[order].astype(np.int32))


class PassageBank:
    """An append-only device store of passage token embeddings (fp16 rows, one mask byte per row) under the caller's ids.
    Created by RerankEngine.create_bank; usable by every interaction engine of the same device and li_dim."""

    def __init__(self, engine, capacity_rows: int, max_passages: int):
        from . import _lib as L
        self._L, self.lib = L, engine.lib
        self.device, self.li_dim = engine.device, int(engine.arch["li_dim"])
        self.table = BankTable()
        self.padded_len = 0                  # the longest Lc an add has seen: the default padded context length of a forward
        h = C.c_void_p()
        L.check(self.lib.rr_bank_create(engine.h, int(capacity_rows), int(max_passages), C.byref(h)), engine.h, "rr_bank_create")
        self.h = h

    def __del__(self):
        self.close()

    def close(self) -> None:
        h = getattr(self, "h", None)
        if h:
            try:
                self.lib.rr_bank_destroy(h)
            except Exception:
                pass
            self.h = None

    def __len__(self) -> int:
        return len(self.table)

    def __contains__(self, passage_id) -> bool:
        return passage_id in self.table

    def _check(self, rc: int, what: str, bad_shape=AssertionError) -> None:
        if rc >= 0:
            return
        L = self._L
        exc = bad_shape if rc == L.RR_ERR_BAD_SHAPE else L._EXC.get(rc, RuntimeError)
        raise exc(f"{what}: {self.lib.rr_status_string(rc).decode()}: {self.lib.rr_bank_last_error(self.h).decode()}")

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def info(self) -> dict:
        """rr_bank_info: passages held, rows used, row capacity."""
        p, r, c = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        self._check(self.lib.rr_bank_info(self.h, C.byref(p), C.byref(r), C.byref(c)), "rr_bank_info")
        return dict(passages=int(p.value), rows_used=int(r.value), capacity_rows=int(c.value))

    def add(self, passage_ids: Sequence, context_li, context_mask, lengths: Optional[Sequence[int]] = None) -> int:
        """Append the passages `passage_ids` from the padded tensors a retriever produces: `context_li` [n, Lc, D] (host or
        device; float32 or float16, anything else goes through float32) and the 0/1 `context_mask` [n, Lc].  Values are kept as
        `context_li.half()`, the mask as (mask != 0), positions unchanged.  `lengths`: the rows each passage keeps (1 + index of
        its last unmasked token, at least 1) as the host knows them; without it they are derived on the device and copied once.
        Returns the first of the n dense indices.  An id added twice raises ValueError, a length outside [1, Lc] ValueError,
        rows or passage slots that do not suffice MemoryError; the bank is unchanged then."""
        import numpy as np
        import torch
        from .pair_inputs import pair_lengths
        L = self._L
        ids = list(passage_ids)
        n = len(ids)
        if context_li.dim() != 3 or context_li.shape[0] != n or context_li.shape[2] != self.li_dim:
            raise ValueError(f"context_li must be [{n}, Lc, {self.li_dim}], got {tuple(context_li.shape)}")
        Lc = int(context_li.shape[1])
        self.table.check_new(ids)
        dt = context_li.dtype if context_li.dtype in (torch.float32, torch.float16) else torch.float32
        li = context_li.to(device=self.device, dtype=dt).contiguous()
        cm = context_mask.reshape(n, Lc).to(device=self.device, dtype=torch.float32).contiguous()
        if lengths is None:
            lengths = pair_lengths(cm).cpu().numpy()
        ln = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1), dtype=np.int32)
        if ln.size != n:
            raise ValueError(f"{ln.size} lengths for {n} passages")
        first = C.c_int32(-1)
        self._check(self.lib.rr_bank_add(self.h, L.ptr(li), L.RR_F16 if dt == torch.float16 else L.RR_F32, L.ptr(cm), ln.ctypes.data,
                                         n, Lc, C.byref(first), self._stream()), "rr_bank_add", bad_shape=ValueError)
        self.table.append(ids, ln.tolist(), int(first.value))
        self.padded_len = max(self.padded_len, Lc)
        return int(first.value)

    def lookup(self, passage_ids: Sequence):
        """(indices, lengths) of `passage_ids`; KeyError names an id the bank does not hold."""
        return self.table.lookup(passage_ids)

    def read(self, passage_id):
        """One passage back on the host (rr_bank_read; synchronises the current stream): (rows [len, D] float16, mask [len]
        uint8)."""
        import torch
        idx, lens = self.table.lookup([passage_id])
        n = int(lens[0])
        rows = torch.empty((n, self.li_dim), dtype=torch.float16)
        mask = torch.empty(n, dtype=torch.uint8)
        got = self.lib.rr_bank_read(self.h, int(idx[0]), rows.data_ptr(), mask.data_ptr(), n, self._stream())
        self._check(got, "rr_bank_read")
        assert got == n, f"the bank holds {got} rows for passage {passage_id!r}, the table {n}"
        return rows, mask

    def clear(self) -> None:
        """Forget every passage (rr_bank_clear; the capacity stays).  Forwards that read the bank must have completed."""
        self._check(self.lib.rr_bank_clear(self.h), "rr_bank_clear")
        self.table.clear()
