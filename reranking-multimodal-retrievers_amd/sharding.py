"""Multi-GPU execution of one rerank batch: candidate pairs are independent, so the N = Bq*K pairs are
split into contiguous per-rank slices (weights replicated), every rank runs the encoder on its slice, the
fp32 logits are exchanged with ONE `all_gather_into_tensor` (RCCL over xGMI when the backend is "nccl" on
ROCm; gloo in the CPU tests) and the scoring head + top-K run redundantly on every rank.

The reference has no such exchange (DDP shards queries, every rank writes its own JSON —
/root/reference/src/executors/Reranker_base_executor.py:1118-1121); this is the new collective of SURVEY §8e.

Buffers: the send slice, the gathered block and the compacted logits (+ status words) are allocated once per
(device, world size, slice length, heads) and reused by every later batch of that shape — no allocation and no
`torch.cat` in the steady state.  Both heads of the 2H_BCE variant travel in the same collective.  The collective is
enqueued by `torch.distributed` behind the work stream's kernels (ProcessGroupNCCL waits on the current stream's
event and the current stream waits on the collective), so the encoder of the next batch may already be enqueued.

Errors are COLLECTIVE: an exception inside one rank's encoder — e.g. the sticky RR_ERR_RANGE of a handle whose
pair slice left the fp16 range, which depends on that rank's own pairs — must not leave the other ranks waiting in the
all-gather.  Every rank's block therefore ends in one status word (0 ok / 1 range error / 2 any other error); a failing rank
still takes part in the exchange (zero logits, its status word set) and every rank raises after it: the failing rank its own
exception, the others `ShardPeerError` (an OverflowError when the peer's was one) naming the ranks.  Reading the status words
is one host read of `world` floats per batch; a loop that must not synchronise per batch passes `defer_status=True`: the words
are folded into a device-side running maximum (no allocation, no host read) and NOBODY raises — a rank whose encoder failed keeps
taking part with zero logits and its status word set — until `check_deferred_status()`, which such a loop calls before it uses its
results (and which the next non-deferred call runs first): there every rank reads the same maximum and raises together.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional, Tuple

import torch
import torch.distributed as dist


def shard_range(n_pairs: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous slice [begin, end) of rank `rank`; sizes differ by at most one, earlier ranks larger."""
    q, r = divmod(n_pairs, world)
    b = rank * q + min(rank, r)
    return b, b + q + (1 if rank < r else 0)


STATUS_OK, STATUS_RANGE, STATUS_ERROR = 0, 1, 2


class ShardPeerError(RuntimeError):
    """Another rank's encoder failed in this batch (its own process carries the original exception)."""


class ShardPeerRangeError(ShardPeerError, OverflowError):
    """Another rank's handle reported RR_ERR_RANGE (OverflowError there): the batch's logits are unreliable on every rank."""


class _GatherPlan:
    """Preallocated buffers of one (device, dtype, world, n_pairs, n_heads) exchange.  A rank's block is
    [head 0: per | head 1: per | status word]."""

    def __init__(self, device, dtype, world: int, n_pairs: int, heads: int):
        self.world, self.n, self.heads = world, n_pairs, heads
        self.per = -(-n_pairs // world)                                  # ceil(N / W): the padded slice length
        self.blk = heads * self.per + 1                                  # + the status word
        self.host = None
        self.send = torch.zeros(self.blk, dtype=dtype, device=device)
        self.sent_status = STATUS_OK                                     # what send[-1] holds (rewritten only when it changes: no launch in the steady state)
        self.recv = torch.empty(world * self.blk, dtype=dtype, device=device)
        # compaction map: full[h][i] = recv[rank(i), h, i - begin(rank)], then the `world` status words — one index_select, no cat
        idx = torch.empty(heads, n_pairs, dtype=torch.int64)
        for r in range(world):
            b, e = shard_range(n_pairs, r, world)
            for h in range(heads):
                idx[h, b:e] = torch.arange(e - b) + r * self.blk + h * self.per
        status = torch.arange(world, dtype=torch.int64) * self.blk + (self.blk - 1)
        self.index = torch.cat([idx.reshape(-1), status]).to(device)
        self.full = torch.empty(heads * n_pairs + world, dtype=dtype, device=device)
        self.status_accum = torch.zeros(world, dtype=dtype, device=device)   # deferred mode: running maximum of the status words
        self.status_host = torch.empty(world, dtype=dtype, device="cpu")
        if torch.device(device).type == "cuda":
            self.status_host = self.status_host.pin_memory()


_PLANS: "OrderedDict[tuple, _GatherPlan]" = None      # small LRU: a serving loop sees a handful of batch sizes (the full one, the last one)
_MAX_PLANS = 8


def _plan(device, dtype, world, n_pairs, heads, group=None) -> _GatherPlan:
    from collections import OrderedDict
    global _PLANS
    if _PLANS is None:
        _PLANS = OrderedDict()
    key = (str(device), dtype, world, n_pairs, heads, id(group) if group is not None else 0)
    p = _PLANS.get(key)
    if p is None:
        p = _PLANS[key] = _GatherPlan(device, dtype, world, n_pairs, heads)
        while len(_PLANS) > _MAX_PLANS:
            _PLANS.popitem(last=False)
    else:
        _PLANS.move_to_end(key)
    return p


def gather_logits(local: torch.Tensor, n_pairs: int, group=None, local2: Optional[torch.Tensor] = None, status: int = STATUS_OK,
                  want_status: bool = False, defer_status: bool = False):
    """All-gather the ragged per-rank logit slices (and, for the two-head variant, the second head's) into the full
    [n_pairs] vector(s) with ONE collective.  Returns (full, full2 | None) — and, with `want_status`, the `world` status
    words every rank sent (a device tensor of the logits' dtype) as a third element; the tensors are views of buffers that the
    next call with the same shape overwrites.  `defer_status`: fold the status words into the plan's running maximum for
    check_deferred_status() instead."""
    world = dist.get_world_size(group)
    heads = 1 if local2 is None else 2
    p = _plan(local.device, local.dtype, world, n_pairs, heads, group)
    n_loc = local.numel()
    p.send[:n_loc].copy_(local.reshape(-1))
    if local2 is not None:
        p.send[p.per: p.per + n_loc].copy_(local2.reshape(-1))
    if status != p.sent_status:
        p.send[p.blk - 1] = float(status)
        p.sent_status = status
    if p.send.is_cuda and dist.get_backend(group) == "gloo":
        # rehearsal on one GPU (bench.py --rehearse-one-gpu): gloo has no device all-gather, stage through the host
        if p.host is None:
            p.host = (torch.empty_like(p.send, device="cpu").pin_memory(), torch.empty_like(p.recv, device="cpu").pin_memory())
        p.host[0].copy_(p.send)
        dist.all_gather_into_tensor(p.host[1], p.host[0], group=group)
        p.recv.copy_(p.host[1])
    else:
        dist.all_gather_into_tensor(p.recv, p.send, group=group)
    torch.index_select(p.recv, 0, p.index, out=p.full)
    full1, full2 = p.full[:n_pairs], (p.full[n_pairs:2 * n_pairs] if heads == 2 else None)
    if defer_status:
        torch.maximum(p.status_accum, p.full[heads * n_pairs:], out=p.status_accum)
        _PENDING[id(p)] = (p, dist.get_rank(group))
    return (full1, full2, p.full[heads * n_pairs:]) if want_status else (full1, full2)


_PENDING: Dict[int, tuple] = {}      # plans whose running status maximum has not been looked at: id -> (plan, rank)
_OWN_DEFERRED: list = []             # this rank's own encoder exceptions of deferred batches (the first one is re-raised)


def check_deferred_status():
    """Look at what the `defer_status` batches since the last check reported: one host read per plan in use.  Every rank holds the
    same maxima, so every rank raises here together (the rank whose encoder failed its own first exception, its peers
    ShardPeerError) or none does.  The results of the batches since the failure are to be discarded by the caller."""
    own = _OWN_DEFERRED[0] if _OWN_DEFERRED else None
    failed = None
    for p, rank in list(_PENDING.values()):
        p.status_host.copy_(p.status_accum)               # synchronises with the stream the gathers ran on
        words = p.status_host.tolist()
        p.status_accum.zero_()
        if failed is None and any(int(w) != STATUS_OK for w in words):
            failed = (words, rank)
    _PENDING.clear()
    _OWN_DEFERRED.clear()
    if failed is not None:
        _raise_collectively(failed[0], failed[1], own)
    elif own is not None:
        raise own


def _raise_collectively(status_words, rank: int, own: Optional[BaseException]):
    """Every rank sees the same status words, so every rank raises (or none does)."""
    bad = [(r, int(s)) for r, s in enumerate(status_words) if int(s) != STATUS_OK]
    if not bad:
        return
    if own is not None:
        raise own
    ranks = [r for r, _ in bad]
    if all(s == STATUS_RANGE for _, s in bad):
        raise ShardPeerRangeError(f"rank(s) {ranks} reported an activation-range error (RR_ERR_RANGE) in this batch; "
                                  f"this rank ({rank}) discards the gathered logits")
    raise ShardPeerError(f"rank(s) {ranks} failed in their encoder in this batch (status {dict(bad)}); this rank ({rank}) "
                         f"discards the gathered logits")


class ShardedReranker:
    """Wraps a per-rank `encode(pair_begin, pair_end) -> (logits_slice, logits2_slice | None)` and a
    `head(logits, logits2) -> dict` into the sharded forward.  `RerankEngine` provides both on the GPU; the gloo CPU
    tests plug in a CPU stand-in engine to cover the slicing / gather / head plumbing."""

    def __init__(self, encode: Callable, head: Callable, group=None, two_heads: Optional[bool] = None, empty: Optional[Callable] = None,
                 defer_status: bool = False):
        """`empty(n) -> tensor` makes the zero slice a failing rank sends (device / dtype of the logits); `two_heads` tells
        whether that rank must send a second head (both are only needed when `encode` can raise)."""
        self.encode, self.head, self.group, self.two_heads, self.empty = encode, head, group, two_heads, empty
        self.defer_status = defer_status

    def __call__(self, n_pairs: int):
        rank, world = dist.get_rank(self.group), dist.get_world_size(self.group)
        if not self.defer_status and (_PENDING or _OWN_DEFERRED):
            check_deferred_status()         # earlier deferred batches are settled before a batch that reports immediately
        b, e = shard_range(n_pairs, rank, world)
        own, status = None, STATUS_OK
        try:
            l1, l2 = self.encode(b, e)
        except Exception as ex:      # noqa: BLE001 — the exchange must still happen on this rank (see the module docstring)
            if self.empty is None:
                raise
            own, status = ex, (STATUS_RANGE if isinstance(ex, OverflowError) else STATUS_ERROR)
            l1 = self.empty(e - b)
            l2 = self.empty(e - b) if self.two_heads else None
        full1, full2, st = gather_logits(l1, n_pairs, self.group, l2, status=status, want_status=True, defer_status=self.defer_status)
        if self.defer_status:
            if own is not None:
                _OWN_DEFERRED.append(own)                 # raised by check_deferred_status(), together with the peers
        else:
            _raise_collectively(st.tolist(), rank, own)   # one host read of `world` floats per batch
        return self.head(full1, full2)


def sharded_forward(engine, input_ids, attention_mask, token_type_ids, Bq: int, K: int, image_cls=None,
                    image_patches=None, labels: Optional[torch.Tensor] = None, group=None, want_scores=False,
                    defer_status: bool = False):
    """One rerank batch over all ranks of `group` with `engine` (a RerankEngine) on each rank.  Every rank holds the
    whole id tensors (they are 3 x 8 B per token — 1.2 MB per query of 100 x 512 — against ~10 TFLOP of encoder work) and
    encodes only its pair slice; image-derived per-query work is done for the queries the slice touches."""
    N = Bq * K
    two_heads = engine.arch["loss_fn"] == "2H_BCE"

    def encode(b, e):
        if e <= b:                       # more ranks than pairs: this rank contributes an empty slice
            z = torch.empty(0, dtype=torch.float32, device=input_ids.device)
            return z, (z if two_heads else None)
        r = engine.forward_ids(input_ids, attention_mask, token_type_ids, Bq, K, image_cls, image_patches, None,
                               pair_range=(b, e), want_loss=False)
        return r["logits"][b:e], (r["logits2"][b:e] if two_heads else None)

    def head(l1, l2):
        out = engine.head(l1, l2, labels, Bq, K, want_scores=want_scores, want_order=True)
        # the gathered vectors are views of the exchange buffers, which the next call of the same shape overwrites: hand the
        # caller its own N floats (an eval loop keeps the outputs of many batches)
        out["logits"] = l1.clone()
        if l2 is not None:
            out["logits2"] = l2.clone()
        return out

    def empty(n):
        return torch.zeros(n, dtype=torch.float32, device=input_ids.device)

    return ShardedReranker(encode, head, group, two_heads=two_heads, empty=empty, defer_status=defer_status)(N)


def sharded_forward_lists(engine, input_ids, attention_mask, token_type_ids, list_sizes, image_cls=None, image_patches=None,
                          labels: Optional[torch.Tensor] = None, group=None, want_scores=False, defer_status: bool = False,
                          lengths=None, **packed_kw):
    """`sharded_forward` for lists of unequal length: query q owns list_sizes[q] >= 1 of the N = sum(list_sizes) pairs, stored
    list after list.  The pair slices are cut as there (`shard_range` over N, so a list may straddle ranks); a rank encodes its
    slice over PACKED rows, logits only (`engine.forward_ids_packed(..., pair_lists=...)`: the per-query image features are
    picked per pair through the pair-to-list index), and after the one all-gather every rank runs `engine.head_lists` on the
    full logits.  `lengths`: the N pairs' token counts as the host knows them (spares each rank a device -> host copy);
    `packed_kw`: granule / segment_cost_rows of the packed forward.  Status words, the deferred mode and the collective errors
    are ShardedReranker's.  Returns head_lists' dict (loss, list_loss, order flat and local to each list, scores) plus
    `logits` (/ `logits2`)."""
    sizes = [int(k) for k in list_sizes]
    assert sizes and min(sizes) >= 1, "every list holds at least one candidate"
    N = sum(sizes)
    assert input_ids.shape[0] == N, f"{input_ids.shape[0]} pairs for lists of {N} candidates"
    two_heads = engine.arch["loss_fn"] == "2H_BCE"
    pair_lists = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))

    def encode(b, e):
        if e <= b:                       # more ranks than pairs: this rank contributes an empty slice
            z = torch.empty(0, dtype=torch.float32, device=input_ids.device)
            return z, (z if two_heads else None)
        r = engine.forward_ids_packed(input_ids[b:e], attention_mask[b:e], None if token_type_ids is None else token_type_ids[b:e],
                                      None, None, image_cls, image_patches, None, pair_lists=pair_lists[b:e],
                                      lengths=None if lengths is None else lengths[b:e], want_loss=False, **packed_kw)
        return r["logits"], (r["logits2"] if two_heads else None)

    def head(l1, l2):
        out = engine.head_lists(l1, l2, labels, sizes, want_scores=want_scores, want_order=True)
        out["logits"] = l1.clone()       # the gathered vectors are views of the exchange buffers (see sharded_forward)
        if l2 is not None:
            out["logits2"] = l2.clone()
        return out

    def empty(n):
        return torch.zeros(n, dtype=torch.float32, device=input_ids.device)

    return ShardedReranker(encode, head, group, two_heads=two_heads, empty=empty, defer_status=defer_status)(N)


# ---- a passage bank split over ranks ------------------------------------------------------------------------------------------------
# A bank cannot be replicated like weights.  Every rank holds the passages of its slice of the corpus in a bank of its own (rank
# r's passages are the global indices part_offsets[r] .. part_offsets[r + 1] - 1), the QUERIES are the caller's to replicate (every
# rank calls with the same query tensors), every rank searches its bank, the k-lists travel with ONE all-gather and are merged on
# every rank by rr_bank_merge_topk (include/rerank_mi355.h, THE MERGED LIST): with the exact search the result is, byte for byte,
# the search of one bank holding the whole corpus; with a PlaidSearch it is BY DEFINITION the merge of the per-rank pruned searches
# (each rank keeps its own ndocs).  The merged winners are then reranked where their embeddings live (sharded_retrieve_and_rerank):
# the owner of a passage computes its logit, no embedding travels, and nothing balances that work between ranks: a query whose
# winners all live on one rank is that rank's to rerank alone.  Errors are collective as described at the top of the module.
# RCCL with more than one rank has never executed in this project's tests: this path rests on the gloo tests
# (tests/test_sharding_bank_gloo.py) and on in-process GPU tests that run the "ranks" one after another (tests/test_gpu_bank_merge.py).
class _BlockPlan:
    """Preallocated buffers of one (device, dtype, world, block length) exchange of equal blocks; the last word of a block is its
    rank's status.  A search's block is int32 [nq * k indices | nq * k score bits | nq counts | status word], a rerank's float32
    [heads * nq * k logits | status word]."""

    def __init__(self, device, dtype, world: int, blk: int):
        self.world, self.blk = world, blk
        self.send = torch.zeros(blk, dtype=dtype, device=device)
        self.recv = torch.empty(world * blk, dtype=dtype, device=device)
        self.host = None


_BLOCK_PLANS = None


def _block_plan(device, dtype, world, blk, group=None) -> _BlockPlan:
    from collections import OrderedDict
    global _BLOCK_PLANS
    if _BLOCK_PLANS is None:
        _BLOCK_PLANS = OrderedDict()
    key = (str(device), dtype, world, blk, id(group) if group is not None else 0)
    p = _BLOCK_PLANS.get(key)
    if p is None:
        p = _BLOCK_PLANS[key] = _BlockPlan(device, dtype, world, blk)
        while len(_BLOCK_PLANS) > _MAX_PLANS:
            _BLOCK_PLANS.popitem(last=False)
    else:
        _BLOCK_PLANS.move_to_end(key)
    return p


def _all_gather(recv: torch.Tensor, send: torch.Tensor, plan, group) -> None:
    """One all_gather_into_tensor; under gloo, device tensors are staged through pinned host memory (plan.host), as gather_logits
    does for the one-GPU rehearsal."""
    if send.is_cuda and dist.get_backend(group) == "gloo":
        if plan.host is None:
            plan.host = (torch.empty_like(send, device="cpu").pin_memory(), torch.empty_like(recv, device="cpu").pin_memory())
        plan.host[0].copy_(send)
        dist.all_gather_into_tensor(plan.host[1], plan.host[0], group=group)
        recv.copy_(plan.host[1])
    else:
        dist.all_gather_into_tensor(recv, send, group=group)


def exchange_bank_results(local, part_offsets, k: int, group=None, merge: Optional[Callable] = None, engine=None,
                          n_queries: Optional[int] = None, device=None) -> dict:
    """The k-lists of every rank's bank search merged into the global list, on every rank alike.  `local`: this rank's
    {"indices" int32 [nq, k] LOCAL bank indices, "scores" float32 [nq, k], "counts" int32 [nq]} (passage_bank.search_bank_part),
    or a callable that returns it (the local search: then `n_queries`, and `device` unless `engine` is given, say what a rank
    whose search raised sends).  `part_offsets`: the world + 1 host offsets of the ranks' banks (ShardedBank.refresh).  ONE
    all_gather_into_tensor of an int32 block per rank; the merge then reads the received block in place, through strides:
    `merge`(indices, scores, counts, part_offsets, k, part_stride=, count_stride=, want_parts=True), default
    `engine`.bank_merge_topk.  Returns its dict {"indices" global, "scores", "counts", "parts"} plus "part_offsets".
    A rank whose local search raised still takes part, with counts 0 and its status word set; every rank raises after the
    exchange: that rank its own exception, the others ShardPeerError."""
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    own, status = None, STATUS_OK
    if callable(local):
        try:
            local = local()
        except Exception as ex:      # noqa: BLE001 — the exchange must still happen on this rank
            own, status, local = ex, (STATUS_RANGE if isinstance(ex, OverflowError) else STATUS_ERROR), None
    k = int(k)
    if local is not None:
        nq, device = int(local["indices"].shape[0]), local["indices"].device
        assert tuple(local["indices"].shape) == (nq, k) == tuple(local["scores"].shape) and local["counts"].numel() == nq, \
            f"a rank's lists are [n_queries, {k}] with one count per query"
    else:
        if n_queries is None or (device is None and engine is None):
            raise own
        nq, device = int(n_queries), (engine.device if device is None else device)
    w = nq * k
    p = _block_plan(device, torch.int32, world, 2 * w + nq + 1, group)
    if local is not None:
        p.send[:w].copy_(local["indices"].reshape(-1))
        p.send[w:2 * w].copy_(local["scores"].reshape(-1).view(torch.int32))
        p.send[2 * w:2 * w + nq].copy_(local["counts"].reshape(-1))
    else:
        p.send[2 * w:2 * w + nq].zero_()
    p.send[p.blk - 1] = status
    _all_gather(p.recv, p.send, p, group)
    blocks = p.recv.view(world, p.blk)
    _raise_collectively(blocks[:, p.blk - 1].tolist(), rank, own)      # one host read of `world` words per search
    if merge is None:
        if engine is None:
            raise ValueError("exchange_bank_results: give the engine whose bank_merge_topk merges, or a merge function")
        merge = engine.bank_merge_topk
    out = merge(blocks[:, :w].unflatten(1, (nq, k)), blocks[:, w:2 * w].view(torch.float32).unflatten(1, (nq, k)),
                blocks[:, 2 * w:2 * w + nq], part_offsets, k, part_stride=p.blk, count_stride=p.blk, want_parts=True)
    out["part_offsets"] = [int(x) for x in part_offsets]
    return out


class ShardedBank:
    """This rank's PassageBank as one part of a corpus split over the ranks of `group`, rank after rank in corpus order.
    `refresh()` is a load-time collective: it all-gathers every rank's passage count into `part_offsets` and the passage ids
    (all_gather_object) into the global id table `ids`, and records the bank's `generation` (raised by PassageBank.remove and by
    PassageBank.clear); call it again after adds, after a removal (each rank removes locally, then all refresh) and after a clear:
    until then a search raises, also when the bank has been refilled to its old count.  `search` is the local search plus the
    exchange.  The queries are the caller's to replicate: every rank passes the same `query_li`.  A pruned search (`plaid`) needs
    codes on every rank: compressed banks, or fp16 banks with a centroid table (PassageBank.set_centroids), each rank's its own."""

    def __init__(self, bank, group=None):
        self.bank, self.group = bank, group
        self.part_offsets = None
        self.ids = None
        self.generation = None

    def refresh(self) -> None:
        world = dist.get_world_size(self.group)
        counts = [None] * world
        dist.all_gather_object(counts, len(self.bank), group=self.group)
        tables = [None] * world
        dist.all_gather_object(tables, list(self.bank.table.ids), group=self.group)
        assert [len(t) for t in tables] == counts
        self.part_offsets = [0]
        for c in counts:
            self.part_offsets.append(self.part_offsets[-1] + int(c))
        if self.part_offsets[-1] >= 1 << 31:
            raise OverflowError(f"ShardedBank: {self.part_offsets[-1]} passages (global indices are int32)")
        self.ids = [pid for t in tables for pid in t]
        self.generation = getattr(self.bank, "generation", 0)

    def search_merged(self, engine, query_li, k: int, plaid=None, filter=None, merge: Optional[Callable] = None) -> dict:
        """The merged result on the device, as exchange_bank_results returns it (global indices, scores, counts, parts)."""
        from .passage_bank import search_bank_part
        if self.part_offsets is None:
            raise RuntimeError("ShardedBank: call refresh() (on every rank) before the first search, and again after adds")
        rank = dist.get_rank(self.group)
        if self.part_offsets[rank + 1] - self.part_offsets[rank] != len(self.bank) or self.generation != getattr(self.bank, "generation", 0):
            raise RuntimeError("ShardedBank: the bank has changed since refresh(): call it again on every rank")
        return exchange_bank_results(lambda: search_bank_part(engine, self.bank, query_li, k, plaid, filter), self.part_offsets, k,
                                     self.group, merge=merge, engine=engine, n_queries=int(query_li.shape[0]))

    def search(self, engine, query_li, k: int, plaid=None, filter=None):
        """The k best passages of the WHOLE corpus per query: this rank searches its bank with k_local = min(k, len(bank))
        (the exact search, or with `plaid` / `filter`, a BankFilter of THIS rank's bank, what PassageBank.search runs for
        them), one all-gather, the merge.  Returns (passage_ids: per query the ids best first, at their true length; scores
        float32 [n_queries, k] on the device; counts int32 [n_queries]; parts int32 [n_queries, k]: the rank that holds each
        winner), the same on every rank.  Copies the merged indices to the host (synchronises)."""
        r = self.search_merged(engine, query_li, k, plaid, filter)
        ids = [[self.ids[g] for g in row[:c]] for row, c in zip(r["indices"].tolist(), r["counts"].tolist())]
        return ids, r["scores"], r["counts"], r["parts"]


def _rerank_heads(model) -> int:
    return 2 if model.engine.arch["loss_fn"] == "2H_BCE" else 1


def rerank_owned(model, bank, merged: dict, part: int, query_late_interaction, query_mask, **kw) -> torch.Tensor:
    """The logits of the merged winners that live in `bank`, part `part` of the corpus: a zeroed float32 [heads * nq * k] buffer
    (heads: 2 for 2H_BCE) with the logit of every winner whose part is `part` at its merged position q * k + i (the second head
    behind the first).  One engine.forward_interaction_bank over those winners, lists of unequal length per query; a part that
    owns none runs no forward.  `merged`: exchange_bank_results' dict.  Process-free: a test runs the parts one after another."""
    parts, idx = merged["parts"], merged["indices"]
    nq, k = int(parts.shape[0]), int(parts.shape[1])
    heads = _rerank_heads(model)
    buf = torch.zeros(heads * nq * k, dtype=torch.float32, device=idx.device)
    mine = (parts == int(part)).reshape(-1)
    pos = mine.nonzero().reshape(-1)                                    # merged positions, query after query
    if pos.numel() == 0:
        return buf
    local = (idx.reshape(-1)[pos] - int(merged["part_offsets"][part])).tolist()
    per_query = torch.bincount(torch.div(pos, k, rounding_mode="floor"), minlength=nq).tolist()
    sel = [q for q, n in enumerate(per_query) if n]
    ids = [bank.table.ids[j] for j in local]
    sel_t = torch.tensor(sel, device=query_late_interaction.device)
    r = model.engine.forward_interaction_bank(bank, query_late_interaction.index_select(0, sel_t),
                                              query_mask.reshape(nq, -1).index_select(0, sel_t.to(query_mask.device)), ids, None, None,
                                              None, list_sizes=[per_query[q] for q in sel], want_loss=False, want_order=True, **kw)
    buf[pos] = r["logits"]
    if heads == 2:
        buf[pos + nq * k] = r["logits2"]
    return buf


def combine_owned(buffers: torch.Tensor, parts: torch.Tensor) -> torch.Tensor:
    """buffers [n_parts, heads * nq * k] (rerank_owned's, part after part), parts int32 [nq, k] -> [heads, nq * k]: every merged
    position taken from its owner's buffer with one torch.gather whose index is computed from `parts` on the device.  No sum: the
    bits, -0 included, arrive unchanged.  A position behind a query's count (part -1) reads part 0's zero."""
    n = parts.numel()
    heads = int(buffers.shape[1]) // n
    assert heads * n == buffers.shape[1], f"buffers {tuple(buffers.shape)} for {n} merged positions"
    owner = parts.reshape(1, 1, n).clamp(min=0).to(torch.int64).expand(1, heads, n)
    return torch.gather(buffers.unflatten(1, (heads, n)), 0, owner).view(heads, n)


def head_over_merged(model, logits: torch.Tensor, counts, k: int, labels=None, **kw):
    """The scoring head over the merged lists: `logits` [heads, nq * k] (combine_owned), list q the first counts[q] positions of
    row q.  Returns the model's RerankOutput (logits list after list, order local to each list)."""
    sizes = [int(c) for c in counts]
    if min(sizes) < 1:
        raise ValueError(f"query {sizes.index(min(sizes))} found no candidate")
    dev = logits.device
    gather = torch.cat([torch.arange(c, dtype=torch.int32) + q * k for q, c in enumerate(sizes)]).to(dev)
    l1 = logits[0].contiguous()
    l2 = logits[1].contiguous() if logits.shape[0] == 2 else None
    N = sum(sizes)
    kw.setdefault("want_order", True)
    r = model.engine.head_lists(l1, l2, model._labels(labels, N), sizes, gather=gather, **kw)
    r["logits"] = l1.index_select(0, gather.long())
    if l2 is not None:
        r["logits2"] = l2.index_select(0, gather.long())
    return model._output(r, model._flat_logits(r))


def sharded_retrieve_and_rerank(model, shard: ShardedBank, query_late_interaction, query_mask, k: int, plaid=None, filter=None,
                                labels=None, **kw):
    """InteractionRerankModel.retrieve_and_rerank over a bank split over ranks: (passage_ids, RerankOutput), the same on every
    rank.  1. shard.search (local search, one all-gather, the merge).  2. every rank runs forward_interaction_bank over the merged
    winners whose part is its own (rerank_owned).  3. / 4. the zeroed [heads * nq * k] buffers travel with one all-gather.
    5. every position is taken from its owner's block (combine_owned).  6. the head runs over the merged lists with
    list_sizes = counts, redundantly on every rank, as sharded_forward_lists does.  A query that found no candidate raises
    ValueError on every rank, as retrieve_and_rerank does; an exception inside one rank's forward is collective (ShardPeerError
    on the others).  The owner computes: nothing balances the rerank work between ranks.  `kw`: granule / segment_cost_rows /
    fusion_from_li ... of forward_interaction_bank."""
    eng, group = model.engine, shard.group
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    merged = shard.search_merged(eng, query_late_interaction, k, plaid, filter)
    counts = merged["counts"].tolist()
    if min(counts) < 1:
        raise ValueError(f"sharded_retrieve_and_rerank: query {counts.index(min(counts))} found no candidate")
    nq, k = int(merged["parts"].shape[0]), int(k)
    heads = _rerank_heads(model)
    own, status = None, STATUS_OK
    try:
        buf = rerank_owned(model, shard.bank, merged, rank, query_late_interaction, query_mask, **kw)
    except Exception as ex:      # noqa: BLE001 — the exchange must still happen on this rank
        own, status = ex, (STATUS_RANGE if isinstance(ex, OverflowError) else STATUS_ERROR)
        buf = torch.zeros(heads * nq * k, dtype=torch.float32, device=merged["parts"].device)
    p = _block_plan(buf.device, torch.float32, world, heads * nq * k + 1, group)
    p.send[:buf.numel()].copy_(buf)
    p.send[p.blk - 1] = float(status)
    _all_gather(p.recv, p.send, p, group)
    blocks = p.recv.view(world, p.blk)
    _raise_collectively(blocks[:, p.blk - 1].tolist(), rank, own)
    logits = combine_owned(blocks[:, :heads * nq * k], merged["parts"])
    ids = [[shard.ids[g] for g in row[:c]] for row, c in zip(merged["indices"].tolist(), counts)]
    return ids, head_over_merged(model, logits, counts, k, labels=labels)
