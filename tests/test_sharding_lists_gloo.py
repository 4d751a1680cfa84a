"""CPU, gloo, world 2 and 8: rmr_amd.sharding.sharded_forward_lists (pair slices cut over N = sum of the list sizes, so that lists
straddle rank borders; the packed forward in its logits-only mode on each slice; one all-gather; head_lists on every rank) gives
every rank the logits, orders, list losses and loss of world 1, and an error on one rank is raised on every rank."""
import os

import pytest
import torch
import torch.distributed as dist

from helpers import O
from test_sharding_gloo import _run_world

SIZES = [5, 1, 3, 7, 4, 2, 5, 6, 2]          # N = 35: divisible by neither 2 nor 8, lists straddle the borders of both worlds


class _CpuListEngine:
    """CPU stand-in with the part of RerankEngine's interface sharded_forward_lists uses: forward_ids_packed in its
    logits-only mode (`pair_lists`) and head_lists.  A pair's logit is a fixed function of its token ids and of its QUERY's
    image feature, so a slicing, ordering or pair-to-list mistake shows up in the numbers."""

    def __init__(self, loss_fn, fail=None):
        self.arch = {"loss_fn": loss_fn}
        self.calls, self.fail = [], fail

    def forward_ids_packed(self, ids, am, tt, Bq, K, cls, pat, labels, pair_lists=None, lengths=None, want_loss=True, **kw):
        if self.fail is not None:
            raise self.fail("RR_ERR_RANGE stand-in" if self.fail is OverflowError else "encoder failed")
        assert Bq is None and K is None and labels is None and not want_loss and pair_lists is not None
        assert len(pair_lists) == ids.shape[0] == am.shape[0] and (lengths is None or len(lengths) == ids.shape[0])
        self.calls.append(ids.shape[0])
        f = (ids.double() * torch.arange(1, ids.shape[1] + 1)).sum(1) + cls[pair_lists.long(), 0].double()
        return dict(logits=torch.sin(f).float(), logits2=torch.cos(f).float())

    def head_lists(self, l1, l2, labels, list_sizes, want_scores=False, want_order=True, **kw):
        assert torch.isfinite(l1).all() and l1.numel() == sum(list_sizes)
        ranked = l2 if self.arch["loss_fn"] == "2H_BCE" else l1
        rows = torch.split(ranked, list(list_sizes))
        order = torch.tensor([i for r in rows for i in O.rank_descending_stable(r.tolist())], dtype=torch.int32)
        return dict(order=order, scores=torch.sigmoid(ranked) if want_scores else None,
                    list_loss=torch.stack([r.double().mean().float() for r in rows]), loss=ranked.double().mean().float())


def _inputs():
    N = sum(SIZES)
    ids = torch.randint(1, 1000, (N, 16), generator=torch.Generator().manual_seed(3))
    cls = torch.randn(len(SIZES), 4, generator=torch.Generator().manual_seed(4))
    return ids, cls, list(range(3, 3 + N))


def _single_rank(loss_fn):
    ids, cls, lengths = _inputs()
    eng = _CpuListEngine(loss_fn)
    table = torch.repeat_interleave(torch.arange(len(SIZES)), torch.tensor(SIZES))
    r = eng.forward_ids_packed(ids, ids, ids, None, None, cls, cls, None, pair_lists=table, want_loss=False)
    two = loss_fn == "2H_BCE"
    h = eng.head_lists(r["logits"], r["logits2"] if two else None, None, SIZES)
    return r["logits"].tolist(), r["logits2"].tolist() if two else None, h["order"].tolist(), h["list_loss"].tolist(), h["loss"].item()


def _worker(rank, world, port, loss_fn, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from rmr_amd.sharding import shard_range, sharded_forward_lists
        ids, cls, lengths = _inputs()
        eng = _CpuListEngine(loss_fn)
        outs = []
        for _ in range(2):                                   # the second call reuses the preallocated gather buffers
            out = sharded_forward_lists(eng, ids, ids, ids, SIZES, cls, cls, lengths=lengths, want_scores=True)
            outs.append((out["logits"].tolist(), None if out.get("logits2") is None else out["logits2"].tolist(),
                         out["order"].tolist(), out["list_loss"].tolist(), out["loss"].item()))
        b, e = shard_range(sum(SIZES), rank, world)
        assert eng.calls == [e - b] * 2                      # this rank encoded its slice, and nothing else
        assert outs[0] == outs[1]
        q.put((rank,) + outs[0])
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 8])
@pytest.mark.parametrize("loss_fn", ["BCE", "2H_BCE", "negative_sampling"])
def test_sharded_lists_match_single_rank(world, loss_fn):
    from rmr_amd import shard_range
    N = sum(SIZES)
    assert N % world != 0
    offsets = [sum(SIZES[:i]) for i in range(len(SIZES) + 1)]
    borders = [shard_range(N, r, world)[0] for r in range(1, world)]
    assert any(b not in offsets for b in borders), "no list straddles a rank border"
    want = _single_rank(loss_fn)
    res = _run_world(_worker, world, (loss_fn,))
    assert [r[0] for r in res] == list(range(world))
    for rank, l1, l2, order, list_loss, loss in res:
        assert l1 == want[0] and l2 == want[1]
        assert order == want[2] and list_loss == want[3] and loss == want[4]


def _failing_worker(rank, world, port, bad_rank, exc_name, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from rmr_amd.sharding import ShardPeerError, sharded_forward_lists
        exc = {"OverflowError": OverflowError, "ValueError": ValueError}[exc_name]
        ids, cls, _ = _inputs()
        ok = _CpuListEngine("BCE")
        first = sharded_forward_lists(ok, ids, ids, ids, SIZES, cls, cls)["logits"].tolist()
        eng = _CpuListEngine("BCE", fail=exc if rank == bad_rank else None)
        raised = None
        try:
            sharded_forward_lists(eng, ids, ids, ids, SIZES, cls, cls)
        except Exception as ex:      # noqa: BLE001
            raised = (type(ex).__name__, isinstance(ex, OverflowError), isinstance(ex, ShardPeerError), str(ex))
        t = torch.tensor([float(rank)])
        dist.all_reduce(t)                                   # nobody is stuck in a collective
        again = sharded_forward_lists(ok, ids, ids, ids, SIZES, cls, cls)["logits"].tolist()
        q.put((rank, raised, float(t), first == again))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,exc_name", [(2, "OverflowError"), (8, "ValueError")])
def test_an_error_on_one_rank_is_raised_on_every_rank(world, exc_name):
    bad = 1
    res = _run_world(_failing_worker, world, (bad, exc_name), timeout=240)
    for rank, raised, total, same in res:
        assert raised is not None, f"rank {rank} did not raise"
        name, is_overflow, is_peer, msg = raised
        if rank == bad:
            assert name == exc_name and not is_peer
        else:
            assert is_peer and "[1]" in msg and is_overflow == (exc_name == "OverflowError")
        assert total == float(sum(range(world))) and same
