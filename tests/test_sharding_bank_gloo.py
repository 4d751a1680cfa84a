"""CPU, gloo, world 2 and 3: rmr_amd.sharding.exchange_bank_results (one all-gather of every rank's k-lists, then the merge over the
received block in place) with the merge injected from the host definition rr_util_bank_merge_topk.  The local results are cut from
one random score table, so the expected global answer is a numpy sort of that table; shard sizes are unequal, one is below k, one
shard is empty.  Every rank gets the same bytes; a rank whose local search raises makes every rank raise.  combine_owned on CPU
tensors.  Then the whole path (ShardedBank.refresh / search, sharded_retrieve_and_rerank) over CPU stand-ins for the engine and the
banks: every rank reranks the winners it owns and nothing else, every rank ends with the ids, logits and order of the one table,
and a forward that fails on one rank is raised on every rank."""
import datetime
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist

from test_sharding_gloo import _run_world

NQ, K = 4, 6
SIZES = {2: [11, 3], 3: [9, 0, 5]}            # unequal; 3 and 5 are below k; an empty shard
VALUES = np.array([0.0, -0.0, 2.5, 2.5, -1.0, np.inf, -np.inf, np.nan, 0.75], dtype=np.float32)


def _table(world):
    rng = np.random.default_rng(40 + world)
    n = sum(SIZES[world])
    t = rng.standard_normal((NQ, n)).astype(np.float32)
    ties = rng.random((NQ, n)) < 0.5
    t[ties] = VALUES[rng.integers(0, VALUES.size, size=int(ties.sum()))]
    return t


def _stable_desc(row):
    nan = np.isnan(row)
    mag = np.where(nan, np.float32(0), row) + np.float32(0)
    return np.lexsort((np.arange(row.size), -mag.astype(np.float64), ~nan))


def _local(world, rank):
    """This rank's "search": the k_local = min(k, size) best of its slice of the table, local indices, padded to k."""
    off = np.concatenate([[0], np.cumsum(SIZES[world])])
    t = _table(world)[:, off[rank]:off[rank + 1]]
    kl = min(K, t.shape[1])
    idx = np.full((NQ, K), -1, dtype=np.int32)
    sc = np.full((NQ, K), -np.inf, dtype=np.float32)
    for q in range(NQ):
        o = _stable_desc(t[q])[:kl]
        idx[q, :kl], sc[q, :kl] = o, t[q][o]
    return dict(indices=torch.from_numpy(idx), scores=torch.from_numpy(sc), counts=torch.full((NQ,), kl, dtype=torch.int32)), off.tolist()


def _expected(world):
    t = _table(world)
    off = np.concatenate([[0], np.cumsum(SIZES[world])])
    kk = min(K, t.shape[1])
    idx = np.full((NQ, K), -1, dtype=np.int32)
    sc = np.full((NQ, K), -np.inf, dtype=np.float32)
    parts = np.full((NQ, K), -1, dtype=np.int32)
    for q in range(NQ):
        o = _stable_desc(t[q])[:kk]
        idx[q, :kk], sc[q, :kk] = o, t[q][o]
        parts[q, :kk] = np.searchsorted(off, o, side="right") - 1
    return idx.tobytes(), sc.tobytes(), np.full(NQ, kk, dtype=np.int32).tobytes(), parts.tobytes()


def _host_merge(indices, scores, counts, part_offsets, k, part_stride=None, count_stride=None, want_parts=False):
    """RerankEngine.bank_merge_topk's interface over CPU tensors, through the host definition."""
    from rmr_amd import _lib
    lib = _lib.load()
    P, nq, k_in = indices.shape
    off = np.asarray(part_offsets, dtype=np.int32)
    out = dict(indices=torch.empty((nq, k), dtype=torch.int32), scores=torch.empty((nq, k), dtype=torch.float32),
               counts=torch.empty(nq, dtype=torch.int32), parts=torch.empty((nq, k), dtype=torch.int32))
    rc = lib.rr_util_bank_merge_topk(indices.data_ptr(), scores.data_ptr(), counts.data_ptr(), int(part_stride), int(count_stride), P,
                                     off.ctypes.data, nq, k_in, k, out["indices"].data_ptr(), out["scores"].data_ptr(),
                                     out["counts"].data_ptr(), out["parts"].data_ptr())
    assert rc == 0, rc
    return out


def _init(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))


def _worker(rank, world, port, q):
    _init(rank, world, port)
    try:
        from rmr_amd.sharding import exchange_bank_results
        local, off = _local(world, rank)
        outs = []
        for _ in range(2):                                   # the second call reuses the preallocated buffers
            r = exchange_bank_results(local, off, K, merge=_host_merge)
            assert r["part_offsets"] == off
            outs.append(tuple(r[n].numpy().tobytes() for n in ("indices", "scores", "counts", "parts")))
        assert outs[0] == outs[1]
        q.put((rank,) + outs[0])
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_every_rank_gets_the_bytes_of_the_global_sort(world):
    assert min(SIZES[world]) < K and len(set(SIZES[world])) == world and (world == 2 or 0 in SIZES[world])
    want = _expected(world)
    res = _run_world(_worker, world, ())
    assert [r[0] for r in res] == list(range(world))
    for rank, *got in res:
        assert tuple(got) == want, f"rank {rank}"


def _failing_worker(rank, world, port, bad_rank, exc_name, q):
    _init(rank, world, port)
    try:
        from rmr_amd.sharding import ShardPeerError, exchange_bank_results
        exc = {"OverflowError": OverflowError, "ValueError": ValueError}[exc_name]
        local, off = _local(world, rank)

        def search():
            if rank == bad_rank:
                raise exc("the local search failed")
            return local
        first = exchange_bank_results(local, off, K, merge=_host_merge)["indices"].tolist()
        raised = None
        try:
            exchange_bank_results(search, off, K, merge=_host_merge, n_queries=NQ, device="cpu")
        except Exception as ex:      # noqa: BLE001
            raised = (type(ex).__name__, isinstance(ex, OverflowError), isinstance(ex, ShardPeerError), str(ex))
        t = torch.tensor([float(rank)])
        dist.all_reduce(t)                                   # nobody is stuck in a collective
        again = exchange_bank_results(lambda: local, off, K, merge=_host_merge, n_queries=NQ, device="cpu")["indices"].tolist()
        q.put((rank, raised, float(t), first == again))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,exc_name", [(2, "OverflowError"), (3, "ValueError")])
def test_a_failed_local_search_is_raised_on_every_rank(world, exc_name):
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


@pytest.mark.parametrize("heads", [1, 2])
def test_combine_owned_takes_every_position_from_its_owner(heads):
    from rmr_amd.sharding import combine_owned
    nq, k, n_parts = 3, 5, 3
    gen = torch.Generator().manual_seed(7)
    parts = torch.randint(-1, n_parts, (nq, k), generator=gen, dtype=torch.int32)
    parts[0, 0], parts[2, 4] = -1, 2
    truth = torch.randn(heads, nq * k, generator=gen)
    truth[0, 3] = -0.0
    parts[0, 3] = 1
    owned = parts.reshape(-1)[None, None, :] == torch.arange(n_parts)[:, None, None]
    blocks = torch.zeros(n_parts, heads * nq * k + 1)                      # as received: a status word behind every buffer
    blocks[:, :-1] = (truth[None] * owned).reshape(n_parts, -1)
    blocks[:, :-1][~owned.expand(n_parts, heads, nq * k).reshape(n_parts, -1)] = 0.0
    got = combine_owned(blocks[:, :-1], parts)
    want = torch.where(parts.reshape(1, -1) >= 0, truth, torch.zeros(()))
    assert got.shape == (heads, nq * k) and torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert got.view(torch.int32)[0, 3].item() == -(1 << 31)                # the -0 of its owner, not a sum's +0


# ---- the whole sharded path over CPU stand-ins: ShardedBank.refresh / search and sharded_retrieve_and_rerank ---------------------------
class _Table:
    def __init__(self, ids):
        self.ids = ids


class _CpuBank:
    """A rank's slice of the score table under the ids "d<global number>"."""

    def __init__(self, world, rank):
        off = np.concatenate([[0], np.cumsum(SIZES[world])])
        self.scores = _table(world)[:, off[rank]:off[rank + 1]]
        self.table = _Table([f"d{g}" for g in range(off[rank], off[rank + 1])])

    def __len__(self):
        return len(self.table.ids)


def _logit(pid, qrow):
    return float(np.sin(np.float64(0.37 * int(pid[1:]) + float(qrow[0, 0]))))


class _CpuBankEngine:
    """The part of RerankEngine the sharded bank path uses: bank_search (an exact search: no counts), bank_merge_topk (the host
    definition), forward_interaction_bank over lists of unequal length (a pair's logit is a fixed function of its passage id and
    of its QUERY's first value) and head_lists."""
    device = torch.device("cpu")

    def __init__(self, loss_fn="BCE", fail=None):
        self.arch = {"loss_fn": loss_fn}
        self.fail, self.pairs = fail, []

    def bank_search(self, bank, q, k):
        assert 1 <= k <= len(bank)
        idx = np.stack([_stable_desc(row)[:k] for row in bank.scores]).astype(np.int32)
        return dict(indices=torch.from_numpy(idx), scores=torch.from_numpy(np.take_along_axis(bank.scores, idx.astype(np.int64), 1)))

    bank_merge_topk = staticmethod(_host_merge)

    def forward_interaction_bank(self, bank, q, qm, ids, Bq, K, labels, list_sizes=None, want_loss=True, want_order=False, **kw):
        if self.fail is not None:
            raise self.fail("the forward failed")
        assert Bq is None and K is None and labels is None and not want_loss and q.shape[0] == len(list_sizes) == qm.shape[0]
        assert sum(list_sizes) == len(ids) and min(list_sizes) >= 1 and all(i in bank.table.ids for i in ids)
        self.pairs.append(len(ids))
        rows = [qi for qi, n in enumerate(list_sizes) for _ in range(n)]
        l1 = torch.tensor([_logit(pid, q[qi]) for pid, qi in zip(ids, rows)], dtype=torch.float32)
        return dict(logits=l1, logits2=-l1)

    def head_lists(self, l1, l2, labels, list_sizes, gather=None, want_order=True, **kw):
        ranked = (l2 if self.arch["loss_fn"] == "2H_BCE" else l1)[gather.long()]
        rows = torch.split(ranked, list(list_sizes))
        order = torch.tensor([i for r in rows for i in _stable_desc(r.numpy()).tolist()], dtype=torch.int32)
        return dict(order=order, loss=ranked.double().mean().float(), list_loss=torch.stack([r.double().mean().float() for r in rows]))


class _CpuBankModel:
    def __init__(self, engine):
        self.engine = engine

    def _labels(self, labels, N):
        return None

    @staticmethod
    def _output(r, logits):
        return dict(r, logits=logits)

    def _flat_logits(self, r):
        return r["logits"]


def _queries():
    return torch.randn(NQ, 3, 4, generator=torch.Generator().manual_seed(12)), torch.ones(NQ, 3)


def _rerank_worker(rank, world, port, loss_fn, bad_rank, q):
    _init(rank, world, port)
    try:
        from rmr_amd.sharding import ShardedBank, ShardPeerError, sharded_retrieve_and_rerank
        ql, qm = _queries()
        eng = _CpuBankEngine(loss_fn)
        model = _CpuBankModel(eng)
        shard = ShardedBank(_CpuBank(world, rank))
        shard.refresh()
        assert shard.part_offsets == np.concatenate([[0], np.cumsum(SIZES[world])]).tolist() and len(shard.ids) == sum(SIZES[world])
        ids, scores, counts, parts = shard.search(eng, ql, K)
        got_ids, out = sharded_retrieve_and_rerank(model, shard, ql, qm, K)
        assert got_ids == ids
        mine = int((parts == rank).sum())
        assert eng.pairs == ([mine] if mine else []), "this rank ran the forward over the winners it owns, and nothing else"
        raised = None
        if bad_rank >= 0:
            bad = _CpuBankModel(_CpuBankEngine(loss_fn, fail=ValueError if rank == bad_rank else None))
            try:
                sharded_retrieve_and_rerank(bad, shard, ql, qm, K)
            except Exception as ex:      # noqa: BLE001
                raised = (type(ex).__name__, isinstance(ex, ShardPeerError))
            t = torch.tensor([1.0])
            dist.all_reduce(t)                               # nobody is stuck in a collective
            assert float(t) == world
        q.put((rank, ids, scores.numpy().tobytes(), parts.numpy().tobytes(), out["logits"].tolist(),
               None if out.get("logits2") is None else out["logits2"].tolist(), out["order"].tolist(), raised))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,loss_fn", [(2, "2H_BCE"), (3, "BCE")])
def test_sharded_search_and_rerank_over_stand_ins(world, loss_fn):
    want_i, want_s, _, want_p = _expected(world)
    idx = np.frombuffer(want_i, dtype=np.int32).reshape(NQ, K)
    ql, _ = _queries()
    want_ids = [[f"d{g}" for g in row] for row in idx.tolist()]
    want_logits = [np.float32(_logit(pid, ql[qi])).item() for qi, row in enumerate(want_ids) for pid in row]
    bad = 2 if world == 3 else -1                        # (rank 1 holds the empty shard: it owns no winner and runs no forward)
    res = _run_world(_rerank_worker, world, (loss_fn, bad))
    assert len({r[6].__repr__() for r in res}) == 1
    for rank, ids, sc, parts, l1, l2, order, raised in res:
        assert ids == want_ids and sc == want_s and parts == want_p, f"rank {rank}"
        assert l1 == want_logits and (l2 == [-x for x in want_logits] if loss_fn == "2H_BCE" else l2 is None)
        ranked = np.array(l2 if loss_fn == "2H_BCE" else l1, dtype=np.float32).reshape(NQ, K)
        assert order == [i for row in ranked for i in _stable_desc(row).tolist()]
        if bad >= 0:
            assert raised == (("ValueError", False) if rank == bad else ("ShardPeerError", True))
