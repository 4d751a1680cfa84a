"""CPU, gloo, world 2: a ShardedBank and a removal.  refresh() records the bank's generation beside its passage count, and
search_merged raises the "refresh first" error when either differs.  The case the count alone cannot see: a rank removes one
passage and adds one, so its bank is as long as before but holds other passages under the old numbers; a search then would hand
out stale ids.  It raises instead, on that rank and (through the exchange) nowhere silently; after refresh() on every rank the
search answers with the new ids.  The same through clear(): a rank clears its bank and refills it to the old count with other ids;
there the stand-in runs PassageBank.clear itself (over a stub of the C call), so that what raises the generation is the library's
own method.  CPU stand-ins for the engine and the banks, as tests/test_sharding_bank_gloo.py has them."""
import numpy as np
import torch.distributed as dist

from test_sharding_bank_gloo import K, NQ, SIZES, _CpuBank, _CpuBankEngine, _init, _queries, _stable_desc, _table
from test_sharding_gloo import _run_world

from rmr_amd import BankTable, PassageBank

WORLD = 2
CHANGED_RANK, GONE, NEW_ID = 0, 4, "d100"


class _RemovableBank(_CpuBank):
    """_CpuBank with PassageBank's generation, and a removal followed by an equal-sized add."""
    generation = 0

    def remove_then_add(self, local, new_id, new_scores):
        ids = self.table.ids
        self.table.ids = ids[:local] + ids[local + 1:] + [new_id]
        self.scores = np.concatenate([np.delete(self.scores, local, axis=1), new_scores[:, None]], axis=1)
        self.generation += 1


class _ClearStub:
    """What PassageBank.clear calls of the C library."""

    def __init__(self):
        self.cleared = 0

    def rr_bank_clear(self, h):
        self.cleared += 1
        return 0


class _ClearableBank(_CpuBank):
    """_CpuBank that is cleared by PassageBank.clear itself: the generation is whatever the library's method makes of it."""
    generation = PassageBank.generation
    clear, _check = PassageBank.clear, PassageBank._check

    def __init__(self, world, rank):
        super().__init__(world, rank)
        ids, self.table = self.table.ids, BankTable()
        self.table.append(ids, [1] * len(ids))
        self.lib, self.h = _ClearStub(), None

    def refill(self, ids, scores):
        assert len(self.table) == 0 and self.lib.cleared == 1
        self.table.append(ids, [1] * len(ids))
        self.scores = scores


def _refill():
    """Rank CHANGED_RANK's bank after the clear: as many passages as before, other ids, the old scores column by column reversed."""
    n0 = SIZES[WORLD][CHANGED_RANK]
    return [f"d{200 + j}" for j in range(n0)], np.ascontiguousarray(_table(WORLD)[:, :n0][:, ::-1])


def _clear_worker(rank, world, port, q):
    _init(rank, world, port)
    try:
        from rmr_amd.sharding import ShardedBank
        ql, _ = _queries()
        eng = _CpuBankEngine()
        bank = _ClearableBank(world, rank)
        shard = ShardedBank(bank)
        shard.refresh()
        before = shard.search(eng, ql, K)[0]
        if rank == CHANGED_RANK:
            bank.clear()
            bank.refill(*_refill())
        assert len(bank) == SIZES[world][rank], "the count has not changed on any rank"
        raised = None
        if rank == CHANGED_RANK:                                  # refused before the collective: the other rank does not enter it
            import rmr_amd.sharding as S
            exchange = S.exchange_bank_results

            def went_through(*a, **kw):                           # a search that is not refused must not wait for the other rank
                raise AssertionError("the search reached the exchange")
            S.exchange_bank_results = went_through
            try:
                shard.search(eng, ql, K)
            except RuntimeError as ex:
                raised = str(ex)
            except AssertionError as ex:
                raised = f"NOT REFUSED: {ex}"
            finally:
                S.exchange_bank_results = exchange
        dist.barrier()
        shard.refresh()
        assert shard.generation == bank.generation
        after = shard.search(eng, ql, K)[0]
        q.put((rank, before, raised, after))
    finally:
        dist.destroy_process_group()


def _new_scores():
    return np.linspace(3.0, 4.5, NQ).astype(np.float32)          # above every finite entry of the table but its +inf


def _worker(rank, world, port, q):
    _init(rank, world, port)
    try:
        from rmr_amd.sharding import ShardedBank
        ql, _ = _queries()
        eng = _CpuBankEngine()
        bank = _RemovableBank(world, rank)
        shard = ShardedBank(bank)
        shard.refresh()
        assert shard.generation == 0
        before = shard.search(eng, ql, K)[0]
        if rank == CHANGED_RANK:
            bank.remove_then_add(GONE, NEW_ID, _new_scores())
        assert len(bank) == SIZES[world][rank], "the count has not changed on any rank"
        raised = None
        if rank == CHANGED_RANK:                                  # refused before the collective: the other rank does not enter it
            try:
                shard.search(eng, ql, K)
            except RuntimeError as ex:
                raised = str(ex)
        dist.barrier()
        shard.refresh()
        assert shard.generation == bank.generation
        after = shard.search(eng, ql, K)[0]
        q.put((rank, before, raised, after))
    finally:
        dist.destroy_process_group()


def test_a_removal_and_an_equal_sized_add_need_a_refresh():
    res = _run_world(_worker, WORLD, ())
    t = _table(WORLD)
    n0 = SIZES[WORLD][0]
    changed = np.concatenate([np.delete(t[:, :n0], GONE, axis=1), _new_scores()[:, None], t[:, n0:]], axis=1)
    ids = [f"d{g}" for g in range(n0) if g != GONE] + [NEW_ID] + [f"d{g}" for g in range(n0, t.shape[1])]
    want_before = [[f"d{g}" for g in _stable_desc(row)[:K]] for row in t]
    want_after = [[ids[g] for g in _stable_desc(row)[:K]] for row in changed]
    assert any(NEW_ID in row for row in want_after) and want_after != want_before
    for rank, before, raised, after in res:
        assert before == want_before and after == want_after, f"rank {rank}"
        if rank == CHANGED_RANK:
            assert raised is not None and "refresh()" in raised and "changed" in raised
        else:
            assert raised is None


def test_a_clear_and_a_refill_to_the_same_count_need_a_refresh():
    assert CHANGED_RANK == 0
    res = _run_world(_clear_worker, WORLD, ())
    t = _table(WORLD)
    n0 = SIZES[WORLD][0]
    new_ids, new_scores = _refill()
    changed = np.concatenate([new_scores, t[:, n0:]], axis=1)
    ids = new_ids + [f"d{g}" for g in range(n0, t.shape[1])]
    want_before = [[f"d{g}" for g in _stable_desc(row)[:K]] for row in t]
    want_after = [[ids[g] for g in _stable_desc(row)[:K]] for row in changed]
    assert any(set(new_ids) & set(row) for row in want_after) and want_after != want_before
    for rank, before, raised, after in res:
        assert before == want_before and after == want_after, f"rank {rank}"
        if rank == CHANGED_RANK:
            assert raised is not None and "refresh()" in raised and "changed" in raised, f"a search after clear() and a refill: {raised}"
        else:
            assert raised is None
