"""GPU: rr_bank_search_filtered_sparse where its counted selection changes path ("CANDIDATE FILTERS", include/rerank_mi355.h):
9 000 passages of one row at D 64 (three selection slices of 4096), with per-row candidate counts on both sides of every border
of topk_select_counted_kernel: 0 and 1, k (1024) and its neighbours, one slice (4096) and its neighbours, two slices and the
whole range.  And the first and the last stage alone, through their diagnostic operators.

Every comparison is against rr_bank_search_filtered on the same arguments, as bytes, and against the numpy restatement
bank_filter_ref.filtered_topk on the exact scores (bank_li_scores' maxsim); never against the sparse form itself."""
import functools

import numpy as np
import pytest
import torch

import bank_filter_ref as ref
from test_gpu_bank_li_scores import POISON, _queries
from test_gpu_bank_search import IPOISON
from test_gpu_bank_search_filter import _checked, _dev_bits, _outputs, _range_bits, _same_bytes, _stream
from test_gpu_bank_search_sparse import _sparse_equals_dense
from test_gpu_li_scores import _engine as _bare_engine

pytestmark = pytest.mark.gpu

D, PB, LQ = 64, 9000, 8
COUNTS = (0, 1, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 8193, 9000)
TWINS_A = tuple(range(4091, 4102))          # equal scores on both sides of place 4096 when every bit is set
TWINS_B = tuple(range(4191, 4202))          # ... and when the first 100 passages are filtered out (places 4091 .. 4101)


@functools.lru_cache(maxsize=None)
def _case():
    """(engine, bank of 9 000 one-row passages, 11 queries, their exact scores float32 [11, 9000]).  The passages TWINS_A and
    TWINS_B hold one and the same row, the mean of query 0's tokens: equal scores, and query 0's best."""
    eng = _bare_engine(D)
    q = _queries(len(COUNTS), LQ, D, seed=21)
    gen = torch.Generator(device="cuda").manual_seed(22)
    li = torch.nn.functional.normalize(torch.randn(PB, 1, D, generator=gen, device="cuda"), dim=-1)
    li[list(TWINS_A + TWINS_B), 0] = torch.nn.functional.normalize(q[0].mean(0), dim=-1)
    bank = eng.create_bank(PB, PB)
    bank.add(list(range(PB)), li.half(), torch.ones(PB, 1), lengths=[1] * PB)
    nq = q.shape[0]
    ms = eng.bank_li_scores(bank, q, list(range(PB)) * nq, pair_query=np.repeat(np.arange(nq), PB), padded_len=1)["maxsim"]
    torch.cuda.synchronize()
    return eng, bank, q, ms.reshape(nq, PB).cpu().numpy()


def _rows_of(counts, seed):
    rng = np.random.default_rng(seed)
    allowed = np.zeros((len(counts), PB), dtype=bool)
    for r, c in enumerate(counts):
        allowed[r, rng.choice(PB, size=c, replace=False)] = True
    return allowed


def _equals_dense_and_ref(eng, bank, q, scores, allowed, k, what):
    gi, gs, gc = _sparse_equals_dense(eng, bank, q, k, _dev_bits(_range_bits(allowed, 0, passages=PB)), first=0, n=PB, what=what)
    wi, ws, wc = ref.filtered_topk(scores[:q.shape[0]], allowed, k)
    assert np.array_equal(gc.cpu().numpy(), wc), f"{what}: counts {gc.tolist()} for {wc.tolist()}"
    assert np.array_equal(gi.cpu().numpy(), wi), f"{what}: indices"
    assert np.array_equal(gs.cpu().numpy().view(np.int32), ws.view(np.int32)), f"{what}: scores"
    return gi, gs, gc


@pytest.mark.parametrize("k", [1024, 7])
def test_counts_around_every_border_of_the_counted_selection(k):
    eng, bank, q, scores = _case()
    gi, gs, gc = _equals_dense_and_ref(eng, bank, q, scores, _rows_of(COUNTS, 30), k, f"a row per query, k {k}")
    assert gc.tolist() == [min(c, k) for c in COUNTS]


def test_one_shared_row_across_a_slice_border():
    eng, bank, q, scores = _case()
    q2 = q[:2].contiguous()
    for c in (4097, 1025):
        gi, gs, gc = _equals_dense_and_ref(eng, bank, q2, scores, _rows_of((c,), 31 + c), 1024, f"one shared row of {c}")
        assert gc.tolist() == [1024, 1024]


def test_a_short_list_passes_through_the_later_passes_unchanged():
    """Counts 5, 4 100 and 9 000 in one call: the host launches the two passes 9 000 entries need; the list of 5 is one slice from
    the start and its survivors go through the second pass as they are."""
    eng, bank, q, scores = _case()
    q3 = q[:3].contiguous()
    for k in (1024, 3):
        gi, gs, gc = _equals_dense_and_ref(eng, bank, q3, scores, _rows_of((5, 4100, 9000), 32), k, f"counts 5 / 4100 / 9000, k {k}")
        assert gc.tolist() == [min(5, k), k, k]


def test_equal_scores_across_a_slice_border_keep_the_order_of_the_bank():
    eng, bank, q, scores = _case()
    q1 = q[:1].contiguous()
    every = np.ones((1, PB), dtype=bool)
    gi, gs, gc = _equals_dense_and_ref(eng, bank, q1, scores, every, 30, "every bit set")
    assert gi[0, :22].tolist() == list(TWINS_A + TWINS_B), "the twins are query 0's best, by ascending bank index"
    assert len(set(gs[0, :22].cpu().numpy().view(np.int32).tolist())) == 1
    back = every.copy()
    back[0, :100] = False                                         # TWINS_B now lie at the places 4091 .. 4101
    back[0, list(TWINS_A[::2])] = False
    gi, gs, gc = _equals_dense_and_ref(eng, bank, q1, scores, back, 30, "the first 100 filtered out")
    assert gi[0, :16].tolist() == list(TWINS_A[1::2] + TWINS_B)


# ---- the stages alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first,n", [(37, 40007), (37, 250), (64, 4096), (5, 27)])
def test_filter_compact_equals_flatnonzero(first, n):
    """first = 37: a word of the range takes its bits from two filter words; 40 007 passages: 1251 words, two rounds of the
    compaction's 1024; (5, 27): the range inside one filter word."""
    from rmr_amd import _lib as L
    lib = L.load()
    passages, rows = first + n + 50, 3
    rng = np.random.default_rng(first + n)
    allowed = rng.random((rows, passages)) < np.array([[0.5], [0.02], [1.0]])
    allowed[1, first] = allowed[1, first + n - 1] = True          # the first and the last passage of the range
    bits = _dev_bits(ref.pack_bits([np.flatnonzero(r) for r in allowed], passages, False, ref.words(passages) + 1))
    bits[:, -1] = -1                                              # set bits beyond the bank
    cand = torch.full((rows + 1, n), IPOISON, device="cuda", dtype=torch.int32)
    cnt = torch.full((rows + 1,), IPOISON, device="cuda", dtype=torch.int32)
    assert lib.rr_op_filter_compact(bits.data_ptr(), rows, bits.shape[1], first, n, cand.data_ptr(), cnt.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    got, got_cnt = cand.cpu().numpy(), cnt.cpu().numpy()
    assert got_cnt[rows] == IPOISON and (got[rows] == IPOISON).all(), "nothing behind the rows"
    for r in range(rows):
        want = np.flatnonzero(allowed[r, first:first + n])
        assert got_cnt[r] == len(want) and np.array_equal(got[r, :len(want)], want), f"row {r}"
        assert (got[r, len(want):] == IPOISON).all(), "nothing behind the count"
    cand.fill_(IPOISON)
    cnt.fill_(IPOISON)
    one = bits[1:2].contiguous()                                  # one row: the shared filter of a call
    assert lib.rr_op_filter_compact(one.data_ptr(), 1, one.shape[1], first, n, cand.data_ptr(), cnt.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    want = np.flatnonzero(allowed[1, first:first + n])
    assert cnt.tolist() == [len(want)] + [IPOISON] * rows and np.array_equal(cand[0, :len(want)].cpu().numpy(), want)
    assert (cand[0, len(want):] == IPOISON).all() and (cand[1:] == IPOISON).all()
    cand.fill_(IPOISON)
    assert lib.rr_op_filter_compact(bits.data_ptr(), rows, ref.words(first + n) - 1, first, n, cand.data_ptr(), cnt.data_ptr(), _stream()) \
        == L.RR_ERR_BAD_SHAPE
    assert lib.rr_op_filter_compact(None, rows, bits.shape[1], first, n, cand.data_ptr(), cnt.data_ptr(), _stream()) == L.RR_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert (cand == IPOISON).all(), "a refused call writes nothing"


def _counted(lib, sc, counts, cand, rows, k, first):
    nl, n = sc.shape
    gi = torch.full((nl + 1, k), IPOISON, device="cuda", dtype=torch.int32)
    gs = torch.full((nl + 1, k), POISON, device="cuda")
    gc = torch.full((nl + 1,), IPOISON, device="cuda", dtype=torch.int32)
    rc = lib.rr_op_topk_select_counted(sc.data_ptr(), nl, n, counts.data_ptr(), None if cand is None else cand.data_ptr(), rows, k, first,
                                       gi.data_ptr(), gs.data_ptr(), gc.data_ptr(), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return _checked((gi, gs, gc), nl, k)


@pytest.mark.parametrize("k", [1024, 5])
def test_counted_selection_on_hand_made_rows(k):
    """Compact rows over a range of 9 000 holding NaN, +-inf, +-0 and many ties, a candidate list per row; behind every count the
    compact row holds NaN and +inf and the candidate list -1: read as a score either would rank first, read as a passage the
    index would be first - 1."""
    from rmr_amd import _lib as L
    lib = L.load()
    n, first = PB, 11
    counts = [0, 6, 4096, 4100, 9000]
    rng = np.random.default_rng(50 + k)
    values = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.5, 1.5, -2.25, 3.0, 1e-30], dtype=np.float32)
    dense = np.full((len(counts), n), -np.inf, dtype=np.float32)
    allowed = np.zeros((len(counts), n), dtype=bool)
    sc = np.empty((len(counts), n), dtype=np.float32)
    sc[:, 0::2], sc[:, 1::2] = np.nan, np.inf                     # poison
    cand = np.full((len(counts), n), -1, dtype=np.int32)
    for r, c in enumerate(counts):
        where = np.sort(rng.choice(n, size=c, replace=False))
        vals = values[rng.integers(0, len(values), size=c)]
        if c == 6:
            vals = np.array([-np.inf, 0.0, np.nan, -0.0, np.inf, -np.inf], dtype=np.float32)
        cand[r, :c], sc[r, :c] = where, vals
        allowed[r, where], dense[r, where] = True, vals
    got = _counted(lib, torch.from_numpy(sc).cuda(), torch.tensor(counts, dtype=torch.int32).cuda(), torch.from_numpy(cand).cuda(),
                   len(counts), k, first)
    wi, ws, wc = ref.filtered_topk(dense, allowed, k, first=first)
    assert np.array_equal(got[2].cpu().numpy(), wc) and np.array_equal(got[0].cpu().numpy(), wi)
    gs = got[1].cpu().numpy()
    nan = np.isnan(ws)
    assert np.array_equal(np.isnan(gs), nan) and np.array_equal(gs.view(np.int32)[~nan], ws.view(np.int32)[~nan])
    assert wc[1] == 4 and wi[1, :4].tolist() == [first + int(cand[1, j]) for j in (2, 4, 1, 3)], "NaN, +inf, +0 before -0 by place; -inf absent"
    # one shared list for every row of scores, and no list at all: a place is the passage
    shared = _counted(lib, torch.from_numpy(sc[3:5]).cuda(), torch.tensor([4100], dtype=torch.int32).cuda(), torch.from_numpy(cand[3:4]).cuda(),
                      1, k, first)
    d2 = np.full((2, n), -np.inf, dtype=np.float32)
    d2[:, cand[3, :4100]] = sc[3:5, :4100]
    wi, ws, wc = ref.filtered_topk(d2, allowed[3:4], k, first=first)
    assert np.array_equal(shared[2].cpu().numpy(), wc) and np.array_equal(shared[0].cpu().numpy(), wi)
    plain = _counted(lib, torch.from_numpy(sc[3:4]).cuda(), torch.tensor([4100], dtype=torch.int32).cuda(), None, 1, k, 0)
    d3 = np.full((1, n), -np.inf, dtype=np.float32)
    d3[0, :4100] = sc[3, :4100]
    wi, ws, wc = ref.filtered_topk(d3, np.arange(n)[None, :] < 4100, k)
    assert np.array_equal(plain[2].cpu().numpy(), wc) and np.array_equal(plain[0].cpu().numpy(), wi)
    assert lib.rr_op_topk_select_counted(None, 1, n, None, None, 1, k, 0, None, None, None, None) == L.RR_ERR_BAD_ARG
