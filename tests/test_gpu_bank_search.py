"""GPU: exact top-k MaxSim search over a passage bank (rr_bank_search / RerankEngine.bank_search, include/rerank_mi355.h).

The oracle throughout is what the library already offers for the same answer: the MaxSim of every (query, passage) pair from
rr_bank_li_scores (padded to the longest passage), then torch.sort(descending=True, stable=True).  The search must give its
indices and its scores bit for bit: on an fp16 bank, on compressed banks (which must also equal their fp16 twin), over more than
one selection slice, over a range, at D = 16 through the raw operator, and the selection alone on crafted scores (ties, +-inf,
NaN, ramps, every slice boundary).  Refused calls write nothing.
"""
import numpy as np
import pytest
import torch

from test_gpu_bank_li_scores import LENS, POISON, _mask, _queries
from test_gpu_li_scores import _engine as _bare_engine
from test_gpu_plaid_bank import N_CENTROIDS, _codec, _fp16_twin, _rows

pytestmark = pytest.mark.gpu

DUPES = [1, 4]                            # the passages stored a second time under new ids: exact ties at different indices
SMALL_LENS = LENS + [LENS[i] for i in DUPES]
FULL = (0, 3)                             # two fully masked passages (1 row and 17 rows): a tie at Lq times -9999
IPOISON = -77


def _small_masks():
    m = _mask(LENS, full=FULL[1])
    m[FULL[0]][:] = 0
    return m + [m[i].clone() for i in DUPES]


def _ids(n):
    return [f"p{i}" for i in range(n)]


def _small_fp16_bank(eng, D, seed):
    gen = torch.Generator().manual_seed(seed)
    Lc = max(LENS)
    li = torch.nn.functional.normalize(torch.randn(len(LENS), Lc, D, generator=gen), dim=-1)
    li = torch.cat([li, li[DUPES]])
    cm = torch.zeros(len(SMALL_LENS), Lc)
    for i, m in enumerate(_small_masks()):
        cm[i, :SMALL_LENS[i]] = m.float()
    bank = eng.create_bank(sum(SMALL_LENS) + 4, len(SMALL_LENS) + 1)
    bank.add(_ids(len(SMALL_LENS)), li, cm, lengths=SMALL_LENS)
    return bank


def _small_plaid_bank(eng, D, nbits, seed):
    codec = _codec(D, nbits)
    codes, res = _rows(codec, sum(LENS), seed)
    first = np.concatenate([[0], np.cumsum(LENS)])
    for i in DUPES:
        codes = torch.cat([codes, codes[first[i]:first[i + 1]]])
        res = torch.cat([res, res[first[i]:first[i + 1]]])
    bank = eng.create_bank(sum(SMALL_LENS) + 4, len(SMALL_LENS) + 1, codec=codec)
    bank.add_compressed(_ids(len(SMALL_LENS)), codes, res, SMALL_LENS, mask=torch.cat(_small_masks()))
    return bank


def _oracle(eng, bank, q, first=0, count=None):
    """(indices int32 [nq, n] absolute, scores [nq, n]) of the stable descending sort of rr_bank_li_scores' MaxSim over every
    (query, passage of the range), padded to the longest passage of the bank."""
    P = len(bank)
    n = P - first if count is None else count
    nq = q.shape[0]
    ids = [f"p{i}" for i in range(first, first + n)] * nq
    pq = np.repeat(np.arange(nq), n)
    ms = eng.bank_li_scores(bank, q, ids, pair_query=pq, padded_len=int(max(bank.table.lengths)))["maxsim"].reshape(nq, n)
    s, i = _stable_sort(ms)
    return i + first, s


def _stable_sort(scores):
    """torch.sort(descending=True, stable=True) per row, on the host (a comparison sort: +0 == -0, NaN first): (values, int32
    indices) back on the device."""
    s, i = torch.sort(scores.cpu(), dim=1, descending=True, stable=True)
    return s.cuda(), i.to(torch.int32).cuda()


def _same(got, want_i, want_s, k, tag=""):
    assert got["indices"].dtype == torch.int32 and got["indices"].shape == (want_i.shape[0], k)
    assert got["scores"].dtype == torch.float32 and got["scores"].shape == (want_i.shape[0], k)
    bad = (got["indices"] != want_i[:, :k]).nonzero()
    assert bad.numel() == 0, f"{tag}: indices differ first at {bad[0].tolist()}: {got['indices'][tuple(bad[0])].item()} for " \
                             f"{want_i[tuple(bad[0])].item()}"
    assert torch.equal(got["scores"], want_s[:, :k]), f"{tag}: scores differ by {(got['scores'] - want_s[:, :k]).abs().max().item():.3e}"


# ---- 1. a small bank, the whole order ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lq", [5, 32, 130])                   # below one tile, a whole column block, more than one column block
@pytest.mark.parametrize("kind", ["fp16", "nbits1", "nbits2", "nbits4", "nbits8"])
def test_small_bank_whole_order_equals_sorted_bank_li_scores(kind, Lq):
    D, P = 64, len(SMALL_LENS)
    eng = _bare_engine(D)
    bank = _small_fp16_bank(eng, D, seed=7 + Lq) if kind == "fp16" else _small_plaid_bank(eng, D, int(kind[5:]), seed=11 + Lq)
    q = _queries(3, Lq, D, seed=100 + Lq)
    want_i, want_s = _oracle(eng, bank, q)
    got = eng.bank_search(bank, q, P)
    again = eng.bank_search(bank, q, P)
    torch.cuda.synchronize()
    _same(got, want_i, want_s, P, kind)
    assert torch.equal(again["indices"], got["indices"]) and torch.equal(again["scores"], got["scores"])
    s, idx = got["scores"].cpu(), got["indices"].cpu()
    for qi in range(3):
        order = idx[qi].tolist()
        assert sorted(order) == list(range(P))
        for a, b in ((DUPES[0], len(LENS)), (DUPES[1], len(LENS) + 1), FULL):      # exact ties: the lower index comes first, next to it
            assert s[qi, order.index(a)] == s[qi, order.index(b)] and order.index(b) == order.index(a) + 1
        assert order[-2:] == list(FULL) and float(s[qi, -1]) == -9999.0 * Lq
    if kind != "fp16":                                                             # ... and the fp16 bank of the decoded rows
        twin = _fp16_twin(eng, bank, SMALL_LENS, max(SMALL_LENS))
        ref = eng.bank_search(twin, q, P)
        torch.cuda.synchronize()
        assert torch.equal(ref["indices"], got["indices"]) and torch.equal(ref["scores"], got["scores"])


def test_search_follows_adds_and_a_clear():
    """The device table is brought up to date by the first search after an add, and rebuilt after a clear."""
    D = 64
    eng = _bare_engine(D)
    gen = torch.Generator().manual_seed(5)
    li = torch.nn.functional.normalize(torch.randn(6, 8, D, generator=gen), dim=-1)
    cm = torch.ones(6, 8)
    q = _queries(2, 7, D, seed=3)
    bank = eng.create_bank(200, 16)
    bank.add(_ids(3), li[:3], cm[:3], lengths=[8, 3, 5])
    _same(eng.bank_search(bank, q, 3), *_oracle(eng, bank, q), 3, "three")
    bank.add(["p3", "p4", "p5"], li[3:], cm[3:], lengths=[2, 8, 1])
    _same(eng.bank_search(bank, q, 6), *_oracle(eng, bank, q), 6, "six")
    bank.clear()
    bank.add(_ids(4), li[2:], cm[2:], lengths=[1, 7, 2, 8])
    _same(eng.bank_search(bank, q, 4), *_oracle(eng, bank, q), 4, "after clear")
    ids, sc = bank.search(eng, q, 2, first=1)
    want_i, want_s = _oracle(eng, bank, q, first=1)
    assert ids == [[f"p{j}" for j in row] for row in want_i[:, :2].tolist()] and torch.equal(sc, want_s[:, :2])


# ---- 2. more than one selection slice ----------------------------------------------------------------------------------------
_BIG = {}


def _big(P):
    """(engine, fp16 bank of P passages of 1 .. 24 random unit rows, two queries, the oracle over the whole bank), built once."""
    if P not in _BIG:
        D, Lc = 64, 24
        eng = _bare_engine(D)
        gen = torch.Generator(device="cuda").manual_seed(P)
        li = torch.nn.functional.normalize(torch.randn(P, Lc, D, generator=gen, device="cuda"), dim=-1).half()
        lens = (torch.arange(P) * 7 % Lc + 1).tolist()
        cm = (torch.arange(Lc)[None, :] < torch.tensor(lens)[:, None]).float()
        bank = eng.create_bank(sum(lens), P)
        bank.add(_ids(P), li, cm, lengths=lens)
        q = _queries(2, 20, D, seed=P)
        _BIG[P] = (eng, bank, q, _oracle(eng, bank, q))
    return _BIG[P]


@pytest.mark.parametrize("k", [1, 100, 1024])
@pytest.mark.parametrize("P", [4097, 9000])                    # one entry into a second slice; three slices, the last partial
def test_more_than_one_selection_slice(P, k):
    eng, bank, q, (want_i, want_s) = _big(P)
    got = eng.bank_search(bank, q, k)
    torch.cuda.synchronize()
    _same(got, want_i, want_s, k, f"P{P}_k{k}")


@pytest.mark.parametrize("k", [1, 100, 1024])
def test_a_range_of_the_bank_with_absolute_indices(k):
    eng, bank, q, _ = _big(9000)
    want_i, want_s = _oracle(eng, bank, q, first=37, count=4096)
    got = eng.bank_search(bank, q, k, first=37, count=4096)
    torch.cuda.synchronize()
    assert int(got["indices"].min()) >= 37 and int(got["indices"].max()) < 37 + 4096
    _same(got, want_i, want_s, k, f"range_k{k}")
    tail = eng.bank_search(bank, q, 5, first=8990)               # count None: through the last passage
    torch.cuda.synchronize()
    _same(tail, *_oracle(eng, bank, q, first=8990), 5, "tail")


# ---- 3. the raw operator: D = 16, and nbits 8 at the smallest D its codec takes ----------------------------------------------
def _table_dev(lens):
    a = np.zeros(len(lens), dtype=np.dtype([("first", "<i8"), ("len", "<i4"), ("unused", "<i4")]))
    a["first"], a["len"] = np.concatenate([[0], np.cumsum(lens)[:-1]]), lens
    return torch.from_numpy(a.view(np.uint8).copy()).cuda()


def _pairs_dev(lens, nq):
    first = np.concatenate([[0], np.cumsum(lens)[:-1]])
    a = np.zeros(len(lens) * nq, dtype=np.dtype([("first", "<i8"), ("len", "<i4"), ("query", "<i4")]))
    a["first"], a["len"], a["query"] = np.tile(first, nq), np.tile(lens, nq), np.repeat(np.arange(nq), len(lens))
    return torch.from_numpy(a.view(np.uint8).copy()).cuda()


# a codec takes D that is a multiple of 8 * nbits: at D = 16 that is nbits 1 and 2; nbits 8 starts at D = 64
@pytest.mark.parametrize("D,nbits", [(16, 0), (16, 1), (16, 2), (64, 8)])
@pytest.mark.parametrize("Lq", [5, 32, 130])
def test_raw_operator_against_op_bank_li_scores_and_a_stable_sort(D, nbits, Lq):
    from rmr_amd import _lib as L
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    lens, nq = SMALL_LENS, 3
    P, R, Lc = len(lens), sum(lens), max(lens)
    mask_d = torch.cat(_small_masks()).cuda()
    q = _queries(nq, Lq, D, seed=D + Lq)
    if nbits:
        codec = _codec(D, nbits)
        codes, res = _rows(codec, R, seed=Lq + nbits)
        keep = (codes.cuda(), res.cuda(), codec.centroids.cuda(), codec.bucket_weights.cuda())
        src = (None, L.ptr(mask_d), nbits, *(L.ptr(t) for t in keep), N_CENTROIDS)
    else:
        gen = torch.Generator().manual_seed(16 + Lq)
        keep = (torch.nn.functional.normalize(torch.randn(R, D, generator=gen), dim=-1).half().cuda(),)
        src = (L.ptr(keep[0]), L.ptr(mask_d), 0, None, None, None, None, 0)
    pairs, table = _pairs_dev(lens, nq), _table_dev(lens)
    ms = torch.full((nq * P,), POISON, device="cuda")
    assert lib.rr_op_bank_li_scores(L.ptr(q), Lq, D, L.ptr(pairs), nq * P, Lc, *src, None, L.ptr(ms), st) == 0
    want_s, want_i = _stable_sort(ms.reshape(nq, P))
    for first, n, k in ((0, P, P), (0, P, 3), (2, 5, 5)):
        gi = torch.full((nq + 1, k), IPOISON, device="cuda", dtype=torch.int32)
        gs = torch.full((nq + 1, k), POISON, device="cuda")
        assert lib.rr_op_bank_search(L.ptr(q), nq, Lq, D, L.ptr(table), first, n, k, *src, L.ptr(gi), L.ptr(gs), st) == 0
        torch.cuda.synchronize()
        if (first, n) == (0, P):
            wi, ws = want_i[:, :k], want_s[:, :k]
        else:
            ws, wi = _stable_sort(ms.reshape(nq, P)[:, first:first + n])
            wi = wi + first
        assert torch.equal(gi[:nq], wi) and torch.equal(gs[:nq], ws), f"first {first} n {n} k {k}"
        assert (gi[nq:] == IPOISON).all() and (gs[nq:] == POISON).all()
    assert lib.rr_op_bank_search(L.ptr(q), nq, Lq, D, L.ptr(table), 0, P, P + 1, *src, L.ptr(gi), L.ptr(gs), st) == L.RR_ERR_BAD_SHAPE


# ---- 4. the selection alone ----------------------------------------------------------------------------------------------------
def _select(scores, k, want_scores=True):
    from rmr_amd import _lib as L
    lib = L.load()
    lists, n = scores.shape
    gi = torch.full((lists + 1, k), IPOISON, device="cuda", dtype=torch.int32)
    gs = torch.full((lists + 1, k), POISON, device="cuda")
    rc = lib.rr_op_topk_select(L.ptr(scores), lists, n, k, L.ptr(gi), L.ptr(gs) if want_scores else None,
                               torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert (gi[lists:] == IPOISON).all() and (gs[lists:] == POISON).all()
    return gi[:lists], gs[:lists]


@pytest.mark.parametrize("n", [1, 4095, 4096, 4097, 3 * 4096 + 1])
def test_topk_select_on_crafted_scores(n):
    gen = torch.Generator().manual_seed(n)
    ramp = torch.arange(n, dtype=torch.float32)
    few = torch.randint(0, 7, (n,), generator=gen).float() - 3.0          # seven distinct values, +-0 among them: ties everywhere
    few[few == 0] = torch.where(torch.arange(int((few == 0).sum())) % 2 == 0, 0.0, -0.0)
    inf = torch.randn(n, generator=gen)
    inf[::5], inf[3::7] = float("inf"), float("-inf")
    nan = inf.clone()
    nan[n // 2] = float("nan")
    lists = torch.stack([torch.full((n,), 2.5), -ramp, ramp, few, torch.randn(n, generator=gen), inf, nan]).cuda()
    NAN_LIST = lists.shape[0] - 1
    want_s, want_i = _stable_sort(lists)
    assert bool(torch.isnan(want_s[NAN_LIST, 0])) and int(want_i[NAN_LIST, 0]) == n // 2      # torch ranks the NaN first
    for k in sorted({1, n if n <= 1024 else 1024, min(n, 1024)}):
        gi, gs = _select(lists, k)
        assert gi[0].tolist() == list(range(k)), "all-equal scores keep index order"
        assert torch.equal(gi, want_i[:, :k]), f"n {n} k {k}: lists {sorted(set((gi != want_i[:, :k]).nonzero()[:, 0].tolist()))} differ"
        assert torch.equal(gs[:NAN_LIST], want_s[:NAN_LIST, :k])
        got_nan, ref_nan = torch.isnan(gs[NAN_LIST]), torch.isnan(want_s[NAN_LIST, :k])
        assert torch.equal(got_nan, ref_nan) and bool(got_nan[0]) and int(got_nan.sum()) == 1
        assert torch.equal(gs[NAN_LIST][~got_nan], want_s[NAN_LIST, :k][~ref_nan])
        only_i, untouched = _select(lists, k, want_scores=False)
        assert torch.equal(only_i, gi) and (untouched == POISON).all()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def _raw(eng, bank, q, first, n, k, gi, gs, q_ptr=None, handle=True, bank_h=True, n_queries=None, Lq=None):
    from rmr_amd import _lib as L
    return eng.lib.rr_bank_search(eng.h if handle else None, bank.h if bank_h else None, L.ptr(q) if q_ptr is None else q_ptr,
                                  q.shape[0] if n_queries is None else n_queries, q.shape[1] if Lq is None else Lq, first, n, k,
                                  L.ptr(gi) if gi is not None else None, L.ptr(gs), torch.cuda.current_stream().cuda_stream)


def test_refusals_write_nothing():
    from rmr_amd import _lib as L
    D, Lq = 64, 9
    eng, other, full = _bare_engine(D), _bare_engine(128), _bare_engine(D, "full_context")
    P = len(SMALL_LENS)
    big = _big(4097)[1]
    q = _queries(2, Lq, D, seed=53)
    gi = torch.full((2, 1025), IPOISON, device="cuda", dtype=torch.int32)
    gs = torch.full((2, 1025), POISON, device="cuda")
    for bank in (_small_fp16_bank(eng, D, seed=51), _small_plaid_bank(eng, D, 4, seed=51)):
        assert _raw(eng, bank, q, 0, P, 0, gi, gs) == L.RR_ERR_BAD_SHAPE                      # k = 0
        assert _raw(eng, bank, q, 0, P, P + 1, gi, gs) == L.RR_ERR_BAD_SHAPE                  # k above the range
        assert _raw(eng, bank, q, 2, 3, 4, gi, gs) == L.RR_ERR_BAD_SHAPE
        assert _raw(eng, bank, q, 2, -1, P - 1, gi, gs) == L.RR_ERR_BAD_SHAPE                 # -1: P - 2 passages
        assert _raw(eng, bank, q, 1, P, 1, gi, gs) == L.RR_ERR_BAD_SHAPE                      # a range past the end
        assert b"holds 8" in eng.lib.rr_last_error(eng.h)
        assert _raw(eng, bank, q, P, -1, 1, gi, gs) == L.RR_ERR_BAD_SHAPE                     # an empty range
        assert _raw(eng, bank, q, -1, 2, 1, gi, gs) == L.RR_ERR_BAD_SHAPE
        assert _raw(eng, bank, q, 0, 0, 1, gi, gs) == L.RR_ERR_BAD_SHAPE
        assert _raw(eng, bank, q, 0, -2, 1, gi, gs) == L.RR_ERR_BAD_SHAPE
        assert _raw(eng, bank, q, 0, P, 1, gi, gs, n_queries=0) == L.RR_ERR_BAD_SHAPE
        assert _raw(eng, bank, q, 0, P, 1, gi, gs, Lq=0) == L.RR_ERR_BAD_SHAPE
        assert _raw(eng, bank, q, 0, P, 1, gi, gs, q_ptr=L.ptr(q) + 4) == L.RR_ERR_BAD_ARG    # a misaligned query
        assert _raw(eng, bank, q, 0, P, 1, gi, gs, q_ptr=0) == L.RR_ERR_BAD_ARG
        assert _raw(eng, bank, q, 0, P, 1, None, gs) == L.RR_ERR_BAD_ARG
        assert _raw(eng, bank, q, 0, P, 1, gi, gs, handle=False) == L.RR_ERR_BAD_ARG
        assert _raw(eng, bank, q, 0, P, 1, gi, gs, bank_h=False) == L.RR_ERR_BAD_ARG
        assert _raw(full, bank, q, 0, P, 1, gi, gs) == L.RR_ERR_BAD_ARG                       # a full-context handle
        assert _raw(other, bank, q, 0, P, 1, gi, gs) == L.RR_ERR_BAD_SHAPE                    # another li_dim
        assert b"li_dim" in other.lib.rr_last_error(other.h)
    assert _raw(eng, big, q, 0, -1, 1025, gi, gs) == L.RR_ERR_UNSUPPORTED                     # k = 1025 of 4097
    assert b"1024" in eng.lib.rr_last_error(eng.h)
    torch.cuda.synchronize()
    assert (gi == IPOISON).all() and (gs == POISON).all()
    with pytest.raises(ValueError):
        eng.bank_search(bank, q, 0)
    with pytest.raises(ValueError):
        eng.bank_search(bank, q, P + 1)
    with pytest.raises(ValueError):
        eng.bank_search(bank, q, 1, first=1, count=P)
    with pytest.raises(NotImplementedError):
        eng.bank_search(big, q, 1025)
    with pytest.raises(ValueError):
        full.bank_search(bank, q, 1)                                                          # RR_ERR_BAD_ARG
    assert _raw(eng, big, q, 0, -1, 1024, gi[:, :1024].contiguous(), None) == 0               # and what is right is taken
    torch.cuda.synchronize()


def test_a_capturing_stream_is_refused_and_nothing_is_written():
    from rmr_amd import _lib as L
    D = 64
    eng = _bare_engine(D)
    bank = _small_fp16_bank(eng, D, seed=55)
    q = _queries(2, 9, D, seed=57)
    gi = torch.full((2, 3), IPOISON, device="cuda", dtype=torch.int32)
    gs = torch.full((2, 3), POISON, device="cuda")
    probe = torch.zeros(1, device="cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        assert _raw(eng, bank, q, 0, -1, 3, gi, gs) == 0          # the table and the block exist: only the capture is in the way
        torch.cuda.synchronize()
        gi.fill_(IPOISON)
        gs.fill_(POISON)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            probe.add_(1.0)                                        # the graph holds this node alone
            rc = _raw(eng, bank, q, 0, -1, 3, gi, gs)
            msg = eng.lib.rr_last_error(eng.h)
        graph.replay()
        torch.cuda.synchronize()
    assert rc == L.RR_ERR_BAD_ARG and b"captured" in msg
    assert probe.item() == 1.0 and (gi == IPOISON).all() and (gs == POISON).all()
    assert _raw(eng, bank, q, 0, -1, 3, gi, gs) == 0
    torch.cuda.synchronize()
    assert not (gi == IPOISON).any()


def test_profile_books_the_scoring_flops_in_the_tail_class():
    D, Lq = 64, 9
    eng = _bare_engine(D)
    bank = _small_fp16_bank(eng, D, seed=61)
    q = _queries(2, Lq, D, seed=63)
    eng.bank_search(bank, q, 3)
    eng.set_profiling(True)
    try:
        eng.get_profile(reset=True)
        eng.bank_search(bank, q, 3)
        p = eng.get_profile(reset=True)
    finally:
        eng.set_profiling(False)
    assert p["tail"]["launches"] == 2 and p["tail"]["flops"] == 2.0 * 2 * sum(SMALL_LENS) * Lq * D and p["tail"]["ms"] > 0
    assert sum(v["launches"] for v in p.values()) == 2


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------
def test_retrieve_and_rerank_on_the_drop_in_class():
    from test_gpu_passage_bank import _model
    from test_gpu_plaid_bank import _two_queries
    m, g = _model("int_tiny")
    q, qm = _two_queries(g)
    D, Lc = q.shape[2], int(g["Lc"])
    with pytest.raises(RuntimeError):
        m.retrieve(q, 2)
    gen = torch.Generator().manual_seed(71)
    P = 12
    lens = [1 + (5 * i) % Lc for i in range(P)]
    li = torch.nn.functional.normalize(torch.randn(P, Lc, D, generator=gen), dim=-1)
    cm = (torch.arange(Lc)[None, :] < torch.tensor(lens)[:, None]).float()
    bank = m.create_bank(sum(lens), P)
    names = [("doc", i) for i in range(P)]
    bank.add(names, li, cm, lengths=lens)
    ids, out = m.retrieve_and_rerank(q, qm, k=8)
    found, scores = m.retrieve(q, 8)
    assert ids == found and len(ids) == 2 and all(len(r) == 8 and len(set(r)) == 8 for r in ids)
    ms = m.retriever_scores(q, names * 2, K=P)["maxsim"].reshape(2, P)
    ws, wi = torch.sort(ms, dim=1, descending=True, stable=True)
    assert ids == [[names[j] for j in row] for row in wi[:, :8].tolist()] and torch.equal(scores, ws[:, :8])
    ref = m.forward_passages(q, qm, [pid for row in ids for pid in row], 7)
    torch.cuda.synchronize()
    assert out.logits.shape == ref.logits.shape and torch.equal(out.logits, ref.logits)
