"""GPU: PLAID-pruned top-k search over a compressed passage bank (rr_bank_search_plaid / RerankEngine.bank_search_plaid,
include/rerank_mi355.h).

The oracle is built from what the library offered before this call existed: S from rr_li_scores on float32(centroids), the cells,
the candidates and the two pruning stages from tests/plaid_search_ref.py on those bits, the exact scores from rr_bank_search over
the whole bank (rr_bank_li_scores where the bank is larger than a search returns).  Every intermediate (rr_bank_search_plaid_tap)
and the result are compared bit for bit; no tolerance anywhere."""
import numpy as np
import pytest
import torch

import plaid_search_ref as ref
from test_gpu_bank_li_scores import POISON
from test_gpu_bank_search import IPOISON
from test_gpu_li_scores import _engine as _bare_engine

pytestmark = pytest.mark.gpu

LEN_CYCLE = [1, 15, 16, 17, 40, 63, 64, 65, 130]       # at and around the 16-row tile and the 64-code scan step
N_BASE, N_TOPICS = 270, 4
DUPES = list(range(5, 270, 9))                          # stored a second time under new ids: exact ties at different indices
FULLY_MASKED = 13
NDOCS, K, THRESHOLD = 32, 8, 0.3


def _codec(D, nbits, C, seed=0):
    from rmr_amd import PlaidCodec
    gen = torch.Generator().manual_seed(1000 * D + 10 * nbits + C + seed)
    cen = torch.nn.functional.normalize(torch.randn(C, D, generator=gen), dim=-1)
    w = torch.randn(1 << nbits, generator=gen) * (0.5 / D ** 0.5)
    w[0] = 0.0
    return PlaidCodec(cen, w, nbits)


def _topic_rows(codec, lens, seed, topics_from=None):
    """Codes drawn per passage from N_TOPICS centroids (of `topics_from`, default all), random residual bytes."""
    gen = torch.Generator().manual_seed(seed)
    C = codec.n_centroids
    pool = torch.arange(C) if topics_from is None else torch.tensor(topics_from)
    codes = []
    for ln in lens:
        t = pool[torch.randperm(len(pool), generator=gen)[:N_TOPICS]]
        codes.append(t[torch.randint(0, len(t), (ln,), generator=gen)])
    codes = torch.cat(codes).to(torch.int32)
    res = torch.randint(0, 256, (len(codes), codec.residual_bytes), generator=gen, dtype=torch.uint8)
    return codes, res


def _near_queries(codec, nq, Lq, seed, near=5):
    """Unit query tokens drawn near a handful of centroids per query, so that cells and threshold select."""
    gen = torch.Generator().manual_seed(seed)
    C, D = codec.centroids.shape
    qs = []
    for _ in range(nq):
        pick = torch.randperm(C, generator=gen)[:near][torch.randint(0, near, (Lq,), generator=gen)]
        qs.append(torch.nn.functional.normalize(codec.centroids[pick].float() + 0.9 * torch.randn(Lq, D, generator=gen) / D ** 0.5, dim=-1))
    return torch.stack(qs).cuda()


def _build(eng, codec, lens, codes, res, mask):
    bank = eng.create_bank(sum(lens) + 4, len(lens) + 1, codec=codec)
    bank.add_compressed([f"p{i}" for i in range(len(lens))], codes, res, lens, mask=mask)
    return bank


def _S(eng, codec, q):
    """rr_li_scores on float32(centroids), one context block per query: S [nq, C, Lq] (numpy)."""
    nq = q.shape[0]
    C = codec.n_centroids
    ctx = codec.centroids.half().float().cuda()[None].expand(nq, -1, -1).contiguous()
    sc = eng.li_scores(q, ctx, torch.ones(nq, C, device="cuda"), nq, 1, want_maxsim=False)["scores"]
    torch.cuda.synchronize()
    return sc.cpu().numpy()


def _exact_all(eng, bank, q):
    """exact [nq, P] from rr_bank_search over the whole bank (P <= 1024)."""
    P = len(bank)
    r = eng.bank_search(bank, q, P)
    torch.cuda.synchronize()
    out = np.zeros((q.shape[0], P), dtype=np.float32)
    idx, sc = r["indices"].cpu().numpy(), r["scores"].cpu().numpy()
    for qi in range(q.shape[0]):
        out[qi, idx[qi]] = sc[qi]
    return out, idx


_CASES = {}


def _case(name, Lq):
    """(engine, codec, bank, queries, codes, mask, lens, S, exact, exhaustive order) of case A / B at Lq, built once."""
    if (name, Lq) not in _CASES:
        D, nbits = {"A": (64, 8), "B": (128, 2)}[name]
        eng = _bare_engine(D)
        codec = _codec(D, nbits, 64)
        base = [LEN_CYCLE[i % len(LEN_CYCLE)] for i in range(N_BASE)]
        codes, res = _topic_rows(codec, base, seed=D + Lq)
        first = np.concatenate([[0], np.cumsum(base)])
        masks = []
        for i, ln in enumerate(base):
            m = torch.ones(ln, dtype=torch.uint8)
            if i % 2:
                m[2::3] = 0                                       # interior masked rows
            if i == FULLY_MASKED:
                m[:] = 0
            masks.append(m)
        lens = base + [base[i] for i in DUPES]
        codes = torch.cat([codes] + [codes[first[i]:first[i + 1]] for i in DUPES])
        res = torch.cat([res] + [res[first[i]:first[i + 1]] for i in DUPES])
        mask = torch.cat(masks + [masks[i] for i in DUPES])
        bank = _build(eng, codec, lens, codes, res, mask)
        q = _near_queries(codec, 3, Lq, seed=7 * D + Lq)
        exact, order = _exact_all(eng, bank, q)
        _CASES[(name, Lq)] = (eng, codec, bank, q, codes.numpy(), mask.numpy(), lens, _S(eng, codec, q), exact, order)
    return _CASES[(name, Lq)]


def _oracle(S, codes, mask, lens, exact, Lqc, ncells, thr, ndocs, k):
    out = []
    for qi in range(S.shape[0]):
        w = ref.prune(S[qi][:, :Lqc], codes, mask, lens, ncells, thr, ndocs)
        w["final"] = ref.final(w["list2"], exact[qi], k)
        out.append(w)
    return out


def _padded(lists, width):
    return np.array([l + [-1] * (width - len(l)) for l in lists], dtype=np.int32)


def _check_result(got, want, exact, k, add=0):
    idx, sc, cnt = got["indices"].cpu().numpy(), got["scores"].cpu().numpy(), got["counts"].cpu().numpy()
    assert idx.dtype == np.int32 and sc.dtype == np.float32 and cnt.dtype == np.int32
    for qi, w in enumerate(want):
        f = w["final"]
        assert cnt[qi] == len(f), f"query {qi}: count {cnt[qi]} for {len(f)}"
        assert idx[qi, :len(f)].tolist() == [p + add for p in f], f"query {qi}: {idx[qi].tolist()} for {f}"
        assert np.array_equal(sc[qi, :len(f)].view(np.int32), exact[qi][f].view(np.int32)), f"query {qi}: scores"
        assert (idx[qi, len(f):] == -1).all() and np.isneginf(sc[qi, len(f):]).all()


# ---- 1. stage by stage -----------------------------------------------------------------------------------------------------------
CONFIGS = [(name, Lq, Lqc, ncells) for name in "AB" for Lq, Lqc in ((5, 5), (32, 20), (130, 70)) for ncells in (1, 2)]


@pytest.mark.parametrize("name,Lq,Lqc,ncells", CONFIGS)
def test_every_stage_against_the_oracle(name, Lq, Lqc, ncells):
    eng, codec, bank, q, codes, mask, lens, S, exact, _ = _case(name, Lq)
    P, C, nq = len(lens), codec.n_centroids, q.shape[0]
    want = _oracle(S, codes, mask, lens, exact, Lqc, ncells, THRESHOLD, NDOCS, K)
    for qi, w in enumerate(want):                                 # the case bites, on the oracle alone
        cand = int((w["a1"] != ref.NEG_INF).sum())
        assert 0 < cand < P - 1 and np.isneginf(w["a1"][FULLY_MASKED]), f"query {qi}: {cand} candidates of {P}"
        assert cand > len(w["list1"]) == NDOCS and len(w["list2"]) == NDOCS // 4 and len(w["final"]) == K
        assert w["keep"].any() and not w["keep"].all()
    got = eng.bank_search_plaid(bank, q, K, ncells=ncells, centroid_score_threshold=THRESHOLD, ndocs=NDOCS, coarse_tokens=Lqc)
    torch.cuda.synchronize()
    tS = eng.bank_search_plaid_tap("S").reshape(nq, C, Lqc)
    assert np.array_equal(tS.view(np.int32), np.ascontiguousarray(S[:, :, :Lqc]).view(np.int32)), "S"
    assert np.array_equal(eng.bank_search_plaid_tap("cells").reshape(nq, C).astype(bool), np.stack([w["cells"] for w in want])), "cells"
    assert np.array_equal(eng.bank_search_plaid_tap("keep").reshape(nq, C).astype(bool), np.stack([w["keep"] for w in want])), "keep"
    a1 = eng.bank_search_plaid_tap("a1").reshape(nq, P)
    bad = np.argwhere(a1.view(np.int32) != np.stack([w["a1"] for w in want]).view(np.int32))
    assert bad.size == 0, f"A1 differs at {bad[:4].tolist()}: {a1[tuple(bad[0])]} for {want[bad[0][0]]['a1'][bad[0][1]]}"
    assert np.array_equal(eng.bank_search_plaid_tap("list1").reshape(nq, NDOCS), _padded([w["list1"] for w in want], NDOCS)), "stage-1 list"
    assert np.array_equal(eng.bank_search_plaid_tap("list2").reshape(nq, NDOCS // 4), _padded([w["list2"] for w in want], NDOCS // 4)), "stage-2 list"
    _check_result(got, want, exact, K)


def test_pruning_changes_a_result_and_ties_break_by_index():
    """On the oracle: at least one configuration's final list differs from the exhaustive top-k (pruning is not a no-op on these
    banks), and a duplicate comes behind its original wherever both survive, in a run of one score with ascending indices."""
    differs = pairs = 0
    for name, Lq, Lqc, ncells in CONFIGS:
        eng, codec, bank, q, codes, mask, lens, S, exact, order = _case(name, Lq)
        for qi, w in enumerate(_oracle(S, codes, mask, lens, exact, Lqc, ncells, THRESHOLD, NDOCS, K)):
            differs += w["final"] != order[qi, :K].tolist()
            for lst, sc in ((w["list1"], w["a1"]), (w["list2"], w["a2"])):
                for j, d in enumerate(DUPES):
                    if d in lst and N_BASE + j in lst:          # a run of one score (other passages may share it), indices ascending
                        run = lst[lst.index(d):lst.index(N_BASE + j) + 1]
                        assert len(run) >= 2 and run == sorted(run) and len({float(sc[p]) for p in run}) == 1
                        pairs += 1
    assert differs >= 1 and pairs >= 1, (differs, pairs)


# ---- 2. the degenerate configuration is the exhaustive search --------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 50, 200])
def test_every_centroid_a_cell_and_no_cut_equals_bank_search(k):
    D, C, P = 64, 16, 200
    eng = _bare_engine(D)
    codec = _codec(D, 4, C)
    lens = [LEN_CYCLE[i % len(LEN_CYCLE)] for i in range(P)]
    codes, res = _topic_rows(codec, lens, seed=k)
    masks = [torch.ones(ln, dtype=torch.uint8) for ln in lens]
    for m in masks[::2]:
        m[2::3] = 0                                               # interior masked rows; every passage keeps an unmasked row
    bank = _build(eng, codec, lens, codes, res, torch.cat(masks))
    q = _near_queries(codec, 2, 32, seed=3)
    want = eng.bank_search(bank, q, k)
    got = eng.bank_search_plaid(bank, q, k, ncells=C, centroid_score_threshold=0.45, ndocs=1024)
    torch.cuda.synchronize()
    assert torch.equal(got["indices"], want["indices"]) and torch.equal(got["scores"], want["scores"])
    assert got["counts"].tolist() == [k, k]


@pytest.mark.parametrize("D,nbits,Lq", [(16, 1, 40), (16, 2, 70), (64, 8, 40), (64, 4, 200)])
def test_listed_scores_at_one_bit_and_the_64_column_block_equal_bank_search(D, nbits, Lq):
    """The list-driven form of the scoring kernel where no other test takes it: nbits 1, the block of 64 columns (Lq 40), 128
    columns in one block and in two.  41 passages: the last workgroup of the list holds one.  Every centroid a cell, no cut.  A
    handle takes li_dim in multiples of 64, so both searches run through their handle-free operators (rr_op_bank_search_plaid,
    rr_op_bank_search: the launchers of the two calls over the same rows), as the D = 16 cases of test_gpu_bank_search.py do."""
    from rmr_amd import _lib as L
    from test_gpu_bank_search import _table_dev
    lib, st = L.load(), torch.cuda.current_stream().cuda_stream
    C, P, nq = 16, 41, 2
    codec = _codec(D, nbits, C)
    lens = [LEN_CYCLE[i % len(LEN_CYCLE)] for i in range(P - 1)] + [1]
    codes, res = _topic_rows(codec, lens, seed=Lq)
    masks = [torch.ones(ln, dtype=torch.uint8) for ln in lens]
    for m in masks[::2]:
        m[2::3] = 0                                               # interior masked rows; every passage keeps an unmasked row
    keep = (torch.cat(masks).cuda(), codes.cuda(), res.cuda(), codec.centroids.cuda(), codec.bucket_weights.cuda())
    mask_p, comp = L.ptr(keep[0]), (nbits, *(L.ptr(t) for t in keep[1:]), C)
    table = _table_dev(lens)
    q = _near_queries(codec, nq, Lq, seed=5)
    for first, n in ((0, P), (1, P - 2)):
        k = n
        wi, gi = (torch.full((nq, k), IPOISON, device="cuda", dtype=torch.int32) for _ in range(2))
        ws, gs = (torch.full((nq, k), POISON, device="cuda") for _ in range(2))
        gc = torch.full((nq,), IPOISON, device="cuda", dtype=torch.int32)
        assert lib.rr_op_bank_search(L.ptr(q), nq, Lq, D, L.ptr(table), first, n, k, None, mask_p, *comp, L.ptr(wi), L.ptr(ws), st) == 0
        assert lib.rr_op_bank_search_plaid(L.ptr(q), nq, Lq, Lq, D, L.ptr(table), first, n, C, 0.45, 1024, k, mask_p, *comp, L.ptr(gi),
                                           L.ptr(gs), L.ptr(gc), st) == 0
        torch.cuda.synchronize()
        assert sorted(wi[0].tolist()) == list(range(first, first + n))
        assert torch.equal(gi, wi) and torch.equal(gs, ws), f"first {first} n {n}"
        assert gc.tolist() == [k, k]


# ---- 3. short lists ----------------------------------------------------------------------------------------------------------------
def test_short_and_empty_lists_and_nothing_else_written():
    from rmr_amd import _lib as L
    D, C, P, k = 64, 64, 40, 5
    eng = _bare_engine(D)
    codec = _codec(D, 8, C)
    lens = [LEN_CYCLE[i % len(LEN_CYCLE)] for i in range(P)]
    codes, res = _topic_rows(codec, lens, seed=9, topics_from=list(range(8, 32)))
    first = np.concatenate([[0], np.cumsum(lens)])
    holders = [4, 17, 30]
    for p in holders:
        codes[first[p]] = 3                                       # three passages hold a token of centroid 3
    bank = _build(eng, codec, lens, codes, res, None)
    gen = torch.Generator().manual_seed(1)
    tok = lambda c: torch.nn.functional.normalize(codec.centroids[c].float()[None] + 0.3 * torch.randn(6, D, generator=gen) / D ** 0.5, dim=-1)
    q = torch.stack([tok(3), tok(45)]).cuda()                     # query 0 near centroid 3, query 1 near a centroid no passage holds
    S = _S(eng, codec, q)
    exact, _ = _exact_all(eng, bank, q)
    want = _oracle(S, codes.numpy(), None, lens, exact, 6, 1, 0.45, 32, k)
    assert sorted(want[0]["final"]) == holders and want[1]["final"] == [] and not (want[1]["a1"] != ref.NEG_INF).any()
    gi = torch.full((3, k), IPOISON, device="cuda", dtype=torch.int32)
    gs = torch.full((3, k), POISON, device="cuda")
    gc = torch.full((3,), IPOISON, device="cuda", dtype=torch.int32)
    rc = eng.lib.rr_bank_search_plaid(eng.h, bank.h, L.ptr(q), 2, 6, 6, 0, -1, 1, 0.45, 32, k, L.ptr(gi), L.ptr(gs), L.ptr(gc),
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0, eng.lib.rr_last_error(eng.h)
    torch.cuda.synchronize()
    _check_result(dict(indices=gi[:2], scores=gs[:2], counts=gc[:2]), want, exact, k)
    assert gc.tolist() == [3, 0, IPOISON] and (gi[2] == IPOISON).all() and (gs[2] == POISON).all()
    only = torch.full((3, k), IPOISON, device="cuda", dtype=torch.int32)          # scores_out NULL
    assert eng.lib.rr_bank_search_plaid(eng.h, bank.h, L.ptr(q), 2, 6, 6, 0, -1, 1, 0.45, 32, k, L.ptr(only), None, L.ptr(gc),
                                        torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(only, gi)
    found, _ = bank.search(eng, q, k, plaid=__import__("rmr_amd").PlaidSearch(1, 0.45, 32))
    assert found == [[f"p{p}" for p in want[0]["final"]], []]


# ---- 4. more than one selection slice, a range, many queries -----------------------------------------------------------------------
_BIG = {}


def _big():
    if not _BIG:
        D, C, P = 64, 64, 9000
        eng = _bare_engine(D)
        codec = _codec(D, 2, C)
        lens = (torch.arange(P) * 3 % 4 + 1).tolist()            # 1 .. 4 rows
        codes, res = _topic_rows(codec, lens, seed=P)
        bank = _build(eng, codec, lens, codes, res, None)
        _BIG.update(eng=eng, codec=codec, bank=bank, lens=lens, codes=codes.numpy())
    return _BIG


def test_more_than_one_selection_slice_over_a_range():
    b = _big()
    eng, codec, bank, lens = b["eng"], b["codec"], b["bank"], b["lens"]
    first, n, ndocs, k = 37, 8900, 1024, 100
    q = _near_queries(codec, 2, 32, seed=11)
    S = _S(eng, codec, q)
    row0 = sum(lens[:first])
    codes = b["codes"][row0:row0 + sum(lens[first:first + n])]
    want = [ref.prune(S[qi][:, :24], codes, None, lens[first:first + n], 2, 0.3, ndocs) for qi in range(2)]
    exact = np.full((2, n), np.nan, dtype=np.float32)             # of the stage-2 survivors: rr_bank_li_scores' MaxSim
    for qi, w in enumerate(want):
        assert len(w["list1"]) == ndocs < int((w["a1"] != ref.NEG_INF).sum()) < n and len(w["list2"]) == ndocs // 4
        ms = eng.bank_li_scores(bank, q[qi:qi + 1], [f"p{first + p}" for p in w["list2"]])["maxsim"]
        exact[qi, w["list2"]] = ms.cpu().numpy()
        w["final"] = ref.final(w["list2"], exact[qi], k)
    got = eng.bank_search_plaid(bank, q, k, ncells=2, centroid_score_threshold=0.3, ndocs=ndocs, coarse_tokens=24, first=first, count=n)
    torch.cuda.synchronize()
    assert np.array_equal(eng.bank_search_plaid_tap("list1").reshape(2, ndocs), _padded([w["list1"] for w in want], ndocs))
    assert np.array_equal(eng.bank_search_plaid_tap("list2").reshape(2, ndocs // 4), _padded([w["list2"] for w in want], ndocs // 4))
    _check_result(got, want, exact, k, add=first)
    assert int(got["indices"].min()) >= first and int(got["indices"].max()) < first + n


def test_sixteen_queries_in_one_call_equal_sixteen_calls_and_two_runs_agree():
    b = _big()
    eng, codec, bank = b["eng"], b["codec"], b["bank"]
    q = _near_queries(codec, 16, 20, seed=13)
    kw = dict(ncells=2, centroid_score_threshold=0.3, ndocs=256, coarse_tokens=12, first=5, count=4500)
    a = eng.bank_search_plaid(bank, q, 64, **kw)
    again = eng.bank_search_plaid(bank, q, 64, **kw)
    torch.cuda.synchronize()
    for key in ("indices", "scores", "counts"):
        assert torch.equal(a[key].view(torch.int32), again[key].view(torch.int32)), f"two runs: {key}"
    assert int(a["counts"].min()) == 64
    for qi in range(16):
        one = eng.bank_search_plaid(bank, q[qi:qi + 1], 64, **kw)
        for key in ("indices", "scores", "counts"):
            assert torch.equal(one[key][0].view(torch.int32), a[key][qi].view(torch.int32)), f"query {qi}: {key}"


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def _raw(eng, bank, q, gi, gs, gc, Lqc=None, first=0, n=-1, ncells=1, thr=0.3, ndocs=16, k=2):
    from rmr_amd import _lib as L
    return eng.lib.rr_bank_search_plaid(eng.h, bank.h, L.ptr(q), q.shape[0], q.shape[1], q.shape[1] if Lqc is None else Lqc, first, n,
                                        ncells, thr, ndocs, k, L.ptr(gi) if gi is not None else None, L.ptr(gs),
                                        L.ptr(gc) if gc is not None else None, torch.cuda.current_stream().cuda_stream)


def _small(eng, D=64, C=64):
    codec = _codec(D, 8, C)
    lens = LEN_CYCLE * 2
    codes, res = _topic_rows(codec, lens, seed=21)
    return codec, _build(eng, codec, lens, codes, res, None)


def test_refusals_write_nothing():
    from rmr_amd import _lib as L
    D = 64
    eng = _bare_engine(D)
    codec, bank = _small(eng)
    q = _near_queries(codec, 2, 9, seed=23)
    gi = torch.full((2, 300), IPOISON, device="cuda", dtype=torch.int32)
    gs = torch.full((2, 300), POISON, device="cuda")
    gc = torch.full((2,), IPOISON, device="cuda", dtype=torch.int32)
    plain = eng.create_bank(64, 4)
    plain.add(["a", "b"], torch.nn.functional.normalize(torch.randn(2, 8, D), dim=-1), torch.ones(2, 8), lengths=[8, 3])
    assert _raw(eng, plain, q, gi, gs, gc, k=1) == L.RR_ERR_UNSUPPORTED and b"fp16 bank" in eng.lib.rr_last_error(eng.h)
    assert _raw(eng, bank, q, gi, gs, gc, ndocs=1025) == L.RR_ERR_UNSUPPORTED and b"1024" in eng.lib.rr_last_error(eng.h)
    assert _raw(eng, bank, q, gi, gs, gc, ndocs=3, k=1) == L.RR_ERR_BAD_SHAPE
    assert _raw(eng, bank, q, gi, gs, gc, ndocs=16, k=5) == L.RR_ERR_BAD_SHAPE                 # k > ndocs / 4
    assert _raw(eng, bank, q, gi, gs, gc, ndocs=1024, k=19) == L.RR_ERR_BAD_SHAPE              # k > the 18 passages
    assert _raw(eng, bank, q, gi, gs, gc, k=0) == L.RR_ERR_BAD_SHAPE
    assert _raw(eng, bank, q, gi, gs, gc, Lqc=10) == L.RR_ERR_BAD_SHAPE                        # Lq_coarse > Lq
    assert _raw(eng, bank, q, gi, gs, gc, Lqc=0) == L.RR_ERR_BAD_SHAPE
    assert _raw(eng, bank, q, gi, gs, gc, ncells=0) == L.RR_ERR_BAD_SHAPE
    assert _raw(eng, bank, q, gi, gs, gc, ncells=17) == L.RR_ERR_UNSUPPORTED
    assert _raw(eng, bank, q, gi, gs, gc, ncells=65) == L.RR_ERR_BAD_SHAPE
    assert _raw(eng, bank, q, gi, gs, None) == L.RR_ERR_BAD_ARG                                # counts_out is required
    assert _raw(eng, bank, q, None, gs, gc) == L.RR_ERR_BAD_ARG
    assert _raw(eng, bank, q, gi, gs, gc, first=1, n=18) == L.RR_ERR_BAD_SHAPE and b"holds 18" in eng.lib.rr_last_error(eng.h)
    assert _raw(_bare_engine(128), bank, q, gi, gs, gc) == L.RR_ERR_BAD_SHAPE                  # another li_dim
    assert _raw(_bare_engine(D, "full_context"), bank, q, gi, gs, gc) == L.RR_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert (gi == IPOISON).all() and (gs == POISON).all() and (gc == IPOISON).all()
    with pytest.raises(NotImplementedError):
        eng.bank_search_plaid(plain, q, 1, ncells=1, centroid_score_threshold=0.3, ndocs=16)
    with pytest.raises(ValueError):
        eng.bank_search_plaid(bank, q, 5, ncells=1, centroid_score_threshold=0.3, ndocs=16)
    with pytest.raises(NotImplementedError):
        eng.bank_search_plaid(bank, q, 1, ncells=1, centroid_score_threshold=0.3, ndocs=1025)
    assert _raw(eng, bank, q, gi[:, :2].contiguous(), None, gc) == 0                           # and what is right is taken
    torch.cuda.synchronize()
    assert gc.tolist() != [IPOISON, IPOISON]


def test_a_capturing_stream_is_refused_and_nothing_is_written():
    from rmr_amd import _lib as L
    eng = _bare_engine(64)
    codec, bank = _small(eng)
    q = _near_queries(codec, 2, 9, seed=25)
    gi = torch.full((2, 2), IPOISON, device="cuda", dtype=torch.int32)
    gs = torch.full((2, 2), POISON, device="cuda")
    gc = torch.full((2,), IPOISON, device="cuda", dtype=torch.int32)
    probe = torch.zeros(1, device="cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        assert _raw(eng, bank, q, gi, gs, gc) == 0                # the table and the block exist: only the capture is in the way
        torch.cuda.synchronize()
        gi.fill_(IPOISON); gs.fill_(POISON); gc.fill_(IPOISON)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            probe.add_(1.0)
            rc = _raw(eng, bank, q, gi, gs, gc)
            msg = eng.lib.rr_last_error(eng.h)
        graph.replay()
        torch.cuda.synchronize()
    assert rc == L.RR_ERR_BAD_ARG and b"captured" in msg
    assert probe.item() == 1.0 and (gi == IPOISON).all() and (gs == POISON).all() and (gc == IPOISON).all()


# ---- 6. adds, a clear, the drop-in class -------------------------------------------------------------------------------------------
def test_search_follows_adds_and_a_clear():
    D, C = 64, 16
    eng = _bare_engine(D)
    codec = _codec(D, 4, C)
    lens = [8, 3, 5, 2, 8, 1, 7]
    codes, res = _topic_rows(codec, lens, seed=31)
    first = np.concatenate([[0], np.cumsum(lens)])
    q = _near_queries(codec, 2, 7, seed=33)
    bank = eng.create_bank(200, 16, codec=codec)
    kw = dict(ncells=C, centroid_score_threshold=0.0, ndocs=1024)                # the degenerate configuration: bank_search's result

    def same(n):
        want, got = eng.bank_search(bank, q, n), eng.bank_search_plaid(bank, q, n, **kw)
        torch.cuda.synchronize()
        assert torch.equal(got["indices"], want["indices"]) and torch.equal(got["scores"], want["scores"]) and got["counts"].tolist() == [n, n]
    bank.add_compressed(["p0", "p1", "p2"], codes[:first[3]], res[:first[3]], lens[:3])
    got = eng.bank_search_plaid(bank, q, 3, **kw)                                 # the pruned search itself uploads the table
    torch.cuda.synchronize()
    assert sorted(got["indices"][0].tolist()) == [0, 1, 2]
    same(3)
    bank.add_compressed(["p3", "p4", "p5", "p6"], codes[first[3]:], res[first[3]:], lens[3:])
    same(7)
    bank.clear()
    bank.add_compressed(["x0", "x1"], codes[first[2]:first[4]], res[first[2]:first[4]], lens[2:4])
    same(2)


def test_retrieve_and_rerank_with_plaid_on_the_drop_in_class():
    from rmr_amd import PlaidSearch
    from test_gpu_passage_bank import _model
    from test_gpu_plaid_bank import _two_queries
    m, g = _model("int_tiny")
    q, qm = _two_queries(g)
    D, Lc = q.shape[2], int(g["Lc"])
    codec = _codec(D, 8, 64)
    P = 24
    lens = [1 + (5 * i) % Lc for i in range(P)]
    codes, res = _topic_rows(codec, lens, seed=41)
    bank = m.create_bank(sum(lens), P, codec=codec)
    names = [("doc", i) for i in range(P)]
    bank.add_compressed(names, codes, res, lens)
    plaid = PlaidSearch(2, 0.0, 16)
    ids, out = m.retrieve_and_rerank(q, qm, 4, plaid=plaid)
    found, scores = m.retrieve(q, 4, plaid=plaid)
    assert ids == found and len(ids) == 2 and all(1 <= len(r) <= 4 and len(set(r)) == len(r) for r in ids)
    ms = m.retriever_scores(q, [pid for row in ids for pid in row], list_sizes=[len(r) for r in ids])["maxsim"]
    assert torch.equal(ms, torch.cat([scores[i, :len(r)] for i, r in enumerate(ids)]))
    ref_out = m.forward_passages(q, qm, [pid for row in ids for pid in row], 3, candidates_per_query=[len(r) for r in ids])
    torch.cuda.synchronize()
    assert out.logits.shape == ref_out.logits.shape and torch.equal(out.logits, ref_out.logits)
