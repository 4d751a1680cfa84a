"""GPU: the inverted file of a compressed bank built on the device (rr_bank_build_ivf / rr_bank_ivf_info / rr_bank_ivf_read) and
the pruned search that takes its candidates from it (rr_bank_search_plaid_ivf), include/rerank_mi355.h.

1. The file read back equals the host definition (rr_util_plaid_ivf) and the numpy restatement of tests/test_bank_ivf_cpu.py
   exactly, on a bank that crosses every boundary of the build: more passages than one LDS sort slice, a list longer than a
   slice, a passage of more than two 64-row steps with repeated codes, interior masked rows, a fully masked passage, an empty
   list.  Two builds give equal bytes.
2. rr_bank_search_plaid_ivf equals rr_bank_search_plaid bit for bit, poisoned outputs included, over the shapes that search is
   tested at and the edges of the new steps (bitmap word edges, more than one selection slice, ties at every cut, no candidate).
3. Lifetime and refusals.   4. The Python surface.
Exact equality everywhere; no tolerance."""
import numpy as np
import pytest
import torch

from test_bank_ivf_cpu import ivf_lib, ivf_numpy
from test_gpu_bank_li_scores import POISON
from test_gpu_bank_search import IPOISON
from test_gpu_bank_search_plaid import (CONFIGS, K, LEN_CYCLE, NDOCS, THRESHOLD, _big, _build, _case, _codec, _near_queries, _small,
                                        _topic_rows)
from test_gpu_li_scores import _engine as _bare_engine

pytestmark = pytest.mark.gpu


def _outputs(nq, k, extra=1):
    """Poisoned outputs with `extra` rows more than the call writes."""
    return (torch.full((nq + extra, k), IPOISON, device="cuda", dtype=torch.int32), torch.full((nq + extra, k), POISON, device="cuda"),
            torch.full((nq + extra,), IPOISON, device="cuda", dtype=torch.int32))


def _raw(entry, eng, bank, q, out, k, Lqc=None, first=0, n=-1, ncells=1, thr=0.3, ndocs=16):
    from rmr_amd import _lib as L
    gi, gs, gc = out
    return getattr(eng.lib, entry)(eng.h, bank.h, L.ptr(q), q.shape[0], q.shape[1], q.shape[1] if Lqc is None else Lqc, first, n, ncells, thr,
                                   ndocs, k, L.ptr(gi) if gi is not None else None, L.ptr(gs), L.ptr(gc) if gc is not None else None,
                                   torch.cuda.current_stream().cuda_stream)


def _both(eng, bank, q, k, **kw):
    """Both entries on poisoned outputs: every byte equal, nothing written behind the call's rows.  Returns (indices, scores,
    counts) of the call's rows."""
    nq = q.shape[0]
    want, got = _outputs(nq, k), _outputs(nq, k)
    assert _raw("rr_bank_search_plaid", eng, bank, q, want, k, **kw) == 0, eng.lib.rr_last_error(eng.h)
    assert _raw("rr_bank_search_plaid_ivf", eng, bank, q, got, k, **kw) == 0, eng.lib.rr_last_error(eng.h)
    torch.cuda.synchronize()
    for name, w, g in zip(("indices", "scores", "counts"), want, got):
        assert torch.equal(g.view(torch.int32), w.view(torch.int32)), f"{name}: {g[:nq].tolist()} for {w[:nq].tolist()}"
    gi, gs, gc = got
    assert (gi[nq:] == IPOISON).all() and (gs[nq:] == POISON).all() and (gc[nq:] == IPOISON).all()
    cnt = gc[:nq].tolist()
    for qi, c in enumerate(cnt):                                         # -1 / -inf behind the count
        assert 0 <= c <= k and (gi[qi, c:] == -1).all() and torch.isneginf(gs[qi, c:]).all() and (gi[qi, :c] >= 0).all()
    return gi[:nq], gs[:nq], gc[:nq]


# ---- 1. the build --------------------------------------------------------------------------------------------------------------------
P5K, C5K, LONG, LONG_ROWS, EVERYWHERE, UNUSED, ALL_MASKED = 5000, 400, 77, 150, 7, 123, 4000
_B5K = {}


def _bank5k():
    """5 000 passages of 1 .. 5 rows over 400 centroids (two bitmap workgroups of 256); passage LONG holds 150 rows of ten codes in
    turn (0 and C - 1 among them); centroid EVERYWHERE is the first, unmasked row of every passage but ALL_MASKED, whose rows are
    all masked; no row holds UNUSED; every third passage of three rows or more has an interior masked row."""
    if not _B5K:
        eng = _bare_engine(64)
        codec = _codec(64, 2, C5K)
        lens = (torch.arange(P5K) * 3 % 5 + 1).tolist()
        lens[LONG] = LONG_ROWS
        codes, res = _topic_rows(codec, lens, seed=P5K, topics_from=[c for c in range(C5K) if c not in (EVERYWHERE, UNUSED)])
        first = np.concatenate([[0], np.cumsum(lens)])
        mask = torch.ones(len(codes), dtype=torch.uint8)
        ten = torch.tensor([0, C5K - 1, 11, 12, 13, 200, 255, 256, 257, 300], dtype=torch.int32)
        codes[first[LONG]:first[LONG + 1]] = ten[torch.arange(LONG_ROWS) % 10]
        mask[first[LONG] + 5:first[LONG + 1]:7] = 0
        for p in range(0, P5K, 3):
            if lens[p] >= 3:
                mask[first[p] + 1] = 0
        codes[first[:-1]] = EVERYWHERE
        mask[first[:-1]] = 1
        mask[first[ALL_MASKED]:first[ALL_MASKED + 1]] = 0
        bank = _build(eng, codec, lens, codes, res, mask)
        _B5K.update(eng=eng, codec=codec, bank=bank, lens=lens, codes=codes.numpy(), mask=mask.numpy())
    return _B5K


def _read_raw(bank):
    """(offsets, pids) through rr_bank_ivf_read into poisoned host buffers sized by rr_bank_ivf_info."""
    import ctypes
    lib = bank.lib
    p, n, m = ctypes.c_int32(-1), ctypes.c_int64(-1), ctypes.c_int32(-1)
    assert lib.rr_bank_ivf_info(bank.h, ctypes.byref(p), ctypes.byref(n), ctypes.byref(m)) == 0
    offsets = np.full(bank.codec.n_centroids + 2, -7, dtype=np.int64)
    pids = np.full(n.value + 2, -7, dtype=np.int32)
    assert lib.rr_bank_ivf_read(bank.h, offsets.ctypes.data, pids.ctypes.data, torch.cuda.current_stream().cuda_stream) == 0
    assert offsets[-1] == -7 and (pids[n.value:] == -7).all(), "nothing is written behind the file"
    return offsets[:-1], pids[:n.value], dict(passages_covered=p.value, postings=n.value, longest_list=m.value)


def test_the_build_equals_the_definition_and_two_builds_agree():
    b = _bank5k()
    bank, lens, codes, mask = b["bank"], b["lens"], b["codes"], b["mask"]
    info = bank.build_ivf()
    offsets, pids, raw_info = _read_raw(bank)
    want_off, want_pids = ivf_numpy(codes, mask, lens, C5K)
    host_off, host_pids = ivf_lib(codes, mask, lens, C5K)
    assert np.array_equal(host_off, want_off) and np.array_equal(host_pids, want_pids), "the host definition"
    assert np.array_equal(offsets, want_off), "offsets"
    bad = np.flatnonzero(pids != want_pids)
    assert bad.size == 0, f"pids differ at {bad[:5].tolist()}: {pids[bad[:5]].tolist()} for {want_pids[bad[:5]].tolist()}"
    lengths = np.diff(offsets)
    assert info == raw_info == dict(passages_covered=P5K, postings=int(offsets[-1]), longest_list=int(lengths.max()))
    # the fixture bites: a list above one sort slice, lists inside one, an empty one, the long passage once per list
    assert lengths[EVERYWHERE] == P5K - 1 > 4096 and lengths[UNUSED] == 0 and 1 < np.median(lengths[lengths > 0]) < 4096
    assert ALL_MASKED not in pids.tolist()
    for c in (0, C5K - 1, 256):
        lst = pids[offsets[c]:offsets[c + 1]].tolist()
        assert lst.count(LONG) == 1 and lst == sorted(lst)
    bank.build_ivf()
    again_off, again_pids, again_info = _read_raw(bank)
    assert np.array_equal(again_off, offsets) and np.array_equal(again_pids, pids) and again_info == raw_info, "two builds"
    got_pids, got_lengths = bank.ivf()
    assert got_pids.dtype == torch.int32 and got_lengths.dtype == torch.int64
    assert np.array_equal(got_pids.numpy(), pids) and np.array_equal(got_lengths.numpy(), lengths)


# ---- 2. the search equals the scan path ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,Lq,Lqc,ncells", CONFIGS)
def test_search_equals_the_scan_path_at_its_own_shapes(name, Lq, Lqc, ncells):
    eng, codec, bank, q = _case(name, Lq)[:4]
    bank.build_ivf()
    gi, gs, gc = _both(eng, bank, q, K, Lqc=Lqc, ncells=ncells, thr=THRESHOLD, ndocs=NDOCS)
    assert gc.tolist() == [K] * q.shape[0]


@pytest.mark.parametrize("k", [1, 50, 200])
def test_every_centroid_a_cell_and_no_cut_equals_both_searches(k):
    D, C, P = 64, 16, 200
    eng = _bare_engine(D)
    codec = _codec(D, 4, C)
    lens = [LEN_CYCLE[i % len(LEN_CYCLE)] for i in range(P)]
    codes, res = _topic_rows(codec, lens, seed=k)
    masks = [torch.ones(ln, dtype=torch.uint8) for ln in lens]
    for m in masks[::2]:
        m[2::3] = 0                                               # interior masked rows; every passage keeps an unmasked row
    bank = _build(eng, codec, lens, codes, res, torch.cat(masks))
    bank.build_ivf()
    q = _near_queries(codec, 2, 32, seed=3)
    gi, gs, gc = _both(eng, bank, q, k, ncells=C, thr=0.45, ndocs=1024)
    want = eng.bank_search(bank, q, k)
    torch.cuda.synchronize()
    assert torch.equal(gi, want["indices"]) and torch.equal(gs, want["scores"]) and gc.tolist() == [k, k]


def test_a_threshold_that_empties_stage_one_for_some_candidates():
    eng, codec, bank, q = _case("A", 32)[:4]
    bank.build_ivf()
    Lqc, nq, C, P = 20, q.shape[0], codec.n_centroids, len(bank)
    eng.bank_search_plaid(bank, q, K, ncells=2, centroid_score_threshold=0.0, ndocs=NDOCS, coarse_tokens=Lqc)
    S = eng.bank_search_plaid_tap("S").reshape(nq, C, Lqc)
    cells = eng.bank_search_plaid_tap("cells").reshape(nq, C).astype(bool)
    thr = float(np.quantile(S[0].max(axis=1)[cells[0]], 0.75))    # a quarter of query 0's cells is kept, and hardly another centroid
    eng.bank_search_plaid(bank, q, K, ncells=2, centroid_score_threshold=thr, ndocs=NDOCS, coarse_tokens=Lqc)
    a1 = eng.bank_search_plaid_tap("a1").reshape(nq, P)[0]
    empty = np.float32(0.0)
    for _ in range(Lqc):
        empty = np.float32(empty + np.float32(-9999.0))
    cand = ~np.isneginf(a1)
    assert (a1[cand] == empty).any() and (a1[cand] != empty).any(), "some candidates without a kept code, some with"
    _both(eng, bank, q, K, Lqc=Lqc, ncells=2, thr=thr, ndocs=NDOCS)
    gi, gs, gc = _both(eng, bank, q, K, Lqc=Lqc, ncells=2, thr=2.0, ndocs=NDOCS)      # no centroid kept: A1 ties everywhere
    assert gc.tolist() == [K] * nq


def test_a_query_without_a_candidate():
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
    bank.build_ivf()
    gen = torch.Generator().manual_seed(1)
    tok = lambda c: torch.nn.functional.normalize(codec.centroids[c].float()[None] + 0.3 * torch.randn(6, D, generator=gen) / D ** 0.5, dim=-1)
    q = torch.stack([tok(3), tok(45)]).cuda()                     # query 0 near centroid 3, query 1 near a centroid no passage holds
    gi, gs, gc = _both(eng, bank, q, k, ncells=1, thr=0.45, ndocs=32)
    assert gc.tolist() == [3, 0] and sorted(gi[0, :3].tolist()) == holders
    assert (gi[1] == -1).all() and torch.isneginf(gs[1]).all()


def test_sixteen_queries_in_one_call_equal_sixteen_calls():
    b = _big()
    eng, codec, bank = b["eng"], b["codec"], b["bank"]
    bank.build_ivf()
    q = _near_queries(codec, 16, 20, seed=13)
    kw = dict(ncells=2, thr=0.3, ndocs=256, Lqc=12, first=5, n=4500)
    gi, gs, gc = _both(eng, bank, q, 64, **kw)
    assert int(gc.min()) == 64
    for qi in range(16):
        one = _outputs(1, 64)
        assert _raw("rr_bank_search_plaid_ivf", eng, bank, q[qi:qi + 1], one, 64, **kw) == 0
        torch.cuda.synchronize()
        assert torch.equal(one[0][0], gi[qi]) and torch.equal(one[1][0].view(torch.int32), gs[qi].view(torch.int32)) and one[2][0] == gc[qi]


@pytest.mark.parametrize("first,n", [(37, 4900), (1, 4999), (33, 4097), (4063, 31)])
def test_a_range_off_the_bitmap_words_over_more_than_one_selection_slice(first, n):
    """Inside the 5 000-passage bank: first_passage and n_passages no multiples of 32; the longest list covers the bank, so the
    candidate lists have room for the whole range (cap = n: above 4096 two selection slices).  Query 2 opens centroid EVERYWHERE:
    every passage of the range with an unmasked row is its candidate."""
    b = _bank5k()
    eng, codec, bank = b["eng"], b["codec"], b["bank"]
    bank.build_ivf()
    q = _near_queries(codec, 3, 16, seed=17)
    q[2, 0] = torch.nn.functional.normalize(codec.centroids[EVERYWHERE].float(), dim=-1).cuda()
    k = min(100, n // 4)
    gi, gs, gc = _both(eng, bank, q, k, Lqc=12, ncells=2, thr=0.3, ndocs=1024, first=first, n=n)
    assert gc[2] == k and int(gi[gi >= 0].min()) >= first and int(gi.max()) < first + n


def test_ties_across_every_cut_break_by_bank_index():
    """Sixty passages that are twenty copies each of three: A1, A2 and the exact score take three values, so the cut at ndocs, at
    ndocs / 4 and at k each falls inside a run of equal scores and the lower bank index survives."""
    D, C = 64, 320
    eng = _bare_engine(D)
    codec = _codec(D, 4, C)
    three = [3, 5, 2]
    c3, r3 = _topic_rows(codec, three, seed=51, topics_from=list(range(300, 320)))
    f3 = np.concatenate([[0], np.cumsum(three)])
    order = [i % 3 for i in range(60)]
    lens = [three[i] for i in order]
    codes = torch.cat([c3[f3[i]:f3[i + 1]] for i in order])
    res = torch.cat([r3[f3[i]:f3[i + 1]] for i in order])
    bank = _build(eng, codec, lens, codes, res, None)
    bank.build_ivf()
    gen = torch.Generator().manual_seed(52)
    q = torch.nn.functional.normalize(codec.centroids[c3.long()][None, :8].float() + 0.2 * torch.randn(2, 8, D, generator=gen) / D ** 0.5,
                                      dim=-1).cuda()
    gi, gs, gc = _both(eng, bank, q, 4, ncells=4, thr=0.0, ndocs=16)
    assert gc.tolist() == [4, 4]
    for qi in range(2):                                           # 16 of 60 survive stage 1, 4 stage 2: copies of one passage, lowest first
        idx = gi[qi].tolist()
        assert len({i % 3 for i in idx}) == 1 and idx == sorted(idx) and idx[0] < 3 and idx == [idx[0] + 3 * j for j in range(4)]
        assert len(set(gs[qi].tolist())) == 1


# ---- 3. lifetime and refusals --------------------------------------------------------------------------------------------------------
def test_lifetime_adds_a_clear_and_the_covered_prefix():
    from rmr_amd import _lib as L
    D, C = 64, 16
    eng = _bare_engine(D)
    codec = _codec(D, 4, C)
    lens = [8, 3, 5, 2, 8, 1, 7]
    codes, res = _topic_rows(codec, lens, seed=31)
    first = np.concatenate([[0], np.cumsum(lens)])
    q = _near_queries(codec, 2, 7, seed=33)
    bank = eng.create_bank(200, 16, codec=codec)
    bank.add_compressed(["p0", "p1", "p2"], codes[:first[3]], res[:first[3]], lens[:3])
    kw = dict(ncells=2, thr=0.0, ndocs=16)
    out = _outputs(2, 2)
    assert bank.ivf_info() == dict(passages_covered=0, postings=0, longest_list=0)
    assert _raw("rr_bank_search_plaid_ivf", eng, bank, q, out, 2, **kw) == L.RR_ERR_UNSUPPORTED       # no file
    assert b"rr_bank_build_ivf" in eng.lib.rr_last_error(eng.h)
    assert bank.lib.rr_bank_ivf_read(bank.h, None, None, torch.cuda.current_stream().cuda_stream) == L.RR_ERR_BAD_ARG
    with pytest.raises(ValueError):
        bank.ivf()
    assert bank.build_ivf()["passages_covered"] == 3
    _both(eng, bank, q, 2, **kw)
    bank.add_compressed(["p3", "p4", "p5", "p6"], codes[first[3]:], res[first[3]:], lens[3:])
    assert bank.ivf_info()["passages_covered"] == 3
    assert _raw("rr_bank_search_plaid_ivf", eng, bank, q, out, 2, **kw) == L.RR_ERR_UNSUPPORTED       # beyond the covered prefix
    assert b"rr_bank_build_ivf" in eng.lib.rr_last_error(eng.h)
    assert _raw("rr_bank_search_plaid_ivf", eng, bank, q, out, 1, first=2, n=2, **kw) == L.RR_ERR_UNSUPPORTED
    _both(eng, bank, q, 2, first=0, n=3, **kw)                    # within it the file still holds
    _both(eng, bank, q, 1, first=1, n=2, **kw)
    assert bank.build_ivf()["passages_covered"] == 7
    _both(eng, bank, q, 4, **kw)
    _both(eng, bank, q, 1, first=3, n=4, **kw)
    bank.clear()
    assert bank.ivf_info()["passages_covered"] == 0
    bank.add_compressed(["x0", "x1"], codes[first[2]:first[4]], res[first[2]:first[4]], lens[2:4])
    assert _raw("rr_bank_search_plaid_ivf", eng, bank, q, out, 1, **kw) == L.RR_ERR_UNSUPPORTED       # a clear drops the file
    torch.cuda.synchronize()
    assert (out[0] == IPOISON).all() and (out[1] == POISON).all() and (out[2] == IPOISON).all(), "a refused call writes nothing"
    assert bank.build_ivf()["passages_covered"] == 2
    _both(eng, bank, q, 1, **kw)
    with pytest.raises(NotImplementedError):
        eng.bank_search_plaid_ivf(_added(eng, codec), q, 1, ncells=1, centroid_score_threshold=0.3, ndocs=16)


def _added(eng, codec):
    """A compressed bank with two passages and no inverted file."""
    codes, res = _topic_rows(codec, [2, 3], seed=61)
    bank = eng.create_bank(16, 4, codec=codec)
    bank.add_compressed(["a", "b"], codes, res, [2, 3])
    return bank


def test_refusals_write_nothing():
    from rmr_amd import _lib as L
    D = 64
    eng = _bare_engine(D)
    codec, bank = _small(eng)
    bank.build_ivf()
    q = _near_queries(codec, 2, 9, seed=23)
    out = _outputs(2, 300, extra=0)
    gi, gs, gc = out
    ivf = lambda *a, **kw: _raw("rr_bank_search_plaid_ivf", *a, **kw)
    plain = eng.create_bank(64, 4)
    plain.add(["a", "b"], torch.nn.functional.normalize(torch.randn(2, 8, D), dim=-1), torch.ones(2, 8), lengths=[8, 3])
    assert plain.lib.rr_bank_build_ivf(plain.h, torch.cuda.current_stream().cuda_stream) == L.RR_ERR_UNSUPPORTED
    assert b"fp16 bank" in plain.lib.rr_bank_last_error(plain.h)
    with pytest.raises(NotImplementedError):
        plain.build_ivf()
    assert ivf(eng, plain, q, out, 1) == L.RR_ERR_UNSUPPORTED and b"fp16 bank" in eng.lib.rr_last_error(eng.h)
    empty = eng.create_bank(64, 4, codec=codec)
    assert empty.lib.rr_bank_build_ivf(empty.h, torch.cuda.current_stream().cuda_stream) == L.RR_ERR_BAD_SHAPE
    assert ivf(eng, bank, q, out, 2, ndocs=1025) == L.RR_ERR_UNSUPPORTED and b"1024" in eng.lib.rr_last_error(eng.h)
    assert ivf(eng, bank, q, out, 1, ndocs=3) == L.RR_ERR_BAD_SHAPE
    assert ivf(eng, bank, q, out, 5, ndocs=16) == L.RR_ERR_BAD_SHAPE                       # k > ndocs / 4
    assert ivf(eng, bank, q, out, 19, ndocs=1024) == L.RR_ERR_BAD_SHAPE                    # k > the 18 passages
    assert ivf(eng, bank, q, out, 0) == L.RR_ERR_BAD_SHAPE
    assert ivf(eng, bank, q, out, 2, Lqc=10) == L.RR_ERR_BAD_SHAPE                         # Lq_coarse > Lq
    assert ivf(eng, bank, q, out, 2, Lqc=0) == L.RR_ERR_BAD_SHAPE
    assert ivf(eng, bank, q, out, 2, ncells=0) == L.RR_ERR_BAD_SHAPE
    assert ivf(eng, bank, q, out, 2, ncells=17) == L.RR_ERR_UNSUPPORTED
    assert ivf(eng, bank, q, out, 2, ncells=65) == L.RR_ERR_BAD_SHAPE
    assert ivf(eng, bank, q, (gi, gs, None), 2) == L.RR_ERR_BAD_ARG                        # counts_out is required
    assert ivf(eng, bank, q, (None, gs, gc), 2) == L.RR_ERR_BAD_ARG
    assert ivf(eng, bank, q, out, 2, first=1, n=18) == L.RR_ERR_BAD_SHAPE and b"holds 18" in eng.lib.rr_last_error(eng.h)
    assert ivf(_bare_engine(128), bank, q, out, 2) == L.RR_ERR_BAD_SHAPE                   # another li_dim
    assert ivf(_bare_engine(D, "full_context"), bank, q, out, 2) == L.RR_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert (gi == IPOISON).all() and (gs == POISON).all() and (gc == IPOISON).all()
    with pytest.raises(NotImplementedError):
        eng.bank_search_plaid_ivf(plain, q, 1, ncells=1, centroid_score_threshold=0.3, ndocs=16)
    with pytest.raises(ValueError):
        eng.bank_search_plaid_ivf(bank, q, 5, ncells=1, centroid_score_threshold=0.3, ndocs=16)
    assert ivf(eng, bank, q, (gi[:, :2].contiguous(), None, gc), 2) == 0                   # and what is right is taken
    torch.cuda.synchronize()
    assert gc.tolist() != [IPOISON, IPOISON]


def test_a_capturing_stream_is_refused_and_nothing_is_written():
    from rmr_amd import _lib as L
    eng = _bare_engine(64)
    codec, bank = _small(eng)
    bank.build_ivf()
    q = _near_queries(codec, 2, 9, seed=25)
    out = _outputs(2, 2, extra=0)
    gi, gs, gc = out
    probe = torch.zeros(1, device="cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        assert _raw("rr_bank_search_plaid_ivf", eng, bank, q, out, 2) == 0       # the table and the block exist: only the capture is in the way
        torch.cuda.synchronize()
        gi.fill_(IPOISON); gs.fill_(POISON); gc.fill_(IPOISON)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            probe.add_(1.0)
            rc = _raw("rr_bank_search_plaid_ivf", eng, bank, q, out, 2)
            msg = eng.lib.rr_last_error(eng.h)
            rc_build = bank.lib.rr_bank_build_ivf(bank.h, torch.cuda.current_stream().cuda_stream)
            msg_build = bank.lib.rr_bank_last_error(bank.h)
        graph.replay()
        torch.cuda.synchronize()
    assert rc == L.RR_ERR_BAD_ARG and b"captured" in msg
    assert rc_build == L.RR_ERR_BAD_ARG and b"captured" in msg_build
    assert probe.item() == 1.0 and (gi == IPOISON).all() and (gs == POISON).all() and (gc == IPOISON).all()
    assert bank.ivf_info()["passages_covered"] == len(bank), "the refused rebuild left the file"


# ---- 4. the Python surface -----------------------------------------------------------------------------------------------------------
def test_the_python_surface_and_the_saved_file(tmp_path):
    from rmr_amd import PlaidSearch
    b = _bank5k()
    eng, codec, bank = b["eng"], b["codec"], b["bank"]
    info = bank.build_ivf()
    assert eng.bank_build_ivf(bank) == info
    q = _near_queries(codec, 2, 16, seed=71)
    scan, ivf = PlaidSearch(2, 0.3, 64, coarse_tokens=12), PlaidSearch(2, 0.3, 64, coarse_tokens=12, ivf=True)
    want_ids, want_scores = bank.search(eng, q, 10, plaid=scan)
    got_ids, got_scores = bank.search(eng, q, 10, plaid=ivf)
    assert got_ids == want_ids and all(len(r) >= 1 for r in got_ids) and torch.equal(got_scores, want_scores)
    want_ids, _ = bank.search(eng, q, 10, plaid=scan, first=100, count=999)
    got_ids, _ = bank.search(eng, q, 10, plaid=ivf, first=100, count=999)
    assert got_ids == want_ids
    path = bank.save_ivf(str(tmp_path / "index"))
    assert path.endswith("ivf.pid.pt")
    pids, lengths = torch.load(path)
    want_off, want_pids = ivf_numpy(b["codes"], b["mask"], b["lens"], C5K)
    assert pids.dtype == torch.int32 and lengths.dtype == torch.int64
    assert np.array_equal(pids.numpy(), want_pids) and np.array_equal(lengths.numpy(), np.diff(want_off))


def test_retrieve_and_rerank_with_the_inverted_file_on_the_drop_in_class():
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
    bank.add_compressed([("doc", i) for i in range(P)], codes, res, lens)
    with pytest.raises(NotImplementedError):
        m.retrieve(q, 4, plaid=PlaidSearch(2, 0.0, 16, ivf=True))
    bank.build_ivf()
    want_ids, want = m.retrieve_and_rerank(q, qm, 4, plaid=PlaidSearch(2, 0.0, 16))
    got_ids, got = m.retrieve_and_rerank(q, qm, 4, plaid=PlaidSearch(2, 0.0, 16, ivf=True))
    found, scores = m.retrieve(q, 4, plaid=PlaidSearch(2, 0.0, 16, ivf=True))
    found_scan, scores_scan = m.retrieve(q, 4, plaid=PlaidSearch(2, 0.0, 16))
    torch.cuda.synchronize()
    assert got_ids == want_ids == found == found_scan and torch.equal(scores, scores_scan) and torch.equal(got.logits, want.logits)
