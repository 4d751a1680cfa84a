"""GPU: the three bank searches under a caller's candidate filter (rr_bank_search_filtered, rr_bank_search_plaid_filtered,
rr_bank_search_plaid_ivf_filtered, rr_bank_filter_fill; "CANDIDATE FILTERS", include/rerank_mi355.h).

Everything is held to what the library offered before: the exact search to the scores of rr_bank_search over the same range and
the numpy restatement of the filtered order (tests/bank_filter_ref.py); the pruned search to rr_bank_search_plaid on a second bank
whose filtered-out passages are fully masked (PROPERTY B); the inverted-file form to the filtered scan form; all three, with every
bit set, to their unfiltered entries.  Outputs are poisoned first and compared as bytes; no tolerance anywhere.  The filters of
the search tests are packed in numpy and uploaded, so they do not depend on rr_bank_filter_fill, which has its own test."""
import numpy as np
import pytest
import torch

import bank_filter_ref as ref
from test_gpu_bank_li_scores import POISON, _queries
from test_gpu_bank_search import IPOISON
from test_gpu_bank_search_plaid import LEN_CYCLE, _build, _codec, _near_queries, _topic_rows
from test_gpu_li_scores import _engine as _bare_engine

pytestmark = pytest.mark.gpu

D, NQ = 64, 3
P, FIRST, N = 300, 37, 250                 # the range [37, 287): neither end on a bitmap word
FULLY_MASKED = (41, 130)
NAN_PASSAGE = 100


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev_bits(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int32)).cuda()


def _range_bits(allowed: np.ndarray, first: int, passages: int = P, ld=None) -> np.ndarray:
    """The filter uint32 [rows, ld] whose bits of the range [first, first + allowed.shape[1]) are `allowed`, all others clear."""
    full = np.zeros((allowed.shape[0], passages), dtype=bool)
    full[:, first:first + allowed.shape[1]] = allowed
    return ref.pack_bits([np.flatnonzero(r) for r in full], passages, False, ld)


def _outputs(nq, k, extra=1):
    return (torch.full((nq + extra, k), IPOISON, device="cuda", dtype=torch.int32), torch.full((nq + extra, k), POISON, device="cuda"),
            torch.full((nq + extra,), IPOISON, device="cuda", dtype=torch.int32))


def _checked(out, nq, k):
    """Nothing behind the call's rows, -1 / -inf behind every count: (indices, scores, counts) of the call's rows."""
    gi, gs, gc = out
    assert (gi[nq:] == IPOISON).all() and (gs[nq:] == POISON).all() and (gc[nq:] == IPOISON).all()
    for qi, c in enumerate(gc[:nq].tolist()):
        assert 0 <= c <= k and (gi[qi, c:] == -1).all() and torch.isneginf(gs[qi, c:]).all() and (gi[qi, :c] >= 0).all()
    return gi[:nq], gs[:nq], gc[:nq]


def _same_bytes(got, want, what=""):
    for name, g, w in zip(("indices", "scores", "counts"), got, want):
        assert torch.equal(g.view(torch.int32), w.view(torch.int32)), f"{what} {name}: {g.tolist()} for {w.tolist()}"


# ---- the exact search ------------------------------------------------------------------------------------------------------------
def _raw_exact(eng, bank, q, out, k, bits, first=FIRST, n=N, rows=None, ld=None, null_filter=False):
    from rmr_amd import _lib as L
    gi, gs, gc = out
    return eng.lib.rr_bank_search_filtered(eng.h, bank.h, L.ptr(q), q.shape[0], q.shape[1], first, n, k,
                                           None if null_filter else L.ptr(bits), bits.shape[0] if rows is None else rows,
                                           bits.shape[1] if ld is None else ld, L.ptr(gi), L.ptr(gs), L.ptr(gc), _stream())


def _lens_masks():
    lens = [(7 * i) % 40 + 1 for i in range(P)]                   # 1 .. 40 rows
    masks = [torch.ones(ln, dtype=torch.uint8) for ln in lens]
    for i, m in enumerate(masks):
        if i % 3 == 1:
            m[1::2] = 0                                           # interior masked rows
    for i in FULLY_MASKED:
        masks[i][:] = 0
    return lens, masks


_EXACT = {}


def _exact_case(kind):
    """(engine, bank of 300 passages, three queries, the exact scores float32 [3, N] of the range from rr_bank_search with k = N),
    fp16 (with a passage that scores NaN) or compressed, built once."""
    if kind not in _EXACT:
        eng = _bare_engine(D)
        lens, masks = _lens_masks()
        if kind == "fp16":
            gen = torch.Generator().manual_seed(5)
            li = torch.nn.functional.normalize(torch.randn(P, 40, D, generator=gen), dim=-1)
            li[NAN_PASSAGE, 0, 3] = float("nan")                  # its first row is unmasked: the passage scores NaN
            cm = torch.zeros(P, 40)
            for i, m in enumerate(masks):
                cm[i, :lens[i]] = m.float()
            bank = eng.create_bank(sum(lens) + 4, P + 1)
            bank.add([f"p{i}" for i in range(P)], li, cm, lengths=lens)
        else:
            codec = _codec(D, int(kind[5:]), 64)
            codes, res = _topic_rows(codec, lens, seed=9)
            bank = _build(eng, codec, lens, codes, res, torch.cat(masks))
        q = _queries(NQ, 32, D, seed=77)
        r = eng.bank_search(bank, q, N, first=FIRST, count=N)
        torch.cuda.synchronize()
        scores = np.zeros((NQ, N), dtype=np.float32)
        idx, sc = r["indices"].cpu().numpy() - FIRST, r["scores"].cpu().numpy()
        for qi in range(NQ):
            assert sorted(idx[qi].tolist()) == list(range(N))
            scores[qi, idx[qi]] = sc[qi]
        if kind == "fp16":
            assert np.isnan(scores[:, NAN_PASSAGE - FIRST]).all() and np.isnan(scores).sum() == NQ
        _EXACT[kind] = (eng, bank, q, scores)
    return _EXACT[kind]


def _exact_equals_ref(eng, bank, q, scores, allowed, k, bits=None, what=""):
    bits = _dev_bits(_range_bits(allowed, FIRST)) if bits is None else bits
    out = _outputs(NQ, k)
    assert _raw_exact(eng, bank, q, out, k, bits) == 0, eng.lib.rr_last_error(eng.h)
    torch.cuda.synchronize()
    gi, gs, gc = _checked(out, NQ, k)
    wi, ws, wc = ref.filtered_topk(scores, allowed, k, first=FIRST)
    assert np.array_equal(gc.cpu().numpy(), wc), f"{what}: counts {gc.tolist()} for {wc.tolist()}"
    assert np.array_equal(gi.cpu().numpy(), wi), f"{what}: indices"
    got = gs.cpu().numpy()
    nan = np.isnan(ws)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], ws.view(np.int32)[~nan]), f"{what}: scores"
    return gi, gs, gc


@pytest.mark.parametrize("kind", ["fp16", "nbits8", "nbits2"])
def test_exact_search_under_shared_and_per_query_filters(kind):
    eng, bank, q, scores = _exact_case(kind)
    rng = np.random.default_rng(3)
    shared = rng.random((1, N)) < 0.5
    _exact_equals_ref(eng, bank, q, scores, shared, 20, what="one shared row")
    _exact_equals_ref(eng, bank, q, scores, shared, N, what="one shared row, k = n")          # k above what the row allows
    three = rng.random((3, N)) < np.array([[0.8], [0.3], [0.05]])
    _exact_equals_ref(eng, bank, q, scores, three, 20, what="three rows")
    three[1] = False                                              # a row that is empty
    gi, gs, gc = _exact_equals_ref(eng, bank, q, scores, three, 20, what="an empty row")
    assert gc[1] == 0 and (gi[1] == -1).all() and torch.isneginf(gs[1]).all()
    few = np.zeros((1, N), dtype=bool)
    few[0, [0, 17, 31, 32, N - 1]] = True                         # fewer set bits than k; the first and the last passage of the range
    gi, gs, gc = _exact_equals_ref(eng, bank, q, scores, few, 20, what="fewer bits than k")
    assert gc.tolist() == [5] * NQ


def test_exact_search_ignores_bits_outside_the_range_and_beyond_the_bank():
    eng, bank, q, scores = _exact_case("fp16")
    allowed = np.random.default_rng(4).random((1, N)) < 0.4
    inside = _range_bits(allowed, FIRST, ld=ref.words(P) + 2)     # 12 words: two behind the bank's last
    noisy = inside.copy()
    noisy[0, 0] = 0xffffffff                                      # passages 0 .. 31, in front of the range
    noisy[0, 1] |= np.uint32((1 << (FIRST - 32)) - 1)             # 32 .. 36
    noisy[0, (FIRST + N) >> 5] |= np.uint32(0xffffffff) << np.uint32((FIRST + N) & 31)      # 287 .. 319: behind the range and the bank
    noisy[0, ref.words(P):] = 0xffffffff
    assert not np.array_equal(noisy, inside)
    a = _exact_equals_ref(eng, bank, q, scores, allowed, 30, bits=_dev_bits(inside), what="clean")
    b = _exact_equals_ref(eng, bank, q, scores, allowed, 30, bits=_dev_bits(noisy), what="noisy")
    _same_bytes(a, b)


def test_exact_search_with_chunks_the_filter_empties():
    eng, bank, q, scores = _exact_case("nbits8")
    assert eng.lib.rr_set_tuning(b"search_chunk", 4) == 0         # 63 chunks, the last of two passages
    try:
        holes = np.zeros((1, N), dtype=bool)
        holes[0, 8:12] = True                                     # one whole chunk
        holes[0, 101] = holes[0, 203] = True                      # chunks with one allowed passage; every other chunk is empty
        _exact_equals_ref(eng, bank, q, scores, holes, 10, what="empty chunks")
        last = np.zeros((3, N), dtype=bool)
        last[:, N - 1] = True                                     # the last passage of the last, partial chunk alone
        last[2, N - 1] = False
        last[2, N - 2] = True
        gi, gs, gc = _exact_equals_ref(eng, bank, q, scores, last, 3, what="the last passage")
        assert gi[:, 0].tolist() == [FIRST + N - 1, FIRST + N - 1, FIRST + N - 2] and gc.tolist() == [1, 1, 1]
    finally:
        assert eng.lib.rr_set_tuning(b"search_chunk", 16) == 0


def test_a_nan_scoring_passage_allowed_and_filtered_out():
    eng, bank, q, scores = _exact_case("fp16")
    allowed = np.random.default_rng(6).random((1, N)) < 0.5
    allowed[0, NAN_PASSAGE - FIRST] = True
    gi, gs, gc = _exact_equals_ref(eng, bank, q, scores, allowed, 5, what="NaN allowed")
    assert gi[:, 0].tolist() == [NAN_PASSAGE] * NQ and torch.isnan(gs[:, 0]).all(), "it ranks first"
    allowed[0, NAN_PASSAGE - FIRST] = False
    gi, gs, gc = _exact_equals_ref(eng, bank, q, scores, allowed, 5, what="NaN filtered out")
    assert not (gi == NAN_PASSAGE).any() and not torch.isnan(gs).any(), "it is absent"


def test_exact_search_over_more_than_one_selection_pass():
    """4096 + 37 passages of one row: the selection over the dense row takes two slices and a second pass before the list pass."""
    Pb, first = 4096 + 37, 5
    n = Pb - first
    eng = _bare_engine(D)
    gen = torch.Generator(device="cuda").manual_seed(8)
    li = torch.nn.functional.normalize(torch.randn(Pb, 1, D, generator=gen, device="cuda"), dim=-1).half()
    bank = eng.create_bank(Pb, Pb)
    bank.add(list(range(Pb)), li, torch.ones(Pb, 1), lengths=[1] * Pb)
    q = _queries(2, 8, D, seed=9)
    ms = eng.bank_li_scores(bank, q, list(range(first, Pb)) * 2, pair_query=np.repeat(np.arange(2), n), padded_len=1)["maxsim"]
    scores = ms.reshape(2, n).cpu().numpy()
    allowed = np.random.default_rng(8).random((1, n)) < 0.5
    bits = _dev_bits(_range_bits(allowed, first, passages=Pb))
    for k in (100, 1024):
        out = _outputs(2, k)
        assert _raw_exact(eng, bank, q, out, k, bits, first=first, n=n) == 0, eng.lib.rr_last_error(eng.h)
        torch.cuda.synchronize()
        gi, gs, gc = _checked(out, 2, k)
        wi, ws, wc = ref.filtered_topk(scores, allowed, k, first=first)
        assert gc.tolist() == [k, k] and np.array_equal(gi.cpu().numpy(), wi)
        assert np.array_equal(gs.cpu().numpy().view(np.int32), ws.view(np.int32))


# ---- the pruned search -----------------------------------------------------------------------------------------------------------
NDOCS, K, NCELLS, THR = 32, 8, 1, 0.3
_PLAID = {}


def _plaid_case():
    """A compressed bank of 300 passages (lengths around the scan's steps, interior masked rows, two fully masked passages) with
    its inverted file, three queries, and what it was built from."""
    if not _PLAID:
        eng = _bare_engine(D)
        codec = _codec(D, 8, 64)
        lens = [LEN_CYCLE[i % len(LEN_CYCLE)] for i in range(P)]
        codes, res = _topic_rows(codec, lens, seed=12)
        masks = [torch.ones(ln, dtype=torch.uint8) for ln in lens]
        for i, m in enumerate(masks):
            if i % 2:
                m[2::3] = 0
        for i in FULLY_MASKED:
            masks[i][:] = 0
        bank = _build(eng, codec, lens, codes, res, torch.cat(masks))
        bank.build_ivf()
        _PLAID.update(eng=eng, codec=codec, bank=bank, lens=lens, codes=codes, res=res, masks=masks, q=_near_queries(codec, NQ, 32, seed=13))
    return _PLAID


def _masked_twin(c, allowed_row):
    """The bank of _plaid_case with every row of a passage outside `allowed_row` (bool [P]) masked."""
    masks = [m if allowed_row[i] else torch.zeros_like(m) for i, m in enumerate(c["masks"])]
    return _build(c["eng"], c["codec"], c["lens"], c["codes"], c["res"], torch.cat(masks))


def _raw_plaid(entry, eng, bank, q, out, k, bits=None, first=0, n=-1, rows=None, ld=None, null_filter=False, ncells=NCELLS, thr=THR,
               ndocs=NDOCS, Lqc=20):
    from rmr_amd import _lib as L
    gi, gs, gc = out
    fargs = [] if bits is None and not null_filter else [None if null_filter else L.ptr(bits), bits.shape[0] if rows is None else rows,
                                                         bits.shape[1] if ld is None else ld]
    return getattr(eng.lib, entry)(eng.h, bank.h, L.ptr(q), q.shape[0], q.shape[1], Lqc, first, n, ncells, thr, ndocs, k, *fargs,
                                   L.ptr(gi), L.ptr(gs), L.ptr(gc), _stream())


def _run(entry, eng, bank, q, k, **kw):
    out = _outputs(q.shape[0], k)
    assert _raw_plaid(entry, eng, bank, q, out, k, **kw) == 0, eng.lib.rr_last_error(eng.h)
    torch.cuda.synchronize()
    return _checked(out, q.shape[0], k)


@pytest.mark.parametrize("first,n", [(0, P), (FIRST, N)])
def test_pruned_search_property_b_shared_filter(first, n):
    c = _plaid_case()
    eng, bank, q = c["eng"], c["bank"], c["q"]
    allowed = np.zeros(P, dtype=bool)
    allowed[first:first + n] = np.random.default_rng(21).random(n) < 0.5
    bits = _dev_bits(ref.pack_bits([np.flatnonzero(allowed)], P, False))
    plain = _run("rr_bank_search_plaid", eng, bank, q, K, first=first, n=n)
    a1_plain = eng.bank_search_plaid_tap("a1").reshape(NQ, n)
    got = _run("rr_bank_search_plaid_filtered", eng, bank, q, K, bits=bits, first=first, n=n)
    a1 = eng.bank_search_plaid_tap("a1").reshape(NQ, n)           # the tap covers the filtered entry
    cand_plain, cand = ~np.isneginf(a1_plain), ~np.isneginf(a1)
    assert np.array_equal(cand, cand_plain & allowed[None, first:first + n]), "candidates: bit set AND a code in the cell set"
    for qi in range(NQ):                                          # the filter removes some candidates of every query, not all
        assert 0 < cand[qi].sum() < cand_plain[qi].sum() < n, (cand[qi].sum(), cand_plain[qi].sum())
    assert np.array_equal(a1.view(np.int32)[cand], a1_plain.view(np.int32)[cand]), "A1 of a surviving candidate is unchanged"
    want = _run("rr_bank_search_plaid", eng, _masked_twin(c, allowed), q, K, first=first, n=n)
    _same_bytes(got, want, "PROPERTY B")
    assert not all(torch.equal(g, p) for g, p in zip(got, plain)), "the filter changed the result"
    _same_bytes(_run("rr_bank_search_plaid_ivf_filtered", eng, bank, q, K, bits=bits, first=first, n=n), got, "inverted-file form")


def test_pruned_search_property_b_per_query_filter():
    c = _plaid_case()
    eng, bank, q = c["eng"], c["bank"], c["q"]
    allowed = np.random.default_rng(22).random((NQ, P)) < np.array([[0.7], [0.4], [0.2]])
    bits = _dev_bits(ref.pack_bits([np.flatnonzero(r) for r in allowed], P, False))
    got = _run("rr_bank_search_plaid_filtered", eng, bank, q, K, bits=bits)
    ivf = _run("rr_bank_search_plaid_ivf_filtered", eng, bank, q, K, bits=bits)
    _same_bytes(ivf, got, "inverted-file form")
    for qi in range(NQ):                                          # query by query, each against its own masked bank
        want = _run("rr_bank_search_plaid", eng, _masked_twin(c, allowed[qi]), q[qi:qi + 1].contiguous(), K)
        _same_bytes([g[qi:qi + 1] for g in got], want, f"PROPERTY B, query {qi}")


@pytest.mark.parametrize("first,n", [(0, P), (32, 200), (FIRST, N), (FIRST, 37), (1, 31)])
def test_inverted_file_form_equals_the_filtered_scan_form(first, n):
    """first 0 and 32: a bitmap word is one filter word; 37 and 1: it takes its bits from two (the funnel shift); n = 200, 250, 37,
    31: the range's last bitmap word is partial; [1, 32) lies inside one filter word."""
    c = _plaid_case()
    eng, bank, q = c["eng"], c["bank"], c["q"]
    rng = np.random.default_rng(100 * first + n)
    k = min(K, n // 4)
    for rows in (1, NQ):
        allowed = rng.random((rows, P)) < 0.5                      # set bits outside the range too: they change nothing
        if rows == NQ:
            allowed[1, first:first + n] = False                    # a filter that leaves query 1 no candidate
        bits = _dev_bits(ref.pack_bits([np.flatnonzero(r) for r in allowed], P, False))
        scan = _run("rr_bank_search_plaid_filtered", eng, bank, q, k, bits=bits, first=first, n=n, ncells=2)
        ivf = _run("rr_bank_search_plaid_ivf_filtered", eng, bank, q, k, bits=bits, first=first, n=n, ncells=2)
        _same_bytes(ivf, scan, f"rows {rows}")
        idx = scan[0].cpu().numpy()
        for qi in range(NQ):
            assert all(allowed[qi if rows == NQ else 0, j] and first <= j < first + n for j in idx[qi][idx[qi] >= 0])
        if rows == NQ:
            assert scan[2][1] == 0 and (n < 200 or scan[2][0] > 0)


def test_every_bit_set_gives_the_unfiltered_bytes():
    c = _plaid_case()
    eng, bank, q = c["eng"], c["bank"], c["q"]
    for rows in (1, NQ):
        ones = _dev_bits(ref.pack_bits([np.arange(P)] * rows, P, False))
        for first, n in ((0, P), (FIRST, N)):
            for entry in ("rr_bank_search_plaid", "rr_bank_search_plaid_ivf"):
                want = _run(entry, eng, bank, q, K, first=first, n=n, ncells=2)
                _same_bytes(_run(entry + "_filtered", eng, bank, q, K, bits=ones, first=first, n=n, ncells=2), want, entry)
    for kind in ("fp16", "nbits2"):
        eng, bank, q, scores = _exact_case(kind)
        ones = _dev_bits(_range_bits(np.ones((1, N), dtype=bool), FIRST))       # every bit of the range, none outside
        for k in (1, 50, N):
            want = eng.bank_search(bank, q, k, first=FIRST, count=N)
            out = _outputs(NQ, k)
            assert _raw_exact(eng, bank, q, out, k, ones) == 0
            torch.cuda.synchronize()
            gi, gs, gc = _checked(out, NQ, k)
            assert torch.equal(gi, want["indices"]) and torch.equal(gs.view(torch.int32), want["scores"].view(torch.int32))
            assert gc.tolist() == [k] * NQ


def test_missing_and_stale_inverted_file_refusals_are_unchanged():
    from rmr_amd import _lib as L
    eng = _bare_engine(D)
    codec = _codec(D, 4, 16)
    lens = [8, 3, 5, 2, 8, 1, 7]
    codes, res = _topic_rows(codec, lens, seed=31)
    f = np.concatenate([[0], np.cumsum(lens)])
    q = _near_queries(codec, 2, 7, seed=33)
    bank = eng.create_bank(200, 16, codec=codec)
    bank.add_compressed(["p0", "p1", "p2"], codes[:f[3]], res[:f[3]], lens[:3])
    ones = _dev_bits(np.full((1, 1), 0xffffffff, dtype=np.uint32))
    kw = dict(bits=ones, ncells=2, thr=0.0, ndocs=16, Lqc=7)
    out = _outputs(2, 2, extra=0)
    entry = "rr_bank_search_plaid_ivf_filtered"
    assert _raw_plaid(entry, eng, bank, q, out, 2, **kw) == L.RR_ERR_UNSUPPORTED and b"rr_bank_build_ivf" in eng.lib.rr_last_error(eng.h)
    assert _raw_plaid(entry, eng, bank, q, out, 2, **{**kw, "null_filter": True}) == L.RR_ERR_UNSUPPORTED, "in front of the filter checks"
    bank.build_ivf()
    bank.add_compressed(["p3", "p4", "p5", "p6"], codes[f[3]:], res[f[3]:], lens[3:])
    assert _raw_plaid(entry, eng, bank, q, out, 2, **kw) == L.RR_ERR_UNSUPPORTED and b"rr_bank_build_ivf" in eng.lib.rr_last_error(eng.h)
    torch.cuda.synchronize()
    assert (out[0] == IPOISON).all() and (out[1] == POISON).all() and (out[2] == IPOISON).all()
    _same_bytes(_run(entry, eng, bank, q, 1, first=0, n=3, **kw), _run("rr_bank_search_plaid_filtered", eng, bank, q, 1, first=0, n=3, **kw))


def test_filter_refusals_write_nothing():
    from rmr_amd import _lib as L
    c = _plaid_case()
    eng, bank, q = c["eng"], c["bank"], c["q"]
    bits = _dev_bits(ref.pack_bits([np.arange(P)] * NQ, P, False))               # [3, 10]
    out = _outputs(NQ, K, extra=0)
    calls = [lambda **kw: _raw_exact(eng, bank, q, out, K, bits, **kw)] + \
            [lambda e=e, **kw: _raw_plaid(e, eng, bank, q, out, K, bits=bits, **kw)
             for e in ("rr_bank_search_plaid_filtered", "rr_bank_search_plaid_ivf_filtered")]
    for call in calls:
        assert call(null_filter=True) == L.RR_ERR_BAD_ARG and b"filter_bits" in eng.lib.rr_last_error(eng.h)
        assert call(rows=2) == L.RR_ERR_BAD_SHAPE and b"filter_rows" in eng.lib.rr_last_error(eng.h)      # 2 rows for 3 queries
        assert call(first=0, n=P, ld=9) == L.RR_ERR_BAD_SHAPE and b"filter_ld" in eng.lib.rr_last_error(eng.h)
        assert call(first=FIRST, n=N, ld=8) == L.RR_ERR_BAD_SHAPE                 # [37, 287) takes nine words
        torch.cuda.synchronize()
        assert (out[0] == IPOISON).all() and (out[1] == POISON).all() and (out[2] == IPOISON).all(), "a refused call writes nothing"
        assert call(first=FIRST, n=N, ld=9) == 0                                  # ... and nine are taken
        torch.cuda.synchronize()
        for t, poison in zip(out, (IPOISON, POISON, IPOISON)):
            assert not (t == poison).all()
            t.fill_(poison)
    assert _raw_exact(eng, bank, q, (out[0], out[1], None), K, bits) == L.RR_ERR_BAD_ARG                   # counts_out is required
    assert eng.lib.rr_bank_search_filtered(eng.h, None, L.ptr(q), NQ, q.shape[1], FIRST, N, K, L.ptr(bits), NQ, bits.shape[1], L.ptr(out[0]),
                                           L.ptr(out[1]), None, _stream()) == L.RR_ERR_BAD_ARG              # ... beside the null bank, as one check
    assert _raw_exact(eng, bank, q, out, N + 1, bits) == L.RR_ERR_BAD_SHAPE       # the refusals of rr_bank_search stand
    torch.cuda.synchronize()
    assert (out[0] == IPOISON).all() and (out[1] == POISON).all() and (out[2] == IPOISON).all()
    f = c["bank"].filter(allowed=["p1"])
    with pytest.raises(ValueError, match="rows"):
        eng.bank_search_filtered(bank, q[:2], K, type(f)(bits, NQ, P))
    with pytest.raises(ValueError, match="built for 100"):
        eng.bank_search_plaid_filtered(bank, q, K, type(f)(bits, NQ, 100), ncells=1, centroid_score_threshold=0.3, ndocs=NDOCS)


# ---- rr_bank_filter_fill ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exclude", [0, 1])
def test_filter_fill_equals_the_host_restatement_and_repeats(exclude):
    c = _plaid_case()
    bank = c["bank"]
    lib = bank.lib
    rng = np.random.default_rng(40 + exclude)
    rows = [rng.integers(0, P, size=150).tolist() + [0, P - 1, P - 1], [], rng.integers(0, P, size=5000).tolist()]      # repeats; empty; long
    idx = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows])
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    ld = ref.words(P) + 2
    want = np.zeros((3, ld), dtype=np.uint32)
    assert lib.rr_util_bank_filter_bits(idx.ctypes.data, off.ctypes.data, 3, exclude, P, want.ctypes.data, ld) == 0
    assert np.array_equal(want, ref.pack_bits(rows, P, bool(exclude), ld))
    runs = []
    for _ in range(2):
        dev = torch.full((4, ld), IPOISON, device="cuda", dtype=torch.int32)
        assert lib.rr_bank_filter_fill(bank.h, idx.ctypes.data, off.ctypes.data, 3, exclude, dev.data_ptr(), ld, _stream()) == 0, \
            lib.rr_bank_last_error(bank.h)
        torch.cuda.synchronize()
        assert (dev[3] == IPOISON).all(), "nothing behind the rows"
        runs.append(dev[:3].cpu().numpy().view(np.uint32))
    assert np.array_equal(runs[0], want) and np.array_equal(runs[1], want)
    dev = torch.full((3, ld), IPOISON, device="cuda", dtype=torch.int32)
    from rmr_amd import _lib as L
    bad = idx.copy()
    bad[7] = P
    assert lib.rr_bank_filter_fill(bank.h, bad.ctypes.data, off.ctypes.data, 3, exclude, dev.data_ptr(), ld, _stream()) == L.RR_ERR_BAD_SHAPE
    assert lib.rr_bank_filter_fill(bank.h, idx.ctypes.data, off.ctypes.data, 3, exclude, dev.data_ptr(), ref.words(P) - 1, _stream()) \
        == L.RR_ERR_BAD_SHAPE
    torch.cuda.synchronize()
    assert (dev == IPOISON).all(), "a refused fill writes nothing"
    ids = [[f"p{j}" for j in r] for r in rows]
    f = bank.filter(excluded=ids) if exclude else bank.filter(allowed=ids)
    torch.cuda.synchronize()
    assert (f.rows, f.passages, tuple(f.bits.shape)) == (3, P, (3, ref.words(P)))
    assert np.array_equal(f.bits.cpu().numpy().view(np.uint32), want[:, :ref.words(P)])


# ---- Python ----------------------------------------------------------------------------------------------------------------------
def test_passage_bank_search_with_a_filter():
    from rmr_amd import PlaidSearch
    c = _plaid_case()
    eng, bank, q = c["eng"], c["bank"], c["q"]
    top, _ = bank.search(eng, q, 12)
    f = bank.filter(excluded=[row[:3] for row in top])            # a row per query: what the query has been shown
    ids, scores = bank.search(eng, q, 9, filter=f)
    assert ids == [row[3:] for row in top]
    few = bank.filter(allowed=top[0][:4])                         # one shared row of four passages
    ids, scores = bank.search(eng, q, 9, filter=few)
    assert all(sorted(r) == sorted(top[0][:4]) for r in ids) and ids[0] == top[0][:4] and torch.isneginf(scores[:, 4:]).all()
    for plaid in (PlaidSearch(2, 0.3, 64, coarse_tokens=20), PlaidSearch(2, 0.3, 64, coarse_tokens=20, ivf=True)):
        found, _ = bank.search(eng, q, 10, plaid=plaid)
        ids, _ = bank.search(eng, q, 10, plaid=plaid, filter=bank.filter(excluded=[r[:2] for r in found]))
        assert all(not set(r) & set(fr[:2]) and len(r) >= 1 for r, fr in zip(ids, found))


def test_retrieve_excluded_and_rerank_allowed_on_the_drop_in_class():
    from test_gpu_passage_bank import _model
    from test_gpu_plaid_bank import _two_queries
    m, g = _model("int_tiny")
    q, qm = _two_queries(g)
    Dm, Lc = q.shape[2], int(g["Lc"])
    gen = torch.Generator().manual_seed(71)
    Pm, k = 40, 6
    lens = [1 + (5 * i) % Lc for i in range(Pm)]
    li = torch.nn.functional.normalize(torch.randn(Pm, Lc, Dm, generator=gen), dim=-1)
    cm = (torch.arange(Lc)[None, :] < torch.tensor(lens)[:, None]).float()
    bank = m.create_bank(sum(lens), Pm)
    names = [("doc", i) for i in range(Pm)]
    bank.add(names, li, cm, lengths=lens)
    top, top_scores = m.retrieve(q, k + 3)
    ids, scores = m.retrieve(q, k, excluded=[row[:3] for row in top])
    assert ids == [row[3:] for row in top] and torch.equal(scores, top_scores[:, 3:])
    allowed = names[3:30:4]                                       # seven passages for both queries
    got_ids, out = m.retrieve_and_rerank(q, qm, k, allowed=allowed)
    assert all(len(r) == k and set(r) <= set(allowed) for r in got_ids)
    want = m.forward_passages(q, qm, [pid for row in got_ids for pid in row], k - 1, candidates_per_query=[k, k])
    torch.cuda.synchronize()
    assert torch.equal(out.logits, want.logits)
    with pytest.raises(ValueError, match="found no candidate"):
        m.retrieve_and_rerank(q, qm, k, allowed=[[names[0]], []])
    with pytest.raises(KeyError):
        m.retrieve(q, k, excluded=[("doc", Pm)])
