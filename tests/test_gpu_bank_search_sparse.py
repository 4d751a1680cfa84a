"""GPU: the list-driven form of the filtered exact search (rr_bank_search_filtered_sparse; "CANDIDATE FILTERS",
include/rerank_mi355.h) on the 300-passage banks of tests/test_gpu_bank_search_filter.py.

DEFINITION under test: for every argument set rr_bank_search_filtered accepts, the three outputs are that entry's bytes.  So every
case runs both entries on the same arguments into poisoned buffers and compares bytes, and where the exact scores of the range are
at hand also against the numpy restatement of the filtered order (tests/bank_filter_ref.py).  Nothing is compared with the sparse
form itself; no tolerance anywhere.  The counted selection's slice borders are in tests/test_gpu_bank_search_sparse_scale.py."""
import numpy as np
import pytest
import torch

import bank_filter_ref as ref
from test_gpu_bank_li_scores import POISON, _queries
from test_gpu_bank_search import IPOISON
from test_gpu_bank_search_filter import (D, FIRST, FULLY_MASKED, N, NAN_PASSAGE, NQ, P, _checked, _dev_bits, _exact_case, _outputs, _range_bits,
                                         _raw_exact, _same_bytes, _stream)

pytestmark = pytest.mark.gpu


def _raw_sparse(eng, bank, q, out, k, bits, first=FIRST, n=N, rows=None, ld=None, null_filter=False):
    from rmr_amd import _lib as L
    gi, gs, gc = out
    return eng.lib.rr_bank_search_filtered_sparse(eng.h, bank.h, L.ptr(q), q.shape[0], q.shape[1], first, n, k,
                                                  None if null_filter else L.ptr(bits), bits.shape[0] if rows is None else rows,
                                                  bits.shape[1] if ld is None else ld, L.ptr(gi), L.ptr(gs), L.ptr(gc), _stream())


def _sparse_equals_dense(eng, bank, q, k, bits, first=FIRST, n=N, what=""):
    """Both entries on the same arguments, each into its own poisoned buffers: the sparse entry's (indices, scores, counts), which
    are the dense entry's bytes."""
    nq = q.shape[0]
    dense, sparse = _outputs(nq, k), _outputs(nq, k)
    assert _raw_exact(eng, bank, q, dense, k, bits, first=first, n=n) == 0, eng.lib.rr_last_error(eng.h)
    assert _raw_sparse(eng, bank, q, sparse, k, bits, first=first, n=n) == 0, eng.lib.rr_last_error(eng.h)
    torch.cuda.synchronize()
    want, got = _checked(dense, nq, k), _checked(sparse, nq, k)
    _same_bytes(got, want, what)
    return got


def _sparse_equals_ref(eng, bank, q, scores, allowed, k, bits=None, what=""):
    """... over the range [FIRST, FIRST + N), and against filtered_topk on the exact scores of that range."""
    bits = _dev_bits(_range_bits(allowed, FIRST)) if bits is None else bits
    gi, gs, gc = _sparse_equals_dense(eng, bank, q, k, bits, what=what)
    wi, ws, wc = ref.filtered_topk(scores, allowed, k, first=FIRST)
    assert np.array_equal(gc.cpu().numpy(), wc), f"{what}: counts {gc.tolist()} for {wc.tolist()}"
    assert np.array_equal(gi.cpu().numpy(), wi), f"{what}: indices"
    got = gs.cpu().numpy()
    nan = np.isnan(ws)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], ws.view(np.int32)[~nan]), f"{what}: scores"
    return gi, gs, gc


@pytest.mark.parametrize("kind", ["fp16", "nbits8", "nbits2"])
def test_shared_and_per_query_filters(kind):
    eng, bank, q, scores = _exact_case(kind)
    rng = np.random.default_rng(3)
    shared = rng.random((1, N)) < 0.5
    _sparse_equals_ref(eng, bank, q, scores, shared, 20, what="one shared row")
    _sparse_equals_ref(eng, bank, q, scores, shared, N, what="one shared row, k = n")         # k above what the row allows
    three = rng.random((3, N)) < np.array([[0.8], [0.3], [0.05]])
    _sparse_equals_ref(eng, bank, q, scores, three, 20, what="three rows")
    three[1] = False                                              # a row that is empty
    gi, gs, gc = _sparse_equals_ref(eng, bank, q, scores, three, 20, what="an empty row")
    assert gc[1] == 0 and (gi[1] == -1).all() and torch.isneginf(gs[1]).all()
    few = np.zeros((1, N), dtype=bool)
    few[0, [0, 17, 31, 32, N - 1]] = True                         # fewer set bits than k; the first and the last passage of the range
    gi, gs, gc = _sparse_equals_ref(eng, bank, q, scores, few, 20, what="five bits")
    assert gc.tolist() == [5] * NQ


@pytest.mark.parametrize("kind", ["fp16", "nbits2"])
def test_every_bit_set_gives_the_bytes_of_the_unfiltered_search(kind):
    eng, bank, q, scores = _exact_case(kind)
    for rows in (1, NQ):
        ones = _dev_bits(_range_bits(np.ones((rows, N), dtype=bool), FIRST))
        for k in (1, 50, N):
            want = eng.bank_search(bank, q, k, first=FIRST, count=N)
            out = _outputs(NQ, k)
            assert _raw_sparse(eng, bank, q, out, k, ones) == 0, eng.lib.rr_last_error(eng.h)
            torch.cuda.synchronize()
            gi, gs, gc = _checked(out, NQ, k)
            assert torch.equal(gi, want["indices"]) and torch.equal(gs.view(torch.int32), want["scores"].view(torch.int32))
            assert gc.tolist() == [k] * NQ


def test_bits_outside_the_range_and_beyond_the_bank_are_never_consulted():
    eng, bank, q, scores = _exact_case("fp16")
    allowed = np.random.default_rng(4).random((1, N)) < 0.4
    inside = _range_bits(allowed, FIRST, ld=ref.words(P) + 2)     # 12 words: two behind the bank's last
    noisy = inside.copy()
    noisy[0, 0] = 0xffffffff                                      # passages 0 .. 31, in front of the range
    noisy[0, 1] |= np.uint32((1 << (FIRST - 32)) - 1)             # 32 .. 36
    noisy[0, (FIRST + N) >> 5] |= np.uint32(0xffffffff) << np.uint32((FIRST + N) & 31)      # 287 .. 319: behind the range and the bank
    noisy[0, ref.words(P):] = 0xffffffff
    assert not np.array_equal(noisy, inside)
    a = _sparse_equals_ref(eng, bank, q, scores, allowed, 30, bits=_dev_bits(inside), what="clean")
    b = _sparse_equals_ref(eng, bank, q, scores, allowed, 30, bits=_dev_bits(noisy), what="noisy")
    _same_bytes(a, b)


def test_the_nan_passage_and_the_fully_masked_passages():
    eng, bank, q, scores = _exact_case("fp16")
    allowed = np.random.default_rng(6).random((1, N)) < 0.5
    allowed[0, NAN_PASSAGE - FIRST] = True
    gi, gs, gc = _sparse_equals_ref(eng, bank, q, scores, allowed, 5, what="NaN allowed")
    assert gi[:, 0].tolist() == [NAN_PASSAGE] * NQ and torch.isnan(gs[:, 0]).all(), "it ranks first"
    allowed[0, NAN_PASSAGE - FIRST] = False
    gi, gs, gc = _sparse_equals_ref(eng, bank, q, scores, allowed, 5, what="NaN filtered out")
    assert not (gi == NAN_PASSAGE).any() and not torch.isnan(gs).any(), "it is absent"
    for kind in ("fp16", "nbits8"):
        eng, bank, q, scores = _exact_case(kind)
        masked = np.zeros((1, N), dtype=bool)
        masked[0, [p - FIRST for p in FULLY_MASKED]] = True
        masked[0, [3, 200]] = True
        gi, gs, gc = _sparse_equals_ref(eng, bank, q, scores, masked, 10, what=f"{kind}: fully masked passages allowed")
        assert gc.tolist() == [4] * NQ and all(set(FULLY_MASKED) <= set(r[:4]) for r in gi.tolist())


@pytest.mark.parametrize("kind", ["fp16", "nbits8"])
@pytest.mark.parametrize("first,n", [(64, 200), (0, P)])
def test_a_range_on_a_word_border_and_the_whole_bank(kind, first, n):
    eng, bank, q, _ = _exact_case(kind)
    rng = np.random.default_rng(first + n)
    for rows in (1, NQ):
        allowed = rng.random((rows, P)) < 0.3                     # set bits outside the range too
        bits = _dev_bits(ref.pack_bits([np.flatnonzero(r) for r in allowed], P, False))
        gi, gs, gc = _sparse_equals_dense(eng, bank, q, 25, bits, first=first, n=n, what=f"[{first}, {first} + {n}), {rows} rows")
        for qi in range(NQ):
            a = allowed[qi if rows == NQ else 0]
            assert int(gc[qi]) == min(25, int(a[first:first + n].sum())) and all(a[j] and first <= j < first + n for j in gi[qi, :int(gc[qi])].tolist())


@pytest.mark.parametrize("kind", ["fp16", "nbits8"])
def test_chunks_partly_and_wholly_behind_the_count(kind):
    """search_chunk 4: a row of c candidates fills ceil(c / 4) chunks, the last partly when c is no multiple of 4; the other 63 -
    ceil(c / 4) workgroups of the query lie wholly behind the count."""
    eng, bank, q, scores = _exact_case(kind)
    assert eng.lib.rr_set_tuning(b"search_chunk", 4) == 0
    try:
        rng = np.random.default_rng(11)
        for counts in ((1, 4, 5), (16, 17, 1)):
            allowed = np.zeros((3, N), dtype=bool)
            for r, c in enumerate(counts):
                allowed[r, rng.choice(N, size=c, replace=False)] = True
            gi, gs, gc = _sparse_equals_ref(eng, bank, q, scores, allowed, 20, what=f"counts {counts}")
            assert gc.tolist() == [min(c, 20) for c in counts]
    finally:
        assert eng.lib.rr_set_tuning(b"search_chunk", 16) == 0


@pytest.mark.parametrize("kind", ["fp16", "nbits8"])
def test_more_than_one_column_block(kind):
    """Lq 150 at D 64: the column block holds at most 128 query tokens, so a passage's running sum waits in LDS between two blocks
    under the new picker."""
    eng, bank, _, _ = _exact_case(kind)
    q = _queries(NQ, 150, D, seed=78)
    rng = np.random.default_rng(12)
    for rows in (1, NQ):
        allowed = rng.random((rows, N)) < 0.4
        _sparse_equals_dense(eng, bank, q, 20, _dev_bits(_range_bits(allowed, FIRST)), what=f"Lq 150, {rows} rows")


def test_refusals_are_the_dense_entry_s_and_write_nothing():
    from rmr_amd import _lib as L
    eng, bank, q, _ = _exact_case("nbits8")
    bits = _dev_bits(ref.pack_bits([np.arange(P)] * NQ, P, False))               # [3, 10]
    out = _outputs(NQ, 20, extra=0)
    big = _outputs(NQ, 1025, extra=0)

    def call(entry, k=20, o=out, fptr=bits.data_ptr(), rows=NQ, ld=10, counts=True):
        return getattr(eng.lib, entry)(eng.h, bank.h, L.ptr(q), NQ, q.shape[1], FIRST, N, k, fptr, rows, ld, L.ptr(o[0]), L.ptr(o[1]),
                                       L.ptr(o[2]) if counts else None, _stream())
    cases = [
        ("k 0", L.RR_ERR_BAD_SHAPE, dict(k=0)),
        ("k > n", L.RR_ERR_BAD_SHAPE, dict(k=N + 1)),
        ("k 1025", L.RR_ERR_BAD_SHAPE, dict(k=1025, o=big)),       # of 250 passages: refused as k > n, in front of the k > 1024 check (below)
        ("NULL filter", L.RR_ERR_BAD_ARG, dict(fptr=None)),
        ("misaligned filter", L.RR_ERR_BAD_ARG, dict(fptr=bits.data_ptr() + 2)),
        ("filter_rows 2 of 3 queries", L.RR_ERR_BAD_SHAPE, dict(rows=2)),
        ("a short filter_ld", L.RR_ERR_BAD_SHAPE, dict(ld=8)),    # [37, 287) takes nine words
        ("NULL counts_out", L.RR_ERR_BAD_ARG, dict(counts=False)),
    ]
    for what, status, kw in cases:
        dense = call("rr_bank_search_filtered", **kw)
        dense_msg = eng.lib.rr_last_error(eng.h)
        sparse = call("rr_bank_search_filtered_sparse", **kw)
        msg = eng.lib.rr_last_error(eng.h)
        assert dense == status and sparse == dense, f"{what}: {sparse} for the dense entry's {dense}"
        assert msg == dense_msg.replace(b"rr_bank_search_filtered", b"rr_bank_search_filtered_sparse"), f"{what}: {msg}"
        torch.cuda.synchronize()
        for t, poison in zip(out + big, (IPOISON, POISON, IPOISON) * 2):
            assert (t == poison).all(), f"{what}: a refused call writes nothing"
    assert call("rr_bank_search_filtered_sparse", ld=9) == 0      # ... and nine words are taken
    torch.cuda.synchronize()
    assert not (out[2] == IPOISON).any()


def test_k_above_1024_is_unsupported_as_in_the_dense_entry():
    """k = 1025 of 1100 passages: the refusal that is the selection's own (a pass keeps k of 4096)."""
    from rmr_amd import _lib as L
    from test_gpu_li_scores import _engine as _bare_engine
    Pb = 1100
    eng = _bare_engine(D)
    gen = torch.Generator(device="cuda").manual_seed(3)
    li = torch.nn.functional.normalize(torch.randn(Pb, 1, D, generator=gen, device="cuda"), dim=-1).half()
    bank = eng.create_bank(Pb, Pb)
    bank.add(list(range(Pb)), li, torch.ones(Pb, 1), lengths=[1] * Pb)
    q = _queries(2, 8, D, seed=9)
    bits = _dev_bits(ref.pack_bits([np.arange(0, Pb, 3)], Pb, False))
    out = _outputs(2, 1025, extra=0)
    dense = _raw_exact(eng, bank, q, out, 1025, bits, first=0, n=Pb)
    sparse = _raw_sparse(eng, bank, q, out, 1025, bits, first=0, n=Pb)
    assert dense == sparse == L.RR_ERR_UNSUPPORTED and b"rr_bank_search_filtered_sparse: k=1025" in eng.lib.rr_last_error(eng.h)
    torch.cuda.synchronize()
    assert (out[0] == IPOISON).all() and (out[1] == POISON).all() and (out[2] == IPOISON).all()
    _sparse_equals_dense(eng, bank, q, 1024, bits, first=0, n=Pb, what="k 1024 of 367 allowed")


# ---- Python ----------------------------------------------------------------------------------------------------------------------
def test_python_surface_equals_the_dense_path():
    from rmr_amd import search_banks
    from test_gpu_bank_merge import K, OFF, _world
    w = _world("int_tiny")
    m, eng, q, one, three = w["model"], w["eng"], w["q"], w["one"], w["three"]
    names = [f"p{i}" for i in (3, 40, 97, 98, 99, 100, 101, 102, 150, 151, 152, 200, 250, 296, 299)]
    f = one.filter(allowed=names)
    want_ids, want_sc = one.search(eng, q, K, filter=f)
    ids, sc = one.search(eng, q, K, filter=f, sparse=True)
    assert ids == want_ids and torch.equal(sc.view(torch.int32), want_sc.view(torch.int32))
    per_query = one.filter(excluded=[row[:3] for row in want_ids])
    want_ids, want_sc = one.search(eng, q, 12, first=5, count=280, filter=per_query)
    ids, sc = one.search(eng, q, 12, first=5, count=280, filter=per_query, sparse=True)
    assert ids == want_ids and torch.equal(sc.view(torch.int32), want_sc.view(torch.int32))
    had = m.bank
    m.bank = one
    try:
        want_ids, want_sc = m.retrieve(q, K, allowed=names)
        ids, sc = m.retrieve(q, K, allowed=names, sparse=True)
        assert ids == want_ids and torch.equal(sc.view(torch.int32), want_sc.view(torch.int32))
    finally:
        m.bank = had
    filters = [b.filter(allowed=[n for n in names if OFF[i] <= int(n[1:]) < OFF[i + 1]]) for i, b in enumerate(three)]
    want = search_banks(eng, three, q, K, filters=filters)
    got = search_banks(eng, three, q, K, filters=filters, sparse=True)
    assert got[0] == want[0] and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)) and torch.equal(got[2], want[2])
    one_ids, one_sc = one.search(eng, q, K, filter=f, sparse=True)
    assert got[0] == one_ids and torch.equal(got[1].view(torch.int32), one_sc.view(torch.int32)), "three banks as the one bank"
