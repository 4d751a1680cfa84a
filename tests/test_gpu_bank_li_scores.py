"""GPU: rr_bank_li_scores — the retriever's MaxSim and score matrix (colbert_score, flmr_utils.py:22-48) straight from a passage
bank, fp16 or compressed, through RerankEngine.bank_li_scores, PassageBank.maxsim and InteractionRerankModel.retriever_scores.

Contract (include/rerank_mi355.h): the outputs are bit for bit what rr_li_scores returns with K = 1, query_li[pair_query] per
pair, context_li = float32(the bank's rows) zero-padded to padded_context_len and context_mask = the bank's mask bytes.  Every
equality below is torch.equal.  The float64 check of the fp16 cases uses the bounds derived in tests/test_gpu_li_scores.py, each
multiplied by (1 + 2^-10): a unit row rounded to fp16 exceeds norm 1 by at most 2^-11.

A handle's li_dim is a multiple of 64 (rr_create), so the dimension 16 — one step of the kernel's walk over D, and the only
dimension at which a wave decodes fewer rows per pass than its lanes could take — is reached through the raw-pointer operators
rr_op_bank_li_scores / rr_op_li_scores (include/rerank_mi355_diag.h), which launch the same kernels: test_dimension_16_*."""

import numpy as np
import pytest
import torch

from helpers import record_margin
from li_scores_ref import MASKED, li_scores_formula
from test_gpu_li_scores import _bounds
from test_gpu_li_scores import _engine as _bare_engine
from test_gpu_plaid_bank import N_CENTROIDS, _codec, _engine, _fp16_twin, _rows, _two_queries

pytestmark = pytest.mark.gpu

POISON = 12345.5
LENS = [1, 15, 16, 17, 40, 64]          # below, at and above a 16-row tile; 64 = a padded length of 64 without pad rows
FULLY_MASKED = 3                         # the passage of 17 rows
PAIR_PASSAGE = [5, 2, 0, 3, 5, 1, 4, 2, 3, 0, 5, 4]      # shuffled, every passage, repeats
PAIR_QUERY = [2, 0, 1, 1, 0, 2, 1, 0, 2, 0, 1, 2]        # not monotone


def _mask(lens, full=FULLY_MASKED):
    """One row of mask bytes per passage at its own length: interior holes, passage `full` all zero."""
    rows = []
    for i, ln in enumerate(lens):
        m = torch.ones(ln, dtype=torch.uint8)
        m[2::3] = 0
        if i == full:
            m[:] = 0
        rows.append(m)
    return rows


def _queries(n, Lq, D, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, Lq, D, generator=gen), dim=-1).cuda()


def _fp16_bank(eng, D, seed, lens=LENS, full=FULLY_MASKED):
    """An fp16 bank of unit rows under the ids "p0", "p1", ... with _mask's masks."""
    gen = torch.Generator().manual_seed(seed)
    Lc = max(lens)
    li = torch.nn.functional.normalize(torch.randn(len(lens), Lc, D, generator=gen), dim=-1)
    cm = torch.zeros(len(lens), Lc)
    for i, m in enumerate(_mask(lens, full)):
        cm[i, :lens[i]] = m.float()
    bank = eng.create_bank(sum(lens) + 4, len(lens) + 1)
    bank.add([f"p{i}" for i in range(len(lens))], li, cm, lengths=lens)
    return bank


def _plaid_bank(eng, D, nbits, seed, lens=LENS):
    """A compressed bank under the same ids: _rows' random codes (row 0: the zero-norm row) and _mask's masks."""
    codec = _codec(D, nbits)
    codes, res = _rows(codec, sum(lens), seed)
    bank = eng.create_bank(sum(lens) + 4, len(lens) + 1, codec=codec)
    bank.add_compressed([f"p{i}" for i in range(len(lens))], codes, res, lens, mask=torch.cat(_mask(lens)))
    return bank


def _padded(bank, passages, Lc):
    """What the contract hands rr_li_scores in the bank's place: float32(bank.read rows) zero-padded to Lc and the mask bytes as
    floats, one entry per pair."""
    c = torch.zeros(len(passages), Lc, bank.li_dim)
    cm = torch.zeros(len(passages), Lc)
    for i, p in enumerate(passages):
        rows, mask = bank.read(f"p{p}")
        c[i, :rows.shape[0]], cm[i, :rows.shape[0]] = rows.float(), mask.float()
    return c, cm


def _ids(passages):
    return [f"p{p}" for p in passages]


def _check_against_li_scores(eng, bank, q, Lc, tag=None):
    """scores + MaxSim, MaxSim only and a second call of bank_li_scores on the module's pair list, against eng.li_scores (K = 1) on
    the padded float32 rows; the output discipline of pad rows and the fully masked passage; with `tag` the float64 bounds too."""
    Lq, D = q.shape[1], q.shape[2]
    c, cm = _padded(bank, PAIR_PASSAGE, Lc)
    qsel = q[PAIR_QUERY].contiguous()
    ref = eng.li_scores(qsel, c.cuda(), cm.cuda(), len(PAIR_PASSAGE), 1)
    kw = dict(pair_query=PAIR_QUERY, padded_len=Lc)
    got = eng.bank_li_scores(bank, q, _ids(PAIR_PASSAGE), want_scores=True, **kw)
    only = eng.bank_li_scores(bank, q, _ids(PAIR_PASSAGE), **kw)
    again = eng.bank_li_scores(bank, q, _ids(PAIR_PASSAGE), want_scores=True, **kw)
    torch.cuda.synchronize()
    assert got["scores"].shape == (len(PAIR_PASSAGE), Lc, Lq) and got["maxsim"].shape == (len(PAIR_PASSAGE),)
    assert torch.equal(got["scores"], ref["scores"]), \
        f"scores differ from rr_li_scores: {(got['scores'] - ref['scores']).abs().max().item():.3e}"
    assert torch.equal(got["maxsim"], ref["maxsim"])
    assert "scores" not in only and torch.equal(only["maxsim"], got["maxsim"])
    assert torch.equal(again["scores"], got["scores"]) and torch.equal(again["maxsim"], got["maxsim"])
    sc, ms = got["scores"].cpu(), got["maxsim"].cpu()
    for i, p in enumerate(PAIR_PASSAGE):
        assert (sc[i, LENS[p]:] == MASKED).all(), "rows at or beyond a passage's length are -9999"
        if p == FULLY_MASKED:
            assert (sc[i] == MASKED).all() and ms[i].item() == MASKED * Lq
    assert (sc[~cm.bool()] == MASKED).all() and bool(torch.isfinite(sc).all())
    if tag is not None:
        m64, s64 = li_scores_formula(qsel.cpu(), c, cm, 1, torch.float64)
        keep = cm.bool()
        d_s, d_m = (sc.double() - s64)[keep].abs().max().item(), (ms.double() - m64).abs().max().item()
        b_s, b_m = (b * (1.0 + 2.0 ** -10) for b in _bounds(D, Lq))
        print(f"[{tag}] scores |d| {d_s:.3e} (bound {b_s:.3e}), maxsim |d| {d_m:.3e} (bound {b_m:.3e})")
        record_margin(f"bank_li_scores/{tag}", scores_max_abs=d_s, scores_bound=b_s, maxsim_max_abs=d_m, maxsim_bound=b_m)
        assert d_s <= b_s and d_m <= b_m
    return got


# ---- 1. fp16 bank == rr_li_scores ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lq", [1, 16, 17, 33, 65, 113, 130])          # the JT thresholds, and a second column block
@pytest.mark.parametrize("D", [64, 128, 512])                          # the shapes in use; 512: the LDS rule halves JT
def test_fp16_bank_equals_li_scores_bit_for_bit(D, Lq):
    eng = _bare_engine(D)
    bank = _fp16_bank(eng, D, seed=1000 + D + Lq)
    q = _queries(3, Lq, D, seed=D + Lq)
    for Lc in (64, 70):                                                 # the pad rows end on a tile boundary and inside a tile
        _check_against_li_scores(eng, bank, q, Lc, tag=f"D{D}_Lq{Lq}_Lc{Lc}")


# ---- 2. compressed bank == its fp16 twin == rr_li_scores -------------------------------------------------------------------------
@pytest.mark.parametrize("D,nbits,Lq", [(64, 1, 33), (64, 2, 113), (64, 4, 17), (64, 8, 130), (128, 1, 130), (128, 2, 16),
                                        (128, 4, 65), (128, 8, 113), (512, 8, 33)])
def test_compressed_bank_equals_its_fp16_twin_bit_for_bit(D, nbits, Lq):
    eng = _bare_engine(D)
    bank = _plaid_bank(eng, D, nbits, seed=7 * D + nbits)
    rows0, _ = bank.read("p0")
    assert not bool(rows0[0].view(torch.int16).any()), "bank row 0 is the zero-norm row"
    twin = _fp16_twin(eng, bank, LENS, max(LENS))
    q = _queries(3, Lq, D, seed=D + nbits)
    for Lc in (64, 70):
        got = _check_against_li_scores(eng, bank, q, Lc)               # through read()'s rows: against rr_li_scores
        ref = eng.bank_li_scores(twin, q, _ids(PAIR_PASSAGE), pair_query=PAIR_QUERY, padded_len=Lc, want_scores=True)
        torch.cuda.synchronize()
        assert torch.equal(got["scores"], ref["scores"]) and torch.equal(got["maxsim"], ref["maxsim"])


def _pairs_dev(first_rows, lens, queries):
    """rr_bank_pair [n] {int64 first_row; int32 len; int32 query} on the device."""
    a = np.zeros(len(lens), dtype=np.dtype([("first", "<i8"), ("len", "<i4"), ("query", "<i4")]))
    a["first"], a["len"], a["query"] = first_rows, lens, queries
    return torch.from_numpy(a.view(np.uint8).copy()).cuda()


@pytest.mark.parametrize("Lq", [1, 16, 17, 33, 65, 113, 130])
def test_dimension_16_fp16_and_nbits_1_through_the_raw_operators(Lq):
    """D = 16: the fp16 rows against rr_op_li_scores (the kernel of rr_li_scores) bit for bit and against float64, and nbits 1
    codes against the fp16 rows the host decoder gives (rr_util_plaid_decode_rows: what rr_bank_read returns)."""
    from rmr_amd import _lib as L
    lib = L.load()
    D, st = 16, torch.cuda.current_stream().cuda_stream
    codec = _codec(D, 1)
    codes, res = _rows(codec, sum(LENS), seed=160 + Lq)
    decoded = codec.decode(codes, res)                                  # [R, 16] fp16; row 0 has norm zero
    assert not bool(decoded[0].view(torch.int16).any())
    gen = torch.Generator().manual_seed(16 + Lq)
    plain = torch.nn.functional.normalize(torch.randn(sum(LENS), D, generator=gen), dim=-1).half()    # the fp16 case: unit rows
    mask = torch.cat(_mask(LENS))
    first = np.concatenate([[0], np.cumsum(LENS)[:-1]])
    pairs = _pairs_dev(first[PAIR_PASSAGE], np.array(LENS)[PAIR_PASSAGE], PAIR_QUERY)
    q = _queries(3, Lq, D, seed=Lq)
    n = len(PAIR_PASSAGE)
    cen, w = codec.centroids.cuda(), codec.bucket_weights.cuda()
    codes_d, res_d, mask_d = codes.cuda(), res.cuda(), mask.cuda()
    for Lc in (64, 70):
        for kind, bank_rows in (("fp16", plain), ("nbits1", decoded)):
            c, cm = torch.zeros(n, Lc, D), torch.zeros(n, Lc)
            for i, p in enumerate(PAIR_PASSAGE):
                c[i, :LENS[p]] = bank_rows[first[p]:first[p] + LENS[p]].float()
                cm[i, :LENS[p]] = mask[first[p]:first[p] + LENS[p]].float()
            qsel, cd, cmd = q[PAIR_QUERY].contiguous(), c.cuda(), cm.cuda()
            rs, rm = torch.full((n, Lc, Lq), POISON, device="cuda"), torch.full((n,), POISON, device="cuda")
            assert lib.rr_op_li_scores(L.ptr(qsel), L.ptr(cd), L.ptr(cmd), n, 1, Lq, Lc, D, L.ptr(rs), L.ptr(rm), st) == 0
            gs, gm = torch.full((n + 2, Lc, Lq), POISON, device="cuda"), torch.full((n + 2,), POISON, device="cuda")
            om = torch.full((n,), POISON, device="cuda")
            rows_d = bank_rows.cuda()
            src = (L.ptr(rows_d), L.ptr(mask_d), 0, None, None, None, None, 0) if kind == "fp16" else \
                (None, L.ptr(mask_d), 1, L.ptr(codes_d), L.ptr(res_d), L.ptr(cen), L.ptr(w), N_CENTROIDS)
            assert lib.rr_op_bank_li_scores(L.ptr(q), Lq, D, L.ptr(pairs), n, Lc, *src, L.ptr(gs), L.ptr(gm), st) == 0
            assert lib.rr_op_bank_li_scores(L.ptr(q), Lq, D, L.ptr(pairs), n, Lc, *src, None, L.ptr(om), st) == 0
            torch.cuda.synchronize()
            assert torch.equal(gs[:n], rs) and torch.equal(gm[:n], rm) and torch.equal(om, rm), f"{kind} Lc {Lc}"
            assert (gs[n:] == POISON).all() and (gm[n:] == POISON).all()
            if kind == "fp16":
                m64, s64 = li_scores_formula(qsel.cpu(), c, cm, 1, torch.float64)
                keep = cm.bool()
                d_s = (gs[:n].cpu().double() - s64)[keep].abs().max().item()
                d_m = (gm[:n].cpu().double() - m64).abs().max().item()
                b_s, b_m = (b * (1.0 + 2.0 ** -10) for b in _bounds(D, Lq))
                print(f"[D16_Lq{Lq}_Lc{Lc}] scores |d| {d_s:.3e} (bound {b_s:.3e}), maxsim |d| {d_m:.3e} (bound {b_m:.3e})")
                record_margin(f"bank_li_scores/D16_Lq{Lq}_Lc{Lc}", scores_max_abs=d_s, scores_bound=b_s, maxsim_max_abs=d_m,
                              maxsim_bound=b_m)
                assert d_s <= b_s and d_m <= b_m


# ---- 3. agreement with the forward ----------------------------------------------------------------------------------------------
def test_maxsim_equals_the_forwards_and_works_on_mores():
    eng, g = _engine("int_tiny")
    meng, _ = _engine("mores_tiny")
    D, Lc = int(eng.arch["li_dim"]), int(g["Lc"])
    assert int(meng.arch["li_dim"]) == D
    lens = [1, 7, 33, Lc, 12, 20]
    bank = _fp16_bank(eng, D, seed=31, lens=lens, full=None)
    q, qm = _two_queries(g)
    ids = _ids([2, 0, 2, 3, 2, 1])
    fwd = eng.forward_interaction_bank(bank, q, qm, ids, 2, 3, granule=8, padded_len=Lc, fusion_from_li=True,
                                       fusion_multiplier=5.0, want_maxsim=True)
    got = eng.bank_li_scores(bank, q, ids, K=3, padded_len=Lc)
    by_lists = eng.bank_li_scores(bank, q, ids, list_sizes=[3, 3])
    conv = bank.maxsim(eng, q, ids, K=3)
    mores = meng.bank_li_scores(bank, q, ids, K=3, padded_len=Lc, want_scores=True)   # the shared bank on a MORES handle
    full = eng.bank_li_scores(bank, q, ids, K=3, padded_len=Lc, want_scores=True)
    torch.cuda.synchronize()
    assert torch.equal(got["maxsim"], fwd["maxsim"])
    assert torch.equal(by_lists["maxsim"], got["maxsim"]) and torch.equal(conv, got["maxsim"])   # pad rows never win a maximum
    assert torch.equal(mores["maxsim"], got["maxsim"]) and torch.equal(mores["scores"], full["scores"])
    with pytest.raises(KeyError, match="'nope'"):
        eng.bank_li_scores(bank, q, ["p0", "nope"], K=1)


def test_retriever_scores_of_the_drop_in_class_on_a_mores_model():
    from test_gpu_passage_bank import _model
    m, g = _model("mores_tiny")
    D = g["query_li"].shape[2]
    with pytest.raises(RuntimeError):
        m.retriever_scores(torch.zeros(1, 4, D), ["p0"])
    m.bank = _fp16_bank(m.engine, D, seed=37)
    q = _queries(3, 9, D, seed=5)
    r = m.retriever_scores(q, _ids(PAIR_PASSAGE), pair_query=PAIR_QUERY, want_scores=True)
    ref = m.engine.bank_li_scores(m.bank, q, _ids(PAIR_PASSAGE), pair_query=PAIR_QUERY, want_scores=True)
    torch.cuda.synchronize()
    assert r["scores"].shape == (12, 64, 9) and torch.equal(r["scores"], ref["scores"]) and torch.equal(r["maxsim"], ref["maxsim"])


# ---- 4. output discipline / 6. refusals -----------------------------------------------------------------------------------------
def _raw(eng, bank, q, pp, pq, Lc, scores, maxsim, n_queries=None, n_pairs=None, Lq=None, handle=True, bank_h=True, q_ptr=None):
    from rmr_amd import _lib as L
    pp, pq = np.ascontiguousarray(pp, dtype=np.int32), np.ascontiguousarray(pq, dtype=np.int32)
    return eng.lib.rr_bank_li_scores(eng.h if handle else None, bank.h if bank_h else None, L.ptr(q) if q_ptr is None else q_ptr,
                                     q.shape[0] if n_queries is None else n_queries, q.shape[1] if Lq is None else Lq,
                                     pp.ctypes.data, pq.ctypes.data, len(pp) if n_pairs is None else n_pairs, Lc, L.ptr(scores),
                                     L.ptr(maxsim), torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("kind", ["fp16", "nbits8"])
def test_only_the_calls_rows_are_written(kind):
    D, Lq, Lc, n = 64, 17, 70, len(PAIR_PASSAGE)
    eng = _bare_engine(D)
    bank = _fp16_bank(eng, D, seed=41) if kind == "fp16" else _plaid_bank(eng, D, 8, seed=41)
    q = _queries(3, Lq, D, seed=43)
    ps = torch.full((n + 3, Lc, Lq), POISON, device="cuda")
    pm = torch.full((n + 3,), POISON, device="cuda")
    assert _raw(eng, bank, q, PAIR_PASSAGE, PAIR_QUERY, Lc, ps, pm) == 0
    want = eng.bank_li_scores(bank, q, _ids(PAIR_PASSAGE), pair_query=PAIR_QUERY, padded_len=Lc, want_scores=True)
    torch.cuda.synchronize()
    assert torch.equal(ps[:n], want["scores"]) and torch.equal(pm[:n], want["maxsim"])
    assert (ps[n:] == POISON).all() and (pm[n:] == POISON).all()
    for i, p in enumerate(PAIR_PASSAGE):
        assert (ps[i, LENS[p]:] == MASKED).all()
        if p == FULLY_MASKED:
            assert (ps[i] == MASKED).all() and pm[i].item() == MASKED * Lq


def test_refusals_write_nothing():
    from rmr_amd import _lib as L
    D, Lq, Lc, n = 64, 9, 64, len(PAIR_PASSAGE)
    eng, other, full = _bare_engine(D), _bare_engine(128), _bare_engine(D, "full_context")
    bank, plaid = _fp16_bank(eng, D, seed=51), _plaid_bank(eng, D, 4, seed=51)
    q = _queries(3, Lq, D, seed=53)
    ps = torch.full((n, Lc, Lq), POISON, device="cuda")
    pm = torch.full((n,), POISON, device="cuda")
    pp, pq = PAIR_PASSAGE, PAIR_QUERY
    for b in (bank, plaid):
        assert _raw(eng, b, q, pp, pq, Lc, None, None) == L.RR_ERR_BAD_ARG                      # no output at all
        assert b"both null" in eng.lib.rr_last_error(eng.h)
        assert _raw(eng, b, q, pp, pq, Lc, ps, pm, handle=False) == L.RR_ERR_BAD_ARG
        assert _raw(eng, b, q, pp, pq, Lc, ps, pm, bank_h=False) == L.RR_ERR_BAD_ARG
        assert _raw(eng, b, q, pp, pq, Lc, ps, pm, q_ptr=0) == L.RR_ERR_BAD_ARG
        assert _raw(eng, b, q, pp, pq, Lc, ps, pm, q_ptr=L.ptr(q) + 4) == L.RR_ERR_BAD_ARG      # alignment
        st = torch.cuda.current_stream().cuda_stream
        one = np.zeros(1, dtype=np.int32)
        assert eng.lib.rr_bank_li_scores(eng.h, b.h, L.ptr(q), 3, Lq, None, one.ctypes.data, 1, Lc, L.ptr(ps), L.ptr(pm), st) == L.RR_ERR_BAD_ARG
        assert eng.lib.rr_bank_li_scores(eng.h, b.h, L.ptr(q), 3, Lq, one.ctypes.data, None, 1, Lc, L.ptr(ps), L.ptr(pm), st) == L.RR_ERR_BAD_ARG
        assert _raw(full, b, q, pp, pq, Lc, ps, pm) == L.RR_ERR_BAD_ARG                         # not an interaction handle
        assert _raw(other, b, q, pp, pq, Lc, ps, pm) == L.RR_ERR_BAD_SHAPE                      # another li_dim
        assert b"li_dim" in other.lib.rr_last_error(other.h)
        for kw in (dict(n_queries=0), dict(Lq=0), dict(n_pairs=0), dict(n_pairs=-1)):
            assert _raw(eng, b, q, pp, pq, Lc, ps, pm, **kw) == L.RR_ERR_BAD_SHAPE
        assert _raw(eng, b, q, pp, pq, 0, ps, pm) == L.RR_ERR_BAD_SHAPE
        assert _raw(eng, b, q, pp[:-1] + [len(LENS)], pq, Lc, ps, pm) == L.RR_ERR_BAD_SHAPE     # a passage index outside the bank
        assert _raw(eng, b, q, [-1] + pp[1:], pq, Lc, ps, pm) == L.RR_ERR_BAD_SHAPE
        assert _raw(eng, b, q, pp, pq[:-1] + [3], Lc, ps, pm) == L.RR_ERR_BAD_SHAPE             # a query index outside n_queries
        assert _raw(eng, b, q, pp, [-1] + pq[1:], Lc, ps, pm) == L.RR_ERR_BAD_SHAPE
        assert _raw(eng, b, q, pp, pq, 63, ps, pm) == L.RR_ERR_BAD_SHAPE                        # passage 5 holds 64 rows
        assert b"64 rows" in eng.lib.rr_last_error(eng.h)
    torch.cuda.synchronize()
    assert (ps == POISON).all() and (pm == POISON).all()
    with pytest.raises(ValueError):
        eng.bank_li_scores(bank, q, _ids(pp), pair_query=pq, want_scores=False, want_maxsim=False)
    with pytest.raises(KeyError, match="'p6'"):
        eng.bank_li_scores(bank, q, _ids(pp[:-1]) + ["p6"], pair_query=pq)
    with pytest.raises(AssertionError):
        other.bank_li_scores(bank, _queries(3, Lq, 128, seed=1), _ids(pp), pair_query=pq)       # RR_ERR_BAD_SHAPE
    with pytest.raises(ValueError):
        full.bank_li_scores(bank, q, _ids(pp), pair_query=pq)                                   # RR_ERR_BAD_ARG
    with pytest.raises(AssertionError):
        eng.bank_li_scores(bank, q, _ids(pp), pair_query=pq, padded_len=63)
    with pytest.raises(AssertionError):
        eng.bank_li_scores(bank, q, _ids(pp))                                                   # three queries: which one?
    assert _raw(eng, bank, q, pp, pq, Lc, ps, pm) == 0                                          # and what is right is taken
    torch.cuda.synchronize()
    assert not (ps == POISON).any() and not (pm == POISON).any()


@pytest.mark.parametrize("kind", ["fp16", "nbits4"])
def test_a_capturing_stream_is_refused_and_nothing_is_written(kind):
    """The call stages its descriptors from the host: under stream capture it returns RR_ERR_BAD_ARG, records nothing into the graph
    and writes nothing; the same call outside the capture is taken."""
    from rmr_amd import _lib as L
    D, Lq, Lc, n = 64, 9, 64, len(PAIR_PASSAGE)
    eng = _bare_engine(D)
    bank = _fp16_bank(eng, D, seed=55) if kind == "fp16" else _plaid_bank(eng, D, 4, seed=55)
    q = _queries(3, Lq, D, seed=57)
    ps = torch.full((n, Lc, Lq), POISON, device="cuda")
    pm = torch.full((n,), POISON, device="cuda")
    probe = torch.zeros(1, device="cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        assert _raw(eng, bank, q, PAIR_PASSAGE, PAIR_QUERY, Lc, ps, pm) == 0          # warm-up on the capture stream
        torch.cuda.synchronize()
        ps.fill_(POISON)
        pm.fill_(POISON)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            probe.add_(1.0)                                                            # the graph holds this node alone
            rc = _raw(eng, bank, q, PAIR_PASSAGE, PAIR_QUERY, Lc, ps, pm)
            msg = eng.lib.rr_last_error(eng.h)
        graph.replay()
        torch.cuda.synchronize()
    assert rc == L.RR_ERR_BAD_ARG and b"captured" in msg
    assert probe.item() == 1.0 and (ps == POISON).all() and (pm == POISON).all()
    assert _raw(eng, bank, q, PAIR_PASSAGE, PAIR_QUERY, Lc, ps, pm) == 0
    torch.cuda.synchronize()
    assert not (pm == POISON).any()


# ---- 5. non-finite rows -----------------------------------------------------------------------------------------------------------
def test_non_finite_rows():
    D, Lq = 64, 9
    eng = _bare_engine(D)
    lens = [8, 8, 8, 8, 8, 8]
    gen = torch.Generator().manual_seed(7)

    def bank_of(li):
        cm = torch.ones(6, 8)
        cm[1, 5], cm[2, 6] = 0, 0
        b = eng.create_bank(48, 6)
        b.add(_ids(range(6)), li, cm, lengths=lens)
        return b
    li = torch.nn.functional.normalize(torch.randn(6, 8, D, generator=gen), dim=-1)
    li[1, 5] = float("nan")                                # under a mask hole
    li[2, 6, 3] = float("inf")                             # under a mask hole
    clean = bank_of(li)
    li[3, 2, 1] = float("nan")                             # an unmasked NaN in passage 3
    dirty = bank_of(li)
    q = _queries(2, Lq, D, seed=9)
    ids, pq = _ids([0, 1, 2, 3, 4, 5, 3]), [0, 1, 0, 1, 0, 1, 0]
    r = eng.bank_li_scores(dirty, q, ids, pair_query=pq, want_scores=True)
    only = eng.bank_li_scores(dirty, q, ids, pair_query=pq)
    ok = eng.bank_li_scores(clean, q, ids, pair_query=pq, want_scores=True)
    torch.cuda.synchronize()
    sc, ms = r["scores"].cpu(), r["maxsim"].cpu()
    assert (sc[1, 5] == MASKED).all() and (sc[2, 6] == MASKED).all()
    assert torch.isnan(sc[3, 2]).all() and torch.isnan(sc[6, 2]).all()
    others = torch.ones(7, 8, dtype=torch.bool)
    others[3, 2], others[6, 2] = False, False
    assert torch.isfinite(sc[others]).all(), "a NaN row must not leak into other rows"
    fine = [0, 1, 2, 4, 5]
    assert torch.isnan(ms[[3, 6]]).all() and torch.isnan(only["maxsim"].cpu()[[3, 6]]).all()
    assert torch.equal(ms[fine], ok["maxsim"].cpu()[fine]) and torch.equal(only["maxsim"].cpu()[fine], ms[fine])
    assert torch.equal(sc[fine], ok["scores"].cpu()[fine]) and bool(torch.isfinite(ok["maxsim"]).all())


# ---- 7. profile -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fp16", "nbits8"])
def test_profile_books_one_tail_launch_with_the_flops_of_the_rows_that_exist(kind):
    D, Lq, Lc = 128, 113, 70
    eng = _bare_engine(D)
    bank = _fp16_bank(eng, D, seed=61) if kind == "fp16" else _plaid_bank(eng, D, 8, seed=61)
    q = _queries(3, Lq, D, seed=63)
    eng.set_profiling(True)
    try:
        eng.get_profile(reset=True)
        eng.bank_li_scores(bank, q, _ids(PAIR_PASSAGE), pair_query=PAIR_QUERY, padded_len=Lc, want_scores=True)
        p = eng.get_profile(reset=True)
    finally:
        eng.set_profiling(False)
    rows = sum(LENS[i] for i in PAIR_PASSAGE)
    assert p["tail"]["launches"] == 1 and p["tail"]["flops"] == 2.0 * rows * Lq * D and p["tail"]["ms"] > 0
    assert sum(v["launches"] for v in p.values()) == 1


# ---- 8. past 4 GiB ----------------------------------------------------------------------------------------------------------------
def test_scored_passages_past_4_gib_of_bank_rows():
    """17 000 zero passages of 1 024 rows of 128 fp16 values fill 4.46 GB: the passages added behind them lie beyond byte 2^32 of the
    bank.  Their scores equal those of the same passages in a small bank; a row offset cut to 32 bits would read zero rows."""
    from test_gpu_large_index import _need
    D, Lq = 128, 33
    eng = _bare_engine(D)
    n0, L0 = 17000, 1024
    big = n0 * L0 * D * 2
    _need(2 * big + n0 * L0 * 5 + (1 << 28))
    small = _fp16_bank(eng, D, seed=71)
    q = _queries(3, Lq, D, seed=73)
    want = eng.bank_li_scores(small, q, _ids(PAIR_PASSAGE), pair_query=PAIR_QUERY, padded_len=70, want_scores=True)
    bank = eng.create_bank(n0 * L0 + sum(LENS), n0 + len(LENS))
    zeros = torch.zeros([n0, L0, D], dtype=torch.float16, device="cuda")
    bank.add(range(n0), zeros, torch.ones(n0, L0, device="cuda"), lengths=[L0] * n0)
    del zeros
    li, cm = torch.zeros(len(LENS), 64, D, dtype=torch.float16), torch.zeros(len(LENS), 64)
    for i, ln in enumerate(LENS):
        rows, mask = small.read(f"p{i}")
        li[i, :ln], cm[i, :ln] = rows, mask.float()
    assert bank.add(_ids(range(len(LENS))), li, cm, lengths=LENS) == n0 and bank.info()["rows_used"] * D * 2 > 1 << 32
    assert bank.lookup(["p0"])[0][0] == n0 and n0 * L0 * D * 2 > 1 << 32
    got = eng.bank_li_scores(bank, q, _ids(PAIR_PASSAGE), pair_query=PAIR_QUERY, padded_len=70, want_scores=True)
    torch.cuda.synchronize()
    assert bool((want["maxsim"] != 0).all())
    assert torch.equal(got["scores"], want["scores"]) and torch.equal(got["maxsim"], want["maxsim"])
    bank.close()
    torch.cuda.empty_cache()
