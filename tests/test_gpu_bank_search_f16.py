"""GPU: the exhaustive bank search whose first pass runs on the fp16 matrix core (rr_bank_search_f16 / RerankEngine.bank_search_f16,
PassageBank.search(fast=), rr_op_bank_scores_f16; include/rerank_mi355.h, csrc/bank_search_f16.hip).

Fixtures and the definition in numpy: tests/bank_f16_cases.py.  Four grounds.
EXACT INPUTS (multiples of 2^-3 in [-2, 2]: every partial sum exact in float32, the query exact in fp16): the approximate pass must
give the exact search's dense scores bit for bit, whatever the matrix core's order, the call must return rr_bank_search's bytes, and
at slack 0 the certificate must be the numpy condition (k = ndocs < n ties score_k with a*: not certified, and that is the point).
RANDOM UNIT ROWS: every returned score is rr_bank_li_scores' maxsim of its pair, a certified row is rr_bank_search's row, every query
is certified at the default slack (tests/test_bank_f16_cpu.py shows in float64 that the fixture leaves twice the slack), and three
runs give the same bytes.
ADVERSARIAL: one nonzero product per score; the exact winner is invisible to the fp16 query and must not be certified away.
THE MEASURED BOUND: max |A - float64(A)| / (sum_j ||fp16(q_j)|| max ||x||) on the random fixtures against the header's D 2^-22.
Measured on an MI355X (profiles/bank_f16_parity_margins.json): at most 2.3e-07, 1.5e-02 of D 2^-22 at D 64 and 6.4e-03 of it at D 128: far
below the quarter of the constant at which the header asks for a larger one.  Refused calls write nothing.
"""
import numpy as np
import pytest
import torch

import bank_f16_cases as C
from helpers import record_margin
from test_gpu_bank_search import IPOISON, POISON, _table_dev
from test_gpu_li_scores import _engine
from test_gpu_plaid_bank import _codec, _rows

pytestmark = pytest.mark.gpu

NDOCS, K = 64, 16
_BANKS = {}


def _centroids(D):
    gen = torch.Generator().manual_seed(D)
    return torch.nn.functional.normalize(torch.randn(33, D, generator=gen), dim=-1).half()


def _bank(eng, fx, coded=False):
    """the fixture's passages in a bank of `eng`, added in two adds; `coded`: an fp16 bank with a centroid table"""
    P, half = len(fx["lens"]), len(fx["lens"]) // 2
    bank = eng.create_bank(int(np.sum(fx["lens"])) + 8, P + 4, **(dict(centroids=_centroids(fx["D"])) if coded else {}))
    for lo, hi in ((0, half), (half, P)):
        li, cm, lens = C.padded(fx, lo, hi)
        bank.add([f"p{i}" for i in range(lo, hi)], torch.from_numpy(li), torch.from_numpy(cm), lengths=lens)
    return bank


def _case(name, make):
    """(fixture, engine, plain bank, coded bank, q on the device), built once per name"""
    if name not in _BANKS:
        fx = make()
        eng = _engine(fx["D"])
        plain = _bank(eng, fx)
        rows, mask = plain.read("p1")                                      # the bank holds the fixture's rows as they are
        a = C.first_rows(fx["lens"])[1]
        assert np.array_equal(rows.float().cpu().numpy(), fx["rows"][a:a + fx["lens"][1]])
        _BANKS[name] = (fx, eng, plain, _bank(eng, fx, coded=True), torch.from_numpy(fx["q"]).cuda())
    return _BANKS[name]


def _dense_exact(eng, bank, q, first, n, li=False):
    """float32 [nq, n]: rr_bank_search's score of every passage of the range (k = n up to 1024 passages; beyond, rr_bank_li_scores'
    maxsim, which rr_bank_search's score is bit for bit; `li`: that one at any size)"""
    nq = q.shape[0]
    if n <= 1024 and not li:
        r = eng.bank_search(bank, q, n, first=first, count=n)
        out = torch.empty((nq, n), device="cuda")
        out.scatter_(1, (r["indices"] - first).long(), r["scores"])
        return out
    ids = [f"p{i}" for i in range(first, first + n)] * nq
    return eng.bank_li_scores(bank, q, ids, pair_query=np.repeat(np.arange(nq), n))["maxsim"].reshape(nq, n)


def _op_scores(fx, q, first=0, n=None):
    """A [nq, n] from rr_op_bank_scores_f16 over the fixture's rows as raw device arrays"""
    from rmr_amd import _lib as L
    lib = L.load()
    n = len(fx["lens"]) - first if n is None else n
    rows = torch.from_numpy(fx["rows"]).half().cuda()
    mask, table = torch.from_numpy(fx["mask"]).cuda(), _table_dev(fx["lens"])
    out = torch.full((q.shape[0] + 1, n), POISON, device="cuda")
    rc = lib.rr_op_bank_scores_f16(L.ptr(q), q.shape[0], q.shape[1], fx["D"], L.ptr(table), first, n, L.ptr(rows), L.ptr(mask), L.ptr(out),
                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert (out[q.shape[0]:] == POISON).all()
    return out[:q.shape[0]]


def _same_bytes(a, b, tag):
    for key in ("indices", "scores", "certified"):
        assert torch.equal(a[key], b[key]), f"{tag}: {key} differ"


EXACT_CASES = [("mixed", 128, 17, 32), ("mixed", 64, 3, 5), ("mixed", 128, 1, 5), ("mixed", 64, 3, 32), ("short", 64, 3, 5), ("short", 128, 1, 32)]


@pytest.mark.parametrize("kind,D,nq,Lq", EXACT_CASES)
def test_exact_inputs_give_the_exact_search_bit_for_bit(kind, D, nq, Lq):
    fx, eng, plain, coded, q = _case(("exact", kind, D, nq, Lq), lambda: C.exact_fixture(kind, D, nq, Lq, seed=D + Lq + nq))
    P = len(fx["lens"])
    ranges = [(0, P), (37, P - 137)] + ([(P - 200, 200)] if kind == "short" else [])
    for first, n in ranges:
        E = _dense_exact(eng, plain, q, first, n)
        A = _op_scores(fx, q, first, n)
        assert torch.equal(A, E), f"A differs from the exact scores at {(A != E).nonzero()[:3].tolist()} (range {first}, {n})"
        assert np.array_equal(E.cpu().numpy().astype(np.float64), C.exact64(fx, first=first, count=n))       # ... which are exact
        E_np = E.cpu().numpy()
        for ndocs, k in ((NDOCS, K), (NDOCS, NDOCS), (1024, K)):
            got = eng.bank_search_f16(plain, q, k, ndocs, slack=0.0, first=first, count=n)
            want = eng.bank_search(plain, q, k, first=first, count=n)
            torch.cuda.synchronize()
            tag = f"{kind} D {D} range ({first}, {n}) ndocs {ndocs} k {k}"
            assert torch.equal(got["indices"], want["indices"]) and torch.equal(got["scores"], want["scores"]), tag
            idx, sc, cert = C.search_f16(E_np, E_np, ndocs, k, 0.0, first)
            assert np.array_equal(got["indices"].cpu().numpy(), idx) and np.array_equal(got["scores"].cpu().numpy(), sc), tag
            assert got["certified"].cpu().tolist() == cert.tolist(), tag
            if ndocs >= n:
                assert cert.all(), tag
            elif k == ndocs:
                assert not cert.any(), tag                                 # score_k is a*: never strictly above it
            _same_bytes(eng.bank_search_f16(coded, q, k, ndocs, slack=0.0, first=first, count=n), got, tag + " coded")


RANDOM_CASES = [(128, 17, 32), (64, 3, 5), (128, 1, 5), (64, 17, 32)]


@pytest.mark.parametrize("D,nq,Lq", RANDOM_CASES)
def test_random_unit_rows_exact_scores_certificates_and_the_measured_bound(D, nq, Lq):
    fx, eng, plain, coded, q = _case(("random", D, nq, Lq), lambda: C.random_fixture(D, nq, Lq, seed=D + Lq))
    P = len(fx["lens"])
    E = _dense_exact(eng, plain, q, 0, P, li=True)                         # rr_bank_li_scores' maxsim of every pair
    want = eng.bank_search(plain, q, K)
    runs = [eng.bank_search_f16(plain, q, K, NDOCS) for _ in range(3)]
    torch.cuda.synchronize()
    got = runs[0]
    assert torch.equal(got["scores"], E.gather(1, got["indices"].long())), "a returned score is not its pair's exact score"
    cert = got["certified"].bool()
    assert torch.equal(got["indices"][cert], want["indices"][cert]) and torch.equal(got["scores"][cert], want["scores"][cert])
    assert cert.all(), f"queries {(~cert).nonzero().flatten().tolist()} are not certified at the default slack"
    for r in runs[1:]:
        _same_bytes(r, got, "run to run")
    _same_bytes(eng.bank_search_f16(coded, q, K, NDOCS), got, "coded")
    from rmr_amd import F16Search
    _same_bytes(plain.search(eng, q, K, fast=F16Search(NDOCS)), got, "PassageBank.search")
    part = eng.bank_search_f16(plain, q, K, NDOCS, first=16, count=P - 48)
    assert torch.equal(part["scores"], E.gather(1, part["indices"].long())) and int(part["indices"].min()) >= 16
    # the measured bound of the approximate pass
    A = _op_scores(fx, q).cpu().numpy().astype(np.float64)
    A64 = C.approx64(fx)
    qn = np.linalg.norm(C.fp16_rne(fx["q"]).astype(np.float64), axis=-1).sum(axis=-1)           # [nq]
    xmax = np.linalg.norm(fx["rows"].astype(np.float64), axis=-1).max()
    real = np.abs(A64) < 9000.0                                            # (the fully masked passage: Lq * -9999 on both sides)
    assert np.array_equal(A[~real], A64[~real])
    measured = float((np.abs(A - A64) / (qn[:, None] * xmax))[real].max())
    const = D * 2.0 ** -22
    print(f"bank_f16 measured bound D {D} nq {nq} Lq {Lq}: {measured:.3e} = {measured / const:.3e} of D 2^-22 = {const:.3e}")
    record_margin(f"bank_f16/accumulation/D{D}_nq{nq}_Lq{Lq}", measured=measured, constant=const, measured_over_constant=measured / const)
    assert measured <= const
    assert np.abs(A - E.cpu().numpy().astype(np.float64))[real].max() <= C.default_slack(fx["q"], D)     # the whole slack holds here


@pytest.mark.parametrize("D", [64, 128])
def test_adversarial_winner_is_not_certified_away(D):
    fx, eng, plain, coded, q = _case(("adversarial", D), lambda: C.adversarial_fixture(D, NDOCS))
    n = len(fx["lens"])
    want = eng.bank_search(plain, q, K)
    assert int(want["indices"][0, 0]) == n - 1 and float(want["scores"][0, 0]) == 1.0 + 2.0 ** -12
    assert (_op_scores(fx, q) == 1.0).all()
    for slack in (0.0, None):
        got = eng.bank_search_f16(plain, q, K, NDOCS, slack=slack)
        torch.cuda.synchronize()
        assert got["indices"][0].tolist() == list(range(K)), "ties in A go by bank index: the e1 passage is no survivor"
        assert (got["scores"] == np.float32(1.0 - 2.0 ** -13)).all() and got["certified"].tolist() == [0]
    whole = eng.bank_search_f16(plain, q, K, 1024, slack=0.0)              # every passage rescored: the exact result, certified
    assert torch.equal(whole["indices"], want["indices"]) and torch.equal(whole["scores"], want["scores"]) and whole["certified"].tolist() == [1]


def _raw(eng, bank, q, first, n, ndocs, k, slack, out, cert=True, stream=None):
    from rmr_amd import _lib as L
    return eng.lib.rr_bank_search_f16(eng.h, bank.h, L.ptr(q), q.shape[0], q.shape[1], first, n, ndocs, k, slack, L.ptr(out[0]), L.ptr(out[1]),
                                      L.ptr(out[2]) if cert else None, torch.cuda.current_stream().cuda_stream if stream is None else stream)


def _poisoned(nq, k):
    return (torch.full((nq, k), IPOISON, device="cuda", dtype=torch.int32), torch.full((nq, k), POISON, device="cuda"),
            torch.full((nq,), IPOISON, device="cuda", dtype=torch.int32))


def _untouched(out):
    torch.cuda.synchronize()
    return bool((out[0] == IPOISON).all() and (out[1] == POISON).all() and (out[2] == IPOISON).all())


def test_refusals_write_nothing():
    from rmr_amd import _lib as L
    D = 64
    fx, eng, plain, coded, q = _case(("random", D, 3, 5), lambda: C.random_fixture(D, 3, 5, seed=D + 5))
    P = len(fx["lens"])
    out = _poisoned(3, 1025)
    codec = _codec(D, 4)
    comp = eng.create_bank(64, 8, codec=codec)
    codes, res = _rows(codec, 12, seed=3)
    comp.add_compressed(["a", "b", "c", "d"], codes, res, [5, 1, 4, 2])
    assert _raw(eng, comp, q, 0, -1, 4, 2, 0.0, out) == L.RR_ERR_UNSUPPORTED and b"compressed" in eng.lib.rr_last_error(eng.h)
    for bank in (plain, coded):
        assert _raw(eng, bank, q, 0, -1, 8, 9, 0.0, out) == L.RR_ERR_BAD_SHAPE                # k > ndocs
        assert _raw(eng, bank, q, 0, -1, 8, 0, 0.0, out) == L.RR_ERR_BAD_SHAPE
        assert _raw(eng, bank, q, 0, 4, 8, 5, 0.0, out) == L.RR_ERR_BAD_SHAPE                 # k > n_passages
        assert _raw(eng, bank, q, 0, -1, 1025, 4, 0.0, out) == L.RR_ERR_UNSUPPORTED           # ndocs > 1024
        assert _raw(eng, bank, q, 0, -1, 8, 4, float("nan"), out) == L.RR_ERR_BAD_ARG
        assert _raw(eng, bank, q, 0, -1, 8, 4, -1e-6, out) == L.RR_ERR_BAD_ARG
        assert _raw(eng, bank, q, 0, -1, 8, 4, 0.0, out, cert=False) == L.RR_ERR_BAD_ARG      # certified_out is required
        assert _raw(eng, bank, q, 1, P, 8, 4, 0.0, out) == L.RR_ERR_BAD_SHAPE                 # rr_bank_search's range check stands
    assert _untouched(out)
    with pytest.raises(NotImplementedError):
        eng.bank_search_f16(comp, q, 2, 4)
    with pytest.raises(ValueError):
        eng.bank_search_f16(plain, q, 9, 8)
    out = _poisoned(3, 4)
    assert _raw(eng, plain, q, 0, -1, 8, 4, 0.0, out) == 0                                    # the same arguments, accepted
    torch.cuda.synchronize()
    assert not (out[0] == IPOISON).any() and not (out[1] == POISON).any() and not (out[2] == IPOISON).any()


def test_a_capturing_stream_is_refused_and_nothing_is_written():
    from rmr_amd import _lib as L
    D = 64
    fx, eng, plain, coded, q = _case(("random", D, 3, 5), lambda: C.random_fixture(D, 3, 5, seed=D + 5))
    out = _poisoned(3, 4)
    probe = torch.zeros(1, device="cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        assert _raw(eng, plain, q, 0, -1, 8, 4, 0.0, out, stream=st.cuda_stream) == 0          # the table and the block exist
        torch.cuda.synchronize()
        for t in out:
            t.fill_(IPOISON if t.dtype == torch.int32 else POISON)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            probe.add_(1.0)                                                # the graph holds this node alone
            rc = _raw(eng, plain, q, 0, -1, 8, 4, 0.0, out, stream=st.cuda_stream)
            msg = eng.lib.rr_last_error(eng.h)
        graph.replay()
    torch.cuda.synchronize()
    assert rc == L.RR_ERR_BAD_ARG and b"captured" in msg
    assert probe.item() == 1.0 and _untouched(out)


def test_parts_and_several_banks_carry_the_certificate():
    """search_bank_part / search_banks with fast=: two banks holding the halves of the random fixture give the one bank's exact
    result, and the merged certificate is the AND of the parts'."""
    from rmr_amd import F16Search, search_bank_part, search_banks
    D, nq, Lq = 64, 3, 5
    fx, eng, plain, coded, q = _case(("random", D, nq, Lq), lambda: C.random_fixture(D, nq, Lq, seed=D + Lq))
    P, half = len(fx["lens"]), len(fx["lens"]) // 2
    banks = []
    for lo, hi in ((0, half), (half, P)):
        b = eng.create_bank(int(np.sum(fx["lens"][lo:hi])) + 8, hi - lo + 4)
        li, cm, lens = C.padded(fx, lo, hi)
        b.add([f"p{i}" for i in range(lo, hi)], torch.from_numpy(li), torch.from_numpy(cm), lengths=lens)
        banks.append(b)
    fast = F16Search(NDOCS)
    parts = [search_bank_part(eng, b, q, K, fast=fast) for b in banks]
    assert all(set(p) == {"indices", "scores", "counts", "certified"} and p["counts"].tolist() == [K] * nq for p in parts)
    ids, scores, counts, cert = search_banks(eng, banks, q, K, fast=fast)
    want_ids, want_scores = plain.search(eng, q, K)
    assert torch.equal(cert, torch.minimum(parts[0]["certified"], parts[1]["certified"])) and cert.tolist() == [1] * nq
    assert ids == want_ids and torch.equal(scores, want_scores) and counts.tolist() == [K] * nq
