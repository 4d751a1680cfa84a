"""GPU: the first pass of the fp16 matrix-core searches (bank_scores_f16_kernel, bank_scores_f16_plaid_kernel) at EVERY LAUNCH FORM,
against float64 numpy, and the default slack on queries outside fp16's range.

bank_f16_cases.FORM_SHAPES reaches all ten (NT, TP) instantiations, one, two and three or more passes over the query (psum, col_lim
and the padded tiles of a last pass) at every cap of the query block (D 64 .. 1024), and tests/test_bank_f16_forms_cpu.py asserts
that from the launcher's own host function.  The passages: the "mixed" kind (300 of 1 .. 40 rows) and the "long" kind (71 of 1 ..
257 rows: the kernel's two-tile row loop runs up to eight times, lengths end on, before and behind a tile; masks on both sides
of tile and step edges; a partial last chunk).
1. EXACT INPUTS: rr_op_bank_scores_f16 == float64 numpy, bit for bit.  The reference shares nothing with either kernel.
2. RANDOM UNIT ROWS over the long passages: the measured accumulation error against the header's D 2^-22, recorded
   (profiles/bank_f16_parity_margins.json, bank_f16/accumulation/long_*), first measurements at D 256 .. 1024 and 257-row passages.
   Measured on an MI355X: at most 3.4e-07; 2.3e-02 of the constant at worst (D 64, Lq 257), 1.0e-02 at D 128, 4.5e-03 at D 256,
   2.5e-03 at D 512, 9.2e-04 at D 1024: far below the quarter of the constant at which the header asks for a larger one.
3. THE PLAID KERNEL at the same forms over the long lengths: equal to the fp16 kernel over the decoded rows (torch.equal).  With 1
   the twin is itself verified there, so a mistake in the design the two kernels share no longer passes.
4. END TO END through an engine on the long exact fixture: rr_bank_search's bytes, the numpy certificate; coded and compressed banks.
5. OUT-OF-RANGE QUERIES: a query that is infinite or zero in fp16 is not certified at the default slack while the exact winner is
   missing; with every passage rescored it is rr_bank_search's result, certified.  A NaN query is refused, nothing written.
"""
import ctypes

import numpy as np
import pytest
import torch

import bank_f16_cases as C
from helpers import record_margin
from test_gpu_bank_search_f16 import _bank, _op_scores, _poisoned, _raw, _same_bytes, _untouched
from test_gpu_bank_search_f16_plaid import _op_pair, _queries
from test_gpu_bank_search_f16_plaid import _raw as _raw_plaid
from test_gpu_li_scores import _engine
from test_gpu_plaid_bank import _codec, _fp16_twin, _rows

pytestmark = pytest.mark.gpu

NDOCS, K = 64, 16
SUBRANGE = {"mixed": (37, 163), "long": (5, 53)}                          # (first, n): no end on a chunk of 32 passages
_EXACT, _CODED = {}, {}


def _form(nq, Lq, D, plaid=False):
    from rmr_amd import _lib as L
    out = [ctypes.c_int(-7) for _ in range(3)]
    assert L.load().rr_op_bank_scores_f16_form(nq, Lq, D, int(plaid), *[ctypes.byref(o) for o in out]) == 0
    return tuple(o.value for o in out)


def _exact(kind, D, nq, Lq):
    """(fixture, its exact scores in float64 numpy cast to float32, the query on the device), computed once"""
    key = (kind, D, nq, Lq)
    if key not in _EXACT:
        fx = C.exact_fixture(kind, D, nq, Lq, seed=D + Lq + nq)
        E64 = C.exact64(fx)
        E = E64.astype(np.float32)
        assert np.array_equal(E.astype(np.float64), E64), "the fixture's scores are exact in float32"
        _EXACT[key] = (fx, E, torch.from_numpy(fx["q"]).cuda())
    return _EXACT[key]


@pytest.mark.parametrize("kind", ["mixed", "long"])
@pytest.mark.parametrize("D,nq,Lq", C.FORM_SHAPES)
def test_exact_inputs_give_float64_bit_for_bit_at_every_form(D, nq, Lq, kind):
    fx, E, q = _exact(kind, D, nq, Lq)
    P = len(fx["lens"])
    first, n = SUBRANGE[kind]
    assert first % 32 and (first + n) % 32 and first + n < P
    for a, cnt in ((0, P), (first, n)):
        A = _op_scores(fx, q, a, cnt).cpu().numpy()                       # (checks the row of poison behind the output)
        want = E[:, a:a + cnt]
        bad = np.argwhere(A != want)
        assert np.array_equal(A, want), (f"form {_form(nq, Lq, D)} range ({a}, {cnt}): {len(bad)} of {A.size} differ, first (query, passage) "
                                         f"{bad[:4].tolist()}: {[float(A[i, j]) for i, j in bad[:4]]} for {[float(want[i, j]) for i, j in bad[:4]]}, "
                                         f"lengths {[fx['lens'][a + j] for i, j in bad[:4]]}")


# one shape per (cap of the block, passes): (D, n_queries, Lq, cap, passes)
ACCUMULATION_CASES = [(64, 3, 49, 8, 1), (128, 3, 130, 8, 2), (64, 1, 257, 8, 3), (256, 1, 64, 4, 1), (256, 2, 65, 4, 2), (256, 1, 200, 4, 4),
                      (512, 1, 32, 2, 1), (512, 2, 33, 2, 2), (512, 1, 100, 2, 4), (1024, 1, 16, 1, 1), (1024, 2, 17, 1, 2), (1024, 1, 40, 1, 3)]


@pytest.mark.parametrize("D,nq,Lq,cap,passes", ACCUMULATION_CASES)
def test_random_unit_rows_over_long_passages_stay_under_the_accumulation_constant(D, nq, Lq, cap, passes):
    assert (D, nq, Lq) in C.FORM_SHAPES and _form(64, 4096, D)[0] == cap and _form(nq, Lq, D)[2] == passes
    fx = C.random_fixture_long(D, nq, Lq, seed=D + Lq)
    A = _op_scores(fx, torch.from_numpy(fx["q"]).cuda()).cpu().numpy().astype(np.float64)
    A64, E64 = C.approx64(fx), C.exact64(fx)
    qn = np.linalg.norm(C.fp16_rne(fx["q"]).astype(np.float64), axis=-1).sum(axis=-1)           # [nq]
    xmax = np.linalg.norm(fx["rows"].astype(np.float64), axis=-1).max()
    real = np.abs(A64) < 9000.0                                            # (the fully masked passage: Lq * -9999 on both sides)
    assert (~real).sum() == nq and np.array_equal(A[~real], A64[~real])
    measured = float((np.abs(A - A64) / (qn[:, None] * xmax))[real].max())
    const = D * 2.0 ** -22
    print(f"bank_f16 measured bound, long passages, D {D} nq {nq} Lq {Lq} (cap {cap}, {passes} passes): {measured:.3e} = "
          f"{measured / const:.3e} of D 2^-22 = {const:.3e}")
    record_margin(f"bank_f16/accumulation/long_D{D}_nq{nq}_Lq{Lq}", measured=measured, constant=const, measured_over_constant=measured / const)
    assert measured <= const
    assert np.abs(A - E64)[real].max() <= C.default_slack(fx["q"], D)     # the whole slack holds here


def _coded(D, nbits):
    """random codes and residual bytes over the long lengths with the long masks, once per (D, nbits)"""
    if (D, nbits) not in _CODED:
        rng = np.random.default_rng(1000 * D + nbits)
        lens = C.long_lens(rng)
        codec = _codec(D, nbits)
        codes, res = _rows(codec, sum(lens), seed=D + nbits)
        _CODED[(D, nbits)] = (codec, codes, res, torch.from_numpy(C.long_masks(lens, rng)), lens)
    return _CODED[(D, nbits)]


# nbits 8 at every form the plaid launcher takes; nbits 1, 2 and 4 at one multi-pass shape each; D 32 (nbits 8 starts at D 64) at nbits 4
PLAID_CASES = [(D, nq, Lq, 8) for D, nq, Lq in C.FORM_SHAPES if D in (64, 128, 256)] + [(32, 3, 20, 4), (128, 1, 129, 1), (64, 3, 130, 2), (256, 2, 65, 4)]


@pytest.mark.parametrize("D,nq,Lq,nbits", PLAID_CASES)
def test_the_plaid_kernel_equals_the_fp16_kernel_over_the_decoded_rows_at_every_form(D, nq, Lq, nbits):
    codec, codes, res, mask, lens = _coded(D, nbits)
    assert nbits == 8 or D == 32 or _form(nq, Lq, D, plaid=True)[2] > 1
    q = _queries(D, nq, Lq)
    first, n = SUBRANGE["long"]
    for a, cnt in ((0, len(lens)), (first, n)):
        got, want = _op_pair(codec, codes, res, mask, lens, q, a, cnt)
        assert torch.equal(got, want), (f"D {D} nbits {nbits} nq {nq} Lq {Lq} form {_form(nq, Lq, D, plaid=True)} range ({a}, {cnt}): A differs "
                                        f"at {(got != want).nonzero()[:3].tolist()}")


@pytest.mark.parametrize("nq,Lq", [(3, 130), (2, 49)])
@pytest.mark.parametrize("D", [64, 128])
def test_long_passages_end_to_end_through_an_engine(D, nq, Lq):
    fx, E, q = _exact("long", D, nq, Lq)
    eng = _engine(D)
    plain, coded = _bank(eng, fx), _bank(eng, fx, coded=True)
    P = len(fx["lens"])
    first, n = SUBRANGE["long"]
    for a, cnt in ((0, P), (first, n)):
        got = eng.bank_search_f16(plain, q, K, NDOCS, slack=0.0, first=a, count=cnt)
        want = eng.bank_search(plain, q, K, first=a, count=cnt)
        torch.cuda.synchronize()
        tag = f"D {D} nq {nq} Lq {Lq} range ({a}, {cnt})"
        assert torch.equal(got["indices"], want["indices"]) and torch.equal(got["scores"], want["scores"]), tag
        idx, sc, cert = C.search_f16(E[:, a:a + cnt], E[:, a:a + cnt], NDOCS, K, 0.0, a)
        assert np.array_equal(got["indices"].cpu().numpy(), idx) and np.array_equal(got["scores"].cpu().numpy(), sc), tag
        assert got["certified"].cpu().tolist() == cert.tolist(), tag
        _same_bytes(eng.bank_search_f16(coded, q, K, NDOCS, slack=0.0, first=a, count=cnt), got, tag + " coded")
        whole = eng.bank_search_f16(plain, q, K, 1024, slack=0.0, first=a, count=cnt)
        assert torch.equal(whole["indices"], want["indices"]) and torch.equal(whole["scores"], want["scores"]) and whole["certified"].tolist() == [1] * nq
    # a compressed bank over the long lengths and the fp16 bank of its decoded rows: the same bytes from the two entries
    codec, codes, res, mask, lens = _coded(D, 8)
    comp = eng.create_bank(sum(lens) + 8, len(lens) + 4, codec=codec)
    comp.add_compressed([f"p{i}" for i in range(len(lens))], codes, res, lens, mask=mask)
    twin = _fp16_twin(eng, comp, lens, max(lens))
    qr = _queries(D, nq, Lq)
    for a, cnt in ((0, len(lens)), (first, n)):
        for ndocs in (NDOCS, 1024):
            _same_bytes(eng.bank_search_f16_plaid(comp, qr, K, ndocs, first=a, count=cnt), eng.bank_search_f16(twin, qr, K, ndocs, first=a, count=cnt),
                        f"compressed D {D} nq {nq} Lq {Lq} range ({a}, {cnt}) ndocs {ndocs}")
    want = eng.bank_search(comp, qr, K)
    whole = eng.bank_search_f16_plaid(comp, qr, K, 1024)
    assert torch.equal(whole["indices"], want["indices"]) and torch.equal(whole["scores"], want["scores"]) and whole["certified"].tolist() == [1] * nq


def _unit_bank(eng, D, n, low, high):
    """A compressed bank of n one-row passages in adversarial_fixture's layout: a decoded row is a unit vector, so the rows are the
    centroid `low` (normalised) at the low indices and `high` at the highest; zero weights: the decoded row is the centroid."""
    from rmr_amd import PlaidCodec
    cen = torch.zeros(2, D)
    cen[0, :2], cen[1, :2] = torch.tensor(low), torch.tensor(high)
    codec = PlaidCodec(torch.nn.functional.normalize(cen, dim=-1), torch.zeros(2), 1)
    bank = eng.create_bank(n + 4, n + 2, codec=codec)
    codes = torch.zeros(n, dtype=torch.int32)
    codes[n - 1] = 1
    bank.add_compressed([f"p{i}" for i in range(n)], codes, torch.zeros((n, codec.residual_bytes), dtype=torch.uint8), [1] * n)
    return bank


def _out_of_range_banks(eng, D, which):
    """[(name, bank, entry)]: the fixture in a plain bank, and its like in a compressed bank (unit rows: the winner differs from
    the others in direction, -0.6 e1 + 0.8 e2 against -e1 under the query 70000 e1, e1 against 0.6 e1 + 0.8 e2 under 2^-26 e1)"""
    fx = (C.overflow_fixture if which == "overflow" else C.underflow_fixture)(D, NDOCS)
    low, high = ((-1.0, 0.0), (-0.6, 0.8)) if which == "overflow" else ((0.6, 0.8), (1.0, 0.0))
    return fx, [("plain", _bank(eng, fx), eng.bank_search_f16), ("compressed", _unit_bank(eng, D, len(fx["lens"]), low, high), eng.bank_search_f16_plaid)]


@pytest.mark.parametrize("which", ["overflow", "underflow"])
def test_a_query_outside_the_range_of_fp16_is_not_certified_at_the_default_slack(which):
    from rmr_amd import F16Search
    D = 64
    eng = _engine(D)
    fx, banks = _out_of_range_banks(eng, D, which)
    n = len(fx["lens"])
    q = torch.from_numpy(fx["q"]).cuda()
    slack = F16Search(NDOCS).slack_for(q)
    assert slack == float("inf") if which == "overflow" else slack == pytest.approx(C.default_slack(fx["q"], D), rel=1e-9)
    for name, bank, entry in banks:
        want = eng.bank_search(bank, q, K)
        assert int(want["indices"][0, 0]) == n - 1 and float(want["scores"][0, 0]) > float(want["scores"][0, 1]), f"{name}: the exact winner"
        for got in (entry(bank, q, K, NDOCS), bank.search(eng, q, K, fast=F16Search(NDOCS))):
            torch.cuda.synchronize()
            assert got["indices"][0].tolist() == list(range(K)), f"{name}: every A ties, the survivors go by bank index"
            assert bool((got["scores"][0] == want["scores"][0, 1]).all()), f"{name}: the exact scores of the losers"
            assert got["certified"].tolist() == [0], f"{name}: the exact winner is missing and the query is certified"
        for got in (entry(bank, q, K, 1024), bank.search(eng, q, K, fast=F16Search(1024))):      # m == n: every passage rescored
            assert torch.equal(got["indices"], want["indices"]) and torch.equal(got["scores"], want["scores"]) and got["certified"].tolist() == [1], name
    if which == "overflow":
        A = _op_scores(fx, q)
        assert bool(torch.isneginf(A).all()), "the fp16 query is +inf: every A is -inf"
    else:
        assert bool((_op_scores(fx, q) == 0.0).all()), "the fp16 query is 0: every A is 0"


def test_infinite_queries_are_never_certified_and_nan_queries_are_refused():
    from rmr_amd import F16Search, _lib as L
    D = 64
    eng = _engine(D)
    fx, banks = _out_of_range_banks(eng, D, "underflow")                   # rows 0.5 e1 and 1.0 e1 (compressed: unit rows)
    q = torch.from_numpy(fx["q"]).cuda()
    q[0, 0, 0] = float("inf")
    assert F16Search(NDOCS).slack_for(q) == float("inf")
    for name, bank, entry in banks:
        for got in (entry(bank, q, K, NDOCS), bank.search(eng, q, K, fast=F16Search(NDOCS))):
            assert got["certified"].tolist() == [0], name
    q[0, 0, 1] = float("nan")
    slack = F16Search(NDOCS).slack_for(q)
    assert slack != slack
    for (name, bank, entry), raw in zip(banks, (_raw, _raw_plaid)):
        out = _poisoned(1, K)
        assert raw(eng, bank, q, 0, -1, NDOCS, K, slack, out) == L.RR_ERR_BAD_ARG, name
        assert _untouched(out), f"{name}: a refused call wrote something"
        with pytest.raises(ValueError):
            entry(bank, q, K, NDOCS)
        with pytest.raises(ValueError):
            bank.search(eng, q, K, fast=F16Search(NDOCS))
