"""GPU: the exhaustive search of a COMPRESSED bank whose first pass runs on the fp16 matrix core (rr_bank_search_f16_plaid /
RerankEngine.bank_search_f16_plaid, PassageBank.search(fast=) on a compressed bank, rr_op_bank_scores_f16_plaid; include/rerank_mi355.h,
csrc/bank_search_f16_plaid.hip).  Every equality is torch.equal: no tolerance anywhere.

THE TWIN.  A decoded row is fp16, so the call must give, byte for byte, what rr_bank_search_f16 gives on the fp16 bank filled with
the compressed bank's read() rows and masks: A (the operators over raw arrays), indices, scores and certificates.
THE COMPRESSED BANK ITSELF.  Every returned score is rr_bank_li_scores' maxsim of its pair on the compressed bank, a certified row is
rr_bank_search's row on it, with ndocs >= n the result is rr_bank_search's, three runs give the same bytes.
A CERTIFICATE THAT IS NOT VACUOUS.  bank_f16_cases.random_fixture compressed on the device (add_compress) with a codec from its own
residuals: every query certified at the default slack with ndocs 64 < n at nbits 8 and 4 (tests/test_bank_f16_plaid_cpu.py shows
in float64, on the host definitions alone, that the fixture leaves twice the slack; nbits 2 and 1 are held to the twin only).
ADVERSARIAL.  bank_f16_cases.adversarial_fixture's rows are reachable in code space (centroids e2 and e1, every weight zero: the
decoded row is the centroid): the e1 passage is not certified away.  Refused calls write nothing.
"""
import numpy as np
import pytest
import torch

import bank_f16_cases as C
import bank_f16_plaid_cases as CP
from test_gpu_bank_search import IPOISON, POISON, _table_dev
from test_gpu_li_scores import _engine
from test_gpu_plaid_bank import N_CENTROIDS, _codec, _fill, _fp16_twin, _rows

pytestmark = pytest.mark.gpu

NDOCS, K = 64, 16
# 300 passages; the lengths reach the tail tile alone (1, 15, 16), a pair of tiles (17, 31, 32) and a pair plus a tail (33, 47);
# passage 1 is one row at row index 2, which _fill masks (every third row of the first add): a fully masked passage
_EDGE = [2, 1, 15, 16, 17, 31, 32, 33, 47]
LENS_A = _EDGE + [(7 * i) % 40 + 1 for i in range(141)]
LENS_B = _EDGE[::-1] + [(11 * i) % 28 + 1 for i in range(141)]
SHAPES = [(1, 5), (3, 32), (17, 32), (1, 130)]                            # (n_queries, Lq); Lq 130: more than one pass of the query block
_CASES = {}


def _queries(D, nq, Lq):
    gen = torch.Generator().manual_seed(1000 * D + 10 * nq + Lq)
    return torch.nn.functional.normalize(torch.randn(nq, Lq, D, generator=gen), dim=-1).cuda()


def _case(D, nbits):
    """(engine, compressed bank, its fp16 twin, codec, codes, residuals, mask, lengths), built once per (D, nbits)"""
    if (D, nbits) not in _CASES:
        eng = _engine(D)
        codec = _codec(D, nbits)
        bank, codes, res, mask, lens = _fill(eng, codec, LENS_A, LENS_B, seed=D + nbits)
        assert len(lens) == 300 and int(codes.min()) == 0 and int(codes.max()) == N_CENTROIDS - 1
        rows1, mask1 = bank.read("p1")
        assert not bool(mask1.any()), "passage 1 is fully masked"
        assert not bool(bank.read("p0")[0][0].view(torch.int16).any()), "row 0 has norm zero"
        _CASES[(D, nbits)] = (eng, bank, _fp16_twin(eng, bank, lens, max(lens)), codec, codes, res, mask, lens)
    return _CASES[(D, nbits)]


def _op_pair(codec, codes, res, mask, lens, q, first, n):
    """(A from rr_op_bank_scores_f16_plaid over the raw compressed arrays, A from rr_op_bank_scores_f16 over the decoded rows), each
    with a poisoned extra row that must stay untouched"""
    from rmr_amd import _lib as L
    lib = L.load()
    D, nq, Lq = codec.dim, q.shape[0], q.shape[1]
    st = torch.cuda.current_stream().cuda_stream
    table = _table_dev(lens)
    d = dict(codes=codes.cuda(), res=res.cuda().contiguous(), mask=mask.cuda(), cen=codec.centroids.cuda(), w=codec.bucket_weights.cuda(),
             rows=codec.decode(codes, res).cuda())
    got = torch.full((nq + 1, n), POISON, device="cuda")
    want = torch.full((nq + 1, n), POISON, device="cuda")
    rc = lib.rr_op_bank_scores_f16_plaid(L.ptr(q), nq, Lq, D, L.ptr(table), first, n, L.ptr(d["mask"]), codec.nbits, L.ptr(d["codes"]),
                                         L.ptr(d["res"]), L.ptr(d["cen"]), L.ptr(d["w"]), codec.n_centroids, L.ptr(got), st)
    assert rc == 0, rc
    rc = lib.rr_op_bank_scores_f16(L.ptr(q), nq, Lq, D, L.ptr(table), first, n, L.ptr(d["rows"]), L.ptr(d["mask"]), L.ptr(want), st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert (got[nq:] == POISON).all() and (want[nq:] == POISON).all()
    return got[:nq], want[:nq]


def _same_bytes(a, b, tag):
    for key in ("indices", "scores", "certified"):
        assert torch.equal(a[key], b[key]), f"{tag}: {key} differ"


@pytest.mark.parametrize("nbits", [1, 2, 4, 8])
@pytest.mark.parametrize("D", [64, 128])
def test_twin_equality_the_fp16_bank_of_the_decoded_rows(D, nbits):
    eng, bank, twin, codec, codes, res, mask, lens = _case(D, nbits)
    P = len(lens)
    o = sum(lens[:6])
    assert torch.equal(bank.read("p6")[0].view(torch.int16), codec.decode(codes[o:o + lens[6]], res[o:o + lens[6]]).view(torch.int16))
    for nq, Lq in SHAPES:
        q = _queries(D, nq, Lq)
        for first, n in ((0, P), (37, P - 137)):                           # chunks of 32 start off a boundary and end short
            tag = f"D {D} nbits {nbits} nq {nq} Lq {Lq} range ({first}, {n})"
            got, want = _op_pair(codec, codes, res, mask, lens, q, first, n)
            assert torch.equal(got, want), f"{tag}: A differs at {(got != want).nonzero()[:3].tolist()}"
            for ndocs, k in ((NDOCS, K), (NDOCS, NDOCS), (1024, K)):
                a = eng.bank_search_f16_plaid(bank, q, k, ndocs, first=first, count=n)
                b = eng.bank_search_f16(twin, q, k, ndocs, first=first, count=n)
                torch.cuda.synchronize()
                _same_bytes(a, b, f"{tag} ndocs {ndocs} k {k}")


@pytest.mark.parametrize("D,nbits", [(32, 4), (256, 8)])
def test_twin_equality_of_the_first_pass_at_d_32_and_256(D, nbits):
    """the operators over raw arrays (no handle takes li_dim 32): D / 8 = 4 lanes per row (16 rows per pass) and 32 (2 rows per pass)"""
    codec = _codec(D, nbits)
    lens = LENS_A[:40] + LENS_B[:24]
    codes, res = _rows(codec, sum(lens), seed=D)
    mask = torch.ones(sum(lens), dtype=torch.uint8)
    mask[torch.arange(2, sum(lens), 3)] = 0
    for nq, Lq in SHAPES:
        q = _queries(D, nq, Lq)
        for first, n in ((0, len(lens)), (3, len(lens) - 9)):
            got, want = _op_pair(codec, codes, res, mask, lens, q, first, n)
            assert torch.equal(got, want), f"D {D} nq {nq} Lq {Lq} range ({first}, {n}): A differs at {(got != want).nonzero()[:3].tolist()}"


@pytest.mark.parametrize("D,nbits", [(64, 4), (128, 8)])
def test_exact_on_the_compressed_bank_itself(D, nbits):
    eng, bank, twin, codec, codes, res, mask, lens = _case(D, nbits)
    P, nq = len(lens), 3
    q = _queries(D, nq, 32)
    ids = [f"p{i}" for i in range(P)] * nq
    E = eng.bank_li_scores(bank, q, ids, pair_query=np.repeat(np.arange(nq), P))["maxsim"].reshape(nq, P)
    want = eng.bank_search(bank, q, K)
    runs = [eng.bank_search_f16_plaid(bank, q, K, NDOCS) for _ in range(3)]
    whole = eng.bank_search_f16_plaid(bank, q, K, 1024)                    # ndocs >= n: every passage is rescored
    torch.cuda.synchronize()
    got = runs[0]
    assert torch.equal(got["scores"], E.gather(1, got["indices"].long())), "a returned score is not its pair's exact score"
    cert = got["certified"].bool()
    assert torch.equal(got["indices"][cert], want["indices"][cert]) and torch.equal(got["scores"][cert], want["scores"][cert])
    for r in runs[1:]:
        _same_bytes(r, got, "run to run")
    assert not bool(torch.isinf(whole["scores"]).any()) and whole["certified"].tolist() == [1] * nq
    assert torch.equal(whole["indices"], want["indices"]) and torch.equal(whole["scores"], want["scores"])


def _compressed_random(D, nq, Lq, nbits):
    """bank_f16_cases.random_fixture in a compressed bank: compressed on the device (add_compress), two adds"""
    key = ("random", D, nq, Lq, nbits)
    if key not in _CASES:
        fx = C.random_fixture(D, nq, Lq, seed=D + Lq)
        eng = _engine(D)
        codec = CP.fixture_codec(fx, nbits)
        P, half = len(fx["lens"]), len(fx["lens"]) // 2
        bank = eng.create_bank(int(np.sum(fx["lens"])) + 8, P + 4, codec=codec)
        for lo, hi in ((0, half), (half, P)):
            li, cm, lens = C.padded(fx, lo, hi)
            bank.add_compress([f"p{i}" for i in range(lo, hi)], torch.from_numpy(li), torch.from_numpy(cm), lengths=lens)
        _CASES[key] = (fx, eng, bank, torch.from_numpy(fx["q"]).cuda())
    return _CASES[key]


@pytest.mark.parametrize("nbits", [8, 4])
@pytest.mark.parametrize("D,nq,Lq", [(128, 17, 32), (64, 3, 5)])
def test_every_query_of_the_planted_fixture_is_certified(D, nq, Lq, nbits):
    """a condition on the fixture, shown on the host definitions in tests/test_bank_f16_plaid_cpu.py; nbits 2 and 1 are not held to
    it (their decoded rows blur the planted copies), the twin test covers them"""
    fx, eng, bank, q = _compressed_random(D, nq, Lq, nbits)
    assert NDOCS < len(fx["lens"])
    got = eng.bank_search_f16_plaid(bank, q, K, NDOCS)
    want = eng.bank_search(bank, q, K)
    torch.cuda.synchronize()
    cert = got["certified"].bool()
    assert cert.all(), f"queries {(~cert).nonzero().flatten().tolist()} are not certified at the default slack"
    assert torch.equal(got["indices"], want["indices"]) and torch.equal(got["scores"], want["scores"])


@pytest.mark.parametrize("D", [64, 128])
def test_adversarial_winner_is_not_certified_away(D):
    from rmr_amd import PlaidCodec
    fx = C.adversarial_fixture(D, NDOCS)
    n = len(fx["lens"])
    cen = torch.zeros(2, D)
    cen[0, 1], cen[1, 0] = 1.0, 1.0                                        # code 0: e2, code 1: e1; zero weights: the row is the centroid
    codec = PlaidCodec(cen, torch.zeros(2), 1)
    eng = _engine(D)
    bank = eng.create_bank(n + 4, n + 2, codec=codec)
    codes = torch.zeros(n, dtype=torch.int32)
    codes[n - 1] = 1
    bank.add_compressed([f"p{i}" for i in range(n)], codes, torch.zeros((n, codec.residual_bytes), dtype=torch.uint8), [1] * n)
    assert np.array_equal(bank.read(f"p{n - 1}")[0].float().cpu().numpy(), fx["rows"][n - 1:]) and \
        np.array_equal(bank.read("p0")[0].float().cpu().numpy(), fx["rows"][:1]), "the fixture's rows are reachable in code space"
    q = torch.from_numpy(fx["q"]).cuda()
    want = eng.bank_search(bank, q, K)
    assert int(want["indices"][0, 0]) == n - 1 and float(want["scores"][0, 0]) == 1.0 + 2.0 ** -12
    for slack in (0.0, None):
        got = eng.bank_search_f16_plaid(bank, q, K, NDOCS, slack=slack)
        torch.cuda.synchronize()
        assert got["indices"][0].tolist() == list(range(K)), "ties in A go by bank index: the e1 passage is no survivor"
        assert (got["scores"] == np.float32(1.0 - 2.0 ** -13)).all() and got["certified"].tolist() == [0]
    whole = eng.bank_search_f16_plaid(bank, q, K, 1024, slack=0.0)          # every passage rescored: the exact result, certified
    assert torch.equal(whole["indices"], want["indices"]) and torch.equal(whole["scores"], want["scores"]) and whole["certified"].tolist() == [1]


def _raw(eng, bank, q, first, n, ndocs, k, slack, out, cert=True, stream=None):
    from rmr_amd import _lib as L
    return eng.lib.rr_bank_search_f16_plaid(eng.h, bank.h, L.ptr(q), q.shape[0], q.shape[1], first, n, ndocs, k, slack, L.ptr(out[0]),
                                            L.ptr(out[1]), L.ptr(out[2]) if cert else None,
                                            torch.cuda.current_stream().cuda_stream if stream is None else stream)


def _poisoned(nq, k):
    return (torch.full((nq, k), IPOISON, device="cuda", dtype=torch.int32), torch.full((nq, k), POISON, device="cuda"),
            torch.full((nq,), IPOISON, device="cuda", dtype=torch.int32))


def _untouched(out):
    torch.cuda.synchronize()
    return bool((out[0] == IPOISON).all() and (out[1] == POISON).all() and (out[2] == IPOISON).all())


def test_refusals_write_nothing():
    from rmr_amd import _lib as L
    D = 64
    eng, bank, twin, codec, codes, res, mask, lens = _case(D, 4)
    P = len(lens)
    q = _queries(D, 3, 5)
    out = _poisoned(3, 1025)
    gen = torch.Generator().manual_seed(D)
    coded = eng.create_bank(64, 8, centroids=torch.nn.functional.normalize(torch.randn(33, D, generator=gen), dim=-1).half())
    coded.add(["a", "b", "c", "d"], torch.nn.functional.normalize(torch.randn(4, 5, D, generator=gen), dim=-1), torch.ones(4, 5), lengths=[5, 1, 4, 2])
    for fp16 in (twin, coded):                                             # an fp16 bank, plain or coded
        assert _raw(eng, fp16, q, 0, -1, 4, 2, 0.0, out) == L.RR_ERR_UNSUPPORTED and b"rr_bank_search_f16" in eng.lib.rr_last_error(eng.h)
    assert _raw(eng, bank, q, 0, -1, 8, 9, 0.0, out) == L.RR_ERR_BAD_SHAPE                    # k > ndocs
    assert _raw(eng, bank, q, 0, -1, 8, 0, 0.0, out) == L.RR_ERR_BAD_SHAPE
    assert _raw(eng, bank, q, 0, 4, 8, 5, 0.0, out) == L.RR_ERR_BAD_SHAPE                     # k > n_passages
    assert _raw(eng, bank, q, 0, -1, 1025, 4, 0.0, out) == L.RR_ERR_UNSUPPORTED               # ndocs > 1024
    assert _raw(eng, bank, q, 0, -1, 8, 4, float("nan"), out) == L.RR_ERR_BAD_ARG
    assert _raw(eng, bank, q, 0, -1, 8, 4, -1e-6, out) == L.RR_ERR_BAD_ARG
    assert _raw(eng, bank, q, 0, -1, 8, 4, 0.0, out, cert=False) == L.RR_ERR_BAD_ARG          # certified_out is required
    assert _raw(eng, bank, q, 1, P, 8, 4, 0.0, out) == L.RR_ERR_BAD_SHAPE                     # a range past the bank
    assert _untouched(out)
    with pytest.raises(NotImplementedError):
        eng.bank_search_f16_plaid(twin, q, 2, 4)
    with pytest.raises(NotImplementedError):
        eng.bank_search_f16(bank, q, 2, 4)                                 # the fp16 entry's refusal stands
    with pytest.raises(ValueError):
        eng.bank_search_f16_plaid(bank, q, 9, 8)
    out = _poisoned(3, 4)
    assert _raw(eng, bank, q, 0, -1, 8, 4, 0.0, out) == 0                                      # the same arguments, accepted
    torch.cuda.synchronize()
    assert not (out[0] == IPOISON).any() and not (out[1] == POISON).any() and not (out[2] == IPOISON).any()


def test_a_capturing_stream_is_refused_and_nothing_is_written():
    from rmr_amd import _lib as L
    D = 64
    eng, bank, twin, codec, codes, res, mask, lens = _case(D, 4)
    q = _queries(D, 3, 5)
    out = _poisoned(3, 4)
    probe = torch.zeros(1, device="cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        assert _raw(eng, bank, q, 0, -1, 8, 4, 0.0, out, stream=st.cuda_stream) == 0           # the table and the block exist
        torch.cuda.synchronize()
        for t in out:
            t.fill_(IPOISON if t.dtype == torch.int32 else POISON)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            probe.add_(1.0)                                                # the graph holds this node alone
            rc = _raw(eng, bank, q, 0, -1, 8, 4, 0.0, out, stream=st.cuda_stream)
            msg = eng.lib.rr_last_error(eng.h)
        graph.replay()
    torch.cuda.synchronize()
    assert rc == L.RR_ERR_BAD_ARG and b"captured" in msg
    assert probe.item() == 1.0 and _untouched(out)


def test_the_python_surface_gives_the_one_banks_bytes():
    """PassageBank.search(fast=), search_bank_part, search_banks(fast=) over two compressed halves and retrieve(fast=,
    return_certified=True): the one compressed bank's result, the merged certificate the minimum of the parts'."""
    from rmr_amd import F16Search, InteractionRerankModel, search_bank_part, search_banks
    D, nq, Lq = 64, 3, 5
    fx, eng, bank, q = _compressed_random(D, nq, Lq, 8)
    P, half = len(fx["lens"]), len(fx["lens"]) // 2
    fast = F16Search(NDOCS)
    one = eng.bank_search_f16_plaid(bank, q, K, NDOCS)
    _same_bytes(bank.search(eng, q, K, fast=fast), one, "PassageBank.search")
    part = search_bank_part(eng, bank, q, K, fast=fast)
    _same_bytes(part, one, "search_bank_part")
    assert part["counts"].tolist() == [K] * nq
    banks = []
    for lo, hi in ((0, half), (half, P)):
        b = eng.create_bank(int(np.sum(fx["lens"][lo:hi])) + 8, hi - lo + 4, codec=bank.codec)
        li, cm, lens = C.padded(fx, lo, hi)
        b.add_compress([f"p{i}" for i in range(lo, hi)], torch.from_numpy(li), torch.from_numpy(cm), lengths=lens)
        banks.append(b)
    parts = [search_bank_part(eng, b, q, K, fast=fast) for b in banks]
    ids, scores, counts, cert = search_banks(eng, banks, q, K, fast=fast)
    want_ids, want_scores = bank.search(eng, q, K)
    assert torch.equal(cert, torch.minimum(parts[0]["certified"], parts[1]["certified"])) and cert.tolist() == [1] * nq
    assert ids == want_ids and torch.equal(scores, want_scores) and counts.tolist() == [K] * nq
    assert ids == [[f"p{j}" for j in row] for row in one["indices"].tolist()] and torch.equal(scores, one["scores"])
    model = object.__new__(InteractionRerankModel)
    model.bank, model.engine = bank, eng
    r_ids, r_scores, r_cert = model.retrieve(q, K, fast=fast, return_certified=True)
    assert r_ids == ids and torch.equal(r_scores, one["scores"]) and torch.equal(r_cert, one["certified"])
