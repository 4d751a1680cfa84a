"""GPU: an fp16 passage bank with a centroid table, a "coded" fp16 bank (rr_bank_set_centroids, include/rerank_mi355.h): one centroid
code per row beside the fp16 rows, assigned on the device, and with them the pruned searches, the inverted file, the filters, the
removal and the sharded search of a compressed bank, the exact stage on the bank's own fp16 rows.  Every equality is bitwise.

Shapes.  li_dim 128 and 64.  A bank of li_dim 16 cannot exist (rr_create wants li_dim a multiple of 64, and a bank belongs to a
handle), so the second width is 64, the narrowest a bank can have; the assignment kernel itself runs at 16 in
tests/test_gpu_plaid_compress.py.  C = 200 centroids (not a multiple of 64: stage 0 pads to ceil64), 300
passages of 1 .. 40 rows in two adds, interior masked rows, one passage without an unmasked row, passages of one row; 4 200 passages
of 1 .. 3 rows (the selection of the pruned search crosses a 4 096 slice); "compress_chunk" 64 (four splits of the 200 centroids).
The PROPERTY (ncells = n_centroids) needs n_centroids <= 16, the most cells a query token may open: it runs on the 16 centroids
and the passages of tests/bank_life.py.

F is the coded bank, P a compressed bank (nbits 8) filled by rr_bank_add_compress from the same tensors and table, N a plain fp16 bank.
The oracle of a pruned search is made of the device's own parts, as for the compressed bank: S from the tap of stage 0, the
pruning restated in numpy (tests/plaid_search_ref.py) over the codes read back, the exact scores from rr_bank_li_scores on F."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import bank_life
import bank_remove_cases as RC
import plaid_search_ref as R
from plaid_ivf_exact_cases import ivf_fast
from test_bank_ivf_cpu import ivf_lib
from test_gpu_li_scores import _engine as _bare_engine
from test_gpu_passage_bank import _engine as _golden_engine
from test_gpu_passage_bank import _fixture_bank, _labels, _same
from test_sharding_gloo import _run_world

pytestmark = pytest.mark.gpu

N_CENTROIDS, PASSAGES, MAX_LEN = 200, 300, 40
FULLY_MASKED = 123
NDOCS = 64                                    # k = ndocs / 4 = 16
SEARCH = dict(ncells=2, centroid_score_threshold=0.3, ndocs=NDOCS)


def _L():
    from rmr_amd import _lib as L
    return L, L.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _eng(D):
    return _bare_engine(D) if D == 128 else _golden_engine("int_tiny")[0]


def _codec(D, C_, seed=0):
    """Unit fp16 centroids, nbits 8, cutoffs 2^-26 off the grid of residuals (as tests/bank_life.py)."""
    from rmr_amd import PlaidCodec
    gen = torch.Generator().manual_seed(7000 + 10 * D + C_ + seed)
    cen = torch.nn.functional.normalize(torch.randn(C_, D, generator=gen), dim=-1).half()
    return PlaidCodec(cen, torch.linspace(-0.1, 0.1, 256), 8, bucket_cutoffs=torch.linspace(-0.1, 0.1, 255) + 2.0 ** -26)


def _corpus(cen, lens, seed, calls=2, fully_masked=None):
    """The padded tensors of `calls` adds: [(ids, x float32 [n, Lc, D], m float32 [n, Lc], lens)].  A passage holds noisy unit rows of
    three of the centroids (so a query's cells reach a part of the corpus); every third passage of three rows or more has
    interior masked rows; passage `fully_masked` has no unmasked row."""
    gen = torch.Generator().manual_seed(seed)
    Cn, D = cen.shape
    cen = cen.float()
    out, per = [], (len(lens) + calls - 1) // calls
    for c0 in range(0, len(lens), per):
        ln = lens[c0:c0 + per]
        n, Lc = len(ln), max(ln)
        topics = torch.randint(0, Cn, (n, 3), generator=gen)
        pick = topics.gather(1, torch.randint(0, 3, (n, Lc), generator=gen))
        x = torch.nn.functional.normalize(cen[pick] + 0.5 * torch.randn(n, Lc, D, generator=gen) / D ** 0.5, dim=-1)
        m = torch.zeros(n, Lc)
        for i, l in enumerate(ln):
            m[i, :l] = 1.0
            if (c0 + i) % 3 == 1 and l >= 3:
                m[i, 1:l - 1:2] = 0.0
            if c0 + i == fully_masked:
                m[i] = 0.0
        out.append(([f"p{c0 + i}" for i in range(n)], x, m, list(ln)))
    return out


def _queries(cen, nq, Lq, seed):
    """Unit query tokens near two centroids each."""
    gen = torch.Generator().manual_seed(seed)
    Cn, D = cen.shape
    near = torch.randint(0, Cn, (nq, 2), generator=gen)
    pick = near.gather(1, torch.randint(0, 2, (nq, Lq), generator=gen))
    return torch.nn.functional.normalize(cen.float()[pick] + 0.3 * torch.randn(nq, Lq, D, generator=gen) / D ** 0.5, dim=-1).cuda()


def _fill(bank, corpus, compress=False):
    for ids, x, m, lens in corpus:
        (bank.add_compress if compress else bank.add)(ids, x, m, lengths=lens)
    return bank


def _codes_of(bank):
    return torch.cat([bank.codes(pid) for pid in bank.table.ids]).numpy()


def _rows_of(bank):
    got = [bank.read(pid) for pid in bank.table.ids]
    return torch.cat([r for r, _ in got]), torch.cat([m for _, m in got]).numpy()


def _ivf_bytes(bank):
    pids, lengths = bank.ivf()
    return pids.numpy().tobytes(), lengths.numpy().tobytes()


@functools.lru_cache(maxsize=None)
def _case(D):
    """F, P and N over one corpus and one table, with what the tests share: the codes and rows read back, the queries, the exact
    scores of every (query, passage) on F."""
    eng = _eng(D)
    codec = _codec(D, N_CENTROIDS)
    lens = [(7 * i) % MAX_LEN + 1 for i in range(PASSAGES)]
    assert set(lens) == set(range(1, MAX_LEN + 1)) and lens[FULLY_MASKED] >= 3
    corpus = _corpus(codec.centroids, lens, seed=D, fully_masked=FULLY_MASKED)
    rows, slots = sum(lens) + 64, PASSAGES + 8
    F = _fill(eng.create_bank(rows, slots, centroids=codec.centroids), corpus)
    P = _fill(eng.create_bank(rows, slots, codec=codec), corpus, compress=True)
    N = _fill(eng.create_bank(rows, slots), corpus)
    q = _queries(codec.centroids, 3, 8 if D == 128 else 20, seed=D + 1)
    ids = list(F.table.ids)
    exact = F.maxsim(eng, q, ids * q.shape[0], K=len(ids)).reshape(q.shape[0], len(ids)).cpu().numpy()
    frows, fmask = _rows_of(F)
    return dict(eng=eng, codec=codec, lens=lens, corpus=corpus, F=F, P=P, N=N, q=q, exact=exact, codes=_codes_of(F), rows=frows, mask=fmask)


# ---- 1. the codes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [128, 64])
def test_codes_are_the_compressed_row_s_and_the_compressed_bank_s(D):
    c = _case(D)
    F, P, codec = c["F"], c["P"], c["codec"]
    want, _ = codec.compress(c["rows"])                       # rr_util_plaid_compress_rows on the stored fp16 rows
    assert np.array_equal(c["codes"], want.numpy())
    assert c["mask"][sum(c["lens"][:FULLY_MASKED]):sum(c["lens"][:FULLY_MASKED + 1])].sum() == 0 and (c["mask"] == 0).sum() > 100
    r0 = 0
    for pid, ln in zip(F.table.ids, c["lens"]):
        assert torch.equal(F.codes(pid), P.read_compressed(pid)[0]), pid
        assert torch.equal(P.codes(pid), P.read_compressed(pid)[0])
        assert np.array_equal(F.codes(pid).numpy(), c["codes"][r0:r0 + ln])
        r0 += ln
    assert len(set(c["codes"].tolist())) > 150, "the rows spread over the table"
    assert F.format() == dict(nbits=0, n_centroids=N_CENTROIDS, bytes_per_row=2 * D + 1 + 4)
    assert c["N"].format() == dict(nbits=0, n_centroids=0, bytes_per_row=2 * D + 1)
    assert F.n_centroids == N_CENTROIDS and torch.equal(F.centroids, codec.centroids) and c["N"].n_centroids == 0 and c["N"].centroids is None
    assert P.n_centroids == N_CENTROIDS


def test_rows_first_or_table_first_split_or_not_the_codes_are_the_same():
    c = _case(128)
    eng, codec, corpus = c["eng"], c["codec"], c["corpus"]
    L, lib = _L()
    rows, slots = sum(c["lens"]) + 64, PASSAGES + 8
    G = _fill(eng.create_bank(rows, slots), corpus)           # filled first, the table afterwards
    G.set_centroids(codec.centroids)
    assert np.array_equal(_codes_of(G), c["codes"])
    assert lib.rr_set_tuning(b"compress_chunk", 64) == L.RR_OK       # four splits of the 200 centroids
    try:
        H = _fill(eng.create_bank(rows, slots, centroids=codec.centroids), corpus)
        assert np.array_equal(_codes_of(H), c["codes"]), "rr_bank_add under four splits"
        G.set_centroids(codec.centroids)
        assert np.array_equal(_codes_of(G), c["codes"]), "rr_bank_set_centroids under four splits"
    finally:
        assert lib.rr_set_tuning(b"compress_chunk", 0) == L.RR_OK


def test_a_second_table_gives_its_codes_and_drops_the_inverted_file():
    c = _case(128)
    eng, corpus = c["eng"], c["corpus"]
    G = _fill(eng.create_bank(sum(c["lens"]) + 64, PASSAGES + 8, centroids=c["codec"].centroids), corpus)
    assert G.build_ivf()["passages_covered"] == PASSAGES
    other = _codec(128, 77, seed=5)
    G.set_centroids(other.centroids)
    assert G.ivf_info() == dict(passages_covered=0, postings=0, longest_list=0)
    assert G.n_centroids == 77 and G.format()["n_centroids"] == 77
    assert np.array_equal(_codes_of(G), other.compress(c["rows"])[0].numpy())
    rows, mask = _rows_of(G)
    assert torch.equal(rows.view(torch.int16), c["rows"].view(torch.int16)) and np.array_equal(mask, c["mask"])
    assert G.build_ivf()["passages_covered"] == PASSAGES
    off, pids = ivf_lib(_codes_of(G), mask, c["lens"], 77)
    assert _ivf_bytes(G) == (pids.tobytes(), np.diff(off).tobytes())


# ---- 2. the rows are untouched ------------------------------------------------------------------------------------------------------
def test_what_reads_the_rows_gives_the_plain_bank_s_bits():
    c = _case(128)
    eng, F, N, q = c["eng"], c["F"], c["N"], c["q"]
    nrows, nmask = _rows_of(N)
    assert torch.equal(c["rows"].view(torch.int16), nrows.view(torch.int16)) and np.array_equal(c["mask"], nmask)
    ids = list(F.table.ids)[::7]
    kw = dict(K=len(ids), want_scores=True)
    a, b = eng.bank_li_scores(F, q, ids * 3, **kw), eng.bank_li_scores(N, q, ids * 3, **kw)
    assert torch.equal(a["maxsim"], b["maxsim"]) and torch.equal(a["scores"], b["scores"])
    a, b = eng.bank_search(F, q, 50), eng.bank_search(N, q, 50)
    assert torch.equal(a["indices"], b["indices"]) and torch.equal(a["scores"], b["scores"])
    flt = list(F.table.ids)[1::3]
    for sparse in (False, True):
        (ia, sa), (ib, sb) = (bk.search(eng, q, 20, filter=bk.filter(allowed=flt), sparse=sparse) for bk in (F, N))
        assert ia == ib and torch.equal(sa, sb)


def test_the_forward_from_a_coded_bank_is_the_plain_bank_s():
    eng, g = _golden_engine("int_tiny")
    Bq, K = int(g["Bq"]), int(g["K"])
    plain, (q, c, qm, cm) = _fixture_bank(eng, g, extra=2)
    coded, _ = _fixture_bank(eng, g, extra=2)
    coded.set_centroids(_codec(64, 33).centroids)
    ids = [f"d{i}" for i in range(Bq * K)]
    kw = dict(granule=8, want_order=True, want_scores=True)
    want = eng.forward_interaction_bank(plain, q, qm, ids, Bq, K, _labels(g), **kw)
    got = eng.forward_interaction_bank(coded, q, qm, ids, Bq, K, _labels(g), **kw)
    torch.cuda.synchronize()
    _same(got, want, ("logits", "logits2", "loss", "order", "scores"))


# ---- 3. the pruned searches ---------------------------------------------------------------------------------------------------------
def _check_lists(r, exact, k, first=0):
    """What every pruned result on F must be, given the exact scores of F: the scores are those, the order is their rank order,
    -1 / -inf behind the count.  Returns the index lists."""
    idx, sc, cnt = r["indices"].cpu().numpy(), r["scores"].cpu().numpy(), r["counts"].tolist()
    out = []
    for qi, cn in enumerate(cnt):
        assert 0 <= cn <= k and (idx[qi, cn:] == -1).all() and np.isneginf(sc[qi, cn:]).all()
        got = idx[qi, :cn].tolist()
        assert len(set(got)) == cn and all(first <= p for p in got)
        assert np.array_equal(sc[qi, :cn].view(np.int32), exact[qi][got].view(np.int32)), f"query {qi}: the scores are rr_bank_li_scores'"
        assert got == R.order(exact[qi], got), f"query {qi}: rank order"
        out.append(got)
    return out


def _four_entries(eng, F, P, q, exact, k, allowed_ids, **kw):
    """rr_bank_search_plaid, rr_bank_search_plaid_ivf and the filtered form of each on F and on P: equal counts, equal index sets,
    and on F the scores and the order of the exact scores.  Returns F's lists of the two unfiltered entries and of the two filtered."""
    for bk in (F, P):
        if bk.ivf_info()["passages_covered"] < len(bk):
            bk.build_ivf()
    ff, fp = F.filter(allowed=allowed_ids), P.filter(allowed=allowed_ids)
    lists = []
    for entry, filtered in (("bank_search_plaid", False), ("bank_search_plaid_ivf", False), ("bank_search_plaid_filtered", True),
                            ("bank_search_plaid_ivf_filtered", True)):
        rF = getattr(eng, entry)(F, q, k, *([ff] if filtered else []), **kw)
        rP = getattr(eng, entry)(P, q, k, *([fp] if filtered else []), **kw)
        torch.cuda.synchronize()
        assert torch.equal(rF["counts"], rP["counts"]), entry
        got = _check_lists(rF, exact, k)
        iP, cP = rP["indices"].cpu().numpy(), rP["counts"].tolist()
        for qi, g in enumerate(got):
            assert set(g) == set(iP[qi, :cP[qi]].tolist()), f"{entry}, query {qi}: stages 0 - 2 see the same codes"
        lists.append(got)
    assert lists[0] == lists[1] and lists[2] == lists[3], "the inverted file gives the scan's result"
    return lists[0], lists[2]


@pytest.mark.parametrize("D", [128, 64])
def test_pruned_searches_on_the_coded_bank(D):
    c = _case(D)
    eng, F, P, q, exact, lens = c["eng"], c["F"], c["P"], c["q"], c["exact"], c["lens"]
    nq, Lq, k = q.shape[0], q.shape[1], NDOCS // 4
    allowed = [pid for i, pid in enumerate(F.table.ids) if i % 3 != 2]
    plain, filtered = _four_entries(eng, F, P, q, exact, k, allowed, **SEARCH)
    # the oracle from the device's own parts, and the conditions on the inputs
    eng.bank_search_plaid(F, q, k, **SEARCH)
    S = eng.bank_search_plaid_tap("S").reshape(nq, N_CENTROIDS, Lq)
    lost, partial = 0, 0
    gone = np.array([i % 3 == 2 for i in range(PASSAGES)])
    for qi in range(nq):
        pr = R.prune(S[qi], c["codes"], c["mask"], lens, SEARCH["ncells"], SEARCH["centroid_score_threshold"], NDOCS)
        cand = int((~np.isneginf(pr["a1"])).sum())
        assert len(pr["list2"]) >= 1, "every query keeps a survivor"
        lost += len(pr["list2"]) < cand
        partial += cand < PASSAGES
        assert pr["a1"][FULLY_MASKED] == -np.inf, "no unmasked row: no candidate"
        assert plain[qi] == R.final(pr["list2"], exact[qi], k), f"query {qi}"
        masked = np.where(np.repeat(gone, lens), 0, c["mask"])         # a filtered-out passage: as if fully masked
        pf = R.prune(S[qi], c["codes"], masked, lens, SEARCH["ncells"], SEARCH["centroid_score_threshold"], NDOCS)
        assert filtered[qi] == R.final(pf["list2"], exact[qi], k), f"query {qi}, filtered"
        assert all(p % 3 != 2 for p in filtered[qi])
    assert lost >= 1 and partial >= 1, "the pruning is exercised, and the candidates are fewer than the passages"


def test_a_selection_over_more_than_one_slice():
    D, n = 64, 4200
    eng = _eng(D)
    codec = _codec(D, N_CENTROIDS)
    lens = [i % 3 + 1 for i in range(n)]
    corpus = _corpus(codec.centroids, lens, seed=4200, calls=1)
    F = _fill(eng.create_bank(sum(lens), n, centroids=codec.centroids), corpus)
    P = _fill(eng.create_bank(sum(lens), n, codec=codec), corpus, compress=True)
    q = _queries(codec.centroids, 2, 8, seed=42)
    ids = list(F.table.ids)
    exact = F.maxsim(eng, q, ids * 2, K=n).reshape(2, n).cpu().numpy()
    kw = dict(ncells=8, centroid_score_threshold=0.3, ndocs=256)
    plain, _ = _four_entries(eng, F, P, q, exact, 64, ids[::2], **kw)
    eng.bank_search_plaid(F, q, 64, **kw)
    a1 = eng.bank_search_plaid_tap("a1").reshape(2, n)
    assert ((~np.isneginf(a1)).sum(axis=1) > 256).all() and (~np.isneginf(a1[:, 4096:])).any(), "candidates on both sides of the slice border"
    assert all(len(g) == 64 for g in plain)


# ---- 4. the property ----------------------------------------------------------------------------------------------------------------
def _life_corpus(n, seed, serial0=0):
    """Passages of tests/bank_life.py (li_dim 64, 16 centroids, unit rows, its masks) as one padded add."""
    lens = [RC.GPU_LENGTHS[i % len(RC.GPU_LENGTHS)] % 37 + 1 for i in range(n)]
    ps = bank_life.make_passages("plaid8", [f"s{serial0 + i}" for i in range(n)], lens, serial0, seed, via="add_compress")
    Lc = max(lens)
    x, m = torch.zeros(n, Lc, bank_life.D), torch.zeros(n, Lc)
    for i, p in enumerate(ps):
        x[i, :p["length"]] = torch.from_numpy(p["x"])
        m[i, :p["length"]] = torch.from_numpy(p["mask"].astype(np.float32))
    return [([p["id"] for p in ps], x, m, lens)]


def test_every_centroid_a_cell_and_no_cut_is_the_exact_search():
    eng = _eng(64)
    codec = bank_life.codec_of("plaid8")
    Cn, n = bank_life.C_CENTROIDS, 200
    corpus = _life_corpus(n, seed=11)
    rows = sum(corpus[0][3])
    F = _fill(eng.create_bank(rows, n, centroids=codec.centroids), corpus)
    F.build_ivf()
    q = _queries(codec.centroids, 2, 32, seed=3)
    for k in (1, 200):
        want = eng.bank_search(F, q, k)
        for entry in (eng.bank_search_plaid, eng.bank_search_plaid_ivf):
            got = entry(F, q, k, ncells=Cn, centroid_score_threshold=0.45, ndocs=1024)
            torch.cuda.synchronize()
            # (the passage without an unmasked row is no candidate; its exact score, Lq * -9999, ranks last: k = 200 leaves it out)
            cnt = got["counts"].tolist()
            assert cnt == [min(k, n - 1)] * 2
            for qi, cn in enumerate(cnt):
                assert torch.equal(got["indices"][qi, :cn], want["indices"][qi, :cn]) and torch.equal(got["scores"][qi, :cn], want["scores"][qi, :cn])


# ---- 5. the inverted file -----------------------------------------------------------------------------------------------------------
def test_inverted_file_build_extend_and_load():
    c = _case(128)
    eng, codec, F, P = c["eng"], c["codec"], c["F"], c["P"]
    F.build_ivf()
    P.build_ivf()
    off, pids = ivf_lib(c["codes"], c["mask"], c["lens"], N_CENTROIDS)
    off2, pids2 = ivf_fast(c["codes"], c["mask"], c["lens"], N_CENTROIDS)
    assert np.array_equal(off, off2) and np.array_equal(pids, pids2)
    want = (pids.astype(np.int32).tobytes(), np.diff(off).astype(np.int64).tobytes())
    assert _ivf_bytes(F) == want and _ivf_bytes(P) == want
    assert F.ivf_info() == dict(passages_covered=PASSAGES, postings=len(pids), longest_list=int(np.diff(off).max()))
    # a bank of its own for what changes it: add, extend == a fresh build
    lens = c["lens"]
    more = _corpus(codec.centroids, [5, 1, 40, 17, 2, 9, 33], seed=99, calls=1)
    more = [([f"m{i}" for i in range(7)],) + more[0][1:]]
    G = _fill(eng.create_bank(sum(lens) + 200, PASSAGES + 8, centroids=codec.centroids), c["corpus"])
    G.build_ivf()
    _fill(G, more)
    assert G.ivf_info()["passages_covered"] == PASSAGES and len(G) == PASSAGES + 7
    assert G.extend_ivf()["passages_covered"] == PASSAGES + 7
    extended = _ivf_bytes(G)
    assert G.build_ivf()["passages_covered"] == PASSAGES + 7 and _ivf_bytes(G) == extended
    rows, mask = _rows_of(G)
    goff, gpids = ivf_lib(_codes_of(G), mask, lens + more[0][3], N_CENTROIDS)
    assert extended == (gpids.astype(np.int32).tobytes(), np.diff(goff).astype(np.int64).tobytes())
    # load: the bytes back in (verified), then one corrupted list
    pair = G.ivf()
    fresh = _fill(_fill(eng.create_bank(sum(lens) + 200, PASSAGES + 8, centroids=codec.centroids), c["corpus"]), more)
    assert fresh.load_ivf(pair, verify=True)["passages_covered"] == PASSAGES + 7 and _ivf_bytes(fresh) == extended
    bad = pair[0].clone()
    lengths = pair[1]
    lst = int(torch.nonzero(lengths >= 2)[0])
    at = int(lengths[:lst].sum())
    present = set(bad[at:at + int(lengths[lst])].tolist())
    bad[at + int(lengths[lst]) - 1] = next(p for p in range(PASSAGES + 6, -1, -1) if p not in present and p > int(bad[at + int(lengths[lst]) - 2]))
    with pytest.raises(ValueError, match="not the inverted file"):
        fresh.load_ivf((bad, lengths), verify=True)
    assert _ivf_bytes(fresh) == extended, "a refused file leaves the bank's own"


# ---- 6. remove ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["every_other", "middle_block", "first", "all_but_one"])
def test_remove_moves_rows_codes_and_mask_together(name):
    c = _case(128)
    eng, codec, corpus, lens, q = c["eng"], c["codec"], c["corpus"], c["lens"], c["q"]
    G = _fill(eng.create_bank(sum(lens), PASSAGES, centroids=codec.centroids), corpus)
    G.build_ivf()
    gone = RC.removal_set(name, PASSAGES)
    keep = [p for p in range(PASSAGES) if p not in set(gone)]
    r = G.remove([f"p{p}" for p in gone])
    assert r["passages"] == len(keep) and r["rows_freed"] == sum(lens[p] for p in gone)
    first = np.concatenate([[0], np.cumsum(lens)])
    pick = np.concatenate([np.arange(first[p], first[p + 1]) for p in keep])
    rows, mask = _rows_of(G)
    assert G.table.ids == [f"p{p}" for p in keep]
    assert torch.equal(rows.view(torch.int16), c["rows"][pick].view(torch.int16)) and np.array_equal(mask, c["mask"][pick])
    assert np.array_equal(_codes_of(G), c["codes"][pick])
    # a fresh coded bank of the survivors, filled in one add
    Lc = max(lens[p] for p in keep)
    x, m = torch.zeros(len(keep), Lc, 128), torch.zeros(len(keep), Lc)
    half = len(corpus[0][0])
    for i, p in enumerate(keep):
        _, cx, cm, _ = corpus[p // half]
        x[i, :lens[p]], m[i, :lens[p]] = cx[p % half, :lens[p]], cm[p % half, :lens[p]]
    fresh = eng.create_bank(sum(lens), PASSAGES, centroids=codec.centroids)
    fresh.add([f"p{p}" for p in keep], x, m, lengths=[lens[p] for p in keep])
    fresh.build_ivf()
    assert np.array_equal(_codes_of(fresh), c["codes"][pick])
    assert G.ivf_info() == fresh.ivf_info() and _ivf_bytes(G) == _ivf_bytes(fresh)
    k = min(NDOCS // 4, len(keep))
    for entry in (eng.bank_search_plaid, eng.bank_search_plaid_ivf):
        a, b = entry(G, q, k, **SEARCH), entry(fresh, q, k, **SEARCH)
        torch.cuda.synchronize()
        for key in ("indices", "scores", "counts"):
            assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), (entry.__name__, key)
    G.clear()
    assert len(G) == 0 and G.ivf_info()["passages_covered"] == 0 and G.n_centroids == N_CENTROIDS
    _fill(G, corpus[:1])
    assert np.array_equal(_codes_of(G), c["codes"][:sum(corpus[0][3])]), "the table outlives rr_bank_clear"


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_say_why():
    L, lib = _L()
    c = _case(128)
    eng, codec, F, P, N, q = c["eng"], c["codec"], c["F"], c["P"], c["N"], c["q"]
    cen = codec.centroids
    err = lambda b: lib.rr_bank_last_error(b.h).decode()

    def state(b):
        return (b.info(), b.format(), b.ivf_info(), _codes_of(b).tobytes() if b.n_centroids else b"")
    F.build_ivf()
    before = {id(b): state(b) for b in (F, P, N)}
    # rr_bank_set_centroids: a compressed bank; 0 and 262145 centroids; a capturing stream
    assert lib.rr_bank_set_centroids(P.h, cen.data_ptr(), N_CENTROIDS, _st()) == L.RR_ERR_UNSUPPORTED
    assert err(P) == "rr_bank_set_centroids on a compressed bank: its codes belong to its residuals (rr_bank_create_plaid)"
    with pytest.raises(NotImplementedError):
        P.set_centroids(cen)
    for bank in (F, N):
        for bad in (0, 262145):
            assert lib.rr_bank_set_centroids(bank.h, cen.data_ptr(), bad, _st()) == L.RR_ERR_BAD_SHAPE
            assert err(bank) == f"rr_bank_set_centroids: n_centroids={bad} (1..262144)"
        assert lib.rr_bank_set_centroids(bank.h, None, 5, _st()) == L.RR_ERR_BAD_ARG
    with pytest.raises(ValueError):
        N.set_centroids(cen[:, :64])
    st = torch.cuda.Stream()
    probe = torch.zeros(1, device="cuda")
    got = {}
    with torch.cuda.stream(st):
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            probe.add_(1.0)
            for name, bank in (("F", F), ("N", N)):
                got[name] = (lib.rr_bank_set_centroids(bank.h, cen.data_ptr(), N_CENTROIDS, st.cuda_stream), err(bank))
        graph.replay()
        torch.cuda.synchronize()
    says = "rr_bank_set_centroids cannot be captured into a graph (it allocates, copies from host memory and synchronises)"
    assert got == {"F": (L.RR_ERR_BAD_ARG, says), "N": (L.RR_ERR_BAD_ARG, says)} and probe.item() == 1.0
    # no residuals: the export and the stored form
    doclens, R_ = np.full(4, -7, dtype=np.int32), C.c_int64(-7)
    assert lib.rr_bank_export_plaid(F.h, 0, 4, doclens.ctypes.data, None, None, 0, C.byref(R_), _st()) == L.RR_ERR_UNSUPPORTED
    assert "no residuals" in err(F) and (doclens == -7).all() and R_.value == -7
    codes = torch.full((64,), -7, dtype=torch.int32)
    assert lib.rr_bank_read_plaid(F.h, 0, codes.data_ptr(), None, None, 64, _st()) == L.RR_ERR_UNSUPPORTED
    assert "no residuals" in err(F) and (codes == -7).all()
    for call in (F.export_compressed, lambda: F.save_plaid_index("/nonexistent/never-written"), lambda: F.read_compressed("p0")):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(NotImplementedError, match="add_compress"):
        F.save_plaid_index("/nonexistent/never-written")
    # the adds a coded bank keeps refusing, as any fp16 bank
    x, ones, one = torch.randn(1, 8, 128).cuda(), torch.ones(1, 8).cuda(), np.array([8], dtype=np.int32)
    first = C.c_int32(-7)
    assert lib.rr_bank_add_compress(F.h, x.data_ptr(), L.RR_F32, ones.data_ptr(), one.ctypes.data, 1, 8, C.byref(first), _st()) == L.RR_ERR_UNSUPPORTED
    assert lib.rr_bank_add_plaid(F.h, codes.data_ptr(), codes.data_ptr(), None, one.ctypes.data, 1, C.byref(first), _st()) == L.RR_ERR_UNSUPPORTED
    assert first.value == -7
    # a plain fp16 bank, still: every pruned entry, the inverted file, the codes
    gi = torch.full((3, 4), -7, device="cuda", dtype=torch.int32)
    gs = torch.full((3, 4), -7.0, device="cuda")
    gc = torch.full((3,), -7, device="cuda", dtype=torch.int32)
    bits = torch.full((1, (PASSAGES + 31) // 32), -1, device="cuda", dtype=torch.int32)
    for entry in ("rr_bank_search_plaid", "rr_bank_search_plaid_ivf", "rr_bank_search_plaid_filtered", "rr_bank_search_plaid_ivf_filtered"):
        extra = [bits.data_ptr(), 1, bits.shape[1]] if entry.endswith("filtered") else []
        rc = getattr(lib, entry)(eng.h, N.h, q.data_ptr(), 3, q.shape[1], q.shape[1], 0, -1, 2, 0.3, 16, 4, *extra, gi.data_ptr(), gs.data_ptr(),
                                 gc.data_ptr(), _st())
        assert rc == L.RR_ERR_UNSUPPORTED
        assert lib.rr_last_error(eng.h).decode() == f"{entry}: an fp16 bank (compressed banks only: the stages read the centroid codes)"
    torch.cuda.synchronize()
    assert (gi == -7).all() and (gs == -7.0).all() and (gc == -7).all()
    assert lib.rr_bank_build_ivf(N.h, _st()) == L.RR_ERR_UNSUPPORTED and err(N) == "rr_bank_build_ivf on an fp16 bank: it holds no codes"
    assert lib.rr_bank_extend_ivf(N.h, _st()) == L.RR_ERR_UNSUPPORTED and err(N) == "rr_bank_extend_ivf on an fp16 bank: it holds no codes"
    off = np.zeros(N_CENTROIDS + 1, dtype=np.int64)
    assert lib.rr_bank_load_ivf(N.h, off.ctypes.data, None, 1, _st()) == L.RR_ERR_UNSUPPORTED
    assert lib.rr_bank_read_codes(N.h, 0, codes.data_ptr(), 64, _st()) == L.RR_ERR_UNSUPPORTED and (codes == -7).all()
    assert "rr_bank_set_centroids" in err(N)
    assert lib.rr_bank_read_codes(F.h, PASSAGES, codes.data_ptr(), 64, _st()) == L.RR_ERR_BAD_SHAPE
    assert lib.rr_bank_read_codes(F.h, 0, None, 0, _st()) == c["lens"][0]
    for call in (N.build_ivf, N.extend_ivf, lambda: N.codes("p0"), lambda: N.search(eng, q, 4, plaid=_plaid())):
        with pytest.raises(NotImplementedError):
            call()
    assert {id(b): state(b) for b in (F, P, N)} == before


# ---- 8. Python ----------------------------------------------------------------------------------------------------------------------
def _plaid(ivf=False):
    from rmr_amd import PlaidSearch
    return PlaidSearch(SEARCH["ncells"], SEARCH["centroid_score_threshold"], SEARCH["ndocs"], ivf=ivf)


def test_the_python_surface_returns_the_same_lists():
    from rmr_amd import InteractionRerankModel, search_banks
    c = _case(64)
    eng, g = _golden_engine("int_tiny")
    assert eng is c["eng"]
    F, P, q, exact, k = c["F"], c["P"], c["q"], c["exact"], NDOCS // 4
    allowed = [pid for i, pid in enumerate(F.table.ids) if i % 3 != 2]
    plain, filtered = _four_entries(eng, F, P, q, exact, k, allowed, **SEARCH)
    name = lambda lists: [[f"p{p}" for p in row] for row in lists]
    for ivf in (False, True):
        ids, scores = F.search(eng, q, k, plaid=_plaid(ivf))
        assert ids == name(plain)
        ids, _ = F.search(eng, q, k, plaid=_plaid(ivf), filter=F.filter(allowed=allowed))
        assert ids == name(filtered)
    model = InteractionRerankModel.__new__(InteractionRerankModel)
    model.engine, model.bank = eng, F
    ids, _ = model.retrieve(q, k, plaid=_plaid(), allowed=allowed)
    assert ids == name(filtered)
    ids, _ = model.retrieve(q, k, plaid=_plaid(ivf=True))
    assert ids == name(plain)
    # two coded banks searched as one: by definition the merge of the two pruned searches
    A, B = _two_halves(eng, c)
    merged, ms, mc = search_banks(eng, [A, B], q, k, plaid=_plaid())
    torch.cuda.synchronize()
    half = len(A)
    for qi, row in enumerate(merged):
        pos = [int(p[1:]) for p in row]
        assert np.array_equal(ms[qi, :len(row)].cpu().numpy().view(np.int32), exact[qi][pos].view(np.int32)) and pos == R.order(exact[qi], pos)
        parts = [eng.bank_search_plaid(bk, q, min(k, len(bk)), **SEARCH) for bk in (A, B)]
        pool = [int(i) + o for r, o in zip(parts, (0, half)) for i in r["indices"][qi, :int(r["counts"][qi])].tolist()]
        assert pos == R.order(exact[qi], pool)[:k]
    with pytest.raises(NotImplementedError, match="add_compress"):
        F.save_plaid_index("/nonexistent/never-written")


def _two_halves(eng, c):
    """The corpus of _case as two coded banks, one per add."""
    codec, corpus = c["codec"], c["corpus"]
    return [_fill(eng.create_bank(sum(part[3]) + 8, len(part[0]) + 1, centroids=codec.centroids), [part]) for part in corpus]


def _shard_worker(rank, world, port, out):
    import datetime
    import os

    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    try:
        from rmr_amd.sharding import ShardedBank
        c = _case(64)
        eng = c["eng"]
        bank = _two_halves(eng, c)[rank]
        shard = ShardedBank(bank)
        shard.refresh()
        ids, scores, counts, parts = shard.search(eng, c["q"], NDOCS // 4, plaid=_plaid())
        out.put((rank, ids, scores.cpu().numpy().tobytes(), counts.tolist(), parts.tolist()))
    finally:
        dist.destroy_process_group()


def test_a_sharded_coded_bank_is_the_merge_of_its_parts():
    """gloo, world 2, one coded bank per rank: every rank gets what search_banks gives over the two banks in one process."""
    from rmr_amd import search_banks
    c = _case(64)
    eng, q, k = c["eng"], c["q"], NDOCS // 4
    A, B = _two_halves(eng, c)
    want_ids, want_scores, want_counts = search_banks(eng, [A, B], q, k, plaid=_plaid())
    torch.cuda.synchronize()
    res = _run_world(_shard_worker, 2, ())
    for rank, ids, scores, counts, parts in res:
        assert ids == want_ids and scores == want_scores.cpu().numpy().tobytes() and counts == want_counts.tolist(), f"rank {rank}"
        for row, prow in zip(ids, parts):
            assert [int(int(p[1:]) >= len(A)) for p in row] == prow[:len(row)]
