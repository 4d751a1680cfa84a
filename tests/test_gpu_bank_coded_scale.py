"""GPU: a coded fp16 bank (rr_bank_set_centroids, include/rerank_mi355.h) at real centroid counts, against float64, and its
re-assignment over more than one launch.

tests/test_gpu_bank_coded.py is bitwise against the library's own parts (the host definition of the code, the stage-0 tap,
rr_bank_li_scores, a compressed bank that runs the same stages) at 200 centroids and Lq 8 / 20 / 32.  Here the inputs are the coded
exact cases of tests/coded_exact_cases.py: rows and centroid table on which every row . centroid and every row . token is exact, so
a float64 numpy computation that calls nothing of the library predicts every code (the LOWEST index among thousands of exactly tied
maxima a case, many across index 256), the inverted file, every tap of the pruned search and the result, at C = 257 ... 262 144 and at
every width of stage 3 on fp16 rows: Lq 4 (JT 1), 32 (JT 2), 48 (JT 4), 100 at D 128 (JT 8, one column block) and 130 at D 64 (JT 8,
two blocks with the carry between them).  tests/test_coded_exact_cases_cpu.py shows on the oracle alone that the cases bite: the
oracle cannot be met by a bank that behaves like the compressed bank of the same case.

The last test re-assigns 2^20 + 37 rows: one full launch of rr_bank_set_centroids and a tail of 37 rows whose plan has another
column tile and other splits; row r is a known entry of a pool of exact rows, so a launch that starts at the wrong row is seen.
No tolerance anywhere."""
import numpy as np
import pytest
import torch

import coded_exact_cases as K
from test_gpu_bank_search_plaid import _check_result, _padded
from test_gpu_bank_search_plaid_scale import _same_bits
from test_gpu_li_scores import _engine as _bare_engine

pytestmark = pytest.mark.gpu

_BANKS = {}


def _padded_rows(rows, mask, lens):
    """fp16 [n, Lc, D] and float32 [n, Lc] on the device from rows [R, D] / mask [R] back to back."""
    n, Lc, D = len(lens), max(lens), rows.shape[1]
    x, m = torch.zeros(n, Lc, D, dtype=torch.float16), torch.zeros(n, Lc)
    r0 = 0
    for i, ln in enumerate(lens):
        x[i, :ln], m[i, :ln] = torch.from_numpy(rows[r0:r0 + ln]), torch.from_numpy(mask[r0:r0 + ln].astype(np.float32))
        r0 += ln
    return x.cuda(), m.cuda()


def _banks(name):
    """(engine, bank with the table given at creation, bank filled first and given the table afterwards), built once."""
    if name not in _BANKS:
        case, _, _ = K.get(name)
        eng = _bare_engine(case["D"])
        lens = case["lens"]
        ids = [f"p{i}" for i in range(len(lens))]
        x, m = _padded_rows(case["rows"], case["mask"], lens)
        first = eng.create_bank(sum(lens) + 4, len(lens) + 1, centroids=case["centroids"])
        first.add(ids, x, m, lengths=lens)
        after = eng.create_bank(sum(lens) + 4, len(lens) + 1)
        after.add(ids, x, m, lengths=lens)
        after.set_centroids(case["centroids"])
        _BANKS[name] = (eng, first, after)
    return _BANKS[name]


def _codes_of(bank):
    return torch.cat([bank.codes(pid) for pid in bank.table.ids]).numpy()


def _same_codes(got, want, shared, what):
    bad = np.flatnonzero(got != want)
    tied = "" if shared is None or not bad.size else f"; {int((shared[bad].sum(axis=1) > 1).sum())} of them rows with a tied maximum"
    assert bad.size == 0, f"{what}: {bad.size} of {len(want)} codes differ{tied}, first rows {bad[:6].tolist()}: {got[bad[:6]].tolist()} for {want[bad[:6]].tolist()}"


def _search_and_check(eng, bank, case, want, flt=None):
    """The scan form with every tap and the inverted-file form, against `want`, bit for bit."""
    C, Lqc, ndocs, k, nq, n = case["C"], case["Lqc"], case["ndocs"], case["k"], case["nq"], len(case["lens"])
    q = torch.from_numpy(case["queries"]).cuda()
    k1, k2 = min(ndocs, n), min(ndocs // 4, n)
    kw = dict(ncells=case["ncells"], centroid_score_threshold=case["threshold"], ndocs=ndocs, coarse_tokens=Lqc)
    scan, ivf = (eng.bank_search_plaid, eng.bank_search_plaid_ivf) if flt is None else (eng.bank_search_plaid_filtered, eng.bank_search_plaid_ivf_filtered)
    extra = [] if flt is None else [flt]
    got = scan(bank, q, k, *extra, **kw)
    torch.cuda.synchronize()
    _same_bits(eng.bank_search_plaid_tap("S").reshape(nq, C, Lqc), case["S"][:, :, :Lqc], "S")
    for key in ("cells", "keep"):
        t = eng.bank_search_plaid_tap(key).reshape(nq, C).astype(bool)
        bad = np.argwhere(t != np.stack([w[key] for w in want]))
        assert bad.size == 0, f"{key} differs at (query, centroid) {bad[:6].tolist()}"
    _same_bits(eng.bank_search_plaid_tap("a1").reshape(nq, n), np.stack([w["a1"] for w in want]), "A1")
    l1, l2 = eng.bank_search_plaid_tap("list1").reshape(nq, k1), eng.bank_search_plaid_tap("list2").reshape(nq, k2)
    w1, w2 = _padded([w["list1"] for w in want], k1), _padded([w["list2"] for w in want], k2)
    assert np.array_equal(l1, w1), f"stage-1 list: {l1.tolist()} for {w1.tolist()}"
    assert np.array_equal(l2, w2), f"stage-2 list: {l2.tolist()} for {w2.tolist()}"
    _check_result(got, want, case["exact"], k)
    got = ivf(bank, q, k, *extra, **kw)
    torch.cuda.synchronize()
    _check_result(got, want, case["exact"], k)


@pytest.mark.parametrize("name", K.CASES)
def test_codes_file_and_every_stage_against_float64(name):
    case, want, filtered = K.get(name)
    eng, first, after = _banks(name)
    pids, lengths = K.ivf_of(case)
    allowed = [f"p{i}" for i in np.flatnonzero(~K.every_third(case))]
    for what, bank in (("the table at creation", first), ("the table behind the rows", after)):
        _same_codes(_codes_of(bank), case["codes64"], case["shared"], f"{name}, {what}")
        assert bank.build_ivf()["passages_covered"] == len(case["lens"])
        gp, gl = bank.ivf()
        assert np.array_equal(gl.numpy(), lengths) and gl.dtype == torch.int64, f"{name}, {what}: list lengths"
        assert np.array_equal(gp.numpy(), pids) and gp.dtype == torch.int32, f"{name}, {what}: postings"
        _search_and_check(eng, bank, case, want)
        _search_and_check(eng, bank, case, filtered, flt=bank.filter(allowed=allowed))


# ---- rr_bank_set_centroids over more than one launch ------------------------------------------------------------------------------
POOL_CASE = "c1000"
LAUNCH_ROWS = 1 << 20                                      # SET_CENTROIDS_ROWS of csrc/bank_api.hip
TAIL = 37                                                  # at most 64 rows: the tail's plan has another column tile
PASSAGE_ROWS, ADDS = 128, 4


def test_set_centroids_over_a_full_launch_and_a_tail_of_37_rows():
    case, _, _ = K.get(POOL_CASE)
    D, pool, pool_codes = case["D"], case["rows"], case["codes64"]
    R = LAUNCH_ROWS + TAIL
    pick = ((np.arange(R, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 32) % np.uint64(len(pool))).astype(np.int64)
    want = pool_codes[pick]
    tied = int((case["shared"][pick[LAUNCH_ROWS:]].sum(axis=1) > 1).sum())
    assert len(np.unique(pick[LAUNCH_ROWS:])) == TAIL and tied >= 1, f"the tail: {tied} rows with a tied maximum"
    assert not np.array_equal(want[:TAIL], want[LAUNCH_ROWS:]), "a tail assigned from the rows of the first launch is seen"
    assert not np.array_equal(want[LAUNCH_ROWS - TAIL:LAUNCH_ROWS], want[LAUNCH_ROWS:])
    n_full = LAUNCH_ROWS // PASSAGE_ROWS
    per = n_full // ADDS
    eng = _bare_engine(D)
    after = eng.create_bank(R, n_full + 1)
    first = eng.create_bank(R, n_full + 1, centroids=case["centroids"])
    ones = torch.ones(per, PASSAGE_ROWS, device="cuda")
    for a in range(ADDS):
        x = torch.from_numpy(pool[pick[a * per * PASSAGE_ROWS:(a + 1) * per * PASSAGE_ROWS]]).view(per, PASSAGE_ROWS, D).cuda()
        for bank in (after, first):
            bank.add(range(a * per, (a + 1) * per), x, ones, lengths=[PASSAGE_ROWS] * per)
    x = torch.from_numpy(pool[pick[LAUNCH_ROWS:]]).view(1, TAIL, D).cuda()
    for bank in (after, first):
        bank.add([n_full], x, ones[:1, :TAIL], lengths=[TAIL])
        assert bank.info()["rows_used"] == R and len(bank) == n_full + 1
    del x
    after.set_centroids(case["centroids"])
    _same_codes(_codes_of(after), want, None, "filled first, then rr_bank_set_centroids: two launches")
    _same_codes(_codes_of(first), want, None, "the table at creation: a launch per add")
    # one pruned search, scan and inverted file, on both banks: equal bytes
    q = torch.from_numpy(case["queries"]).cuda()
    kw = dict(ncells=case["ncells"], centroid_score_threshold=case["threshold"], ndocs=case["ndocs"], coarse_tokens=case["Lqc"])
    got = []
    for bank in (after, first):
        assert bank.build_ivf()["passages_covered"] == n_full + 1
        for entry in (eng.bank_search_plaid, eng.bank_search_plaid_ivf):
            r = entry(bank, q, case["k"], **kw)
            torch.cuda.synchronize()
            got.append(tuple(r[key].cpu().numpy().tobytes() for key in ("indices", "scores", "counts")))
            assert (r["counts"] >= 1).all()
    assert got[0] == got[1] == got[2] == got[3], "scan and inverted file, on the two banks"
    pa, pb = after.ivf(), first.ivf()
    assert torch.equal(pa[0], pb[0]) and torch.equal(pa[1], pb[1])
    after.close()
    first.close()
