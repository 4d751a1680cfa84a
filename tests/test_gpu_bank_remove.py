"""GPU: rr_bank_remove ("REMOVING PASSAGES", include/rerank_mi355.h; PassageBank.remove).  One contract: a bank that has had passages
removed is indistinguishable from a fresh bank filled with the survivors in their original order.  Every case builds bank A with
all passages and bank B fresh from the survivors, removes from A, and compares what the library offers to look at a bank with:
info, read / read_compressed of every survivor, export_compressed, the inverted file, bank_li_scores and the searches.  Bits
only (torch.equal); no tolerance anywhere.  The default staging block holds every case in one window; bank_move_kb = 4 cuts
them into many (at D = 512 a window holds four rows).  A handle's li_dim is a multiple of 64, so no bank has 16-byte fp16 rows
(D = 8) or 1-byte residual rows (D = 8, nbits = 1): those two shapes run the same plan, kernel and copies on raw arrays through
rr_op_bank_move_rows and are compared with a gather of the survivors' rows."""
import numpy as np
import pytest
import torch

from bank_remove_cases import GPU_LENGTHS, GPU_REMOVAL_SETS, removal_set
from test_gpu_bank_li_scores import _queries
from test_gpu_bank_search_plaid import _codec, _near_queries, _topic_rows
from test_gpu_li_scores import _engine as _bare_engine

pytestmark = pytest.mark.gpu

N = 40
LENS = [GPU_LENGTHS[i % len(GPU_LENGTHS)] for i in range(N)]
IDS = [f"p{i}" for i in range(N)]
DEFAULT_KB = 262144


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _masks(lens):
    """Interior zeros in every third passage of three rows or more; first and last row always count (no passage exports empty)."""
    masks = [torch.ones(ln, dtype=torch.uint8) for ln in lens]
    for i, m in enumerate(masks):
        if i % 3 == 1 and len(m) >= 3:
            m[1:-1:2] = 0
    return masks


def _bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == torch.float16 else t


def _shifts(lens, new_index):
    """Per survivor, the rows its first row moved down by."""
    first = np.concatenate([[0], np.cumsum(lens)])
    keep = [p for p in range(len(lens)) if new_index[p] >= 0]
    new_first = np.concatenate([[0], np.cumsum([lens[p] for p in keep])])
    return [int(first[p] - new_first[new_index[p]]) for p in keep]


def _want_index(n, remove):
    gone = set(remove)
    want = np.full(n, -1, dtype=np.int32)
    want[[p for p in range(n) if p not in gone]] = np.arange(n - len(gone))
    return want


class _Window:
    """bank_move_kb set for a block, the default restored behind it."""

    def __init__(self, eng, kb):
        self.eng, self.kb = eng, kb

    def __enter__(self):
        assert self.eng.lib.rr_set_tuning(b"bank_move_kb", self.kb) == 0

    def __exit__(self, *exc):
        assert self.eng.lib.rr_set_tuning(b"bank_move_kb", DEFAULT_KB) == 0


def test_the_tunable_has_a_range():
    eng = _bare_engine(64)
    try:
        for bad in (3, 0, -1, (1 << 20) + 1):
            assert eng.lib.rr_set_tuning(b"bank_move_kb", bad) != 0
        for good in (4, 1 << 20):
            assert eng.lib.rr_set_tuning(b"bank_move_kb", good) == 0
    finally:
        assert eng.lib.rr_set_tuning(b"bank_move_kb", DEFAULT_KB) == 0


# ---- rows no handle's li_dim gives (a handle takes multiples of 64): the kernel on raw arrays ------------------------------------------
def _moved_raw(arrays, remove, kb):
    """rr_op_bank_move_rows (rr_bank_remove's plan, kernel and copies) on each of `arrays` ([rows, ...] device tensors over the
    passages of LENS); each must then hold the survivors' rows back to back."""
    from rmr_amd import _lib as L
    lib = L.load()
    lens = np.ascontiguousarray(LENS, dtype=np.int32)
    rem = np.ascontiguousarray(remove, dtype=np.int32)
    first = np.concatenate([[0], np.cumsum(LENS)])
    gone = set(remove)
    keep_rows = [torch.arange(first[p], first[p + 1]) for p in range(N) if p not in gone]
    keep_rows = torch.cat(keep_rows).cuda() if keep_rows else torch.zeros(0, dtype=torch.long, device="cuda")
    for t in arrays:
        assert t.is_contiguous() and t.shape[0] == sum(LENS)
        want = t[keep_rows].clone()
        row_bytes = t[0].numel() * t.element_size()
        assert lib.rr_set_tuning(b"bank_move_kb", kb) == 0
        try:
            rc = lib.rr_op_bank_move_rows(L.ptr(t), row_bytes, lens.ctypes.data, N, rem.ctypes.data if rem.size else None, len(rem), _stream())
        finally:
            assert lib.rr_set_tuning(b"bank_move_kb", DEFAULT_KB) == 0
        assert rc == 0
        got = t[:len(keep_rows)]
        assert torch.equal(_bits(got), _bits(want)), f"{row_bytes}-byte rows"


# ---- 1. fp16 banks ----------------------------------------------------------------------------------------------------------------
_FP16 = {}


def _fp16_rows(D):
    if D not in _FP16:
        gen = torch.Generator().manual_seed(100 + D)
        li = torch.nn.functional.normalize(torch.randn(N, max(LENS), D, generator=gen), dim=-1).half()
        cm = torch.zeros(N, max(LENS))
        for i, m in enumerate(_masks(LENS)):
            cm[i, :LENS[i]] = m.float()
        _FP16[D] = (li.cuda(), cm.cuda())
    return _FP16[D]


def _fp16_bank(eng, D, keep, rows=None, slots=None):
    li, cm = _fp16_rows(D)
    bank = eng.create_bank(sum(LENS) + 4 if rows is None else rows, N + 1 if slots is None else slots)
    if keep:
        idx = torch.tensor(keep, device="cuda")
        bank.add([IDS[p] for p in keep], li[idx], cm[idx], lengths=[LENS[p] for p in keep])
    return bank


def _exact_order(eng, bank, q):
    r = eng.bank_search(bank, q, len(bank))
    torch.cuda.synchronize()
    return r["indices"].cpu(), r["scores"].cpu()


@pytest.mark.parametrize("kb", [DEFAULT_KB, 4])
@pytest.mark.parametrize("which", GPU_REMOVAL_SETS)
@pytest.mark.parametrize("D", [8, 64, 512])
def test_fp16_bank_equals_a_fresh_bank_of_the_survivors(D, which, kb):
    remove = removal_set(which, N)
    if D == 8:                                    # 16-byte rows: a one-row removal shifts everything by 16 bytes; no handle has this li_dim
        gen = torch.Generator().manual_seed(108)
        return _moved_raw([torch.randn(sum(LENS), D, generator=gen).half().cuda()], remove, kb)
    eng = _bare_engine(D)
    keep = [p for p in range(N) if p not in set(remove)]
    A, B = _fp16_bank(eng, D, list(range(N))), _fp16_bank(eng, D, keep)
    q = _queries(2, 9, D, seed=31)
    before = _exact_order(eng, A, q)
    with _Window(eng, kb):
        got = A.remove([IDS[p] for p in remove])
    new_index = got["new_index"]
    assert np.array_equal(new_index, _want_index(N, remove)) and new_index.dtype == np.int32
    assert got["passages"] == len(keep) and got["rows_freed"] == sum(LENS[p] for p in remove)
    assert A.info() == B.info() and len(A) == len(B) == len(keep) and A.table.ids == B.table.ids
    assert A.generation == (1 if remove else 0)
    if which == "first":
        assert set(_shifts(LENS, new_index)) == {1}, "a one-row removal: everything moves by one row"
    for p in remove:
        assert IDS[p] not in A
    for p in keep:
        (ra, ma), (rb, mb) = A.read(IDS[p]), B.read(IDS[p])
        assert torch.equal(_bits(ra), _bits(rb)) and torch.equal(ma, mb), f"passage {p}"
    if keep:
        ids = [IDS[p] for p in keep] * 2
        pq = [0] * len(keep) + [1] * len(keep)
        sa = eng.bank_li_scores(A, q, ids, pair_query=pq, want_scores=True)
        sb = eng.bank_li_scores(B, q, ids, pair_query=pq, want_scores=True)
        torch.cuda.synchronize()
        assert torch.equal(sa["maxsim"].view(torch.int32), sb["maxsim"].view(torch.int32))
        assert torch.equal(sa["scores"].view(torch.int32), sb["scores"].view(torch.int32))
        ia, xa = _exact_order(eng, A, q)
        ib, xb = _exact_order(eng, B, q)
        assert torch.equal(ia, ib) and torch.equal(xa.view(torch.int32), xb.view(torch.int32))
        # the order over all N passages from before the removal, mapped through new_index, is the survivors' order
        mapped = torch.from_numpy(new_index)[before[0].long()]
        for row, want in zip(mapped, ib):
            assert torch.equal(row[row >= 0], want)
    A.close()
    B.close()


# ---- 2. compressed banks ----------------------------------------------------------------------------------------------------------
_PLAID = {}
C_CENTROIDS = 16


def _plaid_rows(D, nbits):
    if (D, nbits) not in _PLAID:
        codec = _codec(D, nbits, C_CENTROIDS)
        codes, res = _topic_rows(codec, LENS, seed=7 + D)
        first = np.concatenate([[0], np.cumsum(LENS)])
        _PLAID[D, nbits] = (codec, codes, res, torch.cat(_masks(LENS)), first)
    return _PLAID[D, nbits]


def _plaid_bank(eng, D, nbits, keep, extra_rows=4, masked=True, codec=None):
    own, codes, res, mask, first = _plaid_rows(D, nbits)
    codec = own if codec is None else codec
    bank = eng.create_bank(sum(LENS) + extra_rows, N + 1, codec=codec)
    if keep:
        rows = torch.cat([torch.arange(first[p], first[p + 1]) for p in keep])
        bank.add_compressed([IDS[p] for p in keep], codes[rows], res[rows], [LENS[p] for p in keep], mask=mask[rows] if masked else None)
    return bank


def _same_compressed(A, B, keep):
    assert A.info() == B.info() and A.table.ids == B.table.ids
    for p in keep:
        for a, b in zip(A.read_compressed(IDS[p]), B.read_compressed(IDS[p])):
            assert torch.equal(a, b), f"passage {p}"
    if keep:
        (ca, ra, da), (cb, rb, db) = A.export_compressed(), B.export_compressed()
        assert list(da) == list(db) and torch.equal(ca, cb) and torch.equal(ra, rb)


def _same_ivf(A, B):
    assert A.ivf_info() == B.ivf_info()
    (pa, la), (pb, lb) = A.ivf(), B.ivf()
    assert torch.equal(pa, pb) and torch.equal(la, lb)


def _same_searches(eng, A, B, q, count=None, ivf=True):
    from rmr_amd import PlaidSearch
    n = len(B) if count is None else count
    k = min(8, n)
    for plaid in [None, PlaidSearch(2, 0.3, 32)] + ([PlaidSearch(2, 0.3, 32, ivf=True)] if ivf else []):
        kk = n if plaid is None else k
        (ia, sa), (ib, sb) = A.search(eng, q, kk, count=count, plaid=plaid), B.search(eng, q, kk, count=count, plaid=plaid)
        assert ia == ib and torch.equal(sa.view(torch.int32), sb.view(torch.int32)), f"{plaid}"


@pytest.mark.parametrize("kb", [DEFAULT_KB, 4])
@pytest.mark.parametrize("which", GPU_REMOVAL_SETS)
@pytest.mark.parametrize("D,nbits", [(128, 8), (64, 2), (8, 1)])     # residual rows of 128, 16 and 1 byte
def test_compressed_bank_equals_a_fresh_bank_of_the_survivors(D, nbits, which, kb):
    if D == 8:                                    # 1-byte residual rows; no handle has this li_dim: the three arrays through the kernel
        gen = torch.Generator().manual_seed(81)
        R = sum(LENS)
        return _moved_raw([torch.randint(0, 256, (R, 1), generator=gen, dtype=torch.uint8).cuda(),
                           torch.randint(0, 1 << 20, (R,), generator=gen, dtype=torch.int32).cuda(), torch.cat(_masks(LENS)).cuda()],
                          removal_set(which, N), kb)
    eng = _bare_engine(D)
    codec = _plaid_rows(D, nbits)[0]
    assert codec.residual_bytes == {(128, 8): 128, (64, 2): 16}[D, nbits]
    remove = removal_set(which, N)
    keep = [p for p in range(N) if p not in set(remove)]
    A, B = _plaid_bank(eng, D, nbits, list(range(N))), _plaid_bank(eng, D, nbits, keep)
    assert A.build_ivf()["passages_covered"] == N
    with _Window(eng, kb):
        got = A.remove([IDS[p] for p in remove])
    new_index = got["new_index"]
    assert np.array_equal(new_index, _want_index(N, remove))
    assert got["passages"] == len(keep) and got["rows_freed"] == sum(LENS[p] for p in remove)
    # the misaligned cases of the 4-byte codes and the mask bytes: shifts of 1, 3 and 17 rows
    want_shift = {"first": 1, "second": 3, "third": 17}.get(which)
    if want_shift:
        assert set(_shifts(LENS, new_index)[new_index[remove[0] + 1]:]) == {want_shift}
    _same_compressed(A, B, keep)
    if not keep:
        assert A.ivf_info()["passages_covered"] == 0 and A.info()["rows_used"] == 0
    else:
        B.build_ivf()
        _same_ivf(A, B)
        _same_searches(eng, A, B, _near_queries(codec, 2, 9, seed=41))
    A.close()
    B.close()


# ---- 3. the inverted file covers a prefix -----------------------------------------------------------------------------------------
def test_inverted_file_over_a_prefix_follows_its_survivors():
    from rmr_amd import PlaidSearch
    D, nbits, covered = 64, 2, 24
    eng = _bare_engine(D)
    codec, codes, res, mask, first = _plaid_rows(D, nbits)
    A = _plaid_bank(eng, D, nbits, list(range(covered)))
    A.build_ivf()
    rows = torch.arange(first[covered], first[N])
    A.add_compressed(IDS[covered:], codes[rows], res[rows], LENS[covered:], mask=mask[rows])
    remove = [3, 30, 11, 39, 12]
    keep = [p for p in range(N) if p not in remove]
    keep_cov = [p for p in keep if p < covered]
    A.remove([IDS[p] for p in remove])
    B = _plaid_bank(eng, D, nbits, keep_cov)
    B.build_ivf()
    assert A.ivf_info()["passages_covered"] == len(keep_cov) == covered - 3
    _same_ivf(A, B)
    rows = torch.cat([torch.arange(first[p], first[p + 1]) for p in keep if p >= covered])
    B.add_compressed([IDS[p] for p in keep if p >= covered], codes[rows], res[rows], [LENS[p] for p in keep if p >= covered], mask=mask[rows])
    _same_compressed(A, B, keep)
    q = _near_queries(codec, 2, 9, seed=43)
    _same_searches(eng, A, B, q, count=len(keep_cov))
    _same_searches(eng, A, B, q, ivf=False)
    with pytest.raises(NotImplementedError):                       # beyond the file, as before
        A.search(eng, q, 4, plaid=PlaidSearch(2, 0.3, 32, ivf=True))
    # a removal behind the covered prefix leaves the file as it is; one that takes the whole prefix drops it
    A.remove([IDS[keep[-1]]])
    _same_ivf(A, B)
    A.remove([IDS[p] for p in keep_cov])
    assert A.ivf_info()["passages_covered"] == 0 and len(A) == len(keep) - 1 - len(keep_cov)
    A.close()
    B.close()


# ---- 4. capacity comes back ---------------------------------------------------------------------------------------------------------
def test_rows_and_passage_slots_come_back():
    D = 64
    eng = _bare_engine(D)
    li, cm = _fp16_rows(D)
    extra = torch.nn.functional.normalize(torch.randn(1, 64, D, generator=torch.Generator().manual_seed(3)), dim=-1).half().cuda()
    ones = torch.ones(1, 64, device="cuda")
    for rows, slots in ((sum(LENS), N + 5), (sum(LENS) + 500, N)):          # full in rows; full in passage slots
        bank = _fp16_bank(eng, D, list(range(N)), rows=rows, slots=slots)
        before = bank.info()
        with pytest.raises(MemoryError):
            bank.add(["new"], extra, ones, lengths=[64])
        assert bank.info() == before and "new" not in bank
        got = bank.remove([IDS[3]])                                         # 64 rows and one slot
        assert got["rows_freed"] == 64 and LENS[3] == 64
        assert bank.add(["new"], extra, ones, lengths=[64]) == N - 1
        r, m = bank.read("new")
        assert torch.equal(_bits(r), _bits(extra[0].cpu())) and bool(m.all())
        r, m = bank.read(IDS[N - 1])
        assert torch.equal(_bits(r), _bits(li[N - 1, :LENS[N - 1]].cpu()))
        assert bank.info()["passages"] == N and bank.info()["rows_used"] == sum(LENS)
        bank.remove(["new"])
        assert bank.add([IDS[3]], li[3:4], cm[3:4], lengths=[64]) == N - 1, "a removed id may come back"
        r, m = bank.read(IDS[3])
        assert torch.equal(_bits(r), _bits(li[3, :64].cpu())) and torch.equal(m, (cm[3, :64] != 0).to(torch.uint8).cpu())
        bank.close()


# ---- 5. refusals change nothing -----------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    from rmr_amd import _lib as L
    D, nbits = 64, 2
    eng = _bare_engine(D)
    A = _plaid_bank(eng, D, nbits, list(range(N)))
    A.build_ivf()

    def state():
        return A.info(), [tuple(t.clone() for t in A.read_compressed(i)) for i in IDS], A.ivf(), A.ivf_info(), list(A.table.ids), A.generation

    def same(x, y):
        assert x[0] == y[0] and x[3:] == y[3:] and torch.equal(x[2][0], y[2][0]) and torch.equal(x[2][1], y[2][1])
        for a, b in zip(x[1], y[1]):
            assert all(torch.equal(s, t) for s, t in zip(a, b))

    before = state()
    out = np.full(N, -7, dtype=np.int32)

    def raw(indices, n=None, stream=None):
        idx = np.ascontiguousarray(indices, dtype=np.int32)
        return eng.lib.rr_bank_remove(A.h, idx.ctypes.data if idx.size else None, len(idx) if n is None else n, out.ctypes.data,
                                      _stream() if stream is None else stream)

    assert raw([5, 9, 5]) == L.RR_ERR_BAD_SHAPE and b"index 5 is given twice" in eng.lib.rr_bank_last_error(A.h)
    assert raw([5, N]) == L.RR_ERR_BAD_SHAPE and f"index {N} ".encode() in eng.lib.rr_bank_last_error(A.h)
    assert raw([-1]) == L.RR_ERR_BAD_SHAPE and b"index -1 " in eng.lib.rr_bank_last_error(A.h)
    assert raw([1], n=-1) == L.RR_ERR_BAD_SHAPE
    assert raw([], n=2) == L.RR_ERR_BAD_ARG
    assert eng.lib.rr_bank_remove(None, None, 0, None, _stream()) == L.RR_ERR_BAD_ARG
    probe = torch.zeros(1, device="cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            probe.add_(1.0)                                                  # the graph holds this node alone
            rc = raw([4], stream=torch.cuda.current_stream().cuda_stream)
            msg = eng.lib.rr_bank_last_error(A.h)
        graph.replay()
        torch.cuda.synchronize()
    assert rc == L.RR_ERR_BAD_ARG and b"captured" in msg and probe.item() == 1.0
    with pytest.raises(KeyError, match="nobody"):
        A.remove([IDS[2], "nobody"])
    with pytest.raises(ValueError, match="twice"):
        A.remove([IDS[2], IDS[7], IDS[2]])
    assert (out == -7).all(), "a refused call writes no map"
    same(before, state())
    assert raw([]) == 0 and out.tolist() == list(range(N)), "n == 0: RR_OK and the identity"
    same(before, state())
    A.close()


# ---- 6. staleness -------------------------------------------------------------------------------------------------------------------
def test_a_filter_from_before_a_removal_is_refused_and_a_saved_index_holds_the_survivors(tmp_path):
    D, nbits = 64, 2
    eng = _bare_engine(D)
    from rmr_amd import PlaidCodec
    base = _plaid_rows(D, nbits)[0]
    codec = PlaidCodec(base.centroids, base.bucket_weights, nbits, bucket_cutoffs=torch.linspace(-0.1, 0.1, (1 << nbits) - 1))   # an index stores them
    remove = removal_set("every_other", N)
    keep = [p for p in range(N) if p not in set(remove)]
    A, B = _plaid_bank(eng, D, nbits, list(range(N)), masked=False, codec=codec), _plaid_bank(eng, D, nbits, keep, masked=False, codec=codec)
    allowed = [IDS[p] for p in keep[::3]]
    stale = A.filter(allowed=allowed)
    q = _near_queries(codec, 2, 9, seed=47)
    A.search(eng, q, 3, filter=stale)
    A.remove([IDS[p] for p in remove])
    with pytest.raises(ValueError, match="build it again"):
        A.search(eng, q, 3, filter=stale)
    (ia, sa), (ib, sb) = A.search(eng, q, 3, filter=A.filter(allowed=allowed)), B.search(eng, q, 3, filter=B.filter(allowed=allowed))
    assert ia == ib and torch.equal(sa.view(torch.int32), sb.view(torch.int32))
    A.build_ivf()
    A.save_plaid_index(str(tmp_path / "index"))
    from rmr_amd import read_plaid_index
    Cb = eng.create_bank(sum(LENS) + 4, N + 1, codec=read_plaid_index(str(tmp_path / "index"))[0])
    assert Cb.load_plaid_index(str(tmp_path / "index"), ivf=True) == len(keep)
    _same_compressed(Cb, B, keep)
    B.build_ivf()
    _same_ivf(Cb, B)
    for b in (A, B, Cb):
        b.close()


# ---- 7. past 4 GiB ------------------------------------------------------------------------------------------------------------------
def test_rows_move_across_byte_2_to_the_32():
    """17 000 zero passages of 1 024 rows of 128 fp16 values fill 4.46 GB; seeded passages behind them.  Passage 0 goes: every later
    row moves down by 1 024 rows, the seeded ones from beyond byte 2^32, across many windows of the default staging block."""
    from test_gpu_large_index import _need
    eng = _bare_engine(128)
    n0, L0, D = 17000, 1024, 128
    big = n0 * L0 * D * 2
    _need(2 * big + n0 * L0 * 5 + (1 << 28))
    gen = torch.Generator().manual_seed(11)
    lens = [130, 1, 64, 17, 3]
    li = torch.nn.functional.normalize(torch.randn(len(lens), 130, D, generator=gen), dim=-1).half().cuda()
    cm = torch.ones(len(lens), 130, device="cuda")
    cm[0, 5:9] = 0
    bank = eng.create_bank(n0 * L0 + sum(lens), n0 + len(lens))
    zeros = torch.zeros([n0, L0, D], dtype=torch.float16, device="cuda")
    bank.add(range(n0), zeros, torch.ones(n0, L0, device="cuda"), lengths=[L0] * n0)
    del zeros
    ids = [f"s{i}" for i in range(len(lens))]
    assert bank.add(ids, li, cm, lengths=lens) == n0 and (bank.info()["rows_used"] - sum(lens) - L0) * D * 2 > 1 << 32
    got = bank.remove([0])
    assert got["rows_freed"] == L0 and got["new_index"][0] == -1 and np.array_equal(got["new_index"][1:], np.arange(n0 + len(lens) - 1))
    assert bank.info()["rows_used"] == (n0 - 1) * L0 + sum(lens)
    for i, pid in enumerate(ids):
        rows, mask = bank.read(pid)
        assert torch.equal(_bits(rows), _bits(li[i, :lens[i]].cpu())) and torch.equal(mask, (cm[i, :lens[i]] != 0).to(torch.uint8).cpu())
    for pid in (1, n0 // 2, n0 - 1):
        rows0, m0 = bank.read(pid)
        assert rows0.shape == (L0, D) and not bool(rows0.view(torch.int16).any()) and bool(m0.all())
    bank.close()
    torch.cuda.empty_cache()
