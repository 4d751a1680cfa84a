"""GPU: the full text of the refusals that the bank entry points share — rr_forward_interaction_bank, rr_bank_li_scores,
rr_bank_search, rr_bank_add, rr_bank_add_plaid and rr_bank_add_compress — and of those of rr_bank_create, rr_bank_create_plaid,
rr_bank_read, rr_bank_read_plaid and rr_bank_set_plaid_cutoffs (include/rerank_mi355.h).

The other bank suites sample these messages by substring; here the return code and the COMPLETE rr_last_error /
rr_bank_last_error string of each is pinned, written out by hand from the format strings of csrc/bank_api.hip, on an fp16 bank and
on an nbits = 2 bank of three passages (2, 5 and 3 rows) with Lq = 4.  Every call is refused on the host before anything is
enqueued: an output buffer a call was handed keeps its sentinel, a bank keeps its contents.

Not pinned: rr_bank_add_compress's "li_dim %d (a multiple of 16 ...)" refusal.  It needs a compressed bank of li_dim 8, the only
li_dim a codec takes that is no multiple of 16, and rr_create takes no li_dim that is not a multiple of 64."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_passage_bank import _engine
from test_gpu_plaid_bank import _codec, _rows

pytestmark = pytest.mark.gpu

LENS = [2, 5, 3]
ROWS, CAP_ROWS, SLOTS = sum(LENS), sum(LENS) + 2, len(LENS) + 1      # two rows and one slot are free
NQ, LQ, LC = 2, 4, 5
POISON, IPOISON = -12345.0, -77
PP, PQ = [0, 1, 2], [0, 1, 1]
CUTOFFS = [-0.05, 0.0, 0.05]
FIB, BLS, SEARCH = "rr_forward_interaction_bank", "rr_bank_li_scores", "rr_bank_search"


class _Setup:
    def __init__(self):
        from rmr_amd import _lib as L
        self.L = L
        self.eng, _ = _engine("int_tiny")                               # li_dim 64
        wide, _ = _engine("int_base")                                   # li_dim 128
        D = self.D = int(self.eng.arch["li_dim"])
        assert D == 64 and int(wide.arch["li_dim"]) == 128
        gen = torch.Generator().manual_seed(7)
        li = torch.nn.functional.normalize(torch.randn(len(LENS), LC, D, generator=gen), dim=-1)
        cm = (torch.arange(LC)[None, :] < torch.tensor(LENS)[:, None]).float()
        ids = [f"p{i}" for i in range(len(LENS))]
        self.fp16 = self.eng.create_bank(CAP_ROWS, SLOTS)
        self.fp16.add(ids, li, cm, lengths=LENS)
        from rmr_amd import PlaidCodec
        bare = self.codec = _codec(D, 2)                                # no cutoffs
        codec = PlaidCodec(bare.centroids, bare.bucket_weights, 2, bucket_cutoffs=torch.tensor(CUTOFFS))
        self.codes, self.res = _rows(codec, ROWS, seed=9)
        self.plaid = self.eng.create_bank(CAP_ROWS, SLOTS, codec=codec)
        self.bare = self.eng.create_bank(CAP_ROWS, SLOTS, codec=bare)   # a compressed bank that cannot compress: empty
        self.plaid.add_compressed(ids, self.codes, self.res, LENS)
        self.other = wide.create_bank(8, 2)                             # a second engine's bank: rows of 128
        # one spare row behind the queries, so that the pointer 4 bytes on still points into the tensor
        self.qbuf = torch.nn.functional.normalize(torch.randn(NQ * LQ + 1, D, generator=gen), dim=-1).cuda()
        self.q = self.qbuf[:NQ * LQ].view(NQ, LQ, D)
        self.qm = torch.ones(NQ, LQ, device="cuda")
        self.logits = [torch.full((len(PP),), POISON, device="cuda") for _ in range(2)]
        self.scores = torch.full((len(PP), LC, LQ), POISON, device="cuda")
        self.maxsim = torch.full((len(PP),), POISON, device="cuda")
        self.top_i = torch.full((NQ, 2), IPOISON, device="cuda", dtype=torch.int32)
        self.top_s = torch.full((NQ, 2), POISON, device="cuda")
        # what a raw rr_bank_add takes: one passage of LC padded rows on the device
        self.add_li = torch.randn(2, LC, D, generator=gen).cuda()
        self.add_cm = torch.ones(2, LC, device="cuda")

    def banks(self):
        return (("fp16", self.fp16), ("nbits2", self.plaid))

    def stream(self):
        return torch.cuda.current_stream().cuda_stream

    def err(self):
        return self.eng.lib.rr_last_error(self.eng.h).decode()

    def bank_err(self, bank):
        return self.eng.lib.rr_bank_last_error(bank.h).decode()

    # the three calls that read a bank through the handle, on the sentinel-filled outputs
    def fib(self, bank, q_ptr=None, pp=PP, pq=PQ, seg_len=LC):
        pp, pq = np.asarray(pp, dtype=np.int32), np.asarray(pq, dtype=np.int32)
        return self.eng.lib.rr_forward_interaction_bank(
            self.eng.h, bank.h, self.q.data_ptr() if q_ptr is None else q_ptr, self.qm.data_ptr(), NQ, LQ, pp.ctypes.data,
            pq.ctypes.data, 1, (C.c_int32 * 1)(len(pp)), (C.c_int32 * 1)(seg_len), LC, 0, 1.0, self.logits[0].data_ptr(),
            self.logits[1].data_ptr(), None, self.stream())

    def bls(self, bank, q_ptr=None, pp=PP, pq=PQ, padded=LC):
        pp, pq = np.asarray(pp, dtype=np.int32), np.asarray(pq, dtype=np.int32)
        return self.eng.lib.rr_bank_li_scores(
            self.eng.h, bank.h, self.q.data_ptr() if q_ptr is None else q_ptr, NQ, LQ, pp.ctypes.data, pq.ctypes.data, len(pp),
            padded, self.scores.data_ptr(), self.maxsim.data_ptr(), self.stream())

    def search(self, bank, q_ptr=None):
        return self.eng.lib.rr_bank_search(
            self.eng.h, bank.h, self.q.data_ptr() if q_ptr is None else q_ptr, NQ, LQ, 0, -1, 2, self.top_i.data_ptr(),
            self.top_s.data_ptr(), self.stream())

    # rr_bank_add / rr_bank_add_compress (`entry`) on the padded device tensors; li, dtype, cm, ln, n: what a case hands over instead
    def add(self, bank, lengths, first, entry="rr_bank_add", **over):
        ln = np.asarray(lengths, dtype=np.int32)
        a = dict(li=self.add_li.data_ptr(), dtype=self.L.RR_F32, cm=self.add_cm.data_ptr(), ln=ln.ctypes.data, n=len(ln))
        a.update(over)
        return getattr(self.eng.lib, entry)(bank.h, a["li"], a["dtype"], a["cm"], a["ln"], a["n"], LC, C.byref(first), self.stream())

    def add_compress(self, bank, lengths, first, **over):
        return self.add(bank, lengths, first, entry="rr_bank_add_compress", **over)

    def add_plaid(self, bank, lengths, first):
        ln = np.asarray(lengths, dtype=np.int32)
        cd = np.ascontiguousarray(self.codes[:int(ln.sum())].numpy(), dtype=np.int32)
        rs = np.ascontiguousarray(self.res[:int(ln.sum())].numpy(), dtype=np.uint8)
        return self.eng.lib.rr_bank_add_plaid(bank.h, cd.ctypes.data, rs.ctypes.data, None, ln.ctypes.data, len(ln), C.byref(first),
                                              self.stream())

    def untouched(self):
        torch.cuda.synchronize()
        floats = self.logits + [self.scores, self.maxsim, self.top_s]
        return all(bool((t == POISON).all()) for t in floats) and bool((self.top_i == IPOISON).all())

    def banks_unchanged(self):
        want = dict(passages=len(LENS), rows_used=ROWS, capacity_rows=CAP_ROWS)
        held = all({k: b.info()[k] for k in want} == want and len(b) == len(LENS) for b in (self.fp16, self.plaid))
        return held and self.bare.info()["passages"] == 0 and self.bare.info()["rows_used"] == 0


@pytest.fixture(scope="module")
def s():
    return _Setup()


def test_a_bank_of_another_li_dim_and_a_misaligned_query(s):
    L = s.L
    for what, call in ((FIB, s.fib), (BLS, s.bls), (SEARCH, s.search)):
        assert call(s.other) == L.RR_ERR_BAD_SHAPE
        assert s.err() == f"{what}: the bank holds rows of 128, the handle's li_dim is 64"
        for _, bank in s.banks():
            assert call(bank, q_ptr=s.q.data_ptr() + 4) == L.RR_ERR_BAD_ARG
            assert s.err() == f"{what}: query_li must be 16-byte aligned"
    assert s.untouched()


def test_pair_indices_and_row_limits(s):
    L = s.L
    for _, bank in s.banks():
        for what, call in ((FIB, s.fib), (BLS, s.bls)):
            assert call(bank, pp=[0, 1, 3]) == L.RR_ERR_BAD_SHAPE
            assert s.err() == f"{what}: pair 2 names passage 3, the bank holds 3"
            assert call(bank, pp=[-1, 1, 2]) == L.RR_ERR_BAD_SHAPE
            assert s.err() == f"{what}: pair 0 names passage -1, the bank holds 3"
            assert call(bank, pq=[0, NQ, 1]) == L.RR_ERR_BAD_SHAPE
            assert s.err() == f"{what}: pair 1 names query 2 of 2"
        assert s.fib(bank, seg_len=4) == L.RR_ERR_BAD_SHAPE              # passage 1 holds 5 rows
        assert s.err() == f"{FIB}: pair 1: passage 1 holds 5 rows, its segment 4"
        assert s.bls(bank, padded=4) == L.RR_ERR_BAD_SHAPE
        assert s.err() == f"{BLS}: pair 1: passage 1 holds 5 rows, padded_context_len is 4"
    assert s.untouched()


def test_add_admission_and_the_wrong_kind_of_bank(s):
    L = s.L
    first = C.c_int32(-7)
    for what, add, bank in (("rr_bank_add", s.add, s.fp16), ("rr_bank_add_plaid", s.add_plaid, s.plaid)):
        assert add(bank, [1, 1], first) == L.RR_ERR_OOM                  # two passages, one slot is free
        assert s.bank_err(bank) == f"{what}: 3 + 2 passages exceed the bank's 4 slots"
        assert add(bank, [3], first) == L.RR_ERR_OOM                     # three rows, two are free
        assert s.bank_err(bank) == f"{what}: 10 + 3 rows exceed the bank's 12"
    assert s.add(s.plaid, [1], first) == L.RR_ERR_UNSUPPORTED
    assert s.bank_err(s.plaid) == "rr_bank_add on a compressed bank: it takes residual codes (rr_bank_add_plaid); nothing here compresses"
    assert s.add_plaid(s.fp16, [1], first) == L.RR_ERR_UNSUPPORTED
    assert s.bank_err(s.fp16) == "rr_bank_add_plaid on an fp16 bank: it takes embeddings (rr_bank_add)"
    assert first.value == -7 and s.banks_unchanged()


def test_the_padded_adds_refuse_alike(s):
    """rr_bank_add and rr_bank_add_compress, each on its own kind of bank, in the order they refuse: the wrong kind of bank (and for
    the compressing add a codec without cutoffs), a null argument, the dtype, the alignment, n / Lc, a length, the slots, the rows."""
    L = s.L
    first = C.c_int32(-7)
    for what, add, bank in (("rr_bank_add", s.add, s.fp16), ("rr_bank_add_compress", s.add_compress, s.plaid)):
        for null in ("li", "cm", "ln"):
            assert add(bank, [1], first, **{null: None}) == L.RR_ERR_BAD_ARG
            assert s.bank_err(bank) == f"{what}: null argument"
        assert add(bank, [1], first, dtype=L.RR_BF16) == L.RR_ERR_BAD_DTYPE
        assert s.bank_err(bank) == f"{what}: dtype 1 (RR_F32 or RR_F16)"
        assert add(bank, [1], first, dtype=7) == L.RR_ERR_BAD_DTYPE
        assert s.bank_err(bank) == f"{what}: dtype 7 (RR_F32 or RR_F16)"
        assert add(bank, [1], first, li=s.add_li.data_ptr() + 4) == L.RR_ERR_BAD_ARG
        assert s.bank_err(bank) == f"{what}: context_li must be 16-byte aligned"
        assert add(bank, [1], first, n=0) == L.RR_ERR_BAD_SHAPE
        assert s.bank_err(bank) == f"{what}: n=0 Lc=5"
        assert add(bank, [1, 0], first) == L.RR_ERR_BAD_SHAPE
        assert s.bank_err(bank) == f"{what}: passage 1 has length 0 (1..5)"
        assert add(bank, [6], first) == L.RR_ERR_BAD_SHAPE               # Lc is 5
        assert s.bank_err(bank) == f"{what}: passage 0 has length 6 (1..5)"
        assert add(bank, [1, 1], first) == L.RR_ERR_OOM                  # two passages, one slot is free
        assert s.bank_err(bank) == f"{what}: 3 + 2 passages exceed the bank's 4 slots"
        assert add(bank, [3], first) == L.RR_ERR_OOM                     # three rows, two are free
        assert s.bank_err(bank) == f"{what}: 10 + 3 rows exceed the bank's 12"
        # the kind of bank is asked before anything else: here with a null argument, a dtype and an n that would be refused too
        wrong = s.plaid if bank is s.fp16 else s.fp16
        assert add(wrong, [1], first, li=None, dtype=7, n=0) == L.RR_ERR_UNSUPPORTED
        assert s.bank_err(wrong) == ("rr_bank_add on a compressed bank: it takes residual codes (rr_bank_add_plaid); nothing here compresses"
                                     if bank is s.fp16 else
                                     "rr_bank_add_compress on an fp16 bank: it keeps embeddings as fp16 rows (rr_bank_add)")
    assert s.add_compress(s.bare, [1], first, li=None) == L.RR_ERR_UNSUPPORTED        # the cutoffs are asked before the arguments
    assert s.bank_err(s.bare) == "rr_bank_add_compress: the bank has no bucket cutoffs (rr_bank_set_plaid_cutoffs)"
    assert first.value == -7 and s.banks_unchanged()


def test_create_refusals(s):
    """rr_bank_create and rr_bank_create_plaid report through the handle; a refused call leaves *out null."""
    L, lib = s.L, s.eng.lib
    full = type(s.eng)(dict(s.eng.arch, model_kind="full_context"))      # no weights: a handle is all the call asks for
    cen, w = s.codec.centroids.data_ptr(), s.codec.bucket_weights.data_ptr()
    NC = s.codec.n_centroids

    def plain(h, cap, slots, out):
        return lib.rr_bank_create(h, cap, slots, out)

    def plaid(h, cap, slots, out, nbits=2, nc=NC, cen=cen, w=w):
        return lib.rr_bank_create_plaid(h, cap, slots, nbits, nc, cen, w, out)

    def err(h):
        return lib.rr_last_error(h).decode()
    for what, create, tail in (("rr_bank_create", plain, ""), ("rr_bank_create_plaid", plaid, f" n_centroids={NC}")):
        out = C.c_void_p(0xdead0)
        assert create(s.eng.h, 8, 4, None) == L.RR_ERR_BAD_ARG
        assert err(s.eng.h) == f"{what}: null out"
        assert create(full.h, 8, 4, C.byref(out)) == L.RR_ERR_BAD_ARG
        assert err(full.h) == f"{what} on a full-context model" and out.value is None
        for cap, slots in ((0, 4), (-1, 4), (8, 0), ((1 << 40) + 1, 4)):
            out = C.c_void_p(0xdead0)
            assert create(s.eng.h, cap, slots, C.byref(out)) == L.RR_ERR_BAD_SHAPE
            assert err(s.eng.h) == f"{what}: capacity_rows={cap} max_passages={slots}{tail}" and out.value is None
    out = C.c_void_p(0xdead0)
    what = "rr_bank_create_plaid"
    for null in (dict(cen=None), dict(w=None)):
        assert plaid(s.eng.h, 8, 4, C.byref(out), nbits=3, nc=0, **null) == L.RR_ERR_BAD_ARG    # before the shape and the counts
        assert err(s.eng.h) == f"{what}: null table"
    assert plaid(s.eng.h, 0, 4, C.byref(out), nbits=3) == L.RR_ERR_UNSUPPORTED                  # before the capacity
    assert err(s.eng.h) == f"{what}: nbits 3, li_dim 64 (nbits 1, 2, 4 or 8; li_dim a power of two in [8, 512], a multiple of 8 * nbits)"
    assert plaid(s.eng.h, 8, 4, C.byref(out), nbits=16) == L.RR_ERR_UNSUPPORTED                 # 64 is no multiple of 8 * 16
    assert err(s.eng.h) == f"{what}: nbits 16, li_dim 64 (nbits 1, 2, 4 or 8; li_dim a power of two in [8, 512], a multiple of 8 * nbits)"
    for nc in (0, -3, (1 << 24) + 1):
        assert plaid(s.eng.h, 8, 4, C.byref(out), nc=nc) == L.RR_ERR_BAD_SHAPE
        assert err(s.eng.h) == f"{what}: capacity_rows=8 max_passages=4 n_centroids={nc}"
    assert out.value is None and s.banks_unchanged()


def test_read_refusals_and_the_length_only_call(s):
    L, lib = s.L, s.eng.lib
    D = s.D
    rows = torch.full((LC, D), 7.0, dtype=torch.float16)
    codes = torch.full((LC,), IPOISON, dtype=torch.int32)
    res = torch.full((LC, s.codec.residual_bytes), 0xA5, dtype=torch.uint8)
    mask = torch.full((LC,), 0xA5, dtype=torch.uint8)

    def read(bank, index, cap, outs=True):
        return lib.rr_bank_read(bank.h, index, rows.data_ptr() if outs else None, mask.data_ptr() if outs else None, cap, s.stream())

    def read_plaid(bank, index, cap, outs=True):
        return lib.rr_bank_read_plaid(bank.h, index, codes.data_ptr() if outs else None, res.data_ptr() if outs else None,
                                      mask.data_ptr() if outs else None, cap, s.stream())
    for what, call, banks in (("rr_bank_read", read, (s.fp16, s.plaid)), ("rr_bank_read_plaid", read_plaid, (s.plaid,))):
        for bank in banks:
            for index in (3, -1):
                assert call(bank, index, LC) == L.RR_ERR_BAD_SHAPE
                assert s.bank_err(bank) == f"{what}: passage {index} of 3"
                assert call(bank, index, 0, outs=False) == L.RR_ERR_BAD_SHAPE          # the index comes before the length-only answer
                assert s.bank_err(bank) == f"{what}: passage {index} of 3"
            assert call(bank, 1, 4) == L.RR_ERR_BAD_SHAPE                              # passage 1 holds 5 rows
            assert s.bank_err(bank) == f"{what}: passage 1 holds 5 rows, the buffers 4"
            assert [call(bank, i, 0, outs=False) for i in range(3)] == LENS            # all outputs null: the length, whatever the capacity
    assert read_plaid(s.fp16, 1, LC) == L.RR_ERR_UNSUPPORTED
    assert s.bank_err(s.fp16) == "rr_bank_read_plaid on an fp16 bank: it holds no codes (rr_bank_read)"
    assert read_plaid(s.fp16, 7, 0, outs=False) == L.RR_ERR_UNSUPPORTED                # the kind of bank comes before the index
    assert s.bank_err(s.fp16) == "rr_bank_read_plaid on an fp16 bank: it holds no codes (rr_bank_read)"
    assert bool((rows == 7.0).all()) and bool((codes == IPOISON).all()) and bool((res == 0xA5).all()) and bool((mask == 0xA5).all())
    assert s.banks_unchanged()


def test_cutoffs_refusals(s):
    L, lib = s.L, s.eng.lib
    what = "rr_bank_set_plaid_cutoffs"

    def put(bank, values):
        v = np.asarray(values, dtype=np.float32)
        return lib.rr_bank_set_plaid_cutoffs(bank.h, v.ctypes.data if values is not None else None)
    assert put(s.fp16, None) == L.RR_ERR_UNSUPPORTED                                   # the kind of bank comes before the argument
    assert s.bank_err(s.fp16) == f"{what} on an fp16 bank: it holds embeddings as they are (rr_bank_add)"
    for bank in (s.plaid, s.bare):
        assert put(bank, None) == L.RR_ERR_BAD_ARG
        assert s.bank_err(bank) == f"{what}: null argument"
        assert put(bank, [0.0, float("nan"), -1.0]) == L.RR_ERR_BAD_SHAPE
        assert s.bank_err(bank) == f"{what}: cutoff 1 is NaN"
        assert put(bank, [-0.5, 0.25, 0.125]) == L.RR_ERR_BAD_SHAPE
        assert s.bank_err(bank) == f"{what}: cutoff 2 (0.125) lies below cutoff 1 (0.25): the sequence must not decrease"
        assert put(bank, [0.5, -1.0, 2.0]) == L.RR_ERR_BAD_SHAPE
        assert s.bank_err(bank) == f"{what}: cutoff 1 (-1) lies below cutoff 0 (0.5): the sequence must not decrease"
    first = C.c_int32(-7)
    assert s.add_compress(s.bare, [1], first) == L.RR_ERR_UNSUPPORTED                  # a refused table is no table
    assert s.bank_err(s.bare) == "rr_bank_add_compress: the bank has no bucket cutoffs (rr_bank_set_plaid_cutoffs)"
    assert first.value == -7 and s.banks_unchanged()


def test_a_capturing_stream(s):
    """Every call that stages, uploads or copies from the host refuses a stream that is being captured, in its own words; nothing
    but the probe enters the graph, and the same calls are taken once the capture is over."""
    L = s.L
    staged = "cannot be captured into a graph (it stages its descriptors from the host)"
    want = {}
    for kind, _ in s.banks():
        want[kind, FIB] = f"{FIB} {staged}"
        want[kind, BLS] = f"{BLS} {staged}"
        want[kind, SEARCH] = f"{SEARCH} cannot be captured into a graph (it may upload the bank's passage table and grow its block)"
    want["fp16", "add"] = f"rr_bank_add {staged}"
    want["nbits2", "add"] = "rr_bank_add_plaid cannot be captured into a graph (it copies from host memory and synchronises)"
    want["nbits2", "add_compress"] = f"rr_bank_add_compress {staged}"
    got = {}
    first = C.c_int32(-7)
    probe = torch.zeros(1, device="cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for _, bank in s.banks():                                       # warm-up on the capture stream: only the capture is in the way
            assert s.fib(bank) == 0 and s.bls(bank) == 0 and s.search(bank) == 0
        torch.cuda.synchronize()
        for t in s.logits + [s.scores, s.maxsim, s.top_s]:
            t.fill_(POISON)
        s.top_i.fill_(IPOISON)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            probe.add_(1.0)                                             # the graph holds this node alone
            for kind, bank in s.banks():
                for what, call in ((FIB, s.fib), (BLS, s.bls), (SEARCH, s.search)):
                    got[kind, what] = (call(bank), s.err())
                add = s.add if kind == "fp16" else s.add_plaid
                got[kind, "add"] = (add(bank, [1], first), s.bank_err(bank))
                if kind == "nbits2":
                    got[kind, "add_compress"] = (s.add_compress(bank, [1], first), s.bank_err(bank))
        graph.replay()
        torch.cuda.synchronize()
    assert got == {k: (L.RR_ERR_BAD_ARG, v) for k, v in want.items()}
    assert probe.item() == 1.0 and first.value == -7 and s.untouched() and s.banks_unchanged()
    for _, bank in s.banks():
        assert s.fib(bank) == 0 and s.bls(bank) == 0 and s.search(bank) == 0
    torch.cuda.synchronize()
    assert not (s.logits[0] == POISON).any() and not (s.scores == POISON).any() and not (s.top_i == IPOISON).any()
