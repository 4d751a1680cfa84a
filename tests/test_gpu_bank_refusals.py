"""GPU: the full text of the refusals that the bank entry points share — rr_forward_interaction_bank, rr_bank_li_scores,
rr_bank_search, rr_bank_add and rr_bank_add_plaid (include/rerank_mi355.h).

The other bank suites sample these messages by substring; here the return code and the COMPLETE rr_last_error /
rr_bank_last_error string of each is pinned, written out by hand from the format strings of csrc/rr_api.hip, on an fp16 bank and
on an nbits = 2 bank of three passages (2, 5 and 3 rows) with Lq = 4.  Every call is refused on the host before anything is
enqueued: an output buffer a call was handed keeps its sentinel, a bank keeps its contents."""
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
        codec = _codec(D, 2)
        self.codes, self.res = _rows(codec, ROWS, seed=9)
        self.plaid = self.eng.create_bank(CAP_ROWS, SLOTS, codec=codec)
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

    def add(self, bank, lengths, first):
        ln = np.asarray(lengths, dtype=np.int32)
        return self.eng.lib.rr_bank_add(bank.h, self.add_li.data_ptr(), self.L.RR_F32, self.add_cm.data_ptr(), ln.ctypes.data, len(ln), LC,
                                        C.byref(first), self.stream())

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
        return all({k: b.info()[k] for k in want} == want and len(b) == len(LENS) for b in (self.fp16, self.plaid))


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
        graph.replay()
        torch.cuda.synchronize()
    assert got == {k: (L.RR_ERR_BAD_ARG, v) for k, v in want.items()}
    assert probe.item() == 1.0 and first.value == -7 and s.untouched() and s.banks_unchanged()
    for _, bank in s.banks():
        assert s.fib(bank) == 0 and s.bls(bank) == 0 and s.search(bank) == 0
    torch.cuda.synchronize()
    assert not (s.logits[0] == POISON).any() and not (s.scores == POISON).any() and not (s.top_i == IPOISON).any()
