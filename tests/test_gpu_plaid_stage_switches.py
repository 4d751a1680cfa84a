"""GPU: the two stop-after switches of the pruned bank search (rr_set_tuning "plaid_stop_after" for rr_bank_search_plaid,
"plaid_ivf_stop_after" for rr_bank_search_plaid_ivf) and what a call books per stage, on the one plan, stage driver and cost routine
both forms share (csrc/bank_search_plaid.hip, csrc/bank_api.hip).

For each form and each legal stop value, on poisoned outputs: the call returns RR_OK; below the last stage the outputs are still
poison, bit for bit; at the last stage they equal, bit for bit, the outputs of a call made before any switch was touched.  A value
outside the range is refused and leaves the switch where it was, which the next call's result shows.  Setting one key does not change
the other form.  The launches, FLOPs and bytes booked in the "tail" class are those of the commit before the two forms were folded
into one: host arithmetic, compared with ==.

Cases: the bank of test_gpu_bank_ivf.py::test_a_query_without_a_candidate (D 64, 64 centroids, 40 passages, 2 queries, ncells 1,
ndocs 32) at k = 5 and k = 1, and one bank of 4097 one-row passages that share one centroid: the scan form's selection over the A1
row takes two slices of 4096, and the longest list covers the bank, so the inverted-file form's rows are as wide as the range."""
import numpy as np
import pytest
import torch

from test_gpu_bank_ivf import _outputs, _raw
from test_gpu_bank_search_plaid import LEN_CYCLE, _build, _codec, _topic_rows
from test_gpu_li_scores import _engine as _bare_engine

pytestmark = pytest.mark.gpu

SCAN, IVF = "rr_bank_search_plaid", "rr_bank_search_plaid_ivf"
KEY = {SCAN: b"plaid_stop_after", IVF: b"plaid_ivf_stop_after"}
STAGES = {SCAN: 8, IVF: 9}
D, C, KW = 64, 64, dict(ncells=1, thr=0.45, ndocs=32)

# (launches, flops, bytes) of the "tail" class of ONE call at stop value 0, 1, ... of each form (the sum over the stages the call
# ran), taken by running _walk of this file on commit 89e19e9 (the parent of the change that folded the two plans, drivers and cost
# tables into one).  k does not enter the costs: the two small cases book the same.
_SMALL = {
    SCAN: [(1, 98304.0, 14336.0), (2, 98304.0, 17408.0), (3, 98304.0, 20480.0), (4, 98304.0, 30225.0), (5, 98304.0, 31185.0),
           (6, 98304.0, 32209.0), (7, 618393.6000000001, 165617.40000000002), (8, 618393.6000000001, 165873.40000000002)],
    IVF: [(1, 98304.0, 14336.0), (2, 98304.0, 17408.0), (3, 98304.0, 20480.0), (4, 98304.0, 21470.0), (5, 98304.0, 40640.0),
          (6, 98304.0, 41600.0), (7, 98304.0, 42624.0), (8, 618393.6000000001, 176032.40000000002),
          (9, 618393.6000000001, 176288.40000000002)],
}
PARENT = {
    "k5": _SMALL,
    "k1": _SMALL,
    "two_slices": {
        SCAN: [(1, 98304.0, 14336.0), (2, 98304.0, 17408.0), (3, 98304.0, 20480.0), (4, 98304.0, 172069.0), (5, 98304.0, 270397.0),
               (6, 98304.0, 271421.0), (7, 110592.0, 274573.0), (8, 110592.0, 274829.0)],
        IVF: [(1, 98304.0, 14336.0), (2, 98304.0, 17408.0), (3, 98304.0, 20480.0), (4, 98304.0, 121880.75), (5, 98304.0, 392282.75),
              (6, 98304.0, 490610.75), (7, 98304.0, 491634.75), (8, 110592.0, 494786.75), (9, 110592.0, 495042.75)],
    },
}

_CASES = {}


def _case(name):
    """(engine, bank with its inverted file, queries, k).  Query 0 lies near centroid 3, query 1 near a centroid no passage holds."""
    if name not in _CASES:
        eng = _bare_engine(D)
        codec = _codec(D, 8, C)
        if name == "two_slices":
            lens = [1] * 4097
            codes, res = _topic_rows(codec, lens, seed=19, topics_from=[3])
        else:
            lens = [LEN_CYCLE[i % len(LEN_CYCLE)] for i in range(40)]
            codes, res = _topic_rows(codec, lens, seed=9, topics_from=list(range(8, 32)))
            first = np.concatenate([[0], np.cumsum(lens)])
            for p in (4, 17, 30):
                codes[first[p]] = 3                               # three passages hold a token of centroid 3
        bank = _build(eng, codec, lens, codes, res, None)
        bank.build_ivf()
        gen = torch.Generator().manual_seed(1)
        tok = lambda c: torch.nn.functional.normalize(codec.centroids[c].float()[None] + 0.3 * torch.randn(6, D, generator=gen) / D ** 0.5, dim=-1)
        _CASES[name] = (eng, bank, torch.stack([tok(3), tok(45)]).cuda(), 1 if name == "k1" else 5)
    return _CASES[name]


def _same_bits(got, want):
    return all(torch.equal(g.view(torch.int32), w.view(torch.int32)) for g, w in zip(got, want))


def _call(case, entry):
    """One call on poisoned outputs: (outputs, what the profile booked for it in the tail class, launches of the other classes)."""
    eng, bank, q, k = case
    out = _outputs(q.shape[0], k)
    eng.get_profile(reset=True)
    assert _raw(entry, eng, bank, q, out, k, **KW) == 0, eng.lib.rr_last_error(eng.h)
    torch.cuda.synchronize()
    p = eng.get_profile(reset=True)
    assert sum(v["launches"] for name, v in p.items() if name != "tail") == 0
    return out, (p["tail"]["launches"], p["tail"]["flops"], p["tail"]["bytes"])


def _walk(name):
    """Every check of this file but the comparison with PARENT; returns {entry: [booking at stop 0, 1, ...]}."""
    from rmr_amd import _lib as L
    case = _case(name)
    eng, bank, q, k = case
    poison = _outputs(q.shape[0], k)
    set_key = lambda entry, v: eng.lib.rr_set_tuning(KEY[entry], v)
    eng.set_profiling(True)
    try:
        base, full = {}, {}
        for entry in (SCAN, IVF):                                  # before any switch is touched
            base[entry], full[entry] = _call(case, entry)
            assert not _same_bits(base[entry], poison) and full[entry][0] == STAGES[entry]
        assert _same_bits(base[IVF], base[SCAN])
        booked = {SCAN: [], IVF: []}
        for entry, other in ((SCAN, IVF), (IVF, SCAN)):
            last = STAGES[entry] - 1
            for stop in range(STAGES[entry]):
                assert set_key(entry, stop) == L.RR_OK
                out, book = _call(case, entry)
                assert book[0] == stop + 1
                assert _same_bits(out, base[entry] if stop == last else poison), f"{entry} at {stop}"
                booked[entry].append(book)
                out, book = _call(case, other)                     # the other form does not see this key
                assert _same_bits(out, base[other]) and book == full[other], f"{other} with {entry} at {stop}"
            assert booked[entry][last] == full[entry]
            assert set_key(entry, 2) == L.RR_OK
            for bad in (-1, STAGES[entry]):                        # refused, and the switch stays at 2
                assert set_key(entry, bad) == L.RR_ERR_BAD_ARG
                out, book = _call(case, entry)
                assert book == booked[entry][2] and _same_bits(out, poison), f"{entry} after {bad}"
            assert set_key(entry, last) == L.RR_OK
            out, book = _call(case, entry)
            assert _same_bits(out, base[entry]) and book == full[entry]
        return booked
    finally:
        for entry in (SCAN, IVF):
            set_key(entry, STAGES[entry] - 1)
        eng.set_profiling(False)


@pytest.mark.parametrize("name", ["k5", "k1", "two_slices"])
def test_stop_after_switches_and_the_booking_of_both_forms(name):
    booked = _walk(name)
    for entry in (SCAN, IVF):
        for stop, (got, want) in enumerate(zip(booked[entry], PARENT[name][entry])):
            print(f"{name} {entry} stop {stop}: booked {got}, parent {want}")
        assert booked[entry] == PARENT[name][entry], entry
