"""GPU: the filtered pruned searches (rr_bank_search_plaid_filtered, rr_bank_search_plaid_ivf_filtered) at the sizes the search is
made for: 16 384 centroids, 40 007 passages (the `wide` case of tests/plaid_ivf_exact_cases.py: compact rows narrower than the range,
two rounds of the compaction, a query with more than 4 096 unfiltered candidates), under one shared filter of about half the passages
and under one filter row per query.  Both forms are held to the float64 oracle evaluated on the masks zeroed for the filtered-out
passages (tests/plaid_filter_exact_cases.py; tests/test_plaid_filter_exact_cases_cpu.py shows that every query keeps k candidates)
and to each other, bit for bit on poisoned outputs."""
import numpy as np
import pytest
import torch

import bank_filter_ref as ref
import plaid_filter_exact_cases as F
import plaid_ivf_exact_cases as V
from test_gpu_bank_ivf_scale import _bank
from test_gpu_bank_search_filter import _checked, _dev_bits, _outputs, _raw_plaid, _same_bytes
from test_gpu_bank_search_plaid import _check_result

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("which", ["shared", "per_query"])
def test_filtered_forms_against_the_float64_oracle_and_each_other(which):
    case, _ = V.get(F.CASE)
    want = F.oracle(which)
    eng, bank = _bank("big")
    bank.build_ivf()
    allowed = F.filters()[0 if which == "shared" else 1]
    P, k, nq = len(case["lens"]), case["k"], case["nq"]
    bits = _dev_bits(ref.pack_bits([np.flatnonzero(r) for r in allowed], P, False))
    q = torch.from_numpy(case["queries"]).cuda()
    got = {}
    for entry in ("rr_bank_search_plaid_filtered", "rr_bank_search_plaid_ivf_filtered"):
        out = _outputs(nq, k)
        assert _raw_plaid(entry, eng, bank, q, out, k, bits=bits, ncells=case["ncells"], thr=case["threshold"], ndocs=case["ndocs"],
                          Lqc=case["Lqc"]) == 0, eng.lib.rr_last_error(eng.h)
        torch.cuda.synchronize()
        gi, gs, gc = got[entry] = _checked(out, nq, k)
        assert gc.tolist() == [k] * nq
        _check_result(dict(indices=gi, scores=gs, counts=gc), want, case["exact"], k)
    _same_bytes(got["rr_bank_search_plaid_ivf_filtered"], got["rr_bank_search_plaid_filtered"], "the two forms")
