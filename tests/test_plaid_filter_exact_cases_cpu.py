"""CPU: the fixture of tests/test_gpu_bank_search_filter_scale.py bites, shown on the oracle alone (tests/plaid_filter_exact_cases.py):
under the shared filter and under the per-query filters every query keeps at least k candidates, so the GPU test compares full
lists; the filters remove candidates of every query and change a final list; no filtered-out passage is a candidate."""
import numpy as np
import pytest

import plaid_filter_exact_cases as F
import plaid_ivf_exact_cases as V


@pytest.mark.parametrize("which", ["shared", "per_query"])
def test_every_query_keeps_k_candidates_and_the_filter_changes_the_lists(which):
    case, plain = V.get(F.CASE)
    shared, per_query = F.filters()
    want = F.oracle(which)
    k, changed = case["k"], 0
    assert len(want) == case["nq"] == len(F.DENSITY) and 0.45 < shared.mean() < 0.55
    for qi, (w, p) in enumerate(zip(want, plain)):
        allowed = shared[0] if which == "shared" else per_query[qi]
        cand, cand_plain = w["a1"] != -np.inf, p["a1"] != -np.inf
        assert np.array_equal(cand, cand_plain & allowed), f"query {qi}: candidates are the unfiltered candidates the filter allows"
        assert k <= cand.sum() < cand_plain.sum(), f"query {qi}: {cand.sum()} of {cand_plain.sum()} candidates"
        assert len(w["final"]) == k and all(allowed[j] for j in w["final"]), f"query {qi}: a full list of allowed passages"
        assert np.array_equal(w["cells"], p["cells"]) and np.array_equal(w["keep"], p["keep"]), "stages 0 - 2 do not see the filter"
        changed += w["final"] != p["final"]
    assert changed >= 1
