"""Candidate filters at the sizes the pruned search is made for: the `wide` case of tests/plaid_ivf_exact_cases.py (16 384 centroids,
40 007 passages, four queries; its generators and those of tests/plaid_exact_cases.py are used as they are) under one shared filter of
about half the passages and under one filter row per query, and the float64 oracle of those modules evaluated on the masks ZEROED for
the filtered-out passages: PROPERTY B of rr_bank_search_plaid_filtered (include/rerank_mi355.h) as a definition.  Helper of
tests/test_plaid_filter_exact_cases_cpu.py and tests/test_gpu_bank_search_filter_scale.py.  Calls nothing of the library."""
import numpy as np

import plaid_exact_cases as X
import plaid_ivf_exact_cases as V

CASE = "wide"
DENSITY = [0.9, 0.5, 0.25, 0.1]            # of the per-query rows; query 0's candidates all lie from passage 32 768 on

_BUILT = {}


def filters():
    """(shared bool [1, P], per_query bool [nq, P]), the same in every process."""
    if "filters" not in _BUILT:
        case, _ = V.get(CASE)
        P = len(case["lens"])
        rng = np.random.default_rng(31)
        _BUILT["filters"] = (rng.random((1, P)) < 0.5, rng.random((case["nq"], P)) < np.array(DENSITY)[:, None])
    return _BUILT["filters"]


def masked(case, allowed_row):
    """The case with every row of a passage outside `allowed_row` (bool [P]) masked."""
    out = dict(case)
    out["mask"] = case["mask"] * np.repeat(allowed_row, case["lens"]).astype(case["mask"].dtype)
    return out


def oracle(which):
    """Per query dict(cells, keep, a1, a2, list1, list2, final) of the case under the `shared` or the `per_query` filter."""
    if which not in _BUILT:
        case, _ = V.get(CASE)
        shared, per_query = filters()
        if which == "shared":
            _BUILT[which] = X.oracle(masked(case, shared[0]))
        else:
            _BUILT[which] = [X.oracle(masked(case, per_query[qi]), S=case["S"][qi:qi + 1], exact=case["exact"][qi:qi + 1])[0]
                             for qi in range(case["nq"])]
    return _BUILT[which]
