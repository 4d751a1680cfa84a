"""CPU: the fixtures of tests/test_gpu_bank_search_f16.py in float64 (tests/bank_f16_cases.py) and the host side of the fp16
matrix-core search: F16Search's checks and what PassageBank.search, search_bank_part, search_banks and retrieve refuse before they
reach an engine.  No device, no library call."""
import numpy as np
import pytest

import bank_f16_cases as C
from rmr_amd import F16Search, InteractionRerankModel, PassageBank, PlaidSearch, f16_default_slack, search_bank_part, search_banks

NDOCS, K = 64, 16
RANDOM_CASES = [(128, 17, 32), (64, 3, 5), (128, 1, 5), (64, 17, 32)]      # (D, n_queries, Lq) of the GPU test


@pytest.mark.parametrize("D,nq,Lq", RANDOM_CASES)
def test_random_fixture_leaves_the_certificate_twice_the_default_slack(D, nq, Lq):
    """In float64 the k-th exact score stands at least 2 x the default slack above the (ndocs + 1)-th best, for every query: with
    |A - E| <= slack a passage outside the survivors has A <= a* <= (ndocs + 1)-th best E + slack < k-th E - slack, so "every query
    certified" on the GPU is what the bound predicts, not a coincidence."""
    fx = C.random_fixture(D, nq, Lq, seed=D + Lq)
    E = C.exact64(fx)
    slack = C.default_slack(fx["q"], D)
    assert slack == pytest.approx(f16_default_slack(np.linalg.norm(fx["q"].astype(np.float64), axis=-1).sum(axis=-1).max(), D, Lq), rel=1e-12)
    for qi in range(nq):
        s = E[qi, C.rank_order(E[qi])]
        assert s[K - 1] - s[NDOCS] >= 2.0 * slack, (qi, s[K - 1], s[NDOCS], slack)
    assert np.abs(C.approx64(fx) - E).max() <= slack                      # the query's rounding alone stays inside it
    assert (C.search_f16(C.approx64(fx), E, NDOCS, K, slack)[2] == 1).all()


@pytest.mark.parametrize("D", [64, 128])
def test_adversarial_fixture_expects_another_result_than_the_exact_search(D):
    fx = C.adversarial_fixture(D, NDOCS)
    n = len(fx["lens"])
    E, A = C.exact64(fx), C.approx64(fx)
    assert (A == 1.0).all() and E[0, n - 1] == 1.0 + 2.0 ** -12 and (E[0, :n - 1] == 1.0 - 2.0 ** -13).all()
    assert C.rank_order(E[0])[0] == n - 1                                 # the exact search returns the e1 passage first
    for slack in (0.0, C.default_slack(fx["q"], D)):
        idx, sc, cert = C.search_f16(A, E, NDOCS, K, slack)
        assert idx[0].tolist() == list(range(K)) and (sc == 1.0 - 2.0 ** -13).all() and cert.tolist() == [0]


def test_f16search_arguments():
    f = F16Search(64)
    assert f.ndocs == 64 and f.slack is None and "64" in repr(f)
    assert F16Search(1024, 0.0).slack == 0.0 and F16Search(1, 0.25).slack == 0.25
    for bad in (0, -3):
        with pytest.raises(ValueError):
            F16Search(bad)
    with pytest.raises(NotImplementedError):
        F16Search(1025)
    for bad in (-1e-9, float("nan"), -float("inf")):
        with pytest.raises(ValueError):
            F16Search(8, bad)
    assert F16Search(8, 0.5).slack_for(None) == 0.5                       # a given slack reads no query
    import torch
    q = torch.nn.functional.normalize(torch.randn(3, 7, 64), dim=-1)
    q[1] *= 2.0
    assert F16Search(8).slack_for(q) == pytest.approx(f16_default_slack(14.0, 64, 7), rel=1e-6)
    assert f16_default_slack(32.0, 128, 32) == pytest.approx((1 + 2 ** -10) * (32 * (2 ** -11 + 128 * 2 ** -22 + 32 * 2 ** -22) + 32 * 128 ** 0.5 * 2 ** -25),
                                                             rel=1e-12)


def test_fast_is_refused_with_plaid_filter_or_sparse_before_an_engine_is_touched():
    bank = object.__new__(PassageBank)                                    # the check stands in front of every use of the bank
    bank.h = None
    fast, plaid = F16Search(8), PlaidSearch(2, 0.45, 64)
    for kw in (dict(plaid=plaid), dict(filter=object()), dict(filter=object(), sparse=True), dict(sparse=True)):
        with pytest.raises(ValueError, match="fast="):
            bank.search(None, None, 4, fast=fast, **kw)
        with pytest.raises(ValueError, match="fast="):
            search_bank_part(None, bank, None, 4, fast=fast, **kw)
    with pytest.raises(ValueError, match="fast="):
        search_banks(None, [bank], None, 4, fast=fast, plaid=plaid)
    with pytest.raises(ValueError, match="fast="):
        search_banks(None, [bank], None, 4, fast=fast, filters=[None])
    model = object.__new__(InteractionRerankModel)
    model.bank = bank
    for kw in (dict(plaid=plaid), dict(allowed=["a"]), dict(excluded=["a"]), dict(filter=object())):
        with pytest.raises(ValueError, match="fast="):
            model.retrieve(None, 4, fast=fast, **kw)
        with pytest.raises(ValueError, match="fast="):
            model.retrieve_and_rerank(None, None, 4, fast=fast, **kw)
    with pytest.raises(ValueError, match="return_certified"):
        model.retrieve(None, 4, return_certified=True)
