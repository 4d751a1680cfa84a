"""CPU: the fp16-matrix-core search over COMPRESSED banks (rr_bank_search_f16_plaid) as far as it stands without a device: the fixture
of tests/test_gpu_bank_search_f16_plaid.py's certificate test through the host definitions of the codec, in float64, and the
dispatch of `fast=` on the bank's format.  (tests/test_abi_cpu.py, unchanged, sees rr_bank_search_f16_plaid and
rr_op_bank_scores_f16_plaid declared, bound and exported.)"""
import numpy as np
import pytest
import torch

import bank_f16_cases as C
import bank_f16_plaid_cases as CP
from rmr_amd import F16Search, InteractionRerankModel, PassageBank, RerankEngine
from rmr_amd.passage_bank import BankTable

NDOCS, K = 64, 16
CERT_CASES = [(128, 17, 32), (64, 3, 5)]                                  # (D, n_queries, Lq) of the GPU test


@pytest.mark.parametrize("nbits", [8, 4])
@pytest.mark.parametrize("D,nq,Lq", CERT_CASES)
def test_compressed_random_fixture_is_certified_at_twice_the_default_slack(D, nq, Lq, nbits):
    """bank_f16_cases.random_fixture, its rows compressed and decoded by the host definitions with a codec from its own residuals:
    on A and E of the decoded rows in float64 the definition certifies every query at TWICE the default slack with ndocs 64 < n.
    So "every query certified at the default slack" on the GPU rests on the reference arithmetic alone: with |A - E| <= slack the
    device's a* is at most slack above the float64 one and its k-th score the same."""
    fx = C.random_fixture(D, nq, Lq, seed=D + Lq)
    dfx, codes, res = CP.decoded_fixture(fx, CP.fixture_codec(fx, nbits))
    assert codes.min() >= 0 and codes.max() < CP.N_CENTROIDS and len(np.unique(codes.numpy())) > CP.N_CENTROIDS // 2
    norms = np.linalg.norm(dfx["rows"].astype(np.float64), axis=-1)
    assert norms.max() <= 1.0 + 2.0 ** -10, "a decoded row's norm is within the R f16_default_slack assumes"
    A, E = C.approx64(dfx), C.exact64(dfx)
    slack = C.default_slack(fx["q"], D)
    assert np.abs(A - E).max() <= slack                                   # the query's rounding alone stays inside it
    assert NDOCS < A.shape[1]
    idx, sc, cert = C.search_f16(A, E, NDOCS, K, 2.0 * slack)
    assert (cert == 1).all(), f"queries {np.flatnonzero(cert == 0).tolist()} are not certified at twice the default slack"
    for qi in range(nq):                                                  # ... and what is certified is the exact search's row
        assert idx[qi].tolist() == C.rank_order(E[qi])[:K].tolist()


_RESULT = dict(indices=torch.tensor([[2, 0, 1]]), scores="s", certified="c")


class _Recorder:
    """an engine that only says which entry was called"""

    def __init__(self):
        self.calls = []

    def bank_search_f16(self, bank, q, k, ndocs, slack, **kw):
        self.calls.append(("f16", k, ndocs, slack, kw))
        return dict(_RESULT)

    def bank_search_f16_plaid(self, bank, q, k, ndocs, slack, **kw):
        self.calls.append(("f16_plaid", k, ndocs, slack, kw))
        return dict(_RESULT)


def _bare_bank(codec, n=4):
    bank = object.__new__(PassageBank)
    bank.h, bank.codec, bank.table = None, codec, BankTable()
    bank.table.append([f"p{i}" for i in range(n)], [1] * n)
    return bank


def test_fast_dispatches_on_the_banks_format():
    fast = F16Search(8, 0.25)
    for codec, want in ((object(), "f16_plaid"), (None, "f16")):
        eng, bank = _Recorder(), _bare_bank(codec)
        r = bank.search(eng, None, 3, first=1, count=3, fast=fast)
        assert r == _RESULT
        assert eng.calls == [(want, 3, 8, 0.25, dict(first=1, count=3))]
        model = object.__new__(InteractionRerankModel)
        model.bank, model.engine = bank, eng
        ids, scores, cert = model.retrieve(None, 3, fast=fast, return_certified=True)
        assert ids == [["p2", "p0", "p1"]] and scores == "s" and cert == "c"
        assert [c[0] for c in eng.calls] == [want, want]


def test_the_engine_entries_refuse_the_other_format_before_the_library():
    eng = object.__new__(RerankEngine)
    eng.arch, eng.device = dict(li_dim=64), torch.device("cpu")
    q = torch.zeros(2, 5, 64)
    with pytest.raises(NotImplementedError, match="compressed"):
        RerankEngine.bank_search_f16(eng, _bare_bank(object()), q, 2, 4)   # the refusal of the fp16 entry stands
    with pytest.raises(NotImplementedError, match="bank_search_f16"):
        RerankEngine.bank_search_f16_plaid(eng, _bare_bank(None), q, 2, 4)
    for bad_k, ndocs in ((0, 4), (5, 8), (5, 4)):                         # k < 1, k > passages, k > ndocs
        with pytest.raises(ValueError, match="bank_search_f16_plaid"):
            RerankEngine.bank_search_f16_plaid(eng, _bare_bank(object()), q, bad_k, ndocs)
    with pytest.raises(NotImplementedError):
        RerankEngine.bank_search_f16_plaid(eng, _bare_bank(object()), q, 2, 1025)
