"""CPU: what an fp16 bank with a centroid table (rr_bank_set_centroids, include/rerank_mi355.h) needs no device for: the two new entry
points are declared, exported and bound, and refuse a NULL bank before they touch a device; the Python surface decides between a
plain fp16 bank, a coded one and a compressed one on the host (the pruned search asks for codes, not for a codec; ncells is held
against the centroid count of either source; saving an index names add_compress).  The device side: tests/test_gpu_bank_coded.py."""
import os
import re

import pytest
import torch

from rmr_amd import BankTable, PassageBank, PlaidCodec, PlaidSearch
from rmr_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 64


def _stub(centroids=None, codec=None, n=3):
    """A PassageBank without a device: the host table and what set_centroids / a codec leave behind."""
    bank = PassageBank.__new__(PassageBank)
    bank.table = BankTable()
    bank.table.append([f"p{i}" for i in range(n)], [2 + i for i in range(n)])
    bank.h, bank.codec, bank.li_dim, bank.generation = None, codec, D, 0
    bank._centroids = None if centroids is None else centroids.half()
    return bank


def _codec(C_=5):
    cen = torch.nn.functional.normalize(torch.randn(C_, D, generator=torch.Generator().manual_seed(C_)), dim=-1)
    return PlaidCodec(cen, torch.linspace(-0.1, 0.1, 4), 2, bucket_cutoffs=torch.tensor([-0.05, 0.0, 0.05]))


def test_the_entry_points_are_declared_exported_and_refuse_a_null_bank():
    lib = L.load()
    main = open(os.path.join(ROOT, "include", "rerank_mi355.h")).read()
    diag = open(os.path.join(ROOT, "include", "rerank_mi355_diag.h")).read()
    assert re.search(r"^int rr_bank_set_centroids\(rr_bank_handle b, const uint16_t\* centroids_f16_host, int32_t n_centroids, void\* hip_stream\);",
                     main, re.M)
    assert re.search(r"^int rr_bank_read_codes\(rr_bank_handle b, int32_t index, int32_t\* codes_out, int32_t capacity_rows, void\* hip_stream\);",
                     diag, re.M)
    assert "rr_bank_set_centroids" in L.EXPORTED and "rr_bank_read_codes" in L.EXPORTED
    cen = torch.zeros(4, D, dtype=torch.float16)
    codes = torch.full((4,), -7, dtype=torch.int32)
    assert lib.rr_bank_set_centroids(None, cen.data_ptr(), 4, None) == L.RR_ERR_BAD_ARG
    assert lib.rr_bank_read_codes(None, 0, codes.data_ptr(), 4, None) == L.RR_ERR_BAD_ARG and (codes == -7).all()
    assert lib.rr_bank_last_error(None) == b""
    assert "fp16 banks without a centroid table" in main and "Out of scope: ndocs > 1024, fp16 banks." not in main


def test_centroids_come_from_the_table_or_from_the_codec():
    cen = _codec().centroids
    plain, coded, compressed = _stub(), _stub(centroids=cen), _stub(codec=_codec())
    assert plain.centroids is None and plain.n_centroids == 0
    assert coded.n_centroids == 5 and torch.equal(coded.centroids, cen.half()) and coded.centroids.dtype == torch.float16
    assert compressed.n_centroids == 5 and compressed.centroids is compressed.codec.centroids
    with pytest.raises(NotImplementedError, match="compressed bank"):
        compressed.set_centroids(cen)
    with pytest.raises(ValueError, match=r"centroids must be \[C, 64\]"):
        plain.set_centroids(torch.zeros(5, 32))
    with pytest.raises(ValueError, match="not both"):
        PassageBank(None, 8, 2, codec=_codec(), centroids=cen)


def test_what_needs_residuals_refuses_a_coded_bank_and_names_add_compress():
    coded, plain = _stub(centroids=_codec().centroids), _stub()
    for call in (lambda b: b.save_plaid_index("/nonexistent/never-written"), lambda b: b.export_compressed()):
        with pytest.raises(NotImplementedError, match="add_compress into a compressed bank"):
            call(coded)
        with pytest.raises(NotImplementedError, match="on an fp16 bank: it holds no codes"):      # a plain bank: as it always said
            call(plain)
    with pytest.raises(NotImplementedError):
        coded.read_compressed("p0")
    with pytest.raises(NotImplementedError, match="set_centroids"):
        plain.codes("p0")
    for name in ("build_ivf", "extend_ivf"):
        with pytest.raises(NotImplementedError, match="on an fp16 bank: it holds no centroid codes"):
            getattr(plain, name)()
    with pytest.raises(NotImplementedError, match="on an fp16 bank: it holds no centroid codes"):
        plain.load_ivf((torch.zeros(0, dtype=torch.int32), torch.zeros(5, dtype=torch.int64)))
    with pytest.raises(ValueError, match="4 lists, the codec holds 5 centroids"):                # a coded bank: the table's count
        coded.load_ivf((torch.zeros(0, dtype=torch.int32), torch.zeros(4, dtype=torch.int64)))


class _Engine:
    """RerankEngine's pruned entries down to the library call, which a bank without codes, or a bad ncells, never reaches."""
    arch = {"li_dim": D}
    device = torch.device("cpu")

    def __init__(self):
        from rmr_amd.model import RerankEngine
        self.bank_search_plaid = lambda *a, **kw: RerankEngine.bank_search_plaid(self, *a, **kw)
        self.bank_search_plaid_ivf = lambda *a, **kw: RerankEngine.bank_search_plaid_ivf(self, *a, **kw)


def test_the_pruned_search_asks_for_codes_and_holds_ncells_to_either_source():
    eng, q = _Engine(), torch.zeros(2, 4, D)
    for ivf in (False, True):
        ps = PlaidSearch(2, 0.4, 16, ivf=ivf)
        with pytest.raises(NotImplementedError, match="an fp16 bank \\(the pruned search reads the centroid codes of a compressed bank\\)"):
            _stub().search(eng, q, 2, plaid=ps)
        for bank in (_stub(centroids=_codec().centroids), _stub(codec=_codec())):
            with pytest.raises(ValueError, match="ncells = 6 of 5 centroids"):
                bank.search(eng, q, 2, plaid=PlaidSearch(6, 0.4, 16, ivf=ivf))
            with pytest.raises(ValueError, match="k = 5 of ndocs // 4 = 4 survivors and 3 passages"):      # past the codes check, past ncells
                bank.search(eng, q, 5, plaid=ps)
