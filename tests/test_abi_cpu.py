"""CPU: the C-ABI library builds, loads, exports every symbol include/rerank_mi355.h declares, and the product
path refuses to run without a GPU (no fallback).  No compute calls here."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()                                   # hipcc cross-compiles gfx950 without a GPU
    from rmr_amd import _lib
    return _lib.load()


def _declared_functions(header="rerank_mi355.h"):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(rr_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_are_exported_and_bound(lib):
    from rmr_amd import _lib
    names = _declared_functions()
    diag = _declared_functions("rerank_mi355_diag.h")
    assert len(names) >= 20 and len(diag) >= 20 and not set(names) & set(diag)
    for n in names + diag:
        assert hasattr(lib, n), f"{n} declared under include/ but not exported"
    assert set(names) | set(diag) == set(_lib.EXPORTED), "ctypes table and headers disagree"
    # rerank_mi355.h is the PRODUCT ABI INTEGRATION.md binds; operators, tuning switches, stamps and debug
    # taps live in rerank_mi355_diag.h
    assert not [n for n in names if n.startswith(("rr_op_", "rr_util_", "rr_debug")) or n in
                ("rr_set_tuning", "rr_set_gemm_stagger", "rr_set_gemm_variant", "rr_set_gemm_stamps", "rr_set_attn_stamps",
                 "rr_set_attn_redo_stats", "rr_set_op_dtype", "rr_set_debug")]


def test_gemm_objects_hold_no_packed_f32(lib):
    """The build refuses device code with compiler-formed v_pk_{add,mul,fma}_f32 in the GEMM / elementwise objects (gfx950
    stale-lane hazard behind a vmcnt wait, DESIGN.md "Numerics"); here the check runs on the objects the library was linked from."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("rr_build", os.path.join(ROOT, "reranking-multimodal-retrievers_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    for o in b.NO_PACKED_F32:
        b.check_no_packed_f32(os.path.join(b.HERE, "build", o))


def test_version_and_status_strings(lib):
    assert b"gfx950" in lib.rr_version()
    assert lib.rr_status_string(0) == b"ok"
    assert lib.rr_status_string(-2) == b"bad shape"


def test_config_struct_layout_matches_header():
    from rmr_amd import _lib
    # 8 + 1 + 1 + 12 + 1 + 1 + 7 four-byte fields
    assert C.sizeof(_lib.RRConfig) == 4 * 32     # 31 fields of ABI 1 + fp8 (ABI 2)
    assert C.sizeof(_lib.RRProfile) == 8 * 7 * 4


def test_no_gpu_means_loud_failure(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import rmr_amd
    from rmr_amd import _lib
    c = _lib.RRConfig()
    c.abi_version = _lib.RR_ABI_VERSION
    for k, v in dict(vocab_size=100, hidden=128, layers=1, heads=2, intermediate=256, max_pos=64, type_vocab=2,
                     li_dim=64, ce_hidden=128, ce_layers=1, ce_heads=2, ce_intermediate=256, ce_max_pos=64).items():
        setattr(c, k, v)
    h = C.c_void_p()
    rc = lib.rr_create(C.byref(c), C.byref(h))
    assert rc == _lib.RR_ERR_NO_DEVICE and not h.value
    assert b"no CPU path" in lib.rr_last_error(None)
    with pytest.raises(RuntimeError):
        rmr_amd.RerankEngine(rmr_amd.make_arch())
    with pytest.raises(RuntimeError):
        rmr_amd.FullContextRerankModel(dict(loss_fn="BCE"))


def test_bad_abi_version_rejected(lib):
    from rmr_amd import _lib
    c = _lib.RRConfig()
    c.abi_version = 99
    h = C.c_void_p()
    assert lib.rr_create(C.byref(c), C.byref(h)) == _lib.RR_ERR_BAD_ARG
    assert lib.rr_create(None, C.byref(h)) == _lib.RR_ERR_BAD_ARG


def test_product_never_imports_the_oracle():
    """The oracle is test infrastructure: nothing under the package may import it."""
    pkg = os.path.join(ROOT, "reranking-multimodal-retrievers_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dp, f)).read()
                assert "oracle" not in txt.replace("test oracle", "").replace("the oracle's scheme", ""), f
    assert "oracle" not in open(os.path.join(ROOT, "rmr_amd.py")).read()


def test_weight_spec_matches_library_required_names():
    """Host-side name table == the reference state_dict keys the C side asks for (checked without a GPU by
    parsing the names out of the C source is brittle; instead compare with the oracle's independent table)."""
    import rmr_amd
    from oracle import rerank_oracle as O
    a = rmr_amd.make_arch(dict(loss_fn="BCE"))
    ours = [(n, tuple(s)) for n, s, _ in rmr_amd.weight_spec(a)]
    theirs = [(n, tuple(s)) for n, s, _ in O.weight_spec(O.OracleConfig(), vision=True)]
    assert ours == theirs
    assert len(ours) == 5 + 12 * 16 + 1 + 6 + 26 + 2 + 2 + 4 + 16 + 4
    sd = rmr_amd.synthetic_state_dict(rmr_amd.make_arch(dict(loss_fn="BCE"), layers=1, vocab_size=50), seed=3,
                                      hf_init=False)
    ref = O.make_weights(O.OracleConfig(layers=1, vocab_size=50), seed=3, vision=True)
    assert all((sd[k] == ref[k]).all() for k in ref) and set(sd) == set(ref)


def test_host_row_quantiser_matches_torch_e4m3():
    """rr_util_quantize_rows_e4m3 (the weight packer of rr_config.fp8; pure host code) against torch.float8_e4m3fn:
    per-row scale amax / 448, round to nearest even, including subnormal codes, exact zeros and a zero row."""
    import ctypes as C

    import torch
    from rmr_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(3)
    W = torch.randn(37, 256, generator=g) * torch.logspace(-4, 1, 37)[:, None]
    W[5] = 0.0
    W[7, :20] = W[7].abs().max() * torch.logspace(-6, -1, 20)           # deep into the subnormal codes of that row
    W[9, 3] = 0.0
    out = torch.empty(37, 256, dtype=torch.uint8)
    sc = torch.empty(37)
    assert lib.rr_util_quantize_rows_e4m3(W.data_ptr(), 37, 256, out.data_ptr(), sc.data_ptr()) == 0
    amax = W.abs().amax(1)
    want_s = torch.where(amax > 0, amax * (1.0 / 448.0), torch.ones_like(amax))
    assert torch.equal(sc, want_s)
    want = (W * (1.0 / want_s)[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    same = (out == want) | ((out & 0x7f) == 0) & ((want & 0x7f) == 0)     # +0 / -0 both encode zero
    assert same.all(), f"{int((~same).sum())} codes differ"


def test_host_row_quantiser_e4m3_gives_a_row_with_a_nan_or_inf_a_non_finite_scale():
    """The e4m3 sibling of tests/test_int8_cpu.py test_a_nan_or_inf_in_a_weight_row_makes_its_scale_non_finite: the row maximum
    (fmaxf) dropped a NaN and the clamp turned it into -448 under a finite scale.  Now the row's scale is NaN; rows without a
    NaN / inf pack bit for bit as before."""
    import torch
    from rmr_amd import _lib
    lib = _lib.load()

    def quant(W):
        out = torch.empty(W.shape, dtype=torch.uint8)
        sc = torch.empty(W.shape[0])
        assert lib.rr_util_quantize_rows_e4m3(W.contiguous().data_ptr(), W.shape[0], W.shape[1], out.data_ptr(), sc.data_ptr()) == 0
        return out, sc

    out, sc = quant(torch.tensor([[0.5, float("nan"), -0.25, 0.1], [0.5, 0.25, -0.25, 0.1]]))
    assert not torch.isfinite(sc[0]) and sc[1].item() == (torch.tensor(0.5) * (1.0 / 448.0)).item()
    assert out[1].view(torch.float8_e4m3fn).float().tolist() == [448.0, 224.0, -224.0, 88.0]
    g = torch.Generator().manual_seed(9)
    W = torch.randn(64, 256, generator=g) * torch.logspace(-3, 1, 64)[:, None]
    bad = W.clone()
    bad[3, 0], bad[10, 255], bad[20, 7], bad[33, 100], bad[33, 101] = float("nan"), float("nan"), float("inf"), float("-inf"), float("nan")
    rows = torch.tensor([3, 10, 20, 33])
    keep = torch.ones(64, dtype=torch.bool)
    keep[rows] = False
    o0, s0 = quant(W)
    o1, s1 = quant(bad)
    assert not torch.isfinite(s1[rows]).any()
    assert torch.equal(s1[keep].view(torch.int32), s0[keep].view(torch.int32)) and torch.equal(o1[keep], o0[keep])
