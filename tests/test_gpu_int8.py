"""GPU: the int8 (W8A8) form of rr_config.fp8 (handle option "q8_format" = 1, csrc/gemm_fp8.hip with I8 = true).

The int8 GEMM accumulates exact int32 sums, so the operator tests compare against the exact int64 product of the codes times the
row / channel scales: the only tolerance is the rounding of the output (and the GELU approximation, three orders below it).  The
forward tests compare the device with the int8 emulation (tests/int8_emulation.py) and with the fp32 reference; the ranking tests
decide which subset of the stack the int8 default may cover (DESIGN.md "int8")."""
import numpy as np
import pytest
import torch

from helpers import ROOT  # noqa: F401
import oracle.rerank_oracle as O
from int8_emulation import int8_rounding, quant_rows_i8

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from rmr_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _i8_operands(M, N, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randn(M, K, device="cuda", generator=g) * (0.2 + 3.0 * torch.rand(M, 1, device="cuda", generator=g))
    w = torch.randn(N, K, device="cuda", generator=g) * (0.01 + 0.08 * torch.rand(N, 1, device="cuda", generator=g))
    bias = torch.randn(N, device="cuda", generator=g) * 0.1
    qa, sa = quant_rows_i8(a)
    qw, sw = quant_rows_i8(w)
    return qa.to(torch.int8), sa.reshape(-1).contiguous(), qw.to(torch.int8), sw.reshape(-1).contiguous(), bias


def _expected(qa, sa, qw, sw, bias, rows, epi):
    """The kernel's arithmetic in fp64 from the exact product: f32(acc) * f32(sa * sw) + bias (+ GELU); exact sums < 2^53."""
    acc = (qa[rows].double() @ qw.double().t()).float().double()
    v = acc * (sa[rows, None] * sw[None, :]).double() + bias.double()
    if epi == 1:
        v = torch.nn.functional.gelu(v)
    return v


def _run_gemm(lib, qa, qw, bias, sa, sw, M, N, K, epi):
    out = torch.full((M, N), float("nan"), dtype=torch.float32 if epi == 2 else torch.bfloat16, device="cuda")
    rc = lib.rr_op_gemm_i8_rc(qa.data_ptr(), qw.data_ptr(), bias.data_ptr(), sa.data_ptr(), sw.data_ptr(), M, N, K, epi,
                              out.data_ptr(), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out


# >= 512 tiles of 256 x 256 with N % 8 == 0 and epilogue 0 / 1: the persistent ring (one, two, three and 32 K-tiles; ragged M and N);
# the rest: the two-stage kernel
@pytest.mark.parametrize("M,N,K,epi", [(33_001, 1000, 128, 0), (33_100, 1024, 256, 1), (66_000, 776, 384, 0), (32_800, 1024, 4096, 1),
                                       (33_000, 1024, 256, 2), (300, 384, 256, 0), (300, 384, 256, 1), (37, 260, 128, 2),
                                       (513, 1024, 4096, 2), (517, 1000, 384, 0)])
def test_gemm_i8_matches_the_exact_product(lib, M, N, K, epi):
    qa, sa, qw, sw, bias = _i8_operands(M, N, K, M + N + K + epi)
    out = _run_gemm(lib, qa, qw, bias, sa, sw, M, N, K, epi)
    for r0 in sorted({0, max(0, M // 2 - 150), max(0, M - 300)}):          # the start, the middle and the partial last tile
        rows = slice(r0, min(M, r0 + 300))
        ref = _expected(qa, sa, qw, sw, bias, rows, epi)
        got = out[rows].double()
        assert torch.isfinite(got).all()
        # the output rounding only: 1 ulp of bf16 (2^-7 relative at most), a few fp32 ulps; + the GELU approximation (6.4e-7)
        tol = (2.0 ** -7 if epi != 2 else 4 * 2.0 ** -23) * ref.abs() + (2e-6 if epi == 1 else 1e-30)
        bad = (got - ref).abs() > tol
        assert not bad.any(), f"rows {r0}: {int(bad.sum())} of {bad.numel()} beyond tolerance, max |d| {(got - ref).abs().max().item():.3e}"


def test_gemm_i8_rejects_bad_shapes_and_epilogues(lib):
    x = torch.zeros(256, 256, dtype=torch.int8, device="cuda")
    out = torch.zeros(256, 256, device="cuda")
    assert lib.rr_op_gemm_i8_rc(x.data_ptr(), x.data_ptr(), 0, 0, 0, 256, 256, 192, 2, out.data_ptr(), _stream()) != 0   # K % 128
    assert lib.rr_op_gemm_i8_rc(x.data_ptr(), x.data_ptr(), 0, 0, 0, 256, 254, 128, 2, out.data_ptr(), _stream()) != 0   # N % 4
    for epi in (3, 4, -1):                                                  # no int8 GELU-to-8-bit / residual epilogue
        assert lib.rr_op_gemm_i8_rc(x.data_ptr(), x.data_ptr(), 0, 0, 0, 256, 256, 128, epi, out.data_ptr(), _stream()) != 0


@pytest.mark.parametrize("epi", [0, 1])
def test_gemm_i8_rows_do_not_depend_on_where_their_tile_lies(lib, epi):
    """Exact integer sums and a per-element epilogue: a row's bits depend neither on its place in the matrix, nor on M, nor on the
    kernel (ring at 66 000 rows against the two-stage kernel on 300 of those rows taken from the middle)."""
    M, N, K, r0, m = 66_000, 1024, 768, 31_111, 300
    qa, sa, qw, sw, bias = _i8_operands(M, N, K, 77 + epi)
    big = _run_gemm(lib, qa, qw, bias, sa, sw, M, N, K, epi)
    sub, ssub = qa[r0:r0 + m].contiguous(), sa[r0:r0 + m].contiguous()
    small = _run_gemm(lib, sub, qw, bias, ssub, sw, m, N, K, epi)
    assert torch.equal(big[r0:r0 + m], small)
    shifted = torch.roll(qa, 4097, 0).contiguous()                          # the same rows in other tiles of the ring
    big2 = _run_gemm(lib, shifted, qw, bias, torch.roll(sa, 4097, 0).contiguous(), sw, M, N, K, epi)
    assert torch.equal(torch.roll(big2, -4097, 0), big)


def test_layernorm_i8_matches_the_emulation(lib):
    """LayerNorm -> per-row int8 (rr_op_layernorm_i8): scales = row amax / 127 of the LayerNorm output, codes = the emulation's
    rounding of the same values; a code may differ by one step only where the fp32 LayerNorm arithmetic of torch and the device
    (last-bit differences) straddles a rounding boundary."""
    rows, cols = 777, 1024
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(rows, cols, generator=g) * 1.3 + 0.4)
    x[3] = 0.0                                                              # zero variance: LN output = beta
    x[5, 11] = 40.0                                                         # an outlier element sets its row's scale
    gamma, beta = 1 + 0.2 * torch.randn(cols, generator=g), 0.1 * torch.randn(cols, generator=g)
    beta0 = beta.clone()
    out = torch.zeros(rows, cols, dtype=torch.int8, device="cuda")
    sc = torch.zeros(rows, device="cuda")
    st = torch.zeros(rows, 2, device="cuda")
    eps = 1e-12
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    assert lib.rr_op_layernorm_i8(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), eps, rows, cols, out.data_ptr(), sc.data_ptr(),
                                  st.data_ptr(), _stream()) == 0
    # a zero row (gamma = beta = 0): scale 1, codes 0
    z = torch.zeros(4, cols, device="cuda")
    out0 = torch.ones(4, cols, dtype=torch.int8, device="cuda")
    sc0 = torch.zeros(4, device="cuda")
    assert lib.rr_op_layernorm_i8(z.data_ptr(), z[0].data_ptr(), z[0].data_ptr(), eps, 4, cols, out0.data_ptr(), sc0.data_ptr(), 0,
                                  _stream()) == 0
    torch.cuda.synchronize()
    assert (sc0 == 1.0).all() and (out0 == 0).all()
    y = torch.nn.functional.layer_norm(x, (cols,), gamma, beta0, eps)
    q, s = quant_rows_i8(y)
    got_q, got_s = out.cpu().float(), sc.cpu()
    assert torch.allclose(got_s, s.reshape(-1), rtol=3e-6, atol=0)
    assert got_q.abs().max().item() <= 127
    d = (got_q - q).abs()
    assert d.max().item() <= 1
    frac = (y / s).abs() % 1.0
    near_tie = (frac - 0.5).abs() < 2e-3
    assert not (d > 0)[~near_tie].any(), f"{int((d > 0)[~near_tie].sum())} codes differ away from a rounding boundary"
    assert (d > 0).float().mean().item() < 2e-3
    assert torch.allclose(st[:, 0].cpu(), x.mean(1), atol=1e-5)


# ---- forward ---------------------------------------------------------------------------------------------------------------------
def _small_cfg():
    cfg = O.OracleConfig(vocab_size=2000, hidden=256, layers=3, heads=4, intermediate=1024, max_pos=64, ce_hidden=256,
                         ce_heads=4, ce_intermediate=1024, ce_layers=2, ce_max_pos=128, li_dim=64)
    cfg.loss_fn = "BCE"
    return cfg


def _i8_engine(cfg, w, dt, vision=False, first=None):
    import rmr_amd
    from helpers import arch_from_cfg
    arch = arch_from_cfg(cfg, vision, dt)
    arch["fp8"] = 1
    arch["q8_format"] = 1
    eng = rmr_amd.RerankEngine(arch)
    if first is not None:
        eng.set_option("fp8_first_layer", first)
    eng.load_state_dict(w)
    return eng


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_int8_forward_small_model_against_the_emulation(dt):
    """Whole-stack int8 on a 3-layer 256-wide model (cross encoder of 1 and 2 layers): the device forward against the oracle with
    the same int8 rounding points, and the drift both have from the fp32 forward; then the subset options."""
    from helpers import record_margin
    t16 = torch.float16 if dt == "fp16" else torch.bfloat16
    for ce_layers in (1, 2):
        cfg = _small_cfg()
        cfg.ce_layers = ce_layers
        Bq, K, S = 2, 6, 64
        w = O.make_weights(cfg, seed=2, vision=False)
        ids, am, tt = O.make_pair_batch(cfg, Bq, K, S, seed=4)
        eng = _i8_engine(cfg, w, dt, first=0)
        assert eng.get_option("q8_format") == 1
        r = eng.forward_ids(ids.cuda(), am.cuda(), tt.cuda(), Bq, K, want_order=True)
        torch.cuda.synchronize()
        got = r["logits"].cpu()
        with torch.no_grad():
            ref = O.full_context_forward(cfg, w, ids, am, tt, Bq, K).logits.reshape(-1)
            with int8_rounding(t16) as mm:
                emu = O.full_context_forward(cfg, w, ids, am, tt, Bq, K, mm=mm).logits.reshape(-1)
        d_emu, d_ref, e_ref = (got - emu).abs().max().item(), (got - ref).abs().max().item(), (emu - ref).abs().max().item()
        print(f"[int8 small/{dt}/ce{ce_layers}] device vs same-rounding emulation {d_emu:.2e}; device vs fp32 {d_ref:.2e}; "
              f"emulation vs fp32 {e_ref:.2e}")
        record_margin(f"int8_small/{dt}/ce{ce_layers}", vs_emulation=d_emu, vs_fp32=d_ref, emulation_vs_fp32=e_ref)
        assert torch.isfinite(got).all()
        assert d_emu <= max(2e-3, 0.5 * e_ref)
        assert d_ref <= 2.0 * e_ref + 1e-3
        assert r["order"].cpu().tolist() == [O.rank_descending_stable(x) for x in got.view(Bq, K).tolist()]
        for first, qkv in ((1, 1), (2, 1), (0, 0)):
            eng.set_option("fp8_first_layer", first)
            eng.set_option("fp8_qkv", qkv)
            got_s = eng.forward_ids(ids.cuda(), am.cuda(), tt.cuda(), Bq, K)["logits"].cpu()
            with torch.no_grad(), int8_rounding(t16, fp8_first=first, fp8_qkv=bool(qkv)) as mm:
                emu_s = O.full_context_forward(cfg, w, ids, am, tt, Bq, K, mm=mm).logits.reshape(-1)
            d_s, e_s = (got_s - emu_s).abs().max().item(), (emu_s - ref).abs().max().item()
            print(f"[int8 small/{dt}/ce{ce_layers}] first int8 layer {first}, int8 QKV {qkv}: device vs emulation {d_s:.2e}; "
                  f"emulation vs fp32 {e_s:.2e}")
            assert torch.isfinite(got_s).all() and d_s <= max(2e-3, 0.5 * e_s)


def test_int8_handle_options():
    """"q8_format" is latched by rr_finalize_weights; "fp8_ffn_down" = 1 is refused on an int8 handle; an e4m3 handle with
    "q8_format" pinned to 0 computes exactly what one left at the default does."""
    import rmr_amd
    from helpers import arch_from_cfg
    cfg = _small_cfg()
    w = O.make_weights(cfg, seed=3, vision=False)
    Bq, K, S = 2, 5, 64
    ids, am, tt = O.make_pair_batch(cfg, Bq, K, S, seed=6)
    args = (ids.cuda(), am.cuda(), tt.cuda(), Bq, K)
    arch = arch_from_cfg(cfg, False, "fp16")
    arch["fp8"] = 1
    default = rmr_amd.RerankEngine(arch)
    assert default.get_option("q8_format") == 0
    default.load_state_dict(w)
    pinned = rmr_amd.RerankEngine(dict(arch, q8_format=0))
    pinned.load_state_dict(w)
    a, b = default.forward_ids(*args)["logits"], pinned.forward_ids(*args)["logits"]
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    with pytest.raises(Exception, match="latched"):
        pinned.set_option("q8_format", 1)
    pinned.set_option("q8_format", 0)                       # the latched value itself is accepted
    i8 = _i8_engine(cfg, w, "fp16")
    assert i8.get_option("q8_format") == 1
    with pytest.raises(Exception, match="latched"):
        i8.set_option("q8_format", 0)
    with pytest.raises(Exception, match="fp8_ffn_down"):
        i8.set_option("fp8_ffn_down", 1)
    c = i8.forward_ids(*args)["logits"]
    torch.cuda.synchronize()
    assert torch.isfinite(c).all() and not torch.equal(c, a)
    pre = rmr_amd.RerankEngine(dict(arch, q8_format=1))
    with pytest.raises(Exception, match="fp8_ffn_down"):
        pre.set_option("fp8_ffn_down", 1)


# The c5_full gate of the int8 whole stack: the bf16 rule (helpers.fullsize_bf16_gate: 1.5 x the reference's own bf16-autocast drift)
def test_int8_whole_stack_against_the_c5_golden():
    from helpers import fullsize_bf16_gate, load_fullsize, margin_stats, record_margin
    cfg, w, vision, qs = load_fullsize("c5_full")
    eng = _i8_engine(cfg, w, "fp16", vision, first=0)
    q = qs[0]
    K = q["ids"].shape[0]
    ref, ac = q["fp32"], q["autocast"]
    r = eng.forward_ids(q["ids"].cuda(), q["am"].cuda(), q["tt"].cuda(), 1, K)
    torch.cuda.synchronize()
    got = r["logits"].cpu()
    st = margin_stats(got, ref)
    gate = fullsize_bf16_gate("c5_full")
    print(f"[c5_full/int8+fp16 whole stack] K={K}: |dlogit| vs fp32 max {st['max_abs']:.3e}, centred {st['centred']:.3e}; rho "
          f"{st['rho']:.4f}; top-5 {st['top5']}; reference bf16-autocast drift {(ac - ref).abs().max():.3e}; gate {gate:.3e}")
    record_margin("c5_full/int8+fp16/whole_stack", gate_abs=gate, reference_bf16_autocast_drift=float((ac - ref).abs().max()), **st)
    assert torch.isfinite(got).all()
    assert st["max_abs"] <= gate


# ---- ranking: the point of the int8 form ----------------------------------------------------------------------------------------
# Device study (tests/tools/int8_subset_study.py, profiles/r06_int8_subset_study.json; DESIGN.md "int8").  "Ranks with margin" is the
# rule of tests/test_gpu_fp8.py: on every list where the rule binds the fp32 top-5 set is kept with centred drift <= gap / 2.  The
# binding list that decides is c5_sep_wide q0 (half-gap 0.180): centred drift 0.197 with int8 in all 24 layers (e4m3: 0.596), 0.206
# in the last 18, 0.150 in the last 12 (the default), 0.100 in the last 8.
INT8_WHOLE_STACK_RANKS = False       # frozen verdict of "q8_format" 1 with "fp8_first_layer" 0; a change that flips it edits this line
INT8_SAFE_LAYERS = 12                # rr_api.hip INT8_SAFE_LAYERS: the int8 default covers the last min(layers, this) layers


def _fixtures():
    import os
    from helpers import GOLDEN, RANKING_FIXTURES_C5
    return [n for n in RANKING_FIXTURES_C5 if os.path.exists(os.path.join(GOLDEN, f"{n}.npz"))]


def _rank(eng, name, qs, tag):
    from helpers import margin_stats, ranking_yardstick, record_margin, top5_set
    rows = []
    for qi, q in enumerate(qs):
        y = ranking_yardstick(q)
        sel, ref = y["sel"], y["ref"]
        r = eng.forward_ids(q["ids"][sel].cuda(), q["am"][sel].cuda(), q["tt"][sel].cuda(), 1, len(sel), want_order=True)
        torch.cuda.synchronize()
        lg = r["logits"].cpu()
        st = margin_stats(lg, ref)
        kept = top5_set(lg) == top5_set(ref)
        print(f"[{name}/{tag} q{qi}] |dlogit| {st['max_abs']:.3e} centred {st['centred']:.3e} (gap/2 {0.5 * y['gap']:.3f}) rho "
              f"{st['rho']:.4f} top-5 {st['top5']} {'kept' if kept else 'LOST'}; rule {'binds' if y['binds'] else 'does not bind'}")
        record_margin(f"{name}/q{qi}/{tag}", gap_5_6=y["gap"], top5_set_kept=bool(kept), rule_binds=y["binds"], **st)
        assert torch.isfinite(lg).all() and r["order"][0].cpu().tolist() == O.rank_descending_stable(lg.tolist())
        rows.append(dict(stats=st, kept=kept, y=y))
    return rows


def _ranks_with_margin(rows):
    binding = [r for r in rows if r["y"]["binds"]]
    return binding, all(r["kept"] and r["stats"]["centred"] <= 0.5 * r["y"]["gap"] for r in binding)


@pytest.mark.parametrize("name", _fixtures())
def test_int8_default_subset_ranks_wherever_the_reference_arithmetic_does(name):
    from helpers import load_fullsize
    cfg, w, vision, qs = load_fullsize(name)
    eng = _i8_engine(cfg, w, "fp16", vision)
    assert eng.get_option("fp8_first_layer") == max(0, cfg.layers - INT8_SAFE_LAYERS) and eng.get_option("fp8_qkv") == 1
    rows = _rank(eng, name, qs, "int8/default")
    _, ok = _ranks_with_margin(rows)
    assert ok


def test_int8_whole_stack_verdict_is_the_frozen_one():
    from helpers import load_fullsize
    all_rows = []
    for name in _fixtures():
        cfg, w, vision, qs = load_fullsize(name)
        eng = _i8_engine(cfg, w, "fp16", vision, first=0)
        all_rows += _rank(eng, name, qs, "int8/whole_stack")
        del eng
        torch.cuda.empty_cache()
    binding, ok = _ranks_with_margin(all_rows)
    assert binding, "no fixture binds: the verdict would be vacuous"
    assert ok == INT8_WHOLE_STACK_RANKS


# ---- outliers ---------------------------------------------------------------------------------------------------------------------
INT8_NO_SMOOTH_FACTOR = 10.0         # frozen: without the gain migration the outlier model's drift is at least this x the smoothed one's (measured 26 x)


def test_int8_keeps_outlier_models_accurate_and_the_smoothing_is_why(lib):
    """The outlier weights of tests/test_gpu_outliers.py (LayerNorm gains x50 / x50 / x300 in three dimensions of every text-encoder
    LayerNorm, the consuming columns compensated) on the c2 shape, whole-stack int8.  Drift = relative error of the text encoder's
    output on the ORDINARY dimensions (the ones a per-row int8 scale set by an outlier dimension crushes; the outlier model's
    logits barely move, its LayerNorms divide every ordinary dimension by the outliers' variance): it stays within 2 x the int8
    drift of the same model without outliers; with the diagnostic switch "q8_smooth" 0 (plain per-channel int8) it is clearly
    worse — the gain migration is what keeps it."""
    from helpers import load_golden, record_margin
    from test_gpu_outliers import DIMS, _outlier_weights
    cfg = load_golden("c2")["cfg"]
    Bq, K, S = 2, 6, 64
    ids, am, tt = O.make_pair_batch(cfg, Bq, K, S, seed=5)
    args = (ids.cuda(), am.cuda(), tt.cuda(), Bq, K)
    ordinary = torch.ones(cfg.hidden, dtype=torch.bool)
    ordinary[[d for d, _ in DIMS]] = False
    d, dl = {}, {}
    for tag, scales, smooth in (("plain", (), 1), ("outliers", DIMS, 1), ("outliers_no_smooth", DIMS, 0)):
        w = _outlier_weights(cfg, scales)
        ref = O.full_context_forward(cfg, w, ids, am, tt, Bq, K, want_taps=True)
        gold_h = ref.taps[f"text_layer_{cfg.layers - 1}"][..., ordinary]
        gold = ref.logits.reshape(-1)
        assert lib.rr_set_tuning(b"q8_smooth", smooth) == 0
        try:
            eng = _i8_engine(cfg, w, "fp16", first=0)
        finally:
            lib.rr_set_tuning(b"q8_smooth", 1)
        eng.set_debug(True)
        got = eng.forward_ids(*args)["logits"].cpu()
        th = eng.debug_read("text_hidden", Bq * K * S * cfg.hidden).view(Bq * K, S, cfg.hidden)[..., ordinary]
        assert torch.isfinite(got).all() and torch.isfinite(th).all()
        d[tag] = ((th - gold_h).norm() / gold_h.norm()).item()
        dl[tag] = (got - gold).abs().max().item() / gold.std().item()
    print("int8 whole stack: text-encoder output, relative error on the ordinary dimensions:", d, "| max |dlogit| / logit std:", dl)
    record_margin("outliers_c2_S64/int8", text_rel_err=d, logit_err_over_std=dl)
    assert d["outliers"] <= 2.0 * d["plain"]
    assert d["outliers_no_smooth"] >= INT8_NO_SMOOTH_FACTOR * d["outliers"]
