"""The row and glue kernels of elementwise.hip at op level (rr_op_embed_ln, rr_op_ce_embed_ln, rr_op_li_normalize, rr_op_key_bias,
rr_op_joint_masks, rr_op_interaction_bias, rr_op_vit_im2col, rr_op_vit_embed_ln, rr_op_cast16, rr_op_gather_rows, rr_op_cls_heads,
rr_op_ln_finalize): each against a float64 reference of the same operation, at the row lengths, row counts, index forms and
values where such kernels go wrong.  The forwards reach these kernels only through their logits goldens.

Where the design makes a relation exact it is asserted bitwise: masks, biases, gathers, im2col, casts, the 16-bit LayerNorm rows
(= the fp32 rows rounded), constant rows (= beta), the clamped embedding rows, and the L2-normalised rows (= the 16-bit value
nearest the float64 result, up to LI_SLACK next to a rounding midpoint).  The rest is gated against float64 in units of the fp32
rounding of the row (U times the magnitudes the kernel forms: _ln_ref, test_cls_heads, test_ln_finalize_statistics) at values
measured on an MI355X (parity_margins.json keys row_kernels.*)."""
from contextlib import contextmanager

import pytest
import torch

from helpers import O, record_margin

pytestmark = pytest.mark.gpu

RR_ERR_BAD_ARG, RR_ERR_BAD_SHAPE = -1, -2
T16 = {0: torch.bfloat16, 1: torch.float16}
NEG = -1e30
RANGE_SS_FP16 = 9.0e8          # rr_common.h RR_RANGE_SS_FP16
U = 2.0 ** -24
ROW_COLS = [4, 128, 260, 768, 1024, 2044, 2048]     # 260: 65 float4s, lane 0 holds two; 2048 = 64 lanes x MAX_V4 float4s
# Gates, each in units of the fp32 rounding of its row (U times the magnitudes the kernel forms), measured on an MI355X over every
# case of this file (parity_margins.json keys row_kernels.*); each gate is about twice the largest measured value:
LN_UNITS = 8.0         # LayerNorm-family fp32 rows vs float64 (measured: 4.1, embed_ln 241 x 17 x 768; mean-1e3 rows 2.6)
DOT_UNITS = 1.0        # classifier heads vs float64, unit U x sum |h w| (measured: 0.16, T = 1, cols 768)
STATS_UNITS = 4.0      # ln_finalize mean and rstd vs float64 (measured: mean 2.2 at cols 4096, rstd 1.1 at cols 776)
LI_SLACK = 2.0 ** -20  # relative window around the float64 result in which either 16-bit neighbour is accepted (16 fp32 ulps;
                       # measured: 7 of 133 120 values take the other neighbour inside it, D = 2048 fp16)


@pytest.fixture(scope="module")
def lib():
    import rmr_amd  # noqa: F401
    from rmr_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else 0


@contextmanager
def _op_dtype(lib, dt):
    assert lib.rr_set_op_dtype(dt) == 0
    try:
        yield T16[dt]
    finally:
        lib.rr_set_op_dtype(0)


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _filled16(shape, t16):
    """16-bit buffer of NaNs (0x7fff in both types): a row the kernel does not write keeps these bits."""
    return torch.full(shape, 0x7fff, dtype=torch.int16, device="cuda").view(t16)


def _ln_ref(x64, g64, b64, eps):
    """float64 LayerNorm (the oracle's) and the fp32 rounding unit of each row: U x the largest magnitude the kernel forms,
    (|x - mean| + |mean|) * rstd * |gamma| + |beta| — the mean's rounding enters scaled by rstd."""
    y = O.layer_norm(x64, {"ln.weight": g64, "ln.bias": b64}, "ln", eps)
    mean = x64.mean(-1, keepdim=True)
    rstd = (x64.var(-1, unbiased=False, keepdim=True) + eps).rsqrt()
    unit = U * (((x64 - mean).abs() + mean.abs()) * rstd * g64.abs() + b64.abs()).amax(-1, keepdim=True)
    return y, unit.clamp_min(1e-300)


def _ln_units(got32, ref, unit):
    return float(((got32.double().cpu() - ref) / unit).abs().max())


def _check_ln(key, got32, got16, ref, unit, t16):
    """fp32 rows within LN_UNITS of float64; 16-bit rows == the fp32 rows rounded, bit for bit."""
    units = _ln_units(got32, ref, unit)
    record_margin(f"row_kernels.{key}", ln_units=units)
    assert units <= LN_UNITS, f"{key}: {units:.1f} units from float64"
    if got16 is not None:
        assert torch.equal(_bits(got16), _bits(got32.to(t16)))


def _params(cols, seed):
    g = torch.Generator().manual_seed(seed)
    gamma = 1 + 0.2 * torch.randn(cols, generator=g)
    beta = 0.1 * torch.randn(cols, generator=g)
    return g, gamma, beta


# ------------------------------------------------------------------------------------------------ embeddings + LayerNorm
def _embed(lib, ids, tts, word, pos, typ, gamma, beta, eps, S, vocab, type_vocab, t16, rc=0):
    rows, cols = ids.numel(), gamma.numel()
    o32 = torch.full((rows, cols), float("nan"), device="cuda")
    o16 = _filled16((rows, cols), t16)
    got = lib.rr_op_embed_ln(_ptr(ids), _ptr(tts), _ptr(word), _ptr(pos), _ptr(typ), _ptr(gamma), _ptr(beta), eps, rows, S, cols,
                             vocab, type_vocab, _ptr(o32), _ptr(o16), _stream())
    assert got == rc
    torch.cuda.synchronize()
    return o32, o16


def _embed_case(lib, dt, n, S, cols, with_tt, seed):
    vocab, type_vocab = 50, 3
    g, gamma, beta = _params(cols, seed)
    word = torch.randn(vocab, cols, generator=g)
    pos = 2 * torch.randn(S, cols, generator=g)          # distinct position and type rows: a wrong row index is O(1)
    typ = 2 * torch.randn(type_vocab, cols, generator=g)
    ids = torch.randint(0, vocab, (n, S), generator=g)
    tts = torch.randint(0, type_vocab, (n, S), generator=g) if with_tt else None
    w = {"e.word_embeddings.weight": word.double(), "e.position_embeddings.weight": pos.double(),
         "e.token_type_embeddings.weight": typ.double(), "e.LayerNorm.weight": gamma.double(), "e.LayerNorm.bias": beta.double()}
    eps = 1e-12
    ref = O.bert_embeddings(w, "e", eps, input_ids=ids, token_type_ids=tts).reshape(n * S, cols)
    x64 = (word[ids] + typ[tts if with_tt else torch.zeros_like(ids)] + pos[None]).double().reshape(n * S, cols)
    _, unit = _ln_ref(x64, gamma.double(), beta.double(), eps)
    with _op_dtype(lib, dt) as t16:
        o32, o16 = _embed(lib, ids.cuda(), tts.cuda() if with_tt else None, word.cuda(), pos.cuda(), typ.cuda(), gamma.cuda(),
                          beta.cuda(), eps, S, vocab, type_vocab, t16)
    _check_ln(f"embed_ln.dt{dt}.{n}x{S}x{cols}.tt{int(with_tt)}", o32, o16, ref, unit, t16)


@pytest.mark.parametrize("cols", ROW_COLS)
@pytest.mark.parametrize("dt", [0, 1])
def test_embed_ln_row_lengths(lib, dt, cols):
    _embed_case(lib, dt, 3, 77, cols, True, cols + dt)         # 231 rows: the last block holds 3 rows


@pytest.mark.parametrize("n,S,with_tt", [(1, 1, True), (1, 5, False), (241, 17, True), (2, 77, False)])
def test_embed_ln_row_counts_and_token_types(lib, n, S, with_tt):
    _embed_case(lib, n % 2, n, S, 768, with_tt, n + S)          # 1, 5, 4097 and 154 rows


def test_embed_ln_clamps_ids_into_the_tables(lib):
    """ids -1, -3, vocab, vocab + 2 and token types -1, -3, type_vocab, type_vocab + 2 read the clamped rows.  Each table sits
    inside a larger allocation with SENT NaN rows on both sides, and every id here lies within SENT rows of its table: a broken
    clamp reads a NaN row, never memory outside the allocation."""
    SENT = 3
    vocab, type_vocab, S, cols = 40, 2, 9, 256
    g, gamma, beta = _params(cols, 5)
    word_big = torch.full((vocab + 2 * SENT, cols), float("nan"))
    word_big[SENT:-SENT] = torch.randn(vocab, cols, generator=g)
    typ_big = torch.full((type_vocab + 2 * SENT, cols), float("nan"))
    typ_big[SENT:-SENT] = torch.randn(type_vocab, cols, generator=g)
    pos = torch.randn(S, cols, generator=g)
    ids = torch.randint(0, vocab, (2, S), generator=g)
    tts = torch.randint(0, type_vocab, (2, S), generator=g)
    ids[0, 0], ids[0, 3], ids[1, 5], ids[1, 8] = -1, vocab, -SENT, vocab + SENT - 1
    tts[0, 1], tts[1, 2], tts[0, 6], tts[1, 8] = -1, type_vocab, -SENT, type_vocab + SENT - 1
    assert int(ids.min()) >= -SENT and int(ids.max()) < vocab + SENT and int(tts.min()) >= -SENT and int(tts.max()) < type_vocab + SENT
    ids_c, tts_c = ids.clamp(0, vocab - 1), tts.clamp(0, type_vocab - 1)
    wb, tb = word_big.cuda(), typ_big.cuda()
    word_d, typ_d = wb[SENT:-SENT], tb[SENT:-SENT]
    ids_d, tts_d, idc_d, ttc_d = ids.cuda(), tts.cuda(), ids_c.cuda(), tts_c.cuda()
    args = (word_d, pos.cuda(), typ_d, gamma.cuda(), beta.cuda(), 1e-12, S, vocab, type_vocab)
    for dt in (0, 1):
        with _op_dtype(lib, dt) as t16:
            o32, o16 = _embed(lib, ids_d, tts_d, *args, t16)
            c32, c16 = _embed(lib, idc_d, ttc_d, *args, t16)
        assert torch.isfinite(o32).all()
        assert torch.equal(_bits(o32), _bits(c32)) and torch.equal(_bits(o16), _bits(c16))
    w = {"e.word_embeddings.weight": word_big[SENT:-SENT].double(), "e.position_embeddings.weight": pos.double(),
         "e.token_type_embeddings.weight": typ_big[SENT:-SENT].double(), "e.LayerNorm.weight": gamma.double(),
         "e.LayerNorm.bias": beta.double()}
    ref = O.bert_embeddings(w, "e", 1e-12, input_ids=ids_c, token_type_ids=tts_c).reshape(2 * S, cols)
    x64 = (word_big[SENT:-SENT][ids_c] + typ_big[SENT:-SENT][tts_c] + pos[None]).double().reshape(2 * S, cols)
    _, unit = _ln_ref(x64, gamma.double(), beta.double(), 1e-12)
    _check_ln("embed_ln.clamp", o32, o16, ref, unit, T16[1])


# ------------------------------------------------------------------------------------------------ cross-encoder embeddings
def _ce_positions(T, s_text, vis_pos0):
    if s_text < 0 or s_text > T:
        return list(range(T))
    return [t if t < s_text else vis_pos0 + (t - s_text) for t in range(T)]


@pytest.mark.parametrize("T,s_text,vis_pos0", [(40, 25, 32), (40, 25, 25), (40, 0, 6), (40, -1, 0), (40, 41, 50), (40, 40, 3)])
def test_ce_embed_ln_positions_and_cls_rows(lib, T, s_text, vis_pos0):
    """Bucketed positions (text t < s_text at t, the rest at vis_pos0 + t - s_text), s_text < 0 / > T (plain positions).  cls32:
    the fp32 output of the CLS rows only (the buffer is NaN-filled), bit-identical to the full call, and every 16-bit row."""
    n, cols, eps = 3, 768, 1e-12
    pt = _ce_positions(T, s_text, vis_pos0)
    g, gamma, beta = _params(cols, T + s_text + vis_pos0)
    pos = 2 * torch.randn(max(pt) + 1, cols, generator=g)
    typ0 = torch.randn(cols, generator=g)
    x = torch.randn(n, T, cols, generator=g)
    w = {"c.position_embeddings.weight": pos[pt].double(), "c.token_type_embeddings.weight": typ0[None].double(),
         "c.LayerNorm.weight": gamma.double(), "c.LayerNorm.bias": beta.double()}
    ref = O.bert_embeddings(w, "c", eps, inputs_embeds=x.double()).reshape(n * T, cols)
    _, unit = _ln_ref((x + typ0 + pos[pt][None]).double().reshape(n * T, cols), gamma.double(), beta.double(), eps)
    cls_rows = (torch.arange(n * T) % T == 0).cuda()
    x_d, pos_d, typ0_d, gamma_d, beta_d = x.cuda(), pos.cuda(), typ0.cuda(), gamma.cuda(), beta.cuda()
    for dt in (0, 1):
        out = {}
        with _op_dtype(lib, dt) as t16:
            for cls32 in (0, 1):
                o32 = torch.full((n * T, cols), float("nan"), device="cuda")
                o16 = _filled16((n * T, cols), t16)
                assert lib.rr_op_ce_embed_ln(_ptr(x_d), _ptr(pos_d), _ptr(typ0_d), _ptr(gamma_d), _ptr(beta_d), eps, n * T, T,
                                             cols, _ptr(o32), _ptr(o16), s_text, vis_pos0, cls32, _stream()) == 0
                torch.cuda.synchronize()
                out[cls32] = (o32, o16)
        _check_ln(f"ce_embed_ln.dt{dt}.T{T}.s{s_text}.v{vis_pos0}", *out[0], ref, unit, t16)
        o32, o16 = out[1]
        assert torch.isnan(o32[~cls_rows]).all(), "cls32 wrote a non-CLS fp32 row"
        assert torch.equal(_bits(o32[cls_rows]), _bits(out[0][0][cls_rows]))
        assert torch.equal(_bits(o16), _bits(out[0][1]))


# ------------------------------------------------------------------------------------------------ LayerNorm numerics, every kernel
def _run_ln_family(lib, kind, x, gamma, beta, eps, t16):
    """One LayerNorm-family kernel on the rows x with zero position / type rows (x + 0 + 0 == x exactly)."""
    R, cols = x.shape
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    o32 = torch.full((R, cols), float("nan"), device="cuda")
    o16 = _filled16((R, cols), t16)
    z = torch.zeros(R + 1, cols, device="cuda")
    s = _stream()
    if kind == "layernorm":
        rc = lib.rr_op_layernorm(_ptr(xd), _ptr(gd), _ptr(bd), eps, R, cols, _ptr(o32), _ptr(o16), s)
    elif kind == "embed_ln":
        ids = torch.arange(R, device="cuda")
        rc = lib.rr_op_embed_ln(_ptr(ids), 0, _ptr(xd), _ptr(z), _ptr(z), _ptr(gd), _ptr(bd), eps, R, R, cols, R, 1, _ptr(o32),
                                _ptr(o16), s)
    elif kind == "ce_embed_ln":
        rc = lib.rr_op_ce_embed_ln(_ptr(xd), _ptr(z), _ptr(z), _ptr(gd), _ptr(bd), eps, R, R, cols, _ptr(o32), _ptr(o16), -1, 0, 0, s)
    else:
        o16 = None
        rc = lib.rr_op_vit_embed_ln(_ptr(xd[1:]), _ptr(xd[0]), _ptr(z), _ptr(gd), _ptr(bd), eps, R, R, cols, _ptr(o32), s)
    assert rc == 0
    torch.cuda.synchronize()
    return o32, o16


@pytest.mark.parametrize("kind", ["layernorm", "embed_ln", "ce_embed_ln", "vit_embed_ln"])
@pytest.mark.parametrize("eps", [1e-12, 1e-5])
@pytest.mark.parametrize("dt", [0, 1])
def test_layernorm_family_numerics(lib, kind, eps, dt):
    """Rows of mean 1e3 and standard deviation 1e-2 (the mean's fp32 rounding, scaled by rstd = 1e2, dominates), ordinary rows,
    and constant rows, whose output is exactly beta (the fp32 sums of a constant with few significant bits are exact)."""
    cols = 1024
    g, gamma, beta = _params(cols, 17)
    off = 1e3 + 1e-2 * torch.randn(6, cols, generator=g, dtype=torch.float64)
    plain = 3 * torch.randn(5, cols, generator=g, dtype=torch.float64) + 0.5
    const = torch.tensor([1000.0, -3.5, 0.0, 2.0 ** -10, 96.0], dtype=torch.float64)[:, None].expand(5, cols)
    x = torch.cat([off, plain, const]).float()        # 16 rows; vit_embed_ln takes row 0 as the class embedding
    with _op_dtype(lib, dt) as t16:
        o32, o16 = _run_ln_family(lib, kind, x, gamma, beta, eps, t16)
    ref, unit = _ln_ref(x.double(), gamma.double(), beta.double(), eps)
    _check_ln(f"ln_numerics.{kind}.dt{dt}.eps{eps:g}", o32[:11], None if o16 is None else o16[:11], ref[:11], unit[:11], t16)
    assert torch.equal(_bits(o32[11:]), _bits(beta.cuda().expand(5, cols)))
    if o16 is not None:
        assert torch.equal(_bits(o16), _bits(o32.to(t16)))


# ------------------------------------------------------------------------------------------------ late-interaction rows
def _li(lib, src, dst_shape, t16, *, ids=None, ids_stride=0, n_pairs, rpb, D, T, t_off=0, pair_off=0, bdiv=1, src_batch_off=0,
        normalize=1, maskf=None, split=1 << 30, shift=0, rc=0, dst=None):
    dst = _filled16(dst_shape, t16) if dst is None else dst
    got = lib.rr_op_li_normalize(_ptr(src), _ptr(ids), ids_stride, n_pairs, rpb, D, T, t_off, pair_off, bdiv, src_batch_off,
                                 _ptr(dst), normalize, _ptr(maskf), split, shift, _stream())
    assert got == rc
    torch.cuda.synchronize()
    return dst


def _li_expect(src, mask, normalize, pair_off, bdiv, src_batch_off, n_pairs):
    """float64 rows of every destination pair: src row of batch (p + pair_off) // bdiv - src_batch_off, times its mask, through
    F.normalize (eps 1e-12) as the oracle's query stage does."""
    sb = (torch.arange(n_pairs) + pair_off) // bdiv - src_batch_off
    x = src.double()[sb] * mask.double()[..., None]
    return torch.nn.functional.normalize(x, p=2, dim=-1) if normalize else x


def _check_nearest16(key, got, ref64, t16):
    """got == the 16-bit value nearest ref64; within LI_SLACK (relative) of a rounding midpoint either neighbour is accepted."""
    slack = ref64.abs() * LI_SLACK
    lo, hi = (ref64 - slack).to(t16), (ref64 + slack).to(t16)
    g = _bits(got.cpu())
    ok = (g == _bits(lo)) | (g == _bits(hi))
    near = int((g != _bits(ref64.to(t16))).sum())
    record_margin(f"row_kernels.{key}", not_nearest_within_slack=near, n=int(g.numel()))
    assert bool(ok.all()), f"{key}: {int((~ok).sum())} values are not the nearest 16-bit value"


def _li_rows(dst, t_off, rpb, split, shift):
    return [t_off + j + (shift if j >= split else 0) for j in range(rpb)]


def _check_li(key, dst, expect, rows, normalize, t16):
    n, T = dst.shape[0], dst.shape[1]
    got = dst[:, rows]
    if normalize:
        _check_nearest16(key, got, expect, t16)
    else:
        assert torch.equal(_bits(got.cpu()), _bits(expect.float().to(t16))), key
    rest = [t for t in range(T) if t not in set(rows)]
    assert (_bits(dst[:, rest]) == 0x7fff).all(), f"{key}: a row outside the destination rows was written"


@pytest.mark.parametrize("D", ROW_COLS)
@pytest.mark.parametrize("dt", [0, 1])
def test_li_normalize_ids_mask(lib, dt, D):
    """Text rows (rr_forward): mask id != 0, normalise, rows 0 .. S-1 of each pair's T rows.  Pair 0 row 3 is all-zero after the
    mask (exact zeros), row 4 has a norm below 1e-12 (x / 1e-12, a normal 16-bit number)."""
    n, S, T = 5, 13, 21
    g = torch.Generator().manual_seed(D + dt)
    src = torch.randn(n * S, D, generator=g)
    src[4] = 1e-14 * (1 + torch.rand(D, generator=g))                 # |x| / 1e-12 in [0.01, 0.02]
    ids = torch.randint(1, 100, (n, S), generator=g)
    ids[:, -3:] = 0
    ids[0, 3] = 0
    with _op_dtype(lib, dt) as t16:
        dst = _li(lib, src.cuda(), (n, T, D), t16, ids=ids.cuda(), ids_stride=S, n_pairs=n, rpb=S, D=D, T=T)
    expect = _li_expect(src.view(n, S, D), (ids != 0).double(), 1, 0, 1, 0, n)
    assert (expect[0, 3] == 0).all() and (expect[0, 4].abs() >= 0.0099).all()
    _check_li(f"li_normalize.ids.dt{dt}.D{D}", dst, expect, list(range(S)), 1, t16)
    assert (dst[0, 3].float() == 0).all()


@pytest.mark.parametrize("q_len,P", [(1, 1), (7, 4), (12, 9)])
@pytest.mark.parametrize("dt", [0, 1])
def test_li_normalize_joint_reorder(lib, dt, q_len, P):
    """RerankModel text rows: float mask, [query | image | context] reorder (rows j >= q_len move down by P)."""
    n, S, D = 6, 12, 128
    T = S + P
    g = torch.Generator().manual_seed(q_len * 10 + P + dt)
    src = torch.randn(n * S, D, generator=g)
    maskf = (torch.rand(n, S, generator=g) > 0.3).float()
    with _op_dtype(lib, dt) as t16:
        dst = _li(lib, src.cuda(), (n, T, D), t16, ids=torch.ones(n, S, dtype=torch.long, device="cuda"), ids_stride=S, n_pairs=n,
                  rpb=S, D=D, T=T, maskf=maskf.cuda(), split=q_len, shift=P)
    expect = _li_expect(src.view(n, S, D), maskf, 1, 0, 1, 0, n)
    _check_li(f"li_normalize.joint.dt{dt}.q{q_len}.P{P}", dst, expect, _li_rows(dst, 0, S, q_len, P), 1, t16)


@pytest.mark.parametrize("pair_off,K,q_lo", [(7, 3, 2), (1, 5, 0), (0, 1, 0), (4, 4, 1)])
@pytest.mark.parametrize("dt", [0, 1])
def test_li_normalize_vision_prefix_broadcast(lib, dt, pair_off, K, q_lo):
    """The vision prefix rows of each query broadcast to its K pairs: pair p reads prefix (p + pair_off) // K - q_lo, written at
    t_off = the pair's image position.  pair_off not a multiple of K: the slice starts mid-query."""
    n, PL, D, T, vis = 10, 4, 128, 30, 17
    nq = (n - 1 + pair_off) // K - q_lo + 1
    g = torch.Generator().manual_seed(pair_off * 31 + K + dt)
    src = torch.randn(nq * PL, D, generator=g)
    with _op_dtype(lib, dt) as t16:
        dst = _li(lib, src.cuda(), (n, T, D), t16, n_pairs=n, rpb=PL, D=D, T=T, t_off=vis, pair_off=pair_off, bdiv=K,
                  src_batch_off=q_lo)
    expect = _li_expect(src.view(nq, PL, D), torch.ones(n, PL), 1, pair_off, K, q_lo, n)
    _check_li(f"li_normalize.prefix.dt{dt}.off{pair_off}.K{K}", dst, expect, list(range(vis, vis + PL)), 1, t16)


@pytest.mark.parametrize("dt", [0, 1])
def test_li_normalize_mapping_rows_and_plain_convert(lib, dt):
    """Mapping-network rows at t_off = vis + PL (normalised), then the interaction rerankers' plain convert (normalize 0): query
    rows broadcast to K pairs from mid-query, context rows at t_off = Lq — bit-exact casts."""
    n, np_, D, T, vis, PL = 7, 9, 256, 40, 13, 4
    g = torch.Generator().manual_seed(60 + dt)
    mapped = torch.randn(n * np_, D, generator=g)
    with _op_dtype(lib, dt) as t16:
        dst = _li(lib, mapped.cuda(), (n, T, D), t16, n_pairs=n, rpb=np_, D=D, T=T, t_off=vis + PL)
    expect = _li_expect(mapped.view(n, np_, D), torch.ones(n, np_), 1, 0, 1, 0, n)
    _check_li(f"li_normalize.mapping.dt{dt}", dst, expect, list(range(vis + PL, vis + PL + np_)), 1, t16)

    Lq, Lc, K, pair_off = 6, 11, 4, 3
    nq = (n - 1 + pair_off) // K + 1
    q = torch.randn(nq * Lq, D, generator=g) * 40
    c = torch.randn(n * Lc, D, generator=g) * 40
    with _op_dtype(lib, dt) as t16:
        dst = _li(lib, q.cuda(), (n, Lq + Lc, D), t16, n_pairs=n, rpb=Lq, D=D, T=Lq + Lc, pair_off=pair_off, bdiv=K, normalize=0)
        qx = _li_expect(q.view(nq, Lq, D), torch.ones(n, Lq), 0, pair_off, K, 0, n)
        _check_li(f"li_normalize.plain_q.dt{dt}", dst, qx, list(range(Lq)), 0, t16)
        dst = _li(lib, c.cuda(), None, t16, n_pairs=n, rpb=Lc, D=D, T=Lq + Lc, t_off=Lq, normalize=0, dst=dst)
    assert torch.equal(_bits(dst.cpu()), _bits(torch.cat([qx, c.view(n, Lc, D).double()], 1).float().to(t16)))


# ------------------------------------------------------------------------------------------------ masks and biases
def _bias(m):
    return torch.where(m != 0, 0.0, NEG).float()


@pytest.mark.parametrize("S,P,q_len", [(150, 1, 1), (150, 81, 32), (150, 130, 150), (70, 81, 32), (64, 1, 32)])
def test_joint_masks(lib, S, P, q_len):
    """Instruction token absent, at 0, 1, 2, 63, 64, 65, S-1 and repeated (the first occurrence wins, also when a later lane
    finds its own occurrence first); zero ids inside rows; attention mask differing from ids != 0; instruction_token < 0."""
    tok = 7
    g = torch.Generator().manual_seed(S + P + q_len)
    places = [None, 0, 1, 2, 63, 64, 65, S - 1, (3, 66), (70, 5), (129, 64), (1, 0)]
    places = [p for p in places if p is None or all(v < S for v in (p if isinstance(p, tuple) else (p,)))]
    n = len(places)
    ids = torch.randint(1, 1000, (n, S), generator=g)
    ids[ids == tok] = tok + 1
    ids[torch.rand(n, S, generator=g) < 0.15] = 0
    for r, p in enumerate(places):
        for v in (() if p is None else (p if isinstance(p, tuple) else (p,))):
            ids[r, v] = tok
    am = (torch.rand(n, S, generator=g) > 0.2).long() * torch.randint(1, 3, (n, S), generator=g)
    dummy = torch.zeros(n, S + P, 1)
    ids_d, am_d = ids.cuda(), am.cuda()
    for t in (tok, -1):
        tb = torch.full((n, S), float("nan"), device="cuda")
        lm = torch.full((n, S), float("nan"), device="cuda")
        cb = torch.full((n, S + P), float("nan"), device="cuda")
        assert lib.rr_op_joint_masks(_ptr(ids_d), _ptr(am_d), n, S, P, q_len, t, _ptr(tb), _ptr(lm), _ptr(cb), _stream()) == 0
        torch.cuda.synchronize()
        mask = O.instruction_query_mask(ids, tok if t >= 0 else None)
        _, cm = O.reorder_query_image_context(dummy, mask, q_len, S)
        assert torch.equal(lm.cpu(), mask), f"li_mask, instruction_token {t}"
        assert torch.equal(_bits(tb.cpu()), _bits(_bias(am)))
        assert torch.equal(_bits(cb.cpu()), _bits(_bias(cm))), f"ce_bias, instruction_token {t}"


@pytest.mark.parametrize("S,T", [(37, 37), (37, 70), (129, 200)])
def test_key_bias(lib, S, T):
    n = 5
    g = torch.Generator().manual_seed(S + T)
    ids = torch.randint(0, 4, (n, S), generator=g)
    am = torch.randint(0, 3, (n, S), generator=g)
    tb = torch.full((n, S), float("nan"), device="cuda")
    cb = torch.full((n, T), float("nan"), device="cuda")
    ids_d, am_d = ids.cuda(), am.cuda()
    assert lib.rr_op_key_bias(_ptr(ids_d), _ptr(am_d), n, S, T, _ptr(tb), _ptr(cb), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(tb.cpu()), _bits(_bias(am)))
    ce = torch.cat([_bias(O.token_mask(ids)), torch.zeros(n, T - S)], 1)
    assert torch.equal(_bits(cb.cpu()), _bits(ce))


@pytest.mark.parametrize("pair_off,K", [(0, 1), (5, 1), (2, 3), (7, 4)])
def test_interaction_bias(lib, pair_off, K):
    """[query | context] key bias, the query mask of pair p being row (p + pair_off) // K; each output NULL in turn."""
    n, Lq, Lc = 9, 32, 45
    nq = (n - 1 + pair_off) // K + 1
    g = torch.Generator().manual_seed(pair_off * 7 + K)
    qm = (torch.rand(nq, Lq, generator=g) > 0.3).float()
    cm = (torch.rand(n, Lc, generator=g) > 0.3).float() * 2
    qrow = qm[(torch.arange(n) + pair_off) // K]
    want = {"cat": _bias(torch.cat([qrow, cm], 1)), "q": _bias(qrow), "c": _bias(cm)}
    qm_d, cm_d = qm.cuda(), cm.cuda()
    for null in (None, "cat", "q", "c"):
        out = {k: torch.full(v.shape, float("nan"), device="cuda") for k, v in want.items()}
        p = {k: 0 if k == null else _ptr(v) for k, v in out.items()}
        assert lib.rr_op_interaction_bias(_ptr(qm_d), _ptr(cm_d), n, Lq, Lc, pair_off, K, p["cat"], p["q"], p["c"], _stream()) == 0
        torch.cuda.synchronize()
        for k, v in out.items():
            if k == null:
                assert torch.isnan(v).all()
            else:
                assert torch.equal(_bits(v.cpu()), _bits(want[k])), (k, null)


# ------------------------------------------------------------------------------------------------ ViT front end
@pytest.mark.parametrize("IS,ps", [(224, 32), (224, 14), (336, 14)])
@pytest.mark.parametrize("dt", [0, 1])
def test_vit_im2col(lib, dt, IS, ps):
    B = 2
    Kd = 3 * ps * ps
    Kp = (Kd + 63) // 64 * 64 + 64                  # at least 64 padding columns
    np_ = (IS // ps) ** 2
    px = torch.randn(B, 3, IS, IS, generator=torch.Generator().manual_seed(IS + ps + dt))
    px_d = px.cuda()
    with _op_dtype(lib, dt) as t16:
        out = _filled16((B * np_, Kp), t16)
        assert lib.rr_op_vit_im2col(_ptr(px_d), _ptr(out), B, IS, ps, Kp, _stream()) == 0
        torch.cuda.synchronize()
    cols = torch.nn.functional.unfold(px, kernel_size=ps, stride=ps).transpose(1, 2).reshape(B * np_, Kd)   # clip_vision_forward
    want = torch.cat([cols, torch.zeros(B * np_, Kp - Kd)], 1).to(t16)
    assert torch.equal(_bits(out.cpu()), _bits(want))
    assert (_bits(out[:, Kd:]) == 0).all()


@pytest.mark.parametrize("np_,cols", [(49, 768), (256, 1024), (9, 260), (50, 2048)])
def test_vit_embed_ln(lib, np_, cols):
    """[class_embedding ; patches] + position_embedding -> pre_layrnorm (eps 1e-5), B = 3 images."""
    B, T = 3, np_ + 1
    g, gamma, beta = _params(cols, np_ + cols)
    patches = torch.randn(B, np_, cols, generator=g)
    cls = 3 * torch.randn(cols, generator=g) + 1
    pos = torch.randn(T, cols, generator=g)
    o32 = torch.full((B * T, cols), float("nan"), device="cuda")
    patches_d, cls_d, pos_d, gamma_d, beta_d = patches.cuda(), cls.cuda(), pos.cuda(), gamma.cuda(), beta.cuda()
    assert lib.rr_op_vit_embed_ln(_ptr(patches_d), _ptr(cls_d), _ptr(pos_d), _ptr(gamma_d), _ptr(beta_d), O.VIT_LN_EPS, B * T, T, cols,
                                  _ptr(o32), _stream()) == 0
    torch.cuda.synchronize()
    x = (torch.cat([cls.expand(B, 1, cols), patches], 1) + pos[None]).double().reshape(B * T, cols)
    ref, unit = _ln_ref(x, gamma.double(), beta.double(), O.VIT_LN_EPS)
    _check_ln(f"vit_embed_ln.np{np_}.c{cols}", o32, None, ref, unit, None)


# ------------------------------------------------------------------------------------------------ casts and gathers
def _special_values():
    f = torch.tensor([0.0, -0.0, 65520.0, 65519.0, -65520.0, -65519.0, 65504.0, 65536.0, 3.4028235e38, -3.4028235e38,
                      1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -23,
                      2.0 ** -149, -(2.0 ** -149), 1e-40, 2.0 ** -126 * (1 - 2.0 ** -23), 2.0 ** -126, 2.0 ** -24, 2.0 ** -25,
                      3 * 2.0 ** -26, 6e-8, 1e-6, -1e-6, float("inf"), float("-inf"), float("nan"), -float("nan"), 1.0],
                     dtype=torch.float64).float()
    return f


@pytest.mark.parametrize("n", [4, 4 * (3 * 256 + 5)])
@pytest.mark.parametrize("dt", [0, 1])
def test_cast16(lib, dt, n):
    """Round to nearest even as torch casts: signed zeros, fp16 overflow (65520 -> inf, 65519 -> 65504), ties, fp32 and
    fp16 subnormals; NaN stays NaN (payload not compared)."""
    g = torch.Generator().manual_seed(n + dt)
    x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-30, 30, (n,), generator=g).float())
    sp = _special_values()
    k = min(n, sp.numel())
    x[-k:] = sp[:k]                                 # the ragged last block holds the special values
    x_d = x.cuda()
    with _op_dtype(lib, dt) as t16:
        y = _filled16((n,), t16)
        assert lib.rr_op_cast16(_ptr(x_d), _ptr(y), n, _stream()) == 0
        torch.cuda.synchronize()
    want = x.to(t16)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(y.cpu()), nan)
    assert torch.equal(_bits(y.cpu())[~nan], _bits(want)[~nan])


@pytest.mark.parametrize("elem", [2, 4])
def test_gather_rows(lib, elem):
    """The CLS gather (row 0 of each pair's T rows) and the query broadcast (pair p <- query (p + off) // K - q_lo, all its rows),
    16-bit and fp32 rows: bit-exact copies."""
    dtype = torch.int16 if elem == 2 else torch.int32
    H, n, T = 200, 7, 33
    g = torch.Generator().manual_seed(elem)
    src = torch.randint(-30000, 30000, (n, T, H), generator=g).to(dtype)
    dst = torch.full((n, H), -1, dtype=dtype, device="cuda")
    src_d = src.cuda()
    assert lib.rr_op_gather_rows(_ptr(src_d), _ptr(dst), n, 1, T, H * elem, 0, 1, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), src[:, 0])
    Lq, K, off, q_lo, n = 6, 3, 7, 2, 10
    nq = (n - 1 + off) // K - q_lo + 1
    q = torch.randint(-30000, 30000, (nq, Lq, H), generator=g).to(dtype)
    dst = torch.full((n, Lq, H), -1, dtype=dtype, device="cuda")
    q_d = q.cuda()
    assert lib.rr_op_gather_rows(_ptr(q_d), _ptr(dst), n, Lq, Lq, H * elem, off, K, q_lo, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), q[(torch.arange(n) + off) // K - q_lo])


# ------------------------------------------------------------------------------------------------ classifier heads
@pytest.mark.parametrize("T,cols", [(1, 768), (593, 1024), (5, 260)])
def test_cls_heads(lib, T, cols):
    """logit_k[p] = <h[p, 0], w_k> + b_k over 7 pairs (the last block holds 3); out2 NULL with w2 still valid."""
    n = 7
    g = torch.Generator().manual_seed(T + cols)
    h = torch.randn(n, T, cols, generator=g) * 2
    h[:, 1:] = float("nan")                          # only the CLS rows may be read
    w1, w2 = torch.randn(cols, generator=g) * 0.05, torch.randn(cols, generator=g) * 0.05
    b1, b2 = torch.tensor([0.25]), torch.tensor([-1.5])
    hd, w1_d, b1_d, w2_d, b2_d = h.cuda(), w1.cuda(), b1.cuda(), w2.cuda(), b2.cuda()
    for two in (True, False):
        o1 = torch.full((n,), float("nan"), device="cuda")
        o2 = torch.full((n,), float("nan"), device="cuda")
        assert lib.rr_op_cls_heads(_ptr(hd), T, cols, n, _ptr(w1_d), _ptr(b1_d), _ptr(w2_d), _ptr(b2_d), _ptr(o1),
                                   _ptr(o2) if two else 0, _stream()) == 0
        torch.cuda.synchronize()
        h0 = h[:, 0].double()
        for k, (o, w, b) in enumerate(((o1, w1, b1), (o2, w2, b2)) if two else ((o1, w1, b1),)):
            ref = h0 @ w.double() + float(b)
            unit = U * ((h0 * w.double()).abs().sum(-1) + abs(float(b)))
            units = float(((o.cpu().double() - ref) / unit).abs().max())
            record_margin(f"row_kernels.cls_heads.T{T}.c{cols}.out{k + 1}.two{int(two)}", dot_units=units)
            assert units <= DOT_UNITS, (k, two, units)
        if not two:
            assert torch.isnan(o2).all()


# ------------------------------------------------------------------------------------------------ folded LayerNorm statistics
def _partials(x64):
    """(mean, M2) of every 128-column group of each row (the last group cols - 128 (nparts - 1) wide), rounded to fp32 as the
    residual GEMM's epilogue leaves them."""
    cols = x64.shape[1]
    out = []
    for c0 in range(0, cols, 128):
        blk = x64[:, c0:c0 + 128]
        m = blk.mean(-1)
        out.append(torch.stack([m, ((blk - m[:, None]) ** 2).sum(-1)], -1))
    return torch.stack(out, 1).float()


def _finalize(lib, part, cols, eps, flag=None, range_ss=RANGE_SS_FP16):
    rows, nparts = part.shape[:2]
    stats = torch.full((rows, 2), float("nan"), device="cuda")
    part_d = part.cuda()
    assert lib.rr_op_ln_finalize(_ptr(part_d), nparts, cols, eps, rows, _ptr(stats), _ptr(flag), range_ss, _stream()) == 0
    torch.cuda.synchronize()
    return stats.cpu()


@pytest.mark.parametrize("cols", [128, 768, 776, 1000, 4096])
def test_ln_finalize_statistics(lib, cols):
    """Chan merge of the per-group partials against the float64 statistics of the rows; 776 and 1000 end in a partial group."""
    rows, eps = 300, 1e-12
    g = torch.Generator().manual_seed(cols)
    groups = (cols + 127) // 128
    offs = torch.repeat_interleave(2 * torch.randn(rows, groups, generator=g, dtype=torch.float64), 128, 1)[:, :cols]
    x = 3 * torch.randn(rows, cols, generator=g, dtype=torch.float64) + 0.5 + offs
    x[-20:] = 1e3 + torch.randn(20, cols, generator=g, dtype=torch.float64)
    x = x.float().double()
    st = _finalize(lib, _partials(x), cols, eps)
    mean, var = x.mean(-1), x.var(-1, unbiased=False)
    rstd = 1 / torch.sqrt(var + eps)
    gm = _partials(x)[..., 0].double().abs().amax(-1)
    mu = ((st[:, 0].double() - mean) / (U * (gm + var.sqrt()))).abs().max()
    ru = ((st[:, 1].double() / rstd - 1) / (U * (1 + gm / var.sqrt()))).abs().max()
    record_margin(f"row_kernels.ln_finalize.c{cols}", mean_units=float(mu), rstd_units=float(ru))
    assert mu <= STATS_UNITS and ru <= STATS_UNITS, (float(mu), float(ru))


@pytest.mark.parametrize("case", ["below", "above", "nan", "inf", "bf16_finite", "bf16_nan", "bf16_inf", "no_flag"])
def test_ln_finalize_range_flag(lib, case):
    """The fp16 range guard: raised by a row whose sum of squares reaches range_ss (rows at 0.5x and 2x RR_RANGE_SS_FP16) or is
    not finite; with range_ss = +inf (bf16 operand rows) by the non-finite rows only; stays 0 when no row qualifies.  no_flag:
    range_flag NULL with a row that would raise it — the statistics are those of the call with a flag, bit for bit, and float64's."""
    rows, cols = 37, 768
    g = torch.Generator().manual_seed(3)
    z = torch.randn(rows, cols, generator=g, dtype=torch.float64) + 0.3
    x = z * torch.sqrt(0.5 * RANGE_SS_FP16 / (z * z).sum(-1, keepdim=True))      # every row at 0.5x the limit
    if case in ("above", "bf16_finite", "no_flag"):
        x[11] *= 2.0                                                             # one row at 2x
    if case in ("nan", "bf16_nan"):
        x[20, 5] = float("nan")
    if case in ("inf", "bf16_inf"):
        x[36, 700] = float("inf")
    ss = float("inf") if case.startswith("bf16") else RANGE_SS_FP16
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = _finalize(lib, _partials(x), cols, 1e-12, flag, ss)
    want = {"below": 0, "above": 1, "nan": 1, "inf": 1, "bf16_finite": 0, "bf16_nan": 1, "bf16_inf": 1, "no_flag": 1}
    assert int(flag.item()) == want[case]
    if case == "no_flag":
        st0 = _finalize(lib, _partials(x), cols, 1e-12, None, ss)
        assert torch.equal(_bits(st0), _bits(st))
        mean, var = x.mean(-1), x.var(-1, unbiased=False)
        gm = _partials(x)[..., 0].double().abs().amax(-1)
        assert ((st0[:, 0].double() - mean) / (U * (gm + var.sqrt()))).abs().max() <= STATS_UNITS
        assert ((st0[:, 1].double() * torch.sqrt(var + 1e-12) - 1) / (U * (1 + gm / var.sqrt()))).abs().max() <= STATS_UNITS


# ------------------------------------------------------------------------------------------------ host-side refusals
def test_refusals_launch_nothing(lib):
    """Every failed host check returns before the launch: NULLs that are not optional, misalignment, cols % 4, cols > 2048, sizes
    <= 0 and index forms that would leave the buffers.  Buffers are large enough that a wrongly accepted call stays inside them."""
    s = _stream()
    big, out, ids_t = torch.zeros(1 << 16, device="cuda"), torch.zeros(1 << 16, device="cuda"), torch.zeros(4096, dtype=torch.long,
                                                                                                         device="cuda")
    f, o, ids = big.data_ptr(), out.data_ptr(), ids_t.data_ptr()     # o: the outputs of the calls that are accepted
    f4 = f + 4                                         # 4-byte aligned, not 16
    E = lib.rr_op_embed_ln
    assert E(ids, 0, f, f, f, f, f, 1e-12, 2, 2, 8, 4, 1, o, o + 256, s) == 0
    torch.cuda.synchronize()
    for cols in (2052, 6, 0):
        assert E(ids, 0, f, f, f, f, f, 1e-12, 2, 2, cols, 4, 1, f, f, s) == RR_ERR_BAD_SHAPE
    assert E(ids, 0, f, f, f, f, f, 1e-12, 0, 2, 8, 4, 1, f, f, s) == RR_ERR_BAD_SHAPE
    assert E(ids, 0, f, f, f, f, f, 1e-12, 2, 2, 8, 0, 1, f, f, s) == RR_ERR_BAD_SHAPE
    assert E(ids, 0, f, f, f, f, f, 1e-12, 2, 2, 8, 4, 1, 0, f, s) == RR_ERR_BAD_ARG
    assert E(ids, 0, f, f, f, f, f, 1e-12, 2, 2, 8, 4, 1, f, 0, s) == RR_ERR_BAD_ARG
    assert E(ids, 0, f4, f, f, f, f, 1e-12, 2, 2, 8, 4, 1, f, f, s) == RR_ERR_BAD_ARG
    C_ = lib.rr_op_ce_embed_ln
    assert C_(f, f, f, f, f, 1e-12, 2, 2, 2052, f, f, -1, 0, 0, s) == RR_ERR_BAD_SHAPE
    assert C_(f, f, f, f, f, 1e-12, 2, 2, 8, 0, f, -1, 0, 1, s) == RR_ERR_BAD_ARG          # cls32 still needs the fp32 output
    assert C_(f, f, f, f, f, 1e-12, 2, 2, 8, f, f, 1, -1, 0, s) == RR_ERR_BAD_SHAPE
    L = lib.rr_op_li_normalize
    assert L(f, 0, 0, 2, 4, 8, 4, 0, 0, 1, 0, o, 1, 0, 1 << 30, 0, s) == 0
    torch.cuda.synchronize()
    assert L(f, 0, 0, 2, 4, 2052, 4, 0, 0, 1, 0, f, 1, 0, 1 << 30, 0, s) == RR_ERR_BAD_SHAPE
    assert L(f, 0, 0, 2, 4, 8, 4, 1, 0, 1, 0, f, 1, 0, 1 << 30, 0, s) == RR_ERR_BAD_SHAPE      # t_off + rows > T
    assert L(f, 0, 0, 2, 4, 8, 6, 0, 0, 1, 0, f, 1, 0, 2, 3, s) == RR_ERR_BAD_SHAPE           # reorder past T
    assert L(f, 0, 0, 2, 4, 8, 4, 0, 1, 2, 1, f, 1, 0, 1 << 30, 0, s) == RR_ERR_BAD_SHAPE     # first source batch < 0
    assert L(f, 0, 0, 2, 4, 8, 4, 0, 0, 0, 0, f, 1, 0, 1 << 30, 0, s) == RR_ERR_BAD_SHAPE
    assert L(f, ids, 2, 2, 4, 8, 4, 0, 0, 1, 0, f, 1, 0, 1 << 30, 0, s) == RR_ERR_BAD_SHAPE   # ids rows shorter than the pair
    assert L(f4, 0, 0, 2, 4, 8, 4, 0, 0, 1, 0, f, 1, 0, 1 << 30, 0, s) == RR_ERR_BAD_ARG
    assert L(f, 0, 0, 2, 4, 8, 4, 0, 0, 1, 0, 0, 1, 0, 1 << 30, 0, s) == RR_ERR_BAD_ARG
    assert lib.rr_op_key_bias(ids, ids, 2, 4, 3, f, f, s) == RR_ERR_BAD_SHAPE
    assert lib.rr_op_key_bias(ids, ids, 2, 4, 4, f, 0, s) == RR_ERR_BAD_ARG
    assert lib.rr_op_key_bias(ids, ids, 0, 4, 4, f, f, s) == RR_ERR_BAD_SHAPE
    J = lib.rr_op_joint_masks
    assert J(ids, ids, 2, 4, 1, 5, 7, f, f, f, s) == RR_ERR_BAD_SHAPE
    assert J(ids, ids, 2, 4, -1, 2, 7, f, f, f, s) == RR_ERR_BAD_SHAPE
    for k in range(5):
        p = [ids, ids, f, f, f]
        p[k] = 0
        assert J(p[0], p[1], 2, 4, 1, 2, 7, p[2], p[3], p[4], s) == RR_ERR_BAD_ARG
    I_ = lib.rr_op_interaction_bias
    assert I_(0, f, 2, 4, 4, 0, 1, f, f, f, s) == RR_ERR_BAD_ARG
    assert I_(f, 0, 2, 4, 4, 0, 1, f, f, f, s) == RR_ERR_BAD_ARG
    assert I_(f, f, 2, 4, 4, 0, 0, f, f, f, s) == RR_ERR_BAD_SHAPE
    assert lib.rr_op_vit_im2col(f, f, 1, 28, 14, 500, s) == RR_ERR_BAD_SHAPE                   # Kp < 3 ps^2
    assert lib.rr_op_vit_im2col(f, 0, 1, 28, 14, 640, s) == RR_ERR_BAD_ARG
    assert lib.rr_op_vit_embed_ln(f, f, f, f, f, 1e-5, 2, 2, 2052, f, s) == RR_ERR_BAD_SHAPE
    assert lib.rr_op_vit_embed_ln(f, f, f, f, f, 1e-5, 2, 2, 8, 0, s) == RR_ERR_BAD_ARG
    assert lib.rr_op_vit_embed_ln(f, f4, f, f, f, 1e-5, 2, 2, 8, f, s) == RR_ERR_BAD_ARG
    assert lib.rr_op_cast16(f, f, 6, s) == RR_ERR_BAD_SHAPE
    assert lib.rr_op_cast16(f, f, 0, s) == RR_ERR_BAD_SHAPE
    assert lib.rr_op_cast16(f4, f, 8, s) == RR_ERR_BAD_ARG
    G = lib.rr_op_gather_rows
    assert G(f, f, 2, 1, 4, 24, 0, 1, 0, s) == RR_ERR_BAD_SHAPE                               # row bytes % 16
    assert G(f, f, 2, 5, 4, 32, 0, 1, 0, s) == RR_ERR_BAD_SHAPE                               # rows_take > rows per batch
    assert G(f, f, 2, 1, 4, 32, 1, 2, 1, s) == RR_ERR_BAD_SHAPE
    assert G(f4, f, 2, 1, 4, 32, 0, 1, 0, s) == RR_ERR_BAD_ARG
    H_ = lib.rr_op_cls_heads
    assert H_(f, 1, 8, 2, f, f, 0, 0, f, 0, s) == RR_ERR_BAD_ARG                             # w2 is read even without out2
    assert H_(f, 1, 8, 2, f, f, f, 0, f, f, s) == RR_ERR_BAD_ARG                             # out2 needs b2
    assert H_(f, 1, 8, 2, f, 0, f, f, f, f, s) == RR_ERR_BAD_ARG
    assert H_(f, 1, 6, 2, f, f, f, f, f, f, s) == RR_ERR_BAD_SHAPE
    assert H_(f, 1, 8, 0, f, f, f, f, f, f, s) == RR_ERR_BAD_SHAPE
    F_ = lib.rr_op_ln_finalize
    assert F_(f, 6, 768, 1e-12, 2, o, 0, RANGE_SS_FP16, s) == 0
    torch.cuda.synchronize()
    assert F_(f, 7, 776, 1e-12, 2, o, 0, RANGE_SS_FP16, s) == 0
    torch.cuda.synchronize()
    assert F_(f, 6, 776, 1e-12, 2, f, 0, RANGE_SS_FP16, s) == RR_ERR_BAD_SHAPE
    assert F_(f, 6, 768, 1e-12, 0, f, 0, RANGE_SS_FP16, s) == RR_ERR_BAD_SHAPE
    assert F_(f4, 6, 768, 1e-12, 2, f, 0, RANGE_SS_FP16, s) == RR_ERR_BAD_ARG
    assert F_(f, 6, 768, 1e-12, 2, 0, 0, RANGE_SS_FP16, s) == RR_ERR_BAD_ARG
