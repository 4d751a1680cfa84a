"""Every launch form of the attention kernel at op level (rr_op_attention_ex, rr_op_attention_segs) and the attention-fusion
bias builders (rr_op_fusion_adj, rr_op_fusion_adj_segs): the one-launch segmented kernels and their per-segment redo, the
reversed walk of large grids, the dense-bias online kernel, the fixed-reference schedule on short rows, q_batch_off.

Two references: exact softmax attention in float64 (helpers.attn_ref) and the device's rounding points
(helpers.attn_emulation = oracle.multi_head_attention_bf16, output rounded to the operand type).  Gates: bitwise equality
where the design promises it; elsewhere max |kernel - emulation| <= GATE (measured on an MI355X, see GATE) and the kernel's
drift from float64 at most DRIFT_FACTOR times the emulation's own."""
import ctypes as C
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from helpers import O, attn_emulation, attn_ref, record_margin

pytestmark = pytest.mark.gpu

RR_ERR_BAD_SHAPE = -2
T16 = {0: torch.bfloat16, 1: torch.float16}
# max |kernel - emulation| per operand type, measured on an MI355X over every case of this file (parity_margins.json keys
# attention_forms.*): bf16 0.0156, fp16 0.00195, one unit in the last place at |O| in [2, 4) — largest where Tk = 1 and the
# fixed-reference form returns v through a 16-bit P of about 1 divided by its unrounded fp32 sum, which the emulation (P = 1
# exactly) does not round.  The gate is that measured value.
GATE = {0: 2.0 ** -6, 1: 2.0 ** -9}
# drift from float64 <= DRIFT_FACTOR x max(the emulation's drift, one output rounding at |O| in [2, 4)): the floor covers cases the
# emulation reproduces exactly (Tk = 1).  Measured ratio: at most 2.1 (short segments and short rows, both operand types).
DRIFT_FACTOR = 3.0
FUSION_GATE = 1e-6         # builders vs float64, per unit of the multiplier (measured: 7.8e-7)

@pytest.fixture(scope="module")
def lib():
    import rmr_amd  # noqa: F401
    from rmr_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@contextmanager
def _op_dtype(lib, dt):
    assert lib.rr_set_op_dtype(dt) == 0
    try:
        yield T16[dt]
    finally:
        lib.rr_set_op_dtype(0)


@contextmanager
def _redo_stats(lib):
    st = torch.zeros(2, dtype=torch.int64, device="cuda")
    assert lib.rr_set_attn_redo_stats(st.data_ptr()) == 0
    try:
        yield st
    finally:
        lib.rr_set_attn_redo_stats(None)


def _ptr(t, elems=0):
    return t.data_ptr() + elems * t.element_size() if t is not None else 0


def _attn(lib, q, k, v, bias, heads, *, qdiv=1, qoff=0, B=None, dense=None, sched=0, mode=-1, rc=0):
    """rr_op_attention_ex on contiguous q [Bq, Tq, H], k / v [B, Tk, H]; dense [B, Tq, ld] or None."""
    B = k.shape[0] if B is None else B
    Tq, Tk, H = q.shape[1], k.shape[1], q.shape[2]
    out = torch.full((B, Tq, H), float("nan"), dtype=q.dtype, device="cuda")
    got = lib.rr_op_attention_ex(_ptr(q), _ptr(k), _ptr(v), H, H, _ptr(bias), B, heads, Tq, Tk, qdiv, qoff, _ptr(out), H,
                                 _ptr(dense), dense.shape[2] if dense is not None else 0, sched, mode, _stream())
    assert got == rc
    torch.cuda.synchronize()
    return out


def _check(key, got, q, k, v, bias, heads, **kw):
    """got against both references; records the margins, then applies GATE and DRIFT_FACTOR."""
    dt = 1 if q.dtype == torch.float16 else 0
    exact = attn_ref(q, k, v, bias, heads, **kw)
    emu = attn_emulation(q, k, v, bias, heads, **kw)
    g = got.double()
    assert torch.isfinite(g).all(), key
    e_emu = (g - emu).abs().max().item()
    d_got, d_emu = (g - exact).abs().max().item(), (emu - exact).abs().max().item()
    return dict(key=key, dt=dt, vs_emulation=e_emu, drift=d_got, emulation_drift=d_emu)


def _gate(stats, name):
    """Fold a list of _check results into one margin record per operand type and assert each against the gates."""
    def ratio(x):
        return x["drift"] / max(x["emulation_drift"], GATE[x["dt"]] / 2)

    for dt in (0, 1):
        s = [x for x in stats if x["dt"] == dt]
        if not s:
            continue
        worst, r = max(s, key=lambda x: x["vs_emulation"]), max(s, key=ratio)
        record_margin(f"attention_forms.{name}.{'fp16' if dt else 'bf16'}", vs_emulation=worst["vs_emulation"],
                      worst_case=worst["key"], drift_ratio=ratio(r), drift_ratio_case=r["key"], gate=GATE[dt], cases=len(s))
    for x in stats:
        assert x["vs_emulation"] <= GATE[x["dt"]], x
        assert ratio(x) <= DRIFT_FACTOR, x


def _ulp_close(got, want, dt):
    """|got - want| <= one unit in the last place of the 16-bit output (want in float64)."""
    eps = 2.0 ** -7 if dt == torch.bfloat16 else 2.0 ** -10
    return bool(((got.double() - want).abs() <= eps * want.abs() + 1e-6).all())


def _key_bias(g, B, Tk, patterns):
    """[B, Tk] 0 / -1e30: pattern per sequence 'none' | 'tail' | 'left' | 'all' | 'rand'; every other pattern keeps >= 1 key."""
    bias = torch.zeros(B, Tk)
    for b in range(B):
        p = patterns[b % len(patterns)]
        if p == "tail" and Tk > 1:
            bias[b, int(torch.randint(1, Tk, (1,), generator=g)):] = -1e30
        elif p == "left" and Tk > 1:
            bias[b, :int(torch.randint(1, Tk, (1,), generator=g))] = -1e30
        elif p == "rand":
            keep = torch.rand(Tk, generator=g) > 0.4
            keep[int(torch.randint(0, Tk, (1,), generator=g))] = True
            bias[b] = torch.where(keep, 0.0, -1e30)
        elif p == "all":
            bias[b] = -1e30
    return bias


def _spike(q, k, b, head, ki, amount):
    """Every query row of sequence b, head `head`, becomes one small vector u and key ki becomes u * amount / |u|^2: all of the
    (sequence, head)'s rows score `amount` (log2 domain) on key ki and little on the others (|u . k| ~ 0.6), so every workgroup of
    that (sequence, head), and no other, meets the trigger."""
    cols = slice(head * 64, (head + 1) * 64)
    u = q[b, 0, cols].float() * 0.3
    q[b, :, cols] = u
    k[b, ki, cols] = u * (amount / float((u ** 2).sum()))


# ---- segmented (packed) self-attention ----------------------------------------------------------------------------------
class Segs:
    """A packed layer: segment s = n[s] sequences of len[s] rows, back to back; q / k / v / key bias per row."""

    def __init__(self, lens, ns, heads, t16, seed, patterns=("tail", "left", "none", "rand"), scale=0.25):
        g = torch.Generator().manual_seed(seed)
        self.lens, self.ns, self.heads, self.H = list(lens), list(ns), heads, heads * 64
        self.row0 = np.cumsum([0] + [n * L for n, L in zip(ns, lens)])[:-1].astype(np.int64)
        R = int(sum(n * L for n, L in zip(ns, lens)))
        self.q = torch.randn(R, self.H, generator=g) * scale
        self.k = torch.randn(R, self.H, generator=g)
        self.v = torch.randn(R, self.H, generator=g)
        self.bias = torch.cat([_key_bias(g, n, L, patterns).flatten() for n, L in zip(ns, lens)])
        self.t16 = t16

    def view(self, x, s):
        r0, n, L = int(self.row0[s]), self.ns[s], self.lens[s]
        return x[r0:r0 + n * L].view(n, L, -1)

    def device(self):
        return (self.q.to(self.t16).cuda(), self.k.to(self.t16).cuda(), self.v.to(self.t16).cuda(), self.bias.cuda())

    def run(self, lib, sched, mode, rc=0):
        q, k, v, bias = self.device()
        out = torch.full_like(q, float("nan"))
        nseg = len(self.lens)
        sn, sl = np.array(self.ns, np.int32), np.array(self.lens, np.int32)
        got = lib.rr_op_attention_segs(_ptr(q), self.H, _ptr(k), _ptr(v), self.H, _ptr(bias), self.heads, nseg, sn.ctypes.data,
                                       sl.ctypes.data, self.row0.ctypes.data, _ptr(out), self.H, sched, mode, _stream())
        assert got == rc
        torch.cuda.synchronize()
        return out

    def run_per_segment(self, lib, sched, mode):
        q, k, v, bias = self.device()
        out = torch.full_like(q, float("nan"))
        for s in range(len(self.lens)):
            r0, n, L = int(self.row0[s]), self.ns[s], self.lens[s]
            assert lib.rr_op_attention_ex(_ptr(q, r0 * self.H), _ptr(k, r0 * self.H), _ptr(v, r0 * self.H), self.H, self.H,
                                          _ptr(bias, r0), n, self.heads, L, L, 1, 0, _ptr(out, r0 * self.H), self.H, 0, 0,
                                          sched, mode, _stream()) == 0
        torch.cuda.synchronize()
        return out

    def check(self, key, out):
        q, k, v, bias = self.device()
        return [_check(f"{key}.seg{s}", self.view(out, s), self.view(q, s), self.view(k, s), self.view(v, s),
                       self.view(bias, s).view(self.ns[s], self.lens[s]), self.heads) for s in range(len(self.lens))]


SEG_LENS = [1, 7, 63, 64, 65, 255, 256, 257, 700]
SEG_NS = [1, 3, 17]


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("heads", [12, 1])
def test_segments_one_launch_equals_per_segment_launches(lib, dt, heads):
    """rr_op_attention_segs (one fixed-reference launch over all segments + one redo launch) against one rr_op_attention_ex per
    segment with the same schedule_blocks: bit for bit for every fixed_mode (1 / 2 / 3 all take the 64-row form in the one
    launch; per segment, 1 takes the 32-row form, which is bitwise the same), and the online form (fixed_mode 0) per segment.
    Lengths around the 64-key tile and the 256-row workgroup, 1 / 3 / 17 sequences per segment (heads = 1: groups round to 8),
    tail, left and random key padding."""
    with _op_dtype(lib, dt) as t16:
        sg = Segs(SEG_LENS, [SEG_NS[i % 3] for i in range(len(SEG_LENS))], heads, t16, seed=100 + 10 * dt + heads)
        outs, stats = {}, []
        for mode in (0, 1, 2, 3):
            one = sg.run(lib, 4096, mode)
            per = sg.run_per_segment(lib, 4096, mode)
            assert torch.equal(one, per), f"fixed_mode {mode}: one launch != per-segment launches"
            outs[mode] = one
            stats += sg.check(f"segs.h{heads}.mode{mode}", one)
        assert torch.equal(outs[1], outs[2]) and torch.equal(outs[2], outs[3])     # 32- and 64-row fixed forms
        assert not torch.equal(outs[0], outs[2])                                   # ... and the fixed form did run
    _gate(stats, "segments")


@pytest.mark.parametrize("nseg", [64, 65])
def test_segment_table_limit(lib, nseg):
    """ATTN_MAX_SEGS = 64 segments go in one launch; 65 fall back to one launch per segment.  Both bitwise equal to the
    per-segment calls and within the gates."""
    lens = [SEG_LENS[(4 * i) % len(SEG_LENS)] for i in range(nseg)]
    ns = [1 + i % 2 for i in range(nseg)]
    sg = Segs(lens, ns, 2, torch.bfloat16, seed=nseg)
    one = sg.run(lib, 2048, 3)
    assert torch.equal(one, sg.run_per_segment(lib, 2048, 3))
    _gate(sg.check(f"seg_limit{nseg}", one), f"segment_limit{nseg}")


@pytest.mark.parametrize("dt", [0, 1])
def test_segments_redo_recomputes_the_flagged_workgroups(lib, dt):
    """Redo triggers in segments 2 and later: a sequence with no valid key (every workgroup of its heads flagged), a +230 spike in
    one head (a row sum beyond 2^64), and with fp16 operands a +20 spike (P beyond 65504).  The redo launch maps its flagged
    workgroups back to their segment (seg_of): the redo statistics count exactly those, the recomputed rows equal the online
    form bit for bit, the keyless sequence is uniform over its keys, and every sequence without a trigger is bitwise what the
    same launch gives without any trigger."""
    lens, ns, heads = [65, 130, 300, 257, 64, 513], [3, 2, 4, 2, 5, 2], 4
    with _op_dtype(lib, dt) as t16:
        clean = Segs(lens, ns, heads, t16, seed=7 + dt, patterns=("tail", "none", "left"))
        trig = Segs(lens, ns, heads, t16, seed=7 + dt, patterns=("tail", "none", "left"))
        s_all, b_all = 2, 1                                  # segment 2, sequence 1: no valid key
        r = int(trig.row0[s_all]) + b_all * lens[s_all]
        trig.bias[r:r + lens[s_all]] = -1e30
        q3, k3 = trig.view(trig.q, 3), trig.view(trig.k, 3)
        trig.bias[int(trig.row0[3]):int(trig.row0[3]) + lens[3]] = 0.0     # sequence 0 of segment 3: every key valid
        _spike(q3, k3, 0, 2, 230, 230.0)                    # segment 3 (257 rows), sequence 0, head 2: 2 workgroups
        spikes = [(3, 0, 2)]
        if dt == 1:
            q5, k5 = trig.view(trig.q, 5), trig.view(trig.k, 5)
            trig.bias[int(trig.row0[5]) + lens[5]:int(trig.row0[5]) + 2 * lens[5]] = 0.0
            _spike(q5, k5, 1, 1, 400, 20.0)                  # segment 5 (513 rows), sequence 1, head 1: 3 workgroups
            spikes.append((5, 1, 1))
        expected = heads * ((lens[s_all] + 255) // 256) + sum((lens[s] + 255) // 256 for s, _, _ in spikes)
        with _redo_stats(lib) as st:
            got = trig.run(lib, 4096, 2)
            torch.cuda.synchronize()
            flagged, looked = st.tolist()
        assert flagged == expected and flagged > 0, (flagged, expected)
        assert looked == sum(((n * heads + 7) // 8) * 8 * ((L + 255) // 256) for n, L in zip(ns, lens))
        online = trig.run(lib, 4096, 0)
        base = clean.run(lib, 4096, 2)
        # the recomputed workgroups ARE the online form
        assert torch.equal(trig.view(got, s_all)[b_all], trig.view(online, s_all)[b_all])
        for s, b, h in spikes:
            assert torch.equal(trig.view(got, s)[b, :, h * 64:(h + 1) * 64], trig.view(online, s)[b, :, h * 64:(h + 1) * 64])
        v_all = trig.view(trig.v, s_all)[b_all].to(t16).double().cuda()
        assert _ulp_close(trig.view(got, s_all)[b_all], v_all.mean(0, keepdim=True).expand_as(v_all), t16)
        touched = {(s_all, b_all)} | {(s, b) for s, b, _ in spikes}
        for s in range(len(lens)):
            for b in range(ns[s]):
                if (s, b) not in touched:
                    assert torch.equal(trig.view(got, s)[b], clean.view(base, s)[b]), (s, b)
        stats = trig.check("segs_redo", got)
    _gate(stats, "segments_redo")


def test_reversed_walk_with_redo(lib):
    """Launches of >= 2 048 workgroups of 256 rows walk the (sequence, head) groups of each XCD's chunk in alternating
    directions; the redo launch must map its flagged workgroups with the same direction.  Triggers in the first and the last
    groups and one keyless sequence; with m_alternate = 1 two consecutive launches take both directions: both equal, bit for bit,
    to a launch with m_alternate = 0, with the same redo count."""
    B, heads, T = 96, 12, 400                      # 96 x 12 groups x 2 query blocks of 256 = 2 304 workgroups
    H = heads * 64
    g = torch.Generator().manual_seed(21)
    q = torch.randn(B, T, H, generator=g) * 0.25
    k = torch.randn(B, T, H, generator=g)
    v = torch.randn(B, T, H, generator=g)
    bias = _key_bias(g, B, T, ("tail", "none", "left"))
    bias[0] = 0.0
    bias[95] = 0.0
    _spike(q, k, 0, 0, 350, 230.0)                 # group 0 (sequence 0, head 0): 2 workgroups
    _spike(q, k, 95, 11, 200, 230.0)               # group 1151: 2 workgroups
    bias[1] = -1e30                                # groups 12..23: 24 workgroups
    q, k, v, bias = q.bfloat16().cuda(), k.bfloat16().cuda(), v.bfloat16().cuda(), bias.cuda()
    outs, counts = [], []
    try:
        for alt in (1, 1, 0):
            if alt == 1 and not outs:
                assert lib.rr_set_tuning(b"m_alternate", 1) == 0    # resets the launch counter: ascending, then descending
            if alt == 0:
                assert lib.rr_set_tuning(b"m_alternate", 0) == 0
            with _redo_stats(lib) as st:
                outs.append(_attn(lib, q, k, v, bias, heads, mode=3))
                counts.append(st.tolist()[0])
        online = _attn(lib, q, k, v, bias, heads, mode=0)
    finally:
        lib.rr_set_tuning(b"m_alternate", 1)
        lib.rr_set_tuning(b"attn_fixed_ref", -1)
    assert counts == [28, 28, 28], counts
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])
    assert torch.equal(outs[0][0, :, :64], online[0, :, :64])
    assert torch.equal(outs[0][95, :, 11 * 64:], online[95, :, 11 * 64:])
    assert torch.equal(outs[0][1], online[1])
    assert not torch.equal(outs[0][2:95], online[2:95])
    sel = [0, 1, 2, 47, 94, 95]
    _gate([_check("reversed_walk", outs[0][sel], q[sel], k[sel], v[sel], bias[sel], heads)], "reversed_walk")


@pytest.mark.parametrize("dt", [0, 1])
def test_short_rows_under_the_fixed_schedule(lib, dt):
    """The forwards force the fixed-reference schedule on small launches through schedule_blocks (the padded call's grid):
    MORES cross-attention (Tq != Tk), packed segments, the CLS-only layer (Tq = 1).  Tk < 64 is one partial tile.  The 32- and
    64-row fixed forms bitwise equal; both and the online form within the gates."""
    stats = []
    with _op_dtype(lib, dt) as t16:
        for Tq in (1, 17, 129, 256, 257):
            for Tk in (1, 7, 63, 64, 65, 130):
                g = torch.Generator().manual_seed(1000 * Tq + Tk)
                B, heads = 3, 2
                q = (torch.randn(B, Tq, 128, generator=g) * 0.25).to(t16).cuda()
                k = torch.randn(B, Tk, 128, generator=g).to(t16).cuda()
                v = torch.randn(B, Tk, 128, generator=g).to(t16).cuda()
                bias = _key_bias(g, B, Tk, ("none", "left", "tail")).cuda()
                f1 = _attn(lib, q, k, v, bias, heads, sched=1024, mode=1)
                f2 = _attn(lib, q, k, v, bias, heads, sched=1024, mode=2)
                on = _attn(lib, q, k, v, bias, heads, sched=1024, mode=0)
                assert torch.equal(f1, f2), (Tq, Tk)
                stats.append(_check(f"short.{Tq}x{Tk}.fixed", f1, q, k, v, bias, heads))
                stats.append(_check(f"short.{Tq}x{Tk}.online", on, q, k, v, bias, heads))
    _gate(stats, "short_rows")


# ---- dense (attention-fusion) bias --------------------------------------------------------------------------------------
def _fusion_bias(g, builder, B, T, mult):
    if T == 1:
        return torch.randn(B, 1, 1, generator=g) * mult
    if builder == "joint":                         # fusion_adjacency: T = P + S tokens [query | image | context]
        ql, S = 3, max(4, T // 2)
        P = T - S
        return O.fusion_adjacency(torch.randn(B, S, ql + P, generator=g) * 3.0, ql, P, S, float(mult))
    Lq = max(1, T // 3)
    return O.interaction_fusion_adjacency(torch.randn(B, T - Lq, Lq, generator=g) * 3.0, float(mult))


@pytest.mark.parametrize("builder", ["joint", "interaction"])
@pytest.mark.parametrize("dt", [0, 1])
def test_dense_bias_online_kernel(lib, dt, builder):
    """attn_fwd_kernel<DT, true>: T around the tile and beyond 1 024 keys (bias-chunk reload), dense_ld with and without 64
    columns of slack whose junk (1e3) must not leak, fusion multipliers 1 and 20, a tail-padded and a keyless sequence (uniform
    over all Tk keys, as finfo.min + adj gives).  A fixed_mode > 0 launch on a large schedule still runs the online form."""
    stats = []
    with _op_dtype(lib, dt) as t16:
        for T in (1, 50, 64, 200, 1100):
            for slack in (0, 64):
                for mult in (1, 20):
                    g = torch.Generator().manual_seed(T * 7 + slack + mult)
                    B, heads = 3, 2
                    ld = (T + 63) // 64 * 64 + slack
                    adj = _fusion_bias(g, builder, B, T, mult).float()
                    dense = torch.full((B, T, ld), 1e3)
                    dense[:, :, :T] = adj
                    dense = dense.cuda()
                    q = (torch.randn(B, T, 128, generator=g) * 0.25).to(t16).cuda()
                    k = torch.randn(B, T, 128, generator=g).to(t16).cuda()
                    v = torch.randn(B, T, 128, generator=g).to(t16).cuda()
                    bias = _key_bias(g, B, T, ("none", "tail", "all")).cuda()
                    got = _attn(lib, q, k, v, bias, heads, dense=dense)
                    fixed = _attn(lib, q, k, v, bias, heads, dense=dense, sched=1 << 20, mode=3)
                    assert torch.equal(got, fixed), (T, slack, mult)
                    stats.append(_check(f"dense.{builder}.T{T}.ld{ld}.m{mult}", got, q, k, v, bias, heads, dense=adj.cuda()))
                    want = v[2].double().mean(0, keepdim=True).expand(T, 128)
                    assert _ulp_close(got[2], want, t16), (T, slack, mult)
        # refusals: dense_ld below Tk, dense_ld not a multiple of 64
        q = torch.zeros(1, 200, 64, dtype=t16, device="cuda")
        for ld in (128, 256 + 32):
            d = torch.zeros(1, 200, ld, device="cuda")
            _attn(lib, q, q, q, None, 1, dense=d, rc=RR_ERR_BAD_SHAPE)
    _gate(stats, f"dense_{builder}")


# ---- fusion-bias builders ------------------------------------------------------------------------------------------------
def _adj_ref(scores, form, Tq, Tc, mult):
    """The oracle's adjacency over [Tq query / image tokens | Tc context tokens] of each pair, float64."""
    s = scores.double()
    if form == "joint" and Tq >= 3:                # fusion_adjacency cuts the context rows [2, 2 - ql) of scores [N, S, ql + P]
        return O.fusion_adjacency(s, 3, Tq - 3, Tc + 3, float(mult))
    row0 = 2 if form == "joint" else 0
    return O.interaction_fusion_adjacency(s[:, row0:row0 + Tc], float(mult))


@pytest.mark.parametrize("form", ["joint", "interaction"])
def test_fusion_bias_builders(lib, form):
    """fusion_adj_kernel (padded call, pairs pair0..) and fusion_adj_segs_kernel (packed call: segments whose sequences end after
    Tk < Tc context tokens, normalised over all Tc) against the oracle adjacencies in float64.  Tq = 300 exceeds the 256 threads
    of a workgroup.  Outputs pre-filled with NaN: every written element finite, the padding columns exactly 0, nothing beyond."""
    row0 = 2 if form == "joint" else 0
    worst = 0.0
    for Tq in (1, 81, 300):
        for Tc in (1, 64, 200):
            g = torch.Generator().manual_seed(Tq * 1000 + Tc)
            S = Tc + 3 if form == "joint" else Tc
            N, pair0, n = 6, 2, 3
            scores = torch.randn(N, S, Tq, generator=g) * 3.0
            sc = scores.cuda()
            for mult in (1.0, 20.0):
                # padded
                T = Tq + Tc
                ld = (T + 63) // 64 * 64
                out = torch.full((n * T * ld + 64,), float("nan"), device="cuda")
                assert lib.rr_op_fusion_adj(_ptr(sc), S, Tq, Tc, C.c_float(mult), pair0, n, _ptr(out), ld, row0, _stream()) == 0
                torch.cuda.synchronize()
                a = out[:n * T * ld].view(n, T, ld).cpu()
                assert torch.isnan(out[n * T * ld:]).all()
                assert torch.isfinite(a).all() and (a[:, :, T:] == 0).all(), (Tq, Tc)
                ref = _adj_ref(scores[pair0:pair0 + n], form, Tq, Tc, mult)
                err = (a[:, :, :T].double() - ref).abs().max().item() / mult
                worst = max(worst, err)
                assert err <= FUSION_GATE, (Tq, Tc, mult, err)
                # packed: 3 segments of 2 / 1 / 3 pairs, Tk = Tc, about Tc / 2 and Tc - 7 context tokens
                sn = np.array([2, 1, 3], np.int32)
                tk = np.array([Tc, max(1, Tc // 2), max(1, Tc - 7)], np.int32)
                sizes = [int(sn[s]) * (Tq + int(tk[s])) * ((Tq + int(tk[s]) + 63) // 64 * 64) for s in range(3)]
                out = torch.full((sum(sizes) + 64,), float("nan"), device="cuda")
                assert lib.rr_op_fusion_adj_segs(_ptr(sc), S, Tq, Tc, C.c_float(mult), 3, sn.ctypes.data, tk.ctypes.data, _ptr(out),
                                                 row0, _stream()) == 0
                torch.cuda.synchronize()
                assert torch.isnan(out[sum(sizes):]).all()
                full = _adj_ref(scores, form, Tq, Tc, mult)
                off, p = 0, 0
                for s in range(3):
                    Ts = Tq + int(tk[s])
                    lds = (Ts + 63) // 64 * 64
                    a = out[off:off + sizes[s]].view(int(sn[s]), Ts, lds).cpu()
                    assert torch.isfinite(a).all() and (a[:, :, Ts:] == 0).all(), (Tq, Tc, s)
                    err = (a[:, :, :Ts].double() - full[p:p + int(sn[s]), :Ts, :Ts]).abs().max().item() / mult
                    worst = max(worst, err)
                    assert err <= FUSION_GATE, (Tq, Tc, s, mult, err)
                    off += sizes[s]
                    p += int(sn[s])
    record_margin(f"attention_forms.fusion_builders.{form}", max_abs_per_mult=worst, gate=FUSION_GATE)
    # refusals
    sc = torch.zeros(4, 300, 81, device="cuda")
    out = torch.zeros(1 << 20, device="cuda")
    one = np.array([1] * 65, np.int32)
    f = C.c_float(1.0)
    assert lib.rr_op_fusion_adj(_ptr(sc), 300, 81, 100, f, 0, 2, _ptr(out), 128, row0, _stream()) == RR_ERR_BAD_SHAPE   # ld < Tq + Tc
    assert lib.rr_op_fusion_adj(_ptr(sc), 300, 81, 100, f, 0, 2, _ptr(out), 200, row0, _stream()) == RR_ERR_BAD_SHAPE   # ld % 64
    assert lib.rr_op_fusion_adj(_ptr(sc), 300, 8193, 1, f, 0, 1, _ptr(out), 8256, row0, _stream()) == RR_ERR_BAD_SHAPE  # Tq > 8192
    assert lib.rr_op_fusion_adj_segs(_ptr(sc), 300, 81, 100, f, 65, one.ctypes.data, one.ctypes.data, _ptr(out), row0,
                                     _stream()) == RR_ERR_BAD_SHAPE                                                     # nseg > 64
    tk = np.array([101], np.int32)
    assert lib.rr_op_fusion_adj_segs(_ptr(sc), 300, 81, 100, f, 1, one.ctypes.data, tk.ctypes.data, _ptr(out), row0,
                                     _stream()) == RR_ERR_BAD_SHAPE                                                     # seg_tk > Tc
    torch.cuda.synchronize()
    assert (out == 0).all()
