"""Attention fusion from the retriever's own late-interaction tensors: `fusion_from_li=True` of the interaction forwards
(rr_forward_interaction_fusion_li / rr_forward_interaction_packed_fusion_li) and the `retriever_*_li` keywords of the joint
forwards.  The scores are what rr_li_scores computes (tests/test_gpu_li_scores.py), so every forward here must equal, bit for
bit, the existing forward fed with `preflmr_scores = li_scores(...)["scores"]`; one test holds the path against the oracle on
scores of the shape a retriever produces (values up to 1, whole rows at -9999)."""
import ast
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, O, arch_from_cfg
from li_scores_ref import aligned_context, li_scores_formula, retriever_inputs

pytestmark = pytest.mark.gpu

MULT = 20.0


def _npz(name):
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False)
    g = {k: z[k] for k in z.files}
    g["cfg"] = O.OracleConfig(**ast.literal_eval(str(g["cfg_json"])))
    g["cfg"].loss_fn = str(g["loss_fn"]) if "loss_fn" in g else "2H_BCE"
    return g


def _int_engine(name, dtype, exact=False, mores=False):
    import rmr_amd
    g = _npz(name)
    arch = arch_from_cfg(g["cfg"], False, dtype)
    arch["model_kind"] = "mores" if mores else "interaction"
    eng = rmr_amd.RerankEngine(arch)
    w = O.make_interaction_weights(g["cfg"], mores, seed=0)
    eng.load_state_dict(w)
    if exact:
        eng.set_option("resid_split", 0)       # the condition include/rerank_mi355.h states for packed = padded, bit for bit
    return eng, g, w


def _int_args(g):
    return [torch.from_numpy(g[k]).cuda() for k in ("query_li", "context_li", "query_mask", "context_mask")]


def _same(a, b, keys=("logits", "logits2", "loss", "scores", "order")):
    for k in keys:
        assert (a.get(k) is None) == (b.get(k) is None), k
        if a.get(k) is not None:
            assert torch.equal(a[k], b[k]), f"{k} differs: {(a[k].float() - b[k].float()).abs().max().item():.3e}"


@pytest.mark.parametrize("name", ["int_tiny", "int_base"])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_padded_from_li_equals_explicit_scores(name, dtype):
    eng, g, _ = _int_engine(name, dtype)
    Bq, K = int(g["Bq"]), int(g["K"])
    N = Bq * K
    args = _int_args(g)
    lab = torch.from_numpy(g["labels"]).cuda() if g["labels"].size else None
    li = eng.li_scores(args[0], args[1], args[3], Bq, K)
    kw = dict(want_scores=True, want_order=True, fusion_multiplier=MULT)
    ref = eng.forward_interaction(*args, Bq, K, lab, preflmr_scores=li["scores"], **kw)
    got = eng.forward_interaction(*args, Bq, K, lab, fusion_from_li=True, want_maxsim=True, **kw)
    plain = eng.forward_interaction(*args, Bq, K, lab)
    torch.cuda.synchronize()
    _same(ref, got)
    assert torch.equal(got["maxsim"], li["maxsim"])
    assert not torch.equal(plain["logits"], got["logits"]), "the fusion bias must reach the logits"
    # pair slices compose (a slice starts inside a query)
    cut = max(1, N // 2 - 1)
    a = eng.forward_interaction(*args, Bq, K, lab, pair_range=(0, cut), fusion_from_li=True, want_maxsim=True, fusion_multiplier=MULT)
    b = eng.forward_interaction(*args, Bq, K, lab, pair_range=(cut, N), fusion_from_li=True, want_maxsim=True, fusion_multiplier=MULT)
    a_ref = eng.forward_interaction(*args, Bq, K, lab, pair_range=(0, cut), preflmr_scores=li["scores"], fusion_multiplier=MULT)
    torch.cuda.synchronize()
    assert torch.equal(a["logits"][:cut], a_ref["logits"][:cut])
    assert torch.equal(torch.cat([a["maxsim"][:cut], b["maxsim"][cut:]]), li["maxsim"])
    assert torch.equal(torch.cat([a["logits"][:cut], b["logits"][cut:]]), got["logits"])


@pytest.mark.parametrize("name", ["int_tiny", "int_base"])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("holes", [False, True])
def test_packed_from_li_equals_padded_and_explicit(name, dtype, holes):
    eng, g, _ = _int_engine(name, dtype, exact=True)
    Bq, K = int(g["Bq"]), int(g["K"])
    N = Bq * K
    args = _int_args(g)
    if holes:                       # retriever-made inputs: holes inside the passages, one pair without a valid token
        q, c, cm = retriever_inputs(Bq, K, args[0].shape[1], args[1].shape[1], args[0].shape[2], seed=21, full_mask_pair=N - 1)
        args = [q.cuda(), c.cuda(), args[2], cm.cuda()]
    li = eng.li_scores(args[0], args[1], args[3], Bq, K)
    kw = dict(want_scores=True, want_order=True, fusion_multiplier=MULT)
    pad = eng.forward_interaction(*args, Bq, K, None, fusion_from_li=True, want_maxsim=True, **kw)
    pk = eng.forward_interaction_packed(*args, Bq, K, None, fusion_from_li=True, want_maxsim=True, granule=16, **kw)
    pk_ref = eng.forward_interaction_packed(*args, Bq, K, None, preflmr_scores=li["scores"], granule=16, **kw)
    torch.cuda.synchronize()
    assert pk["packed_segments"] >= 2 and pk["packed_rows"] < N * args[1].shape[1], "the segment table must cut pairs"
    _same(pad, pk)
    _same(pk_ref, pk)
    assert torch.equal(pk["maxsim"], li["maxsim"])
    # lists of unequal length over the same contexts: one query row per list
    sizes = [1, N - 1] if Bq == 1 else [K - 1, N - K + 1]
    ql = args[0][:1].repeat(2, 1, 1) if Bq == 1 else args[0]
    qml = args[2][:1].repeat(2, 1) if Bq == 1 else args[2]
    per_pair = torch.repeat_interleave(torch.arange(2), torch.tensor(sizes)).cuda()
    li_l = eng.li_scores(ql.index_select(0, per_pair), args[1], args[3], N, 1)
    ls = eng.forward_interaction_packed(ql, args[1], qml, args[3], None, None, None, list_sizes=sizes, fusion_from_li=True,
                                        want_maxsim=True, granule=16, **kw)
    ls_ref = eng.forward_interaction_packed(ql, args[1], qml, args[3], None, None, None, list_sizes=sizes,
                                            preflmr_scores=li_l["scores"], granule=16, **kw)
    torch.cuda.synchronize()
    _same(ls_ref, ls, keys=("logits", "logits2", "loss", "scores", "order", "list_loss"))
    assert torch.equal(ls["maxsim"], li_l["maxsim"])


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_from_li_against_the_same_rounding_oracle(dtype):
    """int_tiny weights, contexts that answer their query (li_scores_ref.aligned_context), fusion_multiplier 20: the device
    forward against O.interaction_forward(preflmr_scores = the formula in torch, mm = the device's rounding), with the gate
    the existing fusion test uses on this geometry (3e-4, tests/test_gpu_interaction.py).  The fp32 oracle must move by at
    least ten gates when the fusion is switched on, or the comparison shows nothing."""
    gate = 3e-4
    eng, g, w = _int_engine("int_tiny", dtype)
    cfg, Bq, K = g["cfg"], int(g["Bq"]), int(g["K"])
    q, c0, qm, cm = (torch.from_numpy(g[k]) for k in ("query_li", "context_li", "query_mask", "context_mask"))
    c = aligned_context(q, c0, qm, cm, K, noise=0.3)
    _, sc = li_scores_formula(q, c, cm, K)
    with torch.no_grad():
        off = O.interaction_forward(cfg, w, q, c, qm, cm, K, None, False)
        on = O.interaction_forward(cfg, w, q, c, qm, cm, K, None, False, preflmr_scores=sc, fusion_multiplier=MULT)
        with O.device_rounding(torch.bfloat16 if dtype == "bf16" else torch.float16) as mm:
            emu = O.interaction_forward(cfg, w, q, c, qm, cm, K, None, False, mm=mm, preflmr_scores=sc, fusion_multiplier=MULT)
    effect = (on.logits - off.logits).abs().max().item()
    r = eng.forward_interaction(q.cuda(), c.cuda(), qm.cuda(), cm.cuda(), Bq, K, None, fusion_from_li=True, fusion_multiplier=MULT)
    torch.cuda.synchronize()
    demu = (r["logits"].cpu().view(-1) - emu.logits.view(-1)).abs().max().item()
    d32 = (r["logits"].cpu().view(-1) - on.logits.view(-1)).abs().max().item()
    print(f"[from_li/{dtype}] fusion moves the fp32 oracle by {effect:.3e}; device vs same-rounding oracle {demu:.3e}, vs fp32 {d32:.3e}")
    assert effect >= 10 * gate
    assert demu <= gate


def test_drop_in_module_and_refusals():
    import rmr_amd
    g = _npz("int_tiny")
    cfg, Bq, K = g["cfg"], int(g["Bq"]), int(g["K"])
    w = O.make_interaction_weights(cfg, False, seed=0)
    conf = dict(cross_encoder_num_hidden_layers=cfg.ce_layers, cross_encoder_max_position_embeddings=cfg.ce_max_pos,
                loss_fn="BCE", pos_weight=None, interaction_type="NORMAL", arch=arch_from_cfg(cfg, False, "fp16"))
    args = _int_args(g)
    labels = [float(x) for x in g["labels"]]
    m = rmr_amd.InteractionRerankModel(conf, state_dict=w)
    m.engine.set_option("resid_split", 0)
    li = m.engine.li_scores(args[0], args[1], args[3], Bq, K)
    ref = m(args[0], args[1], K - 1, args[2], args[3], preflmr_scores=li["scores"], fusion_multiplier=MULT, labels=labels)
    got = m(args[0], args[1], K - 1, args[2], args[3], fusion_from_li=True, fusion_multiplier=MULT, labels=labels, want_maxsim=True)
    torch.cuda.synchronize()
    assert torch.equal(ref.logits, got.logits) and torch.equal(ref.loss, got.loss) and torch.equal(got.maxsim, li["maxsim"])
    mp = rmr_amd.InteractionRerankModel(dict(conf, packed_rows=True), state_dict=w)
    mp.engine.set_option("resid_split", 0)
    pk = mp(args[0], args[1], K - 1, args[2], args[3], fusion_from_li=True, fusion_multiplier=MULT, labels=labels)
    sizes = [K + 1, K - 1]
    pl = mp(args[0], args[1], K - 1, args[2], args[3], fusion_from_li=True, fusion_multiplier=MULT, candidates_per_query=sizes)
    pl_ref = mp(args[0], args[1], K - 1, args[2], args[3], fusion_multiplier=MULT, candidates_per_query=sizes,
                preflmr_scores=m.engine.li_scores(args[0].index_select(0, torch.tensor([0] * sizes[0] + [1] * sizes[1]).cuda()),
                                                  args[1], args[3], Bq * K, 1)["scores"])
    torch.cuda.synchronize()
    assert torch.equal(pk.logits, got.logits) and torch.equal(pl.logits, pl_ref.logits)
    for fn in (m.engine.forward_interaction, m.engine.forward_interaction_packed):
        with pytest.raises(ValueError):                    # both sources of scores
            fn(*args, Bq, K, None, preflmr_scores=li["scores"], fusion_from_li=True)
        with pytest.raises(ValueError):                    # the MaxSim comes with the from-li path
            fn(*args, Bq, K, None, want_maxsim=True)
    with pytest.raises(ValueError):
        m(args[0], args[1], K - 1, args[2], args[3], preflmr_scores=li["scores"], fusion_from_li=True)


def test_mores_refuses_fusion_from_li():
    eng, g, _ = _int_engine("mores_tiny", "fp16", mores=True)
    Bq, K = int(g["Bq"]), int(g["K"])
    args = _int_args(g)
    msgs = []
    for fn in (eng.forward_interaction, eng.forward_interaction_packed):
        with pytest.raises(NotImplementedError) as e:      # mores_model.py:72-73
            fn(*args, Bq, K, None, fusion_from_li=True)
        msgs.append(str(e.value).split(":")[-1])
    with pytest.raises(NotImplementedError) as e:
        fn(*args, Bq, K, None, preflmr_scores=torch.zeros(Bq * K, args[1].shape[1], args[0].shape[1]).cuda())
    assert msgs[0] == msgs[1] == str(e.value).split(":")[-1]     # the existing message
    plain = eng.forward_interaction(*args, Bq, K, None)           # the refusal left the handle usable
    torch.cuda.synchronize()
    assert torch.isfinite(plain["logits"]).all()
    assert "scores" in eng.li_scores(args[0], args[1], args[3], Bq, K)    # the operator itself works on any handle


def test_reserved_from_li_forward_is_capturable_into_a_graph():
    """rr_reserve(with_fusion = 2) covers the score block: an engine that has never run a forward captures the from-li forward
    right after it (a forward that had to grow a block under capture is refused) and the replay gives the eager bits.  The
    eager run, and the warm-up of the kernels on the capture stream, belong to a second engine with the same weights."""
    warm, g, _ = _int_engine("int_tiny", "fp16")
    eng, _, _ = _int_engine("int_tiny", "fp16")
    Bq, K = int(g["Bq"]), int(g["K"])
    args = _int_args(g)
    Lq, Lc = args[0].shape[1], args[1].shape[1]
    kw = dict(fusion_from_li=True, want_maxsim=True, want_order=True, fusion_multiplier=MULT)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        eager = warm.forward_interaction(*args, Bq, K, None, **kw)
        torch.cuda.synchronize()
        eng.reserve(Bq * K, Bq, Lq, Lc, with_fusion=2)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            out = eng.forward_interaction(*args, Bq, K, None, **kw)
        out["logits"].zero_()
        out["maxsim"].zero_()
        graph.replay()
        torch.cuda.synchronize()
    for k in ("logits", "order", "maxsim", "loss"):
        assert torch.equal(out[k], eager[k]), k


# ---- joint family ---------------------------------------------------------------------------------------------------------
def test_joint_retriever_embeddings_equal_explicit_scores():
    import rmr_amd
    g = _npz("rm_fuse_tiny")
    cfg = g["cfg"]
    cfg.loss_fn = "2H_BCE"
    eng = rmr_amd.RerankEngine(arch_from_cfg(cfg, True, "fp16"))
    eng.load_state_dict(O.make_weights(cfg, seed=0, vision=True))
    eng.set_option("resid_split", 0)
    t = lambda k: torch.from_numpy(g[k]).cuda()
    Bq, K, S, ql = int(g["Bq"]), int(g["K"]), int(g["S"]), int(g["ql"])
    N, P = Bq * K, cfg.prefix_len + cfg.n_patches
    ids = torch.cat([t("query_input_ids").repeat_interleave(K, 0), t("context_input_ids")[:, 2:2 - ql]], 1).long().contiguous()
    am = torch.cat([t("query_attention_mask").repeat_interleave(K, 0), t("context_attention_mask")[:, 2:2 - ql]], 1).long().contiguous()
    cls, pat, instr = t("image_cls"), t("image_patches"), int(g["instruction_token_id"])
    # the retriever's embeddings of the query (text + image tokens) and of the context rows, unit norm; its mask = the context's
    rq, rc, _ = retriever_inputs(Bq, K, ql + P, S, cfg.li_dim, seed=31)
    rq, rc, rcm = rq.cuda(), rc.cuda(), t("context_attention_mask").float()
    sc = eng.li_scores(rq, rc, rcm, Bq, K, want_maxsim=False)["scores"]
    assert tuple(sc.shape) == (N, S, ql + P)
    kw = dict(want_order=True, want_scores=True, fusion_multiplier=MULT)
    rkw = dict(retriever_query_li=rq, retriever_context_li=rc, retriever_context_mask=rcm)
    ref = eng.forward_joint(ids, am, Bq, K, ql, cls, pat, instr, preflmr_scores=sc, **kw)
    got = eng.forward_joint(ids, am, Bq, K, ql, cls, pat, instr, **rkw, **kw)
    plain = eng.forward_joint(ids, am, Bq, K, ql, cls, pat, instr)
    pk_ref = eng.forward_joint_packed(ids, am, Bq, K, ql, cls, pat, instr, preflmr_scores=sc, granule=8, **kw)
    pk = eng.forward_joint_packed(ids, am, Bq, K, ql, cls, pat, instr, granule=8, **rkw, **kw)
    sl = eng.forward_joint(ids, am, Bq, K, ql, cls, pat, instr, pair_range=(1, N - 1), fusion_multiplier=MULT, **rkw)
    sl_ref = eng.forward_joint(ids, am, Bq, K, ql, cls, pat, instr, pair_range=(1, N - 1), fusion_multiplier=MULT, preflmr_scores=sc)
    torch.cuda.synchronize()
    _same(ref, got)
    _same(pk_ref, pk)
    assert pk["packed_segments"] >= 2
    assert torch.equal(sl["logits"][1:N - 1], sl_ref["logits"][1:N - 1])
    assert not torch.equal(plain["logits"], got["logits"])
    sizes = [K + 1, K - 1]
    per_pair = torch.repeat_interleave(torch.arange(2), torch.tensor(sizes)).cuda()
    sc_l = eng.li_scores(rq.index_select(0, per_pair), rc, rcm, N, 1, want_maxsim=False)["scores"]
    ls_ref = eng.forward_joint_packed(ids, am, None, None, ql, cls, pat, instr, preflmr_scores=sc_l, granule=8, list_sizes=sizes, **kw)
    ls = eng.forward_joint_packed(ids, am, None, None, ql, cls, pat, instr, granule=8, list_sizes=sizes, **rkw, **kw)
    torch.cuda.synchronize()
    _same(ls_ref, ls)
    with pytest.raises(ValueError):
        eng.forward_joint(ids, am, Bq, K, ql, cls, pat, instr, preflmr_scores=sc, **rkw)
    with pytest.raises(ValueError):
        eng.forward_joint_packed(ids, am, Bq, K, ql, cls, pat, instr, preflmr_scores=sc, **rkw)
    with pytest.raises(ValueError):                        # the three tensors go together
        eng.forward_joint(ids, am, Bq, K, ql, cls, pat, instr, retriever_query_li=rq)
    # the drop-in class passes the keywords through
    conf = dict(arch=arch_from_cfg(cfg, True, "fp16"), loss_fn="2H_BCE", pos_weight=cfg.pos_weight,
                cross_encoder_num_hidden_layers=cfg.ce_layers, cross_encoder_max_position_embeddings=cfg.ce_max_pos,
                instruction_token_id=instr)
    m = rmr_amd.RerankModel(conf, state_dict=O.make_weights(cfg, seed=0, vision=True))
    m.engine.set_option("resid_split", 0)
    cargs = (t("query_input_ids"), t("query_attention_mask"), None, t("context_input_ids"), t("context_attention_mask"), K - 1)
    d_ref = m(*cargs, preflmr_scores=sc, fusion_multiplier=MULT, image_features=(cls, pat))
    d_got = m(*cargs, fusion_multiplier=MULT, image_features=(cls, pat), **rkw)
    torch.cuda.synchronize()
    assert torch.equal(d_ref.logits, d_got.logits) and torch.equal(d_got.logits.view(-1), got["logits"])
    with pytest.raises(ValueError):
        m(*cargs, preflmr_scores=sc, image_features=(cls, pat), **rkw)
