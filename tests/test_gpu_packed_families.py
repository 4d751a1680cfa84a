"""GPU: packed variable-length forwards of the joint (RerankModel) and interaction (NORMAL, MORES) rerankers —
rr_forward_joint_packed / rr_forward_interaction_packed through RerankEngine.forward_joint_packed /
forward_interaction_packed and the drop-in classes' `packed_rows` key — against the padded calls of the same handle.

Equality (include/rerank_mi355.h): bit for bit with "resid_split" = 0 (the row-count rule of the residual stream cannot
interfere); with the default options within the fp16 parity gate (1e-3) and the same order."""
import ast
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, O, arch_from_cfg

pytestmark = pytest.mark.gpu

GATE = 1e-3          # fp16 parity gate


def _npz(name):
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def _cfg(g, loss_fn):
    cfg = O.OracleConfig(**ast.literal_eval(str(g["cfg_json"])))
    cfg.loss_fn = loss_fn
    return cfg


# ---- joint (RerankModel) ---------------------------------------------------------------------------------------------
def _joint_engine(cfg, dtype="fp16", exact=True):
    import rmr_amd
    eng = rmr_amd.RerankEngine(arch_from_cfg(cfg, True, dtype))
    eng.load_state_dict(O.make_weights(cfg, seed=0, vision=True))
    if exact:
        eng.set_option("resid_split", 0)
    return eng


def _joint_inputs(g):
    """The joint sequence exactly as RerankModel.forward assembles it (rerank_model.py:191-224)."""
    t = lambda k: torch.from_numpy(g[k]).cuda()
    K, ql = int(g["K"]), g["query_input_ids"].shape[1]
    q_ids = t("query_input_ids").repeat_interleave(K, 0)
    q_am = t("query_attention_mask").repeat_interleave(K, 0)
    ids = torch.cat([q_ids, t("context_input_ids")[:, 2:2 - ql]], 1).long().contiguous()
    am = torch.cat([q_am, t("context_attention_mask")[:, 2:2 - ql]], 1).long().contiguous()
    return ids, am, ql


def _check(pad, pk, exact, what):
    d = (pad["logits"] - pk["logits"]).abs().max().item()
    d2 = (pad["logits2"] - pk["logits2"]).abs().max().item()
    print(f"[{what}] packed vs padded: |dlogit| {d:.3e} / second head {d2:.3e}; rows {pk['packed_rows']} in "
          f"{pk['packed_segments']} segments")
    if exact:
        assert torch.equal(pad["logits"], pk["logits"]), f"{what}: packed logits not bit-identical ({d:.3e})"
        if pad.get("loss") is not None:
            assert pad["loss"].item() == pk["loss"].item()
    else:
        assert d <= GATE
        if pad.get("loss") is not None:
            assert abs(pad["loss"].item() - pk["loss"].item()) <= GATE
    if pad.get("order") is not None:
        if exact or d == 0.0:
            assert torch.equal(pad["order"], pk["order"])
        else:       # the same order wherever the padded logits are further apart than the two calls' difference
            K = pad["order"].shape[1]
            lp = pad["logits"].view(-1, K)
            ranked = torch.gather(lp, 1, pk["order"].long())
            assert (ranked[:, 1:] <= ranked[:, :-1] + 2 * d).all()


@pytest.mark.parametrize("name", ["rm_tiny", "rm_fuse_tiny"])
@pytest.mark.parametrize("granule", [8, 16])
def test_joint_packed_equals_padded_tiny(name, granule):
    g = _npz(name)
    cfg = _cfg(g, "2H_BCE")
    eng = _joint_engine(cfg)
    ids, am, ql = _joint_inputs(g)
    Bq, K = int(g["Bq"]), int(g["K"])
    cls, pat = torch.from_numpy(g["image_cls"]).cuda(), torch.from_numpy(g["image_patches"]).cuda()
    kw = dict(want_order=True, want_scores=True)
    if int(g["fusion"]):
        kw.update(preflmr_scores=torch.from_numpy(g["preflmr_scores"]).cuda(), fusion_multiplier=float(g["fusion_multiplier"]))
    instr = int(g["instruction_token_id"])
    pad = eng.forward_joint(ids, am, Bq, K, ql, cls, pat, instr, **kw)
    pk = eng.forward_joint_packed(ids, am, Bq, K, ql, cls, pat, instr, granule=granule, **kw)
    torch.cuda.synchronize()
    assert pk["packed_segments"] >= 2 and pk["packed_rows"] < Bq * K * ids.shape[1]
    _check(pad, pk, True, f"{name}/granule {granule}")
    assert torch.equal(pad["logits2"], pk["logits2"]) and torch.equal(pad["scores"], pk["scores"])


def _joint_base_batch(Bq, K, S, ql, vocab, seed):
    """c3-shaped joint sequences: [CLS] query [SEP] padded to ql, then a context part of U[64, S] - ql tokens."""
    gen = torch.Generator().manual_seed(seed)
    N = Bq * K
    ids = torch.zeros(N, S, dtype=torch.int64)
    for qi in range(Bq):
        qlen = int(torch.randint(8, ql - 1, (1,), generator=gen))
        q = torch.cat([torch.tensor([101]), torch.randint(1000, vocab, (qlen,), generator=gen), torch.tensor([102])])
        for j in range(K):
            ids[qi * K + j, :q.numel()] = q
    total = torch.randint(64, S + 1, (N,), generator=gen)
    for p in range(N):
        nc = int(total[p]) - ql
        ids[p, ql:ql + nc] = torch.randint(1000, vocab, (nc,), generator=gen)
        ids[p, ql + nc - 1] = 102
    am = (ids != 0).long()
    return ids, am


@pytest.mark.parametrize("fusion", [False, True])
def test_joint_packed_equals_padded_c3_geometry(fusion):
    """c3 geometry (bert-base text encoder, 81 vision tokens, one cross-encoder layer), 200 pairs of joint length U[64, 512].
    Not bit for bit (include/rerank_mi355.h): image features are per pair in a packed call, so the mapping network's first
    layer runs GEMMs of another row count than the padded call's per-query ones; within the parity gate, same order."""
    import rmr_amd
    arch = rmr_amd.make_arch(dict(cross_encoder_num_hidden_layers=1, cross_encoder_max_position_embeddings=750, loss_fn="2H_BCE",
                                  pos_weight=None, compute_dtype="fp16"))
    eng = rmr_amd.RerankEngine(arch)
    eng.load_state_dict(rmr_amd.synthetic_state_dict(arch, seed=0))
    eng.set_option("resid_split", 0)
    Bq, K, S, ql = 2, 100, 512, 32
    ids, am = _joint_base_batch(Bq, K, S, ql, arch["vocab_size"], seed=7)
    ids, am = ids.cuda(), am.cuda()
    from rmr_amd.synthetic import image_features
    cls, pat = [t.cuda() for t in image_features(Bq, arch["n_patches"], arch["vision_hidden"])]
    kw = dict(want_order=True)
    if fusion:
        P = arch["prefix_len"] + arch["n_patches"]
        gen = torch.Generator().manual_seed(3)
        kw.update(preflmr_scores=torch.randn(Bq * K, S, ql + P, generator=gen).cuda(), fusion_multiplier=5.0)
    pad = eng.forward_joint(ids, am, Bq, K, ql, cls, pat, None, **kw)
    pk = eng.forward_joint_packed(ids, am, Bq, K, ql, cls, pat, None, granule=64, **kw)
    torch.cuda.synchronize()
    assert pk["packed_segments"] >= 4 and pk["packed_rows"] < 0.7 * Bq * K * S
    _check(pad, pk, False, f"joint c3 geometry fusion={fusion}")


# ---- interaction (NORMAL, MORES) ----------------------------------------------------------------------------------------
def _int_engine(name, dtype="fp16", exact=True):
    import rmr_amd
    g = _npz(name)
    cfg = _cfg(g, str(g["loss_fn"]))
    mores = bool(g["mores"])
    arch = arch_from_cfg(cfg, False, dtype)
    arch["model_kind"] = "mores" if mores else "interaction"
    eng = rmr_amd.RerankEngine(arch)
    eng.load_state_dict(O.make_interaction_weights(cfg, mores, seed=0))
    if exact:
        eng.set_option("resid_split", 0)
    return eng, g


def _int_args(g):
    return [torch.from_numpy(g[k]).cuda() for k in ("query_li", "context_li", "query_mask", "context_mask")]


def _labels(g):
    return torch.from_numpy(g["labels"]).cuda() if g["labels"].size else None


def _scores(g, seed=5):
    if "preflmr_scores" in g and g["preflmr_scores"].size:
        return torch.from_numpy(g["preflmr_scores"]).cuda(), float(g["fusion_multiplier"])
    gen = torch.Generator().manual_seed(seed)
    N, Lc, Lq = g["context_li"].shape[0], g["context_li"].shape[1], g["query_li"].shape[1]
    return torch.randn(N, Lc, Lq, generator=gen).cuda(), 5.0


@pytest.mark.parametrize("name", ["int_tiny", "int_fuse_tiny", "int_base"])
@pytest.mark.parametrize("fusion", [False, True])
def test_interaction_normal_packed_equals_padded(name, fusion):
    eng, g = _int_engine(name)
    Bq, K = int(g["Bq"]), int(g["K"])
    args = _int_args(g)
    kw = dict(want_order=True, want_scores=True)
    if fusion:
        ps, mult = _scores(g)
        kw.update(preflmr_scores=ps, fusion_multiplier=mult)
    pad = eng.forward_interaction(*args, Bq, K, _labels(g), **kw)
    pk = eng.forward_interaction_packed(*args, Bq, K, _labels(g), granule=16, **kw)
    torch.cuda.synchronize()
    assert pk["packed_segments"] >= 2 and pk["packed_rows"] < Bq * K * args[1].shape[1]
    _check(pad, pk, True, f"{name} fusion={fusion}")
    # the host-known lengths give the same call
    lens = ((args[3] != 0) * torch.arange(1, args[3].shape[1] + 1, device="cuda")).amax(1).cpu().tolist()
    host = eng.forward_interaction_packed(*args, Bq, K, _labels(g), granule=16, lengths=lens, **kw)
    torch.cuda.synchronize()
    assert torch.equal(host["logits"], pk["logits"])


@pytest.mark.parametrize("name", ["mores_tiny", "mores_base"])
def test_mores_packed_equals_padded_and_refuses_fusion(name):
    eng, g = _int_engine(name)
    Bq, K = int(g["Bq"]), int(g["K"])
    args = _int_args(g)
    pad = eng.forward_interaction(*args, Bq, K, _labels(g), want_order=True)
    pk = eng.forward_interaction_packed(*args, Bq, K, _labels(g), granule=16, want_order=True)
    torch.cuda.synchronize()
    assert pk["packed_segments"] >= 2
    _check(pad, pk, True, name)
    assert torch.equal(pad["loss"], pk["loss"])
    ps, mult = _scores(g)
    statuses = []
    for fn in (eng.forward_interaction, eng.forward_interaction_packed):
        with pytest.raises(NotImplementedError) as e:                        # mores_model.py:72-73
            fn(*args, Bq, K, None, preflmr_scores=ps, fusion_multiplier=mult)
        statuses.append(str(e.value).split(":")[1])
    assert statuses[0] == statuses[1]


@pytest.mark.parametrize("kind", ["normal", "normal_fusion", "mores"])
def test_interaction_packed_equals_padded_at_200_pairs(kind):
    """int_base geometry (Lq 113, Lc 512), 2 queries x 100 candidates of context length U[64, 512]: the padded call's attention
    grid selects the fixed-reference schedule here, the packed call must follow it."""
    import rmr_amd
    g = _npz("mores_base" if kind == "mores" else "int_base")
    cfg = _cfg(g, "BCE")
    arch = arch_from_cfg(cfg, False, "fp16")
    arch["model_kind"] = "mores" if kind == "mores" else "interaction"
    eng = rmr_amd.RerankEngine(arch)
    eng.load_state_dict(O.make_interaction_weights(cfg, kind == "mores", seed=0))
    eng.set_option("resid_split", 0)
    Bq, K, Lq, Lc, D = 2, 100, 113, 512, cfg.li_dim
    gen = torch.Generator().manual_seed(11)
    q, c = torch.randn(Bq, Lq, D, generator=gen).cuda(), torch.randn(Bq * K, Lc, D, generator=gen).cuda()
    qm = torch.ones(Bq, Lq)
    qm[:, 90:] = 0
    clen = torch.randint(64, Lc + 1, (Bq * K,), generator=gen)
    cm = (torch.arange(Lc)[None, :] < clen[:, None]).float().cuda()
    kw = dict(want_order=True)
    if kind == "normal_fusion":
        kw.update(preflmr_scores=torch.randn(Bq * K, Lc, Lq, generator=gen).cuda(), fusion_multiplier=5.0)
    pad = eng.forward_interaction(q, c, qm.cuda(), cm, Bq, K, **kw)
    pk = eng.forward_interaction_packed(q, c, qm.cuda(), cm, Bq, K, granule=32, lengths=clen.tolist(), **kw)
    torch.cuda.synchronize()
    assert pk["packed_segments"] >= 8 and pk["packed_rows"] < 0.7 * Bq * K * Lc
    _check(pad, pk, True, f"interaction 200 pairs {kind}")


# ---- the fusion normaliser trap ---------------------------------------------------------------------------------------
def test_fusion_normalisers_run_over_the_padded_context_axis():
    """Clearly non-zero scores on the PAD positions of the context axis: the padded call's softmax over the context tokens
    gives them most of the mass.  A builder that normalised over the segment's length instead computes what the padded call
    computes with those scores at -1e4 (exp underflows to exactly 0): measured 1.2e-2 (interaction) / 7.3e-3 (joint) from the
    padded call, against a gate of 1e-3.  Packed must equal padded bit for bit."""
    eng, g = _int_engine("int_fuse_tiny")
    Bq, K = int(g["Bq"]), int(g["K"])
    args = _int_args(g)
    ps, mult = _scores(g)                  # the fixture's multiplier, 20
    Lc = args[1].shape[1]
    lens = ((args[3] != 0) * torch.arange(1, Lc + 1, device="cuda")).amax(1)
    pad_pos = torch.arange(Lc, device="cuda")[None, :] >= lens[:, None]          # [N, Lc]
    trap = torch.where(pad_pos[:, :, None], ps + 10.0, ps)
    wrong = torch.where(pad_pos[:, :, None], torch.full_like(ps, -1e4), ps)
    pad = eng.forward_interaction(*args, Bq, K, None, preflmr_scores=trap, fusion_multiplier=mult, want_order=True)
    seg = eng.forward_interaction(*args, Bq, K, None, preflmr_scores=wrong, fusion_multiplier=mult)
    pk = eng.forward_interaction_packed(*args, Bq, K, None, preflmr_scores=trap, fusion_multiplier=mult, granule=1,
                                        want_order=True)
    torch.cuda.synchronize()
    miss = (seg["logits"] - pad["logits"]).abs().max().item()
    print(f"segment-normalised bias misses the padded call by {miss:.3e}")
    assert miss > 5 * GATE
    _check(pad, pk, True, "int_fuse_tiny trap")

    # the joint family: context rows 2 + kc of the scores, kc >= the pair's context length are pad positions
    gj = _npz("rm_fuse_tiny")
    ej = _joint_engine(_cfg(gj, "2H_BCE"))
    ids, am, ql = _joint_inputs(gj)
    S = ids.shape[1]
    Bq, K = int(gj["Bq"]), int(gj["K"])
    cls, pat = torch.from_numpy(gj["image_cls"]).cuda(), torch.from_numpy(gj["image_patches"]).cuda()
    psj, multj = torch.from_numpy(gj["preflmr_scores"]).cuda(), float(gj["fusion_multiplier"])
    jl = ((am != 0) * torch.arange(1, S + 1, device="cuda")).amax(1)
    row = torch.arange(S, device="cuda")[None, :]
    padj = (row >= 2 + (jl - ql)[:, None]) & (row < 2 + S - ql)                 # score rows of pad context tokens
    trapj = torch.where(padj[:, :, None], psj + 10.0, psj)
    wrongj = torch.where(padj[:, :, None], torch.full_like(psj, -1e4), psj)
    instr = int(gj["instruction_token_id"])
    padr = ej.forward_joint(ids, am, Bq, K, ql, cls, pat, instr, preflmr_scores=trapj, fusion_multiplier=multj, want_order=True)
    segr = ej.forward_joint(ids, am, Bq, K, ql, cls, pat, instr, preflmr_scores=wrongj, fusion_multiplier=multj)
    pkr = ej.forward_joint_packed(ids, am, Bq, K, ql, cls, pat, instr, preflmr_scores=trapj, fusion_multiplier=multj, granule=1,
                                  want_order=True)
    torch.cuda.synchronize()
    missj = (segr["logits"] - padr["logits"]).abs().max().item()
    print(f"joint: segment-normalised bias misses the padded call by {missj:.3e}")
    assert missj > 5 * GATE
    _check(padr, pkr, True, "rm_fuse_tiny trap")


# ---- goldens -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["int_tiny", "int_fuse_tiny", "int_base", "mores_tiny", "mores_base"])
def test_packed_interaction_on_the_goldens(name):
    """Default options (fp16): the packed call against the fp32 stock-HF golden, within the gates test_gpu_interaction.py uses."""
    eng, g = _int_engine(name, exact=False)
    Bq, K = int(g["Bq"]), int(g["K"])
    args = _int_args(g)
    kw = {}
    fused = "preflmr_scores" in g and g["preflmr_scores"].size > 0
    if fused:
        kw = dict(preflmr_scores=torch.from_numpy(g["preflmr_scores"]).cuda(), fusion_multiplier=float(g["fusion_multiplier"]))
    r = eng.forward_interaction_packed(*args, Bq, K, _labels(g), want_order=True, **kw)
    torch.cuda.synchronize()
    d = (r["logits"].cpu() - torch.from_numpy(g["logits"]).reshape(-1)).abs().max().item()
    print(f"[{name}] packed |dlogit| vs fp32 golden {d:.2e}")
    assert d <= (3e-4 if fused else 1e-3)
    assert abs(r["loss"].item() - float(g["loss"])) < (2e-3 if fused else 1e-2)
    assert r["order"].cpu().tolist() == [O.rank_descending_stable(x) for x in r["logits"].cpu().view(Bq, K).tolist()]


@pytest.mark.parametrize("name", ["rm_tiny", "rm_fuse_tiny"])
def test_packed_joint_on_the_goldens(name):
    g = _npz(name)
    eng = _joint_engine(_cfg(g, "2H_BCE"), exact=False)
    ids, am, ql = _joint_inputs(g)
    Bq, K = int(g["Bq"]), int(g["K"])
    kw = {}
    fused = bool(int(g["fusion"]))
    if fused:
        kw = dict(preflmr_scores=torch.from_numpy(g["preflmr_scores"]).cuda(), fusion_multiplier=float(g["fusion_multiplier"]))
    r = eng.forward_joint_packed(ids, am, Bq, K, ql, torch.from_numpy(g["image_cls"]).cuda(),
                                 torch.from_numpy(g["image_patches"]).cuda(), int(g["instruction_token_id"]), **kw)
    torch.cuda.synchronize()
    d = (r["logits"].cpu() - torch.from_numpy(g["logits"]).reshape(-1)).abs().max().item()
    print(f"[{name}] packed |dlogit| vs fp32 golden {d:.2e}, loss {r['loss'].item():.6f} vs {float(g['loss']):.6f}")
    assert d < (2.5e-4 if fused else 1e-3)
    assert abs(r["loss"].item() - float(g["loss"])) < 2e-3


# ---- shape errors ------------------------------------------------------------------------------------------------------
def test_packed_calls_refuse_bad_segment_tables():
    import ctypes as C
    from rmr_amd import _lib as L
    g = _npz("rm_tiny")
    ej = _joint_engine(_cfg(g, "2H_BCE"), exact=False)
    buf = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()
    st = torch.cuda.current_stream().cuda_stream

    def joint(ns, ls, S=64, ql=8):
        return ej.lib.rr_forward_joint_packed(ej.h, p, p, p, p, None, 1.0, len(ns), (C.c_int32 * len(ns))(*ns),
                                              (C.c_int32 * len(ls))(*ls), S, ql, -1, p, p, st)
    assert joint([1] * 65, [40] * 65) == L.RR_ERR_BAD_SHAPE                   # more than 64 segments
    assert joint([2], [65]) == L.RR_ERR_BAD_SHAPE                             # above the padded length
    assert joint([2], [8]) == L.RR_ERR_BAD_SHAPE                              # not longer than the query part
    assert joint([2, 1], [40, 0]) == L.RR_ERR_BAD_SHAPE                       # an empty segment
    assert joint([0, 1], [40, 48]) == L.RR_ERR_BAD_SHAPE

    ei, gi = _int_engine("int_tiny", exact=False)

    def inter(ns, ls, Lc=40, Lq=9):
        return ei.lib.rr_forward_interaction_packed(ei.h, p, p, p, p, None, 1.0, len(ns), (C.c_int32 * len(ns))(*ns),
                                                    (C.c_int32 * len(ls))(*ls), Lc, Lq, p, p, st)
    assert inter([1] * 65, [16] * 65) == L.RR_ERR_BAD_SHAPE
    assert inter([2], [41]) == L.RR_ERR_BAD_SHAPE
    assert inter([2], [0]) == L.RR_ERR_BAD_SHAPE
    ce_max = int(ei.arch["ce_max_pos"])
    assert inter([2], [16], Lc=ce_max - 9 + 1) == L.RR_ERR_BAD_SHAPE        # Lq + padded_context_len > ce_max_pos
    assert ei.lib.rr_forward_interaction_packed(ei.h, p, p, p, p, None, 1.0, 1, None, None, 40, 9, p, p, st) == L.RR_ERR_BAD_ARG
    torch.cuda.synchronize()


# ---- drop-in classes ---------------------------------------------------------------------------------------------------
def test_drop_in_classes_with_packed_rows_agree_with_the_default_classes():
    import rmr_amd
    # RerankModel
    g = _npz("rm_tiny")
    cfg = _cfg(g, "2H_BCE")
    w = O.make_weights(cfg, seed=0, vision=True)
    conf = dict(cross_encoder_num_hidden_layers=cfg.ce_layers, cross_encoder_max_position_embeddings=cfg.ce_max_pos,
                loss_fn="2H_BCE", pos_weight=cfg.pos_weight, instruction_token_id=int(g["instruction_token_id"]),
                arch=arch_from_cfg(cfg, True, "fp16"))
    t = lambda k: torch.from_numpy(g[k]).cuda()
    args = (t("query_input_ids"), t("query_attention_mask"), None, t("context_input_ids"), t("context_attention_mask"),
            int(g["K"]) - 1)
    outs = [rmr_amd.RerankModel(dict(conf, packed_rows=p), state_dict=w)(*args, image_features=(t("image_cls"), t("image_patches")),
                                                                         want_order=True) for p in (False, True)]
    torch.cuda.synchronize()
    assert (outs[0].logits - outs[1].logits).abs().max().item() <= GATE
    assert abs(outs[0].loss.item() - outs[1].loss.item()) <= GATE and torch.equal(outs[0].order, outs[1].order)

    # InteractionRerankModel, NORMAL and MORES
    for name, kind in (("int_tiny", "NORMAL"), ("mores_tiny", "MORES")):
        gi = _npz(name)
        ci = _cfg(gi, str(gi["loss_fn"]))
        wi = O.make_interaction_weights(ci, kind == "MORES", seed=0)
        confi = dict(cross_encoder_num_hidden_layers=ci.ce_layers, cross_encoder_max_position_embeddings=ci.ce_max_pos,
                     loss_fn=ci.loss_fn, interaction_type=kind, arch=arch_from_cfg(ci, False, "fp16"))
        a = [torch.from_numpy(gi[k]).cuda() for k in ("query_li", "context_li")]
        m = [torch.from_numpy(gi[k]).cuda() for k in ("query_mask", "context_mask")]
        lab = [float(x) for x in gi["labels"]] if gi["labels"].size else None
        oi = [rmr_amd.InteractionRerankModel(dict(confi, packed_rows=p), state_dict=wi)(a[0], a[1], int(gi["K"]) - 1, m[0], m[1],
                                                                                         labels=lab, want_order=True)
              for p in (False, True)]
        torch.cuda.synchronize()
        assert (oi[0].logits - oi[1].logits).abs().max().item() <= GATE, name
        assert abs(oi[0].loss.item() - oi[1].loss.item()) <= GATE and torch.equal(oi[0].order, oi[1].order)

    # FullContextRerankModel.forward_ids
    from helpers import golden_inputs, load_golden
    gf = load_golden("tiny")
    ids, am, tt, (cls, pat) = golden_inputs(gf)
    cf = gf["cfg"]
    wf = O.make_weights(cf, seed=0, vision=gf["vision"])
    conff = dict(cross_encoder_num_hidden_layers=cf.ce_layers, cross_encoder_max_position_embeddings=cf.ce_max_pos,
                 loss_fn=cf.loss_fn, pos_weight=cf.pos_weight, arch=arch_from_cfg(cf, gf["vision"], "fp16"))
    img = (cls.cuda(), pat.cuda()) if cls is not None else (None, None)
    of = [rmr_amd.FullContextRerankModel(dict(conff, packed_rows=p), state_dict=wf).forward_ids(
        ids.cuda(), am.cuda(), tt.cuda(), gf["K"] - 1, *img, labels=gf["labels_list"], want_order=True) for p in (False, True)]
    torch.cuda.synchronize()
    assert (of[0].logits - of[1].logits).abs().max().item() <= GATE
    assert abs(of[0].loss.item() - of[1].loss.item()) <= GATE and torch.equal(of[0].order, of[1].order)
