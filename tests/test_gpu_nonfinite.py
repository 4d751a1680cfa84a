"""GPU: a NaN in a weight that reaches the reference's logits is never ranked silently.

include/rerank_mi355.h promises that a forward raises the range flag when a row is not finite ("inf / NaN in the inputs or the
weights").  For each floating-point tensor of the state dict, one at a time, one element is set to NaN (element 0, and one element
at an index seeded by the tensor's name), a fresh engine is built (the sticky flag belongs to the handle) and runs one forward.
  * Condition, decided by the reference alone: the fp32 oracle on the same poisoned weights; the pairs whose oracle logit is not
    finite form P.  An empty P means the element is not an input of this forward: such (tensor, element) cases are skipped, and
    the skipped ones must equal the literal list NOT_INPUTS below, so the test cannot skip its way to green.
  * Assertion: the device logits are non-finite on every pair of P, or eng.activation_range_exceeded() is true after the
    forward.  Finite logits on a pair of P with the flag clear is the failure.
NaN is ordinary data to every kernel: nothing here faults, and nothing loops on a failing step.
On the commit before this test, erf-GELU returned -3e-8 for a NaN (min and med3 drop it) and the host packers of the 8-bit weights
turned a NaN into the most negative code under a finite scale: every FFN-up weight and bias (text encoder, cross-encoder, mapping
network) and, in the 8-bit configurations, every Q / K / V weight was ranked with finite logits and a clear flag
(profiles/nonfinite_parent_build.log).  With gelu_erf_fast / gelu_erf_fast2 NaN-transparent and a NaN scale for such a weight row,
no tensor of any sweep is silent.  The whole file takes about 80 s on an MI355X.
The host weight packers of the 8-bit configurations (CPU-only) are covered by tests/test_int8_cpu.py and tests/test_abi_cpu.py."""
import ast
import os
import zlib

import numpy as np
import pytest
import torch

from helpers import GOLDEN, arch_from_cfg, golden_inputs, load_golden
import oracle.rerank_oracle as O

pytestmark = pytest.mark.gpu

_CASES = {}


def _npz(name):
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def case(name):
    """One forward of one model family: its weights `w`, the tensors `keys` to poison, `oracle(w)` -> the fp32 reference outputs
    [n, ...] and `device(w, dt, packed, q8_format)` -> (outputs [n, ...], range flag).  `tiny_mm` (vision tokens), `tiny_2h` (two
    heads): forward_ids on the goldens' batch; `q8_small`: the 3-layer 256-wide text model of
    test_fp8_forward_small_model_against_the_oracle_emulation, for the 8-bit configurations; `rm_tiny`: forward_joint; `int_tiny`:
    forward_interaction; `vit_tiny`: encode_image (outputs per image: CLS row and patch rows together)."""
    if name in _CASES:
        return _CASES[name]
    import rmr_amd
    c = dict(name=name, P={})
    cuda = lambda t: None if t is None else t.cuda()

    def engine(arch, w, q8_format=None):
        if q8_format is not None:
            arch["fp8"] = 1
        eng = rmr_amd.RerankEngine(arch)
        if q8_format is not None:
            eng.set_option("fp8_first_layer", 0)             # the whole stack on the 8-bit GEMMs
            eng.set_option("q8_format", q8_format)
        eng.load_state_dict(w)
        return eng

    def finish(eng, out):
        torch.cuda.synchronize()
        return out.float().cpu(), eng.activation_range_exceeded()

    if name in ("tiny_mm", "tiny_2h", "q8_small"):
        if name == "q8_small":
            cfg = O.OracleConfig(vocab_size=2000, hidden=256, layers=3, heads=4, intermediate=1024, max_pos=64, ce_hidden=256,
                                 ce_heads=4, ce_intermediate=1024, ce_layers=2, ce_max_pos=128, li_dim=64)
            cfg.loss_fn = "BCE"
            vision, Bq, K, S, img = False, 2, 6, 64, (None, None)
            ids, am, tt = O.make_pair_batch(cfg, Bq, K, S, seed=4)
            c["w"] = O.make_weights(cfg, seed=2, vision=False)
        else:
            g = load_golden(name)
            cfg, vision, Bq, K, S = g["cfg"], g["vision"], g["Bq"], g["K"], g["S"]
            ids, am, tt, img = golden_inputs(g)
            c["w"] = O.make_weights(cfg, seed=0, vision=vision)
        c["oracle"] = lambda w: O.full_context_forward(cfg, w, ids, am, tt, Bq, K, img[0], img[1]).logits.reshape(-1)

        def device(w, dt, packed=False, q8_format=None):
            eng = engine(arch_from_cfg(cfg, vision, dt), w, q8_format)
            args = (ids.cuda(), am.cuda(), tt.cuda(), Bq, K, cuda(img[0]), cuda(img[1]))
            r = eng.forward_ids_packed(*args, None, granule=S // 4) if packed else eng.forward_ids(*args)
            return finish(eng, r["logits"].reshape(-1))
    elif name == "rm_tiny":
        g = _npz(name)
        cfg = O.OracleConfig(**ast.literal_eval(str(g["cfg_json"])))
        cfg.loss_fn = "2H_BCE"
        t = lambda k: torch.from_numpy(g[k])
        Bq, K, ql, instr = int(g["Bq"]), int(g["K"]), g["query_input_ids"].shape[1], int(g["instruction_token_id"])
        j_ids = torch.cat([t("query_input_ids").repeat_interleave(K, 0), t("context_input_ids")[:, 2:2 - ql]], 1).long().contiguous()
        j_am = torch.cat([t("query_attention_mask").repeat_interleave(K, 0), t("context_attention_mask")[:, 2:2 - ql]], 1).long().contiguous()
        c["w"] = O.make_weights(cfg, seed=0, vision=True)
        c["oracle"] = lambda w: O.rerank_model_forward(cfg, w, t("query_input_ids"), t("query_attention_mask"), t("context_input_ids"),
                                                       t("context_attention_mask"), K, t("image_cls"), t("image_patches"),
                                                       instr).logits.reshape(-1)

        def device(w, dt, packed=False, q8_format=None):
            eng = engine(arch_from_cfg(cfg, True, dt), w)
            args = (j_ids.cuda(), j_am.cuda(), Bq, K, ql, t("image_cls").cuda(), t("image_patches").cuda(), instr)
            r = eng.forward_joint_packed(*args, granule=16) if packed else eng.forward_joint(*args)
            return finish(eng, r["logits"].reshape(-1))
    elif name == "int_tiny":
        g = _npz(name)
        cfg = O.OracleConfig(**ast.literal_eval(str(g["cfg_json"])))
        cfg.loss_fn = str(g["loss_fn"])
        t = lambda k: torch.from_numpy(g[k])
        Bq, K, mores = int(g["Bq"]), int(g["K"]), bool(g["mores"])
        c["w"] = O.make_interaction_weights(cfg, mores, seed=0)
        c["oracle"] = lambda w: O.interaction_forward(cfg, w, t("query_li"), t("context_li"), t("query_mask"), t("context_mask"), K,
                                                      None, mores).logits.reshape(-1)

        def device(w, dt, packed=False, q8_format=None):
            arch = arch_from_cfg(cfg, False, dt)
            arch["model_kind"] = "mores" if mores else "interaction"
            eng = engine(arch, w)
            args = (t("query_li").cuda(), t("context_li").cuda(), t("query_mask").cuda(), t("context_mask").cuda(), Bq, K)
            r = eng.forward_interaction_packed(*args, granule=16) if packed else eng.forward_interaction(*args)
            return finish(eng, r["logits"].reshape(-1))
    elif name == "vit_tiny":
        g = _npz(name)
        kw = dict(vocab_size=2000, hidden=128, layers=1, heads=2, intermediate=256, max_pos=64, ce_hidden=128, ce_heads=2,
                  ce_intermediate=256, ce_layers=1, ce_max_pos=160, li_dim=64, prefix_len=4, cross_attn_len=32)   # tests/test_gpu_vision.py
        kw.update(ast.literal_eval(str(g["cfg_json"])))
        cfg, B = O.OracleConfig(**kw), int(g["B"])
        px = O.make_pixel_values(cfg, B, seed=int(g["pixel_seed"]))
        vit = O.make_vit_weights(cfg, seed=int(g["weight_seed"]))
        c["w"] = dict(O.make_weights(cfg, seed=0, vision=True))
        c["w"].update(vit)
        c["keys"] = [k for k, v in vit.items() if v.is_floating_point()]       # the tensors of THIS forward
        c["oracle"] = lambda w: torch.cat([x.reshape(B, -1) for x in O.clip_vision_forward(cfg, w, px)], 1)

        def device(w, dt, packed=False, q8_format=None):
            arch = arch_from_cfg(cfg, True, dt)
            arch.update(vit_layers=cfg.vit_layers, vit_heads=cfg.vit_heads, vit_intermediate=cfg.vit_intermediate,
                        vit_image_size=cfg.vit_image_size, vit_patch_size=cfg.vit_patch_size)
            eng = engine(arch, w)
            cls, pat = eng.encode_image(px.cuda())
            return finish(eng, torch.cat([cls.reshape(B, -1), pat.reshape(B, -1)], 1))
    else:
        raise KeyError(name)
    c["device"] = device
    c.setdefault("keys", [k for k, v in c["w"].items() if v.is_floating_point()])
    _CASES[name] = c
    return c


def element(c, key, which):
    if which == 0:
        return 0
    g = torch.Generator().manual_seed(zlib.crc32(key.encode()))
    return int(torch.randint(c["w"][key].numel(), (1,), generator=g))


def poisoned(c, key, which):
    w = dict(c["w"])
    t = w[key].clone()
    t.view(-1)[element(c, key, which)] = float("nan")
    w[key] = t
    return w


def _bad_items(out):
    """[n, ...] outputs -> [n] bool: the item (pair, image) has a non-finite output."""
    return ~torch.isfinite(out.reshape(out.shape[0], -1)).all(1)


def oracle_P(c, key, which):
    """Items whose fp32 oracle output is not finite with w[key][element] = NaN (cached per case)."""
    if (key, which) not in c["P"]:
        torch.set_num_threads(8)
        with torch.no_grad():
            c["P"][(key, which)] = _bad_items(c["oracle"](poisoned(c, key, which)))
    return c["P"][(key, which)]


# (tensor, element: 0 = the first, 1 = the seeded one) whose NaN reaches no logit of the fp32 oracle on the case's batch, worked
# out with oracle_P on the CPU: the head the loss alone reads (single-head losses never read classifier2; with "2H_BCE" the
# returned logits are the second head's), embedding rows of tokens / positions / types that the batch does not contain.
_WORD = "context_text_encoder.bert_model.embeddings.word_embeddings.weight"
_CE_TYPE = "reranker.bert_model.embeddings.token_type_embeddings.weight"
_CE_POS = "reranker.bert_model.embeddings.position_embeddings.weight"
NOT_INPUTS = {
    "tiny_mm": [(_WORD, 1), (_CE_TYPE, 1), ("reranker.classifier2.weight", 0), ("reranker.classifier2.weight", 1),
                ("reranker.classifier2.bias", 0), ("reranker.classifier2.bias", 1)],
    "tiny_2h": [(_WORD, 1), (_CE_TYPE, 1), ("reranker.classifier1.weight", 0), ("reranker.classifier1.weight", 1),
                ("reranker.classifier1.bias", 0), ("reranker.classifier1.bias", 1)],
    "q8_small": [(_CE_POS, 1), ("reranker.classifier2.weight", 0), ("reranker.classifier2.weight", 1),
                 ("reranker.classifier2.bias", 0), ("reranker.classifier2.bias", 1)],
    "rm_tiny": [(_WORD, 1), ("context_text_encoder.bert_model.embeddings.token_type_embeddings.weight", 1), (_CE_TYPE, 1),
                ("reranker.classifier1.weight", 0), ("reranker.classifier1.weight", 1), ("reranker.classifier1.bias", 0),
                ("reranker.classifier1.bias", 1)],
    "int_tiny": [(_CE_TYPE, 1), ("reranker.classifier2.weight", 0), ("reranker.classifier2.weight", 1),
                 ("reranker.classifier2.bias", 0), ("reranker.classifier2.bias", 1)],
    "vit_tiny": [],
}

# A device forward may legitimately never read an element the oracle reads: by NAME, with the reason in the code.  None.
DEVICE_NEVER_READS = []


def sweep(name, dt, packed, elements, q8_format=None):
    c = case(name)
    with torch.no_grad():
        ref = c["oracle"](c["w"])
    clean, flag = c["device"](c["w"], dt, packed, q8_format)
    assert torch.isfinite(clean).all() and not flag, "the unpoisoned model must run clean"
    assert (clean.reshape(-1) - ref.reshape(-1)).abs().max().item() < 0.25, "device and oracle do not run the same model"
    skipped, silent = [], []
    for key in c["keys"]:
        for which in elements:
            P = oracle_P(c, key, which)
            if not bool(P.any()):
                skipped.append((key, which))
                continue
            if key in DEVICE_NEVER_READS:
                continue
            out, flag = c["device"](poisoned(c, key, which), dt, packed, q8_format)
            finite_on_P = ~_bad_items(out)[P]
            if not flag and bool(finite_on_P.any()):
                silent.append((key, which, int(finite_on_P.sum()), int(P.sum())))
    print(f"[nonfinite {name} {dt} packed={packed} q8={q8_format}] {len(c['keys'])} tensors x {len(elements)} elements, "
          f"{len(skipped)} not inputs, {len(silent)} silent")
    for s in silent:
        print("   SILENT", s)
    want_skipped = sorted(tuple(x) for x in NOT_INPUTS[name] if x[1] in elements)
    assert sorted(skipped) == want_skipped, (sorted(set(skipped) - set(want_skipped)), sorted(set(want_skipped) - set(skipped)))
    assert not silent, f"{len(silent)} poisoned tensors ranked silently (tensor, element, finite items of P, |P|): {silent}"


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["tiny_mm", "tiny_2h"])
def test_nan_weight_is_never_ranked_silently(name, dt, packed):
    """The default configuration (folded LayerNorm, split residual stream): every tensor, both elements."""
    sweep(name, dt, packed, (0, 1))


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["tiny_mm", "tiny_2h"])
def test_nan_weight_with_the_unfolded_fp32_stream(name, dt, packed):
    """ln_fold = 0, resid_split = 0 (the process-wide switches of tests/test_gpu_outliers.py): every tensor, both elements."""
    from rmr_amd import _lib
    lib = _lib.load()
    try:
        assert lib.rr_set_tuning(b"ln_fold", 0) == 0 and lib.rr_set_tuning(b"resid_split", 0) == 0
        sweep(name, dt, packed, (0, 1))
    finally:
        lib.rr_set_tuning(b"ln_fold", 1)
        lib.rr_set_tuning(b"resid_split", 1)


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("q8_format", [0, 1], ids=["e4m3", "int8"])
def test_nan_weight_in_the_8bit_configurations(q8_format, dt, packed):
    """fp8 = 1 with fp8_first_layer = 0 (every layer on the 8-bit GEMMs), e4m3 and int8 weights: every tensor, both elements.  The host
    packers give a row that holds a NaN a NaN scale, the quantising LayerNorm a NaN row scale."""
    sweep("q8_small", dt, packed, (0, 1), q8_format)


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["rm_tiny", "int_tiny"])
def test_nan_weight_in_the_joint_and_interaction_rerankers(name, dt, packed):
    """forward_joint (RerankModel, `rm_tiny`) and forward_interaction (`int_tiny`) against their oracles: every tensor, both elements."""
    sweep(name, dt, packed, (0, 1))


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_nan_weight_in_the_vision_tower(dt):
    """encode_image on `vit_tiny`: an image whose oracle features are not finite has non-finite device features, or the flag is up."""
    sweep("vit_tiny", dt, False, (0, 1))
