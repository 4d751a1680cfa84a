"""Host-side mirror of the reference's reranker plug-in interface, on top of librerank_mi355.so.

Reference interface mirrored (paths relative to /root/reference/):
  * plug-in construction `RerankerClass(reranker_config)` — src/executors/Reranker_base_executor.py:191-202
  * `FullContextRerankModel.forward(query_text_sequences, query_pixel_values, context_text_sequences,
     num_negative_examples, labels=None)` — src/models/rerank/rerank_model.py:523-591
  * return `EasyDict(loss=<0-dim tensor>, logits=<tensor>)` consumed at Reranker_base_executor.py:922-927
  * error behaviour: AssertionError on N != Bq*K / label count (rerank_model.py:527-529), ValueError for
    labels with negative_sampling (utils.py:233), NotImplementedError for unsupported variants.

Nothing here computes: tensors are only allocated and handed to the C ABI by address.  If the HIP
library is missing, or no MI355X is visible, construction raises — there is no eager/CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence

import torch

from . import _lib as L
from .pair_inputs import group_pairs_by_length, pack_fusion_scores, pack_rows, pair_lengths, scatter_packed


class RerankOutput(dict):
    """EasyDict-style result: `.loss` (0-dim fp32 device tensor), `.logits` (fp32 device tensor)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    __setattr__ = dict.__setitem__


def _get(cfg, name, default=None):
    if cfg is None:
        return default
    if isinstance(cfg, dict):
        return cfg.get(name, default)
    return getattr(cfg, name, default)


# bert-base-uncased / PreFLMR ViT-B architecture (configuration_flmr.py:90-122,220-236,332-350)
FLMR_DEFAULTS = dict(vocab_size=30522, hidden=768, layers=12, heads=12, intermediate=3072, max_pos=512,
                     type_vocab=2, ln_eps=1e-12, li_dim=128, vision_hidden=768, prefix_len=32, n_patches=49,
                     map_layers=1, cross_attn_len=32)
# CLIP ViT-B/32 vision tower (FLMRVisionConfig, configuration_flmr.py:90-104); vit_layers = 0 leaves the image
# features to the caller (image_feature_fn / image_features=)
VIT_DEFAULTS = dict(vit_layers=0, vit_heads=12, vit_intermediate=3072, vit_image_size=224, vit_patch_size=32)
CE_DEFAULTS = dict(ce_hidden=768, ce_heads=12, ce_intermediate=3072)   # cross_encoder_config_base = bert-base-uncased


def make_arch(reranker_config=None, **overrides) -> dict:
    """Architecture dict from a reference-style `reranker_config` (EasyDict/dict/object with
    `cross_encoder_num_hidden_layers`, `cross_encoder_max_position_embeddings`, `loss_fn`, `pos_weight`,
    ... — monoBERT_pointwise.jsonnet:111-122) plus optional `arch` overrides for the FLMR side."""
    a = dict(FLMR_DEFAULTS)
    a.update(CE_DEFAULTS)
    a.update(VIT_DEFAULTS)
    if _get(reranker_config, "vision_encoder", False):     # run the CLIP tower inside the library
        a["vit_layers"] = 12
    a.update(ce_layers=_get(reranker_config, "cross_encoder_num_hidden_layers", 1),
             ce_max_pos=_get(reranker_config, "cross_encoder_max_position_embeddings", 750),
             loss_fn=_get(reranker_config, "loss_fn", "BCE"),
             pos_weight=_get(reranker_config, "pos_weight", None),
             has_vision=1,
             compute_dtype=_get(reranker_config, "compute_dtype", "bf16"),   # "bf16" | "fp16" MFMA operands
             model_kind="full_context")
    a.update(_get(reranker_config, "arch", None) or {})
    a.update(overrides)
    return a


def weight_spec(a: dict) -> List[tuple]:
    """(name, shape, kind) of every tensor the path reads, named by the reference state_dict keys."""
    H, I, D = a["hidden"], a["intermediate"], a["li_dim"]

    def layer(p, Hh, Ii, cross):
        out = []
        for att in ["attention"] + (["crossattention"] if cross else []):
            for n in ("query", "key", "value"):
                out += [(f"{p}.{att}.self.{n}.weight", (Hh, Hh), "w"), (f"{p}.{att}.self.{n}.bias", (Hh,), "b")]
            out += [(f"{p}.{att}.output.dense.weight", (Hh, Hh), "w"), (f"{p}.{att}.output.dense.bias", (Hh,), "b"),
                    (f"{p}.{att}.output.LayerNorm.weight", (Hh,), "g"), (f"{p}.{att}.output.LayerNorm.bias", (Hh,), "b")]
        out += [(f"{p}.intermediate.dense.weight", (Ii, Hh), "w"), (f"{p}.intermediate.dense.bias", (Ii,), "b"),
                (f"{p}.output.dense.weight", (Hh, Ii), "w"), (f"{p}.output.dense.bias", (Hh,), "b"),
                (f"{p}.output.LayerNorm.weight", (Hh,), "g"), (f"{p}.output.LayerNorm.bias", (Hh,), "b")]
        return out

    s = []
    kind = a.get("model_kind", "full_context")
    if kind != "full_context":          # InteractionRerankModel: input mapping + reranker only
        Hc, Ic = a["ce_hidden"], a["ce_intermediate"]
        s += [("cross_encoder_input_mapping.weight", (Hc, D), "w"), ("cross_encoder_input_mapping.bias", (Hc,), "b")]
        if kind == "interaction":
            p = "reranker.bert_model"
            s += [(f"{p}.embeddings.position_embeddings.weight", (a["ce_max_pos"], Hc), "e"),
                  (f"{p}.embeddings.token_type_embeddings.weight", (a["type_vocab"], Hc), "e"),
                  (f"{p}.embeddings.LayerNorm.weight", (Hc,), "g"), (f"{p}.embeddings.LayerNorm.bias", (Hc,), "b")]
            for i in range(a["ce_layers"]):
                s += layer(f"{p}.encoder.layer.{i}", Hc, Ic, False)
        else:
            for i in range(a["ce_layers"]):
                s += layer(f"reranker.interaction_module.{i}", Hc, Ic, True)
        s += [("reranker.classifier1.weight", (1, Hc), "w"), ("reranker.classifier1.bias", (1,), "b"),
              ("reranker.classifier2.weight", (1, Hc), "w"), ("reranker.classifier2.bias", (1,), "b")]
        return s
    p = "context_text_encoder.bert_model"
    s += [(f"{p}.embeddings.word_embeddings.weight", (a["vocab_size"], H), "e"),
          (f"{p}.embeddings.position_embeddings.weight", (a["max_pos"], H), "e"),
          (f"{p}.embeddings.token_type_embeddings.weight", (a["type_vocab"], H), "e"),
          (f"{p}.embeddings.LayerNorm.weight", (H,), "g"), (f"{p}.embeddings.LayerNorm.bias", (H,), "b")]
    for i in range(a["layers"]):
        s += layer(f"{p}.encoder.layer.{i}", H, I, False)
    s += [("context_text_encoder_linear.weight", (D, H), "w")]
    if a["has_vision"]:
        Vh, PL = a["vision_hidden"], a["prefix_len"]
        s += [("context_vision_projection.model.0.weight", (D * PL // 2, Vh), "w"),
              ("context_vision_projection.model.0.bias", (D * PL // 2,), "b"),
              ("context_vision_projection.model.2.weight", (D * PL, D * PL // 2), "w"),
              ("context_vision_projection.model.2.bias", (D * PL,), "b"),
              ("transformer_mapping_input_linear.weight", (H, Vh), "w"),
              ("transformer_mapping_input_linear.bias", (H,), "b")]
        for i in range(a["map_layers"]):
            s += layer(f"transformer_mapping_network.layer.{i}", H, I, True)
        s += [("transformer_mapping_output_linear.weight", (D, H), "w"),
              ("transformer_mapping_output_linear.bias", (D,), "b")]
    if a.get("vit_layers", 0) > 0:
        s += vit_weight_spec(a)
    Hc, Ic = a["ce_hidden"], a["ce_intermediate"]
    s += [("cross_encoder_input_mapping.weight", (Hc, D), "w"), ("cross_encoder_input_mapping.bias", (Hc,), "b")]
    p = "reranker.bert_model"
    s += [(f"{p}.embeddings.position_embeddings.weight", (a["ce_max_pos"], Hc), "e"),
          (f"{p}.embeddings.token_type_embeddings.weight", (a["type_vocab"], Hc), "e"),
          (f"{p}.embeddings.LayerNorm.weight", (Hc,), "g"), (f"{p}.embeddings.LayerNorm.bias", (Hc,), "b")]
    for i in range(a["ce_layers"]):
        s += layer(f"{p}.encoder.layer.{i}", Hc, Ic, False)
    s += [("reranker.classifier1.weight", (1, Hc), "w"), ("reranker.classifier1.bias", (1,), "b"),
          ("reranker.classifier2.weight", (1, Hc), "w"), ("reranker.classifier2.bias", (1,), "b")]
    return s


VIT_PREFIX = "context_vision_encoder.vision_model.vision_model"   # FLMRVisionModel -> CLIPVisionModel -> transformer


def vit_weight_spec(a: dict) -> List[tuple]:
    """CLIP vision tower tensors under the reference's state_dict keys (modeling_flmr.py:1684-1757)."""
    Vh, Iv, ps, v = a["vision_hidden"], a["vit_intermediate"], a["vit_patch_size"], VIT_PREFIX
    s = [(f"{v}.embeddings.class_embedding", (Vh,), "e"),
         (f"{v}.embeddings.patch_embedding.weight", (Vh, 3, ps, ps), "w"),
         (f"{v}.embeddings.position_embedding.weight", (a["n_patches"] + 1, Vh), "e"),
         (f"{v}.pre_layrnorm.weight", (Vh,), "g"), (f"{v}.pre_layrnorm.bias", (Vh,), "b")]
    for i in range(a["vit_layers"]):
        l = f"{v}.encoder.layers.{i}"
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            s += [(f"{l}.self_attn.{n}.weight", (Vh, Vh), "w"), (f"{l}.self_attn.{n}.bias", (Vh,), "b")]
        s += [(f"{l}.layer_norm1.weight", (Vh,), "g"), (f"{l}.layer_norm1.bias", (Vh,), "b"),
              (f"{l}.mlp.fc1.weight", (Iv, Vh), "w"), (f"{l}.mlp.fc1.bias", (Iv,), "b"),
              (f"{l}.mlp.fc2.weight", (Vh, Iv), "w"), (f"{l}.mlp.fc2.bias", (Vh,), "b"),
              (f"{l}.layer_norm2.weight", (Vh,), "g"), (f"{l}.layer_norm2.bias", (Vh,), "b")]
    return s


def synthetic_state_dict(a: dict, seed: int = 0, hf_init: bool = True, gain: float = 1.0) -> Dict[str, torch.Tensor]:
    """Seeded random-init weights (HF init: N(0, 0.02) matrices/embeddings, LN 1/0, zero biases —
    modeling_flmr.py:199-214) for benchmarks: there are no checkpoints in the build environment.
    Each tensor has its own generator seeded by (seed, index), identical to the test oracle's scheme so the
    CPU baseline can be fed the very same weights.  `gain` > 1 widens the Linear matrices only (the test suite's weight generator
    does the same): at 2.5 attention is peaked and a candidate list spreads over ~0.2 in logit, as in tests/golden c3_sep."""
    w = {}
    for idx, (name, shape, kind) in enumerate(weight_spec(a)):
        g = torch.Generator().manual_seed(seed * 1000003 + idx)
        if kind in ("w", "e"):
            t = torch.randn(shape, generator=g) * (0.02 * (gain if kind == "w" else 1.0))
        elif kind == "g":
            t = torch.ones(shape) if hf_init else 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            t = torch.zeros(shape) if hf_init else 0.05 * torch.randn(shape, generator=g)
        w[name] = t
    return w


def _ptrs(out: dict) -> list:
    """The output pointers of a forward / head call, in the C ABI's order (absent outputs are null)."""
    return [L.ptr(out[k]) for k in ("logits", "logits2", "loss", "scores", "order") if k in out]


def _bank_centroids(bank) -> int:
    """The centroids a bank's codes index: a compressed bank's codec's, an fp16 bank's table's (PassageBank.set_centroids); 0: no codes."""
    n = getattr(bank, "n_centroids", None)
    if n is None:
        codec = getattr(bank, "codec", None)
        n = 0 if codec is None else codec.n_centroids
    return int(n)


def _bank_search_args(eng, name: str, bank, query_li: torch.Tensor, first: int, count: Optional[int], needs_codes: bool = False):
    """What RerankEngine.bank_search and bank_search_plaid (`name`) check and prepare alike: (first, n, n_queries, Lq, the queries
    as contiguous float32 on the engine's device)."""
    D = eng.arch["li_dim"]
    if query_li.dim() != 3 or query_li.shape[2] != D:
        raise ValueError(f"query_li {tuple(query_li.shape)}: [n_queries, Lq, {D}]")
    if needs_codes and not _bank_centroids(bank):      # a compressed bank, or an fp16 bank with a centroid table
        raise NotImplementedError(f"{name}: an fp16 bank (the pruned search reads the centroid codes of a compressed bank)")
    held = len(bank)
    first = int(first)
    n = held - first if count is None else int(count)
    if first < 0 or n < 1 or first + n > held:
        raise ValueError(f"{name}: passages [{first}, {first} + {n}) of a bank that holds {held}")
    nq, Lq = int(query_li.shape[0]), int(query_li.shape[1])
    if nq < 1 or Lq < 1:
        raise ValueError(f"query_li {tuple(query_li.shape)}: no query tokens")
    return first, n, nq, Lq, query_li.to(device=eng.device, dtype=torch.float32).contiguous()


def _bank_search_filtered(eng, what: str, bank, query_li, k, filter, first, count) -> dict:
    """RerankEngine.bank_search_filtered and bank_search_filtered_sparse (`what`; the entry is rr_ + what): one set of checks, one
    result dict."""
    first, n, nq, Lq, q = _bank_search_args(eng, what, bank, query_li, first, count)
    k = int(k)
    if k < 1 or k > n:
        raise ValueError(f"{what}: k = {k} of {n} passages")
    if k > 1024:
        raise NotImplementedError(f"{what}: k = {k} (at most 1024)")
    fargs = _bank_filter_args(what, filter, nq, first, n)
    out = dict(indices=torch.empty((nq, k), device=eng.device, dtype=torch.int32),
               scores=torch.empty((nq, k), device=eng.device, dtype=torch.float32),
               counts=torch.empty((nq,), device=eng.device, dtype=torch.int32))
    L.check(getattr(eng.lib, "rr_" + what)(eng.h, bank.h, L.ptr(q), nq, Lq, first, n, k, *fargs, L.ptr(out["indices"]),
                                           L.ptr(out["scores"]), L.ptr(out["counts"]), eng._stream()), eng.h, "rr_" + what)
    return out


def _bank_filter_args(name: str, filter, nq: int, first: int, n: int) -> list:
    """The three filter arguments of a filtered search (bits, rows, words per row) from a BankFilter, checked against the call:
    one row or one per query, built for at least the passages of the range (ValueError)."""
    rows, ld = int(filter.bits.shape[0]), int(filter.bits.shape[1])
    if rows not in (1, nq):
        raise ValueError(f"{name}: a filter of {rows} rows for {nq} queries (1, or one per query)")
    if filter.passages < first + n or ld * 32 < first + n:
        raise ValueError(f"{name}: the filter was built for {filter.passages} passages, the range ends at {first + n}: build it again "
                         "(PassageBank.filter)")
    return [L.ptr(filter.bits), rows, ld]


def _bank_search_plaid(eng, entry: str, bank, query_li: torch.Tensor, k: int, *, ncells: int, centroid_score_threshold: float, ndocs: int,
                       coarse_tokens: Optional[int] = None, first: int = 0, count: Optional[int] = None, filter=None) -> dict:
    """RerankEngine.bank_search_plaid and bank_search_plaid_ivf, and their filtered entries (`filter`: a BankFilter): the checks
    before the library, the outputs, the call of `entry`."""
    first, n, nq, Lq, q = _bank_search_args(eng, "bank_search_plaid", bank, query_li, first, count, needs_codes=True)
    n_centroids = _bank_centroids(bank)
    Lqc = Lq if coarse_tokens is None else int(coarse_tokens)
    if Lqc < 1 or Lqc > Lq:
        raise ValueError(f"bank_search_plaid: coarse_tokens = {Lqc} of {Lq} query tokens")
    ncells, ndocs, k = int(ncells), int(ndocs), int(k)
    if ncells < 1 or ncells > n_centroids:
        raise ValueError(f"bank_search_plaid: ncells = {ncells} of {n_centroids} centroids")
    if ncells > 16:
        raise NotImplementedError(f"bank_search_plaid: ncells = {ncells} (at most 16)")
    if ndocs < 4:
        raise ValueError(f"bank_search_plaid: ndocs = {ndocs} (at least 4)")
    if ndocs > 1024:
        raise NotImplementedError(f"bank_search_plaid: ndocs = {ndocs} (at most 1024)")
    if k < 1 or k > min(ndocs // 4, n):
        raise ValueError(f"bank_search_plaid: k = {k} of ndocs // 4 = {ndocs // 4} survivors and {n} passages")
    out = dict(indices=torch.empty((nq, k), device=eng.device, dtype=torch.int32),
               scores=torch.empty((nq, k), device=eng.device, dtype=torch.float32),
               counts=torch.empty((nq,), device=eng.device, dtype=torch.int32))
    fargs = [] if filter is None else _bank_filter_args("bank_search_plaid", filter, nq, first, n)
    L.check(getattr(eng.lib, entry)(eng.h, bank.h, L.ptr(q), nq, Lq, Lqc, first, n, ncells, float(centroid_score_threshold), ndocs, k,
                                     *fargs, L.ptr(out["indices"]), L.ptr(out["scores"]), L.ptr(out["counts"]), eng._stream()),
            eng.h, entry)
    return out


class RerankEngine:
    """Owns one `rr_handle` (one model replica on one GPU)."""

    def __init__(self, arch: dict, device: Optional[torch.device] = None):
        self.lib = L.load()
        if not torch.cuda.is_available():
            raise RuntimeError("rmr_amd needs an MI355X (gfx950) visible to HIP; there is no CPU fallback")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.arch = dict(arch)
        c = L.RRConfig()
        c.abi_version = L.RR_ABI_VERSION
        for k in ("vocab_size", "hidden", "layers", "heads", "intermediate", "max_pos", "type_vocab", "li_dim",
                  "ce_hidden", "ce_layers", "ce_heads", "ce_intermediate", "ce_max_pos", "has_vision",
                  "vision_hidden", "prefix_len", "n_patches", "map_layers", "cross_attn_len"):
            setattr(c, k, int(arch[k]))
        c.ln_eps = float(arch["ln_eps"])
        if arch["loss_fn"] not in L.LOSS_KINDS:
            raise ValueError(f"Unknown loss function {arch['loss_fn']}")        # utils.py:222-223
        c.loss_kind = L.LOSS_KINDS[arch["loss_fn"]]
        c.pos_weight = float("nan") if arch.get("pos_weight") is None else float(arch["pos_weight"])
        cd = arch.get("compute_dtype", "bf16")
        if cd not in L.COMPUTE_DTYPES:
            raise ValueError(f"compute_dtype must be one of {sorted(L.COMPUTE_DTYPES)}, got {cd!r}")
        c.compute_dtype = L.COMPUTE_DTYPES[cd]
        mk = arch.get("model_kind", "full_context")
        if mk not in L.MODEL_KINDS:
            raise ValueError(f"model_kind must be one of {sorted(L.MODEL_KINDS)}, got {mk!r}")
        c.model_kind = L.MODEL_KINDS[mk]
        for k, v in VIT_DEFAULTS.items():
            setattr(c, k, int(arch.get(k, v)))
        c.fp8 = int(bool(arch.get("fp8", 0)))      # BASELINE configs[4]: e4m3 QKV / FFN-up GEMMs (rr_config.fp8)
        c.device = self.device.index if self.device.index is not None else torch.cuda.current_device()
        h = C.c_void_p()
        L.check(self.lib.rr_create(C.byref(c), C.byref(h)), None, "rr_create")
        self.h = h
        self.finalized = False
        if arch.get("q8_format") is not None:      # 8-bit operand format of rr_config.fp8 (0 e4m3, 1 int8): latched at finalize
            self.set_option("q8_format", int(arch["q8_format"]))

    def __del__(self):
        h = getattr(self, "h", None)
        if h:
            try:
                self.lib.rr_destroy(h)
            except Exception:
                pass
            self.h = None

    # ---- weights ------------------------------------------------------------------------------
    def required_weight_names(self) -> List[str]:
        n = self.lib.rr_num_required_weights(self.h)
        return [self.lib.rr_required_weight_name(self.h, i).decode() for i in range(n)]

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = False, prefix: str = "") -> List[str]:
        """Feed a reference-named state_dict (Lightning ckpt keys carry a `reranker.` executor prefix:
        pass prefix="reranker.").  Unknown keys are ignored like load_state_dict(strict=False)
        (Reranker_base_executor.py:366-381); missing required tensors raise KeyError."""
        unexpected = []
        for k, t in sd.items():
            if prefix:
                if not k.startswith(prefix):
                    unexpected.append(k)
                    continue
                k = k[len(prefix):]
            t = t.detach().to("cpu").contiguous()
            if t.dtype == torch.float32:
                dt = L.RR_F32
            elif t.dtype == torch.bfloat16:
                dt = L.RR_BF16
            elif t.dtype == torch.float16:
                dt = L.RR_F16
            else:
                raise ValueError(f"{k}: unsupported dtype {t.dtype}")
            shape = (C.c_int64 * max(1, t.dim()))(*t.shape)
            known = C.c_int(0)
            L.check(self.lib.rr_load_weight(self.h, k.encode(), t.data_ptr(), dt, t.dim(), shape, C.byref(known)),
                    self.h, "rr_load_weight")
            if not known.value:
                unexpected.append(k)
        if strict and unexpected:
            raise KeyError(f"unexpected keys: {unexpected[:5]}...")
        L.check(self.lib.rr_finalize_weights(self.h), self.h, "rr_finalize_weights")
        self.finalized = True
        return unexpected

    # ---- forward ------------------------------------------------------------------------------
    def forward_ids(self, input_ids: torch.Tensor, attention_mask: torch.Tensor,
                    token_type_ids: Optional[torch.Tensor], Bq: int, K: int,
                    image_cls: Optional[torch.Tensor] = None, image_patches: Optional[torch.Tensor] = None,
                    labels: Optional[torch.Tensor] = None, want_scores: bool = False, want_order: bool = False,
                    pair_range: Optional[Sequence[int]] = None, want_loss: bool = True):
        """One pass over the tokenised pair batch.  All tensors live on `self.device`.
        Returns dict(logits [N] fp32, logits2 [N], loss 0-dim | None, scores | None, order [Bq,K] | None)."""
        dev = self.device
        N = input_ids.shape[0]
        assert N == Bq * K, f"expanded batch {Bq}*{K} != {N}"                 # rerank_model.py:527
        S = input_ids.shape[1]
        for t in (input_ids, attention_mask) + ((token_type_ids,) if token_type_ids is not None else ()):
            if t.dtype != torch.int64 or t.device != dev or tuple(t.shape) != (N, S):
                raise ValueError("input_ids/attention_mask/token_type_ids must be int64 [N,S] on the model device")
        if labels is not None:
            assert labels.numel() == N, "len(labels) != expanded batch size"   # rerank_model.py:528-529
            labels = labels.to(device=dev, dtype=torch.float32).contiguous()
        if image_cls is not None:
            image_cls = image_cls.to(device=dev, dtype=torch.float32).contiguous()
            image_patches = image_patches.to(device=dev, dtype=torch.float32).contiguous()
            if image_cls.shape[0] != Bq or image_patches.shape[0] != Bq:
                raise AssertionError("image features must be per query: [Bq, ...]")
        pb, pe, out = self._outputs(Bq, K, pair_range, want_loss, want_scores, want_order)
        L.check(self.lib.rr_forward(self.h, L.ptr(input_ids), L.ptr(attention_mask), L.ptr(token_type_ids),
                                    L.ptr(image_cls), L.ptr(image_patches), Bq, K, S, L.ptr(labels), pb, pe, *_ptrs(out),
                                    self._stream()), self.h, "rr_forward")
        return out

    def forward_ids_bucketed(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, token_type_ids: Optional[torch.Tensor],
                             Bq: int, K: int, image_cls: Optional[torch.Tensor] = None,
                             image_patches: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
                             buckets: Sequence[int] = (128, 256, 384), want_scores: bool = False,
                             want_order: bool = False):
        """The same result as `forward_ids` on right-padded pairs, computed per LENGTH BUCKET: the reference pads every pair
        to max_decoder_source_length (utils.py:157-165) and real passages are far shorter, so the pairs are grouped by the
        smallest bucket length that holds their last non-pad position, each group runs with that row length (its GEMMs,
        LayerNorms and query rows shrink in proportion; rr_set_padded_seq_len keeps the cross-encoder's vision positions) and
        the head / top-K run once on the reassembled logits (rr_head).  One device -> host copy of N lengths per call.
        Bucket sizes: every group is its own forward (~135 launches) over fewer pairs, so few, wide buckets win: measured
        on 800 pairs of length U[64, 512] (bench.py --regime realistic --bucketed): (128, 256, 384) 71.5 ms, (192, 320) 74.8,
        (256,) 77.8, five buckets 77.5, seven 82.1, against 94.5 ms padded.
        Text-only: logits bit-identical to forward_ids WHILE every bucket and the padded call lie on the same side of two size
        thresholds (include/rerank_mi355.h, rr_set_padded_seq_len: the 1 024-workgroup attention schedule switch and the
        128-tile switch between the fp32 and the (hi, lo) residual stream, about 11k rows at hidden 768); across them, and with
        vision tokens (other key-tile cuts in the cross-encoder's attention), equal to the parity tolerance — 1e-3 in fp16,
        measured ~2e-4 — not to the bit.  Returns the dict of forward_ids."""
        dev = self.device
        N, S = input_ids.shape
        assert N == Bq * K
        lens = pair_lengths(input_ids, attention_mask)                 # 1 + index of the last non-pad position
        # with vision tokens the mapping network attends to the first cross_attn_len text rows: no bucket below that (the
        # library refuses it: RR_ERR_BAD_SHAPE)
        floor = min(S, int(self.arch.get("cross_attn_len", 32))) if image_cls is not None else 1
        sizes = sorted({max(int(b), floor) for b in buckets if 0 < int(b) < S and max(int(b), floor) < S}) + [S]
        which = torch.bucketize(lens, torch.tensor(sizes, device=dev))  # smallest bucket with size >= len
        counts = torch.bincount(which, minlength=len(sizes)).cpu().tolist()
        logits = torch.empty(N, dtype=torch.float32, device=dev)
        logits2 = torch.empty(N, dtype=torch.float32, device=dev)
        two = self.arch["loss_fn"] == "2H_BCE"
        L.check(self.lib.rr_set_padded_seq_len(self.h, S), self.h, "rr_set_padded_seq_len")
        try:
            order_by_bucket = torch.argsort(which, stable=True)
            o = 0
            for b, n in enumerate(counts):
                if n == 0:
                    continue
                idx = order_by_bucket[o: o + n]
                o += n
                Sb = sizes[b]
                sub = [t.index_select(0, idx)[:, :Sb].contiguous() if t is not None else None
                       for t in (input_ids, attention_mask, token_type_ids)]
                cls_b = pat_b = None
                if image_cls is not None:                               # per pair here: the group mixes candidates of several queries
                    q = torch.div(idx, K, rounding_mode="floor")
                    cls_b, pat_b = image_cls.index_select(0, q), image_patches.index_select(0, q)
                r = self.forward_ids(sub[0], sub[1], sub[2], n, 1, cls_b, pat_b, None, want_loss=False)
                logits.index_copy_(0, idx, r["logits"])
                if two:
                    logits2.index_copy_(0, idx, r["logits2"])
        finally:
            self.lib.rr_set_padded_seq_len(self.h, 0)
        out = self.head(logits, logits2 if two else None, labels, Bq, K, want_scores=want_scores, want_order=want_order)
        out["logits"], out["logits2"] = logits, logits2
        out["bucket_rows"] = sum(n * sizes[b] for b, n in enumerate(counts))      # rows actually computed (N * S when nothing fits a bucket)
        return out

    def forward_ids_packed(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, token_type_ids: Optional[torch.Tensor],
                           Bq: int, K: int, image_cls: Optional[torch.Tensor] = None,
                           image_patches: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
                           granule: int = 16, want_scores: bool = False, want_order: bool = False,
                           lengths: Optional[Sequence[int]] = None, segment_cost_rows: int = 0, want_loss: bool = True,
                           list_sizes: Optional[Sequence[int]] = None, pair_lists=None):
        """The same result as `forward_ids` on right-padded pairs, computed over PACKED rows (rr_forward_packed): the pairs are
        grouped by their length rounded up to a multiple of `granule` and laid out group after group, so that every GEMM /
        LayerNorm pass of a layer runs once over the rows that exist — the reference pads every pair to
        max_decoder_source_length (utils.py:157-165) — while attention runs once per group.  Against forward_ids_bucketed
        (one whole forward per group): the same rows at granule 128, but one large GEMM launch and ONE attention launch per
        layer for all groups instead of one per group, which is what lets the granule shrink (measured on lengths U[64, 512]:
        granule 64 / 32 / 16 / 8 -> 62.1 / 60.6 / 59.7 / 62.5 ms against 93.2 padded).  Logits: bit-identical to forward_ids_bucketed on the same groups, i.e.
        to forward_ids for text-only models.  `lengths`: the pairs' token counts (1 + index of the last non-pad position) as
        the HOST knows them from the tokenizer (pair_inputs.prepare_full_context_inputs keeps them); without it they are
        derived on the device and the group counts cost one device -> host copy per call, which drains the stream between
        two forwards.  `segment_cost_rows`: merge neighbouring lengths where a segment's fixed launches cost more than the rows
        the merge pads (pair_inputs.group_pairs_by_length).  `list_sizes` / `pair_lists` in place of (Bq, K) (pass None for both):
        lists of unequal length, or a slice of them (see `_packed`).  Returns the dict of forward_ids plus `packed_rows`,
        `packed_segments`."""
        N, S = input_ids.shape
        Bq, K, pair_query = self._layout(N, Bq, K, list_sizes, pair_lists)
        floor = int(self.arch.get("cross_attn_len", 32)) if image_cls is not None else 1   # the mapping network's cross-attention window

        def launch(order, seg_n, seg_len, sn, sl, lp, lp2):
            ids_p, am_p = pack_rows(input_ids, order, seg_n, seg_len), pack_rows(attention_mask, order, seg_n, seg_len)
            tt_p = pack_rows(token_type_ids, order, seg_n, seg_len) if token_type_ids is not None else None
            cls_p = pat_p = None
            if image_cls is not None:                                   # per pair: a group mixes candidates of several queries
                q = pair_query(order)
                cls_p = image_cls.index_select(0, q).float().contiguous()
                pat_p = image_patches.index_select(0, q).float().contiguous()
            L.check(self.lib.rr_forward_packed(self.h, L.ptr(ids_p), L.ptr(am_p), L.ptr(tt_p), L.ptr(cls_p), L.ptr(pat_p), len(seg_n),
                                               sn, sl, S, L.ptr(lp), L.ptr(lp2), self._stream()), self.h, "rr_forward_packed")
        return self._packed(launch, (input_ids, attention_mask), lengths, S, floor, granule, segment_cost_rows, Bq, K, labels,
                            want_loss, want_scores, want_order, list_sizes=list_sizes, pair_lists=pair_lists, n_pairs=N)

    def assemble_pairs(self, pool: torch.Tensor, desc, order, seg_n: Sequence[int], seg_len: Sequence[int], special_ids: Sequence[int],
                       with_token_types: bool = True):
        """rr_assemble_pairs: the packed int64 (input_ids, attention_mask, token_type_ids) rows of rr_forward_packed, built on the
        device from the compact tokens of NativePairTokenizer.prepare_compact.  `pool`: int32 device tensor; `desc`: host int32
        [N, 4] (query offset, la, context offset, lb); `order`: host pair order; `seg_n` / `seg_len`: the segment table
        (group_pairs_by_length); `special_ids`: (cls, sep, pad).  The padded [N, S] rows are order = arange(N), seg_n = [N],
        seg_len = [S].  A descriptor outside the pool or longer than its segment raises ValueError before anything is written."""
        import numpy as np
        dev = self.device
        if pool.dtype != torch.int32 or pool.device != dev or not pool.is_contiguous():
            raise ValueError("pool must be a contiguous int32 tensor on the model device")
        desc = np.ascontiguousarray(desc, dtype=np.int32)
        order = np.ascontiguousarray(order, dtype=np.int32).reshape(-1)
        if desc.ndim != 2 or desc.shape[1] != 4 or desc.shape[0] != order.shape[0]:
            raise ValueError("desc must be [N, 4] with one order entry per pair")
        rows = sum(int(n) * int(l) for n, l in zip(seg_n, seg_len))
        ids, am = (torch.empty(rows, dtype=torch.int64, device=dev) for _ in range(2))
        tt = torch.empty(rows, dtype=torch.int64, device=dev) if with_token_types else None
        cls_id, sep_id, pad_id = (int(x) for x in special_ids)
        rc = self.lib.rr_assemble_pairs(self.h, L.ptr(pool), pool.numel(), desc.ctypes.data, desc.shape[0], order.ctypes.data,
                                        len(seg_n), (C.c_int32 * len(seg_n))(*seg_n), (C.c_int32 * len(seg_n))(*seg_len), cls_id,
                                        sep_id, pad_id, L.ptr(ids), L.ptr(am), L.ptr(tt), self._stream())
        if rc == L.RR_ERR_BAD_SHAPE:        # a bad descriptor is a bad argument of this call, not an expanded-batch mismatch
            raise ValueError(f"rr_assemble_pairs: {self.lib.rr_last_error(self.h).decode()}")
        L.check(rc, self.h, "rr_assemble_pairs")
        return ids, am, tt

    def forward_tokens_packed(self, pool: torch.Tensor, desc, Bq: int, K: int, image_cls: Optional[torch.Tensor] = None,
                              image_patches: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
                              granule: int = 16, segment_cost_rows: int = 0, want_scores: bool = False, want_order: bool = False,
                              want_loss: bool = True, padded_len: int = 512, special_ids: Sequence[int] = (101, 102, 0),
                              list_sizes: Optional[Sequence[int]] = None):
        """forward_ids_packed from COMPACT tokens (NativePairTokenizer.prepare_compact): the pool on the device, the
        descriptors on the host, the rows assembled on the device by rr_assemble_pairs where forward_ids_packed packs padded
        rows with pack_rows.  `padded_len` is the length the padded call would use (max_decoder_source_length), `special_ids`
        the tokenizer's (cls, sep, pad).  Same grouping, image features per pair, scatter and head as forward_ids_packed, so
        the same logits: bit for bit for text-only models.  Returns the dict of forward_ids_packed."""
        import numpy as np
        desc = np.ascontiguousarray(desc, dtype=np.int32)
        N = Bq * K if list_sizes is None else int(sum(list_sizes))
        assert desc.shape == (N, 4), f"expanded batch {Bq}*{K} != {desc.shape[0]}"
        Bq, K, pair_query = self._layout(N, Bq, K, list_sizes, None)
        lengths = desc[:, 1].astype(np.int64) + desc[:, 3] + 3
        floor = int(self.arch.get("cross_attn_len", 32)) if image_cls is not None else 1

        def launch(order, seg_n, seg_len, sn, sl, lp, lp2, order_h):
            ids_p, am_p, tt_p = self.assemble_pairs(pool, desc, order_h, seg_n, seg_len, special_ids)
            cls_p = pat_p = None
            if image_cls is not None:                                   # per pair: a group mixes candidates of several queries
                q = pair_query(order)
                cls_p = image_cls.index_select(0, q).float().contiguous()
                pat_p = image_patches.index_select(0, q).float().contiguous()
            L.check(self.lib.rr_forward_packed(self.h, L.ptr(ids_p), L.ptr(am_p), L.ptr(tt_p), L.ptr(cls_p), L.ptr(pat_p), len(seg_n),
                                               sn, sl, int(padded_len), L.ptr(lp), L.ptr(lp2), self._stream()), self.h,
                    "rr_forward_packed")
        return self._packed(launch, (), lengths, int(padded_len), floor, granule, segment_cost_rows, Bq, K, labels, want_loss,
                            want_scores, want_order, host_order=True, list_sizes=list_sizes, n_pairs=N)

    def assemble_joint(self, pool: torch.Tensor, desc, order, seg_n: Sequence[int], seg_len: Sequence[int], query_len: int,
                       padded_len: int, special_ids: Sequence[int]):
        """rr_assemble_joint: the packed int64 (joint_input_ids, joint_attention_mask) rows of rr_forward_joint_packed, built on
        the device from compact tokens.  `pool`: int32 device tensor holding every query's `query_len` ids then its
        `query_len` mask values, and the context runs of NativePairTokenizer.prepare_contexts_compact; `desc`: host int32
        [N, 3] (query offset, context offset, m); `order` / `seg_n` / `seg_len`: the packed order and segment table;
        `padded_len`: the padded joint length (max_decoder_source_length); `special_ids`: the tokenizer's (cls, sep, pad).
        Row of a pair: q_ids | the first padded_len - query_len entries of t[0:m] [SEP] [PAD]..., mask q_mask | 1 | 0, cut to its
        segment.  A descriptor outside the pool or longer than its segment, or a segment table rr_forward_joint_packed would
        refuse, raises ValueError before anything is written."""
        import numpy as np
        dev = self.device
        if pool.dtype != torch.int32 or pool.device != dev or not pool.is_contiguous():
            raise ValueError("pool must be a contiguous int32 tensor on the model device")
        desc = np.ascontiguousarray(desc, dtype=np.int32)
        order = np.ascontiguousarray(order, dtype=np.int32).reshape(-1)
        if desc.ndim != 2 or desc.shape[1] != 3 or desc.shape[0] != order.shape[0]:
            raise ValueError("desc must be [N, 3] with one order entry per pair")
        rows = sum(int(n) * int(l) for n, l in zip(seg_n, seg_len))
        ids, am = (torch.empty(rows, dtype=torch.int64, device=dev) for _ in range(2))
        _, sep_id, pad_id = (int(x) for x in special_ids)
        rc = self.lib.rr_assemble_joint(self.h, L.ptr(pool), pool.numel(), desc.ctypes.data, desc.shape[0], order.ctypes.data,
                                        len(seg_n), (C.c_int32 * len(seg_n))(*seg_n), (C.c_int32 * len(seg_n))(*seg_len),
                                        int(query_len), int(padded_len), sep_id, pad_id, L.ptr(ids), L.ptr(am), self._stream())
        if rc == L.RR_ERR_BAD_SHAPE:        # a bad descriptor is a bad argument of this call, not an expanded-batch mismatch
            raise ValueError(f"rr_assemble_joint: {self.lib.rr_last_error(self.h).decode()}")
        L.check(rc, self.h, "rr_assemble_joint")
        return ids, am

    def forward_joint_tokens_packed(self, pool: torch.Tensor, desc, Bq: int, K: int, query_len: int, image_cls: torch.Tensor,
                                    image_patches: torch.Tensor, instruction_token_id: Optional[int] = None, granule: int = 16,
                                    segment_cost_rows: int = 0, want_scores: bool = False, want_order: bool = False,
                                    want_loss: bool = True, padded_len: int = 512, special_ids: Sequence[int] = (101, 102, 0),
                                    list_sizes: Optional[Sequence[int]] = None):
        """forward_joint_packed from COMPACT tokens (see assemble_joint): the pool on the device, the descriptors on the host,
        the joint rows assembled on the device where forward_joint_packed packs padded rows with pack_rows.  `image_cls` /
        `image_patches` are PER QUERY ([Bq, ...]: the ViT runs once per query) and expanded per pair in packed order on the
        device.  A pair's length is query_len + min(m + 1, padded_len - query_len), what forward_joint_packed derives from the
        padded rows, so the grouping, the rows and the logits are those of forward_joint_packed on the same inputs, bit for
        bit.  The head is rr_head_joint (loss_fn(logits, logits), rerank_model.py:328).  Returns the dict of
        forward_joint_packed."""
        import numpy as np
        if image_cls is None or image_patches is None:
            raise NotImplementedError("text_only is not implemented for this model")        # rerank_model.py:184-185
        desc = np.ascontiguousarray(desc, dtype=np.int32)
        N, ql, S = (Bq * K if list_sizes is None else int(sum(list_sizes))), int(query_len), int(padded_len)
        assert desc.shape == (N, 3), f"expanded batch {Bq}*{K} != {desc.shape[0]}"
        Bq, K, pair_query = self._layout(N, Bq, K, list_sizes, None)
        if image_cls.shape[0] != Bq or image_patches.shape[0] != Bq:
            raise AssertionError("image features must be per query: [Bq, ...]")
        lengths = ql + np.minimum(desc[:, 2].astype(np.int64) + 1, S - ql)
        floor = max(ql + 1, min(S, int(self.arch.get("cross_attn_len", 32))))
        f32 = dict(device=self.device, dtype=torch.float32)
        instr = -1 if instruction_token_id is None else int(instruction_token_id)

        def launch(order, seg_n, seg_len, sn, sl, lp, lp2, order_h):
            ids_p, am_p = self.assemble_joint(pool, desc, order_h, seg_n, seg_len, ql, S, special_ids)
            q = pair_query(order)                                     # image features per pair: a segment mixes queries
            cls_p = image_cls.to(**f32).index_select(0, q).contiguous()
            pat_p = image_patches.to(**f32).index_select(0, q).contiguous()
            L.check(self.lib.rr_forward_joint_packed(self.h, L.ptr(ids_p), L.ptr(am_p), L.ptr(cls_p), L.ptr(pat_p), None, 1.0,
                                                     len(seg_n), sn, sl, S, ql, instr, L.ptr(lp), L.ptr(lp2), self._stream()),
                    self.h, "rr_forward_joint_packed")
        return self._packed(launch, (), lengths, S, floor, granule, segment_cost_rows, Bq, K, None, want_loss, want_scores,
                            want_order, joint=True, host_order=True, list_sizes=list_sizes, n_pairs=N)

    def activation_range_exceeded(self, reset: bool = True) -> bool:
        """True when, since the last reset, a pre-LayerNorm residual row came within a factor 2 of the fp16 range (or was
        not finite) — rr_activation_range_flag; synchronises the current stream, so call it once per batch group, not per
        forward.  The remedy is an engine with compute_dtype="bf16" (DESIGN.md "Numerics")."""
        flag = C.c_int(0)
        L.check(self.lib.rr_activation_range_flag(self.h, int(reset), C.byref(flag), torch.cuda.current_stream(self.device).cuda_stream),
                self.h, "rr_activation_range_flag")
        return flag.value != 0

    def encode_image(self, pixel_values: torch.Tensor):
        """CLIP vision tower (rr_encode_image): pixel_values [B,3,IS,IS] -> (last_hidden_state[:,0] [B,Vh],
        hidden_states[-2][:,1:] [B,np,Vh]) — what rerank_model.py:408-411,424-426 takes from context_vision_encoder."""
        a, dev = self.arch, self.device
        IS = int(a.get("vit_image_size", 224))
        if pixel_values.dim() == 5:                                   # [B,1,3,H,W] as the datasets deliver it
            pixel_values = pixel_values.reshape(-1, *pixel_values.shape[2:])
        if tuple(pixel_values.shape[1:]) != (3, IS, IS):
            raise AssertionError(f"pixel_values must be [B,3,{IS},{IS}], got {tuple(pixel_values.shape)}")
        px = pixel_values.to(device=dev, dtype=torch.float32).contiguous()
        B = px.shape[0]
        cls = torch.empty((B, a["vision_hidden"]), dtype=torch.float32, device=dev)
        patches = torch.empty((B, a["n_patches"], a["vision_hidden"]), dtype=torch.float32, device=dev)
        L.check(self.lib.rr_encode_image(self.h, L.ptr(px), B, L.ptr(cls), L.ptr(patches),
                                         torch.cuda.current_stream(dev).cuda_stream), self.h, "rr_encode_image")
        return cls, patches

    def forward_joint(self, joint_input_ids: torch.Tensor, joint_attention_mask: torch.Tensor, Bq: int, K: int,
                      query_len: int, image_cls: torch.Tensor, image_patches: torch.Tensor,
                      instruction_token_id: Optional[int] = None, want_scores: bool = False, want_order: bool = False,
                      pair_range: Optional[Sequence[int]] = None, want_loss: bool = True,
                      preflmr_scores: Optional[torch.Tensor] = None, fusion_multiplier: float = 1.0,
                      retriever_query_li: Optional[torch.Tensor] = None, retriever_context_li: Optional[torch.Tensor] = None,
                      retriever_context_mask: Optional[torch.Tensor] = None):
        """RerankModel.forward semantics on the assembled joint sequence (see rr_forward_joint); `preflmr_scores`
        [N, S, query_len + image tokens] switches the PreFLMR attention fusion on (rr_forward_joint_fusion).  In its place the
        retriever's embeddings `retriever_query_li` [Bq, query_len + image tokens, D], `retriever_context_li` [N, S, D] and
        `retriever_context_mask` [N, S] may be given: the scores are then computed on the device (li_scores)."""
        dev = self.device
        N, S = joint_input_ids.shape
        assert N == Bq * K
        preflmr_scores = self._retriever_scores(preflmr_scores, retriever_query_li, retriever_context_li, retriever_context_mask,
                                                Bq, K, pair_range)
        f32 = dict(device=dev, dtype=torch.float32)
        cls = patches = None
        if image_cls is not None:
            cls, patches = image_cls.to(**f32).contiguous(), image_patches.to(**f32).contiguous()
        pb, pe, out = self._outputs(Bq, K, pair_range, want_loss, want_scores, want_order)
        stream = self._stream()
        instr = -1 if instruction_token_id is None else int(instruction_token_id)
        ids, am = L.ptr(joint_input_ids.contiguous()), L.ptr(joint_attention_mask.contiguous())
        if preflmr_scores is not None:
            P = self.arch["prefix_len"] + self.arch["n_patches"]
            ps = preflmr_scores.to(**f32).contiguous()
            if tuple(ps.shape) != (N, S, int(query_len) + P):                                   # rerank_model.py:280-284
                raise AssertionError(f"preflmr_scores must be [{N}, {S}, {int(query_len) + P}], got {tuple(ps.shape)}")
            L.check(self.lib.rr_forward_joint_fusion(self.h, ids, am, L.ptr(cls), L.ptr(patches), L.ptr(ps), float(fusion_multiplier),
                                                     Bq, K, S, int(query_len), instr, pb, pe, *_ptrs(out), stream),
                    self.h, "rr_forward_joint_fusion")
        else:
            L.check(self.lib.rr_forward_joint(self.h, ids, am, L.ptr(cls), L.ptr(patches), Bq, K, S, int(query_len), instr, pb, pe,
                                              *_ptrs(out), stream), self.h, "rr_forward_joint")
        return out

    def forward_interaction(self, query_li: torch.Tensor, context_li: torch.Tensor, query_mask: torch.Tensor,
                            context_mask: torch.Tensor, Bq: int, K: int, labels: Optional[torch.Tensor] = None,
                            want_scores: bool = False, want_order: bool = False,
                            pair_range: Optional[Sequence[int]] = None, want_loss: bool = True,
                            preflmr_scores: Optional[torch.Tensor] = None, fusion_multiplier: float = 1.0,
                            fusion_from_li: bool = False, want_maxsim: bool = False):
        """Interaction rerankers: late-interaction tensors [Bq,Lq,D] / [N,Lc,D] and 0/1 masks [Bq,Lq] / [N,Lc];
        `preflmr_scores` [N, Lc, Lq] switches the attention fusion on (rr_forward_interaction_fusion).  `fusion_from_li`: the
        fusion scores are the retriever's own, computed inside the call from query_li / context_li / context_mask
        (rr_forward_interaction_fusion_li; flmr_utils.py:22-48), `want_maxsim` adds the retriever's score of every pair of the
        slice as `maxsim` [N]."""
        if fusion_from_li and preflmr_scores is not None:
            raise ValueError("fusion_from_li=True computes the scores itself: do not pass preflmr_scores as well")
        if want_maxsim and not fusion_from_li:
            raise ValueError("want_maxsim needs fusion_from_li=True (or call li_scores)")
        dev = self.device
        N = context_li.shape[0]
        assert N == Bq * K and query_li.shape[0] == Bq, \
            f"{tuple(query_li.shape)}, {tuple(context_li.shape)}, {K - 1}"        # interaction_rerank_model.py:123
        Lq, Lc = query_li.shape[1], context_li.shape[1]
        f32 = dict(device=dev, dtype=torch.float32)
        query_li, context_li = query_li.to(**f32).contiguous(), context_li.to(**f32).contiguous()
        query_mask = query_mask.reshape(Bq, Lq).to(**f32).contiguous()
        context_mask = context_mask.reshape(N, Lc).to(**f32).contiguous()
        if labels is not None:
            assert labels.numel() == N
            labels = labels.to(**f32).contiguous()
        pb, pe, out = self._outputs(Bq, K, pair_range, want_loss, want_scores, want_order)
        stream = self._stream()
        tensors = L.ptr(query_li), L.ptr(context_li), L.ptr(query_mask), L.ptr(context_mask)
        if fusion_from_li:
            maxsim = torch.empty(N, **f32) if want_maxsim else None
            L.check(self.lib.rr_forward_interaction_fusion_li(self.h, *tensors, float(fusion_multiplier), Bq, K, Lq, Lc,
                                                              L.ptr(labels), pb, pe, *_ptrs(out), L.ptr(maxsim), stream),
                    self.h, "rr_forward_interaction_fusion_li")
            if want_maxsim:
                out["maxsim"] = maxsim
        elif preflmr_scores is not None:
            ps = preflmr_scores.to(**f32).contiguous()
            if tuple(ps.shape) != (N, Lc, Lq):
                raise AssertionError(f"preflmr_scores must be [{N}, {Lc}, {Lq}], got {tuple(ps.shape)}")
            L.check(self.lib.rr_forward_interaction_fusion(self.h, *tensors, L.ptr(ps), float(fusion_multiplier), Bq, K, Lq, Lc,
                                                           L.ptr(labels), pb, pe, *_ptrs(out), stream),
                    self.h, "rr_forward_interaction_fusion")
        else:
            L.check(self.lib.rr_forward_interaction(self.h, *tensors, Bq, K, Lq, Lc, L.ptr(labels), pb, pe, *_ptrs(out), stream),
                    self.h, "rr_forward_interaction")
        return out

    def forward_joint_packed(self, joint_input_ids: torch.Tensor, joint_attention_mask: torch.Tensor, Bq: int, K: int,
                             query_len: int, image_cls: torch.Tensor, image_patches: torch.Tensor,
                             instruction_token_id: Optional[int] = None, want_scores: bool = False, want_order: bool = False,
                             want_loss: bool = True, preflmr_scores: Optional[torch.Tensor] = None,
                             fusion_multiplier: float = 1.0, granule: int = 16, lengths: Optional[Sequence[int]] = None,
                             segment_cost_rows: int = 0, list_sizes: Optional[Sequence[int]] = None, pair_lists=None,
                             retriever_query_li: Optional[torch.Tensor] = None,
                             retriever_context_li: Optional[torch.Tensor] = None,
                             retriever_context_mask: Optional[torch.Tensor] = None):
        """`forward_joint` over PACKED rows (rr_forward_joint_packed): the pairs are grouped by the length of their joint
        sequence (1 + last non-pad position of the joint ids / mask) rounded up to `granule`, at least query_len + 1 and the
        mapping network's cross-attention window, and laid out group after group, so that the text encoder and the cross
        encoder compute only the rows that exist.  `preflmr_scores` [N, S, query_len + image tokens] as forward_joint takes
        it; its context rows go over padded (the reference normalises over the padded context axis).  The head runs on the
        scattered logits (rr_head_joint: the reference's loss_fn(logits, logits), rerank_model.py:328).  `lengths`: the pairs'
        joint lengths as the host knows them (no device -> host copy).  The sharded path and pair_range slices are not
        packed.  `retriever_query_li` / `retriever_context_li` / `retriever_context_mask` in place of `preflmr_scores`, as
        forward_joint takes them (one query row per list with `list_sizes`).  Returns the dict of forward_joint plus
        `packed_rows`, `packed_segments`."""
        dev = self.device
        N, S = joint_input_ids.shape
        Bq, K, pair_query = self._layout(N, Bq, K, list_sizes, pair_lists)
        preflmr_scores = self._retriever_scores(preflmr_scores, retriever_query_li, retriever_context_li, retriever_context_mask,
                                                Bq, K, None, pair_query=pair_query, N=N)
        if image_cls is None or image_patches is None:
            raise NotImplementedError("text_only is not implemented for this model")        # rerank_model.py:184-185
        ql = int(query_len)
        f32 = dict(device=dev, dtype=torch.float32)
        ids, am = joint_input_ids.to(dev).contiguous(), joint_attention_mask.to(dev).contiguous()
        floor = max(ql + 1, min(S, int(self.arch.get("cross_attn_len", 32))))
        if preflmr_scores is not None:
            P = self.arch["prefix_len"] + self.arch["n_patches"]
            if tuple(preflmr_scores.shape) != (N, S, ql + P):                                  # rerank_model.py:280-284
                raise AssertionError(f"preflmr_scores must be [{N}, {S}, {ql + P}], got {tuple(preflmr_scores.shape)}")
        instr = -1 if instruction_token_id is None else int(instruction_token_id)

        def launch(order, seg_n, seg_len, sn, sl, lp, lp2):
            ids_p, am_p = pack_rows(ids, order, seg_n, seg_len), pack_rows(am, order, seg_n, seg_len)
            q = pair_query(order)                                     # image features per pair: a segment mixes queries
            cls_p = image_cls.to(**f32).index_select(0, q).contiguous()
            pat_p = image_patches.to(**f32).index_select(0, q).contiguous()
            ps = None if preflmr_scores is None else pack_fusion_scores(preflmr_scores.to(**f32), order, 2, S - ql)
            L.check(self.lib.rr_forward_joint_packed(self.h, L.ptr(ids_p), L.ptr(am_p), L.ptr(cls_p), L.ptr(pat_p), L.ptr(ps),
                                                     float(fusion_multiplier), len(seg_n), sn, sl, S, ql, instr, L.ptr(lp),
                                                     L.ptr(lp2), self._stream()), self.h, "rr_forward_joint_packed")
        return self._packed(launch, (ids, am), lengths, S, floor, granule, segment_cost_rows, Bq, K, None, want_loss, want_scores,
                            want_order, joint=True, list_sizes=list_sizes, pair_lists=pair_lists, n_pairs=N)

    def forward_interaction_packed(self, query_li: torch.Tensor, context_li: torch.Tensor, query_mask: torch.Tensor,
                                   context_mask: torch.Tensor, Bq: int, K: int, labels: Optional[torch.Tensor] = None,
                                   want_scores: bool = False, want_order: bool = False, want_loss: bool = True,
                                   preflmr_scores: Optional[torch.Tensor] = None, fusion_multiplier: float = 1.0,
                                   granule: int = 16, lengths: Optional[Sequence[int]] = None, segment_cost_rows: int = 0,
                                   list_sizes: Optional[Sequence[int]] = None, pair_lists=None,
                                   fusion_from_li: bool = False, want_maxsim: bool = False):
        """`forward_interaction` over PACKED rows (rr_forward_interaction_packed, NORMAL and MORES): the pairs are grouped by
        their context length (1 + last non-zero position of `context_mask`) rounded up to `granule`; NORMAL computes the
        cross-encoder rows [query | context] that exist, MORES the doc-side rows.  `preflmr_scores` [N, Lc, Lq] goes over
        padded along the context axis (the reference's normalisers run over it).  `lengths`: the context lengths as the host
        knows them (no device -> host copy).  The sharded path and pair_range slices are not packed.  Returns the dict of
        forward_interaction plus `packed_rows` (context rows computed), `packed_segments`.  `fusion_from_li` / `want_maxsim` as
        forward_interaction takes them (rr_forward_interaction_packed_fusion_li): nothing padded goes over, the positions beyond
        a pair's segment count as masked rows of the score matrix."""
        if fusion_from_li and preflmr_scores is not None:
            raise ValueError("fusion_from_li=True computes the scores itself: do not pass preflmr_scores as well")
        if want_maxsim and not fusion_from_li:
            raise ValueError("want_maxsim needs fusion_from_li=True (or call li_scores)")
        dev = self.device
        N = context_li.shape[0]
        if list_sizes is None and pair_lists is None:
            assert N == Bq * K and query_li.shape[0] == Bq, \
                f"{tuple(query_li.shape)}, {tuple(context_li.shape)}, {K - 1}"        # interaction_rerank_model.py:123
        Bq, K, pair_query = self._layout(N, Bq, K, list_sizes, pair_lists)
        if list_sizes is not None:
            assert query_li.shape[0] == Bq, f"{tuple(query_li.shape)}: one query per list, {Bq} lists"
        Lq, Lc = query_li.shape[1], context_li.shape[1]
        f32 = dict(device=dev, dtype=torch.float32)
        cm = context_mask.reshape(N, Lc).to(**f32).contiguous()
        if preflmr_scores is not None and tuple(preflmr_scores.shape) != (N, Lc, Lq):
            raise AssertionError(f"preflmr_scores must be [{N}, {Lc}, {Lq}], got {tuple(preflmr_scores.shape)}")

        extra = {}

        def launch(order, seg_n, seg_len, sn, sl, lp, lp2):
            q = pair_query(order)                                     # query tensors per pair
            q_p = query_li.to(**f32).index_select(0, q).contiguous()
            qm_p = query_mask.reshape(-1, Lq).to(**f32).index_select(0, q).contiguous()
            c_p = pack_rows(context_li.to(**f32), order, seg_n, seg_len)
            cm_p = pack_rows(cm, order, seg_n, seg_len)
            if fusion_from_li:
                mp = torch.empty(N, **f32) if want_maxsim else None
                L.check(self.lib.rr_forward_interaction_packed_fusion_li(self.h, L.ptr(q_p), L.ptr(c_p), L.ptr(qm_p), L.ptr(cm_p),
                                                                         float(fusion_multiplier), len(seg_n), sn, sl, Lc, Lq,
                                                                         L.ptr(lp), L.ptr(lp2), L.ptr(mp), self._stream()),
                        self.h, "rr_forward_interaction_packed_fusion_li")
                if want_maxsim:
                    extra["maxsim"] = scatter_packed(mp, order)
                return
            ps = None if preflmr_scores is None else pack_fusion_scores(preflmr_scores.to(**f32), order)
            L.check(self.lib.rr_forward_interaction_packed(self.h, L.ptr(q_p), L.ptr(c_p), L.ptr(qm_p), L.ptr(cm_p), L.ptr(ps),
                                                           float(fusion_multiplier), len(seg_n), sn, sl, Lc, Lq, L.ptr(lp),
                                                           L.ptr(lp2), self._stream()), self.h, "rr_forward_interaction_packed")
        out = self._packed(launch, (cm,), lengths, Lc, 1, granule, segment_cost_rows, Bq, K, labels, want_loss, want_scores,
                           want_order, list_sizes=list_sizes, pair_lists=pair_lists, n_pairs=N)
        out.update(extra)
        return out

    def create_bank(self, capacity_rows: int, max_passages: int, codec=None, centroids=None):
        """A device-resident passage-embedding bank (rr_bank_create; passage_bank.PassageBank) of `capacity_rows` token rows
        and at most `max_passages` passages on this engine's device with its li_dim.  It outlives the engine and serves every
        interaction engine of the device with the same li_dim (NORMAL and MORES).  `codec` (passage_bank.PlaidCodec): a
        compressed bank (rr_bank_create_plaid) that holds the residual codes of a ColBERTv2 / PLAID index and decodes them in the
        forward; filled with add_compressed / load_plaid_index, or, when the codec carries its bucket cutoffs (they are set on the
        bank here, rr_bank_set_plaid_cutoffs), from embeddings on the device with add_compress.  `centroids` ([C, li_dim], e.g.
        PlaidCodec.train(...).centroids; not with `codec`): an fp16 bank with a centroid table (PassageBank.set_centroids,
        rr_bank_set_centroids): it keeps the fp16 rows, every `add` assigns a centroid code per row on the device, and the pruned
        searches, the inverted file and the filters take it as they take a compressed bank."""
        from .passage_bank import PassageBank
        return PassageBank(self, capacity_rows, max_passages, codec, centroids=centroids)

    def forward_interaction_bank(self, bank, query_li: torch.Tensor, query_mask: torch.Tensor, passage_ids, Bq: int, K: int,
                                 labels: Optional[torch.Tensor] = None, list_sizes: Optional[Sequence[int]] = None,
                                 granule: int = 16, segment_cost_rows: int = 0, fusion_from_li: bool = False,
                                 fusion_multiplier: float = 1.0, want_maxsim: bool = False, want_scores: bool = False,
                                 want_order: bool = False, want_loss: bool = True, pair_range=None,
                                 padded_len: Optional[int] = None, plan: Optional[dict] = None):
        """`forward_interaction_packed` with the context side named by passage id and read from `bank`
        (rr_forward_interaction_bank, NORMAL and MORES): `query_li` [Bq, Lq, D] / `query_mask` [Bq, Lq] per query, `passage_ids`
        the N = Bq * K candidates in pair order (`list_sizes` in place of (Bq, K), both None then: lists of unequal length).  The
        context lengths come from the bank's host table, so nothing is copied from the device to group the pairs, nothing is
        uploaded or packed for the context side, and a passage may serve any number of pairs.  `padded_len`: the context length
        the padded call would use (the fusion normalisers, the attention schedule and NORMAL's position limit follow it);
        default: the longest Lc an `add` of the bank has seen.  `plan`: passage_bank.plan_bank_batch's result for this call,
        when the ids were looked up and grouped already (`passage_ids` is not read then).  An id the bank does not hold raises
        KeyError naming it.  Logits: bit for bit those of forward_interaction_packed on float32(bank rows) and the bank's masks;
        on an fp16 engine also those of the call on the original float32 tensors (include/rerank_mi355.h).  `pair_range` and
        sharded slices are not covered.  Returns the dict of forward_interaction_packed."""
        import numpy as np
        from .passage_bank import plan_bank_batch
        if pair_range is not None:
            raise ValueError("forward_interaction_bank does not take pair_range: the sharded path and slices are not packed")
        if want_maxsim and not fusion_from_li:
            raise ValueError("want_maxsim needs fusion_from_li=True (or call li_scores)")
        dev = self.device
        Lc = int(bank.padded_len if padded_len is None else padded_len)
        if plan is None:
            plan = plan_bank_batch(bank.table, passage_ids, K if list_sizes is None else None, list_sizes, Lc, granule,
                                   segment_cost_rows)
        N = int(plan["indices"].size)
        if list_sizes is None:
            assert N == Bq * K and query_li.shape[0] == Bq, f"{tuple(query_li.shape)}, {N} passages, {K - 1}"
        Bq, K, _ = self._layout(N, Bq, K, list_sizes, None)
        assert query_li.shape[0] == Bq, f"{tuple(query_li.shape)}: one query per list, {Bq} lists"
        Lq = query_li.shape[1]
        f32 = dict(device=dev, dtype=torch.float32)
        q = query_li.to(**f32).contiguous()
        qm = query_mask.reshape(Bq, Lq).to(**f32).contiguous()
        pp = np.ascontiguousarray(plan["pair_passage"], dtype=np.int32)
        pq = np.ascontiguousarray(plan["pair_query"], dtype=np.int32)
        extra = {}

        def launch(order, seg_n, seg_len, sn, sl, lp, lp2):
            mp = torch.empty(N, **f32) if want_maxsim else None
            L.check(self.lib.rr_forward_interaction_bank(self.h, bank.h, L.ptr(q), L.ptr(qm), Bq, Lq, pp.ctypes.data, pq.ctypes.data,
                                                         len(seg_n), sn, sl, Lc, int(bool(fusion_from_li)), float(fusion_multiplier),
                                                         L.ptr(lp), L.ptr(lp2), L.ptr(mp), self._stream()),
                    self.h, "rr_forward_interaction_bank")
            if want_maxsim:
                extra["maxsim"] = scatter_packed(mp, order)
        out = self._packed(launch, (), plan["lengths"], Lc, 1, granule, segment_cost_rows, Bq, K, labels, want_loss, want_scores,
                           want_order, list_sizes=list_sizes, n_pairs=N, grouping=(plan["order"], plan["seg_n"], plan["seg_len"]))
        out.update(extra)
        return out

    def bank_li_scores(self, bank, query_li: torch.Tensor, passage_ids, pair_query=None, K: Optional[int] = None,
                       list_sizes: Optional[Sequence[int]] = None, want_scores: bool = False, want_maxsim: bool = True,
                       padded_len: Optional[int] = None) -> dict:
        """`li_scores` with the context side named by passage id and read from `bank`, fp16 or compressed (rr_bank_li_scores;
        colbert_score, flmr_utils.py:22-48): `maxsim` [n_pairs] and, with `want_scores`, `scores` [n_pairs, padded_len, Lq]
        (-9999 on masked rows and beyond a passage's length), in exact float32, pair order.  `query_li` [n_queries, Lq, D];
        the query of pair i is `pair_query[i]`, or i // K, or given by `list_sizes` (pairs of query 0 first, then query 1, ...),
        as forward_interaction_bank lays pairs out; with none of the three and one query, every pair is that query's.
        `padded_len`: default the longest passage of the call.  NORMAL and MORES engines, weights loaded or not.  Bit for bit
        li_scores(K = 1) on float32(bank rows) and the bank's masks.  An id the bank does not hold raises KeyError naming it."""
        import numpy as np
        from .passage_bank import plan_bank_scores
        if not (want_scores or want_maxsim):
            raise ValueError("bank_li_scores: want_scores or want_maxsim")
        D = self.arch["li_dim"]
        assert query_li.dim() == 3 and query_li.shape[2] == D, f"query_li {tuple(query_li.shape)}: [n_queries, Lq, {D}]"
        nq, Lq = int(query_li.shape[0]), int(query_li.shape[1])
        if pair_query is None and K is None and list_sizes is None:
            assert nq == 1, "bank_li_scores: pair_query, K or list_sizes says which query a pair belongs to"
            K = len(passage_ids)
        plan = plan_bank_scores(bank.table, passage_ids, nq, pair_query, K, list_sizes, padded_len)
        N, Lc = int(plan["indices"].size), plan["padded_len"]
        f32 = dict(device=self.device, dtype=torch.float32)
        q = query_li.to(**f32).contiguous()
        pp = np.ascontiguousarray(plan["pair_passage"], dtype=np.int32)
        pq = np.ascontiguousarray(plan["pair_query"], dtype=np.int32)
        out = dict(scores=torch.empty((N, Lc, Lq), **f32) if want_scores else None,
                   maxsim=torch.empty(N, **f32) if want_maxsim else None)
        L.check(self.lib.rr_bank_li_scores(self.h, bank.h, L.ptr(q), nq, Lq, pp.ctypes.data, pq.ctypes.data, N, Lc,
                                           L.ptr(out["scores"]), L.ptr(out["maxsim"]), self._stream()), self.h, "rr_bank_li_scores")
        return {k: v for k, v in out.items() if v is not None}

    def bank_search(self, bank, query_li: torch.Tensor, k: int, first: int = 0, count: Optional[int] = None) -> dict:
        """Exact top-k MaxSim search over `bank`, fp16 or compressed (rr_bank_search): every passage of the dense index range
        [first, first + count) (`count` None: through the last passage) is scored against every query of `query_li`
        [n_queries, Lq, D] with the retriever's MaxSim (colbert_score, flmr_utils.py:22-48; bit for bit the `maxsim` of
        bank_li_scores), and per query the k best are returned in the order of torch.sort(descending=True, stable=True):
        {"indices": int32 [n_queries, k] dense bank indices, "scores": float32 [n_queries, k]}, both on the device.
        1 <= k <= min(count, 1024) (ValueError / NotImplementedError).  NORMAL and MORES engines, weights loaded or not."""
        first, n, nq, Lq, q = _bank_search_args(self, "bank_search", bank, query_li, first, count)
        k = int(k)
        if k < 1 or k > n:
            raise ValueError(f"bank_search: k = {k} of {n} passages")
        if k > 1024:
            raise NotImplementedError(f"bank_search: k = {k} (at most 1024)")
        out = dict(indices=torch.empty((nq, k), device=self.device, dtype=torch.int32),
                   scores=torch.empty((nq, k), device=self.device, dtype=torch.float32))
        L.check(self.lib.rr_bank_search(self.h, bank.h, L.ptr(q), nq, Lq, first, n, k, L.ptr(out["indices"]), L.ptr(out["scores"]),
                                        self._stream()), self.h, "rr_bank_search")
        return out

    def bank_search_f16(self, bank, query_li: torch.Tensor, k: int, ndocs: int, slack: Optional[float] = None, first: int = 0,
                        count: Optional[int] = None) -> dict:
        """Exhaustive search of an fp16 `bank` (plain or coded) whose first pass runs on the fp16 matrix core (rr_bank_search_f16):
        every passage of the range gets an approximate MaxSim, the `ndocs` approximately best per query are rescored exactly and
        the k best of those are returned: {"indices": int32 [n_queries, k], "scores": float32 [n_queries, k], each score bit for
        bit bank_search's for that passage, "certified": int32 [n_queries]}, on the device.  certified[q] = 1: the row is provably
        bank_search's, bytes included (include/rerank_mi355.h gives the proof); 0: still the exact best k of the query's ndocs
        approximately best.  `slack`: the bound on |approximate - exact| the certificate uses; None: the header's bound evaluated
        on `query_li` for unit rows (passage_bank.f16_default_slack: one small reduction on the device and one read-back).
        1 <= k <= min(ndocs, count), ndocs <= 1024; compressed banks: NotImplementedError (bank_search_f16_plaid takes them)."""
        from .passage_bank import F16Search
        first, n, nq, Lq, q = _bank_search_args(self, "bank_search_f16", bank, query_li, first, count)
        fast = F16Search(ndocs, slack)
        k = int(k)
        if k < 1 or k > n or k > fast.ndocs:
            raise ValueError(f"bank_search_f16: k = {k}, ndocs = {fast.ndocs}, {n} passages")
        if getattr(bank, "codec", None) is not None:
            raise NotImplementedError("bank_search_f16: a compressed bank (fp16 banks only)")
        out = dict(indices=torch.empty((nq, k), device=self.device, dtype=torch.int32),
                   scores=torch.empty((nq, k), device=self.device, dtype=torch.float32),
                   certified=torch.empty((nq,), device=self.device, dtype=torch.int32))
        L.check(self.lib.rr_bank_search_f16(self.h, bank.h, L.ptr(q), nq, Lq, first, n, fast.ndocs, k, fast.slack_for(q), L.ptr(out["indices"]),
                                            L.ptr(out["scores"]), L.ptr(out["certified"]), self._stream()), self.h, "rr_bank_search_f16")
        return out

    def bank_search_f16_plaid(self, bank, query_li: torch.Tensor, k: int, ndocs: int, slack: Optional[float] = None, first: int = 0,
                              count: Optional[int] = None) -> dict:
        """bank_search_f16 for a COMPRESSED `bank` (rr_bank_search_f16_plaid): the first pass decodes the rows it multiplies, once
        per block of queries, and feeds them to the fp16 matrix core.  The same arguments and the same dict, and byte for byte
        what bank_search_f16 returns on the fp16 bank that holds the bank's decoded rows (`PassageBank.read`), "certified"
        included; every score is bank_search's on the compressed bank, and a certified row is bank_search's row.  li_dim 64, 128
        or 256; an fp16 bank: NotImplementedError (bank_search_f16 is its entry)."""
        from .passage_bank import F16Search
        first, n, nq, Lq, q = _bank_search_args(self, "bank_search_f16_plaid", bank, query_li, first, count)
        fast = F16Search(ndocs, slack)
        k = int(k)
        if k < 1 or k > n or k > fast.ndocs:
            raise ValueError(f"bank_search_f16_plaid: k = {k}, ndocs = {fast.ndocs}, {n} passages")
        if getattr(bank, "codec", None) is None:
            raise NotImplementedError("bank_search_f16_plaid: an fp16 bank (compressed banks only; bank_search_f16 searches an fp16 bank)")
        out = dict(indices=torch.empty((nq, k), device=self.device, dtype=torch.int32),
                   scores=torch.empty((nq, k), device=self.device, dtype=torch.float32),
                   certified=torch.empty((nq,), device=self.device, dtype=torch.int32))
        L.check(self.lib.rr_bank_search_f16_plaid(self.h, bank.h, L.ptr(q), nq, Lq, first, n, fast.ndocs, k, fast.slack_for(q), L.ptr(out["indices"]),
                                                  L.ptr(out["scores"]), L.ptr(out["certified"]), self._stream()), self.h, "rr_bank_search_f16_plaid")
        return out

    def bank_search_filtered(self, bank, query_li: torch.Tensor, k: int, filter, first: int = 0, count: Optional[int] = None) -> dict:
        """bank_search over the passages of the range that `filter` (a BankFilter, PassageBank.filter: one set for every query,
        or one per query) allows (rr_bank_search_filtered): a passage outside the set is not scored.  {"indices": int32
        [n_queries, k] dense bank indices, -1 behind the count; "scores": float32 [n_queries, k], -inf there; "counts": int32
        [n_queries]}, on the device; k may exceed the number of allowed passages.  With every passage allowed: bank_search's
        result.  The selection still walks one score per passage of the range, however few the filter allows:
        bank_search_filtered_sparse returns the same bytes with every stage over the allowed passages alone
        (profiles/bank_search_sparse_bench.json.log says from which density on it is the faster one)."""
        return _bank_search_filtered(self, "bank_search_filtered", bank, query_li, k, filter, first, count)

    def bank_search_filtered_sparse(self, bank, query_li: torch.Tensor, k: int, filter, first: int = 0, count: Optional[int] = None) -> dict:
        """bank_search_filtered, list-driven (rr_bank_search_filtered_sparse): the same arguments, checks and result, byte for byte.
        The filter's rows are compacted into candidate lists on the device, the scoring workgroups walk those lists and the
        selection reads their counts, so the work of the call follows the passages the filter allows, not the range."""
        return _bank_search_filtered(self, "bank_search_filtered_sparse", bank, query_li, k, filter, first, count)

    def bank_search_plaid_filtered(self, bank, query_li: torch.Tensor, k: int, filter, **kw) -> dict:
        """bank_search_plaid with the candidates restricted to what `filter` (a BankFilter) allows (rr_bank_search_plaid_filtered):
        the result of bank_search_plaid on a bank whose filtered-out passages are fully masked.  The arguments and the outputs of
        bank_search_plaid."""
        return _bank_search_plaid(self, "rr_bank_search_plaid_filtered", bank, query_li, k, filter=filter, **kw)

    def bank_search_plaid_ivf_filtered(self, bank, query_li: torch.Tensor, k: int, filter, **kw) -> dict:
        """bank_search_plaid_filtered with the candidates from the bank's inverted file (rr_bank_search_plaid_ivf_filtered): bit
        for bit the same result."""
        return _bank_search_plaid(self, "rr_bank_search_plaid_ivf_filtered", bank, query_li, k, filter=filter, **kw)

    def bank_build_ivf(self, bank) -> dict:
        """Build, or rebuild, the inverted file of a COMPRESSED `bank` (or an fp16 one with a centroid table) over every passage it holds now (rr_bank_build_ivf; per
        centroid the sorted unique passages with an unmasked token of that code, the reference's ivf.pid.pt).  A load-time call
        on this engine's current stream: it allocates and synchronises.  Returns bank.ivf_info()."""
        return bank.build_ivf()

    def bank_extend_ivf(self, bank) -> dict:
        """Take the inverted file of a COMPRESSED `bank` over the passages added since it was built (rr_bank_extend_ivf): the bytes
        of a fresh bank_build_ivf, from a walk of the new passages alone.  Nothing happens when the file covers the bank; without a
        file it is bank_build_ivf.  A load-time call on this engine's current stream.  Returns bank.ivf_info()."""
        return bank.extend_ivf()

    def bank_export_plaid(self, bank, first: int = 0, count: Optional[int] = None):
        """A range of a COMPRESSED `bank` as an index stores it, on the device (rr_bank_export_plaid): (codes int32 [R], residuals
        uint8 [R, li_dim * nbits / 8], doclens list), the unmasked rows of every passage back to back: bank.export_compressed.  A
        save-time call on this engine's current stream: it synchronises."""
        return bank.export_compressed(first, count)

    def bank_load_ivf(self, bank, path_or_pair, verify: bool = True) -> dict:
        """Take the inverted file of a COMPRESSED `bank` from an ivf.pid.pt (a path, or the pair it holds) instead of building it
        (rr_bank_load_ivf), verified against a fresh build unless verify=False: bank.load_ivf.  Returns bank.ivf_info()."""
        return bank.load_ivf(path_or_pair, verify=verify)

    def bank_search_plaid_ivf(self, bank, query_li: torch.Tensor, k: int, **kw) -> dict:
        """bank_search_plaid with the candidates taken from the bank's inverted file (rr_bank_search_plaid_ivf): the same
        arguments, the same checks and bit for bit the same result; the work of a query follows the lists of its cells, not the
        rows of the range.  NotImplementedError when the bank has no file or the range reaches beyond the passages it covers
        (bank_build_ivf)."""
        return _bank_search_plaid(self, "rr_bank_search_plaid_ivf", bank, query_li, k, **kw)

    def bank_search_plaid(self, bank, query_li: torch.Tensor, k: int, *, ncells: int, centroid_score_threshold: float, ndocs: int,
                          coarse_tokens: Optional[int] = None, first: int = 0, count: Optional[int] = None) -> dict:
        """PLAID's pruned top-k search over a COMPRESSED `bank`, or an fp16 one with a centroid table (rr_bank_search_plaid; the reference's
        colbert/search/index_storage.py:86-184): per query the cells of the first `coarse_tokens` query tokens (None: all) give
        the candidates, two centroid-only passes keep `ndocs` and then ndocs // 4 of them, and the survivors get the exact MaxSim
        of bank_search.  {"indices": int32 [n_queries, k] dense bank indices, -1 behind the count; "scores": float32
        [n_queries, k], -inf there; "counts": int32 [n_queries]}, on the device.  1 <= ncells <= min(centroids, 16),
        4 <= ndocs <= 1024, 1 <= k <= min(ndocs // 4, count) (ValueError / NotImplementedError before the library)."""
        return _bank_search_plaid(self, "rr_bank_search_plaid", bank, query_li, k, ncells=ncells, centroid_score_threshold=centroid_score_threshold,
                                  ndocs=ndocs, coarse_tokens=coarse_tokens, first=first, count=count)

    def bank_merge_topk(self, indices: torch.Tensor, scores: torch.Tensor, counts: Optional[torch.Tensor], part_offsets, k: int, *,
                        part_stride: Optional[int] = None, count_stride: Optional[int] = None, want_parts: bool = False) -> dict:
        """The k-lists of P parts merged into one list over global indices (rr_bank_merge_topk, "THE MERGED LIST" in
        include/rerank_mi355.h): `indices` int32 / `scores` float32 [P, n_queries, k_in] of LOCAL indices per part, `counts` int32
        [P, n_queries] or None (every list is full), all on this engine's device; `part_offsets` the P + 1 host offsets of the
        parts in the global index space.  With `part_stride` / `count_stride` (in 4-byte words) the three tensors may be views
        into one gathered block whose parts lie further apart than their lists: only their first element's address and their
        shapes are read then.  Per query the first k real entries in the one rank order of the searches over (score, global
        index): {"indices": int32 [n_queries, k] global, -1 behind the count; "scores": float32 [n_queries, k], -inf there;
        "counts": int32 [n_queries]; with `want_parts` "parts": int32 [n_queries, k], the part an entry came from}.  Merging the
        bank_search results of the parts of a corpus gives, byte for byte, bank_search over the whole corpus.  1 <= k <= k_in,
        P <= 64, P * k_in <= 8192 (AssertionError / NotImplementedError from the library)."""
        import numpy as np
        if indices.dim() != 3 or scores.shape != indices.shape:
            raise ValueError(f"bank_merge_topk: indices {tuple(indices.shape)} and scores {tuple(scores.shape)}: both [parts, n_queries, k_in]")
        if indices.dtype != torch.int32 or scores.dtype != torch.float32 or (counts is not None and counts.dtype != torch.int32):
            raise ValueError("bank_merge_topk: indices and counts are int32, scores float32")
        P, nq, k_in = (int(x) for x in indices.shape)
        if counts is not None and tuple(counts.shape) != (P, nq):
            raise ValueError(f"bank_merge_topk: counts {tuple(counts.shape)}: [{P}, {nq}]")
        for t in (indices, scores, counts):
            if t is not None and t.device != self.device:
                raise ValueError(f"bank_merge_topk: a tensor on {t.device}, the engine on {self.device}")
        off = np.ascontiguousarray(np.asarray(part_offsets, dtype=np.int64).reshape(-1))
        if off.size != P + 1 or (off.size and (off.min() < -(1 << 31) or off.max() >= (1 << 31))):
            raise ValueError(f"bank_merge_topk: part_offsets holds {off.size} int32 offsets for {P} parts ({P + 1})")
        off = off.astype(np.int32)
        if part_stride is None:
            indices, scores = indices.contiguous(), scores.contiguous()
            part_stride = nq * k_in
        if count_stride is None:
            counts = None if counts is None else counts.contiguous()
            count_stride = nq
        k = int(k)
        if k < 1 or k > k_in:
            raise AssertionError(f"bank_merge_topk: k = {k} of lists of {k_in}")
        out = dict(indices=torch.empty((nq, k), device=self.device, dtype=torch.int32),
                   scores=torch.empty((nq, k), device=self.device, dtype=torch.float32),
                   counts=torch.empty((nq,), device=self.device, dtype=torch.int32),
                   parts=torch.empty((nq, k), device=self.device, dtype=torch.int32) if want_parts else None)
        L.check(self.lib.rr_bank_merge_topk(self.h, indices.data_ptr(), scores.data_ptr(), 0 if counts is None else counts.data_ptr(),
                                            int(part_stride), int(count_stride), P, off.ctypes.data, nq, k_in, k, L.ptr(out["indices"]),
                                            L.ptr(out["scores"]), L.ptr(out["counts"]), L.ptr(out["parts"]), self._stream()),
                self.h, "rr_bank_merge_topk")
        return {n: v for n, v in out.items() if v is not None}

    def bank_search_plaid_tap(self, name: str):
        """One intermediate of this engine's last bank_search_plaid call as a numpy array (rr_bank_search_plaid_tap,
        include/rerank_mi355_diag.h): "S", "cells", "keep", "a1", "list1", "list2".  Flat; the caller knows the shape."""
        import numpy as np
        dt = {"S": np.float32, "a1": np.float32, "cells": np.uint8, "keep": np.uint8, "list1": np.int32, "list2": np.int32}[name]
        cap = 1 << 20
        while True:
            buf = np.empty(cap, dtype=np.uint8)
            got = int(self.lib.rr_bank_search_plaid_tap(self.h, name.encode(), buf.ctypes.data, cap))
            if got == L.RR_ERR_BAD_SHAPE and cap < (1 << 34):
                cap *= 8
                continue
            if got < 0:
                L.check(got, self.h, "rr_bank_search_plaid_tap")
            return buf[:got].view(dt).copy()

    def li_scores(self, query_li: torch.Tensor, context_li: torch.Tensor, context_mask: torch.Tensor, Bq: int, K: int,
                  pair_range: Optional[Sequence[int]] = None, want_scores: bool = True, want_maxsim: bool = True) -> dict:
        """The frozen retriever's score of every pair and the matrix behind it (rr_li_scores; colbert_score,
        flmr_utils.py:22-48) from query_li [Bq, Lq, D], context_li [N, Lc, D] and the 0/1 context_mask [N, Lc], N = Bq * K:
        `scores` [N, Lc, Lq] (context token x query token, -9999 on masked context rows: what the executor hands over as
        retrieval_results.scores_raw) and `maxsim` [N], in exact float32.  With `pair_range` only that slice of the outputs is
        written (the rest is uninitialised).  Engines of any model kind."""
        if not (want_scores or want_maxsim):
            raise ValueError("li_scores: want_scores or want_maxsim")
        N = context_li.shape[0]
        assert N == Bq * K and query_li.shape[0] == Bq, f"{tuple(query_li.shape)}, {tuple(context_li.shape)}, Bq={Bq} K={K}"
        Lq, Lc, D = query_li.shape[1], context_li.shape[1], self.arch["li_dim"]
        assert query_li.shape[2] == D and context_li.shape[2] == D, f"late-interaction dim {D}"
        f32 = dict(device=self.device, dtype=torch.float32)
        query_li, context_li = query_li.to(**f32).contiguous(), context_li.to(**f32).contiguous()
        context_mask = context_mask.reshape(N, Lc).to(**f32).contiguous()
        pb, pe = (0, N) if pair_range is None else (int(pair_range[0]), int(pair_range[1]))
        out = dict(scores=torch.empty((N, Lc, Lq), **f32) if want_scores else None,
                   maxsim=torch.empty(N, **f32) if want_maxsim else None)
        L.check(self.lib.rr_li_scores(self.h, L.ptr(query_li), L.ptr(context_li), L.ptr(context_mask), Bq, K, Lq, Lc, pb, pe,
                                      L.ptr(out["scores"]), L.ptr(out["maxsim"]), self._stream()), self.h, "rr_li_scores")
        return {k: v for k, v in out.items() if v is not None}

    def _retriever_scores(self, preflmr_scores, query_li, context_li, context_mask, Bq, K, pair_range, pair_query=None, N=None):
        """`preflmr_scores` of a joint forward: as given, or from the retriever's embeddings (li_scores).  With a list layout
        (K is None) the query rows are handed over per pair."""
        given = [t is not None for t in (query_li, context_li, context_mask)]
        if not any(given):
            return preflmr_scores
        if preflmr_scores is not None:
            raise ValueError("give preflmr_scores or the retriever_*_li tensors, not both")
        if not all(given):
            raise ValueError("retriever_query_li, retriever_context_li and retriever_context_mask go together")
        if K is None:
            q = pair_query(torch.arange(N, device=self.device))
            query_li, Bq, K = query_li.to(self.device).index_select(0, q), N, 1
        return self.li_scores(query_li, context_li, context_mask, Bq, K, pair_range, want_maxsim=False)["scores"]

    def head(self, logits: torch.Tensor, logits2: Optional[torch.Tensor], labels: Optional[torch.Tensor], Bq: int,
             K: int, want_scores: bool = False, want_order: bool = True, want_loss: bool = True, joint: bool = False):
        """Scoring head on complete logits (after the cross-rank all-gather).  `joint`: RerankModel's loss, the reference's
        loss_fn(logits, logits) (rr_head_joint, rerank_model.py:328; no labels)."""
        out = self._head_outputs(Bq, K, want_loss, want_scores, want_order)
        if joint:
            L.check(self.lib.rr_head_joint(self.h, L.ptr(logits), L.ptr(logits2), Bq, K, *_ptrs(out), self._stream()),
                    self.h, "rr_head_joint")
            return out
        if labels is not None:
            labels = labels.to(device=self.device, dtype=torch.float32).contiguous()
        L.check(self.lib.rr_head(self.h, L.ptr(logits), L.ptr(logits2), L.ptr(labels), Bq, K, *_ptrs(out), self._stream()),
                self.h, "rr_head")
        return out

    def head_lists(self, logits: torch.Tensor, logits2: Optional[torch.Tensor], labels: Optional[torch.Tensor],
                   list_sizes: Sequence[int], want_scores: bool = False, want_order: bool = True, want_loss: bool = True,
                   gather: Optional[torch.Tensor] = None, joint: bool = False):
        """The scoring head over lists of unequal length (rr_head_lists): list q holds list_sizes[q] >= 1 candidates (at most
        4096), the pairs stored list after list.  `logits` / `logits2` [N] on the device; `gather` (int32 [N] on the device):
        pair p's logits are read at logits[gather[p]], which lets a packed forward's logits be consumed in packed order;
        `labels` [N] in pair order (None: the first candidate of every list is the positive); `joint`: RerankModel's loss
        (rr_head_joint's).  Returns loss (scalar), list_loss [n_lists] (each list's own loss, what `head` gives for it alone),
        scores [N] and order [N] int32 (each list's descending stable rank, as indices local to the list), as wanted.  An empty
        list raises AssertionError, a list above 4096 NotImplementedError."""
        import numpy as np
        sizes = np.asarray(list_sizes, dtype=np.int64).reshape(-1)
        off = np.zeros(sizes.size + 1, dtype=np.int32)
        np.cumsum(sizes, out=off[1:])
        N, dev = int(sizes.sum()), self.device
        assert logits.numel() == N, f"{logits.numel()} logits for lists of {N} candidates"
        if labels is not None:
            labels = labels.to(device=dev, dtype=torch.float32).contiguous()
            assert labels.numel() == N
        if gather is not None:
            assert gather.dtype == torch.int32 and gather.numel() == N and gather.device == dev
        out = dict(loss=torch.empty((), dtype=torch.float32, device=dev) if want_loss else None,
                   list_loss=torch.empty(sizes.size, dtype=torch.float32, device=dev) if want_loss else None,
                   scores=torch.empty(N, dtype=torch.float32, device=dev) if want_scores else None,
                   order=torch.empty(N, dtype=torch.int32, device=dev) if want_order else None)
        L.check(self.lib.rr_head_lists(self.h, L.ptr(logits), L.ptr(logits2), None if joint else L.ptr(labels), int(sizes.size),
                                       off.ctypes.data, L.ptr(gather), int(joint),
                                       *[L.ptr(out[k]) for k in ("loss", "list_loss", "scores", "order")], self._stream()),
                self.h, "rr_head_lists")
        return out

    # ---- plumbing shared by the forwards
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _head_outputs(self, Bq: int, K: int, want_loss: bool, want_scores: bool, want_order: bool) -> dict:
        dev = self.device
        return dict(loss=torch.empty((), dtype=torch.float32, device=dev) if want_loss else None,
                    scores=torch.empty(Bq * K, dtype=torch.float32, device=dev) if want_scores else None,
                    order=torch.empty((Bq, K), dtype=torch.int32, device=dev) if want_order else None)

    def _outputs(self, Bq: int, K: int, pair_range, want_loss: bool, want_scores: bool, want_order: bool):
        """(pair_begin, pair_end, outputs) of a padded forward: logits / logits2 [N] always, loss / scores / order when the call
        covers every pair and they are wanted."""
        N = Bq * K
        pb, pe = (0, N) if pair_range is None else (int(pair_range[0]), int(pair_range[1]))
        full = pb == 0 and pe == N
        out = dict(logits=torch.empty(N, dtype=torch.float32, device=self.device),
                   logits2=torch.empty(N, dtype=torch.float32, device=self.device))
        out.update(self._head_outputs(Bq, K, full and want_loss, full and want_scores, full and want_order))
        return pb, pe, out

    def _layout(self, N: int, Bq, K, list_sizes, pair_lists):
        """(Bq, K, pair_query) of a packed forward.  Uniform: pair p belongs to query p // K.  `list_sizes`: lists of unequal
        length, pair p belongs to the list that holds it (K is None from here on).  `pair_lists` (sharded slices): the list
        index of each of the call's N pairs, given.  pair_query(order) is the device int64 query index of the pairs `order`."""
        if list_sizes is None and pair_lists is None:
            assert N == Bq * K
            return Bq, K, lambda order: torch.div(order, K, rounding_mode="floor")
        if pair_lists is None:
            sizes = torch.as_tensor(list_sizes, dtype=torch.int64).reshape(-1)
            assert sizes.numel() > 0 and int(sizes.min()) >= 1 and int(sizes.sum()) == N, \
                f"list_sizes {sizes.tolist()} do not partition {N} pairs into non-empty lists"
            pair_lists = torch.repeat_interleave(torch.arange(sizes.numel()), sizes)
        table = torch.as_tensor(pair_lists, dtype=torch.int64).reshape(-1).to(self.device, non_blocking=True)
        assert table.numel() == N, "one list index per pair"
        return (None if list_sizes is None else len(list_sizes)), None, lambda order: table.index_select(0, order.long())

    def _packed(self, launch, rows, lengths, padded_len: int, floor: int, granule: int, segment_cost_rows: int, Bq: int, K: int,
                labels, want_loss: bool, want_scores: bool, want_order: bool, joint: bool = False, host_order: bool = False,
                list_sizes=None, pair_lists=None, n_pairs: Optional[int] = None, grouping=None) -> dict:
        """What the packed forwards share: the pairs' lengths (`lengths` from the host, else derived from the [N, padded_len]
        tensors `rows` on the device: one device -> host copy) -> segments (group_pairs_by_length) -> the pair order on the
        device -> the ctypes segment tables -> `launch(order, seg_n, seg_len, seg_pairs, seg_lens, logits, logits2)` (with
        `host_order`, the host pair order as one more argument), which packs its inputs and makes the call -> the logits
        scattered back to pair order -> the scoring head over them.
        `list_sizes` in place of (Bq, K): lists of unequal length; the head is rr_head_lists over the PACKED logits with the
        packed order's inverse as its gather, and the result also holds `list_loss`; `order` is flat [N], local to each list.
        `pair_lists` without `list_sizes` (a rank's slice of a sharded batch): logits only, no head.
        `grouping`: (order, seg_pairs, seg_len) as group_pairs_by_length returned them for these lengths, when the caller has
        grouped already (passage_bank.plan_bank_batch, on another thread); nothing is derived then."""
        N = Bq * K if n_pairs is None else n_pairs
        assert granule > 0
        if labels is not None:
            assert labels.numel() == N
        if grouping is not None:
            order_h, seg_n, seg_len = grouping
        else:
            if lengths is None:
                lengths = pair_lengths(*rows).cpu().numpy()
            order_h, seg_n, seg_len = group_pairs_by_length(lengths, padded_len, granule, floor, segment_cost_rows)
        assert len(order_h) == N, "one length per pair"
        order = torch.from_numpy(order_h).to(self.device, non_blocking=True)
        lp, lp2 = (torch.empty(N, dtype=torch.float32, device=self.device) for _ in range(2))
        launch(order, seg_n, seg_len, (C.c_int32 * len(seg_n))(*seg_n), (C.c_int32 * len(seg_n))(*seg_len), lp, lp2,
               *((order_h,) if host_order else ()))
        logits, logits2 = scatter_packed(lp, order), scatter_packed(lp2, order)
        two = self.arch["loss_fn"] == "2H_BCE"
        if list_sizes is not None:
            inverse = torch.empty(N, dtype=torch.int32, device=self.device)
            inverse[order] = torch.arange(N, dtype=torch.int32, device=self.device)
            out = self.head_lists(lp, lp2 if two else None, labels, list_sizes, want_scores=want_scores, want_order=want_order,
                                  want_loss=want_loss, gather=inverse, joint=joint)
        elif pair_lists is not None:
            out = {}
        else:
            out = self.head(logits, logits2 if two else None, labels, Bq, K, want_scores=want_scores, want_order=want_order,
                            want_loss=want_loss, joint=joint)
        out.update(logits=logits, logits2=logits2, packed_rows=sum(n * s for n, s in zip(seg_n, seg_len)),
                   packed_segments=len(seg_n))
        return out

    # ---- debugging / profiling ------------------------------------------------------------------
    def set_debug(self, on: bool):
        L.check(self.lib.rr_set_debug(self.h, int(on)), self.h)

    def debug_read(self, name: str, numel: int) -> torch.Tensor:
        out = torch.empty(numel, dtype=torch.float32)
        n = self.lib.rr_debug_read(self.h, name.encode(), out.data_ptr(), numel)
        if n < 0:
            L.check(int(n), self.h, "rr_debug_read")
        return out[:n]

    def set_profiling(self, on: bool):
        L.check(self.lib.rr_set_profiling(self.h, int(on)), self.h)

    def get_profile(self, reset: bool = True) -> Dict[str, dict]:
        p = L.RRProfile()
        L.check(self.lib.rr_get_profile(self.h, C.byref(p), int(reset)), self.h, "rr_get_profile")
        return {k: dict(ms=p.ms[i], launches=p.launches[i], flops=p.flops[i], bytes=p.bytes[i])
                for i, k in enumerate(L.KERNEL_CLASSES)}

    def workspace_bytes(self, n_pairs: int, S: int) -> int:
        return int(self.lib.rr_workspace_bytes(self.h, n_pairs, S))

    def set_option(self, key: str, value: int):
        """Pin a numerics option of THIS engine (rr_set_option: "ln_lite", "ln_fold", "resid_split", "resid_lo8", "ce_cls_only",
        "fp8_ffn_down", "fp8_first_layer", "fp8_qkv", "q8_format", "attn_fixed_ref"); -1 = follow the process-wide diagnostic
        switch again.  "q8_format" (0 e4m3, 1 int8; also arch["q8_format"]) is latched by load_state_dict: changing it afterwards
        raises."""
        L.check(self.lib.rr_set_option(self.h, key.encode(), int(value)), self.h, "rr_set_option")

    def get_option(self, key: str) -> int:
        """The EFFECTIVE value of a numerics option (rr_get_option; keys as set_option, "q8_format" included)."""
        import ctypes
        v = ctypes.c_int(0)
        L.check(self.lib.rr_get_option(self.h, key.encode(), ctypes.byref(v)), self.h, "rr_get_option")
        return int(v.value)

    def reserve(self, n_pairs: int, n_queries: int, len_a: int, len_b: int = 0, with_fusion: int = 0,
                packed: bool = False):
        """Allocate everything a forward of at most this shape needs (rr_reserve) on the current stream: afterwards the
        forward neither allocates nor synchronises (a precondition for capturing it into a hipGraph).  `packed`: for
        forward_ids_packed / forward_ids_bucketed / forward_joint_packed / forward_interaction_packed, whose per-query
        tensors are per PAIR (n_queries = n_pairs, as include/rerank_mi355.h documents for the packed calls).  `with_fusion`:
        0 / False none, 1 / True the attention-fusion bias, 2 the bias and the score block of the `fusion_from_li` forwards."""
        if packed:
            n_queries = n_pairs
        L.check(self.lib.rr_reserve(self.h, int(n_pairs), int(n_queries), int(len_a), int(len_b), int(with_fusion),
                                    torch.cuda.current_stream(self.device).cuda_stream), self.h, "rr_reserve")


class _FrozenStub(torch.nn.Module):
    """Placeholder for `context_vision_encoder`: the executor only iterates its `named_parameters()` to
    freeze them (Reranker_base_executor.py:204-207).  The CLIP ViT is upstream of this path."""


class _DropIn(torch.nn.Module):
    """What the drop-in classes share: the engine's weights, the labels, the packed-or-padded routing and the output."""

    def load_state_dict(self, state_dict, strict: bool = False, prefix: str = ""):  # type: ignore[override]
        return self.engine.load_state_dict(state_dict, strict=strict, prefix=prefix)

    def _labels(self, labels: Optional[List[float]], N: int) -> Optional[torch.Tensor]:
        """A labels list as an fp32 device tensor (utils.py:232-233, rerank_model.py:528-529)."""
        if labels is None:
            return None
        assert isinstance(labels, list), "Labels must be a list"
        if self.engine.arch["loss_fn"] == "negative_sampling":
            raise AssertionError("Labels should not be provided for negative sampling loss function")
        assert len(labels) == N
        return torch.tensor(labels, dtype=torch.float32, device=self.engine.device)

    def _route(self, padded, packed, kw: dict):
        """Config `packed_rows`: the same logits over packed rows; calls with `pair_range` (the sharded path) stay padded."""
        if self.packed_rows and kw.get("pair_range") is None:
            kw.pop("pair_range", None)
            return packed
        return padded

    @staticmethod
    def _output(r: dict, logits: torch.Tensor) -> RerankOutput:
        out = RerankOutput(loss=r["loss"], logits=logits)
        for k in ("scores", "order", "logits2", "list_loss", "maxsim"):
            if r.get(k) is not None:
                out[k] = r[k]
        return out

    def _lists(self, candidates_per_query, N: int, kw: dict) -> List[int]:
        """The list layout of a call with `candidates_per_query` (no such keyword in the reference, which reranks one query per
        forward and so never meets two list lengths in one batch): packed rows only, the sizes partition the N contexts."""
        if not self.packed_rows or kw.get("pair_range") is not None:
            raise ValueError("candidates_per_query needs config.packed_rows = True (and no pair_range): lists of unequal length "
                             "go through the packed forwards only")
        sizes = [int(k) for k in candidates_per_query]
        assert sizes and min(sizes) >= 1 and sum(sizes) == N, \
            f"candidates_per_query {sizes} must be positive and sum to the {N} contexts"
        kw.pop("pair_range", None)
        kw.setdefault("want_order", True)
        return sizes

    def _flat_logits(self, r: dict) -> torch.Tensor:
        return r["logits"] if self.engine.arch["loss_fn"] == "negative_sampling" else r["logits"].view(-1, 1)

    def _ranked_logits(self, r: dict, Bq: int, K: int) -> torch.Tensor:
        return r["logits"].view(Bq, K) if self.engine.arch["loss_fn"] == "negative_sampling" else r["logits"].view(Bq * K, 1)


class FullContextRerankModel(_DropIn):
    """Drop-in for the reference's `FullContextRerankModel` (rerank_model.py:515-591), inference only.

    `config` is the reference `reranker_config` (EasyDict/dict).  Extra, optional keys:
      `arch`            – dict overriding the FLMR/BERT architecture defaults (tests use tiny shapes)
      `tokenizer`       – any HF-style tokenizer (encode/decode/batch_encode_plus); required only for the
                          text call signature (no vocab file exists in the build environment)
      `vision_encoder`  – True: run the CLIP ViT-B/32 tower inside the library (rr_encode_image; the state_dict must
                          then hold `context_vision_encoder.vision_model.vision_model.*`)
      `image_feature_fn`– otherwise a callable pixel_values[Bq,3,224,224] -> (cls [Bq,Vh], patches [Bq,np,Vh]) that
                          wraps the reference-side `context_vision_encoder`
      `text_only`       – build without the vision weights (`text_only` module of the reference configs)
      `native_tokenizer`– True: assemble the pair inputs with the library's multi-threaded C++ WordPiece tokenizer
                          (rr_tok_prepare_pairs) built from `tokenizer`'s vocabulary instead of calling `tokenizer`
      `packed_rows`     – True: `forward_ids` and the text `forward` run over packed rows (RerankEngine.forward_ids_packed; the
                          text call hands the tokenizer's pair lengths over, no device -> host copy).  Default False: padded.
                          Calls with `pair_range` (the sharded path) stay padded.

    `forward` / `forward_ids` take an optional keyword `candidates_per_query` (a sequence of ints whose sum is the number of
    contexts): query i owns the next candidates_per_query[i] contexts, `num_negative_examples` is not read, `.logits` is flat
    ([N, 1] for the pointwise losses as today, [N] for negative_sampling) and the output carries `order` ([N] int32, each
    query's rank as indices local to its list) and `list_loss` (each query's own loss).  It needs `packed_rows`.  The reference
    has no such keyword: it reranks one query per forward (Reranker_base_executor.py:807-976).
    """

    def __init__(self, config, state_dict: Optional[Dict[str, torch.Tensor]] = None, device=None):
        super().__init__()
        self.config = config
        arch = make_arch(config)
        if _get(config, "text_only", False):
            arch["has_vision"] = 0
        self.engine = RerankEngine(arch, device)
        self.max_query_length = _get(config, "max_query_length", 32)
        self.max_decoder_source_length = _get(config, "max_decoder_source_length", 512)
        self.max_context_length = self.max_decoder_source_length - self.max_query_length - 4   # HEAD_TOKEN_LEEWAY
        self.query_tokenizer = _get(config, "tokenizer", None)
        self.native_tokenizer = None
        if _get(config, "native_tokenizer", False):
            if self.query_tokenizer is None:
                raise ValueError("native_tokenizer needs config.tokenizer (for its vocabulary)")
            from .pair_inputs import NativePairTokenizer
            self.native_tokenizer = NativePairTokenizer(self.query_tokenizer,
                                                        do_lower_case=getattr(self.query_tokenizer, "do_lower_case", True))
        self.image_feature_fn = _get(config, "image_feature_fn", None)
        self.packed_rows = bool(_get(config, "packed_rows", False))
        self.context_vision_encoder = _FrozenStub()
        if state_dict is not None:
            self.engine.load_state_dict(state_dict)

    # tensor fast path (synthetic benchmarks, pre-tokenised callers)
    def forward_ids(self, input_ids, attention_mask, token_type_ids, num_negative_examples: int,
                    image_cls=None, image_patches=None, labels: Optional[List[float]] = None, candidates_per_query=None,
                    **kw) -> RerankOutput:
        N = input_ids.shape[0]
        if candidates_per_query is not None:
            sizes = self._lists(candidates_per_query, N, kw)
            r = self.engine.forward_ids_packed(input_ids, attention_mask, token_type_ids, None, None, image_cls, image_patches,
                                               self._labels(labels, N), list_sizes=sizes, **kw)
            return self._output(r, self._flat_logits(r))
        K = num_negative_examples + 1
        assert N % K == 0, "expanded batch size must be batch_size * (num_negative_examples + 1)"
        Bq = N // K
        eng = self.engine
        r = self._route(eng.forward_ids, eng.forward_ids_packed, kw)(input_ids, attention_mask, token_type_ids, Bq, K, image_cls,
                                                                     image_patches, self._labels(labels, N), **kw)
        return self._output(r, self._ranked_logits(r, Bq, K))

    def forward(self, query_text_sequences, query_pixel_values, context_text_sequences, num_negative_examples,
                labels=None, candidates_per_query=None) -> RerankOutput:
        text_only = query_pixel_values is None
        batch_size = len(query_text_sequences)
        pair_queries = query_text_sequences
        if candidates_per_query is not None:          # every pair names its query: the tokenizers take one count per call
            sizes = self._lists(candidates_per_query, len(context_text_sequences), {})
            assert len(sizes) == batch_size, "one candidates_per_query entry per query"
            pair_queries = [q for q, k in zip(query_text_sequences, sizes) for _ in range(k)]
            num_negative_examples = 0
        expanded = len(pair_queries) * (num_negative_examples + 1)
        assert expanded == len(context_text_sequences)                                     # rerank_model.py:527
        if labels:
            assert len(labels) == expanded
        if self.query_tokenizer is None:
            raise RuntimeError("text call signature needs config.tokenizer (an HF-style BERT tokenizer)")
        if self.native_tokenizer is not None:
            enc = self.native_tokenizer.prepare_full_context_inputs(
                list(pair_queries), list(context_text_sequences), self.max_query_length, self.max_context_length,
                self.max_decoder_source_length, num_negative_examples + 1, pin_memory=True)
        else:
            from .pair_inputs import prepare_full_context_inputs
            enc = prepare_full_context_inputs(pair_queries, context_text_sequences, self.query_tokenizer,
                                              self.max_query_length, self.max_context_length,
                                              self.max_decoder_source_length, num_negative_examples + 1)
        dev = self.engine.device
        cls = patches = None
        if not text_only:
            if self.image_feature_fn is not None:
                cls, patches = self.image_feature_fn(query_pixel_values)
            elif self.engine.arch.get("vit_layers", 0) > 0:
                cls, patches = self.engine.encode_image(query_pixel_values)
            else:
                raise NotImplementedError("query_pixel_values given but neither config.vision_encoder nor "
                                          "config.image_feature_fn (CLIP ViT) is set")
        kw = {}
        if self.packed_rows:              # the tokenizer's output is host memory: the pair lengths cost no device -> host copy
            kw["lengths"] = pair_lengths(enc["input_ids"], enc["attention_mask"]).numpy()
        return self.forward_ids(enc["input_ids"].to(dev), enc["attention_mask"].to(dev),
                                enc["token_type_ids"].to(dev), num_negative_examples, cls, patches,
                                labels if labels else None, candidates_per_query=candidates_per_query, **kw)


class InteractionRerankModel(_DropIn):
    """Drop-in for the reference's `InteractionRerankModel` (interaction_rerank_model.py:86-166), inference only:
    `config.interaction_type` "MORES" selects the MORES stack (mores_model.py), anything else the CrossEncoder.
    Optional config key `packed_rows` (default False): `forward` runs over packed rows (RerankEngine.forward_interaction_packed;
    pass `lengths=` to spare the device -> host copy of the context lengths).  Calls with `pair_range` stay padded.
    `forward` takes the optional keyword `candidates_per_query` of FullContextRerankModel (lists of unequal length; needs
    `packed_rows`; no reference counterpart), and `fusion_from_li=True` in place of `preflmr_scores`: the attention fusion then
    runs on the retriever's scores computed from the call's own late-interaction tensors (RerankEngine.li_scores; what the
    executor passes as `retrieval_results.scores_raw`), `want_maxsim=True` adds them per pair as `maxsim`.
    `create_bank` / `forward_passages`: the candidates' embeddings in a device-resident bank (passage_bank.PassageBank), named by
    passage id per call; `retriever_scores`: the retriever's MaxSim / score matrix of such pairs from the bank; `rerank_dataset_pipelined` runs the executor's loop from it."""

    def __init__(self, config, state_dict: Optional[Dict[str, torch.Tensor]] = None, device=None):
        super().__init__()
        self.config = config
        kind = "mores" if _get(config, "interaction_type", "NORMAL") == "MORES" else "interaction"
        arch = make_arch(config, model_kind=kind, has_vision=0)
        self.engine = RerankEngine(arch, device)
        self.packed_rows = bool(_get(config, "packed_rows", False))
        self.bank = None                      # create_bank / forward_passages
        if state_dict is not None:
            self.engine.load_state_dict(state_dict)

    def create_bank(self, capacity_rows: int, max_passages: int, codec=None, centroids=None):
        """Give the model a passage-embedding bank (RerankEngine.create_bank; `codec`: a compressed one; `centroids`: an fp16 one with a centroid table) and return it; `bank` may also be assigned a bank
        another model of the same device and li_dim created."""
        self.bank = self.engine.create_bank(capacity_rows, max_passages, codec, centroids=centroids)
        return self.bank

    def forward_passages(self, query_late_interaction, query_mask, passage_ids, num_negative_examples, labels=None,
                         candidates_per_query=None, fusion_from_li=False, fusion_multiplier=1, **kw) -> RerankOutput:
        """`forward` with the candidates named by passage id and their embeddings read from `self.bank`
        (RerankEngine.forward_interaction_bank; always over packed rows): the output `forward` gives for the banked tensors.
        `candidates_per_query` as `forward` takes it.  No reference counterpart (its executor recomputes the embeddings per
        query, Reranker_base_executor.py:877-885)."""
        if self.bank is None:
            raise RuntimeError("forward_passages needs a bank: model.create_bank(capacity_rows, max_passages), then bank.add(...)")
        Bq, N = query_late_interaction.size(0), len(passage_ids)
        common = dict(fusion_from_li=bool(fusion_from_li), fusion_multiplier=float(fusion_multiplier), **kw)
        if candidates_per_query is not None:
            sizes = [int(k) for k in candidates_per_query]
            assert sizes and min(sizes) >= 1 and sum(sizes) == N and len(sizes) == Bq, \
                f"candidates_per_query {sizes} must be positive, one per query, and sum to the {N} passages"
            common.setdefault("want_order", True)
            r = self.engine.forward_interaction_bank(self.bank, query_late_interaction, query_mask, passage_ids, None, None,
                                                     self._labels(labels, N), list_sizes=sizes, **common)
            return self._output(r, self._flat_logits(r))
        K = num_negative_examples + 1
        assert Bq * K == N, f"{query_late_interaction.shape}, {N} passages, {num_negative_examples}"
        r = self.engine.forward_interaction_bank(self.bank, query_late_interaction, query_mask, passage_ids, Bq, K,
                                                 self._labels(labels, N), **common)
        return self._output(r, self._ranked_logits(r, Bq, K))

    def retriever_scores(self, query_late_interaction, passage_ids, **kw) -> dict:
        """The frozen retriever's score of (query, passage) pairs from `self.bank` (RerankEngine.bank_li_scores; colbert_score,
        flmr_utils.py:22-48): {"maxsim"} and, with want_scores=True, {"scores"}.  NORMAL and MORES models."""
        if self.bank is None:
            raise RuntimeError("retriever_scores needs a bank: model.create_bank(capacity_rows, max_passages), then bank.add(...)")
        return self.engine.bank_li_scores(self.bank, query_late_interaction, passage_ids, **kw)

    def retrieve(self, query_late_interaction, k: int, plaid=None, allowed=None, excluded=None, filter=None, sparse: bool = False,
                 fast=None, return_certified: bool = False, **kw):
        """The k best passages of `self.bank` per query by the frozen retriever's MaxSim, every passage scored
        (PassageBank.search): (passage_ids: one list per query, best first; scores float32 [n_queries, k] on the device).
        `plaid` (a PlaidSearch): PLAID's pruned search over a compressed bank, or an fp16 bank with a centroid table, instead; a query's list may then be shorter than k.
        `allowed` / `excluded` (passage ids: a flat sequence for every query, or a list of lists, one per query), or `filter` (a
        BankFilter built by bank.filter): only the allowed passages compete (the reference's filter_fn); one of the three at most.
        A query's list then has its true length, at most k.  `sparse` (with one of the three, without `plaid`; ValueError
        otherwise): the filtered exact search in its list-driven form (RerankEngine.bank_search_filtered_sparse), the same result.
        `fast` (an F16Search; fp16 and compressed banks, with none of the above: ValueError otherwise): the exhaustive search whose first pass
        runs on the fp16 matrix core (RerankEngine.bank_search_f16): exact scores, and with `return_certified` the tuple ends in
        the certificate, int32 [n_queries] on the device (1: the list is provably the exact search's)."""
        if self.bank is None:
            raise RuntimeError("retrieve needs a bank: model.create_bank(capacity_rows, max_passages), then bank.add(...)")
        if return_certified and fast is None:
            raise ValueError("retrieve: return_certified=True needs fast= (an F16Search)")
        if fast is not None:
            if plaid is not None or allowed is not None or excluded is not None or filter is not None or sparse:
                raise ValueError("retrieve: fast= with plaid, a filter or sparse (the fp16 first pass scores every passage of the bank)")
            r = self.bank.search(self.engine, query_late_interaction, k, fast=fast, **kw)
            ids = self.bank.table.ids
            out = ([[ids[j] for j in row] for row in r["indices"].tolist()], r["scores"])
            return out + (r["certified"],) if return_certified else out
        if sparse:                                # before a filter is built or the library is called
            if allowed is None and excluded is None and filter is None:
                raise ValueError("retrieve: sparse=True needs allowed / excluded or a filter")
            if plaid is not None:
                raise ValueError("retrieve: sparse=True with plaid (the pruned searches touch candidates only already)")
            kw["sparse"] = True
        if plaid is not None:
            kw["plaid"] = plaid
        if allowed is not None or excluded is not None:
            if filter is not None:
                raise ValueError("retrieve: give allowed / excluded or a filter built from them, not both")
            filter = self.bank.filter(allowed=allowed, excluded=excluded)
        if filter is not None:
            kw["filter"] = filter
        return self.bank.search(self.engine, query_late_interaction, k, **kw)

    def retrieve_and_rerank(self, query_late_interaction, query_mask, k: int, plaid=None, allowed=None, excluded=None, filter=None,
                            sparse: bool = False, fast=None, **kw):
        """`retrieve` then `forward_passages` on what it found, k candidates per query in retrieval order: (passage_ids, the
        RerankOutput).  `kw` goes to forward_passages (labels default as there: candidate 0 of every query).  With `plaid`, or
        under `allowed` / `excluded` / `filter` (as retrieve takes them), the lists may be of unequal length: they go to
        forward_passages as candidates_per_query; a query that found no candidate raises ValueError.  `sparse`, `fast`: as retrieve
        takes them (`fast` returns k candidates per query, as the exact search does)."""
        filtered = allowed is not None or excluded is not None or filter is not None
        if fast is not None:
            if plaid is not None or filtered or sparse:
                raise ValueError("retrieve_and_rerank: fast= with plaid, a filter or sparse")
            ids, _ = self.retrieve(query_late_interaction, k, fast=fast)
            flat = [pid for row in ids for pid in row]
            return ids, self.forward_passages(query_late_interaction, query_mask, flat, int(k) - 1, **kw)
        if sparse and (plaid is not None or not filtered):
            raise ValueError("retrieve_and_rerank: sparse=True needs allowed / excluded or a filter, and no plaid")
        if plaid is None and not filtered:
            ids, _ = self.retrieve(query_late_interaction, k)
            flat = [pid for row in ids for pid in row]
            return ids, self.forward_passages(query_late_interaction, query_mask, flat, int(k) - 1, **kw)
        ids, _ = self.retrieve(query_late_interaction, k, plaid=plaid, allowed=allowed, excluded=excluded, filter=filter,
                               **(dict(sparse=True) if sparse else {}))
        sizes = [len(row) for row in ids]
        if min(sizes) < 1:
            under = " and ".join((["its filter"] if filtered else []) + ([repr(plaid)] if plaid is not None else []))
            raise ValueError(f"retrieve_and_rerank: query {sizes.index(0)} found no candidate under {under}")
        flat = [pid for row in ids for pid in row]
        return ids, self.forward_passages(query_late_interaction, query_mask, flat, int(k) - 1, candidates_per_query=sizes, **kw)

    def forward(self, query_late_interaction, context_late_interaction, num_negative_examples, query_mask,
                context_mask, preflmr_scores=None, fusion_multiplier=1, labels=None, candidates_per_query=None,
                fusion_from_li=False, **kw) -> RerankOutput:
        Bq = query_late_interaction.size(0)
        N = context_late_interaction.size(0)
        if fusion_from_li:                    # (without it the engine is called exactly as before)
            kw["fusion_from_li"] = True
        if candidates_per_query is not None:
            sizes = self._lists(candidates_per_query, N, kw)
            r = self.engine.forward_interaction_packed(
                query_late_interaction, context_late_interaction, query_mask, context_mask, None, None, self._labels(labels, N),
                preflmr_scores=preflmr_scores, fusion_multiplier=float(fusion_multiplier), list_sizes=sizes, **kw)
            return self._output(r, self._flat_logits(r))
        K = num_negative_examples + 1
        assert Bq * K == N, f"{query_late_interaction.shape}, {context_late_interaction.shape}, {num_negative_examples}"
        eng = self.engine
        r = self._route(eng.forward_interaction, eng.forward_interaction_packed, kw)(
            query_late_interaction, context_late_interaction, query_mask, context_mask, Bq, K, self._labels(labels, N),
            preflmr_scores=preflmr_scores, fusion_multiplier=float(fusion_multiplier), **kw)
        return self._output(r, self._ranked_logits(r, Bq, K))


class RerankModel(_DropIn):
    """Drop-in for the reference's `RerankModel` (rerank_model.py:76-331; the "softmax"/2-head variant), inference
    only.  Extra optional config keys: `arch`, `image_feature_fn` (pixel_values -> (cls, patches)),
    `instruction_token_id` (id of `mask_instruction_token`, rerank_model.py:161-169; None = no instruction masking),
    `packed_rows` (default False: `forward` runs over packed rows, RerankEngine.forward_joint_packed; pass `lengths=` with the
    joint sequences' lengths to spare the device -> host copy; calls with `pair_range` stay padded), `decoder_tokenizer` (the
    executor's context tokenizer, an HF-style BERT tokenizer: the vocabulary of `native_tokenizer`, which
    rerank_dataset_pipelined tokenises the retrieved passages with) and `max_decoder_source_length` (the context rows'
    padded length; must equal the text encoder's max_pos, as `forward` asserts).  `forward` takes the optional keyword
    `candidates_per_query` of FullContextRerankModel (lists of unequal length; needs `packed_rows`; no reference counterpart),
    and, in place of `preflmr_scores`, the retriever's embeddings `retriever_query_li` [Bq, query_len + image tokens, D],
    `retriever_context_li` [N, S, D] and `retriever_context_mask` [N, S]: the scores are computed on the device
    (RerankEngine.li_scores); giving both raises ValueError."""

    def __init__(self, config, state_dict: Optional[Dict[str, torch.Tensor]] = None, device=None):
        super().__init__()
        self.config = config
        self.engine = RerankEngine(make_arch(config), device)
        self.image_feature_fn = _get(config, "image_feature_fn", None)
        self.instruction_token_id = _get(config, "instruction_token_id", None)
        self.packed_rows = bool(_get(config, "packed_rows", False))
        self.max_decoder_source_length = int(_get(config, "max_decoder_source_length", self.engine.arch["max_pos"]))
        assert self.max_decoder_source_length == self.engine.arch["max_pos"], \
            f"max_decoder_source_length {self.max_decoder_source_length} != max_pos {self.engine.arch['max_pos']}"   # :202
        self.decoder_tokenizer = _get(config, "decoder_tokenizer", None)
        self.native_tokenizer = None
        if self.decoder_tokenizer is not None:
            from .pair_inputs import NativePairTokenizer
            self.native_tokenizer = NativePairTokenizer(self.decoder_tokenizer,
                                                        do_lower_case=getattr(self.decoder_tokenizer, "do_lower_case", True))
        self.context_vision_encoder = _FrozenStub()
        if state_dict is not None:
            self.engine.load_state_dict(state_dict)

    def forward(self, query_input_ids, query_attention_mask, query_pixel_values, context_input_ids,
                context_attention_mask, num_negative_examples, preflmr_scores=None, fusion_multiplier=1, labels=None,
                image_features=None, candidates_per_query=None, **kw) -> RerankOutput:
        if query_pixel_values is None and image_features is None:
            raise NotImplementedError("text_only is not implemented for this model")        # rerank_model.py:184-185
        K = num_negative_examples + 1
        Bq = query_input_ids.size(0)
        sizes = None
        if candidates_per_query is not None:
            sizes = self._lists(candidates_per_query, context_input_ids.size(0), kw)
            assert len(sizes) == Bq, "one candidates_per_query entry per query"
            K = torch.tensor(sizes, device=self.engine.device)                              # repeats per query
        N = Bq * K if sizes is None else sum(sizes)
        assert N == context_input_ids.size(0)                                               # :188
        if labels:
            assert len(labels) == N                                                         # :189-190
        ql, S = query_input_ids.size(1), context_input_ids.size(1)
        assert S == self.engine.arch["max_pos"]                                             # :202
        dev = self.engine.device
        # joint sequence exactly as :191-224 builds it (index plumbing on device tensors, no arithmetic)
        q_ids = query_input_ids.to(dev).repeat_interleave(K, dim=0)
        q_am = query_attention_mask.to(dev).repeat_interleave(K, dim=0)
        joint_ids = torch.cat([q_ids, context_input_ids.to(dev)[:, 2:2 - ql]], dim=1).to(torch.int64).contiguous()
        joint_am = torch.cat([q_am, context_attention_mask.to(dev)[:, 2:2 - ql]], dim=1).to(torch.int64).contiguous()
        if image_features is not None:
            cls, patches = image_features
        else:
            if self.image_feature_fn is not None:
                cls, patches = self.image_feature_fn(query_pixel_values)
            elif self.engine.arch.get("vit_layers", 0) > 0:
                cls, patches = self.engine.encode_image(query_pixel_values)
            else:
                raise NotImplementedError("query_pixel_values given but neither config.vision_encoder nor "
                                          "config.image_feature_fn (CLIP ViT) is set")
        eng = self.engine
        if sizes is not None:
            r = eng.forward_joint_packed(joint_ids, joint_am, None, None, ql, cls, patches, self.instruction_token_id,
                                         preflmr_scores=preflmr_scores, fusion_multiplier=float(fusion_multiplier),
                                         list_sizes=sizes, **kw)
            return self._output(r, r["logits"].view(N, 1))
        r = self._route(eng.forward_joint, eng.forward_joint_packed, kw)(
            joint_ids, joint_am, Bq, K, ql, cls, patches, self.instruction_token_id, preflmr_scores=preflmr_scores,
            fusion_multiplier=float(fusion_multiplier), **kw)
        return self._output(r, r["logits"].view(N, 1))
