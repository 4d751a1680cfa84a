/*
 * rerank_mi355.h — C ABI of librerank_mi355.so
 *
 * MI355X (gfx950) native cross-encoder rerank forward: the batched
 * (query x K-candidate) BERT-style encoder, the 128-d late-interaction bottleneck,
 * the optional vision prefix / mapping network, the Lc-layer cross encoder, the
 * pointwise (sigmoid/BCE), two-head (softmax/CE) or listwise (softmax/CE) scoring head
 * and the descending stable top-K order, executed as hand-written HIP kernels on a
 * caller-supplied HIP stream.
 *
 * Drop-in boundary (citations are into /root/reference/):
 *   - the call `self.reranker(**batch_input)` in the Rerank executor
 *     (src/executors/Reranker_base_executor.py:603,758,902-903,922) whose callee is
 *     FullContextRerankModel.forward (src/models/rerank/rerank_model.py:523-591) /
 *     RerankModel.forward (:171-331);
 *   - the reference has no FFI of its own for this path (it is pure PyTorch), so the
 *     entry points below are what a ctypes/pybind binding of that module's
 *     __init__/load_state_dict/forward would bind.  INTEGRATION.md shows the
 *     reference-side stub.
 *
 * Conventions
 *   - plain C, no torch types; every pointer marked DEVICE is a HIP device pointer
 *     that the library BORROWS for the duration of the call; HOST pointers are read
 *     before the call returns.
 *   - every function returns rr_status (0 = ok, <0 = error); rr_last_error() gives a
 *     human-readable message for the last failure on that handle.  The library never
 *     aborts/exits and never silently falls back to a CPU path.
 *   - a handle is NOT thread-safe; several handles per process are fine.  All kernels
 *     are enqueued on the hipStream_t passed in (as void*); rr_forward does not
 *     synchronise the device or the stream.
 */
#ifndef RERANK_MI355_H
#define RERANK_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RR_ABI_VERSION 2

typedef enum rr_status {
  RR_OK = 0,
  RR_ERR_BAD_ARG = -1,      /* null pointer / bad enum / handle misuse            (Python: ValueError)          */
  RR_ERR_BAD_SHAPE = -2,    /* N != Bq*K, S > max_pos, label count ...            (Python: AssertionError,
                                rerank_model.py:188-190,202,527-529)                                             */
  RR_ERR_BAD_DTYPE = -3,    /* unsupported weight dtype                            (Python: ValueError,
                                attention_fusion.py:97-100)                                                      */
  RR_ERR_UNSUPPORTED = -4,  /* configuration the kernels do not cover              (Python: NotImplementedError,
                                rerank_model.py:185, mores_model.py:72-73)                                       */
  RR_ERR_HIP = -5,          /* a HIP runtime call failed                           (Python: RuntimeError)        */
  RR_ERR_OOM = -6,          /* device allocation failed                            (Python: MemoryError)         */
  RR_ERR_MISSING_WEIGHT = -7, /* rr_finalize_weights: a required tensor was never loaded (Python: KeyError)      */
  RR_ERR_NO_DEVICE = -8,    /* no gfx950 device visible                            (Python: RuntimeError)        */
  RR_ERR_RANGE = -9         /* an EARLIER forward of this handle raised the fp16 activation range flag: its logits are
                               unreliable (rr_activation_range_flag below; no reference counterpart) (Python: OverflowError) */
} rr_status;

typedef enum rr_dtype { RR_F32 = 0, RR_BF16 = 1, RR_F16 = 2 } rr_dtype;

/* scoring head / loss (src/models/rerank/utils.py:208-254) */
typedef enum rr_loss_kind {
  RR_LOSS_BCE = 0,               /* pointwise: BCEWithLogits(pos_weight), logits [N,1]                */
  RR_LOSS_2H_BCE = 1,            /* two heads: CrossEntropy([l1,l2], weight=[1,pos_weight]); logits_out = l2 */
  RR_LOSS_NEGATIVE_SAMPLING = 2  /* listwise: logits viewed [Bq,K], CrossEntropy(target = 0)          */
} rr_loss_kind;

/* Architecture.  Field names follow the reference configs
 * (configuration_flmr.py:220-236,332-350; monoBERT_pointwise.jsonnet:111-122). */
typedef struct rr_config {
  int32_t abi_version;        /* = RR_ABI_VERSION */
  /* FLMR text encoder (= BertModel) */
  int32_t vocab_size, hidden, layers, heads, intermediate, max_pos, type_vocab;
  float ln_eps;
  int32_t li_dim;             /* late-interaction dim (128) */
  /* cross encoder (rerank_model.py:89-101) */
  int32_t ce_hidden, ce_layers, ce_heads, ce_intermediate, ce_max_pos;
  /* vision prefix + transformer mapping network (modeling_flmr.py:603-664); has_vision=0 => text_only */
  int32_t has_vision, vision_hidden, prefix_len, n_patches, map_layers, cross_attn_len;
  /* head */
  int32_t loss_kind;          /* rr_loss_kind */
  float pos_weight;           /* NaN = none (utils.py:210,215) */
  int32_t device;             /* HIP device ordinal */
  int32_t compute_dtype;      /* 16-bit MFMA operand type: 0 = bf16 (default; the reference runs bf16-mixed),
                                 1 = fp16 (same MFMA rate, 3 more mantissa bits: logits within 1e-3 of the fp32
                                 forward; range +-65504 is ample for BERT activations, accumulation/residual/
                                 LayerNorm/softmax stay fp32 in both modes) */
  int32_t model_kind;         /* rr_model_kind: which reference reranker class the handle stands for */
  /* optional CLIP ViT image-feature producer (rr_encode_image); vit_layers = 0 => features come from the caller.
     Defaults of FLMRVisionConfig (configuration_flmr.py:90-104): 12 layers, 12 heads, 3072, 224, 32; hidden =
     vision_hidden, n_patches must equal (vit_image_size / vit_patch_size)^2, head dim 64. */
  int32_t vit_layers, vit_heads, vit_intermediate, vit_image_size, vit_patch_size;
  int32_t fp8;                /* 1 = BASELINE configs[4] mode: the QKV (layers >= 1 of a stack) and FFN-up GEMMs of the text and
                                 cross encoder take e4m3 operands on the block-scaled matrix core — activations quantised per row
                                 by the LayerNorm that produces them, weights per output channel at rr_finalize_weights —
                                 while attention and the GEMMs feeding the residual stream stay in compute_dtype.  Logit drift
                                 is reported separately (north_star's 1e-3 is a 16-bit figure); needs hidden % 128 == 0. */
} rr_config;

/* reranker families */
typedef enum rr_model_kind {
  RR_MODEL_FULL_CONTEXT = 0,  /* FullContextRerankModel (monoBERT / monoPreFLMR), rerank_model.py:515-591  -> rr_forward */
  RR_MODEL_INTERACTION = 1,   /* InteractionRerankModel, interaction_type NORMAL (ModPreFLMR-BERT),
                                 interaction_rerank_model.py:110-166                          -> rr_forward_interaction */
  RR_MODEL_MORES = 2          /* InteractionRerankModel, interaction_type MORES (ModPreFLMR-IB), mores_model.py:21-94 */
} rr_model_kind;

typedef struct rr_model* rr_handle;

/* Per-kernel-class device time accumulated while profiling is on (rr_set_profiling). */
typedef enum rr_kernel_class {
  RR_K_GEMM = 0, RR_K_ATTENTION = 1, RR_K_LAYERNORM = 2, RR_K_EMBED = 3, RR_K_TAIL = 4, RR_K_HEAD = 5,
  RR_K_GEMM_FP8 = 6,          /* 8-bit GEMM launches (e4m3 or int8) of rr_config.fp8 (priced against the 8-bit matrix-core peak) */
  RR_K_COUNT = 7
} rr_kernel_class;

typedef struct rr_profile {
  double ms[RR_K_COUNT];      /* summed device ms per class (HIP events on the work stream) */
  int64_t launches[RR_K_COUNT];
  double flops[RR_K_COUNT];   /* algorithmic FLOPs issued per class (2*M*N*K, 4*T^2*dh per head ...) */
  double bytes[RR_K_COUNT];   /* algorithmic HBM bytes (operands read once + results written once) */
} rr_profile;

const char* rr_version(void);
const char* rr_status_string(int status);

/* rr_create: allocate a model for `cfg` on cfg->device.  Replaces RerankerClass(reranker_config)
 * (Reranker_base_executor.py:191-202 -> rerank_model.py:81-101,515-520). */
int rr_create(const rr_config* cfg, rr_handle* out);
int rr_destroy(rr_handle h);
const char* rr_last_error(rr_handle h);

/* rr_load_weight: copy ONE tensor (HOST pointer, row-major, `dtype`) into library-owned
 * device memory, converting/packing as the kernels need.  `name` is the reference
 * state_dict key without the executor's `reranker.` prefix, e.g.
 * "context_text_encoder.bert_model.encoder.layer.0.attention.self.query.weight"
 * (Reranker_base_executor.py:351-381 loads these with strict=False: unknown names are
 * ignored and reported through *known = 0).  Replaces load_state_dict. */
int rr_load_weight(rr_handle h, const char* name, const void* host_data, int dtype,
                   int ndim, const int64_t* shape, int* known);
/* rr_finalize_weights: verify every tensor the configured path reads was loaded, build
 * fused/packed forms (QKV concat, log2(e)/sqrt(dh) folded into Wq and bq).  Must precede rr_forward. */
int rr_finalize_weights(rr_handle h);
/* number of tensors the configured path requires, and the i-th required name */
int rr_num_required_weights(rr_handle h);
const char* rr_required_weight_name(rr_handle h, int i);

/* Bytes of grow-only device workspace rr_forward would hold for this shape. */
int64_t rr_workspace_bytes(rr_handle h, int n_pairs, int seq_len);

/* rr_reserve: allocate once, outside the forward, everything a forward over at most n_pairs pairs of n_queries queries
 * would otherwise grow on first use (workspace, the attention kernels' redo flags for `hip_stream`, and with
 * with_fusion != 0 the attention-fusion bias).  len_a = seq_len for full-context models, Lq for interaction models;
 * len_b = Lc (interaction models only).  After rr_reserve no forward of that or a smaller shape allocates, frees or
 * synchronises, which makes the forward capturable into a hipGraph; without it the first forward of a larger shape
 * grows the buffers (synchronising the stream) and a forward under stream capture that would have to grow fails with
 * RR_ERR_BAD_ARG.  Graphs captured earlier stay replayable when a LATER call on the same handle (a larger rr_forward,
 * rr_encode_image, the fusion bias) outgrows a buffer: once rr_reserve has been called or a capture has been seen on the
 * handle, an outgrown block is retired until rr_destroy instead of freed, and the attention redo-flag buffers are never
 * freed; such a replay computes in the old blocks it was captured with (and overlaps nothing the handle still uses).  What
 * a replay does NOT survive: rr_destroy of the handle.  The module's constructor-time analogue in the reference: none
 * (PyTorch's caching allocator).
 * with_fusion: 0 = no attention fusion, 1 = the fusion bias, 2 = the bias and, on a NORMAL interaction handle, the score block
 * [n_pairs, Lc, Lq] that rr_forward_interaction_fusion_li / rr_forward_interaction_packed_fusion_li compute into (on other
 * handles 2 means 1: their scores stay with the caller, rr_li_scores). */
int rr_reserve(rr_handle h, int n_pairs, int n_queries, int len_a, int len_b, int with_fusion, void* hip_stream);

/* Length-bucketed execution (SURVEY.md "Variable length"; the reference pads every pair to max_decoder_source_length,
 * utils.py:157-165).  After rr_set_padded_seq_len(h, S_pad) a full-context rr_forward may be called with a seq_len S <= S_pad —
 * the host hands over only the first S columns of the pairs whose real length fits — and computes what the S_pad-long call
 * computes for those pairs: text positions are 0..S-1 either way, padded keys contribute exactly 0 to every softmax, and the
 * vision tokens of the cross-encoder keep the positions S_pad.. they have behind the padded text.  Text-only models: logits bit
 * for bit those of the padded call; with vision tokens the cross-encoder's key tiles are cut at other places, i.e. equal up to
 * fp32 summation order.  "Bit for bit" holds while the shorter call's attention grid and the padded call's are on the same
 * side of the 1 024-workgroup threshold between the online and the fixed-reference softmax schedule (a bucket of a few
 * pairs runs the online form: same values up to rounding); rr_forward_packed has no such condition.  0 switches it off.
 * ROW-COUNT DEPENDENCE OF THE ROUNDINGS (every forward entry point): a GEMM row's values never depend on the rows that share its
 * launch, but the form the residual stream takes between the two residual epilogues of a layer does — (hi, lo) 16-bit pairs where
 * the call has at least 128 tiles of 256 x 256 rows x hidden (about 11k rows at hidden 768: the persistent ring runs there),
 * fp32 rows below.  A bucket, a pair_begin / pair_end slice or a multi-GPU shard under that size therefore agrees with the
 * large call to the parity tolerance (1e-3 in fp16; measured ~2e-4 on c3_full: tests/test_gpu_parity_fullsize.py,
 * test_sharded_slices_and_the_whole_list_agree_within_the_parity_gate), not to the bit.  "resid_split" = 0 removes the
 * dependence (fp32 rows at every size, +3 % time at the bench shape).
 * Python: RerankEngine.forward_ids_bucketed. */
int rr_set_padded_seq_len(rr_handle h, int padded_seq_len);

/* Per-handle numerics options: everything that changes WHICH arithmetic a forward of this handle runs lives in the handle
 * ("no global state => several handles per process"; the reference's analogue is the reranker_config each
 * module instance owns, Reranker_base_executor.py:191-202).  Two handles of one process may differ in any of them; a change
 * takes effect with the next forward of THAT handle.
 *   key              values                 default   meaning
 *   "ln_lite"        0 | 1                  1         1: residuals are recomputed from LayerNorm statistics; 0: every LayerNorm
 *                                                     writes its fp32 output and the residual GEMMs read it back (reference dataflow)
 *   "ln_fold"        0 | 1                  1         1: LayerNorm folded into the consumer GEMMs (QKV, FFN-up); 0: LayerNorm kernels
 *   "resid_split"    0 | 1                  1         1: pre-LayerNorm rows between the residual epilogues as 16-bit hi + lo
 *                                                     (where the persistent ring runs); 0: fp32 rows
 *   "resid_lo8"      0 | 1                  by dtype  form of that lo half.  1: e5m2 bytes of (x - hi) * 16 (6 bytes per element through
 *                                                     the residual epilogues instead of 8: -1.6 % step time at the bench shape; x kept to
 *                                                     >= 14 significant bits behind an fp16 hi, 11 behind a bf16 hi); 0: fp16 (22 / 19
 *                                                     bits).  Default: 1 for fp16 handles (drift against the fp32 goldens unchanged),
 *                                                     0 for bf16 handles (it would add ~20 % to theirs)
 *   "ce_cls_only"    0 | 1                  1         1: the cross-encoder's last layer computes queries / FFN for the CLS row of a
 *                                                     pair only (all the classifiers read, utils.py:105-108); 0: every row
 *   "fp8_ffn_down"   0 | 1                  0         rr_config.fp8 only: FFN-down on the e4m3 ring too (GELU output as e4m3 under a
 *                                                     static scale of 8); 0: FFN-down keeps 16-bit operands
 *   "fp8_first_layer" 0 .. layers           layers-1  rr_config.fp8 only: text-encoder layers with an index below this value keep
 *                                                     16-bit operands (the folded-LayerNorm dataflow); layers from it on run the
 *                                                     e4m3 configuration.  `layers` (or more) = no e4m3 GEMM at all; 0 = every
 *                                                     layer (the whole-stack form: 1.13x the 16-bit line on bert-large, and
 *                                                     MEASURED not to keep the fp32 top-5 on the ranking fixtures — opt in only
 *                                                     with a checkpoint you have validated).  A perturbation injected early is
 *                                                     amplified by every later layer, so e4m3 goes into the LAST layers first;
 *                                                     the default (the last layer only) is the largest subset that ranks with a margin that survives
 *                                                     a re-draw of unrelated roundings (DESIGN.md "fp8").  int8 handles
 *                                                     ("q8_format" 1): default layers-12
 *   "fp8_qkv"        0 | 1                  1         rr_config.fp8 only: 0 = of an e4m3 layer only the FFN takes e4m3 operands,
 *                                                     its QKV projection keeps 16-bit ones
 *   "q8_format"      0 | 1                  0         rr_config.fp8 only: the 8-bit operand format.  0 = e4m3 (the block-scaled
 *                                                     MFMA); 1 = int8 (W8A8: v_mfma_i32_*_i8, int32 accumulation, activations
 *                                                     per row by the producing LayerNorm (amax / 127), weights per output
 *                                                     channel, each LayerNorm's gain outliers migrated into the consumer weights
 *                                                     by powers of two at rr_finalize_weights).  Same GEMMs as e4m3 (QKV of
 *                                                     layers >= 1, FFN-up); "fp8_first_layer" / "fp8_qkv" apply unchanged, the
 *                                                     default of "fp8_first_layer" for int8 handles is layers - 12 (the
 *                                                     last 12 layers: the largest suffix that keeps the fp32 top-5 with
 *                                                     margin on the ranking fixtures; the whole stack runs 1.10x the 16-bit
 *                                                     line but does not, DESIGN.md "int8"); "fp8_ffn_down" = 1 is refused.
 *                                                     Latched by rr_finalize_weights (it packs ONE format): a later change
 *                                                     returns RR_ERR_BAD_ARG
 *   "attn_fixed_ref" 0 | 1 | 2 | 3          3         softmax schedule of large attention grids: 0 online only, 1 fixed reference
 *                                                     with 32 query rows per wave, 2 with 64, 3: 2 where 256-row workgroups pad no
 *                                                     more rows than 128-row ones, else 1
 * value -1 = "not set": the handle follows the process-wide diagnostic switch of the same name (rr_set_tuning), which is what
 * every option starts as.  rr_get_option returns the EFFECTIVE value.  RR_ERR_BAD_ARG: unknown key, value out of range. */
int rr_set_option(rr_handle h, const char* key, int value);
int rr_get_option(rr_handle h, const char* key, int* value_out);

/* Range guard of the 16-bit residual rows.  With the folded LayerNorm the RAW pre-LayerNorm rows are MFMA operands and the
 * `hi` half of the residual stream; fp16 (the mode that meets 1e-3) ends at 65 504.  The kernel that merges the rows'
 * LayerNorm statistics raises a device-side flag when a row's sum of squares reaches 9e8 (no element of a row below that can
 * exceed 3e4) or is not finite; BERT-family activations stay four orders of magnitude below.  rr_activation_range_flag
 * copies the flag to *flag_out (synchronises `hip_stream`; call it outside the hot loop, e.g. once per evaluation batch
 * group) and clears it when reset != 0.  A raised flag means: rebuild the handle with compute_dtype = 0 (bf16, the
 * reference's autocast type, same exponent range as fp32).  Python: RerankEngine.activation_range_exceeded().
 * STICKY ERROR: every forward ends with an asynchronous copy of the flag word into pinned host memory (no synchronisation), and
 * every forward BEGINS by looking at that word: once a forward has raised the flag, the next rr_forward* call on the handle
 * returns RR_ERR_RANGE instead of computing — a caller that never polls cannot keep ranking with out-of-range activations for
 * more than the one batch whose logits it was about to read anyway.  rr_activation_range_flag(reset = 1) clears it (then build
 * the handle with compute_dtype = bf16 for this checkpoint).
 * The 9e8 limit applies to compute_dtype = fp16 handles only.  A bf16 handle (fp32's exponent range) raises the flag, and is
 * refused afterwards, only when a row is NOT FINITE (inf / NaN in the inputs or the weights); 3e4 is an ordinary value there.
 */
int rr_activation_range_flag(rr_handle h, int reset, int* flag_out, void* hip_stream);

/* rr_forward_packed: the same computation over PACKED rows (SURVEY.md "Variable length"): the caller
 * groups the pairs into n_segments segments of equal row length seg_len[i] <= padded_seq_len (the length the reference
 * would pad to, utils.py:157-165; every pair's non-pad tokens must fit its segment's length) and hands over
 *   input_ids / attention_mask / token_type_ids : DEVICE int64, sum_i seg_pairs[i] * seg_len[i] entries: segment after
 *       segment, inside a segment pair after pair, seg_len[i] entries per pair (token_type_ids may be NULL);
 *   image_cls / image_patches : DEVICE float32 PER PAIR, [n, vision_hidden] / [n, n_patches, vision_hidden] in the packed
 *       pair order, or both NULL (a segment mixes the candidates of several queries);
 *   logits_out (/ logits2_out for 2H_BCE) : DEVICE float32 [n] in the packed pair order; the caller scatters them back
 *       and runs rr_head on the [Bq, K] block.
 * Every GEMM, every LayerNorm statistics pass and the attention of a layer run ONCE over all rows of the call (attention as
 * one launch over the segments' workgroups when the padded call's grid selects the fixed-reference schedule); the embedding
 * gathers and the CLS heads run once per segment.  A pair's logit equals what rr_forward computes for it after
 * rr_set_padded_seq_len(padded_seq_len) at seq_len = seg_len[i], hence what the padded call computes: bit for bit for
 * text-only models (attention runs the schedule the padded call's grid would choose, whatever the segment's size); with
 * vision tokens up to fp32 summation order in the cross-encoder's attention and in the per-pair vision GEMMs (1.3e-4 at
 * 800 pairs, tests/test_gpu_parity_fullsize.py).  For rr_reserve count n_queries = n_pairs (image features are per pair).
 * No reference counterpart (it pads); Python: RerankEngine.forward_ids_packed.  RR_ERR_BAD_SHAPE: more than 64 segments,
 * an empty segment, a length above padded_seq_len or, with image features, below the mapping network's cross-attention
 * window (32). */
int rr_forward_packed(rr_handle h, const int64_t* input_ids, const int64_t* attention_mask, const int64_t* token_type_ids,
                      const float* image_cls, const float* image_patches, int n_segments, const int32_t* seg_pairs,
                      const int32_t* seg_len, int padded_seq_len, float* logits_out, float* logits2_out, void* hip_stream);

/* rr_assemble_pairs: the token inputs of rr_forward_packed built on the device from rr_tok_prepare_compact's output, instead of
 * uploading padded int64 rows.  pool: DEVICE int32 [pool_len]; desc: HOST int32 [n_pairs, 4] (query offset, la, context
 * offset, lb) in pair order; order: HOST int32 [n_pairs], the packed pair order (pair order[i] is the i-th packed pair);
 * n_segments / seg_pairs / seg_len: HOST segment table as rr_forward_packed takes it (1..64 segments, sum seg_pairs = n_pairs).
 * Writes input_ids / attention_mask / token_type_ids (DEVICE int64, sum_s seg_pairs[s] * seg_len[s] entries, segment after
 * segment, pair after pair; token_type_ids may be NULL): [CLS] q[:la] [SEP] c[:lb] [SEP] with mask 1, type 1 on c[:lb] and the
 * closing [SEP], then pad_id with mask 0 and type 0 — rr_tok_prepare_pairs' row of the pair, cut to its segment's length.  The
 * padded [N, S] layout is one segment of length S with the identity order.  Every descriptor is checked on the host BEFORE
 * anything is enqueued (non-negative lengths and offsets, both runs inside the pool, la + lb + 3 <= its segment's length, order a
 * permutation): any violation returns RR_ERR_BAD_SHAPE and writes nothing.  The library stages the descriptors to the device
 * itself (desc and order may be reused when the call returns).  Enqueued on hip_stream; not capturable into a graph. */
int rr_assemble_pairs(rr_handle h, const int32_t* pool, int64_t pool_len, const int32_t* desc, int n_pairs, const int32_t* order,
                      int n_segments, const int32_t* seg_pairs, const int32_t* seg_len, int64_t cls_id, int64_t sep_id,
                      int64_t pad_id, int64_t* input_ids, int64_t* attention_mask, int64_t* token_type_ids, void* hip_stream);

/* rr_assemble_joint: the joint rows of rr_forward_joint_packed built on the device from compact tokens, instead of the
 * reference's cat(query_input_ids, context_input_ids[:, 2 : 2 - query_len]) over padded rows (RerankModel.forward,
 * rerank_model.py:191-222, on tokenize_retrieved_docs' [N, 512] output, Reranker_base_executor.py:1056-1066).
 * pool: DEVICE int32 [pool_len], holding every query's query_len ids followed by its query_len attention-mask values (as the
 * dataset gives them), and the context runs of rr_tok_prepare_contexts_compact; desc: HOST int32 [n_pairs, 3] (query offset,
 * context offset, m) in pair order: the query's ids at pool[qoff .. qoff + query_len), its mask behind them, the context's
 * t[0:m] at pool[coff .. coff + m); order / n_segments / seg_pairs / seg_len as rr_assemble_pairs takes them.  Writes
 * joint_input_ids / joint_attention_mask (DEVICE int64, sum_s seg_pairs[s] * seg_len[s] entries, packed as rr_forward_joint_packed
 * reads them): q_ids | the first padded_seq_len - query_len entries of t[0:m] [SEP] [PAD]..., mask q_mask | 1 ... 1 | 0 ..., cut
 * to the segment's length.  A pair's real length is query_len + min(m + 1, padded_seq_len - query_len) (a passage that fills
 * its window loses the [SEP], as in the reference).  Checked on the host BEFORE anything is enqueued: 0 < query_len <
 * padded_seq_len, every seg_len in (query_len, padded_seq_len] and at least min(padded_seq_len, cross_attn_len) (the
 * preconditions of rr_forward_joint_packed), order a permutation, non-negative offsets and m, the query's 2 * query_len values
 * and the context run inside the pool, every pair's real length within its segment's; any violation returns RR_ERR_BAD_SHAPE and
 * writes nothing.  The library stages the descriptors itself; enqueued on hip_stream; not capturable into a graph. */
int rr_assemble_joint(rr_handle h, const int32_t* pool, int64_t pool_len, const int32_t* desc, int n_pairs, const int32_t* order,
                      int n_segments, const int32_t* seg_pairs, const int32_t* seg_len, int query_len, int padded_seq_len,
                      int64_t sep_id, int64_t pad_id, int64_t* joint_input_ids, int64_t* joint_attention_mask, void* hip_stream);

/* rr_forward: one pass of the hot path over N = Bq*K (query,candidate) pairs.
 *   input_ids, attention_mask, token_type_ids : DEVICE int64 [N,S] row-major, query-major pair order
 *       (prepare_full_context_inputs, utils.py:129-167).  attention_mask masks keys in the text
 *       encoder; the cross-encoder mask is (input_id != 0) (rerank_model.py:385-392,562).
 *   image_cls     : DEVICE float32 [Bq, vision_hidden] or NULL (text_only) — CLIP last_hidden_state[:,0]
 *   image_patches : DEVICE float32 [Bq, n_patches, vision_hidden] or NULL — CLIP hidden_states[-2][:,1:]
 *       (per query; repeated over the K pairs inside, rerank_model.py:541-544)
 *   labels        : DEVICE float32 [N] or NULL (NULL: first candidate of each query is the positive,
 *       utils.py:239-243; must be NULL for RR_LOSS_NEGATIVE_SAMPLING, utils.py:233)
 *   logits_out    : DEVICE float32 [N]   (= [N,1] pointwise / [Bq,K] listwise; 2H_BCE: second head)
 *   logits2_out   : DEVICE float32 [N] or NULL (first head of 2H_BCE / classifier2 otherwise)
 *   loss_out      : DEVICE float32 [1] or NULL
 *   scores_out    : DEVICE float32 [N] or NULL — sigmoid(logit) (pointwise) / softmax over K (listwise)
 *   order_out     : DEVICE int32 [Bq,K] or NULL — per query, candidate indices sorted by logit,
 *       descending, ties in retrieval order (Reranker_base_executor.py:934-935)
 *   pair_begin/pair_end : this rank's contiguous slice [pair_begin, pair_end) of the N pairs
 *       (multi-GPU sharding; 0,N = everything).  Only that slice of logits_out is written; the head
 *       (loss/scores/order) is computed by rr_head after the caller has all-gathered logits.
 *       With the full range the head runs inside rr_forward.
 * A call (or slice) of more than 2^30 rows — pairs x (seq_len + vision tokens) — returns RR_ERR_BAD_SHAPE before anything is
 * allocated or launched (row counts are 32-bit inside a forward); rr_reserve and the interaction / packed forwards likewise.
 */
int rr_forward(rr_handle h, const int64_t* input_ids, const int64_t* attention_mask,
               const int64_t* token_type_ids, const float* image_cls, const float* image_patches,
               int Bq, int K, int S, const float* labels, int pair_begin, int pair_end,
               float* logits_out, float* logits2_out, float* loss_out, float* scores_out,
               int32_t* order_out, void* hip_stream);

/* rr_encode_image: the frozen CLIP vision tower the rerankers call once per query
 * (rerank_model.py:408-411,424-426 -> FLMRVisionModel.forward, modeling_flmr.py:1701-1757 -> CLIPVisionTransformer):
 * patch convolution (stride = kernel, no bias) as an im2col GEMM, [class | patches] + position embedding,
 * pre_layrnorm, vit_layers pre-LN blocks with quick-GELU MLPs.  Weights: the reference state_dict keys
 * "context_vision_encoder.vision_model.vision_model.*" (required when cfg.vit_layers > 0; post_layernorm is not read).
 *   pixel_values      : DEVICE float32 [B, 3, vit_image_size, vit_image_size]
 *   image_cls_out     : DEVICE float32 [B, vision_hidden]            = last_hidden_state[:, 0] (no post_layernorm)
 *   image_patches_out : DEVICE float32 [B, n_patches, vision_hidden] = hidden_states[-2][:, 1:]
 * The outputs are exactly the image_cls / image_patches arguments of rr_forward / rr_forward_joint. */
int rr_encode_image(rr_handle h, const float* pixel_values, int B, float* image_cls_out, float* image_patches_out,
                    void* hip_stream);

/* rr_forward_joint: RerankModel.forward (the "softmax"/2-head variant, rerank_model.py:171-331) from the joint
 * sequence the caller assembled as the reference does (:204-224): joint_ids = cat(query_ids repeated K times,
 * context_ids[:, 2 : 2 - query_len]) [N,S], same for the mask.  Inside: token types 0, query_mask with instruction
 * masking (id != 0 and (pos > first instruction_token_id position or pos < 2), :481-506; instruction_token_id < 0
 * = plain id != 0), cross-encoder token order [query | image | context] (:257-274), and the reference's
 * `loss_fn(logits, logits)` (:328: labels are ignored, the loss uses the logits as targets).  Image features are
 * mandatory (NotImplementedError for text_only, :184-185).  Attention fusion: rr_forward_joint_fusion. */
int rr_forward_joint(rr_handle h, const int64_t* joint_input_ids, const int64_t* joint_attention_mask,
                     const float* image_cls, const float* image_patches, int Bq, int K, int S, int query_len,
                     int64_t instruction_token_id, int pair_begin, int pair_end, float* logits_out,
                     float* logits2_out, float* loss_out, float* scores_out, int32_t* order_out, void* hip_stream);

/* rr_forward_joint_fusion: rr_forward_joint with the PreFLMR attention fusion of RerankModel.forward
 * (`preflmr_scores`, `fusion_multiplier`; rerank_model.py:276-319, attention_fusion.py:84-102; the executor passes the
 * retriever's `scores_raw`, Reranker_base_executor.py:888-891).
 *   preflmr_scores : DEVICE float32 [N, S, query_len + prefix_len + n_patches] — context token x query/image token.
 * Rows 2 .. 2 + S - query_len of every pair (the context tokens that are in the joint sequence) give an additive
 * attention bias over the cross-encoder tokens [query | image | context] in every cross-encoder layer: query rows get
 * softmax-over-context-tokens, context rows softmax-over-query-tokens, the self blocks 0, all times fusion_multiplier. */
int rr_forward_joint_fusion(rr_handle h, const int64_t* joint_input_ids, const int64_t* joint_attention_mask,
                            const float* image_cls, const float* image_patches, const float* preflmr_scores,
                            float fusion_multiplier, int Bq, int K, int S, int query_len, int64_t instruction_token_id,
                            int pair_begin, int pair_end, float* logits_out, float* logits2_out, float* loss_out,
                            float* scores_out, int32_t* order_out, void* hip_stream);

/* rr_forward_interaction: the Interaction rerankers, fed by the frozen retriever's late-interaction outputs
 * (Reranker_base_executor.py:877-885 builds the call).  All pointers DEVICE float32:
 *   query_li [Bq, Lq, li_dim], context_li [N, Lc, li_dim], query_mask [Bq, Lq] and context_mask [N, Lc] (0/1).
 * Outputs, labels, pair slice and head semantics are those of rr_forward.  (No attention fusion here: the reference's
 * interaction executor path never passes it and MORES raises NotImplementedError for it, mores_model.py:72-73.) */
int rr_forward_interaction(rr_handle h, const float* query_li, const float* context_li, const float* query_mask,
                           const float* context_mask, int Bq, int K, int Lq, int Lc, const float* labels,
                           int pair_begin, int pair_end, float* logits_out, float* logits2_out, float* loss_out,
                           float* scores_out, int32_t* order_out, void* hip_stream);

/* rr_forward_interaction_fusion: the same with the PreFLMR attention fusion of InteractionRerankModel.forward
 * (interaction_rerank_model.py:131-142; NORMAL interaction type only, MORES raises NotImplementedError,
 * mores_model.py:72-73): preflmr_scores DEVICE float32 [N, Lc, Lq] (context token x query token) becomes the additive
 * bias [[0, softmax(scores^T)], [softmax(scores), 0]] * fusion_multiplier over the tokens [query | context]. */
int rr_forward_interaction_fusion(rr_handle h, const float* query_li, const float* context_li, const float* query_mask,
                                  const float* context_mask, const float* preflmr_scores, float fusion_multiplier, int Bq,
                                  int K, int Lq, int Lc, const float* labels, int pair_begin, int pair_end,
                                  float* logits_out, float* logits2_out, float* loss_out, float* scores_out,
                                  int32_t* order_out, void* hip_stream);

/* rr_li_scores: the retriever's own score of every pair and the matrix behind it, on the device, from the late-interaction
 * tensors rr_forward_interaction takes.  Replaces colbert_score (src/models/flmr/models/flmr/flmr_utils.py:22-48, reached through
 * FLMRModelForRetrieval.score, modeling_flmr.py:932-936,1601-1602), whose second return value the executor hands to the
 * rerankers as retrieval_results.scores_raw -> preflmr_scores (Reranker_base_executor.py:877-891).  Any model kind: the joint
 * family calls it with Lq = query_len + prefix_len + n_patches and Lc = S and passes the result to rr_forward_joint_fusion.
 *   query_li [Bq, Lq, li_dim], context_li [N, Lc, li_dim], context_mask [N, Lc] (any 0/1 pattern) : DEVICE float32, N = Bq * K;
 *       query_li / context_li 16-byte aligned (RR_ERR_BAD_ARG).  No query mask: the reference sums over every query token.
 *   scores_out : DEVICE float32 [N, Lc, Lq] or NULL.  scores[p][c][j] = dot(context_li[p][c], query_li[p / K][j]) in exact
 *       float32 (one fmaf chain over li_dim per entry, the same chain whatever the slice or shape), and -9999.0f on every row c
 *       with context_mask[p][c] == 0, whatever that row's embedding holds (the reference assigns, NaN / inf included).
 *   maxsim_out : DEVICE float32 [N] or NULL.  maxsim[p] = sum over j of max over c of scores[p][c][j], columns added in
 *       ascending order by one thread: the same bits on every run, with and without scores_out.  A NaN in an unmasked row makes
 *       its pair's maxsim NaN (torch.max semantics); a fully masked pair gives -9999 * Lq.
 *   pair_begin / pair_end : only rows [pair_begin, pair_end) of the outputs are written.  K = 1 is the per-pair form.
 * At least one output (RR_ERR_BAD_ARG); null inputs RR_ERR_BAD_ARG; non-positive sizes or a slice outside [0, Bq * K)
 * RR_ERR_BAD_SHAPE; all before anything is enqueued.  Without scores_out nothing of size [N, Lc, Lq] is written anywhere.
 * Allocates nothing, capturable into a graph.  Python: RerankEngine.li_scores. */
int rr_li_scores(rr_handle h, const float* query_li, const float* context_li, const float* context_mask, int Bq, int K, int Lq,
                 int Lc, int pair_begin, int pair_end, float* scores_out, float* maxsim_out, void* hip_stream);

/* rr_forward_interaction_fusion_li: rr_forward_interaction_fusion without preflmr_scores: the scores of the slice are computed
 * from query_li / context_li / context_mask as rr_li_scores computes them (flmr_utils.py:22-48) into a block of the handle
 * ([n, Lc, Lq]; rr_reserve with_fusion = 2 covers it), and the forward continues as rr_forward_interaction_fusion does on that
 * block: logits bit for bit those of rr_forward_interaction_fusion(preflmr_scores = rr_li_scores(...)).
 *   maxsim_out : DEVICE float32 [N] or NULL: the retriever's MaxSim of the pairs of the slice (only those are written).
 * MORES handles: RR_ERR_UNSUPPORTED (mores_model.py:72-73), before anything is enqueued.
 * Python: RerankEngine.forward_interaction(fusion_from_li=True). */
int rr_forward_interaction_fusion_li(rr_handle h, const float* query_li, const float* context_li, const float* query_mask,
                                     const float* context_mask, float fusion_multiplier, int Bq, int K, int Lq, int Lc,
                                     const float* labels, int pair_begin, int pair_end, float* logits_out, float* logits2_out,
                                     float* loss_out, float* scores_out, int32_t* order_out, float* maxsim_out, void* hip_stream);

/* rr_head: scoring head + loss + top-K order over complete logits [Bq*K] (after the RCCL
 * all-gather of per-rank slices).  Same semantics as the tail of rr_forward. */
int rr_head(rr_handle h, const float* logits, const float* logits2, const float* labels, int Bq, int K,
            float* loss_out, float* scores_out, int32_t* order_out, void* hip_stream);

/* rr_forward_joint_packed / rr_forward_interaction_packed: rr_forward_joint(_fusion) and rr_forward_interaction(_fusion) over
 * PACKED rows, with the conventions of rr_forward_packed: the caller groups the pairs into n_segments (1..64) segments of equal
 * length seg_len[i] (every pair's non-pad positions must fit it), hands over the per-pair tensors segment after segment and,
 * inside a segment, pair after pair at THAT length, and gets logits_out (/ logits2_out) DEVICE float32 [n] in that packed pair
 * order back; it scatters them and runs the head (rr_head_joint / rr_head) on the [Bq, K] block.  Per-query tensors are handed
 * over PER PAIR in packed order.  preflmr_scores (NULL = no attention fusion) stays PADDED along the context axis, in packed
 * pair order: the reference's softmax over the context tokens runs over the whole padded axis (rerank_model.py:305,
 * interaction_rerank_model.py:134), so the bias of a shorter pair still needs the scores of its pad positions.
 * For rr_reserve count n_queries = n_pairs; with_fusion covers the packed bias.  No reference counterpart (it pads).
 * RR_ERR_BAD_SHAPE: more than 64 segments, an empty segment, a length above the padded length.
 *
 * rr_forward_joint_packed (Python: RerankEngine.forward_joint_packed):
 *   joint_input_ids / joint_attention_mask : DEVICE int64, sum_i seg_pairs[i] * seg_len[i] entries, the first seg_len[i]
 *       columns of the [query_len | context] joint sequence rr_forward_joint takes (padded_seq_len columns there);
 *   image_cls / image_patches : DEVICE float32 [n, vision_hidden] / [n, n_patches, vision_hidden] (mandatory, as for
 *       rr_forward_joint);
 *   preflmr_scores : DEVICE float32 [n, padded_seq_len - query_len, query_len + prefix_len + n_patches] — the context rows
 *       (2 .. 2 + padded_seq_len - query_len) of rr_forward_joint_fusion's scores.
 *   Every seg_len[i] must exceed query_len (the whole query part is kept) and reach the mapping network's cross-attention
 *   window min(padded_seq_len, 32) (RR_ERR_BAD_SHAPE).  The joint sequence [query | image | context] is padded at its end,
 *   so no position moves, and the text encoder, the masks, the fusion bias and the cross encoder compute what the padded call
 *   computes for every pair.  NOT bit for bit in general: image features are per pair here, so the mapping network's first
 *   layer runs its GEMMs over n instead of Bq queries' rows, and a GEMM of another row count may run other tile shapes with
 *   another fp32 summation order (as in rr_forward_packed with vision tokens).  Measured with "resid_split" = 0: bit for bit
 *   on the 6-pair fixtures, 9.8e-5 (1.6e-4 with fusion) at 200 pairs of the c3 geometry — within the 1e-3 parity gate
 *   (tests/test_gpu_packed_families.py).
 * rr_forward_interaction_packed (Python: RerankEngine.forward_interaction_packed), NORMAL and MORES handles:
 *   query_li [n, Lq, li_dim], query_mask [n, Lq] : DEVICE float32 per pair;
 *   context_li [sum seg_pairs[i] * seg_len[i], li_dim], context_mask [sum seg_pairs[i] * seg_len[i]] : DEVICE float32, the
 *       first seg_len[i] context tokens of every pair;
 *   preflmr_scores : DEVICE float32 [n, padded_context_len, Lq] (NORMAL only: MORES returns RR_ERR_UNSUPPORTED as
 *       rr_forward_interaction_fusion does, mores_model.py:72-73).
 *   NORMAL: Lq + padded_context_len must not exceed ce_max_pos (RR_ERR_BAD_SHAPE).  MORES: the query side keeps its n * Lq
 *   rows; the doc-side Linear, every layer's K / V projection and the cross-attention (per segment, Tk = seg_len) run over the
 *   packed doc rows.  A pair's logits equal rr_forward_interaction(_fusion)'s for it BIT FOR BIT, NORMAL with and without
 *   fusion and MORES, while "resid_split" = 0 (or both calls are on the same side of its row-count rule): padding sits at the
 *   end of [query | context], no position moves, the attention of a packed call runs the schedule the padded call's grid
 *   selects, and a fusion bias always runs the online form, as in the padded call (tests/test_gpu_packed_families.py: the
 *   fixtures and 200 pairs of the int_base geometry). */
int rr_forward_joint_packed(rr_handle h, const int64_t* joint_input_ids, const int64_t* joint_attention_mask,
                            const float* image_cls, const float* image_patches, const float* preflmr_scores,
                            float fusion_multiplier, int n_segments, const int32_t* seg_pairs, const int32_t* seg_len,
                            int padded_seq_len, int query_len, int64_t instruction_token_id,
                            float* logits_out, float* logits2_out, void* hip_stream);
int rr_forward_interaction_packed(rr_handle h, const float* query_li, const float* context_li, const float* query_mask,
                                  const float* context_mask, const float* preflmr_scores, float fusion_multiplier,
                                  int n_segments, const int32_t* seg_pairs, const int32_t* seg_len, int padded_context_len,
                                  int Lq, float* logits_out, float* logits2_out, void* hip_stream);
/* rr_forward_interaction_packed_fusion_li: rr_forward_interaction_packed with the attention fusion computed from the packed
 * tensors themselves (rr_forward_interaction_fusion_li; flmr_utils.py:22-48), so nothing padded is handed over any more: the
 * positions of a pair beyond its seg_len[i] are pad positions, i.e. masked rows (-9999) of the padded score matrix the library
 * builds in its own block [n, padded_context_len, Lq], and the bias is the one the padded call builds, bit for bit, normalisers
 * over the padded axis included.  maxsim_out : DEVICE float32 [n] in packed pair order, or NULL.  NORMAL handles only (MORES:
 * RR_ERR_UNSUPPORTED).  Python: RerankEngine.forward_interaction_packed(fusion_from_li=True). */
int rr_forward_interaction_packed_fusion_li(rr_handle h, const float* query_li, const float* context_li, const float* query_mask,
                                            const float* context_mask, float fusion_multiplier, int n_segments,
                                            const int32_t* seg_pairs, const int32_t* seg_len, int padded_context_len, int Lq,
                                            float* logits_out, float* logits2_out, float* maxsim_out, void* hip_stream);

/* ---- Passage-embedding bank of the interaction rerankers.  They rerank from embeddings that already exist: the frozen retriever's
 * context token embeddings, which the reference hands over in fp16 (`D = D.half()`, modeling_flmr.py:1554-1555).  A bank keeps
 * them on the device in that form, each passage at its own length, so that a forward names passages by index instead of taking a
 * padded float32 context_li [N, Lc, li_dim] per call.  Passages are appended, and removed in place (rr_bank_remove, REMOVING
 * PASSAGES below); the rows always lie back to back: per passage rows [len, li_dim] as fp16, one mask byte per row, and a host-side
 * table (first row as int64, length).  No reference counterpart (it recomputes or reloads the embeddings per batch).
 * Python: rmr_amd.PassageBank, RerankEngine.create_bank / forward_interaction_bank.
 *
 * rr_bank_create: a bank of capacity_rows rows and at most max_passages passages on h's device with h's li_dim (a multiple of 8,
 * at most 512: RR_ERR_UNSUPPORTED otherwise; interaction handles only).  Its lifetime is its own — rr_destroy(h) does not free it,
 * rr_bank_destroy does (it synchronises the device) — and every handle of that device with the same li_dim may use it: one bank
 * serves a NORMAL and a MORES handle.  RR_ERR_OOM when the device allocation fails (message: rr_last_error(h)).  A bank is not
 * thread-safe, and the stream order is the caller's: a forward reads what the rr_bank_add calls enqueued before it on the same
 * stream (or on a stream it has been ordered behind) wrote.
 * rr_bank_clear forgets every passage (capacity kept; forwards still in flight must have completed).  rr_bank_info: passages held,
 * rows used, row capacity (any pointer may be NULL).  rr_bank_last_error: the message of the last failed rr_bank_* call on b. */
typedef struct rr_bank* rr_bank_handle;
int rr_bank_create(rr_handle h, int64_t capacity_rows, int32_t max_passages, rr_bank_handle* out);
int rr_bank_destroy(rr_bank_handle b);
int rr_bank_clear(rr_bank_handle b);
const char* rr_bank_last_error(rr_bank_handle b);
int rr_bank_info(rr_bank_handle b, int32_t* passages_out, int64_t* rows_used_out, int64_t* capacity_rows_out);
/* rr_bank_add: append n passages from the padded tensors a retriever produces.
 *   context_li   : DEVICE [n, Lc, li_dim], float32 (dtype RR_F32) or fp16 bits (RR_F16), 16-byte aligned
 *   context_mask : DEVICE float32 [n, Lc]
 *   lengths      : HOST int32 [n], 1 <= lengths[i] <= Lc: passage i keeps rows 0 .. lengths[i] - 1 (everything behind its last
 *                  unmasked token may go; a passage without an unmasked token has length 1)
 * Values are rounded to fp16, round to nearest even — what .half() gives; fp16 input is copied.  The mask byte of a kept row is
 * (mask != 0); rows at or beyond the length count as masked in every forward.  Interior zeros of the mask (punctuation on the
 * retriever's skiplist) are kept and no position moves.  The passages get the dense indices *first_index_out .. + n - 1
 * (first_index_out may be NULL).  The call appends all n passages or refuses before anything is enqueued and leaves the bank
 * unchanged: RR_ERR_BAD_SHAPE for a length outside [1, Lc], RR_ERR_OOM when the rows or the passage slots do not suffice,
 * RR_ERR_BAD_DTYPE for another dtype.  The library stages the (first row, length) table itself: enqueued on hip_stream, not
 * capturable into a graph (RR_ERR_BAD_ARG under stream capture). */
int rr_bank_add(rr_bank_handle b, const void* context_li, int dtype, const float* context_mask, const int32_t* lengths, int n, int Lc,
                int32_t* first_index_out, void* hip_stream);
/* ---- Compressed bank: the rows as a ColBERTv2 / PLAID index stores them (one int32 centroid code and li_dim * nbits / 8 bytes of
 * bucketised residual per token, third_party/ColBERT/colbert/indexing/index_saver.py:33-46; every reference config builds its index
 * with "nbits": 8), decoded on the device inside the gather of rr_forward_interaction_bank.  Replaces the reference's own native
 * kernel on the retriever-to-reranker hand-over (third_party/ColBERT/colbert/indexing/codecs/decompress_residuals.cu) and the
 * F.normalize behind it (codecs/residual.py:242-278).  Bytes per token at li_dim 128: 257 as fp16, 133 / 69 / 37 / 21 at nbits 8 /
 * 4 / 2 / 1.  Nothing here computes embeddings; rr_plaid_kmeans and rr_plaid_residuals (below) train the codec's tables from
 * embeddings on the device; rr_bank_add_compress compresses embeddings
 * that are on the device against the codec's tables; rr_bank_search searches exhaustively;
 * rr_bank_search_plaid runs PLAID's candidate generation and centroid pruning over the codes a compressed bank holds.
 *
 * THE DECODED ROW, for a row with code c, residual bytes r[0 .. D * nbits / 8), centroids [C, D] fp16 (the index stores them with
 * .half(), residual.py:161) and float32 bucket weights w[2^nbits]:
 *   element e lies in byte j = e / (8 / nbits), group g = e % (8 / nbits) counted from the MOST significant end;
 *   x = (r[j] >> (8 - nbits * (g + 1))) & (2^nbits - 1); bucket = x with its nbits bits reversed (binarize writes the bucket's bit
 *   0 first and np.packbits fills bytes MSB-first, residual.py:188-204; reversed_bit_map and decompression_lookup_table, :51-95,
 *   undo exactly that);
 *   s_e = float(centroid[c][e]) + w[bucket], one float32 add;
 *   n = sqrtf(sum_e s_e^2) in float32, summed in ONE fixed order: per chunk of 8 consecutive elements an fmaf chain from zero,
 *   element 0 first (q = fmaf(s_0, s_0, 0); q = fmaf(s_k, s_k, q), k = 1..7), then the D / 8 chunk sums added as a pairwise tree over
 *   neighbours (q_0 + q_1, q_2 + q_3, ...; again on the results, until one is left);
 *   y_e = fp16_rne(s_e / fmaxf(n, 1e-12f)), square root and divide correctly rounded.
 * That is the reference's CPU branch (residual.py:264-275) followed by the .half() the bank applies to everything it keeps.  The
 * gather rounds to fp16 FIRST and then converts fp16 -> float32 -> the handle's operand type as it does for an fp16 bank's rows:
 * a compressed bank is bit for bit an fp16 bank that holds the decoded rows, on fp16 and bf16 handles and in the float32 copies of
 * the attention fusion.  rr_util_plaid_decode_rows (rerank_mi355_diag.h) is this definition in host code.
 *
 * rr_bank_create_plaid: rr_bank_create for compressed rows.  nbits in {1, 2, 4, 8}; h's li_dim a power of two in [8, 512] and a
 * multiple of 8 * nbits (the reference asserts that, residual.py:195): RR_ERR_UNSUPPORTED otherwise.
 *   centroids_f16  : HOST [n_centroids, li_dim] fp16 bits (centroids.pt)
 *   bucket_weights : HOST float32 [2^nbits]        (the second tensor of buckets.pt)
 * Both are copied to the device before the call returns; per row of capacity the bank allocates the code, the residual bytes and
 * the mask byte.  Everything rr_bank_create says about lifetime, sharing between handles and thread safety holds.
 * rr_bank_add_plaid: append n passages, rows concatenated passage after passage as the index stores them, R = sum lengths.
 *   codes     : HOST int32 [R]                       residuals : HOST uint8 [R, li_dim * nbits / 8]
 *   mask      : HOST uint8 [R], or NULL = all ones (the ColBERT indexer has dropped the skiplist tokens already)
 *   lengths   : HOST int32 [n], every length >= 1 (doclens)
 * Checked on the host before anything is enqueued, a refused call leaves the bank unchanged: every length >= 1 and every code in
 * [0, n_centroids) (RR_ERR_BAD_SHAPE), the row and the passage capacity (RR_ERR_OOM).  A LOAD-TIME call: it copies from the
 * caller's host memory on hip_stream and synchronises that stream, so the host buffers may be reused when it returns; not
 * capturable into a graph (RR_ERR_BAD_ARG under stream capture).  An inverted file the bank holds (THE INVERTED FILE, below) does
 * not cover the new passages until rr_bank_extend_ivf is called.
 * rr_bank_format: nbits (0 for an fp16 bank), the number of centroids (0; an fp16 bank with a centroid table, rr_bank_set_centroids
 * below: its number) and the device bytes one row takes (mask byte included);
 * any pointer may be NULL.
 * The two formats do not mix: rr_bank_add on a compressed bank and rr_bank_add_plaid on an fp16 bank return RR_ERR_UNSUPPORTED.
 * rr_bank_clear / rr_bank_info / rr_bank_destroy / rr_bank_read and rr_forward_interaction_bank take either kind unchanged.
 * Python: rmr_amd.PlaidCodec, RerankEngine.create_bank(codec=...), PassageBank.add_compressed / load_plaid_index,
 * rmr_amd.read_plaid_index. */
int rr_bank_create_plaid(rr_handle h, int64_t capacity_rows, int32_t max_passages, int nbits, int32_t n_centroids,
                         const uint16_t* centroids_f16, const float* bucket_weights, rr_bank_handle* out);
int rr_bank_add_plaid(rr_bank_handle b, const int32_t* codes, const uint8_t* residuals, const uint8_t* mask, const int32_t* lengths,
                      int n, int32_t* first_index_out, void* hip_stream);
int rr_bank_format(rr_bank_handle b, int32_t* nbits_out, int32_t* n_centroids_out, int64_t* bytes_per_row_out);
/* ---- Compressing embeddings into a compressed bank on the device: what the reference's indexer does with
 * ResidualCodec.compress (third_party/ColBERT/colbert/indexing/codecs/residual.py:169-221, CPU branch), from the padded tensors a
 * retriever produces, without the [centroids x rows] score matrix that code materialises and without a host round trip.
 *
 * THE COMPRESSED ROW, for one kept row with input values v[0 .. D), centroids [C, D] fp16 and cutoffs[0 .. 2^nbits - 1):
 *   1. x_e = fp16_rne(v_e): what .half() gives, what rr_bank_add stores and what the reference's indexer is handed; fp16 input
 *      is taken as is.  Everything below uses float32(x_e).
 *   2. S[c], the score against centroid c, is the float32 fmaf chain rr_li_scores computes for the context row float32(centroid c)
 *      against the query column x: acc = fmaf(a_d, b_d, acc) from 0, d in the order t outer (steps of 16), e in 0..3, g in 0..3,
 *      d = 16 t + 4 g + e (one v_mfma_f32_16x16x4_f32 after another).  Bit for bit the scores_out entry of rr_op_li_scores, and
 *      stage 0 of rr_bank_search_plaid, for that (centroid, column).
 *   3. code = the centroid with the largest rank key of (S[c], c), the order of the bank searches: a NaN score wins, otherwise the
 *      highest score, and on equal scores (+0 == -0) the LOWEST centroid index.  Deterministic from run to run and independent of
 *      how the centroid range is divided among waves and workgroups (no atomics).
 *   4. r_e = float32(x_e) - float32(centroid[code][e]), one float32 subtraction; bucket_e = the number of cutoffs strictly below
 *      r_e.  Every comparison with a NaN is false: a NaN residual has bucket 0 (torch.bucketize places a NaN differently; no
 *      index holds one).
 *   5. Packing is the inverse of THE DECODED ROW above: element e goes to byte e / (8 / nbits), group e % (8 / nbits) counted from
 *      the most significant end, the bucket's nbits bits reversed.
 *   6. Mask and positions exactly as rr_bank_add: a passage keeps rows 0 .. len - 1, the mask byte is (mask != 0), interior masked
 *      rows are kept and compressed like any other row, no position moves.
 * rr_util_plaid_compress_rows (rerank_mi355_diag.h) is this definition in host code.
 *
 * rr_bank_set_plaid_cutoffs: the codec's bucket cutoffs (the FIRST tensor of buckets.pt), HOST float32 [2^nbits - 1], copied to the
 * device before the call returns.  RR_ERR_UNSUPPORTED on an fp16 bank, RR_ERR_BAD_SHAPE for a NaN or a decreasing sequence (equal
 * neighbours are allowed).  May be called again (it then synchronises the device); the new cutoffs apply to later adds only.
 * rr_bank_add_compress: rr_bank_add for a compressed bank: the same arguments with the same meaning, alignment, admission rules,
 * staging and graph-capture refusal.  On success all n passages are appended; a refused call leaves the bank unchanged, and
 * every refusal comes from the host before anything is enqueued: RR_ERR_UNSUPPORTED on an fp16 bank (use rr_bank_add), without
 * cutoffs, and for an li_dim that is not a multiple of 16 (the matrix-core step; li_dim 8, which a compressed bank otherwise
 * takes, is out); the rest as rr_bank_add.  It enqueues on hip_stream and does not synchronise, except when the bank's scratch
 * (8 bytes per kept row of the call, times 1 + the number of centroid splits; grow-only) has to grow: then it synchronises the
 * device once.  Two adds of one bank in flight on different streams would share that scratch: order them.  As after
 * rr_bank_add_plaid, an inverted file covers the new passages only after rr_bank_extend_ivf (on the same stream, or behind the add).
 * rr_bank_add on a compressed bank still refuses.  Python: PlaidCodec(bucket_cutoffs=...), PassageBank.add_compress. */
int rr_bank_set_plaid_cutoffs(rr_bank_handle b, const float* cutoffs_host);
int rr_bank_add_compress(rr_bank_handle b, const void* context_li, int dtype, const float* context_mask, const int32_t* lengths, int n,
                         int Lc, int32_t* first_index_out, void* hip_stream);
/* ---- An fp16 bank with a centroid table: a "coded" fp16 bank.  The pruned searches and the inverted file read one centroid code
 * per row, the centroid table, the mask bytes and the passage table; their last stage is the exact score, which an fp16 bank
 * defines on its own rows.  rr_bank_set_centroids gives an fp16 bank the table and the code per row; the bank keeps its fp16 rows,
 * and every entry that reads them (rr_bank_read, rr_bank_li_scores, rr_bank_search and its filtered forms,
 * rr_forward_interaction_bank) gives the bits it gave before.
 *   centroids_f16_host : HOST fp16 bits [n_centroids, li_dim] (PlaidCodec.train's table, or any other)
 *   n_centroids        : 1 .. 262144 (RR_ERR_BAD_SHAPE outside; the limit of the pruned search)
 * RR_ERR_UNSUPPORTED on a compressed bank (its codes belong to its residuals) and for an li_dim that is not a multiple of 16 (the
 * matrix-core step of the assignment and of stage 0).  A LOAD-TIME call: it synchronises the device (adds on any stream have
 * written their rows), allocates 4 bytes per row of capacity and the table, copies the table, assigns a code to every row the
 * bank holds now (in launches of at most 2^20 rows, 64-bit row offsets; their scratch follows rr_bank_add_compress's grow-only
 * rule) and synchronises hip_stream.  RR_ERR_BAD_ARG under stream capture.  A refusal or a failed allocation leaves the bank as
 * it was (RR_ERR_OOM).  Called again it replaces the table and assigns every row anew (centroids retrained after the bank has
 * grown), and it drops an inverted file the bank holds, whose lists name the old codes.
 * THE CODE OF A ROW is THE COMPRESSED ROW steps 2 - 3 with x = the stored fp16 row: the same rank key, the same tie rule, the
 * same independence of how the centroid range is split (rr_set_tuning("compress_chunk")); interior masked rows get a code like any
 * other row.  So for equal input the codes are bit for bit those rr_bank_add_compress writes into a compressed bank of the same
 * table, whatever its nbits and cutoffs.
 * On a coded bank rr_bank_add ingests as before and assigns the codes of the new rows behind the ingest on the same stream
 * (the assignment kernel of rr_bank_add_compress with a codes-only ending: its 64-bit key per row and centroid split is the only
 * intermediate, no residual is formed or written); admission, refusal before the first enqueue and the capture refusal are unchanged, and the
 * scratch grows as rr_bank_add_compress's does (one device synchronisation when it has to).  rr_bank_add_compress,
 * rr_bank_add_plaid and rr_bank_set_plaid_cutoffs keep refusing an fp16 bank, coded or not.  rr_bank_format reports nbits 0,
 * n_centroids and 2 li_dim + 1 + 4 bytes per row.
 * A coded bank is taken, under the contract they have on a compressed bank, by rr_bank_search_plaid, rr_bank_search_plaid_ivf and
 * their _filtered forms (stage 3 reads the fp16 rows: bit for bit rr_bank_search's score on this bank), rr_bank_build_ivf,
 * rr_bank_extend_ivf, rr_bank_ivf_info, rr_bank_ivf_read, rr_bank_load_ivf, rr_bank_remove (rows, codes and mask bytes move
 * together) and rr_bank_clear (the table stays).  rr_bank_export_plaid and rr_bank_read_plaid (rerank_mi355_diag.h) refuse it with
 * RR_ERR_UNSUPPORTED: there are no residuals; rr_bank_read_codes there reads the codes.  An fp16 bank WITHOUT a table behaves in
 * every entry as it always has.  Python: RerankEngine.create_bank(centroids=...), PassageBank.set_centroids / centroids /
 * n_centroids / codes. */
int rr_bank_set_centroids(rr_bank_handle b, const uint16_t* centroids_f16_host, int32_t n_centroids, void* hip_stream);
/* ---- Training a PLAID codec on the device: the centroid table by k-means and the residuals the bucket statistics are taken
 * from.  Replaces, in third_party/ColBERT/colbert/indexing/collection_indexer.py of the reference, train (:211-228),
 * _concatenate_and_split_sample (:230-261), _train_kmeans (:263-293), _compute_avg_residual (:295-319) and compute_faiss_kmeans
 * (:452-465).  faiss's random generator and its cluster-splitting rule cannot be reproduced, so the definition is this library's
 * own; Lloyd's algorithm with L2 distance is what faiss runs.
 *
 * THE TRAINED CENTROIDS.  Inputs: rows [R, D] float32 or fp16, C distinct initial row indices init_rows in [0, R), niters >= 0, a
 * 64-bit seed.
 *   1. Rounding.  x = fp16_rne(row), as in THE COMPRESSED ROW step 1.  Everything below uses float32(x).
 *   2. Initial table.  T [C, D] of fp16 values: T[c] = x[init_rows[c]].
 *   3. Bias.  h[c] = -0.5f * q(c), q(c) the float32 sum of squares of float32(T[c][e]) summed in the fixed order of THE DECODED
 *      ROW's norm: per chunk of 8 an fmaf chain from zero, then the pairwise tree over neighbours.
 *   4. Per iteration i = 0 .. niters - 1:
 *      Assignment.  S[c] is the fmaf chain of THE COMPRESSED ROW step 2; S'[c] = S[c] + h[c], one float32 add; code[r] is the
 *        centroid with the largest rank key of (S'[c], c): the nearest centroid in L2, equal scores going to the lowest index.
 *      Sum.  n[c] is the number of rows with code c, A[c][e] the int64 sum over those rows of fix(x[r][e]), fix(v) = clamp(v,
 *        -256, 256) * 2^24 as an integer (exact: every fp16 value is a multiple of 2^-24), fix(NaN) = 0.  Integer addition has
 *        one result in any order, so the sum is made with 64-bit vector atomics and stays deterministic.  R <= 2^30 keeps it
 *        inside int64; more rows return RR_ERR_UNSUPPORTED.
 *      Update, for n[c] > 0.  T[c][e] = fp16_rne(float32(double(A[c][e]) / double(n[c] * 2^24))): the int64 -> double
 *        conversion, the double division and double -> float32 each round to nearest even.
 *      Empty cluster, n[c] == 0.  T[c] = x[rho]: z = seed ^ ((uint64(i) << 32) | c); z += 0x9E3779B97F4A7C15;
 *        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^= z >> 31; rho = z mod R.  Each
 *        cluster computes this on the device by itself: no scan and no host round trip.
 *      Bias again.  h is recomputed from the new T.
 *      Statistics.  stats[i][0] = the number of rows whose code differs from the previous iteration's (in iteration 0: R);
 *        stats[i][1] = the number of clusters re-seeded.
 *   5. Output.  centroids_out[c][e] = fp16_rne(float32(T[c][e]) / fmaxf(norm, 1e-12f)), the norm as in THE DECODED ROW.
 *      counts = n of the last assignment, all zero when niters == 0.
 * D must be a power of two in [16, 512]: the matrix-core step needs a multiple of 16, and the pairwise tree of the norm is
 * defined for a power of two (what rr_bank_create_plaid takes anyway).
 * rr_util_plaid_kmeans (rerank_mi355_diag.h) is this definition in host code; the device equals it bit for bit, from run to run
 * and however the centroid range is split.
 *
 * rr_plaid_kmeans: D is h's li_dim.  rows [n_rows, D] (dtype RR_F32 or RR_F16, 16-byte aligned) and all outputs are DEVICE
 * pointers: centroids_f16_out [n_centroids, D] fp16 bits (16-byte aligned), counts_out int32 [n_centroids] or NULL, stats_out int32
 * [niters, 2] or NULL.  init_rows_host: HOST int32 [n_centroids].  Every refusal comes from the host before anything is enqueued,
 * with a message in rr_last_error: RR_ERR_BAD_DTYPE for another dtype, RR_ERR_UNSUPPORTED for the li_dim and for n_rows > 2^30,
 * RR_ERR_BAD_ARG for a null or misaligned pointer, for rows on another device than the handle's and under stream capture,
 * RR_ERR_BAD_SHAPE for n_centroids < 1 or > n_rows, niters < 0 and an initial index out of range or named twice.  The call
 * synchronises hip_stream once at the start (init_rows staged; the handle's grow-only training block grown) and not again: the
 * iterations are enqueued back to back.  Two training calls of one handle in flight on different streams would share that block:
 * order them.
 * rr_plaid_residuals: THE COMPRESSED ROW steps 1 - 4 without the buckets, of n_rows DEVICE rows against a finished table
 * centroids_f16 [n_centroids, D] (DEVICE, 16-byte aligned; no bias): codes_out int32 [n_rows] and residuals_out float32 [n_rows, D]
 * (r_e of step 4; 16-byte aligned), both DEVICE.  Refusals as above; it does not synchronise unless the block has to grow.
 * Python: rmr_amd.PlaidCodec.train / PlaidCodec.save, rmr_amd.plaid_num_partitions. */
int rr_plaid_kmeans(rr_handle h, const void* rows, int dtype, int64_t n_rows, const int32_t* init_rows_host, int32_t n_centroids,
                    int niters, uint64_t seed, uint16_t* centroids_f16_out, int32_t* counts_out, int32_t* stats_out, void* hip_stream);
int rr_plaid_residuals(rr_handle h, const void* rows, int dtype, int64_t n_rows, const uint16_t* centroids_f16, int32_t n_centroids,
                       int32_t* codes_out, float* residuals_out, void* hip_stream);
/* rr_forward_interaction_bank: rr_forward_interaction_packed (fusion_from_li != 0: rr_forward_interaction_packed_fusion_li) with
 * the context side taken from a bank.  NORMAL and MORES handles.
 *   query_li [n_queries, Lq, li_dim], query_mask [n_queries, Lq] : DEVICE float32, per QUERY (query_li 16-byte aligned)
 *   pair_passage, pair_query : HOST int32 [n], n = sum seg_pairs: the bank index and the query index of every pair, in the
 *       PACKED pair order (segment after segment, pair after pair).  A passage may appear in any number of pairs.
 *   n_segments / seg_pairs / seg_len / padded_context_len, logits_out / logits2_out / maxsim_out : as the packed calls take them
 *       (maxsim_out only with fusion_from_li).
 * One gather launch per segment writes the 16-bit [query | context] rows the cross encoder / the MORES stack consume (context
 * rows fp16 -> float32 -> the handle's operand type, zero beyond the passage's length; the rows of a compressed bank decoded to
 * fp16 first, see rr_bank_create_plaid) and the float mask rows; the rest of the
 * forward is the packed call's.  Without fusion nothing of size [n, Lc, li_dim] in float32 is written.  With fusion_from_li the
 * gather also writes float32 copies of the call's query and context rows into a grow-only block of the handle, which the score
 * kernel of rr_li_scores reads unchanged (cost: 4 bytes per element written and read again; the score block dominates it).
 * Checked on the host BEFORE anything is enqueued, a refused call writes nothing: bank and handle on one device (RR_ERR_BAD_ARG)
 * with one li_dim (RR_ERR_BAD_SHAPE); MORES with fusion_from_li (RR_ERR_UNSUPPORTED, mores_model.py:72-73); the segment table
 * (1..64 non-empty segments, lengths in (0, padded_context_len]); every passage index inside the bank, every passage's length <=
 * its segment's length, every query index inside n_queries (RR_ERR_BAD_SHAPE); and what rr_forward_interaction_packed checks.
 * The library stages the per-pair descriptors itself, through the slots rr_assemble_pairs uses: NOT capturable into a graph
 * (RR_ERR_BAD_ARG under stream capture).
 * CONTRACT: logits (and maxsim_out) are bit for bit those of rr_forward_interaction_packed / _packed_fusion_li called with the
 * same segment table and query_li[pair_query], query_mask[pair_query] per pair, context_li = float32(bank rows) (zero beyond a
 * passage's length) and context_mask = the bank's mask bytes.  On an fp16 handle (compute_dtype 1) that is also, bit for bit,
 * the call on the ORIGINAL float32 tensors: float32 -> fp16 happens once either way.  On a bf16 handle it is NOT: float32 -> fp16
 * -> bf16 differs from float32 -> bf16 on 3.3 - 3.5 % of the elements of unit-scale embeddings (532 of 15 360 and 13 004 of
 * 393 216 on the test fixtures; logits moved by 5e-5 .. 1e-3 there) — the reference's own fp16 hand-over rounds twice as well. */
int rr_forward_interaction_bank(rr_handle h, rr_bank_handle b, const float* query_li, const float* query_mask, int n_queries, int Lq,
                                const int32_t* pair_passage, const int32_t* pair_query, int n_segments, const int32_t* seg_pairs,
                                const int32_t* seg_len, int padded_context_len, int fusion_from_li, float fusion_multiplier,
                                float* logits_out, float* logits2_out, float* maxsim_out, void* hip_stream);

/* rr_bank_li_scores: the retriever's own score of (query, passage) pairs straight from a bank: what colbert_score returns
 * (flmr_utils.py:22-48), the [Lc, Lq] matrix and the MaxSim of every pair, i.e. rr_li_scores without the padded float32
 * context_li.  Any interaction handle of the bank's device and li_dim, NORMAL or MORES, with or without weights loaded; either
 * bank format.  li_dim must be a multiple of 16 (RR_ERR_UNSUPPORTED).
 *   query_li [n_queries, Lq, li_dim] : DEVICE float32, per QUERY, 16-byte aligned.  No query mask: the reference sums over
 *       every query token.
 *   pair_passage, pair_query : HOST int32 [n_pairs]: the bank index and the query index of every pair, in any order; a passage
 *       or a query may appear any number of times.
 *   scores_out : DEVICE float32 [n_pairs, padded_context_len, Lq] or NULL; -9999 on masked rows and on the rows at or beyond
 *       the passage's length (pad rows, which count once in the column maximum and cost no arithmetic).
 *   maxsim_out : DEVICE float32 [n_pairs] or NULL.
 * ONE launch over the pair list (one workgroup per pair), booked in the profile's `tail` class with
 * 2 * sum(len) * Lq * li_dim FLOPs.  An fp16 bank's rows are converted to float32 in the load (exact); a compressed bank's rows
 * are decoded tile by tile in LDS by the one definition of the decoded row (rr_bank_create_plaid), rounded to fp16 first: no
 * buffer of rows x li_dim is written to global memory.  Nothing is allocated beyond the descriptor staging.
 * Checked on the host BEFORE anything is enqueued, a refused call writes nothing: null handle, bank or inputs, both outputs
 * null, a misaligned query_li, bank and handle on different devices, a full-context handle (RR_ERR_BAD_ARG); a different li_dim,
 * non-positive sizes, a passage index outside the bank, a query index outside n_queries, a passage longer than
 * padded_context_len (RR_ERR_BAD_SHAPE).  The descriptors are staged through the slots rr_assemble_pairs uses: NOT capturable
 * into a graph (RR_ERR_BAD_ARG under stream capture).
 * CONTRACT: scores_out and maxsim_out are bit for bit what rr_li_scores returns when called with K = 1, query_li[pair_query]
 * per pair, context_li = float32(the bank's rows) zero-padded to padded_context_len and context_mask = the bank's mask bytes, 0
 * beyond the length.  Hence a compressed bank gives the bits of an fp16 bank holding rr_bank_read's rows, MaxSim is the same
 * with and without the score block and from run to run, and it equals the maxsim_out of
 * rr_forward_interaction_bank(fusion_from_li = 1) for the same pairs. */
int rr_bank_li_scores(rr_handle h, rr_bank_handle b, const float* query_li, int n_queries, int Lq, const int32_t* pair_passage,
                      const int32_t* pair_query, int n_pairs, int padded_context_len, float* scores_out, float* maxsim_out,
                      void* hip_stream);

/* rr_bank_search: exact top-k MaxSim search over a range of a bank: the candidates a reranker starts from, taken from the bank
 * itself.  The reference reads them from a file a separate PLAID search wrote (third_party/ColBERT/colbert/search/
 * index_storage.py:86-98: candidate generation, two centroid-score pruning passes, exact MaxSim on the ndocs / 4 survivors, sort);
 * here EVERY passage of the range is scored with what that last stage computes (colbert_score, flmr_utils.py:22-48) and the k best
 * per query are returned, so no recall is lost to pruning.  Handles, bank formats and li_dim as rr_bank_li_scores takes them.
 *   query_li [n_queries, Lq, li_dim] : DEVICE float32, 16-byte aligned; no query mask.  n_queries <= 65535.
 *   first_passage, n_passages : the bank indices first_passage .. first_passage + n_passages - 1 are searched; n_passages = -1:
 *       through the last passage.  (A rank can search its slice of a bank; rr_bank_merge_topk merges the results of ranks.)
 *   indices_out : DEVICE int32 [n_queries, k], bank indices.   scores_out : DEVICE float32 [n_queries, k], or NULL.
 *   k : 1 <= k <= min(n_passages, 1024).  A selection pass sorts slices of 4096 candidates in LDS (as rr_head's rank does) and
 *       keeps k of each: with k <= 1024 every pass shrinks the list at least fourfold, so the passes end after
 *       log4(n_passages / 4096) + 1 launches and the survivor buffers stay a quarter of the scores.  A larger k: RR_ERR_UNSUPPORTED.
 * SCORE of a passage: bit for bit the maxsim_out of rr_bank_li_scores for that (query, passage) with padded_context_len = the
 * passage's own length.  A larger padded_context_len adds rows of -9999 to every column maximum, which changes the value only
 * if every unmasked score of a column is below -9999: impossible for unit rows (|score| <= 1), so for those the score is the
 * maxsim_out at ANY padded_context_len.  A fully masked passage scores the sum of Lq times -9999.  A compressed bank gives the
 * bits of the fp16 bank of its decoded rows.
 * ORDER per query: that of torch.sort(scores, descending=True, stable=True) truncated to k: higher score first, equal scores
 * (+0 == -0) by ascending bank index, NaN ahead of every number (NaNs among themselves by index); the same from run to run.
 * Two kernels, booked in the profile's `tail` class: one scoring launch over (passage chunk, query) with 2 * sum(len) * Lq *
 * li_dim FLOPs per query (a workgroup stages its query block once and walks a chunk of passages, a wave per passage), then the
 * selection passes (no atomics).  One float per (query, passage) and the survivor indices live in a grow-only block of the
 * handle: 4 * n_queries * n_passages * (1 + k / 2048) bytes.  The bank keeps a device copy of its passage table for this call (16 bytes per passage), brought up to
 * date by the first search after an rr_bank_add / rr_bank_add_plaid / rr_bank_clear: THAT search uploads the new entries and
 * synchronises hip_stream once.
 * Checked on the host BEFORE anything is enqueued, a refused call writes nothing: null handle, bank, query_li or indices_out,
 * misaligned pointers, bank and handle on different devices, a full-context handle (RR_ERR_BAD_ARG); a different li_dim,
 * non-positive sizes, a range that is empty or not inside the bank, k < 1 or k > n_passages (RR_ERR_BAD_SHAPE).
 * LIMITS: k <= 1024; not capturable into a graph (RR_ERR_BAD_ARG under stream capture: the call may upload the table and grow
 * its block); one device per call (a bank split over ranks or banks: search each part and merge the k-lists with rr_bank_merge_topk below); every passage of the range competes (restrict
 * by range, by a candidate filter with rr_bank_search_filtered below, or prune by centroid with rr_bank_search_plaid).  (Python: RerankEngine.bank_search, PassageBank.search,
 * InteractionRerankModel.retrieve / retrieve_and_rerank.) */
int rr_bank_search(rr_handle h, rr_bank_handle b, const float* query_li, int n_queries, int Lq, int32_t first_passage,
                   int32_t n_passages, int k, int32_t* indices_out, float* scores_out, void* hip_stream);

/* rr_bank_search_f16: exhaustive search over a range of an FP16 bank (plain or coded) whose first pass runs on the fp16 matrix
 * core and whose survivors are rescored exactly: every returned score is rr_bank_search's score of that passage bit for bit, and
 * certified_out says per query whether the k results are PROVABLY rr_bank_search's.  PLAID's shape (approximate, then exact)
 * without centroids: no recall is lost to cells.  Arguments, range, alignment, device checks, the table upload and the
 * graph-capture refusal exactly as rr_bank_search has them; scores_out may be NULL.
 *   ndocs : the survivors per query that are rescored, k <= ndocs <= 1024.   k : 1 <= k <= min(ndocs, n_passages).
 *   slack : a bound on |A - E| over the range (below), >= 0.   certified_out : DEVICE int32 [n_queries], required.
 * STAGES per query, n the passages of the range, "order" rr_bank_search's one total order (NaN first, higher score, lower index):
 *   1. A[p] for every passage: its MaxSim with the query rounded once to fp16 (round to nearest even) and the fp16 rows as they
 *      lie in the bank, accumulated by v_mfma_f32_16x16x32_f16 (csrc/bank_search_f16.hip: a workgroup owns a chunk of passages and
 *      a block of queries, so a row is read from HBM once per query block, not once per query).  A product of two fp16 values is
 *      exact in float32: only the query's rounding and the accumulation differ from the exact score E[p].
 *   2. the first m = min(ndocs, n) passages in order over A: the survivors.
 *   3. E of every survivor: the listed form of rr_bank_search's scoring kernel, hence its bits.
 *   4. the first k survivors in order over (E, bank index): indices_out = bank indices, scores_out = E.
 *   5. certified_out = 1 if m == n; else 1 iff score_k and a* are not NaN and score_k > a* + slack (a float32 sum), score_k the
 *      k-th returned score and a* = A of the last survivor.  (An exact score of -inf is absent, as in the pruned searches: -1 /
 *      -inf at the end of the list, and the query is not certified.)
 * PROOF.  A passage outside the survivors has A <= a*.  If slack bounds |A - E| over the range, its E <= a* + slack < score_k:
 * strictly below the k-th result.  The survivors hold every passage that can rank among the first k, stage 4 orders them as
 * rr_bank_search does, so indices_out and scores_out are rr_bank_search's bytes.  A query that is not certified still gets exact
 * scores of real passages, in order: the best k among its ndocs approximately best.
 * SLACK.  The bound it stands for: |A - E| <= sum_j ||q_j||2 * R * (2^-11 + D * 2^-22) + Lq * 2^-22 * |E| + Lq * sqrt(D) * 2^-25 * R,
 * R the largest row norm (<= 1 + 2^-10 for unit rows stored as fp16), FOR QUERY ELEMENTS BELOW 65520 IN MAGNITUDE.  2^-11 is the
 * query's rounding to fp16 (relative, per element: derivable) inside fp16's normal range; below 2^-14 the error of an element is
 * absolute, at most 2^-25 (half the subnormal spacing), so ||q_j - fp16(q_j)|| <= 2^-11 ||q_j|| + sqrt(D) * 2^-25: the last term,
 * without which a query of elements below 2^-25 (all zero in fp16) was certified falsely.  An element of magnitude >= 65520
 * rounds to infinity: NO finite slack bounds |A - E| then, and a caller that certifies such queries must pass +inf (accepted:
 * the query is certified only when every passage of the range is rescored, m == n).  D * 2^-24
 * would cover ANY order of float32 additions of the exact products under round to nearest; the matrix core's internal order and
 * rounding are not documented, so the constant is 4 times that, and how far the hardware stays under it is MEASURED
 * (tests/test_gpu_bank_search_f16.py, tests/test_gpu_bank_f16_forms.py, profiles/bank_f16_parity_margins.json).  Lq * 2^-22 * |E| is
 * the column sum.  Python's default (F16Search(slack=None)) evaluates the bound with R = 1 + 2^-10 and |E| <= sum_j ||q_j||2 * R,
 * maximised over the call's queries, and is +inf when an element of the call's queries is infinite or >= 65520 in magnitude.
 * SCRATCH in the grow-only block rr_bank_search uses, each term rounded up to 16 bytes: A and E (4 n_queries n each), the two
 * survivor buffers of the selection (4 n_queries ceil(n / 4096) m each, none for n <= 4096), the survivors (4 n_queries m), two
 * counts (4 n_queries each) and, without scores_out, 4 n_queries k: at most 4 n_queries n (2 + ndocs / 2048) + O(n_queries ndocs).
 * Five launches (one more per further selection pass above 4096 passages) and one memset, booked in the profile's `tail` class; no atomics: the same bytes from run to run.
 * REFUSED before anything is enqueued, nothing written: what rr_bank_search refuses, a null certified_out, a NaN or negative slack
 * (RR_ERR_BAD_ARG); k < 1, k > ndocs, k > n_passages (RR_ERR_BAD_SHAPE); ndocs > 1024, a compressed bank (its exhaustive search
 * is bound by the decode, not by the matrix core: this entry's first pass reads fp16 rows; rr_bank_search_f16_plaid below decodes a
 * row once per query block and takes compressed banks), li_dim not a multiple of 32 (RR_ERR_UNSUPPORTED).
 * WHICH TO USE: profiles/README.md "bank_search_f16_bench".  (Python: RerankEngine.bank_search_f16, PassageBank.search(fast=F16Search(ndocs)).) */
int rr_bank_search_f16(rr_handle h, rr_bank_handle b, const float* query_li, int n_queries, int Lq, int32_t first_passage,
                       int32_t n_passages, int ndocs, int k, float slack, int32_t* indices_out, float* scores_out,
                       int32_t* certified_out, void* hip_stream);

/* rr_bank_search_f16_plaid: rr_bank_search_f16 over a range of a COMPRESSED bank.  Arguments, stages 1 - 5, the certificate and its
 * proof, SLACK, SCRATCH, the launches and the graph-capture refusal are rr_bank_search_f16's, word for word.  ITS RESULTS ARE THOSE
 * OF rr_bank_search_f16 ON THE FP16 BANK THAT HOLDS THE DECODED ROWS, BYTE FOR BYTE, certified_out included; every returned score is
 * rr_bank_search's score of that passage on the compressed bank, and a certified row is rr_bank_search's row on it.
 *   Stage 1 (csrc/bank_search_f16_plaid.hip): a wave decodes the two 16-row tiles it is about to multiply into an LDS tile of its
 * own (THE DECODED ROW, "a compressed bank is bit for bit an fp16 bank that holds the decoded rows": a decoded row IS fp16) and
 * feeds them to v_mfma_f32_16x16x32_f16 in the order of the fp16 kernel: equal operand bits, the same instruction chain, so A is the
 * fp16 entry's A over the decoded rows bit for bit, and the slack bound with its measured accumulation constant
 * (profiles/bank_f16_parity_margins.json) stands without a new measurement.  A row is decoded once per QUERY BLOCK (4 queries at
 * Lq 32), not once per query as rr_bank_search decodes it.  Stage 3 is the listed form of rr_bank_search's kernel on the compressed
 * rows.  A decoded row's norm is within the R = 1 + 2^-10 that Python's default slack assumes.
 * REFUSED before anything is enqueued, nothing written: what rr_bank_search_f16 refuses, but an fp16 bank, plain or coded, in place
 * of a compressed one (RR_ERR_UNSUPPORTED: rr_bank_search_f16 is the entry for it), and li_dim other than 32, 64, 128 or 256
 * (RR_ERR_UNSUPPORTED: the four decoded tiles [32][li_dim + 16] fp16 of a workgroup take 132 KB of LDS at li_dim 512 and leave no
 * room for a query block).  rr_set_tuning("f16_stop_after") applies to both entries.
 * WHICH TO USE: profiles/README.md "bank_search_f16_plaid_bench".  (Python: RerankEngine.bank_search_f16_plaid; PassageBank.search(
 * fast=F16Search(ndocs)) picks the entry by the bank's format.) */
int rr_bank_search_f16_plaid(rr_handle h, rr_bank_handle b, const float* query_li, int n_queries, int Lq, int32_t first_passage,
                             int32_t n_passages, int ndocs, int k, float slack, int32_t* indices_out, float* scores_out,
                             int32_t* certified_out, void* hip_stream);

/* rr_bank_search_plaid: PLAID's staged, centroid-pruned top-k search over a range of a COMPRESSED bank (the reference:
 * third_party/ColBERT/colbert/search/index_storage.py:86-184, candidate_generation.py, filter_pids.cpp), from what the bank holds
 * already: a centroid code per row, the fp16 centroid table, the passage table.  This entry reads no IVF (rr_bank_search_plaid_ivf
 * below does, with the same result): the candidate set the
 * reference reads from its IVF (per centroid the passages holding a token with that code: _build_ivf, indexing/
 * collection_indexer.py:393-431, sorts the embedding ids by code and counts them per centroid; optimize_ivf, indexing/utils.py:8-48,
 * maps every embedding id to its passage and keeps the unique passages of each centroid) comes from one scan over the codes of
 * the range.  An fp16 bank without a centroid table (rr_bank_set_centroids): RR_ERR_UNSUPPORTED; with one, stage 3 reads its
 * fp16 rows.  Handles, li_dim, query_li,
 * first_passage / n_passages, alignment, device checks and the graph-capture refusal exactly as rr_bank_search has them.
 *   Lq_coarse : 1 <= Lq_coarse <= Lq (RR_ERR_BAD_SHAPE): stages 0-2 use the first Lq_coarse query tokens, the exact stage all Lq
 *       (the reference cuts the query to query_maxlen for the approximate stages, index_storage.py:77).
 *   ncells    : 1 <= ncells <= n_centroids (RR_ERR_BAD_SHAPE), at most 16 (RR_ERR_UNSUPPORTED).
 *   ndocs     : 4 <= ndocs (RR_ERR_BAD_SHAPE) <= 1024 (RR_ERR_UNSUPPORTED: the k <= 1024 of the selection kernel).
 *   k         : 1 <= k <= min(ndocs / 4, n_passages) (RR_ERR_BAD_SHAPE).   n_centroids <= 262144 (RR_ERR_UNSUPPORTED).
 *   indices_out int32 [n_queries, k], scores_out float32 [n_queries, k] or NULL, counts_out int32 [n_queries] (required): DEVICE.
 * Per query, over the passages of the range.  "Order" is rr_bank_search's one total order: NaN first, then higher score, then
 * ascending bank index for equal scores.  -inf is the "absent" mark throughout: a passage whose score at some stage is a genuine
 * -inf counts as absent from that stage on.  Masked rows contribute nothing at any stage.
 *   STAGE 0, centroid scores: S[c][j], c < n_centroids, j < Lq_coarse, float32: bit for bit the scores_out entry rr_li_scores gives
 *     for a context row equal to float32(centroid c) against query column j (its kernel runs over the centroid table cut into
 *     pseudo-passages of 64).  The reference's GPU branch does this product in fp16, its CPU branch in float32: float32 here.
 *   CELLS: for each of the Lq_coarse columns the first ncells centroids of that column in order (get_cells,
 *     candidate_generation.py:12-20, ties made definite); the cell set of the query is their union.
 *   CANDIDATES: a passage is a candidate iff at least one of its unmasked rows has a code in the cell set.
 *   STAGE 1: keep[c] = (max_j S[c][j] >= centroid_score_threshold; a row of S holding a NaN is not kept).  A candidate scores
 *     A1 = sum_j max(-9999, max over its unmasked rows r with keep[code_r] of S[code_r][j]), columns summed 0, 1, ... Lq_coarse - 1
 *     in sequence from 0.0f in float32 (the reference's CPU definition, filter_pids.cpp:27-66; a NaN sticks in a maximum).  A
 *     candidate without a kept code scores Lq_coarse * -9999.  The first min(ndocs, candidates) candidates in order survive.
 *   STAGE 2: A2, the same sum with every keep true; the first min(ndocs / 4, survivors) in order survive.
 *   STAGE 3: the survivors are scored with all Lq columns: bit for bit the score rr_bank_search returns for (query, passage).
 *   OUTPUT: the first k in order; counts_out[q] = the number of real entries, entries behind it hold index -1 and score -inf.
 * PROPERTY: with ncells = n_centroids every passage with an unmasked row is a candidate; if also ndocs / 4 >= n_passages, the
 * result is rr_bank_search's, bit for bit (where no exact score is -inf).  The same bytes from run to run: no global atomics,
 * nothing depends on scheduling.
 * Eight launches and the selection passes (csrc/bank_search_plaid.hip), booked in the profile's `tail` class: stage 0 with 2 *
 * n_queries * ceil64(n_centroids) * Lq * li_dim FLOPs, stage 3 with 2 * n_queries * min(ndocs / 4, n) * (mean rows per passage of
 * the range) * Lq * li_dim (the survivors are counted on the device only: an upper bound).  Scratch in the grow-only block
 * rr_bank_search uses, each term rounded up to 16 bytes, Cp = ceil64(n_centroids), W = ceil(n_centroids / 32), k1 = min(ndocs, n),
 * k2 = min(ndocs / 4, n): 4 nq Cp Lq + 16 nq Cp / 64 + Cp + 4 nq Lq_coarse ncells + 8 nq W + 8 nq n + 4 nq (k1 + k2 + 1)
 * + 8 * (n > 4096 ? nq ceil(n / 4096) k1 : 0) bytes.
 * Checked on the host BEFORE anything is enqueued; a refused call writes nothing.  Not capturable into a graph (RR_ERR_BAD_ARG).
 * Out of scope: ndocs > 1024, fp16 banks without a centroid table.  A bank split over ranks: the per-part results merged by rr_bank_merge_topk below (which DEFINES the sharded pruned search).  A caller-supplied candidate filter: rr_bank_search_plaid_filtered
 * below; candidates from an IVF: rr_bank_build_ivf / rr_bank_search_plaid_ivf below.  (Python:
 * RerankEngine.bank_search_plaid, PlaidSearch with PassageBank.search / InteractionRerankModel.retrieve / retrieve_and_rerank.) */
int rr_bank_search_plaid(rr_handle h, rr_bank_handle b, const float* query_li, int n_queries, int Lq, int Lq_coarse,
                         int32_t first_passage, int32_t n_passages, int ncells, float centroid_score_threshold, int ndocs, int k,
                         int32_t* indices_out, float* scores_out, int32_t* counts_out, void* hip_stream);

/* THE INVERTED FILE of a compressed bank (or of an fp16 bank with a centroid table, rr_bank_set_centroids: every entry of this
 * section takes it as it takes a compressed bank; "an fp16 bank" below is one without a table), and the pruned search that takes
 * its candidates from it.
 * DEFINITION.  The file covers the passages 0 .. P-1 the bank held when it was built.  With C = n_centroids, list[c], c < C, is the
 * set of passages that have at least one UNMASKED row r with clamp(code_r, 0, C-1) == c (the clamp of rr_bank_search_plaid's
 * scan), in ascending bank index, every passage once per list.  Stored as offsets int64 [C + 1] (offsets[0] = 0, list[c] =
 * pids[offsets[c] .. offsets[c + 1])) and pids int32 [offsets[C]].  This is the content of the reference's ivf.pid.pt, (ivf,
 * ivf_lengths) with ivf_lengths the differences of offsets (_build_ivf, third_party/ColBERT/colbert/indexing/
 * collection_indexer.py:393-431; optimize_ivf, indexing/utils.py:8-48), with one difference: masked rows do not count (the
 * reference's indexer has dropped them before it builds).  The same bytes from run to run.  In host code: rr_util_plaid_ivf
 * (rerank_mi355_diag.h).
 * rr_bank_build_ivf builds, or rebuilds, the file over EVERY passage now in the bank, on the device (csrc/bank_ivf.hip: first
 * occurrences of a code per passage counted with 32-bit vector atomics, an exclusive scan, a fill through per-centroid cursors,
 * then every list sorted: in LDS up to 4096 entries, through a bitmap of P bits above).  A load-time call: it allocates
 * (8 (C + 1) + 4 postings bytes kept; 16 P + 4 C + P / 8 bytes for the call), reads the postings total and the longest list back
 * and synchronises hip_stream; not capturable into a graph (RR_ERR_BAD_ARG).  An fp16 bank: RR_ERR_UNSUPPORTED; an empty bank:
 * RR_ERR_BAD_SHAPE; a failed allocation: RR_ERR_OOM with the bank unchanged: a previous file survives a failed rebuild.
 * LIFETIME: rr_bank_clear drops the file; passages added after a build (rr_bank_add_plaid, rr_bank_add_compress, rr_bank_add) leave it valid
 * for its prefix 0 .. P-1 until rr_bank_extend_ivf (below) extends it over them, or a new build covers them; rr_bank_remove leaves
 * the bank with the file over the survivors of that prefix, rebuilt by this builder when one of them went; rr_bank_destroy frees it.
 * rr_bank_ivf_info: passages_covered (0: no file), the postings total and the longest list; any pointer may be NULL.
 * rr_bank_ivf_read copies offsets [C + 1] and pids [postings] to HOST buffers (either may be NULL) and synchronises hip_stream;
 * RR_ERR_BAD_ARG without a file.  Errors of these calls: rr_bank_last_error.
 * rr_bank_load_ivf takes a file from HOST arrays instead of building it: offsets_host int64 [C + 1] and pids_host int32
 * [offsets_host[C]] (an ivf.pid.pt read back, its ivf_lengths summed into offsets; PassageBank.load_ivf does that).  The loaded file
 * covers EVERY passage the bank holds now; longest_list and postings come from the offsets.  Checked on the host before anything is
 * allocated, RR_ERR_BAD_SHAPE with the first offending list named in rr_bank_last_error: offsets_host[0] != 0, an offset below its
 * predecessor, a pid outside [0, passages held), a list that does not ascend strictly.  An fp16 bank: RR_ERR_UNSUPPORTED; an empty
 * bank: RR_ERR_BAD_SHAPE; under stream capture: RR_ERR_BAD_ARG; a failed allocation: RR_ERR_OOM.  verify != 0: the file is also
 * compared, byte for byte, with a fresh build over the bank (rr_bank_build_ivf's kernels into a temporary, read back): a difference
 * is RR_ERR_BAD_SHAPE.  That is the guard against the file of ANOTHER index, which passes the checks above and would change search
 * results silently; verify == 0 trusts the caller and costs the upload alone.  After every refusal and failure the bank keeps the
 * file it had.  A load-time call: it allocates and synchronises hip_stream.
 *
 * rr_bank_extend_ivf extends the file over the passages added since it was built.  CONTRACT: afterwards the bank holds the
 * inverted file over EVERY passage it holds now, byte for byte the file rr_bank_build_ivf would build at that moment: offsets, pids,
 * passages_covered, postings and longest_list, the same bytes from run to run; so every rr_bank_search_plaid_ivf*, rr_bank_ivf_read
 * and saved file equals that of a fresh build.  A file over P0 < P passages is extended as under HOW; P0 == P: RR_OK, nothing is
 * allocated, enqueued or synchronised and the file is untouched; with no file the call IS rr_bank_build_ivf (the same builder), so
 * a caller may call this one entry after every add.  The refusals are those of rr_bank_build_ivf, in its order: a NULL bank
 * (RR_ERR_BAD_ARG), an fp16 bank (RR_ERR_UNSUPPORTED), an empty bank (RR_ERR_BAD_SHAPE), a capturing stream (RR_ERR_BAD_ARG).
 * ALL OR NOTHING: the extended file is built beside the old one and takes its place only when complete; after RR_ERR_OOM or
 * RR_ERR_HIP the bank keeps the file it had and rr_bank_last_error names the step that failed.  A load-time call: it allocates
 * (8 (C + 1) + 4 (postings_old + postings_new) bytes kept; for the call the old file, which is freed when the new one has taken its
 * place, 16 (P - P0) + 4 C bytes, and (P - P0) / 8 bytes of bitmap when a list gains more than 4096 passages), reads the new
 * postings total and the longest list back and synchronises hip_stream.
 * HOW (csrc/bank_ivf.hip).  An add only brings indices above every index of the file, so a new list is the old list followed by
 * the sorted new entries.  The count walks the passages P0 .. P-1 alone; one scan launch turns the old offsets and the new counts
 * into the new offsets, the total and the longest merged list; one launch copies the old postings to their new places, the work
 * cut into runs of 512 postings (not by list: one list holding every passage costs what many short ones cost; the grid does not
 * depend on longest_list), 16-byte accesses where source and destination are aligned alike and narrower ones elsewhere; the fill
 * walks the new passages again and writes through cursors that start behind each list's old entries; and only the TAILS are
 * sorted, in LDS up to 4096 entries, through a bitmap of P - P0 bits above.  The old part of a list is never touched again.
 * Integer vector atomics only, 64-bit offsets.  Against a rebuild it saves the two walks over the old rows and the sort of the old
 * entries: tools/bench_bank_ivf_extend.py, profiles/bank_ivf_extend_bench.json.log.
 *
 * rr_bank_search_plaid_ivf takes exactly the arguments of rr_bank_search_plaid.  CONTRACT: indices_out, scores_out and counts_out
 * are bit for bit those of rr_bank_search_plaid with the same arguments, the -1 / -inf behind the count included; its checks, its
 * refusals and the graph-capture refusal are those of rr_bank_search_plaid, in the same order.  One refusal more, behind the
 * others: RR_ERR_UNSUPPORTED when the bank has no inverted file, or when [first_passage, first_passage + n_passages) reaches
 * beyond passages_covered; rr_last_error says to call rr_bank_build_ivf (rr_bank_extend_ivf serves as well).
 * Stages 0 - 2 (centroid scores, cells, bitmaps) are rr_bank_search_plaid's.  Its scan and its selection over the dense rows are
 * replaced: CANDIDATES: per query a bitmap over the passages of the range; every distinct cell of the query ORs in the passages of
 * its list that lie in the range (a set: no order enters), and the bitmap is compacted into an ASCENDING candidate list [nq][cap]
 * with a count, cap = max(1, min(n_passages, Lq_coarse * ncells * longest_list)).  A place in that list follows bank-index order,
 * so the tie rule of the order (lower index first) holds for places.  SCORES: A1 and A2 of the listed candidates, a wave per
 * candidate, by the arithmetic of the scan (one device function under both kernels), into compact rows [nq][cap], -inf behind
 * the count.  SELECTION: the selection passes of rr_bank_search over the compact A1 row; the later stages address places of the
 * compact rows and the last one maps a place back to its bank index.  Nothing depends on scheduling.
 * The bitmap pass writes, sets and reads n_passages / 8 bytes per query, and a candidate costs the scan's 5 bytes per row; the
 * scan it replaces reads 5 bytes per row of the whole range per call.  Scratch in the grow-only block rr_bank_search uses, each
 * term rounded up to 16 bytes, Cp, W, k2 as above, k1 = min(ndocs, cap), Wn = ceil(n / 32): 4 nq Cp Lq + 16 nq Cp / 64 + Cp
 * + 4 nq Lq_coarse ncells + 8 nq W + 4 nq Wn + 12 nq cap + 4 nq (k1 + k2 + 2) + 8 * (cap > 4096 ? nq ceil(cap / 4096) k1 : 0)
 * bytes: with cap <= n never more than rr_bank_search_plaid's but for the bitmap and the candidate list (8 nq n against
 * 4 nq (n / 32 + 3 cap)).  Ten launches, a memset and the selection passes, booked in the profile's `tail` class.
 * LIMITS: those of rr_bank_search_plaid (ndocs <= 1024, one device per call with rr_bank_merge_topk behind it for a split bank, compressed banks); rr_bank_search_plaid_tap does not cover
 * this entry.  Under a candidate filter: rr_bank_search_plaid_ivf_filtered below.  (Python: RerankEngine.bank_build_ivf / bank_extend_ivf / bank_search_plaid_ivf, PassageBank.build_ivf / extend_ivf / ivf / save_ivf / load_ivf,
 * PlaidSearch(..., ivf=True).) */
int rr_bank_build_ivf(rr_bank_handle b, void* hip_stream);
int rr_bank_extend_ivf(rr_bank_handle b, void* hip_stream);
int rr_bank_ivf_info(rr_bank_handle b, int32_t* passages_covered_out, int64_t* postings_out, int32_t* longest_list_out);
int rr_bank_ivf_read(rr_bank_handle b, int64_t* offsets_host_out, int32_t* pids_host_out, void* hip_stream);
int rr_bank_load_ivf(rr_bank_handle b, const int64_t* offsets_host, const int32_t* pids_host, int verify, void* hip_stream);

/* REMOVING PASSAGES.  rr_bank_remove drops n passages of either kind of bank and compacts what remains, on the device.
 *   indices_host       : HOST int32 [n]: the dense indices to drop, in any order, distinct, each in [0, passages held).
 *   new_index_host_out : HOST int32 [passages held before the call], or NULL: old dense index -> new dense index, -1 for a removed
 *                        passage.
 * CONTRACT: afterwards the bank is indistinguishable from a fresh bank filled with the survivors in their original order.  The
 * survivors keep their relative order and are renumbered 0 .. passages - n - 1; rows_used shrinks by the removed rows; rows and
 * passage slots are free for later adds.  Every array the bank holds (fp16 rows, mask bytes, codes, residual bytes) equals the
 * fresh bank's over [0, rows_used), to the bit, so every rr_bank_read*, rr_bank_li_scores, rr_forward_interaction_bank,
 * rr_bank_search* and rr_bank_export_plaid result does.  n == 0: RR_OK, nothing changes, the map is the identity.  Removing every
 * passage leaves the state of rr_bank_clear.
 * THE INVERTED FILE: a bank that holds a file over its first P passages holds afterwards the file over the survivors among those P
 * (a prefix of the new bank), built by rr_bank_build_ivf's builder and so with the bytes a fresh build gives; with no survivor
 * among them the file is dropped; with no removed passage among them it stays as it is.  Passages behind the prefix stay
 * uncovered: rr_bank_extend_ivf takes the file over them, as after an add.
 * A LOAD-TIME CALL, like rr_bank_build_ivf: it allocates a staging block (at most 256 MiB, and 32 bytes per run of surviving rows and window),
 * enqueues on hip_stream and synchronises it before it returns; not capturable into a graph.  Work on OTHER streams that reads the
 * bank must have completed, as for rr_bank_clear.  A bank is still not thread-safe: in particular, no removal while another thread
 * looks passages up (the producer thread of a pipelined rerank loop).  Filters built before the call (rr_bank_filter_fill) name the
 * old indices: build them again.  The search's device table is invalidated from the first moved passage on; the next search
 * uploads the rest again, as after an add.
 * ALL OR NOTHING: every refusal comes before anything is enqueued or changed.  RR_ERR_BAD_ARG: a NULL bank, NULL indices with
 * n > 0, a capturing stream.  RR_ERR_BAD_SHAPE: n < 0, an index outside the bank, an index given twice (rr_bank_last_error names
 * it).  RR_ERR_OOM: the staging block cannot be allocated; the bank is unchanged.  THE ONE EXCEPTION: the inverted file is rebuilt
 * after the rows have moved.  If that fails, the passages ARE removed (new_index_host_out is written), the file is dropped, and the
 * call returns the builder's status (RR_ERR_OOM / RR_ERR_HIP); rr_bank_last_error says that the file is gone and must be built
 * again (rr_bank_build_ivf).
 * HOW (csrc/bank_move.hip): from the host table the runs of surviving rows behind the first removed passage, each moving down by a
 * shift that never decreases.  Moving them all in one launch would overwrite rows another workgroup has yet to read, and nothing
 * here waits for another workgroup: the destination rows are cut into windows, per window one launch gathers the window's rows
 * into the staging block and one device-to-device copy puts it in place, in stream order; a later window reads nothing an earlier
 * one wrote.  64-bit byte offsets; 16-byte accesses where source and destination are aligned alike, narrower ones elsewhere (the
 * 4-byte codes, the mask bytes and residual rows under 16 bytes land misaligned relative to their sources).  The plan in host
 * code: rr_util_bank_remove_plan (rerank_mi355_diag.h).  (Python: PassageBank.remove.) */
int rr_bank_remove(rr_bank_handle b, const int32_t* indices_host, int n, int32_t* new_index_host_out, void* hip_stream);

/* rr_bank_export_plaid: a range of a COMPRESSED bank as a ColBERTv2 / PLAID index stores it, written on the device: the way back to
 * disk of what rr_bank_add_plaid / rr_bank_add_compress put in (Python: PassageBank.export_compressed / save_plaid_index).
 * DEFINITION.  For the passages first_passage .. first_passage + n_passages - 1 in bank order, the UNMASKED rows of each passage
 * (mask byte != 0), in row order, back to back:
 *   codes_out        : DEVICE int32 [R], 4-byte aligned.
 *   residuals_out    : DEVICE uint8 [R, li_dim * nbits / 8], aligned to min(16, li_dim * nbits / 8) bytes.
 *   doclens_host_out : HOST int32 [n_passages]: the unmasked rows of passage i; it may be 0.
 *   *rows_host_out   : HOST: R, the sum of the doclens.
 * These are the bytes the reference's indexer would have stored for the passages: it drops the skiplist tokens before it compresses
 * (third_party/ColBERT/colbert/indexing/index_saver.py:70-90, collection_encoder.py), so MASKED ROWS DO NOT TRAVEL.  A bank loaded
 * from the export (rr_bank_add_plaid with the doclens, no mask) gives the same MaxSim, the same search results and the same inverted
 * file, bit for bit; it is NOT a snapshot of the bank: the codes and bytes under masked rows, and the positions of the kept rows
 * inside their passage, are gone.  A passage of doclen 0 cannot be added again (rr_bank_add_plaid refuses it).
 * SIZING CALL: codes_out and residuals_out both NULL: only doclens_host_out and *rows_host_out are written.
 * REFUSALS, every one from the host, writing nothing: exactly one of codes_out / residuals_out NULL, a NULL doclens_host_out or
 * rows_host_out, a misaligned output, a capturing stream (RR_ERR_BAD_ARG); an fp16 bank, with or without a centroid table: it holds no residuals
 * (RR_ERR_UNSUPPORTED); n_passages < 1 or a
 * range that is not inside the bank (RR_ERR_BAD_SHAPE); both outputs given and capacity_rows < R (RR_ERR_BAD_SHAPE, decided after
 * the count and before any row is moved; rr_bank_last_error names R).
 * Three kernels (csrc/bank_export.hip), no global atomics, the same bytes from run to run: a count (a wave per passage, 64 mask
 * bytes a step, ballot and popcount), the exclusive scan of the doclens into 64-bit row offsets (the scan of the inverted file's
 * counts), and the move (a wave per passage; the ballot ranks the kept rows of a step, whose residual bytes go out as one contiguous
 * run in 16-byte accesses).  Every row and byte offset is 64-bit.  The kernels walk the bank's device passage table, brought up to
 * date as the first search after an add does.  A save-time call, like rr_bank_build_ivf: it allocates 12 n_passages + 24 bytes for
 * the call and synchronises hip_stream, because it reads R back.  Errors: rr_bank_last_error. */
int rr_bank_export_plaid(rr_bank_handle b, int32_t first_passage, int32_t n_passages, int32_t* doclens_host_out, int32_t* codes_out,
                         uint8_t* residuals_out, int64_t capacity_rows, int64_t* rows_host_out, void* hip_stream);
int rr_bank_search_plaid_ivf(rr_handle h, rr_bank_handle b, const float* query_li, int n_queries, int Lq, int Lq_coarse,
                             int32_t first_passage, int32_t n_passages, int ncells, float centroid_score_threshold, int ndocs, int k,
                             int32_t* indices_out, float* scores_out, int32_t* counts_out, void* hip_stream);

/* CANDIDATE FILTERS: the three searches restricted to a caller's set of passages per query (the reference: filter_fn of
 * Searcher.search / search_all / dense_search, third_party/ColBERT/colbert/searcher.py:68-134, applied by IndexScorer.rank between
 * candidate generation and the pruning stages, colbert/search/index_storage.py:86-93).  A passage outside the set is never a
 * candidate and costs no scoring work.
 * THE FILTER: filter_bits, DEVICE uint32 [filter_rows][filter_ld], 4-byte aligned.  Bit (i & 31) of word (i >> 5) of a row stands
 * for bank index i: ABSOLUTE, not relative to the range, so one filter serves any range and a rank searching its slice does not
 * shift it.  filter_rows is 1 (one set for every query) or n_queries (row q for query q); anything else: RR_ERR_BAD_SHAPE.
 * filter_ld >= ceil((first_passage + n_passages) / 32), else RR_ERR_BAD_SHAPE.  A NULL or misaligned filter_bits: RR_ERR_BAD_ARG
 * (the unfiltered entries exist for "no filter").  Bits of indices outside [first_passage, first_passage + n_passages) are never
 * consulted, set bits beyond the bank's passage count in the last word included.  The filter is read by the kernels of the call:
 * it must stay unchanged until the call has completed on hip_stream.
 * Each entry keeps the checks, refusals, check order, graph-capture refusal and the "a refused call writes nothing" rule of its
 * unfiltered entry (its name in rr_last_error aside); the filter checks above come behind that entry's other refusals.
 *
 * rr_bank_search_filtered: rr_bank_search over the passages of the range whose bit is set.  A competitor's score is bit for bit
 * rr_bank_search's, the order rr_bank_search's one order.  -inf means absent, as in the pruned search: a competitor whose exact
 * score is a genuine -inf counts as absent.  counts_out int32 [n_queries] (DEVICE, required; NULL: RR_ERR_BAD_ARG) gets the number
 * of real entries of a query, at most k; behind it indices_out holds -1 and scores_out -inf.  1 <= k <= min(n_passages, 1024) as
 * rr_bank_search has it; k may exceed the number of allowed passages.  PROPERTY: with every bit of the range set, indices_out and
 * scores_out are rr_bank_search's and every count is k (where no score is -inf).
 * The scoring kernel of rr_bank_search with one more picker (csrc/bank_search.hip): a workgroup none of whose chunk's passages is
 * allowed writes its -inf entries and ends before it stages its query block; a wave whose passage has a clear bit writes -inf,
 * reads no row of the bank and issues no matrix instruction; the bit is a scalar load.  Then rr_bank_search's selection passes over
 * the dense row, unchanged, and one pass of the pruned search's list kernel over their k survivors, which drops the absent, writes
 * the tail and counts.  The block grows by 4 n_queries k bytes over rr_bank_search's.
 * LIMIT: the selection walks the dense row of n_passages scores per query, however few bits are set; the list-driven form below
 * does not.  Measured on one MI355X (tools/bench_bank_search_filter.py --sparse, profiles/bank_search_sparse_bench.json.log; a
 * compressed bank of 12 M rows as 100 000 and as 800 000 passages, 1 and 16 queries, one filter row and a row per query): the
 * list-driven form is the faster one at every measured density below 1.0 (sparse / dense 0.87 .. 0.77 at 50 % allowed, 0.64 ..
 * 0.44 at 10 %, 0.91 .. 0.33 at 1 %, 0.95 .. 0.28 at 0.1 %, the larger gains at 16 queries and at 800 000 passages); with every
 * bit set it equals this entry at 16 queries and costs 3 % (100 000 passages) to 10 % (800 000) more at one query.  Against
 * rr_bank_li_scores over the explicit pair list and a top-k of its maxsim_out, the route this paragraph used to recommend, the
 * list-driven form is 1.6 to 60 times faster, except at ONE query over 100 000 passages with about a thousand allowed passages or
 * fewer, where the pair list is still ahead (1.3 x at 1 %, 2.9 x at 0.1 %).
 *
 * rr_bank_search_filtered_sparse: the list-driven form of rr_bank_search_filtered.  DEFINITION: for every argument set
 * rr_bank_search_filtered accepts, indices_out, scores_out and counts_out are that entry's bytes; its checks, check order, refusals
 * (k > 1024: RR_ERR_UNSUPPORTED; a NULL counts_out: RR_ERR_BAD_ARG; ...), graph-capture refusal and "a refused call writes nothing"
 * are that entry's, its own name in rr_last_error aside.  What differs is the work: every stage runs over the passages the filter
 * allows, not over the range.  (1) One workgroup per filter row writes the set bits of the range as an ascending list of
 * range-relative indices cand[row][0 .. cnt[row]) and cnt[row] (csrc/bank_ivf.hip: the compaction kernel of the inverted-file search
 * over the filter's own words, the last word cut to the range; no atomics).  (2) The scoring kernel under one more picker
 * (csrc/bank_search.hip, pick_places): a workgroup owns search_chunk consecutive PLACES of its query's candidate row (one shared
 * filter row: every query's) and writes their scores to those places of a compact row of pitch n_passages; a workgroup behind the
 * count returns before it stages its query block.  fp16 and compressed banks.  (3) topk_select_counted_kernel: rr_bank_search's
 * selection over the first cnt places of the compact rows, the place in the key (places ascend with the bank index: ties break as
 * before); the host launches the passes n_passages would need, each pass derives its list's length from cnt on the device, a slice
 * behind it ends at once, and the last pass maps a place to first_passage + cand[row][place], drops the -inf scorers, writes
 * -1 / -inf behind the count and counts_out.  Nothing is read back: the call is as asynchronous as the dense form.
 * SCRATCH (the handle's grow-only search block): the dense form's bytes, 4 n_queries n_passages + 2 * 4 n_queries ceil(n_passages /
 * 4096) k (none at n_passages <= 4096) + 4 n_queries k, plus 4 filter_rows n_passages for cand and 4 filter_rows for cnt, each
 * term rounded up to 16 bytes.  The profile books the three launches in the `tail` class, FLOPs and bytes for the range's mean
 * passage length times the pitch: an upper bound, as the pruned search books its survivors.
 *
 * rr_bank_search_plaid_filtered: rr_bank_search_plaid with CANDIDATES read as: the passage's bit is set AND at least one of its
 * unmasked rows has a code in the cell set.  Stages 0 to 3 and OUTPUT are otherwise word for word rr_bank_search_plaid's.
 * PROPERTY A: with every bit of the range set, the result is the bytes of rr_bank_search_plaid.  PROPERTY B: the result is the
 * bytes of rr_bank_search_plaid on a bank that differs only in that every row of a filtered-out passage is masked; with a filter
 * row per query this holds query by query.  The scan decides a clear bit before it reads the passage's table entry, codes or mask
 * bytes: a filtered-out passage costs one bit and its two -inf, not 5 bytes per row.  No scratch beyond rr_bank_search_plaid's;
 * rr_bank_search_plaid_tap covers this entry.
 *
 * rr_bank_search_plaid_ivf_filtered: the bytes of rr_bank_search_plaid_filtered, with the candidates from the bank's inverted
 * file; the one refusal rr_bank_search_plaid_ivf adds stands in the same place, in front of the filter checks.  The per-query
 * bitmap of the candidate step is ANDed with the filter's bits of the range as it is compacted (a range that does not start at a
 * multiple of 32 takes a bitmap word's bits from two filter words); cap and the layout of the block stay rr_bank_search_plaid_ivf's.
 *
 * rr_bank_filter_fill writes a filter for bank `b` from HOST index lists: row r of filter_bits (DEVICE uint32 [rows][filter_ld],
 * 4-byte aligned) gets the bank indices indices_host[offsets_host[r] .. offsets_host[r + 1]), offsets_host int64 [rows + 1] from
 * 0, ascending; duplicates are allowed, a row may be empty.  exclude == 0: exactly those bits are set.  exclude != 0: every bit
 * 0 .. passages - 1 is set except those (passages: what the bank holds now).  Bits at or beyond `passages`, up to filter_ld words,
 * are zero in both modes.  An index outside [0, passages), offsets that do not start at 0 or descend, rows outside 1 .. 65535, an
 * empty bank or filter_ld < ceil(passages / 32): RR_ERR_BAD_SHAPE, and nothing is written; NULL or misaligned pointers, a
 * capturing stream: RR_ERR_BAD_ARG.  The lists are staged as rr_bank_add stages its descriptors (the bank's pinned slot pair, one
 * asynchronous copy) and one kernel writes the bits (csrc/bank_ivf.hip: a workgroup per row fills its words, then clears or sets
 * the listed bits with 32-bit vector atomicAnd / atomicOr; an AND or an OR has one result, so the bytes do not depend on
 * scheduling).  Errors: rr_bank_last_error.  In host code: rr_util_bank_filter_bits (rerank_mi355_diag.h).  A filter describes
 * the bank it was filled for: passages added later have clear bits under exclude == 0 and under exclude != 0 alike.
 * (Python: RerankEngine.bank_search_filtered / bank_search_filtered_sparse / bank_search_plaid_filtered / bank_search_plaid_ivf_filtered, PassageBank.filter,
 * PassageBank.search(filter=), InteractionRerankModel.retrieve / retrieve_and_rerank(allowed=, excluded=, filter=).) */
int rr_bank_search_filtered(rr_handle h, rr_bank_handle b, const float* query_li, int n_queries, int Lq, int32_t first_passage,
                            int32_t n_passages, int k, const uint32_t* filter_bits, int filter_rows, int64_t filter_ld,
                            int32_t* indices_out, float* scores_out, int32_t* counts_out, void* hip_stream);
int rr_bank_search_filtered_sparse(rr_handle h, rr_bank_handle b, const float* query_li, int n_queries, int Lq, int32_t first_passage,
                                   int32_t n_passages, int k, const uint32_t* filter_bits, int filter_rows, int64_t filter_ld,
                                   int32_t* indices_out, float* scores_out, int32_t* counts_out, void* hip_stream);
int rr_bank_search_plaid_filtered(rr_handle h, rr_bank_handle b, const float* query_li, int n_queries, int Lq, int Lq_coarse,
                                  int32_t first_passage, int32_t n_passages, int ncells, float centroid_score_threshold, int ndocs, int k,
                                  const uint32_t* filter_bits, int filter_rows, int64_t filter_ld, int32_t* indices_out,
                                  float* scores_out, int32_t* counts_out, void* hip_stream);
int rr_bank_search_plaid_ivf_filtered(rr_handle h, rr_bank_handle b, const float* query_li, int n_queries, int Lq, int Lq_coarse,
                                      int32_t first_passage, int32_t n_passages, int ncells, float centroid_score_threshold, int ndocs,
                                      int k, const uint32_t* filter_bits, int filter_rows, int64_t filter_ld, int32_t* indices_out,
                                      float* scores_out, int32_t* counts_out, void* hip_stream);
int rr_bank_filter_fill(rr_bank_handle b, const int32_t* indices_host, const int64_t* offsets_host, int rows, int exclude,
                        uint32_t* filter_bits, int64_t filter_ld, void* hip_stream);

/* rr_bank_merge_topk: the k-lists of P parts of a corpus (the banks of P ranks, several banks of one process, or ranges of one
 * bank) merged into one list over GLOBAL indices, on the device.  What a bank split over ranks needs behind its searches.
 * THE MERGED LIST.
 * Inputs:
 *   P = n_parts, 1 <= P <= 64.   nq = n_queries, 1 <= nq <= 65535.
 *   Per part p and query q a list of k_in entries:
 *     indices_in[p][q][i] : int32, LOCAL indices of part p.
 *     scores_in[p][q][i]  : float32.
 *     counts_in[p][q]     : int32, or counts_in NULL: every list holds k_in entries.
 *   part_offsets_host : HOST int32 [P + 1].  Part p stands for the global indices part_offsets[p] .. part_offsets[p + 1] - 1.
 * Rules:
 *   - Entry (p, q, i) is REAL iff i < clamp(counts_in[p][q], 0, k_in) and 0 <= indices_in[p][q][i] < part_offsets[p + 1] -
 *     part_offsets[p].  Its global index is g = part_offsets[p] + indices_in[p][q][i].
 *   - The score takes part as it is: NaN, +-inf and -0 included.  Inside the count, -inf is a number like any other.
 *   - Nothing is assumed about the order of the incoming lists.
 *   - Per query, the real entries of all parts are ordered by the one rank order of the searches on (score, g): NaN first, higher
 *     score, equal scores (+0 == -0) by ascending g (rank_key(score, g) of csrc/rank_order.h, a larger key first).
 *   - The first min(k, real entries) are written to indices_out[q][.] (the global index g), scores_out[q][.] (or NULL: the bits of
 *     the entry's score, a -0 and a NaN's payload included) and parts_out[q][.] (or NULL: the part p the entry came from).
 *     counts_out[q] (required) gets their number.  Behind the count the rows hold -1 / -inf / -1 up to k.
 *   - A local index listed twice within a part appears twice.  Entries that agree in part, index and rank of the score (two +-0,
 *     two NaNs) keep the order they have in their list: the order of a STABLE sort of the entries taken part by part.
 *   - 1 <= k <= k_in.  The global top k is contained in the union of the per-part top k_in only for k <= k_in, and the call
 *     promises exactly that.
 * PROPERTY.  Let part p hold the rr_bank_search result, with k_in >= k, of a bank holding the passages part_offsets[p] .. of a
 * corpus in corpus order.  Then the merged list is, byte for byte, rr_bank_search with k over one bank holding the whole corpus.
 * The same holds for the ranges [first, first + n) of one bank, each list made local again (index - first).  It holds for
 * rr_bank_search_filtered, with counts.  It holds for rr_bank_search_plaid* with ncells = n_centroids and ndocs / 4 >= every
 * part's size.  IN GENERAL a sharded PLAID search is DEFINED as the merge of the per-part PLAID searches with the same
 * parameters; it is NOT the PLAID search of the union, because each part keeps its own ndocs survivors.  A part with fewer than k
 * passages is searched with its own size as k and padded, with its count saying so.
 * Arrays: every in and out array is DEVICE, 4-byte aligned.  part_stride is the distance in 4-byte words from part p to part p + 1,
 * the same for indices_in and scores_in, >= n_queries * k_in; count_stride likewise for counts_in, >= n_queries.  So the block an
 * all-gather delivers serves directly, [P][ indices | score bits | counts | ... ], as three base pointers into one buffer.  No
 * further layout is imposed.  indices_out / scores_out / parts_out [n_queries, k], counts_out [n_queries].
 * One kernel (csrc/bank_merge.hip), one workgroup per query, booked in the profile's `tail` class: the 64-bit keys of the P * k_in
 * entries, padded with key 0 to the next power of two, are sorted in LDS by the bitonic network and the first k leave; a winner's
 * part is found by a search of g in part_offsets, which travels as a kernel argument.  No global atomics, nothing depends on
 * scheduling: the same bytes from run to run.  Nothing is allocated, nothing staged; the handle's search block is not touched.
 * REFUSALS, every one from the host before anything is enqueued; a refused call writes nothing; the sentence: rr_last_error(h).
 *   RR_ERR_BAD_ARG     : a NULL handle, indices_in, scores_in, part_offsets_host, indices_out or counts_out; a misaligned
 *                        pointer; a full-context handle; a capturing stream (as every bank search refuses them).
 *   RR_ERR_BAD_SHAPE   : n_parts, n_queries, k_in or k non-positive; k > k_in; a stride below its minimum; part_offsets_host[0] < 0
 *                        or a descending offset (an empty part is allowed).
 *   RR_ERR_UNSUPPORTED : n_parts > 64; n_queries > 65535; n_parts * k_in > 8192 (8 ranks of the largest k the searches take: 64 KB
 *                        of keys).
 * LIMITS: the parts' lists must already be on this device (the collective is the caller's: Python sharding.ShardedBank does it with
 * one all-gather); int32 global indices, so a corpus of at most 2^31 - 1 passages.  In host code: rr_util_bank_merge_topk
 * (rerank_mi355_diag.h).  (Python: RerankEngine.bank_merge_topk, passage_bank.search_banks, sharding.ShardedBank /
 * exchange_bank_results / sharded_retrieve_and_rerank.) */
int rr_bank_merge_topk(rr_handle h, const int32_t* indices_in, const float* scores_in, const int32_t* counts_in, int64_t part_stride,
                       int64_t count_stride, int n_parts, const int32_t* part_offsets_host, int n_queries, int k_in, int k,
                       int32_t* indices_out, float* scores_out, int32_t* counts_out, int32_t* parts_out, void* hip_stream);

/* rr_head_joint: rr_head with the head RerankModel.forward runs (rr_forward_joint): `loss_fn(logits, logits)`
 * (rerank_model.py:328) — the labels are the logits themselves (2H_BCE: the two heads as class-probability targets).  The
 * head of a packed joint call, after the scatter.  negative_sampling with loss_out: RR_ERR_UNSUPPORTED, as rr_forward_joint. */
int rr_head_joint(rr_handle h, const float* logits, const float* logits2, int Bq, int K, float* loss_out, float* scores_out,
                  int32_t* order_out, void* hip_stream);

/* rr_head_lists: rr_head / rr_head_joint over a LIST LAYOUT: n_lists lists, list q holding k_q >= 1 candidates (at most 4096,
 * as K of rr_head), pairs stored list after list, N = sum k_q.  The reference reranks one query per forward and takes whatever
 * its retriever returned for it (src/executors/Reranker_base_executor.py:807-976), so lists of unequal length work there query
 * by query; this is the head that lets several of them share one forward here.  No reference counterpart as one call.
 * (Python: RerankEngine.head_lists.)
 *   list_offsets : HOST int32 [n_lists + 1], offsets[q] = k_0 + ... + k_{q-1}, offsets[n_lists] = N.  Checked before anything
 *       is enqueued: offsets[0] == 0 and strictly ascending (no empty list), else RR_ERR_BAD_SHAPE; a list above 4096
 *       RR_ERR_UNSUPPORTED, as rr_head answers K > 4096.  A refused call writes nothing.  May be reused when the call returns.
 *   logits / logits2 : DEVICE float32 [N] (logits2: the first head, 2H_BCE only, as for rr_head).
 *   gather : DEVICE int32 [N] or NULL.  Pair p's logits are read at logits[gather[p]] (and logits2[gather[p]]); NULL = p.  With
 *       the inverse of a packed forward's pair order the head consumes the logits in packed order, without the scatter in
 *       between.  Must hold indices in [0, N); the array is on the device and is not checked.
 *   labels : DEVICE float32 [N] in pair order (never gathered) or NULL = the first candidate of EVERY list is the positive
 *       (src/models/rerank/utils.py:239-243, per list).  joint = 1 ignores it.
 *   joint : 0 = rr_head's loss; 1 = rr_head_joint's (the logits are their own targets, read through the same gather).
 *   loss_out : DEVICE float32 scalar or NULL.  The per-list partial sums and weights reduced in list order, as rr_head reduces
 *       its per-query partials: BCE kinds and the joint loss = the mean over all N pairs (what the reference's loss function
 *       returns for the concatenated logits), negative_sampling = the mean over lists of CE(target = the list's first
 *       candidate) (the mean of what the reference computes query by query), weighted 2H_BCE = weight-normalised over all pairs.
 *   list_loss_out : DEVICE float32 [n_lists] or NULL: list q's own loss, what rr_head returns for that list alone (Bq = 1).
 *   scores_out : DEVICE float32 [N] or NULL, pair order.  order_out : DEVICE int32 [N] or NULL: list q's descending, retrieval-
 *       order-stable rank at order_out[offsets[q] .. offsets[q + 1]), as indices LOCAL to the list (0 .. k_q - 1).
 * With offsets = [0, K, 2K, ...], gather = NULL, loss_out, scores_out and order_out hold rr_head's (joint = 1: rr_head_joint's)
 * bits for (Bq, K): the same arithmetic in the same order (tests/test_gpu_lists.py).  Every combination rr_head / rr_head_joint
 * reject is rejected in the same way (labels with negative_sampling, 2H_BCE without logits2, joint on an interaction handle,
 * joint with negative_sampling and a loss).  The library stages the offsets itself, through the slots rr_assemble_pairs uses;
 * enqueued on hip_stream; NOT capturable into a graph (RR_ERR_BAD_ARG under stream capture). */
int rr_head_lists(rr_handle h, const float* logits, const float* logits2, const float* labels, int n_lists,
                  const int32_t* list_offsets, const int32_t* gather, int joint, float* loss_out, float* list_loss_out,
                  float* scores_out, int32_t* order_out, void* hip_stream);

/* ---- Host-side pair-input assembly (no GPU involved): WordPiece tokenisation of the (query, candidate) texts into the
 * int64 [N, S] tensors rr_forward takes.  Replaces prepare_full_context_inputs (src/models/rerank/utils.py:129-167) and
 * the BertTokenizer encode / decode / batch_encode_plus calls under it (transformers 4.38.2 slow tokenizer semantics).
 * All pointers HOST.  A handle is immutable after creation and may be shared by threads. */
typedef struct rr_tokenizer* rr_tokenizer_handle;
/* vocab_tokens[i] = UTF-8 token with id i (the lines of vocab.txt); must contain [UNK] [CLS] [SEP] [PAD]. */
int rr_tok_create(const char* const* vocab_tokens, int vocab_size, int do_lower_case, rr_tokenizer_handle* out);
int rr_tok_destroy(rr_tokenizer_handle h);
/* encode(text, add_special_tokens=False, max_length=max_tokens, truncation=True); max_tokens < 0 = no limit.
 * Returns the number of ids written, or <0 (RR_ERR_BAD_SHAPE: capacity too small). */
int rr_tok_encode(rr_tokenizer_handle h, const char* text, int max_tokens, int32_t* ids_out, int capacity);
/* decode(ids) with clean_up_tokenization_spaces=True; returns the byte length (NUL-terminated), or <0. */
int rr_tok_decode(rr_tokenizer_handle h, const int32_t* ids, int n, char* out, int capacity);
/* The whole of prepare_full_context_inputs: queries[n_queries], contexts[n_queries * docs_per_query] (query-major);
 * every text is truncated by an encode -> decode -> encode round trip (max_query_length / max_context_length tokens),
 * pairs are encoded [CLS] q [SEP] c [SEP] with LONGEST_FIRST truncation to max_length and right padding (pad id,
 * mask 0, type 0).  Outputs int64 [N, max_length], e.g. pinned buffers; n_threads <= 0 = hardware concurrency. */
int rr_tok_prepare_pairs(rr_tokenizer_handle h, const char* const* queries, int n_queries, const char* const* contexts,
                         int docs_per_query, int max_query_length, int max_context_length, int max_length, int n_threads,
                         int64_t* input_ids, int64_t* attention_mask, int64_t* token_type_ids);
/* The same pairs in COMPACT form, for rr_assemble_pairs: identical round trips, budgets and LONGEST_FIRST truncation, no
 * padded rows.  pool (int32, pool_capacity entries) receives every query's round-tripped ids once (query order), followed by
 * every pair's kept context ids c[:lb] (pair order); desc (int32 [N, 4]) receives per pair (query offset, la, context offset,
 * lb), offsets into pool: pair p is [CLS] q[:la] [SEP] c[:lb] [SEP], la + lb + 3 <= max_length tokens, exactly the non-pad
 * part of rr_tok_prepare_pairs' row p.  *pool_needed = the entries the pool needs; when that exceeds pool_capacity the call
 * returns RR_ERR_BAD_SHAPE and writes neither pool nor desc (grow the buffer and call again).  n_threads as rr_tok_prepare_pairs. */
int rr_tok_prepare_compact(rr_tokenizer_handle h, const char* const* queries, int n_queries, const char* const* contexts,
                           int docs_per_query, int max_query_length, int max_context_length, int max_length, int n_threads,
                           int32_t* pool, int64_t pool_capacity, int64_t* pool_needed, int32_t* desc);
/* Context-encoder tokenisation in COMPACT form, for rr_assemble_joint; replaces FLMRContextEncoderTokenizer.__call__
 * (tokenization_flmr.py:120-150: ". " + text, padding="max_length", truncation=True, ids[:, 1] = [unused1]) as
 * tokenize_retrieved_docs calls it (Reranker_base_executor.py:1056-1066).  Writes each context's t[0:min(len(t), max_tokens)],
 * t = encode(text) without special tokens, once into pool (int32, pool_capacity entries, context order), and offsets[i] /
 * lengths[i] (int32 [n_contexts]); with max_tokens = max_length - 3 the reference's row is [CLS] [unused1] t[0:m] [SEP] [PAD]...
 * (the "." of the prefix is always a token of its own).  *pool_needed = the entries the pool needs; when that exceeds
 * pool_capacity the call returns RR_ERR_BAD_SHAPE and writes neither pool, offsets nor lengths.  n_threads as
 * rr_tok_prepare_pairs. */
int rr_tok_prepare_contexts_compact(rr_tokenizer_handle h, const char* const* contexts, int n_contexts, int max_tokens,
                                    int n_threads, int32_t* pool, int64_t pool_capacity, int64_t* pool_needed, int32_t* offsets,
                                    int32_t* lengths);

/* Profiling: when on, rr_forward brackets every kernel launch with HIP events on the work
 * stream; rr_get_profile synchronises, accumulates and returns the per-class totals. */
int rr_set_profiling(rr_handle h, int on);
int rr_get_profile(rr_handle h, rr_profile* out, int reset);

/* Diagnostic and test-support entry points (debug taps, stand-alone operators rr_op_*, process-wide tuning switches, in-kernel
 * timelines) are exported by the same library but are NOT part of the product ABI: include/rerank_mi355_diag.h. */

#ifdef __cplusplus
}
#endif
#endif /* RERANK_MI355_H */
