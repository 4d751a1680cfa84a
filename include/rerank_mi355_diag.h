/*
 * rerank_mi355_diag.h — diagnostic and test-support entry points of librerank_mi355.so
 *
 * NOT the product ABI.  include/rerank_mi355.h is what a binding of the reference's reranker binds; the
 * functions below exist for the parity tests (stand-alone operators, debug taps), the A/B tools under tools/ (process-wide
 * switches that select between equivalent kernels or move time) and the in-kernel timelines.  They are process-wide, not
 * thread-safe against running forwards, carry no compatibility promise and are never needed on the product path: what
 * changes the arithmetic of a forward is a per-handle option (rr_set_option in rerank_mi355.h).
 * The arithmetic they expose follows stock HF BERT behind /root/reference/src/models/flmr/models/flmr/modeling_flmr.py:1622
 * (text encoder) and /root/reference/src/models/rerank/attention_fusion.py:133-144 (cross-encoder layers).
 */
#ifndef RERANK_MI355_DIAG_H
#define RERANK_MI355_DIAG_H

#include "rerank_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Debug taps: copy an internal activation of the LAST rr_forward to HOST memory as float32.
 * names: "text_hidden" [n,S,H], "late_interaction" [n,T,D], "ce_hidden" [n,T,Hc]. Returns element
 * count written, or <0.  Synchronises the stream.  Test-only. */
int64_t rr_debug_read(rr_handle h, const char* name, float* host_out, int64_t max_elems);

int rr_set_debug(rr_handle h, int on);   /* keep a copy of the text-encoder output for rr_debug_read */

/* Stand-alone operator entry points (unit parity tests call the kernels through these).
 * All pointers DEVICE.  bf16 tensors are uint16_t bit patterns.  Kd % 64 == 0, N % 4 == 0. */
int rr_op_gemm_bf16(const uint16_t* A /*[M,Kd]*/, const uint16_t* W /*[N,Kd]*/, const float* bias /*[N]|NULL*/,
                    int M, int N, int Kd,
                    int epilogue /*0: +bias -> bf16; 1: +bias, erf-GELU -> bf16; 2: +bias -> f32; 3: +bias, tanh -> bf16;
                                   5: +bias, quick-GELU -> bf16*/,
                    void* out, void* hip_stream);
/* out f32 [M,N] = A W^T + bias + resid */
int rr_op_gemm_resid_f32(const uint16_t* A, const uint16_t* W, const float* bias, const float* resid /*[M,N]*/,
                         int M, int N, int Kd, float* out, void* hip_stream);
/* The LayerNorm-statistics dataflow the layers use between blocks: rr_op_layernorm_stats writes the 16-bit normalised
 * rows (and optionally the fp32 ones) plus stats[row] = (mean, rstd); rr_op_gemm_ln_resid_f32 then forms its residual
 * as (x - mean) * rstd * gamma + beta from the LayerNorm's INPUT x:  out = A W^T + bias + LN(x). */
int rr_op_layernorm_stats(const float* x, const float* gamma, const float* beta, float eps, int rows, int cols,
                          float* out_f32 /*|NULL*/, uint16_t* out_bf16, float* stats /*[rows,2]*/, void* hip_stream);
int rr_op_gemm_ln_resid_f32(const uint16_t* A, const uint16_t* W, const float* bias, const float* x /*[M,N]*/,
                            const float* stats /*[M,2]*/, const float* gamma /*[N]*/, const float* beta /*[N]*/, int M,
                            int N, int Kd, float* out, void* hip_stream);
/* softmax(q k^T + key_bias) v per head (head dim 64; q is expected pre-scaled by log2(e)/sqrt(64): the kernel takes
 * base-2 exponentials of q k^T as it is; key_bias is additive in that domain, 0 / -1e30).
 * q row (b,t): q + ((b / q_batch_div) * Tq + t) * q_stride + head*64 ; k,v row (b,t): (b*Tk + t) * kv_stride + head*64;
 * key_bias f32 [B,Tk] additive (0 = attend, -1e30 = masked) or NULL.  q_stride, kv_stride and out_stride are multiples of 8
 * elements (16-byte row chunks). */
int rr_op_attention_bf16(const uint16_t* q, const uint16_t* k, const uint16_t* v, int q_stride, int kv_stride,
                         const float* key_bias, int B, int heads, int Tq, int Tk, int q_batch_div, uint16_t* out,
                         int out_stride, void* hip_stream);
/* rr_op_attention_bf16 with every launch form the forwards use (rr_op_attention_bf16 is this call with q_batch_off 0, no dense
 * bias, schedule_blocks 0 and fixed_mode -1).  q row (b,t): q + (((b + q_batch_off) / q_batch_div) * Tq + t) * q_stride + head*64.
 * dense_bias: f32 [B][Tq][dense_ld] added to the scores in the natural-log domain (attention fusion; dense_ld a multiple of 64,
 * >= Tk; it always runs the online form), or NULL.  schedule_blocks > 0: the grid size that picks the schedule (a packed forward
 * passes its padded call's grid); 0 = this call's own grid.  fixed_mode 0..3: the schedule ("attn_fixed_ref" values), -1 = the
 * process-wide switch. */
int rr_op_attention_ex(const uint16_t* q, const uint16_t* k, const uint16_t* v, int q_stride, int kv_stride,
                       const float* key_bias, int B, int heads, int Tq, int Tk, int q_batch_div, int q_batch_off, uint16_t* out,
                       int out_stride, const float* dense_bias, int dense_ld, int64_t schedule_blocks, int fixed_mode,
                       void* hip_stream);
/* Self-attention over the segments of a packed layer (Tq = Tk = seg_len[s]): segment s holds seg_n[s] sequences whose rows lie
 * back to back from row seg_row0[s] of q / k / v / out (row r at q + r * q_stride, ...); key_bias is one f32 per row, or NULL.
 * One fixed-reference launch (and its redo launch) for all segments when the schedule is the fixed-reference one and nseg <= 64,
 * else one rr_op_attention_ex per segment.  seg_* are HOST arrays. */
int rr_op_attention_segs(const uint16_t* q, int q_stride, const uint16_t* k, const uint16_t* v, int kv_stride,
                         const float* key_bias, int heads, int nseg, const int* seg_n, const int* seg_len, const int64_t* seg_row0,
                         uint16_t* out, int out_stride, int64_t schedule_blocks, int fixed_mode, void* hip_stream);
/* Attention-fusion bias builders.  scores f32 [*][S][Tq]; the Tc context rows of pair p start at row row0 of its scores.
 * rr_op_fusion_adj: pairs pair0 .. pair0 + n - 1 -> adj [n][Tq + Tc][ld] (ld a multiple of 64, >= Tq + Tc; columns
 * [Tq + Tc, ld) written as 0).  rr_op_fusion_adj_segs: nseg <= 64 segments of seg_n[s] pairs (HOST arrays) whose sequences end
 * after seg_tk[s] <= Tc context tokens, normalised over all Tc; segment s as [seg_n[s]][Tq + seg_tk[s]][round_up(Tq + seg_tk[s],
 * 64)], the segments back to back. */
int rr_op_fusion_adj(const float* scores, int S, int Tq, int Tc, float mult, int pair0, int n, float* adj, int ld, int row0,
                     void* hip_stream);
int rr_op_fusion_adj_segs(const float* scores, int S, int Tq, int Tc, float mult, int nseg, const int* seg_n, const int* seg_tk,
                          float* adj, int row0, void* hip_stream);
/* Tuning hooks (tools/bench_gemm.py). rr_set_gemm_variant forces a kernel / tile configuration: 0..3 = gemm_kernel_s
 * {128x128x2st, 128x128x4st, 256x256x2st, 256x128x3st} with the direct epilogue, 10 = 256x256x2st with the LDS-staged
 * epilogue, 11 / 12 = gemm_kernel_h (half-tile ring) with the direct / LDS-staged epilogue, 13 = its diagnostic timeline
 * build, 14 = gemm_kernel_hp (persistent ring); -1 = shape heuristic (default).  rr_set_gemm_stamps: DEVICE buffer of
 * 8 uint64 per workgroup that receives s_memtime stamps (entry, first tile ready, main loop done, end), or NULL.
 * Both are process-wide and diagnostic. */
/* e4m3 (OCP fp8) GEMM on the block-scaled matrix core (v_mfma_scale_f32_16x16x128_f8f6f4, block scales 2^0):
 * out = epi(scale * A8[M,K] . W8[N,K]^T + bias), A8/W8 row-major e4m3 bytes, scale = the product of the two per-tensor
 * dequantisation scales, epilogue 0 = bf16 out, 1 = bf16(erf-GELU), 2 = f32 out.  K % 128 == 0, N % 4 == 0.
 * Per-tensor-scale form (BASELINE configs[4]); the forward uses rr_op_gemm_fp8_rc's scaling. */
int rr_op_gemm_fp8(const uint8_t* A8, const uint8_t* W8, const float* bias, float scale, int M, int N, int K, int epilogue,
                   void* out, void* hip_stream);
/* The form the model forward uses: out = epi(row_scale[m] * col_scale[n] * (A8 . W8^T) + bias), activations quantised per row
 * (rr_op_layernorm_q8), weights per output channel; either scale vector may be NULL (= 1).  Large problems run the
 * persistent ring on v_mfma_scale_f32_32x32x64_f8f6f4, small ones the two-stage kernel. */
int rr_op_gemm_fp8_rc(const uint8_t* A8, const uint8_t* W8, const float* bias, const float* row_scale, const float* col_scale,
                      int M, int N, int K, int epilogue, void* out, void* hip_stream);
/* The two GEMMs of the fp8 configuration's FFN on the persistent e4m3 ring (shapes with at least 512 tiles of 256 x 256,
 * K % 128 == 0, N % 16 == 0; RR_ERR_BAD_SHAPE otherwise):
 *   rr_op_gemm_fp8_gelu_e4m3: out8[M,N] = e4m3(clamp(out_mul * gelu(row_scale[m] * col_scale[n] * (A8 . W8^T) + bias), +-448)):
 *     the GELU output under ONE static scale (the forward uses 8), the A operand of
 *   rr_op_gemm_fp8_resid: out[M,N] (f32) = scale * col_scale[n] * (A8 . W8^T) + bias + r, r = resid[M,N] when stats == NULL,
 *     else gamma * (resid - mean_m) * rstd_m + beta with stats[m] = (mean, rstd) — the fp32-stream residual epilogue of
 *     rr_op_gemm_ln_resid_f32 behind an e4m3 GEMM.  Reference seam: BertIntermediate / BertOutput of stock HF BERT. */
int rr_op_gemm_fp8_gelu_e4m3(const uint8_t* A8, const uint8_t* W8, const float* bias, const float* row_scale, const float* col_scale,
                             float out_mul, int M, int N, int K, uint8_t* out8, void* hip_stream);
int rr_op_gemm_fp8_resid(const uint8_t* A8, const uint8_t* W8, const float* bias, float scale, const float* col_scale,
                         const float* resid, const float* stats, const float* gamma, const float* beta, int M, int N, int K, float* out,
                         void* hip_stream);
/* Per-tensor e4m3 quantisation for rr_op_gemm_fp8: out[i] = e4m3(clamp(x[i] / scale, +-448)), round to nearest even;
 * x holds n (a multiple of 8) f32 values (x_is_f32 != 0) or bf16 values.  rr_op_amax: *out_dev (device float) = max |x|
 * (exact and order-independent), from which the caller derives scale = amax / 448. */
int rr_op_quantize_fp8(const void* x, int x_is_f32, float scale, uint8_t* out, size_t n, void* hip_stream);
int rr_op_amax(const void* x, int x_is_f32, size_t n, float* out_dev, void* hip_stream);
/* LayerNorm folded into the consumer GEMM (north_star "fused LayerNorm+QKV"), the two halves stand-alone:
 *   rr_op_gemm_resid_lnprep: out_f32 = A W^T + bias + resid (as rr_op_gemm_resid_f32) and, from the same epilogue, x16_out =
 *     the 16-bit copy of those rows plus per-row LayerNorm statistics stats_out[row] = (mean, rstd) of out_f32's rows
 *     (merged from per-128-column partials in part_scratch [M, ceil(N/128), 2]).  N % 8 == 0.
 *   rr_op_gemm_lnfold: out = epi(rstd_m * (A_raw W_folded^T - mean_m * csum) + dvec), epilogue 0 = 16-bit, 1 = 16-bit erf-GELU,
 *     2 = f32; with W_folded = 16bit(W * gamma), csum_n = sum_k W_folded[n,k], dvec = W beta + b this is
 *     epi(LayerNorm(x) W^T + b) for the raw rows x whose 16-bit copy is A_raw. */
int rr_op_gemm_resid_lnprep(const uint16_t* A, const uint16_t* W, const float* bias, const float* resid, int M, int N, int Kd,
                            float eps, float* out_f32, uint16_t* x16_out, float* stats_out, float* part_scratch, void* hip_stream);
/* The same residual epilogue on the SPLIT residual stream: a pre-LayerNorm row x travels as hi = its 16-bit
 * operand rounding (the consumer GEMM's A rows) + lo = fp16(x - hi) instead of a separate fp32 copy.  Residual rows come in as
 * (hi_in, lo_in) [M,N] — normalised on the fly with (ln_stats [M,2], ln_gamma, ln_beta) when ln_stats != NULL — and the output
 * rows x = A W^T + bias + residual leave as (x16_out, lo_out) plus their statistics; hi_in == x16_out and lo_in == lo_out
 * (in place) is allowed.  With the process-wide "resid_lo8" in effect (rr_set_tuning; default: on for the fp16 operand type) lo_in /
 * lo_out are e5m2 BYTES of (x - hi) * 16 in the epilogues' private layout — rows r and r + 16 of an aligned 32-row group
 * interleaved in units of 8 columns, ceil(M / 32) * 32 rows of N bytes (csrc/rr_common.h lo8_pair_offset; tests/test_gpu_ops.py
 * _lo8_to_device_layout).  Only for shapes the persistent ring kernel runs (>= 128 tiles of 256 x 256 — rr_set_tuning "gemm_ring_min_tiles" —, N % 8 == 0), otherwise
 * RR_ERR_UNSUPPORTED. */
int rr_op_gemm_resid_split(const uint16_t* A, const uint16_t* W, const float* bias, const uint16_t* hi_in, const uint16_t* lo_in,
                           const float* ln_stats, const float* ln_gamma, const float* ln_beta, int M, int N, int Kd, float eps,
                           uint16_t* x16_out, uint16_t* lo_out, float* stats_out, float* part_scratch, void* hip_stream);
/* Test support: the fp32 residual rows the split-stream epilogue forms from a (hi, lo) pair — hi + lo, LayerNorm-recomputed when
 * `stats` (mean, rstd per row) / gamma / beta are given — with the epilogue's own expression, so that rr_op_gemm_resid_lnprep fed
 * these rows is a bit-exact expectation for rr_op_gemm_resid_split (tests/test_gpu_ops.py).  hi in the operand type of
 * rr_set_op_dtype, lo fp16; cols even. */
int rr_op_split_residual_value(const uint16_t* hi, const uint16_t* lo, const float* stats, const float* gamma, const float* beta,
                               int rows, int cols, float* out, void* hip_stream);
int rr_op_gemm_lnfold(const uint16_t* A_raw, const uint16_t* W_folded, const float* dvec, const float* csum, const float* stats,
                      int M, int N, int Kd, int epilogue, void* out, void* hip_stream);
/* LayerNorm whose output is an fp8 GEMM operand: out8[row] = e4m3(LN(x[row]) / row_scale[row]), row_scale = row amax / 448,
 * stats (may be NULL) = (mean, rstd).  rr_util_quantize_rows_e4m3 is the HOST routine the weight packer uses (per output
 * channel = per row of W [rows, cols]): usable without a GPU.  A row that holds a NaN or an inf gets the scale NaN (the scale
 * multiplies the whole output column in the GEMM epilogue); rr_util_quantize_rows_i8 likewise. */
int rr_op_layernorm_q8(const float* x, const float* gamma, const float* beta, float eps, int rows, int cols, uint8_t* out8,
                       float* row_scale, float* stats, void* hip_stream);
int rr_util_quantize_rows_e4m3(const float* w_host, int rows, int cols, uint8_t* out_host, float* scales_host);
/* int8 forms of the 8-bit configuration (handle option "q8_format" = 1):
 *   rr_op_gemm_i8_rc: out[M,N] = epi(row_scale[m] * col_scale[n] * (A8 . W8^T) + bias), A8 [M,K] / W8 [N,K] signed int8 codes,
 *     int32 accumulation (exact), converted to f32 once; epilogue 0 (16-bit, operand type of rr_set_op_dtype), 1 (erf-GELU ->
 *     16-bit), 2 (f32); either scale vector may be NULL (= 1).  K % 128 == 0, N % 4 == 0; >= 512 tiles of 256 x 256 (and N % 8
 *     == 0, epilogue 0 / 1) run the persistent ring, the rest the two-stage kernel.
 *   rr_op_layernorm_i8: out8[row] = clamp(rint(LN(x[row]) / row_scale[row]), +-127), row_scale = row amax / 127 (1 for a zero
 *     row), stats (may be NULL) = (mean, rstd).
 *   rr_util_quantize_rows_i8: the HOST per-output-channel packer (amax / 127, rint, +-127); rr_util_smooth_scales: the host
 *     smoothing rule s_j = 2^round(log2(max(|gamma_j|, |beta_j|) / median)), clamped to [1, 2^10].  Both usable without a GPU. */
int rr_op_gemm_i8_rc(const int8_t* A8, const int8_t* W8, const float* bias, const float* row_scale, const float* col_scale,
                     int M, int N, int K, int epilogue, void* out, void* hip_stream);
int rr_op_layernorm_i8(const float* x, const float* gamma, const float* beta, float eps, int rows, int cols, int8_t* out8,
                       float* row_scale, float* stats, void* hip_stream);
int rr_util_quantize_rows_i8(const float* w_host, int rows, int cols, int8_t* out_host, float* scales_host);
int rr_util_smooth_scales(const float* gamma_host, const float* beta_host, int n, float* s_host);
int rr_set_gemm_variant(int variant);
/* Process-wide DIAGNOSTIC switches (A/B tools, tests): the default every handle option of the same name follows until
 * rr_set_option pins it ("ln_lite", "ln_fold", "resid_split", "resid_lo8", "ce_cls_only", "fp8_ffn_down", "q8_format", "attn_fixed_ref": see rr_set_option),
 * "q8_smooth" (1: the int8 packer of rr_finalize_weights migrates LayerNorm gain outliers into the weights; 0: plain per-channel int8),
 * plus switches that select between bit-identical kernels or only move time: "resid_fast" (default 1: plain fp32 residual GEMMs
 * on the split forms' epilogue), "resid_touch" (0: L2 touch of the next residual pass), "gemm_desync" (0: start skew of the XCDs,
 * percent of a tile period), "persistent_gemm" (1), "gemm_ring_min_tiles" (128: smallest problem, in 256 x 256 tiles, on the
 * persistent ring), "m_alternate" (1: consecutive large launches of the layer chain walk the rows in opposite directions, so that
 * a consumer starts on the rows its producer wrote last; results bit-identical either way),
 * "attn_prio" (1), "li_lds_kb" (72; 16 .. 150: the LDS bytes per workgroup, in KiB, above which the score kernels of rr_li_scores /
 * rr_bank_li_scores halve their column block; 72 keeps two workgroups per CU, 150 takes the widest block at one).  "resid_lo8": -1 (the built-in default) = by operand type (1 for fp16, 0 for bf16), 0 / 1 = for every handle that has not
 * pinned it; the environment variable RR_RESID_LO8 = 0 | 1, read once at load, replaces the built-in -1 (lets an unmodified test
 * run take either form).  Not thread-safe against running forwards; never needed on the product path. */
int rr_set_tuning(const char* key, int value);
int rr_set_op_dtype(int dt);          /* operand dtype (0 bf16 / 1 fp16) of the stand-alone rr_op_* entry points */
int rr_set_gemm_stamps(void* device_buf);
int rr_set_attn_stamps(void* device_buf);   /* diagnostic timeline of the attention kernel: 4 x 8 uint64 per workgroup, or NULL */
int rr_set_attn_redo_stats(void* device_buf);   /* diagnostic: DEVICE 2 x uint64 — the redo launches of the fixed-reference attention add (workgroups flagged for the online recompute, workgroups looked at) — or NULL */
int rr_set_gemm_stagger(int unit);   /* diagnostic codes of the 16-bit GEMM kernels, 0 = none: 1..49 start skew of the first dispatch wave in
                                       s_sleep(127) units; 50..55 tile-order groups of 2..64 row panels, 56 row-major, 57 = round 4's rule (groups of 8 also for N <= 1024); 59 = the persistent ring
                                       WITHOUT its serpentine K walk (every second block of 1 024 output columns accumulates its K-tiles from the
                                       last to the first: gemm_bf16.hip k_walk_reversed; with 59 the ring no longer agrees to the bit with the
                                       simple kernel, which keeps the rule); 61..64 timeline builds only */
int rr_op_layernorm(const float* x, const float* gamma, const float* beta, float eps, int rows, int cols,
                    float* out_f32, uint16_t* out_bf16, void* hip_stream);

/* The row and glue kernels of the forwards, stand-alone (each passes straight through to its launcher; the forwards call the
 * launchers directly).  All pointers DEVICE; every 16-bit output is in the operand type of rr_set_op_dtype.  Row kernels run one
 * wave per row: cols (D) a multiple of 4, at most 2048.  Buffers the kernel reads or writes with 16-byte (8-byte: 16-bit rows,
 * float2 statistics) accesses must be aligned to that.  What the host can check is checked before the launch: a NULL that is
 * not optional or a misaligned buffer gives RR_ERR_BAD_ARG, a size or shape the kernel cannot take RR_ERR_BAD_SHAPE; neither
 * launches anything. */
/* BertEmbeddings: row r = (word[ids[r]] + type[tts[r]]) + pos[r % S] -> LayerNorm; ids clamped to [0, vocab), token types to
 * [0, type_vocab); tts NULL = type 0.  Both outputs required. */
int rr_op_embed_ln(const int64_t* ids, const int64_t* tts, const float* word, const float* pos, const float* type,
                   const float* gamma, const float* beta, float eps, int rows, int S, int cols, int vocab, int type_vocab,
                   float* out_f32, uint16_t* out16, void* hip_stream);
/* Cross-encoder embeddings: row r (t = r % T) = (x[r] + type0) + pos[p(t)] -> LayerNorm, p(t) = t for t < s_text, else
 * vis_pos0 + t - s_text; s_text < 0 or > T: plain positions.  cls32 != 0: out_f32 written for the rows t == 0 only (out16 for
 * every row).  Both outputs required. */
int rr_op_ce_embed_ln(const float* x, const float* pos, const float* type0, const float* gamma, const float* beta, float eps,
                      int rows, int T, int cols, float* out_f32, uint16_t* out16, int s_text, int vis_pos0, int cls32,
                      void* hip_stream);
/* Late-interaction rows: destination row (p, j < rows_per_batch) = src row ((p + pair_off) / bdiv - src_batch_off, j) times its
 * mask, L2-normalised (F.normalize, eps 1e-12) when normalize != 0, cast to 16 bits into dst [n_pairs][T][D] at row
 * t_off + j + (j >= split ? shift : 0).  Mask: maskf[p * rows_per_batch + j] if maskf, else (ids[p * ids_stride + j] != 0) if
 * ids, else 1. */
int rr_op_li_normalize(const float* src, const int64_t* ids, int ids_stride, int n_pairs, int rows_per_batch, int D, int T,
                       int t_off, int pair_off, int bdiv, int src_batch_off, uint16_t* dst, int normalize, const float* maskf,
                       int split, int shift, void* hip_stream);
/* Key-padding biases (0 / -1e30): text_bias [n][S] from am != 0; ce_bias [n][T] from ids != 0 for t < S, 0 for t >= S. */
int rr_op_key_bias(const int64_t* ids, const int64_t* am, int n, int S, int T, float* text_bias, float* ce_bias, void* hip_stream);
/* RerankModel masks: text_bias [n][S] from am; li_mask [n][S] = instruction query mask (id != 0 and (s > sep or s < 2), sep =
 * first position of instruction_token clamped to >= 1; instruction_token < 0: id != 0); ce_bias [n][S + P] = that mask as a bias,
 * reordered to [query (q_len) | P zeros | rest]. */
int rr_op_joint_masks(const int64_t* ids, const int64_t* am, int n, int S, int P, int q_len, int64_t instruction_token,
                      float* text_bias, float* li_mask, float* ce_bias, void* hip_stream);
/* Interaction rerankers' biases from 0/1 masks: pair p's query mask is qmask row (p + pair_off) / K; cat_bias [n][Lq + Lc],
 * q_bias [n][Lq], c_bias [n][Lc], each optional. */
int rr_op_interaction_bias(const float* qmask, const float* cmask, int n, int Lq, int Lc, int pair_off, int K, float* cat_bias,
                           float* q_bias, float* c_bias, void* hip_stream);
/* CLIP patch im2col: px f32 [B][3][IS][IS] -> out [B * (IS / ps)^2][Kp], columns (c, ky, kx), zeros in [3 ps^2, Kp). */
int rr_op_vit_im2col(const float* px, uint16_t* out, int B, int IS, int ps, int Kp, void* hip_stream);
/* [cls_emb ; patches] + pos -> LayerNorm (fp32 only): row r = b * T + t; t = 0 takes cls_emb, t > 0 patch row b * (T - 1) + t - 1. */
int rr_op_vit_embed_ln(const float* patches, const float* cls_emb, const float* pos, const float* gamma, const float* beta,
                       float eps, int rows, int T, int cols, float* out_f32, void* hip_stream);
/* f32 [n] -> 16 bits, round to nearest even; n a multiple of 4. */
int rr_op_cast16(const float* x, uint16_t* y, int64_t n, void* hip_stream);
/* Row gather / broadcast of row_bytes-byte rows (a multiple of 16): dst row (p, j < rows_take) = src row
 * ((p + batch_off) / bdiv - src_batch_off) * src_rows_per_batch + j. */
int rr_op_gather_rows(const void* src, void* dst, int n_dst_batches, int rows_take, int src_rows_per_batch, int row_bytes,
                      int batch_off, int bdiv, int src_batch_off, void* hip_stream);
/* Classifier heads on the CLS rows: out1[p] = <h32[p * T], w1> + b1[0]; out2 (optional, then b2 too) likewise with w2 / b2.
 * w2 is read even when out2 is NULL. */
int rr_op_cls_heads(const float* h32, int T, int cols, int n_pairs, const float* w1, const float* b1, const float* w2,
                    const float* b2, float* out1, float* out2, void* hip_stream);
/* Merge per-128-column-group (mean, M2) partials [rows][nparts] (nparts = ceil(cols / 128), the last group cols - 128 (nparts - 1)
 * wide) into stats [rows] = (mean, 1 / sqrt(M2 / cols + eps)).  range_flag (optional int): OR-ed with 1 by every row whose sum of
 * squares is not below range_ss (NaN included). */
int rr_op_ln_finalize(const float* part, int nparts, int cols, float eps, int rows, float* stats, int* range_flag, float range_ss,
                      void* hip_stream);
/* Read one passage of a bank back to HOST memory: rows_out [len, li_dim] fp16 bits (a compressed bank: the decoded rows), mask_out [len] bytes (either may be NULL;
 * both NULL = only the length), buffers of capacity_rows rows.  Synchronises hip_stream (the stream the rr_bank_add calls went to)
 * and copies synchronously.  Returns the passage's length, or < 0 (RR_ERR_BAD_SHAPE: no such passage, buffers too small). */
int rr_bank_read(rr_bank_handle b, int32_t index, uint16_t* rows_out, uint8_t* mask_out, int32_t capacity_rows, void* hip_stream);
/* PLAID residual decode (the decoded row: rerank_mi355.h, rr_bank_create_plaid; replaces codecs/decompress_residuals.cu and the
 * F.normalize of third_party/ColBERT/colbert/indexing/codecs/residual.py:242-278 of the reference).
 * rr_util_plaid_decode_rows: pure HOST code, usable without a GPU, in the summation order of the kernels: the bit-level definition
 * the device is held to.  centroids_f16 [n_centroids, D] fp16 bits, bucket_weights float32 [2^nbits], codes int32 [n_rows],
 * residuals uint8 [n_rows, D * nbits / 8] -> rows_out_f16 [n_rows, D] fp16 bits.  RR_ERR_UNSUPPORTED for an nbits / D the bank does
 * not take, RR_ERR_BAD_SHAPE for a code outside [0, n_centroids).
 * rr_op_plaid_decode_rows: the same over raw DEVICE pointers, rows [first_row, first_row + n_rows) of codes / residuals (64-bit
 * row offsets) -> rows_out_f16 [n_rows, D]; the device function of the bank's gather, so its bits are the gather's.  residuals
 * 8-byte aligned, centroids and the output 16-byte aligned.  A code outside [0, n_centroids) is clamped into it (nothing outside
 * the table is read). */
int rr_util_plaid_decode_rows(const uint16_t* centroids_f16, int32_t n_centroids, const float* bucket_weights, int nbits, int D,
                              const int32_t* codes, const uint8_t* residuals, int64_t n_rows, uint16_t* rows_out_f16);
int rr_op_plaid_decode_rows(const uint16_t* centroids_f16, int32_t n_centroids, const float* bucket_weights, int nbits, int D,
                            const int32_t* codes, const uint8_t* residuals, int64_t first_row, int64_t n_rows,
                            uint16_t* rows_out_f16, void* hip_stream);
/* PLAID residual compression (the compressed row: rerank_mi355.h, rr_bank_add_compress; the reference's ResidualCodec.compress,
 * codecs/residual.py:169-221).
 * rr_util_plaid_compress_rows: pure HOST code, usable without a GPU: the definition, the score chain written as explicit fmaf in
 * the stated order.  rows [n_rows, D] float32 (dtype RR_F32) or fp16 bits (RR_F16), centroids_f16 [n_centroids, D] fp16 bits,
 * cutoffs float32 [2^nbits - 1] -> codes_out int32 [n_rows], residuals_out uint8 [n_rows, D * nbits / 8].  D a multiple of 16 in
 * [16, 512] and of 8 * nbits, nbits 1, 2, 4 or 8: RR_ERR_UNSUPPORTED otherwise.
 * rr_op_plaid_compress_rows: the two kernels of rr_bank_add_compress over raw DEVICE pointers, without a handle, at the same
 * shapes (D = 16, 32, 48, ... that no handle takes included).  rows, centroids 16-byte aligned, residuals_out 8-byte aligned;
 * cutoffs must not decrease (not checked: the bucket is found by binary search).  It allocates its scratch for the call and
 * synchronises hip_stream before it returns.
 * rr_set_tuning("compress_chunk") (0; or a multiple of 16 in [16, 2^24]): the centroids of one split of the assignment kernel; 0
 * lets the launch choose (enough splits for about four workgroups per CU, at least 256 centroids each).  The codes do not depend on it.
 * rr_set_tuning("compress_stop_after") (1; 0 or 1): 0 ends a call behind the assignment kernel (timing by difference; codes, bytes
 * and mask bytes are then not written).
 * rr_bank_read_plaid: the STORED form of one passage of a compressed bank, the raw twin of rr_bank_read: codes_out int32 [len],
 * residuals_out uint8 [len, li_dim * nbits / 8], mask_out [len] in HOST memory (any may be NULL; all NULL = only the length),
 * buffers of capacity_rows rows.  Synchronises hip_stream and copies synchronously.  Returns the length or < 0
 * (RR_ERR_UNSUPPORTED on an fp16 bank, with or without a centroid table: it holds no residuals).
 * rr_bank_read_codes: the centroid codes of one passage, codes_out int32 [len] in HOST memory (NULL = only the length), from a
 * compressed bank or an fp16 bank with a centroid table (rr_bank_set_centroids); RR_ERR_UNSUPPORTED on an fp16 bank without one.
 * Synchronises hip_stream and copies synchronously, as rr_bank_read. */
int rr_util_plaid_compress_rows(const void* rows, int dtype, int64_t n_rows, int D, const uint16_t* centroids_f16, int32_t n_centroids,
                                const float* cutoffs, int nbits, int32_t* codes_out, uint8_t* residuals_out);
int rr_op_plaid_compress_rows(const void* rows, int dtype, int64_t n_rows, int D, const uint16_t* centroids_f16, int32_t n_centroids,
                              const float* cutoffs, int nbits, int32_t* codes_out, uint8_t* residuals_out, void* hip_stream);
int rr_bank_read_plaid(rr_bank_handle b, int32_t index, int32_t* codes_out, uint8_t* residuals_out, uint8_t* mask_out,
                       int32_t capacity_rows, void* hip_stream);
int rr_bank_read_codes(rr_bank_handle b, int32_t index, int32_t* codes_out, int32_t capacity_rows, void* hip_stream);
/* PLAID codec training (THE TRAINED CENTROIDS: rerank_mi355.h, rr_plaid_kmeans).
 * rr_util_plaid_kmeans: pure HOST code, usable without a GPU: the definition, every step in the stated order.  rows [n_rows, D]
 * float32 (RR_F32) or fp16 bits (RR_F16), init_rows int32 [n_centroids] -> centroids_f16_out [n_centroids, D] fp16 bits, counts_out
 * int32 [n_centroids] or NULL, stats_out int32 [niters, 2] or NULL.  The codes of rr_plaid_kmeans: RR_ERR_BAD_DTYPE,
 * RR_ERR_UNSUPPORTED (D not a power of two in [16, 512]; n_rows > 2^30), RR_ERR_BAD_SHAPE (n_centroids outside [1, n_rows],
 * niters < 0, an initial index out of range or named twice).
 * rr_op_plaid_kmeans / rr_op_plaid_residuals: rr_plaid_kmeans / rr_plaid_residuals over raw DEVICE pointers without a handle, D given
 * (D = 16 and 32, which no handle takes, are reachable here only): the same kernels, checks and codes, no message.  They allocate
 * their scratch for the call and synchronise hip_stream before they return.
 * rr_set_tuning("kmeans_stop_after") (2; 0, 1 or 2): 0 ends every iteration of rr_plaid_kmeans behind the assignment kernel, 1
 * behind the accumulation (timing by difference; the outputs are then meaningless). */
int rr_util_plaid_kmeans(const void* rows, int dtype, int64_t n_rows, int D, const int32_t* init_rows, int32_t n_centroids, int niters,
                         uint64_t seed, uint16_t* centroids_f16_out, int32_t* counts_out, int32_t* stats_out);
int rr_op_plaid_kmeans(const void* rows, int dtype, int64_t n_rows, int D, const int32_t* init_rows_host, int32_t n_centroids, int niters,
                       uint64_t seed, uint16_t* centroids_f16_out, int32_t* counts_out, int32_t* stats_out, void* hip_stream);
int rr_op_plaid_residuals(const void* rows, int dtype, int64_t n_rows, int D, const uint16_t* centroids_f16, int32_t n_centroids,
                          int32_t* codes_out, float* residuals_out, void* hip_stream);
/* The score kernels of rr_li_scores and rr_bank_li_scores (rerank_mi355.h) over raw DEVICE pointers, at any D that is a multiple of
 * 16: a handle's li_dim is a multiple of 64, so D = 16 (one step of the kernel's walk over D) and D = 32 are reachable here only.
 * rr_op_li_scores: n pairs, query (pair index) / K; query_li [.., Lq, D], context_li [n, Lc, D], context_mask [n, Lc] float32;
 * scores_out [n, Lc, Lq] / maxsim_out [n], either may be NULL.
 * rr_op_bank_li_scores: pairs = DEVICE array [n_pairs] of {int64 first_row; int32 len; int32 query} (len <= padded_context_len;
 * NOT checked against the buffers: the caller answers for them); nbits 0: rows_f16 [rows, D] fp16 bits (8-byte aligned); nbits 1,
 * 2, 4, 8: codes / residuals / centroids_f16 / bucket_weights as rr_op_plaid_decode_rows takes them; mask_bytes [rows].
 * query_li 16-byte aligned.  RR_ERR_UNSUPPORTED for a D or nbits the kernels do not take. */
int rr_op_li_scores(const float* query_li, const float* context_li, const float* context_mask, int n, int K, int Lq, int Lc, int D,
                    float* scores_out, float* maxsim_out, void* hip_stream);
int rr_op_bank_li_scores(const float* query_li, int Lq, int D, const void* pairs, int n_pairs, int padded_context_len,
                         const uint16_t* rows_f16, const uint8_t* mask_bytes, int nbits, const int32_t* codes, const uint8_t* residuals,
                         const uint16_t* centroids_f16, const float* bucket_weights, int32_t n_centroids, float* scores_out,
                         float* maxsim_out, void* hip_stream);
/* The kernels of rr_bank_search (rerank_mi355.h) over raw DEVICE pointers, at any D that is a multiple of 16 (D = 16 is reachable
 * here only).  Both allocate their scratch per call and synchronise hip_stream before they free it.
 * rr_op_bank_search: table = DEVICE array of {int64 first_row; int32 len; int32 unused}, 16-byte aligned, one entry per passage
 * (NOT checked against the buffers: the caller answers for them); the passages first_passage .. first_passage + n_passages - 1 of
 * it are searched; rows / mask / nbits / codes / residuals / tables as rr_op_bank_li_scores takes them; indices_out int32
 * [n_queries, k] (table indices), scores_out float32 [n_queries, k] or NULL; 1 <= k <= min(n_passages, 1024).
 * rr_op_topk_select: the selection alone: scores float32 [n_lists, n] -> the first k of every list in the order of
 * torch.sort(descending=True, stable=True) (NaN first, ties by ascending index): indices_out int32 [n_lists, k], scores_out
 * float32 [n_lists, k] or NULL; n_lists <= 65535.
 * rr_op_filter_compact: the first stage of rr_bank_search_filtered_sparse alone: filter_bits as that entry takes them (DEVICE uint32
 * [filter_rows, filter_ld], bit = absolute bank index) -> cand_out int32 [filter_rows, n_passages]: the set bits of [first_passage,
 * first_passage + n_passages) of a row as ascending range-relative indices, counts_out int32 [filter_rows] their numbers; entries
 * behind a count are not written.  filter_rows 1 .. 65535, filter_ld >= ceil((first_passage + n_passages) / 32).
 * rr_op_topk_select_counted: its last stage alone: list l is the first counts[r] entries of scores float32 [n_lists, n] (r = 0 if
 * rows == 1, else l; rows is 1 or n_lists; counts int32 [rows], clamped into [0, n]); whatever lies behind a count is never read.
 * Of the entries that are not -inf the first k in rr_op_topk_select's order: indices_out int32 [n_lists, k] = first_passage +
 * cand[r][place] (cand int32 [rows, n]; NULL: first_passage + place), scores_out float32 [n_lists, k] or NULL, -1 / -inf behind
 * them, counts_out int32 [n_lists] their numbers.  1 <= k <= min(n, 1024).
 * rr_set_tuning("search_chunk") (16; 4 .. 128): the passages one workgroup of the scoring kernel walks. */
int rr_op_bank_search(const float* query_li, int n_queries, int Lq, int D, const void* table, int32_t first_passage,
                      int32_t n_passages, int k, const uint16_t* rows_f16, const uint8_t* mask_bytes, int nbits, const int32_t* codes,
                      const uint8_t* residuals, const uint16_t* centroids_f16, const float* bucket_weights, int32_t n_centroids,
                      int32_t* indices_out, float* scores_out, void* hip_stream);
int rr_op_topk_select(const float* scores, int n_lists, int n, int k, int32_t* indices_out, float* scores_out, void* hip_stream);
int rr_op_filter_compact(const uint32_t* filter_bits, int filter_rows, int64_t filter_ld, int32_t first_passage, int32_t n_passages,
                         int32_t* cand_out, int32_t* counts_out, void* hip_stream);
int rr_op_topk_select_counted(const float* scores, int n_lists, int n, const int32_t* counts, const int32_t* cand, int rows, int k,
                              int32_t first_passage, int32_t* indices_out, float* scores_out, int32_t* counts_out, void* hip_stream);

/* rr_op_bank_scores_f16: the first pass of rr_bank_search_f16 (rerank_mi355.h) alone, over raw DEVICE pointers: scores_out float32
 * [n_queries, n_passages] = A, the MaxSim of every query, rounded once to fp16, against the passages first_passage ..
 * first_passage + n_passages - 1 of `table` (as rr_op_bank_search takes it), accumulated on v_mfma_f32_16x16x32_f16
 * (csrc/bank_search_f16.hip).  rows_f16 DEVICE fp16 bits, 16-byte aligned; mask_bytes one byte per row; D a multiple of 32
 * (otherwise RR_ERR_UNSUPPORTED).  On inputs whose partial sums are all exact in float32 and whose query is exact in fp16, A is the
 * exact score bit for bit.  No scratch, no synchronisation.
 * rr_set_tuning("f16_stop_after") (3; 0 .. 3): the last stage an rr_bank_search_f16 call runs: 0 the approximate scores, 1 the
 * survivors, 2 their exact scores, 3 all; below 3 the outputs are not written (tools/bench_bank_search_f16.py times the stages). */
int rr_op_bank_scores_f16(const float* query_li, int n_queries, int Lq, int D, const void* table, int32_t first_passage,
                          int32_t n_passages, const uint16_t* rows_f16, const uint8_t* mask_bytes, float* scores_out, void* hip_stream);
/* rr_op_bank_scores_f16_plaid: the first pass of rr_bank_search_f16_plaid (rerank_mi355.h) alone: rr_op_bank_scores_f16 over the
 * rows of a compressed bank, given as rr_op_bank_li_scores takes them (mask_bytes, nbits 1, 2, 4 or 8, codes, residuals,
 * centroids_f16, bucket_weights, n_centroids; codes are clamped into [0, n_centroids)).  scores_out is BIT FOR BIT what
 * rr_op_bank_scores_f16 writes over the rows rr_op_plaid_decode_rows decodes (csrc/bank_search_f16_plaid.hip).  D 32, 64, 128 or
 * 256 (otherwise RR_ERR_UNSUPPORTED).  No scratch, no synchronisation.  rr_set_tuning("f16_stop_after") applies to
 * rr_bank_search_f16_plaid as to rr_bank_search_f16. */
int rr_op_bank_scores_f16_plaid(const float* query_li, int n_queries, int Lq, int D, const void* table, int32_t first_passage,
                                int32_t n_passages, const uint8_t* mask_bytes, int nbits, const int32_t* codes, const uint8_t* residuals,
                                const uint16_t* centroids_f16, const float* bucket_weights, int32_t n_centroids, float* scores_out,
                                void* hip_stream);
/* rr_op_bank_scores_f16_form: the launch form rr_op_bank_scores_f16 (plaid == 0) or rr_op_bank_scores_f16_plaid (plaid != 0) takes
 * for n_queries queries of Lq tokens at D, from the very host function the launch calls: *nt_out the column tiles (16 query tokens
 * each) of a workgroup's query block, *tp_out the tiles of one query in a pass (a power of two <= nt; nt / tp queries share a
 * block), *passes_out the passes over a query, ceil(ceil(Lq / 16) / tp).  The kernel instantiated is <nt, tp>.  HOST pointers.
 * Launches nothing and touches no device.  Returns what the operator returns for a refused shape: RR_ERR_UNSUPPORTED for a D it
 * does not take (fp16: not a multiple of 32; plaid: not 32, 64, 128 or 256), RR_ERR_BAD_SHAPE for n_queries or Lq out of range,
 * RR_ERR_HIP where the launch itself refuses (a D whose narrowest block does not fit the LDS), and writes nothing then. */
int rr_op_bank_scores_f16_form(int n_queries, int Lq, int D, int plaid, int* nt_out, int* tp_out, int* passes_out);

/* rr_bank_search_plaid (rerank_mi355.h) from the inside.
 * rr_op_bank_search_plaid: the stages over raw DEVICE pointers, as rr_op_bank_search takes a compressed bank's (table, mask, codes,
 * residuals, tables; codes are clamped into [0, n_centroids)); allocates its scratch per call and synchronises hip_stream.
 * rr_bank_search_plaid_tap: one intermediate of the handle's LAST rr_bank_search_plaid call, copied to HOST memory (synchronises
 * the call's stream); valid until the next search of either kind on the handle.  Returns the bytes written or < 0.  Names:
 *   "S" float32 [n_queries, n_centroids, Lq_coarse];  "cells" / "keep" uint8 [n_queries, n_centroids] (1: in the cell set / kept);
 *   "a1" float32 [n_queries, n_passages]: A1 of every passage of the range, -inf for a non-candidate;
 *   "list1" int32 [n_queries, min(ndocs, n_passages)]: the stage-1 survivors in order, range-relative, -1 behind them;
 *   "list2" int32 [n_queries, min(ndocs / 4, n_passages)]: the stage-2 survivors likewise.
 * rr_util_plaid_prune: cells, candidates, stage 1 and stage 2 of ONE query in pure HOST code, usable without a GPU: the written-
 * down definition the device is held to.  S float32 [n_centroids, Lq_coarse]; codes int32 / mask uint8 (NULL: all ones) over the
 * rows of the n_passages passages back to back, lengths int32 [n_passages].  Outputs, each optional: cells_out uint8
 * [n_centroids], a1_out / a2_out float32 [n_passages] (-inf: no candidate), list1_out int32 [min(ndocs, n_passages)] with its
 * length in n1_out, list2_out int32 [min(ndocs / 4, n_passages)] with n2_out.  RR_ERR_BAD_SHAPE for a code outside the table.
 * rr_set_tuning("plaid_stop_after") (7; 0 .. 7): the last stage a call runs (timing by difference; below 7 nothing is output).
 * rr_set_tuning("plaid_ivf_stop_after") (8; 0 .. 8): the same for rr_bank_search_plaid_ivf: 0 - 2 as above, 3 candidates, 4 the
 * listed A1 / A2, 5 the selection of ndocs, 6 the selection of ndocs / 4, 7 the exact scores, 8 the output.
 * rr_set_tuning("sparse_stop_after") (2; 0 .. 2): the last stage an rr_bank_search_filtered_sparse call runs: 0 the compaction of the
 * filter rows, 1 the scores of the places, 2 the counted selection (timing by difference; below 2 nothing is output).
 * rr_util_plaid_ivf: THE INVERTED FILE (rerank_mi355.h) in pure HOST code, usable without a GPU: the written-down definition
 * rr_bank_build_ivf is held to.  codes int32 / mask uint8 (NULL: all ones) over the rows of the n_passages passages back to back,
 * lengths int32 [n_passages] (each >= 1); codes are clamped into [0, n_centroids).  offsets_out int64 [n_centroids + 1] is always
 * written and *postings_out (or NULL) gets offsets_out[n_centroids]; pids_out (or NULL, to size it first) holds room for
 * pids_capacity entries: RR_ERR_BAD_SHAPE, with pids_out untouched, when the postings do not fit.
 * rr_bank_search_plaid_tap covers rr_bank_search_plaid_filtered as it covers rr_bank_search_plaid ("a1": -inf for a passage the
 * filter removed as for any other non-candidate).
 * rr_util_bank_filter_bits: the bitmap rr_bank_filter_fill (rerank_mi355.h, "CANDIDATE FILTERS") writes, in pure HOST code, usable
 * without a GPU: bits_out uint32 [rows][filter_ld] in host memory for a bank of `passages` passages, from indices int32 and offsets
 * int64 [rows + 1] as that call takes them.  RR_ERR_BAD_SHAPE, with bits_out untouched, for an index outside [0, passages), offsets
 * that do not start at 0 or descend, passages < 1, rows < 1 or filter_ld < ceil(passages / 32). */
int rr_op_bank_search_plaid(const float* query_li, int n_queries, int Lq, int Lq_coarse, int D, const void* table, int32_t first_passage,
                            int32_t n_passages, int ncells, float centroid_score_threshold, int ndocs, int k, const uint8_t* mask_bytes,
                            int nbits, const int32_t* codes, const uint8_t* residuals, const uint16_t* centroids_f16,
                            const float* bucket_weights, int32_t n_centroids, int32_t* indices_out, float* scores_out,
                            int32_t* counts_out, void* hip_stream);
int64_t rr_bank_search_plaid_tap(rr_handle h, const char* name, void* host_out, int64_t max_bytes);
/* rr_op_bank_export_plaid: the kernels of rr_bank_export_plaid (rerank_mi355.h) over raw DEVICE pointers, without a handle, so that
 * the row size and the table layout can be varied: table as rr_op_bank_search takes it (passages in any order, with gaps; NOT checked
 * against the buffers), the passages first_passage .. first_passage + n_passages - 1 of it; mask_bytes / codes / residuals the row
 * arrays, resid_row_bytes a power of two in [1, 512] (RR_ERR_UNSUPPORTED otherwise); residuals and residuals_out aligned to
 * min(16, resid_row_bytes).  doclens_out int32 [n_passages] and offsets_out int64 [n_passages + 1] (or NULL) on the DEVICE:
 * offsets_out[n_passages] = R.  codes_out int32 [R] / residuals_out uint8 [R, resid_row_bytes] with room for capacity_rows rows;
 * both NULL: a sizing call.  capacity_rows < R: RR_ERR_BAD_SHAPE with NO output written, doclens_out and offsets_out included.
 * Allocates its block per call and synchronises hip_stream. */
int rr_op_bank_export_plaid(const void* table, int32_t first_passage, int32_t n_passages, const uint8_t* mask_bytes, const int32_t* codes,
                            const uint8_t* residuals, int resid_row_bytes, int32_t* doclens_out, int64_t* offsets_out, int32_t* codes_out,
                            uint8_t* residuals_out, int64_t capacity_rows, void* hip_stream);
int rr_util_plaid_prune(const float* S, int32_t n_centroids, int Lq_coarse, const int32_t* codes, const uint8_t* mask,
                        const int32_t* lengths, int32_t n_passages, int ncells, float centroid_score_threshold, int ndocs,
                        uint8_t* cells_out, float* a1_out, float* a2_out, int32_t* list1_out, int32_t* n1_out, int32_t* list2_out,
                        int32_t* n2_out);
int rr_util_plaid_ivf(const int32_t* codes, const uint8_t* mask, const int32_t* lengths, int32_t n_passages, int32_t n_centroids,
                      int64_t* offsets_out, int32_t* pids_out, int64_t pids_capacity, int64_t* postings_out);
int rr_util_bank_filter_bits(const int32_t* indices, const int64_t* offsets, int rows, int exclude, int32_t passages,
                             uint32_t* bits_out, int64_t filter_ld);
/* rr_op_bank_merge_topk: the kernel of rr_bank_merge_topk (rerank_mi355.h, "THE MERGED LIST") over raw DEVICE pointers, without a
 * handle: the same arguments, the same refusals in the same order (a capturing stream included; no handle, so no sentence and no
 * profile).
 * rr_util_bank_merge_topk: THE MERGED LIST in pure HOST code, usable without a GPU: the written-down definition the kernel is held to
 * (the real entries of a query taken part by part, sorted stably by the rank key).  The same arguments over HOST arrays, the same
 * checks and refusals; a refused call writes nothing. */
int rr_op_bank_merge_topk(const int32_t* indices_in, const float* scores_in, const int32_t* counts_in, int64_t part_stride,
                          int64_t count_stride, int n_parts, const int32_t* part_offsets_host, int n_queries, int k_in, int k,
                          int32_t* indices_out, float* scores_out, int32_t* counts_out, int32_t* parts_out, void* hip_stream);
int rr_util_bank_merge_topk(const int32_t* indices_in, const float* scores_in, const int32_t* counts_in, int64_t part_stride,
                            int64_t count_stride, int n_parts, const int32_t* part_offsets, int n_queries, int k_in, int k,
                            int32_t* indices_out, float* scores_out, int32_t* counts_out, int32_t* parts_out);
/* rr_util_bank_remove_plan: what rr_bank_remove (rerank_mi355.h, "REMOVING PASSAGES") does to a bank whose n passages have
 * `lengths` (int32 [n], each >= 1) when the m distinct indices `remove` (int32 [m], each in [0, n)) go, in pure HOST code, usable
 * without a GPU: the written-down definition, and the function rr_bank_remove itself calls.  new_index_out int32 [n] (or NULL): old
 * dense index -> new, -1 for a removed passage.  moves_out int64 [moves_cap][4] (or NULL, to size it first): the moves (window,
 * src_row, dst_row, rows) in the order they are carried out: the destination rows from the first moved row on are cut into windows
 * of window_rows rows (>= 1), and every maximal run of consecutive surviving rows behind the first removed passage is cut at the
 * window borders.  A window's moves are gathered into a staging block of window_rows rows and copied to dst_row of its first move;
 * the passages in front of the first removed one give no move.  *n_moves_out (or NULL): the number of moves.  RR_ERR_BAD_SHAPE,
 * with NOTHING written, for an index outside [0, n) or given twice, a length below 1, window_rows < 1, or more moves than moves_cap.
 * rr_op_bank_move_rows: that plan carried out by rr_bank_remove's kernel and copies (csrc/bank_move.hip) on ONE raw DEVICE array of
 * sum(lengths) rows of row_bytes bytes (16-byte aligned; row_bytes a power of two or a multiple of 16, at most 1024:
 * RR_ERR_UNSUPPORTED otherwise), without a bank, so that row sizes no handle's li_dim gives (a handle takes multiples of 64) can be
 * moved: 16-byte fp16 rows of D = 8, residual rows of 1 to 8 bytes.  Afterwards the array holds the survivors' rows back to back;
 * the bytes behind them are unspecified.  The refusals of the plan (RR_ERR_BAD_SHAPE), a NULL or misaligned array and a capturing
 * stream (RR_ERR_BAD_ARG) come before anything is enqueued.  Allocates its staging per call ("bank_move_kb") and synchronises
 * hip_stream.
 * rr_set_tuning("bank_move_kb") (262144; 4 .. 1048576): the KiB of rr_bank_remove's staging block; window_rows = that over the
 * bytes of the bank's widest per-row array.  It selects no algorithm: tests reach many windows at a small shape, the bench sweeps it. */
int rr_op_bank_move_rows(void* array, int row_bytes, const int32_t* lengths_host, int32_t n, const int32_t* remove_host, int32_t m,
                         void* hip_stream);
int rr_util_bank_remove_plan(const int32_t* lengths, int32_t n, const int32_t* remove, int32_t m, int64_t window_rows,
                             int32_t* new_index_out, int64_t* moves_out, int64_t moves_cap, int64_t* n_moves_out);
#ifdef __cplusplus
}
#endif
#endif /* RERANK_MI355_DIAG_H */
