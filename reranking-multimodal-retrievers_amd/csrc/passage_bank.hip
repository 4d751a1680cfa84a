// Passage-embedding bank of the interaction rerankers (rr_bank_*, rr_forward_interaction_bank; include/rerank_mi355.h): the
// frozen retriever's context token embeddings kept on the device as the reference hands them over, in fp16 (D = D.half(),
// src/models/flmr/models/flmr/modeling_flmr.py:1554-1555), each passage at its own length, one mask byte per row.
//
//   bank_ingest_kernel  padded [n, Lc, D] float32 / fp16 rows + float mask  ->  bank rows (fp16, round to nearest even: what
//                       .half() gives) and mask bytes, rows 0 .. len - 1 of every passage, positions unchanged.
//   bank_gather_kernel  one segment of a packed forward: the concatenated 16-bit [query | context] rows forward_interaction
//                       builds with li_normalize(normalize = 0) (a plain conversion to the handle's operand type), the query
//                       rows from query_li[pair_query], the context rows from the bank (fp16 -> float32 -> operand type, exact
//                       for fp16 handles, one rounding for bf16), zero rows beyond a passage's length; the float mask rows the
//                       bias kernel reads; and, for the attention fusion only, float32 copies of the same rows for li_scores.
//
//   bank_gather_plaid_kernel  bank_gather_kernel over a COMPRESSED bank (rr_bank_create_plaid): a context row is a ColBERTv2 /
//                       PLAID residual code (one int32 centroid index and D * nbits / 8 bytes of bucketised residual, as
//                       third_party/ColBERT/colbert/indexing/index_saver.py:33-46 of the reference writes them) and is decoded in
//                       the gather by plaid_load8 / plaid_finish8: what the reference's decompress_residuals.cu + F.normalize do
//                       (codecs/residual.py:242-278), then rounded to fp16 FIRST and converted fp16 -> float32 -> operand type as
//                       the fp16 bank's rows are, so that a compressed bank is bit for bit an fp16 bank of its decoded rows.
//   bank_decode_plaid_kernel  rows [first_row, first_row + n) decoded to fp16 by the same device function (rr_bank_read on a
//                       compressed bank, rr_op_plaid_decode_rows).
//   rr_plaid_decode_rows_host  the same arithmetic in host code (rr_util_plaid_decode_rows): the bit-level definition.
//   rr_plaid_compress_rows_host  the other direction in host code (rr_util_plaid_compress_rows): the definition bank_compress.hip's
//                       kernels are held to.
// LAUNCHERS: rr_launch_bank_ingest, rr_launch_bank_gather and rr_launch_plaid_decode.  The last two take an rr_bank_view
// (rr_common.h); the gather picks its kernel by the view's nbits.  A runtime nbits becomes a template argument in one place,
// plaid_with_nbits (plaid_decode.h), which the host decoder uses too; plaid_tables_ok there is the check of a compressed view.
//
// THE DECODED ROW (one definition, plaid_bucket / plaid_sumsq8 / the pairwise tree / plaid_finish8 of plaid_decode.h, compiled for both sides):
//   element e lies in residual byte e / (8 / nbits), group g = e % (8 / nbits) counted from the most significant end;
//   x = (byte >> (8 - nbits * (g + 1))) & (2^nbits - 1); bucket = x with its nbits bits reversed (binarize writes bit 0 first and
//   packbits fills bytes MSB-first, residual.py:188-204);  s_e = float(centroid[code][e]) + w[bucket], one float32 add;
//   sum of squares in float32: per 8-element chunk q = fmaf(s_7, s_7, ... fmaf(s_1, s_1, fmaf(s_0, s_0, 0)) ...), then the D / 8
//   chunk sums are added as a pairwise tree over neighbours (q_0 + q_1, q_2 + q_3, ... and again until one is left) — the
//   butterfly of the lane group, whose lanes all end with the same bits because a float add commutes;
//   n = sqrtf(sum), y_e = fp16_rne(s_e / fmaxf(n, 1e-12f)): correctly rounded square root and divide on both sides.
//
// All four are row kernels of one shape: a lane moves 8 elements (one 16-byte fp16 chunk; 32 bytes of a float32 source as two 16-byte loads),
// a row takes D / 8 lanes, and a wave takes 64 / (D / 8) rows (4 at D = 128, 8 at D = 64) so that no lane idles at the
// dimensions in use; four waves per 256-thread block as the row kernels of elementwise.hip.  Row offsets are 64-bit: a bank
// passes 4 GiB (2^31 elements) at 16.8 M rows of D = 128.  No LDS, no scratch.  The compressed kernels need D a power of two (the
// lane group of a row is then a power of two and the butterfly stays inside it) and never leave before the butterfly: every lane
// of a wave reaches it, loads and stores are predicated.  The bucket weights (at most 256 floats, 1 KiB) are read through the
// vector cache: a block decodes 16 - 32 rows, and filling LDS per block would cost a barrier and as many bytes as the rows do.
#include <cmath>
#include <vector>

#include "plaid_decode.h"      // load8, plaid_bucket / plaid_sumsq8 / plaid_scale, plaid_load8, plaid_finish8
#include "rank_order.h"        // rank_key: the host definition of the compressed row picks its code by it
#include "rr_common.h"

namespace {

// one lane group (lpr = D / 8 lanes) per SOURCE row (i, j) of the padded input; rows at or beyond the passage's length do nothing
template <bool SRC_F16>
__global__ __launch_bounds__(256) void bank_ingest_kernel(const void* __restrict__ src, const float* __restrict__ mask,
                                                          const rr_bank_slot* __restrict__ slots, long long n_rows, int Lc, int D,
                                                          int lpr, int rpw, uint16_t* __restrict__ rows,
                                                          uint8_t* __restrict__ mask_bytes) {
  const int lane = threadIdx.x & 63, sub = lane / lpr, c8 = lane - sub * lpr;
  if (sub >= rpw) return;
  const long long r = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * rpw + sub;
  if (r >= n_rows) return;
  const long long i = r / Lc;
  const int j = (int)(r - i * Lc);
  const rr_bank_slot s = slots[i];
  if (j >= s.len) return;
  const long long dst = s.first_row + j;
  const size_t esz = SRC_F16 ? 2 : 4;
  const char* srow = (const char*)src + (size_t)r * D * esz;
  if constexpr (SRC_F16) {
    ((uint4*)(rows + (size_t)dst * D))[c8] = ((const uint4*)srow)[c8];
  } else {
    float v[8];
    load8<false>(srow, c8, v);
    ((uint4*)(rows + (size_t)dst * D))[c8] = make_uint4(pack2h(v[0], v[1]), pack2h(v[2], v[3]), pack2h(v[4], v[5]), pack2h(v[6], v[7]));
  }
  if (c8 == 0) mask_bytes[dst] = mask[r] != 0.f ? 1 : 0;
}

// one lane group per DESTINATION row (p, t) of a segment of n pairs of T = Lq + S rows
template <int DT>
__global__ __launch_bounds__(256) void bank_gather_kernel(const rr_bank_pair* __restrict__ pairs, int n, int Lq, int S, int D, int lpr,
                                                          int rpw, const float* __restrict__ query_li,
                                                          const float* __restrict__ query_mask, const uint16_t* __restrict__ rows,
                                                          const uint8_t* __restrict__ mask_bytes, bf16_t* __restrict__ li16,
                                                          float* __restrict__ qmask_out, float* __restrict__ cmask_out,
                                                          float* __restrict__ q32_out, float* __restrict__ c32_out) {
  const int lane = threadIdx.x & 63, sub = lane / lpr, c8 = lane - sub * lpr;
  if (sub >= rpw) return;
  const int T = Lq + S;
  const long long r = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * rpw + sub;
  if (r >= (long long)n * T) return;
  const int p = (int)(r / T), t = (int)(r - (long long)p * T);
  const rr_bank_pair d = pairs[p];
  float v[8];
  float* f32 = nullptr;
  if (t < Lq) {
    const size_t q = (size_t)d.query * Lq + t;
    load8<false>(query_li + q * D, c8, v);
    if (c8 == 0) qmask_out[(size_t)p * Lq + t] = query_mask[q];
    if (q32_out) f32 = q32_out + ((size_t)p * Lq + t) * D;
  } else {
    const int j = t - Lq;
    const bool in = j < d.len;
    if (in) {
      load8<true>(rows + (size_t)(d.first_row + j) * D, c8, v);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = 0.f;
    }
    if (c8 == 0) cmask_out[(size_t)p * S + j] = (in && mask_bytes[d.first_row + j]) ? 1.0f : 0.0f;
    if (c32_out) f32 = c32_out + ((size_t)p * S + j) * D;
  }
  ((uint4*)(li16 + (size_t)r * D))[c8] =
      make_uint4(pack2<DT>(v[0], v[1]), pack2<DT>(v[2], v[3]), pack2<DT>(v[4], v[5]), pack2<DT>(v[6], v[7]));
  if (f32) {
    ((float4*)f32)[2 * c8] = make_float4(v[0], v[1], v[2], v[3]);
    ((float4*)f32)[2 * c8 + 1] = make_float4(v[4], v[5], v[6], v[7]);
  }
}

// bank_gather_kernel with the context rows decoded from a compressed bank; outputs as there
template <int DT, int NBITS>
__global__ __launch_bounds__(256) void bank_gather_plaid_kernel(const rr_bank_pair* __restrict__ pairs, int n, int Lq, int S, int D,
                                                                int lpr, int rpw, const float* __restrict__ query_li,
                                                                const float* __restrict__ query_mask, const int32_t* __restrict__ codes,
                                                                const uint8_t* __restrict__ resid, const uint16_t* __restrict__ centroids,
                                                                const float* __restrict__ weights, int C,
                                                                const uint8_t* __restrict__ mask_bytes, bf16_t* __restrict__ li16,
                                                                float* __restrict__ qmask_out, float* __restrict__ cmask_out,
                                                                float* __restrict__ q32_out, float* __restrict__ c32_out) {
  const int lane = threadIdx.x & 63, sub = lane / lpr, c8 = lane - sub * lpr;
  const int T = Lq + S;
  const long long r = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * rpw + sub;
  const bool live = sub < rpw && r < (long long)n * T;
  const long long rr = live ? r : 0;                   // a dead lane computes on row 0 and stores nothing
  const int p = (int)(rr / T), t = (int)(rr - (long long)p * T);
  const rr_bank_pair d = pairs[p];
  const int j = t - Lq;
  const bool ctx = live && j >= 0, in = ctx && j < d.len;
  float s[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = 0.f;
  if (in) plaid_load8<NBITS>(codes, resid, centroids, weights, C, d.first_row + j, D, c8, s);
  plaid_finish8(s, lpr);                               // all 64 lanes
  float* f32 = nullptr;
  if (live && !ctx) {
    const size_t q = (size_t)d.query * Lq + t;
    load8<false>(query_li + q * D, c8, s);
    if (c8 == 0) qmask_out[(size_t)p * Lq + t] = query_mask[q];
    if (q32_out) f32 = q32_out + ((size_t)p * Lq + t) * D;
  } else if (ctx) {
    if (c8 == 0) cmask_out[(size_t)p * S + j] = (in && mask_bytes[d.first_row + j]) ? 1.0f : 0.0f;
    if (c32_out) f32 = c32_out + ((size_t)p * S + j) * D;
  }
  if (live)
    ((uint4*)(li16 + (size_t)r * D))[c8] =
        make_uint4(pack2<DT>(s[0], s[1]), pack2<DT>(s[2], s[3]), pack2<DT>(s[4], s[5]), pack2<DT>(s[6], s[7]));
  if (f32) {
    ((float4*)f32)[2 * c8] = make_float4(s[0], s[1], s[2], s[3]);
    ((float4*)f32)[2 * c8 + 1] = make_float4(s[4], s[5], s[6], s[7]);
  }
}

// rows [first_row, first_row + n) of a compressed store -> out [n][D] fp16 bits
template <int NBITS>
__global__ __launch_bounds__(256) void bank_decode_plaid_kernel(const int32_t* __restrict__ codes, const uint8_t* __restrict__ resid,
                                                                const uint16_t* __restrict__ centroids,
                                                                const float* __restrict__ weights, int C, long long first_row,
                                                                long long n, int D, int lpr, int rpw, uint16_t* __restrict__ out) {
  const int lane = threadIdx.x & 63, sub = lane / lpr, c8 = lane - sub * lpr;
  const long long r = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * rpw + sub;
  const bool live = sub < rpw && r < n;
  float s[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = 0.f;
  if (live) plaid_load8<NBITS>(codes, resid, centroids, weights, C, first_row + r, D, c8, s);
  plaid_finish8(s, lpr);                               // all 64 lanes
  if (live)
    ((uint4*)(out + (size_t)r * D))[c8] = make_uint4(pack2h(s[0], s[1]), pack2h(s[2], s[3]), pack2h(s[4], s[5]), pack2h(s[6], s[7]));
}

template <int NBITS>
void plaid_decode_rows_host(const uint16_t* centroids, int C, const float* weights, int D, const int32_t* codes, const uint8_t* resid,
                            long long n_rows, uint16_t* out) {
  const int lpr = D / 8;
  float s[512], q[64];
  for (long long row = 0; row < n_rows; ++row) {
    const uint16_t* crow = centroids + (size_t)codes[row] * D;
    const uint8_t* rrow = resid + (size_t)row * ((size_t)D / 8 * NBITS);
    for (int c8 = 0; c8 < lpr; ++c8) {
      uint8_t r[NBITS];
      for (int b = 0; b < NBITS; ++b) r[b] = rrow[c8 * NBITS + b];
      float c[8];
      for (int k = 0; k < 8; ++k) {
        const uint16_t hb = crow[8 * c8 + k];                                   // fp16 bits -> float, exact
        const uint32_t sign = (uint32_t)(hb & 0x8000u) << 16, e = (hb >> 10) & 31u, m = hb & 0x3ffu;
        float v;
        if (e == 0) v = (sign ? -1.f : 1.f) * ((float)m * 5.9604644775390625e-8f);   // subnormal or zero: m * 2^-24, exact
        else if (e == 31) v = __builtin_bit_cast(float, sign | 0x7f800000u | (m << 13));
        else v = __builtin_bit_cast(float, sign | ((e + 112u) << 23) | (m << 13));
        c[k] = v + weights[plaid_bucket<NBITS>(r, k)];
      }
      for (int k = 0; k < 8; ++k) s[8 * c8 + k] = c[k];
      q[c8] = plaid_sumsq8(c);
    }
    for (int w = lpr; w > 1; w >>= 1)
      for (int i = 0; i < w / 2; ++i) q[i] = q[2 * i] + q[2 * i + 1];
    const float d = plaid_scale(sqrtf(q[0]));
    for (int e = 0; e < D; ++e) out[(size_t)row * D + e] = plaid_f16_bits(s[e] / d);
  }
}

// what a compressed bank takes: nbits in {1, 2, 4, 8}, D a power of two in [8, 512] with D % (8 * nbits) == 0 (residual.py:195)
bool plaid_shape(int nbits, int D) {
  if (nbits != 1 && nbits != 2 && nbits != 4 && nbits != 8) return false;
  return D >= 8 && D <= 512 && (D & (D - 1)) == 0 && D % (8 * nbits) == 0;
}

// lanes per row and rows per wave of a copy over rows of D elements (D % 8 == 0, D <= 512)
bool row_shape(int D, int* lpr, int* rpw) {
  if (D <= 0 || (D & 7) || D > 512) return false;
  *lpr = D / 8;
  *rpw = 64 / *lpr;
  return true;
}

}  // namespace

// the n passages of the padded source `in` (rr_common.h) into the bank's rows / mask bytes.  The caller has checked the rows against
// the capacity.
hipError_t rr_launch_bank_ingest(const rr_padded_rows& in, int D, uint16_t* rows, uint8_t* mask_bytes, hipStream_t st) {
  int lpr = 0, rpw = 0;
  if (in.n <= 0 || in.Lc <= 0 || !row_shape(D, &lpr, &rpw) || !in.src || !in.mask || !in.slots || !rows || !mask_bytes) return hipErrorInvalidValue;
  if ((((uintptr_t)in.src) | ((uintptr_t)rows)) & 15) return hipErrorInvalidValue;    // 16-byte row chunks
  const long long n_rows = (long long)in.n * in.Lc, per_block = 4LL * rpw, blocks = (n_rows + per_block - 1) / per_block;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  if (in.src_f16)
    hipLaunchKernelGGL(bank_ingest_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, in.src, in.mask, in.slots, n_rows, in.Lc, D, lpr, rpw,
                       rows, mask_bytes);
  else
    hipLaunchKernelGGL(bank_ingest_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, in.src, in.mask, in.slots, n_rows, in.Lc, D, lpr, rpw,
                       rows, mask_bytes);
  return hipGetLastError();
}

// one segment (n pairs, S context rows each) of rr_forward_interaction_bank: li16 [n][Lq + S][D] in the operand type dt,
// qmask_out [n][Lq], cmask_out [n][S]; q32_out [n][Lq][D] / c32_out [n][S][D] float32 or both null (no attention fusion).  The
// context rows come from `bank`: bank_gather_kernel on fp16 rows, bank_gather_plaid_kernel on a compressed bank's tables
hipError_t rr_launch_bank_gather(const rr_bank_pair* pairs, int n, int Lq, int S, int D, const float* query_li,
                                 const float* query_mask, const rr_bank_view& bank, bf16_t* li16, int dt, float* qmask_out,
                                 float* cmask_out, float* q32_out, float* c32_out, hipStream_t st) {
  int lpr = 0, rpw = 0;
  if (n <= 0 || Lq <= 0 || S <= 0 || !row_shape(D, &lpr, &rpw) || !pairs || !query_li || !query_mask || !bank.mask || !li16 ||
      !qmask_out || !cmask_out || (!q32_out) != (!c32_out))
    return hipErrorInvalidValue;
  if ((((uintptr_t)query_li) | ((uintptr_t)li16) | ((uintptr_t)q32_out) | ((uintptr_t)c32_out)) & 15) return hipErrorInvalidValue;
  if (bank.nbits ? !plaid_tables_ok(bank, D) : (!bank.rows || (((uintptr_t)bank.rows) & 15))) return hipErrorInvalidValue;
  const long long n_rows = (long long)n * (Lq + S), per_block = 4LL * rpw, blocks = (n_rows + per_block - 1) / per_block;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  // the two kernels take the same arguments but for where a context row comes from (src)
  auto run = [&](auto kernel, auto... src) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, st, pairs, n, Lq, S, D, lpr, rpw, query_li, query_mask, src...,
                       bank.mask, li16, qmask_out, cmask_out, q32_out, c32_out);
  };
  auto plaid = [&](auto dtc) {
    plaid_with_nbits(bank.nbits, [&](auto nb) {
      run(bank_gather_plaid_kernel<decltype(dtc)::value, decltype(nb)::value>, bank.codes, bank.resid, bank.centroids, bank.weights,
          bank.n_centroids);
    });
  };
  if (!bank.nbits) run(dt ? bank_gather_kernel<1> : bank_gather_kernel<0>, bank.rows);
  else if (dt) plaid(std::integral_constant<int, 1>{});
  else plaid(std::integral_constant<int, 0>{});
  return hipGetLastError();
}

// rows [first_row, first_row + n_rows) of a compressed bank's (codes, resid) decoded into out [n_rows][D] fp16 bits, all on the device
hipError_t rr_launch_plaid_decode(const rr_bank_view& bank, int D, long long first_row, long long n_rows, uint16_t* out, hipStream_t st) {
  int lpr = 0, rpw = 0;
  if (!plaid_tables_ok(bank, D) || !row_shape(D, &lpr, &rpw) || first_row < 0 || n_rows <= 0 || !out || (((uintptr_t)out) & 15))
    return hipErrorInvalidValue;
  const long long per_block = 4LL * rpw, blocks = (n_rows + per_block - 1) / per_block;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  plaid_with_nbits(bank.nbits, [&](auto nb) {
    hipLaunchKernelGGL(bank_decode_plaid_kernel<decltype(nb)::value>, dim3((unsigned)blocks), dim3(256), 0, st, bank.codes, bank.resid,
                       bank.centroids, bank.weights, bank.n_centroids, first_row, n_rows, D, lpr, rpw, out);
  });
  return hipGetLastError();
}

bool rr_plaid_shape_ok(int nbits, int D) { return plaid_shape(nbits, D); }

// rr_util_plaid_decode_rows: host memory throughout; false when the shape is not one plaid_shape takes or a code lies outside [0, C)
bool rr_plaid_decode_rows_host(const uint16_t* centroids, int C, const float* weights, int nbits, int D, const int32_t* codes,
                               const uint8_t* resid, long long n_rows, uint16_t* out) {
  if (!plaid_shape(nbits, D) || C <= 0) return false;
  for (long long i = 0; i < n_rows; ++i)
    if (codes[i] < 0 || codes[i] >= C) return false;
  plaid_with_nbits(nbits, [&](auto nb) {
    plaid_decode_rows_host<decltype(nb)::value>(centroids, C, weights, D, codes, resid, n_rows, out);
  });
  return true;
}

// rr_util_plaid_compress_rows: THE COMPRESSED ROW (include/rerank_mi355.h, rr_bank_add_compress) in host code, the score chain as
// explicit fmaf in the order of the matrix core (t outer in steps of 16, e, then g; d = 16 t + 4 g + e); false for a shape
// rr_plaid_compress_shape_ok does not take.  Host memory throughout.
bool rr_plaid_compress_rows_host(const void* rows, int rows_f16, long long n_rows, int D, const uint16_t* centroids, int C,
                                 const float* cutoffs, int nbits, int32_t* codes_out, uint8_t* resid_out) {
  if (!rr_plaid_compress_shape_ok(nbits, D) || C <= 0 || n_rows < 0) return false;
  std::vector<float> cf((size_t)C * D), x((size_t)D);
  for (size_t i = 0; i < cf.size(); ++i) cf[i] = plaid_f16_value(centroids[i]);
  const int n_cut = (1 << nbits) - 1;
  const size_t rb = (size_t)D / 8 * nbits;
  for (long long row = 0; row < n_rows; ++row) {
    for (int e = 0; e < D; ++e)
      x[(size_t)e] = plaid_f16_value(rows_f16 ? ((const uint16_t*)rows)[(size_t)row * D + e]
                                              : plaid_f16_bits(((const float*)rows)[(size_t)row * D + e]));
    unsigned long long best = 0;
    for (int c = 0; c < C; ++c) {
      const float* a = cf.data() + (size_t)c * D;
      float acc = 0.f;
      for (int t = 0; t < D; t += 16)
        for (int e = 0; e < 4; ++e)
          for (int g = 0; g < 4; ++g) acc = fmaf(a[t + 4 * g + e], x[(size_t)(t + 4 * g + e)], acc);
      const unsigned long long key = rank_key(acc, (uint32_t)c);
      if (key > best) best = key;
    }
    const int code = (int)rank_key_index(best);
    codes_out[row] = code;
    uint8_t* out = resid_out + (size_t)row * rb;
    for (size_t i = 0; i < rb; ++i) out[i] = 0;
    for (int e = 0; e < D; ++e) {
      const float res = x[(size_t)e] - cf[(size_t)code * D + e];
      int bucket = 0;
      for (int j = 0; j < n_cut; ++j) bucket += cutoffs[j] < res ? 1 : 0;
      for (int j = 0; j < nbits; ++j) {
        const size_t p = (size_t)e * nbits + j;            // np.packbits: bit j of the bucket, bit 0 first, bytes from the top
        out[p >> 3] |= (uint8_t)(((bucket >> j) & 1) << (7 - (p & 7)));
      }
    }
  }
  return true;
}
