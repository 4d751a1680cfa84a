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
// Both are copy kernels: a lane moves 8 elements (one 16-byte fp16 chunk; 32 bytes of a float32 source as two 16-byte loads),
// a row takes D / 8 lanes, and a wave takes 64 / (D / 8) rows (4 at D = 128, 8 at D = 64) so that no lane idles at the
// dimensions in use; four waves per 256-thread block as the row kernels of elementwise.hip.  Row offsets are 64-bit: a bank
// passes 4 GiB (2^31 elements) at 16.8 M rows of D = 128.  No LDS, no scratch.
#include "rr_common.h"

namespace {

__device__ __forceinline__ uint32_t pack2h(float lo, float hi) { return pack2<1>(lo, hi); }

// 8 consecutive elements of a source row as floats; SRC_F16: the row holds fp16 bits
template <bool SRC_F16>
__device__ __forceinline__ void load8(const void* row, int c8, float (&v)[8]) {
  if constexpr (SRC_F16) {
    const uint4 u = ((const uint4*)row)[c8];
    const float2 a = unpack2<1>(u.x), b = unpack2<1>(u.y), c = unpack2<1>(u.z), d = unpack2<1>(u.w);
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y; v[4] = c.x; v[5] = c.y; v[6] = d.x; v[7] = d.y;
  } else {
    const float4 a = ((const float4*)row)[2 * c8], b = ((const float4*)row)[2 * c8 + 1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
}

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

// lanes per row and rows per wave of a copy over rows of D elements (D % 8 == 0, D <= 512)
bool row_shape(int D, int* lpr, int* rpw) {
  if (D <= 0 || (D & 7) || D > 512) return false;
  *lpr = D / 8;
  *rpw = 64 / *lpr;
  return true;
}

}  // namespace

// n passages of the padded source [n, Lc, D] (src_f16: fp16 bits, else float32) and mask [n, Lc] into the bank's rows / mask
// bytes; slots[i] = (first destination row, length) on the device.  The caller has checked the rows against the capacity.
hipError_t rr_launch_bank_ingest(const void* src, int src_f16, const float* mask, const rr_bank_slot* slots, int n, int Lc, int D,
                                 uint16_t* rows, uint8_t* mask_bytes, hipStream_t st) {
  int lpr = 0, rpw = 0;
  if (n <= 0 || Lc <= 0 || !row_shape(D, &lpr, &rpw) || !src || !mask || !slots || !rows || !mask_bytes) return hipErrorInvalidValue;
  if ((((uintptr_t)src) | ((uintptr_t)rows)) & 15) return hipErrorInvalidValue;       // 16-byte row chunks
  const long long n_rows = (long long)n * Lc, per_block = 4LL * rpw, blocks = (n_rows + per_block - 1) / per_block;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  if (src_f16)
    hipLaunchKernelGGL(bank_ingest_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, src, mask, slots, n_rows, Lc, D, lpr, rpw,
                       rows, mask_bytes);
  else
    hipLaunchKernelGGL(bank_ingest_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, src, mask, slots, n_rows, Lc, D, lpr, rpw,
                       rows, mask_bytes);
  return hipGetLastError();
}

// one segment (n pairs, S context rows each) of rr_forward_interaction_bank: li16 [n][Lq + S][D] in the operand type dt,
// qmask_out [n][Lq], cmask_out [n][S]; q32_out [n][Lq][D] / c32_out [n][S][D] float32 or both null (no attention fusion)
hipError_t rr_launch_bank_gather(const rr_bank_pair* pairs, int n, int Lq, int S, int D, const float* query_li,
                                 const float* query_mask, const uint16_t* rows, const uint8_t* mask_bytes, bf16_t* li16, int dt,
                                 float* qmask_out, float* cmask_out, float* q32_out, float* c32_out, hipStream_t st) {
  int lpr = 0, rpw = 0;
  if (n <= 0 || Lq <= 0 || S <= 0 || !row_shape(D, &lpr, &rpw) || !pairs || !query_li || !query_mask || !rows || !mask_bytes ||
      !li16 || !qmask_out || !cmask_out || (!q32_out) != (!c32_out))
    return hipErrorInvalidValue;
  if ((((uintptr_t)query_li) | ((uintptr_t)rows) | ((uintptr_t)li16) | ((uintptr_t)q32_out) | ((uintptr_t)c32_out)) & 15)
    return hipErrorInvalidValue;
  const long long n_rows = (long long)n * (Lq + S), per_block = 4LL * rpw, blocks = (n_rows + per_block - 1) / per_block;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  if (dt)
    hipLaunchKernelGGL(bank_gather_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, pairs, n, Lq, S, D, lpr, rpw, query_li,
                       query_mask, rows, mask_bytes, li16, qmask_out, cmask_out, q32_out, c32_out);
  else
    hipLaunchKernelGGL(bank_gather_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, st, pairs, n, Lq, S, D, lpr, rpw, query_li,
                       query_mask, rows, mask_bytes, li16, qmask_out, cmask_out, q32_out, c32_out);
  return hipGetLastError();
}
