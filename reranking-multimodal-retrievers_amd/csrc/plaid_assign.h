// The nearest-centroid assignment kernel of the PLAID codec, shared by bank_compress.hip (rr_bank_add_compress: the code of THE
// COMPRESSED ROW) and plaid_train.hip (rr_plaid_kmeans: the assignment step of THE TRAINED CENTROIDS; rr_plaid_residuals).  One
// definition, so that both run the same instruction sequence on the same float32 values.
//   compress_assign_kernel    the shape of li_scores_kernel with the sides named anew: a workgroup of 4 waves stages a block
//                             of 16 JT rows in LDS as float32 after the fp16 rounding ([16 JT][D + 4], JT from li_pick_jt: 8 up
//                             to D = 128, 2 at D = 512), its waves walk the 16-row tiles of the fp16 centroid table (8-byte loads
//                             requested a step ahead, converted exactly, the e-outer / tile-inner matrix loop) and every lane
//                             folds its four accumulator rows into a running best 64-bit rank key per column tile in place of the
//                             column maximum.  The keys meet across the four lane groups by shuffles and across the waves in
//                             LDS.  grid.y splits the centroid range in chunks of `chunk` centroids (a multiple of 16, so that no
//                             tile straddles two splits; rr_set_tuning("compress_chunk")): split s writes its best key per row
//                             to keys[s][row].  A maximum over keys has one possible result, so the code does not depend on how
//                             the range is split over waves or workgroups, and nothing is atomic.
//   BIAS                      a compile-time variant: the key is taken of S[c] + bias[c], one float32 add behind the chain (k-means:
//                             bias[c] = -|c|^2 / 2 turns the largest score into the nearest centroid in L2).  bias holds a multiple
//                             of 16 entries (a lane loads the four of its accumulator rows at once).  BIAS == false is the kernel
//                             rr_bank_add_compress has always run: the variant adds nothing to its instruction stream.
// Traffic: C * D * 2 bytes of centroids per row block (from L2 after the first), 8 bytes written per row and split.
#pragma once
#include <atomic>

#include "li_sources.h"    // f32x4, half4, li_lds_attr, li_pick_jt, pack2h, load8
#include "rank_order.h"
#include "rr_common.h"

namespace {

constexpr int CP_JT_MAX = 8;

__device__ __forceinline__ unsigned long long key_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

template <int CP_JT, bool SRC_F16, bool BIAS>
__global__ __launch_bounds__(256) void compress_assign_kernel(const void* __restrict__ src, const long long* __restrict__ map,
                                                              long long R, int D, const uint16_t* __restrict__ centroids, int C,
                                                              int chunk, unsigned long long* __restrict__ keys,
                                                              const float* __restrict__ bias) {
  constexpr int JB = 16 * CP_JT;           // rows (columns of the score tile) per block
  extern __shared__ __attribute__((aligned(16))) float xblk[];      // [JB][D + 4]: the block's rows, fp16 values as float32
  const int ldq = D + 4;
  __shared__ unsigned long long wkey[4][JB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4;
  const long long j0 = (long long)blockIdx.x * JB;
  const int c_begin = (int)blockIdx.y * chunk, c_end = min(C, c_begin + chunk);
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  for (int i = threadIdx.x; i < JB * (D / 4); i += 256) {
    const int row = i / (D / 4), col = (i - row * (D / 4)) * 4;
    f32x4 v = zero4;
    if (j0 + row < R) {
      const long long s = map ? map[j0 + row] : j0 + row;
      if constexpr (SRC_F16) {
        v = half4((const uint16_t*)src + (size_t)s * D + col);
      } else {
        const f32x4 f = *(const f32x4*)((const float*)src + (size_t)s * D + col);
        const float2 a = unpack2<1>(pack2h(f[0], f[1])), b = unpack2<1>(pack2h(f[2], f[3]));      // fp16, round to nearest even
        v = f32x4{a.x, a.y, b.x, b.y};
      }
    }
    *(f32x4*)(xblk + row * ldq + col) = v;
  }
  __syncthreads();

  unsigned long long best[CP_JT];
#pragma unroll
  for (int t = 0; t < CP_JT; ++t) best[t] = 0ull;          // no entry's key: ranks behind every centroid
  const int t_end = (c_end + 15) / 16;
  for (int ct = c_begin / 16 + wave; ct < t_end; ct += 4) {
    const int c = ct * 16 + li;                             // the centroid this lane feeds to the matrix core
    const bool c_ok = c < c_end;
    f32x4 acc[CP_JT];
#pragma unroll
    for (int t = 0; t < CP_JT; ++t) acc[t] = zero4;
    const uint16_t* crow = centroids + (size_t)(c_ok ? c : c_begin) * D + 4 * g;
    const float* qrow = xblk + li * ldq + 4 * g;
    f32x4 a = c_ok ? half4(crow) : zero4;
    for (int d = 0; d < D; d += 16) {
      const f32x4 a_n = (c_ok && d + 16 < D) ? half4(crow + d + 16) : zero4;      // requested before the step's matrix instructions
      f32x4 b[CP_JT];
#pragma unroll
      for (int t = 0; t < CP_JT; ++t) b[t] = *(const f32x4*)(qrow + t * 16 * ldq + d);
      // e outside, tiles inside: consecutive instructions write different accumulators
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int t = 0; t < CP_JT; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[t][e], acc[t], 0, 0, 0);
      }
      a = a_n;
    }
    // accumulator element r of this lane: centroid ct * 16 + 4 g + r, row j0 + t * 16 + li
    f32x4 hb = zero4;
    if constexpr (BIAS) hb = *(const f32x4*)(bias + ct * 16 + 4 * g);      // padded to a multiple of 16 entries
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int cidx = ct * 16 + 4 * g + r;
      if (cidx >= c_end) continue;
#pragma unroll
      for (int t = 0; t < CP_JT; ++t) {
        float s = acc[t][r];
        if constexpr (BIAS) s += hb[r];
        best[t] = key_max(best[t], rank_key(s, (uint32_t)cidx));
      }
    }
  }
#pragma unroll
  for (int t = 0; t < CP_JT; ++t) {
    unsigned long long v = best[t];
    v = key_max(v, __shfl_xor(v, 16, 64));
    v = key_max(v, __shfl_xor(v, 32, 64));
    if (g == 0) wkey[wave][t * 16 + li] = v;
  }
  __syncthreads();
  if (threadIdx.x < JB && j0 + threadIdx.x < R) {
    const int x = threadIdx.x;
    keys[(size_t)blockIdx.y * (size_t)R + (size_t)(j0 + x)] =
        key_max(key_max(wkey[0][x], wkey[1][x]), key_max(wkey[2][x], wkey[3][x]));
  }
}

template <int JT, bool F16, bool BIAS>
hipError_t assign_launch(const void* src, const long long* map, long long R, int D, const uint16_t* centroids, int C,
                         const rr_compress_plan& pl, unsigned long long* keys, const float* bias, hipStream_t st) {
  static std::atomic<unsigned long long> attr_set{0};
  const hipError_t e = li_lds_attr((const void*)compress_assign_kernel<JT, F16, BIAS>, attr_set);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((compress_assign_kernel<JT, F16, BIAS>), dim3((unsigned)pl.row_blocks, (unsigned)pl.splits), dim3(256), pl.lds, st, src,
                     map, R, D, centroids, C, pl.chunk, keys, bias);
  return hipGetLastError();
}

// the instantiation of a plan's column block; bias == null: the plain score (BIAS false)
template <bool F16, bool BIAS>
hipError_t assign_pick(const void* src, const long long* map, long long R, int D, const uint16_t* centroids, int C,
                       const rr_compress_plan& pl, unsigned long long* keys, const float* bias, hipStream_t st) {
  if (pl.jt == 1) return assign_launch<1, F16, BIAS>(src, map, R, D, centroids, C, pl, keys, bias, st);
  if (pl.jt == 2) return assign_launch<2, F16, BIAS>(src, map, R, D, centroids, C, pl, keys, bias, st);
  if (pl.jt == 4) return assign_launch<4, F16, BIAS>(src, map, R, D, centroids, C, pl, keys, bias, st);
  return assign_launch<CP_JT_MAX, F16, BIAS>(src, map, R, D, centroids, C, pl, keys, bias, st);
}

}  // namespace
