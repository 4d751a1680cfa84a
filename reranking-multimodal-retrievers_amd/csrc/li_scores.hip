// Late-interaction score matrix and MaxSim of the frozen retriever (rr_li_scores, include/rerank_mi355.h): what colbert_score
// returns for every (query, candidate) pair (flmr_utils.py:22-48), from the tensors the interaction forward already takes.
//   scores[p][c][j] = dot(context_li[p][c][:], query_li[q][j][:]) over D, q = (pair0 + p) / K; -9999 on every row c whose
//                     context_mask is 0 and on the rows Lc_in <= c < Lc (a packed pair's pad positions) — assigned, so a
//                     masked row is -9999 whatever its embedding holds;
//   maxsim[p]       = sum_j max_c scores[p][c][j], every query token, columns summed 0, 1, ... Lq-1 by one thread.
// Exact float32 on the f32-input matrix core: one v_mfma_f32_16x16x4_f32 is a k-ordered fmaf chain, so an entry is one fixed
// fmaf chain over D whatever the launch (the lane group g of k runs over d = 16 t + 4 g + e; t, e ascending in time, g inside
// the instruction).  One workgroup of 4 waves per pair.  For a block of 16 JT query columns (JT = 1, 2, 4, 8 after Lq and D)
// the block's query rows are staged in LDS once ([16 JT][D + 4] floats: 66 KB at JT 8, D 128, two workgroups per CU).  A wave
// owns the context tiles (16 rows) wave, wave + 4, ...: it keeps JT accumulator tiles, walks D in steps of 16 (one 16-byte
// global load of its context rows, requested a step ahead, one ds_read_b128 per query tile), writes the tile rows and folds
// them into a running column maximum per query tile.  The maxima meet in LDS: lanes of one column by shuffles, the waves by
// a [4][16 JT] block, and thread 0 adds the block's columns to the pair's sum.  Traffic per pair: Lc * D * 4 read per column
// block (one block up to Lq = 128), Lc * Lq * 4 written; nothing else is stored, and without `scores` nothing but maxsim[p].
// Measured at 800 pairs of 113 x 512 x 128 (profiles/li_scores_bench.json.log): 0.22 ms, 0.21 ms without the score block,
// 54 TFLOP/s of the 155 the f32 matrix core gives.  (The first form read the query tiles from L2 in every context tile, 64 KB
// per tile pass against 32 KB of L1: 0.33 ms, and requesting the context rows ahead changed nothing there.  What is left:
// 800 workgroups on 512 slots run as two uneven rounds, and a workgroup stages its 64 KB before it computes.)
// NaN: a column maximum keeps a NaN once it has seen one (torch.max does; fmaxf would drop it), masked rows never feed it.
#include <atomic>

#include "rr_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int LI_JT_MAX = 8;             // query tiles (16 columns) per column block: 1, 2, 4 or 8, after Lq
constexpr float LI_MASKED = -9999.0f;

__device__ __forceinline__ float nan_max(float m, float v) { return (v > m || v != v) ? v : m; }

template <int LI_JT>
__global__ __launch_bounds__(256) void li_scores_kernel(const float* __restrict__ query_li, const float* __restrict__ context_li,
                                                        const float* __restrict__ context_mask, int K, int Lq, int Lc_in, int Lc,
                                                        int D, int pair0, float* __restrict__ scores, float* __restrict__ maxsim) {
  constexpr int LI_JB = 16 * LI_JT;      // columns per block
  extern __shared__ __attribute__((aligned(16))) float qblk[];      // [LI_JB][D + 4]: the block's query rows
  const int ldq = D + 4;                 // row stride: the 16 rows of a tile start 4 banks apart (D is a multiple of 64)
  __shared__ float colmax[4][LI_JB];
  __shared__ float blockmax[LI_JB];
  const int p = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4;
  const float* Q = query_li + (size_t)((pair0 + p) / K) * Lq * D;
  const float* Cx = context_li + (size_t)p * Lc_in * D;
  const float* M = context_mask + (size_t)p * Lc_in;
  float* out = scores ? scores + (size_t)p * Lc * Lq : nullptr;
  const int c_tiles = (Lc + 15) / 16;
  float sum = 0.0f;                      // thread 0 only
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  for (int j0 = 0; j0 < Lq; j0 += LI_JB) {
    float cmax[LI_JT];
#pragma unroll
    for (int t = 0; t < LI_JT; ++t) cmax[t] = -INFINITY;
    // the query rows j0 .. j0 + 16 JT - 1 of this block (zero rows beyond Lq) go to LDS once, for every context tile of the
    // pair: read from L2 by every tile instead, they were what the kernel waited for (64 KB per tile pass against 32 KB of L1)
    __syncthreads();
    for (int i = threadIdx.x; i < LI_JB * (D / 4); i += 256) {
      const int row = i / (D / 4), col = (i - row * (D / 4)) * 4;
      *(f32x4*)(qblk + row * ldq + col) = j0 + row < Lq ? *(const f32x4*)(Q + (size_t)(j0 + row) * D + col) : zero4;
    }
    __syncthreads();
    for (int ct = wave; ct < c_tiles; ct += 4) {
      const int c = ct * 16 + li;                           // the context row this lane feeds to the matrix core
      const bool c_ok = c < Lc_in;
      const float* crow = Cx + (size_t)(c_ok ? c : 0) * D + 4 * g;
      f32x4 acc[LI_JT];
#pragma unroll
      for (int t = 0; t < LI_JT; ++t) acc[t] = zero4;
      const float* qrow = qblk + li * ldq + 4 * g;
      f32x4 a = c_ok ? *(const f32x4*)crow : zero4;
      for (int d = 0; d < D; d += 16) {
        // the context rows come from HBM: those of step d + 16 are requested before the matrix instructions of step d issue
        const f32x4 a_n = (c_ok && d + 16 < D) ? *(const f32x4*)(crow + d + 16) : zero4;
        f32x4 b[LI_JT];
#pragma unroll
        for (int t = 0; t < LI_JT; ++t) b[t] = *(const f32x4*)(qrow + t * 16 * ldq + d);
        // e outside, tiles inside: consecutive instructions write different accumulators (40 cycles dependent latency, 32 issue)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
          for (int t = 0; t < LI_JT; ++t)
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[t][e], acc[t], 0, 0, 0);
        }
        a = a_n;
      }
      // accumulator element r of this lane: row ct * 16 + 4 g + r, column j0 + t * 16 + li
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = ct * 16 + 4 * g + r;
        if (row >= Lc) continue;
        const bool keep = row < Lc_in && M[row] != 0.0f;
#pragma unroll
        for (int t = 0; t < LI_JT; ++t) {
          const int j = j0 + t * 16 + li;
          if (j < Lq) {
            const float v = keep ? acc[t][r] : LI_MASKED;
            if (out) out[(size_t)row * Lq + j] = v;
            cmax[t] = nan_max(cmax[t], v);
          }
        }
      }
    }
    if (maxsim) {
#pragma unroll
      for (int t = 0; t < LI_JT; ++t) {
        float v = cmax[t];
        v = nan_max(v, __shfl_xor(v, 16, 64));
        v = nan_max(v, __shfl_xor(v, 32, 64));
        if (g == 0) colmax[wave][t * 16 + li] = v;
      }
      __syncthreads();
      if (threadIdx.x < LI_JB) {
        const int x = threadIdx.x;
        blockmax[x] = nan_max(nan_max(colmax[0][x], colmax[1][x]), nan_max(colmax[2][x], colmax[3][x]));
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        const int cols = min(LI_JB, Lq - j0);
        for (int x = 0; x < cols; ++x) sum += blockmax[x];
      }
    }
  }
  if (maxsim && threadIdx.x == 0) maxsim[p] = sum;
}

}  // namespace

// n pairs from pair pair0 of the query-major pair order on; context_li / context_mask / scores / maxsim point at the first of
// them.  Lc_in rows per pair are read, Lc >= Lc_in rows per pair written (the rest as masked rows).  scores or maxsim may be null.
hipError_t rr_launch_li_scores(const float* query_li, const float* context_li, const float* context_mask, int n, int K, int Lq,
                               int Lc_in, int Lc, int D, int pair0, float* scores, float* maxsim, hipStream_t st) {
  if (n <= 0 || K <= 0 || Lq <= 0 || Lc_in <= 0 || Lc < Lc_in || D <= 0 || D % 16 || pair0 < 0 || !query_li || !context_li ||
      !context_mask || (!scores && !maxsim))
    return hipErrorInvalidValue;
  if ((((uintptr_t)query_li) | ((uintptr_t)context_li)) & 15) return hipErrorInvalidValue;   // 16-byte row loads
  // the narrowest column block that takes Lq in one pass (a tile without a column is matrix-core time), 128 columns beyond;
  // halved while its query rows [16 JT][D + 4] would not leave room for two workgroups per CU (D above 128)
  int jt = Lq <= 16 ? 1 : Lq <= 32 ? 2 : Lq <= 64 ? 4 : LI_JT_MAX;
  auto lds_bytes = [&](int t) { return (size_t)16 * t * (D + 4) * sizeof(float); };
  while (jt > 1 && lds_bytes(jt) > 72 * 1024) jt /= 2;
  const size_t lds = lds_bytes(jt);
  if (lds > 150 * 1024) return hipErrorInvalidValue;
#define LI_LAUNCH(JT)                                                                                                          \
  do {                                                                                                                         \
    static std::atomic<unsigned long long> attr_set{0};   /* per device ordinal (see gemm_bf16.hip ensure_lds_attr) */        \
    int dev = 0;                                                                                                               \
    hipError_t e = hipGetDevice(&dev);                                                                                         \
    if (e != hipSuccess) return e;                                                                                             \
    if (dev < 0 || dev >= 64 || !((attr_set.load(std::memory_order_acquire) >> dev) & 1ull)) {                                 \
      e = hipFuncSetAttribute((const void*)li_scores_kernel<JT>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);      \
      if (e != hipSuccess) return e;                                                                                           \
      if (dev >= 0 && dev < 64) attr_set.fetch_or(1ull << dev, std::memory_order_release);                                     \
    }                                                                                                                          \
    hipLaunchKernelGGL(li_scores_kernel<JT>, dim3((unsigned)n), dim3(256), lds, st, query_li, context_li, context_mask, K, Lq, \
                       Lc_in, Lc, D, pair0, scores, maxsim);                                                                   \
  } while (0)
  if (jt == 1) LI_LAUNCH(1);
  else if (jt == 2) LI_LAUNCH(2);
  else if (jt == 4) LI_LAUNCH(4);
  else LI_LAUNCH(LI_JT_MAX);
#undef LI_LAUNCH
  return hipGetLastError();
}
