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
//
// ONE KERNEL BODY, three sources of a context tile's operand (the lane (li, g) of a wave feeds row ct * 16 + li, elements
// d + 4 g + e of it, to the matrix core; where those four floats come from is all that differs):
//   li_src_f32    rr_li_scores and the forward's fusion: padded float32 rows [n][Lc_in][D] and a float mask, query (pair0 + p) / K;
//   li_src_f16    rr_bank_li_scores on an fp16 bank: a pair list of rr_bank_pair {first_row, len, query} as the bank gathers take
//                 it, four fp16 values (one 8-byte load, requested a step ahead like the float32 rows) from
//                 rows + (first_row + c) * D with 64-bit offsets, converted to float32 (exact), the bank's mask bytes;
//   li_src_plaid  the same on a compressed bank: before its matrix instructions a wave decodes its own 16-row tile with
//                 plaid_load8 / plaid_finish8 (plaid_decode.h, THE decoded row) in passes of 64 / (D / 8) rows, every lane of the
//                 wave reaching the butterfly, stores the fp16 values into a wave-private LDS tile [16][D + 8] behind the query
//                 block (4 waves x 16 x (D + 8) x 2 bytes: 17 KB at D 128, 65 KB at D 512; the + 8 puts the 16 rows of a
//                 ds_read_b64 4 banks apart) and reads its operand from there.  No barrier: the tile belongs to one wave, whose LDS
//                 operations complete in order; wavefront-scope fences keep the compiler from moving the reads over the writes.
//                 Nothing of rows x D goes to global memory.
// A bank pair holds len rows; the rows len .. Lc - 1 are pad rows (-9999, once in the column maximum), and a tile that lies
// wholly beyond the pair's rows runs no matrix instruction and no decode (its accumulators stay zero and every row of it is
// masked; the float32 source takes the same path for Lc_in <= c < Lc).  The arithmetic of an entry is the same instruction
// sequence on the same float32 values in all three, so the three agree bit for bit on equal rows.
// LAUNCHERS: rr_launch_li_scores (li_src_f32) and rr_launch_bank_li_scores, which takes an rr_bank_view (rr_common.h) and leaves the
// choice between li_src_f16 and li_src_plaid<nbits> to li_with_bank_source.  That helper, the two bank sources, the once-per-device
// LDS attribute (li_lds_attr) and the width of the column block (li_pick_jt, here under the li_lds_kb tunable) live in li_sources.h,
// shared with bank_search.hip.  The tile step (stage, cursor, look-ahead load, the e-outer / t-inner matrix loop) is written out in
// both kernel bodies: as a shared __forceinline__ function it compiled to a different instruction stream in every instantiation.
#include "li_sources.h"    // f32x4, nan_max, half4, li_src_f16, li_src_plaid, li_with_bank_source, li_lds_attr, li_pick_jt
#include "rr_common.h"

namespace {

constexpr int LI_JT_MAX = 8;             // query tiles (16 columns) per column block: 1, 2, 4 or 8, after Lq

// ---- the sources of a context tile's operand.  open(p, D): the pair's query, its rows and how many it holds; row(pr, c, g, ..):
// the cursor of lane (li, g) on context row c (a row the pair holds), at(cur, d) its four floats of step d; keep(pr, row): the mask.
struct li_src_f32 {
  const float* context_li;
  const float* context_mask;
  int K, Lc_in, pair0;
  static constexpr bool TILE = false;
  struct pair_t { const float* rows; const float* mask; int len, query, out; };
  typedef const float* cursor;
  __device__ __forceinline__ pair_t open(int p, int D) const {
    return pair_t{context_li + (size_t)p * Lc_in * D, context_mask + (size_t)p * Lc_in, Lc_in, (pair0 + p) / K, p};
  }
  __device__ __forceinline__ cursor row(const pair_t& pr, int c, int g, int D, int li, const uint16_t*) const {
    return pr.rows + (size_t)c * D + 4 * g;
  }
  static __device__ __forceinline__ f32x4 at(cursor cur, int d) { return *(const f32x4*)(cur + d); }
  __device__ __forceinline__ bool keep(const pair_t& pr, int row) const { return pr.mask[row] != 0.0f; }
};

template <int LI_JT, class SRC>
__global__ __launch_bounds__(256) void li_scores_kernel(const float* __restrict__ query_li, const SRC src, int Lq, int Lc, int D,
                                                        float* __restrict__ scores, float* __restrict__ maxsim) {
  constexpr int LI_JB = 16 * LI_JT;      // columns per block
  extern __shared__ __attribute__((aligned(16))) float qblk[];      // [LI_JB][D + 4]: the block's query rows; TILE: the tiles behind
  const int ldq = D + 4;                 // row stride: at a handle's D (a multiple of 64) the 16 rows of a tile start 4 banks
                                         // apart; the operators' D = 16 / 32 / 48 give strides of 20 / 36 / 52 dwords (right, not tuned)
  __shared__ float colmax[4][LI_JB];
  __shared__ float blockmax[LI_JB];
  const int p = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4;
  const typename SRC::pair_t pr = src.open(p, D);
  const int Lc_in = pr.len;              // the rows the pair holds; Lc_in .. Lc - 1 are written as masked rows
  const float* Q = query_li + (size_t)pr.query * Lq * D;
  uint16_t* tile = SRC::TILE ? (uint16_t*)(qblk + LI_JB * ldq) + wave * 16 * (D + LI_TILE_PAD) : nullptr;
  float* out = scores ? scores + (size_t)pr.out * Lc * Lq : nullptr;
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
      f32x4 acc[LI_JT];
#pragma unroll
      for (int t = 0; t < LI_JT; ++t) acc[t] = zero4;
      if (ct * 16 < Lc_in) {                                // wave-uniform: a tile beyond the pair's rows holds masked rows only
        if constexpr (SRC::TILE) {
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the reads of the last tile stay in front of these writes
          src.stage(pr, ct, D, lane, tile);
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // lanes read what other lanes of the wave wrote
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        const typename SRC::cursor crow = src.row(pr, c_ok ? c : 0, g, D, li, tile);
        const float* qrow = qblk + li * ldq + 4 * g;
        f32x4 a = c_ok ? SRC::at(crow, 0) : zero4;
        for (int d = 0; d < D; d += 16) {
          // the context rows come from HBM (a compressed bank's: from the wave's LDS tile): those of step d + 16 are requested
          // before the matrix instructions of step d issue
          const f32x4 a_n = (c_ok && d + 16 < D) ? SRC::at(crow, d + 16) : zero4;
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
      }
      // accumulator element r of this lane: row ct * 16 + 4 g + r, column j0 + t * 16 + li
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = ct * 16 + 4 * g + r;
        if (row >= Lc) continue;
        const bool keep = row < Lc_in && src.keep(pr, row);
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
  if (maxsim && threadIdx.x == 0) maxsim[pr.out] = sum;
}

// rr_set_tuning("li_lds_kb"): the LDS bytes of a workgroup above which the column block is halved (72: two workgroups per CU)
std::atomic<int> g_li_lds_kb{72};

template <int JT, class SRC>
hipError_t li_launch_jt(const float* query_li, const SRC& src, int n, int Lq, int Lc, int D, size_t lds, float* scores, float* maxsim,
                        hipStream_t st) {
  static std::atomic<unsigned long long> attr_set{0};
  const hipError_t e = li_lds_attr((const void*)li_scores_kernel<JT, SRC>, attr_set);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((li_scores_kernel<JT, SRC>), dim3((unsigned)n), dim3(256), lds, st, query_li, src, Lq, Lc, D, scores, maxsim);
  return hipGetLastError();
}

// one workgroup per pair; tile_bytes: the decoded tiles of the four waves behind the query block (0 unless SRC::TILE).  The
// column block is halved above li_lds_kb (D above 128; a compressed bank at D = 128 already)
template <class SRC>
hipError_t li_launch(const float* query_li, const SRC& src, int n, int Lq, int Lc, int D, size_t tile_bytes, float* scores,
                     float* maxsim, hipStream_t st) {
  size_t lds = 0;
  const int jt = li_pick_jt(Lq, D, tile_bytes, (size_t)g_li_lds_kb.load(std::memory_order_relaxed) * 1024, &lds);
  if (jt == 0) return hipErrorInvalidValue;
  if (jt == 1) return li_launch_jt<1>(query_li, src, n, Lq, Lc, D, lds, scores, maxsim, st);
  if (jt == 2) return li_launch_jt<2>(query_li, src, n, Lq, Lc, D, lds, scores, maxsim, st);
  if (jt == 4) return li_launch_jt<4>(query_li, src, n, Lq, Lc, D, lds, scores, maxsim, st);
  return li_launch_jt<LI_JT_MAX>(query_li, src, n, Lq, Lc, D, lds, scores, maxsim, st);
}

}  // namespace

int rr_set_li_lds_kb(int kb) {
  if (kb < 16 || kb > 150) return -1;
  g_li_lds_kb.store(kb, std::memory_order_relaxed);
  return 0;
}

// n pairs from pair pair0 of the query-major pair order on; context_li / context_mask / scores / maxsim point at the first of
// them.  Lc_in rows per pair are read, Lc >= Lc_in rows per pair written (the rest as masked rows).  scores or maxsim may be null.
hipError_t rr_launch_li_scores(const float* query_li, const float* context_li, const float* context_mask, int n, int K, int Lq,
                               int Lc_in, int Lc, int D, int pair0, float* scores, float* maxsim, hipStream_t st) {
  if (n <= 0 || K <= 0 || Lq <= 0 || Lc_in <= 0 || Lc < Lc_in || D <= 0 || D % 16 || pair0 < 0 || !query_li || !context_li ||
      !context_mask || (!scores && !maxsim))
    return hipErrorInvalidValue;
  if ((((uintptr_t)query_li) | ((uintptr_t)context_li)) & 15) return hipErrorInvalidValue;   // 16-byte row loads
  return li_launch(query_li, li_src_f32{context_li, context_mask, K, Lc_in, pair0}, n, Lq, Lc, D, 0, scores, maxsim, st);
}

// the same over a pair list and a bank, fp16 or compressed (li_with_bank_source, li_sources.h): pairs [n] on the device, each
// checked on the host (first_row + len inside the bank, len <= Lc, query inside query_li); scores [n][Lc][Lq], maxsim [n], either may
// be null.  slot [n] (device) or null: workgroup p writes row slot[p] of the outputs, so that the host can start the longest
// passages first (one workgroup per pair: 800 pairs of 64 .. 512 rows on 512 slots end 20 - 25 % sooner that way,
// profiles/bank_li_scores_bench_call_order.json.log) and the caller still gets its own order; a permutation of 0 .. n - 1, checked
// by whoever builds it
hipError_t rr_launch_bank_li_scores(const rr_bank_pair* pairs, const int32_t* slot, int n, int Lq, int Lc, int D, const float* query_li,
                                    const rr_bank_view& bank, float* scores, float* maxsim, hipStream_t st) {
  if (n <= 0 || Lq <= 0 || Lc <= 0 || !pairs || !query_li || (!scores && !maxsim) || (((uintptr_t)query_li) & 15)) return hipErrorInvalidValue;
  return li_with_bank_source(pairs, slot, bank, D, [&](const auto& src, size_t tile_bytes) {
    return li_launch(query_li, src, n, Lq, Lc, D, tile_bytes, scores, maxsim, st);
  });
}
