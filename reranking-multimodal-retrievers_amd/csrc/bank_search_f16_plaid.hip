// The first pass of rr_bank_search_f16_plaid (include/rerank_mi355.h): bank_scores_f16_kernel (bank_search_f16.hip) over a COMPRESSED
// bank.  A decoded row is fp16 by definition (plaid_finish8: fp16 FIRST), so the decoded rows feed v_mfma_f32_16x16x32_f16 as the rows
// of an fp16 bank do, and A is BIT FOR BIT what rr_launch_bank_scores_f16 gives over the decoded rows: the slack bound and the
// measured accumulation constant of rr_bank_search_f16 stand for this kernel without a measurement of its own.
//
// bank_scores_f16_plaid_kernel<NBITS, LPR, NT, TP>.  The grid (a chunk of F16P_CHUNK passages x the query blocks, blockIdx = chunk * query
// blocks + query block), the staging of the block's query rows ([16 NT][D + F16P_PAD] fp16, rounded once), the B fragments, the passes
// over a query of more than NT tiles (psum) and the epilogue are bank_scores_f16_kernel's, COPIED (li_sources.h: code moved into
// shared helpers has changed the instruction streams of existing kernels before; that kernel keeps its registers and occupancy).
// What differs is where the A operand comes from: a row is decoded once per QUERY BLOCK, not once per query as rr_bank_search does.
//   DECODE INTO LDS.  A wave takes whole passages, two 16-row tiles at a time, and first decodes those (up to) 32 rows into its own
// LDS tile [32][D + F16P_PAD] fp16 as li_src_plaid::stage does: D / 8 lanes per row, 64 / (D / 8) rows per pass, wave-uniform
// passes in which EVERY lane reaches plaid_finish8 (its butterfly is cross-lane), stores predicated, codes clamped (plaid_load8).
// Unlike stage, the kernel is compiled per D (LPR = D / 8) and writes the passes of a batch out in straight-line code with the
// loads clamped to the passage's last row instead of predicated (f16p_stage says why), and reads the bucket weights from a copy
// in LDS.  Rows behind the passage's length are not stored and never read: their lanes feed zeros, as in the fp16 kernel.  The
// tile is wave-private: no workgroup barrier, the wave waits for its own LDS writes (wavefront fences around the staging, as bank_search_scores_kernel has them).
//   THE A FRAGMENT of row tile u and k-step s is one ds_read_b128 per lane: lane l holds row 16 u + (l & 15), elements 32 s +
// 8 (l >> 4) + j: the very access of the B fragment, on a tile of the same row pitch.  THE PAD argument of bank_search_f16.hip
// therefore applies to this layout unchanged: D + 16 fp16 is 2 (mod 4) slots of 16 bytes, no bank conflict in any 16-lane group.
//   THE SAME CHAIN.  For a (row tile, column tile) one accumulator takes k-steps 0, 32, ... in order, on the operand bits the fp16
// kernel would load from global memory: equal bits in, equal bits out (tests/test_gpu_bank_search_f16_plaid.py holds it to that
// with torch.equal).
//   LDS.  At D 128 the query block (NT 8) takes 36 KB and the four tiles 36 KB: two workgroups per CU.  The query block shrinks as
// rr_launch_bank_scores_f16's does (64 KB), then until block and tiles fit 72 KB or, failing that, 150 KB.  D 512 IS REFUSED: its
// four tiles alone are 132 KB and leave room for one column tile; accepted are D 32, 64, 128 and 256 (a power of two, so that the
// lanes of a row are an aligned group of the butterfly, and a multiple of 32, the k-step).
#include <atomic>

#include "li_sources.h"
#include "rank_order.h"
#include "rr_common.h"

namespace {

constexpr int F16P_NT_MAX = 8;           // column tiles (16 query tokens) of a query block
constexpr int F16P_CHUNK = 32;           // passages of a workgroup's chunk (psum): F16_CHUNK of bank_search_f16.hip
constexpr int F16P_PAD = 16;             // fp16 values behind a row in LDS, query rows and decoded rows alike (see THE PAD)
constexpr int F16P_D_MAX = 256;
#ifndef F16P_BATCH_N
#define F16P_BATCH_N 4
#endif
constexpr int F16P_BATCH = F16P_BATCH_N;    // passes of a batch of the decode (f16p_stage).  Measured at D 128, Lq 32:
                                            // 8 is faster at one query, 4 at sixteen and sixty-four

__device__ __forceinline__ f16x8 lds_f16x8(const uint16_t* p) { return __builtin_bit_cast(f16x8, *(const uint4*)p); }

template <int NBITS>
struct f16p_tables {
  const int32_t* codes;
  const uint8_t* resid;
  const uint16_t* centroids;
  const float* weights;
  int C;
};

// rows c0 .. c0 + 16 R - 1 of the passage at first_row (those below len) decoded into tile [16 R][ldt].  LPR = D / 8 lanes per row,
// 64 / LPR rows per pass, the passes of a batch (up to F16P_BATCH) written out in straight-line code: a lane whose row lies behind the passage
// loads the passage's LAST row instead (in bounds, len >= 1) and stores nothing, so no load sits behind a branch and the requests of
// a whole batch (codes, then residual bytes and centroid chunks) are in flight together: with two waves per SIMD resident the
// decode is bound by the latency of that chain, not by its bytes.  The lanes of a row are an aligned group of LPR: what a lane
// without a row of its own feeds the butterfly of plaid_finish8 stays inside its group.  `weights` is the workgroup's LDS copy.
template <int NBITS, int LPR, int R>
__device__ __forceinline__ void f16p_stage(const f16p_tables<NBITS>& tb, const float* weights, long long first_row, int len, int c0, int ldt,
                                           int lane, uint16_t* tile) {
  constexpr int D = 8 * LPR, RPW = 64 / LPR, PASSES = 16 * R / RPW, B = PASSES < F16P_BATCH ? PASSES : F16P_BATCH;
  const int sub = lane / LPR, c8 = lane - sub * LPR;
#pragma unroll
  for (int p0 = 0; p0 < PASSES; p0 += B) {
    float s[B][8];
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const int c = c0 + (p0 + b) * RPW + sub;
      plaid_load8<NBITS>(tb.codes, tb.resid, tb.centroids, weights, tb.C, first_row + min(c, len - 1), D, c8, s[b]);
    }
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const int r = (p0 + b) * RPW + sub;
      plaid_finish8(s[b], LPR);                            // all 64 lanes; s now holds fp16 values, packing them is exact
      if (c0 + r < len)
        *(uint4*)(tile + r * ldt + 8 * c8) =
            make_uint4(pack2h(s[b][0], s[b][1]), pack2h(s[b][2], s[b][3]), pack2h(s[b][4], s[b][5]), pack2h(s[b][6], s[b][7]));
    }
  }
}

// f16_tiles of bank_search_f16.hip with the A fragments read from the wave's decoded tile
template <int NT, int TP, int R>
__device__ __forceinline__ void f16p_tiles(const uint16_t* tile, int ldt, const uint8_t* __restrict__ pmask, int len, int c0, int D, int ldq,
                                           const uint16_t* bq, int li, int g, int col_lim, float (&cmax)[NT]) {
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const f16x8 zero8 = __builtin_bit_cast(f16x8, make_uint4(0u, 0u, 0u, 0u));
  f32x4 acc[R][NT];
  const uint16_t* ap[R];
  bool ok[R];
  f16x8 a[R];
#pragma unroll
  for (int u = 0; u < R; ++u) {
    ok[u] = c0 + 16 * u + li < len;                            // the context row this lane feeds to the matrix core is decoded
    ap[u] = tile + (16 * u + li) * ldt + 8 * g;
    a[u] = ok[u] ? lds_f16x8(ap[u]) : zero8;
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[u][t] = zero4;
  }
  for (int d = 0; d < D; d += 32) {
    f16x8 a_n[R];
#pragma unroll
    for (int u = 0; u < R; ++u) a_n[u] = (ok[u] && d + 32 < D) ? lds_f16x8(ap[u] + d + 32) : zero8;      // requested a step ahead
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const f16x8 b = __builtin_bit_cast(f16x8, *(const uint4*)(bq + t * 16 * ldq + d));
#pragma unroll
      for (int u = 0; u < R; ++u) acc[u][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[u], b, acc[u][t], 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < R; ++u) a[u] = a_n[u];
  }
  // accumulator element r of this lane: row c0 + 16 u + 4 g + r, column tile t, column li of it
#pragma unroll
  for (int u = 0; u < R; ++u) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = c0 + 16 * u + 4 * g + r;
      if (row >= len) continue;
      const bool keep = pmask[row] != 0;
#pragma unroll
      for (int t = 0; t < NT; ++t)
        if (((t & (TP - 1)) << 4) + li < col_lim) cmax[t] = nan_max(cmax[t], keep ? acc[u][t][r] : LI_MASKED);
    }
  }
}

// the staging of R row tiles between the fences a wave-private tile needs, then their products
template <int NBITS, int LPR, int NT, int TP, int R>
__device__ __forceinline__ void f16p_step(const f16p_tables<NBITS>& tb, const float* weights, long long first_row, uint16_t* tile, int ldt,
                                          const uint8_t* __restrict__ pmask, int len, int c0, int D, int ldq, const uint16_t* bq, int lane, int li,
                                          int g, int col_lim, float (&cmax)[NT]) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the reads of the last tiles stay in front of these writes
  f16p_stage<NBITS, LPR, R>(tb, weights, first_row, len, c0, ldt, lane, tile);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // lanes read what other lanes of the wave wrote
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  f16p_tiles<NT, TP, R>(tile, ldt, pmask, len, c0, D, ldq, bq, li, g, col_lim, cmax);
}

// Two waves per SIMD is what the LDS of a launch at D 128 allows, so the kernel is compiled for that (amdgpu_waves_per_eu): the
// accumulators then lie in the unified register file beside the batch of the decode, within 256 registers and without scratch
// (profiles/bank_f16_plaid_kernel_resources.txt; without the attribute the NT 8, TP 8 form took 264 and one wave per SIMD).
template <int NBITS, int LPR, int NT, int TP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void bank_scores_f16_plaid_kernel(
    const float* __restrict__ query_li, const f16p_tables<NBITS> tb, const uint8_t* __restrict__ mask_bytes, const rr_bank_slot* __restrict__ table,
    int n, int nq, int nqb, int Lq, float* __restrict__ out) {
  constexpr int tp = TP;                 // tiles of one query in a pass (a power of two, <= NT)
  constexpr int D = 8 * LPR;
  __shared__ float wl[1 << NBITS];       // the bucket weights: eight lookups per lane and pass, from LDS
  if (threadIdx.x < (1 << NBITS)) wl[threadIdx.x] = tb.weights[threadIdx.x];      // (read behind the barriers of the first pass)
  extern __shared__ __attribute__((aligned(16))) uint16_t qh[];      // [16 NT][D + F16P_PAD] the block's query rows, fp16; behind them
                                                                     // [4][32][D + F16P_PAD] the waves' decoded tiles
  __shared__ float psum[F16P_CHUNK];     // the running sum of the workgroup's passages between passes (one query per block then)
  const int ldq = D + F16P_PAD, d8n = D / 8;
  const int qb = blockIdx.x % nqb, p0 = (blockIdx.x / nqb) * F16P_CHUNK, pn = min(F16P_CHUNK, n - p0);
  const int q0 = qb * (NT / tp);         // the block's first query
  const int passes = ((Lq + 15) / 16 + tp - 1) / tp;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, g = lane >> 4;
  uint16_t* tile = qh + 16 * NT * ldq + wave * 32 * ldq;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  for (int ps = 0; ps < passes; ++ps) {
    const int j0 = ps * tp * 16;         // the first token of the pass, in every query of the block
    __syncthreads();                     // every wave is done with the last pass's query rows (and psum is written)
    for (int i = threadIdx.x; i < 16 * NT * d8n; i += 256) {
      const int col = i / d8n, d8 = (i - col * d8n) * 8, t = col >> 4;
      const int q = q0 + t / tp, tok = j0 + ((t & (tp - 1)) << 4) + (col & 15);
      f32x4 x = zero4, y = zero4;
      if (q < nq && tok < Lq) {
        const float* s = query_li + ((size_t)q * Lq + tok) * D + d8;
        x = *(const f32x4*)s;
        y = *(const f32x4*)(s + 4);
      }
      *(uint4*)(qh + col * ldq + d8) = make_uint4(pack2h(x[0], x[1]), pack2h(x[2], x[3]), pack2h(y[0], y[1]), pack2h(y[2], y[3]));
    }
    __syncthreads();
    const bool last = ps + 1 == passes;
    const int col_lim = Lq - j0;         // the columns of a query this pass still holds
    const uint16_t* bq = qh + li * ldq + 8 * g;
    for (int i = wave; i < pn; i += 4) {                        // a passage belongs to one wave
      const rr_bank_slot sl = table[p0 + i];                    // the same entry in every lane: kept in scalar registers
      const long long first_row = uniform_i64(sl.first_row);
      const int len = __builtin_amdgcn_readfirstlane(sl.len), c_tiles = (len + 15) / 16;
      const uint8_t* pmask = mask_bytes + first_row;
      float cmax[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) cmax[t] = -INFINITY;
      int ct = 0;
      for (; ct + 2 <= c_tiles; ct += 2) f16p_step<NBITS, LPR, NT, TP, 2>(tb, wl, first_row, tile, ldq, pmask, len, ct * 16, D, ldq, bq, lane, li, g, col_lim, cmax);
      if (ct < c_tiles) f16p_step<NBITS, LPR, NT, TP, 1>(tb, wl, first_row, tile, ldq, pmask, len, ct * 16, D, ldq, bq, lane, li, g, col_lim, cmax);
      float sum = 0.0f;                                         // every lane of the wave carries the same sum
      int cl = col_lim;
      asm volatile("" : "+s"(cl));                              // (as bank_scores_f16_kernel: else the column tests are hoisted and spill)
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int tt = t & (tp - 1);
        if (tt == 0) sum = ps ? psum[i] : 0.0f;                 // a query begins
        float v = cmax[t];
        v = nan_max(v, __shfl_xor(v, 16, 64));
        v = nan_max(v, __shfl_xor(v, 32, 64));
#pragma unroll
        for (int l = 0; l < 16; ++l) {
          const float x = __shfl(v, l, 64);
          if ((tt << 4) + l < cl) sum += x;               // columns 0, 1, ... Lq - 1, one after the other
        }
        if (tt == tp - 1 && lane == 0) {
          const int q = q0 + t / tp;
          if (!last) psum[i] = sum;
          else if (q < nq) out[(size_t)q * n + p0 + i] = sum;
        }
        __builtin_amdgcn_sched_barrier(0);                      // a tile's sixteen lane reads at a time
      }
    }
  }
}

template <int NBITS, int LPR, int NT, int TP>
hipError_t f16p_launch_nt(const float* query_li, const rr_bank_view& bank, const rr_bank_slot* table, int n, int nq, int nqb, int Lq, size_t lds,
                          float* out, hipStream_t st) {
  static std::atomic<unsigned long long> attr_set{0};
  const hipError_t e = li_lds_attr((const void*)bank_scores_f16_plaid_kernel<NBITS, LPR, NT, TP>, attr_set);
  if (e != hipSuccess) return e;
  const long long blocks = (((long long)n + F16P_CHUNK - 1) / F16P_CHUNK) * nqb;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const f16p_tables<NBITS> tb{bank.codes, bank.resid, bank.centroids, bank.weights, bank.n_centroids};
  hipLaunchKernelGGL((bank_scores_f16_plaid_kernel<NBITS, LPR, NT, TP>), dim3((unsigned)blocks), dim3(256), lds, st, query_li, tb, bank.mask, table, n,
                     nq, nqb, Lq, out);
  return hipGetLastError();
}

// the (NT, TP) of a launch at LPR lanes per row; NT_MAX: the widest query block the LDS leaves at that D
template <int NBITS, int LPR, int NT_MAX>
hipError_t f16p_launch_d(int nt, int tp, const float* query_li, const rr_bank_view& bank, const rr_bank_slot* table, int n, int nq, int nqb, int Lq,
                         size_t lds, float* out, hipStream_t st) {
#define F16P_CASE(NT_, TP_)                           \
  if constexpr (NT_ <= NT_MAX)                        \
    if (nt == NT_ && tp == TP_) return f16p_launch_nt<NBITS, LPR, NT_, TP_>(query_li, bank, table, n, nq, nqb, Lq, lds, out, st)
  F16P_CASE(1, 1); F16P_CASE(2, 1); F16P_CASE(2, 2); F16P_CASE(4, 1); F16P_CASE(4, 2); F16P_CASE(4, 4);
  F16P_CASE(8, 1); F16P_CASE(8, 2); F16P_CASE(8, 4); F16P_CASE(8, 8);
#undef F16P_CASE
  return hipErrorInvalidValue;
}

int f16p_pow2_ceil(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

size_t f16p_tile_bytes(int D) { return (size_t)4 * 32 * (D + F16P_PAD) * sizeof(uint16_t); }                  // the four waves' decoded tiles
size_t f16p_q_bytes(int nt, int D) { return (size_t)16 * nt * (D + F16P_PAD) * sizeof(uint16_t); }           // the block's query rows

}  // namespace

bool rr_bank_scores_f16_plaid_dim_ok(int D) { return D >= 32 && D <= F16P_D_MAX && !(D & (D - 1)); }

// The form of a launch of bank_scores_f16_plaid_kernel, as rr_bank_scores_f16_form gives the fp16 kernel's; the D-dependent cap of
// the block (the four decoded tiles share the LDS with it) is part of it.  Host arithmetic alone.
hipError_t rr_bank_scores_f16_plaid_form(int nq, int Lq, int D, int* nt_out, int* tp_out, int* passes_out) {
  if (nq <= 0 || Lq <= 0 || !rr_bank_scores_f16_plaid_dim_ok(D)) return hipErrorInvalidValue;
  const size_t tile_bytes = f16p_tile_bytes(D);
  int nt = F16P_NT_MAX;
  while (nt > 1 && f16p_q_bytes(nt, D) > (size_t)64 * 1024) nt /= 2;           // as rr_bank_scores_f16_form
  int nt2 = nt;                                                                // two workgroups per CU where a block allows it
  while (nt2 > 1 && f16p_q_bytes(nt2, D) + tile_bytes > (size_t)72 * 1024) nt2 /= 2;
  if (f16p_q_bytes(nt2, D) + tile_bytes <= (size_t)72 * 1024) nt = nt2;
  while (nt > 1 && f16p_q_bytes(nt, D) + tile_bytes > (size_t)150 * 1024) nt /= 2;
  if (f16p_q_bytes(nt, D) + tile_bytes > (size_t)150 * 1024) return hipErrorInvalidValue;
  const int tiles = (Lq + 15) / 16;
  const int tp = std::min(f16p_pow2_ceil(tiles), nt);               // tiles of one query in a pass
  nt = (int)std::min<long long>(nt, (long long)tp * f16p_pow2_ceil(nq));      // no wider than the call's queries
  *nt_out = nt;
  *tp_out = tp;
  *passes_out = (tiles + tp - 1) / tp;                              // as the kernel counts them
  return hipSuccess;
}

// out [nq][n]: the approximate MaxSim (fp16 matrix core) of every query against the passages table[0 .. n) of a compressed bank
hipError_t rr_launch_bank_scores_f16_plaid(const rr_bank_slot* table, int n, int nq, int Lq, int D, const float* query_li, const rr_bank_view& bank,
                                           float* out, hipStream_t st) {
  if (n <= 0 || nq <= 0 || Lq <= 0 || !rr_bank_scores_f16_plaid_dim_ok(D) || !table || !query_li || !out || !bank.nbits || !bank.mask ||
      !plaid_tables_ok(bank, D))
    return hipErrorInvalidValue;
  if ((((uintptr_t)query_li) | ((uintptr_t)table)) & 15) return hipErrorInvalidValue;
  int nt = 0, tp = 0, passes = 0;
  const hipError_t fe = rr_bank_scores_f16_plaid_form(nq, Lq, D, &nt, &tp, &passes);
  if (fe != hipSuccess) return fe;
  const int qpb = nt / tp, nqb = (nq + qpb - 1) / qpb;
  const size_t lds = f16p_q_bytes(nt, D) + f16p_tile_bytes(D);
  return plaid_with_nbits(bank.nbits, [&](auto nb) -> hipError_t {
    constexpr int NB = decltype(nb)::value;
    if constexpr (NB <= 4)
      if (D == 32) return f16p_launch_d<NB, 4, 8>(nt, tp, query_li, bank, table, n, nq, nqb, Lq, lds, out, st);      // (nbits 8: D from 64)
    if (D == 64) return f16p_launch_d<NB, 8, 8>(nt, tp, query_li, bank, table, n, nq, nqb, Lq, lds, out, st);
    if (D == 128) return f16p_launch_d<NB, 16, 8>(nt, tp, query_li, bank, table, n, nq, nqb, Lq, lds, out, st);
    if (D == 256) return f16p_launch_d<NB, 32, 4>(nt, tp, query_li, bank, table, n, nq, nqb, Lq, lds, out, st);
    return hipErrorInvalidValue;
  });
}
