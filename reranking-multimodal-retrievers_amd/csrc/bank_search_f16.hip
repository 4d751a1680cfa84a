// The first pass of rr_bank_search_f16 (include/rerank_mi355.h): A[q][p], the MaxSim of every query against every passage of a range
// of an fp16 bank, on v_mfma_f32_16x16x32_f16.  An APPROXIMATION of what bank_search_scores_kernel (bank_search.hip) computes: the
// query is rounded once to fp16 (round to nearest even, as the reference's GPU branch does with Q.half()); a bank row is fp16 as it
// lies in memory; a product of two fp16 values is exact in float32, so only the query's rounding and the order and rounding of the
// matrix core's accumulation differ from the exact kernel.  The caller rescores the survivors exactly, so no bit of A is ever returned.
//
// bank_scores_f16_kernel<NT, TP>.  A workgroup (4 waves) owns a chunk of F16_CHUNK consecutive passages and a BLOCK OF QUERIES: NT column
// tiles of 16 query tokens, tp tiles per query (tp a power of two, the query's ceil(Lq / 16) tiles rounded up; the tiles behind Lq are
// padding) and NT / tp queries; blockIdx = chunk * query blocks + query block, so that the query blocks of one chunk run side by side
// and a row comes from HBM once.  NT is as wide as 64 KB of LDS and nq allow (8 tiles at D 128: 36 KB; the accumulators of two
// row tiles are 8 NT registers, 156 registers in all at NT 8, TP 2: three workgroups per CU).  A query of more than NT tiles is walked in passes of NT tiles with the running
// sum of a passage waiting in LDS (psum) between passes, as the exact kernel does.
//   The block's fp16 query rows are staged in LDS once per workgroup and pass: [16 NT][D + 16] fp16.  The B operand of tile t and
// k-step s is one ds_read_b128 per lane: lane l holds B[k = 32 s + 8 (l >> 4) + j][column l & 15] = row (16 t + (l & 15)) of that image,
// elements 32 s + 8 (l >> 4) + j.  THE PAD: with D a multiple of 32 a row of D + 16 fp16 is 2 (mod 4) slots of 16 bytes, so inside each
// of ds_read_b128's four 16-lane groups ({0-3, 12-15, 20-27}, ...) the eight lanes of one k-octet fall on eight distinct even slots
// and the eight of the other on eight distinct odd ones: no bank conflict (a pad of 8 fp16, one access width, leaves one slot 2-way).
//   A wave takes whole passages (passage wave, wave + 4, ... of the chunk), two 16-row tiles at a time.  Each lane loads its A
// fragment straight from global memory, 16 bytes per k-step: lane l holds row l & 15, k = 8 (l >> 4) + j of the step.  No LDS for
// rows.  A fragment is used against every column tile of the block, and a B fragment read from LDS against both row tiles: at one
// ds_read_b128 per matrix instruction four SIMDs would ask the LDS for 16 of every 16 cycles, at one per two for 8.  Rows behind the
// passage's length are not loaded; their lanes feed zeros and their results are dropped.
//   The epilogue is the exact kernel's: nan_max column maxima with LI_MASKED for masked rows, the four lane groups met by two
// shuffles, columns >= Lq never counted, and the columns of one query summed 0, 1, ... Lq - 1 in sequence from 0.0f by every lane
// alike.  No atomics: the same bytes from run to run.  A fully masked passage scores Lq * -9999.
// rr_launch_bank_scores_f16: fp16 rows only (plain or coded fp16 banks: li_src_f16's rows), D a multiple of 32, rows 16-byte aligned.
// f16_certify_kernel: the certificate of rr_bank_search_f16 (one thread per query).
#include <atomic>

#include "li_sources.h"
#include "rank_order.h"
#include "rr_common.h"

namespace {

constexpr int F16_NT_MAX = 8;            // column tiles (16 query tokens) of a query block
constexpr int F16_CHUNK = 32;            // passages of a workgroup's chunk (psum)
constexpr int F16_PAD = 16;              // fp16 values behind a query row in LDS (see THE PAD)

__device__ __forceinline__ f16x8 load_f16x8(const uint16_t* p) { return __builtin_bit_cast(f16x8, *(const uint4*)p); }

// R row tiles (1 or 2) of one passage from row c0 on against the NT column tiles in LDS; cmax: the running column maxima
template <int NT, int TP, int R>
__device__ __forceinline__ void f16_tiles(const uint16_t* __restrict__ prow, const uint8_t* __restrict__ pmask, int len, int c0, int D, int ldq,
                                          const uint16_t* bq, int li, int g, int col_lim, float (&cmax)[NT]) {
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const f16x8 zero8 = __builtin_bit_cast(f16x8, make_uint4(0u, 0u, 0u, 0u));
  f32x4 acc[R][NT];
  const uint16_t* ap[R];
  bool ok[R];
  f16x8 a[R];
#pragma unroll
  for (int u = 0; u < R; ++u) {
    const int c = c0 + 16 * u + li;                            // the context row this lane feeds to the matrix core
    ok[u] = c < len;
    ap[u] = prow + (size_t)(ok[u] ? c : 0) * D + 8 * g;
    a[u] = ok[u] ? load_f16x8(ap[u]) : zero8;
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[u][t] = zero4;
  }
  for (int d = 0; d < D; d += 32) {
    f16x8 a_n[R];
#pragma unroll
    for (int u = 0; u < R; ++u) a_n[u] = (ok[u] && d + 32 < D) ? load_f16x8(ap[u] + d + 32) : zero8;      // requested a step ahead
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

template <int NT, int TP>
__global__ __launch_bounds__(256) void bank_scores_f16_kernel(const float* __restrict__ query_li, const uint16_t* __restrict__ rows,
                                                              const uint8_t* __restrict__ mask_bytes, const rr_bank_slot* __restrict__ table, int n,
                                                              int nq, int nqb, int Lq, int D, float* __restrict__ out) {
  constexpr int tp = TP;                 // tiles of one query in a pass (a power of two, <= NT)
  extern __shared__ __attribute__((aligned(16))) uint16_t qh[];      // [16 NT][D + F16_PAD]: the block's query rows, fp16
  __shared__ float psum[F16_CHUNK];      // the running sum of the workgroup's passages between passes (one query per block then)
  const int ldq = D + F16_PAD, d8n = D / 8;
  const int qb = blockIdx.x % nqb, p0 = (blockIdx.x / nqb) * F16_CHUNK, pn = min(F16_CHUNK, n - p0);
  const int q0 = qb * (NT / tp);         // the block's first query
  const int passes = ((Lq + 15) / 16 + tp - 1) / tp;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, g = lane >> 4;
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
      const uint16_t* prow = rows + (size_t)first_row * D;
      const uint8_t* pmask = mask_bytes + first_row;
      float cmax[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) cmax[t] = -INFINITY;
      int ct = 0;
      for (; ct + 2 <= c_tiles; ct += 2) f16_tiles<NT, TP, 2>(prow, pmask, len, ct * 16, D, ldq, bq, li, g, col_lim, cmax);
      if (ct < c_tiles) f16_tiles<NT, TP, 1>(prow, pmask, len, ct * 16, D, ldq, bq, li, g, col_lim, cmax);
      float sum = 0.0f;                                         // every lane of the wave carries the same sum
      int cl = col_lim;
      asm volatile("" : "+s"(cl));                              // (else the 16 NT column tests below are hoisted out of the passage loop
                                                                // and held in scalar registers, which spill)
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
        __builtin_amdgcn_sched_barrier(0);                      // a tile's sixteen lane reads at a time: all NT at once spill scalar registers

      }
    }
  }
}

// certified[q] of rr_bank_search_f16: the call returned k real passages (cnt[q] == k: no exact score was -inf) and either every
// passage of the range was rescored (m == n), or the k-th exact score lies above a* + slack, a* = A of the last survivor (float32 sum)
__global__ void f16_certify_kernel(const float* __restrict__ A, long long n, const int32_t* __restrict__ surv, int m, const float* __restrict__ scores,
                                   const int32_t* __restrict__ cnt, int k, float slack, int nq, int32_t* __restrict__ certified) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  int ok = cnt[q] == k;
  if (ok && (long long)m < n) {
    const float sk = scores[(size_t)q * k + k - 1], a = A[(size_t)q * n + surv[(size_t)q * m + m - 1]];
    ok = sk == sk && a == a && sk > a + slack;
  }
  certified[q] = ok;
}

template <int NT, int TP>
hipError_t f16_launch_nt(const float* query_li, const rr_bank_view& bank, const rr_bank_slot* table, int n, int nq, int nqb, int Lq, int D, size_t lds,
                         float* out, hipStream_t st) {
  static std::atomic<unsigned long long> attr_set{0};
  const hipError_t e = li_lds_attr((const void*)bank_scores_f16_kernel<NT, TP>, attr_set);
  if (e != hipSuccess) return e;
  const long long blocks = (((long long)n + F16_CHUNK - 1) / F16_CHUNK) * nqb;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((bank_scores_f16_kernel<NT, TP>), dim3((unsigned)blocks), dim3(256), lds, st, query_li, bank.rows, bank.mask, table, n, nq,
                     nqb, Lq, D, out);
  return hipGetLastError();
}

int pow2_ceil(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

size_t f16_lds_bytes(int nt, int D) { return (size_t)16 * nt * (D + F16_PAD) * sizeof(uint16_t); }

}  // namespace

// The form of a launch of bank_scores_f16_kernel for nq queries of Lq tokens at D: the block's column tiles *nt, the tiles of one
// query in a pass *tp, the passes over a query.  Host arithmetic alone; hipErrorInvalidValue for a shape the launch refuses.
hipError_t rr_bank_scores_f16_form(int nq, int Lq, int D, int* nt_out, int* tp_out, int* passes_out) {
  if (nq <= 0 || Lq <= 0 || D <= 0 || D % 32) return hipErrorInvalidValue;
  int nt = F16_NT_MAX;
  while (nt > 1 && f16_lds_bytes(nt, D) > (size_t)64 * 1024) nt /= 2;
  if (f16_lds_bytes(nt, D) > (size_t)150 * 1024) return hipErrorInvalidValue;
  const int tiles = (Lq + 15) / 16;
  const int tp = std::min(pow2_ceil(tiles), nt);               // tiles of one query in a pass
  nt = (int)std::min<long long>(nt, (long long)tp * pow2_ceil(nq));      // no wider than the call's queries
  *nt_out = nt;
  *tp_out = tp;
  *passes_out = (tiles + tp - 1) / tp;                         // as the kernel counts them
  return hipSuccess;
}

// out [nq][n]: the approximate MaxSim (fp16 matrix core) of every query against the passages table[0 .. n) of an fp16 bank
hipError_t rr_launch_bank_scores_f16(const rr_bank_slot* table, int n, int nq, int Lq, int D, const float* query_li, const rr_bank_view& bank,
                                     float* out, hipStream_t st) {
  if (n <= 0 || nq <= 0 || Lq <= 0 || D <= 0 || D % 32 || !table || !query_li || !out || bank.nbits || !bank.rows || !bank.mask) return hipErrorInvalidValue;
  if ((((uintptr_t)query_li) | ((uintptr_t)table) | ((uintptr_t)bank.rows)) & 15) return hipErrorInvalidValue;
  int nt = 0, tp = 0, passes = 0;
  const hipError_t fe = rr_bank_scores_f16_form(nq, Lq, D, &nt, &tp, &passes);
  if (fe != hipSuccess) return fe;
  const int qpb = nt / tp, nqb = (nq + qpb - 1) / qpb;
  const size_t lds = f16_lds_bytes(nt, D);
#define F16_CASE(NT_, TP_) \
  if (nt == NT_ && tp == TP_) return f16_launch_nt<NT_, TP_>(query_li, bank, table, n, nq, nqb, Lq, D, lds, out, st)
  F16_CASE(1, 1); F16_CASE(2, 1); F16_CASE(2, 2); F16_CASE(4, 1); F16_CASE(4, 2); F16_CASE(4, 4);
  F16_CASE(8, 1); F16_CASE(8, 2); F16_CASE(8, 4); F16_CASE(8, 8);
#undef F16_CASE
  return hipErrorInvalidValue;
}

hipError_t rr_launch_f16_certify(const float* A, long long n, const int32_t* surv, int m, const float* scores, const int32_t* cnt, int k, float slack,
                                 int nq, int32_t* certified, hipStream_t st) {
  if (!A || !surv || !scores || !cnt || !certified || nq < 1 || m < 1 || k < 1 || k > m || (long long)m > n) return hipErrorInvalidValue;
  hipLaunchKernelGGL(f16_certify_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, A, n, surv, m, scores, cnt, k, slack, nq, certified);
  return hipGetLastError();
}
