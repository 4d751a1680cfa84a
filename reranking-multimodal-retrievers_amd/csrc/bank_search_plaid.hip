// PLAID-pruned top-k search over a range of a COMPRESSED passage bank (rr_bank_search_plaid, include/rerank_mi355.h): the staged
// search of the reference (third_party/ColBERT/colbert/search/index_storage.py:86-184, candidate_generation.py) with every tie made
// definite, from what a compressed bank already holds: one int32 centroid code per row, the fp16 centroid table, the passage table.
// An fp16 bank that holds these too (rr_bank_set_centroids; the view's nbits == 0 with codes and centroids) runs the same stages; only
// the exact stage reads rows, and it reads the bank's fp16 rows (rr_launch_bank_search_scores_listed decides by the view).
// Two forms, one plan (rr_plaid_search_plan) and one stage driver (rr_launch_plaid_search_stage): rr_bank_search_plaid takes the
// candidate set from one scan over the codes of the range, rr_bank_search_plaid_ivf from the bank's inverted file.  A call is a
// HEAD of three stages, a CANDIDATE STEP of one stage (scan) or two (inverted file) that leaves A1 and A2 in two rows of `pitch`
// entries a query, and a TAIL of four stages over those rows; a caller sees the stages numbered in sequence, 0 - 7 or 0 - 8.  One
// launch each unless noted.
// HEAD
//   0  S [nq][Cp][Lq] float32, S[q][c][j] = <float32(centroid c), query q column j>: li_scores_kernel (li_scores.hip) over the
//      centroid table taken as an fp16 bank of pseudo-passages of 64 centroids (Cp = C rounded up to 64; a prep launch writes the
//      pair list and the all-ones mask), so an entry has the bits rr_li_scores gives.  All Lq columns are computed (the kernel
//      finds query q at q * Lq * D); the stages below read the first Lq_coarse of a row.
//   1  plaid_cells_kernel: a workgroup per (query, column) takes the first ncells centroids of the column in rank order (NaN first,
//      higher score, lower index), one block-wide maximum per cell over the 64-bit keys of rank_order.h: keys are distinct, so
//      the result does not depend on scheduling.
//   2  plaid_bitmaps_kernel: per query the cell set and keep[c] = (max_j S[c][j] >= threshold; a NaN in the row: false) as bitmaps
//      of C bits.  A workgroup owns 256 centroids: the cell bits meet in LDS (ds_or), keep bits by ballot; no global atomics.
// CANDIDATE STEP, scan form (stage 3; pitch = n, an entry of a row is a passage of the range)
//   plaid_scan_kernel, the hot path: a workgroup belongs to one query and 64 consecutive passages, holds the query's two
//      bitmaps in LDS (C / 4 bytes) and a WAVE takes whole passages.  Lanes load 64 codes and mask bytes per step and test them
//      against the cell bitmap; a ballot decides candidacy.  A non-candidate costs its codes and mask bytes and writes -inf.  A
//      Under a caller's filter (FILTERED, rr_bank_search_plaid_filtered) a passage whose bit is clear is no candidate, decided
//      before its table entry, codes or mask bytes are read: it costs one bit (a scalar load of the word) and its two -inf.  A
//      candidate walks its unmasked rows: lane j owns column j, one row of S per code is one coalesced read (Lq_coarse * 4 bytes),
//      the column maxima with (A1) and without (A2) the keep test are kept side by side, and the columns are summed 0, 1, ...
//      Lq_coarse - 1 in sequence from 0.0f by constant-lane shuffles, a chain every lane carries.  Above 64 columns the passage
//      is walked once per block of 64 and the chain goes on (plaid_a1_a2).  A1 and A2 go to two dense rows [nq][n].
// CANDIDATE STEP, inverted-file form (stages 3 and 4; pitch = cap, an entry of a row is a PLACE in the query's candidate list)
//   rr_launch_ivf_candidates (bank_ivf.hip): a bitmap per query set from the lists of its cells and compacted in ascending order
//      into cand [nq][cap] with its count; places follow bank-index order, so the tie rule holds.
//   plaid_score_listed_kernel: A1 / A2 of the listed candidates into compact rows [nq][cap] by plaid_a1_a2, the device function the
//      scan computes them with.
// TAIL (stages 4 - 7, or 5 - 8), over the rows [nq][pitch] and via = the candidate lists (inverted file) or null (scan)
//   rr_launch_topk_select (bank_search.hip) over the A1 row: the first min(ndocs, pitch) per query; ties by index.
//   plaid_list_select_kernel: stage-1 survivors (A1 != -inf) ordered by A2, the first ndocs / 4 kept, with their count.
//   rr_launch_bank_search_scores_listed (bank_search.hip): bank_search_scores_kernel itself, the kernel of rr_bank_search, with
//      a workgroup's passages picked from the stage-2 list of its query, one per wave: the entry itself (pick_list), or the
//      passage at that place of via (pick_via); the exact score overwrites the entry's place of the A2 row.
//   plaid_list_select_kernel again: by exact score, the first k, mapped through via back to passages; -1 / -inf behind the count,
//      and the count.
// -inf is the "absent" mark of every row and list: an entry that holds it at some stage is not a survivor of that stage.
// The rank order of every list (NaN first, higher score, lower index) and its 64-bit key are those of rr_bank_search: rank_order.h
// (the bitonic network over keys is written out in plaid_list_select_kernel as in topk_select_kernel; rank_order.h says why).
// rr_plaid_prune_host restates cells, candidates, stage 1 and stage 2 in host code over the same key: the written-down definition.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "li_sources.h"
#include "rank_order.h"
#include "rr_common.h"

namespace {

constexpr int PS_CHUNK = 64;             // passages per workgroup of the scan (16 per wave)
constexpr int LIST_MAX = 1024;           // entries plaid_list_select_kernel sorts (ndocs)
constexpr int PSEUDO = 64;               // centroids per pseudo-passage of stage 0

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
  return ((unsigned long long)hi << 32) | lo;
}

// stage 0 prep: the pair list of the pseudo-passages ((query, block of 64 centroids), query-major) and the all-ones mask bytes
__global__ __launch_bounds__(256) void plaid_prep_kernel(rr_bank_pair* pairs, int blocks, int nq, int C, uint8_t* ones, int Cp) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < blocks * nq) {
    const int q = i / blocks, b = i - q * blocks;
    pairs[i] = rr_bank_pair{(int64_t)b * PSEUDO, min(PSEUDO, C - b * PSEUDO), q};
  }
  if (i < Cp) ones[i] = 1;
}

__global__ __launch_bounds__(256) void plaid_cells_kernel(const float* __restrict__ S, long long s_q, int s_ld, int C, int Lqc, int ncells,
                                                          int32_t* __restrict__ cells) {
  __shared__ unsigned long long wbest[2][4];
  const int q = blockIdx.x / Lqc, j = blockIdx.x - q * Lqc, tid = threadIdx.x;
  const float* col = S + (size_t)q * s_q + j;
  unsigned long long prev = 0ull;
  for (int r = 0; r < ncells; ++r) {
    unsigned long long best = 0ull;                           // below every key
    for (int c = tid; c < C; c += 256) {
      const unsigned long long key = rank_key(col[(size_t)c * s_ld], (uint32_t)c);
      if ((r == 0 || key < prev) && key > best) best = key;
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
      const unsigned long long o = shfl_xor_u64(best, m);
      if (o > best) best = o;
    }
    if ((tid & 63) == 0) wbest[r & 1][tid >> 6] = best;
    __syncthreads();                                          // (the buffers alternate: one barrier per cell)
    prev = max(max(wbest[r & 1][0], wbest[r & 1][1]), max(wbest[r & 1][2], wbest[r & 1][3]));
    if (tid == 0) cells[((size_t)q * Lqc + j) * ncells + r] = (int32_t)rank_key_index(prev);
  }
}

__global__ __launch_bounds__(256) void plaid_bitmaps_kernel(const float* __restrict__ S, long long s_q, int s_ld, int C, int Lqc, int ncells,
                                                            float thr, const int32_t* __restrict__ cells, int W,
                                                            uint32_t* __restrict__ cellbits, uint32_t* __restrict__ keepbits) {
  __shared__ uint32_t cb[8], kb[8];
  const int q = blockIdx.y, tid = threadIdx.x, c = blockIdx.x * 256 + tid;
  if (tid < 8) cb[tid] = 0u;
  __syncthreads();
  const int32_t* cl = cells + (size_t)q * Lqc * ncells;
  for (int i = tid; i < Lqc * ncells; i += 256) {
    const int cc = cl[i];
    if ((cc >> 8) == (int)blockIdx.x) atomicOr(&cb[(cc & 255) >> 5], 1u << (cc & 31));      // LDS; an OR has one result
  }
  bool keep = false;
  if (c < C) {
    const float* row = S + (size_t)q * s_q + (size_t)c * s_ld;
    float m = -INFINITY;
    for (int j = 0; j < Lqc; ++j) m = nan_max(m, row[j]);
    keep = m >= thr;
  }
  const unsigned long long b = __ballot(keep);
  if ((tid & 63) == 0) {
    kb[(tid >> 6) * 2] = (uint32_t)b;
    kb[(tid >> 6) * 2 + 1] = (uint32_t)(b >> 32);
  }
  __syncthreads();
  if (tid < 8 && blockIdx.x * 8 + tid < W) {
    cellbits[(size_t)q * W + blockIdx.x * 8 + tid] = cb[tid];
    keepbits[(size_t)q * W + blockIdx.x * 8 + tid] = kb[tid];
  }
}

// A1 (s1) and A2 (s2) of ONE candidate passage, by the whole wave (every lane ends with both): lane j owns column j, one row of S per
// unmasked row of the passage, the column maxima with and without the keep test (keep: the query's keep bitmap in LDS) side by
// side, the columns summed 0, 1, ... Lq_coarse - 1 in sequence from 0.0f.  The one body under plaid_scan_kernel and
// plaid_score_listed_kernel, so that both give the same bits.
__device__ __forceinline__ void plaid_a1_a2(const float* __restrict__ Sq, int s_ld, int C, int Lqc, const uint32_t* keep,
                                            const int32_t* __restrict__ codes, const uint8_t* __restrict__ mask, long long first_row, int len,
                                            int lane, float& s1, float& s2) {
  s1 = 0.0f;
  s2 = 0.0f;
  for (int j0 = 0; j0 < Lqc; j0 += 64) {
    const int j = j0 + lane;
    const bool j_ok = j < Lqc;
    float m1 = LI_MASKED, m2 = LI_MASKED;
    for (int base = 0; base < len; base += 64) {
      const int r = base + lane;
      int code = 0, mk = 0;
      if (r < len) {
        code = min(max(codes[first_row + r], 0), C - 1);
        mk = mask[first_row + r];
      }
      const int cnt = min(64, len - base);
      for (int t = 0; t < cnt; ++t) {
        if (!__builtin_amdgcn_readlane(mk, t)) continue;      // a masked row contributes nothing
        const int c = __builtin_amdgcn_readlane(code, t);
        const bool kept = (keep[c >> 5] >> (c & 31)) & 1u;
        const float v = j_ok ? Sq[(size_t)c * s_ld + j] : LI_MASKED;
        m2 = nan_max(m2, v);
        if (kept) m1 = nan_max(m1, v);
      }
    }
    const int cols = min(64, Lqc - j0);
    for (int l = 0; l < cols; ++l) {                          // columns 0, 1, ... Lq_coarse - 1, one after the other
      s1 += __shfl(m1, l, 64);
      s2 += __shfl(m2, l, 64);
    }
  }
}

template <bool FILTERED>
__global__ __launch_bounds__(256) void plaid_scan_kernel(const float* __restrict__ S, long long s_q, int s_ld, int C, int Lqc,
                                                         const uint32_t* __restrict__ cellbits, const uint32_t* __restrict__ keepbits, int W,
                                                         const int32_t* __restrict__ codes, const uint8_t* __restrict__ mask,
                                                         const rr_bank_slot* __restrict__ table, int n, int nq, float* __restrict__ a1,
                                                         float* __restrict__ a2, const rr_passage_filter filter) {
  extern __shared__ uint32_t bits[];     // [W] cell set, [W] keep
  const int q = blockIdx.x % nq, p0 = (blockIdx.x / nq) * PS_CHUNK, pn = min(PS_CHUNK, n - p0);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = threadIdx.x; i < W; i += 256) {
    bits[i] = cellbits[(size_t)q * W + i];
    bits[W + i] = keepbits[(size_t)q * W + i];
  }
  __syncthreads();
  const float* Sq = S + (size_t)q * s_q;
  for (int i = wave; i < pn; i += 4) {                        // a passage belongs to one wave
    if constexpr (FILTERED)
      if (!filter.allowed(q, p0 + i)) {                       // wave-uniform: no candidate, and nothing of the passage is read
        if (lane == 0) {
          a1[(size_t)q * n + p0 + i] = -INFINITY;
          a2[(size_t)q * n + p0 + i] = -INFINITY;
        }
        continue;
      }
    const rr_bank_slot sl = table[p0 + i];
    const long long first_row = uniform_i64(sl.first_row);
    const int len = __builtin_amdgcn_readfirstlane(sl.len);
    bool cand = false;
    for (int base = 0; base < len && !cand; base += 64) {
      const int r = base + lane;
      bool hit = false;
      if (r < len && mask[first_row + r]) {
        const int c = min(max(codes[first_row + r], 0), C - 1);
        hit = (bits[c >> 5] >> (c & 31)) & 1u;
      }
      cand = __ballot(hit) != 0ull;
    }
    float s1 = -INFINITY, s2 = -INFINITY;
    if (cand) plaid_a1_a2(Sq, s_ld, C, Lqc, bits + W, codes, mask, first_row, len, lane, s1, s2);      // wave-uniform
    if (lane == 0) {
      a1[(size_t)q * n + p0 + i] = s1;
      a2[(size_t)q * n + p0 + i] = s2;
    }
  }
}

// Stage 4 of rr_bank_search_plaid_ivf: A1 and A2 (plaid_a1_a2, the arithmetic of the scan) of the LISTED candidates of a query:
// entry i < min(cnt[q], cap) of cand[q][0 .. cap) (range-relative, clamped into [0, n)) goes to a1 / a2 [q][i] of the compact rows
// [nq][cap]; the entries behind the count are written by the candidate step.  A workgroup belongs to one query (blockIdx % nq), holds
// its keep bitmap in LDS and takes four entries a round, one per wave, `groups` workgroups of a query striding over its list; a
// workgroup whose first round lies behind the count ends before it loads anything.
__global__ __launch_bounds__(256) void plaid_score_listed_kernel(const float* __restrict__ S, long long s_q, int s_ld, int C, int Lqc,
                                                                 const uint32_t* __restrict__ keepbits, int W, const int32_t* __restrict__ codes,
                                                                 const uint8_t* __restrict__ mask, const rr_bank_slot* __restrict__ table, int n,
                                                                 int nq, int groups, const int32_t* __restrict__ cand, int cap,
                                                                 const int32_t* __restrict__ cnt, float* __restrict__ a1, float* __restrict__ a2) {
  extern __shared__ uint32_t bits[];     // [W] keep
  const int q = blockIdx.x % nq, g = blockIdx.x / nq, have = min(cnt[q], cap);
  if (g * 4 >= have) return;             // the whole workgroup
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = threadIdx.x; i < W; i += 256) bits[i] = keepbits[(size_t)q * W + i];
  __syncthreads();
  const float* Sq = S + (size_t)q * s_q;
  for (int i = g * 4 + wave; i < have; i += groups * 4) {     // a candidate belongs to one wave
    const int p = min(max(__builtin_amdgcn_readfirstlane(cand[(size_t)q * cap + i]), 0), n - 1);
    const rr_bank_slot sl = table[p];
    float s1, s2;
    plaid_a1_a2(Sq, s_ld, C, Lqc, bits, codes, mask, uniform_i64(sl.first_row), __builtin_amdgcn_readfirstlane(sl.len), lane, s1, s2);
    if (lane == 0) {
      a1[(size_t)q * cap + i] = s1;
      a2[(size_t)q * cap + i] = s2;
    }
  }
}

// One workgroup per query: the entries list_in[q][0 .. cnt) (cnt = cnt_in[q], or n_in) whose score (and whose entry of valid_row, if
// given) is not -inf, in rank order by scores[q][entry]; the first `keep` go to list_out[q] (+ add) and scores_out[q], -1 / -inf
// behind them up to `keep`, their number to cnt_out[q].  cnt <= 1024.  map (or null) [.][n]: list_out gets map[q][entry] in place of
// the entry (rr_bank_search_plaid_ivf: an entry is a place in the query's candidate list, the output its passage).
__global__ __launch_bounds__(256) void plaid_list_select_kernel(const float* __restrict__ scores, const float* __restrict__ valid_row, long long n,
                                                                const int32_t* __restrict__ list_in, int in_ld, const int32_t* __restrict__ cnt_in,
                                                                int n_in, int keep, int32_t* __restrict__ list_out, int out_ld,
                                                                int32_t* __restrict__ cnt_out, int add, float* __restrict__ scores_out,
                                                                const int32_t* __restrict__ map) {
  __shared__ unsigned long long key[LIST_MAX];
  __shared__ int valid;
  const int q = blockIdx.x, tid = threadIdx.x;
  const int cnt = min(cnt_in ? cnt_in[q] : n_in, LIST_MAX);
  const float* row = scores + (size_t)q * n;
  int n2 = 2;
  while (n2 < cnt) n2 <<= 1;
  if (tid == 0) valid = 0;
  for (int i = tid; i < n2; i += 256) {
    unsigned long long kv = 0ull;                             // absent: behind every entry
    if (i < cnt) {
      const int idx = list_in[(size_t)q * in_ld + i];
      const float s = row[idx];
      if (s != -INFINITY && (!valid_row || valid_row[(size_t)q * n + idx] != -INFINITY)) kv = rank_key(s, (uint32_t)idx);
    }
    key[i] = kv;
  }
  __syncthreads();
  for (int kk = 2; kk <= n2; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n2; i += 256) {
        const int l = i ^ j;
        if (l > i) {
          const bool up = (i & kk) == 0;                      // a run in rank order (larger key first)
          const unsigned long long a = key[i], b = key[l];
          if (up ? a < b : a > b) { key[i] = b; key[l] = a; }
        }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < n2; i += 256)
    if (key[i] != 0ull && (i == n2 - 1 || key[i + 1] == 0ull)) valid = i + 1;      // one thread at most
  __syncthreads();
  const int kept = min(keep, valid);
  for (int i = tid; i < keep; i += 256) {
    int32_t o = -1;
    float s = -INFINITY;
    if (i < kept) {
      const int idx = (int)rank_key_index(key[i]);
      o = (map ? map[(size_t)q * n + idx] : idx) + add;
      s = row[idx];
    }
    list_out[(size_t)q * out_ld + i] = o;
    if (scores_out) scores_out[(size_t)q * out_ld + i] = s;
  }
  if (tid == 0) cnt_out[q] = kept;
}

size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

// the order of the lists on the host: NaN first, higher score, lower index
bool ranks_before(float sa, int ia, float sb, int ib) { return rank_key(sa, (uint32_t)ia) > rank_key(sb, (uint32_t)ib); }
float host_nan_max(float m, float v) { return (v > m || v != v) ? v : m; }

}  // namespace

hipError_t rr_launch_list_select(const float* scores, long long n, int nq, const int32_t* list_in, int n_in, int keep, int32_t* list_out,
                                 int32_t* cnt_out, int add, float* scores_out, hipStream_t st) {
  if (!scores || !list_in || !list_out || !cnt_out || nq < 1 || n_in < 1 || n_in > LIST_MAX || keep < 1 || keep > n_in) return hipErrorInvalidValue;
  hipLaunchKernelGGL(plaid_list_select_kernel, dim3((unsigned)nq), dim3(256), 0, st, scores, nullptr, n, list_in, n_in, nullptr, n_in, keep, list_out,
                     keep, cnt_out, add, scores_out, nullptr);
  return hipGetLastError();
}

// The block of a call.  longest == 0: the scan form, score rows of n entries.  longest > 0, the longest list of the bank's inverted
// file: the inverted-file form, with the bitmaps, the candidate lists and their counts, and score rows of cap entries: a query has
// Lq_coarse * ncells cell entries and a list holds at most `longest` passages, and never more than the range.
rr_plaid_search_layout rr_plaid_search_plan(int nq, int n, int C, int Lq, int Lqc, int ncells, int ndocs, int longest) {
  rr_plaid_search_layout l{};
  const bool ivf = longest > 0;
  l.stages = ivf ? RR_PLAID_IVF_SEARCH_STAGES : RR_PLAID_SEARCH_STAGES;
  l.Cp = (C + PSEUDO - 1) / PSEUDO * PSEUDO;
  l.W = (C + 31) / 32;
  if (ivf) {
    l.cap = (int)std::max<long long>(1, std::min<long long>(n, (long long)Lqc * ncells * longest));
    l.Wn = (n + 31) / 32;
  }
  l.pitch = ivf ? l.cap : n;
  l.k1 = std::min(ndocs, l.pitch);
  l.k2 = std::min(ndocs / 4, n);
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += up16(bytes); return o; };
  l.S = take((size_t)nq * l.Cp * Lq * sizeof(float));
  l.pairs = take((size_t)nq * (l.Cp / PSEUDO) * sizeof(rr_bank_pair));
  l.ones = take((size_t)l.Cp);
  l.cells = take((size_t)nq * Lqc * ncells * sizeof(int32_t));
  l.cellbits = take((size_t)nq * l.W * sizeof(uint32_t));
  l.keepbits = take((size_t)nq * l.W * sizeof(uint32_t));
  if (ivf) {
    l.bm = take((size_t)nq * l.Wn * sizeof(uint32_t));
    l.cand = take((size_t)nq * l.cap * sizeof(int32_t));
    l.ccnt = take((size_t)nq * sizeof(int32_t));
  }
  l.a1 = take((size_t)nq * l.pitch * sizeof(float));
  l.a2 = take((size_t)nq * l.pitch * sizeof(float));
  l.list1 = take((size_t)nq * l.k1 * sizeof(int32_t));
  l.list2 = take((size_t)nq * l.k2 * sizeof(int32_t));
  l.cnt2 = take((size_t)nq * sizeof(int32_t));
  l.tmp_entries = rr_topk_select_scratch(nq, l.pitch, l.k1);
  l.tmp_a = take(l.tmp_entries * sizeof(int32_t));
  l.tmp_b = take(l.tmp_entries * sizeof(int32_t));
  l.total = off;
  return l;
}

// Stage `stage` of l.stages.  The candidate step takes one stage number in the scan form and two in the inverted-file form; the
// tail's four follow it.
hipError_t rr_launch_plaid_search_stage(int stage, const rr_plaid_search_args& a, const rr_plaid_search_layout& l, hipStream_t st) {
  const int C = a.bank.n_centroids;
  const bool ivf = l.stages == RR_PLAID_IVF_SEARCH_STAGES;
  // (a row source for the exact stage: residual codes, or the fp16 rows of a bank with a centroid table)
  if (!a.scratch || !a.query_li || !a.table || (!a.bank.nbits && !a.bank.rows) || !a.bank.codes || !a.bank.mask || !a.bank.centroids || C < 1 ||
      C > RR_PLAID_SEARCH_MAX_CENTROIDS || a.nq < 1 || a.n < 1 || a.Lqc < 1 || a.Lqc > a.Lq || a.ncells < 1 || a.ncells > std::min(C, 16) ||
      a.ndocs < 4 || a.ndocs > LIST_MAX || a.k < 1 || a.k > l.k2 || !a.indices_out || !a.counts_out ||
      (l.stages != RR_PLAID_SEARCH_STAGES && !ivf) || l.pitch != (ivf ? l.cap : a.n) || l.k1 < 1 || l.k1 > l.pitch ||
      (ivf && (l.cap < 1 || l.cap > a.n || !a.ivf.offsets || !a.ivf.pids || (long long)a.first + a.n > a.ivf.passages)) ||
      (a.filter.bits && ((a.filter.rows != 1 && a.filter.rows != a.nq) || a.filter.first != a.first ||
                         a.filter.ld < ((long long)a.first + a.n + 31) / 32)))
    return hipErrorInvalidValue;
  // the steps of both forms in one sequence; a stage number skips the candidate steps of the other form
  enum { SCORES, CELLS, BITMAPS, SCAN, IVF_LISTS, IVF_SCORES, SELECT_NDOCS, SELECT_QUARTER, EXACT, SELECT_K };
  const int step = stage < 0 || stage >= l.stages ? -1 : stage < SCAN ? stage : ivf ? stage + 1 : stage == SCAN ? SCAN : stage + 2;
  float* S = (float*)(a.scratch + l.S);
  const long long s_q = (long long)l.Cp * a.Lq;
  rr_bank_pair* pairs = (rr_bank_pair*)(a.scratch + l.pairs);
  uint8_t* ones = (uint8_t*)(a.scratch + l.ones);
  int32_t* cells = (int32_t*)(a.scratch + l.cells);
  uint32_t* cellbits = (uint32_t*)(a.scratch + l.cellbits);
  uint32_t* keepbits = (uint32_t*)(a.scratch + l.keepbits);
  float* a1 = (float*)(a.scratch + l.a1);
  float* a2 = (float*)(a.scratch + l.a2);
  int32_t* list1 = (int32_t*)(a.scratch + l.list1);
  int32_t* list2 = (int32_t*)(a.scratch + l.list2);
  int32_t* cnt2 = (int32_t*)(a.scratch + l.cnt2);
  int32_t* cand = ivf ? (int32_t*)(a.scratch + l.cand) : nullptr;      // the tail's via: a place in a row -> its passage
  int32_t* ccnt = ivf ? (int32_t*)(a.scratch + l.ccnt) : nullptr;
  switch (step) {
    case SCORES: {
      const int blocks = l.Cp / PSEUDO, items = std::max(blocks * a.nq, l.Cp);
      hipLaunchKernelGGL(plaid_prep_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, pairs, blocks, a.nq, C, ones, l.Cp);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
      const rr_bank_view cent{0, 0, a.bank.centroids, nullptr, nullptr, nullptr, nullptr, ones};
      return rr_launch_bank_li_scores(pairs, nullptr, blocks * a.nq, a.Lq, PSEUDO, a.D, a.query_li, cent, S, nullptr, st);
    }
    case CELLS:
      hipLaunchKernelGGL(plaid_cells_kernel, dim3((unsigned)(a.nq * a.Lqc)), dim3(256), 0, st, S, s_q, a.Lq, C, a.Lqc, a.ncells, cells);
      return hipGetLastError();
    case BITMAPS:
      hipLaunchKernelGGL(plaid_bitmaps_kernel, dim3((unsigned)((C + 255) / 256), (unsigned)a.nq), dim3(256), 0, st, S, s_q, a.Lq, C, a.Lqc,
                         a.ncells, a.thr, cells, l.W, cellbits, keepbits);
      return hipGetLastError();
    case SCAN: {
      const long long blocks = ((long long)a.n + PS_CHUNK - 1) / PS_CHUNK * a.nq;
      if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
      if (a.filter.bits)
        hipLaunchKernelGGL(plaid_scan_kernel<true>, dim3((unsigned)blocks), dim3(256), (size_t)2 * l.W * sizeof(uint32_t), st, S, s_q, a.Lq, C,
                           a.Lqc, cellbits, keepbits, l.W, a.bank.codes, a.bank.mask, a.table, a.n, a.nq, a1, a2, a.filter);
      else
        hipLaunchKernelGGL(plaid_scan_kernel<false>, dim3((unsigned)blocks), dim3(256), (size_t)2 * l.W * sizeof(uint32_t), st, S, s_q, a.Lq, C,
                           a.Lqc, cellbits, keepbits, l.W, a.bank.codes, a.bank.mask, a.table, a.n, a.nq, a1, a2, rr_passage_filter{});
      return hipGetLastError();
    }
    case IVF_LISTS:
      return rr_launch_ivf_candidates(a.ivf, C, cells, a.Lqc * a.ncells, a.nq, a.first, a.n, (uint32_t*)(a.scratch + l.bm), l.Wn, cand, l.cap,
                                      ccnt, a1, a2, a.filter, st);
    case IVF_SCORES: {
      const int groups = std::min((l.cap + 3) / 4, 2048);     // workgroups of a query; they stride over its list
      hipLaunchKernelGGL(plaid_score_listed_kernel, dim3((unsigned)((long long)groups * a.nq)), dim3(256), (size_t)l.W * sizeof(uint32_t), st,
                         S, s_q, a.Lq, C, a.Lqc, keepbits, l.W, a.bank.codes, a.bank.mask, a.table, a.n, a.nq, groups, cand, l.cap, ccnt, a1, a2);
      return hipGetLastError();
    }
    case SELECT_NDOCS:
      return rr_launch_topk_select(a1, a.nq, l.pitch, l.k1, 0, l.tmp_entries ? (int32_t*)(a.scratch + l.tmp_a) : nullptr,
                                   l.tmp_entries ? (int32_t*)(a.scratch + l.tmp_b) : nullptr, list1, nullptr, st);
    case SELECT_QUARTER:
      hipLaunchKernelGGL(plaid_list_select_kernel, dim3((unsigned)a.nq), dim3(256), 0, st, a2, a1, (long long)l.pitch, list1, l.k1, nullptr, l.k1,
                         std::min(a.ndocs / 4, l.k2), list2, l.k2, cnt2, 0, nullptr, nullptr);
      return hipGetLastError();
    case EXACT:
      return rr_launch_bank_search_scores_listed(a.table, a.n, a.nq, a.Lq, a.D, a.query_li, a.bank, list2, l.k2, cnt2, cand, l.cap, a2, st);
    case SELECT_K:
      hipLaunchKernelGGL(plaid_list_select_kernel, dim3((unsigned)a.nq), dim3(256), 0, st, a2, nullptr, (long long)l.pitch, list2, l.k2, cnt2, 0,
                         a.k, a.indices_out, a.k, a.counts_out, a.first, a.scores_out, cand);
      return hipGetLastError();
  }
  return hipErrorInvalidValue;
}

// Cells, candidates, stage 1 and stage 2 of ONE query on the host, from a given S (rr_util_plaid_prune, rerank_mi355_diag.h).
// Passages lie back to back in codes / mask.  Returns false for a code outside [0, C).
bool rr_plaid_prune_host(const float* S, int C, int Lqc, int s_ld, const int32_t* codes, const uint8_t* mask, const int32_t* lengths,
                         int n, int ncells, float thr, int ndocs, uint8_t* cells_out, float* a1_out, float* a2_out, int32_t* list1_out,
                         int32_t* n1_out, int32_t* list2_out, int32_t* n2_out) {
  std::vector<uint8_t> cell((size_t)C, 0), keep((size_t)C, 0);
  std::vector<int> order((size_t)C);
  for (int j = 0; j < Lqc; ++j) {
    for (int c = 0; c < C; ++c) order[(size_t)c] = c;
    std::partial_sort(order.begin(), order.begin() + ncells, order.end(),
                      [&](int x, int y) { return ranks_before(S[(size_t)x * s_ld + j], x, S[(size_t)y * s_ld + j], y); });
    for (int r = 0; r < ncells; ++r) cell[(size_t)order[(size_t)r]] = 1;
  }
  for (int c = 0; c < C; ++c) {
    float m = -INFINITY;
    for (int j = 0; j < Lqc; ++j) m = host_nan_max(m, S[(size_t)c * s_ld + j]);
    keep[(size_t)c] = m >= thr;
  }
  if (cells_out) memcpy(cells_out, cell.data(), (size_t)C);
  std::vector<float> a1((size_t)n), a2((size_t)n);
  size_t row0 = 0;
  for (int p = 0; p < n; ++p) {
    const int len = lengths[p];
    bool cand = false;
    for (int r = 0; r < len; ++r) {
      const int c = codes[row0 + r];
      if (c < 0 || c >= C) return false;
      if ((!mask || mask[row0 + r]) && cell[(size_t)c]) cand = true;
    }
    float s1 = -INFINITY, s2 = -INFINITY;
    if (cand) {
      s1 = 0.0f;
      s2 = 0.0f;
      for (int j = 0; j < Lqc; ++j) {
        float m1 = -9999.0f, m2 = -9999.0f;
        for (int r = 0; r < len; ++r) {
          if (mask && !mask[row0 + r]) continue;
          const int c = codes[row0 + r];
          const float v = S[(size_t)c * s_ld + j];
          m2 = host_nan_max(m2, v);
          if (keep[(size_t)c]) m1 = host_nan_max(m1, v);
        }
        s1 += m1;
        s2 += m2;
      }
    }
    a1[(size_t)p] = s1;
    a2[(size_t)p] = s2;
    row0 += (size_t)len;
  }
  if (a1_out) memcpy(a1_out, a1.data(), (size_t)n * sizeof(float));
  if (a2_out) memcpy(a2_out, a2.data(), (size_t)n * sizeof(float));
  std::vector<int> l1;
  for (int p = 0; p < n; ++p)
    if (a1[(size_t)p] != -INFINITY) l1.push_back(p);
  std::sort(l1.begin(), l1.end(), [&](int x, int y) { return ranks_before(a1[(size_t)x], x, a1[(size_t)y], y); });
  if ((int)l1.size() > ndocs) l1.resize((size_t)ndocs);
  std::vector<int> l2;
  for (int p : l1)
    if (a2[(size_t)p] != -INFINITY) l2.push_back(p);
  std::sort(l2.begin(), l2.end(), [&](int x, int y) { return ranks_before(a2[(size_t)x], x, a2[(size_t)y], y); });
  if ((int)l2.size() > ndocs / 4) l2.resize((size_t)(ndocs / 4));
  if (n1_out) *n1_out = (int32_t)l1.size();
  if (n2_out) *n2_out = (int32_t)l2.size();
  if (list1_out) for (size_t i = 0; i < l1.size(); ++i) list1_out[i] = l1[i];
  if (list2_out) for (size_t i = 0; i < l2.size(); ++i) list2_out[i] = l2[i];
  return true;
}
