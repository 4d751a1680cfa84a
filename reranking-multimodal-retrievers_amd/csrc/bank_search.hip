// Exact top-k MaxSim search over a range of a passage bank (rr_bank_search, include/rerank_mi355.h): the score PLAID's last stage
// computes (colbert_score, flmr_utils.py:22-48) for EVERY passage of the range, then the k best per query.  Two kernels.
//
// (a) bank_search_scores_kernel: one float per (query, passage), out[q][p] = the maxsim of li_scores_kernel (li_scores.hip) for
//     that pair with padded_context_len = the passage's own length, bit for bit: the same operand sources (li_sources.h), the
//     same v_mfma_f32_16x16x4_f32 chain per entry (D in ascending steps of 16, e = 0..3 inside a step), nan_max column maxima,
//     and the columns summed 0, 1, ... Lq - 1 in sequence from 0.0f.  What differs is who does it.  A workgroup (4 waves) belongs
//     to one query and one contiguous chunk of passages: it stages the query's column block in LDS once per chunk ([16 JT][D + 4]
//     floats, 17 KB at Lq 32, D 128) where li_scores_kernel stages it once per pair, and a WAVE takes whole passages (passage
//     wave, wave + 4, ... of the chunk), tile after tile.  So a column maximum never leaves the wave: the four lane groups g meet
//     by two shuffles, the sixteen columns of a tile are read back lane by lane (constant-lane shuffles) into one sequential sum
//     that every lane of the wave carries, and there is no barrier inside the passage loop.  A maximum is the same whichever order
//     its rows arrive in (a NaN sticks; +0 / -0 cannot change a sum that starts at +0), so the wave-per-passage order of the rows
//     gives li_scores_kernel's bits.  For Lq above one column block the workgroup walks its chunk once per block and the running
//     sum of a passage waits in LDS (psum) between blocks: the sum stays ONE chain over all Lq columns.
//     Chunking: chunks are short (16 passages, 4 per wave; rr_set_tuning("search_chunk")) and consecutive workgroups are the
//     queries of one chunk (blockIdx = chunk * n_queries + query), so that a chunk's rows are read from HBM once and by the other
//     queries from L2 / MALL.  The grid is static, so what passages of unequal length cost is the last round of workgroups: 100 000
//     passages of 64 .. 180 rows are 6250 chunks per query on about 1536 resident workgroups (80 VGPRs at JT 2: 6 waves per SIMD),
//     four rounds, and a workgroup that drew long passages delays the end by its own chunk only.  Measured on that bank at Lq 32
//     (tools/bench_bank_search.py, profiles/bank_search_bench.json.log "search_ms" / "search_ms_at_chunk", ms per call): one
//     query, fp16: 8 / 16 / 32 / 64 / 128 passages per chunk took 1.72 / 1.90 / 1.84 / 2.15 / 2.51, compressed 3.02 / 3.14 / 3.17 /
//     3.42 / 3.81; 16 queries, fp16: 19.30 / 19.12 / 18.92 / 18.96 / 18.97, compressed 38.9 / 37.9 / 37.1 / 36.8 / 36.7.  Long
//     chunks lose up to a third at one query (few rounds, an uneven last one) and gain 3 % at sixteen; 8, 16 and 32 lie within
//     what two boxes differ by (a first run gave 1.76 / 1.74 / 2.05 at one query), and below 16 the 17 KB query block restaged
//     per chunk shows at sixteen queries.  16 it is.  On the device alone the scoring launch takes 1.17 x the time of
//     li_scores_kernel over the same pairs at one query on the fp16 bank (that launch gets its pairs longest first from the host
//     and fills every slot with one pair), and 0.95 / 0.88 / 0.82 x compressed, at 16 queries fp16, and both: the call wins by
//     what it no longer stages and sorts on the host.
//     WHICH passages a workgroup owns is a template parameter (PICK): pick_range, the chunk above, for rr_bank_search; pick_list,
//     four entries of a per-query list with a count, one per wave, for the exact scores of rr_bank_search_plaid's tail
//     (bank_search_plaid.hip), which are therefore these bits; pick_via, pick_list through the candidate list of
//     rr_bank_search_plaid_ivf (a list entry is a place in that list, and the score goes to that place of a compact row).  The
//     range form compiles to the instructions it had before the picker existed.  pick_range_bits is pick_range under a caller's
//     filter (rr_bank_search_filtered): a workgroup whose chunk has no set bit writes its -inf entries and ends before it stages
//     the query block, and a wave whose passage has a clear bit writes -inf, reads no row and issues no matrix instruction.  The
//     bit is read wave-uniformly (a scalar load of the word).  The selection (b) runs over the dense row as it is, then one
//     plaid_list_select_kernel pass over its k survivors drops the -inf and writes the tail and the count.  pick_places is the
//     list-driven form of that search (rr_bank_search_filtered_sparse): pick_range's chunk over the PLACES of a candidate row
//     (the filter's set bits, compacted by ivf_compact_kernel, bank_ivf.hip) with a count; a workgroup behind the count ends before
//     it stages the query block, and the scores go to a compact row that topk_select_counted_kernel selects from: (b) over the
//     first `count` places, each pass's length derived from the count on the device, the list pass folded into its last pass.
// (b) topk_select_kernel: each workgroup sorts a slice of at most 4096 (score, index) in LDS by ONE total order and keeps its
//     first k (k <= 1024, so a pass is a strict reduction); passes repeat over the survivors until one slice is left.  The order
//     and its 64-bit key are rank_order.h's, shared with the pruned search: keys are distinct, so the bitonic network (written out
//     here and in plaid_list_select_kernel, see rank_order.h) has one possible result.  Survivors travel as indices; a pass reads
//     their scores again from the score row.
// LAUNCHERS: rr_launch_bank_search_scores and rr_launch_bank_search_scores_listed take an rr_bank_view (rr_common.h), fp16 or
// compressed (the listed form too: pick_list or, given a candidate list, pick_via), rr_launch_bank_search_scores_places
// (pick_places; fp16 or compressed), rr_launch_topk_select and rr_launch_topk_select_counted.  The
// operand sources, the view-to-source dispatch (li_with_bank_source), the once-per-device LDS attribute (li_lds_attr) and the
// width of the column block (li_pick_jt, here with a fixed 72 KB) live in li_sources.h, shared with li_scores.hip; the tile step
// is written out in this kernel body and in li_scores_kernel's (see li_scores.hip's header).
#include <algorithm>
#include <atomic>
#include <type_traits>

#include "li_sources.h"
#include "rank_order.h"
#include "rr_common.h"

namespace {

constexpr int BS_JT_MAX = 8;             // query tiles (16 columns) per column block
constexpr int BS_CHUNK_MAX = 128;        // passages of a workgroup's chunk (psum)
constexpr int SEL_SLICE = 4096;          // (score, index) entries one workgroup sorts
constexpr int SEL_THREADS = 512;

// Which passages a workgroup of the scoring kernel owns, and where their scores go (PICK).  at(q, p0, i, n): the table entry of
// the workgroup's passage i; slot(q, n, p0, i, pi): its place in `out`.
// pick_range: `chunk` consecutive passages of the range; out is the dense [nq][n].
struct pick_range {
  int chunk;
  static constexpr int PSUM = BS_CHUNK_MAX;
  static constexpr bool LISTED = false;
  static constexpr bool FILTERED = false;
  __device__ __forceinline__ int first(int c) const { return c * chunk; }
  __device__ __forceinline__ int count(int, int p0, int n) const { return min(chunk, n - p0); }
  __device__ __forceinline__ int at(int, int p0, int i, int) const { return p0 + i; }
  __device__ __forceinline__ size_t slot(int q, int n, int p0, int i, int) const { return (size_t)q * n + p0 + i; }
};
// pick_range_bits: pick_range under a filter.  allowed(q, p0, i): the bit of the workgroup's passage i; any(q, p0, pn): whether one
// of its pn passages has its bit set (the words of the chunk, at most five, their ends cut to the chunk).
struct pick_range_bits : pick_range {
  rr_passage_filter f;
  static constexpr bool FILTERED = true;
  __device__ __forceinline__ bool allowed(int q, int p0, int i) const { return f.allowed(q, p0 + i); }
  __device__ __forceinline__ bool any(int q, int p0, int pn) const {
    const int a = f.first + p0, b = a + pn - 1;               // the chunk's first and last bank index
    uint32_t seen = 0u;
    for (int w = a >> 5; w <= (b >> 5); ++w) {
      uint32_t m = 0xffffffffu;
      if (w == (a >> 5)) m &= 0xffffffffu << (a & 31);
      if (w == (b >> 5)) m &= 0xffffffffu >> (31 - (b & 31));
      seen |= f.word(q, w) & m;
    }
    return seen != 0u;
  }
};
// pick_list: four entries, one per wave, of the first cnt[q] of list[q][0 .. list_ld) (an entry outside [0, n) is clamped); a score
// goes to its passage's entry of the dense row out[q][.].  A workgroup behind the count has nothing to do.
struct pick_list {
  const int32_t* list;
  int list_ld;
  const int32_t* cnt;
  static constexpr int PSUM = 4;
  static constexpr bool LISTED = true;
  static constexpr bool FILTERED = false;
  __device__ __forceinline__ int first(int c) const { return c * 4; }
  __device__ __forceinline__ int count(int q, int p0, int) const { return min(4, cnt[q] - p0); }
  __device__ __forceinline__ int at(int q, int p0, int i, int n) const {
    return min(max(__builtin_amdgcn_readfirstlane(list[(size_t)q * list_ld + p0 + i]), 0), n - 1);
  }
  __device__ __forceinline__ size_t slot(int q, int n, int, int, int pi) const { return (size_t)q * n + pi; }
};
// pick_via: pick_list through a candidate list: a list entry is a PLACE of cand[q][0 .. cap) (clamped), the passage is the entry of
// cand there (clamped into [0, n)), and the score goes to that place of the compact row out[q][0 .. cap).
struct pick_via {
  const int32_t* list;
  int list_ld;
  const int32_t* cnt;
  const int32_t* cand;
  int cap;
  static constexpr int PSUM = 4;
  static constexpr bool LISTED = true;
  static constexpr bool FILTERED = false;
  __device__ __forceinline__ int first(int c) const { return c * 4; }
  __device__ __forceinline__ int count(int q, int p0, int) const { return min(4, cnt[q] - p0); }
  __device__ __forceinline__ int place(int q, int p0, int i) const {
    return min(max(__builtin_amdgcn_readfirstlane(list[(size_t)q * list_ld + p0 + i]), 0), cap - 1);
  }
  __device__ __forceinline__ int at(int q, int p0, int i, int n) const {
    return min(max(__builtin_amdgcn_readfirstlane(cand[(size_t)q * cap + place(q, p0, i)]), 0), n - 1);
  }
  __device__ __forceinline__ size_t slot(int q, int, int p0, int i, int) const { return (size_t)q * cap + place(q, p0, i); }
};
// pick_places: `chunk` consecutive PLACES of the query's candidate row cand[r][0 .. pitch), r = 0 for one shared row (rows == 1), else
// the query; the first cnt[r] places hold passages (clamped into [0, n)), and a score goes to its place of the compact row
// out[q][0 .. pitch).  pick_range's chunk over a list: the query block is staged once per chunk, not once per four entries.  A
// workgroup behind the count has nothing to do.
struct pick_places {
  int chunk;
  const int32_t* cand;
  const int32_t* cnt;
  int rows;
  int pitch;
  static constexpr int PSUM = BS_CHUNK_MAX;
  static constexpr bool LISTED = true;
  static constexpr bool FILTERED = false;
  __device__ __forceinline__ int row(int q) const { return rows == 1 ? 0 : q; }
  __device__ __forceinline__ int first(int c) const { return c * chunk; }
  __device__ __forceinline__ int count(int q, int p0, int) const { return min(chunk, min(cnt[row(q)], pitch) - p0); }
  __device__ __forceinline__ int at(int q, int p0, int i, int n) const {
    return min(max(__builtin_amdgcn_readfirstlane(cand[(size_t)row(q) * pitch + p0 + i]), 0), n - 1);
  }
  __device__ __forceinline__ size_t slot(int q, int, int p0, int i, int) const { return (size_t)q * pitch + p0 + i; }
};

template <int JT, class SRC, class PICK>
__global__ __launch_bounds__(256) void bank_search_scores_kernel(const float* __restrict__ query_li, const SRC src,
                                                                 const rr_bank_slot* __restrict__ table, int n, int nq, const PICK pick,
                                                                 int Lq, int D, float* __restrict__ out) {
  constexpr int JB = 16 * JT;            // columns per block
  extern __shared__ __attribute__((aligned(16))) float qblk[];      // [JB][D + 4]: the block's query rows; TILE: the tiles behind
  __shared__ float psum[PICK::PSUM];     // the running column sum of the workgroup's passages between column blocks
  const int ldq = D + 4;                 // as li_scores_kernel
  const int q = blockIdx.x % nq, p0 = pick.first(blockIdx.x / nq), pn = pick.count(q, p0, n);
  if constexpr (PICK::LISTED)
    if (pn <= 0) return;                 // the whole workgroup
  if constexpr (PICK::FILTERED)
    if (!pick.any(q, p0, pn)) {          // the whole workgroup: no passage of the chunk is allowed
      for (int i = threadIdx.x; i < pn; i += 256) out[pick.slot(q, n, p0, i, 0)] = -INFINITY;
      return;
    }
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, g = lane >> 4;
  const float* Q = query_li + (size_t)q * Lq * D;
  uint16_t* tile = SRC::TILE ? (uint16_t*)(qblk + JB * ldq) + wave * 16 * (D + LI_TILE_PAD) : nullptr;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  for (int j0 = 0; j0 < Lq; j0 += JB) {
    __syncthreads();                     // every wave is done with the last block's query rows (and psum is written)
    for (int i = threadIdx.x; i < JB * (D / 4); i += 256) {
      const int row = i / (D / 4), col = (i - row * (D / 4)) * 4;
      *(f32x4*)(qblk + row * ldq + col) = j0 + row < Lq ? *(const f32x4*)(Q + (size_t)(j0 + row) * D + col) : zero4;
    }
    __syncthreads();
    const bool last = j0 + JB >= Lq;
    for (int i = wave; i < pn; i += 4) {                      // a passage belongs to one wave
      if constexpr (PICK::FILTERED)
        if (!pick.allowed(q, p0, i)) {                        // wave-uniform: the passage is not read
          if (last && lane == 0) out[pick.slot(q, n, p0, i, 0)] = -INFINITY;
          continue;
        }
      const int pi = pick.at(q, p0, i, n);
      const rr_bank_slot sl = table[pi];                      // the same entry in every lane: kept in scalar registers
      const typename SRC::pair_t pr = src.of(uniform_i64(sl.first_row), __builtin_amdgcn_readfirstlane(sl.len), q, 0, D);
      const int len = pr.len, c_tiles = (len + 15) / 16;
      float cmax[JT];
#pragma unroll
      for (int t = 0; t < JT; ++t) cmax[t] = -INFINITY;
      for (int ct = 0; ct < c_tiles; ++ct) {
        const int c = ct * 16 + li;                           // the context row this lane feeds to the matrix core
        const bool c_ok = c < len;
        f32x4 acc[JT];
#pragma unroll
        for (int t = 0; t < JT; ++t) acc[t] = zero4;
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
          const f32x4 a_n = (c_ok && d + 16 < D) ? SRC::at(crow, d + 16) : zero4;      // requested a step ahead
          f32x4 b[JT];
#pragma unroll
          for (int t = 0; t < JT; ++t) b[t] = *(const f32x4*)(qrow + t * 16 * ldq + d);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int t = 0; t < JT; ++t)
              acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[t][e], acc[t], 0, 0, 0);
          }
          a = a_n;
        }
        // accumulator element r of this lane: row ct * 16 + 4 g + r, column j0 + t * 16 + li
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = ct * 16 + 4 * g + r;
          if (row >= len) continue;
          const bool keep = src.keep(pr, row);
#pragma unroll
          for (int t = 0; t < JT; ++t)
            if (j0 + t * 16 + li < Lq) cmax[t] = nan_max(cmax[t], keep ? acc[t][r] : LI_MASKED);
        }
      }
      float sum = j0 ? psum[i] : 0.0f;                        // every lane of the wave carries the same sum
#pragma unroll
      for (int t = 0; t < JT; ++t) {
        float v = cmax[t];
        v = nan_max(v, __shfl_xor(v, 16, 64));
        v = nan_max(v, __shfl_xor(v, 32, 64));
#pragma unroll
        for (int l = 0; l < 16; ++l) {
          const float x = __shfl(v, l, 64);
          if (j0 + t * 16 + l < Lq) sum += x;                 // columns 0, 1, ... Lq - 1, one after the other
        }
      }
      if (lane == 0) {
        if (last) out[pick.slot(q, n, p0, i, pi)] = sum;
        else psum[i] = sum;
      }
    }
  }
}

// rr_set_tuning("search_chunk"): passages per workgroup of the scoring kernel
std::atomic<int> g_search_chunk{16};

// one launch of `chunks` workgroups per query; the width of the column block is decided here for both pickers
template <int JT, class SRC, class PICK>
hipError_t search_launch_jt(const float* query_li, const SRC& src, const rr_bank_slot* table, int n, int nq, long long chunks, const PICK& pick,
                            int Lq, int D, size_t lds, float* out, hipStream_t st) {
  static std::atomic<unsigned long long> attr_set{0};
  const hipError_t e = li_lds_attr((const void*)bank_search_scores_kernel<JT, SRC, PICK>, attr_set);
  if (e != hipSuccess) return e;
  const long long blocks = chunks * nq;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((bank_search_scores_kernel<JT, SRC, PICK>), dim3((unsigned)blocks), dim3(256), lds, st, query_li, src, table, n, nq,
                     pick, Lq, D, out);
  return hipGetLastError();
}

template <class SRC, class PICK>
hipError_t search_launch(const float* query_li, const SRC& src, const rr_bank_slot* table, int n, int nq, long long chunks, const PICK& pick,
                         int Lq, int D, size_t tile_bytes, float* out, hipStream_t st) {
  // the column block is halved above a fixed 72 KB (any width gives the same bits: the sum is carried between blocks)
  size_t lds = 0;
  const int jt = li_pick_jt(Lq, D, tile_bytes, (size_t)72 * 1024, &lds);
  if (jt == 0) return hipErrorInvalidValue;
  if (jt == 1) return search_launch_jt<1>(query_li, src, table, n, nq, chunks, pick, Lq, D, lds, out, st);
  if (jt == 2) return search_launch_jt<2>(query_li, src, table, n, nq, chunks, pick, Lq, D, lds, out, st);
  if (jt == 4) return search_launch_jt<4>(query_li, src, table, n, nq, chunks, pick, Lq, D, lds, out, st);
  return search_launch_jt<BS_JT_MAX>(query_li, src, table, n, nq, chunks, pick, Lq, D, lds, out, st);
}

bool scores_args_ok(const rr_bank_slot* table, int n, int nq, int Lq, const float* query_li, const float* out) {
  return n > 0 && nq > 0 && Lq > 0 && table && query_li && out && !((((uintptr_t)query_li) | ((uintptr_t)table)) & 15);
}

// One pass.  List `blockIdx.y`, slice `blockIdx.x` of its n_in entries: entry i is index idx_in[list][i] of the score row (idx_in
// null: i itself).  The slice's first min(k, entries) in rank order go to idx_out[list * out_ld + slice * k ...]; the last pass
// (one slice) writes `add` + index and, if asked, the scores.
__global__ __launch_bounds__(SEL_THREADS) void topk_select_kernel(const float* __restrict__ scores, long long n, const int32_t* __restrict__ idx_in,
                                                                  long long in_ld, int n_in, int k, int32_t* __restrict__ idx_out,
                                                                  long long out_ld, int add, float* __restrict__ scores_out) {
  __shared__ unsigned long long key[SEL_SLICE];
  const int list = blockIdx.y, base = blockIdx.x * SEL_SLICE, cnt = min(SEL_SLICE, n_in - base), tid = threadIdx.x;
  const float* row = scores + (size_t)list * n;
  int n2 = 1;
  while (n2 < cnt) n2 <<= 1;
  for (int i = tid; i < n2; i += SEL_THREADS) {
    unsigned long long kv = 0ull;                             // padding ranks behind every entry
    if (i < cnt) {
      const int idx = idx_in ? idx_in[(size_t)list * in_ld + base + i] : base + i;
      kv = rank_key(row[idx], (uint32_t)idx);
    }
    key[i] = kv;
  }
  __syncthreads();
  for (int kk = 2; kk <= n2; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n2; i += SEL_THREADS) {
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
  const int keep = min(k, cnt);
  const bool final_pass = gridDim.x == 1;
  for (int i = tid; i < keep; i += SEL_THREADS) {
    const int idx = (int)rank_key_index(key[i]);
    if (final_pass) {
      idx_out[(size_t)list * out_ld + i] = idx + add;
      if (scores_out) scores_out[(size_t)list * out_ld + i] = row[idx];
    } else {
      idx_out[(size_t)list * out_ld + (size_t)blockIdx.x * k + i] = idx;
    }
  }
}

// the entries a list of cnt entries still has at pass `pass` of the selection: the host loop of rr_launch_topk_select, on the device
__device__ __forceinline__ int counted_entries(int cnt, int k, int pass) {
  int n_in = cnt;
  for (int p = 0; p < pass; ++p) {
    const int slices = (n_in + SEL_SLICE - 1) / SEL_SLICE;
    n_in = slices ? (slices - 1) * k + min(k, n_in - (slices - 1) * SEL_SLICE) : 0;      // (one slice: its min(k, n_in) survivors again)
  }
  return n_in;
}

// topk_select_kernel over COMPACT rows: list `blockIdx.y` is the first cnt_in[r] places of scores[list][0 .. pitch), r = 0 for one
// shared row (rows == 1), else the list; whatever lies behind the count is never read.  The key holds the place, and places ascend
// with the bank index, so the order is topk_select_kernel's.  The grid is the one the whole pitch would need; what a list holds at
// pass `pass` follows from its count (counted_entries), and a slice behind that ends at once.  The last pass (one slice) drops the
// -inf scorers, maps a place to add + cand[r][place] (cand null: add + place) and writes -1 / -inf behind the survivors up to k and
// their number to counts_out: what plaid_list_select_kernel does for the dense form.
__global__ __launch_bounds__(SEL_THREADS) void topk_select_counted_kernel(const float* __restrict__ scores, int pitch, const int32_t* __restrict__ cnt_in,
                                                                          const int32_t* __restrict__ cand, long long cand_ld, int rows,
                                                                          const int32_t* __restrict__ idx_in, long long in_ld, int pass, int k,
                                                                          int32_t* __restrict__ idx_out, long long out_ld, int add,
                                                                          float* __restrict__ scores_out, int32_t* __restrict__ counts_out) {
  __shared__ unsigned long long key[SEL_SLICE];
  __shared__ int valid;
  const int list = blockIdx.y, r = rows == 1 ? 0 : list, base = blockIdx.x * SEL_SLICE, tid = threadIdx.x;
  const bool final_pass = gridDim.x == 1;
  const int n_in = counted_entries(min(max(cnt_in[r], 0), pitch), k, pass);
  const int cnt = max(min(SEL_SLICE, n_in - base), 0);
  if (!final_pass && cnt == 0) return;                        // the whole workgroup: the slice lies behind the list
  const float* row = scores + (size_t)list * pitch;
  int n2 = 1;
  while (n2 < cnt) n2 <<= 1;
  if (tid == 0) valid = 0;
  for (int i = tid; i < n2; i += SEL_THREADS) {
    unsigned long long kv = 0ull;                             // padding, and in the last pass the absent, rank behind every entry
    if (i < cnt) {
      const int idx = idx_in ? idx_in[(size_t)list * in_ld + base + i] : base + i;
      const float s = row[idx];
      if (!final_pass || s != -INFINITY) kv = rank_key(s, (uint32_t)idx);
    }
    key[i] = kv;
  }
  __syncthreads();
  for (int kk = 2; kk <= n2; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n2; i += SEL_THREADS) {
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
  if (!final_pass) {
    const int keep = min(k, cnt);
    for (int i = tid; i < keep; i += SEL_THREADS)
      idx_out[(size_t)list * out_ld + (size_t)blockIdx.x * k + i] = (int)rank_key_index(key[i]);
    return;
  }
  for (int i = tid; i < n2; i += SEL_THREADS)
    if (key[i] != 0ull && (i == n2 - 1 || key[i + 1] == 0ull)) valid = i + 1;      // one thread at most
  __syncthreads();
  const int kept = min(k, valid);
  for (int i = tid; i < k; i += SEL_THREADS) {
    int32_t o = -1;
    float s = -INFINITY;
    if (i < kept) {
      const int idx = (int)rank_key_index(key[i]);
      o = (cand ? cand[(size_t)r * cand_ld + idx] : idx) + add;
      s = row[idx];
    }
    idx_out[(size_t)list * out_ld + i] = o;
    if (scores_out) scores_out[(size_t)list * out_ld + i] = s;
  }
  if (tid == 0) counts_out[list] = kept;
}

}  // namespace

int rr_set_search_chunk(int passages) {
  if (passages < 4 || passages > BS_CHUNK_MAX) return -1;
  g_search_chunk.store(passages, std::memory_order_relaxed);
  return 0;
}

// out [nq][n]: the MaxSim of every query against the passages table[0 .. n) of a bank, fp16 or compressed (li_with_bank_source);
// under a filter (filter.bits given) -inf for a passage whose bit is clear
hipError_t rr_launch_bank_search_scores(const rr_bank_slot* table, int n, int nq, int Lq, int D, const float* query_li,
                                        const rr_bank_view& bank, const rr_passage_filter& filter, float* out, hipStream_t st) {
  if (!scores_args_ok(table, n, nq, Lq, query_li, out)) return hipErrorInvalidValue;
  if (filter.bits && ((filter.rows != 1 && filter.rows != nq) || filter.first < 0 || filter.ld < ((long long)filter.first + n + 31) / 32))
    return hipErrorInvalidValue;
  const int chunk = g_search_chunk.load(std::memory_order_relaxed);
  auto with = [&](const auto& pick) {    // (a dispatch per picker, as below)
    return li_with_bank_source(nullptr, nullptr, bank, D, [&](const auto& src, size_t tile_bytes) {
      return search_launch(query_li, src, table, n, nq, ((long long)n + chunk - 1) / chunk, pick, Lq, D, tile_bytes, out, st);
    });
  };
  return !filter.bits ? with(pick_range{chunk}) : with(pick_range_bits{{chunk}, filter});
}

// the same MaxSim for the passages list[q][0 .. cnt[q]) (entries of table[0 .. n), cnt[q] <= list_ld) of every query q, written to
// out[q][entry] of the dense [nq][n]; the rest of `out` is left as it is.  The pruned search is the caller: a compressed bank, or
// an fp16 bank with codes (the view's nbits == 0: li_src_f16, the rows rr_bank_search reads).
// cand / cap null / 0: pick_list.  Given: pick_via, a list entry is a place in cand [nq][cap] and out the compact [nq][cap].
hipError_t rr_launch_bank_search_scores_listed(const rr_bank_slot* table, int n, int nq, int Lq, int D, const float* query_li,
                                               const rr_bank_view& bank, const int32_t* list, int list_ld, const int32_t* cnt,
                                               const int32_t* cand, int cap, float* out, hipStream_t st) {
  if (!scores_args_ok(table, n, nq, Lq, query_li, out) || !list || !cnt || list_ld <= 0 || (cand ? cap <= 0 : cap != 0))
    return hipErrorInvalidValue;
  auto with = [&](const auto& pick) {    // (a dispatch per picker: the kernels stay in the order the object had them in)
    return li_with_bank_source(nullptr, nullptr, bank, D, [&](const auto& src, size_t tile_bytes) -> hipError_t {
      return search_launch(query_li, src, table, n, nq, (list_ld + 3) / 4, pick, Lq, D, tile_bytes, out, st);
    });
  };
  return !cand ? with(pick_list{list, list_ld, cnt}) : with(pick_via{list, list_ld, cnt, cand, cap});
}

// the same MaxSim for the passages cand[r][0 .. cnt[r]) (range-relative entries of table[0 .. n); r = 0 if rows == 1, else the query;
// cand [rows][pitch], cnt[r] <= pitch) of every query, written to the passage's PLACE of the compact out [nq][pitch]; the places
// behind a count are left as they are.  pick_places: chunks of search_chunk places, fp16 and compressed banks alike.
hipError_t rr_launch_bank_search_scores_places(const rr_bank_slot* table, int n, int nq, int Lq, int D, const float* query_li,
                                               const rr_bank_view& bank, const int32_t* cand, const int32_t* cnt, int rows, int pitch,
                                               float* out, hipStream_t st) {
  if (!scores_args_ok(table, n, nq, Lq, query_li, out) || !cand || !cnt || (rows != 1 && rows != nq) || pitch <= 0) return hipErrorInvalidValue;
  const int chunk = g_search_chunk.load(std::memory_order_relaxed);
  return li_with_bank_source(nullptr, nullptr, bank, D, [&](const auto& src, size_t tile_bytes) {
    return search_launch(query_li, src, table, n, nq, ((long long)pitch + chunk - 1) / chunk, pick_places{chunk, cand, cnt, rows, pitch}, Lq, D,
                         tile_bytes, out, st);
  });
}

// int32 entries of EACH of the two survivor buffers rr_launch_topk_select needs (0: one slice, none)
size_t rr_topk_select_scratch(int n_lists, int n, int k) {
  if (n <= SEL_SLICE) return 0;
  return (size_t)n_lists * (size_t)((n + SEL_SLICE - 1) / SEL_SLICE) * (size_t)k;
}

// the first k of every list scores [n_lists][n] in rank order: indices_out [n_lists][k] (+ add), scores_out [n_lists][k] or null.
// 1 <= k <= min(n, 1024); tmp_a / tmp_b: rr_topk_select_scratch entries each
hipError_t rr_launch_topk_select(const float* scores, int n_lists, int n, int k, int add, int32_t* tmp_a, int32_t* tmp_b,
                                 int32_t* indices_out, float* scores_out, hipStream_t st) {
  if (!scores || !indices_out || n_lists <= 0 || n_lists > 65535 || n <= 0 || k < 1 || k > n || k > 1024) return hipErrorInvalidValue;
  if (n > SEL_SLICE && (!tmp_a || !tmp_b)) return hipErrorInvalidValue;
  const long long ld = (long long)((n + SEL_SLICE - 1) / SEL_SLICE) * k;      // row pitch of both survivor buffers
  const int32_t* in = nullptr;
  int32_t* bufs[2] = {tmp_a, tmp_b};
  int n_in = n, pass = 0;
  for (;;) {
    const int slices = (n_in + SEL_SLICE - 1) / SEL_SLICE;
    const bool final_pass = slices == 1;
    int32_t* o = final_pass ? indices_out : bufs[pass & 1];
    hipLaunchKernelGGL(topk_select_kernel, dim3((unsigned)slices, (unsigned)n_lists), dim3(SEL_THREADS), 0, st, scores, (long long)n, in, ld,
                       n_in, k, o, final_pass ? (long long)k : ld, add, final_pass ? scores_out : nullptr);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || final_pass) return e;
    // every slice but the last is full and leaves k; the last leaves what it holds, at most k: the survivors are contiguous
    n_in = (slices - 1) * k + std::min(k, n_in - (slices - 1) * SEL_SLICE);
    in = o;
    ++pass;
  }
}

// rr_launch_topk_select over compact rows (topk_select_counted_kernel): list l is the first cnt[r] entries of scores[l][0 .. pitch),
// r = 0 if rows == 1, else l; rows is 1 or n_lists.  Of their entries that are not -inf the first k in rank order go to indices_out
// [n_lists][k] as add + cand[r][place] (cand [rows][cand_ld >= pitch]; null: add + place) and to scores_out (or null), -1 / -inf behind
// them, their number to counts_out [n_lists].  The passes are those `pitch` entries would need: the counts stay on the device, and
// nothing is read back.  1 <= k <= min(pitch, 1024); tmp_a / tmp_b: rr_topk_select_scratch(n_lists, pitch, k) entries each.
hipError_t rr_launch_topk_select_counted(const float* scores, int n_lists, int pitch, const int32_t* cnt, const int32_t* cand, long long cand_ld,
                                         int rows, int k, int add, int32_t* tmp_a, int32_t* tmp_b, int32_t* indices_out, float* scores_out,
                                         int32_t* counts_out, hipStream_t st) {
  if (!scores || !cnt || !indices_out || !counts_out || n_lists <= 0 || n_lists > 65535 || pitch <= 0 || k < 1 || k > pitch || k > 1024)
    return hipErrorInvalidValue;
  if ((rows != 1 && rows != n_lists) || (cand && cand_ld < pitch)) return hipErrorInvalidValue;
  if (pitch > SEL_SLICE && (!tmp_a || !tmp_b)) return hipErrorInvalidValue;
  const long long ld = (long long)((pitch + SEL_SLICE - 1) / SEL_SLICE) * k;  // row pitch of both survivor buffers
  const int32_t* in = nullptr;
  int32_t* bufs[2] = {tmp_a, tmp_b};
  int n_in = pitch, pass = 0;
  for (;;) {
    const int slices = (n_in + SEL_SLICE - 1) / SEL_SLICE;
    const bool final_pass = slices == 1;
    int32_t* o = final_pass ? indices_out : bufs[pass & 1];
    hipLaunchKernelGGL(topk_select_counted_kernel, dim3((unsigned)slices, (unsigned)n_lists), dim3(SEL_THREADS), 0, st, scores, pitch, cnt, cand,
                       cand_ld, rows, in, ld, pass, k, o, final_pass ? (long long)k : ld, add, final_pass ? scores_out : nullptr,
                       final_pass ? counts_out : nullptr);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || final_pass) return e;
    n_in = (slices - 1) * k + std::min(k, n_in - (slices - 1) * SEL_SLICE);    // (a shorter list's own length: counted_entries)
    in = o;
    ++pass;
  }
}
