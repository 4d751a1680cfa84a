// The inverted file of a compressed passage bank (rr_bank_build_ivf, include/rerank_mi355.h, "THE INVERTED FILE"): per centroid the
// sorted unique passages with an unmasked row of that code, what the reference keeps as ivf.pid.pt (_build_ivf, third_party/ColBERT/
// colbert/indexing/collection_indexer.py:393-431; optimize_ivf, indexing/utils.py:8-48), built from the codes the bank holds; and
// the candidate step of rr_bank_search_plaid_ivf, which reads it (candidate_generation.py).
// BUILD, rr_ivf_build (a load-time call: it allocates and synchronises):
//   (a) ivf_mark_kernel<false>: a WAVE per passage.  Lanes load 64 codes per step (masked: -1) and a row is a FIRST OCCURRENCE iff
//       no earlier unmasked row of the passage has its code: the rows of the same step are compared lane by lane (readlane, the
//       step stays in registers), the rows of earlier steps are loaded again step by step and compared the same way, so a passage
//       of any length takes no LDS.  A first occurrence adds 1 to its centroid's count (32-bit vector atomic on integers: one
//       result in any order).
//   (b) ivf_scan_kernel: one workgroup, the exclusive scan of the counts into int64 offsets [C + 1], the postings total and the
//       longest list, which the host reads back to size `pids` and the search's scratch.
//   (c) ivf_mark_kernel<true>: the same walk; a first occurrence takes a place in its list through the centroid's atomic cursor.
//       WHICH place depends on scheduling; (d) removes that.
//   (d) ivf_sort_kernel: a workgroup per list of 2 .. 4096 entries sorts it ascending in LDS (a bitonic network over distinct
//       integers: one result).  A longer list is rebuilt: its passages set their bits in a bitmap of P bits (atomicOr: a set has
//       no order) and ivf_compact_kernel writes the set bits out in ascending order.
// EXTEND, rr_ivf_build with `old`, the file over the first P0 < P passages (rr_bank_extend_ivf; a load-time call like the build, the
// same function): an add only brings indices above every index of the file, so a new list is the old list followed by the sorted
// new entries.  The file is written into fresh allocations; `old` is only read.
//   (a) ivf_mark_kernel<false> over the passages P0 .. P - 1 alone: the table holds the new slots, p_base = P0 makes slot p the
//       bank passage P0 + p.
//   (b) ivf_scan_kernel with the old offsets: offsets[c] = old[c] + the exclusive scan of the new counts, the total, the longest
//       MERGED list and the longest TAIL (what (d) has to sort), one launch, int64.  A list's tail starts at offsets[c] +
//       (old[c + 1] - old[c]): both offset arrays are live for the call, so (c) and (d) compute it and no array holds it.
//   (s) ivf_shift_copy_kernel: the old postings to their new places.  The shift offsets[c] - old[c] never decreases with c and the
//       destination is fresh, so one launch does it; the work is cut into runs of IVF_SHIFT_RUN old postings, not by list (one list
//       holding every passage costs what many short ones cost; the grid is postings_old / IVF_SHIFT_RUN, whatever the longest list).
//   (c) ivf_mark_kernel<true> over the new passages, the cursors starting at the tails.
//   (d) ivf_sort_kernel over the tails of 2 .. 4096 entries; a longer tail through the bitmap, which covers the P - P0 new passages
//       (bit i: passage P0 + i; the compaction adds P0 back).  The old part of a list is never touched again.
// SEARCH, rr_launch_ivf_candidates: per query a bitmap over the passages of the range is cleared, ivf_candidates_kernel (a
// workgroup per (query, cell entry); an entry that repeats an earlier one of its query ends at once) ORs in the passages of the
// cell's list that lie inside the range (found by two binary searches: the list is sorted), and ivf_compact_kernel turns every
// bitmap into the ascending candidate list [nq][cap] with its count and writes -inf behind the count into the two compact score
// rows.  Sets and sorted lists only: nothing depends on scheduling.  Under a caller's filter (rr_bank_search_plaid_ivf_filtered)
// the compaction ANDs every word it reads with the filter's bits of those passages: the filter is indexed by bank index and the
// bitmap starts at the range's first passage, so a word takes its bits from two filter words when that is no multiple of 32
// (rr_passage_filter::range_word).  No launch more.
// rr_launch_filter_fill (rr_bank_filter_fill): filter_fill_kernel, a workgroup per row, writes the row's words (zeros, or ones below
// the passage count), meets at a barrier and then clears or sets the bits of the row's list with vector atomicAnd / atomicOr: an AND
// or an OR has one result.  rr_filter_bits_host restates it (rr_util_bank_filter_bits).
// ivf_compact_kernel: ONE workgroup of 1024 per bitmap walks it 1024 words a time: a popcount per word, an inclusive scan over the
// workgroup (wave shuffles, the sixteen wave totals through LDS), and every thread writes the bits of its word from its place on.
// WHERE a word comes from is a type (WORDS): words_bitmap, the bitmap ANDed with a filter, as above; words_filter, the filter's own
// bits of the range and no bitmap (rr_launch_filter_compact: the candidate rows of rr_bank_search_filtered_sparse), the last word cut
// to the range.  The type holds no data, so the bitmap form keeps its arguments and its instructions.
// rr_ivf_host restates the definition in host code (rr_util_plaid_ivf).
#include <algorithm>
#include <cmath>
#include <vector>

#include "rank_order.h"
#include "rr_common.h"

namespace {

constexpr int IVF_SORT_MAX = 4096;       // entries ivf_sort_kernel sorts in LDS
constexpr int IVF_COMPACT_THREADS = 1024;
constexpr int IVF_SHIFT_THREADS = 128;   // ivf_shift_copy_kernel: a workgroup and
constexpr int IVF_SHIFT_RUN = 512;       // the old postings it moves: 2 KB, one 16-byte access a thread

__device__ __forceinline__ long long shfl_up_i64(long long v, int d) {
  const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)((unsigned long long)v >> 32), d, 64);
  return (long long)(((unsigned long long)hi << 32) | lo);
}

// table [P]: the passages the launch walks; slot p is bank passage p_base + p, the index a list holds.  old_offsets (or null; the
// extend): a list's cursor starts behind the old_offsets[c + 1] - old_offsets[c] entries it holds already, at its tail.
template <bool FILL>
__global__ __launch_bounds__(256) void ivf_mark_kernel(const int32_t* __restrict__ codes, const uint8_t* __restrict__ mask,
                                                       const rr_bank_slot* __restrict__ table, int P, int p_base, int C,
                                                       uint32_t* __restrict__ counts, const int64_t* __restrict__ offsets,
                                                       const int64_t* __restrict__ old_offsets, int32_t* __restrict__ pids) {
  const int lane = threadIdx.x & 63;
  const long long pl = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pl >= P) return;                                        // the whole wave
  const int p = __builtin_amdgcn_readfirstlane((int)pl);
  const rr_bank_slot sl = table[p];
  const long long first_row = uniform_i64(sl.first_row);
  const int len = __builtin_amdgcn_readfirstlane(sl.len);
  for (int base = 0; base < len; base += 64) {
    const int r = base + lane;
    int code = -1;                                            // masked, or behind the end: no occurrence
    if (r < len && mask[first_row + r]) code = min(max(codes[first_row + r], 0), C - 1);
    bool first = code >= 0;
    for (int eb = 0; eb < base; eb += 64) {                   // the steps before this one: 64 rows each, all inside the passage
      int ec = -1;
      if (mask[first_row + eb + lane]) ec = min(max(codes[first_row + eb + lane], 0), C - 1);
      for (int t = 0; t < 64; ++t)
        if (__builtin_amdgcn_readlane(ec, t) == code) first = false;      // (-1 meets -1 only where first is false already)
    }
    const int cnt = min(64, len - base);
    for (int t = 0; t < cnt; ++t)
      if (__builtin_amdgcn_readlane(code, t) == code && t < lane) first = false;
    if (first) {
      const uint32_t pos = atomicAdd(&counts[code], 1u);
      if constexpr (FILL) {
        int64_t o = offsets[code];
        if (old_offsets) o += old_offsets[code + 1] - old_offsets[code];
        if ((int64_t)pos < offsets[code + 1] - o) pids[o + pos] = p_base + p;
      }
    }
  }
}

// info[0]: the postings total, info[1]: the longest list.  old (or null; the extend) [C + 1]: the offsets of a file whose lists the
// counts are appended to: offsets[c] = old[c] + the exclusive scan, the total and the longest list are those of the merged lists
// (old[c + 1] - old[c] + counts[c]: at most the passages held, 32 bits), and info[2] is the longest tail, max counts[c].
__global__ __launch_bounds__(1024) void ivf_scan_kernel(const uint32_t* __restrict__ counts, int C, const int64_t* __restrict__ old,
                                                        int64_t* __restrict__ offsets, int64_t* __restrict__ info) {
  __shared__ long long wsum[16];
  __shared__ uint32_t wmax[16], wtail[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long per = ((long long)C + 1023) / 1024;
  const int c0 = tid * per < C ? (int)(tid * per) : C, c1 = c0 + per < C ? (int)(c0 + per) : C;
  long long s = 0;
  uint32_t mx = 0, tl = 0;
  for (int c = c0; c < c1; ++c) {
    s += counts[c];
    mx = max(mx, counts[c] + (old ? (uint32_t)(old[c + 1] - old[c]) : 0u));
    tl = max(tl, counts[c]);
  }
  long long incl = s;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long o = shfl_up_i64(incl, d);
    if (lane >= d) incl += o;
  }
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, m, 64));
    tl = max(tl, (uint32_t)__shfl_xor((int)tl, m, 64));
  }
  if (lane == 63) wsum[wave] = incl;
  if (lane == 0) {
    wmax[wave] = mx;
    wtail[wave] = tl;
  }
  __syncthreads();
  long long run = incl - s;
  for (int w = 0; w < wave; ++w) run += wsum[w];
  for (int c = c0; c < c1; ++c) {
    offsets[c] = run + (old ? old[c] : 0);
    run += counts[c];
  }
  if (tid == 1023) {                                          // the last thread ends at the total
    if (old) run += old[C];
    offsets[C] = run;
    info[0] = run;
  }
  if (tid == 0) {
    uint32_t m = 0, t = 0;
    for (int w = 0; w < 16; ++w) {
      m = max(m, wmax[w]);
      t = max(t, wtail[w]);
    }
    info[1] = m;
    if (old) info[2] = t;
  }
}

// workgroup c sorts list c, or with old_offsets (the extend) its tail alone: the entries behind the old_offsets[c + 1] -
// old_offsets[c] the list held before
__global__ __launch_bounds__(256) void ivf_sort_kernel(const int64_t* __restrict__ offsets, const int64_t* __restrict__ old_offsets,
                                                       int32_t* __restrict__ pids) {
  __shared__ uint32_t key[IVF_SORT_MAX];
  const int64_t o = offsets[blockIdx.x] + (old_offsets ? old_offsets[blockIdx.x + 1] - old_offsets[blockIdx.x] : 0);
  const int64_t cnt64 = offsets[blockIdx.x + 1] - o;
  if (cnt64 < 2 || cnt64 > IVF_SORT_MAX) return;              // the whole workgroup
  const int cnt = (int)cnt64, tid = threadIdx.x;
  int n2 = 2;
  while (n2 < cnt) n2 <<= 1;
  for (int i = tid; i < n2; i += 256) key[i] = i < cnt ? (uint32_t)pids[o + i] : 0xffffffffu;      // padding behind every passage
  __syncthreads();
  for (int kk = 2; kk <= n2; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n2; i += 256) {
        const int l = i ^ j;
        if (l > i) {
          const bool up = (i & kk) == 0;                      // an ascending run
          const uint32_t a = key[i], b = key[l];
          if (up ? a > b : a < b) { key[i] = b; key[l] = a; }
        }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < cnt; i += 256) pids[o + i] = (int32_t)key[i];
}

// n units of U bytes from s to d, both U-aligned, by the IVF_SHIFT_THREADS threads of the workgroup
template <typename unit_t>
__device__ __forceinline__ void shift_units(const int32_t* __restrict__ s, int32_t* __restrict__ d, int n, int tid) {
  const unit_t* __restrict__ su = (const unit_t*)s;
  unit_t* __restrict__ du = (unit_t*)d;
  for (int i = tid; i < n; i += IVF_SHIFT_THREADS) du[i] = su[i];
}

// The extend's copy of the old postings to their places in the new file: entry i of list c goes from old_pids[old_offsets[c] + i] to
// new_pids[new_offsets[c] + i].  The work is cut by POSTINGS: workgroup g owns old_pids[g * IVF_SHIFT_RUN ...), IVF_SHIFT_RUN entries,
// finds the list of its first entry by binary search over old_offsets (block-uniform: the loads are scalar) and walks the lists
// from there.  A piece, the entries of one list inside the run, is contiguous on both sides; the two sides are aligned alike modulo
// w = the lowest set bit of the byte shift (at most 16): 4-byte accesses up to the first w-aligned source byte, w-byte accesses
// from there, 4-byte accesses for the rest (the piece copy of bank_move.hip at E = 4).  Plain vector loads and stores.
__global__ __launch_bounds__(IVF_SHIFT_THREADS) void ivf_shift_copy_kernel(const int64_t* __restrict__ old_offsets,
                                                                           const int64_t* __restrict__ new_offsets, int C,
                                                                           const int32_t* __restrict__ old_pids, int32_t* __restrict__ new_pids) {
  const int tid = threadIdx.x;
  const long long total = uniform_i64(old_offsets[C]);
  const long long r0 = (long long)blockIdx.x * IVF_SHIFT_RUN;
  if (r0 >= total) return;                                    // the whole workgroup
  const long long r1 = r0 + IVF_SHIFT_RUN < total ? r0 + IVF_SHIFT_RUN : total;
  int lo = 0, hi = C - 1;                                     // the last list that starts at or below r0: the one that holds entry r0
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (uniform_i64(old_offsets[mid]) <= r0) lo = mid;
    else hi = mid - 1;
  }
  int c = lo;
  long long r = r0;
  while (r < r1 && c < C) {
    const long long end = uniform_i64(old_offsets[c + 1]);
    const long long stop = end < r1 ? end : r1;
    const int cnt = (int)(stop - r);                          // at most IVF_SHIFT_RUN; none for an empty list
    if (cnt > 0) {
      const int32_t* s = old_pids + r;
      int32_t* d = new_pids + r + (uniform_i64(new_offsets[c]) - uniform_i64(old_offsets[c]));
      const unsigned rel = ((unsigned)(uintptr_t)s - (unsigned)(uintptr_t)d) & 15u;
      const int w = rel ? (int)(rel & (0u - rel)) : 16;       // 4, 8 or 16
      if (w == 4) {
        shift_units<uint32_t>(s, d, cnt, tid);
      } else {
        int head = (int)(((unsigned)w - ((unsigned)(uintptr_t)s & (unsigned)(w - 1))) & (unsigned)(w - 1)) >> 2;
        if (head > cnt) head = cnt;
        const int per = w >> 2, body = (cnt - head) / per;
        shift_units<uint32_t>(s, d, head, tid);
        if (w == 8) shift_units<uint2>(s + head, d + head, body, tid);
        else shift_units<uint4>(s + head, d + head, body, tid);
        shift_units<uint32_t>(s + head + body * per, d + head + body * per, cnt - head - body * per, tid);
      }
    }
    r = stop;
    ++c;
  }
}

// the passages list[0 .. cnt) as bits of bm (bit pid - first; a passage outside [first, first + n) sets none)
__global__ __launch_bounds__(256) void ivf_list_bits_kernel(const int32_t* __restrict__ list, long long cnt, int first, int n,
                                                            uint32_t* __restrict__ bm) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < cnt; i += (long long)gridDim.x * 256) {
    const long long r = (long long)list[i] - first;
    if (r >= 0 && r < n) atomicOr(&bm[r >> 5], 1u << (r & 31));
  }
}

__device__ __forceinline__ long long ivf_lower_bound(const int32_t* __restrict__ pids, long long lo, long long hi, long long v) {
  while (lo < hi) {                                           // the first entry of the sorted pids[lo .. hi) that is >= v
    const long long mid = lo + ((hi - lo) >> 1);
    if (pids[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// workgroup (e, q): cell entry e of query q (cells [nq][E]); the passages of its list inside [first, first + n) set their bits
__global__ __launch_bounds__(256) void ivf_candidates_kernel(const int32_t* __restrict__ cells, int E, int C, const int64_t* __restrict__ offsets,
                                                             const int32_t* __restrict__ pids, int first, int n, uint32_t* __restrict__ bm,
                                                             int Wn) {
  const int e = blockIdx.x, q = blockIdx.y, tid = threadIdx.x;
  const int32_t* cl = cells + (size_t)q * E;
  const int c = min(max(cl[e], 0), C - 1);
  bool dup = false;
  for (int i = tid; i < e; i += 256)
    if (min(max(cl[i], 0), C - 1) == c) dup = true;
  if (__syncthreads_or(dup)) return;                          // an earlier entry of the query walks this list
  const long long a = ivf_lower_bound(pids, offsets[c], offsets[c + 1], first);
  const long long b = ivf_lower_bound(pids, a, offsets[c + 1], (long long)first + n);
  uint32_t* row = bm + (size_t)q * Wn;
  for (long long i = a + tid; i < b; i += 256) {
    const long long r = (long long)pids[i] - first;
    if (r >= 0 && r < n) atomicOr(&row[r >> 5], 1u << (r & 31));      // an OR has one result
  }
}

// the word source of ivf_compact_kernel: a bitmap row (ANDed with the filter, if one is given), or the filter's bits of the range alone
struct words_bitmap { static constexpr bool FILTER_ALONE = false; };
struct words_filter { static constexpr bool FILTER_ALONE = true; };

// Workgroup q: the set bits of bm[q][0 .. Wn) in ascending order, bit + add, to out[q * out_ld ...] (at most cap of them), their
// number to cnt_out[q]; fill_a / fill_b (or null) [nq][cap] get -inf behind the count.  filter.bits given: a word is ANDed with the
// filter's bits of its passages (n: the passages of the range) as it is read.  words_filter: bm is not read, word w is the filter's
// bits of the range-relative passages 32 w .. 32 w + 31 below n, and workgroup q is filter row q.
template <class WORDS>
__global__ __launch_bounds__(IVF_COMPACT_THREADS) void ivf_compact_kernel(const uint32_t* __restrict__ bm, int Wn, int32_t* __restrict__ out,
                                                                          long long out_ld, int cap, int32_t* __restrict__ cnt_out, int add,
                                                                          float* __restrict__ fill_a, float* __restrict__ fill_b,
                                                                          const rr_passage_filter filter, int n) {
  __shared__ int wtot[2][16];
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t* row = bm + (size_t)q * Wn;
  int32_t* o = out + (size_t)q * out_ld;
  long long base = 0;
  int round = 0;
  for (int w0 = 0; w0 < Wn; w0 += IVF_COMPACT_THREADS, round ^= 1) {
    const int w = w0 + tid;
    uint32_t word;
    if constexpr (WORDS::FILTER_ALONE) {
      word = w < Wn ? filter.range_word(q, w, n) : 0u;
      if (w == Wn - 1 && (n & 31)) word &= (1u << (n & 31)) - 1u;      // the last word ends with the range
    } else {
      word = w < Wn ? row[w] : 0u;
      if (filter.bits && word) word &= filter.range_word(q, w, n);
    }
    const int pc = __popc(word);
    int incl = pc;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int x = __shfl_up(incl, d, 64);
      if (lane >= d) incl += x;
    }
    if (lane == 63) wtot[round][wave] = incl;
    __syncthreads();                                          // (the buffers alternate: one barrier per round)
    long long pos = base + incl - pc;
    int tot = 0;
    for (int i = 0; i < 16; ++i) {
      if (i < wave) pos += wtot[round][i];
      tot += wtot[round][i];
    }
    while (word) {
      const int b = __ffs(word) - 1;
      word &= word - 1;
      if (pos < cap) o[pos] = w * 32 + b + add;
      ++pos;
    }
    base += tot;
  }
  const int cnt = base < cap ? (int)base : cap;
  if (tid == 0) cnt_out[q] = cnt;
  if (fill_a)
    for (int i = cnt + tid; i < cap; i += IVF_COMPACT_THREADS) {
      fill_a[(size_t)q * cap + i] = -INFINITY;
      fill_b[(size_t)q * cap + i] = -INFINITY;
    }
}

// Workgroup r: row r of bits [rows][ld] from the indices[offsets[r] .. offsets[r + 1]) (inside [0, passages): checked on the host)
__global__ __launch_bounds__(1024) void filter_fill_kernel(const int64_t* __restrict__ offsets, const int32_t* __restrict__ indices, int exclude,
                                                           int passages, uint32_t* __restrict__ bits, long long ld) {
  uint32_t* row = bits + (size_t)blockIdx.x * ld;
  for (long long w = threadIdx.x; w < ld; w += 1024) {
    uint32_t v = 0u;
    if (exclude && w * 32 < passages) v = passages - w * 32 >= 32 ? 0xffffffffu : (1u << (passages - w * 32)) - 1u;
    row[w] = v;
  }
  __syncthreads();                                            // the row is this workgroup's alone
  for (int64_t i = offsets[blockIdx.x] + threadIdx.x; i < offsets[blockIdx.x + 1]; i += 1024) {
    const int p = indices[i];
    if (p < 0 || p >= passages) continue;
    if (exclude) atomicAnd(&row[p >> 5], ~(1u << (p & 31)));
    else atomicOr(&row[p >> 5], 1u << (p & 31));
  }
}

}  // namespace

hipError_t rr_launch_filter_fill(const int64_t* offsets, const int32_t* indices, int rows, int exclude, int passages, uint32_t* bits,
                                 long long ld, hipStream_t st) {
  if (!offsets || !indices || !bits || rows < 1 || passages < 1 || ld < ((long long)passages + 31) / 32) return hipErrorInvalidValue;
  hipLaunchKernelGGL(filter_fill_kernel, dim3((unsigned)rows), dim3(1024), 0, st, offsets, indices, exclude, passages, bits, ld);
  return hipGetLastError();
}

bool rr_filter_bits_host(const int32_t* indices, const int64_t* offsets, int rows, int exclude, int passages, uint32_t* bits, long long ld) {
  if (rows < 1 || passages < 1 || ld < ((long long)passages + 31) / 32 || offsets[0] != 0) return false;
  for (int r = 0; r < rows; ++r)
    if (offsets[r + 1] < offsets[r]) return false;
  for (int64_t i = 0; i < offsets[rows]; ++i)
    if (indices[i] < 0 || indices[i] >= passages) return false;
  for (int r = 0; r < rows; ++r) {
    uint32_t* row = bits + (size_t)r * ld;
    for (long long w = 0; w < ld; ++w) {
      uint32_t v = 0u;
      if (exclude && w * 32 < passages) v = passages - w * 32 >= 32 ? 0xffffffffu : (1u << (passages - w * 32)) - 1u;
      row[w] = v;
    }
    for (int64_t i = offsets[r]; i < offsets[r + 1]; ++i) {
      const int p = indices[i];
      if (exclude) row[p >> 5] &= ~(1u << (p & 31));
      else row[p >> 5] |= 1u << (p & 31);
    }
  }
  return true;
}

// ivf_scan_kernel for another caller (the export of a bank, bank_export.hip): the exclusive scan of counts [n] into offsets [n + 1],
// info[0] their total, info[1] the largest
hipError_t rr_launch_count_scan(const uint32_t* counts, int n, int64_t* offsets, int64_t* info, hipStream_t st) {
  if (!counts || !offsets || !info || n < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ivf_scan_kernel, dim3(1), dim3(1024), 0, st, counts, n, nullptr, offsets, info);
  return hipGetLastError();
}

void rr_ivf_free(rr_ivf* f) {
  if (f->offsets) (void)hipFree(f->offsets);
  if (f->pids) (void)hipFree(f->pids);
  *f = rr_ivf{};
}

// The inverted file over the P passages (first[i], len[i]) of a bank with codes (compressed, or fp16 rows with a centroid table: the
// view's codes, mask and n_centroids are all that is read; host table), into *out (which must be empty).  With
// `old`, a file over the first old->passages < P of them, the file is EXTENDED (rr_bank_extend_ivf): only the passages behind the
// old ones are walked, and *old is read, never written.  On a failure nothing is left allocated and *out stays empty;
// hipErrorOutOfMemory: an allocation failed.  Synchronises `st`.
hipError_t rr_ivf_build(const rr_bank_view& bank, const int64_t* first, const int32_t* len, int P, hipStream_t st, rr_ivf* out, const rr_ivf* old,
                        const char** failed_step) {
  const int C = bank.n_centroids;
  if (!bank.codes || !bank.mask || C < 1 || P < 1 || !first || !len || out->offsets || out->pids) return hipErrorInvalidValue;
  if (old && (!old->offsets || !old->pids || old->passages < 1 || old->passages >= P || old->postings < 0)) return hipErrorInvalidValue;
  const int P0 = old ? old->passages : 0, N = P - P0;         // the passages P0 .. P - 1 are walked
  const int64_t* old_offsets = old ? old->offsets : nullptr;
  const size_t Wn = ((size_t)N + 31) / 32;
  rr_bank_slot* table = nullptr;
  uint32_t* counts = nullptr;
  int64_t* info = nullptr;
  uint32_t* bm = nullptr;
  rr_ivf f{};
  hipError_t e = hipSuccess;
  const char* step = "allocating the table, the counts and the offsets";      // what a failure is booked under
  auto ok = [&](hipError_t x) {
    if (e == hipSuccess && x != hipSuccess) {
      e = x;
      if (failed_step) *failed_step = step;
    }
    return e == hipSuccess;
  };
  std::vector<rr_bank_slot> slots((size_t)N);
  for (int i = 0; i < N; ++i) slots[(size_t)i] = rr_bank_slot{first[P0 + i], len[P0 + i], 0};
  int64_t host_info[3] = {0, 0, 0};
  const unsigned mark_blocks = (unsigned)(((long long)N + 3) / 4);
  if (ok(hipMalloc((void**)&table, (size_t)N * sizeof(rr_bank_slot))) && ok(hipMalloc((void**)&counts, (size_t)C * sizeof(uint32_t))) &&
      ok(hipMalloc((void**)&info, 3 * sizeof(int64_t))) && ok(hipMalloc((void**)&f.offsets, ((size_t)C + 1) * sizeof(int64_t))) &&
      ok(hipMemcpyAsync(table, slots.data(), slots.size() * sizeof(rr_bank_slot), hipMemcpyHostToDevice, st)) &&
      ok(hipMemsetAsync(counts, 0, (size_t)C * sizeof(uint32_t), st))) {
    step = "the count and the scan";
    hipLaunchKernelGGL(ivf_mark_kernel<false>, dim3(mark_blocks), dim3(256), 0, st, bank.codes, bank.mask, table, N, P0, C, counts, nullptr, nullptr,
                       nullptr);
    hipLaunchKernelGGL(ivf_scan_kernel, dim3(1), dim3(1024), 0, st, counts, C, old_offsets, f.offsets, info);
    ok(hipGetLastError());
    ok(hipMemcpyAsync(host_info, info, (old ? 3 : 2) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    ok(hipStreamSynchronize(st));                             // `slots` and host_info are pageable memory of this call
  }
  int64_t longest_sorted = 0;                                 // the longest run the sort has to order: a list, or a tail
  if (e == hipSuccess) {
    f.passages = P;
    f.postings = host_info[0];
    f.longest = (int32_t)host_info[1];
    longest_sorted = old ? host_info[2] : host_info[1];
    if (f.postings < (old ? old->postings : 0) || f.longest < 0 || f.longest > P || longest_sorted < 0 || longest_sorted > N)
      ok(hipErrorUnknown);
  }
  const int64_t shift_blocks = old ? (old->postings + IVF_SHIFT_RUN - 1) / IVF_SHIFT_RUN : 0;
  if (e == hipSuccess && shift_blocks > 0x7fffffffLL) ok(hipErrorInvalidValue);
  step = "allocating the postings";
  if (e == hipSuccess && ok(hipMalloc((void**)&f.pids, (size_t)std::max<int64_t>(f.postings, 1) * sizeof(int32_t))) &&
      ok(hipMemsetAsync(counts, 0, (size_t)C * sizeof(uint32_t), st))) {
    step = old ? "the copy of the old postings, the fill and the sort of the tails" : "the fill and the sort";
    if (shift_blocks > 0)
      hipLaunchKernelGGL(ivf_shift_copy_kernel, dim3((unsigned)shift_blocks), dim3(IVF_SHIFT_THREADS), 0, st, old_offsets, f.offsets, C, old->pids,
                         f.pids);
    hipLaunchKernelGGL(ivf_mark_kernel<true>, dim3(mark_blocks), dim3(256), 0, st, bank.codes, bank.mask, table, N, P0, C, counts, f.offsets,
                       old_offsets, f.pids);
    hipLaunchKernelGGL(ivf_sort_kernel, dim3((unsigned)C), dim3(256), 0, st, f.offsets, old_offsets, f.pids);
    ok(hipGetLastError());
  }
  if (e == hipSuccess && longest_sorted > IVF_SORT_MAX) {     // the lists (tails) one LDS slice does not hold, one after the other
    std::vector<int64_t> off((size_t)C + 1), was(old ? (size_t)C + 1 : 0);
    int32_t* cnt_dev = (int32_t*)info;                        // the compaction's count: not needed again
    step = "the bitmap pass over the long lists";
    if (ok(hipMalloc((void**)&bm, Wn * sizeof(uint32_t))) &&
        ok(hipMemcpyAsync(off.data(), f.offsets, off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st)) &&
        (!old || ok(hipMemcpyAsync(was.data(), old_offsets, was.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st))) &&
        ok(hipStreamSynchronize(st))) {
      for (int c = 0; c < C && e == hipSuccess; ++c) {
        const int64_t start = off[(size_t)c] + (old ? was[(size_t)c + 1] - was[(size_t)c] : 0), cnt = off[(size_t)c + 1] - start;
        if (cnt <= IVF_SORT_MAX) continue;
        if (!ok(hipMemsetAsync(bm, 0, Wn * sizeof(uint32_t), st))) break;
        const unsigned blocks = (unsigned)std::min<int64_t>((cnt + 255) / 256, 4096);
        // bit i: passage P0 + i; the compaction adds P0 back
        hipLaunchKernelGGL(ivf_list_bits_kernel, dim3(blocks), dim3(256), 0, st, f.pids + start, (long long)cnt, P0, N, bm);
        hipLaunchKernelGGL(ivf_compact_kernel<words_bitmap>, dim3(1), dim3(IVF_COMPACT_THREADS), 0, st, bm, (int)Wn, f.pids + start, 0LL, (int)cnt, cnt_dev, P0,
                           nullptr, nullptr, rr_passage_filter{}, N);
        ok(hipGetLastError());
      }
    }
  }
  ok(hipStreamSynchronize(st));                               // before the scratch goes
  if (e != hipSuccess) (void)hipGetLastError();
  if (table) (void)hipFree(table);
  if (counts) (void)hipFree(counts);
  if (info) (void)hipFree(info);
  if (bm) (void)hipFree(bm);
  if (e != hipSuccess) {
    rr_ivf_free(&f);
    return e;
  }
  *out = f;
  return hipSuccess;
}

// stage 3 of rr_bank_search_plaid_ivf: cand [nq][cap] ascending range-relative candidates of every query, ccnt [nq] their numbers,
// -inf behind them in a1 / a2 [nq][cap]; bm [nq][Wn] scratch, Wn = ceil(n / 32); cells [nq][E] from stage 1
hipError_t rr_launch_ivf_candidates(const rr_ivf& f, int C, const int32_t* cells, int E, int nq, int first, int n, uint32_t* bm, int Wn,
                                    int32_t* cand, int cap, int32_t* ccnt, float* a1, float* a2, const rr_passage_filter& filter,
                                    hipStream_t st) {
  if (filter.bits && ((filter.rows != 1 && filter.rows != nq) || filter.first != first || filter.ld < ((long long)first + n + 31) / 32))
    return hipErrorInvalidValue;
  if (!f.offsets || !f.pids || !cells || !bm || !cand || !ccnt || !a1 || !a2 || C < 1 || E < 1 || nq < 1 || nq > 65535 || first < 0 || n < 1 ||
      (long long)first + n > f.passages || Wn != (n + 31) / 32 || cap < 1 || cap > n)
    return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(bm, 0, (size_t)nq * Wn * sizeof(uint32_t), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ivf_candidates_kernel, dim3((unsigned)E, (unsigned)nq), dim3(256), 0, st, cells, E, C, f.offsets, f.pids, first, n, bm, Wn);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ivf_compact_kernel<words_bitmap>, dim3((unsigned)nq), dim3(IVF_COMPACT_THREADS), 0, st, bm, Wn, cand, (long long)cap, cap, ccnt, 0, a1, a2,
                     filter, n);
  return hipGetLastError();
}

// the candidate rows of rr_bank_search_filtered_sparse: cand [filter.rows][n] gets the range-relative passages of [filter.first,
// filter.first + n) whose bit is set in filter row r, ascending, cnt [filter.rows] their numbers.  One workgroup per row, no atomics.
hipError_t rr_launch_filter_compact(const rr_passage_filter& filter, int n, int32_t* cand, int32_t* cnt, hipStream_t st) {
  if (!filter.bits || !cand || !cnt || filter.rows < 1 || filter.rows > 65535 || filter.first < 0 || n < 1 ||
      filter.ld < ((long long)filter.first + n + 31) / 32)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(ivf_compact_kernel<words_filter>, dim3((unsigned)filter.rows), dim3(IVF_COMPACT_THREADS), 0, st, nullptr, (n + 31) / 32, cand,
                     (long long)n, n, cnt, 0, nullptr, nullptr, filter, n);
  return hipGetLastError();
}

// rr_bank_load_ivf: an EMPTY *out from host arrays that rr_ivf_check_host (ivf_check.h) has passed: offsets [C + 1], pids
// [offsets[C]], over P passages, `longest` its longest list.  On a failure nothing is left allocated.  Synchronises `st`.
hipError_t rr_ivf_load(const int64_t* offsets_host, const int32_t* pids_host, int C, int P, int32_t longest, hipStream_t st, rr_ivf* out) {
  if (!offsets_host || C < 1 || P < 1 || out->offsets || out->pids || (offsets_host[C] > 0 && !pids_host)) return hipErrorInvalidValue;
  rr_ivf f{};
  f.passages = P;
  f.postings = offsets_host[C];
  f.longest = longest;
  hipError_t e = hipMalloc((void**)&f.offsets, ((size_t)C + 1) * sizeof(int64_t));
  if (e == hipSuccess) e = hipMalloc((void**)&f.pids, (size_t)std::max<int64_t>(f.postings, 1) * sizeof(int32_t));
  if (e == hipSuccess) e = hipMemcpyAsync(f.offsets, offsets_host, ((size_t)C + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && f.postings > 0) e = hipMemcpyAsync(f.pids, pids_host, (size_t)f.postings * sizeof(int32_t), hipMemcpyHostToDevice, st);
  const hipError_t es = hipStreamSynchronize(st);             // the host arrays are the caller's again
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) {
    (void)hipGetLastError();
    rr_ivf_free(&f);
    return e;
  }
  *out = f;
  return hipSuccess;
}

hipError_t rr_ivf_read(const rr_ivf& f, int C, int64_t* offsets_host, int32_t* pids_host, hipStream_t st) {
  hipError_t e = hipSuccess;
  if (offsets_host) e = hipMemcpyAsync(offsets_host, f.offsets, ((size_t)C + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && pids_host && f.postings > 0)
    e = hipMemcpyAsync(pids_host, f.pids, (size_t)f.postings * sizeof(int32_t), hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);
  return e != hipSuccess ? e : es;
}

// THE INVERTED FILE in host code (rr_util_plaid_ivf, rerank_mi355_diag.h).  Passages lie back to back in codes / mask.  offsets_out
// [C + 1] is always written; pids_out (or null) holds room for pids_capacity entries.  Returns the postings total.
int64_t rr_ivf_host(const int32_t* codes, const uint8_t* mask, const int32_t* lengths, int n, int C, int64_t* offsets_out, int32_t* pids_out,
                    int64_t pids_capacity) {
  std::vector<int64_t> count((size_t)C, 0);
  std::vector<int32_t> last((size_t)C, -1);                   // the last passage counted for a centroid: passages come in ascending order
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 1) {
      int64_t run = 0;
      for (int c = 0; c < C; ++c) {
        offsets_out[c] = run;
        run += count[(size_t)c];
        count[(size_t)c] = 0;
        last[(size_t)c] = -1;
      }
      offsets_out[C] = run;
      if (!pids_out || run > pids_capacity) return run;
    }
    size_t row = 0;
    for (int p = 0; p < n; ++p) {
      for (int r = 0; r < lengths[p]; ++r, ++row) {
        if (mask && !mask[row]) continue;
        const int c = std::min(std::max(codes[row], 0), C - 1);
        if (last[(size_t)c] == p) continue;
        last[(size_t)c] = p;
        if (pass == 1) pids_out[offsets_out[c] + count[(size_t)c]] = p;
        ++count[(size_t)c];
      }
    }
  }
  return offsets_out[C];
}
