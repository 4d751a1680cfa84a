// The merge of per-part top-k lists into one list over GLOBAL indices (rr_bank_merge_topk, "THE MERGED LIST" in
// include/rerank_mi355.h): what a bank split over ranks, or over several banks of one process, needs behind its searches.  One
// kernel, one workgroup per query.
//
// bank_merge_kernel: entry (p, e) of the P * k_in a query has is REAL iff e < clamp(counts[p][q], 0, k_in) and its local index lies
// inside part p; its key is rank_key(score, part_offsets[p] + local) (rank_order.h: the one order of the searches), every other
// entry and the padding up to n2, the next power of two (at least 2), gets key 0, which ranks behind every entry.  The keys are
// sorted in LDS by the bitonic network (written out here as in topk_select_kernel and plaid_list_select_kernel; rank_order.h says
// why it is no shared function; a thread takes a compare-exchange PAIR per step, so half the threads of the other two copies do the
// same work) and the first k leave.  No second array travels with the keys, so the 8192 entries of the largest call are exactly
// the 64 KB a workgroup has without asking for more.  What a key does not carry is found again:
//   the part     the last p with part_offsets[p] <= g, a binary search in the 65 offsets (a kernel argument by value; read with a
//                variable index straight from the argument segment: no copy, nothing staged).
//   the score    the image of a score in its key is invertible except for what the order itself merges: +0 / -0 and the NaNs.
//                Those alone are read again: the winner's part is walked for the r-th real entry with its key, r = the number of
//                equal keys in front of it in the sorted row.  Equal keys name one (part, local index), so that is the order a
//                STABLE sort of the entries in (part, entry) order gives: the host definition below is that sort.
// Nothing depends on scheduling (distinct keys have one sorted order, equal keys are interchangeable in LDS and told apart as
// above): the same bytes from run to run, no atomics of any kind.
#include <algorithm>
#include <vector>

#include "rank_order.h"
#include "rr_common.h"

namespace {

struct merge_offsets { int32_t v[RR_MERGE_MAX_PARTS + 1]; };

// the score whose image a key holds, for every image but the two that stand for more than one bit pattern (zero, NaN)
__host__ __device__ __forceinline__ bool merge_image_exact(uint32_t im) { return im != 0x80000000u && im != 0xffffffffu; }
__host__ __device__ __forceinline__ float merge_image_score(uint32_t im) {
  return __builtin_bit_cast(float, (im & 0x80000000u) ? (im & 0x7fffffffu) : ~im);
}

__global__ __launch_bounds__(1024) void bank_merge_kernel(const int32_t* __restrict__ idx_in, const float* __restrict__ sc_in,
                                                          const int32_t* __restrict__ cnt_in, long long part_stride, long long count_stride,
                                                          int P, const merge_offsets off, int k_in, int k, int n2,
                                                          int32_t* __restrict__ idx_out, float* __restrict__ sc_out,
                                                          int32_t* __restrict__ cnt_out, int32_t* __restrict__ parts_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long key[];       // [n2]; the kernel has no static LDS in front of it
  const int q = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, total = P * k_in;
  const size_t row = (size_t)q * k_in;
  for (int i = tid; i < n2; i += nt) {
    unsigned long long kv = 0ull;                             // absent entries and padding rank behind every entry
    if (i < total) {
      const int p = i / k_in, e = i - p * k_in;
      const int c = cnt_in ? min(max(cnt_in[(size_t)p * count_stride + q], 0), k_in) : k_in;
      if (e < c) {
        const int li = idx_in[(size_t)p * part_stride + row + e];
        const int o = off.v[p];
        if (li >= 0 && li < off.v[p + 1] - o) kv = rank_key(sc_in[(size_t)p * part_stride + row + e], (uint32_t)(o + li));
      }
    }
    key[i] = kv;
  }
  __syncthreads();
  for (int kk = 2; kk <= n2; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (n2 >> 1); t += nt) {
        const int i = 2 * t - (t & (j - 1)), l = i + j;       // the pair (i, i ^ j), i without bit j
        const bool up = (i & kk) == 0;                        // a run in rank order (larger key first)
        const unsigned long long a = key[i], b = key[l];
        if (up ? a < b : a > b) { key[i] = b; key[l] = a; }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < k; i += nt) {
    const unsigned long long kv = key[i];
    const size_t o = (size_t)q * k + i;
    if (kv == 0ull) {                                         // behind the count
      idx_out[o] = -1;
      if (sc_out) sc_out[o] = -INFINITY;
      if (parts_out) parts_out[o] = -1;
      if (i == 0) cnt_out[q] = 0;
      continue;
    }
    if (i + 1 == k || key[i + 1] == 0ull) cnt_out[q] = i + 1; // the last real entry that leaves
    const int g = (int)rank_key_index(kv);
    int lo = 0, hi = P - 1;                                   // the last part whose offset is <= g (empty parts share an offset)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (off.v[mid] <= g) lo = mid; else hi = mid - 1;
    }
    idx_out[o] = g;
    if (parts_out) parts_out[o] = lo;
    if (!sc_out) continue;
    const uint32_t im = (uint32_t)(kv >> 32);
    float s = merge_image_score(im);
    if (!merge_image_exact(im)) {                             // a zero or a NaN: its own bits, from its list
      int r = 0;
      while (r < i && key[i - 1 - r] == kv) ++r;
      const int li = g - off.v[lo];
      const int c = cnt_in ? min(max(cnt_in[(size_t)lo * count_stride + q], 0), k_in) : k_in;
      const size_t base = (size_t)lo * part_stride + row;
      for (int e = 0; e < c; ++e) {
        if (idx_in[base + e] != li) continue;
        const float x = sc_in[base + e];
        if (rank_score_image(x) != im) continue;
        s = x;
        if (r-- == 0) break;
      }
    }
    sc_out[o] = s;
  }
}

}  // namespace

// What rr_bank_merge_topk, rr_op_bank_merge_topk and rr_util_bank_merge_topk refuse alike, in one order, before anything is read
// beyond part_offsets or written: RR_OK, or the status and in msg (at least 160 bytes) the sentence.
int rr_merge_check(const void* indices_in, const void* scores_in, const void* counts_in, long long part_stride, long long count_stride,
                   int n_parts, const int32_t* part_offsets, int n_queries, int k_in, int k, const void* indices_out, const void* scores_out,
                   const void* counts_out, const void* parts_out, char* msg, size_t msg_len) {
  msg[0] = 0;
  if (!indices_in || !scores_in || !part_offsets || !indices_out || !counts_out) {
    snprintf(msg, msg_len, "null argument");
    return -1;                                                // RR_ERR_BAD_ARG
  }
  if ((((uintptr_t)indices_in) | ((uintptr_t)scores_in) | ((uintptr_t)counts_in) | ((uintptr_t)indices_out) | ((uintptr_t)scores_out) |
       ((uintptr_t)counts_out) | ((uintptr_t)parts_out)) & 3) {
    snprintf(msg, msg_len, "misaligned pointer (every array is 4-byte aligned)");
    return -1;
  }
  if (n_parts < 1 || n_queries < 1 || k_in < 1 || k < 1) {
    snprintf(msg, msg_len, "n_parts=%d n_queries=%d k_in=%d k=%d", n_parts, n_queries, k_in, k);
    return -2;                                                // RR_ERR_BAD_SHAPE
  }
  if (k > k_in) {
    snprintf(msg, msg_len, "k=%d above k_in=%d (the global top k lies in the union of the per-part top k_in only for k <= k_in)", k, k_in);
    return -2;
  }
  if (n_parts > RR_MERGE_MAX_PARTS) {
    snprintf(msg, msg_len, "n_parts=%d (at most %d)", n_parts, RR_MERGE_MAX_PARTS);
    return -4;                                                // RR_ERR_UNSUPPORTED
  }
  if (n_queries > 65535) {
    snprintf(msg, msg_len, "n_queries=%d (at most 65535)", n_queries);
    return -4;
  }
  if ((long long)n_parts * k_in > RR_MERGE_MAX_ENTRIES) {
    snprintf(msg, msg_len, "n_parts * k_in = %lld entries per query (at most %d: the keys of a query are sorted in 64 KB of LDS)",
             (long long)n_parts * k_in, RR_MERGE_MAX_ENTRIES);
    return -4;
  }
  if (part_stride < (long long)n_queries * k_in || (counts_in && count_stride < n_queries)) {
    snprintf(msg, msg_len, "part_stride=%lld (at least n_queries * k_in = %lld) count_stride=%lld (at least n_queries = %d)", part_stride,
             (long long)n_queries * k_in, count_stride, n_queries);
    return -2;
  }
  if (part_offsets[0] < 0) {
    snprintf(msg, msg_len, "part_offsets[0]=%d", part_offsets[0]);
    return -2;
  }
  for (int p = 0; p < n_parts; ++p)
    if (part_offsets[p + 1] < part_offsets[p]) {
      snprintf(msg, msg_len, "part_offsets descend at part %d (%d, then %d)", p, part_offsets[p], part_offsets[p + 1]);
      return -2;
    }
  return 0;
}

// one launch over arguments rr_merge_check has passed
hipError_t rr_launch_bank_merge(const int32_t* indices_in, const float* scores_in, const int32_t* counts_in, long long part_stride,
                                long long count_stride, int n_parts, const int32_t* part_offsets_host, int n_queries, int k_in, int k,
                                int32_t* indices_out, float* scores_out, int32_t* counts_out, int32_t* parts_out, hipStream_t st) {
  if (n_parts < 1 || n_parts > RR_MERGE_MAX_PARTS || n_queries < 1 || n_queries > 65535 || k < 1 || k > k_in ||
      (long long)n_parts * k_in > RR_MERGE_MAX_ENTRIES)
    return hipErrorInvalidValue;
  merge_offsets off;
  for (int p = 0; p <= RR_MERGE_MAX_PARTS; ++p) off.v[p] = part_offsets_host[std::min(p, n_parts)];
  int n2 = 2;
  while (n2 < n_parts * k_in) n2 <<= 1;
  const int threads = std::min(1024, std::max(64, n2 / 2));
  hipLaunchKernelGGL(bank_merge_kernel, dim3((unsigned)n_queries), dim3((unsigned)threads), (size_t)n2 * sizeof(unsigned long long), st,
                     indices_in, scores_in, counts_in, part_stride, count_stride, n_parts, off, k_in, k, n2, indices_out, scores_out,
                     counts_out, parts_out);
  return hipGetLastError();
}

// THE MERGED LIST in host code (rr_util_bank_merge_topk) over arguments rr_merge_check has passed: the real entries of a query in
// (part, entry) order, sorted STABLY by key, larger first
void rr_bank_merge_host(const int32_t* indices_in, const float* scores_in, const int32_t* counts_in, long long part_stride,
                        long long count_stride, int n_parts, const int32_t* part_offsets, int n_queries, int k_in, int k,
                        int32_t* indices_out, float* scores_out, int32_t* counts_out, int32_t* parts_out) {
  struct entry { unsigned long long key; float score; int32_t part; };
  std::vector<entry> es;
  es.reserve((size_t)n_parts * k_in);
  for (int q = 0; q < n_queries; ++q) {
    es.clear();
    for (int p = 0; p < n_parts; ++p) {
      const int c = counts_in ? std::min(std::max(counts_in[(size_t)p * count_stride + q], 0), k_in) : k_in;
      const long long size = (long long)part_offsets[p + 1] - part_offsets[p];
      for (int e = 0; e < c; ++e) {
        const size_t at = (size_t)p * part_stride + (size_t)q * k_in + e;
        const int32_t li = indices_in[at];
        if (li < 0 || li >= size) continue;
        es.push_back(entry{rank_key(scores_in[at], (uint32_t)(part_offsets[p] + li)), scores_in[at], p});
      }
    }
    std::stable_sort(es.begin(), es.end(), [](const entry& a, const entry& b) { return a.key > b.key; });
    const int keep = (int)std::min<size_t>((size_t)k, es.size());
    for (int i = 0; i < k; ++i) {
      const size_t o = (size_t)q * k + i;
      indices_out[o] = i < keep ? (int32_t)rank_key_index(es[(size_t)i].key) : -1;
      if (scores_out) scores_out[o] = i < keep ? es[(size_t)i].score : -INFINITY;
      if (parts_out) parts_out[o] = i < keep ? es[(size_t)i].part : -1;
    }
    counts_out[q] = keep;
  }
}
