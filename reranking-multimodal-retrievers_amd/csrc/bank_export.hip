// The export of a compressed passage bank as a PLAID index stores it (rr_bank_export_plaid, include/rerank_mi355.h; the diagnostic
// twin rr_op_bank_export_plaid, rerank_mi355_diag.h): the UNMASKED rows of the passages table[0 .. n), in table order and row order,
// back to back: a code and rb = D * nbits / 8 residual bytes per row, what the reference's indexer keeps for a passage after it has
// dropped the skiplist tokens (third_party/ColBERT/colbert/indexing/index_saver.py:70-90).  Three kernels, no atomics, nothing
// depends on scheduling:
//   (a) export_count_kernel: a WAVE per passage reads 64 mask bytes a step; ballot and popcount give the passage's doclen.
//   (b) the exclusive scan of the doclens into int64 row offsets [n + 1] and their total: ivf_scan_kernel (bank_ivf.hip,
//       rr_launch_count_scan), the scan the inverted file's counts go through.
//   (c) export_move_kernel<W>: a WAVE per passage walks it 64 rows a step.  The ballot of the step's mask bytes gives every kept row
//       its rank among the step's kept rows; destination row = passage offset + rows kept in earlier steps + rank.  The lane that
//       owns a kept row writes its code.  The residual bytes of the step's kept rows form ONE contiguous destination run of
//       kept * rb bytes.  W = 16 (rb a multiple of 16): the run is cut into 16-byte units, lane l takes the units l, l + 64, ...;
//       unit u belongs to kept row u / (rb / 16), whose source row is the position of that set bit of the ballot (nth_set_bit:
//       five popcounts, no LDS), so a wave stores 1 KiB of consecutive bytes per access and loads runs of rb bytes.  W = 1, 2, 4, 8
//       (rb = W): the owning lane moves its row in one access.  A step with no kept row loads nothing but its mask bytes.
// All row and byte offsets are 64-bit.  rr_export_plaid is the driver under both entries (a save-time call: it allocates its
// doclens / offsets block, reads the row total back and synchronises).
#include <cstring>
#include <vector>

#include "rank_order.h"
#include "rr_common.h"

namespace {

// the position of the j-th (from 0) set bit of m; j < popcount(m)
__device__ __forceinline__ int nth_set_bit(unsigned long long m, int j) {
  uint32_t w = (uint32_t)m;
  int pos = 0;
  const int c_lo = __popc(w);
  if (j >= c_lo) {
    j -= c_lo;
    w = (uint32_t)(m >> 32);
    pos = 32;
  }
#pragma unroll
  for (int s = 16; s >= 1; s >>= 1) {
    const uint32_t part = w & ((1u << s) - 1u);
    const int c = __popc(part);
    if (j >= c) {
      j -= c;
      w >>= s;
      pos += s;
    } else {
      w = part;
    }
  }
  return pos;
}

__global__ __launch_bounds__(256) void export_count_kernel(const rr_bank_slot* __restrict__ table, int n, const uint8_t* __restrict__ mask,
                                                           int32_t* __restrict__ doclens) {
  const int lane = threadIdx.x & 63;
  const long long pl = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pl >= n) return;                                        // the whole wave
  const int p = __builtin_amdgcn_readfirstlane((int)pl);
  const rr_bank_slot sl = table[p];
  const long long first_row = uniform_i64(sl.first_row);
  const int len = __builtin_amdgcn_readfirstlane(sl.len);
  int kept = 0;
  for (int base = 0; base < len; base += 64) {
    const int r = base + lane;
    const bool keep = r < len && mask[first_row + r] != 0;
    kept += __popcll(__ballot(keep));
  }
  if (lane == 0) doclens[p] = kept;
}

template <int W> struct export_unit;
template <> struct export_unit<1> { typedef uint8_t type; };
template <> struct export_unit<2> { typedef uint16_t type; };
template <> struct export_unit<4> { typedef uint32_t type; };
template <> struct export_unit<8> { typedef uint2 type; };
template <> struct export_unit<16> { typedef uint4 type; };

template <int W>
__global__ __launch_bounds__(256) void export_move_kernel(const rr_bank_slot* __restrict__ table, int n, const uint8_t* __restrict__ mask,
                                                          const int32_t* __restrict__ codes, const uint8_t* __restrict__ resid, int rb,
                                                          const int64_t* __restrict__ offsets, int32_t* __restrict__ codes_out,
                                                          uint8_t* __restrict__ resid_out) {
  typedef typename export_unit<W>::type unit_t;
  const int lane = threadIdx.x & 63;
  const long long pl = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pl >= n) return;                                        // the whole wave
  const int p = __builtin_amdgcn_readfirstlane((int)pl);
  const rr_bank_slot sl = table[p];
  const long long first_row = uniform_i64(sl.first_row);
  const int len = __builtin_amdgcn_readfirstlane(sl.len);
  long long dst_row = uniform_i64(offsets[p]);                // the passage's first destination row, then that of the step
  for (int base = 0; base < len; base += 64) {
    const int r = base + lane;
    const bool keep = r < len && mask[first_row + r] != 0;
    const unsigned long long kept_bits = __ballot(keep);
    const int kept = __popcll(kept_bits);
    if (kept == 0) continue;                                  // (wave-uniform) nothing of this step is read but its mask bytes
    const long long src_row = first_row + base;               // of lane 0
    const int rank = __popcll(kept_bits & ((1ull << lane) - 1ull));
    if (keep) codes_out[dst_row + rank] = codes[src_row + lane];
    if constexpr (W == 16) {
      const int upr = rb >> 4;                                // units per row: a power of two
      const int sh = __ffs(upr) - 1;
      const int units = kept << sh;
      const unit_t* __restrict__ src = (const unit_t*)(resid + src_row * rb);
      unit_t* __restrict__ dst = (unit_t*)(resid_out + dst_row * rb);
#pragma unroll 4
      for (int u = lane; u < units; u += 64) {
        const int s = nth_set_bit(kept_bits, u >> sh);
        dst[u] = src[((long long)s << sh) + (u & (upr - 1))];
      }
    } else {
      if (keep) ((unit_t*)resid_out)[dst_row + rank] = ((const unit_t*)resid)[src_row + lane];
    }
    dst_row += kept;
  }
}

// doclens [n] of the passages table[0 .. n) (device)
hipError_t launch_export_count(const rr_bank_slot* table, int n, const uint8_t* mask, int32_t* doclens, hipStream_t st) {
  if (!table || !mask || !doclens || n < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(export_count_kernel, dim3((unsigned)(((long long)n + 3) / 4)), dim3(256), 0, st, table, n, mask, doclens);
  return hipGetLastError();
}

// the kept rows of table[0 .. n) to codes_out / resid_out from the row offsets [n] of the scan (device)
hipError_t launch_export_move(const rr_bank_slot* table, int n, const uint8_t* mask, const int32_t* codes, const uint8_t* resid, int rb,
                                 const int64_t* offsets, int32_t* codes_out, uint8_t* resid_out, hipStream_t st) {
  if (!table || !mask || !codes || !resid || !offsets || !codes_out || !resid_out || n < 1 || !rr_export_row_bytes_ok(rb))
    return hipErrorInvalidValue;
  const int w = rb < 16 ? rb : 16;
  if ((((uintptr_t)resid) | ((uintptr_t)resid_out)) & (uintptr_t)(w - 1)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(((long long)n + 3) / 4)), block(256);
  switch (w) {
    case 1: hipLaunchKernelGGL(export_move_kernel<1>, grid, block, 0, st, table, n, mask, codes, resid, rb, offsets, codes_out, resid_out); break;
    case 2: hipLaunchKernelGGL(export_move_kernel<2>, grid, block, 0, st, table, n, mask, codes, resid, rb, offsets, codes_out, resid_out); break;
    case 4: hipLaunchKernelGGL(export_move_kernel<4>, grid, block, 0, st, table, n, mask, codes, resid, rb, offsets, codes_out, resid_out); break;
    case 8: hipLaunchKernelGGL(export_move_kernel<8>, grid, block, 0, st, table, n, mask, codes, resid, rb, offsets, codes_out, resid_out); break;
    default: hipLaunchKernelGGL(export_move_kernel<16>, grid, block, 0, st, table, n, mask, codes, resid, rb, offsets, codes_out, resid_out); break;
  }
  return hipGetLastError();
}

}  // namespace

bool rr_export_row_bytes_ok(int rb) { return rb >= 1 && rb <= 512 && (rb & (rb - 1)) == 0; }

// Count, scan, read the total back, and move when there is somewhere to move to.  *rows_out = R whenever hipSuccess is returned.
// codes_out / resid_out both null: a sizing call.  Both given and capacity_rows < R: NOTHING is written (no doclens, no offsets, no
// row) and hipSuccess is returned: the caller compares *rows_out with its capacity.  doclens_host / doclens_dev / offsets_dev: each
// optional; offsets_dev int64 [n + 1].  Synchronises st.
hipError_t rr_export_plaid(const rr_bank_slot* table, int n, const uint8_t* mask, const int32_t* codes, const uint8_t* resid, int rb,
                           int32_t* doclens_host, int32_t* doclens_dev, int64_t* offsets_dev, int32_t* codes_out, uint8_t* resid_out,
                           int64_t capacity_rows, int64_t* rows_out, hipStream_t st) {
  if (!table || !mask || !rows_out || n < 1 || (codes_out == nullptr) != (resid_out == nullptr)) return hipErrorInvalidValue;
  // one block: offsets int64 [n + 1], info int64 [2], doclens int32 [n]
  const size_t off_bytes = ((size_t)n + 1) * sizeof(int64_t), info_bytes = 2 * sizeof(int64_t), len_bytes = (size_t)n * sizeof(int32_t);
  char* blk = nullptr;
  hipError_t e = hipMalloc((void**)&blk, off_bytes + info_bytes + len_bytes);
  if (e != hipSuccess) return e;
  int64_t* offsets = (int64_t*)blk;
  int64_t* info = (int64_t*)(blk + off_bytes);
  int32_t* doclens = (int32_t*)(blk + off_bytes + info_bytes);
  auto ok = [&](hipError_t x) { if (e == hipSuccess && x != hipSuccess) e = x; return e == hipSuccess; };
  int64_t host_info[2] = {0, 0};
  std::vector<int32_t> lens;
  if (doclens_host) lens.resize((size_t)n);
  if (ok(launch_export_count(table, n, mask, doclens, st)) && ok(rr_launch_count_scan((const uint32_t*)doclens, n, offsets, info, st)) &&
      ok(hipMemcpyAsync(host_info, info, sizeof host_info, hipMemcpyDeviceToHost, st)) &&
      (!doclens_host || ok(hipMemcpyAsync(lens.data(), doclens, len_bytes, hipMemcpyDeviceToHost, st))))
    ok(hipStreamSynchronize(st));
  const int64_t R = host_info[0];
  if (e == hipSuccess && R < 0) e = hipErrorUnknown;
  const bool fits = !codes_out || capacity_rows >= R;
  if (e == hipSuccess && fits) {
    if (doclens_dev) ok(hipMemcpyAsync(doclens_dev, doclens, len_bytes, hipMemcpyDeviceToDevice, st));
    if (offsets_dev) ok(hipMemcpyAsync(offsets_dev, offsets, off_bytes, hipMemcpyDeviceToDevice, st));
    if (codes_out && R > 0) ok(launch_export_move(table, n, mask, codes, resid, rb, offsets, codes_out, resid_out, st));
  }
  const hipError_t es = hipStreamSynchronize(st);             // before the block goes
  ok(es);
  if (e != hipSuccess) (void)hipGetLastError();
  (void)hipFree(blk);
  if (e != hipSuccess) return e;
  if (fits && doclens_host) memcpy(doclens_host, lens.data(), len_bytes);
  *rows_out = R;
  return hipSuccess;
}
