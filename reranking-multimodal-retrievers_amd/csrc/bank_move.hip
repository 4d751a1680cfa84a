// The row compaction behind rr_bank_remove (include/rerank_mi355.h, "REMOVING PASSAGES"): the rows of the surviving passages moved
// down in place so that they lie back to back again, every per-row array of the bank alike (fp16 rows, or codes and residual bytes;
// mask bytes).
//
// THE PLAN (rr_bank_remove_plan; rr_util_bank_remove_plan is the same function over caller arrays).  From the lengths and the
// removed indices the host derives the RUNS, maximal blocks of consecutive surviving rows behind the first removed passage, each
// (src_row, dst_row, rows) with dst_row < src_row; the shift src_row - dst_row never decreases from one run to the next.  The
// passages in front of the first removed one do not move and are no run.  One parallel launch that moved every run in place would
// be wrong: the destination of run j overlaps the tail of run j - 1 that another workgroup has not read yet.  Nothing here waits
// for another workgroup.  The order comes from the stream instead: the destination rows are cut into WINDOWS of window_rows rows
// from the first moved row on; the runs are cut at the window borders into MOVES (window, src_row, dst_row, rows).  Per window one
// launch gathers the window's rows from their sources into a staging block, and one contiguous device-to-device copy puts the block
// at the destination.  Every source row of window w + 1 lies at or behind its own destination, which lies behind the end of window
// w: what a window overwrites, no later window reads.
//
// THE GATHER (bank_move_gather_kernel<E>).  A workgroup owns a tile of consecutive destination rows of the window (about 32 KB).
// It finds the move its first row lies in by binary search over dst_row in the window's part of the move table (on the device,
// uploaded once per call; block-uniform arguments, so the loads are scalar), then walks the moves of its tile.  A piece, the rows
// of one move inside the tile, is one contiguous byte range on both sides: rows * rb bytes, all offsets 64-bit.  E = min(rb, 16)
// is the element both sides are always aligned to (rb a power of two, or a multiple of 16).  At E = 16 every access is 16 bytes.
// Below it (codes: 4 bytes a row; mask: 1; residual rows under 16 bytes) the staging side starts where the window does and the
// source side where the shift puts it, so the two are aligned alike only modulo w = the lowest set bit of their distance: the
// piece is copied in E-byte elements up to the first w-aligned byte, in w-byte accesses (up to 16) from there, and the rest in
// E-byte elements again.  Plain vector loads and stores, no LDS, no atomics.
// No row-copy helper of passage_bank.hip / bank_export.hip fits: the ingest and gather kernels convert as they copy, the export's
// walks one passage per wave under its mask.
#include <algorithm>
#include <atomic>
#include <vector>

#include "rank_order.h"
#include "rr_common.h"

// ---- the plan (host)
int rr_bank_remove_plan(const int32_t* lengths, int n, const int32_t* remove, int m, int64_t window_rows, std::vector<int32_t>* new_index,
                        std::vector<rr_bank_move>* moves, int32_t* bad_index) {
  if (bad_index) *bad_index = -1;
  if (n < 0 || m < 0 || window_rows < 1) return RR_REMOVE_PLAN_BAD_SHAPE;
  std::vector<uint8_t> gone((size_t)n, 0);
  for (int i = 0; i < m; ++i) {
    const int32_t p = remove[i];
    if (p < 0 || p >= n) {
      if (bad_index) *bad_index = p;
      return RR_REMOVE_PLAN_OUTSIDE;
    }
    if (gone[(size_t)p]) {
      if (bad_index) *bad_index = p;
      return RR_REMOVE_PLAN_TWICE;
    }
    gone[(size_t)p] = 1;
  }
  for (int p = 0; p < n; ++p)
    if (lengths[p] < 1) {
      if (bad_index) *bad_index = p;
      return RR_REMOVE_PLAN_BAD_SHAPE;
    }
  new_index->assign((size_t)n, -1);
  moves->clear();
  // the runs, cut at the window borders as they grow: `open` is the move the next surviving passage may extend
  int64_t src = 0, dst = 0, base = -1;
  int32_t next = 0;
  bool moved = false, open = false;
  for (int p = 0; p < n; ++p) {
    const int64_t len = lengths[p];
    if (gone[(size_t)p]) {
      src += len;
      moved = true;
      open = false;                                 // a gap in the sources ends the run
      continue;
    }
    (*new_index)[(size_t)p] = next++;
    if (moved) {
      if (base < 0) base = dst;
      int64_t s = src, d = dst, left = len;
      while (left > 0) {
        const int64_t w = (d - base) / window_rows;
        const int64_t take = std::min(left, base + (w + 1) * window_rows - d);
        if (open && moves->back().window == w)
          moves->back().rows += take;
        else
          moves->push_back(rr_bank_move{w, s, d, take});
        open = true;
        s += take;
        d += take;
        left -= take;
      }
    }
    src += len;
    dst += len;
  }
  return 0;
}

// ---- the gather
namespace {

template <int U> struct move_unit;
template <> struct move_unit<1> { typedef uint8_t type; };
template <> struct move_unit<2> { typedef uint16_t type; };
template <> struct move_unit<4> { typedef uint32_t type; };
template <> struct move_unit<8> { typedef uint2 type; };
template <> struct move_unit<16> { typedef uint4 type; };

// n units of U bytes from s to d, both U-aligned, by the 256 threads of the workgroup
template <int U>
__device__ __forceinline__ void copy_units(const uint8_t* __restrict__ s, uint8_t* __restrict__ d, long long n, int tid) {
  typedef typename move_unit<U>::type unit_t;
  const unit_t* __restrict__ su = (const unit_t*)s;
  unit_t* __restrict__ du = (unit_t*)d;
#pragma unroll 4
  for (long long i = tid; i < n; i += 256) du[i] = su[i];
}

// one piece: `bytes` (a multiple of E) from s to d, both E-aligned; block-uniform arguments
template <int E>
__device__ __forceinline__ void move_piece(const uint8_t* __restrict__ s, uint8_t* __restrict__ d, long long bytes, int tid) {
  if constexpr (E == 16) {
    copy_units<16>(s, d, bytes >> 4, tid);
  } else {
    const unsigned rel = ((unsigned)(uintptr_t)s - (unsigned)(uintptr_t)d) & 15u;
    const int w = rel ? (int)(rel & (0u - rel)) : 16;         // the widest access at which both sides are aligned at the same bytes
    if (w <= E) {
      copy_units<E>(s, d, bytes / E, tid);
      return;
    }
    long long head = (long long)((w - (int)((uintptr_t)s & (uintptr_t)(w - 1))) & (w - 1));
    if (head > bytes) head = bytes;
    const long long body = (bytes - head) & ~(long long)(w - 1);
    copy_units<E>(s, d, head / E, tid);
    const uint8_t* sb = s + head;
    uint8_t* db = d + head;
    if (E < 2 && w == 2) copy_units<2>(sb, db, body >> 1, tid);
    else if (E < 4 && w == 4) copy_units<4>(sb, db, body >> 2, tid);
    else if (E < 8 && w == 8) copy_units<8>(sb, db, body >> 3, tid);
    else copy_units<16>(sb, db, body >> 4, tid);
    copy_units<E>(sb + body, db + body, (bytes - head - body) / E, tid);
  }
}

template <int E>
__global__ __launch_bounds__(256) void bank_move_gather_kernel(const rr_bank_move* __restrict__ moves, int n_moves, long long win_dst_row,
                                                               long long win_rows, int tile_rows, const uint8_t* __restrict__ src,
                                                               uint8_t* __restrict__ staging, int rb) {
  const int tid = threadIdx.x;
  const long long t0 = win_dst_row + (long long)blockIdx.x * tile_rows;
  const long long win_end = win_dst_row + win_rows;
  if (t0 >= win_end) return;                                  // the whole workgroup
  const long long t1 = t0 + tile_rows < win_end ? t0 + tile_rows : win_end;
  // the last move whose dst_row is at or below t0 (moves[0].dst_row == win_dst_row <= t0)
  int lo = 0, hi = n_moves - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (uniform_i64(moves[mid].dst_row) <= t0) lo = mid;
    else hi = mid - 1;
  }
  int j = lo;
  long long r = t0;
  while (r < t1 && j < n_moves) {
    const long long m_src = uniform_i64(moves[j].src_row), m_dst = uniform_i64(moves[j].dst_row), m_rows = uniform_i64(moves[j].rows);
    const long long off = r - m_dst;
    if (off < 0 || off >= m_rows) break;                       // a table that does not cover the window: nothing is read past it
    const long long cnt = m_rows - off < t1 - r ? m_rows - off : t1 - r;
    move_piece<E>(src + (m_src + off) * rb, staging + (r - win_dst_row) * rb, cnt * rb, tid);
    r += cnt;
    ++j;
  }
}

// rr_set_tuning("bank_move_kb"): the KiB of rr_bank_remove's staging block
std::atomic<int> g_bank_move_kb{RR_BANK_MOVE_KB_DEFAULT};

}  // namespace

int rr_set_bank_move_kb(int kb) {
  if (kb < 4 || kb > (1 << 20)) return -1;
  g_bank_move_kb.store(kb, std::memory_order_relaxed);
  return 0;
}
size_t rr_bank_move_staging_bytes() { return (size_t)g_bank_move_kb.load(std::memory_order_relaxed) * 1024; }

bool rr_bank_move_row_bytes_ok(int rb) { return rb >= 1 && rb <= 1024 && ((rb & (rb - 1)) == 0 || rb % 16 == 0); }

hipError_t rr_launch_bank_move_gather(const rr_bank_move* moves_dev, int n_moves, long long win_dst_row, long long win_rows, const void* src,
                                      void* staging, int rb, hipStream_t st) {
  if (!moves_dev || !src || !staging || n_moves < 1 || win_dst_row < 0 || win_rows < 1 || !rr_bank_move_row_bytes_ok(rb)) return hipErrorInvalidValue;
  const int e = rb < 16 ? rb : 16;
  if ((((uintptr_t)src) | ((uintptr_t)staging)) & 15) return hipErrorInvalidValue;
  const int tile_rows = std::max(1, 32768 / rb);
  const long long tiles = (win_rows + tile_rows - 1) / tile_rows;
  if (tiles > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)tiles), block(256);
  const uint8_t* s = (const uint8_t*)src;
  uint8_t* d = (uint8_t*)staging;
  switch (e) {
    case 1: hipLaunchKernelGGL(bank_move_gather_kernel<1>, grid, block, 0, st, moves_dev, n_moves, win_dst_row, win_rows, tile_rows, s, d, rb); break;
    case 2: hipLaunchKernelGGL(bank_move_gather_kernel<2>, grid, block, 0, st, moves_dev, n_moves, win_dst_row, win_rows, tile_rows, s, d, rb); break;
    case 4: hipLaunchKernelGGL(bank_move_gather_kernel<4>, grid, block, 0, st, moves_dev, n_moves, win_dst_row, win_rows, tile_rows, s, d, rb); break;
    case 8: hipLaunchKernelGGL(bank_move_gather_kernel<8>, grid, block, 0, st, moves_dev, n_moves, win_dst_row, win_rows, tile_rows, s, d, rb); break;
    default: hipLaunchKernelGGL(bank_move_gather_kernel<16>, grid, block, 0, st, moves_dev, n_moves, win_dst_row, win_rows, tile_rows, s, d, rb); break;
  }
  return hipGetLastError();
}

// The moves of a plan carried out on every array of `arrays` (base pointer 16-byte aligned, rb bytes a row): window by window, per
// array one gather into `staging` (room for the longest window's rows of the widest array) and one copy to the destination.
// moves_dev: the same table on the device.  Everything is enqueued on st; nothing synchronises.
hipError_t rr_bank_move_run(const rr_bank_move* moves_host, size_t n_moves, const rr_bank_move* moves_dev, const rr_move_array* arrays,
                            int n_arrays, void* staging, hipStream_t st) {
  size_t i0 = 0;
  while (i0 < n_moves) {
    size_t i1 = i0;
    long long rows = 0;
    while (i1 < n_moves && moves_host[i1].window == moves_host[i0].window) rows += moves_host[i1++].rows;
    const long long dst_row = moves_host[i0].dst_row;
    for (int a = 0; a < n_arrays; ++a) {
      const size_t rb = (size_t)arrays[a].rb;
      hipError_t e = rr_launch_bank_move_gather(moves_dev + i0, (int)(i1 - i0), dst_row, rows, arrays[a].base, staging, arrays[a].rb, st);
      if (e != hipSuccess) return e;
      e = hipMemcpyAsync((uint8_t*)arrays[a].base + (size_t)dst_row * rb, staging, (size_t)rows * rb, hipMemcpyDeviceToDevice, st);
      if (e != hipSuccess) return e;
    }
    i0 = i1;
  }
  return hipSuccess;
}
