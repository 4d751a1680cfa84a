// Training of a PLAID codec on the device (rr_plaid_kmeans, rr_plaid_residuals; include/rerank_mi355.h, THE TRAINED CENTROIDS): what
// the reference's indexer does with faiss k-means and _compute_avg_residual
// (third_party/ColBERT/colbert/indexing/collection_indexer.py:211-319, 452-465): Lloyd's iteration with L2 distance from given
// initial rows, and the residuals of held-out rows against the finished table, from which the caller takes the bucket quantiles.
// FIVE KERNELS:
//   compress_assign_kernel<.., BIAS>  (plaid_assign.h) the assignment: the matrix-core kernel of rr_bank_add_compress with the bias
//                             h[c] = -|T[c]|^2 / 2 added to every score, so that the largest key is the nearest centroid in L2.
//                             Its splits, its key scratch and rr_plaid_compress_plan are those of a compression.
//   train_accumulate_kernel   the maximum over the splits' keys, code[r] written and compared with the previous iteration's, then
//                             fix(x) = clamp(x, -256, 256) * 2^24 added into A[code][e] with 64-bit integer vector atomics and 1
//                             into n[code] with a 32-bit one.  Every fp16 value is a multiple of 2^-24, so fix is exact, and
//                             integer addition has one result in any order: the sums do not depend on scheduling.  A wave
//                             instruction covers 64 consecutive elements of one row (512 contiguous bytes of A; at D < 64 the 64 / D
//                             rows of a pass side by side).
//   train_update_kernel       one lane group (D / 8 lanes) per centroid, the shape of compress_residual_kernel: the mean
//                             fp16(float(double(A) / double(n 2^24))), or for an empty cluster the row rho(seed, iteration, c) of
//                             the source (a splitmix64 step the cluster computes by itself); the new T row, h[c], the count, the
//                             re-seed count; A and n zeroed for the next iteration.  INIT: the same kernel writes the initial
//                             table from init_rows.
//   train_finalise_kernel     T[c] / max(|T[c]|, 1e-12) -> fp16: plaid_finish8, the norm of THE DECODED ROW.
//   train_residual_kernel     rr_plaid_residuals: code and float32 residual of every row against a finished table (THE COMPRESSED
//                             ROW steps 1 - 4 without the buckets), behind the plain assignment.
// Nothing synchronises between the iterations: every kernel reads what the one before it on the stream wrote.
// rr_plaid_kmeans_host is the definition in host code (rr_util_plaid_kmeans), the one the device is held to bit for bit.
// Measured on one MI355X (profiles/plaid_train_bench.json.log, tools/bench_plaid_train.py): 262 144 fp16 rows, D 128, 4 096 centroids:
// 3.07 ms per iteration on the device, of which the assignment takes 2.58 ms (106.7 TFLOP/s of the 155 the f32 matrix core gives; the
// same kernel without bias reaches 101.9 under rr_bank_add_compress), the accumulation 0.37 ms and the update 0.12 ms: accumulation and
// update are 0.16 of an iteration.  The accumulation adds 268 MB through 64-bit integer atomics in that time: 721 GB/s of added bytes
// with 512 contiguous bytes per wave instruction, the first measurement of that rate here.  The same iteration composed from torch
// (float32 matmul in chunks, argmax, index_add_) takes 4.69 ms: the library's takes 0.65 of it.
#include <algorithm>
#include <cmath>
#include <vector>

#include "plaid_assign.h"
#include "plaid_decode.h"

namespace {

constexpr int ACC_PASSES = 4;          // row passes of a wave of the accumulate kernel

// rr_set_tuning("kmeans_stop_after"): 2: all; 0: an iteration ends behind the assignment, 1: behind the accumulation (timing by
// difference; the outputs are then meaningless)
std::atomic<int> g_kmeans_stop_after{2};

// fix(v) of the definition; v holds an fp16 value
__host__ __device__ __forceinline__ long long train_fix(float v) {
  if (v != v) return 0;
  const float c = v < -256.f ? -256.f : (v > 256.f ? 256.f : v);
  return (long long)(c * 16777216.f);                      // exact: a multiple of 2^-24 of magnitude <= 2^8
}

// the re-seed row of cluster c in iteration i (splitmix64 over seed ^ (i << 32 | c))
__host__ __device__ __forceinline__ unsigned long long train_reseed_row(unsigned long long seed, int iter, int c, unsigned long long R) {
  unsigned long long z = seed ^ (((unsigned long long)(uint32_t)iter << 32) | (unsigned long long)(uint32_t)c);
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z % R;
}

__device__ __forceinline__ void round8_f16(float (&v)[8]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float2 f = unpack2<1>(pack2h(v[2 * k], v[2 * k + 1]));
    v[2 * k] = f.x; v[2 * k + 1] = f.y;
  }
}

template <bool SRC_F16>
__global__ __launch_bounds__(256) void train_accumulate_kernel(const void* __restrict__ src, long long R, int D, int C,
                                                               const unsigned long long* __restrict__ keys, int splits,
                                                               int32_t* __restrict__ codes, unsigned long long* __restrict__ A,
                                                               uint32_t* __restrict__ n, uint32_t* __restrict__ stats) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int epl = D < 64 ? D : 64;                         // elements of one row in a wave instruction
  const int rpp = 64 / epl;                                // rows of a pass
  const int sub = lane / epl, e0 = lane - sub * epl;
  const long long r_base = ((long long)blockIdx.x * 4 + wave) * (ACC_PASSES * rpp);
  uint32_t changed = 0;
  for (int p = 0; p < ACC_PASSES; ++p) {                   // wave-uniform: every lane reaches the ballot
    const long long r = r_base + (long long)p * rpp + sub;
    bool ch = false;
    if (r < R) {
      unsigned long long key = 0ull;
      for (int s = 0; s < splits; ++s) key = key_max(key, keys[(size_t)s * (size_t)R + (size_t)r]);
      const int code = (int)min(rank_key_index(key), (uint32_t)(C - 1));      // every split holds a centroid: the key is an entry's
      if (e0 == 0) {
        ch = codes[r] != code;
        codes[r] = code;
        atomicAdd(n + code, 1u);
      }
      unsigned long long* arow = A + (size_t)code * D;
      for (int e = e0; e < D; e += 64) {
        float v;
        if constexpr (SRC_F16) v = unpack2<1>((uint32_t)((const uint16_t*)src)[(size_t)r * D + e]).x;
        else v = unpack2<1>(pack2h(((const float*)src)[(size_t)r * D + e], 0.f)).x;
        atomicAdd(arow + e, (unsigned long long)train_fix(v));
      }
    }
    changed += (uint32_t)__popcll(__ballot(ch));
  }
  if (lane == 0 && changed) atomicAdd(stats, changed);
}

// one lane group (lpr = D / 8 lanes, a power of two) per centroid
template <bool SRC_F16, bool INIT>
__global__ __launch_bounds__(256) void train_update_kernel(const void* __restrict__ src, long long R, int D, int lpr, int rpw, int C,
                                                           const int32_t* __restrict__ init_rows, unsigned long long seed, int iter,
                                                           unsigned long long* __restrict__ A, uint32_t* __restrict__ n,
                                                           uint16_t* __restrict__ T, float* __restrict__ h,
                                                           int32_t* __restrict__ counts, uint32_t* __restrict__ stats) {
  const int lane = threadIdx.x & 63, sub = lane / lpr, c8 = lane - sub * lpr;
  const long long c = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * rpw + sub;
  const bool live = sub < rpw && c < C;
  float s[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = 0.f;
  if (live) {
    const uint32_t cnt = INIT ? 0u : n[c];
    unsigned long long* arow = A + (size_t)c * D + 8 * c8;
    if (INIT || cnt == 0u) {
      const long long rho = INIT ? (long long)init_rows[c] : (long long)train_reseed_row(seed, iter, (int)c, (unsigned long long)R);
      load8<SRC_F16>((const char*)src + (size_t)rho * D * (SRC_F16 ? 2 : 4), c8, s);
      if constexpr (!SRC_F16) round8_f16(s);
    } else {
      const double den = (double)((unsigned long long)cnt << 24);
#pragma unroll
      for (int k = 0; k < 8; ++k) s[k] = (float)__ddiv_rn((double)(long long)arow[k], den);
      round8_f16(s);
    }
    ((uint4*)(T + (size_t)c * D))[c8] = make_uint4(pack2h(s[0], s[1]), pack2h(s[2], s[3]), pack2h(s[4], s[5]), pack2h(s[6], s[7]));
#pragma unroll
    for (int k = 0; k < 4; ++k) ((ulonglong2*)arow)[k] = make_ulonglong2(0ull, 0ull);
    if (c8 == 0) {
      n[c] = 0u;
      if (!INIT) {
        if (counts) counts[c] = (int32_t)cnt;
        if (cnt == 0u) atomicAdd(stats + 1, 1u);
      }
    }
  }
  float q = plaid_sumsq8(s);                               // all 64 lanes: the butterfly is cross-lane
  for (int o = 1; o < lpr; o <<= 1) q += __shfl_xor(q, o, 64);
  if (live && c8 == 0) h[c] = -0.5f * q;
}

__global__ __launch_bounds__(256) void train_finalise_kernel(const uint16_t* __restrict__ T, int C, int D, int lpr, int rpw,
                                                             uint16_t* __restrict__ out) {
  const int lane = threadIdx.x & 63, sub = lane / lpr, c8 = lane - sub * lpr;
  const long long c = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * rpw + sub;
  const bool live = sub < rpw && c < C;
  float s[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = 0.f;
  if (live) load8<true>(T + (size_t)c * D, c8, s);
  plaid_finish8(s, lpr);                                   // all 64 lanes
  if (live)
    ((uint4*)(out + (size_t)c * D))[c8] = make_uint4(pack2h(s[0], s[1]), pack2h(s[2], s[3]), pack2h(s[4], s[5]), pack2h(s[6], s[7]));
}

// one lane group per row: the code and the float32 residual against that centroid row
template <bool SRC_F16>
__global__ __launch_bounds__(256) void train_residual_kernel(const void* __restrict__ src, long long R, int D, int lpr, int rpw,
                                                             const uint16_t* __restrict__ centroids, int C,
                                                             const unsigned long long* __restrict__ keys, int splits,
                                                             int32_t* __restrict__ codes, float* __restrict__ resid) {
  const int lane = threadIdx.x & 63, sub = lane / lpr, c8 = lane - sub * lpr;
  if (sub >= rpw) return;
  const long long r = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * rpw + sub;
  if (r >= R) return;
  unsigned long long key = 0ull;
  for (int s = 0; s < splits; ++s) key = key_max(key, keys[(size_t)s * (size_t)R + (size_t)r]);
  const int code = (int)min(rank_key_index(key), (uint32_t)(C - 1));
  float v[8], cv[8];
  load8<SRC_F16>((const char*)src + (size_t)r * D * (SRC_F16 ? 2 : 4), c8, v);
  if constexpr (!SRC_F16) round8_f16(v);
  load8<true>(centroids + (size_t)code * D, c8, cv);
  float4* out = (float4*)(resid + (size_t)r * D) + 2 * c8;
  out[0] = make_float4(v[0] - cv[0], v[1] - cv[1], v[2] - cv[2], v[3] - cv[3]);
  out[1] = make_float4(v[4] - cv[4], v[5] - cv[5], v[6] - cv[6], v[7] - cv[7]);
  if (c8 == 0) codes[r] = code;
}

inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// blocks of a kernel with one lane group per item
inline bool group_grid(long long items, int D, int* lpr, int* rpw, unsigned* blocks) {
  *lpr = D / 8;
  *rpw = 64 / *lpr;
  const long long b = (items + 4LL * *rpw - 1) / (4LL * *rpw);
  if (b <= 0 || b > 0x7fffffffLL) return false;
  *blocks = (unsigned)b;
  return true;
}

}  // namespace

int rr_set_kmeans_stop_after(int stage) {
  if (stage < 0 || stage > 2) return -1;
  g_kmeans_stop_after.store(stage, std::memory_order_relaxed);
  return 0;
}

// what the training kernels take: D a power of two in [16, 512] (the matrix-core step, and the pairwise tree of the norm)
bool rr_plaid_train_shape_ok(int D) { return D >= 16 && D <= 512 && (D & (D - 1)) == 0; }

// where the intermediates of a training call lie in its scratch; assign.jt == 0: a shape the kernels do not take
rr_kmeans_plan rr_plaid_kmeans_plan(long long R, int C, int D, int niters) {
  rr_kmeans_plan pl{};
  if (!rr_plaid_train_shape_ok(D) || niters < 0) return pl;
  pl.assign = rr_plaid_compress_plan(R, C, D);
  if (pl.assign.jt == 0) return pl;
  const size_t Cp = ((size_t)C + 15) & ~(size_t)15;
  size_t off = 0;
  pl.init_off = off;  off = up16(off + (size_t)C * sizeof(int32_t));
  pl.T_off = off;     off = up16(off + (size_t)C * D * sizeof(uint16_t));
  pl.h_off = off;     off = up16(off + Cp * sizeof(float));
  pl.A_off = off;     off = up16(off + (size_t)C * D * sizeof(unsigned long long));
  pl.n_off = off;     off = up16(off + (size_t)C * sizeof(uint32_t));
  pl.codes_off = off; off = up16(off + (size_t)R * sizeof(int32_t));
  pl.stats_off = off; off = up16(off + ((size_t)niters + 1) * 2 * sizeof(uint32_t));
  pl.keys_off = off;  off = up16(off + (size_t)pl.assign.splits * (size_t)R * sizeof(unsigned long long));
  pl.total = off;
  return pl;
}

// THE TRAINED CENTROIDS over device rows; init_rows lie at scratch + pl.init_off already.  Everything is enqueued on st, nothing
// synchronises.  counts_out / stats_out may be null.
hipError_t rr_launch_plaid_kmeans(const void* rows, int rows_f16, long long R, int D, int C, int niters, unsigned long long seed,
                                  char* scratch, const rr_kmeans_plan& pl, uint16_t* centroids_out, int32_t* counts_out,
                                  int32_t* stats_out, hipStream_t st) {
  if (!rows || !scratch || !centroids_out || pl.assign.jt == 0 || !rr_plaid_train_shape_ok(D) || R <= 0 || R > (1LL << 30) || C <= 0 ||
      C > R || niters < 0)
    return hipErrorInvalidValue;
  if (((((uintptr_t)rows) | ((uintptr_t)scratch) | ((uintptr_t)centroids_out)) & 15) || (((uintptr_t)counts_out) & 3) ||
      (((uintptr_t)stats_out) & 3))
    return hipErrorInvalidValue;
  const int32_t* init_rows = (const int32_t*)(scratch + pl.init_off);
  uint16_t* T = (uint16_t*)(scratch + pl.T_off);
  float* h = (float*)(scratch + pl.h_off);
  unsigned long long* A = (unsigned long long*)(scratch + pl.A_off);
  uint32_t* n = (uint32_t*)(scratch + pl.n_off);
  int32_t* codes = (int32_t*)(scratch + pl.codes_off);
  uint32_t* stats = stats_out ? (uint32_t*)stats_out : (uint32_t*)(scratch + pl.stats_off);
  unsigned long long* keys = (unsigned long long*)(scratch + pl.keys_off);
  int lpr = 0, rpw = 0;
  unsigned cblocks = 0;
  if (!group_grid(C, D, &lpr, &rpw, &cblocks)) return hipErrorInvalidValue;
  const int epl = D < 64 ? D : 64, rows_per_block = 4 * ACC_PASSES * (64 / epl);
  const long long ablocks = (R + rows_per_block - 1) / rows_per_block;
  if (ablocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(codes, 0xff, (size_t)R * sizeof(int32_t), st);       // no row has code -1: iteration 0 changes all R
  if (e == hipSuccess && niters) e = hipMemsetAsync(stats, 0, (size_t)niters * 2 * sizeof(uint32_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(h, 0, (size_t)(pl.A_off - pl.h_off), st);
  if (e == hipSuccess && counts_out && niters == 0) e = hipMemsetAsync(counts_out, 0, (size_t)C * sizeof(int32_t), st);
  if (e != hipSuccess) return e;
  auto update = [&](auto f16, auto init, int iter) {
    hipLaunchKernelGGL((train_update_kernel<decltype(f16)::value, decltype(init)::value>), dim3(cblocks), dim3(256), 0, st, rows, R, D, lpr,
                       rpw, C, init_rows, seed, iter, A, n, T, h, counts_out, stats + 2 * (size_t)std::max(iter, 0));
  };
  using yes = std::true_type;
  using no = std::false_type;
  if (rows_f16) update(yes{}, yes{}, -1);
  else update(no{}, yes{}, -1);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const int stop = g_kmeans_stop_after.load(std::memory_order_relaxed);
  for (int i = 0; i < niters; ++i) {
    e = rows_f16 ? assign_pick<true, true>(rows, nullptr, R, D, T, C, pl.assign, keys, h, st)
                 : assign_pick<false, true>(rows, nullptr, R, D, T, C, pl.assign, keys, h, st);
    if (e != hipSuccess) return e;
    if (stop < 1) continue;
    if (rows_f16)
      hipLaunchKernelGGL(train_accumulate_kernel<true>, dim3((unsigned)ablocks), dim3(256), 0, st, rows, R, D, C, keys, pl.assign.splits, codes,
                         A, n, stats + 2 * (size_t)i);
    else
      hipLaunchKernelGGL(train_accumulate_kernel<false>, dim3((unsigned)ablocks), dim3(256), 0, st, rows, R, D, C, keys, pl.assign.splits, codes,
                         A, n, stats + 2 * (size_t)i);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (stop < 2) continue;
    if (rows_f16) update(yes{}, no{}, i);
    else update(no{}, no{}, i);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(train_finalise_kernel, dim3(cblocks), dim3(256), 0, st, T, C, D, lpr, rpw, centroids_out);
  return hipGetLastError();
}

// codes and float32 residuals of R device rows against a finished table; scratch holds pl.total bytes (the splits' keys at
// pl.keys_off)
hipError_t rr_launch_plaid_residuals(const void* rows, int rows_f16, long long R, int D, const uint16_t* centroids, int C, char* scratch,
                                     const rr_compress_plan& pl, int32_t* codes_out, float* resid_out, hipStream_t st) {
  if (!rows || !centroids || !scratch || !codes_out || !resid_out || pl.jt == 0 || !rr_plaid_train_shape_ok(D) || R <= 0 || C <= 0)
    return hipErrorInvalidValue;
  if (((((uintptr_t)rows) | ((uintptr_t)centroids) | ((uintptr_t)scratch) | ((uintptr_t)resid_out)) & 15) || (((uintptr_t)codes_out) & 3))
    return hipErrorInvalidValue;
  unsigned long long* keys = (unsigned long long*)(scratch + pl.keys_off);
  hipError_t e = rows_f16 ? assign_pick<true, false>(rows, nullptr, R, D, centroids, C, pl, keys, nullptr, st)
                          : assign_pick<false, false>(rows, nullptr, R, D, centroids, C, pl, keys, nullptr, st);
  if (e != hipSuccess) return e;
  int lpr = 0, rpw = 0;
  unsigned blocks = 0;
  if (!group_grid(R, D, &lpr, &rpw, &blocks)) return hipErrorInvalidValue;
  if (rows_f16)
    hipLaunchKernelGGL(train_residual_kernel<true>, dim3(blocks), dim3(256), 0, st, rows, R, D, lpr, rpw, centroids, C, keys, pl.splits,
                       codes_out, resid_out);
  else
    hipLaunchKernelGGL(train_residual_kernel<false>, dim3(blocks), dim3(256), 0, st, rows, R, D, lpr, rpw, centroids, C, keys, pl.splits,
                       codes_out, resid_out);
  return hipGetLastError();
}

// rr_util_plaid_kmeans: THE TRAINED CENTROIDS (include/rerank_mi355.h) in host code.  Host memory throughout; false for a shape or
// an argument the definition does not take (the caller has checked init_rows).
bool rr_plaid_kmeans_host(const void* rows, int rows_f16, long long R, int D, const int32_t* init_rows, int C, int niters,
                          unsigned long long seed, uint16_t* centroids_out, int32_t* counts_out, int32_t* stats_out) {
  if (!rr_plaid_train_shape_ok(D) || R <= 0 || R > (1LL << 30) || C <= 0 || C > R || niters < 0) return false;
  const size_t Ds = (size_t)D;
  std::vector<uint16_t> xb((size_t)R * Ds), Tb((size_t)C * Ds);
  std::vector<float> x((size_t)R * Ds), T((size_t)C * Ds), h((size_t)C);
  for (size_t i = 0; i < x.size(); ++i) {
    xb[i] = rows_f16 ? ((const uint16_t*)rows)[i] : plaid_f16_bits(((const float*)rows)[i]);
    x[i] = plaid_f16_value(xb[i]);
  }
  // the sum of squares of a table row in the order of THE DECODED ROW's norm
  auto sumsq = [&](const float* row) {
    float q[64];
    const int lpr = D / 8;
    for (int c8 = 0; c8 < lpr; ++c8) {
      float s[8];
      for (int k = 0; k < 8; ++k) s[k] = row[8 * c8 + k];
      q[c8] = plaid_sumsq8(s);
    }
    for (int w = lpr; w > 1; w >>= 1)
      for (int i = 0; i < w / 2; ++i) q[i] = q[2 * i] + q[2 * i + 1];
    return q[0];
  };
  auto set_row = [&](int c, long long r) {
    for (size_t e = 0; e < Ds; ++e) {
      Tb[(size_t)c * Ds + e] = xb[(size_t)r * Ds + e];
      T[(size_t)c * Ds + e] = x[(size_t)r * Ds + e];
    }
  };
  for (int c = 0; c < C; ++c) {
    if (init_rows[c] < 0 || init_rows[c] >= R) return false;
    set_row(c, init_rows[c]);
    h[(size_t)c] = -0.5f * sumsq(T.data() + (size_t)c * Ds);
  }
  std::vector<int32_t> codes((size_t)R, -1);
  std::vector<long long> A((size_t)C * Ds);
  std::vector<uint32_t> n((size_t)C, 0u);
  for (int it = 0; it < niters; ++it) {
    std::fill(A.begin(), A.end(), 0LL);
    std::fill(n.begin(), n.end(), 0u);
    int32_t changed = 0, reseeded = 0;
    for (long long r = 0; r < R; ++r) {
      const float* xr = x.data() + (size_t)r * Ds;
      unsigned long long best = 0;
      for (int c = 0; c < C; ++c) {
        const float* a = T.data() + (size_t)c * Ds;
        float acc = 0.f;
        for (int t = 0; t < D; t += 16)
          for (int e = 0; e < 4; ++e)
            for (int g = 0; g < 4; ++g) acc = fmaf(a[t + 4 * g + e], xr[t + 4 * g + e], acc);
        const float biased = acc + h[(size_t)c];
        const unsigned long long key = rank_key(biased, (uint32_t)c);
        if (key > best) best = key;
      }
      const int code = (int)rank_key_index(best);
      changed += codes[(size_t)r] != code;
      codes[(size_t)r] = code;
      ++n[(size_t)code];
      for (size_t e = 0; e < Ds; ++e) A[(size_t)code * Ds + e] += train_fix(xr[e]);
    }
    for (int c = 0; c < C; ++c) {
      if (n[(size_t)c] == 0u) {
        set_row(c, (long long)train_reseed_row(seed, it, c, (unsigned long long)R));
        ++reseeded;
      } else {
        const double den = (double)((unsigned long long)n[(size_t)c] << 24);
        for (size_t e = 0; e < Ds; ++e) {
          const uint16_t b = plaid_f16_bits((float)((double)A[(size_t)c * Ds + e] / den));
          Tb[(size_t)c * Ds + e] = b;
          T[(size_t)c * Ds + e] = plaid_f16_value(b);
        }
      }
    }
    for (int c = 0; c < C; ++c) h[(size_t)c] = -0.5f * sumsq(T.data() + (size_t)c * Ds);
    if (stats_out) { stats_out[2 * it] = changed; stats_out[2 * it + 1] = reseeded; }
  }
  for (int c = 0; c < C; ++c) {
    const float* row = T.data() + (size_t)c * Ds;
    const float d = plaid_scale(sqrtf(sumsq(row)));
    for (size_t e = 0; e < Ds; ++e) centroids_out[(size_t)c * Ds + e] = plaid_f16_bits(row[e] / d);
    if (counts_out) counts_out[c] = (int32_t)n[(size_t)c];
  }
  return true;
}
