// Compression of embeddings into the rows of a compressed passage bank (rr_bank_add_compress, rr_op_plaid_compress_rows;
// include/rerank_mi355.h): what the reference's ResidualCodec.compress does on its CPU branch
// (third_party/ColBERT/colbert/indexing/codecs/residual.py:169-221), without the [centroids x rows] matrix it materialises.
//   code     = the centroid c with the largest rank_key(S[c], c) (rank_order.h: NaN first, then the highest score, equal scores by
//              the LOWEST index), S[c] the float32 fmaf chain of li_scores.hip for the context row float32(centroid c) against the
//              query column x = float32(fp16_rne(row)): one v_mfma_f32_16x16x4_f32 after another, d = 16 t + 4 g + e, t and e
//              ascending in time, g inside the instruction.  Bit for bit the scores_out entry of rr_op_li_scores for that pair.
//   residual = x_e - float32(centroid[code][e]), one float32 subtraction; bucket_e = the number of cutoffs strictly below it (a NaN
//              residual: 0); the bucket's nbits bits are written least significant first into a bit stream that fills bytes from
//              the most significant end (np.packbits): the inverse of THE DECODED ROW's unpacking (passage_bank.hip).
// THREE KERNELS per call:
//   compress_map_kernel       bank calls only: the call's kept rows are rows 0 .. len - 1 of every passage of the padded source
//                             [n][Lc][D]; destination row i (0 .. R - 1, the bank row first_row + i) reads map[i] = p * Lc + j.
//                             Written from the staged rr_bank_slot entries, 8 bytes per kept row, so that the two kernels below
//                             see a dense list of rows whatever the passages' lengths.
//   compress_assign_kernel    (a) plaid_assign.h, shared with the codec training of plaid_train.hip (which runs it with a per-centroid
//                             bias; here BIAS is false): a workgroup of 4 waves stages a block of 16 JT rows in LDS, its waves walk
//                             the 16-row tiles of the fp16 centroid table on the matrix core and keep a running best 64-bit rank
//                             key per row; grid.y splits the centroid range in chunks of `chunk` centroids
//                             (rr_set_tuning("compress_chunk")), split s writes its best key per row to keys[s][row].  A maximum
//                             over keys has one possible result, so the code does not depend on how the range is split over waves
//                             or workgroups, and nothing is atomic.
//   compress_residual_kernel  (b) a row kernel of passage_bank.hip's shape (a lane moves 8 elements, D / 8 lanes per row): the
//                             maximum over the splits' keys, the int32 code, the residual against that centroid row, the bucket by
//                             a branch-free binary search over the cutoffs in LDS (at most 255, non-decreasing: the count of
//                             cutoffs below r), nbits packed bytes per lane and the mask byte.  Plain vector stores only.
//   compress_codes_kernel     the codes-only ending that takes (b)'s place for an fp16 bank with a centroid table
//                             (rr_launch_plaid_assign_codes: rr_bank_set_centroids, rr_bank_add): the maximum over the splits' keys
//                             and the int32 code, 4 bytes written per row; (a) then reads the bank's fp16 rows where they lie, no map.
// Traffic of (a): C * D * 2 bytes of centroids per row block (from L2 after the first), 8 bytes written per row and split.
// Measured on one MI355X (profiles/bank_compress_bench.json.log, tools/bench_bank_compress.py): 512 passages padded to 180 rows,
// 61 250 kept rows, D 128, nbits 8, 65 536 centroids: rr_bank_add_compress 10.2 ms per call with its synchronisation, 10.12 ms on
// the device, of which the row map and (a) take 10.09 ms: 101.9 TFLOP/s of the 155 the f32 matrix core gives (li_scores_kernel
// reaches 54: it writes its score block and runs one workgroup per pair; here a workgroup of the 479 x 2 grid walks 32 768
// centroids behind one staging of its rows).  The path composed from torch on the same tensors (float32 matmul in chunks with
// .max(0), bucketize, bit packing, rr_bank_add_plaid through the host) takes 14.85 ms: the fused call takes 0.69 of it.  The two
// paths' codes and bytes agreed on all 7 670 rows compared.
#include <algorithm>

#include "plaid_assign.h"  // compress_assign_kernel, assign_pick, key_max; li_sources.h (load8, pack2h, li_pick_jt), rank_order.h
#include "rr_common.h"

namespace {

// destination row -> source row of the padded input, from the staged slots: one thread per source position (p, j)
__global__ __launch_bounds__(256) void compress_map_kernel(const rr_bank_slot* __restrict__ slots, long long n_src, int Lc,
                                                           long long base, long long* __restrict__ map) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_src) return;
  const long long p = r / Lc;
  const int j = (int)(r - p * Lc);
  const rr_bank_slot s = slots[p];
  if (j < s.len) map[s.first_row - base + j] = r;
}

// one lane group (lpr = D / 8 lanes) per row of the call; outputs are indexed by the call's row (the caller passes the bank's
// stores at its first destination row)
template <int NBITS, bool SRC_F16>
__global__ __launch_bounds__(256) void compress_residual_kernel(const void* __restrict__ src, const long long* __restrict__ map,
                                                                const float* __restrict__ mask, long long R, int D, int lpr, int rpw,
                                                                const uint16_t* __restrict__ centroids, int C,
                                                                const float* __restrict__ cutoffs,
                                                                const unsigned long long* __restrict__ keys, int splits,
                                                                int32_t* __restrict__ codes, uint8_t* __restrict__ resid,
                                                                uint8_t* __restrict__ mask_bytes) {
  constexpr int NC = (1 << NBITS) - 1;
  __shared__ float cut[256];
  if (threadIdx.x < NC) cut[threadIdx.x] = cutoffs[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63, sub = lane / lpr, c8 = lane - sub * lpr;
  if (sub >= rpw) return;
  const long long r = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * rpw + sub;
  if (r >= R) return;
  unsigned long long key = 0ull;
  for (int s = 0; s < splits; ++s) key = key_max(key, keys[(size_t)s * (size_t)R + (size_t)r]);
  const int code = (int)min(rank_key_index(key), (uint32_t)(C - 1));      // every split holds a centroid: the key is an entry's
  const long long s = map ? map[r] : r;
  float v[8], cv[8];
  load8<SRC_F16>((const char*)src + (size_t)s * D * (SRC_F16 ? 2 : 4), c8, v);
  if constexpr (!SRC_F16) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float2 f = unpack2<1>(pack2h(v[2 * k], v[2 * k + 1]));
      v[2 * k] = f.x; v[2 * k + 1] = f.y;
    }
  }
  load8<true>(centroids + (size_t)code * D, c8, cv);
  uint32_t out[NBITS];
#pragma unroll
  for (int b = 0; b < NBITS; ++b) out[b] = 0u;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float res = v[k] - cv[k];
    uint32_t bucket = 0;                                   // the cutoffs strictly below res; every compare with a NaN is false
#pragma unroll
    for (int step = 1 << (NBITS - 1); step; step >>= 1)
      if (cut[bucket + step - 1] < res) bucket += step;
#pragma unroll
    for (int j = 0; j < NBITS; ++j) {
      const int p = k * NBITS + j;                         // position in the lane's bit stream: bit j of the bucket, bit 0 first
      out[p >> 3] |= ((bucket >> j) & 1u) << (7 - (p & 7));
    }
  }
  uint8_t* rp = resid + (size_t)r * ((size_t)D / 8 * NBITS) + (size_t)c8 * NBITS;
  if constexpr (NBITS == 1) {
    rp[0] = (uint8_t)out[0];
  } else if constexpr (NBITS == 2) {
    *(uint16_t*)rp = (uint16_t)(out[0] | (out[1] << 8));
  } else if constexpr (NBITS == 4) {
    *(uint32_t*)rp = out[0] | (out[1] << 8) | (out[2] << 16) | (out[3] << 24);
  } else {
    *(uint2*)rp = make_uint2(out[0] | (out[1] << 8) | (out[2] << 16) | (out[3] << 24),
                             out[4] | (out[5] << 8) | (out[6] << 16) | (out[7] << 24));
  }
  if (c8 == 0) {
    codes[r] = code;
    if (mask_bytes) mask_bytes[r] = mask[s] != 0.f ? 1 : 0;
  }
}

// the codes-only ending of the assignment (rr_launch_plaid_assign_codes): one thread per row, the maximum over the splits' keys as
// compress_residual_kernel takes it, the int32 code, nothing else read or written
__global__ __launch_bounds__(256) void compress_codes_kernel(const unsigned long long* __restrict__ keys, int splits, long long R, int C,
                                                             int32_t* __restrict__ codes) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  unsigned long long key = 0ull;
  for (int s = 0; s < splits; ++s) key = key_max(key, keys[(size_t)s * (size_t)R + (size_t)r]);
  codes[r] = (int)min(rank_key_index(key), (uint32_t)(C - 1));
}

// rr_set_tuning("compress_chunk"): the centroids of one split of the assignment kernel; 0: chosen by the launch (below)
std::atomic<int> g_compress_chunk{0};
// rr_set_tuning("compress_stop_after"): 0: a call ends behind the assignment kernel (timing by difference; nothing is output)
std::atomic<int> g_compress_stop_after{1};

}  // namespace

int rr_set_compress_chunk(int centroids) {
  if (centroids != 0 && (centroids < 16 || centroids > (1 << 24) || centroids % 16)) return -1;
  g_compress_chunk.store(centroids, std::memory_order_relaxed);
  return 0;
}

int rr_set_compress_stop_after(int stage) {
  if (stage < 0 || stage > 1) return -1;
  g_compress_stop_after.store(stage, std::memory_order_relaxed);
  return 0;
}

// what a compression takes: nbits in {1, 2, 4, 8}, D a multiple of 16 (the matrix-core step) in [16, 512] and of 8 * nbits
bool rr_plaid_compress_shape_ok(int nbits, int D) {
  if (nbits != 1 && nbits != 2 && nbits != 4 && nbits != 8) return false;
  return D >= 16 && D <= 512 && D % 16 == 0 && D % (8 * nbits) == 0;
}

// The launch shape of R rows against C centroids and where the intermediates lie in the call's scratch.  Column block: li_pick_jt
// under the 72 KB that keep two workgroups on a CU.  Splits: with `compress_chunk` unset, as many as bring the grid to about four
// workgroups per CU (1024), each at least 256 centroids (four tiles per wave) and at most 64 of them; jt == 0: a shape the kernels
// do not take.
rr_compress_plan rr_plaid_compress_plan(long long R, int C, int D) {
  rr_compress_plan pl{};
  if (R <= 0 || C <= 0 || C > (1 << 24) || D < 16 || D > 512 || D % 16) return pl;
  size_t lds = 0;
  const int jt = li_pick_jt(R > 64 ? 128 : (int)R, D, 0, (size_t)72 * 1024, &lds);
  const long long row_blocks = (R + 16 * jt - 1) / (16 * jt);
  if (jt == 0 || row_blocks > 0x7fffffffLL) return pl;
  int chunk = g_compress_chunk.load(std::memory_order_relaxed);
  if (chunk == 0) {
    const long long want = std::max(1LL, std::min(64LL, 1024 / row_blocks));
    const long long per = std::max(256LL, ((long long)C + want - 1) / want);
    chunk = (int)((per + 15) / 16 * 16);
  }
  const long long splits = ((long long)C + chunk - 1) / chunk;
  if (splits > 65535) return pl;                           // grid.y
  pl.jt = jt;
  pl.row_blocks = (int)row_blocks;
  pl.splits = (int)splits;
  pl.chunk = chunk;
  pl.lds = lds;
  pl.map_off = 0;
  pl.keys_off = ((size_t)R * sizeof(long long) + 15) & ~(size_t)15;
  pl.total = pl.keys_off + (size_t)splits * (size_t)R * sizeof(unsigned long long);
  return pl;
}

// The kernels over R rows.  in.slots != null: a bank call, the rows are the kept rows of the padded source `in` (rr_common.h; `base`
// the first destination row of the call), mask_bytes written; in.slots == null: in.src holds the R rows back to back, no mask.
// codes / resid / mask_bytes point at the call's first row.
hipError_t rr_launch_plaid_compress(const rr_padded_rows& in, long long base, long long R, int D, int nbits, const uint16_t* centroids, int C,
                                    const float* cutoffs, char* scratch, const rr_compress_plan& pl, int32_t* codes, uint8_t* resid,
                                    uint8_t* mask_bytes, hipStream_t st) {
  const void* src = in.src;
  if (!src || !centroids || !cutoffs || !scratch || !codes || !resid || R <= 0 || pl.jt == 0 || !rr_plaid_compress_shape_ok(nbits, D) ||
      C <= 0)
    return hipErrorInvalidValue;
  if (in.slots && (!in.mask || !mask_bytes || in.n <= 0 || in.Lc <= 0)) return hipErrorInvalidValue;
  // 16-byte row chunks of the source and the centroids, 8-byte keys and residual stores
  if (((((uintptr_t)src) | ((uintptr_t)centroids) | ((uintptr_t)scratch)) & 15) || (((uintptr_t)resid) & 7) || (((uintptr_t)codes) & 3))
    return hipErrorInvalidValue;
  long long* map = in.slots ? (long long*)(scratch + pl.map_off) : nullptr;
  unsigned long long* keys = (unsigned long long*)(scratch + pl.keys_off);
  if (in.slots) {
    const long long n_src = (long long)in.n * in.Lc, blocks = (n_src + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(compress_map_kernel, dim3((unsigned)blocks), dim3(256), 0, st, in.slots, n_src, in.Lc, base, map);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipError_t e = in.src_f16 ? assign_pick<true, false>(src, map, R, D, centroids, C, pl, keys, nullptr, st)
                            : assign_pick<false, false>(src, map, R, D, centroids, C, pl, keys, nullptr, st);
  if (e != hipSuccess) return e;
  if (g_compress_stop_after.load(std::memory_order_relaxed) == 0) return hipSuccess;
  const int lpr = D / 8, rpw = 64 / lpr;
  const long long per_block = 4LL * rpw, blocks = (R + per_block - 1) / per_block;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  plaid_with_nbits(nbits, [&](auto nb) {
    constexpr int NB = decltype(nb)::value;
    if (in.src_f16)
      hipLaunchKernelGGL((compress_residual_kernel<NB, true>), dim3((unsigned)blocks), dim3(256), 0, st, src, map, in.mask, R, D, lpr, rpw,
                         centroids, C, cutoffs, keys, pl.splits, codes, resid, mask_bytes);
    else
      hipLaunchKernelGGL((compress_residual_kernel<NB, false>), dim3((unsigned)blocks), dim3(256), 0, st, src, map, in.mask, R, D, lpr, rpw,
                         centroids, C, cutoffs, keys, pl.splits, codes, resid, mask_bytes);
  });
  return hipGetLastError();
}

// The codes of R fp16 rows that lie back to back (an fp16 bank with a centroid table): compress_assign_kernel as above, without a
// row map, then compress_codes_kernel.  The keys are the only intermediate: 8 bytes per row and split.
hipError_t rr_launch_plaid_assign_codes(const uint16_t* rows_f16, long long R, int D, const uint16_t* centroids, int C, char* scratch,
                                        const rr_compress_plan& pl, int32_t* codes, hipStream_t st) {
  if (!rows_f16 || !centroids || !scratch || !codes || R <= 0 || pl.jt == 0 || D < 16 || D > 512 || D % 16 || C <= 0)
    return hipErrorInvalidValue;
  if (((((uintptr_t)rows_f16) | ((uintptr_t)centroids)) & 7) || (((uintptr_t)scratch) & 15) || (((uintptr_t)codes) & 3)) return hipErrorInvalidValue;
  unsigned long long* keys = (unsigned long long*)(scratch + pl.keys_off);
  const hipError_t e = assign_pick<true, false>(rows_f16, nullptr, R, D, centroids, C, pl, keys, nullptr, st);
  if (e != hipSuccess) return e;
  const long long blocks = (R + 255) / 256;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(compress_codes_kernel, dim3((unsigned)blocks), dim3(256), 0, st, keys, pl.splits, R, C, codes);
  return hipGetLastError();
}
