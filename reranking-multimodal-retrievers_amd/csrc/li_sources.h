// The bank-side operand sources of the late-interaction score kernels, shared by li_scores.hip (one workgroup per pair,
// rr_bank_li_scores) and bank_search.hip (one wave per passage, rr_bank_search and stage 6 of rr_bank_search_plaid): where the
// four floats a lane feeds to one v_mfma_f32_16x16x4_f32 step come from.  One definition, so that both kernels run the same
// instruction sequence on the same float32 values (li_scores.hip's header comment describes the sources).  The rest of what the two kernels share lives here too:
//   li_with_bank_source an rr_bank_view as the source a kernel template takes (li_src_f16 or li_src_plaid<NBITS>), with the checks
//                       of each kind: the one place the launchers (rr_launch_bank_li_scores, rr_launch_bank_search_scores and
//                       its _listed form) decide between fp16 and compressed;
//   li_lds_attr / li_pick_jt   the launch rule: the dynamic-LDS attribute once per device, the width of the column block.
// The tile step of the two kernels is NOT here: moved into one __forceinline__ function it changed the instruction stream of every
// instantiation of both kernels (same registers, LDS and instruction counts within 3, another schedule), so each body keeps its copy.
#pragma once
#include <atomic>

#include "plaid_decode.h"      // plaid_load8 / plaid_finish8, pack2h, plaid_with_nbits, plaid_tables_ok
#include "rr_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr float LI_MASKED = -9999.0f;
constexpr int LI_TILE_PAD = 8;           // fp16 values behind a row of a decoded tile (li_src_plaid)

__device__ __forceinline__ float nan_max(float m, float v) { return (v > m || v != v) ? v : m; }

// four fp16 values (8 bytes, global or LDS) as the float32 operand of one step
__device__ __forceinline__ f32x4 half4(const uint16_t* p) {
  const uint2 u = *(const uint2*)p;
  const float2 a = unpack2<1>(u.x), b = unpack2<1>(u.y);
  return f32x4{a.x, a.y, b.x, b.y};
}

// open(p, D): pair p of the pair list; of(first_row, len, query, out): the same for a passage named by its table entry.  row(pr,
// c, g, ..): the cursor of lane (li, g) on context row c (a row the pair holds), at(cur, d) its four floats of step d; keep(pr,
// row): the mask.
struct li_src_f16 {
  const rr_bank_pair* pairs;
  const int32_t* slot;               // the output row of workgroup p, or null: p itself
  const uint16_t* rows;
  const uint8_t* mask_bytes;
  static constexpr bool TILE = false;
  struct pair_t { const uint16_t* rows; const uint8_t* mask; int len, query, out; };
  typedef const uint16_t* cursor;
  __device__ __forceinline__ pair_t of(long long first_row, int len, int query, int out, int D) const {
    return pair_t{rows + (size_t)first_row * D, mask_bytes + first_row, len, query, out};
  }
  __device__ __forceinline__ pair_t open(int p, int D) const {
    const rr_bank_pair d = pairs[p];
    return of(d.first_row, d.len, d.query, slot ? slot[p] : p, D);
  }
  __device__ __forceinline__ cursor row(const pair_t& pr, int c, int g, int D, int li, const uint16_t*) const {
    return pr.rows + (size_t)c * D + 4 * g;
  }
  static __device__ __forceinline__ f32x4 at(cursor cur, int d) { return half4(cur + d); }
  __device__ __forceinline__ bool keep(const pair_t& pr, int row) const { return pr.mask[row] != 0; }
};

template <int NBITS>
struct li_src_plaid {
  const rr_bank_pair* pairs;
  const int32_t* slot;
  const int32_t* codes;
  const uint8_t* resid;
  const uint16_t* centroids;
  const float* weights;
  int C;
  const uint8_t* mask_bytes;
  static constexpr bool TILE = true;
  struct pair_t { long long first_row; const uint8_t* mask; int len, query, out; };
  typedef const uint16_t* cursor;
  __device__ __forceinline__ pair_t of(long long first_row, int len, int query, int out, int) const {
    return pair_t{first_row, mask_bytes + first_row, len, query, out};
  }
  __device__ __forceinline__ pair_t open(int p, int D) const {
    const rr_bank_pair d = pairs[p];
    return of(d.first_row, d.len, d.query, slot ? slot[p] : p, D);
  }
  // the wave's tile ct decoded into `tile` [16][D + LI_TILE_PAD] fp16: passes of rpw rows, D / 8 lanes per row as the bank's row
  // kernels; the pass loop is wave-uniform and EVERY lane reaches plaid_finish8 (its butterfly is cross-lane), loads and stores
  // are predicated; rows the pair does not hold are not written (and never read: row() is asked for held rows only)
  __device__ __forceinline__ void stage(const pair_t& pr, int ct, int D, int lane, uint16_t* tile) const {
    const int lpr = D / 8, rpw = min(64 / lpr, 16), sub = lane / lpr, c8 = lane - sub * lpr;
    for (int r0 = 0; r0 < 16; r0 += rpw) {
      const int r = r0 + sub, c = ct * 16 + r;
      const bool in = sub < rpw && c < pr.len;
      float s[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) s[k] = 0.f;
      if (in) plaid_load8<NBITS>(codes, resid, centroids, weights, C, pr.first_row + c, D, c8, s);
      plaid_finish8(s, lpr);                               // all 64 lanes; s now holds fp16 values, packing them is exact
      if (in)
        *(uint4*)(tile + r * (D + LI_TILE_PAD) + 8 * c8) =
            make_uint4(pack2h(s[0], s[1]), pack2h(s[2], s[3]), pack2h(s[4], s[5]), pack2h(s[6], s[7]));
    }
  }
  __device__ __forceinline__ cursor row(const pair_t&, int, int g, int D, int li, const uint16_t* tile) const {
    return tile + li * (D + LI_TILE_PAD) + 4 * g;
  }
  static __device__ __forceinline__ f32x4 at(cursor cur, int d) { return half4(cur + d); }
  __device__ __forceinline__ bool keep(const pair_t& pr, int row) const { return pr.mask[row] != 0; }
};

// f(source, tile_bytes) over the rows of `bank`; tile_bytes: the decoded tiles of the four waves behind the query block (0 for
// fp16 rows).  16-byte query loads are the caller's check; here: 8-byte loads of fp16 rows, plaid_tables_ok of compressed ones.
// nbits == 0 is the fp16 source whether or not the view also carries codes and a centroid table (rr_bank_set_centroids): the codes
// are the pruned stages' business, the rows scored are the fp16 rows.
template <class F>
hipError_t li_with_bank_source(const rr_bank_pair* pairs, const int32_t* slot, const rr_bank_view& bank, int D, F&& f) {
  if (D <= 0 || D % 16 || !bank.mask) return hipErrorInvalidValue;
  if (!bank.nbits) {
    if (!bank.rows || (((uintptr_t)bank.rows) & 7)) return hipErrorInvalidValue;
    return f(li_src_f16{pairs, slot, bank.rows, bank.mask}, (size_t)0);
  }
  if (!plaid_tables_ok(bank, D)) return hipErrorInvalidValue;
  const size_t tile_bytes = (size_t)4 * 16 * (D + LI_TILE_PAD) * sizeof(uint16_t);
  return plaid_with_nbits(bank.nbits, [&](auto nb) {
    return f(li_src_plaid<decltype(nb)::value>{pairs, slot, bank.codes, bank.resid, bank.centroids, bank.weights, bank.n_centroids, bank.mask},
             tile_bytes);
  });
}

// up to 150 KB of dynamic LDS for `kernel`, asked for once per device ordinal (attr_set: one word per kernel instantiation; see
// gemm_bf16.hip ensure_lds_attr)
inline hipError_t li_lds_attr(const void* kernel, std::atomic<unsigned long long>& attr_set) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= 64 || !((attr_set.load(std::memory_order_acquire) >> dev) & 1ull)) {
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64) attr_set.fetch_or(1ull << dev, std::memory_order_release);
  }
  return hipSuccess;
}

// the query tiles (16 columns) of a column block: the narrowest block that takes Lq in one pass (a tile without a column is
// matrix-core time), 128 columns beyond; halved while its query rows [16 JT][D + 4] and the decoded tiles exceed `limit` bytes (room
// for two workgroups per CU at 72 KB).  *lds: the dynamic LDS of the launch; 0 when even that exceeds what a workgroup can have
inline int li_pick_jt(int Lq, int D, size_t tile_bytes, size_t limit, size_t* lds) {
  int jt = Lq <= 16 ? 1 : Lq <= 32 ? 2 : Lq <= 64 ? 4 : 8;
  auto lds_bytes = [&](int t) { return (size_t)16 * t * (D + 4) * sizeof(float) + tile_bytes; };
  while (jt > 1 && lds_bytes(jt) > limit) jt /= 2;
  *lds = lds_bytes(jt);
  return *lds > 150 * 1024 ? 0 : jt;
}

}  // namespace
