// The bank-side operand sources of the late-interaction score kernels, shared by li_scores.hip (one workgroup per pair,
// rr_bank_li_scores) and bank_search.hip (one wave per passage, rr_bank_search): where the four floats a lane feeds to one
// v_mfma_f32_16x16x4_f32 step come from.  One definition, so that both kernels run the same instruction sequence on the same
// float32 values (li_scores.hip's header comment describes the sources).
#pragma once
#include "plaid_decode.h"      // plaid_load8 / plaid_finish8, pack2h
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

}  // namespace
