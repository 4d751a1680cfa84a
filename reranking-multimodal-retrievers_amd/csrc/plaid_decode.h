// Row loaders and the PLAID residual decode of the passage bank, shared by the row kernels (passage_bank.hip) and the score
// kernel that reads its context rows from a bank (li_scores.hip).  THE DECODED ROW is defined in passage_bank.hip's header
// comment; plaid_bucket / plaid_sumsq8 / plaid_scale are compiled for both sides, plaid_load8 / plaid_finish8 are the one
// device definition every kernel decodes with.  plaid_with_nbits is the one place a runtime nbits becomes a template argument,
// plaid_tables_ok what every launcher checks of a compressed rr_bank_view, plaid_f16_bits / plaid_f16_value the fp16 conversions of
// the host definitions (passage_bank.hip, plaid_train.hip).
#pragma once
#include <type_traits>

#include "rr_common.h"

namespace {

__device__ __forceinline__ uint32_t pack2h(float lo, float hi) { return pack2<1>(lo, hi); }

// f(std::integral_constant<int, NBITS>) for nbits = 1, 2, 4 or 8 (rr_plaid_shape_ok has checked it; anything else takes 8)
template <class F>
inline auto plaid_with_nbits(int nbits, F&& f) {
  switch (nbits) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    default: return f(std::integral_constant<int, 8>{});
  }
}

// the tables of a compressed bank as a kernel reads them: 16-byte centroid chunks, nbits <= 8 residual bytes at once, int32 codes
inline bool plaid_tables_ok(const rr_bank_view& v, int D) {
  return rr_plaid_shape_ok(v.nbits, D) && v.n_centroids > 0 && v.codes && v.resid && v.centroids && v.weights &&
         !(((uintptr_t)v.centroids) & 15) && !(((uintptr_t)v.resid) & 7) && !(((uintptr_t)v.codes) & 3);
}

// float32 -> fp16 bits, round to nearest even, in host code (the device's conversion instruction rounds the same way)
inline uint16_t plaid_f16_bits(float f) {
  const uint32_t u = __builtin_bit_cast(uint32_t, f), sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
  if (a >= 0x7f800000u) return (uint16_t)(sign | (a > 0x7f800000u ? 0x7e00u : 0x7c00u));
  if (a >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                     // rounds to 65536 or beyond: inf
  if (a < 0x33000001u) return (uint16_t)sign;                                  // at most 2^-25: zero (the tie goes to even)
  const int e = (int)(a >> 23) - 127;
  uint32_t m = (a & 0x7fffffu) | 0x800000u;
  const int shift = e >= -14 ? 13 : 13 + (-14 - e);                            // subnormal halves lose more bits
  const uint32_t keep = m >> shift, rest = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
  uint32_t h = e >= -14 ? (((uint32_t)(e + 15) << 10) + (keep - 0x400u)) : keep;
  if (rest > half || (rest == half && (h & 1u))) ++h;                           // a carry into the exponent is the right value
  return (uint16_t)(sign | h);
}

// fp16 bits -> float, exact (host)
inline float plaid_f16_value(uint16_t hb) {
  const uint32_t sign = (uint32_t)(hb & 0x8000u) << 16, e = (hb >> 10) & 31u, m = hb & 0x3ffu;
  if (e == 0) return (sign ? -1.f : 1.f) * ((float)m * 5.9604644775390625e-8f);
  if (e == 31) return __builtin_bit_cast(float, sign | 0x7f800000u | (m << 13));
  return __builtin_bit_cast(float, sign | ((e + 112u) << 23) | (m << 13));
}

// 8 consecutive elements of a source row as floats; SRC_F16: the row holds fp16 bits
template <bool SRC_F16>
__device__ __forceinline__ void load8(const void* row, int c8, float (&v)[8]) {
  if constexpr (SRC_F16) {
    const uint4 u = ((const uint4*)row)[c8];
    const float2 a = unpack2<1>(u.x), b = unpack2<1>(u.y), c = unpack2<1>(u.z), d = unpack2<1>(u.w);
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y; v[4] = c.x; v[5] = c.y; v[6] = d.x; v[7] = d.y;
  } else {
    const float4 a = ((const float4*)row)[2 * c8], b = ((const float4*)row)[2 * c8 + 1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
}

// ---- PLAID residual decode.  plaid_bucket: the bucket of element k (0..7) of a lane's chunk from its NBITS residual bytes
// (r[b] = byte b of the chunk, in memory order).
template <int NBITS>
__host__ __device__ __forceinline__ uint32_t plaid_bucket(const uint8_t (&r)[NBITS], int k) {
  constexpr int per = 8 / NBITS;                       // elements per byte
  const int g = k % per;
  const uint32_t x = ((uint32_t)r[k / per] >> (8 - NBITS * (g + 1))) & ((1u << NBITS) - 1u);
  return __builtin_bitreverse32(x) >> (32 - NBITS);
}
// the sum of squares of one 8-element chunk: an explicit fmaf chain, element 0 first
__host__ __device__ __forceinline__ float plaid_sumsq8(const float (&s)[8]) {
  float q = fmaf(s[0], s[0], 0.f);
#pragma unroll
  for (int k = 1; k < 8; ++k) q = fmaf(s[k], s[k], q);
  return q;
}
// the divisor of the definition
__host__ __device__ __forceinline__ float plaid_scale(float n) { return fmaxf(n, 1e-12f); }

// one lane's chunk c8 of bank row `row`: s[0..8) = centroid + bucket weight.  code is clamped to [0, C): rr_bank_add_plaid has
// checked it on the host, rr_op_plaid_decode_rows runs over raw pointers and must not read outside the table.
template <int NBITS>
__device__ __forceinline__ void plaid_load8(const int32_t* __restrict__ codes, const uint8_t* __restrict__ resid,
                                            const uint16_t* __restrict__ centroids, const float* __restrict__ weights, int C,
                                            long long row, int D, int c8, float (&s)[8]) {
  const int code = min(max(codes[row], 0), C - 1);
  const uint8_t* rp = resid + (size_t)row * ((size_t)D / 8 * NBITS) + (size_t)c8 * NBITS;
  uint8_t r[NBITS];
  if constexpr (NBITS == 1) {
    r[0] = rp[0];
  } else if constexpr (NBITS == 2) {
    const uint32_t u = *(const uint16_t*)rp;
    r[0] = (uint8_t)u; r[1] = (uint8_t)(u >> 8);
  } else if constexpr (NBITS == 4) {
    const uint32_t u = *(const uint32_t*)rp;
#pragma unroll
    for (int b = 0; b < 4; ++b) r[b] = (uint8_t)(u >> (8 * b));
  } else {
    const uint2 u = *(const uint2*)rp;
#pragma unroll
    for (int b = 0; b < 4; ++b) { r[b] = (uint8_t)(u.x >> (8 * b)); r[4 + b] = (uint8_t)(u.y >> (8 * b)); }
  }
  float cv[8];
  load8<true>(centroids + (size_t)code * D, c8, cv);
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = cv[k] + weights[plaid_bucket<NBITS>(r, k)];
}

// s[0..8) of a lane (zeros where the lane decodes nothing) -> the decoded values as floats that hold fp16 values.  EVERY lane
// of the wave calls this: the butterfly over the lpr lanes of a row (lpr a power of two, the group aligned to it) is cross-lane.
__device__ __forceinline__ void plaid_finish8(float (&s)[8], int lpr) {
  float q = plaid_sumsq8(s);
  for (int o = 1; o < lpr; o <<= 1) q += __shfl_xor(q, o, 64);
  const float d = plaid_scale(sqrtf(q));
  uint32_t h[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) h[k] = pack2<1>(s[2 * k] / d, s[2 * k + 1] / d);      // fp16 FIRST, as the fp16 bank holds it
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float2 f = unpack2<1>(h[k]);
    s[2 * k] = f.x; s[2 * k + 1] = f.y;
  }
}

}  // namespace
