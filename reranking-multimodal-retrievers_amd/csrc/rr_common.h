// Shared device/host helpers for librerank_mi355 (gfx950 only; wave = 64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

typedef uint16_t bf16_t;  // raw bf16 bit pattern
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;

#define RR_WAVE 64

// ---- bf16 <-> f32 (round-to-nearest-even; NaN stays NaN via the plain cast, which hipcc
// lowers to v_cvt_pk_bf16_f32 on gfx950 — MI355X_MICROARCH "Correctness boundaries").
__device__ __forceinline__ bf16_t f2bf(float f) {
  __bf16 b = (__bf16)f;
  return __builtin_bit_cast(bf16_t, b);
}
__device__ __forceinline__ float bf2f(bf16_t b) {
  return __builtin_bit_cast(float, ((uint32_t)b) << 16);
}
__device__ __forceinline__ uint32_t pack2bf(float lo, float hi) {
  typedef __attribute__((ext_vector_type(2))) float f32x2_;
  typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_;
  const f32x2_ v = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_));   // one v_cvt_pk_bf16_f32
}

// ---- 16-bit operand type of the MFMA path: DT 0 = bf16 (default, what the reference's bf16-mixed runs use),
// DT 1 = fp16 (same MFMA rate, 3 more mantissa bits; buffers are the same uint16 carriers).
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
template <int DT>
__device__ __forceinline__ uint32_t pack2(float lo, float hi) {
  if constexpr (DT == 0) {
    return pack2bf(lo, hi);
  } else {
    typedef __attribute__((ext_vector_type(2))) float f32x2_;
    typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_;
    const f32x2_ v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2_));   // round-to-nearest-even
  }
}
// the two 16-bit values of a packed word back as floats (exact)
template <int DT>
__device__ __forceinline__ float2 unpack2(uint32_t u) {
  if constexpr (DT == 0) {
    return make_float2(__builtin_bit_cast(float, u << 16), __builtin_bit_cast(float, u & 0xffff0000u));
  } else {
    typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_;
    const f16x2_ v = __builtin_bit_cast(f16x2_, u);
    return make_float2((float)v[0], (float)v[1]);
  }
}
// v_fma_mix_f32 (fp32 multiply-add whose operands may be the halves of packed fp16 registers): float(h) + float(l) and
// f - float(h) in ONE instruction each instead of convert + convert + add / convert + subtract.  h * 1.0 and h * -1.0 are
// exact, so the results are bit for bit those of the separate instructions.  hipcc does not form it from C++ (it emits
// v_cvt_f32_f16 + v_add_f32).  HALF: 0 = low, 1 = high half of the packed word.  VOP3P like the packed-f32 ops of the
// stale-lane hazard (DESIGN.md "Numerics"): a caller that feeds freshly loaded registers fences them first (mix_fence).
// `tok` (mix_fence) is an ordering-only operand: it ties the instruction behind the fence of the loads it reads.
template <int HALF>
__device__ __forceinline__ float mix_add_f16(uint32_t h, uint32_t l, uint32_t tok) {
  float d;
  if constexpr (HALF == 0) asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,1]" : "=v"(d) : "v"(h), "v"(l), "v"(tok));
  else asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[1,0,1] op_sel_hi:[1,0,1]" : "=v"(d) : "v"(h), "v"(l), "v"(tok));
  return d;
}
template <int HALF>
__device__ __forceinline__ float mix_add_f16_f32(float h, uint32_t l, uint32_t tok) {      // h (fp32) + float(half of l)
  float d;
  if constexpr (HALF == 0) asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(l), "v"(h), "v"(tok));
  else asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(l), "v"(h), "v"(tok));
  return d;
}
template <int HALF>
__device__ __forceinline__ float mix_sub_f16(float f, uint32_t h) {           // f - float(half of h)
  float d;
  if constexpr (HALF == 0) asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(h), "v"(f));
  else asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(h), "v"(f));
  return d;
}
// Two wait states between a counted vmcnt release of freshly loaded registers and their first VOP3P reader.  The loaded
// registers are INPUTS only (as in/out operands of an asm statement hipcc copied them out of the load destinations, with a
// vmcnt(0) behind every load: the next pass's residual loads became synchronous, 4.9k -> 36k cycles per tile); the
// returned token orders the readers behind the fence.
__device__ __forceinline__ uint32_t mix_fence(const uint4& a, const uint4& b) {
  uint32_t t;
  asm volatile("s_nop 1\n\tv_mov_b32 %0, 0" : "=v"(t) : "v"(a.x), "v"(b.x));
  return t;
}
__device__ __forceinline__ uint32_t mix_fence(const uint4& a, const uint2& b) {
  uint32_t t;
  asm volatile("s_nop 1\n\tv_mov_b32 %0, 0" : "=v"(t) : "v"(a.x), "v"(b.x));
  return t;
}
// ---- streaming accesses of the GEMM epilogues.  An output row is written once and next read by another launch, a residual
// row is read once: neither is worth an L2 line, and the lines they would take are the operand panels the workgroups of an
// XCD share (RR_NT bit 0: outputs stored with the `nt` hint, bit 1: residual rows loaded with it; measured in DESIGN.md).
#ifndef RR_NT
#define RR_NT 1
#endif
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2_;
__device__ __forceinline__ void store_stream(void* p, const uint4& v) {
  if constexpr ((RR_NT & 1) != 0) __builtin_nontemporal_store(u32x4_{v.x, v.y, v.z, v.w}, (u32x4_*)p);
  else *(uint4*)p = v;
}
__device__ __forceinline__ void store_stream(void* p, const uint2& v) {
  if constexpr ((RR_NT & 1) != 0) __builtin_nontemporal_store(u32x2_{v.x, v.y}, (u32x2_*)p);
  else *(uint2*)p = v;
}
__device__ __forceinline__ void store_stream(void* p, const float4& v) {
  if constexpr ((RR_NT & 1) != 0) __builtin_nontemporal_store(f32x4{v.x, v.y, v.z, v.w}, (f32x4*)p);
  else *(float4*)p = v;
}
__device__ __forceinline__ uint4 load_stream_u4(const void* p) {
  if constexpr ((RR_NT & 2) != 0) {
    const u32x4_ v = __builtin_nontemporal_load((const u32x4_*)p);
    return make_uint4(v.x, v.y, v.z, v.w);
  } else {
    return *(const uint4*)p;
  }
}
__device__ __forceinline__ float4 load_stream_f4(const void* p) {
  if constexpr ((RR_NT & 2) != 0) {
    const f32x4 v = __builtin_nontemporal_load((const f32x4*)p);
    return make_float4(v.x, v.y, v.z, v.w);
  } else {
    return *(const float4*)p;
  }
}
__device__ __forceinline__ uint2 load_stream_u2(const void* p) {
  if constexpr ((RR_NT & 2) != 0) {
    const u32x2_ v = __builtin_nontemporal_load((const u32x2_*)p);
    return make_uint2(v.x, v.y);
  } else {
    return *(const uint2*)p;
  }
}
// ---- 8-bit `lo` half of the split residual stream (GemmFold::lo_bits == 8): lo = x - hi travels as OCP e5m2 ("bf8") of
// lo * 2^RR_LO8_SHIFT, converted by gfx950's scaled pack / unpack instructions (the scale operand is the MX block scale 2^-SHIFT:
// encode divides by it, decode multiplies).  |lo| <= ulp(hi) / 2, so three significant bits of lo put x at 14 (fp16 hi) / 11
// (bf16 hi) significant bits in the worst case, a power of two beyond what the 16-bit MFMA operand keeps of it anyway; the
// shift keeps lo * 2^SHIFT a NORMAL e5m2 number (>= 2^-14) for every |x| >= 2^-7 (fp16 hi) and below the e5m2 maximum (57 344)
// for |x| < 2^22 (fp16 rows end at 6.5e4; bf16 rows beyond 9e5 saturate lo, i.e. fall back to the hi half's precision); smaller
// x keep an absolute error <= 2^-21.  WORD: 0 / 1 = the low / high 16 bits of the packed dword (two e5m2 values each).
constexpr int RR_LO8_SHIFT = 4;
#ifndef RR_RESID_LO8_DEFAULT
#define RR_RESID_LO8_DEFAULT (-1)   // process-wide default of the "resid_lo8" option (rr_api.hip): -1 = by operand type (fp16: on, bf16: off)
#endif
// Memory layout of the 8-bit lo rows, private to the residual epilogues that write and read them: rows r and r + 16 of an aligned
// group of 32 rows are interleaved in units of 8 columns, so that a lane's 8 columns of BOTH rows are one 16-byte chunk (8-byte
// accesses reach 0.54 - 0.70 x of the 16-byte rate here).  Byte offset of the chunk that holds columns col .. col + 7 (col % 8 == 0)
// of row r (r % 32 < 16: first 8 bytes) and row r + 16 (last 8 bytes); ld = columns per row.  The buffer spans ceil(M / 32) * 32 rows.
__device__ __forceinline__ size_t lo8_pair_offset(int r, int col, int ld) {
  return ((size_t)(r >> 5) * 16 + (r & 15)) * (size_t)(2 * ld) + (size_t)col * 2;
}
template <int WORD>
__device__ __forceinline__ float2 lo8_decode(uint32_t w, float mx_scale, uint32_t tok) {   // two e5m2 -> fp32, times mx_scale
  typedef __attribute__((ext_vector_type(2))) float f32x2_;
  f32x2_ d;
  if constexpr (WORD == 0) asm("v_cvt_scalef32_pk_f32_bf8 %0, %1, %2" : "=v"(d) : "v"(w), "s"(mx_scale), "v"(tok));
  else asm("v_cvt_scalef32_pk_f32_bf8 %0, %1, %2 op_sel:[1,0,0]" : "=v"(d) : "v"(w), "s"(mx_scale), "v"(tok));
  return make_float2(d.x, d.y);
}
template <int WORD>
__device__ __forceinline__ uint32_t lo8_encode(uint32_t old, float a, float b, float mx_scale) {   // e5m2(a / mx_scale), e5m2(b / mx_scale) into half WORD of `old`
  if constexpr (WORD == 0) asm("v_cvt_scalef32_pk_bf8_f32 %0, %1, %2, %3" : "+v"(old) : "v"(a), "v"(b), "s"(mx_scale));
  else asm("v_cvt_scalef32_pk_bf8_f32 %0, %1, %2, %3 op_sel:[0,0,0,1]" : "+v"(old) : "v"(a), "v"(b), "s"(mx_scale));
  return old;
}
__device__ __forceinline__ uint32_t pack2rt(float lo, float hi, int dt) { return dt ? pack2<1>(lo, hi) : pack2<0>(lo, hi); }
template <int DT>
__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
  if constexpr (DT == 0) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
template <int DT>
__device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) {
  if constexpr (DT == 0) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// erf-GELU, gelu(x) = max(x, 0) - z Phi(-z) with z = min(|x|, 5.7) and log2 Phi(-z) a polynomial in z: plain VALU operations
// and ONE transcendental (the exp2) instead of eleven and two (exp2 + rcp) for the Abramowitz-Stegun 7.1.26 form of round 1 — the
// GELU runs exposed in the FFN-up epilogue, 128 values per lane and tile, vector-issue-bound.
// RR_GELU_DEGREE 5 (round 5): a minimax fit of the ABSOLUTE error of z 2^p(z) on [0, 5.7] (Lawson reweighting:
// tools/study/fit_gelu_tail.py): |gelu - exact| <= 6.4e-7 over [-12, 12] evaluated in fp32 with fused multiply-adds, relative error <= 2.8e-4
// wherever |gelu| >= 1e-3 — two FMAs per value fewer than the degree-7 fit of rounds 2-4 (4.8e-7 / 3.4e-5; RR_GELU_DEGREE 7 keeps
// it for A/B runs), still two to three orders below the 16-bit rounding of the output (fp16: 4.9e-4 relative).
// Beyond |x| = 5.7 the neglected term is below 6e-8.
// NaN in, NaN out: max(x, 0) is formed as x - min(x, 0) — min drops a NaN (IEEE minNum), the subtraction brings it back — where
// med3(x, 0, +inf) returned 0 for a NaN and, with z = min(|NaN|, 5.7) = 5.7, made gelu(NaN) = -1e-8: a NaN in an FFN-up weight or
// bias became an ordinary column and never reached the range guard (tests/test_gpu_nonfinite.py).  +inf -> +inf, -inf -> NaN.
#ifndef RR_GELU_DEGREE
#define RR_GELU_DEGREE 5
#endif
__device__ __forceinline__ float gelu_erf_fast(float x) {
  const float z = fminf(fabsf(x), 5.7f);
#if RR_GELU_DEGREE == 7
  float p = -1.403277905e-06f;
  p = fmaf(p, z, 5.490869060e-05f);
  p = fmaf(p, z, -8.929630618e-04f);
  p = fmaf(p, z, 8.417915996e-03f);
  p = fmaf(p, z, -5.388785911e-02f);
  p = fmaf(p, z, -4.584285712e-01f);
  p = fmaf(p, z, -1.151314700e+00f);
  p = fmaf(p, z, -9.999805559e-01f);
#else
  float p = -4.733084352e-04f;
  p = fmaf(p, z, 7.084545679e-03f);
  p = fmaf(p, z, -5.182733759e-02f);
  p = fmaf(p, z, -4.599924982e-01f);
  p = fmaf(p, z, -1.150787830e+00f);
  p = fmaf(p, z, -1.000037670e+00f);
#endif
  return fmaf(-z, __builtin_amdgcn_exp2f(p), x - fminf(x, 0.0f));   // x - min(x, 0) = max(x, 0), exact for every finite x; NaN stays NaN
}

// The same function on two values with the Horner chain as v_pk_fma_f32 (two fp32 lanes per instruction at the full VALU
// rate: 8 packed multiply-adds for the pair instead of 16 scalar ones; |x|, min, exp2 and max(x, 0) stay scalar).
// Every packed operand is VALU-produced (z from v_min, p from the previous packed op, coefficients from SGPR pairs), so the
// stale-lane hazard of packed-f32 ops behind a vmcnt release (DESIGN.md "Numerics") cannot arise here; each lane's result
// is the same IEEE fma chain as gelu_erf_fast, bit for bit.
#ifndef RR_PK_GELU
#define RR_PK_GELU 1
#endif
typedef __attribute__((ext_vector_type(2))) float f32x2;
__device__ __forceinline__ f32x2 gelu_erf_fast2(f32x2 x) {
  const f32x2 z = {fminf(fabsf(x.x), 5.7f), fminf(fabsf(x.y), 5.7f)};
#if RR_GELU_DEGREE == 7
  f32x2 p = {-1.403277905e-06f, -1.403277905e-06f};
  p = __builtin_elementwise_fma(p, z, f32x2{5.490869060e-05f, 5.490869060e-05f});
  p = __builtin_elementwise_fma(p, z, f32x2{-8.929630618e-04f, -8.929630618e-04f});
  p = __builtin_elementwise_fma(p, z, f32x2{8.417915996e-03f, 8.417915996e-03f});
  p = __builtin_elementwise_fma(p, z, f32x2{-5.388785911e-02f, -5.388785911e-02f});
  p = __builtin_elementwise_fma(p, z, f32x2{-4.584285712e-01f, -4.584285712e-01f});
  p = __builtin_elementwise_fma(p, z, f32x2{-1.151314700e+00f, -1.151314700e+00f});
  p = __builtin_elementwise_fma(p, z, f32x2{-9.999805559e-01f, -9.999805559e-01f});
#else
  f32x2 p = {-4.733084352e-04f, -4.733084352e-04f};
  p = __builtin_elementwise_fma(p, z, f32x2{7.084545679e-03f, 7.084545679e-03f});
  p = __builtin_elementwise_fma(p, z, f32x2{-5.182733759e-02f, -5.182733759e-02f});
  p = __builtin_elementwise_fma(p, z, f32x2{-4.599924982e-01f, -4.599924982e-01f});
  p = __builtin_elementwise_fma(p, z, f32x2{-1.150787830e+00f, -1.150787830e+00f});
  p = __builtin_elementwise_fma(p, z, f32x2{-1.000037670e+00f, -1.000037670e+00f});
#endif
  const f32x2 e = {__builtin_amdgcn_exp2f(p.x), __builtin_amdgcn_exp2f(p.y)};
  const f32x2 m = {x.x - fminf(x.x, 0.0f), x.y - fminf(x.y, 0.0f)};   // as gelu_erf_fast; scalar: the build admits no packed add
  return __builtin_elementwise_fma(-z, e, m);
}

// LDS byte offset of 16-byte chunk `c` (0..7) of row `row` in a [rows][64 x bf16] tile image
// (128-byte rows).  XOR with (row>>1)&7 keeps every ds_read_b128 lane group (16 rows of one
// chunk column, cdna_hip_programming.md §2 / T2) on 16 distinct 16-byte slots of the
// 256-byte bank row => conflict-free.
__device__ __forceinline__ int swz128(int row, int c) { return row * 128 + ((c ^ ((row >> 1) & 7)) << 4); }

// LDS-DMA of 64 x 16 B: LDS destination = wave-uniform byte address (M0) + lane*16, per-lane global source.
// Issued from inline asm on purpose: hipcc's waitcnt pass treats the builtin form like a FLAT access and
// then degrades every later `s_waitcnt lgkmcnt(N)` in the loop to lgkmcnt(0), which serialises the
// ds_read -> MFMA software pipeline.  The DMA is counted by hand (wait_vmcnt below); no compiler-visible
// VMEM load lives inside the main loop (cdna_hip_programming.md §5.7 item 1).
__device__ __forceinline__ void glds16(const void* gsrc, uint32_t lds_dst_wave_base) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(lds_dst_wave_base)
      : "memory");
}
// same, global address = 64-bit scalar base + 32-bit per-lane byte offset (keeps 1 VGPR per source instead of 2)
__device__ __forceinline__ void glds16_so(const void* sbase, uint32_t voff, uint32_t lds_dst_wave_base) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %3\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %2\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase), "s"(lds_dst_wave_base)
      : "memory");
}

// 4 bytes per lane into LDS (wave-uniform destination + lane*4): used as a no-register "touch" that pulls one 128-byte
// line per lane towards the XCD's L2 ahead of the real loads (the bytes that land in LDS are never read)
__device__ __forceinline__ void glds4_so(const void* sbase, uint32_t voff, uint32_t lds_dst_wave_base) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %3\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dword %1, %2\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase), "s"(lds_dst_wave_base)
      : "memory");
}

__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)p;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// host-side launcher signatures (implemented in the .hip files) ---------------------------------
enum GemmEpilogue {
  EPI_BIAS_BF16 = 0,       // C = bf16(A W^T + b)
  EPI_BIAS_GELU_BF16 = 1,  // C = bf16(gelu_erf(A W^T + b))
  EPI_BIAS_F32 = 2,        // C = f32(A W^T + b)
  EPI_BIAS_TANH_BF16 = 3,  // C = bf16(tanh(A W^T + b))
  EPI_BIAS_RESID_F32 = 4,  // C = f32(A W^T + b + R)
  EPI_BIAS_QGELU_BF16 = 5  // C = 16bit(quick_gelu(A W^T + b)), x * sigmoid(1.702 x)  (CLIP ViT MLP)
};

// A [M,Kd] bf16 (row stride lda), W [N,Kd] bf16 (row stride ldw), bias [N] f32 or null,
// resid [M,N] f32 (row stride ldr, EPI 4) ; C row stride ldc (elements of its type).
hipError_t rr_launch_gemm(const bf16_t* A, int lda, const bf16_t* W, int ldw, const float* bias,
                          const float* resid, int ldr, void* C, int ldc, int M, int N, int Kd,
                          int epilogue, int dt, hipStream_t st);

// LayerNorm folded into the consumer GEMM (gemm_bf16.hip "LnResid"): producer outputs of a residual GEMM (`x16` 16-bit copy
// of the fp32 result rows, row stride ldx; `part` [M][nparts] per-128-column-group (mean, sum of squared deviations),
// nparts = ceil(N / 128)) and/or consumer inputs (`in_stats` [M] (mean, rstd) of the raw A rows, `csum` [N] column sums
// of the gamma-folded weight; `bias` then holds d = W beta + b).
struct GemmFold {
  bf16_t* x16 = nullptr;
  int ldx = 0;
  float* part = nullptr;
  int nparts = 0;
  const float* in_stats = nullptr;
  const float* csum = nullptr;
  // split residual stream (persistent ring kernel only; rr_gemm_split_ok): a pre-LayerNorm row x is carried as the pair
  // hi = 16-bit operand rounding of x (the very `x16` rows the consumer GEMM reads) + lo = fp16(x - hi), 22 (fp16 operands)
  // or 19 (bf16) significant bits, instead of a third copy in fp32: the residual epilogue moves 8 instead of 10 bytes
  // per element.  r_hi / r_lo: where THIS launch's residual rows come from (in place of `resid`); lo_out: where the lo
  // half of the output rows goes (the hi half is x16; the fp32 output C is then not written).  In-place use (r_hi == x16,
  // r_lo == lo_out) is allowed: an element is read and written by the same thread, read first.
  const bf16_t* r_hi = nullptr;
  const bf16_t* r_lo = nullptr;
  int ld16 = 0;
  bf16_t* lo_out = nullptr;
  // 16: lo rows are fp16 [M][ld16]; 8: e5m2 bytes of lo * 2^RR_LO8_SHIFT, [M][ld16] BYTES (r_lo / lo_out point at bytes): the
  // residual epilogue moves 6 instead of 8 bytes per element and touches 3 instead of 4 cache lines per 64 columns
  int lo_bits = 16;
};
// true when a GEMM with M x N output will run on the kernel that implements the split residual stream
bool rr_gemm_split_ok(int M, int N);
hipError_t rr_launch_gemm_ln(const bf16_t* A, int lda, const bf16_t* W, int ldw, const float* bias, const float* resid,
                             int ldr, const float* ln_stats, const float* ln_gamma, const float* ln_beta, void* C, int ldc,
                             int M, int N, int Kd, int epilogue, int dt, hipStream_t st);
hipError_t rr_launch_gemm_fold(const bf16_t* A, int lda, const bf16_t* W, int ldw, const float* bias, const float* resid,
                               int ldr, const float* ln_stats, const float* ln_gamma, const float* ln_beta,
                               const GemmFold& fold, void* C, int ldc, int M, int N, int Kd, int epilogue, int dt,
                               hipStream_t st);
// (mean, sum of squared deviations) per 128-column group -> (mean, rstd) per row (Chan's pairwise merge, fp32)
// Walking direction of the next large launch of the layer chain (QKV -> attention -> attention-out -> FFN-up -> FFN-down -> ...):
// consecutive launches walk the rows in opposite directions (rr_set_tuning("m_alternate", 0) switches it off), so that a consumer
// starts on the rows its producer wrote LAST — the ones the 256 MB memory-side cache may still hold.  Speed only: every tile /
// block computes the same values whichever order they run in (logits bit-identical; three interleaved A/Bs of the c3 step on one
// box: 87.44 / 87.61 / 87.46 ms off, 87.22 / 87.50 / 87.28 on).  A process-wide launch counter decides, nothing else depends on it;
// launches of fewer than two tiles per CU / 2 048 attention blocks do not take part.  0 = ascending.
int rr_m_direction_next();
constexpr float RR_RANGE_SS_FP16 = 9.0e8f;      // row sum of squares below which no element can exceed 3e4 (fp16 operand rows)
hipError_t rr_launch_ln_finalize(const float* part, int nparts, int cols, float eps, int rows, float* stats, hipStream_t st,
                                 int* range_flag = nullptr, float range_ss = RR_RANGE_SS_FP16);

// fp8 (csrc/gemm_fp8.hip, elementwise.hip)
hipError_t rr_launch_gemm_fp8(const uint8_t* A, int lda, const uint8_t* W, int ldw, const float* bias, float scale,
                              const float* row_scale, const float* col_scale, void* C, int ldc, int M, int N, int Kd,
                              int epilogue, int dt, hipStream_t st, float out_mul = 1.0f, const float* resid = nullptr,
                              int ldr = 0, const float* rstats = nullptr, const float* rgamma = nullptr,
                              const float* rbeta = nullptr);
bool rr_gemm_fp8_ring_ok(int M, int N, int Kd);   // the shapes whose e4m3 GEMM runs on the persistent ring (epilogues 3 / 4 exist there only)
hipError_t rr_launch_layernorm_q8(const float* x, const float* gamma, const float* beta, float eps, int rows, int cols,
                                  uint8_t* out8, float* row_scale, float* stats_out, hipStream_t st);
// int8 forms (W8A8, handle option "q8_format" = 1): signed codes, one scale per row / output channel, epilogues 0 - 2 only
hipError_t rr_launch_gemm_i8(const int8_t* A, int lda, const int8_t* W, int ldw, const float* bias, float scale,
                             const float* row_scale, const float* col_scale, void* C, int ldc, int M, int N, int Kd,
                             int epilogue, int dt, hipStream_t st);
hipError_t rr_launch_layernorm_i8(const float* x, const float* gamma, const float* beta, float eps, int rows, int cols,
                                  int8_t* out8, float* row_scale, float* stats_out, hipStream_t st);

// Multi-head attention, head dim 64.  q rows: q + (bq*Tq + t)*q_stride + head*64, where
// bq = (b + q_batch_off) / q_batch_div;  k,v rows: (b*Tk + t)*kv_stride + head*64;  key_bias [B,Tk] f32 additive
// (0 valid, -1e30 masked) or null;  out rows: (b*Tq + t)*out_stride + head*64 (bf16).
hipError_t rr_launch_attention(const bf16_t* q, int q_stride, int q_batch_div, int q_batch_off, const bf16_t* k,
                               const bf16_t* v, int kv_stride, const float* key_bias, int B,
                               int heads, int Tq, int Tk, bf16_t* out, int out_stride, int dt,
                               hipStream_t st, const float* dense_bias = nullptr, int dense_ld = 0, long schedule_blocks = 0,
                               int fixed_mode = -1);
hipError_t rr_launch_attention_segs(const bf16_t* q, int q_stride, const bf16_t* k, const bf16_t* v, int kv_stride,
                                    const float* key_bias, int heads, int nseg, const int* seg_n, const int* seg_len,
                                    const long long* seg_row0, bf16_t* out, int out_stride, int dt, hipStream_t st,
                                    long schedule_blocks, int fixed_mode = -1);
// dense_bias: optional additive bias [B][Tq][dense_ld] (dense_ld a multiple of 64 >= Tk, zero padded), PreFLMR fusion
hipError_t rr_launch_fusion_adj(const float* scores, int S, int Tq, int Tc, float mult, int pair0, int n, float* adj, int ld,
                                hipStream_t st, int row0 = 2);
// the same for a packed call, ONE launch: nseg (<= 64) segments of seg_n[s] pairs (HOST arrays) in the packed order, whose
// sequences end after seg_tk[s] of the Tc context tokens; the softmax normalisers still run over all Tc.  adj holds the
// segments one after the other, segment s as [seg_n[s]][Tq + seg_tk[s]][round_up(Tq + seg_tk[s], 64)]
#define RR_FUSION_MAX_SEGS 64
hipError_t rr_launch_fusion_adj_segs(const float* scores, int S, int Tq, int Tc, float mult, int nseg, const int* seg_n,
                                     const int* seg_tk, float* adj, hipStream_t st, int row0);
// the retriever's late-interaction score matrix [n][Lc][Lq] (-9999 on masked rows and on rows Lc_in <= c < Lc) and MaxSim [n]
// of n pairs from pair pair0 on, in exact f32 (li_scores.hip); context_li / context_mask hold Lc_in rows per pair; scores or
// maxsim may be null
hipError_t rr_launch_li_scores(const float* query_li, const float* context_li, const float* context_mask, int n, int K, int Lq,
                               int Lc_in, int Lc, int D, int pair0, float* scores, float* maxsim, hipStream_t st);

// CLIP ViT front end: im2col of the stride = kernel patch convolution, and [class | patches] + position -> pre_layrnorm
hipError_t rr_launch_vit_im2col(const float* px, bf16_t* out, int B, int IS, int ps, int Kp, int dt, hipStream_t st);
hipError_t rr_launch_vit_embed_ln(const float* patches, const float* cls_emb, const float* pos, const float* gamma,
                                  const float* beta, float eps, int rows, int T, int cols, float* o32, hipStream_t st);

hipError_t rr_launch_layernorm(const float* x, const float* gamma, const float* beta, float eps,
                               int rows, int cols, float* out_f32, bf16_t* out_bf16, int dt, hipStream_t st);

// rr_assemble_pairs: one packed pair as the host stages it (descriptor checked against pool and segment; row0 = its first entry
// in the packed rows, len = its segment's length)
struct rr_asm_pair { int32_t qoff, la, coff, lb, len, row0, unused0, unused1; };
hipError_t rr_launch_assemble_pairs(const int32_t* pool, long long pool_len, const rr_asm_pair* pairs, int n_pairs, long long cls,
                                    long long sep, long long pad, int64_t* ids, int64_t* am, int64_t* tt, hipStream_t st);

// rr_assemble_joint: one packed pair of the joint family as the host stages it (descriptor checked against pool and segment;
// the query's ql ids then its ql mask values at qoff, the context run t[0:m] at coff, ctx_w = padded length - ql the context
// window of the joint row, row0 = its first entry in the packed rows, len = its segment's length)
struct rr_asm_joint { int32_t qoff, ql, coff, m, ctx_w, len, row0, unused0; };
hipError_t rr_launch_assemble_joint(const int32_t* pool, long long pool_len, const rr_asm_joint* pairs, int n_pairs, long long sep,
                                    long long pad, int64_t* ids, int64_t* am, hipStream_t st);

// Passage bank (passage_bank.hip).  rr_bank_slot: one passage of an rr_bank_add as the host stages it (its first row in the bank,
// its length).  rr_bank_pair: one packed pair of rr_forward_interaction_bank (the passage's first bank row and length, the pair's
// query), checked against the bank, the segment and n_queries before it is staged.
struct rr_bank_slot { int64_t first_row; int32_t len, unused0; };
struct rr_bank_pair { int64_t first_row; int32_t len, query; };
// The padded source of an add as both launchers that take one read it: src [n][Lc][D] (src_f16: fp16 bits, else float32), mask
// [n][Lc] float32, slots[i] = (first destination row, length) on the device.  slots == null (rr_launch_plaid_compress alone): src
// holds its rows back to back, no mask, n and Lc unused.
struct rr_padded_rows { const void* src; int src_f16; const float* mask; const rr_bank_slot* slots; int n, Lc; };
hipError_t rr_launch_bank_ingest(const rr_padded_rows& in, int D, uint16_t* rows, uint8_t* mask_bytes, hipStream_t st);
// The context rows of a bank as the launchers take them, fp16 or compressed (PLAID residual codes): nbits == 0: `rows` [.][D] fp16
// bits; else codes [.] int32, resid [.][D * nbits / 8], centroids [n_centroids][D] fp16 bits, weights [2^nbits] float32.  mask:
// one byte per row.  All on the device.  bank_api.hip builds it from an rr_bank (bank_view), the diagnostic operators from their
// loose pointers; every launcher below decides between the two kinds inside.  nbits == 0 with non-null codes and centroids: fp16
// rows WITH codes (rr_bank_set_centroids): a row source reads `rows` as of any fp16 bank, the pruned stages and the inverted file
// read codes / centroids / n_centroids as of a compressed bank.
struct rr_bank_view {
  int nbits, n_centroids;
  const uint16_t* rows;
  const int32_t* codes;
  const uint8_t* resid;
  const uint16_t* centroids;
  const float* weights;
  const uint8_t* mask;
};
// the bytes one context row costs a kernel that reads it (a compressed row: its code, its residual bytes and the centroid row from L2)
inline double rr_bank_row_bytes(const rr_bank_view& v, int D) { return v.nbits ? 4.0 + D * (v.nbits / 8.0 + 2.0) : 2.0 * D; }
// one segment of rr_forward_interaction_bank; a compressed bank's rows are decoded in the gather (passage_bank.hip)
hipError_t rr_launch_bank_gather(const rr_bank_pair* pairs, int n, int Lq, int S, int D, const float* query_li,
                                 const float* query_mask, const rr_bank_view& bank, bf16_t* li16, int dt, float* qmask_out,
                                 float* cmask_out, float* q32_out, float* c32_out, hipStream_t st);
// compressed bank: the stand-alone decode of a row range (rows and mask of the view unused)
hipError_t rr_launch_plaid_decode(const rr_bank_view& bank, int D, long long first_row, long long n_rows, uint16_t* out, hipStream_t st);
int rr_set_li_lds_kb(int kb);      // rr_set_tuning("li_lds_kb"): 16 .. 150, -1 outside (li_scores.hip)
// the score matrix [n][Lc][Lq] and MaxSim [n] of a pair list with the context rows read from a bank: the kernel of
// rr_launch_li_scores over another operand source, bit for bit its result on the same rows (li_scores.hip); slot [n] on the device
// or null: the output row of workgroup p
hipError_t rr_launch_bank_li_scores(const rr_bank_pair* pairs, const int32_t* slot, int n, int Lq, int Lc, int D, const float* query_li,
                                    const rr_bank_view& bank, float* scores, float* maxsim, hipStream_t st);
// A caller's candidate filter as the three filtered searches take it ("CANDIDATE FILTERS", include/rerank_mi355.h): bits [rows][ld]
// uint32 on the device, bit (i & 31) of word (i >> 5) of a row = the ABSOLUTE bank index i; rows 1 (every query) or n_queries;
// `first`: the bank index of the range's first passage.  bits == null: no filter.  word(q, w) and allowed(q, p) (p range-relative)
// are asked with wave-uniform arguments, so the word is a scalar load.
struct rr_passage_filter {
  const uint32_t* bits;
  int rows;
  long long ld;
  int first;
  __device__ __forceinline__ uint32_t word(int q, int w) const { return bits[(size_t)(rows == 1 ? 0 : q) * ld + w]; }
  __device__ __forceinline__ bool allowed(int q, int p) const {
    const int i = first + p;
    return (word(q, i >> 5) >> (i & 31)) & 1u;
  }
  // the filter bits of the range-relative passages 32 w .. 32 w + 31 of a range of n: a range that does not start at a multiple of
  // 32 takes them from two words of the row (a funnel shift); no word behind the range's last is read
  __device__ __forceinline__ uint32_t range_word(int q, int w, int n) const {
    const long long i = (long long)first + (long long)w * 32;
    const int fw = (int)(i >> 5), sh = (int)(i & 31);
    const uint32_t lo = word(q, fw);
    const uint32_t hi = (sh && ((long long)fw + 1) * 32 < (long long)first + n) ? word(q, fw + 1) : 0u;
    return (uint32_t)((((unsigned long long)hi << 32) | lo) >> sh);
  }
};
// rr_bank_search (bank_search.hip): out [nq][n] = the MaxSim of every query against the passages table[0 .. n) (the bits of
// rr_launch_bank_li_scores' maxsim at Lc = the passage's length), and the selection: the first k of every list in the order of a
// stable descending sort (NaN first, ties by ascending index), indices + add; tmp_a / tmp_b hold rr_topk_select_scratch int32 each
// filter.bits given (rr_bank_search_filtered): a passage whose bit is clear gets -inf and is not read
hipError_t rr_launch_bank_search_scores(const rr_bank_slot* table, int n, int nq, int Lq, int D, const float* query_li,
                                        const rr_bank_view& bank, const rr_passage_filter& filter, float* out, hipStream_t st);
// the same for the passages list[q][0 .. cnt[q]) of every query (cnt[q] <= list_ld; entries of table[0 .. n)), written to the
// passage's entry of the dense out [nq][n]; fp16 rows or compressed.  With cand (cap > 0; or null and 0) for the passages
// cand[q][list[q][i]], i < cnt[q]: a list entry is a PLACE in the query's candidate list cand [nq][cap] (entries of table[0 .. n)),
// and the score goes to that place of the compact out [nq][cap] (rr_bank_search_plaid_ivf)
hipError_t rr_launch_bank_search_scores_listed(const rr_bank_slot* table, int n, int nq, int Lq, int D, const float* query_li,
                                               const rr_bank_view& bank, const int32_t* list, int list_ld, const int32_t* cnt,
                                               const int32_t* cand, int cap, float* out, hipStream_t st);
// the passages 0 .. cnt - 1 of a row from list / offsets as a bitmap (rr_bank_filter_fill; bank_ivf.hip): staged [rows + 1] int64
// offsets and the int32 indices behind them, both on the device; bits [rows][ld].  exclude: every bit below `passages` but those.
hipError_t rr_launch_filter_fill(const int64_t* offsets, const int32_t* indices, int rows, int exclude, int passages, uint32_t* bits,
                                 long long ld, hipStream_t st);
// the definition in host code (rr_util_bank_filter_bits); false, with nothing written, for an index outside [0, passages), offsets
// that do not ascend from 0 or ld < ceil(passages / 32)
bool rr_filter_bits_host(const int32_t* indices, const int64_t* offsets, int rows, int exclude, int passages, uint32_t* bits, long long ld);
// One workgroup per list (plaid_list_select_kernel, bank_search_plaid.hip): the entries list_in[q][0 .. n_in) whose score in
// scores [nq][n] is not -inf, in rank order; the first `keep` (n_in <= 1024) to list_out [nq][keep] (+ add) and scores_out (or null),
// -1 / -inf behind them, their number to cnt_out [nq].  The last step of rr_bank_search_filtered.
hipError_t rr_launch_list_select(const float* scores, long long n, int nq, const int32_t* list_in, int n_in, int keep, int32_t* list_out,
                                 int32_t* cnt_out, int add, float* scores_out, hipStream_t st);
size_t rr_topk_select_scratch(int n_lists, int n, int k);
hipError_t rr_launch_topk_select(const float* scores, int n_lists, int n, int k, int add, int32_t* tmp_a, int32_t* tmp_b,
                                 int32_t* indices_out, float* scores_out, hipStream_t st);
// rr_bank_search_f16 (bank_search_f16.hip): out [nq][n] = the MaxSim of every query, rounded once to fp16, against the passages
// table[0 .. n) of an fp16 bank (plain or coded), accumulated by v_mfma_f32_16x16x32_f16: an approximation of
// rr_launch_bank_search_scores' row, a query block per workgroup.  D a multiple of 32, rows 16-byte aligned.
// rr_launch_f16_certify: certified [nq] from A [nq][n], the survivors surv [nq][m] in rank order over A, the k exact scores
// [nq][k] and their counts cnt [nq] (rr_launch_list_select's): cnt == k and (m == n or score_k > A[last survivor] + slack).
hipError_t rr_launch_bank_scores_f16(const rr_bank_slot* table, int n, int nq, int Lq, int D, const float* query_li, const rr_bank_view& bank,
                                     float* out, hipStream_t st);
hipError_t rr_launch_f16_certify(const float* A, long long n, const int32_t* surv, int m, const float* scores, const int32_t* cnt, int k, float slack,
                                 int nq, int32_t* certified, hipStream_t st);
// rr_bank_search_f16_plaid (bank_search_f16_plaid.hip): rr_launch_bank_scores_f16's out over a COMPRESSED bank, bit for bit what that
// launch gives over the decoded rows; a row is decoded once per query block, into LDS.  rr_bank_scores_f16_plaid_dim_ok: the D it
// takes (32, 64, 128, 256: the decoded tiles of D 512 leave no room for a query block).
bool rr_bank_scores_f16_plaid_dim_ok(int D);
// rr_bank_scores_f16_form / rr_bank_scores_f16_plaid_form: what the two launches above and below choose for (nq, Lq, D), and nothing
// else: the block's column tiles nt, the tiles of one query in a pass tp (the kernel instantiated is <nt, tp>), the passes over a
// query; hipErrorInvalidValue for a shape the launch refuses.  The launches call them (rr_op_bank_scores_f16_form reads them out).
hipError_t rr_bank_scores_f16_form(int nq, int Lq, int D, int* nt_out, int* tp_out, int* passes_out);
hipError_t rr_bank_scores_f16_plaid_form(int nq, int Lq, int D, int* nt_out, int* tp_out, int* passes_out);
hipError_t rr_launch_bank_scores_f16_plaid(const rr_bank_slot* table, int n, int nq, int Lq, int D, const float* query_li, const rr_bank_view& bank,
                                           float* out, hipStream_t st);
// The list-driven form of the filtered exact search (rr_bank_search_filtered_sparse), stage by stage.
// rr_launch_filter_compact (bank_ivf.hip): cand [filter.rows][n] = the range-relative passages of [filter.first, filter.first + n) whose
// bit is set, ascending, cnt [filter.rows] their numbers; a workgroup per row, no atomics.
// rr_launch_bank_search_scores_places (bank_search.hip): the MaxSim of query q against the passages cand[r][0 .. cnt[r]) (r = 0 if
// rows == 1, else q) to those places of the compact out [nq][pitch]; nothing behind a count is read or written.
// rr_launch_topk_select_counted: rr_launch_topk_select over the first cnt[r] places of the compact rows, with rr_launch_list_select's
// ending: the -inf scorers dropped, add + cand[r][place] (cand null: add + place), -1 / -inf behind, counts_out.  The scratch is
// rr_topk_select_scratch(n_lists, pitch, k); the counts are read on the device alone.
hipError_t rr_launch_filter_compact(const rr_passage_filter& filter, int n, int32_t* cand, int32_t* cnt, hipStream_t st);
hipError_t rr_launch_bank_search_scores_places(const rr_bank_slot* table, int n, int nq, int Lq, int D, const float* query_li,
                                               const rr_bank_view& bank, const int32_t* cand, const int32_t* cnt, int rows, int pitch,
                                               float* out, hipStream_t st);
hipError_t rr_launch_topk_select_counted(const float* scores, int n_lists, int pitch, const int32_t* cnt, const int32_t* cand, long long cand_ld,
                                         int rows, int k, int add, int32_t* tmp_a, int32_t* tmp_b, int32_t* indices_out, float* scores_out,
                                         int32_t* counts_out, hipStream_t st);
int rr_set_search_chunk(int passages);      // rr_set_tuning("search_chunk"): 4 .. 128, -1 outside
// rr_bank_merge_topk (bank_merge.hip; "THE MERGED LIST", include/rerank_mi355.h): per-part k-lists over local indices into one list
// over global indices, one workgroup per query.  rr_merge_check: what the three entry points refuse alike before anything is read
// or written (RR_OK, or the status with its sentence in msg); rr_launch_bank_merge and rr_bank_merge_host (the definition in host
// code) take arguments it has passed.
constexpr int RR_MERGE_MAX_PARTS = 64;
constexpr int RR_MERGE_MAX_ENTRIES = 8192;  // n_parts * k_in: 64 KB of keys
int rr_merge_check(const void* indices_in, const void* scores_in, const void* counts_in, long long part_stride, long long count_stride,
                   int n_parts, const int32_t* part_offsets, int n_queries, int k_in, int k, const void* indices_out, const void* scores_out,
                   const void* counts_out, const void* parts_out, char* msg, size_t msg_len);
hipError_t rr_launch_bank_merge(const int32_t* indices_in, const float* scores_in, const int32_t* counts_in, long long part_stride,
                                long long count_stride, int n_parts, const int32_t* part_offsets_host, int n_queries, int k_in, int k,
                                int32_t* indices_out, float* scores_out, int32_t* counts_out, int32_t* parts_out, hipStream_t st);
void rr_bank_merge_host(const int32_t* indices_in, const float* scores_in, const int32_t* counts_in, long long part_stride,
                        long long count_stride, int n_parts, const int32_t* part_offsets, int n_queries, int k_in, int k,
                        int32_t* indices_out, float* scores_out, int32_t* counts_out, int32_t* parts_out);
// rr_bank_remove (bank_move.hip; "REMOVING PASSAGES", include/rerank_mi355.h).  rr_bank_remove_plan is the one definition of what a
// removal does: new_index [n] (old dense index -> new, -1: removed) and the moves, the runs of surviving rows behind the first
// removed passage cut at the borders of the windows of window_rows destination rows, in order.  0, or one of the statuses below
// with nothing written (*bad_index: the index outside [0, n) or named twice).  rr_launch_bank_move_gather: the rows of one window
// ([win_dst_row, + win_rows), covered by moves_dev[0 .. n_moves)) of one array (rb bytes a row: a power of two, or a multiple of 16,
// at most 1024; src and staging 16-byte aligned) from their sources to the front of `staging`.  rr_bank_move_run: a whole plan over
// several arrays, per window and array that launch and one device-to-device copy; enqueues only.
struct rr_bank_move { int64_t window, src_row, dst_row, rows; };
struct rr_move_array { void* base; int rb; };
constexpr int RR_REMOVE_PLAN_BAD_SHAPE = 1, RR_REMOVE_PLAN_OUTSIDE = 2, RR_REMOVE_PLAN_TWICE = 3;
constexpr int RR_BANK_MOVE_KB_DEFAULT = 262144;
int rr_bank_remove_plan(const int32_t* lengths, int n, const int32_t* remove, int m, int64_t window_rows, std::vector<int32_t>* new_index,
                        std::vector<rr_bank_move>* moves, int32_t* bad_index);
bool rr_bank_move_row_bytes_ok(int rb);
hipError_t rr_launch_bank_move_gather(const rr_bank_move* moves_dev, int n_moves, long long win_dst_row, long long win_rows, const void* src,
                                      void* staging, int rb, hipStream_t st);
hipError_t rr_bank_move_run(const rr_bank_move* moves_host, size_t n_moves, const rr_bank_move* moves_dev, const rr_move_array* arrays,
                            int n_arrays, void* staging, hipStream_t st);
int rr_set_bank_move_kb(int kb);            // rr_set_tuning("bank_move_kb"): 4 .. 1048576, -1 outside
size_t rr_bank_move_staging_bytes();
// The inverted file of a compressed bank (bank_ivf.hip; "THE INVERTED FILE", include/rerank_mi355.h): offsets [n_centroids + 1] and
// pids [postings] on the device, the passages it covers and its longest list.  rr_ivf_build fills an EMPTY one over the host table
// (first, len) of P passages (it allocates and synchronises st; hipErrorOutOfMemory: an allocation failed, nothing is kept), with
// `old`, a file over the first old->passages < P of them, by extending that one (rr_bank_extend_ivf; *old is only read); *failed_step (or null) names
// the step a failure came from;
// rr_ivf_read copies it to host buffers (either may be null) and synchronises; rr_ivf_host is the definition in host code: it
// always writes offsets_out and returns the postings total, pids_out (or null) with room for pids_capacity entries.
struct rr_ivf { int64_t* offsets; int32_t* pids; int32_t passages; int64_t postings; int32_t longest; };
hipError_t rr_ivf_build(const rr_bank_view& bank, const int64_t* first, const int32_t* len, int P, hipStream_t st, rr_ivf* out,
                        const rr_ivf* old = nullptr, const char** failed_step = nullptr);
void rr_ivf_free(rr_ivf* f);
hipError_t rr_ivf_read(const rr_ivf& f, int C, int64_t* offsets_host, int32_t* pids_host, hipStream_t st);
int64_t rr_ivf_host(const int32_t* codes, const uint8_t* mask, const int32_t* lengths, int n, int C, int64_t* offsets_out, int32_t* pids_out,
                    int64_t pids_capacity);
// rr_bank_load_ivf: an EMPTY file filled from host arrays that rr_ivf_check_host (ivf_check.h) has passed (allocates, synchronises st)
hipError_t rr_ivf_load(const int64_t* offsets_host, const int32_t* pids_host, int C, int P, int32_t longest, hipStream_t st, rr_ivf* out);
// the scan of the inverted file's counts for another caller: offsets [n + 1] from counts [n], info[0] the total, info[1] the largest
hipError_t rr_launch_count_scan(const uint32_t* counts, int n, int64_t* offsets, int64_t* info, hipStream_t st);
// rr_bank_export_plaid / rr_op_bank_export_plaid (bank_export.hip): the unmasked rows of the passages table[0 .. n) back to back, a
// code and rb residual bytes each (rb a power of two in [1, 512]; resid and resid_out aligned to min(rb, 16)).  rr_export_plaid
// counts, scans, reads the row total back into *rows_out and moves: codes_out / resid_out both null is a sizing call; both given
// with capacity_rows < *rows_out writes NOTHING and still returns hipSuccess (the caller compares).  doclens_host [n], doclens_dev
// [n], offsets_dev int64 [n + 1]: each optional.  Allocates its block for the call and synchronises st.
bool rr_export_row_bytes_ok(int rb);
hipError_t rr_export_plaid(const rr_bank_slot* table, int n, const uint8_t* mask, const int32_t* codes, const uint8_t* resid, int rb,
                           int32_t* doclens_host, int32_t* doclens_dev, int64_t* offsets_dev, int32_t* codes_out, uint8_t* resid_out,
                           int64_t capacity_rows, int64_t* rows_out, hipStream_t st);
// the candidate step of rr_bank_search_plaid_ivf: per query the passages of [first, first + n) in the lists of its cells
// (cells [nq][E]) as an ascending range-relative list cand [nq][cap] with its count ccnt [nq]; -inf behind the count in a1 / a2
// [nq][cap]; bm [nq][Wn], Wn = ceil(n / 32): scratch
// filter.bits given: the bitmap is ANDed with the filter's bits of the range as it is compacted
hipError_t rr_launch_ivf_candidates(const rr_ivf& f, int C, const int32_t* cells, int E, int nq, int first, int n, uint32_t* bm, int Wn,
                                    int32_t* cand, int cap, int32_t* ccnt, float* a1, float* a2, const rr_passage_filter& filter,
                                    hipStream_t st);
// rr_bank_search_plaid and rr_bank_search_plaid_ivf (bank_search_plaid.hip): the staged, centroid-pruned search over a compressed
// bank.  The arguments of a call as its stages take them (table: the first passage of the range; indices + first), where the
// intermediates of the call lie in `scratch` (byte offsets, 16-byte aligned; rr_plaid_search_plan), and one launcher that runs one
// stage so that a caller can book each.  Eight stages with the candidates from a scan of the range: 0 - 2 the head, 3 the scan,
// 4 - 7 the tail.  Nine from the bank's inverted file: 0 - 2 the head, 3 the candidate lists (bank_ivf.hip), 4 A1 / A2 of the listed
// candidates into compact rows [nq][cap], 5 - 8 the tail over the compact rows, its last stage mapping a place in the candidate
// list back to its passage.
constexpr int RR_PLAID_SEARCH_STAGES = 8;
constexpr int RR_PLAID_IVF_SEARCH_STAGES = 9;
constexpr int RR_PLAID_SEARCH_MAX_CENTROIDS = 1 << 18;      // two bitmaps of a query in the scan's LDS: 64 KB
struct rr_plaid_search_args {
  int nq, n, first, Lq, Lqc, D, ncells, ndocs, k;
  float thr;
  const float* query_li;
  const rr_bank_slot* table;
  rr_bank_view bank;
  char* scratch;
  int32_t* indices_out;
  float* scores_out;
  int32_t* counts_out;
  rr_ivf ivf;                 // rr_bank_search_plaid_ivf alone: the bank's inverted file
  rr_passage_filter filter;   // the filtered entries alone (bits null: none): a passage whose bit is clear is no candidate
};
struct rr_plaid_search_layout {
  int stages;                 // RR_PLAID_SEARCH_STAGES or RR_PLAID_IVF_SEARCH_STAGES: which form the plan is for
  int Cp, W, k1, k2;          // centroids rounded up to 64; words of a bitmap; entries of a stage-1 / stage-2 list
  int pitch;                  // entries of a query's row of a1 / a2: n, or cap
  size_t S, pairs, ones, cells, cellbits, keepbits, a1, a2, list1, list2, cnt2, tmp_a, tmp_b, tmp_entries, total;
  // the inverted-file form alone (0 in the scan form): entries of a candidate list and of a compact score row; words of a query's
  // bitmap over the range; the bitmaps, the candidate lists and their counts
  int cap, Wn;
  size_t bm, cand, ccnt;
};
// longest: 0 for the scan form, the longest list of the bank's inverted file (> 0) for the inverted-file form
rr_plaid_search_layout rr_plaid_search_plan(int nq, int n, int C, int Lq, int Lqc, int ncells, int ndocs, int longest);
hipError_t rr_launch_plaid_search_stage(int stage, const rr_plaid_search_args& a, const rr_plaid_search_layout& l, hipStream_t st);
bool rr_plaid_prune_host(const float* S, int C, int Lqc, int s_ld, const int32_t* codes, const uint8_t* mask, const int32_t* lengths,
                         int n, int ncells, float thr, int ndocs, uint8_t* cells_out, float* a1_out, float* a2_out, int32_t* list1_out,
                         int32_t* n1_out, int32_t* list2_out, int32_t* n2_out);
bool rr_plaid_shape_ok(int nbits, int D);
// rr_bank_add_compress / rr_op_plaid_compress_rows (bank_compress.hip): embeddings -> (code, packed residual bytes).  The launch
// shape of a call and where its intermediates lie in `scratch` (16-byte aligned, `total` bytes): map [R] int64 (bank calls),
// keys [splits][R] 64-bit rank keys.  jt == 0: a shape the kernels do not take.
struct rr_compress_plan { int jt, row_blocks, splits, chunk; size_t lds, map_off, keys_off, total; };
bool rr_plaid_compress_shape_ok(int nbits, int D);
int rr_set_compress_chunk(int centroids);      // rr_set_tuning("compress_chunk"): 0 (chosen per launch) or a multiple of 16 in [16, 2^24], -1 outside
int rr_set_compress_stop_after(int stage);     // rr_set_tuning("compress_stop_after"): 1 (all) or 0 (the assignment kernel only), -1 outside
rr_compress_plan rr_plaid_compress_plan(long long R, int C, int D);
hipError_t rr_launch_plaid_compress(const rr_padded_rows& in, long long base, long long R, int D, int nbits, const uint16_t* centroids, int C,
                                    const float* cutoffs, char* scratch, const rr_compress_plan& pl, int32_t* codes, uint8_t* resid,
                                    uint8_t* mask_bytes, hipStream_t st);
// The codes alone (rr_bank_set_centroids, rr_bank_add on an fp16 bank with a centroid table): the assignment kernel over the R fp16
// rows that lie back to back at rows_f16 (the caller's first row; 64-bit offsets inside), then the maximum over the splits' keys as
// the int32 code, 4 bytes a row.  No residual is formed.  scratch: pl.total bytes (the map part unused); codes: the first row's.
hipError_t rr_launch_plaid_assign_codes(const uint16_t* rows_f16, long long R, int D, const uint16_t* centroids, int C, char* scratch,
                                        const rr_compress_plan& pl, int32_t* codes, hipStream_t st);
// rr_util_plaid_compress_rows: the definition in host code (passage_bank.hip, beside the host decoder)
bool rr_plaid_compress_rows_host(const void* rows, int rows_f16, long long n_rows, int D, const uint16_t* centroids, int C,
                                 const float* cutoffs, int nbits, int32_t* codes_out, uint8_t* resid_out);
bool rr_plaid_decode_rows_host(const uint16_t* centroids, int C, const float* weights, int nbits, int D, const int32_t* codes,
                               const uint8_t* resid, long long n_rows, uint16_t* out);
// rr_plaid_kmeans / rr_plaid_residuals (plaid_train.hip): codec training.  Where the intermediates of a k-means call lie in its
// `scratch` (16-byte aligned, `total` bytes): init_rows [C] int32 (staged by the caller), T [C][D] fp16 table, h [C up to 16] float32
// bias, A [C][D] int64 sums, n [C] counts, codes [R] int32 of the previous iteration, stats (when the caller wants none), the
// assignment's keys [splits][R].  assign: the launch shape of the assignment (rr_plaid_compress_plan); assign.jt == 0: a shape the
// kernels do not take.
struct rr_kmeans_plan { rr_compress_plan assign; size_t init_off, T_off, h_off, A_off, n_off, codes_off, stats_off, keys_off, total; };
bool rr_plaid_train_shape_ok(int D);           // D a power of two in [16, 512]
int rr_set_kmeans_stop_after(int stage);       // rr_set_tuning("kmeans_stop_after"): 2 (all), 1 (assignment + accumulation), 0 (assignment), -1 outside
rr_kmeans_plan rr_plaid_kmeans_plan(long long R, int C, int D, int niters);
hipError_t rr_launch_plaid_kmeans(const void* rows, int rows_f16, long long R, int D, int C, int niters, unsigned long long seed,
                                  char* scratch, const rr_kmeans_plan& pl, uint16_t* centroids_out, int32_t* counts_out,
                                  int32_t* stats_out, hipStream_t st);
hipError_t rr_launch_plaid_residuals(const void* rows, int rows_f16, long long R, int D, const uint16_t* centroids, int C, char* scratch,
                                     const rr_compress_plan& pl, int32_t* codes_out, float* resid_out, hipStream_t st);
// rr_util_plaid_kmeans: the definition in host code
bool rr_plaid_kmeans_host(const void* rows, int rows_f16, long long R, int D, const int32_t* init_rows, int C, int niters,
                          unsigned long long seed, uint16_t* centroids_out, int32_t* counts_out, int32_t* stats_out);
