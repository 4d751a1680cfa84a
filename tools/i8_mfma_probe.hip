// Probe: the int8 MFMA forms gemm_fp8.hip uses with I8 = true, on exact integer data (gfx950).
//   hipcc --offload-arch=gfx950 -O2 tools/i8_mfma_probe.hip -o tools/bin/i8_probe && tools/bin/i8_probe
// What the kernels rely on: each lane's 32-byte fragment of a 64-deep k-step (A and B loaded by the SAME pattern: lane l,
// row/col l&31, bytes [32 (l>>5), +32) for 32x32; row/col l&15, bytes [32 (l>>4), +32) of a 128-deep step for 16x16) feeds
// two i8 MFMAs as its two 16-byte halves.  Whatever order the hardware gives k inside a half, A and B see the same one, so the
// two products sum every k exactly once.  Checked here: (1) that split against the exact int64 product (both shapes, random
// full-range codes -127..127 and an asymmetric B), (2) the natural map by itself, for the record: lane l holds
// A[row][k = 16 (l>>5) + j] (32x32x32) / A[row][k = 16 (l>>4) + j] (16x16x64), j = 0..15 in byte order, likewise B; C/D as every
// 32x32 / 16x16 MFMA.  Prints one line per check and exits non-zero on any mismatch.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <vector>

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(16))) int i32x16;

// 32x32, one 64-deep k-step.  A [32][64], B stored [n][k] = [32][64].  split = 1: the kernels' two-halves pattern,
// 0: one 32x32x32 MFMA over k < 32 with the natural-map hypothesis (lane half h: bytes [16 h, +16)).
__global__ void probe32(const int8_t* A, const int8_t* B, int* D, int split) {
  const int l = threadIdx.x, r = l & 31, h = l >> 5;
  i32x16 c;
  for (int i = 0; i < 16; ++i) c[i] = 0;
  if (split) {
    const i32x4* ap = (const i32x4*)(A + r * 64 + 32 * h);
    const i32x4* bp = (const i32x4*)(B + r * 64 + 32 * h);
    c = __builtin_amdgcn_mfma_i32_32x32x32_i8(ap[0], bp[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_i32_32x32x32_i8(ap[1], bp[1], c, 0, 0, 0);
  } else {
    c = __builtin_amdgcn_mfma_i32_32x32x32_i8(*(const i32x4*)(A + r * 64 + 16 * h), *(const i32x4*)(B + r * 64 + 16 * h), c, 0, 0, 0);
  }
  for (int i = 0; i < 16; ++i) D[((i & 3) + 8 * (i >> 2) + 4 * h) * 32 + r] = c[i];     // row, col = r
}

// 16x16, one 128-deep k-step.  A [16][128], B [16][128].  split = 0: one 16x16x64 MFMA over k < 64 (lane group g = l>>4:
// bytes [16 g, +16)).
__global__ void probe16(const int8_t* A, const int8_t* B, int* D, int split) {
  const int l = threadIdx.x, r = l & 15, g = l >> 4;
  i32x4 c = {0, 0, 0, 0};
  if (split) {
    const i32x4* ap = (const i32x4*)(A + r * 128 + 32 * g);
    const i32x4* bp = (const i32x4*)(B + r * 128 + 32 * g);
    c = __builtin_amdgcn_mfma_i32_16x16x64_i8(ap[0], bp[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_i32_16x16x64_i8(ap[1], bp[1], c, 0, 0, 0);
  } else {
    c = __builtin_amdgcn_mfma_i32_16x16x64_i8(*(const i32x4*)(A + r * 128 + 16 * g), *(const i32x4*)(B + r * 128 + 16 * g), c, 0, 0, 0);
  }
  for (int i = 0; i < 4; ++i) D[(4 * g + i) * 16 + r] = c[i];                            // row = 4 (l>>4) + reg, col = l&15
}

static int check(const char* what, const std::vector<int8_t>& A, const std::vector<int8_t>& B, int n, int kd, int kuse,
                 const std::vector<int>& out) {
  int bad = 0, badT = 0;
  for (int m = 0; m < n; ++m)
    for (int c = 0; c < n; ++c) {
      long long ref = 0, refT = 0;
      for (int k = 0; k < kuse; ++k) { ref += (long long)A[m * kd + k] * B[c * kd + k]; refT += (long long)A[c * kd + k] * B[m * kd + k]; }
      if (out[m * n + c] != ref) ++bad;
      if (out[m * n + c] != refT) ++badT;
    }
  printf("%-44s mismatches %4d / %d (as D^T: %d)\n", what, bad, n * n, badT);
  return bad;
}

int main() {
  uint32_t s = 12345;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (int)((s >> 8) % 255) - 127; };
  int fails = 0;
  for (int n : {32, 16}) {
    const int kd = n == 32 ? 64 : 128;
    std::vector<int8_t> A(n * kd), B(n * kd);
    std::vector<int> out(n * n);
    for (int i = 0; i < n * kd; ++i) A[i] = (int8_t)rnd();
    for (int c = 0; c < n; ++c)                                          // asymmetric B: column c's codes carry c
      for (int k = 0; k < kd; ++k) B[c * kd + k] = (int8_t)(((k * 7 + c * 3) % 255) - 127);
    int8_t *dA, *dB;
    int* dD;
    hipMalloc(&dA, A.size()); hipMalloc(&dB, B.size()); hipMalloc(&dD, out.size() * 4);
    hipMemcpy(dA, A.data(), A.size(), hipMemcpyHostToDevice);
    hipMemcpy(dB, B.data(), B.size(), hipMemcpyHostToDevice);
    for (int split : {1, 0}) {
      if (n == 32) hipLaunchKernelGGL(probe32, dim3(1), dim3(64), 0, 0, dA, dB, dD, split);
      else hipLaunchKernelGGL(probe16, dim3(1), dim3(64), 0, 0, dA, dB, dD, split);
      if (hipMemcpy(out.data(), dD, out.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) { printf("device error\n"); return 2; }
      char what[96];
      snprintf(what, sizeof what, "%dx%d %s", n, n, split ? "two halves of the 32-byte fragment" : "natural map, one MFMA");
      const int b = check(what, A, B, n, kd, split ? kd : kd / 2, out);
      fails += split ? b : 0;       // the kernels depend on the split form only; the natural map is recorded
    }
    hipFree(dA); hipFree(dB); hipFree(dD);
  }
  printf(fails ? "FAIL\n" : "OK\n");
  return fails ? 1 : 0;
}
