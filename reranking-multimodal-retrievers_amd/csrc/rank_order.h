// The ONE rank order of the bank searches (bank_search.hip, bank_search_plaid.hip), that of torch.sort(descending=True,
// stable=True): NaN ahead of every number, higher score first, equal scores (+0 == -0) by ascending index.  Score and index are
// packed into one 64-bit key, an order-preserving image of the float above and the complement of the index below: a LARGER key
// ranks first, keys of distinct indices are distinct, and 0 is no entry's key (it pads, and ranks behind every entry).  So a
// sort or a maximum over keys has one possible result: no atomics, nothing depends on scheduling.  Host and device read the same
// definition (rr_plaid_prune_host orders its lists by it).  The bitonic network over keys in LDS is NOT here: as one
// __forceinline__ function template it changed the schedule of topk_select_kernel (one instruction more, other compare forms) and
// the selection stages measured 3 .. 5 % slower (profiles/search_core_ab.json.log, first job), so each selection kernel keeps its
// copy.  Beside the key: a 64-bit value read as wave-uniform, as every kernel that walks the passage table does.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace {

// the order-preserving image of a score: NaN above +inf, -0 as +0, then the usual sign flip; never 0
__host__ __device__ __forceinline__ uint32_t rank_score_image(float s) {
  if (s != s) return 0xffffffffu;
  uint32_t u = __builtin_bit_cast(uint32_t, s);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ __forceinline__ unsigned long long rank_key(float s, uint32_t idx) {
  return ((unsigned long long)rank_score_image(s) << 32) | (unsigned long long)(0xffffffffu - idx);
}
__host__ __device__ __forceinline__ uint32_t rank_key_index(unsigned long long key) { return 0xffffffffu - (uint32_t)key; }

// a 64-bit value every lane of the wave holds alike (a table entry's first row), moved to scalar registers
__device__ __forceinline__ long long uniform_i64(int64_t v) {
  return (long long)(((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
                     (uint32_t)__builtin_amdgcn_readfirstlane((int)v));
}

}  // namespace
