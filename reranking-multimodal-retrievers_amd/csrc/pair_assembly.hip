// Pair-input assembly on the device (rr_assemble_pairs, include/rerank_mi355.h): the int64 input_ids / attention_mask /
// token_type_ids rows rr_forward_packed reads, expanded from the compact token pool of rr_tok_prepare_compact.  The row of a
// pair is what rr_tok_prepare_pairs writes (csrc/pair_tokenizer.cpp): [CLS] q[:la] [SEP] c[:lb] [SEP], mask 1 on those
// la + lb + 3 tokens, type 1 on c[:lb] and the closing [SEP], then [PAD] / mask 0 / type 0 up to the segment's length.
// Memory only: one workgroup per packed pair, the query's ids are read by all K pairs of the query (from L2), every store is a
// coalesced 8-byte run.  The host has checked every descriptor against the pool and its segment before the launch; the bound
// test on the pool index below keeps a bad descriptor from ever reading outside it all the same.
//
// The joint rows of rr_forward_joint_packed (rr_assemble_joint) come from the same kind of pool: per pair the query's ql ids
// and ql mask values as the dataset gave them, then the first ctx_w entries of t[0:m] [SEP] [PAD]... with mask 1 on t and the
// [SEP] (RerankModel.forward's cat(q, ctx[:, 2 : 2 - ql]), rerank_model.py:191-222), cut to the segment's length.
#include "rr_common.h"

namespace {

__global__ __launch_bounds__(256) void assemble_pairs_kernel(const int32_t* __restrict__ pool, long long pool_len,
                                                             const rr_asm_pair* __restrict__ pairs, long long cls, long long sep,
                                                             long long pad, int64_t* __restrict__ ids, int64_t* __restrict__ am,
                                                             int64_t* __restrict__ tt) {
  const rr_asm_pair d = pairs[blockIdx.x];
  const int q_end = 1 + d.la, c_beg = q_end + 1, c_end = c_beg + d.lb;
  const size_t base = (size_t)(unsigned)d.row0;
  for (int j = threadIdx.x; j < d.len; j += blockDim.x) {
    long long id = pad, src = -1;
    int64_t m = 1, t = 0;
    if (j == 0) id = cls;
    else if (j < q_end) src = (long long)d.qoff + (j - 1);
    else if (j == q_end) id = sep;
    else if (j < c_end) { src = (long long)d.coff + (j - c_beg); t = 1; }
    else if (j == c_end) { id = sep; t = 1; }
    else m = 0;
    if (src >= 0) id = src < pool_len ? (long long)pool[src] : pad;
    ids[base + j] = id;
    am[base + j] = m;
    if (tt) tt[base + j] = t;
  }
}

__global__ __launch_bounds__(256) void assemble_joint_kernel(const int32_t* __restrict__ pool, long long pool_len,
                                                             const rr_asm_joint* __restrict__ pairs, long long sep, long long pad,
                                                             int64_t* __restrict__ ids, int64_t* __restrict__ am) {
  const rr_asm_joint d = pairs[blockIdx.x];
  const int kept = d.m < d.ctx_w ? d.m : d.ctx_w;           // context tokens inside the joint row's window
  const int c_end = d.ql + kept;
  const bool has_sep = d.m < d.ctx_w;                        // a passage that fills the window loses its [SEP]
  const size_t base = (size_t)(unsigned)d.row0;
  for (int j = threadIdx.x; j < d.len; j += blockDim.x) {
    long long id = pad;
    int64_t mk = 0;
    if (j < d.ql) {
      const long long src = (long long)d.qoff + j, msrc = src + d.ql;
      id = src < pool_len ? (long long)pool[src] : pad;
      mk = msrc < pool_len ? (int64_t)pool[msrc] : 0;
    } else if (j < c_end) {
      const long long src = (long long)d.coff + (j - d.ql);
      id = src < pool_len ? (long long)pool[src] : pad;
      mk = 1;
    } else if (j == c_end && has_sep) {
      id = sep;
      mk = 1;
    }
    ids[base + j] = id;
    am[base + j] = mk;
  }
}

}  // namespace

hipError_t rr_launch_assemble_pairs(const int32_t* pool, long long pool_len, const rr_asm_pair* pairs, int n_pairs, long long cls,
                                    long long sep, long long pad, int64_t* ids, int64_t* am, int64_t* tt, hipStream_t st) {
  if (n_pairs <= 0 || pool_len < 0 || !pairs || !ids || !am) return hipErrorInvalidValue;
  hipLaunchKernelGGL(assemble_pairs_kernel, dim3((unsigned)n_pairs), dim3(256), 0, st, pool, pool_len, pairs, cls, sep, pad, ids,
                     am, tt);
  return hipGetLastError();
}

hipError_t rr_launch_assemble_joint(const int32_t* pool, long long pool_len, const rr_asm_joint* pairs, int n_pairs, long long sep,
                                    long long pad, int64_t* ids, int64_t* am, hipStream_t st) {
  if (n_pairs <= 0 || pool_len < 0 || !pairs || !ids || !am) return hipErrorInvalidValue;
  hipLaunchKernelGGL(assemble_joint_kernel, dim3((unsigned)n_pairs), dim3(256), 0, st, pool, pool_len, pairs, sep, pad, ids, am);
  return hipGetLastError();
}
