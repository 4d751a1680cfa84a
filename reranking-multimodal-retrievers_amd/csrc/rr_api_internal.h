// librerank_mi355 — what the two units of the C ABI share (rr_api.hip: the forwards; bank_api.hip: the passage bank and PLAID):
// the handle and the bank, error reporting, profiling, the grow-only blocks and the staging slots.  Internal: not installed.
#pragma once
#include "../../include/rerank_mi355_diag.h"   // product ABI (rerank_mi355.h) + the diagnostic entry points
#include "rr_common.h"

#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <algorithm>
#include <cstring>
#include <exception>
#include <functional>
#include <limits>
#include <map>
#include <new>
#include <string>
#include <vector>

struct HostTensor {
  std::vector<int64_t> shape;
  std::vector<float> data;
};

// Per-BertLayer device weights (fused/packed forms).
struct LayerW {
  bf16_t *wqkv = nullptr, *wo = nullptr, *w1 = nullptr, *w2 = nullptr;
  float *bqkv = nullptr, *bo = nullptr, *b1 = nullptr, *b2 = nullptr;
  float *ln1g = nullptr, *ln1b = nullptr, *ln2g = nullptr, *ln2b = nullptr;
  // LayerNorm folded into the consumer GEMM (gemm_bf16.hip LnResid): W' = 16bit(W * gamma), c = row sums of W',
  // d = W beta + b.  wqkv_f folds the PREVIOUS layer's output LayerNorm (null for the first layer of a stack), w1_f this
  // layer's attention-output LayerNorm.
  bf16_t *wqkv_f = nullptr, *w1_f = nullptr;
  float *cqkv_f = nullptr, *dqkv_f = nullptr, *c1_f = nullptr, *d1_f = nullptr;
  // fp8 mode (cfg.fp8): e4m3 weights, one scale per output channel — int8 codes when the handle's "q8_format" is 1 (w2_8 null:
  // FFN-down keeps 16-bit operands there)
  uint8_t *wqkv8 = nullptr, *w1_8 = nullptr, *w2_8 = nullptr;
  float *sqkv = nullptr, *s1 = nullptr, *s2 = nullptr;
  // int8: the quantising LayerNorms' private affine gamma / s, beta / s (host_smooth_scales); residuals keep ln1g / ln2g
  float *ln1g_q = nullptr, *ln1b_q = nullptr, *ln2g_q = nullptr, *ln2b_q = nullptr;
  // cross-attention (transformer mapping network only)
  bf16_t *wq_c = nullptr, *wkv_c = nullptr, *wo_c = nullptr;
  float *bq_c = nullptr, *bkv_c = nullptr, *bo_c = nullptr, *lncg = nullptr, *lncb = nullptr;
};

struct ProfEvent {
  hipEvent_t a, b;
  int kclass;
  int start;      // >= 0: this launch starts where launch `start` of the pool ended (its `b` event; `a` was not recorded), -1: at its own `a`
};

// Options of a handle that change which arithmetic a forward runs (include/rerank_mi355.h, rr_set_option)
enum RrOption { RR_OPT_LN_LITE = 0, RR_OPT_LN_FOLD, RR_OPT_CE_CLS_ONLY, RR_OPT_FP8_FFN_DOWN, RR_OPT_RESID_SPLIT, RR_OPT_ATTN_FIXED_REF,
                RR_OPT_FP8_FIRST_LAYER, RR_OPT_FP8_QKV, RR_OPT_RESID_LO8, RR_OPT_Q8_FORMAT, RR_OPT_COUNT };
static const char* const kOptionKeys[RR_OPT_COUNT] = {"ln_lite", "ln_fold", "ce_cls_only", "fp8_ffn_down", "resid_split", "attn_fixed_ref",
                                                      "fp8_first_layer", "fp8_qkv", "resid_lo8", "q8_format"};

struct rr_model {
  rr_config cfg;
  int dt = 0;                       // 16-bit operand dtype: 0 bf16, 1 fp16 (cfg.compute_dtype)
  std::string err;
  bool finalized = false;
  std::map<std::string, std::vector<int64_t>> required;   // name -> expected shape
  std::vector<std::string> required_order;
  std::map<std::string, HostTensor> host;                  // staged until finalize
  std::vector<void*> dev_allocs;

  // device weights
  float *word = nullptr, *pos = nullptr, *type = nullptr, *emb_g = nullptr, *emb_b = nullptr;
  std::vector<LayerW> text_layers, ce_layers, map_layers;
  bf16_t* w_li = nullptr;                                   // context_text_encoder_linear [D,H]
  bf16_t *w_vp0 = nullptr, *w_vp2 = nullptr, *w_min = nullptr, *w_mout = nullptr;
  float *b_vp0 = nullptr, *b_vp2 = nullptr, *b_min = nullptr, *b_mout = nullptr;
  bf16_t* w_cemap = nullptr;
  float* b_cemap = nullptr;
  float *ce_pos = nullptr, *ce_type = nullptr, *ce_emb_g = nullptr, *ce_emb_b = nullptr;
  float *cls1_w = nullptr, *cls1_b = nullptr, *cls2_w = nullptr, *cls2_b = nullptr;
  // PreFLMR attention-fusion bias (grow-only, only when rr_forward_joint_fusion is used)
  float* adj = nullptr;
  size_t adj_cap = 0;
  // late-interaction score block [n][Lc][Lq] of the *_fusion_li forwards (grow-only; rr_reserve with_fusion = 2)
  float* li_sc = nullptr;
  size_t li_sc_cap = 0;
  // what rr_forward_interaction_bank's gather writes beside the 16-bit rows (grow-only): the float mask rows of the call, and with
  // fusion_from_li the float32 copies of its query / context rows that li_scores reads
  char* bank_blk = nullptr;
  size_t bank_blk_cap = 0;
  // rr_bank_search (grow-only): the score of every (query, passage) of the call, then the two survivor buffers of the selection
  char* search_blk = nullptr;
  size_t search_blk_cap = 0;
  // rr_plaid_kmeans / rr_plaid_residuals (grow-only): the table, the sums and the assignment's keys of a call (rr_kmeans_plan)
  char* train_blk = nullptr;
  size_t train_blk_cap = 0;
  // rr_bank_search_plaid shares that block; what its LAST call left there (rr_bank_search_plaid_tap), until the next search
  rr_plaid_search_args plaid_last{};
  rr_plaid_search_layout plaid_last_layout{};
  bool plaid_last_ok = false;
  // CLIP ViT (optional)
  std::vector<LayerW> vit_layers;
  bf16_t* vit_wpatch = nullptr;                             // [Vh, Kp] patch convolution, zero-padded to Kp
  float *vit_cls = nullptr, *vit_pos = nullptr, *vit_pre_g = nullptr, *vit_pre_b = nullptr;
  int vit_kp = 0;

  // workspace (grow-only)
  char* ws = nullptr;
  size_t ws_cap = 0;
  const float* cls_rows = nullptr;     // set by run_cross_encoder when its last layer ran on the CLS rows only: [n, Hc] fp32 (else null)
  int* range_flag_host = nullptr;      // pinned copy of range_flag, refreshed asynchronously at the end of every forward (sticky RR_ERR_RANGE)
  int* range_flag = nullptr;           // device word raised by ln_finalize when a residual row nears the fp16 range (rr_activation_range_flag)
  int padded_S = 0;                    // rr_set_padded_seq_len: the padded text length whose cross-encoder positions a shorter forward keeps (0 = off)
  // Per-handle numerics options (rr_set_option): -1 = follow the process-wide diagnostic switch of the same name (rr_set_tuning),
  // 0 / 1 / ... = pinned for this handle.  Two handles of one process may differ (no global state on the path).
  int opt[RR_OPT_COUNT] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
  int q8_fmt = -1;                     // "q8_format" as latched by rr_finalize_weights (-1 before): 0 e4m3, 1 int8 weights were packed
  bool pinned_blocks = false;          // a stream capture was seen on this handle: outgrown blocks are retired, not freed
  std::vector<void*> retired;          // outgrown workspace / bias blocks that a captured graph may still reference; freed by rr_destroy

  // last-forward taps
  bool debug = false;
  float* tap_text = nullptr;
  size_t tap_text_elems = 0;
  const bf16_t* tap_li = nullptr;
  size_t tap_li_elems = 0;
  const float* tap_ce = nullptr;
  size_t tap_ce_elems = 0;
  hipStream_t last_stream = nullptr;

  // profiling
  bool profiling = false;
  std::vector<ProfEvent> ev_pool;
  size_t ev_used = 0;
  // Chained events: a launch that directly follows another profiled launch on the same stream takes that launch's end event as
  // its start — one hipEventRecord per launch instead of two (an event costs the step ~3 us of idle queue: 274 of them were
  // 0.95 % of the c3 step, gpurun log in docs/rounds/r05.md).  Anything else the library enqueues in between (RR_HIP: copies,
  // memsets) and every new API call break the chain, so foreign work is never billed to a kernel class.
  int prof_chain = -1;
  hipStream_t prof_chain_st = nullptr;
  rr_profile prof{};

  // rr_assemble_pairs / rr_assemble_joint: two staging slots for the checked descriptors (pinned host -> device), used in turn.
  // `done` is recorded behind the assembly launch that read the slot: the slot is refilled only after it completed.
  struct AsmSlot { void* host = nullptr; void* dev = nullptr; size_t cap = 0; hipEvent_t done = nullptr; };
  AsmSlot asm_slot[2];
  int asm_next = 0;
};

// rr_bank_* (include/rerank_mi355.h): a device store of passages, rows back to back (appended; rr_bank_remove compacts).  rows [capacity_rows][D] fp16 bits, one mask byte
// per row, and the host table (first row, length) per passage.  Its own staging slots: rr_bank_add belongs to no handle.
// A compressed bank (rr_bank_create_plaid, nbits != 0) holds per row a centroid code and D * nbits / 8 residual bytes in place of
// `rows`, and the codec's tables: centroids [n_centroids][D] fp16 bits, weights [2^nbits] float32.
struct rr_bank {
  int device = 0, D = 0;
  int64_t cap_rows = 0, used_rows = 0;
  int32_t max_passages = 0;
  uint16_t* rows = nullptr;
  uint8_t* mask = nullptr;
  int nbits = 0, n_centroids = 0;
  int32_t* codes = nullptr;
  uint8_t* resid = nullptr;
  uint16_t* centroids = nullptr;
  float* weights = nullptr;
  size_t resid_row_bytes() const { return (size_t)D / 8 * (size_t)nbits; }
  // an fp16 bank that rr_bank_set_centroids gave a table: nbits == 0, `rows` AND codes [capacity_rows] / centroids / n_centroids
  // (no resid, no weights); has_codes(): what the pruned searches and the inverted file ask of a bank
  bool coded() const { return !nbits && codes != nullptr; }
  bool has_codes() const { return nbits != 0 || codes != nullptr; }
  std::vector<int64_t> first;
  std::vector<int32_t> len;
  // the device copy of (first, len) that rr_bank_search's kernel walks: 16 bytes per passage, allocated and brought up to date
  // by the first search after an add (table_n passages of it are current); nothing else reads it
  rr_bank_slot* table = nullptr;
  size_t table_cap = 0, table_n = 0;
  // rr_bank_add_compress: the codec's bucket cutoffs [2^nbits - 1] on the device (rr_bank_set_plaid_cutoffs; null until then) and
  // the grow-only scratch of a call (row map and the splits' rank keys, rr_compress_plan)
  float* cutoffs = nullptr;
  bool has_cutoffs = false;
  char* cscratch = nullptr;
  size_t cscratch_cap = 0;
  // rr_bank_build_ivf: the inverted file over the first ivf.passages passages (0: none); rr_bank_clear drops it
  rr_ivf ivf{};
  std::string err;
  rr_model::AsmSlot slot[2];
  int next = 0;
};
// the one place an rr_bank becomes the row source the launchers take (rr_common.h)
inline rr_bank_view bank_view(const rr_bank* b) {
  return rr_bank_view{b->nbits, b->n_centroids, b->rows, b->codes, b->resid, b->centroids, b->weights, b->mask};
}

inline int fail(rr_model* m, int code, const char* fmt, ...) noexcept {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (m) { try { m->err = buf; } catch (...) {} }
  return code;
}

// No C++ exception crosses the C ABI: every extern "C" entry point runs its body through guarded().  bad_alloc (host
// vectors/maps/strings of the weight staging, the event pool, ...) -> RR_ERR_OOM, anything else -> RR_ERR_BAD_ARG with the
// message kept for rr_last_error().
template <class R = int, class F>
R guarded(rr_model* m, F&& body) noexcept {
  if (m) m->prof_chain = -1;                       // events never chain across API calls (the caller may have used the stream)
  try {
    return body();
  } catch (const std::bad_alloc&) {
    return (R)fail(m, RR_ERR_OOM, "out of host memory");
  } catch (const std::exception& e) {
    return (R)fail(m, RR_ERR_BAD_ARG, "internal error: %s", e.what());
  } catch (...) {
    return (R)fail(m, RR_ERR_BAD_ARG, "internal error (unknown exception)");
  }
}

#define RR_HIP(m, call)                                                                        \
  do {                                                                                         \
    if (m) (m)->prof_chain = -1;                /* whatever this enqueues is not part of the next profiled launch */ \
    hipError_t e_ = (call);                                                                    \
    if (e_ != hipSuccess)                                                                      \
      return fail(m, e_ == hipErrorOutOfMemory ? RR_ERR_OOM : RR_ERR_HIP, "%s failed: %s", #call, \
                  hipGetErrorString(e_));                                                      \
  } while (0)

struct Prof {
  rr_model* m;
  hipStream_t st;
  int idx = -1;
  Prof(rr_model* m_, hipStream_t st_, int kclass, double flops, double bytes) : m(m_), st(st_) {
    if (!m->profiling) return;
    if (m->ev_used == m->ev_pool.size()) {
      ProfEvent e{};
      if (hipEventCreate(&e.a) != hipSuccess || hipEventCreate(&e.b) != hipSuccess) return;
      m->ev_pool.push_back(e);
    }
    const bool chained = m->prof_chain >= 0 && m->prof_chain_st == st && (size_t)m->prof_chain + 1 == m->ev_used;
    idx = (int)m->ev_used++;
    m->ev_pool[idx].kclass = kclass;
    m->ev_pool[idx].start = chained ? m->prof_chain : -1;
    m->prof.launches[kclass] += 1;
    m->prof.flops[kclass] += flops;
    m->prof.bytes[kclass] += bytes;
    if (!chained) (void)hipEventRecord(m->ev_pool[idx].a, st);
  }
  ~Prof() {
    if (idx < 0) return;
    const bool ok = hipEventRecord(m->ev_pool[idx].b, st) == hipSuccess;
    m->prof_chain = ok ? idx : -1;
    m->prof_chain_st = st;
  }
};

#define RR_RUN(m, st, kclass, flops, bytes, call)                                              \
  do {                                                                                         \
    hipError_t e_;                                                                             \
    {                                                                                          \
      Prof p_(m, st, kclass, flops, bytes);                                                    \
      e_ = (call);                                                                             \
    }                                                                                          \
    if (e_ != hipSuccess) return fail(m, RR_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
  } while (0)

#define RR_TRY(x)            \
  do {                       \
    int rc_ = (x);           \
    if (rc_ != RR_OK) return rc_; \
  } while (0)

inline float host_bf2f(uint16_t b) {
  uint32_t u = ((uint32_t)b) << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
inline float host_h2f(uint16_t h) {
  const uint32_t s = (h >> 15) & 1, e = (h >> 10) & 31, m = h & 1023;
  float v;
  if (e == 0) v = ldexpf((float)m, -24);
  else if (e == 31) v = m ? NAN : INFINITY;
  else v = ldexpf((float)(m | 1024), (int)e - 25);
  return s ? -v : v;
}

// defined in rr_api.hip (set_plaid_stop_after: in bank_api.hip)
int capture_guard(rr_model* m, hipStream_t st, const char* sentence, const char* what);
int release_block(rr_model* m, void* p, hipStream_t st);
int check_rows(rr_model* m, const char* what, long long n, int T);
hipError_t stage_slot(rr_model::AsmSlot& a, const void* data, size_t bytes, size_t min_cap, hipStream_t st);
int asm_stage(rr_model* m, const char* what, const void* data, size_t bytes, hipStream_t st, void** dev);
int asm_done(rr_model* m, hipStream_t st);
int set_plaid_stop_after(bool ivf, int value);
int set_sparse_stop_after(int value);
int set_f16_stop_after(int value);

const char* const CAP_GROWS = "%s would have to grow during stream capture; call rr_reserve for the largest shape before capturing";
const char* const CAP_STAGES = "%s cannot be captured into a graph (it stages its descriptors from the host)";
// a grow-only device block of the handle (ws, adj, li_sc, search_blk, bank_blk); `what` names it in the refusal
template <class T>
int ensure_block(rr_model* m, T*& ptr, size_t& cap, size_t bytes, hipStream_t st, const char* what) {
  if (bytes <= cap) return RR_OK;
  if (const int rc = capture_guard(m, st, CAP_GROWS, what)) {
    m->pinned_blocks = true;
    return rc;
  }
  if (ptr) {
    RR_TRY(release_block(m, ptr, st));
    ptr = nullptr;
    cap = 0;
  }
  RR_HIP(m, hipMalloc((void**)&ptr, bytes));
  cap = bytes;
  return RR_OK;
}

// What every call that reads a bank through a handle asks first: an interaction model, bank and handle on one device, rows of li_dim.
inline int bank_usable(rr_model* m, const char* what, const rr_bank* b) {
  const rr_config& c = m->cfg;
  if (c.model_kind == RR_MODEL_FULL_CONTEXT) return fail(m, RR_ERR_BAD_ARG, "%s on a full-context model", what);
  if (b->device != c.device) return fail(m, RR_ERR_BAD_ARG, "%s: the bank lives on device %d, the handle on %d", what, b->device, c.device);
  if (b->D != c.li_dim) return fail(m, RR_ERR_BAD_SHAPE, "%s: the bank holds rows of %d, the handle's li_dim is %d", what, b->D, c.li_dim);
  return RR_OK;
}
// Pair i of a call, (passage pi of the bank, query qi of n_queries), as the checked descriptor the kernels take.  The passage must
// fit `limit` rows; limit_is: how the caller's message names that limit.  Inlined: it runs once per pair of every call.
__attribute__((always_inline)) inline int bank_checked_pair(rr_model* m, const char* what, const rr_bank* b, long long i, int32_t pi, int32_t qi, int n_queries,
                                    int limit, const char* limit_is, rr_bank_pair* out) {
  const long long held = (long long)b->first.size();
  if (pi < 0 || pi >= held) return fail(m, RR_ERR_BAD_SHAPE, "%s: pair %lld names passage %d, the bank holds %lld", what, i, pi, held);
  if (qi < 0 || qi >= n_queries) return fail(m, RR_ERR_BAD_SHAPE, "%s: pair %lld names query %d of %d", what, i, qi, n_queries);
  const int32_t len = b->len[(size_t)pi];
  if (len > limit) return fail(m, RR_ERR_BAD_SHAPE, "%s: pair %lld: passage %d holds %d rows, %s %d", what, i, pi, len, limit_is, limit);
  *out = rr_bank_pair{b->first[(size_t)pi], len, qi};
  return RR_OK;
}
