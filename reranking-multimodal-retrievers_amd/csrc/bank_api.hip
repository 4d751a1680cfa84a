// librerank_mi355 — the passage bank and the PLAID host side of the C ABI (see include/rerank_mi355.h for the contract):
// rr_bank_*, rr_plaid_*, the bank searches and their diagnostic rr_op_* / rr_util_* entry points.  rr_api.hip holds the forwards.
#include "rr_api_internal.h"
#include "ivf_check.h"

// ---- rr_bank_* (include/rerank_mi355.h)
static int bfail(rr_bank* b, int code, const char* fmt, ...) noexcept {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (b) { try { b->err = buf; } catch (...) {} }
  return code;
}
#define RR_BHIP(b, call)                                                                                                  \
  do {                                                                                                                    \
    hipError_t e_ = (call);                                                                                               \
    if (e_ != hipSuccess)                                                                                                 \
      return bfail(b, e_ == hipErrorOutOfMemory ? RR_ERR_OOM : RR_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
  } while (0)

// capture_guard for the calls that report through the bank
static int bank_capture_guard(rr_bank* b, hipStream_t st, const char* sentence, const char* what) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs == hipStreamCaptureStatusNone) return RR_OK;
  return bfail(b, RR_ERR_BAD_ARG, sentence, what);
}

static void bank_free(rr_bank* b) {
  if (b->rows) (void)hipFree(b->rows);
  if (b->mask) (void)hipFree(b->mask);
  if (b->codes) (void)hipFree(b->codes);
  if (b->resid) (void)hipFree(b->resid);
  if (b->centroids) (void)hipFree(b->centroids);
  if (b->weights) (void)hipFree(b->weights);
  if (b->table) (void)hipFree(b->table);
  if (b->cutoffs) (void)hipFree(b->cutoffs);
  if (b->cscratch) (void)hipFree(b->cscratch);
  rr_ivf_free(&b->ivf);
  for (auto& a : b->slot) {
    if (a.host) (void)hipHostFree(a.host);
    if (a.dev) (void)hipFree(a.dev);
    if (a.done) (void)hipEventDestroy(a.done);
  }
  delete b;
}

// what rr_bank_create and rr_bank_create_plaid do behind their own argument checks: the bank of the handle's device and li_dim with
// its device stores (nbits == 0: fp16 rows; else codes, residual bytes and the codec's tables copied from the host)
static hipError_t bank_new(rr_handle h, int64_t capacity_rows, int32_t max_passages, int nbits, int32_t n_centroids,
                           const uint16_t* centroids_f16, const float* bucket_weights, rr_bank_handle* out) {
  rr_bank* b = new rr_bank();
  b->device = h->cfg.device;
  b->D = h->cfg.li_dim;
  b->cap_rows = capacity_rows;
  b->max_passages = max_passages;
  b->nbits = nbits;
  b->n_centroids = n_centroids;
  const size_t cbytes = (size_t)n_centroids * b->D * sizeof(uint16_t), wbytes = ((size_t)1 << nbits) * sizeof(float);
  hipError_t e;
  if (nbits) {
    e = hipMalloc((void**)&b->codes, (size_t)capacity_rows * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&b->resid, (size_t)capacity_rows * b->resid_row_bytes());
  } else {
    e = hipMalloc((void**)&b->rows, (size_t)capacity_rows * b->D * sizeof(uint16_t));
  }
  if (e == hipSuccess) e = hipMalloc((void**)&b->mask, (size_t)capacity_rows);
  if (nbits) {
    if (e == hipSuccess) e = hipMalloc((void**)&b->centroids, cbytes);
    if (e == hipSuccess) e = hipMalloc((void**)&b->weights, wbytes);
    if (e == hipSuccess) e = hipMemcpy(b->centroids, centroids_f16, cbytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(b->weights, bucket_weights, wbytes, hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    bank_free(b);
    return e;
  }
  b->first.reserve((size_t)std::min<int64_t>(max_passages, 1 << 20));
  b->len.reserve((size_t)std::min<int64_t>(max_passages, 1 << 20));
  *out = b;
  return hipSuccess;
}

// rr_bank_create and rr_bank_create_plaid (`plaid`: compressed rows and the codec's tables copied to the device): the checks, each
// call's own between the model kind and the capacity, then the device and bank_new
static int bank_create(rr_handle h, const char* what, bool plaid, int64_t capacity_rows, int32_t max_passages, int nbits, int32_t n_centroids,
                       const uint16_t* centroids_f16, const float* bucket_weights, rr_bank_handle* out) {
  if (!h) return RR_ERR_BAD_ARG;
  if (!out) return fail(h, RR_ERR_BAD_ARG, "%s: null out", what);
  *out = nullptr;
  const int D = h->cfg.li_dim;
  if (h->cfg.model_kind == RR_MODEL_FULL_CONTEXT) return fail(h, RR_ERR_BAD_ARG, "%s on a full-context model", what);
  if (plaid && (!centroids_f16 || !bucket_weights)) return fail(h, RR_ERR_BAD_ARG, "%s: null table", what);
  if (plaid && !rr_plaid_shape_ok(nbits, D))
    return fail(h, RR_ERR_UNSUPPORTED, "%s: nbits %d, li_dim %d (nbits 1, 2, 4 or 8; li_dim a power of two in [8, 512], a multiple of 8 * nbits)",
                what, nbits, D);
  if (!plaid && (D <= 0 || (D & 7) || D > 512)) return fail(h, RR_ERR_UNSUPPORTED, "%s: li_dim %d (a multiple of 8, at most 512)", what, D);
  if (capacity_rows <= 0 || max_passages <= 0 || capacity_rows > (1LL << 40) || (plaid && (n_centroids <= 0 || n_centroids > (1 << 24))))
    return plaid ? fail(h, RR_ERR_BAD_SHAPE, "%s: capacity_rows=%lld max_passages=%d n_centroids=%d", what, (long long)capacity_rows, max_passages,
                        n_centroids)
                 : fail(h, RR_ERR_BAD_SHAPE, "%s: capacity_rows=%lld max_passages=%d", what, (long long)capacity_rows, max_passages);
  RR_HIP(h, hipSetDevice(h->cfg.device));
  const hipError_t e = bank_new(h, capacity_rows, max_passages, nbits, n_centroids, centroids_f16, bucket_weights, out);
  if (e == hipSuccess) return RR_OK;
  const int rc = e == hipErrorOutOfMemory ? RR_ERR_OOM : RR_ERR_HIP;
  return plaid ? fail(h, rc, "%s: %lld rows of %d at %d bits, %d centroids: %s", what, (long long)capacity_rows, D, nbits, n_centroids,
                      hipGetErrorString(e))
               : fail(h, rc, "%s: %lld rows of %d: %s", what, (long long)capacity_rows, D, hipGetErrorString(e));
}

int rr_bank_create(rr_handle h, int64_t capacity_rows, int32_t max_passages, rr_bank_handle* out) {
  return guarded(h, [&]() -> int { return bank_create(h, "rr_bank_create", false, capacity_rows, max_passages, 0, 0, nullptr, nullptr, out); });
}

int rr_bank_create_plaid(rr_handle h, int64_t capacity_rows, int32_t max_passages, int nbits, int32_t n_centroids, const uint16_t* centroids_f16,
                         const float* bucket_weights, rr_bank_handle* out) {
  return guarded(h, [&]() -> int { return bank_create(h, "rr_bank_create_plaid", true, capacity_rows, max_passages, nbits, n_centroids, centroids_f16, bucket_weights, out); });
}

int rr_bank_destroy(rr_bank_handle b) {
  return guarded(nullptr, [&]() -> int {
    if (!b) return RR_ERR_BAD_ARG;
    (void)hipSetDevice(b->device);
    (void)hipDeviceSynchronize();
    bank_free(b);
    return RR_OK;
  });
}

// Admission of n passages, shared by both kinds of add: every length in 1 .. max_len (0: no upper bound), *rows their sum, and
// the bank's slot and row limits.
static int bank_admit(rr_bank* b, const char* what, const int32_t* lengths, int n, int max_len, int64_t* rows) {
  *rows = 0;
  for (int i = 0; i < n; ++i) {
    if (lengths[i] < 1 || (max_len && lengths[i] > max_len))
      return max_len ? bfail(b, RR_ERR_BAD_SHAPE, "%s: passage %d has length %d (1..%d)", what, i, lengths[i], max_len)
                     : bfail(b, RR_ERR_BAD_SHAPE, "%s: passage %d has length %d (at least 1)", what, i, lengths[i]);
    *rows += lengths[i];
  }
  const int64_t have = (int64_t)b->first.size();
  if (have + n > b->max_passages)
    return bfail(b, RR_ERR_OOM, "%s: %lld + %d passages exceed the bank's %d slots", what, (long long)have, n, b->max_passages);
  if (b->used_rows + *rows > b->cap_rows)
    return bfail(b, RR_ERR_OOM, "%s: %lld + %lld rows exceed the bank's %lld", what, (long long)b->used_rows, (long long)*rows,
                 (long long)b->cap_rows);
  return RR_OK;
}
// ... and once their rows are on their way: the admitted passages appended to the host table, back to back from used_rows on
static void bank_append(rr_bank* b, const int32_t* lengths, int n, int32_t* first_index_out) {
  if (first_index_out) *first_index_out = (int32_t)b->first.size();
  for (int i = 0; i < n; ++i) {
    b->first.push_back(b->used_rows);
    b->len.push_back(lengths[i]);
    b->used_rows += lengths[i];
  }
}

// What rr_bank_add and rr_bank_add_compress (a compressed bank) do behind their own refusals.  Every check on the host first, so
// that everything that can refuse comes before the first enqueue; then one staged upload of the (first row, length) slots and the
// launch: the ingest kernel into the fp16 rows, or the kernels of bank_compress.hip (their scratch grown first) into the codes and
// residual bytes; mask bytes either way.
static int bank_add_padded(rr_bank* b, const char* what, const void* context_li, int dtype, const float* context_mask, const int32_t* lengths,
                           int n, int Lc, int32_t* first_index_out, void* hip_stream) {
  if (!context_li || !context_mask || !lengths) return bfail(b, RR_ERR_BAD_ARG, "%s: null argument", what);
  if (dtype != RR_F32 && dtype != RR_F16) return bfail(b, RR_ERR_BAD_DTYPE, "%s: dtype %d (RR_F32 or RR_F16)", what, dtype);
  if (((uintptr_t)context_li) & 15) return bfail(b, RR_ERR_BAD_ARG, "%s: context_li must be 16-byte aligned", what);
  if (n <= 0 || Lc <= 0 || (long long)n * Lc > (1LL << 40)) return bfail(b, RR_ERR_BAD_SHAPE, "%s: n=%d Lc=%d", what, n, Lc);
  int64_t rows = 0;
  RR_TRY(bank_admit(b, what, lengths, n, Lc, &rows));
  hipStream_t st = (hipStream_t)hip_stream;
  RR_TRY(bank_capture_guard(b, st, CAP_STAGES, what));
  const rr_compress_plan pl = b->has_codes() ? rr_plaid_compress_plan(rows, b->n_centroids, b->D) : rr_compress_plan{};      // (coded fp16: the codes behind the ingest)
  if (b->has_codes() && pl.jt == 0)
    return bfail(b, RR_ERR_BAD_SHAPE, "%s: %lld rows against %d centroids at the compress_chunk in force do not fit a launch", what,
                 (long long)rows, b->n_centroids);
  RR_BHIP(b, hipSetDevice(b->device));
  if (b->cscratch_cap < pl.total) {                // grow-only; calls still in flight read the old block (an fp16 bank's plan: 0 bytes)
    RR_BHIP(b, hipDeviceSynchronize());
    if (b->cscratch) { RR_BHIP(b, hipFree(b->cscratch)); b->cscratch = nullptr; b->cscratch_cap = 0; }
    RR_BHIP(b, hipMalloc((void**)&b->cscratch, pl.total));
    b->cscratch_cap = pl.total;
  }
  const int64_t r0 = b->used_rows;
  std::vector<rr_bank_slot> staged((size_t)n);
  int64_t row = r0;
  for (int i = 0; i < n; ++i) {
    staged[(size_t)i] = rr_bank_slot{row, lengths[i], 0};
    row += lengths[i];
  }
  rr_model::AsmSlot& a = b->slot[b->next];
  RR_BHIP(b, stage_slot(a, staged.data(), staged.size() * sizeof(rr_bank_slot), (size_t)1024 * sizeof(rr_bank_slot), st));
  const rr_padded_rows in{context_li, dtype == RR_F16, context_mask, (const rr_bank_slot*)a.dev, n, Lc};
  if (b->nbits)
    RR_BHIP(b, rr_launch_plaid_compress(in, r0, rows, b->D, b->nbits, b->centroids, b->n_centroids, b->cutoffs, b->cscratch, pl, b->codes + r0,
                                        b->resid + (size_t)r0 * b->resid_row_bytes(), b->mask + r0, st));
  else
    RR_BHIP(b, rr_launch_bank_ingest(in, b->D, b->rows, b->mask, st));
  if (b->coded())                                    // the new rows' codes, from the fp16 rows the ingest has just written
    RR_BHIP(b, rr_launch_plaid_assign_codes(b->rows + (size_t)r0 * b->D, rows, b->D, b->centroids, b->n_centroids, b->cscratch, pl, b->codes + r0, st));
  RR_BHIP(b, hipEventRecord(a.done, st));
  b->next ^= 1;
  bank_append(b, lengths, n, first_index_out);
  return RR_OK;
}

int rr_bank_add(rr_bank_handle b, const void* context_li, int dtype, const float* context_mask, const int32_t* lengths, int n, int Lc,
                int32_t* first_index_out, void* hip_stream) {
  return guarded(nullptr, [&]() -> int {
    const char* what = "rr_bank_add";
    if (!b) return RR_ERR_BAD_ARG;
    if (b->nbits) return bfail(b, RR_ERR_UNSUPPORTED, "%s on a compressed bank: it takes residual codes (rr_bank_add_plaid); nothing here compresses", what);
    return bank_add_padded(b, what, context_li, dtype, context_mask, lengths, n, Lc, first_index_out, hip_stream);
  });
}

// every check on the host first; then three copies (a fill for a NULL mask) and one synchronisation: a load-time call
int rr_bank_add_plaid(rr_bank_handle b, const int32_t* codes, const uint8_t* residuals, const uint8_t* mask, const int32_t* lengths, int n,
                      int32_t* first_index_out, void* hip_stream) {
  return guarded(nullptr, [&]() -> int {
    const char* what = "rr_bank_add_plaid";
    if (!b) return RR_ERR_BAD_ARG;
    if (!b->nbits) return bfail(b, RR_ERR_UNSUPPORTED, "%s on an fp16 bank: it takes embeddings (rr_bank_add)", what);
    if (!codes || !residuals || !lengths) return bfail(b, RR_ERR_BAD_ARG, "%s: null argument", what);
    if (n <= 0) return bfail(b, RR_ERR_BAD_SHAPE, "%s: n=%d", what, n);
    int64_t rows = 0;
    RR_TRY(bank_admit(b, what, lengths, n, 0, &rows));
    for (int64_t i = 0; i < rows; ++i)               // behind the capacity check: rows is bounded by it here
      if (codes[i] < 0 || codes[i] >= b->n_centroids)
        return bfail(b, RR_ERR_BAD_SHAPE, "%s: row %lld has centroid code %d, the codec %d centroids", what, (long long)i, codes[i], b->n_centroids);
    hipStream_t st = (hipStream_t)hip_stream;
    RR_TRY(bank_capture_guard(b, st, "%s cannot be captured into a graph (it copies from host memory and synchronises)", what));
    RR_BHIP(b, hipSetDevice(b->device));
    const int64_t r0 = b->used_rows;
    const size_t rb = b->resid_row_bytes();
    RR_BHIP(b, hipMemcpyAsync(b->codes + r0, codes, (size_t)rows * sizeof(int32_t), hipMemcpyHostToDevice, st));
    RR_BHIP(b, hipMemcpyAsync(b->resid + (size_t)r0 * rb, residuals, (size_t)rows * rb, hipMemcpyHostToDevice, st));
    if (mask) RR_BHIP(b, hipMemcpyAsync(b->mask + r0, mask, (size_t)rows, hipMemcpyHostToDevice, st));
    else RR_BHIP(b, hipMemsetAsync(b->mask + r0, 1, (size_t)rows, st));
    RR_BHIP(b, hipStreamSynchronize(st));            // the host buffers are the caller's again
    bank_append(b, lengths, n, first_index_out);
    return RR_OK;
  });
}

// rr_bank_set_plaid_cutoffs (include/rerank_mi355.h): validated on the host, then copied; a load-time call
int rr_bank_set_plaid_cutoffs(rr_bank_handle b, const float* cutoffs_host) {
  return guarded(nullptr, [&]() -> int {
    const char* what = "rr_bank_set_plaid_cutoffs";
    if (!b) return RR_ERR_BAD_ARG;
    if (!b->nbits) return bfail(b, RR_ERR_UNSUPPORTED, "%s on an fp16 bank: it holds embeddings as they are (rr_bank_add)", what);
    if (!cutoffs_host) return bfail(b, RR_ERR_BAD_ARG, "%s: null argument", what);
    const int n = (1 << b->nbits) - 1;
    for (int i = 0; i < n; ++i) {
      if (cutoffs_host[i] != cutoffs_host[i]) return bfail(b, RR_ERR_BAD_SHAPE, "%s: cutoff %d is NaN", what, i);
      if (i && cutoffs_host[i] < cutoffs_host[i - 1])
        return bfail(b, RR_ERR_BAD_SHAPE, "%s: cutoff %d (%g) lies below cutoff %d (%g): the sequence must not decrease", what, i,
                     (double)cutoffs_host[i], i - 1, (double)cutoffs_host[i - 1]);
    }
    RR_BHIP(b, hipSetDevice(b->device));
    if (!b->cutoffs) RR_BHIP(b, hipMalloc((void**)&b->cutoffs, 256 * sizeof(float)));
    else RR_BHIP(b, hipDeviceSynchronize());         // adds already enqueued keep the cutoffs they were given
    RR_BHIP(b, hipMemcpy(b->cutoffs, cutoffs_host, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    b->has_cutoffs = true;
    return RR_OK;
  });
}

// rr_bank_add_compress: what a bank must be to compress, then rr_bank_add's body
int rr_bank_add_compress(rr_bank_handle b, const void* context_li, int dtype, const float* context_mask, const int32_t* lengths, int n, int Lc,
                         int32_t* first_index_out, void* hip_stream) {
  return guarded(nullptr, [&]() -> int {
    const char* what = "rr_bank_add_compress";
    if (!b) return RR_ERR_BAD_ARG;
    if (!b->nbits) return bfail(b, RR_ERR_UNSUPPORTED, "%s on an fp16 bank: it keeps embeddings as fp16 rows (rr_bank_add)", what);
    if (!b->has_cutoffs) return bfail(b, RR_ERR_UNSUPPORTED, "%s: the bank has no bucket cutoffs (rr_bank_set_plaid_cutoffs)", what);
    if (b->D % 16) return bfail(b, RR_ERR_UNSUPPORTED, "%s: li_dim %d (a multiple of 16: the matrix-core step of the centroid search)", what, b->D);
    return bank_add_padded(b, what, context_li, dtype, context_mask, lengths, n, Lc, first_index_out, hip_stream);
  });
}

// rr_bank_set_centroids (include/rerank_mi355.h): an fp16 bank becomes, or stays, a coded one.  Every refusal on the host; then
// every allocation (the new table, the codes of a first call, the scratch grown), so that a failure leaves the bank as it was; only
// then the table is copied and takes its place, an inverted file over the old codes goes, and the rows the bank holds are assigned
// in launches of at most SET_CENTROIDS_ROWS rows (the keys of a launch bound the scratch, not the bank)
constexpr int64_t SET_CENTROIDS_ROWS = (int64_t)1 << 20;
int rr_bank_set_centroids(rr_bank_handle b, const uint16_t* centroids_f16_host, int32_t n_centroids, void* hip_stream) {
  return guarded(nullptr, [&]() -> int {
    const char* what = "rr_bank_set_centroids";
    if (!b) return RR_ERR_BAD_ARG;
    if (b->nbits) return bfail(b, RR_ERR_UNSUPPORTED, "%s on a compressed bank: its codes belong to its residuals (rr_bank_create_plaid)", what);
    if (!centroids_f16_host) return bfail(b, RR_ERR_BAD_ARG, "%s: null argument", what);
    if (b->D % 16) return bfail(b, RR_ERR_UNSUPPORTED, "%s: li_dim %d (a multiple of 16: the matrix-core step of the centroid search)", what, b->D);
    if (n_centroids < 1 || n_centroids > RR_PLAID_SEARCH_MAX_CENTROIDS)
      return bfail(b, RR_ERR_BAD_SHAPE, "%s: n_centroids=%d (1..%d)", what, n_centroids, RR_PLAID_SEARCH_MAX_CENTROIDS);
    const int64_t held_rows = b->used_rows, step = std::min(held_rows, SET_CENTROIDS_ROWS);
    const rr_compress_plan pl = step ? rr_plaid_compress_plan(step, n_centroids, b->D) : rr_compress_plan{};
    const int64_t tail = step ? held_rows % step : 0;       // the rows of a shorter last launch, with a plan of its own
    const rr_compress_plan pl_tail = tail ? rr_plaid_compress_plan(tail, n_centroids, b->D) : pl;
    if (step && (pl.jt == 0 || pl_tail.jt == 0))
      return bfail(b, RR_ERR_BAD_SHAPE, "%s: %lld rows against %d centroids at the compress_chunk in force do not fit a launch", what,
                   (long long)step, n_centroids);
    const size_t need = std::max(pl.total, pl_tail.total);
    hipStream_t st = (hipStream_t)hip_stream;
    RR_TRY(bank_capture_guard(b, st, "%s cannot be captured into a graph (it allocates, copies from host memory and synchronises)", what));
    RR_BHIP(b, hipSetDevice(b->device));
    RR_BHIP(b, hipDeviceSynchronize());              // adds in flight write the rows read below; searches read the table that goes
    const size_t cbytes = (size_t)n_centroids * b->D * sizeof(uint16_t);
    uint16_t* table = nullptr;
    int32_t* codes = b->codes;
    char* scratch = nullptr;
    hipError_t e = hipMalloc((void**)&table, cbytes);
    if (e == hipSuccess && !codes) e = hipMalloc((void**)&codes, (size_t)b->cap_rows * sizeof(int32_t));
    if (e == hipSuccess && b->cscratch_cap < need) e = hipMalloc((void**)&scratch, need);
    if (e == hipSuccess) e = hipMemcpy(table, centroids_f16_host, cbytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      if (table) (void)hipFree(table);
      if (codes && codes != b->codes) (void)hipFree(codes);
      if (scratch) (void)hipFree(scratch);
      return bfail(b, e == hipErrorOutOfMemory ? RR_ERR_OOM : RR_ERR_HIP, "%s: %lld rows of capacity, %d centroids of %d: %s (the bank is unchanged)",
                   what, (long long)b->cap_rows, n_centroids, b->D, hipGetErrorString(e));
    }
    if (scratch) {                                   // grow-only, as an add grows it (the device was synchronised above: no add still reads the old block)
      if (b->cscratch) (void)hipFree(b->cscratch);
      b->cscratch = scratch;
      b->cscratch_cap = need;
    }
    if (b->centroids) (void)hipFree(b->centroids);
    b->centroids = table;
    b->codes = codes;
    b->n_centroids = n_centroids;
    rr_ivf_free(&b->ivf);                            // its lists name the codes of the table that went
    for (int64_t r0 = 0; r0 < held_rows; r0 += step) {
      const int64_t R = std::min(step, held_rows - r0);
      const rr_compress_plan& p = R == step ? pl : pl_tail;
      RR_BHIP(b, rr_launch_plaid_assign_codes(b->rows + (size_t)r0 * b->D, R, b->D, b->centroids, n_centroids, b->cscratch, p, b->codes + r0, st));
    }
    RR_BHIP(b, hipStreamSynchronize(st));
    return RR_OK;
  });
}

// rr_op_plaid_compress_rows (include/rerank_mi355_diag.h): the kernels over loose device pointers; its scratch lives for the call
int rr_op_plaid_compress_rows(const void* rows, int dtype, int64_t n_rows, int D, const uint16_t* centroids_f16, int32_t n_centroids,
                              const float* cutoffs, int nbits, int32_t* codes_out, uint8_t* residuals_out, void* hip_stream) {
  return guarded(nullptr, [&]() -> int {
    if (!rows || !centroids_f16 || !cutoffs || !codes_out || !residuals_out) return RR_ERR_BAD_ARG;
    if (dtype != RR_F32 && dtype != RR_F16) return RR_ERR_BAD_DTYPE;
    if (!rr_plaid_compress_shape_ok(nbits, D)) return RR_ERR_UNSUPPORTED;
    if (n_rows <= 0 || n_rows > (1LL << 31) || n_centroids <= 0 || n_centroids > (1 << 24)) return RR_ERR_BAD_SHAPE;
    if (((((uintptr_t)rows) | ((uintptr_t)centroids_f16)) & 15) || (((uintptr_t)residuals_out) & 7) || (((uintptr_t)codes_out) & 3) ||
        (((uintptr_t)cutoffs) & 3))
      return RR_ERR_BAD_ARG;
    const rr_compress_plan pl = rr_plaid_compress_plan(n_rows, n_centroids, D);
    if (pl.jt == 0) return RR_ERR_BAD_SHAPE;
    hipStream_t st = (hipStream_t)hip_stream;
    char* scratch = nullptr;
    hipError_t e = hipMalloc((void**)&scratch, pl.total);
    if (e != hipSuccess) return e == hipErrorOutOfMemory ? RR_ERR_OOM : RR_ERR_HIP;
    e = rr_launch_plaid_compress(rr_padded_rows{rows, dtype == RR_F16, nullptr, nullptr, 0, 0}, 0, n_rows, D, nbits, centroids_f16, n_centroids,
                                 cutoffs, scratch, pl, codes_out, residuals_out, nullptr, st);
    const hipError_t e2 = hipStreamSynchronize(st);
    (void)hipFree(scratch);
    return e == hipSuccess && e2 == hipSuccess ? RR_OK : RR_ERR_HIP;
  });
}

// What rr_plaid_kmeans and rr_plaid_residuals check of their rows alike, in the order the bank entries refuse
static int plaid_train_rows_ok(rr_model* m, const char* what, int D, const void* rows, int dtype, int64_t n_rows, int32_t n_centroids) {
  if (dtype != RR_F32 && dtype != RR_F16) return fail(m, RR_ERR_BAD_DTYPE, "%s: dtype %d (RR_F32 or RR_F16)", what, dtype);
  if (!rr_plaid_train_shape_ok(D))
    return fail(m, RR_ERR_UNSUPPORTED, "%s: li_dim %d (a power of two in [16, 512]: the matrix-core step and the tree of the norm)", what, D);
  if (((uintptr_t)rows) & 15) return fail(m, RR_ERR_BAD_ARG, "%s: rows must be 16-byte aligned", what);
  if (n_rows > (1LL << 30))
    return fail(m, RR_ERR_UNSUPPORTED, "%s: %lld rows (at most 2^30: the fixed-point sums stay inside 64 bits)", what, (long long)n_rows);
  if (n_rows < 1) return fail(m, RR_ERR_BAD_SHAPE, "%s: n_rows=%lld", what, (long long)n_rows);
  if (n_centroids < 1 || n_centroids > n_rows)
    return fail(m, RR_ERR_BAD_SHAPE, "%s: %d centroids of %lld rows (1 .. n_rows)", what, n_centroids, (long long)n_rows);
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, rows) != hipSuccess) {
    (void)hipGetLastError();                       // not a pointer the runtime knows: the caller answers for it
  } else if (m && at.type == hipMemoryTypeDevice && at.device != m->cfg.device) {
    return fail(m, RR_ERR_BAD_ARG, "%s: rows live on device %d, the handle on %d", what, at.device, m->cfg.device);
  }
  return RR_OK;
}

// the scratch of a training call: the handle's grow-only block, or without a handle (the diagnostic operators) a block of its own,
// released behind a synchronisation by plaid_train_done
static int plaid_train_scratch(rr_model* m, size_t bytes, hipStream_t st, char** out) {
  if (m) {
    RR_HIP(m, hipSetDevice(m->cfg.device));
    RR_TRY(ensure_block(m, m->train_blk, m->train_blk_cap, bytes, st, "the codec training's block"));
    *out = m->train_blk;
    return RR_OK;
  }
  RR_HIP(m, hipMalloc((void**)out, bytes));
  return RR_OK;
}
static int plaid_train_done(rr_model* m, char* scratch, hipStream_t st, int rc) {
  if (m) return rc;
  const hipError_t e = hipStreamSynchronize(st);
  (void)hipFree(scratch);
  return rc != RR_OK ? rc : e == hipSuccess ? RR_OK : RR_ERR_HIP;
}

// rr_plaid_kmeans (include/rerank_mi355.h, THE TRAINED CENTROIDS): every refusal on the host, one synchronisation behind the staging
// of init_rows, then the kernels of plaid_train.hip back to back
static int rr_plaid_kmeans_impl(rr_model* m, const char* what, int D, const void* rows, int dtype, int64_t n_rows, const int32_t* init_rows_host, int32_t n_centroids,
                                int niters, uint64_t seed, uint16_t* centroids_f16_out, int32_t* counts_out, int32_t* stats_out,
                                void* hip_stream) {
  if (!rows || !init_rows_host || !centroids_f16_out) return fail(m, RR_ERR_BAD_ARG, "%s: null argument", what);
  RR_TRY(plaid_train_rows_ok(m, what, D, rows, dtype, n_rows, n_centroids));
  if ((((uintptr_t)centroids_f16_out) & 15) || ((((uintptr_t)counts_out) | ((uintptr_t)stats_out)) & 3))
    return fail(m, RR_ERR_BAD_ARG, "%s: centroids_f16_out must be 16-byte aligned, counts_out and stats_out 4-byte", what);
  if (niters < 0) return fail(m, RR_ERR_BAD_SHAPE, "%s: niters=%d", what, niters);
  {
    std::vector<int32_t> sorted(init_rows_host, init_rows_host + n_centroids);
    std::sort(sorted.begin(), sorted.end());
    if (sorted.front() < 0 || sorted.back() >= n_rows)
      return fail(m, RR_ERR_BAD_SHAPE, "%s: an initial row index outside [0, %lld)", what, (long long)n_rows);
    for (size_t i = 1; i < sorted.size(); ++i)
      if (sorted[i] == sorted[i - 1]) return fail(m, RR_ERR_BAD_SHAPE, "%s: initial row %d is named twice", what, sorted[i]);
  }
  const rr_kmeans_plan pl = rr_plaid_kmeans_plan(n_rows, n_centroids, D, niters);
  if (pl.assign.jt == 0)
    return fail(m, RR_ERR_BAD_SHAPE, "%s: %lld rows against %d centroids at the compress_chunk in force do not fit a launch", what,
                (long long)n_rows, n_centroids);
  hipStream_t st = (hipStream_t)hip_stream;
  RR_TRY(capture_guard(m, st, CAP_STAGES, what));
  char* scratch = nullptr;
  RR_TRY(plaid_train_scratch(m, pl.total, st, &scratch));
  auto run = [&]() -> int {
    RR_HIP(m, hipMemcpyAsync(scratch + pl.init_off, init_rows_host, (size_t)n_centroids * sizeof(int32_t), hipMemcpyHostToDevice, st));
    RR_HIP(m, hipStreamSynchronize(st));           // the caller's init_rows are its own again; nothing below synchronises
    RR_HIP(m, rr_launch_plaid_kmeans(rows, dtype == RR_F16, n_rows, D, n_centroids, niters, (unsigned long long)seed, scratch, pl,
                                     centroids_f16_out, counts_out, stats_out, st));
    return RR_OK;
  };
  return plaid_train_done(m, scratch, st, run());
}

// rr_plaid_residuals: codes and float32 residuals of device rows against a finished table
static int rr_plaid_residuals_impl(rr_model* m, const char* what, int D, const void* rows, int dtype, int64_t n_rows, const uint16_t* centroids_f16, int32_t n_centroids,
                                   int32_t* codes_out, float* residuals_out, void* hip_stream) {
  if (!rows || !centroids_f16 || !codes_out || !residuals_out) return fail(m, RR_ERR_BAD_ARG, "%s: null argument", what);
  if (dtype != RR_F32 && dtype != RR_F16) return fail(m, RR_ERR_BAD_DTYPE, "%s: dtype %d (RR_F32 or RR_F16)", what, dtype);
  if (!rr_plaid_train_shape_ok(D))
    return fail(m, RR_ERR_UNSUPPORTED, "%s: li_dim %d (a power of two in [16, 512]: the matrix-core step and the tree of the norm)", what, D);
  if (((((uintptr_t)rows) | ((uintptr_t)centroids_f16) | ((uintptr_t)residuals_out)) & 15) || (((uintptr_t)codes_out) & 3))
    return fail(m, RR_ERR_BAD_ARG, "%s: rows, centroids_f16 and residuals_out must be 16-byte aligned, codes_out 4-byte", what);
  if (n_rows < 1 || n_rows > (1LL << 31) || n_centroids < 1)
    return fail(m, RR_ERR_BAD_SHAPE, "%s: n_rows=%lld n_centroids=%d", what, (long long)n_rows, n_centroids);
  const rr_compress_plan pl = rr_plaid_compress_plan(n_rows, n_centroids, D);
  if (pl.jt == 0)
    return fail(m, RR_ERR_BAD_SHAPE, "%s: %lld rows against %d centroids at the compress_chunk in force do not fit a launch", what,
                (long long)n_rows, n_centroids);
  hipStream_t st = (hipStream_t)hip_stream;
  RR_TRY(capture_guard(m, st, "%s cannot be captured into a graph (it may grow the handle's training block)", what));
  char* scratch = nullptr;
  RR_TRY(plaid_train_scratch(m, pl.total, st, &scratch));
  auto run = [&]() -> int {
    RR_HIP(m, rr_launch_plaid_residuals(rows, dtype == RR_F16, n_rows, D, centroids_f16, n_centroids, scratch, pl, codes_out, residuals_out, st));
    return RR_OK;
  };
  return plaid_train_done(m, scratch, st, run());
}

int rr_op_plaid_decode_rows(const uint16_t* centroids_f16, int32_t n_centroids, const float* bucket_weights, int nbits, int D, const int32_t* codes,
                            const uint8_t* residuals, int64_t first_row, int64_t n_rows, uint16_t* rows_out_f16, void* hip_stream) {
  return guarded(nullptr, [&]() -> int {
    if (!centroids_f16 || !bucket_weights || !codes || !residuals || !rows_out_f16) return fail(nullptr, RR_ERR_BAD_ARG, "rr_op_plaid_decode_rows: null argument");
    if (!rr_plaid_shape_ok(nbits, D)) return RR_ERR_UNSUPPORTED;
    if (n_centroids <= 0 || first_row < 0 || n_rows <= 0 || first_row > (1LL << 40) || n_rows > (1LL << 40)) return RR_ERR_BAD_SHAPE;
    if (((((uintptr_t)centroids_f16) | ((uintptr_t)rows_out_f16)) & 15) || (((uintptr_t)residuals) & 7) || (((uintptr_t)codes) & 3))
      return RR_ERR_BAD_ARG;
    const rr_bank_view bank{nbits, n_centroids, nullptr, codes, residuals, centroids_f16, bucket_weights, nullptr};
    const hipError_t e = rr_launch_plaid_decode(bank, D, first_row, n_rows, rows_out_f16, (hipStream_t)hip_stream);
    return e == hipSuccess ? RR_OK : RR_ERR_HIP;
  });
}

// rr_bank_read (rows_out, mask_out) and rr_bank_read_plaid (codes_out, resid_out, mask_out) behind their own refusals: one passage
// copied to the host.  All outputs null: its length alone, nothing synchronised.
static int bank_read(rr_bank* b, const char* what, int32_t index, uint16_t* rows_out, int32_t* codes_out, uint8_t* resid_out, uint8_t* mask_out,
                     int32_t capacity_rows, void* hip_stream) {
  if (index < 0 || (size_t)index >= b->first.size()) return bfail(b, RR_ERR_BAD_SHAPE, "%s: passage %d of %zu", what, index, b->first.size());
  const int32_t len = b->len[(size_t)index];
  if (!rows_out && !codes_out && !resid_out && !mask_out) return len;
  if (capacity_rows < len) return bfail(b, RR_ERR_BAD_SHAPE, "%s: passage %d holds %d rows, the buffers %d", what, index, len, capacity_rows);
  RR_BHIP(b, hipSetDevice(b->device));
  RR_BHIP(b, hipStreamSynchronize((hipStream_t)hip_stream));
  const int64_t r0 = b->first[(size_t)index];
  const size_t rb = b->resid_row_bytes();
  if (rows_out && b->nbits) {                      // decoded by the kernel function the gather uses
    const size_t bytes = (size_t)len * b->D * sizeof(uint16_t);
    uint16_t* tmp = nullptr;
    RR_BHIP(b, hipMalloc((void**)&tmp, bytes));
    hipError_t e = rr_launch_plaid_decode(bank_view(b), b->D, r0, len, tmp, (hipStream_t)hip_stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)hip_stream);
    if (e == hipSuccess) e = hipMemcpy(rows_out, tmp, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(tmp);
    RR_BHIP(b, e);
  } else if (rows_out) {
    RR_BHIP(b, hipMemcpy(rows_out, b->rows + (size_t)r0 * b->D, (size_t)len * b->D * sizeof(uint16_t), hipMemcpyDeviceToHost));
  }
  if (codes_out) RR_BHIP(b, hipMemcpy(codes_out, b->codes + r0, (size_t)len * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (resid_out) RR_BHIP(b, hipMemcpy(resid_out, b->resid + (size_t)r0 * rb, (size_t)len * rb, hipMemcpyDeviceToHost));
  if (mask_out) RR_BHIP(b, hipMemcpy(mask_out, b->mask + r0, (size_t)len, hipMemcpyDeviceToHost));
  return len;
}

int rr_bank_read(rr_bank_handle b, int32_t index, uint16_t* rows_out, uint8_t* mask_out, int32_t capacity_rows, void* hip_stream) {
  return guarded(nullptr, [&]() -> int {
    if (!b) return RR_ERR_BAD_ARG;
    return bank_read(b, "rr_bank_read", index, rows_out, nullptr, nullptr, mask_out, capacity_rows, hip_stream);
  });
}

// rr_bank_read_plaid: the stored form of one passage of a compressed bank
int rr_bank_read_plaid(rr_bank_handle b, int32_t index, int32_t* codes_out, uint8_t* resid_out, uint8_t* mask_out, int32_t capacity_rows,
                       void* hip_stream) {
  return guarded(nullptr, [&]() -> int {
    const char* what = "rr_bank_read_plaid";
    if (!b) return RR_ERR_BAD_ARG;
    if (b->coded())
      return bfail(b, RR_ERR_UNSUPPORTED, "%s on an fp16 bank with a centroid table: it holds codes but no residuals (rr_bank_read_codes, rr_bank_read)", what);
    if (!b->nbits) return bfail(b, RR_ERR_UNSUPPORTED, "%s on an fp16 bank: it holds no codes (rr_bank_read)", what);
    return bank_read(b, what, index, nullptr, codes_out, resid_out, mask_out, capacity_rows, hip_stream);
  });
}

// rr_bank_read_codes (include/rerank_mi355_diag.h): the codes of one passage, of a compressed or a coded fp16 bank
int rr_bank_read_codes(rr_bank_handle b, int32_t index, int32_t* codes_out, int32_t capacity_rows, void* hip_stream) {
  return guarded(nullptr, [&]() -> int {
    const char* what = "rr_bank_read_codes";
    if (!b) return RR_ERR_BAD_ARG;
    if (!b->has_codes()) return bfail(b, RR_ERR_UNSUPPORTED, "%s on an fp16 bank without a centroid table: it holds no codes (rr_bank_set_centroids)", what);
    return bank_read(b, what, index, nullptr, codes_out, nullptr, nullptr, capacity_rows, hip_stream);
  });
}

// rr_bank_build_ivf and rr_bank_extend_ivf (include/rerank_mi355.h): one body, the same refusals in the same order.  The file is
// built beside the one the bank holds and takes its place only when complete.  `extend`: a file that covers every passage is left as
// it is, one over a prefix is extended (rr_ivf_build reads it), and without a file the call is the build.
static int bank_ivf_call(rr_bank* b, bool extend, void* hip_stream) {
  const char* what = extend ? "rr_bank_extend_ivf" : "rr_bank_build_ivf";
  if (!b) return RR_ERR_BAD_ARG;
  if (!b->has_codes()) return bfail(b, RR_ERR_UNSUPPORTED, "%s on an fp16 bank: it holds no codes", what);
  const long long held = (long long)b->first.size();
  if (held < 1) return bfail(b, RR_ERR_BAD_SHAPE, "%s: the bank holds no passage", what);
  hipStream_t st = (hipStream_t)hip_stream;
  RR_TRY(bank_capture_guard(b, st, "%s cannot be captured into a graph (it allocates and synchronises)", what));
  const int covered = b->ivf.passages;
  if (extend && covered == held) return RR_OK;            // nothing to add: nothing allocated, enqueued or synchronised
  RR_BHIP(b, hipSetDevice(b->device));
  rr_ivf f{};
  const bool from_old = extend && covered > 0 && covered < held;
  const char* step = "";
  const hipError_t e = rr_ivf_build(bank_view(b), b->first.data(), b->len.data(), (int)held, st, &f, from_old ? &b->ivf : nullptr, &step);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    if (extend)
      return bfail(b, e == hipErrorOutOfMemory ? RR_ERR_OOM : RR_ERR_HIP, "%s: %lld passages behind the %d the file covers, %d centroids: %s "
                   "failed: %s (the bank and its file are unchanged)", what, held - covered, covered, b->n_centroids, step, hipGetErrorString(e));
    return bfail(b, e == hipErrorOutOfMemory ? RR_ERR_OOM : RR_ERR_HIP, "%s: %lld passages, %d centroids: %s (the bank is unchanged)", what, held,
                 b->n_centroids, hipGetErrorString(e));
  }
  rr_ivf_free(&b->ivf);                               // hipFree waits for a search that still reads the previous file
  b->ivf = f;
  return RR_OK;
}
int rr_bank_build_ivf(rr_bank_handle b, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return bank_ivf_call(b, false, hip_stream); });
}
int rr_bank_extend_ivf(rr_bank_handle b, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return bank_ivf_call(b, true, hip_stream); });
}

int rr_bank_ivf_info(rr_bank_handle b, int32_t* passages_covered_out, int64_t* postings_out, int32_t* longest_list_out) {
  return guarded(nullptr, [&]() -> int {
    if (!b) return RR_ERR_BAD_ARG;
    if (passages_covered_out) *passages_covered_out = b->ivf.passages;
    if (postings_out) *postings_out = b->ivf.postings;
    if (longest_list_out) *longest_list_out = b->ivf.longest;
    return RR_OK;
  });
}

int rr_bank_ivf_read(rr_bank_handle b, int64_t* offsets_host_out, int32_t* pids_host_out, void* hip_stream) {
  return guarded(nullptr, [&]() -> int {
    const char* what = "rr_bank_ivf_read";
    if (!b) return RR_ERR_BAD_ARG;
    if (!b->ivf.passages) return bfail(b, RR_ERR_BAD_ARG, "%s: the bank has no inverted file (rr_bank_build_ivf)", what);
    hipStream_t st = (hipStream_t)hip_stream;
    RR_TRY(bank_capture_guard(b, st, "%s cannot be captured into a graph (it synchronises)", what));
    RR_BHIP(b, hipSetDevice(b->device));
    RR_BHIP(b, rr_ivf_read(b->ivf, b->n_centroids, offsets_host_out, pids_host_out, st));
    return RR_OK;
  });
}

// rr_bank_filter_fill (include/rerank_mi355.h): the lists checked on the host, staged through the bank's slot pair as an add stages
// its descriptors ([rows + 1] int64 offsets, then the int32 indices), one launch
int rr_bank_filter_fill(rr_bank_handle b, const int32_t* indices_host, const int64_t* offsets_host, int rows, int exclude, uint32_t* filter_bits,
                        int64_t filter_ld, void* hip_stream) {
  return guarded(nullptr, [&]() -> int {
    const char* what = "rr_bank_filter_fill";
    if (!b) return RR_ERR_BAD_ARG;
    if (!offsets_host || !filter_bits || (((uintptr_t)filter_bits) & 3)) return bfail(b, RR_ERR_BAD_ARG, "%s: null or misaligned argument", what);
    const long long held = (long long)b->first.size();
    if (rows < 1 || rows > 65535) return bfail(b, RR_ERR_BAD_SHAPE, "%s: rows=%d (1..65535)", what, rows);
    if (held < 1) return bfail(b, RR_ERR_BAD_SHAPE, "%s: the bank holds no passage", what);
    if (filter_ld < (held + 31) / 32)
      return bfail(b, RR_ERR_BAD_SHAPE, "%s: filter_ld=%lld words, %lld passages take %lld", what, (long long)filter_ld, held, (held + 31) / 32);
    if (offsets_host[0] != 0) return bfail(b, RR_ERR_BAD_SHAPE, "%s: offsets[0]=%lld", what, (long long)offsets_host[0]);
    for (int r = 0; r < rows; ++r)
      if (offsets_host[r + 1] < offsets_host[r]) return bfail(b, RR_ERR_BAD_SHAPE, "%s: offsets descend at row %d", what, r);
    const int64_t total = offsets_host[rows];
    if (total > 0 && !indices_host) return bfail(b, RR_ERR_BAD_ARG, "%s: null indices", what);
    if (total > ((int64_t)1 << 30)) return bfail(b, RR_ERR_BAD_SHAPE, "%s: %lld indices", what, (long long)total);
    for (int64_t i = 0; i < total; ++i)
      if (indices_host[i] < 0 || indices_host[i] >= held)
        return bfail(b, RR_ERR_BAD_SHAPE, "%s: entry %lld names passage %d, the bank holds %lld", what, (long long)i, indices_host[i], held);
    hipStream_t st = (hipStream_t)hip_stream;
    RR_TRY(bank_capture_guard(b, st, "%s cannot be captured into a graph (it stages the lists)", what));
    RR_BHIP(b, hipSetDevice(b->device));
    const size_t off_bytes = ((size_t)rows + 1) * sizeof(int64_t);
    std::vector<char> upload(off_bytes + (size_t)total * sizeof(int32_t));
    memcpy(upload.data(), offsets_host, off_bytes);
    if (total) memcpy(upload.data() + off_bytes, indices_host, (size_t)total * sizeof(int32_t));
    rr_model::AsmSlot& a = b->slot[b->next];
    RR_BHIP(b, stage_slot(a, upload.data(), upload.size(), (size_t)1024 * sizeof(rr_bank_slot), st));
    RR_BHIP(b, rr_launch_filter_fill((const int64_t*)a.dev, (const int32_t*)((const char*)a.dev + off_bytes), rows, exclude != 0, (int)held,
                                     filter_bits, (long long)filter_ld, st));
    RR_BHIP(b, hipEventRecord(a.done, st));
    b->next ^= 1;
    return RR_OK;
  });
}

int rr_util_bank_filter_bits(const int32_t* indices, const int64_t* offsets, int rows, int exclude, int32_t passages, uint32_t* bits_out,
                             int64_t filter_ld) {
  return guarded(nullptr, [&]() -> int {
    if (!offsets || !bits_out) return RR_ERR_BAD_ARG;
    if (rows < 1 || passages < 1) return RR_ERR_BAD_SHAPE;
    if (offsets[0] == 0 && offsets[rows] > 0 && !indices) return RR_ERR_BAD_ARG;
    return rr_filter_bits_host(indices, offsets, rows, exclude != 0, passages, bits_out, (long long)filter_ld) ? RR_OK : RR_ERR_BAD_SHAPE;
  });
}

int rr_util_plaid_ivf(const int32_t* codes, const uint8_t* mask, const int32_t* lengths, int32_t n_passages, int32_t n_centroids,
                      int64_t* offsets_out, int32_t* pids_out, int64_t pids_capacity, int64_t* postings_out) {
  return guarded(nullptr, [&]() -> int {
    if (!codes || !lengths || !offsets_out) return RR_ERR_BAD_ARG;
    if (n_passages < 1 || n_centroids < 1 || (pids_out && pids_capacity < 0)) return RR_ERR_BAD_SHAPE;
    for (int p = 0; p < n_passages; ++p)
      if (lengths[p] < 1) return RR_ERR_BAD_SHAPE;
    const int64_t total = rr_ivf_host(codes, mask, lengths, n_passages, n_centroids, offsets_out, pids_out, pids_out ? pids_capacity : 0);
    if (postings_out) *postings_out = total;
    return pids_out && total > pids_capacity ? RR_ERR_BAD_SHAPE : RR_OK;
  });
}

// rr_bank_li_scores (include/rerank_mi355.h): every check on the host first, then one staged upload and one launch
static int bank_li_scores_call(rr_handle h, rr_bank* b, const float* query_li, int n_queries, int Lq, const int32_t* pair_passage,
                               const int32_t* pair_query, int n_pairs, int padded_context_len, float* scores_out, float* maxsim_out,
                               void* hip_stream) {
  const char* what = "rr_bank_li_scores";
  if (!h) return RR_ERR_BAD_ARG;
  rr_model* m = h;
  const rr_config& c = m->cfg;
  if (!b || !query_li || !pair_passage || !pair_query) return fail(m, RR_ERR_BAD_ARG, "%s: null argument", what);
  if (!scores_out && !maxsim_out) return fail(m, RR_ERR_BAD_ARG, "%s: scores_out and maxsim_out are both null", what);
  RR_TRY(bank_usable(m, what, b));
  const int D = c.li_dim;
  if (D % 16) return fail(m, RR_ERR_UNSUPPORTED, "%s: li_dim %d (a multiple of 16)", what, D);
  if (((uintptr_t)query_li) & 15) return fail(m, RR_ERR_BAD_ARG, "%s: query_li must be 16-byte aligned", what);
  if (n_queries <= 0 || Lq <= 0 || n_pairs <= 0 || padded_context_len <= 0)
    return fail(m, RR_ERR_BAD_SHAPE, "%s: n_queries=%d Lq=%d n_pairs=%d padded_context_len=%d", what, n_queries, Lq, n_pairs,
                padded_context_len);
  if (n_pairs > (1 << 24)) return fail(m, RR_ERR_BAD_SHAPE, "%s: %d pairs", what, n_pairs);
  RR_TRY(check_rows(m, what, n_pairs, padded_context_len));
  std::vector<rr_bank_pair> checked((size_t)n_pairs);
  double rows = 0.0;
  for (int i = 0; i < n_pairs; ++i) {
    RR_TRY(bank_checked_pair(m, what, b, i, pair_passage[i], pair_query[i], n_queries, padded_context_len, "padded_context_len is",
                             &checked[(size_t)i]));
    rows += checked[(size_t)i].len;
  }
  // one workgroup per pair, dispatched in launch order: the longest passages go first (stable, so equal lengths keep call order)
  // and every workgroup is told which output row is its pair's.  One upload: [n] descriptors in launch order, then [n] int32
  // output rows.
  std::vector<int32_t> order((size_t)n_pairs);
  for (int i = 0; i < n_pairs; ++i) order[(size_t)i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return checked[(size_t)x].len > checked[(size_t)y].len; });
  const size_t desc_bytes = (size_t)n_pairs * sizeof(rr_bank_pair);
  std::vector<char> upload(desc_bytes + (size_t)n_pairs * sizeof(int32_t));
  rr_bank_pair* up = (rr_bank_pair*)upload.data();
  for (int i = 0; i < n_pairs; ++i) up[i] = checked[(size_t)order[(size_t)i]];
  memcpy(upload.data() + desc_bytes, order.data(), (size_t)n_pairs * sizeof(int32_t));
  hipStream_t st = (hipStream_t)hip_stream;
  void* dev = nullptr;
  RR_TRY(asm_stage(m, what, upload.data(), upload.size(), st, &dev));      // refuses a capturing stream
  const int32_t* slot = (const int32_t*)((const char*)dev + desc_bytes);
  m->last_stream = st;
  // bytes: the rows that exist (a compressed row: its code, its residual bytes and the centroid row from L2), one mask byte per
  // row, the query block per pair, the outputs; pad rows cost their -9999 in the score block only
  const rr_bank_view bank = bank_view(b);
  const double bytes = rows * (rr_bank_row_bytes(bank, D) + 1.0) + (double)n_pairs * (16.0 + 4.0 * Lq * D) +
                       (scores_out ? 4.0 * n_pairs * (double)padded_context_len * Lq : 0.0) + (maxsim_out ? 4.0 * n_pairs : 0.0);
  RR_RUN(m, st, RR_K_TAIL, 2.0 * rows * Lq * D, bytes,
         rr_launch_bank_li_scores((const rr_bank_pair*)dev, slot, n_pairs, Lq, padded_context_len, D, query_li, bank, scores_out, maxsim_out, st));
  return asm_done(m, st);
}

// the bank's device copy of its passage table, brought up to date (only after an add): what every search does first
static int bank_table_current(rr_model* m, rr_bank* b, hipStream_t st) {
  const long long held = (long long)b->first.size();
  if (b->table_n < (size_t)held) {                  // the first search after an add
    if (b->table_cap < (size_t)held) {
      if (b->table) { RR_HIP(m, hipFree(b->table)); b->table = nullptr; }      // hipFree waits for whatever still reads it
      b->table_cap = 0;
      b->table_n = 0;
      const size_t cap = std::min<size_t>((size_t)b->max_passages, std::max<size_t>((size_t)held * 2, 1024));
      RR_HIP(m, hipMalloc((void**)&b->table, cap * sizeof(rr_bank_slot)));
      b->table_cap = cap;
    }
    std::vector<rr_bank_slot> up((size_t)held - b->table_n);
    for (size_t i = 0; i < up.size(); ++i) up[i] = rr_bank_slot{b->first[b->table_n + i], b->len[b->table_n + i], 0};
    RR_HIP(m, hipMemcpyAsync(b->table + b->table_n, up.data(), up.size() * sizeof(rr_bank_slot), hipMemcpyHostToDevice, st));
    RR_HIP(m, hipStreamSynchronize(st));            // `up` is pageable memory of this call
    b->table_n = (size_t)held;
  }
  return RR_OK;
}

// What rr_bank_search and rr_bank_search_plaid (`pruned`: banks with codes only, compressed or coded fp16; `counted`: counts_out is required, as in the pruned and
// the filtered entries, and null with the other null arguments) do alike before their first launch: the
// shared checks, the range resolved into (first_passage, *n), then `limits(n)`, the call's own refusals, where they have always stood;
// the device, the bank's table brought up to date, and *rows: the rows of the range (passages lie back to back), for the profile
static int bank_search_begin(rr_model* m, const char* what, bool pruned, bool counted, rr_bank* b, const float* query_li, int n_queries, int Lq,
                             int32_t first_passage, int32_t n_passages, const int32_t* indices_out, const float* scores_out,
                             const int32_t* counts_out, hipStream_t st, int* n, double* rows, const std::function<int(int)>& limits) {
  if (!b || !query_li || !indices_out || (counted && !counts_out)) return fail(m, RR_ERR_BAD_ARG, "%s: null argument", what);
  RR_TRY(bank_usable(m, what, b));
  if (pruned && !b->has_codes()) return fail(m, RR_ERR_UNSUPPORTED, "%s: an fp16 bank (compressed banks only: the stages read the centroid codes)", what);
  if (m->cfg.li_dim % 16) return fail(m, RR_ERR_UNSUPPORTED, "%s: li_dim %d (a multiple of 16)", what, m->cfg.li_dim);
  if (((uintptr_t)query_li) & 15) return fail(m, RR_ERR_BAD_ARG, "%s: query_li must be 16-byte aligned", what);
  if ((((uintptr_t)indices_out) | ((uintptr_t)scores_out) | ((uintptr_t)counts_out)) & 3) return fail(m, RR_ERR_BAD_ARG, "%s: misaligned output", what);
  if (n_queries <= 0 || n_queries > 65535 || Lq <= 0) return fail(m, RR_ERR_BAD_SHAPE, "%s: n_queries=%d (1..65535) Lq=%d", what, n_queries, Lq);
  const long long held = (long long)b->first.size(), n_ll = n_passages == -1 ? held - (long long)first_passage : (long long)n_passages;
  if (first_passage < 0 || n_ll <= 0 || (long long)first_passage + n_ll > held)
    return fail(m, RR_ERR_BAD_SHAPE, "%s: passages [%d, %d + %lld) of a bank that holds %lld", what, first_passage, first_passage, n_ll, held);
  *n = (int)n_ll;
  RR_TRY(limits(*n));
  RR_TRY(capture_guard(m, st, "%s cannot be captured into a graph (it may upload the bank's passage table and grow its block)", what));
  RR_HIP(m, hipSetDevice(m->cfg.device));
  RR_TRY(bank_table_current(m, b, st));
  const size_t last = (size_t)first_passage + (size_t)*n - 1;
  *rows = (double)(b->first[last] + b->len[last] - b->first[(size_t)first_passage]);
  return RR_OK;
}

// A caller's filter as the three filtered searches (`what`) check it, behind their other refusals ("CANDIDATE FILTERS",
// include/rerank_mi355.h); np: the passages of the resolved range
struct FilterArg { const uint32_t* bits; int rows; int64_t ld; };
static int bank_filter_check(rr_model* m, const char* what, const FilterArg& f, int n_queries, int32_t first_passage, int np) {
  if (!f.bits) return fail(m, RR_ERR_BAD_ARG, "%s: null filter_bits (the unfiltered entry takes no filter)", what);
  if (((uintptr_t)f.bits) & 3) return fail(m, RR_ERR_BAD_ARG, "%s: misaligned filter_bits", what);
  if (f.rows != 1 && f.rows != n_queries) return fail(m, RR_ERR_BAD_SHAPE, "%s: filter_rows=%d (1 or n_queries=%d)", what, f.rows, n_queries);
  const long long need = ((long long)first_passage + np + 31) / 32;
  if (f.ld < need)
    return fail(m, RR_ERR_BAD_SHAPE, "%s: filter_ld=%lld words, passages [%d, %d + %d) take %lld", what, (long long)f.ld, first_passage,
                first_passage, np, need);
  return RR_OK;
}

// rr_set_tuning("sparse_stop_after"): the last stage an rr_bank_search_filtered_sparse call runs (0 the compaction, 1 the scores, 2
// all); below 2 the outputs are not written: tools/bench_bank_search_filter.py --sparse --profile times the stages by difference.
// A diagnostic switch, set between calls (as the pruned search's).
static int g_sparse_stop_after = 2;
int set_sparse_stop_after(int value) {
  if (value < 0 || value > 2) return RR_ERR_BAD_ARG;
  g_sparse_stop_after = value;
  return RR_OK;
}

// rr_bank_search (include/rerank_mi355.h): one scoring launch over the range and the selection passes.  filter (or null):
// rr_bank_search_filtered, the scores under the filter, the same selection, then one list pass that drops the absent and counts.
// sparse (with a filter): rr_bank_search_filtered_sparse, the same checks in the same order, then the filter's rows compacted into
// candidate lists, the scores of their places and the counted selection: every stage over the allowed passages alone
static int bank_search_call(rr_handle h, rr_bank* b, const float* query_li, int n_queries, int Lq, int32_t first_passage,
                            int32_t n_passages, int k, const FilterArg* filter, bool sparse, int32_t* indices_out, float* scores_out,
                            int32_t* counts_out, void* hip_stream) {
  const char* what = sparse ? "rr_bank_search_filtered_sparse" : filter ? "rr_bank_search_filtered" : "rr_bank_search";
  if (!h) return RR_ERR_BAD_ARG;
  rr_model* m = h;
  hipStream_t st = (hipStream_t)hip_stream;
  int n = 0;
  double rows = 0.0;
  RR_TRY(bank_search_begin(m, what, false, filter != nullptr, b, query_li, n_queries, Lq, first_passage, n_passages, indices_out, scores_out, counts_out, st, &n,
                           &rows, [&](int np) {
                             if (k < 1 || k > np) return fail(m, RR_ERR_BAD_SHAPE, "%s: k=%d of %d passages", what, k, np);
                             if (k > 1024) return fail(m, RR_ERR_UNSUPPORTED, "%s: k=%d (at most 1024: a selection pass keeps k of 4096)", what, k);
                             return filter ? bank_filter_check(m, what, *filter, n_queries, first_passage, np) : (int)RR_OK;
                           }));
  const int D = m->cfg.li_dim;
  const size_t sc_bytes = (((size_t)n_queries * n * sizeof(float)) + 15) & ~(size_t)15;
  const size_t tmp_bytes = ((rr_topk_select_scratch(n_queries, n, k) * sizeof(int32_t)) + 15) & ~(size_t)15;
  const size_t top_bytes = filter ? (((size_t)n_queries * k * sizeof(int32_t)) + 15) & ~(size_t)15 : 0;      // the selection's k, before the list pass
  // (the sparse form: the dense form's bytes, so that calls of both forms grow the block once, then cand [filter_rows][n] and cnt)
  const size_t cand_bytes = sparse ? (((size_t)filter->rows * n * sizeof(int32_t)) + 15) & ~(size_t)15 : 0;
  const size_t cnt_bytes = sparse ? (((size_t)filter->rows * sizeof(int32_t)) + 15) & ~(size_t)15 : 0;
  RR_TRY(ensure_block(m, m->search_blk, m->search_blk_cap, sc_bytes + 2 * tmp_bytes + top_bytes + cand_bytes + cnt_bytes, st,
                      "the bank search's block"));
  m->plaid_last_ok = false;                         // the block no longer holds a pruned search's intermediates
  float* sc = (float*)m->search_blk;
  int32_t* tmp_a = tmp_bytes ? (int32_t*)(m->search_blk + sc_bytes) : nullptr;
  int32_t* tmp_b = tmp_bytes ? (int32_t*)(m->search_blk + sc_bytes + tmp_bytes) : nullptr;
  m->last_stream = st;
  const rr_bank_view bank = bank_view(b);
  // bytes: the range's rows and mask bytes once (the queries of a chunk run side by side), the table, the query block per
  // workgroup of 16 passages, one float per (query, passage)
  const double bytes = rows * (rr_bank_row_bytes(bank, D) + 1.0) + 16.0 * n + (double)n_queries * (n / 16.0 + 1.0) * 4.0 * Lq * D + 4.0 * n_queries * (double)n;
  if (sparse) {
    // how many passages a row allows is known on the device only: FLOPs and bytes are booked for the range's mean passage length
    // times the pitch, an upper bound (as the pruned search books its survivors)
    int32_t* cand = (int32_t*)(m->search_blk + sc_bytes + 2 * tmp_bytes + top_bytes);
    int32_t* cnt = (int32_t*)(m->search_blk + sc_bytes + 2 * tmp_bytes + top_bytes + cand_bytes);
    const rr_passage_filter f{filter->bits, filter->rows, (long long)filter->ld, first_passage};
    RR_RUN(m, st, RR_K_TAIL, 0.0, (double)filter->rows * (n / 8.0 + 4.0 * n + 4.0), rr_launch_filter_compact(f, n, cand, cnt, st));
    if (g_sparse_stop_after < 1) return RR_OK;
    RR_RUN(m, st, RR_K_TAIL, 2.0 * n_queries * rows * Lq * D, bytes + 4.0 * n_queries * (double)n,
           rr_launch_bank_search_scores_places(b->table + first_passage, n, n_queries, Lq, D, query_li, bank, cand, cnt, filter->rows, n, sc, st));
    if (g_sparse_stop_after < 2) return RR_OK;
    RR_RUN(m, st, RR_K_TAIL, 0.0, 12.0 * n_queries * (double)n + 16.0 * n_queries * (double)k,
           rr_launch_topk_select_counted(sc, n_queries, n, cnt, cand, (long long)n, filter->rows, k, first_passage, tmp_a, tmp_b, indices_out,
                                         scores_out, counts_out, st));
    return RR_OK;
  }
  RR_RUN(m, st, RR_K_TAIL, 2.0 * n_queries * rows * Lq * D, bytes,
         rr_launch_bank_search_scores(b->table + first_passage, n, n_queries, Lq, D, query_li, bank,
                                      filter ? rr_passage_filter{filter->bits, filter->rows, (long long)filter->ld, first_passage} : rr_passage_filter{},
                                      sc, st));
  if (!filter) {
    RR_RUN(m, st, RR_K_TAIL, 0.0, 12.0 * n_queries * (double)n,
           rr_launch_topk_select(sc, n_queries, n, k, first_passage, tmp_a, tmp_b, indices_out, scores_out, st));
    return RR_OK;
  }
  int32_t* top = (int32_t*)(m->search_blk + sc_bytes + 2 * tmp_bytes);
  RR_RUN(m, st, RR_K_TAIL, 0.0, 12.0 * n_queries * (double)n, rr_launch_topk_select(sc, n_queries, n, k, 0, tmp_a, tmp_b, top, nullptr, st));
  RR_RUN(m, st, RR_K_TAIL, 0.0, 16.0 * n_queries * (double)k,
         rr_launch_list_select(sc, (long long)n, n_queries, top, k, k, indices_out, counts_out, first_passage, scores_out, st));
  return RR_OK;
}

// rr_set_tuning("f16_stop_after"): the last stage an rr_bank_search_f16 or rr_bank_search_f16_plaid call runs (0 the approximate scores, 1 the survivors, 2 their
// exact scores, 3 all); below 3 the outputs are not written: tools/bench_bank_search_f16.py times the stages by difference.  A
// diagnostic switch, set between calls (as the sparse form's).
static int g_f16_stop_after = 3;
int set_f16_stop_after(int value) {
  if (value < 0 || value > 3) return RR_ERR_BAD_ARG;
  g_f16_stop_after = value;
  return RR_OK;
}

// rr_bank_search_f16 and, `plaid`, rr_bank_search_f16_plaid (include/rerank_mi355.h): A over the range on the fp16 matrix core, its
// m = min(ndocs, n) first per query, their exact scores by the listed form of rr_bank_search's kernel, the first k of those, and the
// certificate.  One function under both entries: the kind of bank each takes and the launch that writes A are all that differ (the
// listed kernel reads fp16 and compressed rows alike, as stage 3 of the pruned search has it).
static int bank_search_f16_call(rr_handle h, bool plaid, rr_bank* b, const float* query_li, int n_queries, int Lq, int32_t first_passage, int32_t n_passages,
                                int ndocs, int k, float slack, int32_t* indices_out, float* scores_out, int32_t* certified_out, void* hip_stream) {
  const char* what = plaid ? "rr_bank_search_f16_plaid" : "rr_bank_search_f16";
  if (!h) return RR_ERR_BAD_ARG;
  rr_model* m = h;
  hipStream_t st = (hipStream_t)hip_stream;
  int n = 0;
  double rows = 0.0;
  RR_TRY(bank_search_begin(m, what, false, true, b, query_li, n_queries, Lq, first_passage, n_passages, indices_out, scores_out, certified_out, st, &n,
                           &rows, [&](int np) {
                             if (k < 1 || k > ndocs || k > np) return fail(m, RR_ERR_BAD_SHAPE, "%s: k=%d ndocs=%d of %d passages", what, k, ndocs, np);
                             if (ndocs > 1024) return fail(m, RR_ERR_UNSUPPORTED, "%s: ndocs=%d (at most 1024: a selection pass keeps ndocs of 4096)", what, ndocs);
                             if (!(slack >= 0.0f)) return fail(m, RR_ERR_BAD_ARG, "%s: slack=%g (>= 0, not NaN)", what, (double)slack);
                             if (plaid) {
                               if (!bank_view(b).nbits) return fail(m, RR_ERR_UNSUPPORTED, "%s: an fp16 bank (compressed banks only: rr_bank_search_f16 searches an fp16 bank)", what);
                               if (!rr_bank_scores_f16_plaid_dim_ok(m->cfg.li_dim))
                                 return fail(m, RR_ERR_UNSUPPORTED, "%s: li_dim %d (32, 64, 128 or 256: the decoded tiles must fit the LDS)", what, m->cfg.li_dim);
                               return (int)RR_OK;
                             }
                             if (bank_view(b).nbits) return fail(m, RR_ERR_UNSUPPORTED, "%s: a compressed bank (fp16 banks only: the first pass reads fp16 rows)", what);
                             if (m->cfg.li_dim % 32) return fail(m, RR_ERR_UNSUPPORTED, "%s: li_dim %d (a multiple of 32)", what, m->cfg.li_dim);
                             return (int)RR_OK;
                           }));
  const int D = m->cfg.li_dim, nd = std::min(ndocs, n);
  auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
  const size_t sc_bytes = up((size_t)n_queries * n * sizeof(float));                             // A, and E behind it
  const size_t tmp_bytes = up(rr_topk_select_scratch(n_queries, n, nd) * sizeof(int32_t));
  const size_t surv_bytes = up((size_t)n_queries * nd * sizeof(int32_t)), cnt_bytes = up((size_t)n_queries * sizeof(int32_t));
  const size_t ks_bytes = scores_out ? 0 : up((size_t)n_queries * k * sizeof(float));           // the certificate reads the k-th score
  RR_TRY(ensure_block(m, m->search_blk, m->search_blk_cap, 2 * sc_bytes + 2 * tmp_bytes + surv_bytes + 2 * cnt_bytes + ks_bytes, st,
                      "the bank search's block"));
  m->plaid_last_ok = false;                         // the block no longer holds a pruned search's intermediates
  char* p = m->search_blk;
  float* A = (float*)p;
  float* E = (float*)(p + sc_bytes);
  int32_t* tmp_a = tmp_bytes ? (int32_t*)(p + 2 * sc_bytes) : nullptr;
  int32_t* tmp_b = tmp_bytes ? (int32_t*)(p + 2 * sc_bytes + tmp_bytes) : nullptr;
  int32_t* surv = (int32_t*)(p + 2 * sc_bytes + 2 * tmp_bytes);
  int32_t* cnt_in = (int32_t*)(p + 2 * sc_bytes + 2 * tmp_bytes + surv_bytes);
  int32_t* cnt_out = (int32_t*)(p + 2 * sc_bytes + 2 * tmp_bytes + surv_bytes + cnt_bytes);
  float* ks = scores_out ? scores_out : (float*)(p + 2 * sc_bytes + 2 * tmp_bytes + surv_bytes + 2 * cnt_bytes);
  m->last_stream = st;
  const rr_bank_view bank = bank_view(b);
  const rr_bank_slot* table = b->table + first_passage;
  const double tiles = std::ceil(Lq / 16.0);
  // A: the rows and mask bytes once (the query blocks of a chunk run side by side), the table, the query block per workgroup of 32
  // passages, one float per (query, passage); FLOPs of whole column tiles are what the matrix core runs, Lq columns what is booked
  // (a compressed row: its residual bytes, its code, its mask byte and the centroid it names: rr_bank_row_bytes)
  RR_RUN(m, st, RR_K_TAIL, 2.0 * n_queries * rows * Lq * D, rows * (rr_bank_row_bytes(bank, D) + 1.0) + 16.0 * n + (n / 32.0 + 1.0) * n_queries * tiles * 16.0 * 4.0 * D + 4.0 * n_queries * (double)n,
         plaid ? rr_launch_bank_scores_f16_plaid(table, n, n_queries, Lq, D, query_li, bank, A, st)
               : rr_launch_bank_scores_f16(table, n, n_queries, Lq, D, query_li, bank, A, st));
  if (g_f16_stop_after < 1) return RR_OK;
  RR_RUN(m, st, RR_K_TAIL, 0.0, 12.0 * n_queries * (double)n, rr_launch_topk_select(A, n_queries, n, nd, 0, tmp_a, tmp_b, surv, nullptr, st));
  if (g_f16_stop_after < 2) return RR_OK;
  RR_HIP(m, hipMemsetD32Async((hipDeviceptr_t)cnt_in, nd, (size_t)n_queries, st));      // every query's list is full
  // E: booked for the range's mean passage length, as the pruned search books its survivors
  const double srows = rows / n * nd * n_queries;
  RR_RUN(m, st, RR_K_TAIL, 2.0 * srows * Lq * D, srows * (rr_bank_row_bytes(bank, D) + 1.0) + (double)n_queries * nd * (20.0 + Lq * D),
         rr_launch_bank_search_scores_listed(table, n, n_queries, Lq, D, query_li, bank, surv, nd, cnt_in, nullptr, 0, E, st));
  if (g_f16_stop_after < 3) return RR_OK;
  RR_RUN(m, st, RR_K_TAIL, 0.0, 16.0 * n_queries * (double)nd,
         rr_launch_list_select(E, (long long)n, n_queries, surv, nd, k, indices_out, cnt_out, first_passage, ks, st));
  RR_RUN(m, st, RR_K_TAIL, 0.0, 24.0 * n_queries,
         rr_launch_f16_certify(A, (long long)n, surv, nd, ks, cnt_out, k, slack, n_queries, certified_out, st));
  return RR_OK;
}

// the scratch of the diagnostic search operators: allocated per call and freed behind a synchronisation of the stream
static int op_select_with_scratch(const float* scores, int n_lists, int n, int k, int add, int32_t* indices_out, float* scores_out, hipStream_t st) {
  const size_t entries = rr_topk_select_scratch(n_lists, n, k);
  int32_t* tmp = nullptr;
  if (entries && hipMalloc((void**)&tmp, 2 * entries * sizeof(int32_t)) != hipSuccess) { (void)hipGetLastError(); return RR_ERR_OOM; }
  hipError_t e = rr_launch_topk_select(scores, n_lists, n, k, add, tmp, tmp ? tmp + entries : nullptr, indices_out, scores_out, st);
  if (tmp) {
    const hipError_t e2 = hipStreamSynchronize(st);
    if (e == hipSuccess) e = e2;
    (void)hipFree(tmp);
  }
  return e == hipSuccess ? RR_OK : RR_ERR_HIP;
}

int rr_op_topk_select(const float* scores, int n_lists, int n, int k, int32_t* indices_out, float* scores_out, void* hip_stream) {
  return guarded(nullptr, [&]() -> int {
    if (!scores || !indices_out) return RR_ERR_BAD_ARG;
    if (n_lists <= 0 || n_lists > 65535 || n <= 0 || k < 1 || k > n) return RR_ERR_BAD_SHAPE;
    if (k > 1024) return RR_ERR_UNSUPPORTED;
    return op_select_with_scratch(scores, n_lists, n, k, 0, indices_out, scores_out, (hipStream_t)hip_stream);
  });
}

// rr_op_filter_compact and rr_op_topk_select_counted (include/rerank_mi355_diag.h): the first and the last stage of
// rr_bank_search_filtered_sparse over loose device pointers
int rr_op_filter_compact(const uint32_t* filter_bits, int filter_rows, int64_t filter_ld, int32_t first_passage, int32_t n_passages,
                         int32_t* cand_out, int32_t* counts_out, void* hip_stream) {
  return guarded(nullptr, [&]() -> int {
    if (!filter_bits || !cand_out || !counts_out) return RR_ERR_BAD_ARG;
    if ((((uintptr_t)filter_bits) | ((uintptr_t)cand_out) | ((uintptr_t)counts_out)) & 3) return RR_ERR_BAD_ARG;
    if (filter_rows < 1 || filter_rows > 65535 || first_passage < 0 || n_passages < 1 ||
        filter_ld < ((long long)first_passage + n_passages + 31) / 32)
      return RR_ERR_BAD_SHAPE;
    const rr_passage_filter f{filter_bits, filter_rows, (long long)filter_ld, first_passage};
    return rr_launch_filter_compact(f, n_passages, cand_out, counts_out, (hipStream_t)hip_stream) == hipSuccess ? RR_OK : RR_ERR_HIP;
  });
}

int rr_op_topk_select_counted(const float* scores, int n_lists, int n, const int32_t* counts, const int32_t* cand, int rows, int k,
                              int32_t first_passage, int32_t* indices_out, float* scores_out, int32_t* counts_out, void* hip_stream) {
  return guarded(nullptr, [&]() -> int {
    if (!scores || !counts || !indices_out || !counts_out) return RR_ERR_BAD_ARG;
    if (n_lists <= 0 || n_lists > 65535 || n <= 0 || k < 1 || k > n || (rows != 1 && rows != n_lists)) return RR_ERR_BAD_SHAPE;
    if (k > 1024) return RR_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t entries = rr_topk_select_scratch(n_lists, n, k);
    int32_t* tmp = nullptr;
    if (entries && hipMalloc((void**)&tmp, 2 * entries * sizeof(int32_t)) != hipSuccess) { (void)hipGetLastError(); return RR_ERR_OOM; }
    hipError_t e = rr_launch_topk_select_counted(scores, n_lists, n, counts, cand, (long long)n, rows, k, first_passage, tmp,
                                                 tmp ? tmp + entries : nullptr, indices_out, scores_out, counts_out, st);
    if (tmp) {
      const hipError_t e2 = hipStreamSynchronize(st);
      if (e == hipSuccess) e = e2;
      (void)hipFree(tmp);
    }
    return e == hipSuccess ? RR_OK : RR_ERR_HIP;
  });
}

int rr_op_bank_search(const float* query_li, int n_queries, int Lq, int D, const void* table, int32_t first_passage, int32_t n_passages, int k,
                      const uint16_t* rows_f16, const uint8_t* mask_bytes, int nbits, const int32_t* codes, const uint8_t* residuals,
                      const uint16_t* centroids_f16, const float* bucket_weights, int32_t n_centroids, int32_t* indices_out, float* scores_out,
                      void* hip_stream) {
  return guarded(nullptr, [&]() -> int {
    if (!query_li || !table || !mask_bytes || !indices_out) return RR_ERR_BAD_ARG;
    if (nbits ? (!codes || !residuals || !centroids_f16 || !bucket_weights) : !rows_f16) return RR_ERR_BAD_ARG;
    if ((((uintptr_t)query_li) | ((uintptr_t)table)) & 15) return RR_ERR_BAD_ARG;
    if (D <= 0 || D % 16 || (nbits && !rr_plaid_shape_ok(nbits, D))) return RR_ERR_UNSUPPORTED;
    if (n_queries <= 0 || n_queries > 65535 || Lq <= 0 || first_passage < 0 || n_passages <= 0 || (nbits && n_centroids <= 0) || k < 1 || k > n_passages)
      return RR_ERR_BAD_SHAPE;
    if (k > 1024) return RR_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)hip_stream;
    float* sc = nullptr;
    if (hipMalloc((void**)&sc, (size_t)n_queries * n_passages * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); return RR_ERR_OOM; }
    const rr_bank_slot* t = (const rr_bank_slot*)table + first_passage;
    const rr_bank_view bank{nbits, n_centroids, rows_f16, codes, residuals, centroids_f16, bucket_weights, mask_bytes};
    const hipError_t e = rr_launch_bank_search_scores(t, n_passages, n_queries, Lq, D, query_li, bank, rr_passage_filter{}, sc, st);
    int rc = e == hipSuccess ? op_select_with_scratch(sc, n_queries, n_passages, k, first_passage, indices_out, scores_out, st) : RR_ERR_HIP;
    if (hipStreamSynchronize(st) != hipSuccess && rc == RR_OK) rc = RR_ERR_HIP;
    (void)hipFree(sc);
    return rc;
  });
}

// rr_op_bank_scores_f16 (include/rerank_mi355_diag.h): the first pass of rr_bank_search_f16 over raw device pointers
int rr_op_bank_scores_f16(const float* query_li, int n_queries, int Lq, int D, const void* table, int32_t first_passage, int32_t n_passages,
                          const uint16_t* rows_f16, const uint8_t* mask_bytes, float* scores_out, void* hip_stream) {
  return guarded(nullptr, [&]() -> int {
    if (!query_li || !table || !rows_f16 || !mask_bytes || !scores_out) return RR_ERR_BAD_ARG;
    if ((((uintptr_t)query_li) | ((uintptr_t)table) | ((uintptr_t)rows_f16)) & 15) return RR_ERR_BAD_ARG;
    if (D <= 0 || D % 32) return RR_ERR_UNSUPPORTED;
    if (n_queries <= 0 || n_queries > 65535 || Lq <= 0 || first_passage < 0 || n_passages <= 0) return RR_ERR_BAD_SHAPE;
    const rr_bank_view bank{0, 0, rows_f16, nullptr, nullptr, nullptr, nullptr, mask_bytes};
    const hipError_t e = rr_launch_bank_scores_f16((const rr_bank_slot*)table + first_passage, n_passages, n_queries, Lq, D, query_li, bank, scores_out,
                                                   (hipStream_t)hip_stream);
    return e == hipSuccess ? RR_OK : RR_ERR_HIP;
  });
}

// rr_op_bank_scores_f16_plaid (include/rerank_mi355_diag.h): the first pass of rr_bank_search_f16_plaid over raw device pointers
int rr_op_bank_scores_f16_plaid(const float* query_li, int n_queries, int Lq, int D, const void* table, int32_t first_passage, int32_t n_passages,
                                const uint8_t* mask_bytes, int nbits, const int32_t* codes, const uint8_t* residuals, const uint16_t* centroids_f16,
                                const float* bucket_weights, int32_t n_centroids, float* scores_out, void* hip_stream) {
  return guarded(nullptr, [&]() -> int {
    if (!query_li || !table || !mask_bytes || !codes || !residuals || !centroids_f16 || !bucket_weights || !scores_out) return RR_ERR_BAD_ARG;
    if (((((uintptr_t)query_li) | ((uintptr_t)table) | ((uintptr_t)centroids_f16)) & 15) || (((uintptr_t)residuals) & 7) || (((uintptr_t)codes) & 3))
      return RR_ERR_BAD_ARG;
    if (!rr_bank_scores_f16_plaid_dim_ok(D) || !rr_plaid_shape_ok(nbits, D)) return RR_ERR_UNSUPPORTED;
    if (n_queries <= 0 || n_queries > 65535 || Lq <= 0 || first_passage < 0 || n_passages <= 0 || n_centroids <= 0) return RR_ERR_BAD_SHAPE;
    const rr_bank_view bank{nbits, n_centroids, nullptr, codes, residuals, centroids_f16, bucket_weights, mask_bytes};
    const hipError_t e = rr_launch_bank_scores_f16_plaid((const rr_bank_slot*)table + first_passage, n_passages, n_queries, Lq, D, query_li, bank,
                                                         scores_out, (hipStream_t)hip_stream);
    return e == hipSuccess ? RR_OK : RR_ERR_HIP;
  });
}

// rr_op_bank_scores_f16_form (include/rerank_mi355_diag.h): the launch form of either first pass; host arithmetic, no device
int rr_op_bank_scores_f16_form(int n_queries, int Lq, int D, int plaid, int* nt_out, int* tp_out, int* passes_out) {
  return guarded(nullptr, [&]() -> int {
    if (!nt_out || !tp_out || !passes_out) return RR_ERR_BAD_ARG;
    if (plaid ? !rr_bank_scores_f16_plaid_dim_ok(D) : (D <= 0 || D % 32)) return RR_ERR_UNSUPPORTED;      // the operators' checks, in their order
    if (n_queries <= 0 || n_queries > 65535 || Lq <= 0) return RR_ERR_BAD_SHAPE;
    const hipError_t e = plaid ? rr_bank_scores_f16_plaid_form(n_queries, Lq, D, nt_out, tp_out, passes_out)
                               : rr_bank_scores_f16_form(n_queries, Lq, D, nt_out, tp_out, passes_out);
    return e == hipSuccess ? RR_OK : RR_ERR_HIP;
  });
}

// rr_set_tuning("plaid_stop_after") [0] and ("plaid_ivf_stop_after") [1]: the last stage an rr_bank_search_plaid call (7: all) and
// an rr_bank_search_plaid_ivf call (8: all) runs; below it the outputs are not written: tools/bench_bank_search_plaid.py times the
// stages by difference.  Diagnostic switches, set between calls (as g_op_dt).
static const int g_plaid_stages[2] = {RR_PLAID_SEARCH_STAGES, RR_PLAID_IVF_SEARCH_STAGES};
static int g_plaid_stop_after[2] = {RR_PLAID_SEARCH_STAGES - 1, RR_PLAID_IVF_SEARCH_STAGES - 1};
int set_plaid_stop_after(bool ivf, int value) {
  if (value < 0 || value >= g_plaid_stages[ivf]) return RR_ERR_BAD_ARG;
  g_plaid_stop_after[ivf] = value;
  return RR_OK;
}

// what rr_bank_search_plaid and rr_op_bank_search_plaid refuse alike, in the order the header gives; msg: the sentence for the handle
static int plaid_search_limits(int n_centroids, int n, int Lq, int Lq_coarse, int ncells, int ndocs, int k, const char** msg) {
  *msg = "";
  if (Lq_coarse < 1 || Lq_coarse > Lq) { *msg = "1 <= Lq_coarse <= Lq"; return RR_ERR_BAD_SHAPE; }
  if (ncells < 1 || ncells > n_centroids) { *msg = "1 <= ncells <= n_centroids"; return RR_ERR_BAD_SHAPE; }
  if (ncells > 16) { *msg = "ncells at most 16"; return RR_ERR_UNSUPPORTED; }
  if (ndocs < 4) { *msg = "ndocs at least 4"; return RR_ERR_BAD_SHAPE; }
  if (ndocs > 1024) { *msg = "ndocs at most 1024 (the selection kernel keeps at most 1024 of a slice)"; return RR_ERR_UNSUPPORTED; }
  if (k < 1 || k > std::min(ndocs / 4, n)) { *msg = "1 <= k <= min(ndocs / 4, n_passages)"; return RR_ERR_BAD_SHAPE; }
  if (n_centroids > RR_PLAID_SEARCH_MAX_CENTROIDS) { *msg = "more than 262144 centroids"; return RR_ERR_UNSUPPORTED; }
  return RR_OK;
}

// What the stages of a pruned search (bank_search_plaid.hip) are booked with: flops / bytes [l.stages]; rows: the rows of the range.
// FLOPs: stage 0 exactly; the exact scores for ndocs / 4 survivors of the range's mean length (their number is known on the device
// only: an upper bound).  Bytes: what a stage must read and write once.
static void plaid_search_costs(const rr_plaid_search_args& a, const rr_plaid_search_layout& l, double rows, double* flops, double* bytes) {
  const int n = a.n, Lq = a.Lq, D = a.D;
  const double nq = a.nq, C = l.Cp, SLq = 4.0 * a.Lqc, cap = l.cap, pitch = l.pitch;
  std::fill(flops, flops + l.stages, 0.0);
  flops[0] = 2.0 * nq * C * Lq * D;
  bytes[0] = 2.0 * C * D + nq * (4.0 * Lq * D + 4.0 * C * Lq);
  bytes[1] = nq * C * SLq * std::min(a.ncells, 2);
  bytes[2] = nq * C * SLq;
  int s = 3;
  if (l.stages == RR_PLAID_IVF_SEARCH_STAGES) {
    // the candidate step clears, sets and reads a bitmap of the range per query and writes the lists and the -inf behind them (the
    // postings it reads are known on the device only); the listed scores read about 5 bytes per row of a candidate (at most cap of
    // them: an upper bound)
    bytes[s++] = nq * (n / 8.0 * 3.0 + 12.0 * cap);
    bytes[s++] = nq * cap * (5.0 * (rows / n) + 28.0);
  } else {
    bytes[s++] = 5.0 * rows + 16.0 * n + 8.0 * nq * n;      // the scan's candidates add a row of S per unmasked row
  }
  bytes[s++] = 12.0 * nq * pitch;                            // the selection reads the A1 row
  bytes[s++] = 16.0 * nq * l.k1;
  flops[s] = 2.0 * nq * l.k2 * (rows / n) * Lq * D;
  bytes[s++] = nq * l.k2 * (rows / n) * (rr_bank_row_bytes(a.bank, D) + 1.0);
  bytes[s++] = 16.0 * nq * l.k2;
}

// rr_bank_search_plaid (include/rerank_mi355.h): the block, and the stages of bank_search_plaid.hip, each booked on its own.
// ivf: rr_bank_search_plaid_ivf, the same checks, one more refusal, and the plan that reads the bank's inverted file
static int bank_search_plaid_call(rr_handle h, bool ivf, rr_bank* b, const float* query_li, int n_queries, int Lq, int Lq_coarse,
                                  int32_t first_passage, int32_t n_passages, int ncells, float threshold, int ndocs, int k,
                                  const FilterArg* filter, int32_t* indices_out, float* scores_out, int32_t* counts_out, void* hip_stream) {
  const char* what = filter ? (ivf ? "rr_bank_search_plaid_ivf_filtered" : "rr_bank_search_plaid_filtered")
                            : (ivf ? "rr_bank_search_plaid_ivf" : "rr_bank_search_plaid");
  if (!h) return RR_ERR_BAD_ARG;
  rr_model* m = h;
  hipStream_t st = (hipStream_t)hip_stream;
  int n = 0;
  double rows = 0.0;
  RR_TRY(bank_search_begin(m, what, true, true, b, query_li, n_queries, Lq, first_passage, n_passages, indices_out, scores_out, counts_out, st, &n, &rows,
                           [&](int np) {
                             const char* msg;
                             const int rc = plaid_search_limits(b->n_centroids, np, Lq, Lq_coarse, ncells, ndocs, k, &msg);
                             if (rc)
                               return fail(m, rc, "%s: %s (Lq=%d Lq_coarse=%d ncells=%d ndocs=%d k=%d, %d passages, %d centroids)", what, msg, Lq,
                                           Lq_coarse, ncells, ndocs, k, np, b->n_centroids);
                             if (ivf && !b->ivf.passages)
                               return fail(m, RR_ERR_UNSUPPORTED, "%s: the bank has no inverted file: call rr_bank_build_ivf first", what);
                             if (ivf && (long long)first_passage + np > b->ivf.passages)
                               return fail(m, RR_ERR_UNSUPPORTED, "%s: passages [%d, %d + %d) reach beyond the %d the inverted file covers: call "
                                           "rr_bank_build_ivf again", what, first_passage, first_passage, np, b->ivf.passages);
                             return filter ? bank_filter_check(m, what, *filter, n_queries, first_passage, np) : (int)RR_OK;
                           }));
  const int D = m->cfg.li_dim;
  // (a file none of whose lists has an entry still takes the inverted-file form: its rows are one entry wide at the least)
  const rr_plaid_search_layout l = rr_plaid_search_plan(n_queries, n, b->n_centroids, Lq, Lq_coarse, ncells, ndocs,
                                                        ivf ? std::max(b->ivf.longest, 1) : 0);
  m->plaid_last_ok = false;
  RR_TRY(ensure_block(m, m->search_blk, m->search_blk_cap, l.total, st, "the bank search's block"));
  m->last_stream = st;
  const rr_plaid_search_args a{n_queries, n, first_passage, Lq, Lq_coarse, D, ncells, ndocs, k, threshold, query_li, b->table + first_passage,
                               bank_view(b), m->search_blk, indices_out, scores_out, counts_out, ivf ? b->ivf : rr_ivf{},
                               filter ? rr_passage_filter{filter->bits, filter->rows, (long long)filter->ld, first_passage} : rr_passage_filter{}};
  double flops[RR_PLAID_IVF_SEARCH_STAGES], bytes[RR_PLAID_IVF_SEARCH_STAGES];
  plaid_search_costs(a, l, rows, flops, bytes);
  const int stop = g_plaid_stop_after[ivf];
  for (int s = 0; s < l.stages && s <= stop; ++s)
    RR_RUN(m, st, RR_K_TAIL, flops[s], bytes[s], rr_launch_plaid_search_stage(s, a, l, st));
  if (ivf) return RR_OK;                            // (no tap: plaid_last_ok stays false)
  m->plaid_last = a;
  m->plaid_last_layout = l;
  m->plaid_last_ok = true;
  return RR_OK;
}

// rr_bank_search_plaid_tap (include/rerank_mi355_diag.h): one intermediate of the handle's last pruned search, copied to the host
static int64_t bank_search_plaid_tap(rr_handle h, const char* name, void* host_out, int64_t max_bytes) {
  if (!h || !name || !host_out) return RR_ERR_BAD_ARG;
  rr_model* m = h;
  if (!m->plaid_last_ok) return fail(m, RR_ERR_BAD_ARG, "rr_bank_search_plaid_tap: no rr_bank_search_plaid call since the last search of this handle");
  const rr_plaid_search_args& a = m->plaid_last;
  const rr_plaid_search_layout& l = m->plaid_last_layout;
  const int C = a.bank.n_centroids;
  if (hipSetDevice(m->cfg.device) != hipSuccess || hipStreamSynchronize(m->last_stream) != hipSuccess) return fail(m, RR_ERR_HIP, "stream sync failed");
  const std::string nm = name;
  auto fetch = [&](size_t off, size_t bytes, void* dst) { return hipMemcpy(dst, a.scratch + off, bytes, hipMemcpyDeviceToHost) == hipSuccess; };
  auto room = [&](size_t bytes) { return (int64_t)bytes <= max_bytes; };
  if (nm == "S") {                       // float32 [nq][C][Lq_coarse]
    const size_t out = (size_t)a.nq * C * a.Lqc * 4;
    if (!room(out)) return fail(m, RR_ERR_BAD_SHAPE, "buffer too small");
    std::vector<float> t((size_t)a.nq * l.Cp * a.Lq);
    if (!fetch(l.S, t.size() * 4, t.data())) return RR_ERR_HIP;
    float* o = (float*)host_out;
    for (int q = 0; q < a.nq; ++q)
      for (int cc = 0; cc < C; ++cc)
        memcpy(o + ((size_t)q * C + cc) * a.Lqc, t.data() + ((size_t)q * l.Cp + cc) * a.Lq, (size_t)a.Lqc * 4);
    return (int64_t)out;
  }
  if (nm == "cells" || nm == "keep") {   // uint8 [nq][C]
    const size_t out = (size_t)a.nq * C;
    if (!room(out)) return fail(m, RR_ERR_BAD_SHAPE, "buffer too small");
    std::vector<uint32_t> t((size_t)a.nq * l.W);
    if (!fetch(nm == "cells" ? l.cellbits : l.keepbits, t.size() * 4, t.data())) return RR_ERR_HIP;
    uint8_t* o = (uint8_t*)host_out;
    for (int q = 0; q < a.nq; ++q)
      for (int cc = 0; cc < C; ++cc) o[(size_t)q * C + cc] = (t[(size_t)q * l.W + (cc >> 5)] >> (cc & 31)) & 1u;
    return (int64_t)out;
  }
  if (nm == "a1") {                      // float32 [nq][n]
    const size_t out = (size_t)a.nq * a.n * 4;
    if (!room(out)) return fail(m, RR_ERR_BAD_SHAPE, "buffer too small");
    return fetch(l.a1, out, host_out) ? (int64_t)out : (int64_t)RR_ERR_HIP;
  }
  if (nm == "list1") {                   // int32 [nq][min(ndocs, n)], range-relative; -1 where the entry is no candidate
    const size_t out = (size_t)a.nq * l.k1 * 4;
    if (!room(out)) return fail(m, RR_ERR_BAD_SHAPE, "buffer too small");
    std::vector<float> a1((size_t)a.nq * a.n);
    if (!fetch(l.list1, out, host_out) || !fetch(l.a1, a1.size() * 4, a1.data())) return RR_ERR_HIP;
    int32_t* o = (int32_t*)host_out;
    for (int q = 0; q < a.nq; ++q)
      for (int i = 0; i < l.k1; ++i) {
        int32_t& e = o[(size_t)q * l.k1 + i];
        if (e < 0 || e >= a.n || a1[(size_t)q * a.n + e] == -INFINITY) e = -1;
      }
    return (int64_t)out;
  }
  if (nm == "list2") {                   // int32 [nq][min(ndocs / 4, n)], range-relative; -1 behind the survivors
    const size_t out = (size_t)a.nq * l.k2 * 4;
    if (!room(out)) return fail(m, RR_ERR_BAD_SHAPE, "buffer too small");
    return fetch(l.list2, out, host_out) ? (int64_t)out : (int64_t)RR_ERR_HIP;
  }
  return fail(m, RR_ERR_BAD_ARG, "unknown tap %s", name);
}

int rr_op_bank_search_plaid(const float* query_li, int n_queries, int Lq, int Lq_coarse, int D, const void* table, int32_t first_passage,
                            int32_t n_passages, int ncells, float threshold, int ndocs, int k, const uint8_t* mask_bytes, int nbits,
                            const int32_t* codes, const uint8_t* residuals, const uint16_t* centroids_f16, const float* bucket_weights,
                            int32_t n_centroids, int32_t* indices_out, float* scores_out, int32_t* counts_out, void* hip_stream) {
  return guarded(nullptr, [&]() -> int {
    if (!query_li || !table || !mask_bytes || !indices_out || !counts_out || !codes || !residuals || !centroids_f16 || !bucket_weights) return RR_ERR_BAD_ARG;
    if ((((uintptr_t)query_li) | ((uintptr_t)table)) & 15) return RR_ERR_BAD_ARG;
    if (!nbits || D <= 0 || D % 16 || !rr_plaid_shape_ok(nbits, D)) return RR_ERR_UNSUPPORTED;
    if (n_queries <= 0 || n_queries > 65535 || Lq <= 0 || first_passage < 0 || n_passages <= 0 || n_centroids <= 0) return RR_ERR_BAD_SHAPE;
    const char* msg;
    if (const int rc = plaid_search_limits(n_centroids, n_passages, Lq, Lq_coarse, ncells, ndocs, k, &msg)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    const rr_plaid_search_layout l = rr_plaid_search_plan(n_queries, n_passages, n_centroids, Lq, Lq_coarse, ncells, ndocs, 0);
    char* blk = nullptr;
    if (hipMalloc((void**)&blk, l.total) != hipSuccess) { (void)hipGetLastError(); return RR_ERR_OOM; }
    const rr_bank_view bank{nbits, n_centroids, nullptr, codes, residuals, centroids_f16, bucket_weights, mask_bytes};
    const rr_plaid_search_args a{n_queries, n_passages, first_passage, Lq, Lq_coarse, D, ncells, ndocs, k, threshold, query_li,
                                 (const rr_bank_slot*)table + first_passage, bank, blk, indices_out, scores_out, counts_out};
    int rc = RR_OK;
    for (int s = 0; s < l.stages && rc == RR_OK; ++s)
      if (rr_launch_plaid_search_stage(s, a, l, st) != hipSuccess) rc = RR_ERR_HIP;
    if (hipStreamSynchronize(st) != hipSuccess && rc == RR_OK) rc = RR_ERR_HIP;
    (void)hipFree(blk);
    return rc;
  });
}

// rr_bank_export_plaid (include/rerank_mi355.h): every refusal on the host; the count, the scan and the move over the bank's device
// passage table (csrc/bank_export.hip)
int rr_bank_export_plaid(rr_bank_handle b, int32_t first_passage, int32_t n_passages, int32_t* doclens_host_out, int32_t* codes_out, uint8_t* residuals_out,
                         int64_t capacity_rows, int64_t* rows_host_out, void* hip_stream) {
  return guarded(nullptr, [&]() -> int {
    const char* what = "rr_bank_export_plaid";
    if (!b) return RR_ERR_BAD_ARG;
    if (!doclens_host_out || !rows_host_out) return bfail(b, RR_ERR_BAD_ARG, "%s: null doclens_host_out or rows_host_out", what);
    if ((codes_out == nullptr) != (residuals_out == nullptr))
      return bfail(b, RR_ERR_BAD_ARG, "%s: codes_out and residuals_out are given together, or both NULL (a sizing call)", what);
    if (b->coded())
      return bfail(b, RR_ERR_UNSUPPORTED, "%s on an fp16 bank with a centroid table: it holds codes but no residuals (rr_bank_add_compress into a "
                   "compressed bank writes them)", what);
    if (!b->nbits) return bfail(b, RR_ERR_UNSUPPORTED, "%s on an fp16 bank: it holds no codes", what);
    const long long held = (long long)b->first.size();
    if (n_passages < 1 || first_passage < 0 || (long long)first_passage + n_passages > held)
      return bfail(b, RR_ERR_BAD_SHAPE, "%s: passages [%d, %d + %d) of a bank that holds %lld", what, first_passage, first_passage, n_passages, held);
    const int rb = (int)b->resid_row_bytes();
    if (codes_out && ((((uintptr_t)codes_out) & 3) || (((uintptr_t)residuals_out) & (uintptr_t)(std::min(rb, 16) - 1))))
      return bfail(b, RR_ERR_BAD_ARG, "%s: codes_out must be 4-byte aligned, residuals_out %d-byte", what, std::min(rb, 16));
    if (codes_out && capacity_rows < 0) return bfail(b, RR_ERR_BAD_SHAPE, "%s: capacity_rows=%lld", what, (long long)capacity_rows);
    hipStream_t st = (hipStream_t)hip_stream;
    RR_TRY(bank_capture_guard(b, st, "%s cannot be captured into a graph (it allocates and synchronises)", what));
    RR_BHIP(b, hipSetDevice(b->device));
    if (const int rc = bank_table_current(nullptr, b, st)) return bfail(b, rc, "%s: the bank's device passage table could not be brought up to date", what);
    int64_t R = 0;
    const hipError_t e = rr_export_plaid(b->table + first_passage, n_passages, b->mask, b->codes, b->resid, rb, doclens_host_out, nullptr, nullptr,
                                         codes_out, residuals_out, capacity_rows, &R, st);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return bfail(b, e == hipErrorOutOfMemory ? RR_ERR_OOM : RR_ERR_HIP, "%s: %d passages: %s", what, n_passages, hipGetErrorString(e));
    }
    if (codes_out && capacity_rows < R)
      return bfail(b, RR_ERR_BAD_SHAPE, "%s: the passages hold %lld unmasked rows, the buffers %lld (nothing was written)", what, (long long)R,
                   (long long)capacity_rows);
    *rows_host_out = R;
    return RR_OK;
  });
}

int rr_op_bank_export_plaid(const void* table, int32_t first_passage, int32_t n_passages, const uint8_t* mask_bytes, const int32_t* codes,
                            const uint8_t* residuals, int resid_row_bytes, int32_t* doclens_out, int64_t* offsets_out, int32_t* codes_out,
                            uint8_t* residuals_out, int64_t capacity_rows, void* hip_stream) {
  return guarded(nullptr, [&]() -> int {
    if (!table || !mask_bytes || !doclens_out || (codes_out == nullptr) != (residuals_out == nullptr)) return RR_ERR_BAD_ARG;
    if (codes_out && (!codes || !residuals)) return RR_ERR_BAD_ARG;
    if (!rr_export_row_bytes_ok(resid_row_bytes)) return RR_ERR_UNSUPPORTED;
    const uintptr_t ra = (uintptr_t)(std::min(resid_row_bytes, 16) - 1);
    if ((((uintptr_t)table) & 15) || ((((uintptr_t)doclens_out) | ((uintptr_t)codes) | ((uintptr_t)codes_out)) & 3) || (((uintptr_t)offsets_out) & 7) ||
        ((((uintptr_t)residuals) | ((uintptr_t)residuals_out)) & ra))
      return RR_ERR_BAD_ARG;
    if (first_passage < 0 || n_passages < 1 || (codes_out && capacity_rows < 0)) return RR_ERR_BAD_SHAPE;
    hipStream_t st = (hipStream_t)hip_stream;
    int64_t R = 0;
    const hipError_t e = rr_export_plaid((const rr_bank_slot*)table + first_passage, n_passages, mask_bytes, codes, residuals, resid_row_bytes, nullptr,
                                         doclens_out, offsets_out, codes_out, residuals_out, capacity_rows, &R, st);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return e == hipErrorOutOfMemory ? RR_ERR_OOM : RR_ERR_HIP;
    }
    return codes_out && capacity_rows < R ? RR_ERR_BAD_SHAPE : RR_OK;
  });
}

// rr_bank_load_ivf (include/rerank_mi355.h): the caller's file checked on the host (ivf_check.h), uploaded beside the one the bank holds,
// with `verify` compared with a fresh build, and put in its place only then
int rr_bank_load_ivf(rr_bank_handle b, const int64_t* offsets_host, const int32_t* pids_host, int verify, void* hip_stream) {
  return guarded(nullptr, [&]() -> int {
    const char* what = "rr_bank_load_ivf";
    if (!b) return RR_ERR_BAD_ARG;
    if (!offsets_host) return bfail(b, RR_ERR_BAD_ARG, "%s: null offsets", what);
    if (!b->has_codes()) return bfail(b, RR_ERR_UNSUPPORTED, "%s on an fp16 bank: it holds no codes", what);
    const long long held = (long long)b->first.size();
    if (held < 1) return bfail(b, RR_ERR_BAD_SHAPE, "%s: the bank holds no passage", what);
    const int C = b->n_centroids;
    if (offsets_host[0] == 0 && offsets_host[C] > 0 && !pids_host) return bfail(b, RR_ERR_BAD_ARG, "%s: null pids", what);
    int64_t longest = 0;
    int list = 0;
    char why[160];
    if (!rr_ivf_check_host(offsets_host, pids_host, C, held, &longest, &list, why, sizeof why))
      return bfail(b, RR_ERR_BAD_SHAPE, "%s: list %d: %s (the bank is unchanged)", what, list, why);
    hipStream_t st = (hipStream_t)hip_stream;
    RR_TRY(bank_capture_guard(b, st, "%s cannot be captured into a graph (it allocates and synchronises)", what));
    RR_BHIP(b, hipSetDevice(b->device));
    rr_ivf f{}, g{};
    hipError_t e = rr_ivf_load(offsets_host, pids_host, C, (int)held, (int32_t)longest, st, &f);
    bool same = true;
    if (e == hipSuccess && verify) {                  // the guard against a file of another index: a fresh build must give these bytes
      e = rr_ivf_build(bank_view(b), b->first.data(), b->len.data(), (int)held, st, &g);
      if (e == hipSuccess) {
        same = g.postings == f.postings && g.longest == f.longest;
        if (same) {
          std::vector<int64_t> off((size_t)C + 1);
          std::vector<int32_t> pid((size_t)std::max<int64_t>(g.postings, 1));
          e = rr_ivf_read(g, C, off.data(), pid.data(), st);
          if (e == hipSuccess)
            same = !memcmp(off.data(), offsets_host, off.size() * sizeof(int64_t)) &&
                   (g.postings == 0 || !memcmp(pid.data(), pids_host, (size_t)g.postings * sizeof(int32_t)));
        }
      }
      rr_ivf_free(&g);
    }
    if (e != hipSuccess) {
      (void)hipGetLastError();
      rr_ivf_free(&f);
      return bfail(b, e == hipErrorOutOfMemory ? RR_ERR_OOM : RR_ERR_HIP, "%s: %lld passages, %d centroids: %s (the bank is unchanged)", what, held, C,
                   hipGetErrorString(e));
    }
    if (!same) {
      rr_ivf_free(&f);
      return bfail(b, RR_ERR_BAD_SHAPE, "%s: the file is not the inverted file of the %lld passages this bank holds (a file of another index? "
                   "the bank is unchanged)", what, held);
    }
    rr_ivf_free(&b->ivf);                             // hipFree waits for a search that still reads the previous file
    b->ivf = f;
    return RR_OK;
  });
}

int rr_util_plaid_prune(const float* S, int32_t n_centroids, int Lq_coarse, const int32_t* codes, const uint8_t* mask, const int32_t* lengths,
                        int32_t n_passages, int ncells, float threshold, int ndocs, uint8_t* cells_out, float* a1_out, float* a2_out,
                        int32_t* list1_out, int32_t* n1_out, int32_t* list2_out, int32_t* n2_out) {
  return guarded(nullptr, [&]() -> int {
    if (!S || !codes || !lengths) return RR_ERR_BAD_ARG;
    if (n_centroids < 1 || Lq_coarse < 1 || n_passages < 1 || ncells < 1 || ncells > n_centroids || ndocs < 4) return RR_ERR_BAD_SHAPE;
    for (int p = 0; p < n_passages; ++p)
      if (lengths[p] < 1) return RR_ERR_BAD_SHAPE;
    return rr_plaid_prune_host(S, n_centroids, Lq_coarse, Lq_coarse, codes, mask, lengths, n_passages, ncells, threshold, ndocs, cells_out, a1_out,
                               a2_out, list1_out, n1_out, list2_out, n2_out) ? RR_OK : RR_ERR_BAD_SHAPE;
  });
}

// rr_bank_merge_topk (include/rerank_mi355.h, THE MERGED LIST): every refusal on the host, then one launch; nothing is allocated and
// the handle's search block is not touched
static int bank_merge_call(rr_handle h, const int32_t* indices_in, const float* scores_in, const int32_t* counts_in, int64_t part_stride,
                           int64_t count_stride, int n_parts, const int32_t* part_offsets_host, int n_queries, int k_in, int k,
                           int32_t* indices_out, float* scores_out, int32_t* counts_out, int32_t* parts_out, void* hip_stream) {
  const char* what = "rr_bank_merge_topk";
  if (!h) return RR_ERR_BAD_ARG;
  rr_model* m = h;
  if (m->cfg.model_kind == RR_MODEL_FULL_CONTEXT) return fail(m, RR_ERR_BAD_ARG, "%s on a full-context model", what);
  char msg[256];
  if (const int rc = rr_merge_check(indices_in, scores_in, counts_in, part_stride, count_stride, n_parts, part_offsets_host, n_queries, k_in, k,
                                    indices_out, scores_out, counts_out, parts_out, msg, sizeof msg))
    return fail(m, rc, "%s: %s", what, msg);
  hipStream_t st = (hipStream_t)hip_stream;
  RR_TRY(capture_guard(m, st, "%s cannot be captured into a graph (no bank search can, and it reads what they wrote)", what));
  RR_HIP(m, hipSetDevice(m->cfg.device));
  m->last_stream = st;
  // bytes: every entry's index and score, the counts, the rows that leave
  const double bytes = 8.0 * n_parts * (double)n_queries * k_in + 4.0 * n_parts * (double)n_queries + 12.0 * n_queries * (double)k;
  RR_RUN(m, st, RR_K_TAIL, 0.0, bytes,
         rr_launch_bank_merge(indices_in, scores_in, counts_in, part_stride, count_stride, n_parts, part_offsets_host, n_queries, k_in, k,
                              indices_out, scores_out, counts_out, parts_out, st));
  return RR_OK;
}

int rr_bank_merge_topk(rr_handle h, const int32_t* indices_in, const float* scores_in, const int32_t* counts_in, int64_t part_stride,
                       int64_t count_stride, int n_parts, const int32_t* part_offsets_host, int n_queries, int k_in, int k,
                       int32_t* indices_out, float* scores_out, int32_t* counts_out, int32_t* parts_out, void* hip_stream) {
  return guarded(h, [&]() -> int {
    return bank_merge_call(h, indices_in, scores_in, counts_in, part_stride, count_stride, n_parts, part_offsets_host, n_queries, k_in, k,
                           indices_out, scores_out, counts_out, parts_out, hip_stream);
  });
}

// rr_op_bank_merge_topk (include/rerank_mi355_diag.h): the same launch over raw device pointers, without a handle
int rr_op_bank_merge_topk(const int32_t* indices_in, const float* scores_in, const int32_t* counts_in, int64_t part_stride, int64_t count_stride,
                          int n_parts, const int32_t* part_offsets_host, int n_queries, int k_in, int k, int32_t* indices_out,
                          float* scores_out, int32_t* counts_out, int32_t* parts_out, void* hip_stream) {
  return guarded(nullptr, [&]() -> int {
    char msg[256];
    if (const int rc = rr_merge_check(indices_in, scores_in, counts_in, part_stride, count_stride, n_parts, part_offsets_host, n_queries, k_in,
                                      k, indices_out, scores_out, counts_out, parts_out, msg, sizeof msg))
      return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    RR_TRY(capture_guard(nullptr, st, "%s cannot be captured into a graph", "rr_op_bank_merge_topk"));
    const hipError_t e = rr_launch_bank_merge(indices_in, scores_in, counts_in, part_stride, count_stride, n_parts, part_offsets_host, n_queries,
                                              k_in, k, indices_out, scores_out, counts_out, parts_out, st);
    return e == hipSuccess ? RR_OK : RR_ERR_HIP;
  });
}

// rr_util_bank_merge_topk: THE MERGED LIST in pure host code over host arrays, behind the same refusals
int rr_util_bank_merge_topk(const int32_t* indices_in, const float* scores_in, const int32_t* counts_in, int64_t part_stride, int64_t count_stride,
                            int n_parts, const int32_t* part_offsets, int n_queries, int k_in, int k, int32_t* indices_out, float* scores_out,
                            int32_t* counts_out, int32_t* parts_out) {
  return guarded(nullptr, [&]() -> int {
    char msg[256];
    if (const int rc = rr_merge_check(indices_in, scores_in, counts_in, part_stride, count_stride, n_parts, part_offsets, n_queries, k_in, k,
                                      indices_out, scores_out, counts_out, parts_out, msg, sizeof msg))
      return rc;
    rr_bank_merge_host(indices_in, scores_in, counts_in, part_stride, count_stride, n_parts, part_offsets, n_queries, k_in, k, indices_out,
                       scores_out, counts_out, parts_out);
    return RR_OK;
  });
}

// The moves of a plan carried out over `arrays` (widest: the bytes of a row of the widest of them): one block for the move table
// and the staging of the longest window, the moves enqueued on st, st synchronised, the block freed.  *allocated: the block was
// there (a failure before it changed nothing); *bytes: its size.
static hipError_t bank_move_block(const std::vector<rr_bank_move>& moves, const rr_move_array* arrays, int na, size_t widest, hipStream_t st,
                                  bool* allocated, size_t* bytes) {
  int64_t longest = 0, rows = 0;                  // of a window: the moves of one lie side by side
  for (size_t i = 0; i < moves.size(); ++i) {
    rows = (i && moves[i].window == moves[i - 1].window ? rows : 0) + moves[i].rows;
    longest = std::max(longest, rows);
  }
  const size_t table_bytes = (moves.size() * sizeof(rr_bank_move) + 15) & ~(size_t)15;
  *bytes = table_bytes + (((size_t)longest * widest + 15) & ~(size_t)15);
  *allocated = false;
  char* blk = nullptr;
  hipError_t e = hipMalloc((void**)&blk, *bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return e;
  }
  *allocated = true;
  e = hipMemcpyAsync(blk, moves.data(), moves.size() * sizeof(rr_bank_move), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = rr_bank_move_run(moves.data(), moves.size(), (const rr_bank_move*)blk, arrays, na, blk + table_bytes, st);
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  (void)hipFree(blk);
  if (e != hipSuccess) (void)hipGetLastError();
  return e;
}

// rr_bank_remove (include/rerank_mi355.h, REMOVING PASSAGES): the plan on the host (rr_bank_remove_plan, bank_move.hip: every refusal
// comes out of it or stands in front of it), the staging block and the move table on the device, the moves over every per-row
// array window by window, one synchronisation; the host table only then.  Last, the inverted file over the surviving prefix,
// from the builder rr_bank_build_ivf uses.
int rr_bank_remove(rr_bank_handle b, const int32_t* indices_host, int n, int32_t* new_index_host_out, void* hip_stream) {
  return guarded(nullptr, [&]() -> int {
    const char* what = "rr_bank_remove";
    if (!b) return RR_ERR_BAD_ARG;
    if (n < 0) return bfail(b, RR_ERR_BAD_SHAPE, "%s: n=%d", what, n);
    if (n > 0 && !indices_host) return bfail(b, RR_ERR_BAD_ARG, "%s: null indices", what);
    hipStream_t st = (hipStream_t)hip_stream;
    RR_TRY(bank_capture_guard(b, st, "%s cannot be captured into a graph (it allocates its staging block and synchronises)", what));
    const int held = (int)b->first.size();
    const size_t rb = b->resid_row_bytes();
    const size_t widest = b->nbits ? std::max<size_t>(rb, sizeof(int32_t)) : (size_t)b->D * sizeof(uint16_t);
    const int64_t window_rows = (int64_t)(rr_bank_move_staging_bytes() / widest);      // at least 4: 4 KiB over 1024 bytes a row
    std::vector<int32_t> new_index;
    std::vector<rr_bank_move> moves;
    int32_t bad = -1;
    const int prc = rr_bank_remove_plan(b->len.data(), held, indices_host, n, window_rows, &new_index, &moves, &bad);
    if (prc == RR_REMOVE_PLAN_OUTSIDE) return bfail(b, RR_ERR_BAD_SHAPE, "%s: index %d lies outside the bank's %d passages", what, bad, held);
    if (prc == RR_REMOVE_PLAN_TWICE) return bfail(b, RR_ERR_BAD_SHAPE, "%s: index %d is given twice", what, bad);
    if (prc) return bfail(b, RR_ERR_BAD_SHAPE, "%s: n=%d of %d passages", what, n, held);
    if (n == 0) {
      if (new_index_host_out && held) memcpy(new_index_host_out, new_index.data(), (size_t)held * sizeof(int32_t));
      return RR_OK;
    }
    RR_BHIP(b, hipSetDevice(b->device));
    if (!moves.empty()) {
      rr_move_array arrays[3];
      int na = 0;
      if (b->nbits) {
        arrays[na++] = rr_move_array{b->resid, (int)rb};
        arrays[na++] = rr_move_array{b->codes, (int)sizeof(int32_t)};
      } else {
        arrays[na++] = rr_move_array{b->rows, (int)widest};
        if (b->coded()) arrays[na++] = rr_move_array{b->codes, (int)sizeof(int32_t)};      // the codes travel with their rows
      }
      arrays[na++] = rr_move_array{b->mask, 1};
      bool allocated = false;
      size_t bytes = 0;
      const hipError_t e = bank_move_block(moves, arrays, na, widest, st, &allocated, &bytes);
      if (e != hipSuccess && !allocated)
        return bfail(b, e == hipErrorOutOfMemory ? RR_ERR_OOM : RR_ERR_HIP, "%s: a staging block of %zu bytes: %s (the bank is unchanged)", what, bytes,
                     hipGetErrorString(e));
      if (e != hipSuccess)
        return bfail(b, RR_ERR_HIP, "%s: moving the rows failed: %s (the bank's rows are undefined: clear it)", what, hipGetErrorString(e));
    } else {
      RR_BHIP(b, hipStreamSynchronize(st));         // only trailing passages go: nothing moves
    }
    // the host table: the survivors back to back, in their order
    int first_gone = held;
    int64_t row = 0;
    size_t kept = 0;
    for (int p = 0; p < held; ++p) {
      if (new_index[(size_t)p] < 0) {
        first_gone = std::min(first_gone, p);
        continue;
      }
      b->first[kept] = row;
      b->len[kept] = b->len[(size_t)p];
      row += b->len[kept++];
    }
    b->first.resize(kept);
    b->len.resize(kept);
    b->used_rows = row;
    b->table_n = std::min(b->table_n, (size_t)first_gone);    // the search's device table is current up to the first moved passage
    if (new_index_host_out) memcpy(new_index_host_out, new_index.data(), (size_t)held * sizeof(int32_t));
    // the inverted file covered passages 0 .. P - 1: it now covers the survivors among them, a prefix of the bank
    const int P = b->ivf.passages;
    if (P > first_gone) {
      int P2 = 0;
      for (int p = 0; p < P; ++p) P2 += new_index[(size_t)p] >= 0;
      rr_ivf f{};
      const hipError_t e = P2 ? rr_ivf_build(bank_view(b), b->first.data(), b->len.data(), P2, st, &f) : hipSuccess;
      rr_ivf_free(&b->ivf);                           // hipFree waits for a search that still reads the previous file
      if (e != hipSuccess) {
        (void)hipGetLastError();
        return bfail(b, e == hipErrorOutOfMemory ? RR_ERR_OOM : RR_ERR_HIP, "%s: the %d passages are removed, but the inverted file over the "
                     "remaining %d of its passages could not be built: %s; the file is gone and must be built again (rr_bank_build_ivf)", what, n,
                     P2, hipGetErrorString(e));
      }
      b->ivf = f;
    }
    return RR_OK;
  });
}

// rr_op_bank_move_rows (include/rerank_mi355_diag.h): the plan and the moves of rr_bank_remove over one raw device array
int rr_op_bank_move_rows(void* array, int row_bytes, const int32_t* lengths_host, int32_t n, const int32_t* remove_host, int32_t m, void* hip_stream) {
  return guarded(nullptr, [&]() -> int {
    if (!array || (((uintptr_t)array) & 15) || (n > 0 && !lengths_host) || (m > 0 && !remove_host)) return RR_ERR_BAD_ARG;
    if (!rr_bank_move_row_bytes_ok(row_bytes)) return RR_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)hip_stream;
    RR_TRY(capture_guard(nullptr, st, "%s cannot be captured into a graph", "rr_op_bank_move_rows"));
    std::vector<int32_t> new_index;
    std::vector<rr_bank_move> moves;
    const int64_t window_rows = (int64_t)(rr_bank_move_staging_bytes() / (size_t)row_bytes);
    if (rr_bank_remove_plan(lengths_host, n, remove_host, m, window_rows, &new_index, &moves, nullptr)) return RR_ERR_BAD_SHAPE;
    if (moves.empty()) return RR_OK;
    const rr_move_array one{array, row_bytes};
    bool allocated = false;
    size_t bytes = 0;
    const hipError_t e = bank_move_block(moves, &one, 1, (size_t)row_bytes, st, &allocated, &bytes);
    return e == hipSuccess ? RR_OK : e == hipErrorOutOfMemory ? RR_ERR_OOM : RR_ERR_HIP;
  });
}

// rr_util_bank_remove_plan (include/rerank_mi355_diag.h): rr_bank_remove's plan over the caller's arrays
int rr_util_bank_remove_plan(const int32_t* lengths, int32_t n, const int32_t* remove, int32_t m, int64_t window_rows, int32_t* new_index_out,
                             int64_t* moves_out, int64_t moves_cap, int64_t* n_moves_out) {
  return guarded(nullptr, [&]() -> int {
    if ((n > 0 && !lengths) || (m > 0 && !remove) || (moves_out && moves_cap < 0)) return RR_ERR_BAD_ARG;
    std::vector<int32_t> new_index;
    std::vector<rr_bank_move> moves;
    if (rr_bank_remove_plan(lengths, n, remove, m, window_rows, &new_index, &moves, nullptr)) return RR_ERR_BAD_SHAPE;
    if (moves_out && (int64_t)moves.size() > moves_cap) return RR_ERR_BAD_SHAPE;
    static_assert(sizeof(rr_bank_move) == 4 * sizeof(int64_t), "a move is four int64");
    if (new_index_out && n) memcpy(new_index_out, new_index.data(), (size_t)n * sizeof(int32_t));
    if (moves_out && !moves.empty()) memcpy(moves_out, moves.data(), moves.size() * sizeof(rr_bank_move));
    if (n_moves_out) *n_moves_out = (int64_t)moves.size();
    return RR_OK;
  });
}

// ---- the entry points that share a body above (run through guarded(): no C++ exception crosses the ABI), and the small ones
int rr_bank_clear(rr_bank_handle b) {
  if (!b) return RR_ERR_BAD_ARG;
  b->first.clear();
  b->len.clear();
  b->used_rows = 0;
  b->table_n = 0;                 // the search's device table is rebuilt from the next passages
  if (b->ivf.passages) {          // the inverted file names passages that are gone (hipFree waits for what still reads it)
    (void)hipSetDevice(b->device);
    rr_ivf_free(&b->ivf);
  }
  return RR_OK;
}
const char* rr_bank_last_error(rr_bank_handle b) { return b ? b->err.c_str() : ""; }
int rr_bank_info(rr_bank_handle b, int32_t* passages_out, int64_t* rows_used_out, int64_t* capacity_rows_out) {
  if (!b) return RR_ERR_BAD_ARG;
  if (passages_out) *passages_out = (int32_t)b->first.size();
  if (rows_used_out) *rows_used_out = b->used_rows;
  if (capacity_rows_out) *capacity_rows_out = b->cap_rows;
  return RR_OK;
}
int rr_util_plaid_compress_rows(const void* rows, int dtype, int64_t n_rows, int D, const uint16_t* centroids_f16, int32_t n_centroids, const float* cutoffs, int nbits, int32_t* codes_out, uint8_t* residuals_out) {
  if (!rows || !centroids_f16 || !cutoffs || !codes_out || !residuals_out) return RR_ERR_BAD_ARG;
  if (dtype != RR_F32 && dtype != RR_F16) return RR_ERR_BAD_DTYPE;
  if (!rr_plaid_compress_shape_ok(nbits, D)) return RR_ERR_UNSUPPORTED;
  if (n_centroids <= 0 || n_centroids > (1 << 24) || n_rows < 0) return RR_ERR_BAD_SHAPE;
  return guarded(nullptr, [&]() -> int {
    return rr_plaid_compress_rows_host(rows, dtype == RR_F16, n_rows, D, centroids_f16, n_centroids, cutoffs, nbits, codes_out, residuals_out) ? RR_OK : RR_ERR_BAD_SHAPE;
  });
}
int rr_plaid_kmeans(rr_handle h, const void* rows, int dtype, int64_t n_rows, const int32_t* init_rows_host, int32_t n_centroids, int niters, uint64_t seed, uint16_t* centroids_f16_out, int32_t* counts_out, int32_t* stats_out, void* hip_stream) {
  return guarded(h, [&]() -> int { return h ? rr_plaid_kmeans_impl(h, "rr_plaid_kmeans", h->cfg.li_dim, rows, dtype, n_rows, init_rows_host, n_centroids, niters, seed, centroids_f16_out, counts_out, stats_out, hip_stream) : RR_ERR_BAD_ARG; });
}
int rr_op_plaid_kmeans(const void* rows, int dtype, int64_t n_rows, int D, const int32_t* init_rows_host, int32_t n_centroids, int niters, uint64_t seed, uint16_t* centroids_f16_out, int32_t* counts_out, int32_t* stats_out, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_plaid_kmeans_impl(nullptr, "rr_op_plaid_kmeans", D, rows, dtype, n_rows, init_rows_host, n_centroids, niters, seed, centroids_f16_out, counts_out, stats_out, hip_stream); });
}
int rr_op_plaid_residuals(const void* rows, int dtype, int64_t n_rows, int D, const uint16_t* centroids_f16, int32_t n_centroids, int32_t* codes_out, float* residuals_out, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_plaid_residuals_impl(nullptr, "rr_op_plaid_residuals", D, rows, dtype, n_rows, centroids_f16, n_centroids, codes_out, residuals_out, hip_stream); });
}
int rr_plaid_residuals(rr_handle h, const void* rows, int dtype, int64_t n_rows, const uint16_t* centroids_f16, int32_t n_centroids, int32_t* codes_out, float* residuals_out, void* hip_stream) {
  return guarded(h, [&]() -> int { return h ? rr_plaid_residuals_impl(h, "rr_plaid_residuals", h->cfg.li_dim, rows, dtype, n_rows, centroids_f16, n_centroids, codes_out, residuals_out, hip_stream) : RR_ERR_BAD_ARG; });
}
int rr_util_plaid_kmeans(const void* rows, int dtype, int64_t n_rows, int D, const int32_t* init_rows, int32_t n_centroids, int niters, uint64_t seed, uint16_t* centroids_f16_out, int32_t* counts_out, int32_t* stats_out) {
  return guarded(nullptr, [&]() -> int {
    if (!rows || !init_rows || !centroids_f16_out) return RR_ERR_BAD_ARG;
    if (dtype != RR_F32 && dtype != RR_F16) return RR_ERR_BAD_DTYPE;
    if (!rr_plaid_train_shape_ok(D) || n_rows > (1LL << 30)) return RR_ERR_UNSUPPORTED;
    if (n_rows < 1 || n_centroids < 1 || n_centroids > n_rows || niters < 0) return RR_ERR_BAD_SHAPE;
    std::vector<int32_t> sorted(init_rows, init_rows + n_centroids);
    std::sort(sorted.begin(), sorted.end());
    if (sorted.front() < 0 || sorted.back() >= n_rows) return RR_ERR_BAD_SHAPE;
    for (size_t i = 1; i < sorted.size(); ++i)
      if (sorted[i] == sorted[i - 1]) return RR_ERR_BAD_SHAPE;
    return rr_plaid_kmeans_host(rows, dtype == RR_F16, n_rows, D, init_rows, n_centroids, niters, (unsigned long long)seed, centroids_f16_out, counts_out, stats_out) ? RR_OK : RR_ERR_BAD_SHAPE;
  });
}
int rr_bank_format(rr_bank_handle b, int32_t* nbits_out, int32_t* n_centroids_out, int64_t* bytes_per_row_out) {
  if (!b) return RR_ERR_BAD_ARG;
  if (nbits_out) *nbits_out = b->nbits;
  if (n_centroids_out) *n_centroids_out = b->n_centroids;
  if (bytes_per_row_out) *bytes_per_row_out = b->nbits ? (int64_t)(4 + b->resid_row_bytes() + 1) : (int64_t)b->D * 2 + 1 + (b->coded() ? 4 : 0);
  return RR_OK;
}
int rr_util_plaid_decode_rows(const uint16_t* centroids_f16, int32_t n_centroids, const float* bucket_weights, int nbits, int D, const int32_t* codes, const uint8_t* residuals, int64_t n_rows, uint16_t* rows_out_f16) {
  if (!centroids_f16 || !bucket_weights || !codes || !residuals || !rows_out_f16) return RR_ERR_BAD_ARG;
  if (!rr_plaid_shape_ok(nbits, D)) return RR_ERR_UNSUPPORTED;
  if (n_centroids <= 0 || n_rows < 0) return RR_ERR_BAD_SHAPE;
  return guarded(nullptr, [&]() -> int {
    return rr_plaid_decode_rows_host(centroids_f16, n_centroids, bucket_weights, nbits, D, codes, residuals, n_rows, rows_out_f16) ? RR_OK : RR_ERR_BAD_SHAPE;
  });
}
int rr_bank_li_scores(rr_handle h, rr_bank_handle b, const float* query_li, int n_queries, int Lq, const int32_t* pair_passage, const int32_t* pair_query, int n_pairs, int padded_context_len, float* scores_out, float* maxsim_out, void* hip_stream) {
  return guarded(h, [&]() -> int { return bank_li_scores_call(h, b, query_li, n_queries, Lq, pair_passage, pair_query, n_pairs, padded_context_len, scores_out, maxsim_out, hip_stream); });
}
int rr_bank_search(rr_handle h, rr_bank_handle b, const float* query_li, int n_queries, int Lq, int32_t first_passage, int32_t n_passages, int k, int32_t* indices_out, float* scores_out, void* hip_stream) {
  return guarded(h, [&]() -> int { return bank_search_call(h, b, query_li, n_queries, Lq, first_passage, n_passages, k, nullptr, false, indices_out, scores_out, nullptr, hip_stream); });
}
int rr_bank_search_f16(rr_handle h, rr_bank_handle b, const float* query_li, int n_queries, int Lq, int32_t first_passage, int32_t n_passages, int ndocs, int k, float slack, int32_t* indices_out, float* scores_out, int32_t* certified_out, void* hip_stream) {
  return guarded(h, [&]() -> int { return bank_search_f16_call(h, false, b, query_li, n_queries, Lq, first_passage, n_passages, ndocs, k, slack, indices_out, scores_out, certified_out, hip_stream); });
}
int rr_bank_search_f16_plaid(rr_handle h, rr_bank_handle b, const float* query_li, int n_queries, int Lq, int32_t first_passage, int32_t n_passages, int ndocs, int k, float slack, int32_t* indices_out, float* scores_out, int32_t* certified_out, void* hip_stream) {
  return guarded(h, [&]() -> int { return bank_search_f16_call(h, true, b, query_li, n_queries, Lq, first_passage, n_passages, ndocs, k, slack, indices_out, scores_out, certified_out, hip_stream); });
}
int rr_bank_search_filtered(rr_handle h, rr_bank_handle b, const float* query_li, int n_queries, int Lq, int32_t first_passage, int32_t n_passages, int k, const uint32_t* filter_bits, int filter_rows, int64_t filter_ld, int32_t* indices_out, float* scores_out, int32_t* counts_out, void* hip_stream) {
  const FilterArg f{filter_bits, filter_rows, filter_ld};
  return guarded(h, [&]() -> int { return bank_search_call(h, b, query_li, n_queries, Lq, first_passage, n_passages, k, &f, false, indices_out, scores_out, counts_out, hip_stream); });
}
int rr_bank_search_filtered_sparse(rr_handle h, rr_bank_handle b, const float* query_li, int n_queries, int Lq, int32_t first_passage, int32_t n_passages, int k, const uint32_t* filter_bits, int filter_rows, int64_t filter_ld, int32_t* indices_out, float* scores_out, int32_t* counts_out, void* hip_stream) {
  const FilterArg f{filter_bits, filter_rows, filter_ld};
  return guarded(h, [&]() -> int { return bank_search_call(h, b, query_li, n_queries, Lq, first_passage, n_passages, k, &f, true, indices_out, scores_out, counts_out, hip_stream); });
}
int rr_bank_search_plaid_filtered(rr_handle h, rr_bank_handle b, const float* query_li, int n_queries, int Lq, int Lq_coarse, int32_t first_passage, int32_t n_passages, int ncells, float centroid_score_threshold, int ndocs, int k, const uint32_t* filter_bits, int filter_rows, int64_t filter_ld, int32_t* indices_out, float* scores_out, int32_t* counts_out, void* hip_stream) {
  const FilterArg f{filter_bits, filter_rows, filter_ld};
  return guarded(h, [&]() -> int { return bank_search_plaid_call(h, false, b, query_li, n_queries, Lq, Lq_coarse, first_passage, n_passages, ncells, centroid_score_threshold, ndocs, k, &f, indices_out, scores_out, counts_out, hip_stream); });
}
int rr_bank_search_plaid_ivf_filtered(rr_handle h, rr_bank_handle b, const float* query_li, int n_queries, int Lq, int Lq_coarse, int32_t first_passage, int32_t n_passages, int ncells, float centroid_score_threshold, int ndocs, int k, const uint32_t* filter_bits, int filter_rows, int64_t filter_ld, int32_t* indices_out, float* scores_out, int32_t* counts_out, void* hip_stream) {
  const FilterArg f{filter_bits, filter_rows, filter_ld};
  return guarded(h, [&]() -> int { return bank_search_plaid_call(h, true, b, query_li, n_queries, Lq, Lq_coarse, first_passage, n_passages, ncells, centroid_score_threshold, ndocs, k, &f, indices_out, scores_out, counts_out, hip_stream); });
}
int rr_bank_search_plaid(rr_handle h, rr_bank_handle b, const float* query_li, int n_queries, int Lq, int Lq_coarse, int32_t first_passage, int32_t n_passages, int ncells, float centroid_score_threshold, int ndocs, int k, int32_t* indices_out, float* scores_out, int32_t* counts_out, void* hip_stream) {
  return guarded(h, [&]() -> int { return bank_search_plaid_call(h, false, b, query_li, n_queries, Lq, Lq_coarse, first_passage, n_passages, ncells, centroid_score_threshold, ndocs, k, nullptr, indices_out, scores_out, counts_out, hip_stream); });
}
int rr_bank_search_plaid_ivf(rr_handle h, rr_bank_handle b, const float* query_li, int n_queries, int Lq, int Lq_coarse, int32_t first_passage, int32_t n_passages, int ncells, float centroid_score_threshold, int ndocs, int k, int32_t* indices_out, float* scores_out, int32_t* counts_out, void* hip_stream) {
  return guarded(h, [&]() -> int { return bank_search_plaid_call(h, true, b, query_li, n_queries, Lq, Lq_coarse, first_passage, n_passages, ncells, centroid_score_threshold, ndocs, k, nullptr, indices_out, scores_out, counts_out, hip_stream); });
}
int64_t rr_bank_search_plaid_tap(rr_handle h, const char* name, void* host_out, int64_t max_bytes) {
  return guarded<int64_t>(h, [&]() -> int64_t { return bank_search_plaid_tap(h, name, host_out, max_bytes); });
}
int rr_op_bank_li_scores(const float* query_li, int Lq, int D, const void* pairs, int n_pairs, int padded_context_len, const uint16_t* rows_f16, const uint8_t* mask_bytes, int nbits, const int32_t* codes, const uint8_t* residuals, const uint16_t* centroids_f16, const float* bucket_weights, int32_t n_centroids, float* scores_out, float* maxsim_out, void* hip_stream) {
  if (!query_li || !pairs || !mask_bytes || (!scores_out && !maxsim_out)) return RR_ERR_BAD_ARG;
  if (nbits ? (!codes || !residuals || !centroids_f16 || !bucket_weights) : !rows_f16) return RR_ERR_BAD_ARG;
  if (D <= 0 || D % 16 || (nbits && !rr_plaid_shape_ok(nbits, D))) return RR_ERR_UNSUPPORTED;
  if (Lq <= 0 || n_pairs <= 0 || padded_context_len <= 0 || (nbits && n_centroids <= 0)) return RR_ERR_BAD_SHAPE;
  const rr_bank_view bank{nbits, n_centroids, rows_f16, codes, residuals, centroids_f16, bucket_weights, mask_bytes};
  const hipError_t e = rr_launch_bank_li_scores((const rr_bank_pair*)pairs, nullptr, n_pairs, Lq, padded_context_len, D, query_li, bank, scores_out, maxsim_out, (hipStream_t)hip_stream);
  return e == hipSuccess ? RR_OK : RR_ERR_HIP;
}
