// librerank_mi355 — C ABI implementation (see include/rerank_mi355.h for the contract).
//
// Host-side orchestration of the rerank forward as a fixed kernel sequence on one HIP stream.
// The sequence restates /root/reference/src/models/rerank/rerank_model.py:523-591
// (FullContextRerankModel.forward) -> :333-479 (RerankModel.query) -> utils.py:85-108 (CrossEncoder)
// -> utils.py:228-254 (head); everything runs on the device, there is no CPU fallback.
#include "rr_api_internal.h"

// launchers implemented in the other translation units
hipError_t rr_launch_embed_ln(const int64_t*, const int64_t*, const float*, const float*, const float*, const float*,
                              const float*, float, int, int, int, int, int, float*, bf16_t*, int, hipStream_t);
hipError_t rr_launch_ce_embed_ln(const float*, const float*, const float*, const float*, const float*, float, int, int,
                                 int, float*, bf16_t*, int, hipStream_t, int s_text = -1, int vis_pos0 = 0, int cls32_only = 0);
hipError_t rr_launch_li_normalize(const float*, const int64_t*, int, int, int, int, int, int, int, int, int, bf16_t*,
                                  int, int, const float*, int, int, hipStream_t);
hipError_t rr_launch_joint_masks(const int64_t*, const int64_t*, int, int, int, int, long long, float*, float*, float*,
                                 hipStream_t);
hipError_t rr_launch_interaction_bias(const float*, const float*, int, int, int, int, int, float*, float*, float*,
                                      hipStream_t);
hipError_t rr_launch_split_residual_value(const bf16_t* hi, const bf16_t* lo, const float* stats, const float* gamma, const float* beta,
                                          int rows, int cols, int dt, float* out, hipStream_t st);
hipError_t rr_launch_layernorm_stats(const float*, const float*, const float*, float, int, int, float*, bf16_t*, float*,
                                     int, hipStream_t);
hipError_t rr_launch_key_bias(const int64_t*, const int64_t*, int, int, int, float*, float*, hipStream_t);
hipError_t rr_launch_f32_to_bf16(const float*, bf16_t*, size_t, int, hipStream_t);
hipError_t rr_launch_quant_e4m3(const void*, int, float, uint8_t*, size_t, hipStream_t);
hipError_t rr_launch_amax(const void*, int, size_t, float*, hipStream_t);
hipError_t rr_launch_gather_rows(const void*, void*, int, int, int, int, int, int, int, hipStream_t);
hipError_t rr_launch_cls_heads(const float*, int, int, int, const float*, const float*, const float*, const float*,
                               float*, float*, hipStream_t);
hipError_t rr_launch_head(const float*, const float*, const float*, int, int, int, float, int, float*, int32_t*,
                          float*, float*, float*, hipStream_t);
hipError_t rr_launch_head_lists(const float*, const float*, const float*, int, const int32_t*, const int32_t*, int, int, int,
                                float, int, float*, int32_t*, float*, float*, float*, float*, hipStream_t);
hipError_t rr_attention_reserve(int B, int heads, int Tq, hipStream_t st);

namespace {

uint16_t host_f2bf(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
uint16_t host_f2h(float f) {      // IEEE binary16, round-to-nearest-even
  uint32_t u;
  memcpy(&u, &f, 4);
  const uint32_t sign = (u >> 16) & 0x8000u;
  u &= 0x7fffffffu;
  if (u > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);              // NaN
  if (u >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);             // >= 65520 -> inf
  if (u < 0x33000001u) return (uint16_t)sign;                           // < 2^-25 -> 0
  if (u < 0x38800000u) {                                                // subnormal half
    const int e = (int)(u >> 23);
    uint32_t m = (u & 0x7fffffu) | 0x800000u;
    const int shift = 126 - e;                                          // 14 .. 24
    const uint32_t half = m >> shift, rem = m & ((1u << shift) - 1), mid = 1u << (shift - 1);
    return (uint16_t)(sign | (half + ((rem > mid) || (rem == mid && (half & 1)))));
  }
  uint32_t h = ((u - 0x38000000u) >> 13);
  const uint32_t rem = u & 0x1fffu;
  h += (rem > 0x1000u) || (rem == 0x1000u && (h & 1));
  return (uint16_t)(sign | h);
}

// OCP e4m3fn, round to nearest even, saturating at +-448 (what v_cvt_pk_fp8_f32 produces for |x| <= 448 on gfx950)
uint8_t host_f2e4m3(float f) {
  if (f != f) return 0x7f;
  const uint8_t sign = std::signbit(f) ? 0x80 : 0;
  float a = fabsf(f);
  if (a >= 448.0f) return sign | 0x7e;
  if (a < ldexpf(1.0f, -6)) {                                   // subnormal: multiples of 2^-9
    const int m = (int)nearbyintf(ldexpf(a, 9));                // 0 .. 8 (8 = the smallest normal)
    return sign | (uint8_t)m;
  }
  int e;
  const float fr = frexpf(a, &e);                               // a = fr * 2^e, fr in [0.5, 1)
  e -= 1;                                                       // a = (2 fr) * 2^e, 2 fr in [1, 2)
  int m = (int)nearbyintf((2.0f * fr - 1.0f) * 8.0f);           // 0 .. 8
  if (m == 8) { m = 0; e += 1; }
  if (e > 8 || (e == 8 && m > 6)) return sign | 0x7e;
  return sign | (uint8_t)(((e + 7) << 3) | m);
}
// rows of W [rows, cols] -> e4m3 with one scale per row (amax / 448; a zero row gets scale 1; a row that holds a NaN or an inf
// gets the scale NaN — the scale multiplies the whole output column in the GEMM epilogue — and codes without meaning)
void host_quantize_rows(const float* W, size_t rows, size_t cols, uint8_t* out, float* scales) {
  for (size_t r = 0; r < rows; ++r) {
    float amax = 0.f;
    bool finite = true;                                         // fmaxf drops a NaN and the clamp below turns one into -448
    for (size_t k = 0; k < cols; ++k) { amax = fmaxf(amax, fabsf(W[r * cols + k])); finite = finite && std::isfinite(W[r * cols + k]); }
    const float sc = amax > 0.f ? amax * (1.0f / 448.0f) : 1.0f, inv = 1.0f / sc;
    scales[r] = finite ? sc : std::numeric_limits<float>::quiet_NaN();   // a NaN / inf in the row: the whole output column is NaN
    for (size_t k = 0; k < cols; ++k) out[r * cols + k] = host_f2e4m3(fminf(fmaxf(W[r * cols + k] * inv, -448.0f), 448.0f));
  }
}

// rows of W [rows, cols] -> int8 codes with one scale per row (amax / 127; a zero row gets scale 1): round to nearest even,
// clamped to +-127 (the code range stays symmetric, -128 never occurs); a row that holds a NaN or an inf gets the scale NaN
void host_quantize_rows_i8(const float* W, size_t rows, size_t cols, int8_t* out, float* scales) {
  for (size_t r = 0; r < rows; ++r) {
    float amax = 0.f;
    bool finite = true;                                         // fmaxf drops a NaN and the clamp below turns one into -127
    for (size_t k = 0; k < cols; ++k) { amax = fmaxf(amax, fabsf(W[r * cols + k])); finite = finite && std::isfinite(W[r * cols + k]); }
    const float sc = amax > 0.f ? amax * (1.0f / 127.0f) : 1.0f, inv = 1.0f / sc;
    scales[r] = finite ? sc : std::numeric_limits<float>::quiet_NaN();   // a NaN / inf in the row: the whole output column is NaN
    for (size_t k = 0; k < cols; ++k) out[r * cols + k] = (int8_t)nearbyintf(fminf(fmaxf(W[r * cols + k] * inv, -127.0f), 127.0f));
  }
}
// Outlier smoothing of the int8 configuration ("gamma migration", Wei et al. 2022, Outlier Suppression): per channel j of a
// LayerNorm that feeds an int8 GEMM, s_j = 2^round(log2(m_j / median m)) clamped to [1, 2^10], m_j = max(|gamma_j|, |beta_j|)
// (median: element n/2 of the sorted m; ties of the rounding go up).  The quantising LayerNorm reads gamma / s, beta / s, the
// consumer weight columns are multiplied by s before their per-channel quantisation: a power of two, so both are exact in fp32
// and the product is unchanged before quantisation; the channels whose LayerNorm gain is an outlier stop setting the row's scale.
void host_smooth_scales(const float* gamma, const float* beta, size_t n, float* s) {
  std::vector<float> mv(n);
  for (size_t j = 0; j < n; ++j) mv[j] = fmaxf(fabsf(gamma[j]), fabsf(beta[j]));
  std::vector<float> sorted(mv);
  std::nth_element(sorted.begin(), sorted.begin() + n / 2, sorted.end());
  const double med = n ? (double)sorted[n / 2] : 0.0;
  for (size_t j = 0; j < n; ++j) {
    int e = 0;
    if (med > 0.0 && mv[j] > 0.f) e = (int)std::floor(std::log2((double)mv[j] / med) + 0.5);
    s[j] = ldexpf(1.0f, e < 0 ? 0 : e > 10 ? 10 : e);
  }
}

}  // namespace

// largest value of an option (the smallest is always -1 = "not set")
static int option_max(int which) { return which == RR_OPT_ATTN_FIXED_REF ? 3 : which == RR_OPT_FP8_FIRST_LAYER ? 4096 : 1; }

namespace {

// ---- required-weight table -------------------------------------------------------------------
void req(rr_model* m, const std::string& name, std::vector<int64_t> shape) {
  m->required[name] = std::move(shape);
  m->required_order.push_back(name);
}
void req_layer(rr_model* m, const std::string& p, int H, int I, bool cross) {
  const char* atts[2] = {"attention", "crossattention"};
  for (int a = 0; a < (cross ? 2 : 1); ++a) {
    const std::string ap = p + "." + atts[a];
    for (const char* n : {"query", "key", "value"}) {
      req(m, ap + ".self." + n + ".weight", {H, H});
      req(m, ap + ".self." + n + ".bias", {H});
    }
    req(m, ap + ".output.dense.weight", {H, H});
    req(m, ap + ".output.dense.bias", {H});
    req(m, ap + ".output.LayerNorm.weight", {H});
    req(m, ap + ".output.LayerNorm.bias", {H});
  }
  req(m, p + ".intermediate.dense.weight", {I, H});
  req(m, p + ".intermediate.dense.bias", {I});
  req(m, p + ".output.dense.weight", {H, I});
  req(m, p + ".output.dense.bias", {H});
  req(m, p + ".output.LayerNorm.weight", {H});
  req(m, p + ".output.LayerNorm.bias", {H});
}
void build_required(rr_model* m) {
  const rr_config& c = m->cfg;
  const int H = c.hidden, I = c.intermediate, D = c.li_dim;
  if (c.model_kind != RR_MODEL_FULL_CONTEXT) {
    // InteractionRerankModel (interaction_rerank_model.py:96-109): only the input mapping + the reranker
    const int Hc = c.ce_hidden, Ic = c.ce_intermediate;
    req(m, "cross_encoder_input_mapping.weight", {Hc, D});
    req(m, "cross_encoder_input_mapping.bias", {Hc});
    if (c.model_kind == RR_MODEL_INTERACTION) {
      const std::string p = "reranker.bert_model";
      req(m, p + ".embeddings.position_embeddings.weight", {c.ce_max_pos, Hc});
      req(m, p + ".embeddings.token_type_embeddings.weight", {c.type_vocab, Hc});
      req(m, p + ".embeddings.LayerNorm.weight", {Hc});
      req(m, p + ".embeddings.LayerNorm.bias", {Hc});
      for (int i = 0; i < c.ce_layers; ++i) req_layer(m, p + ".encoder.layer." + std::to_string(i), Hc, Ic, false);
    } else {   // MORES (mores_model.py:60-69)
      for (int i = 0; i < c.ce_layers; ++i)
        req_layer(m, "reranker.interaction_module." + std::to_string(i), Hc, Ic, true);
    }
    req(m, "reranker.classifier1.weight", {1, Hc});
    req(m, "reranker.classifier1.bias", {1});
    req(m, "reranker.classifier2.weight", {1, Hc});
    req(m, "reranker.classifier2.bias", {1});
    return;
  }
  std::string p = "context_text_encoder.bert_model";
  req(m, p + ".embeddings.word_embeddings.weight", {c.vocab_size, H});
  req(m, p + ".embeddings.position_embeddings.weight", {c.max_pos, H});
  req(m, p + ".embeddings.token_type_embeddings.weight", {c.type_vocab, H});
  req(m, p + ".embeddings.LayerNorm.weight", {H});
  req(m, p + ".embeddings.LayerNorm.bias", {H});
  for (int i = 0; i < c.layers; ++i) req_layer(m, p + ".encoder.layer." + std::to_string(i), H, I, false);
  req(m, "context_text_encoder_linear.weight", {D, H});
  if (c.has_vision) {
    const int Vh = c.vision_hidden, mid = D * c.prefix_len / 2, outd = D * c.prefix_len;
    req(m, "context_vision_projection.model.0.weight", {mid, Vh});
    req(m, "context_vision_projection.model.0.bias", {mid});
    req(m, "context_vision_projection.model.2.weight", {outd, mid});
    req(m, "context_vision_projection.model.2.bias", {outd});
    req(m, "transformer_mapping_input_linear.weight", {H, Vh});
    req(m, "transformer_mapping_input_linear.bias", {H});
    for (int i = 0; i < c.map_layers; ++i)
      req_layer(m, "transformer_mapping_network.layer." + std::to_string(i), H, I, true);
    req(m, "transformer_mapping_output_linear.weight", {D, H});
    req(m, "transformer_mapping_output_linear.bias", {D});
  }
  if (c.vit_layers > 0) {   // FLMRVisionModel.vision_model (CLIPVisionModel) .vision_model (CLIPVisionTransformer)
    const int Vh = c.vision_hidden, Iv = c.vit_intermediate, ps = c.vit_patch_size;
    const std::string v = "context_vision_encoder.vision_model.vision_model";
    req(m, v + ".embeddings.class_embedding", {Vh});
    req(m, v + ".embeddings.patch_embedding.weight", {Vh, 3, ps, ps});
    req(m, v + ".embeddings.position_embedding.weight", {c.n_patches + 1, Vh});
    req(m, v + ".pre_layrnorm.weight", {Vh});
    req(m, v + ".pre_layrnorm.bias", {Vh});
    for (int i = 0; i < c.vit_layers; ++i) {
      const std::string l = v + ".encoder.layers." + std::to_string(i);
      for (const char* n : {"q_proj", "k_proj", "v_proj", "out_proj"}) {
        req(m, l + ".self_attn." + n + ".weight", {Vh, Vh});
        req(m, l + ".self_attn." + n + ".bias", {Vh});
      }
      req(m, l + ".layer_norm1.weight", {Vh});
      req(m, l + ".layer_norm1.bias", {Vh});
      req(m, l + ".mlp.fc1.weight", {Iv, Vh});
      req(m, l + ".mlp.fc1.bias", {Iv});
      req(m, l + ".mlp.fc2.weight", {Vh, Iv});
      req(m, l + ".mlp.fc2.bias", {Vh});
      req(m, l + ".layer_norm2.weight", {Vh});
      req(m, l + ".layer_norm2.bias", {Vh});
    }
  }
  const int Hc = c.ce_hidden, Ic = c.ce_intermediate;
  req(m, "cross_encoder_input_mapping.weight", {Hc, D});
  req(m, "cross_encoder_input_mapping.bias", {Hc});
  p = "reranker.bert_model";
  req(m, p + ".embeddings.position_embeddings.weight", {c.ce_max_pos, Hc});
  req(m, p + ".embeddings.token_type_embeddings.weight", {c.type_vocab, Hc});
  req(m, p + ".embeddings.LayerNorm.weight", {Hc});
  req(m, p + ".embeddings.LayerNorm.bias", {Hc});
  for (int i = 0; i < c.ce_layers; ++i) req_layer(m, p + ".encoder.layer." + std::to_string(i), Hc, Ic, false);
  req(m, "reranker.classifier1.weight", {1, Hc});
  req(m, "reranker.classifier1.bias", {1});
  req(m, "reranker.classifier2.weight", {1, Hc});
  req(m, "reranker.classifier2.bias", {1});
}

// ---- device upload helpers -------------------------------------------------------------------
int dev_alloc(rr_model* m, void** out, size_t bytes) {
  RR_HIP(m, hipMalloc(out, bytes ? bytes : 16));
  m->dev_allocs.push_back(*out);
  return RR_OK;
}
int up_f32(rr_model* m, const std::vector<float>& v, float** out) {
  int rc = dev_alloc(m, (void**)out, v.size() * 4);
  if (rc) return rc;
  RR_HIP(m, hipMemcpy(*out, v.data(), v.size() * 4, hipMemcpyHostToDevice));
  return RR_OK;
}
int up_bf16(rr_model* m, const std::vector<float>& v, bf16_t** out) {   // 16-bit MFMA operand in the model's compute dtype
  std::vector<uint16_t> t(v.size());
  if (m->dt) for (size_t i = 0; i < v.size(); ++i) t[i] = host_f2h(v[i]);
  else for (size_t i = 0; i < v.size(); ++i) t[i] = host_f2bf(v[i]);
  int rc = dev_alloc(m, (void**)out, t.size() * 2);
  if (rc) return rc;
  RR_HIP(m, hipMemcpy(*out, t.data(), t.size() * 2, hipMemcpyHostToDevice));
  return RR_OK;
}
const std::vector<float>& HT(rr_model* m, const std::string& n) { return m->host.at(n).data; }

std::vector<float> cat(std::initializer_list<const std::vector<float>*> parts, float first_scale) {
  std::vector<float> o;
  bool first = true;
  for (auto* p : parts) {
    const size_t n0 = o.size();
    o.insert(o.end(), p->begin(), p->end());
    if (first && first_scale != 1.0f)
      for (size_t i = n0; i < o.size(); ++i) o[i] *= first_scale;
    first = false;
  }
  return o;
}

// Folded form of a Linear [N, K] (+ bias [N]) behind LayerNorm(gamma, beta) [K]: see LayerW.
int up_folded(rr_model* m, const std::vector<float>& W, const std::vector<float>& b, const std::vector<float>& gamma,
              const std::vector<float>& beta, bf16_t** w_out, float** c_out, float** d_out) {
  const size_t K = gamma.size(), N = W.size() / K;
  std::vector<uint16_t> w16(W.size());
  std::vector<float> c(N), d(N);
  for (size_t n = 0; n < N; ++n) {
    double cs = 0.0, ds = 0.0;
    for (size_t k = 0; k < K; ++k) {
      const float wg = W[n * K + k] * gamma[k];
      const uint16_t r = m->dt ? host_f2h(wg) : host_f2bf(wg);
      w16[n * K + k] = r;
      cs += (double)(m->dt ? host_h2f(r) : host_bf2f(r));          // the sum the MFMA forms for a constant row, exactly
      ds += (double)W[n * K + k] * (double)beta[k];
    }
    c[n] = (float)cs;
    d[n] = (float)(ds + (b.empty() ? 0.0 : (double)b[n]));
  }
  int rc = dev_alloc(m, (void**)w_out, w16.size() * 2);
  if (rc) return rc;
  RR_HIP(m, hipMemcpy(*w_out, w16.data(), w16.size() * 2, hipMemcpyHostToDevice));
  RR_TRY(up_f32(m, c, c_out));
  return up_f32(m, d, d_out);
}

int up_fp8(rr_model* m, const std::vector<float>& W, size_t cols, uint8_t** w_out, float** s_out) {
  const size_t rows = W.size() / cols;
  std::vector<uint8_t> q(W.size());
  std::vector<float> sc(rows);
  host_quantize_rows(W.data(), rows, cols, q.data(), sc.data());
  int rc = dev_alloc(m, (void**)w_out, q.size());
  if (rc) return rc;
  RR_HIP(m, hipMemcpy(*w_out, q.data(), q.size(), hipMemcpyHostToDevice));
  return up_f32(m, sc, s_out);
}

extern int g_q8_smooth;
// int8 ("q8_format" 1): the smoothing powers of two of a LayerNorm (all 1 with the diagnostic switch "q8_smooth" 0)
std::vector<float> q8_smoothing(const std::vector<float>& gamma, const std::vector<float>& beta) {
  std::vector<float> s(gamma.size(), 1.0f);
  if (g_q8_smooth) host_smooth_scales(gamma.data(), beta.data(), gamma.size(), s.data());
  return s;
}
std::vector<float> div_by(const std::vector<float>& v, const std::vector<float>& s) {
  std::vector<float> o(v.size());
  for (size_t j = 0; j < v.size(); ++j) o[j] = v[j] / s[j];
  return o;
}
// W [N, cols] with its columns multiplied by the smoothing s [cols] -> int8 codes, one scale per output channel
int up_i8(rr_model* m, const std::vector<float>& W, const std::vector<float>& s, uint8_t** w_out, float** s_out) {
  const size_t cols = s.size(), rows = W.size() / cols;
  std::vector<float> Ws(W.size());
  for (size_t r = 0; r < rows; ++r)
    for (size_t k = 0; k < cols; ++k) Ws[r * cols + k] = W[r * cols + k] * s[k];
  std::vector<int8_t> q(W.size());
  std::vector<float> sc(rows);
  host_quantize_rows_i8(Ws.data(), rows, cols, q.data(), sc.data());
  int rc = dev_alloc(m, (void**)w_out, q.size());
  if (rc) return rc;
  RR_HIP(m, hipMemcpy(*w_out, q.data(), q.size(), hipMemcpyHostToDevice));
  return up_f32(m, sc, s_out);
}

// prev_ln: state_dict prefix of the LayerNorm whose output feeds this layer's QKV ("" = none: first layer of a stack)
int pack_layer(rr_model* m, const std::string& p, int heads, int Hd, bool cross, LayerW* L, const std::string& prev_ln = "") {
  const float qs = 1.4426950408889634f / sqrtf((float)(Hd / heads));   // log2(e)/sqrt(dh): the attention kernels take base-2 exponentials of Q K^T as it is
  const std::string a = p + ".attention";
  RR_TRY(up_bf16(m, cat({&HT(m, a + ".self.query.weight"), &HT(m, a + ".self.key.weight"), &HT(m, a + ".self.value.weight")}, qs), &L->wqkv));
  RR_TRY(up_f32(m, cat({&HT(m, a + ".self.query.bias"), &HT(m, a + ".self.key.bias"), &HT(m, a + ".self.value.bias")}, qs), &L->bqkv));
  RR_TRY(up_bf16(m, HT(m, a + ".output.dense.weight"), &L->wo));
  RR_TRY(up_f32(m, HT(m, a + ".output.dense.bias"), &L->bo));
  RR_TRY(up_f32(m, HT(m, a + ".output.LayerNorm.weight"), &L->ln1g));
  RR_TRY(up_f32(m, HT(m, a + ".output.LayerNorm.bias"), &L->ln1b));
  if (cross) {
    const std::string c = p + ".crossattention";
    RR_TRY(up_bf16(m, cat({&HT(m, c + ".self.query.weight")}, qs), &L->wq_c));
    RR_TRY(up_f32(m, cat({&HT(m, c + ".self.query.bias")}, qs), &L->bq_c));
    RR_TRY(up_bf16(m, cat({&HT(m, c + ".self.key.weight"), &HT(m, c + ".self.value.weight")}, 1.0f), &L->wkv_c));
    RR_TRY(up_f32(m, cat({&HT(m, c + ".self.key.bias"), &HT(m, c + ".self.value.bias")}, 1.0f), &L->bkv_c));
    RR_TRY(up_bf16(m, HT(m, c + ".output.dense.weight"), &L->wo_c));
    RR_TRY(up_f32(m, HT(m, c + ".output.dense.bias"), &L->bo_c));
    RR_TRY(up_f32(m, HT(m, c + ".output.LayerNorm.weight"), &L->lncg));
    RR_TRY(up_f32(m, HT(m, c + ".output.LayerNorm.bias"), &L->lncb));
  }
  RR_TRY(up_bf16(m, HT(m, p + ".intermediate.dense.weight"), &L->w1));
  RR_TRY(up_f32(m, HT(m, p + ".intermediate.dense.bias"), &L->b1));
  if (!cross && m->cfg.fp8 && m->q8_fmt == 1) {
    // int8: FFN-up behind this layer's attention-output LayerNorm; QKV behind the previous layer's output LayerNorm (none in
    // front of the first layer of a stack, whose QKV never takes int8 operands: packed unsmoothed); this layer's output
    // LayerNorm gets its private affine for the next layer's QKV
    const std::vector<float>&g1 = HT(m, a + ".output.LayerNorm.weight"), &b1 = HT(m, a + ".output.LayerNorm.bias");
    const std::vector<float>&g2 = HT(m, p + ".output.LayerNorm.weight"), &b2 = HT(m, p + ".output.LayerNorm.bias");
    const std::vector<float> s1 = q8_smoothing(g1, b1), s2 = q8_smoothing(g2, b2);
    const std::vector<float> sp = prev_ln.empty() ? std::vector<float>((size_t)Hd, 1.0f)
                                                  : q8_smoothing(HT(m, prev_ln + ".weight"), HT(m, prev_ln + ".bias"));
    RR_TRY(up_i8(m, cat({&HT(m, a + ".self.query.weight"), &HT(m, a + ".self.key.weight"), &HT(m, a + ".self.value.weight")}, qs),
                 sp, &L->wqkv8, &L->sqkv));
    RR_TRY(up_i8(m, HT(m, p + ".intermediate.dense.weight"), s1, &L->w1_8, &L->s1));
    RR_TRY(up_f32(m, div_by(g1, s1), &L->ln1g_q));
    RR_TRY(up_f32(m, div_by(b1, s1), &L->ln1b_q));
    RR_TRY(up_f32(m, div_by(g2, s2), &L->ln2g_q));
    RR_TRY(up_f32(m, div_by(b2, s2), &L->ln2b_q));
  } else if (!cross && m->cfg.fp8) {
    RR_TRY(up_fp8(m, cat({&HT(m, a + ".self.query.weight"), &HT(m, a + ".self.key.weight"), &HT(m, a + ".self.value.weight")}, qs),
                  (size_t)Hd, &L->wqkv8, &L->sqkv));
    RR_TRY(up_fp8(m, HT(m, p + ".intermediate.dense.weight"), (size_t)Hd, &L->w1_8, &L->s1));
    RR_TRY(up_fp8(m, HT(m, p + ".output.dense.weight"), (size_t)m->cfg.intermediate, &L->w2_8, &L->s2));
  }
  if (!cross) {   // plain encoder layers: folded forms for the LayerNorm -> QKV and LayerNorm -> FFN-up seams
    RR_TRY(up_folded(m, HT(m, p + ".intermediate.dense.weight"), HT(m, p + ".intermediate.dense.bias"),
                     HT(m, a + ".output.LayerNorm.weight"), HT(m, a + ".output.LayerNorm.bias"), &L->w1_f, &L->c1_f, &L->d1_f));
    if (!prev_ln.empty())
      RR_TRY(up_folded(m, cat({&HT(m, a + ".self.query.weight"), &HT(m, a + ".self.key.weight"), &HT(m, a + ".self.value.weight")}, qs),
                       cat({&HT(m, a + ".self.query.bias"), &HT(m, a + ".self.key.bias"), &HT(m, a + ".self.value.bias")}, qs),
                       HT(m, prev_ln + ".weight"), HT(m, prev_ln + ".bias"), &L->wqkv_f, &L->cqkv_f, &L->dqkv_f));
  }
  RR_TRY(up_bf16(m, HT(m, p + ".output.dense.weight"), &L->w2));
  RR_TRY(up_f32(m, HT(m, p + ".output.dense.bias"), &L->b2));
  RR_TRY(up_f32(m, HT(m, p + ".output.LayerNorm.weight"), &L->ln2g));
  RR_TRY(up_f32(m, HT(m, p + ".output.LayerNorm.bias"), &L->ln2b));
  return RR_OK;
}

// CLIPEncoderLayer: q/k/v fused with CLIP's q scaling (dh^-0.5 applied to q_proj's output, bias included) folded in
int pack_vit_layer(rr_model* m, const std::string& l, int heads, int Vh, LayerW* L) {
  const float qs = 1.4426950408889634f / sqrtf((float)(Vh / heads));   // log2(e)/sqrt(dh), as pack_layer
  const std::string a = l + ".self_attn";
  RR_TRY(up_bf16(m, cat({&HT(m, a + ".q_proj.weight"), &HT(m, a + ".k_proj.weight"), &HT(m, a + ".v_proj.weight")}, qs), &L->wqkv));
  RR_TRY(up_f32(m, cat({&HT(m, a + ".q_proj.bias"), &HT(m, a + ".k_proj.bias"), &HT(m, a + ".v_proj.bias")}, qs), &L->bqkv));
  RR_TRY(up_bf16(m, HT(m, a + ".out_proj.weight"), &L->wo));
  RR_TRY(up_f32(m, HT(m, a + ".out_proj.bias"), &L->bo));
  RR_TRY(up_f32(m, HT(m, l + ".layer_norm1.weight"), &L->ln1g));
  RR_TRY(up_f32(m, HT(m, l + ".layer_norm1.bias"), &L->ln1b));
  RR_TRY(up_bf16(m, HT(m, l + ".mlp.fc1.weight"), &L->w1));
  RR_TRY(up_f32(m, HT(m, l + ".mlp.fc1.bias"), &L->b1));
  RR_TRY(up_bf16(m, HT(m, l + ".mlp.fc2.weight"), &L->w2));
  RR_TRY(up_f32(m, HT(m, l + ".mlp.fc2.bias"), &L->b2));
  RR_TRY(up_f32(m, HT(m, l + ".layer_norm2.weight"), &L->ln2g));
  RR_TRY(up_f32(m, HT(m, l + ".layer_norm2.bias"), &L->ln2b));
  return RR_OK;
}

int pack_vit(rr_model* m) {
  const rr_config& c = m->cfg;
  const int Vh = c.vision_hidden, Kd = 3 * c.vit_patch_size * c.vit_patch_size, Kp = (Kd + 63) / 64 * 64;
  const std::string v = "context_vision_encoder.vision_model.vision_model";
  m->vit_kp = Kp;
  const std::vector<float>& wp = HT(m, v + ".embeddings.patch_embedding.weight");   // [Vh, 3*ps*ps] row-major
  std::vector<float> padded((size_t)Vh * Kp, 0.f);
  for (int r = 0; r < Vh; ++r) memcpy(&padded[(size_t)r * Kp], &wp[(size_t)r * Kd], (size_t)Kd * 4);
  RR_TRY(up_bf16(m, padded, &m->vit_wpatch));
  RR_TRY(up_f32(m, HT(m, v + ".embeddings.class_embedding"), &m->vit_cls));
  RR_TRY(up_f32(m, HT(m, v + ".embeddings.position_embedding.weight"), &m->vit_pos));
  RR_TRY(up_f32(m, HT(m, v + ".pre_layrnorm.weight"), &m->vit_pre_g));
  RR_TRY(up_f32(m, HT(m, v + ".pre_layrnorm.bias"), &m->vit_pre_b));
  m->vit_layers.resize(c.vit_layers);
  for (int i = 0; i < c.vit_layers; ++i)
    RR_TRY(pack_vit_layer(m, v + ".encoder.layers." + std::to_string(i), c.vit_heads, Vh, &m->vit_layers[i]));
  return RR_OK;
}

// ---- workspace -------------------------------------------------------------------------------
struct Bump {
  char* base;
  size_t off = 0;
  explicit Bump(char* b) : base(b) {}
  template <class T>
  T* take(size_t n) {
    off = (off + 255) & ~(size_t)255;
    T* p = base ? (T*)(base + off) : nullptr;
    off += n * sizeof(T);
    return p;
  }
};

struct Work {
  float *h32, *pre, *pre2, *stats_a, *stats_b, *li32, *text_bias, *ce_bias, *l1, *l2, *part_l, *part_w, *li_mask, *lnpart, *rowscale;
  bf16_t *h16, *qkv, *ctx, *mid, *li16;
  char* cls_scratch;                   // the CLS-only cross-encoder layer's n-row buffers (run_cross_encoder)
  // vision
  bf16_t *cls16, *vp_mid16, *pat16, *t16, *vqkv, *vctx, *a16, *q_c, *enc16, *kv_c, *cctx, *c16, *vmid, *m16;
  float *vp_out32, *t32, *vpre, *a32, *a32b, *cpre, *c32, *m32, *mo32;
};

// Workspace of the CLIP ViT over B images
struct VitWork {
  bf16_t *cols, *n16, *qkv, *ctx, *mid;
  float *patch32, *xa, *xb;
};
size_t layout_vit(const rr_config& c, int kp, int B, char* base, VitWork* w) {
  Bump b(base);
  const size_t np = c.n_patches, R = (size_t)B * (np + 1), Vh = c.vision_hidden;
  w->cols = b.take<bf16_t>((size_t)B * np * kp);
  w->patch32 = b.take<float>((size_t)B * np * Vh);
  w->xa = b.take<float>(R * Vh);
  w->xb = b.take<float>(R * Vh);
  w->n16 = b.take<bf16_t>(R * Vh);
  w->qkv = b.take<bf16_t>(R * 3 * Vh);
  w->ctx = b.take<bf16_t>(R * Vh);
  w->mid = b.take<bf16_t>(R * c.vit_intermediate);
  return (b.off + 255) & ~(size_t)255;
}

size_t imax(size_t a, size_t b) { return a > b ? a : b; }

// n-row buffers of the CLS-only cross-encoder layer (run_cross_encoder): 11 regions, 30 Hc + 2 Ic bytes per pair plus the
// 256-byte alignment of each.  A region of its own (carved out of w.mid they overran it for rows shorter than ~6).
size_t cls_scratch_bytes(const rr_config& c, int n) {
  return (size_t)n * (30 * (size_t)c.ce_hidden + 2 * (size_t)c.ce_intermediate) + 11 * 256;
}
// Lays out the workspace for n local pairs of (at most) Bq queries; base == nullptr => size query.
size_t layout(const rr_config& c, int n, int Bq, int S, bool vision, char* base, Work* w) {
  Bump b(base);
  const int P = vision ? c.prefix_len + c.n_patches : 0, T = S + P;
  const size_t R = (size_t)n * S, RT = (size_t)n * T, Rm = imax(R, RT);
  const size_t Hm = imax(c.hidden, c.ce_hidden), Im = imax(c.intermediate, c.ce_intermediate);
  w->h32 = b.take<float>(Rm * Hm);
  w->pre = b.take<float>(Rm * Hm);
  w->pre2 = b.take<float>(Rm * Hm);
  w->stats_a = b.take<float>(Rm * 2);
  w->stats_b = b.take<float>(Rm * 2);
  w->lnpart = b.take<float>(Rm * 2 * ((Hm + 127) / 128));
  w->rowscale = b.take<float>(Rm);
  w->h16 = b.take<bf16_t>(Rm * Hm);
  w->qkv = b.take<bf16_t>(Rm * 3 * Hm);
  w->ctx = b.take<bf16_t>(Rm * Hm);
  w->mid = b.take<bf16_t>(Rm * Im);
  w->li32 = b.take<float>(R * c.li_dim);
  w->li16 = b.take<bf16_t>(RT * c.li_dim);
  w->text_bias = b.take<float>(R);
  w->ce_bias = b.take<float>(RT);
  w->li_mask = b.take<float>(R);
  w->l1 = b.take<float>(n);
  w->l2 = b.take<float>(n);
  w->part_l = b.take<float>(Bq);
  w->part_w = b.take<float>(Bq);
  w->cls_scratch = b.take<char>(cls_scratch_bytes(c, n));
  if (vision) {
    const size_t Hh = c.hidden, np = c.n_patches, Vh = c.vision_hidden, D = c.li_dim, PL = c.prefix_len;
    const size_t ca = (size_t)(S < c.cross_attn_len ? S : c.cross_attn_len);
    const size_t nb = c.map_layers > 1 ? imax((size_t)n, (size_t)Bq) : (size_t)Bq;   // batches in the self-attn block
    w->cls16 = b.take<bf16_t>((size_t)Bq * Vh);
    w->vp_mid16 = b.take<bf16_t>((size_t)Bq * D * PL / 2);
    w->vp_out32 = b.take<float>((size_t)Bq * D * PL);
    w->pat16 = b.take<bf16_t>((size_t)Bq * np * Vh);
    w->t32 = b.take<float>((size_t)Bq * np * Hh);
    w->t16 = b.take<bf16_t>((size_t)Bq * np * Hh);
    w->vqkv = b.take<bf16_t>(nb * np * 3 * Hh);
    w->vctx = b.take<bf16_t>(nb * np * Hh);
    w->vpre = b.take<float>(nb * np * Hh);
    w->a32 = b.take<float>(nb * np * Hh);
    w->a16 = b.take<bf16_t>(nb * np * Hh);
    w->q_c = b.take<bf16_t>(nb * np * Hh);
    w->enc16 = b.take<bf16_t>((size_t)n * ca * Hh);
    w->kv_c = b.take<bf16_t>((size_t)n * ca * 2 * Hh);
    w->cctx = b.take<bf16_t>((size_t)n * np * Hh);
    w->a32b = b.take<float>((size_t)n * np * Hh);
    w->cpre = b.take<float>((size_t)n * np * Hh);
    w->c32 = b.take<float>((size_t)n * np * Hh);
    w->c16 = b.take<bf16_t>((size_t)n * np * Hh);
    w->vmid = b.take<bf16_t>((size_t)n * np * c.intermediate);
    w->m32 = b.take<float>((size_t)n * np * Hh);
    w->m16 = b.take<bf16_t>((size_t)n * np * Hh);
    w->mo32 = b.take<float>((size_t)n * np * D);
  }
  return (b.off + 255) & ~(size_t)255;
}

}  // namespace
// Growth outside rr_reserve synchronises the stream and replaces the old block: legal on a plain stream, not while the
// stream is being captured into a graph -> refused there.  A graph captured EARLIER holds the old block's address in its
// kernel nodes: once a capture has been SEEN on this handle (pinned_blocks; every forward looks), an outgrown
// block is not freed but retired until rr_destroy, so that replaying such a graph after a later, larger forward stays
// valid (it computes in the old block).
// capture_guard: RR_ERR_BAD_ARG when `st` is being captured, with the caller's sentence about `what` (CAP_*; null: no message).
int capture_guard(rr_model* m, hipStream_t st, const char* sentence, const char* what) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs == hipStreamCaptureStatusNone) return RR_OK;
  return sentence ? fail(m, RR_ERR_BAD_ARG, sentence, what) : RR_ERR_BAD_ARG;
}
// every forward notes a capture in progress, also when nothing has to grow
static void note_capture(rr_model* m, hipStream_t st) {
  if (!m->pinned_blocks && capture_guard(m, st, nullptr, nullptr) != RR_OK) m->pinned_blocks = true;
}
int release_block(rr_model* m, void* p, hipStream_t st) {
  if (!p) return RR_OK;
  RR_HIP(m, hipStreamSynchronize(st));
  if (m->pinned_blocks) m->retired.push_back(p);
  else RR_HIP(m, hipFree(p));
  return RR_OK;
}
namespace {

int ensure_ws(rr_model* m, size_t bytes, hipStream_t st) {
  note_capture(m, st);
  return ensure_block(m, m->ws, m->ws_cap, bytes, st, "the workspace");
}

double gemm_flops(double M, double N, double K) { return 2.0 * M * N * K; }
double gemm_bytes(double M, double N, double K, double out_elt) { return 2.0 * (M * K + N * K) + out_elt * M * N; }

#define RR_GEMM(m, st, A, lda, W, bias, resid, ldr, C, ldc, M, N, K, epi, outb)                         \
  RR_RUN(m, st, RR_K_GEMM, gemm_flops(M, N, K), gemm_bytes(M, N, K, outb) + (((const void*)(resid) != nullptr) ? 4.0 * (M) * (N) : 0.0), \
         rr_launch_gemm(A, lda, W, K, bias, resid, ldr, C, ldc, M, N, K, epi, m->dt, st))

extern "C" int rr_set_gemm_persistent(int on);
extern "C" int rr_set_resid_touch(int on);
extern "C" int rr_set_attn_prio(int on);
extern "C" int rr_set_attn_fixed_ref(int on);
extern "C" int rr_set_resid_fast(int on);
extern "C" int rr_set_gemm_ring_min_tiles(int n);
extern "C" int rr_set_gemm_small_half_rows(int on);
extern "C" int rr_set_gemm_grid_cus(int n);
extern "C" int rr_set_resid_split(int on);
extern "C" int rr_set_gemm_desync(int pct);
extern "C" int rr_set_m_alternate(int on);
int g_ln_lite = 1;   // tuning (rr_set_tuning "ln_lite"): 1 = recompute the residual from LN statistics, 0 = materialise fp32

// Where a layer's residual comes from: either materialised fp32 rows (after an embedding LayerNorm), or the previous
// LayerNorm's INPUT plus its row statistics and affine (the fp32 normalised stream is never written in between).
struct ResidSrc {
  const float* x;
  const float* stats;   // nullptr = x holds the residual itself
  const float* g;
  const float* b;
  // split residual stream (GemmFold in rr_common.h): the rows as hi (16-bit operand rows) + lo (fp16) instead of fp32 x
  const bf16_t* hi = nullptr;
  const bf16_t* lo = nullptr;
};

#define RR_GEMM_LN(m, st, A, lda, W, bias, rs, C, ldc, M, N, K, outb)                                            \
  RR_RUN(m, st, RR_K_GEMM, gemm_flops(M, N, K), gemm_bytes(M, N, K, outb) + 4.0 * (M) * (N),                     \
         rr_launch_gemm_ln(A, lda, W, K, bias, (rs).x, N, (rs).stats, (rs).g, (rs).b, C, ldc, M, N, K,           \
                           EPI_BIAS_RESID_F32, m->dt, st))
// residual GEMM that also emits the 16-bit copy of its rows (-> x16) and their LayerNorm statistics partials
#define RR_GEMM_LN_PREP(m, st, A, lda, W, bias, rs, C, ldc, M, N, K, fold)                                         \
  RR_RUN(m, st, RR_K_GEMM, gemm_flops(M, N, K),                                                                    \
         gemm_bytes(M, N, K, (fold).lo_out ? 2.0 : 4.0) + ((fold).r_hi ? 2.0 + (fold).lo_bits / 8.0 : 4.0) * (M) * (N) + \
             ((fold).lo_out ? (fold).lo_bits / 8.0 : 2.0) * (M) * (N),                                                \
         rr_launch_gemm_fold(A, lda, W, K, bias, (rs).x, N, (rs).stats, (rs).g, (rs).b, fold, C, ldc, M, N, K,     \
                             EPI_BIAS_RESID_F32, m->dt, st))
// GEMM whose A operand holds raw pre-LayerNorm rows; the LayerNorm is applied in the epilogue (folded weights)
#define RR_GEMM_FOLDED(m, st, A, lda, Wf, dvec, fold, C, ldc, M, N, K, epi)                                         \
  RR_RUN(m, st, RR_K_GEMM, gemm_flops(M, N, K), gemm_bytes(M, N, K, 2.0) + 8.0 * (M),                              \
         rr_launch_gemm_fold(A, lda, Wf, K, dvec, nullptr, 0, nullptr, nullptr, nullptr, fold, C, ldc, M, N, K, epi, m->dt, st))

int g_ce_cls_only = 1;                   // tuning (rr_set_tuning "ce_cls_only"): 1 = the cross-encoder's last layer computes the CLS rows only
int g_fp8_ffn_down = 0;                  // tuning (rr_set_tuning "fp8_ffn_down"): 1 = FFN-down of the fp8 configuration on the e4m3 ring too (opt-in: ADVICE r3, DESIGN.md "fp8")
// tuning / option "fp8_first_layer": text-encoder layers below this index keep 16-bit operands in the fp8 configuration.
// -1 (default) = layers - FP8_SAFE_LAYERS: the subset that keeps the fp32 top-5 with margin on every ranking fixture whose list the
// reference's own bf16-autocast arithmetic ranks (tests/test_gpu_fp8.py, profiles/r05_*_fp8_subset_study.json; DESIGN.md "fp8").  ONE
// layer: with two the centred drift on the binding lists is 0.14 - 0.19 against half-gaps of 0.18 / 0.25 depending on how unrelated
// roundings fall (the degree of the GELU polynomial moved it from 0.137 to 0.193) — no margin; with one it is 0.09 - 0.10.
int g_fp8_first_layer = -1;
constexpr int FP8_SAFE_LAYERS = 1;
// The default for int8 handles ("q8_format" 1): the last INT8_SAFE_LAYERS layers, the largest suffix that ranks with margin on the
// c5 ranking fixtures (tests/tools/int8_subset_study.py, profiles/r06_int8_subset_study.json; DESIGN.md "int8").  TWELVE: on the binding
// list c5_sep_wide q0 the centred drift is 0.150 with 12 int8 layers, 0.206 with 18 and 0.197 with all 24, against a half-gap of
// 0.180 (16 / 8 layers: 0.100 / 0.074) — the whole stack does not rank with margin, twelve layers do.
constexpr int INT8_SAFE_LAYERS = 12;
inline int fp8_first_layer_of(int opt, int layers, bool i8 = false) {
  const int safe = i8 ? INT8_SAFE_LAYERS : FP8_SAFE_LAYERS;
  return opt >= 0 ? (opt < layers ? opt : layers) : (layers > safe ? layers - safe : 0);
}
// tuning / option "q8_format": the 8-bit operand format of rr_config.fp8 — 0 e4m3 (block-scaled MFMA), 1 int8 (W8A8: int8 MFMA,
// int32 accumulation, per-row activation / per-channel weight scales, LayerNorm gains migrated into the weights).  Latched by
// rr_finalize_weights, which packs the weights in that one format.
int g_q8_format = 0;
// tuning "q8_smooth" (diagnostic, read by rr_finalize_weights): 1 = the int8 packer migrates LayerNorm gain outliers into the
// consumer weights (host_smooth_scales), 0 = plain per-channel int8 (shows what the smoothing is worth)
int g_q8_smooth = 1;
int g_fp8_qkv = 1;                       // tuning / option "fp8_qkv": 0 = only the FFN of an fp8 layer takes e4m3 operands, its QKV projection stays 16-bit
constexpr float FP8_GELU_MUL = 8.0f;     // static scale of the e4m3 GELU output feeding it
int g_ln_fold = 1;   // tuning (rr_set_tuning "ln_fold"): 1 = LayerNorm folded into the consumer GEMMs, 0 = LayerNorm kernels
// tuning / option "resid_lo8": 1 = the lo half of the split residual stream travels as e5m2 bytes (rr_common.h RR_LO8_SHIFT; 6 instead
// of 8 bytes per element through the residual epilogues, x kept to >= 14 / 11 significant bits), 0 = as fp16 (22 / 19 bits).
// -1 (the built-in default) = by operand type: 1 for fp16 handles — three more bits than the operand the GEMMs read anyway, the
// drift against the fp32 goldens does not move (profiles/r05_ad_lo8_forced_margins.json) — and 0 for bf16 handles, whose 8-bit hi would
// leave x at 11 bits (c3_full 2.8e-3 -> 3.3e-3, c5_full 3.4e-3 -> 4.3e-3: inside the gate, but not given away by default).
// (environment RR_RESID_LO8 = 0 | 1 overrides the built-in default for a whole process: lets the unmodified test suite run either form)
static int resid_lo8_default() { const char* e = getenv("RR_RESID_LO8"); return e && *e ? atoi(e) != 0 : RR_RESID_LO8_DEFAULT; }
int g_resid_lo8 = resid_lo8_default();
inline bool resid_lo8_of(int opt, int dt) { return opt < 0 ? dt == 1 : opt != 0; }

// limit of the range guard (ln_finalize_kernel): fp16 operand rows are refused from 3e4 on, bf16 rows only when not finite
inline float range_ss_of(const rr_model* m) { return m->dt == 1 ? RR_RANGE_SS_FP16 : __builtin_inff(); }

extern "C" int rr_get_resid_split(void);
// effective value of a handle option: the handle's own setting, else the process-wide switch
inline int opt_of(const rr_model* m, int which) {
  if (m->opt[which] >= 0) return m->opt[which];
  switch (which) {
    case RR_OPT_LN_LITE: return g_ln_lite;
    case RR_OPT_LN_FOLD: return g_ln_fold;
    case RR_OPT_CE_CLS_ONLY: return g_ce_cls_only;
    case RR_OPT_FP8_FFN_DOWN: return g_fp8_ffn_down;
    case RR_OPT_RESID_SPLIT: return rr_get_resid_split();
    case RR_OPT_FP8_FIRST_LAYER: return g_fp8_first_layer;
    case RR_OPT_FP8_QKV: return g_fp8_qkv;
    case RR_OPT_RESID_LO8: return g_resid_lo8;
    case RR_OPT_Q8_FORMAT: return m->q8_fmt >= 0 ? m->q8_fmt : g_q8_format;
    default: return -1;      // RR_OPT_ATTN_FIXED_REF: -1 lets the attention launcher take its own process-wide mode
  }
}

// One post-LN BertLayer over `rows` = batch*Tseq rows (self-attention only).
// In: the previous LayerNorm's output as MFMA operand in w.h16 — either normalised (`folded_in` false: after an embedding
// LayerNorm, or when folding is off) or, `folded_in` true, the RAW rows of that LayerNorm's input, whose statistics are
// rs.stats and whose affine is folded into L.wqkv_f — and `rs`, where the residual comes from.
// Out: w.h16 / folded_in / rs for the next layer (and w.h32 + normalised w.h16 when `want_h32`: last layer of a stack).
//
// Folded dataflow (north_star "fused LayerNorm+QKV"): no LayerNorm kernel between the GEMMs.  The residual GEMMs
// (attention output, FFN down) write their fp32 rows, the same rows in 16 bits and per-row statistics partials; a
// rows x 8-byte finalize merges the partials; QKV / FFN-up read the raw 16-bit rows and apply (mean, rstd) in their
// epilogue: LN(x) W^T + b = rstd (x W'^T - mean c) + d.
enum OperandKind { OP_NORMALISED = 0, OP_RAW_FOLDED = 1, OP_E4M3 = 2 };   // what w.h16 holds on entry to a layer (see run_layer; OP_E4M3: the 8-bit codes of "q8_format")

#define RR_GEMM_FP8(m, st, A8, lda, W8, bias, rsc, csc, C, ldc, M, N, K, epi)                                       \
  RR_RUN(m, st, RR_K_GEMM_FP8, gemm_flops(M, N, K), 1.0 * (M) * (K) + 1.0 * (N) * (K) + 2.0 * (M) * (N) + 4.0 * (M), \
         (m)->q8_fmt == 1                                                                                              \
             ? rr_launch_gemm_i8((const int8_t*)(A8), lda, (const int8_t*)(W8), K, bias, 1.0f, rsc, csc, C, ldc, M, N, K, epi, m->dt, st) \
             : rr_launch_gemm_fp8((const uint8_t*)(A8), lda, W8, K, bias, 1.0f, rsc, csc, C, ldc, M, N, K, epi, m->dt, st))
// the LayerNorm that quantises a GEMM operand: e4m3 with the true affine, int8 with its private (smoothed) one
#define RR_LN_Q8(m, st, x, L, which, eps, rows, Hd, stats)                                                              \
  RR_RUN(m, st, RR_K_LAYERNORM, 0.0, 5.0 * (rows) * (Hd),                                                              \
         (m)->q8_fmt == 1 ? rr_launch_layernorm_i8(x, (L).which##g_q, (L).which##b_q, eps, rows, Hd, (int8_t*)w.h16, w.rowscale, stats, st) \
                          : rr_launch_layernorm_q8(x, (L).which##g, (L).which##b, eps, rows, Hd, (uint8_t*)w.h16, w.rowscale, stats, st))

// Packed execution (rr_forward_packed): the pairs of a call are grouped into SEGMENTS of equal row length; a segment's pairs
// lie back to back in every activation buffer, the segments one after the other, so the row-wise kernels (every GEMM, the
// LayerNorm statistics) run ONCE over all rows of the call while the kernels that know where a pair starts (attention, the
// embeddings, the gathers, the CLS heads) are launched once per segment on offset pointers.  The plain forward is the
// special case of one segment.
struct Seg {
  int n, S, T;             // pairs; text rows per pair; cross-encoder rows per pair (S + vision tokens)
  size_t p0, r0, rt0;      // first pair; first text row; first cross-encoder row of the segment
};
struct SegView {           // what run_layer needs: rows per pair and the first row of every segment, for ONE of the two stacks
  int n, len;
  size_t row0;
};

int run_layer(rr_model* m, hipStream_t st, const LayerW& L, int batch, int Tseq, int Hd, int heads, int I, float eps,
              const float* key_bias, Work& w, ResidSrc& rs, int& in_kind, bool want_h32, bool want_f32,
              const float* dense_bias = nullptr, int dense_ld = 0, const std::vector<SegView>* segs = nullptr, int fp8_layer = -1,
              bool next_fp8 = false) {
  // fp8_layer: -1 = every layer that holds e4m3 weights runs the fp8 configuration (cfg.fp8), 0 / 1 = the caller's per-layer
  // choice ("fp8_first_layer"); next_fp8: the NEXT layer of the stack runs the fp8 configuration, whose residual epilogues read
  // fp32 rows — a folded layer in front of it leaves its output rows as fp32 (w.pre2) instead of the (hi, lo) pair.
  // segs + dense_bias (packed attention fusion, rr_forward_*_packed): the bias holds the segments one after the other, segment
  // i as [n_i][len_i][round_up(len_i, 64)] (dense_ld is not read)
  int rows = batch * Tseq;
  if (segs) {
    size_t r = 0;
    for (const SegView& g : *segs) r += (size_t)g.n * g.len;
    rows = (int)r;
  }
  const int nparts = (Hd + 127) / 128;
  const bool ln_lite = opt_of(m, RR_OPT_LN_LITE) != 0;
  const int attn_mode = opt_of(m, RR_OPT_ATTN_FIXED_REF);
  const bool fp8 = m->cfg.fp8 && fp8_layer != 0 && ln_lite && L.w1_8 && (Hd % 128 == 0);
  const bool fp8_qkv_next = opt_of(m, RR_OPT_FP8_QKV) != 0;      // the e4m3 rows this layer leaves feed the next layer's QKV projection
  const bool fold = !fp8 && opt_of(m, RR_OPT_LN_FOLD) && ln_lite && L.w1_f && (Hd % 8 == 0);
  if (in_kind == OP_RAW_FOLDED) {
    if (!L.wqkv_f) return fail(m, RR_ERR_BAD_ARG, "internal: folded operand into a layer without folded QKV weights");
    GemmFold f;
    f.in_stats = rs.stats;
    f.csum = L.cqkv_f;
    RR_GEMM_FOLDED(m, st, w.h16, Hd, L.wqkv_f, L.dqkv_f, f, w.qkv, 3 * Hd, rows, 3 * Hd, Hd, EPI_BIAS_BF16);
  } else if (in_kind == OP_E4M3) {
    if (!L.wqkv8) return fail(m, RR_ERR_BAD_ARG, "internal: e4m3 operand into a layer without e4m3 QKV weights");
    RR_GEMM_FP8(m, st, w.h16, Hd, L.wqkv8, L.bqkv, w.rowscale, L.sqkv, w.qkv, 3 * Hd, rows, 3 * Hd, Hd, 0);
  } else {
    RR_GEMM(m, st, w.h16, Hd, L.wqkv, L.bqkv, nullptr, 0, w.qkv, 3 * Hd, rows, 3 * Hd, Hd, EPI_BIAS_BF16, 2.0);
  }
  if (segs && dense_bias) {
    // the padded call with a dense bias runs the online form whatever its grid (the fixed-reference schedule excludes it):
    // one online launch per segment on offset pointers is that call's arithmetic for every pair
    const float* db = dense_bias;
    for (const SegView& g : *segs) {
      const int ld = (g.len + 63) / 64 * 64;
      const size_t o = g.row0;
      RR_RUN(m, st, RR_K_ATTENTION, 4.0 * g.n * (double)g.len * g.len * Hd, 2.0 * 4.0 * g.n * g.len * Hd + 4.0 * g.n * g.len * ld,
             rr_launch_attention(w.qkv + o * 3 * Hd, 3 * Hd, 1, 0, w.qkv + o * 3 * Hd + Hd, w.qkv + o * 3 * Hd + 2 * Hd, 3 * Hd,
                                 key_bias + o, g.n, heads, g.len, g.len, w.ctx + o * Hd, Hd, m->dt, st, db, ld, 0, attn_mode));
      db += (size_t)g.n * g.len * ld;
    }
  } else if (segs) {
    // the schedule (online / fixed reference) of the PADDED call over the same pairs: batch pairs of Tseq rows; all segments
    // in ONE launch (rr_launch_attention_segs) where that schedule is the fixed-reference one
    const long sched = (((long)batch * heads + 7) / 8) * 8 * ((Tseq + 127) / 128);
    std::vector<int> sn, sl;
    std::vector<long long> sr;
    double fl = 0.0;
    for (const SegView& g : *segs) {
      sn.push_back(g.n); sl.push_back(g.len); sr.push_back((long long)g.row0);
      fl += 4.0 * g.n * (double)g.len * g.len * Hd;
    }
    RR_RUN(m, st, RR_K_ATTENTION, fl, 2.0 * 4.0 * rows * Hd,
           rr_launch_attention_segs(w.qkv, 3 * Hd, w.qkv + Hd, w.qkv + 2 * Hd, 3 * Hd, key_bias, heads, (int)sn.size(), sn.data(),
                                    sl.data(), sr.data(), w.ctx, Hd, m->dt, st, sched, attn_mode));
  } else {
    RR_RUN(m, st, RR_K_ATTENTION, 4.0 * batch * (double)Tseq * Tseq * Hd, 2.0 * 4.0 * rows * Hd,
           rr_launch_attention(w.qkv, 3 * Hd, 1, 0, w.qkv + Hd, w.qkv + 2 * Hd, 3 * Hd, key_bias, batch, heads, Tseq,
                               Tseq, w.ctx, Hd, m->dt, st, dense_bias, dense_ld, 0, attn_mode));
  }
  if (!ln_lite) {   // reference dataflow for A/B runs: every LayerNorm writes the fp32 stream, residuals read it back
    RR_GEMM_LN(m, st, w.ctx, Hd, L.wo, L.bo, rs, w.pre, Hd, rows, Hd, Hd, 4.0);
    RR_RUN(m, st, RR_K_LAYERNORM, 0.0, 10.0 * rows * Hd,
           rr_launch_layernorm(w.pre, L.ln1g, L.ln1b, eps, rows, Hd, w.h32, w.h16, m->dt, st));
    RR_GEMM(m, st, w.h16, Hd, L.w1, L.b1, nullptr, 0, w.mid, I, rows, I, Hd, EPI_BIAS_GELU_BF16, 2.0);
    const ResidSrc r0{w.h32, nullptr, nullptr, nullptr};
    RR_GEMM_LN(m, st, w.mid, I, L.w2, L.b2, r0, w.pre, Hd, rows, Hd, I, 4.0);
    RR_RUN(m, st, RR_K_LAYERNORM, 0.0, 10.0 * rows * Hd,
           rr_launch_layernorm(w.pre, L.ln2g, L.ln2b, eps, rows, Hd, w.h32, w.h16, m->dt, st));
    rs = r0;
    in_kind = OP_NORMALISED;
    return RR_OK;
  }
  if (fp8) {
    // configs[4]: the two LayerNorm outputs are quantised to e4m3 (one scale per row) by the LayerNorm kernel itself and
    // feed FFN-up / the next layer's QKV on the block-scaled matrix core; attention output and FFN-down stay 16-bit
    RR_GEMM_LN(m, st, w.ctx, Hd, L.wo, L.bo, rs, w.pre, Hd, rows, Hd, Hd, 4.0);
    RR_LN_Q8(m, st, w.pre, L, ln1, eps, rows, Hd, w.stats_a);
    const ResidSrc r1{w.pre, w.stats_a, L.ln1g, L.ln1b};
    // FFN-down on the e4m3 ring as well (rr_set_tuning "fp8_ffn_down", default 1) where both GEMMs of the FFN run the
    // persistent kernel: the GELU epilogue of FFN-up emits e4m3 bytes under ONE static power-of-two scale (GELU's range is
    // [-0.17, max pre-activation]: x 8 keeps 3 mantissa bits down to 2e-3 and saturates at 56), FFN-down multiplies its
    // accumulators by 1/8 and its per-channel weight scales and adds the LayerNorm-recomputed residual row in its epilogue
    if (m->q8_fmt == 1 && opt_of(m, RR_OPT_FP8_FFN_DOWN))
      return fail(m, RR_ERR_BAD_ARG, "fp8_ffn_down = 1 needs q8_format 0 (there is no int8 FFN-down)");
    const bool down8 = opt_of(m, RR_OPT_FP8_FFN_DOWN) && L.w2_8 && (I % 128 == 0) && rr_gemm_fp8_ring_ok(rows, I, Hd) && rr_gemm_fp8_ring_ok(rows, Hd, I);
    if (down8) {
      RR_RUN(m, st, RR_K_GEMM_FP8, gemm_flops(rows, I, Hd), 1.0 * rows * Hd + 1.0 * I * Hd + 1.0 * rows * I + 4.0 * rows,
             rr_launch_gemm_fp8((const uint8_t*)w.h16, Hd, L.w1_8, Hd, L.b1, 1.0f, w.rowscale, L.s1, w.mid, I, rows, I, Hd, 3, m->dt, st,
                                FP8_GELU_MUL));
      RR_RUN(m, st, RR_K_GEMM_FP8, gemm_flops(rows, Hd, I), 1.0 * rows * I + 1.0 * Hd * I + 8.0 * rows * Hd + 8.0 * rows,
             rr_launch_gemm_fp8((const uint8_t*)w.mid, I, L.w2_8, I, L.b2, 1.0f / FP8_GELU_MUL, nullptr, L.s2, w.pre2, Hd, rows, Hd, I, 4,
                                m->dt, st, 1.0f, r1.x, Hd, r1.stats, r1.g, r1.b));
    } else {
      RR_GEMM_FP8(m, st, w.h16, Hd, L.w1_8, L.b1, w.rowscale, L.s1, w.mid, I, rows, I, Hd, 1);
      RR_GEMM_LN(m, st, w.mid, I, L.w2, L.b2, r1, w.pre2, Hd, rows, Hd, I, 4.0);
    }
    if (want_h32 || !fp8_qkv_next || !next_fp8) {      // 16-bit normalised rows: end of the stack, "fp8_qkv" 0, or a 16-bit layer follows
      RR_RUN(m, st, RR_K_LAYERNORM, 0.0, (want_h32 && want_f32 ? 10.0 : 6.0) * rows * Hd,
             rr_launch_layernorm_stats(w.pre2, L.ln2g, L.ln2b, eps, rows, Hd, want_h32 && want_f32 ? w.h32 : nullptr, w.h16, w.stats_b,
                                       m->dt, st));
      in_kind = OP_NORMALISED;
    } else {
      RR_LN_Q8(m, st, w.pre2, L, ln2, eps, rows, Hd, w.stats_b);
      in_kind = OP_E4M3;
    }
    rs = ResidSrc{w.pre2, w.stats_b, L.ln2g, L.ln2b};
    return RR_OK;
  }
  if (fold) {
    // Split residual stream (rr_gemm_split_ok: the persistent ring kernel runs these shapes): a pre-LayerNorm row lives
    // as hi = the 16-bit operand rows in w.h16 + lo = fp16(x - hi) in the memory of w.pre, both updated in place by the
    // residual epilogues (an element is read and written by the same thread), instead of a third, fp32 copy: 8 instead of
    // 10 bytes per element through the two HBM-bound epilogues of a layer — 6 with "resid_lo8" (lo as e5m2 bytes in the same
    // memory, rows paired for 16-byte accesses: rr_common.h lo8_pair_offset), the default of fp16 handles.  The last layer of a stack writes fp32 rows
    // (w.pre2) for the LayerNorm kernel that materialises the stack's output.
    const bool split = opt_of(m, RR_OPT_RESID_SPLIT) && rr_gemm_split_ok(rows, Hd);
    bf16_t* const lo16 = (bf16_t*)w.pre;          // (with "resid_lo8": rows of Hd BYTES in the same memory)
    GemmFold fo;
    fo.lo_bits = resid_lo8_of(opt_of(m, RR_OPT_RESID_LO8), m->dt) ? 8 : 16;
    fo.x16 = w.h16;
    fo.ldx = Hd;
    fo.part = w.lnpart;
    fo.nparts = nparts;
    GemmFold f1 = fo;                      // attention-out: residual = rs, output -> (h16, lo16) or fp32 w.pre
    f1.r_hi = rs.hi; f1.r_lo = rs.lo; f1.ld16 = Hd;
    if (split) f1.lo_out = lo16;
    RR_GEMM_LN_PREP(m, st, w.ctx, Hd, L.wo, L.bo, rs, w.pre, Hd, rows, Hd, Hd, f1);
    RR_RUN(m, st, RR_K_LAYERNORM, 0.0, 8.0 * rows * (nparts + 1),
           rr_launch_ln_finalize(w.lnpart, nparts, Hd, eps, rows, w.stats_a, st, m->range_flag, range_ss_of(m)));
    GemmFold fi;
    fi.in_stats = w.stats_a;
    fi.csum = L.c1_f;
    RR_GEMM_FOLDED(m, st, w.h16, Hd, L.w1_f, L.d1_f, fi, w.mid, I, rows, I, Hd, EPI_BIAS_GELU_BF16);
    ResidSrc r1{w.pre, w.stats_a, L.ln1g, L.ln1b};
    if (split) { r1.x = nullptr; r1.hi = w.h16; r1.lo = lo16; }
    GemmFold f2 = fo;                      // FFN-down: residual = r1, output -> (h16, lo16) in place, or fp32 w.pre2
    f2.r_hi = r1.hi; f2.r_lo = r1.lo; f2.ld16 = Hd;
    const bool split_out = split && !want_h32 && !next_fp8;
    if (split_out) f2.lo_out = lo16;
    RR_GEMM_LN_PREP(m, st, w.mid, I, L.w2, L.b2, r1, w.pre2, Hd, rows, Hd, I, f2);
    RR_RUN(m, st, RR_K_LAYERNORM, 0.0, 8.0 * rows * (nparts + 1),
           rr_launch_ln_finalize(w.lnpart, nparts, Hd, eps, rows, w.stats_b, st, m->range_flag, range_ss_of(m)));
    rs = ResidSrc{w.pre2, w.stats_b, L.ln2g, L.ln2b};
    if (split_out) { rs.x = nullptr; rs.hi = w.h16; rs.lo = lo16; }
    in_kind = OP_RAW_FOLDED;
    if (want_h32) {   // last layer of a stack: its consumers (CLS heads, 768->128 projection, debug taps) take normalised rows
      RR_RUN(m, st, RR_K_LAYERNORM, 0.0, (want_f32 ? 10.0 : 6.0) * rows * Hd,
             rr_launch_layernorm(w.pre2, L.ln2g, L.ln2b, eps, rows, Hd, want_f32 ? w.h32 : nullptr, w.h16, m->dt, st));
      in_kind = OP_NORMALISED;
    }
    return RR_OK;
  }
  RR_GEMM_LN(m, st, w.ctx, Hd, L.wo, L.bo, rs, w.pre, Hd, rows, Hd, Hd, 4.0);
  RR_RUN(m, st, RR_K_LAYERNORM, 0.0, 6.0 * rows * Hd,
         rr_launch_layernorm_stats(w.pre, L.ln1g, L.ln1b, eps, rows, Hd, nullptr, w.h16, w.stats_a, m->dt, st));
  RR_GEMM(m, st, w.h16, Hd, L.w1, L.b1, nullptr, 0, w.mid, I, rows, I, Hd, EPI_BIAS_GELU_BF16, 2.0);
  const ResidSrc r1{w.pre, w.stats_a, L.ln1g, L.ln1b};
  RR_GEMM_LN(m, st, w.mid, I, L.w2, L.b2, r1, w.pre2, Hd, rows, Hd, I, 4.0);
  RR_RUN(m, st, RR_K_LAYERNORM, 0.0, ((want_h32 && want_f32) ? 10.0 : 6.0) * rows * Hd,
         rr_launch_layernorm_stats(w.pre2, L.ln2g, L.ln2b, eps, rows, Hd, (want_h32 && want_f32) ? w.h32 : nullptr, w.h16,
                                   w.stats_b, m->dt, st));
  rs = ResidSrc{w.pre2, w.stats_b, L.ln2g, L.ln2b};
  in_kind = OP_NORMALISED;
  return RR_OK;
}

// One forward call as an exported entry point hands it over (include/rerank_mi355.h); forward_full and forward_interaction
// take it.  FAM_INTERACTION is NORMAL or MORES, after the handle's model_kind.
enum Family { FAM_FULL, FAM_JOINT, FAM_INTERACTION };
struct Request {
  Family family = FAM_FULL;
  // full / joint: token ids, attention mask, token types [pairs, len] and the per-query image features
  const int64_t *ids = nullptr, *mask = nullptr, *token_types = nullptr;
  const float *image_cls = nullptr, *image_patches = nullptr;
  // interaction: late-interaction tensors query_li [Bq, Lq, D], context_li [N, Lc, D] and their 0/1 masks
  const float *query_li = nullptr, *context_li = nullptr, *query_mask = nullptr, *context_mask = nullptr;
  int Bq = 0, K = 0;
  int len = 0;                 // full / joint: S, the row length (packed: the padded one); interaction: Lc, the context length
  int q_len = 0;               // joint: query tokens at the head of the joint sequence; interaction: Lq
  long long instruction_token = -1;
  const float* labels = nullptr;
  int pair_begin = 0, pair_end = 0;
  float *logits = nullptr, *logits2 = nullptr, *loss = nullptr, *scores = nullptr;
  int32_t* order = nullptr;
  hipStream_t stream = nullptr;
  const float* fusion_scores = nullptr;   // PreFLMR attention fusion (joint / NORMAL interaction)
  float fusion_mult = 1.0f;
  bool fusion_from_li = false;            // interaction: the fusion scores are computed from the call's own tensors (rr_li_scores)
  float* maxsim = nullptr;                // ... and the retriever's MaxSim of every pair [N] goes here (optional)
  bool packed = false;                    // rr_forward_*_packed: the segment table (pairs, length per pair)
  int n_segments = 0;
  const int32_t *seg_pairs = nullptr, *seg_len = nullptr;
  // rr_forward_interaction_bank: the context rows and masks come from `bank` through the checked per-pair descriptors (packed pair
  // order); query_li / query_mask are per QUERY and the descriptors name each pair's query
  const rr_bank* bank = nullptr;
  const std::vector<rr_bank_pair>* bank_pairs = nullptr;
};

// The rows of a forward: the segment list (one segment for a padded or length-bucketed call) and what the cross-encoder needs
// to know about it.
struct RowPlan {
  std::vector<Seg> segs;
  int n = 0;                   // pairs
  bool packed = false;         // the call came as a segment table: the text stack runs per segment
  bool ce_segs = false;        // the cross-encoder runs per segment (run_layer's SegView list)
  int vis_pos0 = -1;           // first cross-encoder position of the vision tokens; -1: plain positions 0 .. T-1
  int sched_T = 0;             // rows per pair the cross-encoder's attention schedule assumes
};

// `len` rows per pair of the call (packed: the padded length) plus `extra` cross-encoder rows (vision tokens P; interaction:
// query tokens Lq).  bucket_of > 0: a full-context call of a shorter length bucket (rr_set_padded_seq_len), whose vision
// tokens keep the positions behind the padded text.
RowPlan plan_rows(Family fam, int n, int len, int extra, const std::vector<std::pair<int, int>>& table, int bucket_of) {
  RowPlan p;
  p.n = n;
  p.packed = !table.empty();
  size_t p0 = 0, r0 = 0, rt0 = 0;
  for (const auto& g : table) {
    p.segs.push_back(Seg{g.first, g.second, g.second + extra, p0, r0, rt0});
    p0 += (size_t)g.first;
    r0 += (size_t)g.first * g.second;
    rt0 += (size_t)g.first * (g.second + extra);
  }
  if (!p.packed) p.segs.push_back(Seg{n, len, len + extra, 0, 0, 0});
  const bool full = fam == FAM_FULL;      // (joint: [query | image | context] is padded at its end, no position moves)
  p.vis_pos0 = !full ? -1 : p.packed ? len : bucket_of > 0 ? bucket_of : -1;
  // a full-context packed call of ONE segment runs its cross-encoder as a bucketed call does, on the schedule of its own rows
  p.ce_segs = p.packed && !(full && p.segs.size() == 1);
  p.sched_T = p.ce_segs ? len + extra : p.segs.back().T;   // (per segment: the padded call's rows per pair)
  return p;
}

// The scoring head over complete logits [Bq, K] (rr_launch_head).  joint: RerankModel's loss_fn(logits, logits)
// (rerank_model.py:328) — the logits are their own targets, and 2H_BCE takes loss kind 3.
int launch_head(rr_model* m, hipStream_t st, const Work& w, const float* logits, const float* logits2, const float* labels, int Bq,
                int K, bool joint, float* loss, float* scores, int32_t* order) {
  const rr_config& c = m->cfg;
  const bool two = c.loss_kind == RR_LOSS_2H_BCE;
  const int has_pw = !std::isnan(c.pos_weight);
  RR_RUN(m, st, RR_K_HEAD, 0.0, 12.0 * Bq * K,
         rr_launch_head(logits, two ? logits2 : nullptr, joint ? logits : labels, Bq, K, (joint && two) ? 3 : c.loss_kind,
                        has_pw ? c.pos_weight : 1.0f, has_pw, scores, order, loss, w.part_l, w.part_w, st));
  return RR_OK;
}

// The head and pair-slice part of a request (both forwards, rr_head, rr_head_joint): loss / scores / order need every pair,
// and what the scoring head reads must be there when it runs.
int check_head(rr_model* m, const char* what, int Bq, int K, int pair_begin, long long pair_end, const float* labels,
               const float* logits2, const float* loss, const float* scores, const int32_t* order, bool joint) {
  const rr_config& c = m->cfg;
  const long long N = (long long)Bq * K;
  if (pair_begin < 0 || pair_end > N || pair_begin >= pair_end)
    return fail(m, RR_ERR_BAD_SHAPE, "%s: pair slice [%d,%lld) outside [0,%lld)", what, pair_begin, pair_end, N);
  const bool full = pair_begin == 0 && pair_end == N, head = loss || scores || order;
  if (c.loss_kind == RR_LOSS_NEGATIVE_SAMPLING && labels)
    return fail(m, RR_ERR_BAD_ARG, "Labels should not be provided for negative sampling loss function");
  if (!full && head) return fail(m, RR_ERR_BAD_ARG, "loss/scores/order need the full pair range; use rr_head after gathering logits");
  if (c.loss_kind == RR_LOSS_2H_BCE && head && !logits2) return fail(m, RR_ERR_BAD_ARG, "%s: 2H_BCE head needs logits2 (first head)", what);
  if (K > 4096 && head) return fail(m, RR_ERR_UNSUPPORTED, "%s: K=%d > 4096", what, K);
  if (joint && c.loss_kind == RR_LOSS_NEGATIVE_SAMPLING && loss)
    return fail(m, RR_ERR_UNSUPPORTED, "RerankModel with negative_sampling loss is not covered (no reference config)");
  return RR_OK;
}

}  // namespace
// Row counts travel as int through the layer chain (run_layer's `rows`, the row kernels' grids and their n * T products): a call
// whose n pairs of T rows do not fit is refused here, before anything is allocated or launched.  2^30 rows is the limit of the
// packed calls too (packed_segments); the workspace of that many rows is beyond any card (audit: tests/test_gpu_large_index.py).
constexpr long long RR_MAX_ROWS = 1LL << 30;
int check_rows(rr_model* m, const char* what, long long n, int T) {
  if (n * (long long)T > RR_MAX_ROWS) return fail(m, RR_ERR_BAD_SHAPE, "%s: %lld pairs of %d rows exceed %lld rows per call", what, n, T, RR_MAX_ROWS);
  return RR_OK;
}
namespace {

// CLS heads + (when this call covers every pair) the scoring head.  classifier1 -> "logits", classifier2 ->
// "logits_secondary" (utils.py:105-108); for 2H_BCE the ranked logit is the second head (rerank_model.py:589-590).
int run_heads(rr_model* m, hipStream_t st, Work& w, const std::vector<Seg>& segs, const Request& r) {
  const rr_config& c = m->cfg;
  const int Hc = c.ce_hidden;
  std::vector<Seg> one;
  if (m->cls_rows) {      // the cross-encoder's last layer ran on the CLS rows only (run_cross_encoder): n contiguous rows
    int n = 0;
    for (const Seg& g : segs) n += g.n;
    one.push_back(Seg{n, 1, 1, 0, 0, 0});
  }
  for (const Seg& g : (m->cls_rows ? one : segs)) {
    float* out_a = r.logits + r.pair_begin + g.p0;
    float* out_b = (r.logits2 ? r.logits2 + r.pair_begin : w.l2) + g.p0;
    const float* h = m->cls_rows ? m->cls_rows : w.h32 + g.rt0 * Hc;
    if (c.loss_kind == RR_LOSS_2H_BCE) {
      RR_RUN(m, st, RR_K_HEAD, 4.0 * g.n * Hc, 8.0 * g.n * Hc,
             rr_launch_cls_heads(h, g.T, Hc, g.n, m->cls2_w, m->cls2_b, m->cls1_w, m->cls1_b, out_a, out_b, st));
    } else {
      RR_RUN(m, st, RR_K_HEAD, 4.0 * g.n * Hc, 8.0 * g.n * Hc,
             rr_launch_cls_heads(h, g.T, Hc, g.n, m->cls1_w, m->cls1_b, m->cls2_w, m->cls2_b, out_a, out_b, st));
    }
  }
  if (r.pair_begin == 0 && r.pair_end == r.Bq * r.K && (r.loss || r.scores || r.order))
    return launch_head(m, st, w, r.logits, r.logits2, r.labels, r.Bq, r.K, r.family == FAM_JOINT, r.loss, r.scores, r.order);
  return RR_OK;
}

// CrossEncoder over AttentionFusionBertModel (utils.py:85-108, attention_fusion.py:61-160): Linear(D -> Hc) ->
// embeddings(inputs_embeds) -> Lc layers.  Input: w.li16 [n*T, D], w.ce_bias [n, T]; output: w.h32 [n*T, Hc].
// The rows, the vision tokens' positions and the attention schedule come from the plan (plan_rows).  Per segment with `adj`:
// the bias is laid out per segment (run_layer).
int run_cross_encoder(rr_model* m, hipStream_t st, Work& w, const RowPlan& plan, const float* adj, int adj_ld) {
  const rr_config& c = m->cfg;
  const std::vector<Seg>& segs = plan.segs;
  const int vis_pos0 = plan.vis_pos0;
  const int D = c.li_dim, Hc = c.ce_hidden, Ic = c.ce_intermediate;
  const Seg& last = segs.back();
  const int RT = (int)(last.rt0 + (size_t)last.n * last.T);
  int n = 0;
  for (const Seg& g : segs) n += g.n;
  RR_GEMM(m, st, w.li16, D, m->w_cemap, m->b_cemap, nullptr, 0, w.pre, Hc, RT, Hc, D, EPI_BIAS_F32, 4.0);
  std::vector<SegView> view;
  const bool cls_only = opt_of(m, RR_OPT_CE_CLS_ONLY) && !m->debug && !adj && c.ce_layers == 1;
  for (const Seg& g : segs) {      // (cls_only: the fp32 copy of the embedding rows is the residual of the CLS rows only)
    RR_RUN(m, st, RR_K_EMBED, 0.0, (cls_only ? 10.0 : 14.0) * g.n * g.T * Hc,
           rr_launch_ce_embed_ln(w.pre + g.rt0 * Hc, m->ce_pos, m->ce_type, m->ce_emb_g, m->ce_emb_b, c.ln_eps, g.n * g.T, g.T, Hc,
                                 w.h32 + g.rt0 * Hc, w.h16 + g.rt0 * Hc, m->dt, st, vis_pos0 >= 0 ? g.S : -1,
                                 vis_pos0 >= 0 ? vis_pos0 : 0, cls_only ? 1 : 0));
    view.push_back(SegView{g.n, g.T, g.rt0});
  }
  m->cls_rows = nullptr;
  if (cls_only) {
    // Only the CLS row of every pair leaves the cross-encoder (the classifiers read hidden state [:, 0], utils.py:105-108):
    // in its LAST layer every row is needed as a key and a value, but queries, attention output, both LayerNorms and the
    // FFN only for that one row.  With one layer (every reference config: cross_encoder_num_hidden_layers = 1) the input is
    // the materialised embedding LayerNorm output, so: K / V projection over all rows, then n-row launches for the rest.
    // The reference computes all T rows and drops T - 1 of them; the taps (rr_set_debug) keep the full layer.
    const LayerW& L = m->ce_layers[0];
    const int heads = c.ce_heads;
    Bump b(w.cls_scratch);
    bf16_t* x16 = b.take<bf16_t>((size_t)n * Hc);
    float* x32 = b.take<float>((size_t)n * Hc);
    bf16_t* q16 = b.take<bf16_t>((size_t)n * Hc);
    bf16_t* ctx16 = b.take<bf16_t>((size_t)n * Hc);
    float* pre_a = b.take<float>((size_t)n * Hc);
    float* a32 = b.take<float>((size_t)n * Hc);
    bf16_t* a16 = b.take<bf16_t>((size_t)n * Hc);
    bf16_t* mid16 = b.take<bf16_t>((size_t)n * Ic);
    float* pre_b = b.take<float>((size_t)n * Hc);
    float* out32 = b.take<float>((size_t)n * Hc);
    bf16_t* out16 = b.take<bf16_t>((size_t)n * Hc);
    if (b.off > cls_scratch_bytes(c, n)) return fail(m, RR_ERR_BAD_ARG, "internal: CLS-only scratch %zu > %zu bytes", b.off, cls_scratch_bytes(c, n));
    RR_GEMM(m, st, w.h16, Hc, L.wqkv + (size_t)Hc * Hc, L.bqkv + Hc, nullptr, 0, w.qkv + Hc, 3 * Hc, RT, 2 * Hc, Hc, EPI_BIAS_BF16, 2.0);
    for (const Seg& g : segs) {
      RR_RUN(m, st, RR_K_TAIL, 0.0, 12.0 * g.n * Hc,
             rr_launch_gather_rows(w.h16 + g.rt0 * Hc, x16 + g.p0 * Hc, g.n, 1, g.T, Hc * 2, 0, 1, 0, st));
      RR_RUN(m, st, RR_K_TAIL, 0.0, 12.0 * g.n * Hc,
             rr_launch_gather_rows(w.h32 + g.rt0 * Hc, x32 + g.p0 * Hc, g.n, 1, g.T, Hc * 4, 0, 1, 0, st));
    }
    RR_GEMM(m, st, x16, Hc, L.wqkv, L.bqkv, nullptr, 0, q16, Hc, n, Hc, Hc, EPI_BIAS_BF16, 2.0);
    for (const Seg& g : segs) {
      const bf16_t* kv = w.qkv + g.rt0 * 3 * Hc;
      RR_RUN(m, st, RR_K_ATTENTION, 4.0 * g.n * (double)g.T * Hc, 2.0 * 2.0 * g.n * g.T * Hc,
             rr_launch_attention(q16 + g.p0 * Hc, Hc, 1, 0, kv + Hc, kv + 2 * Hc, 3 * Hc, w.ce_bias + g.rt0, g.n, heads, 1, g.T,
                                 ctx16 + g.p0 * Hc, Hc, m->dt, st, nullptr, 0, (((long)n * heads + 7) / 8) * 8,   // (the one-segment call's schedule)
                                 opt_of(m, RR_OPT_ATTN_FIXED_REF)));
    }
    RR_GEMM(m, st, ctx16, Hc, L.wo, L.bo, x32, Hc, pre_a, Hc, n, Hc, Hc, EPI_BIAS_RESID_F32, 4.0);
    RR_RUN(m, st, RR_K_LAYERNORM, 0.0, 10.0 * n * Hc, rr_launch_layernorm(pre_a, L.ln1g, L.ln1b, c.ln_eps, n, Hc, a32, a16, m->dt, st));
    RR_GEMM(m, st, a16, Hc, L.w1, L.b1, nullptr, 0, mid16, Ic, n, Ic, Hc, EPI_BIAS_GELU_BF16, 2.0);
    RR_GEMM(m, st, mid16, Ic, L.w2, L.b2, a32, Hc, pre_b, Hc, n, Hc, Ic, EPI_BIAS_RESID_F32, 4.0);
    RR_RUN(m, st, RR_K_LAYERNORM, 0.0, 10.0 * n * Hc, rr_launch_layernorm(pre_b, L.ln2g, L.ln2b, c.ln_eps, n, Hc, out32, out16, m->dt, st));
    m->cls_rows = out32;
    m->tap_ce = nullptr;
    m->tap_ce_elems = 0;
    return RR_OK;
  }
  {
    ResidSrc rs{w.h32, nullptr, nullptr, nullptr};
    int folded = OP_NORMALISED;
    for (int l = 0; l < c.ce_layers; ++l)
      RR_TRY(run_layer(m, st, m->ce_layers[l], n, plan.sched_T, Hc, c.ce_heads, Ic, c.ln_eps, w.ce_bias, w, rs, folded,
                       l == c.ce_layers - 1, true,          // the CLS heads read the fp32 rows of the last layer
                       adj, adj_ld,                         // attention fusion: the same bias in every layer
                       plan.ce_segs ? &view : nullptr));
  }
  m->tap_ce = w.h32;
  m->tap_ce_elems = (size_t)RT * Hc;
  return RR_OK;
}

// Workspace of the interaction rerankers: n local pairs, Lq query tokens, Lc context tokens.
size_t layout_interaction(const rr_config& c, int n, int Bq, int Lq, int Lc, char* base, Work* w) {
  Bump b(base);
  const size_t T = (size_t)Lq + Lc, RT = (size_t)n * T, Hc = c.ce_hidden, Ic = c.ce_intermediate, D = c.li_dim;
  w->h32 = b.take<float>(RT * Hc);
  w->pre = b.take<float>(RT * Hc);
  w->pre2 = b.take<float>(RT * Hc);
  w->stats_a = b.take<float>(RT * 2);
  w->stats_b = b.take<float>(RT * 2);
  w->lnpart = b.take<float>(RT * 2 * ((Hc + 127) / 128));
  w->rowscale = b.take<float>(RT);
  w->h16 = b.take<bf16_t>(RT * Hc);
  w->qkv = b.take<bf16_t>(RT * 3 * Hc);
  w->ctx = b.take<bf16_t>(RT * Hc);
  w->mid = b.take<bf16_t>(RT * Ic);
  w->li16 = b.take<bf16_t>(RT * D);
  w->ce_bias = b.take<float>(RT);
  w->text_bias = b.take<float>((size_t)n * Lq);   // MORES: query-side self-attention bias
  w->li32 = b.take<float>((size_t)n * Lc);        // MORES: context-side cross-attention bias
  w->l1 = b.take<float>(n);
  w->l2 = b.take<float>(n);
  w->part_l = b.take<float>(Bq);
  w->part_w = b.take<float>(Bq);
  w->cls_scratch = b.take<char>(cls_scratch_bytes(c, n));   // (an interaction reranker with ONE cross-encoder layer takes the CLS-only path too)
  if (c.model_kind == RR_MODEL_MORES) {
    w->a32 = b.take<float>((size_t)n * Lq * Hc);
    w->a16 = b.take<bf16_t>((size_t)n * Lq * Hc);
    w->q_c = b.take<bf16_t>((size_t)n * Lq * Hc);
    w->enc16 = b.take<bf16_t>((size_t)n * Lc * Hc);       // doc = Linear(context_late_interaction)
    w->kv_c = b.take<bf16_t>((size_t)n * Lc * 2 * Hc);
    w->t32 = b.take<float>((size_t)Bq * Lq * Hc);          // Linear(query_late_interaction), per query
  }
  return (b.off + 255) & ~(size_t)255;
}

}  // namespace

extern "C" {

const char* rr_version(void) { return "librerank_mi355 0.2.0 (gfx950, abi 2)"; }

const char* rr_status_string(int s) {
  switch (s) {
    case RR_OK: return "ok";
    case RR_ERR_BAD_ARG: return "bad argument";
    case RR_ERR_BAD_SHAPE: return "bad shape";
    case RR_ERR_BAD_DTYPE: return "bad dtype";
    case RR_ERR_UNSUPPORTED: return "unsupported configuration";
    case RR_ERR_HIP: return "HIP runtime error";
    case RR_ERR_OOM: return "out of device memory";
    case RR_ERR_MISSING_WEIGHT: return "missing weight";
    case RR_ERR_NO_DEVICE: return "no gfx950 device";
    case RR_ERR_RANGE: return "fp16 activation range exceeded in an earlier forward";
    default: return "unknown status";
  }
}

static thread_local std::string g_create_err;

static int rr_create_impl(const rr_config* cfg, rr_handle* out) {
  if (!cfg || !out) return RR_ERR_BAD_ARG;
  *out = nullptr;
  if (cfg->abi_version != RR_ABI_VERSION) { g_create_err = "abi_version mismatch"; return RR_ERR_BAD_ARG; }
  auto bad = [&](const char* why) { g_create_err = why; return RR_ERR_UNSUPPORTED; };
  const rr_config& c = *cfg;
  if (c.hidden <= 0 || c.heads <= 0 || c.hidden != c.heads * 64) return bad("text encoder head dim must be 64");
  if (c.ce_hidden <= 0 || c.ce_heads <= 0 || c.ce_hidden != c.ce_heads * 64) return bad("cross encoder head dim must be 64");
  if (c.hidden % 64 || c.intermediate % 64 || c.ce_hidden % 64 || c.ce_intermediate % 64 || c.li_dim % 64)
    return bad("hidden/intermediate/li_dim must be multiples of 64");
  if (c.hidden > 2048 || c.ce_hidden > 2048 || c.li_dim > 2048) return bad("row length above 2048 not supported");
  if (c.layers < 0 || c.ce_layers < 0 || c.vocab_size <= 0 || c.max_pos <= 0 || c.ce_max_pos <= 0 || c.type_vocab <= 0)
    return bad("bad layer/vocab/position counts");
  if (c.loss_kind < 0 || c.loss_kind > 2) return bad("unknown loss_kind");
  if (c.has_vision) {
    if (c.vision_hidden % 64 || c.prefix_len <= 0 || c.n_patches <= 0 || c.map_layers < 0 || c.cross_attn_len <= 0 ||
        (c.li_dim * c.prefix_len / 2) % 64)
      return bad("bad vision configuration");
  }
  if (c.vit_layers < 0) return bad("vit_layers < 0");
  if (c.vit_layers > 0) {
    if (c.model_kind != RR_MODEL_FULL_CONTEXT || !c.has_vision) return bad("the CLIP ViT needs a full-context model with has_vision");
    if (c.vit_heads <= 0 || c.vision_hidden != c.vit_heads * 64) return bad("CLIP ViT head dim must be 64");
    if (c.vit_intermediate <= 0 || c.vit_intermediate % 64 || c.vision_hidden > 2048) return bad("bad CLIP ViT widths");
    if (c.vit_patch_size <= 0 || c.vit_image_size <= 0 || c.vit_image_size % c.vit_patch_size)
      return bad("vit_image_size must be a multiple of vit_patch_size");
    const int g = c.vit_image_size / c.vit_patch_size;
    if (g * g != c.n_patches) return bad("n_patches must equal (vit_image_size / vit_patch_size)^2");
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || c.device < 0 || c.device >= ndev) {
    g_create_err = "no HIP device visible (librerank_mi355 has no CPU path)";
    return RR_ERR_NO_DEVICE;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, c.device) != hipSuccess) return RR_ERR_HIP;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    g_create_err = std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only";
    return RR_ERR_NO_DEVICE;
  }
  if (hipSetDevice(c.device) != hipSuccess) return RR_ERR_HIP;
  if (c.compute_dtype != 0 && c.compute_dtype != 1) return bad("compute_dtype must be 0 (bf16) or 1 (fp16)");
  if (c.fp8 != 0 && c.fp8 != 1) return bad("fp8 must be 0 or 1");
  if (c.fp8 && ((c.hidden % 128) || (c.ce_hidden % 128))) return bad("fp8 mode needs hidden sizes that are multiples of 128");
  if (c.model_kind < 0 || c.model_kind > 2) return bad("model_kind must be 0 (full context), 1 (interaction) or 2 (MORES)");
  rr_model* m = new rr_model();
  m->cfg = c;
  m->dt = c.compute_dtype;
  build_required(m);
  *out = m;
  return RR_OK;
}

const char* rr_last_error(rr_handle h) { return h ? h->err.c_str() : g_create_err.c_str(); }

static int rr_destroy_impl(rr_handle h) {
  if (!h) return RR_ERR_BAD_ARG;
  (void)hipSetDevice(h->cfg.device);
  (void)hipDeviceSynchronize();
  for (void* p : h->dev_allocs) (void)hipFree(p);
  for (void* p : h->retired) (void)hipFree(p);
  if (h->range_flag_host) (void)hipHostFree(h->range_flag_host);
  if (h->ws) (void)hipFree(h->ws);
  if (h->tap_text) (void)hipFree(h->tap_text);
  if (h->adj) (void)hipFree(h->adj);
  if (h->li_sc) (void)hipFree(h->li_sc);
  if (h->bank_blk) (void)hipFree(h->bank_blk);
  if (h->search_blk) (void)hipFree(h->search_blk);
  if (h->train_blk) (void)hipFree(h->train_blk);
  for (auto& e : h->ev_pool) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  for (auto& a : h->asm_slot) {
    if (a.host) (void)hipHostFree(a.host);
    if (a.dev) (void)hipFree(a.dev);
    if (a.done) (void)hipEventDestroy(a.done);
  }
  delete h;
  return RR_OK;
}

int rr_num_required_weights(rr_handle h) { return h ? (int)h->required_order.size() : RR_ERR_BAD_ARG; }
const char* rr_required_weight_name(rr_handle h, int i) {
  if (!h || i < 0 || i >= (int)h->required_order.size()) return nullptr;
  return h->required_order[i].c_str();
}

static int rr_load_weight_impl(rr_handle h, const char* name, const void* data, int dtype, int ndim, const int64_t* shape,
                   int* known) {
  if (!h || !name || !data || ndim < 0 || (ndim > 0 && !shape)) return fail(h, RR_ERR_BAD_ARG, "rr_load_weight: null argument");
  if (h->finalized) return fail(h, RR_ERR_BAD_ARG, "rr_load_weight after rr_finalize_weights");
  auto it = h->required.find(name);
  if (known) *known = it != h->required.end();
  if (it == h->required.end()) return RR_OK;   // strict=False semantics: ignore tensors the path does not read
  if (dtype != RR_F32 && dtype != RR_BF16 && dtype != RR_F16) return fail(h, RR_ERR_BAD_DTYPE, "%s: dtype %d", name, dtype);
  const auto& want = it->second;
  bool ok = (int)want.size() == ndim;
  size_t n = 1;
  for (int i = 0; ok && i < ndim; ++i) { ok = want[i] == shape[i]; n *= (size_t)shape[i]; }
  if (!ok) {
    std::string ws, gs;
    for (auto d : want) ws += std::to_string(d) + ",";
    for (int i = 0; i < ndim; ++i) gs += std::to_string(shape[i]) + ",";
    return fail(h, RR_ERR_BAD_SHAPE, "%s: expected shape [%s] got [%s]", name, ws.c_str(), gs.c_str());
  }
  HostTensor t;
  t.shape = want;
  t.data.resize(n);
  if (dtype == RR_F32) memcpy(t.data.data(), data, n * 4);
  else if (dtype == RR_BF16) for (size_t i = 0; i < n; ++i) t.data[i] = host_bf2f(((const uint16_t*)data)[i]);
  else for (size_t i = 0; i < n; ++i) t.data[i] = host_h2f(((const uint16_t*)data)[i]);
  h->host[name] = std::move(t);
  return RR_OK;
}

static int rr_finalize_weights_impl(rr_handle h) {
  if (!h) return RR_ERR_BAD_ARG;
  if (h->finalized) return RR_OK;
  for (const auto& n : h->required_order)
    if (!h->host.count(n)) return fail(h, RR_ERR_MISSING_WEIGHT, "missing weight: %s", n.c_str());
  rr_model* m = h;
  const rr_config& c = m->cfg;
  RR_HIP(m, hipSetDevice(c.device));       // before ANY allocation: the engine's device need not be the current one
  if (!m->range_flag) {
    RR_TRY(dev_alloc(m, (void**)&m->range_flag, sizeof(int)));
    RR_HIP(m, hipMemset(m->range_flag, 0, sizeof(int)));
    RR_HIP(m, hipHostMalloc((void**)&m->range_flag_host, sizeof(int), hipHostMallocDefault));
    *m->range_flag_host = 0;
  }
  {
    const int q8 = opt_of(m, RR_OPT_Q8_FORMAT);
    if (c.fp8 && q8 == 1 && opt_of(m, RR_OPT_FP8_FFN_DOWN) == 1)
      return fail(m, RR_ERR_BAD_ARG, "fp8_ffn_down = 1 needs q8_format 0 (there is no int8 FFN-down)");
    m->q8_fmt = q8;                       // latched: the 8-bit weights below are packed in this one format
  }
  if (c.model_kind != RR_MODEL_FULL_CONTEXT) {
    RR_TRY(up_bf16(m, HT(m, "cross_encoder_input_mapping.weight"), &m->w_cemap));
    RR_TRY(up_f32(m, HT(m, "cross_encoder_input_mapping.bias"), &m->b_cemap));
    m->ce_layers.resize(c.ce_layers);
    if (c.model_kind == RR_MODEL_INTERACTION) {
      const std::string q = "reranker.bert_model";
      RR_TRY(up_f32(m, HT(m, q + ".embeddings.position_embeddings.weight"), &m->ce_pos));
      RR_TRY(up_f32(m, HT(m, q + ".embeddings.token_type_embeddings.weight"), &m->ce_type));
      RR_TRY(up_f32(m, HT(m, q + ".embeddings.LayerNorm.weight"), &m->ce_emb_g));
      RR_TRY(up_f32(m, HT(m, q + ".embeddings.LayerNorm.bias"), &m->ce_emb_b));
      for (int i = 0; i < c.ce_layers; ++i)
        RR_TRY(pack_layer(m, q + ".encoder.layer." + std::to_string(i), c.ce_heads, c.ce_hidden, false, &m->ce_layers[i],
                          i ? q + ".encoder.layer." + std::to_string(i - 1) + ".output.LayerNorm" : std::string()));
    } else {
      for (int i = 0; i < c.ce_layers; ++i)
        RR_TRY(pack_layer(m, "reranker.interaction_module." + std::to_string(i), c.ce_heads, c.ce_hidden, true,
                          &m->ce_layers[i]));
    }
    RR_TRY(up_f32(m, HT(m, "reranker.classifier1.weight"), &m->cls1_w));
    RR_TRY(up_f32(m, HT(m, "reranker.classifier1.bias"), &m->cls1_b));
    RR_TRY(up_f32(m, HT(m, "reranker.classifier2.weight"), &m->cls2_w));
    RR_TRY(up_f32(m, HT(m, "reranker.classifier2.bias"), &m->cls2_b));
    m->host.clear();
    m->finalized = true;
    return RR_OK;
  }
  std::string p = "context_text_encoder.bert_model";
  RR_TRY(up_f32(m, HT(m, p + ".embeddings.word_embeddings.weight"), &m->word));
  RR_TRY(up_f32(m, HT(m, p + ".embeddings.position_embeddings.weight"), &m->pos));
  RR_TRY(up_f32(m, HT(m, p + ".embeddings.token_type_embeddings.weight"), &m->type));
  RR_TRY(up_f32(m, HT(m, p + ".embeddings.LayerNorm.weight"), &m->emb_g));
  RR_TRY(up_f32(m, HT(m, p + ".embeddings.LayerNorm.bias"), &m->emb_b));
  m->text_layers.resize(c.layers);
  for (int i = 0; i < c.layers; ++i)
    RR_TRY(pack_layer(m, p + ".encoder.layer." + std::to_string(i), c.heads, c.hidden, false, &m->text_layers[i],
                      i ? p + ".encoder.layer." + std::to_string(i - 1) + ".output.LayerNorm" : std::string()));
  RR_TRY(up_bf16(m, HT(m, "context_text_encoder_linear.weight"), &m->w_li));
  if (c.has_vision) {
    RR_TRY(up_bf16(m, HT(m, "context_vision_projection.model.0.weight"), &m->w_vp0));
    RR_TRY(up_f32(m, HT(m, "context_vision_projection.model.0.bias"), &m->b_vp0));
    RR_TRY(up_bf16(m, HT(m, "context_vision_projection.model.2.weight"), &m->w_vp2));
    RR_TRY(up_f32(m, HT(m, "context_vision_projection.model.2.bias"), &m->b_vp2));
    RR_TRY(up_bf16(m, HT(m, "transformer_mapping_input_linear.weight"), &m->w_min));
    RR_TRY(up_f32(m, HT(m, "transformer_mapping_input_linear.bias"), &m->b_min));
    m->map_layers.resize(c.map_layers);
    for (int i = 0; i < c.map_layers; ++i)
      RR_TRY(pack_layer(m, "transformer_mapping_network.layer." + std::to_string(i), c.heads, c.hidden, true,
                        &m->map_layers[i]));
    RR_TRY(up_bf16(m, HT(m, "transformer_mapping_output_linear.weight"), &m->w_mout));
    RR_TRY(up_f32(m, HT(m, "transformer_mapping_output_linear.bias"), &m->b_mout));
  }
  if (c.vit_layers > 0) RR_TRY(pack_vit(m));
  RR_TRY(up_bf16(m, HT(m, "cross_encoder_input_mapping.weight"), &m->w_cemap));
  RR_TRY(up_f32(m, HT(m, "cross_encoder_input_mapping.bias"), &m->b_cemap));
  p = "reranker.bert_model";
  RR_TRY(up_f32(m, HT(m, p + ".embeddings.position_embeddings.weight"), &m->ce_pos));
  RR_TRY(up_f32(m, HT(m, p + ".embeddings.token_type_embeddings.weight"), &m->ce_type));
  RR_TRY(up_f32(m, HT(m, p + ".embeddings.LayerNorm.weight"), &m->ce_emb_g));
  RR_TRY(up_f32(m, HT(m, p + ".embeddings.LayerNorm.bias"), &m->ce_emb_b));
  m->ce_layers.resize(c.ce_layers);
  for (int i = 0; i < c.ce_layers; ++i)
    RR_TRY(pack_layer(m, p + ".encoder.layer." + std::to_string(i), c.ce_heads, c.ce_hidden, false, &m->ce_layers[i],
                      i ? p + ".encoder.layer." + std::to_string(i - 1) + ".output.LayerNorm" : std::string()));
  RR_TRY(up_f32(m, HT(m, "reranker.classifier1.weight"), &m->cls1_w));
  RR_TRY(up_f32(m, HT(m, "reranker.classifier1.bias"), &m->cls1_b));
  RR_TRY(up_f32(m, HT(m, "reranker.classifier2.weight"), &m->cls2_w));
  RR_TRY(up_f32(m, HT(m, "reranker.classifier2.bias"), &m->cls2_b));
  m->host.clear();
  m->finalized = true;
  return RR_OK;
}

static int64_t rr_workspace_bytes_impl(rr_handle h, int n_pairs, int seq_len) {
  if (!h || n_pairs <= 0 || seq_len <= 0) return RR_ERR_BAD_ARG;
  Work w;
  return (int64_t)layout(h->cfg, n_pairs, n_pairs, seq_len, h->cfg.has_vision != 0, nullptr, &w);
}

/* rr_reserve: allocate, once and outside the forward, everything a forward over at most n_pairs pairs of n_queries
 * queries would otherwise grow on first use: the workspace, the attention redo flags of `hip_stream`, and (with_fusion)
 * the attention-fusion bias.  len_a = seq_len (full-context models) or Lq (interaction), len_b = Lc (interaction only). */
static int rr_reserve_impl(rr_handle h, int n_pairs, int n_queries, int len_a, int len_b, int with_fusion, void* hip_stream) {
  if (!h) return RR_ERR_BAD_ARG;
  rr_model* m = h;
  const rr_config& c = m->cfg;
  if (n_pairs <= 0 || n_queries <= 0 || len_a <= 0) return fail(m, RR_ERR_BAD_SHAPE, "rr_reserve: n_pairs=%d n_queries=%d len=%d", n_pairs, n_queries, len_a);
  hipStream_t st = (hipStream_t)hip_stream;
  RR_TRY(check_rows(m, "rr_reserve", n_pairs,
                    c.model_kind == RR_MODEL_FULL_CONTEXT ? len_a + (c.has_vision ? c.prefix_len + c.n_patches : 0) : len_a + (len_b > 0 ? len_b : 0)));
  RR_HIP(m, hipSetDevice(c.device));
  Work w{};
  size_t need;
  int T;
  if (c.model_kind == RR_MODEL_FULL_CONTEXT) {
    need = layout(c, n_pairs, n_queries, len_a, c.has_vision != 0, nullptr, &w);
    T = len_a + (c.has_vision ? c.prefix_len + c.n_patches : 0);
    RR_HIP(m, rr_attention_reserve(n_pairs, c.heads, len_a, st));
  } else {
    if (len_b <= 0) return fail(m, RR_ERR_BAD_SHAPE, "rr_reserve: interaction models need len_b = Lc");
    need = layout_interaction(c, n_pairs, n_queries, len_a, len_b, nullptr, &w);
    T = len_a + len_b;
  }
  RR_HIP(m, rr_attention_reserve(n_pairs, c.ce_heads, T, st));
  RR_TRY(ensure_ws(m, need, st));
  if (with_fusion) RR_TRY(ensure_block(m, m->adj, m->adj_cap, (size_t)n_pairs * T * ((T + 63) / 64 * 64) * sizeof(float), st, "the attention-fusion bias buffer"));
  if (with_fusion == 2 && c.model_kind == RR_MODEL_INTERACTION)      // the score block of rr_forward_interaction*_fusion_li
    RR_TRY(ensure_block(m, m->li_sc, m->li_sc_cap, (size_t)n_pairs * len_b * len_a * sizeof(float), st, "the late-interaction score block"));
  return RR_OK;
}

static int rr_encode_image_impl(rr_handle h, const float* pixel_values, int B, float* image_cls_out, float* image_patches_out,
                    void* hip_stream) {
  if (!h || !pixel_values || !image_cls_out || !image_patches_out) return fail(h, RR_ERR_BAD_ARG, "rr_encode_image: null argument");
  rr_model* m = h;
  const rr_config& c = m->cfg;
  if (c.vit_layers <= 0) return fail(m, RR_ERR_UNSUPPORTED, "rr_encode_image: the handle was created without a CLIP ViT (vit_layers = 0)");
  if (!m->finalized) return fail(m, RR_ERR_BAD_ARG, "rr_encode_image before rr_finalize_weights");
  if (B <= 0) return fail(m, RR_ERR_BAD_SHAPE, "rr_encode_image: B=%d", B);
  hipStream_t st = (hipStream_t)hip_stream;
  RR_HIP(m, hipSetDevice(c.device));
  const int Vh = c.vision_hidden, Iv = c.vit_intermediate, np = c.n_patches, T = np + 1, R = B * T, Kp = m->vit_kp;
  const float eps = 1e-5f;   // CLIPVisionConfig.layer_norm_eps
  VitWork w;
  const size_t need = layout_vit(c, Kp, B, nullptr, &w);
  RR_TRY(ensure_ws(m, need, st));
  layout_vit(c, Kp, B, m->ws, &w);
  m->last_stream = st;

  RR_RUN(m, st, RR_K_EMBED, 0.0, 4.0 * B * 3 * c.vit_image_size * c.vit_image_size + 2.0 * B * np * Kp,
         rr_launch_vit_im2col(pixel_values, w.cols, B, c.vit_image_size, c.vit_patch_size, Kp, m->dt, st));
  RR_GEMM(m, st, w.cols, Kp, m->vit_wpatch, nullptr, nullptr, 0, w.patch32, Vh, B * np, Vh, Kp, EPI_BIAS_F32, 4.0);
  RR_RUN(m, st, RR_K_EMBED, 0.0, 8.0 * R * Vh,
         rr_launch_vit_embed_ln(w.patch32, m->vit_cls, m->vit_pos, m->vit_pre_g, m->vit_pre_b, eps, R, T, Vh, w.xa, st));
  float *x = w.xa, *y = w.xb;   // fp32 residual stream (pre-LN blocks: the stream itself is never normalised)
  auto emit_patches = [&](const float* src) {
    return hipMemcpy2DAsync(image_patches_out, (size_t)np * Vh * 4, src + Vh, (size_t)T * Vh * 4, (size_t)np * Vh * 4, B,
                            hipMemcpyDeviceToDevice, st);
  };
  for (int l = 0; l < c.vit_layers; ++l) {
    const LayerW& L = m->vit_layers[l];
    if (l == c.vit_layers - 1) RR_RUN(m, st, RR_K_TAIL, 0.0, 8.0 * B * np * Vh, emit_patches(x));   // hidden_states[-2]
    RR_RUN(m, st, RR_K_LAYERNORM, 0.0, 6.0 * R * Vh, rr_launch_layernorm(x, L.ln1g, L.ln1b, eps, R, Vh, nullptr, w.n16, m->dt, st));
    RR_GEMM(m, st, w.n16, Vh, L.wqkv, L.bqkv, nullptr, 0, w.qkv, 3 * Vh, R, 3 * Vh, Vh, EPI_BIAS_BF16, 2.0);
    RR_RUN(m, st, RR_K_ATTENTION, 4.0 * B * (double)T * T * Vh, 2.0 * 4.0 * R * Vh,
           rr_launch_attention(w.qkv, 3 * Vh, 1, 0, w.qkv + Vh, w.qkv + 2 * Vh, 3 * Vh, nullptr, B, c.vit_heads, T, T,
                               w.ctx, Vh, m->dt, st, nullptr, 0, 0, opt_of(m, RR_OPT_ATTN_FIXED_REF)));
    RR_GEMM(m, st, w.ctx, Vh, L.wo, L.bo, x, Vh, y, Vh, R, Vh, Vh, EPI_BIAS_RESID_F32, 4.0);
    RR_RUN(m, st, RR_K_LAYERNORM, 0.0, 6.0 * R * Vh, rr_launch_layernorm(y, L.ln2g, L.ln2b, eps, R, Vh, nullptr, w.n16, m->dt, st));
    RR_GEMM(m, st, w.n16, Vh, L.w1, L.b1, nullptr, 0, w.mid, Iv, R, Iv, Vh, EPI_BIAS_QGELU_BF16, 2.0);
    RR_GEMM(m, st, w.mid, Iv, L.w2, L.b2, y, Vh, x, Vh, R, Vh, Iv, EPI_BIAS_RESID_F32, 4.0);
  }
  RR_RUN(m, st, RR_K_TAIL, 0.0, 8.0 * B * Vh,
         hipMemcpy2DAsync(image_cls_out, (size_t)Vh * 4, x, (size_t)T * Vh * 4, (size_t)Vh * 4, B, hipMemcpyDeviceToDevice, st));
  return RR_OK;
}

// rr_head / rr_head_joint: the scoring head on gathered logits (joint: with RerankModel.forward's loss, as rr_forward_joint
// runs it)
static int head_call(rr_handle h, const char* what, bool joint, const float* logits, const float* logits2, const float* labels,
                     int Bq, int K, float* loss_out, float* scores_out, int32_t* order_out, void* hip_stream) {
  if (!h || !logits) return fail(h, RR_ERR_BAD_ARG, "%s: null argument", what);
  if (Bq <= 0 || K <= 0) return fail(h, RR_ERR_BAD_SHAPE, "%s: Bq=%d K=%d", what, Bq, K);
  const rr_config& c = h->cfg;
  if (joint && c.model_kind != RR_MODEL_FULL_CONTEXT) return fail(h, RR_ERR_BAD_ARG, "rr_head_joint on an interaction model");
  RR_TRY(check_head(h, what, Bq, K, 0, (long long)Bq * K, labels, logits2, loss_out, scores_out, order_out, joint));
  hipStream_t st = (hipStream_t)hip_stream;
  RR_HIP(h, hipSetDevice(c.device));
  Work w;
  const size_t need = layout(c, 1, Bq, 8, false, nullptr, &w);
  RR_TRY(ensure_ws(h, need, st));
  layout(c, 1, Bq, 8, false, h->ws, &w);
  return launch_head(h, st, w, logits, logits2, labels, Bq, K, joint, loss_out, scores_out, order_out);
}

// rr_head_lists (include/rerank_mi355.h): the scoring head over lists of unequal length.  Every check on the host first; then
// the offsets go up through the staging slots of rr_assemble_pairs, with the per-list partials behind them in the same block:
// [offsets: n_lists + 1 | part_loss: n_lists | part_w: n_lists], so nothing here is sized by a query count of the workspace.
// Sharing the two slots means that this call waits, on the host, for the launch that read its slot two staged calls ago: in
// the pipelined loop (assemble, head, assemble, head, ...) that is the previous batch's head, i.e. the host runs at most one
// batch ahead of the device, which is what that loop does anyway (profiles/strings_to_records_lists_ragged.json.log).
static int head_lists_call(rr_handle h, const float* logits, const float* logits2, const float* labels, int n_lists,
                           const int32_t* off, const int32_t* gather, int joint, float* loss_out, float* list_loss_out,
                           float* scores_out, int32_t* order_out, void* hip_stream) {
  const char* what = "rr_head_lists";
  if (!h) return RR_ERR_BAD_ARG;
  if (!logits || !off) return fail(h, RR_ERR_BAD_ARG, "%s: null argument", what);
  if (n_lists <= 0 || n_lists > (1 << 24)) return fail(h, RR_ERR_BAD_SHAPE, "%s: %d lists", what, n_lists);
  if (off[0] != 0) return fail(h, RR_ERR_BAD_SHAPE, "%s: list_offsets[0] = %d, not 0", what, off[0]);
  int longest = 0;
  for (int q = 0; q < n_lists; ++q) {
    if (off[q + 1] <= off[q])
      return fail(h, RR_ERR_BAD_SHAPE, "%s: list %d is empty or descending (offsets %d, %d)", what, q, off[q], off[q + 1]);
    longest = std::max(longest, off[q + 1] - off[q]);
  }
  const rr_config& c = h->cfg;
  if (joint && c.model_kind != RR_MODEL_FULL_CONTEXT) return fail(h, RR_ERR_BAD_ARG, "%s: joint = 1 on an interaction model", what);
  const float* loss_any = loss_out ? loss_out : list_loss_out;
  RR_TRY(check_head(h, what, 1, longest, 0, longest, labels, logits2, loss_any, scores_out, order_out, joint != 0));
  const int N = off[n_lists];
  hipStream_t st = (hipStream_t)hip_stream;
  std::vector<int32_t> staged((size_t)3 * n_lists + 1, 0);
  std::copy(off, off + n_lists + 1, staged.begin());
  void* dev = nullptr;
  RR_TRY(asm_stage(h, what, staged.data(), staged.size() * sizeof(int32_t), st, &dev));
  const int32_t* off_d = (const int32_t*)dev;
  float* part_l = (float*)(off_d + n_lists + 1);
  float* part_w = part_l + n_lists;
  const bool two = c.loss_kind == RR_LOSS_2H_BCE;
  const int has_pw = !std::isnan(c.pos_weight);
  RR_RUN(h, st, RR_K_HEAD, 0.0, 12.0 * N,
         rr_launch_head_lists(logits, two ? logits2 : nullptr, joint ? nullptr : labels, joint != 0, off_d, gather, n_lists, N,
                              (joint && two) ? 3 : c.loss_kind, has_pw ? c.pos_weight : 1.0f, has_pw, scores_out, order_out,
                              loss_out, list_loss_out, part_l, part_w, st));
  return asm_done(h, st);
}

// Sticky range error (include/rerank_mi355.h, rr_activation_range_flag): look at what the PREVIOUS forwards left in the pinned
// word (no synchronisation: a copy still in flight simply reports one call later), refuse to go on once it is raised.
static int range_guard_enter(rr_model* m) {
  if (m->range_flag_host && *(volatile int*)m->range_flag_host) {
    if (m->dt == 1)
      return fail(m, RR_ERR_RANGE, "an earlier forward's pre-LayerNorm rows left the fp16 range (flag %d): its logits are unreliable; "
                                   "clear with rr_activation_range_flag(reset = 1) and use compute_dtype = bf16 for this checkpoint",
                  *(volatile int*)m->range_flag_host);
    return fail(m, RR_ERR_RANGE, "an earlier forward's pre-LayerNorm rows were not finite (flag %d; bf16 rows have fp32's range, so "
                                 "this is inf / NaN in the inputs or weights): clear with rr_activation_range_flag(reset = 1)",
                *(volatile int*)m->range_flag_host);
  }
  return RR_OK;
}
static int range_guard_exit(rr_model* m, hipStream_t st) {
  if (m->range_flag && m->range_flag_host)
    RR_HIP(m, hipMemcpyAsync(m->range_flag_host, m->range_flag, sizeof(int), hipMemcpyDeviceToHost, st));
  return RR_OK;
}

// Attention-fusion bias of a forward into m->adj from scores over the Tq + Tc tokens of every pair.  Padded call: scores
// [N][Tc + s_off][Tq], context rows from row0 on, of pairs pair_begin.., bias [n][T][*adj_ld = round_up(T, 64)]
// (rr_launch_fusion_adj).  Packed call: scores [n][Tc][Tq] (the context rows, packed pair order, padded context axis), segment
// g's pairs end after g.S - s_off context tokens (joint: g.S - q_len; interaction: g.S), so its rows are g.T = Tq + that; one
// launch, layout per segment as run_layer reads it: [g.n][g.T][round_up(g.T, 64)] (rr_launch_fusion_adj_segs, *adj_ld = 0).
static int fusion_bias(rr_model* m, hipStream_t st, const RowPlan& plan, const float* scores, int Tq, int Tc, int s_off, int row0,
                       float mult, int pair_begin, int* adj_ld) {
  if (!plan.packed) {
    const int T = Tq + Tc, rows = Tc + s_off, n = plan.n;
    *adj_ld = (T + 63) / 64 * 64;
    const size_t need = (size_t)n * T * *adj_ld * sizeof(float);
    RR_TRY(ensure_block(m, m->adj, m->adj_cap, need, st, "the attention-fusion bias buffer"));
    RR_RUN(m, st, RR_K_TAIL, 0.0, 4.0 * n * (double)rows * Tq + (double)need,
           rr_launch_fusion_adj(scores, rows, Tq, Tc, mult, pair_begin, n, m->adj, *adj_ld, st, row0));
    return RR_OK;
  }
  size_t need = 0;
  double rd = 0.0;
  std::vector<int> sn, tk;
  for (const Seg& g : plan.segs) {
    if (g.T != Tq + g.S - s_off) return fail(m, RR_ERR_BAD_ARG, "internal: fusion bias rows %d != %d + %d", g.T, Tq, g.S - s_off);
    need += (size_t)g.n * g.T * ((g.T + 63) / 64 * 64) * sizeof(float);
    rd += 4.0 * g.n * (double)Tc * Tq;
    sn.push_back(g.n);
    tk.push_back(g.S - s_off);
  }
  *adj_ld = 0;
  RR_TRY(ensure_block(m, m->adj, m->adj_cap, need, st, "the attention-fusion bias buffer"));
  RR_RUN(m, st, RR_K_TAIL, 0.0, rd + (double)need,
         rr_launch_fusion_adj_segs(scores, Tc, Tq, Tc, mult, (int)plan.segs.size(), sn.data(), tk.data(), m->adj, st, 0));
  return RR_OK;
}

// Segment table of a packed call (rr_forward_*_packed, include/rerank_mi355.h): 1..64 non-empty segments of lengths in
// (min_len, r.len]; the call then covers all its pairs, one per query (Bq = pairs, K = 1).
static int packed_segments(rr_model* m, const char* what, Request& r, int min_len, int extra_rows,
                           std::vector<std::pair<int, int>>* out) {
  if (!r.seg_pairs || !r.seg_len) return fail(m, RR_ERR_BAD_ARG, "%s: null segment tables", what);
  if (r.n_segments <= 0 || r.n_segments > 64) return fail(m, RR_ERR_BAD_SHAPE, "%s: %d segments (1..64)", what, r.n_segments);
  long long pairs = 0, rows = 0;
  for (int i = 0; i < r.n_segments; ++i) {
    if (r.seg_pairs[i] <= 0 || r.seg_len[i] <= min_len || r.seg_len[i] > r.len)
      return fail(m, RR_ERR_BAD_SHAPE, "%s: segment %d holds %d pairs of length %d (lengths in (%d, %d])", what, i, r.seg_pairs[i],
                  r.seg_len[i], min_len, r.len);
    out->emplace_back(r.seg_pairs[i], r.seg_len[i]);
    pairs += r.seg_pairs[i];
    rows += (long long)r.seg_pairs[i] * (r.seg_len[i] + extra_rows);
  }
  if (pairs > (1 << 24) || rows > (1LL << 30)) return fail(m, RR_ERR_BAD_SHAPE, "%s: %lld pairs / %lld rows", what, pairs, rows);
  r.Bq = r.pair_end = (int)pairs;
  r.K = 1;
  r.pair_begin = 0;
  return RR_OK;
}

}  // extern "C"
// One staged upload: `bytes` of checked host descriptors into a staging slot (pinned host half, device half, at least min_cap
// bytes each), once the launch that last read that slot has completed (its event), and an async copy to the device half on `st`.
// The handle's slot pair (asm_stage) and a bank's (rr_bank_add) both go through here.
hipError_t stage_slot(rr_model::AsmSlot& a, const void* data, size_t bytes, size_t min_cap, hipStream_t st) {
  hipError_t e = a.done ? hipEventSynchronize(a.done) : hipEventCreateWithFlags(&a.done, hipEventDisableTiming);
  if (e != hipSuccess) return e;
  if (a.cap < bytes) {
    if (a.host) { if ((e = hipHostFree(a.host)) != hipSuccess) return e; a.host = nullptr; }
    if (a.dev) { if ((e = hipFree(a.dev)) != hipSuccess) return e; a.dev = nullptr; }
    a.cap = 0;
    const size_t cap = std::max(bytes, min_cap);
    if ((e = hipHostMalloc(&a.host, cap, hipHostMallocDefault)) != hipSuccess) return e;
    if ((e = hipMalloc(&a.dev, cap)) != hipSuccess) return e;
    a.cap = cap;
  }
  memcpy(a.host, data, bytes);
  return hipMemcpyAsync(a.dev, a.host, bytes, hipMemcpyHostToDevice, st);
}

// The descriptor upload of rr_assemble_pairs / rr_assemble_joint and of the bank calls of a handle: into the next of the handle's
// two slots.  asm_done records the slot's event behind the launch that reads it and hands the next call the other slot.
int asm_stage(rr_model* m, const char* what, const void* data, size_t bytes, hipStream_t st, void** dev) {
  RR_TRY(capture_guard(m, st, CAP_STAGES, what));
  RR_HIP(m, hipSetDevice(m->cfg.device));
  rr_model::AsmSlot& a = m->asm_slot[m->asm_next];
  RR_HIP(m, stage_slot(a, data, bytes, (size_t)1024 * sizeof(rr_asm_pair), st));
  *dev = a.dev;
  return RR_OK;
}

int asm_done(rr_model* m, hipStream_t st) {
  RR_HIP(m, hipEventRecord(m->asm_slot[m->asm_next].done, st));
  m->asm_next ^= 1;
  return RR_OK;
}

extern "C" {
// rr_assemble_pairs (include/rerank_mi355.h): every check on the host first, then one staged upload and one launch.
static int rr_assemble_pairs_impl(rr_handle h, const int32_t* pool, int64_t pool_len, const int32_t* desc, int n_pairs,
                                  const int32_t* order, int n_segments, const int32_t* seg_pairs, const int32_t* seg_len,
                                  int64_t cls_id, int64_t sep_id, int64_t pad_id, int64_t* input_ids, int64_t* attention_mask,
                                  int64_t* token_type_ids, void* hip_stream) {
  const char* what = "rr_assemble_pairs";
  if (!h) return RR_ERR_BAD_ARG;
  rr_model* m = h;
  if (!desc || !order || !seg_pairs || !seg_len || !input_ids || !attention_mask || (!pool && pool_len > 0))
    return fail(m, RR_ERR_BAD_ARG, "%s: null argument", what);
  if (pool_len < 0 || n_pairs <= 0 || n_segments <= 0 || n_segments > 64)
    return fail(m, RR_ERR_BAD_SHAPE, "%s: pool_len=%lld, %d pairs, %d segments (1..64)", what, (long long)pool_len, n_pairs,
                n_segments);
  long long pairs = 0, rows = 0;
  for (int s = 0; s < n_segments; ++s) {
    if (seg_pairs[s] <= 0 || seg_len[s] < 3)
      return fail(m, RR_ERR_BAD_SHAPE, "%s: segment %d holds %d pairs of length %d", what, s, seg_pairs[s], seg_len[s]);
    pairs += seg_pairs[s];
    rows += (long long)seg_pairs[s] * seg_len[s];
  }
  if (pairs != n_pairs || rows > INT32_MAX)
    return fail(m, RR_ERR_BAD_SHAPE, "%s: the segments hold %lld pairs (%lld rows), the call has %d", what, pairs, rows, n_pairs);
  std::vector<char> seen((size_t)n_pairs, 0);
  for (int i = 0; i < n_pairs; ++i) {
    const int32_t p = order[i];
    if (p < 0 || p >= n_pairs || seen[(size_t)p]) return fail(m, RR_ERR_BAD_SHAPE, "%s: order is not a permutation (entry %d = %d)", what, i, p);
    seen[(size_t)p] = 1;
  }
  std::vector<rr_asm_pair> staged((size_t)n_pairs);
  int i = 0;
  long long row0 = 0;
  for (int s = 0; s < n_segments; ++s)
    for (int k = 0; k < seg_pairs[s]; ++k, ++i, row0 += seg_len[s]) {
      const int32_t* d = desc + 4 * (size_t)order[i];
      if (d[0] < 0 || d[1] < 0 || d[2] < 0 || d[3] < 0 || (long long)d[0] + d[1] > pool_len || (long long)d[2] + d[3] > pool_len ||
          (long long)d[1] + d[3] + 3 > seg_len[s])
        return fail(m, RR_ERR_BAD_SHAPE, "%s: pair %d (query offset %d, la %d, context offset %d, lb %d) does not fit a pool of %lld "
                    "ids and its segment's length %d", what, order[i], d[0], d[1], d[2], d[3], (long long)pool_len, seg_len[s]);
      staged[(size_t)i] = rr_asm_pair{d[0], d[1], d[2], d[3], seg_len[s], (int32_t)row0, 0, 0};
    }
  hipStream_t st = (hipStream_t)hip_stream;
  void* dev = nullptr;
  RR_TRY(asm_stage(m, what, staged.data(), staged.size() * sizeof(rr_asm_pair), st, &dev));
  RR_RUN(m, st, RR_K_EMBED, 0.0, (double)rows * (token_type_ids ? 24.0 : 16.0) + 4.0 * (double)rows,
         rr_launch_assemble_pairs(pool, pool_len, (const rr_asm_pair*)dev, n_pairs, cls_id, sep_id, pad_id, input_ids, attention_mask,
                                  token_type_ids, st));
  return asm_done(m, st);
}

// rr_assemble_joint (include/rerank_mi355.h): the joint family's rows, checked and staged as rr_assemble_pairs does.
static int rr_assemble_joint_impl(rr_handle h, const int32_t* pool, int64_t pool_len, const int32_t* desc, int n_pairs,
                                  const int32_t* order, int n_segments, const int32_t* seg_pairs, const int32_t* seg_len, int query_len,
                                  int padded_seq_len, int64_t sep_id, int64_t pad_id, int64_t* joint_input_ids,
                                  int64_t* joint_attention_mask, void* hip_stream) {
  const char* what = "rr_assemble_joint";
  if (!h) return RR_ERR_BAD_ARG;
  rr_model* m = h;
  if (!desc || !order || !seg_pairs || !seg_len || !joint_input_ids || !joint_attention_mask || (!pool && pool_len > 0))
    return fail(m, RR_ERR_BAD_ARG, "%s: null argument", what);
  const int ql = query_len, S = padded_seq_len;
  if (pool_len < 0 || n_pairs <= 0 || n_segments <= 0 || n_segments > 64 || ql <= 0 || S <= ql)
    return fail(m, RR_ERR_BAD_SHAPE, "%s: pool_len=%lld, %d pairs, %d segments (1..64), query_len %d, padded length %d", what,
                (long long)pool_len, n_pairs, n_segments, ql, S);
  const int floor_len = std::min(S, m->cfg.cross_attn_len);   // the mapping network's cross-attention window
  long long pairs = 0, rows = 0;
  for (int s = 0; s < n_segments; ++s) {
    if (seg_pairs[s] <= 0 || seg_len[s] <= ql || seg_len[s] < floor_len || seg_len[s] > S)
      return fail(m, RR_ERR_BAD_SHAPE, "%s: segment %d holds %d pairs of length %d (lengths in (%d, %d], at least %d)", what, s,
                  seg_pairs[s], seg_len[s], ql, S, floor_len);
    pairs += seg_pairs[s];
    rows += (long long)seg_pairs[s] * seg_len[s];
  }
  if (pairs != n_pairs || rows > INT32_MAX)
    return fail(m, RR_ERR_BAD_SHAPE, "%s: the segments hold %lld pairs (%lld rows), the call has %d", what, pairs, rows, n_pairs);
  std::vector<char> seen((size_t)n_pairs, 0);
  for (int i = 0; i < n_pairs; ++i) {
    const int32_t p = order[i];
    if (p < 0 || p >= n_pairs || seen[(size_t)p]) return fail(m, RR_ERR_BAD_SHAPE, "%s: order is not a permutation (entry %d = %d)", what, i, p);
    seen[(size_t)p] = 1;
  }
  const int ctx_w = S - ql;
  std::vector<rr_asm_joint> staged((size_t)n_pairs);
  int i = 0;
  long long row0 = 0;
  for (int s = 0; s < n_segments; ++s)
    for (int k = 0; k < seg_pairs[s]; ++k, ++i, row0 += seg_len[s]) {
      const int32_t* d = desc + 3 * (size_t)order[i];
      const long long real = (long long)ql + std::min((long long)d[2] + 1, (long long)ctx_w);
      if (d[0] < 0 || d[1] < 0 || d[2] < 0 || (long long)d[0] + 2LL * ql > pool_len || (long long)d[1] + d[2] > pool_len ||
          real > seg_len[s])
        return fail(m, RR_ERR_BAD_SHAPE, "%s: pair %d (query offset %d, context offset %d, m %d) does not fit a pool of %lld ids and "
                    "its segment's length %d", what, order[i], d[0], d[1], d[2], (long long)pool_len, seg_len[s]);
      staged[(size_t)i] = rr_asm_joint{d[0], ql, d[1], d[2], ctx_w, seg_len[s], (int32_t)row0, 0};
    }
  hipStream_t st = (hipStream_t)hip_stream;
  void* dev = nullptr;
  RR_TRY(asm_stage(m, what, staged.data(), staged.size() * sizeof(rr_asm_joint), st, &dev));
  RR_RUN(m, st, RR_K_EMBED, 0.0, (double)rows * 16.0 + 8.0 * (double)rows,
         rr_launch_assemble_joint(pool, pool_len, (const rr_asm_joint*)dev, n_pairs, sep_id, pad_id, joint_input_ids,
                                  joint_attention_mask, st));
  return asm_done(m, st);
}

// FullContextRerankModel.forward (rerank_model.py:523-591) on the tokenised pairs.  FAM_JOINT: RerankModel.forward semantics
// (rerank_model.py:171-331) on the pre-assembled joint sequence: token types all 0, query_mask with instruction masking,
// cross-encoder order [query | image | context], and the reference's `loss_fn(logits, logits)` quirk (:328).
// Packed: the token arrays hold the segments' pairs back to back at THEIR row length, image features per pair, r.len = the
// padded length the reference would use.
static int forward_full(rr_handle h, Request r) {
  if (!h) return RR_ERR_BAD_ARG;
  rr_model* m = h;
  const rr_config& c = m->cfg;
  const bool joint = r.family == FAM_JOINT;
  const bool vision = r.image_cls != nullptr || r.image_patches != nullptr;
  const int P = vision ? c.prefix_len + c.n_patches : 0;
  std::vector<std::pair<int, int>> table;
  if (r.packed)
    RR_TRY(packed_segments(m, joint ? "rr_forward_joint_packed" : "rr_forward_packed", r, joint ? std::max(r.q_len, 0) : 0,
                           joint ? c.prefix_len + c.n_patches : P, &table));
  if (c.model_kind != RR_MODEL_FULL_CONTEXT) return fail(m, RR_ERR_BAD_ARG, "rr_forward on an interaction model; use rr_forward_interaction");
  if (!m->finalized) return fail(m, RR_ERR_BAD_ARG, "rr_forward before rr_finalize_weights");
  RR_TRY(range_guard_enter(m));
  if (!r.ids || !r.mask || !r.logits) return fail(m, RR_ERR_BAD_ARG, "rr_forward: null input_ids/attention_mask/logits_out");
  const int Bq = r.Bq, K = r.K, S = r.len, q_len = r.q_len, pair_begin = r.pair_begin;
  if (Bq <= 0 || K <= 0 || S <= 0) return fail(m, RR_ERR_BAD_SHAPE, "rr_forward: Bq=%d K=%d S=%d", Bq, K, S);
  RR_TRY(check_head(m, "rr_forward", Bq, K, pair_begin, r.pair_end, r.labels, r.logits2, r.loss, r.scores, r.order, joint));
  if (S > c.max_pos) return fail(m, RR_ERR_BAD_SHAPE, "seq_len %d exceeds max_position_embeddings %d", S, c.max_pos);
  if (vision && !(r.image_cls && r.image_patches)) return fail(m, RR_ERR_BAD_ARG, "image_cls and image_patches must be given together");
  if (vision && !c.has_vision) return fail(m, RR_ERR_UNSUPPORTED, "image features passed to a text_only model");
  const int T = S + P;
  if (T > c.ce_max_pos)
    return fail(m, RR_ERR_BAD_SHAPE, "cross-encoder length %d exceeds cross_encoder_max_position_embeddings %d", T, c.ce_max_pos);
  RR_TRY(check_rows(m, "rr_forward", (long long)r.pair_end - pair_begin, T));
  // length-bucketed forward (rr_set_padded_seq_len): S is this call's (shorter) row length, the cross-encoder positions of the
  // vision tokens are those behind the padded text
  int bucket_of = 0;
  if (m->padded_S > 0 && !joint && !r.packed && S != m->padded_S) {
    if (S > m->padded_S) return fail(m, RR_ERR_BAD_SHAPE, "seq_len %d exceeds the padded length %d set by rr_set_padded_seq_len", S, m->padded_S);
    if (m->padded_S + P > c.ce_max_pos)
      return fail(m, RR_ERR_BAD_SHAPE, "padded cross-encoder length %d exceeds cross_encoder_max_position_embeddings %d", m->padded_S + P, c.ce_max_pos);
    // the mapping network's cross-attention reads the first cross_attn_len text rows of a pair: a bucket shorter than that
    // would read fewer rows than the padded call does (rr_forward_packed refuses the same case)
    if (vision && S < (m->padded_S < c.cross_attn_len ? m->padded_S : c.cross_attn_len))
      return fail(m, RR_ERR_BAD_SHAPE, "bucketed seq_len %d is below the %d text rows the vision mapping network attends to", S,
                  m->padded_S < c.cross_attn_len ? m->padded_S : c.cross_attn_len);
    bucket_of = m->padded_S;
  }
  if (joint) {
    if (!vision) return fail(m, RR_ERR_UNSUPPORTED, "text_only is not implemented for this model");   // rerank_model.py:184-185
    if (q_len <= 0 || q_len >= S) return fail(m, RR_ERR_BAD_SHAPE, "query length %d outside (0,%d)", q_len, S);
  }

  hipStream_t st = r.stream;
  RR_HIP(m, hipSetDevice(c.device));
  const int n = r.pair_end - pair_begin;
  const int q_lo = pair_begin / K, q_hi = (r.pair_end - 1) / K, nq = q_hi - q_lo + 1;   // queries touched by the slice
  Work w;
  const size_t need = layout(c, n, Bq, S, vision, nullptr, &w);
  RR_TRY(ensure_ws(m, need, st));
  layout(c, n, Bq, S, vision, m->ws, &w);
  m->last_stream = st;

  const int Hd = c.hidden, I = c.intermediate, D = c.li_dim;
  const int64_t* ids = r.ids + (size_t)pair_begin * S;
  const int64_t* am = r.mask + (size_t)pair_begin * S;
  const int64_t* tts = r.token_types ? r.token_types + (size_t)pair_begin * S : nullptr;
  const RowPlan plan = plan_rows(r.family, n, S, P, table, bucket_of);
  const std::vector<Seg>& segs = plan.segs;
  std::vector<SegView> text_view;
  for (const Seg& g : segs) text_view.push_back(SegView{g.n, g.S, g.r0});
  const int R = (int)(segs.back().r0 + (size_t)segs.back().n * segs.back().S);       // text rows of the call
  const int RT = (int)(segs.back().rt0 + (size_t)segs.back().n * segs.back().T);     // cross-encoder rows
  const std::vector<SegView>* tv = plan.packed ? &text_view : nullptr;

  // ---- masks -> additive key bias (text: tokenizer mask; cross encoder: id != 0, vision = 1)
  const int txt_split = joint ? q_len : (1 << 30), txt_shift = joint ? P : 0;   // [query | image | context] reorder
  if (joint) {
    for (const Seg& g : segs)
      RR_RUN(m, st, RR_K_EMBED, 0.0, 24.0 * g.n * g.S + 4.0 * g.n * g.T,
             rr_launch_joint_masks(ids + g.r0, am + g.r0, g.n, g.S, P, q_len, r.instruction_token, w.text_bias + g.r0,
                                   w.li_mask + g.r0, w.ce_bias + g.rt0, st));
  } else {
    for (const Seg& g : segs)
      RR_RUN(m, st, RR_K_EMBED, 0.0, 16.0 * g.n * g.S + 8.0 * g.n * g.T,
             rr_launch_key_bias(ids + g.r0, am + g.r0, g.n, g.S, g.T, w.text_bias + g.r0, w.ce_bias + g.rt0, st));
  }
  // ---- text encoder (FLMRTextModel = BertModel)
  for (const Seg& g : segs)
    RR_RUN(m, st, RR_K_EMBED, 0.0, (3 * 4.0 + 6.0) * g.n * g.S * Hd,
           rr_launch_embed_ln(ids + g.r0, tts ? tts + g.r0 : nullptr, m->word, m->pos, m->type, m->emb_g, m->emb_b, c.ln_eps,
                              g.n * g.S, g.S, Hd, c.vocab_size, c.type_vocab, w.h32 + g.r0 * Hd, w.h16 + g.r0 * Hd, m->dt, st));
  {
    ResidSrc rs{w.h32, nullptr, nullptr, nullptr};      // embeddings LayerNorm output, materialised
    int folded = OP_NORMALISED;
    const int fp8_from = c.fp8 ? fp8_first_layer_of(opt_of(m, RR_OPT_FP8_FIRST_LAYER), c.layers, m->q8_fmt == 1) : 0;   // layers below it keep 16-bit operands
    for (int l = 0; l < c.layers; ++l)                    // the last layer's normalised rows feed the 768 -> 128 projection
      RR_TRY(run_layer(m, st, m->text_layers[l], n, S, Hd, c.heads, I, c.ln_eps, w.text_bias, w, rs, folded,
                       l == c.layers - 1, m->debug, nullptr, 0, tv, c.fp8 ? (l >= fp8_from ? 1 : 0) : -1,
                       c.fp8 && l + 1 < c.layers && l + 1 >= fp8_from));
  }
  if (m->debug) {
    const size_t el = (size_t)R * Hd;
    if (m->tap_text_elems < el) {
      if (m->tap_text) { RR_HIP(m, hipStreamSynchronize(st)); RR_HIP(m, hipFree(m->tap_text)); m->tap_text = nullptr; }
      RR_HIP(m, hipMalloc((void**)&m->tap_text, el * 4));
    }
    m->tap_text_elems = el;
    RR_HIP(m, hipMemcpyAsync(m->tap_text, w.h32, el * 4, hipMemcpyDeviceToDevice, st));
  }
  // ---- 768 -> 128 projection (no bias), mask, L2 normalise -> li16[:, :S]
  RR_GEMM(m, st, w.h16, Hd, m->w_li, nullptr, nullptr, 0, w.li32, D, R, D, Hd, EPI_BIAS_F32, 4.0);
  for (const Seg& g : segs)
    RR_RUN(m, st, RR_K_TAIL, 0.0, 6.0 * g.n * g.S * D + 8.0 * g.n * g.S,
           rr_launch_li_normalize(w.li32 + g.r0 * D, ids + g.r0, g.S, g.n, g.S, D, g.T, 0, 0, 1, 0, w.li16 + g.rt0 * D, m->dt, 1,
                                  joint ? w.li_mask + g.r0 : nullptr, txt_split, txt_shift, st));

  if (vision) {
    const int np = c.n_patches, PL = c.prefix_len, Vh = c.vision_hidden, mid = D * PL / 2, outd = D * PL;
    auto vis_at = [&](const Seg& g) { return joint ? q_len : g.S; };   // where a pair's image tokens go: behind its query / its text
    const float* cls = r.image_cls + (size_t)q_lo * Vh;
    const float* pat = r.image_patches + (size_t)q_lo * np * Vh;
    // prefix MLP (per query): Linear -> Tanh -> Linear -> view [PL, D]
    RR_RUN(m, st, RR_K_TAIL, 0.0, 6.0 * nq * Vh, rr_launch_f32_to_bf16(cls, w.cls16, (size_t)nq * Vh, m->dt, st));
    RR_GEMM(m, st, w.cls16, Vh, m->w_vp0, m->b_vp0, nullptr, 0, w.vp_mid16, mid, nq, mid, Vh, EPI_BIAS_TANH_BF16, 2.0);
    RR_GEMM(m, st, w.vp_mid16, mid, m->w_vp2, m->b_vp2, nullptr, 0, w.vp_out32, outd, nq, outd, mid, EPI_BIAS_F32, 4.0);
    for (const Seg& g : segs)           // (packed: per pair, K = 1 -> pair p0 + i reads prefix p0 + i)
      RR_RUN(m, st, RR_K_TAIL, 0.0, 6.0 * g.n * PL * D,
             rr_launch_li_normalize(w.vp_out32, nullptr, 0, g.n, PL, D, g.T, vis_at(g), pair_begin + (int)g.p0, K,
                                    q_lo, w.li16 + g.rt0 * D, m->dt, 1, nullptr, 1 << 30, 0, st));
    // mapping network: input linear + self-attention block depend on the image only => per query
    RR_RUN(m, st, RR_K_TAIL, 0.0, 6.0 * nq * np * Vh, rr_launch_f32_to_bf16(pat, w.pat16, (size_t)nq * np * Vh, m->dt, st));
    RR_GEMM(m, st, w.pat16, Vh, m->w_min, m->b_min, nullptr, 0, w.t32, Hd, nq * np, Hd, Vh, EPI_BIAS_F32, 4.0);
    RR_RUN(m, st, RR_K_TAIL, 0.0, 6.0 * nq * np * Hd, rr_launch_f32_to_bf16(w.t32, w.t16, (size_t)nq * np * Hd, m->dt, st));
    int ca = S < c.cross_attn_len ? S : c.cross_attn_len;
    for (const Seg& g : segs) ca = g.S < ca ? g.S : ca;
    if (plan.packed && ca != (S < c.cross_attn_len ? S : c.cross_attn_len))
      return fail(m, RR_ERR_BAD_SHAPE, "packed segment shorter than the %d rows the mapping network's cross-attention reads", c.cross_attn_len);
    // pair-specific text states the cross-attention reads: first `ca` rows of every pair (rerank_model.py:438-442)
    for (const Seg& g : segs)
      RR_RUN(m, st, RR_K_TAIL, 0.0, 4.0 * g.n * ca * Hd,
             rr_launch_gather_rows(w.h16 + g.r0 * Hd, w.enc16 + g.p0 * ca * Hd, g.n, ca, g.S, Hd * 2, 0, 1, 0, st));
    const float* tin32 = w.t32;    // [nq*np, Hd] (per query) for layer 0; per pair afterwards
    const bf16_t* tin16 = w.t16;
    for (int l = 0; l < c.map_layers; ++l) {
      const LayerW& L = m->map_layers[l];
      const bool per_query = (l == 0);
      const int bt = per_query ? nq : n;           // batches entering this layer
      // self-attention (no mask: the reference passes attention_mask=None, rerank_model.py:450-454)
      RR_GEMM(m, st, tin16, Hd, L.wqkv, L.bqkv, nullptr, 0, w.vqkv, 3 * Hd, bt * np, 3 * Hd, Hd, EPI_BIAS_BF16, 2.0);
      RR_RUN(m, st, RR_K_ATTENTION, 4.0 * bt * (double)np * np * Hd, 8.0 * bt * np * Hd,
             rr_launch_attention(w.vqkv, 3 * Hd, 1, 0, w.vqkv + Hd, w.vqkv + 2 * Hd, 3 * Hd, nullptr, bt, c.heads, np, np,
                                 w.vctx, Hd, m->dt, st, nullptr, 0, 0, opt_of(m, RR_OPT_ATTN_FIXED_REF)));
      RR_GEMM(m, st, w.vctx, Hd, L.wo, L.bo, tin32, Hd, w.vpre, Hd, bt * np, Hd, Hd, EPI_BIAS_RESID_F32, 4.0);
      RR_RUN(m, st, RR_K_LAYERNORM, 0.0, 10.0 * bt * np * Hd,
             rr_launch_layernorm(w.vpre, L.ln1g, L.ln1b, c.ln_eps, bt * np, Hd, w.a32, w.a16, m->dt, st));
      // cross-attention: queries from `a`, keys/values from the pair's first `ca` text states
      RR_GEMM(m, st, w.a16, Hd, L.wq_c, L.bq_c, nullptr, 0, w.q_c, Hd, bt * np, Hd, Hd, EPI_BIAS_BF16, 2.0);
      RR_GEMM(m, st, w.enc16, Hd, L.wkv_c, L.bkv_c, nullptr, 0, w.kv_c, 2 * Hd, n * ca, 2 * Hd, Hd, EPI_BIAS_BF16, 2.0);
      RR_RUN(m, st, RR_K_ATTENTION, 4.0 * n * (double)np * ca * Hd, 2.0 * n * (2.0 * np + 2.0 * ca) * Hd,
             rr_launch_attention(w.q_c, Hd, per_query ? K : 1, per_query ? pair_begin - q_lo * K : 0, w.kv_c,
                                 w.kv_c + Hd, 2 * Hd, nullptr, n, c.heads, np, ca, w.cctx, Hd, m->dt, st, nullptr, 0, 0, opt_of(m, RR_OPT_ATTN_FIXED_REF)));
      const float* resid = w.a32;
      if (per_query) {   // broadcast the per-query residual to the pairs
        RR_RUN(m, st, RR_K_TAIL, 0.0, 8.0 * n * np * Hd,
               rr_launch_gather_rows(w.a32, w.a32b, n, np, np, Hd * 4, pair_begin, K, q_lo, st));
        resid = w.a32b;
      }
      RR_GEMM(m, st, w.cctx, Hd, L.wo_c, L.bo_c, resid, Hd, w.cpre, Hd, n * np, Hd, Hd, EPI_BIAS_RESID_F32, 4.0);
      RR_RUN(m, st, RR_K_LAYERNORM, 0.0, 10.0 * n * np * Hd,
             rr_launch_layernorm(w.cpre, L.lncg, L.lncb, c.ln_eps, n * np, Hd, w.c32, w.c16, m->dt, st));
      RR_GEMM(m, st, w.c16, Hd, L.w1, L.b1, nullptr, 0, w.vmid, I, n * np, I, Hd, EPI_BIAS_GELU_BF16, 2.0);
      RR_GEMM(m, st, w.vmid, I, L.w2, L.b2, w.c32, Hd, w.cpre, Hd, n * np, Hd, I, EPI_BIAS_RESID_F32, 4.0);
      RR_RUN(m, st, RR_K_LAYERNORM, 0.0, 10.0 * n * np * Hd,
             rr_launch_layernorm(w.cpre, L.ln2g, L.ln2b, c.ln_eps, n * np, Hd, w.m32, w.m16, m->dt, st));
      tin32 = w.m32;
      tin16 = w.m16;
    }
    if (c.map_layers == 0) {   // degenerate: no mapping layer, features are per query -> broadcast
      RR_RUN(m, st, RR_K_TAIL, 0.0, 4.0 * n * np * Hd,
             rr_launch_gather_rows(w.t16, w.m16, n, np, np, Hd * 2, pair_begin, K, q_lo, st));
    }
    RR_GEMM(m, st, w.m16, Hd, m->w_mout, m->b_mout, nullptr, 0, w.mo32, D, n * np, D, Hd, EPI_BIAS_F32, 4.0);
    for (const Seg& g : segs)
      RR_RUN(m, st, RR_K_TAIL, 0.0, 6.0 * g.n * np * D,
             rr_launch_li_normalize(w.mo32 + g.p0 * np * D, nullptr, 0, g.n, np, D, g.T, vis_at(g) + PL, 0, 1, 0,
                                    w.li16 + g.rt0 * D, m->dt, 1, nullptr, 1 << 30, 0, st));
  }
  m->tap_li = w.li16;
  m->tap_li_elems = (size_t)RT * D;

  const float* adj = nullptr;
  int adj_ld = 0;
  if (r.fusion_scores) {   // rerank_model.py:276-319: scores [N, S, q_len + P] (packed: the context rows) -> additive bias
    if (!joint) return fail(m, RR_ERR_BAD_ARG, "attention fusion belongs to the joint (RerankModel) forward");
    RR_TRY(fusion_bias(m, st, plan, r.fusion_scores, q_len + P, S - q_len, q_len, 2, r.fusion_mult, pair_begin, &adj_ld));
    adj = m->adj;
  }
  RR_TRY(run_cross_encoder(m, st, w, plan, adj, adj_ld));
  RR_TRY(run_heads(m, st, w, segs, r));
  return range_guard_exit(m, st);
}

/* InteractionRerankModel.forward (interaction_rerank_model.py:110-166) from the retriever's late-interaction
 * tensors.  NORMAL: cat(query, context) -> Linear -> CrossEncoder; MORES (mores_model.py:21-94): Lc layers of
 * cross-attention(query -> doc) -> self-attention -> FFN over the query tokens. */
static int forward_interaction(rr_handle h, Request r) {
  // packed: context_li / context_mask hold the segments' pairs back to back at THEIR context length, query_li / query_mask one
  // entry per pair, r.len = the padded context length
  if (!h) return RR_ERR_BAD_ARG;
  rr_model* m = h;
  const rr_config& c = m->cfg;
  const int Lq = r.q_len;
  std::vector<std::pair<int, int>> table;
  if (r.packed) RR_TRY(packed_segments(m, "rr_forward_interaction_packed", r, 0, Lq < 0 ? 0 : Lq, &table));
  if (c.model_kind == RR_MODEL_FULL_CONTEXT) return fail(m, RR_ERR_BAD_ARG, "rr_forward_interaction on a full-context model");
  if (!m->finalized) return fail(m, RR_ERR_BAD_ARG, "rr_forward_interaction before rr_finalize_weights");
  if (r.fusion_from_li && c.model_kind == RR_MODEL_MORES)
    return fail(m, RR_ERR_UNSUPPORTED, "Attention adj is not implemented for MORES");   // mores_model.py:72-73
  RR_TRY(range_guard_enter(m));
  if (!r.query_li || !r.query_mask || !r.logits || (!r.bank && (!r.context_li || !r.context_mask)))
    return fail(m, RR_ERR_BAD_ARG, "rr_forward_interaction: null tensor");
  const int Bq = r.Bq, K = r.K, Lc = r.len, pair_begin = r.pair_begin;
  if (Bq <= 0 || K <= 0 || Lq <= 0 || Lc <= 0) return fail(m, RR_ERR_BAD_SHAPE, "Bq=%d K=%d Lq=%d Lc=%d", Bq, K, Lq, Lc);
  const int T = Lq + Lc;
  RR_TRY(check_head(m, "rr_forward_interaction", Bq, K, pair_begin, r.pair_end, r.labels, r.logits2, r.loss, r.scores, r.order,
                    false));
  if (c.model_kind == RR_MODEL_INTERACTION && T > c.ce_max_pos)
    return fail(m, RR_ERR_BAD_SHAPE, "sequence %d exceeds cross_encoder_max_position_embeddings %d", T, c.ce_max_pos);
  RR_TRY(check_rows(m, "rr_forward_interaction", (long long)r.pair_end - pair_begin, T));

  hipStream_t st = r.stream;
  RR_HIP(m, hipSetDevice(c.device));
  const int n = r.pair_end - pair_begin;
  Work w{};
  const size_t need = layout_interaction(c, n, Bq, Lq, Lc, nullptr, &w);
  RR_TRY(ensure_ws(m, need, st));
  layout_interaction(c, n, Bq, Lq, Lc, m->ws, &w);
  m->last_stream = st;
  const int D = c.li_dim, Hc = c.ce_hidden, Ic = c.ce_intermediate;
  const float* cli = r.bank ? nullptr : r.context_li + (size_t)pair_begin * Lc * D;
  const float* cm = r.bank ? nullptr : r.context_mask + (size_t)pair_begin * Lc;
  const float *qli = r.query_li, *qm = r.query_mask;
  // segments: Seg.S = context tokens per pair, Seg.r0 = first context row, Seg.rt0 = first row of the concatenated
  // [query | context] sequence
  const RowPlan plan = plan_rows(FAM_INTERACTION, n, Lc, Lq, table, 0);
  const std::vector<Seg>& segs = plan.segs;
  const Seg& last = segs.back();
  const int C = (int)(last.r0 + (size_t)last.n * last.S), RT = (int)(last.rt0 + (size_t)last.n * last.T);

  if (r.bank) {
    // the 16-bit [query | context] rows straight from the bank, one launch per segment, with the float mask rows the bias kernel
    // reads (per pair, as the packed call takes them) and, for the attention fusion, float32 copies of the rows for li_scores
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
    const size_t o_cm = take((size_t)C * 4), o_qm = take((size_t)n * Lq * 4);
    const size_t o_c32 = r.fusion_from_li ? take((size_t)C * D * 4) : 0, o_q32 = r.fusion_from_li ? take((size_t)n * Lq * D * 4) : 0;
    RR_TRY(ensure_block(m, m->bank_blk, m->bank_blk_cap, off, st, "the bank forward's block"));
    float *cm_w = (float*)(m->bank_blk + o_cm), *qm_w = (float*)(m->bank_blk + o_qm);
    float* c32 = r.fusion_from_li ? (float*)(m->bank_blk + o_c32) : nullptr;
    float* q32 = r.fusion_from_li ? (float*)(m->bank_blk + o_q32) : nullptr;
    void* dev = nullptr;
    RR_TRY(asm_stage(m, "rr_forward_interaction_bank", r.bank_pairs->data(), r.bank_pairs->size() * sizeof(rr_bank_pair), st, &dev));
    // bytes of a context row: what the bank's row costs (compressed rows are decoded in the gather), its 16-bit copy, its float32 copy
    const rr_bank_view bank = bank_view(r.bank);
    const double ctx_row = rr_bank_row_bytes(bank, D) + D * (2.0 + (c32 ? 4.0 : 0.0));
    for (const Seg& g : segs)
      RR_RUN(m, st, RR_K_TAIL, 0.0, (double)g.n * (Lq * D * (4.0 + 2.0 + (q32 ? 4.0 : 0.0)) + (double)g.S * ctx_row),
             rr_launch_bank_gather((const rr_bank_pair*)dev + g.p0, g.n, Lq, g.S, D, r.query_li, r.query_mask, bank, w.li16 + g.rt0 * D, m->dt,
                                   qm_w + g.p0 * Lq, cm_w + g.r0, q32 ? q32 + g.p0 * Lq * D : nullptr, c32 ? c32 + g.r0 * D : nullptr, st));
    RR_TRY(asm_done(m, st));
    cm = cm_w;
    qm = qm_w;
    cli = c32;
    if (q32) qli = q32;
  }
  for (const Seg& g : segs)
    RR_RUN(m, st, RR_K_EMBED, 0.0, 8.0 * g.n * g.T,
           rr_launch_interaction_bias(qm, cm + g.r0, g.n, Lq, g.S, pair_begin + (int)g.p0, K, w.ce_bias + g.rt0,
                                      w.text_bias + g.p0 * Lq, w.li32 + g.r0, st));
  // operands in 16 bits, query rows broadcast to the K pairs of the query (repeat_interleave, :128-129); a bank call's gather
  // has written them
  for (size_t s = 0; !r.bank && s < segs.size(); ++s) {
    const Seg& g = segs[s];
    RR_RUN(m, st, RR_K_TAIL, 0.0, 6.0 * g.n * Lq * D,
           rr_launch_li_normalize(r.query_li, nullptr, 0, g.n, Lq, D, g.T, 0, pair_begin + (int)g.p0, K, 0, w.li16 + g.rt0 * D, m->dt, 0,
                                  nullptr, 1 << 30, 0, st));
    RR_RUN(m, st, RR_K_TAIL, 0.0, 6.0 * g.n * g.S * D,
           rr_launch_li_normalize(cli + g.r0 * D, nullptr, 0, g.n, g.S, D, g.T, Lq, 0, 1, 0, w.li16 + g.rt0 * D, m->dt, 0, nullptr,
                                  1 << 30, 0, st));
  }
  m->tap_li = w.li16;
  m->tap_li_elems = (size_t)RT * D;

  if (c.model_kind == RR_MODEL_INTERACTION) {
    const float* adj = nullptr;
    int adj_ld = 0;
    // interaction_rerank_model.py:131-142: scores [N, Lc, Lq] over the tokens [query | context] (packed: the context axis stays
    // padded, the reference's normalisers run over it)
    if (r.fusion_from_li) {
      // the retriever's scores_raw of the slice (flmr_utils.py:22-48) into the handle's block [n][Lc][Lq], then as the padded
      // call with explicit scores; a packed pair's rows beyond its segment are masked rows of the padded matrix
      RR_TRY(ensure_block(m, m->li_sc, m->li_sc_cap, (size_t)n * Lc * Lq * sizeof(float), st, "the late-interaction score block"));
      float* ms = r.maxsim ? r.maxsim + pair_begin : nullptr;
      for (const Seg& g : segs)
        RR_RUN(m, st, RR_K_TAIL, 2.0 * g.n * (double)g.S * Lq * D, 4.0 * g.n * ((double)g.S * D + (double)Lc * Lq),
               rr_launch_li_scores(qli, cli + g.r0 * D, cm + g.r0, g.n, K, Lq, g.S, Lc, D, pair_begin + (int)g.p0,
                                   m->li_sc + g.p0 * Lc * Lq, ms ? ms + g.p0 : nullptr, st));
      RR_TRY(fusion_bias(m, st, plan, m->li_sc, Lq, Lc, 0, 0, r.fusion_mult, 0, &adj_ld));
      adj = m->adj;
    } else if (r.fusion_scores) {
      RR_TRY(fusion_bias(m, st, plan, r.fusion_scores, Lq, Lc, 0, 0, r.fusion_mult, pair_begin, &adj_ld));
      adj = m->adj;
    }
    RR_TRY(run_cross_encoder(m, st, w, plan, adj, adj_ld));
    RR_TRY(run_heads(m, st, w, segs, r));
    return range_guard_exit(m, st);
  }
  if (r.fusion_scores) return fail(m, RR_ERR_UNSUPPORTED, "Attention adj is not implemented for MORES");   // mores_model.py:72-73

  // ---- MORES: hidden = Linear(query) [n*Lq, Hc] (no embeddings, no LayerNorm), doc = Linear(context) [n*Lc, Hc]
  // gather the two token groups out of the concatenated 16-bit buffer into contiguous GEMM operands
  // (packed: the query side keeps its n * Lq rows, the doc side holds the C rows that exist)
  for (const Seg& g : segs)
    RR_RUN(m, st, RR_K_TAIL, 0.0, 4.0 * g.n * Lq * D,
           rr_launch_gather_rows(w.li16 + g.rt0 * D, w.a16 + g.p0 * Lq * D, g.n, Lq, g.T, D * 2, 0, 1, 0, st));
  RR_GEMM(m, st, w.a16, D, m->w_cemap, m->b_cemap, nullptr, 0, w.h32, Hc, n * Lq, Hc, D, EPI_BIAS_F32, 4.0);
  RR_RUN(m, st, RR_K_TAIL, 0.0, 6.0 * n * Lq * Hc, rr_launch_f32_to_bf16(w.h32, w.h16, (size_t)n * Lq * Hc, m->dt, st));
  for (const Seg& g : segs)
    RR_RUN(m, st, RR_K_TAIL, 0.0, 4.0 * g.n * g.S * D,
           rr_launch_gather_rows((const char*)w.li16 + ((size_t)g.rt0 + Lq) * D * 2, w.ctx + g.r0 * D, g.n, g.S, g.T, D * 2, 0, 1, 0,
                                 st));
  RR_GEMM(m, st, w.ctx, D, m->w_cemap, m->b_cemap, nullptr, 0, w.enc16, Hc, C, Hc, D, EPI_BIAS_BF16, 2.0);
  // cross-attention per segment (Tk = its context length) under the padded call's schedule (its grid: n pairs x Lq rows)
  const long x_sched = plan.packed ? (((long)n * c.ce_heads + 7) / 8) * 8 * ((Lq + 127) / 128) : 0;
  for (int l = 0; l < c.ce_layers; ++l) {
    const LayerW& L = m->ce_layers[l];
    const int rq = n * Lq;
    // cross-attention first (MORES_BertLayer.forward, mores_model.py:31-41): queries from the query tokens, keys/values from doc
    RR_GEMM(m, st, w.h16, Hc, L.wq_c, L.bq_c, nullptr, 0, w.q_c, Hc, rq, Hc, Hc, EPI_BIAS_BF16, 2.0);
    RR_GEMM(m, st, w.enc16, Hc, L.wkv_c, L.bkv_c, nullptr, 0, w.kv_c, 2 * Hc, C, 2 * Hc, Hc, EPI_BIAS_BF16, 2.0);
    for (const Seg& g : segs)
      RR_RUN(m, st, RR_K_ATTENTION, 4.0 * g.n * (double)Lq * g.S * Hc, 2.0 * g.n * (2.0 * Lq + 2.0 * g.S) * Hc,
             rr_launch_attention(w.q_c + g.p0 * Lq * Hc, Hc, 1, 0, w.kv_c + g.r0 * 2 * Hc, w.kv_c + g.r0 * 2 * Hc + Hc, 2 * Hc,
                                 w.li32 + g.r0, g.n, c.ce_heads, Lq, g.S, w.ctx + g.p0 * Lq * Hc, Hc, m->dt, st, nullptr, 0, x_sched,
                                 opt_of(m, RR_OPT_ATTN_FIXED_REF)));
    RR_GEMM(m, st, w.ctx, Hc, L.wo_c, L.bo_c, w.h32, Hc, w.pre, Hc, rq, Hc, Hc, EPI_BIAS_RESID_F32, 4.0);
    RR_RUN(m, st, RR_K_LAYERNORM, 0.0, 10.0 * rq * Hc,
           rr_launch_layernorm(w.pre, L.lncg, L.lncb, c.ln_eps, rq, Hc, w.a32, w.a16, m->dt, st));
    // self-attention over the query tokens
    RR_GEMM(m, st, w.a16, Hc, L.wqkv, L.bqkv, nullptr, 0, w.qkv, 3 * Hc, rq, 3 * Hc, Hc, EPI_BIAS_BF16, 2.0);
    RR_RUN(m, st, RR_K_ATTENTION, 4.0 * n * (double)Lq * Lq * Hc, 8.0 * rq * Hc,
           rr_launch_attention(w.qkv, 3 * Hc, 1, 0, w.qkv + Hc, w.qkv + 2 * Hc, 3 * Hc, w.text_bias, n, c.ce_heads, Lq, Lq,
                               w.ctx, Hc, m->dt, st, nullptr, 0, 0, opt_of(m, RR_OPT_ATTN_FIXED_REF)));
    RR_GEMM(m, st, w.ctx, Hc, L.wo, L.bo, w.a32, Hc, w.pre, Hc, rq, Hc, Hc, EPI_BIAS_RESID_F32, 4.0);
    RR_RUN(m, st, RR_K_LAYERNORM, 0.0, 10.0 * rq * Hc,
           rr_launch_layernorm(w.pre, L.ln1g, L.ln1b, c.ln_eps, rq, Hc, w.a32, w.a16, m->dt, st));
    // FFN
    RR_GEMM(m, st, w.a16, Hc, L.w1, L.b1, nullptr, 0, w.mid, Ic, rq, Ic, Hc, EPI_BIAS_GELU_BF16, 2.0);
    RR_GEMM(m, st, w.mid, Ic, L.w2, L.b2, w.a32, Hc, w.pre, Hc, rq, Hc, Ic, EPI_BIAS_RESID_F32, 4.0);
    RR_RUN(m, st, RR_K_LAYERNORM, 0.0, 10.0 * rq * Hc,
           rr_launch_layernorm(w.pre, L.ln2g, L.ln2b, c.ln_eps, rq, Hc, w.h32, w.h16, m->dt, st));
  }
  m->tap_ce = w.h32;
  m->tap_ce_elems = (size_t)n * Lq * Hc;
  const std::vector<Seg> one{Seg{n, Lq, Lq, 0, 0, 0}};
  RR_TRY(run_heads(m, st, w, one, r));
  return range_guard_exit(m, st);
}

// rr_forward_interaction_bank (include/rerank_mi355.h): everything about the bank, the segment table and the per-pair indices is
// checked here, on the host; forward_interaction then checks what it checks for a packed call, stages the descriptors and runs.
static int forward_interaction_bank(rr_handle h, rr_bank* b, const float* query_li, const float* query_mask, int n_queries, int Lq,
                                    const int32_t* pair_passage, const int32_t* pair_query, int n_segments, const int32_t* seg_pairs,
                                    const int32_t* seg_len, int padded_context_len, int fusion_from_li, float fusion_multiplier,
                                    float* logits_out, float* logits2_out, float* maxsim_out, void* hip_stream) {
  const char* what = "rr_forward_interaction_bank";
  if (!h) return RR_ERR_BAD_ARG;
  rr_model* m = h;
  const rr_config& c = m->cfg;
  if (!b || !query_li || !query_mask || !pair_passage || !pair_query || !seg_pairs || !seg_len || !logits_out)
    return fail(m, RR_ERR_BAD_ARG, "%s: null argument", what);
  RR_TRY(bank_usable(m, what, b));
  if (fusion_from_li && c.model_kind == RR_MODEL_MORES)
    return fail(m, RR_ERR_UNSUPPORTED, "Attention adj is not implemented for MORES");   // mores_model.py:72-73
  if (maxsim_out && !fusion_from_li) return fail(m, RR_ERR_BAD_ARG, "%s: maxsim_out needs fusion_from_li", what);
  if (((uintptr_t)query_li) & 15) return fail(m, RR_ERR_BAD_ARG, "%s: query_li must be 16-byte aligned", what);
  hipStream_t st = (hipStream_t)hip_stream;
  RR_TRY(capture_guard(m, st, CAP_STAGES, what));
  if (n_queries <= 0 || Lq <= 0 || padded_context_len <= 0)
    return fail(m, RR_ERR_BAD_SHAPE, "%s: n_queries=%d Lq=%d padded_context_len=%d", what, n_queries, Lq, padded_context_len);
  if (n_segments <= 0 || n_segments > 64) return fail(m, RR_ERR_BAD_SHAPE, "%s: %d segments (1..64)", what, n_segments);
  long long pairs = 0;
  for (int s = 0; s < n_segments; ++s) {
    if (seg_pairs[s] <= 0 || seg_len[s] <= 0 || seg_len[s] > padded_context_len)
      return fail(m, RR_ERR_BAD_SHAPE, "%s: segment %d holds %d pairs of length %d (lengths in (0, %d])", what, s, seg_pairs[s], seg_len[s],
                  padded_context_len);
    pairs += seg_pairs[s];
  }
  if (pairs > (1 << 24)) return fail(m, RR_ERR_BAD_SHAPE, "%s: %lld pairs", what, pairs);
  std::vector<rr_bank_pair> staged((size_t)pairs);
  size_t i = 0;
  for (int s = 0; s < n_segments; ++s)
    for (int k = 0; k < seg_pairs[s]; ++k, ++i)
      RR_TRY(bank_checked_pair(m, what, b, (long long)i, pair_passage[i], pair_query[i], n_queries, seg_len[s], "its segment", &staged[i]));
  Request r;
  r.family = FAM_INTERACTION; r.query_li = query_li; r.query_mask = query_mask;
  r.fusion_from_li = fusion_from_li != 0; r.maxsim = maxsim_out; r.fusion_mult = fusion_multiplier;
  r.packed = true; r.n_segments = n_segments; r.seg_pairs = seg_pairs; r.seg_len = seg_len; r.len = padded_context_len; r.q_len = Lq;
  r.logits = logits_out; r.logits2 = logits2_out; r.stream = st;
  r.bank = b; r.bank_pairs = &staged;
  return forward_interaction(h, r);
}

// rr_li_scores (include/rerank_mi355.h): the stand-alone operator, any model kind; every check before anything is enqueued
static int li_scores_call(rr_handle h, const float* query_li, const float* context_li, const float* context_mask, int Bq, int K,
                          int Lq, int Lc, int pair_begin, int pair_end, float* scores_out, float* maxsim_out, void* hip_stream) {
  const char* what = "rr_li_scores";
  if (!h) return RR_ERR_BAD_ARG;
  rr_model* m = h;
  if (!query_li || !context_li || !context_mask) return fail(m, RR_ERR_BAD_ARG, "%s: null tensor", what);
  if (!scores_out && !maxsim_out) return fail(m, RR_ERR_BAD_ARG, "%s: scores_out and maxsim_out are both null", what);
  if (Bq <= 0 || K <= 0 || Lq <= 0 || Lc <= 0) return fail(m, RR_ERR_BAD_SHAPE, "%s: Bq=%d K=%d Lq=%d Lc=%d", what, Bq, K, Lq, Lc);
  const long long N = (long long)Bq * K;
  if (pair_begin < 0 || pair_end > N || pair_begin >= pair_end)
    return fail(m, RR_ERR_BAD_SHAPE, "%s: pair slice [%d,%d) outside [0,%lld)", what, pair_begin, pair_end, N);
  RR_TRY(check_rows(m, what, (long long)pair_end - pair_begin, Lc));
  if ((((uintptr_t)query_li) | ((uintptr_t)context_li)) & 15)
    return fail(m, RR_ERR_BAD_ARG, "%s: query_li / context_li must be 16-byte aligned", what);
  const int D = m->cfg.li_dim, n = pair_end - pair_begin;
  hipStream_t st = (hipStream_t)hip_stream;
  RR_HIP(m, hipSetDevice(m->cfg.device));
  m->last_stream = st;
  const size_t b = (size_t)pair_begin;
  RR_RUN(m, st, RR_K_TAIL, 2.0 * n * (double)Lc * Lq * D,
         4.0 * n * ((double)Lc * D + (scores_out ? (double)Lc * Lq : 0.0)) + 4.0 * Bq * (double)Lq * D,
         rr_launch_li_scores(query_li, context_li + b * Lc * D, context_mask + b * Lc, n, K, Lq, Lc, Lc, D, pair_begin,
                             scores_out ? scores_out + b * Lc * Lq : nullptr, maxsim_out ? maxsim_out + b : nullptr, st));
  return RR_OK;
}

static int64_t rr_debug_read_impl(rr_handle h, const char* name, float* host_out, int64_t max_elems) {
  if (!h || !name || !host_out) return RR_ERR_BAD_ARG;
  if (hipSetDevice(h->cfg.device) != hipSuccess) return RR_ERR_HIP;
  if (hipStreamSynchronize(h->last_stream) != hipSuccess) return fail(h, RR_ERR_HIP, "stream sync failed");
  const std::string n = name;
  if (n == "text_hidden") {
    if (!h->tap_text) return fail(h, RR_ERR_BAD_ARG, "text_hidden tap needs rr_set_debug(1) before rr_forward");
    if ((int64_t)h->tap_text_elems > max_elems) return fail(h, RR_ERR_BAD_SHAPE, "buffer too small");
    if (hipMemcpy(host_out, h->tap_text, h->tap_text_elems * 4, hipMemcpyDeviceToHost) != hipSuccess) return RR_ERR_HIP;
    return (int64_t)h->tap_text_elems;
  }
  if (n == "ce_hidden") {
    if (!h->tap_ce || (int64_t)h->tap_ce_elems > max_elems) return fail(h, RR_ERR_BAD_SHAPE, "no tap / buffer too small");
    if (hipMemcpy(host_out, h->tap_ce, h->tap_ce_elems * 4, hipMemcpyDeviceToHost) != hipSuccess) return RR_ERR_HIP;
    return (int64_t)h->tap_ce_elems;
  }
  if (n == "late_interaction") {
    if (!h->tap_li || (int64_t)h->tap_li_elems > max_elems) return fail(h, RR_ERR_BAD_SHAPE, "no tap / buffer too small");
    std::vector<uint16_t> t(h->tap_li_elems);
    if (hipMemcpy(t.data(), h->tap_li, t.size() * 2, hipMemcpyDeviceToHost) != hipSuccess) return RR_ERR_HIP;
    for (size_t i = 0; i < t.size(); ++i) host_out[i] = h->dt ? host_h2f(t[i]) : host_bf2f(t[i]);
    return (int64_t)t.size();
  }
  return fail(h, RR_ERR_BAD_ARG, "unknown tap %s", name);
}

int rr_set_debug(rr_handle h, int on) {
  if (!h) return RR_ERR_BAD_ARG;
  h->debug = on != 0;
  return RR_OK;
}

int rr_set_profiling(rr_handle h, int on) {
  if (!h) return RR_ERR_BAD_ARG;
  h->profiling = on != 0;
  return RR_OK;
}

static int rr_get_profile_impl(rr_handle h, rr_profile* out, int reset) {
  if (!h || !out) return RR_ERR_BAD_ARG;
  RR_HIP(h, hipSetDevice(h->cfg.device));
  for (size_t i = 0; i < h->ev_used; ++i) {
    ProfEvent& e = h->ev_pool[i];
    RR_HIP(h, hipEventSynchronize(e.b));
    float ms = 0.f;
    RR_HIP(h, hipEventElapsedTime(&ms, e.start >= 0 ? h->ev_pool[e.start].b : e.a, e.b));
    h->prof.ms[e.kclass] += ms;
  }
  h->ev_used = 0;
  *out = h->prof;
  if (reset) h->prof = rr_profile{};
  return RR_OK;
}

// ---- per-handle numerics options ---------------------------------------------------------------
static int option_index(const char* key) {
  if (!key) return -1;
  for (int i = 0; i < RR_OPT_COUNT; ++i)
    if (!strcmp(key, kOptionKeys[i])) return i;
  return -1;
}
extern "C" int rr_get_attn_fixed_ref(void);
int rr_set_option(rr_handle h, const char* key, int value) {
  if (!h) return RR_ERR_BAD_ARG;
  return guarded(h, [&]() -> int {
    const int i = option_index(key);
    if (i < 0) return fail(h, RR_ERR_BAD_ARG, "rr_set_option: unknown key '%s'", key ? key : "(null)");
    if (value < -1 || value > option_max(i))
      return fail(h, RR_ERR_BAD_ARG, "rr_set_option: %s = %d out of range", key, value);
    if (i == RR_OPT_Q8_FORMAT && h->q8_fmt >= 0 && (value < 0 ? g_q8_format : value) != h->q8_fmt)
      return fail(h, RR_ERR_BAD_ARG, "rr_set_option: q8_format is latched by rr_finalize_weights (the weights are packed as %s)",
                  h->q8_fmt ? "int8" : "e4m3");
    if (h->cfg.fp8 && value == 1 && ((i == RR_OPT_FP8_FFN_DOWN && opt_of(h, RR_OPT_Q8_FORMAT) == 1) ||
                                     (i == RR_OPT_Q8_FORMAT && opt_of(h, RR_OPT_FP8_FFN_DOWN) == 1)))
      return fail(h, RR_ERR_BAD_ARG, "rr_set_option: fp8_ffn_down = 1 needs q8_format 0 (there is no int8 FFN-down)");
    h->opt[i] = value;
    return RR_OK;
  });
}
int rr_get_option(rr_handle h, const char* key, int* value_out) {
  if (!h || !value_out) return RR_ERR_BAD_ARG;
  return guarded(h, [&]() -> int {
    const int i = option_index(key);
    if (i < 0) return fail(h, RR_ERR_BAD_ARG, "rr_get_option: unknown key '%s'", key ? key : "(null)");
    // the EFFECTIVE value: opt_of keeps -1 for an unpinned "attn_fixed_ref" (the launcher then takes its process-wide mode);
    // a reader is shown that mode
    const int v = opt_of(h, i);
    *value_out = (i == RR_OPT_ATTN_FIXED_REF && v < 0) ? rr_get_attn_fixed_ref()
                 : i == RR_OPT_FP8_FIRST_LAYER ? fp8_first_layer_of(v, h->cfg.layers, opt_of(h, RR_OPT_Q8_FORMAT) == 1)
                 : i == RR_OPT_RESID_LO8 ? (int)resid_lo8_of(v, h->dt) : v;
    return RR_OK;
  });
}

// ---- stand-alone operators ---------------------------------------------------------------------
int rr_set_tuning(const char* key, int value) {
  if (!key) return RR_ERR_BAD_ARG;
  if (!strcmp(key, "ln_lite")) { g_ln_lite = value != 0; return RR_OK; }
  if (!strcmp(key, "ln_fold")) { g_ln_fold = value != 0; return RR_OK; }
  if (!strcmp(key, "fp8_ffn_down")) { g_fp8_ffn_down = value != 0; return RR_OK; }
  if (!strcmp(key, "fp8_first_layer")) { g_fp8_first_layer = value < 0 ? -1 : value; return RR_OK; }
  if (!strcmp(key, "fp8_qkv")) { g_fp8_qkv = value != 0; return RR_OK; }
  if (!strcmp(key, "q8_format")) { if (value < 0 || value > 1) return RR_ERR_BAD_ARG; g_q8_format = value; return RR_OK; }
  if (!strcmp(key, "q8_smooth")) { g_q8_smooth = value != 0; return RR_OK; }
  if (!strcmp(key, "ce_cls_only")) { g_ce_cls_only = value != 0; return RR_OK; }
  if (!strcmp(key, "persistent_gemm")) return rr_set_gemm_persistent(value);
  if (!strcmp(key, "resid_touch")) return rr_set_resid_touch(value);
  if (!strcmp(key, "resid_split")) return rr_set_resid_split(value);
  if (!strcmp(key, "resid_lo8")) { g_resid_lo8 = value < 0 ? resid_lo8_default() : (value != 0); return RR_OK; }
  if (!strcmp(key, "resid_fast")) return rr_set_resid_fast(value);
  if (!strcmp(key, "gemm_ring_min_tiles")) return rr_set_gemm_ring_min_tiles(value) == 0 ? RR_OK : RR_ERR_BAD_ARG;
  if (!strcmp(key, "gemm_small_half_rows")) { rr_set_gemm_small_half_rows(value); return RR_OK; }
  if (!strcmp(key, "gemm_grid_cus")) { rr_set_gemm_grid_cus(value); return RR_OK; }
  if (!strcmp(key, "gemm_desync")) return rr_set_gemm_desync(value) == 0 ? RR_OK : RR_ERR_BAD_ARG;
  if (!strcmp(key, "m_alternate")) return rr_set_m_alternate(value);
  if (!strcmp(key, "li_lds_kb")) return rr_set_li_lds_kb(value) == 0 ? RR_OK : RR_ERR_BAD_ARG;
  if (!strcmp(key, "search_chunk")) return rr_set_search_chunk(value) == 0 ? RR_OK : RR_ERR_BAD_ARG;
  if (!strcmp(key, "bank_move_kb")) return rr_set_bank_move_kb(value) == 0 ? RR_OK : RR_ERR_BAD_ARG;
  if (!strcmp(key, "compress_chunk")) return rr_set_compress_chunk(value) == 0 ? RR_OK : RR_ERR_BAD_ARG;
  if (!strcmp(key, "compress_stop_after")) return rr_set_compress_stop_after(value) == 0 ? RR_OK : RR_ERR_BAD_ARG;
  if (!strcmp(key, "kmeans_stop_after")) return rr_set_kmeans_stop_after(value) == 0 ? RR_OK : RR_ERR_BAD_ARG;
  if (!strcmp(key, "plaid_stop_after")) return set_plaid_stop_after(false, value);
  if (!strcmp(key, "plaid_ivf_stop_after")) return set_plaid_stop_after(true, value);
  if (!strcmp(key, "sparse_stop_after")) return set_sparse_stop_after(value);
  if (!strcmp(key, "f16_stop_after")) return set_f16_stop_after(value);
  if (!strcmp(key, "attn_prio")) return rr_set_attn_prio(value);
  if (!strcmp(key, "attn_fixed_ref")) return rr_set_attn_fixed_ref(value);
  return RR_ERR_BAD_ARG;
}

static int g_op_dt = 0;   // operand dtype used by the stand-alone rr_op_* entry points (rr_set_op_dtype)
int rr_set_op_dtype(int dt) {
  if (dt != 0 && dt != 1) return RR_ERR_BAD_ARG;
  g_op_dt = dt;
  return RR_OK;
}

static int rr_op_gemm_bf16_impl(const uint16_t* A, const uint16_t* W, const float* bias, int M, int N, int Kd, int epilogue,
                    void* out, void* hip_stream) {
  if (!A || !W || !out) return RR_ERR_BAD_ARG;
  if (epilogue < 0 || epilogue > 5 || epilogue == 4) return RR_ERR_BAD_ARG;   // 4 (residual) has its own entry point
  const int epi_map[6] = {EPI_BIAS_BF16, EPI_BIAS_GELU_BF16, EPI_BIAS_F32, EPI_BIAS_TANH_BF16, -1, EPI_BIAS_QGELU_BF16};
  hipError_t e = rr_launch_gemm(A, Kd, W, Kd, bias, nullptr, 0, out, N, M, N, Kd, epi_map[epilogue], g_op_dt, (hipStream_t)hip_stream);
  return e == hipSuccess ? RR_OK : (e == hipErrorInvalidValue ? RR_ERR_BAD_SHAPE : RR_ERR_HIP);
}

static int rr_op_gemm_fp8_impl(const uint8_t* A8, const uint8_t* W8, const float* bias, float scale, int M, int N, int K, int epilogue,
                   void* out, void* hip_stream) {
  if (!A8 || !W8 || !out) return RR_ERR_BAD_ARG;
  if (epilogue < 0 || epilogue > 2) return RR_ERR_BAD_ARG;
  hipError_t e = rr_launch_gemm_fp8(A8, K, W8, K, bias, scale, nullptr, nullptr, out, N, M, N, K, epilogue, g_op_dt, (hipStream_t)hip_stream);
  return e == hipSuccess ? RR_OK : (e == hipErrorInvalidValue ? RR_ERR_BAD_SHAPE : RR_ERR_HIP);
}

static int rr_op_gemm_fp8_rc_impl(const uint8_t* A8, const uint8_t* W8, const float* bias, const float* row_scale,
                                  const float* col_scale, int M, int N, int K, int epilogue, void* out, void* hip_stream) {
  if (!A8 || !W8 || !out) return RR_ERR_BAD_ARG;
  if (epilogue < 0 || epilogue > 2) return RR_ERR_BAD_ARG;
  hipError_t e = rr_launch_gemm_fp8(A8, K, W8, K, bias, 1.0f, row_scale, col_scale, out, N, M, N, K, epilogue, g_op_dt,
                                    (hipStream_t)hip_stream);
  return e == hipSuccess ? RR_OK : (e == hipErrorInvalidValue ? RR_ERR_BAD_SHAPE : RR_ERR_HIP);
}
static int rr_op_gemm_fp8_gelu_e4m3_impl(const uint8_t* A8, const uint8_t* W8, const float* bias, const float* row_scale,
                                         const float* col_scale, float out_mul, int M, int N, int K, uint8_t* out8, void* hip_stream) {
  if (!A8 || !W8 || !out8) return RR_ERR_BAD_ARG;
  hipError_t e = rr_launch_gemm_fp8(A8, K, W8, K, bias, 1.0f, row_scale, col_scale, out8, N, M, N, K, 3, g_op_dt, (hipStream_t)hip_stream,
                                    out_mul);
  return e == hipSuccess ? RR_OK : (e == hipErrorInvalidValue ? RR_ERR_BAD_SHAPE : RR_ERR_HIP);
}
static int rr_op_gemm_fp8_resid_impl(const uint8_t* A8, const uint8_t* W8, const float* bias, float scale, const float* col_scale,
                                     const float* resid, const float* stats, const float* gamma, const float* beta, int M, int N,
                                     int K, float* out, void* hip_stream) {
  if (!A8 || !W8 || !out || !resid) return RR_ERR_BAD_ARG;
  hipError_t e = rr_launch_gemm_fp8(A8, K, W8, K, bias, scale, nullptr, col_scale, out, N, M, N, K, 4, g_op_dt, (hipStream_t)hip_stream,
                                    1.0f, resid, N, stats, gamma, beta);
  return e == hipSuccess ? RR_OK : (e == hipErrorInvalidValue ? RR_ERR_BAD_SHAPE : RR_ERR_HIP);
}
static int rr_op_layernorm_q8_impl(const float* x, const float* gamma, const float* beta, float eps, int rows, int cols,
                                   uint8_t* out8, float* row_scale, float* stats, void* hip_stream) {
  if (!x || !gamma || !beta || !out8 || !row_scale) return RR_ERR_BAD_ARG;
  hipError_t e = rr_launch_layernorm_q8(x, gamma, beta, eps, rows, cols, out8, row_scale, stats, (hipStream_t)hip_stream);
  return e == hipSuccess ? RR_OK : (e == hipErrorInvalidValue ? RR_ERR_BAD_SHAPE : RR_ERR_HIP);
}
static int rr_op_gemm_i8_rc_impl(const int8_t* A8, const int8_t* W8, const float* bias, const float* row_scale,
                                 const float* col_scale, int M, int N, int K, int epilogue, void* out, void* hip_stream) {
  if (!A8 || !W8 || !out) return RR_ERR_BAD_ARG;
  if (epilogue < 0 || epilogue > 2) return RR_ERR_BAD_ARG;
  hipError_t e = rr_launch_gemm_i8(A8, K, W8, K, bias, 1.0f, row_scale, col_scale, out, N, M, N, K, epilogue, g_op_dt,
                                   (hipStream_t)hip_stream);
  return e == hipSuccess ? RR_OK : (e == hipErrorInvalidValue ? RR_ERR_BAD_SHAPE : RR_ERR_HIP);
}
static int rr_op_layernorm_i8_impl(const float* x, const float* gamma, const float* beta, float eps, int rows, int cols,
                                   int8_t* out8, float* row_scale, float* stats, void* hip_stream) {
  if (!x || !gamma || !beta || !out8 || !row_scale) return RR_ERR_BAD_ARG;
  hipError_t e = rr_launch_layernorm_i8(x, gamma, beta, eps, rows, cols, out8, row_scale, stats, (hipStream_t)hip_stream);
  return e == hipSuccess ? RR_OK : (e == hipErrorInvalidValue ? RR_ERR_BAD_SHAPE : RR_ERR_HIP);
}
static int rr_op_quantize_fp8_impl(const void* x, int x_is_f32, float scale, uint8_t* out, size_t n, void* hip_stream) {
  if (!x || !out) return RR_ERR_BAD_ARG;
  hipError_t e = rr_launch_quant_e4m3(x, x_is_f32, scale, out, n, (hipStream_t)hip_stream);
  return e == hipSuccess ? RR_OK : (e == hipErrorInvalidValue ? RR_ERR_BAD_SHAPE : RR_ERR_HIP);
}

static int rr_op_amax_impl(const void* x, int x_is_f32, size_t n, float* out_dev, void* hip_stream) {
  if (!x || !out_dev) return RR_ERR_BAD_ARG;
  hipError_t e = rr_launch_amax(x, x_is_f32, n, out_dev, (hipStream_t)hip_stream);
  return e == hipSuccess ? RR_OK : (e == hipErrorInvalidValue ? RR_ERR_BAD_SHAPE : RR_ERR_HIP);
}

static int rr_op_gemm_resid_f32_impl(const uint16_t* A, const uint16_t* W, const float* bias, const float* resid, int M, int N,
                         int Kd, float* out, void* hip_stream) {
  if (!A || !W || !out || !resid) return RR_ERR_BAD_ARG;
  hipError_t e = rr_launch_gemm(A, Kd, W, Kd, bias, resid, N, out, N, M, N, Kd, EPI_BIAS_RESID_F32, g_op_dt, (hipStream_t)hip_stream);
  return e == hipSuccess ? RR_OK : (e == hipErrorInvalidValue ? RR_ERR_BAD_SHAPE : RR_ERR_HIP);
}

static int rr_op_attention_ex_impl(const uint16_t* q, const uint16_t* k, const uint16_t* v, int q_stride, int kv_stride,
                                   const float* key_bias, int B, int heads, int Tq, int Tk, int q_batch_div, int q_batch_off,
                                   uint16_t* out, int out_stride, const float* dense_bias, int dense_ld, int64_t schedule_blocks,
                                   int fixed_mode, void* hip_stream) {
  if (!q || !k || !v || !out) return RR_ERR_BAD_ARG;
  hipError_t e = rr_launch_attention(q, q_stride, q_batch_div, q_batch_off, k, v, kv_stride, key_bias, B, heads, Tq, Tk, out,
                                     out_stride, g_op_dt, (hipStream_t)hip_stream, dense_bias, dense_ld, (long)schedule_blocks,
                                     fixed_mode);
  return e == hipSuccess ? RR_OK : (e == hipErrorInvalidValue ? RR_ERR_BAD_SHAPE : RR_ERR_HIP);
}

static int rr_op_attention_segs_impl(const uint16_t* q, int q_stride, const uint16_t* k, const uint16_t* v, int kv_stride,
                                     const float* key_bias, int heads, int nseg, const int* seg_n, const int* seg_len,
                                     const int64_t* seg_row0, uint16_t* out, int out_stride, int64_t schedule_blocks, int fixed_mode,
                                     void* hip_stream) {
  if (!q || !k || !v || !out || !seg_n || !seg_len || !seg_row0 || nseg <= 0) return RR_ERR_BAD_ARG;
  const std::vector<long long> row0(seg_row0, seg_row0 + nseg);
  hipError_t e = rr_launch_attention_segs(q, q_stride, k, v, kv_stride, key_bias, heads, nseg, seg_n, seg_len, row0.data(), out,
                                          out_stride, g_op_dt, (hipStream_t)hip_stream, (long)schedule_blocks, fixed_mode);
  return e == hipSuccess ? RR_OK : (e == hipErrorInvalidValue ? RR_ERR_BAD_SHAPE : RR_ERR_HIP);
}

static int rr_op_fusion_adj_impl(const float* scores, int S, int Tq, int Tc, float mult, int pair0, int n, float* adj, int ld,
                                 int row0, void* hip_stream) {
  if (!scores || !adj) return RR_ERR_BAD_ARG;
  hipError_t e = rr_launch_fusion_adj(scores, S, Tq, Tc, mult, pair0, n, adj, ld, (hipStream_t)hip_stream, row0);
  return e == hipSuccess ? RR_OK : (e == hipErrorInvalidValue ? RR_ERR_BAD_SHAPE : RR_ERR_HIP);
}

static int rr_op_fusion_adj_segs_impl(const float* scores, int S, int Tq, int Tc, float mult, int nseg, const int* seg_n,
                                      const int* seg_tk, float* adj, int row0, void* hip_stream) {
  if (!scores || !adj || !seg_n || !seg_tk) return RR_ERR_BAD_ARG;
  hipError_t e = rr_launch_fusion_adj_segs(scores, S, Tq, Tc, mult, nseg, seg_n, seg_tk, adj, (hipStream_t)hip_stream, row0);
  return e == hipSuccess ? RR_OK : (e == hipErrorInvalidValue ? RR_ERR_BAD_SHAPE : RR_ERR_HIP);
}

static int rr_op_gemm_ln_resid_f32_impl(const uint16_t* A, const uint16_t* W, const float* bias, const float* x, const float* stats,
                            const float* gamma, const float* beta, int M, int N, int Kd, float* out, void* hip_stream) {
  if (!A || !W || !out || !x || !stats || !gamma || !beta) return RR_ERR_BAD_ARG;
  hipError_t e = rr_launch_gemm_ln(A, Kd, W, Kd, bias, x, N, stats, gamma, beta, out, N, M, N, Kd, EPI_BIAS_RESID_F32, g_op_dt,
                                   (hipStream_t)hip_stream);
  return e == hipSuccess ? RR_OK : (e == hipErrorInvalidValue ? RR_ERR_BAD_SHAPE : RR_ERR_HIP);
}
/* The two halves of the folded LayerNorm, stand-alone for the operator tests. */
static int rr_op_gemm_resid_lnprep_impl(const uint16_t* A, const uint16_t* W, const float* bias, const float* resid, int M, int N,
                                        int Kd, float eps, float* out_f32, uint16_t* x16_out, float* stats_out,
                                        float* part_scratch, void* hip_stream) {
  if (!A || !W || !resid || !out_f32 || !x16_out || !stats_out || !part_scratch) return RR_ERR_BAD_ARG;
  GemmFold f;
  f.x16 = x16_out;
  f.ldx = N;
  f.part = part_scratch;
  f.nparts = (N + 127) / 128;
  hipError_t e = rr_launch_gemm_fold(A, Kd, W, Kd, bias, resid, N, nullptr, nullptr, nullptr, f, out_f32, N, M, N, Kd,
                                     EPI_BIAS_RESID_F32, g_op_dt, (hipStream_t)hip_stream);
  if (e == hipSuccess) e = rr_launch_ln_finalize(part_scratch, f.nparts, N, eps, M, stats_out, (hipStream_t)hip_stream);
  return e == hipSuccess ? RR_OK : (e == hipErrorInvalidValue ? RR_ERR_BAD_SHAPE : RR_ERR_HIP);
}
/* The residual epilogue on the split stream: residual rows (hi, lo) [+ LayerNorm from (stats, gamma, beta)] in, output rows
 * (x16_out, lo_out) + statistics out; in-place use (hi_in == x16_out, lo_in == lo_out) is what the forward does. */
static int rr_op_gemm_resid_split_impl(const uint16_t* A, const uint16_t* W, const float* bias, const uint16_t* hi_in,
                                       const uint16_t* lo_in, const float* ln_stats, const float* ln_gamma, const float* ln_beta,
                                       int M, int N, int Kd, float eps, uint16_t* x16_out, uint16_t* lo_out, float* stats_out,
                                       float* part_scratch, void* hip_stream) {
  if (!A || !W || !hi_in || !lo_in || !x16_out || !lo_out || !stats_out || !part_scratch) return RR_ERR_BAD_ARG;
  if (!rr_gemm_split_ok(M, N)) return RR_ERR_UNSUPPORTED;      // shapes the persistent ring kernel does not run
  GemmFold f;
  f.x16 = x16_out;
  f.ldx = N;
  f.part = part_scratch;
  f.nparts = (N + 127) / 128;
  f.r_hi = hi_in;
  f.r_lo = lo_in;
  f.ld16 = N;
  f.lo_out = lo_out;
  f.lo_bits = resid_lo8_of(g_resid_lo8, g_op_dt) ? 8 : 16;     // process-wide "resid_lo8": lo_in / lo_out are then e5m2 BYTES in the paired-row layout
  hipError_t e = rr_launch_gemm_fold(A, Kd, W, Kd, bias, nullptr, 0, ln_stats, ln_gamma, ln_beta, f, nullptr, N, M, N, Kd,
                                     EPI_BIAS_RESID_F32, g_op_dt, (hipStream_t)hip_stream);
  if (e == hipSuccess) e = rr_launch_ln_finalize(part_scratch, f.nparts, N, eps, M, stats_out, (hipStream_t)hip_stream);
  return e == hipSuccess ? RR_OK : (e == hipErrorInvalidValue ? RR_ERR_BAD_SHAPE : RR_ERR_HIP);
}
static int rr_op_gemm_lnfold_impl(const uint16_t* A_raw, const uint16_t* W_folded, const float* dvec, const float* csum,
                                  const float* stats, int M, int N, int Kd, int epilogue, void* out, void* hip_stream) {
  if (!A_raw || !W_folded || !csum || !stats || !out) return RR_ERR_BAD_ARG;
  if (epilogue < 0 || epilogue > 2) return RR_ERR_BAD_ARG;
  GemmFold f;
  f.in_stats = stats;
  f.csum = csum;
  const int epi_map[3] = {EPI_BIAS_BF16, EPI_BIAS_GELU_BF16, EPI_BIAS_F32};
  hipError_t e = rr_launch_gemm_fold(A_raw, Kd, W_folded, Kd, dvec, nullptr, 0, nullptr, nullptr, nullptr, f, out, N, M, N, Kd,
                                     epi_map[epilogue], g_op_dt, (hipStream_t)hip_stream);
  return e == hipSuccess ? RR_OK : (e == hipErrorInvalidValue ? RR_ERR_BAD_SHAPE : RR_ERR_HIP);
}
static int rr_op_split_residual_value_impl(const uint16_t* hi, const uint16_t* lo, const float* stats, const float* gamma,
                                           const float* beta, int rows, int cols, float* out, void* hip_stream) {
  if (!hi || !lo || !out) return RR_ERR_BAD_ARG;
  hipError_t e = rr_launch_split_residual_value(hi, lo, stats, gamma, beta, rows, cols, g_op_dt, out, (hipStream_t)hip_stream);
  return e == hipSuccess ? RR_OK : (e == hipErrorInvalidValue ? RR_ERR_BAD_SHAPE : RR_ERR_HIP);
}
static int rr_op_layernorm_stats_impl(const float* x, const float* gamma, const float* beta, float eps, int rows, int cols,
                          float* out_f32, uint16_t* out_bf16, float* stats, void* hip_stream) {
  if (!x || !gamma || !beta || !out_bf16 || !stats) return RR_ERR_BAD_ARG;
  hipError_t e = rr_launch_layernorm_stats(x, gamma, beta, eps, rows, cols, out_f32, out_bf16, stats, g_op_dt, (hipStream_t)hip_stream);
  return e == hipSuccess ? RR_OK : (e == hipErrorInvalidValue ? RR_ERR_BAD_SHAPE : RR_ERR_HIP);
}
static int rr_op_layernorm_impl(const float* x, const float* gamma, const float* beta, float eps, int rows, int cols,
                    float* out_f32, uint16_t* out_bf16, void* hip_stream) {
  if (!x || !gamma || !beta || (!out_f32 && !out_bf16)) return RR_ERR_BAD_ARG;
  hipError_t e = rr_launch_layernorm(x, gamma, beta, eps, rows, cols, out_f32, out_bf16, g_op_dt, (hipStream_t)hip_stream);
  return e == hipSuccess ? RR_OK : (e == hipErrorInvalidValue ? RR_ERR_BAD_SHAPE : RR_ERR_HIP);
}

// ---- row and glue kernels of elementwise.hip, stand-alone.  Several launchers validate nothing, and several kernels add a row
// offset to an output pointer before testing it; these checks stand in front of them, and a failed one launches nothing.
static bool op_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
static bool op_row_cols(int cols) { return cols > 0 && (cols & 3) == 0 && cols <= 2048; }   // one wave per row, MAX_V4 = 8
static int op_status(hipError_t e) { return e == hipSuccess ? RR_OK : (e == hipErrorInvalidValue ? RR_ERR_BAD_SHAPE : RR_ERR_HIP); }

static int rr_op_embed_ln_impl(const int64_t* ids, const int64_t* tts, const float* word, const float* pos, const float* type,
                               const float* gamma, const float* beta, float eps, int rows, int S, int cols, int vocab,
                               int type_vocab, float* out_f32, uint16_t* out16, void* hip_stream) {
  if (!ids || !word || !pos || !type || !gamma || !beta || !out_f32 || !out16) return RR_ERR_BAD_ARG;
  for (const void* p : {(const void*)word, (const void*)pos, (const void*)type, (const void*)gamma, (const void*)beta,
                        (const void*)out_f32})
    if (!op_aligned(p, 16)) return RR_ERR_BAD_ARG;
  if (!op_aligned(out16, 8)) return RR_ERR_BAD_ARG;
  if (rows <= 0 || S <= 0 || vocab <= 0 || type_vocab <= 0 || !op_row_cols(cols)) return RR_ERR_BAD_SHAPE;
  return op_status(rr_launch_embed_ln(ids, tts, word, pos, type, gamma, beta, eps, rows, S, cols, vocab, type_vocab, out_f32, out16,
                                      g_op_dt, (hipStream_t)hip_stream));
}
static int rr_op_ce_embed_ln_impl(const float* x, const float* pos, const float* type0, const float* gamma, const float* beta,
                                  float eps, int rows, int T, int cols, float* out_f32, uint16_t* out16, int s_text, int vis_pos0,
                                  int cls32, void* hip_stream) {
  if (!x || !pos || !type0 || !gamma || !beta || !out_f32 || !out16) return RR_ERR_BAD_ARG;
  for (const void* p : {(const void*)x, (const void*)pos, (const void*)type0, (const void*)gamma, (const void*)beta,
                        (const void*)out_f32})
    if (!op_aligned(p, 16)) return RR_ERR_BAD_ARG;
  if (!op_aligned(out16, 8)) return RR_ERR_BAD_ARG;
  if (rows <= 0 || T <= 0 || vis_pos0 < 0 || !op_row_cols(cols)) return RR_ERR_BAD_SHAPE;
  return op_status(rr_launch_ce_embed_ln(x, pos, type0, gamma, beta, eps, rows, T, cols, out_f32, out16, g_op_dt,
                                         (hipStream_t)hip_stream, s_text, vis_pos0, cls32));
}
static int rr_op_li_normalize_impl(const float* src, const int64_t* ids, int ids_stride, int n_pairs, int rows_per_batch, int D,
                                   int T, int t_off, int pair_off, int bdiv, int src_batch_off, uint16_t* dst, int normalize,
                                   const float* maskf, int split, int shift, void* hip_stream) {
  if (!src || !dst || !op_aligned(src, 16) || !op_aligned(dst, 8)) return RR_ERR_BAD_ARG;
  if (n_pairs <= 0 || rows_per_batch <= 0 || !op_row_cols(D) || T <= 0 || bdiv <= 0 || t_off < 0 || pair_off < 0 ||
      src_batch_off < 0 || pair_off / bdiv < src_batch_off || split < 0 || shift < 0 || (ids && ids_stride < rows_per_batch))
    return RR_ERR_BAD_SHAPE;
  const int j = rows_per_batch - 1;                       // the last destination row of a pair lies inside its T rows
  if ((long long)t_off + j + (j >= split ? shift : 0) >= T) return RR_ERR_BAD_SHAPE;
  return op_status(rr_launch_li_normalize(src, ids, ids_stride, n_pairs, rows_per_batch, D, T, t_off, pair_off, bdiv, src_batch_off,
                                          dst, g_op_dt, normalize, maskf, split, shift, (hipStream_t)hip_stream));
}
static int rr_op_key_bias_impl(const int64_t* ids, const int64_t* am, int n, int S, int T, float* text_bias, float* ce_bias,
                               void* hip_stream) {
  if (!ids || !am || !text_bias || !ce_bias) return RR_ERR_BAD_ARG;
  if (n <= 0 || S <= 0 || T < S || (long long)n * T > INT_MAX) return RR_ERR_BAD_SHAPE;
  return op_status(rr_launch_key_bias(ids, am, n, S, T, text_bias, ce_bias, (hipStream_t)hip_stream));
}
static int rr_op_joint_masks_impl(const int64_t* ids, const int64_t* am, int n, int S, int P, int q_len, int64_t instruction_token,
                                  float* text_bias, float* li_mask, float* ce_bias, void* hip_stream) {
  if (!ids || !am || !text_bias || !li_mask || !ce_bias) return RR_ERR_BAD_ARG;
  if (n <= 0 || S <= 0 || P < 0 || q_len < 0 || q_len > S) return RR_ERR_BAD_SHAPE;
  return op_status(rr_launch_joint_masks(ids, am, n, S, P, q_len, (long long)instruction_token, text_bias, li_mask, ce_bias,
                                         (hipStream_t)hip_stream));
}
static int rr_op_interaction_bias_impl(const float* qmask, const float* cmask, int n, int Lq, int Lc, int pair_off, int K,
                                       float* cat_bias, float* q_bias, float* c_bias, void* hip_stream) {
  if (!qmask || !cmask) return RR_ERR_BAD_ARG;
  if (n <= 0 || Lq <= 0 || Lc <= 0 || K <= 0 || pair_off < 0 || (long long)n * (Lq + Lc) > INT_MAX) return RR_ERR_BAD_SHAPE;
  return op_status(rr_launch_interaction_bias(qmask, cmask, n, Lq, Lc, pair_off, K, cat_bias, q_bias, c_bias,
                                              (hipStream_t)hip_stream));
}
static int rr_op_vit_im2col_impl(const float* px, uint16_t* out, int B, int IS, int ps, int Kp, void* hip_stream) {
  if (!px || !out) return RR_ERR_BAD_ARG;
  if (B <= 0 || ps <= 0 || IS < ps || Kp < 3 * ps * ps) return RR_ERR_BAD_SHAPE;
  return op_status(rr_launch_vit_im2col(px, out, B, IS, ps, Kp, g_op_dt, (hipStream_t)hip_stream));
}
static int rr_op_vit_embed_ln_impl(const float* patches, const float* cls_emb, const float* pos, const float* gamma, const float* beta,
                                   float eps, int rows, int T, int cols, float* out_f32, void* hip_stream) {
  if (!patches || !cls_emb || !pos || !gamma || !beta || !out_f32) return RR_ERR_BAD_ARG;
  for (const void* p : {(const void*)patches, (const void*)cls_emb, (const void*)pos, (const void*)gamma, (const void*)beta,
                        (const void*)out_f32})
    if (!op_aligned(p, 16)) return RR_ERR_BAD_ARG;
  if (rows <= 0 || T <= 0 || !op_row_cols(cols)) return RR_ERR_BAD_SHAPE;
  return op_status(rr_launch_vit_embed_ln(patches, cls_emb, pos, gamma, beta, eps, rows, T, cols, out_f32, (hipStream_t)hip_stream));
}
static int rr_op_cast16_impl(const float* x, uint16_t* y, int64_t n, void* hip_stream) {
  if (!x || !y || !op_aligned(x, 16) || !op_aligned(y, 8)) return RR_ERR_BAD_ARG;
  if (n <= 0 || (n & 3)) return RR_ERR_BAD_SHAPE;
  return op_status(rr_launch_f32_to_bf16(x, y, (size_t)n, g_op_dt, (hipStream_t)hip_stream));
}
static int rr_op_gather_rows_impl(const void* src, void* dst, int n_dst_batches, int rows_take, int src_rows_per_batch, int row_bytes,
                                  int batch_off, int bdiv, int src_batch_off, void* hip_stream) {
  if (!src || !dst || !op_aligned(src, 16) || !op_aligned(dst, 16)) return RR_ERR_BAD_ARG;
  if (n_dst_batches <= 0 || rows_take <= 0 || src_rows_per_batch < rows_take || row_bytes <= 0 || (row_bytes & 15) || bdiv <= 0 ||
      batch_off < 0 || src_batch_off < 0 || batch_off / bdiv < src_batch_off)
    return RR_ERR_BAD_SHAPE;
  return op_status(rr_launch_gather_rows(src, dst, n_dst_batches, rows_take, src_rows_per_batch, row_bytes, batch_off, bdiv,
                                         src_batch_off, (hipStream_t)hip_stream));
}
static int rr_op_cls_heads_impl(const float* h32, int T, int cols, int n_pairs, const float* w1, const float* b1, const float* w2,
                                const float* b2, float* out1, float* out2, void* hip_stream) {
  if (!h32 || !w1 || !b1 || !w2 || !out1 || (out2 && !b2)) return RR_ERR_BAD_ARG;
  if (!op_aligned(h32, 16) || !op_aligned(w1, 16) || !op_aligned(w2, 16)) return RR_ERR_BAD_ARG;
  if (T <= 0 || n_pairs <= 0 || cols <= 0 || (cols & 3)) return RR_ERR_BAD_SHAPE;
  return op_status(rr_launch_cls_heads(h32, T, cols, n_pairs, w1, b1, w2, b2, out1, out2, (hipStream_t)hip_stream));
}
static int rr_op_ln_finalize_impl(const float* part, int nparts, int cols, float eps, int rows, float* stats, int* range_flag,
                                  float range_ss, void* hip_stream) {
  if (!part || !stats || !op_aligned(part, 8) || !op_aligned(stats, 8)) return RR_ERR_BAD_ARG;
  if (rows <= 0 || cols <= 0 || nparts != (cols + 127) / 128) return RR_ERR_BAD_SHAPE;
  return op_status(rr_launch_ln_finalize(part, nparts, cols, eps, rows, stats, (hipStream_t)hip_stream, range_flag, range_ss));
}


// ---- the exported entry points: bodies above, run through guarded() so that no C++ exception crosses the ABI
int rr_create(const rr_config* cfg, rr_handle* out) {
  return guarded(nullptr, [&]() -> int { return rr_create_impl(cfg, out); });
}
int rr_destroy(rr_handle h) {
  return guarded(h, [&]() -> int { return rr_destroy_impl(h); });
}
int rr_load_weight(rr_handle h, const char* name, const void* data, int dtype, int ndim, const int64_t* shape, int* known) {
  return guarded(h, [&]() -> int { return rr_load_weight_impl(h, name, data, dtype, ndim, shape, known); });
}
int rr_finalize_weights(rr_handle h) {
  return guarded(h, [&]() -> int { return rr_finalize_weights_impl(h); });
}
int rr_encode_image(rr_handle h, const float* pixel_values, int B, float* image_cls_out, float* image_patches_out, void* hip_stream) {
  return guarded(h, [&]() -> int { return rr_encode_image_impl(h, pixel_values, B, image_cls_out, image_patches_out, hip_stream); });
}
// the forwards: the arguments into one Request (forward_full / forward_interaction)
int rr_head(rr_handle h, const float* logits, const float* logits2, const float* labels, int Bq, int K, float* loss_out, float* scores_out, int32_t* order_out, void* hip_stream) {
  return guarded(h, [&]() -> int { return head_call(h, "rr_head", false, logits, logits2, labels, Bq, K, loss_out, scores_out, order_out, hip_stream); });
}
int rr_head_lists(rr_handle h, const float* logits, const float* logits2, const float* labels, int n_lists, const int32_t* list_offsets, const int32_t* gather, int joint, float* loss_out, float* list_loss_out, float* scores_out, int32_t* order_out, void* hip_stream) {
  return guarded(h, [&]() -> int { return head_lists_call(h, logits, logits2, labels, n_lists, list_offsets, gather, joint, loss_out, list_loss_out, scores_out, order_out, hip_stream); });
}
int rr_head_joint(rr_handle h, const float* logits, const float* logits2, int Bq, int K, float* loss_out, float* scores_out, int32_t* order_out, void* hip_stream) {
  return guarded(h, [&]() -> int { return head_call(h, "rr_head_joint", true, logits, logits2, nullptr, Bq, K, loss_out, scores_out, order_out, hip_stream); });
}
int rr_forward(rr_handle h, const int64_t* input_ids, const int64_t* attention_mask, const int64_t* token_type_ids, const float* image_cls, const float* image_patches, int Bq, int K, int S, const float* labels, int pair_begin, int pair_end, float* logits_out, float* logits2_out, float* loss_out, float* scores_out, int32_t* order_out, void* hip_stream) {
  return guarded(h, [&]() -> int {
    Request r;
    r.ids = input_ids; r.mask = attention_mask; r.token_types = token_type_ids; r.image_cls = image_cls; r.image_patches = image_patches;
    r.Bq = Bq; r.K = K; r.len = S; r.labels = labels; r.pair_begin = pair_begin; r.pair_end = pair_end;
    r.logits = logits_out; r.logits2 = logits2_out; r.loss = loss_out; r.scores = scores_out; r.order = order_out; r.stream = (hipStream_t)hip_stream;
    return forward_full(h, r);
  });
}
int rr_forward_packed(rr_handle h, const int64_t* input_ids, const int64_t* attention_mask, const int64_t* token_type_ids, const float* image_cls, const float* image_patches, int n_segments, const int32_t* seg_pairs, const int32_t* seg_len, int padded_seq_len, float* logits_out, float* logits2_out, void* hip_stream) {
  return guarded(h, [&]() -> int {
    Request r;
    r.ids = input_ids; r.mask = attention_mask; r.token_types = token_type_ids; r.image_cls = image_cls; r.image_patches = image_patches;
    r.packed = true; r.n_segments = n_segments; r.seg_pairs = seg_pairs; r.seg_len = seg_len; r.len = padded_seq_len;
    r.logits = logits_out; r.logits2 = logits2_out; r.stream = (hipStream_t)hip_stream;
    return forward_full(h, r);
  });
}
int rr_assemble_pairs(rr_handle h, const int32_t* pool, int64_t pool_len, const int32_t* desc, int n_pairs, const int32_t* order, int n_segments, const int32_t* seg_pairs, const int32_t* seg_len, int64_t cls_id, int64_t sep_id, int64_t pad_id, int64_t* input_ids, int64_t* attention_mask, int64_t* token_type_ids, void* hip_stream) {
  return guarded(h, [&]() -> int {
    return rr_assemble_pairs_impl(h, pool, pool_len, desc, n_pairs, order, n_segments, seg_pairs, seg_len, cls_id, sep_id, pad_id,
                                  input_ids, attention_mask, token_type_ids, hip_stream);
  });
}
int rr_assemble_joint(rr_handle h, const int32_t* pool, int64_t pool_len, const int32_t* desc, int n_pairs, const int32_t* order, int n_segments, const int32_t* seg_pairs, const int32_t* seg_len, int query_len, int padded_seq_len, int64_t sep_id, int64_t pad_id, int64_t* joint_input_ids, int64_t* joint_attention_mask, void* hip_stream) {
  return guarded(h, [&]() -> int {
    return rr_assemble_joint_impl(h, pool, pool_len, desc, n_pairs, order, n_segments, seg_pairs, seg_len, query_len, padded_seq_len,
                                  sep_id, pad_id, joint_input_ids, joint_attention_mask, hip_stream);
  });
}
int rr_forward_joint(rr_handle h, const int64_t* joint_input_ids, const int64_t* joint_attention_mask, const float* image_cls, const float* image_patches, int Bq, int K, int S, int query_len, int64_t instruction_token_id, int pair_begin, int pair_end, float* logits_out, float* logits2_out, float* loss_out, float* scores_out, int32_t* order_out, void* hip_stream) {
  return guarded(h, [&]() -> int {
    Request r;
    r.family = FAM_JOINT; r.ids = joint_input_ids; r.mask = joint_attention_mask; r.image_cls = image_cls; r.image_patches = image_patches;
    r.Bq = Bq; r.K = K; r.len = S; r.q_len = query_len; r.instruction_token = instruction_token_id; r.pair_begin = pair_begin; r.pair_end = pair_end;
    r.logits = logits_out; r.logits2 = logits2_out; r.loss = loss_out; r.scores = scores_out; r.order = order_out; r.stream = (hipStream_t)hip_stream;
    return forward_full(h, r);
  });
}
int rr_forward_joint_fusion(rr_handle h, const int64_t* joint_input_ids, const int64_t* joint_attention_mask, const float* image_cls, const float* image_patches, const float* preflmr_scores, float fusion_multiplier, int Bq, int K, int S, int query_len, int64_t instruction_token_id, int pair_begin, int pair_end, float* logits_out, float* logits2_out, float* loss_out, float* scores_out, int32_t* order_out, void* hip_stream) {
  return guarded(h, [&]() -> int {
    if (h && !preflmr_scores) return fail(h, RR_ERR_BAD_ARG, "rr_forward_joint_fusion: preflmr_scores is null (use rr_forward_joint)");
    Request r;
    r.family = FAM_JOINT; r.ids = joint_input_ids; r.mask = joint_attention_mask; r.image_cls = image_cls; r.image_patches = image_patches;
    r.fusion_scores = preflmr_scores; r.fusion_mult = fusion_multiplier;
    r.Bq = Bq; r.K = K; r.len = S; r.q_len = query_len; r.instruction_token = instruction_token_id; r.pair_begin = pair_begin; r.pair_end = pair_end;
    r.logits = logits_out; r.logits2 = logits2_out; r.loss = loss_out; r.scores = scores_out; r.order = order_out; r.stream = (hipStream_t)hip_stream;
    return forward_full(h, r);
  });
}
int rr_forward_joint_packed(rr_handle h, const int64_t* joint_input_ids, const int64_t* joint_attention_mask, const float* image_cls, const float* image_patches, const float* preflmr_scores, float fusion_multiplier, int n_segments, const int32_t* seg_pairs, const int32_t* seg_len, int padded_seq_len, int query_len, int64_t instruction_token_id, float* logits_out, float* logits2_out, void* hip_stream) {
  return guarded(h, [&]() -> int {
    Request r;
    r.family = FAM_JOINT; r.ids = joint_input_ids; r.mask = joint_attention_mask; r.image_cls = image_cls; r.image_patches = image_patches;
    r.fusion_scores = preflmr_scores; r.fusion_mult = fusion_multiplier;
    r.packed = true; r.n_segments = n_segments; r.seg_pairs = seg_pairs; r.seg_len = seg_len; r.len = padded_seq_len;
    r.q_len = query_len; r.instruction_token = instruction_token_id;
    r.logits = logits_out; r.logits2 = logits2_out; r.stream = (hipStream_t)hip_stream;
    return forward_full(h, r);
  });
}
int rr_forward_interaction(rr_handle h, const float* query_li, const float* context_li, const float* query_mask, const float* context_mask, int Bq, int K, int Lq, int Lc, const float* labels, int pair_begin, int pair_end, float* logits_out, float* logits2_out, float* loss_out, float* scores_out, int32_t* order_out, void* hip_stream) {
  return guarded(h, [&]() -> int {
    Request r;
    r.family = FAM_INTERACTION; r.query_li = query_li; r.context_li = context_li; r.query_mask = query_mask; r.context_mask = context_mask;
    r.Bq = Bq; r.K = K; r.q_len = Lq; r.len = Lc; r.labels = labels; r.pair_begin = pair_begin; r.pair_end = pair_end;
    r.logits = logits_out; r.logits2 = logits2_out; r.loss = loss_out; r.scores = scores_out; r.order = order_out; r.stream = (hipStream_t)hip_stream;
    return forward_interaction(h, r);
  });
}
int rr_forward_interaction_fusion(rr_handle h, const float* query_li, const float* context_li, const float* query_mask, const float* context_mask, const float* preflmr_scores, float fusion_multiplier, int Bq, int K, int Lq, int Lc, const float* labels, int pair_begin, int pair_end, float* logits_out, float* logits2_out, float* loss_out, float* scores_out, int32_t* order_out, void* hip_stream) {
  return guarded(h, [&]() -> int {
    if (h && !preflmr_scores) return fail(h, RR_ERR_BAD_ARG, "rr_forward_interaction_fusion: preflmr_scores is null");
    Request r;
    r.family = FAM_INTERACTION; r.query_li = query_li; r.context_li = context_li; r.query_mask = query_mask; r.context_mask = context_mask;
    r.fusion_scores = preflmr_scores; r.fusion_mult = fusion_multiplier;
    r.Bq = Bq; r.K = K; r.q_len = Lq; r.len = Lc; r.labels = labels; r.pair_begin = pair_begin; r.pair_end = pair_end;
    r.logits = logits_out; r.logits2 = logits2_out; r.loss = loss_out; r.scores = scores_out; r.order = order_out; r.stream = (hipStream_t)hip_stream;
    return forward_interaction(h, r);
  });
}
int rr_forward_interaction_packed(rr_handle h, const float* query_li, const float* context_li, const float* query_mask, const float* context_mask, const float* preflmr_scores, float fusion_multiplier, int n_segments, const int32_t* seg_pairs, const int32_t* seg_len, int padded_context_len, int Lq, float* logits_out, float* logits2_out, void* hip_stream) {
  return guarded(h, [&]() -> int {
    Request r;
    r.family = FAM_INTERACTION; r.query_li = query_li; r.context_li = context_li; r.query_mask = query_mask; r.context_mask = context_mask;
    r.fusion_scores = preflmr_scores; r.fusion_mult = fusion_multiplier;
    r.packed = true; r.n_segments = n_segments; r.seg_pairs = seg_pairs; r.seg_len = seg_len; r.len = padded_context_len; r.q_len = Lq;
    r.logits = logits_out; r.logits2 = logits2_out; r.stream = (hipStream_t)hip_stream;
    return forward_interaction(h, r);
  });
}
int rr_forward_interaction_fusion_li(rr_handle h, const float* query_li, const float* context_li, const float* query_mask, const float* context_mask, float fusion_multiplier, int Bq, int K, int Lq, int Lc, const float* labels, int pair_begin, int pair_end, float* logits_out, float* logits2_out, float* loss_out, float* scores_out, int32_t* order_out, float* maxsim_out, void* hip_stream) {
  return guarded(h, [&]() -> int {
    Request r;
    r.family = FAM_INTERACTION; r.query_li = query_li; r.context_li = context_li; r.query_mask = query_mask; r.context_mask = context_mask;
    r.fusion_from_li = true; r.maxsim = maxsim_out; r.fusion_mult = fusion_multiplier;
    r.Bq = Bq; r.K = K; r.q_len = Lq; r.len = Lc; r.labels = labels; r.pair_begin = pair_begin; r.pair_end = pair_end;
    r.logits = logits_out; r.logits2 = logits2_out; r.loss = loss_out; r.scores = scores_out; r.order = order_out; r.stream = (hipStream_t)hip_stream;
    return forward_interaction(h, r);
  });
}
int rr_forward_interaction_packed_fusion_li(rr_handle h, const float* query_li, const float* context_li, const float* query_mask, const float* context_mask, float fusion_multiplier, int n_segments, const int32_t* seg_pairs, const int32_t* seg_len, int padded_context_len, int Lq, float* logits_out, float* logits2_out, float* maxsim_out, void* hip_stream) {
  return guarded(h, [&]() -> int {
    Request r;
    r.family = FAM_INTERACTION; r.query_li = query_li; r.context_li = context_li; r.query_mask = query_mask; r.context_mask = context_mask;
    r.fusion_from_li = true; r.maxsim = maxsim_out; r.fusion_mult = fusion_multiplier;
    r.packed = true; r.n_segments = n_segments; r.seg_pairs = seg_pairs; r.seg_len = seg_len; r.len = padded_context_len; r.q_len = Lq;
    r.logits = logits_out; r.logits2 = logits2_out; r.stream = (hipStream_t)hip_stream;
    return forward_interaction(h, r);
  });
}
int rr_forward_interaction_bank(rr_handle h, rr_bank_handle b, const float* query_li, const float* query_mask, int n_queries, int Lq, const int32_t* pair_passage, const int32_t* pair_query, int n_segments, const int32_t* seg_pairs, const int32_t* seg_len, int padded_context_len, int fusion_from_li, float fusion_multiplier, float* logits_out, float* logits2_out, float* maxsim_out, void* hip_stream) {
  return guarded(h, [&]() -> int { return forward_interaction_bank(h, b, query_li, query_mask, n_queries, Lq, pair_passage, pair_query, n_segments, seg_pairs, seg_len, padded_context_len, fusion_from_li, fusion_multiplier, logits_out, logits2_out, maxsim_out, hip_stream); });
}
int rr_op_li_scores(const float* query_li, const float* context_li, const float* context_mask, int n, int K, int Lq, int Lc, int D, float* scores_out, float* maxsim_out, void* hip_stream) {
  if (!query_li || !context_li || !context_mask || (!scores_out && !maxsim_out)) return RR_ERR_BAD_ARG;
  if (D <= 0 || D % 16) return RR_ERR_UNSUPPORTED;
  if (n <= 0 || K <= 0 || Lq <= 0 || Lc <= 0) return RR_ERR_BAD_SHAPE;
  return rr_launch_li_scores(query_li, context_li, context_mask, n, K, Lq, Lc, Lc, D, 0, scores_out, maxsim_out, (hipStream_t)hip_stream) == hipSuccess ? RR_OK : RR_ERR_HIP;
}
int rr_li_scores(rr_handle h, const float* query_li, const float* context_li, const float* context_mask, int Bq, int K, int Lq, int Lc, int pair_begin, int pair_end, float* scores_out, float* maxsim_out, void* hip_stream) {
  return guarded(h, [&]() -> int { return li_scores_call(h, query_li, context_li, context_mask, Bq, K, Lq, Lc, pair_begin, pair_end, scores_out, maxsim_out, hip_stream); });
}
int rr_get_profile(rr_handle h, rr_profile* out, int reset) {
  return guarded(h, [&]() -> int { return rr_get_profile_impl(h, out, reset); });
}
int rr_op_gemm_bf16(const uint16_t* A, const uint16_t* W, const float* bias, int M, int N, int Kd, int epilogue, void* out, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_gemm_bf16_impl(A, W, bias, M, N, Kd, epilogue, out, hip_stream); });
}
int rr_op_gemm_fp8(const uint8_t* A8, const uint8_t* W8, const float* bias, float scale, int M, int N, int K, int epilogue, void* out, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_gemm_fp8_impl(A8, W8, bias, scale, M, N, K, epilogue, out, hip_stream); });
}
int rr_op_quantize_fp8(const void* x, int x_is_f32, float scale, uint8_t* out, size_t n, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_quantize_fp8_impl(x, x_is_f32, scale, out, n, hip_stream); });
}
int rr_op_amax(const void* x, int x_is_f32, size_t n, float* out_dev, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_amax_impl(x, x_is_f32, n, out_dev, hip_stream); });
}
int rr_op_gemm_resid_f32(const uint16_t* A, const uint16_t* W, const float* bias, const float* resid, int M, int N, int Kd, float* out, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_gemm_resid_f32_impl(A, W, bias, resid, M, N, Kd, out, hip_stream); });
}
int rr_op_attention_bf16(const uint16_t* q, const uint16_t* k, const uint16_t* v, int q_stride, int kv_stride, const float* key_bias, int B, int heads, int Tq, int Tk, int q_batch_div, uint16_t* out, int out_stride, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_attention_ex_impl(q, k, v, q_stride, kv_stride, key_bias, B, heads, Tq, Tk, q_batch_div, 0, out, out_stride, nullptr, 0, 0, -1, hip_stream); });
}
int rr_op_attention_ex(const uint16_t* q, const uint16_t* k, const uint16_t* v, int q_stride, int kv_stride, const float* key_bias, int B, int heads, int Tq, int Tk, int q_batch_div, int q_batch_off, uint16_t* out, int out_stride, const float* dense_bias, int dense_ld, int64_t schedule_blocks, int fixed_mode, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_attention_ex_impl(q, k, v, q_stride, kv_stride, key_bias, B, heads, Tq, Tk, q_batch_div, q_batch_off, out, out_stride, dense_bias, dense_ld, schedule_blocks, fixed_mode, hip_stream); });
}
int rr_op_attention_segs(const uint16_t* q, int q_stride, const uint16_t* k, const uint16_t* v, int kv_stride, const float* key_bias, int heads, int nseg, const int* seg_n, const int* seg_len, const int64_t* seg_row0, uint16_t* out, int out_stride, int64_t schedule_blocks, int fixed_mode, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_attention_segs_impl(q, q_stride, k, v, kv_stride, key_bias, heads, nseg, seg_n, seg_len, seg_row0, out, out_stride, schedule_blocks, fixed_mode, hip_stream); });
}
int rr_op_fusion_adj(const float* scores, int S, int Tq, int Tc, float mult, int pair0, int n, float* adj, int ld, int row0, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_fusion_adj_impl(scores, S, Tq, Tc, mult, pair0, n, adj, ld, row0, hip_stream); });
}
int rr_op_fusion_adj_segs(const float* scores, int S, int Tq, int Tc, float mult, int nseg, const int* seg_n, const int* seg_tk, float* adj, int row0, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_fusion_adj_segs_impl(scores, S, Tq, Tc, mult, nseg, seg_n, seg_tk, adj, row0, hip_stream); });
}
int rr_op_gemm_ln_resid_f32(const uint16_t* A, const uint16_t* W, const float* bias, const float* x, const float* stats, const float* gamma, const float* beta, int M, int N, int Kd, float* out, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_gemm_ln_resid_f32_impl(A, W, bias, x, stats, gamma, beta, M, N, Kd, out, hip_stream); });
}
int rr_op_layernorm_stats(const float* x, const float* gamma, const float* beta, float eps, int rows, int cols, float* out_f32, uint16_t* out_bf16, float* stats, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_layernorm_stats_impl(x, gamma, beta, eps, rows, cols, out_f32, out_bf16, stats, hip_stream); });
}
int rr_op_layernorm(const float* x, const float* gamma, const float* beta, float eps, int rows, int cols, float* out_f32, uint16_t* out_bf16, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_layernorm_impl(x, gamma, beta, eps, rows, cols, out_f32, out_bf16, hip_stream); });
}
int rr_op_gemm_resid_lnprep(const uint16_t* A, const uint16_t* W, const float* bias, const float* resid, int M, int N, int Kd,
                            float eps, float* out_f32, uint16_t* x16_out, float* stats_out, float* part_scratch, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_gemm_resid_lnprep_impl(A, W, bias, resid, M, N, Kd, eps, out_f32, x16_out, stats_out, part_scratch, hip_stream); });
}
int rr_op_gemm_resid_split(const uint16_t* A, const uint16_t* W, const float* bias, const uint16_t* hi_in, const uint16_t* lo_in,
                           const float* ln_stats, const float* ln_gamma, const float* ln_beta, int M, int N, int Kd, float eps,
                           uint16_t* x16_out, uint16_t* lo_out, float* stats_out, float* part_scratch, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_gemm_resid_split_impl(A, W, bias, hi_in, lo_in, ln_stats, ln_gamma, ln_beta, M, N, Kd, eps, x16_out, lo_out, stats_out, part_scratch, hip_stream); });
}
int rr_op_split_residual_value(const uint16_t* hi, const uint16_t* lo, const float* stats, const float* gamma, const float* beta,
                               int rows, int cols, float* out, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_split_residual_value_impl(hi, lo, stats, gamma, beta, rows, cols, out, hip_stream); });
}
int rr_op_gemm_lnfold(const uint16_t* A_raw, const uint16_t* W_folded, const float* dvec, const float* csum, const float* stats,
                      int M, int N, int Kd, int epilogue, void* out, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_gemm_lnfold_impl(A_raw, W_folded, dvec, csum, stats, M, N, Kd, epilogue, out, hip_stream); });
}
int rr_op_gemm_fp8_rc(const uint8_t* A8, const uint8_t* W8, const float* bias, const float* row_scale, const float* col_scale,
                      int M, int N, int K, int epilogue, void* out, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_gemm_fp8_rc_impl(A8, W8, bias, row_scale, col_scale, M, N, K, epilogue, out, hip_stream); });
}
int rr_op_gemm_fp8_gelu_e4m3(const uint8_t* A8, const uint8_t* W8, const float* bias, const float* row_scale, const float* col_scale,
                             float out_mul, int M, int N, int K, uint8_t* out8, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_gemm_fp8_gelu_e4m3_impl(A8, W8, bias, row_scale, col_scale, out_mul, M, N, K, out8, hip_stream); });
}
int rr_op_gemm_fp8_resid(const uint8_t* A8, const uint8_t* W8, const float* bias, float scale, const float* col_scale,
                         const float* resid, const float* stats, const float* gamma, const float* beta, int M, int N, int K, float* out,
                         void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_gemm_fp8_resid_impl(A8, W8, bias, scale, col_scale, resid, stats, gamma, beta, M, N, K, out, hip_stream); });
}
int rr_op_layernorm_q8(const float* x, const float* gamma, const float* beta, float eps, int rows, int cols, uint8_t* out8,
                       float* row_scale, float* stats, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_layernorm_q8_impl(x, gamma, beta, eps, rows, cols, out8, row_scale, stats, hip_stream); });
}
int rr_util_quantize_rows_e4m3(const float* w_host, int rows, int cols, uint8_t* out_host, float* scales_host) {
  if (!w_host || !out_host || !scales_host || rows <= 0 || cols <= 0) return RR_ERR_BAD_ARG;
  return guarded(nullptr, [&]() -> int { host_quantize_rows(w_host, (size_t)rows, (size_t)cols, out_host, scales_host); return RR_OK; });
}
int rr_op_gemm_i8_rc(const int8_t* A8, const int8_t* W8, const float* bias, const float* row_scale, const float* col_scale,
                     int M, int N, int K, int epilogue, void* out, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_gemm_i8_rc_impl(A8, W8, bias, row_scale, col_scale, M, N, K, epilogue, out, hip_stream); });
}
int rr_op_layernorm_i8(const float* x, const float* gamma, const float* beta, float eps, int rows, int cols, int8_t* out8,
                       float* row_scale, float* stats, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_layernorm_i8_impl(x, gamma, beta, eps, rows, cols, out8, row_scale, stats, hip_stream); });
}
int rr_util_quantize_rows_i8(const float* w_host, int rows, int cols, int8_t* out_host, float* scales_host) {
  if (!w_host || !out_host || !scales_host || rows <= 0 || cols <= 0) return RR_ERR_BAD_ARG;
  return guarded(nullptr, [&]() -> int { host_quantize_rows_i8(w_host, (size_t)rows, (size_t)cols, out_host, scales_host); return RR_OK; });
}
int rr_util_smooth_scales(const float* gamma_host, const float* beta_host, int n, float* s_host) {
  if (!gamma_host || !beta_host || !s_host || n <= 0) return RR_ERR_BAD_ARG;
  return guarded(nullptr, [&]() -> int { host_smooth_scales(gamma_host, beta_host, (size_t)n, s_host); return RR_OK; });
}
int rr_activation_range_flag(rr_handle h, int reset, int* flag_out, void* hip_stream) {
  if (!h || !flag_out) return RR_ERR_BAD_ARG;
  return guarded(h, [&]() -> int {
    rr_model* m = h;
    *flag_out = 0;
    if (!m->range_flag) return RR_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    RR_HIP(m, hipSetDevice(m->cfg.device));
    RR_HIP(m, hipMemcpyAsync(flag_out, m->range_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    if (reset) RR_HIP(m, hipMemsetAsync(m->range_flag, 0, sizeof(int), st));
    RR_HIP(m, hipStreamSynchronize(st));
    if (m->range_flag_host) *m->range_flag_host = reset ? 0 : *flag_out;
    return RR_OK;
  });
}
int rr_set_padded_seq_len(rr_handle h, int padded_seq_len) {
  if (!h || padded_seq_len < 0) return RR_ERR_BAD_ARG;
  return guarded(h, [&]() -> int {
    if (padded_seq_len > h->cfg.max_pos) return fail(h, RR_ERR_BAD_SHAPE, "padded_seq_len %d exceeds max_position_embeddings %d", padded_seq_len, h->cfg.max_pos);
    h->padded_S = padded_seq_len;
    return RR_OK;
  });
}
int rr_reserve(rr_handle h, int n_pairs, int n_queries, int len_a, int len_b, int with_fusion, void* hip_stream) {
  return guarded(h, [&]() -> int { return rr_reserve_impl(h, n_pairs, n_queries, len_a, len_b, with_fusion, hip_stream); });
}
int64_t rr_workspace_bytes(rr_handle h, int n_pairs, int seq_len) {
  return guarded<int64_t>(h, [&]() -> int64_t { return rr_workspace_bytes_impl(h, n_pairs, seq_len); });
}
int64_t rr_debug_read(rr_handle h, const char* name, float* host_out, int64_t max_elems) {
  return guarded<int64_t>(h, [&]() -> int64_t { return rr_debug_read_impl(h, name, host_out, max_elems); });
}
int rr_op_embed_ln(const int64_t* ids, const int64_t* tts, const float* word, const float* pos, const float* type, const float* gamma,
                   const float* beta, float eps, int rows, int S, int cols, int vocab, int type_vocab, float* out_f32, uint16_t* out16,
                   void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_embed_ln_impl(ids, tts, word, pos, type, gamma, beta, eps, rows, S, cols, vocab, type_vocab, out_f32, out16, hip_stream); });
}
int rr_op_ce_embed_ln(const float* x, const float* pos, const float* type0, const float* gamma, const float* beta, float eps, int rows,
                      int T, int cols, float* out_f32, uint16_t* out16, int s_text, int vis_pos0, int cls32, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_ce_embed_ln_impl(x, pos, type0, gamma, beta, eps, rows, T, cols, out_f32, out16, s_text, vis_pos0, cls32, hip_stream); });
}
int rr_op_li_normalize(const float* src, const int64_t* ids, int ids_stride, int n_pairs, int rows_per_batch, int D, int T, int t_off,
                       int pair_off, int bdiv, int src_batch_off, uint16_t* dst, int normalize, const float* maskf, int split, int shift,
                       void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_li_normalize_impl(src, ids, ids_stride, n_pairs, rows_per_batch, D, T, t_off, pair_off, bdiv, src_batch_off, dst, normalize, maskf, split, shift, hip_stream); });
}
int rr_op_key_bias(const int64_t* ids, const int64_t* am, int n, int S, int T, float* text_bias, float* ce_bias, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_key_bias_impl(ids, am, n, S, T, text_bias, ce_bias, hip_stream); });
}
int rr_op_joint_masks(const int64_t* ids, const int64_t* am, int n, int S, int P, int q_len, int64_t instruction_token, float* text_bias,
                      float* li_mask, float* ce_bias, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_joint_masks_impl(ids, am, n, S, P, q_len, instruction_token, text_bias, li_mask, ce_bias, hip_stream); });
}
int rr_op_interaction_bias(const float* qmask, const float* cmask, int n, int Lq, int Lc, int pair_off, int K, float* cat_bias,
                           float* q_bias, float* c_bias, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_interaction_bias_impl(qmask, cmask, n, Lq, Lc, pair_off, K, cat_bias, q_bias, c_bias, hip_stream); });
}
int rr_op_vit_im2col(const float* px, uint16_t* out, int B, int IS, int ps, int Kp, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_vit_im2col_impl(px, out, B, IS, ps, Kp, hip_stream); });
}
int rr_op_vit_embed_ln(const float* patches, const float* cls_emb, const float* pos, const float* gamma, const float* beta, float eps,
                       int rows, int T, int cols, float* out_f32, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_vit_embed_ln_impl(patches, cls_emb, pos, gamma, beta, eps, rows, T, cols, out_f32, hip_stream); });
}
int rr_op_cast16(const float* x, uint16_t* y, int64_t n, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_cast16_impl(x, y, n, hip_stream); });
}
int rr_op_gather_rows(const void* src, void* dst, int n_dst_batches, int rows_take, int src_rows_per_batch, int row_bytes, int batch_off,
                      int bdiv, int src_batch_off, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_gather_rows_impl(src, dst, n_dst_batches, rows_take, src_rows_per_batch, row_bytes, batch_off, bdiv, src_batch_off, hip_stream); });
}
int rr_op_cls_heads(const float* h32, int T, int cols, int n_pairs, const float* w1, const float* b1, const float* w2, const float* b2,
                    float* out1, float* out2, void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_cls_heads_impl(h32, T, cols, n_pairs, w1, b1, w2, b2, out1, out2, hip_stream); });
}
int rr_op_ln_finalize(const float* part, int nparts, int cols, float eps, int rows, float* stats, int* range_flag, float range_ss,
                      void* hip_stream) {
  return guarded(nullptr, [&]() -> int { return rr_op_ln_finalize_impl(part, nparts, cols, eps, rows, stats, range_flag, range_ss, hip_stream); });
}

}  // extern "C"
