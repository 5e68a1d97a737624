// KV-cached generation on a SlamEngine (include/slam_engine.h): the cache binding, the FP8 copy of the decode projections,
// slam_prefill, slam_decode_step, slam_kv_repeat, the three slam_extend* entry points and slam_kv_rewind. The kernels are in
// decode.hip and quant.hip; the prefill runs the training forward's own layer loop (forward_layers, engine.hip).
#include <hip/hip_runtime.h>
#include <math.h>

#include "engine_impl.h"

namespace {
// decode-time projection: the weight-streaming kernel up to SKINNY_MAX_M rows (split-K partials in the backward-only dact
// buffer), the tiled GEMM beyond; fp32 outputs always take the streaming kernel (in 64-row chunks)
int decode_proj(SlamEngine* h, const bf16_t* X, const bf16_t* W, bf16_t* Y, float* Yf, const bf16_t* bias, const bf16_t* resid,
                int M, int N, int K, hipStream_t st) {
  if (Yf || M <= SKINNY_MAX_M) {
    float* ws = (float*)h->dact;
    const size_t ws_bytes = (size_t)h->max_tokens * h->d.intermediate * sizeof(bf16_t);
    // valid FP8 codes of this matrix: the same stream at half the bytes, the same bits (the parameters hold Wdq)
    if (h->w8_valid) {
      const auto it = h->w8_mats.find(W - h->params);
      if (it != h->w8_mats.end() && it->second.N == N && it->second.K == K) {
        ++h->w8_launches;
        return gemm_skinny_w8(X, it->second.q, it->second.e, Y, Yf, bias, resid, M, N, K, ws, ws_bytes, st);
      }
    }
    return gemm_skinny(X, W, Y, Yf, bias, resid, M, N, K, ws, ws_bytes, st);
  }
  return gemm_nt(X, W, Y, bias, resid, M, N, K, st);
}
// the matrices of the FP8 decode copy in buffer order: offset in the parameter buffer, N, K
struct W8Shape { int64_t off; int N, K; };
static std::vector<W8Shape> w8_matrix_list(const SlamEngine* h, bool include_head) {
  const SlamModelDesc& d = h->d;
  const int HD = d.n_heads * d.head_dim;
  std::vector<W8Shape> v;
  for (int l = 0; l < d.n_layers; ++l) {
    const LayerOff& o = h->lo[l];
    v.push_back({o.wqkv, h->QKV, d.hidden});
    v.push_back({o.wo, d.hidden, HD});
    v.push_back({o.wgu, 2 * d.intermediate, d.hidden});
    v.push_back({o.wd, d.hidden, d.intermediate});
  }
  if (include_head) v.push_back({h->off_head, d.vocab, d.hidden});
  return v;
}
// why the FP8 decode copy cannot exist for this engine (nullptr: it can)
static const char* w8_refusal(const SlamEngine* h) {
  if (h->arch == 1) return "FP8 decode weights: the OPT family has no decode path";
  const SlamModelDesc& d = h->d;
  if (d.hidden % W8_K_GRAIN || d.intermediate % W8_K_GRAIN || (d.n_heads * d.head_dim) % W8_K_GRAIN)
    return "FP8 decode weights need hidden, intermediate and n_heads * head_dim to be multiples of 64";
  return nullptr;
}
// The second half of a cached layer over M rows (la[l].o -> hs[l + 1]): out-projection + residual, norm, gate|up, SwiGLU, down +
// residual
static int cached_mlp(SlamEngine* h, int l, int M, hipStream_t st) {
  const int H = h->d.hidden, I = h->d.intermediate, HD = h->d.n_heads * h->d.head_dim;
  const bf16_t* P = h->params;
  const LayerOff& o = h->lo[l];
  LayerAct& a = h->la[l];
  CK(decode_proj(h, a.o, P + o.wo, a.hmid, nullptr, nullptr, h->hs[l], M, H, HD, st));
  CK(norm_fwd(h, a.hmid, o.ln2, o.ln2_b, a.x2, a.mu2, a.rstd2, M, st));
  CK(decode_proj(h, a.x2, P + o.wgu, a.gu, nullptr, nullptr, nullptr, M, 2 * I, H, st));
  CK(swiglu_fwd(a.gu, a.act, M, I, GU_BLK, st));
  CK(decode_proj(h, a.act, P + o.wd, h->hs[l + 1], nullptr, nullptr, a.hmid, M, H, I, st));
  return SLAM_OK;
}
// The last-token head of prefill, decode step and extend: final norm of the B rows of x, one fp32 head launch over them
static int last_token_head(SlamEngine* h, const bf16_t* x, int B, float* logits, hipStream_t st) {
  CK(norm_fwd(h, x, h->off_norm, h->off_norm_b, h->hf, h->muf, h->rstdf, B, st));
  CK(decode_proj(h, h->hf, h->params + h->off_head, nullptr, logits, nullptr, nullptr, B, h->d.vocab, h->d.hidden, st));
  return SLAM_OK;
}

// slam_extend, slam_extend_score and slam_extend_logits: one body. EXT_LAST is slam_extend, launch for launch; EXT_SCORE adds,
// between the layer loop and the last-token head, the final norm of all B T rows and the fused head + row statistics; EXT_ALL
// replaces the last-token head by the final norm and the fp32 head of all B T rows (logits_out is then the [B][T][vocab] array).
enum ExtendMode { EXT_LAST, EXT_SCORE, EXT_ALL };
int extend_common(SlamEngine* h, const int64_t* ids, const int32_t* new_lens, int32_t* lens, int32_t B, int32_t T,
                  float* logits_out, ExtendMode mode, float* lp_out, int64_t* argmax_out, slam_stream_t stream) {
  const bool score = mode == EXT_SCORE;
  if (!h || !ids || !new_lens || !lens || !logits_out || B <= 0 || T <= 0 || (score && !lp_out)) return SLAM_EINVAL;
  if (!h->params || !h->ws) return h->fail(SLAM_ESTATE, "bind params and workspace first");
  if (h->arch == 1) return h->fail(SLAM_EINVAL, "KV-cached generation is implemented for the Qwen2 family only");
  if (!h->kv) return h->fail(SLAM_ESTATE, "bind a KV cache first");
  if ((int64_t)B * T > h->max_tokens) return h->fail(SLAM_ENOMEM, "B*T exceeds bound workspace tokens");
  if ((int64_t)2 * B > h->max_tokens) return h->fail(SLAM_ENOMEM, "extend needs a workspace of at least 2 B tokens");
  if ((int64_t)(h->kv_ready ? h->kv_hi : 0) + T > h->kv_cap) return h->fail(SLAM_ESTATE, "extend past the KV cache capacity");
  if (!h->kv_ready) return h->fail(SLAM_ESTATE, "slam_extend needs a slam_prefill into the bound cache first");
  if (B != h->kv_B) return h->fail(SLAM_EINVAL, "extend batch differs from the decode batch");
  const SlamModelDesc& d = h->d;
  if (score && score_rows_workspace_bytes(B * T, d.vocab) > (size_t)h->max_tokens * h->vpad * sizeof(bf16_t))
    return h->fail(SLAM_ENOMEM, "chunk partials exceed the logits buffer");
  hipStream_t st = (hipStream_t)stream;
  const int H = d.hidden, L = d.n_layers, nH = d.n_heads, nKV = d.n_kv_heads, hd = d.head_dim;
  const int M = B * T;
  const bf16_t* P = h->params;
  h->have_fwd = false;
  h->fwd_drop = false;
  GemmTuneScope tune_scope(&h->gemm_tune);
  CK(join_optimizer(h, st));
  CK(join_params(h, st));
  // scratch in buffers only backward and the loss read: the tokens' int64 positions (dh_a), attention split partials and,
  // behind the layer loop, the fp32 logits of all B rows (the logits buffer: 2 B <= workspace tokens covers 4 B vocab bytes)
  int64_t* pos = (int64_t*)h->dh_a;
  const float qscale = 1.44269504088896340736f / sqrtf((float)hd);
  CK(extend_positions(lens, pos, B, T, st));
  CK(rope_table(pos, M, T, hd, d.rope_theta, h->cosb, h->sinb, h->cosq, h->sinq, qscale, st));
  CK(embed_fwd(ids, P + h->off_embed, h->hs[0], M, H, d.vocab, st));
  const size_t part_bytes = (size_t)h->max_tokens * h->vpad * sizeof(bf16_t);
  const int kv_bound = h->kv_hi + T;
  const bool q3 = h->arch == 3;  // Qwen3: no bias, and the per-head norm sits between the projection and the rotation
  const bool fused_rope = !q3 && M > SKINNY_MAX_M && hd == 64 && (H % 64 == 0) && (h->QKV % 128 == 0);
  for (int l = 0; l < L; ++l) {
    const LayerOff& o = h->lo[l];
    LayerAct& a = h->la[l];
    CK(norm_fwd(h, h->hs[l], o.ln1, o.ln1_b, a.x1, a.mu1, a.rstd1, M, st));
    if (fused_rope) {
      CK(gemm_nt_rope(a.x1, P + o.wqkv, a.qkv, P + o.bqkv, h->cosb, h->sinb, h->cosq, h->sinq, nH, nH + nKV, M, h->QKV, H, st));
    } else {
      CK(decode_proj(h, a.x1, P + o.wqkv, a.qkv, nullptr, q3 ? nullptr : P + o.bqkv, nullptr, M, h->QKV, H, st));
      if (q3) CK(qknorm_rope_fwd(a.qkv, h->QKV, M, nH, nKV, hd, P + o.q_norm, P + o.k_norm, h->cosb, h->sinb, h->cosq, h->sinq, d.rms_eps, nullptr, nullptr, st));
      else CK(rope_apply(a.qkv, h->QKV, M, nH + nKV, hd, h->cosb, h->sinb, 0, st, nH, qscale));
    }
    CK(attn_extend(a.qkv, lens, new_lens, kv_k(h, l), kv_v(h, l), h->kv_cap, B, T, nH, nKV, hd, kv_bound, a.o, (float*)h->logits,
                   part_bytes, st));
    CK(cached_mlp(h, l, M, st));
  }
  if (score) {
    // every chunk position: final norm of the B T rows, then the head fused with the row statistics. Scratch behind the layer
    // loop: the targets (int64 [B T]) in the backward-only dqkv buffer, chunk partials and target scores at the start of the
    // logits buffer (the attention partials are dead; the last-token logits below overwrite it after these launches)
    int64_t* tg = (int64_t*)h->dqkv;
    CK(extend_targets(ids, new_lens, tg, B, T, st));
    CK(norm_fwd(h, h->hs[L], h->off_norm, h->off_norm_b, h->hf, h->muf, h->rstdf, M, st));
    CK(score_rows(h->hf, P + h->off_head, tg, h->logit_mask, M, d.vocab, H, new_lens, T, lp_out, argmax_out, h->logits,
                  part_bytes, st));
  }
  if (mode == EXT_ALL) {
    // every chunk position: final norm of the B T rows, then the fp32 head in groups of G rows through the logits buffer (the
    // attention partials are dead; G fp32 rows of vocab fit in 2 G bf16 rows of vpad), each group's real rows stored behind it
    CK(norm_fwd(h, h->hs[L], h->off_norm, h->off_norm_b, h->hf, h->muf, h->rstdf, M, st));
    const int G = (int)std::min<int64_t>(h->max_tokens / 2, 32768);
    float* lg = (float*)h->logits;
    for (int m0 = 0; m0 < M; m0 += G) {
      const int rows = std::min(G, M - m0);
      CK(decode_proj(h, h->hf + (size_t)m0 * H, P + h->off_head, nullptr, lg, nullptr, nullptr, rows, d.vocab, H, st));
      CK(extend_store_rows(lg, logits_out, new_lens, m0, rows, B, T, d.vocab, st));
    }
    CK(lens_add(lens, new_lens, B, T, st));
    if (h->kv_hi == h->kv_T) h->kv_T += T;
    h->kv_hi += T;
    return SLAM_OK;
  }
  // each row's last real token: gather, final norm, one fp32 head launch over B rows; inert rows keep their logits and lens
  CK(gather_last_rows(h->hs[L], h->dx, new_lens, B, T, H, st));
  float* lg = (float*)h->logits;
  CK(last_token_head(h, h->dx, B, lg, st));
  CK(extend_finish(lg, logits_out, new_lens, lens, B, T, d.vocab, st));
  if (h->kv_hi == h->kv_T) h->kv_T += T;  // no decode step since the prefill: slam_kv_repeat stays legal
  h->kv_hi += T;
  return SLAM_OK;
}
}  // namespace

extern "C" {

size_t slam_kv_cache_bytes(SlamEngine* h, int32_t max_batch, int32_t capacity) {
  if (!h || max_batch <= 0 || capacity <= 0) return 0;
  const SlamModelDesc& d = h->d;
  return (size_t)d.n_layers * 2 * max_batch * d.n_kv_heads * capacity * d.head_dim * sizeof(bf16_t);
}
int slam_bind_kv_cache(SlamEngine* h, void* cache, size_t bytes, int32_t max_batch, int32_t capacity) {
  if (!h || !cache || max_batch <= 0 || capacity <= 0) return SLAM_EINVAL;
  if (((uintptr_t)cache) & 255) return h->fail(SLAM_EINVAL, "KV cache must be 256-byte aligned");
  if (bytes < slam_kv_cache_bytes(h, max_batch, capacity)) return h->fail(SLAM_ENOMEM, "KV cache too small");
  h->kv = (bf16_t*)cache;
  h->kv_bmax = max_batch;
  h->kv_cap = capacity;
  h->kv_ready = false;
  return SLAM_OK;
}

size_t slam_decode_w8_bytes(SlamEngine* h, int32_t include_head) {
  if (!h || w8_refusal(h)) return 0;
  size_t bytes = 0;
  for (const W8Shape& m : w8_matrix_list(h, include_head != 0)) bytes += w8_bytes(m.N, m.K);
  return bytes;
}

int slam_bind_decode_w8(SlamEngine* h, void* buf, size_t bytes, int32_t include_head) {
  if (!h) return SLAM_EINVAL;
  h->w8 = nullptr;
  h->w8_valid = false;
  h->w8_head = false;
  h->w8_launches = 0;
  h->w8_mats.clear();
  if (!buf) return SLAM_OK;
  if (const char* why = w8_refusal(h)) return h->fail(SLAM_EINVAL, why);
  if (((uintptr_t)buf) & 255) return h->fail(SLAM_EINVAL, "FP8 decode weights must be 256-byte aligned");
  if (bytes < slam_decode_w8_bytes(h, include_head)) return h->fail(SLAM_ENOMEM, "FP8 decode weight buffer too small");
  char* p = (char*)buf;
  for (const W8Shape& m : w8_matrix_list(h, include_head != 0)) {
    h->w8_mats[m.off] = SlamEngine::W8Mat{m.N, m.K, (uint8_t*)p, (int8_t*)(p + w8_exps_offset(m.N, m.K))};
    p += w8_bytes(m.N, m.K);
  }
  h->w8 = (char*)buf;
  h->w8_head = include_head != 0;
  return SLAM_OK;
}

int slam_quantize_decode_w8(SlamEngine* h, slam_stream_t stream) {
  if (!h) return SLAM_EINVAL;
  if (!h->params) return h->fail(SLAM_ESTATE, "bind params first");
  if (!h->w8) return h->fail(SLAM_ESTATE, "bind FP8 decode weights first (slam_bind_decode_w8)");
  hipStream_t st = (hipStream_t)stream;
  CK(join_optimizer(h, st));
  CK(join_params(h, st));
  h->w8_valid = false;
  for (const auto& kv : h->w8_mats) {  // rows are independent and the matrices disjoint: the order does not matter
    const SlamEngine::W8Mat& m = kv.second;
    const int r = quantize_rows_fp8(h->params + kv.first, m.q, m.e, m.N, m.K, st);
    if (r) return r == -1 ? h->fail(SLAM_EINVAL, "FP8 decode weights: a parameter matrix is not 16-byte aligned") : r;
  }
  CK(refresh_transposed_images(h, stream));
  h->w8_valid = true;
  return SLAM_OK;
}

int slam_decode_w8_state(SlamEngine* h) { return !h || !h->w8 ? 0 : h->w8_valid ? 2 : 1; }
int64_t slam_decode_w8_launches(SlamEngine* h) { return h ? h->w8_launches : 0; }

int slam_prefill(SlamEngine* h, const int64_t* ids, const int32_t* lens, int32_t B, int32_t T, float* logits_out,
                 slam_stream_t stream) {
  if (!h || !ids || !lens || !logits_out || B <= 0 || T <= 0) return SLAM_EINVAL;
  if (!h->params || !h->ws) return h->fail(SLAM_ESTATE, "bind params and workspace first");
  if (h->arch == 1) return h->fail(SLAM_EINVAL, "KV-cached generation is implemented for the Qwen2 family only");
  if (!h->kv) return h->fail(SLAM_ESTATE, "bind a KV cache first");
  if (B > h->kv_bmax || T > h->kv_cap) return h->fail(SLAM_EINVAL, "prefill batch exceeds the bound KV cache");
  if ((int64_t)B * T > h->max_tokens) return h->fail(SLAM_ENOMEM, "B*T exceeds bound workspace tokens");
  const SlamModelDesc& d = h->d;
  hipStream_t st = (hipStream_t)stream;
  const int H = d.hidden, L = d.n_layers, M = B * T;
  h->have_fwd = false;
  h->fwd_drop = false;  // generation never drops ...
  h->fwd_neft = false;  // ... and never draws NEFTune noise
  h->kv_ready = false;
  GemmTuneScope tune_scope(&h->gemm_tune);
  // "recompute" = 2 with more layers than slots: the layers share their q|k|v buffers, so each layer's K / V leave inside the loop
  const bool shared_qkv = h->recompute == 2 && L > RC_SLOTS;
  CK(forward_layers(h, ids, nullptr, nullptr, nullptr, M, T, st, shared_qkv ? lens : nullptr, B));
  for (int l = 0; l < L && !shared_qkv; ++l)
    CK(kv_scatter(h->la[l].qkv, kv_k(h, l), kv_v(h, l), lens, B, T, d.n_heads, d.n_kv_heads, d.head_dim, h->kv_cap, st));
  // logits of each row's last prompt token only: gather, final norm, one fp32 head launch over B rows
  CK(gather_last_rows(h->hs[L], h->dx, lens, B, T, H, st));
  CK(last_token_head(h, h->dx, B, logits_out, st));
  h->kv_B = B;
  h->kv_hi = T;
  h->kv_T = T;
  h->kv_ready = true;
  return SLAM_OK;
}

int slam_decode_step(SlamEngine* h, const int64_t* ids, int32_t* lens, int32_t B, float* logits_out, slam_stream_t stream) {
  if (!h || !ids || !lens || !logits_out || B <= 0) return SLAM_EINVAL;
  if (!h->params || !h->ws) return h->fail(SLAM_ESTATE, "bind params and workspace first");
  if (h->arch == 1) return h->fail(SLAM_EINVAL, "KV-cached generation is implemented for the Qwen2 family only");
  if (!h->kv) return h->fail(SLAM_ESTATE, "bind a KV cache first");
  if (!h->kv_ready) return h->fail(SLAM_ESTATE, "slam_decode_step needs a slam_prefill into the bound cache first");
  if (B != h->kv_B) return h->fail(SLAM_EINVAL, "decode batch differs from the prefill batch");
  if (h->kv_hi + 1 > h->kv_cap) return h->fail(SLAM_ESTATE, "decode step past the KV cache capacity");
  if ((int64_t)2 * B > h->max_tokens) return h->fail(SLAM_ENOMEM, "decode needs a workspace of at least 2 B tokens");
  const SlamModelDesc& d = h->d;
  hipStream_t st = (hipStream_t)stream;
  const int H = d.hidden, L = d.n_layers, nH = d.n_heads, nKV = d.n_kv_heads, hd = d.head_dim;
  const bf16_t* P = h->params;
  h->have_fwd = false;
  GemmTuneScope tune_scope(&h->gemm_tune);
  CK(join_optimizer(h, st));
  CK(join_params(h, st));
  // scratch in buffers only backward reads: fp32 QKV projection (dqkv: B x QKV x 4 bytes <= 2B x QKV x 2), the rows' int64
  // positions (nlse), attention split partials (the logits buffer)
  float* qkvf = (float*)h->dqkv;
  int64_t* pos = (int64_t*)h->nlse;
  const float qscale = 1.44269504088896340736f / sqrtf((float)hd);
  const bool q3 = h->arch == 3;
  CK(lens_to_pos(lens, pos, B, st));
  CK(rope_table(pos, B, 1, hd, d.rope_theta, h->cosb, h->sinb, h->cosq, h->sinq, qscale, st));
  CK(embed_fwd(ids, P + h->off_embed, h->hs[0], B, H, d.vocab, st));
  const size_t part_bytes = (size_t)h->max_tokens * h->vpad * sizeof(bf16_t);
  for (int l = 0; l < L; ++l) {
    const LayerOff& o = h->lo[l];
    LayerAct& a = h->la[l];
    CK(norm_fwd(h, h->hs[l], o.ln1, o.ln1_b, a.x1, a.mu1, a.rstd1, B, st));
    CK(decode_proj(h, a.x1, P + o.wqkv, nullptr, qkvf, nullptr, nullptr, B, h->QKV, H, st));
    // Qwen3: the q and k heads are normalised in the fp32 row; attn_decode then rotates and rounds once, without a bias
    if (q3) CK(qknorm_rows_f32(qkvf, h->QKV, B, nH, nKV, hd, P + o.q_norm, P + o.k_norm, d.rms_eps, st));
    CK(attn_decode(qkvf, q3 ? nullptr : P + o.bqkv, h->cosb, h->sinb, h->cosq, h->sinq, lens, kv_k(h, l), kv_v(h, l), h->kv_cap, B, nH, nKV, hd,
                   h->kv_hi + 1, a.o, (float*)h->logits, part_bytes, st));
    CK(cached_mlp(h, l, B, st));
  }
  CK(last_token_head(h, h->hs[L], B, logits_out, st));
  CK(lens_inc(lens, B, st));
  h->kv_hi += 1;
  return SLAM_OK;
}

int slam_kv_repeat(SlamEngine* h, int32_t n, int32_t* lens, float* logits, slam_stream_t stream) {
  if (!h || !lens || n < 1) return SLAM_EINVAL;
  if (!h->kv) return h->fail(SLAM_ESTATE, "bind a KV cache first");
  if (!h->kv_ready) return h->fail(SLAM_ESTATE, "slam_kv_repeat needs a slam_prefill into the bound cache first");
  if (h->kv_hi != h->kv_T) return h->fail(SLAM_ESTATE, "slam_kv_repeat after a decode step: prefill again");
  if ((int64_t)h->kv_B * n > h->kv_bmax) return h->fail(SLAM_EINVAL, "B * n rows exceed the bound KV cache");
  if (n == 1) return SLAM_OK;
  const SlamModelDesc& d = h->d;
  CK(kv_repeat(h->kv, lens, logits, h->kv_B, n, h->kv_bmax, d.n_layers, d.n_kv_heads, d.head_dim, h->kv_cap, h->kv_hi, d.vocab,
               (hipStream_t)stream));
  h->kv_B *= n;
  return SLAM_OK;
}

int slam_extend(SlamEngine* h, const int64_t* ids, const int32_t* new_lens, int32_t* lens, int32_t B, int32_t T,
                float* logits_out, slam_stream_t stream) {
  return extend_common(h, ids, new_lens, lens, B, T, logits_out, EXT_LAST, nullptr, nullptr, stream);
}

int slam_extend_score(SlamEngine* h, const int64_t* ids, const int32_t* new_lens, int32_t* lens, int32_t B, int32_t T,
                      float* logits_out, float* lp_out, int64_t* argmax_out, slam_stream_t stream) {
  return extend_common(h, ids, new_lens, lens, B, T, logits_out, EXT_SCORE, lp_out, argmax_out, stream);
}

int slam_extend_logits(SlamEngine* h, const int64_t* ids, const int32_t* new_lens, int32_t* lens, int32_t B, int32_t T,
                       float* logits_all, slam_stream_t stream) {
  return extend_common(h, ids, new_lens, lens, B, T, logits_all, EXT_ALL, nullptr, nullptr, stream);
}

int slam_kv_rewind(SlamEngine* h, int32_t hi) {
  if (!h) return SLAM_EINVAL;
  if (!h->kv) return h->fail(SLAM_ESTATE, "bind a KV cache first");
  if (!h->kv_ready) return h->fail(SLAM_ESTATE, "slam_kv_rewind needs a slam_prefill into the bound cache first");
  if (hi < 1 || hi > h->kv_hi) return h->fail(SLAM_EINVAL, "slam_kv_rewind: hi outside 1 .. the current bound");
  h->kv_hi = hi;
  h->kv_T = -1;  // as after a decode step: slam_kv_repeat is refused until the next prefill
  return SLAM_OK;
}

}  // extern "C"
