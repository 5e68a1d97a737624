// The single-op doors of the C ABI (include/slam_engine.h, slam_op_*): one kernel launcher each, for the parity tests and
// for consumers that drive single kernels. None of them takes a SlamEngine, so this file sees kernels.h only.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/slam_engine.h"
#include "kernels.h"

using namespace slam;

namespace {

// slam_op_attn_decode workspace: int64 positions [B], cos / sin / pre-scaled cos / sin tables [B][hd/2], split partials
size_t attn_decode_op_head(int B, int head_dim) { return (((size_t)B * 8 + 255) & ~(size_t)255) + (((size_t)4 * B * (head_dim / 2) * 4 + 255) & ~(size_t)255); }

// the argument ranges of the three q / k norm entry points, checked before anything is launched (the kernels index heads in
// 32 bits: elementwise.hip)
static bool qknorm_dims_ok(int M, int nH, int nKV, int head_dim) {
  if (M <= 0 || nH <= 0 || nKV <= 0 || (head_dim != 64 && head_dim != 128)) return false;
  return (uint64_t)M * (uint64_t)(nH + nKV) * (uint64_t)(head_dim / 8) < (1ull << 31) - 1024;
}

static bool drop_site_ok(int M, int H, int32_t thr16, int64_t call, int32_t stream_id, int64_t index0, DropSite* d) {
  if (M <= 0 || H <= 0 || (H & 7) || thr16 < 0 || thr16 > 65535 || call < 0 || call > 0xffffffffLL || stream_id < 0 || index0 < 0 ||
      (index0 & 7))
    return false;
  d->thr16 = thr16;
  d->call = (uint32_t)call;
  d->site = (uint32_t)stream_id;
  d->index0 = index0;
  return true;
}

}  // namespace

extern "C" {

int slam_op_unpad_pack_spans(const int64_t* ids, const int64_t* labels, const int32_t* starts, const int32_t* lens, int32_t B,
                             int32_t T, int32_t M_packed, int32_t pad_id, void* scratch, size_t scratch_bytes, slam_stream_t s) {
  if (!ids || !lens || !scratch || B <= 0 || T <= 0 || (int64_t)B * T > 0x7fffffc0LL) return SLAM_EINVAL;
  const int64_t mmax = (((int64_t)B * T + 63) / 64) * 64;
  if (M_packed <= 0 || (M_packed & 63) || M_packed > mmax) return SLAM_EINVAL;
  if (((uintptr_t)scratch & 255) || scratch_bytes < unpad_scratch_bytes(B, T)) return SLAM_EINVAL;
  return unpad_pack(ids, labels, starts, lens, B, T, M_packed, pad_id, unpad_view(scratch, B, T), (hipStream_t)s);
}
int slam_op_unpad_pack(const int64_t* ids, const int64_t* labels, const int32_t* lens, int32_t B, int32_t T, int32_t M_packed,
                       int32_t pad_id, void* scratch, size_t scratch_bytes, slam_stream_t s) {
  return slam_op_unpad_pack_spans(ids, labels, nullptr, lens, B, T, M_packed, pad_id, scratch, scratch_bytes, s);
}

// ---- single-op entry points ------------------------------------------------------------------
int slam_op_gemm_nt(const void* X, const void* W, void* Y, const void* bias, const void* resid, int M, int N, int K,
                    int use_glds, slam_stream_t s) {
  GemmTune t = *gemm_default_tune();  // the process default with the staging mode of this call
  t.glds = use_glds != 0;
  GemmTuneScope scope(&t);
  return gemm_nt((const bf16_t*)X, (const bf16_t*)W, (bf16_t*)Y, (const bf16_t*)bias, (const bf16_t*)resid, M, N, K, (hipStream_t)s);
}
int slam_op_gemm_nt_swiglu(const void* X, const void* W, void* Y, void* act, int M, int N, int K, slam_stream_t s) {
  return gemm_nt_swiglu((const bf16_t*)X, (const bf16_t*)W, (bf16_t*)Y, (bf16_t*)act, M, N, K, (hipStream_t)s);
}
int slam_op_gemm_nt_dswiglu(const void* dY, const void* Wt, void* gu, int M, int I, int H, slam_stream_t s) {
  return gemm_nt_dswiglu((const bf16_t*)dY, (const bf16_t*)Wt, (bf16_t*)gu, M, I, H, (hipStream_t)s);
}
int slam_op_gemm_nn(const void* dY, const void* W, void* dX, const void* resid, int M, int N, int K, slam_stream_t s) {
  return gemm_nn((const bf16_t*)dY, (const bf16_t*)W, (bf16_t*)dX, (const bf16_t*)resid, M, N, K, (hipStream_t)s);
}
size_t slam_op_gemm_tn_workspace(int M, int N, int K) { return gemm_tn_workspace_bytes(M, N, K); }
int slam_op_gemm_tn(const void* dY, const void* X, float* dW, int accumulate, int M, int N, int K, float* ws,
                    slam_stream_t s) {
  // capacity = what slam_op_gemm_tn_workspace(M, N, K) promises (the caller's contract; recomputing the bound here would put
  // a host-side planning sweep into every launch)
  static int cm = 0, cn = 0, ck = 0;
  static size_t cap = 0;
  if (cm != M || cn != N || ck != K) { cap = gemm_tn_workspace_bytes(M, N, K); cm = M; cn = N; ck = K; }
  return gemm_tn((const bf16_t*)dY, (const bf16_t*)X, dW, accumulate, M, N, K, N, K, ws, cap, (hipStream_t)s);
}
int slam_op_gemm_tn_image(const void* dY, const void* X, float* dW, void* dW_bf16, int accumulate, int M, int N, int K, float* ws,
                          int background, slam_stream_t s) {
  const size_t cap = gemm_tn_workspace_bytes(M, N, K);
  return gemm_tn((const bf16_t*)dY, (const bf16_t*)X, dW, accumulate, M, N, K, N, K, ws, cap, (hipStream_t)s, background, (bf16_t*)dW_bf16);
}
size_t slam_op_gemm_skinny_workspace(int M, int N, int K) { return gemm_skinny_workspace_bytes(M, N, K); }
int slam_op_gemm_skinny(const void* X, const void* W, void* Y, int y_f32, const void* bias, const void* resid, int M, int N, int K,
                        float* ws, size_t ws_bytes, slam_stream_t s) {
  return gemm_skinny((const bf16_t*)X, (const bf16_t*)W, y_f32 ? nullptr : (bf16_t*)Y, y_f32 ? (float*)Y : nullptr,
                     (const bf16_t*)bias, (const bf16_t*)resid, M, N, K, ws, ws_bytes, (hipStream_t)s);
}
size_t slam_op_w8_bytes(int N, int K) { return (N <= 0 || K <= 0 || K % W8_K_GRAIN) ? 0 : w8_bytes(N, K); }
size_t slam_op_w8_exps_offset(int N, int K) { return (N <= 0 || K <= 0 || K % W8_K_GRAIN) ? 0 : w8_exps_offset(N, K); }
int slam_op_quantize_rows_fp8(void* W, void* codes, void* exps, int N, int K, slam_stream_t s) {
  const int r = quantize_rows_fp8((bf16_t*)W, (uint8_t*)codes, (int8_t*)exps, N, K, (hipStream_t)s);
  return r == -1 ? SLAM_EINVAL : r;
}
int slam_op_dequantize_rows_fp8(const void* codes, const void* exps, void* W, int N, int K, slam_stream_t s) {
  const int r = dequantize_rows_fp8((const uint8_t*)codes, (const int8_t*)exps, (bf16_t*)W, N, K, (hipStream_t)s);
  return r == -1 ? SLAM_EINVAL : r;
}
int slam_op_gemm_skinny_w8(const void* X, const void* codes, const void* exps, void* Y, int y_f32, const void* bias, const void* resid,
                           int M, int N, int K, float* ws, size_t ws_bytes, slam_stream_t s) {
  const int r = gemm_skinny_w8((const bf16_t*)X, (const uint8_t*)codes, (const int8_t*)exps, y_f32 ? nullptr : (bf16_t*)Y,
                               y_f32 ? (float*)Y : nullptr, (const bf16_t*)bias, (const bf16_t*)resid, M, N, K, ws, ws_bytes,
                               (hipStream_t)s);
  return r == -1 ? SLAM_EINVAL : r;
}
size_t slam_op_score_rows_workspace(int M, int V) { return score_rows_workspace_bytes(M, V); }
int slam_op_score_rows(const void* X, const void* W, const int64_t* targets, const uint8_t* colmask, float* lp, int64_t* argmax,
                       int M, int V, int K, void* ws, size_t ws_bytes, slam_stream_t s) {
  if (!X || !W || !targets || !lp || !ws || M <= 0 || M > SCORE_MAX_M || V <= 0 || V > SCORE_MAX_V || K <= 0 || (K & 7))
    return SLAM_EINVAL;
  if ((((uintptr_t)X | (uintptr_t)W | (uintptr_t)ws) & 15) || (((uintptr_t)targets | (uintptr_t)argmax) & 7) || ((uintptr_t)lp & 3))
    return SLAM_EINVAL;
  if (ws_bytes < score_rows_workspace_bytes(M, V)) return SLAM_EINVAL;
  return score_rows((const bf16_t*)X, (const bf16_t*)W, targets, colmask, M, V, K, nullptr, 0, lp, argmax, ws, ws_bytes,
                    (hipStream_t)s);
}
size_t slam_op_attn_decode_workspace(int B, int nH, int nKV, int head_dim, int kv_bound) {
  if (B <= 0 || nKV <= 0 || kv_bound <= 0) return 0;
  const int chunk = attn_decode_chunk(B, nH, nKV, head_dim, kv_bound, (size_t)-1);
  return attn_decode_op_head(B, head_dim) + attn_decode_part_bytes(B, nH, head_dim, (kv_bound + chunk - 1) / chunk);
}
int slam_op_attn_decode(const float* qkv, const void* bias, const int32_t* lens, void* k_cache, void* v_cache, void* o, void* ws,
                        size_t ws_bytes, int B, int nH, int nKV, int head_dim, int capacity, int kv_bound, float theta,
                        slam_stream_t s) {
  if (!qkv || !lens || !k_cache || !v_cache || !o || !ws || B <= 0 || (head_dim != 64 && head_dim != 128)) return SLAM_EINVAL;
  const size_t head = attn_decode_op_head(B, head_dim);
  if (ws_bytes <= head) return SLAM_ENOMEM;
  hipStream_t st = (hipStream_t)s;
  char* w = (char*)ws;
  int64_t* pos = (int64_t*)w;
  float* tab = (float*)(w + (((size_t)B * 8 + 255) & ~(size_t)255));
  const size_t n = (size_t)B * (head_dim / 2);
  int r = lens_to_pos(lens, pos, B, st);
  if (r) return r;
  r = rope_table(pos, B, 1, head_dim, theta, tab, tab + n, tab + 2 * n, tab + 3 * n, 1.44269504088896340736f / sqrtf((float)head_dim), st);
  if (r) return r;
  return attn_decode(qkv, (const bf16_t*)bias, tab, tab + n, tab + 2 * n, tab + 3 * n, lens, (bf16_t*)k_cache, (bf16_t*)v_cache,
                     capacity, B, nH, nKV, head_dim, kv_bound, (bf16_t*)o, (float*)(w + head), ws_bytes - head, st);
}
size_t slam_op_attn_extend_workspace(int B, int T, int nH, int nKV, int head_dim, int kv_bound) {
  if (B <= 0 || T <= 0 || nH <= 0 || nKV <= 0 || kv_bound <= 0) return 0;
  const int chunk = attn_extend_chunk(B, T, nH, nKV, head_dim, kv_bound, (size_t)-1);
  return attn_extend_part_bytes(B, T, nH, head_dim, (kv_bound + chunk - 1) / chunk);
}
int slam_op_attn_extend(const void* qkv, const int32_t* base_lens, const int32_t* new_lens, void* k_cache, void* v_cache,
                        void* o, void* ws, size_t ws_bytes, int B, int T, int nH, int nKV, int head_dim, int capacity,
                        int kv_bound, slam_stream_t s) {
  if (!qkv || !base_lens || !new_lens || !k_cache || !v_cache || !o || B <= 0 || T <= 0 || nH <= 0 || nKV <= 0) return SLAM_EINVAL;
  if ((head_dim != 64 && head_dim != 128) || nH % nKV || nH / nKV > 8 || kv_bound <= 0 || kv_bound > capacity) return SLAM_EINVAL;
  const int r = attn_extend((const bf16_t*)qkv, base_lens, new_lens, (bf16_t*)k_cache, (bf16_t*)v_cache, capacity, B, T, nH, nKV,
                            head_dim, kv_bound, (bf16_t*)o, (float*)ws, ws ? ws_bytes : 0, (hipStream_t)s);
  return r == -1 ? SLAM_EINVAL : r;
}
int slam_op_rmsnorm_fwd(const void* x, const void* w, void* y, float* rstd, int M, int H, float eps, slam_stream_t s) {
  return rmsnorm_fwd((const bf16_t*)x, (const bf16_t*)w, (bf16_t*)y, rstd, M, H, eps, (hipStream_t)s);
}
size_t slam_op_rmsnorm_bwd_workspace(int M, int H) { return (size_t)rmsnorm_bwd_blocks(M) * H * sizeof(float); }
int slam_op_rmsnorm_bwd(const void* dy, const void* x, const void* w, const float* rstd, const void* dres, void* dx,
                        float* dw, float* ws, int M, int H, slam_stream_t s) {
  return rmsnorm_bwd((const bf16_t*)dy, (const bf16_t*)x, (const bf16_t*)w, rstd, (const bf16_t*)dres, (bf16_t*)dx, dw,
                     0, ws, M, H, (hipStream_t)s);
}
int slam_op_layernorm_fwd(const void* x, const void* w, const void* b, void* y, float* mean, float* rstd, int M, int H, float eps,
                          slam_stream_t s) {
  return layernorm_fwd((const bf16_t*)x, (const bf16_t*)w, (const bf16_t*)b, (bf16_t*)y, mean, rstd, M, H, eps, (hipStream_t)s);
}
size_t slam_op_layernorm_bwd_workspace(int M, int H) { return (size_t)2 * rmsnorm_bwd_blocks(M) * H * sizeof(float); }
int slam_op_layernorm_bwd(const void* dy, const void* x, const void* w, const float* mean, const float* rstd, const void* dres,
                          void* dx, float* dw, float* db, float* ws, int M, int H, slam_stream_t s) {
  const int nb = rmsnorm_bwd_blocks(M);
  float* pw = ws;
  float* pb = ws + (size_t)nb * H;
  int r = layernorm_bwd((const bf16_t*)dy, (const bf16_t*)x, (const bf16_t*)w, mean, rstd, (const bf16_t*)dres, (bf16_t*)dx, pw, pb,
                        M, H, (hipStream_t)s);
  if (r) return r;
  r = colsum_finish_many(pw, 0, nb, H, dw, 0, 1, 0, (hipStream_t)s);
  if (r) return r;
  return colsum_finish_many(pb, 0, nb, H, db, 0, 1, 0, (hipStream_t)s);
}
int slam_op_embed_pos_fwd(const int64_t* ids, const int64_t* position_ids, const void* E, const void* P, void* out, int64_t* prow,
                          int M, int H, int V, int T, int n_rows_p, slam_stream_t s) {
  return embed_pos_fwd(ids, position_ids, (const bf16_t*)E, (const bf16_t*)P, (bf16_t*)out, prow, M, H, V, T, n_rows_p, (hipStream_t)s);
}
int slam_op_embed_fwd(const int64_t* ids, const void* E, void* out, int M, int H, int V, slam_stream_t s) {
  if (!ids || !E || !out || M <= 0 || H <= 0 || (H & 7) || V <= 0) return SLAM_EINVAL;
  return embed_fwd(ids, (const bf16_t*)E, (bf16_t*)out, M, H, V, (hipStream_t)s);
}
int slam_op_embed_noise_fwd(const int64_t* ids, const int64_t* position_ids, const void* E, const void* P, void* out, int64_t* prow,
                            int M, int H, int V, int T, int n_rows_p, float s, int64_t seed, int64_t call, int64_t index0,
                            slam_stream_t stream) {
  if (!ids || !E || !out || M <= 0 || H <= 0 || (H & 7) || V <= 0 || !(s >= 0.f) || !__builtin_isfinite(s) || call < 0 ||
      call > 0xffffffffLL || index0 < 0 || (index0 & 7) || (P && (T <= 0 || n_rows_p <= 0)))
    return SLAM_EINVAL;
  NeftSite n;
  n.s = s;
  n.seed = (uint64_t)seed;
  n.call = (uint32_t)call;
  n.index0 = index0;
  return embed_noise_fwd(ids, position_ids, (const bf16_t*)E, (const bf16_t*)P, (bf16_t*)out, prow, M, H, V, T, n_rows_p, n,
                         (hipStream_t)stream);
}
int slam_op_gemm_nt_relu(const void* X, const void* W, void* act, const void* bias, int M, int N, int K, slam_stream_t s) {
  return gemm_nt_relu((const bf16_t*)X, (const bf16_t*)W, (bf16_t*)act, (const bf16_t*)bias, M, N, K, (hipStream_t)s);
}
int slam_op_gemm_nt_drelu(const void* dY, const void* Wt, void* dact, const void* act, int M, int N, int K, slam_stream_t s) {
  return gemm_nt_drelu((const bf16_t*)dY, (const bf16_t*)Wt, (bf16_t*)dact, (const bf16_t*)act, M, N, K, (hipStream_t)s);
}
int slam_op_relu_bwd(void* d, const void* act, int64_t n, slam_stream_t s) {
  if (n < 0) return SLAM_EINVAL;
  return relu_bwd((bf16_t*)d, (const bf16_t*)act, (size_t)n, (hipStream_t)s);
}
int slam_op_rope(void* qkv, int ld, int M, int T, int n_rot_heads, int head_dim, const int64_t* position_ids, float theta,
                 int backward, float* cs_ws, slam_stream_t s) {
  const size_t half = (size_t)head_dim / 2;
  int r = rope_table(position_ids, M, T, head_dim, theta, cs_ws, cs_ws + (size_t)M * half, nullptr, nullptr, 1.f, (hipStream_t)s);
  if (r) return r;
  return rope_apply((bf16_t*)qkv, ld, M, n_rot_heads, head_dim, cs_ws, cs_ws + (size_t)M * half, backward, (hipStream_t)s);
}
int slam_op_qknorm_rope_fwd(void* qkv, const void* w_q, const void* w_k, const int64_t* position_ids, float theta, float eps,
                            int M, int T, int nH, int nKV, int head_dim, void* raw_out, float* rstd_out, float* table_ws,
                            slam_stream_t s) {
  if (!qkv || !w_q || !w_k || !table_ws || T <= 0 || !qknorm_dims_ok(M, nH, nKV, head_dim)) return SLAM_EINVAL;
  const size_t n = (size_t)M * (head_dim / 2);
  const float qscale = 1.44269504088896340736f / sqrtf((float)head_dim);
  int r = rope_table(position_ids, M, T, head_dim, theta, table_ws, table_ws + n, table_ws + 2 * n, table_ws + 3 * n, qscale, (hipStream_t)s);
  if (r) return r;
  r = qknorm_rope_fwd((bf16_t*)qkv, (nH + 2 * nKV) * head_dim, M, nH, nKV, head_dim, (const bf16_t*)w_q, (const bf16_t*)w_k, table_ws,
                      table_ws + n, table_ws + 2 * n, table_ws + 3 * n, eps, (bf16_t*)raw_out, rstd_out, (hipStream_t)s);
  return r == -1 ? SLAM_EINVAL : r;
}
size_t slam_op_qknorm_bwd_workspace(int M, int nH, int nKV, int head_dim) {
  if (!qknorm_dims_ok(M, nH, nKV, head_dim)) return 0;
  return (size_t)2 * qknorm_bwd_blocks(M, nH, nKV, head_dim) * head_dim * sizeof(float);
}
int slam_op_qknorm_bwd(void* dqkv, const void* raw, const float* rstd, const void* w_q, const void* w_k, float* dw_q, float* dw_k,
                       float* ws, int M, int nH, int nKV, int head_dim, slam_stream_t s) {
  if (!dqkv || !raw || !rstd || !w_q || !w_k || !dw_q || !dw_k || !ws || !qknorm_dims_ok(M, nH, nKV, head_dim)) return SLAM_EINVAL;
  const int nb = qknorm_bwd_blocks(M, nH, nKV, head_dim);
  float* pk = ws + (size_t)nb * head_dim;
  int r = qknorm_bwd((bf16_t*)dqkv, (nH + 2 * nKV) * head_dim, M, nH, nKV, head_dim, (const bf16_t*)raw, rstd, (const bf16_t*)w_q,
                     (const bf16_t*)w_k, nb, ws, pk, (hipStream_t)s);
  if (r) return r == -1 ? SLAM_EINVAL : r;
  r = colsum_finish_many(ws, 0, nb, head_dim, dw_q, 0, 1, 0, (hipStream_t)s);
  if (r) return r;
  return colsum_finish_many(pk, 0, nb, head_dim, dw_k, 0, 1, 0, (hipStream_t)s);
}
int slam_op_qknorm_rows_f32(float* qkv, const void* w_q, const void* w_k, float eps, int B, int nH, int nKV, int head_dim,
                            slam_stream_t s) {
  if (!qkv || !w_q || !w_k || !qknorm_dims_ok(B, nH, nKV, head_dim)) return SLAM_EINVAL;
  const int r = qknorm_rows_f32(qkv, (nH + 2 * nKV) * head_dim, B, nH, nKV, head_dim, (const bf16_t*)w_q, (const bf16_t*)w_k, eps,
                                (hipStream_t)s);
  return r == -1 ? SLAM_EINVAL : r;
}
int slam_op_swiglu_fwd(const void* gu, void* act, int M, int I, slam_stream_t s) {
  return swiglu_fwd((const bf16_t*)gu, (bf16_t*)act, M, I, I, (hipStream_t)s);
}
int slam_op_swiglu_bwd(void* gu, const void* dact, int M, int I, slam_stream_t s) {
  return swiglu_bwd((bf16_t*)gu, (const bf16_t*)dact, M, I, I, (hipStream_t)s);
}
int slam_op_attn_fwd(const void* qkv, void* o, float* lse2, const int32_t* seg_start, int M, int nH, int nKV,
                     int head_dim, slam_stream_t s) {
  // the forward runs in the engine's heaviest-first block order; the op entry keeps a process-lifetime plan buffer for it
  static int* plan = nullptr;
  static size_t cap = 0;
  const size_t need = attn_plan_ints(M);
  if (need > cap) {
    if (plan) (void)hipFree(plan);
    if (hipMalloc(&plan, need * sizeof(int)) != hipSuccess) { plan = nullptr; cap = 0; return (int)hipErrorOutOfMemory; }
    cap = need;
  }
  const AttnTune tune = attn_default_tune();
  int r = attn_plan(seg_start, nullptr, M, head_dim, tune, plan, (hipStream_t)s);
  if (r) return r;
  return attn_fwd((const bf16_t*)qkv, (bf16_t*)o, lse2, seg_start, plan, tune, M, nH, nKV, head_dim, (hipStream_t)s);
}
size_t slam_op_attn_bwd_workspace(int M, int nH, int head_dim) {
  // the ABI call has no KV-head count: sized for nKV = nH (plain multi-head attention), the largest case
  return attn_bwd_workspace_bytes(M, nH, head_dim) + (size_t)2 * M * nH * sizeof(float) + attn_plan_ints(M) * sizeof(int) + 64;
}
int slam_op_attn_bwd(const void* qkv, const void* o, const void* d_o, const float* lse2, void* dqkv, float* ws,
                     const int32_t* seg_start, const int32_t* seg_end, int M, int nH, int nKV, int head_dim,
                     slam_stream_t s) {
  float* ndsum = ws;
  float* nlse = ws + (size_t)M * nH;
  float* part = ws + (size_t)2 * M * nH;
  int* plan = reinterpret_cast<int*>(part + attn_bwd_workspace_bytes(M, nH, head_dim) / sizeof(float));
  const AttnTune tune = attn_default_tune();
  int r = attn_plan(seg_start, seg_end, M, head_dim, tune, plan, (hipStream_t)s);
  if (r) return r;
  return attn_bwd((const bf16_t*)qkv, (const bf16_t*)o, (const bf16_t*)d_o, lse2, ndsum, nlse, (bf16_t*)dqkv, part, seg_start,
                  seg_end, plan, tune, nullptr, nullptr, M, nH, nKV, head_dim, (hipStream_t)s);
}
// the backward as slam_backward runs it: dq / dk leave rotated back through the cos / sin tables of the rows' positions
int slam_op_attn_bwd_rope(const void* qkv, const void* o, const void* d_o, const float* lse2, void* dqkv, float* ws,
                          const int32_t* seg_start, const int32_t* seg_end, const int64_t* position_ids, int T, float theta,
                          int M, int nH, int nKV, int head_dim, float* table_ws, slam_stream_t s) {
  if (!qkv || !o || !d_o || !lse2 || !dqkv || !ws || !seg_start || !seg_end || !table_ws) return SLAM_EINVAL;
  if (M <= 0 || nH <= 0 || nKV <= 0 || nH % nKV || (head_dim != 64 && head_dim != 128)) return SLAM_EINVAL;
  if (!position_ids && T <= 0) return SLAM_EINVAL;
  float* cs = table_ws;
  float* sn = table_ws + (size_t)M * (head_dim / 2);
  int r = rope_table(position_ids, M, T, head_dim, theta, cs, sn, nullptr, nullptr, 1.f, (hipStream_t)s);
  if (r) return r;
  float* ndsum = ws;
  float* nlse = ws + (size_t)M * nH;
  float* part = ws + (size_t)2 * M * nH;
  int* plan = reinterpret_cast<int*>(part + attn_bwd_workspace_bytes(M, nH, head_dim) / sizeof(float));
  const AttnTune tune = attn_default_tune();
  r = attn_plan(seg_start, seg_end, M, head_dim, tune, plan, (hipStream_t)s);
  if (r) return r;
  return attn_bwd((const bf16_t*)qkv, (const bf16_t*)o, (const bf16_t*)d_o, lse2, ndsum, nlse, (bf16_t*)dqkv, part, seg_start,
                  seg_end, plan, tune, cs, sn, M, nH, nKV, head_dim, (hipStream_t)s);
}
// the QKV projection of the head_dim-64 models: bias + rotate-half RoPE + the query heads' pre-scale in the GEMM epilogue
int slam_op_gemm_nt_rope(const void* X, const void* W, void* Y, const void* bias, const int64_t* position_ids, float theta,
                         int q_heads, int rope_heads, int M, int T, int N, int K, float* table_ws, slam_stream_t s) {
  if (!X || !W || !Y || !table_ws || M <= 0 || N <= 0 || K <= 0) return SLAM_EINVAL;
  if ((K % 64) || (N % 128)) return SLAM_EINVAL;  // the shapes slam_forward routes to gemm_nt + rope_apply
  if (q_heads < 0 || rope_heads < q_heads || (size_t)rope_heads * 64 > (size_t)N) return SLAM_EINVAL;
  if (!position_ids && T <= 0) return SLAM_EINVAL;
  const size_t n = (size_t)M * 32;
  float *cs = table_ws, *sn = table_ws + n, *csq = table_ws + 2 * n, *snq = table_ws + 3 * n;
  int r = rope_table(position_ids, M, T, 64, theta, cs, sn, csq, snq, 1.44269504088896340736f / sqrtf(64.f), (hipStream_t)s);
  if (r) return r;
  return gemm_nt_rope((const bf16_t*)X, (const bf16_t*)W, (bf16_t*)Y, (const bf16_t*)bias, cs, sn, csq, snq, q_heads, rope_heads,
                      M, N, K, (hipStream_t)s);
}
// a bias gradient as slam_backward forms it: partial rows per row block, then the fixed-order finish
size_t slam_op_colsum_workspace(int M, int N) {
  if (M <= 0 || N <= 0) return 0;
  return (size_t)colsum_blocks(M) * N * sizeof(float);
}
int slam_op_colsum(const void* X, int ld, int M, int N, float* out, int accumulate, float* ws, slam_stream_t s) {
  if (!X || !out || !ws || M <= 0 || N <= 0 || ld < N) return SLAM_EINVAL;
  if ((N % 8) || (ld % 8)) return SLAM_EINVAL;  // the kernel reads 16-byte chunks
  int r = colsum_bf16((const bf16_t*)X, ld, M, N, nullptr, 1, ws, (hipStream_t)s);
  if (r) return r;
  return colsum_finish_many(ws, 0, colsum_blocks(M), N, out, 0, 1, accumulate != 0, (hipStream_t)s);
}
int slam_op_cross_entropy(const void* logits, const int64_t* labels, double num_items, void* dlogits, float* row_loss,
                          float* scratch2, int B, int T, int Vp, int V, slam_stream_t s) {
  return cross_entropy((const bf16_t*)logits, labels, num_items, (bf16_t*)dlogits, row_loss, scratch2, scratch2 + 1, B,
                       T, Vp, V, nullptr, 0.f, nullptr, (hipStream_t)s);
}
int slam_op_cross_entropy_smooth(const void* logits, const int64_t* labels, double num_items, void* dlogits, float* row_loss,
                                 float* row_smooth, float* scratch2, int B, int T, int Vp, int V, float epsilon,
                                 slam_stream_t s) {
  if (!logits || !labels || !row_loss || !scratch2 || B <= 0 || T <= 0 || V <= 0) return SLAM_EINVAL;
  if (!(epsilon >= 0.f && epsilon < 1.f) || (epsilon > 0.f && !row_smooth)) return SLAM_EINVAL;
  return cross_entropy((const bf16_t*)logits, labels, num_items, (bf16_t*)dlogits, row_loss, scratch2, scratch2 + 1, B,
                       T, Vp, V, nullptr, epsilon, row_smooth, (hipStream_t)s);
}
// the movers and scalers of the logits / d-logits buffer (slam_forward's logits_out, slam_backward's grad_scale, the DPO row weights)
int slam_op_copy_cols(const void* src, int ld_src, void* dst, int ld_dst, int M, int ncols, slam_stream_t s) {
  if (!src || !dst || M <= 0 || ncols <= 0 || ld_src < ncols || ld_dst < ncols) return SLAM_EINVAL;
  return copy_cols((const bf16_t*)src, ld_src, (bf16_t*)dst, ld_dst, M, ncols, (hipStream_t)s);
}
int slam_op_unpad_logits_spans(const void* src, int Vp, void* dst, int V, const int32_t* off, const int32_t* starts, int B, int T,
                               int Mp, slam_stream_t s) {
  if (!src || !dst || !off || B <= 0 || T <= 0 || Mp <= 0 || V <= 0 || V > Vp || (Vp & 7)) return SLAM_EINVAL;
  return unpad_logits((const bf16_t*)src, Vp, (bf16_t*)dst, V, off, starts, B, T, Mp, (hipStream_t)s);
}
int slam_op_unpad_logits(const void* src, int Vp, void* dst, int V, const int32_t* off, int B, int T, int Mp, slam_stream_t s) {
  return slam_op_unpad_logits_spans(src, Vp, dst, V, off, nullptr, B, T, Mp, s);
}
int slam_op_scale_bf16(void* x, int64_t n, float scale, slam_stream_t s) {
  if (!x || n <= 0 || (n & 7)) return SLAM_EINVAL;  // the kernel goes in 16-byte chunks
  return scale_bf16((bf16_t*)x, (size_t)n, scale, (hipStream_t)s);
}
int slam_op_scale_rows_bf16(void* x, const float* coef, int M, int T, int ncols, slam_stream_t s) {
  if (!x || !coef || M <= 0 || T <= 0 || ncols <= 0 || (ncols & 7)) return SLAM_EINVAL;
  return scale_rows_bf16((bf16_t*)x, coef, M, T, ncols, (hipStream_t)s);
}
int slam_op_scale_rows_unpadded_bf16(void* x, const float* coef, const int32_t* row, int Mp, int ncols, slam_stream_t s) {
  if (!x || !coef || !row || Mp <= 0 || ncols <= 0 || (ncols & 7)) return SLAM_EINVAL;
  return scale_rows_unpadded_bf16((bf16_t*)x, coef, row, Mp, ncols, (hipStream_t)s);
}
size_t slam_op_embed_bwd_workspace(int M, int Vp) { return embed_bwd_workspace_ints(M, Vp) * sizeof(int); }
int slam_op_embed_bwd(const int64_t* ids, const void* dh, float* dE, int M, int H, int Vp, int V, int pad_id, void* ws,
                      slam_stream_t s) {
  return embed_bwd(ids, (const bf16_t*)dh, dE, M, H, Vp, V, pad_id, (int*)ws, (hipStream_t)s);
}
int slam_op_sr_round_bf16(const float* x, void* y_bf16, int64_t n, int64_t index0, int64_t seed, int32_t step, int32_t which,
                          slam_stream_t s) {
  if (!x || !y_bf16 || n < 0 || index0 < 0 || step < 1 || which < 0 || which > 2) return SLAM_EINVAL;
  return sr_round_bf16(x, (bf16_t*)y_bf16, (size_t)n, index0, (uint64_t)seed, step, which, (hipStream_t)s);
}

int slam_op_dropout_add(void* y, const void* resid, int M, int H, int32_t thr16, int64_t seed, int64_t call, int32_t stream_id,
                        int64_t index0, slam_stream_t s) {
  DropSite d;
  if (!y || !resid || !drop_site_ok(M, H, thr16, call, stream_id, index0, &d)) return SLAM_EINVAL;
  d.seed = (uint64_t)seed;
  return dropout_add((bf16_t*)y, (const bf16_t*)resid, M, H, d, (hipStream_t)s);
}
int slam_op_dropout_bwd(const void* dy, void* dy_masked, int M, int H, int32_t thr16, int64_t seed, int64_t call, int32_t stream_id,
                        int64_t index0, slam_stream_t s) {
  DropSite d;
  if (!dy || !dy_masked || dy == dy_masked || !drop_site_ok(M, H, thr16, call, stream_id, index0, &d)) return SLAM_EINVAL;
  d.seed = (uint64_t)seed;
  return dropout_bwd((const bf16_t*)dy, (bf16_t*)dy_masked, M, H, d, (hipStream_t)s);
}

}  // extern "C"
