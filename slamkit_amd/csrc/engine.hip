// C ABI + step orchestration of the Slam engine (see include/slam_engine.h).
// Replaces everything below UnitLM.forward / Trainer.training_step in the reference call stack
// (SURVEY.md §3.1-3.2): Qwen2Model.forward (modeling_qwen2.py:342-402), the tied lm_head (:465),
// compute_loss (unit_lm.py:13-29), autograd backward, clip_grad_norm_ and AdamW.
// This file: the engine's state (create / destroy / bind / layout, the workspace carve, slam_set_option), its streams and
// events, the forward, the backward and the loss side. KV-cached generation is engine_cache.hip, the optimizer entry points
// engine_optim.hip, the RCCL exchange engine_comm.hip; the single-op doors (ops.hip) and the token-choice entry points
// (sampling.hip) never touch a SlamEngine. engine_impl.h is what the four engine files share.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include "engine_impl.h"

namespace {

// an identity rotation: cs = 1, sn = 0, and the query tables carry only the pre-scale (OPT has no RoPE; the attention
// kernels still take their queries pre-scaled and attn_bwd rotates dq / dk back through these tables)
__global__ void ident_rope_kernel(float* cs, float* sn, float* csq, float* snq, size_t n, float qscale) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  cs[i] = 1.f;
  sn[i] = 0.f;
  csq[i] = qscale;
  snq[i] = 0.f;
}

__global__ void seg_fill_kernel(int* seg_start, int* seg_end, int M, int T) {
  int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  int s = (m / T) * T;
  seg_start[m] = s;
  seg_end[m] = s + T;
}

struct Carver {
  char* base;
  size_t off = 0;
  template <typename T>
  T* take(size_t n) {
    off = (off + 255) & ~(size_t)255;
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += n * sizeof(T);
    return p;
  }
};

size_t max_gemm_ws(const SlamEngine* e, int M) {
  const SlamModelDesc& d = e->d;
  size_t w = 0;
  auto upd = [&](int N, int K) { size_t b = gemm_tn_workspace_bytes(M, N, K); if (b > w) w = b; };
  upd(e->QKV, d.hidden);
  upd(d.hidden, d.n_heads * d.head_dim);
  upd(2 * d.intermediate, d.hidden);
  upd(d.hidden, d.intermediate);
  upd(e->vpad, d.hidden);
  return w;
}

size_t carve(SlamEngine* e, char* base, int64_t Mmax) {
  const SlamModelDesc& d = e->d;
  const size_t M = (size_t)Mmax, H = d.hidden, I = d.intermediate, L = d.n_layers;
  Carver c{base};
  e->hs.resize(L + 1);
  e->la.resize(L);
  for (size_t l = 0; l <= L; ++l) e->hs[l] = c.take<bf16_t>(M * H);
  const bool opt = e->arch == 1;
  // "recompute": layer l shares the buffers named by the level with every layer l' = l (mod S); the first S layers carve them
  const int rc = e->recompute;
  const size_t S = rc ? (L < RC_SLOTS ? L : (size_t)RC_SLOTS) : L;
  for (size_t l = 0; l < L; ++l) {
    LayerAct& a = e->la[l];
    const LayerAct* s = l < S ? nullptr : &e->la[l % S];  // the layer that carved this layer's slot
    const bool all = s && rc == 2, xs = s && rc >= 1, as = s && (rc == 2 || (rc == 1 && !opt));
    a.hmid = all ? s->hmid : c.take<bf16_t>(M * H);
    a.x1 = xs ? s->x1 : c.take<bf16_t>(M * H);
    a.x2 = xs ? s->x2 : c.take<bf16_t>(M * H);
    a.qkv = all ? s->qkv : c.take<bf16_t>(M * e->QKV);
    a.o = all ? s->o : c.take<bf16_t>(M * d.n_heads * d.head_dim);
    a.gu = all ? s->gu : c.take<bf16_t>(M * (opt ? 1 : 2) * I);
    a.act = as ? s->act : c.take<bf16_t>(M * I);
    a.rstd1 = all ? s->rstd1 : c.take<float>(M);
    a.rstd2 = all ? s->rstd2 : c.take<float>(M);
    a.lse = all ? s->lse : c.take<float>(M * d.n_heads);
    if (opt) {
      a.mu1 = all ? s->mu1 : c.take<float>(M);
      a.mu2 = all ? s->mu2 : c.take<float>(M);
    }
    if (e->arch == 3) {  // kept per layer wherever qkv is: backward needs xhat of the heads the in-place store overwrote
      const size_t nQK = (size_t)d.n_heads + d.n_kv_heads;
      a.qk_raw = all ? s->qk_raw : c.take<bf16_t>(M * nQK * d.head_dim);
      a.qk_rstd = all ? s->qk_rstd : c.take<float>(M * nQK);
    }
  }
  e->hf = c.take<bf16_t>(M * H);
  e->rstdf = c.take<float>(M);
  if (opt) {
    e->muf = c.take<float>(M);
    e->prow = c.take<int64_t>(M);
  }
  const size_t VP = (size_t)e->vpad;
  // ONE [M][Vp] buffer: the loss kernel replaces the logits with d loss / d logits in place (2 x 5 GB -> 5 GB at
  // M = 16384, Vp = 152,320); callers that want the logits get their copy before the loss runs
  e->logits = c.take<bf16_t>(M * VP);
  e->dlogits = e->logits;
  // OPT: the position table's scatter shares the scatter workspace with the large-vocabulary one (in order, on one stream)
  const int scatter_rows = opt ? (e->vpad == VPAD_SMALL || e->npos > e->vpad ? e->npos : e->vpad) : e->vpad;
  e->onehot = e->vpad == VPAD_SMALL ? c.take<bf16_t>(M * VP) : nullptr;
  e->embed_ws = nullptr;
  if (e->vpad != VPAD_SMALL || opt) e->embed_ws = c.take<int>(embed_bwd_workspace_ints((int)M, scatter_rows));
  e->row_loss = c.take<float>(M);
  e->dh_a = c.take<bf16_t>(M * H);
  e->dx = c.take<bf16_t>(M * H);
  e->dact = c.take<bf16_t>(M * I);
  e->dqkv = c.take<bf16_t>(M * e->QKV);
  e->d_o = c.take<bf16_t>(M * d.n_heads * d.head_dim);
  e->dsum = c.take<float>(M * d.n_heads);
  e->nlse = c.take<float>(M * d.n_heads);
  e->dkv_part = c.take<float>(attn_bwd_workspace_bytes((int)M, d.n_kv_heads, d.head_dim) / sizeof(float));
  e->cosb = c.take<float>(M * (d.head_dim / 2));
  e->sinb = c.take<float>(M * (d.head_dim / 2));
  e->cosq = c.take<float>(M * (d.head_dim / 2));
  e->sinq = c.take<float>(M * (d.head_dim / 2));
  e->seg_s = c.take<int>(M);
  e->seg_e = c.take<int>(M);
  e->attn_plan_buf = c.take<int>(attn_plan_ints((int)M));
  e->gemm_ws_bytes = max_gemm_ws(e, (int)M);
  e->gemm_ws = c.take<float>(e->gemm_ws_bytes / sizeof(float));
  size_t part = (size_t)rmsnorm_bwd_blocks((int)M) * H;
  size_t part2 = (size_t)colsum_blocks((int)M) * e->QKV;
  if (part2 > part) part = part2;
  if (part < 1024) part = 1024;
  const size_t n_chunks = ((size_t)e->n_params + grad_chunk_elems() - 1) / grad_chunk_elems();  // gradient-norm chunk sums
  if (part < n_chunks) part = n_chunks;
  if (opt && part < 2 * (size_t)rmsnorm_bwd_blocks((int)M) * H) part = 2 * (size_t)rmsnorm_bwd_blocks((int)M) * H;  // final LN: dw | db
  e->part_ws = c.take<float>(part);
  e->ln_ps = (size_t)rmsnorm_bwd_blocks((int)M) * H;
  e->bias_ps = (size_t)colsum_blocks((int)M) * e->QKV;
  e->ln_part = c.take<float>(e->ln_ps * 2 * L);
  e->bias_part = c.take<float>(e->bias_ps * L);
  if (opt) {
    e->hb_ps = (size_t)colsum_blocks((int)M) * H;
    e->ib_ps = (size_t)colsum_blocks((int)M) * I;
    e->lnb_part = c.take<float>(e->ln_ps * 2 * L);
    e->bo_part = c.take<float>(e->hb_ps * L);
    e->b1_part = c.take<float>(e->ib_ps * L);
    e->b2_part = c.take<float>(e->hb_ps * L);
  }
  {  // GradSink slots of one backward: every launch that stores final gradient values, under any plan
    const size_t HD = (size_t)d.n_heads * d.head_dim;
    size_t emb = gemm_tn_sumsq_slots(e->vpad, (int)H);
    const size_t conv = (size_t)f32_to_bf16_sumsq_slots((size_t)e->vpad * H);
    if (conv > emb) emb = conv;
    size_t per_layer = gemm_tn_sumsq_slots(e->QKV, (int)H) + gemm_tn_sumsq_slots((int)H, (int)HD) +
                       gemm_tn_sumsq_slots((int)(2 * I), (int)H) + gemm_tn_sumsq_slots((int)H, (int)I) +
                       2 * ((H + 15) / 16) + ((size_t)e->QKV + 15) / 16;
    size_t tail = (H + 15) / 16;
    if (e->untied) tail += gemm_tn_sumsq_slots(e->vpad, (int)H);  // the head's gradient is a final store of its own
    if (opt) {  // + fc1 at N = I, the LayerNorm biases, bo, b1, b2, the final norm's bias and the position table's conversion
      per_layer += gemm_tn_sumsq_slots((int)I, (int)H) + 2 * ((H + 15) / 16) + 2 * ((H + 15) / 16) + (I + 15) / 16;
      tail += (H + 15) / 16 + (size_t)f32_to_bf16_sumsq_slots((size_t)e->npos * H) + (size_t)e->npos * H / grad_chunk_elems() + 1;
    }
    e->gn_cap = emb + L * per_layer + tail + 64;
    e->gn_part = c.take<float>(e->gn_cap);
  }
  e->scal = c.take<float>(64);
  // "dropout_thr16" != 0: the masked residual gradients, behind everything else (the layout above is the same with and without)
  for (int p = 0; p < 2; ++p)
    for (int s = 0; s < 2; ++s) e->dmask[p][s] = e->dropout_thr16 ? c.take<bf16_t>(M * H) : nullptr;
  return (c.off + 255) & ~(size_t)255;
}

void add_tensor(SlamEngine* e, const std::string& name, int64_t& off, int64_t rows, int64_t cols) {
  SlamTensorInfo t;
  memset(&t, 0, sizeof(t));
  snprintf(t.name, sizeof(t.name), "%s", name.c_str());
  t.offset = off;
  t.rows = rows;
  t.cols = cols;
  e->tensors.push_back(t);
  off += rows * cols;
}

const char* const kFamName[F_COUNT] = {
    "qkv_fwd", "attn_fwd", "o_fwd", "gateup_fwd", "down_fwd", "norm_fwd", "head_fwd", "loss",
    "down_dgrad_dswiglu", "gateup_dgrad", "o_dgrad", "qkv_dgrad", "attn_bwd", "norm_bwd", "head_dgrad",
    "wd_wgrad", "wgu_wgrad", "wo_wgrad", "wqkv_wgrad", "head_wgrad", "embed_wgrad"};

int ensure_wside(SlamEngine* h) {
  if (h->wside && h->wside_cus_applied == h->wside_cus) return 0;
  hipError_t e;
  if (h->wside) {  // the mask changed: replace the stream
    (void)hipStreamSynchronize(h->wside);
    (void)hipStreamDestroy(h->wside);
    h->wside = nullptr;
  }
  if (h->wside_cus > 0) {
    uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int n = h->wside_cus > 256 ? 256 : h->wside_cus;
    for (int i = 0; i < n; ++i) mask[i >> 5] |= 1u << (i & 31);
    e = hipExtStreamCreateWithCUMask(&h->wside, 8, mask);
  } else {
    e = hipStreamCreateWithFlags(&h->wside, hipStreamNonBlocking);
  }
  if (e != hipSuccess) return (int)e;
  h->wside_cus_applied = h->wside_cus;
  if (h->ev_w.empty()) {
    h->ev_w.resize((size_t)(h->d.n_layers + 1) * 8);
    for (auto& ev : h->ev_w) {
      e = hipEventCreateWithFlags(&ev, sync_event_flags());
      if (e != hipSuccess) return (int)e;
    }
  }
  return 0;
}

// Qwen3: blocks of the q / k norm backward over M tokens - what the kernel would like, capped so that the two partial slabs
// fit the layer's (otherwise unused) bias slab of colsum_blocks(M) x QKV floats: at least 3 / 2 colsum_blocks(M) blocks
int qn_blocks(const SlamEngine* h, int M) {
  const SlamModelDesc& d = h->d;
  const int want = qknorm_bwd_blocks(M, d.n_heads, d.n_kv_heads, d.head_dim);
  const int cap = (int)((size_t)colsum_blocks(M) * h->QKV / (2 * (size_t)d.head_dim));
  return want < cap ? want : cap;
}

}  // namespace

namespace slam_impl {  // what the other engine files call too (engine_impl.h)

// Flags of the events that only order the engine's streams among themselves. Without hipEventDisableSystemFence every
// hipEventRecord carries a SYSTEM-scope release - cache write-back and invalidation in the middle of the backward, seven
// times per layer; nothing on the host reads device memory through these events (SLAM_EVENT_SYSTEM_FENCE=1 restores it).
unsigned sync_event_flags() {
  static const unsigned f = [] {
    const char* e = getenv("SLAM_EVENT_SYSTEM_FENCE");
    return (unsigned)hipEventDisableTiming | ((e && e[0] == '1') ? 0u : (unsigned)hipEventDisableSystemFence);
  }();
  return f;
}

// first event of a timing pair around a launch of family `fam` on `st`; returns the pair's slot, -1 when timing is off or failed
int fam_begin(SlamEngine* h, int fam, hipStream_t st) {
  if (!h->time_families) return -1;
  const size_t at = h->fam_marks.size() * 2;
  while (h->fam_ev.size() < at + 2) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return -1;
    h->fam_ev.push_back(e);
  }
  if (hipEventRecord(h->fam_ev[at], st) != hipSuccess) return -1;
  h->fam_marks.push_back({fam, at});
  return (int)at;
}
void fam_end(SlamEngine* h, int slot, hipStream_t st) {
  if (slot >= 0) (void)hipEventRecord(h->fam_ev[(size_t)slot + 1], st);
}

int ensure_side(SlamEngine* h) {
  if (h->side) return 0;
  hipError_t e = hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking);
  if (e != hipSuccess) return (int)e;
  e = hipEventCreateWithFlags(&h->ev_fork, sync_event_flags());
  if (e != hipSuccess) return (int)e;
  h->ev_chunk.resize(h->d.n_layers + 2);
  for (auto& ev : h->ev_chunk) {
    e = hipEventCreateWithFlags(&ev, sync_event_flags());
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}
// make `st` wait for chunk i of a pending overlapped optimizer step
int wait_chunk(SlamEngine* h, int i, hipStream_t st) {
  if (!h->opt_pending) return 0;
  return (int)hipStreamWaitEvent(st, h->ev_chunk[i], 0);
}
// ... for all of it (the chunks are recorded in order on one stream: the last event covers them)
int join_optimizer(SlamEngine* h, hipStream_t st) {
  if (!h->opt_pending) return 0;
  h->opt_pending = false;
  return (int)hipStreamWaitEvent(st, h->ev_chunk.back(), 0);
}

// make `st` wait for the pending writers of parameters in [lo, hi); the stall is bracketed by two timing events
int wait_params(SlamEngine* h, int64_t lo, int64_t hi, hipStream_t st) {
  for (size_t i = 0; i < h->pwaits.size();) {
    SlamEngine::ParamWait& w = h->pwaits[i];
    if (w.lo < hi && lo < w.hi) {
      hipError_t r;
      // two timing events per wait are two more packets on the caller's stream: measurement runs only. The pool is read and
      // reset by slam_param_wait_ms. A caller that reads rarely (logging_steps >> 80) fills it: the pairs that have completed
      // - all but the last step's - are folded into a running sum and their slots reused, so the reported total stays complete;
      // a wait that still finds no slot is counted in pw_untimed (slam_param_wait_untimed) instead of vanishing
      if (h->time_param_waits && h->pw_used + 2 > 4096) {
        size_t keep = 0;
        for (size_t k = 0; k + 1 < h->pw_used; k += 2) {
          float ms = 0.f;
          if (hipEventQuery(h->pw_ev[k + 1]) == hipSuccess && hipEventElapsedTime(&ms, h->pw_ev[k], h->pw_ev[k + 1]) == hipSuccess) {
            h->pw_acc_ms += ms;
          } else {  // still in flight: keep the pair (swap it to the front)
            std::swap(h->pw_ev[keep], h->pw_ev[k]);
            std::swap(h->pw_ev[keep + 1], h->pw_ev[k + 1]);
            keep += 2;
          }
        }
        h->pw_used = keep;
        if (h->pw_used + 2 > 4096) ++h->pw_untimed;
      }
      if (h->time_param_waits && h->pw_used + 2 <= 4096) {
        if (h->pw_used + 2 > h->pw_ev.size()) {
          for (int k = 0; k < 2; ++k) {
            hipEvent_t e;
            r = hipEventCreate(&e);
            if (r != hipSuccess) return (int)r;
            h->pw_ev.push_back(e);
          }
        }
        r = hipEventRecord(h->pw_ev[h->pw_used], st);
        if (r == hipSuccess) r = hipStreamWaitEvent(st, w.ev, 0);
        if (r == hipSuccess) r = hipEventRecord(h->pw_ev[h->pw_used + 1], st);
        h->pw_used += 2;
      } else {
        r = hipStreamWaitEvent(st, w.ev, 0);
      }
      if (r != hipSuccess) return (int)r;
      h->pwaits.erase(h->pwaits.begin() + i);
    } else {
      ++i;
    }
  }
  return 0;
}
int join_params(SlamEngine* h, hipStream_t st) { return h->pwaits.empty() ? 0 : wait_params(h, 0, h->n_params, st); }

// The family's row norm over M rows: LayerNorm with a bias and a saved mean (OPT; boff and mu are OPT's alone), else RMSNorm
int norm_fwd(SlamEngine* h, const bf16_t* x, int64_t woff, int64_t boff, bf16_t* y, float* mu, float* rstd, int M, hipStream_t st) {
  const bf16_t* P = h->params;
  if (h->arch == 1) return layernorm_fwd(x, P + woff, P + boff, y, mu, rstd, M, h->d.hidden, h->d.rms_eps, st);
  return rmsnorm_fwd(x, P + woff, y, rstd, M, h->d.hidden, h->d.rms_eps, st);
}

}  // namespace slam_impl

namespace {

// One decoder layer's forward launches over M tokens: hs[l] -> la[l] (-> hs[l + 1]). The one body that slam_forward,
// slam_prefill and the recomputation in slam_backward share, so a re-run issues the forward's own calls in the forward's own
// order. `rerun` (backward, "recompute" = 2): the layer's parameters are already final for this step (no chunk / parameter
// waits), the gate|up timing events are left alone and the down projection is skipped - its only output is hs[l + 1], which
// backward no longer needs and already re-uses as the gradient of hmid. The caller holds the GemmTuneScope.
int layer_forward(SlamEngine* h, int l, int M, bool rerun, hipStream_t st) {
  const SlamModelDesc& d = h->d;
  const int H = d.hidden, I = d.intermediate, L = d.n_layers, nH = d.n_heads, nKV = d.n_kv_heads;
  const bf16_t* P = h->params;
  const float qscale = 1.44269504088896340736f / sqrtf((float)d.head_dim);
  const bool opt = h->arch == 1;
  const LayerOff& o = h->lo[l];
  LayerAct& a = h->la[l];
  if (!rerun) {
    CK(wait_chunk(h, 1 + l, st));
    CK(wait_params(h, o.ln1, o.ln1 + h->layer_stride, st));
  }
  TK(F_NORM_FWD, st, norm_fwd(h, h->hs[l], o.ln1, o.ln1_b, a.x1, a.mu1, a.rstd1, M, st));
  if (h->arch == 3) {  // Qwen3: no bias; per-head RMSNorm + RoPE in one pass behind the projection (never the fused epilogue)
    const int slot = fam_begin(h, F_QKV_FWD, st);
    CK(gemm_nt(a.x1, P + o.wqkv, a.qkv, nullptr, nullptr, M, h->QKV, H, st));
    CK(qknorm_rope_fwd(a.qkv, h->QKV, M, nH, nKV, d.head_dim, P + o.q_norm, P + o.k_norm, h->cosb, h->sinb, h->cosq, h->sinq,
                       d.rms_eps, a.qk_raw, a.qk_rstd, st));
    fam_end(h, slot, st);
  } else if (d.head_dim == 64 && (H % 64 == 0) && (h->QKV % 128 == 0)) {  // bias + RoPE fused into the projection epilogue
    TK(F_QKV_FWD, st, gemm_nt_rope(a.x1, P + o.wqkv, a.qkv, P + o.bqkv, h->cosb, h->sinb, h->cosq, h->sinq, nH, nH + nKV, M, h->QKV, H, st));
  } else {
    const int slot = fam_begin(h, F_QKV_FWD, st);
    CK(gemm_nt(a.x1, P + o.wqkv, a.qkv, P + o.bqkv, nullptr, M, h->QKV, H, st));
    CK(rope_apply(a.qkv, h->QKV, M, nH + nKV, d.head_dim, h->cosb, h->sinb, 0, st, nH, qscale));
    fam_end(h, slot, st);
  }
  TK(F_ATTN_FWD, st, attn_fwd(a.qkv, a.o, a.lse, h->cur_seg_s, h->attn_plan_buf, h->attn_tune, M, nH, nKV, d.head_dim, st));
  if (opt) {  // out_proj bias + residual, LayerNorm, fc1 bias + ReLU, fc2 bias + residual
    // residual dropout (armed forward): the two projections write bias only, the mask and the residual follow in one pass
    // (site 0 behind out_proj, 1 behind fc2). A re-run draws the forward's own mask again from the call that forward remembered.
    const bool drop = h->fwd_drop;
    DropSite ds = h->fwd_site;
    ds.site = 2u * (uint32_t)l;
    {
      const int slot = fam_begin(h, F_O_FWD, st);
      CK(gemm_nt(a.o, P + o.wo, a.hmid, P + o.bo, drop ? nullptr : h->hs[l], M, H, nH * d.head_dim, st));
      if (drop) CK(dropout_add(a.hmid, h->hs[l], M, H, ds, st));
      fam_end(h, slot, st);
    }
    TK(F_NORM_FWD, st, norm_fwd(h, a.hmid, o.ln2, o.ln2_b, a.x2, a.mu2, a.rstd2, M, st));
    TK(F_GATEUP_FWD, st, gemm_nt_relu(a.x2, P + o.wgu, a.act, P + o.b1, M, I, H, st));
    if (!rerun) {
      ds.site += 1;
      const int slot = fam_begin(h, F_DOWN_FWD, st);
      CK(gemm_nt(a.act, P + o.wd, h->hs[l + 1], P + o.b2, drop ? nullptr : a.hmid, M, H, I, st));
      if (drop) CK(dropout_add(h->hs[l + 1], a.hmid, M, H, ds, st));
      fam_end(h, slot, st);
    }
    return SLAM_OK;
  }
  TK(F_O_FWD, st, gemm_nt(a.o, P + o.wo, a.hmid, nullptr, h->hs[l], M, H, nH * d.head_dim, st));
  TK(F_NORM_FWD, st, norm_fwd(h, a.hmid, o.ln2, o.ln2_b, a.x2, a.mu2, a.rstd2, M, st));
  const bool timed = !rerun && h->time_gateup && h->tg_ev.size() == (size_t)(2 * L);
  if (timed) CK((int)hipEventRecord(h->tg_ev[2 * l], st));
  {
    const int slot = fam_begin(h, F_GATEUP_FWD, st);
    if (h->fuse_swiglu) {
      CK(gemm_nt_swiglu(a.x2, P + o.wgu, a.gu, a.act, M, 2 * I, H, st));
    } else {
      CK(gemm_nt(a.x2, P + o.wgu, a.gu, nullptr, nullptr, M, 2 * I, H, st));
      CK(swiglu_fwd(a.gu, a.act, M, I, GU_BLK, st));
    }
    fam_end(h, slot, st);
  }
  if (timed) CK((int)hipEventRecord(h->tg_ev[2 * l + 1], st));
  if (!rerun) TK(F_DOWN_FWD, st, gemm_nt(a.act, P + o.wd, h->hs[l + 1], nullptr, a.hmid, M, H, I, st));
  return SLAM_OK;
}

// "recompute" = 1: layer l's x1, x2 and (Qwen2) act, rebuilt in backward into the layer's shared slot from what the layer
// kept - hs[l], hmid and gu - by the kernels that made them in the forward, so the bits are the forward's. With the SwiGLU
// fused into the gate|up projection (fuse_swiglu) act came from the projection's fp32 accumulators, which the stored bf16
// gate|up no longer holds: that launch is re-run whole and rewrites gu with the values it has. The row statistics are
// rewritten with their own values too. OPT keeps act (its fc1 pre-activation is never stored): x1 and x2 only.
int rebuild_selective(SlamEngine* h, int l, int M, hipStream_t st) {
  const int H = h->d.hidden, I = h->d.intermediate;
  const bf16_t* P = h->params;
  const LayerOff& o = h->lo[l];
  LayerAct& a = h->la[l];
  TK(F_NORM_FWD, st, norm_fwd(h, h->hs[l], o.ln1, o.ln1_b, a.x1, a.mu1, a.rstd1, M, st));
  TK(F_NORM_FWD, st, norm_fwd(h, a.hmid, o.ln2, o.ln2_b, a.x2, a.mu2, a.rstd2, M, st));
  if (h->arch == 1) return SLAM_OK;
  if (h->fuse_swiglu) TK(F_GATEUP_FWD, st, gemm_nt_swiglu(a.x2, P + o.wgu, a.gu, a.act, M, 2 * I, H, st));
  else TK(F_GATEUP_FWD, st, swiglu_fwd(a.gu, a.act, M, I, GU_BLK, st));
  return SLAM_OK;
}

}  // namespace

namespace slam_impl {

// The decoder layer loop of a forward over M = B*T tokens: segments, attention plan, RoPE tables, embedding and every layer,
// leaving the last residual stream in hs[L] (slam_forward and slam_prefill continue from there). kv_lens (slam_prefill over
// kv_B rows, and only when the layers share their q|k|v buffer): each layer's K / V go to the cache before the next layer
// overwrites them.
int forward_layers(SlamEngine* h, const int64_t* ids, const int64_t* position_ids, const int32_t* seg_start,
                   const int32_t* seg_end, int M, int T, hipStream_t st, const int32_t* kv_lens, int kv_B) {
  const SlamModelDesc& d = h->d;
  const int H = d.hidden, L = d.n_layers;
  const bf16_t* P = h->params;
  if (seg_start) {
    h->cur_seg_s = seg_start;
    h->cur_seg_e = seg_end;
  } else {
    seg_fill_kernel<<<(M + 255) / 256, 256, 0, st>>>(h->seg_s, h->seg_e, M, T);
    h->cur_seg_s = h->seg_s;
    h->cur_seg_e = h->seg_e;
  }
  if (h->time_families) h->fam_marks.clear();  // the marks of a step = its last forward + backward
  CK(attn_plan(h->cur_seg_s, h->cur_seg_e, M, d.head_dim, h->attn_tune, h->attn_plan_buf, st));
  // queries are stored pre-scaled by head_dim^-0.5 * log2(e) (folded into their rotation tables: one rounding), so the
  // attention kernels' scores leave the matrix pipe in the exp2 domain
  const float qscale = 1.44269504088896340736f / sqrtf((float)d.head_dim);
  const bool opt = h->arch == 1;
  if (opt) {
    const size_t n = (size_t)M * (d.head_dim / 2);
    ident_rope_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(h->cosb, h->sinb, h->cosq, h->sinq, n, qscale);
    CK((int)hipGetLastError());
  } else {
    CK(rope_table(position_ids, M, T, d.head_dim, d.rope_theta, h->cosb, h->sinb, h->cosq, h->sinq, qscale, st));
  }
  CK(wait_chunk(h, 0, st));
  CK(wait_params(h, h->off_embed, h->lo[0].ln1, st));
  if (h->fwd_neft)
    CK(embed_noise_fwd(ids, position_ids, P + h->off_embed, opt ? P + h->off_pos : nullptr, h->hs[0], opt ? h->prow : nullptr, M, H,
                       d.vocab, T, h->npos, h->fwd_neft_site, st));
  else if (opt) CK(embed_pos_fwd(ids, position_ids, P + h->off_embed, P + h->off_pos, h->hs[0], h->prow, M, H, d.vocab, T, h->npos, st));
  else CK(embed_fwd(ids, P + h->off_embed, h->hs[0], M, H, d.vocab, st));
  for (int l = 0; l < L; ++l) {
    CK(layer_forward(h, l, M, false, st));
    if (kv_lens) CK(kv_scatter(h->la[l].qkv, kv_k(h, l), kv_v(h, l), kv_lens, kv_B, T, d.n_heads, d.n_kv_heads, d.head_dim, h->kv_cap, st));
  }
  CK(join_optimizer(h, st));
  CK(join_params(h, st));
  return SLAM_OK;
}

// the transposed weight images from the bound parameters (slam_refresh_transposed, and every entry point that rewrote them)
int refresh_transposed_images(SlamEngine* h, slam_stream_t stream) {
  if (!h->params_t) return SLAM_OK;
  if (!h->params) return h->fail(SLAM_ESTATE, "bind params first");
  hipStream_t st = (hipStream_t)stream;
  CK(join_optimizer(h, st));
  CK(join_params(h, st));
  h->params_t_dirty = false;
  // embedding and head, then every layer at once: the layers have the same shapes at a constant stride
  const auto tr = transpose_group(h, st);
  CK(for_each_param_group(h, 0, tr));
  CK(for_each_param_group(h, h->d.n_layers + 1, tr));
  CK(for_each_layer_tensor(h, 0, h->d.n_layers, tr));
  return SLAM_OK;
}

}  // namespace slam_impl

extern "C" {

const char* slam_version(void) { return "slam-engine gfx950 r6"; }

int slam_engine_create(const SlamModelDesc* desc, SlamEngine** out) { return slam_engine_create_arch(desc, 0, 0, out); }

int slam_engine_create_arch(const SlamModelDesc* desc, int32_t arch, int32_t n_positions, SlamEngine** out) {
  return slam_engine_create_ex(desc, arch, n_positions, 0, out);
}

int slam_engine_create_ex(const SlamModelDesc* desc, int32_t arch, int32_t n_positions, int32_t flags, SlamEngine** out) {
  if (!desc || !out) return SLAM_EINVAL;
  const SlamModelDesc& d = *desc;
  if (arch != 0 && arch != 1 && arch != 3) return SLAM_EINVAL;  // 2 is not a family
  if (flags & ~SLAM_MODEL_UNTIED_HEAD) return SLAM_EINVAL;
  const bool untied = (flags & SLAM_MODEL_UNTIED_HEAD) != 0;
  if (untied && arch == 1) return SLAM_EINVAL;
  if ((d.head_dim != 64 && d.head_dim != 128) || d.n_heads <= 0 || d.n_kv_heads <= 0 || d.n_heads % d.n_kv_heads) return SLAM_EINVAL;
  if (d.hidden % 8 || d.hidden > (arch == 1 ? 2048 : 4096) || d.vocab <= 0) return SLAM_EINVAL;  // the row-norm kernels' limits
  if (d.n_layers <= 0) return SLAM_EINVAL;
  if (arch != 1 && d.intermediate % GU_BLK) return SLAM_EINVAL;
  if (arch == 3 && (d.intermediate <= 0 || d.n_heads / d.n_kv_heads > 8)) return SLAM_EINVAL;  // the decode kernels' group limit
  // OPT: multi-head attention (kv = q heads), head_dim 64, a position table of n_positions + 2 rows
  if (arch == 1 && (d.n_kv_heads != d.n_heads || d.head_dim != 64 || d.intermediate <= 0 || d.intermediate % 8 || n_positions <= 0))
    return SLAM_EINVAL;
  SlamEngine* e = new SlamEngine();
  e->d = d;
  e->arch = arch;
  e->untied = untied;
  e->npos = arch == 1 ? n_positions + 2 : 0;
  e->QKV = (d.n_heads + 2 * d.n_kv_heads) * d.head_dim;
  e->vpad = d.vocab <= VPAD_SMALL ? VPAD_SMALL : ((d.vocab + 255) / 256) * 256;  // 256: the LM-head GEMM can take the 256 x 256 kernel
  e->fuse_swiglu = arch != 1 && (d.hidden % 64 == 0) && ((2 * d.intermediate) % 128 == 0);
  int64_t off = 0;
  e->off_embed = off;
  add_tensor(e, "embed", off, e->vpad, d.hidden);
  if (arch == 1) {
    e->off_pos = off;
    add_tensor(e, "pos_embed", off, e->npos, d.hidden);
  }
  e->lo.resize(d.n_layers);
  for (int l = 0; l < d.n_layers; ++l) {
    std::string p = "layers." + std::to_string(l) + ".";
    LayerOff& o = e->lo[l];
    const size_t t0 = e->tensors.size();
    if (arch == 1) {
      o.ln1 = off;   add_tensor(e, p + "ln1", off, d.hidden, 1);
      o.ln1_b = off; add_tensor(e, p + "ln1_b", off, d.hidden, 1);
      o.wqkv = off;  add_tensor(e, p + "wqkv", off, e->QKV, d.hidden);
      o.bqkv = off;  add_tensor(e, p + "bqkv", off, e->QKV, 1);
      o.wo = off;    add_tensor(e, p + "wo", off, d.hidden, d.n_heads * d.head_dim);
      o.bo = off;    add_tensor(e, p + "bo", off, d.hidden, 1);
      o.ln2 = off;   add_tensor(e, p + "ln2", off, d.hidden, 1);
      o.ln2_b = off; add_tensor(e, p + "ln2_b", off, d.hidden, 1);
      o.wgu = off;   add_tensor(e, p + "w1", off, d.intermediate, d.hidden);
      o.b1 = off;    add_tensor(e, p + "b1", off, d.intermediate, 1);
      o.wd = off;    add_tensor(e, p + "w2", off, d.hidden, d.intermediate);
      o.b2 = off;    add_tensor(e, p + "b2", off, d.hidden, 1);
    } else if (arch == 3) {
      o.ln1 = off;    add_tensor(e, p + "ln1", off, d.hidden, 1);
      o.wqkv = off;   add_tensor(e, p + "wqkv", off, e->QKV, d.hidden);
      o.bqkv = -1;
      o.q_norm = off; add_tensor(e, p + "q_norm", off, d.head_dim, 1);
      o.k_norm = off; add_tensor(e, p + "k_norm", off, d.head_dim, 1);
      o.wo = off;     add_tensor(e, p + "wo", off, d.hidden, d.n_heads * d.head_dim);
      o.ln2 = off;    add_tensor(e, p + "ln2", off, d.hidden, 1);
      o.wgu = off;    add_tensor(e, p + "wgu", off, 2 * d.intermediate, d.hidden);
      o.wd = off;     add_tensor(e, p + "wd", off, d.hidden, d.intermediate);
    } else {
      o.ln1 = off;  add_tensor(e, p + "ln1", off, d.hidden, 1);
      o.wqkv = off; add_tensor(e, p + "wqkv", off, e->QKV, d.hidden);
      o.bqkv = off; add_tensor(e, p + "bqkv", off, e->QKV, 1);
      o.wo = off;   add_tensor(e, p + "wo", off, d.hidden, d.n_heads * d.head_dim);
      o.ln2 = off;  add_tensor(e, p + "ln2", off, d.hidden, 1);
      o.wgu = off;  add_tensor(e, p + "wgu", off, 2 * d.intermediate, d.hidden);
      o.wd = off;   add_tensor(e, p + "wd", off, d.hidden, d.intermediate);
    }
    if (l == 0)
      for (size_t i = t0; i < e->tensors.size(); ++i) e->layer0.push_back((int)i);
  }
  e->layer_stride = d.n_layers > 1 ? e->lo[1].ln1 - e->lo[0].ln1 : (off - e->lo[0].ln1);
  e->off_norm = off;
  add_tensor(e, "norm", off, d.hidden, 1);
  if (arch == 1) {
    e->off_norm_b = off;
    add_tensor(e, "norm_b", off, d.hidden, 1);
  }
  e->off_head = e->off_embed;
  if (untied) {
    e->off_head = off;
    add_tensor(e, "lm_head", off, e->vpad, d.hidden);
  }
  e->n_params = off;
  *out = e;
  return SLAM_OK;
}

void slam_engine_destroy(SlamEngine* h) {
  if (h) (void)slam_comm_destroy(h);  // a communicator the caller did not release (needs RCCL's symbols: not the destructor's job)
  delete h;
}
const char* slam_last_error(SlamEngine* h) { return h ? h->err.c_str() : "null engine"; }
int64_t slam_param_count(SlamEngine* h) { return h ? h->n_params : 0; }
int32_t slam_tensor_count(SlamEngine* h) { return h ? (int32_t)h->tensors.size() : 0; }
int slam_tensor_info(SlamEngine* h, int32_t i, SlamTensorInfo* out) {
  if (!h || !out || i < 0 || i >= (int32_t)h->tensors.size()) return SLAM_EINVAL;
  *out = h->tensors[i];
  return SLAM_OK;
}
int slam_bind_params(SlamEngine* h, void* params_bf16, float* grads_f32) {
  if (!h || !params_bf16) return SLAM_EINVAL;
  h->params = (bf16_t*)params_bf16;
  h->grads = grads_f32;
  h->w8_valid = false;
  return SLAM_OK;
}
// the caller wrote the parameters: FP8 decode codes made from the earlier values are stale
int slam_refresh_transposed(SlamEngine* h, slam_stream_t stream) {
  if (!h) return SLAM_EINVAL;
  h->w8_valid = false;
  return refresh_transposed_images(h, stream);
}
int slam_bind_params_t(SlamEngine* h, void* params_t_bf16) {
  if (!h) return SLAM_EINVAL;
  const SlamModelDesc& d = h->d;
  if (params_t_bf16 && ((d.hidden & 63) || (d.intermediate & 63) || (h->QKV & 63) || ((d.n_heads * d.head_dim) & 63)))
    return h->fail(SLAM_EINVAL, "transposed weight images need dims that are multiples of 64");
  h->params_t = (bf16_t*)params_t_bf16;
  return SLAM_OK;
}
size_t slam_workspace_bytes(SlamEngine* h, int64_t max_tokens) {
  if (!h || max_tokens <= 0) return 0;
  GemmTuneScope tune_scope(&h->gemm_tune);
  SlamEngine tmp;
  tmp.d = h->d;
  tmp.arch = h->arch;
  tmp.npos = h->npos;
  tmp.QKV = h->QKV;
  tmp.vpad = h->vpad;
  tmp.untied = h->untied;
  tmp.n_params = h->n_params;
  tmp.recompute = h->recompute;
  tmp.dropout_thr16 = h->dropout_thr16;
  return carve(&tmp, nullptr, max_tokens);
}
int slam_bind_workspace(SlamEngine* h, void* ws, size_t bytes, int64_t max_tokens) {
  if (!h || !ws || max_tokens <= 0) return SLAM_EINVAL;
  if (((uintptr_t)ws) & 255) return h->fail(SLAM_EINVAL, "workspace must be 256-byte aligned");
  size_t need = slam_workspace_bytes(h, max_tokens);
  if (bytes < need) return h->fail(SLAM_ENOMEM, "workspace too small");
  carve(h, (char*)ws, max_tokens);
  h->ws = (char*)ws;
  h->ws_bytes = bytes;
  h->max_tokens = max_tokens;
  h->have_fwd = false;
  return SLAM_OK;
}
int slam_set_option(SlamEngine* h, const char* key, int64_t value) {
  if (!key) return SLAM_EINVAL;
  if (!strncmp(key, "gemm_", 5)) {  // kernel-selection knobs: this engine's (h) or the process default's (h = NULL)
    const int r = gemm_tune_set(h ? &h->gemm_tune : gemm_default_tune(), key, (long)value);
    if (r > 0) return SLAM_OK;
    return h ? h->fail(SLAM_EINVAL, std::string(r < 0 ? "value out of range for option " : "unknown option ") + key) : SLAM_EINVAL;
  }
  if (!strcmp(key, "attn_jq") || !strcmp(key, "attn_kw") || !strcmp(key, "attn_nch") || !strcmp(key, "attn_prio")) {
    // with an engine: that engine's launches (takes effect at its next forward, which rebuilds the attention plan);
    // without: the process default picked up by the single-op entry points and by engines created afterwards
    AttnTune t = h ? h->attn_tune : attn_default_tune();
    (key[5] == 'j' ? t.jq : key[5] == 'k' ? t.kw : key[5] == 'n' ? t.nch : t.prio) = (int)value;
    if (h) { h->attn_tune = t; h->have_fwd = false; } else attn_set_default_tune(t);
    return SLAM_OK;
  }
  if (!strcmp(key, "overlap_adamw") && h) { h->overlap_adamw = value != 0; return SLAM_OK; }
  if (!strcmp(key, "adamw_sr") && h) {
    if (value < 0 || value > 1) return h->fail(SLAM_EINVAL, "value out of range for option adamw_sr (0 or 1)");
    h->adamw_sr = (int)value;
    return SLAM_OK;
  }
  if (!strcmp(key, "adamw_sr_seed") && h) { h->adamw_sr_seed = (uint64_t)value; return SLAM_OK; }
  if (!strcmp(key, "bwd_wgrad_stream") && h) { h->wgrad_stream = value != 0; return SLAM_OK; }
  if (!strcmp(key, "bwd_aux_side") && h) { h->aux_side = value != 0; return SLAM_OK; }
  if (!strcmp(key, "bwd_wgrad_cus") && h) { h->wside_cus = (int)value; return SLAM_OK; }
  if (!strcmp(key, "time_param_waits") && h) { h->time_param_waits = value != 0; return SLAM_OK; }
  if (!strcmp(key, "time_gateup") && h) {
    if (value && h->tg_ev.empty()) {
      h->tg_ev.resize((size_t)2 * h->d.n_layers);
      for (auto& e : h->tg_ev)
        if (hipEventCreate(&e) != hipSuccess) { h->tg_ev.clear(); return h->fail(SLAM_ESTATE, "hipEventCreate failed"); }
    }
    h->time_gateup = value != 0;
    return SLAM_OK;
  }
  if (!strcmp(key, "time_families") && h) { h->time_families = value != 0; if (!value) h->fam_marks.clear(); return SLAM_OK; }
  if (!strcmp(key, "grad_overwrite_next") && h) { h->overwrite_next = value != 0; return SLAM_OK; }
  if (!strcmp(key, "grad_norm_partials") && h) { h->norm_partials = value != 0; return SLAM_OK; }
  if (!strcmp(key, "grad_final_next") && h) {
    if (value < 0 || value > 2) return h->fail(SLAM_EINVAL, "grad_final_next takes 0, 1 or 2");
    h->final_next = (int)value;
    return SLAM_OK;
  }
  if (!strcmp(key, "recompute") && h) {
    if (value < 0 || value > 2) return h->fail(SLAM_EINVAL, "value out of range for option recompute (0, 1 or 2)");
    if ((int)value != h->recompute) {  // the workspace layout depends on the level: the bound one no longer fits
      h->recompute = (int)value;
      h->ws = nullptr;
      h->ws_bytes = 0;
      h->max_tokens = 0;
      h->have_fwd = h->have_loss = false;
      h->kv_ready = false;
    }
    return SLAM_OK;
  }
  if (!strcmp(key, "dropout_thr16") && h) {
    if (value < 0 || value > 65535) return h->fail(SLAM_EINVAL, "value out of range for option dropout_thr16 (0 .. 65535)");
    if (value != 0 && h->arch != 1) return h->fail(SLAM_EINVAL, "dropout_thr16: residual dropout exists for the OPT family only");
    if ((value != 0) != (h->dropout_thr16 != 0)) {  // the masked-gradient buffers come or go: the bound workspace no longer fits
      h->ws = nullptr;
      h->ws_bytes = 0;
      h->max_tokens = 0;
      h->have_fwd = h->have_loss = false;
      h->kv_ready = false;
    }
    h->dropout_thr16 = (int)value;
    if (!value) h->dropout_call_next = -1;
    return SLAM_OK;
  }
  if (!strcmp(key, "dropout_seed") && h) { h->dropout_seed = (uint64_t)value; return SLAM_OK; }
  if (!strcmp(key, "dropout_call_next") && h) {
    if (value < 0 || value > 0xffffffffLL) return h->fail(SLAM_EINVAL, "value out of range for option dropout_call_next (0 .. 2^32 - 1)");
    if (h->dropout_thr16) h->dropout_call_next = value;  // ignored while dropout is off
    return SLAM_OK;
  }
  if (!strcmp(key, "neftune_call_next") && h) {
    if (value < 0 || value > 0xffffffffLL) return h->fail(SLAM_EINVAL, "value out of range for option neftune_call_next (0 .. 2^32 - 1)");
    if (h->neftune_alpha > 0.f) h->neftune_call_next = value;  // ignored while NEFTune is off
    return SLAM_OK;
  }
  if (!strcmp(key, "fuse_swiglu") && h) { h->fuse_swiglu = value != 0; return SLAM_OK; }
  if (!strcmp(key, "fuse_dswiglu") && h) { h->fuse_dswiglu = value != 0; return SLAM_OK; }
  if (!strcmp(key, "fuse_adamw_t") && h) { h->fuse_adamw_t = value != 0; return SLAM_OK; }
  return h ? h->fail(SLAM_EINVAL, std::string("unknown option ") + key) : SLAM_EINVAL;
}

}  // extern "C"

// slam_forward, and the tail of slam_forward_unpadded_spans: `up` = the packed arrays of a padding-free call over up_B x up_T
// (ids .. seg_end then point into them and (B, T) = (1, M_packed)); its logits go back to the batch's own layout, row b's from
// column up_starts[b] on (nullable: 0; the caller's array, read in this call only).
static int forward_common(SlamEngine* h, const int64_t* ids, const int64_t* labels, const int64_t* position_ids,
                          const int32_t* seg_start, const int32_t* seg_end, int32_t B, int32_t T, double num_items,
                          float* loss_out, void* logits_out, const UnpadView* up, const int32_t* up_starts, int up_B, int up_T,
                          slam_stream_t stream) {
  // "dropout_call_next" arms this call and no other: a refused forward uses it up too, so no later one inherits it
  const int64_t armed_call = h->dropout_call_next, neft_call = h->neftune_call_next;
  h->dropout_call_next = -1;
  h->neftune_call_next = -1;
  h->fwd_neft = false;
  if (!ids || B <= 0 || T <= 0) return SLAM_EINVAL;
  if (!h->params || !h->ws) return h->fail(SLAM_ESTATE, "bind params and workspace first");
  const int64_t M64 = (int64_t)B * T;
  if (M64 > h->max_tokens) return h->fail(SLAM_ENOMEM, "B*T exceeds bound workspace tokens");
  if ((seg_start == nullptr) != (seg_end == nullptr)) return h->fail(SLAM_EINVAL, "seg_start/seg_end both or none");
  if (labels && !loss_out) return h->fail(SLAM_EINVAL, "labels given without loss_out");
  if (labels && h->label_smoothing > 0.f && h->logit_mask)
    return h->fail(SLAM_ESTATE, "label smoothing with a logit mask set: masked scoring is a likelihood, not a training loss");
  const int M = (int)M64;
  const SlamModelDesc& d = h->d;
  hipStream_t st = (hipStream_t)stream;
  const int H = d.hidden, L = d.n_layers;
  const bf16_t* P = h->params;
  h->have_fwd = false;
  // "dropout_call_next" armed this forward and no other: whatever happens below, the next one starts unarmed
  h->fwd_drop = h->arch == 1 && h->dropout_thr16 > 0 && armed_call >= 0;
  if (h->fwd_drop) {
    h->fwd_site = DropSite();
    h->fwd_site.thr16 = h->dropout_thr16;
    h->fwd_site.seed = h->dropout_seed;
    h->fwd_site.call = (uint32_t)armed_call;
  }
  // "neftune_call_next", the same way: s from the batch as the caller passed it (a padding-free call's padded width), the
  // element index from the layout that is launched
  if (h->neftune_alpha > 0.f && neft_call >= 0) {
    h->fwd_neft = true;
    h->fwd_neft_site = NeftSite();
    h->fwd_neft_site.s = (float)((double)h->neftune_alpha / sqrt((double)(up ? up_T : T) * (double)H) / 65536.0);
    h->fwd_neft_site.seed = h->neftune_seed;
    h->fwd_neft_site.call = (uint32_t)neft_call;
  }
  GemmTuneScope tune_scope(&h->gemm_tune);
  const int fl = forward_layers(h, ids, position_ids, seg_start, seg_end, M, T, st);
  h->fwd_neft = false;  // this forward's launch and no other
  CK(fl);
  TK(F_NORM_FWD, st, norm_fwd(h, h->hs[L], h->off_norm, h->off_norm_b, h->hf, h->muf, h->rstdf, M, st));
  const int VP = h->vpad;
  TK(F_HEAD_FWD, st, gemm_nt(h->hf, P + h->off_head, h->logits, nullptr, nullptr, M, VP, H, st));
  h->have_loss = false;
  if (logits_out && up) CK(unpad_logits(h->logits, VP, (bf16_t*)logits_out, d.vocab, up->off, up_starts, up_B, up_T, M, st));
  else if (logits_out) CK(copy_cols(h->logits, VP, (bf16_t*)logits_out, d.vocab, M, d.vocab, st));
  if (labels) {
    TK(F_LOSS, st, cross_entropy(h->logits, labels, num_items, h->dlogits, h->row_loss, h->scal + 0, h->scal + 1, B, T, VP,
                     d.vocab, h->logit_mask, h->label_smoothing, h->dsum, st));
    CK((int)hipMemcpyAsync(loss_out, h->scal + 1, sizeof(float), hipMemcpyDeviceToDevice, st));
    h->have_loss = true;
    h->loss_smoothed = h->label_smoothing > 0.f;
  }
  h->B = B;
  h->T = T;
  h->last_ids = ids;
  h->unpadded = up != nullptr;
  if (up) { h->up = *up; h->up_B = up_B; h->up_T = up_T; h->up_has_labels = labels != nullptr; }
  h->last_tokens = M;
  h->have_fwd = true;
  return SLAM_OK;
}

extern "C" {

int slam_forward(SlamEngine* h, const int64_t* ids, const int64_t* labels, const int64_t* position_ids,
                 const int32_t* seg_start, const int32_t* seg_end, int32_t B, int32_t T, double num_items,
                 float* loss_out, void* logits_out, slam_stream_t stream) {
  if (!h) return SLAM_EINVAL;
  return forward_common(h, ids, labels, position_ids, seg_start, seg_end, B, T, num_items, loss_out, logits_out, nullptr, nullptr, 0,
                        0, stream);
}

size_t slam_unpadded_scratch_bytes(int32_t B, int32_t T) {
  if (B <= 0 || T <= 0 || (int64_t)B * T > 0x7fffffc0LL) return 0;
  return unpad_scratch_bytes(B, T);
}

int slam_forward_unpadded(SlamEngine* h, const int64_t* ids, const int64_t* labels, const int32_t* lens, int32_t B, int32_t T,
                          int32_t M_packed, void* scratch, size_t scratch_bytes, double num_items, float* loss_out,
                          void* logits_out, slam_stream_t stream) {
  return slam_forward_unpadded_spans(h, ids, labels, nullptr, lens, B, T, M_packed, scratch, scratch_bytes, num_items, loss_out,
                                     logits_out, stream);
}

int slam_forward_unpadded_spans(SlamEngine* h, const int64_t* ids, const int64_t* labels, const int32_t* starts,
                                const int32_t* lens, int32_t B, int32_t T, int32_t M_packed, void* scratch, size_t scratch_bytes,
                                double num_items, float* loss_out, void* logits_out, slam_stream_t stream) {
  if (!h) return SLAM_EINVAL;
  const int64_t armed_call = h->dropout_call_next, neft_call = h->neftune_call_next;  // a refused call uses the arming up, as slam_forward does
  auto refuse = [&](int code, const char* m) { h->dropout_call_next = h->neftune_call_next = -1; return h->fail(code, m); };
  if (!ids || !lens || !scratch || B <= 0 || T <= 0 || (int64_t)B * T > 0x7fffffc0LL) return refuse(SLAM_EINVAL, "forward_unpadded: bad argument");
  const int64_t mmax = (((int64_t)B * T + 63) / 64) * 64;
  if (M_packed <= 0 || (M_packed & 63) || M_packed > mmax) return refuse(SLAM_EINVAL, "M_packed must be a multiple of 64 in (0, B*T rounded up to 64]");
  if (((uintptr_t)scratch & 255) || scratch_bytes < unpad_scratch_bytes(B, T)) return refuse(SLAM_EINVAL, "scratch: 256-byte aligned, slam_unpadded_scratch_bytes(B, T) bytes");
  if (!h->params || !h->ws) return refuse(SLAM_ESTATE, "bind params and workspace first");
  if (M_packed > h->max_tokens) return refuse(SLAM_ENOMEM, "M_packed exceeds bound workspace tokens");
  if (labels && !loss_out) return refuse(SLAM_EINVAL, "labels given without loss_out");
  h->have_fwd = false;
  const UnpadView v = unpad_view(scratch, B, T);
  int rc = unpad_pack(ids, labels, starts, lens, B, T, M_packed, h->d.pad_token_id, v, (hipStream_t)stream);
  if (rc != 0) { h->dropout_call_next = h->neftune_call_next = -1; return rc; }
  h->dropout_call_next = armed_call;
  h->neftune_call_next = neft_call;
  return forward_common(h, v.ids, labels ? v.labels : nullptr, v.pos, v.seg_s, v.seg_e, 1, M_packed, num_items, loss_out, logits_out,
                        &v, starts, B, T, stream);
}

int64_t slam_last_forward_tokens(SlamEngine* h) { return h && h->have_fwd ? h->last_tokens : 0; }

}  // extern "C"

namespace {
// One slam_backward call: what its steps share, and the steps. slam_backward fills it (begin), then runs head(), layer(l) from
// the top layer down with finish_slabs() at the bucket boundaries, embedding() and the join. The decoder layer is written
// once: the families differ in which projections carry a bias, in the norm and the activation (DESIGN.md §5 has the table).
// Weight-gradient launches go to the main stream, or (bwd_wgrad_stream) to the side stream `ws` behind an event that the
// main stream records once their operands exist. Every cross-stream edge costs the recording AND the waiting stream a
// barrier packet (~6 us of queue bubble each, measured in the kernel trace), so the schedule keeps them few:
//  * no side -> main edges at all: every gradient a weight-gradient GEMM reads lives in a buffer nothing overwrites
//    until the next forward - the gradient of hs[l] goes into layer l's (dead) hmid buffer, the gradient of hmid[l]
//    into the (dead) hs[l+1] buffer, d(qkv) of layer l into layer l+1's (dead) qkv buffer; all three are buffers only
//    main-stream kernels read, and only earlier in this backward;
//  * main -> side: one event per weight-gradient GEMM, recorded as soon as its operands exist. Handing them over in
//    batches (two or one event per layer) was measured and is worse (+0.8 / +1.5 ms per Slam-358M step): the side stream
//    needs its work as early as it can have it.
struct Backward {
  SlamEngine* const h;
  const hipStream_t st;  // the caller's stream: the dgrad / attention / norm chain
  const SlamModelDesc& d = h->d;
  const int M = h->B * h->T, H = d.hidden, I = d.intermediate, L = d.n_layers;
  const bf16_t *const P = h->params, *const Pt = h->params_t;  // Pt: the transposed weight images (nullable)
  float* const G = h->grads;
  const bool opt = h->arch == 1, q3 = h->arch == 3;
  const bool two = h->wgrad_stream != 0, aux = two && h->aux_side != 0;  // bwd_wgrad_stream, bwd_aux_side
  const int rc = h->recompute;
  const bool slot_edges = rc && two && L > RC_SLOTS, drop = opt && h->fwd_drop;
  const int qnb = q3 ? qn_blocks(h, M) : 0;  // Qwen3: blocks of the q / k norm backward
  hipStream_t ws = st;     // the weight gradients' stream: h->wside with bwd_wgrad_stream (begin)
  int acc = 1, fin = 0;    // 0: this backward stores gradients, 1: it adds to them; "grad_final_next" of this call
  bf16_t* IMG = nullptr;   // bf16 image of the gradients (nullable)
  bool partials = false;   // the final-value stores emit sum-of-squares partials
  GradSink sink_store{};   // of the launch in flight: sink() fills it, take() reads what the launch used
  int ev_used = 0;         // events of ev_w handed out by edge()
  bf16_t* dh = nullptr;    // the gradient on its way down: wrt hs[l + 1] when layer(l) starts, wrt hs[l] when it returns

  int make_events(std::vector<hipEvent_t>& ev) {  // one per layer, created by the first call that needs them
    if (!ev.empty()) return SLAM_OK;
    ev.resize((size_t)L);
    for (auto& e : ev)
      if (hipEventCreateWithFlags(&e, sync_event_flags()) != hipSuccess) { ev.clear(); return h->fail(SLAM_ESTATE, "hipEventCreate failed"); }
    return SLAM_OK;
  }
  // consumes what armed this call (grad_overwrite_next, the gradient image, grad_final_next) and readies streams and events
  int begin(float grad_scale, bool have_cb) {
    if (grad_scale != 1.0f) CK(scale_bf16(h->dlogits, (size_t)M * h->vpad, grad_scale, st));
    // first micro-batch of an optimizer step: every gradient tensor is written exactly once below (the tied embedding
    // twice: head first, gather side second; untied, lm_head once by the head and the embedding once by the gather side,
    // which then stores - or zeroes the tensor before its scatter), so it may be STORED instead of accumulated and the buffer needs no
    // zeroing pass (4 B/param written by AdamW + 4 B/param re-read by the wgrad epilogues)
    acc = h->overwrite_next ? 0 : 1;
    h->overwrite_next = false;
    // bf16 communication image of the gradients (slam_set_grad_image): written by the SAME kernels that store the final fp32
    // values (unsplit weight-gradient tiles, slab reduces, the norm / bias finish kernel) - no conversion pass over the buffer
    h->last_grad_img = IMG = h->grad_img;
    h->grad_img = nullptr;
    // last backward of an optimizer step ("grad_final_next"): sum-of-squares partials from the final-value stores, and
    // (mode 2) final values in the bf16 image only. Every launch that stores final values takes its slots in launch order.
    fin = h->final_next;
    h->final_next = 0;
    h->gfinal = 0;
    h->g16 = nullptr;
    if (fin == 2 && !IMG) return h->fail(SLAM_ESTATE, "grad_final_next = 2 needs slam_set_grad_image before the backward");
    // known from here on: the bucket callbacks run INSIDE this call, and the engine-side exchange they may start
    // (slam_allreduce_grads_async / slam_reduce_scatter_grads_async) asks where the gradients live
    h->gfinal = fin;
    h->g16 = fin == 2 ? IMG : nullptr;
    partials = fin && !have_cb && h->norm_partials;  // with a bucket callback the gradients are about to be exchanged: partials of the local ones are of no use
    h->gn_valid = false;
    if (partials) {
      CK((int)hipMemsetAsync(h->gn_part, 0, h->gn_cap * sizeof(float), st));  // blocks without a final store leave their slot alone
      h->gn_used = 0;
    }
    if (two) CK(ensure_wside(h));
    ws = two ? h->wside : st;
    // "recompute": layer l's slot (l mod 3) last held layer l + 3. On the caller's stream everything of that layer is behind us;
    // on the weight-gradient stream its last reader is layer l + 2's Wqkv gradient and bias column sums, whose d(qkv) lives in
    // la[l + 3].qkv. Layer l + 1's weight gradients touch the slots of layers l + 1 and l + 2 only. So one side -> main edge per
    // layer (ev_rc), a whole layer old by the time it is waited for ("Activation recomputation", has the table).
    if (int r = slot_edges ? make_events(h->ev_rc) : 0) return r;
    // residual dropout: this backward belongs to a forward that dropped. The masked copies live in two buffer pairs by layer
    // parity; on the weight-gradient stream layer l's last reader is its Wo gradient, which layer l - 2 waits for (ev_dm[l])
    if (drop && !h->dmask[0][0]) return h->fail(SLAM_ESTATE, "dropout: the bound workspace has no masked-gradient buffers");
    if (int r = drop && two ? make_events(h->ev_dm) : 0) return r;
    return SLAM_OK;
  }
  int edge(hipStream_t from, hipStream_t to) {  // `to` continues after everything enqueued on `from` so far
    if (from == to) return 0;
    if ((size_t)ev_used >= h->ev_w.size()) return SLAM_ESTATE;
    hipEvent_t e = h->ev_w[ev_used++];
    if (hipError_t r = hipEventRecord(e, from)) return (int)r;
    return (int)hipStreamWaitEvent(to, e, 0);
  }
  int fork() { return two ? edge(st, ws) : 0; }
  bf16_t* img(int64_t off) const { return IMG ? IMG + off : nullptr; }
  GradSink* sink() {  // the slots from gn_used on; take(r) after the launch
    if (!fin) return nullptr;
    sink_store.img_only = fin == 2;
    sink_store.sumsq = partials ? h->gn_part + h->gn_used : nullptr;
    sink_store.cap = (int)(h->gn_cap - h->gn_used);
    sink_store.used = 0;
    return &sink_store;
  }
  int take(int r) {
    if (partials && r == 0) h->gn_used += (size_t)sink_store.used;
    return r;
  }
  // dX[M,K] = dY[M,N] W[N,K]: with a transposed image W^T[K,N] it is the contraction-contiguous form
  int dgrad(const bf16_t* dY, int64_t woff, bf16_t* dX, int N, int K) {
    return Pt ? gemm_nt(dY, Pt + woff, dX, nullptr, nullptr, M, K, N, st) : gemm_nn(dY, P + woff, dX, nullptr, M, N, K, st);
  }
  // dW (+)= a^T b on the weight-gradient stream. handed_over: ws already waits for everything enqueued on st so far
  // is_final: the launch stores the tensor's final values (everything but the head's half of the tied embedding gradient)
  int wgrad(int fam, const bf16_t* a, const bf16_t* b, float* g, int n, int k, bf16_t* gi, bool is_final = true, bool handed_over = false) {
    if (!handed_over) CK(fork());
    const int slot = fam_begin(h, fam, ws);
    const int r = take(gemm_tn(a, b, g, acc, M, n, k, n, k, h->gemm_ws, h->gemm_ws_bytes, ws, two ? 1 : 0, gi, is_final ? sink() : nullptr));
    fam_end(h, slot, ws);
    return r;
  }
  // A projection's gradients from dY [M][n] and its input X [M][k]. The bias column sums go to the layer's slab `bias_part`
  // (null: the projection has no bias): on the weight-gradient stream behind a hand-over (aux), which then serves the
  // weight gradient too - both read dY - else on the main stream. Then the weight gradient.
  int proj_wgrad(int fam, const bf16_t* dY, const bf16_t* X, int64_t woff, int n, int k, float* bias_part) {
    const bool side_cols = bias_part && aux;
    if (side_cols) CK(fork());
    if (bias_part) CK(colsum_bf16(dY, n, M, n, nullptr, 1, bias_part, side_cols ? ws : st));
    return wgrad(fam, dY, X, G + woff, n, k, img(woff), true, side_cols);
  }
  // one launch that finishes `cnt` same-shaped tensors (the first at `off`) from their partial slabs, on `s`
  int finish(const float* part, size_t part_stride, int nb, int N, int64_t off, size_t out_stride, int cnt, hipStream_t s) {
    return take(colsum_finish_many(part, part_stride, nb, N, G + off, out_stride, cnt, acc, s, img(off), sink()));
  }
  // The family's norm backward: dx = d(norm)(dy) + dres, and per-block partials of the weight (LayerNorm: and bias) gradient.
  // slab >= 0: a layer's norm - the partials go to that slab of ln_part (lnb_part) and finish_slabs reduces them. slab < 0:
  // the final norm - partials in part_ws; the RMSNorm kernel finishes its weight gradient itself, head() LayerNorm's two.
  int norm_bwd(const bf16_t* dy, const bf16_t* x, int64_t woff, const float* mu, const float* rstd, const bf16_t* dres, bf16_t* dx, int slab) {
    const bool last = slab < 0;
    float* pw = last ? h->part_ws : h->ln_part + (size_t)slab * h->ln_ps;
    const int slot = fam_begin(h, F_NORM_BWD, st);
    if (opt) {
      float* pb = last ? h->part_ws + (size_t)rmsnorm_bwd_blocks(M) * H : h->lnb_part + (size_t)slab * h->ln_ps;
      CK(layernorm_bwd(dy, x, P + woff, mu, rstd, dres, dx, pw, pb, M, H, st));
    } else {
      const int r = rmsnorm_bwd(dy, x, P + woff, rstd, dres, dx, last ? G + woff : nullptr, last ? acc : 1, pw, M, H, st,
                                last ? img(woff) : nullptr, last ? sink() : nullptr);
      CK(last ? take(r) : r);
    }
    fam_end(h, slot, st);
    return SLAM_OK;
  }
  int rebuild(int l) {
    if (slot_edges && l + RC_SLOTS - 1 < L) CK((int)hipStreamWaitEvent(st, h->ev_rc[(size_t)l + RC_SLOTS - 1], 0));
    h->gemm_tune.shared = 0;  // the forward's launches plan for a GPU of their own: so do their re-runs
    const int r = rc == 2 ? layer_forward(h, l, M, true, st) : rebuild_selective(h, l, M, st);
    h->gemm_tune.shared = two ? 1 : 0;
    return r;
  }
  // the weight-gradient stream has everything of layer l that reads a shared slot
  int slot_done(int l) { return slot_edges && l >= RC_SLOTS - 1 ? (int)hipEventRecord(h->ev_rc[(size_t)l], ws) : 0; }
  // residual dropout: dy becomes its masked, rescaled copy - what flows into the projection in front of `site`
  int masked(const bf16_t*& dy, int l, int site) {
    DropSite ds = h->fwd_site;
    ds.site = 2u * (uint32_t)l + (uint32_t)site;
    bf16_t* dm = h->dmask[l & 1][site];
    const int r = dropout_bwd(dy, dm, M, H, ds, st);
    dy = dm;
    return r;
  }
  // LM head and final norm: dlogits -> dh, the gradient wrt hs[L]
  int head() {
    // tied head: dE += dlogits^T hf ; dhf = dlogits E - not final, the gather side adds to the tensor in embedding().
    // Untied head: d lm_head = dlogits^T hf ; dhf = dlogits lm_head - the head's own tensor (off_head), final
    CK(wgrad(F_HEAD_WGRAD, h->dlogits, h->hf, G + h->off_head, h->vpad, H, h->untied ? img(h->off_head) : nullptr, h->untied));
    TK(F_HEAD_DGRAD, st, dgrad(h->dlogits, h->off_head, h->dx, h->vpad, H));
    dh = h->dh_a;
    CK(norm_bwd(h->dx, h->hs[L], h->off_norm, h->muf, h->rstdf, nullptr, dh, -1));
    if (opt) {  // final LayerNorm: dw | db slabs in part_ws, one finish launch per tensor
      const int nbl = rmsnorm_bwd_blocks(M);
      CK(finish(h->part_ws, 0, nbl, H, h->off_norm, 0, 1, st));
      CK(finish(h->part_ws + (size_t)nbl * H, 0, nbl, H, h->off_norm_b, 0, 1, st));
    }
    return SLAM_OK;
  }
  // One decoder layer, for every family: dh (wrt hs[l + 1]) -> dh (wrt hs[l]), the layer's weight gradients and its partial slabs
  int layer(int l) {
    const int nH = d.n_heads, nKV = d.n_kv_heads, HD = nH * d.head_dim, GU = opt ? I : 2 * I;  // GU: columns of gate|up / fc1
    const LayerOff& o = h->lo[l];
    LayerAct& a = h->la[l];
    bf16_t* dh2 = h->hs[l + 1];                              // grad wrt hmid[l]: hs[l+1] was last read by the norm backward above it
    bf16_t* dqkv = l + 1 < L ? h->la[l + 1].qkv : h->dqkv;   // layer l+1's q|k|v were last read by its attention backward
    if (rc) CK(rebuild(l));  // before the first reader below, and before the activation backward overwrites gu
    // MLP: down / fc2 (OPT: bias), activation, gate|up / fc1 (OPT: bias). d(gate|up) [M][2I] (OPT: d(fc1) [M][I]) goes to this layer's own gu
    // buffer, which nothing overwrites before the next forward (its weight gradient and OPT's b1 column sums read it on the side stream)
    // residual dropout: what flows into fc2 / out_proj is the masked, rescaled copy of the residual gradient; the norm
    // backward below keeps reading the unmasked dh / dh2 as the residual branch's share
    const bf16_t *dhm = dh, *dh2m = dh2;
    if (drop && two && l + 2 < L) CK((int)hipStreamWaitEvent(st, h->ev_dm[(size_t)l + 2], 0));  // a whole layer old by now
    if (drop) CK(masked(dhm, l, 1));
    CK(proj_wgrad(F_WD_WGRAD, dhm, a.act, o.wd, H, I, opt ? h->b2_part + (size_t)l * h->hb_ps : nullptr));
    const int slot = fam_begin(h, F_DOWN_DGRAD, st);
    if (opt && Pt) CK(gemm_nt_drelu(dhm, Pt + o.wd, a.gu, a.act, M, I, H, st));  // the ReLU backward in the dgrad epilogue
    else if (opt) {
      CK(dgrad(dhm, o.wd, a.gu, H, I));
      CK(relu_bwd(a.gu, a.act, (size_t)M * I, st));
    } else if (Pt && h->fuse_dswiglu && (I % 128 == 0) && (H % 64 == 0)) {
      CK(gemm_nt_dswiglu(dhm, Pt + o.wd, a.gu, M, I, H, st));  // d(act) stays in registers; a.gu -> d(gate|up)
    } else {
      CK(dgrad(dhm, o.wd, h->dact, H, I));
      CK(swiglu_bwd(a.gu, h->dact, M, I, GU_BLK, st));  // a.gu now holds d(gate|up)
    }
    fam_end(h, slot, st);
    CK(proj_wgrad(F_WGU_WGRAD, a.gu, a.x2, o.wgu, GU, H, opt ? h->b1_part + (size_t)l * h->ib_ps : nullptr));
    TK(F_GATEUP_DGRAD, st, dgrad(a.gu, o.wgu, h->dx, GU, H));
    CK(norm_bwd(h->dx, a.hmid, o.ln2, a.mu2, a.rstd2, dh, dh2, 2 * l + 1));
    // attention: out projection (OPT: bias; both: residual), then one attention backward (OPT: identity rotation tables)
    if (drop) CK(masked(dh2m, l, 0));
    CK(proj_wgrad(F_WO_WGRAD, dh2m, a.o, o.wo, H, HD, opt ? h->bo_part + (size_t)l * h->hb_ps : nullptr));
    if (drop && two) CK((int)hipEventRecord(h->ev_dm[(size_t)l], ws));  // the last reader of this layer's masked copies on ws
    TK(F_O_DGRAD, st, dgrad(dh2m, o.wo, h->d_o, H, HD));
    TK(F_ATTN_BWD, st, attn_bwd(a.qkv, a.o, h->d_o, a.lse, h->dsum, h->nlse, dqkv, h->dkv_part, h->cur_seg_s, h->cur_seg_e, h->attn_plan_buf, h->attn_tune, h->cosb, h->sinb,
                M, nH, nKV, d.head_dim, st));  // dq / dk come out already rotated back
    float* qkv_part = h->bias_part + (size_t)l * h->bias_ps;
    // Qwen3: dq / dk are gradients of the NORMED heads; the per-head norm backward turns them into gradients of the
    // projection in place, before the Wqkv weight gradient and the dgrad read d(qkv). No bias, so no column sums: the
    // slab holds the partials of dw_q and dw_k, and the weight gradient takes a hand-over of its own
    if (q3) TK(F_NORM_BWD, st, qknorm_bwd(dqkv, h->QKV, M, nH, nKV, d.head_dim, a.qk_raw, a.qk_rstd, P + o.q_norm, P + o.k_norm, qnb, qkv_part,
                                          qkv_part + (size_t)qnb * d.head_dim, st));
    CK(proj_wgrad(F_WQKV_WGRAD, dqkv, a.x1, o.wqkv, h->QKV, H, q3 ? nullptr : qkv_part));
    CK(slot_done(l));
    TK(F_QKV_DGRAD, st, dgrad(dqkv, o.wqkv, h->dx, h->QKV, H));
    dh = a.hmid;  // grad wrt hs[l]: hmid[l] was last read by the ln2 backward above
    CK(norm_bwd(h->dx, h->hs[l], o.ln1, a.mu1, a.rstd1, dh2, dh, 2 * l));
    return SLAM_OK;
  }
  // The layers [l, l + cnt) are complete: finish their norm / bias partial slabs, one launch per kind of tensor. The order of
  // these launches is the order of their sum-of-squares slots, and slam_grad_norm adds the partials in slot order.
  int finish_slabs(int l, int cnt) {
    const LayerOff& o = h->lo[l];
    const int hd = d.head_dim, nbl = rmsnorm_bwd_blocks(M), nbc = colsum_blocks(M);
    const size_t ls = (size_t)h->layer_stride, lnp = h->ln_ps;
    hipStream_t fs = aux ? ws : st;  // aux: after the norm backward above (the hand-over) and the column sums already on ws
    if (aux) CK(fork());
    CK(finish(h->ln_part + (size_t)(2 * l) * lnp, 2 * lnp, nbl, H, o.ln1, ls, cnt, fs));
    CK(finish(h->ln_part + (size_t)(2 * l + 1) * lnp, 2 * lnp, nbl, H, o.ln2, ls, cnt, fs));
    const float* pq = h->bias_part + (size_t)l * h->bias_ps;
    if (q3) {  // the q / k norm weights: two more slabs, finished like the layer norms'
      CK(finish(pq, h->bias_ps, qnb, hd, o.q_norm, ls, cnt, fs));
      CK(finish(pq + (size_t)qnb * hd, h->bias_ps, qnb, hd, o.k_norm, ls, cnt, fs));
    } else {
      CK(finish(pq, h->bias_ps, nbc, h->QKV, o.bqkv, ls, cnt, fs));
    }
    if (opt) {  // LayerNorm biases, out_proj / fc1 / fc2 biases
      CK(finish(h->lnb_part + (size_t)(2 * l) * lnp, 2 * lnp, nbl, H, o.ln1_b, ls, cnt, fs));
      CK(finish(h->lnb_part + (size_t)(2 * l + 1) * lnp, 2 * lnp, nbl, H, o.ln2_b, ls, cnt, fs));
      CK(finish(h->bo_part + (size_t)l * h->hb_ps, h->hb_ps, nbc, H, o.bo, ls, cnt, fs));
      CK(finish(h->b1_part + (size_t)l * h->ib_ps, h->ib_ps, nbc, I, o.b1, ls, cnt, fs));
      CK(finish(h->b2_part + (size_t)l * h->hb_ps, h->hb_ps, nbc, H, o.b2, ls, cnt, fs));
    }
    return SLAM_OK;
  }
  // a scatter only touches the rows that occur in the batch: a tensor finished by one gets its image from a conversion pass
  // (which also emits its partials when the values kept are the rounded ones)
  int finish_scattered(int64_t off, size_t ne) {
    const bool fused = fin == 2 && partials;  // the conversion sums the squares of the rounded values it stores
    const size_t chunks = (ne + grad_chunk_elems() - 1) / grad_chunk_elems();  // fp32 values kept: chunk sums of the tensor's own range
    const size_t slots = !partials ? 0 : fused ? (size_t)f32_to_bf16_sumsq_slots(ne) : chunks;
    if (h->gn_used + slots > h->gn_cap) return h->fail(SLAM_ESTATE, "gradient-norm partial slots exhausted");
    float* part = h->gn_part + h->gn_used;
    if (fused) CK(f32_to_bf16_sumsq(G + off, IMG + off, ne, part, ws));
    else if (IMG) CK(f32_to_bf16(G + off, IMG + off, ne, ws));  // "grad_final_next" = 2 always has one
    if (partials && !fused) CK(grad_sumsq_chunks(G + off, 0, ne, 0, ne, part, ws));
    h->gn_used += slots;
    return SLAM_OK;
  }
  // gather-side embedding gradient (padding_idx row suppressed): small vocabularies run it as
  // dE += onehot(ids)^T dh0 on the wgrad GEMM, large ones as a token-ordered scatter; both deterministic
  // (on the wgrad stream: ordered after the head's contribution to the same rows)
  int embedding() {
    const int VP = h->vpad;
    CK(fork());
    const int slot = fam_begin(h, F_EMBED_WGRAD, ws);
    // tied: the head wrote (or added to) the tensor above, the gather side always adds. Untied: the gather side is the
    // embedding gradient's only writer - a storing backward stores (one-hot GEMM) or zeroes first (scatter)
    const int eacc = h->untied ? acc : 1;
    if (VP == VPAD_SMALL) {
      CK(onehot(h->last_ids, h->onehot, M, VP, d.vocab, d.pad_token_id, ws));
      CK(take(gemm_tn(h->onehot, dh, G + h->off_embed, eacc, M, VP, H, VP, H, h->gemm_ws, h->gemm_ws_bytes, ws, two ? 1 : 0, img(h->off_embed), sink())));
    } else {
      if (!eacc) CK((int)hipMemsetAsync(G + h->off_embed, 0, (size_t)VP * H * sizeof(float), ws));
      CK(embed_bwd(h->last_ids, dh, G + h->off_embed, M, H, VP, d.vocab, d.pad_token_id, h->embed_ws, ws));
      CK(finish_scattered(h->off_embed, (size_t)VP * H));
    }
    if (opt) {  // learned positions: deterministic token-ordered scatter by position row (no padding_idx), zeroed first when storing
      const size_t ne = (size_t)h->npos * H;
      if (!acc) CK((int)hipMemsetAsync(G + h->off_pos, 0, ne * sizeof(float), ws));
      CK(embed_bwd(h->prow, dh, G + h->off_pos, M, H, h->npos, h->npos, -1, h->embed_ws, ws));
      CK(finish_scattered(h->off_pos, ne));
    }
    fam_end(h, slot, ws);
    return SLAM_OK;
  }
};
}  // namespace

extern "C" {

int slam_backward(SlamEngine* h, float grad_scale, int32_t bucket_layers, slam_bucket_cb cb, void* user,
                  slam_stream_t stream) {
  if (!h) return SLAM_EINVAL;
  if (!h->have_fwd || !h->have_loss) return h->fail(SLAM_ESTATE, "backward needs a forward with labels");
  if (!h->grads) return h->fail(SLAM_ESTATE, "no gradient buffer bound");
  hipStream_t st = (hipStream_t)stream;
  CK(join_optimizer(h, st));
  CK(join_params(h, st));
  h->ag_ev_used = 0;  // every parameter arrival has been waited for: the pool is free for the next step's gathers
  if (h->params_t_dirty) CK(slam_refresh_transposed(h, stream));
  Backward b{h, st};
  if (int r = b.begin(grad_scale, cb != nullptr)) return r;
  GemmTuneScope tune_scope(&h->gemm_tune);
  struct SharedGuard {  // dgrad launches of this call may plan for a GPU they share with the wgrad stream
    GemmTune* t;
    SharedGuard(GemmTune* t_, int on) : t(t_) { t->shared = on; }
    ~SharedGuard() { t->shared = 0; }
  } shared_guard(&h->gemm_tune, b.two ? 1 : 0);
  if (int r = b.head()) return r;
  const int L = b.L, bl = bucket_layers > 0 ? bucket_layers : L;
  int64_t bucket_end = h->n_params;  // exclusive end of the not-yet-reported range
  int fin_hi = L;                    // layers >= fin_hi have their norm/bias partial slabs finished
  for (int l = L - 1; l >= 0; --l) {
    if (int r = b.layer(l)) return r;
    // bucket boundaries: every `bl` layers from the top, and after each of the last two layers so that the
    // final all-reduce (exposed behind the end of backward) only carries layer 0 + the embedding
    const bool boundary = cb && l > 0 && ((((L - l) % bl) == 0) || l <= 2);
    if (l == 0 || boundary) {
      if (int r = b.finish_slabs(l, fin_hi - l)) return r;
      fin_hi = l;
    }
    if (boundary) {
      // the side stream is in order: its last launch of layer l covers every wgrad of the range. Order it after the
      // finish kernels above as well and hand IT to the consumer (slam_bucket_stream): main does not stall here.
      if (!b.aux) CK(b.fork());  // aux: the finish kernels ARE on the side stream, behind a hand-over of their own
      h->bucket_stream = b.two ? b.ws : nullptr;
      cb(user, h->lo[l].ln1, bucket_end - h->lo[l].ln1);
      h->bucket_stream = nullptr;
      bucket_end = h->lo[l].ln1;
    }
  }
  if (int r = b.embedding()) return r;
  if (b.two) CK(b.edge(b.ws, st));  // join: everything after slam_backward on `stream` sees complete gradients
  if (cb) cb(user, 0, bucket_end);
  h->have_loss = false;  // a.gu was consumed; a second backward needs a new forward
  h->gn_valid = b.partials;
  return SLAM_OK;
}

slam_stream_t slam_bucket_stream(SlamEngine* h) { return h ? (slam_stream_t)h->bucket_stream : nullptr; }

int slam_set_logit_mask(SlamEngine* h, const uint8_t* mask) {
  if (!h) return SLAM_EINVAL;
  h->logit_mask = mask;
  return SLAM_OK;
}
int32_t slam_padded_vocab(SlamEngine* h) { return h ? h->vpad : 0; }

int slam_set_label_smoothing(SlamEngine* h, float epsilon) {
  if (!h) return SLAM_EINVAL;
  if (!(epsilon >= 0.f && epsilon < 1.f)) return h->fail(SLAM_EINVAL, "label smoothing epsilon must be in [0, 1)");
  h->label_smoothing = epsilon;
  return SLAM_OK;
}

int slam_set_neftune(SlamEngine* h, float alpha, int64_t seed) {
  if (!h) return SLAM_EINVAL;
  if (!(alpha >= 0.f) || !__builtin_isfinite(alpha)) return h->fail(SLAM_EINVAL, "neftune alpha must be finite and >= 0");
  h->neftune_alpha = alpha;
  h->neftune_seed = (uint64_t)seed;
  if (alpha == 0.f) h->neftune_call_next = -1;
  return SLAM_OK;
}

int slam_seq_loglik(SlamEngine* h, const int64_t* labels, int32_t B, int32_t T, float* ll_out, float* cnt_out,
                    slam_stream_t stream) {
  if (!h || !labels || !ll_out || !cnt_out) return SLAM_EINVAL;
  if (h->have_fwd && h->unpadded) return h->fail(SLAM_ESTATE, "seq_loglik after an unpadded forward: use slam_seq_loglik_unpadded");
  if (!h->have_fwd || B != h->B || T != h->T) return h->fail(SLAM_ESTATE, "seq_loglik needs the matching forward");
  CK(seq_loglik(h->row_loss, labels, B, T, ll_out, cnt_out, (hipStream_t)stream));
  return SLAM_OK;
}

int slam_seq_loglik_unpadded(SlamEngine* h, int32_t B, float* ll_out, float* cnt_out, slam_stream_t stream) {
  if (!h || !ll_out || !cnt_out) return SLAM_EINVAL;
  if (!h->have_fwd || !h->unpadded || !h->up_has_labels || B != h->up_B)
    return h->fail(SLAM_ESTATE, "seq_loglik_unpadded needs the matching unpadded forward with labels");
  CK(seq_loglik_unpadded(h->row_loss, h->up.labels, h->up.off, B, h->B * h->T, ll_out, cnt_out, (hipStream_t)stream));
  return SLAM_OK;
}

int slam_scale_loss_rows(SlamEngine* h, const float* seq_coef, int32_t B, int32_t T, slam_stream_t stream) {
  if (!h || !seq_coef) return SLAM_EINVAL;
  if (h->have_loss && h->unpadded) return h->fail(SLAM_ESTATE, "scale_loss_rows after an unpadded forward: use slam_scale_loss_unpadded");
  if (!h->have_loss || B != h->B || T != h->T) return h->fail(SLAM_ESTATE, "scale_loss_rows needs the matching forward with labels");
  if (h->loss_smoothed) return h->fail(SLAM_ESTATE, "scale_loss_rows after a label-smoothed forward: sequence objectives need the plain loss");
  CK(scale_rows_bf16(h->dlogits, seq_coef, B * T, T, h->vpad, (hipStream_t)stream));
  return SLAM_OK;
}

int slam_scale_loss_unpadded(SlamEngine* h, const float* seq_coef, int32_t B, slam_stream_t stream) {
  if (!h || !seq_coef) return SLAM_EINVAL;
  if (!h->have_fwd || !h->have_loss || !h->unpadded || B != h->up_B)
    return h->fail(SLAM_ESTATE, "scale_loss_unpadded needs the matching unpadded forward with labels");
  if (h->loss_smoothed) return h->fail(SLAM_ESTATE, "scale_loss_unpadded after a label-smoothed forward: sequence objectives need the plain loss");
  CK(scale_rows_unpadded_bf16(h->dlogits, seq_coef, h->up.row, h->B * h->T, h->vpad, (hipStream_t)stream));
  return SLAM_OK;
}

int slam_gateup_launch_ms(SlamEngine* h, float* ms_out, int32_t n) {
  if (!h || !ms_out || n < h->d.n_layers) return SLAM_EINVAL;
  if (!h->time_gateup || h->tg_ev.size() != (size_t)(2 * h->d.n_layers)) return h->fail(SLAM_ESTATE, "set the time_gateup option and run a forward first");
  for (int l = 0; l < h->d.n_layers; ++l) {
    float ms = 0.f;
    hipError_t e = hipEventSynchronize(h->tg_ev[2 * l + 1]);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, h->tg_ev[2 * l], h->tg_ev[2 * l + 1]);
    if (e != hipSuccess) return h->fail((int)e, "gate|up timing events are not recorded");
    ms_out[l] = ms;
  }
  return SLAM_OK;
}

const char* slam_family_name(int32_t family) { return (family >= 0 && family < F_COUNT) ? kFamName[family] : nullptr; }

int slam_family_ms(SlamEngine* h, int32_t* family_out, float* ms_out, int32_t capacity, int32_t* count_out) {
  if (!h || !family_out || !ms_out || !count_out || capacity < 0) return SLAM_EINVAL;
  int32_t n = 0;
  for (const auto& mk : h->fam_marks) {
    if (n >= capacity) break;
    float ms = 0.f;
    hipError_t e = hipEventSynchronize(h->fam_ev[mk.second + 1]);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, h->fam_ev[mk.second], h->fam_ev[mk.second + 1]);
    if (e != hipSuccess) return h->fail((int)e, "family timing events are not recorded (set time_families before the step)");
    family_out[n] = mk.first;
    ms_out[n] = ms;
    ++n;
  }
  *count_out = n;
  return SLAM_OK;
}

int slam_join(SlamEngine* h, slam_stream_t stream) {
  if (!h) return SLAM_EINVAL;
  CK(join_optimizer(h, (hipStream_t)stream));
  CK(join_params(h, (hipStream_t)stream));
  return SLAM_OK;
}

}  // extern "C"
