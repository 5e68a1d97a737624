// The engine's private interface: SlamEngine and what the engine's own translation units share (engine.hip, engine_cache.hip,
// engine_optim.hip, engine_comm.hip). Not part of the C ABI and not for the kernel files: those see kernels.h only.
// Everything shared lives in slam_impl; the entry points of include/slam_engine.h are the only C-named functions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/slam_engine.h"
#include "kernels.h"

using namespace slam;

namespace slam_impl {

constexpr int VPAD_SMALL = 512;  // vocabularies up to 512 (the speech-unit LMs) use the one-wave CE and one-hot wgrad paths
constexpr int GU_BLK = 32;  // Wgu rows / gate|up columns come in blocks of 32 gate + 32 up
constexpr int RC_SLOTS = 3;  // "recompute": shared activation slots (layer l uses slot l mod 3; DESIGN.md has the hazard table)

// OPT (arch 1) keeps fc1 in `wgu` and fc2 in `wd`; ln1_b, bo, ln2_b, b1, b2 are OPT's alone. Qwen3 (arch 3) has no bqkv (-1);
// q_norm, k_norm are Qwen3's alone
struct LayerOff {
  int64_t ln1, wqkv, bqkv, wo, ln2, wgu, wd;
  int64_t ln1_b = -1, bo = -1, ln2_b = -1, b1 = -1, b2 = -1;
  int64_t q_norm = -1, k_norm = -1;
};

// OPT: gu is [M][I] (the layer's d(act) in backward), act the post-ReLU fc1 output; mu1 / mu2 the LayerNorm means
struct LayerAct {
  bf16_t *hmid, *x1, *x2, *qkv, *o, *gu, *act;
  float *rstd1, *rstd2, *lse;
  float *mu1 = nullptr, *mu2 = nullptr;
  // Qwen3: the raw (pre-norm) q|k columns of the projection [M][(nH + nKV) hd] and the heads' rstd [M][nH + nKV]
  bf16_t* qk_raw = nullptr;
  float* qk_rstd = nullptr;
};

}  // namespace slam_impl

using namespace slam_impl;

struct SlamEngine {
  SlamModelDesc d;
  int arch = 0;  // 0 Qwen2, 1 OPT, 3 Qwen3 (slam_engine_create_arch)
  int npos = 0;  // OPT: rows of the learned position table (n_positions + 2, HF's offset)
  int QKV;  // (nH + 2 nKV) * hd
  int vpad = VPAD_SMALL;  // embedding / logits rows: 512, or vocab rounded up to 256 beyond that
  int64_t n_params;
  int64_t off_embed, off_norm, layer_stride = 0;
  int64_t off_pos = -1, off_norm_b = -1;  // OPT
  bool untied = false;   // SLAM_MODEL_UNTIED_HEAD: the head GEMM's weight is the tensor "lm_head" behind the final norm
  int64_t off_head = 0;  // the head's weight: off_embed when tied
  std::vector<LayerOff> lo;
  std::vector<SlamTensorInfo> tensors;
  std::vector<int> layer0;  // indices into `tensors` of layer 0's tensors, in layout order
  std::string err;

  bf16_t* params = nullptr;
  bf16_t* params_t = nullptr;  // transposed weight images (optional)
  float* grads = nullptr;

  // workspace
  char* ws = nullptr;
  size_t ws_bytes = 0;
  int64_t max_tokens = 0;
  std::vector<bf16_t*> hs;  // L+1 residual streams
  std::vector<LayerAct> la;
  bf16_t *hf, *logits, *dlogits, *onehot, *dh_a, *dx, *dact, *dqkv, *d_o;
  int* embed_ws = nullptr;
  const uint8_t* logit_mask = nullptr;  // optional [vpad] bytes: non-zero = column excluded from the softmax
  // slam_set_label_smoothing: epsilon of the loss of every following forward with labels (0 = the plain kernels). The per-row
  // smooth terms live in `dsum` (M * n_heads floats that only the attention backward uses): they are written and summed inside
  // the loss launch sequence itself, so nothing else sees them. loss_smoothed: the last forward's d loss / d logits carries
  // the smoothed target (the sequence-objective scalings refuse it).
  float label_smoothing = 0.f;
  bool loss_smoothed = false;

  // optimizer overlap ("overlap_adamw"): AdamW + the weight-image refresh run in per-layer chunks on an
  // engine-owned side stream; the next forward waits for chunk l right before layer l, so the HBM-bound update of
  // the later layers runs under the MFMA-bound first layers of the next step
  bool overwrite_next = false;  // "grad_overwrite_next": the next backward stores gradients instead of adding to them
  bf16_t* grad_img = nullptr;   // slam_set_grad_image: the next backward also writes every final gradient value there, as bf16
  // "grad_final_next" (round 6): the next backward is the LAST of its optimizer step. 1: every kernel that stores a final
  // gradient value also emits the sum of squares of its block (GradSink, kernels.h) - slam_grad_norm adds ~60 k partials
  // instead of reading the buffer again. 2: additionally the final values go to the bf16 image ONLY (the reference's own
  // gradient precision, config/model/slam.yaml:9): slam_grad_norm / slam_adamw_* then read the image (2 B/param instead of 4).
  int final_next = 0;
  int gfinal = 0;               // what the last backward did (0: plain - gradients in `grads`, norm from chunk sums)
  bf16_t* g16 = nullptr;        // gfinal == 2: where the gradients are
  float* gn_part = nullptr;     // sum-of-squares partials of the last final backward
  size_t gn_cap = 0, gn_used = 0;
  int norm_partials = 1;        // "grad_norm_partials" = 0: never emit them (slam_grad_norm always takes the chunked pass)
  bool gn_valid = false;        // ... and whether they describe the gradients the clip will see: not when that backward reported
                                // buckets to a callback (data parallel: the norm is that of the EXCHANGED gradients, from chunk sums)
  int overlap_adamw = 0;
  // "adamw_sr" / "adamw_sr_seed": the bf16 state stores of AdamW round stochastically (kernels.h AdamSR); stateless - the bits
  // follow from the seed, the step the caller passes and the element's index in the flat buffer
  int adamw_sr = 0;
  uint64_t adamw_sr_seed = 0;
  // slam_set_decay_mask: the tensors that take weight_decay = 0, as the sorted bounds of their merged ranges (kernels.h
  // AdamNoDecay). nd_host decides per parameter group where the optimizer walks the model (adamw_model); nd_dev - engine-owned
  // device memory, the same bounds + the sentinel - is what the flat and ranged kernels search. Empty / null: uniform decay.
  std::vector<uint64_t> nd_host;
  uint64_t* nd_dev = nullptr;
  bool no_decay(int64_t off) const {
    return ((std::upper_bound(nd_host.begin(), nd_host.end(), (uint64_t)off) - nd_host.begin()) & 1) != 0;
  }
  // slam_adafactor_set_segments: the HF parameters over the flat buffer (kernels.h AfSeg), laid out over state and workspace;
  // af_plan.segs - engine-owned device memory - is what the kernels search. af_ws: the caller's workspace.
  std::vector<AfSeg> af_host;
  AfPlan af_plan;
  float* af_ws = nullptr;
  // slam_muon_set_segments: the Muon matrices (kernels.h MuSeg, class order); mu_plan.segs is engine-owned device memory.
  // mu_ws: the caller's workspace (mu_plan.ws_bytes).
  std::vector<MuSeg> mu_host;
  MuPlan mu_plan;
  char* mu_ws = nullptr;
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr;
  std::vector<hipEvent_t> ev_chunk;  // [0] embedding, [1 + l] layer l, [L + 1] final norm (+ an untied lm_head and its transposed image)
  bool opt_pending = false;

  // "bwd_wgrad_stream": the weight-gradient GEMMs of backward run on a second engine-owned stream. They are off the
  // critical path (nothing in backward reads a weight gradient), so their blocks fill the CU slots the dgrad / attention
  // chain leaves idle: the N = 896 launches occupy 448 of 512 block slots, and a kernel in its HBM-bound epilogue
  // (down-proj dgrad with the fused SwiGLU backward) leaves the MFMA pipes free. Event pairs order every wgrad after the
  // kernel that produces its operands and every buffer re-use on the main stream after the wgrad that reads it.
  AttnTune attn_tune = attn_default_tune();
  GemmTune gemm_tune = *gemm_default_tune();
  int wgrad_stream = 1;  // measured +3.6 % step throughput on Slam-358M (282.2k -> 292.3k tok/s, same box)
  // "bwd_aux_side" (round 6): the launches of backward that nothing on the dgrad chain reads - the bias column sums of d(qkv)
  // and the norm / bias finish kernels - go to the weight-gradient stream as well: the caller's stream IS the critical path
  // (every kernel on it feeds the next), the weight-gradient stream has ~230 us of slack per layer
  int aux_side = 1;
  hipStream_t wside = nullptr;
  // "bwd_wgrad_cus" > 0: the wgrad stream is created with a CU mask of that many CUs (the low bits of the mask: on gfx950
  // bit i is XCD i % 8, shader engine (i / 8) % 4, CU i / 32 - a prefix of 32 k bits is k CUs in every shader engine of every
  // XCD), so that the dgrad / attention / RMSNorm chain on the caller's stream always finds CUs the background GEMMs cannot
  // occupy. hipExtStreamCreateWithCUMask makes a BLOCKING stream: it synchronises implicitly with the NULL stream, so the
  // caller must then run the step on a non-default stream (the trainer and bench.py do when the option is set).
  int wside_cus = 0, wside_cus_applied = 0;
  bool time_gateup = false;        // "time_gateup": timing events around every gate|up projection launch of a forward
  std::vector<hipEvent_t> tg_ev;   // 2 per layer
  // "time_families": timing-event pairs around the launches of every family of slam_forward / slam_backward (slam_family_ms),
  // each on the stream the launch goes to - the in-step duration of a launch between its real neighbours, what a kernel
  // trace shows for it. Two more packets per launch: measurement steps only.
  bool time_families = false;
  std::vector<hipEvent_t> fam_ev;                 // pool, reused step after step
  std::vector<std::pair<int, size_t>> fam_marks;  // (family id, index of the pair's first event)
  hipStream_t bucket_stream = nullptr;  // see slam_bucket_stream
  // engine-side gradient exchange (slam_comm_*): one RCCL communicator, one communication stream, an event pool
  void* comm = nullptr;                 // ncclComm_t
  int comm_world = 0, comm_rank = 0;
  std::vector<hipEvent_t> ag_ev;        // "parameters of this bucket have arrived" (slam_allgather_params_async -> the next forward)
  size_t ag_ev_used = 0;
  hipStream_t comm_stream = nullptr;
  std::vector<hipEvent_t> comm_ev;
  size_t comm_ev_used = 0;
  bf16_t* last_grad_img = nullptr;      // the image the last slam_backward wrote (slam_allreduce_grads_async, bf16 exchange)
  std::vector<hipEvent_t> ev_w;  // per layer (+1 for the head / embedding): 4 main->side, 3 side->main
  // "recompute" (see slam_set_option in the header): 0 every layer keeps its forward activations, 1 x1 / x2 / act live in
  // min(L, 3) shared slots and are rebuilt in backward, 2 the whole LayerAct does and backward re-runs the layer's forward
  int recompute = 0;
  std::vector<hipEvent_t> ev_rc;  // per layer: "the weight-gradient stream is done with layer l" (orders the slot re-use)
  // Residual dropout (OPT; see slam_set_option in the header). "dropout_call_next" arms the NEXT slam_forward only; that forward
  // copies (thr, seed, call) into fwd_drop for its own backward and recomputation. Nothing of the mask is stored.
  int dropout_thr16 = 0;
  uint64_t dropout_seed = 0;
  int64_t dropout_call_next = -1;  // -1: not armed
  bool fwd_drop = false;           // the last slam_forward applied dropout ...
  DropSite fwd_site;               // ... with these (site and index0 filled per launch)
  // NEFTune (slam_set_neftune in the header): "neftune_call_next" arms the NEXT slam_forward only; that forward's embedding
  // launch draws the noise. Nothing is stored and nothing re-runs the launch: the residual streams hs[l] are kept at every
  // "recompute" level.
  float neftune_alpha = 0.f;
  uint64_t neftune_seed = 0;
  int64_t neftune_call_next = -1;  // -1: not armed
  bool fwd_neft = false;           // forward_layers launches the noisy gather ...
  NeftSite fwd_neft_site;          // ... with these
  // backward's masked copies of the residual gradients, [layer parity][site] x [M][H]: the weight-gradient stream reads layer
  // l's after the caller's stream has moved on, so layer l - 2 waits for ev_dm[l] before it overwrites them
  bf16_t* dmask[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
  std::vector<hipEvent_t> ev_dm;   // per layer: "the weight-gradient stream is done with layer l's masked gradients"

  ~SlamEngine() {
    if (wside) { (void)hipStreamSynchronize(wside); (void)hipStreamDestroy(wside); }
    for (hipEvent_t e : fam_ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : ev_w) (void)hipEventDestroy(e);
    for (hipEvent_t e : ev_rc) (void)hipEventDestroy(e);
    for (hipEvent_t e : ev_dm) (void)hipEventDestroy(e);
    if (side) { (void)hipStreamSynchronize(side); (void)hipStreamDestroy(side); }
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    for (hipEvent_t e : ev_chunk) (void)hipEventDestroy(e);
    for (hipEvent_t e : pw_ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : tg_ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : comm_ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : ag_ev) (void)hipEventDestroy(e);
    if (comm_stream) { (void)hipStreamSynchronize(comm_stream); (void)hipStreamDestroy(comm_stream); }
    if (nd_dev) (void)hipFree(nd_dev);
    if (af_plan.segs) (void)hipFree((void*)af_plan.segs);
    if (mu_plan.segs) (void)hipFree((void*)mu_plan.segs);
  }
  // parameter ranges another stream is still writing (sharded optimizer: the bf16 parameter all-gather on the
  // communication stream): the next reader waits for the event right before its first read of the range
  struct ParamWait { int64_t lo, hi; hipEvent_t ev; };
  std::vector<ParamWait> pwaits;
  std::vector<hipEvent_t> pw_ev;   // timing pairs around the waits (exposed all-gather time), reused step after step
  size_t pw_used = 0;
  double pw_acc_ms = 0.0;          // waits whose event pairs were folded into a sum when the pool filled up (not yet reported)
  int64_t pw_untimed = 0;          // waits that could not be bracketed (pool full of pairs still in flight): reported, never silent
  bool params_t_dirty = false;     // ranged optimizer updates leave the transposed weight images stale until backward needs them
  bool time_param_waits = false;   // "time_param_waits": bracket the parameter waits of a forward with timing events (slam_param_wait_ms)
  float* nlse = nullptr;
  float *cosq = nullptr, *sinq = nullptr;  // the query heads' RoPE tables: cos / sin times head_dim^-0.5 * log2(e)
  float *rstdf, *row_loss, *dsum, *dkv_part, *cosb, *sinb, *gemm_ws, *part_ws, *scal;
  // per-layer partial slabs: [2L][nb_ln][H], [L][nb_cs][QKV]. Qwen3 has no q|k|v bias: layer l's slab holds the partials of
  // dw_q [qn_blocks][hd] and, behind them, of dw_k (qn_blocks caps the launch so that both fit)
  float *ln_part, *bias_part;
  size_t ln_ps = 0, bias_ps = 0;
  // OPT: LayerNorm bias slabs [2L][nb_ln][H]; bo, b1, b2 slabs [L][nb_cs][H | I | H]; final-norm mean; position rows of the tokens
  float *lnb_part = nullptr, *bo_part = nullptr, *b1_part = nullptr, *b2_part = nullptr, *muf = nullptr;
  size_t hb_ps = 0, ib_ps = 0;
  int64_t* prow = nullptr;
  size_t gemm_ws_bytes = 0;
  int *seg_s, *seg_e, *attn_plan_buf;

  // last forward
  int B = 0, T = 0;
  bool have_fwd = false, have_loss = false;
  bool fuse_swiglu = false, fuse_dswiglu = true;
  bool fuse_adamw_t = true;  // "fuse_adamw_t": AdamW writes the transposed weight images itself (0: separate transpose pass)
  const int64_t* last_ids = nullptr;
  // the last forward was slam_forward_unpadded over up_B x up_T: (B, T) = (1, M_packed), `up` its packed arrays (borrowed
  // scratch) - slam_seq_loglik_unpadded / slam_scale_loss_unpadded read them, the dense-row forms are refused
  bool unpadded = false;
  UnpadView up{};
  int up_B = 0, up_T = 0;
  bool up_has_labels = false;
  int64_t last_tokens = 0;  // token rows the last forward executed (slam_last_forward_tokens)
  const int* cur_seg_s = nullptr;
  const int* cur_seg_e = nullptr;

  // KV cache of slam_prefill / slam_decode_step (caller-owned): per layer K[kv_bmax][nKV][kv_cap][hd] then V (same shape)
  bf16_t* kv = nullptr;
  int kv_bmax = 0, kv_cap = 0;
  int kv_B = 0;          // rows of the last prefill
  int kv_hi = 0;         // host bound of every row's cached length: the prefill's T, + 1 per decode step, + T per slam_extend
  int kv_T = 0;          // the last prefill's T + the T of every slam_extend that no decode step preceded: kv_hi != kv_T once
                         // a decode step was taken (slam_kv_repeat)
  bool kv_ready = false; // a prefill filled the bound cache

  // FP8 copy of the decode projections (slam_bind_decode_w8, caller-owned): codes + exponents of wqkv, wo, wgu, wd of every
  // layer, then of the head matrix when w8_head. w8_valid: the codes describe the bound parameters (slam_quantize_decode_w8
  // set it; every entry point that writes or rebinds parameters clears it, and decode_proj then reads the bf16 parameters)
  struct W8Mat { int N, K; uint8_t* q; int8_t* e; };
  char* w8 = nullptr;
  bool w8_head = false, w8_valid = false;
  int64_t w8_launches = 0;
  std::unordered_map<int64_t, W8Mat> w8_mats;  // by the matrix's offset in the parameter buffer

  int fail(int code, const std::string& m) {
    err = m;
    return code;
  }
};

#define CK(expr)                                                                     \
  do {                                                                               \
    int _r = (expr);                                                                 \
    if (_r != 0) {                                                                   \
      char _b[256];                                                                  \
      snprintf(_b, sizeof(_b), "%s failed with %d (%s) at %s:%d", #expr, _r,         \
               _r > 0 ? hipGetErrorString((hipError_t)_r) : "engine", __FILE__, __LINE__); \
      return h->fail(_r, _b);                                                        \
    }                                                                                \
  } while (0)

namespace slam_impl {

// launch families of the step (slam_family_name); ids are stable within a library build only
enum Fam {
  F_QKV_FWD, F_ATTN_FWD, F_O_FWD, F_GATEUP_FWD, F_DOWN_FWD, F_NORM_FWD, F_HEAD_FWD, F_LOSS,
  F_DOWN_DGRAD, F_GATEUP_DGRAD, F_O_DGRAD, F_QKV_DGRAD, F_ATTN_BWD, F_NORM_BWD, F_HEAD_DGRAD,
  F_WD_WGRAD, F_WGU_WGRAD, F_WO_WGRAD, F_WQKV_WGRAD, F_HEAD_WGRAD, F_EMBED_WGRAD, F_COUNT
};

// Defined in engine.hip, beside their comments: the streams and events of the engine, the waits for a pending optimizer step
// and for parameters in flight, the family's row norm, the decoder layer loop and the refresh of the transposed weight images.
unsigned sync_event_flags();
int fam_begin(SlamEngine* h, int fam, hipStream_t st);
void fam_end(SlamEngine* h, int slot, hipStream_t st);
int ensure_side(SlamEngine* h);
int wait_chunk(SlamEngine* h, int i, hipStream_t st);
int join_optimizer(SlamEngine* h, hipStream_t st);
int wait_params(SlamEngine* h, int64_t lo, int64_t hi, hipStream_t st);
int join_params(SlamEngine* h, hipStream_t st);
int norm_fwd(SlamEngine* h, const bf16_t* x, int64_t woff, int64_t boff, bf16_t* y, float* mu, float* rstd, int M, hipStream_t st);
int forward_layers(SlamEngine* h, const int64_t* ids, const int64_t* position_ids, const int32_t* seg_start,
                   const int32_t* seg_end, int M, int T, hipStream_t st, const int32_t* kv_lens = nullptr, int kv_B = 0);
int refresh_transposed_images(SlamEngine* h, slam_stream_t stream);

// CK around a launch (or a short run of launches) of one family on one stream
#define TK(fam, stream_, expr)                      \
  do {                                              \
    const int _slot = fam_begin(h, (fam), (stream_)); \
    CK(expr);                                       \
    fam_end(h, _slot, (stream_));                   \
  } while (0)

// The parameter layout as the optimizer and the refresh of the transposed images walk it: fn(offset, rows, cols, batch) for
// every group of `batch` same-shaped tensors at a stride of layer_stride; cols == 1: a vector of `rows` elements (no GEMM reads
// a transposed image of one). Here the tensors of layers l0 .. l0 + nl, one group per tensor kind, in layer 0's layout order.
template <typename F>
int for_each_layer_tensor(SlamEngine* h, int l0, int nl, F&& fn) {
  for (int ti : h->layer0) {
    const SlamTensorInfo& t = h->tensors[ti];
    if (int r = fn(t.offset + (int64_t)l0 * h->layer_stride, t.rows, (int)t.cols, nl)) return r;
  }
  return 0;
}
// chunk 0 = embedding (+ OPT's positions), 1 + l = decoder layer l, L + 1 = final norm (+ bias) and, with an untied head, lm_head
// (the tensors behind the layers; forward joins the last chunk before the head GEMM); chunk < 0 = all, the layers as batches of L
template <typename F>
int for_each_param_group(SlamEngine* h, int chunk, F&& fn) {
  const int L = h->d.n_layers, H = h->d.hidden;
  int r = 0;
  if (chunk <= 0) {
    r = fn(h->off_embed, h->vpad, H, 1);
    if (!r && h->arch == 1) r = fn(h->off_pos, (int64_t)h->npos * H, 1, 1);
  }
  if (!r && chunk < 0) r = for_each_layer_tensor(h, 0, L, fn);
  if (!r && chunk >= 1 && chunk <= L) r = for_each_layer_tensor(h, chunk - 1, 1, fn);
  if (!r && (chunk < 0 || chunk == L + 1)) {
    r = fn(h->off_norm, H, 1, 1);
    if (!r && h->arch == 1) r = fn(h->off_norm_b, H, 1, 1);
    if (!r && h->untied) r = fn(h->off_head, h->vpad, H, 1);
  }
  return r;
}
// the separate transpose pass as a visitor of the same walk: one launch per group of matrices, grid.z = batch
inline auto transpose_group(SlamEngine* h, hipStream_t st) {
  return [h, st](int64_t off, int64_t rows, int cols, int batch) {
    return cols == 1 ? 0 : transpose_bf16(h->params + off, h->params_t + off, (int)rows, cols, batch, (size_t)h->layer_stride, st);
  };
}

// K and V of layer l in the bound cache
inline bf16_t* kv_k(SlamEngine* h, int l) {
  return h->kv + (size_t)l * 2 * h->kv_bmax * h->d.n_kv_heads * h->kv_cap * h->d.head_dim;
}
inline bf16_t* kv_v(SlamEngine* h, int l) { return kv_k(h, l) + (size_t)h->kv_bmax * h->d.n_kv_heads * h->kv_cap * h->d.head_dim; }

}  // namespace slam_impl
