// C ABI + step orchestration of the Slam engine (see include/slam_engine.h).
// Replaces everything below UnitLM.forward / Trainer.training_step in the reference call stack
// (SURVEY.md §3.1-3.2): Qwen2Model.forward (modeling_qwen2.py:342-402), the tied lm_head (:465),
// compute_loss (unit_lm.py:13-29), autograd backward, clip_grad_norm_ and AdamW.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <dlfcn.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

// RCCL: types only - the library is looked up at run time (slam_comm_*). A box without the RCCL headers still builds the engine
// (the handful of declarations below follow rccl.h / nccl.h; their values are part of the library's stable ABI).
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
#else
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclInt8 = 0, ncclUint8 = 1, ncclInt32 = 2, ncclUint32 = 3, ncclInt64 = 4, ncclUint64 = 5, ncclFloat16 = 6, ncclFloat32 = 7,
               ncclFloat64 = 8, ncclBfloat16 = 9 } ncclDataType_t;
typedef enum { ncclSum = 0 } ncclRedOp_t;
#endif

#include "../../include/slam_engine.h"
#include "kernels.h"

using namespace slam;

namespace {

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

}  // namespace

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

namespace {

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

// Flags of the events that only order the engine's streams among themselves. Without hipEventDisableSystemFence every
// hipEventRecord carries a SYSTEM-scope release - cache write-back and invalidation in the middle of the backward, seven
// times per layer; nothing on the host reads device memory through these events (SLAM_EVENT_SYSTEM_FENCE=1 restores it).
static unsigned sync_event_flags() {
  static const unsigned f = [] {
    const char* e = getenv("SLAM_EVENT_SYSTEM_FENCE");
    return (unsigned)hipEventDisableTiming | ((e && e[0] == '1') ? 0u : (unsigned)hipEventDisableSystemFence);
  }();
  return f;
}

// launch families of the step (slam_family_name); ids are stable within a library build only
enum Fam {
  F_QKV_FWD, F_ATTN_FWD, F_O_FWD, F_GATEUP_FWD, F_DOWN_FWD, F_NORM_FWD, F_HEAD_FWD, F_LOSS,
  F_DOWN_DGRAD, F_GATEUP_DGRAD, F_O_DGRAD, F_QKV_DGRAD, F_ATTN_BWD, F_NORM_BWD, F_HEAD_DGRAD,
  F_WD_WGRAD, F_WGU_WGRAD, F_WO_WGRAD, F_WQKV_WGRAD, F_HEAD_WGRAD, F_EMBED_WGRAD, F_COUNT
};
const char* const kFamName[F_COUNT] = {
    "qkv_fwd", "attn_fwd", "o_fwd", "gateup_fwd", "down_fwd", "norm_fwd", "head_fwd", "loss",
    "down_dgrad_dswiglu", "gateup_dgrad", "o_dgrad", "qkv_dgrad", "attn_bwd", "norm_bwd", "head_dgrad",
    "wd_wgrad", "wgu_wgrad", "wo_wgrad", "wqkv_wgrad", "head_wgrad", "embed_wgrad"};

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
// CK around a launch (or a short run of launches) of one family on one stream
#define TK(fam, stream_, expr)                      \
  do {                                              \
    const int _slot = fam_begin(h, (fam), (stream_)); \
    CK(expr);                                       \
    fam_end(h, _slot, (stream_));                   \
  } while (0)

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
// AdamW (`a`: the update at element 0 of the flat buffers) over a chunk of the model with transposed weight images bound:
// every matrix goes through the tile kernel that writes its transposed image in the same pass (no separate transpose launch),
// the vectors between them through the strided kernel. A group is whole tensors, so the no-decay set (slam_set_decay_mask) is
// applied here, on the host: a tensor outside the decay set is launched with wd = 0 through the same kernels, and a batch of
// layers goes out layer by layer only where the flags differ across the layers (never under the HF rule).
int adamw_model(SlamEngine* h, const AdamArgs& a, int chunk, hipStream_t st) {
  return for_each_param_group(h, chunk, [&](int64_t off, int64_t rows, int cols, int batch) {
    auto run = [&](int64_t o, int nb, bool decay) {
      AdamArgs g = a.at(o);
      g.nd = AdamNoDecay{};
      if (!decay) g.wd = 0;
      if (cols == 1) return adamw_strided(g, (size_t)rows, nb, (size_t)h->layer_stride, st);
      return adamw_tiles(g, (int)rows, cols, nb, (size_t)h->layer_stride, st);
    };
    if (h->nd_host.empty()) return run(off, batch, true);
    const bool nd0 = h->no_decay(off);
    bool same = true;
    for (int l = 1; l < batch; ++l) same = same && h->no_decay(off + l * h->layer_stride) == nd0;
    if (same) return run(off, batch, !nd0);
    for (int l = 0; l < batch; ++l) {
      const int64_t o = off + l * h->layer_stride;
      if (int r = run(o, 1, !h->no_decay(o))) return r;
    }
    return 0;
  });
}
// the separate transpose pass as a visitor of the same walk: one launch per group of matrices, grid.z = batch
auto transpose_group(SlamEngine* h, hipStream_t st) {
  return [h, st](int64_t off, int64_t rows, int cols, int batch) {
    return cols == 1 ? 0 : transpose_bf16(h->params + off, h->params_t + off, (int)rows, cols, batch, (size_t)h->layer_stride, st);
  };
}

// K and V of layer l in the bound cache
bf16_t* kv_k(SlamEngine* h, int l) {
  return h->kv + (size_t)l * 2 * h->kv_bmax * h->d.n_kv_heads * h->kv_cap * h->d.head_dim;
}
bf16_t* kv_v(SlamEngine* h, int l) { return kv_k(h, l) + (size_t)h->kv_bmax * h->d.n_kv_heads * h->kv_cap * h->d.head_dim; }

// Qwen3: blocks of the q / k norm backward over M tokens - what the kernel would like, capped so that the two partial slabs
// fit the layer's (otherwise unused) bias slab of colsum_blocks(M) x QKV floats: at least 3 / 2 colsum_blocks(M) blocks
int qn_blocks(const SlamEngine* h, int M) {
  const SlamModelDesc& d = h->d;
  const int want = qknorm_bwd_blocks(M, d.n_heads, d.n_kv_heads, d.head_dim);
  const int cap = (int)((size_t)colsum_blocks(M) * h->QKV / (2 * (size_t)d.head_dim));
  return want < cap ? want : cap;
}

// The family's row norm over M rows: LayerNorm with a bias and a saved mean (OPT; boff and mu are OPT's alone), else RMSNorm
int norm_fwd(SlamEngine* h, const bf16_t* x, int64_t woff, int64_t boff, bf16_t* y, float* mu, float* rstd, int M, hipStream_t st) {
  const bf16_t* P = h->params;
  if (h->arch == 1) return layernorm_fwd(x, P + woff, P + boff, y, mu, rstd, M, h->d.hidden, h->d.rms_eps, st);
  return rmsnorm_fwd(x, P + woff, y, rstd, M, h->d.hidden, h->d.rms_eps, st);
}

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

// The decoder layer loop of a forward over M = B*T tokens: segments, attention plan, RoPE tables, embedding and every layer,
// leaving the last residual stream in hs[L] (slam_forward and slam_prefill continue from there). kv_lens (slam_prefill over
// kv_B rows, and only when the layers share their q|k|v buffer): each layer's K / V go to the cache before the next layer
// overwrites them.
int forward_layers(SlamEngine* h, const int64_t* ids, const int64_t* position_ids, const int32_t* seg_start,
                   const int32_t* seg_end, int M, int T, hipStream_t st, const int32_t* kv_lens = nullptr, int kv_B = 0) {
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

}  // namespace

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
static int refresh_transposed_images(SlamEngine* h, slam_stream_t stream);
// the caller wrote the parameters: FP8 decode codes made from the earlier values are stale
int slam_refresh_transposed(SlamEngine* h, slam_stream_t stream) {
  if (!h) return SLAM_EINVAL;
  h->w8_valid = false;
  return refresh_transposed_images(h, stream);
}
static int refresh_transposed_images(SlamEngine* h, slam_stream_t stream) {
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

// slam_forward, and the tail of slam_forward_unpadded: `up` = the packed arrays of a padding-free call over up_B x up_T (ids ..
// seg_end then point into them and (B, T) = (1, M_packed)); its logits go back to the batch's own layout.
static int forward_common(SlamEngine* h, const int64_t* ids, const int64_t* labels, const int64_t* position_ids,
                          const int32_t* seg_start, const int32_t* seg_end, int32_t B, int32_t T, double num_items,
                          float* loss_out, void* logits_out, const UnpadView* up, int up_B, int up_T, slam_stream_t stream) {
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
  if (logits_out && up) CK(unpad_logits(h->logits, VP, (bf16_t*)logits_out, d.vocab, up->off, up_B, up_T, M, st));
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

int slam_forward(SlamEngine* h, const int64_t* ids, const int64_t* labels, const int64_t* position_ids,
                 const int32_t* seg_start, const int32_t* seg_end, int32_t B, int32_t T, double num_items,
                 float* loss_out, void* logits_out, slam_stream_t stream) {
  if (!h) return SLAM_EINVAL;
  return forward_common(h, ids, labels, position_ids, seg_start, seg_end, B, T, num_items, loss_out, logits_out, nullptr, 0, 0,
                        stream);
}

size_t slam_unpadded_scratch_bytes(int32_t B, int32_t T) {
  if (B <= 0 || T <= 0 || (int64_t)B * T > 0x7fffffc0LL) return 0;
  return unpad_scratch_bytes(B, T);
}

int slam_forward_unpadded(SlamEngine* h, const int64_t* ids, const int64_t* labels, const int32_t* lens, int32_t B, int32_t T,
                          int32_t M_packed, void* scratch, size_t scratch_bytes, double num_items, float* loss_out,
                          void* logits_out, slam_stream_t stream) {
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
  int rc = unpad_pack(ids, labels, lens, B, T, M_packed, h->d.pad_token_id, v, (hipStream_t)stream);
  if (rc != 0) { h->dropout_call_next = h->neftune_call_next = -1; return rc; }
  h->dropout_call_next = armed_call;
  h->neftune_call_next = neft_call;
  return forward_common(h, v.ids, labels ? v.labels : nullptr, v.pos, v.seg_s, v.seg_e, 1, M_packed, num_items, loss_out, logits_out,
                        &v, B, T, stream);
}

int64_t slam_last_forward_tokens(SlamEngine* h) { return h && h->have_fwd ? h->last_tokens : 0; }

int slam_op_unpad_pack(const int64_t* ids, const int64_t* labels, const int32_t* lens, int32_t B, int32_t T, int32_t M_packed,
                       int32_t pad_id, void* scratch, size_t scratch_bytes, slam_stream_t s) {
  if (!ids || !lens || !scratch || B <= 0 || T <= 0 || (int64_t)B * T > 0x7fffffc0LL) return SLAM_EINVAL;
  const int64_t mmax = (((int64_t)B * T + 63) / 64) * 64;
  if (M_packed <= 0 || (M_packed & 63) || M_packed > mmax) return SLAM_EINVAL;
  if (((uintptr_t)scratch & 255) || scratch_bytes < unpad_scratch_bytes(B, T)) return SLAM_EINVAL;
  return unpad_pack(ids, labels, lens, B, T, M_packed, pad_id, unpad_view(scratch, B, T), (hipStream_t)s);
}

/* ---- KV-cached generation ---------------------------------------------------------------------------------------------*/
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
// residual. static: a function of an unnamed namespace inside extern "C" keeps its C name and appears in the dynamic symbol table
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
}  // namespace

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

namespace {
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

int slam_grad_norm(SlamEngine* h, float max_norm, float* norm_out, slam_stream_t stream) {
  if (!h || !norm_out) return SLAM_EINVAL;
  if (!h->grads || !h->ws) return h->fail(SLAM_ESTATE, "bind params and workspace first");
  CK(join_optimizer(h, (hipStream_t)stream));
  if (h->gn_valid) {  // the last backward emitted the partial sums of squares with its final-value stores: add them, in slot order
    CK(grad_norm_from_chunks(h->gn_part, h->gn_used, max_norm, norm_out, (hipStream_t)stream));
    return SLAM_OK;
  }
  // chunk sums over the buffer the gradients are in (the bf16 image after a "grad_final_next" = 2 backward whose buckets were exchanged)
  const int g16 = h->gfinal == 2;
  const size_t n = (size_t)h->n_params;
  CK(grad_sumsq_chunks(g16 ? (const void*)h->g16 : (const void*)h->grads, g16, n, 0, n, h->part_ws, (hipStream_t)stream));
  CK(grad_norm_from_chunks(h->part_ws, (n + grad_chunk_elems() - 1) / grad_chunk_elems(), max_norm, norm_out, (hipStream_t)stream));
  return SLAM_OK;
}

// the update as the engine's state fixes it, at element 0 of the flat buffers (the gradients where the last backward left
// them); the state arrays are the caller's
static AdamArgs adam_args(SlamEngine* h, int mode, const float* norm_out, double lr, double b1, double b2, double eps, double wd,
                          int step, int zero_grad) {
  AdamArgs a;
  a.mode = mode;
  a.params = h->params;
  a.params_t = h->params_t;
  a.g_bf16 = h->gfinal == 2;  // the last backward kept its final values in bf16 only (slam_set_grad_image's buffer)
  a.g = a.g_bf16 ? (void*)h->g16 : (void*)h->grads;
  a.clip = norm_out;
  a.lr = lr; a.b1 = b1; a.b2 = b2; a.eps = eps; a.wd = wd;
  a.step = step; a.zero_grad = zero_grad;
  a.sr.on = h->adamw_sr; a.sr.seed = h->adamw_sr_seed;
  if (h->nd_dev) { a.nd.bounds = h->nd_dev; a.nd.n = (int)h->nd_host.size(); }
  return a;
}

static int adamw_any(SlamEngine* h, int mode, float* master, void* m, void* v, const float* norm_out, double lr, double b1, double b2,
                     double eps, double wd, int32_t step, int32_t zero_grad, slam_stream_t stream) {
  if (!h || !m || !v || step < 1 || (mode != 2 && !master)) return SLAM_EINVAL;
  if (!h->grads || !h->params) return h->fail(SLAM_ESTATE, "bind params first");
  if (h->n_params & 7) return h->fail(SLAM_EINVAL, "parameter count must be a multiple of 8");
  hipStream_t st = (hipStream_t)stream;
  CK(join_optimizer(h, st));
  CK(join_params(h, st));
  h->w8_valid = false;
  const bool fused = h->params_t != nullptr && h->fuse_adamw_t;
  AdamArgs a = adam_args(h, mode, norm_out, lr, b1, b2, eps, wd, step, zero_grad);
  a.master = master; a.m = m; a.v = v;
  // zeroing belongs to the fp32 accumulation buffer: the kernels cannot do it while they read the bf16 image
  if (a.g_bf16 && zero_grad) CK((int)hipMemsetAsync(h->grads, 0, (size_t)h->n_params * sizeof(float), st));
  if (!h->overlap_adamw || mode != 0) {
    if (fused) {
      CK(adamw_model(h, a, -1, st));
      h->params_t_dirty = false;
      return SLAM_OK;
    }
    CK(adamw_flat(a, (size_t)h->n_params, st));
    return slam_refresh_transposed(h, stream);
  }
  // "overlap_adamw" (fp32 state): per-layer chunks on the engine's side stream; the next forward waits per layer
  CK(ensure_side(h));
  CK((int)hipEventRecord(h->ev_fork, st));
  CK((int)hipStreamWaitEvent(h->side, h->ev_fork, 0));
  const int L = h->d.n_layers;
  for (int c = 0; c < L + 2; ++c) {
    if (fused) {
      CK(adamw_model(h, a, c, h->side));
    } else {
      const int64_t lo = c == 0 ? 0 : c <= L ? h->lo[c - 1].ln1 : h->off_norm;
      const int64_t hi = c == 0 ? h->lo[0].ln1 : c < L ? h->lo[c].ln1 : c == L ? h->off_norm : h->n_params;
      CK(adamw_flat(a.at(lo), (size_t)(hi - lo), h->side));
      if (h->params_t) CK(for_each_param_group(h, c, transpose_group(h, h->side)));
    }
    CK((int)hipEventRecord(h->ev_chunk[c], h->side));
  }
  h->opt_pending = true;
  return SLAM_OK;
}

int slam_adamw_step(SlamEngine* h, float* master, float* m, float* v, const float* norm_out, double lr, double b1,
                    double b2, double eps, double wd, int32_t step, int32_t zero_grad, slam_stream_t stream) {
  return adamw_any(h, 0, master, m, v, norm_out, lr, b1, b2, eps, wd, step, zero_grad, stream);
}

int slam_adamw_step_bf16_moments(SlamEngine* h, float* master, void* exp_avg_bf16, void* exp_avg_sq_bf16, const float* norm_out,
                                 double lr, double b1, double b2, double eps, double wd, int32_t step, int32_t zero_grad,
                                 slam_stream_t stream) {
  return adamw_any(h, 1, master, exp_avg_bf16, exp_avg_sq_bf16, norm_out, lr, b1, b2, eps, wd, step, zero_grad, stream);
}

int slam_adamw_step_bf16(SlamEngine* h, void* exp_avg_bf16, void* exp_avg_sq_bf16, const float* norm_out, double lr,
                         double b1, double b2, double eps, double wd, int32_t step, int32_t zero_grad, slam_stream_t stream) {
  return adamw_any(h, 2, nullptr, exp_avg_bf16, exp_avg_sq_bf16, norm_out, lr, b1, b2, eps, wd, step, zero_grad, stream);
}

// ---- sharded optimizer (data-parallel "rs_ag": reduce-scatter gradients, update the owned 1/N shard, all-gather bf16
// parameters) ------------------------------------------------------------------------------------------------------
int64_t slam_grad_chunk_elems(void) { return grad_chunk_elems(); }
int slam_grad_sumsq_chunks(SlamEngine* h, int64_t offset, int64_t count, float* chunk_sums, slam_stream_t stream) {
  if (!h || !chunk_sums || offset < 0 || count < 0) return SLAM_EINVAL;
  if (!h->grads) return h->fail(SLAM_ESTATE, "no gradient buffer bound");
  const int g16 = h->gfinal == 2;  // the gradients (a reduced shard of them) are in the bf16 image
  int r = grad_sumsq_chunks(g16 ? (const void*)h->g16 : (const void*)h->grads, g16, (size_t)h->n_params, (size_t)offset, (size_t)count, chunk_sums,
                            (hipStream_t)stream);
  if (r < 0) return h->fail(SLAM_EINVAL, "range must start on a chunk boundary and end on one (or at the end of the buffer)");
  CK(r);
  return SLAM_OK;
}

int slam_grad_norm_from_chunks(SlamEngine* h, const float* chunk_sums, float max_norm, float* norm_out, slam_stream_t stream) {
  if (!h || !chunk_sums || !norm_out) return SLAM_EINVAL;
  const size_t nc = ((size_t)h->n_params + grad_chunk_elems() - 1) / grad_chunk_elems();
  CK(grad_norm_from_chunks(chunk_sums, nc, max_norm, norm_out, (hipStream_t)stream));
  return SLAM_OK;
}

// the three slam_adamw_range* entry points: elements [offset, offset + count) of the engine's buffers against the caller's
// shard of the state, which starts at that element (master: NULL in mode 2). Mode 2 updates 8 elements per thread, the others 4.
static int adamw_range_impl(SlamEngine* h, int mode, int64_t offset, int64_t count, float* master, void* m, void* v, const float* norm_out,
                            double lr, double b1, double b2, double eps, double wd, int32_t step, int32_t zero_grad, slam_stream_t stream) {
  const int64_t mask = mode == 2 ? 7 : 3;
  if (!h || (mode != 2 && !master) || !m || !v || step < 1 || offset < 0 || count < 0 || offset + count > h->n_params || (offset & mask) ||
      (count & mask))
    return SLAM_EINVAL;
  if (!h->grads || !h->params) return h->fail(SLAM_ESTATE, "bind params first");
  hipStream_t st = (hipStream_t)stream;
  CK(join_optimizer(h, st));
  h->w8_valid = false;
  AdamArgs a = adam_args(h, mode, norm_out, lr, b1, b2, eps, wd, step, zero_grad).at(offset);
  a.master = master; a.m = m; a.v = v;
  // as in adamw_any: the kernels cannot clear the fp32 accumulation buffer while they read the bf16 image - here the range only
  if (a.g_bf16 && zero_grad && count) CK((int)hipMemsetAsync(h->grads + offset, 0, (size_t)count * sizeof(float), st));
  if (count) CK(adamw_flat(a, (size_t)count, st));
  h->params_t_dirty = h->params_t != nullptr;
  return SLAM_OK;
}

int slam_adamw_range(SlamEngine* h, int64_t offset, int64_t count, float* master, float* m, float* v, const float* norm_out,
                     double lr, double b1, double b2, double eps, double wd, int32_t step, int32_t zero_grad,
                     slam_stream_t stream) {
  return adamw_range_impl(h, 0, offset, count, master, m, v, norm_out, lr, b1, b2, eps, wd, step, zero_grad, stream);
}

int slam_adamw_range_bf16_moments(SlamEngine* h, int64_t offset, int64_t count, float* master, void* m_bf16, void* v_bf16,
                                  const float* norm_out, double lr, double b1, double b2, double eps, double wd, int32_t step,
                                  int32_t zero_grad, slam_stream_t stream) {
  return adamw_range_impl(h, 1, offset, count, master, m_bf16, v_bf16, norm_out, lr, b1, b2, eps, wd, step, zero_grad, stream);
}

int slam_adamw_range_bf16(SlamEngine* h, int64_t offset, int64_t count, void* m_bf16, void* v_bf16, const float* norm_out,
                          double lr, double b1, double b2, double eps, double wd, int32_t step, int32_t zero_grad,
                          slam_stream_t stream) {
  return adamw_range_impl(h, 2, offset, count, nullptr, m_bf16, v_bf16, norm_out, lr, b1, b2, eps, wd, step, zero_grad, stream);
}

int slam_set_decay_mask(SlamEngine* h, const uint8_t* decay, int32_t n_tensors) {
  if (!h) return SLAM_EINVAL;
  std::vector<uint64_t> b;
  if (decay) {
    const size_t nt = h->tensors.size();
    if (n_tensors != (int32_t)nt) return h->fail(SLAM_EINVAL, "decay mask: n_tensors must equal slam_tensor_count");
    for (size_t i = 0; i < nt; ++i) {
      if (decay[i]) continue;
      const uint64_t lo = (uint64_t)h->tensors[i].offset, hi = (uint64_t)(i + 1 < nt ? h->tensors[i + 1].offset : h->n_params);
      if ((lo | hi) & 7) return h->fail(SLAM_EINVAL, "decay mask: tensor bounds must be multiples of 8");
      if (!b.empty() && b.back() == lo) b.back() = hi;  // adjacent no-decay tensors: one range
      else { b.push_back(lo); b.push_back(hi); }
    }
  }
  uint64_t* dev = nullptr;
  if (!b.empty()) {
    std::vector<uint64_t> up(b);
    up.push_back(UINT64_MAX);  // the sentinel that ends a thread's walk
    CK((int)hipMalloc(&dev, up.size() * sizeof(uint64_t)));
    const int r = (int)hipMemcpy(dev, up.data(), up.size() * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (r) { (void)hipFree(dev); CK(r); }
  }
  if (h->nd_dev) CK((int)hipFree(h->nd_dev));  // synchronises with the device: no update in flight still reads the old table
  h->nd_dev = dev;
  h->nd_host.swap(b);
  return SLAM_OK;
}

// ---- Adafactor (the contract is in the header; the kernels in adafactor.hip) ---------------------------------------------
int slam_adafactor_set_segments(SlamEngine* h, const SlamAdafactorSegment* segs, int32_t n) {
  if (!h) return SLAM_EINVAL;
  std::vector<AfSeg> t;
  if (segs || n) {
    if (!segs || n < 1) return h->fail(SLAM_EINVAL, "adafactor segments: a table of n >= 1 segments, or NULL and 0 to clear");
    std::vector<std::pair<int64_t, int64_t>> iv;  // the element intervals the segments cover
    int64_t tiles = 0;
    for (int32_t i = 0; i < n; ++i) {
      const SlamAdafactorSegment& g = segs[i];
      const std::string at = "adafactor segment " + std::to_string(i) + ": ";
      if (g.rows < 1 || g.cols < 1) return h->fail(SLAM_EINVAL, at + "rows and cols must be positive");
      if (g.factored != 0 && g.factored != 1) return h->fail(SLAM_EINVAL, at + "factored is 0 or 1");
      if (!g.factored && g.rows != 1) return h->fail(SLAM_EINVAL, at + "a vector (factored = 0) has rows = 1 and cols = its length");
      if (g.pattern < 0 || g.pattern > 2) return h->fail(SLAM_EINVAL, at + "pattern is 0 (contiguous), 1 or 2 (32 rows of every 64, phase 0 or 32)");
      if (g.pattern && (g.rows % 32)) return h->fail(SLAM_EINVAL, at + "rows in groups of 32 need rows % 32 == 0");
      if ((g.offset & 7) || (g.cols & 7)) return h->fail(SLAM_EINVAL, at + "misaligned: offset and cols must be multiples of 8");
      const int64_t c = g.cols;
      const int64_t span = g.pattern ? ((int64_t)(g.rows / 32 - 1) * 64 + (g.pattern == 2 ? 32 : 0) + 32) * c : (int64_t)g.rows * c;
      if (g.offset < 0 || g.offset > h->n_params || span > h->n_params - g.offset)
        return h->fail(SLAM_EINVAL, at + "out of range: it leaves [0, slam_param_count)");
      if (!g.pattern) {
        iv.push_back({g.offset, g.offset + span});
      } else {
        for (int64_t k = 0; k < g.rows / 32; ++k) {
          const int64_t lo = g.offset + (k * 64 + (g.pattern == 2 ? 32 : 0)) * c;
          iv.push_back({lo, lo + 32 * c});
        }
      }
      AfSeg s;
      s.off = g.offset; s.rows = g.rows; s.cols = g.cols; s.factored = g.factored;
      s.phase = g.pattern == 0 ? -1 : g.pattern == 1 ? 0 : 32;
      tiles += (int64_t)((g.rows + AF_TILE_ROWS - 1) / AF_TILE_ROWS) * ((g.cols + AF_TILE_COLS - 1) / AF_TILE_COLS);
      t.push_back(s);
    }
    if (tiles > 0x7fffffff) return h->fail(SLAM_EINVAL, "adafactor segments: more tiles than one launch holds");
    std::sort(iv.begin(), iv.end());
    for (size_t i = 1; i < iv.size(); ++i)
      if (iv[i].first < iv[i - 1].second) return h->fail(SLAM_EINVAL, "adafactor segments overlap: two segments share an element");
  }
  AfPlan plan;
  AfSeg* dev = nullptr;
  if (!t.empty()) {
    adafactor_layout(t.data(), (int)t.size(), &plan);
    CK((int)hipMalloc(&dev, t.size() * sizeof(AfSeg)));
    const int r = (int)hipMemcpy(dev, t.data(), t.size() * sizeof(AfSeg), hipMemcpyHostToDevice);
    if (r) { (void)hipFree(dev); CK(r); }
    plan.segs = dev;
  }
  if (h->af_plan.segs) CK((int)hipFree((void*)h->af_plan.segs));  // synchronises with the device: no step in flight reads the old table
  h->af_plan = plan;
  h->af_host.swap(t);
  h->af_ws = nullptr;  // sized for the table that went
  return SLAM_OK;
}
int slam_adafactor_sizes(SlamEngine* h, int64_t* state_floats, size_t* workspace_bytes) {
  if (!h || !state_floats || !workspace_bytes) return SLAM_EINVAL;
  if (h->af_host.empty()) return h->fail(SLAM_ESTATE, "adafactor: no segment table (slam_adafactor_set_segments)");
  *state_floats = h->af_plan.state_floats;
  *workspace_bytes = (size_t)h->af_plan.ws_floats * sizeof(float);
  return SLAM_OK;
}
int slam_adafactor_bind_workspace(SlamEngine* h, void* workspace, size_t bytes) {
  if (!h) return SLAM_EINVAL;
  if (!workspace) { h->af_ws = nullptr; return SLAM_OK; }
  if (h->af_host.empty()) return h->fail(SLAM_ESTATE, "adafactor: no segment table (slam_adafactor_set_segments)");
  if (((uintptr_t)workspace) & 15) return h->fail(SLAM_EINVAL, "adafactor workspace must be 16-byte aligned");
  if (bytes < (size_t)h->af_plan.ws_floats * sizeof(float)) return h->fail(SLAM_ENOMEM, "adafactor workspace too small");
  h->af_ws = (float*)workspace;
  return SLAM_OK;
}
int slam_adafactor_step(SlamEngine* h, float* master, float* state, const float* norm_out, double lr, double eps1,
                        double clip_threshold, double decay_rate, double wd, int32_t step, int32_t zero_grad, slam_stream_t stream) {
  if (!h) return SLAM_EINVAL;
  if (h->af_host.empty()) return h->fail(SLAM_ESTATE, "adafactor step without a segment table (slam_adafactor_set_segments)");
  if (h->overlap_adamw) return h->fail(SLAM_ESTATE, "adafactor step with overlap_adamw on: the overlapped chunks belong to AdamW");
  if (!state) return h->fail(SLAM_EINVAL, "adafactor step: state_f32 is NULL");
  if (step < 1) return h->fail(SLAM_EINVAL, "adafactor step: step counts from 1");
  if (!(clip_threshold > 0)) return h->fail(SLAM_EINVAL, "adafactor step: clip_threshold must be positive");
  if (!h->af_ws) return h->fail(SLAM_ESTATE, "adafactor step without a workspace (slam_adafactor_bind_workspace)");
  if (!h->grads || !h->params) return h->fail(SLAM_ESTATE, "bind params first");
  hipStream_t st = (hipStream_t)stream;
  CK(join_optimizer(h, st));
  CK(join_params(h, st));
  h->w8_valid = false;
  AfArgs a;
  a.master = master; a.params = h->params; a.state = state; a.ws = h->af_ws; a.clip = norm_out;
  a.g_bf16 = h->gfinal == 2;  // the last backward kept its final values in bf16 only (slam_set_grad_image's buffer)
  a.g = a.g_bf16 ? (const void*)h->g16 : (const void*)h->grads;
  const double beta = 1.0 - pow((double)step, decay_rate);  // HF: python doubles, fp32 in the kernel
  a.lr = (float)lr; a.eps1 = (float)eps1; a.clip_threshold = (float)clip_threshold; a.wd = (float)wd;
  a.beta = (float)beta; a.one_minus_beta = (float)(1.0 - beta);
  a.step = step;
  a.sr.on = h->adamw_sr; a.sr.seed = h->adamw_sr_seed;
  if (h->nd_dev) { a.nd.bounds = h->nd_dev; a.nd.n = (int)h->nd_host.size(); }
  CK(adafactor_step(h->af_plan, a, st));
  if (zero_grad) CK((int)hipMemsetAsync(h->grads, 0, (size_t)h->n_params * sizeof(float), st));
  return slam_refresh_transposed(h, stream);
}

int slam_add_param_wait(SlamEngine* h, int64_t offset, int64_t count, void* event) {
  if (!h || !event || offset < 0 || count <= 0 || offset + count > h->n_params) return SLAM_EINVAL;
  h->pwaits.push_back({offset, offset + count, (hipEvent_t)event});
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

// fp32 gradient range <-> bf16 communication image (the data-parallel exchange in bf16: the reference's DDP reduces bf16
// gradients because its parameters are bf16, config/model/slam.yaml:9)
int slam_pack_grads_bf16(SlamEngine* h, int64_t offset, int64_t count, void* dst_bf16, slam_stream_t stream) {
  if (!h || !dst_bf16 || offset < 0 || count < 0 || offset + count > h->n_params || (offset & 3) || (count & 3)) return SLAM_EINVAL;
  if (!h->grads) return h->fail(SLAM_ESTATE, "no gradient buffer bound");
  if (count) CK(f32_to_bf16(h->grads + offset, (bf16_t*)dst_bf16, (size_t)count, (hipStream_t)stream));
  return SLAM_OK;
}
int slam_set_grad_image(SlamEngine* h, void* grads_bf16) {
  if (!h) return SLAM_EINVAL;
  h->grad_img = (bf16_t*)grads_bf16;
  return SLAM_OK;
}
int slam_unpack_grads_bf16(SlamEngine* h, int64_t offset, int64_t count, const void* src_bf16, slam_stream_t stream) {
  if (!h || !src_bf16 || offset < 0 || count < 0 || offset + count > h->n_params || (offset & 3) || (count & 3)) return SLAM_EINVAL;
  if (!h->grads) return h->fail(SLAM_ESTATE, "no gradient buffer bound");
  if (count) CK(bf16_to_f32((const bf16_t*)src_bf16, h->grads + offset, (size_t)count, (hipStream_t)stream));
  return SLAM_OK;
}

// ---- engine-side gradient exchange over RCCL (slam_allreduce_grads_async) -----------------------------------
// Replaces, for a consumer WITHOUT torch.distributed, what accelerate's DDP wrapper does for the reference
// (/root/reference config/training_args/default.yaml:18, cli/train.py:51,61: torchrun sets RANK / WORLD_SIZE, the HF Trainer
// wraps the model in DistributedDataParallel). The Python trainer keeps issuing its collectives through torch.distributed
// (slamkit_amd/trainer/dp.py): same RCCL underneath. RCCL is NOT a link-time dependency of the engine: it is looked up at the
// first slam_comm_* call (the copy a host process has already loaded - torch's - is the one dlopen returns).
namespace {
struct Rccl {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*ReduceScatter)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
// resolved ONCE, by whichever thread gets here first (function-local static: C++11 guarantees the others wait - a
// single-process multi-GPU consumer calls slam_comm_init from one thread per rank at the same time, ncclCommInitRank blocks
// until all have joined)
const Rccl* rccl() {
  static const Rccl r = [] {
    Rccl t;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      t.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (t.lib) break;
    }
    if (t.lib) {
      t.GetUniqueId = (decltype(t.GetUniqueId))dlsym(t.lib, "ncclGetUniqueId");
      t.CommInitRank = (decltype(t.CommInitRank))dlsym(t.lib, "ncclCommInitRank");
      t.CommDestroy = (decltype(t.CommDestroy))dlsym(t.lib, "ncclCommDestroy");
      t.AllReduce = (decltype(t.AllReduce))dlsym(t.lib, "ncclAllReduce");
      t.ReduceScatter = (decltype(t.ReduceScatter))dlsym(t.lib, "ncclReduceScatter");
      t.AllGather = (decltype(t.AllGather))dlsym(t.lib, "ncclAllGather");
      t.GetErrorString = (decltype(t.GetErrorString))dlsym(t.lib, "ncclGetErrorString");
      if (!t.GetUniqueId || !t.CommInitRank || !t.CommDestroy || !t.AllReduce || !t.ReduceScatter || !t.AllGather) t.lib = nullptr;
    }
    return t;
  }();
  return r.lib ? &r : nullptr;
}
}  // namespace

int slam_comm_unique_id(void* id_out, int32_t bytes) {
  if (!id_out || bytes < (int32_t)sizeof(ncclUniqueId)) return SLAM_EINVAL;
  const Rccl* r = rccl();
  if (!r) return SLAM_EUNSUPPORTED;
  ncclUniqueId id;
  if (r->GetUniqueId(&id) != ncclSuccess) return SLAM_ESTATE;
  memcpy(id_out, &id, sizeof(id));
  return SLAM_OK;
}

int slam_comm_init(SlamEngine* h, const void* id, int32_t rank, int32_t world) {
  if (!h || !id || world <= 0 || rank < 0 || rank >= world) return SLAM_EINVAL;
  if (h->comm) return h->fail(SLAM_ESTATE, "communicator already initialised");
  const Rccl* r = rccl();
  if (!r) return h->fail(SLAM_EUNSUPPORTED, "librccl.so.1 not found");
  ncclUniqueId uid;
  memcpy(&uid, id, sizeof(uid));
  if (!h->comm_stream) CK((int)hipStreamCreateWithFlags(&h->comm_stream, hipStreamNonBlocking));  // before the communicator: nothing to undo on failure
  ncclComm_t c = nullptr;
  const ncclResult_t e = r->CommInitRank(&c, world, uid, rank);
  if (e != ncclSuccess) return h->fail(SLAM_ESTATE, r->GetErrorString ? r->GetErrorString(e) : "ncclCommInitRank failed");
  h->comm = c;
  h->comm_world = world;
  h->comm_rank = rank;
  return SLAM_OK;
}

int slam_comm_destroy(SlamEngine* h) {
  if (!h) return SLAM_EINVAL;
  if (h->comm) {
    if (h->comm_stream) (void)hipStreamSynchronize(h->comm_stream);
    const Rccl* r = rccl();
    if (r) (void)r->CommDestroy((ncclComm_t)h->comm);
    h->comm = nullptr;
    h->comm_world = 0;
  }
  return SLAM_OK;
}

int slam_allreduce_grads_async(SlamEngine* h, int64_t offset, int64_t count, int32_t bf16_exchange, slam_stream_t ready) {
  if (!h || offset < 0 || count < 0 || offset + count > h->n_params) return SLAM_EINVAL;
  if (!h->comm) return h->fail(SLAM_ESTATE, "slam_comm_init first");
  if (!h->grads) return h->fail(SLAM_ESTATE, "no gradient buffer bound");
  if (bf16_exchange && (!h->last_grad_img || (offset & 3) || (count & 3)))
    return h->fail(SLAM_ESTATE, "bf16 exchange: bind an image with slam_set_grad_image before the backward (ranges in multiples of 4)");
  if (!count) return SLAM_OK;
  const Rccl* r = rccl();
  // communication stream behind the producers of the range
  if (h->comm_ev_used == h->comm_ev.size()) {
    hipEvent_t e;
    CK((int)hipEventCreateWithFlags(&e, sync_event_flags()));  // SLAM_EVENT_SYSTEM_FENCE=1 covers the path whose data leaves the device
    h->comm_ev.push_back(e);
  }
  hipEvent_t ev = h->comm_ev[h->comm_ev_used++];
  CK((int)hipEventRecord(ev, (hipStream_t)ready));
  CK((int)hipStreamWaitEvent(h->comm_stream, ev, 0));
  ncclResult_t e;
  if (bf16_exchange) {
    bf16_t* img = h->last_grad_img + offset;
    e = r->AllReduce(img, img, (size_t)count, ncclBfloat16, ncclSum, (ncclComm_t)h->comm, h->comm_stream);
    if (e == ncclSuccess && h->gfinal != 2) CK(bf16_to_f32(img, h->grads + offset, (size_t)count, h->comm_stream));  // gfinal 2: read where they are
  } else {
    e = r->AllReduce(h->grads + offset, h->grads + offset, (size_t)count, ncclFloat32, ncclSum, (ncclComm_t)h->comm, h->comm_stream);
  }
  if (e != ncclSuccess) return h->fail(SLAM_ESTATE, r->GetErrorString ? r->GetErrorString(e) : "ncclAllReduce failed");
  return SLAM_OK;
}

// ---- the reduce-scatter / all-gather form of the exchange (what the Python trainer runs as ddp_algo = "rs_ag"; SURVEY.md §5
// comm row, §8e: every one of a GPU's 7 xGMI links carries one shard concurrently) for the torch-free consumer -------------------
static int comm_behind(SlamEngine* h, hipStream_t ready) {  // the communication stream continues after everything on `ready`
  if (h->comm_ev_used == h->comm_ev.size()) {
    hipEvent_t e;
    CK((int)hipEventCreateWithFlags(&e, sync_event_flags()));
    h->comm_ev.push_back(e);
  }
  hipEvent_t ev = h->comm_ev[h->comm_ev_used++];
  CK((int)hipEventRecord(ev, ready));
  CK((int)hipStreamWaitEvent(h->comm_stream, ev, 0));
  return SLAM_OK;
}

int slam_reduce_scatter_grads_async(SlamEngine* h, int64_t offset, int64_t count, int32_t bf16_exchange, slam_stream_t ready) {
  if (!h || offset < 0 || count < 0 || offset + count > h->n_params) return SLAM_EINVAL;
  if (!h->comm) return h->fail(SLAM_ESTATE, "slam_comm_init first");
  if (!h->grads) return h->fail(SLAM_ESTATE, "no gradient buffer bound");
  const int64_t w = h->comm_world, s = count / w;
  if (count % w || (s & 7) || (offset & 7)) return h->fail(SLAM_EINVAL, "reduce-scatter: count must be world x a multiple of 8 elements, offset a multiple of 8");
  if (bf16_exchange && !h->last_grad_img) return h->fail(SLAM_ESTATE, "bf16 exchange: bind an image with slam_set_grad_image before the backward");
  if (!count) return SLAM_OK;
  const Rccl* r = rccl();
  if (int rc = comm_behind(h, (hipStream_t)ready)) return rc;
  const int64_t mine = offset + (int64_t)h->comm_rank * s;
  ncclResult_t e;
  if (bf16_exchange) {
    bf16_t* img = h->last_grad_img;
    e = r->ReduceScatter(img + offset, img + mine, (size_t)s, ncclBfloat16, ncclSum, (ncclComm_t)h->comm, h->comm_stream);
    // gradients kept in bf16 only (grad_final_next = 2): the reduced shard is read where it is; else widen it into the fp32 buffer
    if (e == ncclSuccess && h->gfinal != 2) CK(bf16_to_f32(img + mine, h->grads + mine, (size_t)s, h->comm_stream));
  } else {
    e = r->ReduceScatter(h->grads + offset, h->grads + mine, (size_t)s, ncclFloat32, ncclSum, (ncclComm_t)h->comm, h->comm_stream);
  }
  if (e != ncclSuccess) return h->fail(SLAM_ESTATE, r->GetErrorString ? r->GetErrorString(e) : "ncclReduceScatter failed");
  return SLAM_OK;
}

int slam_allgather_params_async(SlamEngine* h, int64_t offset, int64_t count, slam_stream_t ready) {
  if (!h || offset < 0 || count < 0 || offset + count > h->n_params) return SLAM_EINVAL;
  if (!h->comm) return h->fail(SLAM_ESTATE, "slam_comm_init first");
  if (!h->params) return h->fail(SLAM_ESTATE, "bind params first");
  const int64_t w = h->comm_world, s = count / w;
  if (count % w || (s & 7) || (offset & 7)) return h->fail(SLAM_EINVAL, "all-gather: count must be world x a multiple of 8 elements, offset a multiple of 8");
  if (!count) return SLAM_OK;
  const Rccl* r = rccl();
  if (int rc = comm_behind(h, (hipStream_t)ready)) return rc;
  bf16_t* P = h->params;
  const ncclResult_t e = r->AllGather(P + offset + (int64_t)h->comm_rank * s, P + offset, (size_t)s, ncclBfloat16, (ncclComm_t)h->comm, h->comm_stream);
  if (e != ncclSuccess) return h->fail(SLAM_ESTATE, r->GetErrorString ? r->GetErrorString(e) : "ncclAllGather failed");
  // the next reader of the range (slam_forward, layer by layer) waits for the arrival right before its first read
  if (h->ag_ev_used == h->ag_ev.size()) {
    hipEvent_t ev;
    CK((int)hipEventCreateWithFlags(&ev, sync_event_flags()));
    h->ag_ev.push_back(ev);
  }
  hipEvent_t ev = h->ag_ev[h->ag_ev_used++];
  CK((int)hipEventRecord(ev, h->comm_stream));
  h->pwaits.push_back({offset, offset + count, ev});
  h->params_t_dirty = h->params_t != nullptr;
  h->w8_valid = false;
  return SLAM_OK;
}

int slam_comm_finish(SlamEngine* h, slam_stream_t stream) {
  if (!h) return SLAM_EINVAL;
  if (!h->comm_stream || !h->comm_ev_used) return SLAM_OK;
  if (h->comm_ev_used == h->comm_ev.size()) {
    hipEvent_t e;
    CK((int)hipEventCreateWithFlags(&e, sync_event_flags()));  // SLAM_EVENT_SYSTEM_FENCE=1 covers the path whose data leaves the device
    h->comm_ev.push_back(e);
  }
  hipEvent_t ev = h->comm_ev[h->comm_ev_used];
  CK((int)hipEventRecord(ev, h->comm_stream));
  CK((int)hipStreamWaitEvent((hipStream_t)stream, ev, 0));
  h->comm_ev_used = 0;  // the pool is reused by the next step (events are re-recorded; the waits above were already enqueued)
  return SLAM_OK;
}

int slam_param_wait_ms(SlamEngine* h, float* total_ms) {
  if (!h || !total_ms) return SLAM_EINVAL;
  float tot = 0.f;
  for (size_t i = 0; i + 1 < h->pw_used; i += 2) {
    float ms = 0.f;
    if (hipEventSynchronize(h->pw_ev[i + 1]) == hipSuccess && hipEventElapsedTime(&ms, h->pw_ev[i], h->pw_ev[i + 1]) == hipSuccess) tot += ms;
  }
  h->pw_used = 0;
  *total_ms = tot + (float)h->pw_acc_ms;
  h->pw_acc_ms = 0.0;
  return SLAM_OK;
}

int slam_param_wait_untimed(SlamEngine* h, int64_t* n) {
  if (!h || !n) return SLAM_EINVAL;
  *n = h->pw_untimed;
  h->pw_untimed = 0;
  return SLAM_OK;
}

int slam_join(SlamEngine* h, slam_stream_t stream) {
  if (!h) return SLAM_EINVAL;
  CK(join_optimizer(h, (hipStream_t)stream));
  CK(join_params(h, (hipStream_t)stream));
  return SLAM_OK;
}

int slam_zero_grads(SlamEngine* h, slam_stream_t stream) {
  if (!h || !h->grads) return SLAM_EINVAL;
  CK(join_optimizer(h, (hipStream_t)stream));
  CK((int)hipMemsetAsync(h->grads, 0, (size_t)h->n_params * sizeof(float), (hipStream_t)stream));
  return SLAM_OK;
}

int slam_cast_params(SlamEngine* h, const float* master, slam_stream_t stream) {
  if (!h || !master || !h->params) return SLAM_EINVAL;
  CK(join_optimizer(h, (hipStream_t)stream));
  CK(f32_to_bf16(master, h->params, (size_t)h->n_params, (hipStream_t)stream));
  return slam_refresh_transposed(h, stream);
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
namespace {
// slam_op_attn_decode workspace: int64 positions [B], cos / sin / pre-scaled cos / sin tables [B][hd/2], split partials
size_t attn_decode_op_head(int B, int head_dim) { return (((size_t)B * 8 + 255) & ~(size_t)255) + (((size_t)4 * B * (head_dim / 2) * 4 + 255) & ~(size_t)255); }
}  // namespace
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
// the argument ranges of the three q / k norm entry points, checked before anything is launched (the kernels index heads in
// 32 bits: elementwise.hip)
static bool qknorm_dims_ok(int M, int nH, int nKV, int head_dim) {
  if (M <= 0 || nH <= 0 || nKV <= 0 || (head_dim != 64 && head_dim != 128)) return false;
  return (uint64_t)M * (uint64_t)(nH + nKV) * (uint64_t)(head_dim / 8) < (1ull << 31) - 1024;
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

size_t slam_sample_workspace_bytes(int32_t B, int32_t vocab, int32_t top_k) { return sample_workspace_bytes(B, vocab, top_k); }
// slam_sample_tokens and slam_sample_tokens_at: one argument block; the plain call is steps = NULL, group = 1, out_col = step
static int sample_any(const float* logits, int32_t B, int32_t vocab, const uint8_t* banned, const SlamSampleDesc* desc,
                      const int64_t* row_ids, const int32_t* eos_ids, uint8_t* done, int64_t* next, int64_t* out,
                      int64_t out_stride, void* ws, size_t ws_bytes, const uint32_t* steps, int32_t group, int64_t out_col,
                      slam_stream_t stream, const SlamWarpDesc* warp = nullptr) {
  if (!desc || (desc->do_sample != 0 && desc->do_sample != 1) || desc->n_eos > 16) return SLAM_EINVAL;
  SampleArgs a;  // sample_tokens refuses the rest (-1 = SLAM_EINVAL) before it launches anything
  if (warp) {
    a.min_p = warp->min_p;
    a.typical_p = warp->typical_p;
    a.epsilon_cutoff = warp->epsilon_cutoff;
    a.eta_cutoff = warp->eta_cutoff;
  }
  a.logits = logits;
  a.B = B;
  a.vocab = vocab;
  a.banned = banned;
  a.do_sample = desc->do_sample;
  a.top_k = desc->top_k;
  a.temperature = desc->temperature;
  a.top_p = desc->top_p;
  a.seed = desc->seed;
  a.step = desc->step;
  a.pad_id = desc->pad_id;
  a.n_eos = desc->n_eos;
  a.row_ids = row_ids;
  a.eos_ids = eos_ids;
  a.done = done;
  a.next = next;
  a.out = out;
  a.out_stride = out_stride;
  a.steps = steps;
  a.group = group;
  a.out_col = out_col;
  a.ws = ws;
  a.ws_bytes = ws_bytes;
  return sample_tokens(a, (hipStream_t)stream);
}
int slam_sample_tokens(const float* logits, int32_t B, int32_t vocab, const uint8_t* banned, const SlamSampleDesc* desc,
                       const int64_t* row_ids, const int32_t* eos_ids, uint8_t* done, int64_t* next, int64_t* out,
                       int64_t out_stride, void* ws, size_t ws_bytes, slam_stream_t stream) {
  return sample_any(logits, B, vocab, banned, desc, row_ids, eos_ids, done, next, out, out_stride, ws, ws_bytes, nullptr, 1, -1,
                    stream);
}
int slam_sample_tokens_at(const float* logits, int32_t B, int32_t vocab, const uint8_t* banned, const SlamSampleDesc* desc,
                          const int64_t* row_ids, const int32_t* eos_ids, uint8_t* done, int64_t* next, int64_t* out,
                          int64_t out_stride, void* ws, size_t ws_bytes, const uint32_t* steps, int32_t group, int32_t out_col,
                          slam_stream_t stream) {
  if (group < 1 || out_col < 0 || ((uintptr_t)steps & 3)) return SLAM_EINVAL;
  return sample_any(logits, B, vocab, banned, desc, row_ids, eos_ids, done, next, out, out_stride, ws, ws_bytes, steps, group,
                    out_col, stream);
}
int slam_sample_tokens_warped(const float* logits, int32_t B, int32_t vocab, const uint8_t* banned, const SlamSampleDesc* desc,
                              const int64_t* row_ids, const int32_t* eos_ids, uint8_t* done, int64_t* next, int64_t* out,
                              int64_t out_stride, void* ws, size_t ws_bytes, const uint32_t* steps, int32_t group,
                              int32_t out_col, const SlamWarpDesc* warp, slam_stream_t stream) {
  static_assert(sizeof(SlamWarpDesc) == 16 && sizeof(SlamSampleDesc) == 40, "the header's layouts");
  if (group < 1 || out_col < 0 || ((uintptr_t)steps & 3)) return SLAM_EINVAL;
  return sample_any(logits, B, vocab, banned, desc, row_ids, eos_ids, done, next, out, out_stride, ws, ws_bytes, steps, group,
                    out_col, stream, warp);
}

int slam_spec_accept(int64_t* chunk, const int64_t* tgt, int32_t B, int32_t K, int32_t max_new, int32_t pad_id,
                     const int32_t* eos_ids, int32_t n_eos, const int32_t* prompt_len, int32_t* n_new, uint8_t* done,
                     int64_t* out, int64_t out_stride, int32_t* lens_t, int32_t* lens_d, int64_t* draft_ids,
                     int32_t* draft_new_lens, int32_t* tgt_new_lens, int32_t* stats, slam_stream_t stream) {
  static_assert(SPEC_MAX_B == 1024 && SPEC_MAX_K == 15, "the header's limits are the kernel's");
  SpecArgs a;  // spec_accept refuses every bad argument (-1 = SLAM_EINVAL) before it launches anything
  a.chunk = chunk;
  a.tgt = tgt;
  a.B = B;
  a.K = K;
  a.max_new = max_new;
  a.pad_id = pad_id;
  a.n_eos = n_eos;
  a.eos_ids = eos_ids;
  a.prompt_len = prompt_len;
  a.n_new = n_new;
  a.done = done;
  a.out = out;
  a.out_stride = out_stride;
  a.lens_t = lens_t;
  a.lens_d = lens_d;
  a.draft_ids = draft_ids;
  a.draft_new_lens = draft_new_lens;
  a.tgt_new_lens = tgt_new_lens;
  a.stats = stats;
  return spec_accept(a, (hipStream_t)stream);
}

int slam_ngram_propose(int64_t* chunk, int32_t* n_prop, int32_t B, int32_t K, int32_t max_ngram, int32_t fill_id,
                       const int64_t* prompt, int64_t prompt_stride, const int32_t* prompt_len, const int64_t* new_tokens,
                       int64_t new_stride, const int32_t* n_new, const uint8_t* done, const int32_t* eos_ids, int32_t n_eos,
                       int32_t* stats, slam_stream_t stream) {
  static_assert(SLAM_NGRAM_MAX == NGRAM_MAX, "the header's limit is the kernel's");
  NgramArgs a;  // ngram_propose refuses every bad argument (-1 = SLAM_EINVAL) before it launches anything
  a.chunk = chunk;
  a.n_prop = n_prop;
  a.B = B;
  a.K = K;
  a.max_ngram = max_ngram;
  a.fill_id = fill_id;
  a.prompt = prompt;
  a.prompt_stride = prompt_stride;
  a.prompt_len = prompt_len;
  a.fresh = new_tokens;
  a.new_stride = new_stride;
  a.n_new = n_new;
  a.done = done;
  a.eos_ids = eos_ids;
  a.n_eos = n_eos;
  a.stats = stats;
  return ngram_propose(a, (hipStream_t)stream);
}

int slam_constrain_scores(const float* logits, float* scores, int32_t B, int32_t vocab, const SlamConstrainDesc* desc,
                          const int64_t* prompt, const int32_t* prompt_len, const int64_t* new_tokens, int64_t new_stride,
                          const uint8_t* done, const int32_t* eos_ids, const int32_t* begin_ids, const int32_t* seq_tokens,
                          const int32_t* seq_offsets, slam_stream_t stream) {
  if (!desc || (desc->ban_eos != 0 && desc->ban_eos != 1)) return SLAM_EINVAL;
  static_assert(SLAM_CONSTRAIN_MAX_SEQS == CONSTRAIN_MAX_SEQS && SLAM_CONSTRAIN_MAX_SEQ_LEN == CONSTRAIN_MAX_SEQ_LEN &&
                    SLAM_CONSTRAIN_MAX_BEGIN == CONSTRAIN_MAX_BEGIN,
                "the header's caps are the kernels'");
  ConstrainArgs a;  // constrain_scores refuses the rest (-1 = SLAM_EINVAL) before it launches anything
  a.logits = logits;
  a.scores = scores;
  a.B = B;
  a.vocab = vocab;
  a.step = desc->step;
  a.ngram = desc->no_repeat_ngram;
  a.n_per_prompt = desc->n_per_prompt;
  a.prompt_stride = desc->prompt_stride;
  a.ban_eos = desc->ban_eos;
  a.n_eos = desc->n_eos;
  a.n_begin = desc->n_begin;
  a.n_seqs = desc->n_seqs;
  a.n_seq_tokens = desc->n_seq_tokens;
  a.prompt = prompt;
  a.prompt_len = prompt_len;
  a.fresh = new_tokens;
  a.new_stride = new_stride;
  a.done = done;
  a.eos_ids = eos_ids;
  a.begin_ids = begin_ids;
  a.seq_tokens = seq_tokens;
  a.seq_offsets = seq_offsets;
  return constrain_scores(a, (hipStream_t)stream);
}

size_t slam_token_logprobs_workspace_bytes(int32_t B, int32_t vocab) { return token_logprobs_workspace_bytes(B, vocab); }
int slam_token_logprobs(const float* logits, int32_t B, int32_t vocab, const int64_t* tokens, const uint8_t* done,
                        uint8_t* finished, float* out, int64_t out_stride, int32_t column, void* ws, size_t ws_bytes,
                        slam_stream_t stream) {
  // token_logprobs refuses every bad argument (-1 = SLAM_EINVAL) before it launches anything
  return token_logprobs(logits, B, vocab, tokens, done, finished, out, out_stride, column, ws, ws_bytes, (hipStream_t)stream);
}

size_t slam_cfg_workspace_bytes(int32_t B, int32_t vocab) { return cfg_workspace_bytes(B, vocab); }
int slam_cfg_scores(const float* logits, int32_t B, int32_t vocab, float guidance_scale, float* scores, void* ws,
                    size_t ws_bytes, slam_stream_t stream) {
  // cfg_scores refuses every bad argument (-1 = SLAM_EINVAL) before it launches anything
  return cfg_scores(logits, B, vocab, guidance_scale, scores, ws, ws_bytes, (hipStream_t)stream);
}
int slam_cfg_mirror_tokens(int64_t* next, int32_t B, slam_stream_t stream) {
  return cfg_mirror_tokens(next, B, (hipStream_t)stream);
}

}  // extern "C"
