// Internal launcher declarations shared by the engine translation units (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

typedef uint16_t bf16_t;

namespace slam {

// gemm.hip
// Kernel-selection / planning knobs of the GEMM dispatch (DESIGN.md section 4 has the measurement behind each default). One
// instance per engine; an engine entry point makes its instance current for the duration of the call (GemmTuneScope).
struct GemmTune {
  int glds = 1;                 // 1 = LDS-DMA staging where the shape allows, 0 = register staging everywhere (parity tests)
  int tn_dma = 1;
  int group_rows = 3, group_rows_256 = 4;   // row-tile groups of the L2-aware block order (128 / 256-row tiles)
  int nt_store = 0;
  int g256 = 1;                 // 256 x 256 NT kernel: 1 = when its fill criterion holds, 0 = never, 2 = whenever the shape allows
  int g256_dswiglu = 1, g256_persist = 1;
  // late start (10-ns ticks) of the persistent blocks that have a tile of slack (plain / SwiGLU forward; SwiGLU backward):
  // their store bursts fall under the other blocks' K loops. Same box, interleaved: 24.88 / 24.95 ms vs 25.05 / 25.17 / 25.39
  int g256_stagger = 1200, g256_stagger_dswiglu = 1200;
  int group_cols_256 = 0;       // > 0: 256-row tile groups are group_rows_256 x group_cols_256 tiles (0 = all columns of a band)
  int g256_persist_cus = 0;     // > 0: blocks of the persistent 256 x 256 grids (multiple of 8; 0 = one per CU): CUs left to RCCL under data parallelism
  int g256_cohorts = 0;         // > 1: start offsets for every persistent block, cohort c of the XCD's slots c * stagger late (probe)
  int shared = 0;               // the launches of this call share the GPU with the engine's wgrad stream (set inside slam_backward)
  int nt224 = 1, nt224_min_k = 2048;
  int tn_splits_override = 0, tn_balanced = 1, bal_bg_max_split = 4;
  int tn224 = 1, tn224_min_m = 16384, tn224_max_split = 16, tn224_bg_min_m = 4096, tn224_bg_max_split = 1;
  // round 5: main loops on v_mfma_f32_32x32x16_bf16 (1) or on the 16x16x32 form (0) in the kernels that have both
  // (128 x 128 NT DMA kernel, 256 x 256 kernels); the 32x32 form sums a 64-deep K-tile in four steps of 16, the 16x16 form
  // in two of 32: results differ in the last bits between the two settings, not between tile shapes under one setting.
  // Measured and OFF (profiles/r5_power_or_stall.md): the 32x32 form needs 3 % fewer cycles and runs at a 7 % lower clock
  // under the board's power limit; Slam-358M step 330.7 k (8 waves) / 323.4 k (4 waves) vs 338.8 k tokens/s
  int mf32 = 0;
  int g256_w4 = 0;              // 256 x 256 tiles on the persistent four-wave kernel (128 x 128 per wave; needs mf32)
  // round 6: the persistent 256 x 256 kernel with its two wave rows as LOADERS (every LDS-DMA, every counted wait, results handed
  // over through LDS) and STORERS (every output store, no vmcnt wait in the K loop): the store drain of a tile runs under the
  // next tile's K loop instead of in front of it (loads and stores share one in-order vmcnt per wave)
  int g256_roles = 0;
  // round 6: the persistent 256 x 256 SwiGLU-backward epilogue issues the gate|up loads of a 64-row quadrant together and the
  // second quadrant's before the first one's stores (two load round trips per tile instead of eight, none behind a store)
  int g256_batch_loads = 1;
};
GemmTune* gemm_default_tune();
GemmTune* gemm_use_tune(GemmTune* t);  // install t (NULL = process default) for this thread; returns the previous one
int gemm_tune_set(GemmTune* t, const char* key, long value);  // "gemm_*" option keys of slam_set_option; 1 = set, 0 = unknown key, -1 = out of range
struct GemmTuneScope {
  GemmTune* old;
  explicit GemmTuneScope(GemmTune* t) : old(gemm_use_tune(t)) {}
  ~GemmTuneScope() { gemm_use_tune(old); }
};
int gemm_nt(const bf16_t* X, const bf16_t* W, bf16_t* Y, const bf16_t* bias, const bf16_t* resid, int M, int N,
            int K, hipStream_t st);
// same, and additionally act[M][N/2] = silu(gate) * up for W rows laid out in 32-row gate/up blocks
int gemm_nt_swiglu(const bf16_t* X, const bf16_t* W, bf16_t* Y, bf16_t* act, int M, int N, int K, hipStream_t st);
// rotate-half RoPE on the first rope_heads 64-column heads; the first q_heads of them with the (pre-scaled) csq / snq tables
int gemm_nt_rope(const bf16_t* X, const bf16_t* W, bf16_t* Y, const bf16_t* bias, const float* cs, const float* sn,
                 const float* csq, const float* snq, int q_heads, int rope_heads, int M, int N, int K, hipStream_t st);
int gemm_nt_dswiglu(const bf16_t* dY, const bf16_t* Wt, bf16_t* gu, int M, int N, int K, hipStream_t st);
// OPT's ReLU FFN: fc1 act = relu(X W^T + bias) (only the post-ReLU activation is stored); fc2 dgrad with the ReLU backward
// fused into the epilogue: dact = (dY Wt^T) * [act > 0]
int gemm_nt_relu(const bf16_t* X, const bf16_t* W, bf16_t* act, const bf16_t* bias, int M, int N, int K, hipStream_t st);
int gemm_nt_drelu(const bf16_t* dY, const bf16_t* Wt, bf16_t* dact, const bf16_t* act, int M, int N, int K, hipStream_t st);
int gemm_nn(const bf16_t* dY, const bf16_t* W, bf16_t* dX, const bf16_t* resid, int M, int N, int K,
            hipStream_t st);
int gemm_tn_splits(int M, int N, int K);
// How a launch delivers the FINAL values of a gradient tensor - the values the clip and the optimizer consume (round 6).
// The last backward of an optimizer step may keep them in bf16 only, like the reference does (its parameters, hence its
// gradients, are bf16: /root/reference config/model/slam.yaml:9), and emits the sum of squares of what it stored from the
// same registers: no fp32 gradient store, no norm pass over the buffer.
struct GradSink {
  int img_only = 0;        // 1: final values are stored to the bf16 image ONLY (partial sums keep using dW / slabs in fp32)
  float* sumsq = nullptr;  // one partial sum of squares per block, of the final values AS KEPT (the rounded ones when img_only),
                           // added in a fixed order inside the block: block b of the GEMM kernel -> sumsq[b], block c
                           // (y-major) of its reduce kernel -> sumsq[gemm blocks + c]. Blocks without a final store write
                           // nothing: the caller clears the slots first.
  int cap = 0;             // slots behind sumsq; a plan that needs more fails with -3
  int used = 0;            // out: slots this launch owns
};
// upper bound of GradSink::used for dW[N][K] under every plan gemm_tn can choose
size_t gemm_tn_sumsq_slots(int N, int K);
size_t gemm_tn_workspace_bytes(int M, int N, int K);
// background = 1: the launch shares the GPU with other streams (the engine's wgrad side stream): plans for CU-time per
// flop instead of chip fill (no K-splitting on the 256 x 224 kernel)
// ws_bytes: capacity of `ws` (from gemm_tn_workspace_bytes(Mmax, N, K) with Mmax >= M): a plan that does not fit returns -3
// img (nullable): bf16 image of dW with the same indexing - every FINAL value of dW (unsplit tile epilogues, slab reduces) is
// also stored there rounded to nearest even: the communication image of a bf16 gradient exchange, without a conversion pass
int gemm_tn(const bf16_t* dY, const bf16_t* X, float* dW, int accumulate, int M, int N, int K, int ldy, int ldx,
            float* ws, size_t ws_bytes, hipStream_t st, int background = 0, bf16_t* img = nullptr, GradSink* sink = nullptr);

// attention.hip
// launch-shape choices of the backward kernels (engine-owned, "attn_jq" / "attn_kw" / "attn_nch" options):
// jq / kw = 16-row fragments per wave in dQ / dK-dV (1 or 2; head_dim 64 only), nch = query-range chunks per key tile (1..4)
struct AttnTune { int jq, kw, nch, prio; };  // prio: s_setprio by LPT rank (0 = off)
AttnTune attn_default_tune();
void attn_set_default_tune(AttnTune t);
size_t attn_plan_ints(int M);
int attn_plan(const int* seg_start, const int* seg_end, int M, int head_dim, AttnTune tune, int* plan, hipStream_t st);
int attn_fwd(const bf16_t* qkv, bf16_t* o, float* lse2, const int* seg_start, const int* plan, AttnTune tune, int M, int nH,
             int nKV, int head_dim, hipStream_t st);
size_t attn_bwd_workspace_bytes(int M, int nKV, int head_dim);
// rope_cs / rope_sn (nullable): fp32 [M][head_dim/2] tables; when given, dq and dk are written already
// rotated back (transpose rotation), i.e. as gradients of the pre-RoPE projections. plan (required) must come from
// attn_plan with the same tune.
// ndsum, nlse: fp32 [nH * M] scratch each (-rowsum(dO*O) and -lse2, written by the dQ kernel for the dK/dV kernel)
int attn_bwd(const bf16_t* qkv, const bf16_t* o, const bf16_t* d_o, const float* lse2, float* ndsum, float* nlse, bf16_t* dqkv,
             float* dkv_part, const int* seg_start, const int* seg_end, const int* plan, AttnTune tune,
             const float* rope_cs, const float* rope_sn, int M, int nH, int nKV, int head_dim, hipStream_t st);

// elementwise.hip
int rmsnorm_fwd(const bf16_t* x, const bf16_t* w, bf16_t* y, float* rstd, int M, int H, float eps, hipStream_t st);
// LayerNorm (OPT): the compile-time LN variant of the RMSNorm kernels - y = bf16((x - mu) rstd w + b), mu / rstd saved
int layernorm_fwd(const bf16_t* x, const bf16_t* w, const bf16_t* b, bf16_t* y, float* mean, float* rstd, int M, int H, float eps,
                  hipStream_t st);
// dx (+ dres) and per-block partial slabs of dw and db ([rmsnorm_bwd_blocks(M)][H] each; colsum_finish_many finishes them)
int layernorm_bwd(const bf16_t* dy, const bf16_t* x, const bf16_t* w, const float* mean, const float* rstd, const bf16_t* dres,
                  bf16_t* dx, float* dw_part, float* db_part, int M, int H, hipStream_t st);
int rmsnorm_bwd_blocks(int M);
int rmsnorm_bwd(const bf16_t* dy, const bf16_t* x, const bf16_t* w, const float* rstd, const bf16_t* dres,
                bf16_t* dx, float* dw, int accumulate, float* part, int M, int H, hipStream_t st, bf16_t* dw_img = nullptr,
                GradSink* sink = nullptr);
int colsum_blocks(int M);
int colsum_bf16(const bf16_t* X, int ld, int M, int N, float* out, int accumulate, float* part, hipStream_t st);
// csq / snq (nullable): the same tables times qscale - the QUERY heads are rotated with these, so that q is stored
// pre-scaled by head_dim^-0.5 * log2(e) (one rounding): the attention kernels' scores come out in the exp2 domain
int rope_table(const int64_t* pos, int M, int T, int head_dim, float theta, float* cs, float* sn, float* csq, float* snq,
               float qscale, hipStream_t st);
int rope_apply(bf16_t* qkv, int ld, int M, int nrot_heads, int head_dim, const float* cs, const float* sn, int backward,
               hipStream_t st, int q_heads = 0, float q_scale = 1.f);
// Qwen3: RMSNorm over head_dim (64 or 128) of every q and k head of qkv [M][ld] with the weights wq / wk [head_dim], then
// rotate-half RoPE (csq / snq for the nH query heads), fp32 throughout, one rounding at the in-place store; the v columns are
// not touched. raw_save (bf16 [M][(nH + nKV) head_dim]: the input bits) and rstd_save (fp32 [M][nH + nKV]) are nullable.
// -1 = unsupported shape or a null pointer, before any launch (qknorm_bwd and qknorm_rows_f32 alike).
int qknorm_rope_fwd(bf16_t* qkv, int ld, int M, int nH, int nKV, int head_dim, const bf16_t* wq, const bf16_t* wk, const float* cs,
                    const float* sn, const float* csq, const float* snq, float eps, bf16_t* raw_save, float* rstd_save,
                    hipStream_t st);
// in place on the q|k columns of dqkv: dx = rstd (dy w - xhat mean_d(dy w xhat)); part_q / part_k: per-block partial slabs
// [nb][head_dim] of dw_q / dw_k = sum dy xhat (colsum_finish_many finishes them, in block order); nb = the launch's blocks,
// 1 .. qknorm_bwd_blocks(..) (the count the kernel likes best)
int qknorm_bwd_blocks(int M, int nH, int nKV, int head_dim);
int qknorm_bwd(bf16_t* dqkv, int ld, int M, int nH, int nKV, int head_dim, const bf16_t* raw, const float* rstd, const bf16_t* wq,
               const bf16_t* wk, int nb, float* part_q, float* part_k, hipStream_t st);
// decode: the q and k heads of the fp32 projection rows [B][ld] normalised in place (weight applied, no rounding to bf16)
int qknorm_rows_f32(float* qkv, int ld, int B, int nH, int nKV, int head_dim, const bf16_t* wq, const bf16_t* wk, float eps,
                    hipStream_t st);
int swiglu_fwd(const bf16_t* gu, bf16_t* act, int M, int I, int blk, hipStream_t st);
int swiglu_bwd(bf16_t* gu, const bf16_t* dact, int M, int I, int blk, hipStream_t st);
int embed_fwd(const int64_t* ids, const bf16_t* E, bf16_t* out, int M, int H, int V, hipStream_t st);
// OPT embedding: out = bf16(E[ids] + P[pos + 2]), pos = position_ids or m % T (indices clamped to the tables); the position
// row of every token goes to prow (int64 [M], nullable) for the backward's scatter
int embed_pos_fwd(const int64_t* ids, const int64_t* pos, const bf16_t* E, const bf16_t* P, bf16_t* out, int64_t* prow, int M, int H,
                  int V, int T, int NP, hipStream_t st);
// NEFTune (include/slam_engine.h, slam_set_neftune): the gather above with noise, out = bf16(E[ids] (+ P[pos + 2]) + n), n =
// (2 r16 - 65535) * s with the 16 random bits of (seed, call, site 0x4E454654, index0 + m H + h). P == nullptr: no position
// table (pos, prow, T and NP are not read). H and index0 multiples of 8, s finite and >= 0.
struct NeftSite { float s = 0.f; uint64_t seed = 0; uint32_t call = 0; int64_t index0 = 0; };
int embed_noise_fwd(const int64_t* ids, const int64_t* pos, const bf16_t* E, const bf16_t* P, bf16_t* out, int64_t* prow, int M, int H,
                    int V, int T, int NP, const NeftSite& n, hipStream_t st);
// d *= [act > 0] (n a multiple of 8): the ReLU backward without the fused fc2 dgrad epilogue
int relu_bwd(bf16_t* d, const bf16_t* act, size_t n, hipStream_t st);
// Residual dropout (OPT): the mask of element (m, n) of a site is a function of (seed, call, site, index0 + m H + n) alone
// (include/slam_engine.h, "dropout_thr16"); thr16 = round(p * 65536), an element is dropped iff its 16 random bits are below it.
// H and index0 multiples of 8.
struct DropSite { int thr16 = 0; uint64_t seed = 0; uint32_t call = 0, site = 0; int64_t index0 = 0; };
// in place: y = bf16(resid + (keep ? y / (1 - q) : 0))
int dropout_add(bf16_t* y, const bf16_t* resid, int M, int H, const DropSite& d, hipStream_t st);
// dm = keep ? bf16(dy / (1 - q)) : 0; dy is left alone
int dropout_bwd(const bf16_t* dy, bf16_t* dm, int M, int H, const DropSite& d, hipStream_t st);
int onehot(const int64_t* ids, bf16_t* oh, int M, int Vp, int V, int pad_id, hipStream_t st);
// gather-side embedding gradient for large vocabularies: dE[ids[m]] += dh[m] in token order (deterministic);
// ws = embed_bwd_workspace_ints(M, Vp) ints
size_t embed_bwd_workspace_ints(int M, int Vp);
int embed_bwd(const int64_t* ids, const bf16_t* dh, float* dE, int M, int H, int Vp, int V, int pad_id, int* ws,
              hipStream_t st);
// eps = label smoothing in [0, 1) (HF LabelSmoother over the V real columns): 0 launches the plain kernels and never touches
// row_smooth; > 0 needs row_smooth (M floats: lse - mean_v z_v per valid row, 0 on ignored rows) and no colmask, else -1.
// row_loss is the plain nll either way; loss = ((1 - eps) sum row_loss + eps sum row_smooth) / denom.
int cross_entropy(const bf16_t* logits, const int64_t* labels, double num_items, bf16_t* dlogits, float* row_loss,
                  float* denom, float* loss, int B, int T, int Vp, int V, const uint8_t* colmask, float eps, float* row_smooth,
                  hipStream_t st);
int seq_loglik(const float* row_loss, const int64_t* labels, int B, int T, float* ll, float* cnt, hipStream_t st);
int copy_cols(const bf16_t* src, int lds_, bf16_t* dst, int ldd, int M, int ncols, hipStream_t st);
int scale_bf16(bf16_t* x, size_t n, float s, hipStream_t st);
int scale_rows_bf16(bf16_t* x, const float* coef, int M, int T, int ncols, hipStream_t st);
// Padding-free execution of padded [B][T] batches (include/slam_engine.h, slam_forward_unpadded / _spans): the packed arrays of
// one batch in caller-owned scratch, every array 256-byte aligned. Mmax = B * T rounded up to 64.
struct UnpadView {
  int64_t *ids, *labels, *pos;  // [Mmax]
  int32_t *seg_s, *seg_e, *row;  // [Mmax]; row = the token's batch row, -1 in the tail
  int32_t* off;                  // [B + 1] exclusive prefix sum of lens
};
size_t unpad_scratch_bytes(int B, int T);
UnpadView unpad_view(void* scratch, int B, int T);
// one launch: the pack rule over m' in [0, Mp); labels nullable (v.labels is then left alone); starts nullable (int32 [B], the
// first real column of each row; nullptr = 0, right padding)
int unpad_pack(const int64_t* ids, const int64_t* labels, const int32_t* starts, const int32_t* lens, int B, int T, int Mp,
               int pad_id, const UnpadView& v, hipStream_t st);
// dst[b][starts[b] + t][0 .. V) = src[off[b] + t][0 .. V) for t < lens[b], 0 elsewhere   (src: Mp rows, Vp long; starts nullable)
int unpad_logits(const bf16_t* src, int Vp, bf16_t* dst, int V, const int32_t* off, const int32_t* starts, int B, int T, int Mp,
                 hipStream_t st);
// per-row sums of -row_loss over valid targets and their counts, over the packed segments (seq_loglik's reduction)
int seq_loglik_unpadded(const float* row_loss, const int64_t* labels_packed, const int32_t* off, int B, int Mp, float* ll,
                        float* cnt, hipStream_t st);
// x[m'][:] *= row[m'] >= 0 ? coef[row[m']] : 0
int scale_rows_unpadded_bf16(bf16_t* x, const float* coef, const int32_t* row, int Mp, int ncols, hipStream_t st);
int grad_chunk_elems();
int grad_sumsq_chunks(const void* g, int g_bf16, size_t n, size_t off, size_t cnt, float* chunk_sums, hipStream_t st);
int grad_norm_from_chunks(const float* chunk_sums, size_t n_chunks, float max_norm, float* out, hipStream_t st);
// Stochastic rounding of the bf16 state stores ("adamw_sr"): the random bits of an element are a function of (seed, step, its
// index in the engine's flat parameter buffer, which array) alone; base = that index for element 0 of the arrays handed over.
// Rounded: m and v wherever they are bf16, p where the bf16 parameters are the state (mode 2). fp32 state (mode 0) ignores it.
struct AdamSR { int on = 0; uint64_t seed = 0; int64_t base = 0; };
// The no-decay set (slam_set_decay_mask): half-open ranges of the flat parameter buffer that take weight_decay = 0. bounds
// (device memory) = lo0, hi0, lo1, hi1, .. - n strictly increasing flat indices, every one a multiple of 8, closed by one
// sentinel bounds[n] = UINT64_MAX: an element lies in a range iff an odd number of bounds is <= its index, and the 4 or 8
// consecutive elements of a kernel thread lie in one range or in none. base = the flat index of element 0 of the arrays handed
// over. bounds == nullptr: wd applies to every element, through the kernels that know nothing of the table.
struct AdamNoDecay { const uint64_t* bounds = nullptr; int n = 0; int64_t base = 0; };
// One AdamW update, from the engine's entry points down to the kernel launch: every pointer is at the same element.
struct AdamArgs {
  int mode = 0;                // 0 = fp32 master + fp32 moments, 1 = fp32 master + bf16 moments, 2 = bf16 parameters + bf16 moments
  float* master = nullptr;     // nullable (mode 2: the bf16 parameters are the state, updated in place)
  bf16_t* params = nullptr;    // the bf16 working copy
  bf16_t* params_t = nullptr;  // nullable: the transposed weight images (adamw_tiles)
  void* g = nullptr;           // gradients: float, or bf16_t when g_bf16 (the last backward kept its final values in bf16 only)
  int g_bf16 = 0;
  void* m = nullptr;           // moments: float in mode 0, else bf16_t
  void* v = nullptr;
  const float* clip = nullptr;  // nullable: slam_grad_norm's output (the gradients are scaled by clip[1])
  double lr = 0, b1 = 0, b2 = 0, eps = 0, wd = 0;
  int step = 1, zero_grad = 0;
  AdamSR sr;
  AdamNoDecay nd;  // honoured by adamw_flat and adamw_strided; adamw_tiles takes one wd for the launch (the caller decides per matrix)
  // the same update `off` elements further on
  AdamArgs at(int64_t off) const {
    AdamArgs a = *this;
    const int64_t gsz = g_bf16 ? 2 : 4, esz = mode == 0 ? 4 : 2;
    if (master) a.master = master + off;
    if (params) a.params = params + off;
    if (params_t) a.params_t = params_t + off;
    if (g) a.g = (char*)g + off * gsz;
    if (m) a.m = (char*)m + off * esz;
    if (v) a.v = (char*)v + off * esz;
    a.sr.base = sr.base + off;
    a.nd.base = nd.base + off;
    return a;
  }
};
// n consecutive elements. Mode 2 goes 8 elements per thread (n and, when rounding stochastically, sr.base multiples of 8),
// modes 0 and 1 four (multiples of 4); with a no-decay table nd.base is a multiple of 8 / 4 as well
int adamw_flat(const AdamArgs& a, size_t n, hipStream_t st);
// `batch` vectors of n elements at a constant stride
int adamw_strided(const AdamArgs& a, size_t n, int batch, size_t stride, hipStream_t st);
// `batch` same-shaped [R][C] matrices (64-multiples) at a constant stride, ALSO writing the transposed bf16 image params_t[C][R]
int adamw_tiles(const AdamArgs& a, int R, int C, int batch, size_t batch_stride, hipStream_t st);
// y[i] = the stochastic rounding of x[i] as the kernels above apply it to flat index index0 + i of array `which` (0 p, 1 m, 2 v)
int sr_round_bf16(const float* x, bf16_t* y, size_t n, int64_t index0, uint64_t seed, int step, int which, hipStream_t st);
// ---- Adafactor (adafactor.hip; the contract is in include/slam_engine.h: slam_adafactor_step) ---------------------------------
// One HF parameter laid over the flat buffer, as the kernels read it. HF row r is row r of the engine tensor at `off`
// (phase < 0) or row (r / 32) * 64 + phase + r % 32 of it (gate / up: groups of 32 rows every 64). A vector is rows = 1,
// cols = numel. A factored segment owns rows + cols state floats (the row factors, then the column factors), a vector numel.
constexpr int AF_TILE_ROWS = 256, AF_TILE_COLS = 256;  // a block's tile; tiles of a segment are numbered row block major
struct AfSeg {
  int64_t off = 0, state = 0;          // first element in the flat buffer / first float in the state buffer
  int64_t rowpart = 0, colpart = 0;    // workspace floats: row partials [rows][n_cb], column partials [n_rb][cols]
  int rows = 0, cols = 0, factored = 0, phase = -1;
  int tile0 = 0, n_rb = 0, n_cb = 0;   // first tile; row blocks and column blocks
  int fin0 = 0;                        // first block of the factor finish (256 factors a block; none for a vector)
};
struct AfPlan {
  const AfSeg* segs = nullptr;  // device
  int n_segs = 0, n_tiles = 0, n_fin = 0;
  int64_t state_floats = 0;
  int64_t segmean = 0, segd = 0, tilepart = 0, ws_floats = 0;  // workspace floats: [n_segs], [n_segs], [n_tiles]; the total
};
struct AfArgs {
  float* master = nullptr;     // nullable: the bf16 parameters are the only copy
  bf16_t* params = nullptr;
  const void* g = nullptr;     // float, or bf16_t when g_bf16
  int g_bf16 = 0;
  float* state = nullptr;
  float* ws = nullptr;
  const float* clip = nullptr;  // nullable: slam_grad_norm's output
  float lr = 0, eps1 = 0, clip_threshold = 1, beta = 0, one_minus_beta = 1, wd = 0;
  int step = 1;
  AdamSR sr;       // rounds the bf16 parameters where they are the only copy; base is not used (a tile knows its flat index)
  AdamNoDecay nd;  // a segment whose first element lies in a range takes wd = 0
};
// host: lays the segments (off, rows, cols, factored, phase given) out over state and workspace; fills the rest and `plan`
void adafactor_layout(AfSeg* segs, int n, AfPlan* plan);
int adafactor_step(const AfPlan& plan, const AfArgs& a, hipStream_t st);
// ---- Muon (muon.hip; the contract is in include/slam_engine.h: slam_muon_step) ------------------------------------------------
// One Muon matrix: an HF [rows][cols] weight over the flat buffer (row pattern as AfSeg), its rows * cols momentum floats (HF
// row-major, segments in TABLE order) and its packed bf16 image [n][m], n = min(rows, cols), m = max(rows, cols): the matrix
// itself, or its transpose when rows > cols. The kernels' table is sorted by shape class (stable), so the packed images and the
// sum-of-squares partials of one class lie behind each other at the constant strides n * m and `parts`.
constexpr int MU_TILE = 64;  // prepare / apply: a block owns 64 rows x 64 columns of the HF matrix; tiles numbered row block major
struct MuSeg {
  int64_t off = 0, mom = 0, pack = 0;  // first element: flat buffer / momentum buffer / packed buffer
  int rows = 0, cols = 0, phase = -1;
  int tile0 = 0, n_tc = 0;             // first tile (= first partial); column tiles
};
struct MuClass {
  int rows = 0, cols = 0, n = 0, m = 0, count = 0;
  int64_t pack = 0;         // first packed element of the class
  int part0 = 0, parts = 0; // first partial of the class; partials (tiles) of one matrix
};
constexpr int MU_MAX_CLASSES = 64;
struct MuPlan {
  const MuSeg* segs = nullptr;  // device, class order
  int n_segs = 0, n_tiles = 0, n_classes = 0;
  MuClass cls[MU_MAX_CLASSES];
  int64_t elems = 0;            // Muon elements = momentum floats = packed elements
  // workspace bytes (each region 256-byte aligned): packed X [elems] | Y [max count n m] | A, P [max count n n] | partials [n_tiles]
  size_t x_off = 0, y_off = 0, a_off = 0, p_off = 0, part_off = 0, ws_bytes = 0;
};
struct MuArgs {
  float* master = nullptr;   // nullable: the bf16 parameters are the only copy
  bf16_t* params = nullptr;
  const void* g = nullptr;   // float, or bf16_t when g_bf16
  int g_bf16 = 0;
  float* gzero = nullptr;    // nullable: the fp32 gradient buffer, whose Muon elements the prepare launch clears
  float* mom = nullptr;
  char* ws = nullptr;
  const float* clip = nullptr;
  double lr = 0, wd = 0;
  float mu = 0.95f, omm = 0.05f;
  int nesterov = 1, ns_steps = 5, adjust_lr = 2, step = 1;
  float a = 3.4445f, b = -4.7750f, c = 2.0315f, eps = 1e-7f;
  AdamSR sr;
  AdamNoDecay nd;
};
// host: segs (off, rows, cols, phase given, table order) -> mom offsets, class order, tiles, packed offsets; fills `plan` but segs
// (the caller uploads the sorted table). -1: more than MU_MAX_CLASSES shape classes or more tiles than a launch holds.
int muon_layout(MuSeg* segs, int n, MuPlan* plan);
int muon_prepare(const MuPlan& plan, const MuArgs& a, hipStream_t st);
int muon_apply(const MuPlan& plan, const MuArgs& a, const bf16_t* o_packed, hipStream_t st);
int muon_step(const MuPlan& plan, const MuArgs& a, hipStream_t st);
// C[i] = beta R[i] + alpha X[i] X[i]^T ([n][n] from [n][m]; lower-triangle tiles, mirrored) and Y[i] = beta R[i] + alpha P[i] X[i]
// ([n][n] x [n][m]); n, m and the strides (elements) multiples of 8; R nullable (then beta is not read)
int muon_syrk(const bf16_t* X, const bf16_t* R, bf16_t* C, int batch, int n, int m, int64_t sx, int64_t sr, int64_t sc, float alpha,
              float beta, hipStream_t st);
int muon_mm(const bf16_t* P, const bf16_t* X, const bf16_t* R, bf16_t* Y, int batch, int n, int m, int64_t sp, int64_t sx, int64_t sr,
            int64_t sy, float alpha, float beta, hipStream_t st);
// Newton-Schulz on `batch` packed [n][m] matrices (n <= m) at stride sx, in place. part: `parts` partial sums of squares per
// matrix at stride parts, or nullptr: computed here into the scratch (muon_ns_partials per matrix). Y [batch n m], A, P [batch n n].
constexpr int MU_NORM_CHUNK = 8192;
inline int muon_ns_partials(int n, int m) { return (int)(((int64_t)n * m + MU_NORM_CHUNK - 1) / MU_NORM_CHUNK); }
size_t muon_ns_workspace_bytes(int batch, int n, int m);
int muon_ns(bf16_t* X, int batch, int n, int m, int64_t sx, const float* part, int parts, int ns_steps, float a, float b, float c,
            float eps, bf16_t* Y, bf16_t* A, bf16_t* P, float* part_scratch, hipStream_t st);
int f32_to_bf16(const float* s, bf16_t* d, size_t n, hipStream_t st);
// the same conversion, emitting one GradSink partial (sum of squares of the rounded values) per 8192-element block
int f32_to_bf16_sumsq_slots(size_t n);
int f32_to_bf16_sumsq(const float* s, bf16_t* d, size_t n, float* sumsq, hipStream_t st);
int bf16_to_f32(const bf16_t* s, float* d, size_t n, hipStream_t st);
int transpose_bf16(const bf16_t* src, bf16_t* dst, int R, int C, int batch, size_t batch_stride, hipStream_t st);
int colsum_finish_many(const float* part, size_t part_stride, int nb, int N, float* out, size_t out_stride, int count,
                       int accumulate, hipStream_t st, bf16_t* img = nullptr,  // img: bf16 image of `out` (same indexing), nullable
                       GradSink* sink = nullptr);


// decode.hip (KV-cached generation)
// Y[M][N] = X[M][K] W[N][K]^T (+ bias[N]) (+ resid[M][N]) for small M: a weight stream on v_mfma_f32_16x16x32_bf16 with split-K.
// Exactly one of Y (bf16) / Yf (fp32) is non-null. ws: fp32 split-K partials (gemm_skinny_workspace_bytes for the full
// split; less or none gives fewer splits). Deterministic: partials are summed in split order by a second launch.
constexpr int SKINNY_MAX_M = 64;  // the engine's decode projections use gemm_skinny up to this many rows, gemm_nt beyond
size_t gemm_skinny_workspace_bytes(int M, int N, int K);
int gemm_skinny(const bf16_t* X, const bf16_t* W, bf16_t* Y, float* Yf, const bf16_t* bias, const bf16_t* resid, int M, int N,
                int K, float* ws, size_t ws_bytes, hipStream_t st);
// FP8 weight stream (quant.hip, decode.hip): W[N][K] as e4m3fn codes Q[N][K] + per-row int8 exponents E[N], Wdq = value(Q) 2^E.
// K must be a multiple of W8_K_GRAIN: the codes of a row keep their 64-deep K block but not their order inside it - byte
// w8_code_pos(k) of the row holds the code of column k, so that the 16 bytes at 64 b + 16 q are, for MFMA lane quarter q, the 8
// codes of columns 64 b + 8 q .. + 7 followed by those of columns 64 b + 32 + 8 q .. + 7 (two consecutive 32-deep steps).
constexpr int W8_K_GRAIN = 64;
constexpr int W8_EXP_MIN = -100, W8_EXP_MAX = 120;
__host__ __device__ inline int w8_code_pos(int k) { return (k & ~63) | (((k >> 3) & 3) << 4) | (((k >> 5) & 1) << 3) | (k & 7); }
inline size_t w8_align(size_t b) { return (b + 255) & ~(size_t)255; }
inline size_t w8_exps_offset(int N, int K) { return w8_align((size_t)N * K); }        // codes first, exponents 256-byte aligned
inline size_t w8_bytes(int N, int K) { return w8_exps_offset(N, K) + w8_align((size_t)N); }
// quantize: Q, E from W, and W rewritten in place with Wdq. dequantize: W[N][K] row-major from Q, E. -1: bad argument.
int quantize_rows_fp8(bf16_t* W, uint8_t* Q, int8_t* E, int N, int K, hipStream_t st);
int dequantize_rows_fp8(const uint8_t* Q, const int8_t* E, bf16_t* W, int N, int K, hipStream_t st);
// gemm_skinny with the W operand read as codes: the MFMA sees exactly the bf16 values of Wdq in the lanes and the K order of
// gemm_skinny(X, Wdq, ..), under the same split plan and reduce launch - the same bits.
int gemm_skinny_w8(const bf16_t* X, const uint8_t* Q, const int8_t* E, bf16_t* Y, float* Yf, const bf16_t* bias,
                   const bf16_t* resid, int M, int N, int K, float* ws, size_t ws_bytes, hipStream_t st);
// one decode step of attention for one layer: qkv = fp32 [B][(nH + 2 nKV) hd] projection WITHOUT bias; bias + RoPE (tables
// cs / sn and the pre-scaled csq / snq of rope_table at the rows' positions lens[b]) are applied in fp32 and rounded once;
// the new K / V go to row lens[b] of kc / vc ([B][nKV][cap][hd] bf16), and o[b] (bf16 [B][nH hd]) attends over rows
// 0 .. lens[b]. kv_bound >= max(lens) + 1 (host bound, <= cap). part: fp32 split partials (attn_decode_part_bytes).
size_t attn_decode_part_bytes(int B, int nH, int head_dim, int ns);
int attn_decode_chunk(int B, int nH, int nKV, int head_dim, int kv_bound, size_t part_bytes);
int attn_decode(const float* qkv, const bf16_t* bias, const float* cs, const float* sn, const float* csq, const float* snq,
                const int* lens, bf16_t* kc, bf16_t* vc, int cap, int B, int nH, int nKV, int head_dim, int kv_bound, bf16_t* o,
                float* part, size_t part_bytes, hipStream_t st);
// prefill: K / V columns of rows t < lens[b] of one layer's qkv [B*T][QKV] into the cache
int kv_scatter(const bf16_t* qkv, bf16_t* kc, bf16_t* vc, const int* lens, int B, int T, int nH, int nKV, int head_dim, int cap,
               hipStream_t st);
int gather_last_rows(const bf16_t* src, bf16_t* dst, const int* lens, int B, int T, int H, hipStream_t st);
int lens_to_pos(const int* lens, int64_t* pos, int B, hipStream_t st);
int lens_inc(int* lens, int B, hipStream_t st);
// chunk attention over the cache (slam_extend): qkv = bf16 [B T][(nH + 2 nKV) hd] as the forward holds it (bias and RoPE
// applied, q pre-scaled). Token t < new_lens[b] of row b: its K / V go to cache row base_lens[b] + t (a launch of its own,
// first), and o[b T + t] (bf16 [B T][nH hd]) attends over cache rows 0 .. base_lens[b] + t on v_mfma_f32_16x16x32_bf16; rows
// t >= new_lens[b] of o are zeros. base_lens[b] + new_lens[b] <= kv_bound <= cap (host bound; the kernels clamp to it).
// part: fp32 split partials (attn_extend_part_bytes), merged in split order; none (or too little) means fewer or one split.
size_t attn_extend_part_bytes(int B, int T, int nH, int head_dim, int ns);
int attn_extend_chunk(int B, int T, int nH, int nKV, int head_dim, int kv_bound, size_t part_bytes);
int attn_extend(const bf16_t* qkv, const int* base_lens, const int* new_lens, bf16_t* kc, bf16_t* vc, int cap, int B, int T,
                int nH, int nKV, int head_dim, int kv_bound, bf16_t* o, float* part, size_t part_bytes, hipStream_t st);
// pos[b T + t] = lens[b] + t
int extend_positions(const int* lens, int64_t* pos, int B, int T, hipStream_t st);
// dst[b] = src[b] (fp32 [B][vocab]) and lens[b] += new_lens[b] for the rows with new_lens[b] > 0; the others keep their bits
int extend_finish(const float* src, float* dst, const int* new_lens, int* lens, int B, int T, int vocab, hipStream_t st);
// slam_extend_logits: rows [m0, m0 + rows) of the chunk's fp32 logits (src row 0 = chunk row m0) into dst [B T][vocab], only
// where t < new_lens[b]; and lens[b] += clamp(new_lens[b], 0, T)
int extend_store_rows(const float* src, float* dst, const int* new_lens, int m0, int rows, int B, int T, int vocab,
                      hipStream_t st);
int lens_add(int* lens, const int* new_lens, int B, int T, hipStream_t st);
// n samples per prompt: rows 0 .. B-1 of the cache kv (L x { K, V } x [bmax][nKV][cap][head_dim]), of lens and of the nullable
// logits [.][vocab] fan out in place to rows b n .. b n + n - 1; only lens[b] keys of a row are copied. One launch per source
// row in descending b (hazard-free for every (B, n): decode.hip's header). kv_bound: host bound of lens.
int kv_repeat(bf16_t* kv, int* lens, float* logits, int B, int n, int bmax, int L, int nKV, int head_dim, int cap, int kv_bound,
              int vocab, hipStream_t st);
// LM head fused with the row statistics (include/slam_engine.h: slam_op_score_rows): for row m of X (bf16 [M][K]) against the
// head W (bf16 [V][K]) on v_mfma_f32_16x16x32_bf16, lp = log-softmax at targets[m] and argmax = the lowest id of the largest
// score, from fp32 accumulators that are never stored. colmask: nullable, >= V bytes, non-zero = the column counts as -inf.
// new_lens == nullptr: lp [M], argmax [M] (nullable). new_lens given (slam_extend_score, M = B T): lp[b][t + 1] and
// argmax[b][t] by that call's layout. ws: score_rows_workspace_bytes(M, V), 16-byte aligned: chunk partials and target scores.
constexpr int SCORE_MAX_M = 0x7fffffc0 / 64;
constexpr int SCORE_MAX_V = 65535 * 512;  // one grid row of blocks per chunk
size_t score_rows_workspace_bytes(int M, int V);       // host only
int score_rows(const bf16_t* X, const bf16_t* W, const int64_t* targets, const uint8_t* colmask, int M, int V, int K,
               const int* new_lens, int T, float* lp, int64_t* argmax, void* ws, size_t ws_bytes, hipStream_t st);
// tg[b T + t] = ids[b][t + 1] when t + 1 < new_lens[b], -100 else
int extend_targets(const int64_t* ids, const int* new_lens, int64_t* tg, int B, int T, hipStream_t st);

}  // namespace slam
