/*
 * slam_engine.h - C ABI of libslam_engine.so, the gfx950 (MI355X) engine behind slamkit's
 * cli/train.py hot path.
 *
 * The reference has no FFI on this path: the boundary is the Python plugin surface
 *   tlm_factory(cfg.model) -> TokenLM            /root/reference slamkit/model/token_lm.py:30-43
 *   UnitLM.forward(input_ids, attention_mask, position_ids, labels, num_items_in_batch)
 *                                                 slamkit/model/unit_lm.py:135-182
 *   compute_loss(logits, labels, num_items_in_batch)   slamkit/model/unit_lm.py:13-29
 *   UnitLM.log_likelihood                          slamkit/model/unit_lm.py:184-194
 *   SLAMTrainer.training_step + HF Trainer step    slamkit/trainer/slam_trainer.py:59-71
 * Each entry point below names the reference call it replaces. All device pointers are BORROWED
 * (PyTorch-ROCm tensor.data_ptr()); the engine never frees them and never synchronises the host:
 * every call only enqueues work on the hipStream_t it is given. Return value 0 = ok, negative =
 * SLAM_E*, positive = hipError_t; slam_last_error() gives text. No exceptions cross the ABI.
 * One engine per process/GPU; calls on one engine must be serialised by the caller.
 */
#ifndef SLAM_ENGINE_H
#define SLAM_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLAM_OK 0
#define SLAM_EINVAL (-1)      /* bad argument / unsupported shape */
#define SLAM_ESTATE (-2)      /* call order (e.g. backward without forward, unbound buffers) */
#define SLAM_ENOMEM (-3)      /* bound workspace too small */
#define SLAM_EUNSUPPORTED (-4) /* an optional run-time dependency is missing (slam_comm_*: librccl) */

typedef struct SlamEngine SlamEngine;
typedef void* slam_stream_t; /* hipStream_t */

/* Qwen2- / Qwen3-shaped decoder description (UnitLMConfig.base_config, unit_lm.py:32-79; Slam-358M values
 * from config/model/slam.yaml + Qwen2.5-0.5B). */
typedef struct SlamModelDesc {
  int32_t n_layers;      /* 24  */
  int32_t hidden;        /* 896 */
  int32_t n_heads;       /* 14  */
  int32_t n_kv_heads;    /* 2   */
  int32_t head_dim;      /* 64 or 128 */
  int32_t intermediate;  /* 4864 */
  int32_t vocab;         /* 502; embedding rows are padded to 512, or to a multiple of 256 beyond 512 */
  int32_t pad_token_id;  /* 0: nn.Embedding(padding_idx) gather-gradient suppression; -1 = none */
  float rms_eps;         /* 1e-6 */
  float rope_theta;      /* 10000 */
} SlamModelDesc;

typedef struct SlamTensorInfo {
  char name[64];      /* "embed", "layers.3.wqkv", "layers.3.bqkv", "layers.3.wo", "layers.3.ln1",
                         "layers.3.ln2", "layers.3.wgu", "layers.3.wd", "norm" (Qwen3: "layers.3.q_norm", "layers.3.k_norm").
                         wqkv rows = q | k | v; wgu rows = blocks of 32 gate_proj rows followed by the
                         matching 32 up_proj rows (row 64b+j = gate[32b+j], row 64b+32+j = up[32b+j]) */
  int64_t offset;     /* element offset in the flat parameter / gradient buffers */
  int64_t rows, cols; /* row-major [rows][cols] (cols = 1 for vectors) */
} SlamTensorInfo;

/* Called from slam_backward (host side, after the producing kernels were enqueued) when the
 * gradient range [offset, offset+count) of the flat fp32 gradient buffer is final. Used by the
 * data-parallel reducer to launch RCCL all-reduces overlapped with the rest of backward
 * (replaces torch DDP's reducer hooks). */
typedef void (*slam_bucket_cb)(void* user, int64_t offset, int64_t count);

/* ---- lifetime -------------------------------------------------------------------------------*/
int slam_engine_create(const SlamModelDesc* desc, SlamEngine** out); /* UnitLM.__init__ :91-112 */
/* The same for a decoder family: arch 0 = Qwen2 (= slam_engine_create, n_positions ignored), arch 1 = pre-LN OPT as HF
 * OPTForCausalLM computes it (facebook/opt-125m, the reference's config/model/default.yaml body; the TWIST-1.3B body):
 * LayerNorm with bias, learned absolute positions (n_positions + 2 rows: HF's offset of 2), ReLU FFN with biases, biases on
 * out_proj / fc2, no RoPE, tied head. Requires n_kv_heads == n_heads and head_dim 64; rms_eps carries the LayerNorm eps,
 * rope_theta is ignored; `intermediate` is OPT's ffn_dim. OPT tensor names, in layout order (every offset a multiple of 8,
 * both embedding tables before layer 0, each layer contiguous from its ln1 at a constant stride, the final norm last):
 *   embed [Vp][H], pos_embed [n_positions + 2][H],
 *   layers.N.{ln1, ln1_b [H], wqkv [3 H][H], bqkv [3 H], wo [H][H], bo [H], ln2, ln2_b [H], w1 [F][H], b1 [F], w2 [H][F], b2 [H]},
 *   norm, norm_b [H].
 * Positions are position_ids, else 0 .. T-1 per row; both table indices are clamped to the tables (a memory guard: callers
 * check their ranges). KV-cached generation (slam_prefill / slam_decode_step / slam_extend) is not implemented for OPT: SLAM_EINVAL.
 * Arch 3 = Qwen3: the Qwen2 body (RMSNorm, RoPE, grouped-query attention, SwiGLU, the Qwen2 limits: hidden % 8 and <= 4096,
 * intermediate a multiple of 32, head_dim 64 or 128, n_heads a multiple of n_kv_heads with at most 8 query heads per KV head;
 * n_positions ignored) with no q / k / v bias and an RMSNorm over head_dim on every q and every k head before RoPE
 * (slam_op_qknorm_rope_fwd below). n_heads * head_dim need not equal hidden. Its layer tensors, in layout order:
 *   layers.N.{ln1 [H], wqkv [(nH + 2 nKV) hd][H], q_norm [hd], k_norm [hd], wo [H][nH hd], ln2 [H], wgu [2 I][H], wd [H][I]}
 * - there is no bqkv. Everything the Qwen2 family offers (training, "recompute", the untied head, KV-cached generation and
 * scoring) holds for arch 3; "Qwen2 only" below means arch 0 and 3. Arch 2 is not a family: SLAM_EINVAL. */
int slam_engine_create_arch(const SlamModelDesc* desc, int32_t arch, int32_t n_positions, SlamEngine** out);
/* The same with model flags (slam_engine_create / slam_engine_create_arch mean flags = 0). Arch 0 and 3 take hidden <= 4096
 * (rows above 2048 run the two-waves-per-row RMSNorm kernels), arch 1 hidden <= 2048.
 * SLAM_MODEL_UNTIED_HEAD (arch 0 and 3; Qwen2.5-7B): the LM head is a tensor of its own, "lm_head" [Vp][H], laid out AFTER
 * "norm" so that every other tensor keeps the offset it has in the tied layout. Its pad rows [vocab, Vp) are zero and stay
 * zero, as the embedding's do. Forward, prefill and decode read the head GEMM's weight there; backward writes
 * d lm_head = dlogits^T hf as that tensor's final value, and the embedding gradient is the gather side alone (rows of ids
 * absent from the batch, and the pad_token_id row, are exactly zero). Unknown flag bits, or the untied flag with arch 1:
 * SLAM_EINVAL. */
#define SLAM_MODEL_UNTIED_HEAD 1
int slam_engine_create_ex(const SlamModelDesc* desc, int32_t arch, int32_t n_positions, int32_t flags, SlamEngine** out);
void slam_engine_destroy(SlamEngine* h);
const char* slam_last_error(SlamEngine* h);
const char* slam_version(void);

/* ---- parameter layout -----------------------------------------------------------------------*/
int64_t slam_param_count(SlamEngine* h);   /* elements in the flat buffers (padded vocab rows incl.) */
int32_t slam_tensor_count(SlamEngine* h);
int slam_tensor_info(SlamEngine* h, int32_t index, SlamTensorInfo* out);
/* params: bf16 [slam_param_count], grads: fp32 [slam_param_count] (model.parameters() / .grad) */
int slam_bind_params(SlamEngine* h, void* params_bf16, float* grads_f32);
/* Optional bf16 [slam_param_count] buffer that receives every weight matrix TRANSPOSED (same
 * offsets): with it the dgrad GEMMs dX = dY W run as the fast contraction-contiguous form
 * dY (W^T)^T. Refreshed by slam_adamw_step / slam_cast_params / slam_refresh_transposed. */
int slam_bind_params_t(SlamEngine* h, void* params_t_bf16);
int slam_refresh_transposed(SlamEngine* h, slam_stream_t stream);

/* ---- workspace ------------------------------------------------------------------------------*/
size_t slam_workspace_bytes(SlamEngine* h, int64_t max_tokens);
int slam_bind_workspace(SlamEngine* h, void* ws, size_t bytes, int64_t max_tokens);

/* ---- forward / loss: UnitLM.forward + compute_loss (unit_lm.py:13-29,135-182) ----------------
 * ids/labels/position_ids: int64 [B*T] device (labels, position_ids nullable).
 * seg_start/seg_end: int32 [B*T] device, nullable -> dense rows of length T. For packed batches
 *   ([1, sum T] from DataCollatorWithFlattening) they give each token's sequence bounds.
 * num_items > 0 -> loss = sum / num_items (reduction "sum"), else mean over valid targets.
 * loss_out: fp32 [1] device (nullable when labels is NULL); logits_out: bf16 [B*T*vocab] device,
 * nullable. */
int slam_forward(SlamEngine* h, const int64_t* ids, const int64_t* labels, const int64_t* position_ids,
                 const int32_t* seg_start, const int32_t* seg_end, int32_t B, int32_t T, double num_items,
                 float* loss_out, void* logits_out, slam_stream_t stream);

/* ---- padding-free execution of right-padded batches (HF / TRL `padding_free`) ------------------------------------------------
 * slam_forward runs a right-padded [B][T] batch position by position: every pad token goes through all layers, the head and
 * the loss. slam_forward_unpadded runs the same batch as B segments of a flattened [1][M_packed] row - the layout of a packed
 * batch - and skips the pads. ids / labels: int64 [B][T] device (labels nullable); lens: int32 [B] DEVICE, 1 <= lens[b] <= T
 * (clamped to [0, T] as a memory guard: callers check their ranges); M_packed: chosen by the host, which knows the collated
 * mask - a multiple of 64 with sum(lens) <= M_packed <= B * T rounded up to 64, and no more than the bound workspace tokens.
 * One kernel packs the batch into `scratch` (caller-owned like the KV cache: 256-byte aligned, slam_unpadded_scratch_bytes(B, T)
 * bytes, BORROWED until slam_backward and the calls below are done); with Mmax = B * T rounded up to 64 it holds
 *   ids int64 [Mmax] | labels int64 [Mmax] | position_ids int64 [Mmax] | seg_start int32 [Mmax] | seg_end int32 [Mmax] |
 *   row int32 [Mmax] | off int32 [B + 1]
 * filled for m' < M_packed by the pack rule (off = exclusive prefix sum of lens): token (b, t), t < lens[b], goes to
 * m' = off[b] + t with ids'[m'] = ids[b][t], labels'[m'] = t == 0 ? -100 : labels[b][t] (the loss targets labels'[m' + 1]:
 * the flattening collator's rule), position_ids'[m'] = t, seg_start' = off[b], seg_end' = off[b + 1], row' = b. The tail
 * [off[B], M_packed) is one dummy segment: the pad id (0 without one), labels -100, positions from 0, row -1. Then the layers,
 * head and loss run exactly as slam_forward does for that packed row ("recompute", OPT's dropout, the logit mask,
 * "grad_final_next" and the bucket callback carry over; the dropout mask is keyed on the PACKED element index, so a token's
 * mask differs from the padded run's). num_items / loss_out as slam_forward. With non-ignored labels at pad positions
 * slam_forward has loss terms for predicting pads; this path has none. logits_out (nullable): bf16 [B][T][vocab], real positions
 * from their packed rows, pad positions zero. slam_backward needs no change. slam_last_forward_tokens: token rows the last
 * forward of either kind executed (B * T, or M_packed), 0 without one.
 * slam_seq_loglik_unpadded / slam_scale_loss_unpadded: slam_seq_loglik / slam_scale_loss_rows over the remembered segments
 * (ll_out, cnt_out, seq_coef: fp32 [B] device; the tail's rows are scaled by 0). SLAM_ESTATE unless the last forward was an
 * unpadded one over B rows (with labels); slam_seq_loglik / slam_scale_loss_rows after an unpadded forward are SLAM_ESTATE too.
 * slam_op_unpad_pack: the pack kernel alone (no engine), same scratch layout.
 *
 * Span batches (left- and both-side-padded rows: HF generate's output, TRL's prompt-left / completion-right pairs):
 * slam_forward_unpadded_spans takes the first real column of every row as well. Row b's real tokens are the columns
 * [starts[b], starts[b] + lens[b]) with 1 <= lens[b], 0 <= starts[b], starts[b] + lens[b] <= T; starts: int32 [B] DEVICE, read
 * only inside this call (by the pack and by the logits scatter), NULL = all zero = right padding: slam_forward_unpadded IS
 * this call with starts = NULL, launch for launch and bit for bit. starts are clamped to [0, T] and lens to [0, T - starts]
 * (a memory guard). The pack rule with spans: token (b, t), starts[b] <= t < starts[b] + lens[b], goes to
 * m' = off[b] + (t - starts[b]) with ids'[m'] = ids[b][t], position_ids'[m'] = t - starts[b] (a row's real tokens count from 0
 * in every family: OPT's own cumsum(mask) - 1 rule in HF, and for RoPE the same relative distances as HF's aranges),
 * labels'[m'] = t == starts[b] ? -100 : labels[b][t] (the first real token of a row is never a target: HF predicts it from
 * a pad query). off, seg_start', seg_end', row', the dummy tail, the scratch size and its layout are those above.
 * logits_out: bf16 [B][T][vocab], row b's real columns from their packed rows, zeros on both sides. Everything after the pack -
 * layers, head, loss, num_items, slam_backward, slam_seq_loglik_unpadded, slam_scale_loss_unpadded, "recompute", label
 * smoothing, the logit mask, NEFTune (scaled by the padded width T), OPT's dropout (keyed on the packed index) - is the
 * padding-free path unchanged: a span batch and the same rows right-padded run the same launches on the same packed arrays.
 * slam_op_unpad_pack_spans: slam_op_unpad_pack with starts (nullable). */
size_t slam_unpadded_scratch_bytes(int32_t B, int32_t T);
int slam_forward_unpadded(SlamEngine* h, const int64_t* ids, const int64_t* labels, const int32_t* lens, int32_t B, int32_t T,
                          int32_t M_packed, void* scratch, size_t scratch_bytes, double num_items, float* loss_out,
                          void* logits_out, slam_stream_t stream);
int slam_forward_unpadded_spans(SlamEngine* h, const int64_t* ids, const int64_t* labels, const int32_t* starts,
                                const int32_t* lens, int32_t B, int32_t T, int32_t M_packed, void* scratch, size_t scratch_bytes,
                                double num_items, float* loss_out, void* logits_out, slam_stream_t stream);
int64_t slam_last_forward_tokens(SlamEngine* h);
int slam_seq_loglik_unpadded(SlamEngine* h, int32_t B, float* ll_out, float* cnt_out, slam_stream_t stream);
int slam_scale_loss_unpadded(SlamEngine* h, const float* seq_coef, int32_t B, slam_stream_t stream);
int slam_op_unpad_pack(const int64_t* ids, const int64_t* labels, const int32_t* lens, int32_t B, int32_t T, int32_t M_packed,
                       int32_t pad_id, void* scratch, size_t scratch_bytes, slam_stream_t s);
int slam_op_unpad_pack_spans(const int64_t* ids, const int64_t* labels, const int32_t* starts, const int32_t* lens, int32_t B,
                             int32_t T, int32_t M_packed, int32_t pad_id, void* scratch, size_t scratch_bytes, slam_stream_t s);

/* ---- KV-cached generation: HF GenerationMixin.generate with use_cache (the reference's speech_lm.py / metric_utils.py call
 * model.generate(input_ids, attention_mask, bad_words_ids, temperature, top_k, max_new_tokens)) ---------------------------
 * The cache is caller-owned like the workspace: bf16, per layer K[max_batch][n_kv_heads][capacity][head_dim] followed by V of
 * the same shape (L x 2 x max_batch x n_kv_heads x capacity x head_dim x 2 bytes); K is stored after RoPE.
 * slam_prefill: ids int64 [B][T] right-padded, lens int32 [B] device (1 <= lens[b] <= T). Runs the forward's layer loop over
 *   the batch, copies each layer's K / V rows 0 .. lens[b]-1 into the cache and writes fp32 logits [B][vocab] of each row's
 *   last prompt token (one head launch over B rows). Replaces the cache contents.
 * slam_decode_step: ids int64 [B] device, one token per row at position lens[b]; appends its K / V, attends over rows
 *   0 .. lens[b], writes fp32 logits [B][vocab] and increments lens ON THE DEVICE (no host synchronisation). B must be the
 *   prefill's B and the workspace at least 2 B tokens. SLAM_ESTATE without a bound cache, without a prefill, or when the
 *   step could pass `capacity` (the host bound: prefill T + steps so far).
 * slam_kv_repeat: n continuations per prompt from one prefill. Precondition: a successful slam_prefill of B rows
 *   (optionally followed by slam_extend calls: a chunked prefill), no slam_decode_step since, and a bound cache with
 *   max_batch >= B n. For every layer, K and V, cache row b (keys
 *   0 .. lens[b]-1) is copied to rows b n .. b n + n - 1, bit for bit; keys at or beyond lens[b] of a destination row are
 *   unspecified and no later call reads them. lens: int32 [B n] device, first B entries filled; afterwards
 *   lens[b n + i] = old lens[b]. logits: nullable, fp32 [B n][vocab], first B rows filled, replicated the same way. Afterwards
 *   the decode batch is B n: slam_decode_step(.., B n, ..) is the next legal call. n == 1 is a no-op returning SLAM_OK.
 *   A further slam_kv_repeat(m) before any decode step is legal too: it fans the B n rows out to B n m rows (row r to rows
 *   r m .. r m + m - 1) under the same argument, given max_batch >= B n m.
 *   The expansion is in place and destination rows of a low b are source rows of a higher b (B = 3, n = 2: row 1 goes to
 *   rows 2 and 3 while row 2 is still a source). The scheme: one launch per source row in DESCENDING b on `stream`, each
 *   covering all layers, K, V, lens and logits. Launch b writes rows [b n, b n + n) except b itself (only row 0 is its own
 *   destination); for b >= 1 these are all > b, so no launch writes what it reads, and a later launch b' < b reads a row that
 *   lies below every destination written before it. Hazard-free for every (B, n). Only lens[b] keys are copied (lens is read
 *   on the device: no host synchronisation), with 16-byte loads and stores of whole key rows.
 *   Errors, all before any launch: SLAM_EINVAL for h or lens NULL, n < 1 or B n > max_batch; SLAM_ESTATE without a bound
 *   cache, without a prefill, or after a decode step. slam_extend calls between the prefill and the fan-out are fine.
 * slam_extend: appends a chunk of up to T tokens per row behind the keys the cache already holds - chunked prefill, a
 *   continuation of a cached sequence. (Teacher-forcing a given continuation or verifying several proposed tokens at once
 *   needs every chunk position scored: slam_extend_score, below.)
 *   ids: int64 [B][T] device, right-padded with any valid id. new_lens: int32 [B] device, 0 <= new_lens[b] <= T: the real
 *   tokens of row b are columns 0 .. new_lens[b]-1. lens: int32 [B] device, the rows' key counts - the array
 *   slam_decode_step advances. Token t of row b runs at position lens[b] + t: one layer loop over B T tokens (the prefill's
 *   projections, norms and MLP), each layer's K / V of the real tokens appended bit for bit to cache rows lens[b] + t, and
 *   attention of every real token over cache rows 0 .. lens[b] + t (exp2 domain, fp32 accumulation, on the matrix pipe;
 *   split partials merged in split order: bit-identical run to run). logits_out: fp32 [B][vocab]; row b receives the logits
 *   of row b's LAST new token when new_lens[b] > 0 (one head launch over B rows), and lens[b] += new_lens[b] ON THE DEVICE -
 *   no host synchronisation anywhere. A row with new_lens[b] == 0 is inert: its logits_out row, lens[b] and every one of its
 *   cache rows keep their bits. The logits of a prompt prefilled in chunks differ from a one-shot slam_prefill's by rounding
 *   only (another attention kernel, the same maths).
 *   Preconditions: a bound cache that a slam_prefill filled; B equal to the current decode batch (the prefill's B, times n
 *   after a slam_kv_repeat); lens[b] + new_lens[b] within the host bound below (it is for every sequence of calls that passes
 *   these arrays on unchanged). Legal after slam_prefill, after decode steps, after slam_kv_repeat and after another
 *   slam_extend. The host bound of the cached lengths advances by T whatever new_lens holds. slam_kv_repeat stays legal
 *   behind any number of slam_extend calls as long as no slam_decode_step ran since the prefill (chunked prefill, then the
 *   fan-out); once a decode step ran, a slam_extend does not make it legal again.
 *   Unspecified: cache rows at or beyond lens[b] + new_lens[b]; the values the padded columns computed (nothing reads them:
 *   their attention output is written as zeros and no K / V of theirs reaches the cache); logits_out and the cache when
 *   new_lens[b] is outside [0, T] or lens[b] is not the row's key count (the kernels clamp both to the host bound, so such a
 *   call stays inside the cache).
 *   Errors, all before any launch: SLAM_EINVAL for a NULL argument, B <= 0, T <= 0, B different from the decode batch, or an
 *   OPT engine; SLAM_ESTATE without bound parameters / workspace, without a bound cache, without a prefill, or when the host
 *   bound + T would pass `capacity`; SLAM_ENOMEM when B T, or the 2 B tokens of the decode scratch, exceed the bound workspace
 *   tokens. Works with every "recompute" level (the layers may share their q|k|v slot: each layer's chunk is consumed before
 *   the next layer's projection).
 * Prefill, extend and decode overwrite the forward activations (slam_backward then needs a new slam_forward).
 * What generation offers: greedy decoding and temperature / top-k / top-p sampling with banned tokens, EOS and pad handling,
 * either chosen by the caller from the logits or on the device by slam_sample_tokens (below; top_k 1 .. 256, reproducible
 * per row); n sampled continuations per prompt from one prefill (slam_kv_repeat), and the model's own log-probability of
 * every chosen token (slam_token_logprobs, below); prompts prefilled in chunks whose size, not the prompt length, sets the
 * workspace, and k tokens per row appended to a live cache (slam_extend); bans that depend on a row's own history - no
 * repeated n-gram, multi-token bad words, no EOS yet - on the device (slam_constrain_scores, below); a draft model's proposals
 * verified K + 1 positions at a time and rolled back where the target disagrees (slam_extend_logits, slam_sample_tokens_at,
 * slam_spec_accept, slam_kv_rewind, below), or proposals looked up in the row's own history (slam_ngram_propose, below). No
 * beam search, no repetition penalty, no OPT. */
size_t slam_kv_cache_bytes(SlamEngine* h, int32_t max_batch, int32_t capacity);
int slam_bind_kv_cache(SlamEngine* h, void* cache, size_t bytes, int32_t max_batch, int32_t capacity);
int slam_prefill(SlamEngine* h, const int64_t* ids, const int32_t* lens, int32_t B, int32_t T, float* logits_out,
                 slam_stream_t stream);
int slam_decode_step(SlamEngine* h, const int64_t* ids, int32_t* lens, int32_t B, float* logits_out, slam_stream_t stream);
int slam_kv_repeat(SlamEngine* h, int32_t n, int32_t* lens, float* logits, slam_stream_t stream);
int slam_extend(SlamEngine* h, const int64_t* ids, const int32_t* new_lens, int32_t* lens, int32_t B, int32_t T,
                float* logits_out, slam_stream_t stream);

/* ---- scoring a given continuation through the cache (teacher forcing, verifying proposed tokens, a frozen reference's
 * log-probs of sampled continuations) ------------------------------------------------------------------------------------------
 * slam_extend_score is slam_extend - the same body, the same launches in the same order, so for equal arguments the cache,
 * lens and logits_out are bit-identical to slam_extend's - plus, between the layer loop and the last-token head, the final
 * norm of all B T chunk rows and the LM head fused with the row statistics (slam_op_score_rows below: fp32 scores that are
 * never rounded to bf16 and never stored).
 *   lp_out   fp32 [B][T] device. Column t with 1 <= t < new_lens[b]: the log-prob OF ids[b][t] given the cache and
 *            ids[b][0 .. t). Columns t >= max(1, new_lens[b]) are 0.0f. Column 0 is NEVER written: it belongs to the caller,
 *            who fills it with slam_token_logprobs(column = 0, out_stride = T) on the logits the rows held before this call
 *            (a prefill's, a decode step's or the previous chunk's logits_out). Chunks chain the same way.
 *   argmax_out  int64 [B][T] device, nullable. t < new_lens[b]: the greedy next token after position t (the lowest id of the
 *            largest score, -1 when no score is above -inf); -1 for t >= new_lens[b]. A proposed token ids[b][t + 1] is
 *            accepted iff it equals argmax_out[b][t].
 * The logit mask (slam_set_logit_mask) is honoured: a masked column counts as -inf, a masked target gives -inf. The rows of
 * padded positions are computed and dropped. Scratch, all in buffers the call leaves free behind the layer loop: the rows'
 * targets (int64 [B T]) in the backward-only d(qkv) buffer; the chunk partials ([B T][chunks] x 16 bytes) and the targets'
 * scores at the start of the logits buffer - the attention split partials that lived there are dead by then, and the
 * last-token fp32 logits are written there only behind these launches (one stream); the normed rows in the final-norm
 * buffer, which the last-token norm then overwrites. Errors: those of slam_extend, plus SLAM_EINVAL for a NULL lp_out, all
 * before any launch; an OPT engine returns SLAM_EINVAL as slam_extend does. */
int slam_extend_score(SlamEngine* h, const int64_t* ids, const int32_t* new_lens, int32_t* lens, int32_t B, int32_t T,
                      float* logits_out, float* lp_out, int64_t* argmax_out, slam_stream_t stream);

/* ---- verifying proposed tokens under a sampler: the logits of every chunk position, and the rollback (draft-model
 * speculative decoding: HF's generate(assistant_model=)) -----------------------------------------------------------------------
 * slam_extend_logits is the third mode of the body slam_extend and slam_extend_score share: the same launches in the same
 * order up to the end of the layer loop, so for equal arguments the cache and lens are bit-identical to slam_extend's. Instead
 * of the last-token head it runs the final norm of all B T chunk rows and the fp32 LM head over all of them (the projection
 * kernel of slam_prefill / slam_decode_step's head; in groups of at most half the bound workspace tokens, each group through
 * the logits buffer, whose attention partials are dead by then).
 *   logits_all  fp32 [B][T][vocab] device, caller-owned. Row (b, t) with t < new_lens[b] receives the logits after token t of
 *               row b: what slam_decode_step would have written had the chunk been fed one token at a time, up to the
 *               rounding between the two attention kernels. Rows with t >= new_lens[b] are NOT written: they keep their bits.
 *   lens[b] += new_lens[b] on the device, by a launch of its own behind the head; a row with new_lens[b] == 0 is inert.
 * There is no logits_out: row (b, new_lens[b] - 1) holds what slam_extend would have put there. The logit mask is NOT applied
 * (the sampler's `banned` does that). The host bound advances by T, as under slam_extend. Errors: those of slam_extend (with
 * logits_all in the place of logits_out), all before any launch.
 * slam_kv_rewind is host-only: it sets the host bound of the cached lengths to hi, 1 <= hi <= the current bound. The caller
 * promises lens[b] <= hi for every row of the arrays it passes on (after it lowered them itself: lowering lens[b] IS the
 * rollback - keys at or beyond lens[b] are unspecified and the next append overwrites them). The kernels keep clamping to the
 * bound, so a broken promise stays inside the cache. Without this call the bound - and with it the split count of the decode /
 * extend attention and the room left below `capacity` - grows by T per slam_extend_logits whatever was kept. slam_kv_repeat is
 * refused afterwards (SLAM_ESTATE), as it is after a decode step. SLAM_EINVAL for h NULL or hi outside the range; SLAM_ESTATE
 * without a bound, prefilled cache. */
int slam_extend_logits(SlamEngine* h, const int64_t* ids, const int32_t* new_lens, int32_t* lens, int32_t B, int32_t T,
                       float* logits_all, slam_stream_t stream);
int slam_kv_rewind(SlamEngine* h, int32_t hi);

/* ---- decoding from FP8 weights: an exact, power-of-two-scaled e4m3 copy of the decode projections ----
 * A decode step (and an extend pass of up to 64 rows) is one stream of the weights. This copy halves the bytes of that stream
 * for wqkv, wo, wgu and wd of every layer (and the head matrix when include_head) without a second model: quantising REPLACES
 * the bf16 parameters by the values the codes stand for, so the bf16 kernels (prefill, extend above 64 rows, slam_forward,
 * scoring) and the FP8 stream compute the same model, bit for bit.
 * The rule, per row n of a matrix W[N][K], amax = max_k |W[n][k]| = f 2^x with 1 <= f < 2:
 *   e[n] = 0 for a zero row, else the smallest integer with amax <= 448 2^e - x - 8 when f <= 1.75, x - 7 above, taken from
 *          the bf16 bits - clamped to [-100, 120];
 *   q[n][k] = the OCP e4m3fn code of W[n][k] 2^-e[n], round to nearest even, the sign of zero kept (|value| <= 448 by
 *          construction: the NaN codes 0x7F / 0xFF never appear and nothing saturates);
 *   Wdq[n][k] = value(q[n][k]) 2^e[n], exact in bf16.
 * The decode kernel turns code -> fp32 -> times 2^e -> high 16 bits and feeds the MFMA exactly as the bf16 kernel is fed from
 * Wdq: same lanes, same K order, same split plan, same reduce launch. Non-finite weights are outside the contract (the caller
 * checks). A row whose amax reaches 1.9375 * 2^127 rounds up to 2^128: do not quantise such weights.
 * Storage: exponents are int8, one per row. Codes take N K bytes; their order inside a row is PRIVATE to the engine (every
 * 64-deep K block is permuted so that a lane's 16-byte load holds its operands of two MFMA steps): read them back with
 * slam_op_dequantize_rows_fp8 only. The path needs K % 64 == 0 for every matrix - hidden, intermediate and
 * n_heads * head_dim multiples of 64; other engines are refused at bind time and decode stays on bf16.
 * slam_decode_w8_bytes: the buffer for all matrices (256-byte aligned sub-buffers; 0 for a refused engine or OPT).
 * slam_bind_decode_w8: caller-owned device buffer, 256-byte aligned; NULL unbinds. Resets the launch counter. SLAM_EINVAL with
 *   a message for OPT (arch 1: no decode path) and for a refused K; SLAM_ENOMEM for a short buffer. State 1 afterwards.
 * slam_quantize_decode_w8: joins the optimizer and pending parameter all-gathers (as slam_decode_step does), quantises the
 *   bound parameters IN PLACE (they become Wdq), refreshes the transposed images if bound, and marks the codes valid (state 2).
 *   With a tied head and include_head the head matrix IS the embedding table: its first `vocab` rows become Wdq too, so the
 *   embedding lookup changes with it. A caller that keeps an fp32 master copies Wdq into it itself.
 * slam_decode_w8_state: 0 unbound, 1 bound but stale, 2 valid. Every entry point that writes or rebinds the parameters drops 2
 *   to 1 - slam_bind_params, slam_cast_params, every slam_adamw_*, slam_allgather_params_async, and slam_refresh_transposed
 *   (what a caller that wrote the buffer itself must call anyway). Decode then runs the bf16 kernels: always correct.
 * slam_decode_w8_launches: FP8 projection launches since the bind (4 per layer, + 1 with the head, per decode step). */
size_t slam_decode_w8_bytes(SlamEngine* h, int32_t include_head);
int slam_bind_decode_w8(SlamEngine* h, void* buf, size_t bytes, int32_t include_head);
int slam_quantize_decode_w8(SlamEngine* h, slam_stream_t stream);
int slam_decode_w8_state(SlamEngine* h);
int64_t slam_decode_w8_launches(SlamEngine* h);

/* ---- choosing the next token on the device (what HF's logits processors + torch.multinomial do between two decode steps) ----
 * slam_sample_tokens needs no engine: it reads fp32 logits [B][vocab] (row stride vocab, 4-byte aligned; odd vocabularies
 * are fine) such as slam_prefill / slam_decode_step wrote, and writes the chosen ids where slam_decode_step reads them, so a
 * generate loop is  prefill, sample(step 0), { decode_step(next), sample(step k) }  on one stream with nothing in between.
 * The contract, for row b with row id r = row_ids ? row_ids[b] : b, step s = desc->step and x_i the logit of token i:
 *   finished   done && done[b]: next[b] = pad_id, the out column gets pad_id, nothing else happens.
 *   scores     banned tokens (banned[i] != 0) and NaN logits count as -inf; +inf counts as FLT_MAX and -0 as +0. A row
 *              without a score above -inf emits pad_id and is NOT marked done.
 *   greedy     (do_sample == 0) the lowest i with x_i == max.
 *   sampling   k' = min(top_k, number of scores above -inf). The candidates are the k' largest scores ordered by (x descending,
 *              i ascending); that order is the rank j. A tie at the k-th value goes to the lower id (HF keeps every such tie:
 *              the one deviation). inv_t = 1.0f / temperature; w_j = expf((x_j - x_0) * inv_t) in fp32, w_0 = 1.
 *              top_p < 1: tail_j = w_{k'-1} + ... + w_j summed in fp32 from the last rank upward, P = tail_0; rank j > 0 is
 *              dropped when tail_j <= (1.0f - top_p) * P (HF's rule, cum <= 1 - top_p on the ascending sort, rank 0 always
 *              kept). The kept ranks are a prefix of m ranks (m = k' for top_p = 1).
 *              cum_j = w_0 + ... + w_j in fp32, in that order; total = cum_{m-1}; u = (philox.w[0] >> 8) * 2^-24; the token
 *              is the candidate of the lowest j with cum_j > u * total, or j = m - 1 if there is none.
 *              Philox4x32-10 (the generator of "adamw_sr" / "dropout_thr16"): counter (r & 0xffffffff, s, r >> 32, 0x53414D50),
 *              key (seed & 0xffffffff, seed >> 32).
 *   after      next[b] = token; out[b * out_stride + s] = token when out is given; done[b] = 1 when done is given and the
 *              token is one of eos_ids[0 .. n_eos).
 * A row's result depends on (its logits, banned, the description, r) alone: not on B, the row's index, the launch shape or
 * an earlier call, and it is the same bits on every run (no floating-point atomics). Rows longer than 2048 take two launches
 * (per-chunk top k into the workspace, then one block per row), shorter ones a single launch.
 * banned: uint8 [vocab]; row_ids: int64 [B]; eos_ids: int32 [n_eos]; done: uint8 [B]; next: int64 [B]; out: int64 - all device
 * memory, nullable where the contract says "when given". ws: slam_sample_workspace_bytes(B, vocab, do_sample ? top_k : 1)
 * bytes of device memory, 8-byte aligned (the function itself is host-only arithmetic: positive for valid arguments, 0 else).
 * SLAM_EINVAL, before anything is launched or dereferenced on the device: logits, desc or next NULL; B <= 0 (or > 65535);
 * vocab <= 0; do_sample other than 0 / 1; sampling with top_k outside 1 .. 256; temperature <= 0; top_p outside (0, 1];
 * n_eos outside 0 .. 16; n_eos > 0 without eos_ids; ws NULL or ws_bytes too small. */
typedef struct SlamSampleDesc {
  int32_t do_sample;   /* 0 greedy, 1 sample */
  int32_t top_k;       /* sampling: 1 .. 256 */
  float temperature;   /* > 0 */
  float top_p;         /* (0, 1] */
  uint64_t seed;
  uint32_t step;       /* index of the new token: 0 for the one drawn from the prefill logits */
  int32_t pad_id;
  int32_t n_eos;       /* 0 .. 16 */
} SlamSampleDesc;
size_t slam_sample_workspace_bytes(int32_t B, int32_t vocab, int32_t top_k);
int slam_sample_tokens(const float* logits, int32_t B, int32_t vocab, const uint8_t* banned, const SlamSampleDesc* desc,
                       const int64_t* row_ids, const int32_t* eos_ids, uint8_t* done, int64_t* next, int64_t* out,
                       int64_t out_stride, void* ws, size_t ws_bytes, slam_stream_t stream);
/* slam_sample_tokens_at is slam_sample_tokens - the same kernels with one more nullable pointer - for rows that sit at
 * different steps: the K + 1 positions of a verified chunk, or sequences that have emitted different numbers of tokens. Row b
 * belongs to sequence q = b / group and is its column j = b % group. Its row id is r = row_ids ? row_ids[q] : q, its step is
 * s = desc->step + (steps ? steps[q] : 0) + j (uint32 arithmetic), and out[b * out_stride + out_col] receives the token when
 * out is given. done and next are indexed by b; logits has B rows. Everything else is slam_sample_tokens' contract, word for
 * word: a row's token is the one slam_sample_tokens picks from the same logits with row id r at step s.
 * steps: uint32 [B / group] device, nullable; row_ids: int64 [B / group]. SLAM_EINVAL as slam_sample_tokens, plus group < 1,
 * B not a multiple of group, or out_col < 0. slam_sample_tokens is the case steps = NULL, group = 1, out_col = desc->step. */
int slam_sample_tokens_at(const float* logits, int32_t B, int32_t vocab, const uint8_t* banned, const SlamSampleDesc* desc,
                          const int64_t* row_ids, const int32_t* eos_ids, uint8_t* done, int64_t* next, int64_t* out,
                          int64_t out_stride, void* ws, size_t ws_bytes, const uint32_t* steps, int32_t group, int32_t out_col,
                          slam_stream_t stream);
/* slam_sample_tokens_warped is slam_sample_tokens_at followed by the second half of HF's warper chain (min_p, typical_p,
 * epsilon_cutoff, eta_cutoff, in GenerationMixin._get_logits_processor's order) on the ranked candidates: HF applies these
 * after top-k, so they only see the k' <= 256 candidates the sampler already holds, and no second pass over the vocabulary
 * is made. warp == NULL or all four off ({0, 1, 0, 0}) IS slam_sample_tokens_at: the same launches, the same tokens, done,
 * next and out, bit for bit. Greedy (do_sample == 0) ignores the warp description beyond its range check, as HF ignores
 * warpers when it does not sample. min_tokens_to_keep is 1 throughout.
 * The contract continues slam_sample_tokens' at the top-p prefix: ranks 0 .. m-1 by (x descending, id ascending), fp32 weights
 * w_j = expf(a_j), a_j = (x_j - x_0) * inv_t (a_0 = 0, w_0 = 1). S is the set of ranks still kept (at first 0 .. m-1); every
 * step below that is on acts on the S the steps before it left. All arithmetic is fp32, one operation at a time:
 *   Z_S   = the sum of w_j over j in S, added in ascending rank order starting from 0.0f.
 *   p_j   = w_j / Z_S;   log p_j = a_j - logf(Z_S)   (from the scaled score, not logf(p_j): finite where w_j underflows).
 *   H_S   = -(the sum of p_j * log p_j over j in S with w_j > 0, added in ascending rank order from 0.0f)   ("0 log 0 = 0").
 *   min_p       on for 0 < min_p <= 1 (0 off). w_top = the weight of the lowest rank in S. Rank j leaves S when
 *               w_j < min_p * w_top (HF's probs < min_p * max prob; the normaliser cancels). The lowest rank never leaves.
 *   typical_p   on for 0 < typical_p < 1 (1 off). s_j = fabsf(-log p_j - H_S). S is ordered by (s ascending, rank ascending):
 *               HF's torch.sort leaves the order of equal s unspecified, this tie rule is ours (the second deviation, beside
 *               the tie at the k-th score). c_i = p of the first i + 1 ranks of that order, added in that order from 0.0f.
 *               last = min(#{i : c_i < typical_p}, |S| - 1). Rank j leaves S when s_j > s of the last-th rank of the order;
 *               the first rank of the order never leaves. S need no longer be a prefix afterwards: rank 0 can leave.
 *   epsilon_cutoff  on for 0 < eps < 1 (0 off). Rank j leaves S when p_j < eps, unless x_j equals the score of the lowest
 *               rank in S (HF exempts scores >= the top-1 score, so every tie at the top stays).
 *   eta_cutoff  on for 0 < eps < 1 (0 off). eta = fminf(eps, sqrtf(eps) * expf(-H_S)); rank j leaves S when p_j < eta, with
 *               the same exemption.
 *   draw        cum runs over the ranks of S in ascending rank order (cum += w_j from 0.0f); total = the last cum; u is the
 *               SAME Philox word as without warpers (one draw per (row id, step), nothing further is consumed); the token
 *               is the candidate of the lowest rank in S with cum > u * total, or of the highest rank in S if there is none.
 * The sums run in the stated order on one thread, the typical_p order is formed by counting (position = the number of ranks
 * of S that come first), so a row's result is the same bits on every run and does not depend on B, the row's index or the
 * launch shape (no floating-point atomics). Because the chain runs on the top-k candidates it equals HF's exactly when
 * 1 <= top_k <= 256 is part of the request. The workspace is slam_sample_tokens_at's (slam_sample_workspace_bytes).
 * SLAM_EINVAL, before anything is launched or dereferenced on the device: slam_sample_tokens_at's list, plus min_p outside
 * [0, 1], typical_p outside (0, 1], epsilon_cutoff or eta_cutoff outside [0, 1), or a NaN in any of the four. */
typedef struct SlamWarpDesc {
  float min_p;           /* [0, 1], 0 = off */
  float typical_p;       /* (0, 1], 1 = off */
  float epsilon_cutoff;  /* [0, 1), 0 = off */
  float eta_cutoff;      /* [0, 1), 0 = off */
} SlamWarpDesc;
int slam_sample_tokens_warped(const float* logits, int32_t B, int32_t vocab, const uint8_t* banned, const SlamSampleDesc* desc,
                              const int64_t* row_ids, const int32_t* eos_ids, uint8_t* done, int64_t* next, int64_t* out,
                              int64_t out_stride, void* ws, size_t ws_bytes, const uint32_t* steps, int32_t group,
                              int32_t out_col, const SlamWarpDesc* warp, slam_stream_t stream);

/* ---- the acceptance rule of draft-model speculative decoding, on the device -------------------------------------------------
 * slam_spec_accept needs no engine. One round of assisted generation proposes K tokens per row with a draft model, lets the
 * target sample its own token at every chunk position (slam_extend_logits + slam_sample_tokens_at with the SAME stateless
 * draw the draft used), and keeps the target's tokens up to and including the first one the draft did not propose. Because
 * the draw is a function of (logits, seed, row id, step), the kept tokens are exactly what one-token-per-step decoding emits.
 * Per row b, with x0 = chunk[b][0] the pending token (emitted, not yet in the target's cache), d_i = chunk[b][i] (1 <= i <= K)
 * the proposals and t_j = tgt[b][j] (0 <= j <= K) the target's token for the position behind column j:
 *   done[b] != 0 on entry: the row emits nothing (m = 0, lag = 0).
 *   otherwise   n_acc = the largest n <= K with d_i == t_{i-1} for all 1 <= i <= n. The candidates are t_0 .. t_{n_acc}; they
 *               are cut to max_new - n_new[b] tokens, then behind the first one that is an eos_ids entry (which sets done[b] =
 *               1); m >= 1 tokens remain (a row whose budget is not positive emits none and is marked done). Reaching
 *               n_new[b] + m == max_new sets done[b] = 1 too.
 * Writes, all of them plain stores of the row's own thread:
 *   out[b * out_stride + n_new[b] + i] = t_i for i < m (nothing else of out is touched); n_new[b] += m;
 *   lens_t[b] = prompt_len[b] + n_new[b] - 1   the target's key count, ABSOLUTE - this store is the rollback;
 *   lag = (m == K + 1); lens_d[b] = lens_t[b] - lag   the draft's key count: after full acceptance its cache lacks d_K;
 *   chunk[b][0] = the last emitted token (unchanged when m = 0);
 *   draft_ids[b][0 .. 2) = lag ? { d_K, t_K } : { chunk[b][0], pad_id }; draft_new_lens[b] = done ? 0 : 1 + lag   (the
 *               draft's catch-up block for slam_extend with T = 2); tgt_new_lens[b] = done ? 0 : K + 1;
 *   stats int32 [5] = { rows not done after the round, max lens_t, max lens_d (both over ALL rows: the arguments of
 *               slam_kv_rewind), tokens emitted this round (sum of m), proposals among them (sum of min(m, n_acc)) }.
 * Rows that are done get lens_t / lens_d written too: the draft's decode steps advance every row. The invariant a round
 * starts from and ends in: the committed sequence of row b is its prompt plus n_new[b] tokens; the target's cache holds it
 * without its last token, the draft's cache that prefix without `lag` more tokens.
 * One launch of one block, a thread per row; integer work only, the five sums / maxima combined through shared memory in a
 * fixed order (no atomics). chunk, tgt: int64 [B][K + 1]; n_new, prompt_len, lens_t, lens_d, draft_new_lens, tgt_new_lens:
 * int32 [B]; done: uint8 [B]; out: int64 [B][out_stride]; draft_ids: int64 [B][2]; eos_ids: int32 [n_eos] - all device memory.
 * SLAM_EINVAL before the launch: a NULL array (eos_ids may be NULL when n_eos == 0); B outside 1 .. 1024; K outside 1 .. 15;
 * n_eos outside 0 .. 16; max_new < 1 or out_stride < max_new. */
int slam_spec_accept(int64_t* chunk, const int64_t* tgt, int32_t B, int32_t K, int32_t max_new, int32_t pad_id,
                     const int32_t* eos_ids, int32_t n_eos, const int32_t* prompt_len, int32_t* n_new, uint8_t* done,
                     int64_t* out, int64_t out_stride, int32_t* lens_t, int32_t* lens_d, int64_t* draft_ids,
                     int32_t* draft_new_lens, int32_t* tgt_new_lens, int32_t* stats, slam_stream_t stream);

/* ---- proposals without a draft model: the tokens that followed an earlier occurrence of the row's own last n-gram (HF's
 * generate(prompt_lookup_num_tokens=, max_matching_ngram_size=), PromptLookupCandidateGenerator) -----------------------------
 * slam_ngram_propose needs no engine. It fills the proposal columns of the chunk that slam_extend_logits verifies and
 * slam_spec_accept judges. The history h of row b is, with pl = prompt_len[b] clamped to [0, prompt_stride] and
 * s = n_new[b] clamped to [0, new_stride]:
 *   h[0 .. pl)        = prompt[b * prompt_stride + 0 .. pl)   (right-padded prompt ids; pads are not history)
 *   h[pl .. pl + s)   = new_tokens[b * new_stride + 0 .. s)   (the `out` buffer of slam_spec_accept, with the n_new it keeps)
 * and Lh = pl + s: the layout slam_constrain_scores reads. Nothing outside these two ranges is read.
 * The rule, restating transformers' PromptLookupCandidateGenerator.get_candidates:
 *   match      for n = min(max_ngram, Lh - 1) down to 1: the smallest idx in [0, Lh - n) with h[idx .. idx + n) ==
 *              h[Lh - n .. Lh). The tail window itself is no candidate; a window that overlaps it is. The longest n with any
 *              match wins, within it the EARLIEST match.
 *   proposals  h[idx + n .. min(idx + n + K, Lh)), cut in front of the first token that is an eos_ids entry. What is left,
 *              n_prop[b] tokens (0 .. K), goes to chunk[b][1 .. 1 + n_prop[b]). A cut that leaves nothing proposes nothing:
 *              there is no fall-back to a shorter n or a later match (HF's behaviour). No match at any n, and Lh <= 1,
 *              propose nothing.
 *   finished   done[b] != 0: n_prop[b] = 0.
 *   fill       chunk[b][1 + n_prop[b] .. K] = fill_id. Column 0 is NEVER touched: slam_spec_accept owns it.
 *   stats      int32 [2], nullable = { rows with n_prop[b] > 0, the sum of n_prop[b] }, by a second launch of one block behind
 *              the first, combined through shared memory in a fixed order (no atomics).
 * One block per row: every thread takes the window ends e = t, t + 256, .. of [0, Lh - 1), counts how many tokens back from e
 * equal the tokens back from the end of h (at most min(max_ngram, Lh - 1)), and the block keeps the longest count, the lowest e
 * among equals; idx + n = e + 1. Integer work only: the same bits on every run, whatever B.
 * chunk int64 [B][K + 1]; n_prop, prompt_len, n_new int32 [B]; prompt int64 [B][prompt_stride]; new_tokens int64
 * [B][new_stride]; done uint8 [B]; eos_ids int32 [n_eos] - all device memory.
 * SLAM_EINVAL before any launch: a NULL array (eos_ids may be NULL when n_eos == 0; stats may be NULL); B outside 1 .. 1024
 * (slam_spec_accept's limit); K outside 1 .. 15; max_ngram outside 1 .. SLAM_NGRAM_MAX; n_eos outside 0 .. 16; a negative
 * stride or one of 2^30 or more. */
#define SLAM_NGRAM_MAX 16
int slam_ngram_propose(int64_t* chunk, int32_t* n_prop, int32_t B, int32_t K, int32_t max_ngram, int32_t fill_id,
                       const int64_t* prompt, int64_t prompt_stride, const int32_t* prompt_len, const int64_t* new_tokens,
                       int64_t new_stride, const int32_t* n_new, const uint8_t* done, const int32_t* eos_ids, int32_t n_eos,
                       int32_t* stats, slam_stream_t stream);

/* ---- per-row bans that depend on the row's own history (HF's no_repeat_ngram_size, multi-token bad_words_ids,
 * min_new_tokens / min_length, begin_suppress_tokens), between the logits and slam_sample_tokens ------------------------------
 * slam_constrain_scores needs no engine. It reads fp32 logits [B][vocab] (row stride vocab, 4-byte aligned; odd vocabularies
 * are fine) and writes scores [B][vocab] of the same layout:
 *   scores[b][i] = -inf for every token i that row b bans, the BITS of logits[b][i] (NaN and +-inf included) everywhere else.
 * scores may be the same pointer as logits: then only the bans are written. (slam_token_logprobs is defined on the raw
 * logits, so a caller who wants log-probs gives scores a buffer of its own, samples from scores and scores the logits.)
 * The history h of row b at step s = desc->step (s new tokens exist) is, with pb = b / n_per_prompt and
 * pl = prompt_len[pb] clamped to [0, prompt_stride]:
 *   h[0 .. pl)        = prompt[pb * prompt_stride + 0 .. pl)   (right-padded prompt ids; pads are not history)
 *   h[pl .. pl + s)   = new_tokens[b * new_stride + 0 .. s)    (the `out` buffer of slam_sample_tokens)
 * and Lh = pl + s. prompt_len is a copy of the lengths taken BEFORE decoding: slam_decode_step increments its lens.
 * Bans, all restating transformers' logits processors on h:
 *   n-gram     n = no_repeat_ngram >= 1 (0 = off): nothing when Lh < n; else, with p = h[Lh - n + 1 .. Lh) (the last n - 1
 *              tokens), every j in 0 .. Lh - n with h[j .. j + n - 1) == p bans h[j + n - 1]. n = 1 bans every token seen.
 *   sequences  n_seqs bad word sequences, sequence q = seq_tokens[seq_offsets[q] .. seq_offsets[q + 1]), of length Lw: bans
 *              its last token when 2 <= Lw <= Lh and the last Lw - 1 history tokens equal its first Lw - 1. A sequence with
 *              Lw < 2, Lw > SLAM_CONSTRAIN_MAX_SEQ_LEN or offsets outside [0, n_seq_tokens] is ignored (single-token bad
 *              words belong in the sampler's banned[vocab]).
 *   ban_eos    (0 / 1, decided per step by the caller: s < min_new_tokens, or prompt width + s < min_length) bans
 *              eos_ids[0 .. n_eos).
 *   begin      begin_ids[0 .. n_begin) are banned when s == 0.
 * A history token or list entry outside [0, vocab) bans nothing and nothing is written for it (it still takes part in the
 * comparisons). A row with done && done[b] is copied, not edited. A row's result depends on (its logits, its history, the
 * description) alone - not on B, the row's index or the launch shape - and is the same bits on every run: behind the copy
 * the only stores are of one constant, so there are no atomics. One launch: grid (chunks of 2048 scores, B); a block copies
 * its chunk (16-byte accesses where logits and scores are equally aligned, 4-byte at the ragged ends and otherwise), then
 * scans the history and stores the bans that fall inside its own chunk.
 * prompt int64 [B / n_per_prompt][prompt_stride]; prompt_len int32 [B / n_per_prompt]; new_tokens int64 [B][new_stride]
 * (nullable when step == 0); done uint8 [B], nullable; eos_ids int32 [n_eos]; begin_ids int32 [n_begin]; seq_tokens int32
 * [n_seq_tokens]; seq_offsets int32 [n_seqs + 1] - all device memory.
 * SLAM_EINVAL, before anything is launched or dereferenced on the device: logits, scores, desc, prompt or prompt_len NULL;
 * B <= 0 or B > 65535; vocab <= 0; no_repeat_ngram < 0; n_per_prompt < 1; B % n_per_prompt != 0; ban_eos other than 0 / 1;
 * step or prompt_stride outside 0 .. 2^30; step > 0 with new_tokens NULL or new_stride < step; n_eos outside 0 .. 16, n_begin
 * outside 0 .. SLAM_CONSTRAIN_MAX_BEGIN, n_seqs outside 0 .. SLAM_CONSTRAIN_MAX_SEQS, n_seq_tokens outside
 * 0 .. SLAM_CONSTRAIN_MAX_SEQS * SLAM_CONSTRAIN_MAX_SEQ_LEN; a positive count without its list(s); logits, scores or an
 * int32 list not 4-byte aligned, prompt or new_tokens not 8-byte aligned. */
#define SLAM_CONSTRAIN_MAX_SEQS 256
#define SLAM_CONSTRAIN_MAX_SEQ_LEN 16
#define SLAM_CONSTRAIN_MAX_BEGIN 256
typedef struct SlamConstrainDesc {
  int32_t step;            /* s: new tokens that exist; 0 for the token drawn from the prefill logits */
  int32_t no_repeat_ngram; /* n >= 1, 0 = off */
  int32_t n_per_prompt;    /* rows b n .. b n + n - 1 share prompt b */
  int32_t prompt_stride;   /* row stride of prompt, in tokens */
  int32_t ban_eos;         /* 0 / 1 */
  int32_t n_eos;           /* 0 .. 16 */
  int32_t n_begin;         /* 0 .. SLAM_CONSTRAIN_MAX_BEGIN */
  int32_t n_seqs;          /* 0 .. SLAM_CONSTRAIN_MAX_SEQS */
  int32_t n_seq_tokens;    /* length of seq_tokens */
} SlamConstrainDesc;
int slam_constrain_scores(const float* logits, float* scores, int32_t B, int32_t vocab, const SlamConstrainDesc* desc,
                          const int64_t* prompt, const int32_t* prompt_len, const int64_t* new_tokens, int64_t new_stride,
                          const uint8_t* done, const int32_t* eos_ids, const int32_t* begin_ids, const int32_t* seq_tokens,
                          const int32_t* seq_offsets, slam_stream_t stream);

/* ---- the log-probability of the chosen token (what a second forward + log_softmax + gather would give) ----------------------
 * slam_token_logprobs needs no engine and runs right behind slam_sample_tokens on the same stream, on the same logits. For
 * row b, with x_i the RAW logit of token i (no banned mask, no temperature, no truncation; NaN counts as -inf and +inf as
 * FLT_MAX, the sampler's reading):
 *   finished && finished[b]:  out[b * out_stride + column] = 0.0f
 *   otherwise:                out[..] = x[tokens[b]] - (m + logf(S)), the model's own log-softmax (the quantity
 *                             sequence_logps sums); 0.0f when tokens[b] is outside [0, vocab); -inf when the row has no score
 *                             above -inf.
 *   then, when finished is given: finished[b] = done ? done[b] : 0.
 * With done = the sampler's flags, the EOS token itself gets its log-prob and the pads behind it get 0, with no torch op
 * between engine calls, also when pad_id is an EOS id.
 * m and S, in fp32: the row is cut into chunks of 2048 scores (the sampler's chunk). In chunk c, m_c = max x_i and
 * s_c = sum of expf(x_i - m_c) (0 when m_c = -inf) in this order: thread t of 256 adds the scores t, t + 256, t + 512, .. of
 * the chunk in that order starting from 0; the 64 lanes of a wave are combined by the xor butterfly v += v[lane ^ o] for
 * o = 32, 16, 8, 4, 2, 1; the four waves as ((w0 + w1) + w2) + w3. m = max_c m_c; S starts at 0 and takes, in chunk order
 * from 0, S = fmaf(s_c, expf(m_c - m), S) - ONE rounding per chunk, a fused multiply-add - with chunks of m_c = -inf skipped.
 * A row of one chunk has S = s_0 (one launch); longer rows take two launches through ws. The result depends on (the row, the token) alone - not on B, the row index, the row's alignment or the
 * launch shape - and is the same bits on every run: no floating-point atomics.
 * logits fp32 [B][vocab] (row stride vocab, 4-byte aligned); tokens int64 [B]; done, finished uint8 [B], nullable; out fp32;
 * ws: slam_token_logprobs_workspace_bytes(B, vocab) bytes, 8-byte aligned (host arithmetic: positive for valid arguments, 0
 * else). SLAM_EINVAL before any launch: logits, tokens, out or ws NULL; B <= 0 or B > 65535; vocab <= 0; logits not 4-byte
 * aligned; ws not 8-byte aligned; ws_bytes too small. */
size_t slam_token_logprobs_workspace_bytes(int32_t B, int32_t vocab);
int slam_token_logprobs(const float* logits, int32_t B, int32_t vocab, const int64_t* tokens, const uint8_t* done,
                        uint8_t* finished, float* out, int64_t out_stride, int32_t column, void* ws, size_t ws_bytes,
                        slam_stream_t stream);

/* ---- classifier-free guidance (HF's guidance_scale), both branches in one decode batch ---------------------------------------
 * slam_cfg_scores needs no engine and changes no engine state: slam_prefill, slam_kv_repeat and slam_decode_step take any row
 * count, and the guided layout is a convention of the caller. logits is fp32 [2 B][vocab] (row stride vocab): row b holds the
 * conditional scores x of sequence b, row B + b its unconditional scores y. scores is fp32 [B][vocab] and must not overlap
 * logits (slam_token_logprobs keeps reading the raw rows afterwards). With g = guidance_scale:
 *   reading      x_i and y_i are read as the sampler and slam_token_logprobs read a score: NaN counts as -inf, +inf as FLT_MAX.
 *   statistics   (m_x, S_x) of row b and (m_y, S_y) of row B + b are slam_token_logprobs' m and S (above): chunks of 2048 scores,
 *                256 threads striding, the xor butterfly, ((w0 + w1) + w2) + w3, chunks combined in chunk order by
 *                S = fmaf(s_c, expf(m_c - m), S). The two calls run the same device code.
 *   normalisers  L_x = m_x + logf(S_x), L_y = m_y + logf(S_y), in fp32.
 *   combination  a_i = x_i - L_x, u_i = y_i - L_y, d_i = a_i - u_i, scores[b][i] = (g * d_i) + u_i: transformers'
 *                guidance_scale * (scores - uncond) + uncond on the two log-softmaxes. Each of the three operations is rounded
 *                to fp32 on its own; none is contracted into a fused multiply-add.
 *   non-finite   (deviations: transformers produces NaN there) a_i = -inf gives -inf; u_i = -inf with a_i finite gives a_i; a
 *                row whose conditional scores are all -inf gives -inf throughout; a row whose unconditional scores are all
 *                -inf gives a_i throughout.
 * A row's result depends on its two input rows and g alone - not on B, the row index, the rows' alignment or the launch
 * shape - and is the same bits on every run: no floating-point atomics. Rows of one chunk take one launch; longer rows take
 * two: the per-chunk (m_c, s_c) of all 2 B rows into ws (slam_token_logprobs' first launch), then the finish. Grid
 * (chunks, B), as slam_constrain_scores. A block stages its chunk of both rows in LDS with 16-byte loads from each row's first
 * 16-byte boundary and stores with 16-byte accesses from the first 16-byte boundary of the scores row (every access is 16
 * bytes wide where the rows are equally aligned); 4-byte accesses at the ragged ends, so odd vocabularies are fine.
 * ws: slam_cfg_workspace_bytes(B, vocab) bytes, 8-byte aligned (host arithmetic: positive for valid arguments, 0 else); it is
 * required for rows of one chunk too.
 * SLAM_EINVAL before any launch or device dereference: logits, scores or ws NULL; B <= 0 or 2 B > 65535; vocab <= 0; a
 * non-finite guidance_scale; logits or scores not 4-byte aligned; ws not 8-byte aligned; ws_bytes too small; the ranges
 * logits[0 .. 2 B vocab) and scores[0 .. B vocab) overlapping.
 *
 * slam_cfg_mirror_tokens: next[B + b] = next[b] for b in 0 .. B-1 (int64, device memory, 8-byte aligned): the sampler writes
 * next[0 .. B) for the conditional rows and slam_decode_step reads next[0 .. 2 B), so a guided step under the engine sampler
 * still has no torch op between two engine calls. SLAM_EINVAL: next NULL or misaligned; B outside 1 .. 32767.
 * The guided step, in transformers' processor order (guidance first): slam_cfg_scores(logits -> scores),
 * slam_constrain_scores(in place on scores), slam_sample_tokens over the B rows of scores, slam_token_logprobs on the raw
 * conditional rows logits[0 .. B), slam_cfg_mirror_tokens, slam_decode_step over 2 B rows. */
size_t slam_cfg_workspace_bytes(int32_t B, int32_t vocab);
int slam_cfg_scores(const float* logits, int32_t B, int32_t vocab, float guidance_scale, float* scores, void* ws,
                    size_t ws_bytes, slam_stream_t stream);
int slam_cfg_mirror_tokens(int64_t* next, int32_t B, slam_stream_t stream);

/* loss.backward(): accumulates d(loss*grad_scale)/dparam into the bound fp32 gradient buffer.
 * bucket_layers = decoder layers per gradient bucket for the callback (<=0: one bucket). */
int slam_backward(SlamEngine* h, float grad_scale, int32_t bucket_layers, slam_bucket_cb cb, void* user,
                  slam_stream_t stream);
/* ---- engine-side gradient exchange (RCCL over xGMI) for a consumer without torch.distributed -----------------------------
 * What DistributedDataParallel does for the reference (/root/reference config/training_args/default.yaml:18, cli/train.py:51,61;
 * SURVEY.md §8a T10, §8b `slam_allreduce_grads_async`). One communicator per engine on the engine's device; RCCL is looked up at the
 * first call (dlopen of librccl.so.1 - the copy the process already has is reused), SLAM_EUNSUPPORTED when it is absent.
 *   rank 0: slam_comm_unique_id(id, 128) -> ship the 128 bytes to every rank -> each rank: slam_comm_init(h, id, rank, world)
 *   per step: slam_backward(h, scale, bucket_layers, cb, ...) with a callback that calls
 *             slam_allreduce_grads_async(h, offset, count, bf16, slam_bucket_stream(h) ? slam_bucket_stream(h) : stream)
 *             -> slam_comm_finish(h, stream) -> slam_grad_norm / slam_adamw_step on `stream`.
 * slam_allreduce_grads_async: grads[offset, offset + count) summed over the ranks (in place) on the engine's communication stream,
 * ordered after everything enqueued so far on `ready`; it returns at once. bf16_exchange = 1: the bf16 image bound by
 * slam_set_grad_image before that backward crosses the wire (half the bytes) and is widened back into the fp32 buffer.
 * slam_comm_finish: `stream` waits for every exchange issued since the last finish. */
#define SLAM_COMM_ID_BYTES 128
int slam_comm_unique_id(void* id_out, int32_t bytes);
int slam_comm_init(SlamEngine* h, const void* id, int32_t rank, int32_t world);
int slam_comm_destroy(SlamEngine* h);
int slam_allreduce_grads_async(SlamEngine* h, int64_t offset, int64_t count, int32_t bf16_exchange, slam_stream_t ready);
int slam_comm_finish(SlamEngine* h, slam_stream_t stream);
/* The reduce-scatter / all-gather form of the same exchange (what slamkit_amd's trainer runs as ddp_algo = "rs_ag"; SURVEY.md
 * §5 comm row, §8e): per bucket the ranks reduce-scatter the gradients - rank r ends up with the summed shard
 * [offset + r s, offset + (r + 1) s), s = count / world (count = world x a multiple of 8) - the optimizer runs on the owned shards
 * (slam_grad_sumsq_chunks + one all-reduce of the chunk sums, slam_adamw_range*), and the updated bf16 PARAMETERS are all-gathered:
 *   callback: slam_reduce_scatter_grads_async(h, offset, count, bf16, ready)      -> slam_comm_finish(h, stream)
 *   update of the owned shards on `stream`, then per bucket, lowest offsets first:
 *             slam_allgather_params_async(h, offset, count, stream)
 * The gather runs on the communication stream under the next forward, which waits for each bucket right before its first read
 * (the engine registers the wait itself - slam_add_param_wait is for consumers with their own communicator). */
int slam_reduce_scatter_grads_async(SlamEngine* h, int64_t offset, int64_t count, int32_t bf16_exchange, slam_stream_t ready);
int slam_allgather_params_async(SlamEngine* h, int64_t offset, int64_t count, slam_stream_t ready);
/* Valid inside a slam_bucket_cb call: the stream on which the reported range is complete - the consumer records its
 * "bucket ready" event THERE. NULL = the stream passed to slam_backward. With the weight-gradient stream on, the
 * intermediate buckets are complete on that engine-owned stream (which has also been ordered after the norm / bias
 * kernels of the range on `stream`), so `stream` itself never waits for the weight gradients at a bucket boundary. */
slam_stream_t slam_bucket_stream(SlamEngine* h);

/* Per-sequence log-likelihood sums of the last forward (UnitLM.log_likelihood :184-194 /
 * calc_nll, slamkit/utils/calculation_utils.py:5-29): ll_out, cnt_out fp32 [B] device. */
/* Modality-restricted scoring (UnitLM.log_likelihood(ignore_tokens=...), unit_lm.py:185-188): columns whose byte
 * in `mask` (device pointer to slam_padded_vocab(h) bytes, borrowed until reset with NULL) is non-zero are treated
 * as -inf by the loss of every following slam_forward; a target inside the mask gives an infinite row loss. */
int slam_set_logit_mask(SlamEngine* h, const uint8_t* mask);
int32_t slam_padded_vocab(SlamEngine* h);
int slam_seq_loglik(SlamEngine* h, const int64_t* labels, int32_t B, int32_t T, float* ll_out, float* cnt_out,
                    slam_stream_t stream);

/* Sequence-level objectives on top of the token log-likelihoods (preference optimisation, TRL DPOTrainer
 * behind /root/reference cli/preference_alignment_train.py:56-65): after a forward with labels and
 * num_items = 1 (so d loss/d logits holds softmax - onehot per valid token), multiply the rows of sequence b
 * by seq_coef[b] (fp32 [B] device) - e.g. +-beta*sigmoid(-x)/n for the sigmoid DPO loss - then slam_backward. */
int slam_scale_loss_rows(SlamEngine* h, const float* seq_coef, int32_t B, int32_t T, slam_stream_t stream);

/* Label smoothing of the training loss (HF TrainingArguments.label_smoothing_factor: transformers.trainer_pt_utils.LabelSmoother
 * with shift_labels). epsilon in [0, 1), else SLAM_EINVAL; it persists until changed and applies to the loss of every following
 * slam_forward / slam_forward_unpadded that is given labels. 0 (the default) launches the plain loss kernels: the bits of an
 * engine that never called this. With V = vocab_size (never the padded row length), p = softmax(z) and lse = logsumexp(z) over
 * the V real columns of a position whose target y is valid:
 *     nll_t = lse - z_y        smooth_t = lse - (1 / V) sum_v z_v        (= the mean over v of -log p_v)
 *     loss = ((1 - epsilon) sum_t nll_t + epsilon sum_t smooth_t) / denom
 *     d loss / d z_j = (p_j - (1 - epsilon) [j == y] - epsilon / V) / denom  for j < V, exactly 0 in the pad columns
 * denom as without smoothing: num_items when positive, else the number of valid targets. Smoothing runs inside the loss kernels'
 * own passes over the logits (no further read or write of a row). Summation order, fixed, so that equal inputs give equal bits:
 * sum_v z_v in fp32 - each thread its columns in ascending order, the lanes of a wave by the xor butterfly, the waves of a row's
 * block in wave order; the two sums over t in double, in the order the plain loss sums its rows, combined as written above.
 * The per-row values that slam_seq_loglik / slam_seq_loglik_unpadded read stay the PLAIN nll_t: after a smoothed forward they
 * return what they return after a plain one. Refused with SLAM_ESTATE: a forward with labels and epsilon > 0 while a logit
 * mask is set (modality-restricted scoring is a likelihood, not a training loss), and slam_scale_loss_rows /
 * slam_scale_loss_unpadded after a smoothed forward (sequence objectives are defined on the plain log-likelihood). */
int slam_set_label_smoothing(SlamEngine* h, float epsilon);

/* NEFTune (HF TrainingArguments.neftune_noise_alpha: transformers.integrations.neftune.neftune_post_forward_hook): uniform noise
 * on the input embeddings of a TRAINING forward, out = E[ids] + U(-mag, mag), mag = alpha / sqrt(T * H). alpha >= 0 and finite,
 * else SLAM_EINVAL with a message; 0 (the default) is off; alpha and seed (read as 64 unsigned bits) persist until changed. The
 * call adds no buffer: a bound workspace stays bound. The noise is drawn INSIDE the embedding gather of an armed forward - no
 * launch, no buffer and no pass over [M][H] more - and NOTHING IS STORED: it is an additive constant, so backward is unchanged,
 * and no "recompute" level re-runs the embedding launch (the residual streams are kept).
 *   generator  Philox4x32-10, key = (seed & 0xffffffff, seed >> 32), counter = (i8 & 0xffffffff, i8 >> 32, call, 0x4E454654),
 *              i8 = i >> 3, i = m * H + h the flat index of the element in the [M][H] layout that is launched. The last counter
 *              word is where "dropout_thr16" has 2 * layer + site: the two never draw the same bits under one seed;
 *   element    j = i & 7 takes r16 = (w[j >> 1] >> 16 (j & 1)) & 0xffff (the mapping of "adamw_sr" / "dropout_thr16");
 *   scale      s = (float)((double)alpha / sqrt((double)T * H) / 65536.0), on the host, once per forward: T of slam_forward, the
 *              padded width T of slam_forward_unpadded (HF sees [B, T]; a flattened packed batch is [1, M]);
 *   noise      t = 2 r16 - 65535 as a float (exact: an odd integer in [-65535, 65535]); n = t * s, ONE fp32 multiply rounded to
 *              nearest, never contracted into the add. 65536 levels symmetric about 0, |n| <= 65535 s < mag;
 *   output     Qwen2 / Qwen3: out = bf16(e + n), e the bf16 table entry as fp32; OPT: out = bf16((E + P) + n), the two fp32
 *              adds in this order (HF adds the noise to the token embedding before the positions: the same sum up to the
 *              order). One rounding to nearest-even. Ids outside [0, vocab) read row 0, as unarmed, and get noise.
 * Option "neftune_call_next" = 0 .. 2^32 - 1 (slam_set_option; anything else is SLAM_EINVAL, "out of range") arms the NEXT
 * slam_forward / slam_forward_unpadded and no other, with this call number, and resets itself; a forward that is refused uses
 * it up as well. Ignored while alpha is 0. A forward that was not armed launches the plain gather - the instruction stream of an
 * engine that never called this - and slam_prefill, slam_decode_step, the slam_extend family and every scoring path never draw
 * noise. Under slam_forward_unpadded the element index is the PACKED one (the "dropout_thr16" contract): a token's noise
 * differs from the padded run's. The noise depends on nothing else - not on the stream, the recompute level or the rank - so a
 * caller that numbers its forwards (optimizer step x accumulation steps + micro-batch) repeats a run exactly. */
int slam_set_neftune(SlamEngine* h, float alpha, int64_t seed);

/* ---- optimizer step: HF Trainer clip_grad_norm_ + torch AdamW --------------
 * norm_out: fp32 [2] device = {global grad norm, clip coefficient}.
 * Where the gradients are read from follows the last slam_backward: the fp32 buffer of slam_bind_params, or - after a
 * backward that ran under slam_set_option(h, "grad_final_next", 2) - the bf16 buffer given to slam_set_grad_image, which then
 * holds the ONLY copy of the step's final gradient values (the reference's own gradient precision: bf16 parameters have
 * bf16 .grad, /root/reference config/model/slam.yaml:9). After "grad_final_next" >= 1 slam_grad_norm adds the per-block sums
 * of squares that backward's final-value stores emitted, in launch / block order (the same bits every run), instead of
 * reading the buffer again. */
int slam_grad_norm(SlamEngine* h, float max_norm, float* norm_out, slam_stream_t stream);
int slam_adamw_step(SlamEngine* h, float* master_f32, float* exp_avg, float* exp_avg_sq, const float* norm_out,
                    double lr, double beta1, double beta2, double eps, double weight_decay, int32_t step,
                    int32_t zero_grad, slam_stream_t stream);
/* The Slam recipe's own optimizer precision (/root/reference config/model/slam.yaml:9 `torch_dtype: bfloat16`: bf16
 * parameters and bf16 Adam moments, torch.optim.AdamW(fused) semantics: fp32 arithmetic per element from the stored bf16
 * values, one rounding on the way back, no fp32 master copy). Updates the BOUND bf16 parameter buffer in place and
 * refreshes the transposed images; exp_avg / exp_avg_sq: bf16 [slam_param_count]. 16 B/param instead of 30. */
int slam_adamw_step_bf16(SlamEngine* h, void* exp_avg_bf16, void* exp_avg_sq_bf16, const float* norm_out, double lr,
                         double beta1, double beta2, double eps, double weight_decay, int32_t step, int32_t zero_grad,
                         slam_stream_t stream);
/* The middle precision: fp32 master weights, Adam moments STORED in bf16 (fp32 arithmetic per element, one rounding on the
 * way back): 22 B/param instead of 30. With transposed weight images bound, all three forms write those images from the
 * optimizer kernel itself (64 x 64 tiles through LDS) - there is no separate transpose pass after the update. */
int slam_adamw_step_bf16_moments(SlamEngine* h, float* master_f32, void* exp_avg_bf16, void* exp_avg_sq_bf16,
                                 const float* norm_out, double lr, double beta1, double beta2, double eps, double weight_decay,
                                 int32_t step, int32_t zero_grad, slam_stream_t stream);
/* ---- sharded optimizer step: the data-parallel "rs_ag" exchange (replaces torch DDP's all-reduce of
 * every gradient followed by N identical optimizer steps, /root/reference config/training_args/default.yaml:18 +
 * site-packages transformers/trainer.py) -------------------------------------------------------------------------------
 * Per gradient bucket the ranks reduce-scatter the gradients, each rank updates the 1/N shard it owns, and the bf16
 * parameters are all-gathered while the next forward already runs. The global gradient norm is defined on fixed chunks of
 * slam_grad_chunk_elems() consecutive elements of the flat buffer: slam_grad_sumsq_chunks fills chunk_sums[k] (fp32
 * [ceil(slam_param_count / chunk)], device) for the chunk-aligned range it is given - a rank fills the chunks of its own
 * shards and leaves zeros elsewhere, the arrays are summed over the ranks (exact: disjoint support), and
 * slam_grad_norm_from_chunks finishes {norm, clip coefficient} exactly as slam_grad_norm does for the whole buffer (which
 * computes the same chunk sums itself): the sharded and the replicated step clip with bit-identical coefficients. */
int64_t slam_grad_chunk_elems(void);
int slam_grad_sumsq_chunks(SlamEngine* h, int64_t offset, int64_t count, float* chunk_sums, slam_stream_t stream);
int slam_grad_norm_from_chunks(SlamEngine* h, const float* chunk_sums, float max_norm, float* norm_out, slam_stream_t stream);
/* slam_adamw_step on elements [offset, offset + count) only (multiples of 4; 8 for the bf16-state form): master / exp_avg /
 * exp_avg_sq point at THE RANGE'S first element (compact per-shard storage or base + offset of full-size buffers). Does not
 * refresh the transposed weight images: the next slam_backward does, after every pending parameter write has landed.
 * zero_grad != 0 (here and in slam_adamw_step*) clears the fp32 gradient buffer over exactly the updated elements, whichever buffer
 * the gradients were read from: after a "grad_final_next" = 2 backward the bf16 image keeps its values and the fp32 buffer is cleared. */
int slam_adamw_range(SlamEngine* h, int64_t offset, int64_t count, float* master_f32, float* exp_avg, float* exp_avg_sq,
                     const float* norm_out, double lr, double beta1, double beta2, double eps, double weight_decay,
                     int32_t step, int32_t zero_grad, slam_stream_t stream);
int slam_adamw_range_bf16_moments(SlamEngine* h, int64_t offset, int64_t count, float* master_f32, void* exp_avg_bf16,
                                  void* exp_avg_sq_bf16, const float* norm_out, double lr, double beta1, double beta2, double eps,
                                  double weight_decay, int32_t step, int32_t zero_grad, slam_stream_t stream);
int slam_adamw_range_bf16(SlamEngine* h, int64_t offset, int64_t count, void* exp_avg_bf16, void* exp_avg_sq_bf16,
                          const float* norm_out, double lr, double beta1, double beta2, double eps, double weight_decay,
                          int32_t step, int32_t zero_grad, slam_stream_t stream);
/* Which tensors weight_decay applies to. By default every element of the flat buffer is decayed (p *= 1 - lr * weight_decay).
 * HF Trainer.create_optimizer decays only the names get_decay_parameter_names returns - no bias, no LayerNorm / RMSNorm
 * parameter - so a reference run with weight_decay != 0 needs this mask (slamkit_amd: UnitLM.hf_decay_flags(),
 * training_args.weight_decay_rule = "hf"). decay: HOST array of n_tensors bytes in slam_tensor_info order, decay[i] == 0 =
 * tensor i is not decayed; n_tensors must equal slam_tensor_count (SLAM_EINVAL otherwise). decay == NULL clears the mask
 * (n_tensors is ignored) and restores uniform decay: the launches are then exactly those of an engine that never had one.
 * Host bookkeeping + one small synchronous upload of an engine-owned table (the merged element ranges of the no-decay
 * tensors; every tensor offset is a multiple of 8, so a kernel thread's 4 or 8 elements never straddle a bound). Legal any
 * time after create, outside stream capture; survives re-binding of parameters and workspace. Every optimizer entry point
 * honours it: slam_adamw_step* on the flat path, on the fused walk that writes the transposed images (decided per tensor on
 * the host: a no-decay tensor is launched with weight_decay = 0) and in the "overlap_adamw" chunks; slam_adamw_range*
 * wherever a shard cuts a tensor. A no-decay element goes through the same arithmetic with weight_decay = 0 (p * 1.0f is
 * exact), so a masked step equals, bit for bit, the unmasked step with the caller's weight_decay on the decayed tensors and
 * the unmasked step with weight_decay = 0 on the others - in every state precision and with "adamw_sr". */
int slam_set_decay_mask(SlamEngine* h, const uint8_t* decay, int32_t n_tensors);

/* ---- Adafactor: HF Trainer's optim = "adafactor" ------------------------------------------------------------------------
 * transformers.optimization.Adafactor as Trainer.get_optimizer_cls_and_kwargs builds it: scale_parameter = False, relative_step =
 * False, beta1 = None (no first moment), eps = (1e-30, 1e-3), clip_threshold = 1.0, decay_rate = -0.8; eps[1] and the
 * parameter's own RMS are unused when scale_parameter is off. Per HF parameter tensor at step t (1-based), in fp32:
 *   g = gradient * norm_out[1];  beta = 1 - t^decay_rate;  s = g^2 + eps1
 *   matrix [R][C]:  row[r] <- beta row[r] + (1 - beta) mean_c s[r][c];   col[c] <- beta col[c] + (1 - beta) mean_r s[r][c]
 *                   u[r][c] = g[r][c] rsqrt(row[r] / mean_r row) rsqrt(col[c])
 *   vector:         v <- beta v + (1 - beta) s;   u = g rsqrt(v)
 *   d = max(1, sqrt(mean u^2) / clip_threshold);   p <- p - weight_decay lr p;   p <- p - lr u / d
 * The reductions are per HF tensor, and HF's tensors are not the engine's (wqkv = q | k | v, bqkv likewise, wgu = gate / up in
 * interleaved 32-row groups, the embedding padded to 512-row multiples): the caller describes them once.
 *
 * SlamAdafactorSegment = one HF parameter laid over the flat buffer: `offset` (elements) of its first row - for pattern 1 / 2
 * of the engine tensor that holds it -, HF `rows` x `cols`, `factored` (1: a matrix with row and column factors; 0: a vector,
 * rows = 1 and cols = its length) and the row `pattern`: 0 = row r is the r-th row of cols elements behind `offset`; 1 / 2 =
 * "groups of 32 rows every 64" with phase 0 / 32: row r is row (r / 32) 64 + phase + r % 32 behind `offset` (rows % 32 == 0).
 *
 * slam_adafactor_set_segments: validates and uploads the table (host bookkeeping + one small synchronous upload; outside stream
 *   capture). SLAM_EINVAL with a message: n < 1, a NULL table, rows or cols < 1, a vector with rows != 1, an unknown pattern or
 *   pattern rows that are no multiple of 32, offset or cols not a multiple of 8, a segment that leaves [0, slam_param_count), two
 *   segments that share an element. segs == NULL with n == 0 clears the table. The table survives re-binding of parameters and
 *   workspaces, like the decay mask. Elements that no segment covers (the embedding's pad rows) are never written by a step.
 * slam_adafactor_sizes: state_floats = the length of the caller's fp32 state buffer: per segment, in table order and without
 *   gaps, rows + cols floats (the row factors, then the column factors) when factored, cols when not; zeros before step 1.
 *   workspace_bytes = the bytes slam_adafactor_bind_workspace needs. SLAM_ESTATE without a table.
 * slam_adafactor_bind_workspace: caller-owned device memory, 16-byte aligned, at least workspace_bytes (SLAM_ENOMEM when
 *   shorter); NULL unbinds. Nothing beyond workspace_bytes is touched; the contents need not survive between steps.
 *
 * slam_adafactor_step: one update of every segment. master_f32 == NULL is the recipe's precision: the bound bf16 parameters are
 *   the only copy - read, updated in fp32 and rounded once on the way back; otherwise the fp32 master is updated and the bf16
 *   copy written from it. state_f32 is never rounded. The gradients are read where the last backward left them (the fp32 buffer,
 *   or the bf16 image after "grad_final_next" = 2); norm_out (nullable) is slam_grad_norm's output, whose [1] scales them.
 *   weight_decay honours slam_set_decay_mask per engine tensor (every HF part of a fused tensor has one class): a masked step
 *   equals, bit for bit, the unmasked step on the decayed segments and the weight_decay = 0 step on the others. zero_grad != 0
 *   clears the whole fp32 gradient buffer behind the update, whichever buffer the gradients were read from. The transposed
 *   weight images are refreshed as after slam_adamw_step. "adamw_sr" = 1: with master_f32 == NULL the stored bf16 parameter is
 *   the stochastic rounding of the fp32 result - array 0 of slam_op_sr_round_bf16, keyed on ("adamw_sr_seed", step, flat index);
 *   with a master the option does nothing.
 *   Six launches for the whole model (+ the image refresh), blocks finding their segment through the table; no atomics. Every
 *   sum runs in an order fixed by the segment's shape - tiles of 256 rows x 256 columns; the orders are listed at the top of
 *   csrc/adafactor.hip - so a step gives the same bits on every run, with zero_grad 0 or 1, and from either gradient buffer
 *   given equal values.
 *   Refused with a message: no segment table or no bound workspace (SLAM_ESTATE); "overlap_adamw" on (SLAM_ESTATE: the
 *   overlapped chunks belong to AdamW); state_f32 NULL or step < 1 (SLAM_EINVAL). There is no ranged form: a shard of the flat
 *   buffer cuts rows and columns. */
typedef struct SlamAdafactorSegment {
  int64_t offset;
  int32_t rows, cols;
  int32_t factored;
  int32_t pattern;
} SlamAdafactorSegment;
int slam_adafactor_set_segments(SlamEngine* h, const SlamAdafactorSegment* segs, int32_t n);
int slam_adafactor_sizes(SlamEngine* h, int64_t* state_floats, size_t* workspace_bytes);
int slam_adafactor_bind_workspace(SlamEngine* h, void* workspace, size_t bytes);
int slam_adafactor_step(SlamEngine* h, float* master_f32, float* state_f32, const float* norm_out, double lr, double eps1,
                        double clip_threshold, double decay_rate, double weight_decay, int32_t step, int32_t zero_grad,
                        slam_stream_t stream);

/* ---- Muon: optim = "muon" ----------------------------------------------------------------------------------------------------
 * torch.optim.Muon as torch 2.10 defines it (torch/optim/_muon.py: _single_tensor_muon, _zeropower_via_newtonschulz), per HF
 * parameter tensor, for the 2-D weights of the decoder layers (q/k/v/o and the MLP matrices); everything else - embeddings, an
 * untied head, norm weights, biases - stays with AdamW, which the caller runs through slam_adamw_range* over the runs of the
 * flat buffer that no Muon matrix covers.
 *
 * For an HF matrix W [rows][cols] with momentum buffer B (fp32, rows * cols floats in HF row-major order, zeros before step 1):
 *   prepare  g = gradient * norm_out[1];  B <- mu B + (1 - mu) g;  U = (1 - mu) g + mu B (nesterov) or B;  X = bf16(U).
 *            fp32, every multiplication and addition rounded by itself; mu = (float)momentum, 1 - mu = (float)(1.0 - momentum).
 *   pack     X is stored [n][m], n = min(rows, cols), m = max(rows, cols): transposed when rows > cols.
 *   norm     s = sum of x^2 over bf16 X in fp32 (order: csrc/muon.hip), nrm = max(bf16(sqrtf(s)), bf16(eps)): torch's norm of a
 *            bf16 tensor is rounded to bf16 before the clamp;  X <- bf16(X / nrm), a correctly rounded fp32 division.
 *   iterate  ns_steps times:  A = bf16(X X^T);  P = bf16(b A + c (A A));  X <- bf16(a X + P X).  Every product is accumulated in
 *            fp32 by v_mfma_f32_16x16x32_bf16 over the contraction index in ascending 32-deep steps and rounded to bf16 once,
 *            after the epilogue fmaf(beta, R, alpha * acc) (alpha * acc alone when there is no R). A and P are symmetric to the
 *            bit: only the 128 x 128 tiles on or below the diagonal are computed and an off-diagonal tile is stored twice.
 *   apply    O = X (transposed back when rows > cols); in fp32, each operation rounded by itself:
 *            p <- p * (float)(1.0 - lr weight_decay);  p <- p - (float)(lr ratio) * O, ratio (double) = 1 for adjust_lr 0 (none),
 *            sqrt(max(1, rows / cols)) for 1 ("original"), 0.2 sqrt(max(rows, cols)) for 2 ("match_rms_adamw").
 *            master_f32 given: the master is updated and the bf16 parameter written from it; NULL: the bf16 parameter is read,
 *            updated and rounded once - with "adamw_sr" = 1 stochastically, array 0 of slam_op_sr_round_bf16 keyed on
 *            ("adamw_sr_seed", step, flat index), as slam_adafactor_step does. slam_set_decay_mask is honoured per segment.
 * No atomics anywhere: a step gives the same bits on every run, with zero_grad 0 or 1 and from either gradient buffer given
 * equal values.
 *
 * SlamMuonSegment = one Muon matrix over the flat buffer; offset / rows / cols / pattern as SlamAdafactorSegment's.
 * slam_muon_set_segments: validates and uploads the table (one small synchronous upload; outside stream capture). SLAM_EINVAL
 *   with a message: n < 1, a NULL table, rows or cols < 1, a segment that is not a matrix (rows or cols < 2), an unknown pattern
 *   or pattern rows that are no multiple of 32, offset, rows or cols not a multiple of 8, a segment that leaves [0,
 *   slam_param_count), two segments that share an element, more than 64 distinct shapes. NULL with n == 0 clears the table.
 *   Segments of equal (rows, cols) form a shape class; the classes are numbered in order of first appearance.
 * slam_muon_sizes: momentum_floats = the length of the caller's fp32 momentum buffer (the segments in table order, without gaps);
 *   workspace_bytes for slam_muon_bind_workspace. SLAM_ESTATE without a table.
 * slam_muon_bind_workspace: caller-owned device memory, 256-byte aligned, at least workspace_bytes (SLAM_ENOMEM when shorter);
 *   NULL unbinds. Nothing beyond workspace_bytes is touched; the contents need not survive between steps. The workspace holds
 *   the packed bf16 image of EVERY Muon matrix (2 bytes per Muon element: prepare and apply are one launch each for the whole
 *   model) and, sized by the largest class because the classes are iterated one after another, a second packed image and the two
 *   Gram buffers, plus one float per 64 x 64 tile. Slam-358M: 716 MB + 418 MB + 2 x 77 MB + 0.3 MB.
 * slam_muon_class_count / slam_muon_class_info: the shape classes and where the workspace holds them: the class's `count` packed
 *   [n][m] matrices lie at x_byte_offset at the stride n * m elements, their sum-of-squares partials (`parts` floats a matrix)
 *   at part_byte_offset.
 *
 * slam_muon_step: prepare (one launch) - per class: norm and scale (one launch), 3 ns_steps product launches over the class as
 *   one batch - apply (one launch), all on `stream`: 2 + classes (1 + 3 ns_steps) launches whatever the number of layers. Only
 *   Muon elements are written. zero_grad != 0 clears the Muon elements of the fp32 gradient buffer (the AdamW ranges clear
 *   theirs). `step` (>= 1) only keys the stochastic rounding. The transposed weight images are left stale as after
 *   slam_adamw_range*: the next slam_backward, or slam_refresh_transposed, refreshes them.
 *   Refused with a message: "overlap_adamw" on, no segment table or no bound workspace (SLAM_ESTATE); ns_steps outside 1 .. 16,
 *   momentum_f32 NULL, momentum outside [0, 1), adjust_lr outside 0 .. 2, step < 1 (SLAM_EINVAL). There is no ranged form.
 * The single-op doors (tests): slam_op_muon_prepare (momentum update, packed X and partials into the workspace), slam_op_muon_ns
 *   (orthogonalise `batch` packed [n][m] matrices, n <= m, multiples of 8, in place at `stride` elements; partials == NULL: the
 *   sums of squares are taken here, over 8192-element chunks; ws: slam_op_muon_ns_workspace bytes, 256-byte aligned) and
 *   slam_op_muon_apply (o_packed == NULL: the workspace's packed image). slam_muon_step equals slam_op_muon_prepare, slam_op_muon_ns
 *   per class on the workspace with prepare's partials, slam_op_muon_apply, bit for bit. slam_op_muon_syrk: C[i] = beta R[i] +
 *   alpha X[i] X[i]^T; slam_op_muon_mm: Y[i] = beta R[i] + alpha P[i] X[i] (P [n][n], X [n][m]); R nullable; strides in elements,
 *   multiples of 8; R and the output share the output's row length. */
typedef struct SlamMuonSegment {
  int64_t offset;
  int32_t rows, cols;
  int32_t pattern;
  int32_t reserved;
} SlamMuonSegment;
typedef struct SlamMuonClass {
  int32_t rows, cols, n, m, count, parts;
  int64_t x_byte_offset, part_byte_offset;
} SlamMuonClass;
int slam_muon_set_segments(SlamEngine* h, const SlamMuonSegment* segs, int32_t n);
int slam_muon_sizes(SlamEngine* h, int64_t* momentum_floats, size_t* workspace_bytes);
int slam_muon_bind_workspace(SlamEngine* h, void* workspace, size_t bytes);
int32_t slam_muon_class_count(SlamEngine* h);
int slam_muon_class_info(SlamEngine* h, int32_t i, SlamMuonClass* out);
int slam_muon_step(SlamEngine* h, float* master_f32, float* momentum_f32, const float* norm_out, double lr, double weight_decay,
                   double momentum, int32_t nesterov, int32_t ns_steps, double a, double b, double c, double eps, int32_t adjust_lr,
                   int32_t step, int32_t zero_grad, slam_stream_t stream);
int slam_op_muon_prepare(SlamEngine* h, float* momentum_f32, const float* norm_out, double momentum, int32_t nesterov,
                         int32_t zero_grad, slam_stream_t stream);
size_t slam_op_muon_ns_workspace(int32_t batch, int32_t n, int32_t m);
int slam_op_muon_ns(void* x_bf16, int32_t batch, int32_t n, int32_t m, int64_t stride, const float* partials, int32_t parts,
                    int32_t ns_steps, double a, double b, double c, double eps, void* ws, size_t ws_bytes, slam_stream_t stream);
int slam_op_muon_apply(SlamEngine* h, float* master_f32, const void* o_packed_bf16, double lr, double weight_decay,
                       int32_t adjust_lr, int32_t step, slam_stream_t stream);
int slam_op_muon_syrk(const void* x, const void* r, void* c, int32_t batch, int32_t n, int32_t m, int64_t stride_x, int64_t stride_r,
                      int64_t stride_c, float alpha, float beta, slam_stream_t stream);
int slam_op_muon_mm(const void* p, const void* x, const void* r, void* y, int32_t batch, int32_t n, int32_t m, int64_t stride_p,
                    int64_t stride_x, int64_t stride_r, int64_t stride_y, float alpha, float beta, slam_stream_t stream);
/* Another stream (the all-gather of a parameter bucket) is still writing the bound bf16 parameters in [offset, offset +
 * count); `event` (hipEvent_t, owned by the caller, alive until the next forward was enqueued) is recorded behind that
 * write. The next slam_forward waits for it right before its first read of the range - layer by layer, so the gather of
 * the later layers runs under the first layers' kernels; every other entry point that touches parameters waits for all
 * of them first. slam_param_wait_ms: total stall of the caller's stream in those waits since the last query (host-
 * synchronising: logging only; the waits are bracketed by timing events only while slam_set_option(h, "time_param_waits", 1)).
 * After a ranged update the transposed weight images are rebuilt at the start of the next slam_backward. */
int slam_add_param_wait(SlamEngine* h, int64_t offset, int64_t count, void* event);
int slam_param_wait_ms(SlamEngine* h, float* total_ms);
/* Waits since the last call that could NOT be bracketed by timing events (the event pool - 2048 pairs, completed pairs are
 * folded into the running total and reused - was full of pairs still in flight): 0 means slam_param_wait_ms is complete. */
int slam_param_wait_untimed(SlamEngine* h, int64_t* n);
/* Measurement hook of bench.py's `roofline`: with slam_set_option(h, "time_gateup", 1) every forward brackets the gate|up
 * projection launch of each layer (the dominant kernel: fused SwiGLU GEMM, 2 M (2I) H flop) with two timing events on the
 * caller's stream; slam_gateup_launch_ms writes the n_layers durations of the last forward (ms; host-synchronising).
 * It times the launch where it runs - inside the step, between its neighbours - which is what rocprofv3 reports for the
 * same launches. No reference counterpart (the reference has no kernel-level timing). */
int slam_gateup_launch_ms(SlamEngine* h, float* ms_out, int32_t n);
/* The same hook for EVERY launch family of the step: with slam_set_option(h, "time_families", 1) slam_forward and
 * slam_backward bracket each launch (projection / attention / norm / loss kernels, the dgrad chain, and the weight-gradient
 * GEMMs on the engine's side stream(s)) with a timing-event pair on the stream the launch goes to. slam_family_ms writes up
 * to `capacity` (family id, ms) records of the last forward + backward in launch order and their number (host-synchronising);
 * slam_family_name maps an id to its name ("gateup_fwd", "wgu_wgrad", ... ; NULL past the last id). A record is the time
 * between the launch's stream reaching it and the launch completing - beside whatever the other stream runs - i.e. the
 * in-step duration a kernel trace reports, not a stand-alone time. Two more packets per launch: measurement steps only.
 * No reference counterpart. */
int slam_family_ms(SlamEngine* h, int32_t* family_out, float* ms_out, int32_t capacity, int32_t* count_out);
const char* slam_family_name(int32_t family);
/* Data-parallel gradient exchange in bf16 (replaces the dtype conversion torch DDP never needs because the reference's
 * gradients ARE bf16: /root/reference config/model/slam.yaml:9 with config/training_args/default.yaml:18): pack
 * grads[offset, offset + count) (fp32) into a bf16 communication buffer (round-to-nearest-even) / widen a reduced bf16 range
 * back into the fp32 gradient buffer. offset and count are multiples of 4; dst / src point at the range's first element. */
int slam_pack_grads_bf16(SlamEngine* h, int64_t offset, int64_t count, void* dst_bf16, slam_stream_t stream);
/* ... or no pack pass at all: grads_bf16 = a bf16 buffer of slam_param_count() elements (NULL = off). The NEXT slam_backward
 * stores every FINAL gradient value there as well, rounded to nearest even, from the kernels that store the fp32 value (weight-
 * gradient tile epilogues, slab reduces, norm / bias finish) - bit-identical to slam_pack_grads_bf16 over the same range, for
 * 2 B/param of extra stores instead of a 6 B/param pass beside a backward that has no idle bandwidth. A range reported through
 * slam_bucket_cb is complete in the image as well. Consumed by that one backward (the last micro-batch of a step). */
int slam_set_grad_image(SlamEngine* h, void* grads_bf16);
int slam_unpack_grads_bf16(SlamEngine* h, int64_t offset, int64_t count, const void* src_bf16, slam_stream_t stream);
/* With slam_set_option(h, "overlap_adamw", 1), slam_adamw_step returns after forking the update onto an engine-owned side
 * stream in per-layer chunks; the next slam_forward waits for chunk l right before layer l and every other entry point
 * joins first. slam_join makes `stream` wait for a pending update before the caller touches the parameter, gradient or
 * optimizer buffers itself (checkpointing, logging). */
int slam_join(SlamEngine* h, slam_stream_t stream);
int slam_zero_grads(SlamEngine* h, slam_stream_t stream);
int slam_cast_params(SlamEngine* h, const float* master_f32, slam_stream_t stream); /* fp32 -> bound bf16 */

/* ---- tuning knobs ---------------------------------------------------------------------------*/
/* Tuning / mode switches. "attn_jq" / "attn_kw" (1 or 2: 16-row fragments per wave in the attention dQ / dK-dV kernels), "attn_nch" (1..4 query-range
 * chunks per key tile), "attn_prio" (wave priority by block length); with h = NULL they set the process default used by the
 * single-op entry points. "bwd_wgrad_cus" = N > 0: the weight-gradient stream is created with a CU mask of N CUs (a BLOCKING
 * stream: run the step on a non-default stream then). "grad_overwrite_next" = 1: the next slam_backward stores the gradients instead of adding to
 * them (first micro-batch of an optimizer step; no zeroing pass needed), then resets itself. "grad_final_next" = 1 | 2: the next
 * slam_backward is the LAST of its optimizer step (HF Trainer: the micro-batch on which `sync_gradients` is true) - every kernel
 * that stores a final gradient value also emits its block's sum of squares for slam_grad_norm; with 2 the final values are
 * stored ONLY as bf16 into the slam_set_grad_image buffer (earlier micro-batches keep accumulating in fp32) and slam_grad_norm /
 * slam_adamw_step* read them there; resets itself. The partial sums are not emitted by a backward that reports buckets to a callback
 * (data parallel: the clip needs the norm of the EXCHANGED gradients - chunk sums after the exchange) nor under
 * "grad_norm_partials" = 0 (slam_grad_norm then always runs the chunked pass, over whichever buffer holds the gradients). "bwd_wgrad_stream" (default
 * 1): slam_backward enqueues the weight-gradient GEMMs on an engine-owned second stream, ordered by events against the
 * dgrad chain on `stream`; `stream` is joined with it before slam_backward returns control of the gradient buffer (every
 * reported bucket range, and the end of the call). "overlap_adamw", "fuse_swiglu", "fuse_dswiglu", "gemm_256",
 * "gemm_256_dswiglu", "gemm_256_persist", "gemm_tn224", "gemm_tn_balanced", "gemm_group_rows" select kernels.
 *
 * "recompute" = 0 | 1 | 2 (default 0; anything else is SLAM_EINVAL, "out of range"): activation recomputation in backward -
 * gradient checkpointing (the reference's `supports_gradient_checkpointing`, HF TrainingArguments.gradient_checkpointing).
 * Results are bit-identical at every level: backward re-runs the forward's own launches on the forward's own inputs.
 *   0  every layer keeps hmid, x1, x2, qkv, o, gu, act, rstd1, rstd2, lse (OPT: + mu1, mu2; Qwen3: + the raw q|k columns and
 *      the heads' rstd) from forward to backward.
 *   1  selective: every layer keeps hmid, qkv, o, gu, the row statistics and lse; x1, x2 and act live in min(n_layers, 3)
 *      shared slots (layer l uses slot l mod 3) and slam_backward rebuilds them before layer l's weight gradients read them:
 *      x1 from the residual stream, x2 from hmid, act from gu (with "fuse_swiglu" the fused gate|up launch is re-run, since its
 *      act comes from fp32 accumulators that gu no longer holds). OPT (arch 1) stores no fc1 pre-activation - its act is the
 *      post-ReLU value and gu holds d(act) - so there level 1 shares x1 and x2 only and act stays per layer.
 *   2  full: every layer keeps only its residual stream; all of the above live in the shared slots and slam_backward re-runs
 *      layer l's forward launches (all but the down projection / fc2) from the residual stream right before the layer's backward,
 *      on `stream`. slam_prefill then scatters each layer's K / V into the cache inside the layer loop.
 * The workspace layout depends on the level (slam_workspace_bytes answers for the current one). CHANGING the level while a
 * workspace is bound unbinds it: slam_forward, slam_prefill, slam_decode_step and slam_backward return SLAM_ESTATE until
 * slam_bind_workspace is called again. Under "time_families" the re-run launches are recorded under the forward families'
 * ids (norm_fwd, qkv_fwd, ...), inside the backward part of the record list; "time_gateup" does not time them.
 *
 * "adamw_sr" = 0 | 1 (default 0; anything else is SLAM_EINVAL, "out of range"): stochastic rounding of the bf16 optimizer state.
 * Round-to-nearest drops every update below half an ulp of the stored value, which at a small learning rate is most of them;
 * with 1, every fp32 -> bf16 store of STATE adds 16 uniform random bits below the kept mantissa and truncates, so the stored
 * value is right on average (exact bf16 values never move; inf / NaN convert as before). Rounded that way:
 *   slam_adamw_step_bf16 / slam_adamw_range_bf16          p, m and v (the bf16 parameters are the state);
 *   slam_adamw_step_bf16_moments / slam_adamw_range_bf16_moments   m and v (the bf16 working copy of the fp32 master keeps
 *                                                          round-to-nearest: the master holds the precision);
 *   slam_adamw_step / slam_adamw_range (fp32 state)        nothing - the option is ignored there.
 * A transposed weight image carries the same rounded value as the row-major parameter. The generator is stateless
 * (Philox4x32-10): key = (seed & 0xffffffff, seed >> 32), counter = (i8 & 0xffffffff, i8 >> 32, step, s) with i8 = the
 * element's index in the flat parameter buffer >> 3, `step` the one the entry point is passed and s = 0 / 1 / 2 for p / m / v;
 * element j = index & 7 takes bits (w[j >> 1] >> 16 (j & 1)) & 0xffff of the four output words. Hence the result does not
 * depend on the kernel form ("fuse_adamw_t", the range entry points, how a sharded update splits the buffer), the stream or
 * the rank, and a run resumed at step k repeats the uninterrupted one. With 0 every bit is what it was without the option.
 * "adamw_sr_seed" = any int64 (default 0): the seed, read as 64 unsigned bits.
 *
 * "dropout_thr16" = 0 .. 65535 (default 0; anything else is SLAM_EINVAL, "out of range"; non-zero on a Qwen2 engine, arch 0, is
 * SLAM_EINVAL too): residual dropout of the OPT family (HF OPTDecoderLayer, `config.dropout`): behind out_proj (site 0) and
 * behind fc2 (site 1) of every layer, before the residual add. thr = round(p * 65536); q = thr / 65536 is the effective drop
 * probability and scale = 1 / (1 - q), in fp32. NOTHING IS STORED: forward, backward and recomputation draw the mask again.
 *   generator  Philox4x32-10, key = (seed & 0xffffffff, seed >> 32), counter = (i8 & 0xffffffff, i8 >> 32, call,
 *              2 * layer + site), i8 = (m * H + n) >> 3 with m the token's row in the [B * T] layout slam_forward is given
 *              (padding rows included) and n the hidden column;
 *   element    j = (m * H + n) & 7 takes r16 = (w[j >> 1] >> 16 (j & 1)) & 0xffff of the four output words (the mapping of
 *              "adamw_sr"); it is DROPPED iff r16 < thr;
 *   forward    out = bf16(resid + (keep ? y * scale : 0)): fp32 arithmetic, one rounding; y is the projection's bf16 output
 *              with its bias; a dropped element is resid itself;
 *   backward   d y = keep ? d out * scale : 0 (rounded to bf16 once, like every gradient between two kernels); the residual
 *              branch and the LayerNorm backward above it keep the unmasked d out.
 * The workspace layout depends only on whether the value is non-zero: at 0 slam_workspace_bytes answers what it answered
 * without the option, otherwise four [max_tokens][hidden] bf16 buffers more (the masked gradients of two layers in flight).
 * Changing between zero and non-zero while a workspace is bound unbinds it, exactly as "recompute" does; changing between two
 * non-zero values does not. A backward always uses the threshold, seed and call its own forward ran with.
 * "dropout_seed" = any int64 (default 0): the seed, read as 64 unsigned bits.
 * "dropout_call_next" = 0 .. 2^32 - 1: arms dropout for the NEXT slam_forward only, with this call number, and resets itself
 * (a forward that is refused uses it up as well). That forward remembers (thr, seed, call) for its own slam_backward, the
 * re-run launches of "recompute" included. A forward that was not armed applies no dropout - evaluation, scoring,
 * slam_prefill and slam_decode_step never see it - and its launches are those of an engine without the option. Ignored while
 * "dropout_thr16" is 0. The mask depends on nothing else: not on the stream, the recompute level, "bwd_wgrad_stream" or the
 * rank, so a caller that numbers its forwards (optimizer step x accumulation steps + micro-batch) repeats a run exactly. */
int slam_set_option(SlamEngine* h, const char* key, int64_t value);

/* ---- single-op entry points (parity tests call each kernel through the ABI) -------------------*/
int slam_op_gemm_nt(const void* X, const void* W, void* Y, const void* bias, const void* resid, int M, int N, int K,
                    int use_glds, slam_stream_t s);
/* gate|up projection with the SwiGLU product fused into the epilogue (W rows in 32-row gate/up blocks):
 * Y[M,N] = X W^T and act[M,N/2] = silu(gate) * up. The dominant kernel of the step (bench.py roofline). */
int slam_op_gemm_nt_swiglu(const void* X, const void* W, void* Y, void* act, int M, int N, int K, slam_stream_t s);
/* down-projection dgrad with the SwiGLU backward fused into the epilogue: d(act)[M,I] = dY[M,H] Wt[I,H]^T never leaves the
 * registers; gu[M,2I] (gate|up pre-activations, 32-column gate/up blocks) is rewritten in place with d(gate|up). */
int slam_op_gemm_nt_dswiglu(const void* dY, const void* Wt, void* gu, int M, int I, int H, slam_stream_t s);
int slam_op_gemm_nn(const void* dY, const void* W, void* dX, const void* resid, int M, int N, int K, slam_stream_t s);
size_t slam_op_gemm_tn_workspace(int M, int N, int K);
int slam_op_gemm_tn(const void* dY, const void* X, float* dW, int accumulate, int M, int N, int K, float* ws,
                    slam_stream_t s);
/* the same weight-gradient GEMM, also writing the bf16 image of every final dW value (slam_set_grad_image's mechanism);
 * background != 0 selects the plans slam_backward uses on its weight-gradient stream */
int slam_op_gemm_tn_image(const void* dY, const void* X, float* dW, void* dW_bf16, int accumulate, int M, int N, int K,
                          float* ws, int background, slam_stream_t s);
/* decode-time projection Y[M,N] = X[M,K] W[N,K]^T (+bias[N]) (+resid[M,N]) for small M (the weight-streaming kernel of
 * slam_decode_step): Y is fp32 when y_f32, else bf16; K a multiple of 8. ws: fp32 split-K partials,
 * slam_op_gemm_skinny_workspace(M, N, K) bytes for the full split (less: fewer splits). Bit-identical run to run. */
size_t slam_op_gemm_skinny_workspace(int M, int N, int K);
int slam_op_gemm_skinny(const void* X, const void* W, void* Y, int y_f32, const void* bias, const void* resid, int M, int N, int K,
                        float* ws, size_t ws_bytes, slam_stream_t s);
/* The FP8 weight stream of slam_quantize_decode_w8 on one matrix (the rule and the storage are stated there). K % 64 == 0, W
 * and codes 16-byte aligned, else SLAM_EINVAL. One allocation of slam_op_w8_bytes(N, K) holds the codes at offset 0 and the
 * int8 exponents at slam_op_w8_exps_offset(N, K) (both 0 for a refused K); the calls take the two pointers.
 * slam_op_quantize_rows_fp8: codes and exponents from W bf16 [N][K], and W rewritten in place with Wdq.
 * slam_op_dequantize_rows_fp8: W bf16 [N][K] row-major = Wdq from codes and exponents.
 * slam_op_gemm_skinny_w8: slam_op_gemm_skinny with codes + exponents in place of W; the bits of
 * slam_op_gemm_skinny(X, Wdq, ..) with the same workspace size. */
size_t slam_op_w8_bytes(int N, int K);
size_t slam_op_w8_exps_offset(int N, int K);
int slam_op_quantize_rows_fp8(void* W, void* codes, void* exps, int N, int K, slam_stream_t s);
int slam_op_dequantize_rows_fp8(const void* codes, const void* exps, void* W, int N, int K, slam_stream_t s);
int slam_op_gemm_skinny_w8(const void* X, const void* codes, const void* exps, void* Y, int y_f32, const void* bias,
                           const void* resid, int M, int N, int K, float* ws, size_t ws_bytes, slam_stream_t s);
/* LM head fused with the row statistics, alone (the hot path of slam_extend_score). X bf16 [M][K] (K % 8 == 0), W bf16 [V][K],
 * both 16-byte aligned. x_i = the fp32 accumulator of v_mfma_f32_16x16x32_bf16 for row m against vocabulary row i, K taken
 * in ascending steps of 32 (a last partial step is zero-filled): its order depends on K alone. x_i is never rounded to bf16
 * and never stored as an [M][V] array. Each score is read as the sampler reads it: NaN counts as -inf, +inf as FLT_MAX; a
 * column i with colmask[i] != 0 (colmask: nullable, uint8, at least V bytes) counts as -inf.
 *   lp[m]      x_target - (m + logf(S)) for target = targets[m] (int64 [M]); 0.0f when the target is outside [0, V) (-100: no
 *              target); -inf when the target is masked or the row has no score above -inf.
 *   argmax[m]  (int64 [M], nullable) the id of the largest x_i, the LOWEST id among equals; -1 when no score is above -inf.
 * m and S, in fp32. The vocabulary is cut into chunks of SLAM_SCORE_CHUNK = 512 columns; the width depends on nothing else.
 * A chunk is 8 groups of 64 consecutive columns. In a group, with m_g = max x_i and e_i = expf(x_i - m_g): for j = 0 .. 15,
 * a_j = (((0 + e_j) + e_{16+j}) + e_{32+j}) + e_{48+j} over the group's columns j, 16 + j, 32 + j, 48 + j (a column at or
 * beyond V, or masked, has e = 0); the sixteen a_j are summed by the xor butterfly a_j += a_{j ^ o} for o = 8, 4, 2, 1, which
 * gives s_g (0 when m_g = -inf). The groups of a chunk are combined in group order, m_c = max m_g, s_c starting at 0 and
 * taking s_c = fmaf(s_g, expf(m_g - m_c), s_c) with groups of m_g = -inf skipped. Each chunk yields (m_c, s_c, best value,
 * best id); the chunks are combined in chunk order the same way, m = max m_c; S = fmaf(s_c, expf(m_c - m), S), skipping chunks
 * of m_c = -inf - one rounding per part. The best id moves to a later group / chunk only on a strictly larger value.
 * No floating-point atomics: the chunk partials go through ws and a SECOND launch merges them in chunk order. A row's result
 * depends on (its X row, W, its target, the mask) alone - not on M, the row's index or the grid - and is the same bits on
 * every run. Tail rows and tail columns are never read out of bounds.
 * ws: slam_op_score_rows_workspace(M, V) bytes of device memory, 16-byte aligned (host arithmetic; 0 for M or V outside the ranges below).
 * SLAM_EINVAL before any launch: X, W, targets, lp or ws NULL; M <= 0 or M > 33554431; V <= 0 or V > 33553920 (65535 chunks); K <= 0 or K % 8 != 0; X, W
 * or ws not 16-byte aligned; targets / argmax not 8-byte, lp not 4-byte aligned; ws_bytes too small. */
#define SLAM_SCORE_CHUNK 512
size_t slam_op_score_rows_workspace(int M, int V);
int slam_op_score_rows(const void* X, const void* W, const int64_t* targets, const uint8_t* colmask, float* lp, int64_t* argmax,
                       int M, int V, int K, void* ws, size_t ws_bytes, slam_stream_t s);
/* one decode step of attention: qkv fp32 [B][(nH + 2 nKV) head_dim] projection without bias, bias bf16 [..] (nullable), lens
 * int32 [B] device = the new token's position. Bias and RoPE are applied in fp32 (queries pre-scaled as in the forward), the
 * new K / V rows are written to row lens[b] of k_cache / v_cache (bf16 [B][nKV][capacity][head_dim]) and o (bf16
 * [B][nH head_dim]) attends over rows 0 .. lens[b]. kv_bound >= max(lens) + 1, <= capacity.
 * ws: slam_op_attn_decode_workspace(B, nH, nKV, head_dim, kv_bound) bytes. */
size_t slam_op_attn_decode_workspace(int B, int nH, int nKV, int head_dim, int kv_bound);
int slam_op_attn_decode(const float* qkv, const void* bias, const int32_t* lens, void* k_cache, void* v_cache, void* o, void* ws,
                        size_t ws_bytes, int B, int nH, int nKV, int head_dim, int capacity, int kv_bound, float theta,
                        slam_stream_t s);
/* chunk attention over the cache (the attention of slam_extend): qkv bf16 [B T][(nH + 2 nKV) head_dim] exactly as the forward's
 * q|k|v buffer holds it - bias and RoPE applied, queries pre-scaled by head_dim^-0.5 * log2(e) (NOT the fp32 pre-bias row of
 * slam_op_attn_decode). Row b T + t is token t of row b's chunk, real when t < new_lens[b] (0 <= new_lens[b] <= T);
 * base_lens[b] (>= 0, may be 0) keys of row b are already in the cache; base_lens[b] + new_lens[b] <= kv_bound <= capacity.
 * The K and V columns of every real token are copied bit for bit to row base_lens[b] + t of k_cache / v_cache (bf16
 * [B][nKV][capacity][head_dim]) by a launch of their own, then o[b T + t] (bf16 [B T][nH head_dim]) = softmax attention of the
 * token's query heads over cache rows 0 .. base_lens[b] + t (16-query tiles on v_mfma_f32_16x16x32_bf16, all heads of a KV
 * group from one pass over its keys, exp2 domain, fp32 accumulation). Rows t >= new_lens[b] of o are zeros; no cache row
 * outside [base_lens[b], base_lens[b] + new_lens[b]) is written. Bit-identical run to run (key splits merged in split order).
 * head_dim 64 or 128, nH / nKV in 1 .. 8; every pointer 16-byte aligned.
 * ws: slam_op_attn_extend_workspace(B, T, nH, nKV, head_dim, kv_bound) bytes (0 when the launch takes one split; ws may then
 * be NULL). */
size_t slam_op_attn_extend_workspace(int B, int T, int nH, int nKV, int head_dim, int kv_bound);
int slam_op_attn_extend(const void* qkv, const int32_t* base_lens, const int32_t* new_lens, void* k_cache, void* v_cache,
                        void* o, void* ws, size_t ws_bytes, int B, int T, int nH, int nKV, int head_dim, int capacity,
                        int kv_bound, slam_stream_t s);
int slam_op_rmsnorm_fwd(const void* x, const void* w, void* y, float* rstd, int M, int H, float eps, slam_stream_t s);
size_t slam_op_rmsnorm_bwd_workspace(int M, int H);
int slam_op_rmsnorm_bwd(const void* dy, const void* x, const void* w, const float* rstd, const void* dres, void* dx,
                        float* dw, float* ws, int M, int H, slam_stream_t s);
/* OPT ops. LayerNorm: y = bf16((x - mean) rstd w + b), fp32 statistics from two passes (mean, rstd saved, fp32 [M]);
 * backward: dx = rstd (g - mean(g) - xhat mean(g xhat)) (+ dres), g = dy w; dw = sum dy xhat, db = sum dy (fp32 [H], stored). */
int slam_op_layernorm_fwd(const void* x, const void* w, const void* b, void* y, float* mean, float* rstd, int M, int H, float eps,
                          slam_stream_t s);
size_t slam_op_layernorm_bwd_workspace(int M, int H);
int slam_op_layernorm_bwd(const void* dy, const void* x, const void* w, const float* mean, const float* rstd, const void* dres,
                          void* dx, float* dw, float* db, float* ws, int M, int H, slam_stream_t s);
/* out[m] = bf16(E[ids[m]] + P[pos + 2]), pos = position_ids[m] or m % T; prow (int64 [M], nullable) receives pos + 2 */
int slam_op_embed_pos_fwd(const int64_t* ids, const int64_t* position_ids, const void* E, const void* P, void* out, int64_t* prow,
                          int M, int H, int V, int T, int n_rows_p, slam_stream_t s);
/* fc1: act[M,N] = relu(X W^T + bias) (only the post-ReLU activation is stored); fc2 dgrad with the ReLU backward fused into the
 * epilogue: dact[M,N] = (dY Wt^T) * [act > 0]; the elementwise form d *= [act > 0] (n a multiple of 8) */
int slam_op_gemm_nt_relu(const void* X, const void* W, void* act, const void* bias, int M, int N, int K, slam_stream_t s);
int slam_op_gemm_nt_drelu(const void* dY, const void* Wt, void* dact, const void* act, int M, int N, int K, slam_stream_t s);
int slam_op_relu_bwd(void* d, const void* act, int64_t n, slam_stream_t s);
int slam_op_rope(void* qkv, int ld, int M, int T, int n_rot_heads, int head_dim, const int64_t* position_ids, float theta,
                 int backward, float* cos_sin_ws /* 2*M*(head_dim/2) floats */, slam_stream_t s);
/* Qwen3's per-head q / k RMSNorm (arch 3), on qkv [M][(nH + 2 nKV) head_dim] (head_dim 64 or 128). For every token and every q
 * or k head, x = the head as the projection wrote it (bf16): rstd = rsqrt(mean_d(x^2) + eps), y = x rstd w with w = w_q for the
 * nH query heads and w_k for the nKV key heads (bf16 [head_dim] each, shared by the heads).
 * slam_op_qknorm_rope_fwd: y is rotated (rotate-half RoPE, tables built from position_ids - NULL: m % T - and theta into table_ws,
 *   4 * M * (head_dim / 2) floats; the query heads also take head_dim^-0.5 * log2(e)) and stored in place, all in fp32 with ONE
 *   rounding to bf16; the v columns are not touched. raw_out (bf16 [M][(nH + nKV) head_dim], nullable) receives the q|k input
 *   bits, rstd_out (fp32 [M][nH + nKV], nullable) the statistics: what the backward needs.
 * slam_op_qknorm_bwd: in place on the q|k columns of dqkv, which hold dy = the gradient of y (slam_op_attn_bwd_rope's output):
 *   g = dy w, dx = rstd (g - xhat mean_d(g xhat)), xhat = raw rstd; dw_q [head_dim] = the sum over tokens and query heads of
 *   dy xhat, dw_k likewise (fp32, stored). Per-block partial slabs in ws (slam_op_qknorm_bwd_workspace bytes) are added in block
 *   order: no floating-point atomics, the same bits every run.
 * slam_op_qknorm_rows_f32: the decode-time form - the q and k heads of fp32 rows [B][(nH + 2 nKV) head_dim] are replaced by y
 *   (fp32, no rounding to bf16); slam_op_attn_decode then rotates and rounds once, with bias = NULL.
 * SLAM_EINVAL before any launch: a NULL pointer (other than the nullable ones), M / B / T / nH / nKV <= 0, head_dim not 64 or 128,
 * or M (nH + nKV) head_dim / 8 >= 2^31 - 1024 (the kernels index heads in 32 bits). */
int slam_op_qknorm_rope_fwd(void* qkv, const void* w_q, const void* w_k, const int64_t* position_ids, float theta, float eps,
                            int M, int T, int nH, int nKV, int head_dim, void* raw_out, float* rstd_out, float* table_ws,
                            slam_stream_t s);
size_t slam_op_qknorm_bwd_workspace(int M, int nH, int nKV, int head_dim);
int slam_op_qknorm_bwd(void* dqkv, const void* raw, const float* rstd, const void* w_q, const void* w_k, float* dw_q, float* dw_k,
                       float* ws, int M, int nH, int nKV, int head_dim, slam_stream_t s);
int slam_op_qknorm_rows_f32(float* qkv, const void* w_q, const void* w_k, float eps, int B, int nH, int nKV, int head_dim,
                            slam_stream_t s);
int slam_op_swiglu_fwd(const void* gu, void* act, int M, int I, slam_stream_t s);
int slam_op_swiglu_bwd(void* gu_inout, const void* dact, int M, int I, slam_stream_t s);
/* attention ops: the QUERY columns of qkv are expected PRE-SCALED by head_dim^-0.5 * log2(e) (the engine's QKV projection
 * folds that factor into the queries' RoPE rotation: one rounding); dqkv's query columns come back as the gradient of
 * the UNSCALED queries. */
int slam_op_attn_fwd(const void* qkv, void* o, float* lse2, const int32_t* seg_start, int M, int nH, int nKV,
                     int head_dim, slam_stream_t s);
size_t slam_op_attn_bwd_workspace(int M, int nH, int head_dim);
int slam_op_attn_bwd(const void* qkv, const void* o, const void* d_o, const float* lse2, void* dqkv, float* ws,
                     const int32_t* seg_start, const int32_t* seg_end, int M, int nH, int nKV, int head_dim,
                     slam_stream_t s);
/* the backward as slam_backward calls it: dq / dk are stored rotated back (transpose RoPE) through fp32 cos / sin tables built
 * from position_ids (NULL: m % T) and theta into table_ws (2 * M * (head_dim / 2) floats, on top of `ws`, which is sized by
 * slam_op_attn_bwd_workspace as for slam_op_attn_bwd); the V columns are those of slam_op_attn_bwd. */
int slam_op_attn_bwd_rope(const void* qkv, const void* o, const void* d_o, const float* lse2, void* dqkv, float* ws,
                          const int32_t* seg_start, const int32_t* seg_end, const int64_t* position_ids, int T, float theta,
                          int M, int nH, int nKV, int head_dim, float* table_ws, slam_stream_t s);
/* the fused QKV projection of the head_dim-64 models: Y[M][N] = rope(X[M][K] W[N][K]^T + bias) on the first rope_heads
 * 64-column heads, the first q_heads of them also times 64^-0.5 * log2(e), the other columns bias only. The four tables
 * (cos, sin and their pre-scaled copies) are built into table_ws (4 * M * 32 floats) from position_ids (NULL: m % T).
 * SLAM_EINVAL for K % 64 or N % 128: slam_forward takes the unfused path (gemm_nt + rope) there. */
int slam_op_gemm_nt_rope(const void* X, const void* W, void* Y, const void* bias /* nullable */, const int64_t* position_ids,
                         float theta, int q_heads, int rope_heads, int M, int T, int N, int K, float* table_ws, slam_stream_t s);
/* out[N] (+)= column sums of the bf16 window X[M][0..N) with row stride ld, the way slam_backward forms a bias gradient:
 * per-row-block partial rows in ws (slam_op_colsum_workspace bytes), added in a fixed order. N and ld multiples of 8. */
size_t slam_op_colsum_workspace(int M, int N);
int slam_op_colsum(const void* X, int ld, int M, int N, float* out, int accumulate, float* ws, slam_stream_t s);
int slam_op_cross_entropy(const void* logits /* bf16 [B*T][Vp] */, const int64_t* labels, double num_items,
                          void* dlogits, float* row_loss, float* scratch2 /* {denom, loss} */, int B, int T,
                          int Vp /* padded row length: 512, or a multiple of 8 beyond */, int V, slam_stream_t s);
/* the loss launch under slam_set_label_smoothing(epsilon): row_loss [B*T] = the plain nll_t as above, row_smooth [B*T] = smooth_t
 * (both 0 on ignored rows), scratch2[1] = the smoothed loss, dlogits (may alias logits) its gradient. epsilon = 0 is
 * slam_op_cross_entropy itself (row_smooth is then not written and may be NULL); outside [0, 1): SLAM_EINVAL. */
int slam_op_cross_entropy_smooth(const void* logits /* bf16 [B*T][Vp] */, const int64_t* labels, double num_items,
                                 void* dlogits, float* row_loss, float* row_smooth, float* scratch2 /* {denom, loss} */, int B,
                                 int T, int Vp, int V, float epsilon, slam_stream_t s);
/* The movers and scalers of the logits / d-logits buffer, one launch each; all bf16, all exact or rounded once. SLAM_EINVAL before
 * any launch for a null pointer, a non-positive size, a row stride below ncols, V > Vp, Vp % 8, n % 8 or (the scalers) ncols % 8.
 * copy_cols: dst[m][0 .. ncols) = src[m][0 .. ncols) with row strides ld_src / ld_dst (slam_forward's logits_out).
 * unpad_logits: dst[b][t][0 .. V) = t < off[b + 1] - off[b] ? src[off[b] + t][0 .. V) : +0, src = Mp rows of Vp, off = int32 [B + 1]
 *   (slam_op_unpad_pack leaves it behind the six [Mmax] arrays of its scratch).
 * unpad_logits_spans: the same with row b's real columns starting at starts[b] (int32 [B], nullable = 0, clamped to [0, T]):
 *   dst[b][t][0 .. V) = 0 <= t - starts[b] < off[b + 1] - off[b] ? src[off[b] + t - starts[b]][0 .. V) : +0.
 * scale_bf16: x[i] = bf16(x[i] * scale), i < n (slam_backward's grad_scale).
 * scale_rows_bf16: x[m][:] *= coef[m / T], x = [M][ncols] (slam_scale_loss_rows).
 * scale_rows_unpadded_bf16: x[m][:] *= row[m] >= 0 ? coef[row[m]] : 0, x = [Mp][ncols], row = int32 [Mp] (slam_scale_loss_unpadded). */
int slam_op_copy_cols(const void* src, int ld_src, void* dst, int ld_dst, int M, int ncols, slam_stream_t s);
int slam_op_unpad_logits(const void* src, int Vp, void* dst, int V, const int32_t* off, int B, int T, int Mp, slam_stream_t s);
int slam_op_unpad_logits_spans(const void* src, int Vp, void* dst, int V, const int32_t* off, const int32_t* starts, int B, int T,
                               int Mp, slam_stream_t s);
int slam_op_scale_bf16(void* x, int64_t n, float scale, slam_stream_t s);
int slam_op_scale_rows_bf16(void* x, const float* coef, int M, int T, int ncols, slam_stream_t s);
int slam_op_scale_rows_unpadded_bf16(void* x, const float* coef, const int32_t* row, int Mp, int ncols, slam_stream_t s);
/* gather-side embedding gradient for vocabularies beyond 512: dE[ids[m]] += dh[m], token order (deterministic) */
size_t slam_op_embed_bwd_workspace(int M, int Vp);
int slam_op_embed_bwd(const int64_t* ids, const void* dh /* bf16 [M][H] */, float* dE /* fp32 [Vp][H] */, int M, int H,
                      int Vp, int V, int pad_id, void* ws, slam_stream_t s);
/* y_bf16[i] = the "adamw_sr" rounding of x[i], with the random bits of flat-buffer index index0 + i of array `which` (0 p, 1 m,
 * 2 v) at optimizer step `step` (>= 1) under `seed`: what the AdamW kernels apply to their state stores, on its own. */
int slam_op_sr_round_bf16(const float* x, void* y_bf16, int64_t n, int64_t index0, int64_t seed, int32_t step, int32_t which,
                          slam_stream_t s);
/* The two kernels of "dropout_thr16" on their own, on bf16 [M][H] (H a multiple of 8): the mask of element (m, n) is the one
 * the option's text defines for flat index index0 + m * H + n (index0 >= 0, a multiple of 8; the engine passes 0), call number
 * `call` (0 .. 2^32 - 1) and stream_id = 2 * layer + site. slam_op_dropout_add, in place: y = bf16(resid + (keep ? y * scale :
 * 0)); slam_op_dropout_bwd: dy_masked = keep ? bf16(dy * scale) : 0, dy itself untouched (another buffer). thr16 = 0 keeps
 * everything at scale 1. */
int slam_op_dropout_add(void* y, const void* resid, int M, int H, int32_t thr16, int64_t seed, int64_t call, int32_t stream_id,
                        int64_t index0, slam_stream_t s);
int slam_op_dropout_bwd(const void* dy, void* dy_masked, int M, int H, int32_t thr16, int64_t seed, int64_t call, int32_t stream_id,
                        int64_t index0, slam_stream_t s);
/* out [M][H] = E[ids[m]] (ids outside [0, V) read row 0): the plain gather of the Qwen2 / Qwen3 forward, H a multiple of 8 */
int slam_op_embed_fwd(const int64_t* ids, const void* E, void* out, int M, int H, int V, slam_stream_t s);
/* The embedding launch of an armed forward on its own (slam_set_neftune): out [M][H] bf16 = the gather of ids from E [V][H]
 * (+ row pos + 2 of P [n_rows_p][H], pos = position_ids[m] or m % T; prow as slam_op_embed_pos_fwd) plus the noise of flat index
 * index0 + m * H + h under (seed, call) at scale s. P = NULL: no position table (position_ids, prow, T and n_rows_p are not
 * read). SLAM_EINVAL before any launch: ids, E or out NULL, M <= 0, V <= 0, H % 8 != 0, with P a T or n_rows_p <= 0, s negative or not finite, call outside
 * 0 .. 2^32 - 1, index0 negative or no multiple of 8 (the engine's own launches pass 0). */
int slam_op_embed_noise_fwd(const int64_t* ids, const int64_t* position_ids, const void* E, const void* P, void* out, int64_t* prow,
                            int M, int H, int V, int T, int n_rows_p, float s, int64_t seed, int64_t call, int64_t index0,
                            slam_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SLAM_ENGINE_H */
