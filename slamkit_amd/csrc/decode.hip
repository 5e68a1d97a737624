// KV-cached generation kernels (slam_prefill / slam_decode_step, include/slam_engine.h):
//  * gemm_skinny: Y[M][N] = X[M][K] W[N][K]^T for a handful of rows. A decode step reads every weight once, so the launch is
//    a weight stream: each wave owns 16 W rows over a K range, loads them 16 B per lane straight into the B operand of
//    v_mfma_f32_16x16x32_bf16 (X rows padded to 16 form the A operand), and splits K until the grid covers the chip. The
//    split-K partials are summed in split order by a second launch: no atomics, the same bits every run.
//  * attn_decode: bias + RoPE of the new token's q / k on the fp32 projection (one rounding, the forward's tables and query
//    pre-scale), K / V appended to the cache, split-KV flash decoding with every query head of a KV group in one pass over the
//    group's keys, partial (m, l, o) merged in the log2 domain by attn_decode_combine in split order.
//  * sample_tokens (slam_sample_tokens): the next token of every row from its fp32 logits, on the device. A candidate is the
//    64-bit composite (order-preserving image of the score << idbits) | (idmask - id): all composites of a row differ and
//    "larger" is exactly "higher score, then lower id", so the top k is an exact radix select (integer LDS histograms, 8 bits a
//    pass, stopping as soon as a digit's bin is taken whole) and needs no float comparison. Rows longer than one chunk go
//    through two launches: every (chunk, row) block selects its local top k into the workspace, one block per row selects
//    among those, ranks the k' survivors and does the weights, the top-p cut, the Philox draw and the EOS / done / pad part.
//    Thread 0 forms the sums in the stated order: no floating-point atomics, nothing depends on the grid.
//    slam_sample_tokens_warped adds min_p / typical_p / epsilon_cutoff / eta_cutoff (HF's order) between the top-p cut and the
//    draw as a further instantiation of that last kernel: a thread per rank holds its membership of the kept set, thread 0
//    forms each normaliser and entropy in rank order, the typical_p order is formed by counting as the rank is.
//  * kv_repeat (slam_kv_repeat): fans the B prefilled cache rows out to B * n rows in place, row b -> rows b n .. b n + n - 1.
//    One launch per source row, in DESCENDING b on the one stream, each covering all layers, K and V, lens and the logits row.
//    Launch b reads row b and writes rows [b n, b n + n) minus b itself (only b = 0 is its own destination); for n >= 2 and
//    b >= 1 every one of those is > b, so a launch never writes what it reads, the destinations of the launches are disjoint,
//    and a row b' < b that a later launch reads is below every destination written before it. Only lens[b] keys are copied
//    (read on the device), as 16-byte loads and stores: bit-exact.
//  * attn_extend (slam_extend): a chunk of new tokens per row against the keys already cached. kv_extend_scatter appends the
//    chunk's K / V first, in a launch of its own; attn_extend then reads keys from the cache only, 16 queries x all heads of a
//    KV group per block on v_mfma_f32_16x16x32_bf16, scores formed transposed so that P feeds the PV product from the registers
//    it was computed in. Key splits are merged in split order by attn_extend_combine.
//  * constrain_scores (slam_constrain_scores): -inf for the tokens a row's own history bans (no repeated n-gram, bad word
//    sequences, EOS ids while the row is too short, begin-suppressed ids), the logits' bits elsewhere. Grid (chunks, B): a
//    block copies its chunk (not in place), then scans the history and stores the bans inside its own chunk. One constant is
//    stored, so equal stores may race: no atomics, no ordering between blocks.
//  * token_logprobs (slam_token_logprobs): the log-softmax of the raw logits row at one token. Chunks of SP_CHUNK scores; in a
//    chunk thread t takes scores t, t + 256, .. in that order, the 64 lanes of a wave are summed by the xor butterfly 32, 16,
//    .., 1, the four waves in wave order; chunks are combined in chunk order, one fused multiply-add each. Rows above one chunk
//    take two launches.
//  * cfg_scores (slam_cfg_scores): classifier-free guidance. Logits rows b and B + b (conditional, unconditional) into scores
//    row b = g (a - u) + u of their log-softmaxes, on token_logprobs' own chunk statistics (the same device functions; rows
//    above one chunk reuse its first launch over the 2 B rows). Grid (chunks, B); three separately rounded operations.
//    cfg_mirror_tokens copies the B chosen tokens behind themselves for the decode step over 2 B rows.
//  * ngram_propose (slam_ngram_propose): prompt-lookup proposals. One block per row scans the row's history once: thread t
//    takes the window ends t, t + 256, .., counts the tokens that match backwards from the end of the history, and a 64-bit
//    key (count << 32 | ~end) picks the longest match, the earliest among equals. Integers only; the two statistics by a second
//    one-block launch in a fixed order.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int SK_WAVES = 4;  // waves per block, one 16-row W tile each
constexpr int SK_U = 4;      // 32-deep K steps per unrolled group: 4 x 16 B loads in flight per lane
constexpr int SK_MIN_STEPS = 4;
constexpr int SK_TARGET_BLOCKS = 1024;

inline unsigned nblk(size_t n, int per) { return (unsigned)((n + per - 1) / per); }

template <bool F32OUT>
SLAM_DEVICE void skinny_store(void* Y, const bf16_t* bias, const bf16_t* resid, int m, int n, int N, float v) {
  const size_t i = (size_t)m * N + n;
  if (bias) v += bf16_to_f32(bias[n]);
  if (resid) v += bf16_to_f32(resid[i]);
  if (F32OUT) reinterpret_cast<float*>(Y)[i] = v;
  else reinterpret_cast<bf16_t*>(Y)[i] = f32_to_bf16(v);
}

// grid (ceil(N / 64), splits, ceil(M / 64)); MT = 16-row tiles of X per 64-row chunk
template <int MT, bool F32OUT>
__global__ __launch_bounds__(256) void gemm_skinny_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ W,
                                                          void* __restrict__ Y, float* __restrict__ part,
                                                          const bf16_t* __restrict__ bias, const bf16_t* __restrict__ resid,
                                                          int M, int N, int K, int kps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = (blockIdx.x * SK_WAVES + wave) * 16;
  if (n0 >= N) return;
  const int q = lane >> 4, j = lane & 15;
  const int m_base = blockIdx.z * 64;
  const int kb = blockIdx.y * kps * 32;
  const int ke = min(K, kb + kps * 32);
  const int nr = min(n0 + j, N - 1);  // tail rows re-read the last row; their results are not stored
  const bf16_t* wrow = W + (size_t)nr * K + 8 * q;
  const bf16_t* xrow[MT];
  bool xv[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = m_base + 16 * t + j;
    xv[t] = m < M;
    xrow[t] = X + (size_t)(xv[t] ? m : 0) * K + 8 * q;
  }
  f32x4_t acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const uint4 zero = {0u, 0u, 0u, 0u};
  for (int k = kb; k < ke; k += 32 * SK_U) {
    uint4 w[SK_U];
#pragma unroll
    for (int u = 0; u < SK_U; ++u) {
      const int kk = k + 32 * u;
      w[u] = (kk + 8 * q < ke) ? *reinterpret_cast<const uint4*>(wrow + kk) : zero;
    }
#pragma unroll
    for (int u = 0; u < SK_U; ++u) {
      const int kk = k + 32 * u;
      const bool kv = kk + 8 * q < ke;
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const uint4 a = (kv && xv[t]) ? *reinterpret_cast<const uint4*>(xrow[t] + kk) : zero;
        acc[t] = mfma16(a, w[u], acc[t]);
      }
    }
  }
  // lane holds acc[t][r] = Y[m_base + 16 t + 4 q + r][n0 + j]
  const int n = n0 + j;
  if (n >= N) return;
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m_base + 16 * t + 4 * q + r;
      if (m >= M) continue;
      if (part) part[((size_t)blockIdx.y * M + m) * N + n] = acc[t][r];
      else skinny_store<F32OUT>(Y, bias, resid, m, n, N, acc[t][r]);
    }
}

// Y = sum over splits in split order (+ bias + residual)
template <bool F32OUT>
__global__ __launch_bounds__(256) void skinny_reduce_kernel(const float* __restrict__ part, int S, void* __restrict__ Y,
                                                            const bf16_t* __restrict__ bias, const bf16_t* __restrict__ resid,
                                                            int M, int N) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t MN = (size_t)M * N;
  if (i >= MN) return;
  float v = 0.f;
  for (int s = 0; s < S; ++s) v += part[s * MN + i];
  skinny_store<F32OUT>(Y, bias, resid, (int)(i / N), (int)(i % N), N, v);
}

struct SkinnyPlan {
  int splits, kps;
};

// splits of the 32-deep K steps so that the grid has about SK_TARGET_BLOCKS blocks of SK_MIN_STEPS steps or more; fewer when
// the partials would not fit in ws_bytes
SkinnyPlan skinny_plan(int M, int N, int K, size_t ws_bytes) {
  const int ksteps = (K + 31) / 32;
  const int tiles = (int)nblk((size_t)N, 16 * SK_WAVES) * (int)nblk((size_t)M, 64);
  const int target = (SK_TARGET_BLOCKS + tiles - 1) / tiles;
  int kps = (ksteps + target - 1) / target;
  if (kps < SK_MIN_STEPS) kps = SK_MIN_STEPS;
  int S = (ksteps + kps - 1) / kps;
  const size_t per = (size_t)M * N * sizeof(float);
  if (S > 1 && (size_t)S * per > ws_bytes) {
    const int smax = (int)(ws_bytes / per);
    if (smax < 2) {
      S = 1;
    } else {
      kps = (ksteps + smax - 1) / smax;
      S = (ksteps + kps - 1) / kps;
    }
  }
  if (S <= 1) { S = 1; kps = ksteps; }
  return {S, kps};
}

template <bool F32OUT>
int launch_skinny(const bf16_t* X, const bf16_t* W, void* Y, const bf16_t* bias, const bf16_t* resid, int M, int N, int K,
                  float* ws, size_t ws_bytes, hipStream_t st) {
  const SkinnyPlan p = skinny_plan(M, N, K, ws ? ws_bytes : 0);
  float* part = p.splits > 1 ? ws : nullptr;
  const dim3 grid(nblk((size_t)N, 16 * SK_WAVES), p.splits, nblk((size_t)M, 64));
  const int mt = ((M < 64 ? M : 64) + 15) / 16;
#define SK_CASE(T) \
  case T: gemm_skinny_kernel<T, F32OUT><<<grid, 256, 0, st>>>(X, W, Y, part, bias, resid, M, N, K, p.kps); break;
  switch (mt) {
    SK_CASE(1)
    SK_CASE(2)
    SK_CASE(3)
    default: gemm_skinny_kernel<4, F32OUT><<<grid, 256, 0, st>>>(X, W, Y, part, bias, resid, M, N, K, p.kps); break;
  }
#undef SK_CASE
  if (part) skinny_reduce_kernel<F32OUT><<<nblk((size_t)M * N, 256), 256, 0, st>>>(part, p.splits, Y, bias, resid, M, N);
  return (int)hipGetLastError();
}

// ---- the same stream from FP8 codes (kernels.h: W8_K_GRAIN, w8_code_pos) --------------------------------------------------
constexpr int SK8_U = 2;  // 64-deep code blocks per unrolled group: the K depth of gemm_skinny_kernel's group

// eight codes (two dwords) -> the B operand: code -> fp32 (v_cvt_pk_f32_fp8) -> times the row's 2^e (exact) -> high 16 bits
SLAM_DEVICE uint4 w8_operand(uint32_t c0, uint32_t c1, float sc) {
  const f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)c0, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)c0, true);
  const f32x2_t c = __builtin_amdgcn_cvt_pk_f32_fp8((int)c1, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)c1, true);
  uint4 w;
  w.x = bf16_hi_pair(a.x * sc, a.y * sc);
  w.y = bf16_hi_pair(b.x * sc, b.y * sc);
  w.z = bf16_hi_pair(c.x * sc, c.y * sc);
  w.w = bf16_hi_pair(d.x * sc, d.y * sc);
  return w;
}

// gemm_skinny_kernel with W read as codes Q[N][K] (K a multiple of 64) and exponents E[N]: same grid, same K range per block,
// the 32-deep steps of a lane in the same order with the same operands. A lane's 16-byte load holds its codes of the two steps
// of one 64-deep block; a K range that starts in the middle of a block (odd kps) skips that block's first step, one that ends
// there its second. Every bound below is a multiple of 32, so a step is valid or not for the whole wave.
template <int MT, bool F32OUT>
__global__ __launch_bounds__(256) void gemm_skinny_w8_kernel(const bf16_t* __restrict__ X, const uint8_t* __restrict__ Q,
                                                             const int8_t* __restrict__ E, void* __restrict__ Y,
                                                             float* __restrict__ part, const bf16_t* __restrict__ bias,
                                                             const bf16_t* __restrict__ resid, int M, int N, int K, int kps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = (blockIdx.x * SK_WAVES + wave) * 16;
  if (n0 >= N) return;
  const int q = lane >> 4, j = lane & 15;
  const int m_base = blockIdx.z * 64;
  const int kb = blockIdx.y * kps * 32;
  const int ke = min(K, kb + kps * 32);
  const int nr = min(n0 + j, N - 1);  // tail rows re-read the last row; their results are not stored
  const uint8_t* qrow = Q + (size_t)nr * K + 16 * q;
  const float sc = __uint_as_float((uint32_t)((int)E[nr] + 127) << 23);  // lane j owns row n0 + j: its scale is a lane constant
  const bf16_t* xrow[MT];
  bool xv[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = m_base + 16 * t + j;
    xv[t] = m < M;
    xrow[t] = X + (size_t)(xv[t] ? m : 0) * K + 8 * q;
  }
  f32x4_t acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const uint4 zero = {0u, 0u, 0u, 0u};
  for (int k = kb & ~63; k < ke; k += 64 * SK8_U) {
    uint4 c[SK8_U];
#pragma unroll
    for (int u = 0; u < SK8_U; ++u) {
      const int kk = k + 64 * u;
      c[u] = kk < ke ? *reinterpret_cast<const uint4*>(qrow + kk) : zero;  // kk < ke <= K, K % 64 == 0: the block is whole
    }
#pragma unroll
    for (int u = 0; u < SK8_U; ++u)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int kk = k + 64 * u + 32 * s;
        if (kk < kb || kk >= ke) continue;
        const uint4 w = s ? w8_operand(c[u].z, c[u].w, sc) : w8_operand(c[u].x, c[u].y, sc);
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          const uint4 a = xv[t] ? *reinterpret_cast<const uint4*>(xrow[t] + kk) : zero;
          acc[t] = mfma16(a, w, acc[t]);
        }
      }
  }
  // lane holds acc[t][r] = Y[m_base + 16 t + 4 q + r][n0 + j]
  const int n = n0 + j;
  if (n >= N) return;
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m_base + 16 * t + 4 * q + r;
      if (m >= M) continue;
      if (part) part[((size_t)blockIdx.y * M + m) * N + n] = acc[t][r];
      else skinny_store<F32OUT>(Y, bias, resid, m, n, N, acc[t][r]);
    }
}

template <bool F32OUT>
int launch_skinny_w8(const bf16_t* X, const uint8_t* Q, const int8_t* E, void* Y, const bf16_t* bias, const bf16_t* resid, int M,
                     int N, int K, float* ws, size_t ws_bytes, hipStream_t st) {
  const SkinnyPlan p = skinny_plan(M, N, K, ws ? ws_bytes : 0);
  float* part = p.splits > 1 ? ws : nullptr;
  const dim3 grid(nblk((size_t)N, 16 * SK_WAVES), p.splits, nblk((size_t)M, 64));
  const int mt = ((M < 64 ? M : 64) + 15) / 16;
#define SK8_CASE(T) \
  case T: gemm_skinny_w8_kernel<T, F32OUT><<<grid, 256, 0, st>>>(X, Q, E, Y, part, bias, resid, M, N, K, p.kps); break;
  switch (mt) {
    SK8_CASE(1)
    SK8_CASE(2)
    SK8_CASE(3)
    default: gemm_skinny_w8_kernel<4, F32OUT><<<grid, 256, 0, st>>>(X, Q, E, Y, part, bias, resid, M, N, K, p.kps); break;
  }
#undef SK8_CASE
  if (part) skinny_reduce_kernel<F32OUT><<<nblk((size_t)M * N, 256), 256, 0, st>>>(part, p.splits, Y, bias, resid, M, N);
  return (int)hipGetLastError();
}

// ---- decode attention ---------------------------------------------------------------------------------------------------
SLAM_DEVICE float rescale(float m, float mn) { return m == -INFINITY ? 0.f : fast_exp2(m - mn); }

// dims d0 .. d0 + 7 of one head (columns c0 ..) of the fp32 projection row, + bias, rotate-half RoPE with tables C / S
template <int HD>
SLAM_DEVICE void rope8(const float* row, const bf16_t* bias, int c0, int d0, const float* C, const float* S, float* out) {
  constexpr int half = HD / 2;
  const bool lo = d0 < half;
  const int dp = lo ? d0 + half : d0 - half;  // partner dims
  const int t0 = lo ? d0 : d0 - half;         // table index
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    float x = row[c0 + d0 + i], p = row[c0 + dp + i];
    if (bias) { x += bf16_to_f32(bias[c0 + d0 + i]); p += bf16_to_f32(bias[c0 + dp + i]); }
    const float c = C[t0 + i], s = S[t0 + i];
    out[i] = lo ? x * c - p * s : x * c + p * s;
  }
}

SLAM_DEVICE void round8(float* v) {
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = bf16_to_f32(f32_to_bf16(v[i]));
}

// grid (ns, nKV, B), 256 threads. Key j of the chunk is handled by the LG = HD / 8 lanes of one slot (8 dims each); every slot
// keeps (m, l, o) for the G query heads of the group. part: [B][nH][ns][HD + 2] = o (unnormalised), m, l.
template <int HD, int G>
__global__ __launch_bounds__(256) void attn_decode_kernel(const float* __restrict__ qkv, const bf16_t* __restrict__ bias,
                                                          const float* __restrict__ cs, const float* __restrict__ sn,
                                                          const float* __restrict__ csq, const float* __restrict__ snq,
                                                          const int* __restrict__ lens, bf16_t* __restrict__ kc,
                                                          bf16_t* __restrict__ vc, int cap, int nH, int nKV, int chunk, int ns,
                                                          float* __restrict__ part) {
  constexpr int LG = HD / 8, SLOTS = 64 / LG, half = HD / 2;
  __shared__ float red[4][G][HD + 2];
  const int s = blockIdx.x, g = blockIdx.y, b = blockIdx.z;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane % LG, slot = lane / LG, d0 = sub * 8;
  const int QKV = (nH + 2 * nKV) * HD;
  const int pos = lens[b];
  const int nkeys = min(pos + 1, cap);
  const float* row = qkv + (size_t)b * QKV;
  const float* C = cs + (size_t)b * half;
  const float* S = sn + (size_t)b * half;
  float qf[G][8];
#pragma unroll
  for (int i = 0; i < G; ++i) {
    rope8<HD>(row, bias, (g * G + i) * HD, d0, csq + (size_t)b * half, snq + (size_t)b * half, qf[i]);
    round8(qf[i]);  // the forward stores q pre-scaled in bf16
  }
  float m_[G], l_[G], o_[G][8];
#pragma unroll
  for (int i = 0; i < G; ++i) {
    m_[i] = -INFINITY;
    l_[i] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) o_[i][e] = 0.f;
  }
  const size_t cbase = ((size_t)b * nKV + g) * cap;
  const int c_end = min(s * chunk + chunk, nkeys);
  for (int j = s * chunk + wave * SLOTS + slot; j < c_end; j += 4 * SLOTS) {
    float kf[8], vf[8];
    bf16_t* kp = kc + (cbase + j) * HD + d0;
    bf16_t* vp = vc + (cbase + j) * HD + d0;
    if (j == pos) {  // the new token: rotate, round once, append
      rope8<HD>(row, bias, (nH + g) * HD, d0, C, S, kf);
      const int cv = (nH + nKV + g) * HD + d0;
#pragma unroll
      for (int e = 0; e < 8; ++e) vf[e] = row[cv + e] + (bias ? bf16_to_f32(bias[cv + e]) : 0.f);
      const uint4 kb = pack_bf16x8(kf), vb = pack_bf16x8(vf);
      *reinterpret_cast<uint4*>(kp) = kb;
      *reinterpret_cast<uint4*>(vp) = vb;
      unpack_bf16x8(kb, kf);
      unpack_bf16x8(vb, vf);
    } else {
      unpack_bf16x8(*reinterpret_cast<const uint4*>(kp), kf);
      unpack_bf16x8(*reinterpret_cast<const uint4*>(vp), vf);
    }
#pragma unroll
    for (int i = 0; i < G; ++i) {
      float sc = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) sc += qf[i][e] * kf[e];
#pragma unroll
      for (int o = 1; o < LG; o <<= 1) sc += __shfl_xor(sc, o, 64);
      const float mn = fmaxf(m_[i], sc);
      const float a = rescale(m_[i], mn), p = fast_exp2(sc - mn);
      l_[i] = l_[i] * a + p;
#pragma unroll
      for (int e = 0; e < 8; ++e) o_[i][e] = o_[i][e] * a + p * vf[e];
      m_[i] = mn;
    }
  }
  // slots of a wave: xor butterfly (both partners compute the same sums)
#pragma unroll
  for (int off = LG; off < 64; off <<= 1)
#pragma unroll
    for (int i = 0; i < G; ++i) {
      const float m2 = __shfl_xor(m_[i], off, 64), l2 = __shfl_xor(l_[i], off, 64);
      const float mn = fmaxf(m_[i], m2);
      const float a = rescale(m_[i], mn), c = rescale(m2, mn);
      l_[i] = l_[i] * a + l2 * c;
#pragma unroll
      for (int e = 0; e < 8; ++e) o_[i][e] = o_[i][e] * a + __shfl_xor(o_[i][e], off, 64) * c;
      m_[i] = mn;
    }
  if (slot == 0) {
#pragma unroll
    for (int i = 0; i < G; ++i) {
#pragma unroll
      for (int e = 0; e < 8; ++e) red[wave][i][d0 + e] = o_[i][e];
      if (sub == 0) { red[wave][i][HD] = m_[i]; red[wave][i][HD + 1] = l_[i]; }
    }
  }
  __syncthreads();
  // waves in wave order
  const int t = threadIdx.x;
  if (t < G * LG) {
    const int i = t / LG, e0 = (t % LG) * 8;
    float mm = -INFINITY;
    for (int w = 0; w < 4; ++w) mm = fmaxf(mm, red[w][i][HD]);
    float l = 0.f, o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int w = 0; w < 4; ++w) {
      const float a = rescale(red[w][i][HD], mm);
      l += red[w][i][HD + 1] * a;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] += red[w][i][e0 + e] * a;
    }
    float* dst = part + (((size_t)b * nH + g * G + i) * ns + s) * (HD + 2);
#pragma unroll
    for (int e = 0; e < 8; ++e) dst[e0 + e] = o[e];
    if (e0 == 0) { dst[HD] = mm; dst[HD + 1] = l; }
  }
}

// grid (nH, B), HD threads: merge the ns partials of one (row, head) in split order
template <int HD>
__global__ __launch_bounds__(128) void attn_decode_combine_kernel(const float* __restrict__ part, int ns, int nH,
                                                                  bf16_t* __restrict__ out) {
  const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  const float* p = part + ((size_t)b * nH + h) * ns * (HD + 2);
  float mm = -INFINITY;
  for (int s = 0; s < ns; ++s) mm = fmaxf(mm, p[s * (HD + 2) + HD]);
  float l = 0.f, o = 0.f;
  for (int s = 0; s < ns; ++s) {
    const float a = rescale(p[s * (HD + 2) + HD], mm);
    l += p[s * (HD + 2) + HD + 1] * a;
    o += p[s * (HD + 2) + d] * a;
  }
  out[((size_t)b * nH + h) * HD + d] = f32_to_bf16(o / l);
}

// ---- small helpers of prefill / decode -------------------------------------------------------------------------------------
// K / V columns of rows t < lens[b] of one layer's qkv [B*T][QKV] -> cache rows t of (b, kv head); grid (.., B)
__global__ __launch_bounds__(256) void kv_scatter_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kc,
                                                         bf16_t* __restrict__ vc, const int* __restrict__ lens, int T, int nH,
                                                         int nKV, int hd, int cap) {
  const int b = blockIdx.y;
  const int per_row = 2 * nKV * hd / 8;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int t = idx / per_row, c = idx % per_row;
  if (t >= T || t >= lens[b] || t >= cap) return;
  const int kv = c / (nKV * hd / 8), r = c % (nKV * hd / 8);
  const int g = r / (hd / 8), d = (r % (hd / 8)) * 8;
  const int QKV = (nH + 2 * nKV) * hd;
  const uint4 v = *reinterpret_cast<const uint4*>(qkv + ((size_t)b * T + t) * QKV + (nH + kv * nKV + g) * hd + d);
  bf16_t* dst = (kv ? vc : kc) + (((size_t)b * nKV + g) * cap + t) * hd + d;
  *reinterpret_cast<uint4*>(dst) = v;
}

// dst[b] = src[b * T + clamp(lens[b] - 1, 0, T - 1)], rows of H bf16
__global__ __launch_bounds__(256) void gather_last_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst,
                                                          const int* __restrict__ lens, int B, int T, int H) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int per = H / 8;
  if (idx >= B * per) return;
  const int b = idx / per, c = idx % per;
  const int t = min(max(lens[b] - 1, 0), T - 1);
  *reinterpret_cast<uint4*>(dst + (size_t)b * H + 8 * c) =
      *reinterpret_cast<const uint4*>(src + ((size_t)b * T + t) * H + 8 * c);
}

__global__ void lens_to_pos_kernel(const int* __restrict__ lens, int64_t* __restrict__ pos, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) pos[b] = lens[b];
}

__global__ void lens_inc_kernel(int* __restrict__ lens, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) lens[b] = lens[b] + 1;
}

// ---- chunk attention over the cache (slam_extend) -----------------------------------------------------------------------------
// Row b appends new_lens[b] tokens behind its base_lens[b] cached keys. Both counts are clamped once per block to what the
// host bound allows, and every address below is formed from the clamped pair: base in [0, kv_bound], nl in
// [0, min(T, kv_bound - base)], so no key index reaches kv_bound (<= cap) and no token index reaches T.
struct ExtRow {
  int base, nl;
};
SLAM_DEVICE ExtRow ext_row(const int* __restrict__ base_lens, const int* __restrict__ new_lens, int b, int T, int kv_bound) {
  ExtRow r;
  r.base = min(max(base_lens[b], 0), kv_bound);
  r.nl = min(max(new_lens[b], 0), min(T, kv_bound - r.base));
  return r;
}

// K / V columns of the real tokens t < nl of qkv [B*T][QKV] -> cache rows base + t of (b, kv head); grid (.., B)
__global__ __launch_bounds__(256) void kv_extend_scatter_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kc,
                                                                bf16_t* __restrict__ vc, const int* __restrict__ base_lens,
                                                                const int* __restrict__ new_lens, int T, int nH, int nKV, int hd,
                                                                int cap, int kv_bound) {
  const int b = blockIdx.y;
  const ExtRow R = ext_row(base_lens, new_lens, b, T, kv_bound);
  const int per_row = 2 * nKV * hd / 8;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int t = idx / per_row, c = idx % per_row;
  if (t >= R.nl) return;
  const int kv = c / (nKV * hd / 8), r = c % (nKV * hd / 8);
  const int g = r / (hd / 8), d = (r % (hd / 8)) * 8;
  const int QKV = (nH + 2 * nKV) * hd;
  const uint4 v = *reinterpret_cast<const uint4*>(qkv + ((size_t)b * T + t) * QKV + (nH + kv * nKV + g) * hd + d);
  bf16_t* dst = (kv ? vc : kc) + (((size_t)b * nKV + g) * cap + R.base + t) * hd + d;
  *reinterpret_cast<uint4*>(dst) = v;
}

constexpr int AE_KB = 32;  // keys per LDS stage: two 16-key score tiles = one 32-deep PV step

// grid (ceil(T / 16), ns, B * nKV), 256 threads: one 16-query tile of one (row, KV group) over the keys of split y. The four
// waves stage each AE_KB-key block of the group once (K row-major, V transposed) and share it: wave w serves query heads
// w and w + 4 of the group. Scores are formed transposed, S^T = K Q^T, so that a lane ends up with P^T[keys][query] in the
// B-operand map of the PV product with no exchange: lane l (qd = l >> 4, j = l & 15) holds query j's keys 4 qd + r of the first
// tile and 16 + 4 qd + r of the second, and V^T is read with its contraction slots in that same key order. The output tile is
// O^T: lane l holds o[query j][d = 16 dt + 4 qd + r]. part == nullptr (one split): o is normalised and stored, rows t >= nl of
// the tile as zeros. Else part[((b T + t) nH + h) ns + split][HD + 4] = o (unnormalised), m, l for real rows; a split whose
// key range starts at or above the tile's last key writes nothing (the combine never reads it).
template <int HD, int G>
__global__ __launch_bounds__(256) void attn_extend_kernel(const bf16_t* __restrict__ qkv, const int* __restrict__ base_lens,
                                                          const int* __restrict__ new_lens, const bf16_t* __restrict__ kc,
                                                          const bf16_t* __restrict__ vc, bf16_t* __restrict__ o,
                                                          float* __restrict__ part, int T, int nH, int nKV, int cap, int kv_bound,
                                                          int chunk, int ns) {
  constexpr int NHW = (G + 3) / 4;      // heads per wave
  constexpr int KS = HD + 8;            // K row stride (bf16): 16-byte rows, fragment reads spread over the banks
  constexpr int VS = AE_KB + 4;         // V^T row stride (bf16): 8-byte rows, 18 dwords apart
  constexpr int DT = HD / 16, KK = HD / 32, PS = HD + 4;
  __shared__ __attribute__((aligned(16))) bf16_t Ks[AE_KB * KS];
  __shared__ __attribute__((aligned(16))) bf16_t Vt[HD * VS];
  const int q0 = blockIdx.x * 16, s = blockIdx.y;
  const int b = blockIdx.z / nKV, g = blockIdx.z % nKV;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qd = lane >> 4, j = lane & 15;
  const ExtRow R = ext_row(base_lens, new_lens, b, T, kv_bound);
  const int QKV = (nH + 2 * nKV) * HD;
  const int tq = q0 + j;                       // this lane's query (token of the chunk)
  const bool real = tq < R.nl;
  const int tile_n = min(q0 + 16, R.nl) - q0;  // real queries of the tile (<= 0: none)
  const int kend = tile_n > 0 ? R.base + q0 + tile_n : 0;  // keys the tile's last real query sees
  const int k_lo = s * chunk;
  const int k_hi = min(k_lo + chunk, kend);
  if (part && k_lo >= k_hi) return;
  const int qlim = R.base + min(tq, R.nl - 1);  // last key of this lane's query (clamped for the rows that are not real)

  uint4 qf[NHW][KK];
  f32x4_t acc[NHW][DT];
  float m_[NHW], l_[NHW];
#pragma unroll
  for (int hh = 0; hh < NHW; ++hh) {
    const int i = wave + 4 * hh;
    m_[hh] = -INFINITY;
    l_[hh] = 0.f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[hh][dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const int tr = max(min(tq, R.nl - 1), 0);
    const bf16_t* qrow = qkv + ((size_t)b * T + tr) * QKV + (size_t)(g * G + min(i, G - 1)) * HD + 8 * qd;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) qf[hh][kk] = *reinterpret_cast<const uint4*>(qrow + 32 * kk);
  }
  const size_t cbase = ((size_t)b * nKV + g) * cap;
  const uint4 zero = {0u, 0u, 0u, 0u};
  constexpr int NV = AE_KB * (HD / 8) / 256;  // 16-byte pieces of a K (and of a V) block per thread
  uint4 kx[NV], vx[NV];
  // the block's K / V pieces of this thread into registers; keys at or beyond k_hi as zeros: p = 0 meets 0, never the
  // cache's bits
  auto fetch = [&](int kb) {
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int v = threadIdx.x + 256 * u;
      const int kr = v / (HD / 8), d0 = (v % (HD / 8)) * 8;
      const bool ok = kb + kr < k_hi;
      const size_t src = (cbase + (ok ? kb + kr : 0)) * HD + d0;
      kx[u] = ok ? *reinterpret_cast<const uint4*>(kc + src) : zero;
      vx[u] = ok ? *reinterpret_cast<const uint4*>(vc + src) : zero;
    }
  };
  if (k_lo < k_hi) fetch(k_lo);
  for (int kb = k_lo; kb < k_hi; kb += AE_KB) {
    __syncthreads();  // the previous block's fragment reads are done
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int v = threadIdx.x + 256 * u;
      const int kr = v / (HD / 8), d0 = (v % (HD / 8)) * 8;
      *reinterpret_cast<uint4*>(&Ks[kr * KS + d0]) = kx[u];
      const uint32_t w[4] = {vx[u].x, vx[u].y, vx[u].z, vx[u].w};
#pragma unroll
      for (int e = 0; e < 8; ++e) Vt[(d0 + e) * VS + kr] = (bf16_t)(w[e >> 1] >> (16 * (e & 1)));
    }
    if (kb + AE_KB < k_hi) fetch(kb + AE_KB);  // the next block's loads fly under this block's products
    __syncthreads();
#pragma unroll
    for (int hh = 0; hh < NHW; ++hh) {
      if (wave + 4 * hh >= G) continue;  // wave-uniform
      // S^T tiles: lane holds key 16 c + 4 qd + r of query j
      f32x4_t sc[2];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        sc[c] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
          const uint4 kf = *reinterpret_cast<const uint4*>(&Ks[(16 * c + j) * KS + 32 * kk + 8 * qd]);
          sc[c] = mfma16(kf, qf[hh][kk], sc[c]);
        }
      }
      float mx = -INFINITY;
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ka = kb + 16 * c + 4 * qd + r;
          const float x = (ka < k_hi && ka <= qlim) ? sc[c][r] : -INFINITY;
          sc[c][r] = x;
          mx = fmaxf(mx, x);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mn = fmaxf(m_[hh], mx);
      const float ms = mn == -INFINITY ? 0.f : mn;  // nothing seen yet: every p below is exp2(-inf) = 0
      const float a = rescale(m_[hh], mn);
      float p[8], ps = 0.f;
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          p[4 * c + r] = fast_exp2(sc[c][r] - ms);
          ps += p[4 * c + r];
        }
      l_[hh] = l_[hh] * a + ps;  // this lane's share; the four lanes of a query are summed at the end
      m_[hh] = mn;
      const uint4 pf = pack_bf16x8(p);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const bf16_t* vrow = &Vt[(16 * dt + j) * VS + 4 * qd];
        const uint2 lo = *reinterpret_cast<const uint2*>(vrow), hi = *reinterpret_cast<const uint2*>(vrow + 16);
        const uint4 vf = {lo.x, lo.y, hi.x, hi.y};
        f32x4_t t = acc[hh][dt];
        t[0] *= a; t[1] *= a; t[2] *= a; t[3] *= a;
        acc[hh][dt] = mfma16(vf, pf, t);
      }
    }
  }
#pragma unroll
  for (int hh = 0; hh < NHW; ++hh) {
    const int i = wave + 4 * hh;
    if (i >= G) continue;
    float l = l_[hh];
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const int hq = g * G + i;
    if (part) {
      if (!real) continue;
      float* dst = part + ((((size_t)b * T + tq) * nH + hq) * ns + s) * PS;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
        *reinterpret_cast<float4*>(dst + 16 * dt + 4 * qd) = make_float4(acc[hh][dt][0], acc[hh][dt][1], acc[hh][dt][2], acc[hh][dt][3]);
      if (qd == 0) { dst[HD] = m_[hh]; dst[HD + 1] = l; }
    } else {
      if (tq >= T) continue;
      const float inv = real ? 1.f / l : 0.f;
      bf16_t* dst = o + (((size_t)b * T + tq) * nH + hq) * HD;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        uint2 w = {0u, 0u};
        if (real) {
          w.x = pack_bf16x2(acc[hh][dt][0] * inv, acc[hh][dt][1] * inv);
          w.y = pack_bf16x2(acc[hh][dt][2] * inv, acc[hh][dt][3] * inv);
        }
        *reinterpret_cast<uint2*>(dst + 16 * dt + 4 * qd) = w;
      }
    }
  }
}

// grid (nH, T, B), HD threads: merge the partials of one (token, head) in split order; rows t >= nl become zeros. Only the
// splits that start at or below the token's own key are read: those are exactly the ones that wrote this row.
template <int HD>
__global__ __launch_bounds__(128) void attn_extend_combine_kernel(const float* __restrict__ part,
                                                                  const int* __restrict__ base_lens,
                                                                  const int* __restrict__ new_lens, int T, int nH, int kv_bound,
                                                                  int chunk, int ns, bf16_t* __restrict__ out) {
  constexpr int PS = HD + 4;
  const int h = blockIdx.x, t = blockIdx.y, b = blockIdx.z, d = threadIdx.x;
  const int bt = b * T + t;
  const ExtRow R = ext_row(base_lens, new_lens, b, T, kv_bound);
  bf16_t* dst = out + ((size_t)bt * nH + h) * HD + d;
  if (t >= R.nl) { *dst = 0; return; }
  const int nsr = min(ns, (R.base + t) / chunk + 1);
  const float* p = part + ((size_t)bt * nH + h) * ns * PS;
  float mm = -INFINITY;
  for (int s = 0; s < nsr; ++s) mm = fmaxf(mm, p[s * PS + HD]);
  float l = 0.f, acc = 0.f;
  for (int s = 0; s < nsr; ++s) {
    const float ms = p[s * PS + HD];
    if (ms == -INFINITY) continue;  // a split with no key for this query
    const float a = fast_exp2(ms - mm);
    l += p[s * PS + HD + 1] * a;
    acc += p[s * PS + d] * a;
  }
  *dst = f32_to_bf16(acc / l);
}

// pos[b T + t] = lens[b] + t
__global__ void extend_pos_kernel(const int* __restrict__ lens, int64_t* __restrict__ pos, int B, int T) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B * T) pos[i] = (int64_t)lens[i / T] + (i % T);
}

// rows with new tokens take their logits row from src; lens[b] += clamp(new_lens[b], 0, T). grid (.., B)
__global__ __launch_bounds__(256) void extend_finish_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                            const int* __restrict__ new_lens, int* __restrict__ lens, int T,
                                                            int vocab) {
  const int b = blockIdx.y;
  const int nl = min(max(new_lens[b], 0), T);
  if (nl == 0) return;
  const size_t row = (size_t)b * vocab;
  for (int c = blockIdx.x * 256 + threadIdx.x; c < vocab; c += gridDim.x * 256) dst[row + c] = src[row + c];
  if (blockIdx.x == 0 && threadIdx.x == 0) lens[b] = lens[b] + nl;
}

// slam_extend_logits: chunk rows [m0, m0 + rows) of fp32 logits (src row 0 = chunk row m0) to dst[B T][vocab]; only the rows
// (b, t) with t < new_lens[b] are stored. grid (.., rows)
__global__ __launch_bounds__(256) void extend_store_rows_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                                const int* __restrict__ new_lens, int m0, int T, int vocab) {
  const int m = m0 + blockIdx.y;
  const int b = m / T, t = m - b * T;
  if (t >= new_lens[b]) return;
  const float* s = src + (size_t)blockIdx.y * vocab;
  float* d = dst + (size_t)m * vocab;
  for (int c = blockIdx.x * 256 + threadIdx.x; c < vocab; c += gridDim.x * 256) d[c] = s[c];
}

// lens[b] += clamp(new_lens[b], 0, T)
__global__ void lens_add_kernel(int* __restrict__ lens, const int* __restrict__ new_lens, int B, int T) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) lens[b] = lens[b] + min(max(new_lens[b], 0), T);
}

// ---- speculative decoding: the acceptance rule (include/slam_engine.h: slam_spec_accept) --------------------------------------
struct SpecParams {
  int B, K, max_new, pad_id, n_eos;
  long long out_stride;
};

// one block of 1024 threads, thread b = row b. Integer work only; the five statistics go through LDS in a fixed order.
__global__ __launch_bounds__(1024) void spec_accept_kernel(int64_t* __restrict__ chunk, const int64_t* __restrict__ tgt,
                                                           const int* __restrict__ eos_ids, const int* __restrict__ prompt_len,
                                                           int* __restrict__ n_new, uint8_t* __restrict__ done,
                                                           int64_t* __restrict__ out, int* __restrict__ lens_t,
                                                           int* __restrict__ lens_d, int64_t* __restrict__ draft_ids,
                                                           int* __restrict__ draft_new_lens, int* __restrict__ tgt_new_lens,
                                                           int* __restrict__ stats, SpecParams P) {
  __shared__ int red[5][16];
  const int b = threadIdx.x, lane = b & 63;
  int live = 0, lt = 0, ld = 0, emitted = 0, accepted = 0;
  if (b < P.B) {
    int64_t* ch = chunk + (size_t)b * (P.K + 1);
    const int64_t* tg = tgt + (size_t)b * (P.K + 1);
    const int nn = min(max(n_new[b], 0), P.max_new);
    bool dn = done[b] != 0;
    int m = 0, nacc = 0;
    if (!dn) {
      while (nacc < P.K && ch[nacc + 1] == tg[nacc]) ++nacc;
      m = min(nacc + 1, P.max_new - nn);  // the budget; not positive only for a row that should have been done
      for (int i = 0; i < m; ++i) {
        bool is_eos = false;
        for (int e = 0; e < P.n_eos; ++e) is_eos = is_eos || (int64_t)eos_ids[e] == tg[i];
        if (is_eos) { m = i + 1; dn = true; break; }
      }
      if (nn + m >= P.max_new) dn = true;
      for (int i = 0; i < m; ++i) out[(long long)b * P.out_stride + nn + i] = tg[i];
      emitted = m;
      accepted = min(m, nacc);
    }
    const int lag = m == P.K + 1 ? 1 : 0;
    const int64_t last = m > 0 ? tg[m - 1] : ch[0];
    const int64_t dK = ch[P.K];
    lt = prompt_len[b] + nn + m - 1;
    ld = lt - lag;
    n_new[b] = nn + m;
    lens_t[b] = lt;
    lens_d[b] = ld;
    ch[0] = last;
    draft_ids[2 * b] = lag ? dK : last;
    draft_ids[2 * b + 1] = lag ? tg[P.K] : (int64_t)P.pad_id;
    draft_new_lens[b] = dn ? 0 : 1 + lag;
    tgt_new_lens[b] = dn ? 0 : P.K + 1;
    done[b] = dn ? 1 : 0;
    live = dn ? 0 : 1;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    live += __shfl_xor(live, o, 64);
    emitted += __shfl_xor(emitted, o, 64);
    accepted += __shfl_xor(accepted, o, 64);
    lt = max(lt, __shfl_xor(lt, o, 64));
    ld = max(ld, __shfl_xor(ld, o, 64));
  }
  if (lane == 0) {
    const int w = b >> 6;
    red[0][w] = live; red[1][w] = lt; red[2][w] = ld; red[3][w] = emitted; red[4][w] = accepted;
  }
  __syncthreads();
  if (b == 0) {
    for (int w = 1; w < 16; ++w) {
      live += red[0][w]; lt = max(lt, red[1][w]); ld = max(ld, red[2][w]); emitted += red[3][w]; accepted += red[4][w];
    }
    stats[0] = live; stats[1] = lt; stats[2] = ld; stats[3] = emitted; stats[4] = accepted;
  }
}

// ---- prompt-lookup proposals (include/slam_engine.h: slam_ngram_propose) -----------------------------------------------------
constexpr int NG_THREADS = 256;
struct NgramParams {
  int K, max_ngram, fill_id, n_eos;
  long long prompt_stride, new_stride;
};

// h[j] of a row: the prompt's real tokens, then the new ones (ConstrainHistory's layout)
struct NgramHistory {
  const int64_t* prompt;
  const int64_t* fresh;
  int pl;
  SLAM_DEVICE int64_t at(int j) const { return j < pl ? prompt[j] : fresh[j - pl]; }
};

// grid B, one block per row. back(e) = the number of j < min(max_ngram, Lh - 1, e + 1) with h[e - j] == h[Lh - 1 - j] for all
// smaller j too: a window of n tokens ending at e (e <= Lh - 2, so the tail window is none) matches the last n tokens iff
// back(e) >= n. The longest n with a match is max back(e), its earliest window the lowest such e; the proposals start at e + 1.
__global__ __launch_bounds__(NG_THREADS) void ngram_propose_kernel(int64_t* __restrict__ chunk, int* __restrict__ n_prop,
                                                                   const int64_t* __restrict__ prompt,
                                                                   const int* __restrict__ prompt_len,
                                                                   const int64_t* __restrict__ fresh,
                                                                   const int* __restrict__ n_new,
                                                                   const uint8_t* __restrict__ done,
                                                                   const int* __restrict__ eos_ids, NgramParams P) {
  __shared__ unsigned long long red[NG_THREADS / 64];
  __shared__ int stop[slam::SPEC_MAX_K + 1];
  const int b = blockIdx.x, t = threadIdx.x;
  NgramHistory h;
  h.pl = (int)min((long long)max(prompt_len[b], 0), P.prompt_stride);
  const int nn = (int)min((long long)max(n_new[b], 0), P.new_stride);
  h.prompt = prompt + (long long)b * P.prompt_stride;
  h.fresh = fresh + (long long)b * P.new_stride;  // dereferenced only for nn > 0
  const int Lh = h.pl + nn;
  unsigned long long key = 0;  // (back << 32) | ~e: larger is "longer, then earlier"; 0 = no match
  if (done[b] == 0 && Lh >= 2) {
    const int nmax = min(P.max_ngram, Lh - 1);
    for (int e = t; e < Lh - 1; e += NG_THREADS) {
      const int lim = min(nmax, e + 1);
      int back = 0;
      while (back < lim && h.at(e - back) == h.at(Lh - 1 - back)) ++back;
      if (back > 0) {
        const unsigned long long k = ((unsigned long long)back << 32) | (unsigned long long)(0xffffffffu - (uint32_t)e);
        key = k > key ? k : key;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o, 64);
    key = other > key ? other : key;
  }
  if ((t & 63) == 0) red[t >> 6] = key;
  __syncthreads();
  key = red[0];
#pragma unroll
  for (int w = 1; w < NG_THREADS / 64; ++w) key = red[w] > key ? red[w] : key;
  int start = 0, count = 0;
  if (key != 0) {
    start = (int)(0xffffffffu - (uint32_t)key) + 1;  // idx + n
    count = min(P.K, Lh - start);                    // >= 1: e <= Lh - 2
  }
  int64_t tok = P.fill_id;
  bool is_eos = false;
  if (t < count) {
    tok = h.at(start + t);
    for (int e = 0; e < P.n_eos; ++e) is_eos = is_eos || (int64_t)eos_ids[e] == tok;
  }
  if (t < P.K) stop[t] = (t < count && !is_eos) ? 0 : 1;  // the proposals end in front of column 1 + t
  __syncthreads();
  if (t < P.K) {
    int np = 0;
    while (np < P.K && !stop[np]) ++np;
    chunk[(size_t)b * (P.K + 1) + 1 + t] = t < np ? tok : (int64_t)P.fill_id;
    if (t == 0) n_prop[b] = np;
  }
}

// one block of 1024 threads, thread b = row b: { rows with a proposal, the sum of n_prop } through LDS in a fixed order
__global__ __launch_bounds__(1024) void ngram_stats_kernel(const int* __restrict__ n_prop, int B, int* __restrict__ stats) {
  __shared__ int red[2][16];
  const int b = threadIdx.x, lane = b & 63;
  int total = b < B ? n_prop[b] : 0;
  int rows = total > 0 ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    rows += __shfl_xor(rows, o, 64);
    total += __shfl_xor(total, o, 64);
  }
  if (lane == 0) { red[0][b >> 6] = rows; red[1][b >> 6] = total; }
  __syncthreads();
  if (b == 0) {
    for (int w = 1; w < 16; ++w) { rows += red[0][w]; total += red[1][w]; }
    stats[0] = rows; stats[1] = total;
  }
}


// ---- token sampling ---------------------------------------------------------------------------------------------------------
constexpr int SP_THREADS = 256;
constexpr int SP_CHUNK = 2048;   // scores per stage-1 block; rows up to this length take the single launch
constexpr int SP_MAXK = 256;     // top_k limit (SlamSampleDesc)
constexpr int SP_CACHE = 4096;   // stage-2 candidates kept in LDS; the rest are re-read from the workspace every pass
constexpr uint32_t SP_NEG_INF_KEY = 0x007fffffu;  // score_key(-inf): a candidate needs a larger key

typedef unsigned long long u64_t;

// order-preserving integer image of a score: banned / NaN -> -inf, +inf -> FLT_MAX, -0 -> +0
SLAM_DEVICE uint32_t score_key(float x, bool banned) {
  if (banned || x != x) x = -INFINITY;
  x = fminf(x, FLT_MAX);
  uint32_t u = __float_as_uint(x);
  if ((u << 1) == 0u) u = 0u;
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
SLAM_DEVICE float key_score(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

struct SampleShared {
  uint32_t hist[256];
  u64_t sel[SP_MAXK];
  float x[SP_MAXK];
  float w[SP_MAXK];
  int id[SP_MAXK];
  int red[SP_THREADS / 64];
  int bc[3];  // the selected digit, the count above it, the digit's own count
  int cnt;
};

// scores [c0, c0 + n) of one row as keys in LDS; n <= SP_CHUNK. The row may start at any 4-byte boundary: scalar loads up to
// the first 16-byte boundary, 16-byte loads from there, scalar loads for the rest.
SLAM_DEVICE void load_keys(const float* __restrict__ row, const uint8_t* __restrict__ banned, int c0, int n, uint32_t* keys) {
  const float* p = row + c0;
  const uint8_t* bn = banned ? banned + c0 : nullptr;
  int head = (int)((4u - (uint32_t)(((uintptr_t)p >> 2) & 3u)) & 3u);
  if (head > n) head = n;
  const int nv = (n - head) >> 2;
  const int t = threadIdx.x;
  if (t < head) keys[t] = score_key(p[t], bn && bn[t]);
  const float4* pv = reinterpret_cast<const float4*>(p + head);
  for (int v = t; v < nv; v += SP_THREADS) {
    const float4 f = pv[v];
    const int i = head + 4 * v;
    keys[i + 0] = score_key(f.x, bn && bn[i + 0]);
    keys[i + 1] = score_key(f.y, bn && bn[i + 1]);
    keys[i + 2] = score_key(f.z, bn && bn[i + 2]);
    keys[i + 3] = score_key(f.w, bn && bn[i + 3]);
  }
  for (int i = head + 4 * nv + t; i < n; i += SP_THREADS) keys[i] = score_key(p[i], bn && bn[i]);
}

// composites of a chunk held as keys in LDS
struct KeySrc {
  const uint32_t* keys;
  int base, idbits;
  uint32_t idmask;
  SLAM_DEVICE u64_t operator()(int i) const { return ((u64_t)keys[i] << idbits) | (u64_t)(idmask - (uint32_t)(base + i)); }
};
// composites that stage 1 wrote: the first ncache from LDS, the rest from the workspace
struct PairSrc {
  const u64_t* cache;
  const u64_t* g;
  int ncache;
  SLAM_DEVICE u64_t operator()(int i) const { return i < ncache ? cache[i] : g[i]; }
};

// The min(k, candidates) largest composites of src(0 .. n) into sh.sel, in no particular order; returns their number.
// Every thread of the block calls it (barriers inside); the result is the same set whatever the order of the items.
template <class Src>
SLAM_DEVICE int select_topk(const Src& src, int n, int k, int idbits, SampleShared& sh) {
  const int t = threadIdx.x, lane = t & 63;
  const u64_t lowest = ((u64_t)SP_NEG_INF_KEY + 1) << idbits;  // candidates are >= this
  int c = 0;
  for (int i = t; i < n; i += SP_THREADS) c += src(i) >= lowest ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if (lane == 0) sh.red[t >> 6] = c;
  if (t == 0) sh.cnt = 0;
  __syncthreads();
  int nvalid = 0;
#pragma unroll
  for (int w = 0; w < SP_THREADS / 64; ++w) nvalid += sh.red[w];
  const int kk = k < nvalid ? k : nvalid;
  if (kk == 0) return 0;
  const int npass = (32 + idbits + 7) / 8;
  u64_t prefix = 0, mask = 0;
  int remaining = kk;
  for (int p = 0; p < npass; ++p) {
    const int shift = 8 * (npass - 1 - p);
    sh.hist[t] = 0;
    __syncthreads();
    for (int i = t; i < n; i += SP_THREADS) {
      const u64_t v = src(i);
      if (v >= lowest && (v & mask) == prefix) atomicAdd(&sh.hist[(uint32_t)(v >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (t < 64) {  // bins from the top: the first one at which the running count reaches `remaining`
      int s[4], local = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) { s[j] = (int)sh.hist[255 - (4 * lane + j)]; local += s[j]; }
      int incl = local;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
      }
      int run = incl - local;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (run < remaining && run + s[j] >= remaining) { sh.bc[0] = 255 - (4 * lane + j); sh.bc[1] = run; sh.bc[2] = s[j]; }
        run += s[j];
      }
    }
    __syncthreads();
    prefix |= (u64_t)sh.bc[0] << shift;
    mask |= (u64_t)255 << shift;
    remaining -= sh.bc[1];
    if (sh.bc[2] == remaining) break;  // the whole bin is in: (v & mask) >= prefix is the selection
  }
  for (int i = t; i < n; i += SP_THREADS) {
    const u64_t v = src(i);
    if (v >= lowest && (v & mask) >= prefix) {
      const int slot = atomicAdd(&sh.cnt, 1);
      if (slot < SP_MAXK) sh.sel[slot] = v;
    }
  }
  __syncthreads();
  return kk;
}

struct SampleParams {
  int do_sample, k, vocab, idbits, nch, pad_id, n_eos;
  float inv_t, top_p;
  uint32_t k0, k1, step;
  long long out_stride, out_col;
  int group;  // rows per sequence: row b is column b % group of sequence b / group (slam_sample_tokens_at)
};

SLAM_DEVICE void emit_token(long long tok, bool mark, int b, const SampleParams& P, const int* eos_ids, uint8_t* done,
                            int64_t* next, int64_t* out) {
  next[b] = tok;
  if (out) out[(long long)b * P.out_stride + P.out_col] = tok;
  if (mark && done)
    for (int e = 0; e < P.n_eos; ++e)
      if (eos_ids[e] == (int)tok) { done[b] = 1; break; }
}

// stage 1, grid (chunks, B): the chunk's top k as composites into ws[b][chunk][k], unused slots 0 (no candidate)
__global__ __launch_bounds__(SP_THREADS) void sample_select_kernel(const float* __restrict__ logits,
                                                                   const uint8_t* __restrict__ banned,
                                                                   const uint8_t* __restrict__ done, SampleParams P,
                                                                   u64_t* __restrict__ ws) {
  __shared__ uint32_t keys[SP_CHUNK];
  __shared__ SampleShared sh;
  const int ch = blockIdx.x, b = blockIdx.y;
  if (done && done[b]) return;
  const int c0 = ch * SP_CHUNK;
  const int n = min(SP_CHUNK, P.vocab - c0);
  load_keys(logits + (size_t)b * P.vocab, banned, c0, n, keys);
  __syncthreads();
  const KeySrc src{keys, c0, P.idbits, (1u << P.idbits) - 1u};
  const int kk = select_topk(src, n, P.k, P.idbits, sh);
  u64_t* dst = ws + ((size_t)b * P.nch + ch) * P.k;
  for (int i = threadIdx.x; i < P.k; i += SP_THREADS) dst[i] = i < kk ? sh.sel[i] : 0ull;
}

// slam_sample_tokens_warped: the description of the plain call, then min_p / typical_p / epsilon_cutoff / eta_cutoff
struct WarpSampleParams : SampleParams {
  float min_p, typical_p, eps_cut, eta_cut;
};
template <bool WARP> struct SampleParamsOf { typedef SampleParams type; };
template <> struct SampleParamsOf<true> { typedef WarpSampleParams type; };

// LDS of the warper chain; a thread owns the rank of its index. The float arrays are read 16 bytes at a time.
struct alignas(16) WarpShared {
  float kw[SP_MAXK];    // w_j of the ranks in S, 0 for the others (adding 0 keeps the bits of a sum over S in rank order)
  float term[SP_MAXK];  // p_j log p_j of the ranks in S with w_j > 0, 0 for the others
  float s[SP_MAXK];     // typical_p: s_j of the ranks in S, NaN for the others (a NaN never counts as "in front")
  float op[SP_MAXK];    // typical_p: p in the (s, rank) order
  float os[SP_MAXK];    // typical_p: s in that order
  u64_t mask[SP_THREADS / 64];  // membership of S, a bit per rank
  float Z, logZ, H, cut;
  int n, top, last;     // |S|, its lowest and its highest rank
};

// a[0] + a[1] + .. + a[n - 1] in that order from 0.0f, on one thread. a is zero behind n up to the next multiple of 4 (x + 0
// is x): 16-byte LDS loads and no branch, so the loads run ahead of the dependent adds.
SLAM_DEVICE float seq_sum(const float* a, int n) {
  const float4* v = reinterpret_cast<const float4*>(a);
  float s = 0.f;
#pragma unroll 8
  for (int i = 0; i < (n + 3) >> 2; ++i) {
    const float4 f = v[i];
    s += f.x;
    s += f.y;
    s += f.z;
    s += f.w;
  }
  return s;
}

// Z_S and log Z_S, summed by thread 0 in rank order, |S| and the lowest and highest rank of S from the waves' ballots; every
// thread of the block calls it with its own rank's membership and weight (barriers inside).
SLAM_DEVICE void warp_normaliser(WarpShared& wsh, int kk, bool in, float w) {
  const int t = threadIdx.x;
  wsh.kw[t] = in ? w : 0.f;
  const u64_t m = __ballot(in);
  if ((t & 63) == 0) wsh.mask[t >> 6] = m;
  __syncthreads();
  if (t == 0) {
    const float z = seq_sum(wsh.kw, kk);
    int n = 0, top = -1, last = 0;
#pragma unroll
    for (int v = 0; v < SP_THREADS / 64; ++v) {
      const u64_t b = wsh.mask[v];
      if (b) {
        n += __popcll(b);
        if (top < 0) top = 64 * v + __ffsll((long long)b) - 1;
        last = 64 * v + 63 - __clzll((long long)b);
      }
    }
    wsh.Z = z;
    wsh.logZ = logf(z);
    wsh.n = n;
    wsh.top = top < 0 ? 0 : top;
    wsh.last = last;
  }
  __syncthreads();
}

// H_S behind warp_normaliser: -(sum of p_j log p_j over S, w_j > 0) in rank order on thread 0. p, lp: this rank's.
SLAM_DEVICE void warp_entropy(WarpShared& wsh, int kk, bool in, float w, float p, float lp) {
  const int t = threadIdx.x;
  wsh.term[t] = (in && w > 0.f) ? p * lp : 0.f;
  __syncthreads();
  if (t == 0) wsh.H = -seq_sum(wsh.term, kk);
  __syncthreads();
}

// one block per row. ROW: the whole row (vocab <= SP_CHUNK) is selected here; else the candidates of stage 1.
// WARP: the warper chain of slam_sample_tokens_warped between the top-p prefix and the draw (sampling only).
template <bool ROW, bool WARP = false>
__global__ __launch_bounds__(SP_THREADS) void sample_finish_kernel(const float* __restrict__ logits,
                                                                   const uint8_t* __restrict__ banned,
                                                                   const int64_t* __restrict__ row_ids,
                                                                   const int* __restrict__ eos_ids, uint8_t* __restrict__ done,
                                                                   int64_t* __restrict__ next, int64_t* __restrict__ out,
                                                                   typename SampleParamsOf<WARP>::type P,
                                                                   const u64_t* __restrict__ ws,
                                                                   const uint32_t* __restrict__ steps) {
  __shared__ u64_t buf[ROW ? SP_CHUNK / 2 : SP_CACHE];
  __shared__ SampleShared sh;
  const int b = blockIdx.x, t = threadIdx.x;
  if (done && done[b]) {
    if (t == 0) emit_token(P.pad_id, false, b, P, eos_ids, done, next, out);
    return;
  }
  int kk;
  if (ROW) {
    uint32_t* keys = reinterpret_cast<uint32_t*>(buf);
    load_keys(logits + (size_t)b * P.vocab, banned, 0, P.vocab, keys);
    __syncthreads();
    const KeySrc src{keys, 0, P.idbits, (1u << P.idbits) - 1u};
    kk = select_topk(src, P.vocab, P.k, P.idbits, sh);
  } else {
    const int n = P.nch * P.k;
    const u64_t* g = ws + (size_t)b * n;
    const int ncache = n < SP_CACHE ? n : SP_CACHE;
    for (int i = t; i < ncache; i += SP_THREADS) buf[i] = g[i];
    __syncthreads();
    const PairSrc src{buf, g, ncache};
    kk = select_topk(src, n, P.k, P.idbits, sh);
  }
  if (kk == 0) {  // no finite score: pad, the row is not marked done
    if (t == 0) emit_token(P.pad_id, false, b, P, eos_ids, done, next, out);
    return;
  }
  // rank j = how many of the k' composites are larger: (score descending, id ascending)
  const uint32_t idmask = (1u << P.idbits) - 1u;
  if (t < kk) {
    const u64_t v = sh.sel[t];
    int r = 0;
    for (int j = 0; j < kk; ++j) r += sh.sel[j] > v ? 1 : 0;
    sh.x[r] = key_score((uint32_t)(v >> P.idbits));
    sh.id[r] = (int)(idmask - ((uint32_t)v & idmask));
  }
  __syncthreads();
  if (!P.do_sample) {
    if (t == 0) emit_token(sh.id[0], true, b, P, eos_ids, done, next, out);
    return;
  }
  if (t < kk) sh.w[t] = t == 0 ? 1.0f : expf((sh.x[t] - sh.x[0]) * P.inv_t);
  __syncthreads();
  if constexpr (WARP) {
    __shared__ WarpShared wsh;
    if (t == 0) {  // the top-p prefix, as in the plain kernel below
      int m = kk;
      if (P.top_p < 1.0f) {
        float tail = 0.f;
        for (int j = kk - 1; j >= 0; --j) tail += sh.w[j];
        const float thr = (1.0f - P.top_p) * tail;
        tail = 0.f;
        for (int j = kk - 1; j > 0; --j) {
          tail += sh.w[j];
          if (tail <= thr) m = j;
          else break;
        }
      }
      wsh.n = m;
    }
    __syncthreads();
    // thread t owns rank t: its membership of S, its scaled score a, weight w and score x
    const bool cand = t < kk;
    bool in = t < wsh.n;
    const float x = cand ? sh.x[t] : 0.f;
    const float a = (cand && t > 0) ? (x - sh.x[0]) * P.inv_t : 0.f;
    const float w = cand ? sh.w[t] : 0.f;
    if (P.min_p > 0.f) {  // S is a prefix: its lowest rank is 0
      if (in && w < P.min_p * sh.w[0]) in = false;
    }
    if (P.typical_p < 1.0f) {
      warp_normaliser(wsh, kk, in, w);
      const float p = w / wsh.Z, lp = a - wsh.logZ;
      warp_entropy(wsh, kk, in, w, p, lp);
      const float s = fabsf(-lp - wsh.H);
      wsh.s[t] = in ? s : __uint_as_float(0x7fc00000u);
      __syncthreads();
      if (in) {  // position in the (s ascending, rank ascending) order = the number of ranks of S in front
        const float4* sv = reinterpret_cast<const float4*>(wsh.s);
        int pos = 0;
        for (int i = 0; i < (kk + 3) >> 2; ++i) {
          const float4 f = sv[i];
          const int j = 4 * i;
          pos += (f.x < s || (f.x == s && j + 0 < t)) ? 1 : 0;
          pos += (f.y < s || (f.y == s && j + 1 < t)) ? 1 : 0;
          pos += (f.z < s || (f.z == s && j + 2 < t)) ? 1 : 0;
          pos += (f.w < s || (f.w == s && j + 3 < t)) ? 1 : 0;
        }
        wsh.op[pos] = p;
        wsh.os[pos] = s;
      }
      __syncthreads();
      if (t == 0) {  // c_i is non-decreasing: #{c_i < mass} is the first i with c_i >= mass; no branch, as in seq_sum
        const float4* pv = reinterpret_cast<const float4*>(wsh.op);
        const int n = wsh.n;
        int last = n - 1;
        bool found = false;
        float c = 0.f;
#pragma unroll 4
        for (int i = 0; i < (n + 3) >> 2; ++i) {
          const float4 f = pv[i];
          const float e[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            c += e[q];
            const bool hit = !found && 4 * i + q < n && !(c < P.typical_p);
            last = hit ? 4 * i + q : last;
            found = found || hit;
          }
        }
        wsh.cut = wsh.os[last];
      }
      __syncthreads();
      if (in && s > wsh.cut) in = false;
    }
    if (P.eps_cut > 0.f) {
      warp_normaliser(wsh, kk, in, w);
      const float p = w / wsh.Z;
      if (in && p < P.eps_cut && x != sh.x[wsh.top]) in = false;
    }
    if (P.eta_cut > 0.f) {
      warp_normaliser(wsh, kk, in, w);
      const float p = w / wsh.Z, lp = a - wsh.logZ;
      warp_entropy(wsh, kk, in, w, p, lp);
      const float eta = fminf(P.eta_cut, sqrtf(P.eta_cut) * expf(-wsh.H));
      if (in && p < eta && x != sh.x[wsh.top]) in = false;
    }
    warp_normaliser(wsh, kk, in, w);  // total = Z of the final S: the same adds in the same order as cum below
    if (t != 0) return;
    const float total = wsh.Z;
    const int q = b / P.group;
    const uint64_t r = row_ids ? (uint64_t)row_ids[q] : (uint64_t)q;
    const uint32_t step = P.step + (steps ? steps[q] : 0u) + (uint32_t)(b - q * P.group);
    const Philox4 rnd = philox4x32_10((uint32_t)r, step, (uint32_t)(r >> 32), 0x53414D50u, P.k0, P.k1);
    const float u = (float)(rnd.w[0] >> 8) * 5.9604644775390625e-08f;  // 2^-24
    const float target = u * total;
    // cum stands still on a rank outside S (its kw is 0), so the first rank with cum > target is in S
    const float4* wv = reinterpret_cast<const float4*>(wsh.kw);
    const int last = wsh.last;
    int pick = -1;
    float cum = 0.f;
#pragma unroll 4
    for (int i = 0; i < (kk + 3) >> 2; ++i) {
      const float4 f = wv[i];
      const float e[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        cum += e[c];
        pick = (pick < 0 && cum > target) ? 4 * i + c : pick;
      }
    }
    emit_token(sh.id[pick < 0 ? last : pick], true, b, P, eos_ids, done, next, out);
    return;
  }
  if (t != 0) return;
  int m = kk;
  if (P.top_p < 1.0f) {
    float tail = 0.f;
    for (int j = kk - 1; j >= 0; --j) tail += sh.w[j];
    const float thr = (1.0f - P.top_p) * tail;
    tail = 0.f;
    for (int j = kk - 1; j > 0; --j) {
      tail += sh.w[j];
      if (tail <= thr) m = j;  // tail grows towards rank 0: the dropped ranks are a suffix
      else break;
    }
  }
  float total = 0.f;
  for (int j = 0; j < m; ++j) total += sh.w[j];
  const int q = b / P.group;  // the row's sequence; group = 1 and steps = NULL are slam_sample_tokens
  const uint64_t r = row_ids ? (uint64_t)row_ids[q] : (uint64_t)q;
  const uint32_t step = P.step + (steps ? steps[q] : 0u) + (uint32_t)(b - q * P.group);
  const Philox4 rnd = philox4x32_10((uint32_t)r, step, (uint32_t)(r >> 32), 0x53414D50u, P.k0, P.k1);
  const float u = (float)(rnd.w[0] >> 8) * 5.9604644775390625e-08f;  // 2^-24
  const float target = u * total;
  int pick = m - 1;
  float cum = 0.f;
  for (int j = 0; j < m; ++j) {
    cum += sh.w[j];
    if (cum > target) { pick = j; break; }
  }
  emit_token(sh.id[pick], true, b, P, eos_ids, done, next, out);
}


// ---- n samples per prompt: cache fan-out ------------------------------------------------------------------------------------
constexpr int KR_MAX_X = 64;  // blocks along a slab (grid-stride beyond)

// One source row b of the cache -> rows b n .. b n + n - 1 (never onto itself). grid (x, nslab + 1): slab y < nslab is
// (layer, K | V, kv head) = [cap][hd] bf16 of which the first lens[b] keys are copied; y == nslab replicates lens and logits.
__global__ __launch_bounds__(256) void kv_repeat_kernel(bf16_t* __restrict__ kv, int* __restrict__ lens,
                                                        float* __restrict__ logits, int b, int n, int bmax, int nKV, int cap,
                                                        int hd, int nslab, int vocab) {
  const int len = lens[b];  // not a destination of this launch
  const int y = blockIdx.y;
  const int i0 = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
  if (y == nslab) {
    for (int i = i0; i < n; i += step)
      if (b * n + i != b) lens[b * n + i] = len;
    if (!logits) return;
    const float* src = logits + (size_t)b * vocab;
    for (int c = i0; c < vocab; c += step) {
      const float v = src[c];
      for (int i = 0; i < n; ++i)
        if (b * n + i != b) logits[(size_t)(b * n + i) * vocab + c] = v;
    }
    return;
  }
  const int lk = y / nKV, g = y % nKV;
  const size_t slab = (size_t)cap * hd;
  const uint4* src = reinterpret_cast<const uint4*>(kv + (((size_t)lk * bmax + b) * nKV + g) * slab);
  const int nv = min(max(len, 0), cap) * (hd / 8);
  for (int v = i0; v < nv; v += step) {
    const uint4 x = src[v];
    for (int i = 0; i < n; ++i) {
      const int r = b * n + i;
      if (r != b) reinterpret_cast<uint4*>(kv + (((size_t)lk * bmax + r) * nKV + g) * slab)[v] = x;
    }
  }
}

// ---- log-probability of a token -----------------------------------------------------------------------------------------------
// NaN -> -inf, +inf -> FLT_MAX: the sampler's reading of a score
SLAM_DEVICE float clean_score(float x) {
  if (x != x) x = -INFINITY;
  return fminf(x, FLT_MAX);
}

// scores [c0, c0 + n) of one row, cleaned, into LDS at their index in the chunk; the loads are those of load_keys
SLAM_DEVICE void load_scores(const float* __restrict__ row, int c0, int n, float* vals) {
  const float* p = row + c0;
  int head = (int)((4u - (uint32_t)(((uintptr_t)p >> 2) & 3u)) & 3u);
  if (head > n) head = n;
  const int nv = (n - head) >> 2;
  const int t = threadIdx.x;
  if (t < head) vals[t] = clean_score(p[t]);
  const float4* pv = reinterpret_cast<const float4*>(p + head);
  for (int v = t; v < nv; v += SP_THREADS) {
    const float4 f = pv[v];
    const int i = head + 4 * v;
    vals[i + 0] = clean_score(f.x);
    vals[i + 1] = clean_score(f.y);
    vals[i + 2] = clean_score(f.z);
    vals[i + 3] = clean_score(f.w);
  }
  for (int i = head + 4 * nv + t; i < n; i += SP_THREADS) vals[i] = clean_score(p[i]);
}

// m = max of vals[0 .. n), s = sum of expf(vals[i] - m) in the stated order (0 when m is -inf). Every thread of the block calls
// it and gets the same pair.
SLAM_DEVICE void chunk_max_sum(const float* vals, int n, float* red, float& m, float& s) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  float mx = -INFINITY;
  for (int i = t; i < n; i += SP_THREADS) mx = fmaxf(mx, vals[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float acc = 0.f;
  if (m != -INFINITY)
    for (int i = t; i < n; i += SP_THREADS) acc += expf(vals[i] - m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  s = ((red[0] + red[1]) + red[2]) + red[3];
}

// (m, S) of a row from stage 1's pairs p[0 .. nch), in chunk order. One thread calls it.
SLAM_DEVICE void combine_chunks(const float2* p, int nch, float& m, float& s) {
  m = -INFINITY;
  s = 0.f;
  for (int c = 0; c < nch; ++c) m = fmaxf(m, p[c].x);
  if (m != -INFINITY)
    for (int c = 0; c < nch; ++c)
      if (p[c].x != -INFINITY) s = __fmaf_rn(p[c].y, expf(p[c].x - m), s);  // one rounding, as the header states
}

struct LogprobParams {
  int vocab, nch, column;
  long long out_stride;
};

// stage 1, grid (chunks, B): (m_c, s_c) of the chunk into ws[b][chunk]
__global__ __launch_bounds__(SP_THREADS) void logprob_chunk_kernel(const float* __restrict__ logits,
                                                                   const uint8_t* __restrict__ finished, LogprobParams P,
                                                                   float2* __restrict__ ws) {
  __shared__ float vals[SP_CHUNK];
  __shared__ float red[SP_THREADS / 64];
  const int ch = blockIdx.x, b = blockIdx.y;
  if (finished && finished[b]) return;  // written by the second launch only
  const int c0 = ch * SP_CHUNK;
  const int n = min(SP_CHUNK, P.vocab - c0);
  load_scores(logits + (size_t)b * P.vocab, c0, n, vals);
  __syncthreads();
  float m, s;
  chunk_max_sum(vals, n, red, m, s);
  if (threadIdx.x == 0) ws[(size_t)b * P.nch + ch] = make_float2(m, s);
}

// one block per row. ROW: the row is one chunk, reduced here (SP_THREADS threads); else thread 0 combines stage 1's pairs.
template <bool ROW>
__global__ __launch_bounds__(SP_THREADS) void logprob_finish_kernel(const float* __restrict__ logits,
                                                                    const int64_t* __restrict__ tokens,
                                                                    const uint8_t* __restrict__ done,
                                                                    uint8_t* __restrict__ finished, float* __restrict__ out,
                                                                    LogprobParams P, const float2* __restrict__ ws) {
  __shared__ float vals[ROW ? SP_CHUNK : 1];
  __shared__ float red[SP_THREADS / 64];
  __shared__ int fin_s;
  const int b = blockIdx.x, t = threadIdx.x;
  if (t == 0) fin_s = finished && finished[b] ? 1 : 0;  // one read: thread 0 rewrites the flag below
  __syncthreads();
  const bool fin = fin_s != 0;
  const float* row = logits + (size_t)b * P.vocab;
  float m = -INFINITY, s = 0.f;
  if (!fin) {
    if (ROW) {
      load_scores(row, 0, P.vocab, vals);
      __syncthreads();
      chunk_max_sum(vals, P.vocab, red, m, s);
    } else if (t == 0) {
      combine_chunks(ws + (size_t)b * P.nch, P.nch, m, s);
    }
  }
  if (t != 0) return;
  float r = 0.f;
  if (!fin) {
    const long long tok = tokens[b];
    if (tok >= 0 && tok < P.vocab) r = m == -INFINITY ? -INFINITY : clean_score(row[tok]) - (m + logf(s));
  }
  out[(long long)b * P.out_stride + P.column] = r;
  if (finished) finished[b] = done ? done[b] : (uint8_t)0;
}

// ---- classifier-free guidance (slam_cfg_scores) --------------------------------------------------------------------------------
// One guided score from the cleaned pair (x, y) and the rows' log-normalisers. x_dead / y_dead: the row has no score above -inf.
// Three operations, each rounded on its own: a fused multiply-add would round g d + u once and change the bits.
SLAM_DEVICE float cfg_combine(float x, float y, float Lx, float Ly, float g, bool x_dead, bool y_dead) {
#pragma clang fp contract(off)
  if (x_dead) return -INFINITY;
  const float a = x - Lx;
  if (a == -INFINITY) return -INFINITY;
  if (y_dead) return a;
  const float u = y - Ly;
  if (u == -INFINITY) return a;
  const float d = a - u;
  const float gd = g * d;
  return gd + u;
}

struct CfgParams {
  int vocab, nch, B;
  float g;
};

// grid (chunks, B). Row b (x) and row B + b (y) of logits, chunk blockIdx.x, into scores row b. ROW: the rows are one chunk and
// their statistics are formed here; else thread 0 (x) and thread 64 (y) combine the pairs logprob_chunk_kernel left in ws for
// the 2 B rows. The chunk of both rows is staged in LDS by load_scores (16-byte loads from each row's own first 16-byte
// boundary) and leaves by 16-byte stores from the first 16-byte boundary of the scores row, 4-byte ones at the ragged ends.
template <bool ROW>
__global__ __launch_bounds__(SP_THREADS) void cfg_scores_kernel(const float* __restrict__ logits, float* __restrict__ scores,
                                                                CfgParams P, const float2* __restrict__ ws) {
  __shared__ float vx[SP_CHUNK];
  __shared__ float vy[SP_CHUNK];
  __shared__ float red[SP_THREADS / 64];
  __shared__ float st[4];
  const int ch = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const int c0 = ch * SP_CHUNK;
  const int n = min(SP_CHUNK, P.vocab - c0);
  load_scores(logits + (size_t)b * P.vocab, c0, n, vx);
  load_scores(logits + (size_t)(P.B + b) * P.vocab, c0, n, vy);
  __syncthreads();
  float mx, sx, my, sy;
  if (ROW) {
    chunk_max_sum(vx, n, red, mx, sx);
    __syncthreads();  // red is reused
    chunk_max_sum(vy, n, red, my, sy);
  } else {
    if (t == 0) combine_chunks(ws + (size_t)b * P.nch, P.nch, st[0], st[1]);
    if (t == 64) combine_chunks(ws + (size_t)(P.B + b) * P.nch, P.nch, st[2], st[3]);
    __syncthreads();
    mx = st[0], sx = st[1], my = st[2], sy = st[3];
  }
  const bool x_dead = mx == -INFINITY, y_dead = my == -INFINITY;
  const float Lx = mx + logf(sx), Ly = my + logf(sy);  // unused when the row is dead
  const float g = P.g;
  float* dst = scores + (size_t)b * P.vocab + c0;
  int head = (int)((4u - (uint32_t)(((uintptr_t)dst >> 2) & 3u)) & 3u);
  if (head > n) head = n;
  const int nv = (n - head) >> 2;
  if (t < head) dst[t] = cfg_combine(vx[t], vy[t], Lx, Ly, g, x_dead, y_dead);
  float4* dv = reinterpret_cast<float4*>(dst + head);
  for (int v = t; v < nv; v += SP_THREADS) {
    const int i = head + 4 * v;
    float4 f;
    f.x = cfg_combine(vx[i + 0], vy[i + 0], Lx, Ly, g, x_dead, y_dead);
    f.y = cfg_combine(vx[i + 1], vy[i + 1], Lx, Ly, g, x_dead, y_dead);
    f.z = cfg_combine(vx[i + 2], vy[i + 2], Lx, Ly, g, x_dead, y_dead);
    f.w = cfg_combine(vx[i + 3], vy[i + 3], Lx, Ly, g, x_dead, y_dead);
    dv[v] = f;
  }
  for (int i = head + 4 * nv + t; i < n; i += SP_THREADS) dst[i] = cfg_combine(vx[i], vy[i], Lx, Ly, g, x_dead, y_dead);
}

// next[B + b] = next[b]: the unconditional twins decode the token their conditional row drew
__global__ __launch_bounds__(256) void cfg_mirror_kernel(int64_t* next, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < B) next[B + b] = next[b];
}

// ---- per-row bans between the logits and the token choice (slam_constrain_scores) -------------------------------------------
// grid (chunks of SP_CHUNK, B). The block copies its chunk of the row bit for bit (skipped in place), then scans the row's
// history and stores -inf for the bans that fall inside its own chunk: no block writes into another's chunk, so there is no
// ordering between blocks, and the only stores behind the copy are of one constant (equal stores may race, harmlessly).
struct ConstrainParams {
  int vocab, step, ngram, n_per_prompt, prompt_stride, ban_eos, n_eos, n_begin, n_seqs, n_seq_tokens;
  long long new_stride;
};

// h[j] of a row: the prompt's real tokens, then the new ones
struct ConstrainHistory {
  const int64_t* prompt;
  const int64_t* fresh;
  int pl;
  SLAM_DEVICE long long at(int j) const { return j < pl ? prompt[j] : fresh[j - pl]; }
};

__global__ __launch_bounds__(SP_THREADS) void constrain_scores_kernel(
    const float* logits, float* scores, const int64_t* __restrict__ prompt, const int* __restrict__ prompt_len,
    const int64_t* __restrict__ fresh, const uint8_t* __restrict__ done, const int* __restrict__ eos_ids,
    const int* __restrict__ begin_ids, const int* __restrict__ seq_tokens, const int* __restrict__ seq_offsets,
    ConstrainParams P) {
  const int ch = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const int c0 = ch * SP_CHUNK;
  const int n = min(SP_CHUNK, P.vocab - c0);
  float* srow = scores + (size_t)b * P.vocab;
  if (logits != scores) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(logits + (size_t)b * P.vocab + c0);
    uint32_t* dst = reinterpret_cast<uint32_t*>(srow + c0);
    int head = 0, nv = 0;
    if ((((uintptr_t)src ^ (uintptr_t)dst) & 15) == 0) {  // equally aligned: 16-byte body, 4-byte ragged ends
      head = (int)((4u - (uint32_t)(((uintptr_t)src >> 2) & 3u)) & 3u);
      if (head > n) head = n;
      nv = (n - head) >> 2;
    }
    if (t < head) dst[t] = src[t];
    const uint4* sv = reinterpret_cast<const uint4*>(src + head);
    uint4* dv = reinterpret_cast<uint4*>(dst + head);
    for (int v = t; v < nv; v += SP_THREADS) dv[v] = sv[v];
    for (int i = head + 4 * nv + t; i < n; i += SP_THREADS) dst[i] = src[i];
    __syncthreads();  // the bans below land on words other threads of this block copied
  }
  if (done && done[b]) return;
  const int pb = b / P.n_per_prompt;
  ConstrainHistory h;
  h.pl = min(max(prompt_len[pb], 0), P.prompt_stride);
  h.prompt = prompt + (size_t)pb * P.prompt_stride;
  h.fresh = fresh + (long long)b * P.new_stride;  // dereferenced only for step > 0
  const int Lh = h.pl + P.step;
  const long long lo = c0, hi = c0 + n;  // a ban outside [lo, hi) is another block's, or nobody's
  const int ng = P.ngram;
  if (ng > 0 && Lh >= ng) {
    const int p0 = Lh - ng + 1;  // the last ng - 1 tokens
    for (int j = t; j <= Lh - ng; j += SP_THREADS) {
      bool eq = true;
      for (int k = 0; k < ng - 1 && eq; ++k) eq = h.at(j + k) == h.at(p0 + k);
      if (!eq) continue;
      const long long tok = h.at(j + ng - 1);
      if (tok >= lo && tok < hi) srow[tok] = -INFINITY;
    }
  }
  for (int i = t; i < P.n_seqs; i += SP_THREADS) {
    const int o0 = seq_offsets[i], o1 = seq_offsets[i + 1];
    if (o0 < 0 || o1 > P.n_seq_tokens || o1 - o0 < 2 || o1 - o0 > slam::CONSTRAIN_MAX_SEQ_LEN) continue;
    const int Lw = o1 - o0;
    if (Lw > Lh) continue;
    bool eq = true;
    for (int k = 0; k < Lw - 1 && eq; ++k) eq = h.at(Lh - (Lw - 1) + k) == (long long)seq_tokens[o0 + k];
    if (!eq) continue;
    const long long tok = seq_tokens[o1 - 1];
    if (tok >= lo && tok < hi) srow[tok] = -INFINITY;
  }
  if (P.ban_eos && t < P.n_eos) {
    const long long tok = eos_ids[t];
    if (tok >= lo && tok < hi) srow[tok] = -INFINITY;
  }
  if (P.step == 0)
    for (int i = t; i < P.n_begin; i += SP_THREADS) {
      const long long tok = begin_ids[i];
      if (tok >= lo && tok < hi) srow[tok] = -INFINITY;
    }
}

// ---- fused head + row statistics (slam_op_score_rows, slam_extend_score) -----------------------------------------------------
// x[m][i] = the fp32 accumulator of X row m against W row i; it lives in the accumulator registers only. The vocabulary is
// cut into chunks of SCORE_CHUNK columns, a chunk into SCORE_GROUPS groups of 64 consecutive columns. One block = 64 rows x
// one chunk; wave w forms groups 2 w and 2 w + 1 one after the other, a group as 4 column tiles x MT row tiles of
// v_mfma_f32_16x16x32_bf16 with both operands loaded 16 B per lane straight into the operand registers (the four waves read
// the same X rows: L1; the row blocks of one chunk are neighbours in the grid and read the same W rows: L2).
// Group statistics of a row, lane j of a 16-lane set holding columns j, 16 + j, 32 + j, 48 + j of the group:
//   m_g = max; s_g = ((((0 + e_j) + e_16+j) + e_32+j) + e_48+j) with e_i = expf(x_i - m_g), then the 16 lanes by the xor
//   butterfly 8, 4, 2, 1 (0 when m_g = -inf); best = the largest score, the lowest id among equals.
// Groups, then chunks, are combined in ascending order by score_merge: one fused multiply-add per part.
constexpr int SCORE_CHUNK = 512;
constexpr int SCORE_GROUPS = SCORE_CHUNK / 64;
constexpr int SCORE_U = 2;      // 32-deep K steps per unrolled group: 16 x 16 B loads in flight per lane
constexpr int SCORE_NONE = 0x7fffffff;  // id of "no score above -inf"

struct ScoreStat {
  float m, s, bv;
  int bi;
};

// parts in ascending order: (m, S) as the header states, best by strictly-greater (the earlier part holds the lower ids)
SLAM_DEVICE void score_merge(ScoreStat& a, float m_max, const float4& p) {
  if (p.x != -INFINITY) a.s = __fmaf_rn(p.y, expf(p.x - m_max), a.s);
  if (p.z > a.bv) { a.bv = p.z; a.bi = __float_as_int(p.w); }
}

// grid (ceil(M / 64), chunks), 256 threads. part[m][chunk] = (m_c, s_c, best value, best id as int bits); xt[m] = the cleaned,
// masked score of targets[m], written by the one lane of the grid that holds it.
template <int MT>
__global__ __launch_bounds__(256) void score_rows_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ W,
                                                         const int64_t* __restrict__ targets,
                                                         const uint8_t* __restrict__ colmask, int M, int V, int K, int nch,
                                                         float4* __restrict__ part, float* __restrict__ xt) {
  __shared__ float4 grp[SCORE_GROUPS][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = lane >> 4, j = lane & 15;
  const int m_base = blockIdx.x * 64;
  const int c0 = blockIdx.y * SCORE_CHUNK;
  const bf16_t* xrow[MT];
  bool xv[MT];
  int tgt[MT][4];  // the target column of row 16 t + 4 q + r, -1: none in [0, V)
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = m_base + 16 * t + j;
    xv[t] = m < M;
    xrow[t] = X + (size_t)(xv[t] ? m : 0) * K + 8 * q;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int mr = m_base + 16 * t + 4 * q + r;
      const long long tv = mr < M ? (long long)targets[mr] : -1;
      tgt[t][r] = tv >= 0 && tv < V ? (int)tv : -1;
    }
  }
  const uint4 zero = {0u, 0u, 0u, 0u};
  for (int p = 0; p < 2; ++p) {
    const int g = 2 * wave + p;
    const int g0 = c0 + 64 * g;
    if (g0 >= V) {  // wave-uniform: a group past the vocabulary holds no score
      grp[g][lane] = make_float4(-INFINITY, 0.f, -INFINITY, __int_as_float(SCORE_NONE));
      continue;
    }
    size_t woff[4];  // element offset of this lane's 8 W values at k = 0
    unsigned dead = 0;  // bit nt: column g0 + 16 nt + j is past the vocabulary or masked
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int n = g0 + 16 * nt + j;
      const int nr = min(n, V - 1);  // tail columns re-read the last row; their scores count as -inf
      woff[nt] = (size_t)nr * K + 8 * q;
      if (n >= V || (colmask && colmask[nr])) dead |= 1u << nt;
    }
    f32x4_t acc[MT][4];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) acc[t][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += 32 * SCORE_U) {
      uint4 w[SCORE_U][4], a[SCORE_U][MT];
#pragma unroll
      for (int u = 0; u < SCORE_U; ++u) {
        const int k = k0 + 32 * u;
        const bool kv = k + 8 * q < K;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) w[u][nt] = kv ? *reinterpret_cast<const uint4*>(W + woff[nt] + k) : zero;
#pragma unroll
        for (int t = 0; t < MT; ++t) a[u][t] = (kv && xv[t]) ? *reinterpret_cast<const uint4*>(xrow[t] + k) : zero;
      }
#pragma unroll
      for (int u = 0; u < SCORE_U; ++u)
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) acc[t][nt] = mfma16(a[u][t], w[u][nt], acc[t][nt]);
    }
    // lane holds acc[t][nt][r] = x[m_base + 16 t + 4 q + r][g0 + 16 nt + j]
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m_base + 16 * t + 4 * q + r;
        float x[4];
        float mg = -INFINITY, bv = -INFINITY;
        int bi = SCORE_NONE;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const int n = g0 + 16 * nt + j;
          x[nt] = (dead >> nt) & 1u ? -INFINITY : clean_score(acc[t][nt][r]);
          mg = fmaxf(mg, x[nt]);
          if (x[nt] > bv) { bv = x[nt]; bi = n; }
          if (tgt[t][r] == n) xt[m] = x[nt];
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {
          mg = fmaxf(mg, __shfl_xor(mg, o, 64));
          const float ov = __shfl_xor(bv, o, 64);
          const int oi = __shfl_xor(bi, o, 64);
          if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        float s = 0.f;
        if (mg != -INFINITY) {
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) s += expf(x[nt] - mg);
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (j == 0) grp[g][16 * t + 4 * q + r] = make_float4(mg, s, bv, __int_as_float(bi));
      }
  }
  __syncthreads();
  const int row = threadIdx.x, m = m_base + row;
  if (row >= 16 * MT || m >= M) return;
  float mc = -INFINITY;
#pragma unroll
  for (int g = 0; g < SCORE_GROUPS; ++g) mc = fmaxf(mc, grp[g][row].x);
  ScoreStat a = {mc, 0.f, -INFINITY, SCORE_NONE};
#pragma unroll
  for (int g = 0; g < SCORE_GROUPS; ++g) score_merge(a, mc, grp[g][row]);
  part[(size_t)m * nch + blockIdx.y] = make_float4(a.m, a.s, a.bv, __int_as_float(a.bi));
}

// one thread per row: the chunks in chunk order. Plain form (new_lens == nullptr): lp[m], argmax[m]. Chunk form (slam_extend_score;
// row m = b T + t): lp[b T + t + 1] for t + 1 < T, the log-prob when t + 1 < new_lens[b] and 0 else - column 0 is never
// written; argmax[b T + t] = -1 for t >= new_lens[b].
__global__ __launch_bounds__(256) void score_finish_kernel(const float4* __restrict__ part, const float* __restrict__ xt,
                                                           const int64_t* __restrict__ targets, int M, int V, int nch,
                                                           const int* __restrict__ new_lens, int T, float* __restrict__ lp,
                                                           int64_t* __restrict__ argmax) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const float4* p = part + (size_t)m * nch;
  float mm = -INFINITY;
  for (int c = 0; c < nch; ++c) mm = fmaxf(mm, p[c].x);
  ScoreStat a = {mm, 0.f, -INFINITY, SCORE_NONE};
  for (int c = 0; c < nch; ++c) score_merge(a, mm, p[c]);
  const long long tok = targets[m];
  float r = 0.f;
  if (tok >= 0 && tok < V) r = mm == -INFINITY ? -INFINITY : xt[m] - (mm + logf(a.s));
  const long long best = a.bv == -INFINITY ? -1 : (long long)a.bi;
  if (!new_lens) {
    lp[m] = r;
    if (argmax) argmax[m] = best;
    return;
  }
  const int b = m / T, t = m % T;
  const int nl = min(max(new_lens[b], 0), T);
  if (t + 1 < T) lp[m + 1] = t + 1 < nl ? r : 0.f;
  if (argmax) argmax[m] = t < nl ? best : -1;
}

// targets of the chunk's rows: row b T + t scores ids[b][t + 1] when that is a real token of the chunk, nothing (-100) else
__global__ __launch_bounds__(256) void extend_targets_kernel(const int64_t* __restrict__ ids, const int* __restrict__ new_lens,
                                                             int64_t* __restrict__ tg, int B, int T) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * T) return;
  const int b = i / T, t = i % T;
  const int nl = min(max(new_lens[b], 0), T);
  tg[i] = t + 1 < nl ? ids[i + 1] : -100;
}

}  // namespace

namespace slam {

size_t gemm_skinny_workspace_bytes(int M, int N, int K) {
  const SkinnyPlan p = skinny_plan(M, N, K, (size_t)-1);
  return p.splits > 1 ? (size_t)p.splits * M * N * sizeof(float) : 0;
}

int gemm_skinny(const bf16_t* X, const bf16_t* W, bf16_t* Y, float* Yf, const bf16_t* bias, const bf16_t* resid, int M, int N,
                int K, float* ws, size_t ws_bytes, hipStream_t st) {
  if (M <= 0 || N <= 0 || K <= 0 || (K & 7) || (!Y == !Yf)) return -1;
  if (((uintptr_t)X | (uintptr_t)W) & 15) return -1;
  if (Yf) return launch_skinny<true>(X, W, Yf, bias, resid, M, N, K, ws, ws_bytes, st);
  return launch_skinny<false>(X, W, Y, bias, resid, M, N, K, ws, ws_bytes, st);
}

int gemm_skinny_w8(const bf16_t* X, const uint8_t* Q, const int8_t* E, bf16_t* Y, float* Yf, const bf16_t* bias,
                   const bf16_t* resid, int M, int N, int K, float* ws, size_t ws_bytes, hipStream_t st) {
  if (!E || M <= 0 || N <= 0 || K <= 0 || (K % W8_K_GRAIN) || (!Y == !Yf)) return -1;
  if (((uintptr_t)X | (uintptr_t)Q) & 15) return -1;
  if (Yf) return launch_skinny_w8<true>(X, Q, E, Yf, bias, resid, M, N, K, ws, ws_bytes, st);
  return launch_skinny_w8<false>(X, Q, E, Y, bias, resid, M, N, K, ws, ws_bytes, st);
}

size_t attn_decode_part_bytes(int B, int nH, int head_dim, int ns) {
  return (size_t)B * nH * ns * (head_dim + 2) * sizeof(float);
}

// keys per split: multiples of 64, about 512 blocks over (splits, KV heads, rows), more keys per split when the partials
// would not fit in part_bytes
int attn_decode_chunk(int B, int nH, int nKV, int head_dim, int kv_bound, size_t part_bytes) {
  const int target = 512 / (B * nKV) > 1 ? 512 / (B * nKV) : 1;
  int chunk = ((kv_bound + target - 1) / target + 63) / 64 * 64;
  if (chunk < 64) chunk = 64;
  while (attn_decode_part_bytes(B, nH, head_dim, (kv_bound + chunk - 1) / chunk) > part_bytes) {
    if (chunk >= kv_bound) return -1;
    chunk *= 2;
  }
  return chunk;
}

int attn_decode(const float* qkv, const bf16_t* bias, const float* cs, const float* sn, const float* csq, const float* snq,
                const int* lens, bf16_t* kc, bf16_t* vc, int cap, int B, int nH, int nKV, int head_dim, int kv_bound, bf16_t* o,
                float* part, size_t part_bytes, hipStream_t st) {
  if (B <= 0 || nKV <= 0 || nH % nKV || kv_bound <= 0 || kv_bound > cap) return -1;
  const int G = nH / nKV;
  if ((head_dim != 64 && head_dim != 128) || G > 8) return -1;
  const int chunk = attn_decode_chunk(B, nH, nKV, head_dim, kv_bound, part_bytes);
  if (chunk <= 0) return -3;
  const int ns = (kv_bound + chunk - 1) / chunk;
  const dim3 grid(ns, nKV, B);
#define AD_CASE(HD, GG)                                                                                                  \
  case GG:                                                                                                               \
    attn_decode_kernel<HD, GG><<<grid, 256, 0, st>>>(qkv, bias, cs, sn, csq, snq, lens, kc, vc, cap, nH, nKV, chunk, ns, \
                                                     part);                                                              \
    break;
#define AD_SWITCH(HD) \
  switch (G) { AD_CASE(HD, 1) AD_CASE(HD, 2) AD_CASE(HD, 3) AD_CASE(HD, 4) AD_CASE(HD, 5) AD_CASE(HD, 6) AD_CASE(HD, 7) AD_CASE(HD, 8) }
  if (head_dim == 64) {
    AD_SWITCH(64)
    attn_decode_combine_kernel<64><<<dim3(nH, B), 64, 0, st>>>(part, ns, nH, o);
  } else {
    AD_SWITCH(128)
    attn_decode_combine_kernel<128><<<dim3(nH, B), 128, 0, st>>>(part, ns, nH, o);
  }
#undef AD_SWITCH
#undef AD_CASE
  return (int)hipGetLastError();
}

int kv_scatter(const bf16_t* qkv, bf16_t* kc, bf16_t* vc, const int* lens, int B, int T, int nH, int nKV, int head_dim, int cap,
               hipStream_t st) {
  const size_t n = (size_t)T * (2 * nKV * head_dim / 8);
  kv_scatter_kernel<<<dim3(nblk(n, 256), B), 256, 0, st>>>(qkv, kc, vc, lens, T, nH, nKV, head_dim, cap);
  return (int)hipGetLastError();
}

int gather_last_rows(const bf16_t* src, bf16_t* dst, const int* lens, int B, int T, int H, hipStream_t st) {
  if (H & 7) return -1;
  gather_last_kernel<<<nblk((size_t)B * (H / 8), 256), 256, 0, st>>>(src, dst, lens, B, T, H);
  return (int)hipGetLastError();
}

int lens_to_pos(const int* lens, int64_t* pos, int B, hipStream_t st) {
  lens_to_pos_kernel<<<nblk((size_t)B, 256), 256, 0, st>>>(lens, pos, B);
  return (int)hipGetLastError();
}

int lens_inc(int* lens, int B, hipStream_t st) {
  lens_inc_kernel<<<nblk((size_t)B, 256), 256, 0, st>>>(lens, B);
  return (int)hipGetLastError();
}

size_t attn_extend_part_bytes(int B, int T, int nH, int head_dim, int ns) {
  return ns > 1 ? (size_t)B * T * nH * ns * (head_dim + 4) * sizeof(float) : 0;
}

// keys per split: multiples of 64, about 512 blocks over (query tiles, splits, KV heads, rows); more keys per split when the
// partials would not fit in part_bytes, down to one split, which needs none
int attn_extend_chunk(int B, int T, int nH, int nKV, int head_dim, int kv_bound, size_t part_bytes) {
  const int64_t tiles = (int64_t)B * nKV * ((T + 15) / 16);
  const int target = 512 / tiles > 1 ? (int)(512 / tiles) : 1;
  int chunk = ((kv_bound + target - 1) / target + 63) / 64 * 64;
  if (chunk < 64) chunk = 64;
  while (attn_extend_part_bytes(B, T, nH, head_dim, (kv_bound + chunk - 1) / chunk) > part_bytes) chunk *= 2;
  return chunk;
}

int attn_extend(const bf16_t* qkv, const int* base_lens, const int* new_lens, bf16_t* kc, bf16_t* vc, int cap, int B, int T,
                int nH, int nKV, int head_dim, int kv_bound, bf16_t* o, float* part, size_t part_bytes, hipStream_t st) {
  if (B <= 0 || T <= 0 || nKV <= 0 || nH % nKV || kv_bound <= 0 || kv_bound > cap) return -1;
  const int G = nH / nKV;
  if ((head_dim != 64 && head_dim != 128) || G > 8) return -1;
  if ((int64_t)B * nKV > 65535 || T > 65535 || (int64_t)B * T > 0x7fffffffLL / (nH * (head_dim + 4))) return -1;
  if (((uintptr_t)qkv | (uintptr_t)kc | (uintptr_t)vc | (uintptr_t)o | (uintptr_t)part) & 15) return -1;
  const int chunk = attn_extend_chunk(B, T, nH, nKV, head_dim, kv_bound, part ? part_bytes : 0);
  const int ns = (kv_bound + chunk - 1) / chunk;
  if (ns > 65535) return -1;
  float* pp = ns > 1 ? part : nullptr;
  const size_t n = (size_t)T * (2 * nKV * head_dim / 8);
  kv_extend_scatter_kernel<<<dim3(nblk(n, 256), B), 256, 0, st>>>(qkv, kc, vc, base_lens, new_lens, T, nH, nKV, head_dim, cap,
                                                                  kv_bound);
  const dim3 grid((T + 15) / 16, ns, B * nKV);
#define AE_CASE(HD, GG)                                                                                                      \
  case GG:                                                                                                                   \
    attn_extend_kernel<HD, GG><<<grid, 256, 0, st>>>(qkv, base_lens, new_lens, kc, vc, o, pp, T, nH, nKV, cap, kv_bound, chunk, \
                                                     ns);                                                                    \
    break;
#define AE_SWITCH(HD) \
  switch (G) { AE_CASE(HD, 1) AE_CASE(HD, 2) AE_CASE(HD, 3) AE_CASE(HD, 4) AE_CASE(HD, 5) AE_CASE(HD, 6) AE_CASE(HD, 7) AE_CASE(HD, 8) }
  if (head_dim == 64) {
    AE_SWITCH(64)
    if (pp) attn_extend_combine_kernel<64><<<dim3(nH, T, B), 64, 0, st>>>(pp, base_lens, new_lens, T, nH, kv_bound, chunk, ns, o);
  } else {
    AE_SWITCH(128)
    if (pp) attn_extend_combine_kernel<128><<<dim3(nH, T, B), 128, 0, st>>>(pp, base_lens, new_lens, T, nH, kv_bound, chunk, ns, o);
  }
#undef AE_SWITCH
#undef AE_CASE
  return (int)hipGetLastError();
}

int extend_positions(const int* lens, int64_t* pos, int B, int T, hipStream_t st) {
  extend_pos_kernel<<<nblk((size_t)B * T, 256), 256, 0, st>>>(lens, pos, B, T);
  return (int)hipGetLastError();
}

int extend_finish(const float* src, float* dst, const int* new_lens, int* lens, int B, int T, int vocab, hipStream_t st) {
  if (B <= 0 || B > 65535) return -1;
  unsigned gx = nblk((size_t)vocab, 256);
  if (gx > 64) gx = 64;
  extend_finish_kernel<<<dim3(gx, B), 256, 0, st>>>(src, dst, new_lens, lens, T, vocab);
  return (int)hipGetLastError();
}

int extend_store_rows(const float* src, float* dst, const int* new_lens, int m0, int rows, int B, int T, int vocab,
                      hipStream_t st) {
  if (rows <= 0 || rows > 65535 || m0 < 0 || T <= 0 || (int64_t)m0 + rows > (int64_t)B * T) return -1;
  unsigned gx = nblk((size_t)vocab, 256);
  if (gx > 64) gx = 64;
  extend_store_rows_kernel<<<dim3(gx, rows), 256, 0, st>>>(src, dst, new_lens, m0, T, vocab);
  return (int)hipGetLastError();
}

int lens_add(int* lens, const int* new_lens, int B, int T, hipStream_t st) {
  lens_add_kernel<<<nblk((size_t)B, 256), 256, 0, st>>>(lens, new_lens, B, T);
  return (int)hipGetLastError();
}

int spec_accept(const SpecArgs& a, hipStream_t st) {
  if (!a.chunk || !a.tgt || !a.prompt_len || !a.n_new || !a.done || !a.out || !a.lens_t || !a.lens_d || !a.draft_ids ||
      !a.draft_new_lens || !a.tgt_new_lens || !a.stats)
    return -1;
  if (a.B < 1 || a.B > SPEC_MAX_B || a.K < 1 || a.K > SPEC_MAX_K || a.n_eos < 0 || a.n_eos > 16 || (a.n_eos > 0 && !a.eos_ids))
    return -1;
  if (a.max_new < 1 || a.out_stride < a.max_new) return -1;
  SpecParams P;
  P.B = a.B;
  P.K = a.K;
  P.max_new = a.max_new;
  P.pad_id = a.pad_id;
  P.n_eos = a.n_eos;
  P.out_stride = a.out_stride;
  spec_accept_kernel<<<1, 1024, 0, st>>>(a.chunk, a.tgt, a.eos_ids, a.prompt_len, a.n_new, a.done, a.out, a.lens_t, a.lens_d,
                                          a.draft_ids, a.draft_new_lens, a.tgt_new_lens, a.stats, P);
  return (int)hipGetLastError();
}

int ngram_propose(const NgramArgs& a, hipStream_t st) {
  if (!a.chunk || !a.n_prop || !a.prompt || !a.prompt_len || !a.fresh || !a.n_new || !a.done) return -1;
  if (a.B < 1 || a.B > SPEC_MAX_B || a.K < 1 || a.K > SPEC_MAX_K || a.max_ngram < 1 || a.max_ngram > NGRAM_MAX) return -1;
  if (a.n_eos < 0 || a.n_eos > 16 || (a.n_eos > 0 && !a.eos_ids)) return -1;
  if (a.prompt_stride < 0 || a.prompt_stride > NGRAM_MAX_STRIDE || a.new_stride < 0 || a.new_stride > NGRAM_MAX_STRIDE) return -1;
  NgramParams P;
  P.K = a.K;
  P.max_ngram = a.max_ngram;
  P.fill_id = a.fill_id;
  P.n_eos = a.n_eos;
  P.prompt_stride = a.prompt_stride;
  P.new_stride = a.new_stride;
  ngram_propose_kernel<<<a.B, NG_THREADS, 0, st>>>(a.chunk, a.n_prop, a.prompt, a.prompt_len, a.fresh, a.n_new, a.done,
                                                   a.eos_ids, P);
  if (a.stats) ngram_stats_kernel<<<1, 1024, 0, st>>>(a.n_prop, a.B, a.stats);
  return (int)hipGetLastError();
}


static int sample_chunks(int vocab) { return (vocab + SP_CHUNK - 1) / SP_CHUNK; }

size_t sample_workspace_bytes(int B, int vocab, int top_k) {
  if (B <= 0 || vocab <= 0) return 0;
  const int k = top_k < 1 ? 1 : top_k;
  return (size_t)B * sample_chunks(vocab) * k * sizeof(u64_t);
}

int sample_tokens(const SampleArgs& a, hipStream_t st) {
  if (!a.logits || !a.next || a.B <= 0 || a.B > 65535 || a.vocab <= 0 || ((uintptr_t)a.logits & 3)) return -1;
  const int k = a.do_sample ? a.top_k : 1;
  if (k < 1 || k > SP_MAXK || !(a.temperature > 0.f) || !(a.top_p > 0.f) || a.top_p > 1.f) return -1;
  if (a.n_eos < 0 || (a.n_eos > 0 && !a.eos_ids)) return -1;
  if (a.group < 1 || a.B % a.group != 0) return -1;
  if (!a.ws || ((uintptr_t)a.ws & 7) || a.ws_bytes < sample_workspace_bytes(a.B, a.vocab, k)) return -1;
  // the negated forms refuse NaN
  if (!(a.min_p >= 0.f && a.min_p <= 1.f) || !(a.typical_p > 0.f && a.typical_p <= 1.f)) return -1;
  if (!(a.epsilon_cutoff >= 0.f && a.epsilon_cutoff < 1.f) || !(a.eta_cutoff >= 0.f && a.eta_cutoff < 1.f)) return -1;
  const bool warped = a.do_sample && (a.min_p > 0.f || a.typical_p < 1.f || a.epsilon_cutoff > 0.f || a.eta_cutoff > 0.f);
  WarpSampleParams P;
  P.min_p = a.min_p;
  P.typical_p = a.typical_p;
  P.eps_cut = a.epsilon_cutoff;
  P.eta_cut = a.eta_cutoff;
  P.do_sample = a.do_sample ? 1 : 0;
  P.k = k;
  P.vocab = a.vocab;
  P.idbits = 1;
  while (P.idbits < 31 && (1u << P.idbits) < (uint32_t)a.vocab) ++P.idbits;
  P.nch = sample_chunks(a.vocab);
  P.pad_id = a.pad_id;
  P.n_eos = a.n_eos;
  P.inv_t = 1.0f / a.temperature;
  P.top_p = a.top_p;
  P.k0 = (uint32_t)a.seed;
  P.k1 = (uint32_t)(a.seed >> 32);
  P.step = a.step;
  P.out_stride = a.out_stride;
  P.out_col = a.out_col >= 0 ? a.out_col : (long long)a.step;
  P.group = a.group;
  u64_t* ws = reinterpret_cast<u64_t*>(a.ws);
  if (warped) {  // stage 1 is the plain call's; the chain runs behind the ranking of the finish kernel
    if (P.nch == 1) {
      sample_finish_kernel<true, true><<<a.B, SP_THREADS, 0, st>>>(a.logits, a.banned, a.row_ids, a.eos_ids, a.done, a.next, a.out, P, ws, a.steps);
    } else {
      sample_select_kernel<<<dim3(P.nch, a.B), SP_THREADS, 0, st>>>(a.logits, a.banned, a.done, P, ws);
      sample_finish_kernel<false, true><<<a.B, SP_THREADS, 0, st>>>(a.logits, a.banned, a.row_ids, a.eos_ids, a.done, a.next, a.out, P, ws, a.steps);
    }
    return (int)hipGetLastError();
  }
  if (P.nch == 1) {
    sample_finish_kernel<true><<<a.B, SP_THREADS, 0, st>>>(a.logits, a.banned, a.row_ids, a.eos_ids, a.done, a.next, a.out, P, ws, a.steps);
  } else {
    sample_select_kernel<<<dim3(P.nch, a.B), SP_THREADS, 0, st>>>(a.logits, a.banned, a.done, P, ws);
    sample_finish_kernel<false><<<a.B, SP_THREADS, 0, st>>>(a.logits, a.banned, a.row_ids, a.eos_ids, a.done, a.next, a.out, P, ws, a.steps);
  }
  return (int)hipGetLastError();
}

int constrain_scores(const ConstrainArgs& a, hipStream_t st) {
  if (!a.logits || !a.scores || !a.prompt || !a.prompt_len || a.B <= 0 || a.B > 65535 || a.vocab <= 0) return -1;
  if (((uintptr_t)a.logits | (uintptr_t)a.scores | (uintptr_t)a.prompt_len) & 3 || ((uintptr_t)a.prompt | (uintptr_t)a.fresh) & 7)
    return -1;
  if (a.step < 0 || a.step > CONSTRAIN_MAX_HISTORY || a.prompt_stride < 0 || a.prompt_stride > CONSTRAIN_MAX_HISTORY) return -1;
  if (a.step > 0 && (!a.fresh || a.new_stride < a.step)) return -1;
  if (a.ngram < 0 || a.n_per_prompt < 1 || a.B % a.n_per_prompt) return -1;
  if (a.n_eos < 0 || a.n_eos > 16 || (a.n_eos > 0 && (!a.eos_ids || ((uintptr_t)a.eos_ids & 3)))) return -1;
  if (a.n_begin < 0 || a.n_begin > CONSTRAIN_MAX_BEGIN || (a.n_begin > 0 && (!a.begin_ids || ((uintptr_t)a.begin_ids & 3)))) return -1;
  if (a.n_seqs < 0 || a.n_seqs > CONSTRAIN_MAX_SEQS || a.n_seq_tokens < 0 || a.n_seq_tokens > CONSTRAIN_MAX_SEQS * CONSTRAIN_MAX_SEQ_LEN)
    return -1;
  if (a.n_seqs > 0 && (!a.seq_tokens || !a.seq_offsets || (((uintptr_t)a.seq_tokens | (uintptr_t)a.seq_offsets) & 3))) return -1;
  ConstrainParams P;
  P.vocab = a.vocab;
  P.step = a.step;
  P.ngram = a.ngram;
  P.n_per_prompt = a.n_per_prompt;
  P.prompt_stride = a.prompt_stride;
  P.ban_eos = a.ban_eos ? 1 : 0;
  P.n_eos = a.n_eos;
  P.n_begin = a.n_begin;
  P.n_seqs = a.n_seqs;
  P.n_seq_tokens = a.n_seq_tokens;
  P.new_stride = a.new_stride;
  constrain_scores_kernel<<<dim3(sample_chunks(a.vocab), a.B), SP_THREADS, 0, st>>>(
      a.logits, a.scores, a.prompt, a.prompt_len, a.fresh, a.done, a.eos_ids, a.begin_ids, a.seq_tokens, a.seq_offsets, P);
  return (int)hipGetLastError();
}

int kv_repeat(bf16_t* kv, int* lens, float* logits, int B, int n, int bmax, int L, int nKV, int head_dim, int cap, int kv_bound,
              int vocab, hipStream_t st) {
  if (!kv || !lens || B <= 0 || n < 1 || (int64_t)B * n > bmax || (head_dim & 7) || kv_bound <= 0 || kv_bound > cap) return -1;
  if (n == 1) return 0;
  const int nslab = L * 2 * nKV;
  if (nslab + 1 > 65535) return -1;
  size_t per = (size_t)kv_bound * (head_dim / 8);
  if (logits && (size_t)vocab > per) per = (size_t)vocab;
  unsigned gx = nblk(per, 256);
  if (gx > (unsigned)KR_MAX_X) gx = KR_MAX_X;
  for (int b = B - 1; b >= 0; --b)  // descending: see the header comment
    kv_repeat_kernel<<<dim3(gx, nslab + 1), 256, 0, st>>>(kv, lens, logits, b, n, bmax, nKV, cap, head_dim, nslab, vocab);
  return (int)hipGetLastError();
}

size_t token_logprobs_workspace_bytes(int B, int vocab) {
  if (B <= 0 || vocab <= 0) return 0;
  return (size_t)B * sample_chunks(vocab) * sizeof(float2);
}

int token_logprobs(const float* logits, int B, int vocab, const int64_t* tokens, const uint8_t* done, uint8_t* finished,
                   float* out, int64_t out_stride, int column, void* ws, size_t ws_bytes, hipStream_t st) {
  if (!logits || !tokens || !out || B <= 0 || B > 65535 || vocab <= 0 || ((uintptr_t)logits & 3)) return -1;
  if (!ws || ((uintptr_t)ws & 7) || ws_bytes < token_logprobs_workspace_bytes(B, vocab)) return -1;
  LogprobParams P;
  P.vocab = vocab;
  P.nch = sample_chunks(vocab);
  P.column = column;
  P.out_stride = out_stride;
  float2* w = reinterpret_cast<float2*>(ws);
  if (P.nch == 1) {
    logprob_finish_kernel<true><<<B, SP_THREADS, 0, st>>>(logits, tokens, done, finished, out, P, w);
  } else {
    logprob_chunk_kernel<<<dim3(P.nch, B), SP_THREADS, 0, st>>>(logits, finished, P, w);
    logprob_finish_kernel<false><<<B, 64, 0, st>>>(logits, tokens, done, finished, out, P, w);
  }
  return (int)hipGetLastError();
}

size_t cfg_workspace_bytes(int B, int vocab) {
  if (B <= 0 || 2 * (int64_t)B > 65535 || vocab <= 0) return 0;
  return (size_t)2 * B * sample_chunks(vocab) * sizeof(float2);
}

int cfg_scores(const float* logits, int B, int vocab, float g, float* scores, void* ws, size_t ws_bytes, hipStream_t st) {
  if (!logits || !scores || !ws || B <= 0 || 2 * (int64_t)B > 65535 || vocab <= 0 || !isfinite(g)) return -1;
  if ((((uintptr_t)logits | (uintptr_t)scores) & 3) || ((uintptr_t)ws & 7) || ws_bytes < cfg_workspace_bytes(B, vocab)) return -1;
  const uintptr_t l0 = (uintptr_t)logits, s0 = (uintptr_t)scores;
  const size_t row = (size_t)vocab * sizeof(float);
  if (l0 < s0 + (size_t)B * row && s0 < l0 + (size_t)2 * B * row) return -1;  // the raw rows are read again afterwards
  CfgParams P;
  P.vocab = vocab;
  P.nch = sample_chunks(vocab);
  P.B = B;
  P.g = g;
  float2* w = reinterpret_cast<float2*>(ws);
  if (P.nch == 1) {
    cfg_scores_kernel<true><<<dim3(1, B), SP_THREADS, 0, st>>>(logits, scores, P, w);
  } else {
    LogprobParams L;
    L.vocab = vocab;
    L.nch = P.nch;
    L.column = 0;
    L.out_stride = 0;
    logprob_chunk_kernel<<<dim3(P.nch, 2 * B), SP_THREADS, 0, st>>>(logits, nullptr, L, w);
    cfg_scores_kernel<false><<<dim3(P.nch, B), SP_THREADS, 0, st>>>(logits, scores, P, w);
  }
  return (int)hipGetLastError();
}

int cfg_mirror_tokens(int64_t* next, int B, hipStream_t st) {
  if (!next || ((uintptr_t)next & 7) || B < 1 || B > 32767) return -1;
  cfg_mirror_kernel<<<nblk((size_t)B, 256), 256, 0, st>>>(next, B);
  return (int)hipGetLastError();
}

static int score_chunks(int V) { return (V + SCORE_CHUNK - 1) / SCORE_CHUNK; }

size_t score_rows_workspace_bytes(int M, int V) {
  if (M <= 0 || V <= 0 || M > SCORE_MAX_M || V > SCORE_MAX_V) return 0;
  return (size_t)M * score_chunks(V) * sizeof(float4) + (size_t)M * sizeof(float);
}

int score_rows(const bf16_t* X, const bf16_t* W, const int64_t* targets, const uint8_t* colmask, int M, int V, int K,
               const int* new_lens, int T, float* lp, int64_t* argmax, void* ws, size_t ws_bytes, hipStream_t st) {
  if (!X || !W || !targets || !lp || !ws || M <= 0 || M > SCORE_MAX_M || V <= 0 || V > SCORE_MAX_V || K <= 0 || (K & 7)) return -1;
  if (((uintptr_t)X | (uintptr_t)W | (uintptr_t)ws) & 15) return -1;
  if (((uintptr_t)targets | (uintptr_t)argmax) & 7 || ((uintptr_t)lp & 3)) return -1;
  if (ws_bytes < score_rows_workspace_bytes(M, V)) return -1;
  if (new_lens && (T <= 0 || M % T)) return -1;
  const int nch = score_chunks(V);
  float4* part = reinterpret_cast<float4*>(ws);
  float* xt = reinterpret_cast<float*>(part + (size_t)M * nch);
  const dim3 grid(nblk((size_t)M, 64), nch);
  const int mt = ((M < 64 ? M : 64) + 15) / 16;
#define SR_CASE(MT) \
  case MT: score_rows_kernel<MT><<<grid, 256, 0, st>>>(X, W, targets, colmask, M, V, K, nch, part, xt); break;
  switch (mt) {
    SR_CASE(1)
    SR_CASE(2)
    SR_CASE(3)
    default: score_rows_kernel<4><<<grid, 256, 0, st>>>(X, W, targets, colmask, M, V, K, nch, part, xt); break;
  }
#undef SR_CASE
  score_finish_kernel<<<nblk((size_t)M, 256), 256, 0, st>>>(part, xt, targets, M, V, nch, new_lens, T, lp, argmax);
  return (int)hipGetLastError();
}

int extend_targets(const int64_t* ids, const int* new_lens, int64_t* tg, int B, int T, hipStream_t st) {
  extend_targets_kernel<<<nblk((size_t)B * T, 256), 256, 0, st>>>(ids, new_lens, tg, B, T);
  return (int)hipGetLastError();
}

}  // namespace slam
