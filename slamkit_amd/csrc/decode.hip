// KV-cached generation kernels: the cache forward (slam_prefill / slam_decode_step / slam_extend*, include/slam_engine.h).
// What chooses the next token from the logits is sampling.hip.
//  * gemm_skinny: Y[M][N] = X[M][K] W[N][K]^T for a handful of rows. A decode step reads every weight once, so the launch is
//    a weight stream: each wave owns 16 W rows over a K range, loads them 16 B per lane straight into the B operand of
//    v_mfma_f32_16x16x32_bf16 (X rows padded to 16 form the A operand), and splits K until the grid covers the chip. The
//    split-K partials are summed in split order by a second launch: no atomics, the same bits every run.
//  * attn_decode: bias + RoPE of the new token's q / k on the fp32 projection (one rounding, the forward's tables and query
//    pre-scale), K / V appended to the cache, split-KV flash decoding with every query head of a KV group in one pass over the
//    group's keys, partial (m, l, o) merged in the log2 domain by attn_decode_combine in split order.
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

// NaN -> -inf, +inf -> FLT_MAX: the sampler's reading of a score (sampling.hip's clean_score, word for word)
SLAM_DEVICE float clean_score(float x) {
  if (x != x) x = -INFINITY;
  return fminf(x, FLT_MAX);
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
