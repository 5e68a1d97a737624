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
#include "decode_attn.h"
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
  return attn_decode_launch<false>(qkv, bias, cs, sn, csq, snq, lens, kc, vc, nullptr, nullptr, cap, B, nH, nKV, head_dim, kv_bound,
                                   o, part, part_bytes, st);
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

int kv_extend_scatter(const bf16_t* qkv, bf16_t* kc, bf16_t* vc, const int* base_lens, const int* new_lens, int B, int T, int nH,
                      int nKV, int head_dim, int cap, int kv_bound, hipStream_t st) {
  const size_t n = (size_t)T * (2 * nKV * head_dim / 8);
  kv_extend_scatter_kernel<<<dim3(nblk(n, 256), B), 256, 0, st>>>(qkv, kc, vc, base_lens, new_lens, T, nH, nKV, head_dim, cap,
                                                                  kv_bound);
  return (int)hipGetLastError();
}

int attn_extend(const bf16_t* qkv, const int* base_lens, const int* new_lens, bf16_t* kc, bf16_t* vc, int cap, int B, int T,
                int nH, int nKV, int head_dim, int kv_bound, bf16_t* o, float* part, size_t part_bytes, hipStream_t st) {
  int chunk, ns;
  float* pp;
  if (int r = attn_extend_plan(qkv, kc, vc, o, part, part_bytes, cap, B, T, nH, nKV, head_dim, kv_bound, &chunk, &ns, &pp)) return r;
  if (int r = kv_extend_scatter(qkv, kc, vc, base_lens, new_lens, B, T, nH, nKV, head_dim, cap, kv_bound, st)) return r;
  return attn_extend_launch<false>(qkv, base_lens, new_lens, kc, vc, nullptr, nullptr, cap, B, T, nH, nKV, head_dim, kv_bound, o, pp,
                                   chunk, ns, st);
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
