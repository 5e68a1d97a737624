// HBM-bound kernels of the Slam forward/backward step for gfx950 (the optimizer's are in optimizer.hip).
// One wave64 per token row for the row-wise ops, 16-byte (bf16x8) accesses everywhere.
// Reference semantics: site-packages transformers/models/qwen2/modeling_qwen2.py
//   RMSNorm :247-252, RoPE :91-135, SwiGLU :41-48, embedding :356;
// loss: /root/reference slamkit/model/unit_lm.py:13-29.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int MAXC_LIMIT = 4;  // chunks of 8 per lane -> hidden <= 2048 (kernels are instantiated for 1..4)

// ------------------------------------------------------------------------------------------
// RMSNorm forward: y = bf16( x * rsqrt(mean(x^2)+eps) * w ), fp32 math, rstd saved.
// LN (OPT's nn.LayerNorm): y = bf16( (x - mu) * rsqrt(var+eps) * w + b ) with mu and var from two passes over the
// registers (no E[x^2] - mu^2 cancellation); mu and rstd saved.
// Algorithmic traffic: 4 B/element (read bf16 + write bf16).
template <int MAXC, bool LN = false>
__global__ __launch_bounds__(256) void rmsnorm_fwd_kernel(const bf16_t* __restrict__ x,
                                                          const bf16_t* __restrict__ w,
                                                          bf16_t* __restrict__ y, float* __restrict__ rstd,
                                                          int M, int H, float eps, const bf16_t* __restrict__ b = nullptr,
                                                          float* __restrict__ mean = nullptr) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int nch = H >> 3;
  const uint4* xr = reinterpret_cast<const uint4*>(x + (size_t)row * H);
  uint4 v[MAXC];
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    int c = lane + 64 * i;
    if (c < nch) {
      v[i] = xr[c];
      float f[8];
      unpack_bf16x8(v[i], f);
#pragma unroll
      for (int j = 0; j < 8; ++j) ss += LN ? f[j] : f[j] * f[j];
    }
  }
  ss = wave_sum(ss);
  float mu = 0.f;
  if constexpr (LN) {  // second pass: centred sum of squares
    mu = ss / (float)H;
    ss = 0.f;
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      int c = lane + 64 * i;
      if (c < nch) {
        float f[8];
        unpack_bf16x8(v[i], f);
#pragma unroll
        for (int j = 0; j < 8; ++j) ss += (f[j] - mu) * (f[j] - mu);
      }
    }
    ss = wave_sum(ss);
    if (lane == 0 && mean) mean[row] = mu;
  }
  const float r = rsqrtf(ss / (float)H + eps);
  if (lane == 0 && rstd) rstd[row] = r;
  uint4* yr = reinterpret_cast<uint4*>(y + (size_t)row * H);
  const uint4* wr = reinterpret_cast<const uint4*>(w);
  const uint4* br = reinterpret_cast<const uint4*>(b);
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    int c = lane + 64 * i;
    if (c < nch) {
      float f[8], g[8];
      unpack_bf16x8(v[i], f);
      unpack_bf16x8(wr[c], g);
      if constexpr (LN) {
        float bb[8];
        unpack_bf16x8(br[c], bb);
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = (f[j] - mu) * r * g[j] + bb[j];
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = f[j] * r * g[j];
      }
      yr[c] = pack_bf16x8(f);
    }
  }
}

// RMSNorm backward. dx = rstd*(dy*w - xhat*mean(dy*w*xhat)) (+ dres); dw partial per block.
// LN: xhat = (x - mu)*rstd, dx = rstd*(g - mean(g) - xhat*mean(g*xhat)) with g = dy*w (+ dres); partials of
// dw = sum dy*xhat and db = sum dy per block.
// Each wave walks rows wave, wave+4*gridDim.. accumulating its dw slice in registers.
// Algorithmic traffic: 6 B/element (+2 with the fused residual-gradient add).
template <int MAXC, bool LN = false>
__global__ __launch_bounds__(256) void rmsnorm_bwd_kernel(const bf16_t* __restrict__ dy,
                                                          const bf16_t* __restrict__ x,
                                                          const bf16_t* __restrict__ w,
                                                          const float* __restrict__ rstd,
                                                          const bf16_t* __restrict__ dres,
                                                          bf16_t* __restrict__ dx, float* __restrict__ dw_part,
                                                          int M, int H, const float* __restrict__ mean = nullptr,
                                                          float* __restrict__ db_part = nullptr) {
  __shared__ float red[4][MAXC * 64 * 8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nch = H >> 3;
  float dwa[MAXC][8], dba[MAXC][8];
#pragma unroll
  for (int i = 0; i < MAXC; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) { dwa[i][j] = 0.f; dba[i][j] = 0.f; }
  const uint4* wr = reinterpret_cast<const uint4*>(w);
  float wv[MAXC][8];
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    int c = lane + 64 * i;
    if (c < nch) unpack_bf16x8(wr[c], wv[i]);
  }
  // software-pipelined over rows: the next row's loads are in flight while this row is reduced
  auto load_row = [&](int row, uint4* rx, uint4* rdy, uint4* rdr) {
    const uint4* xr = reinterpret_cast<const uint4*>(x + (size_t)row * H);
    const uint4* dyr = reinterpret_cast<const uint4*>(dy + (size_t)row * H);
    const uint4* drr = dres ? reinterpret_cast<const uint4*>(dres + (size_t)row * H) : nullptr;
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      int c = lane + 64 * i;
      if (c < nch) {
        rx[i] = xr[c];
        rdy[i] = dyr[c];
        if (drr) rdr[i] = drr[c];
      }
    }
  };
  const int rstep = gridDim.x * 4;
  int row = blockIdx.x * 4 + wave;
  uint4 cx[MAXC], cdy[MAXC], cdr[MAXC];
  float cr = 0.f, cmu = 0.f;
  if (row < M) { load_row(row, cx, cdy, cdr); cr = rstd[row]; if constexpr (LN) cmu = mean[row]; }
  for (; row < M; row += rstep) {
    uint4 nx[MAXC], ndy[MAXC], ndr[MAXC];
    float nr = 0.f, nmu = 0.f;
    const int nrow = row + rstep;
    if (nrow < M) { load_row(nrow, nx, ndy, ndr); nr = rstd[nrow]; if constexpr (LN) nmu = mean[nrow]; }
    const float r = cr;
    float xh[MAXC][8], gy[MAXC][8];
    float dot = 0.f, gsum = 0.f;
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      int c = lane + 64 * i;
      if (c < nch) {
        float fx[8], fd[8];
        unpack_bf16x8(cx[i], fx);
        unpack_bf16x8(cdy[i], fd);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          xh[i][j] = LN ? (fx[j] - cmu) * r : fx[j] * r;
          gy[i][j] = fd[j] * wv[i][j];
          dot += gy[i][j] * xh[i][j];
          dwa[i][j] += fd[j] * xh[i][j];
          if constexpr (LN) { gsum += gy[i][j]; dba[i][j] += fd[j]; }
        }
      }
    }
    dot = wave_sum(dot) / (float)H;
    if constexpr (LN) gsum = wave_sum(gsum) / (float)H;
    uint4* dxr = reinterpret_cast<uint4*>(dx + (size_t)row * H);
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      int c = lane + 64 * i;
      if (c < nch) {
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = LN ? r * (gy[i][j] - gsum - xh[i][j] * dot) : r * (gy[i][j] - xh[i][j] * dot);
        if (dres) {
          float a[8];
          unpack_bf16x8(cdr[i], a);
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] += a[j];
        }
        dxr[c] = pack_bf16x8(o);
      }
    }
#pragma unroll
    for (int i = 0; i < MAXC; ++i) { cx[i] = nx[i]; cdy[i] = ndy[i]; cdr[i] = ndr[i]; }
    cr = nr;
    cmu = nmu;
  }
  // cross-wave reduction of the dw partials, then one row of dw_part per block
#pragma unroll
  for (int i = 0; i < MAXC; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) red[wave][(lane + 64 * i) * 8 + j] = dwa[i][j];
  __syncthreads();
  for (int e = threadIdx.x; e < H; e += 256)
    dw_part[(size_t)blockIdx.x * H + e] = red[0][e] + red[1][e] + red[2][e] + red[3][e];
  if constexpr (LN) {  // the same for db through the same LDS
    __syncthreads();
#pragma unroll
    for (int i = 0; i < MAXC; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) red[wave][(lane + 64 * i) * 8 + j] = dba[i][j];
    __syncthreads();
    for (int e = threadIdx.x; e < H; e += 256)
      db_part[(size_t)blockIdx.x * H + e] = red[0][e] + red[1][e] + red[2][e] + red[3][e];
  }
}

// Wide rows (2048 < hidden <= 4096): a row is split over the two waves of a PAIR, chunk c = (2 i + half) * 64 + lane, so each
// wave keeps at most 4 chunks in registers - the per-wave register budget of the narrow <3> / <4> instantiations - and the
// row statistic is the sum of the two waves' partials, exchanged through LDS and always added as (half 0) + (half 1).
// A block is two pairs (two rows at a time).
constexpr int WIDE_LIMIT = 8;  // chunks of 8 per lane PAIR -> hidden <= 4096

template <int MAXC>
__global__ __launch_bounds__(256) void rmsnorm_fwd_wide_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                               bf16_t* __restrict__ y, float* __restrict__ rstd, int M, int H,
                                                               float eps) {
  __shared__ float part[2][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int pair = wave >> 1, half = wave & 1;
  const int row = blockIdx.x * 2 + pair;
  const bool live = row < M;
  const int nch = H >> 3;
  const uint4* xr = reinterpret_cast<const uint4*>(x + (size_t)(live ? row : 0) * H);
  uint4 v[MAXC];
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    int c = (2 * i + half) * 64 + lane;
    if (live && c < nch) {
      v[i] = xr[c];
      float f[8];
      unpack_bf16x8(v[i], f);
#pragma unroll
      for (int j = 0; j < 8; ++j) ss += f[j] * f[j];
    }
  }
  ss = wave_sum(ss);
  if (lane == 0) part[pair][half] = ss;
  __syncthreads();
  if (!live) return;
  const float r = rsqrtf((part[pair][0] + part[pair][1]) / (float)H + eps);
  if (lane == 0 && half == 0 && rstd) rstd[row] = r;
  uint4* yr = reinterpret_cast<uint4*>(y + (size_t)row * H);
  const uint4* wr = reinterpret_cast<const uint4*>(w);
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    int c = (2 * i + half) * 64 + lane;
    if (c < nch) {
      float f[8], g[8];
      unpack_bf16x8(v[i], f);
      unpack_bf16x8(wr[c], g);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = f[j] * r * g[j];
      yr[c] = pack_bf16x8(f);
    }
  }
}

// Backward for wide rows: pair p of block b walks rows 2 b + p, + 2 gridDim.x, ...; every block runs the same number of
// iterations (a pair past the end idles) because the halves of a row meet at a block barrier once per row. The dot partials
// alternate between two LDS slots, so one barrier per row is enough. Each wave accumulates dw for its own chunks; the two
// pairs are added through LDS at the end (pair 0 + pair 1): one row of dw_part per block, as in the narrow kernel.
template <int MAXC>
__global__ __launch_bounds__(256) void rmsnorm_bwd_wide_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                               const bf16_t* __restrict__ w, const float* __restrict__ rstd,
                                                               const bf16_t* __restrict__ dres, bf16_t* __restrict__ dx,
                                                               float* __restrict__ dw_part, int M, int H) {
  __shared__ float red[2][MAXC * 2 * 64 * 8];
  __shared__ float dpart[2][2][2];  // [parity][pair][half]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int pair = wave >> 1, half = wave & 1;
  const int nch = H >> 3;
  float dwa[MAXC][8], wv[MAXC][8];
  const uint4* wr = reinterpret_cast<const uint4*>(w);
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { dwa[i][j] = 0.f; wv[i][j] = 0.f; }
    int c = (2 * i + half) * 64 + lane;
    if (c < nch) unpack_bf16x8(wr[c], wv[i]);
  }
  auto load_row = [&](int row, uint4* rx, uint4* rdy, uint4* rdr) {
    const uint4* xr = reinterpret_cast<const uint4*>(x + (size_t)row * H);
    const uint4* dyr = reinterpret_cast<const uint4*>(dy + (size_t)row * H);
    const uint4* drr = dres ? reinterpret_cast<const uint4*>(dres + (size_t)row * H) : nullptr;
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      int c = (2 * i + half) * 64 + lane;
      if (c < nch) {
        rx[i] = xr[c];
        rdy[i] = dyr[c];
        if (drr) rdr[i] = drr[c];
      }
    }
  };
  const int rstep = gridDim.x * 2;
  const int first = blockIdx.x * 2;  // pair 0's first row: < M for every launched block
  const int iters = (M - first + rstep - 1) / rstep;
  int row = first + pair;
  uint4 cx[MAXC], cdy[MAXC], cdr[MAXC];
  float cr = 0.f;
  if (row < M) { load_row(row, cx, cdy, cdr); cr = rstd[row]; }
  for (int it = 0; it < iters; ++it, row += rstep) {
    uint4 nx[MAXC], ndy[MAXC], ndr[MAXC];
    float nr = 0.f;
    const int nrow = row + rstep;
    const bool live = row < M;
    if (nrow < M) { load_row(nrow, nx, ndy, ndr); nr = rstd[nrow]; }
    const float r = cr;
    float xh[MAXC][8], gy[MAXC][8];
    float dot = 0.f;
    if (live) {
#pragma unroll
      for (int i = 0; i < MAXC; ++i) {
        int c = (2 * i + half) * 64 + lane;
        if (c < nch) {
          float fx[8], fd[8];
          unpack_bf16x8(cx[i], fx);
          unpack_bf16x8(cdy[i], fd);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            xh[i][j] = fx[j] * r;
            gy[i][j] = fd[j] * wv[i][j];
            dot += gy[i][j] * xh[i][j];
            dwa[i][j] += fd[j] * xh[i][j];
          }
        }
      }
    }
    dot = wave_sum(dot);
    if (lane == 0) dpart[it & 1][pair][half] = dot;
    __syncthreads();
    if (live) {
      dot = (dpart[it & 1][pair][0] + dpart[it & 1][pair][1]) / (float)H;
      uint4* dxr = reinterpret_cast<uint4*>(dx + (size_t)row * H);
#pragma unroll
      for (int i = 0; i < MAXC; ++i) {
        int c = (2 * i + half) * 64 + lane;
        if (c < nch) {
          float o[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = r * (gy[i][j] - xh[i][j] * dot);
          if (dres) {
            float a[8];
            unpack_bf16x8(cdr[i], a);
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] += a[j];
          }
          dxr[c] = pack_bf16x8(o);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < MAXC; ++i) { cx[i] = nx[i]; cdy[i] = ndy[i]; cdr[i] = ndr[i]; }
    cr = nr;
  }
  // the two pairs' dw partials, then one row of dw_part per block
#pragma unroll
  for (int i = 0; i < MAXC; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) red[pair][((2 * i + half) * 64 + lane) * 8 + j] = dwa[i][j];
  __syncthreads();
  for (int e = threadIdx.x; e < H; e += 256) dw_part[(size_t)blockIdx.x * H + e] = red[0][e] + red[1][e];
}

// column sums of a bf16 matrix (bias gradient): part[blockIdx.y][N] fp32. Block = 16 column chunks (8 columns
// each) x 16 row lanes; a row lane walks rows lane, lane + 16 gridDim.y, ...; the 16 row lanes are combined in
// LDS in a fixed order. Algorithmic traffic: 2 B/element read.
__global__ __launch_bounds__(256) void colsum_bf16_kernel(const bf16_t* __restrict__ X, int ld, int M, int N,
                                                          float* __restrict__ part) {
  __shared__ float red[16][16 * 8 + 1];
  const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;  // chunk index
  const bool ok = c * 8 < N;
  float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (ok) {
    for (int m = blockIdx.y * 16 + rl; m < M; m += gridDim.y * 16) {
      float f[8];
      unpack_bf16x8(*reinterpret_cast<const uint4*>(X + (size_t)m * ld + c * 8), f);
#pragma unroll
      for (int j = 0; j < 8; ++j) s[j] += f[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[rl][cl * 8 + j] = s[j];
  __syncthreads();
  if (threadIdx.x < 128) {
    const int col = blockIdx.x * 128 + threadIdx.x;
    if (col < N) {
      float t = 0.f;
#pragma unroll
      for (int k = 0; k < 16; ++k) t += red[k][threadIdx.x];
      part[(size_t)blockIdx.y * N + col] = t;
    }
  }
}

// out[c] = (acc? out[c]:0) + sum_b part[b][c]; block = 16 columns x 16 row-slices, fixed order.
// blockIdx.y selects one of several equally shaped instances (per-layer partial slabs finished together).
// img_only / sumsq: GradSink semantics (kernels.h) - slot = blockIdx.y * gridDim.x + blockIdx.x
__global__ __launch_bounds__(256) void colsum_finish_kernel(const float* __restrict__ part, int nb, int N,
                                                            float* __restrict__ out, int accumulate,
                                                            size_t part_stride, size_t out_stride, bf16_t* __restrict__ img,
                                                            int img_only, float* __restrict__ sumsq) {
  __shared__ float red[16][17];
  part += (size_t)blockIdx.y * part_stride;
  out += (size_t)blockIdx.y * out_stride;
  if (img) img += (size_t)blockIdx.y * out_stride;
  const int cl = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  float s = 0.f;
  if (c < N)
    for (int b = sl; b < nb; b += 16) s += part[(size_t)b * N + c];
  red[sl][cl] = s;
  __syncthreads();
  float sq = 0.f;
  if (sl == 0 && c < N) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += red[k][cl];
    const float o = (accumulate ? out[c] : 0.f) + t;
    if (!img_only) { out[c] = o; sq = o * o; }
    if (img) {
      const bf16_t b = f32_to_bf16(o);
      img[c] = b;
      if (img_only) { const float r = bf16_to_f32(b); sq = r * r; }
    }
  }
  if (sumsq) {  // the 16 column results of the block, added in column order
    __syncthreads();
    if (sl == 0) red[0][cl] = sq;
    __syncthreads();
    if (threadIdx.x == 0) {
      float t = 0.f;
#pragma unroll
      for (int k = 0; k < 16; ++k) t += red[0][k];
      sumsq[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
    }
  }
}

// ------------------------------------------------------------------------------------------
// RoPE tables (fp32 cos/sin [M][hd/2]) from positions; position_ids == nullptr -> m % T.
__global__ void rope_table_kernel(const int64_t* __restrict__ pos, int M, int T, int half, float theta,
                                  float* __restrict__ cs, float* __restrict__ sn, float* __restrict__ csq,
                                  float* __restrict__ snq, float qscale) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * half) return;
  int m = i / half, d = i % half;
  float p = pos ? (float)pos[m] : (float)(m % T);
  float inv = 1.0f / powf(theta, (float)(2 * d) / (float)(2 * half));
  float a = p * inv;
  float s, c;
  sincosf(a, &s, &c);
  cs[i] = c;
  sn[i] = s;
  if (csq) {  // the query heads' table: the rotation and the softmax scale * log2(e) in one multiply (attention.hip)
    csq[i] = c * qscale;
    snq[i] = s * qscale;
  }
}

// In-place rotate-half RoPE on the first `nrot` heads of each row of qkv [M][ld] (head_dim hd, a
// multiple of 16). dir = +1 forward, -1 backward (transpose rotation).
__global__ __launch_bounds__(256) void rope_kernel(bf16_t* __restrict__ qkv, int ld, int M, int nrot, int hd,
                                                   const float* __restrict__ cs, const float* __restrict__ sn,
                                                   float dir, int q_heads, float q_scale) {
  // one thread: 8 low-half elems + their 8 high-half partners of one head; hd/16 threads per head
  size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int tph = hd >> 4, half = hd >> 1;
  int per_row = nrot * tph;
  if (idx >= (size_t)M * per_row) return;
  int m = (int)(idx / per_row), r = (int)(idx % per_row);
  int head = r / tph, part = r % tph;
  bf16_t* base = qkv + (size_t)m * ld + head * hd + part * 8;
  uint4 lo = *reinterpret_cast<uint4*>(base), hi = *reinterpret_cast<uint4*>(base + half);
  float a[8], b[8], c[8], s[8];
  unpack_bf16x8(lo, a);
  unpack_bf16x8(hi, b);
  const float4* cp = reinterpret_cast<const float4*>(cs + (size_t)m * half + part * 8);
  const float4* sp = reinterpret_cast<const float4*>(sn + (size_t)m * half + part * 8);
  *reinterpret_cast<float4*>(c) = cp[0]; *reinterpret_cast<float4*>(c + 4) = cp[1];
  *reinterpret_cast<float4*>(s) = sp[0]; *reinterpret_cast<float4*>(s + 4) = sp[1];
  float o1[8], o2[8];
  const float hs = head < q_heads ? q_scale : 1.f;  // query heads leave pre-scaled by scale * log2(e)
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float sj = s[j] * dir;
    o1[j] = (a[j] * c[j] - b[j] * sj) * hs;
    o2[j] = (b[j] * c[j] + a[j] * sj) * hs;
  }
  *reinterpret_cast<uint4*>(base) = pack_bf16x8(o1);
  *reinterpret_cast<uint4*>(base + half) = pack_bf16x8(o2);
}

// ------------------------------------------------------------------------------------------
// SwiGLU: gu [M][2I] -> act [M][I]. Column layout of gu: blocks of `blk` gate columns followed by the
// matching `blk` up columns (blk = I: the plain gate|up halves; blk = 32: the engine's interleaved
// layout that puts a gate/up pair into the same MFMA lane of the gate|up GEMM epilogue).
__global__ __launch_bounds__(256) void swiglu_fwd_kernel(const bf16_t* __restrict__ gu, bf16_t* __restrict__ act,
                                                         size_t M, int I, int blk) {
  size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  int nch = I >> 3;
  if (idx >= M * nch) return;
  size_t m = idx / nch;
  int c = idx % nch;
  const int a0 = c * 8;
  const bf16_t* row = gu + m * 2 * I + (a0 / blk) * 2 * blk + (a0 % blk);
  float g[8], u[8], o[8];
  unpack_bf16x8(*reinterpret_cast<const uint4*>(row), g);
  unpack_bf16x8(*reinterpret_cast<const uint4*>(row + blk), u);
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = g[j] * fast_sigmoid(g[j]) * u[j];
  *reinterpret_cast<uint4*>(act + m * I + c * 8) = pack_bf16x8(o);
}

// dgu (written in place over gu) from dact
__global__ __launch_bounds__(256) void swiglu_bwd_kernel(bf16_t* __restrict__ gu, const bf16_t* __restrict__ dact,
                                                         size_t M, int I, int blk) {
  size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  int nch = I >> 3;
  if (idx >= M * nch) return;
  size_t m = idx / nch;
  int c = idx % nch;
  const int a0 = c * 8;
  bf16_t* row = gu + m * 2 * I + (a0 / blk) * 2 * blk + (a0 % blk);
  float g[8], u[8], d[8], dg[8], du[8];
  unpack_bf16x8(*reinterpret_cast<const uint4*>(row), g);
  unpack_bf16x8(*reinterpret_cast<const uint4*>(row + blk), u);
  unpack_bf16x8(*reinterpret_cast<const uint4*>(dact + m * I + c * 8), d);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float sg = fast_sigmoid(g[j]);
    float silu = g[j] * sg;
    du[j] = d[j] * silu;
    dg[j] = d[j] * u[j] * sg * (1.f + g[j] * (1.f - sg));
  }
  *reinterpret_cast<uint4*>(row) = pack_bf16x8(dg);
  *reinterpret_cast<uint4*>(row + blk) = pack_bf16x8(du);
}

// ------------------------------------------------------------------------------------------
// NEFTune ("neftune_call_next", include/slam_engine.h): uniform noise on the embedding output, drawn inside the gather. The eight
// elements of a lane's chunk share one Philox call; element j of chunk i8 takes t = 2 r16 - 65535 (exact: an odd integer) and
// n = t * s, one uncontracted fp32 multiply, is added to the fp32 value the plain gather would store.
SLAM_DEVICE void neft_add8(float* a, const NeftKey& k, uint64_t i8) {
  // the multiply and the add round separately (__fmul_rn + __fadd_rn): the operators under this pragma, because the two
  // intrinsics are plain operators in the runtime's headers and the compiler fuses them into one fma all the same
#pragma clang fp contract(off)
  const Philox4 b = philox4x32_10((uint32_t)i8, (uint32_t)(i8 >> 32), k.call, NEFT_SITE, k.k0, k.k1);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float n = (float)(2 * (int)sr_r16(b, j) - 65535) * k.s;
    a[j] = a[j] + n;
  }
}

// Embedding gather: out[m,:] = E[ids[m],:]; NOISE: out[m,:] = bf16(E[ids[m],:] + n), one rounding. The unarmed kernel keeps
// its name and arguments: its instantiation is the code it was before the noisy one existed.
template <bool NOISE>
SLAM_DEVICE void embed_fwd_body(const int64_t* __restrict__ ids, const bf16_t* __restrict__ E, bf16_t* __restrict__ out, size_t M,
                                int H, int V, const NeftKey& k) {
  size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  int nch = H >> 3;
  if (idx >= M * nch) return;
  size_t m = idx / nch;
  int c = idx % nch;
  int64_t id = ids[m];
  if (id < 0 || id >= V) id = 0;
  if (NOISE) {
    float a[8];
    unpack_bf16x8(*reinterpret_cast<const uint4*>(E + (size_t)id * H + c * 8), a);
    neft_add8(a, k, (k.base >> 3) + idx);
    *reinterpret_cast<uint4*>(out + m * H + c * 8) = pack_bf16x8(a);
  } else {
    *reinterpret_cast<uint4*>(out + m * H + c * 8) = *reinterpret_cast<const uint4*>(E + (size_t)id * H + c * 8);
  }
}
__global__ __launch_bounds__(256) void embed_fwd_kernel(const int64_t* __restrict__ ids,
                                                        const bf16_t* __restrict__ E, bf16_t* __restrict__ out,
                                                        size_t M, int H, int V) {
  embed_fwd_body<false>(ids, E, out, M, H, V, NeftKey());
}
__global__ __launch_bounds__(256) void embed_noise_fwd_kernel(const int64_t* __restrict__ ids, const bf16_t* __restrict__ E,
                                                              bf16_t* __restrict__ out, size_t M, int H, int V, NeftKey k) {
  embed_fwd_body<true>(ids, E, out, M, H, V, k);
}

// OPT embedding: out[m,:] = bf16(E[ids[m],:] + P[pos[m] + 2,:]) (one rounding), pos = position_ids or m % T; the
// position row index is also written to prow[m] (the backward's scatter ids). Both indices are clamped to their tables.
// NOISE: out[m,:] = bf16((E + P) + n), the two fp32 adds in this order.
template <bool NOISE>
SLAM_DEVICE void embed_pos_fwd_body(const int64_t* __restrict__ ids, const int64_t* __restrict__ pos, const bf16_t* __restrict__ E,
                                    const bf16_t* __restrict__ P, bf16_t* __restrict__ out, int64_t* __restrict__ prow, size_t M,
                                    int H, int V, int T, int NP, const NeftKey& k) {
  size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  int nch = H >> 3;
  if (idx >= M * nch) return;
  size_t m = idx / nch;
  int c = idx % nch;
  int64_t id = ids[m];
  if (id < 0 || id >= V) id = 0;
  int64_t p = (pos ? pos[m] : (int64_t)(m % (size_t)T)) + 2;
  p = p < 0 ? 0 : (p >= NP ? NP - 1 : p);
  if (c == 0 && prow) prow[m] = p;
  float a[8], b[8];
  unpack_bf16x8(*reinterpret_cast<const uint4*>(E + (size_t)id * H + c * 8), a);
  unpack_bf16x8(*reinterpret_cast<const uint4*>(P + (size_t)p * H + c * 8), b);
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] += b[j];
  if (NOISE) neft_add8(a, k, (k.base >> 3) + idx);
  *reinterpret_cast<uint4*>(out + m * H + c * 8) = pack_bf16x8(a);
}
__global__ __launch_bounds__(256) void embed_pos_fwd_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ pos,
                                                            const bf16_t* __restrict__ E, const bf16_t* __restrict__ P,
                                                            bf16_t* __restrict__ out, int64_t* __restrict__ prow, size_t M,
                                                            int H, int V, int T, int NP) {
  embed_pos_fwd_body<false>(ids, pos, E, P, out, prow, M, H, V, T, NP, NeftKey());
}
__global__ __launch_bounds__(256) void embed_pos_noise_fwd_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ pos,
                                                                  const bf16_t* __restrict__ E, const bf16_t* __restrict__ P,
                                                                  bf16_t* __restrict__ out, int64_t* __restrict__ prow, size_t M,
                                                                  int H, int V, int T, int NP, NeftKey k) {
  embed_pos_fwd_body<true>(ids, pos, E, P, out, prow, M, H, V, T, NP, k);
}

// ReLU backward through the stored post-ReLU activation: d[i] = act[i] > 0 ? d[i] : 0
__global__ __launch_bounds__(256) void relu_bwd_kernel(bf16_t* __restrict__ d, const bf16_t* __restrict__ act, size_t n8) {
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const uint4 a = reinterpret_cast<const uint4*>(act)[i];
  uint4 v = reinterpret_cast<uint4*>(d)[i];
  const uint32_t aw[4] = {a.x, a.y, a.z, a.w};
  uint32_t* vw = reinterpret_cast<uint32_t*>(&v);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t lo = aw[k] & 0xffffu, hi = aw[k] >> 16;
    // a bf16 is > 0 when its sign bit is clear and it is not +0
    const uint32_t keep = ((lo & 0x8000u) == 0 && lo != 0 ? 0xffffu : 0u) | ((hi & 0x8000u) == 0 && hi != 0 ? 0xffff0000u : 0u);
    vw[k] &= keep;
  }
  reinterpret_cast<uint4*>(d)[i] = v;
}

// Residual dropout (OPT, "dropout_thr16"): 8 bf16 per lane and iteration - two 16-byte loads, one Philox call, one 16-byte
// store - grid-stride, no LDS. Forward, in place on y: y = bf16(resid + (keep ? y * scale : 0)), one rounding; a dropped
// element takes resid's own bits.
__global__ __launch_bounds__(256) void dropout_add_kernel(bf16_t* __restrict__ y, const bf16_t* __restrict__ resid, size_t n8,
                                                          DropKey k) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
    const uint4 yv = reinterpret_cast<const uint4*>(y)[i];
    const uint4 rv = reinterpret_cast<const uint4*>(resid)[i];
    const uint32_t keep = drop_keep8(k, (k.base >> 3) + i);
    float yf[8], rf[8];
    unpack_bf16x8(yv, yf);
    unpack_bf16x8(rv, rf);
#pragma unroll
    for (int j = 0; j < 8; ++j) rf[j] = (keep >> j) & 1u ? rf[j] + yf[j] * k.scale : rf[j];
    reinterpret_cast<uint4*>(y)[i] = pack_bf16x8(rf);
  }
}
// Backward: dm = keep ? bf16(dy * scale) : 0 into a second buffer; dy stays what it was (the residual branch's gradient)
__global__ __launch_bounds__(256) void dropout_bwd_kernel(const bf16_t* __restrict__ dy, bf16_t* __restrict__ dm, size_t n8,
                                                          DropKey k) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
    const uint4 dv = reinterpret_cast<const uint4*>(dy)[i];
    const uint32_t keep = drop_keep8(k, (k.base >> 3) + i);
    float f[8];
    unpack_bf16x8(dv, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = (keep >> j) & 1u ? f[j] * k.scale : 0.f;
    reinterpret_cast<uint4*>(dm)[i] = pack_bf16x8(f);
  }
}

// One-hot rows for the gather-side embedding gradient (dE += onehot^T dh0 runs on the wgrad GEMM,
// deterministic); the padding_idx column is suppressed like nn.Embedding(padding_idx).
__global__ __launch_bounds__(256) void onehot_kernel(const int64_t* __restrict__ ids, bf16_t* __restrict__ oh,
                                                     size_t M, int Vp, int V, int pad_id) {
  size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  int nch = Vp >> 3;
  if (idx >= M * nch) return;
  size_t m = idx / nch;
  int c = idx % nch;
  int64_t id = ids[m];
  uint32_t w[4] = {0, 0, 0, 0};
  if (id >= 0 && id < V && id != pad_id && (id >> 3) == c) {
    int j = (int)(id & 7);
    w[j >> 1] = (j & 1) ? 0x3f800000u : 0x00003f80u;
  }
  *reinterpret_cast<uint4*>(oh + m * Vp + c * 8) = make_uint4(w[0], w[1], w[2], w[3]);
}

// ------------------------------------------------------------------------------------------
// Shifted cross-entropy over bf16 logits [M][Vp] (Vp = 512 padded, V valid columns).
// target(m) = labels[m+1] when m is not the last position of its batch row, else ignore.
__global__ void count_valid_kernel(const int64_t* __restrict__ labels, int B, int T, double num_items,
                                   float* __restrict__ denom) {
  __shared__ int red[256];
  int cnt = 0;
  if (num_items <= 0.0) {
    for (int i = threadIdx.x; i < B * T; i += 256) {
      int t = i % T;
      if (t < T - 1 && labels[i + 1] != -100) ++cnt;
    }
  }
  red[threadIdx.x] = cnt;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) denom[0] = num_items > 0.0 ? (float)num_items : (float)red[0];
}

// Label smoothing (HF LabelSmoother; include/slam_engine.h, slam_set_label_smoothing) is the SMOOTH = true instantiation of the
// two row kernels and of loss_finish_kernel; SMOOTH = false compiles to the code these kernels were without it. Per valid row,
//   row_loss = lse - z_y (the PLAIN nll, whatever eps),  row_smooth = lse - (1 / V) sum_{v on} z_v,
//   d loss / d z_j = (p_j - (1 - eps) [j == y] - eps / V) / denom  on the "on" columns, exactly 0 on the others.
// sum_v z_v is taken in the pass that forms max and sum, in fp32: per thread in column order, lanes by the xor butterfly, waves
// in wave order - the same bits every run. No extra read or write of the row.

// one wave per row, Vp == 512 (64 lanes x 8)
// (logits and dlogits may be the SAME buffer: a lane reads its chunk into registers before it writes it)
template <bool SMOOTH>
__global__ __launch_bounds__(256) void ce_kernel(const bf16_t* logits,
                                                 const int64_t* __restrict__ labels,
                                                 const float* __restrict__ denom, bf16_t* dlogits,
                                                 float* __restrict__ row_loss, int B, int T, int Vp, int V,
                                                 const uint8_t* __restrict__ colmask, float eps,
                                                 float* __restrict__ row_smooth) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int M = B * T;
  if (m >= M) return;
  const int t = m % T;
  int64_t tgt = (t < T - 1) ? labels[m + 1] : -100;
  const bool valid = (tgt >= 0 && tgt < V);
  uint4* dl = dlogits ? reinterpret_cast<uint4*>(dlogits + (size_t)m * Vp) + lane : nullptr;
  if (!valid) {  // wave-uniform
    if (dl) *dl = make_uint4(0, 0, 0, 0);
    if (lane == 0) row_loss[m] = 0.f;
    if constexpr (SMOOTH) { if (lane == 0) row_smooth[m] = 0.f; }
    return;
  }
  float f[8];
  unpack_bf16x8(reinterpret_cast<const uint4*>(logits + (size_t)m * Vp)[lane], f);
  // columns >= V (padding) and columns flagged in colmask (modality-restricted scoring: the reference sets
  // those logits to -inf, unit_lm.py:187-188) are outside the softmax
  bool on[8];
  {
    uint2 mk = colmask ? *reinterpret_cast<const uint2*>(colmask + lane * 8) : make_uint2(0, 0);
#pragma unroll
    for (int j = 0; j < 8; ++j) on[j] = (lane * 8 + j < V) && !(((j < 4 ? mk.x : mk.y) >> (8 * (j & 3))) & 0xff);
  }
  float mx = -3.0e38f, zs = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if constexpr (SMOOTH) zs += on[j] ? f[j] : 0.f;
    if (!on[j]) f[j] = -3.0e38f;
    mx = fmaxf(mx, f[j]);
  }
  mx = wave_max(mx);
  float e[8], s = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    e[j] = on[j] ? __expf(f[j] - mx) : 0.f;
    s += e[j];
  }
  s = wave_sum(s);
  const float lse = mx + logf(s);
  // logit of the target
  float tl = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (lane * 8 + j == (int)tgt) tl = f[j];
  tl = wave_sum(tl);
  if (lane == 0) row_loss[m] = (colmask && colmask[tgt]) ? INFINITY : lse - tl;
  float uni = 0.f;  // eps / V, the uniform part of the smoothed target
  if constexpr (SMOOTH) {
    zs = wave_sum(zs);
    uni = eps / (float)V;
    if (lane == 0) row_smooth[m] = lse - zs / (float)V;
  }
  if (dl) {
    const float sc = 1.f / denom[0];
    const float inv = 1.f / s;
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float pj = e[j] * inv;
      if constexpr (SMOOTH) {
        if (on[j]) pj -= uni;  // never on a pad column: those stay exact zeros
        if (lane * 8 + j == (int)tgt) pj -= 1.f - eps;
      } else {
        if (lane * 8 + j == (int)tgt) pj -= 1.f;
      }
      o[j] = pj * sc;
    }
    *dl = pack_bf16x8(o);
  }
}

// Large vocabulary (Vp > 512, a multiple of 8): one 256-thread block per row, two passes over the
// row (online max / sum, then the gradient); the second read hits L2 (a 152k-column row is 300 KB).
// Algorithmic traffic: 2 B/logit read + 2 B/logit written.
// (logits and dlogits may be the SAME buffer - the engine's training path: the gradient replaces the logits chunk by
//  chunk in the second pass, after the barrier behind the first pass and after thread 0 has read the target logit)
template <bool SMOOTH>
__global__ __launch_bounds__(256) void ce_big_kernel(const bf16_t* logits,
                                                     const int64_t* __restrict__ labels,
                                                     const float* __restrict__ denom, bf16_t* dlogits,
                                                     float* __restrict__ row_loss, int B, int T, int Vp, int V,
                                                     const uint8_t* __restrict__ colmask, float eps,
                                                     float* __restrict__ row_smooth) {
  __shared__ float red_m[4], red_s[4];
  __shared__ float red_z[SMOOTH ? 4 : 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = blockIdx.x;
  const int t = m % T;
  const int64_t tgt = (t < T - 1) ? labels[m + 1] : -100;
  const bool valid = (tgt >= 0 && tgt < V);
  const int nch = Vp >> 3;
  const uint4* lr = reinterpret_cast<const uint4*>(logits + (size_t)m * Vp);
  uint4* dl = dlogits ? reinterpret_cast<uint4*>(dlogits + (size_t)m * Vp) : nullptr;
  if (!valid) {  // block-uniform
    if (dl)
      for (int c = tid; c < nch; c += 256) dl[c] = make_uint4(0, 0, 0, 0);
    if (tid == 0) row_loss[m] = 0.f;
    if constexpr (SMOOTH) { if (tid == 0) row_smooth[m] = 0.f; }
    return;
  }
  const float tgt_logit = tid == 0 ? bf16_to_f32(logits[(size_t)m * Vp + tgt]) : 0.f;  // read before any in-place write
  float mx = -3.0e38f, sm = 0.f, zs = 0.f;
  for (int c = tid; c < nch; c += 256) {
    float f[8];
    unpack_bf16x8(lr[c], f);
    const uint2 mk = colmask ? *reinterpret_cast<const uint2*>(colmask + c * 8) : make_uint2(0, 0);
    bool on[8];
    float cm = -3.0e38f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      on[j] = (c * 8 + j < V) && !(((j < 4 ? mk.x : mk.y) >> (8 * (j & 3))) & 0xff);
      if constexpr (SMOOTH) zs += on[j] ? f[j] : 0.f;
      if (!on[j]) f[j] = -3.0e38f;
      cm = fmaxf(cm, f[j]);
    }
    const float nm = fmaxf(mx, cm);
    float cs = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) cs += on[j] ? __expf(f[j] - nm) : 0.f;
    sm = sm * __expf(mx - nm) + cs;
    mx = nm;
  }
  const float wm = wave_max(mx);
  sm = wave_sum(sm * __expf(mx - wm));
  if (lane == 0) { red_m[wave] = wm; red_s[wave] = sm; }
  if constexpr (SMOOTH) {
    zs = wave_sum(zs);
    if (lane == 0) red_z[wave] = zs;
  }
  __syncthreads();
  const float bm = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
  float bs = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) bs += red_s[w] * __expf(red_m[w] - bm);
  const float lse = bm + logf(bs);
  if (tid == 0) row_loss[m] = (colmask && colmask[tgt]) ? INFINITY : lse - tgt_logit;
  float uni = 0.f;  // eps / V, the uniform part of the smoothed target
  if constexpr (SMOOTH) {
    uni = eps / (float)V;
    if (tid == 0) row_smooth[m] = lse - (((red_z[0] + red_z[1]) + red_z[2]) + red_z[3]) / (float)V;
  }
  if (dl) {
    const float sc = 1.f / denom[0];
    // p = exp(z - max) / sum, as in ce_kernel - not exp(z - lse): lse = max + log(sum) is rounded at the magnitude of the
    // logits, and half an ulp of |lse| in the exponent is a relative error of 1e-3 in every p of a row of logits near 3e4
    const float inv = 1.f / bs;
    for (int c = tid; c < nch; c += 256) {
      float f[8], o[8];
      unpack_bf16x8(lr[c], f);
      const uint2 mk = colmask ? *reinterpret_cast<const uint2*>(colmask + c * 8) : make_uint2(0, 0);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int col = c * 8 + j;
        const bool onj = (col < V) && !(((j < 4 ? mk.x : mk.y) >> (8 * (j & 3))) & 0xff);
        float pj = onj ? __expf(f[j] - bm) * inv : 0.f;
        if constexpr (SMOOTH) {
          if (onj) pj -= uni;  // never on a pad column: those stay exact zeros
          if (col == (int)tgt) pj -= 1.f - eps;
        } else {
          if (col == (int)tgt) pj -= 1.f;
        }
        o[j] = pj * sc;
      }
      dl[c] = pack_bf16x8(o);
    }
  }
}

// ---- gather-side embedding gradient for large vocabularies -------------------------------------
// dE[v] += sum over tokens m with ids[m] == v of dh[m], summed in token order (deterministic, no float
// atomics): rank[m] = number of earlier tokens with the same id (brute force through LDS, M^2/2
// integer compares), count[v] by integer atomics, exclusive scan -> list of token indices per id.
__global__ __launch_bounds__(256) void embed_rank_kernel(const int64_t* __restrict__ ids, int M, int V, int pad_id,
                                                         int* __restrict__ rank, int* __restrict__ count) {
  __shared__ int sid[256];
  const int m = blockIdx.x * 256 + threadIdx.x;
  int64_t id64 = m < M ? ids[m] : -1;
  const int id = (id64 >= 0 && id64 < V && id64 != pad_id) ? (int)id64 : -1;
  int r = 0;
  for (int base = 0; base <= blockIdx.x * 256; base += 256) {
    const int j = base + threadIdx.x;
    int64_t v = j < M ? ids[j] : -1;
    __syncthreads();
    sid[threadIdx.x] = (v >= 0 && v < V) ? (int)v : -2;
    __syncthreads();
    const int lim = min(256, m - base);  // only tokens before m
    for (int k = 0; k < lim; ++k) r += (sid[k] == id);
  }
  if (m < M) {
    rank[m] = r;
    if (id >= 0) atomicAdd(count + id, 1);
  }
}
// offset = exclusive scan of count (single block of 1024 threads, each a contiguous slice)
__global__ __launch_bounds__(1024) void embed_scan_kernel(const int* __restrict__ count, int* __restrict__ offset, int V) {
  __shared__ int part[1024];
  const int per = (V + 1023) / 1024;
  const int lo = threadIdx.x * per, hi = min(V, lo + per);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += count[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    int v = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  int run = part[threadIdx.x] - s;
  for (int i = lo; i < hi; ++i) { offset[i] = run; run += count[i]; }
}
__global__ __launch_bounds__(256) void embed_fill_kernel(const int64_t* __restrict__ ids, int M, int V, int pad_id,
                                                         const int* __restrict__ rank, const int* __restrict__ offset,
                                                         int* __restrict__ list) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const int64_t id = ids[m];
  if (id >= 0 && id < V && id != pad_id) list[offset[id] + rank[m]] = m;
}
// one block per vocabulary row with at least one token; thread = 8 columns
__global__ __launch_bounds__(256) void embed_scatter_kernel(const bf16_t* __restrict__ dh, float* __restrict__ dE, int H,
                                                            const int* __restrict__ count, const int* __restrict__ offset,
                                                            const int* __restrict__ list) {
  const int v = blockIdx.x;
  const int n = count[v];
  if (n == 0) return;
  const int* l = list + offset[v];
  for (int c = threadIdx.x; c < (H >> 3); c += 256) {
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < n; ++j) {
      float f[8];
      unpack_bf16x8(*reinterpret_cast<const uint4*>(dh + (size_t)l[j] * H + c * 8), f);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] += f[k];
    }
    float4* o = reinterpret_cast<float4*>(dE + (size_t)v * H + c * 8);
    float4 a = o[0], b = o[1];
    o[0] = make_float4(a.x + acc[0], a.y + acc[1], a.z + acc[2], a.w + acc[3]);
    o[1] = make_float4(b.x + acc[4], b.y + acc[5], b.z + acc[6], b.w + acc[7]);
  }
}

// loss = sum(row_loss) / denom  (single block, fixed order -> deterministic)
// SMOOTH: loss = ((1 - eps) sum(row_loss) + eps sum(row_smooth)) / denom, each sum in that same order, in double
template <bool SMOOTH>
__global__ void loss_finish_kernel(const float* __restrict__ row_loss, int M, const float* __restrict__ denom,
                                   float* __restrict__ loss, float eps, const float* __restrict__ row_smooth) {
  __shared__ double red[256];
  __shared__ double red2[SMOOTH ? 256 : 1];
  double s = 0.0, s2 = 0.0;
  for (int i = threadIdx.x; i < M; i += 256) {
    s += (double)row_loss[i];
    if constexpr (SMOOTH) s2 += (double)row_smooth[i];
  }
  red[threadIdx.x] = s;
  if constexpr (SMOOTH) red2[threadIdx.x] = s2;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (threadIdx.x < k) {
      red[threadIdx.x] += red[threadIdx.x + k];
      if constexpr (SMOOTH) red2[threadIdx.x] += red2[threadIdx.x + k];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double tot = red[0];
    if constexpr (SMOOTH) tot = (1.0 - (double)eps) * red[0] + (double)eps * red2[0];
    loss[0] = denom[0] > 0.f ? (float)(tot / (double)denom[0]) : 0.f;
  }
}

// Per-sequence sum of -row_loss over valid targets (log-likelihood, unit_lm.py:184-194 shape)
__global__ void seq_loglik_kernel(const float* __restrict__ row_loss, const int64_t* __restrict__ labels, int B,
                                  int T, float* __restrict__ ll, float* __restrict__ cnt) {
  int b = blockIdx.x;
  __shared__ float rs[256], rc[256];
  float s = 0.f, c = 0.f;
  for (int t = threadIdx.x; t < T - 1; t += 256) {
    if (labels[(size_t)b * T + t + 1] != -100) { s -= row_loss[(size_t)b * T + t]; c += 1.f; }
  }
  rs[threadIdx.x] = s; rc[threadIdx.x] = c;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (threadIdx.x < k) { rs[threadIdx.x] += rs[threadIdx.x + k]; rc[threadIdx.x] += rc[threadIdx.x + k]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { ll[b] = rs[0]; cnt[b] = rc[0]; }
}

// strided 2-D bf16 copy in 16-byte chunks (padded logits -> user logits needs element copy; see below)
__global__ __launch_bounds__(256) void copy_cols_kernel(const bf16_t* __restrict__ src, int lds_, bf16_t* __restrict__ dst,
                                                        int ldd, size_t M, int ncols) {
  size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= M * (size_t)ncols) return;
  size_t m = idx / ncols;
  int c = idx % ncols;
  dst[m * ldd + c] = src[m * lds_ + c];
}

// dlogits[m][:] *= coef[m / T]  (per-sequence loss weights: DPO's +-beta*sigmoid(-x)/n)
__global__ __launch_bounds__(256) void scale_rows_bf16_kernel(bf16_t* __restrict__ x, const float* __restrict__ coef,
                                                              size_t M, int T, int chunks_per_row) {
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * chunks_per_row) return;
  const float s = coef[(i / chunks_per_row) / T];
  float f[8];
  uint4* p = reinterpret_cast<uint4*>(x) + i;
  unpack_bf16x8(*p, f);
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] *= s;
  *p = pack_bf16x8(f);
}

// ---- padding-free execution of padded batches (slam_forward_unpadded, slam_forward_unpadded_spans) -------------------
// The pack rule in one launch, one thread per packed position m' in [0, Mp): token (b, starts[b] + t), t < lens[b], goes to
// m' = off[b] + t with off the exclusive prefix sum of lens (starts == nullptr: every row starts at column 0, right padding);
// [off[B], Mp) is one dummy segment of pad tokens. Every block scans lens itself,
// 256 rows at a time through LDS with the running total carried along, and a thread takes its row from the chunk whose
// offsets bracket m' - no second launch, no atomics; block 0 also leaves off[] behind for the kernels below. starts are
// clamped to [0, T], lens to [0, T - starts] and segment ends to Mp (a memory guard: callers check their ranges). The 8-byte
// elements are gathered from row starts of any alignment, so accesses are element-wide.
// (Every block repeats the scan: B / 256 rounds of 8 barrier pairs per block, nothing at the callers' B of tens to hundreds.
// Should B reach the thousands, scan once in a launch of its own and let the blocks read off[].)
__global__ __launch_bounds__(256) void unpad_pack_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ labels,
                                                         const int32_t* __restrict__ starts, const int32_t* __restrict__ lens,
                                                         int B, int T, int Mp, int64_t pad_id,
                                                         int64_t* __restrict__ ids_p, int64_t* __restrict__ lab_p,
                                                         int64_t* __restrict__ pos_p, int32_t* __restrict__ seg_s,
                                                         int32_t* __restrict__ seg_e, int32_t* __restrict__ row_p,
                                                         int32_t* __restrict__ off) {
  __shared__ int sc[257];  // sc[i] = lens[c] + ... + lens[c + i - 1] of the current chunk
  const int tid = threadIdx.x;
  const int m = blockIdx.x * 256 + tid;
  int base = 0, row = -1, s0 = 0, s1 = 0;
  if (blockIdx.x == 0 && tid == 0) off[0] = 0;
  for (int c = 0; c < B; c += 256) {
    const int b = c + tid;
    sc[tid + 1] = b < B ? min(max(lens[b], 0), T - (starts ? min(max(starts[b], 0), T) : 0)) : 0;
    if (tid == 0) sc[0] = 0;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const int v = tid >= d ? sc[tid + 1 - d] : 0;
      __syncthreads();
      sc[tid + 1] += v;
      __syncthreads();
    }
    if (blockIdx.x == 0 && b < B) off[b + 1] = base + sc[tid + 1];
    const int total = sc[256];
    if (row < 0 && m >= base && m < base + total) {
      const int r = m - base;
      int lo = 0, hi = 255;  // the last i with sc[i] <= r: its row holds r (empty rows share their offset with the next)
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sc[mid] <= r) lo = mid; else hi = mid - 1;
      }
      row = c + lo;
      s0 = base + sc[lo];
      s1 = base + sc[lo + 1];
    }
    base += total;
    __syncthreads();
  }
  if (m >= Mp) return;
  if (row >= 0) {
    const int t = m - s0;
    const size_t src = (size_t)row * T + (starts ? min(max(starts[row], 0), T) : 0) + t;
    ids_p[m] = ids[src];
    if (lab_p) lab_p[m] = t == 0 ? -100 : labels[src];
    pos_p[m] = t;
    seg_s[m] = s0;
    seg_e[m] = min(s1, Mp);
    row_p[m] = row;
  } else {
    ids_p[m] = pad_id;
    if (lab_p) lab_p[m] = -100;
    pos_p[m] = m - base;
    seg_s[m] = base;
    seg_e[m] = Mp;
    row_p[m] = -1;
  }
}

// Logits back in the batch's own layout: dst[b][starts[b] + t][0 .. V) = packed row off[b] + t for t < lens[b], zeros at the pad
// positions on either side (starts == nullptr: 0; clamped to [0, T] as the pack clamps it).
// One thread per 16-byte chunk when V is a multiple of 8 (every dst row then starts 16-byte aligned), else per element.
template <int W>
__global__ __launch_bounds__(256) void unpad_logits_kernel(const bf16_t* __restrict__ src, int Vp, bf16_t* __restrict__ dst, int V,
                                                           const int32_t* __restrict__ off, const int32_t* __restrict__ starts,
                                                           size_t BT, int T, int Mp) {
  const int per = V / W;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= BT * per) return;
  const size_t bt = idx / per;
  const int c = (int)(idx % per) * W;
  const int b = (int)(bt / T);
  const int t = (int)(bt % T) - (starts ? min(max(starts[b], 0), T) : 0);  // the column within the row's span
  const int o = off[b];
  const bool real = t >= 0 && t < off[b + 1] - o && o + t < Mp;  // (rows past Mp exist only when lens broke their contract)
  if constexpr (W == 8) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (real) v = *reinterpret_cast<const uint4*>(src + (size_t)(o + t) * Vp + c);
    *reinterpret_cast<uint4*>(dst + bt * V + c) = v;
  } else {
    dst[bt * V + c] = real ? src[(size_t)(o + t) * Vp + c] : (bf16_t)0;
  }
}

// seq_loglik_kernel over packed segments: row b's targets are labels'[off[b] + t + 1] for t + 1 < lens[b]
__global__ void seq_loglik_unpadded_kernel(const float* __restrict__ row_loss, const int64_t* __restrict__ labels,
                                           const int32_t* __restrict__ off, int Mp, float* __restrict__ ll,
                                           float* __restrict__ cnt) {
  const int b = blockIdx.x;
  __shared__ float rs[256], rc[256];
  const int o = off[b], n = min(off[b + 1], Mp) - o;  // (clamped to the packed rows: a memory guard)
  float s = 0.f, c = 0.f;
  for (int t = threadIdx.x; t < n - 1; t += 256) {
    if (labels[(size_t)o + t + 1] != -100) { s -= row_loss[(size_t)o + t]; c += 1.f; }
  }
  rs[threadIdx.x] = s; rc[threadIdx.x] = c;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (threadIdx.x < k) { rs[threadIdx.x] += rs[threadIdx.x + k]; rc[threadIdx.x] += rc[threadIdx.x + k]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { ll[b] = rs[0]; cnt[b] = rc[0]; }
}

// dlogits[m'][:] *= coef[row of m'], the tail by 0 (scale_rows_bf16_kernel's m / T is a dense-row index)
__global__ __launch_bounds__(256) void scale_rows_unpadded_bf16_kernel(bf16_t* __restrict__ x, const float* __restrict__ coef,
                                                                       const int32_t* __restrict__ row, size_t M,
                                                                       int chunks_per_row) {
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * chunks_per_row) return;
  const int r = row[i / chunks_per_row];
  const float s = r >= 0 ? coef[r] : 0.f;
  float f[8];
  uint4* p = reinterpret_cast<uint4*>(x) + i;
  unpack_bf16x8(*p, f);
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] *= s;
  *p = pack_bf16x8(f);
}

__global__ __launch_bounds__(256) void scale_bf16_kernel(bf16_t* __restrict__ x, size_t nchunks, float s) {
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nchunks) return;
  float f[8];
  uint4* p = reinterpret_cast<uint4*>(x) + i;
  unpack_bf16x8(*p, f);
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] *= s;
  *p = pack_bf16x8(f);
}

// ------------------------------------------------------------------------------------------
// Qwen3: per-head RMSNorm of the q and k heads (one learned weight [HD] for all q heads, one for all k heads), before RoPE.
// All three kernels number the q|k heads of the batch flat, head g = m * (nH + nKV) + h, and give each head to HD / 8
// consecutive lanes, 8 dims (16 bytes of bf16) per lane: a wave covers 64 / (HD / 8) consecutive heads, every lane group is
// whole, and the head statistics are an xor butterfly over the group's lanes. The rotate-half partner of dims d0 .. d0 + 7
// lives in lane (sub ^ HD / 16) of the same group.
//
// Forward: y = x rstd w in fp32, rotated with the engine's tables (csq / snq for the query heads: the pre-scale), ONE rounding
// at the in-place store. raw / rstd_out (nullable): the input bits [M][(nH + nKV) HD] and rstd [M][nH + nKV] for backward.
// Algorithmic traffic: 2 B/element read, 2 (+ 2 with the saved copy) written; the tables are [M][HD / 2] fp32, read once per head.
template <int HD>
__global__ __launch_bounds__(256) void qknorm_rope_fwd_kernel(bf16_t* __restrict__ qkv, int ld, uint32_t total, int nH, int nQK,
                                                              const bf16_t* __restrict__ wq, const bf16_t* __restrict__ wk,
                                                              const float* __restrict__ cs, const float* __restrict__ sn,
                                                              const float* __restrict__ csq, const float* __restrict__ snq,
                                                              float eps, bf16_t* __restrict__ raw, float* __restrict__ rstd_out) {
  constexpr int LG = HD / 8, half = HD / 2;
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;  // the launcher keeps total * LG below 2^31: 32-bit index arithmetic
  const uint32_t g = t / LG;
  const int d0 = (int)(t % LG) * 8;
  const bool ok = g < total;  // the same for every lane of a group; nobody leaves before the shuffles
  const uint32_t m = ok ? g / (uint32_t)nQK : 0;
  const int h = ok ? (int)(g - m * (uint32_t)nQK) : 0;
  const bool isq = h < nH;
  bf16_t* p = qkv + (size_t)m * ld + (size_t)h * HD + d0;
  uint4 v = make_uint4(0, 0, 0, 0);
  if (ok) v = *reinterpret_cast<const uint4*>(p);
  float x[8], w[8], c[8], s[8];
  unpack_bf16x8(v, x);
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) ss += x[j] * x[j];
#pragma unroll
  for (int o = LG / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  const float r = rsqrtf(ss / (float)HD + eps);
  unpack_bf16x8(*reinterpret_cast<const uint4*>((isq ? wq : wk) + d0), w);
  const bool lo = d0 < half;
  const size_t tb = (size_t)m * half + (lo ? d0 : d0 - half);
  const float4* cp = reinterpret_cast<const float4*>((isq ? csq : cs) + tb);
  const float4* sp = reinterpret_cast<const float4*>((isq ? snq : sn) + tb);
  *reinterpret_cast<float4*>(c) = cp[0]; *reinterpret_cast<float4*>(c + 4) = cp[1];
  *reinterpret_cast<float4*>(s) = sp[0]; *reinterpret_cast<float4*>(s + 4) = sp[1];
  float y[8], o8[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) y[j] = x[j] * r * w[j];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float pr = __shfl_xor(y[j], LG / 2, 64);  // the rotate-half partner dim
    o8[j] = lo ? y[j] * c[j] - pr * s[j] : y[j] * c[j] + pr * s[j];
  }
  if (!ok) return;
  *reinterpret_cast<uint4*>(p) = pack_bf16x8(o8);
  if (raw) *reinterpret_cast<uint4*>(raw + (size_t)g * HD + d0) = v;
  if (rstd_out && d0 == 0) rstd_out[g] = r;
}

// Backward, in place on the q|k columns of d(qkv) (dy = the gradient of the normed, un-rotated head, as attn_bwd leaves it):
// g = dy w, dx = rstd (g - xhat mean_d(g xhat)), xhat = raw rstd. dw_q / dw_k partials: every lane sums dy xhat of its 8 dims
// over the heads it meets (wave `wave` of block b takes the 64 / LG-head chunks 4 b + wave, + 4 gridDim, ..), the lane groups
// of a wave are combined by an xor butterfly, the four waves through LDS in wave order: part_q / part_k [gridDim][HD],
// finished by colsum_finish_many in block order - the same bits every run. Traffic: 4 B/element read, 2 written.
template <int HD>
__global__ __launch_bounds__(256) void qknorm_bwd_kernel(bf16_t* __restrict__ dqkv, int ld, const bf16_t* __restrict__ raw,
                                                         const float* __restrict__ rstd, const bf16_t* __restrict__ wq,
                                                         const bf16_t* __restrict__ wk, uint32_t total, int nH, int nQK,
                                                         float* __restrict__ part_q, float* __restrict__ part_k) {
  constexpr int LG = HD / 8, HPW = 64 / LG;
  __shared__ float red[4][2][HD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int d0 = (lane % LG) * 8, slot = lane / LG;
  float wqv[8], wkv[8], aq[8], ak[8];
  unpack_bf16x8(*reinterpret_cast<const uint4*>(wq + d0), wqv);
  unpack_bf16x8(*reinterpret_cast<const uint4*>(wk + d0), wkv);
#pragma unroll
  for (int j = 0; j < 8; ++j) { aq[j] = 0.f; ak[j] = 0.f; }
  struct Item { uint4 x, dy; float r; bf16_t* dp; bool isq, ok; };
  auto load = [&](uint32_t chunk) {
    Item it;
    const uint32_t g = chunk * HPW + slot;
    it.ok = g < total;
    it.x = it.dy = make_uint4(0, 0, 0, 0);
    it.r = 0.f;
    it.dp = nullptr;
    it.isq = true;
    if (it.ok) {
      const uint32_t m = g / (uint32_t)nQK;
      const int h = (int)(g - m * (uint32_t)nQK);
      it.isq = h < nH;
      it.dp = dqkv + (size_t)m * ld + (size_t)h * HD + d0;
      it.x = *reinterpret_cast<const uint4*>(raw + (size_t)g * HD + d0);
      it.dy = *reinterpret_cast<const uint4*>(it.dp);
      it.r = rstd[g];
    }
    return it;
  };
  const uint32_t nchunks = (total + HPW - 1) / HPW, step = gridDim.x * 4u;
  uint32_t c = blockIdx.x * 4u + wave;
  Item cur{};
  if (c < nchunks) cur = load(c);
  for (; c < nchunks; c += step) {  // the next chunk's loads are in flight while this one is reduced
    Item nxt{};
    if (c + step < nchunks) nxt = load(c + step);
    float fx[8], fd[8], xh[8], gy[8];
    unpack_bf16x8(cur.x, fx);
    unpack_bf16x8(cur.dy, fd);
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      xh[j] = fx[j] * cur.r;
      gy[j] = fd[j] * (cur.isq ? wqv[j] : wkv[j]);
      dot += gy[j] * xh[j];
      const float dwj = fd[j] * xh[j];
      aq[j] += cur.isq ? dwj : 0.f;
      ak[j] += cur.isq ? 0.f : dwj;
    }
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
    dot /= (float)HD;
    float o8[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o8[j] = cur.r * (gy[j] - xh[j] * dot);
    if (cur.ok) *reinterpret_cast<uint4*>(cur.dp) = pack_bf16x8(o8);
    cur = nxt;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
#pragma unroll
    for (int o = LG; o < 64; o <<= 1) {
      aq[j] += __shfl_xor(aq[j], o, 64);
      ak[j] += __shfl_xor(ak[j], o, 64);
    }
  }
  if (slot == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { red[wave][0][d0 + j] = aq[j]; red[wave][1][d0 + j] = ak[j]; }
  }
  __syncthreads();
  if (threadIdx.x < 2 * HD) {
    const int k = threadIdx.x / HD, e = threadIdx.x % HD;
    (k ? part_k : part_q)[(size_t)blockIdx.x * HD + e] = red[0][k][e] + red[1][k][e] + red[2][k][e] + red[3][k][e];
  }
}

// Decode: the q and k heads of the fp32 projection rows [B][ld], normalised in place (fp32 in, fp32 out, weight applied);
// attn_decode then rotates and rounds once.
template <int HD>
__global__ __launch_bounds__(256) void qknorm_rows_f32_kernel(float* __restrict__ qkv, int ld, uint32_t total, int nH, int nQK,
                                                              const bf16_t* __restrict__ wq, const bf16_t* __restrict__ wk,
                                                              float eps) {
  constexpr int LG = HD / 8;
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  const uint32_t g = t / LG;
  const int d0 = (int)(t % LG) * 8;
  const bool ok = g < total;
  const uint32_t m = ok ? g / (uint32_t)nQK : 0;
  const int h = ok ? (int)(g - m * (uint32_t)nQK) : 0;
  float* p = qkv + (size_t)m * ld + (size_t)h * HD + d0;
  float x[8] = {0, 0, 0, 0, 0, 0, 0, 0}, w[8];
  if (ok) {
    *reinterpret_cast<float4*>(x) = reinterpret_cast<const float4*>(p)[0];
    *reinterpret_cast<float4*>(x + 4) = reinterpret_cast<const float4*>(p)[1];
  }
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) ss += x[j] * x[j];
#pragma unroll
  for (int o = LG / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  if (!ok) return;
  const float r = rsqrtf(ss / (float)HD + eps);
  unpack_bf16x8(*reinterpret_cast<const uint4*>((h < nH ? wq : wk) + d0), w);
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = x[j] * r * w[j];
  reinterpret_cast<float4*>(p)[0] = *reinterpret_cast<float4*>(x);
  reinterpret_cast<float4*>(p)[1] = *reinterpret_cast<float4*>(x + 4);
}

}  // namespace

namespace slam {

int rmsnorm_fwd(const bf16_t* x, const bf16_t* w, bf16_t* y, float* rstd, int M, int H, float eps, hipStream_t st) {
  if ((H & 7) || H > WIDE_LIMIT * 512) return -1;
  if (H > MAXC_LIMIT * 512) {  // wide rows: two waves per row
    if (H <= 3072) rmsnorm_fwd_wide_kernel<3><<<(M + 1) / 2, 256, 0, st>>>(x, w, y, rstd, M, H, eps);
    else rmsnorm_fwd_wide_kernel<4><<<(M + 1) / 2, 256, 0, st>>>(x, w, y, rstd, M, H, eps);
    LAUNCH_RET();
  }
  switch ((H / 8 + 63) / 64) {
    case 1: rmsnorm_fwd_kernel<1><<<(M + 3) / 4, 256, 0, st>>>(x, w, y, rstd, M, H, eps); break;
    case 2: rmsnorm_fwd_kernel<2><<<(M + 3) / 4, 256, 0, st>>>(x, w, y, rstd, M, H, eps); break;
    case 3: rmsnorm_fwd_kernel<3><<<(M + 3) / 4, 256, 0, st>>>(x, w, y, rstd, M, H, eps); break;
    default: rmsnorm_fwd_kernel<4><<<(M + 3) / 4, 256, 0, st>>>(x, w, y, rstd, M, H, eps); break;
  }
  LAUNCH_RET();
}

int layernorm_fwd(const bf16_t* x, const bf16_t* w, const bf16_t* b, bf16_t* y, float* mean, float* rstd, int M, int H, float eps,
                  hipStream_t st) {
  if ((H & 7) || H > MAXC_LIMIT * 512) return -1;
  switch ((H / 8 + 63) / 64) {
    case 1: rmsnorm_fwd_kernel<1, true><<<(M + 3) / 4, 256, 0, st>>>(x, w, y, rstd, M, H, eps, b, mean); break;
    case 2: rmsnorm_fwd_kernel<2, true><<<(M + 3) / 4, 256, 0, st>>>(x, w, y, rstd, M, H, eps, b, mean); break;
    case 3: rmsnorm_fwd_kernel<3, true><<<(M + 3) / 4, 256, 0, st>>>(x, w, y, rstd, M, H, eps, b, mean); break;
    default: rmsnorm_fwd_kernel<4, true><<<(M + 3) / 4, 256, 0, st>>>(x, w, y, rstd, M, H, eps, b, mean); break;
  }
  LAUNCH_RET();
}

int rmsnorm_bwd_blocks(int M) { int b = (M + 15) / 16; return b > 512 ? 512 : (b < 1 ? 1 : b); }  // 2 blocks/CU

// sink (nullable, with dw): how the final values of dw are kept (GradSink, kernels.h)
int rmsnorm_bwd(const bf16_t* dy, const bf16_t* x, const bf16_t* w, const float* rstd, const bf16_t* dres,
                bf16_t* dx, float* dw, int accumulate, float* part, int M, int H, hipStream_t st, bf16_t* dw_img, GradSink* sink) {
  if ((H & 7) || H > WIDE_LIMIT * 512) return -1;
  int nb = rmsnorm_bwd_blocks(M);
  if (H > MAXC_LIMIT * 512) {  // wide rows: two waves per row, the same grid and the same [nb][H] partial slab
    if (H <= 3072) rmsnorm_bwd_wide_kernel<3><<<nb, 256, 0, st>>>(dy, x, w, rstd, dres, dx, part, M, H);
    else rmsnorm_bwd_wide_kernel<4><<<nb, 256, 0, st>>>(dy, x, w, rstd, dres, dx, part, M, H);
  } else
  switch ((H / 8 + 63) / 64) {
    case 1: rmsnorm_bwd_kernel<1><<<nb, 256, 0, st>>>(dy, x, w, rstd, dres, dx, part, M, H); break;
    case 2: rmsnorm_bwd_kernel<2><<<nb, 256, 0, st>>>(dy, x, w, rstd, dres, dx, part, M, H); break;
    case 3: rmsnorm_bwd_kernel<3><<<nb, 256, 0, st>>>(dy, x, w, rstd, dres, dx, part, M, H); break;
    default: rmsnorm_bwd_kernel<4><<<nb, 256, 0, st>>>(dy, x, w, rstd, dres, dx, part, M, H); break;
  }
  if (dw) return colsum_finish_many(part, 0, nb, H, dw, 0, 1, accumulate, st, dw_img, sink);  // dw == null: caller finishes later
  LAUNCH_RET();
}
// LayerNorm backward: partial slabs dw_part / db_part [rmsnorm_bwd_blocks(M)][H], finished by the caller (colsum_finish_many)
int layernorm_bwd(const bf16_t* dy, const bf16_t* x, const bf16_t* w, const float* mean, const float* rstd, const bf16_t* dres,
                  bf16_t* dx, float* dw_part, float* db_part, int M, int H, hipStream_t st) {
  if ((H & 7) || H > MAXC_LIMIT * 512) return -1;
  int nb = rmsnorm_bwd_blocks(M);
  switch ((H / 8 + 63) / 64) {
    case 1: rmsnorm_bwd_kernel<1, true><<<nb, 256, 0, st>>>(dy, x, w, rstd, dres, dx, dw_part, M, H, mean, db_part); break;
    case 2: rmsnorm_bwd_kernel<2, true><<<nb, 256, 0, st>>>(dy, x, w, rstd, dres, dx, dw_part, M, H, mean, db_part); break;
    case 3: rmsnorm_bwd_kernel<3, true><<<nb, 256, 0, st>>>(dy, x, w, rstd, dres, dx, dw_part, M, H, mean, db_part); break;
    default: rmsnorm_bwd_kernel<4, true><<<nb, 256, 0, st>>>(dy, x, w, rstd, dres, dx, dw_part, M, H, mean, db_part); break;
  }
  LAUNCH_RET();
}
// finish `count` equally shaped partial slabs in one launch: out[i] (+)= column sums of part[i]
int colsum_finish_many(const float* part, size_t part_stride, int nb, int N, float* out, size_t out_stride, int count,
                       int accumulate, hipStream_t st, bf16_t* img, GradSink* sink) {
  if (count <= 0) return 0;
  const dim3 grid((N + 15) / 16, count);
  if (sink) {
    sink->used = (int)(grid.x * grid.y);
    if (sink->img_only && !img) return -1;
    if (sink->sumsq && sink->used > sink->cap) return -3;
  }
  colsum_finish_kernel<<<grid, 256, 0, st>>>(part, nb, N, out, accumulate, part_stride, out_stride, img, sink ? sink->img_only : 0,
                                             sink ? sink->sumsq : nullptr);
  LAUNCH_RET();
}

int colsum_blocks(int M) { int b = (M + 63) / 64; return b > 128 ? 128 : (b < 1 ? 1 : b); }

int colsum_bf16(const bf16_t* X, int ld, int M, int N, float* out, int accumulate, float* part, hipStream_t st) {
  if (N & 7) return -1;
  int nb = colsum_blocks(M);
  dim3 grid((N / 8 + 15) / 16, nb);
  colsum_bf16_kernel<<<grid, 256, 0, st>>>(X, ld, M, N, part);
  if (out) colsum_finish_kernel<<<(N + 15) / 16, 256, 0, st>>>(part, nb, N, out, accumulate, 0, 0, nullptr, 0, nullptr);
  LAUNCH_RET();
}

int rope_table(const int64_t* pos, int M, int T, int head_dim, float theta, float* cs, float* sn, float* csq, float* snq,
               float qscale, hipStream_t st) {
  int half = head_dim / 2;
  rope_table_kernel<<<nblocks((size_t)M * half, 256), 256, 0, st>>>(pos, M, T, half, theta, cs, sn, csq, snq, qscale);
  LAUNCH_RET();
}

int rope_apply(bf16_t* qkv, int ld, int M, int nrot_heads, int head_dim, const float* cs, const float* sn, int backward,
               hipStream_t st, int q_heads, float q_scale) {
  if (head_dim & 15) return -1;
  rope_kernel<<<nblocks((size_t)M * nrot_heads * (head_dim / 16), 256), 256, 0, st>>>(qkv, ld, M, nrot_heads, head_dim, cs, sn,
                                                                                     backward ? -1.f : 1.f, q_heads, q_scale);
  LAUNCH_RET();
}

// Qwen3's per-head q / k RMSNorm. -1: a shape or pointer the kernels do not take (nothing is launched)
static bool qknorm_shape_ok(int M, int nH, int nKV, int head_dim, int ld) {
  if (!(M > 0 && nH > 0 && nKV > 0 && (head_dim == 64 || head_dim == 128) && ld >= (nH + nKV) * head_dim && (ld & 7) == 0)) return false;
  // the kernels index heads and threads in 32 bits: M (nH + nKV) head_dim / 8 threads (+ a block of slack) must stay below 2^31
  return (uint64_t)M * (uint64_t)(nH + nKV) * (uint64_t)(head_dim / 8) < (1ull << 31) - 1024;
}

int qknorm_rope_fwd(bf16_t* qkv, int ld, int M, int nH, int nKV, int head_dim, const bf16_t* wq, const bf16_t* wk, const float* cs,
                    const float* sn, const float* csq, const float* snq, float eps, bf16_t* raw_save, float* rstd_save,
                    hipStream_t st) {
  if (!qkv || !wq || !wk || !cs || !sn || !csq || !snq || !qknorm_shape_ok(M, nH, nKV, head_dim, ld)) return -1;
  const int nQK = nH + nKV;
  const uint32_t total = (uint32_t)M * (uint32_t)nQK;
  const unsigned grid = nblocks((size_t)total * (head_dim / 8), 256);
  if (head_dim == 64) qknorm_rope_fwd_kernel<64><<<grid, 256, 0, st>>>(qkv, ld, total, nH, nQK, wq, wk, cs, sn, csq, snq, eps, raw_save, rstd_save);
  else qknorm_rope_fwd_kernel<128><<<grid, 256, 0, st>>>(qkv, ld, total, nH, nQK, wq, wk, cs, sn, csq, snq, eps, raw_save, rstd_save);
  LAUNCH_RET();
}

// one wave per 64 / (head_dim / 8) heads at a time, four waves a block, at most 1024 blocks (4 per CU)
int qknorm_bwd_blocks(int M, int nH, int nKV, int head_dim) {
  if (M <= 0 || nH <= 0 || nKV <= 0 || (head_dim != 64 && head_dim != 128)) return 1;
  const size_t hpw = 64 / (head_dim / 8), chunks = ((size_t)M * (nH + nKV) + hpw - 1) / hpw;
  const size_t b = (chunks + 3) / 4;
  return b > 1024 ? 1024 : (int)b;
}

// nb: blocks = rows of the partial slabs (1 .. qknorm_bwd_blocks(..); fewer blocks walk more heads each)
int qknorm_bwd(bf16_t* dqkv, int ld, int M, int nH, int nKV, int head_dim, const bf16_t* raw, const float* rstd, const bf16_t* wq,
               const bf16_t* wk, int nb, float* part_q, float* part_k, hipStream_t st) {
  if (!dqkv || !raw || !rstd || !wq || !wk || !part_q || !part_k || !qknorm_shape_ok(M, nH, nKV, head_dim, ld)) return -1;
  if (nb < 1 || nb > qknorm_bwd_blocks(M, nH, nKV, head_dim)) return -1;
  const int nQK = nH + nKV;
  const uint32_t total = (uint32_t)M * (uint32_t)nQK;
  if (head_dim == 64) qknorm_bwd_kernel<64><<<nb, 256, 0, st>>>(dqkv, ld, raw, rstd, wq, wk, total, nH, nQK, part_q, part_k);
  else qknorm_bwd_kernel<128><<<nb, 256, 0, st>>>(dqkv, ld, raw, rstd, wq, wk, total, nH, nQK, part_q, part_k);
  LAUNCH_RET();
}

int qknorm_rows_f32(float* qkv, int ld, int B, int nH, int nKV, int head_dim, const bf16_t* wq, const bf16_t* wk, float eps,
                    hipStream_t st) {
  if (!qkv || !wq || !wk || !qknorm_shape_ok(B, nH, nKV, head_dim, ld)) return -1;
  const int nQK = nH + nKV;
  const uint32_t total = (uint32_t)B * (uint32_t)nQK;
  const unsigned grid = nblocks((size_t)total * (head_dim / 8), 256);
  if (head_dim == 64) qknorm_rows_f32_kernel<64><<<grid, 256, 0, st>>>(qkv, ld, total, nH, nQK, wq, wk, eps);
  else qknorm_rows_f32_kernel<128><<<grid, 256, 0, st>>>(qkv, ld, total, nH, nQK, wq, wk, eps);
  LAUNCH_RET();
}

int swiglu_fwd(const bf16_t* gu, bf16_t* act, int M, int I, int blk, hipStream_t st) {
  if ((I & 7) || (blk & 7) || I % blk) return -1;
  swiglu_fwd_kernel<<<nblocks((size_t)M * (I / 8), 256), 256, 0, st>>>(gu, act, (size_t)M, I, blk);
  LAUNCH_RET();
}
int swiglu_bwd(bf16_t* gu, const bf16_t* dact, int M, int I, int blk, hipStream_t st) {
  if ((I & 7) || (blk & 7) || I % blk) return -1;
  swiglu_bwd_kernel<<<nblocks((size_t)M * (I / 8), 256), 256, 0, st>>>(gu, dact, (size_t)M, I, blk);
  LAUNCH_RET();
}

int embed_fwd(const int64_t* ids, const bf16_t* E, bf16_t* out, int M, int H, int V, hipStream_t st) {
  embed_fwd_kernel<<<nblocks((size_t)M * (H / 8), 256), 256, 0, st>>>(ids, E, out, (size_t)M, H, V);
  LAUNCH_RET();
}
int embed_pos_fwd(const int64_t* ids, const int64_t* pos, const bf16_t* E, const bf16_t* P, bf16_t* out, int64_t* prow, int M, int H,
                  int V, int T, int NP, hipStream_t st) {
  if ((H & 7) || T <= 0 || NP <= 0) return -1;
  embed_pos_fwd_kernel<<<nblocks((size_t)M * (H / 8), 256), 256, 0, st>>>(ids, pos, E, P, out, prow, (size_t)M, H, V, T, NP);
  LAUNCH_RET();
}
int embed_noise_fwd(const int64_t* ids, const int64_t* pos, const bf16_t* E, const bf16_t* P, bf16_t* out, int64_t* prow, int M, int H,
                    int V, int T, int NP, const NeftSite& n, hipStream_t st) {
  if (M <= 0 || H <= 0 || (H & 7) || !(n.s >= 0.f) || !__builtin_isfinite(n.s) || n.index0 < 0 || (n.index0 & 7)) return -1;
  if (P && (T <= 0 || NP <= 0)) return -1;
  NeftKey k;
  k.k0 = (uint32_t)n.seed; k.k1 = (uint32_t)(n.seed >> 32);
  k.call = n.call; k.s = n.s; k.base = (uint64_t)n.index0;
  const unsigned grid = nblocks((size_t)M * (H / 8), 256);
  if (P) embed_pos_noise_fwd_kernel<<<grid, 256, 0, st>>>(ids, pos, E, P, out, prow, (size_t)M, H, V, T, NP, k);
  else embed_noise_fwd_kernel<<<grid, 256, 0, st>>>(ids, E, out, (size_t)M, H, V, k);
  LAUNCH_RET();
}
int relu_bwd(bf16_t* d, const bf16_t* act, size_t n, hipStream_t st) {
  if (n & 7) return -1;
  relu_bwd_kernel<<<nblocks(n / 8, 256), 256, 0, st>>>(d, act, n / 8);
  LAUNCH_RET();
}
// thr16 = round(p * 65536): q = thr16 / 65536 is the drop probability, the kept values are scaled by 1 / (1 - q) (fp32)
static DropKey drop_key(const DropSite& d) {
  DropKey k;
  k.k0 = (uint32_t)d.seed; k.k1 = (uint32_t)(d.seed >> 32);
  k.call = d.call; k.site = d.site; k.thr = (uint32_t)d.thr16;
  k.scale = 1.0f / (1.0f - (float)d.thr16 / 65536.0f);
  k.base = (uint64_t)d.index0;
  return k;
}
// memory-bound: about 8 blocks per CU's worth of grid at most, the rest by the stride - with the grid chosen so that every
// block runs the same number of iterations (3072 blocks of work are 1536 x 2, not 2048 of which half run twice)
static unsigned dropout_grid(size_t n8) {
  const size_t b = nblocks(n8, 256);
  const size_t iters = (b + 2047) / 2048;
  return (unsigned)((b + iters - 1) / iters);
}
int dropout_add(bf16_t* y, const bf16_t* resid, int M, int H, const DropSite& d, hipStream_t st) {
  if (M <= 0 || H <= 0 || (H & 7) || (d.index0 & 7) || d.index0 < 0 || d.thr16 < 0 || d.thr16 > 65535) return -1;
  const size_t n8 = (size_t)M * H / 8;
  dropout_add_kernel<<<dropout_grid(n8), 256, 0, st>>>(y, resid, n8, drop_key(d));
  LAUNCH_RET();
}
int dropout_bwd(const bf16_t* dy, bf16_t* dm, int M, int H, const DropSite& d, hipStream_t st) {
  if (M <= 0 || H <= 0 || (H & 7) || (d.index0 & 7) || d.index0 < 0 || d.thr16 < 0 || d.thr16 > 65535) return -1;
  const size_t n8 = (size_t)M * H / 8;
  dropout_bwd_kernel<<<dropout_grid(n8), 256, 0, st>>>(dy, dm, n8, drop_key(d));
  LAUNCH_RET();
}
int onehot(const int64_t* ids, bf16_t* oh, int M, int Vp, int V, int pad_id, hipStream_t st) {
  onehot_kernel<<<nblocks((size_t)M * (Vp / 8), 256), 256, 0, st>>>(ids, oh, (size_t)M, Vp, V, pad_id);
  LAUNCH_RET();
}

size_t embed_bwd_workspace_ints(int M, int Vp) { return (size_t)2 * M + 2 * (size_t)Vp + 64; }
int embed_bwd(const int64_t* ids, const bf16_t* dh, float* dE, int M, int H, int Vp, int V, int pad_id, int* ws,
              hipStream_t st) {
  if (H & 7) return -1;
  int* rank = ws;
  int* list = ws + M;
  int* count = ws + 2 * (size_t)M;
  int* offset = count + Vp;
  hipError_t e = hipMemsetAsync(count, 0, (size_t)Vp * sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  embed_rank_kernel<<<(M + 255) / 256, 256, 0, st>>>(ids, M, V, pad_id, rank, count);
  embed_scan_kernel<<<1, 1024, 0, st>>>(count, offset, V);
  embed_fill_kernel<<<(M + 255) / 256, 256, 0, st>>>(ids, M, V, pad_id, rank, offset, list);
  embed_scatter_kernel<<<V, 256, 0, st>>>(dh, dE, H, count, offset, list);
  LAUNCH_RET();
}

int cross_entropy(const bf16_t* logits, const int64_t* labels, double num_items, bf16_t* dlogits, float* row_loss,
                  float* denom, float* loss, int B, int T, int Vp, int V, const uint8_t* colmask, float eps, float* row_smooth,
                  hipStream_t st) {
  if (Vp < 512 || (Vp & 7) || V > Vp) return -1;
  if (!(eps >= 0.f && eps < 1.f)) return -1;
  if (eps > 0.f && (!row_smooth || colmask || V <= 0)) return -1;  // smoothing over a masked vocabulary is not defined here
  int M = B * T;
  count_valid_kernel<<<1, 256, 0, st>>>(labels, B, T, num_items, denom);
  if (eps > 0.f) {
    if (Vp == 512) ce_kernel<true><<<(M + 3) / 4, 256, 0, st>>>(logits, labels, denom, dlogits, row_loss, B, T, Vp, V, colmask, eps, row_smooth);
    else ce_big_kernel<true><<<M, 256, 0, st>>>(logits, labels, denom, dlogits, row_loss, B, T, Vp, V, colmask, eps, row_smooth);
    loss_finish_kernel<true><<<1, 256, 0, st>>>(row_loss, M, denom, loss, eps, row_smooth);
  } else {
    if (Vp == 512) ce_kernel<false><<<(M + 3) / 4, 256, 0, st>>>(logits, labels, denom, dlogits, row_loss, B, T, Vp, V, colmask, 0.f, nullptr);
    else ce_big_kernel<false><<<M, 256, 0, st>>>(logits, labels, denom, dlogits, row_loss, B, T, Vp, V, colmask, 0.f, nullptr);
    loss_finish_kernel<false><<<1, 256, 0, st>>>(row_loss, M, denom, loss, 0.f, nullptr);
  }
  LAUNCH_RET();
}
int seq_loglik(const float* row_loss, const int64_t* labels, int B, int T, float* ll, float* cnt, hipStream_t st) {
  seq_loglik_kernel<<<B, 256, 0, st>>>(row_loss, labels, B, T, ll, cnt);
  LAUNCH_RET();
}
int copy_cols(const bf16_t* src, int lds_, bf16_t* dst, int ldd, int M, int ncols, hipStream_t st) {
  copy_cols_kernel<<<nblocks((size_t)M * ncols, 256), 256, 0, st>>>(src, lds_, dst, ldd, (size_t)M, ncols);
  LAUNCH_RET();
}
int scale_rows_bf16(bf16_t* x, const float* coef, int M, int T, int ncols, hipStream_t st) {
  if (ncols & 7) return -1;
  scale_rows_bf16_kernel<<<nblocks((size_t)M * (ncols / 8), 256), 256, 0, st>>>(x, coef, (size_t)M, T, ncols / 8);
  LAUNCH_RET();
}
static size_t unpad_mmax(int B, int T) { return (((size_t)B * T + 63) / 64) * 64; }
size_t unpad_scratch_bytes(int B, int T) {
  if (B <= 0 || T <= 0) return 0;
  const size_t mm = unpad_mmax(B, T);  // a multiple of 64: every array below starts 256-byte aligned
  return mm * (3 * sizeof(int64_t) + 3 * sizeof(int32_t)) + (((size_t)(B + 1) * sizeof(int32_t) + 255) & ~(size_t)255);
}
UnpadView unpad_view(void* scratch, int B, int T) {
  const size_t mm = unpad_mmax(B, T);
  UnpadView v;
  v.ids = (int64_t*)scratch;
  v.labels = v.ids + mm;
  v.pos = v.labels + mm;
  v.seg_s = (int32_t*)(v.pos + mm);
  v.seg_e = v.seg_s + mm;
  v.row = v.seg_e + mm;
  v.off = v.row + mm;
  return v;
}
int unpad_pack(const int64_t* ids, const int64_t* labels, const int32_t* starts, const int32_t* lens, int B, int T, int Mp,
               int pad_id, const UnpadView& v, hipStream_t st) {
  if (B <= 0 || T <= 0 || Mp <= 0 || (size_t)Mp > unpad_mmax(B, T)) return -1;
  unpad_pack_kernel<<<nblocks((size_t)Mp, 256), 256, 0, st>>>(ids, labels, starts, lens, B, T, Mp, (int64_t)(pad_id > 0 ? pad_id : 0),
                                                              v.ids, labels ? v.labels : nullptr, v.pos, v.seg_s, v.seg_e, v.row,
                                                              v.off);
  LAUNCH_RET();
}
int unpad_logits(const bf16_t* src, int Vp, bf16_t* dst, int V, const int32_t* off, const int32_t* starts, int B, int T, int Mp,
                 hipStream_t st) {
  if (V <= 0 || V > Vp || (Vp & 7)) return -1;
  const size_t BT = (size_t)B * T;
  if (V % 8 == 0) unpad_logits_kernel<8><<<nblocks(BT * (V / 8), 256), 256, 0, st>>>(src, Vp, dst, V, off, starts, BT, T, Mp);
  else unpad_logits_kernel<1><<<nblocks(BT * V, 256), 256, 0, st>>>(src, Vp, dst, V, off, starts, BT, T, Mp);
  LAUNCH_RET();
}
int seq_loglik_unpadded(const float* row_loss, const int64_t* labels_packed, const int32_t* off, int B, int Mp, float* ll,
                        float* cnt, hipStream_t st) {
  seq_loglik_unpadded_kernel<<<B, 256, 0, st>>>(row_loss, labels_packed, off, Mp, ll, cnt);
  LAUNCH_RET();
}
int scale_rows_unpadded_bf16(bf16_t* x, const float* coef, const int32_t* row, int Mp, int ncols, hipStream_t st) {
  if (ncols & 7) return -1;
  scale_rows_unpadded_bf16_kernel<<<nblocks((size_t)Mp * (ncols / 8), 256), 256, 0, st>>>(x, coef, row, (size_t)Mp, ncols / 8);
  LAUNCH_RET();
}
int scale_bf16(bf16_t* x, size_t n, float s, hipStream_t st) {
  if (n & 7) return -1;
  scale_bf16_kernel<<<nblocks(n / 8, 256), 256, 0, st>>>(x, n / 8, s);
  LAUNCH_RET();
}

}  // namespace slam
