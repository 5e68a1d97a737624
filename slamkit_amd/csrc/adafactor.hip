// Adafactor for gfx950: HF transformers.optimization.Adafactor as Trainer builds it (scale_parameter = False, relative_step =
// False, beta1 = None) over the HF parameters laid across the engine's flat buffer (kernels.h AfSeg). Six launches a step for
// the whole model, whatever the number of segments; a block finds its (segment, row block, column block) by a binary search of
// the segment table on wave-uniform loads. Every sum runs in an order fixed by the segment's shape - no atomics - so a step gives
// the same bits on every run, from the fp32 gradient buffer and from a bf16 image that holds the same values.
//
// Tile = 256 rows x 256 columns, 256 threads. Thread t owns the 8 consecutive columns 8 (t % 32) .. of the rows rs + 8 i,
// rs = t / 32, i = 0 .. 31: a half wave reads one contiguous 256-column piece of a row with 16-byte (bf16: one, fp32: two)
// accesses per lane.
//
// The summation orders (s = (g clip)^2 + eps1, fp32 throughout unless stated):
//   row r, column block cb : a thread adds its 8 values left to right; the 32 lanes of the row by the xor butterfly 16, 8, 4, 2, 1
//   row r                  : the column blocks in cb order (af_finish_kernel), divided by cols
//   column c, row block rb : a thread adds its rows i = 0 .. 31 in order; the 8 threads rs = 0 .. 7 of the column in rs order
//   column c               : the row blocks in rb order (af_finish_kernel), divided by rows
//   mean of the row factors: thread k of 256 adds rows k, k + 256, ..; the 256 partials by the halving tree 128, 64, .. 1
//   sum of u^2, tile       : a thread adds its rows in order, the 8 values of a row left to right; the block by block_sum_store
//   sum of u^2, segment    : fp64 - thread k of 256 adds tiles k, k + 256, ..; the halving tree; d = max(1, sqrt(sum / numel) / clip_threshold)
// Rows and columns outside the segment contribute +0.0f, which changes no sum.
#include <math.h>

#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int TR = slam::AF_TILE_ROWS, TC = slam::AF_TILE_COLS;
using slam::AfSeg;

struct AfTile { int si, rb, cb; };
// the segment of block `b` of a numbering in which segment i starts at start(i): the last i with start(i) <= b (segments that
// own no block of the numbering precede, in the table, the one that shares their start)
template <typename F>
SLAM_DEVICE int af_find(int n, int b, F&& start) {
  int lo = 0, hi = n;
  while (lo + 1 < hi) {
    const int mid = (lo + hi) >> 1;
    if (start(mid) <= b) lo = mid;
    else hi = mid;
  }
  return lo;
}
SLAM_DEVICE AfTile af_tile(const AfSeg* segs, int n) {
  const int b = blockIdx.x;
  const int si = af_find(n, b, [&](int i) { return segs[i].tile0; });
  const int t = b - segs[si].tile0, ncb = segs[si].n_cb;
  return {si, t / ncb, t % ncb};
}
// flat index of element (row, col) of a segment
SLAM_DEVICE size_t af_elem(const AfSeg& s, int row, int col) {
  const int prow = s.phase < 0 ? row : ((row >> 5) << 6) + s.phase + (row & 31);
  return (size_t)s.off + (size_t)prow * (size_t)s.cols + (size_t)col;
}
template <typename GT>
SLAM_DEVICE void af_load8(const GT* q, float* f) {
  if constexpr (sizeof(GT) == 4) {
    const float4 a = *reinterpret_cast<const float4*>(q), b = *reinterpret_cast<const float4*>(q + 4);
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
  } else {
    unpack_bf16x8(*reinterpret_cast<const uint4*>(q), f);
  }
}
// every fp32 operation of the update is pinned (no contraction left to the compiler): the bf16-only step and the fp32-master
// step must reach the same fp32 value before they store it
SLAM_DEVICE float af_rsqrt(float x) { return 1.f / sqrtf(x); }
SLAM_DEVICE float af_sq_eps(float g_raw, float cs, float eps1) {
#pragma clang fp contract(off)
  const float g = g_raw * cs;
  return __builtin_fmaf(g, g, eps1);
}
SLAM_DEVICE float af_blend(float old, float mean, float beta, float omb) {
#pragma clang fp contract(off)
  return __builtin_fmaf(beta, old, omb * mean);
}
SLAM_DEVICE float af_u(float g_raw, float cs, float factor) {
#pragma clang fp contract(off)
  return factor * (g_raw * cs);
}

// pass 1: row partials and column partials of s over the factored segments
template <typename GT>
__global__ __launch_bounds__(256) void af_sums_kernel(const AfSeg* __restrict__ segs, int n_segs, const GT* __restrict__ g,
                                                      const float* __restrict__ clip, float eps1, float* __restrict__ ws) {
  const AfTile t = af_tile(segs, n_segs);
  const AfSeg s = segs[t.si];
  if (!s.factored) return;
  __shared__ float cpart[8][TC];
  const int tid = threadIdx.x, cg = tid & 31, rs = tid >> 5;
  const int r0 = t.rb * TR, col = t.cb * TC + cg * 8;
  const bool col_ok = col < s.cols;
  const float cs = clip ? clip[1] : 1.f;
  float cacc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int i = 0; i < TR / 8; ++i) {
    if (r0 + 8 * i >= s.rows) break;  // uniform: nothing of the segment further down
    const int row = r0 + rs + 8 * i;
    const bool ok = col_ok && row < s.rows;
    float sv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (ok) {
      float ga[8];
      af_load8<GT>(g + af_elem(s, row, col), ga);
#pragma unroll
      for (int j = 0; j < 8; ++j) sv[j] = af_sq_eps(ga[j], cs, eps1);
    }
    float rsum = sv[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) rsum += sv[j];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) rsum += __shfl_xor(rsum, o, 64);
    if (cg == 0 && row < s.rows) ws[s.rowpart + (int64_t)row * s.n_cb + t.cb] = rsum;
#pragma unroll
    for (int j = 0; j < 8; ++j) cacc[j] += sv[j];
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) cpart[rs][cg * 8 + j] = cacc[j];
  __syncthreads();
  const int c = t.cb * TC + tid;
  if (c < s.cols) {
    float v = cpart[0][tid];
#pragma unroll
    for (int k = 1; k < 8; ++k) v += cpart[k][tid];
    ws[s.colpart + (int64_t)t.rb * s.cols + c] = v;
  }
}
// pass 1, finish: factor j of a segment (rows first, then columns) <- beta old + (1 - beta) mean of s
__global__ __launch_bounds__(256) void af_finish_kernel(const AfSeg* __restrict__ segs, int n_segs, float* __restrict__ state,
                                                        const float* __restrict__ ws, float beta, float omb) {
  const int b = blockIdx.x;
  const int si = af_find(n_segs, b, [&](int i) { return segs[i].fin0; });
  const AfSeg s = segs[si];
  const int j = (b - s.fin0) * 256 + threadIdx.x;
  if (!s.factored || j >= s.rows + s.cols) return;
  float sum, len;
  if (j < s.rows) {
    const float* p = ws + s.rowpart + (int64_t)j * s.n_cb;
    sum = p[0];
    for (int k = 1; k < s.n_cb; ++k) sum += p[k];
    len = (float)s.cols;
  } else {
    const float* p = ws + s.colpart + (j - s.rows);
    sum = p[0];
    for (int k = 1; k < s.n_rb; ++k) sum += p[(int64_t)k * s.cols];
    len = (float)s.rows;
  }
  float* st = state + s.state + j;
  *st = af_blend(*st, sum / len, beta, omb);
}
// pass 2a: the mean of a segment's row factors, one block a segment
__global__ __launch_bounds__(256) void af_rowmean_kernel(const AfSeg* __restrict__ segs, const float* __restrict__ state,
                                                         float* __restrict__ out) {
  const AfSeg s = segs[blockIdx.x];
  if (!s.factored) return;
  __shared__ float red[256];
  float a = 0.f;
  for (int r = threadIdx.x; r < s.rows; r += 256) a += state[s.state + r];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = red[0] / (float)s.rows;
}
// the update u of a thread's 8 elements of one row: factored g rsqrt(row / mean) rsqrt(col); a vector g rsqrt(v)
struct AfRowCtx { float cf[8]; float mean; };
SLAM_DEVICE void af_ctx(const AfSeg& s, const float* state, float mean, int col, AfRowCtx& c) {
  c.mean = mean;
  if (s.factored) {
#pragma unroll
    for (int j = 0; j < 8; ++j) c.cf[j] = af_rsqrt(state[s.state + s.rows + col + j]);
  }
}
SLAM_DEVICE float af_rowfactor(const AfSeg& s, const float* state, float mean, int row) {
  return af_rsqrt(state[s.state + row] / mean);
}

// pass 2b: sum of u^2 of every tile; a vector's second moment is updated here (one thread owns an element)
template <typename GT>
__global__ __launch_bounds__(256) void af_usq_kernel(const AfSeg* __restrict__ segs, int n_segs, const GT* __restrict__ g,
                                                     const float* __restrict__ clip, float eps1, float beta, float omb,
                                                     float* __restrict__ state, const float* __restrict__ segmean,
                                                     float* __restrict__ tilepart) {
  const AfTile t = af_tile(segs, n_segs);
  const AfSeg s = segs[t.si];
  __shared__ float red[4];
  const int tid = threadIdx.x, cg = tid & 31, rs = tid >> 5;
  const int r0 = t.rb * TR, col = t.cb * TC + cg * 8;
  const bool col_ok = col < s.cols;
  const float cs = clip ? clip[1] : 1.f;
  AfRowCtx cx;
  if (col_ok) af_ctx(s, state, s.factored ? segmean[t.si] : 1.f, col, cx);
  float acc = 0.f;
#pragma unroll 4
  for (int i = 0; i < TR / 8; ++i) {
    if (r0 + 8 * i >= s.rows) break;
    const int row = r0 + rs + 8 * i;
    if (!(col_ok && row < s.rows)) continue;
    float ga[8];
    af_load8<GT>(g + af_elem(s, row, col), ga);
    if (s.factored) {
      const float rf = af_rowfactor(s, state, cx.mean, row);
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float u = af_u(ga[j], cs, rf * cx.cf[j]); acc += u * u; }
    } else {
      float* v = state + s.state + col;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float vn = af_blend(v[j], af_sq_eps(ga[j], cs, eps1), beta, omb);
        v[j] = vn;
        const float u = af_u(ga[j], cs, af_rsqrt(vn));
        acc += u * u;
      }
    }
  }
  block_sum_store<4>(acc, red, tilepart + blockIdx.x);
}
// pass 2c: d = max(1, RMS(u) / clip_threshold) of a segment, one block a segment, in fp64
__global__ __launch_bounds__(256) void af_segd_kernel(const AfSeg* __restrict__ segs, const float* __restrict__ tilepart,
                                                      float clip_threshold, float* __restrict__ out) {
  const AfSeg s = segs[blockIdx.x];
  __shared__ double red[256];
  const int nt = s.n_rb * s.n_cb;
  double a = 0.0;
  for (int k = threadIdx.x; k < nt; k += 256) a += (double)tilepart[s.tile0 + k];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float rms = (float)sqrt(red[0] / ((double)s.rows * (double)s.cols));
    out[blockIdx.x] = fmaxf(1.f, rms / clip_threshold);
  }
}
struct AfHyper { float lr, wd; SrKey sr; const uint64_t* nd; int nd_n; };
SLAM_DEVICE float af_step(float p, float u, float d, float lr, float wd) {
#pragma clang fp contract(off)
  p = __builtin_fmaf(-(wd * lr), p, p);
  return p - (u / d) * lr;
}
// pass 3: p <- p - wd lr p, then p <- p - lr u / d; MASTER: the fp32 master is the state and the bf16 copy is written from it;
// else the bf16 parameters are read, updated in fp32 and rounded once (SR: stochastically, array 0, keyed on the flat index)
template <typename GT, bool MASTER, bool SR>
__global__ __launch_bounds__(256) void af_apply_kernel(const AfSeg* __restrict__ segs, int n_segs, const GT* __restrict__ g,
                                                       const float* __restrict__ clip, const float* __restrict__ state,
                                                       const float* __restrict__ segmean, const float* __restrict__ segd,
                                                       float* __restrict__ master, bf16_t* __restrict__ params, AfHyper h) {
  const AfTile t = af_tile(segs, n_segs);
  const AfSeg s = segs[t.si];
  const int tid = threadIdx.x, cg = tid & 31, rs = tid >> 5;
  const int r0 = t.rb * TR, col = t.cb * TC + cg * 8;
  if (col >= s.cols) return;
  const float cs = clip ? clip[1] : 1.f;
  float wd = h.wd;
  if (h.nd) {  // the number of bounds <= the segment's first element: odd = inside a no-decay range (uniform: scalar loads)
    int lo = 0, hi = h.nd_n;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (h.nd[mid] <= (uint64_t)s.off) lo = mid + 1;
      else hi = mid;
    }
    if (lo & 1) wd = 0.f;
  }
  const float d = segd[t.si];
  AfRowCtx cx;
  af_ctx(s, state, s.factored ? segmean[t.si] : 1.f, col, cx);
#pragma unroll 4
  for (int i = 0; i < TR / 8; ++i) {
    if (r0 + 8 * i >= s.rows) break;
    const int row = r0 + rs + 8 * i;
    if (row >= s.rows) continue;
    const size_t e = af_elem(s, row, col);
    float ga[8], pa[8];
    af_load8<GT>(g + e, ga);
    if constexpr (MASTER) af_load8<float>(master + e, pa);
    else unpack_bf16x8(*reinterpret_cast<const uint4*>(params + e), pa);
    if (s.factored) {
      const float rf = af_rowfactor(s, state, cx.mean, row);
#pragma unroll
      for (int j = 0; j < 8; ++j) pa[j] = af_step(pa[j], af_u(ga[j], cs, rf * cx.cf[j]), d, h.lr, wd);
    } else {
      const float* v = state + s.state + col;
#pragma unroll
      for (int j = 0; j < 8; ++j) pa[j] = af_step(pa[j], af_u(ga[j], cs, af_rsqrt(v[j])), d, h.lr, wd);
    }
    if constexpr (MASTER) {
      *reinterpret_cast<float4*>(master + e) = make_float4(pa[0], pa[1], pa[2], pa[3]);
      *reinterpret_cast<float4*>(master + e + 4) = make_float4(pa[4], pa[5], pa[6], pa[7]);
    }
    if constexpr (SR && !MASTER) *reinterpret_cast<uint4*>(params + e) = sr_pack_bf16x8(pa, h.sr, (uint64_t)e, 0);
    else *reinterpret_cast<uint4*>(params + e) = pack_bf16x8(pa);
  }
}

}  // namespace

namespace slam {

void adafactor_layout(AfSeg* segs, int n, AfPlan* plan) {
  int64_t state = 0, ws = 0;
  int tiles = 0, fin = 0;
  for (int i = 0; i < n; ++i) {
    AfSeg& s = segs[i];
    s.n_rb = (s.rows + AF_TILE_ROWS - 1) / AF_TILE_ROWS;
    s.n_cb = (s.cols + AF_TILE_COLS - 1) / AF_TILE_COLS;
    s.tile0 = tiles;
    tiles += s.n_rb * s.n_cb;
    s.fin0 = fin;
    s.state = state;
    if (s.factored) {
      fin += (s.rows + s.cols + 255) / 256;
      state += (int64_t)s.rows + s.cols;
      s.rowpart = ws;
      ws += (int64_t)s.rows * s.n_cb;
      s.colpart = ws;
      ws += (int64_t)s.n_rb * s.cols;
    } else {
      state += (int64_t)s.rows * s.cols;
    }
  }
  plan->n_segs = n; plan->n_tiles = tiles; plan->n_fin = fin;
  plan->state_floats = state;
  plan->segmean = ws; ws += n;
  plan->segd = ws; ws += n;
  plan->tilepart = ws; ws += tiles;
  plan->ws_floats = ws;
}

template <bool B> using AfFlag = std::integral_constant<bool, B>;
template <typename F> static void af_with(bool b, F&& f) { if (b) f(AfFlag<true>{}); else f(AfFlag<false>{}); }

int adafactor_step(const AfPlan& pl, const AfArgs& a, hipStream_t st) {
  if (pl.n_segs <= 0 || !pl.segs || !a.params || !a.g || !a.state || !a.ws) return -1;
  float* ws = a.ws;
  AfHyper h;
  h.lr = a.lr; h.wd = a.wd;
  h.sr = {(uint32_t)(a.sr.seed & 0xffffffffu), (uint32_t)(a.sr.seed >> 32), (uint32_t)a.step, 0u, 0u};
  h.nd = a.nd.bounds; h.nd_n = a.nd.n;
  const bool sr = a.sr.on && !a.master;
  af_with(a.g_bf16 != 0, [&](auto g16) {
    using GT = std::conditional_t<decltype(g16)::value, bf16_t, float>;
    const GT* g = (const GT*)a.g;
    af_sums_kernel<GT><<<pl.n_tiles, 256, 0, st>>>(pl.segs, pl.n_segs, g, a.clip, a.eps1, ws);
    if (pl.n_fin) af_finish_kernel<<<pl.n_fin, 256, 0, st>>>(pl.segs, pl.n_segs, a.state, ws, a.beta, a.one_minus_beta);
    af_rowmean_kernel<<<pl.n_segs, 256, 0, st>>>(pl.segs, a.state, ws + pl.segmean);
    af_usq_kernel<GT><<<pl.n_tiles, 256, 0, st>>>(pl.segs, pl.n_segs, g, a.clip, a.eps1, a.beta, a.one_minus_beta, a.state,
                                                  ws + pl.segmean, ws + pl.tilepart);
    af_segd_kernel<<<pl.n_segs, 256, 0, st>>>(pl.segs, ws + pl.tilepart, a.clip_threshold, ws + pl.segd);
    af_with(a.master != nullptr, [&](auto master) {
      af_with(sr, [&](auto srf) {
        if constexpr (!(decltype(master)::value && decltype(srf)::value))
          af_apply_kernel<GT, decltype(master)::value, decltype(srf)::value><<<pl.n_tiles, 256, 0, st>>>(
              pl.segs, pl.n_segs, g, a.clip, a.state, ws + pl.segmean, ws + pl.segd, a.master, a.params, h);
      });
    });
  });
  LAUNCH_RET();
}

}  // namespace slam
