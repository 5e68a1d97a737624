// Muon for gfx950: torch.optim.Muon (torch 2.10, _single_tensor_muon / _zeropower_via_newtonschulz) over the decoder layers'
// matrices laid across the engine's flat buffer (kernels.h MuSeg). The contract is in include/slam_engine.h (slam_muon_step).
//
// A step = one prepare launch (all matrices), per shape class one scale launch and 3 ns_steps product launches over the class's
// matrices as one batch, and one apply launch (all matrices): 2 + classes (1 + 3 ns_steps) launches for any number of layers.
//
// prepare / apply: a block owns a 64 x 64 tile of an HF matrix and finds it by a binary search of the class-sorted table on
// wave-uniform loads. Thread t owns the 8 consecutive columns 8 (t % 8) .. of the tile rows t / 8 and t / 8 + 32. A matrix
// with rows > cols is packed transposed through a [64][72] bf16 LDS tile, 16 bytes per access on both sides.
//
// product kernels: 128 x 128 output tile, 4 waves of 64 x 64 (4 x 4 v_mfma_f32_16x16x32_bf16 fragments), 64-deep K-tiles
// staged global -> registers -> LDS with the next K-tile's loads in flight under the MFMAs. Operands with the contraction
// index contiguous ([128][64], 144-byte rows: conflict-free ds_read_b128) are read directly; the [k][j] operand of P X ([64][128],
// 288-byte rows) through ds_read_b64_tr_b16. Rows and columns beyond the matrix are zeros in LDS and masked at the store.
//
// The summation orders (fp32):
//   sum of squares, prepare tile : a thread adds x^2 of its row t / 8 left to right, then of row t / 8 + 32 (elements outside the
//                                  matrix add +0.0f); the block by block_sum_store (xor butterfly 32 .. 1, waves in wave order)
//   sum of squares, 8192 chunk   : (muon_ns without prepare's partials) thread t adds its 8 elements 8 (t + 256 i) .. left to
//                                  right, i = 0 .. 3 in order; the block by block_sum_store
//   sum of squares, matrix       : thread k of 256 adds partials k, k + 256, ..; the halving tree 128, 64, .. 1
//   products                     : K-tiles in order, two 32-deep MFMA steps each, into one fp32 accumulator per element
#include <math.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "common.h"
#include "kernels.h"

namespace {

using slam::MuSeg;
constexpr int TL = slam::MU_TILE;

struct MuTile { int si, tr, tc; };
SLAM_DEVICE MuTile mu_tile(const MuSeg* segs, int n) {
  const int b = blockIdx.x;
  int lo = 0, hi = n;
  while (lo + 1 < hi) {  // the last segment with tile0 <= b (every segment owns at least one tile)
    const int mid = (lo + hi) >> 1;
    if (segs[mid].tile0 <= b) lo = mid;
    else hi = mid;
  }
  const int t = b - segs[lo].tile0, ntc = segs[lo].n_tc;
  return {lo, t / ntc, t % ntc};
}
SLAM_DEVICE size_t mu_elem(const MuSeg& s, int row, int col) {
  const int prow = s.phase < 0 ? row : ((row >> 5) << 6) + s.phase + (row & 31);
  return (size_t)s.off + (size_t)prow * (size_t)s.cols + (size_t)col;
}
template <typename GT>
SLAM_DEVICE void mu_load8(const GT* q, float* f) {
  if constexpr (sizeof(GT) == 4) {
    const float4 a = *reinterpret_cast<const float4*>(q), b = *reinterpret_cast<const float4*>(q + 4);
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
  } else {
    unpack_bf16x8(*reinterpret_cast<const uint4*>(q), f);
  }
}
SLAM_DEVICE void mu_store8(float* q, const float* f) {
  *reinterpret_cast<float4*>(q) = make_float4(f[0], f[1], f[2], f[3]);
  *reinterpret_cast<float4*>(q + 4) = make_float4(f[4], f[5], f[6], f[7]);
}
// every fp32 operation is rounded by itself (no contraction left to the compiler)
SLAM_DEVICE float mu_momentum(float bold, float g, float mu, float omm) {
#pragma clang fp contract(off)
  const float x = mu * bold, y = omm * g;
  return x + y;
}
SLAM_DEVICE float mu_nesterov(float bnew, float g, float mu, float omm) {
#pragma clang fp contract(off)
  const float x = omm * g, y = mu * bnew;
  return x + y;
}
SLAM_DEVICE float mu_add_sq(float acc, float x) {
#pragma clang fp contract(off)
  const float q = x * x;
  return acc + q;
}
SLAM_DEVICE float mu_update(float p, float decay, float lr_adj, float o) {
#pragma clang fp contract(off)
  const float d = p * decay, u = lr_adj * o;
  return d - u;
}
SLAM_DEVICE float bf16_round(float x) { return bf16_to_f32(f32_to_bf16(x)); }

// ---- prepare: B <- mu B + (1 - mu) g; U = (1 - mu) g + mu B (Nesterov) or B; packed X = bf16(U); partial sums of bf16(U)^2 ----
template <typename GT>
__global__ __launch_bounds__(256) void mu_prepare_kernel(const MuSeg* __restrict__ segs, int n_segs, const GT* g,
                                                         float* gzero, const float* __restrict__ clip,
                                                         float* __restrict__ mom, bf16_t* __restrict__ X, float* __restrict__ part,
                                                         float mu, float omm, int nesterov) {
  const MuTile t = mu_tile(segs, n_segs);
  const MuSeg s = segs[t.si];
  __shared__ __attribute__((aligned(16))) bf16_t sm[TL][TL + 8];
  __shared__ float red[4];
  const int tid = threadIdx.x, cg = tid & 7, rr = tid >> 3;
  const bool transposed = s.rows > s.cols;
  const int col = t.tc * TL + cg * 8;
  const float cs = clip ? clip[1] : 1.f;
  bf16_t* const Xs = X + s.pack;
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int lr = rr + 32 * i, row = t.tr * TL + lr;
    const bool ok = col < s.cols && row < s.rows;
    float u[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (ok) {
      const size_t e = mu_elem(s, row, col);
      float ga[8], ba[8];
      mu_load8<GT>(g + e, ga);
      float* mp = mom + s.mom + (size_t)row * s.cols + col;
      mu_load8<float>(mp, ba);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float gg = ga[j] * cs;
        ba[j] = mu_momentum(ba[j], gg, mu, omm);
        u[j] = nesterov ? mu_nesterov(ba[j], gg, mu, omm) : ba[j];
      }
      mu_store8(mp, ba);
      if (gzero) {
        const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        mu_store8(gzero + e, z);
      }
    }
    const uint4 pk = pack_bf16x8(u);
    float xr[8];
    unpack_bf16x8(pk, xr);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = mu_add_sq(acc, xr[j]);
    if (transposed) *reinterpret_cast<uint4*>(&sm[lr][cg * 8]) = pk;
    else if (ok) *reinterpret_cast<uint4*>(Xs + (size_t)row * s.cols + col) = pk;
  }
  if (transposed) {  // uniform over the block
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int pc = rr + 32 * i, scol = t.tc * TL + pc, srow = t.tr * TL + cg * 8;
      if (scol < s.cols && srow < s.rows) {
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = (uint32_t)sm[cg * 8 + 2 * j][pc] | ((uint32_t)sm[cg * 8 + 2 * j + 1][pc] << 16);
        *reinterpret_cast<uint4*>(Xs + (size_t)scol * s.rows + srow) = make_uint4(w[0], w[1], w[2], w[3]);
      }
    }
  }
  block_sum_store<4>(acc, red, part + blockIdx.x);
}

// ---- apply: p <- p (1 - lr wd); p <- p - lr_adj O, scattered through the row pattern, one rounding ----
struct MuHyper { double lr; float decay; int adjust_lr; SrKey sr; const uint64_t* nd; int nd_n; };
template <bool MASTER, bool SR>
__global__ __launch_bounds__(256) void mu_apply_kernel(const MuSeg* __restrict__ segs, int n_segs, const bf16_t* __restrict__ O,
                                                       float* __restrict__ master, bf16_t* __restrict__ params, MuHyper h) {
  const MuTile t = mu_tile(segs, n_segs);
  const MuSeg s = segs[t.si];
  __shared__ __attribute__((aligned(16))) bf16_t sm[TL][TL + 8];
  const int tid = threadIdx.x, cg = tid & 7, rr = tid >> 3;
  const bool transposed = s.rows > s.cols;
  const int col = t.tc * TL + cg * 8;
  const bf16_t* const Os = O + s.pack;
  float decay = h.decay;
  if (h.nd) {  // the number of bounds <= the segment's first element: odd = inside a no-decay range (uniform: scalar loads)
    int lo = 0, hi = h.nd_n;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (h.nd[mid] <= (uint64_t)s.off) lo = mid + 1;
      else hi = mid;
    }
    if (lo & 1) decay = 1.f;
  }
  // lr_adj in double as python computes it, rounded to fp32 once
  double ratio = 1.0;
  if (h.adjust_lr == 1) ratio = sqrt(fmax(1.0, (double)s.rows / (double)s.cols));
  else if (h.adjust_lr == 2) ratio = 0.2 * sqrt((double)max(s.rows, s.cols));
  const float lr_adj = (float)(h.lr * ratio);
  if (transposed) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int pc = rr + 32 * i, scol = t.tc * TL + pc, srow = t.tr * TL + cg * 8;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (scol < s.cols && srow < s.rows) v = *reinterpret_cast<const uint4*>(Os + (size_t)scol * s.rows + srow);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sm[cg * 8 + 2 * j][pc] = (bf16_t)(w[j] & 0xffffu);
        sm[cg * 8 + 2 * j + 1][pc] = (bf16_t)(w[j] >> 16);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int lr = rr + 32 * i, row = t.tr * TL + lr;
    if (!(col < s.cols && row < s.rows)) continue;
    const size_t e = mu_elem(s, row, col);
    float oa[8], pa[8];
    if (transposed) unpack_bf16x8(*reinterpret_cast<const uint4*>(&sm[lr][cg * 8]), oa);
    else unpack_bf16x8(*reinterpret_cast<const uint4*>(Os + (size_t)row * s.cols + col), oa);
    if constexpr (MASTER) mu_load8<float>(master + e, pa);
    else unpack_bf16x8(*reinterpret_cast<const uint4*>(params + e), pa);
#pragma unroll
    for (int j = 0; j < 8; ++j) pa[j] = mu_update(pa[j], decay, lr_adj, oa[j]);
    if constexpr (MASTER) mu_store8(master + e, pa);
    if constexpr (SR && !MASTER) *reinterpret_cast<uint4*>(params + e) = sr_pack_bf16x8(pa, h.sr, (uint64_t)e, 0);
    else *reinterpret_cast<uint4*>(params + e) = pack_bf16x8(pa);
  }
}

// ---- norm: chunk partials of a packed batch, and X / max(bf16(sqrt(sum)), bf16(eps)) ----
constexpr int NC = slam::MU_NORM_CHUNK;
__global__ __launch_bounds__(256) void mu_sumsq_kernel(const bf16_t* __restrict__ X, int64_t sx, int64_t nm, float* __restrict__ part,
                                                       int parts) {
  __shared__ float red[4];
  const bf16_t* x = X + (size_t)blockIdx.y * sx;
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < NC / 2048; ++i) {
    const int64_t e = (int64_t)blockIdx.x * NC + (int64_t)(threadIdx.x + 256 * i) * 8;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (e < nm) unpack_bf16x8(*reinterpret_cast<const uint4*>(x + e), v);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = mu_add_sq(acc, v[j]);
  }
  block_sum_store<4>(acc, red, part + (size_t)blockIdx.y * parts + blockIdx.x);
}
__global__ __launch_bounds__(256) void mu_scale_kernel(const bf16_t* __restrict__ X, int64_t sx, bf16_t* __restrict__ D, int64_t sd,
                                                       int64_t nm, const float* __restrict__ part, int parts, float eps) {
  __shared__ float red[256];
  const float* p = part + (size_t)blockIdx.y * parts;
  float a = 0.f;
  for (int k = threadIdx.x; k < parts; k += 256) a += p[k];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  const float nrm = fmaxf(bf16_round(sqrtf(red[0])), bf16_round(eps));
  const bf16_t* x = X + (size_t)blockIdx.y * sx;
  bf16_t* d = D + (size_t)blockIdx.y * sd;
#pragma unroll
  for (int i = 0; i < NC / 2048; ++i) {
    const int64_t e = (int64_t)blockIdx.x * NC + (int64_t)(threadIdx.x + 256 * i) * 8;
    if (e >= nm) continue;
    float v[8];
    unpack_bf16x8(*reinterpret_cast<const uint4*>(x + e), v);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = v[j] / nrm;
    *reinterpret_cast<uint4*>(d + e) = pack_bf16x8(v);
  }
}

// ---- the batched product kernels ----
constexpr int MT = 128, KT = 64;
constexpr int ROWB = KT * 2 + 16;   // bytes per row of a [128][64] operand tile
constexpr int NNB = MT * 2 + 32;    // bytes per contraction row of the [64][128] operand tile
constexpr int TILE_BYTES = MT * ROWB;
static_assert(KT * NNB <= TILE_BYTES, "the [k][j] tile fits the operand slot");
struct MuMM {
  const bf16_t *A, *B, *R;
  bf16_t* C;
  int M, N, K, lda, ldb, ldc;
  int64_t sA, sB, sR, sC;
  float alpha, beta;
};
// SYM: C = beta R + alpha A A^T (B = A; the tiles on or below the diagonal, numbered row by row; an off-diagonal tile is stored
// twice); else C = beta R + alpha A B with B [K][N]
template <bool SYM>
__global__ __launch_bounds__(256) void mu_mm_kernel(MuMM p) {
  __shared__ __attribute__((aligned(16))) char smem[2 * TILE_BYTES];
  int ti, tj;
  if constexpr (SYM) {
    const int t = blockIdx.x;
    ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    tj = t - ti * (ti + 1) / 2;
  } else {
    const int ntj = (p.N + MT - 1) / MT;
    ti = blockIdx.x / ntj;
    tj = blockIdx.x % ntj;
  }
  const size_t bi = blockIdx.y;
  const bf16_t* A = p.A + bi * p.sA;
  const bf16_t* B = p.B + bi * p.sB;
  const bf16_t* R = p.R ? p.R + bi * p.sR : nullptr;
  bf16_t* C = p.C + bi * p.sC;
  const int row0 = ti * MT, col0 = tj * MT;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wm = w >> 1, wn = w & 1, l15 = lane & 15, g = lane >> 4;
  char* const As = smem;
  char* const Bs = smem + TILE_BYTES;

  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  uint4 ra[4], rb[4];
  auto gload = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = tid + 256 * i;
      {
        const int r = c >> 3, gk = k0 + (c & 7) * 8, gr = row0 + r;
        ra[i] = (gr < p.M && gk < p.K) ? *reinterpret_cast<const uint4*>(A + (size_t)gr * p.lda + gk) : make_uint4(0u, 0u, 0u, 0u);
      }
      if constexpr (SYM) {
        const int r = c >> 3, gk = k0 + (c & 7) * 8, gr = col0 + r;
        rb[i] = (gr < p.N && gk < p.K) ? *reinterpret_cast<const uint4*>(B + (size_t)gr * p.ldb + gk) : make_uint4(0u, 0u, 0u, 0u);
      } else {
        const int gk = k0 + (c >> 4), gj = col0 + (c & 15) * 8;
        rb[i] = (gk < p.K && gj < p.N) ? *reinterpret_cast<const uint4*>(B + (size_t)gk * p.ldb + gj) : make_uint4(0u, 0u, 0u, 0u);
      }
    }
  };
  auto sstore = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = tid + 256 * i;
      *reinterpret_cast<uint4*>(As + (c >> 3) * ROWB + (c & 7) * 16) = ra[i];
      if constexpr (SYM) *reinterpret_cast<uint4*>(Bs + (c >> 3) * ROWB + (c & 7) * 16) = rb[i];
      else *reinterpret_cast<uint4*>(Bs + (c >> 4) * NNB + (c & 15) * 16) = rb[i];
    }
  };

  const int nk = (p.K + KT - 1) / KT;
  gload(0);
  for (int kt = 0; kt < nk; ++kt) {
    __syncthreads();  // the MFMAs of the previous K-tile have read LDS
    sstore();
    __syncthreads();
    if (kt + 1 < nk) gload((kt + 1) * KT);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      uint4 af[4], bf[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        af[f] = *reinterpret_cast<const uint4*>(As + (wm * 64 + f * 16 + l15) * ROWB + kk * 64 + g * 16);
        if constexpr (SYM) {
          bf[f] = *reinterpret_cast<const uint4*>(Bs + (wn * 64 + f * 16 + l15) * ROWB + kk * 64 + g * 16);
        } else {
          const char* q = Bs + (kk * 32 + g * 8 + (l15 >> 2)) * NNB + (wn * 64 + f * 16) * 2 + (l15 & 3) * 8;
          const uint2 lo = lds_tr_read(q), hi = lds_tr_read(q + 4 * NNB);
          bf[f] = make_uint4(lo.x, lo.y, hi.x, hi.y);
        }
      }
      // the column-side fragment is the MFMA's row operand: a lane ends up with 4 consecutive columns of one output row
#pragma unroll
      for (int fm = 0; fm < 4; ++fm)
#pragma unroll
        for (int fn = 0; fn < 4; ++fn) acc[fm][fn] = mfma16(bf[fn], af[fm], acc[fm][fn]);
    }
  }

  const bool mirror = SYM && ti != tj;
#pragma unroll
  for (int fm = 0; fm < 4; ++fm) {
    const int row = row0 + wm * 64 + fm * 16 + l15;
#pragma unroll
    for (int fn = 0; fn < 4; ++fn) {
      const int col = col0 + wn * 64 + fn * 16 + g * 4;
      if (row >= p.M || col >= p.N) continue;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = p.alpha * acc[fm][fn][r];
      if (R) {
        const uint2 rv = *reinterpret_cast<const uint2*>(R + (size_t)row * p.ldc + col);
        const float rf[4] = {__uint_as_float(rv.x << 16), __uint_as_float(rv.x & 0xffff0000u), __uint_as_float(rv.y << 16),
                             __uint_as_float(rv.y & 0xffff0000u)};
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = __builtin_fmaf(p.beta, rf[r], v[r]);
      }
      const uint2 o = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
      *reinterpret_cast<uint2*>(C + (size_t)row * p.ldc + col) = o;
      if (mirror) {
        C[(size_t)(col + 0) * p.ldc + row] = (bf16_t)(o.x & 0xffffu);
        C[(size_t)(col + 1) * p.ldc + row] = (bf16_t)(o.x >> 16);
        C[(size_t)(col + 2) * p.ldc + row] = (bf16_t)(o.y & 0xffffu);
        C[(size_t)(col + 3) * p.ldc + row] = (bf16_t)(o.y >> 16);
      }
    }
  }
}

inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }
inline bool mm_dims_ok(int batch, int n, int m) { return batch >= 1 && batch <= 65535 && n >= 8 && m >= 8 && !(n & 7) && !(m & 7); }

}  // namespace

namespace slam {

int muon_layout(MuSeg* segs, int n, MuPlan* plan) {
  MuPlan pl;
  std::vector<int> cls_of(n);
  int64_t mom = 0;
  for (int i = 0; i < n; ++i) {
    segs[i].mom = mom;
    mom += (int64_t)segs[i].rows * segs[i].cols;
    int c = 0;
    while (c < pl.n_classes && !(pl.cls[c].rows == segs[i].rows && pl.cls[c].cols == segs[i].cols)) ++c;
    if (c == pl.n_classes) {
      if (c == MU_MAX_CLASSES) return -1;
      pl.cls[c].rows = segs[i].rows; pl.cls[c].cols = segs[i].cols;
      pl.cls[c].n = std::min(segs[i].rows, segs[i].cols); pl.cls[c].m = std::max(segs[i].rows, segs[i].cols);
      ++pl.n_classes;
    }
    cls_of[i] = c;
    ++pl.cls[c].count;
  }
  std::vector<int> order(n);
  for (int i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return cls_of[x] < cls_of[y]; });
  std::vector<MuSeg> sorted(n);
  int64_t tiles = 0, pack = 0, max_xy = 0, max_aa = 0;
  int last = -1;
  for (int k = 0; k < n; ++k) {
    MuSeg s = segs[order[k]];
    const int c = cls_of[order[k]];
    const int ntr = (s.rows + MU_TILE - 1) / MU_TILE;
    s.n_tc = (s.cols + MU_TILE - 1) / MU_TILE;
    if (c != last) {
      pl.cls[c].pack = pack; pl.cls[c].part0 = (int)tiles; pl.cls[c].parts = ntr * s.n_tc;
      max_xy = std::max(max_xy, (int64_t)pl.cls[c].count * pl.cls[c].n * pl.cls[c].m);
      max_aa = std::max(max_aa, (int64_t)pl.cls[c].count * pl.cls[c].n * pl.cls[c].n);
      last = c;
    }
    s.tile0 = (int)tiles;
    s.pack = pack;
    tiles += (int64_t)ntr * s.n_tc;
    pack += (int64_t)s.rows * s.cols;
    if (tiles > 0x7fffffff) return -1;
    sorted[k] = s;
  }
  for (int k = 0; k < n; ++k) segs[k] = sorted[k];
  pl.n_segs = n; pl.n_tiles = (int)tiles; pl.elems = pack;
  size_t o = 0;
  pl.x_off = o; o += al256((size_t)pack * 2);
  pl.y_off = o; o += al256((size_t)max_xy * 2);
  pl.a_off = o; o += al256((size_t)max_aa * 2);
  pl.p_off = o; o += al256((size_t)max_aa * 2);
  pl.part_off = o; o += al256((size_t)tiles * 4);
  pl.ws_bytes = o;
  *plan = pl;
  return 0;
}

int muon_prepare(const MuPlan& pl, const MuArgs& a, hipStream_t st) {
  if (pl.n_segs <= 0 || !pl.segs || !a.g || !a.mom || !a.ws) return -1;
  bf16_t* X = (bf16_t*)(a.ws + pl.x_off);
  float* part = (float*)(a.ws + pl.part_off);
  if (a.g_bf16)
    mu_prepare_kernel<bf16_t><<<pl.n_tiles, 256, 0, st>>>(pl.segs, pl.n_segs, (const bf16_t*)a.g, a.gzero, a.clip, a.mom, X, part, a.mu,
                                                          a.omm, a.nesterov);
  else
    mu_prepare_kernel<float><<<pl.n_tiles, 256, 0, st>>>(pl.segs, pl.n_segs, (const float*)a.g, a.gzero, a.clip, a.mom, X, part, a.mu,
                                                         a.omm, a.nesterov);
  LAUNCH_RET();
}

int muon_apply(const MuPlan& pl, const MuArgs& a, const bf16_t* O, hipStream_t st) {
  if (pl.n_segs <= 0 || !pl.segs || !a.params || !O) return -1;
  MuHyper h;
  h.lr = a.lr;
  h.decay = (float)(1.0 - a.lr * a.wd);
  h.adjust_lr = a.adjust_lr;
  h.sr = {(uint32_t)(a.sr.seed & 0xffffffffu), (uint32_t)(a.sr.seed >> 32), (uint32_t)a.step, 0u, 0u};
  h.nd = a.nd.bounds; h.nd_n = a.nd.n;
  if (a.master) mu_apply_kernel<true, false><<<pl.n_tiles, 256, 0, st>>>(pl.segs, pl.n_segs, O, a.master, a.params, h);
  else if (a.sr.on) mu_apply_kernel<false, true><<<pl.n_tiles, 256, 0, st>>>(pl.segs, pl.n_segs, O, a.master, a.params, h);
  else mu_apply_kernel<false, false><<<pl.n_tiles, 256, 0, st>>>(pl.segs, pl.n_segs, O, a.master, a.params, h);
  LAUNCH_RET();
}

int muon_syrk(const bf16_t* X, const bf16_t* R, bf16_t* C, int batch, int n, int m, int64_t sx, int64_t sr, int64_t sc, float alpha,
              float beta, hipStream_t st) {
  if (!X || !C || !mm_dims_ok(batch, n, m) || ((sx | sr | sc) & 7) || sx < 0 || sr < 0 || sc < 0) return -1;
  MuMM p{X, X, R, C, n, n, m, m, m, n, sx, sx, sr, sc, alpha, beta};
  const int T = (n + MT - 1) / MT;
  mu_mm_kernel<true><<<dim3((unsigned)(T * (T + 1) / 2), (unsigned)batch), 256, 0, st>>>(p);
  LAUNCH_RET();
}

int muon_mm(const bf16_t* P, const bf16_t* X, const bf16_t* R, bf16_t* Y, int batch, int n, int m, int64_t sp, int64_t sx, int64_t sr,
            int64_t sy, float alpha, float beta, hipStream_t st) {
  if (!P || !X || !Y || !mm_dims_ok(batch, n, m) || ((sp | sx | sr | sy) & 7) || sp < 0 || sx < 0 || sr < 0 || sy < 0) return -1;
  MuMM p{P, X, R, Y, n, m, n, n, m, m, sp, sx, sr, sy, alpha, beta};
  const unsigned tiles = (unsigned)(((n + MT - 1) / MT) * ((m + MT - 1) / MT));
  mu_mm_kernel<false><<<dim3(tiles, (unsigned)batch), 256, 0, st>>>(p);
  LAUNCH_RET();
}

size_t muon_ns_workspace_bytes(int batch, int n, int m) {
  if (!mm_dims_ok(batch, n, m)) return 0;
  return al256((size_t)batch * n * m * 2) + 2 * al256((size_t)batch * n * n * 2) + al256((size_t)batch * muon_ns_partials(n, m) * 4);
}

int muon_ns(bf16_t* X, int batch, int n, int m, int64_t sx, const float* part, int parts, int ns_steps, float a, float b, float c,
            float eps, bf16_t* Y, bf16_t* A, bf16_t* P, float* part_scratch, hipStream_t st) {
  if (!X || !Y || !A || !P || !mm_dims_ok(batch, n, m) || n > m || sx < (int64_t)n * m || (sx & 7) || ns_steps < 1) return -1;
  const int64_t nm = (int64_t)n * m, nn = (int64_t)n * n;
  const unsigned chunks = (unsigned)muon_ns_partials(n, m);
  if (!part) {
    if (!part_scratch) return -1;
    mu_sumsq_kernel<<<dim3(chunks, (unsigned)batch), 256, 0, st>>>(X, sx, nm, part_scratch, (int)chunks);
    part = part_scratch;
    parts = (int)chunks;
  }
  // the last product writes into X: an odd number of iterations starts from the normalised copy in Y
  bf16_t *cur = (ns_steps & 1) ? Y : X, *oth = (ns_steps & 1) ? X : Y;
  int64_t scur = (ns_steps & 1) ? nm : sx, soth = (ns_steps & 1) ? sx : nm;
  mu_scale_kernel<<<dim3(chunks, (unsigned)batch), 256, 0, st>>>(X, sx, cur, scur, nm, part, parts, eps);
  HIP_CHECK_RET(hipGetLastError());
  for (int it = 0; it < ns_steps; ++it) {
    if (int r = muon_syrk(cur, nullptr, A, batch, n, m, scur, 0, nn, 1.f, 0.f, st)) return r;
    if (int r = muon_syrk(A, A, P, batch, n, n, nn, nn, nn, c, b, st)) return r;
    if (int r = muon_mm(P, cur, cur, oth, batch, n, m, nn, scur, scur, soth, 1.f, a, st)) return r;
    std::swap(cur, oth);
    std::swap(scur, soth);
  }
  return 0;
}

int muon_step(const MuPlan& pl, const MuArgs& a, hipStream_t st) {
  if (int r = muon_prepare(pl, a, st)) return r;
  bf16_t* X = (bf16_t*)(a.ws + pl.x_off);
  const float* part = (const float*)(a.ws + pl.part_off);
  for (int c = 0; c < pl.n_classes; ++c) {
    const MuClass& k = pl.cls[c];
    if (int r = muon_ns(X + k.pack, k.count, k.n, k.m, (int64_t)k.n * k.m, part + k.part0, k.parts, a.ns_steps, a.a, a.b, a.c, a.eps,
                        (bf16_t*)(a.ws + pl.y_off), (bf16_t*)(a.ws + pl.a_off), (bf16_t*)(a.ws + pl.p_off), nullptr, st))
      return r;
  }
  return muon_apply(pl, a, X, st);
}

}  // namespace slam
