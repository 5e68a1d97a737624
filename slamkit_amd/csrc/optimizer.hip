// The optimizer step's kernels for gfx950: the chunked gradient norm -> clip coefficient, AdamW in its three state precisions
// (flat, strided, and the tile form that also writes the transposed weight images), and the f32 <-> bf16 conversions and the
// bf16 transpose that go with them. Reference semantics: torch.optim.AdamW + HF clip_grad_norm_.
#include <stdlib.h>

#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace {

// ------------------------------------------------------------------------------------------
// Gradient norm (fp32 flat buffer) -> clip coefficient, and fused AdamW.
// Canonical chunked sum of squares: chunk k = elements [k C, (k+1) C) of the flat gradient buffer (absolute positions,
// C = GRAD_CHUNK), one block per chunk, fixed summation order inside it. Any partition of the buffer into chunk-aligned
// ranges - the whole buffer on one GPU, one 1/N shard per bucket per rank under the sharded optimizer - produces the
// same chunk sums bit for bit; norm_finish_kernel adds them in fp64 in chunk order.
constexpr int GRAD_CHUNK = 8192;
constexpr int CHUNKS_PER_BLOCK = 16;  // a block walks 16 consecutive chunks (512 KB): fewer, longer blocks stream better
// GT = float: the fp32 gradient buffer; GT = bf16_t: gradients kept in bf16 (same element order, so a value that is exactly
// representable in bf16 gives the same chunk sum through either instantiation)
template <typename GT>
__global__ __launch_bounds__(256) void sumsq_chunks_kernel(const GT* __restrict__ g, size_t n, size_t first_chunk, size_t n_chunks,
                                                           float* __restrict__ chunk_sums) {
  __shared__ float red[CHUNKS_PER_BLOCK][4];
  const size_t kb = (size_t)blockIdx.x * CHUNKS_PER_BLOCK;
  for (int c = 0; c < CHUNKS_PER_BLOCK && kb + c < n_chunks; ++c) {
    const size_t k = first_chunk + kb + c;
    const size_t lo = k * GRAD_CHUNK, hi = lo + GRAD_CHUNK < n ? lo + GRAD_CHUNK : n;
    float4 v[GRAD_CHUNK / 1024];
#pragma unroll
    for (int it = 0; it < GRAD_CHUNK / 1024; ++it) {  // all eight loads in flight before the first add
      const size_t i = lo + (size_t)(it * 256 + threadIdx.x) * 4;
      if (i < hi) {
        if constexpr (sizeof(GT) == 4) {
          v[it] = *reinterpret_cast<const float4*>(g + i);
        } else {
          const uint2 w = *reinterpret_cast<const uint2*>(g + i);
          v[it] = make_float4(__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u), __uint_as_float(w.y << 16),
                              __uint_as_float(w.y & 0xffff0000u));
        }
      } else {
        v[it] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    float s = 0.f;
#pragma unroll
    for (int it = 0; it < GRAD_CHUNK / 1024; ++it) s += v[it].x * v[it].x + v[it].y * v[it].y + v[it].z * v[it].z + v[it].w * v[it].w;
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[c][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x < CHUNKS_PER_BLOCK && kb + threadIdx.x < n_chunks)
    chunk_sums[first_chunk + kb + threadIdx.x] = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
}
// out[0] = ||g||, out[1] = clip coefficient min(1, max_norm/(norm+1e-6)) (1 when max_norm<=0)
// (one block of 1024: a thread adds its strided elements in four independent fp64 chains - the 43,760 chunk sums of the
// Slam-358M buffer took 60 us on 256 threads with one dependent chain each; the order is fixed, so every caller - the
// replicated and the sharded clip - gets the same bits)
__global__ __launch_bounds__(1024) void norm_finish_kernel(const float* __restrict__ part, int nb, float max_norm, float* __restrict__ out) {
  __shared__ double red[1024];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int i = threadIdx.x;
  for (; i + 3 * 1024 < nb; i += 4 * 1024) {
    s0 += (double)part[i]; s1 += (double)part[i + 1024]; s2 += (double)part[i + 2048]; s3 += (double)part[i + 3072];
  }
  for (; i < nb; i += 1024) s0 += (double)part[i];
  red[threadIdx.x] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  for (int k = 512; k > 0; k >>= 1) {
    if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    float nrm = (float)sqrt(red[0]);
    out[0] = nrm;
    float c = 1.f;
    if (max_norm > 0.f) { c = max_norm / (nrm + 1e-6f); if (c > 1.f) c = 1.f; }
    out[1] = c;
  }
}

// sr: the key of the stochastic rounding of the bf16 state stores (read by the SR = true kernels only)
struct AdamHyper { float lr, b1, b2, eps, wd, bc1, bc2_sqrt; int zero_grad; SrKey sr; };
// the no-decay table (kernels.h AdamNoDecay) as the last argument of a MASKED kernel; the others take an empty one and stay,
// instruction for instruction, the kernels they were before there was a table
struct NoDecayTab { const uint64_t* b; int n; uint64_t base; };
struct NoTab {};
template <bool MASKED> using NdArg = std::conditional_t<MASKED, NoDecayTab, NoTab>;
template <typename MT> SLAM_DEVICE void load4(const MT* q, float* f);
template <> SLAM_DEVICE void load4<float>(const float* q, float* f) {
  const float4 t = *reinterpret_cast<const float4*>(q);
  f[0] = t.x; f[1] = t.y; f[2] = t.z; f[3] = t.w;
}
template <> SLAM_DEVICE void load4<bf16_t>(const bf16_t* q, float* f) {
  const uint2 t = *reinterpret_cast<const uint2*>(q);
  f[0] = __uint_as_float(t.x << 16); f[1] = __uint_as_float(t.x & 0xffff0000u);
  f[2] = __uint_as_float(t.y << 16); f[3] = __uint_as_float(t.y & 0xffff0000u);
}
SLAM_DEVICE void store4(float* q, const float* f) { *reinterpret_cast<float4*>(q) = make_float4(f[0], f[1], f[2], f[3]); }
SLAM_DEVICE void store4(bf16_t* q, const float* f) {
  uint2 o;
  o.x = pack_bf16x2(f[0], f[1]); o.y = pack_bf16x2(f[2], f[3]);
  *reinterpret_cast<uint2*>(q) = o;
}
// the bf16 store of 4 consecutive state values at flat index gi of array `which`, rounded stochastically when SR
template <bool SR>
SLAM_DEVICE uint2 round4(const float* f, const SrKey& k, uint64_t gi, uint32_t which) {
  if constexpr (SR) return sr_pack_bf16x4(f, k, gi, which);
  uint2 o;
  o.x = pack_bf16x2(f[0], f[1]); o.y = pack_bf16x2(f[2], f[3]);
  return o;
}
template <bool SR>
SLAM_DEVICE uint4 round8(const float* f, const SrKey& k, uint64_t gi, uint32_t which) {
  if constexpr (SR) return sr_pack_bf16x8(f, k, gi, which);
  return pack_bf16x8(f);
}
template <bool SR, typename MT>
SLAM_DEVICE void store4_state(MT* q, const float* f, const SrKey& k, uint64_t gi, uint32_t which) {
  if constexpr (SR && sizeof(MT) == 2) *reinterpret_cast<uint2*>(q) = sr_pack_bf16x4(f, k, gi, which);
  else store4(q, f);
}
// one element of torch.optim.AdamW (fp32 master: b1 m + (1 - b1) g; bf16 state: torch's fused-kernel form with lerp)
template <bool MASTER>
SLAM_DEVICE void adam_elem(float& p, float& m, float& v, float g, const AdamHyper& h) {
  p *= (1.f - h.lr * h.wd);
  if (MASTER) m = h.b1 * m + (1.f - h.b1) * g;
  else m = m + (1.f - h.b1) * (g - m);
  v = h.b2 * v + (1.f - h.b2) * g * g;
  const float den = sqrtf(v) / h.bc2_sqrt + h.eps;
  p -= (h.lr / h.bc1) * (m / den);
}
// The same update for the stochastically rounded kernels, with every fp32 operation pinned: no contraction left to the compiler,
// the fused multiply-adds written out. Round-to-nearest hides a last-bit fp32 difference between two kernel forms (one contracts
// g * cs into the subtraction, the other does not) except at a tie; stochastic rounding turns it into another bf16 value once
// in 2^16 elements - and every form must store the same bits.
template <bool MASTER>
SLAM_DEVICE void adam_elem_pinned(float& p, float& m, float& v, float g_raw, float cs, const AdamHyper& h) {
#pragma clang fp contract(off)
  const float g = g_raw * cs;
  p = p * (1.f - h.lr * h.wd);
  if (MASTER) m = __builtin_fmaf(h.b1, m, (1.f - h.b1) * g);
  else m = __builtin_fmaf(1.f - h.b1, g - m, m);
  v = __builtin_fmaf(h.b2, v, ((1.f - h.b2) * g) * g);
  const float den = sqrtf(v) / h.bc2_sqrt + h.eps;
  p = __builtin_fmaf(-(h.lr / h.bc1), m / den, p);
}
template <bool MASTER, bool SR>
SLAM_DEVICE void adam_update(float& p, float& m, float& v, float g, float cs, const AdamHyper& h) {
  if constexpr (SR) adam_elem_pinned<MASTER>(p, m, v, g, cs, h);
  else adam_elem<MASTER>(p, m, v, g * cs, h);
}
// MASKED kernels: the hyper-parameters of the thread whose 4 or 8 consecutive elements start at flat index gi - wd = 0 when they
// lie in a range of the no-decay table, so that the element goes through the one expression of adam_elem (p * 1.0f is exact).
// The position in the table = the number of bounds <= gi; odd = inside a range. `first` is the flat index of the block's
// first element, the same for every thread: its binary search runs once per wave on scalar loads of uniform addresses (a table
// of a few hundred bounds: 8 or 9 dependent loads, issued behind the thread's own state loads so that the latencies overlap), and a
// thread walks on from there to its own group - no step at all in the blocks that no bound cuts, which is nearly all of them
// (Slam-358M: 146 bounds in 358 M elements; a block covers 1024 or 2048). The sentinel ends the walk. Measured cost
// (profiles/decay_rule.md): nothing with bf16 gradients, +1 % on the flat kernel with fp32 gradients.
// first / gi arrive relative to the arrays handed over (nd.base = the flat index of their element 0).
template <bool MASKED>
SLAM_DEVICE AdamHyper hyper_at(const AdamHyper& h, const NdArg<MASKED>& nd, uint64_t first, uint64_t gi) {
  if constexpr (MASKED) {
    first += nd.base; gi += nd.base;
    int lo = 0, hi = nd.n;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (nd.b[mid] <= first) lo = mid + 1;
      else hi = mid;
    }
    while (nd.b[lo] <= gi) ++lo;
    AdamHyper r = h;
    if (lo & 1) r.wd = 0.f;
    return r;
  } else {
    return h;
  }
}
// The Slam recipe's optimizer precision (/root/reference config/model/slam.yaml:9 torch_dtype bfloat16 -> bf16 parameters
// and bf16 Adam moments under torch.optim.AdamW(fused=True)): state is STORED in bf16, every update is computed in fp32
// from the stored values and rounded once on the way back (torch's fused kernel: opmath fp32, exp_avg by lerp).
// No fp32 master copy. Traffic: fp32 g read (4) + bf16 p, m, v read and written (12) = 16 B/param.
// SR ("adamw_sr"): p, m and v are rounded stochastically (sr_bf16), keyed on sr.base + i - the element's index in the flat buffer.
// MASKED: wd per thread from the no-decay table (nd.base + i = the flat index).
template <typename GT, bool SR, bool MASKED>
__global__ __launch_bounds__(256) void adamw_bf16_kernel(bf16_t* __restrict__ p, GT* __restrict__ g,
                                                         bf16_t* __restrict__ m, bf16_t* __restrict__ v, size_t n,
                                                         const float* __restrict__ clip, AdamHyper h0, NdArg<MASKED> nd) {
  size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 8;
  if (i >= n) return;
  const float cs = clip ? clip[1] : 1.f;
  float ga[8];
  load4<GT>(g + i, ga);
  load4<GT>(g + i + 4, ga + 4);
  float pa[8], ma[8], va[8];
  unpack_bf16x8(*reinterpret_cast<const uint4*>(p + i), pa);
  unpack_bf16x8(*reinterpret_cast<const uint4*>(m + i), ma);
  unpack_bf16x8(*reinterpret_cast<const uint4*>(v + i), va);
  const AdamHyper h = hyper_at<MASKED>(h0, nd, (uint64_t)blockIdx.x * 2048, i);
#pragma unroll
  for (int j = 0; j < 8; ++j) adam_update<false, SR>(pa[j], ma[j], va[j], ga[j], cs, h);
  *reinterpret_cast<uint4*>(p + i) = round8<SR>(pa, h.sr, h.sr.base + i, 0);
  *reinterpret_cast<uint4*>(m + i) = round8<SR>(ma, h.sr, h.sr.base + i, 1);
  *reinterpret_cast<uint4*>(v + i) = round8<SR>(va, h.sr, h.sr.base + i, 2);
  if constexpr (sizeof(GT) == 4) {
    if (h.zero_grad) {
      *reinterpret_cast<float4*>(g + i) = make_float4(0, 0, 0, 0);
      *reinterpret_cast<float4*>(g + i + 4) = make_float4(0, 0, 0, 0);
    }
  }
}

// ---- AdamW that also writes the TRANSPOSED bf16 weight image (round 3: replaces the separate transpose_bf16 pass after
// the optimizer: 4 B per matrix element of extra traffic and a kernel that ran at 2.4 TB/s). One block = one 64 x 64 tile
// of a [R][C] weight matrix (grid.z = same-shaped matrices at a constant stride: one per layer): every row segment of the
// tile is one contiguous 256 B (fp32) / 128 B (bf16) piece of each state array; the updated bf16 tile goes out row-major
// (pb) and, through a padded LDS tile, column-major (pt[C][R]). Per-element arithmetic is the flat kernels' own.
// MT = float / bf16_t: storage type of the Adam moments; MASTER: fp32 master weights (else the bf16 parameters ARE the state).
// SR (bf16 moments only): m and v are rounded stochastically, and so is p where it is the state (!MASTER; both images carry the
// one rounded value); the working copy of an fp32 master keeps round-to-nearest - the master holds the precision.
// 64 rows (c0 + 64 q ..) of the transposed image pt[C][R] from the finished LDS tile T[col][row]: two 16-byte stores a thread
template <int TC>
SLAM_DEVICE void store_tile_t(const uint16_t (&T)[TC][66], bf16_t* pt, size_t boff, int R, int r0, int c0, int q) {
  const int tid = threadIdx.x;
  const int orow = q * 64 + (tid >> 2), seg = (tid & 3) * 16;  // transposed row c0 + orow, its 16 elements r0 + seg ..
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&T[orow][seg]);
  uint4 a = make_uint4(src[0], src[1], src[2], src[3]), b = make_uint4(src[4], src[5], src[6], src[7]);
  bf16_t* dst = pt + boff + (size_t)(c0 + orow) * R + r0 + seg;
  *reinterpret_cast<uint4*>(dst) = a;
  *reinterpret_cast<uint4*>(dst + 8) = b;
}
template <typename MT, bool MASTER, int TC, typename GT, bool SR>  // tile = 64 rows x TC columns (TC = 64 or 128: 256 B or 512 B fp32 row segments)
__global__ __launch_bounds__(256) void adamw_tile_kernel(float* __restrict__ p, bf16_t* __restrict__ pb, bf16_t* __restrict__ pt,
                                                         GT* __restrict__ g, MT* __restrict__ m, MT* __restrict__ v, int R, int C,
                                                         size_t batch_stride, const float* __restrict__ clip, AdamHyper h) {
  constexpr int TPR = TC / 4, RPP = 256 / TPR, NP = 64 / RPP;  // threads per row, rows per pass, passes
  __shared__ uint16_t T[TC][66];  // transposed bf16 tile: T[col][row], rows padded to 132 B
  const size_t boff = (size_t)blockIdx.z * batch_stride;
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * TC;
  const int tid = threadIdx.x, rr = tid / TPR, cc = (tid % TPR) * 4;
  const float cs = clip ? clip[1] : 1.f;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int row = rr + RPP * i;
    const size_t idx = boff + (size_t)(r0 + row) * C + c0 + cc;
    float ga[4], pa[4], ma[4], va[4];
    load4<GT>(g + idx, ga);
    if (MASTER) load4<float>(p + idx, pa);
    else load4<bf16_t>(pb + idx, pa);
    load4<MT>(m + idx, ma);
    load4<MT>(v + idx, va);
#pragma unroll
    for (int j = 0; j < 4; ++j) adam_update<MASTER, SR>(pa[j], ma[j], va[j], ga[j], cs, h);
    if (MASTER) store4(p + idx, pa);
    store4_state<SR>(m + idx, ma, h.sr, h.sr.base + idx, 1);
    store4_state<SR>(v + idx, va, h.sr, h.sr.base + idx, 2);
    uint2 po;
    if constexpr (SR && !MASTER) {  // rounded once: the row-major store and the transposed image carry the same value
      po = sr_pack_bf16x4(pa, h.sr, h.sr.base + idx, 0);
      *reinterpret_cast<uint2*>(pb + idx) = po;
    } else {
      store4(pb + idx, pa);
    }
    if constexpr (sizeof(GT) == 4) {
      if (h.zero_grad) *reinterpret_cast<float4*>(g + idx) = make_float4(0, 0, 0, 0);
    }
    if constexpr (SR && !MASTER) {
      T[cc + 0][row] = (uint16_t)(po.x & 0xffffu); T[cc + 1][row] = (uint16_t)(po.x >> 16);
      T[cc + 2][row] = (uint16_t)(po.y & 0xffffu); T[cc + 3][row] = (uint16_t)(po.y >> 16);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) T[cc + j][row] = (uint16_t)(pack_bf16x2(pa[j], 0.f) & 0xffffu);
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < TC / 64; ++q) store_tile_t<TC>(T, pt, boff, R, r0, c0, q);
}
// The recipe's precision end to end (bf16 parameters, moments AND gradients: round 6) with 16-byte accesses: a thread owns 8
// consecutive columns (one dwordx4 per array and row instead of two dwordx2), 16 threads per 128-column row segment, 16 rows
// per pass. Per-element arithmetic = adam_elem<false>: the same bits as the kernel above. SR: one Philox call per array and
// 16-byte store (sr_pack_bf16x8).
template <bool SR>
__global__ __launch_bounds__(256) void adamw_tile_bf16x8_kernel(bf16_t* __restrict__ pb, bf16_t* __restrict__ pt, const bf16_t* __restrict__ g,
                                                                bf16_t* __restrict__ m, bf16_t* __restrict__ v, int R, int C,
                                                                size_t batch_stride, const float* __restrict__ clip, AdamHyper h) {
  constexpr int TC = 128, TPR = TC / 8, RPP = 256 / TPR, NP = 64 / RPP;
  __shared__ uint16_t T[TC][66];  // transposed bf16 tile: T[col][row], rows padded to 132 B
  const size_t boff = (size_t)blockIdx.z * batch_stride;
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * TC;
  const int tid = threadIdx.x, rr = tid / TPR, cc = (tid % TPR) * 8;
  const float cs = clip ? clip[1] : 1.f;
  uint4 gq[NP], pq[NP], mq[NP], vq[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) {  // every load of the tile in flight before the first use
    const size_t idx = boff + (size_t)(r0 + rr + RPP * i) * C + c0 + cc;
    gq[i] = *reinterpret_cast<const uint4*>(g + idx);
    pq[i] = *reinterpret_cast<const uint4*>(pb + idx);
    mq[i] = *reinterpret_cast<const uint4*>(m + idx);
    vq[i] = *reinterpret_cast<const uint4*>(v + idx);
  }
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int row = rr + RPP * i;
    const size_t idx = boff + (size_t)(r0 + row) * C + c0 + cc;
    float ga[8], pa[8], ma[8], va[8];
    unpack_bf16x8(gq[i], ga);
    unpack_bf16x8(pq[i], pa);
    unpack_bf16x8(mq[i], ma);
    unpack_bf16x8(vq[i], va);
#pragma unroll
    for (int j = 0; j < 8; ++j) adam_update<false, SR>(pa[j], ma[j], va[j], ga[j], cs, h);
    const uint4 po = round8<SR>(pa, h.sr, h.sr.base + idx, 0);
    *reinterpret_cast<uint4*>(pb + idx) = po;
    *reinterpret_cast<uint4*>(m + idx) = round8<SR>(ma, h.sr, h.sr.base + idx, 1);
    *reinterpret_cast<uint4*>(v + idx) = round8<SR>(va, h.sr, h.sr.base + idx, 2);
    const uint32_t w[4] = {po.x, po.y, po.z, po.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) T[cc + j][row] = (uint16_t)((j & 1) ? (w[j >> 1] >> 16) : (w[j >> 1] & 0xffffu));
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < TC / 64; ++q) store_tile_t<TC>(T, pt, boff, R, r0, c0, q);
}
// the vectors between the matrices (norm weights, biases): count elements at a constant stride, grid.y = instances
template <typename MT, bool MASTER, typename GT, bool SR, bool MASKED>
__global__ __launch_bounds__(256) void adamw_strided_kernel(float* __restrict__ p, bf16_t* __restrict__ pb, GT* __restrict__ g,
                                                            MT* __restrict__ m, MT* __restrict__ v, size_t n, size_t stride,
                                                            const float* __restrict__ clip, AdamHyper h0, NdArg<MASKED> nd) {
  const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
  const size_t idx = (size_t)blockIdx.y * stride + i;
  const float cs = clip ? clip[1] : 1.f;
  float ga[4], pa[4], ma[4], va[4];
  load4<GT>(g + idx, ga);
  if (MASTER) load4<float>(p + idx, pa);
  else load4<bf16_t>(pb + idx, pa);
  load4<MT>(m + idx, ma);
  load4<MT>(v + idx, va);
  const AdamHyper h = hyper_at<MASKED>(h0, nd, (uint64_t)blockIdx.y * stride + (uint64_t)blockIdx.x * 1024, idx);
#pragma unroll
  for (int j = 0; j < 4; ++j) adam_update<MASTER, SR>(pa[j], ma[j], va[j], ga[j], cs, h);
  if (MASTER) store4(p + idx, pa);
  store4_state<SR>(m + idx, ma, h.sr, h.sr.base + idx, 1);
  store4_state<SR>(v + idx, va, h.sr, h.sr.base + idx, 2);
  *reinterpret_cast<uint2*>(pb + idx) = round4<SR && !MASTER>(pa, h.sr, h.sr.base + idx, 0);
  if constexpr (sizeof(GT) == 4) {
    if (h.zero_grad) *reinterpret_cast<float4*>(g + idx) = make_float4(0, 0, 0, 0);
  }
}
// y[i] = sr_bf16(x[i]) with the bits of flat index index0 + i of array `which`: the rounding of the kernels above on its own
__global__ __launch_bounds__(256) void sr_round_bf16_kernel(const float* __restrict__ x, bf16_t* __restrict__ y, size_t n, SrKey k,
                                                            uint32_t which) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t gi = k.base + i;
  y[i] = (bf16_t)sr_bf16(x[i], sr_r16(sr_bits8(k, gi >> 3, which), (int)(gi & 7)));
}

__global__ __launch_bounds__(256) void f32_to_bf16_kernel(const float* __restrict__ s, bf16_t* __restrict__ d, size_t n) {
  size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
  float4 v = *reinterpret_cast<const float4*>(s + i);
  uint2 o;
  o.x = pack_bf16x2(v.x, v.y);
  o.y = pack_bf16x2(v.z, v.w);
  *reinterpret_cast<uint2*>(d + i) = o;
}

// the same conversion over blocks of GRAD_CHUNK elements, each emitting the sum of squares of the ROUNDED values it stored
// (GradSink slot = block index): the image of a gradient tensor that had to be built in fp32 (embedding scatter)
__global__ __launch_bounds__(256) void f32_to_bf16_sumsq_kernel(const float* __restrict__ s, bf16_t* __restrict__ d, size_t n,
                                                                float* __restrict__ sumsq) {
  __shared__ float red[4];
  const size_t lo = (size_t)blockIdx.x * GRAD_CHUNK;
  float ss = 0.f;
#pragma unroll
  for (int it = 0; it < GRAD_CHUNK / 1024; ++it) {
    const size_t i = lo + (size_t)(it * 256 + threadIdx.x) * 4;
    if (i < n) {
      const float4 v = *reinterpret_cast<const float4*>(s + i);
      const uint2 o = make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
      *reinterpret_cast<uint2*>(d + i) = o;
      ss += sq_bf16x2(o.x) + sq_bf16x2(o.y);
    }
  }
  block_sum_store<4>(ss, red, sumsq + blockIdx.x);
}

__global__ __launch_bounds__(256) void bf16_to_f32_kernel(const bf16_t* __restrict__ s, float* __restrict__ d, size_t n) {
  size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
  const uint2 v = *reinterpret_cast<const uint2*>(s + i);
  *reinterpret_cast<float4*>(d + i) = make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u),
                                                  __uint_as_float(v.y << 16), __uint_as_float(v.y & 0xffff0000u));
}

// dst[C][R] = src[R][C]^T, bf16, 64x64 tiles through LDS (R, C multiples of 64)
__global__ __launch_bounds__(256) void transpose_bf16_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst,
                                                             int R, int C, size_t batch_stride) {
  __shared__ uint32_t t[64][33];  // 64 rows x 64 bf16 (+1 dword pad)
  src += (size_t)blockIdx.z * batch_stride;  // same-shaped matrices at a constant stride (one per layer)
  dst += (size_t)blockIdx.z * batch_stride;
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int row = (tid >> 3) + 32 * i, ch = tid & 7;
    uint4 v = *reinterpret_cast<const uint4*>(src + (size_t)(r0 + row) * C + c0 + ch * 8);
    t[row][ch * 4 + 0] = v.x; t[row][ch * 4 + 1] = v.y; t[row][ch * 4 + 2] = v.z; t[row][ch * 4 + 3] = v.w;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int col = (tid >> 3) + 32 * i, rb = tid & 7;  // output row = col, 8 source rows rb*8..
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      uint32_t a = t[rb * 8 + 2 * k][col >> 1], b = t[rb * 8 + 2 * k + 1][col >> 1];
      uint32_t lo = (col & 1) ? (a >> 16) : (a & 0xffffu);
      uint32_t hi = (col & 1) ? (b >> 16) : (b & 0xffffu);
      w[k] = lo | (hi << 16);
    }
    *reinterpret_cast<uint4*>(dst + (size_t)(c0 + col) * R + r0 + rb * 8) = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

}  // namespace

namespace slam {

int grad_chunk_elems() { return GRAD_CHUNK; }
// chunk sums of the chunk-aligned range [off, off + cnt) (cnt may end at n instead of a chunk boundary); g_bf16: the
// gradients are bf16_t at g, not float
int grad_sumsq_chunks(const void* g, int g_bf16, size_t n, size_t off, size_t cnt, float* chunk_sums, hipStream_t st) {
  if ((n & 3) || (off % GRAD_CHUNK) || off + cnt > n || (((off + cnt) % GRAD_CHUNK) && off + cnt != n)) return -1;
  if (cnt == 0) return 0;
  const size_t nc = (cnt + GRAD_CHUNK - 1) / GRAD_CHUNK;
  const unsigned nb = (unsigned)((nc + CHUNKS_PER_BLOCK - 1) / CHUNKS_PER_BLOCK);
  if (g_bf16) sumsq_chunks_kernel<bf16_t><<<nb, 256, 0, st>>>((const bf16_t*)g, n, off / GRAD_CHUNK, nc, chunk_sums);
  else sumsq_chunks_kernel<float><<<nb, 256, 0, st>>>((const float*)g, n, off / GRAD_CHUNK, nc, chunk_sums);
  LAUNCH_RET();
}
int grad_norm_from_chunks(const float* chunk_sums, size_t n_chunks, float max_norm, float* out, hipStream_t st) {
  norm_finish_kernel<<<1, 1024, 0, st>>>(chunk_sums, (int)n_chunks, max_norm, out);
  LAUNCH_RET();
}
static SrKey sr_key(const AdamSR& sr, int step) {
  return {(uint32_t)(sr.seed & 0xffffffffu), (uint32_t)(sr.seed >> 32), (uint32_t)step, 0u, (uint64_t)sr.base};
}
int sr_round_bf16(const float* x, bf16_t* y, size_t n, int64_t index0, uint64_t seed, int step, int which, hipStream_t st) {
  if (n == 0) return 0;
  AdamSR sr;
  sr.on = 1; sr.seed = seed; sr.base = index0;
  sr_round_bf16_kernel<<<nblocks(n, 256), 256, 0, st>>>(x, y, n, sr_key(sr, step), (uint32_t)which);
  LAUNCH_RET();
}
template <bool MASKED> static NdArg<MASKED> nd_arg(const AdamArgs& a) {
  if constexpr (MASKED) return {a.nd.bounds, a.nd.n, (uint64_t)a.nd.base};
  else return {};
}
static AdamHyper adam_hyper(const AdamArgs& a) {
  // bias corrections in double like torch.optim.AdamW (python floats), then fp32 in the kernel
  AdamHyper h;
  h.lr = (float)a.lr; h.b1 = (float)a.b1; h.b2 = (float)a.b2; h.eps = (float)a.eps; h.wd = (float)a.wd;
  h.bc1 = (float)(1.0 - pow(a.b1, (double)a.step));
  h.bc2_sqrt = (float)sqrt(1.0 - pow(a.b2, (double)a.step));
  h.zero_grad = a.zero_grad;
  h.sr = sr_key(a.sr, a.step);
  return h;
}
// Kernel selection at compile time: a run-time choice becomes a std::integral_constant argument of a generic lambda
template <bool B> using Flag = std::integral_constant<bool, B>;
template <typename IsBf16> using Elem = std::conditional_t<IsBf16::value, bf16_t, float>;  // storage type behind an "is bf16" flag
template <typename F> static void with_flag(bool b, F&& f) { if (b) f(Flag<true>{}); else f(Flag<false>{}); }
// fn(m16, master, g16, sr): bf16 moments, fp32 master, bf16 gradients, stochastic rounding. fp32 moments (mode 0) come with a
// master and round nothing stochastically: exactly the combinations a mode allows are instantiated.
template <typename F> static void adam_dispatch(const AdamArgs& a, bool sr_on, F&& fn) {
  with_flag(a.g_bf16, [&](auto g16) {
    if (a.mode == 0) fn(Flag<false>{}, Flag<true>{}, g16, Flag<false>{});
    else with_flag(a.mode == 1, [&](auto master) { with_flag(sr_on, [&](auto sr) { fn(Flag<true>{}, master, g16, sr); }); });
  });
}
int adamw_tiles(const AdamArgs& a, int R, int C, int batch, size_t batch_stride, hipStream_t st) {
  if ((R & 63) || (C & 63) || batch < 1 || a.mode < 0 || a.mode > 2) return -1;
  const bool sr_on = a.sr.on && a.mode != 0;
  if (sr_on && ((a.sr.base & 7) || (batch > 1 && (batch_stride & 7)))) return -1;
  const AdamHyper h = adam_hyper(a);
  static int tile_cols = 128;  // SLAM_ADAMW_TILE_COLS=64: 256-byte row segments (A/B knob)
  static bool read_env = false;
  if (!read_env) { const char* e = getenv("SLAM_ADAMW_TILE_COLS"); if (e && atoi(e) == 64) tile_cols = 64; read_env = true; }
  static int x8 = -1;  // SLAM_ADAMW_X8=0: the 8-byte-access kernel for the all-bf16 case as well (A/B knob)
  if (x8 < 0) { const char* e = getenv("SLAM_ADAMW_X8"); x8 = !(e && e[0] == '0'); }
  auto launch = [&](auto tc) {  // 64 x tc tiles
    constexpr int TC = decltype(tc)::value;
    adam_dispatch(a, sr_on, [&](auto m16, auto master, auto g16, auto sr) {
      using MT = Elem<decltype(m16)>;
      using GT = Elem<decltype(g16)>;
      adamw_tile_kernel<MT, decltype(master)::value, TC, GT, decltype(sr)::value><<<dim3(C / TC, R / 64, batch), 256, 0, st>>>(
          a.master, a.params, a.params_t, (GT*)a.g, (MT*)a.m, (MT*)a.v, R, C, batch_stride, a.clip, h);
    });
  };
  const bool wide = tile_cols == 128 && C % 128 == 0;
  if (wide && a.mode == 2 && a.g_bf16 && x8) {
    with_flag(sr_on, [&](auto sr) {
      adamw_tile_bf16x8_kernel<decltype(sr)::value><<<dim3(C / 128, R / 64, batch), 256, 0, st>>>(
          a.params, a.params_t, (const bf16_t*)a.g, (bf16_t*)a.m, (bf16_t*)a.v, R, C, batch_stride, a.clip, h);
    });
  } else if (wide) {
    launch(std::integral_constant<int, 128>{});
  } else {
    launch(std::integral_constant<int, 64>{});
  }
  LAUNCH_RET();
}
int adamw_strided(const AdamArgs& a, size_t n, int batch, size_t stride, hipStream_t st) {
  if ((n & 3) || batch < 1 || a.mode < 0 || a.mode > 2) return -1;
  if (n == 0) return 0;
  const bool sr_on = a.sr.on && a.mode != 0;
  const bool masked = a.nd.bounds != nullptr;
  if ((sr_on && (a.sr.base & 3)) || (masked && (a.nd.base & 3)) || ((sr_on || masked) && batch > 1 && (stride & 3)))
    return -1;  // a thread's 4 elements share one group of 8
  const AdamHyper h = adam_hyper(a);
  adam_dispatch(a, sr_on, [&](auto m16, auto master, auto g16, auto sr) {
    with_flag(masked, [&](auto mk) {
      using MT = Elem<decltype(m16)>;
      using GT = Elem<decltype(g16)>;
      adamw_strided_kernel<MT, decltype(master)::value, GT, decltype(sr)::value, decltype(mk)::value>
          <<<dim3(nblocks(n / 4, 256), batch), 256, 0, st>>>(a.master, a.params, (GT*)a.g, (MT*)a.m, (MT*)a.v, n, stride, a.clip, h,
                                                             nd_arg<decltype(mk)::value>(a));
    });
  });
  LAUNCH_RET();
}
int adamw_flat(const AdamArgs& a, size_t n, hipStream_t st) {
  if (a.mode != 2) return adamw_strided(a, n, 1, 0, st);  // one instance of the strided kernel
  // bf16 parameters and bf16 moments updated in place, 8 elements (16 bytes per array) per thread
  const bool masked = a.nd.bounds != nullptr;
  if ((n & 7) || (a.sr.on && (a.sr.base & 7)) || (masked && (a.nd.base & 7))) return -1;
  const AdamHyper h = adam_hyper(a);
  with_flag(a.g_bf16, [&](auto g16) {
    with_flag(a.sr.on, [&](auto sr) {
      with_flag(masked, [&](auto mk) {
        using GT = Elem<decltype(g16)>;
        adamw_bf16_kernel<GT, decltype(sr)::value, decltype(mk)::value><<<nblocks(n / 8, 256), 256, 0, st>>>(
            a.params, (GT*)a.g, (bf16_t*)a.m, (bf16_t*)a.v, n, a.clip, h, nd_arg<decltype(mk)::value>(a));
      });
    });
  });
  LAUNCH_RET();
}
int transpose_bf16(const bf16_t* src, bf16_t* dst, int R, int C, int batch, size_t batch_stride, hipStream_t st) {
  if ((R & 63) || (C & 63) || batch < 1) return -1;
  transpose_bf16_kernel<<<dim3(C / 64, R / 64, batch), 256, 0, st>>>(src, dst, R, C, batch_stride);
  LAUNCH_RET();
}
int bf16_to_f32(const bf16_t* s, float* d, size_t n, hipStream_t st) {
  if (n & 3) return -1;
  bf16_to_f32_kernel<<<nblocks(n / 4, 256), 256, 0, st>>>(s, d, n);
  LAUNCH_RET();
}
int f32_to_bf16_sumsq_slots(size_t n) { return (int)((n + GRAD_CHUNK - 1) / GRAD_CHUNK); }
int f32_to_bf16_sumsq(const float* s, bf16_t* d, size_t n, float* sumsq, hipStream_t st) {
  if (n & 3) return -1;
  f32_to_bf16_sumsq_kernel<<<(unsigned)f32_to_bf16_sumsq_slots(n), 256, 0, st>>>(s, d, n, sumsq);
  LAUNCH_RET();
}
int f32_to_bf16(const float* s, bf16_t* d, size_t n, hipStream_t st) {
  if (n & 3) return -1;
  f32_to_bf16_kernel<<<nblocks(n / 4, 256), 256, 0, st>>>(s, d, n);
  LAUNCH_RET();
}

}  // namespace slam
