// Shared-prompt decode (slam_kv_share, include/slam_engine.h): the n rows sampled from one prompt attend ONE copy of the prompt's
// keys. A decode step's attention is three launches over one partials buffer in the decode layout [(row, head)][split][hd + 2]:
//  * attn_prefix_kernel (new, matrix pipe): the n G queries that meet the keys of (prompt b, KV head g) are a small GEMM, not n
//    GEMVs. One block = one key split x one group of 64 QT queries of one (prompt, KV head); it reads the prompt store
//    [prompts][nKV][pcap][hd] once per split whatever n is. Query u of the group's list is (row b n + u / G, head g G + u % G);
//    wave w owns the 16-query tiles w and (QT = 2) w + 4 of the block. Each lane builds its B-operand fragment - dims
//    32 kk + 8 qd .. + 7 of query j = lane & 15, qd = lane >> 4 - from the fp32 projection row with rope8 and one rounding to
//    bf16: the bits attn_decode_kernel's qf holds for the same (row, head), so both parts score with the same queries. The four
//    waves stage each 32-key block once (K row-major, V transposed, attn_extend_kernel's strides, the next block's loads in
//    flight under the products). S^T = K Q^T on v_mfma_f32_16x16x32_bf16 leaves P^T in the B-operand map of the PV product:
//    lane (qd, j) holds query j's keys 4 qd + r and 16 + 4 qd + r of the block, and O^T comes out as
//    o[query j][16 dt + 4 qd + r]. No causal mask inside a prompt: key k counts iff k < min(plens[b], pbound). Keys at or
//    beyond that are staged as zeros and scored -inf, tail queries (u >= n G) read query n G - 1 and store nothing, so neither
//    the store's bits behind a prompt nor a tail lane reaches the output. A split without keys writes (0, -inf, 0).
//  * attn_decode_kernel<.., SH = true> (decode_attn.h): the existing per-key kernel over the keys BEHIND the prompt in the
//    ordinary cache, index shifted by the prompt length; appends the new token; its partials follow the prefix splits.
//  * attn_decode_combine_kernel, unchanged, over ns_prefix + ns_suffix partials in split order: no atomics, same bits each run.
// Scoring in the mode (slam_extend_score / slam_extend_logits): attn_extend_shared_kernel below, chunk attention whose keys come
// from both places in ONE launch with no partials - the extend path's partials do not fit the logits buffer at a 502-row vocabulary.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>

#include "common.h"
#include "decode_attn.h"
#include "kernels.h"

namespace {

inline unsigned nblk(size_t n, int per) { return (unsigned)((n + per - 1) / per); }

// grid (ns_prefix, query groups, prompts * nKV), 256 threads
template <int HD, int QT>
__global__ __launch_bounds__(256) void attn_prefix_kernel(const float* __restrict__ qkv, const bf16_t* __restrict__ bias,
                                                          const float* __restrict__ csq, const float* __restrict__ snq,
                                                          const int* __restrict__ plens, const bf16_t* __restrict__ pk,
                                                          const bf16_t* __restrict__ pv, int pcap, int pbound, int n, int G, int nH,
                                                          int nKV, int chunk, int ns_tot, float* __restrict__ part) {
  constexpr int KS = HD + 8;     // K row stride (bf16): 16-byte rows, fragment reads spread over the banks
  constexpr int VS = AE_KB + 4;  // V^T row stride (bf16): 8-byte rows, 18 dwords apart
  constexpr int DT = HD / 16, KK = HD / 32, half = HD / 2;
  __shared__ __attribute__((aligned(16))) bf16_t Ks[AE_KB * KS];
  __shared__ __attribute__((aligned(16))) bf16_t Vt[HD * VS];
  const int s = blockIdx.x;
  const int b = blockIdx.z / nKV, g = blockIdx.z % nKV;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qd = lane >> 4, j = lane & 15;
  const int NQ = n * G;
  const int QKV = (nH + 2 * nKV) * HD;
  const int plen = min(max(plens[b], 0), pbound);
  const int k_lo = s * chunk;
  const int k_hi = min(k_lo + chunk, plen);

  uint4 qf[QT][KK];
  f32x4_t acc[QT][DT];
  float m_[QT], l_[QT];
  int u_[QT];
#pragma unroll
  for (int hh = 0; hh < QT; ++hh) {
    m_[hh] = -INFINITY;
    l_[hh] = 0.f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[hh][dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    u_[hh] = ((blockIdx.y * QT + hh) * 4 + wave) * 16 + j;
    const int uc = min(u_[hh], NQ - 1);  // tail queries repeat the last one; they are never stored
    const int r = b * n + uc / G, hq = g * G + uc % G;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      float f[8];
      rope8<HD>(qkv + (size_t)r * QKV, bias, hq * HD, 32 * kk + 8 * qd, csq + (size_t)r * half, snq + (size_t)r * half, f);
      qf[hh][kk] = pack_bf16x8(f);  // the one rounding: round8's bits, packed
    }
  }
  const size_t cbase = ((size_t)b * nKV + g) * pcap;
  constexpr int NV = AE_KB * (HD / 8) / 256;  // 16-byte pieces of a K (and of a V) block per thread
  uint4 kx[NV], vx[NV];
  // the block's K / V pieces of this thread into registers; keys at or beyond k_hi as zeros, never the store's bits
  auto fetch = [&](int kb) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int t = threadIdx.x + 256 * v;
      const int kr = t / (HD / 8), d0 = (t % (HD / 8)) * 8;
      const bool ok = kb + kr < k_hi;
      const size_t src = (cbase + (ok ? kb + kr : 0)) * HD + d0;
      kx[v] = ok ? *reinterpret_cast<const uint4*>(pk + src) : uint4{0u, 0u, 0u, 0u};
      vx[v] = ok ? *reinterpret_cast<const uint4*>(pv + src) : uint4{0u, 0u, 0u, 0u};
    }
  };
  if (k_lo < k_hi) fetch(k_lo);
  for (int kb = k_lo; kb < k_hi; kb += AE_KB) {
    __syncthreads();  // the previous block's fragment reads are done
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int t = threadIdx.x + 256 * v;
      const int kr = t / (HD / 8), d0 = (t % (HD / 8)) * 8;
      *reinterpret_cast<uint4*>(&Ks[kr * KS + d0]) = kx[v];
      const uint32_t w[4] = {vx[v].x, vx[v].y, vx[v].z, vx[v].w};
#pragma unroll
      for (int e = 0; e < 8; ++e) Vt[(d0 + e) * VS + kr] = (bf16_t)(w[e >> 1] >> (16 * (e & 1)));
    }
    if (kb + AE_KB < k_hi) fetch(kb + AE_KB);  // the next block's loads fly under this block's products
    __syncthreads();
#pragma unroll
    for (int hh = 0; hh < QT; ++hh) {
      if (u_[hh] - j >= NQ) continue;  // wave-uniform: a tile with no real query
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
          const float x = kb + 16 * c + 4 * qd + r < k_hi ? sc[c][r] : -INFINITY;
          sc[c][r] = x;
          mx = fmaxf(mx, x);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mn = fmaxf(m_[hh], mx);
      const float ms = mn == -INFINITY ? 0.f : mn;
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
  for (int hh = 0; hh < QT; ++hh) {
    float l = l_[hh];
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const int u = u_[hh];
    if (u >= NQ) continue;
    const int r = b * n + u / G, hq = g * G + u % G;
    float* dst = part + (((size_t)r * nH + hq) * ns_tot + s) * (HD + 2);  // 8-byte aligned: (HD + 2) floats per partial
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      *reinterpret_cast<float2*>(dst + 16 * dt + 4 * qd) = make_float2(acc[hh][dt][0], acc[hh][dt][1]);
      *reinterpret_cast<float2*>(dst + 16 * dt + 4 * qd + 2) = make_float2(acc[hh][dt][2], acc[hh][dt][3]);
    }
    if (qd == 0) { dst[HD] = m_[hh]; dst[HD + 1] = l; }
  }
}

// ---- chunk attention over two regions (slam_extend_score / slam_extend_logits in the shared mode) ------------------------------
// A 32-key block of one K / V source into the registers of the NT threads that stage it (NP 16-byte pieces each, thread tid owns
// dims d0 .. d0 + 7 of key kr), keys at or beyond k_hi as zeros; and from there into one stage set, attn_extend_kernel's layout.
template <int HD, int NP, int NT>
SLAM_DEVICE void aes_fetch(const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, size_t cbase, int tid, int kb, int k_hi,
                           uint4* kx, uint4* vx) {
  static_assert(NP * NT == AE_KB * (HD / 8), "the pieces cover one block");
#pragma unroll
  for (int u = 0; u < NP; ++u) {
    const int t = tid + NT * u;
    const int kr = t / (HD / 8), d0 = (t % (HD / 8)) * 8;
    const bool ok = kb + kr < k_hi;
    const size_t src = (cbase + (ok ? kb + kr : 0)) * HD + d0;
    kx[u] = ok ? *reinterpret_cast<const uint4*>(k + src) : uint4{0u, 0u, 0u, 0u};
    vx[u] = ok ? *reinterpret_cast<const uint4*>(v + src) : uint4{0u, 0u, 0u, 0u};
  }
}
template <int HD, int NP, int NT>
SLAM_DEVICE void aes_stage(bf16_t* Ks, bf16_t* Vt, int tid, const uint4* kx, const uint4* vx) {
  constexpr int KS = HD + 8, VS = AE_KB + 4;
#pragma unroll
  for (int u = 0; u < NP; ++u) {
    const int t = tid + NT * u;
    const int kr = t / (HD / 8), d0 = (t % (HD / 8)) * 8;
    *reinterpret_cast<uint4*>(&Ks[kr * KS + d0]) = kx[u];
    const uint32_t w[4] = {vx[u].x, vx[u].y, vx[u].z, vx[u].w};
#pragma unroll
    for (int e = 0; e < 8; ++e) Vt[(d0 + e) * VS + kr] = (bf16_t)(w[e >> 1] >> (16 * (e & 1)));
  }
}

// grid (ceil(T / 16), ceil(n / RB), prompts * nKV), 256 threads: one 16-token tile of the chunk x RB consecutive rows of one prompt
// x one KV head, one launch per layer, no partials: (m, l, o) stay in registers across both key regions. The four waves are
// divided over (row of the block, subset of the group's heads): WPR = 4 / RB waves per row, wave w serves row w / WPR and the
// heads i = w % WPR (mod WPR) of the group. Fragments, score and PV products are attn_extend_kernel's (its comment has the maps).
//  phase 1, the prompt's keys 0 .. min(plens[b], pbound) - 1 from the store: all four waves stage each 32-key block ONCE into
//    stage set 0 and every wave multiplies it with its own row's queries, so one staging serves RB x 16 x G queries. No causal
//    mask: every chunk query sits behind every prompt key.
//  phase 2, the row's own keys 0 .. base_s + t of the ordinary cache (base_s = lens[r] - plens[b], the chunk's tokens already
//    scattered there): K / V differ per row, so row rr of the block has stage set rr, filled by the WPR waves that serve it.
//    attn_extend_kernel's mask: key ka counts iff ka <= base_s + t. The loop runs to the block's maximum over its rows so that
//    every wave meets every barrier; a row that has run out of keys stages zeros and masks them.
// A row index beyond the prompt's n rows repeats row n - 1 and stores nothing; a row without a real query in the tile multiplies
// nothing and stores zeros. Every count is clamped to its host bound before an address is formed: prompt keys < pbound <= pcap,
// suffix keys < sbound <= cap, tokens < T.
template <int HD, int G, int RB>
__global__ __launch_bounds__(256) void attn_extend_shared_kernel(const bf16_t* __restrict__ qkv, const int* __restrict__ lens,
                                                                 const int* __restrict__ new_lens, const int* __restrict__ plens,
                                                                 int n, const bf16_t* __restrict__ pk, const bf16_t* __restrict__ pv,
                                                                 int pcap, int pbound, const bf16_t* __restrict__ kc,
                                                                 const bf16_t* __restrict__ vc, int cap, int sbound,
                                                                 bf16_t* __restrict__ o, int T, int nH, int nKV) {
  constexpr int WPR = 4 / RB;                // waves per row
  constexpr int NHW = (G + WPR - 1) / WPR;   // heads per wave
  constexpr int KS = HD + 8, VS = AE_KB + 4;  // attn_extend_kernel's strides
  constexpr int DT = HD / 16, KK = HD / 32;
  constexpr int SET = AE_KB * KS + HD * VS;  // one stage set: K row-major, then V transposed (a multiple of 16 bytes)
  constexpr int NP1 = AE_KB * (HD / 8) / 256, NP2 = NP1 * RB;  // pieces per thread: 256 threads a block, 64 WPR threads a block
  __shared__ __attribute__((aligned(16))) bf16_t stage[RB * SET];
  const int q0 = blockIdx.x * 16;
  const int b = blockIdx.z / nKV, g = blockIdx.z % nKV;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qd = lane >> 4, j = lane & 15;
  const int rr = wave / WPR, hw = wave % WPR;
  const int QKV = (nH + 2 * nKV) * HD;
  const int plen_raw = max(plens[b], 0);      // the shift of the suffix index, as the scatter's shifted bases took it
  const int plen = min(plen_raw, pbound);     // the keys read from the store
  // every row of the block: what the loop bounds need; this wave's own row: the rest
  int r = 0, base_s = 0, nl = 0, tile_n = 0, kmax = 0;
  bool any = false;
#pragma unroll
  for (int x = 0; x < RB; ++x) {
    const int rx = b * n + min((int)blockIdx.y * RB + x, n - 1);
    const int bx = min(max(lens[rx] - plen_raw, 0), sbound);
    const int nx = min(max(new_lens[rx], 0), min(T, sbound - bx));
    const int tx = min(q0 + 16, nx) - q0;  // real queries of the row's tile (<= 0: none)
    if (tx > 0) { any = true; kmax = max(kmax, bx + q0 + tx); }
    if (x == rr) { r = rx; base_s = bx; nl = nx; tile_n = tx; }
  }
  const bool stores = (int)blockIdx.y * RB + rr < n;
  const bool active = tile_n > 0;  // wave-uniform
  const int tq = q0 + j;           // this lane's query (token of the chunk)
  const bool real = tq < nl;
  const int kend = active ? base_s + q0 + tile_n : 0;  // suffix keys the tile's last real query sees
  const int qlim = base_s + min(tq, nl - 1);           // last suffix key of this lane's query (clamped for the rows not real)

  uint4 qf[NHW][KK];
  f32x4_t acc[NHW][DT];
  float m_[NHW], l_[NHW];
#pragma unroll
  for (int hh = 0; hh < NHW; ++hh) {
    const int i = hw + WPR * hh;
    m_[hh] = -INFINITY;
    l_[hh] = 0.f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[hh][dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const int tr = max(min(tq, nl - 1), 0);
    const bf16_t* qrow = qkv + ((size_t)r * T + tr) * QKV + (size_t)(g * G + min(i, G - 1)) * HD + 8 * qd;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) qf[hh][kk] = *reinterpret_cast<const uint4*>(qrow + 32 * kk);
  }
  // one staged block against this wave's queries: key kb + .. counts iff it is below k_hi and at or below klim
  auto products = [&](const bf16_t* Ks, const bf16_t* Vt, int kb, int k_hi, int klim) {
#pragma unroll
    for (int hh = 0; hh < NHW; ++hh) {
      if (hw + WPR * hh >= G) continue;  // wave-uniform
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
        for (int e = 0; e < 4; ++e) {
          const int ka = kb + 16 * c + 4 * qd + e;
          const float x = (ka < k_hi && ka <= klim) ? sc[c][e] : -INFINITY;
          sc[c][e] = x;
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
        for (int e = 0; e < 4; ++e) {
          p[4 * c + e] = fast_exp2(sc[c][e] - ms);
          ps += p[4 * c + e];
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
  };
  uint4 kx[NP2], vx[NP2];

  // phase 1: the prompt's keys, one staging for the whole block
  const int p_hi = any ? plen : 0;
  const size_t pbase = ((size_t)b * nKV + g) * pcap;
  if (p_hi > 0) aes_fetch<HD, NP1, 256>(pk, pv, pbase, threadIdx.x, 0, p_hi, kx, vx);
  for (int kb = 0; kb < p_hi; kb += AE_KB) {
    __syncthreads();  // the previous block's fragment reads are done
    aes_stage<HD, NP1, 256>(stage, stage + AE_KB * KS, threadIdx.x, kx, vx);
    if (kb + AE_KB < p_hi) aes_fetch<HD, NP1, 256>(pk, pv, pbase, threadIdx.x, kb + AE_KB, p_hi, kx, vx);  // in flight under the products
    __syncthreads();
    if (active) products(stage, stage + AE_KB * KS, kb, p_hi, 0x7fffffff);
  }

  // phase 2: the row's own keys, a stage set per row of the block
  const size_t sbase = ((size_t)r * nKV + g) * cap;
  const int tid2 = threadIdx.x % (64 * WPR);
  bf16_t* Ks2 = stage + rr * SET;
  bf16_t* Vt2 = Ks2 + AE_KB * KS;
  if (kmax > 0) aes_fetch<HD, NP2, 64 * WPR>(kc, vc, sbase, tid2, 0, kend, kx, vx);
  for (int kb = 0; kb < kmax; kb += AE_KB) {
    __syncthreads();  // phase 1's last reads, then the previous block's
    aes_stage<HD, NP2, 64 * WPR>(Ks2, Vt2, tid2, kx, vx);
    if (kb + AE_KB < kmax) aes_fetch<HD, NP2, 64 * WPR>(kc, vc, sbase, tid2, kb + AE_KB, kend, kx, vx);
    __syncthreads();
    if (kb < kend) products(Ks2, Vt2, kb, kend, qlim);  // wave-uniform
  }

#pragma unroll
  for (int hh = 0; hh < NHW; ++hh) {
    const int i = hw + WPR * hh;
    if (i >= G) continue;
    float l = l_[hh];
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (!stores || tq >= T) continue;
    const float inv = real ? 1.f / l : 0.f;
    bf16_t* dst = o + (((size_t)r * T + tq) * nH + g * G + i) * HD;
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

// bases[r] = max(lens[r] - plens[r / n], 0): where row r's next key goes in the ordinary cache
__global__ void shifted_bases_kernel(const int* __restrict__ lens, const int* __restrict__ plens, int n, int* __restrict__ bases,
                                     int R) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < R) bases[r] = max(lens[r] - max(plens[r / n], 0), 0);
}

// slam_kv_share: lens[b] and the logits row b -> rows b n .. b n + n - 1, never onto row b itself. One launch per source row in
// descending b, kv_repeat's scheme and argument (decode.hip's header): no launch writes what it or a later launch reads.
__global__ __launch_bounds__(256) void kv_share_fan_kernel(int* __restrict__ lens, float* __restrict__ logits, int b, int n,
                                                           int vocab) {
  const int len = lens[b];  // not a destination of this launch
  const int i0 = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
  for (int i = i0; i < n; i += step)
    if (b * n + i != b) lens[b * n + i] = len;
  if (!logits) return;
  const float* src = logits + (size_t)b * vocab;
  for (int c = i0; c < vocab; c += step) {
    const float v = src[c];
    for (int i = 0; i < n; ++i)
      if (b * n + i != b) logits[(size_t)(b * n + i) * vocab + c] = v;
  }
}

__global__ void lens_copy_kernel(const int* __restrict__ src, int* __restrict__ dst, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) dst[b] = src[b];
}

}  // namespace

namespace slam {

// Prefix: QT = 2 (128 queries per block) once n G passes 64, so a group up to 128 queries still stages each key block once; key
// splits are multiples of 32 keys, 128 at the least, aiming at about 512 blocks over (splits, KV heads, prompts, query groups).
// Suffix: attn_decode_chunk's rule over the B n rows. While the partials of both parts exceed part_bytes, the part with more
// splits doubles its keys per split; -3 when one split each does not fit.
int attn_shared_plan(int P, int n, int nH, int nKV, int head_dim, int pbound, int sbound, size_t part_bytes, SharedPlan* p) {
  if (P <= 0 || n <= 0 || nKV <= 0 || nH % nKV || pbound <= 0 || sbound <= 0 || (int64_t)P * n > 0x7fffffff / 64) return -1;
  const int G = nH / nKV, NQ = n * G, R = P * n;
  if ((head_dim != 64 && head_dim != 128) || G > 8) return -1;
  p->qt = NQ > 64 ? 2 : 1;
  p->qgroups = (NQ + 64 * p->qt - 1) / (64 * p->qt);
  const int64_t per_split = (int64_t)P * nKV * p->qgroups;
  const int target = 512 / per_split > 1 ? (int)(512 / per_split) : 1;
  p->pchunk = ((pbound + target - 1) / target + 31) / 32 * 32;
  if (p->pchunk < 128) p->pchunk = 128;
  p->schunk = attn_decode_chunk(R, nH, nKV, head_dim, sbound, (size_t)-1);
  for (;;) {
    p->nsp = (pbound + p->pchunk - 1) / p->pchunk;
    p->nss = (sbound + p->schunk - 1) / p->schunk;
    if (attn_decode_part_bytes(R, nH, head_dim, p->nsp + p->nss) <= part_bytes) return 0;
    if (p->nsp == 1 && p->nss == 1) return -3;
    if (p->nsp >= p->nss) p->pchunk *= 2;
    else p->schunk *= 2;
  }
}

int attn_decode_shared(const float* qkv, const bf16_t* bias, const float* cs, const float* sn, const float* csq, const float* snq,
                       const int* lens, const int* plens, int n, const bf16_t* pk, const bf16_t* pv, int pcap, int pbound, bf16_t* kc,
                       bf16_t* vc, int cap, int sbound, int P, int nH, int nKV, int head_dim, bf16_t* o, float* part,
                       size_t part_bytes, hipStream_t st) {
  if (!qkv || !lens || !plens || !pk || !pv || !kc || !vc || !o || !part) return -1;
  if (pbound > pcap || sbound > cap) return -1;
  if (((uintptr_t)pk | (uintptr_t)pv | (uintptr_t)kc | (uintptr_t)vc | (uintptr_t)part) & 15) return -1;
  SharedPlan p;
  if (int r = attn_shared_plan(P, n, nH, nKV, head_dim, pbound, sbound, part_bytes, &p)) return r;
  const int G = nH / nKV, R = P * n, ns = p.nsp + p.nss;
  if ((int64_t)P * nKV > 65535 || p.qgroups > 65535 || R > 65535) return -1;
  const dim3 pgrid(p.nsp, p.qgroups, P * nKV);
#define AP_LAUNCH(HD, QT)                                                                                                        \
  attn_prefix_kernel<HD, QT><<<pgrid, 256, 0, st>>>(qkv, bias, csq, snq, plens, pk, pv, pcap, pbound, n, G, nH, nKV, p.pchunk, ns, part)
  if (head_dim == 64) {
    if (p.qt == 2) AP_LAUNCH(64, 2);
    else AP_LAUNCH(64, 1);
  } else {
    if (p.qt == 2) AP_LAUNCH(128, 2);
    else AP_LAUNCH(128, 1);
  }
#undef AP_LAUNCH
  const dim3 sgrid(p.nss, nKV, R);
  const DecodeShare sh = {plens, n, p.nsp, ns};
#define AS_CASE(HD, GG)                                                                                                        \
  case GG:                                                                                                                     \
    attn_decode_kernel<HD, GG, false, true><<<sgrid, 256, 0, st>>>(qkv, bias, cs, sn, csq, snq, lens, kc, vc, nullptr, nullptr, cap, \
                                                                   nH, nKV, p.schunk, p.nss, part, sh);                        \
    break;
#define AS_SWITCH(HD) \
  switch (G) { AS_CASE(HD, 1) AS_CASE(HD, 2) AS_CASE(HD, 3) AS_CASE(HD, 4) AS_CASE(HD, 5) AS_CASE(HD, 6) AS_CASE(HD, 7) AS_CASE(HD, 8) }
  if (head_dim == 64) {
    AS_SWITCH(64)
    attn_decode_combine_kernel<64><<<dim3(nH, R), 64, 0, st>>>(part, ns, nH, o);
  } else {
    AS_SWITCH(128)
    attn_decode_combine_kernel<128><<<dim3(nH, R), 128, 0, st>>>(part, ns, nH, o);
  }
#undef AS_SWITCH
#undef AS_CASE
  return (int)hipGetLastError();
}

int shifted_bases(const int* lens, const int* plens, int n, int* bases, int R, hipStream_t st) {
  if (!lens || !plens || !bases || n < 1 || R <= 0) return -1;
  shifted_bases_kernel<<<nblk((size_t)R, 256), 256, 0, st>>>(lens, plens, n, bases, R);
  return (int)hipGetLastError();
}

// Rows of a prompt per block, one mapping per head_dim: one row with four head quarters at both (attn_extend_kernel's mapping
// plus the phase switch). The two-row form (RB = 2: two head halves per row, one staging of the prompt for both rows) holds
// scratch at head_dim 128, G = 8, and measured slower at head_dim 64 (Slam-358M, 128 rows x 2048 + 150 keys: 167.5 us a launch
// against 144.3 us; it runs at one wave per SIMD from G = 7). profiles/shared_score.md has both sets of numbers.
constexpr int AES_RB_64 = 1, AES_RB_128 = 1;

int attn_extend_shared(const bf16_t* qkv, const int* lens, const int* new_lens, const int* bases, const int* plens, int n,
                       const bf16_t* pk, const bf16_t* pv, int pcap, int pbound, bf16_t* kc, bf16_t* vc, int cap, int sbound, int P,
                       int T, int nH, int nKV, int head_dim, bf16_t* o, hipStream_t st) {
  if (!qkv || !lens || !new_lens || !bases || !plens || !pk || !pv || !kc || !vc || !o) return -1;
  if (P <= 0 || n <= 0 || T <= 0 || nKV <= 0 || nH % nKV || pbound <= 0 || sbound <= 0 || pbound > pcap || sbound > cap) return -1;
  const int G = nH / nKV;
  if ((head_dim != 64 && head_dim != 128) || G > 8) return -1;
  const int64_t R = (int64_t)P * n;
  if ((int64_t)P * nKV > 65535 || R > 65535 || T > 65535 || R * T > 0x7fffffffLL / (nH * (head_dim + 4))) return -1;
  if (((uintptr_t)qkv | (uintptr_t)pk | (uintptr_t)pv | (uintptr_t)kc | (uintptr_t)vc | (uintptr_t)o) & 15) return -1;
  // the chunk's K / V behind each row's own keys: the unshared scatter launch over the shifted bases
  if (int r = kv_extend_scatter(qkv, kc, vc, bases, new_lens, (int)R, T, nH, nKV, head_dim, cap, sbound, st)) return r;
#define AES_CASE(HD, GG, RB)                                                                                                     \
  case GG:                                                                                                                       \
    attn_extend_shared_kernel<HD, GG, RB><<<dim3((T + 15) / 16, (n + RB - 1) / RB, P * nKV), 256, 0, st>>>(                      \
        qkv, lens, new_lens, plens, n, pk, pv, pcap, pbound, kc, vc, cap, sbound, o, T, nH, nKV);                                \
    break;
#define AES_SWITCH(HD, RB)                                                                                                       \
  switch (G) {                                                                                                                   \
    AES_CASE(HD, 1, RB) AES_CASE(HD, 2, RB) AES_CASE(HD, 3, RB) AES_CASE(HD, 4, RB) AES_CASE(HD, 5, RB) AES_CASE(HD, 6, RB)      \
    AES_CASE(HD, 7, RB) AES_CASE(HD, 8, RB)                                                                                      \
  }
  if (head_dim == 64) { AES_SWITCH(64, AES_RB_64) }
  else { AES_SWITCH(128, AES_RB_128) }
#undef AES_SWITCH
#undef AES_CASE
  return (int)hipGetLastError();
}

int kv_share_fan(int* lens, float* logits, int B, int n, int vocab, hipStream_t st) {
  if (!lens || B <= 0 || n < 1) return -1;
  if (n == 1) return 0;
  unsigned gx = nblk(logits ? (size_t)vocab : (size_t)n, 256);
  if (gx > 64) gx = 64;
  for (int b = B - 1; b >= 0; --b)  // descending: see the kernel
    kv_share_fan_kernel<<<gx, 256, 0, st>>>(lens, logits, b, n, vocab);
  return (int)hipGetLastError();
}

int lens_copy(const int* src, int* dst, int B, hipStream_t st) {
  lens_copy_kernel<<<nblk((size_t)B, 256), 256, 0, st>>>(src, dst, B);
  return (int)hipGetLastError();
}

}  // namespace slam
