// The two attention kernels of cached generation and their launchers, as templates over the cache's element: F8 = false reads
// and appends bf16 keys and values (decode.hip instantiates it), F8 = true reads and appends e4m3 codes with one int8
// power-of-two exponent per key / value vector (decode_kv8.hip; the format is stated in include/slam_engine.h). The two differ
// only in how a key's eight dims per lane get into fp32 registers (decode) or a key block into LDS (extend), and in what the
// appended token leaves in the cache; grid, lane mapping, softmax order and merges are one text. `if constexpr` only: an
// instantiation holds no trace of the other.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>

#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace {

template <bool F8>
using kv_elem_t = std::conditional_t<F8, uint8_t, bf16_t>;

// max over the LG lanes that own one vector (LG a power of two, the lanes consecutive and aligned)
template <int LG>
SLAM_DEVICE int group_max_i(int v) {
#pragma unroll
  for (int o = 1; o < LG; o <<= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// A lane's eight bf16 dims of a vector whose LG lanes are all here -> its eight codes and the vector's exponent
template <int LG>
SLAM_DEVICE uint2 kv8_quantize(const uint4& v, int* e) {
  *e = fp8_exponent(group_max_i<LG>(bf16x8_amax_bits(v)));
  return fp8_encode8(v, pow2i(-*e));
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
// F8: kc / vc hold codes ([B][nKV][cap][HD] bytes), ke / ve one exponent per key ([B][nKV][cap]). A lane loads its 8 code bytes,
// the slot's first lane loads the key's two exponents and the slot reads them by shuffle; code -> fp32 -> times 2^e is the value
// a bf16 cache of the dequantised keys would have handed the same lane, and everything behind it is the same text. The new
// token is rounded to bf16 as ever, quantised in registers (its LG lanes are all here: they share j), stored as codes +
// exponent and scored as dequantised: round once, then use what the cache holds.
// SH (shared-prompt decode, decode_shared.hip; bf16 only): row b belongs to prompt b / sh.n, whose sh.plens[b / sh.n] keys live
// in the prompt store and are served by attn_prefix_kernel. This cache then holds only the keys behind the prompt: key k of the
// row sits at index k - plen, the new token at lens[b] - plen, and the partials go behind the prefix splits of the row
// (split sh.ns_off + s of sh.ns_tot). Tables, queries, lanes and merges are the same text; SH = false holds no trace of it.
struct DecodeNoShare {};
struct DecodeShare {
  const int* plens;  // [prompts]
  int n, ns_off, ns_tot;
};
template <int HD, int G, bool F8, bool SH = false>
__global__ __launch_bounds__(256) void attn_decode_kernel(const float* __restrict__ qkv, const bf16_t* __restrict__ bias,
                                                          const float* __restrict__ cs, const float* __restrict__ sn,
                                                          const float* __restrict__ csq, const float* __restrict__ snq,
                                                          const int* __restrict__ lens, kv_elem_t<F8>* __restrict__ kc,
                                                          kv_elem_t<F8>* __restrict__ vc, int8_t* __restrict__ ke,
                                                          int8_t* __restrict__ ve, int cap, int nH, int nKV, int chunk, int ns,
                                                          float* __restrict__ part,
                                                          std::conditional_t<SH, DecodeShare, DecodeNoShare> sh = {}) {
  static_assert(!(SH && F8), "the shared-prompt mode is bf16 only");
  constexpr int LG = HD / 8, SLOTS = 64 / LG, half = HD / 2;
  __shared__ float red[4][G][HD + 2];
  const int s = blockIdx.x, g = blockIdx.y, b = blockIdx.z;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane % LG, slot = lane / LG, d0 = sub * 8;
  const int QKV = (nH + 2 * nKV) * HD;
  int pos = lens[b];
  if constexpr (SH) pos = max(pos - max(sh.plens[b / sh.n], 0), 0);  // index of the new token among the keys behind the prompt
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
    kv_elem_t<F8>* kp = kc + (cbase + j) * HD + d0;
    kv_elem_t<F8>* vp = vc + (cbase + j) * HD + d0;
    if (j == pos) {  // the new token: rotate, round once, append
      rope8<HD>(row, bias, (nH + g) * HD, d0, C, S, kf);
      const int cv = (nH + nKV + g) * HD + d0;
#pragma unroll
      for (int e = 0; e < 8; ++e) vf[e] = row[cv + e] + (bias ? bf16_to_f32(bias[cv + e]) : 0.f);
      uint4 kb = pack_bf16x8(kf), vb = pack_bf16x8(vf);
      if constexpr (F8) {
        int ek, ev;
        const uint2 kq = kv8_quantize<LG>(kb, &ek), vq = kv8_quantize<LG>(vb, &ev);
        *reinterpret_cast<uint2*>(kp) = kq;
        *reinterpret_cast<uint2*>(vp) = vq;
        if (sub == 0) { ke[cbase + j] = (int8_t)ek; ve[cbase + j] = (int8_t)ev; }
        kb = fp8_dequant8(kq, pow2i(ek));
        vb = fp8_dequant8(vq, pow2i(ev));
      } else {
        *reinterpret_cast<uint4*>(kp) = kb;
        *reinterpret_cast<uint4*>(vp) = vb;
      }
      unpack_bf16x8(kb, kf);
      unpack_bf16x8(vb, vf);
    } else if constexpr (F8) {
      const uint2 kq = *reinterpret_cast<const uint2*>(kp), vq = *reinterpret_cast<const uint2*>(vp);
      int ee = 0;  // both exponents in one register: one shuffle per key
      if (sub == 0) ee = ((int)ke[cbase + j] & 0xff) | ((int)ve[cbase + j] * 256);
      ee = __shfl(ee, lane - sub, 64);
      unpack_bf16x8(fp8_dequant8(kq, pow2i((int)(int8_t)(ee & 0xff))), kf);
      unpack_bf16x8(fp8_dequant8(vq, pow2i(ee >> 8)), vf);
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
    if constexpr (SH) dst = part + (((size_t)b * nH + g * G + i) * sh.ns_tot + sh.ns_off + s) * (HD + 2);
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

constexpr int AE_KB = 32;  // keys per LDS stage: two 16-key score tiles = one 32-deep PV step

// grid (ceil(T / 16), ns, B * nKV), 256 threads: one 16-query tile of one (row, KV group) over the keys of split y. The four
// waves stage each AE_KB-key block of the group once (K row-major, V transposed) and share it: wave w serves query heads
// w and w + 4 of the group. Scores are formed transposed, S^T = K Q^T, so that a lane ends up with P^T[keys][query] in the
// B-operand map of the PV product with no exchange: lane l (qd = l >> 4, j = l & 15) holds query j's keys 4 qd + r of the first
// tile and 16 + 4 qd + r of the second, and V^T is read with its contraction slots in that same key order. The output tile is
// O^T: lane l holds o[query j][d = 16 dt + 4 qd + r]. part == nullptr (one split): o is normalised and stored, rows t >= nl of
// the tile as zeros. Else part[((b T + t) nH + h) ns + split][HD + 4] = o (unnormalised), m, l for real rows; a split whose
// key range starts at or above the tile's last key writes nothing (the combine never reads it).
// F8: kc / vc hold codes, ke / ve one exponent per key. The staging keeps its piece map - thread v owns dims d0 .. d0 + 7 of key
// kr = v / (HD / 8) - so the HD / 8 consecutive lanes of a key read its HD code bytes as one run and a wave reads 512
// consecutive bytes (8 keys of 64 B, or 4 of 128 B); each lane also loads its key's two exponent bytes. The codes wait in
// registers under the previous block's products as the bf16 pieces do, at half the registers, and become bf16 on the way into
// LDS: Ks and Vt receive exactly the bits a bf16 cache of the dequantised keys would have put there, in the same layout (KS, VS
// and the bank spread stay as they are), so from LDS on this is the same kernel. Keys at or beyond k_hi are code 0, exponent 0.
template <int HD, int G, bool F8>
__global__ __launch_bounds__(256) void attn_extend_kernel(const bf16_t* __restrict__ qkv, const int* __restrict__ base_lens,
                                                          const int* __restrict__ new_lens, const kv_elem_t<F8>* __restrict__ kc,
                                                          const kv_elem_t<F8>* __restrict__ vc, const int8_t* __restrict__ ke,
                                                          const int8_t* __restrict__ ve, bf16_t* __restrict__ o,
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
  constexpr int NV = AE_KB * (HD / 8) / 256;  // 16-byte pieces of a K (and of a V) block per thread
  using piece_t = std::conditional_t<F8, uint2, uint4>;  // 8 dims of one key: codes or bf16
  piece_t kx[NV], vx[NV];
  int ex[F8 ? NV : 1];  // F8: the key's exponents, K in the low byte, V above
  // the block's K / V pieces of this thread into registers; keys at or beyond k_hi as zeros: p = 0 meets 0, never the
  // cache's bits
  auto fetch = [&](int kb) {
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int v = threadIdx.x + 256 * u;
      const int kr = v / (HD / 8), d0 = (v % (HD / 8)) * 8;
      const bool ok = kb + kr < k_hi;
      const size_t src = (cbase + (ok ? kb + kr : 0)) * HD + d0;
      kx[u] = ok ? *reinterpret_cast<const piece_t*>(kc + src) : piece_t{};
      vx[u] = ok ? *reinterpret_cast<const piece_t*>(vc + src) : piece_t{};
      if constexpr (F8) ex[u] = ok ? ((int)ke[cbase + kb + kr] & 0xff) | ((int)ve[cbase + kb + kr] * 256) : 0;
    }
  };
  if (k_lo < k_hi) fetch(k_lo);
  for (int kb = k_lo; kb < k_hi; kb += AE_KB) {
    __syncthreads();  // the previous block's fragment reads are done
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int v = threadIdx.x + 256 * u;
      const int kr = v / (HD / 8), d0 = (v % (HD / 8)) * 8;
      uint4 kbf, vbf;
      if constexpr (F8) {
        kbf = fp8_dequant8(kx[u], pow2i((int)(int8_t)(ex[u] & 0xff)));
        vbf = fp8_dequant8(vx[u], pow2i(ex[u] >> 8));
      } else {
        kbf = kx[u];
        vbf = vx[u];
      }
      *reinterpret_cast<uint4*>(&Ks[kr * KS + d0]) = kbf;
      const uint32_t w[4] = {vbf.x, vbf.y, vbf.z, vbf.w};
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

// ---- the launchers, one text for both cache forms (ke / ve: nullptr for bf16) -------------------------------------------------
template <bool F8>
int attn_decode_launch(const float* qkv, const bf16_t* bias, const float* cs, const float* sn, const float* csq, const float* snq,
                       const int* lens, kv_elem_t<F8>* kc, kv_elem_t<F8>* vc, int8_t* ke, int8_t* ve, int cap, int B, int nH,
                       int nKV, int head_dim, int kv_bound, bf16_t* o, float* part, size_t part_bytes, hipStream_t st) {
  if (B <= 0 || nKV <= 0 || nH % nKV || kv_bound <= 0 || kv_bound > cap) return -1;
  const int G = nH / nKV;
  if ((head_dim != 64 && head_dim != 128) || G > 8) return -1;
  const int chunk = slam::attn_decode_chunk(B, nH, nKV, head_dim, kv_bound, part_bytes);
  if (chunk <= 0) return -3;
  const int ns = (kv_bound + chunk - 1) / chunk;
  const dim3 grid(ns, nKV, B);
#define AD_CASE(HD, GG)                                                                                                      \
  case GG:                                                                                                                   \
    attn_decode_kernel<HD, GG, F8><<<grid, 256, 0, st>>>(qkv, bias, cs, sn, csq, snq, lens, kc, vc, ke, ve, cap, nH, nKV, chunk, \
                                                         ns, part);                                                          \
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

// the chunk's K / V are in the cache when this is called (the scatter launch of the caller's cache form, same stream)
template <bool F8>
int attn_extend_launch(const bf16_t* qkv, const int* base_lens, const int* new_lens, const kv_elem_t<F8>* kc,
                       const kv_elem_t<F8>* vc, const int8_t* ke, const int8_t* ve, int cap, int B, int T, int nH, int nKV,
                       int head_dim, int kv_bound, bf16_t* o, float* part, int chunk, int ns, hipStream_t st) {
  const int G = nH / nKV;
  const dim3 grid((T + 15) / 16, ns, B * nKV);
#define AE_CASE(HD, GG)                                                                                                       \
  case GG:                                                                                                                    \
    attn_extend_kernel<HD, GG, F8><<<grid, 256, 0, st>>>(qkv, base_lens, new_lens, kc, vc, ke, ve, o, part, T, nH, nKV, cap,    \
                                                         kv_bound, chunk, ns);                                                \
    break;
#define AE_SWITCH(HD) \
  switch (G) { AE_CASE(HD, 1) AE_CASE(HD, 2) AE_CASE(HD, 3) AE_CASE(HD, 4) AE_CASE(HD, 5) AE_CASE(HD, 6) AE_CASE(HD, 7) AE_CASE(HD, 8) }
  if (head_dim == 64) {
    AE_SWITCH(64)
    if (part) attn_extend_combine_kernel<64><<<dim3(nH, T, B), 64, 0, st>>>(part, base_lens, new_lens, T, nH, kv_bound, chunk, ns, o);
  } else {
    AE_SWITCH(128)
    if (part) attn_extend_combine_kernel<128><<<dim3(nH, T, B), 128, 0, st>>>(part, base_lens, new_lens, T, nH, kv_bound, chunk, ns, o);
  }
#undef AE_SWITCH
#undef AE_CASE
  return (int)hipGetLastError();
}

// argument checks and split plan of a chunk attention call, shared by both cache forms: 0, or the launcher's error
inline int attn_extend_plan(const void* qkv, const void* kc, const void* vc, const void* o, float* part, size_t part_bytes, int cap,
                            int B, int T, int nH, int nKV, int head_dim, int kv_bound, int* chunk, int* ns, float** pp) {
  if (B <= 0 || T <= 0 || nKV <= 0 || nH % nKV || kv_bound <= 0 || kv_bound > cap) return -1;
  const int G = nH / nKV;
  if ((head_dim != 64 && head_dim != 128) || G > 8) return -1;
  if ((int64_t)B * nKV > 65535 || T > 65535 || (int64_t)B * T > 0x7fffffffLL / (nH * (head_dim + 4))) return -1;
  if (((uintptr_t)qkv | (uintptr_t)kc | (uintptr_t)vc | (uintptr_t)o | (uintptr_t)part) & 15) return -1;
  *chunk = slam::attn_extend_chunk(B, T, nH, nKV, head_dim, kv_bound, part ? part_bytes : 0);
  *ns = (kv_bound + *chunk - 1) / *chunk;
  if (*ns > 65535) return -1;
  *pp = *ns > 1 ? part : nullptr;
  return 0;
}

}  // namespace
