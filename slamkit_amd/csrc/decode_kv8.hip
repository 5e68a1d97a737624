// The FP8 KV cache of cached generation (include/slam_engine.h: SLAM_KV_FP8_E4M3): every key and every value vector - one
// (layer, K | V, row, kv head, position), hd elements - as hd e4m3 codes plus one int8 power-of-two exponent, by the rule of the
// FP8 decode weights (common.h: fp8_exponent, fp8_encode8, fp8_dequant4). One layer's view: codes kc / vc [B][nKV][cap][hd]
// bytes in dim order, exponents ke / ve [B][nKV][cap].
//  * kv_scatter_fp8 / kv_extend_scatter_fp8: the prefill's and a chunk's already rotated bf16 K / V -> codes + exponents. The
//    hd / 8 consecutive lanes of a vector load 16 B each, take the absolute maximum of the 15-bit magnitudes across the group
//    by the xor butterfly (integers: order-free), and store 8 codes each as one 8-byte store; the first lane stores the exponent.
//  * attn_decode / attn_extend over codes: the F8 instantiations of decode_attn.h. Their output is, bit for bit, the bf16
//    kernels' output over a bf16 cache that holds the dequantised values.
//  * kv_repeat_fp8: the fan-out of slam_kv_repeat, byte for byte, codes and exponents (the launch order and its hazard argument
//    are kv_repeat's, decode.hip).
#include <hip/hip_runtime.h>

#include "common.h"
#include "decode_attn.h"
#include "kernels.h"

namespace {

inline unsigned nblk8(size_t n, int per) { return (unsigned)((n + per - 1) / per); }

// Lane idx of a token row owns dims d .. d + 7 of vector (kv, g); the LG lanes of a vector are consecutive, aligned and share
// `live`, so the butterfly of a live group meets live lanes only. src: the lane's 16 bytes of the rotated qkv row.
template <int LG>
SLAM_DEVICE void kv8_store(bool live, const bf16_t* src, uint8_t* codes, int8_t* exps, size_t vec, int d) {
  const uint4 v = live ? *reinterpret_cast<const uint4*>(src) : uint4{0u, 0u, 0u, 0u};
  int e;
  const uint2 q = kv8_quantize<LG>(v, &e);
  if (!live) return;
  *reinterpret_cast<uint2*>(codes + vec * (LG * 8) + d) = q;
  if (d == 0) exps[vec] = (int8_t)e;
}

// K / V columns of rows t < lens[b] of one layer's qkv [B*T][QKV] -> cache rows t of (b, kv head); grid (.., B). The index map
// is kv_scatter_kernel's (decode.hip).
template <int HD>
__global__ __launch_bounds__(256) void kv_scatter_fp8_kernel(const bf16_t* __restrict__ qkv, uint8_t* __restrict__ kc,
                                                             uint8_t* __restrict__ vc, int8_t* __restrict__ ke,
                                                             int8_t* __restrict__ ve, const int* __restrict__ lens, int T, int nH,
                                                             int nKV, int cap) {
  constexpr int LG = HD / 8;
  const int b = blockIdx.y;
  const int per_row = 2 * nKV * LG;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int t = idx / per_row, c = idx % per_row;
  const bool live = t < T && t < lens[b] && t < cap;
  const int kv = c / (nKV * LG), r = c % (nKV * LG);
  const int g = r / LG, d = (r % LG) * 8;
  const int QKV = (nH + 2 * nKV) * HD;
  const bf16_t* src = qkv + ((size_t)b * T + (live ? t : 0)) * QKV + (nH + kv * nKV + g) * HD + d;
  kv8_store<LG>(live, src, kv ? vc : kc, kv ? ve : ke, ((size_t)b * nKV + g) * cap + t, d);
}

// K / V columns of the real tokens t < nl of qkv [B*T][QKV] -> cache rows base + t of (b, kv head); grid (.., B)
template <int HD>
__global__ __launch_bounds__(256) void kv_extend_scatter_fp8_kernel(const bf16_t* __restrict__ qkv, uint8_t* __restrict__ kc,
                                                                    uint8_t* __restrict__ vc, int8_t* __restrict__ ke,
                                                                    int8_t* __restrict__ ve, const int* __restrict__ base_lens,
                                                                    const int* __restrict__ new_lens, int T, int nH, int nKV,
                                                                    int cap, int kv_bound) {
  constexpr int LG = HD / 8;
  const int b = blockIdx.y;
  const ExtRow R = ext_row(base_lens, new_lens, b, T, kv_bound);
  const int per_row = 2 * nKV * LG;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int t = idx / per_row, c = idx % per_row;
  const bool live = t < R.nl;
  const int kv = c / (nKV * LG), r = c % (nKV * LG);
  const int g = r / LG, d = (r % LG) * 8;
  const int QKV = (nH + 2 * nKV) * HD;
  const bf16_t* src = qkv + ((size_t)b * T + (live ? t : 0)) * QKV + (nH + kv * nKV + g) * HD + d;
  kv8_store<LG>(live, src, kv ? vc : kc, kv ? ve : ke, ((size_t)b * nKV + g) * cap + R.base + t, d);
}

constexpr int KR8_MAX_X = 64;  // blocks along a slab (grid-stride beyond)

// One source row b of the cache -> rows b n .. b n + n - 1 (never onto itself). grid (x, nslab + 1): slab y < nslab is
// (layer, K | V, kv head): the first lens[b] keys' codes ([cap][hd] bytes, as 16-byte pieces) and exponents ([cap] bytes) are
// copied; y == nslab replicates lens and logits.
__global__ __launch_bounds__(256) void kv_repeat_fp8_kernel(uint8_t* __restrict__ codes, int8_t* __restrict__ exps,
                                                            int* __restrict__ lens, float* __restrict__ logits, int b, int n,
                                                            int bmax, int nKV, int cap, int hd, int nslab, int vocab) {
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
  const int keys = min(max(len, 0), cap);
  const size_t slab = (size_t)cap * hd;
  const size_t srow = ((size_t)lk * bmax + b) * nKV + g;
  const uint4* src = reinterpret_cast<const uint4*>(codes + srow * slab);
  const int nv = keys * (hd / 16);
  for (int v = i0; v < nv; v += step) {
    const uint4 x = src[v];
    for (int i = 0; i < n; ++i) {
      const int r = b * n + i;
      if (r != b) reinterpret_cast<uint4*>(codes + (((size_t)lk * bmax + r) * nKV + g) * slab)[v] = x;
    }
  }
  for (int k = i0; k < keys; k += step) {
    const int8_t e = exps[srow * cap + k];
    for (int i = 0; i < n; ++i) {
      const int r = b * n + i;
      if (r != b) exps[(((size_t)lk * bmax + r) * nKV + g) * cap + k] = e;
    }
  }
}

inline bool kv8_ptrs_ok(const void* kc, const void* vc, const void* ke, const void* ve) {
  return kc && vc && ke && ve && !(((uintptr_t)kc | (uintptr_t)vc) & 15);
}

}  // namespace

namespace slam {

int kv_scatter_fp8(const bf16_t* qkv, uint8_t* kc, uint8_t* vc, int8_t* ke, int8_t* ve, const int* lens, int B, int T, int nH,
                   int nKV, int head_dim, int cap, hipStream_t st) {
  if (!qkv || !lens || !kv8_ptrs_ok(kc, vc, ke, ve) || ((uintptr_t)qkv & 15)) return -1;
  if (B <= 0 || B > 65535 || T <= 0 || nH <= 0 || nKV <= 0 || cap <= 0 || (head_dim != 64 && head_dim != 128)) return -1;
  const dim3 grid(nblk8((size_t)T * (2 * nKV * head_dim / 8), 256), B);
  if (head_dim == 64) kv_scatter_fp8_kernel<64><<<grid, 256, 0, st>>>(qkv, kc, vc, ke, ve, lens, T, nH, nKV, cap);
  else kv_scatter_fp8_kernel<128><<<grid, 256, 0, st>>>(qkv, kc, vc, ke, ve, lens, T, nH, nKV, cap);
  return (int)hipGetLastError();
}

int kv_extend_scatter_fp8(const bf16_t* qkv, uint8_t* kc, uint8_t* vc, int8_t* ke, int8_t* ve, const int* base_lens,
                          const int* new_lens, int B, int T, int nH, int nKV, int head_dim, int cap, int kv_bound, hipStream_t st) {
  if (!qkv || !base_lens || !new_lens || !kv8_ptrs_ok(kc, vc, ke, ve) || ((uintptr_t)qkv & 15)) return -1;
  if (B <= 0 || B > 65535 || T <= 0 || nH <= 0 || nKV <= 0 || (head_dim != 64 && head_dim != 128)) return -1;
  if (kv_bound <= 0 || kv_bound > cap) return -1;
  const dim3 grid(nblk8((size_t)T * (2 * nKV * head_dim / 8), 256), B);
  if (head_dim == 64)
    kv_extend_scatter_fp8_kernel<64><<<grid, 256, 0, st>>>(qkv, kc, vc, ke, ve, base_lens, new_lens, T, nH, nKV, cap, kv_bound);
  else
    kv_extend_scatter_fp8_kernel<128><<<grid, 256, 0, st>>>(qkv, kc, vc, ke, ve, base_lens, new_lens, T, nH, nKV, cap, kv_bound);
  return (int)hipGetLastError();
}

int attn_decode_fp8(const float* qkv, const bf16_t* bias, const float* cs, const float* sn, const float* csq, const float* snq,
                    const int* lens, uint8_t* kc, uint8_t* vc, int8_t* ke, int8_t* ve, int cap, int B, int nH, int nKV,
                    int head_dim, int kv_bound, bf16_t* o, float* part, size_t part_bytes, hipStream_t st) {
  if (!kv8_ptrs_ok(kc, vc, ke, ve)) return -1;
  return attn_decode_launch<true>(qkv, bias, cs, sn, csq, snq, lens, kc, vc, ke, ve, cap, B, nH, nKV, head_dim, kv_bound, o, part,
                                  part_bytes, st);
}

int attn_extend_fp8(const bf16_t* qkv, const int* base_lens, const int* new_lens, uint8_t* kc, uint8_t* vc, int8_t* ke, int8_t* ve,
                    int cap, int B, int T, int nH, int nKV, int head_dim, int kv_bound, bf16_t* o, float* part, size_t part_bytes,
                    hipStream_t st) {
  if (!kv8_ptrs_ok(kc, vc, ke, ve)) return -1;
  int chunk, ns;
  float* pp;
  if (int r = attn_extend_plan(qkv, kc, vc, o, part, part_bytes, cap, B, T, nH, nKV, head_dim, kv_bound, &chunk, &ns, &pp)) return r;
  if (int r = kv_extend_scatter_fp8(qkv, kc, vc, ke, ve, base_lens, new_lens, B, T, nH, nKV, head_dim, cap, kv_bound, st)) return r;
  return attn_extend_launch<true>(qkv, base_lens, new_lens, kc, vc, ke, ve, cap, B, T, nH, nKV, head_dim, kv_bound, o, pp, chunk, ns,
                                  st);
}

int kv_repeat_fp8(uint8_t* codes, int8_t* exps, int* lens, float* logits, int B, int n, int bmax, int L, int nKV, int head_dim,
                  int cap, int kv_bound, int vocab, hipStream_t st) {
  if (!codes || !exps || !lens || B <= 0 || n < 1 || (int64_t)B * n > bmax || (head_dim & 15) || kv_bound <= 0 || kv_bound > cap)
    return -1;
  if (((uintptr_t)codes) & 15) return -1;
  if (n == 1) return 0;
  const int nslab = L * 2 * nKV;
  if (nslab + 1 > 65535) return -1;
  size_t per = (size_t)kv_bound * (head_dim / 16);
  if (logits && (size_t)vocab > per) per = (size_t)vocab;
  unsigned gx = nblk8(per, 256);
  if (gx > (unsigned)KR8_MAX_X) gx = KR8_MAX_X;
  for (int b = B - 1; b >= 0; --b)  // descending: decode.hip's header comment
    kv_repeat_fp8_kernel<<<dim3(gx, nslab + 1), 256, 0, st>>>(codes, exps, lens, logits, b, n, bmax, nKV, cap, head_dim, nslab, vocab);
  return (int)hipGetLastError();
}

}  // namespace slam
