// Weight-only FP8 for the decode stream (slam_quantize_decode_w8, include/slam_engine.h): rows of a bf16 matrix W[N][K] on a
// per-row power-of-two-scaled OCP e4m3fn grid.
//  * Exponent of row n, from the bf16 bits of amax = max_k |W[n][k]| = f 2^x (1 <= f < 2), integers only: 0 for a zero row,
//    else the smallest e with amax <= 448 2^e - that is x - 8 when f <= 1.75 (mantissa field <= 96), x - 7 above - clamped to
//    [W8_EXP_MIN, W8_EXP_MAX]. The maximum is order-free and exact, so the reduction order cannot show.
//  * Code: e4m3fn of W[n][k] 2^-e by v_cvt_pk_fp8_f32 (round to nearest even, the sign of zero kept). The scaling is exact
//    wherever the result is not below the grid, and |W 2^-e| <= 448, so nothing saturates and 0x7F / 0xFF never appear.
//  * Wdq = value(code) 2^e: four significant bits times a power of two, exact in fp32 and in bf16 (the one exception, a row whose
//    amax is within 2^-8 of the largest finite bf16, rounds up to 2^128 = inf; non-finite inputs are outside the contract).
//  * Code order (private to the engine, kernels.h w8_code_pos): every 64-deep K block of a row keeps its 64 bytes, permuted so
//    that 16 consecutive bytes are what one lane of gemm_skinny_w8 feeds to two consecutive 32-deep MFMA steps.
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int QW_WAVES = 4;  // rows per block, one wave each

SLAM_DEVICE int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// the exponent rule on the 15 magnitude bits of amax
SLAM_DEVICE int w8_exponent(int a) {
  if (a == 0) return 0;
  const int xb = a >> 7, m = a & 0x7f;
  if (xb == 0) return slam::W8_EXP_MIN;  // bf16 subnormals: x <= -127
  const int e = xb - 127 - (m <= 96 ? 8 : 7);
  return min(max(e, slam::W8_EXP_MIN), slam::W8_EXP_MAX);
}
SLAM_DEVICE float pow2i(int e) { return __uint_as_float((uint32_t)(e + 127) << 23); }

// the four codes of one dword -> two dwords of bf16 pairs: code -> fp32 -> times 2^e (exact) -> high 16 bits
SLAM_DEVICE uint2 w8_dequant4(uint32_t c, float sc) {
  const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)c, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)c, true);
  uint2 r;
  r.x = bf16_hi_pair(lo.x * sc, lo.y * sc);
  r.y = bf16_hi_pair(hi.x * sc, hi.y * sc);
  return r;
}

// grid ceil(N / 4) x 256 threads: wave w of block b owns row 4 b + w; a lane takes the 8-element chunks lane, lane + 64, ..
__global__ __launch_bounds__(256) void quantize_rows_fp8_kernel(bf16_t* __restrict__ W, uint8_t* __restrict__ Q,
                                                                int8_t* __restrict__ E, int N, int K) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * QW_WAVES + (threadIdx.x >> 6);
  if (n >= N) return;
  bf16_t* wrow = W + (size_t)n * K;
  uint8_t* qrow = Q + (size_t)n * K;
  const int chunks = K >> 3;
  int a = 0;
  for (int c = lane; c < chunks; c += 64) {
    const uint4 v = *reinterpret_cast<const uint4*>(wrow + 8 * c);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) a = max(a, max((int)(w[i] & 0x7fffu), (int)((w[i] >> 16) & 0x7fffu)));
  }
  a = wave_max_i(a);
  const int e = w8_exponent(a);
  if (lane == 0) E[n] = (int8_t)e;
  const float inv = pow2i(-e), sc = pow2i(e);
  for (int c = lane; c < chunks; c += 64) {
    const uint4 v = *reinterpret_cast<const uint4*>(wrow + 8 * c);
    float f[8];
    unpack_bf16x8(v, f);
    int c0 = 0, c1 = 0;
    c0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[0] * inv, f[1] * inv, c0, false);
    c0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[2] * inv, f[3] * inv, c0, true);
    c1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[4] * inv, f[5] * inv, c1, false);
    c1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[6] * inv, f[7] * inv, c1, true);
    *reinterpret_cast<uint2*>(qrow + slam::w8_code_pos(8 * c)) = uint2{(uint32_t)c0, (uint32_t)c1};
    const uint2 d0 = w8_dequant4((uint32_t)c0, sc), d1 = w8_dequant4((uint32_t)c1, sc);
    *reinterpret_cast<uint4*>(wrow + 8 * c) = uint4{d0.x, d0.y, d1.x, d1.y};
  }
}

__global__ __launch_bounds__(256) void dequantize_rows_fp8_kernel(const uint8_t* __restrict__ Q, const int8_t* __restrict__ E,
                                                                  bf16_t* __restrict__ W, int N, int K) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * QW_WAVES + (threadIdx.x >> 6);
  if (n >= N) return;
  const uint8_t* qrow = Q + (size_t)n * K;
  bf16_t* wrow = W + (size_t)n * K;
  const float sc = pow2i(E[n]);
  for (int c = lane; c < (K >> 3); c += 64) {
    const uint2 q = *reinterpret_cast<const uint2*>(qrow + slam::w8_code_pos(8 * c));
    const uint2 d0 = w8_dequant4(q.x, sc), d1 = w8_dequant4(q.y, sc);
    *reinterpret_cast<uint4*>(wrow + 8 * c) = uint4{d0.x, d0.y, d1.x, d1.y};
  }
}

inline bool w8_args_ok(const void* W, const void* Q, const void* E, int N, int K) {
  return W && Q && E && N > 0 && K > 0 && K % slam::W8_K_GRAIN == 0 && !(((uintptr_t)W | (uintptr_t)Q) & 15);
}

}  // namespace

namespace slam {

int quantize_rows_fp8(bf16_t* W, uint8_t* Q, int8_t* E, int N, int K, hipStream_t st) {
  if (!w8_args_ok(W, Q, E, N, K)) return -1;
  quantize_rows_fp8_kernel<<<nblocks((size_t)N, QW_WAVES), 64 * QW_WAVES, 0, st>>>(W, Q, E, N, K);
  LAUNCH_RET();
}

int dequantize_rows_fp8(const uint8_t* Q, const int8_t* E, bf16_t* W, int N, int K, hipStream_t st) {
  if (!w8_args_ok(W, Q, E, N, K)) return -1;
  dequantize_rows_fp8_kernel<<<nblocks((size_t)N, QW_WAVES), 64 * QW_WAVES, 0, st>>>(Q, E, W, N, K);
  LAUNCH_RET();
}

}  // namespace slam
