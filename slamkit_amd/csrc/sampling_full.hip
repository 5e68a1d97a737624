// Token choice over the whole vocabulary (include/slam_engine.h: slam_sample_tokens_full): top_k = 0 with temperature, top-p,
// min-p and epsilon_cutoff. No ranked candidate list exists and a 152,167-float row does not fit in LDS, so nothing is sorted or
// stored: a token's weight becomes a 41-bit integer mass q_i = (uint64)(exp2((x_i - x_max) sc) 2^40) and everything behind it is
// integer arithmetic - sums, a radix select on q whose bins hold MASS (u64) instead of counts, one Philox draw scaled by mulhi64
// and a prefix scan in id order. Integer sums commute, so the result does not depend on how a row is cut over lanes, waves,
// blocks or launches, and integer atomics (LDS and global) are allowed where floating-point ones are not.
//  * rows up to FS_SMALL_MAX scores: ONE launch, one block per row. The row maximum by wave reductions, the q_i into LDS
//    (u64 [4096]), four radix levels (11, 11, 11, 8 bits) on 2048 u64 LDS bins filled by LDS atomics, a block-wide exclusive
//    scan of the kept masses with thread t owning a contiguous id range, and the one thread whose range holds the draw walks it.
//  * longer rows: grid (chunks of FS_CHUNK scores, B), so that B = 1 .. 8 still fills the chip. Launches:
//      full_max      every chunk's (score key << 32 | ~id) maximum into ws; chunk 0 clears the row's state, bins and ticket
//      full_hist<L>  (top_p < 1: L = 0 .. 3) every block re-reads the chunk maxima, recomputes its q_i from the logits (the row
//                    is L2-resident; q is never stored), bins the masses under the prefix chosen so far in LDS and flushes its
//                    non-empty bins once with global u64 atomics; the LAST block to take the row's ticket (__threadfence, then
//                    one atomic counter) reads the 2048 bins, picks the digit, and clears bins and ticket for the next launch
//      full_mass<0>  (epsilon_cutoff > 0) per-chunk mass at or above the cut so far; the last block forms Q1 and the final cut
//      full_mass<1>  per-chunk kept mass; the last block sums them (Q2), draws, finds the chunk by a scan over the chunk
//                    masses and the token by the small form's scan inside that chunk
//    Greedy is full_max + one block per row over the chunk maxima. No block ever waits for another one: a block that is not
//    last simply ends, and the decision of a phase is read by the NEXT launch.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>

#include "../../include/slam_engine.h"
#include "common.h"

namespace slam {

// One argument block from the entry point down to the launches (the meaning of every field: slam_sample_tokens_at).
struct FullSampleArgs {
  const float* logits = nullptr;
  int B = 0, vocab = 0;
  const uint8_t* banned = nullptr;
  int do_sample = 0, top_k = 0;
  float temperature = 1.f, top_p = 1.f;
  uint64_t seed = 0;
  uint32_t step = 0;
  int pad_id = 0, n_eos = 0;
  const int64_t* row_ids = nullptr;
  const int* eos_ids = nullptr;
  uint8_t* done = nullptr;
  int64_t* next = nullptr;
  int64_t* out = nullptr;
  int64_t out_stride = 0;
  const uint32_t* steps = nullptr;
  int group = 1;
  int64_t out_col = 0;
  void* ws = nullptr;
  size_t ws_bytes = 0;
  float min_p = 0.f, typical_p = 1.f, epsilon_cutoff = 0.f, eta_cutoff = 0.f;
};

}  // namespace slam

namespace {

typedef unsigned long long u64_t;

constexpr int FS_THREADS = 256;
constexpr int FS_SMALL_MAX = SLAM_SAMPLE_FULL_SMALL_MAX;  // THE switch: rows up to this length take the one-block form
constexpr int FS_CHUNK = 2048;                            // scores per block of the long form
constexpr int FS_BINS = 2048;                             // 11-bit radix levels: 2048 x 8 B of LDS
constexpr int FS_MAX_VOCAB = 1 << 22;                     // Q <= vocab 2^40 stays below 2^63
constexpr u64_t FS_QMAX = 1ull << 40;                     // the mass of the row maximum
constexpr uint32_t FS_NEG_INF_KEY = 0x007fffffu;          // score_key(-inf): a live row's maximum has a larger key
static_assert(FS_SMALL_MAX >= FS_CHUNK && FS_SMALL_MAX % FS_THREADS == 0, "the small form's LDS and id ranges");

// the sampler's reading of a score: banned / NaN -> -inf, +inf -> FLT_MAX
SLAM_DEVICE float full_score(float x, bool banned) {
  if (banned || x != x) x = -INFINITY;
  return fminf(x, FLT_MAX);
}
// order-preserving integer image of a cleaned score (-0 -> +0), and back
SLAM_DEVICE uint32_t full_key(float x) {
  uint32_t u = __float_as_uint(x);
  if ((u << 1) == 0u) u = 0u;
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
SLAM_DEVICE float full_key_score(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

// q_i: two separately rounded fp32 operations, the device's exp2, an exact scaling by 2^40 and a truncation
SLAM_DEVICE u64_t full_mass_of(float x, float xmax, float sc) {
  const float y = (x - xmax) * sc;
  return (u64_t)(fast_exp2(y) * 1099511627776.0f);
}

// f(i, score) for the scores [c0, c0 + n) of one row, i the index in the chunk. The row may start at any 4-byte boundary:
// scalar loads up to the first 16-byte boundary, 16-byte loads from there, scalar loads for the rest.
template <class F>
SLAM_DEVICE void full_for_scores(const float* __restrict__ row, const uint8_t* __restrict__ banned, int c0, int n, F f) {
  const float* p = row + c0;
  const uint8_t* bn = banned ? banned + c0 : nullptr;
  int head = (int)((4u - (uint32_t)(((uintptr_t)p >> 2) & 3u)) & 3u);
  if (head > n) head = n;
  const int nv = (n - head) >> 2;
  const int t = threadIdx.x;
  if (t < head) f(t, full_score(p[t], bn && bn[t]));
  const float4* pv = reinterpret_cast<const float4*>(p + head);
  for (int v = t; v < nv; v += FS_THREADS) {
    const float4 x = pv[v];
    const int i = head + 4 * v;
    f(i + 0, full_score(x.x, bn && bn[i + 0]));
    f(i + 1, full_score(x.y, bn && bn[i + 1]));
    f(i + 2, full_score(x.z, bn && bn[i + 2]));
    f(i + 3, full_score(x.w, bn && bn[i + 3]));
  }
  for (int i = head + 4 * nv + t; i < n; i += FS_THREADS) f(i, full_score(p[i], bn && bn[i]));
}

struct FullShared {
  u64_t hist[FS_BINS];
  u64_t red[FS_THREADS / 64];
  u64_t pick[2];
  int last;
};

// The block-wide helpers below are called by EVERY thread of the block (barriers inside); `red` is free again on return.
SLAM_DEVICE u64_t full_block_max(u64_t v, u64_t* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64_t other = __shfl_xor(v, o, 64);
    v = other > v ? other : v;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = red[0];
#pragma unroll
  for (int w = 1; w < FS_THREADS / 64; ++w) v = red[w] > v ? red[w] : v;
  __syncthreads();
  return v;
}
// exclusive prefix of v over the threads in thread order, and the block's total
SLAM_DEVICE u64_t full_block_scan(u64_t v, u64_t* red, u64_t& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u64_t incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64_t up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) red[wave] = incl;
  __syncthreads();
  u64_t off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < FS_THREADS / 64; ++w) {
    if (w < wave) off += red[w];
    tot += red[w];
  }
  __syncthreads();
  total = tot;
  return off + incl - v;
}

// (score key << 32) | ~id of the best score of the chunk: larger is "higher score, then lower id"
SLAM_DEVICE u64_t full_chunk_max(const float* row, const uint8_t* banned, int c0, int n, u64_t* red) {
  u64_t best = 0;
  full_for_scores(row, banned, c0, n, [&](int i, float x) {
    const u64_t c = ((u64_t)full_key(x) << 32) | (u64_t)(0xffffffffu - (uint32_t)(c0 + i));
    best = c > best ? c : best;
  });
  return full_block_max(best, red);
}
SLAM_DEVICE bool full_dead(u64_t comp) { return (uint32_t)(comp >> 32) <= FS_NEG_INF_KEY; }

// the masses of the scores [c0, c0 + n) into LDS
SLAM_DEVICE void full_fill(const float* row, const uint8_t* banned, int c0, int n, float xmax, float sc, u64_t* qs) {
  full_for_scores(row, banned, c0, n, [&](int i, float x) { qs[i] = full_mass_of(x, xmax, sc); });
  __syncthreads();
}

// radix level L of the 41-bit mass: its digit sits at bit level_shift(L); the bits above it are the prefix of the levels before
SLAM_DEVICE constexpr int level_shift(int L) { return L == 0 ? 30 : L == 1 ? 19 : L == 2 ? 8 : 0; }
SLAM_DEVICE constexpr int level_bits(int L) { return L == 3 ? 8 : 11; }

// hist[digit] += q for the masses under `prefix` (integer LDS atomics; a mass of 0 adds nothing and is skipped)
SLAM_DEVICE void full_hist_add(const u64_t* qs, int n, u64_t* hist, int L, u64_t prefix) {
  const int shift = level_shift(L), up = shift + level_bits(L);
  const uint32_t mask = (1u << level_bits(L)) - 1u;
  for (int i = threadIdx.x; i < n; i += FS_THREADS) {
    const u64_t q = qs[i];
    if (q != 0 && (q >> up) == prefix) atomicAdd(&hist[(uint32_t)(q >> shift) & mask], q);
  }
}

// thr of the top-p cut from the row's mass Q: tokens are kept while S(q) > thr; thr < Q keeps the maximum
SLAM_DEVICE u64_t full_top_p_thr(float omp, u64_t Q) {
  const u64_t thr = (u64_t)((double)omp * (double)Q);
  return thr < Q ? thr : Q - 1;
}

// One level's decision. v: the thread's bins 8 t .. 8 t + 7 (mass of the values under the prefix, by digit). below: the mass of
// all smaller values. Invariant: below <= thr < below + (sum of the bins), so exactly one digit d has
// below + (bins < d) <= thr < below + (bins <= d). Returns d; below becomes the mass under (prefix, d).
SLAM_DEVICE uint32_t full_decide(const u64_t (&v)[8], u64_t& below, u64_t thr, FullShared& sh) {
  u64_t local = 0, total;
#pragma unroll
  for (int j = 0; j < 8; ++j) local += v[j];
  u64_t run = below + full_block_scan(local, sh.red, total);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (run <= thr && thr < run + v[j]) { sh.pick[0] = 8 * threadIdx.x + j; sh.pick[1] = run; }
    run += v[j];
  }
  __syncthreads();
  const uint32_t d = (uint32_t)sh.pick[0];
  below = sh.pick[1];
  __syncthreads();
  return d;
}

struct FullParams {
  int do_sample, vocab, nch, pad_id, n_eos, group, use_p;
  float sc, omp, eps;  // (1 / temperature) log2(e); 1 - top_p; epsilon_cutoff
  u64_t c_m;           // the min_p cut
  uint32_t k0, k1, step;
  long long out_stride, out_col;
};

SLAM_DEVICE void full_emit(long long tok, bool mark, int b, const FullParams& P, const int* eos_ids, uint8_t* done,
                           int64_t* next, int64_t* out) {
  next[b] = tok;
  if (out) out[(long long)b * P.out_stride + P.out_col] = tok;
  if (mark && done)
    for (int e = 0; e < P.n_eos; ++e)
      if (eos_ids[e] == (int)tok) { done[b] = 1; break; }
}

// the row's 64 random bits: slam_sample_tokens' counter and key, words 0 and 1
SLAM_DEVICE u64_t full_rand(int b, const FullParams& P, const int64_t* row_ids, const uint32_t* steps) {
  const int q = b / P.group;
  const uint64_t r = row_ids ? (uint64_t)row_ids[q] : (uint64_t)q;
  const uint32_t step = P.step + (steps ? steps[q] : 0u) + (uint32_t)(b - q * P.group);
  const Philox4 rnd = philox4x32_10((uint32_t)r, step, (uint32_t)(r >> 32), 0x53414D50u, P.k0, P.k1);
  return ((u64_t)rnd.w[0] << 32) | (u64_t)rnd.w[1];
}

// The index in qs[0 .. n) of the lowest i with q_i >= cut whose prefix sum of kept masses exceeds the target. Thread t owns the
// ids [t per, (t + 1) per). whole: the target is mulhi64(rnd, the kept mass of qs); else it is `target` (below the kept mass).
SLAM_DEVICE int full_draw(const u64_t* qs, int n, u64_t cut, bool whole, u64_t rnd, u64_t target, FullShared& sh) {
  const int per = (n + FS_THREADS - 1) / FS_THREADS;
  const int i0 = min(n, (int)threadIdx.x * per), i1 = min(n, i0 + per);
  u64_t local = 0, total;
  for (int i = i0; i < i1; ++i) local += qs[i] >= cut ? qs[i] : 0ull;
  if (threadIdx.x == 0) sh.pick[0] = 0;  // the maximum is kept, so one thread below overwrites it
  const u64_t excl = full_block_scan(local, sh.red, total);
  if (whole) target = __umul64hi(rnd, total);
  if (excl <= target && target < excl + local) {
    u64_t run = excl;
    for (int i = i0; i < i1; ++i) {
      if (qs[i] >= cut) {
        run += qs[i];
        if (run > target) { sh.pick[0] = (u64_t)i; break; }
      }
    }
  }
  __syncthreads();
  return (int)sh.pick[0];
}

// ---- rows up to FS_SMALL_MAX: one block per row, one launch ---------------------------------------------------------------------
__global__ __launch_bounds__(FS_THREADS) void full_small_kernel(const float* __restrict__ logits,
                                                                const uint8_t* __restrict__ banned,
                                                                const int64_t* __restrict__ row_ids,
                                                                const int* __restrict__ eos_ids, uint8_t* __restrict__ done,
                                                                int64_t* __restrict__ next, int64_t* __restrict__ out,
                                                                FullParams P, const uint32_t* __restrict__ steps) {
  __shared__ u64_t qs[FS_SMALL_MAX];
  __shared__ FullShared sh;
  const int b = blockIdx.x, t = threadIdx.x, n = P.vocab;
  const float* row = logits + (size_t)b * P.vocab;
  if (done && done[b]) {
    if (t == 0) full_emit(P.pad_id, false, b, P, eos_ids, done, next, out);
    return;
  }
  const u64_t comp = full_chunk_max(row, banned, 0, n, sh.red);
  if (full_dead(comp)) {  // no score above -inf: pad, the row is not marked done
    if (t == 0) full_emit(P.pad_id, false, b, P, eos_ids, done, next, out);
    return;
  }
  if (!P.do_sample) {
    if (t == 0) full_emit(0xffffffffu - (uint32_t)comp, true, b, P, eos_ids, done, next, out);
    return;
  }
  full_fill(row, banned, 0, n, full_key_score((uint32_t)(comp >> 32)), P.sc, qs);
  u64_t cut = P.c_m;
  if (P.use_p) {
    u64_t prefix = 0, below = 0, thr = 0;
#pragma unroll
    for (int L = 0; L < 4; ++L) {
      for (int i = t; i < FS_BINS; i += FS_THREADS) sh.hist[i] = 0;
      __syncthreads();
      full_hist_add(qs, n, sh.hist, L, prefix);
      __syncthreads();
      u64_t v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = sh.hist[8 * t + j];
      if (L == 0) {
        u64_t local = 0, Q;
#pragma unroll
        for (int j = 0; j < 8; ++j) local += v[j];
        full_block_scan(local, sh.red, Q);
        thr = full_top_p_thr(P.omp, Q);
      }
      const uint32_t d = full_decide(v, below, thr, sh);
      prefix = (prefix << level_bits(L)) | d;
    }
    cut = prefix > cut ? prefix : cut;
  }
  if (P.eps > 0.f) {
    u64_t local = 0, Q1;
    for (int i = t; i < n; i += FS_THREADS) local += qs[i] >= cut ? qs[i] : 0ull;
    full_block_scan(local, sh.red, Q1);
    const u64_t c_e = (u64_t)ceil((double)P.eps * (double)Q1);
    cut = c_e > cut ? c_e : cut;
    cut = cut < FS_QMAX ? cut : FS_QMAX;
  }
  const int pick = full_draw(qs, n, cut, true, full_rand(b, P, row_ids, steps), 0, sh);
  if (t == 0) full_emit(pick, true, b, P, eos_ids, done, next, out);
}

// ---- longer rows: grid (chunks, B) -------------------------------------------------------------------------------------------
// A row's part of the workspace: FullRow, bins [FS_BINS], cmax [nch], cmass [nch], all u64.
struct alignas(8) FullRow {
  u64_t prefix, below, thr, cut;
  uint32_t ticket, unused;
};
SLAM_DEVICE size_t full_row_words(int nch) { return sizeof(FullRow) / 8 + FS_BINS + 2 * (size_t)nch; }
struct FullWs {
  FullRow* st;
  u64_t* bins;
  u64_t* cmax;
  u64_t* cmass;
  SLAM_DEVICE FullWs(u64_t* ws, int b, int nch) {
    u64_t* p = ws + (size_t)b * full_row_words(nch);
    st = reinterpret_cast<FullRow*>(p);
    bins = p + sizeof(FullRow) / 8;
    cmax = bins + FS_BINS;
    cmass = cmax + nch;
  }
};
// what another block of THIS launch wrote, read past this CU's vector cache
SLAM_DEVICE u64_t full_peek(const u64_t* p) { return __hip_atomic_load(const_cast<u64_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Is this block the last of the row's nch blocks to get here? Everything the block wrote before the call is visible to the
// block that gets `true`. Nobody waits: the others go on (and end).
SLAM_DEVICE bool full_take_ticket(FullRow* st, int nch, FullShared& sh) {
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) sh.last = atomicAdd(&st->ticket, 1u) == (uint32_t)(nch - 1) ? 1 : 0;
  __syncthreads();
  const bool last = sh.last != 0;
  if (last) __threadfence();
  return last;
}

// the row's best composite from the chunk maxima of full_max_kernel (an earlier launch)
SLAM_DEVICE u64_t full_row_max(const u64_t* cmax, int nch, u64_t* red) {
  u64_t best = 0;
  for (int c = threadIdx.x; c < nch; c += FS_THREADS) best = cmax[c] > best ? cmax[c] : best;
  return full_block_max(best, red);
}

__global__ __launch_bounds__(FS_THREADS) void full_max_kernel(const float* __restrict__ logits,
                                                              const uint8_t* __restrict__ banned,
                                                              const uint8_t* __restrict__ done, FullParams P,
                                                              u64_t* __restrict__ ws) {
  __shared__ u64_t red[FS_THREADS / 64];
  const int ch = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  if (done && done[b]) return;
  const FullWs w(ws, b, P.nch);
  const int c0 = ch * FS_CHUNK;
  const u64_t comp = full_chunk_max(logits + (size_t)b * P.vocab, banned, c0, min(FS_CHUNK, P.vocab - c0), red);
  if (t == 0) w.cmax[ch] = comp;
  if (ch == 0) {  // nothing of an earlier call survives: the bins, the ticket and the cut so far (min_p's)
    for (int i = t; i < FS_BINS; i += FS_THREADS) w.bins[i] = 0;
    if (t == 0) *w.st = FullRow{0, 0, 0, P.c_m, 0u, 0u};
  }
}

__global__ __launch_bounds__(FS_THREADS) void full_greedy_kernel(const int* __restrict__ eos_ids, uint8_t* __restrict__ done,
                                                                 int64_t* __restrict__ next, int64_t* __restrict__ out,
                                                                 FullParams P, const u64_t* __restrict__ ws) {
  __shared__ u64_t red[FS_THREADS / 64];
  const int b = blockIdx.x;
  const bool fin = done && done[b];
  u64_t comp = 0;
  if (!fin) comp = full_row_max(FullWs(const_cast<u64_t*>(ws), b, P.nch).cmax, P.nch, red);
  if (threadIdx.x != 0) return;
  if (fin || full_dead(comp)) full_emit(P.pad_id, false, b, P, eos_ids, done, next, out);
  else full_emit(0xffffffffu - (uint32_t)comp, true, b, P, eos_ids, done, next, out);
}

// radix level L of the top-p cut: the chunk's masses under the prefix into LDS bins, one flush, and the last block decides
template <int L>
__global__ __launch_bounds__(FS_THREADS) void full_hist_kernel(const float* __restrict__ logits,
                                                               const uint8_t* __restrict__ banned,
                                                               const uint8_t* __restrict__ done, FullParams P,
                                                               u64_t* __restrict__ ws) {
  __shared__ u64_t qs[FS_CHUNK];
  __shared__ FullShared sh;
  const int ch = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  if (done && done[b]) return;
  const FullWs w(ws, b, P.nch);
  const u64_t comp = full_row_max(w.cmax, P.nch, sh.red);
  if (full_dead(comp)) return;
  const u64_t prefix = L == 0 ? 0ull : w.st->prefix;
  const int c0 = ch * FS_CHUNK, n = min(FS_CHUNK, P.vocab - c0);
  for (int i = t; i < FS_BINS; i += FS_THREADS) sh.hist[i] = 0;
  full_fill(logits + (size_t)b * P.vocab, banned, c0, n, full_key_score((uint32_t)(comp >> 32)), P.sc, qs);
  full_hist_add(qs, n, sh.hist, L, prefix);
  __syncthreads();
  for (int i = t; i < FS_BINS; i += FS_THREADS)
    if (sh.hist[i] != 0) atomicAdd(&w.bins[i], sh.hist[i]);
  if (!full_take_ticket(w.st, P.nch, sh)) return;
  u64_t v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    v[j] = full_peek(&w.bins[8 * t + j]);
    w.bins[8 * t + j] = 0;  // for the next level's launch
  }
  u64_t below = 0, thr;
  if (L == 0) {
    u64_t local = 0, Q;
#pragma unroll
    for (int j = 0; j < 8; ++j) local += v[j];
    full_block_scan(local, sh.red, Q);
    thr = full_top_p_thr(P.omp, Q);
  } else {
    below = w.st->below;
    thr = w.st->thr;
  }
  const uint32_t d = full_decide(v, below, thr, sh);
  if (t == 0) {
    const u64_t np = (prefix << level_bits(L)) | d;
    w.st->prefix = np;
    w.st->below = below;
    w.st->thr = thr;
    if (L == 3 && np > w.st->cut) w.st->cut = np;  // c_p against min_p's cut
    w.st->ticket = 0;
  }
}

// per-chunk mass at or above the cut. FINAL = false: the last block forms Q1 and epsilon_cutoff's cut. FINAL = true: the last
// block forms Q2, draws, and finds the chunk and the token.
template <bool FINAL>
__global__ __launch_bounds__(FS_THREADS) void full_mass_kernel(const float* __restrict__ logits,
                                                               const uint8_t* __restrict__ banned,
                                                               const int64_t* __restrict__ row_ids,
                                                               const int* __restrict__ eos_ids, uint8_t* __restrict__ done,
                                                               int64_t* __restrict__ next, int64_t* __restrict__ out,
                                                               FullParams P, u64_t* __restrict__ ws,
                                                               const uint32_t* __restrict__ steps) {
  __shared__ u64_t qs[FS_CHUNK];
  __shared__ FullShared sh;
  const int ch = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const bool fin = done && done[b];
  const FullWs w(ws, b, P.nch);
  u64_t comp = 0;
  if (!fin) comp = full_row_max(w.cmax, P.nch, sh.red);
  if (fin || full_dead(comp)) {
    if (FINAL && ch == 0 && t == 0) full_emit(P.pad_id, false, b, P, eos_ids, done, next, out);
    return;
  }
  const float* row = logits + (size_t)b * P.vocab;
  const float xmax = full_key_score((uint32_t)(comp >> 32));
  const u64_t cut = w.st->cut;
  const int c0 = ch * FS_CHUNK, n = min(FS_CHUNK, P.vocab - c0);
  full_fill(row, banned, c0, n, xmax, P.sc, qs);
  u64_t local = 0, total;
  for (int i = t; i < n; i += FS_THREADS) local += qs[i] >= cut ? qs[i] : 0ull;
  full_block_scan(local, sh.red, total);
  if (t == 0) w.cmass[ch] = total;
  if (!full_take_ticket(w.st, P.nch, sh)) return;
  local = 0;
  for (int c = t; c < P.nch; c += FS_THREADS) local += full_peek(&w.cmass[c]);
  full_block_scan(local, sh.red, total);
  if (!FINAL) {
    if (t == 0) {
      u64_t c_e = (u64_t)ceil((double)P.eps * (double)total);
      c_e = c_e > cut ? c_e : cut;
      w.st->cut = c_e < FS_QMAX ? c_e : FS_QMAX;
      w.st->ticket = 0;
    }
    return;
  }
  const u64_t target = __umul64hi(full_rand(b, P, row_ids, steps), total);
  if (t == 0) sh.pick[0] = sh.pick[1] = 0;
  u64_t base = 0;  // the kept mass of the chunks in front of the tile
  for (int cb = 0; cb < P.nch; cb += FS_THREADS) {
    const u64_t m = cb + t < P.nch ? full_peek(&w.cmass[cb + t]) : 0ull;
    u64_t tile;
    const u64_t lo = base + full_block_scan(m, sh.red, tile);
    if (lo <= target && target < lo + m) { sh.pick[0] = (u64_t)(cb + t); sh.pick[1] = lo; }
    base += tile;
  }
  __syncthreads();
  const int pc = min((int)sh.pick[0], P.nch - 1);
  const u64_t rel = target - sh.pick[1];
  __syncthreads();
  const int p0 = pc * FS_CHUNK, pn = min(FS_CHUNK, P.vocab - p0);
  full_fill(row, banned, p0, pn, xmax, P.sc, qs);
  const int pick = full_draw(qs, pn, cut, false, 0, rel, sh);
  if (t == 0) {
    full_emit(p0 + pick, true, b, P, eos_ids, done, next, out);
    w.st->ticket = 0;
  }
}

int full_chunks(int vocab) { return (vocab + FS_CHUNK - 1) / FS_CHUNK; }

}  // namespace

namespace slam {

size_t sample_full_workspace_bytes(int B, int vocab) {
  if (B <= 0 || B > 65535 || vocab <= 0 || vocab > FS_MAX_VOCAB) return 0;
  if (vocab <= FS_SMALL_MAX) return 8;  // the one-block form keeps everything in LDS
  return (size_t)B * (sizeof(FullRow) + 8 * ((size_t)FS_BINS + 2 * (size_t)full_chunks(vocab)));
}

int sample_tokens_full(const FullSampleArgs& a, hipStream_t st) {
  if (!a.logits || !a.next || a.B <= 0 || a.B > 65535 || a.vocab <= 0 || a.vocab > FS_MAX_VOCAB || ((uintptr_t)a.logits & 3))
    return -1;
  if (a.top_k != 0 || !(a.temperature > 0.f) || !(a.top_p > 0.f) || a.top_p > 1.f) return -1;
  if (a.n_eos < 0 || (a.n_eos > 0 && !a.eos_ids)) return -1;
  if (a.group < 1 || a.B % a.group != 0 || a.out_col < 0) return -1;
  if (!a.ws || ((uintptr_t)a.ws & 7) || a.ws_bytes < sample_full_workspace_bytes(a.B, a.vocab)) return -1;
  // the negated forms refuse NaN; typical_p and eta_cutoff need a floating-point entropy and stay outside the integer rule
  if (!(a.min_p >= 0.f && a.min_p <= 1.f) || !(a.epsilon_cutoff >= 0.f && a.epsilon_cutoff < 1.f)) return -1;
  if (!(a.typical_p == 1.f) || !(a.eta_cutoff == 0.f)) return -1;
  const float sc = (1.0f / a.temperature) * 1.44269504f;
  if (!isfinite(sc) || !(sc > 0.f)) return -1;
  FullParams P;
  P.do_sample = a.do_sample ? 1 : 0;
  P.vocab = a.vocab;
  P.nch = full_chunks(a.vocab);
  P.pad_id = a.pad_id;
  P.n_eos = a.n_eos;
  P.group = a.group;
  P.use_p = a.top_p < 1.0f ? 1 : 0;
  P.sc = sc;
  P.omp = 1.0f - a.top_p;
  P.eps = a.epsilon_cutoff;
  P.c_m = (u64_t)((double)a.min_p * (double)FS_QMAX);
  P.k0 = (uint32_t)a.seed;
  P.k1 = (uint32_t)(a.seed >> 32);
  P.step = a.step;
  P.out_stride = a.out_stride;
  P.out_col = a.out_col;
  if (a.vocab <= FS_SMALL_MAX) {
    full_small_kernel<<<a.B, FS_THREADS, 0, st>>>(a.logits, a.banned, a.row_ids, a.eos_ids, a.done, a.next, a.out, P, a.steps);
    return (int)hipGetLastError();
  }
  u64_t* ws = reinterpret_cast<u64_t*>(a.ws);
  const dim3 grid(P.nch, a.B);
  full_max_kernel<<<grid, FS_THREADS, 0, st>>>(a.logits, a.banned, a.done, P, ws);
  if (!P.do_sample) {
    full_greedy_kernel<<<a.B, FS_THREADS, 0, st>>>(a.eos_ids, a.done, a.next, a.out, P, ws);
    return (int)hipGetLastError();
  }
  if (P.use_p) {
    full_hist_kernel<0><<<grid, FS_THREADS, 0, st>>>(a.logits, a.banned, a.done, P, ws);
    full_hist_kernel<1><<<grid, FS_THREADS, 0, st>>>(a.logits, a.banned, a.done, P, ws);
    full_hist_kernel<2><<<grid, FS_THREADS, 0, st>>>(a.logits, a.banned, a.done, P, ws);
    full_hist_kernel<3><<<grid, FS_THREADS, 0, st>>>(a.logits, a.banned, a.done, P, ws);
  }
  if (P.eps > 0.f)
    full_mass_kernel<false><<<grid, FS_THREADS, 0, st>>>(a.logits, a.banned, a.row_ids, a.eos_ids, a.done, a.next, a.out, P, ws,
                                                         a.steps);
  full_mass_kernel<true><<<grid, FS_THREADS, 0, st>>>(a.logits, a.banned, a.row_ids, a.eos_ids, a.done, a.next, a.out, P, ws,
                                                      a.steps);
  return (int)hipGetLastError();
}

}  // namespace slam

using namespace slam;

extern "C" {

size_t slam_sample_full_workspace_bytes(int32_t B, int32_t vocab) { return sample_full_workspace_bytes(B, vocab); }

int slam_sample_tokens_full(const float* logits, int32_t B, int32_t vocab, const uint8_t* banned, const SlamSampleDesc* desc,
                            const int64_t* row_ids, const int32_t* eos_ids, uint8_t* done, int64_t* next, int64_t* out,
                            int64_t out_stride, void* ws, size_t ws_bytes, const uint32_t* steps, int32_t group, int32_t out_col,
                            const SlamWarpDesc* warp, slam_stream_t stream) {
  if (!desc || (desc->do_sample != 0 && desc->do_sample != 1) || desc->n_eos > 16) return SLAM_EINVAL;
  if (group < 1 || out_col < 0 || ((uintptr_t)steps & 3)) return SLAM_EINVAL;
  FullSampleArgs a;  // sample_tokens_full refuses the rest (-1 = SLAM_EINVAL) before it launches anything
  if (warp) {
    a.min_p = warp->min_p;
    a.typical_p = warp->typical_p;
    a.epsilon_cutoff = warp->epsilon_cutoff;
    a.eta_cutoff = warp->eta_cutoff;
  }
  a.logits = logits;
  a.B = B;
  a.vocab = vocab;
  a.banned = banned;
  a.do_sample = desc->do_sample;
  a.top_k = desc->top_k;
  a.temperature = desc->temperature;
  a.top_p = desc->top_p;
  a.seed = desc->seed;
  a.step = desc->step;
  a.pad_id = desc->pad_id;
  a.n_eos = desc->n_eos;
  a.row_ids = row_ids;
  a.eos_ids = eos_ids;
  a.done = done;
  a.next = next;
  a.out = out;
  a.out_stride = out_stride;
  a.steps = steps;
  a.group = group;
  a.out_col = out_col;
  a.ws = ws;
  a.ws_bytes = ws_bytes;
  return sample_tokens_full(a, (hipStream_t)stream);
}

}  // extern "C"
