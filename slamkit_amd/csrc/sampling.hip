// Token choice for generation (include/slam_engine.h): the kernels, their launchers and their C entry points. None of them
// takes a SlamEngine; the argument blocks below are private to this file.
//  * sample_tokens (slam_sample_tokens): the next token of every row from its fp32 logits, on the device. A candidate is the
//    64-bit composite (order-preserving image of the score << idbits) | (idmask - id): all composites of a row differ and
//    "larger" is exactly "higher score, then lower id", so the top k is an exact radix select (integer LDS histograms, 8 bits a
//    pass, stopping as soon as a digit's bin is taken whole) and needs no float comparison. Rows longer than one chunk go
//    through two launches: every (chunk, row) block selects its local top k into the workspace, one block per row selects
//    among those, ranks the k' survivors and does the weights, the top-p cut, the Philox draw and the EOS / done / pad part.
//    Thread 0 forms the sums in the stated order: no floating-point atomics, nothing depends on the grid.
//    slam_sample_tokens_warped adds min_p / typical_p / epsilon_cutoff / eta_cutoff (HF's order) between the top-p cut and the
//    draw as a further instantiation of that last kernel: a thread per rank holds its membership of the kept set, thread 0
//    forms each normaliser and entropy in rank order, the typical_p order is formed by counting as the rank is.
//  * constrain_scores (slam_constrain_scores): -inf for the tokens a row's own history bans (no repeated n-gram, bad word
//    sequences, EOS ids while the row is too short, begin-suppressed ids), the logits' bits elsewhere. Grid (chunks, B): a
//    block copies its chunk (not in place), then scans the history and stores the bans inside its own chunk. One constant is
//    stored, so equal stores may race: no atomics, no ordering between blocks.
//  * token_logprobs (slam_token_logprobs): the log-softmax of the raw logits row at one token. Chunks of SP_CHUNK scores; in a
//    chunk thread t takes scores t, t + 256, .. in that order, the 64 lanes of a wave are summed by the xor butterfly 32, 16,
//    .., 1, the four waves in wave order; chunks are combined in chunk order, one fused multiply-add each. Rows above one chunk
//    take two launches.
//  * cfg_scores (slam_cfg_scores): classifier-free guidance. Logits rows b and B + b (conditional, unconditional) into scores
//    row b = g (a - u) + u of their log-softmaxes, on token_logprobs' own chunk statistics (the same device functions; rows
//    above one chunk reuse its first launch over the 2 B rows). Grid (chunks, B); three separately rounded operations.
//    cfg_mirror_tokens copies the B chosen tokens behind themselves for the decode step over 2 B rows.
//  * ngram_propose (slam_ngram_propose): prompt-lookup proposals. One block per row scans the row's history once: thread t
//    takes the window ends t, t + 256, .., counts the tokens that match backwards from the end of the history, and a 64-bit
//    key (count << 32 | ~end) picks the longest match, the earliest among equals. Integers only; the two statistics by a second
//    one-block launch in a fixed order.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>

#include "../../include/slam_engine.h"
#include "common.h"

namespace slam {

// The acceptance rule of speculative decoding (include/slam_engine.h: slam_spec_accept): one block, a thread per row.
constexpr int SPEC_MAX_B = 1024;
constexpr int SPEC_MAX_K = 15;
struct SpecArgs {
  int64_t* chunk = nullptr;        // [B][K + 1]: pending token, then the K proposals; column 0 is rewritten
  const int64_t* tgt = nullptr;    // [B][K + 1]: the target's token behind every column
  int B = 0, K = 0, max_new = 0, pad_id = 0, n_eos = 0;
  const int* eos_ids = nullptr;    // device, [n_eos]
  const int* prompt_len = nullptr;
  int* n_new = nullptr;
  uint8_t* done = nullptr;
  int64_t* out = nullptr;          // [B][out_stride]
  int64_t out_stride = 0;
  int* lens_t = nullptr;
  int* lens_d = nullptr;
  int64_t* draft_ids = nullptr;    // [B][2]
  int* draft_new_lens = nullptr;
  int* tgt_new_lens = nullptr;
  int* stats = nullptr;            // [5]
};
// Prompt-lookup proposals (include/slam_engine.h: slam_ngram_propose): one block per row; a second one-block launch for stats.
constexpr int NGRAM_MAX = 16;            // longest n-gram matched (SLAM_NGRAM_MAX)
constexpr int NGRAM_MAX_STRIDE = (1 << 30) - 1;  // bound of the two strides: a history length stays an int
struct NgramArgs {
  int64_t* chunk = nullptr;         // [B][K + 1]: columns 1 .. K are written, column 0 never
  int* n_prop = nullptr;            // [B]
  int B = 0, K = 0, max_ngram = 0, fill_id = 0, n_eos = 0;
  const int64_t* prompt = nullptr;  // [B][prompt_stride], right-padded
  int64_t prompt_stride = 0;
  const int* prompt_len = nullptr;
  const int64_t* fresh = nullptr;   // [B][new_stride]: the new tokens
  int64_t new_stride = 0;
  const int* n_new = nullptr;
  const uint8_t* done = nullptr;
  const int* eos_ids = nullptr;     // device, [n_eos]
  int* stats = nullptr;             // nullable: [2]
};
// The next token of every row of fp32 logits [B][vocab] (row stride vocab, any 4-byte alignment), chosen on the device by the
// contract of include/slam_engine.h (slam_sample_tokens): one argument block from the entry point down to the launches.
struct SampleArgs {
  const float* logits = nullptr;
  int B = 0, vocab = 0;
  const uint8_t* banned = nullptr;  // nullable: [vocab], non-zero = never chosen
  int do_sample = 0, top_k = 1;     // greedy ignores top_k, temperature and top_p beyond their range checks
  float temperature = 1.f, top_p = 1.f;
  uint64_t seed = 0;
  uint32_t step = 0;
  int pad_id = 0, n_eos = 0;
  const int64_t* row_ids = nullptr;  // nullable: the Philox row id of row b (default b)
  const int* eos_ids = nullptr;      // device, [n_eos]
  uint8_t* done = nullptr;           // nullable: [B], read (finished rows emit pad_id) and set (the token is an EOS id)
  int64_t* next = nullptr;           // [B]
  int64_t* out = nullptr;            // nullable: out[b * out_stride + step] = the token
  int64_t out_stride = 0;
  const uint32_t* steps = nullptr;   // nullable: [B / group], added to step per sequence (slam_sample_tokens_at)
  int group = 1;                     // rows per sequence: row b draws with row id (b / group) at step + steps[..] + b % group
  int64_t out_col = -1;              // the column of out; negative = step
  void* ws = nullptr;                // sample_workspace_bytes(B, vocab, do_sample ? top_k : 1), 8-byte aligned
  size_t ws_bytes = 0;
  // slam_sample_tokens_warped: the second half of HF's warper chain on the ranked candidates. All four off (the defaults),
  // or greedy, takes the launches of slam_sample_tokens_at.
  float min_p = 0.f, typical_p = 1.f, epsilon_cutoff = 0.f, eta_cutoff = 0.f;
};
// scores[b][i] = -inf for the tokens row b's history bans, the bits of logits[b][i] elsewhere (include/slam_engine.h:
// slam_constrain_scores). scores may be logits: then only the bans are written.
constexpr int CONSTRAIN_MAX_SEQS = 256;      // bad word sequences (SLAM_CONSTRAIN_MAX_SEQS)
constexpr int CONSTRAIN_MAX_SEQ_LEN = 16;    // tokens per sequence (SLAM_CONSTRAIN_MAX_SEQ_LEN)
constexpr int CONSTRAIN_MAX_BEGIN = 256;     // begin_suppress ids (SLAM_CONSTRAIN_MAX_BEGIN)
constexpr int CONSTRAIN_MAX_HISTORY = 1 << 30;  // bound of step and of prompt_stride: their sum stays an int
struct ConstrainArgs {
  const float* logits = nullptr;
  float* scores = nullptr;
  int B = 0, vocab = 0;
  int step = 0, ngram = 0, n_per_prompt = 1, prompt_stride = 0;
  int ban_eos = 0, n_eos = 0, n_begin = 0, n_seqs = 0, n_seq_tokens = 0;
  const int64_t* prompt = nullptr;    // [B / n_per_prompt][prompt_stride], right-padded
  const int* prompt_len = nullptr;    // [B / n_per_prompt]
  const int64_t* fresh = nullptr;     // [B][new_stride]: the new tokens; nullable at step 0
  int64_t new_stride = 0;
  const uint8_t* done = nullptr;      // nullable: [B], non-zero = the row is copied, not edited
  const int* eos_ids = nullptr;       // [n_eos]
  const int* begin_ids = nullptr;     // [n_begin]
  const int* seq_tokens = nullptr;    // [n_seq_tokens]
  const int* seq_offsets = nullptr;   // [n_seqs + 1]
};

}  // namespace slam

namespace {

inline unsigned nblk(size_t n, int per) { return (unsigned)((n + per - 1) / per); }

// ---- speculative decoding: the acceptance rule (include/slam_engine.h: slam_spec_accept) --------------------------------------
struct SpecParams {
  int B, K, max_new, pad_id, n_eos;
  long long out_stride;
};

// one block of 1024 threads, thread b = row b. Integer work only; the five statistics go through LDS in a fixed order.
__global__ __launch_bounds__(1024) void spec_accept_kernel(int64_t* __restrict__ chunk, const int64_t* __restrict__ tgt,
                                                           const int* __restrict__ eos_ids, const int* __restrict__ prompt_len,
                                                           int* __restrict__ n_new, uint8_t* __restrict__ done,
                                                           int64_t* __restrict__ out, int* __restrict__ lens_t,
                                                           int* __restrict__ lens_d, int64_t* __restrict__ draft_ids,
                                                           int* __restrict__ draft_new_lens, int* __restrict__ tgt_new_lens,
                                                           int* __restrict__ stats, SpecParams P) {
  __shared__ int red[5][16];
  const int b = threadIdx.x, lane = b & 63;
  int live = 0, lt = 0, ld = 0, emitted = 0, accepted = 0;
  if (b < P.B) {
    int64_t* ch = chunk + (size_t)b * (P.K + 1);
    const int64_t* tg = tgt + (size_t)b * (P.K + 1);
    const int nn = min(max(n_new[b], 0), P.max_new);
    bool dn = done[b] != 0;
    int m = 0, nacc = 0;
    if (!dn) {
      while (nacc < P.K && ch[nacc + 1] == tg[nacc]) ++nacc;
      m = min(nacc + 1, P.max_new - nn);  // the budget; not positive only for a row that should have been done
      for (int i = 0; i < m; ++i) {
        bool is_eos = false;
        for (int e = 0; e < P.n_eos; ++e) is_eos = is_eos || (int64_t)eos_ids[e] == tg[i];
        if (is_eos) { m = i + 1; dn = true; break; }
      }
      if (nn + m >= P.max_new) dn = true;
      for (int i = 0; i < m; ++i) out[(long long)b * P.out_stride + nn + i] = tg[i];
      emitted = m;
      accepted = min(m, nacc);
    }
    const int lag = m == P.K + 1 ? 1 : 0;
    const int64_t last = m > 0 ? tg[m - 1] : ch[0];
    const int64_t dK = ch[P.K];
    lt = prompt_len[b] + nn + m - 1;
    ld = lt - lag;
    n_new[b] = nn + m;
    lens_t[b] = lt;
    lens_d[b] = ld;
    ch[0] = last;
    draft_ids[2 * b] = lag ? dK : last;
    draft_ids[2 * b + 1] = lag ? tg[P.K] : (int64_t)P.pad_id;
    draft_new_lens[b] = dn ? 0 : 1 + lag;
    tgt_new_lens[b] = dn ? 0 : P.K + 1;
    done[b] = dn ? 1 : 0;
    live = dn ? 0 : 1;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    live += __shfl_xor(live, o, 64);
    emitted += __shfl_xor(emitted, o, 64);
    accepted += __shfl_xor(accepted, o, 64);
    lt = max(lt, __shfl_xor(lt, o, 64));
    ld = max(ld, __shfl_xor(ld, o, 64));
  }
  if (lane == 0) {
    const int w = b >> 6;
    red[0][w] = live; red[1][w] = lt; red[2][w] = ld; red[3][w] = emitted; red[4][w] = accepted;
  }
  __syncthreads();
  if (b == 0) {
    for (int w = 1; w < 16; ++w) {
      live += red[0][w]; lt = max(lt, red[1][w]); ld = max(ld, red[2][w]); emitted += red[3][w]; accepted += red[4][w];
    }
    stats[0] = live; stats[1] = lt; stats[2] = ld; stats[3] = emitted; stats[4] = accepted;
  }
}

// ---- prompt-lookup proposals (include/slam_engine.h: slam_ngram_propose) -----------------------------------------------------
constexpr int NG_THREADS = 256;
struct NgramParams {
  int K, max_ngram, fill_id, n_eos;
  long long prompt_stride, new_stride;
};

// h[j] of a row: the prompt's real tokens, then the new ones (ConstrainHistory's layout)
struct NgramHistory {
  const int64_t* prompt;
  const int64_t* fresh;
  int pl;
  SLAM_DEVICE int64_t at(int j) const { return j < pl ? prompt[j] : fresh[j - pl]; }
};

// grid B, one block per row. back(e) = the number of j < min(max_ngram, Lh - 1, e + 1) with h[e - j] == h[Lh - 1 - j] for all
// smaller j too: a window of n tokens ending at e (e <= Lh - 2, so the tail window is none) matches the last n tokens iff
// back(e) >= n. The longest n with a match is max back(e), its earliest window the lowest such e; the proposals start at e + 1.
__global__ __launch_bounds__(NG_THREADS) void ngram_propose_kernel(int64_t* __restrict__ chunk, int* __restrict__ n_prop,
                                                                   const int64_t* __restrict__ prompt,
                                                                   const int* __restrict__ prompt_len,
                                                                   const int64_t* __restrict__ fresh,
                                                                   const int* __restrict__ n_new,
                                                                   const uint8_t* __restrict__ done,
                                                                   const int* __restrict__ eos_ids, NgramParams P) {
  __shared__ unsigned long long red[NG_THREADS / 64];
  __shared__ int stop[slam::SPEC_MAX_K + 1];
  const int b = blockIdx.x, t = threadIdx.x;
  NgramHistory h;
  h.pl = (int)min((long long)max(prompt_len[b], 0), P.prompt_stride);
  const int nn = (int)min((long long)max(n_new[b], 0), P.new_stride);
  h.prompt = prompt + (long long)b * P.prompt_stride;
  h.fresh = fresh + (long long)b * P.new_stride;  // dereferenced only for nn > 0
  const int Lh = h.pl + nn;
  unsigned long long key = 0;  // (back << 32) | ~e: larger is "longer, then earlier"; 0 = no match
  if (done[b] == 0 && Lh >= 2) {
    const int nmax = min(P.max_ngram, Lh - 1);
    for (int e = t; e < Lh - 1; e += NG_THREADS) {
      const int lim = min(nmax, e + 1);
      int back = 0;
      while (back < lim && h.at(e - back) == h.at(Lh - 1 - back)) ++back;
      if (back > 0) {
        const unsigned long long k = ((unsigned long long)back << 32) | (unsigned long long)(0xffffffffu - (uint32_t)e);
        key = k > key ? k : key;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o, 64);
    key = other > key ? other : key;
  }
  if ((t & 63) == 0) red[t >> 6] = key;
  __syncthreads();
  key = red[0];
#pragma unroll
  for (int w = 1; w < NG_THREADS / 64; ++w) key = red[w] > key ? red[w] : key;
  int start = 0, count = 0;
  if (key != 0) {
    start = (int)(0xffffffffu - (uint32_t)key) + 1;  // idx + n
    count = min(P.K, Lh - start);                    // >= 1: e <= Lh - 2
  }
  int64_t tok = P.fill_id;
  bool is_eos = false;
  if (t < count) {
    tok = h.at(start + t);
    for (int e = 0; e < P.n_eos; ++e) is_eos = is_eos || (int64_t)eos_ids[e] == tok;
  }
  if (t < P.K) stop[t] = (t < count && !is_eos) ? 0 : 1;  // the proposals end in front of column 1 + t
  __syncthreads();
  if (t < P.K) {
    int np = 0;
    while (np < P.K && !stop[np]) ++np;
    chunk[(size_t)b * (P.K + 1) + 1 + t] = t < np ? tok : (int64_t)P.fill_id;
    if (t == 0) n_prop[b] = np;
  }
}

// one block of 1024 threads, thread b = row b: { rows with a proposal, the sum of n_prop } through LDS in a fixed order
__global__ __launch_bounds__(1024) void ngram_stats_kernel(const int* __restrict__ n_prop, int B, int* __restrict__ stats) {
  __shared__ int red[2][16];
  const int b = threadIdx.x, lane = b & 63;
  int total = b < B ? n_prop[b] : 0;
  int rows = total > 0 ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    rows += __shfl_xor(rows, o, 64);
    total += __shfl_xor(total, o, 64);
  }
  if (lane == 0) { red[0][b >> 6] = rows; red[1][b >> 6] = total; }
  __syncthreads();
  if (b == 0) {
    for (int w = 1; w < 16; ++w) { rows += red[0][w]; total += red[1][w]; }
    stats[0] = rows; stats[1] = total;
  }
}


// ---- token sampling ---------------------------------------------------------------------------------------------------------
constexpr int SP_THREADS = 256;
constexpr int SP_CHUNK = 2048;   // scores per stage-1 block; rows up to this length take the single launch
constexpr int SP_MAXK = 256;     // top_k limit (SlamSampleDesc)
constexpr int SP_CACHE = 4096;   // stage-2 candidates kept in LDS; the rest are re-read from the workspace every pass
constexpr uint32_t SP_NEG_INF_KEY = 0x007fffffu;  // score_key(-inf): a candidate needs a larger key

typedef unsigned long long u64_t;

// order-preserving integer image of a score: banned / NaN -> -inf, +inf -> FLT_MAX, -0 -> +0
SLAM_DEVICE uint32_t score_key(float x, bool banned) {
  if (banned || x != x) x = -INFINITY;
  x = fminf(x, FLT_MAX);
  uint32_t u = __float_as_uint(x);
  if ((u << 1) == 0u) u = 0u;
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
SLAM_DEVICE float key_score(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

struct SampleShared {
  uint32_t hist[256];
  u64_t sel[SP_MAXK];
  float x[SP_MAXK];
  float w[SP_MAXK];
  int id[SP_MAXK];
  int red[SP_THREADS / 64];
  int bc[3];  // the selected digit, the count above it, the digit's own count
  int cnt;
};

// scores [c0, c0 + n) of one row as keys in LDS; n <= SP_CHUNK. The row may start at any 4-byte boundary: scalar loads up to
// the first 16-byte boundary, 16-byte loads from there, scalar loads for the rest.
SLAM_DEVICE void load_keys(const float* __restrict__ row, const uint8_t* __restrict__ banned, int c0, int n, uint32_t* keys) {
  const float* p = row + c0;
  const uint8_t* bn = banned ? banned + c0 : nullptr;
  int head = (int)((4u - (uint32_t)(((uintptr_t)p >> 2) & 3u)) & 3u);
  if (head > n) head = n;
  const int nv = (n - head) >> 2;
  const int t = threadIdx.x;
  if (t < head) keys[t] = score_key(p[t], bn && bn[t]);
  const float4* pv = reinterpret_cast<const float4*>(p + head);
  for (int v = t; v < nv; v += SP_THREADS) {
    const float4 f = pv[v];
    const int i = head + 4 * v;
    keys[i + 0] = score_key(f.x, bn && bn[i + 0]);
    keys[i + 1] = score_key(f.y, bn && bn[i + 1]);
    keys[i + 2] = score_key(f.z, bn && bn[i + 2]);
    keys[i + 3] = score_key(f.w, bn && bn[i + 3]);
  }
  for (int i = head + 4 * nv + t; i < n; i += SP_THREADS) keys[i] = score_key(p[i], bn && bn[i]);
}

// composites of a chunk held as keys in LDS
struct KeySrc {
  const uint32_t* keys;
  int base, idbits;
  uint32_t idmask;
  SLAM_DEVICE u64_t operator()(int i) const { return ((u64_t)keys[i] << idbits) | (u64_t)(idmask - (uint32_t)(base + i)); }
};
// composites that stage 1 wrote: the first ncache from LDS, the rest from the workspace
struct PairSrc {
  const u64_t* cache;
  const u64_t* g;
  int ncache;
  SLAM_DEVICE u64_t operator()(int i) const { return i < ncache ? cache[i] : g[i]; }
};

// The min(k, candidates) largest composites of src(0 .. n) into sh.sel, in no particular order; returns their number.
// Every thread of the block calls it (barriers inside); the result is the same set whatever the order of the items.
template <class Src>
SLAM_DEVICE int select_topk(const Src& src, int n, int k, int idbits, SampleShared& sh) {
  const int t = threadIdx.x, lane = t & 63;
  const u64_t lowest = ((u64_t)SP_NEG_INF_KEY + 1) << idbits;  // candidates are >= this
  int c = 0;
  for (int i = t; i < n; i += SP_THREADS) c += src(i) >= lowest ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if (lane == 0) sh.red[t >> 6] = c;
  if (t == 0) sh.cnt = 0;
  __syncthreads();
  int nvalid = 0;
#pragma unroll
  for (int w = 0; w < SP_THREADS / 64; ++w) nvalid += sh.red[w];
  const int kk = k < nvalid ? k : nvalid;
  if (kk == 0) return 0;
  const int npass = (32 + idbits + 7) / 8;
  u64_t prefix = 0, mask = 0;
  int remaining = kk;
  for (int p = 0; p < npass; ++p) {
    const int shift = 8 * (npass - 1 - p);
    sh.hist[t] = 0;
    __syncthreads();
    for (int i = t; i < n; i += SP_THREADS) {
      const u64_t v = src(i);
      if (v >= lowest && (v & mask) == prefix) atomicAdd(&sh.hist[(uint32_t)(v >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (t < 64) {  // bins from the top: the first one at which the running count reaches `remaining`
      int s[4], local = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) { s[j] = (int)sh.hist[255 - (4 * lane + j)]; local += s[j]; }
      int incl = local;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
      }
      int run = incl - local;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (run < remaining && run + s[j] >= remaining) { sh.bc[0] = 255 - (4 * lane + j); sh.bc[1] = run; sh.bc[2] = s[j]; }
        run += s[j];
      }
    }
    __syncthreads();
    prefix |= (u64_t)sh.bc[0] << shift;
    mask |= (u64_t)255 << shift;
    remaining -= sh.bc[1];
    if (sh.bc[2] == remaining) break;  // the whole bin is in: (v & mask) >= prefix is the selection
  }
  for (int i = t; i < n; i += SP_THREADS) {
    const u64_t v = src(i);
    if (v >= lowest && (v & mask) >= prefix) {
      const int slot = atomicAdd(&sh.cnt, 1);
      if (slot < SP_MAXK) sh.sel[slot] = v;
    }
  }
  __syncthreads();
  return kk;
}

struct SampleParams {
  int do_sample, k, vocab, idbits, nch, pad_id, n_eos;
  float inv_t, top_p;
  uint32_t k0, k1, step;
  long long out_stride, out_col;
  int group;  // rows per sequence: row b is column b % group of sequence b / group (slam_sample_tokens_at)
};

SLAM_DEVICE void emit_token(long long tok, bool mark, int b, const SampleParams& P, const int* eos_ids, uint8_t* done,
                            int64_t* next, int64_t* out) {
  next[b] = tok;
  if (out) out[(long long)b * P.out_stride + P.out_col] = tok;
  if (mark && done)
    for (int e = 0; e < P.n_eos; ++e)
      if (eos_ids[e] == (int)tok) { done[b] = 1; break; }
}

// stage 1, grid (chunks, B): the chunk's top k as composites into ws[b][chunk][k], unused slots 0 (no candidate)
__global__ __launch_bounds__(SP_THREADS) void sample_select_kernel(const float* __restrict__ logits,
                                                                   const uint8_t* __restrict__ banned,
                                                                   const uint8_t* __restrict__ done, SampleParams P,
                                                                   u64_t* __restrict__ ws) {
  __shared__ uint32_t keys[SP_CHUNK];
  __shared__ SampleShared sh;
  const int ch = blockIdx.x, b = blockIdx.y;
  if (done && done[b]) return;
  const int c0 = ch * SP_CHUNK;
  const int n = min(SP_CHUNK, P.vocab - c0);
  load_keys(logits + (size_t)b * P.vocab, banned, c0, n, keys);
  __syncthreads();
  const KeySrc src{keys, c0, P.idbits, (1u << P.idbits) - 1u};
  const int kk = select_topk(src, n, P.k, P.idbits, sh);
  u64_t* dst = ws + ((size_t)b * P.nch + ch) * P.k;
  for (int i = threadIdx.x; i < P.k; i += SP_THREADS) dst[i] = i < kk ? sh.sel[i] : 0ull;
}

// slam_sample_tokens_warped: the description of the plain call, then min_p / typical_p / epsilon_cutoff / eta_cutoff
struct WarpSampleParams : SampleParams {
  float min_p, typical_p, eps_cut, eta_cut;
};
template <bool WARP> struct SampleParamsOf { typedef SampleParams type; };
template <> struct SampleParamsOf<true> { typedef WarpSampleParams type; };

// LDS of the warper chain; a thread owns the rank of its index. The float arrays are read 16 bytes at a time.
struct alignas(16) WarpShared {
  float kw[SP_MAXK];    // w_j of the ranks in S, 0 for the others (adding 0 keeps the bits of a sum over S in rank order)
  float term[SP_MAXK];  // p_j log p_j of the ranks in S with w_j > 0, 0 for the others
  float s[SP_MAXK];     // typical_p: s_j of the ranks in S, NaN for the others (a NaN never counts as "in front")
  float op[SP_MAXK];    // typical_p: p in the (s, rank) order
  float os[SP_MAXK];    // typical_p: s in that order
  u64_t mask[SP_THREADS / 64];  // membership of S, a bit per rank
  float Z, logZ, H, cut;
  int n, top, last;     // |S|, its lowest and its highest rank
};

// a[0] + a[1] + .. + a[n - 1] in that order from 0.0f, on one thread. a is zero behind n up to the next multiple of 4 (x + 0
// is x): 16-byte LDS loads and no branch, so the loads run ahead of the dependent adds.
SLAM_DEVICE float seq_sum(const float* a, int n) {
  const float4* v = reinterpret_cast<const float4*>(a);
  float s = 0.f;
#pragma unroll 8
  for (int i = 0; i < (n + 3) >> 2; ++i) {
    const float4 f = v[i];
    s += f.x;
    s += f.y;
    s += f.z;
    s += f.w;
  }
  return s;
}

// Z_S and log Z_S, summed by thread 0 in rank order, |S| and the lowest and highest rank of S from the waves' ballots; every
// thread of the block calls it with its own rank's membership and weight (barriers inside).
SLAM_DEVICE void warp_normaliser(WarpShared& wsh, int kk, bool in, float w) {
  const int t = threadIdx.x;
  wsh.kw[t] = in ? w : 0.f;
  const u64_t m = __ballot(in);
  if ((t & 63) == 0) wsh.mask[t >> 6] = m;
  __syncthreads();
  if (t == 0) {
    const float z = seq_sum(wsh.kw, kk);
    int n = 0, top = -1, last = 0;
#pragma unroll
    for (int v = 0; v < SP_THREADS / 64; ++v) {
      const u64_t b = wsh.mask[v];
      if (b) {
        n += __popcll(b);
        if (top < 0) top = 64 * v + __ffsll((long long)b) - 1;
        last = 64 * v + 63 - __clzll((long long)b);
      }
    }
    wsh.Z = z;
    wsh.logZ = logf(z);
    wsh.n = n;
    wsh.top = top < 0 ? 0 : top;
    wsh.last = last;
  }
  __syncthreads();
}

// H_S behind warp_normaliser: -(sum of p_j log p_j over S, w_j > 0) in rank order on thread 0. p, lp: this rank's.
SLAM_DEVICE void warp_entropy(WarpShared& wsh, int kk, bool in, float w, float p, float lp) {
  const int t = threadIdx.x;
  wsh.term[t] = (in && w > 0.f) ? p * lp : 0.f;
  __syncthreads();
  if (t == 0) wsh.H = -seq_sum(wsh.term, kk);
  __syncthreads();
}

// one block per row. ROW: the whole row (vocab <= SP_CHUNK) is selected here; else the candidates of stage 1.
// WARP: the warper chain of slam_sample_tokens_warped between the top-p prefix and the draw (sampling only).
template <bool ROW, bool WARP = false>
__global__ __launch_bounds__(SP_THREADS) void sample_finish_kernel(const float* __restrict__ logits,
                                                                   const uint8_t* __restrict__ banned,
                                                                   const int64_t* __restrict__ row_ids,
                                                                   const int* __restrict__ eos_ids, uint8_t* __restrict__ done,
                                                                   int64_t* __restrict__ next, int64_t* __restrict__ out,
                                                                   typename SampleParamsOf<WARP>::type P,
                                                                   const u64_t* __restrict__ ws,
                                                                   const uint32_t* __restrict__ steps) {
  __shared__ u64_t buf[ROW ? SP_CHUNK / 2 : SP_CACHE];
  __shared__ SampleShared sh;
  const int b = blockIdx.x, t = threadIdx.x;
  if (done && done[b]) {
    if (t == 0) emit_token(P.pad_id, false, b, P, eos_ids, done, next, out);
    return;
  }
  int kk;
  if (ROW) {
    uint32_t* keys = reinterpret_cast<uint32_t*>(buf);
    load_keys(logits + (size_t)b * P.vocab, banned, 0, P.vocab, keys);
    __syncthreads();
    const KeySrc src{keys, 0, P.idbits, (1u << P.idbits) - 1u};
    kk = select_topk(src, P.vocab, P.k, P.idbits, sh);
  } else {
    const int n = P.nch * P.k;
    const u64_t* g = ws + (size_t)b * n;
    const int ncache = n < SP_CACHE ? n : SP_CACHE;
    for (int i = t; i < ncache; i += SP_THREADS) buf[i] = g[i];
    __syncthreads();
    const PairSrc src{buf, g, ncache};
    kk = select_topk(src, n, P.k, P.idbits, sh);
  }
  if (kk == 0) {  // no finite score: pad, the row is not marked done
    if (t == 0) emit_token(P.pad_id, false, b, P, eos_ids, done, next, out);
    return;
  }
  // rank j = how many of the k' composites are larger: (score descending, id ascending)
  const uint32_t idmask = (1u << P.idbits) - 1u;
  if (t < kk) {
    const u64_t v = sh.sel[t];
    int r = 0;
    for (int j = 0; j < kk; ++j) r += sh.sel[j] > v ? 1 : 0;
    sh.x[r] = key_score((uint32_t)(v >> P.idbits));
    sh.id[r] = (int)(idmask - ((uint32_t)v & idmask));
  }
  __syncthreads();
  if (!P.do_sample) {
    if (t == 0) emit_token(sh.id[0], true, b, P, eos_ids, done, next, out);
    return;
  }
  if (t < kk) sh.w[t] = t == 0 ? 1.0f : expf((sh.x[t] - sh.x[0]) * P.inv_t);
  __syncthreads();
  if constexpr (WARP) {
    __shared__ WarpShared wsh;
    if (t == 0) {  // the top-p prefix, as in the plain kernel below
      int m = kk;
      if (P.top_p < 1.0f) {
        float tail = 0.f;
        for (int j = kk - 1; j >= 0; --j) tail += sh.w[j];
        const float thr = (1.0f - P.top_p) * tail;
        tail = 0.f;
        for (int j = kk - 1; j > 0; --j) {
          tail += sh.w[j];
          if (tail <= thr) m = j;
          else break;
        }
      }
      wsh.n = m;
    }
    __syncthreads();
    // thread t owns rank t: its membership of S, its scaled score a, weight w and score x
    const bool cand = t < kk;
    bool in = t < wsh.n;
    const float x = cand ? sh.x[t] : 0.f;
    const float a = (cand && t > 0) ? (x - sh.x[0]) * P.inv_t : 0.f;
    const float w = cand ? sh.w[t] : 0.f;
    if (P.min_p > 0.f) {  // S is a prefix: its lowest rank is 0
      if (in && w < P.min_p * sh.w[0]) in = false;
    }
    if (P.typical_p < 1.0f) {
      warp_normaliser(wsh, kk, in, w);
      const float p = w / wsh.Z, lp = a - wsh.logZ;
      warp_entropy(wsh, kk, in, w, p, lp);
      const float s = fabsf(-lp - wsh.H);
      wsh.s[t] = in ? s : __uint_as_float(0x7fc00000u);
      __syncthreads();
      if (in) {  // position in the (s ascending, rank ascending) order = the number of ranks of S in front
        const float4* sv = reinterpret_cast<const float4*>(wsh.s);
        int pos = 0;
        for (int i = 0; i < (kk + 3) >> 2; ++i) {
          const float4 f = sv[i];
          const int j = 4 * i;
          pos += (f.x < s || (f.x == s && j + 0 < t)) ? 1 : 0;
          pos += (f.y < s || (f.y == s && j + 1 < t)) ? 1 : 0;
          pos += (f.z < s || (f.z == s && j + 2 < t)) ? 1 : 0;
          pos += (f.w < s || (f.w == s && j + 3 < t)) ? 1 : 0;
        }
        wsh.op[pos] = p;
        wsh.os[pos] = s;
      }
      __syncthreads();
      if (t == 0) {  // c_i is non-decreasing: #{c_i < mass} is the first i with c_i >= mass; no branch, as in seq_sum
        const float4* pv = reinterpret_cast<const float4*>(wsh.op);
        const int n = wsh.n;
        int last = n - 1;
        bool found = false;
        float c = 0.f;
#pragma unroll 4
        for (int i = 0; i < (n + 3) >> 2; ++i) {
          const float4 f = pv[i];
          const float e[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            c += e[q];
            const bool hit = !found && 4 * i + q < n && !(c < P.typical_p);
            last = hit ? 4 * i + q : last;
            found = found || hit;
          }
        }
        wsh.cut = wsh.os[last];
      }
      __syncthreads();
      if (in && s > wsh.cut) in = false;
    }
    if (P.eps_cut > 0.f) {
      warp_normaliser(wsh, kk, in, w);
      const float p = w / wsh.Z;
      if (in && p < P.eps_cut && x != sh.x[wsh.top]) in = false;
    }
    if (P.eta_cut > 0.f) {
      warp_normaliser(wsh, kk, in, w);
      const float p = w / wsh.Z, lp = a - wsh.logZ;
      warp_entropy(wsh, kk, in, w, p, lp);
      const float eta = fminf(P.eta_cut, sqrtf(P.eta_cut) * expf(-wsh.H));
      if (in && p < eta && x != sh.x[wsh.top]) in = false;
    }
    warp_normaliser(wsh, kk, in, w);  // total = Z of the final S: the same adds in the same order as cum below
    if (t != 0) return;
    const float total = wsh.Z;
    const int q = b / P.group;
    const uint64_t r = row_ids ? (uint64_t)row_ids[q] : (uint64_t)q;
    const uint32_t step = P.step + (steps ? steps[q] : 0u) + (uint32_t)(b - q * P.group);
    const Philox4 rnd = philox4x32_10((uint32_t)r, step, (uint32_t)(r >> 32), 0x53414D50u, P.k0, P.k1);
    const float u = (float)(rnd.w[0] >> 8) * 5.9604644775390625e-08f;  // 2^-24
    const float target = u * total;
    // cum stands still on a rank outside S (its kw is 0), so the first rank with cum > target is in S
    const float4* wv = reinterpret_cast<const float4*>(wsh.kw);
    const int last = wsh.last;
    int pick = -1;
    float cum = 0.f;
#pragma unroll 4
    for (int i = 0; i < (kk + 3) >> 2; ++i) {
      const float4 f = wv[i];
      const float e[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        cum += e[c];
        pick = (pick < 0 && cum > target) ? 4 * i + c : pick;
      }
    }
    emit_token(sh.id[pick < 0 ? last : pick], true, b, P, eos_ids, done, next, out);
    return;
  }
  if (t != 0) return;
  int m = kk;
  if (P.top_p < 1.0f) {
    float tail = 0.f;
    for (int j = kk - 1; j >= 0; --j) tail += sh.w[j];
    const float thr = (1.0f - P.top_p) * tail;
    tail = 0.f;
    for (int j = kk - 1; j > 0; --j) {
      tail += sh.w[j];
      if (tail <= thr) m = j;  // tail grows towards rank 0: the dropped ranks are a suffix
      else break;
    }
  }
  float total = 0.f;
  for (int j = 0; j < m; ++j) total += sh.w[j];
  const int q = b / P.group;  // the row's sequence; group = 1 and steps = NULL are slam_sample_tokens
  const uint64_t r = row_ids ? (uint64_t)row_ids[q] : (uint64_t)q;
  const uint32_t step = P.step + (steps ? steps[q] : 0u) + (uint32_t)(b - q * P.group);
  const Philox4 rnd = philox4x32_10((uint32_t)r, step, (uint32_t)(r >> 32), 0x53414D50u, P.k0, P.k1);
  const float u = (float)(rnd.w[0] >> 8) * 5.9604644775390625e-08f;  // 2^-24
  const float target = u * total;
  int pick = m - 1;
  float cum = 0.f;
  for (int j = 0; j < m; ++j) {
    cum += sh.w[j];
    if (cum > target) { pick = j; break; }
  }
  emit_token(sh.id[pick], true, b, P, eos_ids, done, next, out);
}

// ---- log-probability of a token -----------------------------------------------------------------------------------------------
// NaN -> -inf, +inf -> FLT_MAX: the sampler's reading of a score
SLAM_DEVICE float clean_score(float x) {
  if (x != x) x = -INFINITY;
  return fminf(x, FLT_MAX);
}

// scores [c0, c0 + n) of one row, cleaned, into LDS at their index in the chunk; the loads are those of load_keys
SLAM_DEVICE void load_scores(const float* __restrict__ row, int c0, int n, float* vals) {
  const float* p = row + c0;
  int head = (int)((4u - (uint32_t)(((uintptr_t)p >> 2) & 3u)) & 3u);
  if (head > n) head = n;
  const int nv = (n - head) >> 2;
  const int t = threadIdx.x;
  if (t < head) vals[t] = clean_score(p[t]);
  const float4* pv = reinterpret_cast<const float4*>(p + head);
  for (int v = t; v < nv; v += SP_THREADS) {
    const float4 f = pv[v];
    const int i = head + 4 * v;
    vals[i + 0] = clean_score(f.x);
    vals[i + 1] = clean_score(f.y);
    vals[i + 2] = clean_score(f.z);
    vals[i + 3] = clean_score(f.w);
  }
  for (int i = head + 4 * nv + t; i < n; i += SP_THREADS) vals[i] = clean_score(p[i]);
}

// m = max of vals[0 .. n), s = sum of expf(vals[i] - m) in the stated order (0 when m is -inf). Every thread of the block calls
// it and gets the same pair.
SLAM_DEVICE void chunk_max_sum(const float* vals, int n, float* red, float& m, float& s) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  float mx = -INFINITY;
  for (int i = t; i < n; i += SP_THREADS) mx = fmaxf(mx, vals[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float acc = 0.f;
  if (m != -INFINITY)
    for (int i = t; i < n; i += SP_THREADS) acc += expf(vals[i] - m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  s = ((red[0] + red[1]) + red[2]) + red[3];
}

// (m, S) of a row from stage 1's pairs p[0 .. nch), in chunk order. One thread calls it.
SLAM_DEVICE void combine_chunks(const float2* p, int nch, float& m, float& s) {
  m = -INFINITY;
  s = 0.f;
  for (int c = 0; c < nch; ++c) m = fmaxf(m, p[c].x);
  if (m != -INFINITY)
    for (int c = 0; c < nch; ++c)
      if (p[c].x != -INFINITY) s = __fmaf_rn(p[c].y, expf(p[c].x - m), s);  // one rounding, as the header states
}

struct LogprobParams {
  int vocab, nch, column;
  long long out_stride;
};

// stage 1, grid (chunks, B): (m_c, s_c) of the chunk into ws[b][chunk]
__global__ __launch_bounds__(SP_THREADS) void logprob_chunk_kernel(const float* __restrict__ logits,
                                                                   const uint8_t* __restrict__ finished, LogprobParams P,
                                                                   float2* __restrict__ ws) {
  __shared__ float vals[SP_CHUNK];
  __shared__ float red[SP_THREADS / 64];
  const int ch = blockIdx.x, b = blockIdx.y;
  if (finished && finished[b]) return;  // written by the second launch only
  const int c0 = ch * SP_CHUNK;
  const int n = min(SP_CHUNK, P.vocab - c0);
  load_scores(logits + (size_t)b * P.vocab, c0, n, vals);
  __syncthreads();
  float m, s;
  chunk_max_sum(vals, n, red, m, s);
  if (threadIdx.x == 0) ws[(size_t)b * P.nch + ch] = make_float2(m, s);
}

// one block per row. ROW: the row is one chunk, reduced here (SP_THREADS threads); else thread 0 combines stage 1's pairs.
template <bool ROW>
__global__ __launch_bounds__(SP_THREADS) void logprob_finish_kernel(const float* __restrict__ logits,
                                                                    const int64_t* __restrict__ tokens,
                                                                    const uint8_t* __restrict__ done,
                                                                    uint8_t* __restrict__ finished, float* __restrict__ out,
                                                                    LogprobParams P, const float2* __restrict__ ws) {
  __shared__ float vals[ROW ? SP_CHUNK : 1];
  __shared__ float red[SP_THREADS / 64];
  __shared__ int fin_s;
  const int b = blockIdx.x, t = threadIdx.x;
  if (t == 0) fin_s = finished && finished[b] ? 1 : 0;  // one read: thread 0 rewrites the flag below
  __syncthreads();
  const bool fin = fin_s != 0;
  const float* row = logits + (size_t)b * P.vocab;
  float m = -INFINITY, s = 0.f;
  if (!fin) {
    if (ROW) {
      load_scores(row, 0, P.vocab, vals);
      __syncthreads();
      chunk_max_sum(vals, P.vocab, red, m, s);
    } else if (t == 0) {
      combine_chunks(ws + (size_t)b * P.nch, P.nch, m, s);
    }
  }
  if (t != 0) return;
  float r = 0.f;
  if (!fin) {
    const long long tok = tokens[b];
    if (tok >= 0 && tok < P.vocab) r = m == -INFINITY ? -INFINITY : clean_score(row[tok]) - (m + logf(s));
  }
  out[(long long)b * P.out_stride + P.column] = r;
  if (finished) finished[b] = done ? done[b] : (uint8_t)0;
}

// ---- classifier-free guidance (slam_cfg_scores) --------------------------------------------------------------------------------
// One guided score from the cleaned pair (x, y) and the rows' log-normalisers. x_dead / y_dead: the row has no score above -inf.
// Three operations, each rounded on its own: a fused multiply-add would round g d + u once and change the bits.
SLAM_DEVICE float cfg_combine(float x, float y, float Lx, float Ly, float g, bool x_dead, bool y_dead) {
#pragma clang fp contract(off)
  if (x_dead) return -INFINITY;
  const float a = x - Lx;
  if (a == -INFINITY) return -INFINITY;
  if (y_dead) return a;
  const float u = y - Ly;
  if (u == -INFINITY) return a;
  const float d = a - u;
  const float gd = g * d;
  return gd + u;
}

struct CfgParams {
  int vocab, nch, B;
  float g;
};

// grid (chunks, B). Row b (x) and row B + b (y) of logits, chunk blockIdx.x, into scores row b. ROW: the rows are one chunk and
// their statistics are formed here; else thread 0 (x) and thread 64 (y) combine the pairs logprob_chunk_kernel left in ws for
// the 2 B rows. The chunk of both rows is staged in LDS by load_scores (16-byte loads from each row's own first 16-byte
// boundary) and leaves by 16-byte stores from the first 16-byte boundary of the scores row, 4-byte ones at the ragged ends.
template <bool ROW>
__global__ __launch_bounds__(SP_THREADS) void cfg_scores_kernel(const float* __restrict__ logits, float* __restrict__ scores,
                                                                CfgParams P, const float2* __restrict__ ws) {
  __shared__ float vx[SP_CHUNK];
  __shared__ float vy[SP_CHUNK];
  __shared__ float red[SP_THREADS / 64];
  __shared__ float st[4];
  const int ch = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const int c0 = ch * SP_CHUNK;
  const int n = min(SP_CHUNK, P.vocab - c0);
  load_scores(logits + (size_t)b * P.vocab, c0, n, vx);
  load_scores(logits + (size_t)(P.B + b) * P.vocab, c0, n, vy);
  __syncthreads();
  float mx, sx, my, sy;
  if (ROW) {
    chunk_max_sum(vx, n, red, mx, sx);
    __syncthreads();  // red is reused
    chunk_max_sum(vy, n, red, my, sy);
  } else {
    if (t == 0) combine_chunks(ws + (size_t)b * P.nch, P.nch, st[0], st[1]);
    if (t == 64) combine_chunks(ws + (size_t)(P.B + b) * P.nch, P.nch, st[2], st[3]);
    __syncthreads();
    mx = st[0], sx = st[1], my = st[2], sy = st[3];
  }
  const bool x_dead = mx == -INFINITY, y_dead = my == -INFINITY;
  const float Lx = mx + logf(sx), Ly = my + logf(sy);  // unused when the row is dead
  const float g = P.g;
  float* dst = scores + (size_t)b * P.vocab + c0;
  int head = (int)((4u - (uint32_t)(((uintptr_t)dst >> 2) & 3u)) & 3u);
  if (head > n) head = n;
  const int nv = (n - head) >> 2;
  if (t < head) dst[t] = cfg_combine(vx[t], vy[t], Lx, Ly, g, x_dead, y_dead);
  float4* dv = reinterpret_cast<float4*>(dst + head);
  for (int v = t; v < nv; v += SP_THREADS) {
    const int i = head + 4 * v;
    float4 f;
    f.x = cfg_combine(vx[i + 0], vy[i + 0], Lx, Ly, g, x_dead, y_dead);
    f.y = cfg_combine(vx[i + 1], vy[i + 1], Lx, Ly, g, x_dead, y_dead);
    f.z = cfg_combine(vx[i + 2], vy[i + 2], Lx, Ly, g, x_dead, y_dead);
    f.w = cfg_combine(vx[i + 3], vy[i + 3], Lx, Ly, g, x_dead, y_dead);
    dv[v] = f;
  }
  for (int i = head + 4 * nv + t; i < n; i += SP_THREADS) dst[i] = cfg_combine(vx[i], vy[i], Lx, Ly, g, x_dead, y_dead);
}

// next[B + b] = next[b]: the unconditional twins decode the token their conditional row drew
__global__ __launch_bounds__(256) void cfg_mirror_kernel(int64_t* next, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < B) next[B + b] = next[b];
}

// ---- per-row bans between the logits and the token choice (slam_constrain_scores) -------------------------------------------
// grid (chunks of SP_CHUNK, B). The block copies its chunk of the row bit for bit (skipped in place), then scans the row's
// history and stores -inf for the bans that fall inside its own chunk: no block writes into another's chunk, so there is no
// ordering between blocks, and the only stores behind the copy are of one constant (equal stores may race, harmlessly).
struct ConstrainParams {
  int vocab, step, ngram, n_per_prompt, prompt_stride, ban_eos, n_eos, n_begin, n_seqs, n_seq_tokens;
  long long new_stride;
};

// h[j] of a row: the prompt's real tokens, then the new ones
struct ConstrainHistory {
  const int64_t* prompt;
  const int64_t* fresh;
  int pl;
  SLAM_DEVICE long long at(int j) const { return j < pl ? prompt[j] : fresh[j - pl]; }
};

__global__ __launch_bounds__(SP_THREADS) void constrain_scores_kernel(
    const float* logits, float* scores, const int64_t* __restrict__ prompt, const int* __restrict__ prompt_len,
    const int64_t* __restrict__ fresh, const uint8_t* __restrict__ done, const int* __restrict__ eos_ids,
    const int* __restrict__ begin_ids, const int* __restrict__ seq_tokens, const int* __restrict__ seq_offsets,
    ConstrainParams P) {
  const int ch = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const int c0 = ch * SP_CHUNK;
  const int n = min(SP_CHUNK, P.vocab - c0);
  float* srow = scores + (size_t)b * P.vocab;
  if (logits != scores) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(logits + (size_t)b * P.vocab + c0);
    uint32_t* dst = reinterpret_cast<uint32_t*>(srow + c0);
    int head = 0, nv = 0;
    if ((((uintptr_t)src ^ (uintptr_t)dst) & 15) == 0) {  // equally aligned: 16-byte body, 4-byte ragged ends
      head = (int)((4u - (uint32_t)(((uintptr_t)src >> 2) & 3u)) & 3u);
      if (head > n) head = n;
      nv = (n - head) >> 2;
    }
    if (t < head) dst[t] = src[t];
    const uint4* sv = reinterpret_cast<const uint4*>(src + head);
    uint4* dv = reinterpret_cast<uint4*>(dst + head);
    for (int v = t; v < nv; v += SP_THREADS) dv[v] = sv[v];
    for (int i = head + 4 * nv + t; i < n; i += SP_THREADS) dst[i] = src[i];
    __syncthreads();  // the bans below land on words other threads of this block copied
  }
  if (done && done[b]) return;
  const int pb = b / P.n_per_prompt;
  ConstrainHistory h;
  h.pl = min(max(prompt_len[pb], 0), P.prompt_stride);
  h.prompt = prompt + (size_t)pb * P.prompt_stride;
  h.fresh = fresh + (long long)b * P.new_stride;  // dereferenced only for step > 0
  const int Lh = h.pl + P.step;
  const long long lo = c0, hi = c0 + n;  // a ban outside [lo, hi) is another block's, or nobody's
  const int ng = P.ngram;
  if (ng > 0 && Lh >= ng) {
    const int p0 = Lh - ng + 1;  // the last ng - 1 tokens
    for (int j = t; j <= Lh - ng; j += SP_THREADS) {
      bool eq = true;
      for (int k = 0; k < ng - 1 && eq; ++k) eq = h.at(j + k) == h.at(p0 + k);
      if (!eq) continue;
      const long long tok = h.at(j + ng - 1);
      if (tok >= lo && tok < hi) srow[tok] = -INFINITY;
    }
  }
  for (int i = t; i < P.n_seqs; i += SP_THREADS) {
    const int o0 = seq_offsets[i], o1 = seq_offsets[i + 1];
    if (o0 < 0 || o1 > P.n_seq_tokens || o1 - o0 < 2 || o1 - o0 > slam::CONSTRAIN_MAX_SEQ_LEN) continue;
    const int Lw = o1 - o0;
    if (Lw > Lh) continue;
    bool eq = true;
    for (int k = 0; k < Lw - 1 && eq; ++k) eq = h.at(Lh - (Lw - 1) + k) == (long long)seq_tokens[o0 + k];
    if (!eq) continue;
    const long long tok = seq_tokens[o1 - 1];
    if (tok >= lo && tok < hi) srow[tok] = -INFINITY;
  }
  if (P.ban_eos && t < P.n_eos) {
    const long long tok = eos_ids[t];
    if (tok >= lo && tok < hi) srow[tok] = -INFINITY;
  }
  if (P.step == 0)
    for (int i = t; i < P.n_begin; i += SP_THREADS) {
      const long long tok = begin_ids[i];
      if (tok >= lo && tok < hi) srow[tok] = -INFINITY;
    }
}

}  // namespace

namespace slam {

int spec_accept(const SpecArgs& a, hipStream_t st) {
  if (!a.chunk || !a.tgt || !a.prompt_len || !a.n_new || !a.done || !a.out || !a.lens_t || !a.lens_d || !a.draft_ids ||
      !a.draft_new_lens || !a.tgt_new_lens || !a.stats)
    return -1;
  if (a.B < 1 || a.B > SPEC_MAX_B || a.K < 1 || a.K > SPEC_MAX_K || a.n_eos < 0 || a.n_eos > 16 || (a.n_eos > 0 && !a.eos_ids))
    return -1;
  if (a.max_new < 1 || a.out_stride < a.max_new) return -1;
  SpecParams P;
  P.B = a.B;
  P.K = a.K;
  P.max_new = a.max_new;
  P.pad_id = a.pad_id;
  P.n_eos = a.n_eos;
  P.out_stride = a.out_stride;
  spec_accept_kernel<<<1, 1024, 0, st>>>(a.chunk, a.tgt, a.eos_ids, a.prompt_len, a.n_new, a.done, a.out, a.lens_t, a.lens_d,
                                          a.draft_ids, a.draft_new_lens, a.tgt_new_lens, a.stats, P);
  return (int)hipGetLastError();
}

int ngram_propose(const NgramArgs& a, hipStream_t st) {
  if (!a.chunk || !a.n_prop || !a.prompt || !a.prompt_len || !a.fresh || !a.n_new || !a.done) return -1;
  if (a.B < 1 || a.B > SPEC_MAX_B || a.K < 1 || a.K > SPEC_MAX_K || a.max_ngram < 1 || a.max_ngram > NGRAM_MAX) return -1;
  if (a.n_eos < 0 || a.n_eos > 16 || (a.n_eos > 0 && !a.eos_ids)) return -1;
  if (a.prompt_stride < 0 || a.prompt_stride > NGRAM_MAX_STRIDE || a.new_stride < 0 || a.new_stride > NGRAM_MAX_STRIDE) return -1;
  NgramParams P;
  P.K = a.K;
  P.max_ngram = a.max_ngram;
  P.fill_id = a.fill_id;
  P.n_eos = a.n_eos;
  P.prompt_stride = a.prompt_stride;
  P.new_stride = a.new_stride;
  ngram_propose_kernel<<<a.B, NG_THREADS, 0, st>>>(a.chunk, a.n_prop, a.prompt, a.prompt_len, a.fresh, a.n_new, a.done,
                                                   a.eos_ids, P);
  if (a.stats) ngram_stats_kernel<<<1, 1024, 0, st>>>(a.n_prop, a.B, a.stats);
  return (int)hipGetLastError();
}


static int sample_chunks(int vocab) { return (vocab + SP_CHUNK - 1) / SP_CHUNK; }

size_t sample_workspace_bytes(int B, int vocab, int top_k) {
  if (B <= 0 || vocab <= 0) return 0;
  const int k = top_k < 1 ? 1 : top_k;
  return (size_t)B * sample_chunks(vocab) * k * sizeof(u64_t);
}

int sample_tokens(const SampleArgs& a, hipStream_t st) {
  if (!a.logits || !a.next || a.B <= 0 || a.B > 65535 || a.vocab <= 0 || ((uintptr_t)a.logits & 3)) return -1;
  const int k = a.do_sample ? a.top_k : 1;
  if (k < 1 || k > SP_MAXK || !(a.temperature > 0.f) || !(a.top_p > 0.f) || a.top_p > 1.f) return -1;
  if (a.n_eos < 0 || (a.n_eos > 0 && !a.eos_ids)) return -1;
  if (a.group < 1 || a.B % a.group != 0) return -1;
  if (!a.ws || ((uintptr_t)a.ws & 7) || a.ws_bytes < sample_workspace_bytes(a.B, a.vocab, k)) return -1;
  // the negated forms refuse NaN
  if (!(a.min_p >= 0.f && a.min_p <= 1.f) || !(a.typical_p > 0.f && a.typical_p <= 1.f)) return -1;
  if (!(a.epsilon_cutoff >= 0.f && a.epsilon_cutoff < 1.f) || !(a.eta_cutoff >= 0.f && a.eta_cutoff < 1.f)) return -1;
  const bool warped = a.do_sample && (a.min_p > 0.f || a.typical_p < 1.f || a.epsilon_cutoff > 0.f || a.eta_cutoff > 0.f);
  WarpSampleParams P;
  P.min_p = a.min_p;
  P.typical_p = a.typical_p;
  P.eps_cut = a.epsilon_cutoff;
  P.eta_cut = a.eta_cutoff;
  P.do_sample = a.do_sample ? 1 : 0;
  P.k = k;
  P.vocab = a.vocab;
  P.idbits = 1;
  while (P.idbits < 31 && (1u << P.idbits) < (uint32_t)a.vocab) ++P.idbits;
  P.nch = sample_chunks(a.vocab);
  P.pad_id = a.pad_id;
  P.n_eos = a.n_eos;
  P.inv_t = 1.0f / a.temperature;
  P.top_p = a.top_p;
  P.k0 = (uint32_t)a.seed;
  P.k1 = (uint32_t)(a.seed >> 32);
  P.step = a.step;
  P.out_stride = a.out_stride;
  P.out_col = a.out_col >= 0 ? a.out_col : (long long)a.step;
  P.group = a.group;
  u64_t* ws = reinterpret_cast<u64_t*>(a.ws);
  if (warped) {  // stage 1 is the plain call's; the chain runs behind the ranking of the finish kernel
    if (P.nch == 1) {
      sample_finish_kernel<true, true><<<a.B, SP_THREADS, 0, st>>>(a.logits, a.banned, a.row_ids, a.eos_ids, a.done, a.next, a.out, P, ws, a.steps);
    } else {
      sample_select_kernel<<<dim3(P.nch, a.B), SP_THREADS, 0, st>>>(a.logits, a.banned, a.done, P, ws);
      sample_finish_kernel<false, true><<<a.B, SP_THREADS, 0, st>>>(a.logits, a.banned, a.row_ids, a.eos_ids, a.done, a.next, a.out, P, ws, a.steps);
    }
    return (int)hipGetLastError();
  }
  if (P.nch == 1) {
    sample_finish_kernel<true><<<a.B, SP_THREADS, 0, st>>>(a.logits, a.banned, a.row_ids, a.eos_ids, a.done, a.next, a.out, P, ws, a.steps);
  } else {
    sample_select_kernel<<<dim3(P.nch, a.B), SP_THREADS, 0, st>>>(a.logits, a.banned, a.done, P, ws);
    sample_finish_kernel<false><<<a.B, SP_THREADS, 0, st>>>(a.logits, a.banned, a.row_ids, a.eos_ids, a.done, a.next, a.out, P, ws, a.steps);
  }
  return (int)hipGetLastError();
}

int constrain_scores(const ConstrainArgs& a, hipStream_t st) {
  if (!a.logits || !a.scores || !a.prompt || !a.prompt_len || a.B <= 0 || a.B > 65535 || a.vocab <= 0) return -1;
  if (((uintptr_t)a.logits | (uintptr_t)a.scores | (uintptr_t)a.prompt_len) & 3 || ((uintptr_t)a.prompt | (uintptr_t)a.fresh) & 7)
    return -1;
  if (a.step < 0 || a.step > CONSTRAIN_MAX_HISTORY || a.prompt_stride < 0 || a.prompt_stride > CONSTRAIN_MAX_HISTORY) return -1;
  if (a.step > 0 && (!a.fresh || a.new_stride < a.step)) return -1;
  if (a.ngram < 0 || a.n_per_prompt < 1 || a.B % a.n_per_prompt) return -1;
  if (a.n_eos < 0 || a.n_eos > 16 || (a.n_eos > 0 && (!a.eos_ids || ((uintptr_t)a.eos_ids & 3)))) return -1;
  if (a.n_begin < 0 || a.n_begin > CONSTRAIN_MAX_BEGIN || (a.n_begin > 0 && (!a.begin_ids || ((uintptr_t)a.begin_ids & 3)))) return -1;
  if (a.n_seqs < 0 || a.n_seqs > CONSTRAIN_MAX_SEQS || a.n_seq_tokens < 0 || a.n_seq_tokens > CONSTRAIN_MAX_SEQS * CONSTRAIN_MAX_SEQ_LEN)
    return -1;
  if (a.n_seqs > 0 && (!a.seq_tokens || !a.seq_offsets || (((uintptr_t)a.seq_tokens | (uintptr_t)a.seq_offsets) & 3))) return -1;
  ConstrainParams P;
  P.vocab = a.vocab;
  P.step = a.step;
  P.ngram = a.ngram;
  P.n_per_prompt = a.n_per_prompt;
  P.prompt_stride = a.prompt_stride;
  P.ban_eos = a.ban_eos ? 1 : 0;
  P.n_eos = a.n_eos;
  P.n_begin = a.n_begin;
  P.n_seqs = a.n_seqs;
  P.n_seq_tokens = a.n_seq_tokens;
  P.new_stride = a.new_stride;
  constrain_scores_kernel<<<dim3(sample_chunks(a.vocab), a.B), SP_THREADS, 0, st>>>(
      a.logits, a.scores, a.prompt, a.prompt_len, a.fresh, a.done, a.eos_ids, a.begin_ids, a.seq_tokens, a.seq_offsets, P);
  return (int)hipGetLastError();
}

// out[b * out_stride + column] = log-softmax of the raw fp32 row b at tokens[b] (include/slam_engine.h: slam_token_logprobs)
size_t token_logprobs_workspace_bytes(int B, int vocab) {
  if (B <= 0 || vocab <= 0) return 0;
  return (size_t)B * sample_chunks(vocab) * sizeof(float2);
}

int token_logprobs(const float* logits, int B, int vocab, const int64_t* tokens, const uint8_t* done, uint8_t* finished,
                   float* out, int64_t out_stride, int column, void* ws, size_t ws_bytes, hipStream_t st) {
  if (!logits || !tokens || !out || B <= 0 || B > 65535 || vocab <= 0 || ((uintptr_t)logits & 3)) return -1;
  if (!ws || ((uintptr_t)ws & 7) || ws_bytes < token_logprobs_workspace_bytes(B, vocab)) return -1;
  LogprobParams P;
  P.vocab = vocab;
  P.nch = sample_chunks(vocab);
  P.column = column;
  P.out_stride = out_stride;
  float2* w = reinterpret_cast<float2*>(ws);
  if (P.nch == 1) {
    logprob_finish_kernel<true><<<B, SP_THREADS, 0, st>>>(logits, tokens, done, finished, out, P, w);
  } else {
    logprob_chunk_kernel<<<dim3(P.nch, B), SP_THREADS, 0, st>>>(logits, finished, P, w);
    logprob_finish_kernel<false><<<B, 64, 0, st>>>(logits, tokens, done, finished, out, P, w);
  }
  return (int)hipGetLastError();
}

// classifier-free guidance (include/slam_engine.h: slam_cfg_scores): scores[b] = g (a - u) + u from the log-softmax a of logits
// row b and u of row B + b, on token_logprobs' row statistics; ws holds the (m_c, s_c) pairs of the 2 B rows.
size_t cfg_workspace_bytes(int B, int vocab) {
  if (B <= 0 || 2 * (int64_t)B > 65535 || vocab <= 0) return 0;
  return (size_t)2 * B * sample_chunks(vocab) * sizeof(float2);
}

int cfg_scores(const float* logits, int B, int vocab, float g, float* scores, void* ws, size_t ws_bytes, hipStream_t st) {
  if (!logits || !scores || !ws || B <= 0 || 2 * (int64_t)B > 65535 || vocab <= 0 || !isfinite(g)) return -1;
  if ((((uintptr_t)logits | (uintptr_t)scores) & 3) || ((uintptr_t)ws & 7) || ws_bytes < cfg_workspace_bytes(B, vocab)) return -1;
  const uintptr_t l0 = (uintptr_t)logits, s0 = (uintptr_t)scores;
  const size_t row = (size_t)vocab * sizeof(float);
  if (l0 < s0 + (size_t)B * row && s0 < l0 + (size_t)2 * B * row) return -1;  // the raw rows are read again afterwards
  CfgParams P;
  P.vocab = vocab;
  P.nch = sample_chunks(vocab);
  P.B = B;
  P.g = g;
  float2* w = reinterpret_cast<float2*>(ws);
  if (P.nch == 1) {
    cfg_scores_kernel<true><<<dim3(1, B), SP_THREADS, 0, st>>>(logits, scores, P, w);
  } else {
    LogprobParams L;
    L.vocab = vocab;
    L.nch = P.nch;
    L.column = 0;
    L.out_stride = 0;
    logprob_chunk_kernel<<<dim3(P.nch, 2 * B), SP_THREADS, 0, st>>>(logits, nullptr, L, w);
    cfg_scores_kernel<false><<<dim3(P.nch, B), SP_THREADS, 0, st>>>(logits, scores, P, w);
  }
  return (int)hipGetLastError();
}

int cfg_mirror_tokens(int64_t* next, int B, hipStream_t st) {
  if (!next || ((uintptr_t)next & 7) || B < 1 || B > 32767) return -1;
  cfg_mirror_kernel<<<nblk((size_t)B, 256), 256, 0, st>>>(next, B);
  return (int)hipGetLastError();
}

}  // namespace slam

using namespace slam;

// slam_sample_tokens and slam_sample_tokens_at: one argument block; the plain call is steps = NULL, group = 1, out_col = step
static int sample_any(const float* logits, int32_t B, int32_t vocab, const uint8_t* banned, const SlamSampleDesc* desc,
                      const int64_t* row_ids, const int32_t* eos_ids, uint8_t* done, int64_t* next, int64_t* out,
                      int64_t out_stride, void* ws, size_t ws_bytes, const uint32_t* steps, int32_t group, int64_t out_col,
                      slam_stream_t stream, const SlamWarpDesc* warp = nullptr) {
  if (!desc || (desc->do_sample != 0 && desc->do_sample != 1) || desc->n_eos > 16) return SLAM_EINVAL;
  SampleArgs a;  // sample_tokens refuses the rest (-1 = SLAM_EINVAL) before it launches anything
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
  return sample_tokens(a, (hipStream_t)stream);
}

extern "C" {

size_t slam_sample_workspace_bytes(int32_t B, int32_t vocab, int32_t top_k) { return sample_workspace_bytes(B, vocab, top_k); }
int slam_sample_tokens(const float* logits, int32_t B, int32_t vocab, const uint8_t* banned, const SlamSampleDesc* desc,
                       const int64_t* row_ids, const int32_t* eos_ids, uint8_t* done, int64_t* next, int64_t* out,
                       int64_t out_stride, void* ws, size_t ws_bytes, slam_stream_t stream) {
  return sample_any(logits, B, vocab, banned, desc, row_ids, eos_ids, done, next, out, out_stride, ws, ws_bytes, nullptr, 1, -1,
                    stream);
}
int slam_sample_tokens_at(const float* logits, int32_t B, int32_t vocab, const uint8_t* banned, const SlamSampleDesc* desc,
                          const int64_t* row_ids, const int32_t* eos_ids, uint8_t* done, int64_t* next, int64_t* out,
                          int64_t out_stride, void* ws, size_t ws_bytes, const uint32_t* steps, int32_t group, int32_t out_col,
                          slam_stream_t stream) {
  if (group < 1 || out_col < 0 || ((uintptr_t)steps & 3)) return SLAM_EINVAL;
  return sample_any(logits, B, vocab, banned, desc, row_ids, eos_ids, done, next, out, out_stride, ws, ws_bytes, steps, group,
                    out_col, stream);
}
int slam_sample_tokens_warped(const float* logits, int32_t B, int32_t vocab, const uint8_t* banned, const SlamSampleDesc* desc,
                              const int64_t* row_ids, const int32_t* eos_ids, uint8_t* done, int64_t* next, int64_t* out,
                              int64_t out_stride, void* ws, size_t ws_bytes, const uint32_t* steps, int32_t group,
                              int32_t out_col, const SlamWarpDesc* warp, slam_stream_t stream) {
  static_assert(sizeof(SlamWarpDesc) == 16 && sizeof(SlamSampleDesc) == 40, "the header's layouts");
  if (group < 1 || out_col < 0 || ((uintptr_t)steps & 3)) return SLAM_EINVAL;
  return sample_any(logits, B, vocab, banned, desc, row_ids, eos_ids, done, next, out, out_stride, ws, ws_bytes, steps, group,
                    out_col, stream, warp);
}

int slam_spec_accept(int64_t* chunk, const int64_t* tgt, int32_t B, int32_t K, int32_t max_new, int32_t pad_id,
                     const int32_t* eos_ids, int32_t n_eos, const int32_t* prompt_len, int32_t* n_new, uint8_t* done,
                     int64_t* out, int64_t out_stride, int32_t* lens_t, int32_t* lens_d, int64_t* draft_ids,
                     int32_t* draft_new_lens, int32_t* tgt_new_lens, int32_t* stats, slam_stream_t stream) {
  static_assert(SPEC_MAX_B == 1024 && SPEC_MAX_K == 15, "the header's limits are the kernel's");
  SpecArgs a;  // spec_accept refuses every bad argument (-1 = SLAM_EINVAL) before it launches anything
  a.chunk = chunk;
  a.tgt = tgt;
  a.B = B;
  a.K = K;
  a.max_new = max_new;
  a.pad_id = pad_id;
  a.n_eos = n_eos;
  a.eos_ids = eos_ids;
  a.prompt_len = prompt_len;
  a.n_new = n_new;
  a.done = done;
  a.out = out;
  a.out_stride = out_stride;
  a.lens_t = lens_t;
  a.lens_d = lens_d;
  a.draft_ids = draft_ids;
  a.draft_new_lens = draft_new_lens;
  a.tgt_new_lens = tgt_new_lens;
  a.stats = stats;
  return spec_accept(a, (hipStream_t)stream);
}

int slam_ngram_propose(int64_t* chunk, int32_t* n_prop, int32_t B, int32_t K, int32_t max_ngram, int32_t fill_id,
                       const int64_t* prompt, int64_t prompt_stride, const int32_t* prompt_len, const int64_t* new_tokens,
                       int64_t new_stride, const int32_t* n_new, const uint8_t* done, const int32_t* eos_ids, int32_t n_eos,
                       int32_t* stats, slam_stream_t stream) {
  static_assert(SLAM_NGRAM_MAX == NGRAM_MAX, "the header's limit is the kernel's");
  NgramArgs a;  // ngram_propose refuses every bad argument (-1 = SLAM_EINVAL) before it launches anything
  a.chunk = chunk;
  a.n_prop = n_prop;
  a.B = B;
  a.K = K;
  a.max_ngram = max_ngram;
  a.fill_id = fill_id;
  a.prompt = prompt;
  a.prompt_stride = prompt_stride;
  a.prompt_len = prompt_len;
  a.fresh = new_tokens;
  a.new_stride = new_stride;
  a.n_new = n_new;
  a.done = done;
  a.eos_ids = eos_ids;
  a.n_eos = n_eos;
  a.stats = stats;
  return ngram_propose(a, (hipStream_t)stream);
}

int slam_constrain_scores(const float* logits, float* scores, int32_t B, int32_t vocab, const SlamConstrainDesc* desc,
                          const int64_t* prompt, const int32_t* prompt_len, const int64_t* new_tokens, int64_t new_stride,
                          const uint8_t* done, const int32_t* eos_ids, const int32_t* begin_ids, const int32_t* seq_tokens,
                          const int32_t* seq_offsets, slam_stream_t stream) {
  if (!desc || (desc->ban_eos != 0 && desc->ban_eos != 1)) return SLAM_EINVAL;
  static_assert(SLAM_CONSTRAIN_MAX_SEQS == CONSTRAIN_MAX_SEQS && SLAM_CONSTRAIN_MAX_SEQ_LEN == CONSTRAIN_MAX_SEQ_LEN &&
                    SLAM_CONSTRAIN_MAX_BEGIN == CONSTRAIN_MAX_BEGIN,
                "the header's caps are the kernels'");
  ConstrainArgs a;  // constrain_scores refuses the rest (-1 = SLAM_EINVAL) before it launches anything
  a.logits = logits;
  a.scores = scores;
  a.B = B;
  a.vocab = vocab;
  a.step = desc->step;
  a.ngram = desc->no_repeat_ngram;
  a.n_per_prompt = desc->n_per_prompt;
  a.prompt_stride = desc->prompt_stride;
  a.ban_eos = desc->ban_eos;
  a.n_eos = desc->n_eos;
  a.n_begin = desc->n_begin;
  a.n_seqs = desc->n_seqs;
  a.n_seq_tokens = desc->n_seq_tokens;
  a.prompt = prompt;
  a.prompt_len = prompt_len;
  a.fresh = new_tokens;
  a.new_stride = new_stride;
  a.done = done;
  a.eos_ids = eos_ids;
  a.begin_ids = begin_ids;
  a.seq_tokens = seq_tokens;
  a.seq_offsets = seq_offsets;
  return constrain_scores(a, (hipStream_t)stream);
}

size_t slam_token_logprobs_workspace_bytes(int32_t B, int32_t vocab) { return token_logprobs_workspace_bytes(B, vocab); }
int slam_token_logprobs(const float* logits, int32_t B, int32_t vocab, const int64_t* tokens, const uint8_t* done,
                        uint8_t* finished, float* out, int64_t out_stride, int32_t column, void* ws, size_t ws_bytes,
                        slam_stream_t stream) {
  // token_logprobs refuses every bad argument (-1 = SLAM_EINVAL) before it launches anything
  return token_logprobs(logits, B, vocab, tokens, done, finished, out, out_stride, column, ws, ws_bytes, (hipStream_t)stream);
}

size_t slam_cfg_workspace_bytes(int32_t B, int32_t vocab) { return cfg_workspace_bytes(B, vocab); }
int slam_cfg_scores(const float* logits, int32_t B, int32_t vocab, float guidance_scale, float* scores, void* ws,
                    size_t ws_bytes, slam_stream_t stream) {
  // cfg_scores refuses every bad argument (-1 = SLAM_EINVAL) before it launches anything
  return cfg_scores(logits, B, vocab, guidance_scale, scores, ws, ws_bytes, (hipStream_t)stream);
}
int slam_cfg_mirror_tokens(int64_t* next, int32_t B, slam_stream_t stream) {
  return cfg_mirror_tokens(next, B, (hipStream_t)stream);
}

}  // extern "C"
