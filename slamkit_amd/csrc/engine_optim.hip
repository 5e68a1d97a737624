// The optimizer side of a SlamEngine (include/slam_engine.h): gradient norm and clip, the AdamW, Adafactor and Muon entry points, the
// no-decay set, the bf16 gradient image, slam_zero_grads and slam_cast_params. The kernels are in optimizer.hip, adafactor.hip and muon.hip.
#include <hip/hip_runtime.h>
#include <math.h>

#include "engine_impl.h"

namespace {

// AdamW (`a`: the update at element 0 of the flat buffers) over a chunk of the model with transposed weight images bound:
// every matrix goes through the tile kernel that writes its transposed image in the same pass (no separate transpose launch),
// the vectors between them through the strided kernel. A group is whole tensors, so the no-decay set (slam_set_decay_mask) is
// applied here, on the host: a tensor outside the decay set is launched with wd = 0 through the same kernels, and a batch of
// layers goes out layer by layer only where the flags differ across the layers (never under the HF rule).
int adamw_model(SlamEngine* h, const AdamArgs& a, int chunk, hipStream_t st) {
  return for_each_param_group(h, chunk, [&](int64_t off, int64_t rows, int cols, int batch) {
    auto run = [&](int64_t o, int nb, bool decay) {
      AdamArgs g = a.at(o);
      g.nd = AdamNoDecay{};
      if (!decay) g.wd = 0;
      if (cols == 1) return adamw_strided(g, (size_t)rows, nb, (size_t)h->layer_stride, st);
      return adamw_tiles(g, (int)rows, cols, nb, (size_t)h->layer_stride, st);
    };
    if (h->nd_host.empty()) return run(off, batch, true);
    const bool nd0 = h->no_decay(off);
    bool same = true;
    for (int l = 1; l < batch; ++l) same = same && h->no_decay(off + l * h->layer_stride) == nd0;
    if (same) return run(off, batch, !nd0);
    for (int l = 0; l < batch; ++l) {
      const int64_t o = off + l * h->layer_stride;
      if (int r = run(o, 1, !h->no_decay(o))) return r;
    }
    return 0;
  });
}

// the update as the engine's state fixes it, at element 0 of the flat buffers (the gradients where the last backward left
// them); the state arrays are the caller's
static AdamArgs adam_args(SlamEngine* h, int mode, const float* norm_out, double lr, double b1, double b2, double eps, double wd,
                          int step, int zero_grad) {
  AdamArgs a;
  a.mode = mode;
  a.params = h->params;
  a.params_t = h->params_t;
  a.g_bf16 = h->gfinal == 2;  // the last backward kept its final values in bf16 only (slam_set_grad_image's buffer)
  a.g = a.g_bf16 ? (void*)h->g16 : (void*)h->grads;
  a.clip = norm_out;
  a.lr = lr; a.b1 = b1; a.b2 = b2; a.eps = eps; a.wd = wd;
  a.step = step; a.zero_grad = zero_grad;
  a.sr.on = h->adamw_sr; a.sr.seed = h->adamw_sr_seed;
  if (h->nd_dev) { a.nd.bounds = h->nd_dev; a.nd.n = (int)h->nd_host.size(); }
  return a;
}

static int adamw_any(SlamEngine* h, int mode, float* master, void* m, void* v, const float* norm_out, double lr, double b1, double b2,
                     double eps, double wd, int32_t step, int32_t zero_grad, slam_stream_t stream) {
  if (!h || !m || !v || step < 1 || (mode != 2 && !master)) return SLAM_EINVAL;
  if (!h->grads || !h->params) return h->fail(SLAM_ESTATE, "bind params first");
  if (h->n_params & 7) return h->fail(SLAM_EINVAL, "parameter count must be a multiple of 8");
  hipStream_t st = (hipStream_t)stream;
  CK(join_optimizer(h, st));
  CK(join_params(h, st));
  h->w8_valid = false;
  const bool fused = h->params_t != nullptr && h->fuse_adamw_t;
  AdamArgs a = adam_args(h, mode, norm_out, lr, b1, b2, eps, wd, step, zero_grad);
  a.master = master; a.m = m; a.v = v;
  // zeroing belongs to the fp32 accumulation buffer: the kernels cannot do it while they read the bf16 image
  if (a.g_bf16 && zero_grad) CK((int)hipMemsetAsync(h->grads, 0, (size_t)h->n_params * sizeof(float), st));
  if (!h->overlap_adamw || mode != 0) {
    if (fused) {
      CK(adamw_model(h, a, -1, st));
      h->params_t_dirty = false;
      return SLAM_OK;
    }
    CK(adamw_flat(a, (size_t)h->n_params, st));
    return slam_refresh_transposed(h, stream);
  }
  // "overlap_adamw" (fp32 state): per-layer chunks on the engine's side stream; the next forward waits per layer
  CK(ensure_side(h));
  CK((int)hipEventRecord(h->ev_fork, st));
  CK((int)hipStreamWaitEvent(h->side, h->ev_fork, 0));
  const int L = h->d.n_layers;
  for (int c = 0; c < L + 2; ++c) {
    if (fused) {
      CK(adamw_model(h, a, c, h->side));
    } else {
      const int64_t lo = c == 0 ? 0 : c <= L ? h->lo[c - 1].ln1 : h->off_norm;
      const int64_t hi = c == 0 ? h->lo[0].ln1 : c < L ? h->lo[c].ln1 : c == L ? h->off_norm : h->n_params;
      CK(adamw_flat(a.at(lo), (size_t)(hi - lo), h->side));
      if (h->params_t) CK(for_each_param_group(h, c, transpose_group(h, h->side)));
    }
    CK((int)hipEventRecord(h->ev_chunk[c], h->side));
  }
  h->opt_pending = true;
  return SLAM_OK;
}

// the three slam_adamw_range* entry points: elements [offset, offset + count) of the engine's buffers against the caller's
// shard of the state, which starts at that element (master: NULL in mode 2). Mode 2 updates 8 elements per thread, the others 4.
static int adamw_range_impl(SlamEngine* h, int mode, int64_t offset, int64_t count, float* master, void* m, void* v, const float* norm_out,
                            double lr, double b1, double b2, double eps, double wd, int32_t step, int32_t zero_grad, slam_stream_t stream) {
  const int64_t mask = mode == 2 ? 7 : 3;
  if (!h || (mode != 2 && !master) || !m || !v || step < 1 || offset < 0 || count < 0 || offset + count > h->n_params || (offset & mask) ||
      (count & mask))
    return SLAM_EINVAL;
  if (!h->grads || !h->params) return h->fail(SLAM_ESTATE, "bind params first");
  hipStream_t st = (hipStream_t)stream;
  CK(join_optimizer(h, st));
  h->w8_valid = false;
  AdamArgs a = adam_args(h, mode, norm_out, lr, b1, b2, eps, wd, step, zero_grad).at(offset);
  a.master = master; a.m = m; a.v = v;
  // as in adamw_any: the kernels cannot clear the fp32 accumulation buffer while they read the bf16 image - here the range only
  if (a.g_bf16 && zero_grad && count) CK((int)hipMemsetAsync(h->grads + offset, 0, (size_t)count * sizeof(float), st));
  if (count) CK(adamw_flat(a, (size_t)count, st));
  h->params_t_dirty = h->params_t != nullptr;
  return SLAM_OK;
}

}  // namespace

extern "C" {

int slam_grad_norm(SlamEngine* h, float max_norm, float* norm_out, slam_stream_t stream) {
  if (!h || !norm_out) return SLAM_EINVAL;
  if (!h->grads || !h->ws) return h->fail(SLAM_ESTATE, "bind params and workspace first");
  CK(join_optimizer(h, (hipStream_t)stream));
  if (h->gn_valid) {  // the last backward emitted the partial sums of squares with its final-value stores: add them, in slot order
    CK(grad_norm_from_chunks(h->gn_part, h->gn_used, max_norm, norm_out, (hipStream_t)stream));
    return SLAM_OK;
  }
  // chunk sums over the buffer the gradients are in (the bf16 image after a "grad_final_next" = 2 backward whose buckets were exchanged)
  const int g16 = h->gfinal == 2;
  const size_t n = (size_t)h->n_params;
  CK(grad_sumsq_chunks(g16 ? (const void*)h->g16 : (const void*)h->grads, g16, n, 0, n, h->part_ws, (hipStream_t)stream));
  CK(grad_norm_from_chunks(h->part_ws, (n + grad_chunk_elems() - 1) / grad_chunk_elems(), max_norm, norm_out, (hipStream_t)stream));
  return SLAM_OK;
}
int slam_adamw_step(SlamEngine* h, float* master, float* m, float* v, const float* norm_out, double lr, double b1,
                    double b2, double eps, double wd, int32_t step, int32_t zero_grad, slam_stream_t stream) {
  return adamw_any(h, 0, master, m, v, norm_out, lr, b1, b2, eps, wd, step, zero_grad, stream);
}

int slam_adamw_step_bf16_moments(SlamEngine* h, float* master, void* exp_avg_bf16, void* exp_avg_sq_bf16, const float* norm_out,
                                 double lr, double b1, double b2, double eps, double wd, int32_t step, int32_t zero_grad,
                                 slam_stream_t stream) {
  return adamw_any(h, 1, master, exp_avg_bf16, exp_avg_sq_bf16, norm_out, lr, b1, b2, eps, wd, step, zero_grad, stream);
}

int slam_adamw_step_bf16(SlamEngine* h, void* exp_avg_bf16, void* exp_avg_sq_bf16, const float* norm_out, double lr,
                         double b1, double b2, double eps, double wd, int32_t step, int32_t zero_grad, slam_stream_t stream) {
  return adamw_any(h, 2, nullptr, exp_avg_bf16, exp_avg_sq_bf16, norm_out, lr, b1, b2, eps, wd, step, zero_grad, stream);
}

// ---- sharded optimizer (data-parallel "rs_ag": reduce-scatter gradients, update the owned 1/N shard, all-gather bf16
// parameters) ------------------------------------------------------------------------------------------------------
int64_t slam_grad_chunk_elems(void) { return grad_chunk_elems(); }
int slam_grad_sumsq_chunks(SlamEngine* h, int64_t offset, int64_t count, float* chunk_sums, slam_stream_t stream) {
  if (!h || !chunk_sums || offset < 0 || count < 0) return SLAM_EINVAL;
  if (!h->grads) return h->fail(SLAM_ESTATE, "no gradient buffer bound");
  const int g16 = h->gfinal == 2;  // the gradients (a reduced shard of them) are in the bf16 image
  int r = grad_sumsq_chunks(g16 ? (const void*)h->g16 : (const void*)h->grads, g16, (size_t)h->n_params, (size_t)offset, (size_t)count, chunk_sums,
                            (hipStream_t)stream);
  if (r < 0) return h->fail(SLAM_EINVAL, "range must start on a chunk boundary and end on one (or at the end of the buffer)");
  CK(r);
  return SLAM_OK;
}

int slam_grad_norm_from_chunks(SlamEngine* h, const float* chunk_sums, float max_norm, float* norm_out, slam_stream_t stream) {
  if (!h || !chunk_sums || !norm_out) return SLAM_EINVAL;
  const size_t nc = ((size_t)h->n_params + grad_chunk_elems() - 1) / grad_chunk_elems();
  CK(grad_norm_from_chunks(chunk_sums, nc, max_norm, norm_out, (hipStream_t)stream));
  return SLAM_OK;
}

int slam_adamw_range(SlamEngine* h, int64_t offset, int64_t count, float* master, float* m, float* v, const float* norm_out,
                     double lr, double b1, double b2, double eps, double wd, int32_t step, int32_t zero_grad,
                     slam_stream_t stream) {
  return adamw_range_impl(h, 0, offset, count, master, m, v, norm_out, lr, b1, b2, eps, wd, step, zero_grad, stream);
}

int slam_adamw_range_bf16_moments(SlamEngine* h, int64_t offset, int64_t count, float* master, void* m_bf16, void* v_bf16,
                                  const float* norm_out, double lr, double b1, double b2, double eps, double wd, int32_t step,
                                  int32_t zero_grad, slam_stream_t stream) {
  return adamw_range_impl(h, 1, offset, count, master, m_bf16, v_bf16, norm_out, lr, b1, b2, eps, wd, step, zero_grad, stream);
}

int slam_adamw_range_bf16(SlamEngine* h, int64_t offset, int64_t count, void* m_bf16, void* v_bf16, const float* norm_out,
                          double lr, double b1, double b2, double eps, double wd, int32_t step, int32_t zero_grad,
                          slam_stream_t stream) {
  return adamw_range_impl(h, 2, offset, count, nullptr, m_bf16, v_bf16, norm_out, lr, b1, b2, eps, wd, step, zero_grad, stream);
}

int slam_set_decay_mask(SlamEngine* h, const uint8_t* decay, int32_t n_tensors) {
  if (!h) return SLAM_EINVAL;
  std::vector<uint64_t> b;
  if (decay) {
    const size_t nt = h->tensors.size();
    if (n_tensors != (int32_t)nt) return h->fail(SLAM_EINVAL, "decay mask: n_tensors must equal slam_tensor_count");
    for (size_t i = 0; i < nt; ++i) {
      if (decay[i]) continue;
      const uint64_t lo = (uint64_t)h->tensors[i].offset, hi = (uint64_t)(i + 1 < nt ? h->tensors[i + 1].offset : h->n_params);
      if ((lo | hi) & 7) return h->fail(SLAM_EINVAL, "decay mask: tensor bounds must be multiples of 8");
      if (!b.empty() && b.back() == lo) b.back() = hi;  // adjacent no-decay tensors: one range
      else { b.push_back(lo); b.push_back(hi); }
    }
  }
  uint64_t* dev = nullptr;
  if (!b.empty()) {
    std::vector<uint64_t> up(b);
    up.push_back(UINT64_MAX);  // the sentinel that ends a thread's walk
    CK((int)hipMalloc(&dev, up.size() * sizeof(uint64_t)));
    const int r = (int)hipMemcpy(dev, up.data(), up.size() * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (r) { (void)hipFree(dev); CK(r); }
  }
  if (h->nd_dev) CK((int)hipFree(h->nd_dev));  // synchronises with the device: no update in flight still reads the old table
  h->nd_dev = dev;
  h->nd_host.swap(b);
  return SLAM_OK;
}

// ---- Adafactor (the contract is in the header; the kernels in adafactor.hip) ---------------------------------------------
int slam_adafactor_set_segments(SlamEngine* h, const SlamAdafactorSegment* segs, int32_t n) {
  if (!h) return SLAM_EINVAL;
  std::vector<AfSeg> t;
  if (segs || n) {
    if (!segs || n < 1) return h->fail(SLAM_EINVAL, "adafactor segments: a table of n >= 1 segments, or NULL and 0 to clear");
    std::vector<std::pair<int64_t, int64_t>> iv;  // the element intervals the segments cover
    int64_t tiles = 0;
    for (int32_t i = 0; i < n; ++i) {
      const SlamAdafactorSegment& g = segs[i];
      const std::string at = "adafactor segment " + std::to_string(i) + ": ";
      if (g.rows < 1 || g.cols < 1) return h->fail(SLAM_EINVAL, at + "rows and cols must be positive");
      if (g.factored != 0 && g.factored != 1) return h->fail(SLAM_EINVAL, at + "factored is 0 or 1");
      if (!g.factored && g.rows != 1) return h->fail(SLAM_EINVAL, at + "a vector (factored = 0) has rows = 1 and cols = its length");
      if (g.pattern < 0 || g.pattern > 2) return h->fail(SLAM_EINVAL, at + "pattern is 0 (contiguous), 1 or 2 (32 rows of every 64, phase 0 or 32)");
      if (g.pattern && (g.rows % 32)) return h->fail(SLAM_EINVAL, at + "rows in groups of 32 need rows % 32 == 0");
      if ((g.offset & 7) || (g.cols & 7)) return h->fail(SLAM_EINVAL, at + "misaligned: offset and cols must be multiples of 8");
      const int64_t c = g.cols;
      const int64_t span = g.pattern ? ((int64_t)(g.rows / 32 - 1) * 64 + (g.pattern == 2 ? 32 : 0) + 32) * c : (int64_t)g.rows * c;
      if (g.offset < 0 || g.offset > h->n_params || span > h->n_params - g.offset)
        return h->fail(SLAM_EINVAL, at + "out of range: it leaves [0, slam_param_count)");
      if (!g.pattern) {
        iv.push_back({g.offset, g.offset + span});
      } else {
        for (int64_t k = 0; k < g.rows / 32; ++k) {
          const int64_t lo = g.offset + (k * 64 + (g.pattern == 2 ? 32 : 0)) * c;
          iv.push_back({lo, lo + 32 * c});
        }
      }
      AfSeg s;
      s.off = g.offset; s.rows = g.rows; s.cols = g.cols; s.factored = g.factored;
      s.phase = g.pattern == 0 ? -1 : g.pattern == 1 ? 0 : 32;
      tiles += (int64_t)((g.rows + AF_TILE_ROWS - 1) / AF_TILE_ROWS) * ((g.cols + AF_TILE_COLS - 1) / AF_TILE_COLS);
      t.push_back(s);
    }
    if (tiles > 0x7fffffff) return h->fail(SLAM_EINVAL, "adafactor segments: more tiles than one launch holds");
    std::sort(iv.begin(), iv.end());
    for (size_t i = 1; i < iv.size(); ++i)
      if (iv[i].first < iv[i - 1].second) return h->fail(SLAM_EINVAL, "adafactor segments overlap: two segments share an element");
  }
  AfPlan plan;
  AfSeg* dev = nullptr;
  if (!t.empty()) {
    adafactor_layout(t.data(), (int)t.size(), &plan);
    CK((int)hipMalloc(&dev, t.size() * sizeof(AfSeg)));
    const int r = (int)hipMemcpy(dev, t.data(), t.size() * sizeof(AfSeg), hipMemcpyHostToDevice);
    if (r) { (void)hipFree(dev); CK(r); }
    plan.segs = dev;
  }
  if (h->af_plan.segs) CK((int)hipFree((void*)h->af_plan.segs));  // synchronises with the device: no step in flight reads the old table
  h->af_plan = plan;
  h->af_host.swap(t);
  h->af_ws = nullptr;  // sized for the table that went
  return SLAM_OK;
}
int slam_adafactor_sizes(SlamEngine* h, int64_t* state_floats, size_t* workspace_bytes) {
  if (!h || !state_floats || !workspace_bytes) return SLAM_EINVAL;
  if (h->af_host.empty()) return h->fail(SLAM_ESTATE, "adafactor: no segment table (slam_adafactor_set_segments)");
  *state_floats = h->af_plan.state_floats;
  *workspace_bytes = (size_t)h->af_plan.ws_floats * sizeof(float);
  return SLAM_OK;
}
int slam_adafactor_bind_workspace(SlamEngine* h, void* workspace, size_t bytes) {
  if (!h) return SLAM_EINVAL;
  if (!workspace) { h->af_ws = nullptr; return SLAM_OK; }
  if (h->af_host.empty()) return h->fail(SLAM_ESTATE, "adafactor: no segment table (slam_adafactor_set_segments)");
  if (((uintptr_t)workspace) & 15) return h->fail(SLAM_EINVAL, "adafactor workspace must be 16-byte aligned");
  if (bytes < (size_t)h->af_plan.ws_floats * sizeof(float)) return h->fail(SLAM_ENOMEM, "adafactor workspace too small");
  h->af_ws = (float*)workspace;
  return SLAM_OK;
}
int slam_adafactor_step(SlamEngine* h, float* master, float* state, const float* norm_out, double lr, double eps1,
                        double clip_threshold, double decay_rate, double wd, int32_t step, int32_t zero_grad, slam_stream_t stream) {
  if (!h) return SLAM_EINVAL;
  if (h->af_host.empty()) return h->fail(SLAM_ESTATE, "adafactor step without a segment table (slam_adafactor_set_segments)");
  if (h->overlap_adamw) return h->fail(SLAM_ESTATE, "adafactor step with overlap_adamw on: the overlapped chunks belong to AdamW");
  if (!state) return h->fail(SLAM_EINVAL, "adafactor step: state_f32 is NULL");
  if (step < 1) return h->fail(SLAM_EINVAL, "adafactor step: step counts from 1");
  if (!(clip_threshold > 0)) return h->fail(SLAM_EINVAL, "adafactor step: clip_threshold must be positive");
  if (!h->af_ws) return h->fail(SLAM_ESTATE, "adafactor step without a workspace (slam_adafactor_bind_workspace)");
  if (!h->grads || !h->params) return h->fail(SLAM_ESTATE, "bind params first");
  hipStream_t st = (hipStream_t)stream;
  CK(join_optimizer(h, st));
  CK(join_params(h, st));
  h->w8_valid = false;
  AfArgs a;
  a.master = master; a.params = h->params; a.state = state; a.ws = h->af_ws; a.clip = norm_out;
  a.g_bf16 = h->gfinal == 2;  // the last backward kept its final values in bf16 only (slam_set_grad_image's buffer)
  a.g = a.g_bf16 ? (const void*)h->g16 : (const void*)h->grads;
  const double beta = 1.0 - pow((double)step, decay_rate);  // HF: python doubles, fp32 in the kernel
  a.lr = (float)lr; a.eps1 = (float)eps1; a.clip_threshold = (float)clip_threshold; a.wd = (float)wd;
  a.beta = (float)beta; a.one_minus_beta = (float)(1.0 - beta);
  a.step = step;
  a.sr.on = h->adamw_sr; a.sr.seed = h->adamw_sr_seed;
  if (h->nd_dev) { a.nd.bounds = h->nd_dev; a.nd.n = (int)h->nd_host.size(); }
  CK(adafactor_step(h->af_plan, a, st));
  if (zero_grad) CK((int)hipMemsetAsync(h->grads, 0, (size_t)h->n_params * sizeof(float), st));
  return slam_refresh_transposed(h, stream);
}

// ---- Muon (the contract is in the header; the kernels in muon.hip) ---------------------------------------------------------
int slam_muon_set_segments(SlamEngine* h, const SlamMuonSegment* segs, int32_t n) {
  if (!h) return SLAM_EINVAL;
  std::vector<MuSeg> t;
  if (segs || n) {
    if (!segs || n < 1) return h->fail(SLAM_EINVAL, "muon segments: a table of n >= 1 segments, or NULL and 0 to clear");
    std::vector<std::pair<int64_t, int64_t>> iv;  // the element intervals the segments cover
    for (int32_t i = 0; i < n; ++i) {
      const SlamMuonSegment& g = segs[i];
      const std::string at = "muon segment " + std::to_string(i) + ": ";
      if (g.rows < 1 || g.cols < 1) return h->fail(SLAM_EINVAL, at + "rows and cols must be positive");
      if (g.rows < 2 || g.cols < 2) return h->fail(SLAM_EINVAL, at + "not a matrix: Muon takes 2-D weights only");
      if (g.pattern < 0 || g.pattern > 2) return h->fail(SLAM_EINVAL, at + "pattern is 0 (contiguous), 1 or 2 (32 rows of every 64, phase 0 or 32)");
      if (g.pattern && (g.rows % 32)) return h->fail(SLAM_EINVAL, at + "rows in groups of 32 need rows % 32 == 0");
      if ((g.offset & 7) || (g.cols & 7) || (g.rows & 7)) return h->fail(SLAM_EINVAL, at + "misaligned: offset, rows and cols must be multiples of 8");
      const int64_t c = g.cols;
      const int64_t span = g.pattern ? ((int64_t)(g.rows / 32 - 1) * 64 + (g.pattern == 2 ? 32 : 0) + 32) * c : (int64_t)g.rows * c;
      if (g.offset < 0 || g.offset > h->n_params || span > h->n_params - g.offset)
        return h->fail(SLAM_EINVAL, at + "out of range: it leaves [0, slam_param_count)");
      if (!g.pattern) {
        iv.push_back({g.offset, g.offset + span});
      } else {
        for (int64_t k = 0; k < g.rows / 32; ++k) {
          const int64_t lo = g.offset + (k * 64 + (g.pattern == 2 ? 32 : 0)) * c;
          iv.push_back({lo, lo + 32 * c});
        }
      }
      MuSeg s;
      s.off = g.offset; s.rows = g.rows; s.cols = g.cols;
      s.phase = g.pattern == 0 ? -1 : g.pattern == 1 ? 0 : 32;
      t.push_back(s);
    }
    std::sort(iv.begin(), iv.end());
    for (size_t i = 1; i < iv.size(); ++i)
      if (iv[i].first < iv[i - 1].second) return h->fail(SLAM_EINVAL, "muon segments overlap: two segments share an element");
  }
  MuPlan plan;
  MuSeg* dev = nullptr;
  if (!t.empty()) {
    if (muon_layout(t.data(), (int)t.size(), &plan))
      return h->fail(SLAM_EINVAL, "muon segments: more shape classes or tiles than one step holds");
    for (int c = 0; c < plan.n_classes; ++c)
      if (plan.cls[c].count > 65535) return h->fail(SLAM_EINVAL, "muon segments: more than 65535 matrices of one shape");
    CK((int)hipMalloc(&dev, t.size() * sizeof(MuSeg)));
    const int r = (int)hipMemcpy(dev, t.data(), t.size() * sizeof(MuSeg), hipMemcpyHostToDevice);
    if (r) { (void)hipFree(dev); CK(r); }
    plan.segs = dev;
  }
  if (h->mu_plan.segs) CK((int)hipFree((void*)h->mu_plan.segs));  // synchronises with the device: no step in flight reads the old table
  h->mu_plan = plan;
  h->mu_host.swap(t);
  h->mu_ws = nullptr;  // sized for the table that went
  return SLAM_OK;
}
int slam_muon_sizes(SlamEngine* h, int64_t* momentum_floats, size_t* workspace_bytes) {
  if (!h || !momentum_floats || !workspace_bytes) return SLAM_EINVAL;
  if (h->mu_host.empty()) return h->fail(SLAM_ESTATE, "muon: no segment table (slam_muon_set_segments)");
  *momentum_floats = h->mu_plan.elems;
  *workspace_bytes = h->mu_plan.ws_bytes;
  return SLAM_OK;
}
int slam_muon_bind_workspace(SlamEngine* h, void* workspace, size_t bytes) {
  if (!h) return SLAM_EINVAL;
  if (!workspace) { h->mu_ws = nullptr; return SLAM_OK; }
  if (h->mu_host.empty()) return h->fail(SLAM_ESTATE, "muon: no segment table (slam_muon_set_segments)");
  if (((uintptr_t)workspace) & 255) return h->fail(SLAM_EINVAL, "muon workspace must be 256-byte aligned");
  if (bytes < h->mu_plan.ws_bytes) return h->fail(SLAM_ENOMEM, "muon workspace too small");
  h->mu_ws = (char*)workspace;
  return SLAM_OK;
}
int32_t slam_muon_class_count(SlamEngine* h) { return h ? h->mu_plan.n_classes : SLAM_EINVAL; }
int slam_muon_class_info(SlamEngine* h, int32_t i, SlamMuonClass* out) {
  if (!h || !out) return SLAM_EINVAL;
  if (i < 0 || i >= h->mu_plan.n_classes) return h->fail(SLAM_EINVAL, "muon class index out of range");
  const MuClass& k = h->mu_plan.cls[i];
  out->rows = k.rows; out->cols = k.cols; out->n = k.n; out->m = k.m; out->count = k.count; out->parts = k.parts;
  out->x_byte_offset = (int64_t)h->mu_plan.x_off + k.pack * 2;
  out->part_byte_offset = (int64_t)h->mu_plan.part_off + (int64_t)k.part0 * 4;
  return SLAM_OK;
}

}  // extern "C"

namespace {
// what the three Muon launch groups share: the checks of a call that touches the engine's buffers, and the arguments
int muon_begin(SlamEngine* h, const char* what, hipStream_t st, MuArgs* a) {
  if (h->overlap_adamw) return h->fail(SLAM_ESTATE, std::string(what) + " with overlap_adamw on: the overlapped chunks belong to AdamW");
  if (h->mu_host.empty()) return h->fail(SLAM_ESTATE, std::string(what) + " without a segment table (slam_muon_set_segments)");
  if (!h->mu_ws) return h->fail(SLAM_ESTATE, std::string(what) + " without a workspace (slam_muon_bind_workspace)");
  if (!h->grads || !h->params) return h->fail(SLAM_ESTATE, "bind params first");
  CK(join_optimizer(h, st));
  CK(join_params(h, st));
  a->params = h->params; a->ws = h->mu_ws;
  a->g_bf16 = h->gfinal == 2;  // the last backward kept its final values in bf16 only (slam_set_grad_image's buffer)
  a->g = a->g_bf16 ? (const void*)h->g16 : (const void*)h->grads;
  a->sr.on = h->adamw_sr; a->sr.seed = h->adamw_sr_seed;
  if (h->nd_dev) { a->nd.bounds = h->nd_dev; a->nd.n = (int)h->nd_host.size(); }
  return SLAM_OK;
}
int muon_momentum_args(SlamEngine* h, const char* what, float* mom, const float* norm_out, double momentum, int nesterov, int zero_grad,
                       MuArgs* a) {
  if (!mom) return h->fail(SLAM_EINVAL, std::string(what) + ": momentum_f32 is NULL");
  if (!(momentum >= 0.0 && momentum < 1.0)) return h->fail(SLAM_EINVAL, std::string(what) + ": momentum must lie in [0, 1)");
  a->mom = mom; a->clip = norm_out;
  a->mu = (float)momentum; a->omm = (float)(1.0 - momentum);
  a->nesterov = nesterov != 0;
  a->gzero = zero_grad ? h->grads : nullptr;
  return SLAM_OK;
}
int muon_apply_args(SlamEngine* h, const char* what, float* master, double lr, double wd, int adjust_lr, int step, MuArgs* a) {
  if (adjust_lr < 0 || adjust_lr > 2) return h->fail(SLAM_EINVAL, std::string(what) + ": adjust_lr is 0 (none), 1 (original) or 2 (match_rms_adamw)");
  if (step < 1) return h->fail(SLAM_EINVAL, std::string(what) + ": step counts from 1");
  a->master = master; a->lr = lr; a->wd = wd; a->adjust_lr = adjust_lr; a->step = step;
  return SLAM_OK;
}
}  // namespace

extern "C" {

int slam_muon_step(SlamEngine* h, float* master, float* mom, const float* norm_out, double lr, double wd, double momentum,
                   int32_t nesterov, int32_t ns_steps, double a, double b, double c, double eps, int32_t adjust_lr, int32_t step,
                   int32_t zero_grad, slam_stream_t stream) {
  if (!h) return SLAM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  MuArgs m;
  if (ns_steps < 1 || ns_steps > 16) return h->fail(SLAM_EINVAL, "muon step: ns_steps must lie in 1 .. 16");
  if (int r = muon_momentum_args(h, "muon step", mom, norm_out, momentum, nesterov, zero_grad, &m)) return r;
  if (int r = muon_apply_args(h, "muon step", master, lr, wd, adjust_lr, step, &m)) return r;
  if (int r = muon_begin(h, "muon step", st, &m)) return r;
  h->w8_valid = false;
  m.ns_steps = ns_steps; m.a = (float)a; m.b = (float)b; m.c = (float)c; m.eps = (float)eps;
  CK(muon_step(h->mu_plan, m, st));
  h->params_t_dirty = h->params_t != nullptr;
  return SLAM_OK;
}
int slam_op_muon_prepare(SlamEngine* h, float* mom, const float* norm_out, double momentum, int32_t nesterov, int32_t zero_grad,
                         slam_stream_t stream) {
  if (!h) return SLAM_EINVAL;
  MuArgs m;
  if (int r = muon_momentum_args(h, "muon prepare", mom, norm_out, momentum, nesterov, zero_grad, &m)) return r;
  if (int r = muon_begin(h, "muon prepare", (hipStream_t)stream, &m)) return r;
  CK(muon_prepare(h->mu_plan, m, (hipStream_t)stream));
  return SLAM_OK;
}
int slam_op_muon_apply(SlamEngine* h, float* master, const void* o_packed, double lr, double wd, int32_t adjust_lr, int32_t step,
                       slam_stream_t stream) {
  if (!h) return SLAM_EINVAL;
  MuArgs m;
  if (int r = muon_apply_args(h, "muon apply", master, lr, wd, adjust_lr, step, &m)) return r;
  if (int r = muon_begin(h, "muon apply", (hipStream_t)stream, &m)) return r;
  h->w8_valid = false;
  CK(muon_apply(h->mu_plan, m, o_packed ? (const bf16_t*)o_packed : (const bf16_t*)(h->mu_ws + h->mu_plan.x_off), (hipStream_t)stream));
  h->params_t_dirty = h->params_t != nullptr;
  return SLAM_OK;
}
size_t slam_op_muon_ns_workspace(int32_t batch, int32_t n, int32_t m) { return muon_ns_workspace_bytes(batch, n, m); }
int slam_op_muon_ns(void* x, int32_t batch, int32_t n, int32_t m, int64_t stride, const float* partials, int32_t parts,
                    int32_t ns_steps, double a, double b, double c, double eps, void* ws, size_t ws_bytes, slam_stream_t stream) {
  const size_t need = muon_ns_workspace_bytes(batch, n, m);
  if (!x || !ws || !need || n > m || ns_steps < 1 || ns_steps > 16 || (partials && parts < 1) || (((uintptr_t)ws) & 255) ||
      (((uintptr_t)x) & 15))
    return SLAM_EINVAL;
  if (ws_bytes < need) return SLAM_ENOMEM;
  const size_t xy = ((size_t)batch * n * m * 2 + 255) & ~(size_t)255, aa = ((size_t)batch * n * n * 2 + 255) & ~(size_t)255;
  char* w = (char*)ws;
  const int r = muon_ns((bf16_t*)x, batch, n, m, stride, partials, parts, ns_steps, (float)a, (float)b, (float)c, (float)eps,
                        (bf16_t*)w, (bf16_t*)(w + xy), (bf16_t*)(w + xy + aa), (float*)(w + xy + 2 * aa), (hipStream_t)stream);
  return r < 0 ? SLAM_EINVAL : r;
}
int slam_op_muon_syrk(const void* x, const void* r, void* c, int32_t batch, int32_t n, int32_t m, int64_t stride_x, int64_t stride_r,
                      int64_t stride_c, float alpha, float beta, slam_stream_t stream) {
  const int e = muon_syrk((const bf16_t*)x, (const bf16_t*)r, (bf16_t*)c, batch, n, m, stride_x, stride_r, stride_c, alpha, beta,
                          (hipStream_t)stream);
  return e < 0 ? SLAM_EINVAL : e;
}
int slam_op_muon_mm(const void* p, const void* x, const void* r, void* y, int32_t batch, int32_t n, int32_t m, int64_t stride_p,
                    int64_t stride_x, int64_t stride_r, int64_t stride_y, float alpha, float beta, slam_stream_t stream) {
  const int e = muon_mm((const bf16_t*)p, (const bf16_t*)x, (const bf16_t*)r, (bf16_t*)y, batch, n, m, stride_p, stride_x, stride_r,
                        stride_y, alpha, beta, (hipStream_t)stream);
  return e < 0 ? SLAM_EINVAL : e;
}

// fp32 gradient range <-> bf16 communication image (the data-parallel exchange in bf16: the reference's DDP reduces bf16
// gradients because its parameters are bf16, config/model/slam.yaml:9)
int slam_pack_grads_bf16(SlamEngine* h, int64_t offset, int64_t count, void* dst_bf16, slam_stream_t stream) {
  if (!h || !dst_bf16 || offset < 0 || count < 0 || offset + count > h->n_params || (offset & 3) || (count & 3)) return SLAM_EINVAL;
  if (!h->grads) return h->fail(SLAM_ESTATE, "no gradient buffer bound");
  if (count) CK(f32_to_bf16(h->grads + offset, (bf16_t*)dst_bf16, (size_t)count, (hipStream_t)stream));
  return SLAM_OK;
}
int slam_set_grad_image(SlamEngine* h, void* grads_bf16) {
  if (!h) return SLAM_EINVAL;
  h->grad_img = (bf16_t*)grads_bf16;
  return SLAM_OK;
}
int slam_unpack_grads_bf16(SlamEngine* h, int64_t offset, int64_t count, const void* src_bf16, slam_stream_t stream) {
  if (!h || !src_bf16 || offset < 0 || count < 0 || offset + count > h->n_params || (offset & 3) || (count & 3)) return SLAM_EINVAL;
  if (!h->grads) return h->fail(SLAM_ESTATE, "no gradient buffer bound");
  if (count) CK(bf16_to_f32((const bf16_t*)src_bf16, h->grads + offset, (size_t)count, (hipStream_t)stream));
  return SLAM_OK;
}

int slam_zero_grads(SlamEngine* h, slam_stream_t stream) {
  if (!h || !h->grads) return SLAM_EINVAL;
  CK(join_optimizer(h, (hipStream_t)stream));
  CK((int)hipMemsetAsync(h->grads, 0, (size_t)h->n_params * sizeof(float), (hipStream_t)stream));
  return SLAM_OK;
}

int slam_cast_params(SlamEngine* h, const float* master, slam_stream_t stream) {
  if (!h || !master || !h->params) return SLAM_EINVAL;
  CK(join_optimizer(h, (hipStream_t)stream));
  CK(f32_to_bf16(master, h->params, (size_t)h->n_params, (hipStream_t)stream));
  return slam_refresh_transposed(h, stream);
}

}  // extern "C"
