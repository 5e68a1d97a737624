// Engine-side gradient exchange over RCCL (slam_allreduce_grads_async): every slam_comm_*, the *_async
// collectives and the parameter waits they leave behind (slam_add_param_wait, slam_param_wait_*).
// Replaces, for a consumer WITHOUT torch.distributed, what accelerate's DDP wrapper does for the reference
// (/root/reference config/training_args/default.yaml:18, cli/train.py:51,61: torchrun sets RANK / WORLD_SIZE, the HF Trainer
// wraps the model in DistributedDataParallel). The Python trainer keeps issuing its collectives through torch.distributed
// (slamkit_amd/trainer/dp.py): same RCCL underneath. RCCL is NOT a link-time dependency of the engine: it is looked up at the
// first slam_comm_* call (the copy a host process has already loaded - torch's - is the one dlopen returns).
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <string.h>

// RCCL: types only - the library is looked up at run time (slam_comm_*). A box without the RCCL headers still builds the engine
// (the handful of declarations below follow rccl.h / nccl.h; their values are part of the library's stable ABI).
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
#else
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclInt8 = 0, ncclUint8 = 1, ncclInt32 = 2, ncclUint32 = 3, ncclInt64 = 4, ncclUint64 = 5, ncclFloat16 = 6, ncclFloat32 = 7,
               ncclFloat64 = 8, ncclBfloat16 = 9 } ncclDataType_t;
typedef enum { ncclSum = 0 } ncclRedOp_t;
#endif

#include "engine_impl.h"

namespace {
struct Rccl {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*ReduceScatter)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
// resolved ONCE, by whichever thread gets here first (function-local static: C++11 guarantees the others wait - a
// single-process multi-GPU consumer calls slam_comm_init from one thread per rank at the same time, ncclCommInitRank blocks
// until all have joined)
const Rccl* rccl() {
  static const Rccl r = [] {
    Rccl t;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      t.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (t.lib) break;
    }
    if (t.lib) {
      t.GetUniqueId = (decltype(t.GetUniqueId))dlsym(t.lib, "ncclGetUniqueId");
      t.CommInitRank = (decltype(t.CommInitRank))dlsym(t.lib, "ncclCommInitRank");
      t.CommDestroy = (decltype(t.CommDestroy))dlsym(t.lib, "ncclCommDestroy");
      t.AllReduce = (decltype(t.AllReduce))dlsym(t.lib, "ncclAllReduce");
      t.ReduceScatter = (decltype(t.ReduceScatter))dlsym(t.lib, "ncclReduceScatter");
      t.AllGather = (decltype(t.AllGather))dlsym(t.lib, "ncclAllGather");
      t.GetErrorString = (decltype(t.GetErrorString))dlsym(t.lib, "ncclGetErrorString");
      if (!t.GetUniqueId || !t.CommInitRank || !t.CommDestroy || !t.AllReduce || !t.ReduceScatter || !t.AllGather) t.lib = nullptr;
    }
    return t;
  }();
  return r.lib ? &r : nullptr;
}
}  // namespace

extern "C" {

int slam_comm_unique_id(void* id_out, int32_t bytes) {
  if (!id_out || bytes < (int32_t)sizeof(ncclUniqueId)) return SLAM_EINVAL;
  const Rccl* r = rccl();
  if (!r) return SLAM_EUNSUPPORTED;
  ncclUniqueId id;
  if (r->GetUniqueId(&id) != ncclSuccess) return SLAM_ESTATE;
  memcpy(id_out, &id, sizeof(id));
  return SLAM_OK;
}

int slam_comm_init(SlamEngine* h, const void* id, int32_t rank, int32_t world) {
  if (!h || !id || world <= 0 || rank < 0 || rank >= world) return SLAM_EINVAL;
  if (h->comm) return h->fail(SLAM_ESTATE, "communicator already initialised");
  const Rccl* r = rccl();
  if (!r) return h->fail(SLAM_EUNSUPPORTED, "librccl.so.1 not found");
  ncclUniqueId uid;
  memcpy(&uid, id, sizeof(uid));
  if (!h->comm_stream) CK((int)hipStreamCreateWithFlags(&h->comm_stream, hipStreamNonBlocking));  // before the communicator: nothing to undo on failure
  ncclComm_t c = nullptr;
  const ncclResult_t e = r->CommInitRank(&c, world, uid, rank);
  if (e != ncclSuccess) return h->fail(SLAM_ESTATE, r->GetErrorString ? r->GetErrorString(e) : "ncclCommInitRank failed");
  h->comm = c;
  h->comm_world = world;
  h->comm_rank = rank;
  return SLAM_OK;
}

int slam_comm_destroy(SlamEngine* h) {
  if (!h) return SLAM_EINVAL;
  if (h->comm) {
    if (h->comm_stream) (void)hipStreamSynchronize(h->comm_stream);
    const Rccl* r = rccl();
    if (r) (void)r->CommDestroy((ncclComm_t)h->comm);
    h->comm = nullptr;
    h->comm_world = 0;
  }
  return SLAM_OK;
}

int slam_allreduce_grads_async(SlamEngine* h, int64_t offset, int64_t count, int32_t bf16_exchange, slam_stream_t ready) {
  if (!h || offset < 0 || count < 0 || offset + count > h->n_params) return SLAM_EINVAL;
  if (!h->comm) return h->fail(SLAM_ESTATE, "slam_comm_init first");
  if (!h->grads) return h->fail(SLAM_ESTATE, "no gradient buffer bound");
  if (bf16_exchange && (!h->last_grad_img || (offset & 3) || (count & 3)))
    return h->fail(SLAM_ESTATE, "bf16 exchange: bind an image with slam_set_grad_image before the backward (ranges in multiples of 4)");
  if (!count) return SLAM_OK;
  const Rccl* r = rccl();
  // communication stream behind the producers of the range
  if (h->comm_ev_used == h->comm_ev.size()) {
    hipEvent_t e;
    CK((int)hipEventCreateWithFlags(&e, sync_event_flags()));  // SLAM_EVENT_SYSTEM_FENCE=1 covers the path whose data leaves the device
    h->comm_ev.push_back(e);
  }
  hipEvent_t ev = h->comm_ev[h->comm_ev_used++];
  CK((int)hipEventRecord(ev, (hipStream_t)ready));
  CK((int)hipStreamWaitEvent(h->comm_stream, ev, 0));
  ncclResult_t e;
  if (bf16_exchange) {
    bf16_t* img = h->last_grad_img + offset;
    e = r->AllReduce(img, img, (size_t)count, ncclBfloat16, ncclSum, (ncclComm_t)h->comm, h->comm_stream);
    if (e == ncclSuccess && h->gfinal != 2) CK(bf16_to_f32(img, h->grads + offset, (size_t)count, h->comm_stream));  // gfinal 2: read where they are
  } else {
    e = r->AllReduce(h->grads + offset, h->grads + offset, (size_t)count, ncclFloat32, ncclSum, (ncclComm_t)h->comm, h->comm_stream);
  }
  if (e != ncclSuccess) return h->fail(SLAM_ESTATE, r->GetErrorString ? r->GetErrorString(e) : "ncclAllReduce failed");
  return SLAM_OK;
}

}  // extern "C"

// ---- the reduce-scatter / all-gather form of the exchange (what the Python trainer runs as ddp_algo = "rs_ag"; SURVEY.md §5
// comm row, §8e: every one of a GPU's 7 xGMI links carries one shard concurrently) for the torch-free consumer -------------------
static int comm_behind(SlamEngine* h, hipStream_t ready) {  // the communication stream continues after everything on `ready`
  if (h->comm_ev_used == h->comm_ev.size()) {
    hipEvent_t e;
    CK((int)hipEventCreateWithFlags(&e, sync_event_flags()));
    h->comm_ev.push_back(e);
  }
  hipEvent_t ev = h->comm_ev[h->comm_ev_used++];
  CK((int)hipEventRecord(ev, ready));
  CK((int)hipStreamWaitEvent(h->comm_stream, ev, 0));
  return SLAM_OK;
}

extern "C" {

int slam_reduce_scatter_grads_async(SlamEngine* h, int64_t offset, int64_t count, int32_t bf16_exchange, slam_stream_t ready) {
  if (!h || offset < 0 || count < 0 || offset + count > h->n_params) return SLAM_EINVAL;
  if (!h->comm) return h->fail(SLAM_ESTATE, "slam_comm_init first");
  if (!h->grads) return h->fail(SLAM_ESTATE, "no gradient buffer bound");
  const int64_t w = h->comm_world, s = count / w;
  if (count % w || (s & 7) || (offset & 7)) return h->fail(SLAM_EINVAL, "reduce-scatter: count must be world x a multiple of 8 elements, offset a multiple of 8");
  if (bf16_exchange && !h->last_grad_img) return h->fail(SLAM_ESTATE, "bf16 exchange: bind an image with slam_set_grad_image before the backward");
  if (!count) return SLAM_OK;
  const Rccl* r = rccl();
  if (int rc = comm_behind(h, (hipStream_t)ready)) return rc;
  const int64_t mine = offset + (int64_t)h->comm_rank * s;
  ncclResult_t e;
  if (bf16_exchange) {
    bf16_t* img = h->last_grad_img;
    e = r->ReduceScatter(img + offset, img + mine, (size_t)s, ncclBfloat16, ncclSum, (ncclComm_t)h->comm, h->comm_stream);
    // gradients kept in bf16 only (grad_final_next = 2): the reduced shard is read where it is; else widen it into the fp32 buffer
    if (e == ncclSuccess && h->gfinal != 2) CK(bf16_to_f32(img + mine, h->grads + mine, (size_t)s, h->comm_stream));
  } else {
    e = r->ReduceScatter(h->grads + offset, h->grads + mine, (size_t)s, ncclFloat32, ncclSum, (ncclComm_t)h->comm, h->comm_stream);
  }
  if (e != ncclSuccess) return h->fail(SLAM_ESTATE, r->GetErrorString ? r->GetErrorString(e) : "ncclReduceScatter failed");
  return SLAM_OK;
}

int slam_allgather_params_async(SlamEngine* h, int64_t offset, int64_t count, slam_stream_t ready) {
  if (!h || offset < 0 || count < 0 || offset + count > h->n_params) return SLAM_EINVAL;
  if (!h->comm) return h->fail(SLAM_ESTATE, "slam_comm_init first");
  if (!h->params) return h->fail(SLAM_ESTATE, "bind params first");
  const int64_t w = h->comm_world, s = count / w;
  if (count % w || (s & 7) || (offset & 7)) return h->fail(SLAM_EINVAL, "all-gather: count must be world x a multiple of 8 elements, offset a multiple of 8");
  if (!count) return SLAM_OK;
  const Rccl* r = rccl();
  if (int rc = comm_behind(h, (hipStream_t)ready)) return rc;
  bf16_t* P = h->params;
  const ncclResult_t e = r->AllGather(P + offset + (int64_t)h->comm_rank * s, P + offset, (size_t)s, ncclBfloat16, (ncclComm_t)h->comm, h->comm_stream);
  if (e != ncclSuccess) return h->fail(SLAM_ESTATE, r->GetErrorString ? r->GetErrorString(e) : "ncclAllGather failed");
  // the next reader of the range (slam_forward, layer by layer) waits for the arrival right before its first read
  if (h->ag_ev_used == h->ag_ev.size()) {
    hipEvent_t ev;
    CK((int)hipEventCreateWithFlags(&ev, sync_event_flags()));
    h->ag_ev.push_back(ev);
  }
  hipEvent_t ev = h->ag_ev[h->ag_ev_used++];
  CK((int)hipEventRecord(ev, h->comm_stream));
  h->pwaits.push_back({offset, offset + count, ev});
  h->params_t_dirty = h->params_t != nullptr;
  h->w8_valid = false;
  return SLAM_OK;
}

int slam_comm_finish(SlamEngine* h, slam_stream_t stream) {
  if (!h) return SLAM_EINVAL;
  if (!h->comm_stream || !h->comm_ev_used) return SLAM_OK;
  if (h->comm_ev_used == h->comm_ev.size()) {
    hipEvent_t e;
    CK((int)hipEventCreateWithFlags(&e, sync_event_flags()));  // SLAM_EVENT_SYSTEM_FENCE=1 covers the path whose data leaves the device
    h->comm_ev.push_back(e);
  }
  hipEvent_t ev = h->comm_ev[h->comm_ev_used];
  CK((int)hipEventRecord(ev, h->comm_stream));
  CK((int)hipStreamWaitEvent((hipStream_t)stream, ev, 0));
  h->comm_ev_used = 0;  // the pool is reused by the next step (events are re-recorded; the waits above were already enqueued)
  return SLAM_OK;
}

int slam_add_param_wait(SlamEngine* h, int64_t offset, int64_t count, void* event) {
  if (!h || !event || offset < 0 || count <= 0 || offset + count > h->n_params) return SLAM_EINVAL;
  h->pwaits.push_back({offset, offset + count, (hipEvent_t)event});
  return SLAM_OK;
}

int slam_param_wait_ms(SlamEngine* h, float* total_ms) {
  if (!h || !total_ms) return SLAM_EINVAL;
  float tot = 0.f;
  for (size_t i = 0; i + 1 < h->pw_used; i += 2) {
    float ms = 0.f;
    if (hipEventSynchronize(h->pw_ev[i + 1]) == hipSuccess && hipEventElapsedTime(&ms, h->pw_ev[i], h->pw_ev[i + 1]) == hipSuccess) tot += ms;
  }
  h->pw_used = 0;
  *total_ms = tot + (float)h->pw_acc_ms;
  h->pw_acc_ms = 0.0;
  return SLAM_OK;
}

int slam_param_wait_untimed(SlamEngine* h, int64_t* n) {
  if (!h || !n) return SLAM_EINVAL;
  *n = h->pw_untimed;
  h->pw_untimed = 0;
  return SLAM_OK;
}

}  // extern "C"
