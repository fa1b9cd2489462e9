// lins_capi_dist.hip — the multi-GPU side of the C ABI (include/lins_ieskf.h): the RCCL loader, lins_rccl_* and
// lins_pose_allgather.
#include <dlfcn.h>

#include "lins_ctx.h"

using namespace lins;

namespace lins {
void rccl_free(lins_ctx* ctx) {
  auto& r = ctx->rccl;
  if (r.comm && r.comm_destroy) (void)r.comm_destroy(r.comm);
  if (r.lib) (void)dlclose(r.lib);
  r = lins_ctx::Rccl{};
}
}  // namespace lins

extern "C" {

/* ---- RCCL pose gather (ncclAllGather of the 192-byte pose records over xGMI) -------------
 * librccl is dlopen()ed on first use — the one already in the process (e.g. PyTorch's) when there is one — and never
 * linked: a build without RCCL still loads, and these calls return LINS_E_UNSUPPORTED.                            */
static int rccl_load(lins_ctx* ctx) {
  auto& r = ctx->rccl;
  if (r.lib) return LINS_OK;
  // The RCCL that belongs to the HIP runtime this library is running on: streams and events are runtime objects, so a
  // librccl bound to ANOTHER copy of libamdhip64 (a Python process may hold PyTorch's bundled ROCm beside the system's)
  // cannot take ours.  Look next to the runtime that resolved our own HIP calls first, then fall back to the loader.
  void* lib = nullptr;
  Dl_info info;
  if (dladdr(reinterpret_cast<void*>(&hipGetDeviceCount), &info) && info.dli_fname) {
    std::string dir(info.dli_fname);
    const size_t slash = dir.rfind('/');
    if (slash != std::string::npos) {
      dir.resize(slash + 1);
      lib = dlopen((dir + "librccl.so.1").c_str(), RTLD_NOW | RTLD_LOCAL);
      if (!lib) lib = dlopen((dir + "librccl.so").c_str(), RTLD_NOW | RTLD_LOCAL);
    }
  }
  if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
  if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
  if (!lib) return LINS_E_UNSUPPORTED;
  r.get_unique_id = reinterpret_cast<decltype(r.get_unique_id)>(dlsym(lib, "ncclGetUniqueId"));
  r.comm_init_rank = reinterpret_cast<decltype(r.comm_init_rank)>(dlsym(lib, "ncclCommInitRank"));
  r.all_gather = reinterpret_cast<decltype(r.all_gather)>(dlsym(lib, "ncclAllGather"));
  r.comm_destroy = reinterpret_cast<decltype(r.comm_destroy)>(dlsym(lib, "ncclCommDestroy"));
  r.get_error_string = reinterpret_cast<decltype(r.get_error_string)>(dlsym(lib, "ncclGetErrorString"));
  if (!r.get_unique_id || !r.comm_init_rank || !r.all_gather || !r.comm_destroy) {
    (void)dlclose(lib);
    r = lins_ctx::Rccl{};
    return LINS_E_UNSUPPORTED;
  }
  r.lib = lib;
  return LINS_OK;
}
static int rccl_fail(lins_ctx* ctx, ncclResult_t e, const char* what) {
  ctx->hip_err = std::string(what) + ": " + (ctx->rccl.get_error_string ? ctx->rccl.get_error_string(e) : "RCCL error");
  return LINS_E_HIP;
}

/* id128: LINS_RCCL_ID_BYTES bytes, made by ONE rank and handed to the others by whatever bootstrap the application has. */
int lins_rccl_unique_id(lins_ctx* ctx, void* id128) {
  if (!ctx || !id128) return LINS_E_ARG;
  int rc = rccl_load(ctx);
  if (rc) return rc;
  ncclUniqueId id;
  ncclResult_t e = ctx->rccl.get_unique_id(&id);
  if (e != ncclSuccess) return rccl_fail(ctx, e, "ncclGetUniqueId");
  static_assert(sizeof(id) == LINS_RCCL_ID_BYTES, "ncclUniqueId");
  std::memcpy(id128, &id, sizeof id);
  return LINS_OK;
}

int lins_rccl_init(lins_ctx* ctx, const void* id128, int rank, int world) {
  if (!ctx || !id128 || world < 1 || rank < 0 || rank >= world) return LINS_E_ARG;
  if (ctx->rccl.comm) return LINS_E_STATE;
  int rc = rccl_load(ctx);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ncclUniqueId id;
  std::memcpy(&id, id128, sizeof id);
  ncclResult_t e = ctx->rccl.comm_init_rank(&ctx->rccl.comm, world, id, rank);
  if (e != ncclSuccess) return rccl_fail(ctx, e, "ncclCommInitRank");
  ctx->rccl.rank = rank, ctx->rccl.world = world;
  return LINS_OK;
}

/* All-gather of fixed-size pieces: every rank contributes n_records pose records at d_local (device), d_all (device)
 * receives world x n_records records in rank order.  Stream-ordered after the last lins_batch_run(): in pipelined mode
 * on the context's communication stream (beside the next run), otherwise on the compute stream.  No host wait.     */
int lins_pose_allgather(lins_ctx* ctx, const void* d_local, int n_records, void* d_all) {
  if (!ctx || !d_local || !d_all || n_records < 0) return LINS_E_ARG;
  if (!ctx->rccl.comm) return LINS_E_STATE;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  auto& q = ctx->pipe;
  hipStream_t st = ctx->stream;
  int set = 0;
  if (q.on) {
    if (q.runs == 0) return LINS_E_STATE;
    set = (int)((q.runs - 1) & 1u);  // the run whose records these are
    HIP_TRY(ctx, hipStreamWaitEvent(q.s_comm, ctx->hist1[q.h_of[set]], 0));
    if (q.run_split[set]) HIP_TRY(ctx, hipStreamWaitEvent(q.s_comm, ctx->hist1b[q.h_of[set]], 0));  // (both launch queues; the queues themselves are not joined)
    st = q.s_comm;
  } else if (int rcs = split_join(ctx)) {  // (the gather runs on the context's stream: behind the second launch queue too)
    return rcs;
  }
  ncclResult_t e = ctx->rccl.all_gather(d_local, d_all, (size_t)n_records * sizeof(lins_pose_record), ncclChar, ctx->rccl.comm, st);
  if (e != ncclSuccess) return rccl_fail(ctx, e, "ncclAllGather");
  if (q.on) {
    HIP_TRY(ctx, hipEventRecord(q.ev_comm[set], q.s_comm));
    q.comm_pending[set] = true;
  }
  return LINS_OK;
}

int lins_rccl_destroy(lins_ctx* ctx) {
  if (!ctx) return LINS_E_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (ctx->pipe.s_comm) HIP_TRY(ctx, hipStreamSynchronize(ctx->pipe.s_comm));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  rccl_free(ctx);
  return LINS_OK;
}

}  // extern "C"
