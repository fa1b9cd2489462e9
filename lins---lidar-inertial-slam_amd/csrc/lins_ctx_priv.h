// lins_ctx_priv.h — what the scan-to-map files of liblins_ieskf.so may use of a lins_ctx (the struct itself is
// lins_ctx.h, shared by the lins_capi*.hip files only): its stream / device, the error-string slot, and one attachment
// slot for the state of the scan-to-map row (freed by lins_destroy through the registered function).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/lins_ieskf.h"
#include "lins_buf.h"

namespace lins {
hipStream_t ctx_stream(lins_ctx* ctx);
int ctx_device(lins_ctx* ctx);
int ctx_fail_hip(lins_ctx* ctx, hipError_t e, const char* what);  // records the message, returns LINS_E_HIP
void** ctx_map_slot(lins_ctx* ctx, void (*free_fn)(void*));       // attachment slot (free_fn is remembered)
// the context's event pair for kernel timing
void ctx_events(lins_ctx* ctx, hipEvent_t* a, hipEvent_t* b);
const lins_params* ctx_params(const lins_ctx* ctx);  // the parameters the context was created with
// lins_capi_streams.hip: the clouds of a stream's last step the mapping node reads, where they lie on the device, in the
// sensor's axes (0 re-projected less sharp, 1 re-projected less flat, 2 outlier).  LINS_E_ARG for a bad stream index,
// LINS_E_STATE before the stream's first step or on a failed streams context.
struct StreamMapClouds {
  const float4* src[3];
  int n[3];
};
int streams_map_clouds(lins_ctx* ctx, int stream, StreamMapClouds* v);
void streams_slam_reset(lins_ctx* ctx);  // lins_streams_slam_capi.hip: the resident odometry records are no longer current
int streams_count(lins_ctx* ctx);  // streams of lins_streams_init (0: none, or a failed streams context)
}  // namespace lins

// every HIP call of the C API files: on failure the message goes to the context and the function returns LINS_E_HIP
#define HIP_TRY(ctx, expr)                          \
  do {                                              \
    hipError_t e__ = (expr);                        \
    if (e__ != hipSuccess) return ctx_fail_hip(ctx, e__, #expr); \
  } while (0)
// growth of a lins_buf.h buffer or group (the policy's int is the hipError_t): HIP_TRY's contract, the message names the growth
#define BUF_TRY(ctx, expr)                          \
  do {                                              \
    int e__ = (expr);                               \
    if (e__) return ctx_fail_hip(ctx, (hipError_t)e__, #expr); \
  } while (0)
