// snapshot_kernels.hip — the two kernels of a stream snapshot (include/lins_snapshot.h): snap_pack gathers every
// device-resident piece of all streams of a call into one staging buffer — the device part of the blobs, byte for byte —
// and snap_unpack scatters such a buffer to where the pieces live.  A slot's key frames are interleaved with every other
// slot's in the archive's arena, so a robot of 2 000 key frames is 2 000 runs; the ring, the scan and the rows add dozens
// more: one table-driven launch per unit size replaces thousands of copies.
//
// Shape: that of the ar_reclaim_* kernels (archive_kernels.hip).  One workgroup of kLmTile lanes per (segment, tile)
// entry of the uploaded table; the module buffers are a small array of base pointers in that table, indexed by the
// segment's buffer id; one unit per lane — a float4 for the clouds, 8 bytes for the rows that are multiples of 8 but not
// of 16 bytes (the same kernel instantiated for that unit); one guarded block, no early return, no LDS, no atomics, no
// cross-lane operation.  What keeps a lane inside the buffers is the table alone: the plan of host/snapshot_format.h,
// whose segments are disjoint and within the buffers' sizes (segments_ok) before the table is uploaded.
#include <hip/hip_runtime.h>

#include "../../include/lins_snapshot.h"
#include "lins_launch.h"
#include "local_map.h"

namespace lins {
namespace {

template <class U>
__global__ __launch_bounds__(kLmTile) void snap_pack_kernel(const lins_snapshot_segment* __restrict__ segs, const int2* __restrict__ tiles,
                                                            void* const* __restrict__ bases, char* __restrict__ stage) {
  const int2 b = tiles[blockIdx.x];
  const lins_snapshot_segment& s = segs[b.x];
  const long long i = (long long)b.y * kLmTile + threadIdx.x;
  if (i < s.units) ((U*)stage)[s.stg_off + i] = ((const U*)bases[s.buffer])[s.buf_off + i];
}

template <class U>
__global__ __launch_bounds__(kLmTile) void snap_unpack_kernel(const lins_snapshot_segment* __restrict__ segs, const int2* __restrict__ tiles,
                                                              void* const* __restrict__ bases, const char* __restrict__ stage) {
  const int2 b = tiles[blockIdx.x];
  const lins_snapshot_segment& s = segs[b.x];
  const long long i = (long long)b.y * kLmTile + threadIdx.x;
  if (i < s.units) ((U*)bases[s.buffer])[s.buf_off + i] = ((const U*)stage)[s.stg_off + i];
}

}  // namespace

void launch_snap_pack(hipStream_t s, int unit, int n_tiles, const lins_snapshot_segment* segs, const int2* tiles, void* const* bases, char* stage) {
  if (!n_tiles) return;
  if (unit == 16) hipLaunchKernelGGL(snap_pack_kernel<float4>, dim3(n_tiles), dim3(kLmTile), 0, s, segs, tiles, bases, stage);
  else hipLaunchKernelGGL(snap_pack_kernel<unsigned long long>, dim3(n_tiles), dim3(kLmTile), 0, s, segs, tiles, bases, stage);
}

void launch_snap_unpack(hipStream_t s, int unit, int n_tiles, const lins_snapshot_segment* segs, const int2* tiles, void* const* bases, const char* stage) {
  if (!n_tiles) return;
  if (unit == 16) hipLaunchKernelGGL(snap_unpack_kernel<float4>, dim3(n_tiles), dim3(kLmTile), 0, s, segs, tiles, bases, stage);
  else hipLaunchKernelGGL(snap_unpack_kernel<unsigned long long>, dim3(n_tiles), dim3(kLmTile), 0, s, segs, tiles, bases, stage);
}

}  // namespace lins
