// odom.cpp — the seam between the filter and the mapping node on the CPU: globalState_ to /laser_odom_to_init and
// transformSum (SE:1150-1154, EC:294-305, LM:711-724), the published orientation of a pose (TF:235-242) and the transform
// fusion node (TF:91-254).  The restatement odom_record_kernel and odom_fuse_kernel (csrc/odom_kernels.hip) are checked
// against; the arithmetic is csrc/odom_math.h in both libraries.

#include "../../../include/lins_host.h"
#include "../odom_math.h"

extern "C" void lins_host_odom_from_global(const double* gs19, lins_stream_odom* out) { lins_od::odom_record(gs19, 1, out); }

extern "C" void lins_host_pose_quat(const float* t6, double* q4) { lins_od::pose_quat(t6, q4); }

extern "C" void lins_host_fuse(const float* bef6, const float* aft6, const float* sum6, lins_fused_pose* out) {
  lins_od::odom_fuse(bef6, aft6, sum6, out);
}
