// map_pose.cpp — the mapping node's pose arithmetic on the CPU: transformAssociateToMap (LM:411-536), the tail of
// transformUpdate (LM:567-576) and the key-frame rule (LM:1655-1671).  The restatement map_associate_kernel and
// map_pose_finish_kernel (csrc/map_pose_kernels.hip) are checked against; the arithmetic is csrc/map_pose_math.h in
// both libraries.

#include "../../../include/lins_host.h"
#include "../map_pose_math.h"

extern "C" void lins_host_map_associate(const float bef[6], const float aft[6], const float sum[6], float tobe[6]) {
  lins_mp::mp_associate(bef, aft, sum, tobe);
}

extern "C" void lins_host_map_transform_update(float tobe[6], int has_imu, float imu_roll, float imu_pitch, const float sum[6], float bef[6],
                                               float aft[6]) {
  lins_mp::mp_transform_update(tobe, has_imu, imu_roll, imu_pitch, sum, bef, aft);
}

extern "C" int lins_host_map_key_rule(float prev[3], const float aft[6], int have_frames) { return lins_mp::mp_key_rule(prev, aft, have_frames); }
