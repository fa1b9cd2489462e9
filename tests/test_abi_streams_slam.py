"""Streams end to end (include/lins_streams_slam.h, include/lins_host.h): the prototypes compile as C, the ctypes mirrors
have the C structs' sizes and offsets, both libraries export the calls."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_CALLS = ("lins_streams_odometry", "lins_streams_map_step_resident", "lins_streams_fuse", "lins_streams_slam_step")
HOST_CALLS = ("lins_host_odom_from_global", "lins_host_pose_quat", "lins_host_fuse")


def test_prototypes_and_layouts_match_the_c_headers(defs):
    protos = r"""
#include "lins_streams_slam.h"
int (*a)(lins_ctx*, lins_stream_odom*) = lins_streams_odometry;
int (*b)(lins_ctx*, int, const int32_t*, const double*, const lins_slam_imu*, lins_map_step_result*) = lins_streams_map_step_resident;
int (*c)(lins_ctx*, int, const int32_t*, lins_fused_pose*) = lins_streams_fuse;
int (*d)(lins_ctx*, const lins_point* const*, const int32_t*, const int32_t*, const double* const*, const double*, const double*, double,
         const lins_slam_imu*, lins_result*, int32_t*, lins_map_step_result*, lins_fused_pose*) = lins_streams_slam_step;
void (*e)(const double*, lins_stream_odom*) = lins_host_odom_from_global;
void (*f)(const float*, double*) = lins_host_pose_quat;
void (*g)(const float*, const float*, const float*, lins_fused_pose*) = lins_host_fuse;
"""
    layout = r"""
#include <stddef.h>
#include <stdio.h>
#include "lins_streams_slam.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(lins_stream_odom), offsetof(lins_stream_odom, position),
         offsetof(lins_stream_odom, orientation), offsetof(lins_stream_odom, transform_sum), offsetof(lins_stream_odom, valid),
         sizeof(lins_fused_pose), offsetof(lins_fused_pose, transform_mapped), offsetof(lins_fused_pose, orientation),
         sizeof(lins_slam_imu), offsetof(lins_slam_imu, pitch), offsetof(lins_slam_imu, has_imu));
  return 0;
}
"""
    gcc = ["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")]
    with tempfile.TemporaryDirectory() as d:
        p, c, exe = os.path.join(d, "p.c"), os.path.join(d, "c.c"), os.path.join(d, "c")
        open(p, "w").write(protos)
        open(c, "w").write(layout)
        subprocess.check_call(gcc + ["-c", p, "-o", os.path.join(d, "p.o")])  # (a changed signature is a compile error)
        subprocess.check_call(gcc + [c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    O, F, I = defs.StreamOdomC, defs.FusedPoseC, defs.SlamImuC
    assert got == [C.sizeof(O), O.position.offset, O.orientation.offset, O.transform_sum.offset, O.valid.offset, C.sizeof(F),
                   F.transform_mapped.offset, F.orientation.offset, C.sizeof(I), I.pitch.offset, I.has_imu.offset]
    assert got[0] == 88 and got[5] == 56 and got[8] == 16  # the layouts the device records share


def test_both_libraries_export_the_calls(host, ieskf):
    for name in HOST_CALLS:
        assert hasattr(host.lib(), name), name
    for name in NEW_CALLS:
        assert name in ieskf.EXPORTS and hasattr(ieskf.lib(), name), name
