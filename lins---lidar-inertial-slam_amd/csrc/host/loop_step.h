// loop_step.h — what the loop thread DECIDES between its device stages (performLoopClosure, LM:1033-1186), defined ONCE
// and compiled into both libraries (lins_loop_step and lins_host_loop_window / _candidate / _accept / _variance; DESIGN.md
// §5.3 "Loop thread's step").  Scalar host work in the style of keyframe_select.h:
//   window     the ids closest - H .. closest + H, clipped to [0, latest], ascending (LM:1087-1098); it may contain
//              `latest` itself, as in the reference.
//   candidate  closest < 0: no loop.  closest == latest: no loop — a departure: the reference would add a factor of a frame
//              with itself (a robot standing still for longer than the time gap finds its own latest frame first).
//              (latest, closest) equal to the pair of the slot's most recent loop factor: a repeat, nothing is aligned or
//              added — a departure: the reference adds the same factor again every second while no new key frame arrives,
//              and the loops' core is dense, at most 64 loops a slot.
//   accept     converged && !(fitness > (double)max_fitness) (LM:1140-1141): max_fitness is the f32
//              historyKeyframeFitnessScore promoted as the reference's comparison promotes it.  A fitness of exactly
//              (double)0.3f passes, DBL_MAX (no source point found a target) does not; a NaN passes HERE, as it passes the
//              reference's expression, and is stopped by the variance.
//   variance   (double)(float)fitness (LM:1171-1175); not finite or not > 0: a rejection (lins_pose_graph_add_loop would
//              refuse it with LINS_E_INPUT).
// Also the camera / lidar frame shuffle of LM:1156-1166 (pose_from), all f32.
#pragma once
#include <stdint.h>

#include <cmath>

#include "../../../include/lins_host.h"

namespace lins_loop {

constexpr int kAlign = -1;  // candidate(): neither "no loop" nor a repeat — the pair goes to the alignment

// ids[0 .. return) = the window; ids holds at least window_size(latest, closest, H) entries.  latest < 0 (no frames),
// closest outside [0, latest] or H < 0: empty.
inline int window_size(int latest, int closest, int H) {
  if (latest < 0 || closest < 0 || closest > latest || H < 0) return 0;
  const long long lo = (long long)closest - H > 0 ? (long long)closest - H : 0;
  const long long hi = (long long)closest + H < latest ? (long long)closest + H : latest;
  return hi - lo + 1 > 2147483647ll ? 2147483647 : (int)(hi - lo + 1);  // (every frame of a slot that holds INT_MAX + 1 of them)
}
inline int window(int latest, int closest, int H, int32_t* ids) {
  const int n = window_size(latest, closest, H);
  const int lo = n && closest > H ? closest - H : 0;
  for (int i = 0; i < n; ++i) ids[i] = lo + i;
  return n;
}

// LINS_LOOP_NONE, LINS_LOOP_REPEAT or kAlign.  last_latest / last_closest: the pair of the slot's most recent loop
// factor, -1 / -1 without one.
inline int candidate(int latest, int closest, int last_latest, int last_closest) {
  if (latest < 0 || closest < 0 || closest >= latest) return LINS_LOOP_NONE;  // (closest > latest: not a frame)
  if (latest == last_latest && closest == last_closest) return LINS_LOOP_REPEAT;
  return kAlign;
}

inline bool accept(int converged, double fitness, float max_fitness) { return converged && !(fitness > (double)max_fitness); }

// lins_loop_step_place's choice among the k candidates the ICP verified: the rank of the smallest fitness among those
// `accept` accepts, the lower rank at a tie, -1 when none is.  (A NaN passes `accept`; it is "smallest" only when every
// accepted fitness is a NaN — the variance rule then rejects the entry.)
inline int choose(int k, const int32_t* converged, const double* fitness, float max_fitness) {
  int at = -1;
  for (int j = 0; j < k; ++j) {
    if (!accept(converged[j], fitness[j], max_fitness)) continue;
    if (at < 0 || fitness[j] < fitness[at] || (std::isnan(fitness[at]) && !std::isnan(fitness[j]))) at = j;
  }
  return at;
}

// false: a rejection; *var is the factor's variance either way
inline bool variance(double fitness, double* var) {
  const double v = (double)(float)fitness;
  if (var) *var = v;
  return std::isfinite(v) && v > 0.0;
}

// getTransformation(x, y, z, roll, pitch, yaw) = Rz(yaw) Ry(pitch) Rx(roll) with translation (x, y, z); f32 in the
// reference's text (pose_from below), f64 for the place-recognition guess (key_pose_matrix)
template <class T>
inline void get_transformation(T x, T y, T z, T roll, T pitch, T yaw, T* t) {
  const T cr = std::cos(roll), sr = std::sin(roll), cp = std::cos(pitch), sp = std::sin(pitch), cy = std::cos(yaw), sy = std::sin(yaw);
  t[0] = cy * cp, t[1] = cy * sp * sr - sy * cr, t[2] = cy * sp * cr + sy * sr, t[3] = x;
  t[4] = sy * cp, t[5] = sy * sp * sr + cy * cr, t[6] = sy * sp * cr - cy * sr, t[7] = y;
  t[8] = -sp, t[9] = cp * sr, t[10] = cp * cr, t[11] = z;
  t[12] = t[13] = t[14] = T(0), t[15] = T(1);
}
// A stored key pose as a 4 x 4 in the axes it is stored in (the mapping node's camera axes), f64: pose_from's
// pclPointToAffine3fCameraToLidar — getTransformation(z, x, y, yaw, roll, pitch), in lidar axes (x, y, z) = camera (z, x, y) —
// taken back to camera axes.  It is Ry(pitch) Rx(roll) Rz(yaw) with translation (x, y, z): what the archive's assembly
// applies to a frame's points (lm_transform_kernel).
inline void key_pose_matrix(const lins_key_pose& p, double* M) {
  double L[16];
  get_transformation<double>(p.z, p.x, p.y, p.yaw, p.roll, p.pitch, L);
  const int lidar_of[3] = {1, 2, 0};  // camera axis -> the lidar axis that is the same direction
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) M[4 * i + j] = L[4 * lidar_of[i] + lidar_of[j]];
    M[4 * i + 3] = L[4 * lidar_of[i] + 3];
  }
  M[12] = M[13] = M[14] = 0.0, M[15] = 1.0;
}
// getTranslationAndEulerAngles
inline void euler_of(const float* t, float& x, float& y, float& z, float& roll, float& pitch, float& yaw) {
  x = t[3], y = t[7], z = t[11];
  roll = std::atan2(t[9], t[10]), pitch = std::asin(-t[8]), yaw = std::atan2(t[4], t[0]);
}
// LM:1156-1166 (lins_host_loop_pose_from)
inline void pose_from(const double T[16], const lins_key_pose& wrong, lins_key_pose* out) {
  float c[16], x, y, z, roll, pitch, yaw;
  for (int i = 0; i < 16; ++i) c[i] = (float)T[i];  // icp.getFinalTransformation() is a Matrix4f
  euler_of(c, x, y, z, roll, pitch, yaw);
  float lidar[16], tw[16], tc[16];
  get_transformation(z, x, y, yaw, roll, pitch, lidar);
  get_transformation(wrong.z, wrong.x, wrong.y, wrong.yaw, wrong.roll, wrong.pitch, tw);  // pclPointToAffine3fCameraToLidar
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) tc[4 * i + j] = ((lidar[4 * i] * tw[j] + lidar[4 * i + 1] * tw[4 + j]) + lidar[4 * i + 2] * tw[8 + j]) + lidar[4 * i + 3] * tw[12 + j];
  euler_of(tc, out->x, out->y, out->z, out->roll, out->pitch, out->yaw);
}

}  // namespace lins_loop
