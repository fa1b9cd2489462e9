// <pcl/common/common.h> — STAND-IN (oracle/ref_shim/README.md).  StateEstimator.hpp uses nothing of it.
// lidar_mapping_node.cpp names pcl::rad2deg (the LM step's stop rule, LM:1622-1627: the real conversion), copyPointCloud
// and, in performLoopClosure (LM:1147-1166, run by ref_mapnode_driver.cpp), transformPointCloud(cloud, cloud, Matrix4f),
// getTransformation, getTranslationAndEulerAngles and Eigen::Affine3f.  Those follow PCL's documented f32 formulas
// (pcl/common/eigen.h: "create a transformation from the given translation and Euler angles (XYZ-convention)"):
//   getTransformation   A = cos yaw, B = sin yaw, C = cos pitch, D = sin pitch, E = cos roll, F = sin roll, DE = D E,
//                       DF = D F;  [A C, A DF - B E, B F + A DE, x;  B C, A E + B DF, B DE - A F, y;  -D, C F, C E, z]
//   getTranslationAndEulerAngles   x, y, z = the last column; roll = atan2(t21, t22), pitch = asin(-t20),
//                       yaw = atan2(t10, t00), the float overloads
//   Affine3f * Affine3f  linear part: 3 x 3 product, translation: lhs.linear * rhs.translation + lhs.translation, sums left
//                       to right (Eigen's own summation order inside a 4 x 4 product is stated, not pinned)
//   transformPointCloud  p' = M(0..2, 0..2) p + M(0..2, 3), intensity kept
#ifndef LINS_REF_SHIM_PCL_COMMON_
#define LINS_REF_SHIM_PCL_COMMON_
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include <cmath>
namespace Eigen {
struct Matrix4f {  // row-major storage; (i, j) as Eigen's
  float m[16];
  Matrix4f() {
    for (int i = 0; i < 16; ++i) m[i] = (i % 5 == 0) ? 1.f : 0.f;
  }
  float& operator()(int i, int j) { return m[4 * i + j]; }
  float operator()(int i, int j) const { return m[4 * i + j]; }
};
struct Affine3f {
  Matrix4f t;
  Affine3f() {}
  Affine3f(const Matrix4f& m) : t(m) {}
  Affine3f& operator=(const Matrix4f& m) {
    t = m;
    return *this;
  }
  float& operator()(int i, int j) { return t(i, j); }
  float operator()(int i, int j) const { return t(i, j); }
  Affine3f operator*(const Affine3f& o) const {
    Affine3f r;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) r(i, j) = (t(i, 0) * o(0, j) + t(i, 1) * o(1, j)) + t(i, 2) * o(2, j);
      r(i, 3) = ((t(i, 0) * o(0, 3) + t(i, 1) * o(1, 3)) + t(i, 2) * o(2, 3)) + t(i, 3);
    }
    return r;
  }
};
}  // namespace Eigen
namespace pcl {
inline float rad2deg(float alpha) { return alpha * 57.29578f; }   // pcl/common/impl/angles.hpp:46-50
inline double rad2deg(double alpha) { return alpha * 57.29578; }  // (the same literal, as PCL has it)
template <class P>
void copyPointCloud(const PointCloud<P>& in, PointCloud<P>& out) {
  out = in;
}
template <class P>
void transformPointCloud(const PointCloud<P>& in, PointCloud<P>& out, const Eigen::Matrix4f& M) {
  PointCloud<P> res = in;
  for (std::size_t i = 0; i < in.points.size(); ++i) {
    const P& p = in.points[i];
    res.points[i].x = M(0, 0) * p.x + M(0, 1) * p.y + M(0, 2) * p.z + M(0, 3);
    res.points[i].y = M(1, 0) * p.x + M(1, 1) * p.y + M(1, 2) * p.z + M(1, 3);
    res.points[i].z = M(2, 0) * p.x + M(2, 1) * p.y + M(2, 2) * p.z + M(2, 3);
  }
  out = res;
}
inline Eigen::Affine3f getTransformation(float x, float y, float z, float roll, float pitch, float yaw) {
  const float A = std::cos(yaw), B = std::sin(yaw), C = std::cos(pitch), D = std::sin(pitch), E = std::cos(roll), F = std::sin(roll);
  const float DE = D * E, DF = D * F;
  Eigen::Affine3f t;
  t(0, 0) = A * C, t(0, 1) = A * DF - B * E, t(0, 2) = B * F + A * DE, t(0, 3) = x;
  t(1, 0) = B * C, t(1, 1) = A * E + B * DF, t(1, 2) = B * DE - A * F, t(1, 3) = y;
  t(2, 0) = -D, t(2, 1) = C * F, t(2, 2) = C * E, t(2, 3) = z;
  t(3, 0) = 0.f, t(3, 1) = 0.f, t(3, 2) = 0.f, t(3, 3) = 1.f;
  return t;
}
inline void getTranslationAndEulerAngles(const Eigen::Affine3f& t, float& x, float& y, float& z, float& roll, float& pitch, float& yaw) {
  x = t(0, 3), y = t(1, 3), z = t(2, 3);
  roll = std::atan2(t(2, 1), t(2, 2));
  pitch = std::asin(-t(2, 0));
  yaw = std::atan2(t(1, 0), t(0, 0));
}
}  // namespace pcl
#endif
