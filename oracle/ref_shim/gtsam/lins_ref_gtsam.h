// gtsam — STAND-IN (oracle/ref_shim/README.md).  lidar_mapping_node.cpp is ONE class; its scan-to-map optimisation
// (LM:1351-1652), which ref_map_driver.cpp runs, never touches GTSAM; its key-frame / loop-closure methods, which
// ref_mapnode_driver.cpp runs, do.  Written from GTSAM's documented behaviour, none of it from GTSAM's sources:
//   Point3 / Rot3 / Pose3   carry values.  Rot3::RzRyRx(x, y, z) is R = Rz(z) Ry(y) Rx(x) in f64 and KEEPS its three
//                           angles: roll() / pitch() / yaw() return them as given.  A rotation that comes out of a product
//                           (compose, between) has no kept angles; there roll = atan2(R21, R22), pitch = asin(-R20),
//                           yaw = atan2(R10, R00).
//   compose / between       (R1 R2, t1 + R1 t2) and inverse().compose(), f64, through the rotation matrix, every sum
//                           left to right.  between() also records its two operands (last_between()), so a driver can
//                           read the poses a factor's measurement was made from.
//   Values                  index -> Pose3: insert, at, size, clear (at() of a missing index: a default Pose3).
//   NonlinearFactorGraph    keeps what was added (prior: index + pose; between: two indices + measurement; the variances).
//   ISAM2                   update(graph, values) stores the values and appends the graph's factors to `factors`, the log
//                           the driver reads; calculateEstimate() returns the stored values.  That is the project's own
//                           stated contract for a loop-free graph (a chain whose initial values satisfy every factor
//                           exactly has them as its optimum).  With a loop factor it SOLVES NOTHING: the driver writes
//                           the estimate.
// STATED, NOT PINNED: real iSAM2's rounding (and the angle extraction of a real Rot3, which goes through a
// decomposition of R) is not knowable here.
#ifndef LINS_REF_SHIM_GTSAM_
#define LINS_REF_SHIM_GTSAM_
#include <boost/shared_ptr.hpp>
#include <eigen3/Eigen/Dense>

#include <cmath>
#include <cstddef>
#include <map>
#include <vector>
namespace gtsam {
typedef Eigen::VectorXd Vector;
struct Point3 {
  double v[3];
  Point3() { v[0] = v[1] = v[2] = 0.0; }
  Point3(double x, double y, double z) { v[0] = x, v[1] = y, v[2] = z; }
  double x() const { return v[0]; }
  double y() const { return v[1]; }
  double z() const { return v[2]; }
};
struct Rot3 {
  double R[9];  // row-major
  double a[3];  // the angles RzRyRx was given
  bool kept;
  Rot3() : kept(true) {
    for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    a[0] = a[1] = a[2] = 0.0;
  }
  static Rot3 RzRyRx(double x, double y, double z) {
    Rot3 r;
    r.a[0] = x, r.a[1] = y, r.a[2] = z;
    const double cx = std::cos(x), sx = std::sin(x), cy = std::cos(y), sy = std::sin(y), cz = std::cos(z), sz = std::sin(z);
    r.R[0] = cz * cy, r.R[1] = cz * sy * sx - sz * cx, r.R[2] = cz * sy * cx + sz * sx;
    r.R[3] = sz * cy, r.R[4] = sz * sy * sx + cz * cx, r.R[5] = sz * sy * cx - cz * sx;
    r.R[6] = -sy, r.R[7] = cy * sx, r.R[8] = cy * cx;
    return r;
  }
  double roll() const { return kept ? a[0] : std::atan2(R[7], R[8]); }
  double pitch() const { return kept ? a[1] : std::asin(-R[6]); }
  double yaw() const { return kept ? a[2] : std::atan2(R[3], R[0]); }
  Rot3 operator*(const Rot3& o) const {
    Rot3 r;
    r.kept = false;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) r.R[3 * i + j] = (R[3 * i] * o.R[j] + R[3 * i + 1] * o.R[3 + j]) + R[3 * i + 2] * o.R[6 + j];
    return r;
  }
  Rot3 inverse() const {
    Rot3 r;
    r.kept = false;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) r.R[3 * i + j] = R[3 * j + i];
    return r;
  }
  Point3 operator*(const Point3& p) const {
    return Point3((R[0] * p.v[0] + R[1] * p.v[1]) + R[2] * p.v[2], (R[3] * p.v[0] + R[4] * p.v[1]) + R[5] * p.v[2],
                  (R[6] * p.v[0] + R[7] * p.v[1]) + R[8] * p.v[2]);
  }
};
struct Pose3 {
  Rot3 r;
  Point3 t;
  Pose3() {}
  Pose3(const Rot3& r_, const Point3& t_) : r(r_), t(t_) {}
  Pose3 compose(const Pose3& o) const {
    const Point3 rt = r * o.t;
    return Pose3(r * o.r, Point3(t.v[0] + rt.v[0], t.v[1] + rt.v[1], t.v[2] + rt.v[2]));
  }
  Pose3 inverse() const {
    const Rot3 ri = r.inverse();
    return Pose3(ri, ri * Point3(-t.v[0], -t.v[1], -t.v[2]));
  }
  inline Pose3 between(const Pose3& o) const;
  Point3 translation() const { return t; }
  Rot3 rotation() const { return r; }
};
struct BetweenCall {
  Pose3 from, to;
};
inline BetweenCall& last_between() {
  static thread_local BetweenCall c;
  return c;
}
inline Pose3 Pose3::between(const Pose3& o) const {
  last_between().from = *this, last_between().to = o;
  return inverse().compose(o);
}
namespace noiseModel {
struct Diagonal {
  typedef boost::shared_ptr<Diagonal> shared_ptr;
  std::vector<double> variances;
  static shared_ptr Variances(const Vector& v) {
    shared_ptr d(new Diagonal());
    for (int i = 0; i < (int)v.size(); ++i) d->variances.push_back(v(i));
    return d;
  }
};
}  // namespace noiseModel
struct FactorRecord {  // what a graph remembers of a factor: a prior has j == i
  bool prior;
  std::size_t i, j;
  Pose3 z;
  std::vector<double> variances;
};
template <class T>
struct PriorFactor {
  FactorRecord rec;
  PriorFactor(std::size_t i, const T& z, const noiseModel::Diagonal::shared_ptr& n) {
    rec.prior = true, rec.i = rec.j = i, rec.z = z;
    if (n) rec.variances = n->variances;
  }
};
template <class T>
struct BetweenFactor {
  FactorRecord rec;
  BetweenFactor(std::size_t i, std::size_t j, const T& z, const noiseModel::Diagonal::shared_ptr& n) {
    rec.prior = false, rec.i = i, rec.j = j, rec.z = z;
    if (n) rec.variances = n->variances;
  }
};
struct NonlinearFactorGraph {
  std::vector<FactorRecord> factors;
  template <class F>
  void add(const F& f) {
    factors.push_back(f.rec);
  }
  void resize(std::size_t n) { factors.resize(n); }
};
struct Values {
  std::map<std::size_t, Pose3> poses;
  template <class T>
  void insert(std::size_t i, const T& p) {
    poses[i] = p;
  }
  void clear() { poses.clear(); }
  std::size_t size() const { return poses.size(); }
  template <class T>
  T at(std::size_t i) const {
    std::map<std::size_t, Pose3>::const_iterator it = poses.find(i);
    return it == poses.end() ? T() : it->second;
  }
};
struct ISAM2Params {
  double relinearizeThreshold;
  int relinearizeSkip;
  ISAM2Params() : relinearizeThreshold(0), relinearizeSkip(0) {}
};
struct ISAM2 {
  Values estimate;
  std::vector<FactorRecord> factors;  // every factor ever handed over, in order
  explicit ISAM2(const ISAM2Params&) {}
  void update() {}
  void update(const NonlinearFactorGraph& g) { factors.insert(factors.end(), g.factors.begin(), g.factors.end()); }
  void update(const NonlinearFactorGraph& g, const Values& v) {
    update(g);
    for (std::map<std::size_t, Pose3>::const_iterator it = v.poses.begin(); it != v.poses.end(); ++it) estimate.poses[it->first] = it->second;
  }
  Values calculateEstimate() const { return estimate; }
};
}  // namespace gtsam
#endif
