// ref_mapnode_driver.cpp — the REFERENCE'S OWN lidar_mapping_node.cpp compiled verbatim into
// oracle/_ref/liblins_ref_mapnode.so: the BOOKKEEPING of the mapping node — transformAssociateToMap, transformUpdate,
// extractSurroundingKeyFrames (both branches), downsampleCurrentScan, saveKeyFramesAndFactor, correctPoses,
// detectLoopClosure, performLoopClosure's glue, publishGlobalMap and run() itself (LM:411-577, 984-1349, 1654-1855) — on
// one persistent MappingHandler per handle, fed and read through a C interface.
//
// TEST INFRASTRUCTURE ONLY (oracle/): loaded by tests/ through oracle/ref_mapnode.py; never by the product.
//
// As in ref_map_driver.cpp the node's text is compiled with `private` spelled `public` and `main` renamed, after every
// standard and stand-in header has been included under its own guard; no line of the node is changed.  One more swap:
// `loopClosureEnableFlag` is a const of parameters.h (true).  parameters.h is included first, under its own guard; after
// that the NAME is a macro for a variable of this file, so the two branches of LM:1204 and the gate of LM:1034 can both be
// run.  Two definitions of one class do not share a library, hence a library of its own (as liblins_ref_seq.so).
//
// What runs against stand-ins (oracle/ref_shim/README.md): GTSAM (values carried, loop-free iSAM2 returns its initial
// values, with a loop factor the DRIVER writes the estimate: set_estimate), PCL's ICP (answers what the driver set), the
// PCL transforms (documented f32 formulas), VoxelGrid, radiusSearch (by distance, then index), tf (the conversions return
// identities: publishTF / publishXYZTF run and publish nothing that is read here).
//
// OUT OF SCOPE: the four message handlers and imuHandler go through tf and quaternions (LM:688-735); feed() and imu() set
// the members those handlers set, from values already in the node's own representation.
#include <math_utils.h>
#include <parameters.h>

#include <gtsam/lins_ref_gtsam.h>
#include <pcl/registration/icp.h>
#include <sensor_msgs/PointCloud2.h>

#include <cstring>
#include <deque>
#include <iostream>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../include/lins_map.h"

static bool lins_ref_mapnode_loop_flag = true;

#define loopClosureEnableFlag (::lins_ref_mapnode_loop_flag)
#define private public
#define main lins_ref_lidar_mapping_node_main
#include <lidar_mapping_node.cpp>
#undef main
#undef private
#undef loopClosureEnableFlag

namespace parameter {  // lins/src/lib/parameters.cpp declares these; values: config/exp_config/exp_port.yaml (as ref_params.inc)
int LINE_NUM = 16;
int SCAN_NUM = 1800;
double SCAN_PERIOD = 0.1;
int VERBOSE = 0;
void readParameters(ros::NodeHandle&) {}  // (yaml reading; only the node's main(), never called, names it)
}  // namespace parameter

namespace {

typedef pcl::PointCloud<PointType> Cloud;

struct Node {
  ros::NodeHandle nh, pnh;
  MappingHandler h;
  bool flag;
  explicit Node(bool f) : nh(), pnh("~"), h(nh, pnh), flag(f) {}
};

// every call enters the node's text with its own handle's flag
struct Enter {
  explicit Enter(Node* n) { lins_ref_mapnode_loop_flag = n->flag; }
};

void fill(Cloud::Ptr& c, const lins_point* p, int n) {
  c->points.resize(n);
  for (int i = 0; i < n; ++i) c->points[i].x = p[i].x, c->points[i].y = p[i].y, c->points[i].z = p[i].z, c->points[i].intensity = p[i].intensity;
  c->width = (std::uint32_t)n, c->height = 1;
}

int copy_out(const std::vector<PointType>& pts, lins_point* out, int cap) {
  const int n = (int)pts.size();
  for (int i = 0; i < n && i < cap; ++i) out[i].x = pts[i].x, out[i].y = pts[i].y, out[i].z = pts[i].z, out[i].intensity = pts[i].intensity;
  return n;
}

bool same(const std::vector<PointType>& a, const std::vector<PointType>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(PointType)) == 0);
}
bool same(const Cloud::Ptr& a, const Cloud::Ptr& b) { return same(a->points, b->points); }
template <class Seq>
bool same_seq(const Seq& a, const Seq& b) {
  if (a.size() != b.size()) return false;
  for (std::size_t i = 0; i < a.size(); ++i)
    if (!same(a[i], b[i])) return false;
  return true;
}
bool same_pose(const gtsam::Pose3& a, const gtsam::Pose3& b) {
  return std::memcmp(a.r.R, b.r.R, sizeof a.r.R) == 0 && std::memcmp(a.t.v, b.t.v, sizeof a.t.v) == 0;
}

const Cloud* pick(Node* n, int which, int id) {
  MappingHandler& h = n->h;
  switch (which) {
    case 0: return id >= 0 && id < (int)h.cornerCloudKeyFrames.size() ? h.cornerCloudKeyFrames[id].get() : nullptr;
    case 1: return id >= 0 && id < (int)h.surfCloudKeyFrames.size() ? h.surfCloudKeyFrames[id].get() : nullptr;
    case 2: return id >= 0 && id < (int)h.outlierCloudKeyFrames.size() ? h.outlierCloudKeyFrames[id].get() : nullptr;
    case 3: return h.laserCloudCornerFromMap.get();
    case 4: return h.laserCloudSurfFromMap.get();
    case 5: return h.laserCloudCornerFromMapDS.get();
    case 6: return h.laserCloudSurfFromMapDS.get();
    case 7: return h.laserCloudCornerLast.get();
    case 8: return h.laserCloudSurfLast.get();
    case 9: return h.laserCloudCornerLastDS.get();
    case 10: return h.laserCloudSurfLastDS.get();
    case 11: return h.laserCloudOutlierLastDS.get();
    case 12: return h.laserCloudSurfTotalLast.get();
    case 13: return h.laserCloudSurfTotalLastDS.get();
    case 14: return h.latestSurfKeyFrameCloud.get();
    case 15: return h.nearHistorySurfKeyFrameCloud.get();
    case 16: return h.nearHistorySurfKeyFrameCloudDS.get();
    case 17: return &lins_ref_shim::icp_call().source;
    case 18: return &lins_ref_shim::icp_call().target;
    case 19: return id >= 0 && id < (int)h.recentCornerCloudKeyFrames.size() ? h.recentCornerCloudKeyFrames[id].get() : nullptr;
    case 20: return id >= 0 && id < (int)h.recentSurfCloudKeyFrames.size() ? h.recentSurfCloudKeyFrames[id].get() : nullptr;
    case 21: return id >= 0 && id < (int)h.recentOutlierCloudKeyFrames.size() ? h.recentOutlierCloudKeyFrames[id].get() : nullptr;
    case 22: return h.surroundingKeyPosesDS.get();
    case 23: return id >= 0 && id < (int)h.surroundingCornerCloudKeyFrames.size() ? h.surroundingCornerCloudKeyFrames[id].get() : nullptr;
    default: return nullptr;
  }
}

float* transform_of(MappingHandler& h, int what) {
  switch (what) {
    case 0: return h.transformLast;
    case 1: return h.transformSum;
    case 2: return h.transformIncre;
    case 3: return h.transformTobeMapped;
    case 4: return h.transformBefMapped;
    case 5: return h.transformAftMapped;
    default: return nullptr;
  }
}

}  // namespace

extern "C" {

void* ref_mapnode_create(int loop_flag) { return new Node(loop_flag != 0); }
void ref_mapnode_destroy(void* p) { delete static_cast<Node*>(p); }

// what laserCloudCornerLastHandler / ...SurfLast... / ...OutlierLast... / laserOdometryHandler leave behind (LM:688-724):
// the three clouds, the four time stamps (all `time`), the four new* flags, transformSum
int ref_mapnode_feed(void* p, const lins_point* corner, int n_corner, const lins_point* surf, int n_surf, const lins_point* outlier, int n_outlier,
                     const float transform_sum[6], double time) {
  if (!p || n_corner < 0 || n_surf < 0 || n_outlier < 0 || !transform_sum) return -1;
  MappingHandler& h = static_cast<Node*>(p)->h;
  h.timeLaserCloudCornerLast = h.timeLaserCloudSurfLast = h.timeLaserCloudOutlierLast = h.timeLaserOdometry = time;
  fill(h.laserCloudCornerLast, corner, n_corner);
  fill(h.laserCloudSurfLast, surf, n_surf);
  fill(h.laserCloudOutlierLast, outlier, n_outlier);
  for (int i = 0; i < 6; ++i) h.transformSum[i] = transform_sum[i];
  h.newLaserCloudCornerLast = h.newLaserCloudSurfLast = h.newLaserCloudOutlierLast = h.newLaserOdometry = true;
  return 0;
}

// What imuHandler leaves behind (LM:726-735) for a message of this stamp whose orientation has this roll and pitch: one
// more entry of the ring of imuQueLength_ samples.  A RESTATEMENT by the driver — the handler itself takes a message and
// goes through tf's quaternion conversion (out of scope) — of four assignments: advance the write index modulo the ring's
// length, store the stamp, store the two angles narrowed to the arrays' float.
int ref_mapnode_imu(void* p, double time, double roll, double pitch) {
  if (!p) return -1;
  MappingHandler& h = static_cast<Node*>(p)->h;
  const int slot = h.imuPointerLast + 1 == imuQueLength_ ? 0 : h.imuPointerLast + 1;
  h.imuTime[slot] = time;
  h.imuRoll[slot] = static_cast<float>(roll);
  h.imuPitch[slot] = static_cast<float>(pitch);
  h.imuPointerLast = slot;
  return 0;
}

// set the node's six-float arrays / robot points directly (what: as ref_mapnode_floats), to start a case from a given state
int ref_mapnode_set_floats(void* p, int what, const float* v) {
  if (!p || !v) return -1;
  MappingHandler& h = static_cast<Node*>(p)->h;
  if (float* t = transform_of(h, what)) {
    for (int i = 0; i < 6; ++i) t[i] = v[i];
    return 0;
  }
  if (what == 6 || what == 7) {
    PointType& q = what == 6 ? h.previousRobotPosPoint : h.currentRobotPosPoint;
    q.x = v[0], q.y = v[1], q.z = v[2], q.intensity = v[3];
    return 0;
  }
  return -1;
}
int ref_mapnode_set_time(void* p, double time_laser_odometry) {
  if (!p) return -1;
  static_cast<Node*>(p)->h.timeLaserOdometry = time_laser_odometry;
  return 0;
}

// run() -> 1 when the scan went through the mapping step (LM:1821), 0 when a gate held it back
int ref_mapnode_run(void* p) {
  if (!p) return -1;
  Node* n = static_cast<Node*>(p);
  Enter e(n);
  const double before = n->h.timeLastProcessing;
  const bool fresh = n->h.newLaserOdometry;
  n->h.run();
  return fresh && !n->h.newLaserOdometry && n->h.timeLastProcessing != before ? 1 : 0;
}

namespace {
// The gate of run() (LM:1807-1824), RESTATED by the driver as three predicates — the only lines of run() that are not a
// call of a member function, and so the only ones the staged form cannot take from the node.  Not the node's text: its
// fidelity is what ref_mapnode_same_state checks against a handle driven by run() itself, at every step of a sequence
// that contains a scan the interval holds back (tests/test_ref_mapnode.py, section j).
bool stamped_with_the_odometry(double t_cloud, double t_odometry) { return std::fabs(t_cloud - t_odometry) < 0.005; }
bool all_four_arrived(const MappingHandler& h) {
  return h.newLaserOdometry && h.newLaserCloudCornerLast && h.newLaserCloudSurfLast && h.newLaserCloudOutlierLast &&
         stamped_with_the_odometry(h.timeLaserCloudCornerLast, h.timeLaserOdometry) &&
         stamped_with_the_odometry(h.timeLaserCloudSurfLast, h.timeLaserOdometry) &&
         stamped_with_the_odometry(h.timeLaserCloudOutlierLast, h.timeLaserOdometry);
}
bool interval_has_passed(const MappingHandler& h) { return h.timeLaserOdometry - h.timeLastProcessing >= mappingProcessInterval; }
}  // namespace

// run() one member function at a time, in run()'s order (LM:1807-1844), so that state can be read between them:
//   0  the gate (above): the four inputs are consumed when all have arrived; -> 1 when the interval lets the scan through
//   1  transformAssociateToMap   2  extractSurroundingKeyFrames   3  downsampleCurrentScan   4  scan2MapOptimization
//   5  saveKeyFramesAndFactor    6  correctPoses   7  publishTF, publishXYZTF, publishKeyPosesAndFrames   8  clearCloud
//   9  transformUpdate alone (scan2MapOptimization calls it last, LM:1650)
// ref_mapnode_same_state holds a handle driven this way against one driven by run().
int ref_mapnode_stage(void* p, int k) {
  if (!p) return -1;
  Node* n = static_cast<Node*>(p);
  Enter e(n);
  MappingHandler& h = n->h;
  switch (k) {
    case 0: {
      if (!all_four_arrived(h)) return 0;
      h.newLaserOdometry = h.newLaserCloudCornerLast = h.newLaserCloudSurfLast = h.newLaserCloudOutlierLast = false;
      if (!interval_has_passed(h)) return 0;
      h.timeLastProcessing = h.timeLaserOdometry;
      return 1;
    }
    case 1: h.transformAssociateToMap(); return 0;
    case 2: h.extractSurroundingKeyFrames(); return 0;
    case 3: h.downsampleCurrentScan(); return 0;
    case 4: h.scan2MapOptimization(); return 0;
    case 5: h.saveKeyFramesAndFactor(); return 0;
    case 6: h.correctPoses(); return 0;
    case 7: h.publishTF(), h.publishXYZTF(), h.publishKeyPosesAndFrames(); return 0;
    case 8: h.clearCloud(); return 0;
    case 9: h.transformUpdate(); return 0;
    default: return -1;
  }
}

// 0 when the two handles hold the same bits in what run() reads and writes: the inputs (the three scan clouds, their
// stamps, the odometry's stamp, the four new* flags, the IMU ring), the six transforms, the robot points, the key poses and
// key-frame clouds, the recent / surrounding deques and list, the filtered scan clouds and the maps, the pointers and
// counters, the estimate and the factor log; -9 otherwise (as scan2map_rounds of ref_map_driver.cpp).  NOT compared: the
// loop thread's members (closestHistoryFrameID, latestFrameIDLoopCloure, potentialLoopFlag and its clouds) — run() neither
// reads nor writes them, and the node leaves the two ids uninitialised until detectLoopClosure() has run.
int ref_mapnode_same_state(void* pa, void* pb) {
  if (!pa || !pb) return -1;
  MappingHandler &a = static_cast<Node*>(pa)->h, &b = static_cast<Node*>(pb)->h;
  if (!same(a.laserCloudCornerLast, b.laserCloudCornerLast) || !same(a.laserCloudSurfLast, b.laserCloudSurfLast) ||
      !same(a.laserCloudOutlierLast, b.laserCloudOutlierLast))
    return -9;
  if (a.timeLaserOdometry != b.timeLaserOdometry || a.timeLaserCloudCornerLast != b.timeLaserCloudCornerLast ||
      a.timeLaserCloudSurfLast != b.timeLaserCloudSurfLast || a.timeLaserCloudOutlierLast != b.timeLaserCloudOutlierLast)
    return -9;
  if (a.newLaserOdometry != b.newLaserOdometry || a.newLaserCloudCornerLast != b.newLaserCloudCornerLast ||
      a.newLaserCloudSurfLast != b.newLaserCloudSurfLast || a.newLaserCloudOutlierLast != b.newLaserCloudOutlierLast)
    return -9;
  if (std::memcmp(a.imuTime, b.imuTime, sizeof a.imuTime) != 0 || std::memcmp(a.imuRoll, b.imuRoll, sizeof a.imuRoll) != 0 ||
      std::memcmp(a.imuPitch, b.imuPitch, sizeof a.imuPitch) != 0)
    return -9;
  for (int w = 0; w < 6; ++w)
    if (std::memcmp(transform_of(a, w), transform_of(b, w), 6 * sizeof(float)) != 0) return -9;
  if (std::memcmp(&a.previousRobotPosPoint, &b.previousRobotPosPoint, sizeof(PointType)) != 0) return -9;
  if (std::memcmp(&a.currentRobotPosPoint, &b.currentRobotPosPoint, sizeof(PointType)) != 0) return -9;
  if (!same(a.cloudKeyPoses3D, b.cloudKeyPoses3D) || a.cloudKeyPoses6D->points.size() != b.cloudKeyPoses6D->points.size()) return -9;
  for (std::size_t i = 0; i < a.cloudKeyPoses6D->points.size(); ++i) {
    const PointTypePose &x = a.cloudKeyPoses6D->points[i], &y = b.cloudKeyPoses6D->points[i];
    const float fx[7] = {x.x, x.y, x.z, x.intensity, x.roll, x.pitch, x.yaw}, fy[7] = {y.x, y.y, y.z, y.intensity, y.roll, y.pitch, y.yaw};
    if (std::memcmp(fx, fy, sizeof fx) != 0 || std::memcmp(&x.time, &y.time, sizeof(double)) != 0) return -9;
  }
  if (!same_seq(a.cornerCloudKeyFrames, b.cornerCloudKeyFrames) || !same_seq(a.surfCloudKeyFrames, b.surfCloudKeyFrames) ||
      !same_seq(a.outlierCloudKeyFrames, b.outlierCloudKeyFrames))
    return -9;
  if (!same_seq(a.recentCornerCloudKeyFrames, b.recentCornerCloudKeyFrames) || !same_seq(a.recentSurfCloudKeyFrames, b.recentSurfCloudKeyFrames) ||
      !same_seq(a.recentOutlierCloudKeyFrames, b.recentOutlierCloudKeyFrames))
    return -9;
  if (a.surroundingExistingKeyPosesID != b.surroundingExistingKeyPosesID || !same_seq(a.surroundingCornerCloudKeyFrames, b.surroundingCornerCloudKeyFrames) ||
      !same_seq(a.surroundingSurfCloudKeyFrames, b.surroundingSurfCloudKeyFrames) ||
      !same_seq(a.surroundingOutlierCloudKeyFrames, b.surroundingOutlierCloudKeyFrames))
    return -9;
  if (!same(a.laserCloudCornerLastDS, b.laserCloudCornerLastDS) || !same(a.laserCloudSurfLastDS, b.laserCloudSurfLastDS) ||
      !same(a.laserCloudOutlierLastDS, b.laserCloudOutlierLastDS) || !same(a.laserCloudSurfTotalLast, b.laserCloudSurfTotalLast) ||
      !same(a.laserCloudSurfTotalLastDS, b.laserCloudSurfTotalLastDS) || !same(a.laserCloudCornerFromMap, b.laserCloudCornerFromMap) ||
      !same(a.laserCloudSurfFromMap, b.laserCloudSurfFromMap) || !same(a.laserCloudCornerFromMapDS, b.laserCloudCornerFromMapDS) ||
      !same(a.laserCloudSurfFromMapDS, b.laserCloudSurfFromMapDS))
    return -9;
  if (a.latestFrameID != b.latestFrameID || a.imuPointerFront != b.imuPointerFront || a.imuPointerLast != b.imuPointerLast ||
      a.aLoopIsClosed != b.aLoopIsClosed || a.isDegenerate != b.isDegenerate || a.timeLastProcessing != b.timeLastProcessing)
    return -9;
  if (a.isamCurrentEstimate.size() != b.isamCurrentEstimate.size() || a.isam->factors.size() != b.isam->factors.size()) return -9;
  for (std::size_t i = 0; i < a.isamCurrentEstimate.size(); ++i)
    if (!same_pose(a.isamCurrentEstimate.at<gtsam::Pose3>(i), b.isamCurrentEstimate.at<gtsam::Pose3>(i))) return -9;
  for (std::size_t i = 0; i < a.isam->factors.size(); ++i) {
    const gtsam::FactorRecord &x = a.isam->factors[i], &y = b.isam->factors[i];
    if (x.prior != y.prior || x.i != y.i || x.j != y.j || !same_pose(x.z, y.z) || x.variances != y.variances) return -9;
  }
  return 0;
}

int ref_mapnode_detect_loop(void* p) {
  if (!p) return -1;
  Node* n = static_cast<Node*>(p);
  Enter e(n);
  return n->h.detectLoopClosure() ? 1 : 0;
}

// performLoopClosure() with the stand-in ICP answering (T row-major 4 x 4 f32, converged, fitness) -> the number of
// factors it handed to iSAM2 (0 or 1)
int ref_mapnode_perform_loop(void* p, const float T[16], int converged, double fitness) {
  if (!p || !T) return -1;
  Node* n = static_cast<Node*>(p);
  Enter e(n);
  lins_ref_shim::IcpAnswer& a = lins_ref_shim::icp_answer();
  for (int i = 0; i < 16; ++i) a.T.m[i] = T[i];
  a.converged = converged != 0, a.fitness = fitness;
  lins_ref_shim::icp_call() = lins_ref_shim::IcpCall();
  const std::size_t before = n->h.isam->factors.size();
  n->h.performLoopClosure();
  return (int)(n->h.isam->factors.size() - before);
}
int ref_mapnode_icp_calls() { return lins_ref_shim::icp_call().calls; }

// isamCurrentEstimate = the n poses (12 doubles each: R row-major, t — gtsam's frame), aLoopIsClosed = true: what a solved
// loop closure leaves for correctPoses()
int ref_mapnode_set_estimate(void* p, const double* poses, int n) {
  if (!p || n < 0 || (n && !poses)) return -1;
  MappingHandler& h = static_cast<Node*>(p)->h;
  h.isamCurrentEstimate.clear();
  for (int i = 0; i < n; ++i) {
    gtsam::Pose3 q;
    q.r.kept = false;
    for (int k = 0; k < 9; ++k) q.r.R[k] = poses[12 * i + k];
    for (int k = 0; k < 3; ++k) q.t.v[k] = poses[12 * i + 9 + k];
    h.isamCurrentEstimate.insert(i, q);
  }
  h.isam->estimate = h.isamCurrentEstimate;
  h.aLoopIsClosed = true;
  return 0;
}

// publishGlobalMap() with one subscriber on its topic -> the number of points published (out: at most cap of them), 0
// when it returned early
int ref_mapnode_global_map(void* p, lins_point* out, int cap) {
  if (!p) return -1;
  Node* n = static_cast<Node*>(p);
  Enter e(n);
  const std::string topic = "/laser_cloud_surround";
  std::map<std::string, sensor_msgs::PointCloud2>& pub = lins_ref_shim::Published<sensor_msgs::PointCloud2>::by_topic();
  pub.erase(topic);
  lins_ref_shim::subscribers()[topic] = 1;
  n->h.publishGlobalMap();
  lins_ref_shim::subscribers().erase(topic);
  const std::map<std::string, sensor_msgs::PointCloud2>::const_iterator it = pub.find(topic);
  return it == pub.end() ? 0 : copy_out(it->second.lins_ref_points, out, cap);
}
// the same call with nobody listening (LM:985) -> 1 when something was published all the same
int ref_mapnode_global_map_unsubscribed(void* p) {
  if (!p) return -1;
  Node* n = static_cast<Node*>(p);
  Enter e(n);
  std::map<std::string, sensor_msgs::PointCloud2>& pub = lins_ref_shim::Published<sensor_msgs::PointCloud2>::by_topic();
  pub.erase("/laser_cloud_surround");
  n->h.publishGlobalMap();
  return pub.count("/laser_cloud_surround") ? 1 : 0;
}

// what: 0 transformLast, 1 Sum, 2 Incre, 3 TobeMapped, 4 BefMapped, 5 AftMapped (6 floats); 6 previousRobotPosPoint,
// 7 currentRobotPosPoint (4 floats)
int ref_mapnode_floats(void* p, int what, float* out) {
  if (!p || !out) return -1;
  MappingHandler& h = static_cast<Node*>(p)->h;
  if (const float* t = transform_of(h, what)) {
    for (int i = 0; i < 6; ++i) out[i] = t[i];
    return 6;
  }
  if (what == 6 || what == 7) {
    const PointType& q = what == 6 ? h.previousRobotPosPoint : h.currentRobotPosPoint;
    out[0] = q.x, out[1] = q.y, out[2] = q.z, out[3] = q.intensity;
    return 4;
  }
  return -1;
}

// cloudKeyPoses3D (x, y, z, intensity), cloudKeyPoses6D (x, y, z, intensity, roll, pitch, yaw) and its time -> count
int ref_mapnode_key_poses(void* p, float* p3, float* p6, double* time, int cap) {
  if (!p) return -1;
  MappingHandler& h = static_cast<Node*>(p)->h;
  const int n = (int)h.cloudKeyPoses3D->points.size();
  if ((int)h.cloudKeyPoses6D->points.size() != n) return -9;
  for (int i = 0; i < n && i < cap; ++i) {
    const PointType& a = h.cloudKeyPoses3D->points[i];
    const PointTypePose& b = h.cloudKeyPoses6D->points[i];
    if (p3) p3[4 * i] = a.x, p3[4 * i + 1] = a.y, p3[4 * i + 2] = a.z, p3[4 * i + 3] = a.intensity;
    if (p6) p6[7 * i] = b.x, p6[7 * i + 1] = b.y, p6[7 * i + 2] = b.z, p6[7 * i + 3] = b.intensity, p6[7 * i + 4] = b.roll, p6[7 * i + 5] = b.pitch, p6[7 * i + 6] = b.yaw;
    if (time) time[i] = b.time;
  }
  return n;
}

// which: 0 / 1 / 2 corner / surf / outlier key frame `id`; 3 / 4 laserCloudCorner / SurfFromMap, 5 / 6 their DS; 7 / 8
// laserCloudCorner / SurfLast, 9 / 10 / 11 corner / surf / outlier LastDS, 12 / 13 laserCloudSurfTotalLast / DS; 14
// latestSurfKeyFrameCloud, 15 / 16 nearHistorySurfKeyFrameCloud / DS; 17 / 18 the source / target handed to ICP; 19 / 20 /
// 21 entry `id` of the recent corner / surf / outlier deque; 22 surroundingKeyPosesDS; 23 entry `id` of the surrounding
// corner deque -> the number of points (out: at most cap of them), -1: no such cloud
int ref_mapnode_cloud(void* p, int which, int id, lins_point* out, int cap) {
  if (!p) return -1;
  const Cloud* c = pick(static_cast<Node*>(p), which, id);
  return c ? copy_out(c->points, out, cap) : -1;
}

// what: 0 surroundingExistingKeyPosesID; 1 the point counts of the recent corner deque's entries, front first; 2 the
// scalars latestFrameID, closestHistoryFrameID, latestFrameIDLoopCloure, potentialLoopFlag, aLoopIsClosed,
// imuPointerFront, imuPointerLast, key frames, recent deque size, isDegenerate -> count
int ref_mapnode_ints(void* p, int what, int* out, int cap) {
  if (!p) return -1;
  MappingHandler& h = static_cast<Node*>(p)->h;
  std::vector<int> v;
  if (what == 0) {
    v = h.surroundingExistingKeyPosesID;
  } else if (what == 1) {
    for (std::size_t i = 0; i < h.recentCornerCloudKeyFrames.size(); ++i) v.push_back((int)h.recentCornerCloudKeyFrames[i]->points.size());
  } else if (what == 2) {
    const int s[10] = {h.latestFrameID, h.closestHistoryFrameID, h.latestFrameIDLoopCloure, h.potentialLoopFlag, h.aLoopIsClosed,
                       h.imuPointerFront, h.imuPointerLast, (int)h.cloudKeyPoses3D->points.size(), (int)h.recentCornerCloudKeyFrames.size(), h.isDegenerate};
    v.assign(s, s + 10);
  } else {
    return -1;
  }
  for (std::size_t i = 0; i < v.size() && (int)i < cap; ++i) out[i] = v[i];
  return (int)v.size();
}

// every factor handed to iSAM2, in order: ij (prior, i, j), z (R row-major, t), the six variances -> count
int ref_mapnode_factors(void* p, int* ij, double* z, double* var, int cap) {
  if (!p) return -1;
  MappingHandler& h = static_cast<Node*>(p)->h;
  const int n = (int)h.isam->factors.size();
  for (int i = 0; i < n && i < cap; ++i) {
    const gtsam::FactorRecord& f = h.isam->factors[i];
    if (ij) ij[3 * i] = f.prior, ij[3 * i + 1] = (int)f.i, ij[3 * i + 2] = (int)f.j;
    if (z) {
      for (int k = 0; k < 9; ++k) z[12 * i + k] = f.z.r.R[k];
      for (int k = 0; k < 3; ++k) z[12 * i + 9 + k] = f.z.t.v[k];
    }
    if (var)
      for (int k = 0; k < 6; ++k) var[6 * i + k] = k < (int)f.variances.size() ? f.variances[k] : 0.0;
  }
  return n;
}

// the operands of the last Pose3::between — the poseFrom / poseTo of the last factor made (LM:1167-1170, 1688-1695): each
// as the three angles RzRyRx was given and the translation, 6 doubles
int ref_mapnode_last_between(double* from, double* to) {
  if (!from || !to) return -1;
  const gtsam::BetweenCall& c = gtsam::last_between();
  if (!c.from.r.kept || !c.to.r.kept) return -9;
  for (int k = 0; k < 3; ++k) from[k] = c.from.r.a[k], from[3 + k] = c.from.t.v[k], to[k] = c.to.r.a[k], to[3 + k] = c.to.t.v[k];
  return 0;
}

// the estimate as correctPoses() reads it: n x 12 doubles -> count
int ref_mapnode_estimate(void* p, double* out, int cap) {
  if (!p) return -1;
  MappingHandler& h = static_cast<Node*>(p)->h;
  const int n = (int)h.isamCurrentEstimate.size();
  for (int i = 0; i < n && i < cap; ++i) {
    const gtsam::Pose3 q = h.isamCurrentEstimate.at<gtsam::Pose3>(i);
    for (int k = 0; k < 9; ++k) out[12 * i + k] = q.r.R[k];
    for (int k = 0; k < 3; ++k) out[12 * i + 9 + k] = q.t.v[k];
  }
  return n;
}

}  // extern "C"
