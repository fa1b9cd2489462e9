// <pcl/registration/icp.h> — STAND-IN (oracle/ref_shim/README.md): performLoopClosure (LM:1127-1141) builds a
// pcl::IterativeClosestPoint, hands it two clouds and reads a 4 x 4, a flag and a fitness back.  The stand-in ALIGNS
// NOTHING: align() records the source and target clouds it was handed (lins_ref_shim::icp_call()) and answers with what
// the driver set beforehand (lins_ref_shim::icp_answer(): the transformation, converged, the fitness score) — so the
// node's glue around the alignment is what a comparison isolates.  STATED, NOT PINNED: PCL ICP's numerics.
#ifndef LINS_REF_SHIM_PCL_ICP_
#define LINS_REF_SHIM_PCL_ICP_
#include <pcl/common/common.h>
namespace lins_ref_shim {
struct IcpAnswer {
  Eigen::Matrix4f T;
  bool converged;
  double fitness;
  IcpAnswer() : converged(false), fitness(0.0) {}
};
struct IcpCall {
  int calls;
  pcl::PointCloud<pcl::PointXYZI> source, target;
  IcpCall() : calls(0) {}
};
inline IcpAnswer& icp_answer() {
  static thread_local IcpAnswer a;
  return a;
}
inline IcpCall& icp_call() {
  static thread_local IcpCall c;
  return c;
}
}  // namespace lins_ref_shim
namespace pcl {
template <class S, class T>
struct IterativeClosestPoint {
  typename PointCloud<S>::Ptr source_;
  typename PointCloud<T>::Ptr target_;
  void setMaxCorrespondenceDistance(double) {}
  void setMaximumIterations(int) {}
  void setTransformationEpsilon(double) {}
  void setEuclideanFitnessEpsilon(double) {}
  void setRANSACIterations(int) {}
  void setInputSource(const typename PointCloud<S>::Ptr& c) { source_ = c; }
  void setInputTarget(const typename PointCloud<T>::Ptr& c) { target_ = c; }
  template <class C>
  void align(C&) {
    lins_ref_shim::IcpCall& call = lins_ref_shim::icp_call();
    ++call.calls;
    if (source_) call.source = *source_;
    if (target_) call.target = *target_;
  }
  bool hasConverged() const { return lins_ref_shim::icp_answer().converged; }
  double getFitnessScore() const { return lins_ref_shim::icp_answer().fitness; }
  Eigen::Matrix4f getFinalTransformation() const { return lins_ref_shim::icp_answer().T; }
};
}  // namespace pcl
#endif
