// pose_graph_host.h — what the CPU restatements of the pose graph share (host/pose_graph.cpp, host/team_graph.cpp): the
// handle, and a phase on the CPU.
#pragma once
#include "../pose_graph.h"

struct lins_host_pose_graph {
  lins_pg::Graph g;
};

namespace lins_pg {

struct HostExec {  // a phase on the CPU: the lanes one after the other
  template <class F>
  void operator()(F f) const {
    for (int t = 0; t < kThreads; ++t) f(t);
  }
};

}  // namespace lins_pg
