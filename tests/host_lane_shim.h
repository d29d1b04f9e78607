// What a host compiler needs to read 3dtk_amd/csrc/query_lane.h, the per-lane code of the query kernels, and to run it on
// kd_build.cpp's host tree: __device__ defined away, the device's square root, bit casts and atomic minimum as plain C++,
// a std::vector for the lane stack.  The CPU-tier tests that execute the device walks (test_walks_host.py,
// test_knn_range_host.py, test_collision_host.py) include this file and add their own extern "C" drivers.  Likewise
// ann_lane.h, the walk of the ANN normals, which test_ann_walk_host.py runs on the oracle's ANN tree.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "tdtk_hip.h"
#include "tdtk_internal.h"
#define __device__
#define __forceinline__ inline
static inline double __dsqrt_rn(double x) { return std::sqrt(x); }
static inline long long __double_as_longlong(double x) { long long v; std::memcpy(&v, &x, 8); return v; }
static inline double __longlong_as_double(long long v) { double x; std::memcpy(&x, &v, 8); return x; }
static inline unsigned long long atomicMin(unsigned long long* p, unsigned long long v)
{ const unsigned long long o = *p; if (v < o) *p = v; return o; }
#include "query_lane.h"
#include "ann_lane.h"

namespace tdtk {
// the far-child stack of the ANN walk (ann_lane.h, AnnStack) on the host
struct HostAnnStack {
  std::vector<uint32_t> ref; std::vector<double> bd; int sp = 0;
  void push(uint32_t r, double b) { if ((int)ref.size() <= sp) { ref.resize(sp + 1); bd.resize(sp + 1); } ref[sp] = r; bd[sp] = b; ++sp; }
  void pop(uint32_t& r, double& b) { --sp; r = ref[sp]; b = bd[sp]; }
};
struct HostStack {
  std::vector<uint32_t> v; std::vector<double> w; int sp = 0;
  void push(uint32_t r, double m) { if ((int)v.size() <= sp) { v.resize(sp + 1); w.resize(sp + 1); } v[sp] = r; w[sp] = m; ++sp; }
  void top(uint32_t& r, double& m) const { r = v[sp]; m = w[sp]; }
};
// the walk arguments of a host tree (the real QueryArgs, everything else zero)
static inline QueryArgs host_args(HostTree& T)
{
  QueryArgs a{}; a.nodes = T.nodes.data(); a.pts = T.pts.data(); a.leaf_tab = T.table_mode ? T.leaf_tab.data() : nullptr;
  a.root_ref = T.root_ref; a.cb = T.cb; a.cmask = (1u << T.cb) - 1; a.node_r = T.node_r.data();
  return a;
}
}
using namespace tdtk;
extern "C" void* host_tree_create(const double* xyz, size_t n, int bucket) {
  HostTree* T = new HostTree; std::string err;
  if (!build_tree(xyz, n, bucket, *T, err)) return nullptr;
  return T;
}
extern "C" void host_tree_destroy(void* p) { delete (HostTree*)p; }
