// What a host compiler needs to read 3dtk_amd/csrc/oct_lane.h, the per-lane code of the octree search kernel: __device__
// defined away, the device's square root and population count as plain C++, an array for the per-level stack.  Stands beside
// host_lane_shim.h (the k-d walks); tests/boctree_model.py compiles it with the extern "C" drivers below.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#define __device__
#define __forceinline__ inline
static inline double __dsqrt_rn(double x) { return std::sqrt(x); }
static inline int __popc(unsigned int x) { return __builtin_popcount(x); }
#include "oct_lane.h"

namespace tdtk {
struct HostOctStack {
  uint32_t a[OCT_MAX_LEVELS], b[OCT_MAX_LEVELS];
  void put(int level, uint32_t x, uint32_t y) { if (level < 0 || level >= OCT_MAX_LEVELS) abort(); a[level] = x; b[level] = y; }
  void get(int level, uint32_t& x, uint32_t& y) const { if (level < 0 || level >= OCT_MAX_LEVELS) abort(); x = a[level]; y = b[level]; }
};
}
using namespace tdtk;

// FindClosest for K queries over a node table and a leaf-ordered point array; -1 when the entry point would refuse the batch
// (oct_in_range, the one statement of the rule: a value not strictly inside +-2^30)
extern "C" int oct_host_find(const void* nodes, const void* pts, const double* add, double mult, int largest_index, unsigned top_bit,
                             const double* q, int K, double maxd2, int* slot, double* d2, int* leaves)
{
  OctView t{};
  t.nodes = static_cast<const OctNode*>(nodes); t.pts = static_cast<const KdPoint*>(pts);
  for (int a = 0; a < 3; a++) t.add[a] = add[a];
  t.mult = mult; t.largest_index = largest_index; t.top_bit = top_bit;
  if (!oct_in_range(__dsqrt_rn(maxd2) * mult + 1)) return -1;
  for (int i = 0; i < K; i++)
    for (int a = 0; a < 3; a++)
      if (!oct_in_range((q[3 * i + a] + add[a]) * mult)) return -1;
  HostOctStack st;
  for (int i = 0; i < K; i++) oct_find_closest(t, q[3 * i], q[3 * i + 1], q[3 * i + 2], maxd2, st, slot[i], d2[i], leaves[i]);
  return 0;
}

extern "C" void oct_host_order(int octant, int* out8)
{
  const uint32_t w = oct_order((uint32_t)octant);
  for (int i = 0; i < 8; i++) out8[i] = (int)((w >> (3 * i)) & 7u);
}
