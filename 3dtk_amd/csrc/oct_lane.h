// The per-lane code of the octree search kernel (octree.hip): BOctTree<double>::FindClosest (include/slam6d/Boctree.h:1573-1681,
// findClosestInLeaf :1361-1379) for one query, over our node table.  Nothing here needs the device: a host compiler reads this
// file once __device__, __forceinline__, __dsqrt_rn and __popc are supplied (tests/host_oct_shim.h), and the CPU tier runs the
// walk that way against the reference's fixture (tests/test_boctree_search_host.py).
//
// The node table (the layout is ours; octree.hip builds it level by level over the sorted cell keys).  One 16-byte slot per
// node of the reference's tree, the root in slot 0, the children of a node in consecutive slots in ascending child index:
//   internal node: masks = valid | leaf << 8 (bitoct::valid / ::leaf), first = the slot of its first child, so that child ci
//                  is slot first + popcount(valid & ((1 << ci) - 1));
//   leaf:          (start, count) = its run in the point array.  The points are KdPoints in the reference's leaf order
//                  (depth-first over the leaves, inside a leaf the order the in-place partitions left).
//
// The walk, rule by rule (each is the reference's own operation on the reference's own values; easy to get subtly wrong):
//   * voxel coordinates: x = int((p + add) * mult), C++ truncation toward zero, negative outside the root cube;
//     closest_v = int(sqrt(maxdist2) * mult + 1).  The entry point refuses batches where one of these, before its
//     conversion, is not strictly inside +-2^30 (oct_in_range: |v| < 2^30), so every int expression below stays inside int32
//     (the extreme, x + closest_v, is 2^31 - 2).
//   * the box [x - closest_v, x + closest_v] is clamped to [0, largest_index] (max with 0 below, min with largest_index above:
//     an upper bound may stay negative and a lower one may exceed largest_index; only the bits tested matter).
//   * descent while the box's two corners select the same child at child_bit: that child a leaf -> scan it, the search is over;
//     missing -> no point; else descend.  Otherwise branching starts here with size = child_bit / 2.
//   * at a branching node the query's octant is (x - cx >= 0) | (y - cy >= 0) << 1 | (z - cz >= 0) << 2 against the node's
//     integer centre, and the eight children are tried in the order OCT_ORDER gives for that octant.  A child is skipped when
//     closest_v == 0 or max(|ccx - x|, |ccy - y|, |ccz - z|) - size > closest_v, with the child's centre c -/+ size per axis and
//     closest_v as it is at that moment.  A leaf child is scanned; an internal child is entered with size / 2.
//   * leaf scan (findClosestInLeaf): nothing when `count` has reached 10 000, else ++count; the points in leaf order,
//     Dist2 = (dx*dx + dy*dy) + dz*dz, accepted with strict <; an acceptance with d2 <= 0.0001 sets closest_v = 0 -- which
//     prunes every child still to come, everywhere: the search has ended --, any other sets closest_v = int(sqrt(d2) * mult + 1).
// The recursion of _FindClosest is an explicit stack with one 8-byte entry per level (STACK: put(level, a, b), get(level, a,
// b)): { masks | octant << 16 | next preference << 19, first }.  A node's centre is not stored: it is its child's centre
// -/+ the node's size, exact in integers; the size of level l is size0 >> l.
#pragma once
#include "tdtk_internal.h"

namespace tdtk {

struct alignas(16) OctNode {
  uint32_t masks;   // internal: valid | leaf << 8
  uint32_t first;   // internal: slot of the first child
  uint32_t start;   // first point of the node's run in the point array
  uint32_t count;   // points of the run (a leaf scans them)
};
static_assert(sizeof(OctNode) == 16, "OctNode must be 16 bytes");

constexpr int OCT_MAX_LEVELS = 21;        // 3 * 21 key bits (reduce.hip)
constexpr int OCT_MAX_LEAVES = 10000;     // params.max_count, Boctree.h:1583
constexpr int OCT_EARLY_POINTS = 10;      // `earlystop && n <= 10`, Boctree.h:1168
constexpr double OCT_INT_LIMIT = 1073741824.0;   // 2^30

// what a walk reads of a tree
struct OctView {
  const OctNode* nodes;
  const KdPoint* pts;
  double add[3], mult;       // init(), Boctree.h:350-353
  int32_t largest_index;     // child_bit_depth[0] * 2 - 1
  uint32_t top_bit;          // child_bit_depth[0] = 1 << (max_depth - 1)
};

// Order of preference of the eight children for each octant of the query: entry i of row o is (OCT_ORDER[o] >> 3 * i) & 7,
// so an octal literal reads right to left.  The rows are the visits the reference makes at a node with all eight children
// (recorded in tests/golden/k20_boctree_search.npz; tests/test_boctree_search_host.py compares).  Each row starts with the
// octant itself and then takes its three face neighbours; the rest follows no rule short enough to write down.
__device__ __forceinline__ uint32_t oct_order(const uint32_t octant)
{
  switch (octant) {
    case 0: return 076534210u;
    case 1: return 076425301u;
    case 2: return 075416302u;
    case 3: return 064507213u;
    case 4: return 032170654u;
    case 5: return 023061745u;
    case 6: return 013052746u;
    default: return 002143657u;
  }
}

// (p + add) * mult and sqrt(maxdist2) * mult + 1 before their conversion to int: false when the conversion would be undefined
// (strictly inside: after truncation |x| and closest_v are at most 2^30 - 1, so x +- closest_v is at most 2^31 - 2)
__device__ __forceinline__ bool oct_in_range(const double v) { return fabs(v) < OCT_INT_LIMIT; }   // a NaN: false

struct OctLane {
  double qx, qy, qz, d2;
  int32_t x, y, z, cv;
  int32_t best;       // slot in the point array, -1: none
  int32_t leaves;     // `count`: leaves scanned
};

template <class VIEW>
__device__ __forceinline__ void oct_scan_leaf(const VIEW& t, const OctNode& leaf, OctLane& q)
{
  if (q.leaves >= OCT_MAX_LEAVES) return;
  q.leaves++;
  for (uint32_t j = 0; j < leaf.count; j++) {
    const KdPoint p = t.pts[leaf.start + j];
    const double dx = q.qx - p.x, dy = q.qy - p.y, dz = q.qz - p.z;
    const double myd2 = (dx * dx + dy * dy) + dz * dz;            // Dist2, globals.icc:238
    if (myd2 < q.d2) {
      q.d2 = myd2;
      q.best = (int32_t)(leaf.start + j);
      q.cv = (myd2 <= 0.0001) ? 0 : (int32_t)(__dsqrt_rn(myd2) * t.mult + 1);
    }
  }
}

// FindClosest for the query (qx, qy, qz): slot of the closest point in the point array (or -1), its Dist2 (maxdist2 when
// none) and the number of leaves scanned.  The caller has checked oct_in_range for the three coordinates and the radius.
template <class VIEW, class STACK>
__device__ __forceinline__ void oct_find_closest(const VIEW& t, const double qx, const double qy, const double qz, const double maxd2,
                                                 STACK& st, int32_t& slot_out, double& d2_out, int32_t& leaves_out)
{
  OctLane q;
  q.qx = qx; q.qy = qy; q.qz = qz; q.d2 = maxd2; q.best = -1; q.leaves = 0;
  q.x = (int32_t)((qx + t.add[0]) * t.mult);
  q.y = (int32_t)((qy + t.add[1]) * t.mult);
  q.z = (int32_t)((qz + t.add[2]) * t.mult);
  q.cv = (int32_t)(__dsqrt_rn(maxd2) * t.mult + 1);
  const int32_t L = t.largest_index;
  const uint32_t xmin = (uint32_t)((q.x - q.cv > 0) ? q.x - q.cv : 0), xmax = (uint32_t)((q.x + q.cv < L) ? q.x + q.cv : L);
  const uint32_t ymin = (uint32_t)((q.y - q.cv > 0) ? q.y - q.cv : 0), ymax = (uint32_t)((q.y + q.cv < L) ? q.y + q.cv : L);
  const uint32_t zmin = (uint32_t)((q.z - q.cv > 0) ? q.z - q.cv : 0), zmax = (uint32_t)((q.z + q.cv < L) ? q.z + q.cv : L);

  uint32_t bit = t.top_bit;
  int32_t cx = (int32_t)bit, cy = (int32_t)bit, cz = (int32_t)bit;
  OctNode nd = t.nodes[0];
  bool branch = true;
  for (;;) {      // the first node where branching is required
    const uint32_t lo = (uint32_t)((xmin & bit) != 0) | ((uint32_t)((ymin & bit) != 0) << 1) | ((uint32_t)((zmin & bit) != 0) << 2);
    const uint32_t hi = (uint32_t)((xmax & bit) != 0) | ((uint32_t)((ymax & bit) != 0) << 1) | ((uint32_t)((zmax & bit) != 0) << 2);
    if (lo != hi) break;
    const uint32_t valid = nd.masks & 0xFFu, leaf = (nd.masks >> 8) & 0xFFu;
    if (!((valid >> lo) & 1u)) { branch = false; break; }            // no child holds the box
    const OctNode ch = t.nodes[nd.first + (uint32_t)__popc(valid & ((1u << lo) - 1u))];
    if ((leaf >> lo) & 1u) { oct_scan_leaf(t, ch, q); branch = false; break; }
    const int32_t h = (int32_t)(bit / 2);
    cx += (lo & 1u) ? h : -h; cy += (lo & 2u) ? h : -h; cz += (lo & 4u) ? h : -h;
    nd = ch;
    bit /= 2;
  }
  if (branch) {
    const int32_t size0 = (int32_t)(bit / 2);
    int level = 0;
    uint32_t masks = nd.masks, first = nd.first;
    uint32_t octant = (uint32_t)(q.x - cx >= 0) | ((uint32_t)(q.y - cy >= 0) << 1) | ((uint32_t)(q.z - cz >= 0) << 2);
    uint32_t order = oct_order(octant);
    uint32_t i = 0;
    for (;;) {
      if (i == 8 || q.cv == 0) {      // this node is done (closest_v == 0 skips every child there is: unwind)
        if (level == 0) break;
        --level;
        uint32_t a, b;
        st.get(level, a, b);
        masks = a & 0xFFFFu; octant = (a >> 16) & 7u; i = a >> 19; first = b;
        order = oct_order(octant);
        const uint32_t came = (order >> (3 * (i - 1))) & 7u;           // the child this node was left for
        const int32_t size = size0 >> level;
        cx -= (came & 1u) ? size : -size; cy -= (came & 2u) ? size : -size; cz -= (came & 4u) ? size : -size;
        continue;
      }
      const uint32_t ci = (order >> (3 * i)) & 7u;
      ++i;
      const uint32_t valid = masks & 0xFFu;
      if (!((valid >> ci) & 1u)) continue;
      const int32_t size = size0 >> level;
      const int32_t ccx = cx + ((ci & 1u) ? size : -size), ccy = cy + ((ci & 2u) ? size : -size), ccz = cz + ((ci & 4u) ? size : -size);
      const int32_t ax = abs(ccx - q.x), ay = abs(ccy - q.y), az = abs(ccz - q.z);
      const int32_t axy = ax > ay ? ax : ay;
      if ((axy > az ? axy : az) - size > q.cv) continue;
      const OctNode ch = t.nodes[first + (uint32_t)__popc(valid & ((1u << ci) - 1u))];
      if ((masks >> (8 + ci)) & 1u) { oct_scan_leaf(t, ch, q); continue; }
      st.put(level, masks | (octant << 16) | (i << 19), first);
      ++level;
      cx = ccx; cy = ccy; cz = ccz;
      masks = ch.masks; first = ch.first;
      octant = (uint32_t)(q.x - cx >= 0) | ((uint32_t)(q.y - cy >= 0) << 1) | ((uint32_t)(q.z - cz >= 0) << 2);
      order = oct_order(octant);
      i = 0;
    }
  }
  slot_out = q.best; d2_out = q.d2; leaves_out = q.leaves;
}

}  // namespace tdtk
