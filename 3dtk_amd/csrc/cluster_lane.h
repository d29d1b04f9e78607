// The per-lane code of radius clustering (tdtk_cluster_radius; kernels in query.hip): the connected components of the graph
// whose nodes are the tree's points and whose edges are the pairs (i, j) with j in KDtreeIndexed::fixedRangeSearch(p_i, r2),
// that is Dist2(p_i, p_j) < r2 -- the relation src/collision/segment_colliding.cc:55-102 groups its points by.  Like
// query_lane.h a host compiler reads this file, once the relaxed agent-scope load and store (__hip_atomic_load,
// __hip_atomic_store, __HIP_MEMORY_SCOPE_AGENT) and atomicCAS / atomicMin / atomicAdd on uint32_t are supplied beside
// host_lane_shim.h's; tests/test_clusters_host.py runs it that way, also under loads that return stale values.
//
// Everything works in SLOT space: slot s is position s of the leaf-ordered point array.  The queries are the tree's own
// points, which already lie in leaf order, so the lanes of a wave walk neighbouring parts of the tree without a binning
// pass.  Where the buckets are padded to groups of four (kernels.hip, "bucket groups") a pad slot repeats the bucket's last
// point; it is recognised by that (slot_is_pad), takes no lane and is never listed by a walk (leaf_span gives real counts).
//
// Four steps, each a launch of its own:
//   init     parent[s] = s, ckey[s] = none, csize[s] = 0
//   link     one lane per real slot s: range_walk around its own point under an emitter that unites s with every listed
//            slot j < s (the relation is symmetric bit for bit, (-d) * (-d) == d * d: the pair is met from its larger slot)
//            that passes the subset and the normal test
//   flatten  every node finds its root, stores it as its link, and adds its input index (atomicMin) and a 1 (atomicAdd)
//            to the root's key and size
//   number   flag the keys of the kept components in input-index space; behind an exclusive scan of the flags
//            (launch_scan_u32) every node reads its label at its root's key, and every root writes first and sizes
//
// The union-find is lock-free.  parent[x] changes in two ways only:
//   hook      atomicCAS(&parent[hi], hi, lo) with lo < hi, by a lane that has found hi and lo as roots of two slots it has to
//             unite.  It succeeds only while hi is still its own parent, so a slot is hooked once.
//   compress  a store of a value READ from parent[] further up the same path (path halving), made only when that value is
//             smaller than the link it replaces was when it was read.
// So every value ever stored in parent[x] is <= x and names a slot of x's component, x itself only before the hook.  A
// read that returns an OLDER value of a cell -- the L2s of the XCDs are not coherent with each other inside a launch, and
// the loads below are L2-served -- therefore yields a valid, older ancestor: it makes a find longer or a CAS fail, and
// corrupts nothing.  A compression may replace a link by an older ancestor; the slot stays hooked (the value is below x), its
// chain still descends strictly and ends at the one slot of the component that was never hooked: in a component C with
// root r (the only never-hooked slot, so the end of every chain in C) no find can return m != r as a root and have the hook
// of r under m succeed, because m's own chain descends to r < m.  The CAS acts on the cell's current value wherever the
// loads came from, and a failed one returns it: a smaller index, from which the lane goes on.  No lane waits for a value
// another lane has to write, and every loop ends because its index strictly decreases.  No fence and no acquire: what a
// launch has linked is visible to the next launch (flatten), not necessarily to its own lanes, and need not be.
#pragma once
#include "query_lane.h"

namespace tdtk {

constexpr uint32_t CL_NO_KEY = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t uf_load(const uint32_t* parent, const uint32_t x)
{
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x as this lane sees it, halving the path on the way
__device__ __forceinline__ uint32_t uf_find(uint32_t* parent, uint32_t x)
{
  for (;;) {
    const uint32_t p = uf_load(parent, x);
    if (p == x) return x;
    const uint32_t g = uf_load(parent, p);
    if (g == p) return p;
    __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // g < p < x
    x = g;
  }
}

__device__ __forceinline__ void uf_unite(uint32_t* parent, uint32_t a, uint32_t b)
{
  if (uf_load(parent, a) == uf_load(parent, b)) return;     // dense clouds leave here almost every time
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const uint32_t old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return;
    a = old;      // hi has been hooked meanwhile: old < hi
    b = lo;
  }
}

// a pad slot of a padded bucket repeats the slot before it; real points have distinct input indices
__device__ __forceinline__ bool slot_is_pad(const QueryArgs& a, const uint32_t s)
{
  return (s & 3u) != 0 && a.pts[s].orig == a.pts[s - 1].orig;
}

__device__ __forceinline__ bool cluster_is_node(const QueryArgs& a, const int32_t orig)
{
  return !a.subset || a.subset[orig] != 0;
}

__device__ __forceinline__ void cluster_init_item(const QueryArgs& a, const uint32_t s)
{
  a.parent[s] = s;
  a.ckey[s] = CL_NO_KEY;
  a.csize[s] = 0u;
}

// the emitter of the link walk
struct LinkEmit {
  const QueryArgs& a;
  uint32_t s;
  double nx, ny, nz;
  __device__ __forceinline__ void operator()(const KdPoint& p, const uint32_t j, double) const
  {
    if (j >= s) return;
    if (!cluster_is_node(a, p.orig)) return;
    if (a.cnormals) {
      const double* m = a.cnormals + 3 * (size_t)p.orig;
      const double c = fabs((nx * m[0] + ny * m[1]) + nz * m[2]);
      if (!(c >= a.min_cos)) return;       // in this sense: a NaN gives no edge
    }
    uf_unite(a.parent, s, j);
  }
};

template <class STACK>
__device__ __forceinline__ void cluster_link_item(const QueryArgs& a, const uint32_t s, STACK& st)
{
  if (slot_is_pad(a, s)) return;
  const KdPoint q = a.pts[s];
  if (!cluster_is_node(a, q.orig)) return;
  LinkEmit emit{a, s, 0.0, 0.0, 0.0};
  if (a.cnormals) {
    const double* m = a.cnormals + 3 * (size_t)q.orig;
    emit.nx = m[0]; emit.ny = m[1]; emit.nz = m[2];
  }
  st.sp = 0;
  range_walk(a, q.x, q.y, q.z, a.r2, st, emit);
}

// behind the link launch: the links are final, only compressions (of other lanes of this launch) still change them
__device__ __forceinline__ void cluster_flatten_item(const QueryArgs& a, const uint32_t s)
{
  if (slot_is_pad(a, s)) return;
  const int32_t orig = a.pts[s].orig;
  if (!cluster_is_node(a, orig)) return;
  uint32_t r = s;
  for (;;) {
    const uint32_t p = uf_load(a.parent, r);
    if (p == r) break;
    r = p;
  }
  if (r != s) __hip_atomic_store(a.parent + s, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  atomicMin(a.ckey + r, (uint32_t)orig);
  atomicAdd(a.csize + r, 1u);
}

__device__ __forceinline__ bool cluster_kept(const QueryArgs& a, const uint32_t size)
{
  return size >= (a.min_size > 1u ? a.min_size : 1u);
}

// only a root with members has a size: no test of pad or subset needed
__device__ __forceinline__ void cluster_flag_item(const QueryArgs& a, const uint32_t s)
{
  if (cluster_kept(a, a.csize[s])) a.cflag[a.ckey[s]] = 1u;
}

__device__ __forceinline__ void cluster_label_item(const QueryArgs& a, const uint32_t s)
{
  if (slot_is_pad(a, s)) return;
  const int32_t orig = a.pts[s].orig;
  int32_t label = -1;
  if (cluster_is_node(a, orig)) {
    const uint32_t r = a.parent[s];
    const uint32_t size = a.csize[r];
    if (cluster_kept(a, size)) {
      const uint32_t key = a.ckey[r];
      label = (int32_t)a.cnum[key];
      if (r == s) { a.cfirst[label] = (int32_t)key; a.csizes_out[label] = size; }
    }
  }
  a.labels[orig] = label;
}

}  // namespace tdtk
