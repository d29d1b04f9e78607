// The per-lane code of the dynamic kd-forest (forest.hip): BkdTree of bkd.h / bkd.cc, the logarithmic method over the
// library's static kd-trees.  A forest is a buffer of fewer than b points and slots 0 .. S-1, each empty or one kd-tree built
// by the device build over the points handed to it; its points carry their forest id (the running insertion counter) in
// KdPoint::orig.  Nothing here needs the device: a host compiler reads this file under tests/host_lane_shim.h, and the CPU
// tier runs this code against the reference's fixture (tests/test_bkd_host.py).  The stack is a template parameter as in
// query_lane.h.  What needs the device -- the kernels, the claims of the remove pass, the gathers of a merge -- is in
// forest.hip.
//
// No tree is descended here: the loops are query_lane.h's knn_walk, range_walk and nearest_walk, which read a ForestSlot as
// they read QueryArgs.  What the forest changes in them is stated once: the point policy LiveById (a walk sees the points
// with orig >= 0 and a list names them by orig, where a tree query sees every point and names it by its slot) and, for
// nearest_walk, the rule LiveClosestRule (the same filter, no node test beside the box test, position and id of the point
// taken).  This file adds the order over the containers -- slots ascending, the buffer -- and the quirks between them.
//
// Layout of every query kernel: ONE launch per call covers all slots and the buffer.  One query per lane, binned first
// (launch_bin), a grid-stride loop; a lane loops over the by-value table of slot descriptors (ForestSlot, at most
// FOREST_MAX_SLOTS) with one stack sized for the deepest tree, then scans the buffer.  The node records are the fp64 KdNode
// ones and every decision is the reference's expression on the reference's values.
//
// Removed points.  A removed point stays where it is and its KdPoint::orig becomes -1: the liveness word is the id itself.
// Every walk loads the whole 32-byte KdPoint anyway, so the test costs no load; a removal is one 4-byte store and
// rewrites no node, no packed child reference and no leaf table, so it is the same in packed and in table mode and a leaf
// that is emptied completely simply contributes nothing.  (The reference swaps the point to the end of its leaf and
// decrements the leaf's count; the sets a walk sees are the same.)  The forest's trees are private to it and never handed
// out as tdtk_tree: under the default policy a walk would see their removed points.
//
// The queries, rule by rule:
//
// FindClosest (BkdTree::FindClosest, bkd.cc:227-259, over KDTreeImpl::_FindClosest, kdTreeImpl.h:345-383: nearest_walk):
//   * per tree: closest_d2 starts at maxdist2; leaf: a point is taken when Dist2 < closest_d2 (strict: the first visited
//     point wins a tie), in bucket order.
//   * internal node: a = max(max(|p0-cx|-hx, |p1-cy|-hy), |p2-cz|-hz); return when a >= 0 && a*a >= closest_d2.
//   * myd = splitval - p[axis]; myd >= 0: child1 first, otherwise child2; the far child only if myd*myd < closest_d2 WHEN
//     THE NEAR CHILD HAS RETURNED: myd*myd goes on the stack and is tested at the pop.
//   * slots in ascending order; a later slot replaces the result only with a strictly smaller Dist2.  Here every tree
//     starts from the best so far instead of maxdist2: a tree then reports a point exactly when the reference would have
//     replaced the result with it.
//   * Q1: the buffer is then scanned in order with strict '<' against the best so far -- which is DBL_MAX, not maxdist2,
//     when no tree point was found.  With no tree point within maxdist2 the nearest buffer point is returned however far
//     away it is.  Nothing found at all: id -1, d2 -1.0.
// kNearestNeighbors (bkd.cc:314-346, over _KNNSearch, the rules of knn_walk in query_lane.h):
//   * the reference takes up to k candidates per slot, in slot order, then every buffer point, stable-sorts them by
//     (dx*dx + dy*dy) + dz*dz and returns the first min(k, candidates).  Here ONE list of k slots goes through all the
//     trees and the buffer in that order: an entry goes in before the first slot that is unset or strictly larger, so
//     equal distances keep their visiting order (slots ascending, the walk's order, then the buffer) and the list is that
//     stable sort cut to k.  A full list prunes a later tree's nodes with the k-th distance so far; a per-tree list could
//     only have kept points the merge drops.
//   * fewer than k live points: the rest of the row is -1 / -1.0.
// fixedRangeSearch (bkd.cc:356-372, over _FixedRangeSearch, the rules of range_walk):
//   * per slot in ascending order the tree's list, Dist2 < r2 (strict), in visiting order.
//   * Q2: then the buffer points in order with Dist2 <= r2 -- a buffer point at exactly r2 is taken, a tree point is not.
// remove (bkd.cc:203-225): the device rule, independent of any tree's shape.  In the lowest container that holds a live
//   point x with Dist2(p, x) < 1e-9 (the buffer before slot 0), the nearest such x goes; the first visited wins a tie.  The
//   find is FindClosest's walk with closest_d2 starting at 1e-9 in every container.  A bit-equal p always reaches its point:
//   its Dist2 is 0, and a box that misses the point by an ulp gives a*a far below 1e-9.  Requests of one call behave as if
//   applied in order (forest.hip, "the remove pass").
// Dist2 = (dx*dx + dy*dy) + dz*dz, dx = point - query; fp64, FMA contraction off.
#pragma once
#include "query_lane.h"

namespace tdtk {

constexpr int FOREST_MAX_SLOTS = 32;
constexpr double FOREST_REMOVE_D2 = 0.000000001;   // bkd.cc:208, kdTreeImpl.h:307
constexpr int32_t FOREST_DEAD = -1;                // KdPoint::orig of a removed point
constexpr int32_t FOREST_UNCLAIMED = 0x7FFFFFFF;   // KdPoint::pad: no request of the running remove pass wants the point

// one slot's tree: what leaf_span and the walks read of QueryArgs.  n == 0: the slot is empty
struct ForestSlot {
  const KdNode* nodes;
  KdPoint* pts;
  const LeafEntry* leaf_tab;   // table mode only
  uint32_t root_ref, cb, cmask;
  uint32_t n;                  // point slots of pts (live and removed)
};

struct ForestArgs {
  QueryArgs q;                 // the queries (x / y / z, order, n), k, r2 (maxdist2, sqRad2), the stack overflow area, the outputs
  KdPoint* buf;                // the buffer, in insertion order
  uint32_t nbuf;
  int nslots;
  // the remove pass: per request in caller order
  int32_t* res;                // -2: pending; -1: matches nothing; >= 0: the id removed
  int32_t* cand_c;             // the container of the request's candidate (0: the buffer, s + 1: slot s)
  uint32_t* cand_p;            // ... and its position there
  uint32_t* ctl;               // [0] the smallest request that lost its claim, [1] requests still pending, [2 + c] points removed from container c
  ForestSlot slot[FOREST_MAX_SLOTS];
};

// the forest's point policy (query_lane.h, "the point policy"): the live points, named by their forest id
struct LiveById {
  static __device__ __forceinline__ bool sees(const KdPoint& p) { return p.orig >= 0; }
  static __device__ __forceinline__ uint32_t name(const KdPoint& p, uint32_t) { return (uint32_t)p.orig; }
};

// _FindClosest over the live points as nearest_walk's rule: no test beside the box test; pos / id are the position and the
// id of closest (unchanged: none)
struct LiveClosestRule {
  uint32_t& pos;
  int32_t& id;
  __device__ __forceinline__ bool skip(const KdPoint& p) const { return p.orig < 0; }
  __device__ __forceinline__ bool prune(const KdNode&, uint32_t) const { return false; }
  __device__ __forceinline__ void take(const KdPoint& p, const uint32_t slot) const { pos = slot; id = p.orig; }
};

// _FindClosest over the live points of one tree: best / pos are closest_d2 / the position of closest (unchanged: none)
template <class STACK>
__device__ void forest_closest_walk(const ForestSlot& t, const double qx, const double qy, const double qz, STACK& st,
                                    double& best, uint32_t& pos, int32_t& id)
{
  LiveClosestRule rule{pos, id};
  st.sp = 0;
  nearest_walk(t, qx, qy, qz, rule, st, best);
}

// ---- one query against the whole forest ---------------------------------------------------------------------------------
// BkdTree::FindClosest with quirk Q1
template <class STACK>
__device__ __forceinline__ void forest_find_closest(const ForestArgs& f, const double qx, const double qy, const double qz,
                                                    const double maxdist2, STACK& st, int32_t& id, double& d2)
{
  double best = maxdist2;
  uint32_t pos = 0;
  id = -1;
  for (int s = 0; s < f.nslots; s++) {
    if (f.slot[s].n == 0) continue;
    forest_closest_walk(f.slot[s], qx, qy, qz, st, best, pos, id);
  }
  if (id < 0) best = 1.7976931348623157e308;   // minDist2 = __DBL_MAX__: no tree point was found
  for (uint32_t i = 0; i < f.nbuf; i++) {
    const KdPoint p = f.buf[i];
    if (p.orig < 0) continue;
    const double md = dist2(p, qx, qy, qz);
    if (md < best) { best = md; id = p.orig; }
  }
  d2 = (id < 0) ? -1.0 : best;
}

// BkdTree::kNearestNeighbors: the list afterwards holds the row (ids in the slots)
template <class LIST, class STACK>
__device__ __forceinline__ void forest_knn(const ForestArgs& f, const double qx, const double qy, const double qz, LIST& L,
                                           STACK& st)
{
  for (int s = 0; s < f.nslots; s++) {
    if (f.slot[s].n == 0) continue;
    st.sp = 0;
    knn_walk<LiveById>(f.slot[s], qx, qy, qz, L, st);
  }
  for (uint32_t i = 0; i < f.nbuf; i++) {
    const KdPoint p = f.buf[i];
    if (p.orig < 0) continue;
    L.insert(dist2(p, qx, qy, qz), (uint32_t)p.orig);
  }
}

// BkdTree::fixedRangeSearch with quirk Q2: EMIT(id, d2) in list order
template <class STACK, class EMIT>
__device__ __forceinline__ void forest_fixed_range(const ForestArgs& f, const double qx, const double qy, const double qz,
                                                   const double r2, STACK& st, EMIT& emit)
{
  auto listed = [&](const KdPoint&, const uint32_t id, const double md) { emit((int32_t)id, md); };
  for (int s = 0; s < f.nslots; s++) {
    if (f.slot[s].n == 0) continue;
    st.sp = 0;
    range_walk<LiveById>(f.slot[s], qx, qy, qz, r2, st, listed);
  }
  for (uint32_t i = 0; i < f.nbuf; i++) {
    const KdPoint p = f.buf[i];
    if (p.orig < 0) continue;
    const double md = dist2(p, qx, qy, qz);
    if (md <= r2) emit(p.orig, md);
  }
}

// the candidate of a remove request: the nearest live point within 1e-9 in the lowest container that has one
// (container 0: the buffer, s + 1: slot s).  false: the request matches nothing
template <class STACK>
__device__ __forceinline__ bool forest_remove_find(const ForestArgs& f, const double px, const double py, const double pz,
                                                   STACK& st, int32_t& cont, uint32_t& pos)
{
  double best = FOREST_REMOVE_D2;
  int32_t id = -1;
  for (uint32_t i = 0; i < f.nbuf; i++) {
    const KdPoint p = f.buf[i];
    if (p.orig < 0) continue;
    const double md = dist2(p, px, py, pz);
    if (md < best) { best = md; id = p.orig; pos = i; }
  }
  if (id >= 0) { cont = 0; return true; }
  for (int s = 0; s < f.nslots; s++) {
    if (f.slot[s].n == 0) continue;
    forest_closest_walk(f.slot[s], px, py, pz, st, best, pos, id);
    if (id >= 0) { cont = s + 1; return true; }
  }
  return false;
}

// the point of container c at position p
__device__ __forceinline__ KdPoint* forest_point(const ForestArgs& f, const int32_t c, const uint32_t p)
{
  return (c == 0 ? f.buf : f.slot[c - 1].pts) + p;
}

}  // namespace tdtk
