// The per-lane code of the query kernels (query.hip): the tree walks, the LDS list, the covariance of a list, the segment
// arithmetic and the per-item bodies of the collision kernels.  Nothing here needs the device: a host compiler reads this
// file once __device__, __forceinline__, __dsqrt_rn, atomicMin and the two bit casts of double are supplied, and the CPU
// tier runs the walks that way against the reference's fixtures (tests/test_walks_host.py, test_knn_range_host.py,
// test_collision_host.py).  The stack is a template parameter of every walk: push(ref, m2), top(ref, m2) and sp, which is
// LaneStackQ (lane_stack.h) on the device.  What needs the device -- the register list, list_normal, the kernels and the
// launchers -- is in query.hip.
//
// Layout of every kernel: one query per lane, the queries spatially binned first (launch_bin) so that the lanes of a
// wave walk neighbouring parts of the tree, a grid-stride loop over the sorted queries, results written straight to the
// caller's position (order[]).  The walk is a DFS with an explicit per-lane stack (LaneStackQ: LDS levels + an HBM overflow
// column sized from the tree's depth); the node records are the fp64 KdNode ones, so every decision below is the reference's
// own expression on the reference's own values -- no fp32 shortcut, nothing to prove under rounding.
//
// The two walks, rule by rule (each is easy to get subtly wrong):
//
// k-NN (_KNNSearch):
//   * list of k slots (distance, point), distances start at -1 ("unset").  "full" = distances[k-1] != -1.
//   * internal node, on entering it: ONLY when the list is full, the box check
//       a = max(max(|p0-cx|-hx, |p1-cy|-hy), |p2-cz|-hz);  prune when a >= 0 && a*a >= distances[k-1]
//     (a node entered while the list is not full is never pruned, however far away it is).
//   * near child first when p[axis] < splitval -- a STRICT '<' (FindClosest and the range search use splitval - p >= 0,
//     so on a split plane the two rules pick different sides).  The far child is never pruned by its plane: it is pushed
//     unconditionally and meets only its own box check when it is popped (with the list as it is then).
//   * a leaf has no box: it is scanned whenever it is reached, in bucket order, over its real count (padded group slots
//     are never looked at).  Each point goes in before the first slot that is unset or holds a strictly larger distance;
//     the last slot drops out.  Equal distances keep their visiting order, a point equal to the k-th distance of a full
//     list is dropped.  Once the list is full, "kth <= d2" therefore means "no slot is larger": skipped without a scan.
//   * fewer than k points in the tree: the list holds M entries, the rest is reported as -1 / -1.0.
// Fixed radius (_FixedRangeSearch), r2 fixed for the whole walk:
//   * internal node: prune when a >= 0 && a*a >= r2 (a as above).
//   * myd = splitval - p[axis]; myd >= 0: child1 first, child2 after it only if myd*myd < r2; otherwise child2 first and
//     child1 under the same condition.  r2 never changes, so the condition is tested when the far child is pushed.
//   * leaf: every point with Dist2 < r2, in bucket order; the list is in visiting order.
// k nearest within a radius (KDtree::kNearestRangeSearch, kd.cc:137-171; _KNNRangeSearch, kdTreeImpl.h:684-745), in the
// pointer flavour: the list's pointers come from calloc, so closest_neighbors[k-1] == 0 is "the list is not full", which is
// distances[k-1] == -1 (a slot gets its pointer and its distance together).  r2 (sqRad2) is fixed for the whole walk:
//   * the k-NN list: k slots, distances start at -1, a point goes in before the first slot that is unset or strictly larger.
//   * leaf: scanned whenever it is reached, in bucket order.  A point is skipped when Dist2 >= r2, in that sense (a NaN
//     distance is NOT skipped); otherwise it is inserted.
//   * internal node: a is computed on EVERY entry, not only when the list is full.  List not full: prune when a >= 0 &&
//     a*a >= r2.  List full: prune when a >= 0 && a*a >= distances[k-1].
//   * myd = splitval - p[axis]; myd >= 0: child1 first, otherwise child2 -- the range search's rule, not _KNNSearch's strict
//     p < splitval.  The far child only if myd*myd < r2: the radius, never the k-th distance, so the test is made at the
//     push.  When the far child is popped it meets its own box test with the list as it is then.
//   * result: the slots with a distance >= 0, in list order, and their number (0 .. k).
// Adaptive k (calculateNormalsAdaptiveKNN, normals.cc:563-682), per point, kidx = kmin .. kmax:
//   * a FRESH k-NN walk with k = kidx + 1: new list, empty stack, the rules above.  Not one walk at kmax + 1 cut to
//     prefixes: a node's box is fl((min+max)/2) +- fl((max-min)/2) and may exclude one of its own points by an ulp, so a
//     point that walk(k) prunes can enter the first k slots of walk(k'), and the reference's answer is walk(k)'s.
//   * nr = the slots with a distance >= 0 (< kidx + 1 only when the cloud has fewer points); mean and covariance over those
//     nr entries in list order, / nr (list_cov); newmat's EigenValues: e1 <= e2 <= e3.
//   * stop when (e1 > 0.25 * e2) && (fabs(1.0 - e2 / e3) < 0.25), in this sense: e3 == 0 gives NaN or inf and false, a list
//     of one point gives the zero matrix and never stops.  No kidx stops: the list of kmax stands.
//   * the normal is column 0 of the LAST eigenvector matrix computed, oriented and normalised as everywhere (orient_normal).
// Dist2 (globals.icc:238) = (dx*dx + dy*dy) + dz*dz, dx = point - query; fp64 everywhere, FMA contraction off (Makefile).
//
// The cylinder, box and segment queries (kdIndexed.cc:164-213, 233-301; kdTreeImpl.h:432-577, 747-913).  p is the query
// the lanes are binned by, v its second vector (dir, p0 or the box's upper corner); maxdist2 is one value per call.  Len2(x)
// = (x0*x0 + x1*x1) + x2*x2, Dot(x, y) = (x0*y0 + x1*y1) + x2*y2, sqr(x) = x*x (globals.icc:197-213, 1374), r = the node's
// bounding-sphere radius (node_r).  Every comparison is kept in the reference's sense ("skip when >=" is not "take when <"
// once a NaN is involved).  Four of them return lists (count walk, scan, fill walk, as the fixed radius does), one a point.
//
// fixedRangeSearchAlongDir (_fixedRangeSearchAlongDir), dir as given -- never normalised:
//   * internal node: p2c = p - centre; prune when Len2(p2c) - sqr(Dot(p2c, dir)) > sqr(r + sqrt(maxdist2)).
//   * BOTH children, child1 first when p[axis] < splitval (strict); no plane test: the far child is always pushed.
//   * leaf: p2p = p - point; every point with Len2(p2p) - sqr(Dot(p2p, dir)) < maxdist2, in bucket order.
// fixedRangeSearchBetween2Points (_fixedRangeSearchBetween2Points): dist = sqrt(Dist2(p, p0)), dir = p0 - p divided by
//   sqrt(d0*d0 + d1*d1 + d2*d2) (Normalize3 -- the same value as dist); p == p0 gives a NaN dir and an empty list.
//   * the method's own node code runs ONLY on the node the walk starts at: it recurses into _fixedRangeSearchAlongDir.  So
//     the root gets the cylinder test above and then two more, as written in the reference (a squared length plus a
//     length in the first):  prune when dist > Len2(p0 - centre) + r,  prune when dist > sqrt(Len2(p - centre)) + r.
//   * everything below the root, and a root that is a leaf: the cylinder walk.
// AABBSearch (_AABBSearch), box [p, v]; a box with p[i] > v[i] is refused on the host before anything is launched:
//   * internal node: prune when cx+hx < p0 || cy+hy < p1 || cz+hz < p2 || cx-hx > v0 || cy-hy > v1 || cz-hz > v2.
//   * splitval > p[axis]: child1, and child2 after it only if splitval < v[axis]; otherwise child2 ALONE.  This is not the
//     geometric set: a point on the split plane that went to child1 is missed by a box whose lower face lies on the plane,
//     and the answer depends on the bucket size.  It is the reference's answer.
//   * leaf: x >= p0 && x <= v0 && y >= p1 && y <= v1 && z >= p2 && z <= v2, in bucket order.
// The segment queries share their set-up (kdIndexed.cc:252-301): segment_dir = p0 - p, segment_len2 = Len2(dir), segment_n
//   = dir / len2 (NOT a unit vector: p + t * n is the projection for t = Dot(x - p, dir)), maxdist_d = sqrt(maxdist2).
//   The comparison point of x (a bucket point or a node centre): t = Dot(x - p, dir);  t < 0: p;  t > len2: p0;  otherwise
//   p + t * n.  comp_d2(x) = Dist2(comp, x).  With p == p0, n is 0/0: t is 0, the third case applies and comp_d2 is NaN.
// segmentSearch_all (_segmentSearch_all): segment_center = p + dir*0.5, segment_r2 = sqr(0.5*sqrt(len2) + sqrt(maxdist2)).
//   * internal node: the box test of segment_center, prune when a >= 0 && a*a >= segment_r2 (a as in the k-NN walk); then
//     prune when comp_d2(centre) > sqr(r + maxdist_d).
//   * both children, child1 first when p[axis] < splitval (strict), no plane test.
//   * leaf: every point with comp_d2(point) < maxdist2 (a NaN comp_d2 takes nothing: p == p0 gives an empty list).
// segmentSearch_1NearestPoint (_segmentSearch_1NearestPoint): closest_d2 starts at sqr(sqrt(Dist2(p, p0)) + sqrt(maxdist2)).
//   * internal node: the box test of p, prune when a >= 0 && a*a >= closest_d2 (its value at that moment); then the same
//     comp_d2(centre) > sqr(r + maxdist_d).
//   * myd = splitval - p[axis]; myd >= 0: child1 first, otherwise child2; the far child only if sqr(myd) < closest_d2 WHEN
//     THE NEAR CHILD HAS RETURNED: myd*myd goes on the stack and is tested against the then-current closest_d2 at the pop.
//   * leaf: a point is skipped when comp_d2(point) >= maxdist2 (a NaN comp_d2 is NOT skipped: p == p0 still finds the nearest
//     point within the initial closest_d2 = sqr(0 + sqrt(maxdist2))); then newdist2 = Dist2(p, point), taken when < closest_d2 (strict: the
//     first visited point wins a tie).
//   * nothing found: index -1 and d2 -1.0 (the reference returns size_t max).
#pragma once
#include "query_args.h"

namespace tdtk {

// one node's box test (kdTreeImpl.h:606-612 / 662-668): std::max(std::max(ax, ay), az)
__device__ __forceinline__ double box_dist(const KdNode& nd, const double qx, const double qy, const double qz)
{
  const double ax = fabs(qx - nd.cx) - nd.hx;
  const double ay = fabs(qy - nd.cy) - nd.hy;
  const double az = fabs(qz - nd.cz) - nd.hz;
  const double ab = (ax < ay) ? ay : ax;
  return (ab < az) ? az : ab;
}

// The tree a walk reads is a template parameter (TREE): any record with nodes, pts, leaf_tab, root_ref, cb and cmask --
// QueryArgs itself, or one slot of the kd-forest (ForestSlot, forest_lane.h).  shape_walk alone needs QueryArgs (r2, node_r).
template <class TREE>
__device__ __forceinline__ void leaf_span(const TREE& a, const uint32_t ref, uint32_t& start, uint32_t& count)
{
  const uint32_t v = ref & REF_VAL;
  if (a.leaf_tab) { const LeafEntry e = a.leaf_tab[v]; start = (uint32_t)e.start; count = (uint32_t)e.count; }
  else { start = v >> a.cb; count = v & a.cmask; }
}

__device__ __forceinline__ double dist2(const KdPoint& p, const double qx, const double qy, const double qz)
{
  const double dx = p.x - qx, dy = p.y - qy, dz = p.z - qz;
  return (dx * dx + dy * dy) + dz * dz;
}

// ---- the k-NN list, in LDS (the register form: ListReg, query.hip) -------------------------------------------------
// in LDS, [slot][lane] (a wave's accesses to one slot are 64 consecutive 8-byte words: no bank conflict)
template <int BLOCK>
struct ListLds {
  double* ld;
  uint32_t* ls;
  int k, cnt;
  double kth;
  __device__ __forceinline__ void init(int kk)
  {
    k = kk; cnt = 0; kth = -1.0;
    for (int j = 0; j < k; j++) { ld[j * BLOCK] = -1.0; ls[j * BLOCK] = 0xFFFFFFFFu; }
  }
  __device__ __forceinline__ bool full() const { return kth != -1.0; }
  __device__ __forceinline__ void insert(const double md, const uint32_t slot)
  {
    if (kth != -1.0 && kth <= md) return;
    int j = 0;
    for (; j < cnt; j++) if (ld[j * BLOCK] > md) break;     // slots >= cnt are unset
    if (j >= k) return;
    // the reference moves slots j .. k-2 up by one; beyond cnt they are unset and stay so
    for (int l = (cnt < k - 1 ? cnt : k - 1); l > j; --l) { ld[l * BLOCK] = ld[(l - 1) * BLOCK]; ls[l * BLOCK] = ls[(l - 1) * BLOCK]; }
    ld[j * BLOCK] = md;
    ls[j * BLOCK] = slot;
    if (cnt < k) ++cnt;
    if (cnt == k) kth = ld[(k - 1) * BLOCK];
  }
  __device__ __forceinline__ double dist(int j) const { return ld[j * BLOCK]; }
  __device__ __forceinline__ uint32_t slot(int j) const { return ls[j * BLOCK]; }
};

// ---- the walks -------------------------------------------------------------------------------------------------
// The point policy (POINTS, the first template parameter of the list walks) decides which bucket points a walk sees and what
// a list names them by.  The default: every point, by its slot in pts.  (The forest's: forest_lane.h.)
struct AllBySlot {
  static __device__ __forceinline__ bool sees(const KdPoint&) { return true; }
  static __device__ __forceinline__ uint32_t name(const KdPoint&, const uint32_t slot) { return slot; }
};

template <class POINTS = AllBySlot, class TREE, class LIST, class STACK>
__device__ void knn_walk(const TREE& a, const double qx, const double qy, const double qz, LIST& L, STACK& st)
{
  uint32_t cur = a.root_ref;
  for (;;) {
    if (cur & REF_LEAF) {
      uint32_t start, count;
      leaf_span(a, cur, start, count);
      for (uint32_t i = 0; i < count; i++) {
        const KdPoint p = a.pts[start + i];
        if (!POINTS::sees(p)) continue;
        L.insert(dist2(p, qx, qy, qz), POINTS::name(p, start + i));
      }
    } else {
      const KdNode nd = a.nodes[cur & REF_VAL];
      bool pruned = false;
      if (L.full()) {
        const double ap = box_dist(nd, qx, qy, qz);
        pruned = (ap >= 0.0 && ap * ap >= L.kth);
      }
      if (!pruned) {
        const uint32_t axis = ((nd.c1 >> 30) & 1u) | (((nd.c2 >> 30) & 1u) << 1);
        const double qa = (axis == 0) ? qx : ((axis == 1) ? qy : qz);
        const uint32_t r1 = nd.c1 & ~REF_AXIS, r2 = nd.c2 & ~REF_AXIS;
        const bool first = qa < nd.splitval;
        st.push(first ? r2 : r1, 0.0);
        cur = first ? r1 : r2;
        continue;
      }
    }
    if (st.sp == 0) break;
    --st.sp;
    double unused;
    st.top(cur, unused);
  }
}

// EMIT(point, its name, d2) for every point of the radius list, in the reference's visiting order
template <class POINTS = AllBySlot, class TREE, class STACK, class EMIT>
__device__ void range_walk(const TREE& a, const double qx, const double qy, const double qz, const double r2, STACK& st,
                           EMIT& emit)
{
  uint32_t cur = a.root_ref;
  for (;;) {
    if (cur & REF_LEAF) {
      uint32_t start, count;
      leaf_span(a, cur, start, count);
      for (uint32_t i = 0; i < count; i++) {
        const KdPoint p = a.pts[start + i];
        if (!POINTS::sees(p)) continue;
        const double md = dist2(p, qx, qy, qz);
        if (md < r2) emit(p, POINTS::name(p, start + i), md);
      }
    } else {
      const KdNode nd = a.nodes[cur & REF_VAL];
      const double ap = box_dist(nd, qx, qy, qz);
      if (!(ap >= 0.0 && ap * ap >= r2)) {
        const uint32_t axis = ((nd.c1 >> 30) & 1u) | (((nd.c2 >> 30) & 1u) << 1);
        const double qa = (axis == 0) ? qx : ((axis == 1) ? qy : qz);
        const uint32_t r1 = nd.c1 & ~REF_AXIS, r2c = nd.c2 & ~REF_AXIS;
        const double myd = nd.splitval - qa;
        const bool first = myd >= 0.0;
        if (myd * myd < r2) st.push(first ? r2c : r1, 0.0);
        cur = first ? r1 : r2c;
        continue;
      }
    }
    if (st.sp == 0) break;
    --st.sp;
    double unused;
    st.top(cur, unused);
  }
}

// k nearest within r2 (_KNNRangeSearch): knn_walk's list under range_walk's child order and plane test
template <class POINTS = AllBySlot, class TREE, class LIST, class STACK>
__device__ void knn_range_walk(const TREE& a, const double qx, const double qy, const double qz, const double r2, LIST& L,
                               STACK& st)
{
  uint32_t cur = a.root_ref;
  for (;;) {
    if (cur & REF_LEAF) {
      uint32_t start, count;
      leaf_span(a, cur, start, count);
      for (uint32_t i = 0; i < count; i++) {
        const KdPoint p = a.pts[start + i];
        if (!POINTS::sees(p)) continue;
        const double md = dist2(p, qx, qy, qz);
        if (md >= r2) continue;
        L.insert(md, POINTS::name(p, start + i));
      }
    } else {
      const KdNode nd = a.nodes[cur & REF_VAL];
      const double ap = box_dist(nd, qx, qy, qz);
      const double bound = L.full() ? L.kth : r2;
      if (!(ap >= 0.0 && ap * ap >= bound)) {
        const uint32_t axis = ((nd.c1 >> 30) & 1u) | (((nd.c2 >> 30) & 1u) << 1);
        const double qa = (axis == 0) ? qx : ((axis == 1) ? qy : qz);
        const uint32_t r1 = nd.c1 & ~REF_AXIS, r2c = nd.c2 & ~REF_AXIS;
        const double myd = nd.splitval - qa;
        const bool first = myd >= 0.0;
        if (myd * myd < r2) st.push(first ? r2c : r1, 0.0);
        cur = first ? r1 : r2c;
        continue;
      }
    }
    if (st.sp == 0) break;
    --st.sp;
    double unused;
    st.top(cur, unused);
  }
}

// calculateNormal (normals.cc:518-558) over a list the caller enumerates: each(f) calls f(point) for the nr points of the
// list in list order, and is called twice (mean, then covariance -- the arithmetic of k_ann_normals: mean / nr, then
// A = (1/nr X^T) X summed in list order, lower triangle of z); eigen3.h does the rest.  nr is read after the first pass (the
// range normals count their list there).
template <class EACH>
__device__ __forceinline__ void list_cov(EACH&& each, const int& nr, double z[3][3])
{
  double mean[3] = {0.0, 0.0, 0.0};
  each([&](const KdPoint& p) { mean[0] += p.x; mean[1] += p.y; mean[2] += p.z; });
  mean[0] /= nr; mean[1] /= nr; mean[2] /= nr;
  const double sc = 1.0 / nr;
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c <= r; c++) z[r][c] = 0.0;
  each([&](const KdPoint& p) {
    const double x[3] = {p.x - mean[0], p.y - mean[1], p.z - mean[2]};
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c <= r; c++) z[r][c] += (sc * x[c]) * x[r];
  });
}

// ---- cylinder, box and segment queries ------------------------------------------------------------------------
// the segment of the two segment queries with the reference's set-up values, and the three-case comparison point
struct Segment {
  double px, py, pz, ex, ey, ez;   // p, p0
  double dx, dy, dz, len2;         // segment_dir, segment_len2
  double nx, ny, nz;               // segment_n = dir / len2
  __device__ __forceinline__ void init(const double px_, const double py_, const double pz_, const double ex_,
                                       const double ey_, const double ez_)
  {
    px = px_; py = py_; pz = pz_; ex = ex_; ey = ey_; ez = ez_;
    dx = ex - px; dy = ey - py; dz = ez - pz;
    len2 = (dx * dx + dy * dy) + dz * dz;
    nx = dx / len2; ny = dy / len2; nz = dz / len2;
  }
  // Dist2(comp, x), comp the comparison point of x
  __device__ __forceinline__ double comp_d2(const double x, const double y, const double z) const
  {
    const double ax = x - px, ay = y - py, az = z - pz;
    const double t = (ax * dx + ay * dy) + az * dz;
    double cx, cy, cz;
    if (t < 0.0) { cx = px; cy = py; cz = pz; }
    else if (t > len2) { cx = ex; cy = ey; cz = ez; }
    else { cx = px + t * nx; cy = py + t * ny; cz = pz + t * nz; }
    const double gx = x - cx, gy = y - cy, gz = z - cz;
    return (gx * gx + gy * gy) + gz * gz;
  }
};

// Len2(p2x) - sqr(Dot(p2x, dir)), p2x = p - x (kdTreeImpl.h:507-510, 519-522)
__device__ __forceinline__ double line_d2(const double px, const double py, const double pz, const double x, const double y,
                                          const double z, const double ux, const double uy, const double uz, double& len2)
{
  const double wx = px - x, wy = py - y, wz = pz - z;
  len2 = (wx * wx + wy * wy) + wz * wz;
  const double dot = (wx * ux + wy * uy) + wz * uz;
  return len2 - dot * dot;
}

// EMIT(point) for every point of the list of query (p, v), in the reference's visiting order
template <int MODE, class STACK, class EMIT>
__device__ void shape_walk(const QueryArgs& a, const double px, const double py, const double pz, const double vx,
                           const double vy, const double vz, STACK& st, EMIT& emit)
{
  const double md2 = a.r2;
  const double maxd = __dsqrt_rn(md2);
  // the cylinder's axis, and Between2Points' dist
  double ux = vx, uy = vy, uz = vz, dist = 0.0;
  if (MODE == SHAPE_BETWEEN) {
    ux = vx - px; uy = vy - py; uz = vz - pz;
    dist = __dsqrt_rn((ux * ux + uy * uy) + uz * uz);
    ux /= dist; uy /= dist; uz /= dist;
  }
  Segment sg;
  double scx = 0.0, scy = 0.0, scz = 0.0, sr2 = 0.0;   // segment_center, segment_r2
  if (MODE == SHAPE_SEGMENT) {
    sg.init(px, py, pz, vx, vy, vz);
    scx = px + sg.dx * 0.5; scy = py + sg.dy * 0.5; scz = pz + sg.dz * 0.5;
    const double sr = 0.5 * __dsqrt_rn(sg.len2) + maxd;
    sr2 = sr * sr;
  }
  bool root = (MODE == SHAPE_BETWEEN);
  uint32_t cur = a.root_ref;
  for (;;) {
    if (cur & REF_LEAF) {
      uint32_t start, count;
      leaf_span(a, cur, start, count);
      for (uint32_t i = 0; i < count; i++) {
        const KdPoint p = a.pts[start + i];
        bool take;
        if (MODE == SHAPE_ALONG_DIR || MODE == SHAPE_BETWEEN) {
          double unused;
          take = line_d2(px, py, pz, p.x, p.y, p.z, ux, uy, uz, unused) < md2;
        } else if (MODE == SHAPE_AABB) {
          take = p.x >= px && p.x <= vx && p.y >= py && p.y <= vy && p.z >= pz && p.z <= vz;
        } else {
          take = sg.comp_d2(p.x, p.y, p.z) < md2;
        }
        if (take) emit(p);
      }
    } else {
      const KdNode nd = a.nodes[cur & REF_VAL];
      bool pruned;
      if (MODE == SHAPE_ALONG_DIR || MODE == SHAPE_BETWEEN) {
        const double r = a.node_r[cur & REF_VAL];
        double len2;
        const double d2c = line_d2(px, py, pz, nd.cx, nd.cy, nd.cz, ux, uy, uz, len2);
        const double lim = r + maxd;
        pruned = d2c > lim * lim;
        if (MODE == SHAPE_BETWEEN && root && !pruned) {
          // "check if not between points", as written (kdTreeImpl.h:465-472)
          const double wx = vx - nd.cx, wy = vy - nd.cy, wz = vz - nd.cz;
          const double dxp2 = (wx * wx + wy * wy) + wz * wz;
          if (dist > dxp2 + r) pruned = true;
          else if (dist > __dsqrt_rn(len2) + r) pruned = true;
        }
      } else if (MODE == SHAPE_AABB) {
        pruned = nd.cx + nd.hx < px || nd.cy + nd.hy < py || nd.cz + nd.hz < pz ||
                 nd.cx - nd.hx > vx || nd.cy - nd.hy > vy || nd.cz - nd.hz > vz;
      } else {
        const double ap = box_dist(nd, scx, scy, scz);
        pruned = (ap >= 0.0 && ap * ap >= sr2);
        if (!pruned) {
          const double lim = a.node_r[cur & REF_VAL] + maxd;
          pruned = sg.comp_d2(nd.cx, nd.cy, nd.cz) > lim * lim;
        }
      }
      if (!pruned) {
        const uint32_t axis = ((nd.c1 >> 30) & 1u) | (((nd.c2 >> 30) & 1u) << 1);
        const double pa = (axis == 0) ? px : ((axis == 1) ? py : pz);
        const uint32_t r1 = nd.c1 & ~REF_AXIS, r2c = nd.c2 & ~REF_AXIS;
        root = false;
        if (MODE == SHAPE_AABB) {
          const double va = (axis == 0) ? vx : ((axis == 1) ? vy : vz);
          if (nd.splitval > pa) {
            if (nd.splitval < va) st.push(r2c, 0.0);
            cur = r1;
          } else {
            cur = r2c;
          }
        } else {
          const bool first = pa < nd.splitval;
          st.push(first ? r2c : r1, 0.0);
          cur = first ? r1 : r2c;
        }
        continue;
      }
    }
    root = false;
    if (st.sp == 0) break;
    --st.sp;
    double unused;
    st.top(cur, unused);
  }
}

// _FindClosest's loop (kdTreeImpl.h:345-383) from q: best is closest_d2, a point is taken when Dist2 < best (strict: the first
// visited point wins a tie), the far child's myd*myd goes on the stack and is tested against the then-current best at the pop.
// What differs between its users is a RULE: skip(point) -- a bucket point the walk does not look at; prune(node, its index) -- a
// test of an internal node beside the box test; take(point, slot) -- notes the point that has just become the closest.
template <class TREE, class RULE, class STACK>
__device__ void nearest_walk(const TREE& a, const double qx, const double qy, const double qz, RULE& rule, STACK& st, double& best)
{
  uint32_t cur = a.root_ref;
  for (;;) {
    if (cur & REF_LEAF) {
      uint32_t start, count;
      leaf_span(a, cur, start, count);
      for (uint32_t i = 0; i < count; i++) {
        const KdPoint p = a.pts[start + i];
        if (rule.skip(p)) continue;
        const double nd2 = dist2(p, qx, qy, qz);
        if (nd2 < best) { best = nd2; rule.take(p, start + i); }
      }
    } else {
      const KdNode nd = a.nodes[cur & REF_VAL];
      const double ap = box_dist(nd, qx, qy, qz);
      bool pruned = (ap >= 0.0 && ap * ap >= best);
      if (!pruned) pruned = rule.prune(nd, cur & REF_VAL);
      if (!pruned) {
        const uint32_t axis = ((nd.c1 >> 30) & 1u) | (((nd.c2 >> 30) & 1u) << 1);
        const double pa = (axis == 0) ? qx : ((axis == 1) ? qy : qz);
        const uint32_t r1 = nd.c1 & ~REF_AXIS, r2c = nd.c2 & ~REF_AXIS;
        const double myd = nd.splitval - pa;
        const bool first = myd >= 0.0;
        st.push(first ? r2c : r1, myd * myd);
        cur = first ? r1 : r2c;
        continue;
      }
    }
    // the far child of the innermost open node, if its plane still lies inside closest_d2
    bool more = false;
    while (st.sp > 0) {
      --st.sp;
      double m2;
      st.top(cur, m2);
      if (m2 < best) { more = true; break; }
    }
    if (!more) break;
  }
}

// the two segment tests of segmentSearch_1NearestPoint as nearest_walk's rule
struct SegmentRule {
  const QueryArgs& a;
  const Segment& sg;
  const double md2, maxd;   // maxdist2, maxdist_d
  uint32_t& bslot;
  __device__ __forceinline__ bool skip(const KdPoint& p) const { return sg.comp_d2(p.x, p.y, p.z) >= md2; }
  __device__ __forceinline__ bool prune(const KdNode& nd, const uint32_t node) const
  {
    const double lim = a.node_r[node] + maxd;
    return sg.comp_d2(nd.cx, nd.cy, nd.cz) > lim * lim;
  }
  __device__ __forceinline__ void take(const KdPoint&, const uint32_t slot) const { bslot = slot; }
};

// segmentSearch_1NearestPoint: best / bslot are closest_d2 / the bucket slot of closest (0xFFFFFFFF: none)
template <class STACK>
__device__ void segment_nearest_walk(const QueryArgs& a, const Segment& sg, STACK& st, double& best,
                                     uint32_t& bslot)
{
  const double md2 = a.r2;
  SegmentRule rule{a, sg, md2, __dsqrt_rn(md2), bslot};
  nearest_walk(a, sg.px, sg.py, sg.pz, rule, st, best);
}

// ---- collision detection along a trajectory (collision_model.cc) ----------------------------------------------------------
// A point model moves through the tree's cloud along F frames (4x4, column-major).  Marking: every tree point within the
// radius of a moved model point (method 1, handle_pointcloud CTYPE1, collision_model.cc:338-367: fixedRangeSearch) or of the
// segment a model point sweeps between two consecutive frames (method 2, CTYPE2, :368-410: segmentSearch_all) gets a 1 in
// a byte mask.  Depth along the model's axis (calculate_collidingdist2, :714-800): per (frame, model point) the nearest tree
// point c1 of the segment from the moved point to its projection on the model's y axis, and every tree point within the
// radius of c1 takes the minimum of Dist2(moved point, c1).  Both results are sets / minima, so they do not depend on the
// order of the queries: item i is (frame or segment i / P, model point i % P), generated in the lane -- nothing of size
// F x P exists anywhere.  The model is uploaded once in spatial order; consecutive lanes take consecutive model points of
// one frame, and a rigid motion keeps neighbours neighbours, so a wave's lanes walk nearby parts of the tree.  The walks are
// range_walk, shape_walk<SHAPE_SEGMENT> and segment_nearest_walk as they stand, under emitters that mark or minimise.

// transform3 (globals.icc:1454-1463) of (x, y, z) by the frame T: (x*T0 + y*T4 + z*T8) + T12, and so on
__device__ __forceinline__ void transform3(const double* T, const double x, const double y, const double z, double& ox,
                                           double& oy, double& oz)
{
  const double xn = x * T[0] + y * T[4] + z * T[8];
  const double yn = x * T[1] + y * T[5] + z * T[9];
  const double zn = x * T[2] + y * T[6] + z * T[10];
  ox = xn + T[12]; oy = yn + T[13]; oz = zn + T[14];
}

// the marking emitter of both list walks: fill_colliding (collision_model.cc:305-310).  Many lanes may store the same 1 to
// the same byte: plain stores, no atomics.  Stored without a look at the byte first ("collision": the test
// costs a dependent load per listed point and saves nothing that was measured)
struct MarkEmit {
  uint8_t* mask;
  __device__ __forceinline__ void operator()(const KdPoint& p) const { mask[p.orig] = 1; }
  __device__ __forceinline__ void operator()(const KdPoint& p, uint32_t, double) const { mask[p.orig] = 1; }
};

// the minimising emitter of the depth walk: "if (dist2 < dist[k]) dist[k] = dist2" for every k of the sphere around c1.
// Non-negative doubles order as their bit patterns do, so the minimum is a 64-bit unsigned atomicMin; the caller passes
// only d2 < 1000.0 (the entries' initial value), so neither a NaN nor a negative zero's sign bit ever gets in
struct DepthEmit {
  unsigned long long* dmin;
  unsigned long long bits;
  __device__ __forceinline__ void operator()(const KdPoint& p, uint32_t, double) const { atomicMin(&dmin[p.orig], bits); }
};

// marking, method 1: item i is model point i % P under frame i / P
template <class STACK>
__device__ __forceinline__ void collide_sphere_item(const QueryArgs& a, const size_t i, STACK& st)
{
  const size_t f = i / a.P, m = i - f * a.P;
  double px, py, pz;
  transform3(a.frames + 16 * f, a.x[m], a.y[m], a.z[m], px, py, pz);
  MarkEmit emit{a.mask};
  st.sp = 0;
  range_walk(a, px, py, pz, a.r2, st, emit);
}

// marking, method 2: item i is the segment model point i % P sweeps from frame i / P to the next one (the reference carries
// point2 over as the next point1: the same value as transforming afresh).  Two identical frames give p == p0 and nothing
template <class STACK>
__device__ __forceinline__ void collide_segment_item(const QueryArgs& a, const size_t i, STACK& st)
{
  const size_t f = i / a.P, m = i - f * a.P;
  const double x = a.x[m], y = a.y[m], z = a.z[m];
  double px, py, pz, ex, ey, ez;
  transform3(a.frames + 16 * f, x, y, z, px, py, pz);
  transform3(a.frames + 16 * (f + 1), x, y, z, ex, ey, ez);
  MarkEmit emit{a.mask};
  st.sp = 0;
  shape_walk<SHAPE_SEGMENT>(a, px, py, pz, ex, ey, ez, st, emit);
}

// depth along the model's axis: item i is model point i % P under frame i / P; the tree holds the colliding points only.
// dist2 = Dist2(point1, pa[c1]) is the walk's closest_d2: the last newdist2 it took, Dist2(p, point) of that very point
template <class STACK>
__device__ __forceinline__ void collide_depth_axis_item(const QueryArgs& a, const size_t i, STACK& st)
{
  const size_t f = i / a.P, m = i - f * a.P;
  const double* T = a.frames + 16 * f;
  const double y = a.y[m];
  double px, py, pz, ex, ey, ez;
  transform3(T, a.x[m], y, a.z[m], px, py, pz);
  transform3(T, 0.0, y, 0.0, ex, ey, ez);
  Segment sg;
  sg.init(px, py, pz, ex, ey, ez);
  const double b0 = __dsqrt_rn(sg.len2) + __dsqrt_rn(a.r2);
  double best = b0 * b0;
  uint32_t bslot = 0xFFFFFFFFu;
  st.sp = 0;
  segment_nearest_walk(a, sg, st, best, bslot);
  if (bslot == 0xFFFFFFFFu) return;       // found nothing
  if (!(best < 1000.0)) return;           // no entry is above its initial 1000: the reference's comparison is never true
  const KdPoint c1 = a.pts[bslot];
  DepthEmit emit{a.dmin, (unsigned long long)__double_as_longlong(best)};
  st.sp = 0;
  range_walk(a, c1.x, c1.y, c1.z, a.r2, st, emit);
}

// the last step of the depth: the minimum as the float the reference stored, and its root in float
__device__ __forceinline__ float collide_depth_value(const unsigned long long bits)
{
  const float d2 = (float)__longlong_as_double((long long)bits);
  return (float)__dsqrt_rn((double)d2);      // == sqrtf(d2): 53 bits are more than twice 24 plus two
}

}  // namespace tdtk
