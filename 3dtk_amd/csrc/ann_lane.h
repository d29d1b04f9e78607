// The per-lane code of the ANN normals (ann.hip): the tree record, the root-cell distance, the k best as a sorted list, the
// far-child stack and ANN's priority search (annkSearch, kd_search.cpp:89-210) as ONE walk, which k_ann_normals calls once
// per query and k_ann_adaptive once per query and k.  Nothing here needs the device: a host compiler reads this file under
// tests/host_lane_shim.h, and tests/test_ann_walk_host.py runs the walk on the library's tree against annkSearch itself --
// lists and visit tallies, entry for entry.
//
// The list is a pair of plain arrays the kernel owns, handed to the functions here by reference, and that form is load-bearing:
// the compiler keeps such arrays as <KMAX x double> / <KMAX x i32> vector values across the walk.  As members of a struct
// (with member functions, or a view of two references) they are split into scalars instead, which costs k_ann_normals<10>
// 11 to 20 more VGPRs and k_ann_normals<16> 38 to 44 spilled SGPRs, where tests/test_host_logic.py allows 16.
#pragma once
#include <cfloat>
#include <cstddef>
#include <cstdint>

#include "tdtk_internal.h"

namespace tdtk {

#define A_LEAF 0x20000000u    // child reference: leaf flag | position (29 bits); c0 bits 30..31 = cutting dimension
#define A_VAL 0x1FFFFFFFu
#define ANN_LDS_STACK 12      // far-child entries per thread kept in LDS; deeper ones spill to global memory
#define ANN_BLOCK 256         // threads of a search workgroup: the row length of the LDS stack

struct AnnNode {          // 32 B: one splitting node (ANNkd_split: cut_val, cd_bnds[2], child[2], cut_dim)
  double cut_val, lo, hi;
  uint32_t c0, c1;        // child references: bit 29 = leaf, bits 0..28 = node index / point position; c0 bits 30..31 = cut_dim
};

// annBoxDistance (kd_util.cpp:127-150): the squared distance of the query from the root cell
__device__ __forceinline__ double ann_box_distance(const double qx, const double qy, const double qz, const double* blo,
                                                   const double* bhi)
{
  const double q[3] = {qx, qy, qz};
  double bd = 0.0;
#pragma unroll
  for (int d = 0; d < 3; d++) {
    if (q[d] < blo[d]) { const double t = blo[d] - q[d]; bd = bd + t * t; }
    else if (q[d] > bhi[d]) { const double t = q[d] - bhi[d]; bd = bd + t * t; }
  }
  return bd;
}

// The k best (ANNmin_k) in KMAX >= k slots, every index static.  The list is the LAST k slots; the k0 = KMAX - k slots in
// front hold the sentinel key -1, which no insertion moves, so the k-th key is always slot KMAX - 1.
template <int KMAX>
__device__ __forceinline__ void ann_list_init(double (&key)[KMAX], uint32_t (&info)[KMAX], const int k0)
{
#pragma unroll
  for (int j = 0; j < KMAX; j++) { key[j] = (j < k0) ? -1.0 : DBL_MAX; info[j] = 0xFFFFFFFFu; }
}
// ANNmin_k::insert (pr_queue_k.h:100-114): behind every key <= dist, the last one drops out
template <int KMAX>
__device__ __forceinline__ void ann_list_insert(double (&key)[KMAX], uint32_t (&info)[KMAX], const double dist,
                                                const uint32_t pos)
{
  double ck = dist;
  uint32_t ci = pos;
  bool shifting = false;
#pragma unroll
  for (int j = 0; j < KMAX; j++) {
    shifting = shifting || (key[j] > ck);
    if (shifting) {
      const double tk = key[j]; key[j] = ck; ck = tk;
      const uint32_t ti = info[j]; info[j] = ci; ci = ti;
    }
  }
}

// The far children a walk has yet to visit, with their box distances.  The device's form: ANN_LDS_STACK levels of
// [level][thread] LDS, deeper ones in the launch's spill columns ([level - ANN_LDS_STACK][thread of the grid]; a tree of
// depth d needs d + 1 - ANN_LDS_STACK of them, ann_spill_entries).  The host's form is a vector (host_lane_shim.h).
struct AnnStack {
  uint32_t (*s_ref)[ANN_BLOCK];
  double (*s_bd)[ANN_BLOCK];
  uint32_t* spill_ref;
  double* spill_bd;
  uint32_t T, tid, tx;     // threads of the grid, this one among them, and within its workgroup
  int sp;
  __device__ __forceinline__ void push(const uint32_t ref, const double bd)
  {
    if (sp < ANN_LDS_STACK) { s_ref[sp][tx] = ref; s_bd[sp][tx] = bd; }
    else { spill_ref[(size_t)(sp - ANN_LDS_STACK) * T + tid] = ref; spill_bd[(size_t)(sp - ANN_LDS_STACK) * T + tid] = bd; }
    sp++;
  }
  __device__ __forceinline__ void pop(uint32_t& ref, double& bd)
  {
    sp--;
    if (sp < ANN_LDS_STACK) { ref = s_ref[sp][tx]; bd = s_bd[sp][tx]; }
    else { ref = spill_ref[(size_t)(sp - ANN_LDS_STACK) * T + tid]; bd = spill_bd[(size_t)(sp - ANN_LDS_STACK) * T + tid]; }
  }
};

// annkSearch for one query: the list (initialised by the caller) filled from the tree in the library's order.  bd is the
// query's distance from the root cell, max_err = (1 + eps)^2.  COUNT: the splitting nodes and leaf points visited are added
// to c_split / c_leaf.
template <int KMAX, bool COUNT, class STACK>
__device__ __forceinline__ void ann_search(const AnnNode* __restrict__ nodes, const KdPoint* __restrict__ pts,
                                           const uint32_t root_ref, const double qx, const double qy, const double qz,
                                           double bd, const double max_err, double (&key)[KMAX], uint32_t (&info)[KMAX],
                                           STACK& st, unsigned& c_split, unsigned& c_leaf)
{
  uint32_t cur = root_ref;
  st.sp = 0;
  for (;;) {
    while (!(cur & A_LEAF)) {                      // ANNkd_split::ann_search (kd_search.cpp:128-170)
      if (COUNT) ++c_split;
      const AnnNode nd = nodes[cur & A_VAL];
      const uint32_t cd = nd.c0 >> 30;
      const double qd = (cd == 0) ? qx : ((cd == 1) ? qy : qz);
      const double cut_diff = qd - nd.cut_val;
      const bool low = cut_diff < 0;
      double box_diff = low ? (nd.lo - qd) : (qd - nd.hi);
      if (box_diff < 0) box_diff = 0;
      const double fbd = bd + (cut_diff * cut_diff - box_diff * box_diff);
      const uint32_t c0 = nd.c0 & (A_LEAF | A_VAL), c1 = nd.c1;
      // the reference tests "box_dist * max_err < max_key()" after the near subtree; the k-th key only ever
      // shrinks, so a far child failing now fails then too and need not be remembered
      if (fbd * max_err < key[KMAX - 1]) st.push(low ? c1 : c0, fbd);
      cur = low ? c0 : c1;
    }
    {                                              // ANNkd_leaf::ann_search, one point (kd_search.cpp:177-210)
      const uint32_t pos = cur & A_VAL;
      if (COUNT) ++c_leaf;
      const KdPoint p = pts[pos];
      const double t0 = qx - p.x, t1 = qy - p.y, t2 = qz - p.z;
      const double dist = (t0 * t0 + t1 * t1) + t2 * t2;
      if (!(dist > key[KMAX - 1])) ann_list_insert(key, info, dist, pos);  // no partial sum exceeded the k-th key
    }
    bool done = false;
    for (;;) {
      if (st.sp == 0) { done = true; break; }
      st.pop(cur, bd);
      if (bd * max_err < key[KMAX - 1]) break;
    }
    if (done) break;
  }
}

}  // namespace tdtk
