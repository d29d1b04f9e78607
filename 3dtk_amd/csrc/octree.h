// Argument blocks and launchers of octree.hip: the device BOctTree (tdtk_octree_*), its build and its search.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "oct_lane.h"

namespace tdtk {

// ---- build: the node table over the sorted cell keys (reduce.hip computes, sorts and orders them) ----------------------
// counts [32]: [L] = nodes at depth L (1 .. depth), [31] = leaves.  Zeroed by the caller.
hipError_t launch_oct_leaf_depth(uint64_t* sorted, size_t n, int depth, int earlystop, uint8_t* ld, uint32_t* counts, hipStream_t s);
// the keys in the caller's order with everything below the point's leaf cleared (what launch_oct_leaf_order partitions by)
hipError_t launch_oct_mask_keys(uint64_t* keys, const uint64_t* sorted_full, const uint8_t* ld, size_t n, int depth, hipStream_t s);
hipError_t launch_oct_mask_sorted(uint64_t* sorted, const uint8_t* ld, size_t n, int depth, hipStream_t s);
// one level: flags [n + 1] (flags[n] = 0) where a node of depth L starts; then, behind their exclusive scan `rank`, the emit
hipError_t launch_oct_level_flags(const uint64_t* sorted, const uint8_t* ld, size_t n, int depth, int L, uint32_t* flags, hipStream_t s);
struct OctEmit {
  const uint64_t* sorted;
  const uint8_t* ld;
  const uint32_t *flags, *rank;             // of level L
  const uint32_t *pflags, *prank;           // of level L - 1 (unused for L == 1)
  OctNode* nodes;
  uint32_t base, pbase;                     // first slot of level L / L - 1
  uint32_t n;
  int depth, L;
};
hipError_t launch_oct_level_emit(const OctEmit& e, hipStream_t s);
hipError_t launch_oct_points(const double* xyz, const uint32_t* perm, size_t n, KdPoint* pts, hipStream_t s);

// ---- search ------------------------------------------------------------------------------------------------------------
// before the walk: the queries into the tree's frame and their range check
struct OctPrepArgs {
  const double *x, *y, *z;   // queries, SoA, spatially sorted
  double *ox, *oy, *oz;      // has_inv: out, transform3(inv, .) of every query (SearchTree::getPtPairs, searchTree.cc:122)
  size_t n;
  Mat4 inv;
  int has_inv;
  double add[3], mult;       // the tree's (OctView)
  uint32_t* bad;             // one word, zeroed by the caller: set when a query's voxel coordinate does not fit +-2^30
};
struct OctSearchArgs {
  OctView T;
  const double *x, *y, *z;   // queries in the tree's frame, SoA, spatially sorted
  size_t n;
  int levels;                // the tree's levels: sizes the per-lane stack
  double maxd2;
  int* kpos;                 // out: the hit's slot in the point array, or -1
  double* d2;                // out, nullable
};
// sets *bad, to be looked at before launch_oct_search
hipError_t launch_oct_prepare(const OctPrepArgs& a, hipStream_t s);
hipError_t launch_oct_search(const OctSearchArgs& a, hipStream_t s);

// ---- the ICP loop (tdtk_icp_match_octree): the same two passes with nothing for the host to do in between ---------------
// the prepare pass of an iteration: first the previous iteration's alignxf in place over the resident scan (k_transform's
// arithmetic: the octree's SearchArgs::pending), then the tree-frame coordinates and the range word as k_oct_prepare
struct OctLoopPrepArgs {
  double *x, *y, *z;         // the resident scan, SoA, spatially sorted: moved in place when has_pending
  double *nx, *ny, *nz;      // its normals (nullable): moved with it
  double *ox, *oy, *oz;      // out: transform3(inv, .) of every (moved) point
  size_t n;
  Mat4 pending, inv;
  int has_pending;
  double add[3], mult;
  uint32_t* bad;             // one word, zeroed by the caller
};
// the walk: reads the range word itself (set: every query gets kpos = -1 and nothing is converted to int) and the -R keep
// bytes (SearchArgs::skip's format, nullable: a query whose byte is set gets kpos = -1 and is not walked)
struct OctLoopSearchArgs {
  OctView T;
  const double *x, *y, *z;   // queries in the tree's frame (OctLoopPrepArgs::ox ..)
  size_t n;
  int levels;
  double maxd2;
  int* kpos;
  const unsigned char* skip;
  const uint32_t* bad;
};
hipError_t launch_oct_loop_prepare(const OctLoopPrepArgs& a, hipStream_t s);
hipError_t launch_oct_loop_search(const OctLoopSearchArgs& a, hipStream_t s);

}  // namespace tdtk
