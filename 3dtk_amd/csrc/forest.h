// Launchers of forest.hip (the dynamic kd-forest) and the host-only insert plan (api_forest.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "forest_lane.h"

namespace tdtk {

// queries: a.q as query_prepare left it (x / y / z, order, n, the overflow area sized for the deepest slot)
hipError_t launch_forest_find_closest(const ForestArgs& a, hipStream_t s);   // a.q.r2 = maxdist2; a.q.idx [n], a.q.d2 [n] (nullable)
hipError_t launch_forest_knn(const ForestArgs& a, hipStream_t s);            // a.q.k <= KNN_MAX_K; a.q.idx [n][k], a.q.d2 (nullable)
hipError_t launch_forest_range_count(const ForestArgs& a, hipStream_t s);    // a.q.r2; a.q.counts [n + 1], caller order
hipError_t launch_forest_range_fill(const ForestArgs& a, hipStream_t s);     // a.q.offsets; a.q.idx, a.q.d2 (nullable)
// one round of the remove pass over the a.q.n requests: find and claim, note the losers, commit (a.res, a.cand_c, a.cand_p, a.ctl)
hipError_t launch_forest_remove_round(const ForestArgs& a, hipStream_t s);
// the gathers of a merge: points [n] of a tree or of the buffer -> xyz [.][3] and ids [.] from position `base` on
hipError_t launch_forest_copy_points(const KdPoint* pts, size_t n, double* xyz, int32_t* ids, size_t base, hipStream_t s);   // none removed
hipError_t launch_forest_live_flags(const KdPoint* pts, size_t n, uint32_t* flags, hipStream_t s);                           // flags [n + 1], flags[n] = 0
hipError_t launch_forest_compact_points(const KdPoint* pts, size_t n, const uint32_t* offs, double* xyz, int32_t* ids, size_t base,
                                        hipStream_t s);                                                                      // the live ones, in storage order
hipError_t launch_forest_copy_new(const double* src_xyz, size_t a, size_t b, int32_t first_id, double* xyz, int32_t* ids, size_t base,
                                  hipStream_t s);                                                                            // new points [a, b)
// a freshly built tree's points: orig = ids[orig] (ids null: as built), pad = FOREST_UNCLAIMED
hipError_t launch_forest_relabel(KdPoint* pts, size_t n, const int32_t* ids, hipStream_t s);

// ---- the insert plan -------------------------------------------------------------------------------------------------------
// What inserting m points one at a time does to a forest, from integers alone: the slot counts, the buffer fill, b and m.
// A segment is { kind, a, b }: FOREST_SEG_SLOT: the live points of old slot a (b: their number); FOREST_SEG_NEW: the new
// points [a, b) in insertion order; FOREST_SEG_BUFFER: the old buffer (b: its fill).
enum { FOREST_SEG_SLOT = 0, FOREST_SEG_NEW = 1, FOREST_SEG_BUFFER = 2 };
struct ForestSeg { int64_t kind, a, b; };
struct ForestPlan {
  std::vector<uint64_t> counts;                 // live points of every final slot (0: empty)
  std::vector<std::vector<ForestSeg>> segs;     // ... and where they come from; an untouched slot s is { { SLOT, s, count } }
  bool keeps_buffer;                            // the old buffer is still (the front of) the buffer: no merge happened
  uint64_t buf_a, buf_b;                        // the new points [buf_a, buf_b) behind it
  uint64_t merges;
};
void forest_plan(const std::vector<uint64_t>& counts, uint64_t fill, uint64_t bucket, uint64_t m, ForestPlan& out);

}  // namespace tdtk
