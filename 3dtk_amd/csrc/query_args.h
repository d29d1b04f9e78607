// The argument block of the query kernels (query.hip) and the constants their per-lane code (query_lane.h) shares with the
// launchers.  No HIP header: a host compiler reads this file as it stands.
#pragma once
#include <cstddef>
#include <cstdint>

#include "tdtk_internal.h"

namespace tdtk {

constexpr int KNN_MAX_K = 64;   // largest k of tdtk_knn_search / tdtk_knn_range_search and their normals (the LDS-list kernel's capacity)

struct QueryArgs {
  const KdNode* nodes;
  const KdPoint* pts;
  const LeafEntry* leaf_tab;   // table mode only
  uint32_t root_ref, cb, cmask;
  const double *x, *y, *z;     // queries, SoA, spatially sorted
  const int32_t* order;        // sorted position -> caller index (nullable: identity)
  size_t n;
  int k;                       // k-NN
  double r2;                   // fixed radius (sqRad2)
  double* ovf_m2;              // stack overflow area: query_overflow_entries(n, max_depth) entries each (nullable when 0)
  uint32_t* ovf_ref;
  int32_t* idx;                // k-NN: [n][k]; range: at offsets
  double* d2;                  // nullable, same layout
  uint32_t* counts;            // range count walk: [n + 1], caller order
  const unsigned long long* offsets;   // range fill walk: [n + 1]
  double rx, ry, rz;           // normals: the scanner position
  double* normals;             // [n][3], caller order
  int32_t* knn_out;            // k-NN normals: the lists [n][k] (nullable); adaptive-k normals: [n][kmax + 1]
  // cylinder / box / segment queries (r2 is their maxdist2; idx / d2 of the nearest-point query: [n], caller order)
  const double* node_r;        // bounding-sphere radius per internal node
  const double *vx, *vy, *vz;  // the query's second vector (dir, p0 or the box's upper corner), sorted like x / y / z
  // adaptive-k normals
  int kmin, kmax;              // adaptive-k normals: every query tries k = kmin + 1 .. kmax + 1
  int32_t* k_used;             // adaptive-k normals: [n] the kidx of the list the normal was computed from (nullable)
  // k nearest within a radius (k, r2, idx / d2 / normals / knn_out as the k-NN kernels')
  int32_t* nr_out;             // [n] the length of every list, caller order (nullable)
  // collision detection along a trajectory: x / y / z are the P model points (spatially sorted), n the number of
  // (frame, model point) or (segment, model point) items, r2 the squared radius
  const double* frames;        // [F][16], column-major
  size_t P;                    // model points
  uint8_t* mask;               // marking: [M], 1 where the model touches the tree's point (input order)
  unsigned long long* dmin;    // depth along the model's axis: [M] the bits of the smallest squared distance
  // radius clustering (cluster_lane.h): n is the tree's slot count (TreeDev::n_slots), the queries are the tree's own points
  // in leaf order (pts), r2 the squared radius.  Slot space: parent / ckey / csize; input-index space: everything else
  uint32_t* parent;            // [n] union-find links
  uint32_t* ckey;              // [n] at a root: the smallest input index of its component (0xFFFFFFFF: none)
  uint32_t* csize;             // [n] at a root: the members of its component
  const uint8_t* subset;       // [M] the nodes (nullable: every point)
  const double* cnormals;      // [M][3] (nullable: no smoothness predicate)
  double min_cos;              // an edge needs fabs(n_i . n_j) >= min_cos
  uint32_t min_size;           // components below it are dropped
  uint32_t* cflag;             // [M + 1] 1 at the key of every kept component; cnum: its exclusive scan (cnum[M]: n_clusters)
  const uint32_t* cnum;
  int32_t* labels;             // [M]
  int32_t* cfirst;             // [M], the first n_clusters written
  uint32_t* csizes_out;        // [M], the first n_clusters written
};

// the four list queries of the shape walks (launch_shape_count / launch_shape_fill)
enum ShapeMode { SHAPE_ALONG_DIR = 0, SHAPE_BETWEEN = 1, SHAPE_AABB = 2, SHAPE_SEGMENT = 3 };

}  // namespace tdtk
