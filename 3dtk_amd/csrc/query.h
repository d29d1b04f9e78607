// Argument block and launchers of query.hip: k nearest neighbours, fixed-radius search and the normals built on them.
#pragma once
#include <hip/hip_runtime.h>

#include "tdtk_internal.h"

namespace tdtk {

constexpr int KNN_MAX_K = 64;   // largest k of tdtk_knn_search / tdtk_normals_knn (the LDS-list kernel's capacity)

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
  int32_t* knn_out;            // k-NN normals: the lists [n][k] (nullable)
};

size_t query_overflow_entries(size_t n, uint32_t max_depth);
hipError_t launch_knn(const QueryArgs& a, bool normals, hipStream_t s);
hipError_t launch_range_count(const QueryArgs& a, hipStream_t s);
hipError_t launch_range_fill(const QueryArgs& a, hipStream_t s);
hipError_t launch_range_normals(const QueryArgs& a, hipStream_t s);
size_t range_scan_temp_bytes(size_t n);
hipError_t launch_range_scan(const uint32_t* counts, unsigned long long* offsets, size_t n, void* tmp, size_t tmp_bytes,
                             hipStream_t s);

}  // namespace tdtk
