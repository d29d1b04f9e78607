// Argument block and launchers of query.hip: k nearest neighbours, fixed-radius and k-nearest-within-radius search, the normals
// built on them, and the
// cylinder / box / segment queries.
#pragma once
#include <hip/hip_runtime.h>

#include "query_args.h"

namespace tdtk {

size_t query_overflow_entries(size_t n, uint32_t max_depth);
hipError_t launch_knn(const QueryArgs& a, bool normals, hipStream_t s);
hipError_t launch_knn_range(const QueryArgs& a, bool normals, hipStream_t s);  // launch_knn within a.r2; a.nr_out
hipError_t launch_knn_adaptive(const QueryArgs& a, hipStream_t s);            // kmax + 1 <= KNN_MAX_K; a.normals, a.k_used, a.knn_out
hipError_t launch_range_count(const QueryArgs& a, hipStream_t s);
hipError_t launch_range_fill(const QueryArgs& a, hipStream_t s);
hipError_t launch_range_normals(const QueryArgs& a, hipStream_t s);
hipError_t launch_shape_count(const QueryArgs& a, int mode, hipStream_t s);   // a.counts, as launch_range_count
hipError_t launch_shape_fill(const QueryArgs& a, int mode, hipStream_t s);    // a.idx at a.offsets, as launch_range_fill
hipError_t launch_segment_nearest(const QueryArgs& a, hipStream_t s);         // a.idx [n], a.d2 [n] (nullable)
// collision detection (a.x / y / z the model, a.frames, a.P, a.n items, a.r2)
hipError_t launch_collide_mark(const QueryArgs& a, int cmethod, hipStream_t s);   // a.mask (cleared by the caller); 1: spheres, 2: segments
hipError_t launch_collide_count(const uint8_t* mask, size_t M, unsigned long long* count, hipStream_t s);   // *count += set bytes
hipError_t launch_collide_depth_init(unsigned long long* dmin, size_t M, hipStream_t s);
hipError_t launch_collide_depth_axis(const QueryArgs& a, hipStream_t s);          // a.dmin
hipError_t launch_collide_depth_finish(const unsigned long long* dmin, size_t M, float* dist, hipStream_t s);
// radius clustering (cluster_lane.h): a.n the tree's slots, a.parent / ckey / csize, a.subset, a.cnormals, a.min_cos, a.r2
hipError_t launch_cluster_init(const QueryArgs& a, hipStream_t s);
hipError_t launch_cluster_link(const QueryArgs& a, uint32_t max_blocks, hipStream_t s);   // max_blocks: a smaller grid (0: none)
hipError_t launch_cluster_flatten(const QueryArgs& a, hipStream_t s);             // + a.cflag (zeroed), a.min_size
hipError_t launch_cluster_label(const QueryArgs& a, hipStream_t s);               // a.cnum; a.labels, a.cfirst, a.csizes_out
size_t range_scan_temp_bytes(size_t n);
hipError_t launch_range_scan(const uint32_t* counts, unsigned long long* offsets, size_t n, void* tmp, size_t tmp_bytes,
                             hipStream_t s);

}  // namespace tdtk
