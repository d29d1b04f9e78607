/*
 * tdtk_hip.h -- C ABI of lib3dtk_hip.so, the MI355X (gfx950) implementation of
 * 3DTK's slam6D ICP correspondence + alignment hot path.
 *
 * Plain C types only; caller owns every host buffer; the library never frees
 * caller memory; no exception crosses this boundary: every function returns
 * TDTK_OK (0) or a negative TDTK_E* code and tdtk_last_error() gives the text
 * (per calling thread).  Handles are opaque; functions are re-entrant across
 * handles.  All floating point is fp64 with FMA contraction off, so that
 * correspondence indices are bit-exact with the reference KDtree.
 *
 * 4x4 matrices are column-major ("OpenGL order", translation in [12..14]) as
 * everywhere in the reference (include/slam6d/globals.icc:298-328).
 *
 * Each entry point names the reference interface it replaces (paths relative
 * to the JMUWRobotics/3DTK checkout).  The reference-side bindings that call
 * these are shown in INTEGRATION.md.
 */
#ifndef TDTK_HIP_H
#define TDTK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TDTK_OK 0
#define TDTK_EINVAL (-1)   /* bad argument (NULL, zero points, bucket < 1 ...)        */
#define TDTK_EDEVICE (-2)  /* no usable gfx950 device / HIP runtime error             */
#define TDTK_ENOMEM (-3)   /* host or device allocation failed                        */
#define TDTK_ESOLVE (-4)   /* minimizer could not be solved (Cholesky failed, ...)    */
#define TDTK_EUNSUP (-5)   /* valid in the reference but not supported on this entry point */
#define TDTK_EPEER (-6)    /* another rank of the communicator failed; the collective result is void on every rank */

typedef struct tdtk_tree tdtk_tree; /* model-scan search tree, resident in HBM   */
typedef struct tdtk_scan tdtk_scan; /* data-scan points (+normals), resident in HBM */

/* include/slam6d/pairingMode.h:4-8 */
enum {
  TDTK_CLOSEST_POINT = 0,
  TDTK_CLOSEST_POINT_ALONG_NORMAL_SIMPLE = 1,
  TDTK_CLOSEST_PLANE_SIMPLE = 2
};

/* minimizer ids == the -a values of src/slam6d/slam6D.cc:696-727.  QUAT / SVD / APX / NAPX are the ones
 * an OpenMP build of the reference can run (Align_Parallel, icp6D.cc:201-219); the other six exist only
 * as serial Align (icp6Dortho.cc, icp6Ddual.cc, icp6Dhelix.cc, icp6Dlumeuler.cc, icp6Dlumquat.cc,
 * icp6Dquatscale.cc) and are computed here from the second-moment block TDTK_WANT_MOM2.      */
enum {
  TDTK_ALGO_QUAT = 1, TDTK_ALGO_SVD = 2, TDTK_ALGO_ORTHO = 3, TDTK_ALGO_DUAL = 4, TDTK_ALGO_HELIX = 5,
  TDTK_ALGO_APX = 6, TDTK_ALGO_LUMEULER = 7, TDTK_ALGO_LUMQUAT = 8, TDTK_ALGO_QUAT_SCALE = 9,
  TDTK_ALGO_NAPX = 10
};

/* which accumulator blocks tdtk_scan_pairs / tdtk_get_pt_pairs should fill */
#define TDTK_WANT_BASE 0u  /* n, sum, centroids, Si: always                              */
#define TDTK_WANT_APX 1u   /* A[6], B[3] of icp6D_APX (src/slam6d/icp6Dapx.cc:203-245)   */
#define TDTK_WANT_NAPX 2u  /* A[21], B[6], sum of icp6D_NAPX (icp6Dnapx.cc:53-95)        */
#define TDTK_WANT_LUM 4u   /* the 15 sums + ss of lum6DEuler::covarianceEuler            */
#define TDTK_WANT_GAPX 8u  /* the per-link blocks of gapx6D::genBArotForLinkedPair (alone) */
#define TDTK_WANT_MOM2 16u /* centred second moments of p1 and of p2 (alone): with n, centroids and
                            * Si they are the full second-moment matrix of (p1 ; p2), from which
                            * every minimizer that is quadratic in the pairs follows            */

/* Merged per-call sums: what T OpenMP threads' (n, sum, centroid_m, centroid_d, Si)
 * of src/slam6d/icp6D.cc:129-192 add up to; feed slot 0 of Align_Parallel with it. */
typedef struct tdtk_pair_sums {
  uint64_t n_queries;    /* queries issued                                             */
  uint64_t n;            /* pairs found (pairs.size())                                  */
  double sum;            /* sum |p1-p2|^2              searchTree.cc:172-177            */
  double centroid_m[3];  /* mean of p1 (model, world)  scan.cc:1253-1259 (normalised)   */
  double centroid_d[3];  /* mean of p2 (data)                                           */
  double Si[9];          /* sum (p1-cm)[a]*(p2-cd)[b] at [a*3+b]   icp6D.cc:170-191     */
  double apx_A[6];       /* A00 A01 A02 A11 A12 A22 about centroid_d (icp6Dapx.cc:203)  */
  double apx_B[3];
  double napx_A[21];     /* upper triangle row-major, about centroid_d                  */
  double napx_B[6];
  double napx_sum;       /* sum ((p1-p2).n)^2                                           */
  double lum[15];        /* sx sy sz xpy xpz ypz xy xz yz MZ[0..5]  lum6Deuler.cc:143-175 */
  double lum_sumd2;      /* sum |p1-p2|^2 (== sum), kept for the ss identity check      */
  /* gapx6D::genBArotForLinkedPair (src/slam6d/gapx6D.cc:153-310), both points centred on
   * centroid_m, including the literal `p1x*p2x + p1y + p2y` diagonal terms (gapx6D.cc:208-210) */
  double gapx_MkMkt[9], gapx_DkDkt[9], gapx_MkDkt[9], gapx_DkMkt[9];   /* row-major 3x3 */
  double gapx_Ak1[3], gapx_Ak2[3];
  double mom_mm[6];      /* sum (p1-cm)(p1-cm)^T: xx xy xz yy yz zz        [TDTK_WANT_MOM2]   */
  double mom_dd[6];      /* sum (p2-cd)(p2-cd)^T                                              */
  double lum_udot;       /* sum u.delta (lum6DQuat's MZ(4), lum6Dquat.cc:163)     [TDTK_WANT_LUM]  */
} tdtk_pair_sums;

typedef struct tdtk_tree_info {
  uint64_t n_points, n_internal, n_leaves;
  uint32_t max_depth, max_leaf_points;
  uint64_t device_bytes;
  double build_ms, upload_ms;
} tdtk_tree_info;

typedef struct tdtk_icp_params {
  int algo;                /* TDTK_ALGO_*                           slam6D.cc:696-727   */
  int pairing_mode;        /* TDTK_CLOSEST_*                        slam6D.cc:756-763   */
  int max_num_iterations;  /* -i                                    icp6D.cc:122        */
  double max_dist_match2;  /* sqr(-d)                               icp6D.cc:80         */
  double epsilon_icp;      /* --epsICP                              icp6D.cc:266-267    */
  int quiet;               /* 0: print the reference's per-iteration RMS line           */
} tdtk_icp_params;

typedef struct tdtk_icp_result {
  int iterations;          /* value icp6D::match returns (icp6D.cc:284)                 */
  int converged;           /* 1 if the epsilon test fired, 0 if the cap / too few pairs */
  uint64_t last_pairs;     /* nr_pointPair                                              */
  double last_rms;         /* last `ret`                                                */
  double total_ms;         /* wall time of the loop (the reference's "TIME" line)       */
  double nn_ms;            /* of which: device time in the correspondence kernel (0 unless tdtk_kernel_timing) */
  double sums_ms;          /* and in the pair-sum kernels behind it (k_final alone when the sums are fused) */
} tdtk_icp_result;

/* ---- library ------------------------------------------------------------ */
const char* tdtk_last_error(void);
int tdtk_device_count(void);
/* Device memory of destroyed trees and scans is kept for the next handle of about that size (up to TDTK_POOL_MB megabytes
 * per device, default 1024; 0: every array goes straight back to the driver).  tdtk_pool_trim gives what is kept back
 * now and returns the number of bytes released.                                                                    */
size_t tdtk_pool_trim(void);
/* Diagnostics: how many device tree builds of this process had to be redone in order because a node cut at the plain
 * parallel sum of its points would have been cut elsewhere at the exact serial sum (build.hip, "speculative splits";
 * the tree that comes out is the same either way).  Expected to stay 0 outside the test that forces it.             */
uint64_t tdtk_build_respeculated(void);
const char* tdtk_version(void);

/* ---- model tree: replaces KDtree::KDtree(double**, int, int) (src/slam6d/kd.cc:46-49,
 * KDTreeImpl::create include/slam6d/kdTreeImpl.h:82-201) as created by
 * BasicScan::createSearchTreePrivate (src/slam6d/basicScan.cc:702-728).
 * xyz = "xyz reduced original" [M][3] row-major in the tree frame; it is COPIED
 * (the reference tree borrows it).  Builds the identical tree (same split rule,
 * same partition order), lays it out breadth-first and uploads it.             */
int tdtk_tree_create(const double* xyz, size_t M, int bucket_size, int device, tdtk_tree** out);
/* The same tree over the points of a resident scan as they are now, in the caller's order: what BasicScan
 * builds over "xyz reduced original" (src/slam6d/basicScan.cc:702-728) when asked before the scan has been moved;
 * the points never visit the host.                                                                    */
int tdtk_tree_create_from_scan(const tdtk_scan* scan, int bucket_size, tdtk_tree** out);
/* KDtreeMetaManaged (src/slam6d/kdMeta.cc:34-134) for a MetaScan: one tree over the CURRENT points of several
 * resident scans, concatenated in the order given (prepareTempIndices, kdMeta.cc:60-79); indices returned by
 * searches on it count through that concatenation.                                                    */
int tdtk_tree_create_from_scans(tdtk_scan* const* scans, int nscans, int bucket_size, tdtk_tree** out);
void tdtk_tree_destroy(tdtk_tree* t);
int tdtk_tree_get_info(const tdtk_tree* t, tdtk_tree_info* info);
/* diagnostic: rebuild the tree with the host builder (kd_build.cpp; this is its only use -- trees are always built on
 * the device) and compare it with the resident one.  mismatches = {node records, node radii, points, structure}. */
int tdtk_tree_verify(const tdtk_tree* t, uint64_t mismatches[4]);
/* diagnostic: which way the device build of this tree took through its hand-over to the subtree finishers (host-side
 * bookkeeping of build.hip's decisions; nothing forces a path).  out = { planned_level (the level the plan hands over at,
 * 0xFFFFFFFF: none), handed_level (the level the delivered tree was handed over at, 0xFFFFFFFF: finished by levels),
 * more_levels (times "one more level"), retried (0 / 1: finishers given up, on by levels with a look every second level),
 * refused_size, refused_count (looks of the retry refused because the largest node exceeds a workgroup's capacity /
 * because the level has more nodes than fin_cap; a look refused for both counts in both), fin_nodes, fin_maxn (the
 * level's nodes and the largest of them at the hand-over), finishers (bit 0 the wave finisher, bit 1 the half-size,
 * bit 2 the full-size workgroup finisher), redone_by_levels (the first attempt met a subtree deeper than the finishers'
 * tables and the build was redone by levels: every field but handed_level describes that first attempt),
 * respeculated, fin_cap (subtrees the tables hold) }.  A tree no device build made: all-ones in out[0], zeros elsewhere. */
int tdtk_tree_build_path(const tdtk_tree* t, uint32_t out[12]);

/* ---- batched KDtree::FindClosest (kd.cc:78-87; _FindClosest kdTreeImpl.h:345-383).
 * q [K][3] in the tree frame, host memory.  idx[k] = index into the xyz given to
 * tdtk_tree_create, or -1 (the reference returns NULL).  d2 nullable.           */
int tdtk_find_closest(const tdtk_tree* t, const double* q, size_t K, double maxdist2,
                      int32_t* idx, double* d2);
/* same with device pointers (inputs already resident in HBM); stream = hipStream_t or NULL.
 * presorted != 0 promises that q is already spatially ordered (skips the binning pass).
 * With a caller's stream the call returns with the work queued on it; the kernels use the calling thread's
 * workspaces, so later tdtk calls of this thread are ordered behind them (stream-wait on an event), but the
 * caller must not issue a second tdtk_find_closest_dev on ANOTHER stream before the first has finished. */
int tdtk_find_closest_dev(const tdtk_tree* t, const double* d_q, size_t K, double maxdist2,
                          int32_t* d_idx, double* d_d2, int presorted, void* stream);

/* batched KDtree::FindClosestAlongDir (kd.cc:89-100; kdTreeImpl.h:390-425) */
int tdtk_find_closest_along_dir(const tdtk_tree* t, const double* q, const double* dir, size_t K,
                                double maxdist2, int32_t* idx, double* d2);

/* ---- batched KDtreeIndexed::kNearestNeighbors (kdIndexed.cc:125-161; _KNNSearch kdTreeImpl.h:627-682).  q [K][3] in
 * the tree frame, host memory.  idx [K][k]: indices into the xyz given to tdtk_tree_create (through the concatenation
 * for trees from scans), nearest first, ties in the reference's visiting order; d2 (nullable) [K][k] their squared
 * distances.  A tree of M < k points gives M entries per row, the rest -1 / -1.0.  Errors: k < 1 (TDTK_EINVAL),
 * k > 64 (TDTK_EUNSUP: the device lists hold at most 64 entries).                                          */
int tdtk_knn_search(const tdtk_tree* t, const double* q, size_t K, int k, int32_t* idx, double* d2);
/* batched KDtree::kNearestRangeSearch (kd.cc:137-171; _KNNRangeSearch kdTreeImpl.h:684-745, the pointer flavour the Python
 * binding offers, py3dtk.cc:538-545): of the points with Dist2 < sqRad2 the k nearest, nearest first, ties in the walk's
 * visiting order.  idx [K][k], -1 behind a row's entries; d2 (nullable) [K][k], -1.0 there; counts (nullable) [K] the
 * number of entries, 0 .. k.  The reference returns the points' coordinates, this call their indices.  Errors, in this
 * order and before anything is launched or written: NULL t / q / idx, k < 1 (TDTK_EINVAL); k > 64 (TDTK_EUNSUP); a
 * non-finite sqRad2 (TDTK_EINVAL -- a deviation: the reference would walk with comparisons that are all false).
 * sqRad2 <= 0 gives empty rows and launches nothing; K == 0 is a no-op.                                      */
int tdtk_knn_range_search(const tdtk_tree* t, const double* q, size_t K, int k, double sqRad2, int32_t* idx, double* d2,
                          int32_t* counts);
/* batched KDtreeIndexed::fixedRangeSearch (kdIndexed.cc:215-230; _FixedRangeSearch kdTreeImpl.h:585-625): every point
 * with Dist2 < sqRad2, in the reference's visiting order, as CSR lists.  offsets [K+1] is always filled (query i owns
 * idx[offsets[i] .. offsets[i+1])) and *total = offsets[K].  When cap < *total nothing else is written and the call
 * returns TDTK_EINVAL: call again with cap >= *total, the lists are the same.  d2 nullable.  sqRad2 <= 0 gives
 * empty lists.                                                                                             */
int tdtk_fixed_range_search(const tdtk_tree* t, const double* q, size_t K, double sqRad2, uint64_t* offsets,
                            int32_t* idx, double* d2, size_t cap, uint64_t* total);
/* ---- the cylinder, box and segment queries of KDtreeIndexed, batched.  Query i is (p[i], v[i]), both [K][3] host memory in
 * the tree frame; maxdist2 is one value per call.  The four list queries return CSR lists under tdtk_fixed_range_search's
 * contract: offsets [K+1] and *total are always filled, cap < *total writes nothing else and returns TDTK_EINVAL (the
 * message names both numbers), K == 0 is a no-op; the lists hold original point indices in the reference's visiting
 * order.  Degenerate input (p == p0, a zero or non-unit dir, NaN / infinite coordinates) gives the reference's answer. */
/* KDtreeIndexed::fixedRangeSearchAlongDir (kdIndexed.cc:195-213; _fixedRangeSearchAlongDir kdTreeImpl.h:491-536): every
 * point closer than sqrt(maxdist2) to the line through p along dir; dir is used as given, not normalised. */
int tdtk_fixed_range_search_along_dir(const tdtk_tree* t, const double* p, const double* dir, size_t K, double maxdist2,
                                      uint64_t* offsets, int32_t* idx, size_t cap, uint64_t* total);
/* KDtreeIndexed::fixedRangeSearchBetween2Points (kdIndexed.cc:164-192; _fixedRangeSearchBetween2Points kdTreeImpl.h:
 * 432-483): the same with dir = (p0 - p) normalised and the reference's two extra tests at the root. */
int tdtk_fixed_range_search_between(const tdtk_tree* t, const double* p, const double* p0, size_t K, double maxdist2,
                                    uint64_t* offsets, int32_t* idx, size_t cap, uint64_t* total);
/* KDtreeIndexed::AABBSearch (kdIndexed.cc:233-250; _AABBSearch kdTreeImpl.h:542-577): the points the reference's box walk
 * collects for the box [lo, hi] -- a subset of the points in the box that depends on the bucket size.  A box with
 * lo[i] > hi[i] anywhere in the batch: TDTK_EINVAL "invalid bbox" (the reference throws), nothing written or launched. */
int tdtk_aabb_search(const tdtk_tree* t, const double* lo, const double* hi, size_t K, uint64_t* offsets, int32_t* idx,
                     size_t cap, uint64_t* total);
/* KDtreeIndexed::segmentSearch_all (kdIndexed.cc:252-278; _segmentSearch_all kdTreeImpl.h:747-820): every point closer
 * than sqrt(maxdist2) to the segment p .. p0. */
int tdtk_segment_search_all(const tdtk_tree* t, const double* p, const double* p0, size_t K, double maxdist2,
                            uint64_t* offsets, int32_t* idx, size_t cap, uint64_t* total);
/* KDtreeIndexed::segmentSearch_1NearestPoint (kdIndexed.cc:280-301; _segmentSearch_1NearestPoint kdTreeImpl.h:828-913):
 * of those points the one nearest to p.  idx [K]: its index or -1 (the reference returns size_t max); d2 (nullable) [K]:
 * its squared distance to p or -1.0. */
int tdtk_segment_search_nearest(const tdtk_tree* t, const double* p, const double* p0, size_t K, double maxdist2,
                                int32_t* idx, double* d2);
/* collision_model's handle_pointcloud (collision_model.cc:312-430): the point model [P][3] moves through the tree's cloud
 * along the trajectory frames [F][16] (column-major, as read_trajectory leaves them); colliding [M] (the tree's input
 * order) gets 1 for every point the model touches and 0 elsewhere, num_colliding their number.  cmethod 1 (CTYPE1,
 * :338-367): the points of fixedRangeSearch(transform3(T_j, m), radius^2) for every frame j and model point m; cmethod 2
 * (CTYPE2, :368-410): the points of segmentSearch_all(transform3(T_j, m), transform3(T_j+1, m), radius^2) for every pair
 * of consecutive frames -- two identical frames give a segment of length zero, which lists nothing.  The queries are
 * generated on the device; nothing of size F x P is stored.  F == 0 with cmethod 1 and F == 1 with cmethod 2 mark nothing;
 * non-finite model or frame entries are not errors (their queries list what the reference's walks list: nothing).
 * TDTK_EINVAL, before anything is launched or written: a NULL, P == 0, radius non-finite or <= 0, cmethod not 1 or 2,
 * cmethod 2 with F == 0 (the reference dereferences an empty vector). */
int tdtk_collision_mark(const tdtk_tree* env, const double* model, size_t P, const double* frames, size_t F, double radius,
                        int cmethod, uint8_t* colliding, uint64_t* num_colliding);
/* calculate_collidingdist (collision_model.cc:637-712): a KDtreeIndexed(bucket) over the non-colliding points of env_xyz
 * [M][3] in ascending index, and for every colliding point, in ascending index, dist = (float)sqrt(Dist2(point, nearest))
 * of FindClosest(point, 1000000).  dist [number of set bytes of colliding].  A colliding point with no non-colliding
 * point within maxdist2 (the reference indexes out of bounds there) keeps 1000.0f; n_unreached (nullable): how many.
 * TDTK_EINVAL: a NULL, no colliding point, no non-colliding point (the reference's tree constructor throws), bucket < 1. */
int tdtk_collision_depth_closest(const double* env_xyz, size_t M, const uint8_t* colliding, int bucket, int device,
                                 float* dist, uint64_t* n_unreached);
/* calculate_collidingdist2 (collision_model.cc:714-800): a KDtreeIndexed(bucket) over the colliding points in ascending
 * index; for every frame and model point (x, y, z): p1 = transform3(T, (x, y, z)), p2 = transform3(T, (0, y, 0)), c1 =
 * segmentSearch_1NearestPoint(p1, p2, radius^2), and every point of fixedRangeSearch(c1, radius^2) takes the minimum of
 * Dist2(p1, c1).  dist [number of set bytes of colliding], by compact index: (float)sqrt of the float the reference
 * keeps, sqrtf(1000.0f) where no query reached the point.  The minimum does not depend on the order of the updates, so the
 * result is the reference's at any number of threads.  TDTK_EINVAL as tdtk_collision_mark, and with no colliding point. */
int tdtk_collision_depth_axis(const double* env_xyz, size_t M, const uint8_t* colliding, const double* model, size_t P,
                              const double* frames, size_t F, double radius, int bucket, int device, float* dist);
/* Radius (Euclidean) clustering: the connected components of the fixed-radius graph over the tree's points -- what
 * src/collision/segment_colliding.cc:55-102 groups the colliding points by (its radius is the literal 20 of :61).
 * RELATION: points i and j are joined exactly when j is in KDtreeIndexed::fixedRangeSearch(p_i, sqRad2), that is
 * Dist2(p_i, p_j) < sqRad2 -- a strict '<', Dist2 = (dx*dx + dy*dy) + dz*dz in fp64 without FMA contraction, as everywhere
 * in this library.  The relation is symmetric bit for bit and does not depend on the bucket size.
 * DEVIATION: the result is pinned to that relation, NOT to the bookkeeping of segment_colliding.cc, which does not
 * produce the components of its own relation: line 77 clears the list line 76 has just appended to when the neighbour is
 * the point itself, and line 100 clears group2points[it], indexed by a POINT, where the merged group current_group was
 * meant -- members are lost and groups survive empty or merged twice (tests/test_clusters_host.py keeps the evidence).
 * NODES: the points with subset[i] != 0 (subset NULL: all M = n_points points; indices are those of the xyz given to
 * tdtk_tree_create, counted through the concatenation for trees built from scans).  A point outside the subset gets label
 * -1 and bridges nothing: clustering a subset on the full tree gives the partition a tree over the subset alone gives
 * (segment_colliding's use: it reads the scan of colliding points).
 * EDGES: Dist2 < sqRad2 and, when normals [M][3] is given, fabs((nx_i*nx_j + ny_i*ny_j) + nz_i*nz_j) >= min_abs_cos,
 * evaluated in this sense (a NaN gives no edge).  This smoothness predicate is THIS LIBRARY'S OWN addition (the
 * order-independent form of planar segmentation); the reference has no counterpart.  normals == NULL ignores min_abs_cos.
 * CANONICAL NUMBERING: a component's key is its smallest member index.  Components with fewer than min_size members are
 * dropped, their points get -1 (min_size 0 and 1 keep everything).  The kept components are numbered 0 .. n_clusters-1 in
 * ascending key order; labels [M]: that number; first (nullable) [M]: first[c] the key, sizes (nullable) [M]: sizes[c] the
 * member count of cluster c -- only the first n_clusters entries of both are written.  The output does not depend on the
 * launch geometry, on the order of the atomics, on the bucket size or on earlier calls.
 * sqRad2 <= 0 launches no walk: range lists are empty, every node is a component of its own.  (A point with a NaN
 * coordinate would be one at any radius, not even its own neighbour -- but no tree holds one: tdtk_tree_create refuses
 * non-finite coordinates, and the reference's constructor does not return on them.)
 * TDTK_EINVAL, checked in this order before anything is launched or written: NULL t, labels or n_clusters; sqRad2
 * non-finite; normals given and min_abs_cos outside [0, 1] or NaN.
 * Nothing of the size of the neighbour lists exists anywhere: a lock-free union-find in leaf order (cluster_lane.h). */
int tdtk_cluster_radius(const tdtk_tree* t, double sqRad2, const uint8_t* subset, const double* normals, double min_abs_cos,
                        uint32_t min_size, int32_t* labels, uint64_t* n_clusters, int32_t* first, uint32_t* sizes);
/* The largest grid (workgroups) the link kernel of tdtk_cluster_radius may take, process-wide; 0 (the default): no cap of
 * its own.  A testing aid like tdtk_kernel_timing -- the labels do not depend on it.  Returns the previous setting. */
int tdtk_cluster_grid_cap(int blocks);
/* ---- the voxel grid of peopleremover (src/peopleremover/common.cc, peopleremover.cc).  A voxel is voxel_of_point
 * (common.cc:48-54): py_div(p, voxel_size) per axis.  Voxel coordinates must fit 21 bits with a margin: every |x / voxel_size|
 * of a point, origin or ray end has to stay below 2^20 - 4, otherwise TDTK_EUNSUP.  Non-finite coordinates and a voxel_size
 * that is not finite and > 0 give TDTK_EINVAL.  Nothing is written to the result arrays of a refused call.
 *
 * walk_voxels (common.cc:112-306) for m rays starts[i] -> ends[i] (both [m][3], host memory): the ordered list of voxels the
 * reference hands to its visitor, every call counted, repeats included, under a visitor that always continues.  CSR lists
 * under tdtk_fixed_range_search's contract: offsets [m+1] and *total are always filled; cap < *total (or voxels == NULL with
 * *total > 0) writes nothing else and returns TDTK_EINVAL: call again with cap >= *total.  voxels [cap][3].  A zero-length
 * ray has an empty list.  More than 2^32 - 1 visits in one call: TDTK_EUNSUP.                                            */
int tdtk_voxel_walk(int device, const double* starts, const double* ends, size_t m, double voxel_size, uint64_t* offsets,
                    int32_t* voxels, size_t cap, uint64_t* total);
/* peopleremover's main() between reading the scans and writing the partition (peopleremover.cc:176-545) with
 * --maxrange-method none: occupancy (voxel -> set of scan ids), one ray from every scan's origin to every one of its points
 * under `visitor` (common.cc:57-103; window [current - diff, current + diff]), the cluster filter when cluster_size > 1
 * (26-connected components of the free voxels, fewer than cluster_size voxels: removed), the half-free voxels when subvoxel
 * != 0 (distance 2), and the split.  xyz [n][3] the points of all scans in the global frame, scan s owning rows
 * scan_offsets[s] .. scan_offsets[s+1] (S + 1 entries, from 0, not decreasing, n = scan_offsets[S] > 0); origins [S][3];
 * ray_ends NULL, or [n][3] where each ray stops instead of at its point (shortened rays: the caller's maxranges).
 * dynamic [n]: 1 where the reference writes the point to the dynamic file, else 0.  info [5]: occupied voxels, freed voxels,
 * free voxels after clustering, half-free voxels -- the four numbers the reference prints -- and the voxel visits of all rays.
 * free_voxels (nullable) [cap][3]: the free voxels after clustering in std::set order (x, then y, then z); cap < info[2]
 * returns TDTK_EINVAL with dynamic and info written.  The reference's defaults: voxel_size 10, diff 0, cluster_size 5,
 * subvoxel 1 (common.cc:432-435).  Not covered: --maxrange-method normals, --reduce, fuzz.                            */
int tdtk_peopleremover(int device, const double* xyz, const uint64_t* scan_offsets, const double* origins,
                       const double* ray_ends, size_t S, double voxel_size, uint64_t diff, uint64_t cluster_size, int subvoxel,
                       uint8_t* dynamic, int32_t* free_voxels, size_t cap, uint64_t* info);
/* HIP-event times of the calling thread's last tdtk_peopleremover, ms: occupancy build, walk, cluster + half-free +
 * classification, and first upload to last download.                                                                 */
int tdtk_peopleremover_timings(double* ms4);
/* ---- the standard 3D Hough transform for plane detection (src/shapes: Hough::SHT hough.cc:222-265, accumulator.cc), up to
 * plane candidates.  An accumulator is C cells (plane directions) x RhoNum bins of rho; counts [C][RhoNum] int32, cell-major.
 * Accumulator types as ConfigFileHough's AccumulatorType: 0 Simple, 1 Ball, 2 Cube, 3 BallI.  dims [4] = { RhoNum, PhiNum,
 * ThetaNum, RhoMax }, the reference's unsigned ints.  An entry of a peak list is the reference's int array: (count, rho,
 * theta, phi) for types 0, 1, 3, (count, rho, face, i, j) for type 2.  Not covered: the randomized variants (RHT, PHT, PPHT,
 * APHT), peakWindow, accumulate(theta, phi, rho) / accumulateRet / accumulateAPHT, and the second half of deletePoints
 * (projection, clustering, convex hull, the deletion of points between peaks).
 *
 * The cell normals of an accumulator, host only: the n of Accumulator*::accumulate(Point) for every cell, in the order of that
 * type's getMax() loops without the rho loop (phi, theta; type 2: face, i, j), quirks as written -- the 0.99999999999 /
 * 0.999999999 factors in phi, the clamps, Normalize3 on every normal, BallI's south pole recognised by i == RhoNum - 1 (which
 * makes RhoNum an input of type 3's table; it is dims[0] for every type).  *C (always filled when the arguments pass) is the
 * number of cells; slice_sizes (nullable) [PhiNum] the cells per phi slice (type 2: [6], nrCells^2 each); normals [cap][3],
 * written when cap >= *C, else nothing is and the call returns TDTK_EINVAL (normals NULL with cap 0: a count).
 * TDTK_EINVAL, in this order: NULL dims or C; type outside 0 .. 3; RhoNum, PhiNum or ThetaNum 0.  TDTK_EUNSUP: PhiNum or
 * ThetaNum >= 2^24; the (PhiNum, ThetaNum) for which the reference's constructor writes outside ballNr or leaves a slice
 * unsized -- type 1: ThetaNum < 2, or a PhiNum whose slice loop (phi += 180.0 / PhiNum while phi < 180.0) does not run
 * exactly PhiNum times; type 2: ThetaNum < 4; type 3: PhiNum < 3 (the message says which).                        */
int tdtk_hough_normals(int type, const uint32_t* dims, double* normals, size_t cap, size_t* C, int32_t* slice_sizes);
/* Accumulator*::accumulate(Point) for every point: counts[c][k] = the points with fabs(p.n_c - rho_k) < D, rho_k = (k + 0.5)
 * * RhoMax / RhoNum, the reference's expressions operation for operation (hough_lane.h) -- the reference's counts bit for bit
 * over the same table.  xyz [N][3] host memory, or NULL: the cloud the calling thread uploaded last on this device (N must be
 * its size).  normals [C][3] host memory: the table is an argument (tdtk_hough_normals gives the reference's).  counts
 * (nullable) [C][RhoNum] host memory; they also stay on the device for tdtk_hough_peaks.  Any RhoNum >= 1; N == 0 gives
 * zeros.  Checked in this order: NULL normals (TDTK_EINVAL); N >= 2^31 (TDTK_EUNSUP); C or RhoNum 0 (TDTK_EINVAL); C *
 * RhoNum >= 2^31 (TDTK_EUNSUP); xyz NULL and no resident cloud of N points (TDTK_EINVAL).  Coordinates are not checked: a
 * NaN votes nowhere, as in the reference.                                                                              */
int tdtk_hough_vote(int device, const double* xyz, size_t N, const double* normals, size_t C, uint32_t RhoNum, uint32_t RhoMax,
                    double D, int32_t* counts);
/* The head of Accumulator*::getMax()'s multiset: the entries with count > (int)(max * PlaneRatio), max the largest count
 * (Hough::SHT's loop condition, hough.cc:248-253), count descending, equal counts in that type's insertion order (rho, phi,
 * theta for types 0, 1, 3; face, i, j, rho for type 2 -- std::multiset::insert puts an equal key behind its equals).  counts
 * [C][RhoNum] host memory, or NULL: the counts of the calling thread's last tdtk_hough_vote on this device, whose C and
 * RhoNum must be this accumulator's.  *n and *max are always filled; cells [cap][4 or 5] is written when cap >= *n, else
 * nothing is and the call returns TDTK_EINVAL (tdtk_fixed_range_search's contract).  The device finds the maximum and
 * compacts the entries; their final order is made on the host.  Checked in this order: NULL dims, n or max, a NaN
 * PlaneRatio (TDTK_EINVAL); tdtk_hough_normals' checks of type and dims; C * RhoNum >= 2^31 (TDTK_EUNSUP); counts NULL
 * without a matching vote (TDTK_EINVAL).                                                                               */
int tdtk_hough_peaks(int device, const int32_t* counts, int type, const uint32_t* dims, double PlaneRatio, int32_t* cells,
                     size_t cap, uint64_t* n, int32_t* max);
/* Accumulator*::getMax(int* cell), host only: the plane { nx, ny, nz, rho } at the centre of a cell, as written for each type
 * -- not the vote's formulas (no 0.999.. factor in phi), and for type 2 the reference reads the entry as (rho, face - 1, i, j)
 * from cell[0 .. 3], which is not the layout its getMax() lists: cell[0] (the count) becomes rho's bin, cell[1] + 1 the face;
 * a face outside 1 .. 6 gives NaN normals (the reference: uninitialised memory).  cell [4] (type 2: [5]).
 * TDTK_EINVAL: NULL; a phi index outside the accumulator (types 1, 3: it selects the slice size); then
 * tdtk_hough_normals' checks of type and dims.                                                                        */
int tdtk_hough_cell_plane(int type, const uint32_t* dims, const int32_t* cell, double* plane4);
/* deletePoints' first loop (hough.cc:759-779): n is normalised first (Normalize3, on a copy), then mask[i] = fabs(p.x*n[0]
 * + p.y*n[1] + p.z*n[2] - rho) < D.  xyz as in tdtk_hough_vote.  mask (nullable) [N] bytes; *count is always filled;
 * indices [cap] the points in input order, written when cap >= *count, else they are not and the call returns TDTK_EINVAL
 * (indices NULL with cap 0 and mask given: mask and count only, TDTK_OK).  TDTK_EINVAL: NULL n or count; no cloud.
 * TDTK_EUNSUP: N >= 2^31.                                                                                             */
int tdtk_hough_plane_points(int device, const double* xyz, size_t N, const double* n, double rho, double D, uint8_t* mask,
                            int32_t* indices, size_t cap, uint64_t* count);
/* calcPlane (hough.cc:1252-1310) over the points xyz[indices[0 .. m)]: centroid, the six centred second moments about it
 * (two fp64 passes on the device, summed in a fixed order: the same bits every run, not the reference's sequential order),
 * then on the host a Jacobi eigensolver, the eigenvector of the eigenvalue smallest in absolute value, plane4[3] = n .
 * centroid and *planarity = that eigenvalue / the sum of the three.  m < 3: *planarity = 0, plane4 untouched, TDTK_OK, as
 * calcPlane returns.  TDTK_EINVAL: NULL indices (with m > 0), plane4 or planarity; no cloud; an index outside [0, N).  */
int tdtk_hough_fit_plane(int device, const double* xyz, size_t N, const int32_t* indices, size_t m, double* plane4,
                         double* planarity);
/* ms5: HIP-event times, ms, of the calling thread's last vote (kernels only), peaks, plane_points and fit_plane (kernels and
 * their small copies), and [4] how often this thread's Hough device buffers were (re)allocated so far: a second vote of the
 * same size allocates nothing.                                                                                        */
int tdtk_hough_timings(double* ms5);
/* ---- the dynamic kd-forest: BkdTree (include/slam6d/bkd.h, src/slam6d/bkd.cc), the logarithmic method over the device
 * kd-trees.  A forest is a buffer of fewer than `bucket` points and slots 0 .. S-1 (S <= 32), each empty or one kd-tree with
 * a live-point count.  Every inserted point gets an id: the running insertion counter (the reference returns pointers).  The
 * contract is the reference's stated as sets ("Dynamic kd-forest"): the layout after any sequence of calls
 * (slots, the id set of every slot, the buffer as a sequence), every returned d2, every id where the answer is unique, the
 * k-NN distance lists, the fixed-radius lists as id sets and the remove counts are the reference's; the order inside one
 * tree's contribution to a list and which of several equidistant points or identical copies inside one container is named
 * are this library's (slots ascending, the walk's visiting order, the buffer in order; the first wins a tie).  A forest's trees
 * are private to it.  Non-finite coordinates: TDTK_EINVAL, nothing changes.  A forest belongs to one host thread at a time. */
typedef struct tdtk_forest tdtk_forest;
int tdtk_forest_create(int bucket, int device, tdtk_forest** out);     /* BkdTree(b): no slots */
/* BkdTree(pts, n, b): max(1, ceil(log2(n / b))) slots (n / b an integer division), the last one a tree over all n points, ids
 * 0 .. n-1.  n == 0: TDTK_EINVAL.                                                                                     */
int tdtk_forest_create_from_points(const double* xyz, size_t n, int bucket, int device, tdtk_forest** out);
void tdtk_forest_destroy(tdtk_forest* f);
/* BkdTree::insert for the m points of xyz [m][3] in order, ids *first_id_out .. + m - 1 (nullable).  The layout is the one m
 * single inserts give; every slot of it that changed is built once (tdtk_forest_plan).                                 */
int tdtk_forest_insert(tdtk_forest* f, const double* xyz, size_t m, int32_t* first_id_out);
/* the last tdtk_forest_insert of f, ms: the plan (host clock), the gathers and the builds of the slots it built (HIP events,
 * summed over those slots), the call end to end (host clock); then the slots built and the merges they stand for.       */
int tdtk_forest_last_insert(const tdtk_forest* f, double out6[6]);
/* BkdTree::remove for the m points of xyz in order: in the lowest container (the buffer before slot 0) that holds a live point
 * with Dist2 < 1e-9 the nearest such point goes.  removed_id_out [m]: its id, or -1 where the request matches nothing.  The
 * requests of one call behave as if applied one after the other.  A tree whose count reaches 0 becomes an empty slot.   */
int tdtk_forest_remove(tdtk_forest* f, const double* xyz, size_t m, int32_t* removed_id_out);
/* counts [32] (the first *nslots written): live points per slot, 0 = empty; the buffer's fill; size(); table_mask: bit s set
 * when the tree of slot s keeps its leaves in a table.  Every output is nullable.                                       */
int tdtk_forest_info(const tdtk_forest* f, int* nslots, uint64_t* counts, uint64_t* buffer_fill, uint64_t* size, uint32_t* table_mask);
/* the live points of slot `slot` in storage order, or of the buffer (slot = -1) in insertion order: ids [cap] and xyz [cap][3]
 * (nullable each), *n their number -- written also when cap is too small, which is TDTK_EINVAL.                        */
int tdtk_forest_collect(const tdtk_forest* f, int slot, int32_t* ids, double* xyz, size_t cap, uint64_t* n);
/* BkdTree::FindClosest for K queries: every tree answers KDtree::FindClosest(p, maxdist2) (strict <), a later slot replaces the
 * result only with a strictly smaller Dist2; the buffer is then scanned against the best so far, which is DBL_MAX -- not
 * maxdist2 -- when no tree point was found (the reference's quirk, kept).  idx [K]: the id or -1; d2 [K] nullable, -1.0 then. */
int tdtk_forest_find_closest(tdtk_forest* f, const double* q, size_t K, double maxdist2, int32_t* idx, double* d2);
/* BkdTree::kNearestNeighbors: rows of k, ascending d2, -1 / -1.0 behind the live points there are; k <= 64 (TDTK_EUNSUP). */
int tdtk_forest_knn(tdtk_forest* f, const double* q, size_t K, int k, int32_t* idx, double* d2);
/* BkdTree::fixedRangeSearch under tdtk_fixed_range_search's contract (offsets [K+1] and *total always; cap < *total returns
 * TDTK_EINVAL with those filled): tree points with Dist2 < sqRad2, buffer points with Dist2 <= sqRad2 (the reference's quirk). */
int tdtk_forest_fixed_range(tdtk_forest* f, const double* q, size_t K, double sqRad2, uint64_t* offsets, int32_t* idx, double* d2,
                            size_t cap, uint64_t* total);
/* The plan of an insert, host only (no device is touched): live counts [nslots] and the buffer's fill (< bucket) before, m
 * points inserted one at a time.  counts_out [32] (the first *nslots_out written); segs [cap_segs][4] = { final slot, kind, a,
 * b } -- kind 0: the live points of old slot a (b of them), 1: the new points [a, b) in order, 2: the old buffer (b points) --,
 * *nsegs their number (cap_segs too small: TDTK_EINVAL, *nsegs set); buf_out = { 1 if the old buffer stays, a, b }: the final
 * buffer is the old one (if it stays) followed by the new points [a, b); *merges (nullable): the merges this stands for.  */
int tdtk_forest_plan(const uint64_t* counts, int nslots, uint64_t fill, int bucket, uint64_t m, int* nslots_out, uint64_t* counts_out,
                     int64_t* segs, size_t cap_segs, size_t* nsegs, uint64_t buf_out[3], uint64_t* merges);

/* ---- BOctTree<double> as a search tree (`slam6D -t 2`; include/slam6d/Boctree.h).  Built on the device from host points;
 * the node table's layout is this library's, the tree it stands for -- which cells are leaves, the order of the leaves and of
 * the points inside a leaf -- is the reference's.  An octree belongs to one host thread at a time. */
typedef struct tdtk_octree tdtk_octree;
typedef struct tdtk_octree_info {
  uint64_t n_points;        /* countPoints()                                                       Boctree.h:447  */
  uint64_t n_nodes;         /* countNodes(): inner nodes, the root included                        Boctree.h:444  */
  uint64_t n_leaves;        /* countOctLeaves()                                                    Boctree.h:446  */
  int32_t max_depth;        /* init(): 1 + halvings of the root size until it is <= voxelSize      Boctree.h:335-340 */
  int32_t largest_index;    /* child_bit_depth[0] * 2 - 1                                          Boctree.h:355  */
  double real_voxelSize, mult, add[3];   /* bit-equal to init()'s                                  Boctree.h:350-353 */
  double center[3], size;   /* the root cube (size: half edge, largest half extent + 1.0)          Boctree.h:249-255 */
  double voxel_size;
  int32_t earlystop, levels;   /* levels: depth of the deepest possible leaf, <= 21 */
  uint64_t device_bytes;
  double build_ms;
} tdtk_octree_info;
/* BOctTree<double>(pts, n, voxelSize, PointType(), earlystop) (Boctree.h:224-270; branch :1164-1195, countPointsAndQueueFast
 * :1267-1301, init :333-356) as BasicScan::createSearchTreePrivate builds it with voxelSize 10.0 and earlystop true
 * (basicScan.cc:714-719): a cell is a leaf when its size is <= voxelSize or, with earlystop, when it holds <= 10 points.
 * xyz [n][3] host memory.  Errors: n == 0, NULL xyz / out, voxel_size not > 0, non-finite coordinates (TDTK_EINVAL -- n == 0
 * is a deviation: the reference builds an empty root that no search can use); more than 21 levels (TDTK_EUNSUP, the bound of
 * tdtk_reduce_octree's 64-bit cell keys).                                                                                  */
int tdtk_octree_create(const double* xyz, size_t n, double voxel_size, int earlystop, int device, tdtk_octree** out);
/* the same over a resident scan's points (its original ones, as tdtk_tree_create_from_scan); indices are the scan's caller order */
int tdtk_octree_create_from_scan(const tdtk_scan* scan, double voxel_size, int earlystop, tdtk_octree** out);
void tdtk_octree_destroy(tdtk_octree* t);
int tdtk_octree_get_info(const tdtk_octree* t, tdtk_octree_info* info);
/* diagnostic: the tree's points in leaf order (AllPoints, Boctree.h:708-740, as indices into the caller's xyz); order [n] */
int tdtk_octree_leaf_order(const tdtk_octree* t, int32_t* order);
/* diagnostic: the node table, four 32-bit words per slot = { valid | leaf << 8, first child's slot, start, count } -- the
 * root in slot 0, then depth by depth, a depth in depth-first order; child ci of a node is slot first + popcount(valid &
 * ((1 << ci) - 1)); (start, count) is the node's run in leaf order.  *slots = n_nodes + n_leaves is always set; table
 * (nullable) [cap][4] is filled when cap >= *slots (else TDTK_EINVAL).                                                  */
int tdtk_octree_node_table(const tdtk_octree* t, uint32_t* table, size_t cap, uint64_t* slots);
/* batched BOctTree::FindClosest (Boctree.h:1573-1681; findClosestInLeaf :1361-1379) with threadNum-private state: q [K][3],
 * idx [K] the caller's index of the returned point or -1, d2 (nullable) [K] its Dist2 (maxdist2 when there is none).  This
 * is NOT the nearest point in general, and not the k-d tree's answer: a point accepted with Dist2 <= 0.0001 ends the search
 * although a nearer one may follow; at most 10 000 leaves are scanned per query, later ones are skipped; ties go to the
 * first point in octree order; the search prunes in whole voxels of real_voxelSize.
 * The reference converts (q + add) * mult and sqrt(maxdist2) * mult + 1 to int.  Where one of these values of the batch is
 * not strictly inside +-2^30 (|v| >= 2^30; a NaN included; a negative maxdist2 gives one) that conversion or the sums formed
 * from it (x +- closest_v) are undefined in C++: the call returns TDTK_EUNSUP for the whole batch and writes nothing.     */
int tdtk_octree_find_closest(const tdtk_octree* t, const double* q, size_t K, double maxdist2, int32_t* idx, double* d2);
/* the same with device pointers (d_q [K][3], d_idx [K], d_d2 [K] nullable), ordered on `stream` (NULL: the calling thread's
 * own stream, and the call returns when the results are there).  The range check needs one look at the device.         */
int tdtk_octree_find_closest_dev(const tdtk_octree* t, const double* d_q, size_t K, double maxdist2, int32_t* d_idx, double* d_d2,
                                 void* stream);
/* SearchTree::getPtPairs (searchTree.cc:92-189) over the octree: tdtk_get_pt_pairs's arguments and results, FindClosest
 * being the octree's.  pairing_mode TDTK_CLOSEST_POINT and TDTK_CLOSEST_PLANE_SIMPLE; TDTK_CLOSEST_POINT_ALONG_NORMAL_SIMPLE
 * returns TDTK_EUNSUP (BOctTree has no FindClosestAlongDir of its own, it inherits SearchTree's).  The range rule of
 * tdtk_octree_find_closest applies to the queries after their transform into the tree's frame.                          */
int tdtk_octree_get_pt_pairs(const tdtk_octree* t, const double source_alignxf[16], const double* xyz_r, const double* normal_r,
                             size_t start, size_t end, int rnd, int pairing_mode, double max_dist_match2, uint32_t want,
                             const double* lum_D /*[6] or NULL*/, int32_t* idx_out, double* p1_out, double* p2_out,
                             double* pn_out, tdtk_pair_sums* sums);

/* calculateNormalsKNN (normals.cc:442-516; calculateNormal :518-558): a KDtree(points, bucket) and, for every point, its
 * k nearest neighbours (itself included), their mean and covariance, the eigenvector of the smallest eigenvalue
 * (newmat EigenValues), oriented so that n . (p - rPos) >= 0, normalised.  normals_out [n][3] in point order (the
 * reference's OpenMP loop pushes in completion order; the single-thread order is point order, the values are the
 * same); knn_out (nullable) [n][k] the lists (-1 beyond n points).  Errors: n == 0, k < 1, bucket < 1 (TDTK_EINVAL);
 * k > 64 (TDTK_EUNSUP).                                                                                    */
int tdtk_normals_knn(const double* xyz, size_t n, int k, const double rPos[3], int bucket, int device,
                     double* normals_out, int32_t* knn_out);
/* calculateNormalsRange (normals.cc:369-439): the same PCA over every point's fixedRangeSearch list (itself included)
 * at sqRad2, in visiting order.  Errors: n == 0, bucket < 1, sqRad2 <= 0 (the reference would divide 0 by 0). */
int tdtk_normals_range(const double* xyz, size_t n, double sqRad2, const double rPos[3], int bucket, int device,
                       double* normals_out);
/* calculateNormalsKNN (normals.cc:442-516) with kNearestRangeSearch (kd.cc:137-171) in place of kNearestNeighbors: the PCA
 * of calculateNormal (normals.cc:518-558) over at most k neighbours, none at Dist2 >= sqRad2, in list order (every point's
 * list holds the point itself).  The reference has NO such estimator: the search and the PCA are its own, their
 * combination is this library's.  normals_out [n][3] in point order; knn_out (nullable) [n][k] the lists, -1 behind their
 * entries; counts_out (nullable) [n] their lengths.  A list of one or two points gives what calculateNormal gives on it.
 * Errors, in this order and before anything is launched or written: NULL xyz / rPos / normals_out, n == 0, k < 1,
 * bucket < 1 (TDTK_EINVAL); k > 64 (TDTK_EUNSUP); sqRad2 non-finite or <= 0 (TDTK_EINVAL, as tdtk_normals_range). */
int tdtk_normals_knn_range(const double* xyz, size_t n, int k, double sqRad2, const double rPos[3], int bucket, int device,
                           double* normals_out, int32_t* knn_out, int32_t* counts_out);
/* calculateNormalsAdaptiveKNN (normals.cc:563-682): a KDtree(points, bucket) (the reference's is 20) and, for every point,
 * kidx = kmin .. kmax: a fresh search for its kidx + 1 nearest neighbours, their mean, covariance and eigenvalues e1 <=
 * e2 <= e3; the loop stops at the first kidx with (e1 > 0.25 * e2) && (fabs(1.0 - e2 / e3) < 0.25), or at kmax.  The
 * normal is the eigenvector of e1 of the last list computed, oriented and normalised as above.  The whole loop runs in
 * one launch, per lane.  normals_out [n][3] in point order; k_used (nullable) [n]: the kidx of that list (kmax both when
 * kmax passed the test and when nothing did); knn_out (nullable) [n][kmax + 1]: that list, -1 behind its entries.
 * Errors, all before anything is launched or written: kmin > kmax ("kmin must not be larger than kmax", the reference's
 * std::invalid_argument), kmin < 0, n == 0, NULL xyz / rPos / normals_out, bucket < 1 (TDTK_EINVAL); kmax + 1 > 64
 * (TDTK_EUNSUP).                                                                                               */
int tdtk_normals_adaptive_knn(const double* xyz, size_t n, int kmin, int kmax, const double rPos[3], int bucket,
                              int device, double* normals_out, int32_t* k_used, int32_t* knn_out);

/* ---- SearchTree::getPtPairs, DataXYZ overload (src/slam6d/searchTree.cc:92-189), fused
 * with the per-thread Si pass of icp6D::match (icp6D.cc:170-191) and the APX/NAPX/LUM
 * pair loops.  Host buffers.  xyz_r = Target "xyz reduced" [*][3]; normal_r nullable
 * unless pairing_mode != 0 or TDTK_WANT_NAPX.  rnd > 1 draws the reference's keep-mask on the
 * host (one std::rand() per candidate in index order, i.e. serial-build semantics; SURVEY N-d)
 * and sends only the kept queries.  idx_out (nullable) [end-start]: model index per query or -1.
 * p1_out/p2_out/pn_out (nullable, [end-start][3]): compact pair list in query order, the
 * PtPair(s, t, normal) the reference pushes (for unmodified minimizers).
 * sums is overwritten (the reference accumulates into sum/centroids; callers add).     */
int tdtk_get_pt_pairs(const tdtk_tree* t, const double source_alignxf[16], const double* xyz_r,
                      const double* normal_r, size_t start, size_t end, int rnd, int pairing_mode,
                      double max_dist_match2, uint32_t want, const double* lum_D /*[6] or NULL*/,
                      int32_t* idx_out, double* p1_out, double* p2_out, double* pn_out,
                      tdtk_pair_sums* sums);

/* ---- device-resident data scan: replaces the "xyz reduced"/"normal reduced" arrays of
 * BasicScan (src/slam6d/basicScan.cc:532-668) for the duration of matching.  Points are
 * copied, spatially reordered once (results are reported in the caller's order).        */
int tdtk_scan_create(const double* xyz_reduced, const double* normal_reduced /*nullable*/, size_t N,
                     int device, tdtk_scan** out);
void tdtk_scan_destroy(tdtk_scan* s);
size_t tdtk_scan_size(const tdtk_scan* s);
/* Scan::transformReduced (src/slam6d/scan.cc:851-875): in-place transform3 of every point
 * (and transform3normal of every normal), incremental, same arithmetic.                 */
int tdtk_scan_transform(tdtk_scan* s, const double alignxf[16]);
/* copy the current points (caller's order) back, e.g. after matching */
int tdtk_scan_download(const tdtk_scan* s, double* xyz_out, double* normal_out /*nullable*/);

/* "xyz reduced original" (BasicScan::copyReducedToOriginal, src/slam6d/basicScan.cc:739-757): after
 * tdtk_scan_mark_original the points as they are now count as the original; the first call that moves the scan
 * (tdtk_scan_transform, tdtk_icp_match, the pose updates) first saves them on the device, so that
 * tdtk_tree_create_from_scan / tdtk_scan_download_original keep answering with the original.            */
int tdtk_scan_mark_original(tdtk_scan* s);
int tdtk_scan_download_original(const tdtk_scan* s, double* xyz_out);

/* Scan::getPtPairs (scan.cc:1220-1260) over a resident scan: whole-scan pass + sums. */
int tdtk_scan_pairs(const tdtk_tree* model, const double source_alignxf[16], tdtk_scan* data,
                    int pairing_mode, double max_dist_match2, uint32_t want,
                    const double* lum_D /*[6] or NULL*/, int32_t* idx_out /*host, nullable*/,
                    tdtk_pair_sums* sums);

/* icp6D::Point_Point_Error (src/slam6d/icp6D.cc:293-367): the closest-point pairs of the scan within
 * max_dist_match of the model, error = -0.39894228 * mean exp(|p1-p2|^2 * log(scale_max) / max_dist_match^2). */
int tdtk_point_point_error(const tdtk_tree* model, const double source_alignxf[16], tdtk_scan* data,
                           double max_dist_match, double scale_max, uint64_t* np_out /*nullable*/, double* error_out);

/* ---- minimizers: icp6Dminimizer::Align_Parallel with the merged sums in slot 0
 * (icp6Dquat.cc:515-634, icp6Dsvd.cc:170-280, icp6Dapx.cc:136-307, icp6Dnapx.cc:34-149),
 * serial-Align semantics (S normalised by 1/n; SVD reflection fix), and the serial-only
 * ORTHO / DUAL / HELIX / LUMEULER / LUMQUAT / QUAT_SCALE from sums filled with TDTK_WANT_MOM2.
 * alignxf is in/out: LUMEULER and LUMQUAT read the current scan's transMat from it
 * (icp6D.cc:237-241); the others ignore the input.  Returns the RMS the reference returns
 * (`ret`) through *rms.                                                                  */
int tdtk_align(int algo, const tdtk_pair_sums* sums, double alignxf[16], double* rms);

/* ---- icp6D::match (src/slam6d/icp6D.cc:104-285), device-resident loop.
 * model_dalignxf = PreviousScan->dalignxf.  data is moved in place exactly like
 * CurrentScan->transform(alignxf, ...) per iteration; data_transMat / data_dalignxf
 * (in/out) get alignxf premultiplied per iteration (Scan::transformMatrix, scan.cc:878-898).
 * trace (nullable, capacity trace_cap rows of 18 doubles): per iteration
 * {pairs, rms, alignxf[16]}.                                                             */
int tdtk_icp_match(const tdtk_tree* model, const double model_dalignxf[16], tdtk_scan* data,
                   double data_transMat[16], double data_dalignxf[16], const tdtk_icp_params* prm,
                   tdtk_icp_result* res, double* trace, int trace_cap);

/* The same loop with `-R <rnd>` (icp6D's rnd, handed to getPtPairs: "take about 1/rnd-th of the numbers only",
 * src/slam6d/searchTree.cc:116-118): per iteration one std::rand() per point of the data scan in its index order decides
 * whether the point is a candidate of that iteration (globals.icc:607-610), drawn on the host at the moment the iteration
 * starts -- the process's random stream is consumed exactly as a serial build of the reference consumes it -- and sent to
 * the device as one bit per point; every point still moves with every alignxf.  rnd <= 1: tdtk_icp_match.            */
int tdtk_icp_match_rnd(const tdtk_tree* model, const double model_dalignxf[16], tdtk_scan* data,
                       double data_transMat[16], double data_dalignxf[16], const tdtk_icp_params* prm, int rnd,
                       tdtk_icp_result* res, double* trace, int trace_cap);

/* icp6D::match on the octree search tree (`slam6D -t 2`): tdtk_icp_match's arguments, checks, messages, results and trace,
 * FindClosest being BOctTree's (tdtk_octree_find_closest: NOT the nearest point in general, so these are not the k-d
 * loop's poses).  All ten minimizers; pairing_mode TDTK_CLOSEST_POINT and TDTK_CLOSEST_PLANE_SIMPLE,
 * TDTK_CLOSEST_POINT_ALONG_NORMAL_SIMPLE returns TDTK_EUNSUP as tdtk_octree_get_pt_pairs.  An iteration is a fixed sequence
 * of launches -- the previous alignxf applied to the scan together with the queries' transform into the tree's frame and
 * their range check, the walk, the pair sums -- and one wait of the host, for the sums.  The range rule of
 * tdtk_octree_find_closest:
 *   sqrt(max_dist_match2) * mult + 1 not strictly inside +-2^30: TDTK_EUNSUP before anything moves (res untouched);
 *   a query whose voxel coordinate is not strictly inside +-2^30 in iteration k: TDTK_EUNSUP with res->iterations = k; the scan, data_transMat
 *   and data_dalignxf then hold exactly the transforms of the k iterations that completed (no query of iteration k was
 *   searched, nothing of it is applied), the other fields of res and the trace rows from k on are not meaningful.
 * The loop keeps no state of a k-d loop and leaves none: the next tdtk_icp_match on this thread starts cold.            */
int tdtk_icp_match_octree(const tdtk_octree* model, const double model_dalignxf[16], tdtk_scan* data,
                          double data_transMat[16], double data_dalignxf[16], const tdtk_icp_params* prm,
                          tdtk_icp_result* res, double* trace, int trace_cap);
/* ... with `-R <rnd>`: tdtk_icp_match_rnd's draws (one std::rand() per point, in index order, when the iteration starts) */
int tdtk_icp_match_octree_rnd(const tdtk_octree* model, const double model_dalignxf[16], tdtk_scan* data,
                              double data_transMat[16], double data_dalignxf[16], const tdtk_icp_params* prm, int rnd,
                              tdtk_icp_result* res, double* trace, int trace_cap);

/* ---- lum6DEuler::covarianceEuler (src/slam6d/lum6Deuler.cc:94-251) for one link:
 * first = model tree + its dalignxf, second = resident data scan.  C[36] row-major, CD[6].
 * Returns the pair count through *m; C/CD are zero if m <= 2 or ss < 1e-13.              */
int tdtk_lum_link(const tdtk_tree* first, const double first_dalignxf[16], tdtk_scan* second,
                  double max_dist_match2, double C[36], double CD[6], uint64_t* m, double* ss);

/* lum6DEuler::FillGB3D's link loop (src/slam6d/lum6Deuler.cc:265-303) for a batch of links on one
 * device: all correspondence passes and reductions are enqueued back to back and synchronised
 * once.  first[i] / first_dalignxf[i*16] / second[i] describe link i.  ss is evaluated from the
 * normal equations (sum|d|^2 - D.MZ, exact for the solved D) instead of a second pass over the
 * pairs; tdtk_lum_link keeps the reference's two-pass form.  Outputs are per link.          */
int tdtk_lum_links(int nlinks, const tdtk_tree* const* first, const double* first_dalignxf,
                   tdtk_scan* const* second, double max_dist_match2, double* C /*[nlinks][36]*/,
                   double* CD /*[nlinks][6]*/, uint64_t* m /*[nlinks]*/, double* ss /*[nlinks]*/);

/* Batched Scan::getPtPairs over a list of links (first[i] = model tree + dalignxf, second[i] =
 * resident data scan) with any accumulator blocks: one sync for the whole batch.  sums[nlinks]. */
int tdtk_links_pair_sums(int nlinks, const tdtk_tree* const* first, const double* first_dalignxf,
                         tdtk_scan* const* second, double max_dist_match2, uint32_t want,
                         tdtk_pair_sums* sums);

/* ---- graph-SLAM back-ends by their -G id (src/slam6d/slam6D.cc:784-804): lum6DEuler 1 (lum6Deuler.cc),
 * lum6DQuat 2 (lum6Dquat.cc), ghelix6DQ2 3 (ghelix6DQ2.cc), gapx6D 4 (gapx6D.cc).
 * tdtk_graph_link_blocks: the per-link quantities of this rank's links (covarianceEuler / covarianceQuat /
 *   genBBdForLinkedPair / genBArotForLinkedPair), tdtk_graph_block_doubles(backend) doubles per link; device
 *   passes batched, one sync.
 * tdtk_graph_solve_update: given the blocks of ALL links (after the all-reduce; zeros for links nobody could
 *   fill), the scatter in link order (FillGB3D and its counterparts), the solve, and the pose update of scans
 *   1..nscans-1: transMat / dalignxf [nscans][16], rPos / rPosTheta [nscans][3] are updated in place, resident
 *   scans (scans[i] may be NULL) are moved, xf_out [nscans][32] (nullable) receives the one or two transforms
 *   applied per scan.  state: ghelix6DQ2's B | bd ((6n)^2 + 6n doubles, zeroed once per doGraphSlam6D call),
 *   gapx6D's T | B | A (3n + (3n)^2 + 3n, likewise); NULL for the LUM back-ends.  *ret = what doGraphSlam6D's loop tests.       */
enum { TDTK_GRAPH_LUMEULER = 1, TDTK_GRAPH_LUMQUAT = 2, TDTK_GRAPH_GHELIX = 3, TDTK_GRAPH_GAPX = 4 };
int tdtk_graph_block_doubles(int backend);
int tdtk_graph_link_blocks(int backend, int nlinks, const tdtk_tree* const* first, const double* first_dalignxf,
                           tdtk_scan* const* second, double max_dist_match2, double* blocks);
int tdtk_graph_solve_update(int backend, int nlinks, const int32_t* from, const int32_t* to, const double* blocks,
                            int nscans, double* transMat, double* dalignxf, double* rPos, double* rPosTheta,
                            tdtk_scan* const* scans, double* state, double* xf_out, double* ret);

/* ---- multi-GPU: one process per GPU, links sharded, ONE all-reduce (sum, fp64) of the per-link blocks per global
 * iteration over RCCL / xGMI (the reference's unit of parallelism is the same: `omp parallel for` over
 * links in FillGB3D, lum6Deuler.cc:270-283).  RCCL is bound at run time; a single-GPU user never touches it.
 * tdtk_comm_unique_id: rank 0 draws the id (ncclGetUniqueId) and hands the 128 bytes to the other ranks by whatever
 *   the host program has (MPI, a file, torch.distributed); tdtk_comm_create: ncclCommInitRank on `device`.
 * tdtk_graph_exchange: blocks[n] <- sum over ranks, in place (host buffer; staged through the communicator's own
 *   device buffer and stream).
 * tdtk_graph_deal_links: owner[l] = rank that evaluates link l -- round-robin / (from+to) % world for scans of equal
 *   size, longest-processing-time-first by the point count of the link's second scan otherwise.
 * tdtk_graph_iteration: link blocks of this rank's links (mine[] = their indices in the link list; first / second /
 *   first_dalignxf describe them in that order) -> exchange -> tdtk_graph_solve_update, all inside the library.
 * Failure semantics with more than one rank: arguments are validated before the link passes; a rank whose link passes
 *   fail still takes part in the collective (a status slot rides behind the blocks), and then EVERY rank returns an
 *   error -- the failing rank its own code, the others TDTK_EPEER -- so nobody is left waiting in ncclAllReduce.  A
 *   failure that cannot be carried through the collective (no staging memory, a failed copy) aborts the communicator
 *   (ncclCommAbort): the peers' collective returns an error and the communicator is dead on all ranks.  The staging
 *   buffers are allocated by tdtk_comm_create.                                                                       */
#define TDTK_COMM_ID_BYTES 128
typedef struct tdtk_comm tdtk_comm;
int tdtk_comm_unique_id(char id[TDTK_COMM_ID_BYTES]);
int tdtk_comm_create(const char id[TDTK_COMM_ID_BYTES], int rank, int world, int device, tdtk_comm** out);
void tdtk_comm_destroy(tdtk_comm* c);
int tdtk_comm_info(const tdtk_comm* c, int* rank, int* world, uint64_t* n_allreduce);
int tdtk_graph_exchange(tdtk_comm* c, double* blocks, size_t n);
/* the number of ranks RCCL itself reports for the communicator (ncclCommCount); tdtk_comm_create fails unless it equals
 * the `world` it was given */
int tdtk_comm_rccl_world(const tdtk_comm* c);
int tdtk_graph_deal_links(int nlinks, const int32_t* from, const int32_t* to, const uint64_t* scan_points /*[nscans] or NULL*/,
                          int nscans, int world, int32_t* owner);
int tdtk_graph_iteration(int backend, tdtk_comm* comm /*nullable*/, int nlinks, const int32_t* from, const int32_t* to,
                         int n_mine, const int32_t* mine, const tdtk_tree* const* first, const double* first_dalignxf,
                         tdtk_scan* const* second, double max_dist_match2, int nscans, double* transMat, double* dalignxf,
                         double* rPos, double* rPosTheta, tdtk_scan* const* scans, double* state, double* xf_out, double* ret);

/* ---- ELCH loop closing (-L 1), host control flow: elch6D::graph_balancer (src/slam6d/elch6D.cc:186-279) on an
 * undirected weighted graph given as an edge list -- weights[f] = 0, weights[l] = 1, every vertex on a shortest path
 * between two junctions gets the distance-proportional value, branches inherit (weights[] entries of vertices the
 * balancer never reaches are left as they were).  tdtk_pair_sums_merge: the base block (n, sum, centroids, Si) of the
 * union of several whole-scan passes, for a MetaScan as the data scan of icp6D::match (scan.cc:1305-1327).       */
int tdtk_elch_graph_balancer(int nvertices, int nedges, const int32_t* from, const int32_t* to, const double* w,
                             int first, int last, double* weights);
int tdtk_pair_sums_merge(int count, const tdtk_pair_sums* parts, tdtk_pair_sums* out);
/* Graph::Graph(int nodes, double cldist2, int loopsize) (src/slam6d/graph.cc:107-130), the graph matchGraph6Dautomatic rebuilds
 * before every LUM round (slam6D.cc:525-532): the chain i -> i + 1, then every pair (j, k) with k - j > loopsize whose scanner
 * positions rPos [nscans][3] are closer than sqrt(cldist2), j-major.  *nlinks = the number of links; at most cap are written. */
int tdtk_graph_links(int nscans, const double* rPos, double cldist2, int loopsize, int32_t* from, int32_t* to, int cap, int* nlinks);

/* Scan::transform for many resident scans at once: scan i is moved in place by A1[i] and then by A2[i]
 * (A2 nullable), e.g. Scan::transformToEuler / transformToQuat (scan.cc:1061-1104) = M4inv(transMat) then
 * the new pose; one kernel launch for all of them.                                               */
int tdtk_scans_transform2(int count, tdtk_scan* const* scans, const double* A1 /*[count][16]*/,
                          const double* A2 /*[count][16] or NULL*/);

/* FillGB3D's scatter-add of every link's (C, CD) into the dense G (6(n-1))^2 / B 6(n-1), in link order
 * (lum6Deuler.cc:285-300), then graphSlam6D::solveSparseCholesky (graphSlam6D.cc:345-379) -> X.
 * from/to are scan numbers (0 = the fixed scan).  With links sharded over ranks, all-reduce the
 * per-link blocks (42 doubles each, zeros for links a rank does not own) and call this on every
 * rank: the result does not depend on the number of ranks.  G_out / B_out nullable.            */
int tdtk_lum_assemble_solve(int nlinks, const int32_t* from, const int32_t* to, const double* C /*[nlinks][36]*/,
                            const double* CD /*[nlinks][6]*/, int nscans, double* X /*[6(nscans-1)]*/,
                            double* G_out, double* B_out);

/* Pose update of lum6DEuler::doGraphSlam6D (lum6Deuler.cc:378-473) for scans 1..n-1:
 * result = Ha^-1 * X_i, pose -= result, Scan::transformToEuler (scan.cc:1061-1083: transform by
 * M4inv(transMat), then by EulerToMatrix4(new pose)).  transMat/dalignxf/rPos/rPosTheta are
 * [n][16]/[n][16]/[n][3]/[n][3], updated in place; scans[i] (nullable) are moved on the device;
 * xf_out (nullable, [n][32]) receives the two matrices applied to scan i so that a caller can
 * queue them for scans that are not resident.  *ret = sum |dxyz| / n  (lum6Deuler.cc:470-473). */
int tdtk_lum_update_poses(int nscans, const double* X, double* transMat, double* dalignxf,
                          double* rPos, double* rPosTheta, tdtk_scan* const* scans, double* xf_out,
                          double* ret);

/* graphSlam6D::solveSparseCholesky(GraphMatrix*, B) (src/slam6d/graphSlam6D.cc:345-379,
 * 477-503): dense SPD solve of G x = B (G row-major n x n, entries with |v| <= 1e-5
 * dropped like convertToCS does).  x may alias B.                                       */
int tdtk_solve_spd(const double* G, const double* B, int n, double* x);
/* graphSlam6D::solveSparseCholesky(const Matrix&, B) (graphSlam6D.cc:302-343) as gapx6D calls it on
 * a matrix that is not exactly symmetric: CSparse's cs_cholsol reads the UPPER triangle only.   */
int tdtk_solve_chol_upper(const double* G, const double* B, int n, double* x);
/* dense inverse (newmat `.i()`), row-major n x n */
int tdtk_invert(const double* A, int n, double* Ainv);

/* ---- octree reduction, "-r <voxelSize>" with the default centre mode: replaces
 * Scan::calcReducedPoints (src/slam6d/scan.cc:577-603, reduction_nrpts == 0) = BOctTree<double>(pts,
 * n, voxelSize) (include/slam6d/Boctree.h:222-270) + GetOctTreeCenter (:928-948).  out_xyz has room
 * for n points; *n_out = number of occupied leaf cells; centres come out in the reference's
 * depth-first child order (that order feeds the kd-tree build, so it matters).               */
int tdtk_reduce_octree(const double* xyz, size_t n, double voxel_size, int device, double* out_xyz,
                       size_t* n_out);
/* The same with `-O <nrpts>` (reduction_nrpts, scan.cc:586-596): 0 = the centres above; 1 = one random point per occupied
 * leaf (BOctTree::GetOctTreeRandom, Boctree.h:985-1018); N > 1 = up to N random points per leaf (Boctree.h:1020-1062 with
 * rm_scatter == false).  Leaves, their order and the order of the points inside a leaf (the reference's in-place
 * partitions, Boctree.h:1737-1816) come from the device; the draws are std::rand() on the host, leaf by leaf, as the
 * reference makes them (seed with std::srand; reproducible against a serial reference build).  TDTK_EUNSUP for
 * nrpts == -1 (GetOctTreeAvg sums into uninitialised memory, Boctree.h:961-964) and for rm_scatter != 0 (the reference's
 * loop walks a stale child pointer there, Boctree.h:1032-1040).  out_xyz has room for n points.                       */
int tdtk_reduce_octree_nrpts(const double* xyz, size_t n, double voxel_size, int nrpts, int rm_scatter, int device,
                             double* out_xyz, size_t* n_out);

/* ---- point normals, "-z" / "-a 10" / pairing modes 1 and 2: replaces Scan::calcNormals
 * (src/slam6d/scan.cc:398-427) = calculateNormalsApxKNN(normals, points, k, rPos, eps)
 * (src/slam6d/normals.cc:35-111; the reference calls it with k = 10, eps = 1.0).  For every point: its k
 * (1+eps)-approximate nearest neighbours exactly as the ANN 1.1.1 kd-tree (bucket size 1, sliding midpoint)
 * returns them -- the same tree is built and walked in the same order on the device --, their mean and
 * covariance, the eigenvector of the smallest eigenvalue (newmat tred2/tql2 arithmetic), flipped so that it
 * points away from rPos... i.e. n . (p - rPos) >= 0, normalised.  Lists and normals are bit-identical to the
 * library's.  normals_out [n][3]; knn_out (nullable) [n][k] neighbour indices in list order (nearest first).
 * Errors: n == 0 ("XYZ data is empty", scan.cc:408), k > n (ANN aborts: kd_search.cpp:103), k > 32,
 * non-finite coordinates.                                                                     */
int tdtk_normals_apx_knn(const double* xyz, size_t n, int k, const double rPos[3], double eps, int device,
                         double* normals_out, int32_t* knn_out);
/* calculateNormalsAdaptiveApxKNN (normals.cc:116-213): the adaptive loop of tdtk_normals_adaptive_knn around
 * annkSearch(p, kidx + 1, eps) on the ANN tree above, each search started afresh (the list for k is no prefix of the
 * list for k + 1 under the (1+eps) bound).  Outputs as tdtk_normals_adaptive_knn.  Errors, all before anything is launched
 * or written: kmin > kmax, kmin < 0, n == 0, NULLs, eps < 0 or not finite, non-finite coordinates (TDTK_EINVAL); kmax + 1 > n
 * ("Requesting more near neighbors than data points", TDTK_EINVAL -- a deviation: ANN aborts the process only when some
 * point actually reaches such a kidx, this refuses the call); kmax + 1 > 32 (TDTK_EUNSUP).                       */
int tdtk_normals_adaptive_apx_knn(const double* xyz, size_t n, int kmin, int kmax, const double rPos[3], double eps,
                                  int device, double* normals_out, int32_t* k_used, int32_t* knn_out);
/* the same for a resident scan, from its current points; the result becomes its "normal reduced" */
int tdtk_scan_calc_normals(tdtk_scan* s, int k, const double rPos[3], double eps);

/* ---- instrumentation: per-kernel device time of the last call on this thread (ms) and
 * traversal counters of the last counting run.                                          */
/* HIP events around the search and pair-sum kernels of every pass: a profiling aid, off by default (process-wide;
 * also TDTK_KERNEL_TIMING=1 in the environment) because the events themselves cost ~10 us per ICP iteration.  While
 * it is off tdtk_icp_result.nn_ms / sums_ms, tdtk_last_kernel_ms and out[0], out[1] of tdtk_last_timings are 0.
 * Returns the previous setting.  (The reference has nothing of the kind: icp6D::match prints its wall time only,
 * icp6D.cc:279-283 -- tdtk_icp_result.total_ms.) */
/* Deferred scan moves.  The batched pose update of a graph-SLAM round (tdtk_graph_solve_update / tdtk_graph_iteration,
 * tdtk_scans_transform2, tdtk_lum_update_poses) returns while the move of the resident scans is still running on the device; a
 * process-wide fence makes the next library call of ANY host thread on that device wait for it before it touches a scan
 * or a tree (every entry point that takes a tree / scan / device argument, including the destroy and mark_original
 * calls).  The read-outs in this section (tdtk_kernel_timing, tdtk_last_kernel_ms, tdtk_last_timings, the visit
 * counters) deliberately do NOT wait -- they touch no scan and must not end the overlap.  TDTK_SYNC_MOVES=1 in the
 * environment restores "the scans have moved when the call returns". */
int tdtk_kernel_timing(int on);
int tdtk_last_kernel_ms(double* nn_ms);
/* out[0] = search kernel, out[1] = pair-sum kernels of the last pass on this thread, out[2] = the k-NN + PCA kernel
 * of the last calcNormals (HIP events on the stream the kernels were launched on), out[3] = wall time of the last
 * device tree build (a chain of ~40 launches) */
int tdtk_last_timings(double out[4]);
/* on != 0: every FindClosest pass of the calling thread on `device` runs the instrumented instantiation of the
 * kernel it would have used (identical traversal and results, slower) and adds to four counters, zeroed here;
 * tdtk_visit_counters reads {internal nodes, buckets, bucket points visited, queries issued} -- the exact
 * n_int / n_pts of SURVEY 8(d)'s algorithmic bytes for exactly the launches that ran (warm radius included) --
 * and, for calcNormals, out[4..6] = {ANN splitting nodes, leaf points visited, points processed}; out[7] = queries of
 * repeated passes that were searched a second time with every quick check (a warm query walks without the quick check of
 * its divergent visits and is searched again, cold, if it accepted a point that improved closest_d2 by a rounding's
 * worth: DESIGN.md section 4, "the quick check deferred").
 * on == 2: while counting, every search also starts cold (no warm start, no deferred quick check): the counters then hold
 * the walk of the reference's _FindClosest (kdTreeImpl.h:345-383) over the same queries -- SURVEY 8(d)'s n_int / n_pts,
 * "properties of (tree, query, maxdist2), independent of implementation"; the results, and so a loop's path, are unchanged.
 * With on == 1 the counters are the launches' OWN walk, which does depend on the implementation: from the third pass of a
 * tdtk_icp_match loop on, queries answered by their certificate (tdtk_skip_counters) are counted in out[3] but visit nothing. */
int tdtk_visit_counting(int device, int on);
int tdtk_visit_counters(int device, uint64_t out[8]);
/* the instrumented passes of tdtk_icp_match since tdtk_visit_counting(device, on): queries of repeated passes answered by their
 * certificate -- the previous hit provably stays nearest (out[0]), or there provably is still none (out[1]): DESIGN.md section 4,
 * "a certificate per query" --, queries handed to a lane and walked (out[2]), second searches (out[3] = tdtk_visit_counters' out[7]) */
int tdtk_skip_counters(int device, uint64_t out[4]);
/* measured roofline denominators: kind 0 = HBM stream copy over `bytes` (read + written per pass), kind 1 =
 * repeated reads of an L2-resident buffer (bytes <= 16 MB); best of `reps` passes in GB/s */
int tdtk_measure_bandwidth(int device, int kind, size_t bytes, int reps, double* gbs);
int tdtk_count_visits(const tdtk_tree* t, const double* q, size_t K, double maxdist2,
                      uint64_t counters[3] /* internal nodes, leaves, leaf points */);
/* Correspondence hashes of the resident loop (off by default, process-wide; returns the previous setting): while on,
 * every iteration of tdtk_icp_match also reduces its correspondences to one word on the device -- the XOR over the found
 * queries of (model index * 1315423911 + query index), both in the caller's numbering, i.e. the hash of the index array
 * SearchTree::getPtPairs' loop walks (searchTree.cc:118-147) -- so that a test can compare the loop's INDICES with the
 * reference's iteration by iteration at a million points without downloading them.  tdtk_icp_index_hashes returns the
 * previous setting; a negative argument only asks.  tdtk_icp_last_hashes: the words of the calling thread's last
 * tdtk_icp_match, on whatever device it ran (*n_out = how many passes it ran, at most 1024 are kept; 0 while switched off). */
int tdtk_icp_index_hashes(int on);
int tdtk_icp_last_hashes(uint64_t* out, int cap, int* n_out);

/* ---- on-disk formats either side of the path (host only): uos ASCII scans with the -m/-M range
 * filter (src/scanio/helper.cc:564-880, src/slam6d/pointfilter.cc:162-188), .pose files
 * (helper.cc:192-234) and .frames files (src/slam6d/basicScan.cc:902-917).                  */
int tdtk_io_read_uos(const char* path, double range_max, double range_min, double** xyz_out,
                     size_t* n_out);
void tdtk_io_free(void* p);
int tdtk_io_read_pose(const char* path, double rPos[3], double rPosTheta[3]);
int tdtk_io_write_frames(const char* path, const double* transMats, const int* types, size_t count,
                         int append);

/* ---- host-only diagnostics (no device needed; used by the CPU test tier) ----------------
 * tdtk_host_tree_layout: run the host tree builder only.  perm_out [M] = caller indices in
 * leaf order (== the reference's post-build pointer order); stats = {internal nodes, leaves,
 * max depth, max leaf points}.  tdtk_host_m4inv / tdtk_host_mmult: the bit-exact M4inv /
 * MMult (globals.icc:762-785, 298-328) used for every query transform.                      */
int tdtk_host_tree_layout(const double* xyz, size_t M, int bucket_size, int32_t* perm_out,
                          uint64_t stats[4]);
/* tdtk_host_tree_levels: the level profile of the host builder's tree.  nseg[d] = nodes (internal and buckets) at depth
 * d (the root: 0), maxn[d] = points of the largest of them, for d < cap; *levels = levels the tree has (may exceed cap). */
int tdtk_host_tree_levels(const double* xyz, size_t M, int bucket_size, int cap, uint32_t* nseg, uint32_t* maxn,
                          int* levels);
int tdtk_host_m4inv(const double in[16], double out[16]);
void tdtk_host_mmult(const double a[16], const double b[16], double out[16]);
/* the pose conversions the pose updates use: EulerToMatrix4 / Matrix4ToEuler (globals.icc:501-576),
 * QuatToMatrix4 / Matrix4ToQuat (globals.icc:988-1075) */
void tdtk_host_euler_to_matrix4(const double rPos[3], const double rPosTheta[3], double out[16]);
void tdtk_host_matrix4_to_euler(const double in[16], double rPosTheta[3], double rPos[3]);
void tdtk_host_quat_to_matrix4(const double quat[4], const double t[3], double out[16]);
void tdtk_host_matrix4_to_quat(const double in[16], double quat[4], double t[3]);

#ifdef __cplusplus
}
#endif
#endif /* TDTK_HIP_H */
