// Argument block and launchers of voxel.hip: the device voxel grid of tdtk_voxel_walk and tdtk_peopleremover.
#pragma once
#include <hip/hip_runtime.h>

#include "voxel_lane.h"

namespace tdtk {

struct VoxArgs {
  // input
  const double* xyz;         // [n][3] points, global frame
  const double* ends;        // [n][3] ray ends, or null: the points
  const double* origins;     // [S][3] scanner positions
  const uint32_t* scan_off;  // [S + 1]
  uint32_t n, S;
  double vs;
  uint64_t diff;
  uint32_t cluster_size;
  int subvoxel;
  // per point
  uint64_t* keys;            // [n] caller order;  keys_s [n] sorted
  uint32_t* scans;           // [n] caller order;  scans_s [n] sorted (stable: ascending inside a key)
  uint64_t* keys_s;
  uint32_t* scans_s;
  uint32_t *fp, *fv, *fb;    // [n + 1] head flags of pairs / voxels / bricks;  ip, iv, ib: their exclusive scans
  uint32_t *ip, *iv, *ib;
  // compact
  uint32_t* pscan;           // [pairs]
  uint32_t* vstart;          // [voxels + 1]
  uint64_t* vkey;            // [voxels]
  uint64_t* bkey;            // [bricks]
  uint32_t* bbase;           // [bricks + 1]
  VoxBrick* table;
  uint32_t mask;
  uint32_t n_pairs, n_vox, n_bricks;
  unsigned char* free_mark;  // [voxels]
  unsigned char* pdyn;       // [pairs]
  uint32_t *parent, *csize;  // [voxels]
  unsigned char* dynamic;    // [n]
  // counters: [0] error bits, [1] visits, [2] freed, [3] free after clustering, [4] half-free
  unsigned long long* ctr;
};

size_t vox_sort_temp_bytes(size_t n);
hipError_t launch_vox_keys(const VoxArgs& a, hipStream_t s);                    // keys, scans; ctr[0]
hipError_t launch_vox_sort_flags(const VoxArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s);   // keys_s, scans_s, f*, i*
hipError_t launch_vox_compact(const VoxArgs& a, hipStream_t s);                 // pscan, vstart, vkey, bkey, bbase
hipError_t launch_vox_table(const VoxArgs& a, hipStream_t s);                   // table (set to VOX_EMPTY by the caller)
hipError_t launch_vox_carve(const VoxArgs& a, hipStream_t s);                   // free_mark (zeroed by the caller); ctr[1]
hipError_t launch_vox_cluster_filter(const VoxArgs& a, hipStream_t s);          // free_mark without the small components
hipError_t launch_vox_classify(const VoxArgs& a, hipStream_t s);                // pdyn, dynamic; ctr[4]

// tdtk_voxel_walk: counts [m + 1] (the last 0), then lists at the exclusive scan of the counts
hipError_t launch_vox_walk_check(const double* starts, const double* ends, size_t m, double vs, unsigned long long* ctr,
                                 hipStream_t s);
hipError_t launch_vox_walk_count(const double* starts, const double* ends, size_t m, double vs, uint32_t* counts,
                                 unsigned long long* ctr, hipStream_t s);       // ctr[1] += visits
hipError_t launch_vox_walk_fill(const double* starts, const double* ends, size_t m, double vs, const uint32_t* offsets,
                                int32_t* voxels, hipStream_t s);

}  // namespace tdtk
