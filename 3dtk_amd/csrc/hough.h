// Launchers of hough.hip (the standard 3D Hough transform of src/shapes: vote, peaks, plane points, plane moments) ; the
// host-only geometry of the reference's four accumulators is hough_geom.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "hough_geom.h"

namespace tdtk {

constexpr uint32_t HOUGH_TILE_INTS = 8192;      // counters of one workgroup's tile in LDS: 32 KiB
constexpr uint32_t HOUGH_TILE_CELLS = 32;       // at most this many cells per tile
constexpr int HOUGH_BLOCK = 256;
constexpr uint32_t HOUGH_MOMENT_BLOCKS = 256;   // partial sums of k_hough_moments: [HOUGH_MOMENT_BLOCKS][6]

// the tile of k_hough_vote for a histogram of rho_num bins per cell: cells x bins, cells * bins <= HOUGH_TILE_INTS
void hough_tile(uint32_t rho_num, uint32_t& cells, uint32_t& bins);

// counts [C][rho_num] int32, every entry written (no memset needed); rho_tab [rho_num] scratch: the bins' rho values
hipError_t launch_hough_vote(const double* xyz, uint32_t n, const double* normals, uint32_t C, uint32_t rho_num, uint32_t rho_max,
                             double D, double* rho_tab, int32_t* counts, hipStream_t s);
// *max_out = max(*max_out, every count): the caller zeroes it
hipError_t launch_hough_max(const int32_t* counts, size_t total, int32_t* max_out, hipStream_t s);
// records (count, linear index) of the entries with count > threshold, in no particular order; *n_out += their number (the
// caller zeroes it); only the first `cap` that arrive are written (records may be null with cap 0: a count)
hipError_t launch_hough_peaks(const int32_t* counts, size_t total, int32_t threshold, int32_t* records, uint32_t cap, uint32_t* n_out,
                              hipStream_t s);
// mask [n] bytes and flags [n + 1] (the last 0) of the points with |p.n - rho| < D
hipError_t launch_hough_plane_mask(const double* xyz, uint32_t n, const double nrm[3], double rho, double D, uint8_t* mask,
                                   uint32_t* flags, hipStream_t s);
// indices [offsets[n]] of the flagged points in input order, offsets the exclusive scan of flags
hipError_t launch_hough_plane_fill(const uint32_t* flags, const uint32_t* offsets, uint32_t n, int32_t* indices, hipStream_t s);
// partial [HOUGH_MOMENT_BLOCKS][6]: per workgroup, pass 0 the sums of x, y, z (and three zeros), pass 1 the sums of
// (x-cx)^2, (y-cy)^2, (z-cz)^2, (x-cx)(y-cy), (x-cx)(z-cz), (y-cy)(z-cz) over idx [m]; added up in block order by the caller
hipError_t launch_hough_moments(const double* xyz, const int32_t* idx, uint32_t m, int pass, const double centroid[3], double* partial,
                                hipStream_t s);

}  // namespace tdtk
