// The per-lane code of the 3D Hough transform (tdtk_hough_vote, tdtk_hough_plane_points; kernels in hough.hip): the two
// point-to-plane predicates of the reference's src/shapes, operation for operation.  Like voxel_lane.h a host compiler reads
// this file (the test's shim defines __device__ / __forceinline__ away): tests/test_hough_host.py runs it that way.
//
// The vote.  Accumulator*::accumulate(Point) (accumulator.cc:123-154, 451-475, 1252-1275, 1564-1598) tests every rho bin k
// of every cell with
//     rho      = (k + 0.5) * RhoMax / RhoNum          RhoMax, RhoNum unsigned ints converted to double, left to right
//     distance = p.x * n[0] + p.y * n[1] + p.z * n[2]  left to right, no contraction
//     vote     = fabs(distance - rho) < MaxPointPlaneDist
// hough_rho and hough_votes are that predicate and nothing else (k_hough_rho tabulates rho once per vote: RhoNum divisions
// instead of one per point, cell and bin -- the same correctly rounded quotient).  hough_window bounds the bins a lane has to try -- computed from the
// distance in floating point and padded by one bin on each side, so its own roundings (a few ulp of a bin index below 2^31)
// cannot cut a voting bin off; whether a bin inside it votes is decided by hough_votes alone.
//
// deletePoints' first loop (hough.cc:769-779) subtracts rho inside the sum -- p.x*n[0] + p.y*n[1] + p.z*n[2] - rho, then
// fabs(..) < MaxPointPlaneDist: the same four roundings in the same order as the vote's, but kept as a function of its own,
// as the reference keeps it as an expression of its own.
#pragma once
#include <cmath>
#include <cstdint>

namespace tdtk {

__device__ __forceinline__ double hough_distance(const double px, const double py, const double pz, const double nx,
                                                 const double ny, const double nz)
{
  return px * nx + py * ny + pz * nz;
}

// rho_max_d, rho_num_d: (double)RhoMax, (double)RhoNum
__device__ __forceinline__ double hough_rho(const uint32_t k, const double rho_max_d, const double rho_num_d)
{
  return ((double)k + 0.5) * rho_max_d / rho_num_d;
}

__device__ __forceinline__ bool hough_votes(const double distance, const double rho_k, const double D)
{
  return fabs(distance - rho_k) < D;
}

// The bins [lo, hi) of [0, RhoNum) that can vote for `distance`: k votes only if (distance - D) / bin - 0.5 < k <
// (distance + D) / bin - 0.5 in exact arithmetic; floor of the left side and ceil of the right are each one bin outside.
// inv_bin = (double)RhoNum / (double)RhoMax: a product instead of the quotient, a few more ulp, far inside the padding.
// Everything is clamped as a double first, so no conversion overflows; fmax / fmin drop a NaN operand, so a NaN bound
// becomes 0 -- an empty or a too wide window, and hough_votes refuses every bin of it, as the reference's comparison does.
// RhoMax == 0 (inv_bin infinite: every rho_k is 0): the whole range.
__device__ __forceinline__ void hough_window(const double distance, const double inv_bin, const double rho_num_d, const double D,
                                             uint32_t& lo, uint32_t& hi)
{
  double a = floor((distance - D) * inv_bin - 0.5), b = ceil((distance + D) * inv_bin - 0.5) + 1.0;
  if (!(inv_bin <= 1.7976931348623157e308)) { a = 0.0; b = rho_num_d; }
  a = fmin(fmax(a, 0.0), rho_num_d);
  b = fmin(fmax(b, 0.0), rho_num_d);
  lo = (uint32_t)a;
  hi = (uint32_t)b;
}

// hough.cc:772-773
__device__ __forceinline__ bool hough_on_plane(const double px, const double py, const double pz, const double nx, const double ny,
                                               const double nz, const double rho, const double D)
{
  const double distance = px * nx + py * ny + pz * nz - rho;
  return fabs(distance) < D;
}

}  // namespace tdtk
