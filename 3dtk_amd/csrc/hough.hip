// The standard 3D Hough transform (Hough::SHT, src/shapes/hough.cc:222-265) on the device: every point votes for every cell
// of the accumulator.  The per-lane predicates are hough_lane.h; here are the kernels around them.
//
//   vote          A workgroup owns a tile of cells x rho bins of the accumulator in LDS (at most HOUGH_TILE_INTS counters,
//                 32 KiB: five workgroups per CU).  It streams ALL points through, one point per lane and trip -- 24
//                 contiguous bytes per lane, the whole cloud re-served by L2 to every workgroup after the first -- and every
//                 lane walks the tile's cells: one three-term dot product against the cell's normal (read from LDS, the same
//                 address in every lane: a broadcast), the window of bins around it (a handful), the reference's predicate
//                 per bin against rho_k from a table (k_hough_rho, RhoNum doubles, L1-resident), an LDS atomic add per
//                 vote.  At the end the tile is written once, with plain stores.  No global atomic anywhere; the counts are
//                 integers, so the order of the adds does not matter.
//                 A histogram with more bins than the tile holds is tiled over rho (cells per tile = 1): a lane then skips
//                 the part of its window outside the tile's bins.
//   max / peaks   the largest counter; the counters above a threshold, compacted (one atomic per wave) into (count, linear
//                 index) records in arrival order -- the host sorts them into the reference's multiset order
//   plane points  |p.n - rho| < D per point: byte mask and 32-bit flags, an exclusive scan (launch_scan_u32), a fill: the
//                 indices in input order
//   moments       calcPlane's two loops (hough.cc:1263-1281) over an index list: per workgroup partial sums in a fixed
//                 order (lane-strided, then a tree in LDS), added up by the host in block order -- the same result every run
#include <hip/hip_runtime.h>

#include "hough.h"
#include "hough_lane.h"

namespace tdtk {

void hough_tile(uint32_t rho_num, uint32_t& cells, uint32_t& bins)
{
  bins = rho_num < HOUGH_TILE_INTS ? rho_num : HOUGH_TILE_INTS;
  if (bins == 0) bins = 1;
  cells = HOUGH_TILE_INTS / bins;
  if (cells > HOUGH_TILE_CELLS) cells = HOUGH_TILE_CELLS;
}

// dynamic LDS: tile_cells normals, then tile_cells * tile_bins counters
__global__ void __launch_bounds__(HOUGH_BLOCK) k_hough_vote(const double* __restrict__ xyz, const uint32_t n,
                                                            const double* __restrict__ normals, const uint32_t C,
                                                            const uint32_t rho_num, const double* __restrict__ rho_tab,
                                                            const double inv_bin, const double D, const uint32_t tile_cells,
                                                            const uint32_t tile_bins, const uint32_t rho_tiles,
                                                            int32_t* __restrict__ counts)
{
  extern __shared__ double s_raw[];
  double* s_n = s_raw;                                               // [tile_cells][3]
  int* s_hist = reinterpret_cast<int*>(s_raw + 3 * tile_cells);      // [tile_cells][tile_bins]
  const uint32_t ct = blockIdx.x / rho_tiles, rt = blockIdx.x - ct * rho_tiles;
  const uint32_t c0 = ct * tile_cells, k0 = rt * tile_bins;
  const uint32_t nc = min(tile_cells, C - c0), nb = min(tile_bins, rho_num - k0);
  const double rho_num_d = (double)rho_num;
  for (uint32_t i = threadIdx.x; i < 3 * nc; i += HOUGH_BLOCK) s_n[i] = normals[3 * (size_t)c0 + i];
  for (uint32_t i = threadIdx.x; i < nc * tile_bins; i += HOUGH_BLOCK) s_hist[i] = 0;
  __syncthreads();
  for (uint32_t p = threadIdx.x; p < n; p += HOUGH_BLOCK) {
    const double px = xyz[3 * (size_t)p], py = xyz[3 * (size_t)p + 1], pz = xyz[3 * (size_t)p + 2];
    for (uint32_t c = 0; c < nc; ++c) {
      const double d = hough_distance(px, py, pz, s_n[3 * c], s_n[3 * c + 1], s_n[3 * c + 2]);
      uint32_t lo, hi;
      hough_window(d, inv_bin, rho_num_d, D, lo, hi);
      lo = max(lo, k0);
      hi = min(hi, k0 + nb);
      for (uint32_t k = lo; k < hi; ++k)
        if (hough_votes(d, rho_tab[k], D)) atomicAdd(&s_hist[c * tile_bins + (k - k0)], 1);
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < nc * nb; i += HOUGH_BLOCK) {
    const uint32_t c = i / nb, k = i - c * nb;
    counts[(size_t)(c0 + c) * rho_num + k0 + k] = s_hist[c * tile_bins + k];
  }
}

__global__ void __launch_bounds__(HOUGH_BLOCK) k_hough_rho(const uint32_t rho_num, const double rho_max_d, double* __restrict__ rho_tab)
{
  const size_t k = (size_t)blockIdx.x * HOUGH_BLOCK + threadIdx.x;
  if (k < rho_num) rho_tab[k] = hough_rho((uint32_t)k, rho_max_d, (double)rho_num);
}

hipError_t launch_hough_vote(const double* xyz, uint32_t n, const double* normals, uint32_t C, uint32_t rho_num, uint32_t rho_max,
                             double D, double* rho_tab, int32_t* counts, hipStream_t s)
{
  if (!C || !rho_num) return hipSuccess;
  hipLaunchKernelGGL(k_hough_rho, dim3((rho_num + HOUGH_BLOCK - 1) / HOUGH_BLOCK), dim3(HOUGH_BLOCK), 0, s, rho_num, (double)rho_max,
                     rho_tab);
  uint32_t tc, tb;
  hough_tile(rho_num, tc, tb);
  const uint32_t cell_tiles = (C + tc - 1) / tc, rho_tiles = (rho_num + tb - 1) / tb;
  const size_t lds = (size_t)tc * 3 * sizeof(double) + (size_t)tc * tb * sizeof(int);
  hipLaunchKernelGGL(k_hough_vote, dim3(cell_tiles * rho_tiles), dim3(HOUGH_BLOCK), lds, s, xyz, n, normals, C, rho_num, rho_tab,
                     (double)rho_num / (double)rho_max, D, tc, tb, rho_tiles, counts);
  return hipGetLastError();
}

__global__ void __launch_bounds__(HOUGH_BLOCK) k_hough_max(const int32_t* __restrict__ counts, const size_t total,
                                                           int32_t* __restrict__ max_out)
{
  int32_t m = 0;
  const size_t stride = (size_t)gridDim.x * HOUGH_BLOCK;
  for (size_t i = (size_t)blockIdx.x * HOUGH_BLOCK + threadIdx.x; i < total; i += stride) m = max(m, counts[i]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off, 64));
  if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(max_out, m);
}

hipError_t launch_hough_max(const int32_t* counts, size_t total, int32_t* max_out, hipStream_t s)
{
  if (!total) return hipSuccess;
  const size_t want = (total + HOUGH_BLOCK - 1) / HOUGH_BLOCK;
  hipLaunchKernelGGL(k_hough_max, dim3((uint32_t)(want < 2048 ? want : 2048)), dim3(HOUGH_BLOCK), 0, s, counts, total, max_out);
  return hipGetLastError();
}

__global__ void __launch_bounds__(HOUGH_BLOCK) k_hough_peaks(const int32_t* __restrict__ counts, const size_t total,
                                                             const int32_t threshold, int32_t* __restrict__ records,
                                                             const uint32_t cap, uint32_t* __restrict__ n_out)
{
  const size_t stride = (size_t)gridDim.x * HOUGH_BLOCK;
  const uint32_t lane = threadIdx.x & 63u;
  // whole waves go round together: the ballot below needs every lane of the wave in the same trip
  const size_t trips = (total + stride - 1) / stride;
  size_t i = (size_t)blockIdx.x * HOUGH_BLOCK + threadIdx.x;
  for (size_t t = 0; t < trips; ++t, i += stride) {
    const int32_t v = (i < total) ? counts[i] : 0;
    const bool hit = (i < total) && v > threshold;
    const unsigned long long m = __ballot(hit);
    if (!m) continue;
    const int leader = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if ((int)lane == leader) base = atomicAdd(n_out, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, leader, 64);
    if (hit) {
      const uint32_t slot = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      if (slot < cap) { records[2 * (size_t)slot] = v; records[2 * (size_t)slot + 1] = (int32_t)(uint32_t)i; }
    }
  }
}

hipError_t launch_hough_peaks(const int32_t* counts, size_t total, int32_t threshold, int32_t* records, uint32_t cap, uint32_t* n_out,
                              hipStream_t s)
{
  if (!total) return hipSuccess;
  const size_t want = (total + HOUGH_BLOCK - 1) / HOUGH_BLOCK;
  hipLaunchKernelGGL(k_hough_peaks, dim3((uint32_t)(want < 2048 ? want : 2048)), dim3(HOUGH_BLOCK), 0, s, counts, total, threshold,
                     records, cap, n_out);
  return hipGetLastError();
}

__global__ void __launch_bounds__(HOUGH_BLOCK) k_hough_plane_points(const double* __restrict__ xyz, const uint32_t n, const double nx,
                                                                    const double ny, const double nz, const double rho,
                                                                    const double D, uint8_t* __restrict__ mask,
                                                                    uint32_t* __restrict__ flags)
{
  const size_t i = (size_t)blockIdx.x * HOUGH_BLOCK + threadIdx.x;
  if (i > n) return;
  uint32_t f = 0;
  if (i < n) {
    f = hough_on_plane(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], nx, ny, nz, rho, D) ? 1u : 0u;
    mask[i] = (uint8_t)f;
  }
  flags[i] = f;          // flags[n] = 0: the scan's last entry is the count
}

hipError_t launch_hough_plane_mask(const double* xyz, uint32_t n, const double nrm[3], double rho, double D, uint8_t* mask,
                                   uint32_t* flags, hipStream_t s)
{
  const uint32_t grid = (uint32_t)(((size_t)n + 1 + HOUGH_BLOCK - 1) / HOUGH_BLOCK);
  hipLaunchKernelGGL(k_hough_plane_points, dim3(grid), dim3(HOUGH_BLOCK), 0, s, xyz, n, nrm[0], nrm[1], nrm[2], rho, D, mask, flags);
  return hipGetLastError();
}

__global__ void __launch_bounds__(HOUGH_BLOCK) k_hough_plane_fill(const uint32_t* __restrict__ flags,
                                                                  const uint32_t* __restrict__ offsets, const uint32_t n,
                                                                  int32_t* __restrict__ indices)
{
  const size_t i = (size_t)blockIdx.x * HOUGH_BLOCK + threadIdx.x;
  if (i < n && flags[i]) indices[offsets[i]] = (int32_t)i;
}

hipError_t launch_hough_plane_fill(const uint32_t* flags, const uint32_t* offsets, uint32_t n, int32_t* indices, hipStream_t s)
{
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_hough_plane_fill, dim3((n + HOUGH_BLOCK - 1) / HOUGH_BLOCK), dim3(HOUGH_BLOCK), 0, s, flags, offsets, n, indices);
  return hipGetLastError();
}

// every workgroup writes its row of `partial`, also when it owns no point (zeros)
__global__ void __launch_bounds__(HOUGH_BLOCK) k_hough_moments(const double* __restrict__ xyz, const int32_t* __restrict__ idx,
                                                               const uint32_t m, const int pass, const double cx, const double cy,
                                                               const double cz, double* __restrict__ partial)
{
  __shared__ double s_sum[6][HOUGH_BLOCK];
  double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const size_t stride = (size_t)gridDim.x * HOUGH_BLOCK;
  for (size_t j = (size_t)blockIdx.x * HOUGH_BLOCK + threadIdx.x; j < m; j += stride) {
    const size_t i = (size_t)idx[j];
    const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    if (pass == 0) {
      a[0] += x; a[1] += y; a[2] += z;
    } else {
      a[0] += (x - cx) * (x - cx);
      a[1] += (y - cy) * (y - cy);
      a[2] += (z - cz) * (z - cz);
      a[3] += (x - cx) * (y - cy);
      a[4] += (x - cx) * (z - cz);
      a[5] += (y - cy) * (z - cz);
    }
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) s_sum[q][threadIdx.x] = a[q];
  __syncthreads();
  for (uint32_t w = HOUGH_BLOCK / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w)
#pragma unroll
      for (int q = 0; q < 6; ++q) s_sum[q][threadIdx.x] += s_sum[q][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x < 6) partial[6 * (size_t)blockIdx.x + threadIdx.x] = s_sum[threadIdx.x][0];
}

hipError_t launch_hough_moments(const double* xyz, const int32_t* idx, uint32_t m, int pass, const double centroid[3], double* partial,
                                hipStream_t s)
{
  hipLaunchKernelGGL(k_hough_moments, dim3(HOUGH_MOMENT_BLOCKS), dim3(HOUGH_BLOCK), 0, s, xyz, idx, m, pass, centroid[0], centroid[1],
                     centroid[2], partial);
  return hipGetLastError();
}

}  // namespace tdtk
