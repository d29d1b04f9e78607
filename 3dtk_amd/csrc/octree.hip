// The reference's BOctTree<double> as a device search tree (`slam6D -t 2`): the node table and the FindClosest kernel.
//
// The tree.  BOctTree<double>(pts, n, voxelSize, PointType(), earlystop) (include/slam6d/Boctree.h:224-270) splits a cell into
// its occupied octants until `_size <= voxelSize || (earlystop && n <= 10)` (branch, :1164-1195), so with earlystop its leaves
// sit at any depth.  reduce.hip already gives the full-depth cell key of every point (k_oct_keys: the root cube, the `>=` cuts
// of the array constructor), the sorted keys and the order the in-place z / y / x partitions leave inside a leaf
// (launch_oct_leaf_order).  What this file adds:
//   k_oct_leaf_depth   the depth of every point's leaf.  A node of depth L is the run of equal L-digit key prefixes in the sorted
//                      keys; a run that holds sorted position i has at most 10 points exactly when at most 10 of the 21
//                      positions i - 10 .. i + 10 share the prefix (a longer run around i would fill more of that window).
//                      The leaf is the first depth >= 1 where that holds, or the full depth.  The same kernel counts the
//                      nodes of every depth and the leaves.
//   k_oct_mask_*       clear the key digits below the leaf.  The partition passes of reduce.hip then find nothing to move
//                      below an early leaf: its points keep the order the passes down to its depth left, as in the reference.
//                      The cleared keys are still sorted (a leaf's keys collapse to the smallest value of their own range).
//   per level L        k_oct_level_flags (where a node of depth L starts), one scan, k_oct_level_emit: the node's slot is
//                      base[L] + rank, its run comes from a binary search of the prefix's end, and it reports itself to its
//                      parent -- an atomicOr of its valid / leaf bit, and the parent's first child stores its own slot.
//   k_oct_points       the KdPoint array in leaf order.
//
// The search.  k_oct_find: one lane per query, the batch in the spatial order launch_bin gives, the walk of oct_lane.h with
// its per-level stack in LDS ([level][lane], 8-byte entries: a wave's accesses to one level are 512 consecutive bytes).  All
// decisions are integer voxel arithmetic; fp64 only for (p + add) * mult, Dist2 and sqrt(d2) * mult + 1, FMA contraction off
// (Makefile), in the reference's association.
//
// The ICP loop.  k_oct_loop_prepare / k_oct_loop_find: the same two passes in the form tdtk_icp_match_octree launches once per
// iteration without looking at the device in between -- the scan's move by the previous alignxf folded into the prepare pass,
// the range word read by the walk itself.
#include <hip/hip_runtime.h>

#include "octree.h"

namespace tdtk {

static inline uint32_t oct_grid(size_t n)
{
  size_t nb = (n + 255) / 256;
  return (uint32_t)(nb > 4096 ? 4096 : (nb ? nb : 1));
}

// digits (levels) two full-depth keys share from the top
__device__ __forceinline__ int oct_common_levels(const uint64_t a, const uint64_t b, const int depth)
{
  const uint64_t x = a ^ b;
  if (!x) return depth;
  const int hb = 63 - __clzll((long long)x);          // highest differing bit, < 3 * depth
  return (3 * depth - 1 - hb) / 3;
}

__device__ __forceinline__ int oct_leaf_depth_at(const uint64_t* __restrict__ sorted, const size_t n, const size_t i, const int depth,
                                                 const int earlystop)
{
  if (!earlystop) return depth;
  const uint64_t key = sorted[i];
  const size_t lo = i >= (size_t)OCT_EARLY_POINTS ? i - OCT_EARLY_POINTS : 0;
  const size_t hi = i + OCT_EARLY_POINTS < n ? i + OCT_EARLY_POINTS : n - 1;
  for (int L = 1; L < depth; L++) {
    int cnt = 0;
    for (size_t j = lo; j <= hi; j++) cnt += oct_common_levels(key, sorted[j], depth) >= L;   // j == i counts itself
    if (cnt <= OCT_EARLY_POINTS) return L;
  }
  return depth;
}

__global__ __launch_bounds__(256) void k_oct_leaf_depth(const uint64_t* __restrict__ sorted, size_t n, int depth, int earlystop,
                                                        uint8_t* __restrict__ ld, uint32_t* __restrict__ counts)
{
  __shared__ uint32_t sh[32];
  if (threadIdx.x < 32) sh[threadIdx.x] = 0;
  __syncthreads();
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int l = oct_leaf_depth_at(sorted, n, i, depth, earlystop);
    ld[i] = (uint8_t)l;
    // position i starts the nodes of the depths its key prefix is new at, down to its leaf
    const int from = i ? oct_common_levels(sorted[i], sorted[i - 1], depth) + 1 : 1;
    for (int L = from; L <= l; L++) atomicAdd(&sh[L], 1u);
    if (from <= l) atomicAdd(&sh[31], 1u);
  }
  __syncthreads();
  if (threadIdx.x < 32 && sh[threadIdx.x]) atomicAdd(&counts[threadIdx.x], sh[threadIdx.x]);
}

__device__ __forceinline__ uint64_t oct_masked(const uint64_t key, const int l, const int depth)
{
  const int sh = 3 * (depth - l);
  return sh ? (key >> sh) << sh : key;
}

__global__ __launch_bounds__(256) void k_oct_mask_keys(uint64_t* __restrict__ keys, const uint64_t* __restrict__ sorted,
                                                       const uint8_t* __restrict__ ld, size_t n, int depth)
{
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint64_t key = keys[i];
    size_t lo = 0, hi = n;                   // any position of the key: equal keys lie in one cell and share its leaf
    while (lo < hi) {
      const size_t m = lo + ((hi - lo) >> 1);
      if (sorted[m] < key) lo = m + 1; else hi = m;
    }
    keys[i] = oct_masked(key, ld[lo < n ? lo : n - 1], depth);
  }
}

__global__ __launch_bounds__(256) void k_oct_mask_sorted(uint64_t* __restrict__ sorted, const uint8_t* __restrict__ ld, size_t n, int depth)
{
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) sorted[i] = oct_masked(sorted[i], ld[i], depth);
}

// (the keys may be masked here: a node of depth L <= ld keeps its L digits)
__global__ __launch_bounds__(256) void k_oct_level_flags(const uint64_t* __restrict__ sorted, const uint8_t* __restrict__ ld, size_t n,
                                                         int depth, int L, uint32_t* __restrict__ flags)
{
  const int sh = 3 * (depth - L);
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += stride)
    flags[i] = (i < n && (int)ld[i] >= L && (i == 0 || (sorted[i] >> sh) != (sorted[i - 1] >> sh))) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_oct_level_emit(const OctEmit e)
{
  const int sh = 3 * (e.depth - e.L);
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < e.n; i += stride) {
    if (e.L == 1 && i == 0) { e.nodes[0].start = 0u; e.nodes[0].count = e.n; }      // the root: every point
    if (!e.flags[i]) continue;
    const uint64_t prefix = e.sorted[i] >> sh;
    uint32_t lo = (uint32_t)i + 1u, hi = e.n;          // end of the run: the first position behind i with another prefix
    while (lo < hi) {
      const uint32_t m = lo + ((hi - lo) >> 1);
      if ((e.sorted[m] >> sh) == prefix) lo = m + 1; else hi = m;
    }
    const uint32_t slot = e.base + e.rank[i];
    const bool leaf = (int)e.ld[i] == e.L;
    e.nodes[slot].start = (uint32_t)i;
    e.nodes[slot].count = lo - (uint32_t)i;
    // the parent: the node of depth L - 1 whose run holds i (its start is the last flagged position <= i)
    const bool first = e.L == 1 ? i == 0 : e.pflags[i] != 0u;
    const uint32_t parent = e.L == 1 ? 0u : e.pbase + e.prank[i] + e.pflags[i] - 1u;
    const uint32_t ci = (uint32_t)(prefix & 7ull);
    atomicOr(&e.nodes[parent].masks, (1u << ci) | (leaf ? (0x100u << ci) : 0u));
    if (first) e.nodes[parent].first = slot;
  }
}

__global__ __launch_bounds__(256) void k_oct_points(const double* __restrict__ xyz, const uint32_t* __restrict__ perm, size_t n,
                                                    KdPoint* __restrict__ pts)
{
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t pos = (size_t)blockIdx.x * blockDim.x + threadIdx.x; pos < n; pos += stride) {
    const uint32_t src = perm[pos];
    KdPoint p;
    p.x = xyz[3 * (size_t)src]; p.y = xyz[3 * (size_t)src + 1]; p.z = xyz[3 * (size_t)src + 2];
    p.orig = (int32_t)src; p.pad = 0;
    pts[pos] = p;
  }
}

hipError_t launch_oct_leaf_depth(uint64_t* sorted, size_t n, int depth, int earlystop, uint8_t* ld, uint32_t* counts, hipStream_t s)
{
  hipLaunchKernelGGL(k_oct_leaf_depth, dim3(oct_grid(n)), dim3(256), 0, s, sorted, n, depth, earlystop, ld, counts);
  return hipGetLastError();
}
hipError_t launch_oct_mask_keys(uint64_t* keys, const uint64_t* sorted_full, const uint8_t* ld, size_t n, int depth, hipStream_t s)
{
  hipLaunchKernelGGL(k_oct_mask_keys, dim3(oct_grid(n)), dim3(256), 0, s, keys, sorted_full, ld, n, depth);
  return hipGetLastError();
}
hipError_t launch_oct_mask_sorted(uint64_t* sorted, const uint8_t* ld, size_t n, int depth, hipStream_t s)
{
  hipLaunchKernelGGL(k_oct_mask_sorted, dim3(oct_grid(n)), dim3(256), 0, s, sorted, ld, n, depth);
  return hipGetLastError();
}
hipError_t launch_oct_level_flags(const uint64_t* sorted, const uint8_t* ld, size_t n, int depth, int L, uint32_t* flags, hipStream_t s)
{
  hipLaunchKernelGGL(k_oct_level_flags, dim3(oct_grid(n + 1)), dim3(256), 0, s, sorted, ld, n, depth, L, flags);
  return hipGetLastError();
}
hipError_t launch_oct_level_emit(const OctEmit& e, hipStream_t s)
{
  hipLaunchKernelGGL(k_oct_level_emit, dim3(oct_grid(e.n)), dim3(256), 0, s, e);
  return hipGetLastError();
}
hipError_t launch_oct_points(const double* xyz, const uint32_t* perm, size_t n, KdPoint* pts, hipStream_t s)
{
  hipLaunchKernelGGL(k_oct_points, dim3(oct_grid(n)), dim3(256), 0, s, xyz, perm, n, pts);
  return hipGetLastError();
}

// ---- search ------------------------------------------------------------------------------------------------------------
constexpr int OCT_BLOCK = 128;

// The queries into the tree's frame -- transform3 (globals.icc:1477-1490): ((x*a0 + y*a4) + z*a8) + a12, as k_search does it
// in its own prologue -- and the range check of what the walk converts to int.  A pass of its own: the walk then carries
// neither the matrix nor the check.
__global__ __launch_bounds__(256) void k_oct_prepare(const OctPrepArgs a)
{
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  bool bad = false;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
    double qx = a.x[i], qy = a.y[i], qz = a.z[i];
    if (a.has_inv) {
      const double tx = qx, ty = qy, tz = qz;
      qx = tx * a.inv.m[0] + ty * a.inv.m[4] + tz * a.inv.m[8] + a.inv.m[12];
      qy = tx * a.inv.m[1] + ty * a.inv.m[5] + tz * a.inv.m[9] + a.inv.m[13];
      qz = tx * a.inv.m[2] + ty * a.inv.m[6] + tz * a.inv.m[10] + a.inv.m[14];
      a.ox[i] = qx; a.oy[i] = qy; a.oz[i] = qz;
    }
    bad |= !oct_in_range((qx + a.add[0]) * a.mult) || !oct_in_range((qy + a.add[1]) * a.mult) || !oct_in_range((qz + a.add[2]) * a.mult);
  }
  if (bad) *a.bad = 1u;        // every lane that sees one stores the same value: a plain store
}

// the per-level stack of a lane: column `lane` of [levels][OCT_BLOCK] 8-byte entries in LDS
struct OctStackLds {
  uint2* col;
  __device__ __forceinline__ void put(const int level, const uint32_t a, const uint32_t b) { col[level * OCT_BLOCK] = make_uint2(a, b); }
  __device__ __forceinline__ void get(const int level, uint32_t& a, uint32_t& b) const { const uint2 e = col[level * OCT_BLOCK]; a = e.x; b = e.y; }
};

__global__ __launch_bounds__(OCT_BLOCK) void k_oct_find(const OctSearchArgs a)
{
  extern __shared__ __attribute__((aligned(16))) uint2 oct_lds[];
  OctStackLds st{oct_lds + threadIdx.x};
  const size_t stride = (size_t)gridDim.x * OCT_BLOCK;
  for (size_t i = (size_t)blockIdx.x * OCT_BLOCK + threadIdx.x; i < a.n; i += stride) {
    double d2;
    int32_t slot, leaves;
    oct_find_closest(a.T, a.x[i], a.y[i], a.z[i], a.maxd2, st, slot, d2, leaves);
    a.kpos[i] = slot;
    if (a.d2) a.d2[i] = d2;
  }
}

// ---- the ICP loop: one iteration is k_oct_loop_prepare, k_oct_loop_find and the pair sums, the host waits for the sums only --
// The scan moves here, not in a launch of its own: Scan::transformReduced (scan.cc:851-875) as k_transform does it -- the
// point (x*a0 + y*a4 + z*a8), then + a12; the normal by the transposed rotation block -- so the scan behind the loop has the
// bits of one moved by tdtk_scan_transform iteration by iteration.  The rest is k_oct_prepare on the moved point.
__global__ __launch_bounds__(256) void k_oct_loop_prepare(const OctLoopPrepArgs a)
{
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  bool bad = false;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
    double px = a.x[i], py = a.y[i], pz = a.z[i];
    if (a.has_pending) {
      const double* m = a.pending.m;
      const double xn = px * m[0] + py * m[4] + pz * m[8];
      const double yn = px * m[1] + py * m[5] + pz * m[9];
      const double zn = px * m[2] + py * m[6] + pz * m[10];
      px = xn + m[12]; py = yn + m[13]; pz = zn + m[14];
      a.x[i] = px; a.y[i] = py; a.z[i] = pz;
      if (a.nx) {
        const double ux = a.nx[i], uy = a.ny[i], uz = a.nz[i];
        a.nx[i] = ux * m[0] + uy * m[1] + uz * m[2];
        a.ny[i] = ux * m[4] + uy * m[5] + uz * m[6];
        a.nz[i] = ux * m[8] + uy * m[9] + uz * m[10];
      }
    }
    const double qx = px * a.inv.m[0] + py * a.inv.m[4] + pz * a.inv.m[8] + a.inv.m[12];
    const double qy = px * a.inv.m[1] + py * a.inv.m[5] + pz * a.inv.m[9] + a.inv.m[13];
    const double qz = px * a.inv.m[2] + py * a.inv.m[6] + pz * a.inv.m[10] + a.inv.m[14];
    a.ox[i] = qx; a.oy[i] = qy; a.oz[i] = qz;
    bad |= !oct_in_range((qx + a.add[0]) * a.mult) || !oct_in_range((qy + a.add[1]) * a.mult) || !oct_in_range((qz + a.add[2]) * a.mult);
  }
  if (bad) *a.bad = 1u;
}

// k_oct_find behind a prepare pass nobody has looked at: the range word is read here, once per wave and the same for all of
// them, and a raised one means no coordinate is converted to int at all -- every query leaves with kpos = -1 and the host,
// which receives the word with the sums, refuses the iteration.  Behind that the loop is k_oct_find's; SKIP (-R): a query
// that was not drawn leaves with kpos = -1, unwalked.
template <bool SKIP>
__global__ __launch_bounds__(OCT_BLOCK) void k_oct_loop_find(const OctLoopSearchArgs a)
{
  extern __shared__ __attribute__((aligned(16))) uint2 oct_lds[];
  OctStackLds st{oct_lds + threadIdx.x};
  const size_t stride = (size_t)gridDim.x * OCT_BLOCK;
  if (*a.bad != 0u) {
    for (size_t i = (size_t)blockIdx.x * OCT_BLOCK + threadIdx.x; i < a.n; i += stride) a.kpos[i] = -1;
    return;
  }
  for (size_t i = (size_t)blockIdx.x * OCT_BLOCK + threadIdx.x; i < a.n; i += stride) {
    if (SKIP && a.skip[i]) { a.kpos[i] = -1; continue; }
    double d2;
    int32_t slot, leaves;
    oct_find_closest(a.T, a.x[i], a.y[i], a.z[i], a.maxd2, st, slot, d2, leaves);
    a.kpos[i] = slot;
  }
}

hipError_t launch_oct_loop_prepare(const OctLoopPrepArgs& a, hipStream_t s)
{
  if (!a.n) return hipSuccess;
  hipLaunchKernelGGL(k_oct_loop_prepare, dim3(oct_grid(a.n)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_oct_loop_search(const OctLoopSearchArgs& a, hipStream_t s)
{
  if (!a.n) return hipSuccess;
  const int depth = a.levels > 1 ? a.levels - 1 : 1;      // as launch_oct_search
  const size_t lds = (size_t)depth * OCT_BLOCK * sizeof(uint2);
  size_t nb = (a.n + OCT_BLOCK - 1) / OCT_BLOCK;
  if (nb > 65536) nb = 65536;
  if (a.skip) hipLaunchKernelGGL(k_oct_loop_find<true>, dim3((uint32_t)nb), dim3(OCT_BLOCK), lds, s, a);
  else hipLaunchKernelGGL(k_oct_loop_find<false>, dim3((uint32_t)nb), dim3(OCT_BLOCK), lds, s, a);
  return hipGetLastError();
}

hipError_t launch_oct_prepare(const OctPrepArgs& a, hipStream_t s)
{
  if (!a.n) return hipSuccess;
  hipLaunchKernelGGL(k_oct_prepare, dim3(oct_grid(a.n)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_oct_search(const OctSearchArgs& a, hipStream_t s)
{
  if (!a.n) return hipSuccess;
  // a node is entered (and its parent's entry stored) at most levels - 1 times on the way down
  const int depth = a.levels > 1 ? a.levels - 1 : 1;
  const size_t lds = (size_t)depth * OCT_BLOCK * sizeof(uint2);
  size_t nb = (a.n + OCT_BLOCK - 1) / OCT_BLOCK;
  if (nb > 65536) nb = 65536;
  hipLaunchKernelGGL(k_oct_find, dim3((uint32_t)nb), dim3(OCT_BLOCK), lds, s, a);
  return hipGetLastError();
}

}  // namespace tdtk
