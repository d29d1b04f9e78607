// The device voxel grid: tdtk_voxel_walk (the reference's walk_voxels as a ray-through-grid query) and tdtk_peopleremover
// (dynamic-object removal by free-space carving, src/peopleremover/peopleremover.cc:176-545).  The per-lane code -- keys,
// the brick table's lookup, the walk, the visitor, the half-free rule -- is voxel_lane.h; here are the kernels around it.
//
//   keys      one lane per point: its voxel key (brick-major, voxel_lane.h) and its scan id; every coordinate checked
//   sort      rocPRIM radix sort of (key, scan), stable, so scan ids ascend inside a key (points come scan by scan)
//   flags     heads of (key, scan) pairs, of voxels, of bricks; three exclusive scans
//   compact   the unique pairs' scan ids, the voxels' CSR starts and keys, the bricks' keys and first voxels
//   table     one lane per brick: its occupancy word from its voxels' low key bits, inserted by a 64-bit CAS on the slot's key
//   carve     one ray per lane, scanner -> point, under the reference's visitor; a free mark is a byte store
//   cluster   26-neighbour union-find over the free voxels (cluster_lane.h's lock-free hook and halving), sizes, removal
//   classify  one lane per voxel: the (voxel, scan) pairs' dynamic bytes, half-free count; one lane per point: its pair's byte
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "kernels.h"
#include "query.h"
#include "query_lane.h"
#include "cluster_lane.h"
#include "voxel.h"

namespace tdtk {

constexpr int V_BLOCK = 256;
constexpr int V_WALK_BLOCK = 64;     // one wave: a long ray holds back 63 lanes, not 255

static inline uint32_t v_grid(size_t n, int block) { return (uint32_t)((n + block - 1) / block); }

__device__ __forceinline__ VoxGrid vox_grid_of(const VoxArgs& a)
{
  VoxGrid g;
  g.table = a.table; g.mask = a.mask; g.vstart = a.vstart; g.pscan = a.pscan; g.vkey = a.vkey; g.n_vox = a.n_vox;
  return g;
}

__device__ __forceinline__ uint32_t vox_point_err(const double* p, const double vs)
{
  return vox_coord_err(p[0], vs) | vox_coord_err(p[1], vs) | vox_coord_err(p[2], vs);
}

__device__ __forceinline__ void vox_add_wave(unsigned long long* ctr, unsigned long long v)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += (unsigned long long)__shfl_xor((long long)v, off, 64);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(ctr, v);
}

__global__ void __launch_bounds__(V_BLOCK) k_vox_keys(const VoxArgs a)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t err = 0;
  if (i < a.n) {
    const double* p = a.xyz + 3 * i;
    err |= vox_point_err(p, a.vs);
    if (a.ends) err |= vox_point_err(a.ends + 3 * i, a.vs);
    uint32_t lo = 0, hi = a.S;                 // the largest scan whose offset is <= i: empty scans own no point
    while (lo < hi) {
      const uint32_t mid = (lo + hi + 1u) >> 1;
      if (a.scan_off[mid] <= i) lo = mid; else hi = mid - 1u;
    }
    a.scans[i] = lo;
    a.keys[i] = err ? 0ull : vox_key_of_point(p, a.vs);
  }
  if (i < a.S) err |= vox_point_err(a.origins + 3 * i, a.vs);
  if (err) atomicOr(a.ctr, (unsigned long long)err);
}

__global__ void __launch_bounds__(V_BLOCK) k_vox_flags(const VoxArgs a)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > a.n) return;
  uint32_t hp = 0, hv = 0, hb = 0;
  if (i < a.n) {
    const uint64_t k = a.keys_s[i];
    if (i == 0) hp = hv = hb = 1u;
    else {
      const uint64_t kp = a.keys_s[i - 1];
      hv = k != kp;
      hb = (k >> 6) != (kp >> 6);
      hp = hv || a.scans_s[i] != a.scans_s[i - 1];
    }
  }
  a.fp[i] = hp; a.fv[i] = hv; a.fb[i] = hb;      // position n: 0, so that the scans' last entries are the totals
}

__global__ void __launch_bounds__(V_BLOCK) k_vox_compact(const VoxArgs a)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > a.n) return;
  if (i == a.n) {
    a.vstart[a.iv[i]] = a.ip[i];
    a.bbase[a.ib[i]] = a.iv[i];
    return;
  }
  if (a.fp[i]) a.pscan[a.ip[i]] = a.scans_s[i];
  if (a.fv[i]) { a.vkey[a.iv[i]] = a.keys_s[i]; a.vstart[a.iv[i]] = a.ip[i]; }
  if (a.fb[i]) { a.bkey[a.ib[i]] = a.keys_s[i] >> 6; a.bbase[a.ib[i]] = a.iv[i]; }
}

__global__ void __launch_bounds__(V_BLOCK) k_vox_table(const VoxArgs a)
{
  const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.n_bricks) return;
  const uint32_t v0 = a.bbase[b], v1 = a.bbase[b + 1];
  uint64_t word = 0;
  for (uint32_t v = v0; v < v1; ++v) word |= 1ull << (a.vkey[v] & 63u);
  const uint64_t bk = a.bkey[b];
  uint32_t h = (uint32_t)vox_hash(bk) & a.mask;
  for (;;) {                                      // brick keys are unique: a slot is either free or somebody else's
    const unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long*>(&a.table[h].key), (unsigned long long)VOX_EMPTY,
                                             (unsigned long long)bk);
    if (old == VOX_EMPTY) break;
    h = (h + 1u) & a.mask;
  }
  a.table[h].word = word;
  a.table[h].base = v0;
}

__global__ void __launch_bounds__(V_WALK_BLOCK) k_vox_carve(const VoxArgs a)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long visits = 0;
  if (i < a.n) {
    const VoxGrid g = vox_grid_of(a);
    const uint32_t scan = a.scans[i];
    VoxCarve visit{g, a.free_mark, 0u, 0u, BrickCache(), 0u};
    vox_window(scan, a.diff, visit.lo, visit.hi);
    const double* o = a.origins + 3 * (size_t)scan;
    const double* e = (a.ends ? a.ends : a.xyz) + 3 * i;
    const double sp[3] = {o[0], o[1], o[2]}, ep[3] = {e[0], e[1], e[2]};
    vox_walk(sp, ep, a.vs, visit);
    visits = visit.visits;
  }
  vox_add_wave(a.ctr + 1, visits);
}

// ---- cluster filter: the 26-connected components of the free voxels (peopleremover.cc:337-418) -------------------------------
template <int STEP>
__global__ void __launch_bounds__(V_BLOCK) k_vox_cluster(const VoxArgs a)
{
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= a.n_vox) return;
  if (STEP == 0) { a.parent[v] = v; a.csize[v] = 0u; return; }
  if (!a.free_mark[v]) return;
  if (STEP == 1) {
    const VoxGrid g = vox_grid_of(a);
    vox_neighbours(g, a.vkey[v], 1, [&](const uint32_t u) {
      if (u < v && a.free_mark[u]) uf_unite(a.parent, v, u);        // adjacency is symmetric: the pair is met from its larger index
    });
  } else if (STEP == 2) {
    uint32_t r = v;
    for (;;) {
      const uint32_t p = uf_load(a.parent, r);
      if (p == r) break;
      r = p;
    }
    if (r != v) __hip_atomic_store(a.parent + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    atomicAdd(a.csize + r, 1u);
  } else {
    if (a.csize[a.parent[v]] < a.cluster_size) a.free_mark[v] = 0;
  }
}

__global__ void __launch_bounds__(V_BLOCK) k_vox_classify_voxels(const VoxArgs a)
{
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long half = 0;
  if (w < a.n_vox) {
    const VoxGrid g = vox_grid_of(a);
    half = vox_classify_voxel(g, a.free_mark, a.subvoxel != 0, w, a.pdyn) ? 1u : 0u;
  }
  vox_add_wave(a.ctr + 4, half);
}

__global__ void __launch_bounds__(V_BLOCK) k_vox_classify_points(const VoxArgs a)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const VoxGrid g = vox_grid_of(a);
  a.dynamic[i] = vox_classify_point(g, a.keys[i], a.scans[i], a.pdyn);
}

// ---- tdtk_voxel_walk -------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(V_BLOCK) k_vox_walk_check(const double* __restrict__ starts, const double* __restrict__ ends,
                                                            const size_t m, const double vs, unsigned long long* __restrict__ ctr)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint32_t err = vox_point_err(starts + 3 * i, vs) | vox_point_err(ends + 3 * i, vs);
  if (err) atomicOr(ctr, (unsigned long long)err);
}

template <bool FILL>
__global__ void __launch_bounds__(V_WALK_BLOCK) k_vox_walk(const double* __restrict__ starts, const double* __restrict__ ends,
                                                           const size_t m, const double vs, uint32_t* __restrict__ counts,
                                                           const uint32_t* __restrict__ offsets, int32_t* __restrict__ voxels,
                                                           unsigned long long* __restrict__ ctr)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long visits = 0;
  if (i < m) {
    const double sp[3] = {starts[3 * i], starts[3 * i + 1], starts[3 * i + 2]};
    const double ep[3] = {ends[3 * i], ends[3 * i + 1], ends[3 * i + 2]};
    VoxList visit{FILL ? voxels + 3 * (size_t)offsets[i] : nullptr, 0u};
    vox_walk(sp, ep, vs, visit);
    if (!FILL) counts[i] = visit.visits;
    visits = visit.visits;
  } else if (i == m && !FILL) counts[m] = 0u;
  if (!FILL) vox_add_wave(ctr + 1, visits);
}

// ---- launchers --------------------------------------------------------------------------------------------------------------
size_t vox_sort_temp_bytes(size_t n)
{
  size_t tmp = 0;
  uint64_t* k = nullptr;
  uint32_t* v = nullptr;
  (void)rocprim::radix_sort_pairs(nullptr, tmp, k, k, v, v, n, 0, 63, (hipStream_t)0);
  const size_t sc = scan_u32_temp_bytes(n + 1);
  return tmp > sc ? tmp : sc;
}

hipError_t launch_vox_keys(const VoxArgs& a, hipStream_t s)
{
  const size_t items = a.n > a.S ? a.n : a.S;
  hipLaunchKernelGGL(k_vox_keys, dim3(v_grid(items, V_BLOCK)), dim3(V_BLOCK), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_vox_sort_flags(const VoxArgs& a, void* tmp, size_t tmp_bytes, hipStream_t s)
{
  hipError_t e = rocprim::radix_sort_pairs(tmp, tmp_bytes, a.keys, a.keys_s, a.scans, a.scans_s, (size_t)a.n, 0, 63, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_vox_flags, dim3(v_grid((size_t)a.n + 1, V_BLOCK)), dim3(V_BLOCK), 0, s, a);
  if ((e = launch_scan_u32(a.fp, a.ip, (size_t)a.n + 1, tmp, tmp_bytes, s)) != hipSuccess) return e;
  if ((e = launch_scan_u32(a.fv, a.iv, (size_t)a.n + 1, tmp, tmp_bytes, s)) != hipSuccess) return e;
  if ((e = launch_scan_u32(a.fb, a.ib, (size_t)a.n + 1, tmp, tmp_bytes, s)) != hipSuccess) return e;
  return hipGetLastError();
}

hipError_t launch_vox_compact(const VoxArgs& a, hipStream_t s)
{
  hipLaunchKernelGGL(k_vox_compact, dim3(v_grid((size_t)a.n + 1, V_BLOCK)), dim3(V_BLOCK), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_vox_table(const VoxArgs& a, hipStream_t s)
{
  hipLaunchKernelGGL(k_vox_table, dim3(v_grid(a.n_bricks, V_BLOCK)), dim3(V_BLOCK), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_vox_carve(const VoxArgs& a, hipStream_t s)
{
  hipLaunchKernelGGL(k_vox_carve, dim3(v_grid(a.n, V_WALK_BLOCK)), dim3(V_WALK_BLOCK), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_vox_cluster_filter(const VoxArgs& a, hipStream_t s)
{
  const dim3 g(v_grid(a.n_vox, V_BLOCK)), b(V_BLOCK);
  hipLaunchKernelGGL(k_vox_cluster<0>, g, b, 0, s, a);
  hipLaunchKernelGGL(k_vox_cluster<1>, g, b, 0, s, a);
  hipLaunchKernelGGL(k_vox_cluster<2>, g, b, 0, s, a);
  hipLaunchKernelGGL(k_vox_cluster<3>, g, b, 0, s, a);
  return hipGetLastError();
}

hipError_t launch_vox_classify(const VoxArgs& a, hipStream_t s)
{
  hipLaunchKernelGGL(k_vox_classify_voxels, dim3(v_grid(a.n_vox, V_BLOCK)), dim3(V_BLOCK), 0, s, a);
  hipLaunchKernelGGL(k_vox_classify_points, dim3(v_grid(a.n, V_BLOCK)), dim3(V_BLOCK), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_vox_walk_check(const double* starts, const double* ends, size_t m, double vs, unsigned long long* ctr,
                                 hipStream_t s)
{
  if (!m) return hipSuccess;
  hipLaunchKernelGGL(k_vox_walk_check, dim3(v_grid(m, V_BLOCK)), dim3(V_BLOCK), 0, s, starts, ends, m, vs, ctr);
  return hipGetLastError();
}

hipError_t launch_vox_walk_count(const double* starts, const double* ends, size_t m, double vs, uint32_t* counts,
                                 unsigned long long* ctr, hipStream_t s)
{
  hipLaunchKernelGGL(k_vox_walk<false>, dim3(v_grid(m + 1, V_WALK_BLOCK)), dim3(V_WALK_BLOCK), 0, s, starts, ends, m, vs, counts,
                     (const uint32_t*)nullptr, (int32_t*)nullptr, ctr);
  return hipGetLastError();
}

hipError_t launch_vox_walk_fill(const double* starts, const double* ends, size_t m, double vs, const uint32_t* offsets,
                                int32_t* voxels, hipStream_t s)
{
  if (!m) return hipSuccess;
  hipLaunchKernelGGL(k_vox_walk<true>, dim3(v_grid(m, V_WALK_BLOCK)), dim3(V_WALK_BLOCK), 0, s, starts, ends, m, vs,
                     (uint32_t*)nullptr, offsets, voxels, (unsigned long long*)nullptr);
  return hipGetLastError();
}

}  // namespace tdtk
