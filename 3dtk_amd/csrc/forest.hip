// lib3dtk_hip.so -- the dynamic kd-forest: BkdTree (include/slam6d/bkd.h, src/slam6d/bkd.cc; Procopiuc et al.), the
// logarithmic method over the device kd-trees.  This file holds what needs the device: the query kernels (one launch per
// call over all slots and the buffer), the remove pass and the gathers of a merge, on query.hip's scaffold (query_dev.h: the
// kernarg block, the lane stack, the launch constants).  Everything a lane does, with the rules of every query, is in
// forest_lane.h; the tree walks themselves are query_lane.h's.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "forest.h"
#include "query_dev.h"

namespace tdtk {

// ---- queries ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(Q_BLOCK) k_forest_find_closest(const ForestArgs a_)
{
  const ForestArgs& f = q_args<ForestArgs>();
  const QueryArgs& a = f.q;
  __shared__ uint4 s_stack[Q_SD][Q_BLOCK];
  for (LaneQueries<Q_BLOCK> q(a, s_stack); q.i < a.n; q.i += q.T) {
    const size_t i = q.i;
    const size_t o = a.order ? (size_t)a.order[i] : i;
    int32_t id;
    double d2;
    forest_find_closest(f, a.x[i], a.y[i], a.z[i], a.r2, q.st, id, d2);
    a.idx[o] = id;
    if (a.d2) a.d2[o] = d2;
  }
}

// KCAP: the list's capacity (k <= KCAP)
template <int KCAP>
__global__ void __launch_bounds__(Q_BLOCK_L) k_forest_knn(const ForestArgs a_)
{
  const ForestArgs& f = q_args<ForestArgs>();
  const QueryArgs& a = f.q;
  __shared__ uint4 s_stack[Q_SD][Q_BLOCK_L];
  __shared__ double s_d[KCAP][Q_BLOCK_L];
  __shared__ uint32_t s_s[KCAP][Q_BLOCK_L];
  ListLds<Q_BLOCK_L> L;
  L.ld = &s_d[0][threadIdx.x];
  L.ls = &s_s[0][threadIdx.x];
  const int k = a.k;
  for (LaneQueries<Q_BLOCK_L> q(a, s_stack); q.i < a.n; q.i += q.T) {
    const size_t i = q.i;
    const size_t o = a.order ? (size_t)a.order[i] : i;
    L.init(k);
    forest_knn(f, a.x[i], a.y[i], a.z[i], L, q.st);
    int32_t* row = a.idx + o * (size_t)k;
    double* drow = a.d2 ? a.d2 + o * (size_t)k : nullptr;
    for (int j = 0; j < k; j++) {
      const bool v = L.dist(j) >= 0.0;
      row[j] = v ? (int32_t)L.slot(j) : -1;
      if (drow) drow[j] = v ? L.dist(j) : -1.0;
    }
  }
}

__global__ void __launch_bounds__(Q_BLOCK) k_forest_range_count(const ForestArgs a_)
{
  const ForestArgs& f = q_args<ForestArgs>();
  const QueryArgs& a = f.q;
  __shared__ uint4 s_stack[Q_SD][Q_BLOCK];
  for (LaneQueries<Q_BLOCK> q(a, s_stack); q.i < a.n; q.i += q.T) {
    const size_t i = q.i;
    uint32_t c = 0;
    auto emit = [&](int32_t, double) { ++c; };
    forest_fixed_range(f, a.x[i], a.y[i], a.z[i], a.r2, q.st, emit);
    a.counts[a.order ? (size_t)a.order[i] : i] = c;
  }
}

__global__ void __launch_bounds__(Q_BLOCK) k_forest_range_fill(const ForestArgs a_)
{
  const ForestArgs& f = q_args<ForestArgs>();
  const QueryArgs& a = f.q;
  __shared__ uint4 s_stack[Q_SD][Q_BLOCK];
  for (LaneQueries<Q_BLOCK> q(a, s_stack); q.i < a.n; q.i += q.T) {
    const size_t i = q.i;
    const size_t o = a.order ? (size_t)a.order[i] : i;
    unsigned long long w = a.offsets[o];
    const unsigned long long end = a.offsets[o + 1];
    auto emit = [&](int32_t id, double md) {
      if (w < end) {       // (the count walk made the same visits: never false)
        a.idx[w] = id;
        if (a.d2) a.d2[w] = md;
      }
      ++w;
    };
    forest_fixed_range(f, a.x[i], a.y[i], a.z[i], a.r2, q.st, emit);
  }
}

// ---- the remove pass -------------------------------------------------------------------------------------------------
// Requests of one call behave as if applied in order, although every request of a round looks for its candidate at once
// (forest_remove_find).  A round: every pending request claims its candidate with an atomic minimum of its own number on the
// point's pad word; a request that finds another number there has lost.  A winner commits (orig = -1) only when its number
// is below the smallest loser's: a request in front of it in the call's order may yet take a point it would have to see
// gone.  Everybody else stays pending for the next round, on the points that are left.  A request that finds nothing is
// done: points only ever go.  The smallest pending request always commits or finds nothing, so every round ends at least
// one; with distinct requests -- a mask over ids -- one round ends them all.
__global__ void k_forest_remove_reset(uint32_t* ctl)
{
  ctl[0] = 0xFFFFFFFFu;
  ctl[1] = 0u;
}

__global__ void __launch_bounds__(Q_BLOCK) k_forest_remove_find(const ForestArgs a_)
{
  const ForestArgs& f = q_args<ForestArgs>();
  const QueryArgs& a = f.q;
  __shared__ uint4 s_stack[Q_SD][Q_BLOCK];
  for (LaneQueries<Q_BLOCK> q(a, s_stack); q.i < a.n; q.i += q.T) {
    const size_t i = q.i;
    const size_t o = a.order ? (size_t)a.order[i] : i;
    if (f.res[o] != -2) continue;
    int32_t c = -1;
    uint32_t p = 0;
    if (forest_remove_find(f, a.x[i], a.y[i], a.z[i], q.st, c, p)) {
      f.cand_c[o] = c;
      f.cand_p[o] = p;
      atomicMin(&forest_point(f, c, p)->pad, (int32_t)o);
    } else {
      f.res[o] = -1;
    }
  }
}

// STEP 0: the smallest request that lost its claim; STEP 1: commit, or stay pending
template <int STEP>
__global__ void __launch_bounds__(256) k_forest_remove_settle(const ForestArgs a_)
{
  const ForestArgs& f = q_args<ForestArgs>();
  const size_t T = (size_t)gridDim.x * blockDim.x;
  for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < f.q.n; o += T) {
    if (f.res[o] != -2) continue;
    const int32_t c = f.cand_c[o];
    KdPoint* pt = forest_point(f, c, f.cand_p[o]);
    const bool won = pt->pad == (int32_t)o;
    if (STEP == 0) {
      if (!won) atomicMin(&f.ctl[0], (uint32_t)o);
    } else if (won && (uint32_t)o < f.ctl[0]) {
      f.res[o] = pt->orig;
      pt->orig = FOREST_DEAD;
      atomicAdd(&f.ctl[2 + c], 1u);
    } else {
      if (won) pt->pad = FOREST_UNCLAIMED;
      atomicAdd(&f.ctl[1], 1u);
    }
  }
}

// ---- the gathers of a merge --------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_forest_copy_points(const KdPoint* __restrict__ pts, const size_t n, double* __restrict__ xyz,
                                                            int32_t* __restrict__ ids, const size_t base)
{
  const size_t T = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += T) {
    const KdPoint p = pts[i];
    double* o = xyz + 3 * (base + i);
    o[0] = p.x; o[1] = p.y; o[2] = p.z;
    ids[base + i] = p.orig;
  }
}

__global__ void __launch_bounds__(256) k_forest_live_flags(const KdPoint* __restrict__ pts, const size_t n, uint32_t* __restrict__ flags)
{
  const size_t T = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += T) flags[i] = (i < n && pts[i].orig >= 0) ? 1u : 0u;
}

__global__ void __launch_bounds__(256) k_forest_compact_points(const KdPoint* __restrict__ pts, const size_t n,
                                                               const uint32_t* __restrict__ offs, double* __restrict__ xyz,
                                                               int32_t* __restrict__ ids, const size_t base)
{
  const size_t T = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += T) {
    const KdPoint p = pts[i];
    if (p.orig < 0) continue;
    const size_t w = base + offs[i];
    double* o = xyz + 3 * w;
    o[0] = p.x; o[1] = p.y; o[2] = p.z;
    ids[w] = p.orig;
  }
}

__global__ void __launch_bounds__(256) k_forest_copy_new(const double* __restrict__ src, const size_t a, const size_t b,
                                                         const int32_t first_id, double* __restrict__ xyz, int32_t* __restrict__ ids,
                                                         const size_t base)
{
  const size_t T = (size_t)gridDim.x * blockDim.x;
  for (size_t i = a + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < b; i += T) {
    const size_t w = base + (i - a);
    xyz[3 * w] = src[3 * i]; xyz[3 * w + 1] = src[3 * i + 1]; xyz[3 * w + 2] = src[3 * i + 2];
    ids[w] = first_id + (int32_t)i;
  }
}

__global__ void __launch_bounds__(256) k_forest_relabel(KdPoint* __restrict__ pts, const size_t n, const int32_t* __restrict__ ids)
{
  const size_t T = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += T) {
    if (ids) pts[i].orig = ids[pts[i].orig];
    pts[i].pad = FOREST_UNCLAIMED;
  }
}

// ---- launchers -------------------------------------------------------------------------------------------------------
typedef void (*ForestKernel)(const ForestArgs);

static hipError_t launch_f(ForestKernel kernel, const ForestArgs& a, hipStream_t s, int block = Q_BLOCK)
{
  if (a.nslots < 0 || a.nslots > FOREST_MAX_SLOTS) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, dim3(q_grid(a.q.n, block)), dim3(block), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_forest_find_closest(const ForestArgs& a, hipStream_t s) { return launch_f(k_forest_find_closest, a, s); }

hipError_t launch_forest_knn(const ForestArgs& a, hipStream_t s)
{
  if (a.q.k < 1 || a.q.k > KNN_MAX_K) return hipErrorInvalidValue;
  return launch_f(a.q.k <= 16 ? k_forest_knn<16> : k_forest_knn<KNN_MAX_K>, a, s, Q_BLOCK_L);
}

hipError_t launch_forest_range_count(const ForestArgs& a, hipStream_t s) { return launch_f(k_forest_range_count, a, s); }
hipError_t launch_forest_range_fill(const ForestArgs& a, hipStream_t s) { return launch_f(k_forest_range_fill, a, s); }

hipError_t launch_forest_remove_round(const ForestArgs& a, hipStream_t s)
{
  if (!a.q.n) return hipSuccess;
  hipLaunchKernelGGL(k_forest_remove_reset, dim3(1), dim3(1), 0, s, a.ctl);
  hipError_t e = launch_f(k_forest_remove_find, a, s);
  if (e != hipSuccess) return e;
  if ((e = launch_f(k_forest_remove_settle<0>, a, s, 256)) != hipSuccess) return e;
  return launch_f(k_forest_remove_settle<1>, a, s, 256);
}

hipError_t launch_forest_copy_points(const KdPoint* pts, size_t n, double* xyz, int32_t* ids, size_t base, hipStream_t s)
{
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_forest_copy_points, dim3(q_grid(n, 256)), dim3(256), 0, s, pts, n, xyz, ids, base);
  return hipGetLastError();
}

hipError_t launch_forest_live_flags(const KdPoint* pts, size_t n, uint32_t* flags, hipStream_t s)
{
  hipLaunchKernelGGL(k_forest_live_flags, dim3(q_grid(n + 1, 256)), dim3(256), 0, s, pts, n, flags);
  return hipGetLastError();
}

hipError_t launch_forest_compact_points(const KdPoint* pts, size_t n, const uint32_t* offs, double* xyz, int32_t* ids, size_t base,
                                        hipStream_t s)
{
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_forest_compact_points, dim3(q_grid(n, 256)), dim3(256), 0, s, pts, n, offs, xyz, ids, base);
  return hipGetLastError();
}

hipError_t launch_forest_copy_new(const double* src_xyz, size_t a, size_t b, int32_t first_id, double* xyz, int32_t* ids, size_t base,
                                  hipStream_t s)
{
  if (b <= a) return hipSuccess;
  hipLaunchKernelGGL(k_forest_copy_new, dim3(q_grid(b - a, 256)), dim3(256), 0, s, src_xyz, a, b, first_id, xyz, ids, base);
  return hipGetLastError();
}

hipError_t launch_forest_relabel(KdPoint* pts, size_t n, const int32_t* ids, hipStream_t s)
{
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_forest_relabel, dim3(q_grid(n, 256)), dim3(256), 0, s, pts, n, ids);
  return hipGetLastError();
}

}  // namespace tdtk
