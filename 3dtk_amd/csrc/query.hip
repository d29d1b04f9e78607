// lib3dtk_hip.so -- k nearest neighbours, fixed-radius search and k-nearest-within-radius search on the resident kd-tree,
// the normal estimators built on them, and the cylinder, box and segment queries: KDTreeImpl::_KNNSearch (kdTreeImpl.h:627-682),
// _FixedRangeSearch (kdTreeImpl.h:585-625), _KNNRangeSearch (kdTreeImpl.h:684-745), calculateNormalsKNN / calculateNormalsRange with calculateNormal's PCA (normals.cc:369-439,
// 442-516, 518-558), _fixedRangeSearchAlongDir / _fixedRangeSearchBetween2Points / _AABBSearch / _segmentSearch_all /
// _segmentSearch_1NearestPoint (kdTreeImpl.h:432-577, 747-913); and collision_model's marking and axis depth fused over the
// range and segment walks (collision_model.cc:312-430, 714-800); and radius clustering, the connected components of the
// fixed-radius graph (segment_colliding.cc:55-102), over the range walk under an emitter that hooks a union-find.
//
// This file holds what needs the device: the register list, list_normal, the kernels and the launchers.  The kernarg block,
// the lane stack's set-up and the launch constants are in query_dev.h (shared with forest.hip); the walks and everything else
// a lane does, with the rules of every walk, are in query_lane.h.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include "kernels.h"
#include "eigen3.h"
#include "query.h"
#include "query_dev.h"
#include "query_lane.h"
#include "cluster_lane.h"

namespace tdtk {

// ---- the k-NN list, in registers (the LDS form: ListLds, query_lane.h) ---------------------------------------------
// KC slots, every index static (nothing goes to scratch).  The list is the LAST k slots, k0 = KC - k;
// the k0 slots in front hold -0.0, which is neither unset (-0.0 < 0.0 is false) nor larger than any distance, so an
// insertion never stops there and never shifts them: the bubble below needs no per-slot test of k, and distances[k-1]
// is always slot KC-1.
// (CHAIN: the adaptive kernel's form of the search for pos, see there)
template <int KC, bool CHAIN = false>
struct ListReg {
  double d[KC];
  uint32_t s[KC];
  double kth;   // distances[k-1]
  __device__ __forceinline__ void init(const int k0)
  {
#pragma unroll
    for (int j = 0; j < KC; j++) { d[j] = (j < k0) ? -0.0 : -1.0; s[j] = 0xFFFFFFFFu; }
    kth = -1.0;
  }
  __device__ __forceinline__ bool full() const { return kth != -1.0; }
  __device__ __forceinline__ void insert(const double md, const uint32_t slot)
  {
    if (kth != -1.0 && kth <= md) return;      // full and no slot larger than md: the reference's loop finds no place
    // the first slot that is unset or strictly larger takes the point (found from the back: a plain minimum, exact even
    // where a NaN distance breaks the order), every slot behind it takes its left neighbour, the last one drops out
    int pos = KC;
#pragma unroll
    for (int j = KC - 1; j >= 0; j--) {
      double mj = md;
      if (CHAIN) asm volatile("" : "+v"(mj), "+v"(pos));
      else asm volatile("" : "+v"(mj));
      pos = (d[j] < 0.0 || d[j] > mj) ? j : pos;
    }
#pragma unroll
    for (int j = KC - 1; j > 0; j--) {
      // (pos - j through an empty asm: the compiler would otherwise form all 2 KC lane masks up front, in SGPRs -- they spill)
      int pj = pos - j;
      asm volatile("" : "+v"(pj));
      const bool up = pj < 0, at = pj == 0;
      d[j] = up ? d[j - 1] : (at ? md : d[j]);
      s[j] = up ? s[j - 1] : (at ? slot : s[j]);
    }
    d[0] = (pos == 0) ? md : d[0];
    s[0] = (pos == 0) ? slot : s[0];
    kth = d[KC - 1];
  }
};

// list_cov and normal_from_cov in one: the same arithmetic (cov_eigen fills the upper triangle itself), kept as a second
// copy because of what the compiler makes of the composition in the register kernels with normals -- 116 -> 121, 170 -> 181
// and 242 -> 254 vector registers, and SGPR spills at KC = 32 (11 in k_knn_reg, 32 in k_knnr_reg); zeroing all nine entries
// in list_cov does not help
template <class EACH>
__device__ __forceinline__ void list_normal(EACH&& each, const int& nr, const double qx, const double qy, const double qz,
                                            const QueryArgs& a, double* out)
{
  double mean[3] = {0.0, 0.0, 0.0};
  each([&](const KdPoint& p) { mean[0] += p.x; mean[1] += p.y; mean[2] += p.z; });
  mean[0] /= nr; mean[1] /= nr; mean[2] /= nr;
  const double sc = 1.0 / nr;
  double z[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  each([&](const KdPoint& p) {
    const double x[3] = {p.x - mean[0], p.y - mean[1], p.z - mean[2]};
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c <= r; c++) z[r][c] += (sc * x[c]) * x[r];
  });
  normal_from_cov(z, qx, qy, qz, a.rx, a.ry, a.rz, out);
}

// ---- kernels ---------------------------------------------------------------------------------------------------
// Every kernel's only parameter is the argument block (q_args); a __global__ function here declares the LDS arrays and
// hands them to its body.
//
// k nearest neighbours (RANGE = false: knn_walk) and k nearest within a radius (RANGE = true: knn_range_walk, and one more
// output: nr_out [n], the length of every list, nullable), one body per list form.  Both end alike: the list as a
// caller-order row (idx and d2, or knn_out for the normals) and, for the normals, list_normal over it.  Under RANGE a list
// may be empty (no point within r2 of a query); list_normal on it gives NaN, calculateNormal's 0 / 0 -- the normals' own
// queries always find themselves, except under k_range_normals' caveat.

// the register-list form: list slot jl is register slot j = k0 + jl
template <int KC, bool NORMALS, bool RANGE>
__device__ __forceinline__ void knn_reg_body(uint4 (*s_stack)[Q_BLOCK])
{
  const QueryArgs& a = q_args();
  LaneQueries<Q_BLOCK> q(a, s_stack);
  ListReg<KC> L;
  const int k = a.k;
  for (; q.i < a.n; q.i += q.T) {
    const size_t i = q.i;
    const double qx = a.x[i], qy = a.y[i], qz = a.z[i];
    const size_t o = a.order ? (size_t)a.order[i] : i;
    // (k0 through an empty asm, per query: as a loop invariant the list's initial values and the slot tests below would be
    // formed once, in SGPRs, and held across the walk -- they spill)
    int k0 = KC - k;
    asm volatile("" : "+v"(k0));
    L.init(k0);
    q.st.sp = 0;
    if (RANGE) knn_range_walk(a, qx, qy, qz, a.r2, L, q.st);
    else knn_walk(a, qx, qy, qz, L, q.st);
    // entries: the slots with a distance >= 0 (kdIndexed.cc:152-156, kd.cc:158-165), which are the first nr -- fewer than k
    // only when the walk met fewer than k points.  (jl through an empty asm per slot, for the reason above.)
    int nr = 0;
#pragma unroll
    for (int j = 0; j < KC; j++) {
      int jl = j - k0;
      asm volatile("" : "+v"(jl));
      nr += (jl >= 0 && L.d[j] >= 0.0) ? 1 : 0;
    }
    if (NORMALS) {
      auto each = [&](auto&& f) {
#pragma unroll
        for (int j = 0; j < KC; j++) {
          int jl = j - k0;
          asm volatile("" : "+v"(jl));
          if (jl >= 0 && jl < nr) f(a.pts[L.s[j]]);
        }
      };
      list_normal(each, nr, qx, qy, qz, a, a.normals + 3 * o);
    }
    if (RANGE && a.nr_out) a.nr_out[o] = nr;
    // (the row after the normal: written first, its loads of the points were kept live across the PCA -- 170 registers
    // instead of 134 at k = 20)
    int32_t* row = NORMALS ? a.knn_out : a.idx;
    row = row ? row + o * k : nullptr;
    double* drow = (!NORMALS && a.d2) ? a.d2 + o * k : nullptr;
#pragma unroll
    for (int j = 0; j < KC; j++) {
      int jl = j - k0;
      asm volatile("" : "+v"(jl));
      if (jl >= 0) {
        const bool v = jl < nr;
        if (row) row[jl] = v ? a.pts[v ? L.s[j] : 0u].orig : -1;     // (an unset slot's point is never loaded)
        if (drow) drow[jl] = v ? L.d[j] : -1.0;
      }
    }
  }
}

template <int KC, bool NORMALS>
__global__ void __launch_bounds__(Q_BLOCK) k_knn_reg(const QueryArgs a_)
{
  __shared__ uint4 s_stack[Q_SD][Q_BLOCK];
  knn_reg_body<KC, NORMALS, false>(s_stack);
}

template <int KC, bool NORMALS>
__global__ void __launch_bounds__(Q_BLOCK) k_knnr_reg(const QueryArgs a_)
{
  __shared__ uint4 s_stack[Q_SD][Q_BLOCK];
  knn_reg_body<KC, NORMALS, true>(s_stack);
}

// the LDS-list form (33 <= k <= 64)
template <bool NORMALS, bool RANGE>
__device__ __forceinline__ void knn_lds_body(uint4 (*s_stack)[Q_BLOCK_L], double (*s_d)[Q_BLOCK_L], uint32_t (*s_s)[Q_BLOCK_L])
{
  const QueryArgs& a = q_args();
  LaneQueries<Q_BLOCK_L> q(a, s_stack);
  ListLds<Q_BLOCK_L> L;
  L.ld = &s_d[0][threadIdx.x];
  L.ls = &s_s[0][threadIdx.x];
  const int k = a.k;
  for (; q.i < a.n; q.i += q.T) {
    const size_t i = q.i;
    const double qx = a.x[i], qy = a.y[i], qz = a.z[i];
    const size_t o = a.order ? (size_t)a.order[i] : i;
    L.init(k);
    q.st.sp = 0;
    if (RANGE) knn_range_walk(a, qx, qy, qz, a.r2, L, q.st);
    else knn_walk(a, qx, qy, qz, L, q.st);
    int nr = 0;
    for (int j = 0; j < k; j++) nr += (L.dist(j) >= 0.0) ? 1 : 0;   // kdIndexed.cc:152-156, kd.cc:158-165
    if (RANGE && a.nr_out) a.nr_out[o] = nr;
    int32_t* row = NORMALS ? a.knn_out : a.idx;
    row = row ? row + o * k : nullptr;
    double* drow = (!NORMALS && a.d2) ? a.d2 + o * k : nullptr;
    for (int j = 0; j < k; j++) {
      const bool v = j < nr;
      if (row) row[j] = v ? a.pts[v ? L.slot(j) : 0u].orig : -1;
      if (drow) drow[j] = v ? L.dist(j) : -1.0;
    }
    if (NORMALS) {
      auto each = [&](auto&& f) { for (int j = 0; j < nr; j++) f(a.pts[L.slot(j)]); };
      list_normal(each, nr, qx, qy, qz, a, a.normals + 3 * o);
    }
  }
}

template <bool NORMALS>
__global__ void __launch_bounds__(Q_BLOCK_L) k_knn_lds(const QueryArgs a_)
{
  __shared__ uint4 s_stack[Q_SD][Q_BLOCK_L];
  __shared__ double s_d[KNN_MAX_K][Q_BLOCK_L];
  __shared__ uint32_t s_s[KNN_MAX_K][Q_BLOCK_L];
  knn_lds_body<NORMALS, false>(s_stack, s_d, s_s);
}

template <bool NORMALS>
__global__ void __launch_bounds__(Q_BLOCK_L) k_knnr_lds(const QueryArgs a_)
{
  __shared__ uint4 s_stack[Q_SD][Q_BLOCK_L];
  __shared__ double s_d[KNN_MAX_K][Q_BLOCK_L];
  __shared__ uint32_t s_s[KNN_MAX_K][Q_BLOCK_L];
  knn_lds_body<NORMALS, true>(s_stack, s_d, s_s);
}

// ---- adaptive-k normals (calculateNormalsAdaptiveKNN) --------------------------------------------------------------
// Every query repeats the whole search for kidx = kmin .. kmax with a fresh list of kidx + 1 slots and an empty stack, runs
// the PCA on each list and stops at the first whose eigenvalues pass adaptive_k_accepts, or at kmax (rules: the header
// comment of query_lane.h).  kidx is a per-lane value.  The two kernels are the two list forms of the k-NN kernels, with their block sizes
// and grids (query_overflow_entries covers both).
// Rows: normals [n][3], k_used [n] (nullable), knn_out [n][kmax + 1] (nullable): the chosen list, -1 behind its nr entries.
//
// ListReg<KC, true>: insert()'s search for pos carries pos through the empty asm of every slot, so that slot j's two
// compares are consumed before slot j - 1's are issued.  Without it the scheduler, in this kernel, issues the compares of
// many slots ahead of their selects, one lane mask in an SGPR pair each: 106 SGPRs and 8 spilled at KC = 32; with it 52 and
// none.  (k_knn_reg keeps the plain form: there the compares stay in order as they are.)

// the register-list form, kmax + 1 <= KC
template <int KC>
__global__ void __launch_bounds__(Q_BLOCK) k_knn_adaptive_reg(const QueryArgs a_)
{
  const QueryArgs& a = q_args();
  __shared__ uint4 s_stack[Q_SD][Q_BLOCK];
  LaneQueries<Q_BLOCK> q(a, s_stack);
  ListReg<KC, true> L;
  // one loop over (query, kidx) steps: a lane whose list passed the test goes on to its next query while its neighbours are
  // still trying longer lists of theirs (as two nested loops the kernel carried two more loop masks beside insert()'s lane
  // masks, and spilled SGPRs at KC = 32)
  int kidx = a.kmin;
  while (q.i < a.n) {
    const size_t i = q.i;
    const double qx = a.x[i], qy = a.y[i], qz = a.z[i];
    // (k0 through an empty asm at every use, as in knn_reg_body: the slot tests stay in vector registers)
    int k0 = KC - (kidx + 1);
    asm volatile("" : "+v"(k0));
    L.init(k0);
    q.st.sp = 0;
    knn_walk(a, qx, qy, qz, L, q.st);
    int nr = 0;
#pragma unroll
    for (int j = 0; j < KC; j++) {
      int jl = j - k0;
      asm volatile("" : "+v"(jl));
      nr += (jl >= 0 && L.d[j] >= 0.0) ? 1 : 0;
    }
    auto each = [&](auto&& f) {
#pragma unroll
      for (int j = 0; j < KC; j++) {
        int jl = j - k0;
        asm volatile("" : "+v"(jl));
        if (jl >= 0 && jl < nr) f(a.pts[L.s[j]]);
      }
    };
    double z[3][3], D[3];
    list_cov(each, nr, z);
    cov_eigen(z, D);
    const int kmax = a.kmax;
    if (!adaptive_k_accepts(D) && kidx < kmax) { ++kidx; continue; }
    const size_t o = a.order ? (size_t)a.order[i] : i;
    orient_normal(z[0][0], z[1][0], z[2][0], qx, qy, qz, a.rx, a.ry, a.rz, a.normals + 3 * o);
    if (a.k_used) a.k_used[o] = kidx;
    if (a.knn_out) {
      int32_t* row = a.knn_out + o * (size_t)(kmax + 1);
#pragma unroll
      for (int j = 0; j < KC; j++) {
        int jl = j - k0;
        asm volatile("" : "+v"(jl));
        if (jl >= 0) {
          const bool v = jl < nr;
          row[jl] = v ? a.pts[v ? L.s[j] : 0u].orig : -1;     // (an unset slot's point is never loaded)
        }
      }
      for (int jl = kidx + 1; jl <= kmax; jl++) row[jl] = -1;
    }
    q.i += q.T;
    kidx = a.kmin;
  }
}

// the LDS-list form (33 <= kmax + 1 <= 64; kmin + 1 may lie below 33), the same loop
__global__ void __launch_bounds__(Q_BLOCK_L) k_knn_adaptive_lds(const QueryArgs a_)
{
  const QueryArgs& a = q_args();
  __shared__ uint4 s_stack[Q_SD][Q_BLOCK_L];
  __shared__ double s_d[KNN_MAX_K][Q_BLOCK_L];
  __shared__ uint32_t s_s[KNN_MAX_K][Q_BLOCK_L];
  LaneQueries<Q_BLOCK_L> q(a, s_stack);
  ListLds<Q_BLOCK_L> L;
  L.ld = &s_d[0][threadIdx.x];
  L.ls = &s_s[0][threadIdx.x];
  int kidx = a.kmin;
  while (q.i < a.n) {
    const size_t i = q.i;
    const double qx = a.x[i], qy = a.y[i], qz = a.z[i];
    const int k = kidx + 1;
    L.init(k);
    q.st.sp = 0;
    knn_walk(a, qx, qy, qz, L, q.st);
    int nr = 0;
    for (int j = 0; j < k; j++) nr += (L.dist(j) >= 0.0) ? 1 : 0;   // kdIndexed.cc:152-156
    auto each = [&](auto&& f) { for (int j = 0; j < nr; j++) f(a.pts[L.slot(j)]); };
    double z[3][3], D[3];
    list_cov(each, nr, z);
    cov_eigen(z, D);
    const int kmax = a.kmax;
    if (!adaptive_k_accepts(D) && kidx < kmax) { ++kidx; continue; }
    const size_t o = a.order ? (size_t)a.order[i] : i;
    orient_normal(z[0][0], z[1][0], z[2][0], qx, qy, qz, a.rx, a.ry, a.rz, a.normals + 3 * o);
    if (a.k_used) a.k_used[o] = kidx;
    if (a.knn_out) {
      int32_t* row = a.knn_out + o * (size_t)(kmax + 1);
      for (int j = 0; j <= kmax; j++) {
        const bool v = j < nr;
        row[j] = v ? a.pts[v ? L.slot(j) : 0u].orig : -1;
      }
    }
    q.i += q.T;
    kidx = a.kmin;
  }
}

// range search, first walk: the length of every list (caller order)
__global__ void __launch_bounds__(Q_BLOCK) k_range_count(const QueryArgs a_)
{
  const QueryArgs& a = q_args();
  __shared__ uint4 s_stack[Q_SD][Q_BLOCK];
  for (LaneQueries<Q_BLOCK> q(a, s_stack); q.i < a.n; q.i += q.T) {
    const size_t i = q.i;
    uint32_t c = 0;
    auto emit = [&](const KdPoint&, uint32_t, double) { ++c; };
    q.st.sp = 0;
    range_walk(a, a.x[i], a.y[i], a.z[i], a.r2, q.st, emit);
    a.counts[a.order ? (size_t)a.order[i] : i] = c;
  }
}

// second walk, the same visits: every list at its offset
__global__ void __launch_bounds__(Q_BLOCK) k_range_fill(const QueryArgs a_)
{
  const QueryArgs& a = q_args();
  __shared__ uint4 s_stack[Q_SD][Q_BLOCK];
  for (LaneQueries<Q_BLOCK> q(a, s_stack); q.i < a.n; q.i += q.T) {
    const size_t i = q.i;
    const size_t o = a.order ? (size_t)a.order[i] : i;
    unsigned long long w = a.offsets[o];
    const unsigned long long end = a.offsets[o + 1];
    auto emit = [&](const KdPoint& p, uint32_t, double md) {
      if (w < end) {       // (the count walk made the same visits: never false)
        a.idx[w] = p.orig;
        if (a.d2) a.d2[w] = md;
      }
      ++w;
    };
    q.st.sp = 0;
    range_walk(a, a.x[i], a.y[i], a.z[i], a.r2, q.st, emit);
  }
}

// calculateNormalsRange: the list has no upper bound and is not stored -- list_normal's two passes over it are two
// identical walks (same visits, same order).  A point normally finds itself (nr >= 1); where it does not -- coordinates so
// large that the box test's |q - c| - h rounds by more than the radius and prunes the point's own leaf, as the reference's
// does -- nr is 0 and the mean is 0 / 0: NaN normals, the reference's calculateNormal on an empty list
__global__ void __launch_bounds__(Q_BLOCK) k_range_normals(const QueryArgs a_)
{
  const QueryArgs& a = q_args();
  __shared__ uint4 s_stack[Q_SD][Q_BLOCK];
  for (LaneQueries<Q_BLOCK> q(a, s_stack); q.i < a.n; q.i += q.T) {
    const size_t i = q.i;
    const double qx = a.x[i], qy = a.y[i], qz = a.z[i];
    const size_t o = a.order ? (size_t)a.order[i] : i;
    int nr = 0;
    bool counted = false;
    auto each = [&](auto&& f) {
      auto emit = [&](const KdPoint& p, uint32_t, double) { f(p); if (!counted) ++nr; };
      q.st.sp = 0;
      range_walk(a, qx, qy, qz, a.r2, q.st, emit);
      counted = true;
    };
    list_normal(each, nr, qx, qy, qz, a, a.normals + 3 * o);
  }
}

// ---- cylinder, box and segment queries ------------------------------------------------------------------------
// first walk of a list query: the length of every list (caller order)
template <int MODE>
__global__ void __launch_bounds__(Q_BLOCK) k_shape_count(const QueryArgs a_)
{
  const QueryArgs& a = q_args();
  __shared__ uint4 s_stack[Q_SD][Q_BLOCK];
  for (LaneQueries<Q_BLOCK> q(a, s_stack); q.i < a.n; q.i += q.T) {
    const size_t i = q.i;
    uint32_t c = 0;
    auto emit = [&](const KdPoint&) { ++c; };
    q.st.sp = 0;
    shape_walk<MODE>(a, a.x[i], a.y[i], a.z[i], a.vx[i], a.vy[i], a.vz[i], q.st, emit);
    a.counts[a.order ? (size_t)a.order[i] : i] = c;
  }
}

// second walk, the same visits: every list at its offset
template <int MODE>
__global__ void __launch_bounds__(Q_BLOCK) k_shape_fill(const QueryArgs a_)
{
  const QueryArgs& a = q_args();
  __shared__ uint4 s_stack[Q_SD][Q_BLOCK];
  for (LaneQueries<Q_BLOCK> q(a, s_stack); q.i < a.n; q.i += q.T) {
    const size_t i = q.i;
    const size_t o = a.order ? (size_t)a.order[i] : i;
    unsigned long long w = a.offsets[o];
    const unsigned long long end = a.offsets[o + 1];
    auto emit = [&](const KdPoint& p) {
      if (w < end) a.idx[w] = p.orig;       // (the count walk made the same visits: never false)
      ++w;
    };
    q.st.sp = 0;
    shape_walk<MODE>(a, a.x[i], a.y[i], a.z[i], a.vx[i], a.vy[i], a.vz[i], q.st, emit);
  }
}

__global__ void __launch_bounds__(Q_BLOCK) k_segment_nearest(const QueryArgs a_)
{
  const QueryArgs& a = q_args();
  __shared__ uint4 s_stack[Q_SD][Q_BLOCK];
  for (LaneQueries<Q_BLOCK> q(a, s_stack); q.i < a.n; q.i += q.T) {
    const size_t i = q.i;
    const size_t o = a.order ? (size_t)a.order[i] : i;
    Segment sg;
    sg.init(a.x[i], a.y[i], a.z[i], a.vx[i], a.vy[i], a.vz[i]);
    const double b0 = __dsqrt_rn(sg.len2) + __dsqrt_rn(a.r2);     // Dist2(p, p0) is Len2(segment_dir), term for term
    double best = b0 * b0;
    uint32_t bslot = 0xFFFFFFFFu;
    q.st.sp = 0;
    segment_nearest_walk(a, sg, q.st, best, bslot);
    const bool found = bslot != 0xFFFFFFFFu;
    a.idx[o] = found ? a.pts[found ? bslot : 0u].orig : -1;
    if (a.d2) a.d2[o] = found ? best : -1.0;
  }
}

// ---- collision detection along a trajectory (the per-item bodies: query_lane.h) ------------------------------------
template <int METHOD>
__global__ void __launch_bounds__(Q_BLOCK) k_collide_mark(const QueryArgs a_)
{
  const QueryArgs& a = q_args();
  __shared__ uint4 s_stack[Q_SD][Q_BLOCK];
  for (LaneQueries<Q_BLOCK> q(a, s_stack); q.i < a.n; q.i += q.T) {
    const size_t i = q.i;
    if (METHOD == 1) collide_sphere_item(a, i, q.st);
    else collide_segment_item(a, i, q.st);
  }
}

__global__ void __launch_bounds__(Q_BLOCK) k_collide_depth_axis(const QueryArgs a_)
{
  const QueryArgs& a = q_args();
  __shared__ uint4 s_stack[Q_SD][Q_BLOCK];
  for (LaneQueries<Q_BLOCK> q(a, s_stack); q.i < a.n; q.i += q.T) collide_depth_axis_item(a, q.i, q.st);
}

// num_colliding: the set bytes of the mask, one atomic per wave
__global__ void __launch_bounds__(256) k_collide_count(const uint8_t* __restrict__ mask, const size_t M,
                                                       unsigned long long* __restrict__ count)
{
  unsigned long long c = 0;
  const size_t T = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += T) c += mask[i] ? 1u : 0u;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += (unsigned long long)__shfl_xor((long long)c, off, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, c);
}

__global__ void __launch_bounds__(256) k_collide_depth_init(unsigned long long* __restrict__ dmin, const size_t M)
{
  const size_t T = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += T)
    dmin[i] = (unsigned long long)__double_as_longlong(1000.0);
}

__global__ void __launch_bounds__(256) k_collide_depth_finish(const unsigned long long* __restrict__ dmin, const size_t M,
                                                              float* __restrict__ dist)
{
  const size_t T = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += T) dist[i] = collide_depth_value(dmin[i]);
}

// ---- radius clustering (the per-item bodies and the argument for the union-find: cluster_lane.h) --------------------
// a.n is the tree's slot count.  The link kernel has the launch shape of the collision kernels; the others are one pass over
// the slots without a walk
__global__ void __launch_bounds__(Q_BLOCK) k_cluster_link(const QueryArgs a_)
{
  const QueryArgs& a = q_args();
  __shared__ uint4 s_stack[Q_SD][Q_BLOCK];
  for (LaneQueries<Q_BLOCK> q(a, s_stack); q.i < a.n; q.i += q.T) cluster_link_item(a, (uint32_t)q.i, q.st);
}

template <int STEP>
__global__ void __launch_bounds__(256) k_cluster_pass(const QueryArgs a)
{
  const size_t T = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += T) {
    if (STEP == 0) cluster_init_item(a, (uint32_t)i);
    else if (STEP == 1) cluster_flatten_item(a, (uint32_t)i);
    else if (STEP == 2) cluster_flag_item(a, (uint32_t)i);
    else cluster_label_item(a, (uint32_t)i);
  }
}

// ---- launchers -------------------------------------------------------------------------------------------------
// the stack overflow area of a launch over n queries, for both block sizes of query_dev.h (the forest's kernels included)
size_t query_overflow_entries(size_t n, uint32_t max_depth)
{
  // a path holds at most max_depth internal nodes, each pushes at most one entry
  const int need = (int)max_depth + 1 - Q_SD;
  if (need <= 0) return 0;
  const size_t lanes = std::max<size_t>((size_t)q_grid(n, Q_BLOCK) * Q_BLOCK, (size_t)q_grid(n, Q_BLOCK_L) * Q_BLOCK_L);
  return lanes * (size_t)need;
}

typedef void (*QueryKernel)(const QueryArgs);

static hipError_t launch_q(QueryKernel kernel, const QueryArgs& a, hipStream_t s, int block = Q_BLOCK)
{
  hipLaunchKernelGGL(kernel, dim3(q_grid(a.n, block)), dim3(block), 0, s, a);
  return hipGetLastError();
}

// the capacity ladder of the three k-NN families: register lists of 4, 10, 20 and 32 slots -- k = 10 (slam6D) and k = 20
// (calc_normals) get lists of exactly their size -- and the LDS list above them; tab: the family's kernels in that order
static hipError_t launch_by_capacity(const QueryKernel (&tab)[5], int k, const QueryArgs& a, hipStream_t s)
{
  const int rung = k <= 4 ? 0 : k <= 10 ? 1 : k <= 20 ? 2 : k <= 32 ? 3 : 4;
  return launch_q(tab[rung], a, s, rung < 4 ? Q_BLOCK : Q_BLOCK_L);
}

hipError_t launch_knn(const QueryArgs& a, bool normals, hipStream_t s)
{
  if (a.k < 1 || a.k > KNN_MAX_K) return hipErrorInvalidValue;
  static const QueryKernel tab[2][5] = {
      {k_knn_reg<4, false>, k_knn_reg<10, false>, k_knn_reg<20, false>, k_knn_reg<32, false>, k_knn_lds<false>},
      {k_knn_reg<4, true>, k_knn_reg<10, true>, k_knn_reg<20, true>, k_knn_reg<32, true>, k_knn_lds<true>}};
  return launch_by_capacity(tab[normals], a.k, a, s);
}

hipError_t launch_knn_range(const QueryArgs& a, bool normals, hipStream_t s)
{
  if (a.k < 1 || a.k > KNN_MAX_K) return hipErrorInvalidValue;
  static const QueryKernel tab[2][5] = {
      {k_knnr_reg<4, false>, k_knnr_reg<10, false>, k_knnr_reg<20, false>, k_knnr_reg<32, false>, k_knnr_lds<false>},
      {k_knnr_reg<4, true>, k_knnr_reg<10, true>, k_knnr_reg<20, true>, k_knnr_reg<32, true>, k_knnr_lds<true>}};
  return launch_by_capacity(tab[normals], a.k, a, s);
}

hipError_t launch_knn_adaptive(const QueryArgs& a, hipStream_t s)
{
  if (a.kmin < 0 || a.kmin > a.kmax || a.kmax + 1 > KNN_MAX_K) return hipErrorInvalidValue;
  static const QueryKernel tab[5] = {k_knn_adaptive_reg<4>, k_knn_adaptive_reg<10>, k_knn_adaptive_reg<20>,
                                     k_knn_adaptive_reg<32>, k_knn_adaptive_lds};
  return launch_by_capacity(tab, a.kmax + 1, a, s);      // by the longest list
}

hipError_t launch_range_count(const QueryArgs& a, hipStream_t s) { return launch_q(k_range_count, a, s); }
hipError_t launch_range_fill(const QueryArgs& a, hipStream_t s) { return launch_q(k_range_fill, a, s); }
hipError_t launch_range_normals(const QueryArgs& a, hipStream_t s) { return launch_q(k_range_normals, a, s); }
hipError_t launch_segment_nearest(const QueryArgs& a, hipStream_t s) { return launch_q(k_segment_nearest, a, s); }

// the count (fill = false) or fill walk of list query `mode` (ShapeMode)
static hipError_t launch_shape(bool fill, int mode, const QueryArgs& a, hipStream_t s)
{
  static const QueryKernel tab[2][4] = {
      {k_shape_count<SHAPE_ALONG_DIR>, k_shape_count<SHAPE_BETWEEN>, k_shape_count<SHAPE_AABB>, k_shape_count<SHAPE_SEGMENT>},
      {k_shape_fill<SHAPE_ALONG_DIR>, k_shape_fill<SHAPE_BETWEEN>, k_shape_fill<SHAPE_AABB>, k_shape_fill<SHAPE_SEGMENT>}};
  if (mode < SHAPE_ALONG_DIR || mode > SHAPE_SEGMENT) return hipErrorInvalidValue;
  return launch_q(tab[fill][mode], a, s);
}
hipError_t launch_shape_count(const QueryArgs& a, int mode, hipStream_t s) { return launch_shape(false, mode, a, s); }
hipError_t launch_shape_fill(const QueryArgs& a, int mode, hipStream_t s) { return launch_shape(true, mode, a, s); }

hipError_t launch_collide_mark(const QueryArgs& a, int cmethod, hipStream_t s)
{
  if (!a.n) return hipSuccess;
  if (cmethod != 1 && cmethod != 2) return hipErrorInvalidValue;
  return launch_q(cmethod == 1 ? k_collide_mark<1> : k_collide_mark<2>, a, s);
}

hipError_t launch_collide_depth_axis(const QueryArgs& a, hipStream_t s)
{
  if (!a.n) return hipSuccess;
  return launch_q(k_collide_depth_axis, a, s);
}

hipError_t launch_collide_count(const uint8_t* mask, size_t M, unsigned long long* count, hipStream_t s)
{
  if (!M) return hipSuccess;
  hipLaunchKernelGGL(k_collide_count, dim3(q_grid(M, 256)), dim3(256), 0, s, mask, M, count);
  return hipGetLastError();
}

hipError_t launch_collide_depth_init(unsigned long long* dmin, size_t M, hipStream_t s)
{
  if (!M) return hipSuccess;
  hipLaunchKernelGGL(k_collide_depth_init, dim3(q_grid(M, 256)), dim3(256), 0, s, dmin, M);
  return hipGetLastError();
}

hipError_t launch_collide_depth_finish(const unsigned long long* dmin, size_t M, float* dist, hipStream_t s)
{
  if (!M) return hipSuccess;
  hipLaunchKernelGGL(k_collide_depth_finish, dim3(q_grid(M, 256)), dim3(256), 0, s, dmin, M, dist);
  return hipGetLastError();
}

// radius clustering: a.n slots.  max_blocks caps the link kernel's grid below q_grid's (0: q_grid's own) -- the result does not
// depend on it; the overflow area is sized for q_grid(a.n), which is never smaller
hipError_t launch_cluster_init(const QueryArgs& a, hipStream_t s)
{
  if (!a.n) return hipSuccess;
  hipLaunchKernelGGL(k_cluster_pass<0>, dim3(q_grid(a.n, 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_cluster_link(const QueryArgs& a, uint32_t max_blocks, hipStream_t s)
{
  if (!a.n) return hipSuccess;
  uint32_t grid = q_grid(a.n, Q_BLOCK);
  if (max_blocks && max_blocks < grid) grid = max_blocks;
  hipLaunchKernelGGL(k_cluster_link, dim3(grid), dim3(Q_BLOCK), 0, s, a);
  return hipGetLastError();
}

// flatten, then (a.cflag zeroed by the caller) the flags of the kept components
hipError_t launch_cluster_flatten(const QueryArgs& a, hipStream_t s)
{
  if (!a.n) return hipSuccess;
  hipLaunchKernelGGL(k_cluster_pass<1>, dim3(q_grid(a.n, 256)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_cluster_pass<2>, dim3(q_grid(a.n, 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

// behind the scan of a.cflag into a.cnum: a.labels, a.cfirst, a.csizes_out
hipError_t launch_cluster_label(const QueryArgs& a, hipStream_t s)
{
  if (!a.n) return hipSuccess;
  hipLaunchKernelGGL(k_cluster_pass<3>, dim3(q_grid(a.n, 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

// counts [n + 1] (counts[n] == 0) -> exclusive 64-bit offsets [n + 1]: offsets[n] is the total
size_t range_scan_temp_bytes(size_t n)
{
  size_t bytes = 0;
  (void)rocprim::exclusive_scan(nullptr, bytes, (const uint32_t*)nullptr, (unsigned long long*)nullptr, 0ull, n + 1,
                                rocprim::plus<unsigned long long>(), (hipStream_t)0);
  return bytes;
}
hipError_t launch_range_scan(const uint32_t* counts, unsigned long long* offsets, size_t n, void* tmp, size_t tmp_bytes,
                             hipStream_t s)
{
  return rocprim::exclusive_scan(tmp, tmp_bytes, counts, offsets, 0ull, n + 1, rocprim::plus<unsigned long long>(), s);
}

}  // namespace tdtk

