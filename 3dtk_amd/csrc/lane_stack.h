// Per-lane DFS stack of the one-query-per-lane tree walks, shared by kernels.hip (the k_search family) and query.hip (the
// k-NN and fixed-radius walks): its overflow path and the 16-byte-entry form LaneStackQ.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace tdtk {

// The overflow path lives in its own (rarely called) functions.  They name their address space (global) in every access,
// so they could be inlined without the compiler merging LDS and global accesses into flat ones -- round 4 measured both
// inlined forms (a per-lane branch; a wave-uniform branch around it): the 32 bytes of scratch per lane that the call frame
// costs every search kernel are gone then, and k_search of the 1M-vs-1M loop takes 0.2008-0.2028 ms instead of
// 0.1937-0.1946 (driver's arguments, gpurun_out/r4h, r4i).  Out of line it stays.
#define TDTK_OVF_INLINE __noinline__
__device__ TDTK_OVF_INLINE void stack_spill(double* g_m2, uint32_t* g_ref, size_t off, uint32_t ref, double m2)
{
  typedef double __attribute__((address_space(1))) * gd;
  typedef uint32_t __attribute__((address_space(1))) * gu;
  ((gd)g_m2)[off] = m2;
  ((gu)g_ref)[off] = ref;
}
__device__ TDTK_OVF_INLINE void stack_fill(const double* g_m2, const uint32_t* g_ref, size_t off, uint32_t& ref,
                                           double& m2)
{
  typedef const double __attribute__((address_space(1))) * gd;
  typedef const uint32_t __attribute__((address_space(1))) * gu;
  m2 = ((gd)g_m2)[off];
  ref = ((gu)g_ref)[off];
}

// The same stack with 16-byte entries { myd^2, far child, - }: one ds_write_b128 / ds_read_b128 and one address per push /
// pop instead of two of each (the persistent-lane kernel, round 3).  8 KB of LDS per 128-thread workgroup at SD = 4.
template <int BLOCK, int SD>
struct LaneStackQ {
  uint4* l_e;      // &lds_e[0][lane]
  double* g_m2;    // overflow area (wave-uniform base), may be null when the tree is shallow ...
  uint32_t* g_ref;
  size_t gcol;     // ... and this lane's column in it (round 6: kept apart -- as two per-lane pointers they were four vector
                   // registers live across the whole kernel for a path hardly ever taken; a column is one, or none)
  size_t gstride;
  int sp;
  __device__ __forceinline__ void push(uint32_t ref, double m2)
  {
    // (the overflow path behind a wave-uniform branch: the common case -- no lane of the wave beyond the LDS levels -- is a
    // scalar jump over it, not code every lane steps through with an empty mask)
    if (__builtin_expect(__ballot(sp >= SD) == 0ull, 1)) {
      l_e[sp * BLOCK] = make_uint4((uint32_t)__double2loint(m2), (uint32_t)__double2hiint(m2), ref, 0u);
    } else {
      if (sp < SD) l_e[sp * BLOCK] = make_uint4((uint32_t)__double2loint(m2), (uint32_t)__double2hiint(m2), ref, 0u);
      else stack_spill(g_m2, g_ref, (size_t)(sp - SD) * gstride + gcol, ref, m2);
    }
    ++sp;
  }
  __device__ __forceinline__ void top(uint32_t& ref, double& m2) const
  {
    const int s = sp;
    if (__builtin_expect(__ballot(s >= SD) == 0ull, 1)) {
      const uint4 e = l_e[s * BLOCK];
      m2 = __hiloint2double((int)e.y, (int)e.x);
      ref = e.z;
    } else if (s < SD) {
      const uint4 e = l_e[s * BLOCK];
      m2 = __hiloint2double((int)e.y, (int)e.x);
      ref = e.z;
    } else {
      stack_fill(g_m2, g_ref, (size_t)(s - SD) * gstride + gcol, ref, m2);
    }
  }
};

}  // namespace tdtk
