// The device scaffold of the one-query-per-lane kernels over the kd-trees: query.hip and forest.hip.  The block sizes, the
// LDS stack levels and the grid cap, the argument block behind the kernarg segment pointer, the lane stack's set-up, the
// opening of a kernel's grid-stride loop, and the grid of a launch.  One set of each: query_overflow_entries (query.hip)
// sizes the overflow area of the lane stack from these constants for every kernel of both files.
#pragma once
#include <hip/hip_runtime.h>

#include "lane_stack.h"
#include "query_args.h"

namespace tdtk {

constexpr int Q_BLOCK = 128;     // register-list and range kernels
constexpr int Q_SD = 16;         // LDS stack levels (16 bytes each): 32 KB per 128-lane workgroup
constexpr int Q_BLOCK_L = 64;    // the LDS-list k-NN kernels: 64 lanes x 64 slots x 12 bytes = 48 KB + 16 KB of stack
constexpr int Q_MAX_BLOCKS = 2048;   // grid-stride cap (256 CUs x 8); the overflow area is sized for it

// The argument block read through the kernarg segment pointer (as kernels.hip's kernarg_block): behind an opaque pointer of
// the constant address space its fields are s_load'ed where they are used instead of being held in SGPRs across the walk
// (the register lists leave no room for that), and a table in it that a loop counter indexes (ForestArgs::slot) is not
// copied to scratch as it would be behind a by-value parameter.  The block is every kernel's only parameter.
template <class ARGS = QueryArgs>
__device__ __forceinline__ const ARGS& q_args()
{
  typedef const ARGS __attribute__((address_space(4))) * kernarg_ptr;
  kernarg_ptr p = (kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return *(const ARGS*)p;
}

template <int BLOCK>
__device__ __forceinline__ void stack_init(LaneStackQ<BLOCK, Q_SD>& st, uint4 (*lds)[BLOCK], const QueryArgs& a)
{
  st.l_e = &lds[0][threadIdx.x];
  st.g_m2 = a.ovf_m2;
  st.g_ref = a.ovf_ref;
  st.gcol = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  st.gstride = (size_t)gridDim.x * BLOCK;
  st.sp = 0;
}

// the opening of every kernel: the lane's stack and its grid-stride position i over the sorted queries (step T).  The loop
// itself stays in the kernel, for (LaneQueries<B> q(a, s_stack); q.i < a.n; q.i += q.T): handed over as a lambda the same
// body costs two to six vector registers in most kernels ("layout of the query code")
template <int BLOCK>
struct LaneQueries {
  LaneStackQ<BLOCK, Q_SD> st;
  size_t i, T;
  __device__ __forceinline__ LaneQueries(const QueryArgs& a, uint4 (*lds)[BLOCK])
  {
    stack_init<BLOCK>(st, lds, a);
    T = (size_t)gridDim.x * BLOCK;
    i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  }
};

static inline uint32_t q_grid(size_t n, int block)
{
  const size_t nb = (n + block - 1) / block;
  return (uint32_t)(nb < (size_t)Q_MAX_BLOCKS ? (nb ? nb : 1) : Q_MAX_BLOCKS);
}

}  // namespace tdtk
