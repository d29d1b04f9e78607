// The per-lane code of the voxel-grid entry points (tdtk_voxel_walk, tdtk_peopleremover; kernels in voxel.hip): the
// reference's free-space carving, src/peopleremover/common.cc and peopleremover.cc, restated so that every voxel list and
// every mask is the reference's bit for bit.  Like query_lane.h a host compiler reads this file (tests/host_lane_shim.h
// defines __device__ / __forceinline__ away; the driver adds __popcll): tests/test_peopleremover_host.py runs it that way.
//
// Voxels.  voxel_of_point (common.cc:29-54) is py_div per axis: the truncated quotient a / b, corrected by the sign of
// fmod(a, b) -- not floor(a / b), which differs where the division rounds up to an integer.  Three coordinates in
// (-2^20 + 4, 2^20 - 4) are biased by 2^20 and packed into one 64-bit key in BRICK-MAJOR order: the upper 19 bits of x, y, z
// (the 4 x 4 x 4 brick), then the lower 2 bits of each (the voxel inside the brick, 6 bits).  Sorting the keys therefore
// lays the voxels of a brick next to each other in the order of their bit in the brick's 64-bit occupancy word, and a
// voxel's index in the compact array is base(brick) + popcount(word below its bit).
//
// Membership.  An open-addressing table (linear probing, at most half full) maps a brick key to { word, base }.  A lane keeps
// the last brick it looked up in registers (BrickCache): a ray that stays inside a brick for several steps, or crosses a
// brick that does not exist -- the empty space in front of the scanner, most of every ray -- pays one probe per brick.
//
// The walk.  vox_walk is walk_voxels (common.cc:112-306) line by line; the comments name the lines a restatement gets
// wrong.  All of it is fp64 in the reference's order of operations, compiled without contraction: tMax is advanced as
// tMaxStart + mult * tDelta, two roundings from exact operands each time (mult < 2^22 is exact as a double, tMaxStart and
// tDelta are the values the reference holds), so the t at which an axis steps is the reference's double and the
// comparisons minVal == tMax decide the same axes.
#pragma once
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define VOX_HD __host__ __device__ __forceinline__      // the key arithmetic: api_voxel.cpp decodes the free voxels' keys
#else
#define VOX_HD __device__ __forceinline__
#endif

namespace tdtk {

constexpr int64_t VOX_BIAS = 1 << 20;
constexpr double VOX_LIMIT = (double)((1 << 20) - 4);    // |a / b| of every input coordinate stays below: the walk's +-1
                                                          // adjustments and the +-2 neighbourhoods stay inside 21 bits
constexpr uint64_t VOX_EMPTY = ~0ull;                     // no brick key: a key has 57 bits
enum { VOX_ERR_NONFINITE = 1u, VOX_ERR_RANGE = 2u, VOX_ERR_TOTAL = 4u };

// 0, or the VOX_ERR_* bit of a coordinate no voxel can be made of
__device__ __forceinline__ uint32_t vox_coord_err(const double a, const double vs)
{
  if (!std::isfinite(a)) return VOX_ERR_NONFINITE;
  return (fabs(a / vs) < VOX_LIMIT) ? 0u : VOX_ERR_RANGE;
}

// common.cc:29-37
__device__ __forceinline__ int64_t vox_py_div(const double a, const double b)
{
  int64_t q = (int64_t)(a / b);
  const double r = fmod(a, b);
  if ((r != 0) && ((r < 0) != (b < 0))) q -= 1;
  return q;
}

// common.cc:39-46
__device__ __forceinline__ double vox_py_mod(const double a, const double b)
{
  double r = fmod(a, b);
  if (r != 0 && ((r < 0) != (b < 0))) r += b;
  return r;
}

VOX_HD uint64_t vox_key(const int64_t x, const int64_t y, const int64_t z)
{
  const uint64_t ux = (uint64_t)(x + VOX_BIAS), uy = (uint64_t)(y + VOX_BIAS), uz = (uint64_t)(z + VOX_BIAS);
  return ((ux >> 2) << 44) | ((uy >> 2) << 25) | ((uz >> 2) << 6) | ((ux & 3u) << 4) | ((uy & 3u) << 2) | (uz & 3u);
}

VOX_HD void vox_unkey(const uint64_t k, int64_t& x, int64_t& y, int64_t& z)
{
  x = (int64_t)((((k >> 44) & 0x7FFFFu) << 2) | ((k >> 4) & 3u)) - VOX_BIAS;
  y = (int64_t)((((k >> 25) & 0x7FFFFu) << 2) | ((k >> 2) & 3u)) - VOX_BIAS;
  z = (int64_t)((((k >> 6) & 0x7FFFFu) << 2) | (k & 3u)) - VOX_BIAS;
}

__device__ __forceinline__ uint64_t vox_key_of_point(const double* p, const double vs)
{
  return vox_key(vox_py_div(p[0], vs), vox_py_div(p[1], vs), vox_py_div(p[2], vs));
}

struct alignas(32) VoxBrick {
  uint64_t key;      // VOX_EMPTY: free slot
  uint64_t word;     // bit b: the voxel with low key bits b exists
  uint32_t base;     // compact index of the brick's first voxel
  uint32_t pad[3];
};

// the occupancy of a call: the brick table in front of the compact voxel array and its CSR of ascending scan ids
struct VoxGrid {
  const VoxBrick* table;
  uint32_t mask;             // slots - 1, slots a power of two >= 2 * bricks
  const uint32_t* vstart;    // [voxels + 1] into pscan
  const uint32_t* pscan;     // [pairs] the unique (voxel, scan) pairs: scan ids, ascending inside a voxel
  const uint64_t* vkey;      // [voxels] ascending
  uint32_t n_vox;
};

struct BrickCache {
  uint64_t key = VOX_EMPTY, word = 0;
  uint32_t base = 0;
};

__device__ __forceinline__ uint64_t vox_hash(uint64_t k)
{
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

// the compact index of the voxel with this key, -1 if no point lies in it
__device__ __forceinline__ int32_t vox_lookup(const VoxGrid& g, BrickCache& c, const uint64_t key)
{
  const uint64_t bk = key >> 6;
  if (bk != c.key) {
    c.key = bk; c.word = 0; c.base = 0;
    uint32_t h = (uint32_t)vox_hash(bk) & g.mask;
    for (;;) {                                       // ends: the table is at most half full
      const uint64_t k = g.table[h].key;
      if (k == bk) { c.word = g.table[h].word; c.base = g.table[h].base; break; }
      if (k == VOX_EMPTY) break;
      h = (h + 1u) & g.mask;
    }
  }
  const uint32_t bit = (uint32_t)key & 63u;
  if (!((c.word >> bit) & 1ull)) return -1;
  return (int32_t)(c.base + (uint32_t)__popcll(c.word & ((1ull << bit) - 1ull)));
}

// f(u) for every occupied voxel u != v within Chebyshev distance `radius` of the voxel with key `key`
template <class F>
__device__ __forceinline__ void vox_neighbours(const VoxGrid& g, const uint64_t key, const int radius, F&& f)
{
  int64_t x, y, z;
  vox_unkey(key, x, y, z);
  BrickCache c;
  for (int i = -radius; i <= radius; ++i)
    for (int j = -radius; j <= radius; ++j)
      for (int k = -radius; k <= radius; ++k) {      // z innermost: neighbouring probes share a brick
        if (i == 0 && j == 0 && k == 0) continue;
        const int32_t u = vox_lookup(g, c, vox_key(x + i, y + j, z + k));
        if (u >= 0) f((uint32_t)u);
      }
}

// ---- walk_voxels, common.cc:112-306 ----------------------------------------------------------------------------------
// visit(x, y, z) -> bool is the reference's visitor; its result is ignored for the first two calls (lines 132 and 195).
template <class V>
__device__ __forceinline__ void vox_walk(const double* sp, const double* ep, const double vs, V& visit)
{
  const double inf = INFINITY;
  double dir[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) dir[a] = ep[a] - sp[a];
  if (dir[0] == 0 && dir[1] == 0 && dir[2] == 0) return;          // :124 a zero-length ray visits nothing
  int64_t sv[3], cv[3], ev[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) { sv[a] = vox_py_div(sp[a], vs); cv[a] = sv[a]; ev[a] = vox_py_div(ep[a], vs); }
  (void)visit(sv[0], sv[1], sv[2]);                                // :132
  if (sv[0] == ev[0] && sv[1] == ev[1] && sv[2] == ev[2]) return;
  double tDelta[3], tMax[3], maxMult[3];
  int step[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (dir[a] == 0) {
      tDelta[a] = 0; step[a] = 0; tMax[a] = inf; maxMult[a] = inf;
    } else {
      step[a] = dir[a] > 0 ? 1 : -1;
      tDelta[a] = (double)step[a] * vs / dir[a];
      tMax[a] = tDelta[a] * (1.0 - vox_py_mod((double)step[a] * (sp[a] / vs), 1.0));
      maxMult[a] = (double)((ev[a] - sv[a]) * step[a]);
      // :155 a negative step that starts exactly on a boundary: the start voxel moves too
      if (step[a] == -1 && tMax[a] == tDelta[a] && sv[a] != ev[a]) { cv[a] -= 1; sv[a] -= 1; maxMult[a] -= 1; }
    }
  }
  (void)visit(cv[0], cv[1], cv[2]);                                // :195
  if (cv[0] == ev[0] && cv[1] == ev[1] && cv[2] == ev[2]) return;
  const bool mixed = (step[0] == 1 || step[1] == 1 || step[2] == 1) && (step[0] == -1 || step[1] == -1 || step[2] == -1);
  uint32_t mult[3] = {0u, 0u, 0u};        // size_t in the reference; below 2^22 here, the same double
  double tMaxStart[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) tMaxStart[a] = tMax[a];
  for (;;) {
    double minVal = tMax[1] < tMax[0] ? tMax[1] : tMax[0];         // std::min
    minVal = tMax[2] < minVal ? tMax[2] : minVal;
    bool st[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      st[a] = (minVal == tMax[a]);
      if (st[a]) {
        mult[a] += 1u;
        cv[a] = sv[a] + (int64_t)mult[a] * step[a];
        tMax[a] = tMaxStart[a] + (double)mult[a] * tDelta[a];       // two roundings, no accumulation, no FMA
      }
    }
    // Not in the reference: an iteration in which no axis with a direction steps changes nothing the exits below read, so
    // the reference would loop forever from here (a tMax that is NaN: a denormal direction across a boundary gives
    // tDelta = inf and inf * 0).  A kernel must end; every walk the reference finishes never takes this exit.
    if (!((st[0] && step[0] != 0) || (st[1] && step[1] != 0) || (st[2] && step[2] != 0))) break;
    if (((st[0] && st[1]) || (st[1] && st[2]) || (st[0] && st[2])) && mixed) {      // :244 the graced voxel
      int64_t av[3] = {cv[0], cv[1], cv[2]};
      bool out = false;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        if (out || !st[a]) continue;
        if (step[a] < 0) {
          if ((double)mult[a] > maxMult[a] + 1) out = true;
          else av[a] += 1;
        } else if ((double)mult[a] > maxMult[a]) out = true;
      }
      if (out) break;
      if (!visit(av[0], av[1], av[2])) break;
    }
    if (st[0] && (double)mult[0] > maxMult[0]) break;              // :291 before the visit of cur_voxel
    if (st[1] && (double)mult[1] > maxMult[1]) break;
    if (st[2] && (double)mult[2] > maxMult[2]) break;
    if (!visit(cv[0], cv[1], cv[2])) break;
  }
}

// ---- visitor, common.cc:57-103 ---------------------------------------------------------------------------------------
// lo .. hi: the window of scan ids around the current one ([current - diff, current + diff], lower end clamped to 0; with
// diff == 0 the id itself).  A free mark is a plain byte store of 1: idempotent, no atomic.
struct VoxCarve {
  const VoxGrid& g;
  unsigned char* free_mark;
  uint32_t lo, hi;
  BrickCache c;
  uint32_t visits;
  __device__ __forceinline__ bool operator()(const int64_t x, const int64_t y, const int64_t z)
  {
    ++visits;
    const int32_t v = vox_lookup(g, c, vox_key(x, y, z));
    if (v < 0) return true;                       // no points at all: go on, nothing to mark
    const uint32_t p1 = g.vstart[v + 1];
    for (uint32_t p = g.vstart[v]; p < p1; ++p) {  // lower_bound(window_start), then <= current + diff
      const uint32_t s = g.pscan[p];
      if (s >= lo) {
        if (s <= hi) return false;
        break;
      }
    }
    free_mark[v] = 1;
    return true;
  }
};

__device__ __forceinline__ void vox_window(const uint64_t current, const uint64_t diff, uint32_t& lo, uint32_t& hi)
{
  const uint64_t h = current + (diff < 0xFFFFFFFFull ? diff : 0xFFFFFFFFull);
  lo = diff > current ? 0u : (uint32_t)(current - diff);
  hi = h > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)h;
}

// the visitor of tdtk_voxel_walk: always continues; counts, and lists where out is given
struct VoxList {
  int32_t* out;      // [.][3] at this ray's offset, or null
  uint32_t visits;
  __device__ __forceinline__ bool operator()(const int64_t x, const int64_t y, const int64_t z)
  {
    if (out) { out[3 * (size_t)visits] = (int32_t)x; out[3 * (size_t)visits + 1] = (int32_t)y; out[3 * (size_t)visits + 2] = (int32_t)z; }
    ++visits;
    return true;
  }
};

// ---- half-free voxels and classification, peopleremover.cc:420-468 and :534-545 -----------------------------------------
// half_voxels[w] is the union of occupied[v] over the free voxels v within distance 2 of w, for w occupied and not free.
// So a (voxel, scan) pair of the occupancy is dynamic if its voxel is free, or -- with subvoxel accuracy -- a free voxel
// within distance 2 holds that scan id.  Returns whether w is a half-free voxel (the count the reference prints).
__device__ __forceinline__ bool vox_classify_voxel(const VoxGrid& g, const unsigned char* free_mark, const bool subvoxel,
                                                   const uint32_t w, unsigned char* pdyn)
{
  const uint32_t p0 = g.vstart[w], p1 = g.vstart[w + 1];
  const unsigned char is_free = free_mark[w];
  for (uint32_t p = p0; p < p1; ++p) pdyn[p] = is_free;
  if (is_free || !subvoxel) return false;
  bool half = false;
  vox_neighbours(g, g.vkey[w], 2, [&](const uint32_t u) {
    if (!free_mark[u]) return;
    half = true;
    uint32_t q = g.vstart[u];
    const uint32_t q1 = g.vstart[u + 1];
    for (uint32_t p = p0; p < p1 && q < q1; ++p) {          // both lists ascend
      const uint32_t s = g.pscan[p];
      while (q < q1 && g.pscan[q] < s) ++q;
      if (q < q1 && g.pscan[q] == s) pdyn[p] = 1;
    }
  });
  return half;
}

// a point of scan `scan` in the voxel with this key (which exists: the point made it)
__device__ __forceinline__ unsigned char vox_classify_point(const VoxGrid& g, const uint64_t key, const uint32_t scan,
                                                            const unsigned char* pdyn)
{
  BrickCache c;
  const int32_t v = vox_lookup(g, c, key);
  if (v < 0) return 0;
  const uint32_t p1 = g.vstart[v + 1];
  for (uint32_t p = g.vstart[v]; p < p1; ++p)
    if (g.pscan[p] == scan) return pdyn[p];
  return 0;
}

}  // namespace tdtk
