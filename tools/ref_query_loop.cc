// The reference's KDtreeIndexed::kNearestNeighbors / fixedRangeSearch and its cylinder, box and segment queries in an OpenMP
// loop over a query batch, timed: the host yardstick of tools/query_bench.py.  Compiled by query_bench.py at run time (g++ -fopenmp -shared); the entry
// points of oracle/_ref/libref3dtk.so arrive as addresses, so no reference header is needed here.
//
// A member function returning std::vector by value is called, under the x86-64 Itanium ABI, with the return slot first and
// `this` second -- which is what a free function `std::vector<size_t> f(const void*, ...)` compiles to, so the symbol is
// called through that type and the returned vector is destroyed here as usual.
#include <omp.h>

#include <chrono>
#include <cmath>
#include <cstddef>
#include <vector>

typedef std::vector<size_t> (*knn_fn)(const void* self, double* p, int k, int thread);
typedef std::vector<size_t> (*range_fn)(const void* self, double* p, double r2, int thread);

// mode 0: kNN with k, mode 1: fixed radius r2.  Returns the wall time in ms; *found = neighbours over all queries.
extern "C" double ref_query_loop(void* fn, const void* tree, const double* q, size_t n, int mode, int k, double r2, int threads,
                                 unsigned long long* found)
{
  unsigned long long tot = 0;
  const auto t0 = std::chrono::steady_clock::now();
#pragma omp parallel for num_threads(threads) schedule(dynamic, 256) reduction(+ : tot)
  for (long i = 0; i < (long)n; i++) {
    double p[3] = {q[3 * i], q[3 * i + 1], q[3 * i + 2]};
    const int th = omp_get_thread_num();
    if (mode == 0) tot += ((knn_fn)fn)(tree, p, k, th).size();
    else tot += ((range_fn)fn)(tree, p, r2, th).size();
  }
  const auto t1 = std::chrono::steady_clock::now();
  *found = tot;
  return std::chrono::duration<double, std::milli>(t1 - t0).count();
}

typedef std::vector<size_t> (*pair_list_fn)(const void* self, double* p, double* v, double maxdist2, int thread);
typedef std::vector<size_t> (*box_fn)(const void* self, double* lo, double* hi, int thread);
typedef size_t (*nearest_fn)(const void* self, double* p, double* p0, double maxdist2, int thread);

// queries of two vectors.  mode 2: fixedRangeSearchAlongDir / fixedRangeSearchBetween2Points / segmentSearch_all (a list,
// maxdist2), mode 3: AABBSearch, mode 4: segmentSearch_1NearestPoint (*found = queries with an answer)
extern "C" double ref_pair_query_loop(void* fn, const void* tree, const double* p, const double* v, size_t n, int mode,
                                      double maxdist2, int threads, unsigned long long* found)
{
  unsigned long long tot = 0;
  const auto t0 = std::chrono::steady_clock::now();
#pragma omp parallel for num_threads(threads) schedule(dynamic, 256) reduction(+ : tot)
  for (long i = 0; i < (long)n; i++) {
    double a[3] = {p[3 * i], p[3 * i + 1], p[3 * i + 2]};
    double b[3] = {v[3 * i], v[3 * i + 1], v[3 * i + 2]};
    const int th = omp_get_thread_num();
    if (mode == 2) tot += ((pair_list_fn)fn)(tree, a, b, maxdist2, th).size();
    else if (mode == 3) tot += ((box_fn)fn)(tree, a, b, th).size();
    else tot += ((nearest_fn)fn)(tree, a, b, maxdist2, th) != (size_t)-1 ? 1 : 0;
  }
  const auto t1 = std::chrono::steady_clock::now();
  *found = tot;
  return std::chrono::duration<double, std::milli>(t1 - t0).count();
}

// ---- collision_model's loops (handle_pointcloud CTYPE1 / CTYPE2, calculate_collidingdist2) over the same entry points ----
// restated from their description in include/tdtk_hip.h; parallel over what the program parallelises (frames, or model
// points for the segments), with its critical section around the depth updates.  Frames are column-major 4x4.
static inline void move3(const double* T, const double* m, double* o)
{
  const double x = m[0] * T[0] + m[1] * T[4] + m[2] * T[8];
  const double y = m[0] * T[1] + m[1] * T[5] + m[2] * T[9];
  const double z = m[0] * T[2] + m[1] * T[6] + m[2] * T[10];
  o[0] = x + T[12]; o[1] = y + T[13]; o[2] = z + T[14];
}

// cmethod 1: range_f = fixedRangeSearch; cmethod 2: list_f = segmentSearch_all.  mask [M] bytes, zeroed by the caller.
extern "C" double ref_collision_mark_loop(void* range_f, void* list_f, const void* tree, const double* model, size_t P,
                                          const double* frames, size_t F, double r2, int cmethod, int threads,
                                          unsigned char* mask)
{
  const auto t0 = std::chrono::steady_clock::now();
  if (cmethod == 1) {
#pragma omp parallel for num_threads(threads) schedule(dynamic)
    for (long j = 0; j < (long)F; j++) {
      const int th = omp_get_thread_num();
      for (size_t m = 0; m < P; m++) {
        double p[3];
        move3(frames + 16 * j, model + 3 * m, p);
        for (size_t k : ((range_fn)range_f)(tree, p, r2, th)) mask[k] = 1;
      }
    }
  } else {
#pragma omp parallel for num_threads(threads) schedule(dynamic)
    for (long m = 0; m < (long)P; m++) {
      const int th = omp_get_thread_num();
      double p1[3], p2[3];
      move3(frames, model + 3 * m, p1);
      for (size_t j = 1; j < F; j++) {
        move3(frames + 16 * j, model + 3 * m, p2);
        for (size_t k : ((pair_list_fn)list_f)(tree, p1, p2, r2, th)) mask[k] = 1;
        p1[0] = p2[0]; p1[1] = p2[1]; p1[2] = p2[2];
      }
    }
  }
  const auto t1 = std::chrono::steady_clock::now();
  return std::chrono::duration<double, std::milli>(t1 - t0).count();
}

// tree over the colliding points pts [n][3]; dist [n] floats
extern "C" double ref_collision_depth_axis_loop(void* near_f, void* range_f, const void* tree, const double* pts, size_t n,
                                                const double* model, size_t P, const double* frames, size_t F, double r2,
                                                int threads, float* dist)
{
  const auto t0 = std::chrono::steady_clock::now();
  for (size_t i = 0; i < n; i++) dist[i] = 1000.0f;
#pragma omp parallel for num_threads(threads) schedule(dynamic)
  for (long j = 0; j < (long)F; j++) {
    const int th = omp_get_thread_num();
    for (size_t m = 0; m < P; m++) {
      const double axis[3] = {0.0, model[3 * m + 1], 0.0};
      double p1[3], p2[3];
      move3(frames + 16 * j, model + 3 * m, p1);
      move3(frames + 16 * j, axis, p2);
      const size_t c1 = ((nearest_fn)near_f)(tree, p1, p2, r2, th);
      if (c1 == (size_t)-1) continue;
      double c[3] = {pts[3 * c1], pts[3 * c1 + 1], pts[3 * c1 + 2]};
      const double dx = c[0] - p1[0], dy = c[1] - p1[1], dz = c[2] - p1[2];
      const double d2 = dx * dx + dy * dy + dz * dz;
      const std::vector<size_t> sphere = ((range_fn)range_f)(tree, c, r2, th);
#pragma omp critical
      for (size_t k : sphere)
        if (d2 < dist[k]) dist[k] = (float)d2;
    }
  }
  for (size_t i = 0; i < n; i++) dist[i] = std::sqrt(dist[i]);
  const auto t1 = std::chrono::steady_clock::now();
  return std::chrono::duration<double, std::milli>(t1 - t0).count();
}
