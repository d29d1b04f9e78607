// The reference's KDtreeIndexed::kNearestNeighbors / fixedRangeSearch and its cylinder, box and segment queries in an OpenMP
// loop over a query batch, timed: the host yardstick of tools/query_bench.py.  Compiled by query_bench.py at run time (g++ -fopenmp -shared); the entry
// points of oracle/_ref/libref3dtk.so arrive as addresses, so no reference header is needed here.
//
// A member function returning std::vector by value is called, under the x86-64 Itanium ABI, with the return slot first and
// `this` second -- which is what a free function `std::vector<size_t> f(const void*, ...)` compiles to, so the symbol is
// called through that type and the returned vector is destroyed here as usual.
#include <omp.h>

#include <chrono>
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
