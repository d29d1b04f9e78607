// TEST INFRASTRUCTURE: a C handle over the reference's own KDtree (pointer flavour, kd.cc) and its kNearestRangeSearch
// (kd.cc:137-171).  Built by oracle/build_ref.sh next to the reference's kd.cc into oracle/_ref/libref_kd.so, or by
// tests/golden/make_golden_knn_range.py into a temporary directory; loaded through ctypes (RefKD there).
//
// kd.o's only undefined reference-side symbol is SearchTree's typeinfo, which the compiler emits with the first out-of-line
// virtual of the class: the three of them (searchTree.h:83-112) get empty bodies here, so the library links with
// --no-undefined and shares no symbol with libref3dtk.so.
#include <vector>
#include "slam6d/kd.h"

double* SearchTree::FindClosestAlongDir(double*, double*, double, int) const { return 0; }
void SearchTree::getPtPairs(std::vector<PtPair>*, double*, double* const*, unsigned int, unsigned int, int, int, double,
                            double&, double*, double*) {}
void SearchTree::getPtPairs(std::vector<PtPair>*, double*, const DataXYZ&, const DataNormal&, unsigned int, unsigned int, int,
                            int, double, double&, double*, double*, PairingMode) {}

struct Handle {
  std::vector<double> xyz;
  std::vector<double*> ptrs;
  KDtree* tree;
};

extern "C" void* kr_create(const double* xyz, int n, int bucket)
{
  Handle* h = new Handle;
  h->xyz.assign(xyz, xyz + 3 * (size_t)n);
  h->ptrs.resize(n);
  for (int i = 0; i < n; i++) h->ptrs[i] = &h->xyz[3 * (size_t)i];
  h->tree = new KDtree(h->ptrs.data(), n, bucket);
  return h;
}

extern "C" void kr_destroy(void* p)
{
  Handle* h = (Handle*)p;
  delete h->tree;
  delete h;
}

// out [nq][k][3] (untouched behind a row's entries), counts [nq]
extern "C" void kr_search(void* p, const double* q, int nq, int k, double r2, double* out, int* counts)
{
  Handle* h = (Handle*)p;
  for (int i = 0; i < nq; i++) {
    double qq[3] = {q[3 * i], q[3 * i + 1], q[3 * i + 2]};
    std::vector<Point> r = h->tree->kNearestRangeSearch(qq, k, r2, 0);
    counts[i] = (int)r.size();
    for (size_t j = 0; j < r.size(); j++) {
      double* o = out + 3 * ((size_t)i * k + j);
      o[0] = r[j].x; o[1] = r[j].y; o[2] = r[j].z;
    }
  }
}
