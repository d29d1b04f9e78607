"""The k-NN walk and the fixed-radius walk of the query kernels (knn_walk, range_walk: 3dtk_amd/csrc/query_lane.h) compiled
for the host and run on kd_build.cpp's host tree: their rows and lists against tests/golden/k8_kdtree_queries.npz, the
reference's KDtreeIndexed::kNearestNeighbors and fixedRangeSearch, entry for entry."""
import ctypes as C
import importlib.util
import os

import numpy as np

import host_lane

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")

_HOST_WALKS = r"""
extern "C" void hq_knn(void* p, const double* q, int nq, int k, int* idx) {
  HostTree& T = *(HostTree*)p;
  QueryArgs a = host_args(T);
  std::vector<double> ld(KNN_MAX_K); std::vector<uint32_t> ls(KNN_MAX_K);
  for (int i = 0; i < nq; i++) {
    ListLds<1> L; L.ld = ld.data(); L.ls = ls.data(); L.init(k);
    HostStack st;
    knn_walk(a, q[3 * i], q[3 * i + 1], q[3 * i + 2], L, st);
    for (int j = 0; j < k; j++) idx[i * k + j] = L.dist(j) >= 0.0 ? a.pts[L.slot(j)].orig : -1;
  }
}
// the list of query i at idx + off[i]; returns the total (idx may be null: the count walk)
extern "C" size_t hq_range(void* p, const double* q, int nq, double r2, unsigned long long* off, int* idx) {
  HostTree& T = *(HostTree*)p;
  QueryArgs a = host_args(T);
  size_t w = 0;
  for (int i = 0; i < nq; i++) {
    off[i] = w;
    auto emit = [&](const KdPoint& pt, uint32_t, double) { if (idx) idx[w] = pt.orig; ++w; };
    HostStack st;
    range_walk(a, q[3 * i], q[3 * i + 1], q[3 * i + 2], r2, st, emit);
  }
  off[nq] = w;
  return w;
}
"""


def _mg():
    spec = importlib.util.spec_from_file_location("make_golden_knn", os.path.join(G, "make_golden_knn.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    return mg


def test_knn_and_range_walks_compiled_for_the_host_equal_the_fixture(tmp_path):
    mg = _mg()
    z = np.load(os.path.join(G, "k8_kdtree_queries.npz"))
    L = host_lane.build(_HOST_WALKS, tmp_path, "hq")
    L.hq_knn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.hq_range.restype = C.c_size_t
    L.hq_range.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
    n = 0
    for name in mg.k8_clouds():
        pts, Q, r2 = np.ascontiguousarray(z[name + "_pts"]), np.ascontiguousarray(z[name + "_q"]), float(z[name + "_r2"][0])
        for b in mg.BUCKETS:
            h = L.host_tree_create(pts.ctypes.data, len(pts), b)
            assert h
            for k in mg.KS:
                idx = np.empty((len(Q), k), np.int32)
                L.hq_knn(h, Q.ctypes.data, len(Q), k, idx.ctypes.data)
                assert np.array_equal(idx, z["%s_b%d_knn%d" % (name, b, k)]), (name, b, k)
                n += 1
            want_off, want_idx = z["%s_b%d_roff" % (name, b)], z["%s_b%d_ridx" % (name, b)]
            off = np.empty(len(Q) + 1, np.uint64)
            total = L.hq_range(h, Q.ctypes.data, len(Q), r2, off.ctypes.data, None)
            ridx = np.empty(total, np.int32)
            assert L.hq_range(h, Q.ctypes.data, len(Q), r2, off.ctypes.data, ridx.ctypes.data) == total
            assert np.array_equal(off, want_off.astype(np.uint64)), (name, b)
            assert ridx.dtype == want_idx.dtype and np.array_equal(ridx, want_idx), (name, b)
            n += 1
            L.host_tree_destroy(h)
    assert n == 7 * 3 * (len(mg.KS) + 1)
