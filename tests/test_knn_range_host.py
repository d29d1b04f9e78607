"""k nearest within a radius (tdtk_knn_range_search / tdtk_normals_knn_range): the CPU tier.  The fixture k12_knn_range.npz
against the reference's compiled kd.cc, against brute force on every row, and against the lists of KDtreeIndexed that
k8_kdtree_queries.npz pins; the device walk compiled for the host against the fixture; the resource remarks of the k_knnr
kernels."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

import host_lane

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(G, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def mr():
    return _load("make_golden_knn_range")


@pytest.fixture(scope="module")
def fx(mr):
    return mr.load()


@pytest.fixture(scope="module")
def k8():
    return np.load(os.path.join(G, "k8_kdtree_queries.npz"))


def _cases(mr):
    for name, (pts, Q, no, _) in mr.G8.k8_clouds().items():
        for ri in range(3):
            for b in mr.BUCKETS:
                for k in mr.KS:
                    yield name, pts, Q, no, ri, b, k


def _d2(mr, pts, Q, rep):
    return mr.G8.dist2(pts, Q[:, None, :], rep)


def test_fixture_equals_the_reference(mr, orc):
    if not mr.have_ref():
        pytest.skip("no reference checkout (src/slam6d/kd.cc)")
    z = np.load(mr.OUT)
    got, stats = mr.compute(orc)
    mr.check_not_vacuous(stats)
    assert sorted(got) == sorted(z.files)
    for key in z.files:
        assert got[key].dtype == z[key].dtype and np.array_equal(got[key], z[key], equal_nan=got[key].dtype.kind == "f"), key


def test_radii_are_the_stated_ones(mr, fx, k8):
    for name, (pts, Q, no, r2) in mr.G8.k8_clouds().items():
        rr = fx.radii(name)
        assert rr == list(mr.radii(k8, name, pts, Q, r2)) and rr[0] == r2 and rr[2] == 1e30
        d10 = _d2(mr, pts, Q, k8["%s_b1_knn10" % name])
        assert rr[1] == (np.median(d10[:, 9]) if len(pts) >= 10 else d10.max() + 1.0)


def test_every_row_against_brute_force(mr, fx):
    """a row's d2 are the min(k, count) smallest Dist2 < r2 of the cloud, ascending; the counts agree; -1 behind the entries"""
    n = 0
    brute = {}
    for name, pts, Q, no, ri, b, k in _cases(mr):
        r2 = fx.radii(name)[ri]
        if (name, ri) not in brute:
            all_d = _d2(mr, pts, Q, np.arange(len(pts))[None, :])
            brute[(name, ri)] = [np.sort(row[row < r2]) for row in all_d]
        rep, cnt = fx.rows(name, ri, b, k), fx.counts(name, ri, b, k)
        assert rep.shape == (len(Q), k) and cnt.shape == (len(Q),)
        d2 = _d2(mr, pts, Q, rep)
        for i in range(len(Q)):
            inball = brute[(name, ri)][i]
            assert cnt[i] == min(k, len(inball)), (name, ri, b, k, i)
            assert (rep[i, cnt[i]:] == -1).all() and (rep[i, :cnt[i]] >= 0).all()
            assert np.array_equal(d2[i, :cnt[i]], inball[:cnt[i]]), (name, ri, b, k, i)
            n += 1
    assert n == sum(len(c[1]) for c in mr.G8.k8_clouds().values()) * 3 * len(mr.BUCKETS) * len(mr.KS)


def test_short_rows_are_the_sorted_fixed_range_lists(mr, fx, k8):
    """count < k: the list never filled, so the walk is _FixedRangeSearch's (same child order, same plane rule) and the row
    is the stable sort by d2 of KDtreeIndexed::fixedRangeSearch's list -- coordinate for coordinate, ties included"""
    n = 0
    for name, pts, Q, no, ri, b, k in _cases(mr):
        if ri != 0:
            continue
        off, ridx = k8["%s_b%d_roff" % (name, b)].astype(np.int64), k8["%s_b%d_ridx" % (name, b)]
        rep, cnt = fx.rows(name, ri, b, k), fx.counts(name, ri, b, k)
        for i in np.nonzero(cnt < k)[0]:
            l = ridx[off[i]:off[i + 1]]
            d = mr.G8.dist2(pts, np.broadcast_to(Q[i], (len(l), 3)), l)
            want = l[np.argsort(d, kind="stable")]
            assert len(want) == cnt[i], (name, b, k, i)
            assert np.array_equal(pts[rep[i, :cnt[i]]], pts[want]), (name, b, k, i)
            n += 1
    assert n > 5000


def test_huge_radius_rows_have_the_knn_distances(mr, fx, k8):
    """r2 = 1e30: the d2 rows equal those of KDtreeIndexed::kNearestNeighbors bit for bit (points tied at the k-th distance
    may differ between the two walks, distances may not)"""
    for name, pts, Q, no, ri, b, k in _cases(mr):
        if ri != 2 or k not in mr.G8.KS:
            continue
        want = _d2(mr, pts, Q, k8["%s_b%d_knn%d" % (name, b, k)])
        assert np.array_equal(_d2(mr, pts, Q, fx.rows(name, ri, b, k)), want), (name, b, k)
        assert np.array_equal(fx.counts(name, ri, b, k), np.full(len(Q), min(k, len(pts))))


def test_fixture_is_not_vacuous_and_small(mr, fx):
    full = short = rows = empty = 0
    for name in mr.LARGE:
        pts, Q, _, _ = mr.G8.k8_clouds()[name]
        rr = fx.radii(name)
        inball = (_d2(mr, pts, Q, np.arange(len(pts))[None, :]) < rr[1]).sum(1)
        for b in mr.BUCKETS:
            cnt = fx.counts(name, 1, b, 10)
            rows += len(cnt)
            full += int(((cnt == 10) & (inball > 10)).sum())
            short += int(((cnt > 0) & (cnt < 10)).sum())
            empty += int((fx.counts(name, 0, b, 10) == 0).sum())
    assert 4 * full >= rows and 4 * short >= rows and empty >= 1, (full, short, rows, empty)
    assert os.path.getsize(mr.OUT) <= os.path.getsize(os.path.join(G, "k8_kdtree_queries.npz"))


def test_fixture_normals(mr, fx):
    """own-point rows only: unit length where finite; lists of one and two points are among them"""
    lens = set()
    for name, (pts, Q, no, _) in mr.G8.k8_clouds().items():
        for ri in range(3):
            for b in mr.BUCKETS:
                for k in mr.NORMAL_KS:
                    n = fx.normals(name, ri, b, k)
                    assert n.shape == (no, 3)
                    fin = np.isfinite(n).all(1)
                    assert np.allclose(np.linalg.norm(n[fin], axis=1), 1.0)
                    cnt = fx.counts(name, ri, b, k)[:no]
                    assert (cnt >= 1).all()               # a point finds itself
                    lens |= set(cnt.tolist())
    assert {1, 2} <= lens


def test_header_exports_and_mirror_name_the_new_entry_points(tdtk):
    from importlib import import_module
    capi = import_module("3dtk_amd._capi")
    hdr = open(os.path.join(ROOT, "include", "tdtk_hip.h")).read()
    for sym in ("tdtk_knn_range_search", "tdtk_normals_knn_range"):
        assert sym in capi.EXPORTS
        assert re.search(r"\bint %s\(" % sym, hdr), sym
    assert hasattr(tdtk, "calculateNormalsKNNRange")
    for m in ("kNearestRangeSearch", "kNearestRangeSearchBatch"):
        assert hasattr(tdtk.KDtree, m)


def test_knn_range_kernels_spill_nothing():
    path = os.path.join(ROOT, "3dtk_amd", "csrc", "query.resource.txt")
    if not os.path.exists(path):
        pytest.skip("no build in this tree (query.resource.txt is written by the Makefile)")
    blocks = [b for b in open(path).read().split("remark: Function Name: ")[1:] if "k_knnr" in b.split()[0]]
    names = [b.split()[0] for b in blocks]
    assert sum("k_knnr_reg" in n for n in names) == 8 and sum("k_knnr_lds" in n for n in names) == 2, names
    for b in blocks:
        for key in ("VGPRs Spill", "SGPRs Spill"):
            m = re.search(key + r": (\d+)", b)
            assert m and int(m.group(1)) == 0, (b.split()[0], key)


# ---- the device walk on the host -----------------------------------------------------------------------------------
# knn_range_walk, the LDS list and the helpers they call, as they stand in query_lane.h (host_lane_shim.h: __device__ defined
# away, a std::vector for the lane stack), with kd_build.cpp's host tree under them
_HOST_WALK = r"""
extern "C" void hw_search(void* p, const double* q, int nq, int k, double r2, int* idx, double* d2, int* cnt) {
  HostTree& T = *(HostTree*)p;
  QueryArgs a = host_args(T);
  std::vector<double> ld(64); std::vector<uint32_t> ls(64);
  for (int i = 0; i < nq; i++) {
    ListLds<1> L; L.ld = ld.data(); L.ls = ls.data(); L.init(k);
    HostStack st;
    knn_range_walk(a, q[3 * i], q[3 * i + 1], q[3 * i + 2], r2, L, st);
    int nr = 0;
    for (int j = 0; j < k; j++) nr += (L.dist(j) >= 0.0) ? 1 : 0;
    cnt[i] = nr;
    for (int j = 0; j < k; j++) { const bool v = j < nr; idx[i * k + j] = v ? a.pts[L.slot(j)].orig : -1; d2[i * k + j] = v ? L.dist(j) : -1.0; }
  }
}
"""


def test_device_walk_compiled_for_the_host_equals_the_fixture(mr, fx, tmp_path):
    L = host_lane.build(_HOST_WALK, tmp_path, "hw")
    L.hw_search.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    n = 0
    for name, (pts, Q, no, _) in mr.G8.k8_clouds().items():
        pts, Q = np.ascontiguousarray(pts), np.ascontiguousarray(Q)
        for b in mr.BUCKETS:
            h = L.host_tree_create(pts.ctypes.data, len(pts), b)
            assert h
            for ri, r2 in enumerate(fx.radii(name)):
                for k in mr.KS:
                    idx = np.empty((len(Q), k), np.int32); d2 = np.empty((len(Q), k)); cnt = np.empty(len(Q), np.int32)
                    L.hw_search(h, Q.ctypes.data, len(Q), k, r2, idx.ctypes.data, d2.ctypes.data, cnt.ctypes.data)
                    rep, have = fx.rows(name, ri, b, k), idx >= 0
                    assert np.array_equal(cnt, fx.counts(name, ri, b, k)), (name, b, ri, k)
                    assert np.array_equal(have, rep >= 0) and np.array_equal(pts[idx[have]], pts[rep[have]]), (name, b, ri, k)
                    assert np.array_equal(d2, np.where(have, _d2(mr, pts, Q, idx), -1.0)), (name, b, ri, k)
                    n += 1
            L.host_tree_destroy(h)
    assert n == 7 * 3 * 3 * len(mr.KS)
