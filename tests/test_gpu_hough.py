"""The standard 3D Hough transform on the device (tdtk_hough_* and their Python mirror) against the fixture k22_hough.npz,
whose counts, peak lists, cell planes and calcPlane results are the reference's own compiled accumulators (the CPU tier pins
the fixture to the live reference).  Counts, peak lists and index lists are compared exactly; the fitted planes within the
bounds derived in tests/hough_fit_bounds.py.

Largest fit_plane errors observed on an MI355X against their bounds, over the fixture's planes: see DESIGN.md section 4, "3D
Hough transform"."""
import ctypes as C
import importlib
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hough_fit_bounds                              # noqa: E402

pytestmark = pytest.mark.gpu
TDTK_EINVAL, TDTK_EUNSUP = -1, -5
_dp, _ip, _u32p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)


def _gold():
    spec = importlib.util.spec_from_file_location("make_golden_hough", os.path.join(G, "make_golden_hough.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


gold = _gold()
CASES = gold.case_list()
NAMES = [c["name"] for c in CASES]
PUBLIC = [c["name"] for c in CASES if c["public"]]


@pytest.fixture(scope="module")
def fx():
    return gold.load()


def dp(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def ip(a):
    return a.ctypes.data_as(_ip) if a is not None else None


def dims_of(case):
    return np.array([case["RhoNum"], case["PhiNum"], case["ThetaNum"], case["RhoMax"]], np.uint32)


def vote(L, case, table, xyz="own", counts="own"):
    pts = case["xyz"] if isinstance(xyz, str) else xyz
    out = np.full((len(table), case["RhoNum"]), -7, np.int32) if isinstance(counts, str) else counts
    rc = L.tdtk_hough_vote(0, dp(pts), len(case["xyz"]), dp(table), len(table), case["RhoNum"], case["RhoMax"], case["D"], ip(out))
    return rc, out


def cfg_of(tdtk, case):
    hough = importlib.import_module("3dtk_amd.hough")
    return hough.ConfigFileHough(AccumulatorType=case["type"], RhoNum=case["RhoNum"], PhiNum=case["PhiNum"], ThetaNum=case["ThetaNum"],
                                 RhoMax=case["RhoMax"], MaxPointPlaneDist=case["D"], PlaneRatio=case["ratio"], MaxPlanes=-1)


@pytest.mark.parametrize("name", NAMES)
def test_vote_over_the_fixtures_table_is_the_references(tdtk, gpu, fx, name):
    case = fx.cases[name]
    rc, counts = vote(tdtk.lib(), case, np.ascontiguousarray(fx.get(name, "table")))
    assert rc == 0, tdtk.lib().tdtk_last_error()
    assert np.array_equal(counts, fx.get(name, "counts"))


@pytest.mark.parametrize("name", NAMES)
def test_vote_on_the_lab_library(tdtk, gpu, lab, fx, name):
    case = fx.cases[name]
    rc, counts = vote(tdtk.lib(), case, np.ascontiguousarray(fx.get(name, "table")))
    assert rc == 0
    assert np.array_equal(counts, fx.get(name, "counts"))


@pytest.mark.parametrize("name", PUBLIC)
def test_votes_through_the_public_path(tdtk, gpu, fx, name):
    """the table from tdtk_hough_normals (this machine's libm): the generator's margin condition makes the counts the same"""
    case = fx.cases[name]
    h = tdtk.Hough(case["xyz"], cfg_of(tdtk, case))
    assert h.normals.shape == fx.get(name, "table").shape
    assert np.array_equal(h.votes(), fx.get(name, "counts"))


@pytest.mark.parametrize("name", ["types_simple", "types_ball", "types_cube", "types_balli", "plane5000"])
def test_votes_through_the_public_path_on_the_lab_library(tdtk, gpu, lab, fx, name):
    case = fx.cases[name]
    assert np.array_equal(tdtk.Hough(case["xyz"], cfg_of(tdtk, case)).votes(), fx.get(name, "counts"))


def peaks(L, case, counts, cap):
    w = gold.entry_width(case)
    cells = np.full((max(cap, 1), w), -7, np.int32)
    n, mx = C.c_uint64(0), C.c_int32(-1)
    d = dims_of(case)
    rc = L.tdtk_hough_peaks(0, ip(counts), case["type"], d.ctypes.data_as(_u32p), case["ratio"], ip(cells), cap, C.byref(n),
                            C.byref(mx))
    return rc, cells, n.value, mx.value


@pytest.mark.parametrize("name", NAMES)
def test_peaks_entry_for_entry(tdtk, gpu, fx, name):
    case = fx.cases[name]
    L = tdtk.lib()
    ref = fx.get(name, "peaks")
    counts = np.ascontiguousarray(fx.get(name, "counts"))
    rc, cells, n, mx = peaks(L, case, counts, len(ref))
    assert rc == 0, L.tdtk_last_error()
    assert n == len(ref) and mx == int(fx.get(name, "max"))
    assert np.array_equal(cells[:n], ref)
    # and from the counts a vote left on the device
    rc, _ = vote(L, case, np.ascontiguousarray(fx.get(name, "table")), counts=None)
    assert rc == 0
    rc, cells, n, mx = peaks(L, case, None, len(ref))
    assert rc == 0 and n == len(ref) and np.array_equal(cells[:n], ref)


def test_peaks_cap_too_small_and_refusals(tdtk, gpu, fx):
    case = fx.cases["types_ball"]
    L = tdtk.lib()
    ref = fx.get("types_ball", "peaks")
    counts = np.ascontiguousarray(fx.get("types_ball", "counts"))
    rc, cells, n, mx = peaks(L, case, counts, len(ref) - 1)
    assert rc == TDTK_EINVAL and n == len(ref) and mx == int(fx.get("types_ball", "max")) and (cells == -7).all()
    assert b"cap" in L.tdtk_last_error()
    d = dims_of(case)
    nn, mm = C.c_uint64(0), C.c_int32(0)
    dpt = d.ctypes.data_as(_u32p)
    assert L.tdtk_hough_peaks(0, ip(counts), 1, None, 0.5, ip(cells), 1, C.byref(nn), C.byref(mm)) == TDTK_EINVAL
    assert L.tdtk_hough_peaks(0, ip(counts), 1, dpt, float("nan"), ip(cells), 1, C.byref(nn), C.byref(mm)) == TDTK_EINVAL
    assert L.tdtk_hough_peaks(0, ip(counts), 7, dpt, 0.5, ip(cells), 1, C.byref(nn), C.byref(mm)) == TDTK_EINVAL
    # counts NULL, but the thread's last vote was another accumulator's
    other = fx.cases["n64"]
    assert vote(L, other, np.ascontiguousarray(fx.get("n64", "table")))[0] == 0
    assert L.tdtk_hough_peaks(0, None, 1, dpt, 0.5, ip(cells), 1, C.byref(nn), C.byref(mm)) == TDTK_EINVAL
    assert b"last vote" in L.tdtk_last_error()


@pytest.mark.parametrize("name", NAMES)
def test_plane_points_index_lists(tdtk, gpu, fx, name):
    case = fx.cases[name]
    h = tdtk.Hough(case["xyz"], cfg_of(tdtk, case))
    planes = fx.get(name, "planes")
    for i, ref in enumerate(fx.inliers(name)):
        mask, idx = h.plane_points(planes[i][:3] * 4.0, planes[i][3])      # Normalize3 first: any length of n (a power of two: the same bits)
        assert idx.dtype == np.int32 and np.array_equal(idx, ref)
        assert np.array_equal(np.flatnonzero(mask), ref)


def test_plane_points_cap_contract(tdtk, gpu, fx):
    case = fx.cases["plane5000"]
    L = tdtk.lib()
    xyz = case["xyz"]
    plane = fx.get("plane5000", "planes")[0]
    ref = fx.inliers("plane5000")[0]
    n = np.ascontiguousarray(plane[:3])
    idx = np.full(len(xyz), -7, np.int32)
    cnt = C.c_uint64(0)
    args = (0, dp(xyz), len(xyz), dp(n), float(plane[3]), case["D"], None)
    assert L.tdtk_hough_plane_points(*args, ip(idx), len(ref) - 1, C.byref(cnt)) == TDTK_EINVAL
    assert cnt.value == len(ref) and (idx == -7).all()
    assert L.tdtk_hough_plane_points(*args, ip(idx), len(ref), C.byref(cnt)) == 0 and np.array_equal(idx[:len(ref)], ref)
    assert L.tdtk_hough_plane_points(0, dp(xyz), len(xyz), None, 1.0, 1.0, None, ip(idx), 1, C.byref(cnt)) == TDTK_EINVAL
    # the resident cloud: NULL xyz with the size of the last upload is that cloud, another size is refused
    assert L.tdtk_hough_plane_points(0, None, len(xyz), dp(n), float(plane[3]), case["D"], None, ip(idx), len(ref), C.byref(cnt)) == 0
    assert np.array_equal(idx[:len(ref)], ref)
    assert L.tdtk_hough_plane_points(0, None, len(xyz) + 1, dp(n), 1.0, 1.0, None, ip(idx), 1, C.byref(cnt)) == TDTK_EINVAL
    assert b"resident" in L.tdtk_last_error()


def test_fit_plane_within_the_derived_bounds(tdtk, gpu, fx):
    worst = dict(normal=0.0, d=0.0, planarity=0.0)
    seen = 0
    for name in NAMES:
        case = fx.cases[name]
        fits = fx.get(name, "fits")
        h = None
        for i, idx in enumerate(fx.inliers(name)):
            ref_plane, ref_planarity, gap, m = fits[i][:4], fits[i][4], fits[i][5], int(fits[i][6])
            if m < 3 or gap < 0.1:
                continue
            h = h or tdtk.Hough(case["xyz"], cfg_of(tdtk, case))
            plane, planarity = h.fit_plane(idx)
            b = hough_fit_bounds.bounds(case["xyz"][idx])
            s = 1.0 if float(plane[:3] @ ref_plane[:3]) > 0 else -1.0
            e_n = float(np.abs(s * plane[:3] - ref_plane[:3]).max())
            e_d = abs(s * plane[3] - ref_plane[3])
            e_p = abs(planarity - ref_planarity)
            print("%-14s plane %d  m %5d  gap %.3f  |dn| %.2e (bound %.2e)  |dd| %.2e (%.2e)  |dplanarity| %.2e (%.2e)" %
                  (name, i, m, gap, e_n, b["tol_normal"], e_d, b["tol_d"], e_p, b["tol_planarity"]))
            assert e_n <= b["tol_normal"] and e_d <= b["tol_d"] and e_p <= b["tol_planarity"], name
            worst = dict(normal=max(worst["normal"], e_n / b["tol_normal"]), d=max(worst["d"], e_d / b["tol_d"]),
                         planarity=max(worst["planarity"], e_p / b["tol_planarity"]))
            seen += 1
    print("largest error / bound:", worst)
    assert seen >= 20


def test_fit_plane_small_sets_and_refusals(tdtk, gpu, fx):
    case = fx.cases["n64"]
    L = tdtk.lib()
    xyz = case["xyz"]
    plane = np.full(4, 9.0)
    pl = C.c_double(5.0)
    idx = np.array([3, 1], np.int32)
    assert L.tdtk_hough_fit_plane(0, dp(xyz), len(xyz), ip(idx), 2, dp(plane), C.byref(pl)) == 0
    assert pl.value == 0.0 and (plane == 9.0).all()                         # calcPlane: n < 3 returns 0, plane untouched
    bad = np.array([3, 1, 64], np.int32)
    assert L.tdtk_hough_fit_plane(0, dp(xyz), len(xyz), ip(bad), 3, dp(plane), C.byref(pl)) == TDTK_EINVAL
    assert L.tdtk_hough_fit_plane(0, dp(xyz), len(xyz), None, 3, dp(plane), C.byref(pl)) == TDTK_EINVAL
    assert L.tdtk_hough_fit_plane(0, dp(xyz), len(xyz), ip(idx), 2, None, C.byref(pl)) == TDTK_EINVAL
    h = tdtk.Hough(xyz, cfg_of(tdtk, case))
    assert h.fit_plane([0, 1]) == (None, 0.0)
    # the same index list twice: the same bits (fixed order of the sums)
    a, pa = h.fit_plane(np.arange(64))
    b, pb = h.fit_plane(np.arange(64))
    assert np.array_equal(a, b) and pa == pb


def test_vote_refusals_in_order(tdtk, gpu, fx):
    case = fx.cases["n64"]
    L = tdtk.lib()
    table = np.ascontiguousarray(fx.get("n64", "table"))
    xyz = case["xyz"]
    out = np.zeros((len(table), 20), np.int32)
    f = L.tdtk_hough_vote
    assert f(0, dp(xyz), 64, None, 20, 20, 100, 4.0, ip(out)) == TDTK_EINVAL
    assert f(0, dp(xyz), 1 << 31, None, 20, 20, 100, 4.0, ip(out)) == TDTK_EINVAL              # NULL before the size
    assert f(0, dp(xyz), 1 << 31, dp(table), 0, 20, 100, 4.0, ip(out)) == TDTK_EUNSUP           # N before C
    assert f(0, dp(xyz), 64, dp(table), 0, 20, 100, 4.0, ip(out)) == TDTK_EINVAL
    assert f(0, dp(xyz), 64, dp(table), 20, 0, 100, 4.0, ip(out)) == TDTK_EINVAL
    assert f(0, dp(xyz), 64, dp(table), 1 << 20, 1 << 11, 100, 4.0, ip(out)) == TDTK_EUNSUP     # C * RhoNum = 2^31
    assert b"2^31" in L.tdtk_last_error()
    assert (out == 0).all()
    # normals: capacity and refusals through the library
    d = dims_of(fx.cases["types_ball"])
    n = C.c_size_t(0)
    small = np.full((117, 3), 9.0)
    assert L.tdtk_hough_normals(1, d.ctypes.data_as(_u32p), dp(small), 117, C.byref(n), None) == TDTK_EINVAL
    assert n.value == 118 and (small == 9.0).all()
    assert L.tdtk_hough_normals(1, None, dp(small), 117, C.byref(n), None) == TDTK_EINVAL
    d2 = np.array([20, 12, 1, 100], np.uint32)
    assert L.tdtk_hough_normals(1, d2.ctypes.data_as(_u32p), None, 0, C.byref(n), None) == TDTK_EUNSUP
    assert b"ThetaNum" in L.tdtk_last_error()
    cell = np.array([0, 0, 0, 12], np.int32)
    plane = np.zeros(4)
    assert L.tdtk_hough_cell_plane(1, d.ctypes.data_as(_u32p), ip(cell), dp(plane)) == TDTK_EINVAL


def test_second_vote_reuses_its_buffers(tdtk, gpu, fx):
    hough = importlib.import_module("3dtk_amd.hough")
    case = fx.cases["rho500"]
    L = tdtk.lib()
    table = np.ascontiguousarray(fx.get("rho500", "table"))
    rc, first = vote(L, case, table)
    assert rc == 0
    before = hough.last_timings()
    rc, second = vote(L, case, table)
    after = hough.last_timings()
    assert rc == 0 and np.array_equal(first, second) and np.array_equal(second, fx.get("rho500", "counts"))
    assert after["allocations"] == before["allocations"] and before["allocations"] >= 1
    assert after["vote_ms"] > 0
    # a smaller vote on the same context as well, and the resident cloud serves a vote with NULL xyz
    small = fx.cases["rho7"]
    assert len(small["xyz"]) == len(case["xyz"])
    rc, _ = vote(L, small, np.ascontiguousarray(fx.get("rho7", "table")))
    assert rc == 0 and hough.last_timings()["allocations"] == before["allocations"]
    rc, again = vote(L, small, np.ascontiguousarray(fx.get("rho7", "table")), xyz=None)
    assert rc == 0 and np.array_equal(again, fx.get("rho7", "counts"))


@pytest.mark.parametrize("name", ["types_simple", "types_ball", "types_cube", "types_balli", "plane5000", "far"])
def test_sht_plane_candidates(tdtk, gpu, fx, name):
    """SHT(): every peak with its plane, inliers and refit, over the undiminished cloud"""
    case = fx.cases[name]
    cfg = cfg_of(tdtk, case)
    cfg.MaxPlanes = 2
    h = tdtk.Hough(case["xyz"], cfg)
    out = h.SHT()
    ref_peaks, planes, inl, fits = fx.get(name, "peaks"), fx.get(name, "planes"), fx.inliers(name), fx.get(name, "fits")
    assert len(out) == min(2, len(ref_peaks))
    for i, cand in enumerate(out):
        assert np.array_equal(cand["cell"], ref_peaks[i])
        assert np.abs(cand["plane"] - planes[i]).max() <= 4 * np.spacing(np.abs(planes[i]).max())
        assert cand["inliers"] == len(inl[i]) and np.array_equal(cand["indices"], inl[i])
        if len(inl[i]) >= 3 and fits[i][5] >= 0.1:
            b = hough_fit_bounds.bounds(case["xyz"][inl[i]])
            assert abs(cand["planarity"] - fits[i][4]) <= b["tol_planarity"]
