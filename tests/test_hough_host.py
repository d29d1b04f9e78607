"""The standard 3D Hough transform (tdtk_hough_*): the CPU tier.  The per-lane device code (3dtk_amd/csrc/hough_lane.h) and
the host-only geometry of the four accumulators (hough_host.cpp) compiled for the host without contraction, against the
fixture tests/golden/k22_hough.npz -- the reference's compiled accumulators -- on every case; where the reference checkout is
present, the live compiled reference against the fixture as well.  Also the compiler's resource remarks of hough.hip, the
declaration and binding of the entry points, and ConfigFileHough."""
import ctypes as C
import importlib
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import host_lane                                    # noqa: E402
import make_golden_hough as gold                    # noqa: E402

DRIVER = r"""
#include "hough_lane.h"
#include "hough_host.cpp"

// k_hough_vote's loop body, one point and cell after the other; windowed = 0 tries every bin instead of hough_window's
extern "C" void hl_vote(const double* xyz, long n, const double* normals, long C, unsigned rho_num, unsigned rho_max, double D,
                        int windowed, int32_t* counts)
{
  const double rho_max_d = (double)rho_max, rho_num_d = (double)rho_num, inv_bin = rho_num_d / rho_max_d;
  std::vector<double> rho(rho_num);
  for (unsigned k = 0; k < rho_num; ++k) rho[k] = hough_rho(k, rho_max_d, rho_num_d);
  for (long c = 0; c < C; ++c)
    for (long i = 0; i < n; ++i) {
      const double d = hough_distance(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], normals[3 * c], normals[3 * c + 1], normals[3 * c + 2]);
      uint32_t lo = 0, hi = rho_num;
      if (windowed) hough_window(d, inv_bin, rho_num_d, D, lo, hi);
      for (uint32_t k = lo; k < hi; ++k)
        if (hough_votes(d, rho[k], D)) counts[c * (long)rho_num + k] += 1;
    }
}

extern "C" void hl_window(double d, unsigned rho_num, unsigned rho_max, double D, uint32_t* lohi)
{
  hough_window(d, (double)rho_num / (double)rho_max, (double)rho_num, D, lohi[0], lohi[1]);
}

extern "C" long hl_plane_points(const double* xyz, long n, const double* n_in, double rho, double D, int32_t* idx)
{
  double nn[3] = {n_in[0], n_in[1], n_in[2]};
  const double norm = std::sqrt(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2]);      // as tdtk_hough_plane_points does
  nn[0] /= norm; nn[1] /= norm; nn[2] /= norm;
  long k = 0;
  for (long i = 0; i < n; ++i)
    if (hough_on_plane(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], nn[0], nn[1], nn[2], rho, D)) idx[k++] = (int32_t)i;
  return k;
}

// tdtk_hough_normals without the capacity contract: the return code, *C, the slice sizes, the table
extern "C" int hl_normals(int type, const uint32_t* dims, double* normals, long cap, long* C, int32_t* sizes, char* msg, int msg_cap)
{
  HoughGeom g; std::string err;
  const int rc = hough_geometry(type, dims[0], dims[1], dims[2], dims[3], g, err);
  if (rc) { strncpy(msg, err.c_str(), msg_cap - 1); msg[msg_cap - 1] = 0; return rc; }
  *C = (long)g.cells;
  for (size_t i = 0; i < g.slices.size(); ++i) sizes[i] = g.slices[i];
  if ((long)g.cells <= cap) hough_geom_normals(g, normals);
  return 0;
}

extern "C" int hl_cell_plane(int type, const uint32_t* dims, const int32_t* cell, double* plane4)
{
  HoughGeom g; std::string err;
  const int rc = hough_geometry(type, dims[0], dims[1], dims[2], dims[3], g, err);
  if (rc) return rc;
  hough_geom_cell_plane(g, cell, plane4);
  return 0;
}

// what tdtk_hough_peaks does behind the device's compaction: threshold, records in arrival order (here: reversed, so that
// the order is made by hough_order_peaks alone), the reference's order and layout
extern "C" long hl_peaks(int type, const uint32_t* dims, const int32_t* counts, double ratio, int32_t* entries, long cap, int32_t* max_out)
{
  HoughGeom g; std::string err;
  if (hough_geometry(type, dims[0], dims[1], dims[2], dims[3], g, err)) return -1;
  const size_t total = g.cells * (size_t)g.rho_num;
  int32_t mx = 0;
  for (size_t i = 0; i < total; ++i) mx = std::max(mx, counts[i]);
  *max_out = mx;
  const int32_t thr = (int32_t)((double)mx * ratio);
  std::vector<std::pair<int32_t, uint32_t>> rec;
  for (size_t i = total; i-- > 0;) if (counts[i] > thr) rec.push_back({counts[i], (uint32_t)i});
  if ((long)rec.size() <= cap) hough_order_peaks(g, rec, entries);
  return (long)rec.size();
}
"""


@pytest.fixture(scope="module")
def lane(tmp_path_factory):
    L = host_lane.build("#include <algorithm>\n#include <utility>\n" + DRIVER, tmp_path_factory.mktemp("hough_lane"), "hough_lane")
    L.hl_vote.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_uint, C.c_uint, C.c_double, C.c_int, C.c_void_p]
    L.hl_vote.restype = None
    L.hl_window.argtypes = [C.c_double, C.c_uint, C.c_uint, C.c_double, C.c_void_p]
    L.hl_window.restype = None
    L.hl_plane_points.restype = C.c_long
    L.hl_plane_points.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_double, C.c_double, C.c_void_p]
    L.hl_normals.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    L.hl_cell_plane.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.hl_peaks.restype = C.c_long
    L.hl_peaks.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_long, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def fixture():
    return gold.load()


NAMES = [c["name"] for c in gold.case_list()]


def dims_of(case):
    return np.array([case["RhoNum"], case["PhiNum"], case["ThetaNum"], case["RhoMax"]], np.uint32)


def ulps(a, b):
    """|a - b| in units of the spacing of b, per component"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.spacing(np.abs(b))


def host_normals(L, case):
    C_ = C.c_long(0)
    sizes = np.zeros(max(case["PhiNum"], 6), np.int32)
    table = np.zeros((1 << 12, 3))
    msg = C.create_string_buffer(512)
    d = dims_of(case)
    rc = L.hl_normals(case["type"], d.ctypes.data, table.ctypes.data, len(table), C.byref(C_), sizes.ctypes.data, msg, 512)
    assert rc == 0, msg.value
    return table[:C_.value], sizes


@pytest.mark.parametrize("name", NAMES)
def test_lane_code_votes_as_the_reference(lane, fixture, name):
    case = fixture.cases[name]
    table, ref = fixture.get(name, "table"), fixture.get(name, "counts")
    xyz = case["xyz"]
    for windowed in (1, 0):
        counts = np.zeros(ref.shape, np.int32)
        lane.hl_vote(xyz.ctypes.data, len(xyz), table.ctypes.data, len(table), case["RhoNum"], case["RhoMax"], case["D"], windowed,
                     counts.ctypes.data)
        assert np.array_equal(counts, ref), "windowed %d" % windowed


def test_window_survives_what_no_cloud_should_hold(lane):
    lohi = np.zeros(2, np.uint32)
    inf, nan = float("inf"), float("nan")
    for d, D, want in ((nan, 1.0, None), (inf, 1.0, None), (-inf, 1.0, None), (1e300, 1.0, None), (50.0, inf, (0, 20)),
                       (50.0, nan, None), (50.0, -1.0, None), (inf, inf, None), (52.5, 4.0, None)):
        lane.hl_window(d, 20, 100, D, lohi.ctypes.data)
        assert 0 <= lohi[0] <= 20 and 0 <= lohi[1] <= 20
        if want:
            assert tuple(lohi) == want
    lane.hl_window(52.5, 20, 100, 4.0, lohi.ctypes.data)      # bins 10 (rho 52.5) and its neighbours at distance 5: only 10 votes
    assert lohi[0] <= 10 < lohi[1] and lohi[1] - lohi[0] <= 5
    lane.hl_window(3.0, 20, 0, 4.0, lohi.ctypes.data)          # RhoMax 0: every rho is 0, the whole range
    assert tuple(lohi) == (0, 20)


@pytest.mark.parametrize("name", NAMES)
def test_peak_order_is_the_multisets(lane, fixture, name):
    case = fixture.cases[name]
    ref = fixture.get(name, "peaks")
    counts = np.ascontiguousarray(fixture.get(name, "counts"))
    w = gold.entry_width(case)
    out = np.zeros((len(ref) + 1, w), np.int32)
    mx = C.c_int32(0)
    d = dims_of(case)
    n = lane.hl_peaks(case["type"], d.ctypes.data, counts.ctypes.data, case["ratio"], out.ctypes.data, len(out), C.byref(mx))
    assert n == len(ref) and mx.value == int(fixture.get(name, "max"))
    assert np.array_equal(out[:n], ref)


@pytest.mark.parametrize("name", NAMES)
def test_normals_and_cell_planes_within_4_ulp(lane, fixture, name):
    case = fixture.cases[name]
    table, sizes = host_normals(lane, case)
    ref = fixture.get(name, "table")
    want, _ = gold.slice_sizes(case)
    assert sizes[:len(want)].tolist() == list(want)
    assert table.shape == ref.shape
    assert ulps(table, ref).max() <= 4
    cells, planes = fixture.get(name, "cells"), fixture.get(name, "planes")
    d = dims_of(case)
    for cell, plane in zip(cells, planes):
        got = np.zeros(4)
        cell = np.ascontiguousarray(cell, np.int32)
        assert lane.hl_cell_plane(case["type"], d.ctypes.data, cell.ctypes.data, got.ctypes.data) == 0
        assert ulps(got, plane).max() <= 4, (cell, got, plane)


def test_cell_plane_is_not_the_votes_normal(lane, fixture):
    """getMax(int*) has no 0.999999999 in phi: the plane of a Ball cell is near, not equal to, the normal the cell votes with"""
    case = fixture.cases["types_ball"]
    table, sizes = host_normals(lane, case)
    got = np.zeros(4)
    cell = np.array([0, 3, 1, 5], np.int32)
    d = dims_of(case)
    lane.hl_cell_plane(case["type"], d.ctypes.data, cell.ctypes.data, got.ctypes.data)
    n = table[sizes[:5].sum() + 1]
    assert np.abs(got[:3] - n).max() < 1e-8 and not np.array_equal(got[:3], n)
    assert got[3] == (3 + 0.5) * 100.0 / 20.0


@pytest.mark.parametrize("name", NAMES)
def test_plane_points_lane_code(lane, fixture, name):
    case = fixture.cases[name]
    xyz = case["xyz"]
    planes = fixture.get(name, "planes")
    for i, ref in enumerate(fixture.inliers(name)):
        idx = np.zeros(len(xyz) + 1, np.int32)
        n = np.ascontiguousarray(planes[i][:3])
        k = lane.hl_plane_points(xyz.ctypes.data, len(xyz), n.ctypes.data, float(planes[i][3]), case["D"], idx.ctypes.data)
        assert np.array_equal(idx[:k], ref)


def test_geometry_refusals(lane):
    """the (PhiNum, ThetaNum) the reference's constructors cannot take are refused, with a message, and exactly those"""
    msg = C.create_string_buffer(512)
    C_ = C.c_long(0)
    sizes = np.zeros(1024, np.int32)

    def rc(t, rho, phi, theta):
        d = np.array([rho, phi, theta, 100], np.uint32)
        return L.hl_normals(t, d.ctypes.data, None, 0, C.byref(C_), sizes.ctypes.data, msg, 512)
    L = lane
    assert rc(4, 20, 12, 16) == -1 and rc(-1, 20, 12, 16) == -1
    for t in range(4):
        assert rc(t, 0, 12, 16) == -1 and rc(t, 20, 0, 16) == -1 and rc(t, 20, 12, 0) == -1
    assert rc(0, 20, 1 << 24, 16) == -5
    assert rc(1, 20, 12, 1) == -5 and b"ThetaNum" in msg.value
    assert rc(2, 20, 12, 3) == -5 and rc(2, 20, 12, 4) == 0 and C_.value == 6
    assert rc(3, 20, 2, 16) == -5 and rc(3, 20, 1, 16) == -5 and rc(3, 20, 3, 16) == 0
    # AccumulatorBall's slice loop adds 180.0 / PhiNum until it reaches 180.0: the PhiNum for which the sum falls short after
    # PhiNum additions make the reference write ballNr[PhiNum]
    bad = []
    for phi in range(1, 400):
        step, x, trips = 180.0 / phi, 0.0, 0
        while x < 180.0:
            x += step
            trips += 1
        got = rc(1, 20, phi, 16)
        assert (got == 0) == (trips == phi), phi
        if trips != phi:
            bad.append(phi)
            assert got == -5 and b"ballNr" in msg.value
        else:
            assert C_.value == sizes[:phi].sum() and (sizes[:phi] >= 1).all()
    assert bad, "no PhiNum below 400 overruns: the refusal is untested"
    assert rc(1, 20, 12, 16) == 0 and sizes[:12].tolist() == [2, 6, 10, 12, 14, 15, 15, 14, 12, 10, 6, 2]


def test_cases_hold_what_they_are_there_for(fixture):
    gold.check_cases(fixture.z)
    assert os.path.getsize(gold.OUT) <= gold.MAX_BYTES


@pytest.mark.skipif(not gold.have_ref(), reason="needs the reference checkout (TDTK_REF)")
def test_live_reference_matches_the_fixture(fixture):
    for name, case in fixture.cases.items():
        res = gold.run_reference(case, case["xyz"])
        assert np.array_equal(res["counts"], fixture.get(name, "counts")), name
        assert np.array_equal(res["peaks"], fixture.get(name, "peaks")) and res["max"] == int(fixture.get(name, "max")), name
        assert np.array_equal(res["cells"], fixture.get(name, "cells")) and np.array_equal(res["planes"], fixture.get(name, "planes")), name
        assert np.array_equal(res["fits"], fixture.get(name, "fits")), name
        for a, b in zip(res["inliers"], fixture.inliers(name)):
            assert np.array_equal(a, b), name
        assert np.array_equal(gold.normals_table(case), fixture.get(name, "table")), name


def test_hough_kernels_spill_nothing():
    """The resource remarks of hough.hip (csrc/Makefile keeps them): no VGPR spill, no SGPR spill, no scratch."""
    path = os.path.join(ROOT, "3dtk_amd", "csrc", "hough.resource.txt")
    if not os.path.exists(path):
        pytest.skip("no build in this tree (hough.resource.txt is written by the Makefile)")
    blocks = open(path).read().split("remark: Function Name: ")[1:]
    names = set()
    for b in blocks:
        name = b.split()[0]
        names.add(name)
        for what in ("VGPRs Spill", "SGPRs Spill", r"ScratchSize \[bytes/lane\]"):
            m = re.search(what + r": (\d+)", b)
            assert m and int(m.group(1)) == 0, (name, what)
    for k in ("k_hough_vote", "k_hough_rho", "k_hough_max", "k_hough_peaks", "k_hough_plane_points", "k_hough_plane_fill",
              "k_hough_moments"):
        assert any(k in n for n in names), k


def test_abi_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "tdtk_hip.h")).read()
    capi = open(os.path.join(ROOT, "3dtk_amd", "_capi.py")).read()
    for sym in ("tdtk_hough_normals", "tdtk_hough_vote", "tdtk_hough_peaks", "tdtk_hough_cell_plane", "tdtk_hough_plane_points",
                "tdtk_hough_fit_plane", "tdtk_hough_timings"):
        assert re.search(r"\bint %s\(" % sym, hdr), sym
        assert '"%s"' % sym in capi and "L.%s.argtypes" % sym in capi, sym


def test_config_file_hough(tmp_path):
    hough = importlib.import_module("3dtk_amd.hough")
    cfg = hough.ConfigFileHough()
    assert (cfg.RhoNum, cfg.ThetaNum, cfg.PhiNum, cfg.RhoMax, cfg.MaxPointPlaneDist) == (500, 360, 176, 1500, 1.5)
    assert (cfg.MaxPlanes, cfg.MinPlaneSize, cfg.MinPlanarity, cfg.PlaneRatio, cfg.PointDist) == (20, 100, 0.3, 0.5, 5.0)
    assert (cfg.AccumulatorType, cfg.AccumulatorMax, cfg.MinSizeAllPoints, cfg.MaxDist, cfg.MinDist) == (3, 100, 20, 500.0, 50.0)
    assert (cfg.PeakWindow, cfg.WindowSize, cfg.TrashMax, cfg.PlaneDir) == (False, 8, 20, "dat/planes/")
    p = tmp_path / "hough.cfg"
    p.write_text("# RhoNum 7\nRhoNum 20\nPhiNum\t12\nThetaNum 16 \nRhoMax 100\nMaxPointPlaneDist 4.5\nAccumulatorType 1\n"
                 "PlaneRatio 0.25\nPlaneDir out/planes/\nPeakWindow 1\n")
    assert cfg.LoadCfg(str(p)) == 0
    assert (cfg.RhoNum, cfg.PhiNum, cfg.ThetaNum, cfg.RhoMax, cfg.MaxPointPlaneDist) == (20, 12, 16, 100, 4.5)
    assert (cfg.AccumulatorType, cfg.PlaneRatio, cfg.PlaneDir, cfg.PeakWindow, cfg.MaxPlanes) == (1, 0.25, "out/planes/", True, 20)
    assert cfg.dims().tolist() == [20, 12, 16, 100]
    assert hough.ConfigFileHough().LoadCfg(str(tmp_path / "missing.cfg")) == -1
    with pytest.raises(TypeError):
        hough.ConfigFileHough(NoSuchField=1)
