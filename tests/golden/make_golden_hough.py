"""Generator of k22_hough.npz: the standard 3D Hough transform pinned to the reference's compiled accumulators.

    python tests/golden/make_golden_hough.py          (needs the reference checkout: $TDTK_REF, default /root/reference)
    python tests/golden/make_golden_hough.py --time   (the reference's accumulate(Point) per point at its default settings)

COMPILED, where it lies, into a temporary directory: src/shapes/accumulator.cc, ConfigFileHough.cc, parascan.cc and hsm3d.cc
against the reference's own headers (they need nothing else), and calcPlane -- src/shapes/hough.cc from its "double
calcPlane(" to the function's closing brace, cut out when the generator runs -- linked with the newmat objects of
oracle/build_ref.sh (oracle/_ref/obj/nm_*.o; the recipe is run when they are missing).  Flags: build_ref.sh's, plus
-ffp-contract=off said explicitly.  Nothing of it reaches the repository.

RESTATED, in DRIVER around them: feeding points to accumulate(Point), walking getMax()'s multiset, getMax(int* cell), and
deletePoints' first loop (hough.cc:759-779: Normalize3, p.x*n[0] + p.y*n[1] + p.z*n[2] - rho, fabs(..) < MaxPointPlaneDist).

The normals table of a case is normals_table() below, a Python restatement (math.sin / math.cos: the C library's, as the
reference's and the library's own) of the four accumulate(Point) loops; the generator
asserts that votes over it (votes(): the predicate in numpy, fp64, the reference's order of operations) reproduce the
reference's count in every cell and bin.  The inputs are not stored: cases() rebuilds them from seeds, the fixture holds a
digest of each.  On cases marked `public` (counts that a test also takes through tdtk_hough_normals, i.e. through the test
machine's libm) the generator asserts the margin | |d - rho_k| - D | > 16 * 2^-53 * (|px| + |py| + |pz| + rho_k) for every point,
cell and bin -- a normal off by up to 4 ulp per component cannot move a vote -- and redraws a cloud that fails from the next seed.

Also imported by the tests (cases, load, votes ...)."""
import ctypes as C
import hashlib
import math
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
OUT = os.path.join(_HERE, "k22_hough.npz")
REF = os.environ.get("TDTK_REF", "/root/reference")
NM_OBJ = os.path.join(_ROOT, "oracle", "_ref", "obj")
MAX_BYTES = 500 * 1000
FLAGS = "-std=c++17 -O3 -fPIC -fopenmp -DOPENMP -DOPENMP_NUM_THREADS=8 -DMAX_OPENMP_NUM_THREADS=512 -ffp-contract=off -w".split()
SIMPLE, BALL, CUBE, BALLI = 0, 1, 2, 3

CALC_HEAD = r"""
#include "newmat/newmatap.h"
using namespace NEWMAT;
#include "slam6d/point.h"
#include <iostream>
#include <vector>
using namespace std;
"""

DRIVER = r"""
#include "shapes/accumulator.h"
#include "slam6d/globals.icc"
#include <chrono>
#include <cstring>
#include <vector>

double calcPlane(std::vector<Point>& ppoints, double plane[4]);

static ConfigFileHough make_cfg(unsigned rho_num, unsigned phi_num, unsigned theta_num, unsigned rho_max, double D)
{
  ConfigFileHough c;
  c.RhoNum = rho_num; c.PhiNum = phi_num; c.ThetaNum = theta_num; c.RhoMax = rho_max; c.MaxPointPlaneDist = D;
  return c;
}

extern "C" void* hg_new(int type, unsigned rho_num, unsigned phi_num, unsigned theta_num, unsigned rho_max, double D)
{
  ConfigFileHough c = make_cfg(rho_num, phi_num, theta_num, rho_max, D);
  switch (type) {
    case 0: return (Accumulator*)new AccumulatorSimple(c);
    case 1: return (Accumulator*)new AccumulatorBall(c);
    case 2: return (Accumulator*)new AccumulatorCube(c);
    default: return (Accumulator*)new AccumulatorBallI(c);
  }
}
extern "C" void hg_delete(void* a) { delete (Accumulator*)a; }

extern "C" double hg_accumulate(void* a, const double* xyz, long n)
{
  auto t0 = std::chrono::steady_clock::now();
  for (long i = 0; i < n; i++) ((Accumulator*)a)->accumulate(Point(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]));
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// getMax()'s multiset in its order, `width` ints per entry; returns the number of entries
extern "C" long hg_getmax(void* a, int width, int* out, long cap)
{
  std::multiset<int*, maxcompare>* l = ((Accumulator*)a)->getMax();
  long k = 0;
  for (std::multiset<int*, maxcompare>::iterator it = l->begin(); it != l->end(); ++it, ++k) {
    if (k < cap) memcpy(out + (size_t)width * k, *it, sizeof(int) * width);
    delete[] *it;
  }
  delete l;
  return k;
}

extern "C" void hg_cell_plane(void* a, int* cell, double* out4)
{
  double* p = ((Accumulator*)a)->getMax(cell);
  memcpy(out4, p, 4 * sizeof(double));
  delete[] p;
}

// hough.cc:759-779
extern "C" long hg_plane_points(const double* xyz, long n_pts, const double* n_in, double rho, double D, int* idx)
{
  double n[3] = {n_in[0], n_in[1], n_in[2]};
  Normalize3(n);
  long k = 0;
  for (long i = 0; i < n_pts; i++) {
    Point p(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    double distance = p.x * n[0] + p.y * n[1] + p.z*n[2] - rho;
    if (fabs(distance) < D) idx[k++] = (int)i;
  }
  return k;
}

extern "C" double hg_calc_plane(const double* xyz, const int* idx, long m, double* plane4)
{
  std::vector<Point> pts;
  for (long i = 0; i < m; i++) pts.push_back(Point(xyz[3 * idx[i]], xyz[3 * idx[i] + 1], xyz[3 * idx[i] + 2]));
  return calcPlane(pts, plane4);
}
"""


def have_ref():
    return os.path.isfile(os.path.join(REF, "src", "shapes", "accumulator.cc"))


_lib = None
_tmp = None


def ref_lib():
    global _lib, _tmp
    if _lib is None:
        if not os.path.isfile(os.path.join(NM_OBJ, "nm_jacobi.o")):
            subprocess.check_call([os.path.join(_ROOT, "oracle", "build_ref.sh"), REF], stdout=subprocess.DEVNULL)
        _tmp = tempfile.TemporaryDirectory(prefix="k22_ref_")
        d = _tmp.name
        src = open(os.path.join(REF, "src", "shapes", "hough.cc")).read()
        a = src.index("double calcPlane(")
        b = src.index("\n}\n", a) + 3
        with open(os.path.join(d, "calc_plane.cc"), "w") as f:
            f.write(CALC_HEAD + src[a:b])
        with open(os.path.join(d, "driver.cc"), "w") as f:
            f.write(DRIVER)
        inc = ["-I" + os.path.join(REF, "include"), "-I" + os.path.join(REF, "3rdparty", "newmat", "newmat-10")]
        units = [(n, os.path.join(REF, "src", "shapes", n + ".cc")) for n in ("accumulator", "ConfigFileHough", "parascan", "hsm3d")]
        units += [(n, os.path.join(d, n + ".cc")) for n in ("calc_plane", "driver")]
        jobs = [subprocess.Popen(["g++"] + FLAGS + inc + ["-c", path, "-o", os.path.join(d, n + ".o")]) for n, path in units]
        for j in jobs:
            if j.wait():
                raise subprocess.CalledProcessError(j.returncode, j.args)
        nm = sorted(os.path.join(NM_OBJ, f) for f in os.listdir(NM_OBJ) if f.startswith("nm_") and f.endswith(".o"))
        so = os.path.join(d, "libhg.so")
        subprocess.check_call(["g++", "-shared", "-fopenmp", "-Wl,--no-undefined", "-o", so] +
                              [os.path.join(d, n + ".o") for n, _ in units] + nm)
        L = C.CDLL(so)
        L.hg_new.restype = C.c_void_p
        L.hg_new.argtypes = [C.c_int, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_double]
        L.hg_delete.argtypes = [C.c_void_p]
        L.hg_accumulate.restype = C.c_double
        L.hg_accumulate.argtypes = [C.c_void_p, C.c_void_p, C.c_long]
        L.hg_getmax.restype = C.c_long
        L.hg_getmax.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long]
        L.hg_cell_plane.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.hg_plane_points.restype = C.c_long
        L.hg_plane_points.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_double, C.c_double, C.c_void_p]
        L.hg_calc_plane.restype = C.c_double
        L.hg_calc_plane.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]
        _lib = L
    return _lib


def _quiet(fn, *a):
    """the reference's constructors and getMax() print to stdout"""
    sys.stdout.flush()
    keep = os.dup(1)
    null = os.open(os.devnull, os.O_WRONLY)
    os.dup2(null, 1)
    try:
        return fn(*a)
    finally:
        os.dup2(keep, 1)
        os.close(null)
        os.close(keep)


# ---- the accumulators' geometry in numpy ---------------------------------------------------------------------------------------
def _rad(deg):
    return (2 * np.pi * deg) / 360


def _deg(rad):
    return (rad * 360) / (2 * np.pi)


def slice_sizes(case):
    """cells per phi slice (type 2: per face), and BallI's (phi_top_rad, step)"""
    t, P, T = case["type"], case["PhiNum"], case["ThetaNum"]
    if t == SIMPLE:
        return [T] * P, None
    if t == CUBE:
        return [(T // 4) ** 2] * 6, None
    if t == BALL:
        step = 180.0 / P
        max_a = 2 * np.pi * 1.0
        r = math.sin(_rad(0.0))
        out = []
        phi = 0.0
        while phi < 180.0:
            r_next = math.sin(_rad(phi + step))
            a = 2 * np.pi * (r + r_next) / 2.0
            c = (360.0 * (max_a / a)) / (T - 1)
            out.append(int(1.0 + 360.0 / c))
            r = r_next
            phi += step
        assert len(out) == P, "the reference's constructor would write outside ballNr"
        return out, None
    step = 180.0 / P
    h_0 = math.cos(_rad(90 - step))
    max_a = (2.0 * np.pi * h_0) / T
    h_top = max_a / (2.0 * np.pi)
    phi_top_rad = math.acos(1 - h_top)
    phi_top_deg = _deg(phi_top_rad)
    step = (180.0 - 2.0 * phi_top_deg) / float(P - 2.0)
    nr = [-1] * P
    nr[0] = nr[P - 1] = 1
    counter = 1
    phi = phi_top_deg
    while phi < 90:
        h_i = math.cos(_rad(phi)) - math.cos(_rad(phi + step))
        a_i = 2 * np.pi * h_i
        assert 0 < counter <= P - 1
        nr[counter] = nr[P - 1 - counter] = int(a_i / max_a)
        counter += 1
        phi += step
    assert min(nr) >= 0
    return nr, (float(phi_top_rad), float(step))


def _normalize3(n):
    norm = math.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
    return [n[0] / norm, n[1] / norm, n[2] / norm]


def _cube_to_s2(face, i, j, width):
    u = (i - 0.5) / float(width)
    u = u * 2 - 1
    v = (j - 0.5) / float(width)
    v = v * 2 - 1
    r = {1: [1.0, u, v], 4: [-1.0, -u, -v], 2: [u, 1.0, v], 5: [-u, -1.0, -v], 3: [u, v, 1.0], 6: [-u, -v, -1.0]}[face]
    return _normalize3(r)


def normals_table(case):
    """[C][3]: the n of accumulate(Point) per cell, in the order of getMax()'s loops without rho"""
    t, P, R = case["type"], case["PhiNum"], case["RhoNum"]
    sizes, balli = slice_sizes(case)
    out = []
    if t == CUBE:
        w = case["ThetaNum"] // 4
        for f in range(6):
            for j in range(1, w + 1):
                for k in range(1, w + 1):
                    out.append(_normalize3(_cube_to_s2(f + 1, j, k, w)))
        return np.array(out, np.float64).reshape(-1, 3)
    for i in range(P):
        if t == SIMPLE:
            phi = (i + 0.5) * np.pi / (P * 0.99999999999)
        elif t == BALL:
            phi = (i + 0.5) * np.pi / (P * 0.999999999)
        else:
            phi = balli[0] + (i - 0.5) * _rad(balli[1])
        for j in range(sizes[i]):
            theta = (j + 0.5) * 2 * np.pi / sizes[i]
            theta = min(theta, 2 * np.pi)
            phi = min(phi, np.pi)
            if t == BALLI and i == 0:
                out.append([0.0, 0.0, 1.0])
            elif t == BALLI and i == R - 1:
                out.append([0.0, 0.0, -1.0])
            else:
                out.append(_normalize3([math.cos(theta) * math.sin(phi), math.sin(theta) * math.sin(phi), math.cos(phi)]))
    return np.array(out, np.float64).reshape(-1, 3)


def rho_bins(case):
    k = np.arange(case["RhoNum"], dtype=np.float64)
    return (k + 0.5) * float(case["RhoMax"]) / float(case["RhoNum"])


def votes(case, xyz, table, margin=False):
    """counts [C][RhoNum] int32 by the reference's predicate; with margin also the smallest slack of the margin condition"""
    rho = rho_bins(case)
    D = case["D"]
    counts = np.zeros((len(table), case["RhoNum"]), np.int32)
    slack = np.inf
    for c, n in enumerate(table):
        d = xyz[:, 0] * n[0] + xyz[:, 1] * n[1] + xyz[:, 2] * n[2]
        for lo in range(0, len(rho), 4096):
            r = rho[lo:lo + 4096]
            a = np.abs(d[:, None] - r[None, :])
            counts[c, lo:lo + 4096] = (a < D).sum(axis=0)
            if margin and len(xyz):
                bound = 16 * 2.0 ** -53 * (np.abs(xyz).sum(axis=1)[:, None] + r[None, :])
                slack = min(slack, float((np.abs(a - D) - bound).min()))
    return (counts, slack) if margin else counts


def entry_width(case):
    return 5 if case["type"] == CUBE else 4


def counts_from_list(case, lst, sizes):
    """getMax()'s entries -> counts [C][RhoNum]"""
    first = np.concatenate([[0], np.cumsum(sizes)])
    if case["type"] == CUBE:
        w = case["ThetaNum"] // 4
        cell = first[lst[:, 2]] + lst[:, 3] * w + lst[:, 4]
    else:
        cell = first[lst[:, 3]] + lst[:, 2]
    counts = np.full((int(first[-1]), case["RhoNum"]), -1, np.int32)
    counts[cell, lst[:, 1]] = lst[:, 0]
    assert (counts >= 0).all()
    return counts


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def _case(name, type, RhoNum, PhiNum, ThetaNum, RhoMax, D, cloud, ratio=0.5, public=True, **kw):
    return dict(name=name, type=type, RhoNum=RhoNum, PhiNum=PhiNum, ThetaNum=ThetaNum, RhoMax=RhoMax, D=float(D), cloud=cloud,
                ratio=ratio, public=public, **kw)


def case_list():
    out = []
    for t, nm in ((SIMPLE, "simple"), (BALL, "ball"), (CUBE, "cube"), (BALLI, "balli")):
        out.append(_case("types_" + nm, t, 20, 12, 16, 100, 4.0, ("uniform", 400, 60.0), ratio=0.0))
    for n in (0, 1, 63, 64, 65, 1000):
        out.append(_case("n%d" % n, SIMPLE, 20, 4, 5, 100, 4.0, ("uniform", n, 60.0), ratio=0.0))
    for r in (1, 7, 500):
        out.append(_case("rho%d" % r, SIMPLE, r, 4, 5, 100, 4.0, ("uniform", 300, 60.0)))
    out.append(_case("rho50000", SIMPLE, 50000, 2, 2, 100, 0.05, ("uniform", 1000, 60.0), public=False))
    out.append(_case("d_tiny", SIMPLE, 20, 4, 5, 100, 0.05, ("uniform", 1000, 60.0)))              # 0.01 bin
    out.append(_case("d_wide", SIMPLE, 20, 4, 5, 100, 12.5, ("uniform", 300, 60.0)))               # 2.5 bins: five votes
    out.append(_case("half_bin", BALLI, 20, 12, 16, 80, 2.0, ("lattice4", 500, 15), public=False))   # bin 4, D 2, z = 4 j
    out.append(_case("balli_rho7", BALLI, 7, 12, 16, 100, 4.0, ("uniform", 300, 60.0)))            # i == RhoNum - 1: slice 6 votes with (0,0,-1)
    out.append(_case("plane5000", BALL, 20, 12, 16, 100, 4.0, ("plane", 5000, 47, 52.5)))          # one cell receives every point
    out.append(_case("outside", SIMPLE, 20, 4, 5, 100, 4.0, ("uniform", 500, 180.0)))              # d < 0 and d > RhoMax
    out.append(_case("far", BALL, 20, 6, 8, 2000000, 30000.0, ("far", 400, 1.0e6, 60.0)))
    return out


def cloud_of(case, seed_shift=0):
    kind = case["cloud"][0]
    seed = 2200 + 1000 * seed_shift + sum(map(ord, case["name"]))
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        _, n, half = case["cloud"]
        return rng.uniform(-half, half, (n, 3))
    if kind == "far":
        _, n, off, half = case["cloud"]
        return off + rng.uniform(-half, half, (n, 3))
    if kind == "lattice4":
        _, n, span = case["cloud"]
        xyz = rng.uniform(-60, 60, (n, 3))
        xyz[:, 2] = 4.0 * rng.integers(-span, span + 1, n)          # z an exact multiple of the bin width
        return xyz
    _, n, cell, rho = case["cloud"]                                  # points on the plane n_cell . p = rho
    nrm = normals_table(case)[cell]
    a = np.cross(nrm, [0.0, 0.0, 1.0])
    a /= np.linalg.norm(a)
    b = np.cross(nrm, a)
    uv = rng.uniform(-40, 40, (n, 2))
    return np.ascontiguousarray(rho * nrm + uv[:, :1] * a + uv[:, 1:] * b)


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, np.float64).tobytes()).digest()[:8], np.uint64)[0]


def cases(z=None):
    """{name: case with 'xyz'}: the clouds rebuilt from their seeds (the seed shift a redraw needed comes from the fixture)"""
    out = {}
    for c in case_list():
        shift = int(z["%s_shift" % c["name"]]) if z is not None else 0
        c["xyz"] = np.ascontiguousarray(cloud_of(c, shift), np.float64)
        out[c["name"]] = c
    return out


# ---- the reference --------------------------------------------------------------------------------------------------------------
def peak_prefix(lst, ratio):
    """Hough::SHT's loop condition (hough.cc:248-253) on getMax()'s list"""
    mx = int(lst[0, 0])
    thr = int(mx * ratio)
    return lst[lst[:, 0] > thr], mx


def eigen_gap(xyz, idx):
    p = xyz[idx]
    w = np.linalg.eigvalsh(np.cov((p - p.mean(0)).T, bias=True) * len(p))
    w = np.sort(np.abs(w))
    return (w[1] - w[0]) / w[2]


def run_reference(case, xyz):
    """everything the fixture holds of one case, from the compiled reference"""
    L = ref_lib()
    w = entry_width(case)
    acc = _quiet(L.hg_new, case["type"], case["RhoNum"], case["PhiNum"], case["ThetaNum"], case["RhoMax"], case["D"])
    L.hg_accumulate(acc, xyz.ctypes.data, len(xyz))
    sizes, _ = slice_sizes(case)
    total = sum(sizes) * case["RhoNum"]
    lst = np.zeros((total, w), np.int32)
    k = _quiet(L.hg_getmax, acc, w, lst.ctypes.data, total)
    assert k == total, (k, total)
    res = dict(list=lst, counts=counts_from_list(case, lst, sizes))
    peaks, mx = peak_prefix(lst, case["ratio"])
    res["peaks"], res["max"] = peaks, mx
    # planes of the first peaks and of fixed cells (the poles and the last slice of the ball types)
    chosen = [e for e in peaks[:12]]
    if case["type"] != CUBE:
        chosen += [np.array([0, 0, 0, 0], np.int32), np.array([0, case["RhoNum"] - 1, 0, case["PhiNum"] - 1], np.int32),
                   np.array([0, 0, sizes[case["PhiNum"] // 2] - 1, case["PhiNum"] // 2], np.int32)]
    else:
        # getMax(int*) of the cube reads (rho, face - 1, i, j) from cell[0 .. 3]: hand it entries of that form
        chosen = [np.array([e[1], e[2], e[3] + 1, e[4] + 1, 0], np.int32) for e in peaks[:12]]
    cells = np.array(chosen, np.int32).reshape(-1, w)
    planes = np.zeros((len(cells), 4))
    for i in range(len(cells)):
        L.hg_cell_plane(acc, cells[i].ctypes.data, planes[i].ctypes.data)
    res["cells"], res["planes"] = cells, planes
    L.hg_delete(acc)
    # inliers and calcPlane of the first two planes
    inl, fits = [], []
    for i in range(min(2, len(peaks))):
        idx = np.zeros(len(xyz), np.int32)
        m = L.hg_plane_points(xyz.ctypes.data, len(xyz), planes[i].ctypes.data, float(planes[i][3]), case["D"], idx.ctypes.data)
        idx = idx[:m].copy()
        inl.append(idx)
        plane = np.zeros(4)
        planarity = L.hg_calc_plane(xyz.ctypes.data, idx.ctypes.data, m, plane.ctypes.data) if m >= 3 else 0.0
        gap = eigen_gap(xyz, idx) if m >= 3 else 0.0
        fits.append(np.concatenate([plane, [planarity, gap, m]]))
    res["inliers"], res["fits"] = inl, np.array(fits).reshape(-1, 7)
    return res


def compute():
    z = {}
    for c in case_list():
        name = c["name"]
        shift = 0
        while True:
            xyz = np.ascontiguousarray(cloud_of(c, shift), np.float64)
            table = normals_table(c)
            mine, slack = votes(c, xyz, table, margin=True)
            if not c["public"] or slack > 0 or len(xyz) == 0:
                break
            shift += 1
            assert shift < 8, name
        res = run_reference(c, xyz)
        assert np.array_equal(mine, res["counts"]), "%s: the restated table does not reproduce the reference's counts" % name
        z[name + "_shift"] = np.int32(shift)
        z[name + "_sha"] = digest(xyz)
        z[name + "_table"] = table
        z[name + "_counts"] = res["counts"]
        z[name + "_peaks"] = res["peaks"]
        z[name + "_max"] = np.int32(res["max"])
        z[name + "_cells"] = res["cells"]
        z[name + "_planes"] = res["planes"]
        z[name + "_fits"] = res["fits"]
        for i, idx in enumerate(res["inliers"]):
            z["%s_inliers%d" % (name, i)] = idx
        print("%-14s C %5d x %5d  N %5d  max %5d  peaks %5d  votes %8d  shift %d  slack %.2e" %
              (name, len(table), c["RhoNum"], len(xyz), res["max"], len(res["peaks"]), int(res["counts"].sum()), shift, slack))
    check_cases(z)
    return z


def check_cases(z):
    """the properties the cases are there for"""
    cs = cases(z)
    assert z["types_ball_counts"].shape == (118, 20) and z["types_balli_counts"].shape == (118, 20)
    assert z["types_cube_counts"].shape == (96, 20) and z["types_simple_counts"].shape == (192, 20)
    assert z["n0_counts"].sum() == 0 and len(z["n0_peaks"]) == 0
    assert z["rho50000_counts"].shape[1] == 50000 and z["rho50000_counts"].sum() > 0
    t, n = z["d_tiny_counts"].sum(), len(cs["d_tiny"]["xyz"]) * 20
    assert 0 < t < n / 20, t                                            # almost nothing votes
    assert (z["d_wide_counts"].sum(axis=1).max() <= 5 * 300) and z["d_wide_counts"].sum() > 3 * z["rho7_counts"].sum() / 2
    # z a multiple of the bin width 4 and D = 2 exactly half a bin: |z - (4k + 2)| >= 2, so the pole cell (0,0,1) gets no vote
    assert np.array_equal(z["half_bin_table"][0], [0.0, 0.0, 1.0]) and z["half_bin_counts"][0].sum() == 0
    assert z["half_bin_counts"].sum() > 0
    assert (z["balli_rho7_table"][:, 2] == -1.0).sum() > 1              # a whole slice votes with the south pole's normal
    assert z["plane5000_max"] == 5000                                   # one cell and bin receives every point
    xyz, table = cs["outside"]["xyz"], z["outside_table"]
    d = xyz @ table.T
    assert (d < -4).any() and (d > 104).any()
    assert np.abs(cs["far"]["xyz"]).min() > 9e5 and z["far_counts"].sum() > 0
    for name in ("types_ball", "plane5000"):                           # planes that mean something: eigen-gap >= 0.1
        f = z[name + "_fits"]
        assert len(f) and (f[:, 5] >= 0.1).all() and (f[:, 6] >= 3).all(), (name, f)
    ties = z["types_simple_peaks"][:, 0]
    assert (np.diff(ties) == 0).sum() > 10                              # equal counts: the multiset's insertion order matters


class Fixture:
    def __init__(self, z):
        self.z = z
        self.cases = cases(z)
        for name, c in self.cases.items():
            assert z[name + "_sha"] == digest(c["xyz"]), "the inputs of %s are not the ones the fixture was made from" % name

    def get(self, name, what):
        return self.z["%s_%s" % (name, what)]

    def inliers(self, name):
        out = []
        while "%s_inliers%d" % (name, len(out)) in self.z:
            out.append(self.z["%s_inliers%d" % (name, len(out))])
        return out


def load(path=OUT):
    return Fixture(dict(np.load(path)))


def save(z, path=OUT):
    """np.savez_compressed with nothing in the file that depends on when it was written"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for k in sorted(z):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(z[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            zf.writestr(zi, buf.getvalue(), compresslevel=9)


BENCH = dict(type=BALLI, RhoNum=500, PhiNum=176, ThetaNum=360, RhoMax=1500, D=1.5, points=100)


def time_reference(xyz=None):
    """seconds per point of the reference's accumulate(Point) at its default settings, one host thread"""
    L = ref_lib()
    if xyz is None:
        xyz = np.random.default_rng(22).uniform(-300, 300, (BENCH["points"], 3))
    xyz = np.ascontiguousarray(xyz, np.float64)
    acc = _quiet(L.hg_new, BENCH["type"], BENCH["RhoNum"], BENCH["PhiNum"], BENCH["ThetaNum"], BENCH["RhoMax"], BENCH["D"])
    sec = L.hg_accumulate(acc, xyz.ctypes.data, len(xyz))
    L.hg_delete(acc)
    return sec / len(xyz)


if __name__ == "__main__":
    if not have_ref():
        raise SystemExit("needs the reference checkout at %s (src/shapes/accumulator.cc)" % REF)
    if "--time" in sys.argv:
        t = time.perf_counter()
        per = time_reference()
        print("reference accumulate(Point), type 3, RhoNum 500, PhiNum 176, ThetaNum 360 (this host, one thread): %.3f s per point "
              "(%d points in %.1f s); 1M points: %.0f s" % (per, BENCH["points"], time.perf_counter() - t, per * 1e6))
        raise SystemExit(0)
    z = compute()
    save(z)
    size = os.path.getsize(OUT)
    print("wrote %s (%d arrays, %d bytes)" % (OUT, len(z), size))
    assert size <= MAX_BYTES, size
