"""Generator of k17_peopleremover.npz: the reference's free-space carving (src/peopleremover) -- the ordered voxel lists of
walk_voxels and the result of the whole pipeline (mask, free set, the four printed counts, visitor calls) -- on rays and
scenes chosen for the places a restatement by reading goes wrong.

    python tests/golden/make_golden_peopleremover.py          (needs the reference checkout: $TDTK_REF, default /root/reference)
    python tests/golden/make_golden_peopleremover.py --time   (the reference's time for tools/query_bench.py's workload)

COMPILED, where it lies: the part of src/peopleremover/common.cc before the first `validate` -- std::hash<voxel>, py_div,
py_mod, voxel_of_point, visitor and walk_voxels -- against the reference's own include/peopleremover/common.h, with the
flags of oracle/build_ref.sh.  The generator cuts that part into its temporary build directory when it runs (the rest of the
file is the command line and compute_maxranges, which need Boost and the quadtree); nothing of it reaches the repository.
common.h includes Boost, scanio, scan.h, normals.h and the spherical quadtree, none of which this image can build, so
stand-in headers of our own (STANDINS below, in the temporary directory only) satisfy those includes: boost::hash_combine,
and forward declarations for boost::any, the program_options and iostreams namespaces, IOType, QuadTree and DataXYZ.  The
compiled functions use none of them but hash_combine, which only orders an unordered_map's buckets.

RESTATED, in DRIVER around those compiled functions, citing the lines: what lives in main() -- the occupancy map
(peopleremover.cc:176-191), the ray loop (:286-323, serial, maxrange method NONE), the cluster filter (:337-418, the
incremental merging as written), the half-free voxels (:420-468) and the classification (:534-545).

The inputs are not stored: cases() rebuilds them from fixed seeds (numpy's PCG64 stream is stable), and the fixture holds a
digest of every input array so that a drift would be seen.  Voxel lists are stored as each ray's first voxel and one byte per
further visit (consecutive visits differ by at most 1 per axis; asserted).

Also imported by the tests (cases, Ref, load ...), so that the fixture and the live reference are checked the same way."""
import ctypes as C
import hashlib
import importlib
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
OUT = os.path.join(_HERE, "k17_peopleremover.npz")
REF = os.environ.get("TDTK_REF", "/root/reference")
MAX_BYTES = 500 * 1000
FLAGS = "-std=c++17 -O3 -fPIC -fopenmp -DOPENMP -DOPENMP_NUM_THREADS=8 -DMAX_OPENMP_NUM_THREADS=512 -w".split()

STANDINS = {
    "boost/functional/hash.hpp": r"""
#pragma once
#include <cstddef>
#include <functional>
namespace boost {
template <class T> inline void hash_combine(std::size_t& seed, const T& v)
{ seed ^= std::hash<T>()(v) + 0x9e3779b9 + (seed << 6) + (seed >> 2); }
}
""",
    "boost/program_options.hpp": "#pragma once\n#include <string>\n#include <vector>\nnamespace boost { class any; namespace program_options {} }\n",
    "boost/iostreams/device/mapped_file.hpp": "#pragma once\nnamespace boost { namespace iostreams {} }\n",
    "scanio/scan_io.h": "#pragma once\n#include <string>\n#include <vector>\nclass IOType;\n",
    "slam6d/normals.h": "#pragma once\n",
    "slam6d/scan.h": "#pragma once\n#include <math.h>\n#include <algorithm>\nclass DataXYZ;\n",      # the real one brings fmod and std::min
    "spherical_quadtree/spherical_quadtree.h": "#pragma once\nclass QuadTree;\n",
}

DRIVER = r"""
#include <peopleremover/common.h>
#include <chrono>
#include <cstdint>
#include <cstring>

static bool list_visitor(struct voxel v, void* data)
{
  ((std::vector<struct voxel>*)data)->push_back(v);
  return true;
}

// walk_voxels under a visitor that records and always continues; returns the number of visits, writes at most cap
extern "C" long pr_walk(const double* s, const double* e, double vs, long cap, long* out)
{
  std::vector<struct voxel> l;
  walk_voxels(s, e, vs, list_visitor, &l);
  for (long i = 0; i < (long)l.size() && i < cap; i++) { out[3 * i] = l[i].x; out[3 * i + 1] = l[i].y; out[3 * i + 2] = l[i].z; }
  return (long)l.size();
}

extern "C" void pr_voxel_of_point(const double* p, double vs, long* out)
{
  struct voxel v = voxel_of_point(p, vs);
  out[0] = v.x; out[1] = v.y; out[2] = v.z;
}

struct counted { struct visitor_args a; uint64_t calls; };
static bool counting_visitor(struct voxel v, void* data)
{
  struct counted* c = (struct counted*)data;
  c->calls += 1;
  return visitor(v, &c->a);
}

static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// main() of peopleremover.cc between reading the scans and writing the partition.  xyz [n][3], scan i owns rows off[i] ..
// off[i+1]; ends null or [n][3] (the p of :290-302 where a maxrange shortens the ray).  info: occupied, freed, free after
// clustering, half-free, visitor calls.  seconds: occupancy, walk, cluster + half-free + classification.
extern "C" long pr_run(const double* xyz, const uint64_t* off, const double* origins, const double* ends, size_t S,
                       double voxel_size, size_t diff, size_t cluster_size, int no_subvoxel_accuracy, uint8_t* dynamic,
                       long* free_out, long cap, uint64_t* info, double* seconds)
{
  double t0 = now();
  // :176-191
  std::unordered_map<struct voxel, std::set<size_t>> voxel_occupied_by_slice;
  for (size_t s = 0; s < S; ++s)
    for (size_t i = off[s]; i < off[s + 1]; ++i)
      voxel_occupied_by_slice[voxel_of_point(xyz + 3 * i, voxel_size)].insert(s);
  info[0] = voxel_occupied_by_slice.size();
  double t1 = now();
  // :222-323
  std::set<struct voxel> free_voxels;
  uint64_t calls = 0;
  for (size_t i = 0; i < S; ++i) {
    std::set<struct voxel> free;
    for (size_t j = off[i]; j < off[i + 1]; ++j) {
      double p[3] = {xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2]};
      if (ends) { p[0] = ends[3 * j]; p[1] = ends[3 * j + 1]; p[2] = ends[3 * j + 2]; }
      struct counted data = {};
      data.a.empty_voxels = &free;
      data.a.voxel_occupied_by_slice = &voxel_occupied_by_slice;
      data.a.current_slice = i;
      data.a.diff = diff;
      walk_voxels(origins + 3 * i, p, voxel_size, counting_visitor, &data);
      calls += data.calls;
    }
    for (struct voxel v : free) free_voxels.insert(v);
  }
  info[1] = free_voxels.size();
  info[4] = calls;
  double t2 = now();
  // :337-418
  if (cluster_size > 1) {
    std::unordered_map<struct voxel, size_t> voxel_to_cluster;
    std::unordered_map<size_t, std::set<struct voxel>> cluster_to_voxel;
    size_t i = 0;
    for (const struct voxel v : free_voxels) {
      std::set<size_t> neighbor_clusters;
      int vradius = 1;
      for (int i = 0 - vradius; i <= vradius; ++i)
        for (int j = 0 - vradius; j <= vradius; ++j)
          for (int k = 0 - vradius; k <= vradius; ++k) {
            if (i == 0 && j == 0 && k == 0) continue;
            std::unordered_map<struct voxel, size_t>::iterator it2 = voxel_to_cluster.find(voxel(v.x + i, v.y + j, v.z + k));
            if (it2 != voxel_to_cluster.end()) neighbor_clusters.insert(it2->second);
          }
      if (neighbor_clusters.size() == 0) {
        voxel_to_cluster[v] = i;
        cluster_to_voxel[i].insert(v);
        i += 1;
        continue;
      }
      if (neighbor_clusters.size() == 1) {
        size_t cluster = *(neighbor_clusters.begin());
        voxel_to_cluster[v] = cluster;
        cluster_to_voxel[cluster].insert(v);
        i += 1;
        continue;
      }
      size_t mincluster = *(neighbor_clusters.begin());
      for (size_t cluster : neighbor_clusters) {
        if (cluster == mincluster) continue;
        for (struct voxel v2 : cluster_to_voxel[cluster]) {
          voxel_to_cluster[v2] = mincluster;
          cluster_to_voxel[mincluster].insert(v2);
        }
        cluster_to_voxel.erase(cluster);
      }
      voxel_to_cluster[v] = mincluster;
      cluster_to_voxel[mincluster].insert(v);
      i += 1;
    }
    for (std::pair<size_t, std::set<struct voxel>> p : cluster_to_voxel) {
      if (p.second.size() >= cluster_size) continue;
      for (struct voxel voxel : p.second) free_voxels.erase(voxel);
    }
  }
  info[2] = free_voxels.size();
  // :420-468
  std::unordered_map<struct voxel, std::set<size_t>> half_voxels;
  if (!no_subvoxel_accuracy) {
    for (struct voxel v : free_voxels) {
      int vradius = 2;
      for (int i = 0 - vradius; i <= vradius; ++i)
        for (int j = 0 - vradius; j <= vradius; ++j)
          for (int k = 0 - vradius; k <= vradius; ++k) {
            if (i == 0 && j == 0 && k == 0) continue;
            struct voxel neighbor = voxel(v.x + i, v.y + j, v.z + k);
            if (free_voxels.find(neighbor) != free_voxels.end()) continue;
            if (voxel_occupied_by_slice.find(neighbor) == voxel_occupied_by_slice.end()) continue;
            for (size_t num : voxel_occupied_by_slice[v]) half_voxels[neighbor].insert(num);
          }
    }
  }
  info[3] = half_voxels.size();
  // :534-545
  for (size_t i = 0; i < S; ++i)
    for (size_t j = off[i]; j < off[i + 1]; ++j) {
      struct voxel voxel = voxel_of_point(xyz + 3 * j, voxel_size);
      dynamic[j] = (free_voxels.find(voxel) != free_voxels.end() ||
                    (half_voxels.find(voxel) != half_voxels.end() && half_voxels[voxel].find(i) != half_voxels[voxel].end())) ? 1 : 0;
    }
  double t3 = now();
  if (seconds) { seconds[0] = t1 - t0; seconds[1] = t2 - t1; seconds[2] = t3 - t2; }
  long k = 0;
  for (struct voxel v : free_voxels) {      // std::set order
    if (k < cap) { free_out[3 * k] = v.x; free_out[3 * k + 1] = v.y; free_out[3 * k + 2] = v.z; }
    k += 1;
  }
  return k;
}
"""


def have_ref():
    return os.path.isfile(os.path.join(REF, "src", "peopleremover", "common.cc"))


_lib = None
_tmp = None


def ref_lib():
    """the head of common.cc + DRIVER, built into a temporary directory (removed at exit)"""
    global _lib, _tmp
    if _lib is None:
        _tmp = tempfile.TemporaryDirectory(prefix="k17_ref_")
        d = _tmp.name
        for rel, text in STANDINS.items():
            os.makedirs(os.path.join(d, "standin", os.path.dirname(rel)), exist_ok=True)
            with open(os.path.join(d, "standin", rel), "w") as f:
                f.write(text)
        src = open(os.path.join(REF, "src", "peopleremover", "common.cc")).read()
        cut = src.index("void validate(")
        with open(os.path.join(d, "common_head.cc"), "w") as f:
            f.write(src[:cut])
        with open(os.path.join(d, "driver.cc"), "w") as f:
            f.write(DRIVER)
        inc = ["-I" + os.path.join(d, "standin"), "-I" + os.path.join(REF, "include")]
        jobs = [subprocess.Popen(["g++"] + FLAGS + inc + ["-c", os.path.join(d, n + ".cc"), "-o", os.path.join(d, n + ".o")])
                for n in ("common_head", "driver")]
        for j in jobs:
            if j.wait():
                raise subprocess.CalledProcessError(j.returncode, j.args)
        so = os.path.join(d, "libpr.so")
        subprocess.check_call(["g++", "-shared", "-fopenmp", "-Wl,--no-undefined", "-o", so, os.path.join(d, "common_head.o"),
                               os.path.join(d, "driver.o")])
        _lib = C.CDLL(so)
        _lib.pr_walk.restype = C.c_long
        _lib.pr_walk.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_long, C.c_void_p]
        _lib.pr_voxel_of_point.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
        _lib.pr_run.restype = C.c_long
        _lib.pr_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_size_t, C.c_size_t,
                                C.c_int, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p]
    return _lib


class Ref:
    """the compiled reference"""

    @staticmethod
    def walk(starts, ends, vs):
        """(counts [m], voxels [total][3] int64)"""
        L = ref_lib()
        s = np.ascontiguousarray(starts, np.float64).reshape(-1, 3)
        e = np.ascontiguousarray(ends, np.float64).reshape(-1, 3)
        counts, lists = np.zeros(len(s), np.int64), []
        buf = np.empty((1 << 16, 3), np.int64)
        for i in range(len(s)):
            k = L.pr_walk(s[i].ctypes.data, e[i].ctypes.data, float(vs), len(buf), buf.ctypes.data)
            assert k <= len(buf)
            counts[i] = k
            lists.append(buf[:k].copy())
        return counts, (np.concatenate(lists) if lists else np.zeros((0, 3), np.int64))

    @staticmethod
    def run(case, seconds=None):
        """(dynamic [n] uint8, free [k][3] int64, info [5])"""
        L = ref_lib()
        xyz = np.ascontiguousarray(np.concatenate(case["scans"]))
        off = np.zeros(len(case["scans"]) + 1, np.uint64)
        off[1:] = np.cumsum([len(s) for s in case["scans"]])
        org = np.ascontiguousarray(case["origins"], np.float64)
        ends = np.ascontiguousarray(np.concatenate(case["ends"])) if case.get("ends") is not None else None
        dyn = np.zeros(len(xyz), np.uint8)
        info = np.zeros(5, np.uint64)
        free = np.zeros((len(xyz), 3), np.int64)
        k = L.pr_run(xyz.ctypes.data, off.ctypes.data, org.ctypes.data, ends.ctypes.data if ends is not None else None,
                     len(case["scans"]), float(case["vs"]), int(case["diff"]), int(case["cluster"]),
                     0 if case["subvoxel"] else 1, dyn.ctypes.data, free.ctypes.data, len(free), info.ctypes.data,
                     seconds.ctypes.data if seconds is not None else None)
        return dyn, free[:k].copy(), info


def _pr():
    if _ROOT not in sys.path:
        sys.path.insert(0, _ROOT)
    return importlib.import_module("3dtk_amd.peopleremover")


# ---- the cases --------------------------------------------------------------------------------------------------------------
VOXEL_SIZES = (0.1, 10.0, 1.0 / 3.0)


def _shapes():
    """rays in voxel units (scaled by each voxel size): (starts, ends)"""
    s, e = [], []

    def ray(a, b):
        s.append(a)
        e.append(b)
    c = (0.5, 0.5, 0.5)
    # one and two zero direction components
    ray(c, (7.3, 0.5, -4.2)); ray(c, (0.5, -6.1, 3.7)); ray(c, (-5.5, 2.25, 0.5))
    ray(c, (0.5, -9.7, 0.5)); ray(c, (8.2, 0.5, 0.5)); ray(c, (0.5, 0.5, -3.0)); ray((2.0, 1.0, 3.0), (2.0, 1.0, -4.0))
    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                sg = np.array([sx, sy, sz], float)
                ray(c, tuple(np.array(c) + 4 * sg))                        # centre diagonal: three axes step together
                ray((2.0, 2.0, 2.0), tuple(2.0 + 3 * sg))                  # corner to corner
                ray((-1.0, -2.0, -3.0), tuple(np.array([-1.0, -2.0, -3.0]) + 3 * sg))
                ray(c, tuple(np.array(c) + sg * (4, 4, 0.3)))              # two axes together, the third creeping
                ray(c, tuple(np.array(c) + sg * (0.3, 3, 3)))
                ray(c, tuple(np.array(c) + sg * (5, 0.2, 5)))
                ray(c, tuple(np.array(c) + sg * (6, 3, 2)))                # pairs meet at some crossings
                ray((1.0, 1.0, 0.5), tuple(np.array([1.0, 1.0, 0.5]) + sg * (0, 0, 5)))      # along an edge
                ray((1.0, 0.5, 1.0), tuple(np.array([1.0, 0.5, 1.0]) + sg * (3, 0, 3)))      # in a face, through edges
    # negative steps that start exactly on a boundary (:155), each axis, pairs, all three
    for m in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1)):
        a = np.where(np.array(m) == 1, 2.0, 0.5)
        ray(tuple(a), tuple(a - np.where(np.array(m) == 1, 3.5, -0.2 - 0.1 * np.arange(3))))
        ray(tuple(a), tuple(a - np.where(np.array(m) == 1, 0.5, 1.7)))      # the adjusted voxel is the end voxel
        ray(tuple(-a), tuple(-a - np.where(np.array(m) == 1, 2.25, 0.0)))
    ray((0.2, 0.2, 0.2), (0.8, 0.7, 0.6))                                   # start and end in one voxel
    ray((-0.2, -0.9, -0.5), (-0.8, -0.1, -0.6))
    ray((1.25, -3.5, 2.0), (1.25, -3.5, 2.0))                               # zero length: nothing
    ray((-7.3, -2.2, -9.9), (-1.1, -8.6, -0.4)); ray((-0.5, -0.5, -0.5), (-6.5, -3.5, -1.5)); ray((-3.0, -3.0, -3.0), (3.0, 3.0, 3.0))
    return np.array(s, np.float64), np.array(e, np.float64)


def walk_cases():
    """[(name, voxel_size, starts [m][3], ends [m][3])]"""
    out = []
    s, e = _shapes()
    for vs in VOXEL_SIZES + (1.0,):
        out.append(("shapes_v%g" % vs, vs, s * vs, e * vs))
    # ~2000 voxels per axis sum: accumulated tMax would drift from mult * tDelta
    out.append(("long_v0.1", 0.1, np.array([[0.037, 0.011, 0.093], [90.0, -40.0, 13.0]]),
                np.array([[140.013, 90.077, -60.04], [-55.5, 41.3, -20.7]])))
    out.append(("long_v0.333", 1.0 / 3.0, np.array([[0.1, 0.2, 0.3]]), np.array([[333.3, -222.2, 111.1]])))
    big = 1.0e6
    out.append(("near1e6_v1", 1.0, np.array([[big + 0.3, big - 0.7, -big + 0.2], [big, big, big], [-big, -big + 0.5, big + 3.25]]),
                np.array([[big + 7.9, big + 3.2, -big - 4.4], [big - 5.0, big - 5.0, big - 5.0], [-big - 6.1, -big + 0.5, big - 2.0]])))
    # voxel_of_point where a / b rounds to an integer: py_div is the truncated quotient corrected by fmod's sign, not floor
    k = np.arange(1, 400, dtype=np.float64)
    for vs in (0.1, 1.0 / 3.0):
        p = np.concatenate([-(k * vs), -(k / (1.0 / vs)), k * vs, -(k * vs) * (1 + 2.0 ** -52)])
        s = np.stack([p, p[::-1], p], axis=1)
        out.append(("pydiv_v%g" % vs, vs, s, s + np.array([0.0, 0.0, 2.5 * vs])))
    rng = np.random.default_rng(1717)
    out.append(("random_v0.1", 0.1, rng.uniform(-50, 50, (2048, 3)) * 0.1, rng.uniform(-50, 50, (2048, 3)) * 0.1))
    # on a quarter-voxel lattice: boundaries, edges and corners are hit all the time
    out.append(("lattice_v10", 10.0, rng.integers(-200, 201, (2048, 3)) * 2.5, rng.integers(-200, 201, (2048, 3)) * 2.5))
    return out


def _case(name, scans, origins, vs=10.0, diff=0, cluster=5, subvoxel=True, ends=None):
    return dict(name=name, scans=[np.ascontiguousarray(s, np.float64).reshape(-1, 3) for s in scans],
                origins=np.ascontiguousarray(origins, np.float64).reshape(-1, 3), vs=vs, diff=diff, cluster=cluster,
                subvoxel=subvoxel, ends=ends)


def _through(origin, centre, k):
    """the point at k times the way from origin through centre"""
    o, c = np.array(origin, float), np.array(centre, float)
    return o + (c - o) * k


def pipeline_cases():
    room = _pr().synthetic_room
    out = []
    scans, org = room(3, 2500, moving=False, seed=3)
    for diff in (0, 1):
        out.append(_case("room3_d%d" % diff, scans, org, diff=diff))
    out.append(_case("room3_c1_nosub", scans, org, cluster=1, subvoxel=False))
    short = [o + (s - o) * 0.7 for s, o in zip(scans, org)]
    out.append(_case("room3_ray_ends", scans, org, ends=short))
    scans, org = room(70, 200, moving=True, seed=70)
    for diff in (0, 3, 100):
        out.append(_case("many70_d%d" % diff, scans, org, diff=diff, cluster=2))
    # the scanner's own voxel (1,0,0) and the next one (0,0,0) -- the start lies on a boundary, the step is negative -- are
    # occupied by the current scan: both visitor results are ignored, the walk goes on and frees scan 1's voxel (-3,0,0)
    s0 = np.array([[15.0, 5.0, 5.0], [5.0, 5.0, 5.0], [-55.0, 5.0, 5.0]])
    s1 = np.array([[-25.0, 5.0, 5.0], [-24.0, 6.0, 4.0]])
    for sub in (False, True):
        out.append(_case("own_voxel_sub%d" % sub, [s0, s1], [[10.0, 5.0, 5.0], [-25.0, 5.0, 100.0]], cluster=1, subvoxel=sub))
    # free components of 4 and 5 voxels in rows, two single voxels touching by a corner, one alone: scan 1 holds them, scan
    # 0 looks through each of them at a floor far below
    rows = [(x, 0, 5) for x in range(0, 4)] + [(x, 6, 5) for x in range(0, 5)] + [(10, 0, 5), (11, 1, 6)] + [(20, 10, 5)]
    cen = (np.array(rows, float) + 0.5) * 10.0
    o0 = np.array([55.0, 35.0, 5000.0])
    floor = np.array([_through(o0, c, 1.03) for c in cen])
    o1 = np.array([-400.0, -300.0, 55.0])
    for cl in (1, 2, 5):
        out.append(_case("clusters_c%d" % cl, [floor, cen], [o0, o1], cluster=cl, subvoxel=False))
    # v = (0,0,5) is freed (scan 1 only, scan 0 looks through); w = (2,0,5), at distance 2, holds scans 1 and 2: with subvoxel
    # accuracy scan 1's points in w are dynamic, scan 2's are not
    v, w = np.array([5.0, 5.0, 55.0]), np.array([25.0, 5.0, 55.0])
    o0 = np.array([5.0, 5.0, 5000.0])
    sc0 = np.array([_through(o0, v, 1.03)])
    sc1 = np.array([v, w + (1.0, 1.0, 1.0)])
    sc2 = np.array([w, w + (-2.0, 2.0, 0.5)])
    for sub in (True, False):
        out.append(_case("halffree_sub%d" % sub, [sc0, sc1, sc2], [o0, [-2000.0, 5.0, 55.0], [25.0, 3000.0, 55.0]], cluster=1,
                         subvoxel=sub))
    return out


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, np.float64).tobytes())
    return np.frombuffer(h.digest()[:8], np.uint64)[0]


# ---- packing of voxel lists -----------------------------------------------------------------------------------------------
def pack_lists(counts, vox):
    """-> (first [rays with visits][3] int32, codes [total - those rays] uint8): code = 9 (dx+1) + 3 (dy+1) + (dz+1)"""
    counts = np.asarray(counts, np.int64)
    off = np.concatenate([[0], np.cumsum(counts)])
    heads = off[:-1][counts > 0]
    d = np.diff(vox, axis=0, prepend=vox[:1])
    keep = np.ones(len(vox), bool)
    keep[heads] = False
    d = d[keep]
    assert np.abs(d).max(initial=0) <= 1
    codes = (9 * (d[:, 0] + 1) + 3 * (d[:, 1] + 1) + (d[:, 2] + 1)).astype(np.uint8)
    first = vox[heads].astype(np.int32)
    assert np.array_equal(unpack_lists(counts, first, codes), vox)
    return first, codes


def unpack_lists(counts, first, codes):
    counts = np.asarray(counts, np.int64)
    total = int(counts.sum())
    off = np.concatenate([[0], np.cumsum(counts)])
    heads = off[:-1][counts > 0]
    d = np.zeros((total, 3), np.int64)
    keep = np.ones(total, bool)
    keep[heads] = False
    c = codes.astype(np.int64)
    d[keep] = np.stack([c // 9 - 1, (c // 3) % 3 - 1, c % 3 - 1], axis=1)
    run = np.cumsum(d, axis=0)
    # restart at every head: subtract the running sum at the head, add the head's voxel
    base = np.zeros((total, 3), np.int64)
    if len(heads):
        seg = np.repeat(np.arange(len(heads)), counts[counts > 0])
        base = first.astype(np.int64)[seg] - run[heads][seg]
    return run + base


def check_cases(res):
    """the properties the pipeline cases are there for, on the reference's results {name: (dyn, free, info)}"""
    fr = lambda n: set(map(tuple, res[n][1].tolist()))     # noqa: E731
    assert res["room3_d0"][0].any() and not res["room3_d0"][0].all()
    assert res["room3_d0"][2][1] > res["room3_d0"][2][2] > 0 and res["room3_d0"][2][3] > 0
    assert res["room3_ray_ends"][2][1] < res["room3_d0"][2][1]
    assert len({tuple(res["many70_d%d" % d][0].tolist()) for d in (0, 3, 100)}) == 3
    assert (-3, 0, 0) in fr("own_voxel_sub0") and (1, 0, 0) not in fr("own_voxel_sub0")
    assert [len(fr("clusters_c%d" % c)) for c in (1, 2, 5)] == [12, 11, 5], [len(fr("clusters_c%d" % c)) for c in (1, 2, 5)]
    assert (20, 10, 5) not in fr("clusters_c2") and (11, 1, 6) in fr("clusters_c2")
    assert fr("halffree_sub1") == {(0, 0, 5)} and res["halffree_sub1"][2][3] == 1 and res["halffree_sub0"][2][3] == 0
    assert res["halffree_sub1"][0].tolist() == [0, 1, 1, 0, 0] and res["halffree_sub0"][0].tolist() == [0, 1, 0, 0, 0]


def compute():
    z = {}
    for name, vs, s, e in walk_cases():
        counts, vox = Ref.walk(s, e, vs)
        first, codes = pack_lists(counts, vox)
        z["walk_" + name + "_counts"] = counts.astype(np.int32)
        z["walk_" + name + "_first"] = first
        z["walk_" + name + "_codes"] = codes
        z["walk_" + name + "_sha"] = digest([s, e])
    res = {}
    for case in pipeline_cases():
        dyn, free, info = Ref.run(case)
        res[case["name"]] = (dyn, free, info)
        z["run_" + case["name"] + "_dyn"] = np.packbits(dyn)
        z["run_" + case["name"] + "_free"] = free.astype(np.int32)
        z["run_" + case["name"] + "_info"] = info
        z["run_" + case["name"] + "_sha"] = digest(case["scans"] + [case["origins"]] + (case["ends"] or []))
    check_cases(res)
    return z


class Fixture:
    def __init__(self, z):
        self.z = z

    def walk(self, name):
        """(counts [m] int64, voxels [total][3] int64)"""
        counts = self.z["walk_" + name + "_counts"].astype(np.int64)
        return counts, unpack_lists(counts, self.z["walk_" + name + "_first"], self.z["walk_" + name + "_codes"])

    def walk_sha(self, name):
        return self.z["walk_" + name + "_sha"]

    def run(self, case):
        """(dynamic [n] uint8, free [k][3] int64, info [5] uint64)"""
        n = sum(len(s) for s in case["scans"])
        name = case["name"]
        assert self.z["run_" + name + "_sha"] == digest(case["scans"] + [case["origins"]] + (case["ends"] or [])), \
            "the inputs of %s are not the ones the fixture was made from" % name
        return (np.unpackbits(self.z["run_" + name + "_dyn"])[:n], self.z["run_" + name + "_free"].astype(np.int64),
                self.z["run_" + name + "_info"])


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


BENCH = dict(n_scans=8, points_per_scan=250000, seed=17)       # tools/query_bench.py --only-peopleremover


def time_reference(runs=3):
    scans, org = _pr().synthetic_room(BENCH["n_scans"], BENCH["points_per_scan"], seed=BENCH["seed"])
    case = _case("bench", scans, org)
    best = None
    for _ in range(runs):
        sec = np.zeros(3)
        t = time.perf_counter()
        dyn, free, info = Ref.run(case, sec)
        total = time.perf_counter() - t
        if best is None or total < best[0]:
            best = (total, sec.copy(), info.copy(), int(dyn.sum()))
    total, sec, info, nd = best
    print("reference (this host, one thread), %d scans x %d points, voxel 10, diff 0, cluster 5, subvoxel:" %
          (BENCH["n_scans"], BENCH["points_per_scan"]))
    print("  occupancy %.1f ms, walk %.1f ms, cluster + half-free + classification %.1f ms, end to end %.1f ms (min of %d)" %
          (1e3 * sec[0], 1e3 * sec[1], 1e3 * sec[2], 1e3 * total, runs))
    print("  occupied %d freed %d after clustering %d half-free %d visits %d (%.1f M visits/s) dynamic points %d" %
          (info[0], info[1], info[2], info[3], info[4], info[4] / sec[1] / 1e6, nd))


if __name__ == "__main__":
    if not have_ref():
        raise SystemExit("needs the reference checkout at %s (src/peopleremover/common.cc)" % REF)
    if "--time" in sys.argv:
        time_reference()
        raise SystemExit(0)
    z = compute()
    save(z)
    size = os.path.getsize(OUT)
    print("wrote %s (%d arrays, %d bytes)" % (OUT, len(z), size))
    for k in sorted(z, key=lambda k: -z[k].nbytes)[:8]:
        print("  %-40s %s %s" % (k, z[k].dtype, z[k].shape))
    assert size <= MAX_BYTES, size
