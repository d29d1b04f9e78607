"""Generator of k20_boctree_search.npz: BOctTree<double> as a SEARCH tree (`slam6D -t 2`) from the reference's own compiled
class -- the constructor with earlystop (include/slam6d/Boctree.h:224-270, branch :1164-1195), init() (:333-356) and
FindClosest (:1573-1681, findClosestInLeaf :1361-1379) -- on clouds chosen for the places a restatement by reading goes wrong:
the early stop at exactly 10 points, `>=` against `>` on centre planes, truncation toward zero of negative voxel coordinates,
the clamp of the descent box, the order of visits per octant, a search stopped by a point within 0.01, the strict `<` of the
leaf scan at maxdist2 == d2, the 10 000-leaf limit.

    python tests/golden/make_golden_boctree_search.py        (needs the reference checkout, found as make_golden_octree.py finds it)

Built exactly as make_golden_octree.py builds its library (whose stand-ins, flags and packing this file imports): Boctree.cc
and allocator.cc are compiled where they lie, next to a driver of our own (DRIVER below), into a temporary directory; nothing
of them reaches the repository.  The driver reads the protected search state (params[0].count, .closest_d2) and init()'s
scalars through a subclass.

Per case (cloud, voxel, earlystop), key prefix <cloud>_v<voxel>_e<0|1>_:
  scalars    max_depth, real_voxelSize, mult, add[3], largest_index, size, center[3]   (float64 [11], the ints exact)
  counts     countNodes, countOctLeaves, countPoints
  leaf       AllPoints as cloud rows (the smallest row with those coordinates; coordinates = cloud[leaf])
and per batch b of the case (queries <cloud>_q<b>, maxdist2 in <..>_b<b>_maxd2):
  pos        position in `leaf` of the FIRST point with the returned coordinates, -1 for NULL: what strict `<` returns, so
             exact duplicates need no case left out
  d2         params[0].closest_d2 after the call (maxdist2 when nothing was accepted)
  leaves     params[0].count: leaves scanned
`visits` [8][8]: for every octant of the query the order in which FindClosest scans the eight leaf children of a root -- data
the program produced: the search is run 64 times on trees whose child k alone holds a point within 0.01 of the query, which
ends the search (closest_v = 0), and params[0].count then says how many leaves were scanned before and with child k.

Also imported by the tests (RefBoct, load, CASES, clouds ...), so that fixture and live reference are checked the same way."""
import ctypes as C
import importlib.util
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def _sibling(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


mo = _sibling("make_golden_octree")

OUT = os.path.join(_HERE, "k20_boctree_search.npz")
MAX_BYTES = mo.MAX_BYTES
REF = mo.REF
have_ref = mo.have_ref

DRIVER = r"""
#include <cstdlib>
#include <cstring>
#include <vector>
#include "slam6d/Boctree.h"

// the default point type: coordinates only
PointType::PointType() { types = 0; pointdim = 3; for (int i = 0; i < 10; i++) dimensionmap[i] = 1; }
unsigned int PointType::getPointDim() { return pointdim; }

// SearchTree's three out-of-line virtuals (searchTree.h:83-112): with them the class's vtable and typeinfo are emitted here
double* SearchTree::FindClosestAlongDir(double*, double*, double, int) const { return 0; }
void SearchTree::getPtPairs(std::vector<PtPair>*, double*, double* const*, unsigned int, unsigned int, int, int, double,
                            double&, double*, double*) {}
void SearchTree::getPtPairs(std::vector<PtPair>*, double*, const DataXYZ&, const DataNormal&, unsigned int, unsigned int, int,
                            int, double, double&, double*, double*, PairingMode) {}

struct Probe : public BOctTree<double> {
  Probe(double* const* pts, int n, double voxel, bool early) : BOctTree<double>(pts, n, voxel, PointType(), early) {}
  void scalars(double* o) const
  {
    o[0] = max_depth; o[1] = real_voxelSize; o[2] = mult; o[3] = add[0]; o[4] = add[1]; o[5] = add[2]; o[6] = largest_index;
    o[7] = size; o[8] = center[0]; o[9] = center[1]; o[10] = center[2];
  }
  int scanned() const { return params[0].count; }
  double best_d2() const { return params[0].closest_d2; }
};

extern "C" void* bs_create(const double* xyz, int n, double voxel, int early)
{
  double** pts = new double*[n ? n : 1];
  for (int i = 0; i < n; i++) {
    pts[i] = new double[3];
    memcpy(pts[i], xyz + 3 * (size_t)i, 3 * sizeof(double));
  }
  Probe* t = new Probe(pts, n, voxel, early != 0);        // the leaves hold copies of the coordinates
  for (int i = 0; i < n; i++) delete[] pts[i];
  delete[] pts;
  return t;
}
extern "C" void bs_destroy(void* h) { delete (Probe*)h; }
extern "C" void bs_info(void* h, double* scalars11, long* counts3)
{
  Probe* t = (Probe*)h;
  t->scalars(scalars11);
  counts3[0] = t->countNodes(); counts3[1] = t->countOctLeaves(); counts3[2] = t->countPoints();
}
extern "C" long bs_all_points(void* h, double* out)
{
  std::vector<double*> c;
  ((Probe*)h)->AllPoints(c);
  for (size_t i = 0; i < c.size(); i++) { memcpy(out + 3 * i, c[i], 3 * sizeof(double)); delete[] c[i]; }
  return (long)c.size();
}
// FindClosest(q[i], maxd2, 0): found[i], the returned coordinates, closest_d2 and count afterwards
extern "C" void bs_find(void* h, const double* q, int K, double maxd2, int* found, double* xyz, double* d2, int* leaves)
{
  Probe* t = (Probe*)h;
  for (int i = 0; i < K; i++) {
    double p[3] = {q[3 * i], q[3 * i + 1], q[3 * i + 2]};
    double* c = static_cast<SearchTree*>(t)->FindClosest(p, maxd2, 0);     // protected in BOctTree: called as slam6D calls it
    found[i] = c != 0;
    for (int a = 0; a < 3; a++) xyz[3 * i + a] = c ? c[a] : 0.0;
    d2[i] = t->best_d2();
    leaves[i] = t->scanned();
  }
}
"""

_lib = None
_tmp = None


def ref_lib():
    """Boctree.cc + allocator.cc + DRIVER, built into a temporary directory (removed at exit)"""
    global _lib, _tmp
    if _lib is None:
        _tmp = tempfile.TemporaryDirectory(prefix="k20_ref_")
        d = _tmp.name
        os.makedirs(os.path.join(d, "standin", "boost", "interprocess"))
        with open(os.path.join(d, "standin", "boost", "interprocess", "offset_ptr.hpp"), "w") as f:
            f.write(mo.OFFSET_PTR)
        with open(os.path.join(d, "driver.cc"), "w") as f:
            f.write(DRIVER)
        inc = ["-I" + os.path.join(REF, "include"), "-I" + os.path.join(REF, "3rdparty", "newmat", "newmat-10"),
               "-I" + os.path.join(d, "standin")]
        jobs = []
        for src, obj in ((os.path.join(REF, "src", "slam6d", "Boctree.cc"), "Boctree.o"),
                         (os.path.join(REF, "src", "slam6d", "allocator.cc"), "allocator.o"),
                         (os.path.join(d, "driver.cc"), "driver.o")):
            jobs.append(subprocess.Popen(["g++"] + mo.FLAGS + inc + ["-c", src, "-o", os.path.join(d, obj)]))
        for j in jobs:
            if j.wait():
                raise subprocess.CalledProcessError(j.returncode, j.args)
        so = os.path.join(d, "libbs.so")
        subprocess.check_call(["g++", "-shared", "-fopenmp", "-Wl,--no-undefined", "-o", so] +
                              [os.path.join(d, o) for o in ("Boctree.o", "allocator.o", "driver.o")])
        _lib = C.CDLL(so)
        _lib.bs_create.restype = C.c_void_p
        _lib.bs_create.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int]
        _lib.bs_destroy.argtypes = [C.c_void_p]
        _lib.bs_info.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.bs_all_points.restype = C.c_long
        _lib.bs_all_points.argtypes = [C.c_void_p, C.c_void_p]
        _lib.bs_find.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double] + [C.c_void_p] * 4
    return _lib


class RefBoct:
    """the reference's BOctTree<double>(pts, n, voxel, PointType(), earlystop)"""

    def __init__(self, pts, voxel, earlystop):
        self.pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        self.h = ref_lib().bs_create(self.pts.ctypes.data, len(self.pts), float(voxel), int(bool(earlystop)))

    def __del__(self):
        if getattr(self, "h", None):
            ref_lib().bs_destroy(self.h)
            self.h = None

    def info(self):
        s, c = np.empty(11), np.empty(3, np.int64)
        ref_lib().bs_info(self.h, s.ctypes.data, c.ctypes.data)
        return s, c

    def all_points(self):
        out = np.empty_like(self.pts)
        m = ref_lib().bs_all_points(self.h, out.ctypes.data)
        assert m == len(self.pts)
        return out

    def find(self, q, maxd2):
        """(found [K] bool, coordinates [K][3], closest_d2 [K], leaves scanned [K])"""
        q = np.ascontiguousarray(q, np.float64).reshape(-1, 3)
        K = len(q)
        found, xyz, d2, leaves = np.empty(K, np.int32), np.empty((K, 3)), np.empty(K), np.empty(K, np.int32)
        ref_lib().bs_find(self.h, q.ctypes.data, K, float(maxd2), found.ctypes.data, xyz.ctypes.data, d2.ctypes.data, leaves.ctypes.data)
        return found.astype(bool), xyz, d2, leaves


# ---- clouds and queries -------------------------------------------------------------------------------------------------
# Everything lies on binary grids (a few bytes of a double each), so that the fixture can hold it.
SIGNS = np.array([[(1.0 if o & 1 else -1.0), (1.0 if o & 2 else -1.0), (1.0 if o & 4 else -1.0)] for o in range(8)])
LIMIT_R2 = 26.0 ** 2                      # the leaf-limit case's maxdist2
LIMIT_LEAVES = 10400                      # one-point leaves the query meets before its partner's


def limit_cloud():
    """More than 10 000 one-point leaves inside the Chebyshev bound and outside the Euclidean radius of the query
    (-0.5, -0.5, -0.5), all in the seven octants the search visits before the one that holds the only partner, (1, 1, 1).
    Root cube: centre 0, half edge 32; voxel 1 gives leaves of edge 2, one odd-integer lattice point each."""
    q = np.array([-0.5, -0.5, -0.5])
    g = np.arange(-31.0, 32.0, 2.0)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    d2 = ((lat - q) ** 2).sum(1)
    # a leaf is scanned when the Chebyshev distance from the query's voxel (31 of 64 per axis; the points are their leaves'
    # centres) to its box is at most closest_v = 27: |p + 1| - 1 <= 27
    cheb = np.abs(lat + 1.0).max(1)
    keep = (d2 > LIMIT_R2 + 1.0) & (cheb <= 28.0) & ~(lat > 0).all(1)
    lat, d2 = lat[keep], d2[keep]
    shell = lat[np.argsort(d2, kind="stable")[:LIMIT_LEAVES]]
    return np.concatenate([[[-31.0, -31.0, -31.0], [31.0, 31.0, 31.0], [1.0, 1.0, 1.0]], shell])


def clouds():
    rng = np.random.default_rng(20)
    c = {}
    c["uniform"] = rng.integers(-50 * 16, 50 * 16, (3000, 3)) / 16.0
    # clusters of 9, 10, 11 and 12 points next to each other, at three scales (= depths): the early stop happens at exactly 10
    parts = []
    for scale, origin in ((8.0, (-200.0, -200.0, -200.0)), (0.5, (40.0, 10.0, -30.0)), (1.0 / 32, (300.0, 300.0, 250.0))):
        for j, cnt in enumerate((9, 10, 11, 12, 10, 11)):
            base = np.array(origin) + scale * 4.0 * np.array([j % 2, (j // 2) % 2, j // 4])
            parts.append(base + scale * rng.integers(0, 64, (cnt, 3)) / 64.0)
    c["clusters"] = np.concatenate(parts)
    lat = rng.integers(0, 63, (2000, 3)).astype(np.float64)       # root half size exactly 32, root centre 31
    lat[0], lat[1] = 0.0, 62.0
    c["lattice62"] = lat
    # octants: for the query 4 * sign of every octant six points at distance 6 along the axes (three of them across a centre
    # plane), the cube's corners keep the root centre at 0
    oc = [20.0 * SIGNS]
    for o in range(8):
        q = 4.0 * SIGNS[o]
        oc.append(np.array([q + 6.0 * s * np.eye(3)[a] for a in range(3) for s in (-1.0, 1.0)]))
    c["octants"] = np.concatenate(oc)
    # stop: a point within 0.01 of the query on the query's side of the root's x plane, a nearer one just across it
    bg = rng.integers(-40 * 4, 40 * 4, (600, 3)) / 4.0
    bg = bg[np.abs(bg).max(1) > 2.0]
    c["stop"] = np.concatenate([[[-40.0, -40.0, -40.0], [40.0, 40.0, 40.0]], bg,
                                [[-2.0 ** -8 - 2.0 ** -7, 0.25, 0.25], [2.0 ** -9, 0.25, 0.25]]])
    c["duplicates"] = rng.permutation(np.repeat(rng.integers(0, 10 * 256, (150, 3)) / 256.0, 7, 0))
    c["one"] = np.array([[3.0, -2.0, 7.5]])
    c["two"] = np.array([[-1.0, -2.0, -3.0], [1.0, 2.0, 3.0]])
    c["limit"] = limit_cloud()
    return {k: np.ascontiguousarray(v, np.float64) for k, v in c.items()}


def queries(c):
    """per cloud the query batches [(queries, maxdist2-or-None)]; None: filled in by edge_batches from the reference's d2"""
    rng = np.random.default_rng(21)
    q = {}
    u = c["uniform"]
    inside = rng.integers(-55 * 16, 55 * 16, (200, 3)) / 16.0
    # outside the root cube on every side: negative voxel coordinates, the clamp
    out = np.concatenate([s * 70.0 * np.eye(3)[a] + rng.integers(-40, 40, (4, 3)) * 1.0 for a in range(3) for s in (-1.0, 1.0)])
    far = np.array([[-300.0, 0.0, 0.0], [0.0, 400.0, 0.0], [200.0, 200.0, 200.0], [-51.0625, -51.0, -51.0]])
    q["uniform"] = [(np.concatenate([inside, u[:40], out]), 625.0),        # branching mostly at the root
                    (np.concatenate([inside[:80], out]), 4.0),             # the descent ends in missing children
                    (np.concatenate([inside[:60], out, far]), 250000.0)]   # the box covers the whole cube
    cl = c["clusters"]
    q["clusters"] = [(np.concatenate([cl[::3], cl[::5] + 2.0 ** -6, np.rint(cl.mean(0))[None]]), 625.0),
                     (np.concatenate([cl[::4] + 2.0 ** -4]), 1e6)]
    lat = c["lattice62"]
    planes = np.array([[x, y, z] for x in (31.0, 15.0, 47.0, 7.0) for y in (31.0, 15.0) for z in (31.0, 30.5, 31.5)])
    q["lattice62"] = [(np.concatenate([planes, lat[:100], lat[100:160] + 0.5, [[-0.5, -0.5, -0.5], [-1.0, 31.0, 63.5]]]), 9.0),
                      (planes, 2500.0)]
    q["octants"] = [(np.concatenate([4.0 * SIGNS, 2.0 ** -4 * SIGNS, np.zeros((1, 3))]), 1e4)]
    st = c["stop"]
    q["stop"] = [(np.concatenate([[[-2.0 ** -8, 0.25, 0.25], [2.0 ** -10, 0.25, 0.25]], st[2:42] + 2.0 ** -5]), 625.0)]
    d = c["duplicates"]
    q["duplicates"] = [(np.concatenate([d[:60], d[60:100] + 2.0 ** -5]), 100.0)]
    q["one"] = [(np.array([[3.0, -2.0, 7.5], [2.0, -2.0, 7.5], [30.0, 0.0, 0.0]]), 625.0),
                (np.array([[3.0, -2.0, 7.5], [2.0, -2.0, 7.5]]), 1.0)]
    q["two"] = [(np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0], [-1.0, -2.0, -2.5], [9.0, 9.0, 9.0]]), 625.0)]
    q["limit"] = [(np.array([[-0.5, -0.5, -0.5], [0.5, 0.5, 0.5]]), LIMIT_R2)]
    return {k: [(np.ascontiguousarray(a, np.float64), m) for a, m in v] for k, v in q.items()}


# (cloud, ((voxel, earlystop), ...)), in the fixture's order
CASES = (("uniform", ((10.0, 1), (1.0, 0))), ("clusters", ((10.0, 1), (0.01, 1), (0.01, 0))), ("lattice62", ((2.0, 0), (2.0, 1), (10.0, 1))),
         ("octants", ((10.0, 1), (1.0, 0))), ("stop", ((10.0, 1), (0.5, 0))), ("duplicates", ((10.0, 1), (0.125, 0))),
         ("one", ((10.0, 1), (0.1, 0))), ("two", ((10.0, 1), (0.1, 0))), ("limit", ((1.0, 0),)))
# maxdist2 exactly d2 and one ulp above it: the queries of batch 0 of these cases again, each at its own radius (one call per query)
EDGE_CASES = (("uniform", 10.0, 1), ("lattice62", 2.0, 0), ("duplicates", 0.125, 0))
EDGE_QUERIES = 24


def prefix(name, voxel, early):
    return "%s_v%g_e%d_" % (name, voxel, early)


def first_pos(pts, leaf, coords, found):
    """position in `leaf` of the first point with exactly those coordinates, -1 where nothing was found"""
    first = {}
    for pos, r in enumerate(leaf):
        first.setdefault(pts[r].tobytes(), pos)
    return np.array([first[np.ascontiguousarray(x).tobytes()] if f else -1 for x, f in zip(coords, found)], np.int32)


def observe_visits():
    """[octant][i] = the child scanned i-th by a query in that octant, at a root with eight leaf children (see the docstring)"""
    order = np.full((8, 8), -1, np.int64)
    for k in range(8):
        pts = np.concatenate([20.0 * SIGNS, 2.0 ** -9 * SIGNS[k][None]])       # child k also holds a point at the centre
        t = RefBoct(pts, 1e6, False)
        s, cnt = t.info()
        assert s[0] == 1 and cnt[0] == 1 and cnt[1] == 8
        for o in range(8):
            found, xyz, d2, leaves = t.find(2.0 ** -10 * SIGNS[o][None], 1e6)
            assert found[0] and d2[0] <= 0.0001 and np.array_equal(xyz[0], pts[8])
            assert order[o, leaves[0] - 1] == -1
            order[o, leaves[0] - 1] = k
    assert (np.sort(order, 1) == np.arange(8)).all()
    return order


def case_rows(pts, voxel, early, batches, edge):
    """one case's arrays from the live reference, by their key suffix"""
    t = RefBoct(pts, voxel, early)
    z = {}
    z["scalars"], z["counts"] = t.info()
    leaf = mo.rep_index(pts, t.all_points())
    z["leaf"] = leaf.astype(np.int32)
    for b, (q, maxd2) in enumerate(batches):
        found, xyz, d2, leaves = t.find(q, maxd2)
        z["b%d_maxd2" % b] = np.array(maxd2)
        z["b%d_pos" % b] = first_pos(pts, leaf, xyz, found)
        z["b%d_d2" % b] = d2
        z["b%d_leaves" % b] = leaves
    if edge:
        q, maxd2 = batches[0]
        found, _, d2, _ = t.find(q, maxd2)
        rows = np.flatnonzero(found & (d2 > 0.0))[:EDGE_QUERIES]
        assert len(rows) == EDGE_QUERIES
        z["edge_rows"] = rows.astype(np.int32)
        for tag, radius in (("at", d2[rows]), ("above", np.nextafter(d2[rows], np.inf))):
            out = [t.find(q[r][None], m) for r, m in zip(rows, radius)]
            z["edge_%s_pos" % tag] = first_pos(pts, leaf, [o[1][0] for o in out], [o[0][0] for o in out])
            z["edge_%s_d2" % tag] = np.array([o[2][0] for o in out])
            z["edge_%s_leaves" % tag] = np.array([o[3][0] for o in out], np.int32)
    return z


def check_properties(c, q, z):
    """what the cases are there for, asserted on the reference's own answers"""
    def rows(name, voxel, early, b):
        p = prefix(name, voxel, early)
        return z[p + "leaf"], z[p + "b%d_pos" % b], z[p + "b%d_d2" % b], z[p + "b%d_leaves" % b]
    # the early stop: more leaves without it, the same points
    p1, p0 = prefix("clusters", 0.01, 1), prefix("clusters", 0.01, 0)
    assert z[p1 + "counts"][1] < z[p0 + "counts"][1] and z[p1 + "counts"][2] == z[p0 + "counts"][2] == len(c["clusters"])
    # a stopped search: the first query gets the point within 0.01 although a nearer one exists
    leaf, pos, d2, _ = rows("stop", 10.0, 1, 0)
    pts, q0 = c["stop"], q["stop"][0][0][0]
    assert 0.0 < d2[0] <= 0.0001 and ((pts - q0) ** 2).sum(1).min() < d2[0]
    # the leaf limit: 10 000 leaves scanned, nothing returned, although the partner lies inside the radius; from the
    # partner's own octant it is found at once
    leaf, pos, d2, leaves = rows("limit", 1.0, 0, 0)
    assert leaves[0] == 10000 and pos[0] == -1 and d2[0] == LIMIT_R2
    assert ((c["limit"][2] - q["limit"][0][0][0]) ** 2).sum() < LIMIT_R2
    assert pos[1] >= 0 and leaf[pos[1]] == 2
    # maxdist2 == d2 returns something else or nothing; one ulp above returns the point
    for name, voxel, early in EDGE_CASES:
        p = prefix(name, voxel, early)
        r = z[p + "edge_rows"]
        assert np.array_equal(z[p + "edge_above_pos"], z[p + "b0_pos"][r]) and np.array_equal(z[p + "edge_above_d2"], z[p + "b0_d2"][r])
        assert (z[p + "edge_at_pos"] != z[p + "b0_pos"][r]).all()
    # queries outside the cube, a descent that ends in a missing child (no leaf scanned, nothing found), branching at the root
    _, pos, _, leaves = rows("uniform", 10.0, 1, 1)
    assert ((pos == -1) & (leaves == 0)).any()
    _, pos, _, leaves = rows("uniform", 10.0, 1, 2)
    assert (pos >= 0).all() and leaves.max() > 50


def compute():
    c, z = clouds(), {}
    q = queries(c)
    z["visits"] = observe_visits().astype(np.int8)
    edges = set(EDGE_CASES)
    for name, variants in CASES:
        pts = c[name]
        z[name], z[name + "_g"] = mo._pack(pts)
        for b, (qq, _) in enumerate(q[name]):
            z["%s_q%d" % (name, b)], z["%s_q%d_g" % (name, b)] = mo._pack(qq)
        for voxel, early in variants:
            for k, v in case_rows(pts, voxel, early, q[name], (name, voxel, early) in edges).items():
                z[prefix(name, voxel, early) + k] = v
    check_properties(c, q, z)
    return z


class Fixture:
    def __init__(self, z):
        self.z = z
        self.visits = z["visits"].astype(np.int64)

    def cases(self):
        return [(name, voxel, early) for name, variants in CASES for voxel, early in variants]

    def cloud(self, name):
        return mo._unpack(self.z[name], self.z[name + "_g"])

    def batches(self, name, voxel, early):
        """[(queries, maxdist2, pos, d2, leaves)]"""
        p, out, b = prefix(name, voxel, early), [], 0
        while "%s_q%d" % (name, b) in self.z:
            qq = mo._unpack(self.z["%s_q%d" % (name, b)], self.z["%s_q%d_g" % (name, b)])
            out.append((qq, float(self.z[p + "b%d_maxd2" % b]), self.z[p + "b%d_pos" % b], self.z[p + "b%d_d2" % b], self.z[p + "b%d_leaves" % b]))
            b += 1
        return out

    def get(self, name, voxel, early, key):
        return self.z[prefix(name, voxel, early) + key]

    def edge(self, name, voxel, early):
        """[(query, maxdist2, pos, d2, leaves)], one query each"""
        qq = self.batches(name, voxel, early)[0][0]
        p, out = prefix(name, voxel, early), []
        rows = self.z[p + "edge_rows"]
        base = self.z[p + "b0_d2"][rows]
        for tag, radius in (("at", base), ("above", np.nextafter(base, np.inf))):
            for i, r in enumerate(rows):
                out.append((qq[r], float(radius[i]), int(self.z[p + "edge_%s_pos" % tag][i]), float(self.z[p + "edge_%s_d2" % tag][i]),
                            int(self.z[p + "edge_%s_leaves" % tag][i])))
        return out


def load(path=OUT):
    return Fixture(dict(np.load(path)))


if __name__ == "__main__":
    if not have_ref():
        raise SystemExit("needs the reference checkout at %s (src/slam6d/Boctree.cc)" % REF)
    z = compute()
    mo.save(z, OUT)
    size = os.path.getsize(OUT)
    print("wrote %s (%d arrays, %d bytes)" % (OUT, len(z), size))
    for k in sorted(z, key=lambda k: -z[k].nbytes)[:8]:
        print("  %-40s %s %s" % (k, z[k].dtype, z[k].shape))
    assert size <= MAX_BYTES, size
