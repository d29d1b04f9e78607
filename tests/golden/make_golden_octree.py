"""Generator of k14_octree.npz: the octree reduction (Scan::calcReducedPoints, scan.cc:560-603) from the reference's own
BOctTree<double> (include/slam6d/Boctree.h, src/slam6d/Boctree.cc, src/slam6d/allocator.cc), on clouds chosen for the places a
restatement by reading can go wrong: points on centre planes, signed zeros, the `size <= voxel` leaf condition, the
within-leaf order the in-place z / y / x partitions leave, the drawing rule of GetOctTreeRandom, the root cube, 21 levels.

    python tests/golden/make_golden_octree.py        (needs the reference checkout: $TDTK_REF, default /root/reference)

Boctree.cc and allocator.cc are compiled where they lie, next to a driver of our own (DRIVER below), into a temporary
directory and loaded through ctypes; nothing of them reaches the repository.  Three things stand in for what this image
cannot build, all of them our own text and none of them part of what is being tested:
  * boost/interprocess/offset_ptr.hpp (OFFSET_PTR below), the one Boost header Boctree.h includes: a plain pointer wrapper.
    Boctree.h uses offset_ptr for six members (root, uroot, mins, maxs and the two child_bit_depth tables) so that a tree
    can live in shared memory; in one address space a raw pointer addresses the same objects, and no arithmetic of the
    tree goes through it.
  * PointType::PointType() and PointType::getPointDim(): point_type.cc pulls in scan.h and Boost threads.  The bodies say
    what the default point type is (xyz only, pointdim 3), which is all the tree reads from it.
  * SearchTree's three out-of-line virtuals (searchTree.h:83-112), empty, so that the class's vtable is emitted (as in
    make_golden_knn_range.py).  The reduction never calls them.
The flags are those of oracle/build_ref.sh (-O3, OpenMP); Boctree.h compiles with them as it is.

The driver builds the tree as Scan::calcReducedPoints does -- BOctTree<double>(pts, n, voxel, PointType()), the array
constructor over one allocation per point -- and copies the result out before the tree is deleted (the random modes return
pointers into the tree).  Three kinds of rows per (cloud, voxel):
  centres   GetOctTreeCenter: the coordinates
  leaf      GetOctTreeRandom(c, 2**30, false): no leaf has more points, so the reference returns every point of every leaf,
            depth-first and in within-leaf order, without one rand() call
  d1, d3    GetOctTreeRandom(c) and GetOctTreeRandom(c, 3, false) after srand(SEED)
The reference returns coordinates.  Every returned point is bit-equal to a point of the cloud (asserted), so a row is the
smallest cloud index with those coordinates: coords = pts[row].  To keep the file small the rows are packed (compute()'s
docstring says how) and read through load(), which undoes it.
rand_probe holds the first 8 values of rand() after srand(SEED) in the generating process: the drawn rows hold for a C
library that gives these.

Also imported by the tests (RefOct, load, CASES ...), so that the fixture and the live reference are checked the same way."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

OUT = os.path.join(_HERE, "k14_octree.npz")
REF = os.environ.get("TDTK_REF", "/root/reference")
SEED = 4711
ALL = 2 ** 30            # nrpts of the leaf rows
MAX_BYTES = 500 * 1000
# points of a large cloud.  The file's size is mostly entropy: a leaf row is a permutation of the cloud (~1.8 bytes per point
# and row after deflate, 13 such rows), a random cloud ~4 bytes per point even on a coarse grid, the centres of a fine voxel
# as much again.  With 20 000 points the file has 2 MB as plain arrays, with 12 000 and all the packing below 580 KB; 10 000
# points fit the 500 KB bound.  That is 40 blocks of 256 threads per pass, and 1 250 points per leaf in the eight-leaf cases.
N_LARGE = 10000

# the flags of oracle/build_ref.sh
FLAGS = "-std=c++17 -O3 -fPIC -fopenmp -DOPENMP -DOPENMP_NUM_THREADS=8 -DMAX_OPENMP_NUM_THREADS=512 -w".split()

# (cloud, voxels), in the fixture's order
CASES = (("lattice62", (0.5, 1.0, 2.0, 25.0)), ("lattice62_negzero", (1.0, 25.0)), ("halfplane", (1.0, 25.0)),
         ("uniform", (0.5, 10.0, 1e6)), ("clusters", (0.001, 10.0)), ("duplicates", (1.0, 1e6)), ("deep21", (0.0005,)),
         ("same", (0.1, 10.0)), ("one", (0.1, 10.0)), ("two", (0.1, 10.0)))
DEEP22_VOXEL = 0.0004    # deep21 at this voxel has 22 levels: the device refuses it, no row is stored

OFFSET_PTR = r"""
#pragma once
#include <cstddef>
// stand-in for boost::interprocess::offset_ptr inside one address space: a raw pointer with the operations Boctree.h uses
namespace boost { namespace interprocess {
template <class T> class offset_ptr {
  T* p;
public:
  offset_ptr() : p(0) {}
  offset_ptr(T* q) : p(q) {}
  offset_ptr& operator=(T* q) { p = q; return *this; }
  T& operator*() const { return *p; }
  T* operator->() const { return p; }
  T& operator[](std::ptrdiff_t i) const { return p[i]; }
  T* get() const { return p; }
  operator T*() const { return p; }
};
}}
"""

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

// Scan::calcReducedPoints (scan.cc:560-603).  nrpts 0: centres, 1: GetOctTreeRandom(c), > 1: GetOctTreeRandom(c, nrpts, false);
// seed >= 0: srand(seed) right before that call.  out [n][3]; returns the number of rows.
extern "C" long ro_reduce(const double* xyz, int n, double voxel, unsigned int nrpts, long seed, double* out)
{
  double** pts = new double*[n ? n : 1];
  for (int i = 0; i < n; i++) {
    pts[i] = new double[3];
    memcpy(pts[i], xyz + 3 * (size_t)i, 3 * sizeof(double));
  }
  BOctTree<double>* oct = new BOctTree<double>(pts, n, voxel, PointType());
  std::vector<double*> c;
  if (seed >= 0) srand((unsigned int)seed);
  if (nrpts == 0) oct->GetOctTreeCenter(c);
  else if (nrpts == 1) oct->GetOctTreeRandom(c);
  else oct->GetOctTreeRandom(c, nrpts, false);
  long m = (long)c.size();
  for (long i = 0; i < m; i++) memcpy(out + 3 * i, c[i], 3 * sizeof(double));
  if (nrpts == 0) for (long i = 0; i < m; i++) delete[] c[i];
  delete oct;
  for (int i = 0; i < n; i++) delete[] pts[i];
  delete[] pts;
  return m;
}

extern "C" void ro_rand_probe(unsigned int seed, int k, int* out)
{
  srand(seed);
  for (int i = 0; i < k; i++) out[i] = rand();
}
"""


def have_ref():
    return os.path.isfile(os.path.join(REF, "src", "slam6d", "Boctree.cc"))


_lib = None
_tmp = None


def ref_lib():
    """Boctree.cc + allocator.cc + DRIVER, built into a temporary directory (removed at exit)"""
    global _lib, _tmp
    if _lib is None:
        _tmp = tempfile.TemporaryDirectory(prefix="k14_ref_")
        d = _tmp.name
        os.makedirs(os.path.join(d, "standin", "boost", "interprocess"))
        with open(os.path.join(d, "standin", "boost", "interprocess", "offset_ptr.hpp"), "w") as f:
            f.write(OFFSET_PTR)
        with open(os.path.join(d, "driver.cc"), "w") as f:
            f.write(DRIVER)
        inc = ["-I" + os.path.join(REF, "include"), "-I" + os.path.join(REF, "3rdparty", "newmat", "newmat-10"),
               "-I" + os.path.join(d, "standin")]
        jobs = []
        for src, obj in ((os.path.join(REF, "src", "slam6d", "Boctree.cc"), "Boctree.o"),
                         (os.path.join(REF, "src", "slam6d", "allocator.cc"), "allocator.o"),
                         (os.path.join(d, "driver.cc"), "driver.o")):
            jobs.append(subprocess.Popen(["g++"] + FLAGS + inc + ["-c", src, "-o", os.path.join(d, obj)]))
        for j in jobs:
            if j.wait():
                raise subprocess.CalledProcessError(j.returncode, j.args)
        so = os.path.join(d, "libro.so")
        subprocess.check_call(["g++", "-shared", "-fopenmp", "-Wl,--no-undefined", "-o", so] +
                              [os.path.join(d, o) for o in ("Boctree.o", "allocator.o", "driver.o")])
        _lib = C.CDLL(so)
        _lib.ro_reduce.restype = C.c_long
        _lib.ro_reduce.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_uint, C.c_long, C.c_void_p]
        _lib.ro_rand_probe.argtypes = [C.c_uint, C.c_int, C.c_void_p]
    return _lib


class RefOct:
    """the reference's BOctTree<double> reduction"""

    @staticmethod
    def _run(pts, voxel, nrpts, seed):
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        out = np.empty_like(pts)
        m = ref_lib().ro_reduce(pts.ctypes.data, len(pts), float(voxel), int(nrpts), int(seed), out.ctypes.data)
        return out[:m].copy()

    @staticmethod
    def centres(pts, voxel):
        return RefOct._run(pts, voxel, 0, -1)

    @staticmethod
    def random(pts, voxel, nrpts, seed):
        """nrpts >= 1; srand(seed) right before the call"""
        assert nrpts >= 1
        return RefOct._run(pts, voxel, nrpts, seed)


def rand_probe(seed=SEED, k=8):
    """the first k values of this process's rand() after srand(seed)"""
    libc = C.CDLL(None)
    libc.srand(C.c_uint(seed))
    return np.array([libc.rand() for _ in range(k)], np.int32)


def depth_of(pts, voxel):
    """levels below the root (Boctree.h:248-268, :1166): the root's children always exist, a child of half size <= voxel is a leaf"""
    pts = np.asarray(pts, np.float64)
    size = float((0.5 * (pts.max(0) - pts.min(0))).max() + 1.0)
    d, sz = 1, size / 2.0
    while sz > voxel:
        sz /= 2.0
        d += 1
    return d


def clouds(n=None):
    """the clouds by name; n: points of a large one.  The random ones lie on binary grids (a few bytes of a double each), so
    that the fixture can hold them; the clouds of full-mantissa doubles are those of the device-against-oracle tests, which
    test_octree_reference_host.py ties to the reference."""
    n = N_LARGE if n is None else n
    rng = np.random.default_rng(14)
    c = {}
    lat = rng.integers(0, 63, (n, 3)).astype(np.float64)
    lat[0], lat[1] = 0.0, 62.0                 # root half size exactly 32, root centre 31
    c["lattice62"] = lat
    nz = lat - 31.0
    nz[nz == 0.0] = -0.0
    c["lattice62_negzero"] = nz
    hp = rng.integers(0, 63, (n, 3)).astype(np.float64)
    hp[:, 2] = 31.0
    hp[0], hp[1] = 0.0, 62.0
    c["halfplane"] = hp
    c["uniform"] = rng.integers(-50 * 16, 50 * 16, (n, 3)) / 16.0
    k = n // 3
    c["clusters"] = np.concatenate([m + np.rint(rng.normal(0.0, 0.01, (cnt, 3)) * 2.0 ** 14) / 2.0 ** 14 for m, cnt in
                                    ((np.array([-1000.0, 0.0, 0.0]), k), (np.array([0.0, 1000.0, 7.0]), k),
                                     (np.array([1000.0, 0.0, 0.0]), n - 2 * k))])
    c["duplicates"] = rng.permutation(np.repeat(rng.integers(0, 10 * 256, (300, 3)) / 256.0, 7, 0))
    c["deep21"] = np.concatenate([rng.integers(0, 2 ** 12, (5000, 3)) / 2.0 ** 12,
                                  np.repeat(rng.integers(0, 2 ** 16, (50, 3)) / 2.0 ** 26, 4, 0),      # [0, 1e-3)
                                  [[2000.0, 2000.0, 2000.0]]])
    c["same"] = np.tile([[5.0, 5.0, 5.0]], (1000, 1))
    c["one"] = np.array([[3.0, -2.0, 7.5]])
    c["two"] = np.array([[-1.0, -2.0, -3.0], [1.0, 2.0, 3.0]])
    return {k: np.ascontiguousarray(v, np.float64) for k, v in c.items()}


def check_clouds(c):
    """the properties the cases are there for"""
    for name in ("lattice62", "lattice62_negzero", "halfplane"):
        p = c[name]
        assert np.array_equal(0.5 * (p.min(0) + p.max(0)), [31.0 if name != "lattice62_negzero" else 0.0] * 3)
        assert (0.5 * (p.max(0) - p.min(0))).max() + 1.0 == 32.0
    lat = c["lattice62"]
    for centre in (31.0, 15.0, 7.0, 3.0, 1.0):                    # centre planes of five successive levels
        assert (lat == centre).any(0).all()
    assert depth_of(lat, 2.0) == 4 and depth_of(lat, 2.0 + 1e-9) == 4 and depth_of(lat, 2.0 - 1e-9) == 5
    nz = c["lattice62_negzero"]
    assert (np.signbit(nz) & (nz == 0.0)).any() and not ((nz == 0.0) & ~np.signbit(nz)).any()
    assert (c["halfplane"][2:, 2] == 31.0).all()
    assert depth_of(c["uniform"], 1e6) == 1
    assert depth_of(c["clusters"], 0.001) == 20
    assert depth_of(c["deep21"], 0.0005) == 21 and depth_of(c["deep21"], DEEP22_VOXEL) == 22
    assert len(np.unique(c["duplicates"], axis=0)) == 300 and len(c["duplicates"]) == 2100


def rep_index(pts, coords):
    """coordinates -> the smallest cloud index with exactly those coordinates (by bits)"""
    key = {}
    for i, p in enumerate(pts):
        key.setdefault(p.tobytes(), i)
    return np.array([key[np.ascontiguousarray(q).tobytes()] for q in coords], np.int64)     # KeyError: not a point of the cloud


def _positions(leaf, row):
    """ascending positions in `leaf` whose entries are `row` (greedy: the first one behind the previous)"""
    where = {}
    for pos, r in enumerate(leaf):
        where.setdefault(int(r), []).append(pos)
    out, prev = [], -1
    for r in row:
        lst = where[int(r)]
        pos = lst[np.searchsorted(lst, prev + 1)]                                            # IndexError: not ascending
        out.append(pos)
        prev = pos
    return np.array(out, np.int64)


def _matching(coarse, fine):
    """positions p with coarse[p] == fine, each position once: the k-th occurrence of a value in fine takes its k-th in coarse"""
    where, seen = {}, {}
    for pos, r in enumerate(coarse):
        where.setdefault(int(r), []).append(pos)
    out = np.empty(len(fine), np.int64)
    for i, r in enumerate(fine):
        k = seen.get(int(r), 0)
        out[i] = where[int(r)][k]
        seen[int(r)] = k + 1
    return out


# ---- packing: what np.load returns <-> what the tests see --------------------------------------------------------------
def _pack(a, rows=False):
    """float64 [m][3] on a binary grid -> (planes, g) with a == (k + g[1:4]) * g[0] bit for bit (asserted) for integers k,
    every zero of a written -0.0 if g[4].  Stored are the byte planes (so that deflate sees equal bytes next to each other)
    of k, or with rows (g[5]) of the differences of k from one row to the next, signs folded into the lowest bit."""
    a = np.ascontiguousarray(a, np.float64).reshape(-1, 3)
    step = 1.0
    while not np.array_equal(np.rint(a / step), a / step):
        step /= 2.0
        assert step > 2.0 ** -60
    k = np.rint(a / step).astype(np.int64)
    lo = k.min(0) if len(k) and not rows else np.zeros(3, np.int64)
    if rows:
        d = np.diff(k, axis=0, prepend=0)
        q = ((d << 1) ^ (d >> 63)).astype(np.uint64)
    else:
        q = (k - lo).astype(np.uint64)
    nb = max(1, (int(q.max()).bit_length() + 7) // 8) if q.size else 1
    zeros = a == 0.0
    negzero = bool(zeros.any() and np.signbit(a[zeros]).all())
    planes = np.ascontiguousarray(q.reshape(-1).view(np.uint8).reshape(-1, 8).T[:nb])
    g = np.array([step, lo[0], lo[1], lo[2], float(negzero), float(rows)])
    assert np.array_equal(_unpack(planes, g).view(np.uint64), a.view(np.uint64))
    return planes, g


def _unpack(planes, g):
    q = np.zeros((planes.shape[1], 8), np.uint8)
    q[:, :planes.shape[0]] = planes.T
    q = q.view(np.uint64).reshape(-1, 3)
    if g[5]:
        k = np.cumsum((q >> np.uint64(1)).astype(np.int64) ^ -(q & np.uint64(1)).astype(np.int64), axis=0)
    else:
        k = q.astype(np.int64)
    a = (k.astype(np.float64) + g[1:4]) * g[0]
    if g[4]:
        a[a == 0.0] = -0.0
    return a


# lattice62_negzero's arrays are stored as their difference from lattice62's of the same name, shape and type (_rebase): the
# shift by 31 and the sign of zero change neither the tree nor an order, and the reference confirms it with rows of zeros
TWIN = ("lattice62_negzero", "lattice62")


def _rebase(z, sign):
    for k in sorted(z):
        if k.startswith(TWIN[0]) and not k.endswith(("_g", "_leaf")):
            other = z.get(TWIN[1] + k[len(TWIN[0]):])
            if other is not None and other.shape == z[k].shape and other.dtype == z[k].dtype:
                z[k] = z[k] + other if sign > 0 else z[k] - other                       # wraps, so it inverts exactly
    return z


def key(name, voxel, kind):
    return "%s_v%g_%s" % (name, voxel, kind)


def compute():
    """the fixture's arrays as they are stored:
      <cloud>, <cloud>_v<voxel>_centres   with their _g: _pack() of the float64 [m][3]
      <cloud>_v<voxel>_leaf               the coarsest voxel of a cloud: the row; a finer one: for each entry its position in the
                                          next coarser voxel's row, minus its own (a finer tree only reorders inside a leaf);
                                          lattice62_negzero: the row minus lattice62's
      <cloud>_v<voxel>_d1, _d3            positions in the leaf row, differenced"""
    c = clouds()
    check_clouds(c)
    z = {"seed": np.array(SEED, np.int64)}
    probe = np.empty(8, np.int32)
    ref_lib().ro_rand_probe(SEED, 8, probe.ctypes.data)
    assert np.array_equal(probe, rand_probe())
    z["rand_probe"] = probe
    rows = {}
    for name, voxels in CASES:
        pts = c[name]
        n = len(pts)
        assert n < 32768
        z[name], z[name + "_g"] = _pack(pts)
        own = np.sort(rep_index(pts, pts))
        coarser = None
        for voxel in sorted(voxels, reverse=True):
            cen = RefOct.centres(pts, voxel)
            leaf = rep_index(pts, RefOct.random(pts, voxel, ALL, SEED))
            assert len(leaf) == n and np.array_equal(np.sort(leaf), own)                    # every point, once each
            z[key(name, voxel, "centres")], z[key(name, voxel, "centres_g")] = _pack(cen, rows=True)
            rows[(name, voxel)] = leaf
            if name == TWIN[0]:
                z[key(name, voxel, "leaf")] = (leaf - rows[(TWIN[1], voxel)]).astype(np.int16)
            elif coarser is None:
                z[key(name, voxel, "leaf")] = leaf.astype(np.int16)
            else:
                pos = _matching(coarser, leaf)
                assert np.array_equal(coarser[pos], leaf)
                z[key(name, voxel, "leaf")] = (pos - np.arange(n)).astype(np.int16)
            coarser = leaf
            for nrpts in (1, 3):
                row = rep_index(pts, RefOct.random(pts, voxel, nrpts, SEED))
                if nrpts == 1:
                    assert len(row) == len(cen)                                             # one per leaf
                pos = _positions(leaf, row)
                assert np.array_equal(leaf[pos], row)
                z[key(name, voxel, "d%d" % nrpts)] = np.diff(pos, prepend=0).astype(np.int16)
    return _rebase(z, -1)


class Fixture:
    """the fixture, unpacked: a row's coordinates are cloud(name)[row]"""

    def __init__(self, z):
        self.z = z
        self.seed = int(z["seed"])
        self.rand_probe = z["rand_probe"]
        self._leaf = {}

    def cases(self):
        return [(name, voxel) for name, voxels in CASES for voxel in voxels]

    def cloud(self, name):
        return _unpack(self.z[name], self.z[name + "_g"])

    def centres(self, name, voxel):
        return _unpack(self.z[key(name, voxel, "centres")], self.z[key(name, voxel, "centres_g")])

    def leaf(self, name, voxel):
        if name == TWIN[0]:
            return self.z[key(name, voxel, "leaf")].astype(np.int64) + self.leaf(TWIN[1], voxel)
        if (name, voxel) not in self._leaf:
            row = None
            for v in sorted(dict(CASES)[name], reverse=True):
                a = self.z[key(name, v, "leaf")].astype(np.int64)
                row = a if row is None else row[a + np.arange(len(a))]
                self._leaf[(name, v)] = row
        return self._leaf[(name, voxel)]

    def drawn(self, name, voxel, nrpts):
        pos = np.cumsum(self.z[key(name, voxel, "d%d" % nrpts)].astype(np.int64))
        return self.leaf(name, voxel)[pos]


def load(path=OUT):
    return Fixture(_rebase(dict(np.load(path)), +1))


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


if __name__ == "__main__":
    if not have_ref():
        raise SystemExit("needs the reference checkout at %s (src/slam6d/Boctree.cc)" % REF)
    z = compute()
    save(z)
    size = os.path.getsize(OUT)
    print("wrote %s (%d arrays, %d bytes)" % (OUT, len(z), size))
    for k in sorted(z, key=lambda k: -z[k].nbytes)[:12]:
        print("  %-40s %s %s" % (k, z[k].dtype, z[k].shape))
    assert size <= MAX_BYTES, size
