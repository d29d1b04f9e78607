"""Generator of k12_knn_range.npz: KDtree::kNearestRangeSearch (kd.cc:137-171, _KNNRangeSearch kdTreeImpl.h:684-745) from the
reference's own compiled kd.cc, on the clouds of k8_kdtree_queries.npz, and the normals the oracle's PCA gives on those lists.

    python tests/golden/make_golden_knn_range.py        (needs the reference checkout: $TDTK_REF, default /root/reference)

kd.cc is compiled as it is, with the flags of oracle/build_ref.sh, next to a driver of our own (oracle/ref_kd_driver.cc) and
loaded through ctypes: oracle/_ref/libref_kd.so where build_ref.sh made it, else a build into a temporary directory; nothing
of it reaches the repository.

The reference returns coordinates (std::vector<Point>), not indices.  Every returned point is bit-equal to a point of the
cloud (asserted), so a row is stored losslessly as the smallest cloud index with those coordinates: coords = pts[rep].  To
keep the file small the rows of all k lie side by side ([Q][sum KS]) and are stored as their difference from the k = 64 row
of bucket 1 ("base"; a shorter row is nearly always its prefix), and the normals as the XOR of their bits with bucket 1's.
The tests read the fixture through load(), which undoes both.

Also imported by the tests (KS, radii, load, RefKD ...), so that the fixture and the live reference are checked the same way."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
sys.path.insert(0, _HERE)
import make_golden_knn as G8  # noqa: E402

OUT = os.path.join(_HERE, "k12_knn_range.npz")
K8 = os.path.join(_HERE, "k8_kdtree_queries.npz")
REF = os.environ.get("TDTK_REF", "/root/reference")

KS = (1, 4, 10, 20, 32, 33, 64)       # the list-capacity edges 10 / 20 / 32 / 33 included
BUCKETS = (1, 5, 20)
NORMAL_KS = (4, 10, 20, 33)
HUGE = 1e30
LARGE = ("uniform", "duplicates", "lattice", "plane", "clusters")
RPOS = G8.RPOS
KOFF = np.concatenate([[0], np.cumsum(KS)])     # row of KS[j]: columns KOFF[j] .. KOFF[j + 1]

# the flags of oracle/build_ref.sh
FLAGS = "-std=c++17 -O3 -fPIC -fopenmp -DOPENMP -DOPENMP_NUM_THREADS=8 -DMAX_OPENMP_NUM_THREADS=512 -w".split()

DRIVER = os.path.join(_ROOT, "oracle", "ref_kd_driver.cc")     # the handle around KDtree and the loop over kNearestRangeSearch
PREBUILT = os.path.join(_ROOT, "oracle", "_ref", "libref_kd.so")   # oracle/build_ref.sh's build of the same two files


def have_ref():
    return os.path.isfile(os.path.join(REF, "src", "slam6d", "kd.cc"))


def have_lib():
    """the prebuilt library is there: what a GPU test asks, which never touches the checkout"""
    return os.path.isfile(PREBUILT)


_lib = None
_tmp = None


def ref_lib():
    """kd.cc + DRIVER: oracle/_ref/libref_kd.so where it was built, else built into a temporary directory (removed at exit)"""
    global _lib, _tmp
    if _lib is None:
        so = PREBUILT
        if not have_lib():
            _tmp = tempfile.TemporaryDirectory(prefix="k12_ref_")
            d = _tmp.name
            inc = ["-I" + os.path.join(REF, "include"), "-I" + os.path.join(REF, "3rdparty", "newmat", "newmat-10")]
            subprocess.check_call(["g++"] + FLAGS + inc + ["-c", os.path.join(REF, "src", "slam6d", "kd.cc"), "-o", os.path.join(d, "kd.o")])
            subprocess.check_call(["g++"] + FLAGS + inc + ["-c", DRIVER, "-o", os.path.join(d, "driver.o")])
            so = os.path.join(d, "libkr.so")
            subprocess.check_call(["g++", "-shared", "-fopenmp", "-Wl,--no-undefined", "-o", so, os.path.join(d, "kd.o"), os.path.join(d, "driver.o")])
        _lib = C.CDLL(so)
        _lib.kr_create.restype = C.c_void_p
        _lib.kr_create.argtypes = [C.c_void_p, C.c_int, C.c_int]
        _lib.kr_destroy.argtypes = [C.c_void_p]
        _lib.kr_search.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
    return _lib


class RefKD:
    """the reference's KDtree (pointer flavour) over pts"""

    def __init__(self, pts, bucket):
        self.L = ref_lib()
        pts = np.ascontiguousarray(pts, np.float64)
        self.h = self.L.kr_create(pts.ctypes.data, len(pts), int(bucket))

    def __del__(self):
        if getattr(self, "h", None):
            self.L.kr_destroy(self.h)

    def search(self, Q, k, r2):
        """(coordinates [Q][k][3], NaN behind a row's entries; counts [Q] int32)"""
        Q = np.ascontiguousarray(Q, np.float64)
        out = np.full((len(Q), k, 3), np.nan)
        cnt = np.zeros(len(Q), np.int32)
        self.L.kr_search(self.h, Q.ctypes.data, len(Q), int(k), float(r2), out.ctypes.data, cnt.ctypes.data)
        return out, cnt


def radii(z8, name, pts, Q, r2):
    """the three radii of a cloud: its k8 r2, the median 10th-neighbour d2 of its queries (k8's rows; the largest d2 + 1 for a
    cloud of fewer than 10 points), 1e30"""
    knn = z8["%s_b1_knn10" % name]
    d2 = G8.dist2(pts, Q[:, None, :], knn)
    mid = float(np.median(d2[:, 9])) if len(pts) >= 10 else float(d2.max() + 1.0)
    return (float(r2), mid, HUGE)


def rep_index(pts, coords, cnt):
    """coordinates -> the smallest cloud index with exactly those coordinates (-1 behind a row's entries)"""
    key = {}
    for i, p in enumerate(pts):
        key.setdefault(p.tobytes(), i)
    rep = -np.ones(coords.shape[:2], np.int16)
    for i in range(coords.shape[0]):
        for j in range(cnt[i]):
            rep[i, j] = key[np.ascontiguousarray(coords[i, j]).tobytes()]     # KeyError: not a point of the cloud
    return rep


def _tile(base):
    """the k = 64 row's prefixes side by side, as the rows of all KS lie"""
    return np.concatenate([base[:, :k] for k in KS], axis=1)[None]


def compute(orc):
    z8 = np.load(K8)
    z = {}
    stats = {"full": 0, "short": 0, "rows": 0, "empty_small": 0}
    for name, (pts, Q, no, r2) in G8.k8_clouds().items():
        rr = radii(z8, name, pts, Q, r2)
        z[name + "_radii"] = np.array(rr)
        trees = [RefKD(pts, b) for b in BUCKETS]
        for ri, r in enumerate(rr):
            rows = np.empty((len(BUCKETS), len(Q), KOFF[-1]), np.int16)
            cnts = np.empty((len(BUCKETS), len(Q), len(KS)), np.int8)
            for bi, t in enumerate(trees):
                for kj, k in enumerate(KS):
                    coords, cnt = t.search(Q, k, r)
                    rep = rep_index(pts, coords, cnt)
                    rows[bi, :, KOFF[kj]:KOFF[kj + 1]] = rep
                    cnts[bi, :, kj] = cnt
                    if k in NORMAL_KS:
                        nrm = np.empty((no, 3))
                        for i in range(no):
                            nrm[i] = G8._pca(orc, Q[i], coords[i, :cnt[i]], RPOS)
                        z.setdefault("%s_r%d_n%d" % (name, ri, k), []).append(nrm.view(np.uint64))
                    if k == 10 and name in LARGE:
                        inball = (G8.dist2(pts, Q[:, None, :], np.arange(len(pts))[None, :]) < r).sum(1)
                        if ri == 1:
                            stats["rows"] += len(Q)
                            stats["full"] += int(((cnt == k) & (inball > k)).sum())
                            stats["short"] += int(((cnt > 0) & (cnt < k)).sum())
                        if ri == 0:
                            stats["empty_small"] += int((cnt == 0).sum())
            base = rows[0][:, KOFF[-2]:].copy()
            z["%s_r%d_base" % (name, ri)] = base
            z["%s_r%d_rows" % (name, ri)] = (rows - _tile(base)).astype(np.int16)
            z["%s_r%d_counts" % (name, ri)] = cnts
        for k in NORMAL_KS:
            for ri in range(3):
                key = "%s_r%d_n%d" % (name, ri, k)
                n = np.stack(z[key])
                n[1:] ^= n[0]
                z[key] = n
    return z, stats


def check_not_vacuous(stats):
    assert 4 * stats["full"] >= stats["rows"], stats
    assert 4 * stats["short"] >= stats["rows"], stats
    assert stats["empty_small"] >= 1, stats


class Fixture:
    """the fixture, unpacked: rows(name, ri, bucket, k) -> rep [Q][k] int16, counts(...) -> [Q], coords = pts[rep]"""

    def __init__(self, z):
        self.z = z

    def radii(self, name):
        return [float(r) for r in self.z[name + "_radii"]]

    def rows(self, name, ri, bucket, k):
        bi, kj = BUCKETS.index(bucket), KS.index(k)
        all_rows = self.z["%s_r%d_rows" % (name, ri)][bi] + _tile(self.z["%s_r%d_base" % (name, ri)])[0]
        return all_rows[:, KOFF[kj]:KOFF[kj + 1]].astype(np.int16)

    def counts(self, name, ri, bucket, k):
        return self.z["%s_r%d_counts" % (name, ri)][BUCKETS.index(bucket), :, KS.index(k)].astype(np.int32)

    def normals(self, name, ri, bucket, k):
        n = self.z["%s_r%d_n%d" % (name, ri, k)]
        bi = BUCKETS.index(bucket)
        return (n[bi] ^ n[0] if bi else n[0]).view(np.float64)


def load(path=OUT):
    return Fixture(np.load(path))


if __name__ == "__main__":
    sys.path.insert(0, _ROOT)
    if not have_ref():
        raise SystemExit("needs the reference checkout at %s (src/slam6d/kd.cc)" % REF)
    from oracle import orc
    z, stats = compute(orc)
    print("non-vacuity at k = 10, middle radius, the five large clouds:", stats)
    check_not_vacuous(stats)
    np.savez_compressed(OUT, **z)
    print("wrote %s (%d arrays, %d bytes; k8: %d bytes)" % (OUT, len(z), os.path.getsize(OUT), os.path.getsize(K8)))
    assert os.path.getsize(OUT) <= os.path.getsize(K8)
