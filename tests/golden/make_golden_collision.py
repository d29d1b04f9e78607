"""Generator of k13_collision.npz: what collision_model's three steps (src/collision/collision_model.cc) give when their
loops run over the reference's own compiled queries (oracle/_ref/libref3dtk.so): KDtreeIndexed::fixedRangeSearch,
segmentSearch_all, segmentSearch_1NearestPoint and FindClosest.

    python tests/golden/make_golden_collision.py     (needs oracle/_ref: a build() where the reference checkout exists)

The four loops are restated here over those query methods:
  mark, cmethod 1  (handle_pointcloud CTYPE1): every index of fixedRangeSearch(transform3(T_j, m), radius^2) is marked
  mark, cmethod 2  (CTYPE2): every index of segmentSearch_all(transform3(T_j, m), transform3(T_j+1, m), radius^2)
  depth_closest    (calculate_collidingdist): a tree over the non-colliding points; per colliding point
                   (float)sqrt(Dist2(point, FindClosest(point, 1000000)))
  depth_axis       (calculate_collidingdist2): a tree over the colliding points; per frame and model point the nearest tree
                   point c1 of the segment transform3(T, (x, y, z)) .. transform3(T, (0, y, 0)), and every k of
                   fixedRangeSearch(c1, radius^2) takes "if (d2 < dist[k]) dist[k] = d2" on floats; the root at the end

  small cases: six of the k8 clouds x buckets (1, 5, 20) x both marking methods: the mask (np.packbits), num_colliding and,
           except on the clouds `seven` and `one`, both depth arrays (float32) over that mask
  large cases (trips, deep at buckets 1 and 20, table, nonfinite; the clouds of make_golden_knn_edges.py): the packed mask,
           num_colliding and the CRC-32 of the float32 depth arrays.  deep also records the axis depth over a mask of
           fifteen points in sixteen: the one case whose depth tree is itself deep
Clouds, models and trajectories are seeded and regenerated, none is stored.

Also imported by the tests, so that the fixture and the live reference are checked the same way."""
import ctypes as C
import importlib.util
import os
import sys
import zlib

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
OUT = os.path.join(_HERE, "k13_collision.npz")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


mgs = _load("make_golden_segments")
SegRef, RefTree, k8_clouds, BUCKETS, leaf_take = mgs.SegRef, mgs.RefTree, mgs.k8_clouds, mgs.BUCKETS, mgs.leaf_take

SMALL = ("uniform", "duplicates", "lattice", "clusters", "seven", "one")
NO_DEPTH = ("seven", "one")       # too few points for both a colliding and a non-colliding tree at every bucket size
METHODS = (1, 2)
MAXDIST2 = 1000000.0              # calculate_collidingdist's FindClosest


def have_ref():
    if _ROOT not in sys.path:
        sys.path.insert(0, _ROOT)
    from oracle import orc
    return orc.have_ref()


# ---- the reference library through ctypes ------------------------------------------------------------------------
class ColRef(SegRef):
    """SegRef + FindClosest (the library's batched driver over KDtreeIndexed::FindClosest), and the three queries of the
    loops taking the ADDRESS of their points (rows of contiguous arrays): half a million calls per case"""

    def __init__(self, pts, bucket):
        super().__init__(pts, bucket)
        R = self.R
        # function objects of their own (CDLL[...] makes a new one): SegRef's prototypes stay as they are
        self.c_range = R["_ZNK13KDtreeIndexed16fixedRangeSearchEPddi"]
        self.c_range.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int]
        self.c_range.restype = C.c_void_p
        self.c_segall = R["_ZNK13KDtreeIndexed17segmentSearch_allEPdS0_di"]
        self.c_segall.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int]
        self.c_segall.restype = C.c_void_p
        self.c_near = R["_ZNK13KDtreeIndexed27segmentSearch_1NearestPointEPdS0_di"]
        self.c_near.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int]
        self.c_near.restype = C.c_size_t
        self.libc = C.CDLL(None)
        self.libc.free.argtypes = [C.c_void_p]
        self.slot = (C.c_uint64 * 3)()
        self.slot_at = C.addressof(self.slot)

    def _take(self):
        """the returned std::vector<size_t> as an array; its buffer is released (operator new is malloc here)"""
        b, e = self.slot[0], self.slot[1]
        if not b:
            return np.zeros(0, np.int64)
        out = np.array((C.c_uint64 * ((e - b) // 8)).from_address(b), np.int64)
        self.libc.free(b)
        return out

    def range_at(self, p, r2):
        self.c_range(self.slot_at, self.kdi, p, r2, 0)
        return self._take()

    def segall_at(self, p, p0, r2):
        self.c_segall(self.slot_at, self.kdi, p, p0, r2, 0)
        return self._take()

    def nearest_at(self, p, p0, r2):
        r = self.c_near(self.kdi, p, p0, r2, 0)
        return -1 if r == 2 ** 64 - 1 else int(r)

    def closest(self, Q, maxd2):
        Q = np.ascontiguousarray(Q, np.float64)
        idx = np.empty(len(Q), np.int32)
        self.R.ref_kdi_find_closest(self.h, Q.ctypes.data_as(C.POINTER(C.c_double)), len(Q), float(maxd2),
                                    idx.ctypes.data_as(C.POINTER(C.c_int32)), 1)
        return idx


# ---- the loops of collision_model.cc ----------------------------------------------------------------------------------
def transform3(T, X):
    """globals.icc:1454-1463 on the rows of X, term for term"""
    with np.errstate(invalid="ignore", over="ignore"):
        x, y, z = X[:, 0], X[:, 1], X[:, 2]
        xn = (x * T[0] + y * T[4]) + z * T[8]
        yn = (x * T[1] + y * T[5]) + z * T[9]
        zn = (x * T[2] + y * T[6]) + z * T[10]
        return np.ascontiguousarray(np.stack([xn + T[12], yn + T[13], zn + T[14]], 1))


def moved(model, frames):
    """[F][P][3]: every model point under every frame"""
    return [transform3(T, model) for T in frames]


def mark(tree, n, model, frames, radius, cmethod):
    """handle_pointcloud: (mask [n] bool, num_colliding)"""
    r2 = radius * radius
    mask = np.zeros(n, bool)
    W = moved(model, frames)
    P = len(model)
    if cmethod == 1:
        for Wj in W:
            base = Wj.ctypes.data
            for m in range(P):
                mask[tree.range_at(base + 24 * m, r2)] = True
    else:
        if len(W) == 0:
            raise ValueError("the reference dereferences an empty trajectory")
        for j in range(len(W) - 1):
            a, b = W[j].ctypes.data, W[j + 1].ctypes.data
            for m in range(P):
                mask[tree.segall_at(a + 24 * m, b + 24 * m, r2)] = True
    return mask, int(mask.sum())


def _dist2(A, B):
    with np.errstate(invalid="ignore", over="ignore"):
        d = B - A
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def depth_closest(env, mask, bucket):
    """calculate_collidingdist: (dist [num_colliding] float32, n_unreached)"""
    rest, hit = np.ascontiguousarray(env[~mask]), np.ascontiguousarray(env[mask])
    c = ColRef(rest, bucket).closest(hit, MAXDIST2)
    found = c >= 0
    out = np.full(len(hit), 1000.0, np.float32)
    out[found] = np.sqrt(_dist2(hit[found], rest[c[found]])).astype(np.float32)
    return out, int((~found).sum())


def depth_axis(env, mask, model, frames, radius, bucket):
    """calculate_collidingdist2: dist [num_colliding] float32, by compact index"""
    r2 = radius * radius
    hit = np.ascontiguousarray(env[mask])
    tree = ColRef(hit, bucket)
    dist = np.full(len(hit), 1000.0, np.float32)
    axis = np.zeros_like(model)
    axis[:, 1] = model[:, 1]
    hit_at = tree.pts.ctypes.data
    for T in frames:
        P1, P2 = transform3(T, model), transform3(T, axis)
        a, b = P1.ctypes.data, P2.ctypes.data
        for m in range(len(model)):
            c1 = tree.nearest_at(a + 24 * m, b + 24 * m, r2)
            if c1 < 0:
                continue
            d2 = np.float64(_dist2(P1[m], tree.pts[c1]))
            idx = tree.range_at(hit_at + 24 * c1, r2)
            sel = d2 < dist[idx].astype(np.float64)
            dist[idx[sel]] = np.float32(d2)
    return np.sqrt(dist)


# ---- models and trajectories -------------------------------------------------------------------------------------------
def frame(axis, angle, t):
    """a rigid motion as the 16 doubles of a column-major 4x4 matrix (Rodrigues' formula)"""
    u = np.asarray(axis, np.float64)
    u = u / np.linalg.norm(u)
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    T = np.zeros(16)
    for col in range(3):
        T[4 * col:4 * col + 3] = R[:, col]
    T[12:15] = t
    T[15] = 1.0
    return T


def small_model(radius, seed):
    """40 points within 1.5 radii of the origin: the origin itself, five with y = 0, three on the y axis (their axis
    segment of the depth has length zero)"""
    rng = np.random.default_rng(seed)
    m = rng.uniform(-1.5, 1.5, (40, 3)) * radius
    m[0] = 0.0
    m[1:6, 1] = 0.0
    m[6:9, 0] = 0.0
    m[6:9, 2] = 0.0
    return m


def small_trajectory(pts, far=500.0):
    """12 frames: ten from the cloud's first point to its middle one, turning on the way, the fifth given twice (a segment
    of length zero), and one far outside the cloud"""
    A, B = pts[0], pts[len(pts) // 2]
    fr = [frame((1.0, 2.0, 3.0), 0.3 * j, A + (B - A) * (j / 9.0)) for j in range(10)]
    fr.insert(5, fr[4].copy())
    fr.append(frame((0.0, 0.0, 1.0), 0.5, pts.max(0) + far))
    return np.array(fr)


def small_case(name):
    """(points, model, frames, radius) of a small case"""
    pts, _, _, r2 = k8_clouds()[name]
    radius = float(np.sqrt(r2))
    model, frames = small_model(radius, 1300 + SMALL.index(name)), small_trajectory(pts)
    if len(pts) < 10:
        # a handful of points within a radius or two of each other: a tight model that stays near the first point, so that
        # some of them are left alone
        model *= 0.2
        frames[:11, 12:15] = pts[0] + 0.1 * (frames[:11, 12:15] - pts[0])
    return pts, model, frames, radius


def curve(n, lo, hi, amp, turns=2.0):
    """n frames along a line from lo to hi with a sine across it, turning about a fixed axis"""
    s = np.linspace(0.0, 1.0, n)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    pos = lo + (hi - lo) * s[:, None] + amp * np.sin(2 * np.pi * turns * s)[:, None] * np.array([0.3, -0.5, 0.8])
    return np.array([frame((2.0, -1.0, 0.5), 1.5 * si, p) for si, p in zip(s, pos)])


LARGE = (("trips", 20), ("deep", 1), ("deep", 20), ("table", 20), ("nonfinite", 20))
NONFINITE_FRAMES = (3, 11)
NONFINITE_POINTS = (2, 17, 30)


def large_case(name):
    """(points, model, frames, radius) of a large case"""
    me = _load("make_golden_knn_edges")
    rng = np.random.default_rng(1390)
    if name == "trips":
        # 700 model points x 800 frames = 560,000 queries: more than twice the lanes of the capped grid
        pts, _ = me.trips_cloud()
        model = rng.uniform(-2.0, 2.0, (700, 3))
        model[:20, 1] = 0.0
        return pts, model, curve(800, (-45, -40, -42), (44, 41, 40), 6.0), 1.0
    if name == "deep":
        # through the geometric core at the origin, where the tree is about 80 levels deep
        pts, _ = me.deep_cloud()
        model = rng.uniform(-1.5, 1.5, (50, 3))
        model[0] = 0.0
        return pts, model, curve(60, (-12, -9, -10), (12, 9, 10), 0.0), 3.0
    if name == "table":
        # through the 40,000 copies of one point and the blob beside them (leaf table mode)
        pts, _, _ = me.table_cloud()
        model = rng.uniform(-0.008, 0.008, (60, 3))
        model[0] = 0.0
        d = np.array([0.06, 0.03, 0.0])
        return pts, model, curve(50, me.TABLE_COPY - d, me.TABLE_COPY + d, 0.0), float(np.sqrt(me.TABLE_R2[0]))
    if name == "nonfinite":
        pts = me.nonfinite_cloud()[0]
        model = rng.uniform(-2.0, 2.0, (40, 3))
        model[0] = 0.0
        model[NONFINITE_POINTS[0], 0] = np.nan
        model[NONFINITE_POINTS[1], 1] = np.inf
        model[NONFINITE_POINTS[2], 2] = -np.inf
        fr = curve(20, (-25, -20, -22), (24, 21, 20), 3.0)
        fr[NONFINITE_FRAMES[0], 13] = np.nan
        fr[NONFINITE_FRAMES[1], 5] = np.inf
        return pts, model, fr, float(np.sqrt(me.NONFINITE_R2))
    raise KeyError(name)


def wide_mask(n):
    """fifteen points in sixteen: a depth tree about as deep as the cloud's own"""
    return (np.arange(n) % 16) != 0


# ---- the fixture --------------------------------------------------------------------------------------------------
def crc(a):
    return np.array([zlib.crc32(np.ascontiguousarray(a, "<f4").tobytes())], np.uint32)


def reference_case(pts, model, frames, radius, bucket, cmethod, depths=True, tree=None):
    """{mask, num, d1, unreached, d2} of one case from the live reference (d1, d2 only with depths)"""
    tree = tree or ColRef(pts, bucket)
    mask, num = mark(tree, len(pts), model, frames, radius, cmethod)
    out = {"mask": mask, "num": num}
    if depths:
        out["d1"], out["unreached"] = depth_closest(pts, mask, bucket)
        out["d2"] = depth_axis(pts, mask, model, frames, radius, bucket)
    return out


def compute():
    z, stats = {}, []
    for name in SMALL:
        pts, model, frames, radius = small_case(name)
        for b in BUCKETS:
            tree = ColRef(pts, b)
            for cm in METHODS:
                r = reference_case(pts, model, frames, radius, b, cm, name not in NO_DEPTH, tree)
                key = "%s_b%d_m%d" % (name, b, cm)
                z[key + "_mask"] = np.packbits(r["mask"])
                z[key + "_num"] = np.array([r["num"]], np.uint64)
                if name not in NO_DEPTH:
                    z[key + "_d1"] = r["d1"]
                    z[key + "_d2"] = r["d2"]
                stats.append((key, len(pts), r["num"], r.get("unreached", 0)))
    for name, b in LARGE:
        pts, model, frames, radius = large_case(name)
        tree = ColRef(pts, b)
        for cm in METHODS:
            r = reference_case(pts, model, frames, radius, b, cm, True, tree)
            key = "%s_b%d_m%d" % (name, b, cm)
            z[key + "_mask"] = np.packbits(r["mask"])
            z[key + "_num"] = np.array([r["num"]], np.uint64)
            z[key + "_d1crc"] = crc(r["d1"])
            z[key + "_d2crc"] = crc(r["d2"])
            stats.append((key, len(pts), r["num"], r["unreached"]))
        if name == "deep":
            z["deep_b%d_wide_d2crc" % b] = crc(depth_axis(pts, wide_mask(len(pts)), model, frames, radius, b))
    return z, stats


def check_not_vacuous(stats):
    """every case marks something and, where the cloud has more than one point, not everything; FindClosest reached all"""
    for key, n, num, unreached in stats:
        assert num >= 1 and (num < n or n == 1) and unreached == 0, (key, n, num, unreached)


class Fixture:
    def __init__(self, z):
        self.z = z

    def mask(self, key, n):
        return np.unpackbits(self.z[key + "_mask"])[:n].astype(bool)

    def num(self, key):
        return int(self.z[key + "_num"][0])


def load(path=OUT):
    return Fixture(np.load(path))


if __name__ == "__main__":
    sys.path.insert(0, _ROOT)
    if not have_ref():
        raise SystemExit("needs oracle/_ref/libref3dtk.so (build() where the reference checkout exists)")
    import time
    t0 = time.time()
    z, stats = compute()
    for s in stats:
        print(s)
    check_not_vacuous(stats)
    np.savez_compressed(OUT, **z)
    print("wrote %s (%d arrays, %d bytes, %.1f s)" % (OUT, len(z), os.path.getsize(OUT), time.time() - t0))
