"""Generator of k13_knn_range_edges.npz: KDtree::kNearestRangeSearch (kd.cc:137-171) of the reference's own compiled kd.cc on
the clouds of make_golden_knn_edges.py -- the branches of k_knnr_reg / k_knnr_lds that the k12 cases never execute: second
grid-stride trips, the stack's overflow on a tree 80 levels deep, leaf table mode, lists shorter than k in every band,
queries on split planes and points at d2 == r2, far and non-finite queries, radii at the ends of the finite range.

    python tests/golden/make_golden_knn_range_edges.py      (needs oracle/_ref/libref_kd.so or the reference checkout)

Every cloud is seeded and regenerated (make_golden_knn_edges.py), none is stored.  The reference returns coordinates; a row
is stored as in k12, as the smallest cloud index with those coordinates (coords = pts[rep]).  Per case (a cloud, a bucket
size, its queries, its radii, its k):
  counts   [radii][k][Q]
  rows     [radii][Q][sum of the k], the rows of all k side by side -- for the cases whose rows are small (STORE_ROWS)
  crc      [radii][k]: CRC-32 of the rows' coordinates (0.0 behind a row's entries) and counts (crc_rows) -- for the others
and, from the device walk compiled for the host (tests/host_lane.py: knn_range_walk of query_lane.h with the LDS list and
a counting stack on kd_build.cpp's tree), per (radius, k, query):
  maxsp    the largest stack height the walk reached
  filled   the list was full at the end
  big      the walk offered the list a point of the tree's largest leaf (Dist2 < r2 there: the table cloud's leaf of copies)
These records are what the tests' preconditions are asserted against; the CPU tier checks that the host walk reproduces
them along with every row and count.

Also imported by the tests (cases(), EDGE_KS, HostWalk, crc_rows ...), so that fixture, live reference and device are
checked the same way."""
import ctypes as C
import importlib.util
import os
import sys
import zlib

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
OUT = os.path.join(_HERE, "k13_knn_range_edges.npz")
K9 = os.path.join(_HERE, "k9_kdtree_query_edges.npz")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


ME = _load("make_golden_knn_edges")
MR = _load("make_golden_knn_range")

# the first and the last k inside every band (ListReg<4|10|20|32>: 2..4, 5..10, 11..20, 21..32; k = 1 is k12's), both ends
# of the LDS list
EDGE_KS = (2, 3, 5, 9, 11, 19, 21, 31, 32, 33, 34, 63, 64)
BAND_KS = (3, 9, 19, 31, 33, 64)          # one k per band, for the cases that are expensive for the reference
TRIPS_KS = (3, 31, 33, 64)
HUGE = 1e30
DBL_MAX = float(np.finfo(np.float64).max)
Q_SD = 16                                 # LaneStackQ's LDS levels (query.hip)

TRIPS_Q = 300_000                         # more than 2048 x 128 lanes, more than twice 2048 x 64
TRIPS_SAMPLE = 2_000                      # the rows the fixture pins (the GPU test: 20,000 live)
# Every squared distance of the deep cloud is below (2 * 1.2e85)^2 = 6e170: with this radius every plane test passes, every
# far child is pushed and the walk is pruned by the box test alone -- with r2 instead of the k-th distance until the list
# fills.  DEEP_R2's 9 and 400 push next to nothing above the core (a level's split value is the centroid of what is left,
# 1e-5 of the radius peeled there): max_sp passes Q_SD for no query at bucket 20 and for 61 of 300 at bucket 1 and r2 = 400
# (test_knn_range_edges_host.py has the figures of every radius tried).
DEEP_FINITE_R2 = 1e200
NONFINITE_R2 = (ME.NONFINITE_R2, 5e-324, 1e-300, DBL_MAX, HUGE)
SHORT_ALL_R2 = 100.0                      # points in [-1, 1]^3, queries in [-2, 2]^3: every d2 <= 27
STORE_ROWS = ("table", "short", "lattice", "nonfinite")


class Case:
    def __init__(self, name, kind, pts, Q, bucket, r2s, ks, **extra):
        self.name, self.kind, self.bucket, self.r2s, self.ks = name, kind, int(bucket), tuple(float(r) for r in r2s), tuple(ks)
        self.pts, self.Q = np.ascontiguousarray(pts, np.float64), np.ascontiguousarray(Q, np.float64)
        self.koff = np.concatenate([[0], np.cumsum(self.ks)])
        self.__dict__.update(extra)

    @property
    def store_rows(self):
        return self.kind in STORE_ROWS


_clouds = {}


def cloud(kind):
    """the clouds of make_golden_knn_edges.py, made once per process"""
    if kind not in _clouds:
        _clouds[kind] = {"trips": ME.trips_cloud, "deep": ME.deep_cloud, "table": ME.table_cloud, "lattice": ME.lattice_cloud,
                         "nonfinite": ME.nonfinite_cloud}[kind]()
    return _clouds[kind]


def trips_queries():
    """(the 300,000 queries, the sorted positions of the sample the fixture pins)"""
    _, Q = cloud("trips")
    return Q[:TRIPS_Q], np.sort(np.random.default_rng(1301).choice(TRIPS_Q, TRIPS_SAMPLE, replace=False))


def trips_radii():
    """k12's middle radius on this cloud -- the median 10th-neighbour d2, here over the first 200 sampled queries by brute
    force -- and 1e30"""
    if "trips_radii" not in _clouds:
        pts, _ = cloud("trips")
        Q, sample = trips_queries()
        q = Q[sample[:200]]
        d = all_d2(pts, q)
        _clouds["trips_radii"] = (float(np.median(np.partition(d, 9, axis=1)[:, 9])), HUGE)
    return _clouds["trips_radii"]


def all_d2(pts, Q):
    """[Q][M] Dist2 (globals.icc:238), exact"""
    dx = pts[None, :, 0] - Q[:, None, 0]; dy = pts[None, :, 1] - Q[:, None, 1]; dz = pts[None, :, 2] - Q[:, None, 2]
    return (dx * dx + dy * dy) + dz * dz


def short_half_r2(pts, Q):
    """a radius that holds about half of a short cloud: the median of all (query, point) d2"""
    return float(np.median(all_d2(pts, Q)))


def table_mixed_queries(pts):
    """16 queries on the way from the copied point to the blob at which 1 .. 60 points lie nearer than the 40,000 copies:
    table_queries() has none, its lists hold copies alone or none.  Such a list takes that many blob points, then copies (for
    k above that number), and blob points alone below it; with a radius between the two distances the copies stay out"""
    rng = np.random.default_rng(9303)
    t = rng.uniform(0.385, 0.46, (600, 1))     # (the ball through the copies reaches the blob's near edge at t = 0.384)
    q = ME.TABLE_COPY + t * (ME.TABLE_BLOB - ME.TABLE_COPY) + rng.uniform(-0.0003, 0.0003, (600, 3))
    d = all_d2(pts, q)
    dc = all_d2(ME.TABLE_COPY[None, :], q)[:, 0]
    nearer = (d < dc[:, None]).sum(1)
    pick = np.nonzero((nearer >= 1) & (nearer <= 60))[0][:16]
    assert len(pick) == 16
    return q[pick]


def cases(kinds=("trips", "deep", "table", "short", "lattice", "nonfinite")):
    """the stored cases, in the fixture's order"""
    out = []
    if "trips" in kinds:
        pts, _ = cloud("trips")
        Q, sample = trips_queries()
        out.append(Case("trips_b20", "trips", pts, Q[sample], 20, trips_radii(), TRIPS_KS))
    if "deep" in kinds:
        pts, geo = cloud("deep")
        for b in ME.DEEP_BUCKETS:
            Q = ME.deep_queries(pts, geo, ME.DEEP_FALLBACK_Q, 22 + b)
            out.append(Case("deep_b%d" % b, "deep", pts, Q, b, (DEEP_FINITE_R2, HUGE), BAND_KS, ngeo=len(Q) // 3))
    if "table" in kinds:
        pts, copies, blob = cloud("table")
        qk, _ = ME.table_queries(pts, blob)
        qk = np.vstack([qk, table_mixed_queries(pts)])
        out.append(Case("table_b20", "table", pts, qk, 20, ME.TABLE_R2 + (HUGE,), BAND_KS, copies=copies, blob=blob))
    if "short" in kinds:
        for M in ME.SHORT_MS:
            pts, Q = ME.short_cloud(M)
            for b in ME.SHORT_BUCKETS:
                out.append(Case("short_m%d_b%d" % (M, b), "short", pts, Q, b, (SHORT_ALL_R2, short_half_r2(pts, Q)), ME.SHORT_KS, M=M))
    if "lattice" in kinds:
        pts, Q = cloud("lattice")
        for b in ME.LATTICE_BUCKETS:
            out.append(Case("lattice_b%d" % b, "lattice", pts, Q[:ME.LATTICE_STORED], b, ME.LATTICE_R2, BAND_KS))
    if "nonfinite" in kinds:
        pts, Q, i_ord, i_nan, i_far = cloud("nonfinite")
        out.append(Case("nonfinite_b20", "nonfinite", pts, Q, 20, NONFINITE_R2, BAND_KS, i_ord=i_ord, i_nan=i_nan, i_far=i_far))
    return out


# ---- rows as coordinates ------------------------------------------------------------------------------------------------
def coords_of(pts, idx):
    """[Q][k][3]: the points of the rows, 0.0 behind a row's entries"""
    return np.where((idx >= 0)[..., None], pts[np.maximum(idx, 0)], 0.0)


def crc_rows(coords, cnt):
    """CRC-32 over the rows' coordinates (anything behind a row's cnt entries counts as 0.0) and their lengths"""
    k = coords.shape[1]
    c = np.where((np.arange(k)[None, :] < cnt[:, None])[..., None], coords, 0.0)
    return zlib.crc32(np.ascontiguousarray(cnt, np.int32).tobytes(), zlib.crc32(np.ascontiguousarray(c, np.float64).tobytes()))


def rep_index(pts, coords, cnt):
    """coordinates -> the smallest cloud index with exactly those coordinates (-1 behind a row's entries)"""
    key = {}
    for i in range(len(pts) - 1, -1, -1):
        key[pts[i].tobytes()] = i
    rep = -np.ones(coords.shape[:2], np.int32)
    for i in range(coords.shape[0]):
        for j in range(cnt[i]):
            rep[i, j] = key[np.ascontiguousarray(coords[i, j]).tobytes()]     # KeyError: not a point of the cloud
    return rep


# ---- the device walk on the host ------------------------------------------------------------------------------------------
HOST_WALK = r"""
struct CountStack : HostStack {
  int max_sp = 0;
  void push(uint32_t r, double m) { HostStack::push(r, m); if (sp > max_sp) max_sp = sp; }
};
// the LDS list, and whether it was offered a slot of [lo, hi)
struct WatchList : ListLds<1> {
  uint32_t lo = 0, hi = 0; int offered = 0;
  void insert(const double md, const uint32_t slot) { if (slot >= lo && slot < hi) ++offered; ListLds<1>::insert(md, slot); }
};
extern "C" void hw_info(void* p, uint32_t* out) {
  HostTree& T = *(HostTree*)p;
  uint32_t best = 0;
  for (uint32_t i = 0; i < T.leaf_tab.size(); i++) if (T.leaf_tab[i].count > T.leaf_tab[best].count) best = i;
  out[0] = T.table_mode ? 1u : 0u; out[1] = T.max_depth; out[2] = T.max_leaf_points;
  out[3] = (uint32_t)T.leaf_tab[best].start; out[4] = (uint32_t)T.leaf_tab[best].count; out[5] = (uint32_t)T.n_internal;
}
// the split values of the internal nodes, with their axes
extern "C" void hw_splits(void* p, double* val, int* axis) {
  HostTree& T = *(HostTree*)p;
  for (size_t i = 0; i < T.n_internal; i++) {
    const KdNode& nd = T.nodes[i];
    val[i] = nd.splitval; axis[i] = (int)(((nd.c1 >> 30) & 1u) | (((nd.c2 >> 30) & 1u) << 1));
  }
}
extern "C" void hw_search(void* p, const double* q, int nq, int k, double r2, int* idx, double* d2, int* cnt, int* maxsp,
                          unsigned char* filled, unsigned char* big) {
  HostTree& T = *(HostTree*)p;
  QueryArgs a = host_args(T);
  uint32_t info[6]; hw_info(p, info);
  std::vector<double> ld(64); std::vector<uint32_t> ls(64);
  for (int i = 0; i < nq; i++) {
    WatchList L; L.ld = ld.data(); L.ls = ls.data(); L.init(k); L.lo = info[3]; L.hi = info[3] + info[4];
    CountStack st;
    knn_range_walk(a, q[3 * i], q[3 * i + 1], q[3 * i + 2], r2, L, st);
    int nr = 0;
    for (int j = 0; j < k; j++) nr += (L.dist(j) >= 0.0) ? 1 : 0;
    cnt[i] = nr; maxsp[i] = st.max_sp; filled[i] = L.full() ? 1 : 0; big[i] = L.offered > 0 ? 1 : 0;
    for (int j = 0; j < k; j++) { const bool v = j < nr; idx[i * k + j] = v ? a.pts[L.slot(j)].orig : -1; d2[i * k + j] = v ? L.dist(j) : -1.0; }
  }
}
"""


class HostWalk:
    """knn_range_walk compiled for the host (tests/host_lane.py), over kd_build.cpp's tree of one cloud"""

    def __init__(self, L, pts, bucket):
        self.L = L
        self.pts = np.ascontiguousarray(pts, np.float64)
        self.h = L.host_tree_create(self.pts.ctypes.data, len(self.pts), int(bucket))
        assert self.h
        info = np.zeros(6, np.uint32)
        L.hw_info(self.h, info.ctypes.data)
        self.table_mode, self.max_depth, self.max_leaf, self.big_start, self.big_count, self.n_internal = [int(v) for v in info]

    def __del__(self):
        if getattr(self, "h", None):
            self.L.host_tree_destroy(self.h)

    def splits(self):
        val = np.empty(self.n_internal); axis = np.empty(self.n_internal, np.int32)
        if self.n_internal:
            self.L.hw_splits(self.h, val.ctypes.data, axis.ctypes.data)
        return val, axis

    def search(self, Q, k, r2, L=None):
        """(idx [Q][k], d2 [Q][k], cnt [Q], max_sp [Q], filled [Q], big [Q]); L: another build of HOST_WALK to walk this tree"""
        Q = np.ascontiguousarray(Q, np.float64)
        n = len(Q)
        idx = np.empty((n, k), np.int32); d2 = np.empty((n, k)); cnt = np.empty(n, np.int32); sp = np.empty(n, np.int32)
        fl = np.empty(n, np.uint8); big = np.empty(n, np.uint8)
        (L or self.L).hw_search(self.h, Q.ctypes.data, n, int(k), float(r2), idx.ctypes.data, d2.ctypes.data, cnt.ctypes.data,
                         sp.ctypes.data, fl.ctypes.data, big.ctypes.data)
        return idx, d2, cnt, sp, fl.astype(bool), big.astype(bool)


def host_lib(tmp_path, name="hwe"):
    """HOST_WALK built through tests/host_lane.py (tmp_path: a pathlib.Path)"""
    sys.path.insert(0, os.path.join(_ROOT, "tests"))
    import host_lane
    L = host_lane.build(HOST_WALK, tmp_path, name)
    L.hw_info.argtypes = [C.c_void_p, C.c_void_p]
    L.hw_splits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.hw_search.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double] + [C.c_void_p] * 6
    return L


# ---- the fixture ----------------------------------------------------------------------------------------------------------
def _small(a, lo, hi):
    for t in (np.int8, np.int16, np.int32):
        if np.iinfo(t).min <= lo and hi <= np.iinfo(t).max:
            return a.astype(t)
    raise ValueError


def compute_case(case, L):
    """what the fixture holds of one case: the reference's rows / counts / CRCs and the host walk's records"""
    z = {}
    t = MR.RefKD(case.pts, case.bucket)
    hw = HostWalk(L, case.pts, case.bucket)
    nr, nk, nq = len(case.r2s), len(case.ks), len(case.Q)
    cnts = np.zeros((nr, nk, nq), np.int32)
    rows = -np.ones((nr, nq, case.koff[-1]), np.int32)
    crcs = np.zeros((nr, nk), np.uint32)
    maxsp = np.zeros((nr, nk, nq), np.int32)
    filled = np.zeros((nr, nk, nq), bool)
    big = np.zeros((nr, nk, nq), bool)
    for ri, r2 in enumerate(case.r2s):
        for kj, k in enumerate(case.ks):
            coords, cnt = t.search(case.Q, k, r2)
            cnts[ri, kj] = cnt
            crcs[ri, kj] = crc_rows(coords, cnt)
            if case.store_rows:
                rows[ri, :, case.koff[kj]:case.koff[kj + 1]] = rep_index(case.pts, coords, cnt)
            _, _, _, sp, fl, bg = hw.search(case.Q, k, r2)
            maxsp[ri, kj], filled[ri, kj], big[ri, kj] = sp, fl, bg
    z[case.name + "_cnt"] = _small(cnts, 0, 64)
    if case.store_rows:
        z[case.name + "_rows"] = _small(rows, -1, len(case.pts))
    else:
        z[case.name + "_crc"] = crcs
    z[case.name + "_maxsp"] = maxsp.astype(np.uint8)
    z[case.name + "_filled"] = np.packbits(filled, axis=-1)
    z[case.name + "_big"] = np.packbits(big, axis=-1)
    return z


def compute(L, kinds=None):
    z = {}
    for case in (cases(kinds) if kinds else cases()):
        z.update(compute_case(case, L))
    return z


class Fixture:
    def __init__(self, z):
        self.z = z

    def counts(self, case, ri, k):
        return self.z[case.name + "_cnt"][ri, case.ks.index(k)].astype(np.int32)

    def rows(self, case, ri, k):
        kj = case.ks.index(k)
        return self.z[case.name + "_rows"][ri][:, case.koff[kj]:case.koff[kj + 1]].astype(np.int32)

    def crc(self, case, ri, k):
        return int(self.z[case.name + "_crc"][ri, case.ks.index(k)])

    def maxsp(self, case, ri, k):
        return self.z[case.name + "_maxsp"][ri, case.ks.index(k)].astype(np.int32)

    def filled(self, case, ri, k):
        return np.unpackbits(self.z[case.name + "_filled"][ri, case.ks.index(k)])[:len(case.Q)].astype(bool)

    def big(self, case, ri, k):
        return np.unpackbits(self.z[case.name + "_big"][ri, case.ks.index(k)])[:len(case.Q)].astype(bool)


def load(path=OUT):
    return Fixture(np.load(path))


if __name__ == "__main__":
    import pathlib
    import tempfile
    if not (MR.have_lib() or MR.have_ref()):
        raise SystemExit("needs oracle/_ref/libref_kd.so or the reference checkout at %s" % MR.REF)
    with tempfile.TemporaryDirectory(prefix="k13_") as d:
        z = compute(host_lib(pathlib.Path(d)))
    np.savez_compressed(OUT, **z)
    print("wrote %s (%d arrays, %d bytes; k9: %d bytes)" % (OUT, len(z), os.path.getsize(OUT), os.path.getsize(K9)))
    assert os.path.getsize(OUT) <= os.path.getsize(K9)
