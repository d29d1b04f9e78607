"""Generator of k10_kdtree_segment_queries.npz: the lists of KDtreeIndexed::fixedRangeSearchAlongDir,
fixedRangeSearchBetween2Points, AABBSearch, segmentSearch_all and the answers of segmentSearch_1NearestPoint from the
reference's own compiled code (oracle/_ref/libref3dtk.so).

    python tests/golden/make_golden_segments.py     (needs oracle/_ref: a build() where the reference checkout exists)

  the seven k8 clouds x buckets (1, 5, 20): every list and every nearest-point answer of every query row (k10_queries:
           query i is p = Q[i], p0 = Q[(i+7) % len(Q)], dir their normalised difference, the box their componentwise min and
           max, maxdist2 the cloud's r2; behind them five degenerate rows: p == p0 with a zero dir and a point box, a
           non-unit dir, a NaN in p / in the box's lower corner, a NaN in p0 / dir / the upper corner, a segment far outside)
  trips, deep, table, nonfinite (the clouds of make_golden_knn_edges.py): for the rows the GPU test compares where the
           reference library is not there, each list's length and the CRC-32 of its int32 entries in list order, and the
           nearest-point indices.  Clouds and queries are seeded and regenerated, none is stored.

Also imported by the tests, so that the fixture and the live reference are checked the same way."""
import ctypes as C
import importlib.util
import os
import sys
import zlib

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
OUT = os.path.join(_HERE, "k10_kdtree_segment_queries.npz")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


mgk = _load("make_golden_knn")
k8_clouds, RefTree, dist2, BUCKETS = mgk.k8_clouds, mgk.RefTree, mgk.dist2, mgk.BUCKETS

LIST_KINDS = ("along", "between", "aabb", "segall")      # the four list queries; "near" is the nearest-point query
N_DEGENERATE = 5


# ---- the reference library through ctypes ------------------------------------------------------------------------
class SegRef(RefTree):
    """RefTree + the five methods: the vector-returning four through the hidden return slot (slot, this, p, v[, maxdist2],
    threadNum), segmentSearch_1NearestPoint with a plain size_t return"""

    def __init__(self, pts, bucket):
        super().__init__(pts, bucket)
        dp = C.POINTER(C.c_double)
        R = self.R
        self.fn = {"along": R._ZNK13KDtreeIndexed24fixedRangeSearchAlongDirEPdS0_di,
                   "between": R._ZNK13KDtreeIndexed30fixedRangeSearchBetween2PointsEPdS0_di,
                   "segall": R._ZNK13KDtreeIndexed17segmentSearch_allEPdS0_di,
                   "aabb": R._ZNK13KDtreeIndexed10AABBSearchEPdS0_i,
                   "near": R._ZNK13KDtreeIndexed27segmentSearch_1NearestPointEPdS0_di}
        for kind in ("along", "between", "segall"):
            self.fn[kind].argtypes = [C.c_void_p, C.c_void_p, dp, dp, C.c_double, C.c_int]
            self.fn[kind].restype = C.c_void_p
        self.fn["aabb"].argtypes = [C.c_void_p, C.c_void_p, dp, dp, C.c_int]
        self.fn["aabb"].restype = C.c_void_p
        self.fn["near"].argtypes = [C.c_void_p, dp, dp, C.c_double, C.c_int]
        self.fn["near"].restype = C.c_size_t

    def lists(self, kind, a, b, md2):
        slot = (C.c_uint64 * 3)()
        pa = (C.c_double * 3)(*[float(v) for v in a])
        pb = (C.c_double * 3)(*[float(v) for v in b])
        if kind == "aabb":
            if (np.asarray(a) > np.asarray(b)).any():
                raise ValueError("invalid bbox (the reference would throw through ctypes)")
            self.fn[kind](C.addressof(slot), self.kdi, pa, pb, 0)
        else:
            self.fn[kind](C.addressof(slot), self.kdi, pa, pb, float(md2), 0)
        return self._read(slot)

    def nearest(self, p, p0, md2):
        pa = (C.c_double * 3)(*[float(v) for v in p])
        pb = (C.c_double * 3)(*[float(v) for v in p0])
        r = self.fn["near"](self.kdi, pa, pb, float(md2), 0)
        return -1 if r == 2 ** 64 - 1 else int(r)


def ref_lists(tree, kind, A, B, md2, rows=None):
    """CSR: (offsets uint64, idx int32) of the listed rows (all by default)"""
    rows = range(len(A)) if rows is None else rows
    lists = [tree.lists(kind, A[i], B[i], md2) for i in rows]
    off = np.zeros(len(lists) + 1, np.uint64)
    off[1:] = np.cumsum([len(l) for l in lists])
    idx = np.concatenate(lists).astype(np.int32) if lists else np.zeros(0, np.int32)
    return off, idx


def ref_nearest(tree, P, P0, md2, rows=None):
    rows = range(len(P)) if rows is None else rows
    return np.array([tree.nearest(P[i], P0[i], md2) for i in rows], np.int32)


# ---- queries ------------------------------------------------------------------------------------------------------
def _unit(d):
    """Normalize3 (globals.icc:253-259), term for term: the dir fixedRangeSearchBetween2Points computes from p and p0"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return d / np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])[..., None]


def k10_queries(pts, Q):
    """dict P, P0, DIR, LO, HI [n + N_DEGENERATE][3] and n, the number of regular rows"""
    n = len(Q)
    P = Q.copy()
    P0 = Q[(np.arange(n) + 7) % n].copy()
    P0[(P0 == P).all(1)] += 0.5
    DIR = _unit(P0 - P)
    LO, HI = np.minimum(P, P0), np.maximum(P, P0)
    nan = np.nan
    far = pts.max(0) + 1000.0
    step = np.array([1.0, 2.0, 3.0])
    a, b, c = Q[0], Q[1 % n], Q[2 % n]
    bc = c + 0.5 if (b == c).all() else c
    p_nan = np.array([nan, a[1], a[2]])
    eP = np.array([a, b, p_nan, a, far])
    eP0 = np.array([a, bc, Q[3 % n], [a[0] + 1.0, nan, a[2]], far + step])
    eDIR = np.array([[0.0, 0.0, 0.0], 2.5 * _unit(bc - b), _unit(step), [0.6, 0.8, nan], _unit(step)])
    eLO = np.array([a, np.minimum(b, bc), p_nan, pts.min(0), far])
    eHI = np.array([a, np.maximum(b, bc), pts.max(0), [a[0], nan, a[2]], far + step])
    return {"P": np.vstack([P, eP]), "P0": np.vstack([P0, eP0]), "DIR": np.vstack([DIR, eDIR]),
            "LO": np.vstack([LO, eLO]), "HI": np.vstack([HI, eHI]), "n": n}


def pair(kind, q):
    """the two vectors of a query kind"""
    if kind == "along":
        return q["P"], q["DIR"]
    if kind == "aabb":
        return q["LO"], q["HI"]
    return q["P"], q["P0"]


# ---- the walks' leaf predicates in numpy, in the reference's operation order --------------------------------------
def _len2(x):
    return (x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]) + x[..., 2] * x[..., 2]


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def comp_d2(X, p, p0):
    """Dist2(comp, x): comp the comparison point of x on the segment p .. p0 (kdTreeImpl.h:756-774)"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = p0 - p
        len2 = _len2(d)
        nrm = d / len2[..., None]
        t = _dot(X - p, d)
        proj = p + t[..., None] * nrm
        comp = np.where((t < 0.0)[..., None], p, np.where((t > len2)[..., None], p0, proj))
        return _len2(X - comp)


def leaf_take(kind, X, a, b, md2):
    """whether the walk's leaf takes point X for query (a, b); all arrays [...][3], broadcast"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if kind in ("along", "between"):
            u = b
            if kind == "between":
                u = b - a
                u = u / np.sqrt((u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2])[..., None]
            w = a - X
            dt = _dot(w, u)
            return _len2(w) - dt * dt < md2
        if kind == "aabb":
            return ((X >= a) & (X <= b)).all(-1)
        if kind == "segall":
            return comp_d2(X, a, b) < md2
        return ~(comp_d2(X, a, b) >= md2)       # "near": the candidates of the nearest-point walk


def check_lists(kind, pts, A, B, md2, off, idx):
    """every entry satisfies the leaf predicate, no index twice in a list"""
    cnt = np.diff(off.astype(np.int64))
    assert off[0] == 0 and int(off[-1]) == len(idx) and (cnt >= 0).all()
    assert ((idx >= 0) & (idx < len(pts))).all()
    row = np.repeat(np.arange(len(cnt)), cnt)
    for s in range(0, len(idx), 1_000_000):
        e = min(s + 1_000_000, len(idx))
        assert leaf_take(kind, pts[idx[s:e]], A[row[s:e]], B[row[s:e]], md2).all(), kind
    key = row.astype(np.int64) * len(pts) + idx
    assert len(np.unique(key)) == len(key), kind


def digest(off, idx):
    """(length, CRC-32 of the int32 entries in list order) per list"""
    cnt = np.diff(off.astype(np.int64)).astype(np.uint32)
    i4 = np.ascontiguousarray(idx, "<i4")
    crc = np.array([zlib.crc32(i4[int(off[i]):int(off[i + 1])].tobytes()) for i in range(len(cnt))], np.uint32)
    return cnt, crc


# ---- the large clouds (make_golden_knn_edges.py) ---------------------------------------------------------------------
FALLBACK_ROWS = 300         # rows per case recorded here; the GPU test compares more against the live library


def _offsets(seed, n, scale):
    return np.random.default_rng(seed).normal(0.0, scale, (n, 3))


def _seg_queries(P, P0):
    d = P0 - P
    return {"P": P, "P0": P0, "DIR": _unit(d), "LO": np.minimum(P, P0), "HI": np.maximum(P, P0), "n": len(P)}


def edge_case(name, bucket=20):
    """(points, query dict as k10_queries, maxdist2 per kind, the rows compared with the reference)"""
    me = _load("make_golden_knn_edges")
    if name == "trips":
        # 200,000 points in a box of 100^3 (0.2 per unit volume), segments about 1.7 long.  The two cylinder walks look
        # along the whole line: 63 maxdist2 points per query at most, so 0.09 keeps 600,000 lists below five million
        pts, Q = me.trips_cloud()
        q = _seg_queries(Q, Q + _offsets(9701, len(Q), 1.0))
        md2 = {"along": 0.09, "between": 0.09, "aabb": 0.0, "segall": 1.0, "near": 1.0}
        rows = np.sort(np.random.default_rng(9702).choice(len(Q), 2_000, replace=False))
    elif name == "deep":
        pts, geo = me.deep_cloud()
        Q = me.deep_queries(pts, geo, 300, 9710 + bucket)
        q = _seg_queries(Q, Q * 1.01 + _offsets(9711, len(Q), 1.5))
        md2 = {"along": 0.09, "between": 0.09, "aabb": 0.0, "segall": 9.0, "near": 9.0}
        rows = np.arange(len(Q))
    elif name == "table":
        pts, copies, blob = me.table_cloud()
        _, (qr0, _) = me.table_queries(pts, blob)
        q = _seg_queries(qr0, qr0 + _offsets(9721, len(qr0), 0.01))
        md2 = dict.fromkeys(LIST_KINDS + ("near",), me.TABLE_R2[0])
        rows = np.arange(len(qr0))
    elif name == "nonfinite":
        pts, Q, _, _, _ = me.nonfinite_cloud()
        P0 = np.roll(Q, 7, axis=0)
        with np.errstate(invalid="ignore", over="ignore"):
            q = _seg_queries(Q, P0)
        # (the box of a row holding a NaN: minimum / maximum give NaN corners, which pass the reference's check)
        md2 = dict.fromkeys(LIST_KINDS + ("near",), me.NONFINITE_R2)
        rows = np.arange(len(Q))
    else:
        raise KeyError(name)
    return pts, q, md2, rows


EDGE_CASES = (("trips", 20), ("deep", 1), ("deep", 20), ("table", 20), ("nonfinite", 20))


def edge_reference(name, bucket, rows_limit=None):
    """what the reference gives on the compared rows of an edge case: {kind: (off, idx)} and the nearest-point indices"""
    pts, q, md2, rows = edge_case(name, bucket)
    rows = rows if rows_limit is None else rows[:rows_limit]
    t = SegRef(pts, bucket)
    out = {}
    for kind in LIST_KINDS:
        A, B = pair(kind, q)
        out[kind] = ref_lists(t, kind, A, B, md2[kind], rows)
    out["near"] = ref_nearest(t, q["P"], q["P0"], md2["near"], rows)
    return out


# ---- the fixture --------------------------------------------------------------------------------------------------
def compute_small():
    z = {}
    for name, (pts, Q, no, r2) in k8_clouds().items():
        q = k10_queries(pts, Q)
        for key in ("P", "P0", "DIR", "LO", "HI"):
            z["%s_%s" % (name, key)] = q[key]
        for b in BUCKETS:
            t = SegRef(pts, b)
            for kind in LIST_KINDS:
                A, B = pair(kind, q)
                off, idx = ref_lists(t, kind, A, B, r2)
                z["%s_b%d_%s_off" % (name, b, kind)] = off.astype(np.uint32)
                z["%s_b%d_%s_idx" % (name, b, kind)] = idx.astype(np.int16)
            z["%s_b%d_near" % (name, b)] = ref_nearest(t, q["P"], q["P0"], r2).astype(np.int16)
    return z


def compute_edges():
    z = {}
    for name, b in EDGE_CASES:
        ref = edge_reference(name, b, FALLBACK_ROWS)
        for kind in LIST_KINDS:
            cnt, crc = digest(*ref[kind])
            z["%s_b%d_%s_cnt" % (name, b, kind)] = cnt
            z["%s_b%d_%s_crc" % (name, b, kind)] = crc
        z["%s_b%d_near" % (name, b)] = ref["near"]
    return z


def compute():
    z = compute_small()
    z.update(compute_edges())
    return z


if __name__ == "__main__":
    sys.path.insert(0, _ROOT)
    from oracle import orc
    if not orc.have_ref():
        raise SystemExit("needs oracle/_ref/libref3dtk.so (build() where the reference checkout exists)")
    z = compute()
    np.savez_compressed(OUT, **z)
    print("wrote %s (%d arrays, %d bytes)" % (OUT, len(z), os.path.getsize(OUT)))
