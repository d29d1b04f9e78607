"""Generator of k8_kdtree_queries.npz: KDtreeIndexed::kNearestNeighbors / fixedRangeSearch lists from the reference's own
compiled code (oracle/_ref/libref3dtk.so), on small seeded clouds that stress the walks' rules, and the normals the
oracle's PCA gives on those lists.

    python tests/golden/make_golden_knn.py        (needs oracle/_ref: a build() where the reference checkout exists)

Also imported by the tests (k8_clouds, ref_knn, ref_range, ...), so that the fixture and the live reference are checked
the same way."""
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
OUT = os.path.join(_HERE, "k8_kdtree_queries.npz")

KS = (1, 10, 20, 64)
BUCKETS = (1, 5, 20)
NORMAL_KS = (10, 20)
RPOS = np.array([0.5, -2.0, 1.0])


def k8_clouds():
    """name -> (points [M][3], queries [Q][3], number of leading queries that are the cloud's own points, r2)"""
    rng = np.random.default_rng(808)
    out = {}

    def own_and_out(pts, n_own, n_out, spread):
        sel = rng.choice(len(pts), size=min(n_own, len(pts)), replace=False)
        lo, hi = pts.min(0) - spread, pts.max(0) + spread
        q_out = rng.uniform(lo, hi, (n_out, 3))
        return np.vstack([pts[sel], q_out]), len(sel)

    u = rng.uniform(-10, 10, (900, 3))
    q, no = own_and_out(u, 60, 20, 3.0)
    out["uniform"] = (u, q, no, 4.0)
    d = rng.uniform(-5, 5, (700, 3))
    d[100:150] = d[0:50]                 # copied blocks: exact duplicates, zero distances
    d[400:420] = d[0:20]
    q, no = own_and_out(d, 60, 20, 2.0)
    out["duplicates"] = (d, q, no, 1.0)
    g = np.stack(np.meshgrid(np.arange(9.0), np.arange(9.0), np.arange(9.0), indexing="ij"), -1).reshape(-1, 3)
    ql = np.vstack([g[rng.choice(len(g), 50, replace=False)],
                    np.floor(rng.uniform(-1, 10, (10, 3))) + 0.5,              # between lattice planes: many ties
                    np.floor(rng.uniform(0, 9, (10, 3)))])                     # on the lattice (= split planes)
    out["lattice"] = (g, ql, 50, 2.0)
    p = np.column_stack([rng.uniform(-8, 8, 800), rng.uniform(-8, 8, 800), np.zeros(800)])
    q, no = own_and_out(p, 60, 20, 2.0)
    out["plane"] = (p, q, no, 2.0)
    centres = rng.uniform(-20, 20, (6, 3))
    c = np.vstack([ce + rng.normal(0, 0.02, (120, 3)) for ce in centres])
    q, no = own_and_out(c, 60, 20, 1.0)
    out["clusters"] = (c, q, no, 0.003)
    s = rng.uniform(-1, 1, (7, 3))
    q, no = own_and_out(s, 7, 5, 1.0)
    out["seven"] = (s, q, no, 0.5)
    one = np.array([[0.25, -0.5, 1.5]])
    out["one"] = (one, np.vstack([one, rng.uniform(-2, 2, (4, 3))]), 1, 1.0)
    return out


def dist2(pts, q, idx):
    """globals.icc Dist2 of the listed points (dx = point - query), -1.0 where idx < 0"""
    idx = np.asarray(idx)
    P = pts[np.maximum(idx, 0)]
    dx = P[..., 0] - q[..., 0]; dy = P[..., 1] - q[..., 1]; dz = P[..., 2] - q[..., 2]
    d = (dx * dx + dy * dy) + dz * dz
    return np.where(idx >= 0, d, -1.0)


# ---- the reference library through ctypes ------------------------------------------------------------------------
class RefTree:
    """KDtreeIndexed of the reference library (oracle/_ref).  kNearestNeighbors / fixedRangeSearch return a
    std::vector<size_t> through the x86-64 hidden return slot: (slot, this, args...).  Single thread, threadNum 0;
    the vectors' buffers are leaked (a few KB per test)."""

    def __init__(self, pts, bucket):
        from oracle import orc
        self.R = orc.ref()
        self.pts = np.ascontiguousarray(pts, np.float64)
        self.h = self.R.ref_kdi_create(self.pts.ctypes.data_as(C.POINTER(C.c_double)), len(self.pts), int(bucket))
        self.kdi = C.c_void_p.from_address(self.h + 24).value     # RefTree { vector<double*> ptrs; KDtreeIndexed* tree; }
        self.knn_fn = self.R._ZNK13KDtreeIndexed17kNearestNeighborsEPdii
        self.knn_fn.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_int, C.c_int]
        self.knn_fn.restype = C.c_void_p
        self.rng_fn = self.R._ZNK13KDtreeIndexed16fixedRangeSearchEPddi
        self.rng_fn.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_double, C.c_int]
        self.rng_fn.restype = C.c_void_p

    def __del__(self):
        if getattr(self, "h", None):
            self.R.ref_kdi_destroy(self.h)

    @staticmethod
    def _read(slot):
        b, e = slot[0], slot[1]
        if not b:
            return np.zeros(0, np.int64)
        n = (e - b) // 8
        return np.array((C.c_uint64 * n).from_address(b), np.int64)

    def knn(self, q, k):
        slot = (C.c_uint64 * 3)()
        p = (C.c_double * 3)(*[float(v) for v in q])
        self.knn_fn(C.addressof(slot), self.kdi, p, int(k), 0)
        return self._read(slot)

    def range(self, q, r2):
        slot = (C.c_uint64 * 3)()
        p = (C.c_double * 3)(*[float(v) for v in q])
        self.rng_fn(C.addressof(slot), self.kdi, p, float(r2), 0)
        return self._read(slot)


def ref_knn(tree, Q, k):
    """[Q][k] int32, -1 beyond the list"""
    out = -np.ones((len(Q), k), np.int32)
    for i, q in enumerate(Q):
        r = tree.knn(q, k)
        out[i, :len(r)] = r
    return out


def ref_range(tree, Q, r2):
    """CSR: (offsets [Q+1] uint64, idx int32)"""
    lists = [tree.range(q, r2) for q in Q]
    off = np.zeros(len(Q) + 1, np.uint64)
    off[1:] = np.cumsum([len(l) for l in lists])
    idx = np.concatenate(lists).astype(np.int32) if lists else np.zeros(0, np.int32)
    return off, idx


def _pca(orc, q, nbrs, rpos=RPOS):
    """orc.normals_from_knn computes the normal of every row of its point array: the query first, its list behind it,
    one list row per point row"""
    m = len(nbrs)
    xyz = np.vstack([q.reshape(1, 3), nbrs])
    lists = np.tile(np.arange(1, m + 1, dtype=np.int32), (m + 1, 1))
    return orc.normals_from_knn(xyz, lists, rpos)[0]


def knn_normals(orc, pts, Q, knn, rpos=RPOS):
    """calculateNormal on each row's list (the rows' queries are cloud points): rows have min(k, M) entries"""
    m = int((knn[0] >= 0).sum())
    nrm = np.empty((len(Q), 3))
    for i in range(len(Q)):
        nrm[i] = _pca(orc, Q[i], pts[knn[i, :m]], rpos)
    return nrm


def range_normals(orc, pts, Q, off, idx, rpos=RPOS):
    nrm = np.empty((len(Q), 3))
    for i in range(len(Q)):
        nrm[i] = _pca(orc, Q[i], pts[idx[int(off[i]):int(off[i + 1])]], rpos)
    return nrm


def compute(orc):
    z = {}
    for name, (pts, Q, no, r2) in k8_clouds().items():
        z[name + "_pts"] = pts
        z[name + "_q"] = Q
        z[name + "_own"] = np.array([no])
        z[name + "_r2"] = np.array([r2])
        for b in BUCKETS:
            t = RefTree(pts, b)
            for k in KS:
                z["%s_b%d_knn%d" % (name, b, k)] = ref_knn(t, Q, k)
            off, idx = ref_range(t, Q, r2)
            z["%s_b%d_roff" % (name, b)] = off
            z["%s_b%d_ridx" % (name, b)] = idx
            for k in NORMAL_KS:
                z["%s_b%d_nknn%d" % (name, b, k)] = knn_normals(orc, pts, Q[:no], z["%s_b%d_knn%d" % (name, b, k)][:no])
            z["%s_b%d_nrange" % (name, b)] = range_normals(orc, pts, Q[:no], off[:no + 1], idx)
    return z


if __name__ == "__main__":
    sys.path.insert(0, _ROOT)
    from oracle import orc
    if not orc.have_ref():
        raise SystemExit("needs oracle/_ref/libref3dtk.so (build() where the reference checkout exists)")
    z = compute(orc)
    np.savez_compressed(OUT, **z)
    print("wrote %s (%d arrays, %d bytes)" % (OUT, len(z), os.path.getsize(OUT)))
