"""Generator of k9_kdtree_query_edges.npz: the clouds and queries of tests/test_gpu_kdtree_query_edges.py (the branches of
query.hip that the k8 cases never execute) and, for the small ones, what KDtreeIndexed::kNearestNeighbors /
fixedRangeSearch of the reference's own compiled code (oracle/_ref/libref3dtk.so) returned on them.

    python tests/golden/make_golden_knn_edges.py     (needs oracle/_ref: a build() where the reference checkout exists)

Every cloud is seeded and regenerated here, none is stored.  The fixture holds index lists and offsets only: the normals
of these cases are computed by the oracle's PCA where they are checked (the oracle library needs no reference checkout).
  table    (one 40,000-point leaf of copies, a 3,000-point leaf, leaf table mode): the k-NN rows of its 200 queries, the
           range lists of its 70 queries.  A list that runs through the leaf of copies holds that leaf's 40,000 entries
           as one contiguous run, the same for every query: the run is stored once (table_big), each such list without it
           and with the position it was cut from (strip_run / restore_run)
  deep     (a tree 80 levels deep): nothing but the lengths of the range lists of the queries the GPU test uses where the
           reference library is not there (see compute)
  short    (M points, k slots, M around k in every list band): all rows
  lattice  (16^3 integers, 2,000 queries on integers and half-integers): the rows and range lists of the first
           LATTICE_STORED queries (the queries are independent draws, so these are a uniform sample; 2,000 queries x 3
           bucket sizes x 6 k would be 600 KB deflated, tie orders do not compress), the three bucket sizes side by side
           per query, as differences to the lattice index of the query's cell.  The tests check all 2,000 against the
           live reference where it exists and against brute force where not
  nonfinite (coordinates 1e160, -1e200, +-inf, NaN among ordinary queries): all rows, all range offsets

Also imported by the tests, so that the fixture and the live reference are checked the same way."""
import importlib.util
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
OUT = os.path.join(_HERE, "k9_kdtree_query_edges.npz")


def _mgk():
    spec = importlib.util.spec_from_file_location("make_golden_knn", os.path.join(_HERE, "make_golden_knn.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


mgk = _mgk()
RefTree, ref_knn, ref_range, dist2, knn_normals, range_normals, RPOS = (
    mgk.RefTree, mgk.ref_knn, mgk.ref_range, mgk.dist2, mgk.knn_normals, mgk.range_normals, mgk.RPOS)

BAND_KS = (3, 10, 20, 32, 33, 64)     # one k in the band of every kernel: k_knn_reg<4|10|20|32> (32: a full register list),
                                      # k_knn_lds at its first and at its last k


# ---- case 1: more queries than lanes ------------------------------------------------------------------------------
def trips_cloud():
    """200,000 uniform points and 600,000 queries: own points, jittered own points, points outside the box (shuffled)"""
    rng = np.random.default_rng(9101)
    pts = rng.uniform(-50, 50, (200_000, 3))
    own = pts[rng.integers(0, len(pts), 250_000)]
    jit = pts[rng.integers(0, len(pts), 250_000)] + rng.normal(0, 0.3, (250_000, 3))
    out = rng.uniform(-70, 70, (100_000, 3))
    out[np.abs(out).max(1) <= 50] *= 1.5
    Q = np.vstack([own, jit, out])
    return pts, Q[rng.permutation(len(Q))]


def trips_normals_cloud():
    """600,000 points: uniform and four dense blobs of 2,500 (a blob point's radius list holds its whole blob)"""
    rng = np.random.default_rng(9102)
    u = rng.uniform(-50, 50, (590_000, 3))
    blobs = [c + rng.normal(0, 0.05, (2_500, 3)) for c in rng.uniform(-40, 40, (4, 3))]
    pts = np.vstack([u] + blobs)
    perm = rng.permutation(len(pts))
    return pts[perm], np.nonzero(perm >= len(u))[0]          # (points, positions of the blob points)


# ---- case 2: a deep tree ------------------------------------------------------------------------------------------
DEEP_GEO = 20_000


def deep_cloud():
    """the reference splits at the centroid: radii growing by 1 % per point peel a few points off per level.  Returns
    (points, positions of the geometric part).  Largest coordinate about 1.2e85: squared distances stay finite."""
    rng = np.random.default_rng(2001)
    v = rng.normal(size=(DEEP_GEO, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    g = (0.05 * 1.01 ** np.arange(DEEP_GEO))[:, None] * v
    u = rng.uniform(-50, 50, (280_000, 3))
    pts = np.vstack([g, u])
    perm = rng.permutation(len(pts))
    return pts[perm], np.nonzero(perm < DEEP_GEO)[0]


def deep_queries(pts, geo, n, seed):
    """n queries: a third from the geometric part, half from the uniform part, the rest outside"""
    rng = np.random.default_rng(seed)
    ng, nout = n // 3, n // 6
    uni = np.setdiff1d(np.arange(len(pts)), geo)
    out = rng.uniform(-80, 80, (nout, 3)) * np.where(rng.random((nout, 1)) < 0.2, 1e3, 1.0)
    return np.vstack([pts[rng.choice(geo, ng, replace=False)], pts[rng.choice(uni, n - ng - nout, replace=False)], out])


DEEP_BUCKETS = (1, 20)
DEEP_R2 = (9.0, 400.0)         # about 29 entries per uniform query; the inner queries' lists run through the geometric core
DEEP_FALLBACK_Q = 300          # queries of the GPU test where the reference library is not there (2,400 where it is)


def deep_range_queries(pts, geo, n, bucket):
    """the range queries of the deep-tree test at bucket size `bucket`, per r2 of DEEP_R2 (the larger on a fifth of them)"""
    Q = deep_queries(pts, geo, n, 22 + bucket)
    return Q, (Q, Q[::5])


def deep_normals_samples(pts, geo):
    """(rows whose k-NN lists are compared, rows whose range normals are compared) of the deep cloud's normals"""
    rng = np.random.default_rng(23)
    knn_rows = np.concatenate([rng.choice(geo, 100, replace=False), rng.choice(len(pts), 300, replace=False)])
    range_rows = np.concatenate([rng.choice(geo, 1_000, replace=False), rng.choice(len(pts), 2_000, replace=False)])
    return knn_rows, range_rows


# ---- case 3: leaf table mode, leaves of thousands of points ---------------------------------------------------------
TABLE_COPY = np.array([1.25, -2.5, 0.75])
TABLE_BLOB = TABLE_COPY + np.array([0.02, 0.01, 0.0])     # blob centre; half extent 0.004: 0.017 away from the copies
TABLE_COPIES = 40_000
TABLE_R2 = (2.0e-4, 1.0e-4)                               # about the blob's diagonal (0.0139^2); the radius 0.01


def table_cloud():
    """30,000 uniform points + 40,000 copies of one point + 3,000 distinct points in a box of half extent 0.004.
    Returns (points, positions of the copies, positions of the blob)"""
    rng = np.random.default_rng(9301)
    u = rng.uniform(-10, 10, (30_000, 3))
    c = np.tile(TABLE_COPY, (TABLE_COPIES, 1))
    b = TABLE_BLOB + rng.uniform(-0.004, 0.004, (3_000, 3))
    pts = np.vstack([u, c, b])
    perm = rng.permutation(len(pts))
    return pts[perm], np.nonzero((perm >= 30_000) & (perm < 70_000))[0], np.nonzero(perm >= 70_000)[0]


def table_queries(pts, blob):
    """(k-NN queries [200], range queries per r2 of TABLE_R2)"""
    rng = np.random.default_rng(9302)
    at = np.tile(TABLE_COPY, (30, 1))
    inb = np.vstack([pts[rng.choice(blob, 40, replace=False)], TABLE_BLOB + rng.uniform(-0.004, 0.004, (30, 3))])
    near = TABLE_COPY + rng.uniform(-0.03, 0.03, (40, 3))
    mid = TABLE_COPY + np.array([0.01, 0.005, 0.0]) + rng.uniform(-0.002, 0.002, (10, 3))
    far = np.vstack([pts[rng.choice(len(pts), 30, replace=False)], rng.uniform(-12, 12, (20, 3))])
    qk = np.vstack([at, inb, near, mid, far])
    # r2 = 2e-4: 8 queries at the copied point and 8 between it and the blob return the 40,000 copies (the latter with blob
    # points behind or in front of them), the others a blob's worth or nothing; r2 = 1e-4 at the copied point: the copies
    qr0 = np.vstack([at[:8], mid[:8], inb[:20], far[:10]])
    qr1 = np.vstack([at[:8], TABLE_COPY + np.array([0.0, 0.0, 0.0099]), TABLE_COPY + np.array([0.0, 0.0, 0.01]),
                     inb[:10], far[:4]])
    return qk, (qr0, qr1)


def strip_run(off, idx, run):
    """CSR lists -> (offsets and entries of the lists without the run, per list the position the run was cut from or -1)"""
    lists, pos = [], []
    for i in range(len(off) - 1):
        l = idx[int(off[i]):int(off[i + 1])]
        p = -1
        if len(run) and len(l) >= len(run):
            for s in np.nonzero(l == run[0])[0]:
                if np.array_equal(l[s:s + len(run)], run):
                    p = int(s)
                    l = np.concatenate([l[:s], l[s + len(run):]])
                    break
        lists.append(l)
        pos.append(p)
    soff = np.zeros(len(lists) + 1, np.uint64)
    soff[1:] = np.cumsum([len(l) for l in lists])
    return soff, np.concatenate(lists).astype(np.int32), np.array(pos, np.int32)


def restore_run(soff, sidx, pos, run):
    lists = []
    for i in range(len(soff) - 1):
        l = sidx[int(soff[i]):int(soff[i + 1])]
        lists.append(l if pos[i] < 0 else np.concatenate([l[:pos[i]], run, l[pos[i]:]]))
    off = np.zeros(len(lists) + 1, np.uint64)
    off[1:] = np.cumsum([len(l) for l in lists])
    return off, np.concatenate(lists).astype(np.int32)


# ---- case 4: fewer points than slots ------------------------------------------------------------------------------
SHORT_MS = (1, 2, 3, 4, 5, 9, 10, 11, 19, 20, 21, 31, 32, 33, 63, 64, 65)
SHORT_KS = (1, 2, 3, 4, 5, 10, 11, 20, 21, 32, 33, 63, 64)
SHORT_BUCKETS = (1, 20)


def short_cases():
    """(M, bucket, k) in the order of the fixture's short_knn blocks"""
    return [(M, b, k) for M in SHORT_MS for b in SHORT_BUCKETS for k in SHORT_KS]


def short_rows(flat):
    """short_knn -> {(M, bucket, k): [12][k] int32}"""
    out, at = {}, 0
    for M, b, k in short_cases():
        out[(M, b, k)] = flat[at:at + 12 * k].reshape(12, k).astype(np.int32)
        at += 12 * k
    assert at == len(flat)
    return out


def short_cloud(M):
    """(points [M], a dozen queries: own points first, then points around the cloud)"""
    rng = np.random.default_rng(9400 + M)
    pts = rng.uniform(-1, 1, (M, 3))
    no = min(M, 6)
    return pts, np.vstack([pts[rng.choice(M, no, replace=False)], rng.uniform(-2, 2, (12 - no, 3))])


# ---- case 5: split planes and exact ties --------------------------------------------------------------------------
LATTICE_N = 16
LATTICE_BUCKETS = (1, 5, 20)
LATTICE_R2 = (1.0, 2.0, 2.25, 3.0)
LATTICE_STORED = 400


def lattice_cloud():
    """the integers [0, 16)^3 (every centroid, so every split value, is an integer or a half-integer) and 2,000 queries
    on the integers and half-integers of [-1.5, 17]^3"""
    a = np.arange(float(LATTICE_N))
    g = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(9501)
    Q = rng.integers(-3, 35, (2_000, 3)) / 2.0
    return g, Q


def _lattice_base(Q):
    c = np.clip(np.floor(Q), 0, LATTICE_N - 1).astype(np.int32)
    return (c[:, 0] * LATTICE_N + c[:, 1]) * LATTICE_N + c[:, 2]


def lattice_pack_knn(Q, rows):
    """rows: one [Q][k] per bucket size -> [Q][buckets][k] int16, entries relative to the query's cell"""
    return (np.stack(rows, 1) - _lattice_base(Q)[:, None, None]).astype(np.int16)


def lattice_unpack_knn(Q, packed):
    full = packed.astype(np.int32) + _lattice_base(Q)[:, None, None]
    return [np.ascontiguousarray(full[:, j]) for j in range(full.shape[1])]


def lattice_pack_range(Q, off, idx):
    return (idx - np.repeat(_lattice_base(Q), np.diff(off.astype(np.int64)))).astype(np.int16)


def lattice_unpack_range(Q, off, packed):
    return packed.astype(np.int32) + np.repeat(_lattice_base(Q), np.diff(off.astype(np.int64)))


# ---- case 6: far and non-finite queries ---------------------------------------------------------------------------
def nonfinite_cloud():
    """(points [20,000], queries [110], positions of the ordinary queries, of the NaN ones, of the far / infinite ones)"""
    rng = np.random.default_rng(9601)
    pts = rng.uniform(-30, 30, (20_000, 3))
    inf, nan = np.inf, np.nan
    far = []
    for v in (1e160, -1e200, inf, -inf):
        far += [[v, 1.0, 2.0], [3.0, v, -4.0], [-5.0, 6.0, v], [v, v, v]]
    far += [[inf, -inf, 0.0], [1e160, -inf, 1e200]]
    nans = [[nan, 1.0, 2.0], [3.0, nan, -4.0], [-5.0, 6.0, nan], [nan, nan, 1.0], [nan, 2.0, nan], [3.0, nan, nan],
            [nan, nan, nan], [nan, inf, 0.0], [-inf, 1.0, nan], [1e200, nan, 0.0]]
    ordinary = np.vstack([pts[rng.choice(len(pts), 50, replace=False)], rng.uniform(-35, 35, (32, 3))])
    Q = np.vstack([ordinary, np.array(far), np.array(nans)])
    perm = rng.permutation(len(Q))
    inv = np.argsort(perm)
    no, nf = len(ordinary), len(far)
    return pts, Q[perm], np.sort(inv[:no]), np.sort(inv[no + nf:]), np.sort(inv[no:no + nf])


NONFINITE_R2 = 9.0


# ---- the fixture --------------------------------------------------------------------------------------------------
def compute(orc=None):
    z = {}
    # deep: list lengths only.  Far out in the geometric part the reference's box test (|q - c| - h on numbers of 1e80)
    # rounds by more than the radius and prunes the leaf that holds the query's own point: its list is not the set
    # d2 < r2 there, so brute force cannot stand in for it.  A list of the recorded length whose entries all lie within r2
    # and differ from each other is the reference's set wherever that set is complete, and as short as the reference's
    # everywhere.
    pts, geo = deep_cloud()
    for b in DEEP_BUCKETS:
        t = RefTree(pts, b)
        _, qs = deep_range_queries(pts, geo, DEEP_FALLBACK_Q, b)
        for j, (q, r2) in enumerate(zip(qs, DEEP_R2)):
            z["deep_b%d_r%d_cnt" % (b, j)] = np.diff(ref_range(t, q, r2)[0].astype(np.int64)).astype(np.uint32)
        if b == 20:
            _, rows = deep_normals_samples(pts, geo)
            z["deep_normals_cnt"] = np.diff(ref_range(t, pts[rows], DEEP_R2[0])[0].astype(np.int64)).astype(np.uint32)
        del t
    # table
    pts, copies, blob = table_cloud()
    qk, qrs = table_queries(pts, blob)
    t = RefTree(pts, 20)
    for k in BAND_KS:
        z["table_knn%d" % k] = ref_knn(t, qk, k)
    big = t.range(TABLE_COPY, TABLE_R2[1]).astype(np.int32)
    z["table_big"] = big
    for j, (q, r2) in enumerate(zip(qrs, TABLE_R2)):
        off, idx = ref_range(t, q, r2)
        soff, sidx, pos = strip_run(off, idx, big)
        z["table_r%d_off" % j] = off
        z["table_r%d_soff" % j] = soff
        z["table_r%d_sidx" % j] = sidx
        z["table_r%d_pos" % j] = pos
    del t
    # short: every (M, bucket, k) row block [12][k] behind the other, in short_cases() order
    short = []
    for M in SHORT_MS:
        pts, Q = short_cloud(M)
        for b in SHORT_BUCKETS:
            t = RefTree(pts, b)
            for k in SHORT_KS:
                short.append(ref_knn(t, Q, k).astype(np.int8).ravel())
    z["short_knn"] = np.concatenate(short)
    # lattice
    pts, Q = lattice_cloud()
    Q = Q[:LATTICE_STORED]
    trees = [RefTree(pts, b) for b in LATTICE_BUCKETS]
    for k in BAND_KS:
        z["lattice_knn%d" % k] = lattice_pack_knn(Q, [ref_knn(t, Q, k) for t in trees])
    for j, r2 in enumerate(LATTICE_R2):
        for b, t in zip(LATTICE_BUCKETS, trees):
            off, idx = ref_range(t, Q, r2)
            z["lattice_b%d_r%d_off" % (b, j)] = off.astype(np.uint32)
            z["lattice_b%d_r%d_idx" % (b, j)] = lattice_pack_range(Q, off, idx)
    del trees
    # nonfinite
    pts, Q, _, _, _ = nonfinite_cloud()
    t = RefTree(pts, 20)
    for k in BAND_KS:
        z["nonfinite_knn%d" % k] = ref_knn(t, Q, k)
    off, idx = ref_range(t, Q, NONFINITE_R2)
    z["nonfinite_roff"] = off
    z["nonfinite_ridx"] = idx
    return z


if __name__ == "__main__":
    sys.path.insert(0, _ROOT)
    from oracle import orc
    if not orc.have_ref():
        raise SystemExit("needs oracle/_ref/libref3dtk.so (build() where the reference checkout exists)")
    z = compute(orc)
    np.savez_compressed(OUT, **z)
    print("wrote %s (%d arrays, %d bytes)" % (OUT, len(z), os.path.getsize(OUT)))
