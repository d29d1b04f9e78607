"""k nearest within a radius (k_knnr_reg<4|10|20|32>, k_knnr_lds, each with and without the PCA) on the branches that
tests/test_gpu_knn_range.py never executes: k strictly inside every list band, normals at KC = 32 and on a full LDS list, a
lane's second grid-stride trip, the stack's HBM overflow on a tree 80 levels deep, leaf table mode, lists shorter than k,
queries on split planes and points at d2 == r2, far and non-finite queries, radii at the ends of the finite range, the
optional outputs, the order of calls on the shared workspaces -- and the invariant the result extraction rests on: a tree
never holds a non-finite point.

Every comparison is exact.  Rows are compared, as coordinates, with the reference's compiled kd.cc where
oracle/_ref/libref_kd.so travelled (LIVE), else with the k13 fixture (tests/golden/make_golden_knn_range_edges.py) for the
stored cases and with brute force (the sorted distances below r2) for the others; normals with the oracle's PCA on the
device's lists.  Each test first asserts the precondition that makes it reach its branch and prints it."""
import ctypes as C
import importlib.util
import os
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
pytestmark = pytest.mark.gpu

# query.hip's launch geometry, restated: a lane takes a second query beyond Q_MAX_BLOCKS x block size queries
Q_MAX_BLOCKS, Q_BLOCK, Q_BLOCK_L, Q_SD = 2048, 128, 64, 16

dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))


@pytest.fixture(scope="module")
def ge():
    spec = importlib.util.spec_from_file_location("make_golden_knn_range_edges", os.path.join(G, "make_golden_knn_range_edges.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def fx(ge):
    return ge.load()


@pytest.fixture(scope="module")
def live(ge):
    """the reference's kd.cc as built by oracle/build_ref.sh -- never the checkout"""
    return ge.MR.have_lib()


def _bits_for(v):
    return int(v).bit_length()


def _check_rows(ge, pts, Q, idx, d2, cnt, k):
    """-1 / -1.0 behind the entries, d2 = Dist2 of the returned points, ascending"""
    assert idx.shape == d2.shape == (len(Q), k) and cnt.shape == (len(Q),)
    behind = np.arange(k)[None, :] >= cnt[:, None]
    assert np.array_equal(idx < 0, behind) and (idx[behind] == -1).all() and (d2[behind] == -1.0).all()
    assert (idx < len(pts)).all()
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, len(Q), 100_000):
            e = min(s + 100_000, len(Q))
            assert np.array_equal(d2[s:e], ge.MR.G8.dist2(pts, Q[s:e, None, :], idx[s:e]))
    assert (np.diff(np.where(behind, np.finfo(np.float64).max, d2), axis=1) >= 0).all()


def _equals_reference(ge, t, pts, Q, rows, idx, cnt, k, r2):
    """the rows `rows` of a batch against RefKD t, coordinate for coordinate"""
    rows = np.asarray(rows)
    coords, want = t.search(Q[rows], k, r2)
    assert np.array_equal(cnt[rows], want), (k, r2)
    have = np.arange(k)[None, :] < want[:, None]
    assert np.array_equal(pts[idx[rows]][have], coords[have]), (k, r2)


def _equals_stored_rows(ge, fx, c, ri, k, idx, cnt):
    assert np.array_equal(cnt, fx.counts(c, ri, k)), (c.name, ri, k)
    rep = fx.rows(c, ri, k)
    have = idx >= 0
    assert np.array_equal(have, rep >= 0) and np.array_equal(c.pts[idx[have]], c.pts[rep[have]]), (c.name, ri, k)


def _sorted_range_rows(kd, Q, r2, k):
    """fixedRangeSearchBatch's lists, each stably sorted by d2, as [Q][k] rows (-1 behind; rows longer than k are cut) and
    their full lengths"""
    off, ridx, rd2 = kd.fixedRangeSearchBatch(Q, r2)
    cnt = np.diff(off.astype(np.int64))
    row = np.repeat(np.arange(len(Q)), cnt)
    o = np.lexsort((np.arange(len(ridx)), rd2, row))
    pos = np.arange(len(ridx)) - np.repeat(off[:-1].astype(np.int64), cnt)
    keep = pos < k
    rows = -np.ones((len(Q), k), np.int32)
    rows[row[keep], pos[keep]] = ridx[o][keep]
    return rows, cnt


def _normals_of_lists(orc, pts, own, knn, cnt, rpos):
    """calculateNormal of the oracle over each row's first cnt entries, the rows grouped by their length (own: the points the
    rows belong to).  A row of no entry: NaN, the reference's 0 / 0"""
    rp = np.ascontiguousarray(rpos, np.float64)
    out = np.full((len(own), 3), np.nan)
    for m in np.unique(cnt):
        rows = np.nonzero(cnt == m)[0]
        if m == 0:
            continue
        xyz = np.ascontiguousarray(np.vstack([own[rows], pts]))
        lists = np.ascontiguousarray(knn[rows, :m] + len(rows), np.int32)
        part = np.empty((len(rows), 3))
        orc.lib().orc_normals_from_knn(dp(xyz), len(rows), int(m), ip(lists), dp(rp), dp(part))
        out[rows] = part
    return out


# ---- 1. every band, k inside it ---------------------------------------------------------------------------------------
def test_every_band_with_k_inside_it(tdtk, gpu, ge, live):
    """ListReg<10|20|32> with k0 = KC - k > 0 under RANGE (k12 has that for ListReg<4> and k = 1 only): the -0.0 front slots
    together with bound = L.full() ? L.kth : r2 and the nr count; the LDS list at its first k, inside and at its last"""
    mr = ge.MR
    f12 = mr.load()
    n = 0
    for name, (pts, Q, no, _) in mr.G8.k8_clouds().items():
        Ds = np.sort(ge.all_d2(pts, Q), axis=1)
        for b in mr.BUCKETS:
            kd = tdtk.KDtree(pts, b)
            t = mr.RefKD(pts, b) if live else None
            for r2 in f12.radii(name):
                want_r, full = (None, None) if live or r2 == ge.HUGE else _sorted_range_rows(kd, Q, r2, max(ge.EDGE_KS))
                inball = (Ds < r2).sum(1)
                for k in ge.EDGE_KS:
                    idx, d2, cnt = kd.kNearestRangeSearchBatch(Q, k, r2)
                    _check_rows(ge, pts, Q, idx, d2, cnt, k)
                    assert np.array_equal(cnt, np.minimum(inball, k)), (name, b, r2, k)
                    m = np.arange(k)[None, :] < cnt[:, None]
                    D = np.pad(Ds[:, :k], ((0, 0), (0, max(0, k - Ds.shape[1]))))
                    assert np.array_equal(np.where(m, d2, -1.0), np.where(m, D, -1.0)), (name, b, r2, k)
                    if live:
                        _equals_reference(ge, t, pts, Q, np.arange(len(Q)), idx, cnt, k, r2)
                    elif r2 == ge.HUGE:
                        assert np.array_equal(d2, kd.kNearestNeighborsBatch(Q, k)[1]), (name, b, k)
                    else:
                        short = cnt < k
                        assert np.array_equal(idx[short], want_r[short][:, :k]), (name, b, r2, k)
                    n += 1
    assert n == 7 * 3 * 3 * len(ge.EDGE_KS)


# ---- 2. normals in every band ----------------------------------------------------------------------------------------
def test_normals_in_every_band(tdtk, orc, gpu, ge):
    """k_knnr_reg<32, true> (k = 21, 31, 32: never run before) and the LDS list with the PCA up to its last slot (k = 64)"""
    mr = ge.MR
    f12 = mr.load()
    lens = set()
    for name, (pts, Q, no, _) in mr.G8.k8_clouds().items():
        for b in mr.BUCKETS:
            kd = tdtk.KDtree(pts, b)
            for r2 in f12.radii(name):
                for k in (3, 9, 19, 21, 31, 32, 34, 64):
                    nrm, knn, cnt = tdtk.calculateNormalsKNNRange(pts, k, r2, mr.RPOS, bucketSize=b, want_knn=True)
                    idx, _, c2 = kd.kNearestRangeSearchBatch(pts, k, r2)
                    assert np.array_equal(knn, idx) and np.array_equal(cnt, c2), (name, b, r2, k)
                    assert (cnt >= 1).all()
                    assert np.array_equal(nrm, _normals_of_lists(orc, pts, pts, knn, cnt, mr.RPOS), equal_nan=True), (name, b, r2, k)
                    lens |= set(cnt.tolist())
    assert {1, 2, 21, 31, 32, 34, 64} <= lens


# ---- 3. second trips ---------------------------------------------------------------------------------------------------
def test_second_grid_stride_trips(tdtk, gpu, ge, fx, live):
    pts, _ = ge.cloud("trips")
    Q, sample = ge.trips_queries()
    K = len(Q)
    assert K > Q_MAX_BLOCKS * Q_BLOCK and K > 2 * Q_MAX_BLOCKS * Q_BLOCK_L and 50_000 < Q_MAX_BLOCKS * Q_BLOCK_L
    (c,) = ge.cases(("trips",))
    print("second trips: %d queries, %d lanes of the register kernels, %d of the LDS kernel; middle r2 %.17g"
          % (K, Q_MAX_BLOCKS * Q_BLOCK, Q_MAX_BLOCKS * Q_BLOCK_L, c.r2s[0]))
    kd = tdtk.KDtree(pts, 20)
    rng = np.random.default_rng(1302)
    t = ge.MR.RefKD(pts, 20) if live else None
    sub = np.sort(rng.choice(K, 20_000, replace=False)) if live else None
    shuffle = rng.permutation(K)
    brute = sample[::4]
    Ds = None
    for ri, r2 in enumerate(c.r2s):
        for k in ge.TRIPS_KS:
            idx, d2, cnt = kd.kNearestRangeSearchBatch(Q, k, r2)
            _check_rows(ge, pts, Q, idx, d2, cnt, k)
            print("second trips, r2 %g k %d: %.3f of the lists are full" % (r2, k, (cnt == k).mean()))
            if ri == 0:          # the middle radius: mostly full lists at k = 3, mostly short ones above
                assert ((cnt == k).mean() > 0.5) if k == 3 else ((cnt < k).mean() > 0.5), k
            else:
                assert (cnt == k).all()
            if live:
                _equals_reference(ge, t, pts, Q, sub, idx, cnt, k, r2)
            else:
                if Ds is None:
                    Ds = np.vstack([np.sort(ge.all_d2(pts, Q[brute[s:s + 50]]), axis=1)[:, :65] for s in range(0, len(brute), 50)])
                want = np.minimum((Ds < r2).sum(1), k)
                assert np.array_equal(cnt[brute], want), (k, r2)
                m = np.arange(k)[None, :] < want[:, None]
                assert np.array_equal(np.where(m, d2[brute], -1.0), np.where(m, Ds[:, :k], -1.0)), (k, r2)
            assert np.array_equal(cnt[sample], fx.counts(c, ri, k)), (k, r2)
            assert ge.crc_rows(ge.coords_of(pts, idx[sample]), cnt[sample]) == fx.crc(c, ri, k), (k, r2)
            # batch invariance: 50,000 queries alone are one trip per lane in every kernel
            for s in (0, 125_000, 250_000):
                i1, d1, c1 = kd.kNearestRangeSearchBatch(Q[s:s + 50_000], k, r2)
                assert np.array_equal(i1, idx[s:s + 50_000]) and np.array_equal(d1, d2[s:s + 50_000]) and \
                    np.array_equal(c1, cnt[s:s + 50_000]), (k, r2, s)
            i2, dd2, c2 = kd.kNearestRangeSearchBatch(Q[shuffle], k, r2)
            assert np.array_equal(i2, idx[shuffle]) and np.array_equal(dd2, d2[shuffle]) and np.array_equal(c2, cnt[shuffle]), (k, r2)


# ---- 4. deep tree, lists --------------------------------------------------------------------------------------------------
# every how many-th query the live reference answers (Q is laid out part by part: a stride keeps the third that lies in the
# geometric part).  With every far child pushed its walk prunes next to nothing: 22 ms per query at k = 64 (CPU, bucket 1)
DEEP_REF_STRIDE = {3: 1, 9: 16, 19: 32, 31: 48, 33: 48, 64: 96}


@pytest.fixture(scope="module")
def deep_trees(tdtk, gpu, ge, live):
    """bucket -> (the stored case, the device tree, the live reference's tree or None, the queries), made once for the cases below"""
    pts, geo = ge.cloud("deep")
    out = {}
    for c in ge.cases(("deep",)):
        n = 2_400 if live else ge.ME.DEEP_FALLBACK_Q
        Q = ge.ME.deep_queries(pts, geo, n, 22 + c.bucket)
        assert live or np.array_equal(Q, c.Q)
        out[c.bucket] = (c, tdtk.KDtree(pts, c.bucket), ge.MR.RefKD(pts, c.bucket) if live else None, Q)
    return out


# One case per (bucket, radius, k): with every far child pushed a lane of the deep cloud walks most of the tree, and a launch
# lasts as long as its slowest lane -- seconds at bucket 1 and k = 64, however few the queries.
@pytest.mark.parametrize("k", [3, 9, 19, 31, 33, 64])
@pytest.mark.parametrize("ri", [0, 1], ids=["finite", "1e30"])
@pytest.mark.parametrize("bucket", [1, 20])
def test_deep_tree_lists_on_the_overflow_stack(tdtk, gpu, ge, fx, live, deep_trees, bucket, ri, k):
    c, kd, t, Q = deep_trees[bucket]
    pts, r2 = c.pts, c.r2s[ri]
    assert c.ks == ge.BAND_KS and c.r2s == (ge.DEEP_FINITE_R2, ge.HUGE)
    info = kd.info()
    assert info["max_depth"] >= 4 * Q_SD
    sp = fx.maxsp(c, ri, k)
    over = int((sp > Q_SD).sum())
    t0 = time.perf_counter()
    idx, d2, cnt = kd.kNearestRangeSearchBatch(Q, k, r2)
    print("deep cloud, bucket %d: max_depth %d; r2 %g k %d: recorded max_sp > Q_SD for %d of %d queries, largest %d; %d queries "
          "in %.2f s" % (bucket, info["max_depth"], r2, k, over, len(sp), sp.max(), len(Q), time.perf_counter() - t0))
    assert over >= 100
    _check_rows(ge, pts, Q, idx, d2, cnt, k)
    if live:
        _equals_reference(ge, t, pts, Q, np.arange(0, len(Q), DEEP_REF_STRIDE[k]), idx, cnt, k, r2)
    else:
        assert np.array_equal(cnt, fx.counts(c, ri, k))
        assert ge.crc_rows(ge.coords_of(pts, idx), cnt) == fx.crc(c, ri, k)


@pytest.mark.parametrize("bucket", [1, 20])
def test_deep_tree_lists_are_the_same_after_a_shallow_trees_call(tdtk, gpu, ge, deep_trees, bucket):
    """a shallow tree's k_knnr launches ask for no overflow area; the deep tree's next call gets its own again"""
    c, kd, _, Q = deep_trees[bucket]
    assert kd.info()["max_depth"] >= 4 * Q_SD and kd.verify() == [0, 0, 0, 0]
    calls = ((0, 3), (0, 33), (1, 64))
    first = {(ri, k): kd.kNearestRangeSearchBatch(Q, k, c.r2s[ri]) for ri, k in calls}
    shallow_pts = np.random.default_rng(21).uniform(-5, 5, (5_000, 3))
    sh = tdtk.KDtree(shallow_pts, 20)
    assert sh.info()["max_depth"] <= Q_SD - 1
    for ri, k in calls:
        sh.kNearestRangeSearchBatch(shallow_pts, 33, 0.25)
        sh.kNearestRangeSearchBatch(shallow_pts, 3, 1e30)
        got = kd.kNearestRangeSearchBatch(Q, k, c.r2s[ri])
        for a, b in zip(got, first[(ri, k)]):
            assert a.dtype == b.dtype and np.array_equal(a, b), (ri, k)


# ---- 5. deep tree, normals ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [9, 33])
def test_deep_tree_normals_overflow_columns_reused(tdtk, orc, gpu, ge, k):
    """300,000 points are more than the 262,144 lanes of the capped grid (131,072 of the LDS kernel): a lane's column of the
    overflow area serves more than one query"""
    pts, geo = ge.cloud("deep")
    n = len(pts)
    assert n > Q_MAX_BLOCKS * Q_BLOCK and n > 2 * Q_MAX_BLOCKS * Q_BLOCK_L
    r2 = ge.DEEP_FINITE_R2
    kd = tdtk.KDtree(pts, 20)
    assert kd.info()["max_depth"] >= 4 * Q_SD
    nrm, knn, cnt = tdtk.calculateNormalsKNNRange(pts, k, r2, ge.ME.RPOS, bucketSize=20, want_knn=True)
    idx, d2, c2 = kd.kNearestRangeSearchBatch(pts, k, r2)
    assert np.array_equal(knn, idx) and np.array_equal(cnt, c2)
    _check_rows(ge, pts, pts, idx, d2, c2, k)
    print("deep normals, k %d: %d points, %d lists shorter than k, %d empty" % (k, n, (cnt < k).sum(), (cnt == 0).sum()))
    assert np.array_equal(nrm, _normals_of_lists(orc, pts, pts, knn, cnt, ge.ME.RPOS), equal_nan=True)


# ---- 6. table mode ----------------------------------------------------------------------------------------------------------
def test_table_mode_leaf_of_equal_distances(tdtk, orc, gpu, ge, fx, live):
    """the a.leaf_tab branch of leaf_span under the k_knnr kernels; in the leaf of 40,000 copies the row is the first k in
    visiting order and kth <= md drops every later copy"""
    (c,) = ge.cases(("table",))
    pts = c.pts
    kd = tdtk.KDtree(pts, 20)
    info = kd.info()
    print("table cloud: n %d, max_leaf_points %d, max_depth %d" % (info["n_points"], info["max_leaf_points"], info["max_depth"]))
    assert _bits_for(info["n_points"]) + _bits_for(info["max_leaf_points"]) > 30       # kd_build.cpp's packing rule
    assert info["max_leaf_points"] >= ge.ME.TABLE_COPIES and kd.verify() == [0, 0, 0, 0]
    assert c.r2s == ge.ME.TABLE_R2 + (ge.HUGE,)
    t = ge.MR.RefKD(pts, 20) if live else None
    is_copy = np.zeros(len(pts), bool)
    is_copy[c.copies] = True
    mixed = 0
    for ri, r2 in enumerate(c.r2s):
        for k in c.ks:
            idx, d2, cnt = kd.kNearestRangeSearchBatch(c.Q, k, r2)
            _check_rows(ge, pts, c.Q, idx, d2, cnt, k)
            if live:
                _equals_reference(ge, t, pts, c.Q, np.arange(len(c.Q)), idx, cnt, k, r2)
            _equals_stored_rows(ge, fx, c, ri, k, idx, cnt)
            cp = is_copy[np.maximum(idx, 0)] & (idx >= 0)
            assert fx.big(c, ri, k)[cp.any(1)].all() and (cp.all(1)).sum() >= 16
            mixed = max(mixed, int((cp.any(1) & ~cp.all(1)).sum()))
            # the copies of a row are distinct points of the leaf
            for i in np.nonzero(cp.any(1))[0]:
                assert len(np.unique(idx[i][cp[i]])) == cp[i].sum()
    print("table cloud: up to %d rows per batch take blob points in front of the copies" % mixed)
    assert mixed >= 8
    for k in (10, 33):
        nrm, knn, cnt = tdtk.calculateNormalsKNNRange(pts, k, ge.ME.TABLE_R2[0], ge.ME.RPOS, bucketSize=20, want_knn=True)
        idx, _, c2 = kd.kNearestRangeSearchBatch(pts, k, ge.ME.TABLE_R2[0])
        assert np.array_equal(knn, idx) and np.array_equal(cnt, c2), k
        assert (cnt[c.copies] == k).all() and is_copy[knn[c.copies]].all()
        assert np.array_equal(nrm, _normals_of_lists(orc, pts, pts, knn, cnt, ge.ME.RPOS), equal_nan=True), k   # copies: zero covariance


# ---- 7. short clouds ----------------------------------------------------------------------------------------------------------
def test_short_clouds_in_every_band(tdtk, orc, gpu, ge, fx, live):
    """M points, k slots, M around k: unset slots behind the entries of every list form, nr < k in the PCA, at a radius that
    holds everything and at one that holds about half the cloud"""
    n = 0
    for c in ge.cases(("short",)):
        kd = tdtk.KDtree(c.pts, c.bucket)
        assert kd.verify() == [0, 0, 0, 0]
        t = ge.MR.RefKD(c.pts, c.bucket) if live else None
        for ri, r2 in enumerate(c.r2s):
            for k in c.ks:
                idx, d2, cnt = kd.kNearestRangeSearchBatch(c.Q, k, r2)
                _check_rows(ge, c.pts, c.Q, idx, d2, cnt, k)
                if ri == 0:
                    assert (cnt == min(k, c.M)).all()
                if live:
                    _equals_reference(ge, t, c.pts, c.Q, np.arange(len(c.Q)), idx, cnt, k, r2)
                _equals_stored_rows(ge, fx, c, ri, k, idx, cnt)
                nrm, knn, nc = tdtk.calculateNormalsKNNRange(c.pts, k, r2, ge.ME.RPOS, bucketSize=c.bucket, want_knn=True)
                i2, _, c2 = kd.kNearestRangeSearchBatch(c.pts, k, r2)
                assert np.array_equal(knn, i2) and np.array_equal(nc, c2), (c.name, ri, k)
                assert np.array_equal(nrm, _normals_of_lists(orc, c.pts, c.pts, knn, nc, ge.ME.RPOS), equal_nan=True), (c.name, ri, k)
                n += 1
    assert n == len(ge.ME.SHORT_MS) * len(ge.ME.SHORT_BUCKETS) * len(ge.ME.SHORT_KS) * 2


# ---- 8. planes and ties -------------------------------------------------------------------------------------------------------
def test_split_planes_and_points_at_the_radius(tdtk, gpu, ge, fx, live):
    """myd == 0 (child1 first, the far child pushed because 0 < r2) and d2 == r2 (md >= r2 skips) with lists that fill
    mid-walk: 2,000 queries on the integers and half-integers around the lattice 16^3"""
    pts, Q = ge.cloud("lattice")
    D = ge.all_d2(pts, Q)
    Ds = np.sort(D, axis=1)[:, :64]
    stored = {c.bucket: c for c in ge.cases(("lattice",))}
    S = ge.ME.LATTICE_STORED
    for b in ge.ME.LATTICE_BUCKETS:
        kd = tdtk.KDtree(pts, b)
        assert kd.verify() == [0, 0, 0, 0]
        c = stored[b]
        t = ge.MR.RefKD(pts, b) if live else None
        for ri, r2 in enumerate(ge.ME.LATTICE_R2):
            inball = (D < r2).sum(1)
            assert (D == r2).any() and inball.any()
            for k in ge.BAND_KS:
                idx, d2, cnt = kd.kNearestRangeSearchBatch(Q, k, r2)
                _check_rows(ge, pts, Q, idx, d2, cnt, k)
                assert np.array_equal(cnt, np.minimum(k, inball)), (b, r2, k)
                m = np.arange(k)[None, :] < cnt[:, None]
                assert np.array_equal(np.where(m, d2, -1.0), np.where(m, Ds[:, :k], -1.0)), (b, r2, k)
                if live:
                    _equals_reference(ge, t, pts, Q, np.arange(len(Q)), idx, cnt, k, r2)
                _equals_stored_rows(ge, fx, c, ri, k, idx[:S], cnt[:S])


# ---- 9. far and non-finite queries, extreme radii -----------------------------------------------------------------------------
def test_far_and_non_finite_queries_and_extreme_radii(tdtk, gpu, ge, fx, live):
    (c,) = ge.cases(("nonfinite",))
    pts, Q, i_ord, i_nan, i_far = c.pts, c.Q, c.i_ord, c.i_nan, c.i_far
    assert len(i_ord) + len(i_nan) + len(i_far) == len(Q) and c.r2s == (9.0, 5e-324, 1e-300, ge.DBL_MAX, 1e30)
    kd = tdtk.KDtree(pts, 20)
    t = ge.MR.RefKD(pts, 20) if live else None
    own = np.zeros(len(Q), bool)          # the ordinary queries that are points of the cloud
    with np.errstate(invalid="ignore", over="ignore"):
        own[i_ord] = (ge.all_d2(pts, Q[i_ord]) == 0.0).any(1)
    assert own.sum() >= 50
    with np.errstate(invalid="ignore", over="ignore"):
        for ri, r2 in enumerate(c.r2s):
            for k in c.ks:
                idx, d2, cnt = kd.kNearestRangeSearchBatch(Q, k, r2)
                # NaN: every distance is NaN, nothing is skipped, nothing counts; far: d2 = inf >= r2 for every finite r2
                assert (cnt[i_nan] == 0).all() and (idx[i_nan] == -1).all() and (d2[i_nan] == -1.0).all(), (r2, k)
                assert (cnt[i_far] == 0).all() and (idx[i_far] == -1).all() and (d2[i_far] == -1.0).all(), (r2, k)
                _check_rows(ge, pts, Q, idx, d2, cnt, k)
                if live:
                    _equals_reference(ge, t, pts, Q, np.arange(len(Q)), idx, cnt, k, r2)
                _equals_stored_rows(ge, fx, c, ri, k, idx, cnt)
                io, do, co = kd.kNearestRangeSearchBatch(Q[i_ord], k, r2)          # the ordinary rows, queried alone
                assert np.array_equal(io, idx[i_ord]) and np.array_equal(do, d2[i_ord]) and np.array_equal(co, cnt[i_ord]), (r2, k)
                if r2 in (5e-324, 1e-300):
                    # nothing but exact duplicates of the query (d2 == 0).  Not every one of them: a node's box is
                    # fl((min+max)/2) +- fl((max-min)/2) and may exclude one of its own points by an ulp, and that ulp
                    # squared is above such a radius -- 3 of the 50 own-point queries find nothing, in the reference too
                    assert (cnt <= own).all() and cnt.sum() >= 40 and (d2[cnt == 1, 0] == 0.0).all(), (r2, k)
                if r2 >= ge.DBL_MAX or r2 == 1e30:
                    assert (cnt[i_ord] == k).all()


# ---- 10. optional outputs and wrappers ------------------------------------------------------------------------------------------
def test_optional_outputs_and_wrappers(tdtk, gpu, ge):
    L = tdtk.lib()
    rng = np.random.default_rng(1310)
    pts = rng.uniform(-10, 10, (30_000, 3))
    pts[500:520] = pts[0:20]
    Q = np.ascontiguousarray(np.vstack([pts[:300], rng.uniform(-12, 12, (300, 3))]))
    kd = tdtk.KDtree(pts, 20)
    r2 = 1.5
    for k in (3, 9, 19, 31, 33, 64):
        idx, d2, cnt = kd.kNearestRangeSearchBatch(Q, k, r2)
        assert (cnt < k).any() and (cnt == k).any() or k == 64
        for want_d2 in (False, True):
            for want_cnt in (False, True):
                gi = np.full((len(Q), k), -7, np.int32); gd = np.full((len(Q), k), -7.0); gc = np.full(len(Q), -7, np.int32)
                assert L.tdtk_knn_range_search(kd._h, dp(Q), len(Q), k, r2, ip(gi), dp(gd) if want_d2 else None,
                                               ip(gc) if want_cnt else None) == 0
                assert np.array_equal(gi, idx), (k, want_d2, want_cnt)
                assert np.array_equal(gd, d2) if want_d2 else (gd == -7.0).all()
                assert np.array_equal(gc, cnt) if want_cnt else (gc == -7).all()
        for i in (0, 5, 299, 300, 599):
            assert kd.kNearestRangeSearch(Q[i], k, r2) == idx[i, :cnt[i]].tolist(), (k, i)
    # tdtk_normals_knn_range: WS_IDX is laid out lists | counts, with no lists (L = 0) when knn_out is NULL
    sub = np.ascontiguousarray(pts[:6_000])
    rp = np.ascontiguousarray(ge.ME.RPOS, np.float64)
    r2 = 4.0
    for k in (9, 33):
        nrm, knn, cnt = tdtk.calculateNormalsKNNRange(sub, k, r2, rp, bucketSize=20, want_knn=True)
        assert (cnt < k).any() and (cnt == k).any()
        for want_knn in (False, True):
            for want_cnt in (False, True):
                gn = np.full((len(sub), 3), -7.0); gk = np.full((len(sub), k), -7, np.int32); gc = np.full(len(sub), -7, np.int32)
                assert L.tdtk_normals_knn_range(dp(sub), len(sub), k, r2, dp(rp), 20, 0, dp(gn), ip(gk) if want_knn else None,
                                                ip(gc) if want_cnt else None) == 0
                assert np.array_equal(gn, nrm, equal_nan=True), (k, want_knn, want_cnt)
                assert np.array_equal(gk, knn) if want_knn else (gk == -7).all()
                assert np.array_equal(gc, cnt) if want_cnt else (gc == -7).all()
    # a tree over two resident scans: the indices count through the concatenation
    sa = tdtk.Scan([0, 0, 0], [0, 0, 0], pts[:11_000], bucketSize=20)
    sb = tdtk.Scan([0, 0, 0], [0, 0, 0], pts[11_000:], bucketSize=20)
    km = tdtk.MetaScan([sa, sb]).getSearchTree()
    for k in (3, 33):
        for a, b in zip(km.kNearestRangeSearchBatch(Q, k, 1.5), kd.kNearestRangeSearchBatch(Q, k, 1.5)):
            assert np.array_equal(a, b), k
    assert (kd.kNearestRangeSearchBatch(Q, 33, 1.5)[0] >= 11_000).any()


# ---- 11. call order ---------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_calls_before_them(tdtk, gpu, ge):
    """the k_knnr launches share the context's workspaces with everything else (WS_IDX as lists | counts, WS_TMPB, the
    overflow area a shallow tree does not ask for): each call below gives what the same call gave first, whatever ran in
    between"""
    me = ge.ME
    dpts, geo = ge.cloud("deep")
    tpts, _, blob = ge.cloud("table")
    spts, _ = ge.cloud("trips")
    Qbig, _ = ge.trips_queries()
    spts = spts[:20_000]
    deep, shallow, table = tdtk.KDtree(dpts, 20), tdtk.KDtree(spts, 20), tdtk.KDtree(tpts, 20)
    assert deep.info()["max_depth"] >= 4 * Q_SD and shallow.info()["max_depth"] <= Q_SD - 1
    assert _bits_for(table.info()["n_points"]) + _bits_for(table.info()["max_leaf_points"]) > 30
    assert len(Qbig) > Q_MAX_BLOCKS * Q_BLOCK
    Qd = me.deep_queries(dpts, geo, 1_500, 81)
    qk, _ = me.table_queries(tpts, blob)
    npts = spts[:4_000]
    calls = {
        "deep3": lambda: deep.kNearestRangeSearchBatch(Qd, 3, ge.DEEP_FINITE_R2),
        "deep33": lambda: deep.kNearestRangeSearchBatch(Qd, 33, ge.DEEP_FINITE_R2),
        "deep64": lambda: deep.kNearestRangeSearchBatch(Qd, 64, 1e30),
        "shallow_small": lambda: shallow.kNearestRangeSearchBatch(Qbig[:7], 33, 9.0),
        "shallow_big": lambda: shallow.kNearestRangeSearchBatch(Qbig, 3, 36.0),
        "shallow_big64": lambda: shallow.kNearestRangeSearchBatch(Qbig, 64, 36.0),
        "table33": lambda: table.kNearestRangeSearchBatch(qk, 33, me.TABLE_R2[0]),
        "table3": lambda: table.kNearestRangeSearchBatch(qk, 3, 1e30),
        "normals": lambda: tdtk.calculateNormalsKNNRange(npts, 20, 9.0, me.RPOS, bucketSize=5, want_knn=True),
        "normals_lds": lambda: tdtk.calculateNormalsKNNRange(npts, 40, 9.0, me.RPOS, bucketSize=5, want_knn=True),
        "knn": lambda: shallow.kNearestNeighborsBatch(Qbig[:50_000], 10),
        "range": lambda: shallow.fixedRangeSearchBatch(Qbig[:50_000], 36.0),
        "clusters": lambda: shallow.clusters(4.0),
    }
    first = {name: f() for name, f in calls.items()}
    order = ["deep33", "shallow_small", "table33", "deep33", "table3", "deep3", "knn",
             "shallow_big", "shallow_small", "shallow_big64", "shallow_small", "range", "deep64",
             "normals", "deep3", "clusters", "normals_lds", "shallow_small", "normals", "table33", "deep64", "knn",
             "shallow_big", "range", "clusters", "normals_lds", "deep33"]
    assert set(order) == set(calls)
    for step, name in enumerate(order):
        got = calls[name]()
        assert len(got) == len(first[name])
        for a, b in zip(got, first[name]):
            if isinstance(a, np.ndarray):
                assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (step, name)
            else:
                assert a == b, (step, name)


# ---- 12. a tree never holds a non-finite point ---------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")], ids=["nan", "inf", "-inf"])
def test_non_finite_tree_points_are_refused_at_every_shape(tdtk, gpu, ge, bad):
    """knn_reg_body / knn_lds_body report "the first nr slots", nr the number of slots with d >= 0; the reference filters slot
    by slot.  The two agree only while a list never mixes NaN and finite distances -- while no tree holds a non-finite point.
    The host builder refuses such a cloud up front (kd_build.cpp); the device build noticed it only where a split left a
    side empty, so a cloud that never splits, or one +inf, got a tree.  Every entry point that builds a tree must refuse:
    TDTK_EINVAL, the caller's arrays untouched, the context usable afterwards."""
    L = tdtk.lib()
    rng = np.random.default_rng(1312)
    rp = np.zeros(3)
    good = rng.uniform(-1, 1, (500, 3))
    shapes = [(1, 20), (7, 20), (200, 1), (200, 5), (200, 20), (40_000, 20)]
    n = 0
    for M, b in shapes:
        base = rng.uniform(-1, 1, (M, 3))
        for axis in range(3):
            for at in sorted({0, (2 * M) // 3}):
                pts = base.copy()
                pts[at, axis] = bad
                tag = (M, b, axis, at)
                with pytest.raises(tdtk.TdtkError) as e:
                    tdtk.KDtree(pts, b)
                assert e.value.code == -1, tag
                sc = tdtk.Scan([0, 0, 0], [0, 0, 0], pts, bucketSize=b)
                with pytest.raises(tdtk.TdtkError) as e:
                    sc.getSearchTree()
                assert e.value.code == -1, tag
                nrm = np.full((M, 3), -7.0); knn = np.full((M, 6), -7, np.int32); cnt = np.full(M, -7, np.int32)
                assert L.tdtk_normals_knn(dp(pts), M, 3, dp(rp), b, 0, dp(nrm), ip(knn)) == -1, tag
                assert L.tdtk_normals_range(dp(pts), M, 1.0, dp(rp), b, 0, dp(nrm)) == -1, tag
                assert L.tdtk_normals_knn_range(dp(pts), M, 3, 1.0, dp(rp), b, 0, dp(nrm), ip(knn), ip(cnt)) == -1, tag
                assert L.tdtk_normals_adaptive_knn(dp(pts), M, 3, 5, dp(rp), b, 0, dp(nrm), ip(cnt), ip(knn)) == -1, tag
                assert (nrm == -7.0).all() and (knn == -7).all() and (cnt == -7).all(), tag
                n += 1
        # the next valid call on the context works
        kd = tdtk.KDtree(good, b)
        idx, d2, c = kd.kNearestRangeSearchBatch(good[:50], 5, 1e30)
        assert (c == 5).all() and np.array_equal(idx[:, 0], np.arange(50)) and kd.verify() == [0, 0, 0, 0]
        assert np.isfinite(tdtk.calculateNormalsKNNRange(good, 5, 1.0, rp, bucketSize=b)).any()
    print("non-finite %r: %d clouds x 6 entry points refused" % (bad, n))
    assert n == 3 * (1 + 2 * 5)
