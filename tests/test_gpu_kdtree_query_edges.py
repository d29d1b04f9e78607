"""The branches of query.hip that tests/test_gpu_kdtree_queries.py never executes: a lane's second and later grid-stride
trips in every kernel, the stack's HBM overflow in every kernel (a tree 80 levels deep), leaf table mode with leaves of
thousands of points, lists shorter than k in every list band, queries on split planes and at tie distances, non-finite
queries, the optional d2 output, and the order of calls on the context's shared workspaces.

Every comparison is exact.  Index lists are compared with the reference library where oracle/_ref travelled
(orc.have_ref()), else with the k9 fixture (tests/golden/make_golden_knn_edges.py) for the small cases and with brute
force (the k smallest distances as a sorted multiset, the set d2 < r2) for the large ones; normals with the oracle's PCA
on those lists.  Each test first asserts the precondition that makes it reach its branch."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
pytestmark = pytest.mark.gpu

# query.hip's launch geometry, restated: a lane takes a second query beyond Q_MAX_BLOCKS x block size queries
Q_MAX_BLOCKS, Q_BLOCK, Q_BLOCK_L, Q_SD = 2048, 128, 64, 16


def _me():
    spec = importlib.util.spec_from_file_location("make_golden_knn_edges", os.path.join(G, "make_golden_knn_edges.py"))
    me = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(me)
    return me


def _k9():
    return np.load(os.path.join(G, "k9_kdtree_query_edges.npz"))


def _all_d2(me, pts, q):
    return me.dist2(pts, np.broadcast_to(q, pts.shape), np.arange(len(pts)))


def _check_knn_lists(me, pts, Q, idx, d2, k):
    """d2 is Dist2 of the returned points, nondecreasing along each list, -1 / -1.0 beyond min(k, M)"""
    m = min(k, len(pts))
    assert idx.shape == (len(Q), k) and (idx[:, m:] == -1).all() and (d2[:, m:] == -1.0).all()
    assert (idx[:, :m] >= 0).all() and (idx[:, :m] < len(pts)).all()
    for s in range(0, len(Q), 100_000):
        e = min(s + 100_000, len(Q))
        want = me.dist2(pts, np.broadcast_to(Q[s:e, None, :], (e - s, m, 3)), idx[s:e, :m])
        assert np.array_equal(d2[s:e, :m], want)
    assert (np.diff(d2[:, :m], axis=1) >= 0).all()


def _check_range_lists(me, pts, Q, off, idx, d2, r2):
    cnt = np.diff(off.astype(np.int64))
    assert off[0] == 0 and off[-1] == len(idx) == len(d2) and (cnt >= 0).all()
    assert np.array_equal(d2, me.dist2(pts, np.repeat(Q, cnt, axis=0), idx)) and (d2 < r2).all()


def _knn_parity(me, t, pts, Q, rows, idx, d2, k):
    """rows of the batch against the reference tree t, or (t is None) against the k smallest of all distances"""
    rows = np.asarray(rows)
    if t is not None:
        assert np.array_equal(idx[rows], me.ref_knn(t, Q[rows], k)), k
    else:
        for i in rows:
            assert np.array_equal(d2[i, :min(k, len(pts))], np.sort(_all_d2(me, pts, Q[i]))[:k]), (k, i)


def _range_parity(me, t, pts, Q, rows, off, idx, r2):
    for i in rows:
        l = idx[int(off[i]):int(off[i + 1])]
        if t is not None:
            assert np.array_equal(l, t.range(Q[i], r2)), i
        else:
            assert len(set(l.tolist())) == len(l)
            assert set(l.tolist()) == set(np.nonzero(_all_d2(me, pts, Q[i]) < r2)[0].tolist()), i


def _range_lengths(off, idx, cnt):
    """the lists have the lengths the reference's had and no entry twice (with _check_range_lists: every entry within r2)"""
    assert np.array_equal(np.diff(off.astype(np.int64)), cnt.astype(np.int64))
    for i in range(len(off) - 1):
        l = idx[int(off[i]):int(off[i + 1])]
        assert len(np.unique(l)) == len(l), i


def _pca_of_lists(orc, pts, Q, off, idx, rpos):
    """calculateNormal of the oracle on each CSR list, one call per list with the query in front of its points (a list
    here may hold the 40,000 copies: nothing quadratic in its length)"""
    rp = np.ascontiguousarray(rpos, np.float64)
    nrm = np.empty((len(Q), 3))
    dp = C.POINTER(C.c_double)
    for i in range(len(Q)):
        l = idx[int(off[i]):int(off[i + 1])]
        xyz = np.ascontiguousarray(np.vstack([Q[i].reshape(1, 3), pts[l]]), np.float64)
        lst = np.arange(1, len(l) + 1, dtype=np.int32)
        one = np.empty(3)
        orc.lib().orc_normals_from_knn(xyz.ctypes.data_as(dp), 1, len(l), lst.ctypes.data_as(C.POINTER(C.c_int32)),
                                       rp.ctypes.data_as(dp), one.ctypes.data_as(dp))
        nrm[i] = one
    return nrm


def _bits_for(v):
    return int(v).bit_length()


# ---- 1. every kernel past its first grid-stride trip ---------------------------------------------------------------
def test_knn_lists_beyond_one_query_per_lane(tdtk, orc, gpu):
    """k_knn_reg<4>, k_knn_reg<32> and k_knn_lds with 600,000 queries: more than twice the 262,144 lanes of the capped
    grid, so most sorted positions are a lane's second or later query (k = 10, 20: test_knn_1m_against_reference)"""
    me = _me()
    pts, Q = me.trips_cloud()
    K = len(Q)
    assert K > 2 * Q_MAX_BLOCKS * Q_BLOCK and K > 2 * Q_MAX_BLOCKS * Q_BLOCK_L
    kd = tdtk.KDtree(pts, 20)
    rng = np.random.default_rng(11)
    t = me.RefTree(pts, 20) if orc.have_ref() else None
    sub = rng.choice(K, 20_000 if t is not None else 2_000, replace=False)
    shuffle = rng.permutation(K)
    for k in (3, 32, 33, 64):
        idx, d2 = kd.kNearestNeighborsBatch(Q, k)
        _check_knn_lists(me, pts, Q, idx, d2, k)
        _knn_parity(me, t, pts, Q, sub, idx, d2, k)
        # batch invariance: 50,000 queries alone are one trip per lane in every kernel
        assert 50_000 < Q_MAX_BLOCKS * Q_BLOCK_L
        for s in (0, 275_000, 550_000):
            i1, d1 = kd.kNearestNeighborsBatch(Q[s:s + 50_000], k)
            assert np.array_equal(i1, idx[s:s + 50_000]) and np.array_equal(d1, d2[s:s + 50_000]), (k, s)
        i2, dd2 = kd.kNearestNeighborsBatch(Q[shuffle], k)
        assert np.array_equal(i2, idx[shuffle]) and np.array_equal(dd2, d2[shuffle]), k


def test_normals_beyond_one_point_per_lane(tdtk, orc, gpu):
    """every NORMALS kernel and k_range_normals on 600,000 points (uniform + dense blobs)"""
    me = _me()
    pts, blob = me.trips_normals_cloud()
    n = len(pts)
    assert n > 2 * Q_MAX_BLOCKS * Q_BLOCK
    kd = tdtk.KDtree(pts, 20)
    rng = np.random.default_rng(12)
    t = me.RefTree(pts, 20) if orc.have_ref() else None
    sub = np.concatenate([rng.choice(n, 2_800, replace=False), rng.choice(blob, 200, replace=False)])
    chk = sub if t is not None else sub[::10]             # (brute force: 600,000 distances per row)
    r2 = None
    for k in (3, 10, 20, 32, 33, 64):
        nrm, knn = tdtk.calculateNormalsKNN(pts, k, me.RPOS, bucketSize=20, want_knn=True)
        idx, d2 = kd.kNearestNeighborsBatch(pts, k)
        assert np.array_equal(knn, idx), k
        _check_knn_lists(me, pts, pts, idx, d2, k)
        _knn_parity(me, t, pts, pts, chk, idx, d2, k)
        assert np.array_equal(nrm, orc.normals_from_knn(pts, knn, me.RPOS)), k
        if k == 20:
            r2 = float(np.median(d2[:, 19]))              # ~20 neighbours per uniform point, 2,500 per blob point
    nr = tdtk.calculateNormalsRange(pts, r2, me.RPOS, bucketSize=20)
    off, idx, d2 = kd.fixedRangeSearchBatch(pts[sub], r2)
    _check_range_lists(me, pts, pts[sub], off, idx, d2, r2)
    assert np.diff(off.astype(np.int64))[-200:].min() >= 2_500
    _range_parity(me, t, pts, pts[sub], range(len(sub)) if t is not None else range(0, len(sub), 10), off, idx, r2)
    assert np.array_equal(nr[sub], _pca_of_lists(orc, pts, pts[sub], off, idx, me.RPOS), equal_nan=True)


# ---- 2. deep trees: the overflow stack in every kernel ---------------------------------------------------------------
def test_deep_tree_every_kernel_on_the_overflow_stack(tdtk, orc, gpu):
    """20,000 points on geometrically growing radii among 280,000 uniform ones: the oracle's tree is 84 / 80 levels deep
    at bucket 1 / 20 (measured on the CPU), five times the stack's LDS levels.  The k-NN walk pushes the far child of
    every internal node, so every query of the geometric part lives in the overflow area."""
    me, z = _me(), _k9()
    pts, geo = me.deep_cloud()
    have = orc.have_ref()
    shallow_pts = np.random.default_rng(21).uniform(-5, 5, (5_000, 3))
    # The device answers all 2,400 queries for every k; the reference library answers every ref_stride[k]-th of them (Q is
    # laid out part by part, so a stride keeps the third that lies in the geometric part).  Far out in the geometric part
    # its walk prunes next to nothing: 33 to 53 ms per query at k = 64 on this cloud (measured on the CPU), 0.03 ms at k = 3.
    ref_stride = {3: 1, 10: 4, 20: 4, 32: 8, 33: 8, 64: 8} if have else dict.fromkeys(me.BAND_KS, 1)
    for b in (1, 20):
        kd = tdtk.KDtree(pts, b)
        info = kd.info()
        print("deep cloud, bucket %d: max_depth %d, max_leaf_points %d" % (b, info["max_depth"], info["max_leaf_points"]))
        assert info["max_depth"] >= 4 * Q_SD
        assert kd.verify() == [0, 0, 0, 0]
        Q, range_qs = me.deep_range_queries(pts, geo, 2_400 if have else me.DEEP_FALLBACK_Q, b)
        ng = len(Q) // 3
        assert 4 * ng >= len(Q) and (np.abs(Q[:ng]).max(1) > 50).sum() > ng // 2     # the geometric part, mostly far out
        t = me.RefTree(pts, b) if have else None
        first = {}
        for k in me.BAND_KS:
            idx, d2 = kd.kNearestNeighborsBatch(Q, k)
            _check_knn_lists(me, pts, Q, idx, d2, k)
            _knn_parity(me, t, pts, Q, range(0, len(Q), ref_stride[k]), idx, d2, k)
            first[k] = (idx, d2)
        # r2 = 9: about 29 entries per uniform query; r2 = 400 on a fifth of the queries: the lists of the inner queries
        # run through the 600 geometric points of radius < 20 around the origin.  Brute force cannot stand in for the
        # reference here: far out its box test (|q - c| - h on numbers of 1e80) rounds by more than the radius and prunes
        # the leaf of the query's own point -- 47 of 100 own-point queries of the geometric part return nothing at
        # bucket 1.  Without the library: the lengths it returned (k9), every entry within r2, none twice.
        for j, (q, r2) in enumerate(zip(range_qs, me.DEEP_R2)):
            off, idx, d2 = kd.fixedRangeSearchBatch(q, r2)
            _check_range_lists(me, pts, q, off, idx, d2, r2)
            if have:
                _range_parity(me, t, pts, q, range(len(q)), off, idx, r2)
            else:
                _range_lengths(off, idx, z["deep_b%d_r%d_cnt" % (b, j)])
        # a shallow tree in between (no overflow area asked for), then the same bytes again
        sh = tdtk.KDtree(shallow_pts, 20)
        assert sh.info()["max_depth"] <= Q_SD - 1
        sh.kNearestNeighborsBatch(shallow_pts, 33)
        sh.fixedRangeSearchBatch(shallow_pts, 0.25)
        for k in (3, 64):
            idx, d2 = kd.kNearestNeighborsBatch(Q, k)
            assert np.array_equal(idx, first[k][0]) and np.array_equal(d2, first[k][1]), (b, k)


def test_deep_tree_normals_overflow_and_capped_grid_together(tdtk, orc, gpu):
    """calculateNormalsKNN / calculateNormalsRange on the whole deep cloud: 300,000 queries are more than the 262,144
    lanes of the capped grid, every lane's column of the overflow area is used by more than one query"""
    me, z = _me(), _k9()
    pts, geo = me.deep_cloud()
    n = len(pts)
    assert n > Q_MAX_BLOCKS * Q_BLOCK
    kd = tdtk.KDtree(pts, 20)
    assert kd.info()["max_depth"] >= 4 * Q_SD and kd.verify() == [0, 0, 0, 0]
    t = me.RefTree(pts, 20) if orc.have_ref() else None
    sub, range_sub = me.deep_normals_samples(pts, geo)          # (k-NN rows: 100 + 300, see ref_stride above)
    for k in me.BAND_KS:
        nrm, knn = tdtk.calculateNormalsKNN(pts, k, me.RPOS, bucketSize=20, want_knn=True)
        idx, d2 = kd.kNearestNeighborsBatch(pts, k)
        assert np.array_equal(knn, idx), k
        _check_knn_lists(me, pts, pts, idx, d2, k)
        _knn_parity(me, t, pts, pts, sub if t is not None else sub[::10], idx, d2, k)
        assert np.array_equal(nrm, orc.normals_from_knn(pts, knn, me.RPOS), equal_nan=True), k
    r2 = me.DEEP_R2[0]
    nr = tdtk.calculateNormalsRange(pts, r2, me.RPOS, bucketSize=20)
    sub = range_sub
    off, idx, d2 = kd.fixedRangeSearchBatch(pts[sub], r2)
    _check_range_lists(me, pts, pts[sub], off, idx, d2, r2)
    if t is not None:
        _range_parity(me, t, pts, pts[sub], range(0, len(sub), 3), off, idx, r2)
    else:
        _range_lengths(off, idx, z["deep_normals_cnt"])
    # (a far geometric point finds itself alone, zero covariance, or -- see the lists' test -- nothing: 0 / 0 as the reference's)
    assert np.array_equal(nr[sub], _pca_of_lists(orc, pts, pts[sub], off, idx, me.RPOS), equal_nan=True)


# ---- 3. table-mode leaves and one-leaf clusters ---------------------------------------------------------------------
# (Out of scope here: a range result of more than 2^32 entries, what the 64-bit offsets are for.  The C interface returns
# into host arrays, so that needs more than 16 GiB twice over.)
def test_table_mode_leaves_of_thousands_of_points(tdtk, orc, gpu):
    me, z = _me(), _k9()
    pts, copies, blob = me.table_cloud()
    kd = tdtk.KDtree(pts, 20)
    info = kd.info()
    print("table cloud: n %d, max_leaf_points %d, max_depth %d" % (info["n_points"], info["max_leaf_points"], info["max_depth"]))
    # kd_build.cpp's packing rule: (start << cb) | count must fit in 30 bits, else the leaves go through leaf_tab
    assert _bits_for(info["n_points"]) + _bits_for(info["max_leaf_points"]) > 30
    assert info["max_leaf_points"] >= me.TABLE_COPIES
    assert kd.verify() == [0, 0, 0, 0]
    qk, qrs = me.table_queries(pts, blob)
    t = me.RefTree(pts, 20) if orc.have_ref() else None
    # with 40,000 equal distances the list is "the first k in visiting order": only the reference (or its recorded
    # rows) can pin that
    for k in me.BAND_KS:
        idx, d2 = kd.kNearestNeighborsBatch(qk, k)
        _check_knn_lists(me, pts, qk, idx, d2, k)
        assert np.array_equal(idx, me.ref_knn(t, qk, k) if t is not None else z["table_knn%d" % k]), k
    big = 0
    for j, (q, r2) in enumerate(zip(qrs, me.TABLE_R2)):
        off, idx, d2 = kd.fixedRangeSearchBatch(q, r2)
        _check_range_lists(me, pts, q, off, idx, d2, r2)
        if t is not None:
            woff, widx = me.ref_range(t, q, r2)
        else:
            woff, widx = me.restore_run(z["table_r%d_soff" % j], z["table_r%d_sidx" % j], z["table_r%d_pos" % j], z["table_big"])
            assert np.array_equal(woff, z["table_r%d_off" % j])
        assert np.array_equal(off, woff) and np.array_equal(idx, widx), j
        big += int((np.diff(off.astype(np.int64)) >= me.TABLE_COPIES).sum())
    assert 16 <= big <= 48                      # the lists that run through the leaf of copies
    for k in (10, 33):
        nrm, knn = tdtk.calculateNormalsKNN(pts, k, me.RPOS, bucketSize=20, want_knn=True)
        assert np.array_equal(knn, kd.kNearestNeighborsBatch(pts, k)[0]), k
        assert np.array_equal(nrm, orc.normals_from_knn(pts, knn, me.RPOS), equal_nan=True), k   # copies: zero covariance
    r2 = me.TABLE_R2[0]
    nr = tdtk.calculateNormalsRange(pts, r2, me.RPOS, bucketSize=20)
    rng = np.random.default_rng(31)
    sub = np.concatenate([rng.choice(copies, 20, replace=False), rng.choice(blob, 100, replace=False),
                          rng.choice(len(pts), 180, replace=False)])
    off, idx, d2 = kd.fixedRangeSearchBatch(pts[sub], r2)
    _check_range_lists(me, pts, pts[sub], off, idx, d2, r2)
    _range_parity(me, t, pts, pts[sub], range(len(sub)), off, idx, r2)
    assert np.array_equal(nr[sub], _pca_of_lists(orc, pts, pts[sub], off, idx, me.RPOS), equal_nan=True)


# ---- 4. short lists in every band -------------------------------------------------------------------------------------
def test_fewer_points_than_slots_in_every_band(tdtk, orc, gpu):
    """M points, k slots, M around k: the -0.0 front slots of a register list together with unset slots behind the
    entries (KC = 4, 10, 20, 32), the LDS list below its k, nr < k in the normals"""
    me, z = _me(), _k9()
    rows = me.short_rows(z["short_knn"])
    have = orc.have_ref()
    for M in me.SHORT_MS:
        pts, Q = me.short_cloud(M)
        for b in me.SHORT_BUCKETS:
            kd = tdtk.KDtree(pts, b)
            assert kd.verify() == [0, 0, 0, 0]
            t = me.RefTree(pts, b) if have else None
            for k in me.SHORT_KS:
                m = min(k, M)
                idx, d2 = kd.kNearestNeighborsBatch(Q, k)
                _check_knn_lists(me, pts, Q, idx, d2, k)
                assert np.array_equal(idx, me.ref_knn(t, Q, k) if have else rows[(M, b, k)]), (M, b, k)
                nrm, knn = tdtk.calculateNormalsKNN(pts, k, me.RPOS, bucketSize=b, want_knn=True)
                assert knn.shape == (M, k) and (knn[:, m:] == -1).all() and (knn[:, :m] >= 0).all()
                assert np.array_equal(knn, kd.kNearestNeighborsBatch(pts, k)[0]), (M, b, k)
                # (fewer than three points: degenerate neighbourhoods)
                assert np.array_equal(nrm, orc.normals_from_knn(pts, np.ascontiguousarray(knn[:, :m]), me.RPOS),
                                      equal_nan=True), (M, b, k)


# ---- 5. split planes and exact ties ---------------------------------------------------------------------------------
def test_queries_on_split_planes_and_at_tie_distances(tdtk, orc, gpu):
    """the k-NN walk descends by q < splitval, the range walk by splitval - q >= 0, the range list leaves d2 == r2 out:
    2,000 queries on the integers and half-integers around the lattice 16^3, whose split values are such numbers"""
    me, z = _me(), _k9()
    pts, Q = me.lattice_cloud()
    have = orc.have_ref()
    S = me.LATTICE_STORED
    D = np.stack([_all_d2(me, pts, q) for q in Q])                 # [2000][4096], exact
    Ds = np.sort(D, axis=1)[:, :max(me.BAND_KS)]
    for r2 in me.LATTICE_R2:
        assert (D == r2).any() and (D < r2).any()
    for jb, b in enumerate(me.LATTICE_BUCKETS):
        kd = tdtk.KDtree(pts, b)
        assert kd.verify() == [0, 0, 0, 0]
        t = me.RefTree(pts, b) if have else None
        for k in me.BAND_KS:
            idx, d2 = kd.kNearestNeighborsBatch(Q, k)
            _check_knn_lists(me, pts, Q, idx, d2, k)
            assert np.array_equal(d2, Ds[:, :k]), (b, k)
            if have:
                assert np.array_equal(idx, me.ref_knn(t, Q, k)), (b, k)
            assert np.array_equal(idx[:S], me.lattice_unpack_knn(Q[:S], z["lattice_knn%d" % k])[jb]), (b, k)
        for j, r2 in enumerate(me.LATTICE_R2):
            off, idx, d2 = kd.fixedRangeSearchBatch(Q, r2)
            _check_range_lists(me, pts, Q, off, idx, d2, r2)
            assert np.array_equal(np.diff(off.astype(np.int64)), (D < r2).sum(1)), (b, r2)
            _range_parity(me, t, pts, Q, range(len(Q)), off, idx, r2)
            woff = z["lattice_b%d_r%d_off" % (b, j)].astype(np.uint64)
            assert np.array_equal(off[:S + 1], woff), (b, r2)
            assert np.array_equal(idx[:int(off[S])], me.lattice_unpack_range(Q[:S], woff, z["lattice_b%d_r%d_idx" % (b, j)])), (b, r2)


# ---- 6. far and non-finite queries ------------------------------------------------------------------------------------
def test_far_and_non_finite_queries(tdtk, orc, gpu):
    """What the reference library returned for these (live where oracle/_ref exists, else as recorded in k9; the
    expectation spelled out below held on the build the fixture was made with): a NaN coordinate gives an empty k-NN
    list and an empty range list, +-inf / 1e160 / -1e200 give k points at distance inf and an empty range list.  The
    ordinary queries of the batch are not disturbed."""
    me, z = _me(), _k9()
    pts, Q, i_ord, i_nan, i_far = me.nonfinite_cloud()
    assert len(pts) <= 100_000 and len(i_nan) + len(i_far) <= 64 and len(i_ord) + len(i_nan) + len(i_far) == len(Q)
    kd = tdtk.KDtree(pts, 20)
    t = me.RefTree(pts, 20) if orc.have_ref() else None
    with np.errstate(invalid="ignore", over="ignore"):
        for k in me.BAND_KS:
            want = me.ref_knn(t, Q, k) if t is not None else z["nonfinite_knn%d" % k]
            assert (want[i_nan] == -1).all() and (want[i_far] >= 0).all() and (want[i_ord] >= 0).all()
            idx, d2 = kd.kNearestNeighborsBatch(Q, k)
            assert np.array_equal(idx, want), k
            assert (d2[i_nan] == -1.0).all() and (d2[i_far] == np.inf).all()
            assert np.array_equal(d2, me.dist2(pts, np.broadcast_to(Q[:, None, :], idx.shape + (3,)), idx))
            io, do = kd.kNearestNeighborsBatch(Q[i_ord], k)
            assert np.array_equal(io, idx[i_ord]) and np.array_equal(do, d2[i_ord]), k
        r2 = me.NONFINITE_R2
        woff, widx = me.ref_range(t, Q, r2) if t is not None else (z["nonfinite_roff"], z["nonfinite_ridx"])
        cnt = np.diff(woff.astype(np.int64))
        assert (cnt[i_nan] == 0).all() and (cnt[i_far] == 0).all() and cnt[i_ord].sum() > 0
        off, idx, d2 = kd.fixedRangeSearchBatch(Q, r2)
        assert np.array_equal(off, woff) and np.array_equal(idx, widx)
        _check_range_lists(me, pts, Q, off, idx, d2, r2)
        nq = Q[np.concatenate([i_nan, i_far])]
        off, idx, _ = kd.fixedRangeSearchBatch(nq, r2)                 # nothing but such queries: total 0
        assert off.tolist() == [0] * (len(nq) + 1) and len(idx) == 0


# ---- 7. optional outputs and single-query wrappers ----------------------------------------------------------------------
def test_d2_null_and_single_query_wrappers(tdtk, gpu):
    L = tdtk.lib()
    rng = np.random.default_rng(71)
    pts = rng.uniform(-10, 10, (30_000, 3))
    pts[500:520] = pts[0:20]
    Q = np.ascontiguousarray(np.vstack([pts[:300], rng.uniform(-12, 12, (300, 3))]))
    kd = tdtk.KDtree(pts, 20)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    for k in (3, 10, 20, 32, 33, 64):
        idx, _ = kd.kNearestNeighborsBatch(Q, k)
        got = np.full((len(Q), k), -7, np.int32)
        assert L.tdtk_knn_search(kd._h, dp(Q), len(Q), k, ip(got), None) == 0
        assert np.array_equal(got, idx), k
        for i in (0, 5, 299, 300, 599):
            assert kd.kNearestNeighbors(Q[i], k) == idx[i].tolist(), (k, i)
    r2 = 1.5
    off, idx, _ = kd.fixedRangeSearchBatch(Q, r2)
    assert len(idx) > len(Q)
    o2 = np.zeros(len(Q) + 1, np.uint64)
    got = np.full(len(idx), -7, np.int32)
    tot = C.c_uint64(0)
    assert L.tdtk_fixed_range_search(kd._h, dp(Q), len(Q), r2, up(o2), ip(got), None, len(got), C.byref(tot)) == 0
    assert tot.value == len(idx) and np.array_equal(o2, off) and np.array_equal(got, idx)
    for i in (0, 5, 299, 300, 599):
        assert kd.fixedRangeSearch(Q[i], r2) == idx[int(off[i]):int(off[i + 1])].tolist(), i
    # a tree smaller than k: the single-query list is the trimmed batch row
    few = rng.uniform(-1, 1, (5, 3))
    kf = tdtk.KDtree(few, 20)
    for k in (4, 10, 32, 64):
        row = kf.kNearestNeighborsBatch(few[:1], k)[0][0]
        assert (row[:min(k, 5)] >= 0).all() and (row[5:] == -1).all()
        assert kf.kNearestNeighbors(few[0], k) == row[:min(k, 5)].tolist(), k
    assert sorted(kf.fixedRangeSearch(few[0], 100.0)) == [0, 1, 2, 3, 4] and kf.fixedRangeSearch([50.0, 0.0, 0.0], 1.0) == []


# ---- 8. call order ----------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_calls_before_them(tdtk, gpu):
    """every call shares the context's workspaces (the overflow area is not asked for by a shallow tree, the others grow by
    free-and-reallocate): each call below gives what the same call gave first, whatever ran in between"""
    me = _me()
    dpts, geo = me.deep_cloud()
    tpts, _, blob = me.table_cloud()
    spts, Qbig = me.trips_cloud()
    spts = spts[:20_000]
    deep, shallow, table = tdtk.KDtree(dpts, 20), tdtk.KDtree(spts, 20), tdtk.KDtree(tpts, 20)
    assert deep.info()["max_depth"] >= 4 * Q_SD and shallow.info()["max_depth"] <= Q_SD - 1
    assert _bits_for(table.info()["n_points"]) + _bits_for(table.info()["max_leaf_points"]) > 30
    assert len(Qbig) > 2 * Q_MAX_BLOCKS * Q_BLOCK
    Qd = me.deep_queries(dpts, geo, 3_000, 81)
    _, (qr0, _) = me.table_queries(tpts, blob)
    npts = spts[:4_000]
    nowhere = Qbig[:1_000] + 1e4
    calls = {
        "deep33": lambda: deep.kNearestNeighborsBatch(Qd, 33),
        "deep3": lambda: deep.kNearestNeighborsBatch(Qd, 3),
        "deep_range": lambda: deep.fixedRangeSearchBatch(Qd, 9.0),
        "shallow_small": lambda: shallow.kNearestNeighborsBatch(Qbig[:7], 10),
        "shallow_big": lambda: shallow.kNearestNeighborsBatch(Qbig, 10),
        "shallow_big64": lambda: shallow.kNearestNeighborsBatch(Qbig, 64),
        "table_range": lambda: table.fixedRangeSearchBatch(qr0, me.TABLE_R2[0]),
        "table20": lambda: table.kNearestNeighborsBatch(qr0, 20),
        "range_millions": lambda: shallow.fixedRangeSearchBatch(Qbig, 36.0),
        "range_nothing": lambda: shallow.fixedRangeSearchBatch(nowhere, 1.0),
        "normals": lambda: tdtk.calculateNormalsKNN(npts, 20, me.RPOS, bucketSize=5, want_knn=True),
    }
    first = {name: f() for name, f in calls.items()}
    assert int(first["range_millions"][0][-1]) > 2_000_000 and int(first["range_nothing"][0][-1]) == 0
    order = ["deep33", "shallow_small", "table_range", "deep33", "table20", "deep3",           # deep / shallow / table
             "shallow_big", "shallow_small", "shallow_big", "shallow_big64", "shallow_small",    # 600,000 / 7 / 600,000
             "range_millions", "range_nothing", "table_range", "range_nothing", "deep_range",   # total 0 after millions
             "deep3", "normals", "deep3", "shallow_small", "normals", "shallow_big64", "deep33"]
    assert set(order) == set(calls)
    for step, name in enumerate(order):
        got = calls[name]()
        assert len(got) == len(first[name])
        for a, b in zip(got, first[name]):
            assert a.dtype == b.dtype and np.array_equal(a, b), (step, name)
