"""k-NN and fixed-radius search on the device kd-tree and the KNN / range normals built on them (query.hip): the GPU tier.
Lists equal KDtreeIndexed::kNearestNeighbors / fixedRangeSearch of the reference's compiled code (live where oracle/_ref
travelled, else the k8 fixture and brute force), normals equal calculateNormal's PCA on those lists, bit for bit."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
pytestmark = pytest.mark.gpu


def _mg():
    spec = importlib.util.spec_from_file_location("make_golden_knn", os.path.join(G, "make_golden_knn.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    return mg


def _check_knn_lists(mg, pts, Q, idx, d2, k):
    """d2 is Dist2 of the returned points, nondecreasing along each list, -1 / -1.0 beyond min(k, M)"""
    m = min(k, len(pts))
    assert idx.shape == (len(Q), k) and (idx[:, m:] == -1).all() and (d2[:, m:] == -1.0).all()
    assert (idx[:, :m] >= 0).all() and (idx[:, :m] < len(pts)).all()
    for s in range(0, len(Q), 100_000):
        e = min(s + 100_000, len(Q))
        want = mg.dist2(pts, np.broadcast_to(Q[s:e, None, :], (e - s, m, 3)), idx[s:e, :m])
        assert np.array_equal(d2[s:e, :m], want)
    assert (np.diff(d2[:, :m], axis=1) >= 0).all()


def test_fixture_parity_knn_range_and_normals(tdtk, gpu):
    mg = _mg()
    z = np.load(os.path.join(G, "k8_kdtree_queries.npz"))
    for name in mg.k8_clouds():
        pts, Q, no, r2 = z[name + "_pts"], z[name + "_q"], int(z[name + "_own"][0]), float(z[name + "_r2"][0])
        for b in mg.BUCKETS:
            kd = tdtk.KDtree(pts, b)
            for k in mg.KS:
                idx, d2 = kd.kNearestNeighborsBatch(Q, k)
                want = z["%s_b%d_knn%d" % (name, b, k)]
                assert np.array_equal(idx, want), (name, b, k)
                assert np.array_equal(d2, mg.dist2(pts, np.broadcast_to(Q[:, None, :], want.shape + (3,)), want)), (name, b, k)
            off, ridx, rd2 = kd.fixedRangeSearchBatch(Q, r2)
            assert np.array_equal(off, z["%s_b%d_roff" % (name, b)]), (name, b)
            assert np.array_equal(ridx, z["%s_b%d_ridx" % (name, b)]), (name, b)
            qrep = np.repeat(Q, np.diff(off.astype(np.int64)), axis=0)
            assert np.array_equal(rd2, mg.dist2(pts, qrep, ridx))
            # the normals of the whole cloud; the fixture has those of its own-point queries
            own = np.array([int(np.nonzero((pts == q).all(1))[0][0]) for q in Q[:no]])
            for k in mg.NORMAL_KS:
                nrm, knn = tdtk.calculateNormalsKNN(pts, k, mg.RPOS, bucketSize=b, want_knn=True)
                lists, _ = kd.kNearestNeighborsBatch(pts, k)
                assert np.array_equal(knn, lists), (name, b, k)
                # (a point's list depends on its coordinates only: a duplicate's row is its twin's)
                assert np.array_equal(knn[own], z["%s_b%d_knn%d" % (name, b, k)][:no]), (name, b, k)
                assert np.array_equal(nrm[own], z["%s_b%d_nknn%d" % (name, b, k)]), (name, b, k)
            nr = tdtk.calculateNormalsRange(pts, r2, mg.RPOS, bucketSize=b)
            assert np.array_equal(nr[own], z["%s_b%d_nrange" % (name, b)]), (name, b)


def test_knn_1m_against_reference(tdtk, orc, gpu):
    mg = _mg()
    rng = np.random.default_rng(1001)
    pts = rng.uniform(-50, 50, (1_000_000, 3))
    kd = tdtk.KDtree(pts, 20)
    sub = rng.choice(len(pts), 20_000 if orc.have_ref() else 2_000, replace=False)
    t = mg.RefTree(pts, 20) if orc.have_ref() else None
    for k in (10, 20):
        idx, d2 = kd.kNearestNeighborsBatch(pts, k)
        _check_knn_lists(mg, pts, pts, idx, d2, k)
        if t is not None:
            assert np.array_equal(idx[sub], mg.ref_knn(t, pts[sub], k)), k
        else:
            for i in sub:
                all_d = mg.dist2(pts, np.broadcast_to(pts[i], pts.shape), np.arange(len(pts)))
                assert np.array_equal(d2[i], np.sort(all_d)[:k])


def test_range_1m_against_reference_and_capacity_retry(tdtk, orc, gpu):
    mg = _mg()
    rng = np.random.default_rng(1002)
    pts = rng.uniform(-50, 50, (1_000_000, 3))
    r2 = (20.0 * 1e6 / len(pts) * 3 / (4 * np.pi)) ** (2.0 / 3.0)     # ~20 neighbours per query
    kd = tdtk.KDtree(pts, 20)
    off, idx, d2 = kd.fixedRangeSearchBatch(pts, r2)
    cnt = np.diff(off.astype(np.int64))
    assert 15 < cnt.mean() < 25 and (cnt >= 1).all()
    assert np.array_equal(d2, mg.dist2(pts, np.repeat(pts, cnt, axis=0), idx)) and (d2 < r2).all()
    sub = rng.choice(len(pts), 20_000 if orc.have_ref() else 2_000, replace=False)
    if orc.have_ref():
        t = mg.RefTree(pts, 20)
        for i in sub:
            assert np.array_equal(idx[off[i]:off[i + 1]], t.range(pts[i], r2)), i
    else:
        for i in sub:
            all_d = mg.dist2(pts, np.broadcast_to(pts[i], pts.shape), np.arange(len(pts)))
            assert set(idx[off[i]:off[i + 1]].tolist()) == set(np.nonzero(all_d < r2)[0].tolist())
    # capacity too small: TDTK_EINVAL, offsets and total filled, nothing else written; the retry gives the same lists
    L = tdtk.lib()
    q = pts[:50_000]
    o1 = np.zeros(len(q) + 1, np.uint64)
    tot = C.c_uint64(0)
    small = np.full(10, -7, np.int32)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    rc = L.tdtk_fixed_range_search(kd._h, dp(np.ascontiguousarray(q)), len(q), r2, up(o1), ip(small), None, 10, C.byref(tot))
    assert rc == -1 and (small == -7).all()
    assert tot.value == int(off[len(q)]) and np.array_equal(o1, off[:len(q) + 1])
    big = np.empty(tot.value, np.int32)
    rc = L.tdtk_fixed_range_search(kd._h, dp(np.ascontiguousarray(q)), len(q), r2, up(o1), ip(big), None, tot.value, C.byref(tot))
    assert rc == 0 and np.array_equal(big, idx[:tot.value])


def test_trees_from_scans_count_through_the_concatenation(tdtk, gpu):
    rng = np.random.default_rng(1003)
    a = rng.uniform(-10, 10, (30_000, 3))
    b = rng.uniform(-10, 10, (20_000, 3)) + [3.0, 0.0, 0.0]
    q = rng.uniform(-12, 12, (5_000, 3))
    sa = tdtk.Scan([0, 0, 0], [0, 0, 0], a)
    sb = tdtk.Scan([0, 0, 0], [0, 0, 0], b)

    def current(sc):
        xyz = np.empty((sc.n, 3)); nrm = np.empty((sc.n, 3))
        tdtk.lib().tdtk_scan_download(sc.handle, xyz.ctypes.data_as(C.POINTER(C.c_double)),
                                      nrm.ctypes.data_as(C.POINTER(C.c_double)))
        return xyz

    for trees, pts in ((sa.getSearchTree(), current(sa)),
                       (tdtk.MetaScan([sa, sb]).getSearchTree(), np.vstack([current(sa), current(sb)]))):
        ref = tdtk.KDtree(pts, 20)
        for k in (1, 10, 20):
            assert np.array_equal(trees.kNearestNeighborsBatch(q, k)[0], ref.kNearestNeighborsBatch(q, k)[0])
        o1, i1, _ = trees.fixedRangeSearchBatch(q, 0.5)
        o2, i2, _ = ref.fixedRangeSearchBatch(q, 0.5)
        assert np.array_equal(o1, o2) and np.array_equal(i1, i2)


def test_normals_on_the_dat_scan_equal_the_pca_of_the_reference_lists(tdtk, orc, gpu):
    mg = _mg()
    z = np.load(os.path.join(G, "dat_scans.npz"))
    pts = np.vstack([z["scan001"], [[9000.0, 9000.0, 9000.0]]])   # + an isolated point: a range list of one, zero covariance
    rpos = z["pose001"][:3]
    kd = tdtk.KDtree(pts, 20)
    for k in (10, 20):
        nrm, knn = tdtk.calculateNormalsKNN(pts, k, rpos, bucketSize=20, want_knn=True)
        if orc.have_ref():
            sub = np.random.default_rng(5).choice(len(pts), 3000, replace=False)
            assert np.array_equal(knn[sub], mg.ref_knn(mg.RefTree(pts, 20), pts[sub], k))
        assert np.array_equal(knn, kd.kNearestNeighborsBatch(pts, k)[0])
        assert np.array_equal(nrm, orc.normals_from_knn(pts, knn, rpos)), k
    r2 = float(np.median(kd.kNearestNeighborsBatch(pts, 20)[1][:, 19]))      # ~20 neighbours per point
    nr = tdtk.calculateNormalsRange(pts, r2, rpos, bucketSize=20)
    off, idx, _ = kd.fixedRangeSearchBatch(pts, r2)
    assert off[-1] - off[-2] == 1 and idx[-1] == len(pts) - 1
    sub = np.concatenate([np.random.default_rng(6).choice(len(pts) - 1, 1500, replace=False), [len(pts) - 1]])
    if orc.have_ref():
        t = mg.RefTree(pts, 20)
        for i in sub[:300]:
            assert np.array_equal(idx[off[i]:off[i + 1]], t.range(pts[i], r2))
    want = mg.range_normals(orc, pts, pts[sub], np.concatenate([[0], np.cumsum([off[i + 1] - off[i] for i in sub])]).astype(np.uint64),
                            np.concatenate([idx[off[i]:off[i + 1]] for i in sub]), rpos)
    assert np.array_equal(nr[sub], want, equal_nan=True)


def test_errors(tdtk, gpu):
    L = tdtk.lib()
    pts = np.random.default_rng(9).uniform(-1, 1, (1000, 3))
    kd = tdtk.KDtree(pts, 20)
    with pytest.raises(tdtk.TdtkError) as e:
        kd.kNearestNeighborsBatch(pts[:10], 0)
    assert e.value.code == -1
    with pytest.raises(tdtk.TdtkError) as e:
        kd.kNearestNeighborsBatch(pts[:10], 65)
    assert e.value.code == -5 and "64" in str(e.value)
    idx, _ = kd.kNearestNeighborsBatch(pts[:10], 64)
    assert (idx >= 0).all()
    with pytest.raises(tdtk.TdtkError) as e:
        tdtk.calculateNormalsKNN(np.zeros((0, 3)), 10, [0, 0, 0])
    assert e.value.code == -1
    with pytest.raises(tdtk.TdtkError) as e:
        tdtk.calculateNormalsKNN(pts, 65, [0, 0, 0])
    assert e.value.code == -5
    with pytest.raises(tdtk.TdtkError) as e:
        tdtk.calculateNormalsRange(np.zeros((0, 3)), 0.1, [0, 0, 0])
    assert e.value.code == -1
    for r2 in (0.0, -1.0):
        with pytest.raises(tdtk.TdtkError) as e:
            tdtk.calculateNormalsRange(pts, r2, [0, 0, 0])
        assert e.value.code == -1
    off, idx, d2 = kd.fixedRangeSearchBatch(pts[:10], 0.0)       # valid: empty lists
    assert off.tolist() == [0] * 11 and len(idx) == 0
    assert L.tdtk_knn_search(kd._h, None, 0, 10, None, None) == 0


def test_apx_knn_normals_unchanged(tdtk, gpu):
    """k_ann_normals after eigen3_newmat moved into a header shared with query.hip: the K7 fixture, bit for bit"""
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(G, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec); spec.loader.exec_module(mg)
    z = np.load(os.path.join(G, "k7_ann_normals.npz"))
    for tag, pts in mg.k7_clouds().items():
        got, knn = tdtk.calculateNormalsApxKNN(pts, 10, [0.0, 0.0, 0.0], 1.0, want_knn=True)
        assert np.array_equal(knn, z[tag + "_knn"]) and np.array_equal(got, z[tag + "_normals"])


def test_knn_every_list_capacity_band(tdtk, orc, gpu):
    """k inside each kernel's capacity band (register lists of 4, 10, 20, 32 slots with the -0.0 front slots, the LDS list
    of 64): lists against the reference library (or brute-force distance multisets), and the KNN normals through them"""
    mg = _mg()
    rng = np.random.default_rng(1004)
    pts = rng.uniform(-20, 20, (60_000, 3))
    pts[1000:1100] = pts[0:100]                                    # duplicates: ties inside every band
    Q = np.vstack([pts[rng.choice(len(pts), 1500, replace=False)], rng.uniform(-22, 22, (500, 3))])
    kd = tdtk.KDtree(pts, 20)
    t = mg.RefTree(pts, 20) if orc.have_ref() else None
    for k in (3, 7, 15, 25, 32, 33, 50):
        idx, d2 = kd.kNearestNeighborsBatch(Q, k)
        _check_knn_lists(mg, pts, Q, idx, d2, k)
        if t is not None:
            assert np.array_equal(idx, mg.ref_knn(t, Q, k)), k
        else:
            for i in range(0, len(Q), 10):
                all_d = mg.dist2(pts, np.broadcast_to(Q[i], pts.shape), np.arange(len(pts)))
                assert np.array_equal(d2[i], np.sort(all_d)[:k]), (k, i)
        sub = pts[:3000]
        nrm, knn = tdtk.calculateNormalsKNN(sub, k, mg.RPOS, bucketSize=5, want_knn=True)
        assert np.array_equal(knn, tdtk.KDtree(sub, 5).kNearestNeighborsBatch(sub, k)[0]), k
        assert np.array_equal(nrm, orc.normals_from_knn(sub, knn, mg.RPOS)), k
