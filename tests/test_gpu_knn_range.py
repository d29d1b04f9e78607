"""k nearest within a radius on the device kd-tree and the normals over its lists (k_knnr_reg / k_knnr_lds): the GPU tier.
Rows equal KDtree::kNearestRangeSearch of the reference's compiled kd.cc (the k12 fixture: coordinates), and index for index
the two identities that tie the walk to the pinned ones: a list that never filled is the d2-sorted fixedRangeSearch list, a
radius that holds everything gives kNearestNeighbors' distances."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
pytestmark = pytest.mark.gpu

dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))


@pytest.fixture(scope="module")
def mr():
    spec = importlib.util.spec_from_file_location("make_golden_knn_range", os.path.join(G, "make_golden_knn_range.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def fx(mr):
    return mr.load()


def _check_rows(mr, pts, Q, idx, d2, cnt, k):
    """-1 / -1.0 behind the entries, d2 = Dist2 of the returned points"""
    assert idx.shape == d2.shape == (len(Q), k) and cnt.shape == (len(Q),)
    behind = np.arange(k)[None, :] >= cnt[:, None]
    assert np.array_equal(idx < 0, behind) and (idx[behind] == -1).all() and (d2[behind] == -1.0).all()
    assert (idx < len(pts)).all()
    for s in range(0, len(Q), 100_000):
        e = min(s + 100_000, len(Q))
        assert np.array_equal(d2[s:e], mr.G8.dist2(pts, Q[s:e, None, :], idx[s:e]), equal_nan=True)


def _sorted_range_rows(kd, Q, r2, k):
    """fixedRangeSearchBatch's lists, each stably sorted by d2, as [Q][k] rows (-1 behind; rows longer than k are cut) and
    their full lengths"""
    off, ridx, rd2 = kd.fixedRangeSearchBatch(Q, r2)
    cnt = np.diff(off.astype(np.int64))
    row = np.repeat(np.arange(len(Q)), cnt)
    o = np.lexsort((np.arange(len(ridx)), rd2, row))          # by row, then d2, then position: the stable sort of every list
    pos = np.arange(len(ridx)) - np.repeat(off[:-1].astype(np.int64), cnt)
    keep = pos < k
    rows = -np.ones((len(Q), k), np.int32)
    rows[row[keep], pos[keep]] = ridx[o][keep]
    return rows, cnt


def test_fixture_parity(tdtk, gpu, mr, fx):
    for name, (pts, Q, no, _) in mr.G8.k8_clouds().items():
        for b in mr.BUCKETS:
            kd = tdtk.KDtree(pts, b)
            for ri, r2 in enumerate(fx.radii(name)):
                for k in mr.KS:
                    tag = (name, b, ri, k)
                    idx, d2, cnt = kd.kNearestRangeSearchBatch(Q, k, r2)
                    _check_rows(mr, pts, Q, idx, d2, cnt, k)
                    assert np.array_equal(cnt, fx.counts(name, ri, b, k)), tag
                    rep = fx.rows(name, ri, b, k)
                    have = idx >= 0
                    assert np.array_equal(have, rep >= 0), tag
                    assert np.array_equal(pts[idx[have]], pts[rep[have]]), tag


def test_index_exactness_against_the_pinned_walks(tdtk, gpu, mr, fx):
    n_short = 0
    for name, (pts, Q, no, _) in mr.G8.k8_clouds().items():
        for b in mr.BUCKETS:
            kd = tdtk.KDtree(pts, b)
            for k in mr.KS:
                for r2 in fx.radii(name)[:2]:
                    idx, _, cnt = kd.kNearestRangeSearchBatch(Q, k, r2)
                    want, full = _sorted_range_rows(kd, Q, r2, k)
                    short = cnt < k
                    assert np.array_equal(cnt, np.minimum(full, k)), (name, b, k, r2)
                    assert np.array_equal(idx[short], want[short]), (name, b, k, r2)
                    n_short += int(short.sum())
                _, d2, cnt = kd.kNearestRangeSearchBatch(Q, k, 1e30)
                assert np.array_equal(d2, kd.kNearestNeighborsBatch(Q, k)[1]), (name, b, k)
                assert (cnt == min(k, len(pts))).all()
    assert n_short > 10000


def test_normals(tdtk, gpu, mr, fx):
    lens = set()
    for name, (pts, Q, no, _) in mr.G8.k8_clouds().items():
        own = np.array([int(np.nonzero((pts == q).all(1))[0][0]) for q in Q[:no]])
        for b in mr.BUCKETS:
            kd = tdtk.KDtree(pts, b)
            for ri, r2 in enumerate(fx.radii(name)):
                for k in mr.NORMAL_KS:
                    tag = (name, b, ri, k)
                    nrm, knn, cnt = tdtk.calculateNormalsKNNRange(pts, k, r2, mr.RPOS, bucketSize=b, want_knn=True)
                    idx, _, c2 = kd.kNearestRangeSearchBatch(pts, k, r2)
                    assert np.array_equal(knn, idx) and np.array_equal(cnt, c2), tag
                    # (a point's list depends on its coordinates only: a duplicate's row is its twin's)
                    assert np.array_equal(cnt[own], fx.counts(name, ri, b, k)[:no]), tag
                    assert np.array_equal(nrm[own], fx.normals(name, ri, b, k), equal_nan=True), tag
                    assert np.array_equal(tdtk.calculateNormalsKNNRange(pts, k, r2, mr.RPOS, bucketSize=b), nrm, equal_nan=True)
                    lens |= set(cnt[own].tolist())
    assert {1, 2} <= lens


def test_grid_stride_second_trip(tdtk, gpu, mr):
    """300 000 queries: above 2048 x 128 lanes (a second trip of the grid-stride loop) and 2048 x 64 (a fifth of the LDS-list
    kernel's); bucket 2 makes the tree deeper than the LDS levels of the lane stack.  No brute force at this size: the two
    identities against the pinned walks."""
    rng = np.random.default_rng(1201)
    pts = rng.uniform(-50, 50, (300_000, 3))
    kd = tdtk.KDtree(pts, 2)
    small = (5.0 * 1e6 / len(pts) * 3 / (4 * np.pi)) ** (2.0 / 3.0)       # ~5 neighbours per query
    want40, full = _sorted_range_rows(kd, pts, small, 40)
    for k in (10, 40):
        idx, d2, cnt = kd.kNearestRangeSearchBatch(pts, k, small)
        _check_rows(mr, pts, pts, idx, d2, cnt, k)
        want = want40[:, :k]
        short = cnt < k
        assert np.array_equal(cnt, np.minimum(full, k)) and short.mean() > 0.9 and (cnt >= 1).all()
        assert np.array_equal(idx[short], want[short]), k
        assert (d2[~short] < small).all() and (np.diff(d2[~short], axis=1) >= 0).all()
        idx, d2, cnt = kd.kNearestRangeSearchBatch(pts, k, 1e30)
        _check_rows(mr, pts, pts, idx, d2, cnt, k)
        assert (cnt == k).all() and np.array_equal(d2, kd.kNearestNeighborsBatch(pts, k)[1]), k


def test_edges(tdtk, gpu, mr):
    L = tdtk.lib()
    seven = mr.G8.k8_clouds()["seven"][0]
    kd = tdtk.KDtree(seven, 20)
    # K = 0: a no-op
    assert L.tdtk_knn_range_search(kd._h, None, 0, 10, 1.0, None, None, None) == 0
    idx, d2, cnt = kd.kNearestRangeSearchBatch(np.zeros((0, 3)), 10, 1.0)
    assert idx.shape == (0, 10) and cnt.shape == (0,)
    # a one-point tree
    one = np.array([[0.25, -0.5, 1.5]])
    k1 = tdtk.KDtree(one, 20)
    idx, d2, cnt = k1.kNearestRangeSearchBatch(np.array([[0.25, -0.5, 1.5], [0.25, -0.5, 2.5], [0.25, -0.5, 2.0]]), 4, 1.0)
    assert idx.tolist() == [[0, -1, -1, -1], [-1] * 4, [0, -1, -1, -1]] and cnt.tolist() == [1, 0, 1]   # (d2 = 1.0 is not < 1.0)
    assert d2.tolist() == [[0.0, -1.0, -1.0, -1.0], [-1.0] * 4, [0.25, -1.0, -1.0, -1.0]]
    assert k1.kNearestRangeSearch(one[0], 4, 1.0) == [0] and k1.kNearestRangeSearch([9.0, 9.0, 9.0], 4, 1.0) == []
    # k larger than the cloud
    idx, d2, cnt = kd.kNearestRangeSearchBatch(seven, 33, 1e30)
    assert (cnt == 7).all() and (idx[:, 7:] == -1).all() and (np.sort(idx[:, :7], axis=1) == np.arange(7)).all()
    assert idx[:, 0].tolist() == list(range(7))
    # sqRad2 = 0 (and below): empty rows
    for r2 in (0.0, -1.0):
        idx, d2, cnt = kd.kNearestRangeSearchBatch(seven, 10, r2)
        assert (idx == -1).all() and (d2 == -1.0).all() and (cnt == 0).all()
    # a NaN coordinate, by the rules: every Dist2 is NaN, so no point is skipped (NaN >= r2 is false) and each goes into the
    # first unset slot (a NaN slot is neither < 0 nor > NaN) until the list is full; a box value of NaN never prunes, and on
    # the NaN axis myd is NaN: child2 first, child1 never.  The list therefore holds points -- with bucket 20 the first
    # min(k, 7) of the one leaf, with bucket 1 and the NaN in z (the axis of every split on the way) point 6 alone: root at the
    # centroid -0.2106 -> {1, 4, 5, 6}, at 0.2297 -> {5, 6}, at 0.5857 -> {6} -- but the result is the slots with a distance
    # >= 0, and NaN >= 0 is false: every row is empty, as kNearestNeighbors' rows are for such a query.
    nan = float("nan")
    for b in (1, 5, 20):
        kb = tdtk.KDtree(seven, b)
        Q = np.array([[nan, 0.0, 0.0], [0.1, nan, 0.2], [0.3, 0.1, nan], [nan, nan, nan], seven[3]])
        for k, r2 in ((1, 0.5), (4, 1e-6), (10, 1e30), (33, 1.0)):
            idx, d2, cnt = kb.kNearestRangeSearchBatch(Q, k, r2)
            assert (idx[:4] == -1).all() and (d2[:4] == -1.0).all() and cnt[:4].tolist() == [0] * 4, (b, k)
            assert idx[4, 0] == 3 and d2[4, 0] == 0.0 and cnt[4] >= 1, (b, k)      # the ordinary query beside them


def test_errors_leave_the_outputs_alone(tdtk, gpu, mr):
    L = tdtk.lib()
    pts = np.ascontiguousarray(mr.G8.k8_clouds()["uniform"][0])
    kd = tdtk.KDtree(pts, 20)
    q = np.ascontiguousarray(pts[:10])
    idx = np.full((10, 64), -7, np.int32); d2 = np.full((10, 64), -7.0); cnt = np.full(10, -7, np.int32)
    rp = np.zeros(3)
    nrm = np.full((len(pts), 3), -7.0); knn = np.full((len(pts), 64), -7, np.int32); nc = np.full(len(pts), -7, np.int32)

    def untouched():
        return (idx == -7).all() and (d2 == -7.0).all() and (cnt == -7).all() and (nrm == -7.0).all() and (knn == -7).all() \
            and (nc == -7).all()

    search = lambda t, qq, k, r2, out=idx: L.tdtk_knn_range_search(t, qq, 10, k, r2, ip(out) if out is not None else None, dp(d2), ip(cnt))
    assert search(None, dp(q), 10, 1.0) == -1
    assert search(kd._h, None, 10, 1.0) == -1
    assert search(kd._h, dp(q), 10, 1.0, None) == -1
    assert search(kd._h, dp(q), 0, 1.0) == -1 and search(kd._h, dp(q), -3, float("nan")) == -1
    assert search(kd._h, dp(q), 65, float("nan")) == -5              # k > 64 is reported before the radius
    for r2 in (float("nan"), float("inf"), -float("inf")):
        assert search(kd._h, dp(q), 10, r2) == -1
    assert untouched()

    normals = lambda x, n, k, r2, r, b, out=nrm: L.tdtk_normals_knn_range(x, n, k, r2, r, b, 0, dp(out) if out is not None else None, ip(knn), ip(nc))
    assert normals(None, len(pts), 10, 1.0, dp(rp), 20) == -1
    assert normals(dp(pts), len(pts), 10, 1.0, None, 20) == -1
    assert normals(dp(pts), len(pts), 10, 1.0, dp(rp), 20, None) == -1
    assert normals(dp(pts), 0, 10, 1.0, dp(rp), 20) == -1
    assert normals(dp(pts), len(pts), 0, 1.0, dp(rp), 20) == -1
    assert normals(dp(pts), len(pts), 65, 1.0, dp(rp), 0) == -1      # bucket < 1 is reported before k > 64
    assert normals(dp(pts), len(pts), 65, float("nan"), dp(rp), 20) == -5
    for r2 in (float("nan"), float("inf"), 0.0, -1.0):
        assert normals(dp(pts), len(pts), 10, r2, dp(rp), 20) == -1
    assert untouched()
    # and through the mirror
    with pytest.raises(tdtk.TdtkError) as e:
        kd.kNearestRangeSearchBatch(q, 65, 1.0)
    assert e.value.code == -5 and "64" in str(e.value)
    with pytest.raises(tdtk.TdtkError) as e:
        kd.kNearestRangeSearchBatch(q, 10, float("inf"))
    assert e.value.code == -1
    with pytest.raises(tdtk.TdtkError) as e:
        tdtk.calculateNormalsKNNRange(pts, 10, 0.0, rp)
    assert e.value.code == -1
    # the calls still work afterwards
    idx2, _, c2 = kd.kNearestRangeSearchBatch(q, 64, 1e30)
    assert (c2 == 64).all() and (idx2 >= 0).all()
