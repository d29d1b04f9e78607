"""The cylinder, box and segment queries on the resident kd-tree against the reference's own compiled code:
fixedRangeSearchAlongDir, fixedRangeSearchBetween2Points, AABBSearch, segmentSearch_all as CSR lists in the reference's
visiting order, segmentSearch_1NearestPoint as one index and one d2 per query.

Every comparison is exact.  Lists are compared with the reference library where oracle/_ref travelled (orc.have_ref()),
else with the k10 fixture (tests/golden/make_golden_segments.py): whole lists for the small clouds, for the large ones each
list's length and the CRC-32 of its entries in list order.  Each edge test first asserts the precondition that makes it
reach its branch."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
pytestmark = pytest.mark.gpu

# query.hip's launch geometry, restated
Q_MAX_BLOCKS, Q_BLOCK, Q_SD = 2048, 128, 16
TDTK_EINVAL = -1


def _ms():
    spec = importlib.util.spec_from_file_location("make_golden_segments", os.path.join(G, "make_golden_segments.py"))
    ms = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ms)
    return ms


def _k10():
    return np.load(os.path.join(G, "k10_kdtree_segment_queries.npz"))


def _device_lists(kd, kind, A, B, md2):
    if kind == "along":
        return kd.fixedRangeSearchAlongDirBatch(A, B, md2)
    if kind == "between":
        return kd.fixedRangeSearchBetween2PointsBatch(A, B, md2)
    if kind == "aabb":
        return kd.AABBSearchBatch(A, B)
    return kd.segmentSearch_allBatch(A, B, md2)


def _check_nearest(ms, pts, P, idx, d2):
    """d2 is Dist2(p, point) of the returned point, -1.0 where there is none"""
    assert idx.dtype == np.int32 and idx.shape == d2.shape == (len(P),)
    assert ((idx >= -1) & (idx < len(pts))).all()
    with np.errstate(invalid="ignore", over="ignore"):
        assert np.array_equal(d2, ms.dist2(pts, P, idx), equal_nan=True)


def _sub_lists(off, idx, rows):
    lists = [idx[int(off[i]):int(off[i + 1])] for i in rows]
    o = np.zeros(len(lists) + 1, np.uint64)
    o[1:] = np.cumsum([len(l) for l in lists])
    return o, (np.concatenate(lists) if lists else np.zeros(0, np.int32))


def _edge_parity(ms, orc, z, name, bucket, pts, q, md2, rows, got, near):
    """the compared rows of an edge case against the live reference, or against the lengths and CRCs it left in k10"""
    if orc.have_ref():
        t = ms.SegRef(pts, bucket)
        for kind in ms.LIST_KINDS:
            A, B = ms.pair(kind, q)
            woff, widx = ms.ref_lists(t, kind, A, B, md2[kind], rows)
            goff, gidx = _sub_lists(*got[kind], rows)
            assert np.array_equal(goff, woff) and np.array_equal(gidx, widx), (name, bucket, kind)
        assert np.array_equal(near[rows], ms.ref_nearest(t, q["P"], q["P0"], md2["near"], rows)), (name, bucket)
    else:
        rows = rows[:ms.FALLBACK_ROWS]
        for kind in ms.LIST_KINDS:
            cnt, crc = ms.digest(*_sub_lists(*got[kind], rows))
            assert np.array_equal(cnt, z["%s_b%d_%s_cnt" % (name, bucket, kind)]), (name, bucket, kind)
            assert np.array_equal(crc, z["%s_b%d_%s_crc" % (name, bucket, kind)]), (name, bucket, kind)
        assert np.array_equal(near[rows], z["%s_b%d_near" % (name, bucket)]), (name, bucket)


def _run_edge_case(ms, tdtk, name, bucket, kd=None):
    pts, q, md2, rows = ms.edge_case(name, bucket)
    kd = kd or tdtk.KDtree(pts, bucket)
    got = {}
    for kind in ms.LIST_KINDS:
        A, B = ms.pair(kind, q)
        got[kind] = _device_lists(kd, kind, A, B, md2[kind])
        print("%s, bucket %d, %s: %d queries, %d entries" % (name, bucket, kind, len(A), len(got[kind][1])))
        ms.check_lists(kind, pts, A, B, md2[kind], *got[kind])
    near, d2 = kd.segmentSearch_1NearestPointBatch(q["P"], q["P0"], md2["near"])
    _check_nearest(ms, pts, q["P"], near, d2)
    hit = near >= 0
    assert ms.leaf_take("near", pts[near[hit]], q["P"][hit], q["P0"][hit], md2["near"]).all()
    return pts, q, md2, rows, got, near, kd


# ---- 1. the small clouds ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["uniform", "duplicates", "lattice", "plane", "clusters", "seven", "one"])
def test_small_clouds_equal_the_reference(tdtk, orc, gpu, name):
    ms, z = _ms(), _k10()
    pts, Q, no, r2 = ms.k8_clouds()[name]
    q = ms.k10_queries(pts, Q)
    n = q["n"]
    for b in ms.BUCKETS:
        kd = tdtk.KDtree(pts, b)
        assert kd.verify() == [0, 0, 0, 0]
        t = ms.SegRef(pts, b) if orc.have_ref() else None
        got = {}
        for kind in ms.LIST_KINDS:
            A, B = ms.pair(kind, q)
            if t is not None:
                woff, widx = ms.ref_lists(t, kind, A, B, r2)
            else:
                woff = z["%s_b%d_%s_off" % (name, b, kind)].astype(np.uint64)
                widx = z["%s_b%d_%s_idx" % (name, b, kind)].astype(np.int32)
            off, idx = _device_lists(kd, kind, A, B, r2)
            assert off.dtype == np.uint64 and idx.dtype == np.int32
            assert np.array_equal(off, woff) and np.array_equal(idx, widx), (name, b, kind)
            assert int(off[n]) > 0
            got[kind] = (off, idx)
        want = ms.ref_nearest(t, q["P"], q["P0"], r2) if t is not None else z["%s_b%d_near" % (name, b)].astype(np.int32)
        near, d2 = kd.segmentSearch_1NearestPointBatch(q["P"], q["P0"], r2)
        assert np.array_equal(near, want), (name, b)
        _check_nearest(ms, pts, q["P"], near, d2)
        assert near[n] >= 0 or name == "one" or not (ms.dist2(pts, np.broadcast_to(q["P"][n], pts.shape),
                                                              np.arange(len(pts))) < r2).any()   # p == p0 still finds
        # Between2Points' root tests fire: same dir, another list (observed on the reference for these cases)
        if (name, b) in (("lattice", 1), ("lattice", 5), ("seven", 1), ("seven", 5)):
            a, w = got["along"], got["between"]
            assert not (np.array_equal(a[0][:n + 1], w[0][:n + 1]) and
                        np.array_equal(a[1][:int(a[0][n])], w[1][:int(w[0][n])])), (name, b)
        # the single-query wrappers are the batch's rows
        for i in (0, n // 2, n, n + 1, n + 3):
            rows = {kind: got[kind][1][int(got[kind][0][i]):int(got[kind][0][i + 1])].tolist() for kind in ms.LIST_KINDS}
            assert kd.fixedRangeSearchAlongDir(q["P"][i], q["DIR"][i], r2) == rows["along"]
            assert kd.fixedRangeSearchBetween2Points(q["P"][i], q["P0"][i], r2, 3) == rows["between"]
            assert kd.AABBSearch(q["LO"][i], q["HI"][i]) == rows["aabb"]
            assert kd.segmentSearch_all(q["P"][i], q["P0"][i], r2) == rows["segall"]
            assert kd.segmentSearch_1NearestPoint(q["P"][i], q["P0"][i], r2) == (None if near[i] < 0 else int(near[i]))


def test_tree_from_scans_equals_the_reference(tdtk, orc, gpu):
    """tdtk_tree_create_from_scans: the indices count through the concatenation"""
    ms, z = _ms(), _k10()
    pts, Q, no, r2 = ms.k8_clouds()["uniform"]
    q = ms.k10_queries(pts, Q)
    sa = tdtk.Scan([0, 0, 0], [0, 0, 0], pts[:400], bucketSize=5)
    sb = tdtk.Scan([0, 0, 0], [0, 0, 0], pts[400:], bucketSize=5)
    kd = tdtk.MetaScan([sa, sb]).getSearchTree()
    cur = []
    for sc in (sa, sb):
        xyz = np.empty((sc.n, 3)); nrm = np.empty((sc.n, 3))
        tdtk.lib().tdtk_scan_download(sc.handle, xyz.ctypes.data_as(C.POINTER(C.c_double)),
                                      nrm.ctypes.data_as(C.POINTER(C.c_double)))
        cur.append(xyz)
    assert np.array_equal(np.vstack(cur), pts)
    t = ms.SegRef(pts, 5) if orc.have_ref() else None
    for kind in ms.LIST_KINDS:
        A, B = ms.pair(kind, q)
        if t is not None:
            woff, widx = ms.ref_lists(t, kind, A, B, r2)
        else:
            woff, widx = z["uniform_b5_%s_off" % kind].astype(np.uint64), z["uniform_b5_%s_idx" % kind].astype(np.int32)
        off, idx = _device_lists(kd, kind, A, B, r2)
        assert np.array_equal(off, woff) and np.array_equal(idx, widx), kind
    want = ms.ref_nearest(t, q["P"], q["P0"], r2) if t is not None else z["uniform_b5_near"].astype(np.int32)
    assert np.array_equal(kd.segmentSearch_1NearestPointBatch(q["P"], q["P0"], r2)[0], want)


# ---- 2. every kernel past its first grid-stride trip ------------------------------------------------------------------
def test_beyond_one_query_per_lane(tdtk, orc, gpu):
    """600,000 queries: more than twice the 262,144 lanes of the capped grid, most sorted positions are a lane's second or
    later query in the four count walks, the four fill walks and the nearest-point walk"""
    ms, z = _ms(), _k10()
    pts, q, md2, rows, got, near, kd = _run_edge_case(ms, tdtk, "trips", 20)
    K = len(q["P"])
    assert K == 600_000 and K > 2 * Q_MAX_BLOCKS * Q_BLOCK and len(pts) == 200_000 and len(rows) == 2_000
    for kind in ms.LIST_KINDS:
        assert 0 < len(got[kind][1]) < 5_000_000, kind
    assert (near >= 0).sum() > K // 2
    _edge_parity(ms, orc, z, "trips", 20, pts, q, md2, rows, got, near)
    # batch invariance: 50,000 queries alone are one trip per lane
    s = 275_000
    sub = {key: (v[s:s + 50_000] if key != "n" else 50_000) for key, v in q.items()}
    for kind in ms.LIST_KINDS:
        A, B = ms.pair(kind, sub)
        off, idx = _device_lists(kd, kind, A, B, md2[kind])
        goff, gidx = got[kind]
        assert np.array_equal(off, goff[s:s + 50_001] - goff[s]) and np.array_equal(idx, gidx[int(goff[s]):int(goff[s + 50_000])])
    assert np.array_equal(kd.segmentSearch_1NearestPointBatch(sub["P"], sub["P0"], md2["near"])[0], near[s:s + 50_000])


# ---- 3. deep trees: the overflow stack ---------------------------------------------------------------------------------
@pytest.mark.parametrize("bucket", [1, 20])
def test_deep_tree_on_the_overflow_stack(tdtk, orc, gpu, bucket):
    """a tree about 80 levels deep, five times the stack's LDS levels: the both-children walks keep one pending sibling per
    level, the box and nearest-point walks one per open near side"""
    ms, z = _ms(), _k10()
    pts, _, _, _ = ms.edge_case("deep", bucket)
    kd = tdtk.KDtree(pts, bucket)
    info = kd.info()
    print("deep cloud, bucket %d: max_depth %d" % (bucket, info["max_depth"]))
    assert info["max_depth"] > Q_SD and info["max_depth"] >= 4 * Q_SD
    pts, q, md2, rows, got, near, kd = _run_edge_case(ms, tdtk, "deep", bucket, kd)
    assert len(rows) == 300 and all(len(got[kind][1]) > 0 for kind in ms.LIST_KINDS) and (near >= 0).any()
    _edge_parity(ms, orc, z, "deep", bucket, pts, q, md2, rows, got, near)


# ---- 4. leaf table mode ------------------------------------------------------------------------------------------------
def test_table_mode_leaves_of_thousands_of_points(tdtk, orc, gpu):
    ms, z = _ms(), _k10()
    pts, _, _, _ = ms.edge_case("table")
    kd = tdtk.KDtree(pts, 20)
    info = kd.info()
    # kd_build.cpp's packing rule: (start << cb) | count must fit in 30 bits, else the leaves go through leaf_tab
    assert int(info["n_points"]).bit_length() + int(info["max_leaf_points"]).bit_length() > 30
    assert info["max_leaf_points"] >= 40_000
    pts, q, md2, rows, got, near, kd = _run_edge_case(ms, tdtk, "table", 20, kd)
    for kind in ms.LIST_KINDS:
        cnt = np.diff(got[kind][0].astype(np.int64))
        assert (cnt >= 40_000).sum() >= 8 and len(got[kind][1]) < 5_000_000, kind     # lists through the leaf of copies
    _edge_parity(ms, orc, z, "table", 20, pts, q, md2, rows, got, near)


# ---- 5. non-finite queries ---------------------------------------------------------------------------------------------
def test_far_and_non_finite_queries(tdtk, orc, gpu):
    """NaN, +-inf, 1e160 and -1e200 in p, p0 (each query's p0 is the p of the query seven places before it), dir and the box
    corners, among ordinary queries: the reference's answers, whatever they are"""
    ms, z = _ms(), _k10()
    with np.errstate(invalid="ignore", over="ignore"):
        pts, q, md2, rows, got, near, kd = _run_edge_case(ms, tdtk, "nonfinite", 20)
        bad = ~(np.isfinite(q["P"]).all(1) & np.isfinite(q["P0"]).all(1))
        assert 28 <= bad.sum() < len(bad) and np.isnan(q["DIR"]).any() and np.isnan(q["LO"]).any() and np.isinf(q["HI"]).any()
        _edge_parity(ms, orc, z, "nonfinite", 20, pts, q, md2, rows, got, near)
        assert all(len(got[kind][1]) > 0 for kind in ms.LIST_KINDS) and (near[~bad] >= 0).any()


# ---- 6. error paths and contracts --------------------------------------------------------------------------------------
def test_error_paths_and_contracts(tdtk, gpu):
    L = tdtk.lib()
    ms = _ms()
    pts, Q, no, r2 = ms.k8_clouds()["uniform"]
    q = ms.k10_queries(pts, Q)
    n = q["n"]
    kd = tdtk.KDtree(pts, 5)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    P, P0, DIR = (np.ascontiguousarray(q[k][:n]) for k in ("P", "P0", "DIR"))
    LO, HI = np.ascontiguousarray(q["LO"][:n]), np.ascontiguousarray(q["HI"][:n])
    calls = {
        "along": lambda K, o, i, cap, t: L.tdtk_fixed_range_search_along_dir(kd._h, dp(P), dp(DIR), K, r2, o, i, cap, t),
        "between": lambda K, o, i, cap, t: L.tdtk_fixed_range_search_between(kd._h, dp(P), dp(P0), K, r2, o, i, cap, t),
        "aabb": lambda K, o, i, cap, t: L.tdtk_aabb_search(kd._h, dp(LO), dp(HI), K, o, i, cap, t),
        "segall": lambda K, o, i, cap, t: L.tdtk_segment_search_all(kd._h, dp(P), dp(P0), K, r2, o, i, cap, t),
    }
    for kind, call in calls.items():
        woff, widx = _device_lists(kd, kind, *ms.pair(kind, {k: (v[:n] if k != "n" else n) for k, v in q.items()}), r2)
        total = int(woff[-1])
        assert total > n
        # cap too small: the error names both numbers, offsets and total are filled, idx is not touched
        off = np.full(n + 1, 7, np.uint64)
        idx = np.full(total, -7, np.int32)
        tot = C.c_uint64(99)
        assert call(n, up(off), ip(idx), total - 1, C.byref(tot)) == TDTK_EINVAL
        msg = L.tdtk_last_error().decode()
        assert str(total) in msg and str(total - 1) in msg, msg
        assert tot.value == total and np.array_equal(off, woff) and (idx == -7).all()
        # ... and a second call with that capacity succeeds
        assert call(n, up(off), ip(idx), total, C.byref(tot)) == 0
        assert tot.value == total and np.array_equal(off, woff) and np.array_equal(idx, widx)
        # K == 0: a no-op that reports an empty result
        off0 = np.full(1, 7, np.uint64)
        tot = C.c_uint64(99)
        assert call(0, up(off0), None, 0, C.byref(tot)) == 0 and off0[0] == 0 and tot.value == 0
        # NULL arguments
        assert call(n, None, ip(idx), total, C.byref(tot)) == TDTK_EINVAL
        assert call(n, up(off), ip(idx), total, None) == TDTK_EINVAL
        assert call(n, up(off), None, total, C.byref(tot)) == TDTK_EINVAL          # lists to write and nowhere to
    tot = C.c_uint64(0)
    off = np.zeros(n + 1, np.uint64)
    idx = np.zeros(8, np.int32)
    assert L.tdtk_fixed_range_search_along_dir(None, dp(P), dp(DIR), n, r2, up(off), ip(idx), 8, C.byref(tot)) == TDTK_EINVAL
    assert L.tdtk_fixed_range_search_along_dir(kd._h, None, dp(DIR), n, r2, up(off), ip(idx), 8, C.byref(tot)) == TDTK_EINVAL
    assert L.tdtk_fixed_range_search_between(kd._h, dp(P), None, n, r2, up(off), ip(idx), 8, C.byref(tot)) == TDTK_EINVAL
    assert L.tdtk_aabb_search(kd._h, dp(LO), None, n, up(off), ip(idx), 8, C.byref(tot)) == TDTK_EINVAL
    assert L.tdtk_segment_search_all(kd._h, None, dp(P0), n, r2, up(off), ip(idx), 8, C.byref(tot)) == TDTK_EINVAL
    # an invalid box anywhere in the batch: refused before anything is written
    for row, ax in ((0, 0), (n // 2, 1), (n - 1, 2)):
        lo = LO.copy()
        lo[row, ax] = HI[row, ax] + 1.0
        off = np.full(n + 1, 7, np.uint64)
        idx = np.full(8, -7, np.int32)
        tot = C.c_uint64(99)
        assert L.tdtk_aabb_search(kd._h, dp(lo), dp(HI), n, up(off), ip(idx), 8, C.byref(tot)) == TDTK_EINVAL
        assert "invalid bbox" in L.tdtk_last_error().decode()
        assert (off == 7).all() and (idx == -7).all() and tot.value == 99
        with pytest.raises(Exception, match="invalid bbox"):
            kd.AABBSearchBatch(lo, HI)
    with pytest.raises(Exception, match="invalid bbox"):
        kd.AABBSearch([1.0, 0.0, 0.0], [0.0, 1.0, 1.0])
    # the nearest-point call: d2 is optional, idx is not; K == 0
    near, d2 = kd.segmentSearch_1NearestPointBatch(P, P0, r2)
    got = np.full(n, -7, np.int32)
    assert L.tdtk_segment_search_nearest(kd._h, dp(P), dp(P0), n, r2, ip(got), None) == 0
    assert np.array_equal(got, near)
    assert L.tdtk_segment_search_nearest(kd._h, dp(P), dp(P0), 0, r2, None, None) == 0
    assert L.tdtk_segment_search_nearest(kd._h, dp(P), dp(P0), n, r2, None, dp(d2)) == TDTK_EINVAL
    assert L.tdtk_segment_search_nearest(kd._h, dp(P), None, n, r2, ip(got), None) == TDTK_EINVAL
    assert L.tdtk_segment_search_nearest(None, dp(P), dp(P0), n, r2, ip(got), None) == TDTK_EINVAL
    # the Python batch forms ask again when the first capacity (32 per query) does not fit
    big = kd.fixedRangeSearchAlongDirBatch(P, DIR, 100.0)
    assert len(big[1]) > 32 * n and int(big[0][-1]) == len(big[1])
    ms.check_lists("along", pts, P, DIR, 100.0, *big)


# ---- 7. shared workspaces ----------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_calls_before_them(tdtk, gpu):
    """the new calls use the context's workspaces next to tdtk_knn_search, tdtk_fixed_range_search and
    tdtk_find_closest_along_dir (the bin's second vector, the counts and the offsets share slots with them): each call
    gives what it gave first, whatever ran in between"""
    ms = _ms()
    me = ms._load("make_golden_knn_edges")
    dpts, geo = me.deep_cloud()
    deep = tdtk.KDtree(dpts, 20)
    assert deep.info()["max_depth"] >= 4 * Q_SD
    rng = np.random.default_rng(1071)
    spts = rng.uniform(-20, 20, (50_000, 3))
    shallow = tdtk.KDtree(spts, 20)
    assert shallow.info()["max_depth"] <= Q_SD - 1
    Qd = me.deep_queries(dpts, geo, 1_500, 1072)
    Qd0 = Qd * 1.01 + rng.normal(0, 1.5, Qd.shape)
    Qs = rng.uniform(-22, 22, (300_000, 3))                          # more queries than lanes
    Qs0 = Qs + rng.normal(0, 1.0, Qs.shape)
    Ds = ms._unit(Qs0 - Qs)
    few = Qs[:9]
    calls = {
        "knn": lambda: shallow.kNearestNeighborsBatch(Qs, 10),
        "range": lambda: shallow.fixedRangeSearchBatch(Qs[:50_000], 4.0),
        "closest_dir": lambda: shallow.FindClosestAlongDirBatch(Qs[:50_000], Ds[:50_000], 1.0),
        "along": lambda: shallow.fixedRangeSearchAlongDirBatch(Qs, Ds, 0.04),
        "along_few": lambda: shallow.fixedRangeSearchAlongDirBatch(few, Ds[:9], 0.25),
        "between": lambda: shallow.fixedRangeSearchBetween2PointsBatch(Qs, Qs0, 0.04),
        "aabb": lambda: shallow.AABBSearchBatch(np.minimum(Qs, Qs0), np.maximum(Qs, Qs0)),
        "segall": lambda: shallow.segmentSearch_allBatch(Qs, Qs0, 1.0),
        "near": lambda: shallow.segmentSearch_1NearestPointBatch(Qs, Qs0, 1.0),
        "deep_segall": lambda: deep.segmentSearch_allBatch(Qd, Qd0, 9.0),
        "deep_near": lambda: deep.segmentSearch_1NearestPointBatch(Qd, Qd0, 9.0),
        "deep_knn": lambda: deep.kNearestNeighborsBatch(Qd, 33),
        "nothing": lambda: shallow.segmentSearch_allBatch(Qs[:1_000] + 1e4, Qs0[:1_000] + 1e4, 1.0),
    }
    first = {name: f() for name, f in calls.items()}
    assert int(first["nothing"][0][-1]) == 0 and all(int(first[k][0][-1]) > 0 for k in ("along", "between", "aabb", "segall"))
    order = ["knn", "along", "closest_dir", "between", "range", "aabb", "along_few", "segall", "nothing", "near", "knn",
             "deep_segall", "along_few", "deep_near", "closest_dir", "near", "deep_knn", "segall", "range", "deep_segall",
             "nothing", "along", "deep_near", "aabb", "between", "deep_knn"]
    assert set(order) == set(calls)
    for step, name in enumerate(order):
        got = calls[name]()
        assert len(got) == len(first[name])
        for a, b in zip(got, first[name]):
            assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), (step, name)
