"""The octree search tree on the device (tdtk_octree_*, BOctTree in 3dtk_amd/slam6d.py) against
tests/golden/k20_boctree_search.npz, which holds what the reference's own compiled BOctTree<double> returns: init()'s
scalars, the node / leaf / point counts, the leaf order and, for every query of every case, the returned point and its
Dist2, by bits.  getPtPairs against the k-d tree where the two searches must agree (a tie-free cloud with no partner within
0.01: tests/test_boctree_search_host.py checks that on the CPU), against the fixture where they differ, its sums inside the
tolerance tests/pair_sums_ref.py derives."""
import ctypes as C
import os

import numpy as np
import pytest

import boctree_model as bm
import pair_sums_ref as R
from boctree_model import dat_pair, move

pytestmark = pytest.mark.gpu

gen = bm.generator()
CASES = [(name, voxel, early) for name, variants in gen.CASES for voxel, early in variants]
I16 = np.eye(4).reshape(16)


@pytest.fixture(scope="module")
def fx():
    return gen.load()


_expect_idx, _check_sums = bm.expect_idx, bm.check_sums


@pytest.mark.parametrize("name,voxel,early", CASES)
def test_tree_and_find_closest_equal_the_reference(tdtk, gpu, fx, name, voxel, early):
    """info() by bits, the counts, the leaf order; FindClosestBatch on every batch and on the per-query radii at d2 and one
    ulp above it: index and Dist2 by bits, nothing skipped"""
    pts = fx.cloud(name)
    t = tdtk.BOctTree(pts, voxel, bool(early))
    info = t.info()
    got = np.array([info["max_depth"], info["real_voxelSize"], info["mult"], *info["add"], info["largest_index"], info["size"],
                    *info["center"]], np.float64)
    assert bm.same_bits(got, fx.get(name, voxel, early, "scalars"))
    assert [info["n_nodes"], info["n_leaves"], info["n_points"]] == [int(v) for v in fx.get(name, voxel, early, "counts")]
    order = t.leaf_order()
    assert bm.same_bits(pts[order], pts[fx.get(name, voxel, early, "leaf")])
    assert np.array_equal(np.sort(order), np.arange(len(pts)))
    # the node table, slot for slot, is the one the CPU tier walks (the restatement's, which that tier ties to the reference)
    assert np.array_equal(t.node_table(), bm.Model(pts, voxel, bool(early)).nodes)
    for qq, maxd2, pos, d2, _ in fx.batches(name, voxel, early):
        idx, gd2 = t.FindClosestBatch(qq, maxd2)
        want = _expect_idx(order, pos)
        assert np.array_equal(idx, want), (name, voxel, early, maxd2, np.flatnonzero(idx != want)[:5])
        assert bm.same_bits(gd2, d2)
    if (name, voxel, early) in set(gen.EDGE_CASES):
        for q1, maxd2, pos, d2, _ in fx.edge(name, voxel, early):
            idx, gd2 = t.FindClosestBatch(q1[None], maxd2)
            assert idx[0] == (order[pos] if pos >= 0 else -1) and bm.same_bits(gd2, [d2]), (name, q1, maxd2)


def test_single_query_form_and_the_answers_that_are_not_the_nearest(tdtk, gpu, fx):
    """FindClosest; the leaf limit (nothing returned although the partner is inside the radius) and the stopped search"""
    pts = fx.cloud("limit")
    t = tdtk.BOctTree(pts, 1.0, False)
    qq, maxd2 = fx.batches("limit", 1.0, 0)[0][:2]
    assert t.FindClosest(qq[0], maxd2) is None and ((pts - qq[0]) ** 2).sum(1).min() < maxd2
    assert t.FindClosest(qq[1], maxd2) == 2
    pts = fx.cloud("stop")
    t = tdtk.BOctTree(pts)
    q0 = fx.batches("stop", 10.0, 1)[0][0][0]
    hit = t.FindClosest(q0, 625.0)
    d2 = ((pts - q0) ** 2).sum(1)
    assert d2[hit] <= 0.0001 and d2.min() < d2[hit]


def test_dev_form_equals_host_form(tdtk, gpu, fx):
    import torch
    pts = fx.cloud("uniform")
    t = tdtk.BOctTree(pts)
    for qq, maxd2, _, _, _ in fx.batches("uniform", 10.0, 1):
        ref_idx, ref_d2 = t.FindClosestBatch(qq, maxd2)
        tq = torch.from_numpy(qq).cuda()
        out_i = torch.full((len(qq),), -7, dtype=torch.int32, device="cuda")
        out_d = torch.empty(len(qq), dtype=torch.float64, device="cuda")
        assert tdtk.lib().tdtk_octree_find_closest_dev(t._h, C.c_void_p(tq.data_ptr()), len(qq), maxd2, C.c_void_p(out_i.data_ptr()),
                                                       C.c_void_p(out_d.data_ptr()), None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(out_i.cpu().numpy(), ref_idx) and bm.same_bits(out_d.cpu().numpy(), ref_d2)
        side = torch.cuda.Stream()
        out_i.fill_(-7)
        side.wait_stream(torch.cuda.current_stream())
        assert tdtk.lib().tdtk_octree_find_closest_dev(t._h, C.c_void_p(tq.data_ptr()), len(qq), maxd2, C.c_void_p(out_i.data_ptr()),
                                                       C.c_void_p(out_d.data_ptr()), C.c_void_p(side.cuda_stream)) == 0
        side.synchronize()
        assert np.array_equal(out_i.cpu().numpy(), ref_idx) and bm.same_bits(out_d.cpu().numpy(), ref_d2)


def test_refusals(tdtk, gpu, fx):
    """n == 0; 22 levels (TDTK_EUNSUP, as the reduction); a radius or a query whose voxel coordinate leaves +-2^30"""
    with pytest.raises(tdtk.TdtkError) as e:
        tdtk.BOctTree(np.empty((0, 3)))
    assert e.value.code == -1
    deep = gen.mo.clouds()["deep21"]
    assert gen.mo.depth_of(deep, 0.0005) == 21 and gen.mo.depth_of(deep, gen.mo.DEEP22_VOXEL) == 22
    assert tdtk.BOctTree(deep, 0.0005, False).info()["levels"] == 21
    with pytest.raises(tdtk.TdtkError) as e:
        tdtk.BOctTree(deep, gen.mo.DEEP22_VOXEL, False)
    assert e.value.code == -5
    with pytest.raises(tdtk.TdtkError) as e:
        tdtk.BOctTree(np.array([[0.0, np.nan, 0.0]]))
    assert e.value.code == -1
    t = tdtk.BOctTree(fx.cloud("two"), 0.1, False)
    limit = 2.0 ** 30 / t.info()["mult"]
    ok = np.zeros((3, 3))
    idx = np.full(3, -7, np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    for q, maxd2 in ((ok, (limit * 1.01) ** 2), (ok, -1.0), (ok, float("nan")), (np.array([[0.0] * 3, [0.0, limit * 1.01, 0.0], [0.0] * 3]), 625.0),
                     (np.array([[0.0] * 3, [0.0] * 3, [np.nan, 0.0, 0.0]]), 625.0)):
        q = np.ascontiguousarray(q)
        rc = tdtk.lib().tdtk_octree_find_closest(t._h, q.ctypes.data_as(dp), 3, maxd2, idx.ctypes.data_as(ip), None)
        assert rc == -5 and (idx == -7).all(), (maxd2, rc)                  # the whole batch, nothing written
    assert t.FindClosestBatch(ok, (limit * 0.5) ** 2)[0].min() >= 0
    with pytest.raises(tdtk.TdtkError) as e:                                 # no FindClosestAlongDir of its own
        t.getPtPairs(I16, ok, np.tile([0.0, 0.0, 1.0], (3, 1)), pairing_mode=tdtk.CLOSEST_POINT_ALONG_NORMAL_SIMPLE)
    assert e.value.code == -5


def test_second_tree_after_destroy_reuses_pooled_blocks(tdtk, gpu, fx):
    pts = fx.cloud("uniform")
    qq, maxd2 = fx.batches("uniform", 10.0, 1)[0][:2]
    t = tdtk.BOctTree(pts)
    first = (t.info(), t.leaf_order(), t.FindClosestBatch(qq, maxd2))
    del t
    tdtk.lib().tdtk_pool_trim()
    t = tdtk.BOctTree(pts)
    del t                                      # its blocks go to the pool's shelves ...
    t = tdtk.BOctTree(pts)                     # ... and come back from there
    assert tdtk.lib().tdtk_pool_trim() == 0    # nothing left on the shelves: the second tree took exactly those blocks
    again = (t.info(), t.leaf_order(), t.FindClosestBatch(qq, maxd2))
    for k in ("n_nodes", "n_leaves", "n_points", "max_depth", "mult", "device_bytes"):
        assert first[0][k] == again[0][k]
    assert np.array_equal(first[1], again[1])
    assert np.array_equal(first[2][0], again[2][0]) and bm.same_bits(first[2][1], again[2][1])


def test_get_pt_pairs_equals_kdtree_on_the_tie_free_pair(tdtk, gpu):
    """the bundled scan pair: idx, the pair list and the raw sums equal KDtree.getPtPairs's; the sums inside the derived
    tolerance; also under a source_alignxf that is not the identity, with rnd, and for a sub-range"""
    model, data = dat_pair()
    oc, kd = tdtk.BOctTree(model), tdtk.KDtree(model)
    A = R.rigid([3.0, -2.0, 5.0], [0.01, -0.02, 0.015])
    for tag, (xf, q) in {"identity": (I16, data), "moved": (A, move(data, A))}.items():
        a, b = oc.getPtPairs(xf, q, max_dist_match2=625.0), kd.getPtPairs(xf, q, max_dist_match2=625.0)
        assert a["n"] == b["n"] > 0.5 * len(q) and np.array_equal(a["idx"], b["idx"])
        assert np.array_equal(a["p1"], b["p1"]) and np.array_equal(a["p2"], b["p2"])
        _check_sums(a, model, xf, 0, "octree getPtPairs, " + tag)
    a, b = oc.getPtPairs(I16, data, startindex=1000, endindex=31001, want=tdtk.WANT_APX), kd.getPtPairs(I16, data, startindex=1000, endindex=31001, want=tdtk.WANT_APX)
    assert np.array_equal(a["idx"], b["idx"]) and len(a["idx"]) == 30001
    _check_sums(a, model, I16, tdtk.WANT_APX, "octree getPtPairs, range, APX")
    C.CDLL(None).srand(11)
    a = oc.getPtPairs(I16, data, rnd=3)
    C.CDLL(None).srand(11)
    b = kd.getPtPairs(I16, data, rnd=3)
    assert np.array_equal(a["idx"], b["idx"]) and 0 < a["n_queries"] < len(data) // 2
    nr = np.tile([0.0, 0.6, 0.8], (len(data), 1))
    a, b = oc.getPtPairs(I16, data, nr, pairing_mode=tdtk.CLOSEST_PLANE_SIMPLE), kd.getPtPairs(I16, data, nr, pairing_mode=tdtk.CLOSEST_PLANE_SIMPLE)
    assert np.array_equal(a["idx"], b["idx"]) and np.array_equal(a["p1"], b["p1"]) and np.array_equal(a["pn"], b["pn"])


@pytest.mark.parametrize("name,voxel,early", [("octants", 10.0, 1), ("duplicates", 10.0, 1), ("stop", 10.0, 1)])
def test_get_pt_pairs_equals_the_fixture_where_the_trees_differ(tdtk, gpu, fx, name, voxel, early):
    """clouds with ties, duplicates and a stopped search: idx is the octree's own answer, the sums belong to that pair list"""
    pts = fx.cloud(name)
    t = tdtk.BOctTree(pts, voxel, bool(early))
    order = t.leaf_order()
    qq, maxd2, pos, d2, _ = fx.batches(name, voxel, early)[0]
    got = t.getPtPairs(I16, qq, max_dist_match2=maxd2)
    want = _expect_idx(order, pos)
    assert np.array_equal(got["idx"], want) and got["n"] == (want >= 0).sum() > 0
    assert np.array_equal(got["p1"], pts[want[want >= 0]]) and np.array_equal(got["p2"], qq[want >= 0])
    if name == "duplicates":
        # its first 60 queries ARE points of the cloud: pairs of length 0, one of which pair_sums_ref's discrimination would
        # leave out without moving `sum`.  The sums are checked on the range behind them (every query off its partner)
        got = t.getPtPairs(I16, qq, startindex=60, max_dist_match2=maxd2)
        assert np.array_equal(got["idx"], want[60:]) and np.array_equal(got["p2"], qq[60:][want[60:] >= 0])
    _check_sums(got, pts, I16, 0, "octree getPtPairs, " + name)
    if name == "octants":          # the k-d tree breaks these ties differently: the test above would not hold here
        assert not np.array_equal(tdtk.KDtree(pts).getPtPairs(I16, qq, max_dist_match2=maxd2)["idx"], got["idx"])


def test_five_iteration_icp_by_hand_equals_the_kdtree_loop(tdtk, gpu):
    """getPtPairs, the minimizer's Align, the transform -- five times, on the bundled pair: the pair list of every iteration
    equals the same loop's on the KDtree"""
    model, data = dat_pair()
    mini = tdtk.icp6D_QUAT(True)
    lists = {}
    for tag, tree in (("octree", tdtk.BOctTree(model)), ("kd", tdtk.KDtree(model))):
        cur, out = data.copy(), []
        for it in range(5):
            r = tree.getPtPairs(I16, cur, max_dist_match2=625.0)
            rms, A = mini.Align_Parallel(r)
            assert rms >= 0
            out.append((r["idx"], r["p1"], r["p2"], A))
            cur = move(cur, A)
        lists[tag] = out
    for it, (a, b) in enumerate(zip(lists["octree"], lists["kd"])):
        assert np.array_equal(a[0], b[0]) and len(a[1]) == len(b[1]), it        # the same pairs, query for query
        # (the two loops' sums come from different kernels -- the k-d pass adds its base sums up inside the search --, so the
        #  poses agree to rounding, not by bits; p1 is the same model point moved by the identity)
        assert np.array_equal(a[1], b[1]) and np.allclose(a[2], b[2], rtol=0, atol=1e-6) and np.allclose(a[3], b[3], rtol=0, atol=1e-9), it
    assert not np.array_equal(lists["kd"][0][0], lists["kd"][4][0])         # the loop moved the scan


def test_from_scan(tdtk, gpu, fx):
    """the tree over a resident scan's points answers in the scan's caller order"""
    pts = fx.cloud("uniform")
    qq, maxd2 = fx.batches("uniform", 10.0, 1)[0][:2]
    h = C.c_void_p()
    dp = C.POINTER(C.c_double)
    assert tdtk.lib().tdtk_scan_create(pts.ctypes.data_as(dp), None, len(pts), 0, C.byref(h)) == 0
    try:
        a, b = tdtk.BOctTree.from_scan(h, len(pts)), tdtk.BOctTree(pts)
        assert np.array_equal(a.leaf_order(), b.leaf_order())
        ra, rb = a.FindClosestBatch(qq, maxd2), b.FindClosestBatch(qq, maxd2)
        assert np.array_equal(ra[0], rb[0]) and bm.same_bits(ra[1], rb[1])
    finally:
        tdtk.lib().tdtk_scan_destroy(h)
