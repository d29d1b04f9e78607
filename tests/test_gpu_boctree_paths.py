"""The octree search tree on the device (tdtk_octree_*, tdtk_icp_match_octree) on the paths tests/test_gpu_boctree.py and
tests/test_gpu_boctree_icp.py do not reach: tests/golden/k22_boctree_paths.npz (the reference's own compiled BOctTree<double>
on tiny clouds, runs of 10 and 11 at both ends of the sorted keys, heavy duplicate groups, a planar cloud, a searched 21-level
tree); trees, query batches and a resident ICP loop above the build and prepare kernels' grid cap of 4096 x 256 threads, so
that their grid-stride loops take a second trip; batch sizes around the search block; a refusal in the middle of a loop;
from_scan on a moved scan; getPtPairs for every `want`; the refusal bound itself.  Everything is compared by bits or by exact
integers against the host build of the walk over the restatement's table (tests/boctree_model.py, which the CPU tier ties to
the reference); the pair sums alone use the tolerance tests/pair_sums_ref.py derives."""
import ctypes as C

import numpy as np
import pytest

import boctree_icp_run as icp
import boctree_model as bm
import pair_sums_ref as R

pytestmark = pytest.mark.gpu

gen = bm.load_generator("make_golden_boctree_paths")
gen20 = bm.generator()
CASES = [(name, voxel, early) for name, variants in gen.CASES for voxel, early in variants]
I16 = np.eye(4).reshape(16)
CAP = 4096 * 256                 # threads of the largest launch of oct_grid (octree.hip) and of reduce.hip's twin
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)
LUM_D = [0.02, -0.01, 0.015, 1e-4, -2e-4, 1.5e-4]


@pytest.fixture(scope="module")
def fx():
    return gen.load()


@pytest.fixture(scope="module")
def fx20():
    return gen20.load()


@pytest.fixture(scope="module")
def lane(tmp_path_factory):
    return bm.host_lane(tmp_path_factory.mktemp("oct_host"))


@pytest.fixture(scope="module")
def uniform(fx20, lane):
    """k20's `uniform` cloud (3000 points) and its restatement at the default voxel 10, earlystop on"""
    return fx20.cloud("uniform"), bm.model_of(fx20, "uniform", 10.0, 1)


def _tree_equals_model(t, m):
    """info() by bits, the counts, leaf_order() and node_table() equal the restatement's"""
    info = t.info()
    assert bm.same_bits(bm.info_scalars(info), m.scalars)
    assert [info["n_nodes"], info["n_leaves"], info["n_points"]] == [m.n_nodes, m.n_leaves, len(m.leaf)]
    assert np.array_equal(t.leaf_order(), m.leaf)
    assert np.array_equal(t.node_table(), m.nodes)


def _walk_idx(lane, m, q, maxd2):
    """the host walk's answer as the device states it: the caller's index of the point (or -1), and Dist2"""
    slot, d2, _ = bm.lane_find(lane, m, q, maxd2)
    return bm.expect_idx(m.leaf, slot), d2


# ---- the second fixture ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,voxel,early", CASES)
def test_tree_and_find_closest_equal_the_reference(tdtk, gpu, fx, name, voxel, early):
    """info() by bits, the counts, the leaf order, the node table slot for slot; FindClosestBatch on every batch: index and
    Dist2 by bits, nothing skipped"""
    pts = fx.cloud(name)
    t = tdtk.BOctTree(pts, voxel, bool(early))
    info = t.info()
    assert bm.same_bits(bm.info_scalars(info), fx.get(name, voxel, early, "scalars"))
    assert [info["n_nodes"], info["n_leaves"], info["n_points"]] == [int(v) for v in fx.get(name, voxel, early, "counts")]
    order = t.leaf_order()
    assert bm.same_bits(pts[order], pts[fx.get(name, voxel, early, "leaf")])
    assert np.array_equal(np.sort(order), np.arange(len(pts)))
    assert np.array_equal(t.node_table(), bm.model_of(fx, name, voxel, early).nodes)
    for qq, maxd2, pos, d2, _ in fx.batches(name, voxel, early):
        idx, gd2 = t.FindClosestBatch(qq, maxd2)
        # (a group of identical points: the fixture names the first position with the coordinates, the device the point it
        #  met first -- the same position, since strict < keeps the first)
        want = bm.expect_idx(order, pos)
        assert np.array_equal(idx, want), (name, voxel, early, maxd2, np.flatnonzero(idx != want)[:5])
        assert bm.same_bits(gd2, d2)


# ---- above the grid cap ------------------------------------------------------------------------------------------------------
BIG_N = CAP + 700
BIG_VOXEL = 10.0


BIG_CLUSTERS = ((9, (200.0, 200.0, 200.0), 1.0 / 32), (10, (240.0, 200.0, 200.0), 1.0 / 32), (11, (191.0, 240.0, 191.0), 16.0),
                (12, (240.0, 240.0, 191.0), 16.0), (10, (200.0, 200.0, 240.0), 1.0 / 32), (11, (240.0, 191.0, 240.0), 16.0))


def _big_cloud():
    """the block, and behind it in key order six clusters, each in a depth-3 cell of its own: those of 9 and 10 points small
    (an early-stop leaf each), those of 11 and 12 points 16 wide, across a cut of the last level"""
    rng = np.random.default_rng(23)
    pts = rng.uniform(-50.0, 50.0, (BIG_N, 3))
    tail = np.concatenate([np.array(base) + scale * rng.integers(0, 64, (cnt, 3)) / 64.0 for cnt, base, scale in BIG_CLUSTERS])
    assert len(tail) == 63
    pts[-63:] = tail
    q = np.concatenate([rng.uniform(-52.0, 52.0, (2048, 3)), tail[rng.integers(0, 63, 2048)] + rng.uniform(-1.0, 1.5, (2048, 3))])
    return pts, q


def test_build_above_the_grid_cap(tdtk, gpu, lane):
    """1 048 576 + 700 points: every build kernel takes the second trip of its grid-stride loop.  Six clusters fall last in
    key order, so the leaves behind position 1 048 576 include theirs: the clusters of 9 and 10 points are early-stop leaves
    above the full depth, those of 11 and 12 points are split at the full depth.  Node table, leaf order and info() equal the
    restatement's; 4096 queries, half around the block and half around the clusters, equal the host walk by bits"""
    pts, q = _big_cloud()
    m = bm.Model(pts, BIG_VOXEL, True)
    assert (np.sort(m.leaf[-63:]) == np.arange(BIG_N - 63, BIG_N)).all()                   # the clusters: last in key order
    lv = [x for x in gen.leaves_of(m) if x[0] >= BIG_N - 63]
    full = m.max_depth - 1
    assert lv[0][0] == BIG_N - 63 >= CAP and sum(k for _, k, _ in lv) == 63
    early = sorted(k for _, k, d in lv if d < full)
    assert early == [9, 10, 10] and all(k <= 12 for _, k, _ in lv) and len(lv) > 6           # 11 and 12: split, at full depth
    for cnt, base, scale in BIG_CLUSTERS:
        mine = [(a, k, d) for a, k, d in lv if ((pts[m.leaf[a:a + k]] >= base) & (pts[m.leaf[a:a + k]] < np.array(base) + scale)).all()]
        assert sum(k for _, k, _ in mine) == cnt and (len(mine) == 1) == (cnt <= 10), (cnt, mine)
    t = tdtk.BOctTree(pts, BIG_VOXEL, True)
    _tree_equals_model(t, m)
    want_idx, want_d2 = _walk_idx(lane, m, q, 4.0)
    assert (want_idx[:2048] >= 0).mean() > 0.5 and (want_idx[2048:] >= BIG_N - 63).sum() > 500 and (want_idx[2048:] == -1).any()
    idx, d2 = t.FindClosestBatch(q, 4.0)
    assert np.array_equal(idx, want_idx) and bm.same_bits(d2, want_d2)


def test_queries_above_the_grid_cap(tdtk, gpu, uniform, lane):
    """1 048 576 + 300 grid queries on the `uniform` tree at maxdist2 4: k_oct_prepare's second trip, through FindClosestBatch
    and through getPtPairs under a source_alignxf that is not the identity (a quarter turn about z and a shift on the grid:
    its inverse is exact, so the walk sees the same coordinates)"""
    pts, m = uniform
    K = CAP + 300
    q = np.random.default_rng(24).integers(-55 * 16, 55 * 16, (K, 3)) / 16.0
    want_idx, want_d2 = _walk_idx(lane, m, q, 4.0)
    assert 0.02 * K < (want_idx >= 0).sum() < 0.98 * K
    t = tdtk.BOctTree(pts)
    idx, d2 = t.FindClosestBatch(q, 4.0)
    assert np.array_equal(idx, want_idx) and bm.same_bits(d2, want_d2)
    A = np.array([0.0, 1.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 3.0, -2.0, 5.0, 1.0])       # column-major
    moved = bm.move(q, A)
    back = np.stack([moved[:, 1] + 2.0, -(moved[:, 0] - 3.0), moved[:, 2] - 5.0], 1)
    assert np.array_equal(back, q)                     # exact on this grid: nothing is rounded on the way there and back
    got = t.getPtPairs(A, moved, max_dist_match2=4.0, want_pairs=False)
    assert np.array_equal(got["idx"], want_idx) and got["n"] == (want_idx >= 0).sum()


@pytest.mark.parametrize("K", [0, 1, 127, 128, 129, 255, 256, 257])
def test_batch_sizes_around_the_block(tdtk, gpu, uniform, fx20, lane, K):
    """K on both sides of the search block (128) and of the prepare block (256): the same prefix of one reference answer;
    K == 0 returns 0 and writes nothing"""
    pts, m = uniform
    qq, maxd2 = fx20.batches("uniform", 10.0, 1)[0][:2]
    qq = np.concatenate([qq, qq[::-1] + 0.5])[:257]
    assert len(qq) == 257
    want_idx, want_d2 = _walk_idx(lane, m, qq, maxd2)
    t = tdtk.BOctTree(pts)
    idx, d2 = np.full(257, -7, np.int32), np.full(257, -7.0)
    q = np.ascontiguousarray(qq[:K])
    assert tdtk.lib().tdtk_octree_find_closest(t._h, q.ctypes.data_as(DP), K, maxd2, idx.ctypes.data_as(IP), d2.ctypes.data_as(DP)) == 0
    assert np.array_equal(idx[:K], want_idx[:K]) and bm.same_bits(d2[:K], want_d2[:K])
    assert (idx[K:] == -7).all() and (d2[K:] == -7.0).all()
    if K == 0:
        assert tdtk.lib().tdtk_octree_find_closest(t._h, None, 0, maxd2, None, None) == 0


def test_resident_loop_above_the_grid_cap(tdtk, gpu, uniform, lane):
    """1 048 576 + 300 scan points, 3 iterations: k_oct_loop_prepare moves the scan in place on the second trip of its loop
    too.  Resident against stepped as on the seam (the scan by bits against a copy moved with tdtk_scan_transform); the pairs of
    iteration 0 are the host walk's"""
    model, m = uniform
    rng = np.random.default_rng(25)
    N = CAP + 300
    data = bm.move(model[np.arange(N) % len(model)] + rng.uniform(-0.25, 0.25, (N, 3)), R.rigid([0.3, -0.2, 0.25], [0.002, -0.003, 0.0025]))
    last = icp.resident_against_stepped(tdtk, model, data, 25.0, 3)
    slot, _, _ = bm.lane_find(lane, m, data, 25.0)
    assert last["trace"][0, 0] == (slot >= 0).sum() > 0.9 * N


# ---- a refusal in the middle of a loop -----------------------------------------------------------------------------------------
def test_refusal_in_mid_loop_leaves_the_completed_iterations(tdtk, gpu, lane, fx20):
    """A scan whose outlier is in range at iteration 0 and is carried across the limit by iteration 0's alignxf: iteration 1
    is refused after k_oct_loop_prepare has moved the scan.  rc, res->iterations and the message; data_transMat and
    data_dalignxf are row 0's alignxf; the scan is, by bits, a copy moved once by tdtk_scan_transform with it; a k-d loop
    afterwards gives its usual trace"""
    rng = np.random.default_rng(5)
    cloud = rng.uniform(-5.0, 5.0, (300, 3))
    m = bm.Model(cloud, 1e-5, True)
    limit = 2.0 ** 30 / m.mult
    near = cloud[:200] + [0.3, 0.0, 0.0]
    outlier = np.array([[-limit - m.add[0] + 0.15, 0.0, 0.0]])
    data = np.concatenate([near, outlier])
    # the step, predicted on the CPU: the host walk's pairs, an SVD
    slot, _, _ = bm.lane_find(lane, m, data, 25.0)
    assert (slot[:200] >= 0).all() and slot[200] == -1
    A0 = bm.horn(cloud[m.leaf[slot[:200]]], near)
    vox = lambda p: (p + m.add) * m.mult                                                       # noqa: E731
    assert np.abs(vox(data)).max() < 2.0 ** 30 - 1e4 and vox(bm.move(data, A0))[200, 0] < -(2.0 ** 30) - 1e4
    assert np.abs(vox(bm.move(data, A0))[:200]).max() < 2.0 ** 29
    assert bm.lane_find(lane, m, bm.move(data, A0), 25.0) is None
    kd_prev = icp.model_scan(tdtk, cloud, 0)
    first = icp.run(tdtk, kd_prev, near, None, 1, 0, 25.0, 6, 0.0)
    fine = tdtk.BOctTree(cloud, 1e-5, True)
    cur = tdtk.Scan(icp.Z3, icp.Z3, data)
    rc, res, tm, da, trace = icp.c_match(tdtk, "tdtk_icp_match_octree", fine._h, cur.handle, 1, 0, 5, 25.0)
    assert rc == -5 and res.iterations == 1 and b"does not fit +-2^30" in tdtk.lib().tdtk_last_error()
    assert trace[0, 0] == 200 and np.allclose(trace[0, 2:], A0, rtol=0, atol=1e-9) and not trace[1:].any()
    row0 = np.ascontiguousarray(trace[0, 2:])
    assert np.array_equal(tm, row0) and np.array_equal(da, row0)
    copy = tdtk.Scan(icp.Z3, icp.Z3, data)
    assert tdtk.lib().tdtk_scan_transform(copy.handle, row0.ctypes.data_as(DP)) == 0
    assert bm.same_bits(cur.get_xyz_reduced(), copy.get_xyz_reduced())
    again = icp.run(tdtk, kd_prev, near, None, 1, 0, 25.0, 6, 0.0)
    # (the same k-d loop on the same input, both times from a cold start: the association of its sums is fixed, so by bits)
    assert first[0] == again[0] and bm.same_bits(first[1]["trace"], again[1]["trace"])


# ---- from_scan on a scan that has moved ------------------------------------------------------------------------------------------
def test_from_scan_after_a_move_is_the_tree_of_the_original(tdtk, gpu, uniform):
    """tdtk_scan_mark_original, tdtk_scan_transform, then BOctTree.from_scan: the tree of the saved points"""
    pts, m = uniform
    h = C.c_void_p()
    assert tdtk.lib().tdtk_scan_create(pts.ctypes.data_as(DP), None, len(pts), 0, C.byref(h)) == 0
    try:
        assert tdtk.lib().tdtk_scan_mark_original(h) == 0
        A = np.ascontiguousarray(R.rigid([30.0, -20.0, 50.0], [0.1, -0.2, 0.15]))
        assert tdtk.lib().tdtk_scan_transform(h, A.ctypes.data_as(DP)) == 0
        now = np.empty_like(pts)
        assert tdtk.lib().tdtk_scan_download(h, now.ctypes.data_as(DP), None) == 0
        assert np.abs(now - pts).max() > 10.0                          # it did move
        _tree_equals_model(tdtk.BOctTree.from_scan(h, len(pts)), m)
    finally:
        tdtk.lib().tdtk_scan_destroy(h)


# ---- getPtPairs: every want --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dat_trees(tdtk, gpu):
    """the bundled tie-free pair: the model's octree and k-d tree; for the sums every twentieth query and its normals (a subset
    on which pair_sums_ref's discrimination holds for every want: one pair less moves each quantity by more than 600
    tolerances, where the whole scan reaches the required 10 only for some); for the pair lists the whole scan and normals"""
    model, data = bm.dat_pair()
    q = np.ascontiguousarray(data[::20])
    nr = np.random.default_rng(26).normal(size=q.shape)
    return model, q, nr, tdtk.BOctTree(model), tdtk.KDtree(model), np.ascontiguousarray(data), np.random.default_rng(27).normal(size=data.shape)


@pytest.mark.parametrize("want", list(range(8)) + [R.WANT_GAPX, R.WANT_MOM2, "lum_D"])
def test_get_pt_pairs_for_every_want(tdtk, dat_trees, want):
    """idx, p1, p2 (and the normals where there are any) equal KDtree.getPtPairs's, on the whole scan and on the subset; on
    the subset the sums inside pair_sums_ref's derived tolerance; a want that needs normals is refused without them"""
    model, q, nr, oc, kd, whole, whole_nr = dat_trees
    D = LUM_D if want == "lum_D" else None
    want = R.WANT_LUM if want == "lum_D" else want
    needs_n = bool(want & R.WANT_NAPX)
    if needs_n:
        with pytest.raises(tdtk.TdtkError) as e:
            oc.getPtPairs(I16, q, want=want)
        assert e.value.code == -1
    kw = dict(normal_r=whole_nr if needs_n else None, max_dist_match2=625.0, want=want, lum_D=D)
    a, b = oc.getPtPairs(I16, whole, **kw), kd.getPtPairs(I16, whole, **kw)
    assert a["n"] == b["n"] > 0.5 * len(whole) and np.array_equal(a["idx"], b["idx"])
    assert np.array_equal(a["p1"], b["p1"]) and np.array_equal(a["p2"], b["p2"]) and np.array_equal(a["pn"], b["pn"])
    kw = dict(normal_r=nr if needs_n else None, max_dist_match2=625.0, want=want, lum_D=D)
    a, b = oc.getPtPairs(I16, q, **kw), kd.getPtPairs(I16, q, **kw)
    assert a["n"] == b["n"] > 0.5 * len(q) and np.array_equal(a["idx"], b["idx"])
    assert np.array_equal(a["p1"], b["p1"]) and np.array_equal(a["p2"], b["p2"]) and np.array_equal(a["pn"], b["pn"])
    unit = R.unit_normals(nr[a["idx"] >= 0]) if needs_n else None
    if needs_n:
        assert np.array_equal(a["pn"], unit)
    bm.check_sums(a, model, I16, want, "octree getPtPairs, want %s%s" % (want, ", lum_D" if D else ""), unit, D)


# ---- the bound on the device ---------------------------------------------------------------------------------------------------
def test_the_bound_on_the_device(tdtk, gpu, lane):
    """|v| == 2^30 exactly -- a radius, a coordinate, both -- is refused with TDTK_EUNSUP and nothing written; the largest
    admitted values (x + closest_v == 2^31 - 2) return the host walk's answer by bits"""
    m = bm.bound_tree()
    t = tdtk.BOctTree(np.array([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]]), 0.1, False)
    _tree_equals_model(t, m)
    for tag, q, maxd2, admitted in bm.bound_cases(m):
        q = np.ascontiguousarray(q)
        idx, d2 = np.full(len(q), -7, np.int32), np.full(len(q), -7.0)
        rc = tdtk.lib().tdtk_octree_find_closest(t._h, q.ctypes.data_as(DP), len(q), maxd2, idx.ctypes.data_as(IP), d2.ctypes.data_as(DP))
        if admitted:
            want_idx, want_d2 = _walk_idx(lane, m, q, maxd2)
            assert rc == 0 and np.array_equal(idx, want_idx) and bm.same_bits(d2, want_d2), tag
        else:
            assert rc == -5 and (idx == -7).all() and (d2 == -7.0).all(), tag
            assert bm.lane_find(lane, m, q, maxd2) is None, tag
