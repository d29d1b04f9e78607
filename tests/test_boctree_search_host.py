"""The octree search tree (tdtk_octree_*): the CPU tier.  The walk the device runs (3dtk_amd/csrc/oct_lane.h, compiled for the
host under tests/host_oct_shim.h) over a node table built by a plain Python restatement of the reference's constructor
(tests/boctree_model.py), against tests/golden/k20_boctree_search.npz -- what the reference's own compiled BOctTree<double>
returned: init()'s scalars, the counts, the leaf order, and per query the returned point, its Dist2 and the number of leaves
scanned, all by bits.  Where the reference checkout is present the fixture is generated again and compared."""
import ctypes as C
import os

import numpy as np
import pytest

import boctree_model as bm
import host_lane

gen = bm.generator()
CASES = [(name, voxel, early) for name, variants in gen.CASES for voxel, early in variants]


@pytest.fixture(scope="module")
def fx():
    return gen.load()


@pytest.fixture(scope="module")
def lane(tmp_path_factory):
    return bm.host_lane(tmp_path_factory.mktemp("oct_host"))


def _model(fx, name, voxel, early):
    return bm.model_of(fx, name, voxel, early)


def test_fixture_is_what_the_generator_says(fx):
    """under the size bound; the clouds and queries are the generator's; the cases and nothing else"""
    assert os.path.getsize(gen.OUT) <= gen.MAX_BYTES
    c = gen.clouds()
    q = gen.queries(c)
    for name, variants in gen.CASES:
        assert bm.same_bits(fx.cloud(name), c[name]), name
        for voxel, early in variants:
            got = fx.batches(name, voxel, early)
            assert len(got) == len(q[name])
            for (qq, maxd2, pos, d2, leaves), (want_q, want_m) in zip(got, q[name]):
                assert bm.same_bits(qq, want_q) and maxd2 == want_m and len(pos) == len(d2) == len(leaves) == len(qq)
    assert len(c["limit"]) <= 12000 and max(len(v) for v in c.values()) == len(c["limit"])


@pytest.mark.parametrize("name,voxel,early", CASES)
def test_model_equals_fixture(fx, name, voxel, early):
    """the restatement's tree is the reference's: init()'s scalars by bits, countNodes / countOctLeaves / countPoints, the
    full leaf order"""
    bm.check_model_equals_fixture(fx, _model(fx, name, voxel, early), name, voxel, early)


@pytest.mark.parametrize("name,voxel,early", CASES)
def test_host_lane_equals_fixture(fx, lane, name, voxel, early):
    """FindClosest of every query of every batch: the returned point (as the first position in leaf order with its
    coordinates: what strict < returns), Dist2 and the leaves scanned, by bits; no case and no query left out"""
    m = _model(fx, name, voxel, early)
    n = bm.check_lane_equals_batches(lane, m, fx, name, voxel, early)
    if (name, voxel, early) in set(gen.EDGE_CASES):
        for q1, maxd2, pos, d2, leaves in fx.edge(name, voxel, early):          # maxdist2 == d2 and one ulp above, per query
            slot, gd2, gl = bm.lane_find(lane, m, q1[None], maxd2)
            assert (int(slot[0]), int(gl[0])) == (pos, leaves) and bm.same_bits(gd2, [d2]), (name, q1, maxd2)
            n += 1
    assert n > 0


def test_order_table_equals_the_recorded_visits(fx, lane):
    """OCT_ORDER (oct_lane.h) against the order in which the reference scanned the eight children, per octant"""
    got = np.empty((8, 8), np.int32)
    for o in range(8):
        row = np.empty(8, np.int32)
        lane.oct_host_order(o, row.ctypes.data)
        got[o] = row
    assert np.array_equal(got, fx.visits)
    assert (np.sort(got, 1) == np.arange(8)).all() and (got[:, 0] == np.arange(8)).all()


def test_leaf_limit_and_stopped_search_in_the_lane(fx, lane):
    """the two answers that are not the nearest point: 10 000 leaves scanned and nothing returned although the partner is
    inside the radius; a point within 0.01 returned although a nearer one exists"""
    m = _model(fx, "limit", 1.0, 0)
    qq, maxd2 = fx.batches("limit", 1.0, 0)[0][:2]
    slot, d2, leaves = bm.lane_find(lane, m, qq, maxd2)
    pts = fx.cloud("limit")
    assert leaves[0] == 10000 and slot[0] == -1 and ((pts - qq[0]) ** 2).sum(1).min() < maxd2
    assert slot[1] >= 0 and m.leaf[slot[1]] == 2
    m = _model(fx, "stop", 10.0, 1)
    qq, maxd2 = fx.batches("stop", 10.0, 1)[0][:2]
    slot, d2, _ = bm.lane_find(lane, m, qq[:1], maxd2)
    assert 0.0 < d2[0] <= 0.0001 and ((fx.cloud("stop") - qq[0]) ** 2).sum(1).min() < d2[0]


def test_out_of_range_batches_are_refused(fx, lane):
    """where sqrt(maxdist2) * mult + 1 or a voxel coordinate leaves +-2^30 the reference's int conversion is undefined"""
    m = _model(fx, "two", 0.1, 0)
    ok = np.zeros((1, 3))
    assert bm.lane_find(lane, m, ok, 625.0) is not None
    limit = 2.0 ** 30 / m.mult
    assert bm.lane_find(lane, m, ok, (limit * 1.01) ** 2) is None and bm.lane_find(lane, m, ok, (limit * 0.5) ** 2) is not None
    assert bm.lane_find(lane, m, ok, -1.0) is None and bm.lane_find(lane, m, ok, np.nan) is None
    assert bm.lane_find(lane, m, [[0.0, limit * 1.01, 0.0]], 625.0) is None
    assert bm.lane_find(lane, m, [[0.0, 0.0, -limit * 1.01]], 625.0) is None
    assert bm.lane_find(lane, m, [[np.nan, 0.0, 0.0]], 625.0) is None


def test_octree_kernels_spill_nothing_and_the_entry_points_are_declared():
    """the compiler's resource remarks (csrc/Makefile keeps them): no kernel of octree.hip spills or uses scratch, and the
    search kernel leaves room for at least four waves per SIMD; every tdtk_octree_* symbol is in the header and the binding"""
    import re
    from importlib import import_module
    path = os.path.join(bm.ROOT, "3dtk_amd", "csrc", "octree.resource.txt")
    if not os.path.exists(path):
        pytest.skip("no build in this tree (octree.resource.txt is written by the Makefile)")
    blocks = {b.split()[0]: b for b in open(path).read().split("remark: Function Name: ")[1:]}
    for want in ("k_oct_find", "k_oct_prepare", "k_oct_leaf_depth", "k_oct_level_flags", "k_oct_level_emit", "k_oct_points"):
        assert any(want in n for n in blocks), want
    for name, b in blocks.items():
        for key in ("VGPRs Spill", "SGPRs Spill", r"ScratchSize \[bytes/lane\]"):
            m = re.search(key + r": (\d+)", b)
            assert m and int(m.group(1)) == 0, (name, key)
    find = [b for n, b in blocks.items() if "k_oct_find" in n][0]
    assert int(re.search(r"VGPRs: (\d+)", find).group(1)) <= 128 and int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", find).group(1)) >= 4
    capi = import_module("3dtk_amd._capi")
    hdr = open(os.path.join(bm.ROOT, "include", "tdtk_hip.h")).read()
    syms = [s for s in capi.EXPORTS if s.startswith("tdtk_octree_")]
    assert len(syms) == 9
    for sym in syms:
        assert re.search(r"\b(int|void) %s\(" % sym, hdr), sym
    assert sorted(set(re.findall(r"\b(tdtk_octree_\w+)\(", hdr))) == sorted(syms)


def test_fixture_equals_the_reference():
    """the generator, run again on the live reference, gives the stored arrays"""
    if not gen.have_ref():
        pytest.skip("no reference checkout (src/slam6d/Boctree.cc)")
    z = np.load(gen.OUT)
    got = gen.compute()
    assert sorted(got) == sorted(z.files)
    for k in z.files:
        assert got[k].dtype == z[k].dtype and got[k].shape == z[k].shape, k
        same = bm.same_bits(got[k], z[k]) if got[k].dtype == np.float64 else np.array_equal(got[k], z[k])
        assert same, k


# ---- the bundled scan pair of the GPU tier's ICP-by-hand test ---------------------------------------------------------------
KNN2 = r"""
extern "C" void hq_two_nearest(void* p, const double* q, int nq, int* idx, double* d2) {
  HostTree& T = *(HostTree*)p;
  QueryArgs a = host_args(T);
  std::vector<double> ld(KNN_MAX_K); std::vector<uint32_t> ls(KNN_MAX_K);
  for (int i = 0; i < nq; i++) {
    ListLds<1> L; L.ld = ld.data(); L.ls = ls.data(); L.init(2);
    HostStack st;
    knn_walk(a, q[3 * i], q[3 * i + 1], q[3 * i + 2], L, st);
    for (int j = 0; j < 2; j++) { idx[2 * i + j] = L.dist(j) >= 0.0 ? a.pts[L.slot(j)].orig : -1; d2[2 * i + j] = L.dist(j); }
  }
}
"""


def test_dat_pair_is_tie_free_along_an_icp(lane, tmp_path):
    """What the GPU tier's five-iteration ICP by hand relies on when it asks the octree's pair lists to equal the k-d tree's:
    on the bundled pair, along five iterations of a closest-point ICP at maxdist2 625, every query's nearest model point is
    unique, none lies within 0.01 (no stopped search), no search comes near the leaf limit -- and the octree walk returns
    exactly that point.  (The poses here come from an SVD on the host; the device loop's differ in the last bits.)"""
    model, cur = bm.dat_pair()
    L = host_lane.build(KNN2, tmp_path, "knn2")
    L.hq_two_nearest.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    T = L.host_tree_create(model.ctypes.data, len(model), 20)
    m = bm.Model(model, 10.0, True)
    try:
        for it in range(5):
            idx, d2 = np.empty((len(cur), 2), np.int32), np.empty((len(cur), 2))
            L.hq_two_nearest(C.c_void_p(T), cur.ctypes.data, len(cur), idx.ctypes.data, d2.ctypes.data)
            hit = d2[:, 0] < 625.0
            assert hit.sum() > 0.5 * len(cur)
            assert (d2[hit, 0] < d2[hit, 1]).all() and (d2[hit, 0] > 0.0001).all(), it
            assert not (d2[~hit, 0] == 625.0).any()
            slot, od2, leaves = bm.lane_find(lane, m, cur, 625.0)
            assert np.array_equal(np.where(slot >= 0, m.leaf[np.maximum(slot, 0)], -1), np.where(hit, idx[:, 0], -1)), it
            assert bm.same_bits(od2[hit], d2[hit, 0]) and leaves.max() < 5000
            cur = bm.move(cur, bm.horn(model[idx[hit, 0]], cur[hit]))
    finally:
        L.host_tree_destroy(C.c_void_p(T))

