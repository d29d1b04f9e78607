"""icp6D::match on the octree search tree on the device (tdtk_icp_match_octree, icp6D.match on a scan with
setSearchTreeParameter(2)) against tests/golden/k21_boctree_icp.npz -- the loop as the reference's own compiled
BOctTree<double>::FindClosest drives it --, against the host-stepped loop over BOctTree.getPtPairs, and against the k-d loop
where the two trees must agree (the bundled pair, which tests/test_boctree_search_host.py shows to be tie-free) and where they
must not (the seam)."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import boctree_model as bm
from boctree_icp_run import POSE_ATOL, Z3
from boctree_icp_run import c_match as _c_match, model_scan as _model_scan, resident_against_stepped as _resident_against_stepped, run as _run
from boctree_model import dat_pair

pytestmark = pytest.mark.gpu


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_boctree_icp", os.path.join(bm.G, "make_golden_boctree_icp.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


gen = _generator()
RUN_IDS = [gen.prefix(r).rstrip("_") for r in gen.RUNS]


@pytest.fixture(scope="module")
def fx():
    return gen.load()


@pytest.fixture
def hashes(tdtk):
    """tdtk_icp_index_hashes on for the test"""
    was = tdtk.lib().tdtk_icp_index_hashes(1)
    yield True
    tdtk.lib().tdtk_icp_index_hashes(was)


@pytest.mark.parametrize("run", gen.RUNS, ids=RUN_IDS)
def test_every_fixture_run(tdtk, gpu, fx, hashes, run):
    """iterations, converged, the pairs and the index hash of every pass equal the fixture exactly -- the hash from the
    fixture's positions in leaf order through the device tree's own leaf order, so exact duplicates leave nothing out --;
    rms and alignxf within the pose bound.  On the seam the k-d loop's correspondences differ from iteration 2 on."""
    name, voxel, early, algo, mode, maxd2, iters, eps, _ = run
    model, data, normals = gen.cloud_of(fx, name)
    p = gen.prefix(run)
    prev = _model_scan(tdtk, model, 2, voxel, early)
    assert isinstance(prev.getSearchTree(), tdtk.BOctTree)
    need_n = mode != 0 or algo == gen.NAPX
    it, last, cur = _run(tdtk, prev, data, normals if need_n else None, algo, mode, maxd2, iters, eps)
    rows = len(fx[p + "rms"])
    print(p, "iterations", it, "pairs", last["trace"][:rows, 0], "rms", last["trace"][:rows, 1])
    print(p, "max |rms - fixture|", np.abs(last["trace"][:rows, 1] - fx[p + "rms"]).max() if rows else 0.0,
          "max |xf - fixture|", np.abs(last["trace"][:rows, 2:] - fx[p + "xf"]).max() if rows else 0.0)
    assert it == int(fx[p + "iterations"]) and last["converged"] == bool(fx[p + "converged"])
    assert last["pairs"] == int(fx[p + "pairs"][-1])
    assert np.array_equal(last["trace"][:rows, 0], fx[p + "pairs"][:rows])
    order = prev.getSearchTree().leaf_order()
    pos = fx[p + "pos"]
    want_idx = np.where(pos >= 0, order[np.maximum(pos, 0)], -1)
    assert last["index_hashes"] == [int(gen.k5_hash(r)) for r in want_idx]
    # (the fixture's own hash names a point by the smallest row with its coordinates: the same test where no two rows are equal)
    rep = gen.mo.rep_index(model, model[order])
    assert [int(gen.k5_hash(np.where(r >= 0, rep[np.maximum(r, 0)], -1))) for r in pos] == [int(h) for h in fx[p + "hash"]]
    assert np.allclose(last["trace"][:rows, 1], fx[p + "rms"], rtol=0, atol=POSE_ATOL)
    assert np.allclose(last["trace"][:rows, 2:], fx[p + "xf"], rtol=0, atol=POSE_ATOL)
    if name == "seam" and algo != gen.NAPX:
        kit, klast, _ = _run(tdtk, _model_scan(tdtk, model, 0), data, None, algo, mode, maxd2, iters, eps)
        assert len(klast["index_hashes"]) >= 3
        assert all(a != b for a, b in zip(klast["index_hashes"][2:], last["index_hashes"][2:]))


def test_resident_loop_equals_the_stepped_loop_on_the_seam(tdtk, gpu, fx, hashes):
    model, data, _ = gen.cloud_of(fx, "seam")
    _resident_against_stepped(tdtk, model, data, gen.SEAM_MAXD2, gen.SEAM_ITERS)


def test_resident_loop_on_the_bundled_pair_equals_stepped_and_the_kd_loop(tdtk, gpu, hashes):
    """81 360 points, 5 iterations at maxdist2 625: resident against stepped as on the seam; the pair is tie-free, so the
    five index hashes are the k-d loop's"""
    model, data = dat_pair()
    last = _resident_against_stepped(tdtk, model, data, 625.0, 5)
    kit, klast, _ = _run(tdtk, _model_scan(tdtk, model, 0), data, None, 1, 0, 625.0, 5, 0.0)
    assert len(last["index_hashes"]) == 5 and last["index_hashes"] == klast["index_hashes"]
    assert np.array_equal(last["trace"][:, 0], klast["trace"][:, 0])


def test_rnd_resident_equals_stepped(tdtk, gpu, fx):
    """-R 3 with srand(11) before each run: the same draws, the same pairs in every iteration, under half the points drawn"""
    model, data, _ = gen.cloud_of(fx, "seam")
    prev = _model_scan(tdtk, model, 2)
    it, last, _ = _run(tdtk, prev, data, None, 1, 0, gen.SEAM_MAXD2, 6, 0.0, rnd=3)
    sit, slast, _ = _run(tdtk, prev, data, None, 1, 0, gen.SEAM_MAXD2, 6, 0.0, rnd=3, stepped=True)
    assert it == sit == 5
    assert np.array_equal(last["trace"][:, 0], slast["trace"][:, 0])
    assert (last["trace"][:, 0] < len(data) / 2).all() and (last["trace"][:, 0] > 3).all()
    assert len(set(last["trace"][:, 0])) > 1                                  # a fresh draw per iteration
    assert np.allclose(last["trace"][:, 2:], slast["trace"][:, 2:], rtol=0, atol=POSE_ATOL)


def test_refusals(tdtk, gpu, fx):
    """pairing mode 1; a radius and a query whose voxel coordinate leaves +-2^30; N == 0 and max_num_iterations == 0 as the
    k-d form; nothing moved by a refused call"""
    model = fx["two_model"]
    data = np.array([[0.5, 0.0, 0.0], [1.0, 2.0, 3.5], [-1.0, -2.5, -3.0], [0.0, 1.0, 0.0], [2.0, 2.0, 2.0]])
    nrm = np.tile([0.0, 0.0, 1.0], (len(data), 1))
    t = tdtk.BOctTree(model, 0.1, False)
    kd = tdtk.KDtree(model)
    cur = tdtk.Scan(Z3, Z3, data, nrm)
    before = cur.get_xyz_reduced()
    rc, res, tm, da, _ = _c_match(tdtk, "tdtk_icp_match_octree", t._h, cur.handle, 1, tdtk.CLOSEST_POINT_ALONG_NORMAL_SIMPLE, 5, 625.0)
    assert rc == -5 and b"pairing mode 1 is not served by the octree" in tdtk.lib().tdtk_last_error()
    limit = 2.0 ** 30 / t.info()["mult"]
    rc, res, tm, da, _ = _c_match(tdtk, "tdtk_icp_match_octree", t._h, cur.handle, 1, 0, 5, (limit * 1.01) ** 2)
    assert rc == -5 and np.array_equal(tm, gen.I16) and np.array_equal(da, gen.I16)
    assert bm.same_bits(cur.get_xyz_reduced(), before)
    rc, res, tm, da, _ = _c_match(tdtk, "tdtk_icp_match_octree", t._h, cur.handle, 1, 0, 5, (limit * 0.5) ** 2)
    assert rc == 0 and res.iterations > 0 and not np.array_equal(tm, gen.I16)
    # a query beyond +-2^30 voxels at iteration 0: a fine tree, a scan far away
    rng = np.random.default_rng(5)
    cloud = rng.uniform(-5.0, 5.0, (300, 3))
    fine = tdtk.BOctTree(cloud, 1e-5, True)
    far = tdtk.Scan(Z3, Z3, cloud[:200] + 1e5)
    before = far.get_xyz_reduced()
    assert 1e5 * fine.info()["mult"] > 2.0 ** 30 > 5.0 * fine.info()["mult"] + 1
    rc, res, tm, da, _ = _c_match(tdtk, "tdtk_icp_match_octree", fine._h, far.handle, 1, 0, 5, 25.0)
    assert rc == -5 and res.iterations == 0 and b"does not fit +-2^30" in tdtk.lib().tdtk_last_error()
    assert np.array_equal(tm, gen.I16) and np.array_equal(da, gen.I16) and bm.same_bits(far.get_xyz_reduced(), before)
    near = tdtk.Scan(Z3, Z3, cloud[:200] + 0.01)                       # the same tree serves a scan that is in range
    rc, res, tm, da, _ = _c_match(tdtk, "tdtk_icp_match_octree", fine._h, near.handle, 1, 0, 3, 25.0)
    assert rc == 0 and res.last_pairs == 200
    # N == 0 and max_num_iterations == 0: the k-d form's answer
    empty = C.c_void_p()
    assert tdtk.lib().tdtk_scan_create(None, None, 0, 0, C.byref(empty)) == 0
    try:
        for scan_h, iters in ((empty, 5), (cur.handle, 0)):
            a = _c_match(tdtk, "tdtk_icp_match_octree", t._h, scan_h, 1, 0, iters, 625.0)
            b = _c_match(tdtk, "tdtk_icp_match", kd._h, scan_h, 1, 0, iters, 625.0)
            assert a[0] == b[0] == 0
            for f in ("iterations", "converged", "last_pairs", "last_rms"):
                assert getattr(a[1], f) == getattr(b[1], f) == 0
            assert np.array_equal(a[2], gen.I16) and np.array_equal(a[3], gen.I16)
        # the argument checks and their messages are tdtk_icp_match's
        for fn, h in (("tdtk_icp_match_octree", t._h), ("tdtk_icp_match", kd._h)):
            assert _c_match(tdtk, fn, h, cur.handle, 1, 0, -1, 625.0)[0] == -1
            msg = tdtk.lib().tdtk_last_error()
            assert b"max_dist_match and max_num_iterations have to be >= 0" in msg
            assert _c_match(tdtk, fn, h, cur.handle, 11, 0, 5, 625.0)[0] == -1
        assert _c_match(tdtk, "tdtk_icp_match_octree", None, cur.handle, 1, 0, 5, 625.0)[0] == -1
    finally:
        tdtk.lib().tdtk_scan_destroy(empty)


def test_a_kd_loop_right_after_an_octree_loop_gives_its_usual_trace(tdtk, gpu, fx, hashes):
    """the octree loop leaves neither certificates nor hits a k-d loop would take for its own"""
    model, data, _ = gen.cloud_of(fx, "seam")
    kd_prev, oc_prev = _model_scan(tdtk, model, 0), _model_scan(tdtk, model, 2)
    first = _run(tdtk, kd_prev, data, None, 1, 0, gen.SEAM_MAXD2, 6, 0.0)
    _run(tdtk, oc_prev, data, None, 1, 0, gen.SEAM_MAXD2, 6, 0.0)
    again = _run(tdtk, kd_prev, data, None, 1, 0, gen.SEAM_MAXD2, 6, 0.0)
    assert first[0] == again[0] == 5
    assert np.array_equal(first[1]["trace"][:, 0], again[1]["trace"][:, 0]) and first[1]["index_hashes"] == again[1]["index_hashes"]
    assert np.allclose(first[1]["trace"], again[1]["trace"], rtol=0, atol=POSE_ATOL)


def test_do_icp_over_three_scans(tdtk, gpu):
    """doICP on the bundled sequence with every scan's tree an octree: the poses of the k-d run to 1e-6 (no ties, no partner
    within 0.01 on these scans); with the trees prepared ahead by other host threads and without: identical"""
    z = np.load(os.path.join(bm.G, "dat_scans.npz"))

    def run(nns, prefetch):
        S = [tdtk.Scan(z["pose%03d" % k][:3], z["pose%03d" % k][3:], z["scan%03d" % k]).setSearchTreeParameter(nns) for k in range(3)]
        icp = tdtk.icp6D(tdtk.icp6D_QUAT(True), 25.0, 50, quiet=True, epsilonICP=1e-5)
        icp.doICP(S, prefetch=prefetch)
        assert all(isinstance(s.kd, tdtk.BOctTree if nns == 2 else tdtk.KDtree) for s in S[:2])
        out = np.array([s.get_transMat() for s in S])
        for s in S:
            s.release()
        return out
    kd, oc, oc_serial = run(0, True), run(2, True), run(2, False)
    print("max |pose octree - k-d|", np.abs(oc - kd).max())
    assert np.array_equal(oc, oc_serial)
    assert np.allclose(oc, kd, rtol=0, atol=1e-6)
    assert not np.array_equal(oc[1], np.eye(4).reshape(16))
