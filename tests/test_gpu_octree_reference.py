"""Octree reduction on the device (tdtk_reduce_octree / tdtk_reduce_octree_nrpts, reduce.hip) against the reference's own
compiled BOctTree<double>, through the fixture k14_octree.npz (tests/golden/make_golden_octree.py; nothing else is read).

Every comparison is by bits: the centres of GetOctTreeCenter in their depth-first order; the full leaf order
(GetOctTreeRandom with more points asked for than any leaf has: every point, leaf by leaf, in the order the reference's
in-place partitions leave, without a rand() call); the rows drawn with nrpts 1 and 3 after srand(seed), where this process's
C library gives the rand() values the fixture was drawn with (only those rows skip otherwise)."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
pytestmark = pytest.mark.gpu


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(G, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


mo = _load("make_golden_octree")
CASES = [(name, voxel) for name, voxels in mo.CASES for voxel in voxels]


@pytest.fixture(scope="module")
def fx():
    return mo.load()


def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("name,voxel", CASES)
def test_centres_equal_the_reference(tdtk, gpu, fx, name, voxel):
    """same count, same order, bit for bit"""
    got = tdtk.calcReducedPoints(fx.cloud(name), voxel)
    want = fx.centres(name, voxel)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert _same(got, want)


@pytest.mark.parametrize("name,voxel", CASES)
def test_leaf_order_equals_the_reference(tdtk, gpu, fx, name, voxel):
    """all n points, leaf by leaf and inside a leaf in the reference's order (launch_oct_leaf_order); no rand() involved"""
    pts = fx.cloud(name)
    got = tdtk.calcReducedPoints(pts, voxel, nrpts=mo.ALL)
    assert got.shape == pts.shape
    assert _same(got, pts[fx.leaf(name, voxel)])


@pytest.mark.parametrize("nrpts", [1, 3])
@pytest.mark.parametrize("name,voxel", CASES)
def test_drawn_rows_equal_the_reference(tdtk, gpu, fx, name, voxel, nrpts):
    probe = mo.rand_probe(fx.seed)
    if not np.array_equal(probe, fx.rand_probe):
        pytest.skip("this C library's rand() after srand(%d) gives %s, the fixture was drawn with %s: the drawn rows hold for "
                    "the generating C library only" % (fx.seed, probe.tolist(), fx.rand_probe.tolist()))
    pts = fx.cloud(name)
    got = tdtk.calcReducedPoints(pts, voxel, nrpts=nrpts, seed=fx.seed)
    want = pts[fx.drawn(name, voxel, nrpts)]
    assert got.shape == want.shape, (got.shape, want.shape)
    assert _same(got, want)


def test_depth_boundary(tdtk, gpu, fx):
    """21 levels (63 key bits) is the deepest tree the device accepts, and there it equals the reference; the same cloud at a
    voxel that needs 22 is refused by both entry points"""
    pts = fx.cloud("deep21")
    assert mo.depth_of(pts, 0.0005) == 21 and mo.depth_of(pts, mo.DEEP22_VOXEL) == 22
    assert _same(tdtk.calcReducedPoints(pts, 0.0005), fx.centres("deep21", 0.0005))
    assert _same(tdtk.calcReducedPoints(pts, 0.0005, nrpts=mo.ALL), pts[fx.leaf("deep21", 0.0005)])
    with pytest.raises(tdtk.TdtkError):
        tdtk.calcReducedPoints(pts, mo.DEEP22_VOXEL)                       # tdtk_reduce_octree
    for nrpts in (1, 3, mo.ALL):
        with pytest.raises(tdtk.TdtkError):
            tdtk.calcReducedPoints(pts, mo.DEEP22_VOXEL, nrpts=nrpts)      # tdtk_reduce_octree_nrpts
    # a refusal leaves the workspaces usable
    assert _same(tdtk.calcReducedPoints(pts, 0.0005), fx.centres("deep21", 0.0005))


@pytest.mark.parametrize("name,voxel", [("uniform", 1e6), ("uniform", 0.5)])
def test_repeatability_across_sizes(tdtk, gpu, fx, name, voxel):
    """the workspaces are reused between calls of different n: each entry point twice, a call of another size (a smaller and a
    larger one in turn) in between, the same bytes -- the reference's"""
    pts = fx.cloud(name)
    small, large = fx.cloud("duplicates"), np.concatenate([fx.cloud("clusters"), fx.cloud("lattice62")])
    want_c, want_l = fx.centres(name, voxel), pts[fx.leaf(name, voxel)]
    for other, ov in ((small, 1.0), (large, 10.0)):
        a = tdtk.calcReducedPoints(pts, voxel)
        tdtk.calcReducedPoints(other, ov)
        b = tdtk.calcReducedPoints(pts, voxel)
        assert a.tobytes() == b.tobytes() and _same(a, want_c)
        a = tdtk.calcReducedPoints(pts, voxel, nrpts=mo.ALL)
        tdtk.calcReducedPoints(other, ov, nrpts=mo.ALL)
        b = tdtk.calcReducedPoints(pts, voxel, nrpts=mo.ALL)
        assert a.tobytes() == b.tobytes() and _same(a, want_l)
