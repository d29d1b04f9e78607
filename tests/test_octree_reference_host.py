"""Octree reduction (tdtk_reduce_octree / tdtk_reduce_octree_nrpts): the CPU tier.  The oracle's restatement
(orc.octree_center / orc.octree_random) against the fixture k14_octree.npz, which holds what the reference's own compiled
BOctTree<double> returns, and -- where the reference checkout is present -- against that class itself on exactly the inputs
where the GPU tier compares the device with the oracle, so that there "device == oracle" means "device == reference", and on
a randomized sweep over shapes and depths.  Every comparison is by bits."""
import importlib.util
import json
import os

import numpy as np
import pytest

from test_gpu_parity import _clouds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


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


@pytest.fixture(scope="module")
def ref():
    if not mo.have_ref():
        pytest.skip("no reference checkout (src/slam6d/Boctree.cc)")
    mo.ref_lib()
    return mo.RefOct


def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _multiset(a):
    return np.unique(np.ascontiguousarray(a).view(np.uint64), axis=0, return_counts=True)


def _oracle_equals_reference(orc, ref, pts, voxel, seeds, tag):
    """centres, the full leaf order, and nrpts 1 and 3 with seeds[nrpts]"""
    assert _same(orc.octree_center(pts, voxel), ref.centres(pts, voxel)), (tag, voxel, "centres")
    assert _same(orc.octree_random(pts, voxel, mo.ALL), ref.random(pts, voxel, mo.ALL, 0)), (tag, voxel, "leaf order")
    for nrpts, seed in sorted(seeds.items()):
        assert _same(orc.octree_random(pts, voxel, nrpts, seed=seed), ref.random(pts, voxel, nrpts, seed)), (tag, voxel, nrpts)


# ---- the fixture ------------------------------------------------------------------------------------------------------
def test_fixture_is_what_the_generator_says(fx):
    """the clouds have the properties their cases are there for; all cases and nothing else; under 500 KB"""
    assert os.path.getsize(mo.OUT) <= mo.MAX_BYTES
    c = {name: fx.cloud(name) for name, _ in mo.CASES}
    mo.check_clouds(c)
    gen = mo.clouds()
    for name in c:
        assert _same(c[name], gen[name]), name
    assert fx.seed == mo.SEED and len(fx.rand_probe) == 8
    assert mo.key("deep21", mo.DEEP22_VOXEL, "centres") not in fx.z          # 22 levels: refused by the device, no row
    for name, voxel in CASES:
        pts, leaf = c[name], fx.leaf(name, voxel)
        assert len(leaf) == len(pts) and np.array_equal(leaf, mo.rep_index(pts, pts[leaf]))      # smallest index of its coordinates
        for a, b in zip(_multiset(pts[leaf]), _multiset(pts)):                                    # every point, once each
            assert np.array_equal(a, b)
        m = len(fx.centres(name, voxel))
        d1, d3 = fx.drawn(name, voxel, 1), fx.drawn(name, voxel, 3)
        assert 1 <= m <= len(pts) and len(d1) == m and m <= len(d3) <= min(3 * m, len(pts))


@pytest.mark.parametrize("name,voxel", CASES)
def test_oracle_equals_fixture(orc, fx, name, voxel):
    """never skips: the restatement against the rows the reference gave"""
    pts = fx.cloud(name)
    assert _same(orc.octree_center(pts, voxel), fx.centres(name, voxel))
    assert _same(orc.octree_random(pts, voxel, mo.ALL), pts[fx.leaf(name, voxel)])
    assert np.array_equal(mo.rand_probe(fx.seed), fx.rand_probe), "this C library's rand() is not the generating one's"
    for nrpts in (1, 3):
        assert _same(orc.octree_random(pts, voxel, nrpts, seed=fx.seed), pts[fx.drawn(name, voxel, nrpts)]), nrpts


def test_oracle_accepts_22_levels_where_the_device_refuses(orc, fx):
    """deep21 at the voxel no row is stored for: 22 levels, and the restatement still runs (the refusal is the device's)"""
    pts = fx.cloud("deep21")
    assert mo.depth_of(pts, mo.DEEP22_VOXEL) == 22
    assert len(orc.octree_center(pts, mo.DEEP22_VOXEL)) >= len(fx.centres("deep21", 0.0005))


def test_fixture_equals_the_reference(ref):
    """the generator, run again, gives the stored arrays"""
    z = np.load(mo.OUT)
    got = mo.compute()
    assert sorted(got) == sorted(z.files)
    for k in z.files:
        assert got[k].dtype == z[k].dtype and got[k].shape == z[k].shape and np.array_equal(got[k], z[k]), k


# ---- the inputs of the GPU tier's device-against-oracle tests (test_gpu_parity.py, test_octree_reduction_*) -------------
@pytest.mark.parametrize("name", ["uniform", "duplicates", "clusters", "plane", "tiny", "grid", "line"])
def test_oracle_equals_reference_on_the_gpu_tier_clouds(orc, ref, name):
    pts = _clouds()[name]
    for voxel in (0.5, 10.0, 1e6):
        _oracle_equals_reference(orc, ref, pts, voxel, {1: 1235, 3: 1237}, name)       # the seeds 1234 + nrpts of that tier


def test_oracle_equals_reference_on_the_bundled_scans(orc, ref):
    z = np.load(os.path.join(G, "dat_scans.npz"))
    for k in range(2):
        _oracle_equals_reference(orc, ref, z["scan%03d" % k], 10.0, {1: 1235, 3: 1237}, "scan%03d" % k)


def test_oracle_equals_reference_at_full_size(orc, ref):
    """the 1M model cloud of k5_hashes.json at voxel 25: centres, one point per leaf with seed 7, the full leaf order"""
    k = json.load(open(os.path.join(G, "k5_hashes.json")))
    M = k["M"]
    m = orc.gen_mt64_uniform(k["seed"], 6 * M, k["lo"], k["hi"])[:3 * M].reshape(M, 3).copy()
    _oracle_equals_reference(orc, ref, m, 25.0, {1: 7}, "k5 model")


# ---- randomized sweep -----------------------------------------------------------------------------------------------
def _sweep_cloud(rng, shape, n):
    if shape == "uniform":
        return rng.uniform(-1, 1, (n, 3)) * rng.choice([1e-3, 1.0, 50.0, 1e4]) + rng.uniform(-100, 100, 3)
    if shape == "lattice":
        side = int(rng.integers(2, 40))
        return rng.integers(0, side, (n, 3)).astype(np.float64) - rng.integers(0, side)
    if shape == "planar":
        p = rng.uniform(-30, 30, (n, 3))
        p[:, int(rng.integers(0, 3))] = rng.choice([0.0, -0.0, 7.25])
        return p
    k = int(rng.integers(1, 5))
    return np.concatenate([rng.normal(rng.uniform(-200, 200, 3), 10.0 ** rng.uniform(-4, 0), (n // k + 1, 3)) for _ in range(k)])[:n]


def test_randomized_sweep_oracle_equals_reference(orc, ref):
    """240 clouds of 50..3000 points, four shapes, the voxel drawn so that the depth is spread over 1..21 (one time in four
    exactly a halved root size: the `size <= voxel` edge)"""
    rng = np.random.default_rng(1414)
    depths = set()
    for it in range(240):
        shape = ("uniform", "lattice", "planar", "clustered")[it % 4]
        pts = np.ascontiguousarray(_sweep_cloud(rng, shape, int(rng.integers(50, 3001))))
        size = float((0.5 * (pts.max(0) - pts.min(0))).max() + 1.0)
        d = 1 + (it // 4) % 21
        voxel = size / 2.0 ** d * (1.0 if rng.integers(0, 4) == 0 else rng.uniform(1.0, 2.0))
        assert mo.depth_of(pts, voxel) == d
        depths.add(d)
        _oracle_equals_reference(orc, ref, pts, voxel, {1: 100 + it, 3: 500 + it}, (it, shape, d))
    assert depths == set(range(1, 22))
