"""Radius clustering on the device (tdtk_cluster_radius, KDtree.clusters, collision.segment_colliding) against the fixture
k15_clusters.npz, whose every neighbour list is the reference's own compiled KDtreeIndexed::fixedRangeSearch (the CPU tier
pins the fixture to the live library), and against the live library at radii the fixture does not hold where oracle/_ref
travelled.  Every comparison is exact: labels (or their CRC-32), n_clusters, first and sizes."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
pytestmark = pytest.mark.gpu

# query.hip's launch geometry, restated
Q_MAX_BLOCKS, Q_BLOCK = 2048, 128
TDTK_EINVAL = -1


@pytest.fixture(scope="module")
def mg():
    spec = importlib.util.spec_from_file_location("make_golden_clusters", os.path.join(G, "make_golden_clusters.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def fx(mg):
    return np.load(mg.OUT)


@pytest.fixture(scope="module")
def clouds(mg):
    """the large clouds and their trees, built once"""
    store = {}

    def get(tdtk, name, bucket):
        if name not in store:
            store[name] = {"pts": mg.large_cloud(name)}
        if bucket not in store[name]:
            store[name][bucket] = tdtk.KDtree(store[name]["pts"], bucket)
        return store[name]["pts"], store[name][bucket]
    return get


def _consistent(mg, got):
    """first and sizes are what the labels imply; clusters ascend by first member"""
    labels, k, first, sizes = got
    n, f, s = mg.of_labels(labels)
    assert labels.dtype == np.int32 and first.dtype == np.int32 and sizes.dtype == np.uint32
    assert k == n and np.array_equal(first, f) and np.array_equal(sizes, s)
    assert (np.diff(first) > 0).all()


def _check_large(mg, fx, key, got):
    _consistent(mg, got)
    labels, k, first, sizes = got
    assert k == int(fx[key + "_n"][0]), key
    assert int(mg.crc(labels)[0]) == int(fx[key + "_crc"][0]), key
    assert (int(sizes.max()) if k else 0) == int(fx[key + "_max"][0]), key


@pytest.mark.parametrize("name", ["uniform", "duplicates", "lattice", "clusters", "seven", "one", "lattice16"])
def test_small_cases(tdtk, gpu, mg, fx, name):
    """3 buckets x 3 radii per k8 cloud; the 16^3 integer lattice at sqRad2 = 1 (all singletons: '<' is strict) and one ulp
    above it (one component)"""
    n = 0
    trees = {}
    for key, pts, b, r2 in mg.small_cases():
        if key.split("_b")[0] != name:
            continue
        if b not in trees:
            trees[b] = tdtk.KDtree(pts, b)
        got = trees[b].clusters(r2, want_sizes=True)
        assert np.array_equal(got[0], fx[key + "_labels"]), key
        _consistent(mg, got)
        n += 1
    assert n == (6 if name == "lattice16" else 9)
    if name == "lattice16":
        assert got[1] == 1 and int(got[3][0]) == 4096


@pytest.mark.parametrize("key", ["mix_r0", "mix_r1", "mix_r2", "chains", "chains_bridge", "deep_b1", "deep_b20", "table",
                                 "nonfinite", "normals_plain", "normals_cos10"])
def test_large_cases(tdtk, gpu, mg, fx, clouds, key):
    """mix at three radii; two shuffled helices (long union-find paths) and their bridge; the deep tree at buckets 1 and 20
    (300,000 slots or more on at most 262,144 lanes: a second trip of the grid-stride loop); leaf-table mode with 40,000
    identical points in one leaf, all hooking one root; the crossing planes with and without the normals predicate"""
    case = {k: (name, b, r2, kw) for k, name, b, r2, kw in mg.large_cases()}[key]
    name, b, r2, kw = case
    pts, kd = clouds(tdtk, name, b)
    if name == "deep":
        assert len(pts) > Q_MAX_BLOCKS * Q_BLOCK
    args = {}
    if "normals" in kw:
        args = {"normals": kw["normals"], "max_angle_deg": 10.0}
        assert np.cos(np.deg2rad(10.0)) == mg.NORMALS_COS
    _check_large(mg, fx, key, kd.clusters(r2, want_sizes=True, **args))
    if key == "chains":
        labels = kd.clusters(r2)[0]
        assert sorted(np.bincount(labels)) == [2500, 2500]


def test_mix_in_many_trips_of_a_small_grid(tdtk, gpu, mg, fx, clouds):
    """the link kernel capped to 8 workgroups of 128 lanes: 20,000 slots or more in twenty trips of the grid-stride loop
    and in another interleaving of the atomics; the labels are the fixture's, and the full grid's"""
    pts, kd = clouds(tdtk, "mix", 20)
    L = tdtk.lib()
    full = [kd.clusters(r2, want_sizes=True) for r2 in mg.MIX_R2]
    was = L.tdtk_cluster_grid_cap(8)
    try:
        assert was == 0 and len(pts) > 19 * 8 * Q_BLOCK
        for j, r2 in enumerate(mg.MIX_R2):
            got = kd.clusters(r2, want_sizes=True)
            _check_large(mg, fx, "mix_r%d" % j, got)
            for a, b in zip(got, full[j]):
                assert np.array_equal(a, b)
    finally:
        assert L.tdtk_cluster_grid_cap(was) == 8
    assert L.tdtk_cluster_grid_cap(0) == 0


def test_subset_on_the_full_tree_is_the_tree_over_the_subset(tdtk, gpu, mg, fx, clouds):
    """the fixture's labels come from a reference tree over the kept points alone; and the device's own tree over them"""
    pts, kd = clouds(tdtk, "mix", 20)
    sub = mg.mix_subset()
    kept = np.flatnonzero(sub)
    alone = tdtk.KDtree(pts[kept], 20)
    for j, r2 in enumerate(mg.MIX_R2):
        got = kd.clusters(r2, subset=sub, want_sizes=True)
        _check_large(mg, fx, "mix_r%d_subset" % j, got)
        assert (got[0][~sub] == -1).all() and (got[0][sub] >= 0).all()
        la, ka, fa, sa = alone.clusters(r2, want_sizes=True)
        assert ka == got[1] and np.array_equal(la, got[0][kept]) and np.array_equal(kept[fa], got[2]) and np.array_equal(sa, got[3])


def test_min_size_drops_and_renumbers(tdtk, gpu, mg, fx, clouds):
    pts, kd = clouds(tdtk, "mix", 20)
    r2 = mg.MIX_R2[0]
    got = kd.clusters(r2, min_size=mg.MIX_MIN_SIZE, want_sizes=True)
    _check_large(mg, fx, "mix_r0_min%d" % mg.MIX_MIN_SIZE, got)
    assert got[3].min() >= mg.MIX_MIN_SIZE and (got[0] == -1).any()
    plain = kd.clusters(r2, want_sizes=True)
    for ms in (0, 1):
        for a, b in zip(kd.clusters(r2, min_size=ms, want_sizes=True), plain):
            assert np.array_equal(a, b)
    # the kept clusters are the plain ones of that size, in the same order
    big = plain[3] >= mg.MIX_MIN_SIZE
    assert np.array_equal(got[2], plain[2][big]) and np.array_equal(got[3], plain[3][big])
    # larger than every component: nothing is kept
    labels, k, first, sizes = kd.clusters(r2, min_size=int(plain[3].max()) + 1, want_sizes=True)
    assert k == 0 and (labels == -1).all() and len(first) == 0 and len(sizes) == 0


def test_live_reference_at_radii_the_fixture_does_not_hold(tdtk, gpu, orc, mg, clouds):
    if not orc.have_ref():
        pytest.skip("no reference library (oracle/_ref/libref3dtk.so)")
    for name, b, r2 in (("mix", 20, 16.0), ("deep", 20, 1.0)):
        assert r2 not in mg.MIX_R2 and r2 != mg.DEEP_R2
        pts, kd = clouds(tdtk, name, b)
        want = mg.reference_labels(pts, b, r2)
        got = kd.clusters(r2, want_sizes=True)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1], name
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]), name
        assert 1 < got[1] < len(pts)


def test_tree_from_two_resident_scans(tdtk, gpu, mg, fx):
    """tdtk_tree_create_from_scans: the labels count through the concatenation"""
    pts = mg.k8_clouds()["uniform"][0]
    sa = tdtk.Scan([0, 0, 0], [0, 0, 0], pts[:400], bucketSize=5)
    sb = tdtk.Scan([0, 0, 0], [0, 0, 0], pts[400:], bucketSize=5)
    kd = tdtk.MetaScan([sa, sb]).getSearchTree()
    one = tdtk.KDtree(pts, 5)
    for j, r2 in enumerate(mg.SMALL_R2["uniform"]):
        got = kd.clusters(r2, want_sizes=True)
        assert np.array_equal(got[0], fx["uniform_b5_r%d_labels" % j])
        for a, b in zip(got, one.clusters(r2, want_sizes=True)):
            assert np.array_equal(a, b)


def test_collision_pipeline_end_to_end(tdtk, gpu, mg):
    """handle_pointcloud, then segment_colliding with its mask: the groups are the components of a tree over the colliding
    points alone, mapped back; groups ascend by first member, members ascend"""
    pts, model, frames, radius = mg.mgc.small_case("uniform")
    kd = tdtk.KDtree(pts, 20)
    mask, num = tdtk.handle_pointcloud(model, kd, frames, radius, 1)
    assert 1 < num < len(pts)
    r2 = 4.0
    groups = tdtk.segment_colliding(kd, mask, sqRad2=r2)
    again = tdtk.segment_colliding(pts, mask, sqRad2=r2, bucketSize=5)
    hit = np.flatnonzero(mask)
    la, ka = tdtk.KDtree(pts[hit], 20).clusters(r2)
    assert len(groups) == ka == len(again) and 1 <= ka <= num
    assert sorted(np.concatenate(groups)) == list(hit)
    firsts = [int(g[0]) for g in groups]
    assert firsts == sorted(firsts)
    for c, g in enumerate(groups):
        assert g.dtype.kind == "i" and (np.diff(g) > 0).all()
        assert np.array_equal(g, hit[la == c]) and np.array_equal(g, again[c])
    # the default radius is the literal of segment_colliding.cc:61; no mask: every point
    labels, k = kd.clusters(20.0)
    every = tdtk.segment_colliding(kd)
    assert len(every) == k and all(np.array_equal(g, np.flatnonzero(labels == c)) for c, g in enumerate(every))


def test_python_mirror(tdtk, gpu, mg, fx):
    pts = mg.k8_clouds()["clusters"][0]
    kd = tdtk.KDtree(pts, 20)
    r2 = mg.SMALL_R2["clusters"][2]
    labels, k = kd.clusters(r2)
    l2, k2, first, sizes = kd.clusters(r2, want_sizes=True)
    assert k == k2 == 6 and np.array_equal(labels, l2) and np.array_equal(labels, fx["clusters_b20_r2_labels"])
    assert len(first) == len(sizes) == 6 and (sizes == 120).all()
    groups = tdtk.segment_colliding(kd, sqRad2=r2)
    assert [int(g[0]) for g in groups] == list(first) and [len(g) for g in groups] == list(sizes)
    with pytest.raises(ValueError):
        kd.clusters(r2, subset=np.ones(3, bool))
    with pytest.raises(ValueError):
        kd.clusters(r2, normals=np.zeros((len(pts), 3)))


def test_rejections_write_nothing(tdtk, gpu, mg):
    """NULL labels or n_clusters, a non-finite sqRad2, min_abs_cos outside [0, 1] or NaN with normals: TDTK_EINVAL with
    labels untouched; normals == NULL ignores min_abs_cos; sqRad2 <= 0 gives M singletons"""
    pts = mg.k8_clouds()["uniform"][0]
    M = len(pts)
    kd = tdtk.KDtree(pts, 20)
    L = tdtk.lib()
    ip = C.POINTER(C.c_int32)
    nrm = np.ascontiguousarray(np.tile([0.0, 0.0, 1.0], (M, 1)))
    dp = nrm.ctypes.data_as(C.POINTER(C.c_double))

    def call(r2, normals, cos, labels, n):
        return L.tdtk_cluster_radius(kd._h, r2, None, normals, cos, 1, labels, n, None, None)

    labels = np.full(M, -7, np.int32)
    n = C.c_uint64(99)
    lp = labels.ctypes.data_as(ip)
    assert call(4.0, None, 0.0, None, C.byref(n)) == TDTK_EINVAL
    assert call(4.0, None, 0.0, lp, None) == TDTK_EINVAL
    for r2 in (np.nan, np.inf, -np.inf):
        assert call(r2, None, 0.0, lp, C.byref(n)) == TDTK_EINVAL
    for cos in (-0.1, 1.5, np.nan, np.inf):
        assert call(4.0, dp, cos, lp, C.byref(n)) == TDTK_EINVAL
    assert (labels == -7).all() and n.value == 99
    want = kd.clusters(4.0)
    for cos in (-0.1, 1.5, np.nan):            # no normals: min_abs_cos is ignored
        assert call(4.0, None, cos, lp, C.byref(n)) == 0
        assert np.array_equal(labels, want[0]) and n.value == want[1]
    for cos in (0.0, 1.0):
        assert call(4.0, dp, cos, lp, C.byref(n)) == 0 and np.array_equal(labels, want[0])
    for r2 in (0.0, -1.0):
        got = kd.clusters(r2, want_sizes=True)
        assert got[1] == M and np.array_equal(got[0], np.arange(M)) and np.array_equal(got[2], np.arange(M))
        assert (got[3] == 1).all()
    sub = np.arange(M) % 2 == 0
    got = kd.clusters(0.0, subset=sub)
    assert got[1] == sub.sum() and np.array_equal(got[0][sub], np.arange(sub.sum())) and (got[0][~sub] == -1).all()


def test_repeated_calls_and_bucket_sizes(tdtk, gpu, mg, fx, clouds):
    """two calls in a row, with another tree's call in between, give identical output; buckets 1, 5 and 20 identical labels"""
    pts, kd = clouds(tdtk, "mix", 20)
    other = tdtk.KDtree(mg.k8_clouds()["uniform"][0], 5)
    r2 = mg.MIX_R2[1]
    a = kd.clusters(r2, want_sizes=True)
    other.clusters(36.0, min_size=3)
    b = kd.clusters(r2, want_sizes=True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for bucket in (1, 5):
        c = tdtk.KDtree(pts, bucket).clusters(r2, want_sizes=True)
        for x, y in zip(a, c):
            assert np.array_equal(x, y)
