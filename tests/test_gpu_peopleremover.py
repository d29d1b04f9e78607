"""peopleremover on the device (tdtk_voxel_walk, tdtk_peopleremover and their Python mirror) against the fixture
k17_peopleremover.npz, whose every voxel list and every mask is the reference's own compiled walk_voxels / visitor /
voxel_of_point (the CPU tier pins the fixture to the live reference).  Every comparison is exact."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
pytestmark = pytest.mark.gpu
TDTK_EINVAL, TDTK_EUNSUP = -1, -5


def _gold():
    spec = importlib.util.spec_from_file_location("make_golden_peopleremover", os.path.join(G, "make_golden_peopleremover.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


gold = _gold()
WALKS = {name: (vs, s, e) for name, vs, s, e in gold.walk_cases()}
RUNS = {c["name"]: c for c in gold.pipeline_cases()}


@pytest.fixture(scope="module")
def fx():
    return gold.load()


@pytest.mark.parametrize("name", sorted(WALKS))
def test_voxel_walk_lists_are_the_references(tdtk, gpu, fx, name):
    vs, s, e = WALKS[name]
    assert fx.walk_sha(name) == gold.digest([s, e]), "the inputs are not the ones the fixture was made from"
    offsets, vox = tdtk.walk_voxels(s, e, vs)
    rc, rv = fx.walk(name)
    assert offsets.dtype == np.uint64 and vox.dtype == np.int32
    assert np.array_equal(np.diff(offsets.astype(np.int64)), rc)
    assert np.array_equal(vox.astype(np.int64), rv)


def test_voxel_walk_count_then_fill(tdtk, gpu, fx):
    """offsets and total are always filled; cap too small writes nothing else, reports the needed size and refuses"""
    vs, s, e = WALKS["shapes_v10"]
    L = tdtk.lib()
    m = len(s)
    rc_counts, rv = fx.walk("shapes_v10")
    off = np.zeros(m + 1, np.uint64)
    total = C.c_uint64(0)
    vox = np.full((len(rv), 3), -77, np.int32)
    a, b = np.ascontiguousarray(s), np.ascontiguousarray(e)
    args = (0, a.ctypes.data_as(C.POINTER(C.c_double)), b.ctypes.data_as(C.POINTER(C.c_double)), m, vs,
            off.ctypes.data_as(C.POINTER(C.c_uint64)), vox.ctypes.data_as(C.POINTER(C.c_int32)))
    assert L.tdtk_voxel_walk(*args, len(rv) - 1, C.byref(total)) == TDTK_EINVAL
    assert total.value == len(rv) and (vox == -77).all()
    assert np.array_equal(np.diff(off.astype(np.int64)), rc_counts)
    assert L.tdtk_voxel_walk(*args, len(rv), C.byref(total)) == 0
    assert np.array_equal(vox.astype(np.int64), rv)
    off0, vox0 = tdtk.walk_voxels(np.zeros((0, 3)), np.zeros((0, 3)), 1.0)       # no ray: no list
    assert off0.tolist() == [0] and vox0.shape == (0, 3)


def _run(tdtk, case):
    masks, counts = tdtk.peopleremover(case["scans"], case["origins"], voxel_size=case["vs"], diff=case["diff"],
                                       cluster_size=case["cluster"], no_subvoxel_accuracy=not case["subvoxel"],
                                       ray_ends=case["ends"], want_free=True)
    return masks, counts


@pytest.mark.parametrize("name", sorted(RUNS))
def test_pipeline_is_the_references(tdtk, gpu, fx, name):
    case = RUNS[name]
    masks, counts = _run(tdtk, case)
    rdyn, rfree, rinfo = fx.run(case)
    got = [counts[k] for k in ("occupied", "freed", "free_after_clustering", "half_free", "visits")]
    assert got == [int(v) for v in rinfo], (got, rinfo)
    assert np.array_equal(counts["free_voxels"].astype(np.int64), rfree)
    assert [len(m) for m in masks] == [len(s) for s in case["scans"]]
    assert np.array_equal(np.concatenate(masks).astype(np.uint8), rdyn)


def test_pipeline_accepts_poses_and_is_repeatable(tdtk, gpu, fx):
    """[S][16] transMatOrg instead of positions; a second call on the same context (workspaces reused) gives the same"""
    case = RUNS["room3_d0"]
    poses = np.tile(np.eye(4).reshape(16), (len(case["scans"]), 1))
    poses[:, 12:15] = case["origins"]
    rdyn = fx.run(case)[0]
    for _ in range(2):
        masks, _ = tdtk.peopleremover(case["scans"], poses)                      # the reference's defaults
        assert np.array_equal(np.concatenate(masks).astype(np.uint8), rdyn)


def _call(tdtk, xyz, offs, org, ends=None, vs=10.0, cap=0, free=None):
    xyz = np.ascontiguousarray(xyz, np.float64)
    offs = np.ascontiguousarray(offs, np.uint64)
    org = np.ascontiguousarray(org, np.float64)
    dyn = np.full(len(xyz), 9, np.uint8)
    info = np.full(5, 99, np.uint64)
    dp = C.POINTER(C.c_double)
    rc = tdtk.lib().tdtk_peopleremover(0, xyz.ctypes.data_as(dp), offs.ctypes.data_as(C.POINTER(C.c_uint64)), org.ctypes.data_as(dp),
                                       ends.ctypes.data_as(dp) if ends is not None else None, len(offs) - 1, vs, 0, 1, 1,
                                       dyn.ctypes.data_as(C.POINTER(C.c_uint8)),
                                       free.ctypes.data_as(C.POINTER(C.c_int32)) if free is not None else None, cap,
                                       info.ctypes.data_as(C.POINTER(C.c_uint64)))
    return rc, dyn, info


def test_refusals(tdtk, gpu, fx):
    case = RUNS["halffree_sub1"]
    xyz = np.concatenate(case["scans"])
    offs = np.concatenate([[0], np.cumsum([len(s) for s in case["scans"]])])
    org = case["origins"]
    rc, dyn, info = _call(tdtk, xyz, offs, org)
    assert rc == 0 and dyn.tolist() == [0, 1, 1, 0, 0]

    def refused(code, **kw):
        a = dict(xyz=xyz, offs=offs, org=org)
        a.update(kw)
        rc, dyn, info = _call(tdtk, **a)
        assert rc == code, (rc, kw.keys())
        assert (dyn == 9).all() and (info == 99).all()                              # nothing written

    for bad in (np.nan, np.inf, -np.inf):
        x = xyz.copy(); x[3, 1] = bad
        refused(TDTK_EINVAL, xyz=x)
        o = org.copy(); o[2, 0] = bad
        refused(TDTK_EINVAL, org=o)
        refused(TDTK_EINVAL, ends=x)
    for vs in (0.0, -1.0, np.nan, np.inf):
        refused(TDTK_EINVAL, vs=vs)
    refused(TDTK_EINVAL, offs=np.array([0, 3, 1, 5]))                               # not monotone
    refused(TDTK_EINVAL, offs=np.array([1, 1, 3, 5]))
    x = xyz.copy(); x[4, 2] = 10.0 * (2 ** 20 - 4)                                  # the first voxel coordinate that does not pack
    refused(TDTK_EUNSUP, xyz=x)
    o = org.copy(); o[0, 1] = -1.0e9
    refused(TDTK_EUNSUP, org=o)
    x[4, 2] = 10.0 * (2 ** 20 - 5)                                                  # the last one that does
    assert _call(tdtk, x, offs, org)[0] == 0
    # cap too small: the needed size is reported, mask and counts are written, the list is not
    free = np.full((4, 3), -77, np.int32)
    rc, dyn, info = _call(tdtk, xyz, offs, org, cap=0, free=free)
    assert rc == TDTK_EINVAL and int(info[2]) == 1 and dyn.tolist() == [0, 1, 1, 0, 0] and (free == -77).all()
    rc, dyn, info = _call(tdtk, xyz, offs, org, cap=4, free=free)
    assert rc == 0 and free[0].tolist() == [0, 0, 5] and (free[1:] == -77).all()
    # the walk query refuses the same way
    L = tdtk.lib()
    off = np.zeros(2, np.uint64)
    total = C.c_uint64(5)
    for s, vs, code in (([np.nan, 0, 0], 1.0, TDTK_EINVAL), ([0, 0, 0], 0.0, TDTK_EINVAL), ([0, 2.0e6, 0], 1.0, TDTK_EUNSUP)):
        a, b = np.array([s], np.float64), np.array([[1.0, 2.0, 3.0]])
        assert L.tdtk_voxel_walk(0, a.ctypes.data_as(C.POINTER(C.c_double)), b.ctypes.data_as(C.POINTER(C.c_double)), 1, vs,
                                 off.ctypes.data_as(C.POINTER(C.c_uint64)), None, 0, C.byref(total)) == code
