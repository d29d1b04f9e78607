"""The kernels around the voxel lane code (voxel.hip: keys, flags, compact, table, carve, the lock-free union-find, classify,
the walk query) and the device's own fmod and fp64 division, on the cases of k18_peopleremover_paths.npz -- the reference's own
compiled results, pinned to the live reference and explained case by case in tests/test_peopleremover_paths_host.py.  Reads
the fixture and its generators only.  Every comparison is exact."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
pytestmark = pytest.mark.gpu
TDTK_EINVAL, TDTK_EUNSUP = -1, -5


def _paths():
    sys.path.insert(0, G)                   # the generator imports the first one, and tests/voxel_keys.py, by name
    spec = importlib.util.spec_from_file_location("make_golden_peopleremover_paths", os.path.join(G, "make_golden_peopleremover_paths.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


paths = _paths()
WALKS = {name: (vs, s, e) for name, vs, s, e in paths.walk_cases()}
RUNS = {c["name"]: c for c in paths.pipeline_cases()}
RANDOM = [n for n in RUNS if n.startswith("rand")]
DP, U64P = C.POINTER(C.c_double), C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def fx():
    return paths.load()


def _flat(case):
    xyz = np.ascontiguousarray(np.concatenate(case["scans"]))
    offs = np.concatenate([[0], np.cumsum([len(s) for s in case["scans"]])]).astype(np.uint64)
    ends = np.ascontiguousarray(np.concatenate(case["ends"])) if case["ends"] is not None else None
    return xyz, offs, np.ascontiguousarray(case["origins"]), ends


def _c_call(tdtk, case, xyz=None, org=None, free=None):
    """tdtk_peopleremover itself, its outputs prefilled: (rc, dynamic, info)"""
    x, offs, o, ends = _flat(case)
    xyz = x if xyz is None else np.ascontiguousarray(xyz)
    org = o if org is None else np.ascontiguousarray(org)
    dyn = np.full(len(xyz), 9, np.uint8)
    info = np.full(5, 99, np.uint64)
    rc = tdtk.lib().tdtk_peopleremover(0, xyz.ctypes.data_as(DP), offs.ctypes.data_as(U64P), org.ctypes.data_as(DP),
                                       ends.ctypes.data_as(DP) if ends is not None else None, len(offs) - 1, case["vs"],
                                       case["diff"], case["cluster"], 1 if case["subvoxel"] else 0,
                                       dyn.ctypes.data_as(C.POINTER(C.c_uint8)),
                                       free.ctypes.data_as(C.POINTER(C.c_int32)) if free is not None else None,
                                       len(free) if free is not None else 0, info.ctypes.data_as(U64P))
    return rc, dyn, info


def _run(tdtk, case):
    """(dynamic [n] uint8, free [k][3] int64, [occupied, freed, free_after_clustering, half_free, visits])"""
    if max(case["diff"], case["cluster"]) >= 1 << 32:            # the entry point itself: the mirror may clamp
        rc, dyn, info = _c_call(tdtk, case)
        assert rc == 0
        free = np.full((int(info[2]), 3), -77, np.int32)
        if len(free):
            rc, dyn2, info2 = _c_call(tdtk, case, free=free)
            assert rc == 0 and np.array_equal(dyn, dyn2) and np.array_equal(info, info2)
        return dyn, free.astype(np.int64), [int(v) for v in info]
    masks, counts = tdtk.peopleremover(case["scans"], case["origins"], voxel_size=case["vs"], diff=case["diff"],
                                       cluster_size=case["cluster"], no_subvoxel_accuracy=not case["subvoxel"],
                                       ray_ends=case["ends"], want_free=True)
    assert [len(m) for m in masks] == [len(s) for s in case["scans"]]
    return (np.concatenate(masks).astype(np.uint8), counts["free_voxels"].astype(np.int64),
            [counts[k] for k in ("occupied", "freed", "free_after_clustering", "half_free", "visits")])


def _check_run(tdtk, fx, name):
    dyn, free, info = _run(tdtk, RUNS[name])
    rdyn, rfree, rinfo = fx.run(RUNS[name])
    assert info == [int(v) for v in rinfo], (name, info, rinfo)
    assert np.array_equal(free, rfree), name
    assert np.array_equal(dyn, rdyn), name


def _check_walk(tdtk, fx, name):
    vs, s, e = WALKS[name]
    assert fx.walk_sha(name) == paths.gold.digest([s, e]), "the inputs are not the ones the fixture was made from"
    offsets, vox = tdtk.walk_voxels(s, e, vs)
    rc, rv = fx.walk(name)
    assert offsets.dtype == np.uint64 and vox.dtype == np.int32
    assert np.array_equal(np.diff(offsets.astype(np.int64)), rc), name
    assert np.array_equal(vox.astype(np.int64), rv), name


@pytest.mark.parametrize("name", [n for n in RUNS if not n.startswith("rand")])
def test_pipeline_is_the_references(tdtk, gpu, fx, name):
    _check_run(tdtk, fx, name)


@pytest.mark.parametrize("name", sorted(WALKS))
def test_voxel_walk_lists_are_the_references(tdtk, gpu, fx, name):
    _check_walk(tdtk, fx, name)


def test_table_cases_again_and_again(tdtk, gpu, fx):
    """the order in which the bricks win their slots is the device's: the result may not depend on it"""
    for _ in range(16):
        for name in ("chain64", "chain128", "bricks32", "bricks33"):
            _check_run(tdtk, fx, name)


def test_random_scenes_in_a_row_with_walks_between(tdtk, gpu, fx):
    """the scenes of tier e in the fixture's order on one context; after every 16th a walk query, whose voxel lists take
    the workspace that held the brick table"""
    assert len(RANDOM) == paths.N_RANDOM
    walks = sorted(WALKS)
    for i, name in enumerate(RANDOM):
        _check_run(tdtk, fx, name)
        if i % 16 == 15:
            _check_walk(tdtk, fx, walks[(i // 16) % len(walks)])


def test_small_after_large_and_both_entry_points_on_one_context(tdtk, gpu, fx):
    for kind, name in (("run", "room8x8193"), ("run", "one_point"), ("walk", "uniform_v0.07"), ("run", "bricks33"),
                       ("run", "bricks32"), ("run", "room8x8193")):
        (_check_run if kind == "run" else _check_walk)(tdtk, fx, name)


def test_refusals_on_the_last_items(tdtk, gpu, fx):
    """a bad coordinate in the last lane's item -- the last point of 257, the last of 9 origins over 4 points, the last of 65
    rays -- is refused, and nothing is written"""
    def refused(code, case, **kw):
        rc, dyn, info = _c_call(tdtk, case, **kw)
        assert rc == code, (rc, case["name"])
        assert (dyn == 9).all() and (info == 99).all()

    case = RUNS["n257"]
    x = _flat(case)[0].copy()
    assert len(x) == 257
    x[256, 2] = np.nan
    refused(TDTK_EINVAL, case, xyz=x)
    case = RUNS["scans9"]
    assert case["origins"].shape == (9, 3) and sum(len(s) for s in case["scans"]) == 4
    for bad, code in ((np.nan, TDTK_EINVAL), (10.0 * (2 ** 20 - 4), TDTK_EUNSUP)):
        o = case["origins"].copy()
        o[8, 1] = bad
        refused(code, case, org=o)
    assert _c_call(tdtk, RUNS["n257"])[0] == 0 and _c_call(tdtk, case)[0] == 0
    vs, s, e = WALKS["uniform_v7.3"]
    s, e = np.ascontiguousarray(np.concatenate([s, s[:1]])), np.concatenate([e, e[:1]])
    e[64, 0] = np.nan
    e = np.ascontiguousarray(e)
    off = np.full(66, 7, np.uint64)
    total = C.c_uint64(5)
    assert tdtk.lib().tdtk_voxel_walk(0, s.ctypes.data_as(DP), e.ctypes.data_as(DP), 65, vs, off.ctypes.data_as(U64P), None, 0,
                                      C.byref(total)) == TDTK_EINVAL
    assert (off == 7).all() and total.value == 5


def test_walk_refuses_more_than_2_32_visits(tdtk, gpu, fx):
    """m copies of the long ray (c visits each, m c >= 2^32 > (m - 1) c): refused; m - 1 copies without a buffer: the count
    pass alone, every offset and the total exact"""
    c = fx.long_count
    m = -(-(1 << 32) // c)
    assert (m - 1) * c < 1 << 32 <= m * c
    s = np.ascontiguousarray(np.tile(fx.long_ray[0], (m, 1)))
    e = np.ascontiguousarray(np.tile(fx.long_ray[1], (m, 1)))
    off = np.full(m + 1, 7, np.uint64)
    total = C.c_uint64(5)
    L = tdtk.lib()
    args = (0, s.ctypes.data_as(DP), e.ctypes.data_as(DP))
    assert L.tdtk_voxel_walk(*args, m, 1.0, off.ctypes.data_as(U64P), None, 0, C.byref(total)) == TDTK_EUNSUP
    assert (off == 7).all() and total.value == 5
    assert L.tdtk_voxel_walk(*args, m - 1, 1.0, off.ctypes.data_as(U64P), None, 0, C.byref(total)) == TDTK_EINVAL
    assert total.value == (m - 1) * c
    assert np.array_equal(off[:m], np.arange(m, dtype=np.uint64) * np.uint64(c)) and off[m] == 7
