"""The voxel grid and peopleremover on the paths the first fixture does not reach (tests/golden/k18_peopleremover_paths.npz,
made by tests/golden/make_golden_peopleremover_paths.py): the CPU tier.  The lane code under the host shim, through the driver
of test_peopleremover_host.py, against the fixture on every case; where the reference checkout is present, the live compiled
reference against the fixture as well; and what each directed case is there for, stated from its inputs and the fixture with
the Python restatement of the key arithmetic (tests/voxel_keys.py), which is compared with the lane code's."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import host_lane                                            # noqa: E402
import voxel_keys as vk                                     # noqa: E402
import make_golden_peopleremover_paths as paths             # noqa: E402
import test_peopleremover_host as first                     # noqa: E402  (its driver, its runners)

gold = paths.gold

KEYS = r"""
extern "C" void pl_keys(const int64_t* xyz, size_t n, uint64_t* key, uint64_t* hash, int64_t* back)
{
  for (size_t i = 0; i < n; ++i) {
    key[i] = vox_key(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    hash[i] = vox_hash(key[i] >> 6);
    vox_unkey(key[i], back[3 * i], back[3 * i + 1], back[3 * i + 2]);
  }
}
"""


@pytest.fixture(scope="module")
def lane(tmp_path_factory):
    L = host_lane.build("#include <array>\n" + first.DRIVER + KEYS, tmp_path_factory.mktemp("voxel_paths_lane"), "voxel_paths_lane")
    L.pl_walk.restype = C.c_long
    L.pl_walk.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_long, C.c_void_p]
    L.pl_run.restype = C.c_long
    L.pl_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_uint64, C.c_uint32, C.c_int,
                         C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]
    L.pl_keys.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def fixture():
    return paths.load()


WALKS = {name: (vs, s, e) for name, vs, s, e in paths.walk_cases()}
RUNS = {c["name"]: c for c in paths.pipeline_cases()}
RANDOM = [n for n in RUNS if n.startswith("rand")]


def test_the_fixture_holds_every_case_and_no_other(fixture):
    assert list(fixture.run_at) == list(RUNS) and list(fixture.walk_at) == [w[0] for w in paths.walk_cases()]
    assert len(RANDOM) == paths.N_RANDOM and len(WALKS) == len(paths.WALK_VS) * len(paths.WALK_KINDS)
    assert all(len(s) == 64 for _, s, _ in WALKS.values())


@pytest.mark.parametrize("name", sorted(WALKS))
def test_walk_lane_code_matches_the_fixture(lane, fixture, name):
    vs, s, e = WALKS[name]
    assert fixture.walk_sha(name) == gold.digest([s, e]), "the inputs are not the ones the fixture was made from"
    counts, vox = first.host_walk(lane, s, e, vs)
    rc, rv = fixture.walk(name)
    assert np.array_equal(counts, rc)
    assert np.array_equal(vox, rv)


def test_long_ray_count_matches_the_fixture(lane, fixture):
    assert np.array_equal(fixture.long_ray, paths.LONG_RAY)
    s, e = np.ascontiguousarray(paths.LONG_RAY[0]), np.ascontiguousarray(paths.LONG_RAY[1])
    assert lane.pl_walk(s.ctypes.data, e.ctypes.data, 1.0, 0, None) == fixture.long_count
    assert 60000 <= fixture.long_count < 65536


def host_run(lane, case):
    """the driver's cluster_size has 32 bits: the clamp of tdtk_peopleremover (api_voxel.cpp) in front of it"""
    return first.run_host(lane, dict(case, cluster=min(case["cluster"], 0xFFFFFFFF)))


def _assert_equal(got, want, name):
    assert np.array_equal(got[2], want[2]), (name, got[2], want[2])
    assert np.array_equal(got[1], want[1]), name
    assert np.array_equal(got[0], want[0]), name


@pytest.mark.parametrize("name", [n for n in RUNS if not n.startswith("rand")])
def test_pipeline_lane_code_matches_the_fixture(lane, fixture, name):
    _assert_equal(host_run(lane, RUNS[name]), fixture.run(RUNS[name]), name)


def test_random_scenes_lane_code_matches_the_fixture(lane, fixture):
    for name in RANDOM:
        _assert_equal(host_run(lane, RUNS[name]), fixture.run(RUNS[name]), name)


@pytest.mark.skipif(not gold.have_ref(), reason="needs the reference checkout (TDTK_REF)")
def test_live_reference_matches_the_fixture(fixture):
    for name, (vs, s, e) in WALKS.items():
        counts, vox = gold.Ref.walk(s, e, vs)
        rc, rv = fixture.walk(name)
        assert np.array_equal(counts, rc) and np.array_equal(vox, rv), name
    s, e = np.ascontiguousarray(paths.LONG_RAY[0]), np.ascontiguousarray(paths.LONG_RAY[1])
    assert gold.ref_lib().pr_walk(s.ctypes.data, e.ctypes.data, 1.0, 0, None) == fixture.long_count
    res = {}
    for name, case in RUNS.items():
        res[name] = gold.Ref.run(case)
        _assert_equal(res[name], fixture.run(case), name)
    paths.check_cases(RUNS, res)


def test_cases_hold_what_they_are_there_for(fixture):
    """from the inputs, the fixture and tests/voxel_keys.py alone (check_cases says what is asserted, group by group)"""
    paths.check_cases(RUNS, {name: fixture.run(case) for name, case in RUNS.items()})
    # f: every voxel size of every kind; the far rays lie beyond half the packable range; the boundary rays start on k * vs
    for vs in paths.WALK_VS:
        for kind in paths.WALK_KINDS:
            counts, vox = fixture.walk("%s_v%g" % (kind, vs))
            assert len(counts) == 64 and counts.sum() > 64
        assert np.abs(fixture.walk("far_v%g" % vs)[1]).min() >= 499000
        assert np.abs(fixture.walk("far_v%g" % vs)[1]).max() > 1000000
        _, s, e = WALKS["boundary_v%g" % vs]
        k = np.rint(s / vs)
        assert np.array_equal(k * vs, s) and np.abs(k).max() <= 300 and np.abs(np.rint(e / vs) - k).max() <= 9
        _, s, e = WALKS["lattice8_v%g" % vs]
        assert 0.1 < ((e - s) == 0).mean() < 0.3
    assert os.path.getsize(paths.OUT) <= paths.MAX_BYTES


def test_restated_keys_and_hash_are_the_lane_codes(lane):
    rng = np.random.default_rng(64)
    lim = (1 << 20) - 4
    xyz = np.concatenate([rng.integers(-lim + 1, lim, (9000, 3)), rng.integers(-40, 40, (1000, 3))]).astype(np.int64)
    key, hsh, back = np.zeros(len(xyz), np.uint64), np.zeros(len(xyz), np.uint64), np.zeros((len(xyz), 3), np.int64)
    lane.pl_keys(xyz.ctypes.data, len(xyz), key.ctypes.data, hsh.ctypes.data, back.ctypes.data)
    assert np.array_equal(back, xyz)
    assert [vk.vox_key(*v) for v in xyz.tolist()] == key.tolist()
    assert [vk.vox_hash(k >> 6) for k in key.tolist()] == hsh.tolist()
    for v in xyz[:200].tolist():
        assert vk.brick_key(v[0] >> 2, v[1] >> 2, v[2] >> 2) == vk.vox_key(*v) >> 6
