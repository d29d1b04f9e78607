"""icp6D::match on the octree search tree (tdtk_icp_match_octree): the CPU tier.  tests/golden/k21_boctree_icp.npz holds the
loop iteration by iteration as the reference's own compiled BOctTree<double>::FindClosest drives it inside the oracle's match
(make_golden_boctree_icp.py).  Here the walk the device runs (oct_lane.h compiled for the host) goes through that same loop and
must give the same answers, query for query and pass for pass; the entry points' names, the kernels' resource remarks and the
Python mirror's dispatch are checked without a device.  Where the reference checkout is present the fixture is generated again."""
import importlib
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

import boctree_model as bm


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


@pytest.fixture(scope="module")
def lane(tmp_path_factory):
    return bm.host_lane(tmp_path_factory.mktemp("oct_host_icp"))


_models = {}


def _model(fx, name, voxel, early):
    key = (name, voxel, early)
    if key not in _models:
        _models[key] = bm.Model(fx[name + "_model"], voxel, early)
    return _models[key]


def test_fixture_is_what_the_generator_says(fx, orc):
    """under the size bound; the clouds are the generator's; every run has its arrays, consistent in length; the seam's runs
    have what the seam is for"""
    assert os.path.getsize(gen.OUT) <= gen.MAX_BYTES
    for name, (m, d, nrm) in gen.clouds().items():
        assert bm.same_bits(fx[name + "_model"], m) and bm.same_bits(fx[name + "_data"], d), name
        assert (nrm is None) == (name + "_normals" not in fx)
    keys = {"iterations", "converged", "pairs", "rms", "xf", "hash", "pos", "far"}
    assert set(fx) == {gen.prefix(r) + k for r in gen.RUNS for k in keys} | {k for k in fx if k.endswith(("_model", "_data", "_normals"))}
    for run in gen.RUNS:
        p = gen.prefix(run)
        passes = len(fx[p + "pairs"])
        assert len(fx[p + "hash"]) == len(fx[p + "pos"]) == len(fx[p + "far"]) == passes
        assert len(fx[p + "rms"]) == len(fx[p + "xf"]) and passes - len(fx[p + "rms"]) in (0, 1)
        assert fx[p + "pos"].shape == (passes, len(fx[run[0] + "_data"]))
        assert np.array_equal((fx[p + "pos"] >= 0).sum(1), fx[p + "pairs"])
        if run[0] == "seam" and run[3] != gen.NAPX:
            assert fx[p + "far"][:2].max() == 0 and fx[p + "far"][2:].min() >= 50       # from iteration 2 on: stopped searches
    assert fx[gen.prefix(gen.RUNS[10]) + "converged"] == 1


@pytest.mark.parametrize("run", gen.RUNS, ids=RUN_IDS)
def test_host_lane_loop_equals_fixture(fx, lane, orc, run):
    """oct_lane.h's FindClosest inside the oracle's loop: positions, hashes and pairs of every pass, iterations and converged
    equal the fixture's exactly (the poses come out of the same arithmetic on the same pairs: by bits)"""
    name, voxel, early = run[:3]
    m = _model(fx, name, voxel, early)
    model = fx[name + "_model"]
    rep_leaf = gen.mo.rep_index(model, model[m.leaf])

    def find(q, maxd2):
        return bm.lane_find(lane, m, q, maxd2)[0]
    got = gen.loop(run, gen.cloud_of(fx, name), rep_leaf, find)
    p = gen.prefix(run)
    for k in ("iterations", "converged", "pairs", "hash", "pos", "far"):
        assert got[k].dtype == fx[p + k].dtype and np.array_equal(got[k], fx[p + k]), (p, k)
    assert bm.same_bits(got["rms"], fx[p + "rms"]) and bm.same_bits(got["xf"], fx[p + "xf"])


def test_the_two_entry_points_are_declared_and_bound(tdtk):
    """tdtk_icp_match_octree and _rnd: in the header, in EXPORTS with tdtk_icp_match's argument lists, in the library -- and
    not under the tdtk_octree_ prefix"""
    capi = sys.modules["3dtk_amd._capi"]
    hdr = open(os.path.join(bm.ROOT, "include", "tdtk_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for sym, like in (("tdtk_icp_match_octree", "tdtk_icp_match"), ("tdtk_icp_match_octree_rnd", "tdtk_icp_match_rnd")):
        assert sym in capi.EXPORTS
        assert re.search(r"\bint %s\(const tdtk_octree\* model," % sym, hdr), sym
        assert getattr(tdtk.lib(), sym).argtypes == getattr(tdtk.lib(), like).argtypes
    assert len([s for s in capi.EXPORTS if s.startswith("tdtk_octree_")]) == 9


def test_loop_kernels_spill_nothing_and_the_walk_keeps_its_occupancy():
    """the compiler's resource remarks (csrc/Makefile keeps them): neither kernel of the loop spills or uses scratch, the walk
    leaves room for at least four waves per SIMD"""
    path = os.path.join(bm.ROOT, "3dtk_amd", "csrc", "octree.resource.txt")
    if not os.path.exists(path):
        pytest.skip("no build in this tree (octree.resource.txt is written by the Makefile)")
    blocks = {b.split()[0]: b for b in open(path).read().split("remark: Function Name: ")[1:]}
    for want, count in (("k_oct_loop_prepare", 1), ("k_oct_loop_find", 2)):          # the walk: with and without -R's bytes
        mine = [b for n, b in blocks.items() if want in n]
        assert len(mine) == count, want
        for b in mine:
            for key in ("VGPRs Spill", "SGPRs Spill", r"ScratchSize \[bytes/lane\]"):
                m = re.search(key + r": (\d+)", b)
                assert m and int(m.group(1)) == 0, (want, key)
    for find in [b for n, b in blocks.items() if "k_oct_loop_find" in n]:
        assert int(re.search(r"VGPRs: (\d+)", find).group(1)) <= 128 and int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", find).group(1)) >= 4


# ---- the Python mirror, without a device ---------------------------------------------------------------------------------
def _scan(tdtk, nns=None):
    s = tdtk.Scan([0, 0, 0], [0, 0, 0], np.arange(30.0).reshape(10, 3))
    if nns is not None:
        s.setSearchTreeParameter(nns)
    return s


def test_set_search_tree_parameter(tdtk):
    """0 and 2 are taken, 1 and 3 are the reference's types this library has not: its own message; setting drops the tree"""
    s = _scan(tdtk)
    assert s.nns_method == 0
    for bad in (1, 3, -1, 4):
        with pytest.raises(RuntimeError, match="SearchTree type not implemented"):
            s.setSearchTreeParameter(bad)
        assert s.nns_method == 0
    s.kd = object()
    assert s.setSearchTreeParameter(2, 17) is s and s.nns_method == 2 and s.bucketSize == 17 and s.kd is None
    s.kd = object()
    s.setSearchTreeParameter(0)
    assert s.nns_method == 0 and s.bucketSize == 20 and s.kd is None


def test_get_search_tree_builds_the_type_that_was_set(tdtk, monkeypatch):
    """type 2: BOctTree.from_scan(handle, n, 10.0, earlystop) -- basicScan.cc:714-719 -- over the resident scan; type 0: the
    k-d tree as before"""
    mod = sys.modules["3dtk_amd.slam6d"]
    calls = []

    class FakeOct(mod.BOctTree):
        @classmethod
        def from_scan(cls, handle, n, voxelSize=10.0, earlystop=True, device=0):
            calls.append(("oct", handle, n, voxelSize, earlystop, device))
            return cls.__new__(cls)

    class FakeKd(mod.KDtree):
        @classmethod
        def from_scan(cls, handle, n, bucketSize=20, device=0):
            calls.append(("kd", handle, n, bucketSize, device))
            return cls.__new__(cls)
    monkeypatch.setattr(mod, "BOctTree", FakeOct)
    monkeypatch.setattr(mod, "KDtree", FakeKd)
    monkeypatch.setattr(mod.Scan, "handle", property(lambda self: "H"))
    s = _scan(tdtk, 2)
    t = s.getSearchTree()
    assert isinstance(t, FakeOct) and s.getSearchTree() is t and calls == [("oct", "H", 10, 10.0, True, 0)]
    s.setSearchTreeParameter(0)
    assert isinstance(s.getSearchTree(), FakeKd) and calls[1] == ("kd", "H", 10, 20, 0)


def test_kd_only_callers_refuse_an_octree_scan_by_name(tdtk, monkeypatch):
    """everything that hands a tdtk_tree to the library raises TDTK_EUNSUP for a scan of type 2, names itself, builds no tree
    and calls nothing"""
    mod = sys.modules["3dtk_amd.slam6d"]
    gs = importlib.import_module("3dtk_amd.graphslam")

    real = tdtk.lib()

    class HostOnly:          # the matrix helpers of the host (tdtk_host_*) pass, everything else is a call that must not happen
        def __getattr__(self, name):
            if name.startswith("tdtk_host_"):
                return getattr(real, name)

            def f(*args):
                raise AssertionError("the library was called")
            return f
    monkeypatch.setattr(mod, "lib", lambda: HostOnly())
    monkeypatch.setattr(mod.Scan, "getSearchTree", lambda self: (_ for _ in ()).throw(AssertionError("a tree was built")))
    a, b, c = _scan(tdtk, 2), _scan(tdtk, 2), _scan(tdtk, 2)
    icp = tdtk.icp6D(tdtk.icp6D_QUAT(True), 5.0, 3, quiet=True)
    g = mod.Graph.chain(3)
    attempts = {
        "icp6D.Point_Point_Error": lambda: icp.Point_Point_Error(a, b, 5.0),
        "icp6D.match with a MetaScan as data": lambda: icp.match(a, mod.MetaScan([b, c])),
        "MetaScan.getSearchTree": lambda: mod.MetaScan([a, b]).getSearchTree(),
        "Scan.getPtPairs": lambda: mod.Scan.getPtPairs(a, b),
        "covarianceEuler": lambda: mod.covarianceEuler(a, b, 25.0),
        "ELCH (close_loop)": lambda: mod.elch6Deuler(True, tdtk.icp6D_QUAT(True), 5.0, 3).close_loop([a, b, c], 0, 2, [(0, 1), (1, 2)]),
        "computeGraph6Dautomatic": lambda: mod.computeGraph6Dautomatic([a, b, c], 10),
        "doGraphSlam6D": lambda: gs.lum_iteration_native(g, [a, b, c], 25.0),
    }
    frames = len(b.frames)
    for who, call in attempts.items():
        with pytest.raises(tdtk.TdtkError) as e:
            call()
        assert e.value.code == -5 and who in str(e.value), who
    assert len(b.frames) == frames          # refused before the MetaScan was touched
    # a k-d scan passes the gate (and reaches the library, which this test has taken away)
    k = _scan(tdtk, 0)
    monkeypatch.setattr(mod.Scan, "getSearchTree", lambda self: type("T", (), {"_h": 7})())
    assert k.kdHandle("x") == 7
    with pytest.raises(AssertionError, match="the library was called"):
        icp.Point_Point_Error(k, b, 5.0)


def test_icp6d_match_dispatches_on_the_trees_type(tdtk, monkeypatch):
    """an octree model scan goes to tdtk_icp_match_octree / _rnd, a k-d one to tdtk_icp_match / _rnd: the same arguments"""
    mod = sys.modules["3dtk_amd.slam6d"]
    called = []

    real = tdtk.lib()

    class Lib:
        def __getattr__(self, name):
            if name.startswith("tdtk_host_"):
                return getattr(real, name)
            if name == "tdtk_icp_index_hashes":
                return lambda on: 0

            def f(*args):
                called.append((name, len(args)))
                return 0
            return f
    monkeypatch.setattr(mod, "lib", lambda: Lib())
    monkeypatch.setattr(mod.Scan, "handle", property(lambda self: "H"))
    for nns, tree in ((2, mod.BOctTree), (0, mod.KDtree)):
        prev, cur = _scan(tdtk, nns), _scan(tdtk, nns)
        prev.kd = tree.__new__(tree)
        prev.kd._h = None
        for rnd in (1, 3):
            icp = tdtk.icp6D(tdtk.icp6D_QUAT(True), 5.0, 4, quiet=True, rnd=rnd, nns_method=nns)
            assert icp.nns_method == nns
            icp.match(prev, cur)
    assert called == [("tdtk_icp_match_octree", 9), ("tdtk_icp_match_octree_rnd", 10), ("tdtk_icp_match", 9), ("tdtk_icp_match_rnd", 10)]


def test_open_directory_passes_the_type_on(tdtk, tmp_path, monkeypatch):
    mod = sys.modules["3dtk_amd.slam6d"]
    monkeypatch.setattr(mod, "read_pose", lambda f: (np.zeros(3), np.zeros(3)))
    monkeypatch.setattr(mod, "read_uos", lambda f, a, b: np.arange(12.0).reshape(4, 3))
    for i in range(2):
        (tmp_path / ("scan%03d.3d" % i)).write_text("")
        (tmp_path / ("scan%03d.pose" % i)).write_text("")
    was = mod.Scan.allScans
    try:
        assert [s.nns_method for s in mod.openDirectory(str(tmp_path), nns_method=2)] == [2, 2]
        assert [s.nns_method for s in mod.openDirectory(str(tmp_path))] == [0, 0]
        with pytest.raises(RuntimeError, match="SearchTree type not implemented"):
            mod.openDirectory(str(tmp_path), nns_method=1)
    finally:
        mod.Scan.allScans = was


def test_fixture_equals_the_reference(fx, orc):
    """the generator, run again on the live reference, gives the stored arrays"""
    if not gen.have_ref():
        pytest.skip("no reference checkout (src/slam6d/Boctree.cc)")
    got = gen.compute()
    assert sorted(got) == sorted(fx)
    for k in fx:
        assert got[k].dtype == fx[k].dtype and got[k].shape == fx[k].shape, k
        same = bm.same_bits(got[k], fx[k]) if got[k].dtype == np.float64 else np.array_equal(got[k], fx[k])
        assert same, k
