"""The dynamic kd-forest on the device (tdtk_forest_*, 3dtk_amd.BkdTree), in the product library: every case of the fixture
k19_bkd.npz (tests/golden/make_golden_bkd.py: the reference's compiled bkd.cc) through the C ABI and its Python mirror, the
layout cases reached three ways; the known-answer tests of testing/kdtree/bkdtree.cc restated with fixed seeds; a tree in table
mode; the error paths; and, after the last case, a fresh tdtk_tree_create whose answers still hold -- the pool blocks the
forests handed back were sound."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import bkd_model
from bkd_replay import replay, ways

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


MK = _load("make_golden_bkd")
CASES = {c.name: c for c in MK.cases()}
RUNS = [(n, w) for n, c in CASES.items() for w in (("one", "single", "ragged") if n.startswith("lay_") else ("one",))]


@pytest.fixture(scope="module")
def fx():
    return MK.load()


class DeviceForest:
    """3dtk_amd.BkdTree under the replay's interface; every d2 it returns is checked against Dist2 of the id on the way"""

    def __init__(self, tdtk, case):
        self.xyz = case.P[:case.ctor].copy()
        self.t = tdtk.BkdTree(case.P[:case.ctor], case.b) if case.ctor else tdtk.BkdTree(case.b)

    def insert(self, pts):
        ids = self.t.insert(pts)
        assert ids.tolist() == list(range(len(self.xyz), len(self.xyz) + len(pts)))
        self.xyz = np.concatenate([self.xyz, pts])

    def remove(self, pts):
        return self.t.remove(pts).tolist(), None

    def layout(self):
        counts, fill, size, _ = self.t.info()
        per = [np.sort(self.t.collect(s)[0]).tolist() for s in range(len(counts))]
        bids, bxyz = self.t.collect(-1)
        assert [len(p) for p in per] == counts and len(bids) == fill and size == sum(counts) + fill == self.t.size()
        assert np.array_equal(bxyz, self.xyz[bids])
        ids, xyz = self.t.collectPts()
        assert np.array_equal(xyz, self.xyz[ids]) and sorted(ids.tolist()) == sorted([x for p in per for x in p] + bids.tolist())
        return counts, [x for p in per for x in p], bids.tolist()

    def _d2(self, ids, Q):
        d = self.xyz[np.maximum(ids, 0)] - Q
        return np.where(ids >= 0, (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], -1.0)

    def find_closest(self, Q, md2):
        idx, d2 = self.t.FindClosest(Q, md2)
        assert np.array_equal(d2, self._d2(idx, Q))
        return idx, d2

    def knn(self, Q, k):
        idx, d2 = self.t.kNearestNeighbors(Q, k)
        assert np.array_equal(d2, self._d2(idx, Q[:, None, :]))
        return idx, d2

    def fixed_range(self, Q, r2):
        off, ids, d2 = self.t.fixedRangeSearch(Q, r2)
        assert np.array_equal(d2, self._d2(ids, np.repeat(Q, np.diff(off.astype(np.int64)), axis=0)))
        return off.astype(np.int64), ids

    def close(self):
        self.t.close()


@pytest.mark.parametrize("name,way", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_case_against_the_fixture(tdtk, gpu, fx, name, way):
    case = CASES[name]
    f = DeviceForest(tdtk, case)
    replay(MK, case, fx, f, calls=lambda a, b: dict(ways(MK, case, a, b))[way])
    f.close()


# ---- testing/kdtree/bkdtree.cc, restated with fixed seeds -----------------------------------------------------------------------
def _kat_tree(tdtk, n, seed):
    t = tdtk.BkdTree(20)
    t.insert([0.0, 0.0, 0.0])
    t.insert(np.random.default_rng(seed).uniform(10.0, 500.0, (n, 3)))
    return t


def test_kat_insertion_closest_remove(tdtk, gpu):
    t = _kat_tree(tdtk, 10000, 11)
    assert t.size() == 10001                                            # simple_insertion_test
    idx, d2 = t.FindClosest([[0.0, 0.0, 0.0001]], bkd_model.DBL_MAX)      # simple_closest_test
    assert idx.tolist() == [0] and d2[0] == 0.0001 * 0.0001
    assert t.remove([0.0, 0.0, 0.0]).tolist() == [0]                      # simple_remove_test
    assert t.remove([0.0, 0.0, 0.0]).tolist() == [-1] and t.size() == 10000
    t.close()


def test_kat_consistency_and_knearest(tdtk, gpu):
    t = tdtk.BkdTree(3)                                                  # simple_consistency_check
    for i in range(10, 101, 10):
        t.insert([float(i)] * 3)
    assert t.remove([20.0, 20.0, 20.0]).tolist() == [1]
    idx, d2 = t.FindClosest([[20.0, 20.0, 20.0]], bkd_model.DBL_MAX)
    assert idx.tolist() in ([0], [2]) and d2[0] == 300.0
    t.close()
    t = _kat_tree(tdtk, 100, 12)                                         # simple_knearest_check
    second = t.insert([0.0, 0.0, 0.001])[0]
    idx, d2 = t.kNearestNeighbors([[0.00001, 0.0, 0.0]], 2)
    assert idx.tolist() == [[0, second]]
    t.close()


# ---- beyond the fixture -----------------------------------------------------------------------------------------------------
def test_a_tree_in_table_mode(tdtk, gpu):
    """40 000 copies of one coordinate are one leaf of more points than a packed child reference counts: the tree keeps its
    leaves in a table.  Three copies go; k-NN and the radius count the rest"""
    rng = np.random.default_rng(13)
    Z = np.array([2.5, 2.5, -1.0])
    P = rng.uniform(-10.0, 10.0, (40050, 3))
    P[rng.permutation(40050)[:40000]] = Z
    t = tdtk.BkdTree(P, 20)
    counts, fill, size, table = t.info()
    assert counts[-1] == 40050 and sum(counts) == 40050 and table == [len(counts) - 1]
    got = t.remove([Z, Z, Z])
    assert (got >= 0).all() and len(set(got.tolist())) == 3 and np.array_equal(P[got], np.tile(Z, (3, 1)))
    assert t.size() == 40047
    idx, d2 = t.kNearestNeighbors([Z], 64)
    assert (d2 == 0.0).all() and len(set(idx[0].tolist())) == 64 and not set(idx[0].tolist()) & set(got.tolist())
    off, ids, d2 = t.fixedRangeSearch([Z, [100.0, 0.0, 0.0]], 1e-6)
    assert off.tolist() == [0, 39997, 39997] and len(set(ids.tolist())) == 39997 and not set(ids.tolist()) & set(got.tolist())
    # a merge collects the tree: its live points, and only those
    more = rng.uniform(-10.0, 10.0, (20 * 2 ** (len(counts) - 1), 3))
    t.insert(more)
    counts2, fill2, size2, _ = t.info()
    assert counts2 == [0] * len(counts) + [40047 + len(more)] and fill2 == 0
    ids, xyz = t.collectPts()
    assert len(ids) == size2 and not set(ids.tolist()) & set(got.tolist()) and np.array_equal(xyz, np.concatenate([P, more])[ids])
    t.close()


def test_remove_by_mask_over_ids(tdtk, gpu):
    P = np.random.default_rng(14).uniform(-10.0, 10.0, (500, 3))
    t = tdtk.BkdTree(20)
    t.insert(P)
    mask = np.zeros(500, bool)
    mask[::7] = True
    got = t.remove(mask)
    assert sorted(got.tolist()) == np.nonzero(mask)[0].tolist() and t.size() == 500 - mask.sum()
    idx, _ = t.FindClosest(P, 1e-12)
    assert np.array_equal(idx, np.where(mask, -1, np.arange(500)))        # (500 = 25 * 20: the buffer is empty, Q1 has nothing to answer with)
    t.close()


def test_errors_change_nothing(tdtk, gpu):
    L = tdtk.lib()
    P = np.random.default_rng(15).uniform(-10.0, 10.0, (50, 3))
    t = tdtk.BkdTree(20)
    t.insert(P)
    before = (t.info(), t.collectPts()[0].tolist())
    bad = P[:5].copy()
    bad[3, 1] = np.nan
    for call in (lambda: t.insert(bad), lambda: t.remove(bad), lambda: t.kNearestNeighbors(P[:2], 0)):
        with pytest.raises(tdtk.TdtkError) as e:
            call()
        assert e.value.code == -1                                         # TDTK_EINVAL
    with pytest.raises(tdtk.TdtkError) as e:
        t.kNearestNeighbors(P[:2], 65)
    assert e.value.code == -5 and "capacity" in str(e.value)          # TDTK_EUNSUP
    assert (t.info(), t.collectPts()[0].tolist()) == before
    with pytest.raises(tdtk.TdtkError):
        tdtk.BkdTree(np.zeros((0, 3)), 20)
    with pytest.raises(tdtk.TdtkError):
        tdtk.BkdTree(0)
    # the list protocol of tdtk_fixed_range_search: too small a capacity fills offsets and the total
    off = np.zeros(3, np.uint64)
    total = C.c_uint64(0)
    rc = L.tdtk_forest_fixed_range(t._h, P[:2].ctypes.data_as(C.POINTER(C.c_double)), 2, 1e30, off.ctypes.data_as(C.POINTER(C.c_uint64)),
                                   None, None, 0, C.byref(total))
    assert rc != 0 and total.value == 100 and off.tolist() == [0, 50, 100]
    t.close()
    # an empty forest answers nothing
    e0 = tdtk.BkdTree(20)
    assert e0.size() == 0 and e0.FindClosest(P[:3], 1e30)[0].tolist() == [-1] * 3 and e0.remove(P[:2]).tolist() == [-1, -1]
    assert (e0.kNearestNeighbors(P[:3], 4)[0] == -1).all() and e0.fixedRangeSearch(P[:3], 1e30)[0].tolist() == [0, 0, 0, 0]
    e0.close()


def test_zz_a_fresh_tree_after_the_forests(tdtk, gpu):
    """after every forest above has come and gone in this context: a new kd-tree over pool blocks they handed back"""
    rng = np.random.default_rng(16)
    P = rng.uniform(-10.0, 10.0, (30000, 3))
    Q = rng.uniform(-10.0, 10.0, (600, 3))
    kd = tdtk.KDtree(P, 20)
    idx, d2 = kd.FindClosestBatch(Q, 25.0)
    d = ((P[None, :, 0] - Q[:, None, 0]) ** 2 + (P[None, :, 1] - Q[:, None, 1]) ** 2) + (P[None, :, 2] - Q[:, None, 2]) ** 2
    assert np.array_equal(idx, d.argmin(1)) and np.array_equal(d2, d.min(1))
