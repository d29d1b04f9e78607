"""GPU tier of the device tree build's hand-over decisions (build.hip: size_up_hand_over, look, hand_over,
enqueue_finishers; the finishers' tables in build_finish.inc).  Every row of tests/build_path_model.ROWS is a cloud that
reaches one outcome -- "one more level", the retry with its looks refused by the size, by the count or by both, a
hand-over with exactly fin_cap nodes, the retry ending in each combination of the size-staged finishers, the 31-level
guard, a subtree exactly as deep as the tables and one level deeper (redone by levels), the bucket bound -- by its shape
alone: no lab switch is set.  test_build_path_host.py pins, without a GPU, which path each cloud must take; here the build
reports the path it took (KDtree.build_path()), and the tree must be the host builder's record for record, its nearest
neighbours the oracle's bit for bit, and the next tree built in the same context (arena and pool reused) sound too."""
import functools

import numpy as np
import pytest

import build_path_model as B

pytestmark = pytest.mark.gpu

MAXD2 = (1e18, 1.0)


@functools.lru_cache(maxsize=None)
def _queries(name):
    """600 queries into the dense part of the cloud (buckets of thousands of points closer together than 0.01: the load
    of the padded bucket groups and the 16-bit shadows) and over the field; None for the comb-in-field clouds."""
    rng = np.random.default_rng(907)
    if name.startswith("lopsided"):
        c = np.array([300.0, -200.0, 50.0])
        q = [c + rng.normal(0, 1e-3, (200, 3)), c + rng.normal(0, 10.0, (200, 3)), rng.uniform(-1000, 1000, (200, 3))]
    elif name.startswith("comb-on-top"):
        teeth = np.outer(2.0 ** np.arange(40), [1.0, 0.5, 0.25])
        p = B.cloud(name)
        q = [teeth[rng.integers(0, 40, 200)] + rng.normal(0, 1e-3, (200, 3)), teeth[rng.integers(0, 40, 200)] + rng.normal(0, 1.0, (200, 3)),
             rng.uniform(-1000, 1000, (200, 3)),
             rng.uniform(p.min(axis=0), p.max(axis=0), (50, 3))]     # ... and 50 over the whole box, 2^499 wide
    else:
        return None
    return np.ascontiguousarray(np.concatenate(q))


@functools.lru_cache(maxsize=None)
def _next_cloud():
    return np.random.default_rng(5).uniform(-50, 50, (40000, 3))


@functools.lru_cache(maxsize=None)
def _expected(tdtk, orc, name, bucket):
    """the prediction of the path and the oracle's neighbours: once per (cloud, bucket), shared by the two libraries"""
    p = B.cloud(name) if name else _next_cloud()
    nseg, maxn = tdtk.host_tree_levels(p, bucket)
    want = B.predict(nseg, maxn, len(p), bucket)
    q = _queries(name) if name else None
    nn = None
    if q is not None:
        T = orc.Tree(p, bucket)
        nn = [T.find_closest(q, md2, 8) for md2 in MAXD2]
    return want, nn


def _check_row(tdtk, orc, name, bucket):
    p = B.cloud(name)
    want, nn = _expected(tdtk, orc, name, bucket)
    kd = tdtk.KDtree(p, bucket)
    assert kd.verify() == [0, 0, 0, 0]
    got = kd.build_path()
    assert got.pop("respeculated") == 0
    assert got == want
    if nn is not None:
        q = _queries(name)
        for md2, (oi, od) in zip(MAXD2, nn):
            gi, gd = kd.FindClosestBatch(q, md2)
            assert np.array_equal(gi, oi) and np.array_equal(gd, od), md2
    kd2 = tdtk.KDtree(_next_cloud(), 20)
    assert kd2.verify() == [0, 0, 0, 0]
    # (a balanced cloud: the planned level, one launch of the full-size finisher, nothing else -- and nothing left over from
    #  the report of the build before it)
    want2 = _expected(tdtk, orc, "", 20)[0]
    assert (want2["planned_level"], want2["handed_level"], want2["fin_nodes"], want2["finishers"]) == (5, 5, 32, 4)
    assert kd2.build_path() == dict(want2, respeculated=0)


@pytest.mark.parametrize("row,name,bucket", B.ROWS, ids=B.ROW_IDS)
def test_device_build_takes_the_predicted_path(tdtk, orc, gpu, row, name, bucket):
    _check_row(tdtk, orc, name, bucket)


def test_device_build_takes_the_predicted_paths_under_the_arena_guards(tdtk, orc, gpu, lab):
    """The same rows in the lab library, where every region of the build's arena has guard bytes behind it that the build
    checks when it is done: a path that writes past a region's end fails here even where the tree comes out right."""
    for row, name, bucket in B.ROWS:
        try:
            _check_row(tdtk, orc, name, bucket)
        except AssertionError as e:
            raise AssertionError("%s, bucket %d (lab library): %s" % (row, bucket, e)) from e
