"""Collision detection along a trajectory on the device (tdtk_collision_mark / _depth_closest / _depth_axis) against
collision_model's loops over the reference's own compiled queries.

Every comparison is exact: masks, counts and bit-equal float32 depths.  The expected values come from the live reference
library where oracle/_ref travelled (make_golden_collision.reference_case), else from the k13 fixture -- except `trips`,
whose 560,000 queries take the reference's single-thread loops half a minute: it is always compared with the fixture, which
the CPU tier pins to the live reference."""
import ctypes as C
import importlib.util
import os
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
pytestmark = pytest.mark.gpu

# query.hip's launch geometry, restated
Q_MAX_BLOCKS, Q_BLOCK, Q_SD = 2048, 128, 16
TDTK_EINVAL = -1


@pytest.fixture(scope="module")
def mg():
    spec = importlib.util.spec_from_file_location("make_golden_collision", os.path.join(G, "make_golden_collision.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def fx(mg):
    return mg.load()


def _crc(a):
    return zlib.crc32(np.ascontiguousarray(a, "<f4").tobytes())


def _device_case(tdtk, pts, model, frames, radius, bucket, cm, depths=True, kd=None):
    kd = kd or tdtk.KDtree(pts, bucket)
    mask, num = tdtk.handle_pointcloud(model, kd, frames, radius, cm)
    out = {"mask": mask, "num": num}
    if depths:
        out["d1"], out["unreached"] = tdtk.calculate_collidingdist(pts, mask, bucket, want_unreached=True)
        out["d2"] = tdtk.calculate_collidingdist2(model, pts, frames, mask, radius, bucket)
    return out


def _check(mg, fx, orc, key, case, bucket, cm, got, depths=True, live=True):
    pts = case[0]
    assert got["mask"].dtype == bool and got["mask"].shape == (len(pts),)
    if live and orc.have_ref():
        want = mg.reference_case(*case, bucket, cm, depths)
        assert np.array_equal(got["mask"], want["mask"]) and got["num"] == want["num"], key
        if depths:
            assert want["unreached"] == 0 and got["unreached"] == 0, key
            for d in ("d1", "d2"):
                assert got[d].dtype == np.float32 and np.array_equal(got[d].view(np.uint32), want[d].view(np.uint32)), (key, d)
        return
    assert np.array_equal(got["mask"], fx.mask(key, len(pts))) and got["num"] == fx.num(key), key
    if depths:
        assert got["unreached"] == 0, key
        for d in ("d1", "d2"):
            assert got[d].dtype == np.float32 and len(got[d]) == got["num"], (key, d)
            if key + "_" + d in fx.z.files:
                assert np.array_equal(got[d].view(np.uint32), fx.z[key + "_" + d].view(np.uint32)), (key, d)
            else:
                assert _crc(got[d]) == int(fx.z[key + "_" + d + "crc"][0]), (key, d)


@pytest.mark.parametrize("name", ["uniform", "duplicates", "lattice", "clusters", "seven", "one"])
def test_small_cases(tdtk, gpu, orc, mg, fx, name):
    """3 buckets x 2 marking methods x 2 depth methods per cloud (the marking alone on `seven` and `one`)"""
    case = mg.small_case(name)
    for b in mg.BUCKETS:
        kd = tdtk.KDtree(case[0], b)
        for cm in mg.METHODS:
            depths = name not in mg.NO_DEPTH
            got = _device_case(tdtk, *case, b, cm, depths, kd)
            _check(mg, fx, orc, "%s_b%d_m%d" % (name, b, cm), case, b, cm, got, depths)


def test_more_queries_than_lanes(tdtk, gpu, orc, mg, fx):
    """trips: 560,000 (frame, point) items on at most 262,144 lanes, so most lanes take a second and a third; and the same
    trajectory in two calls of 400 frames (401 with the shared one for the segments) marks the same set"""
    case = pts, model, frames, radius = mg.large_case("trips")
    assert len(model) * len(frames) > 2 * Q_MAX_BLOCKS * Q_BLOCK
    kd = tdtk.KDtree(pts, 20)
    for cm in mg.METHODS:
        got = _device_case(tdtk, *case, 20, cm, True, kd)
        _check(mg, fx, orc, "trips_b20_m%d" % cm, case, 20, cm, got, live=False)
        first, n1 = tdtk.handle_pointcloud(model, kd, frames[:400 + (cm == 2)], radius, cm)
        second, n2 = tdtk.handle_pointcloud(model, kd, frames[400:], radius, cm)
        assert n1 == first.sum() and n2 == second.sum() and 0 < n1 < got["num"] and 0 < n2 < got["num"]
        assert np.array_equal(first | second, got["mask"])


@pytest.mark.parametrize("bucket", [1, 20])
def test_deep_tree(tdtk, gpu, orc, mg, fx, bucket):
    """a tree about 80 levels deep: the walks run into the overflow stack behind the 16 LDS levels.  The natural depth trees
    are shallow (a thousand colliding points), so the axis depth also runs over a mask of fifteen points in sixteen, whose
    tree is as deep: there both of its walks share the overflow stack"""
    case = pts, model, frames, radius = mg.large_case("deep")
    kd = tdtk.KDtree(pts, bucket)
    assert kd.info()["max_depth"] > Q_SD
    for cm in mg.METHODS:
        got = _device_case(tdtk, *case, bucket, cm, True, kd)
        _check(mg, fx, orc, "deep_b%d_m%d" % (bucket, cm), case, bucket, cm, got)
    wide = mg.wide_mask(len(pts))
    assert tdtk.KDtree(pts[wide], bucket).info()["max_depth"] > Q_SD
    d2 = tdtk.calculate_collidingdist2(model, pts, frames, wide, radius, bucket)
    assert (d2 < np.sqrt(np.float32(1000.0))).sum() > 100
    if orc.have_ref():
        assert np.array_equal(d2.view(np.uint32), mg.depth_axis(pts, wide, model, frames, radius, bucket).view(np.uint32))
    else:
        assert _crc(d2) == int(fx.z["deep_b%d_wide_d2crc" % bucket][0])


def test_leaf_table_mode_and_contended_minima(tdtk, gpu, orc, mg, fx):
    """table: the leaf of 40,000 copies is marked whole, and the axis depth puts the minima of all lanes whose nearest point
    is a copy into the same 40,000 entries.  Twice: bit-identical and the reference's"""
    case = pts, model, frames, radius = mg.large_case("table")
    kd = tdtk.KDtree(pts, 20)
    for cm in mg.METHODS:
        got = _device_case(tdtk, *case, 20, cm, True, kd)
        assert got["num"] >= 40_000
        again = _device_case(tdtk, *case, 20, cm, True, kd)
        assert np.array_equal(again["mask"], got["mask"]) and again["num"] == got["num"]
        for d in ("d1", "d2"):
            assert np.array_equal(again[d].view(np.uint32), got[d].view(np.uint32)), d
        _check(mg, fx, orc, "table_b20_m%d" % cm, case, 20, cm, got)


def test_non_finite_model_points_and_frames(tdtk, gpu, orc, mg, fx):
    """NaN and +-inf in two frames and three model points: their queries mark nothing (what the reference's walks give), the
    others are unaffected"""
    case = pts, model, frames, radius = mg.large_case("nonfinite")
    assert not np.isfinite(model).all() and not np.isfinite(frames).all()
    kd = tdtk.KDtree(pts, 20)
    for cm in mg.METHODS:
        got = _device_case(tdtk, *case, 20, cm, True, kd)
        _check(mg, fx, orc, "nonfinite_b20_m%d" % cm, case, 20, cm, got)
    # method 1 without the non-finite rows: the same set
    good_p = np.setdiff1d(np.arange(len(model)), mg.NONFINITE_POINTS)
    good_f = np.setdiff1d(np.arange(len(frames)), mg.NONFINITE_FRAMES)
    all_rows, _ = tdtk.handle_pointcloud(model, kd, frames, radius, 1)
    finite_rows, _ = tdtk.handle_pointcloud(model[good_p], kd, frames[good_f], radius, 1)
    assert np.array_equal(all_rows, finite_rows)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_rejections_and_empty_trajectories(tdtk, gpu, mg):
    """every rejection: TDTK_EINVAL, tdtk_last_error() set, the outputs untouched; F == 0 (method 1) and F == 1 (method 2)
    are valid and mark nothing"""
    from importlib import import_module
    capi = import_module("3dtk_amd._capi")
    L = tdtk.lib()
    pts, model, frames, radius = mg.small_case("uniform")
    pts, model, frames = (np.ascontiguousarray(a) for a in (pts, model, frames))
    kd = tdtk.KDtree(pts, 20)
    M, P, F = len(pts), len(model), len(frames)
    dp = capi.dptr

    def mark(env=kd._h, model_=model, P_=P, frames_=frames, F_=F, radius_=radius, cm=1, mask_given=True, num_given=True):
        mask = np.full(M, 0xA5, np.uint8)
        num = C.c_uint64(0xDEADBEEF)
        rc = L.tdtk_collision_mark(env, dp(model_), P_, dp(frames_), F_, radius_, cm, _ptr(mask) if mask_given else None,
                                   C.byref(num) if num_given else None)
        return rc, mask, num.value

    bad = [dict(env=None), dict(model_=None), dict(frames_=None), dict(mask_given=False), dict(num_given=False), dict(P_=0),
           dict(radius_=0.0), dict(radius_=-1.0), dict(radius_=float("nan")), dict(radius_=float("inf")), dict(cm=0),
           dict(cm=3), dict(cm=2, F_=0)]
    for kw in bad:
        rc, mask, num = mark(**kw)
        assert rc == TDTK_EINVAL and L.tdtk_last_error(), kw
        assert (mask == 0xA5).all() and num == 0xDEADBEEF, kw
    for cm, F_ in ((1, 0), (2, 1)):
        rc, mask, num = mark(cm=cm, F_=F_)
        assert rc == 0 and not mask.any() and num == 0, (cm, F_)

    colliding, n = tdtk.handle_pointcloud(model, kd, frames, radius, 1)
    col = np.ascontiguousarray(colliding.astype(np.uint8))
    none, every = np.zeros(M, np.uint8), np.ones(M, np.uint8)

    def closest(env=pts, col_=col, dist_given=True, bucket=20):
        dist = np.full(M, -7.0, np.float32)
        unreached = C.c_uint64(0xDEADBEEF)
        rc = L.tdtk_collision_depth_closest(dp(env), M, _ptr(col_), bucket, 0, _ptr(dist) if dist_given else None,
                                            C.byref(unreached))
        return rc, dist, unreached.value

    for kw in (dict(env=None), dict(col_=None), dict(dist_given=False), dict(col_=none), dict(col_=every), dict(bucket=0)):
        rc, dist, unreached = closest(**kw)
        assert rc == TDTK_EINVAL and L.tdtk_last_error(), kw
        assert (dist == -7.0).all() and unreached == 0xDEADBEEF, kw

    def axis(env=pts, col_=col, model_=model, P_=P, frames_=frames, F_=F, radius_=radius, dist_given=True, bucket=20):
        dist = np.full(M, -7.0, np.float32)
        rc = L.tdtk_collision_depth_axis(dp(env), M, _ptr(col_), dp(model_), P_, dp(frames_), F_, radius_, bucket, 0,
                                         _ptr(dist) if dist_given else None)
        return rc, dist

    for kw in (dict(env=None), dict(col_=None), dict(model_=None), dict(frames_=None), dict(dist_given=False), dict(P_=0),
               dict(radius_=0.0), dict(radius_=float("nan")), dict(radius_=float("inf")), dict(col_=none), dict(bucket=0)):
        rc, dist = axis(**kw)
        assert rc == TDTK_EINVAL and L.tdtk_last_error(), kw
        assert (dist == -7.0).all(), kw
    # the mirror raises with the library's message
    with pytest.raises(tdtk.TdtkError):
        tdtk.handle_pointcloud(model, kd, frames, -1.0, 1)


def test_a_call_does_not_depend_on_the_calls_before_it(tdtk, gpu, orc, mg, fx):
    """after a larger environment at twice the radius (everything it marks and minimises stays in the workspaces), the
    smaller case gives what a first call gives"""
    big, small = mg.small_case("uniform"), mg.small_case("clusters")
    assert len(big[0]) > len(small[0])
    for cm in mg.METHODS:
        before = _device_case(tdtk, big[0], big[1], big[2], 2.0 * big[3], 20, cm)
        assert before["num"] > fx.num("uniform_b20_m%d" % cm)
        got = _device_case(tdtk, *small, 20, cm)
        _check(mg, fx, orc, "clusters_b20_m%d" % cm, small, 20, cm, got)
