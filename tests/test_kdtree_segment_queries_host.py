"""The cylinder, box and segment queries on the kd-tree (tdtk_fixed_range_search_along_dir / _between, tdtk_aabb_search,
tdtk_segment_search_all / _nearest): the CPU tier.  The fixture k10_kdtree_segment_queries.npz against the reference library
and against the walks' leaf predicates, the declared entry points, and the resource remarks of the new kernels."""
import importlib
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")

EXPORTS = ("tdtk_fixed_range_search_along_dir", "tdtk_fixed_range_search_between", "tdtk_aabb_search",
           "tdtk_segment_search_all", "tdtk_segment_search_nearest")
METHODS = ("fixedRangeSearchAlongDir", "fixedRangeSearchBetween2Points", "AABBSearch", "segmentSearch_all",
           "segmentSearch_1NearestPoint")


def _ms():
    spec = importlib.util.spec_from_file_location("make_golden_segments", os.path.join(G, "make_golden_segments.py"))
    ms = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ms)
    return ms


def _fixture():
    return np.load(os.path.join(G, "k10_kdtree_segment_queries.npz"))


def _lists(z, name, b, kind):
    return z["%s_b%d_%s_off" % (name, b, kind)].astype(np.uint64), z["%s_b%d_%s_idx" % (name, b, kind)].astype(np.int32)


def _rows(off, idx):
    return [idx[int(off[i]):int(off[i + 1])].tolist() for i in range(len(off) - 1)]


def test_fixture_is_small_and_its_queries_are_the_generators():
    ms, z = _ms(), _fixture()
    assert os.path.getsize(os.path.join(G, "k10_kdtree_segment_queries.npz")) < 500_000
    k8 = np.load(os.path.join(G, "k8_kdtree_queries.npz"))
    for name, (pts, Q, no, r2) in ms.k8_clouds().items():
        assert np.array_equal(k8[name + "_pts"], pts) and float(k8[name + "_r2"][0]) == r2, name
        q = ms.k10_queries(pts, Q)
        assert q["n"] == len(Q) and len(q["P"]) == len(Q) + ms.N_DEGENERATE
        for key in ("P", "P0", "DIR", "LO", "HI"):
            assert np.array_equal(z["%s_%s" % (name, key)], q[key], equal_nan=True), (name, key)
        n = q["n"]
        assert np.array_equal(q["P"][:n], Q) and not (q["P"][:n] == q["P0"][:n]).all(1).any()
        assert not (q["LO"][:n] > q["HI"][:n]).any()
        # the degenerate rows: p == p0 / zero dir / point box, a non-unit dir, NaN in either vector, far outside
        assert np.array_equal(q["P"][n], q["P0"][n]) and not q["DIR"][n].any() and np.array_equal(q["LO"][n], q["HI"][n])
        assert abs(np.linalg.norm(q["DIR"][n + 1]) - 2.5) < 1e-12
        assert np.isnan(q["P"][n + 2]).any() and np.isnan(q["LO"][n + 2]).any()
        assert np.isnan(q["P0"][n + 3]).any() and np.isnan(q["DIR"][n + 3]).any() and np.isnan(q["HI"][n + 3]).any()
        assert (q["P"][n + 4] > pts.max(0) + 999).all()


def test_fixture_equals_the_reference_library(orc):
    if not orc.have_ref():
        pytest.skip("oracle/_ref not built (no reference checkout)")
    ms, z = _ms(), _fixture()
    got = ms.compute()
    assert sorted(got) == sorted(z.files)
    for key in z.files:
        assert got[key].dtype == z[key].dtype and np.array_equal(got[key], z[key], equal_nan=True), key


def test_fixture_lists_satisfy_the_leaf_predicates():
    """every listed point passes the walk's leaf test (numpy, the reference's operation order), no index twice; the lists
    are not empty, and they are the reference's own sets, not the geometric ones"""
    ms, z = _ms(), _fixture()
    aabb_short, seg_short, between_differs = set(), {}, set()
    for name, (pts, Q, no, r2) in ms.k8_clouds().items():
        q = ms.k10_queries(pts, Q)
        n = q["n"]
        for b in ms.BUCKETS:
            got = {}
            for kind in ms.LIST_KINDS:
                off, idx = _lists(z, name, b, kind)
                A, B = ms.pair(kind, q)
                assert len(off) == len(A) + 1
                ms.check_lists(kind, pts, A, B, r2, off, idx)
                assert int(off[n]) > 0, (name, b, kind)
                got[kind] = _rows(off, idx)
            for i in range(n):
                full = {k: set(np.nonzero(ms.leaf_take(k, pts, ms.pair(k, q)[0][i], ms.pair(k, q)[1][i], r2))[0].tolist())
                        for k in ("aabb", "segall")}
                if set(got["aabb"][i]) != full["aabb"]:
                    aabb_short.add(name)
                if set(got["segall"][i]) != full["segall"]:
                    seg_short[(name, i)] = seg_short.get((name, i), 0) + 1
            # DIR is Normalize3(p0 - p) term for term: where the two lists differ, Between2Points' root tests fired
            if got["along"][:n] != got["between"][:n]:
                between_differs.add((name, b))
            # the degenerate rows, as observed on the reference: p == p0 gives nothing for Between2Points and
            # segmentSearch_all, a NaN anywhere and a far segment give nothing at all
            assert got["between"][n] == [] and got["segall"][n] == []
            for kind in ms.LIST_KINDS:
                assert got[kind][n + 2] == got[kind][n + 3] == got[kind][n + 4] == [], (name, b, kind)
            # the non-unit dir widens the cylinder (a cloud of one or seven points has nothing more to take)
            unit = set(np.nonzero(ms.leaf_take("along", pts, q["P"][n + 1], q["DIR"][n + 1] / 2.5, r2))[0].tolist())
            assert set(got["along"][n + 1]) >= unit and (len(got["along"][n + 1]) > len(unit) or len(pts) < 100)
    assert {("lattice", 1), ("lattice", 5), ("seven", 1), ("seven", 5)} <= between_differs
    assert {"uniform", "duplicates", "lattice", "clusters"} <= aabb_short
    assert {k[0] for k in seg_short} <= {"lattice"} and len({k[1] for k in seg_short}) <= 1


def test_fixture_nearest_point_is_the_closest_of_the_segment_list():
    ms, z = _ms(), _fixture()
    for name, (pts, Q, no, r2) in ms.k8_clouds().items():
        q = ms.k10_queries(pts, Q)
        n = q["n"]
        for b in ms.BUCKETS:
            near = z["%s_b%d_near" % (name, b)].astype(np.int32)
            assert near.shape == (n + ms.N_DEGENERATE,) and (near >= -1).all() and (near < len(pts)).all()
            rows = _rows(*_lists(z, name, b, "segall"))
            for i in range(n):
                if not rows[i]:
                    assert near[i] == -1, (name, b, i)
                    continue
                d = ms.dist2(pts, np.broadcast_to(q["P"][i], (len(rows[i]), 3)), np.array(rows[i]))
                assert near[i] in rows[i] and ms.dist2(pts, q["P"][i], near[i]) == d.min(), (name, b, i)
            # p == p0: segment_n is 0/0, the projection NaN, and "NaN >= maxdist2 -> continue" skips nothing: the nearest
            # point within the initial closest_d2 = sqr(sqrt(maxdist2)) of p
            with np.errstate(invalid="ignore"):
                d = ms.dist2(pts, np.broadcast_to(q["P"][n], pts.shape), np.arange(len(pts)))
            lim = np.sqrt(r2) * np.sqrt(r2)
            assert (near[n] == -1 and not (d < lim).any()) or d[near[n]] == d.min() < lim, (name, b)
            assert (near[n + 2:] == -1).all(), (name, b)


def test_entry_points_are_declared_everywhere():
    hdr = open(os.path.join(ROOT, "include", "tdtk_hip.h")).read()
    capi = importlib.import_module("3dtk_amd._capi")
    slam = importlib.import_module("3dtk_amd.slam6d")
    for name in EXPORTS:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in capi.EXPORTS, name
    for ref in ("kdIndexed.cc:195-213", "kdIndexed.cc:164-192", "kdIndexed.cc:233-250", "kdIndexed.cc:252-278",
                "kdIndexed.cc:280-301"):
        assert ref in hdr, ref
    for m in METHODS:
        assert callable(getattr(slam.KDtree, m)) and callable(getattr(slam.KDtree, m + "Batch")), m
    so = os.path.join(ROOT, "3dtk_amd", "lib3dtk_hip.so")
    if os.path.exists(so):
        import subprocess
        syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True).stdout
        for name in EXPORTS:
            assert re.search(r" T %s\b" % name, syms), name


def test_new_query_kernels_spill_nothing():
    path = os.path.join(ROOT, "3dtk_amd", "csrc", "query.resource.txt")
    if not os.path.exists(path):
        pytest.skip("no build in this tree (query.resource.txt is written by the Makefile)")
    blocks = open(path).read().split("remark: Function Name: ")[1:]
    found = {}
    for b in blocks:
        name = b.split()[0]
        if "k_shape_count" in name or "k_shape_fill" in name or "k_segment_nearest" in name:
            for key in ("VGPRs Spill", "SGPRs Spill"):
                m = re.search(key + r": (\d+)", b)
                assert m and int(m.group(1)) == 0, (name, key)
            found[name] = int(re.search(r"VGPRs: (\d+)", b).group(1))
    # a count and a fill kernel per list query, and the nearest-point kernel
    assert sum("k_shape_count" in n for n in found) == 4 and sum("k_shape_fill" in n for n in found) == 4, sorted(found)
    assert sum("k_segment_nearest" in n for n in found) == 1
    assert max(found.values()) <= 128, found          # at least four waves per SIMD's worth of registers
