"""k-NN and fixed-radius search on the kd-tree (tdtk_knn_search / tdtk_fixed_range_search and the normals built on them):
the CPU tier.  The fixture k8_kdtree_queries.npz against the reference library and against brute force, the adapter
functions against slam6d/point.h, and the resource remarks of query.hip."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def _mg():
    spec = importlib.util.spec_from_file_location("make_golden_knn", os.path.join(G, "make_golden_knn.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    return mg


def _fixture():
    return np.load(os.path.join(G, "k8_kdtree_queries.npz"))


def test_fixture_clouds_are_the_generators():
    mg, z = _mg(), _fixture()
    for name, (pts, Q, no, r2) in mg.k8_clouds().items():
        assert np.array_equal(z[name + "_pts"], pts) and np.array_equal(z[name + "_q"], Q), name
        assert int(z[name + "_own"][0]) == no and float(z[name + "_r2"][0]) == r2


def test_fixture_equals_the_reference_library(orc):
    if not orc.have_ref():
        pytest.skip("oracle/_ref not built (no reference checkout)")
    mg, z = _mg(), _fixture()
    got = mg.compute(orc)
    assert sorted(got) == sorted(z.files)
    for key in z.files:
        assert np.array_equal(got[key], z[key]), key


def test_fixture_agrees_with_brute_force():
    """k-NN: the sorted distance multiset of each list is the k smallest of all distances (ties may pick other points,
    the distances cannot differ); range: the set of points with Dist2 < r2."""
    mg, z = _mg(), _fixture()
    for name in mg.k8_clouds():
        pts, Q, r2 = z[name + "_pts"], z[name + "_q"], float(z[name + "_r2"][0])
        for b in mg.BUCKETS:
            for k in mg.KS:
                knn = z["%s_b%d_knn%d" % (name, b, k)]
                for i, q in enumerate(Q):
                    all_d = mg.dist2(pts, np.broadcast_to(q, pts.shape), np.arange(len(pts)))
                    m = min(k, len(pts))
                    assert (knn[i, m:] == -1).all() and (knn[i, :m] >= 0).all()
                    d = mg.dist2(pts, np.broadcast_to(q, (m, 3)), knn[i, :m])
                    assert np.array_equal(d, np.sort(d)), (name, b, k, i)
                    assert np.array_equal(d, np.sort(all_d)[:m]), (name, b, k, i)
            off, idx = z["%s_b%d_roff" % (name, b)], z["%s_b%d_ridx" % (name, b)]
            assert off[0] == 0 and off[-1] == len(idx)
            for i, q in enumerate(Q):
                all_d = mg.dist2(pts, np.broadcast_to(q, pts.shape), np.arange(len(pts)))
                l = idx[int(off[i]):int(off[i + 1])]
                assert len(set(l.tolist())) == len(l)
                assert set(l.tolist()) == set(np.nonzero(all_d < r2)[0].tolist()), (name, b, i)


def test_fixture_normals_are_unit_and_oriented():
    mg, z = _mg(), _fixture()
    for name in mg.k8_clouds():
        Q, no = z[name + "_q"], int(z[name + "_own"][0])
        for b in mg.BUCKETS:
            for key in ["nknn%d" % k for k in mg.NORMAL_KS] + ["nrange"]:
                n = z["%s_b%d_%s" % (name, b, key)]
                assert n.shape == (no, 3)
                fin = np.isfinite(n).all(1)
                assert np.allclose(np.linalg.norm(n[fin], axis=1), 1.0)


def test_normals_adapter_compiles_against_point_h(tmp_path):
    """adapters/normals_hip.h: calculateNormalsKNN_hip / calculateNormalsRange_hip with the reference's signatures
    (normals.cc:442-446, 369-372), against slam6d/point.h alone"""
    ref = os.environ.get("TDTK_REF", "/root/reference")
    if not os.path.exists(os.path.join(ref, "include", "slam6d", "point.h")):
        pytest.skip("no reference checkout (slam6d/point.h)")
    src = tmp_path / "nrm.cc"
    src.write_text('#include "normals_hip.h"\n'
                   "void use(std::vector<Point>& n, const std::vector<Point>& p, const double* r) {\n"
                   "  calculateNormalsKNN_hip(n, p, 20, r, 20);\n"
                   "  calculateNormalsRange_hip(n, p, 0.25, r);\n"
                   "}\n")
    obj = tmp_path / "nrm.o"
    r = subprocess.run(["g++", "-std=c++17", "-c", "-I" + os.path.join(ref, "include"), "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "adapters"), str(src), "-o", str(obj)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    syms = subprocess.run(["nm", "-C", str(obj)], capture_output=True, text=True).stdout
    assert "tdtk_normals_knn" in syms and "tdtk_normals_range" in syms


def test_query_kernels_spill_nothing():
    path = os.path.join(ROOT, "3dtk_amd", "csrc", "query.resource.txt")
    if not os.path.exists(path):
        pytest.skip("no build in this tree (query.resource.txt is written by the Makefile)")
    blocks = open(path).read().split("remark: Function Name: ")[1:]
    names = [b.split()[0] for b in blocks]
    for want in ("k_knn_reg", "k_knn_lds", "k_range_count", "k_range_fill", "k_range_normals"):
        assert any(want in n for n in names), want
    for b in blocks:
        name = b.split()[0]
        for key in ("VGPRs Spill", "SGPRs Spill"):
            m = re.search(key + r": (\d+)", b)
            assert m and int(m.group(1)) == 0, (name, key)
        assert not name.split("tdtk")[-1].lstrip("0123456789").startswith("k_search"), name


def test_header_and_exports_name_the_new_entry_points(tdtk):
    from importlib import import_module
    capi = import_module("3dtk_amd._capi")
    hdr = open(os.path.join(ROOT, "include", "tdtk_hip.h")).read()
    for sym in ("tdtk_knn_search", "tdtk_fixed_range_search", "tdtk_normals_knn", "tdtk_normals_range"):
        assert sym in capi.EXPORTS
        assert re.search(r"\bint %s\(" % sym, hdr), sym
    for fn in ("calculateNormalsKNN", "calculateNormalsRange"):
        assert hasattr(tdtk, fn)
    for m in ("kNearestNeighbors", "kNearestNeighborsBatch", "fixedRangeSearch", "fixedRangeSearchBatch"):
        assert hasattr(tdtk.KDtree, m)


# ---- the k9 fixture (tests/golden/make_golden_knn_edges.py): the cases of test_gpu_kdtree_query_edges.py ---------------
def _me():
    spec = importlib.util.spec_from_file_location("make_golden_knn_edges", os.path.join(G, "make_golden_knn_edges.py"))
    me = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(me)
    return me


def _k9():
    return np.load(os.path.join(G, "k9_kdtree_query_edges.npz"))


def test_k9_fixture_equals_the_reference_library(orc):
    if not orc.have_ref():
        pytest.skip("oracle/_ref not built (no reference checkout)")
    me, z = _me(), _k9()
    got = me.compute(orc)
    assert sorted(got) == sorted(z.files)
    for key in z.files:
        assert got[key].dtype == z[key].dtype and np.array_equal(got[key], z[key]), key


def test_k9_fixture_is_no_larger_than_k8():
    assert os.path.getsize(os.path.join(G, "k9_kdtree_query_edges.npz")) <= os.path.getsize(os.path.join(G, "k8_kdtree_queries.npz"))


def _brute_knn(me, pts, Q, knn, k, tag):
    m = min(k, len(pts))
    assert knn.shape == (len(Q), k) and (knn[:, m:] == -1).all() and (knn[:, :m] >= 0).all() and (knn < len(pts)).all(), tag
    for i, q in enumerate(Q):
        all_d = me.dist2(pts, np.broadcast_to(q, pts.shape), np.arange(len(pts)))
        assert len(set(knn[i, :m].tolist())) == m, (tag, i)
        d = all_d[knn[i, :m]]
        assert np.array_equal(d, np.sort(d)) and np.array_equal(d, np.sort(all_d)[:m]), (tag, i)


def _brute_range(me, pts, Q, off, idx, r2, tag):
    assert off[0] == 0 and off[-1] == len(idx) and len(off) == len(Q) + 1, tag
    for i, q in enumerate(Q):
        all_d = me.dist2(pts, np.broadcast_to(q, pts.shape), np.arange(len(pts)))
        l = idx[int(off[i]):int(off[i + 1])]
        assert len(set(l.tolist())) == len(l), (tag, i)
        assert set(l.tolist()) == set(np.nonzero(all_d < r2)[0].tolist()), (tag, i)


def test_k9_fixture_agrees_with_brute_force():
    """as test_fixture_agrees_with_brute_force: the k smallest distances as a sorted multiset, the set d2 < r2"""
    me, z = _me(), _k9()
    # deep: lengths only; never longer than the set d2 < r2, equal to it for the queries of the uniform part, and shorter
    # for own points far out in the geometric part (the reference's box test rounds by more than the radius there)
    pts, geo = me.deep_cloud()
    for b in me.DEEP_BUCKETS:
        _, qs = me.deep_range_queries(pts, geo, me.DEEP_FALLBACK_Q, b)
        for j, (q, r2) in enumerate(zip(qs, me.DEEP_R2)):
            cnt = z["deep_b%d_r%d_cnt" % (b, j)]
            brute = np.array([int((me.dist2(pts, np.broadcast_to(x, pts.shape), np.arange(len(pts))) < r2).sum()) for x in q])
            assert len(cnt) == len(q) and (cnt <= brute).all(), (b, j)
            inner = np.abs(q).max(1) <= 50
            assert inner.sum() >= len(q) // 2 and np.array_equal(cnt[inner], brute[inner]), (b, j)
    c0 = z["deep_b1_r0_cnt"][:me.DEEP_FALLBACK_Q // 3]
    assert (c0 == 0).sum() > 10 and (c0 == 1).sum() > 10        # own points of the geometric part: lost, or found alone
    # table: the leaf of copies as one run in every list that reaches it
    pts, copies, blob = me.table_cloud()
    qk, qrs = me.table_queries(pts, blob)
    for k in me.BAND_KS:
        _brute_knn(me, pts, qk, z["table_knn%d" % k], k, ("table", k))
    big = z["table_big"]
    assert len(big) == me.TABLE_COPIES and set(big.tolist()) == set(copies.tolist())
    n_big = 0
    for j, (q, r2) in enumerate(zip(qrs, me.TABLE_R2)):
        pos = z["table_r%d_pos" % j]
        off, idx = me.restore_run(z["table_r%d_soff" % j], z["table_r%d_sidx" % j], pos, big)
        assert np.array_equal(off, z["table_r%d_off" % j])
        assert not np.isin(z["table_r%d_sidx" % j], copies).any()        # a list holds the copies as that run or not at all
        _brute_range(me, pts, q, off, idx, r2, ("table", j))
        n_big += int((pos >= 0).sum())
    assert 16 <= n_big <= 48
    # short
    rows = me.short_rows(z["short_knn"])
    for M in me.SHORT_MS:
        pts, Q = me.short_cloud(M)
        assert len(pts) == M and len(Q) == 12
        for b in me.SHORT_BUCKETS:
            for k in me.SHORT_KS:
                _brute_knn(me, pts, Q, rows[(M, b, k)], k, ("short", M, b, k))
    # lattice: the stored queries
    pts, Q = me.lattice_cloud()
    Q = Q[:me.LATTICE_STORED]
    for k in me.BAND_KS:
        per_bucket = me.lattice_unpack_knn(Q, z["lattice_knn%d" % k])
        assert len(per_bucket) == len(me.LATTICE_BUCKETS)
        for b, knn in zip(me.LATTICE_BUCKETS, per_bucket):
            _brute_knn(me, pts, Q, knn, k, ("lattice", b, k))
    ties = 0
    for j, r2 in enumerate(me.LATTICE_R2):
        for b in me.LATTICE_BUCKETS:
            off = z["lattice_b%d_r%d_off" % (b, j)].astype(np.uint64)
            _brute_range(me, pts, Q, off, me.lattice_unpack_range(Q, off, z["lattice_b%d_r%d_idx" % (b, j)]), r2, ("lattice", b, r2))
        ties += sum(int((me.dist2(pts, np.broadcast_to(q, pts.shape), np.arange(len(pts))) == r2).sum()) for q in Q)
    assert ties > 1000                       # distances equal to r2 exist, and are left out
    # nonfinite: ordinary rows by brute force; what the reference returned for the others
    pts, Q, i_ord, i_nan, i_far = me.nonfinite_cloud()
    assert np.isnan(Q[i_nan]).any(1).all() and not np.isnan(Q[i_far]).any() and np.isfinite(Q[i_ord]).all()
    assert (np.abs(Q[i_far]).max(1) >= 1e160).all()
    for k in me.BAND_KS:
        knn = z["nonfinite_knn%d" % k]
        _brute_knn(me, pts, Q[i_ord], knn[i_ord], k, ("nonfinite", k))
        assert (knn[i_nan] == -1).all()
        assert (knn[i_far] >= 0).all() and all(len(set(r.tolist())) == k for r in knn[i_far])
    off, idx = z["nonfinite_roff"], z["nonfinite_ridx"]
    cnt = np.diff(off.astype(np.int64))
    assert (cnt[i_nan] == 0).all() and (cnt[i_far] == 0).all()
    sel = np.concatenate([np.arange(int(off[i]), int(off[i + 1])) for i in i_ord]).astype(np.int64)
    o2 = np.concatenate([[0], np.cumsum(cnt[i_ord])]).astype(np.uint64)
    assert len(sel) == len(idx)
    _brute_range(me, pts, Q[i_ord], o2, idx[sel], me.NONFINITE_R2, "nonfinite")
