"""Collision detection along a trajectory (tdtk_collision_mark / _depth_closest / _depth_axis): the CPU tier.  The fixture
k13_collision.npz against the reference's compiled queries, against the walks' leaf predicates and against brute force; the
per-lane device code of the collision kernels compiled for the host against the fixture; the exports, read_trajectory and
the resource remarks of the k_collide kernels."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import host_lane

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(G, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def mg():
    return _load("make_golden_collision")


@pytest.fixture(scope="module")
def fx(mg):
    return mg.load()


def _small_keys(mg):
    for name in mg.SMALL:
        for b in mg.BUCKETS:
            for cm in mg.METHODS:
                yield name, b, cm, "%s_b%d_m%d" % (name, b, cm)


def test_fixture_equals_the_reference(mg):
    """every array from a fresh run of the four loops over the reference's library (the 560,000 queries of `trips`, three
    times over, are most of this test's half minute)"""
    if not mg.have_ref():
        pytest.skip("no reference library (oracle/_ref/libref3dtk.so)")
    z = np.load(mg.OUT)
    got, stats = mg.compute()
    mg.check_not_vacuous(stats)
    assert sorted(got) == sorted(z.files)
    for key in z.files:
        assert got[key].dtype == z[key].dtype and np.array_equal(got[key], z[key]), key


def test_shapes_are_the_generators(mg, fx):
    n = 0
    for name, b, cm, key in _small_keys(mg):
        pts, model, frames, radius = mg.small_case(name)
        assert model.shape == (40, 3) and frames.shape == (12, 16)
        assert (model[0] == 0).all() and (model[1:6, 1] == 0).all() and (model[6:9, [0, 2]] == 0).all()
        assert np.array_equal(frames[4], frames[5])                      # a segment of length zero
        assert (frames[11, 12:15] > pts.max(0) + 100).all()              # a frame far outside
        assert radius * radius == pytest.approx(mg.k8_clouds()[name][3], rel=1e-15)
        mask = fx.mask(key, len(pts))
        assert mask.sum() == fx.num(key)
        assert (key + "_d1" in fx.z.files) == (name not in mg.NO_DEPTH)
        if name not in mg.NO_DEPTH:
            assert fx.z[key + "_d1"].dtype == np.float32 and fx.z[key + "_d2"].dtype == np.float32
            assert len(fx.z[key + "_d1"]) == fx.num(key) == len(fx.z[key + "_d2"])
        n += 1
    assert n == 6 * 3 * 2
    pts, model, frames, radius = mg.large_case("trips")
    assert len(pts) == 200_000 and len(model) * len(frames) == 560_000 and radius == 1.0
    assert os.path.getsize(mg.OUT) < 500_000


def test_every_case_marks_something_and_not_everything(mg, fx):
    sizes = {"trips": 200_000, "deep": 300_000, "table": 73_000, "nonfinite": 20_000}
    for name, b, cm, key in _small_keys(mg):
        n = len(mg.k8_clouds()[name][0])
        # (the cloud `one` has one point: "something" is "everything" there)
        assert 1 <= fx.num(key) and (fx.num(key) < n or n == 1), key
    for name, b in mg.LARGE:
        for cm in mg.METHODS:
            key = "%s_b%d_m%d" % (name, b, cm)
            assert 1 <= fx.num(key) < sizes[name], key
            assert fx.mask(key, sizes[name]).sum() == fx.num(key)


def _queries(mg, model, frames, cm):
    """(A, B) [Q][3]: the sphere centres (B is None) or the segments of a marking method"""
    W = np.array(mg.moved(model, frames))
    if cm == 1:
        return W.reshape(-1, 3), None
    return W[:-1].reshape(-1, 3), W[1:].reshape(-1, 3)


def _some_query_takes(mg, X, A, B, r2):
    """per row of X: does the leaf predicate of the method's walk take it for at least one query"""
    out = np.zeros(len(X), bool)
    for s in range(0, len(A), 4096):
        a = A[None, s:s + 4096]
        if B is None:
            with np.errstate(invalid="ignore", over="ignore"):
                out |= (mg._dist2(a, X[:, None, :]) < r2).any(1)
        else:
            out |= mg.leaf_take("segall", X[:, None, :], a, B[None, s:s + 4096], r2).any(1)
    return out


def test_every_marked_point_passes_the_leaf_predicate(mg, fx):
    """the walks list only what their leaf test takes: Dist2 < r2 of a sphere centre, comp_d2 < r2 of a segment.  (The
    converse does not hold for the segment walk: its lists are sometimes shorter than the geometric set.)  Method 1's
    sphere walk misses nothing on these clouds, so its mask IS the geometric set"""
    cases = [(n, b, cm, key, mg.small_case(n)) for n, b, cm, key in _small_keys(mg)]
    cases += [(n, b, cm, "%s_b%d_m%d" % (n, b, cm), mg.large_case(n)) for n, b in (("deep", 20), ("nonfinite", 20))
              for cm in mg.METHODS]
    for name, b, cm, key, (pts, model, frames, radius) in cases:
        A, B = _queries(mg, model, frames, cm)
        mask = fx.mask(key, len(pts))
        assert _some_query_takes(mg, pts[mask], A, B, radius * radius).all(), key
        if cm == 1 and name in mg.SMALL:
            assert not _some_query_takes(mg, pts[~mask], A, B, radius * radius).any(), key


def test_rows_with_non_finite_entries_mark_nothing(mg, fx):
    """the marked set of the non-finite case needs no query that a NaN or an infinity went into: every marked point is taken
    by a query of the finite rows alone"""
    pts, model, frames, radius = mg.large_case("nonfinite")
    good_p = np.setdiff1d(np.arange(len(model)), mg.NONFINITE_POINTS)
    assert np.isfinite(model[good_p]).all() and not np.isfinite(model[list(mg.NONFINITE_POINTS)]).all(1).any()
    W = np.array(mg.moved(model, frames))
    for cm in mg.METHODS:
        mask = fx.mask("nonfinite_b20_m%d" % cm, len(pts))
        if cm == 1:
            A, B = W.reshape(-1, 3), None
            fin = np.isfinite(A).all(1)
            A = A[fin]
        else:
            A, B = W[:-1].reshape(-1, 3), W[1:].reshape(-1, 3)
            fin = np.isfinite(A).all(1) & np.isfinite(B).all(1)
            A, B = A[fin], B[fin]
        assert 0 < (~fin).sum() < len(fin)
        assert _some_query_takes(mg, pts[mask], A, B, radius * radius).all()


def test_depths_of_the_fixture(mg, fx):
    """the axis depth is sqrtf of a float <= 1000; the closest depth is the brute-force distance to the nearest
    non-colliding point, (float)sqrt(Dist2)"""
    top = np.sqrt(np.float32(1000.0))
    n = 0
    for name, b, cm, key in _small_keys(mg):
        if name in mg.NO_DEPTH:
            continue
        pts = mg.k8_clouds()[name][0]
        mask = fx.mask(key, len(pts))
        d1, d2 = fx.z[key + "_d1"], fx.z[key + "_d2"]
        assert ((d2 >= 0) & (d2 <= top)).all(), key
        assert (d2 < top).any(), key                    # some query reached some point
        hit, rest = pts[mask], pts[~mask]
        brute = np.sqrt(mg._dist2(hit[:, None, :], rest[None, :, :]).min(1)).astype(np.float32)
        assert np.array_equal(d1, brute), key
        n += 1
    assert n == 4 * 3 * 2


def test_header_exports_and_mirror_name_the_new_entry_points(tdtk):
    from importlib import import_module
    capi = import_module("3dtk_amd._capi")
    hdr = open(os.path.join(ROOT, "include", "tdtk_hip.h")).read()
    so = os.path.join(ROOT, "3dtk_amd", "lib3dtk_hip.so")
    nm = subprocess.run(["nm", "-D", so], capture_output=True, text=True).stdout if os.path.exists(so) else None
    for sym in ("tdtk_collision_mark", "tdtk_collision_depth_closest", "tdtk_collision_depth_axis"):
        assert sym in capi.EXPORTS
        assert re.search(r"\bint %s\(" % sym, hdr), sym
        if nm is not None:
            assert re.search(r" T %s$" % sym, nm, re.M), sym
    for f in ("read_trajectory", "handle_pointcloud", "calculate_collidingdist", "calculate_collidingdist2"):
        assert hasattr(tdtk, f)


def test_read_trajectory_permutes_as_the_reference(tdtk, tmp_path):
    """collision_model.cc:202-217: transformation[i] = sign[i] * tmp[src[i]]"""
    rows = np.arange(32, dtype=np.float64).reshape(2, 16) + 0.5
    p = tmp_path / "trajectory.txt"
    p.write_text("\n".join(" ".join(repr(float(v)) for v in r) for r in rows) + "\n")
    got = tdtk.read_trajectory(str(p))
    assert got.shape == (2, 16) and got.dtype == np.float64
    for t, g in zip(rows, got):
        want = [t[5], -t[9], -t[1], -t[13], -t[6], t[10], t[2], -t[14], -t[4], t[8], t[0], t[12], -t[7], t[11], t[3], t[15]]
        assert np.array_equal(g, np.array(want))


def test_cmethod_3_marks_everything(tdtk):
    mask, num = tdtk.handle_pointcloud(np.zeros((4, 3)), np.zeros((9, 3)), np.zeros((2, 16)), 1.0, 3)
    assert mask.dtype == bool and mask.all() and len(mask) == 9 and num == 9


def test_collision_kernels_spill_nothing():
    """no spills; and no scratch beyond what every walking kernel of query.hip has: the call frame of the out-of-line overflow
    path of the lane stack (lane_stack.h), the figure of k_range_count.  The kernels without a walk use none"""
    path = os.path.join(ROOT, "3dtk_amd", "csrc", "query.resource.txt")
    if not os.path.exists(path):
        pytest.skip("no build in this tree (query.resource.txt is written by the Makefile)")
    all_blocks = open(path).read().split("remark: Function Name: ")[1:]

    def scratch(b):
        return int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))

    frame = [scratch(b) for b in all_blocks if "k_range_count" in b.split()[0]]
    assert len(frame) == 1
    blocks = [b for b in all_blocks if "k_collide" in b.split()[0]]
    names = [b.split()[0] for b in blocks]
    assert sum("k_collide_mark" in n for n in names) == 2 and len(names) == 6, names
    for want in ("k_collide_depth_axis", "k_collide_count", "k_collide_depth_init", "k_collide_depth_finish"):
        assert sum(want in n for n in names) == 1, names
    for b in blocks:
        name = b.split()[0]
        for key in ("VGPRs Spill", "SGPRs Spill"):
            m = re.search(key + r": (\d+)", b)
            assert m and int(m.group(1)) == 0, (name, key)
        walks = "k_collide_mark" in name or "k_collide_depth_axis" in name
        assert scratch(b) == (frame[0] if walks else 0), name


# ---- the per-lane device code on the host ----------------------------------------------------------------------------
# the walks, the emitters and the three per-lane bodies of the collision kernels as they stand in query_lane.h
# (host_lane_shim.h: __device__ defined away, a std::vector for the lane stack, a plain minimum for the atomic), with
# kd_build.cpp's host tree under them.  The model is taken in the caller's order: the results do not depend on it
_HOST_LANE = r"""
static QueryArgs args_of(HostTree& T, const std::vector<double>* soa, size_t P, const double* frames, double radius) {
  QueryArgs a = host_args(T);
  a.x = soa[0].data(); a.y = soa[1].data(); a.z = soa[2].data(); a.P = P; a.frames = frames; a.r2 = radius * radius;
  return a;
}
static void split(const double* model, size_t P, std::vector<double>* soa) {
  for (int c = 0; c < 3; c++) { soa[c].resize(P); for (size_t i = 0; i < P; i++) soa[c][i] = model[3 * i + c]; }
}
extern "C" void hl_mark(void* p, const double* model, size_t P, const double* frames, size_t F, double radius, int cmethod,
                        uint8_t* mask) {
  HostTree& T = *(HostTree*)p;
  std::vector<double> soa[3]; split(model, P, soa);
  QueryArgs a = args_of(T, soa, P, frames, radius);
  a.mask = mask; a.n = (cmethod == 1 ? F : F - 1) * P;
  HostStack st;
  for (size_t i = 0; i < a.n; i++) {
    if (cmethod == 1) collide_sphere_item(a, i, st);
    else collide_segment_item(a, i, st);
  }
}
extern "C" void hl_depth_axis(void* p, size_t nc, const double* model, size_t P, const double* frames, size_t F, double radius,
                              float* dist) {
  HostTree& T = *(HostTree*)p;
  std::vector<double> soa[3]; split(model, P, soa);
  QueryArgs a = args_of(T, soa, P, frames, radius);
  std::vector<unsigned long long> dmin(nc, (unsigned long long)__double_as_longlong(1000.0));
  a.dmin = dmin.data(); a.n = F * P;
  HostStack st;
  for (size_t i = 0; i < a.n; i++) collide_depth_axis_item(a, i, st);
  for (size_t i = 0; i < nc; i++) dist[i] = collide_depth_value(dmin[i]);
}
"""


def test_device_lane_code_compiled_for_the_host_equals_the_fixture(mg, fx, tmp_path):
    """masks of both methods and the axis depth on every small case.  (The closest depth adds no per-lane code: it is the
    FindClosest batch search and (float)sqrt, which test_depths_of_the_fixture restates by brute force.)"""
    L = host_lane.build(_HOST_LANE, tmp_path, "hl")
    L.hl_mark.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_double, C.c_int, C.c_void_p]
    L.hl_depth_axis.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_double, C.c_void_p]
    n = 0
    for name in mg.SMALL:
        pts, model, frames, radius = mg.small_case(name)
        pts, model, frames = (np.ascontiguousarray(a) for a in (pts, model, frames))
        for b in mg.BUCKETS:
            h = L.host_tree_create(pts.ctypes.data, len(pts), b)
            assert h
            for cm in mg.METHODS:
                key = "%s_b%d_m%d" % (name, b, cm)
                mask = np.zeros(len(pts), np.uint8)
                L.hl_mark(h, model.ctypes.data, len(model), frames.ctypes.data, len(frames), radius, cm, mask.ctypes.data)
                assert np.array_equal(mask.astype(bool), fx.mask(key, len(pts))), key
                if name not in mg.NO_DEPTH:
                    hit = np.ascontiguousarray(pts[mask.astype(bool)])
                    hh = L.host_tree_create(hit.ctypes.data, len(hit), b)
                    assert hh
                    d2 = np.empty(len(hit), np.float32)
                    L.hl_depth_axis(hh, len(hit), model.ctypes.data, len(model), frames.ctypes.data, len(frames), radius,
                                    d2.ctypes.data)
                    L.host_tree_destroy(hh)
                    assert np.array_equal(d2, fx.z[key + "_d2"]), key
                n += 1
            L.host_tree_destroy(h)
    assert n == 6 * 3 * 2
