"""k-NN / fixed-radius search and the KNN / range normals on the MI355X: warm end-to-end times (host clock around the
synchronising library call; host arrays in and out), next to calculateNormalsApxKNN on the same cloud and the reference
library's KDtreeIndexed on the host (an OpenMP loop of --ref-threads threads over a --ref-queries subset of the cloud,
scaled up to the whole cloud; labelled as such).  Prints one JSON line.

    python tools/query_bench.py [--sizes 1000000,10000000] [--reps 5] [--ref-queries 100000] [--ref-threads 16]

--segments adds one leg per cylinder / box / segment query at 1M points: 1M queries starting at the cloud's points, segments
a few point spacings long, maxdist2 (the box's half extent) chosen for about 20 entries per list, each next to the
reference's method in the same host loop; --only-segments runs nothing else.

--adaptive adds the adaptive-k normals at 1M points (queries = the points): the exact form at (9, 9) and (19, 19) next to
calculateNormalsKNN k = 10 and 20 in the same run (the same walks plus one evaluation of the rule), at (5, 20) and (10, 20)
with the histogram of k_used and the mean number of walks per point, the ANN form at (9, 9) next to calculateNormalsApxKNN
k = 10 and at (5, 20) (eps = 1.0), and the reference: the fixture generator's loop (tests/golden/make_golden_adaptive.py:
the reference library's searches and newmat's EigenValues, the glue in Python and therefore on one thread whatever
--ref-threads says) on a fiftieth of --ref-queries points, scaled to the whole cloud; --only-adaptive runs nothing else.

--hybrid adds k nearest within a radius at 1M points (queries = the points, k = 10 and 20, the fixed-radius leg's radius of
about 20.6 neighbours): the walk and the normals over its lists, next to the k-NN walk / normals at the same k and the
fixed-radius walk / normals at the same radius in the same run, and the mean list length; --only-hybrid runs nothing else.

--collision adds collision detection along a trajectory: a 1M-point environment (density 1 per unit volume), a model of
10,000 points in a box of 40 x 16 x 16, 300 frames along a curve through the cloud, radius 1 -- 3M (frame, point) items.
Marking with both methods on the resident tree, and both depth calls end to end (host compaction and the tree over the
sub-cloud included); next to them collision_model's loops over the reference library (tools/ref_query_loop.cc) on
--ref-threads threads, whole, where oracle/_ref exists; --only-collision runs nothing else.

--clusters adds radius clustering (tdtk_cluster_radius) on a 1M-point uniform cloud (density 1) at two radii: the
fixed-radius leg's (20.6 neighbours per point: one giant component) and one near the percolation threshold (3 neighbours per
point: many mid-sized components).  Per radius, in the same run: (1) the cluster call end to end and its link kernel alone,
(2) the count walk of tdtk_fixed_range_search on the same inputs -- the same walk without the unions -- (both kernels from
HIP events, tdtk_kernel_timing), (3) what a caller had to do without the entry point: tdtk_fixed_range_search end to end plus
a union-find over its lists on the host (numpy, the fixture generator's), (4) the reference library's fixedRangeSearch loop
over all points on ONE host thread, as segment_colliding's loop is serial (where oracle/_ref exists); --only-clusters runs
nothing else.

--only-peopleremover runs dynamic-object removal (tdtk_peopleremover) alone: a synthetic box room (600 units wide) scanned
from 8 positions, 250 000 points each, with a cube that stands somewhere else in every scan (3dtk_amd.synthetic_room), at
the reference's defaults (voxel 10, diff 0, cluster 5, subvoxel accuracy).  Warm, the minimum of --reps runs: the host call
end to end, and from HIP events the occupancy build, the walk, cluster + half-free + classification, and upload to
download; the voxel visits and visits per second of the walk; the walk again with every scan's points ordered by range
(what divergent ray lengths inside a wave cost).  The reference's time for the same input comes from
`python tests/golden/make_golden_peopleremover.py --time` on a machine that has the checkout (one host thread).

--only-hough runs the standard 3D Hough transform (3dtk_amd.Hough, tdtk_hough_*) alone, at the reference's default settings
(AccumulatorBallI, RhoNum 500, PhiNum 176, ThetaNum 360, RhoMax 1500, MaxPointPlaneDist 1.5) on one scan of 1M points of
3dtk_amd.synthetic_room's box room.  Warm, the minimum of --reps runs, from HIP events: the vote, the peak list, one
plane_points + fit_plane on the first peak; point-cell pairs per second of the vote and the fp64 rate they stand for (5 flops
per pair: three products, two additions; the window and the predicate come on top).  The reference's time for the same vote
comes from `python tests/golden/make_golden_hough.py --time` on a machine that has the checkout: accumulate(Point) over 100
points on one host thread, times N / 100 (the loop is serial and linear in N).

--only-forest runs the dynamic kd-forest (3dtk_amd.BkdTree, tdtk_forest_*) alone: a uniform map (density 1) grown from 0 to
1M points by scans of 100 000 at bucket 20.  Warm, the minimum of --reps runs, per scan: the insert call end to end and its
stages (the plan on the host clock, the gathers and the builds from HIP events), the slots it built and the occupied slots
behind it, next to tdtk_tree_create over all the points so far -- what a caller does today.  On the final forest: FindClosest
of the 1M points at maxdist2 = 625, k-NN at k = 10 and the 20.6-neighbour radius, each next to the same call on one tree over
the same points; then 10 000 removes (the second batch of two, so that the first warms the code).

--only-octree runs the octree search tree (3dtk_amd.BOctTree, tdtk_octree_*) alone: FindClosestBatch of 1M queries at maxdist2
= 625 on a 1M-point uniform cloud (density 1), on the octree (voxel 10, earlystop) and on the k-d tree (bucket 20) -- five runs
each, alternating between the two trees, min / max / median; both builds; whether the two answers agree.

--only-octree-icp runs icp6D::match on the octree search tree alone, per iteration (-a 1, maxdist2 625, epsilon 0, so every
run makes all its iterations: 50 on the pair, 10 on the cloud): the resident loop (icp6D.match on scans with setSearchTreeParameter(2): tdtk_icp_match_octree) next to the loop stepped
from the host (BOctTree.getPtPairs + Align_Parallel + Scan.transform per iteration), on the bundled scan pair and on the 1M-point
uniform cloud of --only-octree (voxel 10, earlystop) -- five runs each, alternating between the two loops, host clock, min / max
/ median; then one resident run with tdtk_kernel_timing on: the walk's and the pair sums' share from HIP events.

Kernel times: run the same command under `rocprofv3 --kernel-trace --stats` (k_knn_reg, k_range_count / k_range_fill,
k_range_normals, k_shape_count / k_shape_fill, k_segment_nearest, k_knn_adaptive_reg / k_knn_adaptive_lds, k_ann_adaptive, k_knnr_reg / k_knnr_lds,
k_collide_mark, k_collide_depth_axis)."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    fn()                                     # warm: code objects, workspaces
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"min_ms": round(min(ts), 3), "median_ms": round(float(np.median(ts)), 3)}


def ref_legs(pts, r2, tag, rng, nq, threads):
    """the reference library's KDtreeIndexed on the host: kNearestNeighbors (k = 10, 20) and fixedRangeSearch in an OpenMP
    loop of `threads` threads (tools/ref_query_loop.cc) over nq random cloud points, scaled to the whole cloud"""
    import ctypes as C
    import subprocess
    import tempfile
    spec = importlib.util.spec_from_file_location("make_golden_knn", os.path.join(ROOT, "tests", "golden", "make_golden_knn.py"))
    mg = importlib.util.module_from_spec(spec); spec.loader.exec_module(mg)
    d = tempfile.mkdtemp()
    so = os.path.join(d, "ref_query_loop.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fopenmp", "-fPIC", "-shared",
                           os.path.join(ROOT, "tools", "ref_query_loop.cc"), "-o", so])
    Lq = C.CDLL(so)
    Lq.ref_query_loop.restype = C.c_double
    Lq.ref_query_loop.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_size_t, C.c_int, C.c_int, C.c_double,
                                  C.c_int, C.POINTER(C.c_ulonglong)]
    t = mg.RefTree(pts, 20)
    q = np.ascontiguousarray(pts[rng.choice(len(pts), nq, replace=False)])
    qp = q.ctypes.data_as(C.POINTER(C.c_double))
    found = C.c_ulonglong(0)
    res = {}
    scale = len(pts) / nq
    label = "ref_host_%dthreads_%dkq_scaled" % (threads, nq // 1000)
    for k in (10, 20):
        fn = C.cast(t.knn_fn, C.c_void_p)
        Lq.ref_query_loop(fn, t.kdi, qp, min(nq, 2000), 0, k, 0.0, threads, C.byref(found))     # warm
        ms = Lq.ref_query_loop(fn, t.kdi, qp, nq, 0, k, 0.0, threads, C.byref(found))
        res["%s_knn_k%d_%s_ms" % (label, k, tag)] = round(ms * scale, 1)
    fn = C.cast(t.rng_fn, C.c_void_p)
    ms = Lq.ref_query_loop(fn, t.kdi, qp, nq, 1, 0, float(r2), threads, C.byref(found))
    res["%s_range_20nn_%s_ms" % (label, tag)] = round(ms * scale, 1)
    return res


def _ref_loop_lib():
    import ctypes as C
    import subprocess
    import tempfile
    so = os.path.join(tempfile.mkdtemp(), "ref_query_loop.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fopenmp", "-fPIC", "-shared",
                           os.path.join(ROOT, "tools", "ref_query_loop.cc"), "-o", so])
    return C.CDLL(so)


def segment_legs(tdtk, pts, tag, rng, reps, nq, threads):
    """fixedRangeSearchAlongDir / Between2Points, AABBSearch, segmentSearch_all / _1NearestPoint: the queries start at the
    cloud's points (density 1 per unit volume), p0 = p + N(0, 1.5) per axis -- segments about 2.4 spacings long.  About 20
    entries per list: the cylinders run through the whole cloud (pi r^2 x 100 = 20), the segment's capsule has
    pi r^2 x 2.4 + 4/3 pi r^3 = 20 at r^2 = 1.5, the box is the cube of volume 20 around p."""
    import ctypes as C
    out = {}
    M = len(pts)
    ext = 100.0 * (M / 1e6) ** (1 / 3)
    P = pts
    P0 = pts + rng.normal(0.0, 1.5, pts.shape)
    d = P0 - P
    DIR = d / np.sqrt((d * d).sum(1))[:, None]
    h = 20.0 ** (1 / 3) / 2
    LO, HI = P - h, P + h
    md2 = {"along_dir": 20.0 / (np.pi * ext), "between": 20.0 / (np.pi * ext), "segment_all": 1.5, "segment_nearest": 1.5}
    kd = tdtk.KDtree(pts, 20)
    legs = {
        "along_dir": (lambda: kd.fixedRangeSearchAlongDirBatch(P, DIR, md2["along_dir"]), P, DIR),
        "between": (lambda: kd.fixedRangeSearchBetween2PointsBatch(P, P0, md2["between"]), P, P0),
        "aabb": (lambda: kd.AABBSearchBatch(LO, HI), LO, HI),
        "segment_all": (lambda: kd.segmentSearch_allBatch(P, P0, md2["segment_all"]), P, P0),
        "segment_nearest": (lambda: kd.segmentSearch_1NearestPointBatch(P, P0, md2["segment_nearest"]), P, P0),
    }
    for name, (fn, _, _) in legs.items():
        out["%s_%s" % (name, tag)] = timed(fn, reps)
        r = fn()
        if name == "segment_nearest":
            out["%s_%s_found" % (name, tag)] = round(float((r[0] >= 0).mean()), 4)
        else:
            out["%s_%s_mean_list" % (name, tag)] = round(float(r[0][-1]) / M, 2)
    from oracle import orc
    if not orc.have_ref() or nq <= 0:
        return out
    spec = importlib.util.spec_from_file_location("make_golden_segments",
                                                  os.path.join(ROOT, "tests", "golden", "make_golden_segments.py"))
    ms = importlib.util.module_from_spec(spec); spec.loader.exec_module(ms)
    Lq = _ref_loop_lib()
    dp = C.POINTER(C.c_double)
    Lq.ref_pair_query_loop.restype = C.c_double
    Lq.ref_pair_query_loop.argtypes = [C.c_void_p, C.c_void_p, dp, dp, C.c_size_t, C.c_int, C.c_double, C.c_int,
                                       C.POINTER(C.c_ulonglong)]
    t = ms.SegRef(pts, 20)
    rows = rng.choice(M, nq, replace=False)
    found = C.c_ulonglong(0)
    label = "ref_host_%dthreads_%dkq_scaled" % (threads, nq // 1000)
    kinds = {"along_dir": ("along", 2), "between": ("between", 2), "aabb": ("aabb", 3), "segment_all": ("segall", 2),
             "segment_nearest": ("near", 4)}
    for name, (_, A, B) in legs.items():
        kind, mode = kinds[name]
        a = np.ascontiguousarray(A[rows]); b = np.ascontiguousarray(B[rows])
        fn = C.cast(t.fn[kind], C.c_void_p)
        args = (fn, t.kdi, a.ctypes.data_as(dp), b.ctypes.data_as(dp))
        Lq.ref_pair_query_loop(*args, min(nq, 2000), mode, float(md2.get(name, 0.0)), threads, C.byref(found))     # warm
        ms_ = Lq.ref_pair_query_loop(*args, nq, mode, float(md2.get(name, 0.0)), threads, C.byref(found))
        out["%s_%s_%s_ms" % (label, name, tag)] = round(ms_ * M / nq, 1)
    return out


def adaptive_legs(tdtk, pts, tag, rng, reps, nq, threads):
    """calculateNormalsAdaptiveKNN / calculateNormalsAdaptiveApxKNN, end to end like the other normals legs (tree build
    included), each next to the fixed-k estimator that walks the same lists"""
    out = {}
    rpos = [0.0, 0.0, 0.0]
    for k in (10, 20):
        out["normals_knn_k%d_%s" % (k, tag)] = timed(lambda: tdtk.calculateNormalsKNN(pts, k, rpos), reps)
        out["adaptive_knn_%d_%d_%s" % (k - 1, k - 1, tag)] = timed(lambda: tdtk.calculateNormalsAdaptiveKNN(pts, k - 1, k - 1, rpos), reps)
    for kmin, kmax in ((5, 20), (10, 20)):
        key = "adaptive_knn_%d_%d_%s" % (kmin, kmax, tag)
        out[key] = timed(lambda: tdtk.calculateNormalsAdaptiveKNN(pts, kmin, kmax, rpos), reps)
        _, ku = tdtk.calculateNormalsAdaptiveKNN(pts, kmin, kmax, rpos, want_k=True)
        out[key + "_k_used_hist"] = np.bincount(ku, minlength=kmax + 1)[kmin:].tolist()
        out[key + "_mean_walks"] = round(float((ku - kmin + 1).mean()), 3)
    out["normals_apxknn_k10_%s" % tag] = timed(lambda: tdtk.calculateNormalsApxKNN(pts, 10, rpos, 1.0), reps)
    out["adaptive_apxknn_9_9_%s" % tag] = timed(lambda: tdtk.calculateNormalsAdaptiveApxKNN(pts, 9, 9, rpos, 1.0), reps)
    key = "adaptive_apxknn_5_20_%s" % tag
    out[key] = timed(lambda: tdtk.calculateNormalsAdaptiveApxKNN(pts, 5, 20, rpos, 1.0), reps)
    _, ku = tdtk.calculateNormalsAdaptiveApxKNN(pts, 5, 20, rpos, 1.0, want_k=True)
    out[key + "_k_used_hist"] = np.bincount(ku, minlength=21)[5:].tolist()
    out[key + "_mean_walks"] = round(float((ku - 5 + 1).mean()), 3)
    from oracle import orc
    if not orc.have_ref() or nq <= 0:
        return out
    # the reference: the generator's loop (library searches and newmat from oracle/_ref, glue in Python).  One thread: the
    # loop calls kNearestNeighbors with threadNum 0 and newmat keeps global state, so it cannot run on several Python
    # threads, and the Python glue is most of its time anyway -- a yardstick for the order of magnitude, labelled as such
    spec = importlib.util.spec_from_file_location("make_golden_adaptive",
                                                  os.path.join(ROOT, "tests", "golden", "make_golden_adaptive.py"))
    ma = importlib.util.module_from_spec(spec); spec.loader.exec_module(ma)
    rows = rng.choice(len(pts), nq, replace=False)
    label = "ref_loop_python_glue_1thread_%dq_scaled" % nq
    t = ma.mgk.RefTree(pts, 20)
    ann = orc.AnnTree(pts, "ref")
    for name, lists in (("adaptive_knn_5_20", ma.exact_lists(t)), ("adaptive_apxknn_5_20", ma.ann_lists(ann, 1.0))):
        t0 = time.perf_counter()
        ma.reference_loop(orc, pts, rows, lists, 5, 20, rpos=np.zeros(3))
        out["%s_%s_%s_ms" % (label, name, tag)] = round((time.perf_counter() - t0) * 1e3 * len(pts) / nq, 1)
    return out


def hybrid_legs(tdtk, pts, tag, reps):
    """kNearestRangeSearch and calculateNormalsKNNRange, end to end like the other legs, each next to the k-NN and the
    fixed-radius form it combines (their kernels, same cloud, same run)"""
    out = {}
    rpos = [0.0, 0.0, 0.0]
    r2 = (20.0 * 3 / (4 * np.pi)) ** (2.0 / 3.0)                   # the fixed-radius leg's: ~20.6 neighbours per query
    kd = tdtk.KDtree(pts, 20)
    out["range_20nn_%s" % tag] = timed(lambda: kd.fixedRangeSearchBatch(pts, r2), reps)
    out["normals_range_%s" % tag] = timed(lambda: tdtk.calculateNormalsRange(pts, r2, rpos), reps)
    for k in (10, 20):
        out["knn_k%d_%s" % (k, tag)] = timed(lambda: kd.kNearestNeighborsBatch(pts, k), reps)
        out["knn_range_k%d_%s" % (k, tag)] = timed(lambda: kd.kNearestRangeSearchBatch(pts, k, r2), reps)
        out["knn_range_k%d_%s_mean_list" % (k, tag)] = round(float(kd.kNearestRangeSearchBatch(pts, k, r2)[2].mean()), 2)
        out["normals_knn_k%d_%s" % (k, tag)] = timed(lambda: tdtk.calculateNormalsKNN(pts, k, rpos), reps)
        out["normals_knn_range_k%d_%s" % (k, tag)] = timed(lambda: tdtk.calculateNormalsKNNRange(pts, k, r2, rpos), reps)
    return out


def collision_legs(tdtk, reps, threads):
    """handle_pointcloud (both methods), calculate_collidingdist and calculate_collidingdist2 on the device, and the same
    loops over the reference library"""
    import ctypes as C
    spec = importlib.util.spec_from_file_location("make_golden_collision",
                                                  os.path.join(ROOT, "tests", "golden", "make_golden_collision.py"))
    mg = importlib.util.module_from_spec(spec); spec.loader.exec_module(mg)
    rng = np.random.default_rng(2031)
    env = rng.uniform(-50, 50, (1_000_000, 3))
    model = rng.uniform(-1.0, 1.0, (10_000, 3)) * np.array([20.0, 8.0, 8.0])
    frames = mg.curve(300, (-35, -30, -32), (34, 31, 30), 8.0)
    radius = 1.0
    out = {"collision_items": len(model) * len(frames)}
    kd = tdtk.KDtree(env, 20)
    masks = {}
    for cm in (1, 2):
        out["collision_mark_m%d_1M" % cm] = timed(lambda: tdtk.handle_pointcloud(model, kd, frames, radius, cm), reps)
        masks[cm], out["collision_mark_m%d_1M_num" % cm] = tdtk.handle_pointcloud(model, kd, frames, radius, cm)
    mask = masks[1]
    out["collision_depth_closest_1M"] = timed(lambda: tdtk.calculate_collidingdist(env, mask), reps)
    out["collision_depth_axis_1M"] = timed(lambda: tdtk.calculate_collidingdist2(model, env, frames, mask, radius), reps)
    d1 = tdtk.calculate_collidingdist(env, mask)
    d2 = tdtk.calculate_collidingdist2(model, env, frames, mask, radius)
    from oracle import orc
    if not orc.have_ref():
        return out
    Lq = _ref_loop_lib()
    dp = C.c_void_p
    Lq.ref_collision_mark_loop.restype = C.c_double
    Lq.ref_collision_mark_loop.argtypes = [dp, dp, dp, dp, C.c_size_t, dp, C.c_size_t, C.c_double, C.c_int, C.c_int, dp]
    Lq.ref_collision_depth_axis_loop.restype = C.c_double
    Lq.ref_collision_depth_axis_loop.argtypes = [dp, dp, dp, dp, C.c_size_t, dp, C.c_size_t, dp, C.c_size_t, C.c_double,
                                                 C.c_int, dp]
    label = "ref_host_%dthreads" % threads
    t = mg.ColRef(env, 20)
    fn = {k: C.cast(f, C.c_void_p) for k, f in (("range", t.c_range), ("segall", t.c_segall), ("near", t.c_near))}
    model_c, frames_c = np.ascontiguousarray(model), np.ascontiguousarray(frames)
    for cm in (1, 2):
        m8 = np.zeros(len(env), np.uint8)
        ms = Lq.ref_collision_mark_loop(fn["range"], fn["segall"], t.kdi, model_c.ctypes.data, len(model), frames_c.ctypes.data,
                                        len(frames), radius * radius, cm, threads, m8.ctypes.data)
        out["%s_collision_mark_m%d_1M_ms" % (label, cm)] = round(ms, 1)
        out["collision_mark_m%d_1M_equal" % cm] = bool(np.array_equal(m8.astype(bool), masks[cm]))
    hit, rest = np.ascontiguousarray(env[mask]), np.ascontiguousarray(env[~mask])
    t0 = time.perf_counter()
    tr = mg.ColRef(rest, 20)
    idx = np.empty(len(hit), np.int32)
    tr.R.ref_kdi_find_closest(tr.h, hit.ctypes.data_as(C.POINTER(C.c_double)), len(hit), mg.MAXDIST2,
                              idx.ctypes.data_as(C.POINTER(C.c_int32)), threads)
    r1 = np.sqrt(mg._dist2(hit, rest[idx])).astype(np.float32)
    out["%s_collision_depth_closest_1M_ms" % label] = round((time.perf_counter() - t0) * 1e3, 1)
    out["collision_depth_closest_1M_equal"] = bool(np.array_equal(r1, d1))
    t0 = time.perf_counter()
    th = mg.ColRef(hit, 20)
    fh = {k: C.cast(f, C.c_void_p) for k, f in (("range", th.c_range), ("near", th.c_near))}
    r2 = np.empty(len(hit), np.float32)
    Lq.ref_collision_depth_axis_loop(fh["near"], fh["range"], th.kdi, th.pts.ctypes.data, len(hit), model_c.ctypes.data,
                                     len(model), frames_c.ctypes.data, len(frames), radius * radius, threads, r2.ctypes.data)
    out["%s_collision_depth_axis_1M_ms" % label] = round((time.perf_counter() - t0) * 1e3, 1)
    out["collision_depth_axis_1M_equal"] = bool(np.array_equal(r2, d2))
    return out


def cluster_legs(tdtk, reps):
    """tdtk_cluster_radius next to the count walk, to the lists + host union-find, and to the reference's serial loop"""
    import ctypes as C
    spec = importlib.util.spec_from_file_location("make_golden_clusters", os.path.join(ROOT, "tests", "golden", "make_golden_clusters.py"))
    mg = importlib.util.module_from_spec(spec); spec.loader.exec_module(mg)
    pts = np.random.default_rng(2033).uniform(-50, 50, (1_000_000, 3))
    kd = tdtk.KDtree(pts, 20)
    L = tdtk.lib()
    out = {}

    def kernel_ms(fn):
        """min over reps warm runs of the kernel the library's events bracket in fn (the link walk / the count walk)"""
        was = L.tdtk_kernel_timing(1)
        ms = C.c_double(0.0)
        ts = []
        try:
            for i in range(reps + 1):
                fn()
                L.tdtk_last_kernel_ms(C.byref(ms))
                if i:
                    ts.append(ms.value)
        finally:
            L.tdtk_kernel_timing(was)
        return round(min(ts), 3)

    legs = (("20nn", (20.0 * 3 / (4 * np.pi)) ** (2.0 / 3.0)), ("3nn", (3.0 * 3 / (4 * np.pi)) ** (2.0 / 3.0)))
    for tag, r2 in legs:
        out["clusters_%s_1M" % tag] = timed(lambda: kd.clusters(r2), reps)
        out["clusters_%s_1M_link_kernel_ms" % tag] = kernel_ms(lambda: kd.clusters(r2))
        labels, k, first, sizes = kd.clusters(r2, want_sizes=True)
        out["clusters_%s_1M_n" % tag] = k
        out["clusters_%s_1M_largest" % tag] = int(sizes.max())
        out["clusters_%s_1M_of_100_or_more" % tag] = int((sizes >= 100).sum())
        out["range_%s_1M" % tag] = timed(lambda: kd.fixedRangeSearchBatch(pts, r2), reps)
        out["range_%s_1M_count_kernel_ms" % tag] = kernel_ms(lambda: kd.fixedRangeSearchBatch(pts, r2))
        off, idx, _ = kd.fixedRangeSearchBatch(pts, r2)
        out["range_%s_1M_mean_list" % tag] = round(float(off[-1]) / len(pts), 2)
        ei = np.repeat(np.arange(len(pts)), np.diff(off.astype(np.int64)))

        def host_uf():
            return mg.canonical(mg.components(len(pts), ei, idx.astype(np.int64)))
        out["host_union_find_%s_1M" % tag] = timed(host_uf, reps)
        out["clusters_%s_1M_equal_host_union_find" % tag] = bool(np.array_equal(host_uf()[0], labels))
    from oracle import orc
    if not orc.have_ref():
        return out
    Lq = _ref_loop_lib()
    Lq.ref_query_loop.restype = C.c_double
    Lq.ref_query_loop.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_size_t, C.c_int, C.c_int, C.c_double,
                                  C.c_int, C.POINTER(C.c_ulonglong)]
    t = mg.ColRef(pts, 20)
    fn = C.cast(t.c_range, C.c_void_p)
    qp = t.pts.ctypes.data_as(C.POINTER(C.c_double))
    found = C.c_ulonglong(0)
    for tag, r2 in legs:
        Lq.ref_query_loop(fn, t.kdi, qp, 2000, 1, 0, float(r2), 1, C.byref(found))     # warm
        ms = Lq.ref_query_loop(fn, t.kdi, qp, len(pts), 1, 0, float(r2), 1, C.byref(found))
        out["ref_host_1thread_range_loop_%s_1M_ms" % tag] = round(ms, 1)
    return out


def peopleremover_legs(tdtk, reps):
    """tdtk_peopleremover on tests/golden/make_golden_peopleremover.py's BENCH workload"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_peopleremover",
                                                  os.path.join(ROOT, "tests", "golden", "make_golden_peopleremover.py"))
    mg = importlib.util.module_from_spec(spec); spec.loader.exec_module(mg)
    pr = importlib.import_module("3dtk_amd.peopleremover")
    scans, org = tdtk.synthetic_room(mg.BENCH["n_scans"], mg.BENCH["points_per_scan"], seed=mg.BENCH["seed"])
    out = {"peopleremover_scans": len(scans), "peopleremover_points": int(sum(len(s) for s in scans))}
    stages = []

    def run():
        masks, counts = tdtk.peopleremover(scans, org)
        stages.append(pr.last_timings())
        return masks, counts
    out["peopleremover_end_to_end"] = timed(run, reps)
    masks, counts = run()
    for k in ("build_ms", "walk_ms", "post_ms", "total_ms"):
        out["peopleremover_" + k] = round(min(s[k] for s in stages[1:]), 3)           # (the first run is the warm-up)
    out.update({"peopleremover_" + k: v for k, v in counts.items()})
    out["peopleremover_dynamic_points"] = int(sum(int(m.sum()) for m in masks))
    out["peopleremover_Mvisits_per_s"] = round(counts["visits"] / out["peopleremover_walk_ms"] / 1e3, 1)
    # the same rays with every scan's points ordered by range: the lanes of a wave then walk rays of nearly equal length, so
    # the difference to the walk above (random directions next to each other) is what divergence inside a wave costs
    by_range = [s[np.argsort(np.linalg.norm(s - o, axis=1), kind="stable")] for s, o in zip(scans, org)]
    stages.clear()
    for _ in range(reps + 1):
        _, c2 = tdtk.peopleremover(by_range, org)
        stages.append(pr.last_timings())
    assert c2 == counts
    out["peopleremover_walk_ms_rays_by_range"] = round(min(s["walk_ms"] for s in stages[1:]), 3)
    return out


def hough_legs(tdtk, reps):
    """the vote, the peaks and one plane's points and fit at the reference's defaults (see the module docstring)"""
    hough = importlib.import_module("3dtk_amd.hough")
    scans, _ = tdtk.synthetic_room(1, 1_000_000, seed=22)
    cfg = hough.ConfigFileHough()
    h = hough.Hough(scans[0], cfg)
    cells, n = len(h.normals), len(h.points)
    out = {"hough_points": n, "hough_cells": cells, "hough_rho_bins": int(cfg.RhoNum)}
    best = {}

    def keep(key):
        ms = hough.last_timings()[key]
        best[key] = min(best.get(key, ms), ms)
    t0 = time.perf_counter()
    cand = None
    for rep in range(reps + 1):                        # the first run is the warm-up
        if rep == 1:
            best.clear()
        h.votes()
        keep("vote_ms")
        h._resident = True                             # the steps behind the vote read the cloud and the counts in place
        try:
            peaks = h.peaks()
            keep("peaks_ms")
            plane = h.cell_plane(peaks[0])
            _, idx = h.plane_points(plane[:3], plane[3])
            keep("plane_points_ms")
            fit, planarity = h.fit_plane(idx)
            keep("fit_ms")
        finally:
            h._resident = False
        cand = dict(cell=peaks[0].tolist(), plane=plane.tolist(), inliers=int(len(idx)),
                    fit=None if fit is None else fit.tolist(), planarity=planarity)
    out["hough_loop_wall_s"] = round(time.perf_counter() - t0, 3)
    for k, v in best.items():
        out["hough_" + k] = round(v, 3)
    pairs = float(n) * cells
    out["hough_Gpairs_per_s"] = round(pairs / best["vote_ms"] / 1e6, 2)
    out["hough_vote_fp64_Tflops"] = round(5 * pairs / best["vote_ms"] / 1e9, 3)
    out["hough_peaks"] = int(len(peaks))
    out["hough_first_candidate"] = cand
    return out


def forest_legs(tdtk, reps):
    """the dynamic kd-forest against the full rebuild and the single tree (see the module docstring)"""
    n_scans, per = 10, 100_000
    pts = np.random.default_rng(2031).uniform(-50, 50, (n_scans * per, 3))
    r2 = (20.0 * 3 / (4 * np.pi)) ** (2.0 / 3.0)
    out = {"forest_bucket": 20, "forest_scan_points": per}
    rows = [dict() for _ in range(n_scans)]
    f = None
    for rep in range(reps + 1):                       # (the first run is the warm-up)
        if f is not None:
            f.close()
        f = tdtk.BkdTree(20)
        for i in range(n_scans):
            scan = pts[i * per:(i + 1) * per]
            t0 = time.perf_counter()
            f.insert(scan)
            ms = (time.perf_counter() - t0) * 1e3
            st = f.last_insert()
            if rep == 0:
                continue
            r = rows[i]
            r["insert_ms"] = min(r.get("insert_ms", 1e30), ms)
            for k in ("plan_ms", "gather_ms", "build_ms"):
                r[k] = min(r.get(k, 1e30), st[k])
            r["slots_built"], r["merges"] = st["slots_built"], st["merges"]
            r["occupied_slots"] = sum(1 for c in f.info()[0] if c)
            r["map_points"] = (i + 1) * per
    for i, r in enumerate(rows):
        r["rebuild_ms"] = timed(lambda: tdtk.KDtree(pts[:(i + 1) * per], 20), reps)["min_ms"]
        for k in ("insert_ms", "plan_ms", "gather_ms", "build_ms"):
            r[k] = round(r[k], 3)
    out["forest_inserts"] = rows
    occ = sum(1 for c in f.info()[0] if c)
    out["forest_final_occupied_slots"] = occ
    out["forest_final_counts"] = f.info()[0]
    kd = tdtk.KDtree(pts, 20)
    out["forest_find_closest_1M"] = timed(lambda: f.FindClosest(pts, 625.0), reps)
    out["tree_find_closest_1M"] = timed(lambda: kd.FindClosestBatch(pts, 625.0), reps)
    out["forest_knn_k10_1M"] = timed(lambda: f.kNearestNeighbors(pts, 10), reps)
    out["tree_knn_k10_1M"] = timed(lambda: kd.kNearestNeighborsBatch(pts, 10), reps)
    out["forest_range_20nn_1M"] = timed(lambda: f.fixedRangeSearch(pts, r2), reps)
    out["tree_range_20nn_1M"] = timed(lambda: kd.fixedRangeSearchBatch(pts, r2), reps)
    # the answers are the single tree's (a uniform cloud: no ties)
    fi, fd = f.FindClosest(pts[:20000], 625.0)
    ti, td = kd.FindClosestBatch(pts[:20000], 625.0)
    assert np.array_equal(fi, ti) and np.array_equal(fd, td)
    fi, fd = f.kNearestNeighbors(pts[:20000], 10)
    ti, td = kd.kNearestNeighborsBatch(pts[:20000], 10)
    assert np.array_equal(fd, td) and np.array_equal(fi, ti)
    pick = np.random.default_rng(2032).permutation(len(pts))[:20000]
    f.remove(pts[pick[:10000]])
    t0 = time.perf_counter()
    got = f.remove(pts[pick[10000:]])
    out["forest_remove_10000_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    assert np.array_equal(np.sort(got), np.sort(pick[10000:]))
    out["forest_remove_occupied_slots"] = occ
    f.close()
    return out


def octree_legs(tdtk, runs=5):
    """FindClosestBatch on the octree (BOctTree at the reference's voxel 10 with earlystop) and on the k-d tree (bucket 20):
    the same 1M-point uniform cloud (density 1), the same 1M queries (the points moved by N(0, 0.3)), maxdist2 625.  Five
    runs each, alternating between the two trees; end to end on the host clock and the search kernel from HIP events"""
    rng = np.random.default_rng(2033)
    pts = rng.uniform(-50, 50, (1_000_000, 3))
    q = pts + rng.normal(0.0, 0.3, pts.shape)
    t0 = time.perf_counter()
    oc = tdtk.BOctTree(pts)
    out = {"octree_build_ms_cold": round((time.perf_counter() - t0) * 1e3, 3)}
    out["octree_build"] = timed(lambda: tdtk.BOctTree(pts), 3)
    out["tree_build"] = timed(lambda: tdtk.KDtree(pts, 20), 3)
    kd = tdtk.KDtree(pts, 20)
    info = oc.info()
    out["octree_info"] = {k: info[k] for k in ("n_nodes", "n_leaves", "levels", "max_depth", "device_bytes")}
    oi, od = oc.FindClosestBatch(q, 625.0)             # warm: code objects, workspaces -- and the answers
    ki, kd2 = kd.FindClosestBatch(q, 625.0)
    same = np.array_equal(oi, ki)
    out["octree_equals_tree"] = bool(same)             # (a uniform cloud: no ties; a query within 0.01 of a point may differ)
    if not same:
        out["octree_differs_at"] = int((oi != ki).sum())
        assert (od[oi != ki] <= 0.0001).all()
    ts = {"octree": [], "tree": []}
    for _ in range(runs):
        for tag, t in (("octree", oc), ("tree", kd)):
            t0 = time.perf_counter()
            t.FindClosestBatch(q, 625.0)
            ts[tag].append((time.perf_counter() - t0) * 1e3)
    for tag, v in ts.items():
        out["%s_find_closest_1M" % tag] = {"min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "median_ms": round(float(np.median(v)), 3)}
    return out


def octree_icp_legs(tdtk, runs=5):
    """the resident octree ICP loop against the host-stepped one, ms per iteration (see the module docstring)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from boctree_model import dat_pair, move
    rng = np.random.default_rng(2033)
    pts = rng.uniform(-50, 50, (1_000_000, 3))
    A = tdtk.EulerToMatrix4([0.3, -0.2, 0.1], [0.002, -0.003, 0.001])
    sets = {"dat_pair": dat_pair() + (50,), "uniform_1M": (pts, move(pts + rng.normal(0.0, 0.3, pts.shape), A), 10)}
    z3 = [0.0, 0.0, 0.0]
    out = {}
    for tag, (model, data, iters) in sets.items():
        out["octree_icp_%s_iterations" % tag] = iters
        prev = tdtk.Scan(z3, z3, model).setSearchTreeParameter(2)
        prev.getSearchTree()

        def one(stepped, timing=False):
            cur = tdtk.Scan(z3, z3, data)
            _ = cur.handle
            icp = tdtk.icp6D(tdtk.icp6D_QUAT(True), 25.0, iters, quiet=True, epsilonICP=0.0)
            was = tdtk.lib().tdtk_kernel_timing(1 if timing else 0)
            t0 = time.perf_counter()
            it = icp._match_stepped(prev, cur) if stepped else icp.match(prev, cur)
            ms = (time.perf_counter() - t0) * 1e3
            tdtk.lib().tdtk_kernel_timing(was)
            assert it == iters - 1
            last = icp.last
            cur.release()
            return ms / iters, last
        ref = {False: one(False)[1], True: one(True)[1]}             # warm: code objects, workspaces -- and the answers
        out["octree_icp_%s_pairs_equal" % tag] = bool(np.array_equal(ref[False]["trace"][:, 0], ref[True]["trace"][:, 0]))
        out["octree_icp_%s_max_pose_diff" % tag] = float(np.abs(ref[False]["trace"][:, 2:] - ref[True]["trace"][:, 2:]).max())
        ts = {"resident": [], "stepped": []}
        for _ in range(runs):
            for name, stepped in (("resident", False), ("stepped", True)):
                ts[name].append(one(stepped)[0])
        for name, v in ts.items():
            out["octree_icp_%s_%s_ms_per_iteration" % (tag, name)] = {"min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                                                                      "median_ms": round(float(np.median(v)), 3)}
        ms, last = one(False, timing=True)
        out["octree_icp_%s_timed_run" % tag] = {"ms_per_iteration": round(ms, 3), "walk_ms_per_iteration": round(last["nn_ms"] / iters, 3),
                                                "sums_ms_per_iteration": round(last["sums_ms"] / iters, 3)}
        prev.release()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-queries", type=int, default=100000)
    ap.add_argument("--ref-threads", type=int, default=16)
    ap.add_argument("--segments", action="store_true", help="add the cylinder / box / segment query legs (1M points)")
    ap.add_argument("--only-segments", action="store_true", help="those legs alone")
    ap.add_argument("--adaptive", action="store_true", help="add the adaptive-k normals legs (1M points)")
    ap.add_argument("--only-adaptive", action="store_true", help="those legs alone")
    ap.add_argument("--hybrid", action="store_true", help="add the k-nearest-within-radius legs (1M points)")
    ap.add_argument("--only-hybrid", action="store_true", help="those legs alone")
    ap.add_argument("--collision", action="store_true", help="add the collision-detection legs (1M points, 3M items)")
    ap.add_argument("--only-collision", action="store_true", help="those legs alone")
    ap.add_argument("--clusters", action="store_true", help="add the radius-clustering legs (1M points, two radii)")
    ap.add_argument("--only-clusters", action="store_true", help="those legs alone")
    ap.add_argument("--only-peopleremover", action="store_true", help="dynamic-object removal on a synthetic room, alone")
    ap.add_argument("--only-hough", action="store_true", help="the standard 3D Hough transform at the reference's defaults, alone")
    ap.add_argument("--only-forest", action="store_true", help="the dynamic kd-forest against rebuilds and the single tree, alone")
    ap.add_argument("--only-octree", action="store_true", help="FindClosestBatch on the octree and on the k-d tree, alone")
    ap.add_argument("--only-octree-icp", action="store_true", help="the resident octree ICP loop against the host-stepped one, alone")
    args = ap.parse_args()
    tdtk = importlib.import_module("3dtk_amd")
    if tdtk.device_count() < 1:
        raise SystemExit("no HIP device: the measurements need the MI355X")
    out = {"workload": "kdtree_queries", "reps": args.reps}
    if args.only_peopleremover:
        out.update(peopleremover_legs(tdtk, args.reps))
        print(json.dumps(out))
        return
    if args.only_hough:
        out.update(hough_legs(tdtk, args.reps))
        print(json.dumps(out))
        return
    if args.only_forest:
        out.update(forest_legs(tdtk, args.reps))
        print(json.dumps(out))
        return
    if args.only_octree:
        out.update(octree_legs(tdtk))
        print(json.dumps(out))
        return
    if args.only_octree_icp:
        out.update(octree_icp_legs(tdtk))
        print(json.dumps(out))
        return
    rng = np.random.default_rng(2024)
    rpos = [0.0, 0.0, 0.0]
    if args.segments or args.only_segments:
        pts = np.random.default_rng(2025).uniform(-50, 50, (1_000_000, 3))
        out.update(segment_legs(tdtk, pts, "1M", np.random.default_rng(2026), args.reps, args.ref_queries, args.ref_threads))
        if args.only_segments:
            print(json.dumps(out))
            return
    if args.adaptive or args.only_adaptive:
        pts = np.random.default_rng(2027).uniform(-50, 50, (1_000_000, 3))
        # (the reference loop is Python glue around the library, about 1.2 ms per point: a fiftieth of --ref-queries)
        out.update(adaptive_legs(tdtk, pts, "1M", np.random.default_rng(2028), args.reps, args.ref_queries // 50, args.ref_threads))
        if args.only_adaptive:
            print(json.dumps(out))
            return
    if args.hybrid or args.only_hybrid:
        pts = np.random.default_rng(2029).uniform(-50, 50, (1_000_000, 3))
        out.update(hybrid_legs(tdtk, pts, "1M", args.reps))
        if args.only_hybrid:
            print(json.dumps(out))
            return
    if args.collision or args.only_collision:
        out.update(collision_legs(tdtk, args.reps, args.ref_threads))
        if args.only_collision:
            print(json.dumps(out))
            return
    if args.clusters or args.only_clusters:
        out.update(cluster_legs(tdtk, args.reps))
        if args.only_clusters:
            print(json.dumps(out))
            return
    for M in [int(s) for s in args.sizes.split(",")]:
        pts = rng.uniform(-50, 50, (M, 3)) * (M / 1e6) ** (1 / 3)     # same density at every size
        r2 = (20.0 * 3 / (4 * np.pi)) ** (2.0 / 3.0)                   # ~20 neighbours per query at that density
        kd = tdtk.KDtree(pts, 20)
        tag = "%dM" % (M // 1_000_000) if M >= 1_000_000 else str(M)
        for k in (10, 20):
            out["knn_k%d_%s" % (k, tag)] = timed(lambda: kd.kNearestNeighborsBatch(pts, k), args.reps)
        if M <= 1_000_000:
            out["range_20nn_%s" % tag] = timed(lambda: kd.fixedRangeSearchBatch(pts, r2), args.reps)
            off, _, _ = kd.fixedRangeSearchBatch(pts, r2)
            out["range_20nn_%s_mean_list" % tag] = round(float(off[-1]) / M, 2)
            for k in (10, 20):
                out["normals_knn_k%d_%s" % (k, tag)] = timed(lambda: tdtk.calculateNormalsKNN(pts, k, rpos), args.reps)
            out["normals_range_%s" % tag] = timed(lambda: tdtk.calculateNormalsRange(pts, r2, rpos), args.reps)
            out["normals_apxknn_k10_%s" % tag] = timed(lambda: tdtk.calculateNormalsApxKNN(pts, 10, rpos, 1.0), args.reps)
            from oracle import orc
            if orc.have_ref():
                out.update(ref_legs(pts, r2, tag, rng, args.ref_queries, args.ref_threads))
        del kd
    print(json.dumps(out))


if __name__ == "__main__":
    main()
