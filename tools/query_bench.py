"""k-NN / fixed-radius search and the KNN / range normals on the MI355X: warm end-to-end times (host clock around the
synchronising library call; host arrays in and out), next to calculateNormalsApxKNN on the same cloud and the reference
library's KDtreeIndexed on the host (an OpenMP loop of --ref-threads threads over a --ref-queries subset of the cloud,
scaled up to the whole cloud; labelled as such).  Prints one JSON line.

    python tools/query_bench.py [--sizes 1000000,10000000] [--reps 5] [--ref-queries 100000] [--ref-threads 16]

Kernel times: run the same command under `rocprofv3 --kernel-trace --stats` (k_knn_reg, k_range_count / k_range_fill,
k_range_normals)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-queries", type=int, default=100000)
    ap.add_argument("--ref-threads", type=int, default=16)
    args = ap.parse_args()
    tdtk = importlib.import_module("3dtk_amd")
    if tdtk.device_count() < 1:
        raise SystemExit("no HIP device: the measurements need the MI355X")
    out = {"workload": "kdtree_queries", "reps": args.reps}
    rng = np.random.default_rng(2024)
    rpos = [0.0, 0.0, 0.0]
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
