"""Test helper of the octree ICP loop (tdtk_icp_match_octree): how the GPU tiers set a model scan up, run icp6D.match resident
or stepped, call the C entry point directly, and what a resident run is held to against the stepped one.  Shared by
tests/test_gpu_boctree_icp.py and tests/test_gpu_boctree_paths.py."""
import ctypes as C
from importlib import import_module

import numpy as np

import boctree_model as bm

Z3 = [0.0, 0.0, 0.0]
I16 = np.eye(4).reshape(16)
POSE_ATOL = 1e-9          # the project's pose bound


def minimizer(tdtk, algo):
    return {1: tdtk.icp6D_QUAT, 2: tdtk.icp6D_SVD, 5: tdtk.icp6D_HELIX, 6: tdtk.icp6D_APX, 10: tdtk.icp6D_NAPX}[algo](True)


def model_scan(tdtk, model, nns, voxel=10.0, early=1):
    """the model scan (pose zero: its original points are `model`) with its tree built"""
    s = tdtk.Scan(Z3, Z3, model).setSearchTreeParameter(nns)
    if nns == 2 and (voxel, early) != (10.0, 1):
        s.kd = tdtk.BOctTree(model, voxel, bool(early))          # a tree other than createSearchTreePrivate's
    s.getSearchTree()
    return s


def run(tdtk, prev, data, normals, algo, mode, maxd2, iters, eps, rnd=1, stepped=False):
    cur = tdtk.Scan(Z3, Z3, data, normals)
    _ = cur.handle
    icp = tdtk.icp6D(minimizer(tdtk, algo), float(np.sqrt(maxd2)), iters, quiet=True, rnd=rnd, epsilonICP=eps)
    assert icp.max_dist_match2 == maxd2
    if rnd > 1:
        C.CDLL(None).srand(11)
    if stepped:
        icp.stepped_rnd = True
        it = icp._match_stepped(prev, cur, mode)
    else:
        it = icp.match(prev, cur, mode)
    return it, icp.last, cur


def resident_against_stepped(tdtk, model, data, maxd2, iters):
    prev = model_scan(tdtk, model, 2)
    it, last, cur = run(tdtk, prev, data, None, 1, 0, maxd2, iters, 0.0)
    sit, slast, scur = run(tdtk, prev, data, None, 1, 0, maxd2, iters, 0.0, stepped=True)
    assert it == sit == iters - 1 and len(last["trace"]) == len(slast["trace"]) == iters
    print("max |alignxf resident - stepped|", np.abs(last["trace"][:, 2:] - slast["trace"][:, 2:]).max())
    assert np.array_equal(last["trace"][:, 0], slast["trace"][:, 0])
    assert np.allclose(last["trace"][:, 2:], slast["trace"][:, 2:], rtol=0, atol=POSE_ATOL)
    # the scan behind the resident loop: a copy moved by tdtk_scan_transform with the loop's own alignxf, row by row -- by bits
    copy = tdtk.Scan(Z3, Z3, data)
    for row in last["trace"]:
        A = np.ascontiguousarray(row[2:])
        assert tdtk.lib().tdtk_scan_transform(copy.handle, A.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert bm.same_bits(cur.get_xyz_reduced(), copy.get_xyz_reduced())
    assert np.allclose(cur.get_transMat(), scur.get_transMat(), rtol=0, atol=1e-8)
    return last


def c_match(tdtk, fn, tree_h, scan_h, algo, mode, iters, maxd2, eps=0.0):
    """the C entry point `fn` as it is: (rc, res, data_transMat, data_dalignxf, trace)"""
    cm = import_module("3dtk_amd._capi")
    prm = cm.IcpParams(int(algo), int(mode), int(iters), float(maxd2), float(eps), 1)
    res = cm.IcpResult()
    tm, da = np.eye(4).reshape(16).copy(), np.eye(4).reshape(16).copy()
    trace = np.zeros((max(1, iters), 18))
    dp = C.POINTER(C.c_double)
    rc = getattr(tdtk.lib(), fn)(tree_h, I16.ctypes.data_as(dp), scan_h, tm.ctypes.data_as(dp), da.ctypes.data_as(dp), C.byref(prm),
                                 C.byref(res), trace.ctypes.data_as(dp), len(trace))
    return rc, res, tm, da, trace
