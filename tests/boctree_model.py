"""Test helper of the octree search tree (tdtk_octree_*): a plain Python restatement of the reference's BOctTree<double> build
(constructor Boctree.h:224-270, branch :1164-1195, countPointsAndQueueFast :1267-1301, fullsort / sort :1737-1816, init
:333-356) that lays the tree out as the device's node table (oct_lane.h), the loader of the fixture's generator, and the
host build of the per-lane walk (oct_lane.h under tests/host_oct_shim.h) that the CPU tier runs over that table."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")

KDPOINT = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("orig", "<i4"), ("pad", "<i4")])


def generator():
    spec = importlib.util.spec_from_file_location("make_golden_boctree_search", os.path.join(G, "make_golden_boctree_search.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _sort(P, a, lo, n, split, axis):
    """sort (Boctree.h:1783-1817): the two-pointer partition of a[lo : lo + n] by P[.][axis] < split; returns the cut"""
    if n == 0:
        return lo
    if n == 1:
        return lo + 1 if P[a[lo]][axis] < split else lo
    left, right = lo, lo + n - 1
    while True:
        while P[a[left]][axis] < split:
            left += 1
            if right < left:
                break
        if right < left:
            break
        while P[a[right]][axis] >= split:
            right -= 1
            if right < left:
                break
        if right < left:
            break
        a[left], a[right] = a[right], a[left]
    return left


def _fullsort(P, a, lo, n, c):
    """fullsort (Boctree.h:1737-1780): z, then y inside each half, then x inside each quarter; the nine block bounds"""
    b = [lo] * 9
    b[8] = lo + n
    L0 = _sort(P, a, lo, n, c[2], 2)
    L1 = _sort(P, a, lo, L0 - lo, c[1], 1)
    b[1] = _sort(P, a, lo, L1 - lo, c[0], 0)
    b[2] = L1
    b[3] = _sort(P, a, L1, L0 - L1, c[0], 0)
    b[4] = L0
    L1 = _sort(P, a, L0, lo + n - L0, c[1], 1)
    b[5] = _sort(P, a, L0, L1 - L0, c[0], 0)
    b[6] = L1
    b[7] = _sort(P, a, L1, lo + n - L1, c[0], 0)
    return b


class Model:
    """nodes: uint32 [slots][4] = (valid | leaf << 8, first child's slot, start, count), the root in slot 0, level by level,
    a level in depth-first order; leaf: the cloud rows in leaf order; pts: the KdPoint array; scalars as the fixture's"""

    def __init__(self, pts, voxel, earlystop):
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        P = [tuple(float(v) for v in p) for p in pts]
        n = len(P)
        lo, hi = pts.min(0), pts.max(0)
        center = [float(0.5 * (lo[k] + hi[k])) for k in range(3)]
        size = max(max(0.5 * (hi[0] - lo[0]), 0.5 * (hi[1] - lo[1])), 0.5 * (hi[2] - lo[2]))
        size = float(size + 1.0)
        a = list(range(n))
        levels = [[]]          # levels[d]: the nodes of depth d as [masks, first, start, count, children]

        def children_of(node, start, cnt, c, sz, depth):
            """countPointsAndQueueFast: the node's occupied octants become children of half size sz"""
            b = _fullsort(P, a, start, cnt, c)
            if len(levels) <= depth + 1:
                levels.append([])
            for j in range(8):
                m = b[j + 1] - b[j]
                if m <= 0:
                    continue
                cc = [c[k] + sz if (j >> k) & 1 else c[k] - sz for k in range(3)]      # childcenter: pcenter -/+ size / 2
                child = [0, 0, b[j], m, []]
                node[0] |= 1 << j
                node[4].append(child)
                levels[depth + 1].append(child)
                if sz <= voxel or (earlystop and m <= 10):                             # branch: a leaf
                    node[0] |= 0x100 << j
                else:
                    children_of(child, b[j], m, cc, sz / 2.0, depth + 1)

        root = [0, 0, 0, n, []]
        levels[0].append(root)
        children_of(root, 0, n, center, size / 2.0, 0)
        slot, k = {}, 0
        for lv in levels:
            for nd in lv:
                slot[id(nd)] = k
                k += 1
        nodes = np.zeros((k, 4), np.uint32)
        for lv in levels:
            for nd in lv:
                nodes[slot[id(nd)]] = (nd[0], slot[id(nd[4][0])] if nd[4] else 0, nd[2], nd[3])
        self.nodes = nodes
        self.leaf = np.array(a, np.int64)
        self.n_leaves = sum(1 for lv in levels for nd in lv if not nd[4] and nd is not root)
        self.n_nodes = k - self.n_leaves
        kp = np.zeros(n, KDPOINT)
        kp["x"], kp["y"], kp["z"], kp["orig"] = pts[self.leaf, 0], pts[self.leaf, 1], pts[self.leaf, 2], self.leaf
        self.pts = kp
        # init()
        rv, max_depth = size, 1
        while rv > voxel:
            rv = rv / 2.0
            max_depth += 1
        self.max_depth, self.real_voxelSize, self.mult = max_depth, rv, 1.0 / rv
        self.add = np.array([-center[k] + size for k in range(3)])
        self.top_bit = 1 << (max_depth - 1)
        self.largest_index = self.top_bit * 2 - 1
        self.size, self.center = size, np.array(center)
        self.scalars = np.array([max_depth, rv, self.mult, *self.add, self.largest_index, size, *center])


_lane = None


def host_lane(tmp_dir):
    """oct_lane.h compiled for the host (FMA contraction off, like the library)"""
    global _lane
    if _lane is None:
        csrc = os.path.join(ROOT, "3dtk_amd", "csrc")
        cc = os.path.join(str(tmp_dir), "oct_host.cc")
        with open(cc, "w") as f:
            f.write('#include "host_oct_shim.h"\n')
        so = os.path.join(str(tmp_dir), "liboct_host.so")
        r = subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                            "-I" + csrc, "-I" + os.path.join(ROOT, "tests"), cc, "-o", so], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        L = C.CDLL(so)
        L.oct_host_find.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_uint, C.c_void_p, C.c_int, C.c_double,
                                    C.c_void_p, C.c_void_p, C.c_void_p]
        L.oct_host_order.argtypes = [C.c_int, C.c_void_p]
        _lane = L
    return _lane


def lane_find(L, m, q, maxd2):
    """the host lane over the model m: (slot in leaf order or -1, d2, leaves scanned), or None where the batch is refused"""
    q = np.ascontiguousarray(q, np.float64).reshape(-1, 3)
    K = len(q)
    slot, d2, leaves = np.empty(K, np.int32), np.empty(K), np.empty(K, np.int32)
    add = np.ascontiguousarray(m.add, np.float64)
    rc = L.oct_host_find(m.nodes.ctypes.data, m.pts.ctypes.data, add.ctypes.data, float(m.mult), int(m.largest_index), int(m.top_bit),
                         q.ctypes.data, K, float(maxd2), slot.ctypes.data, d2.ctypes.data, leaves.ctypes.data)
    return None if rc else (slot, d2, leaves)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- the bundled scan pair of the ICP-by-hand tests ----------------------------------------------------------------------------
def dat_pair():
    """model: scan000 as it is (its pose is zero); data: scan001 moved by its pose, as transform3 moves a point"""
    z = np.load(os.path.join(G, "dat_scans.npz"))
    rP, rT = z["pose001"][:3], z["pose001"][3:]
    sx, cx, sy, cy, sz, cz = np.sin(rT[0]), np.cos(rT[0]), np.sin(rT[1]), np.cos(rT[1]), np.sin(rT[2]), np.cos(rT[2])
    A = np.array([cy * cz, sx * sy * cz + cx * sz, -cx * sy * cz + sx * sz, 0.0,              # EulerToMatrix4, globals.icc:501-531
                  -cy * sz, -sx * sy * sz + cx * cz, cx * sy * sz + sx * cz, 0.0,
                  sy, -sx * cy, cx * cy, 0.0, rP[0], rP[1], rP[2], 1.0])
    return np.ascontiguousarray(z["scan000"]), move(np.ascontiguousarray(z["scan001"]), A)


def move(p, A):
    return np.stack([p[:, 0] * A[k] + p[:, 1] * A[4 + k] + p[:, 2] * A[8 + k] + A[12 + k] for k in range(3)], 1)
