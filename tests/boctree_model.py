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


_generators = {}


def load_generator(name):
    """a fixture generator of tests/golden as a module, loaded once"""
    if name not in _generators:
        spec = importlib.util.spec_from_file_location(name, os.path.join(G, name + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        _generators[name] = m
    return _generators[name]


def generator():
    return load_generator("make_golden_boctree_search")


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


_models = {}


def model_of(fx, name, voxel, early):
    """the restatement over a fixture's cloud, built once per (fixture, case)"""
    key = (id(fx), name, voxel, early)
    if key not in _models:
        _models[key] = (fx, Model(fx.cloud(name), voxel, early))
    return _models[key][1]


def check_model_equals_fixture(fx, m, name, voxel, early):
    """the restatement's tree is the reference's: init()'s scalars by bits, countNodes / countOctLeaves / countPoints, the
    full leaf order; the table's own invariants"""
    pts = fx.cloud(name)
    assert same_bits(m.scalars, fx.get(name, voxel, early, "scalars"))
    assert [m.n_nodes, m.n_leaves, len(pts)] == [int(v) for v in fx.get(name, voxel, early, "counts")]
    assert same_bits(pts[m.leaf], pts[fx.get(name, voxel, early, "leaf")])
    # the table's own invariants: children in ascending child index behind `first`, leaf runs tile the point array in order
    valid = m.nodes[:, 0] & 0xFF
    leafm = (m.nodes[:, 0] >> 8) & 0xFF
    assert (leafm & ~valid).sum() == 0
    runs = []
    for s in range(len(m.nodes)):
        k = 0
        for ci in range(8):
            if (valid[s] >> ci) & 1:
                ch = m.nodes[s, 1] + k
                k += 1
                if (leafm[s] >> ci) & 1:
                    runs.append((int(m.nodes[ch, 2]), int(m.nodes[ch, 3])))
    runs.sort()
    assert runs[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(runs, runs[1:])) and runs[-1][0] + runs[-1][1] == len(pts)
    assert len(runs) == m.n_leaves


def check_lane_equals_batches(L, m, fx, name, voxel, early):
    """FindClosest of every query of every batch: the returned point (as the first position in leaf order with its
    coordinates: what strict < returns), Dist2 and the leaves scanned, by bits; returns the number of queries compared"""
    n = 0
    for qq, maxd2, pos, d2, leaves in fx.batches(name, voxel, early):
        slot, gd2, gl = lane_find(L, m, qq, maxd2)
        assert np.array_equal(slot, pos), (name, voxel, early, maxd2, np.flatnonzero(slot != pos)[:5])
        assert same_bits(gd2, d2) and np.array_equal(gl, leaves), (name, voxel, early, maxd2)
        n += len(qq)
    return n


def expect_idx(order, pos):
    """fixture positions in leaf order -> the caller's indices the device returns for them"""
    return np.where(pos >= 0, order[np.maximum(pos, 0)], -1).astype(np.int32)


def check_sums(got, model, A, want, producer, nrm=None, D=None):
    """the sums inside the tolerance pair_sums_ref derives from the pair list the call returned"""
    import pair_sums_ref as R
    shift = R.shift_of(model, A)
    fin = R.finished(got["p1"], got["p2"], nrm, shift, want, D)
    disc = R.discrimination(got["p1"], got["p2"], nrm, shift, want, D, fin=fin)
    R.check_struct(got["_raw"], fin, disc, producer)


def info_scalars(info):
    """BOctTree.info() in the order of the fixtures' `scalars`"""
    return np.array([info["max_depth"], info["real_voxelSize"], info["mult"], *info["add"], info["largest_index"], info["size"],
                     *info["center"]], np.float64)


def horn(p1, p2):
    """a rigid motion that takes p2 onto p1 in the least-squares sense (SVD), column-major like the library's"""
    c1, c2 = p1.mean(0), p2.mean(0)
    U, _, Vt = np.linalg.svd((p2 - c2).T @ (p1 - c1))
    R = (U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))]) @ Vt).T
    A = np.eye(4)
    A[:3, :3], A[:3, 3] = R, c1 - R @ c2
    return A.T.reshape(16)


# ---- the refusal bound: what the entry points admit may not let x +- closest_v leave int32 ----------------------------------------
TWO30 = 2.0 ** 30


def bound_tree():
    """[[-1,-1,-1],[1,1,1]] at voxel 0.1: mult 16, add 2"""
    m = Model(np.array([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]]), 0.1, False)
    assert m.mult == 16.0 and (m.add == 2.0).all()
    return m


def bound_cv(m, maxd2):
    return np.sqrt(maxd2) * m.mult + 1


def bound_cases(m):
    """[(tag, query, maxdist2, admitted)] around |v| == 2^30.  The radii are found by stepping nextafter around
    ((2^30 - 1) / mult)^2: `exact` is one whose sqrt * mult + 1 is 2^30, `below` the largest under it whose value is smaller."""
    exact = ((TWO30 - 1) / m.mult) ** 2
    for _ in range(64):
        if bound_cv(m, exact) == TWO30:
            break
        exact = np.nextafter(exact, np.inf if bound_cv(m, exact) < TWO30 else -np.inf)
    assert bound_cv(m, exact) == TWO30
    below = exact
    for _ in range(64):
        if bound_cv(m, below) < TWO30:
            break
        below = np.nextafter(below, -np.inf)
    assert bound_cv(m, below) < TWO30 <= bound_cv(m, np.nextafter(below, np.inf)) and int(bound_cv(m, below)) == 2 ** 30 - 1
    hi, lo = TWO30 / m.mult - 2.0, -TWO30 / m.mult - 2.0              # (q + add) * mult == +-2^30 exactly
    assert (hi + 2.0) * 16.0 == TWO30 and (lo + 2.0) * 16.0 == -TWO30
    hi_in, lo_in = np.nextafter(hi, 0.0), np.nextafter(lo, 0.0)
    assert int((hi_in + 2.0) * 16.0) == 2 ** 30 - 1 and int((lo_in + 2.0) * 16.0) == -(2 ** 30 - 1)
    q = lambda x: np.array([[x, 0.25, -0.5]])                         # noqa: E731
    return [("x=+2^30, cv=2^30", q(hi), exact, False), ("x=-2^30, cv=2^30", q(lo), exact, False),
            ("x=+2^30 alone", q(hi), 625.0, False), ("x=-2^30 alone", q(lo), 625.0, False),
            ("cv=2^30 alone", q(0.0), exact, False), ("cv=2^30 alone, y", np.array([[0.0, hi, 0.0]]), 625.0, False),
            ("x=2^30-1, cv=2^30-1", q(hi_in), below, True), ("x=-(2^30-1), cv=2^30-1", q(lo_in), below, True),
            ("x=2^30-1 alone", q(hi_in), 625.0, True), ("x=-(2^30-1) alone", q(lo_in), 625.0, True),
            ("cv=2^30-1 alone", q(0.0), below, True),
            ("all three axes at the bound", np.array([[hi_in, lo_in, hi_in], [lo_in, hi_in, lo_in]]), below, True)]


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
