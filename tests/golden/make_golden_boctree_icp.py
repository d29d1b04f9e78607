"""Generator of k21_boctree_icp.npz: icp6D::match on the octree search tree (`slam6D -t 2`), iteration by iteration, from the
reference's own compiled BOctTree<double>::FindClosest (RefBoct of make_golden_boctree_search.py) inside the oracle's loop
(oracle/icp_oracle.py: match, align, OScan.transform).

    python tests/golden/make_golden_boctree_icp.py        (needs the reference checkout, as make_golden_boctree_search.py)

An iteration is: FindClosest on the current data (searchTree.cc:92-189 around it: the query into the tree's frame, the pair
(transform3(dalignxf, closest), query), in pairing mode 2 the closest point projected onto the query's normal), the minimizer's
align, the move.  The loop itself (`loop`) takes the search as a function, so the CPU tier drives the walk the device runs
(oct_lane.h on the host) through the very same code.

Clouds.  `seam` is the case that separates an octree loop from a k-d loop: 100 queries that settle 0.001 left of the root's x
plane, each with a model point 0.005 further left (within 0.01: FindClosest accepts it and ends the search) and a NEARER one
0.002 to its right, across the plane, which the search never gets to.  From iteration 2 on almost every one of those queries
is answered by the point that is not the nearest.  `octants`, `duplicates`, `one`, `two` are clouds of the search fixture with
its own queries as data: ties and exact duplicates at iteration 0 (one iteration), and the break at <= 3 pairs.

Per run, key prefix <cloud>_v<voxel>_e<0|1>_a<algo>_m<mode>[_<tag>]_ :
  iterations, converged   what icp6D::match returns / whether the epsilon test ended it
  pairs    [passes]       pairs of every pass (a pass that finds <= 3 ends the loop: it is the last entry and has no row below)
  rms, xf  [rows], [rows][16]   the minimizer's return value and alignxf per completed iteration
  hash     [passes] uint64      XOR over the found queries of (model index * 1315423911 + query index) (oracle/oracle.c:555-562),
                                the model index being the smallest cloud row with the returned coordinates
  pos      [passes][N] int32    the returned point as the first position in leaf order with its coordinates, -1 for none
  far      [passes]             queries answered by a point that is not the nearest one
The clouds are stored as plain float64 (<cloud>_model, _data, _normals): the seam's coordinates lie on no binary grid.

What the seam is there for is asserted here on the reference alone: at least 50 answers that are not the nearest in some pass
of every run whose minimizer moves the scan (NAPX under pairing mode 2 with the seam's constant normals does not: its system
is singular, the run pins the pairs of mode 2 and the rule for a minimizer that fails -- rms -1, the identity, the loop goes
on), and every query's answer in every pass of every run unchanged when the query moves by +-1e-5 along each axis -- four orders
above the 1e-9 the poses are pinned to times the coordinates' size (<= 70): a loop that reproduces the poses to that bound
cannot land on another answer, so indices and hashes are compared exactly."""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

import importlib.util


def _sibling(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


gs = _sibling("make_golden_boctree_search")
mo = gs.mo

OUT = os.path.join(_HERE, "k21_boctree_icp.npz")
MAX_BYTES = mo.MAX_BYTES
have_ref = gs.have_ref

QUAT, SVD, HELIX, APX, NAPX = 1, 2, 5, 6, 10
I16 = np.eye(4).reshape(16)
PROBE = 1e-5
SEAM_MAXD2, SEAM_ITERS = 25.0, 8


def seam():
    from oracle import icp_oracle as io
    rng = np.random.default_rng(11)
    bg = rng.integers(-160, 160, (900, 3)) / 4
    bg = bg[np.abs(bg[:, 0]) > 2]
    yz = rng.integers(-140, 140, (100, 2)) / 4
    left = np.column_stack([np.full(100, -0.006), yz])
    right = np.column_stack([np.full(100, 0.001), yz])
    model = np.concatenate([40 * gs.SIGNS, bg, left, right])
    data = np.concatenate([bg[::2], np.column_stack([np.full(100, -0.001), yz])])
    data = data + rng.normal(0, 0.0003, data.shape)
    data = move(data, io.euler_to_matrix4([0.75, -0.5, 0.25], [0.01, -0.015, 0.02]))
    return np.ascontiguousarray(model), np.ascontiguousarray(data)


def move(p, A):
    return np.stack([p[:, 0] * A[k] + p[:, 1] * A[4 + k] + p[:, 2] * A[8 + k] + A[12 + k] for k in range(3)], 1)


def seam_normals(n):
    """constant over the scan, as a wall's.  NAPX's 6 x 6 system then has a block of rank one and cannot be solved: the run
    pins pairing mode 2's pairs and the rule for a minimizer that fails (rms -1, the identity, the loop goes on)"""
    return np.tile([0.6, 0.0, 0.8], (n, 1))


def clouds():
    """name -> (model, data, normals or None)"""
    c = gs.clouds()
    q = gs.queries(c)
    m, d = seam()
    out = {"seam": (m, d, seam_normals(len(d)))}
    for name in ("octants", "duplicates", "one"):
        out[name] = (c[name], q[name][0][0], None)
    out["two"] = (c["two"], q["two"][0][0][:3], None)           # three queries: <= 3 pairs
    return out


# (cloud, voxel, earlystop, algo, pairing mode, maxdist2, max_num_iterations, epsilonICP, tag)
RUNS = tuple(("seam", v, e, a, 0, SEAM_MAXD2, SEAM_ITERS, 0.0, "") for v, e in ((10.0, 1), (0.5, 0)) for a in (QUAT, SVD, APX, HELIX)) + \
       tuple(("seam", v, e, NAPX, 2, SEAM_MAXD2, SEAM_ITERS, 0.0, "") for v, e in ((10.0, 1), (0.5, 0))) + \
       (("seam", 10.0, 1, QUAT, 0, SEAM_MAXD2, 30, 1e-6, "eps"),            # ended by the epsilon test
        ("octants", 10.0, 1, QUAT, 0, 1e4, 1, 1e-7, ""), ("duplicates", 10.0, 1, QUAT, 0, 100.0, 1, 1e-7, ""),
        ("one", 10.0, 1, QUAT, 0, 625.0, 5, 1e-7, ""), ("two", 10.0, 1, QUAT, 0, 625.0, 5, 1e-7, ""))


def prefix(run):
    name, voxel, early, algo, mode, _, _, _, tag = run
    return "%s_v%g_e%d_a%d_m%d%s_" % (name, voxel, early, algo, mode, "_" + tag if tag else "")


def k5_hash(idx):
    """oracle/oracle.c:555-562 over one pass's indices (caller order, -1: none)"""
    idx = np.asarray(idx, np.int64)
    i = np.flatnonzero(idx >= 0).astype(np.uint64)
    if not len(i):
        return np.uint64(0)
    return np.bitwise_xor.reduce(idx[idx >= 0].astype(np.uint64) * np.uint64(1315423911) + i)


class _Source:
    """the model scan of the oracle's match: identity pose, its tree answers through `find`"""

    def __init__(self, pts, rep_leaf, find, hook=None):
        self.pts, self.rep_leaf, self.find, self.hook = pts, rep_leaf, find, hook
        self.dalignxf = I16.copy()
        self.passes = []

    def tree(self):
        return self

    def get_pt_pairs(self, A, xyz, nrm, start, end, mode, maxd2):
        """SearchTree::getPtPairs (searchTree.cc:92-189), the arithmetic of oracle.c's orc_get_pt_pairs"""
        from oracle import orc
        inv, _ = orc.m4inv(A)
        q = move(xyz, inv)                                                         # :122
        pos = np.asarray(self.find(q, maxd2), np.int32)
        found = pos >= 0
        idx = np.where(found, self.rep_leaf[np.maximum(pos, 0)], -1).astype(np.int32)
        if self.hook:
            self.hook(q, maxd2, pos)
        self.passes.append((pos, idx, q))
        p2 = xyz[found]
        p1 = move(self.pts[idx[found]], A)                                         # :147
        pn = np.zeros_like(p2)
        if mode != 0:
            n = nrm[found]
            pn = n / np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])[:, None]      # Normalize3
        if mode == 2:                                                              # :149-162
            t = p1 - p2
            dot = pn[:, 0] * t[:, 0] + pn[:, 1] * t[:, 1] + pn[:, 2] * t[:, 2]
            p1 = pn * dot[:, None] + p2
        return dict(idx=idx, p1=p1, p2=p2, pn=pn, n=int(found.sum()), sum=float(((p1 - p2) ** 2).sum()),
                    centroid_m=p1.sum(0), centroid_d=p2.sum(0))


def loop(run, cloud, rep_leaf, find, hook=None):
    """one run through oracle.icp_oracle.match with `find(q, maxd2) -> positions in leaf order` as the tree's FindClosest;
    rep_leaf [n]: the smallest cloud row with the coordinates of every position in leaf order.  Returns the run's arrays."""
    from oracle import icp_oracle as io
    name, voxel, early, algo, mode, maxd2, iters, eps, tag = run
    model, data, normals = cloud
    src = _Source(model, rep_leaf, find, hook)
    cur = io.OScan([0, 0, 0], [0, 0, 0], data, normals if (mode != 0 or algo == NAPX) else None)
    it, trace = io.match(src, cur, algo, maxd2, iters, eps, mode)
    z = {}
    z["iterations"] = np.array(it, np.int32)
    few = len(trace) < len(src.passes)                 # the last pass found <= 3 pairs
    z["converged"] = np.array(0 if few else int(it != iters - 1), np.int32)
    z["pairs"] = np.array([int((p[1] >= 0).sum()) for p in src.passes], np.int64)
    z["rms"] = np.array([t[1] for t in trace], np.float64)
    z["xf"] = np.array([t[2] for t in trace], np.float64).reshape(-1, 16)
    z["hash"] = np.array([k5_hash(p[1]) for p in src.passes], np.uint64)
    z["pos"] = np.array([p[0] for p in src.passes], np.int32)
    far = []
    for pos, idx, q in src.passes:
        d2 = ((q[:, None, :] - model[None, :, :]) ** 2).sum(2)
        got = np.where(idx >= 0, d2[np.arange(len(q)), np.maximum(idx, 0)], np.inf)
        far.append(int(((idx >= 0) & (got > d2.min(1))).sum()))
    z["far"] = np.array(far, np.int32)
    if eps > 0 and not few and len(trace) > 2:
        # the epsilon test must not sit on its threshold: every difference it looked at is clear of eps by more than the 1e-9
        # the rms values are pinned to
        r = [0.0, 0.0] + [t[1] for t in trace]
        for k in range(2, len(r)):
            for d in (abs(r[k] - r[k - 1]), abs(r[k] - r[k - 2])):
                assert abs(d - eps) > 1e-8, (prefix(run), k, d)
    return z


def ref_find(model, voxel, early):
    """(find, rep_leaf) of the reference's own tree"""
    t = gs.RefBoct(model, voxel, early)
    rep_leaf = mo.rep_index(model, t.all_points())

    def find(q, maxd2):
        found, xyz, _, _ = t.find(q, maxd2)
        return gs.first_pos(model, rep_leaf, xyz, found)
    find.tree = t
    return find, rep_leaf


def compute():
    c, z = clouds(), {}
    for name, (m, d, nrm) in c.items():
        z[name + "_model"], z[name + "_data"] = m, d
        if nrm is not None:
            z[name + "_normals"] = nrm
    assert len(c["seam"][0]) == 1065 and len(c["seam"][1]) == 529
    assert np.array_equal(0.5 * (c["seam"][0].min(0) + c["seam"][0].max(0)), np.zeros(3))        # the root centre
    for run in RUNS:
        model = c[run[0]][0]
        find, rep_leaf = ref_find(model, run[1], run[2])
        unstable = []

        def hook(q, maxd2, pos):
            """every answer again with the query moved by +-PROBE along each axis"""
            bad = np.zeros(len(q), bool)
            for ax in range(3):
                for s in (-PROBE, PROBE):
                    p = q.copy()
                    p[:, ax] += s
                    bad |= find(p, maxd2) != pos
            unstable.append(int(bad.sum()))
        r = loop(run, c[run[0]], rep_leaf, find, hook if run[0] == "seam" else None)
        if run[0] == "seam":
            if run[3] == NAPX:
                # constant normals leave NAPX's system singular -- a pivot below choldc's 1e-7 by twelve orders, on any
                # rounding --: every iteration returns -1 and the identity (icp6Dnapx.cc:103-108), the scan stays where it is
                assert (r["rms"] == -1.0).all() and (r["xf"] == I16).all() and len(r["rms"]) == SEAM_ITERS
            else:
                assert r["far"].max() >= 50, (prefix(run), r["far"])
            assert sum(unstable) == 0, (prefix(run), unstable)
            assert (r["pairs"] == 529).all()
        for k, v in r.items():
            z[prefix(run) + k] = v
    p = prefix(RUNS[0])
    assert z[p + "iterations"] == SEAM_ITERS - 1 and len(z[p + "rms"]) == SEAM_ITERS and abs(z[p + "rms"][-1] - 0.00203) < 1e-5
    pe = prefix(RUNS[10])
    assert RUNS[10][8] == "eps" and z[pe + "converged"] == 1 and 2 < z[pe + "iterations"] < 29
    for name in ("one", "two"):
        pr = prefix([r for r in RUNS if r[0] == name][0])
        assert z[pr + "iterations"] == 0 and len(z[pr + "rms"]) == 0 and len(z[pr + "pairs"]) == 1 and 0 < z[pr + "pairs"][0] <= 3
    return z


def load(path=OUT):
    return dict(np.load(path))


def cloud_of(z, name):
    return z[name + "_model"], z[name + "_data"], z.get(name + "_normals")


if __name__ == "__main__":
    if not have_ref():
        raise SystemExit("needs the reference checkout at %s (src/slam6d/Boctree.cc)" % gs.REF)
    z = compute()
    mo.save(z, OUT)
    size = os.path.getsize(OUT)
    print("wrote %s (%d arrays, %d bytes)" % (OUT, len(z), size))
    for run in RUNS:
        p = prefix(run)
        print("  %-28s it %2d conv %d pairs %s far %s rms %s" % (p, z[p + "iterations"], z[p + "converged"], z[p + "pairs"][:4], z[p + "far"],
                                                                   np.round(z[p + "rms"][-1:], 6)))
    assert size <= MAX_BYTES, size
