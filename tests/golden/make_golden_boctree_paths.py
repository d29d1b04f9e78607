"""Generator of k22_boctree_paths.npz: the reference's own compiled BOctTree<double> as a search tree (built and driven exactly
as make_golden_boctree_search.py does it, whose RefBoct, packing, first_pos, prefix and Fixture reader are imported) on the
clouds that reach what k20_boctree_search.npz leaves out:

  sweep_n<n>  n = 1 .. 257 points on a quarter grid under five (voxel, earlystop): the early-stop window clamped at both ends of
              the sorted keys (n < 21), n on both sides of 10 and 20, one level (voxel 1e6) to eight; 40 queries each with
              frequent ties, at maxdist2 9, 1e4 and 0
  ends_a/_b   a cluster of 10 and one of 11 points in the lowest and the highest corner of the cube: runs of exactly 10 and 11
              at sorted position 0 and n - 1
  heavy       groups of 10, 11, 12 and 25 IDENTICAL points: with earlystop a group of more than 10 never gets to `<= 10`, runs
              to full depth as a chain of single children and ends in a leaf of more than 10 points
  eleven      eleven copies of one point alone at voxel 0.001: 11 slots, a chain of 10 levels
  planar      300 points with z == 2: extent 0 on one axis
  deep        make_golden_octree.py's deep21 cloud at voxel 0.0005: 21 levels, searched; at maxdist2 4e6 the box covers the cube
              and branching starts at the root (the cloud is not stored: its digest is)

    python tests/golden/make_golden_boctree_paths.py        (needs the reference checkout, as the generator it imports)

Per case (cloud, voxel, earlystop), key prefix <cloud>_v<voxel>_e<0|1>_ as in k20: scalars, counts, leaf, and pos / d2 / leaves
as [batches][queries] -- a cloud's batches are its one query array <cloud>_q at each radius of <cloud>_maxd2.
Also imported by the tests."""
import hashlib
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))
import boctree_model as bm                          # noqa: E402

gold = bm.generator()                               # make_golden_boctree_search
mo = gold.mo                                        # make_golden_octree
RefBoct, first_pos, prefix, have_ref = gold.RefBoct, gold.first_pos, gold.prefix, gold.have_ref

OUT = os.path.join(_HERE, "k22_boctree_paths.npz")
MAX_BYTES = gold.MAX_BYTES

SWEEP_N = (1, 2, 3, 9, 10, 11, 12, 20, 21, 22, 64, 257)
SWEEP_VARIANTS = ((0.5, 0), (0.5, 1), (3.0, 1), (10.0, 1), (1e6, 0))
SWEEP_RADII = (9.0, 1e4, 0.0)
ENDS = (("ends_a", (10, 11)), ("ends_b", (11, 10)))       # (points in the lowest corner, in the highest)
HEAVY_GROUPS = ((10, (-12.03125, 5.03125, 3.03125)), (11, (9.53125, -7.46875, 11.03125)), (12, (-3.46875, -14.96875, -9.96875)),
                (25, (14.03125, 12.53125, -5.46875)))
ELEVEN = (0.40625, -1.71875, 2.53125)
DEEP_VOXEL = 0.0005
DEEP_RADII = (0.01, 4e6)


def clouds():
    c = {}
    rng = np.random.default_rng(22)
    for n in SWEEP_N:
        c["sweep_n%d" % n] = rng.integers(-64, 64, (n, 3)) / 4.0
    rng = np.random.default_rng(2201)
    mid = rng.integers(-32, 32, (40, 3)) / 4.0
    for name, (n_lo, n_hi) in ENDS:
        lo = -32.0 + rng.integers(0, 16, (n_lo, 3)) / 16.0
        hi = 32.0 - rng.integers(0, 16, (n_hi, 3)) / 16.0
        lo[0], hi[0] = -32.0, 32.0                         # the cube: centre 0, half edge 33
        c[name] = rng.permutation(np.concatenate([mid, lo, hi]))
    rng = np.random.default_rng(2202)
    parts = [np.tile(p, (cnt, 1)) for cnt, p in HEAVY_GROUPS] + [rng.integers(-64, 64, (30, 3)) / 4.0, [[-16.0] * 3, [16.0] * 3]]
    c["heavy"] = rng.permutation(np.concatenate(parts))
    c["eleven"] = np.tile(ELEVEN, (11, 1))
    rng = np.random.default_rng(2203)
    pl = np.empty((300, 3))
    pl[:, :2] = rng.integers(-200, 200, (300, 2)) / 8.0
    pl[:, 2] = 2.0
    c["planar"] = pl
    c["deep"] = mo.clouds()["deep21"]
    return {k: np.ascontiguousarray(v, np.float64) for k, v in c.items()}


def queries(c):
    """per cloud (queries, radii): a cloud's batch b is its queries at radii[b]"""
    q = {}
    rng = np.random.default_rng(22)
    for n in SWEEP_N:
        rng.integers(-64, 64, (n, 3))                      # (the cloud's own draw: the queries continue the stream behind it)
    for n in SWEEP_N:
        pts = c["sweep_n%d" % n]
        q["sweep_n%d" % n] = (np.concatenate([rng.integers(-80, 81, (16, 3)) / 4.0, rng.uniform(-20.0, 20.0, (16, 3)),
                                              pts[np.arange(8) % n] + [2.0 ** -7, 0.0, 0.0]]), SWEEP_RADII)
    rng = np.random.default_rng(2211)
    for name, _ in ENDS:
        pts = c[name]
        corner = pts[np.abs(pts).min(1) > 30.0]
        q[name] = (np.concatenate([corner + 2.0 ** -7, corner[::3] - [0.25, 0.0, 0.5], [[-40.0] * 3, [40.0] * 3, [-33.0, -33.0, 33.0]],
                                   rng.integers(-140, 141, (16, 3)) / 4.0]), (9.0, 1e4))
    g = np.array([p for _, p in HEAVY_GROUPS])
    q["heavy"] = (np.concatenate([g, g + [2.0 ** -7, 0.0, 0.0], g - [0.0, 0.5, 0.25], g + 0.0625, rng.integers(-70, 71, (20, 3)) / 4.0]),
                  (1.0, 1e4, 0.0))
    e = np.array(ELEVEN)
    q["eleven"] = (np.array([e, e + [2.0 ** -7, 0.0, 0.0], e + [0.0, 2.0 ** -10, 0.0], e + [1.0, 0.0, 0.0], e - 0.75, e + [0.0, 30.0, 0.0]]),
                   (1.0, 1e4, 0.0))
    pl = c["planar"]
    q["planar"] = (np.concatenate([pl[:20] + [0.0, 0.0, 0.75], pl[20:40] - [0.0, 0.0, 1.5], pl[40:50] + [0.125, 0.0, 0.0],
                                   pl[50:60] + [2.0 ** -7, 0.0, 0.0], np.c_[rng.integers(-120, 121, (20, 2)) / 4.0, np.full(20, 2.0)],
                                   rng.integers(-120, 121, (20, 3)) / 4.0]), (9.0, 1e4))
    deep = c["deep"]
    q["deep"] = (deep[:5000:50] + np.random.default_rng(7).integers(-64, 64, (100, 3)) / 2.0 ** 11, DEEP_RADII)
    return {k: (np.ascontiguousarray(a, np.float64), tuple(r)) for k, (a, r) in q.items()}


# (cloud, ((voxel, earlystop), ...)), in the fixture's order
CASES = tuple(("sweep_n%d" % n, SWEEP_VARIANTS) for n in SWEEP_N) + \
    (("ends_a", ((0.5, 1), (0.5, 0))), ("ends_b", ((0.5, 1), (0.5, 0))), ("heavy", ((0.125, 1), (0.125, 0))), ("eleven", ((0.001, 1),)),
     ("planar", ((10.0, 1), (0.5, 0))), ("deep", ((DEEP_VOXEL, 0), (DEEP_VOXEL, 1))))
NOT_STORED = ("deep",)                              # clouds rebuilt from their seed; the fixture holds <cloud>_sha256


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, np.float64).tobytes()).digest(), np.uint8)


def leaf_depths(m):
    """per position of the restatement's leaf order: the depth of the leaf that holds it (the root's children: 1)"""
    out = np.zeros(len(m.leaf), np.int32)
    todo = [(0, 0)]
    while todo:
        s, d = todo.pop()
        valid, leafm, k = int(m.nodes[s, 0]) & 0xFF, (int(m.nodes[s, 0]) >> 8) & 0xFF, 0
        for ci in range(8):
            if (valid >> ci) & 1:
                ch = int(m.nodes[s, 1]) + k
                k += 1
                if (leafm >> ci) & 1:
                    out[int(m.nodes[ch, 2]):int(m.nodes[ch, 2]) + int(m.nodes[ch, 3])] = d + 1
                else:
                    todo.append((ch, d + 1))
    return out


def leaves_of(m):
    """the restatement's leaves as (start, count, depth), in leaf order"""
    d = leaf_depths(m)
    cut = np.flatnonzero(np.r_[True, np.diff(_leaf_id(m)) != 0, True])
    return [(int(a), int(b - a), int(d[a])) for a, b in zip(cut[:-1], cut[1:])]


def _leaf_id(m):
    out = np.zeros(len(m.leaf), np.int64)
    valid, leafm = m.nodes[:, 0] & 0xFF, (m.nodes[:, 0] >> 8) & 0xFF
    for s in range(len(m.nodes)):
        k = 0
        for ci in range(8):
            if (valid[s] >> ci) & 1:
                ch = int(m.nodes[s, 1]) + k
                k += 1
                if (leafm[s] >> ci) & 1:
                    out[int(m.nodes[ch, 2]):int(m.nodes[ch, 2]) + int(m.nodes[ch, 3])] = ch
    return out


def case_rows(pts, voxel, early, qq, radii):
    """one case's arrays from the live reference, by their key suffix"""
    t = RefBoct(pts, voxel, early)
    z = {}
    z["scalars"], z["counts"] = t.info()
    leaf = mo.rep_index(pts, t.all_points())
    z["leaf"] = leaf.astype(np.int32)
    pos, d2, leaves = [], [], []
    for maxd2 in radii:
        found, xyz, gd2, gl = t.find(qq, maxd2)
        pos.append(first_pos(pts, leaf, xyz, found))
        d2.append(gd2)
        leaves.append(gl)
    z["pos"], z["d2"], z["leaves"] = np.array(pos, np.int32), np.array(d2), np.array(leaves, np.int32)
    return z


def _model_of_reference(c, z, name, voxel, early):
    """the restatement, once the reference has confirmed its counts and leaf order for this case"""
    m = bm.Model(c[name], voxel, early)
    p = prefix(name, voxel, early)
    assert [m.n_nodes, m.n_leaves, len(c[name])] == [int(v) for v in z[p + "counts"]], name
    assert bm.same_bits(c[name][m.leaf], c[name][z[p + "leaf"]]), name
    return m


def check_properties(c, q, z):
    """what the cases are there for, asserted on the reference's own answers"""
    # sweep: every query finds a point at 1e4, none at 0, and the searches branch
    many = total = 0
    for n in SWEEP_N:
        for voxel, early in SWEEP_VARIANTS:
            p = prefix("sweep_n%d" % n, voxel, early)
            pos, d2, leaves = z[p + "pos"], z[p + "d2"], z[p + "leaves"]
            assert (pos[1] >= 0).all(), p
            assert (pos[2] == -1).all() and (d2[2] == 0.0).all(), p
            many += int((leaves[:2] >= 2).sum())
            total += leaves[:2].size
    assert many >= 0.4 * total, (many, total)
    # ends: the cluster of 10 is one leaf (at sorted position 0 or n - 1), the cluster of 11 is not
    for name, (n_lo, n_hi) in ENDS:
        m = _model_of_reference(c, z, name, 0.5, 1)
        lv = leaves_of(m)
        pts = c[name][m.leaf]
        assert (pts[:n_lo] < -30.0).all() and (pts[-n_hi:] > 30.0).all()
        assert (lv[0][1] == 10) == (n_lo == 10) and (lv[-1][1] == 10) == (n_hi == 10), (name, lv[0], lv[-1])
        assert lv[0][1] < 11 and lv[-1][1] < 11
        m0 = _model_of_reference(c, z, name, 0.5, 0)
        assert m0.n_leaves > m.n_leaves
    # heavy: groups of more than 10 identical points are leaves of that many points at full depth, the group of 10 higher up
    m = _model_of_reference(c, z, "heavy", 0.125, 1)
    lv, pts = leaves_of(m), c["heavy"][m.leaf]
    full = max(d for _, _, d in lv)
    assert full == mo.depth_of(c["heavy"], 0.125)
    for cnt, p in HEAVY_GROUPS:
        mine = [(a, k, d) for a, k, d in lv if (pts[a:a + k] == p).all(1).any()]
        assert len(mine) == 1 and mine[0][1] == cnt and (pts[mine[0][0]:mine[0][0] + cnt] == p).all(), (cnt, mine)
        assert (mine[0][2] == full) == (cnt > 10), (cnt, mine, full)
    m = _model_of_reference(c, z, "eleven", 0.001, 1)
    assert len(m.nodes) == 11 and leaves_of(m) == [(0, 11, 10)]
    # planar: no extent in z
    assert (c["planar"][:, 2] == 2.0).all()
    for voxel, early in ((10.0, 1), (0.5, 0)):
        p = prefix("planar", voxel, early)
        assert (z[p + "pos"][1] >= 0).all() and (z[p + "pos"][0] == -1).any() and (z[p + "pos"][0] >= 0).any()
    # deep: 21 levels, every query finds a partner that is not within the stop, far from the leaf limit; most answers come
    # out of a leaf of depth 21
    assert mo.depth_of(c["deep"], DEEP_VOXEL) == 21
    for early in (0, 1):
        p = prefix("deep", DEEP_VOXEL, early)
        pos, d2, leaves = z[p + "pos"], z[p + "d2"], z[p + "leaves"]
        assert (pos >= 0).all() and (d2 > 1e-4).mean() >= 0.9 and leaves.max() < 10000, p
        assert leaves[1].max() > 1
        # (the depth of the answers' leaves: without earlystop every leaf lies at depth 21.  With it the 5000 scattered points,
        #  which all the queries sit next to, end in leaves of at most 10 points far above -- none of the answers comes from
        #  depth 21, so "at least half" cannot hold there; what that variant adds is the walk through early leaves at many depths
        #  on the way down a 21-level table, and the fraction is asserted to be what it is: none)
        m = _model_of_reference(c, z, "deep", DEEP_VOXEL, early)
        at21 = (leaf_depths(m)[pos] == 21).mean()
        assert at21 >= 0.5 if early == 0 else at21 == 0.0, (early, at21)
        assert leaf_depths(m).max() == 21


def compute():
    c, z = clouds(), {}
    q = queries(c)
    for name, variants in CASES:
        pts = c[name]
        qq, radii = q[name]
        if name in NOT_STORED:
            z[name + "_sha256"] = digest(pts)
        else:
            z[name], z[name + "_g"] = mo._pack(pts)
        try:
            z[name + "_q"], z[name + "_q_g"] = mo._pack(qq)
        except AssertionError:                               # full-mantissa doubles: stored as they are
            z[name + "_q"] = qq
        z[name + "_maxd2"] = np.array(radii)
        for voxel, early in variants:
            for k, v in case_rows(pts, voxel, early, qq, radii).items():
                z[prefix(name, voxel, early) + k] = v
    check_properties(c, q, z)
    return z


class Fixture(gold.Fixture):
    """the k20 reader over this file's layout: cloud, batches and get answer as there"""

    def __init__(self, z):
        self.z = z
        self._clouds = {}

    def cases(self):
        return [(name, voxel, early) for name, variants in CASES for voxel, early in variants]

    def cloud(self, name):
        if name not in self._clouds:
            if name in NOT_STORED:
                pts = clouds()[name]
                assert np.array_equal(digest(pts), self.z[name + "_sha256"]), name
            else:
                pts = mo._unpack(self.z[name], self.z[name + "_g"])
            self._clouds[name] = pts
        return self._clouds[name]

    def queries(self, name):
        k = name + "_q"
        return mo._unpack(self.z[k], self.z[k + "_g"]) if k + "_g" in self.z else self.z[k]

    def batches(self, name, voxel, early):
        """[(queries, maxdist2, pos, d2, leaves)]"""
        p, qq = prefix(name, voxel, early), self.queries(name)
        return [(qq, float(m), self.z[p + "pos"][b], self.z[p + "d2"][b], self.z[p + "leaves"][b])
                for b, m in enumerate(self.z[name + "_maxd2"])]


def load(path=OUT):
    return Fixture(dict(np.load(path)))


if __name__ == "__main__":
    if not have_ref():
        raise SystemExit("needs the reference checkout at %s (src/slam6d/Boctree.cc)" % gold.REF)
    z = compute()
    mo.save(z, OUT)
    size = os.path.getsize(OUT)
    print("wrote %s (%d arrays, %d bytes)" % (OUT, len(z), size))
    for k in sorted(z, key=lambda k: -z[k].nbytes)[:8]:
        print("  %-40s %s %s" % (k, z[k].dtype, z[k].shape))
    assert size <= MAX_BYTES, size
