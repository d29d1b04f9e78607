"""Inputs of the graph back-end reference tests (lum6DEuler -G 1, lum6DQuat -G 2, ghelix6DQ2 -G 3, gapx6D -G 4): link cases
and small graphs, generated from seeds, so that k16_graph_backends.npz stores results and not clouds.  Imported by the
fixture generator (tests/golden/make_golden_graph_backends.py) and by both test tiers.

A link case is (model, data, max_dist_match): two scans with the identity pose, so that p1 of a pair is a model point as
it stands and the pair list is fully determined by the nearest-neighbour search (no ties: random doubles, or distance 0
to exactly one point).  A graph is a list of scans (local points, initial pose) and a link list.  Scans have 3 000 points
or fewer."""
import numpy as np

BACKENDS = (1, 2, 3, 4)
NAMES = {1: "lum6DEuler", 2: "lum6DQuat", 3: "ghelix6DQ2", 4: "gapx6D"}
MIN_PAIRS = {1: 3, 2: 3, 3: 2, 4: 2}       # `m > 2` (lum6Deuler.cc:141, lum6Dquat.cc:129), `size() <= 1` skipped (ghelix6DQ2.cc:382, gapx6D.cc:434)
N_LINK = 2000
FAR = 1.0e6
AWAY = 1000.0                               # data points moved by this pair with nothing at max_dist_match 0.5

# the small rigid offset between model and data of every noisy link: with it sum |p1 - p2|^2 is about m |offset|^2 whatever the
# noise, which is what makes the normal-equation form of lum6DQuat's ss a difference of nearly equal numbers
_OFF_T = np.array([0.03, -0.02, 0.01])
_OFF_A = (0.001, -0.002, 0.0015)


def _rot(angles):
    a, b, c = angles
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


LINK_CASES = ("pairs0", "pairs1", "pairs2", "pairs3", "noise1", "noise1e-3", "noise1e-6", "aligned", "symmetric", "plane",
              "far_pairs3", "far_noise1", "far_noise1e-3", "far_noise1e-6", "far_aligned")


def link_case(name):
    """-> (model [n][3], data [n][3], max_dist_match)"""
    far = name.startswith("far_")
    base = name[4:] if far else name
    rng = np.random.default_rng(16)
    model = rng.uniform(-10.0, 10.0, (N_LINK, 3))
    moved = model @ _rot(_OFF_A).T + _OFF_T
    maxd = 0.5
    if base.startswith("pairs"):
        k = int(base[5:])
        data = moved + rng.normal(0.0, 1e-3, model.shape)
        data[k:] += AWAY
    elif base.startswith("noise"):
        sigma = float(base[5:])
        data = moved + rng.normal(0.0, sigma, model.shape)
        maxd = 5.0 if sigma == 1.0 else 0.5
    elif base == "aligned":
        data = model.copy()
    elif base == "symmetric":
        half = model[:N_LINK // 2]
        e = rng.normal(0.0, 1e-3, half.shape)
        model = np.concatenate([half, -half])
        data = np.concatenate([half + e, -(half + e)])
    elif base == "plane":
        model[:, 2] = rng.normal(0.0, 0.01, N_LINK)
        data = model @ _rot(_OFF_A).T + _OFF_T + rng.normal(0.0, 1e-3, model.shape)
    else:
        raise ValueError(name)
    if far:
        model = model + FAR
        data = data + FAR
    return np.ascontiguousarray(model), np.ascontiguousarray(data), maxd


def link_pairs_expected(name):
    """the pair count the case is there for (None: whatever the search finds, about N_LINK)"""
    base = name[4:] if name.startswith("far_") else name
    return int(base[5:]) if base.startswith("pairs") else None


# ---- graphs -----------------------------------------------------------------------------------------------------------
GRAPHS = ("chain_closure", "both_directions", "star", "few_pairs", "tiny_symmetric", "weak_symmetric")
N_WEAK = 120
# the graphs whose assembled matrix has nonzero entries under the drop rule's 1e-5, and for which back-ends
DROP_GRAPHS = {"tiny_symmetric": (1, 2, 3, 4), "weak_symmetric": (1, 2)}
N_WORLD = 1500


class Graph:
    def __init__(self, name, points, rPos, rPosTheta, links, maxd, links34=None):
        self.name = name
        self.points = points                # per scan: local points [n][3]
        self.rPos = np.array(rPos, float)   # [nscans][3] initial pose estimates
        self.rPosTheta = np.array(rPosTheta, float)
        self._links = {b: (links34 if (links34 is not None and b >= 3) else links) for b in BACKENDS}
        self.maxd = maxd

    def links(self, backend):
        return list(self._links[backend])

    @property
    def nscans(self):
        return len(self.points)


def _pose_R(th):
    """the rotation of the pose (rPos, rPosTheta = th) as EulerToMatrix4 defines it, p' = R p + rPos (inputs only)"""
    sx, cx, sy, cy, sz, cz = np.sin(th[0]), np.cos(th[0]), np.sin(th[1]), np.cos(th[1]), np.sin(th[2]), np.cos(th[2])
    return np.array([[cy * cz, -cy * sz, sy],
                     [sx * sy * cz + cx * sz, -sx * sy * sz + cx * cz, -sx * cy],
                     [-cx * sy * cz + sx * sz, cx * sy * sz + sx * cz, cx * cy]])


def _local(world, t, th):
    """the world points as a scan at pose (t, th) sees them: R^T (w - t)"""
    return (world - t) @ _pose_R(th)


def graph(name):
    rng = np.random.default_rng(1600 + GRAPHS.index(name))
    scale = 1.0
    ns = {"chain_closure": 4, "both_directions": 4, "star": 5, "few_pairs": 5, "tiny_symmetric": 4, "weak_symmetric": 4}[name]
    world = rng.uniform(-1.0, 1.0, (N_WORLD, 3)) * np.array([10.0, 10.0, 3.0])
    sigma = 0.01
    if name == "tiny_symmetric":
        # coordinates of about 8e-4: the diagonal second moments of ghelix6DQ2 and gapx6D stay above the 1e-5 of the drop rule,
        # the mixed ones fall below it; symmetric about the origin, poses pure rotations about it, noise mirrored: the first
        # moments of every link are rounding-sized, which gives the lum back-ends their small nonzero entries
        scale = 8.0e-5
        sigma = 0.05
        half = world[:N_WORLD // 2]
        world = np.concatenate([half, -half])
    symmetric = name in ("tiny_symmetric", "weak_symmetric")
    if name == "weak_symmetric":
        # the lum back-ends divide their blocks by ss, so at tiny_symmetric's scale their entries are huge and what falls under
        # the drop rule's 1e-5 is rounding.  Here the blocks are small instead: 120 points, noise of 2 on a cloud of 10 (ss of
        # about 10), and the cloud is moved off its centre of symmetry by 3e-8, so that the first moments over ss -- the
        # entries that couple translation and rotation -- are honest numbers of about 5e-6.  Dropping them moves X.
        sigma = 2.0
        half = world[:N_WEAK // 2]
        world = np.concatenate([half, -half]) + 3.0e-8
    true_t = rng.uniform(-0.5, 0.5, (ns, 3))
    true_a = rng.uniform(-0.05, 0.05, (ns, 3))
    est_t = true_t + rng.normal(0.0, 0.02, (ns, 3))
    est_a = true_a + rng.normal(0.0, 0.002, (ns, 3))
    if symmetric:
        true_t[:] = 0.0
        est_t[:] = 0.0
    pts = []
    for i in range(ns):
        if symmetric:
            e = rng.normal(0.0, sigma, (len(world) // 2, 3))
            noise = np.concatenate([e, -e])
        else:
            noise = rng.normal(0.0, sigma, world.shape)
        pts.append(_local(world + noise, true_t[i], true_a[i]) * scale)
    maxd = 8.0 if name == "weak_symmetric" else 1.0 * scale
    links34 = None
    if name == "chain_closure":
        links = [(0, 1), (1, 2), (2, 3), (0, 3)]
    elif name == "both_directions":
        links = [(0, 1), (1, 2), (1, 2), (2, 1), (2, 3)]
    elif name == "star":
        links = [(0, 1), (0, 2), (0, 3), (0, 4)]
    elif name == "few_pairs":
        # scan 4 sees a region of its own, which only scan 3 shares, and two points q1, q2 of the world; scan 2 has no point
        # within 2 of q2.  (1, 4) has 2 pairs: under the lum back-ends' threshold; (2, 4) has 1: under the other two's.
        region = rng.uniform(-1.0, 1.0, (N_WORLD, 3)) * np.array([10.0, 10.0, 3.0]) + np.array([25.0, 0.0, 0.0])
        q = world[:2]
        d2 = ((world - q[1]) ** 2).sum(1)
        keep2 = d2 > 4.0
        pts[2] = _local(world[keep2] + rng.normal(0.0, sigma, (int(keep2.sum()), 3)), true_t[2], true_a[2])
        pts[3] = _local(np.concatenate([world, region]) + rng.normal(0.0, sigma, (2 * N_WORLD, 3)), true_t[3], true_a[3])
        pts[4] = _local(np.concatenate([q, region]) + rng.normal(0.0, sigma, (2 + N_WORLD, 3)), true_t[4], true_a[4])
        links = [(0, 1), (1, 2), (2, 3), (3, 4), (1, 4)]
        links34 = [(0, 1), (1, 2), (2, 3), (3, 4), (1, 4), (2, 4)]
    else:
        links = [(0, 1), (1, 2), (2, 3), (0, 3), (1, 3)]
    # the initial pose estimates (rPos, rPosTheta): the true poses, perturbed
    g = Graph(name, [np.ascontiguousarray(p) for p in pts], est_t * scale, est_a, links, maxd, links34)
    g.scale = scale
    assert all(len(p) <= 3000 for p in g.points)
    return g
