"""Deterministic inputs of the line-search edge tests (tests/test_line_search_reference_host.py on the CPU,
tests/test_gpu_line_search_edges.py on the GPU): the search for the point nearest to a line, KDtree::FindClosestAlongDir
(kdTreeImpl.h:390-425), reached as tdtk_find_closest_along_dir (raw directions) and as pairing mode 1 of getPtPairs (the
normal is normalised and rotated into the tree frame first).  Nothing is stored: every cloud is seeded and regenerated, the
expected answers come from the oracle (oracle/oracle.c), which the host test pins to the reference's compiled tree.

A case is a dict: name, model [M][3], bucket, q [K][3], dirs [K][3] (directions, or normals for mode 1), maxdist2, rows (the
rows to compare: None = all), and for mode 1 also A (source_alignxf, 16 doubles) with q holding the data points in the
world frame.  `planted` lists the rows with a degenerate direction.

The clouds of the other edge suites are imported from tests/golden/make_golden_knn_edges.py, not restated."""
import importlib.util
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

SEARCH_BLOCK = 256          # kernels.hip: k_search<256, 8, ...>, search_grid() caps the grid at 16 workgroups per CU
SEARCH_WG_PER_CU = 16
SEARCH_SD = 8               # LDS levels of the line search's stack
DEFAULT_CUS = 256           # MI355X; the GPU test passes the count it reads from the device
TRIPS_EXTRA = 70_001
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049)
MAXDIST2_VALUES = (0.0, -1.0, 1e-300, np.inf, 1e300, np.nan)
NONUNIT_LENGTHS = (1e-3, 0.5, 2.0, 1e3)
DEGENERATE_SIZES = (1e-200, 1e-160, 1e160, 1e200)


def edges():
    spec = importlib.util.spec_from_file_location("make_golden_knn_edges",
                                                  os.path.join(_HERE, "golden", "make_golden_knn_edges.py"))
    me = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(me)
    return me


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def _case(name, model, bucket, q, dirs, maxdist2, rows=None, **more):
    q = np.ascontiguousarray(q, np.float64)
    dirs = np.ascontiguousarray(dirs, np.float64)
    assert q.shape == dirs.shape and q.shape[1] == 3
    c = dict(name=name, model=np.ascontiguousarray(model, np.float64), bucket=bucket, q=q, dirs=dirs,
             maxdist2=float(maxdist2), rows=rows)
    c.update(more)
    return c


def is_unit_finite(q, dirs):
    """rows with finite input whose direction has length 1 up to rounding"""
    with np.errstate(invalid="ignore", over="ignore"):
        n2 = (dirs * dirs).sum(1)
        return np.isfinite(q).all(1) & np.isfinite(dirs).all(1) & (np.abs(n2 - 1.0) < 1e-12)


def line_d(model, q, dirs, idx):
    """d of the returned points in the reference's association, Len2(p2p) - sqr(Dot(p2p, dir)) with p2p = q - point and
    both sums left to right (kdTreeImpl.h:397-400); rows with idx < 0 give NaN"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = q - model[np.maximum(idx, 0)]
        len2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        dot = (v[:, 0] * dirs[:, 0] + v[:, 1] * dirs[:, 1]) + v[:, 2] * dirs[:, 2]
        d = len2 - dot * dot
    return np.where(idx >= 0, d, np.nan)


def brute_min_d(model, q, dirs, chunk=256):
    """per row the smallest d over all model points, same association (rows with finite input only)"""
    out = np.empty(len(q))
    old = np.seterr(over="ignore", invalid="ignore")
    for s in range(0, len(q), chunk):
        v = q[s:s + chunk, None, :] - model[None, :, :]
        u = dirs[s:s + chunk, None, :]
        len2 = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]
        dot = (v[..., 0] * u[..., 0] + v[..., 1] * u[..., 1]) + v[..., 2] * u[..., 2]
        out[s:s + chunk] = (len2 - dot * dot).min(1)
    np.seterr(**old)
    return out


def tied_rows(model, q, dirs):
    """number of rows in which two or more model points are at the smallest d, exactly"""
    n = 0
    old = np.seterr(over="ignore", invalid="ignore")
    for s in range(0, len(q), 256):
        v = q[s:s + 256, None, :] - model[None, :, :]
        u = dirs[s:s + 256, None, :]
        len2 = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]
        dot = (v[..., 0] * u[..., 0] + v[..., 1] * u[..., 1]) + v[..., 2] * u[..., 2]
        d = len2 - dot * dot
        n += int(((d == d.min(1)[:, None]).sum(1) >= 2).sum())
    np.seterr(**old)
    return n


def equal(a, b):
    """exact, NaN equal to NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def align_matrix():
    """a source_alignxf that is neither the identity nor axis-aligned: rotations about x, y, z by 0.3, -0.5, 0.7 rad and a
    translation (column-major 4x4 as the reference stores it: p' = R p + t)"""
    cx, sx, cy, sy, cz, sz = np.cos(0.3), np.sin(0.3), np.cos(-0.5), np.sin(-0.5), np.cos(0.7), np.sin(0.7)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    R = Rz @ Ry @ Rx
    A = np.eye(4)
    A[:3, :3] = R.T
    A[3, :3] = [3.0, -2.0, 1.5]
    return A.reshape(16).copy(), R, A[3, :3].copy()


def to_world(R, t, p):
    return p @ R.T + t


def degenerate_directions():
    """the planted rows: zero, NaN / +inf / -inf in one component, the sizes whose squared length under- or overflows"""
    nan, inf = np.nan, np.inf
    rows = [[0.0, 0.0, 0.0], [nan, 0.6, 0.8], [0.6, nan, 0.8], [0.6, 0.8, nan], [inf, 0.6, 0.8], [0.6, -inf, 0.8],
            [0.6, 0.8, inf], [-inf, 0.0, 0.0]]
    for s in DEGENERATE_SIZES:
        rows += [[0.6 * s, -0.8 * s, 0.0], [s / 3.0, s / 3.0, -s / 3.0]]
    return np.array(rows)


def _plant(rng, dirs, special, fixed=()):
    """writes `special` over seeded rows of dirs (the rows in `fixed` first); returns the rows, in the order of special"""
    free = np.setdiff1d(np.arange(len(dirs)), np.array(fixed, np.int64))
    at = np.concatenate([np.array(fixed, np.int64), rng.choice(free, len(special) - len(fixed), replace=False)])
    dirs[at] = special
    return at


# ---- trips: more queries than 16 x CUs x 256 ------------------------------------------------------------------------
TRIPS_MAXDIST2 = 4.0e-3      # a line of length ~20 through 2.5 points per unit volume: about half the rows find a partner


def trips_count(cus):
    return SEARCH_WG_PER_CU * int(cus) * SEARCH_BLOCK + TRIPS_EXTRA


def trips(cus=DEFAULT_CUS, sample=20_000):
    """20,000 uniform points (spacing ~0.74), K = 16 CUs 256 + 70,001 queries: model points displaced by a few spacings,
    random unit directions, the degenerate directions planted (among them rows 0 and K - 1: the first slab and the clipped
    last one).  q holds the queries in the tree frame, data the same points in the world frame of A (mode 1)."""
    rng = np.random.default_rng(7101)
    model = rng.uniform(-10, 10, (20_000, 3))
    K = trips_count(cus)
    q = model[rng.integers(0, len(model), K)] + rng.normal(0, 1.5, (K, 3))
    dirs = _unit(rng, K)
    planted = _plant(rng, dirs, degenerate_directions(), fixed=(0, K - 1))
    q[planted] = model[rng.integers(0, len(model), len(planted))]      # (on a model point: see normals_mode1)
    rows = np.union1d(rng.choice(K, sample, replace=False), planted)
    A, R, t = align_matrix()
    return _case("trips", model, 20, q, dirs, TRIPS_MAXDIST2, rows, planted=planted, A=A, data=to_world(R, t, q),
                 shuffle=rng.permutation(K))


# ---- deep: every lane stacks the whole root-to-leaf path of an 80-level tree ---------------------------------------------
DEEP_MAXDIST2 = 1.0


def deep(have_ref, bucket):
    """the 80-level cloud; a third of the queries lies in the geometric part.  Directions by thirds: along the comb (the
    radial direction, the line runs through the dense core), across it (perpendicular to the radius), random"""
    me = edges()
    pts, geo = me.deep_cloud()
    n = 2_400 if have_ref else me.DEEP_FALLBACK_Q
    q = me.deep_queries(pts, geo, n, 7200 + bucket)
    rng = np.random.default_rng(7201 + bucket)
    rad = q / np.linalg.norm(q, axis=1)[:, None]
    rnd = _unit(rng, n)
    acr = np.cross(rad, rnd)
    acr /= np.linalg.norm(acr, axis=1)[:, None]
    kind = np.arange(n) % 3
    dirs = np.where((kind == 0)[:, None], rad, np.where((kind == 1)[:, None], acr, rnd))
    return _case("deep_b%d" % bucket, pts, bucket, q, dirs, DEEP_MAXDIST2, geo=geo)


# ---- table: leaf table mode, a leaf of 40,000 copies ---------------------------------------------------------------------
TABLE_MAXDIST2 = 1.0e-4


def table():
    """600 queries: 100 lines pass 0.005 from the copied point (all 40,000 copies are at the same d: the first in walk order
    wins), 100 pass 0.03 from it (they miss the copies; the blob, 0.02 away, may be hit), 100 run through the blob, 300 are
    ordinary.  through / beside: the first two groups."""
    me = edges()
    pts, copies, blob = me.table_cloud()
    rng = np.random.default_rng(7301)
    u = _unit(rng, 600)
    perp = np.cross(u, _unit(rng, 600))
    perp /= np.linalg.norm(perp, axis=1)[:, None]
    t = rng.uniform(-5, 5, (600, 1))
    q = np.empty((600, 3))
    q[:100] = me.TABLE_COPY + t[:100] * u[:100] + 0.005 * perp[:100]
    q[100:200] = me.TABLE_COPY + t[100:200] * u[100:200] + 0.03 * perp[100:200]
    q[200:300] = pts[rng.choice(blob, 100, replace=False)] + t[200:300] * u[200:300]
    q[300:] = rng.uniform(-11, 11, (300, 3))
    perm = rng.permutation(600)
    inv = np.argsort(perm)
    return _case("table", pts, 20, q[perm], u[perm], TABLE_MAXDIST2, copies=copies, through=np.sort(inv[:100]),
                 beside=np.sort(inv[100:200]))


# ---- on_the_line: d rounds to zero or below, the pruning switches off ---------------------------------------------------------
def uniform_cloud():
    return np.random.default_rng(7001).uniform(-10, 10, (30_000, 3))


def lattice12():
    a = np.arange(12.0)
    return np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)


def on_the_line(which):
    """q = m_i + t u for model points m_i, unit u and |t| log-uniform in 1e-3 .. 1e3: m_i lies on the line up to rounding.
    On the lattice a third of the directions is axis-aligned (d of m_i is exactly 0, and so is that of its whole row)."""
    rng = np.random.default_rng(7401 + (which == "lattice"))
    model = uniform_cloud() if which == "uniform" else lattice12()
    n = 3_000 if which == "uniform" else 1_500
    m = model[rng.integers(0, len(model), n)]
    u = _unit(rng, n)
    if which == "lattice":
        ax = np.eye(3)[rng.integers(0, 3, n)] * rng.choice([-1.0, 1.0], n)[:, None]
        u = np.where((np.arange(n) % 3 == 0)[:, None], ax, u)
    t = 10.0 ** rng.uniform(-3, 3, (n, 1)) * rng.choice([-1.0, 1.0], (n, 1))
    return _case("on_the_line_" + which, model, 20 if which == "uniform" else 5, m + t * u, u, 0.01)


# ---- directions: as given -------------------------------------------------------------------------------------------------
def directions(which):
    """uniform: non-unit lengths, the zero vector and NaN / +-inf components among ordinary rows.  lattice: axis-aligned
    unit vectors from lattice points and half-integers (many points at the same d, the first in walk order wins)."""
    rng = np.random.default_rng(7501 + (which == "lattice"))
    if which == "lattice":
        model = lattice12()
        n = 1_200
        q = rng.integers(-3, 27, (n, 3)) / 2.0
        u = np.eye(3)[rng.integers(0, 3, n)] * rng.choice([-1.0, 1.0], n)[:, None]
        u[::7] = _unit(rng, len(u[::7]))
        return _case("directions_lattice", model, 5, q, u, 4.0, axis=np.setdiff1d(np.arange(n), np.arange(0, n, 7)))
    model = uniform_cloud()
    n = 1_600
    q = model[rng.integers(0, len(model), n)] + rng.normal(0, 1.0, (n, 3))
    u = _unit(rng, n)
    special = [u[i] * s for i, s in enumerate(np.tile(NONUNIT_LENGTHS, 100))]
    special += [r for r in degenerate_directions()[:8]] * 4
    planted = _plant(rng, u, np.array(special))
    return _case("directions_uniform", model, 20, q, u, 0.05, planted=planted)


# ---- nonfinite_q ----------------------------------------------------------------------------------------------------------
def nonfinite_q():
    me = edges()
    pts, Q, i_ord, i_nan, i_far = me.nonfinite_cloud()
    rng = np.random.default_rng(7601)
    return _case("nonfinite_q", pts, 20, Q, _unit(rng, len(Q)), 9.0, ordinary=i_ord, nan=i_nan, far=i_far)


# ---- maxdist2 -------------------------------------------------------------------------------------------------------------
def maxdist2_cases():
    """64 queries on 5,000 points, one case per value (+inf and 1e300 enter every node of the tree for every query)"""
    rng = np.random.default_rng(7701)
    model = rng.uniform(-5, 5, (5_000, 3))
    q = np.vstack([model[rng.integers(0, len(model), 32)] + rng.normal(0, 0.3, (32, 3)), rng.uniform(-6, 6, (32, 3))])
    u = _unit(rng, 64)
    q[:8] = model[:8] + 2.0 * u[:8]          # the model point is on the line: d of about 0 against a maxdist2 of 0, < 0, 1e-300
    return [_case("maxdist2_%r" % v, model, 20, q, u, v) for v in MAXDIST2_VALUES]


# ---- sizes ----------------------------------------------------------------------------------------------------------------
def sizes():
    """one query set on the 30,000-point cloud; every K of SIZES is a prefix of it"""
    rng = np.random.default_rng(7801)
    model = uniform_cloud()
    n = max(SIZES)
    q = model[rng.integers(0, len(model), n)] + rng.normal(0, 1.0, (n, 3))
    return _case("sizes", model, 20, q, _unit(rng, n), 0.05)


# ---- normals_mode1 --------------------------------------------------------------------------------------------------------
MODE1_MAXDIST2 = 2.0e-3


def normals_mode1():
    """getPtPairs(pairing_mode=1): 60,000 model points, 40,000 data points in the world frame of a non-trivial
    source_alignxf, random normals of random lengths, the degenerate ones planted"""
    rng = np.random.default_rng(7901)
    model = rng.uniform(-10, 10, (60_000, 3))
    A, R, t = align_matrix()
    n = 40_000
    local = model[rng.integers(0, len(model), n)] + rng.normal(0, 1.0, (n, 3))
    nr = _unit(rng, n) * 10.0 ** rng.uniform(-2, 2, (n, 1))
    planted = _plant(rng, nr, degenerate_directions(), fixed=(0, n - 1))
    # the planted rows sit on a model point (up to the rounding of A and its inverse): a normal whose length overflows
    # becomes u = 0, the search a closest-point search, and the row pairs; 0 / 0 and x / 0 give NaN and +-inf, and no pair
    local[planted] = model[rng.integers(0, len(model), len(planted))]
    return _case("normals_mode1", model, 20, to_world(R, t, local), nr, MODE1_MAXDIST2, A=A, planted=planted)


def normals_mode1_lattice():
    """mode 1 where the visiting order decides: the 12^3 lattice, data points on integers and half-integers, axis-aligned
    normals whose lengths are powers of two, and a source_alignxf of a quarter turn about z with an integer translation --
    the inverse, the rotated point and the normalised, rotated normal are all exact, so whole rows of lattice points are at
    the same d and the first in walk order wins"""
    rng = np.random.default_rng(7951)
    model = lattice12()
    n = 1_500
    local = rng.integers(-3, 27, (n, 3)) / 2.0
    nr = np.eye(3)[rng.integers(0, 3, n)] * rng.choice([-1.0, 1.0], n)[:, None] * 2.0 ** rng.integers(-8, 9, (n, 1))
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    t = np.array([3.0, -2.0, 1.0])
    A = np.eye(4)
    A[:3, :3] = R.T
    A[3, :3] = t
    return _case("normals_mode1_lattice", model, 5, to_world(R, t, local), nr, 4.0, A=A.reshape(16).copy(), local=local,
                 planted=np.zeros(0, np.int64))


MODE1_NAMES = ("normals_mode1", "normals_mode1_lattice")


def mode1_case(name):
    return {"normals_mode1": normals_mode1, "normals_mode1_lattice": normals_mode1_lattice}[name]()


FIND_CLOSEST_NAMES =(["trips", "deep_b1", "deep_b20", "table", "on_the_line_uniform", "on_the_line_lattice",
                       "directions_uniform", "directions_lattice", "nonfinite_q"]
                      + ["maxdist2_%r" % v for v in MAXDIST2_VALUES] + ["sizes"])


def find_closest_case(name, have_ref, cus=DEFAULT_CUS):
    """the FindClosestAlongDir case of that name (FIND_CLOSEST_NAMES)"""
    if name == "trips":
        return trips(cus)
    if name.startswith("deep_b"):
        return deep(have_ref, int(name[6:]))
    if name.startswith("on_the_line_"):
        return on_the_line(name[12:])
    if name.startswith("directions_"):
        return directions(name[11:])
    if name.startswith("maxdist2_"):
        return maxdist2_cases()[["maxdist2_%r" % v for v in MAXDIST2_VALUES].index(name)]
    return {"table": table, "nonfinite_q": nonfinite_q, "sizes": sizes}[name]()


def compared(c):
    """(q, dirs) of the rows the case compares"""
    return (c["q"], c["dirs"]) if c["rows"] is None else (c["q"][c["rows"]], c["dirs"][c["rows"]])


def shares(idx):
    """(share of rows with a partner, share without)"""
    hit = float((np.asarray(idx) >= 0).mean())
    return hit, 1.0 - hit
