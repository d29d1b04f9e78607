"""Generator of k11_adaptive_normals.npz: calculateNormalsAdaptiveKNN / calculateNormalsAdaptiveApxKNN (normals.cc:563-682,
116-213) on sampled points of the k8 clouds and of the deep cloud, assembled from the reference's own compiled pieces.

    python tests/golden/make_golden_adaptive.py     (needs oracle/_ref: a build() where the reference checkout exists)

normals.cc itself does not compile in this image (normals.h -> scan.h -> Boost), so the status is the one of ApxKNN: the
glue is restated, the pieces are real.  Per point and per kidx = kmin .. kmax (reference_loop):
  lists        KDtreeIndexed::kNearestNeighbors(p, kidx + 1) of oracle/_ref/libref3dtk.so (exact form), or annkSearch of the
               vendored ANN library through orc.AnnTree(pts, "ref").ksearch(p, kidx + 1, eps) (ANN form): a fresh search each
  covariance   in numpy, in the summation order of the reference and of the device: the mean summed in list order and
               divided by nr, then A[r][c] += ((1 / nr) * x[c]) * x[r] in list order (list_cov)
  eigenvalues  newmat's EigenValues through orc.eigen3(A, which="ref")
  the rule     (e1 > 0.25 * e2) && (fabs(1.0 - e2 / e3) < 0.25), stop at the first kidx that passes, else kmax
  the normal   orc.normals_from_knn on the chosen list; the generator asserts that its own covariance + that eigen3's first
               eigenvector, oriented and normalised, is the same vector bit for bit, so the two statements cannot drift apart

The fixture holds, per cloud, the sampled row indices and per case normals[rows] and k_used[rows]; no lists (the GPU test
checks those against the library's own fixed-k search).  Also imported by the tests."""
import importlib.util
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
OUT = os.path.join(_HERE, "k11_adaptive_normals.npz")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


mgk = _load("make_golden_knn")
mge = _load("make_golden_knn_edges")
RPOS, k8_clouds, deep_cloud = mgk.RPOS, mgk.k8_clouds, mge.deep_cloud

BUCKETS = (1, 20)
EXACT_CONFIGS = ((0, 3), (9, 9), (3, 12), (5, 20), (8, 30), (30, 40))     # (30, 40): the LDS-list kernel, k on both sides of 32
ANN_CONFIGS = ((9, 9), (3, 12), (5, 20), (8, 31))
ANN_EPS = (0.0, 1.0)
ANN_SKIP = ("seven", "one")          # kmax + 1 > n: error cases
ROWS = 60
DEEP_ROWS = 40
DEEP_CONFIG = (5, 20)


def sample_rows(name, n, rows=ROWS):
    """a seeded sample of point indices of the cloud (all of them where it has fewer), ascending"""
    if n <= rows:
        return np.arange(n)
    rng = np.random.default_rng([1100, sum(name.encode())])
    return np.sort(rng.choice(n, rows, replace=False))


DEEP_GEO_MAX = 1e60


def deep_rows(pts, geo):
    """half of the deep cloud's sample from its geometric part (the spine of the 80-level tree), half from the uniform part
    (the deepest leaves).  Of the geometric part only points with |p| < 1e60: a covariance entry is about |p|^2 / 100 and
    tred2 squares it, so beyond 1e78 newmat overflows, never converges and throws (the reference ends there; the device
    gives up after newmat's 30 sweeps and returns NaNs)"""
    rng = np.random.default_rng(1101)
    near = geo[np.abs(pts[geo]).max(1) < DEEP_GEO_MAX]
    return np.sort(np.concatenate([rng.choice(near, DEEP_ROWS // 2, replace=False),
                                   rng.choice(np.setdiff1d(np.arange(len(pts)), geo), DEEP_ROWS // 2, replace=False)]))


def list_cov(P):
    """mean and covariance of the list's points P [nr][3] in the device's summation order (np.cumsum adds left to right)"""
    nr = len(P)
    mean = np.cumsum(P, axis=0)[-1] / nr
    X = P - mean
    sc = 1.0 / nr
    A = np.zeros((3, 3))
    for r in range(3):
        for c in range(r + 1):
            A[r, c] = A[c, r] = np.cumsum((sc * X[:, c]) * X[:, r])[-1]
    return A


def accepts(d):
    """the stopping rule, d ascending, in the reference's sense (e3 == 0: NaN or inf, false)"""
    e1, e2, e3 = (np.float64(v) for v in d)
    with np.errstate(divide="ignore", invalid="ignore"):
        return bool((e1 > 0.25 * e2) and (np.abs(1.0 - e2 / e3) < 0.25))


def orient(u0, p, rpos=RPOS):
    """the tail of calculateNormal: column 0 of U flipped towards n . (p - rPos) >= 0, v * (1 / norm)"""
    n = np.array(u0, np.float64)
    pv = p - rpos
    with np.errstate(divide="ignore", invalid="ignore"):
        pv = pv * (1.0 / np.sqrt((pv[0] * pv[0] + pv[1] * pv[1]) + pv[2] * pv[2]))
        if (n[0] * pv[0] + n[1] * pv[1]) + n[2] * pv[2] < 0:
            n = n * -1.0
        return n * (1.0 / np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]))


def adaptive_point(orc, pts, p, lists, kmin, kmax, which, rpos=RPOS):
    """one point of the loop: lists(p, k) -> the point indices of a fresh k-search.  Returns (k_used, chosen list, U)"""
    for kidx in range(kmin, kmax + 1):
        l = np.asarray(lists(p, kidx + 1))
        d, U = orc.eigen3(list_cov(pts[l]), which=which)
        if accepts(d):
            break
    return kidx, l, U


def reference_loop(orc, pts, rows, lists, kmin, kmax, which="ref", rpos=RPOS):
    """-> (normals [len(rows)][3], k_used [len(rows)] int32).  which: whose eigen3 ("ref": newmat itself)"""
    nrm = np.empty((len(rows), 3))
    ku = np.empty(len(rows), np.int32)
    for j, i in enumerate(rows):
        p = pts[i]
        ku[j], l, U = adaptive_point(orc, pts, p, lists, kmin, kmax, which, rpos)
        nrm[j] = mgk._pca(orc, p, pts[l], rpos)
        mine = orient(U[:, 0], p, rpos)
        assert np.array_equal(mine, nrm[j], equal_nan=True), (i, kmin, kmax, mine, nrm[j])
    return nrm, ku


def exact_lists(tree):
    return lambda p, k: tree.knn(p, k)


def ann_lists(ann, eps):
    return lambda p, k: ann.ksearch(p, k, eps)[0][0]


def exact_key(name, b, cfg):
    return "%s_b%d_k%d_%d" % (name, b, cfg[0], cfg[1])


def ann_key(name, cfg, eps):
    return "%s_ann_k%d_%d_e%d" % (name, cfg[0], cfg[1], int(eps))


def compute(orc):
    z = {}
    for name, (pts, _, _, _) in k8_clouds().items():
        rows = sample_rows(name, len(pts))
        z[name + "_rows"] = rows.astype(np.int32)
        for b in BUCKETS:
            t = mgk.RefTree(pts, b)
            for cfg in EXACT_CONFIGS:
                z[exact_key(name, b, cfg) + "_n"], z[exact_key(name, b, cfg) + "_k"] = reference_loop(orc, pts, rows, exact_lists(t), *cfg)
        if name in ANN_SKIP:
            continue
        ann = orc.AnnTree(pts, "ref")
        for cfg in ANN_CONFIGS:
            for eps in ANN_EPS:
                z[ann_key(name, cfg, eps) + "_n"], z[ann_key(name, cfg, eps) + "_k"] = reference_loop(orc, pts, rows, ann_lists(ann, eps), *cfg)
    pts, geo = deep_cloud()
    rows = deep_rows(pts, geo)
    z["deep_rows"] = rows.astype(np.int32)
    t = mgk.RefTree(pts, 1)
    z[exact_key("deep", 1, DEEP_CONFIG) + "_n"], z[exact_key("deep", 1, DEEP_CONFIG) + "_k"] = reference_loop(orc, pts, rows, exact_lists(t), *DEEP_CONFIG)
    ann = orc.AnnTree(pts, "ref")
    for eps in ANN_EPS:
        z[ann_key("deep", DEEP_CONFIG, eps) + "_n"], z[ann_key("deep", DEEP_CONFIG, eps) + "_k"] = reference_loop(orc, pts, rows, ann_lists(ann, eps), *DEEP_CONFIG)
    return z


if __name__ == "__main__":
    sys.path.insert(0, _ROOT)
    from oracle import orc
    if not orc.have_ref():
        raise SystemExit("needs oracle/_ref/libref3dtk.so (build() where the reference checkout exists)")
    z = compute(orc)
    np.savez_compressed(OUT, **z)
    print("wrote %s (%d arrays, %d bytes)" % (OUT, len(z), os.path.getsize(OUT)))
