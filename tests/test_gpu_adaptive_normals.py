"""The adaptive-k normal estimators on the device (calculateNormalsAdaptiveKNN / calculateNormalsAdaptiveApxKNN): against the
fixture k11_adaptive_normals.npz (the reference's loop), against the library's own fixed-k searches and the oracle's PCA on
every row, against the fixed-k estimators where kmin == kmax, on more queries than one grid holds, on the 80-level tree,
and the error cases."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def _load():
    spec = importlib.util.spec_from_file_location("make_golden_adaptive", os.path.join(G, "make_golden_adaptive.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


ma = _load()
RPOS = ma.RPOS
CLOUDS = ma.k8_clouds()
_memo = {}


def fixture():
    if "z" not in _memo:
        _memo["z"] = np.load(os.path.join(G, "k11_adaptive_normals.npz"))
    return _memo["z"]


def deep():
    if "deep" not in _memo:
        _memo["deep"] = ma.deep_cloud()
    return _memo["deep"]


def big_cloud():
    """300,000 uniform points: more than Q_MAX_BLOCKS x Q_BLOCK = 262,144 lanes and more than 1024 x 256 ANN threads"""
    if "big" not in _memo:
        _memo["big"] = np.random.default_rng(1104).uniform(-40, 40, (300_000, 3))
    return _memo["big"]


# ---- 1. fixture parity -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CLOUDS))
def test_exact_equals_the_reference_loop(tdtk, gpu, name):
    z, pts = fixture(), CLOUDS[name][0]
    rows = z[name + "_rows"]
    for b in ma.BUCKETS:
        for cfg in ma.EXACT_CONFIGS:
            nrm, ku = tdtk.calculateNormalsAdaptiveKNN(pts, cfg[0], cfg[1], RPOS, b, want_k=True)
            key = ma.exact_key(name, b, cfg)
            assert np.array_equal(ku[rows], z[key + "_k"]), key
            assert np.array_equal(nrm[rows], z[key + "_n"], equal_nan=True), key


@pytest.mark.parametrize("name", [n for n in CLOUDS if n not in ma.ANN_SKIP])
def test_ann_equals_the_reference_loop(tdtk, gpu, name):
    z, pts = fixture(), CLOUDS[name][0]
    rows = z[name + "_rows"]
    for cfg in ma.ANN_CONFIGS:
        for eps in ma.ANN_EPS:
            nrm, ku = tdtk.calculateNormalsAdaptiveApxKNN(pts, cfg[0], cfg[1], RPOS, eps, want_k=True)
            key = ma.ann_key(name, cfg, eps)
            assert np.array_equal(ku[rows], z[key + "_k"]), key
            assert np.array_equal(nrm[rows], z[key + "_n"], equal_nan=True), key


# ---- 2. lists and rule, without the fixture ----------------------------------------------------------------------------
def _pca_rows(orc, Q, pts, lists):
    """the oracle's calculateNormal for queries Q with their lists [m][nr] (indices into pts)"""
    m, nr = lists.shape
    xyz = np.vstack([Q, pts[lists.ravel()]])
    knn = np.zeros((len(xyz), nr), np.int32)
    knn[:m] = m + np.arange(m * nr, dtype=np.int32).reshape(m, nr)
    return orc.normals_from_knn(xyz, knn, RPOS)[:m]


def check_rows(orc, pts, rows, kmin, kmax, nrm, ku, knn, lists_batch, tag, rule_rows=50):
    """rows of the three outputs against lists_batch(Q, k) -> [len(Q)][k] (-1 beyond the cloud): the list is the k_used + 1
    search's, the normal is the oracle's PCA on it, and -- on rule_rows sampled rows -- the stopping rule recomputed with the
    oracle's eigenvalues is false for every kidx < k_used and true at k_used unless k_used == kmax"""
    rows = np.asarray(rows)
    assert knn.shape == (len(pts), kmax + 1) and ku.shape == (len(pts),) and nrm.shape == (len(pts), 3), tag
    assert (ku[rows] >= kmin).all() and (ku[rows] <= kmax).all(), tag
    for k in np.unique(ku[rows]):
        sel = rows[ku[rows] == k]
        L = lists_batch(pts[sel], int(k) + 1)
        want = -np.ones((len(sel), kmax + 1), np.int32)
        want[:, :k + 1] = L
        assert np.array_equal(knn[sel], want), (tag, int(k))
        nr = min(int(k) + 1, len(pts))
        assert (L[:, :nr] >= 0).all() and (L[:, nr:] == -1).all(), (tag, int(k))
        assert np.array_equal(nrm[sel], _pca_rows(orc, pts[sel], pts, L[:, :nr]), equal_nan=True), (tag, int(k))
    sample = rows if len(rows) <= rule_rows else np.sort(np.random.default_rng(1102).choice(rows, rule_rows, replace=False))
    for kidx in range(kmin, kmax + 1):
        act = sample[ku[sample] >= kidx]
        if not len(act):
            break
        L = lists_batch(pts[act], kidx + 1)
        for i, l in zip(act, L):
            d, _ = orc.eigen3(ma.list_cov(pts[l[l >= 0]]))
            if kidx < ku[i]:
                assert not ma.accepts(d), (tag, int(i), kidx)
            elif ku[i] < kmax:
                assert ma.accepts(d), (tag, int(i), kidx)


@pytest.mark.parametrize("name", ["uniform", "duplicates", "lattice", "seven"])
def test_exact_lists_normals_and_rule_on_every_row(tdtk, orc, gpu, name):
    pts = CLOUDS[name][0]
    for b in (1, 20):
        kd = tdtk.KDtree(pts, b)
        for cfg in ((3, 12), (30, 40)):
            nrm, ku, knn = tdtk.calculateNormalsAdaptiveKNN(pts, cfg[0], cfg[1], RPOS, b, want_k=True, want_knn=True)
            check_rows(orc, pts, np.arange(len(pts)), cfg[0], cfg[1], nrm, ku, knn,
                       lambda Q, k: kd.kNearestNeighborsBatch(Q, k)[0], (name, b, cfg))


@pytest.mark.parametrize("name", ["uniform", "duplicates", "lattice"])
def test_ann_lists_normals_and_rule_on_every_row(tdtk, orc, gpu, name):
    pts = CLOUDS[name][0]
    ann = orc.AnnTree(pts)
    for cfg in ((3, 12), (8, 31)):
        for eps in ma.ANN_EPS:
            nrm, ku, knn = tdtk.calculateNormalsAdaptiveApxKNN(pts, cfg[0], cfg[1], RPOS, eps, want_k=True, want_knn=True)
            check_rows(orc, pts, np.arange(len(pts)), cfg[0], cfg[1], nrm, ku, knn,
                       lambda Q, k: ann.ksearch(Q, k, eps)[0], (name, cfg, eps))


# ---- 3. kmin == kmax is the fixed-k estimator ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["uniform", "one"])
def test_exact_with_one_k_is_the_fixed_k_estimator(tdtk, gpu, name):
    pts = CLOUDS[name][0]
    for k in (1, 10, 21, 32, 33, 64):
        nrm, ku, knn = tdtk.calculateNormalsAdaptiveKNN(pts, k - 1, k - 1, RPOS, 20, want_k=True, want_knn=True)
        fn, fknn = tdtk.calculateNormalsKNN(pts, k, RPOS, 20, want_knn=True)
        assert (ku == k - 1).all(), k
        assert np.array_equal(knn, fknn), k
        assert np.array_equal(nrm, fn, equal_nan=True), k


def test_ann_with_one_k_is_the_fixed_k_estimator(tdtk, gpu):
    pts = CLOUDS["uniform"][0]
    for k in (1, 10, 16, 17, 32):
        for eps in ma.ANN_EPS:
            nrm, ku, knn = tdtk.calculateNormalsAdaptiveApxKNN(pts, k - 1, k - 1, RPOS, eps, want_k=True, want_knn=True)
            fn, fknn = tdtk.calculateNormalsApxKNN(pts, k, RPOS, eps, want_knn=True)
            assert (ku == k - 1).all(), (k, eps)
            assert np.array_equal(knn, fknn), (k, eps)
            assert np.array_equal(nrm, fn, equal_nan=True), (k, eps)


# ---- 4. more than one grid's worth of queries ----------------------------------------------------------------------------
BIG_CFG = (5, 12)


def _big_rows(pts):
    return np.sort(np.random.default_rng(1105).choice(len(pts), 300, replace=False))


def test_exact_on_more_queries_than_lanes(tdtk, orc, gpu):
    pts = big_cloud()
    rows = _big_rows(pts)
    nrm, ku, knn = tdtk.calculateNormalsAdaptiveKNN(pts, BIG_CFG[0], BIG_CFG[1], RPOS, 20, want_k=True, want_knn=True)
    kd = tdtk.KDtree(pts, 20)
    check_rows(orc, pts, rows, BIG_CFG[0], BIG_CFG[1], nrm, ku, knn, lambda Q, k: kd.kNearestNeighborsBatch(Q, k)[0], "big", 300)
    assert len(np.unique(ku)) >= 5
    if orc.have_ref():
        rn, rk = ma.reference_loop(orc, pts, rows, ma.exact_lists(ma.mgk.RefTree(pts, 20)), *BIG_CFG)
        assert np.array_equal(ku[rows], rk) and np.array_equal(nrm[rows], rn, equal_nan=True)


def test_ann_on_more_queries_than_threads(tdtk, orc, gpu):
    pts = big_cloud()
    rows = _big_rows(pts)
    ann = orc.AnnTree(pts)
    for eps in ma.ANN_EPS:
        nrm, ku, knn = tdtk.calculateNormalsAdaptiveApxKNN(pts, BIG_CFG[0], BIG_CFG[1], RPOS, eps, want_k=True, want_knn=True)
        check_rows(orc, pts, rows, BIG_CFG[0], BIG_CFG[1], nrm, ku, knn, lambda Q, k: ann.ksearch(Q, k, eps)[0], ("big", eps), 300)
        assert len(np.unique(ku)) >= 5
        if orc.have_ref():
            rn, rk = ma.reference_loop(orc, pts, rows, ma.ann_lists(orc.AnnTree(pts, "ref"), eps), *BIG_CFG)
            assert np.array_equal(ku[rows], rk) and np.array_equal(nrm[rows], rn, equal_nan=True)


# ---- 5. the deep cloud: the stack's overflow columns under a restarted walk ------------------------------------------------
def test_exact_on_the_deep_tree(tdtk, gpu):
    z, (pts, _) = fixture(), deep()
    rows = z["deep_rows"]
    nrm, ku = tdtk.calculateNormalsAdaptiveKNN(pts, ma.DEEP_CONFIG[0], ma.DEEP_CONFIG[1], RPOS, 1, want_k=True)
    key = ma.exact_key("deep", 1, ma.DEEP_CONFIG)
    assert np.array_equal(ku[rows], z[key + "_k"])
    assert np.array_equal(nrm[rows], z[key + "_n"], equal_nan=True)


def test_ann_on_the_deep_tree(tdtk, gpu):
    z, (pts, _) = fixture(), deep()
    rows = z["deep_rows"]
    for eps in ma.ANN_EPS:
        nrm, ku = tdtk.calculateNormalsAdaptiveApxKNN(pts, ma.DEEP_CONFIG[0], ma.DEEP_CONFIG[1], RPOS, eps, want_k=True)
        key = ma.ann_key("deep", ma.DEEP_CONFIG, eps)
        assert np.array_equal(ku[rows], z[key + "_k"]), eps
        assert np.array_equal(nrm[rows], z[key + "_n"], equal_nan=True), eps


# ---- 6. errors: refused on the host, nothing written ------------------------------------------------------------------------
EINVAL, EUNSUP = -1, -5
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def _call(tdtk, form, pts, kmin, kmax, rpos=(0.5, -2.0, 1.0), bucket=20, eps=0.0, n=None, null=()):
    """the C entry point with sentinel-filled outputs -> (code, message, outputs untouched)"""
    L = tdtk.lib()
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    n = len(pts) if n is None else n
    cols = max(kmax + 1, 1)
    rows = max(len(pts), 1)
    nrm = np.full((rows, 3), 7.5)
    ku = np.full(rows, -77, np.int32)
    knn = np.full((rows, cols), -77, np.int32)
    rp = np.array(rpos, np.float64)
    a_pts = None if "xyz" in null else pts.ctypes.data_as(_dp)
    a_rp = None if "rPos" in null else rp.ctypes.data_as(_dp)
    a_nrm = None if "normals" in null else nrm.ctypes.data_as(_dp)
    if form == "exact":
        rc = L.tdtk_normals_adaptive_knn(a_pts, n, kmin, kmax, a_rp, bucket, 0, a_nrm, ku.ctypes.data_as(_ip), knn.ctypes.data_as(_ip))
    else:
        rc = L.tdtk_normals_adaptive_apx_knn(a_pts, n, kmin, kmax, a_rp, eps, 0, a_nrm, ku.ctypes.data_as(_ip), knn.ctypes.data_as(_ip))
    clean = bool((nrm == 7.5).all() and (ku == -77).all() and (knn == -77).all())
    return rc, L.tdtk_last_error().decode(), clean


def test_errors_are_refused_before_anything_is_written(tdtk, gpu):
    pts = CLOUDS["uniform"][0]
    seven = CLOUDS["seven"][0]
    both = ("exact", "ann")
    cases = []
    for f in both:
        cases += [
            (f, dict(pts=pts, kmin=6, kmax=5), EINVAL, "kmin must not be larger than kmax"),
            (f, dict(pts=pts, kmin=-1, kmax=5), EINVAL, "kmin"),
            (f, dict(pts=pts, kmin=3, kmax=5, n=0), EINVAL, "Could not calculate normals, XYZ data is empty"),
            (f, dict(pts=np.zeros((0, 3)), kmin=3, kmax=5), EINVAL, "Could not calculate normals, XYZ data is empty"),
            (f, dict(pts=pts, kmin=3, kmax=5, null=("xyz",)), EINVAL, ""),
            (f, dict(pts=pts, kmin=3, kmax=5, null=("rPos",)), EINVAL, "rPos"),
            (f, dict(pts=pts, kmin=3, kmax=5, null=("normals",)), EINVAL, "NULL"),
        ]
    cases += [
        ("exact", dict(pts=pts, kmin=3, kmax=5, bucket=0), EINVAL, "bucket"),
        ("exact", dict(pts=pts, kmin=3, kmax=64), EUNSUP, "64"),
        ("exact", dict(pts=pts, kmin=64, kmax=64), EUNSUP, "64"),
        ("ann", dict(pts=pts, kmin=3, kmax=32), EUNSUP, "32"),
        ("ann", dict(pts=pts, kmin=3, kmax=5, eps=-0.5), EINVAL, "eps"),
        ("ann", dict(pts=pts, kmin=3, kmax=5, eps=float("nan")), EINVAL, "eps"),
        ("ann", dict(pts=pts, kmin=3, kmax=5, eps=float("inf")), EINVAL, "eps"),
        ("ann", dict(pts=seven, kmin=3, kmax=7), EINVAL, "Requesting more near neighbors than data points"),
        ("ann", dict(pts=CLOUDS["one"][0], kmin=0, kmax=1), EINVAL, "Requesting more near neighbors than data points"),
    ]
    for form, kw, code, msg in cases:
        rc, err, clean = _call(tdtk, form, **kw)
        assert rc == code and msg in err and clean, (form, {k: v for k, v in kw.items() if k != "pts"}, rc, err, clean)
    # the mirror raises the same
    with pytest.raises(tdtk.TdtkError) as e:
        tdtk.calculateNormalsAdaptiveKNN(pts, 6, 5, RPOS)
    assert e.value.code == EINVAL and "kmin must not be larger than kmax" in str(e.value)
    with pytest.raises(tdtk.TdtkError) as e:
        tdtk.calculateNormalsAdaptiveApxKNN(seven, 3, 7, RPOS)
    assert e.value.code == EINVAL
    # the limits themselves are served, and the library still answers
    rc, _, clean = _call(tdtk, "exact", pts, 60, 63)
    assert rc == 0 and not clean
    rc, _, clean = _call(tdtk, "ann", seven, 3, 6)
    assert rc == 0 and not clean
    nrm, ku = tdtk.calculateNormalsAdaptiveKNN(seven, 0, 3, RPOS, want_k=True)
    z = fixture()
    assert np.array_equal(ku, z[ma.exact_key("seven", 20, (0, 3)) + "_k"])
    assert np.array_equal(nrm, z[ma.exact_key("seven", 20, (0, 3)) + "_n"], equal_nan=True)
    assert np.array_equal(tdtk.calculateNormalsIndexedKNN(pts, 10, RPOS), tdtk.calculateNormalsKNN(pts, 10, RPOS, 20))
