"""The certificate sweep in two round trips (kernels.hip, cert_sweep): a wave reads its whole slab -- up to
four rounds of 64 queries -- before it decides anything, a lane beyond the slab's end reads the last query again and stores
nothing, order_piece takes the cost bytes from the sweep, and the pass that searches thin acceptances again is entered only by a
wave one of whose lanes has marked a query.  Nothing of that may change a bit.

Every case runs the resident loop for 5-6 iterations against a model of ~100 K points and asserts, with the helpers of
test_gpu_cert_skip: every iteration's index hash and pair count are the oracle's, the trace is bit-identical with
TDTK_CERT_SKIP=0, and skipped + walked = n in every pass.

Slab lengths: 256 CUs x 4 SIMDs x 6 waves = 6144 slabs; a slab is ceil(n / 6144) rounded up to 8, at least 128.

The skip and visit counters come from the INSTRUMENTED instantiation of the kernel (COUNT), which is not the timed one: with
the batched sweep it takes 116 vector registers and four waves per SIMD where the product's kernel takes 80 and six.  Its
counts are the product's (the walk is the same); how long a counted pass takes says nothing about the product."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_cert_skip as T      # noqa: E402  (its helpers: _cloud, _frame, _run, _check, _per_pass)

pytestmark = pytest.mark.gpu

SMALL_POSE = ([1.0, -0.5, 0.3], [0.0004, -0.0003, 0.0005])     # the small offset of test_gpu_cert_skip's case 2


def _converging(tdtk, seed, nq, m=None):
    """Data = model points + noise of 1 % of the spacing, in the frame of the small pose."""
    rng = np.random.default_rng(seed)
    if m is None:
        m = rng.uniform(-1000.0, 1000.0, (T.NM, 3))
    D = m[rng.integers(0, len(m), nq)] + rng.normal(0.0, 0.01 * T.SPACING, (nq, 3))
    return m, T._frame(tdtk, D, *SMALL_POSE), rng


def _accounted(pp, nq):
    for it, (skh, skn, walked, _) in enumerate(pp):
        print("pass %d: skipped with a hit %d, without %d, walked %d" % (it, skh, skn, walked))
        assert skh + skn + walked == nq, (it, pp[it])


def test_slab_geometry_of_the_cases():
    """(the sizes below are what the docstrings say: rounds per slab, lanes of the last round, the tail slab)"""
    def slab(n):
        return max(128, -(-(-(-n // 6144)) // 8) * 8)
    assert slab(262145) == 128 and 262145 % 128 == 1
    assert slab(786433) == 136 and 136 - 128 == 8
    assert slab(1179649) == 200 and 200 - 192 == 8


@pytest.mark.parametrize("nq", [262145, 786433, 1179649])
def test_slabs_of_two_three_and_four_rounds(tdtk, orc, gpu, nq):
    """n = 262 145: slabs of 128, two full rounds, the last slab one query.  786 433: slabs of 136, a third round of 8 lanes.
    1 179 649: slabs of 200, a fourth round of 8 lanes.  A converging pair: from the fourth pass on most queries are skipped."""
    iters = 5
    m, d, _ = _converging(tdtk, 300 + nq % 97, nq)
    model, _, _, _ = T._check(tdtk, orc, gpu, m, d, iters)
    pp = T._per_pass(tdtk, gpu, model, d, iters)
    _accounted(pp, nq)
    assert pp[0][:2] == [0, 0] and pp[1][:2] == [0, 0], pp[:2]
    assert sum(p[0] + p[1] for p in pp[3:]) > 0, pp


def _duplicated(tdtk, orc, gpu, seed, pick):
    """A model in which the points pick(m, rng) selects have an exact copy: a query whose hit has one always walks (the runner-up
    IS the hit's distance: test_gpu_cert_skip.test_exact_ties_are_never_skipped).  -> per pass: walked, skipped, queries whose
    previous hit is a duplicated point (from the oracle's indices)."""
    iters, nq = 6, 262145
    rng = np.random.default_rng(seed)
    m = rng.uniform(-1000.0, 1000.0, (T.NM, 3))
    sel = pick(m, rng)
    isdup = np.zeros(T.NM + len(sel), bool)
    isdup[sel] = True
    isdup[T.NM:] = True
    mm = np.concatenate([m, m[sel]])
    D = m[rng.integers(0, T.NM, nq)] + rng.normal(0.0, 0.01 * T.SPACING, (nq, 3))
    d = T._frame(tdtk, D, *SMALL_POSE)
    model, _, _, ref = T._check(tdtk, orc, gpu, mm, d, iters)
    pp = T._per_pass(tdtk, gpu, model, d, iters)
    _accounted(pp, nq)
    ondup = [int(isdup[np.maximum(ref[it][2], 0)][ref[it][2] >= 0].sum()) for it in range(iters)]
    print("queries whose hit is a duplicated point, per pass:", ondup)
    for it in range(iters):
        assert 0.45 * nq <= ondup[it] <= 0.55 * nq, (it, ondup[it])
    for it in range(3, iters):
        skh, skn, walked, _ = pp[it]
        assert walked >= ondup[it - 1], (it, walked, ondup[it - 1])
        assert skh + skn > 0, (it, pp[it])
    return pp, ondup


def test_about_sixty_four_walkers_per_slab(tdtk, orc, gpu):
    """Half of the model points, chosen at random, have an exact copy: the walkers of a slab of 128 are Binomial(128, 1/2) --
    mean 64, sigma 5.7 --, so hundreds of the 2049 slabs list 63, 64 or 65 of them: both sides of one full round of lanes."""
    _duplicated(tdtk, orc, gpu, 311, lambda m, rng: rng.permutation(T.NM)[: T.NM // 2])


def test_slabs_where_everybody_walks_and_slabs_where_nobody_does(tdtk, orc, gpu):
    """Exactly the model points with x < 0 have a copy.  The sorted scan is spatial: slabs all of whose queries walk, slabs
    with no walker at all (an empty hand-out order), and a few mixed ones."""
    _duplicated(tdtk, orc, gpu, 312, lambda m, rng: np.flatnonzero(m[:, 0] < 0.0))


def test_a_posed_model(tdtk, orc, gpu):
    """The model scan has a pose of its own: the sweep maps the old and the new position of every query with `inv`.  The oracle
    gets the same points in the world frame."""
    iters, nq = 5, 262145
    pos, theta = [3.0, -2.0, 1.0], [0.01, 0.02, -0.01]
    rng = np.random.default_rng(313)
    local = rng.uniform(-1000.0, 1000.0, (T.NM, 3))
    world = local.copy()
    orc.transform_points(np.asarray(tdtk.EulerToMatrix4(pos, theta), dtype=np.float64), world)
    _, d, _ = _converging(tdtk, 314, nq, world)
    model = tdtk.Scan(pos, theta, local)
    T._check(tdtk, orc, gpu, world, d, iters, model=model)
    pp = T._per_pass(tdtk, gpu, model, d, iters)
    _accounted(pp, nq)
    assert sum(p[0] + p[1] for p in pp[3:]) > 0, pp


def _loop_with_normals(tdtk, gpu, model, d, iters, cert, counting=False):
    """T._run over a data scan that carries normals (calcNormals() before the loop) -> (index hashes, trace, skip counters,
    normals and points after the loop)."""
    L = tdtk.lib()
    data = tdtk.Scan([0, 0, 0], [0, 0, 0], d)
    data.calcNormals()
    s = (C.c_uint64 * 4)()
    old = os.environ.get("TDTK_CERT_SKIP")
    os.environ["TDTK_CERT_SKIP"] = "1" if cert else "0"
    was = L.tdtk_icp_index_hashes(1)
    if counting:
        L.tdtk_visit_counting(gpu, 1)
    try:
        icp = tdtk.icp6D(tdtk.icp6D_QUAT(True), 25.0, iters, quiet=True, epsilonICP=-1.0)
        assert icp.match(model, data) == iters - 1
        if counting:
            L.tdtk_skip_counters(gpu, s)
    finally:
        L.tdtk_icp_index_hashes(was)
        if counting:
            L.tdtk_visit_counting(gpu, 0)
        if old is None:
            del os.environ["TDTK_CERT_SKIP"]
        else:
            os.environ["TDTK_CERT_SKIP"] = old
    nrm, xyz = data.get_normal_reduced().copy(), data.get_xyz_reduced().copy()
    data.release()
    return list(icp.last["index_hashes"]), icp.last["trace"].copy(), [int(x) for x in s], nrm, xyz


def test_normals_move_with_the_points(tdtk, orc, gpu):
    """The data scan carries normals: the sweep moves them with the points (one more batch behind the points').  Every
    iteration's index hash and pair count are the oracle's, every pass accounts for every query and the later ones do skip --
    the certificates are live on a scan with normals --, and normals and points after the loop are bit-identical with and
    without certificates."""
    iters, nq = 5, 262145
    m, d, _ = _converging(tdtk, 315, nq)
    model = tdtk.Scan([0, 0, 0], [0, 0, 0], m)
    h1, t1, _, n1, x1 = _loop_with_normals(tdtk, gpu, model, d, iters, True)
    h0, t0, _, n0, x0 = _loop_with_normals(tdtk, gpu, model, d, iters, False)
    assert n1 is not None and np.isfinite(n1).all() and np.abs(n1).max() > 0.5
    assert np.array_equal(t1, t0), "the trace depends on TDTK_CERT_SKIP"
    assert h1 == h0
    for it, (h, pairs, _, _) in enumerate(T._oracle(orc, m, d, t1)):
        assert pairs == int(t1[it, 0]), (it, pairs, int(t1[it, 0]))
        assert h == h1[it], (it, "0x%x" % h, "0x%x" % h1[it])
    assert np.array_equal(x1, x0), int((x1 != x0).any(axis=1).sum())
    assert np.array_equal(n1, n0), int((n1 != n0).any(axis=1).sum())
    assert not np.array_equal(x1, d)      # (the loop did move them)
    # per pass, as T._per_pass counts them: counted loops of 1 .. iters iterations, differenced
    cum = [[0, 0, 0, 0]]
    for k in range(1, iters + 1):
        hk, tk, sk, _, _ = _loop_with_normals(tdtk, gpu, model, d, k, True, counting=True)
        assert hk == h1[:k] and np.array_equal(tk, t1[:k])
        cum.append(sk)
    pp = [[b - a for a, b in zip(cum[k], cum[k + 1])] for k in range(iters)]
    _accounted(pp, nq)
    assert pp[0][:2] == [0, 0] and pp[1][:2] == [0, 0], pp[:2]
    for it in range(3, iters):
        assert pp[it][0] + pp[it][1] > 0, (it, pp[it])


@pytest.mark.parametrize("twin", [True, False])
def test_one_mark_in_the_whole_launch(tdtk, orc, gpu, twin):
    """One model point at the cloud's corner has a twin 1e-12 away, and a handful of queries stand on either side of the pair:
    whichever the walk meets second improves closest_d2 by less than SearchArgs::tie, so there are second searches
    (tdtk_visit_counters out[7]) -- and every wave but the one or two that hold those queries skips the pass behind its loop.
    Without the twin nobody marks anything and no wave enters it.  Indices are the oracle's in both."""
    iters, nq, k = 5, 262145, 8
    m, D, rng = T._cloud(316, nq, 0.01 * T.SPACING)
    m[0] = [999.0, 999.0, 999.0]
    if twin:
        m[1] = m[0] + [1e-12, 0.0, 0.0]
        assert m[1, 0] != m[0, 0]
    side = np.where(np.arange(k) % 2 == 0, 1.0, -1.0)
    D[:k] = m[0] + np.stack([side * 0.3, rng.normal(0, 0.05, k), rng.normal(0, 0.05, k)], axis=1)
    d = T._frame(tdtk, D, *SMALL_POSE)
    model, h1, t1, ref = T._check(tdtk, orc, gpu, m, d, iters)
    hc, tc, s, c = T._run(tdtk, gpu, model, d, iters, counting=True)
    assert hc == h1 and np.array_equal(tc, t1)
    assert s[0] + s[1] + s[2] == nq * iters, s
    _accounted(T._per_pass(tdtk, gpu, model, d, iters), nq)
    print("second searches:", c[7], "of them counted by the skip counters:", s[3])
    if twin:
        assert all(int(ref[it][2][j]) in (0, 1) for it in range(iters) for j in range(k))
        assert c[7] >= 1, c
    else:
        assert c[7] == 0, c
