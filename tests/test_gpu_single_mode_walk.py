"""The repeated passes of the resident ICP loop walk in ONE mode (kernels.hip, "the quick check deferred"): every query makes its
divergent visits on the 16-byte split halves without the quick check, a query without a previous hit keeps the check in
wave-uniform visits only, and a query that accepted a point thinly (within SearchArgs::tie of its closest_d2) retires marked and
is searched again behind its wave's slab -- cold, every check, the reference's own walk.

Every test runs the resident loop (tdtk_icp_match) over 262 144 .. 262 145 queries -- the smallest batch that takes the
persistent-lane kernel, whose second and later passes are the DEFER instantiation -- for five iterations and compares EVERY
iteration's index hash and pair count with the oracle's FindClosest over the points moved as the loop's trace says."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 262144
ITERS = 5
MAXD2 = 625.0


def _pose(tdtk):
    """The pose of bench.make_icp_pair: model frame -> data frame is x @ R.T + t."""
    T = tdtk.EulerToMatrix4([10.0, -5.0, 3.0], [0.02, -0.03, 0.05])
    Ti = tdtk.M4inv(T)
    R = np.array([[Ti[0], Ti[4], Ti[8]], [Ti[1], Ti[5], Ti[9]], [Ti[2], Ti[6], Ti[10]]])
    return R, np.array(Ti[12:15])


def _to_data_frame(tdtk, D):
    R, t = _pose(tdtk)
    return np.ascontiguousarray(D @ R.T + t)


def _pair(tdtk, n, seed, nq=None):
    """bench.make_icp_pair's cloud with the data still in the MODEL frame (so a test can place queries), nq queries."""
    rng = np.random.default_rng(seed)
    m = rng.uniform(-1000.0, 1000.0, (n, 3))
    nq = n if nq is None else nq
    src = rng.permutation(n)
    if nq > n:
        src = np.concatenate([src, rng.integers(0, n, nq - n)])
    D = m[src[:nq]] + rng.normal(0.0, 1.0, (nq, 3))
    return m, D, rng


def _add_twins(m, rng, src):
    """Every point of `src` gets a twin 1e-12 .. 1e-11 away along one axis (another point of the model is moved there)."""
    k = len(src)
    dst = np.setdiff1d(np.arange(len(m)), src)[:k]
    off = np.zeros((k, 3))
    off[np.arange(k), rng.integers(0, 3, k)] = rng.uniform(1e-12, 1e-11, k) * rng.choice([-1.0, 1.0], k)
    m[dst] = m[src] + off
    assert not np.array_equal(m[dst], m[src])


def _loop(tdtk, gpu, model, d, mode=0, minimizer=None):
    """One resident loop of ITERS iterations over a fresh data scan.  mode: tdtk_visit_counting (0 off, 1 the kernel's own walk,
    2 every search cold).  -> (index hashes, trace, counters)"""
    L = tdtk.lib()
    data = tdtk.Scan([0, 0, 0], [0, 0, 0], d)
    c = (C.c_uint64 * 8)()
    was = L.tdtk_icp_index_hashes(1)
    if mode:
        L.tdtk_visit_counting(gpu, mode)
    try:
        icp = tdtk.icp6D(minimizer or tdtk.icp6D_QUAT(True), 25.0, ITERS, quiet=True, epsilonICP=-1.0)
        assert icp.match(model, data) == ITERS - 1
        if mode:
            L.tdtk_visit_counters(gpu, c)
    finally:
        L.tdtk_icp_index_hashes(was)
        if mode:
            L.tdtk_visit_counting(gpu, 0)
    data.release()
    return list(icp.last["index_hashes"]), icp.last["trace"].copy(), [int(x) for x in c]


def _threads():
    return max(8, min(96, os.cpu_count() or 8))


def _oracle(orc, m, d, trace):
    """The oracle's FindClosest over the points moved as `trace` says: per iteration (index hash, pairs, indices)."""
    ot = orc.Tree(m, 20)
    cur = d.copy()
    out = []
    for it in range(len(trace)):
        idx, _ = ot.find_closest(cur, MAXD2, _threads())
        out.append((orc.k5_hash(idx), int((idx >= 0).sum()), idx))
        orc.transform_points(trace[it, 2:], cur)
    return out


def _assert_is_the_oracles(orc, m, d, hashes, trace):
    assert len(hashes) == ITERS and len(trace) == ITERS
    ref = _oracle(orc, m, d, trace)
    for it, (h, pairs, _) in enumerate(ref):
        assert pairs == int(trace[it, 0]), (it, pairs, int(trace[it, 0]))
        assert h == hashes[it], (it, "0x%x" % h, "0x%x" % hashes[it])
    return ref


# ---- the clouds, and one plain run + its oracle comparison per cloud, shared by the tests below ----
@pytest.fixture(scope="module")
def twins(tdtk, orc, gpu):
    """10 % of a 262 144-point model gets a twin 1e-12 .. 1e-11 away: thousands of queries see two candidates whose d2 differ
    by less than SearchArgs::tie (~5e-10 here)."""
    m, D, rng = _pair(tdtk, N, 45)
    _add_twins(m, rng, rng.choice(N, N // 10, replace=False))
    d = _to_data_frame(tdtk, D)
    model = tdtk.Scan([0, 0, 0], [0, 0, 0], m)
    hashes, trace, _ = _loop(tdtk, gpu, model, d)
    _assert_is_the_oracles(orc, m, d, hashes, trace)
    return dict(m=m, d=d, model=model, hashes=hashes, trace=trace)


def _nopartner_cloud(tdtk, probe_trace=None):
    """Half the queries pushed 10 .. 40 units beyond a face of the model's box (some within the radius of it, some beyond), a
    cube of side 500 emptied of model points with queries left in it, and in its middle -- in a ball of radius 160 cleared of
    other queries -- ONE query Q with ONE model point J near it.  With the trace of a first run (J parked 75 units off, where it
    pairs with nobody), J goes where the last iteration's Q sees it at d2 == maxd2 exactly: strict `<`, no pair."""
    m, D, rng = _pair(tdtk, N, 46)
    ce = np.array([300.0, 300.0, 300.0])
    inside = np.flatnonzero(np.all(np.abs(m - ce) < 250.0, axis=1))
    for i in inside:                                   # the model's points of the cube go elsewhere
        while np.all(np.abs(m[i] - ce) < 250.0):
            m[i] = rng.uniform(-1000.0, 1000.0, 3)
    half = rng.permutation(N)[: N // 2]
    ax = rng.integers(0, 3, len(half))
    D[half, ax] = rng.choice([-1.0, 1.0], len(half)) * (1000.0 + rng.uniform(10.0, 40.0, len(half)))
    near = np.flatnonzero(np.linalg.norm(D - ce, axis=1) < 160.0)
    D[near, 0] = -1000.0 - rng.uniform(10.0, 40.0, len(near))     # (beyond a face, like the half above)
    assert int(np.all(np.abs(D - ce) < 200.0, axis=1).sum()) > 100  # queries inside the box where the model is empty
    Q = int(near[0]) if len(near) else 0
    D[Q] = ce
    d = _to_data_frame(tdtk, D)
    J = int(np.argmin(np.linalg.norm(m - (ce + [600.0, 0.0, 0.0]), axis=1)))     # some model point: it becomes J
    m[J] = ce + [75.0, 0.0, 0.0]
    if probe_trace is None:
        return m, d, Q, J, None
    # where Q is at each iteration (the loop moves the points with exactly this arithmetic; the model is at the identity pose,
    # so the tree's frame is the world's)
    from oracle import orc
    q = np.empty((ITERS, 3))
    cur = d[Q:Q + 1].copy()
    for it in range(ITERS):
        q[it] = cur[0]
        orc.transform_points(probe_trace[it, 2:], cur)
    k = ITERS - 1
    for a in range(3):
        for s in (-1.0, 1.0):
            Jp = q[k].copy()
            Jp[a] = q[k][a] + 25.0 * s
            dd = (Jp - q)                                  # [ITERS][3]
            d2 = dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1] + dd[:, 2] * dd[:, 2]
            if d2[k] == MAXD2 and np.all(d2[:k] >= MAXD2):
                m[J] = Jp
                return m, d, Q, J, q
    raise AssertionError("no axis puts J at d2 == maxd2 from the last iteration's Q and out of reach of the earlier ones")


@pytest.fixture(scope="module")
def nopartner(tdtk, orc, gpu):
    m0, d, Q, J, _ = _nopartner_cloud(tdtk)
    probe = tdtk.Scan([0, 0, 0], [0, 0, 0], m0)
    _, tr0, _ = _loop(tdtk, gpu, probe, d)
    m, d1, Q1, J1, q = _nopartner_cloud(tdtk, tr0)
    assert np.array_equal(d, d1) and (Q, J) == (Q1, J1)
    model = tdtk.Scan([0, 0, 0], [0, 0, 0], m)
    hashes, trace, _ = _loop(tdtk, gpu, model, d)
    # J pairs with nobody in either place, so the loop is the first run's, Q is where the construction put it ...
    assert np.array_equal(trace, tr0)
    ref = _assert_is_the_oracles(orc, m, d, hashes, trace)
    return dict(m=m, d=d, model=model, hashes=hashes, trace=trace, Q=Q, J=J, q=q, ref=ref)


def test_twins_are_searched_again_behind_the_slab(tdtk, gpu, twins):
    """Case 1.  The plain run equals the oracle (the fixture); the counting run reports second searches (counters[7]) and has
    the same hashes and the same trace."""
    h1, t1, c = _loop(tdtk, gpu, twins["model"], twins["d"], mode=1)
    assert c[7] > 100, c
    assert c[3] == N * ITERS, c
    assert h1 == twins["hashes"] and np.array_equal(t1, twins["trace"])


@pytest.mark.parametrize("nq", [N, N + 1])
def test_a_slab_of_queries_that_all_lie_next_to_twins_and_the_tail_slab(tdtk, orc, gpu, nq):
    """Case 2.  EVERY model point of the cube [-1000, -400]^3 has a twin.  The resident scan is in Morton order over its own
    box, and that cube contains whole cells of the order's third level (1/512 of the box, ~512 queries each, contiguous in
    the order) whatever the 0.05 rad between the two frames does to the cells' edges: at least one stretch of 512 sorted
    queries -- two whole slabs of 256 -- in which every query has two candidates a rounding apart.  262 145 queries: the last
    slab holds one query."""
    m, D, rng = _pair(tdtk, N, 47, nq)
    src = np.flatnonzero(np.all(m < -400.0, axis=1))
    assert 5000 < len(src) < 10000
    _add_twins(m, rng, src)
    d = _to_data_frame(tdtk, D)
    model = tdtk.Scan([0, 0, 0], [0, 0, 0], m)
    hashes, trace, _ = _loop(tdtk, gpu, model, d)
    _assert_is_the_oracles(orc, m, d, hashes, trace)
    h1, t1, c = _loop(tdtk, gpu, model, d, mode=1)
    assert c[7] > 256, c
    assert h1 == hashes and np.array_equal(t1, trace)


def test_queries_without_a_partner_stay_without_one(tdtk, gpu, nopartner):
    """Case 3.  Wherever the oracle says -1 the loop says -1 (the hashes are over all indices, -1 included; the pair counts are
    the oracle's: the fixture).  Here: the cloud is what its docstring says, in every iteration."""
    ref, Q, q, m, J = nopartner["ref"], nopartner["Q"], nopartner["q"], nopartner["m"], nopartner["J"]
    k = ITERS - 1
    dd = m[J] - q[k]
    assert dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2] == MAXD2           # d2 == maxd2 exactly: strict `<`, no pair
    for it in range(ITERS):
        idx = ref[it][2]
        assert idx[Q] == -1, it
        # (half the queries lie 10 .. 40 beyond a face: those nearer than the radius can still find a partner)
        assert 0.35 * N < int((idx < 0).sum()) < 0.60 * N, (it, int((idx < 0).sum()))
    assert not np.any(ref[k][2] == J)                                           # nobody pairs with J


def test_exact_duplicates_in_the_model_resolve_as_in_the_cold_search(tdtk, orc, gpu):
    """Case 4.  3 % of the model's points are exact copies of other points: equal distances, the first one visited wins."""
    m, D, rng = _pair(tdtk, N, 48)
    k = (3 * N) // 100
    src = rng.choice(N, k, replace=False)
    dst = np.setdiff1d(np.arange(N), src)[:k]
    m[dst] = m[src]
    d = _to_data_frame(tdtk, D)
    model = tdtk.Scan([0, 0, 0], [0, 0, 0], m)
    hashes, trace, _ = _loop(tdtk, gpu, model, d)
    _assert_is_the_oracles(orc, m, d, hashes, trace)


def test_a_repeated_pass_without_the_sums_inside(tdtk, orc, gpu, twins):
    """Case 5.  -a 6 (APX) wants sums beyond the base block, so its passes are searches with k_accum behind them: the repeated
    ones are the DEFER instantiation WITHOUT a sums epilogue (FUSE 0), whose second searches are a pass of their own."""
    m, d, model = twins["m"], twins["d"], twins["model"]
    hashes, trace, _ = _loop(tdtk, gpu, model, d, minimizer=tdtk.icp6D_APX(True))
    _assert_is_the_oracles(orc, m, d, hashes, trace)
    h1, t1, c = _loop(tdtk, gpu, model, d, mode=1, minimizer=tdtk.icp6D_APX(True))
    assert c[7] > 100, c
    assert h1 == hashes and np.array_equal(t1, trace)


@pytest.mark.parametrize("cloud", ["twins", "nopartner"])
def test_the_trace_does_not_depend_on_the_walk(tdtk, gpu, cloud, request):
    """Case 6.  tdtk_visit_counting(dev, 2) makes every search of the loop cold (no warm start, no DEFER instantiation): the
    trace is the plain run's bit for bit."""
    f = request.getfixturevalue(cloud)
    h2, t2, c = _loop(tdtk, gpu, f["model"], f["d"], mode=2)
    assert c[7] == 0, c
    assert h2 == f["hashes"] and np.array_equal(t2, f["trace"])
