"""A certificate per query (kernels.hip, "a certificate per query"): from the third pass of a resident ICP
loop on, a query whose previous hit provably stays nearest -- or which provably stays without a partner -- is answered by one
distance computation instead of a walk.  A walk of such a loop prunes against a radius that does not shrink and leaves behind a
lower bound L on the distance to every tree point but its hit.

Every case runs the resident loop (tdtk_icp_match) over 262 145 or 300 001 queries -- just above the smallest batch that takes
the persistent-lane kernel, the tail slab partial -- against a model of ~100 K points, compares EVERY iteration's index hash and
pair count with the oracle's FindClosest over the points moved as the loop's trace says, and asserts that the trace (pairs, RMS,
alignxf per iteration) is bit-identical with TDTK_CERT_SKIP=0 and =1."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NM = 100000
MAXD2 = 625.0
SPACING = 2000.0 / NM ** (1.0 / 3.0)          # ~43 units between neighbours of the uniform model
KAPPA, M_LO, M_HI = 4.0, 1.0 / 64.0, 0.25     # the library's margin policy (api_search.cpp: cert_policy)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frame(tdtk, D, trans, rot):
    """Model frame -> data frame for the pose (trans, rot): x @ R.T + t with (R, t) the inverse pose, as bench.make_icp_pair."""
    Ti = tdtk.M4inv(tdtk.EulerToMatrix4(list(trans), list(rot)))
    R = np.array([[Ti[0], Ti[4], Ti[8]], [Ti[1], Ti[5], Ti[9]], [Ti[2], Ti[6], Ti[10]]])
    return np.ascontiguousarray(D @ R.T + np.array(Ti[12:15]))


def _cloud(seed, nq, noise, nm=NM, half=1000.0):
    rng = np.random.default_rng(seed)
    m = rng.uniform(-half, half, (nm, 3))
    src = rng.integers(0, nm, nq)
    return m, m[src] + rng.normal(0.0, noise, (nq, 3)), rng


def _run(tdtk, gpu, model, d, iters, cert=True, counting=False, rnd=1):
    """One resident loop over a fresh data scan -> (index hashes, trace, skip counters [skipped with a hit, skipped without,
    walked, second searches], visit counters)."""
    L = tdtk.lib()
    data = tdtk.Scan([0, 0, 0], [0, 0, 0], d)
    s, c = (C.c_uint64 * 4)(), (C.c_uint64 * 8)()
    old = os.environ.get("TDTK_CERT_SKIP")
    os.environ["TDTK_CERT_SKIP"] = "1" if cert else "0"
    was = L.tdtk_icp_index_hashes(1)
    if counting:
        L.tdtk_visit_counting(gpu, 1)
    try:
        icp = tdtk.icp6D(tdtk.icp6D_QUAT(True), 25.0, iters, quiet=True, epsilonICP=-1.0, rnd=rnd)
        assert icp.match(model, data) == iters - 1
        if counting:
            L.tdtk_skip_counters(gpu, s)
            L.tdtk_visit_counters(gpu, c)
    finally:
        L.tdtk_icp_index_hashes(was)
        if counting:
            L.tdtk_visit_counting(gpu, 0)
        if old is None:
            del os.environ["TDTK_CERT_SKIP"]
        else:
            os.environ["TDTK_CERT_SKIP"] = old
    data.release()
    return list(icp.last["index_hashes"]), icp.last["trace"].copy(), [int(x) for x in s], [int(x) for x in c]


def _per_pass(tdtk, gpu, model, d, iters):
    """The skip counters of every pass: counted loops of 1 .. iters iterations (the loop is deterministic), differenced."""
    cum = [[0, 0, 0, 0]] + [_run(tdtk, gpu, model, d, k, counting=True)[2] for k in range(1, iters + 1)]
    return [[b - a for a, b in zip(cum[k], cum[k + 1])] for k in range(iters)]


def _threads():
    return max(8, min(96, os.cpu_count() or 8))


def _oracle(orc, m, d, trace):
    """Per iteration: (index hash, pairs, indices, the queries' positions) of the oracle's FindClosest over the moved points."""
    ot = orc.Tree(m, 20)
    cur = d.copy()
    out = []
    for it in range(len(trace)):
        idx, _ = ot.find_closest(cur, MAXD2, _threads())
        out.append((orc.k5_hash(idx), int((idx >= 0).sum()), idx, cur.copy()))
        orc.transform_points(trace[it, 2:], cur)
    return out


def _check(tdtk, orc, gpu, m, d, iters, model=None):
    """The loop with certificates equals the oracle in every iteration and the loop without them bit for bit."""
    model = model or tdtk.Scan([0, 0, 0], [0, 0, 0], m)
    h1, t1, _, _ = _run(tdtk, gpu, model, d, iters, cert=True)
    h0, t0, _, _ = _run(tdtk, gpu, model, d, iters, cert=False)
    assert np.array_equal(t1, t0), "the trace depends on TDTK_CERT_SKIP"
    assert h1 == h0
    ref = _oracle(orc, m, d, t1)
    for it, (h, pairs, _, _) in enumerate(ref):
        assert pairs == int(t1[it, 0]), (it, pairs, int(t1[it, 0]))
        assert h == h1[it], (it, "0x%x" % h, "0x%x" % h1[it])
    return model, h1, t1, ref


@pytest.mark.parametrize("nq", [262145, 300001])
def test_a_pair_in_mid_alignment(tdtk, orc, gpu, nq):
    """Case 1.  The bench's pose over a cube of side 800 (spacing ~17): the queries start up to ~30 units -- more than the model's
    spacing -- from where they belong and move by 0.88 .. 1.34 units (5 .. 8 % of the spacing, measured) in EVERY one of nine
    iterations, so hits change hands all along.  Every pass
    accounts for every query (walked + skipped = N); the cold pass and the pass that writes the first certificates skip nobody;
    later passes do skip."""
    iters = 9
    m, D, _ = _cloud(101, nq, 1.0, half=400.0)
    d = _frame(tdtk, D, [10.0, -5.0, 3.0], [0.02, -0.03, 0.05])
    model, _, trace, ref = _check(tdtk, orc, gpu, m, d, iters)
    moved = [float(np.linalg.norm(ref[it + 1][3] - ref[it][3], axis=1).mean()) for it in range(iters - 1)]
    print("mean move per iteration:", moved)
    assert len(moved) >= 8 and min(moved) > 0.04 * 0.4 * SPACING, moved      # (every iteration: 4 % of this cube's spacing of 17.2)
    changed = sum(int((ref[it + 1][2] != ref[it][2]).sum()) for it in range(1, iters - 1))
    assert changed > 1000, changed                      # hits do change hands on repeated passes
    pp = _per_pass(tdtk, gpu, model, d, iters)
    for it, (skh, skn, walked, _) in enumerate(pp):
        print("pass %d: skipped with a hit %d, without %d, walked %d" % (it, skh, skn, walked))
        assert skh + skn + walked == nq, (it, pp[it])
    assert pp[0][:2] == [0, 0] and pp[1][:2] == [0, 0], pp[:2]
    assert sum(p[0] + p[1] for p in pp[2:]) > 0, pp


def _two_nearest(m, q):
    """Exact distances from every query to its nearest and second-nearest model point."""
    try:
        from scipy.spatial import cKDTree
        dist, _ = cKDTree(m).query(q, k=2, workers=-1)
        return dist[:, 0], dist[:, 1]
    except ImportError:
        from oracle import orc as _orc
        _, d2 = _orc.AnnTree(m).ksearch(q, 2, 0.0)
        return np.sqrt(d2[:, 0]), np.sqrt(d2[:, 1])


def test_a_converging_pair_skips_what_the_policy_admits(tdtk, orc, gpu):
    """Case 2.  Data = model + noise of 1 % of the spacing, a small initial offset, twelve iterations.  The policy is replayed on
    the CPU from the exact first and second neighbour distances at every iteration's positions, the moves between them and the
    library's kappa / caps: a query skips pass p >= 2 iff its previous hit lies at d < min(maxdist, L - delta); a skip leaves
    L - delta; a walk from distance d with m = clamp(kappa delta, d / 64, d / 4) leaves L = min(d_hit + m, second neighbour).
    The kernel may be more cautious by its rounding margins only: it skips at least 0.98 of what the replay admits, and the
    replay admits at least 0.9 of the queries from pass 3 on."""
    iters, nq = 12, 262145
    m, D, _ = _cloud(102, nq, 0.01 * SPACING)
    d = _frame(tdtk, D, [1.0, -0.5, 0.3], [0.0004, -0.0003, 0.0005])
    model, _, trace, ref = _check(tdtk, orc, gpu, m, d, iters)
    pp = _per_pass(tdtk, gpu, model, d, iters)
    L = np.zeros(nq)
    R = np.sqrt(MAXD2)
    for p in range(1, iters):
        q, qprev, prev_idx = ref[p][3], ref[p - 1][3], ref[p - 1][2]
        delta = np.linalg.norm(q - qprev, axis=1)
        d1, d2nd = _two_nearest(m, q)
        has = prev_idx >= 0
        dprev = np.where(has, np.linalg.norm(m[np.maximum(prev_idx, 0)] - q, axis=1), R)   # to the previous hit, or the radius
        skip = (p >= 2) & np.where(has, (dprev < R) & (dprev < L - delta), R <= L - delta)
        dstart = np.minimum(dprev, R)
        mg = np.clip(KAPPA * delta, M_LO * dstart, M_HI * dstart)
        dhit = np.where(d1 < R, d1, R)
        Lwalk = np.minimum(np.minimum(dstart + mg, dhit + mg), np.where(d1 < R, d2nd, d1))
        L = np.where(skip, L - delta, Lwalk)
        admitted, got = int(skip.sum()), pp[p][0] + pp[p][1]
        print("pass %d: the policy admits %d of %d (%.4f), the kernel skipped %d" % (p, admitted, nq, admitted / nq, got))
        assert pp[p][0] + pp[p][1] + pp[p][2] == nq, (p, pp[p])
        assert got >= 0.98 * admitted, (p, got, admitted)
        if p >= 3:
            assert admitted >= 0.9 * nq, (p, admitted)


def test_exact_ties_are_never_skipped(tdtk, orc, gpu):
    """Case 3.  Every model point has an exact copy: a bit-exact tie for every query in EVERY pass, whatever the loop does to the
    data -- the runner-up IS the hit's distance, so no query whose hit has a copy is ever skipped (only the k points below, which
    have none, can be kept by certificate).  A tenth of the queries also start bit-exactly equidistant from two DIFFERENT model
    points; that tie is the cold pass's alone (the first alignxf moves the data off the bisecting plane -- no rigid motion the
    loop computes keeps a query on it), so what it checks is that the winner of a tied cold pass warm-starts the later ones as the
    oracle says.  Indices are the oracle's in every pass: the first one visited wins."""
    iters, nq = 6, 262145
    m, D, rng = _cloud(103, nq, 1.0, NM // 2)
    k = nq // 10                     # equidistant at the start: the model point p and p + (8, 0, 0), the query on the plane between
    tw = rng.choice(len(m), k, replace=False)
    m = np.round(m * 4.0) / 4.0      # (coordinates on a grid of 1/4: the differences below are exact)
    m2 = m.copy()
    m2[tw, 0] += 8.0
    D[:k] = m[tw] + np.stack([np.full(k, 4.0), np.round(rng.normal(0, 1, k) * 4) / 4, np.round(rng.normal(0, 1, k) * 4) / 4], axis=1)
    a, b = m[tw] - D[:k], m2[tw] - D[:k]
    assert np.array_equal((a * a).sum(1), (b * b).sum(1))
    m = np.concatenate([m, m2])      # every point twice, except the moved ones (which are two points 8 apart)
    model, _, _, ref = _check(tdtk, orc, gpu, m, D.copy(), iters)        # (identity pose: the first pass sees the ties as built)
    pp = _per_pass(tdtk, gpu, model, D, iters)
    dup_hit = [int((ref[it][2] >= 0).sum()) for it in range(iters)]
    assert min(dup_hit) > 0.5 * nq
    # only a query whose hit is one of the k moved points (no copy) can keep it by certificate
    for it, (skh, skn, walked, _) in enumerate(pp):
        assert skh + skn + walked == nq, (it, pp[it])
        lone = int(np.isin(ref[it][2], np.concatenate([tw, tw + NM // 2])).sum())
        assert skh <= lone, (it, skh, lone)


def test_twins_are_searched_again_and_carry_no_certificate(tdtk, orc, gpu):
    """Case 4.  The cloud of test_thin_acceptances_are_searched_again: 30 000 model points get a twin 1e-12 .. 1e-11 away.  Second
    searches happen on walks with a fixed radius too, every iteration's indices are the oracle's, and a pass skips at most the
    queries the pass before did not search a second time.  (With a twin that close the runner-up denies the certificate as
    well: the case below has thin acceptances whose runner-up is far.)"""
    import bench
    n, twins, iters = 300000, 30000, 5
    rng = np.random.default_rng(77)
    m, d, T = bench.make_icp_pair(n, seed=44)
    src = rng.choice(n, twins, replace=False)
    dst = np.setdiff1d(np.arange(n), src)[:twins]
    off = np.zeros((twins, 3))
    off[np.arange(twins), rng.integers(0, 3, twins)] = rng.uniform(1e-12, 1e-11, twins) * rng.choice([-1.0, 1.0], twins)
    m[dst] = m[src] + off
    model, h1, t1, _ = _check(tdtk, orc, gpu, m, d, iters)
    hc, tc, s, c = _run(tdtk, gpu, model, d, iters, counting=True)
    assert hc == h1 and np.array_equal(tc, t1)
    assert s[3] > 100 and s[3] == c[7], (s, c)
    assert s[0] + s[1] + s[2] == n * iters, s
    pp = _per_pass(tdtk, gpu, model, d, iters)
    assert sum(q[3] for q in pp) == s[3], (pp, s)
    for it in range(1, iters - 1):
        assert pp[it + 1][0] + pp[it + 1][1] <= n - pp[it][3], (it, pp[it], pp[it + 1])


def test_a_thin_acceptance_with_a_far_runner_up_carries_no_certificate(tdtk, orc, gpu):
    """Case 4, second half.  A converging pair (everybody skips from the third pass on) whose model ends at z = 700; 36 probe
    queries stand alone at z = 850, 368 apart (few enough that their 36 pairs of pass 2 do not move the others), and each has ONE model point J that the third pass -- pass 2, the first that reads
    certificates -- sees one ulp inside maxd2 and the passes before it at or beyond the radius.  Pass 2 walks the probe from
    maxd2, accepts J thinly (it improves closest_d2 by 3e-12, less than SearchArgs::tie) and searches it again; nothing else
    is within 100 units, so W, d_hit + m and the runner-up would all admit a certificate of ~25 + m.  It must carry none: pass 3
    skips at most the queries pass 2 did not search a second time -- and, so that this bound says something, everybody else."""
    iters, nq, t, side = 4, 262145, 2, 6
    P = side * side
    rng = np.random.default_rng(104)
    m = rng.uniform(-1000.0, 1000.0, (NM, 3))
    m[:, 2] = rng.uniform(-1000.0, 700.0, NM)
    m[0] = [999.5, 999.5, 990.0]     # (the top of the model's box, wherever the J's are: the sums are taken about its centre)
    D = m[rng.integers(0, NM, nq)] + rng.normal(0.0, 0.01 * SPACING, (nq, 3))
    g = np.linspace(-920.0, 920.0, side)
    D[:P] = np.stack([np.repeat(g, side), np.tile(g, side), np.full(P, 850.0)], axis=1)
    d = _frame(tdtk, D, [1.0, -0.5, 0.3], [0.0004, -0.0003, 0.0005])
    parked = D[:P] + [0.0, 0.0, 100.0]
    probe = tdtk.Scan([0, 0, 0], [0, 0, 0], np.concatenate([m, parked]))
    _, tr0, _, _ = _run(tdtk, gpu, probe, d, iters)
    q = np.empty((t + 1, P, 3))
    cur = d[:P].copy()
    for it in range(t + 1):
        q[it] = cur
        orc.transform_points(tr0[it, 2:], cur)
    J, built = parked.copy(), np.zeros(P, bool)
    for p in range(P):
        for a in range(3):
            for sg in (-1.0, 1.0):
                Jp = q[t, p].copy()
                Jp[a] = np.nextafter(q[t, p, a] + 25.0 * sg, q[t, p, a])
                dd = Jp - q[:, p]
                d2 = dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1] + dd[:, 2] * dd[:, 2]
                if not built[p] and d2[t] < MAXD2 and MAXD2 - d2[t] < 1e-10 and np.all(d2[:t] >= MAXD2):
                    J[p], built[p] = Jp, True
    nb = int(built.sum())
    print("probes with a J one ulp inside maxd2 at pass %d: %d of %d" % (t, nb, P))
    assert nb >= P // 2, nb
    mm = np.concatenate([m, J])
    model, _, trace, ref = _check(tdtk, orc, gpu, mm, d, iters)
    assert np.array_equal(trace[:t], tr0[:t])
    paired = built & (ref[t][2][:P] == NM + np.arange(P))       # pass t pairs a built probe with its J (says the oracle)
    print("of them paired with their J by the oracle:", int(paired.sum()), "others:", ref[t][2][:P][built & ~paired][:8])
    nb = int(paired.sum())
    assert nb == P, (nb, P)          # (measured: every probe gets its J and the oracle pairs all 36; a drift of the probe run shows here)
    for it in range(t):
        assert np.all(ref[it][2][:P] == -1), it
    pp = _per_pass(tdtk, gpu, model, d, iters)
    for it, row in enumerate(pp):
        print("pass %d: skipped with a hit %d, without %d, walked %d, searched again %d" % (it, *row))
    assert pp[t][3] >= nb, (pp[t], nb)
    assert pp[t + 1][0] + pp[t + 1][1] <= nq - pp[t][3], (pp[t], pp[t + 1])
    assert pp[t + 1][0] + pp[t + 1][1] >= nq - 2 * P, pp[t + 1]


def test_queries_without_a_partner(tdtk, orc, gpu):
    """Case 5.  A third of the queries lie 300 .. 3000 units outside the model's box (off the 16-bit grid): -1 in every pass, and
    answered by their certificate from the third pass on.  Three probes Q0..Q2 sit alone in an emptied cube, each with one model
    point that the THIRD pass -- the first that reads certificates -- sees at d2 == maxd2 exactly (no pair: strict `<`), one ulp
    inside (a pair) and one ulp outside, and the passes before it beyond the radius; whatever the fourth pass makes of them is
    the oracle's business."""
    iters, nq, t = 4, 262145, 2
    m, D, rng = _cloud(105, nq, 1.0)
    ce = np.array([[300.0, 300.0, 300.0], [-400.0, 200.0, -300.0], [100.0, -500.0, 400.0]])
    for c in ce:                                      # model points of the cubes go elsewhere, queries of the balls too
        ins = np.flatnonzero(np.all(np.abs(m - c) < 150.0, axis=1))
        m[ins] = rng.uniform(-1000.0, 1000.0, (len(ins), 3)) * [1.0, 1.0, 0.0] + [0.0, 0.0, 950.0]
        near = np.flatnonzero(np.linalg.norm(D - c, axis=1) < 100.0)
        D[near, 0] = -1500.0
    far = rng.permutation(nq)[: nq // 3]
    far = far[far >= 3]
    ax = rng.integers(0, 3, len(far))
    D[far, ax] = rng.choice([-1.0, 1.0], len(far)) * (1000.0 + rng.uniform(300.0, 3000.0, len(far)))
    D[:3] = ce
    J = np.array([np.argmin(np.linalg.norm(m - (c + [800.0, 0, 0]), axis=1)) for c in ce])     # three model points become the J's
    assert len(set(J.tolist())) == 3
    d = _frame(tdtk, D, [1.0, -0.5, 0.3], [0.0004, -0.0003, 0.0005])

    def build(trace):
        mm = m.copy()
        mm[J] = ce + [120.0, 0.0, 0.0]                # parked: pairs with nobody
        if trace is None:
            return mm
        q = np.empty((iters, 3, 3))
        cur = d[:3].copy()
        for it in range(iters):
            q[it] = cur
            orc.transform_points(trace[it, 2:], cur)
        k = t
        q = q[:t + 1]
        for p, want in enumerate(("eq", "lt", "gt")):
            done = False
            for a in range(3):
                for s in (-1.0, 1.0):
                    Jp = q[k, p].copy()
                    Jp[a] = q[k, p, a] + 25.0 * s
                    if want != "eq":
                        Jp[a] = np.nextafter(Jp[a], q[k, p, a] if want == "lt" else Jp[a] + s)
                    dd = Jp - q[:, p]
                    d2 = dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1] + dd[:, 2] * dd[:, 2]
                    ok = {"eq": d2[k] == MAXD2, "lt": d2[k] < MAXD2, "gt": d2[k] > MAXD2}[want]
                    if ok and np.all(d2[:k] >= MAXD2) and not done:
                        mm[J[p]] = Jp
                        done = True
            assert done, (p, want)
        return mm

    probe = tdtk.Scan([0, 0, 0], [0, 0, 0], build(None))
    _, tr0, _, _ = _run(tdtk, gpu, probe, d, iters)
    mm = build(tr0)
    model, _, trace, ref = _check(tdtk, orc, gpu, mm, d, iters)
    assert np.array_equal(trace[:t], tr0[:t])          # the J's pair with nobody before pass t: the probes are where they were built for
    at = ref[t][2]
    assert at[0] == -1 and at[1] == J[1] and at[2] == -1, at[:3]
    for it in range(t):
        assert np.all(ref[it][2][:3] == -1), it
    for it in range(iters):
        assert np.all(ref[it][2][far] == -1), it
    pp = _per_pass(tdtk, gpu, model, d, iters)
    for it, (skh, skn, walked, _) in enumerate(pp):
        assert skh + skn + walked == nq, (it, pp[it])
        if it >= 2:
            assert skn >= len(far), (it, skn, len(far))


def test_a_runner_up_inside_the_margin_takes_over_when_the_oracle_says(tdtk, orc, gpu):
    """Case 6.  A probe run over case 1's kind of cloud says where 4 000 queries with a hit are at passes 3 and 4, how far their
    hit is (d) and how far they moved (delta).  Each gets an extra model point E straight ahead of its motion at d + m / 2 from
    its position at pass 3, m = clamp(kappa delta, d / 64, d / 4): the runner-up inside the margin of pass 3's walk.  The query
    keeps moving towards E by units per pass, so E becomes the nearest a pass or two later: the hand-over happens in the
    iteration the oracle says (every iteration's indices are the oracle's), for at least a quarter of them on passes 4 .. 7."""
    iters, nq, k = 8, 300001, 4000
    m, D, rng = _cloud(106, nq, 1.0, half=400.0)
    d = _frame(tdtk, D, [10.0, -5.0, 3.0], [0.02, -0.03, 0.05])
    probe = tdtk.Scan([0, 0, 0], [0, 0, 0], m)
    _, tr0, _, _ = _run(tdtk, gpu, probe, d, iters)
    r0 = _oracle(orc, m, d, tr0[:5])
    ok = np.flatnonzero((r0[3][2] >= 0) & (r0[4][2] >= 0))
    S = rng.choice(ok, k, replace=False)
    q3, q4 = r0[3][3][S], r0[4][3][S]
    dh = np.linalg.norm(m[r0[3][2][S]] - q3, axis=1)
    delta = np.linalg.norm(q4 - q3, axis=1)
    mg = np.clip(KAPPA * delta, M_LO * dh, M_HI * dh)
    extra = q3 + (q4 - q3) / delta[:, None] * (dh + 0.5 * mg)[:, None]
    mm = np.concatenate([m, extra])
    _, _, _, ref = _check(tdtk, orc, gpu, mm, d, iters)
    took = np.zeros(k, bool)
    for it in range(4, iters):
        now, before = ref[it][2][S], ref[it - 1][2][S]
        took |= (now >= NM) & (before >= 0) & (before < NM)
    print("hand-overs on passes 4 .. 7:", int(took.sum()), "of", k)
    assert int(took.sum()) > k // 4, int(took.sum())


_CHILD = r"""
import importlib, os, sys
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "tests"))
import test_gpu_cert_skip as T
tdtk = importlib.import_module("3dtk_amd")
m, _, _ = T._cloud(107, 262145, 1.0)
model = tdtk.Scan([0, 0, 0], [0, 0, 0], m)
seed, dev = int(sys.argv[1]), int(sys.argv[2])
h, t, _, _ = T._run(tdtk, dev, model, T._scan_for(tdtk, m, seed), 3)
print(seed, " ".join("%%x" %% x for x in h), t.tobytes().hex())
"""


def _scan_for(tdtk, m, seed):
    """The data of the child process above for `seed`: points of the model m + noise, in the frame of a small pose."""
    D = m[np.random.default_rng(seed).integers(0, len(m), 262145)] + np.random.default_rng(seed + 1).normal(0, 1, (262145, 3))
    return _frame(tdtk, D, [3.0, -2.0, 1.0], [0.004, -0.003, 0.005])


def test_no_certificate_outlives_its_loop(tdtk, orc, gpu):
    """Case 7.  Match (A, B) for three iterations, then (A, C) with len(C) == len(B), then (A, B) again in this process: each
    equals what a fresh process gets for that pair.  And a -R 3 loop skips nobody and equals the loop without certificates."""
    m, _, _ = _cloud(107, 262145, 1.0)
    model = tdtk.Scan([0, 0, 0], [0, 0, 0], m)
    B, Cc = _scan_for(tdtk, m, 201), _scan_for(tdtk, m, 202)
    here = [_run(tdtk, gpu, model, x, 3) for x in (B, Cc, B)]
    fresh = {}
    for seed in (201, 202):          # one fresh process per pair
        out = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, ROOT), str(seed), str(gpu)], capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        w = [l.split() for l in out.stdout.splitlines() if l.startswith(str(seed) + " ")]
        assert len(w) == 1 and len(w[0]) == 5, out.stdout[-500:]
        fresh[seed] = ([int(x, 16) for x in w[0][1:4]], w[0][4])
    for (h, t, _, _), seed in zip(here, (201, 202, 201)):
        assert h == fresh[seed][0], seed
        assert t.tobytes().hex() == fresh[seed][1], seed
    libc = C.CDLL(None)
    libc.srand(4711)                 # (the keep-masks are std::rand() draws: the same ones for both loops)
    h1, t1, s1, _ = _run(tdtk, gpu, model, B, 5, cert=True, counting=True, rnd=3)
    libc.srand(4711)
    h0, t0, _, _ = _run(tdtk, gpu, model, B, 5, cert=False, counting=True, rnd=3)
    assert s1[0] == 0 and s1[1] == 0, s1
    assert h1 == h0 and np.array_equal(t1, t0)
