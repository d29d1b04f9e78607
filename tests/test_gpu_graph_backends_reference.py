"""The graph back-ends on the device against the reference's compiled sources (k16_graph_backends.npz) and the
extended-precision blocks of pair_sums_ref.py: the GPU tier of test_graph_backends_reference_host.py.

Per-link blocks.  tdtk_graph_link_blocks per back-end and link case: the pairing equals the oracle's index for index (whose
pair list has the SHA-256 the reference's had), every block is inside the LIBRARY form's derived tolerance of the
REFERENCE form's extended-precision value -- the same value the fixture's block lies within its own tolerance of -- that
tolerance is at most a tenth of what one pair less changes, blocks that must be zero are exactly zero, a second call
returns the same bits.  Each case prints `graph-blocks <back-end> <case> worst |error| / tolerance`.

What cannot be asserted.  The library takes the lum back-ends' ss from the normal equations,
(sum - D . MZ) / (2m - 3): a difference of two numbers of size m |offset|^2 whose rounding is gamma(m) of that size, while ss
itself is the alignment noise squared.  On the links of SS_UNRESOLVED the derived tolerance of ss, and of C = MM / ss and
CD = MZ / ss with it, is wider than a tenth of what one pair less changes; there the blocks are still inside it, the
discrimination requirement is asserted to FAIL (so that the list cannot go stale), and MM = C ss and MZ = CD ss, which do not
depend on ss, are asserted with the full requirement.  The reference's second pass over the residuals has no such loss
near the origin (asserted for noise1e-6); a second accumulation pass in the search kernels is what would remove it.

Whole rounds.  doGraphSlam6D through the Python classes with resident scans, nrIt 1 and 2, on every graph.  nrIt = 1 against
the fixture at  tol_1 = ||J|| (tol_X + ||A^-1|| (||dr|| + ||dA|| ||X||)) + floor  (the CPU tier's tolerance with the
blocks' own, dA and dr being the scatter of |library tolerance| + |reference tolerance| of every link's block).  The second
iteration starts from poses that differ by up to tol_1, and pairing is not a continuous function of them; so nrIt = 2 is
compared (a) with the pinned restatement's second iteration started from the library's own first, at the same kind of
tolerance tol_2, and (b) with the fixture at  tol_2 + ||J_12|| tol_1,  J_12 the Jacobian of the restatement's whole second
iteration with respect to the six pose parameters of every scan it starts from, by central differences."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import graph_backend_cases as gc
import pair_sums_ref as R
import test_graph_backends_reference_host as H

pytestmark = pytest.mark.gpu
LD = R.LD
U = R.U
mg = H.mg
fx = H.fx

# lum back-ends: links on which the normal-equation ss cannot tell one pair more or less (see above)
SS_UNRESOLVED = {1: ("noise1e-6", "far_pairs3", "far_noise1", "far_noise1e-3", "far_noise1e-6"),
                 2: ("noise1e-6", "far_pairs3", "far_noise1", "far_noise1e-3", "far_noise1e-6")}

_links = {}


def device_link(tdtk, orc, fx, case):
    """the case's two resident scans, the oracle's pairs, the accumulation point; the device's pairing is checked once"""
    if case not in _links:
        p1, p2, a, b, maxd, model = H.link_pairs(orc, fx, case)
        from oracle import icp_oracle as io
        _, data, _ = gc.link_case(case)
        first = tdtk.Scan([0, 0, 0], [0, 0, 0], model)
        second = tdtk.Scan([0, 0, 0], [0, 0, 0], data)
        got = tdtk.Scan.getPtPairs(first, second, max_dist_match2=maxd * maxd, want_idx=True)
        ref = io.get_pt_pairs(a, b, maxd * maxd)
        assert got["n"] == len(p1) == int(fx["link_%s_n" % case])                 # pair counts are exact
        assert np.array_equal(got["idx"], ref["idx"])
        shift = R.shift_of(np.array(first.xyz_reduced_original), np.array(first.dalignxf, float))
        _links[case] = (first, second, p1, p2, maxd, shift)
    return _links[case]


def link_blocks(tdtk, k, first, second, maxd):
    capi = import_module("3dtk_amd._capi")
    Bn = capi.lib().tdtk_graph_block_doubles(k)
    fh = (C.c_void_p * 1)(first.getSearchTree()._h); sh = (C.c_void_p * 1)(second.handle)
    dal = np.ascontiguousarray(np.array(first.dalignxf, float).reshape(1, 16))
    out = np.full((1, Bn), np.nan)
    capi.check(capi.lib().tdtk_graph_link_blocks(k, 1, fh, capi.dptr(dal), sh, float(maxd) * float(maxd), capi.dptr(out)))
    return out[0]


def euler_link_lib(p1, p2, shift=None, drop=None, full=None):
    """LIBRARY form of back-end 1: pair_sums_ref.lum_link (tdtk_lum_links), as a Link"""
    p1, p2 = R._keep(p1, p2, drop)
    m, MM, MZ, ss = R.lum_link(p1, p2)
    L = R.Link(m)
    if MM is None:
        return L
    L.ss = ss
    L.q["MM"], L.q["MZ"] = MM, MZ
    if ss.v >= 0.0000000000001:
        L.q["C"] = [v / ss for v in MM]; L.q["CD"] = [v / ss for v in MZ]
    return L


LIB_LINK = dict(R.LIB_LINK)
LIB_LINK[1] = euler_link_lib
# the library's block as {name: values} per back-end
LIB_LAYOUT = {1: {"C": slice(0, 36), "CD": slice(36, 42)}, 2: {"C": slice(0, 49), "CD": slice(49, 56)},
              3: {"Blk": slice(1, 37), "bd1": slice(37, 43)},
              4: {"cm": slice(1, 4), "cd": slice(4, 7), "MkMkt": slice(7, 16), "DkDkt": slice(16, 25), "MkDkt": slice(25, 34),
                  "DkMkt": slice(34, 43), "Ak1": slice(43, 46), "Ak2": slice(46, 49)}}


def check_block(case, k, got, lib, ref, disc, unresolved=()):
    """got {name: values} inside the library tolerance of the reference form's values; disc(name) -> one pair less / tolerance"""
    worst = 0.0
    for name, val in got.items():
        v, t = ref.values(name), lib.tols(name)
        assert np.all(np.isfinite(val)), (case, k, name)
        err = np.abs(np.asarray(val, LD).ravel() - v)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(t > 0, err / np.where(t > 0, t, 1), np.where(err > 0, np.inf, 0.0)).astype(float)
        worst = max(worst, float(r.max()))
        assert np.all(r <= 1.0), (case, k, name, float(r.max()))
        d = disc(name)
        if d is None:
            continue
        if name in unresolved:
            assert d < 10.0, (case, k, name, "SS_UNRESOLVED is out of date: one pair less moves it by %.3g tolerances" % d)
        else:
            assert d >= 10.0, (case, k, name, "one pair less moves it by only %.3g tolerances" % d)
    return worst


@pytest.mark.parametrize("backend", gc.BACKENDS)
@pytest.mark.parametrize("case", gc.LINK_CASES)
def test_link_blocks(tdtk, orc, gpu, fx, case, backend):
    k = backend
    first, second, p1, p2, maxd, shift = device_link(tdtk, orc, fx, case)
    n = len(p1)
    blk = link_blocks(tdtk, k, first, second, maxd)
    assert np.array_equal(link_blocks(tdtk, k, first, second, maxd), blk), "a second call returns the same bits"
    fixture = fx["link_%s_b%d" % (case, k)]
    aligned = case.endswith("aligned")
    if n < gc.MIN_PAIRS[k] or (aligned and k <= 2):
        # under the back-end's threshold, or ss == 0 exactly: a zero block (gapx6D: but for the centroids, which feed the
        # translation system of every link)
        if k == 4:
            assert not np.any(blk[0:1]) and not np.any(blk[7:])
            ref = R.gapx_link(p1, p2); lib = R.gapx_link_lib(p1, p2, shift)
            check_block(case, k, {"cm": blk[1:4], "cd": blk[4:7]}, lib, ref, lambda name: None)
        else:
            assert not np.any(blk), (case, k)
        if aligned and k == 2:
            # the library's deliberate departure: the reference divides by ss == 0 here
            assert not np.all(np.isfinite(fixture[mg.LINK_LAYOUT[2]["C"]]))
        return
    ref = R.REF_LINK[k](p1, p2)
    lib = LIB_LINK[k](p1, p2, shift)
    got = {name: blk[sl] for name, sl in LIB_LAYOUT[k].items()}
    if k == 3:
        assert blk[0] == 1.0
    if k == 4:
        assert blk[0] == 1.0

    def disc(name):
        if n - 1 < gc.MIN_PAIRS[k] or (n == 1 and name not in ("cm", "cd")):
            return None
        if aligned and name in ("bd1", "Ak1", "Ak2"):
            return None                  # the value is exactly zero with and without the pair: nothing to tell apart
        less = LIB_LINK[k](p1, p2, shift, drop=n // 2)
        move = np.abs(less.values(name) - lib.values(name)); t = lib.tols(name)
        moved = move > 0
        with np.errstate(divide="ignore"):
            return float(np.min(np.where(t[moved] > 0, move[moved] / np.where(t[moved] > 0, t[moved], 1), np.inf))) if moved.any() else None
    unresolved = ("C", "CD") if (k <= 2 and case in SS_UNRESOLVED[k]) else ()
    if k <= 2 and not np.any(blk):
        # the normal-equation ss came out under the guard (ss < 1e-13, api_links.cpp / api_graph.cpp) and the library handed out a zero block where
        # the reference uses the link.  Admissible only where ss is unresolved and its tolerance reaches down to the guard
        assert unresolved and float(ref.ss.v - lib.ss.e) < 0.0000000000001, (case, k, float(ref.ss.v), float(lib.ss.e))
        print("graph-blocks %-10s %-14s ZERO BLOCK: ss = %.3g is inside its tolerance %.3g of the guard  (n = %d)"
              % (gc.NAMES[k], case, float(ref.ss.v), float(lib.ss.e), n))
        return
    worst = check_block(case, k, got, lib, ref, disc, unresolved)
    # the fixture's reference block inside its own tolerance of the same values
    for name, sl in mg.LINK_LAYOUT[k].items():
        if name in ref.q:
            assert np.all(H.ratios(fixture[sl], ref, name) <= 1.0), (case, k, name, "reference")
    if k <= 2:
        # MM = C ss and MZ = CD ss with the library's own ss = m / C[0][0]: what of the block does not depend on ss.  C = fl(MM /
        # ss), ss_hat = fl(m / C00) and the product: four roundings on top of the sum's tolerance
        w = 6 if k == 1 else 7
        ss_hat = LD(n) / LD(blk[0])
        back = {"MM": np.asarray(blk[:w * w], LD) * ss_hat, "MZ": np.asarray(blk[w * w:], LD) * ss_hat}
        for name, val in back.items():
            v, t = ref.values(name), lib.tols(name) + 4 * U * np.abs(ref.values(name))
            assert np.all(np.abs(val - v) <= t), (case, k, name)
            d = disc(name)
            assert d is None or d >= 10.0, (case, k, name, d)
        e_ss = abs(ss_hat - ref.ss.v)
        assert e_ss <= lib.ss.e + 2 * U * abs(ref.ss.v), (case, k, "ss", float(e_ss), float(lib.ss.e))
        if case == "noise1e-6":
            # the loss is the form's: the reference's residual pass resolves the same link
            assert H.discrimination(R.REF_LINK[k], p1, p2, "C") >= 10.0
    print("graph-blocks %-10s %-14s worst |error| / tolerance = %.3g  (n = %d%s)"
          % (gc.NAMES[k], case, worst, n, ", C and CD unresolved" if unresolved else ""))


def test_ghelix_still_refuses_a_link_ending_at_scan_0(tdtk, gpu):
    capi = import_module("3dtk_amd._capi")
    n = 2
    blocks = np.zeros((1, 43)); blocks[0, 0] = 1.0; blocks[0, 1:37] = np.eye(6).ravel()
    frm = np.array([1], np.int32); to = np.array([0], np.int32)
    tm = np.tile(np.eye(4).reshape(16), (3, 1)); da = tm.copy(); rp = np.zeros((3, 3)); rt = np.zeros((3, 3))
    state = np.zeros((6 * n) ** 2 + 6 * n)
    rc = capi.lib().tdtk_graph_solve_update(3, 1, capi.iptr(frm), capi.iptr(to), capi.dptr(blocks), 3, capi.dptr(tm), capi.dptr(da),
                                            capi.dptr(rp), capi.dptr(rt), None, capi.dptr(state), None, None)
    assert rc != 0


# ---- whole rounds -------------------------------------------------------------------------------------------------------
def oracle_scans(io, g):
    return [io.OScan(g.rPos[i], g.rPosTheta[i], g.points[i]) for i in range(g.nscans)]


def restated_iteration(io, k, links, scans, maxd2, state):
    if k == 1:
        return io.lum_iteration(links, scans, maxd2)[0], None
    if k == 2:
        return io.lumquat_iteration(links, scans, maxd2)[0], None
    if k == 3:
        ret, B, bd, _ = io.ghelix_iteration(links, scans, maxd2, *(state or (None, None)))
        return ret, (B, bd)
    ret, state, _ = io.gapx_iteration(links, scans, maxd2, state)
    return ret, state


def copy_state(k, state):
    if state is None:
        return None
    if k == 3:
        return (state[0].copy(), state[1].copy())
    return state.copy()


def scans_poses(scans):
    return np.array([np.concatenate([s.transMat, s.dalignxf, s.rPos, s.rPosTheta]) for s in scans])


def block_term(io, k, links, scans, maxd2, case, carried=None):
    """||A^-1|| (||dr|| + ||dA||_F ||X||) with dA, dr the scatter of every link's |library tolerance| + |reference tolerance|
    (ghelix6DQ2 / gapx6D: plus what the carried system already holds); gapx6D: and ||Bt^-1|| ||dAt|| for the translations.
    -> (term for X, term for the poses, (dA, dr) to carry)"""
    w = {1: 6, 2: 7, 3: 6, 4: 3}[k]
    N = w * (len(scans) - 1)
    dA = np.zeros((N, N)) if carried is None else carried[0].copy()
    dr = np.zeros(N) if carried is None else carried[1].copy()
    dAt = 0.0
    for (f, t) in links:
        r = io.get_pt_pairs(scans[f], scans[t], maxd2)
        p1, p2 = r["p1"][:r["n"]], r["p2"][:r["n"]]
        if k == 4 and r["n"]:
            # the translation system's right hand side takes Ak1 = R(x_f) cm - R(x_t) cd of every link, one pair or many.
            # cm and cd differ between library and reference by at most the two forms' tolerances (their 1-norm bounds the
            # 2-norm); R(x) = I + [x]_x (icp6D_APX::computeRt) has ||R||_2 = sqrt(1 + |x|^2); either side's own product and
            # subtraction are 3 multiplications, 2 additions and 1 subtraction an entry, gamma(6) of ||R|| (|cm|_1 + |cd|_1);
            # and Ak1 goes into two rows (- at f, + at t), so into the norm of the right hand side at most sqrt(2) times.
            cen = R.centroids(p1, p2)
            lcen = LIB_LINK[4](p1, p2, R.shift_of(scans[f].xyz_orig, scans[f].dalignxf))
            e_in = float(sum(x.e for x in cen[0] + cen[1])) + float(lcen.tols("cm").sum() + lcen.tols("cd").sum())
            size = float(sum(abs(x.v) for x in cen[0] + cen[1]))
            rot = float(np.sqrt(1.0 + max(float(x @ x) for x in np.asarray(case.X, float).reshape(-1, 3))))
            dAt += float(np.sqrt(2.0)) * rot * (e_in + 2.0 * float(R.gamma(6)) * size)
        if r["n"] < gc.MIN_PAIRS[k]:
            continue
        model = scans[f].xyz_orig
        shift = R.shift_of(model, scans[f].dalignxf)
        lib, ref = LIB_LINK[k](p1, p2, shift), R.REF_LINK[k](p1, p2)

        def tol(name):
            return (lib.tols(name) + ref.tols(name)).astype(float)
        a, c = (f - 1) * w, (t - 1) * w
        if k <= 2:
            Cm, CD = tol("C").reshape(w, w), tol("CD")
            for s in ([a] if f else []) + [c]:
                dA[s:s + w, s:s + w] += Cm; dr[s:s + w] += CD
            if f:
                dA[a:a + w, c:c + w] += Cm; dA[c:c + w, a:a + w] += Cm
        elif k == 3:
            Bm = tol("Blk").reshape(6, 6)
            bd = np.maximum(tol("bd1"), (lib.tols("bd1") + ref.tols("bd2")).astype(float))
            for s in ([a] if f else []) + [c]:
                dA[s:s + 6, s:s + 6] += Bm; dr[s:s + 6] += bd
            if f:
                dA[a:a + 6, c:c + 6] += Bm; dA[c:c + 6, a:a + 6] += Bm
        else:
            if f:
                dr[a:a + 3] += tol("Ak1"); dA[a:a + 3, a:a + 3] += tol("MkMkt").reshape(3, 3)
                dA[a:a + 3, c:c + 3] += tol("DkMkt").reshape(3, 3); dA[c:c + 3, a:a + 3] += tol("MkDkt").reshape(3, 3)
            dr[c:c + 3] += tol("Ak2"); dA[c:c + 3, c:c + 3] += tol("DkDkt").reshape(3, 3)
    x_term = case.S_inv_norm * (float(np.linalg.norm(dr)) + float(np.linalg.norm(dA)) * float(np.linalg.norm(case.X)))
    pose_term = 0.0
    if k == 4:
        n = len(scans) - 1
        Bt = np.zeros((n, n))
        for (f, t) in links:
            if f:
                Bt[f - 1, f - 1] += 1; Bt[f - 1, t - 1] -= 1; Bt[t - 1, f - 1] -= 1
            Bt[t - 1, t - 1] += 1
        pose_term = float(np.linalg.norm(np.linalg.inv(Bt), 2)) * dAt
    return x_term, pose_term, ((dA, dr) if k >= 3 else None)


def restated_fixture(io, g, k):
    """what the fixture would hold for lum6DQuat on graph g, from the restatement (the one case the reference cannot run)"""
    assert k == 2
    key = "graph_%s_b%d_" % (g.name, k)
    links, maxd2 = g.links(k), g.maxd * g.maxd
    O = oracle_scans(io, g)
    z = {}
    for it in (1, 2):
        blocks = np.zeros((len(links), 56)); npairs = np.zeros(len(links), np.int64)
        for l, (f, t) in enumerate(links):
            Cm, CD, m, _ = io.covariance_quat(O[f], O[t], maxd2)
            blocks[l, :49], blocks[l, 49:], npairs[l] = Cm.ravel(), CD, m
        ret, Gm, B, X = io.lumquat_iteration(links, O, maxd2)
        z[key + "blocks_it%d" % it], z[key + "npairs_it%d" % it] = blocks, npairs
        z[key + "it%d_A" % it], z[key + "it%d_rhs" % it], z[key + "it%d_X" % it] = H.dropped(Gm), B, X
        z[key + "poses%d" % it], z[key + "ret%d" % it] = scans_poses(O), ret
    return z


def library_round(tdtk, g, k, nrIt):
    cls = {1: tdtk.lum6DEuler, 2: tdtk.lum6DQuat, 3: tdtk.ghelix6DQ2, 4: tdtk.gapx6D}[k]
    S = [tdtk.Scan(g.rPos[i], g.rPosTheta[i], g.points[i]) for i in range(g.nscans)]
    gr = tdtk.Graph(g.nscans, links=g.links(k))
    gr.nrScans = g.nscans
    ret = cls(None, g.maxd, g.maxd, epsilonLUM=-1.0).doGraphSlam6D(gr, S, nrIt)
    poses = np.array([np.concatenate([np.asarray(s.transMat, float), np.asarray(s.dalignxf, float), np.asarray(s.rPos, float),
                                      np.asarray(s.rPosTheta, float)]) for s in S])
    for s in S:
        s.release()
    return poses, float(ret)


@pytest.mark.parametrize("graph,backend", H.GRAPH_CASES)
def test_whole_rounds(tdtk, orc, gpu, fx, graph, backend):
    from oracle import icp_oracle as io
    k = backend
    g = gc.graph(graph)
    links, maxd2 = g.links(k), g.maxd * g.maxd
    l1, lret1 = library_round(tdtk, g, k, 1)
    l2, lret2 = library_round(tdtk, g, k, 2)
    assert np.array_equal(library_round(tdtk, g, k, 2)[0], l2), "a second run returns the same bits"
    pinned = (graph, k) != ("few_pairs", 2)
    if pinned:
        c1, c2 = H.case_of(fx, graph, k, 1), H.case_of(fx, graph, k, 2)
    else:
        # the reference cannot run this one (its FillGB3D throws on the link of 2 pairs); the library skips the link, and so
        # does the restatement: its two iterations stand in for the fixture's, tolerances derived the same way
        fake = restated_fixture(io, g, k)
        c1, c2 = H.Case(io, fake, graph, k, 1), H.Case(io, fake, graph, k, 2)
    # iteration 1 against the fixture
    O = oracle_scans(io, g)
    x1, p1, carried = block_term(io, k, links, O, maxd2, c1)
    tol1 = c1.tol_pose(x1) + p1
    err1 = float(np.linalg.norm(H.pose_vector(l1) - H.pose_vector(c1.poses)))
    assert err1 <= tol1, (graph, k, 1, err1, tol1)
    assert abs(lret1 - c1.ret) <= tol1
    # iteration 2: the restatement from the library's own first iteration
    _, state = restated_iteration(io, k, links, O, maxd2, None)

    def second(start_poses):
        """the restatement's second iteration from the poses [scan][38] -> poses after, ret"""
        Q = oracle_scans(io, g)
        for i in range(1, g.nscans):
            Q[i].transformToEuler(start_poses[i, 32:35].copy(), start_poses[i, 35:38].copy())
        ret, _ = restated_iteration(io, k, links, Q, maxd2, copy_state(k, state))
        return Q, ret
    Q = oracle_scans(io, g)
    for i in range(1, g.nscans):
        Q[i].transformToEuler(l1[i, 32:35].copy(), l1[i, 35:38].copy())
    x2, p2, _ = block_term(io, k, links, Q, maxd2, c2, carried)
    tol2 = c2.tol_pose(x2) + p2
    Q, rret2 = second(l1)
    err2 = float(np.linalg.norm(H.pose_vector(l2) - H.pose_vector(scans_poses(Q))))
    assert err2 <= tol2, (graph, k, 2, err2, tol2)
    assert abs(lret2 - rret2) <= tol2
    if not pinned:
        print("graph-rounds %-10s %-15s (restatement only) nrIt 1: |pose error| %.3g  tol %.3g   nrIt 2: %.3g  tol %.3g"
              % (gc.NAMES[k], graph, err1, tol1, err2, tol2))
        return
    # iteration 2 against the fixture: + ||J_12|| tol_1
    npar = 6 * (g.nscans - 1)
    J = np.zeros((len(H.pose_vector(l2)), npar))
    for j in range(npar):
        i, a = 1 + j // 6, 32 + j % 6
        h = 1e-7 * max(1.0, abs(float(l1[i, a])))
        up, dn = l1.copy(), l1.copy()
        up[i, a] += h; dn[i, a] -= h
        J[:, j] = (H.pose_vector(scans_poses(second(up)[0])) - H.pose_vector(scans_poses(second(dn)[0]))) / (2 * h)
    J12 = float(np.linalg.norm(J, 2))
    tolf = tol2 + J12 * tol1
    errf = float(np.linalg.norm(H.pose_vector(l2) - H.pose_vector(c2.poses)))
    print("graph-rounds %-10s %-15s nrIt 1: |pose error| %.3g  tol %.3g   nrIt 2: against the restatement %.3g  tol %.3g, "
          "against the fixture %.3g  tol %.3g  (||J_12|| %.3g)" % (gc.NAMES[k], graph, err1, tol1, err2, tol2, errf, tolf, J12))
    assert errf <= tolf, (graph, k, errf, tolf)
    assert abs(lret2 - c2.ret) <= tolf
