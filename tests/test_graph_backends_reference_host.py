"""The graph back-ends (lum6DEuler -G 1, lum6DQuat -G 2, ghelix6DQ2 -G 3, gapx6D -G 4) against the reference's own compiled
sources: the CPU tier.  k16_graph_backends.npz holds what lum6Deuler.cc, lum6Dquat.cc, ghelix6DQ2.cc, gapx6D.cc and
graphSlam6D.cc compute on the link cases and graphs of graph_backend_cases.py (tests/golden/make_golden_graph_backends.py
says how).  Here
  * the live reference, where the checkout is present, equals the fixture bit for bit;
  * every per-link block of the reference, and of oracle/icp_oracle.py's restatement, lies within the reference's derived
    tolerance of the extended-precision value (pair_sums_ref.py), and that tolerance is at most a tenth of what leaving
    one pair out changes -- a wrong sign or index is off by the size of the quantity;
  * the restated scatter rules, applied to the reference's blocks, give the matrix and right hand side cs_cholsol was handed;
  * tdtk_graph_solve_update, fed the reference's blocks (no GPU: scans = NULL), reproduces the reference's poses and return
    value of every iteration inside a tolerance derived from the conditioning of the solve;
  * every scatter rule is seen to matter: with the rule switched off the restatement's poses move by at least ten times
    that tolerance on the graph built for it.

The tolerances of the solve comparison.  Both sides solve the same dropped symmetric matrix A (n x n, the upper triangle) by
a Cholesky factorisation; each computed solution is the exact one of a matrix within n gamma(3n+1) ||A|| of A (Higham,
Accuracy and Stability, 10.4 and 10.7), and the library's scatter adds its L links into an entry with at most L roundings.
So  ||X_lib - X_ref|| <= tol_X = 2 cond_2(A) (n gamma(3n+1) + L u) ||X||,  to which ghelix6DQ2 adds ||A^-1|| ||bd2 + bd1||:
the library scatters -bd1 where the reference sums a bd2 of its own, and the fixture has both.  The poses follow with the
Jacobian J of the (pinned) restatement's pose update, taken by central differences:  tol_pose = ||J||_2 tol_X +
gamma(64) max(1, |pose|_inf) for the update's own roundings.  The longest chain of them is lum6DEuler's: the new pose from
X and the old one (Ha^-1 X subtracted from it: Ha is 6 x 6, unit but for a 2 x 2 block of determinant -cos(ty), and its
product is of the size of X, not of the pose: 10 roundings of the pose cover it), then transformToEuler: M4inv (an entry
is a sum of 6 products of 3 over a determinant of 4 such sums: at most 7 + 10 + 1 = 18), the product with transMat (4
multiplications, 3 additions: 4 deep), EulerToMatrix4 (a sine or cosine, then at most 3 multiplications and 1 addition: 6),
the second product (4) and Matrix4ToEuler (an atan2 or asin of a quotient: 4).  That is 10 + 18 + 4 + 6 + 4 + 4 = 46 in a
row, each relative to entries of size at most max(1, |pose|_inf); 64 is the next power of two above the count.
DESIGN section 7 records the printed figures."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import graph_backend_cases as gc
import pair_sums_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
LD = R.LD
U = float(R.U)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(G, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


mg = _load("make_golden_graph_backends")
GRAPH_CASES = [(g, k) for g in gc.GRAPHS for k in gc.BACKENDS]


@pytest.fixture(scope="module")
def fx():
    return mg.load()


@pytest.fixture(scope="module")
def ref():
    if not mg.have_ref():
        pytest.skip("no reference checkout (src/slam6d/lum6Dquat.cc)")
    mg.ref_lib()
    return mg.Ref


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the live reference against the fixture -----------------------------------------------------------------------------
def test_fixture_holds_all_cases_and_nothing_else(fx):
    assert os.path.getsize(mg.OUT) <= mg.MAX_BYTES
    want = set()
    for c in gc.LINK_CASES:
        want |= {"link_%s_n" % c, "link_%s_sha" % c} | {"link_%s_b%d" % (c, k) for k in gc.BACKENDS}
    for g, k in GRAPH_CASES:
        key = "graph_%s_b%d_" % (g, k)
        want |= {key + "status", key + "blocks_it1", key + "npairs_it1"}
        if int(fx[key + "status"]) == 0:
            want |= {key + s for s in ("ret1", "ret2", "poses1", "poses2", "blocks_it2", "npairs_it2")}
            want |= {key + "it%d_%s" % (j, s) for j in (1, 2) for s in ("A", "rhs", "X")}
    assert set(fx) == want
    # the one (graph, back-end) the reference cannot run: lum6DQuat with a link of fewer than 3 pairs
    assert [gk for gk in GRAPH_CASES if int(fx["graph_%s_b%d_status" % gk]) != 0] == [("few_pairs", 2)]
    for c in gc.LINK_CASES:
        n = gc.link_pairs_expected(c)
        assert n is None or int(fx["link_%s_n" % c]) == n


@pytest.mark.parametrize("case", gc.LINK_CASES)
def test_live_reference_equals_fixture_links(fx, ref, case):
    z = mg.compute_link(case)
    for k, v in z.items():
        assert _same(v, fx[k]), k


@pytest.mark.parametrize("graph,backend", GRAPH_CASES)
def test_live_reference_equals_fixture_graphs(fx, ref, graph, backend):
    z = mg.compute_graph(graph, backend)
    assert set(z) == {k for k in fx if k.startswith("graph_%s_b%d_" % (graph, backend))}
    for k, v in z.items():
        assert _same(v, fx[k]), k


# ---- per-link blocks: reference and restatement against the extended-precision form -----------------------------------
_pairs = {}


def link_pairs(orc_mod, fx, case):
    """the case's pair list from the oracle's tree (pinned to the reference's bit for bit by test_oracle_vs_ref.py); its
    SHA-256 is the one the reference's own pair list had when the fixture was made"""
    if case not in _pairs:
        from oracle import icp_oracle as io
        model, data, maxd = gc.link_case(case)
        a, b = io.OScan([0, 0, 0], [0, 0, 0], model), io.OScan([0, 0, 0], [0, 0, 0], data)
        r = io.get_pt_pairs(a, b, maxd * maxd)
        p1, p2 = np.ascontiguousarray(r["p1"][:r["n"]]), np.ascontiguousarray(r["p2"][:r["n"]])
        assert np.array_equal(mg.pair_sha(p1, p2), fx["link_%s_sha" % case]), case
        assert len(p1) == int(fx["link_%s_n" % case])
        _pairs[case] = (p1, p2, a, b, maxd, model)
    return _pairs[case]


def ratios(got, L, name):
    """|got - value| / tolerance per entry (inf where the tolerance is 0 and the entry is off)"""
    v, t = L.values(name), L.tols(name)
    err = np.abs(np.asarray(got, LD).ravel() - v)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(t > 0, err / np.where(t > 0, t, 1), np.where(err > 0, np.inf, 0.0)).astype(float)


def discrimination(form, p1, p2, name, *args):
    """min over the entries that move of |move| / tolerance when the middle pair is left out"""
    full, less = form(p1, p2, *args), form(p1, p2, *args, drop=len(p1) // 2)
    if name not in less.q:
        return np.inf
    move = np.abs(less.values(name) - full.values(name)); t = full.tols(name)
    moved = move > 0
    if not moved.any():
        return np.inf
    with np.errstate(divide="ignore"):
        return float(np.min(np.where(t[moved] > 0, move[moved] / np.where(t[moved] > 0, t[moved], 1), np.inf)))


# where the reference's own tolerance for C = MM / ss cannot tell one pair more or less: 1e6 from the origin the translation
# and rotation columns of the 7 x 7 (6 x 6) system are nearly dependent, the first-order bound of D through the inverse is
# large, and with it that of the second-pass ss, whichever form computes it
LUM_UNRESOLVED = ("far_pairs3", "far_noise1", "far_noise1e-3", "far_noise1e-6")


def restated(io, k, p1, p2, a, b, maxd):
    """oracle/icp_oracle.py's blocks in the fixture's LINK_LAYOUT names"""
    if k == 1:
        Cm, CD = io.covariance_euler_from_pairs(p1, p2)[:2]
        return {"C": Cm, "CD": CD}
    if k == 2:
        Cm, CD = io.covariance_quat(a, b, maxd * maxd)[:2]
        return {"C": Cm, "CD": CD}
    if k == 3:
        _, Blk, bd1, bd2 = io.ghelix_link_blocks(p1, p2)
        return {"Blk": Blk, "bd1": bd1, "bd2": bd2}
    r = io.get_pt_pairs(a, b, maxd * maxd)
    names = ("MkMkt", "DkDkt", "MkDkt", "DkMkt", "Ak1", "Ak2")
    out = dict(zip(names, io.gapx_link_blocks(p1, p2, r["cm"]))) if len(p1) else {}
    out["cm"], out["cd"] = r["cm"], r["cd"]
    return out


@pytest.mark.parametrize("backend", gc.BACKENDS)
@pytest.mark.parametrize("case", gc.LINK_CASES)
def test_reference_and_restatement_blocks_within_derived_tolerance(fx, orc, case, backend):
    from oracle import icp_oracle as io
    k = backend
    p1, p2, a, b, maxd, _ = link_pairs(orc, fx, case)
    n = len(p1)
    L = R.REF_LINK[k](p1, p2)
    got = fx["link_%s_b%d" % (case, k)]
    rest = restated(io, k, p1, p2, a, b, maxd)
    lay = mg.LINK_LAYOUT[k]
    if n < gc.MIN_PAIRS[k]:
        # under the threshold the back-end does not use the link: the lum back-ends hand out zeros
        if k <= 2:
            assert not np.any(got) and not np.any(rest["C"]) and not np.any(rest["CD"])
        if k == 4:
            # gapx6D's translation system still takes the centroids of such a link (genBAtransForLinkedPair runs for every
            # link): those of one pair are the pair itself, those of none are zero
            for name in ("cm", "cd"):
                for who, val in (("reference", got[lay[name]]), ("restatement", rest[name])):
                    if n == 0:
                        assert not np.any(val), (case, name, who)
                    else:
                        assert np.all(ratios(val, L, name) <= 1.0), (case, name, who)
                        assert np.array_equal(val, (p1 if name == "cm" else p2)[0]), (case, name, who)
        return
    aligned = case.endswith("aligned")
    if aligned and k <= 2:
        # data == model: ss is exactly 0.  lum6DEuler's guard hands out zeros; lum6DQuat has none and divides by it
        assert L.ss.v == 0 and "C" not in L.q
        if k == 1:
            assert not np.any(got) and not np.any(rest["C"])
        else:
            assert not np.all(np.isfinite(got[lay["C"]])), "the reference's block on an exactly aligned link is inf / NaN"
            assert np.array_equal(np.isnan(rest["C"]), np.isnan(got[lay["C"]].reshape(7, 7)))
            assert np.array_equal(np.isinf(rest["C"]), np.isinf(got[lay["C"]].reshape(7, 7)))
        return
    worst = 0.0
    for name in ("C", "CD", "Blk", "bd1", "bd2", "cm", "cd", "MkMkt", "DkDkt", "MkDkt", "DkMkt", "Ak1", "Ak2"):
        if name not in lay:
            continue
        for who, val in (("reference", got[lay[name]]), ("restatement", rest[name])):
            r = ratios(val, L, name)
            worst = max(worst, float(r.max()))
            assert np.all(r <= 1.0), (case, k, name, who, float(r.max()))
        if n == 1 and name not in ("cm", "cd", "bd1", "bd2", "Blk"):
            continue                     # one pair about its own centroid: zero whatever the pair
        if n - 1 < gc.MIN_PAIRS[k]:
            continue                     # with one pair less the back-end has no block
        d = discrimination(R.REF_LINK[k], p1, p2, name)
        if k <= 2 and case in LUM_UNRESOLVED:
            assert d < 10.0, (case, k, name, "LUM_UNRESOLVED is out of date: %.3g" % d)
            continue
        if aligned and name in ("bd1", "bd2", "Ak1", "Ak2"):
            assert d == np.inf and not np.any(L.values(name))       # exactly zero, with and without the pair
            continue
        assert d >= 10.0, (case, k, name, "one pair less moves it by only %.3g tolerances" % d)
    print("graph-blocks %-10s %-14s reference and restatement: worst |error| / tolerance = %.3g  (n = %d)"
          % (gc.NAMES[k], case, worst, n))


# ---- tdtk_graph_solve_update against the fixture --------------------------------------------------------------------------
def repack(k, ref_blocks, npairs):
    """the reference's per-link quantities in tdtk_graph_block_doubles layout (api_graph.cpp tdtk_graph_link_blocks)"""
    nl = len(ref_blocks)
    out = np.zeros((nl, {1: 42, 2: 56, 3: 43, 4: 49}[k]))
    for l in range(nl):
        b, use = ref_blocks[l], npairs[l] >= gc.MIN_PAIRS[k]
        if k <= 2:
            out[l] = b if use else 0.0
        elif k == 3:
            if use:
                out[l, 0] = 1.0; out[l, 1:37] = b[0:36]; out[l, 37:43] = b[36:42]
        else:
            out[l, 1:7] = b[0:6]                 # the centroids of every link feed the translation system
            if use:
                out[l, 0] = 1.0; out[l, 7:49] = b[6:48]
    return out


scatter, dropped = mg.scatter, mg.dropped      # the scatter rules and the drop rule restated: the generator asserts with them too


def upper_sym(A):
    Uu = np.triu(A)
    return Uu + np.triu(Uu, 1).T


def solve(A, rhs, drop=True):
    """graphSlam6D::solveSparseCholesky: the drop rule, then a Cholesky solve over the upper triangle"""
    S = upper_sym(dropped(A, drop))
    Lc = np.linalg.cholesky(S)
    return np.linalg.solve(Lc.T, np.linalg.solve(Lc, rhs))


def pose_scans(io, poses):
    """pose-only oracle scans (no points) at poses [scan][POSE_WIDTH]"""
    out = []
    for p in poses:
        s = io.OScan([0, 0, 0], [0, 0, 0], np.zeros((0, 3)))
        s.transMat, s.dalignxf, s.rPos, s.rPosTheta = p[0:16].copy(), p[16:32].copy(), p[32:35].copy(), p[35:38].copy()
        out.append(s)
    return out


def initial_poses(io, g):
    out = np.zeros((g.nscans, mg.POSE_WIDTH))
    for i in range(g.nscans):
        s = io.OScan(g.rPos[i], g.rPosTheta[i], np.zeros((0, 3)))
        out[i, 0:16], out[i, 16:32], out[i, 32:35], out[i, 35:38] = s.transMat, s.dalignxf, s.rPos, s.rPosTheta
        out[i, 38:42] = s.get_rPosQuat()
    return out


def pose_update(io, k, links, poses, blocks, X, T=None):
    """the restatement's pose update of back-end k (icp_oracle.py) from the poses [scan][POSE_WIDTH] and a solution X
    -> (poses after [scan][38], ret, gapx6D's T after, what gapx6D's translation step leaves in A).  T: gapx6D's carried
    translation (not modified)."""
    sc = pose_scans(io, poses)
    ns, tot = len(sc), 0.0
    w = {1: 6, 2: 7, 3: 6, 4: 3}[k]
    if k == 4:
        T = np.zeros(3 * (ns - 1)) if T is None else T.copy()
        lay = mg.LINK_LAYOUT[4]
        At = np.zeros(3 * (ns - 1))
        tot = io.gapx_translate_and_move(links, sc, [b[lay["cm"]] for b in blocks], [b[lay["cd"]] for b in blocks], X, T, At)
    for i in range(1, ns):
        Xi = X[(i - 1) * w:i * w]
        if k == 1:
            rP, rPT, dl = io.lum_pose_update(sc[i], Xi); sc[i].transformToEuler(rP, rPT); tot += dl
        elif k == 2:
            rP, rQ, dl = io.lumquat_pose_update(sc[i], Xi); sc[i].transformToQuat(rP, rQ); tot += dl
        elif k == 3:
            axf = io.helix_compute_rt(Xi); sc[i].transform(axf); tot += float(np.sqrt(axf[12] ** 2 + axf[13] ** 2 + axf[14] ** 2))
    out = np.array([np.concatenate([s.transMat, s.dalignxf, s.rPos, s.rPosTheta]) for s in sc])
    return out, tot / ns, T, (At if k == 4 else None)


def pose_vector(poses):
    """what the comparisons look at: transMat, rPos, rPosTheta of scans 1.."""
    p = np.asarray(poses)[1:]
    return np.concatenate([p[:, 0:16].ravel(), p[:, 32:38].ravel()])


class Case:
    """everything the solve comparison of one (graph, back-end, iteration) needs, from the fixture alone"""

    def __init__(self, io, fx, graph, k, it):
        self.g = g = gc.graph(graph)
        self.k, self.it = k, it
        key = "graph_%s_b%d_" % (graph, k)
        self.links = g.links(k)
        self.n = g.nscans - 1
        self.blocks = {j: fx[key + "blocks_it%d" % j] for j in (1, 2)}
        self.npairs = {j: fx[key + "npairs_it%d" % j] for j in (1, 2)}
        self.A, self.rhs, self.X = fx[key + "it%d_A" % it], fx[key + "it%d_rhs" % it], fx[key + "it%d_X" % it]
        self.start = initial_poses(io, g) if it == 1 else fx[key + "poses1"]
        self.poses, self.ret = fx[key + "poses%d" % it], float(fx[key + "ret%d" % it])
        self.X1 = fx[key + "it1_X"]
        S = upper_sym(self.A)
        N = len(S)
        self.cond = float(np.linalg.cond(S))
        back = N * float(R.gamma(3 * N + 1)) + len(self.links) * U
        self.tol_X = 2.0 * self.cond * back * float(np.linalg.norm(self.X))
        if k == 3:
            lay = mg.LINK_LAYOUT[3]
            d = np.zeros(N)
            for j in range(1, it + 1):           # bd carries over: so does what -bd1 misses of bd2
                for l, (f, t) in enumerate(self.links):
                    if self.npairs[j][l] >= gc.MIN_PAIRS[3]:
                        d[(t - 1) * 6:t * 6] += self.blocks[j][l][lay["bd2"]] + self.blocks[j][l][lay["bd1"]]
            self.tol_X += float(np.linalg.norm(np.linalg.inv(S), 2) * np.linalg.norm(d))
        self.io = io
        self.Jnorm = None
        self.S_inv_norm = float(np.linalg.norm(np.linalg.inv(S), 2))

    def T_before(self):
        """gapx6D's T as the iteration finds it: after iteration 1 it is the translation of the poses' update"""
        if self.k != 4 or self.it == 1:
            return None
        return self.after_it1()[2]

    def after_it1(self):
        return pose_update(self.io, 4, self.links, initial_poses(self.io, self.g), self.blocks[1], self.X1)

    def update(self, X):
        return pose_update(self.io, self.k, self.links, self.start, self.blocks[self.it], X, self.T_before())

    def tol_pose(self, more_X=0.0):
        """||J||_2 (tol_X + more_X) + gamma(64) max(1, |pose|_inf), J by central differences of the restatement's pose update"""
        if self.Jnorm is None:
            h = 1e-6 * max(1.0, float(np.abs(self.X).max()))
            J = np.zeros((len(pose_vector(self.poses)), len(self.X)))
            for c in range(len(self.X)):
                e = np.zeros(len(self.X)); e[c] = h
                J[:, c] = (pose_vector(self.update(self.X + e)[0]) - pose_vector(self.update(self.X - e)[0])) / (2 * h)
            self.Jnorm = float(np.linalg.norm(J, 2))
        return self.Jnorm * (self.tol_X + more_X) + float(R.gamma(64)) * max(1.0, float(np.abs(pose_vector(self.poses)).max()))


_cases = {}


def case_of(fx, graph, k, it):
    from oracle import icp_oracle as io
    if (graph, k, it) not in _cases:
        _cases[(graph, k, it)] = Case(io, fx, graph, k, it)
    return _cases[(graph, k, it)]


RUN_CASES = [(g, k) for g, k in GRAPH_CASES if (g, k) != ("few_pairs", 2)]


@pytest.mark.parametrize("graph,backend", RUN_CASES)
def test_restated_scatter_gives_the_matrix_cs_cholsol_was_handed(tdtk, fx, orc, graph, backend):
    """scatter() over the reference's own per-link quantities, then the drop rule, is the reference's matrix and right hand
    side bit for bit: the same additions in the same (link) order.  ghelix6DQ2's B / bd and gapx6D's B and A carry over.
    The library's own solve (the entry tdtk_graph_solve_update's back-end uses, drop rule inside) on that matrix gives the
    reference's X inside tol_X: tdtk_graph_solve_update does not hand X out."""
    import importlib
    capi = importlib.import_module("3dtk_amd._capi")
    k = backend
    state = None
    for it in (1, 2):
        c = case_of(fx, graph, k, it)
        A, rhs = scatter(k, c.links, c.blocks[it], c.npairs[it], c.n, state)
        assert _same(dropped(A), c.A), (graph, k, it, float(np.abs(dropped(A) - c.A).max()))
        assert _same(rhs, c.rhs), (graph, k, it)
        state = (A, rhs) if k == 3 else (A, c.update(c.X)[3]) if k == 4 else None
        if k in gc.DROP_GRAPHS.get(graph, ()):
            small = (A != 0) & (np.abs(A) <= 0.00001)
            assert small.any(), "the graph is there for its nonzero entries under the drop rule's 1e-5"
        X = solve(A, rhs)
        assert np.linalg.norm(X - c.X) <= c.tol_X, (graph, k, it)
        Xl = np.zeros(len(rhs))
        entry = capi.lib().tdtk_solve_chol_upper if k == 4 else capi.lib().tdtk_solve_spd
        capi.check(entry(capi.dptr(np.ascontiguousarray(A)), capi.dptr(rhs), len(rhs), capi.dptr(Xl)))
        err = float(np.linalg.norm(Xl - c.X))
        print("graph-solve %-10s %-15s it %d: |X error| %.3g  tol_X %.3g" % (gc.NAMES[k], graph, it, err, c.tol_X))
        assert err <= c.tol_X, (graph, k, it, err, c.tol_X)


def run_library(tdtk, fx, graph, k):
    """tdtk_graph_solve_update on the reference's blocks, both iterations, state carried, poses reset to the reference's
    before iteration 2 -> [(poses [scan][38], ret)] per iteration"""
    import importlib
    capi = importlib.import_module("3dtk_amd._capi")
    from oracle import icp_oracle as io
    c1 = case_of(fx, graph, k, 1)
    ns = c1.g.nscans
    frm = np.array([a for a, _ in c1.links], np.int32); to = np.array([b for _, b in c1.links], np.int32)
    n = ns - 1
    state = {3: np.zeros((6 * n) ** 2 + 6 * n), 4: np.zeros(3 * n + (3 * n) ** 2 + 3 * n)}.get(k)
    out = []
    for it in (1, 2):
        c = case_of(fx, graph, k, it)
        blocks = np.ascontiguousarray(repack(k, c.blocks[it], c.npairs[it]))
        assert blocks.shape[1] == capi.lib().tdtk_graph_block_doubles(k)
        tm = np.ascontiguousarray(c.start[:, 0:16]); da = np.ascontiguousarray(c.start[:, 16:32])
        rp = np.ascontiguousarray(c.start[:, 32:35]); rt = np.ascontiguousarray(c.start[:, 35:38])
        ret = C.c_double(0.0)
        capi.check(capi.lib().tdtk_graph_solve_update(k, len(frm), capi.iptr(frm), capi.iptr(to), capi.dptr(blocks), ns,
                                                      capi.dptr(tm), capi.dptr(da), capi.dptr(rp), capi.dptr(rt), None,
                                                      capi.dptr(state) if state is not None else None, None, C.byref(ret)))
        out.append((np.concatenate([tm, da, rp, rt], axis=1), float(ret.value)))
    return out


@pytest.mark.parametrize("graph,backend", RUN_CASES)
def test_solve_update_reproduces_the_reference(tdtk, fx, orc, graph, backend):
    k = backend
    got = run_library(tdtk, fx, graph, k)
    for it in (1, 2):
        c = case_of(fx, graph, k, it)
        tol = c.tol_pose()
        poses, ret = got[it - 1]
        # the restatement, now pinned block by block, from the reference's own X: inside the floor alone
        rest, rret = c.update(c.X)[:2]
        if k == 4:
            rret += float((c.npairs[it] >= gc.MIN_PAIRS[4]).sum()) / c.g.nscans       # genBArotForLinkedPair returns 1.0 (sic)
        err_r = float(np.abs(pose_vector(rest) - pose_vector(c.poses)).max())
        err = float(np.linalg.norm(pose_vector(poses) - pose_vector(c.poses)))
        # ret: a mean over the scans of lengths of X's (gapx6D: T's) translation parts, moved by at most the pose tolerance
        err_ret = abs(ret - c.ret)
        print("graph-solve %-10s %-15s it %d: cond %.3g  tol_X %.3g  ||J|| %.3g  tol_pose %.3g  |pose error| %.3g  "
              "|ret error| %.3g  restatement %.3g" % (gc.NAMES[k], graph, it, c.cond, c.tol_X, c.Jnorm, tol, err, err_ret, err_r))
        assert err <= tol, (graph, k, it, err, tol)
        assert err_ret <= tol, (graph, k, it, err_ret, tol)
        assert err_r <= tol and abs(rret - c.ret) <= tol, (graph, k, it, err_r)


@pytest.mark.parametrize("graph,backend", [(g, 1) for g in gc.GRAPHS])
def test_lum_assemble_solve_X(tdtk, fx, orc, graph, backend):
    """lum6DEuler's X itself, which tdtk_lum_assemble_solve hands out"""
    import importlib
    capi = importlib.import_module("3dtk_amd._capi")
    for it in (1, 2):
        c = case_of(fx, graph, 1, it)
        b = repack(1, c.blocks[it], c.npairs[it])
        Cm = np.ascontiguousarray(b[:, :36]); CD = np.ascontiguousarray(b[:, 36:])
        frm = np.array([a for a, _ in c.links], np.int32); to = np.array([t for _, t in c.links], np.int32)
        X = np.zeros(6 * c.n)
        capi.check(capi.lib().tdtk_lum_assemble_solve(len(frm), capi.iptr(frm), capi.iptr(to), capi.dptr(Cm), capi.dptr(CD),
                                                      c.g.nscans, capi.dptr(X), None, None))
        err = float(np.linalg.norm(X - c.X))
        print("graph-solve lum6DEuler %-15s it %d: |X error| %.3g  tol_X %.3g" % (graph, it, err, c.tol_X))
        assert err <= c.tol_X


# ---- every rule is seen to matter -----------------------------------------------------------------------------------------
def moved_by(fx, graph, k, it, state_it1=True, drop=True, **rules):
    """how far the restatement's poses of iteration `it` move when a rule is switched off, in units of the tolerance the
    solve comparison asserts there"""
    c = case_of(fx, graph, k, it)
    state = None
    if it == 2 and k >= 3 and state_it1:
        c1 = case_of(fx, graph, k, 1)
        state = scatter(k, c1.links, c1.blocks[1], c1.npairs[1], c1.n)
        if k == 4:
            state = (state[0], c.after_it1()[3])
    A, rhs = scatter(k, c.links, c.blocks[it], c.npairs[it], c.n, state, **rules)
    X = solve(A, rhs, drop)
    off = pose_vector(c.update(X)[0])
    return float(np.linalg.norm(off - pose_vector(c.poses))) / c.tol_pose()


def test_rule_assign_instead_of_add_matters(fx, orc):
    assert moved_by(fx, "both_directions", 2, 1, assign=False) >= 10.0


@pytest.mark.parametrize("graph,backend", [("weak_symmetric", 1), ("weak_symmetric", 2), ("tiny_symmetric", 3), ("tiny_symmetric", 4)])
def test_rule_drop_matters(fx, orc, graph, backend):
    """the lum back-ends on weak_symmetric, whose blocks are small enough for entries under 1e-5 to count; on
    tiny_symmetric theirs are rounding (the blocks are divided by an ss of 1e-11) and dropping them moves nothing"""
    assert moved_by(fx, graph, backend, 1, drop=False) >= 10.0


@pytest.mark.parametrize("backend", [3, 4])
def test_rule_carried_matrices_matter(fx, orc, backend):
    """ghelix6DQ2's B and bd, gapx6D's B and A: iteration 2 with a fresh system"""
    assert moved_by(fx, "chain_closure", backend, 2, state_it1=False) >= 10.0


def test_rule_carried_T_matters(fx, orc):
    c = case_of(fx, "chain_closure", 4, 2)
    fresh = pose_update(c.io, 4, c.links, c.start, c.blocks[2], c.X, None)[0]
    assert float(np.linalg.norm(pose_vector(fresh) - pose_vector(c.poses))) >= 10.0 * c.tol_pose()


@pytest.mark.parametrize("backend", gc.BACKENDS)
def test_rule_links_out_of_scan_0_matter(fx, orc, backend):
    """chain_closure without its closure (0, 3): the chain stays anchored by (0, 1)"""
    assert moved_by(fx, "chain_closure", backend, 1, first_scan=False) >= 10.0


@pytest.mark.parametrize("backend", [3, 4])
def test_rule_pair_count_threshold_matters(fx, orc, backend):
    """the link of one pair, used although `size() <= 1` skips it.  (For the lum back-ends the rule cannot be switched
    off: with two pairs MM is singular -- det [I -[u1]x; I -[u2]x] = det [u1 - u2]x = 0 -- and there is no block to add.)"""
    assert moved_by(fx, "few_pairs", backend, 1, thresholds=False) >= 10.0
