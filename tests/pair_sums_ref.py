"""Extended-precision reference for the pair sums, with tolerances that are derived, not chosen.

What is computed
----------------
From a pair list (p1, p2, pn) and the accumulation point `shift` -- all of them doubles -- `raw_sums` evaluates in
np.longdouble (64-bit mantissa) every term t_ik of every accumulator column k as accum_body (kernels.hip) defines it, and
per column

    S_k  = sum_i t_ik           the exact sum (to 2^-64; test_pair_sums_reference_host.py checks it against Fractions)
    M_k  = sum_i T_ik           T_ik >= |t_ik|: the term with every product replaced by its absolute value, so that a
                                term that is itself a difference of products (the LUM cross terms, the NAPX c = d x n) is
                                bounded by what its roundings scale with, not by what is left after the cancellation
    IN_k = sum_i sum_a |d t_ik / d p1_a| u |p1_a|      (see "input term")

`finished` turns S into everything finish_sums (api_search.cpp) hands out, and `lum_link` into the MM / MZ / ss of
tdtk_lum_links.  napx_A / napx_B are evaluated directly about the true data centroid, not through finish_sums'
L A0 L^T transport.  The per-link blocks of the graph back-ends (tdtk_graph_link_blocks: lum6DQuat, ghelix6DQ2, gapx6D, and
lum6DEuler's reference form) are at the end of the file, each in the reference's form and in the library's.

The bound on a raw column
-------------------------
u = 2^-53.  Any order of n fp64 additions is within  g(n-1) M_k,  g(m) = m u / (1 - m u),  of the exact sum of the terms
it was handed (Higham, Accuracy and Stability, 4.2: the bound does not depend on the association, which is why it covers
the lanes, the wave shuffles, the LDS pass, the rows and k_final alike).  The terms it is handed are not the exact ones:
a term computed with c_k roundings is within c_k u T_ik of t_ik.  So

    tol(S_k) = (g(n-1) + c_k u) M_k + IN_k

c_k is counted in accum_body (and is the same in chunk_pair_sums and the FUSE 1 / 2 / 3 / 5 epilogues, which hold the same
expressions).  The library is built with -ffp-contract=off; a contraction would only lower a count.  With
p = m - t, m' = m - shift, d' = t - shift (one rounding each), x = (m + t) / 2 (one rounding: the halving is exact):

    ACC_N    1                                   0
    ACC_SUM  px px + py py + pz pz               a square is p (1, twice) and the product (1) = 3; 2 additions   5
    ACC_SM/SD  m', d'                            1
    ACC_P/MM/DD  m' d', m' m', d' d'             3
    ACC_NA   v_r v_s, v = [d' x n ; n]: c = d'_1 n_z - d'_2 n_y is d' (1), product (1), difference (1) = 3 against
             |d'_1 n_z| + |d'_2 n_y|; n itself is an input.  c c: 7, c n: 4, n n: 1
    ACC_NB   v_r                                 3, 0
    ACC_NS   (p.n)^2: p.n is p (1), product (1), two additions = 4; squared 2 * 4 + 1                    9
    ACC_L    x: 1;  x x + y y: 3 + 1 = 4;  x y: 3;  dx: 1;  -z dy + y dz: 3 + 1 = 4
    ACC_LU   x dx + y dy + z dz                  3 + 2 = 5
    ACC_LSS  e_0 = dx - (D0 - y D4 + z D5): the longest chain is y (1), y D4 (1), the two additions inside the bracket
             and the outer difference = 5, against |dx| + |D0| + |y D4| + |z D5|; three squares 2 * 5 + 1, 2 additions   13

Input term.  The kernel that sums recomputes m = A c from the model point; the pair list's p1 was written by another
kernel with the same expression.  Should the two ever differ by a rounding (they do not with contraction off), the term
moves by |dt/dm_a| u |m_a|; IN_k adds that up with the derivative taken from the column's formula.  It is computed from
the data like everything else and is the dominant part only for clouds far from the origin.

Finished quantities
-------------------
finish_sums is a straight-line program of + - * /.  `E` carries a value and a first-order error bound through such a
program: for r = a op b computed in fp64 from inputs off by e_a, e_b

    e(a +- b) = e_a + e_b + u |r|,    e(a b) = |a| e_b + |b| e_a + u |r|,    e(a / b) = e_a / |b| + |a| e_b / b^2 + u |r|

(no u where the operation is exact: a factor 0 or +-1, a summand 0).  `finished` runs finish_sums' own formulas, in its
order of operations, over E(S_k, tol(S_k)); what comes out is each quantity's tolerance -- e.g. for Si_ab = P - Sm Sd / n
    tol = tol(P) + (|Sm| tol(Sd) + |Sd| tol(Sm)) / n + 2 u |Sm Sd / n| + u |Si|.
tdtk_lum_links' ss goes through invert_dense's Gauss-Jordan elimination the same way (`lum_link`).
No constant appears anywhere that is not a counted rounding; nothing is read off a GPU result.

Discrimination
--------------
A tolerance is only worth asserting if a wrong sum would break it.  `discrimination` recomputes every finished quantity
with ONE pair left out -- the pair of median |t|, where a pair's |t| is its weakest column, min_k |t_ik| / tol(S_k):
a typical pair in every column at once -- and returns move / tolerance; the tests require >= 10 for every quantity they
assert.  The one exception is arithmetic, not a concession: with n == 1 the centred
second moments (Si, apx, mom, gapx, the napx c-blocks) are zero for any pair, so leaving the pair out cannot move them;
there the quantities in CENTRED are still compared with the reference but not asked to discriminate.
"""
import numpy as np

LD = np.longdouble
if np.finfo(LD).nmant < 63:
    raise AssertionError("pair_sums_ref needs an extended-precision np.longdouble (nmant >= 63), this one has %d bits"
                         % np.finfo(LD).nmant)
U = LD(2) ** -53

WANT_APX, WANT_NAPX, WANT_LUM, WANT_GAPX, WANT_MOM2 = 1, 2, 4, 8, 16
NO_CROSS = 0x100

# accumulator columns (kernels.h)
ACC_N, ACC_SUM, ACC_SM, ACC_SD, ACC_P, ACC_DD, ACC_NA, ACC_NB, ACC_NS = 0, 1, 2, 5, 8, 17, 23, 44, 50
ACC_L, ACC_LSS, ACC_MM, ACC_LU, ACC_TOTAL = 51, 66, 67, 73, 74
_UP3 = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def gamma(m):
    m = LD(max(int(m), 0))
    return m * U / (LD(1) - m * U)


def kernel_want(want):
    """the columns launch_accum fills for a public `want` (GAPX and MOM2 are both the MM + DD columns on the base block)"""
    if want & NO_CROSS:
        return want
    if want & (WANT_GAPX | WANT_MOM2):
        return WANT_GAPX
    return want & 7


def _terms(p1, p2, pn, shift, want, D=None):
    """yields (column, t[n], T[n], IN[n], c) for every column the kernel instantiation `want` fills"""
    m = np.asarray(p1, LD).reshape(-1, 3); t = np.asarray(p2, LD).reshape(-1, 3)
    sh = np.asarray(shift, LD)
    n = len(m)
    one, zero = np.ones(n, LD), np.zeros(n, LD)
    am = U * np.abs(m)                      # what one rounding of m_a is worth
    p = m - t
    ms, ds = m - sh, t - sh
    yield ACC_N, one, one, zero, 0
    yield ACC_SUM, (p * p).sum(1), (p * p).sum(1), 2 * (np.abs(p) * am).sum(1), 5
    if not (want & NO_CROSS):
        for a in range(3):
            yield ACC_SM + a, ms[:, a], np.abs(ms[:, a]), am[:, a], 1
            yield ACC_SD + a, ds[:, a], np.abs(ds[:, a]), zero, 1
        for a in range(3):
            for b in range(3):
                v = ms[:, a] * ds[:, b]
                yield ACC_P + 3 * a + b, v, np.abs(v), np.abs(ds[:, b]) * am[:, a], 3
        # no column, but what apx_B and gapx_Ak are the sums of ((p1 - p2) x d', all that is left of P_ab - P_ba, whose
        # tolerances -- twice over, for the DD columns apx_B subtracts -- it inherits): column -1 only takes part in
        # choosing the pair the discrimination check leaves out, and carries the two columns in place of a count
        for a, b in ((2, 1), (0, 2), (1, 0)):
            v = p[:, a] * ds[:, b] - p[:, b] * ds[:, a]
            yield -1, v, np.abs(v), zero, (ACC_P + 3 * a + b, ACC_P + 3 * b + a)
    if want & WANT_GAPX:
        for q, (a, b) in enumerate(_UP3):
            v = ms[:, a] * ms[:, b]
            yield ACC_MM + q, v, np.abs(v), np.abs(ms[:, a]) * am[:, b] + np.abs(ms[:, b]) * am[:, a], 3
    if want & (WANT_APX | WANT_GAPX):
        for q, (a, b) in enumerate(_UP3):
            v = ds[:, a] * ds[:, b]
            yield ACC_DD + q, v, np.abs(v), zero, 3
    if want & WANT_NAPX:
        nn = np.asarray(pn, LD).reshape(-1, 3)
        d0, d1, d2 = ds.T
        nx, ny, nz = nn.T
        v = [d1 * nz - d2 * ny, d2 * nx - d0 * nz, d0 * ny - d1 * nx, nx, ny, nz]
        V = [np.abs(d1 * nz) + np.abs(d2 * ny), np.abs(d2 * nx) + np.abs(d0 * nz), np.abs(d0 * ny) + np.abs(d1 * nx),
             np.abs(nx), np.abs(ny), np.abs(nz)]
        cv = [3, 3, 3, 0, 0, 0]
        q = 0
        for r in range(6):
            for s in range(r, 6):
                yield ACC_NA + q, v[r] * v[s], V[r] * V[s], zero, cv[r] + cv[s] + 1
                q += 1
        for r in range(6):
            yield ACC_NB + r, v[r], V[r], zero, cv[r]
        dd = (p * nn).sum(1)
        DDm = np.abs(p * nn).sum(1)
        yield ACC_NS, dd * dd, DDm * DDm, 2 * np.abs(dd) * (np.abs(nn) * am).sum(1), 9
    if want & WANT_LUM:
        x, y, z = ((m + t) / 2).T
        dx, dy, dz = p.T
        ax, ay, az = am.T
        h = LD(0.5)
        for a, w in enumerate((x, y, z)):
            yield ACC_L + a, w, np.abs(w), h * am[:, a], 1
        for k, (a, b, ea, eb) in enumerate(((x, y, ax, ay), (x, z, ax, az), (y, z, ay, az))):
            v = a * a + b * b
            yield ACC_L + 3 + k, v, v, np.abs(a) * ea + np.abs(b) * eb, 4
        for k, (a, b, ea, eb) in enumerate(((x, y, ax, ay), (x, z, ax, az), (y, z, ay, az))):
            v = a * b
            yield ACC_L + 6 + k, v, np.abs(v), h * (np.abs(b) * ea + np.abs(a) * eb), 3
        for a, w in enumerate((dx, dy, dz)):
            yield ACC_L + 9 + a, w, np.abs(w), am[:, a], 1
        A = np.abs
        yield (ACC_L + 12, -z * dy + y * dz, A(z * dy) + A(y * dz),
               (h * A(dy) + A(y)) * az + (A(z) + h * A(dz)) * ay, 4)
        yield (ACC_L + 13, -y * dx + x * dy, A(y * dx) + A(x * dy),
               (h * A(dx) + A(x)) * ay + (A(y) + h * A(dy)) * ax, 4)
        yield (ACC_L + 14, z * dx - x * dz, A(z * dx) + A(x * dz),
               (h * A(dx) + A(x)) * az + (A(z) + h * A(dz)) * ax, 4)
        yield (ACC_LU, x * dx + y * dy + z * dz, A(x * dx) + A(y * dy) + A(z * dz),
               (h * A(dx) + A(x)) * ax + (h * A(dy) + A(y)) * ay + (h * A(dz) + A(z)) * az, 5)
        if D is not None:
            Dl = np.asarray(D, LD)
            e = [dx - (Dl[0] - y * Dl[4] + z * Dl[5]), dy - (Dl[1] - z * Dl[3] + x * Dl[4]),
                 dz - (Dl[2] + y * Dl[3] - x * Dl[5])]
            Em = [A(dx) + A(Dl[0]) + A(y * Dl[4]) + A(z * Dl[5]), A(dy) + A(Dl[1]) + A(z * Dl[3]) + A(x * Dl[4]),
                  A(dz) + A(Dl[2]) + A(y * Dl[3]) + A(x * Dl[5])]
            J = [[one, h * A(Dl[4]) * one, h * A(Dl[5]) * one], [h * A(Dl[4]) * one, one, h * A(Dl[3]) * one],
                 [h * A(Dl[5]) * one, h * A(Dl[3]) * one, one]]
            inp = sum(2 * A(e[r]) * (J[r][0] * ax + J[r][1] * ay + J[r][2] * az) for r in range(3))
            yield ACC_LSS, e[0] * e[0] + e[1] * e[1] + e[2] * e[2], Em[0] * Em[0] + Em[1] * Em[1] + Em[2] * Em[2], inp, 13


class Raw:
    """S, M, IN, c per column, n, and tol(S_k); `used` marks the columns the instantiation fills"""

    def __init__(self, n):
        self.n = int(n)
        self.S = np.zeros(ACC_TOTAL, LD); self.M = np.zeros(ACC_TOTAL, LD); self.IN = np.zeros(ACC_TOTAL, LD)
        self.c = np.zeros(ACC_TOTAL, int); self.used = np.zeros(ACC_TOTAL, bool)
        self.weak = None

    def median_pair(self):
        """the pair to leave out: of median |t|, |t| being the pair's weakest column -- its smallest |t_ik| / tol(S_k) over
        the columns -- so that the pair is a typical one in every column at once"""
        return int(np.argsort(self.weak, kind="stable")[len(self.weak) // 2])

    @property
    def tol(self):
        return (gamma(self.n - 1) + self.c * U) * self.M + self.IN


def raw_sums(p1, p2, pn, shift, want, D=None, drop=None, full=None):
    """the exact columns of the kernel instantiation `want` (kernel_want(public want), or LUM | NO_CROSS for a link).
    drop = j: without pair j (tolerances are not meant to be read off such a result); full: the Raw of the whole list,
    if the caller has it, so that only pair j's terms are evaluated."""
    p1 = np.asarray(p1, float).reshape(-1, 3); p2 = np.asarray(p2, float).reshape(-1, 3)
    pn = np.zeros_like(p1) if pn is None else np.asarray(pn, float).reshape(-1, 3)
    r = Raw(len(p1) - (0 if drop is None else 1))
    if full is not None:
        r.S, r.M, r.IN, r.c, r.used = full.S.copy(), full.M.copy(), full.IN.copy(), full.c.copy(), full.used.copy()
    else:
        mags, pseudo = [], []
        for k, t, T, IN, c in _terms(p1, p2, pn, shift, want, D):
            if k >= 0:
                r.S[k], r.M[k], r.IN[k], r.c[k], r.used[k] = t.sum(), T.sum(), IN.sum(), c, True
                mags.append((k, np.abs(t).astype(float)))
            else:
                pseudo.append((c, np.abs(t).astype(float)))
        # a pair's |t|: its weakest column, each column measured in tolerances (how far leaving the pair out moves the sum)
        tol = r.tol
        weak = np.full(len(p1), np.inf)
        for k, a in mags:
            if tol[k] > 0:
                np.minimum(weak, a / float(tol[k]), out=weak)
        for (ka, kb), a in pseudo:
            np.minimum(weak, a / float(2 * (tol[ka] + tol[kb])), out=weak)
        r.weak = weak
    if drop is not None:
        j = slice(drop, drop + 1)
        for k, t, T, IN, c in _terms(p1[j], p2[j], pn[j], shift, want, D):
            if k >= 0:
                r.S[k] -= t[0]; r.M[k] -= T[0]; r.IN[k] -= IN[0]
    return r


# ---- value + first-order error bound through a straight-line fp64 program ---------------------------------------------
class E:
    __slots__ = ("v", "e")

    def __init__(self, v, e=0):
        self.v = LD(v); self.e = LD(e)

    @staticmethod
    def of(x):
        return x if isinstance(x, E) else E(x)

    def _exact(self, *vals):
        return self.e == 0 and any(self.v == w for w in vals)

    def __add__(self, o):
        o = E.of(o)
        v = self.v + o.v
        r = LD(0) if (self._exact(0) or o._exact(0)) else U * abs(v)
        return E(v, self.e + o.e + r)
    __radd__ = __add__

    def __neg__(self):
        return E(-self.v, self.e)

    def __sub__(self, o):
        return self + (-E.of(o))

    def __rsub__(self, o):
        return E.of(o) + (-self)

    def __mul__(self, o):
        o = E.of(o)
        v = self.v * o.v
        r = LD(0) if (self._exact(0, 1, -1) or o._exact(0, 1, -1)) else U * abs(v)
        return E(v, abs(self.v) * o.e + abs(o.v) * self.e + r)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = E.of(o)
        v = self.v / o.v
        r = LD(0) if o._exact(1, -1) else U * abs(v)
        return E(v, self.e / abs(o.v) + abs(self.v) * o.e / (o.v * o.v) + r)

    def __rtruediv__(self, o):
        return E.of(o) / self


CENTRED = ("Si", "apx_A", "apx_B", "mom_mm", "mom_dd", "gapx_MkMkt", "gapx_DkDkt", "gapx_MkDkt", "gapx_DkMkt",
           "gapx_Ak1", "gapx_Ak2", "napx_A", "napx_B")
FIELDS = ("sum", "centroid_m", "centroid_d", "Si", "apx_A", "apx_B", "napx_A", "napx_B", "napx_sum", "lum", "lum_sumd2",
          "gapx_MkMkt", "gapx_DkDkt", "gapx_MkDkt", "gapx_DkMkt", "gapx_Ak1", "gapx_Ak2", "mom_mm", "mom_dd", "lum_udot")


def _finish_E(raw, shift, want, has_D):
    """finish_sums (api_search.cpp), operation by operation, over E(S_k, tol_k).  -> {field: list of E}; fields `want` does not
    ask for are absent (the library leaves them 0)."""
    tol = raw.tol
    acc = [E(raw.S[k], tol[k]) for k in range(ACC_TOTAL)]
    n = raw.n
    o = {"sum": [acc[ACC_SUM]], "lum_sumd2": [acc[ACC_LSS] if has_D else acc[ACC_SUM]]}
    if n == 0:
        return o
    sh = [E(s) for s in np.asarray(shift, float)]
    Sm, Sd = acc[ACC_SM:ACC_SM + 3], acc[ACC_SD:ACC_SD + 3]
    P = acc[ACC_P:ACC_P + 9]
    wm = [Sm[a] / n for a in range(3)]; wd = [Sd[a] / n for a in range(3)]
    o["centroid_m"] = [sh[a] + wm[a] for a in range(3)]
    o["centroid_d"] = [sh[a] + wd[a] for a in range(3)]
    o["Si"] = [P[a * 3 + b] - Sm[a] * Sd[b] / n for a in range(3) for b in range(3)]

    def full(up):
        return [[up[0], up[1], up[2]], [up[1], up[3], up[4]], [up[2], up[4], up[5]]]
    if want & WANT_APX:
        D2 = full(acc[ACC_DD:ACC_DD + 6])
        Dc = [[D2[a][b] - Sd[a] * Sd[b] / n for b in range(3)] for a in range(3)]
        Ee = [[P[a * 3 + b] - D2[a][b] - (Sm[a] - Sd[a]) * Sd[b] / n for b in range(3)] for a in range(3)]
        o["apx_A"] = [Dc[1][1] + Dc[2][2], -Dc[0][1], -Dc[0][2], Dc[0][0] + Dc[2][2], -Dc[1][2], Dc[0][0] + Dc[1][1]]
        o["apx_B"] = [Ee[2][1] - Ee[1][2], Ee[0][2] - Ee[2][0], Ee[1][0] - Ee[0][1]]
    if want & WANT_NAPX:
        A0 = [[None] * 6 for _ in range(6)]
        q = 0
        for r in range(6):
            for s in range(r, 6):
                A0[r][s] = A0[s][r] = acc[ACC_NA + q]; q += 1
        L = [[E(1.0 if r == s else 0.0) for s in range(6)] for r in range(6)]
        w = wd
        L[0][4] = w[2]; L[0][5] = -w[1]
        L[1][3] = -w[2]; L[1][5] = w[0]
        L[2][3] = w[1]; L[2][4] = -w[0]
        T1 = [[None] * 6 for _ in range(6)]
        for r in range(6):
            for s in range(6):
                v = E(0.0)
                for k in range(6):
                    v = v + L[r][k] * A0[k][s]
                T1[r][s] = v
        o["napx_A"] = []
        for r in range(6):
            for s in range(r, 6):
                v = E(0.0)
                for k in range(6):
                    v = v + T1[r][k] * L[s][k]
                o["napx_A"].append(v)
        o["napx_B"] = []
        for r in range(6):
            v = E(0.0)
            for k in range(6):
                v = v + L[r][k] * acc[ACC_NB + k]
            o["napx_B"].append(v)
        o["napx_sum"] = [acc[ACC_NS]]
    if want & WANT_LUM:
        o["lum"] = acc[ACC_L:ACC_L + 15]
        o["lum_udot"] = [acc[ACC_LU]]
    if want & WANT_MOM2:
        mm, dd = acc[ACC_MM:ACC_MM + 6], acc[ACC_DD:ACC_DD + 6]
        o["mom_mm"] = [mm[q] - Sm[a] * Sm[b] / n for q, (a, b) in enumerate(_UP3)]
        o["mom_dd"] = [dd[q] - Sd[a] * Sd[b] / n for q, (a, b) in enumerate(_UP3)]
    if want & WANT_GAPX:
        MM, DD = full(acc[ACC_MM:ACC_MM + 6]), full(acc[ACC_DD:ACC_DD + 6])
        Sb = [Sd[i] - Sm[i] for i in range(3)]
        Saa = [[MM[i][j] - n * wm[i] * wm[j] for j in range(3)] for i in range(3)]
        Sbb = [[DD[i][j] - wm[i] * Sd[j] - wm[j] * Sd[i] + n * wm[i] * wm[j] for j in range(3)] for i in range(3)]
        Sab = [[P[i * 3 + j] - wm[i] * Sd[j] for j in range(3)] for i in range(3)]

        def sym(S):
            return [S[1][1] + S[2][2], -S[0][1], -S[0][2], -S[0][1], S[0][0] + S[2][2], -S[1][2],
                    -S[0][2], -S[1][2], S[0][0] + S[1][1]]
        o["gapx_MkMkt"] = sym(Saa)
        o["gapx_DkDkt"] = sym(Sbb)
        d11, d22, d33 = Sab[1][1] + Sb[2], Sab[0][0] + Sb[2], Sab[0][0] + Sb[1]
        o["gapx_MkDkt"] = [d11, -Sab[1][0], -Sab[2][0], -Sab[1][0], d22, -Sab[2][1], -Sab[2][0], -Sab[2][1], d33]
        o["gapx_DkMkt"] = [d11, -Sab[0][1], -Sab[0][2], -Sab[0][1], d22, -Sab[1][2], -Sab[0][2], -Sab[1][2], d33]
        o["gapx_Ak2"] = [Sab[2][1] - Sab[1][2], Sab[0][2] - Sab[2][0], Sab[1][0] - Sab[0][1]]
        o["gapx_Ak1"] = [-v for v in o["gapx_Ak2"]]
    return o


def _napx_direct(p2, pn, cd, drop=None):
    """napx_A (21), napx_B (6) about the data centroid cd, straight from the pairs"""
    d = np.asarray(p2, LD).reshape(-1, 3) - cd; nn = np.asarray(pn, LD).reshape(-1, 3)
    if drop is not None:
        keep = np.ones(len(d), bool); keep[drop] = False
        d, nn = d[keep], nn[keep]
    v = [d[:, 1] * nn[:, 2] - d[:, 2] * nn[:, 1], d[:, 2] * nn[:, 0] - d[:, 0] * nn[:, 2],
         d[:, 0] * nn[:, 1] - d[:, 1] * nn[:, 0], nn[:, 0], nn[:, 1], nn[:, 2]]
    return ([(v[r] * v[s]).sum() for r in range(6) for s in range(r, 6)], [v[r].sum() for r in range(6)])


class Finished:
    """ref[field], tol[field]: longdouble arrays; fields the library leaves 0 for this `want` are exact zeros with tol 0"""

    def __init__(self, n):
        self.n = n; self.ref = {}; self.tol = {}


def _sizes():
    return dict(sum=1, centroid_m=3, centroid_d=3, Si=9, apx_A=6, apx_B=3, napx_A=21, napx_B=6, napx_sum=1, lum=15,
                lum_sumd2=1, gapx_MkMkt=9, gapx_DkDkt=9, gapx_MkDkt=9, gapx_DkMkt=9, gapx_Ak1=3, gapx_Ak2=3, mom_mm=6,
                mom_dd=6, lum_udot=1)


def finished(p1, p2, pn, shift, want, D=None, drop=None, full=None):
    """what tdtk_get_pt_pairs / tdtk_links_pair_sums hand out for the public `want` (lum_D = D), with tolerances"""
    raw = raw_sums(p1, p2, pn, shift, kernel_want(want), D, drop, full)
    o = _finish_E(raw, shift, want, D is not None)
    f = Finished(raw.n)
    f.raw = raw
    for name, k in _sizes().items():
        if name in o:
            f.ref[name] = np.array([x.v for x in o[name]], LD); f.tol[name] = np.array([x.e for x in o[name]], LD)
        else:
            f.ref[name] = np.zeros(k, LD); f.tol[name] = np.zeros(k, LD)
    if (want & WANT_NAPX) and raw.n:
        cd = np.asarray(shift, LD) + raw.S[ACC_SD:ACC_SD + 3] / LD(raw.n)
        A, B = _napx_direct(p2, pn, cd, drop)
        f.ref["napx_A"] = np.array(A, LD); f.ref["napx_B"] = np.array(B, LD)
    return f


def discrimination(p1, p2, pn, shift, want, D=None, fin=None):
    """{field: min over its entries of |move| / tol} when the pair Raw.median_pair() is left out (inf where the
    tolerance is 0 and the entry moves, or the block is not asked for)"""
    p1 = np.asarray(p1, float).reshape(-1, 3); p2 = np.asarray(p2, float).reshape(-1, 3)
    fin = fin or finished(p1, p2, pn, shift, want, D)
    if fin.n == 0:
        return {}
    j = fin.raw.median_pair()
    less = finished(p1, p2, pn, shift, want, D, drop=j, full=fin.raw)
    out = {}
    for name in fin.ref:
        if not np.any(fin.tol[name] > 0) and not np.any(fin.ref[name] != 0):
            continue
        if fin.n == 1 and name in CENTRED:
            continue
        move = np.abs(less.ref[name] - fin.ref[name])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(fin.tol[name] > 0, move / fin.tol[name], np.where(move > 0, np.inf, 0.0))
        out[name] = float(ratio.min())
    return out


# ---- tdtk_lum_links ---------------------------------------------------------------------------------------------------
def lum_link(p1, p2, drop=None, full=None):
    """m, MM (36), MZ (6), ss of one lum6DEuler link (api_links.cpp tdtk_lum_links) as E values; ss through invert_dense's
    Gauss-Jordan elimination with partial pivoting, hand-written here over E.  m <= 2: MM, MZ, ss are None (the library
    hands out zero blocks)."""
    raw = raw_sums(p1, p2, None, [0.0, 0.0, 0.0], WANT_LUM | NO_CROSS, None, drop, full)
    m = raw.n
    if m <= 2:
        return m, None, None, None
    tol = raw.tol
    L = [E(raw.S[ACC_L + k], tol[ACC_L + k]) for k in range(15)]
    MM = [[E(0.0) for _ in range(6)] for _ in range(6)]
    MM[0][0] = MM[1][1] = MM[2][2] = E(float(m))
    MM[3][3] = L[5]; MM[4][4] = L[3]; MM[5][5] = L[4]
    MM[0][4] = MM[4][0] = -L[1]; MM[0][5] = MM[5][0] = L[2]
    MM[1][3] = MM[3][1] = -L[2]; MM[1][4] = MM[4][1] = L[0]
    MM[2][3] = MM[3][2] = L[1]; MM[2][5] = MM[5][2] = -L[0]
    MM[3][4] = MM[4][3] = -L[7]; MM[3][5] = MM[5][3] = -L[6]; MM[4][5] = MM[5][4] = -L[8]
    MZ = L[9:15]
    a = [row[:] for row in MM]
    b = [[E(1.0 if r == c else 0.0) for c in range(6)] for r in range(6)]
    for c in range(6):
        piv = max(range(c, 6), key=lambda r: (abs(a[r][c].v), -r))
        if piv != c:
            a[piv], a[c] = a[c], a[piv]; b[piv], b[c] = b[c], b[piv]
        inv = 1.0 / a[c][c]
        for r in range(6):
            if r == c:
                continue
            f = a[r][c] * inv
            if f.v == 0:
                continue
            for k in range(6):
                a[r][k] = a[r][k] - f * a[c][k]
                b[r][k] = b[r][k] - f * b[c][k]
        for k in range(6):
            a[c][k] = a[c][k] * inv
            b[c][k] = b[c][k] * inv
    dmz = E(0.0)
    for r in range(6):
        v = E(0.0)
        for k in range(6):
            v = v + b[r][k] * MZ[k]
        dmz = dmz + v * MZ[r]
    ss = (E(raw.S[ACC_SUM], tol[ACC_SUM]) - dmz) / (2.0 * float(m) - 3.0)
    return m, [x for row in MM for x in row], MZ, ss


# ---- the inputs both tiers use ----------------------------------------------------------------------------------------
def rigid(t, angles):
    """a 4x4 pose in the library's layout (A[4 c + r] = R[r][c], translation in A[12:15]) from three Euler angles"""
    a, b, c = angles
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    R = Rz @ Ry @ Rx
    A = np.zeros(16)
    for r in range(3):
        for col in range(3):
            A[4 * col + r] = R[r, col]
    A[12:15] = t; A[15] = 1.0
    return A


def apply(A, x):
    """x A: the points x (n, 3) moved by the pose A, in plain fp64 (inputs only; nothing is compared with it)"""
    R = np.array([[A[0], A[4], A[8]], [A[1], A[5], A[9]], [A[2], A[6], A[10]]])
    return x @ R.T + A[12:15]


PATTERNS = ("all", "none", "one", "half", "window")
AWAY = -5000.0      # queries moved by this on every axis pair with nothing; being a cluster of their own that is smaller on
                    # every axis, they come first in any order that sorts by position, as whole waves, chunks and slabs


def make_inputs(N, pattern="all", far=False, seed=1):
    """model: 20 000 uniform points in +-200 with 60 duplicates; queries: model points drawn with replacement, moved by a
    non-trivial A, + N(0, 0.4) (`seed` is theirs); far: the model and A's translation offset by 1e6 on every axis.
    -> dict(model, A, d, nr, maxd2)"""
    off = 1.0e6 if far else 0.0
    m = np.random.default_rng(1).uniform(-200, 200, (20000, 3)); m[100:160] = m[0:60]     # the same model for every seed
    rng = np.random.default_rng(seed)
    m += off
    A = rigid(np.array([12.0, -7.0, 3.0]) + off, [0.03, -0.02, 0.04])
    d = apply(A, m[rng.integers(0, len(m), N)]) + rng.normal(0, 0.4, (N, 3))
    nr = rng.normal(size=(N, 3))
    maxd2 = 4.0
    if pattern == "none":
        maxd2 = 1e-12
    elif pattern == "one":
        d[:-1] += AWAY
    elif pattern == "half":
        d[:N // 2] += AWAY
    elif pattern == "window":
        d[:-100] += AWAY
    elif pattern != "all":
        raise ValueError(pattern)
    return dict(model=m, A=A, d=d, nr=nr, maxd2=maxd2)


def shift_of(model, A):
    """the accumulation point of a pass: the model's box centre moved by A (pass_shift, api_search.cpp)"""
    c = 0.5 * (model.min(0) + model.max(0))
    return np.array([c[0] * A[k] + c[1] * A[4 + k] + c[2] * A[8 + k] + A[12 + k] for k in range(3)])


def unit_normals(nr):
    """the normalised data normal as the pair list carries it in pairing mode 0 (the reference leaves it unset there)"""
    return nr / np.sqrt(nr[:, 0] * nr[:, 0] + nr[:, 1] * nr[:, 1] + nr[:, 2] * nr[:, 2])[:, None]


def lum_link_and_one_less(p1, p2):
    """lum_link of the list and of the list without its median pair"""
    full = raw_sums(p1, p2, None, [0.0, 0.0, 0.0], WANT_LUM | NO_CROSS)
    return lum_link(p1, p2, full=full), lum_link(p1, p2, drop=full.median_pair(), full=full)


# ---- the comparison both GPU files make --------------------------------------------------------------------------------
def _fields(s):
    return {f: np.atleast_1d(np.array(getattr(s, f), float)).ravel() for f in FIELDS}


def check_struct(s, fin, disc, producer):
    """s: a tdtk_pair_sums the library filled.  n exact, unrequested blocks exactly 0, the rest inside the derived
    tolerance, every asserted quantity discriminating."""
    assert int(s.n) == fin.n, producer
    worst = 0.0
    got = _fields(s)
    for f, v in got.items():
        assert np.all(np.isfinite(v)), (producer, f)
        ref, tol = fin.ref[f], fin.tol[f]
        if fin.n == 0 or not (np.any(tol > 0) or np.any(ref != 0)):
            assert np.all(v == 0.0), (producer, f, v)          # not asked for (or no pair at all): exactly zero
            continue
        err = np.abs(v.astype(LD) - ref)
        ratio = float(np.max(np.where(tol > 0, err / np.where(tol > 0, tol, 1), np.where(err > 0, np.inf, 0.0))))
        print("pair-sums %-28s %-12s |error| / tolerance = %.3f" % (producer, f, ratio))
        worst = max(worst, ratio)
        assert np.all(err <= tol), (producer, f, ratio, v, ref, tol)
        if f in disc:
            assert disc[f] >= 10.0, (producer, f, "one pair less moves it by only %.2f tolerances" % disc[f])
        else:
            assert fin.n == 1 and f in CENTRED, (producer, f)
    print("pair-sums %-28s worst |error| / tolerance = %.3f  (n = %d)" % (producer, worst, fin.n))


# ---- the graph back-ends' per-link blocks (lum6DQuat, ghelix6DQ2, gapx6D) -----------------------------------------------
# Two forms per back-end.  The REFERENCE form evaluates the reference's own formulas term by term over the pair list in
# np.longdouble: its values are what both the library and the reference are compared with.  Run over `VE` -- E for a whole
# column of pairs at once, every +, -, * charged one rounding u |r| exactly as E does, halving free -- the same program
# gives the tolerance of the reference itself: a pair's term carries the roundings it was computed with, and a left-to-right
# fp64 sum of n of them is within gamma(n-1) sum |t| + sum e_t of their exact sum (Higham 4.2 again; no count is written
# down by hand, the class counts).  The LIBRARY form starts from `finished` -- finish_sums' outputs with their tolerances
# -- and runs the algebra of tdtk_graph_link_blocks (api_graph.cpp), operation by operation, over E.
# Inverses: both newmat's MM.i() (Crout LU, partial pivoting) and the library's invert_dense (Gauss-Jordan, partial pivoting)
# are modelled by the Gauss-Jordan sweep of `_invert_E`; the first-order bound of one elimination with partial pivoting
# stands for the other, whose operations are the same multiplications and subtractions in another order.
class VE:
    """values v[n] and first-order error bounds of a column of fp64 results (0-d arrays for scalars).  The bound has two
    parts: e[n], the roundings, which add up in absolute value; and g[3][n], what an error of the three coordinates of one
    shared input -- the centroid gapx6D centres on -- does to the result, signed and already multiplied by that input's own
    bound, so that it cancels over a sum as the real thing does ((p1 - c) - (p2 - c) does not depend on c at all)."""
    __slots__ = ("v", "e", "g")

    def __init__(self, v, e=None, g=None):
        self.v = np.asarray(v, LD)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, LD)
        self.g = g

    @staticmethod
    def of(x):
        if isinstance(x, VE):
            return x
        if isinstance(x, E):
            return VE(x.v, x.e)
        return VE(x)

    @staticmethod
    def shared(value, bound, axis):
        """coordinate `axis` of the shared input: exact value, error up to `bound`"""
        g = [LD(0), LD(0), LD(0)]
        g[axis] = LD(bound)
        return VE(value, None, g)

    @staticmethod
    def _g(a, fa, b, fb):
        if a.g is None and b.g is None:
            return None
        za = a.g if a.g is not None else [LD(0)] * 3
        zb = b.g if b.g is not None else [LD(0)] * 3
        return [fa * za[k] + fb * zb[k] for k in range(3)]

    def __add__(self, o):
        o = VE.of(o)
        v = self.v + o.v
        return VE(v, self.e + o.e + U * np.abs(v), VE._g(self, 1, o, 1))
    __radd__ = __add__

    def __neg__(self):
        return VE(-self.v, self.e, None if self.g is None else [-x for x in self.g])

    def __sub__(self, o):
        return self + (-VE.of(o))

    def __rsub__(self, o):
        return VE.of(o) + (-self)

    def __mul__(self, o):
        o = VE.of(o)
        v = self.v * o.v
        return VE(v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + U * np.abs(v), VE._g(self, o.v, o, self.v))
    __rmul__ = __mul__

    def half(self):
        return VE(self.v / 2, self.e / 2, None if self.g is None else [x / 2 for x in self.g])          # exact in fp64

    def sum(self):
        """a left-to-right (or any other) fp64 sum of the column -> E"""
        n = self.v.size
        shared = sum(abs(np.sum(np.broadcast_to(x, self.v.shape))) for x in self.g) if self.g is not None else 0
        return E(self.v.sum(), self.e.sum() + gamma(n - 1) * np.abs(self.v).sum() + shared)


def _invert_E(a, n):
    """Gauss-Jordan with partial pivoting (invert_dense, linalg.cpp) over E: a [n][n] of E -> inverse [n][n] of E"""
    a = [row[:] for row in a]
    b = [[E(1.0 if r == c else 0.0) for c in range(n)] for r in range(n)]
    for c in range(n):
        piv = max(range(c, n), key=lambda r: (abs(a[r][c].v), -r))
        if piv != c:
            a[piv], a[c] = a[c], a[piv]; b[piv], b[c] = b[c], b[piv]
        inv = 1.0 / a[c][c]
        for r in range(n):
            if r == c:
                continue
            f = a[r][c] * inv
            if f.v == 0:
                continue
            for k in range(n):
                a[r][k] = a[r][k] - f * a[c][k]
                b[r][k] = b[r][k] - f * b[c][k]
        for k in range(n):
            a[c][k] = a[c][k] * inv
            b[c][k] = b[c][k] * inv
    return b


def _matvec_E(M, x, n):
    out = []
    for r in range(n):
        v = E(0.0)
        for k in range(n):
            v = v + M[r][k] * x[k]
        out.append(v)
    return out


def _keep(p1, p2, drop):
    p1 = np.asarray(p1, float).reshape(-1, 3); p2 = np.asarray(p2, float).reshape(-1, 3)
    if drop is not None:
        k = np.ones(len(p1), bool); k[drop] = False
        p1, p2 = p1[k], p2[k]
    return p1, p2


def _quat_MM(m, sx, sy, sz, xpypz, ypz, xpz, xpy, xy, xz, yz):
    """lum6Dquat.cc:167-188 / api_graph.cpp: the symmetric 7 x 7 MM from its sums (E values)"""
    MM = [[E(0.0) for _ in range(7)] for _ in range(7)]

    def put(r, c, v):
        MM[r][c] = v; MM[c][r] = v
    put(0, 0, E(float(m))); put(1, 1, E(float(m))); put(2, 2, E(float(m)))
    put(3, 3, xpypz); put(4, 4, ypz); put(5, 5, xpz); put(6, 6, xpy)
    put(0, 3, sx); put(0, 5, -sz); put(0, 6, sy)
    put(1, 3, sy); put(1, 4, sz); put(1, 6, -sx)
    put(2, 3, sz); put(2, 4, -sy); put(2, 5, sx)
    put(4, 5, -xy); put(4, 6, -xz); put(5, 6, -yz)
    return MM


class Link:
    """q[name]: list of E (value, tolerance); n: pairs; ss (lum6DQuat only): E"""

    def __init__(self, n):
        self.n = n; self.q = {}; self.ss = None

    def values(self, name):
        return np.array([x.v for x in self.q[name]], LD)

    def tols(self, name):
        return np.array([x.e for x in self.q[name]], LD)


def quat_link(p1, p2, drop=None):
    """REFERENCE form of lum6DQuat::covarianceQuat (lum6Dquat.cc:129-215): C (49), CD (7) and MM, MZ, ss, term by term
    and in the reference's order of operations.  None for n <= 2."""
    p1, p2 = _keep(p1, p2, drop)
    m = len(p1)
    L = Link(m)
    if m <= 2:
        return L
    ak = [VE(p1[:, a]) for a in range(3)]; bk = [VE(p2[:, a]) for a in range(3)]
    x, y, z = [(ak[a] + bk[a]).half() for a in range(3)]
    dx, dy, dz = [ak[a] - bk[a] for a in range(3)]
    sx, sy, sz = x.sum(), y.sum(), z.sum()
    xpy = (x * x + y * y).sum(); xpz = (x * x + z * z).sum(); ypz = (y * y + z * z).sum()
    xpypz = (x * x + y * y + z * z).sum()
    xy = (x * y).sum(); xz = (x * z).sum(); yz = (y * z).sum()
    MZ = [dx.sum(), dy.sum(), dz.sum(), (x * dx + y * dy + z * dz).sum(), (z * dy - y * dz).sum(), (x * dz - z * dx).sum(),
          (y * dx - x * dy).sum()]
    MM = _quat_MM(m, sx, sy, sz, xpypz, ypz, xpz, xpy, xy, xz, yz)
    D = [VE.of(d) for d in _matvec_E(_invert_E(MM, 7), MZ, 7)]
    e0 = dx - (D[0] + x * D[3] - z * D[5] + y * D[6])
    e1 = dy - (D[1] + y * D[3] + z * D[4] - x * D[6])
    e2 = dz - (D[2] + z * D[3] - y * D[4] + x * D[5])
    ss = (e0 * e0 + e1 * e1 + e2 * e2).sum() / (2.0 * m - 3.0)
    L.ss = ss
    L.q["MM"] = [v for row in MM for v in row]; L.q["MZ"] = MZ
    if ss.v > 0:
        si = 1.0 / ss
        L.q["C"] = [v * si for v in L.q["MM"]]; L.q["CD"] = [v * si for v in MZ]
    return L


def euler_link(p1, p2, drop=None):
    """REFERENCE form of lum6DEuler::covarianceEuler (lum6Deuler.cc:141-232): C (36), CD (6), MM, MZ, ss; below the guard
    `ss < 1e-13` there is no C (the reference hands out zeros)"""
    p1, p2 = _keep(p1, p2, drop)
    m = len(p1)
    L = Link(m)
    if m <= 2:
        return L
    ak = [VE(p1[:, a]) for a in range(3)]; bk = [VE(p2[:, a]) for a in range(3)]
    x, y, z = [(ak[a] + bk[a]).half() for a in range(3)]
    dx, dy, dz = [ak[a] - bk[a] for a in range(3)]
    sx, sy, sz = x.sum(), y.sum(), z.sum()
    xpy = (x * x + y * y).sum(); xpz = (x * x + z * z).sum(); ypz = (y * y + z * z).sum()
    xy = (x * y).sum(); xz = (x * z).sum(); yz = (y * z).sum()
    MZ = [dx.sum(), dy.sum(), dz.sum(), (-z * dy + y * dz).sum(), (-y * dx + x * dy).sum(), (z * dx - x * dz).sum()]
    MM = [[E(0.0) for _ in range(6)] for _ in range(6)]

    def put(r, c, v):
        MM[r][c] = v; MM[c][r] = v
    put(0, 0, E(float(m))); put(1, 1, E(float(m))); put(2, 2, E(float(m)))
    put(3, 3, ypz); put(4, 4, xpy); put(5, 5, xpz)
    put(0, 4, -sy); put(0, 5, sz); put(1, 3, -sz); put(1, 4, sx); put(2, 3, sy); put(2, 5, -sx)
    put(3, 4, -xz); put(3, 5, -xy); put(4, 5, -yz)
    D = [VE.of(d) for d in _matvec_E(_invert_E(MM, 6), MZ, 6)]
    e0 = dx - (D[0] - y * D[4] + z * D[5])
    e1 = dy - (D[1] - z * D[3] + x * D[4])
    e2 = dz - (D[2] + y * D[3] - x * D[5])
    ss = (e0 * e0 + e1 * e1 + e2 * e2).sum() / (2.0 * m - 3.0)
    L.ss = ss
    L.q["MM"] = [v for row in MM for v in row]; L.q["MZ"] = MZ
    if ss.v >= 0.0000000000001:
        si = 1.0 / ss
        L.q["C"] = [v * si for v in L.q["MM"]]; L.q["CD"] = [v * si for v in MZ]
    return L


def quat_link_lib(p1, p2, shift, drop=None, full=None):
    """LIBRARY form: finish_sums (want LUM), then tdtk_graph_link_blocks' lum6DQuat branch: MM[3][3] from the three
    second-moment sums halved, ss from the normal equations (sum - D . MZ) / (2m - 3) through invert_dense"""
    fin = finished(p1, p2, None, shift, WANT_LUM, None, drop, full)
    m = fin.n
    L = Link(m); L.fin = fin
    if m <= 2:
        return L
    lum = [E(v, e) for v, e in zip(fin.ref["lum"], fin.tol["lum"])]
    udot = E(fin.ref["lum_udot"][0], fin.tol["lum_udot"][0]); ssum = E(fin.ref["sum"][0], fin.tol["sum"][0])
    sx, sy, sz, xpy, xpz, ypz, xy, xz, yz = lum[:9]
    MZ = [lum[9], lum[10], lum[11], udot, -lum[12], -lum[14], -lum[13]]
    MM = _quat_MM(m, sx, sy, sz, (xpy + xpz + ypz) / 2.0, ypz, xpz, xpy, xy, xz, yz)
    D = _matvec_E(_invert_E(MM, 7), MZ, 7)
    dmz = E(0.0)
    for r in range(7):
        dmz = dmz + D[r] * MZ[r]
    ss = (ssum - dmz) / (2.0 * float(m) - 3.0)
    L.ss = ss
    L.q["MM"] = [v for row in MM for v in row]; L.q["MZ"] = MZ
    if ss.v > 0:
        L.q["C"] = [v / ss for v in L.q["MM"]]; L.q["CD"] = [v / ss for v in MZ]
    return L


def helix_link(p1, p2, drop=None):
    """REFERENCE form of ghelix6DQ2::genBBdForLinkedPair (ghelix6DQ2.cc:107-150): Blk (36, the block the scatter adds),
    bd1 (6), bd2 (6)"""
    p1, p2 = _keep(p1, p2, drop)
    n = len(p1)
    L = Link(n)
    a = [VE(p1[:, k]) for k in range(3)]; b = [VE(p2[:, k]) for k in range(3)]
    p1x, p1y, p1z = a; p2x, p2y, p2z = b
    px2, py2, pz2 = p2x * p2x, p2y * p2y, p2z * p2z
    b40, b50, b42 = (-p2z).sum(), p2y.sum(), p2x.sum()
    b00, b10, b20 = (pz2 + py2).sum(), (p2y * -p2x).sum(), (-p2z * p2x).sum()
    b11, b21, b22 = (pz2 + px2).sum(), (p2z * -p2y).sum(), (px2 + py2).sum()
    dX, dY, dZ = p1x - p2x, p1y - p2y, p1z - p2z
    bd1 = [(-p1z * dY + p1y * dZ).sum(), (p1z * dX - p1x * dZ).sum(), (-p1y * dX + p1x * dY).sum(), dX.sum(), dY.sum(), dZ.sum()]
    bd2 = [(-p2z * -dY + p2y * -dZ).sum(), (p2z * -dX - p2x * -dZ).sum(), (-p2y * -dX + p2x * -dY).sum(), (-dX).sum(),
           (-dY).sum(), (-dZ).sum()]
    B = [[E(0.0) for _ in range(6)] for _ in range(6)]

    def put(r, c, v):
        B[r][c] = v; B[c][r] = v
    for k in (3, 4, 5):
        B[k][k] = E(float(n))
    put(0, 4, b40); put(1, 3, -b40); put(0, 5, b50); put(2, 3, -b50); put(2, 4, b42); put(1, 5, -b42)
    put(0, 1, b10); put(0, 2, b20); put(1, 2, b21)
    B[0][0], B[1][1], B[2][2] = b00, b11, b22
    L.q["Blk"] = [v for row in B for v in row]; L.q["bd1"] = bd1; L.q["bd2"] = bd2
    return L


def helix_link_lib(p1, p2, shift, drop=None, full=None):
    """LIBRARY form: finish_sums (want MOM2), then the ghelix6DQ2 branch: raw moments as centred + m c c^T, bd1 the
    antisymmetric part of Si + m cm cd^T; bd2 is not computed, the scatter uses -bd1"""
    fin = finished(p1, p2, None, shift, WANT_MOM2, None, drop, full)
    n = fin.n
    L = Link(n); L.fin = fin
    if n <= 1:
        return L

    def Es(name):
        return [E(v, e) for v, e in zip(fin.ref[name], fin.tol[name])]
    cm, cd, dd, Si = Es("centroid_m"), Es("centroid_d"), Es("mom_dd"), Es("Si")
    m = float(n)
    ddm = [[dd[0], dd[1], dd[2]], [dd[1], dd[3], dd[4]], [dd[2], dd[4], dd[5]]]
    DD = [[ddm[r][c] + m * cd[r] * cd[c] for c in range(3)] for r in range(3)]
    X = [[Si[r * 3 + c] + m * cm[r] * cd[c] for c in range(3)] for r in range(3)]
    s2 = [m * cd[k] for k in range(3)]
    B = [[E(0.0) for _ in range(6)] for _ in range(6)]

    def put(r, c, v):
        B[r][c] = v; B[c][r] = v
    for k in (3, 4, 5):
        B[k][k] = E(m)
    put(0, 4, -s2[2]); put(1, 3, s2[2]); put(0, 5, s2[1]); put(2, 3, -s2[1]); put(2, 4, s2[0]); put(1, 5, -s2[0])
    put(0, 1, -DD[0][1]); put(0, 2, -DD[0][2]); put(1, 2, -DD[1][2])
    B[0][0], B[1][1], B[2][2] = DD[2][2] + DD[1][1], DD[2][2] + DD[0][0], DD[0][0] + DD[1][1]
    bd1 = [X[2][1] - X[1][2], X[0][2] - X[2][0], X[1][0] - X[0][1]] + [m * (cm[k] - cd[k]) for k in range(3)]
    L.q["Blk"] = [v for row in B for v in row]; L.q["bd1"] = bd1; L.q["bd2"] = [-v for v in bd1]
    return L


def centroids(p1, p2, drop=None):
    """the pair list's centroids as Scan::getPtPairs forms them (a running fp64 sum, then one division): E values about
    the exact centroid"""
    p1, p2 = _keep(p1, p2, drop)
    n = len(p1)
    out = []
    for p in (p1, p2):
        out.append([VE(p[:, a]).sum() / float(n) for a in range(3)] if n else [E(0.0)] * 3)
    return out


def gapx_link(p1, p2, drop=None):
    """REFERENCE form of gapx6D::genBArotForLinkedPair (gapx6D.cc:184-275), both points centred on centroids_m -- the
    centroid as an E value, so that what its own rounding does to every term is part of the tolerance: MkMkt, DkDkt, MkDkt,
    DkMkt (9 each, `p1x * p2x + p1y + p2y` as written), Ak1, Ak2, cm, cd"""
    p1, p2 = _keep(p1, p2, drop)
    n = len(p1)
    L = Link(n)
    cm, cd = centroids(p1, p2)
    L.q["cm"] = cm; L.q["cd"] = cd
    if n == 0:
        return L
    c = [VE.shared(cm[a].v, cm[a].e, a) for a in range(3)]
    p1x, p1y, p1z = [VE(p1[:, a]) - c[a] for a in range(3)]
    p2x, p2y, p2z = [VE(p2[:, a]) - c[a] for a in range(3)]
    p1x2, p1y2, p1z2, p2x2, p2y2, p2z2 = p1x * p1x, p1y * p1y, p1z * p1z, p2x * p2x, p2y * p2y, p2z * p2z
    d33 = (p1x * p2x + p1y + p2y).sum(); d22 = (p1x * p2x + p1z + p2z).sum(); d11 = (p1y * p2y + p1z + p2z).sum()
    m01, m02, m12 = -(p1x * p1y).sum(), -(p1x * p1z).sum(), -(p1y * p1z).sum()
    e01, e02, e12 = -(p2x * p2y).sum(), -(p2x * p2z).sum(), -(p2y * p2z).sum()
    L.q["MkMkt"] = [(p1y2 + p1z2).sum(), m01, m02, m01, (p1x2 + p1z2).sum(), m12, m02, m12, (p1x2 + p1y2).sum()]
    L.q["DkDkt"] = [(p2y2 + p2z2).sum(), e01, e02, e01, (p2x2 + p2z2).sum(), e12, e02, e12, (p2x2 + p2y2).sum()]
    a01, a02, a12 = -(p1y * p2x).sum(), -(p1z * p2x).sum(), -(p1z * p2y).sum()
    c01, c02, c12 = -(p2y * p1x).sum(), -(p2z * p1x).sum(), -(p2z * p1y).sum()
    L.q["MkDkt"] = [d11, a01, a02, a01, d22, a12, a02, a12, d33]
    L.q["DkMkt"] = [d11, c01, c02, c01, d22, c12, c02, c12, d33]
    L.q["Ak1"] = [-(((p1z - p2z) * p2y - (p1y - p2y) * p2z).sum()), -(((p1x - p2x) * p2z - (p1z - p2z) * p2x).sum()),
                  -(((p1y - p2y) * p2x - (p1x - p2x) * p2y).sum())]
    L.q["Ak2"] = [((p1z - p2z) * p1y - (p1y - p2y) * p1z).sum(), ((p1x - p2x) * p1z - (p1z - p2z) * p1x).sum(),
                  ((p1y - p2y) * p1x - (p1x - p2x) * p1y).sum()]
    return L


def gapx_link_lib(p1, p2, shift, drop=None, full=None):
    """LIBRARY form: finish_sums (want GAPX) hands out the blocks as they are copied into the link block"""
    fin = finished(p1, p2, None, shift, WANT_GAPX, None, drop, full)
    L = Link(fin.n); L.fin = fin
    for name, f in (("cm", "centroid_m"), ("cd", "centroid_d"), ("MkMkt", "gapx_MkMkt"), ("DkDkt", "gapx_DkDkt"),
                    ("MkDkt", "gapx_MkDkt"), ("DkMkt", "gapx_DkMkt"), ("Ak1", "gapx_Ak1"), ("Ak2", "gapx_Ak2")):
        L.q[name] = [E(v, e) for v, e in zip(fin.ref[f], fin.tol[f])]
    return L


REF_LINK = {1: euler_link, 2: quat_link, 3: helix_link, 4: gapx_link}
LIB_LINK = {2: quat_link_lib, 3: helix_link_lib, 4: gapx_link_lib}
