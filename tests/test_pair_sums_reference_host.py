"""CPU tier of the pair-sum reference (tests/pair_sums_ref.py): the long-double sums against exact rationals, the oracle's
own fp64 sums inside the derived tolerance, every asserted quantity discriminating at the GPU tier's sizes, and the bound
about the accumulation point against the bound about the origin for a cloud far away."""
from fractions import Fraction as F

import numpy as np
import pytest

import pair_sums_ref as R

KERNEL_WANTS = list(range(8)) + [R.WANT_GAPX, R.WANT_LUM | R.NO_CROSS]
PUBLIC_WANTS = list(range(8)) + [R.WANT_GAPX, R.WANT_MOM2]
LUM_D = [0.02, -0.01, 0.015, 1e-4, -2e-4, 1.5e-4]


def _pairs(orc, N, pattern="all", far=False, mode=0, seed=1):
    c = R.make_inputs(N, pattern, far, seed)
    T = orc.Tree(c["model"], 20)
    md2 = c["maxd2"] if mode != 1 or pattern == "none" else 0.5
    ref = T.get_pt_pairs(c["A"], c["d"], c["nr"], 0, N, mode, md2)
    if mode == 0:
        ref["pn"] = R.unit_normals(c["nr"][ref["idx"] >= 0])
    return c, ref, R.shift_of(c["model"], c["A"])


def _exact_columns(p1, p2, pn, shift, want, D):
    """the columns in exact rational arithmetic over the same doubles, written out pair by pair"""
    S = [F(0)] * R.ACC_TOTAL
    A = [F(0)] * R.ACC_TOTAL                 # sum of |term| (what the comparison is relative to)
    sh = [F(float(s)) for s in shift]
    Dq = [F(float(x)) for x in D] if D is not None else None

    def add(k, t):
        S[k] += t; A[k] += abs(t)
    for i in range(len(p1)):
        m = [F(float(v)) for v in p1[i]]; t = [F(float(v)) for v in p2[i]]; nn = [F(float(v)) for v in pn[i]]
        p = [m[a] - t[a] for a in range(3)]
        ms = [m[a] - sh[a] for a in range(3)]; ds = [t[a] - sh[a] for a in range(3)]
        add(R.ACC_N, F(1)); add(R.ACC_SUM, sum(x * x for x in p))
        if not want & R.NO_CROSS:
            for a in range(3):
                add(R.ACC_SM + a, ms[a]); add(R.ACC_SD + a, ds[a])
                for b in range(3):
                    add(R.ACC_P + 3 * a + b, ms[a] * ds[b])
        up = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
        if want & R.WANT_GAPX:
            for q, (a, b) in enumerate(up):
                add(R.ACC_MM + q, ms[a] * ms[b])
        if want & (R.WANT_APX | R.WANT_GAPX):
            for q, (a, b) in enumerate(up):
                add(R.ACC_DD + q, ds[a] * ds[b])
        if want & R.WANT_NAPX:
            v = [ds[1] * nn[2] - ds[2] * nn[1], ds[2] * nn[0] - ds[0] * nn[2], ds[0] * nn[1] - ds[1] * nn[0]] + nn
            q = 0
            for r in range(6):
                for s in range(r, 6):
                    add(R.ACC_NA + q, v[r] * v[s]); q += 1
                add(R.ACC_NB + r, v[r])
            add(R.ACC_NS, sum(p[a] * nn[a] for a in range(3)) ** 2)
        if want & R.WANT_LUM:
            x, y, z = [(m[a] + t[a]) / 2 for a in range(3)]
            dx, dy, dz = p
            for k, w in enumerate([x, y, z, x * x + y * y, x * x + z * z, y * y + z * z, x * y, x * z, y * z, dx, dy, dz,
                                   -z * dy + y * dz, -y * dx + x * dy, z * dx - x * dz]):
                add(R.ACC_L + k, w)
            add(R.ACC_LU, x * dx + y * dy + z * dz)
            if Dq is not None:
                e0 = dx - (Dq[0] - y * Dq[4] + z * Dq[5]); e1 = dy - (Dq[1] - z * Dq[3] + x * Dq[4])
                e2 = dz - (Dq[2] + y * Dq[3] - x * Dq[5])
                add(R.ACC_LSS, e0 * e0 + e1 * e1 + e2 * e2)
    return S, A


@pytest.mark.parametrize("want", KERNEL_WANTS + ["lum_D"])
def test_long_double_sums_equal_exact_rationals(orc, want):
    D = LUM_D if want == "lum_D" else None
    want = R.WANT_LUM if want == "lum_D" else want
    _, ref, shift = _pairs(orc, 330)
    p1, p2, pn = ref["p1"][:300], ref["p2"][:300], ref["pn"][:300]
    assert len(p1) == 300
    raw = R.raw_sums(p1, p2, pn, shift, want, D)
    S, A = _exact_columns(p1, p2, pn, shift, want, D)
    for k in range(R.ACC_TOTAL):
        if not raw.used[k]:
            assert S[k] == 0 and raw.S[k] == 0, k
            continue
        # a long double holds 64 bits: S_k as two doubles is exact enough to compare at 2^-60
        hi = float(raw.S[k]); lo = float(raw.S[k] - R.LD(hi))
        err = abs(F(hi) + F(lo) - S[k])
        assert err <= F(1, 2 ** 60) * A[k], (k, float(err), float(A[k]))
        assert F(float(raw.M[k])) >= A[k] * (1 - F(1, 2 ** 50)), k          # M_k majorises sum |t|


def test_oracle_fp64_sums_lie_inside_the_derived_tolerance(orc):
    """the 38 900-query case of test_get_pt_pairs_vs_oracle: the oracle adds in query order about the origin"""
    rng = np.random.default_rng(8)
    m = rng.uniform(-200, 200, (60000, 3)); m[100:160] = m[0:60]
    A = R.rigid([12.0, -7.0, 3.0], [0.03, -0.02, 0.04])
    d = R.apply(A, m[rng.permutation(len(m))[:40000]]) + rng.normal(0, 0.4, (40000, 3))
    ref = orc.Tree(m, 20).get_pt_pairs(A, d, None, 100, 39000, 0, 4.0)
    assert ref["n"] > 1000
    raw = R.raw_sums(ref["p1"], ref["p2"], None, [0.0, 0.0, 0.0], 0)
    tol = raw.tol
    assert abs(R.LD(ref["sum"]) - raw.S[R.ACC_SUM]) <= tol[R.ACC_SUM]
    for a in range(3):
        assert abs(R.LD(ref["centroid_m"][a]) - raw.S[R.ACC_SM + a]) <= tol[R.ACC_SM + a]
        assert abs(R.LD(ref["centroid_d"][a]) - raw.S[R.ACC_SD + a]) <= tol[R.ACC_SD + a]
    # and the tolerance means something: it is a few 1e-12 of the sum
    assert tol[R.ACC_SUM] < 1e-11 * raw.S[R.ACC_SUM]


# the largest n each kind of case has in the GPU tier: base sums in pairing mode 0 with every query paired up to the
# hand-over to k_accum (28 * 256 * 256 queries on 256 CUs), anything else in mode 0 up to 300 001, pairing modes 1 and 2
# at 5 001
N_GPU_BASE, N_GPU_WANT, N_GPU_MODES = 2000000, 300001, 5001


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("pattern", ["all", "half"])
def test_every_quantity_discriminates_at_the_gpu_sizes(orc, mode, pattern):
    """move / tolerance of a raw column goes as 1 / n^2 (the move is one term, the tolerance n u sum |t|): measured at a
    reduced n, asserted extrapolated to the GPU tier's n"""
    N = 3000
    c, ref, shift = _pairs(orc, N, pattern, mode=mode)
    n = ref["n"]
    assert n > 500
    for want in PUBLIC_WANTS + ["lum_D"]:
        D = LUM_D if want == "lum_D" else None
        w = R.WANT_LUM if want == "lum_D" else want
        n_gpu = N_GPU_MODES if mode else (N_GPU_BASE if (w == 0 and pattern == "all") else N_GPU_WANT)
        ratios = R.discrimination(ref["p1"], ref["p2"], ref["pn"], shift, w, D)
        assert ratios
        for name, r in ratios.items():
            assert r * (n / n_gpu) ** 2 >= 10.0, (want, name, r)


def test_links_quantities_discriminate(orc):
    _, ref, _ = _pairs(orc, 3000)
    (m, MM, MZ, ss), (m2, MM2, MZ2, ss2) = R.lum_link_and_one_less(ref["p1"], ref["p2"])
    scale = (m / N_GPU_WANT) ** 2
    assert m2 == m - 1
    for a, b in zip(MM + MZ + [ss], MM2 + MZ2 + [ss2]):
        if a.e > 0:
            assert abs(a.v - b.v) / a.e * scale >= 10.0


def test_the_shift_is_what_makes_a_far_cloud_checkable(orc):
    """cloud and pose offset by 1e6: relative to the finished Si, the bound about the accumulation point is at least 1e6
    times tighter than the bound about the origin -- a kernel that dropped the shift (or applied it on one side) could
    not stay inside the former"""
    c, ref, shift = _pairs(orc, 3000, far=True)
    assert ref["n"] > 2000 and np.abs(shift).min() > 9e5
    about_shift = R.finished(ref["p1"], ref["p2"], ref["pn"], shift, 0)
    about_origin = R.finished(ref["p1"], ref["p2"], ref["pn"], [0.0, 0.0, 0.0], 0)
    si = np.abs(about_shift.ref["Si"])
    assert np.all(np.abs(about_shift.ref["Si"] - about_origin.ref["Si"]) <= about_origin.tol["Si"])
    assert np.all(about_origin.tol["Si"] / si >= 1e6 * about_shift.tol["Si"] / si)
    assert all(r >= 10.0 for r in R.discrimination(ref["p1"], ref["p2"], ref["pn"], shift, 0, fin=about_shift).values())
