"""Tolerances for tdtk_hough_fit_plane against the reference's calcPlane (hough.cc:1252-1310), derived, not chosen.

Both sides compute, from the same doubles p_i (n points),

    c    = (sum_i p_i) / n                               the centroid, per axis
    A_ab = sum_i (a_i - c_a) (b_i - c_b)                 the six centred second moments
    (w, V) = eig(A);  k = argmin |w|;  normal = V[:, k];  plane[3] = normal . c;  planarity = w_k / (w_1 + w_2 + w_3)

in fp64 -- the reference sequentially, the device lane-strided, then a tree per workgroup, then block by block.  u = 2^-53,
g(m) = m u / (1 - m u).  The rule is tests/pair_sums_ref.py's: any order of n fp64 additions is within g(n-1) * (sum of the
absolute terms) of the exact sum of the terms it was handed (Higham, Accuracy and Stability, 4.2), and a term computed with
r roundings is within r u |term| of the exact term.  The bound is applied to BOTH sides, since the reference's sequential sum
obeys it too: every tolerance below is the sum of the two sides' bounds, i.e. twice one side's.

Centroid.  One side: |c^ - c| <= dc := g(n-1) (sum_i |a_i|) / n + u |c| (the sum, then one division).

Moments.  With the side's own c^ = c + d: each term is (a_i - c^_a) (one rounding), (b_i - c^_b) (one), their product (one):
3 roundings; the sum adds g(n-1).  And exactly, sum_i (a_i - c_a - d_a)(b_i - c_b - d_b) = A_ab + n d_a d_b, because the sums
of the centred coordinates vanish at the true centroid.  So one side is within

    dA_ab := (g(n-1) + 3 u) * sum_i |a_i - c_a| |b_i - c_b| * (1 + 1e-9) + n dc_a dc_b

of the exact A_ab (the factor covers taking the absolute sum at c instead of c^).  ||dA||_2 <= ||dA||_F =: one side's dM.

Eigen-decomposition.  Both solvers are cyclic Jacobi on a 3 x 3: a rotation perturbs the matrix by at most 8 u ||A||_F
(Wilkinson, The Algebraic Eigenvalue Problem, ch. 5, 3: plane rotations in floating point), a sweep has 3 rotations, and
neither solver needs more than 10 sweeps on a 3 x 3 (quadratic convergence; linalg.cpp stops at off^2 <= 1e-40 diag^2): each
side's computed eigenpairs are exact for a matrix within dJ := 240 u ||A||_F of the one it was handed.  Per side E := dM + dJ;
the two computed decompositions are exact for matrices 2 E apart.

Normal.  Davis-Kahan: the angle t between the two sides' eigenvectors of the smallest eigenvalue has sin t <= 2 E / (gap - 2 E),
gap = w_mid - w_min of the exact A (the fixture's planes have gap >= 0.1 w_max, so the bound means something).  For unit
vectors at angle t <= pi / 2, ||n - n'||_2 = 2 sin(t / 2) <= sqrt(2) sin t; each solver normalises to within 4 u.  Up to sign:
    tol_normal = sqrt(2) * 2 E / (gap - 2 E) + 8 u            (on every component, since |dn_a| <= ||dn||_2)
plane[3] = n . c with both sides' n and c: |d| <= tol_normal * ||c||_2 + ||(2 dc)||_2 + 2 * 3 u * sum_a |n_a c_a|.
Planarity f = w_k / T, T = trace.  Weyl: |dw_k| <= 2 E; |dT| <= 3 * 2 E.  Then
    tol_planarity = (2 E * T + |w_k| * 6 E) / (T * (T - 6 E)) + 4 u |f|.
"""
import numpy as np

U = 2.0 ** -53


def g(m):
    return m * U / (1 - m * U)


def bounds(points):
    """points [n][3] float64 (n >= 3) -> dict: tol_normal, tol_d, tol_planarity, and the exact-side quantities they rest on"""
    p = np.asarray(points, np.longdouble)
    n = len(p)
    c = p.sum(axis=0) / n
    dc = np.array([g(n - 1) * float(np.abs(p[:, a]).sum()) / n + U * abs(float(c[a])) for a in range(3)])
    q = p - c
    A = np.array((q.T @ q), np.float64)
    absq = np.abs(q).astype(np.float64)
    dA = np.zeros((3, 3))
    for a in range(3):
        for b in range(3):
            dA[a, b] = (g(n - 1) + 3 * U) * float((absq[:, a] * absq[:, b]).sum()) * (1 + 1e-9) + n * dc[a] * dc[b]
    dM = float(np.linalg.norm(dA))
    normA = float(np.linalg.norm(A))
    E = dM + 240 * U * normA
    w = np.linalg.eigvalsh(A)
    k = np.argsort(np.abs(w))
    wk, wmid, wmax = w[k[0]], np.abs(w)[k[1]], np.abs(w)[k[2]]
    gap = wmid - abs(wk)
    assert gap > 4 * E, "no bound without a gap"
    T = float(w.sum())
    tol_normal = np.sqrt(2.0) * 2 * E / (gap - 2 * E) + 8 * U
    cf = np.array(c, np.float64)
    tol_d = tol_normal * float(np.linalg.norm(cf)) + float(np.linalg.norm(2 * dc)) + 6 * U * float(np.abs(cf).sum())
    tol_planarity = (2 * E * T + abs(wk) * 6 * E) / (T * (T - 6 * E)) + 4 * U * abs(wk / T)
    return dict(tol_normal=float(tol_normal), tol_d=float(tol_d), tol_planarity=float(tol_planarity), E=E, gap=float(gap),
                rel_gap=float(gap / wmax))
