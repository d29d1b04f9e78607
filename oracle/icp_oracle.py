"""TEST INFRASTRUCTURE ONLY: numpy restatement of the tiny algebra around the hot path --
icp6Dminimizer::Align for all ten -a minimizers, the icp6D::match loop (serial-branch
semantics), the graph back-ends lum6DEuler / lum6DQuat / ghelix6DQ2 / gapx6D, Graph (also the
clpairs variant), Point_Point_Error, and the uos / .pose readers.
The heavy per-point work is done by oracle/oracle.c (oracle/orc.py).

Each function cites the reference file:line it follows.  PINNED by tests/test_oracle_vs_ref.py
against the reference's own minimizer TUs (oracle/_ref) and the committed fixtures in
tests/golden/: the ten minimizers and the match loop; by tests/test_graph_backends_reference_host.py
against k16_graph_backends.npz (the reference's own lum6Deuler.cc / lum6Dquat.cc / ghelix6DQ2.cc /
gapx6D.cc / graphSlam6D.cc, compiled by the fixture's generator): the graph back-ends' per-link
blocks, scatter rules, drop rule and pose updates.  PARITY UNPINNED (restated by reading):
CSparse's factorisation, the clpairs graph, Point_Point_Error.

The eigen / SVD / Cholesky kernels use numpy.linalg (LAPACK) where the reference uses a
closed-form quartic + LU (icp6Dquat.cc:405-513), newmat SVD and Numerical-Recipes Cholesky:
same mathematical result to ~1e-14, deliberately a different implementation from the product's
Jacobi solvers in 3dtk_amd/csrc/linalg.cpp.
"""
import math

import numpy as np

from . import orc

# ---------------------------------------------------------------------------------------
# globals.icc helpers
# ---------------------------------------------------------------------------------------


def euler_to_matrix4(rPos, rPosTheta):
    """globals.icc:501-531"""
    sx, cx = math.sin(rPosTheta[0]), math.cos(rPosTheta[0])
    sy, cy = math.sin(rPosTheta[1]), math.cos(rPosTheta[1])
    sz, cz = math.sin(rPosTheta[2]), math.cos(rPosTheta[2])
    a = np.zeros(16)
    a[0] = cy * cz
    a[1] = sx * sy * cz + cx * sz
    a[2] = -cx * sy * cz + sx * sz
    a[4] = -cy * sz
    a[5] = -sx * sy * sz + cx * cz
    a[6] = cx * sy * sz + sx * cz
    a[8] = sy
    a[9] = -sx * cy
    a[10] = cx * cy
    a[12:15] = rPos
    a[15] = 1
    return a


def matrix4_to_euler(alignxf):
    """globals.icc:541-576 -> (rPosTheta, rPos)"""
    th = [0.0, 0.0, 0.0]
    th[1] = math.asin(alignxf[8]) if alignxf[0] > 0.0 else math.pi - math.asin(alignxf[8])
    Cc = math.cos(th[1])
    if abs(Cc) > 0.005:
        th[0] = math.atan2(-alignxf[9] / Cc, alignxf[10] / Cc)
        th[2] = math.atan2(-alignxf[4] / Cc, alignxf[0] / Cc)
    else:
        th[0] = 0.0
        th[2] = math.atan2(alignxf[1], alignxf[5])
    return np.array(th), np.array(alignxf[12:15])


def _compose(R, cm, cd):
    """column-major 4x4 from row-major R and t = cm - R cd"""
    a = np.zeros(16)
    for r in range(3):
        for c in range(3):
            a[c * 4 + r] = R[r, c]
    a[12:15] = cm - R @ cd
    a[15] = 1
    return a


def _apx_rotation(x):
    """icp6Dapx.cc:104-122"""
    sx, sy, sz = x[0], x[1], x[2]
    cx, cy, cz = math.sqrt(1.0 - sx * sx), math.sqrt(1.0 - sy * sy), math.sqrt(1.0 - sz * sz)
    return np.array([[cy * cz, -cy * sz, sy],
                     [sx * sy * cz + cx * sz, -sx * sy * sz + cx * cz, -sx * cy],
                     [-cx * sy * cz + sx * sz, cx * sy * sz + sx * cz, cx * cy]])


def _choldc_solve(A, B):
    """choldc + cholsl (globals.icc:820-957): fails (None) when a pivot < 1e-7"""
    n = len(B)
    A = A.copy()
    diag = np.zeros(n)
    for i in range(n):
        for j in range(i, n):
            s = A[i, j] - sum(A[i, k] * A[j, k] for k in range(i - 1, -1, -1))
            if i == j:
                if s < 1.0e-7:
                    return None
                diag[i] = math.sqrt(s)
            else:
                A[j, i] = s / diag[i]
    x = np.zeros(n)
    for i in range(n):
        s = B[i] - sum(A[i, k] * x[k] for k in range(i - 1, -1, -1))
        x[i] = s / diag[i]
    for i in range(n - 1, -1, -1):
        s = x[i] - sum(A[k, i] * x[k] for k in range(i + 1, n))
        x[i] = s / diag[i]
    return x


# ---------------------------------------------------------------------------------------
# icp6Dminimizer::Align (serial), from explicit pair lists p1 (model), p2 (data)
# ---------------------------------------------------------------------------------------
def matrix4_to_quat(mat):
    """Matrix4ToQuat (globals.icc:1032-1075) -> (quat[4] = (W, -X, -Y, -Z) normalised, t[3])"""
    T = 1 + mat[0] + mat[5] + mat[10]
    if T > 0.00000001:
        S = math.sqrt(T) * 2
        X = (mat[9] - mat[6]) / S; Y = (mat[2] - mat[8]) / S; Z = (mat[4] - mat[1]) / S; W = 0.25 * S
    elif mat[0] > mat[5] and mat[0] > mat[10]:
        S = math.sqrt(1.0 + mat[0] - mat[5] - mat[10]) * 2
        X = 0.25 * S; Y = (mat[4] + mat[1]) / S; Z = (mat[2] + mat[8]) / S; W = (mat[9] - mat[6]) / S
    elif mat[5] > mat[10]:
        S = math.sqrt(1.0 + mat[5] - mat[0] - mat[10]) * 2
        X = (mat[4] + mat[1]) / S; Y = 0.25 * S; Z = (mat[9] + mat[6]) / S; W = (mat[2] - mat[8]) / S
    else:
        S = math.sqrt(1.0 + mat[10] - mat[0] - mat[5]) * 2
        X = (mat[2] + mat[8]) / S; Y = (mat[9] + mat[6]) / S; Z = 0.25 * S; W = (mat[4] - mat[1]) / S
    q = np.array([W, -X, -Y, -Z])
    return q / math.sqrt(float(q @ q)), np.array(mat[12:15], float)


def quat_to_matrix4(quat, t):
    """QuatToMatrix4 (globals.icc:988-1022), column-major"""
    q11, q22, q33 = quat[1] * quat[1], quat[2] * quat[2], quat[3] * quat[3]
    q03, q13, q23 = quat[0] * quat[3], quat[1] * quat[3], quat[2] * quat[3]
    q02, q12, q01 = quat[0] * quat[2], quat[1] * quat[2], quat[0] * quat[1]
    m = np.zeros(16)
    m[0] = 1 - 2 * (q22 + q33); m[5] = 1 - 2 * (q11 + q33); m[10] = 1 - 2 * (q11 + q22)
    m[4] = 2.0 * (q12 - q03); m[1] = 2.0 * (q12 + q03)
    m[8] = 2.0 * (q13 + q02); m[2] = 2.0 * (q13 - q02)
    m[9] = 2.0 * (q23 - q01); m[6] = 2.0 * (q23 + q01)
    m[12:15] = t
    m[15] = 1.0
    return m


def _skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], float)


def _rt_to_gl(R, t):
    a = np.zeros(16)
    for r in range(3):
        for c in range(3):
            a[c * 4 + r] = R[r, c]
    a[12:15] = t
    a[15] = 1.0
    return a


def _euler_T(x, th):
    """the 4x4 pose matrix both LUMEULER blocks write out (icp6Dlumeuler.cc:144-156, 184-196)"""
    cx, cy, cz = math.cos(th[0]), math.cos(th[1]), math.cos(th[2])
    sx, sy, sz = math.sin(th[0]), math.sin(th[1]), math.sin(th[2])
    T = np.eye(4)
    T[:3, 3] = x
    T[0, :3] = [cy * cz, -cy * sz, sy]
    T[1, :3] = [cz * sx * sy + cx * sz, cx * cz - sx * sy * sz, -cy * sx]
    T[2, :3] = [sx * sz - cx * cz * sy, cz * sx + cx * sy * sz, cx * cy]
    return T


def _quat_T(x, p, qv):
    """(p*p - q.q) I + 2 q q^T + 2 p [q]x with translation x (icp6Dlumquat.cc:168-180, 190-203)"""
    T = np.zeros((4, 4))
    T[:3, :3] = np.eye(3) * (p * p - float(qv @ qv)) + 2 * np.outer(qv, qv) + 2 * p * _skew(qv)
    T[:3, 3] = x
    T[3, 3] = 1
    return T


def _align_serial_only(algo, p1, p2, cm, cd, pose):
    """The minimizers that exist only as serial Align: -a 3 ORTHO, 4 DUAL, 5 HELIX, 7 LUMEULER,
    8 LUMQUAT, 9 QUAT_SCALE (slam6D.cc:703-723).  pose = alignxf on entry (current transMat for 7/8)."""
    n = len(p1)
    s = float(((p1 - p2) ** 2).sum())
    rms = math.sqrt(s / n)
    if algo == 3:   # icp6Dortho.cc:40-157
        H = (p1 - cm).T @ (p2 - cd)
        w, V = np.linalg.eigh(H.T @ H)
        R = H @ sum(np.outer(V[:, k], V[:, k]) / math.sqrt(w[k]) for k in range(3))
        return rms, _rt_to_gl(R, cm - R @ cd)
    if algo == 4:   # icp6Ddual.cc:41-152
        C1 = np.zeros((4, 4)); C2 = np.zeros((4, 4))
        md = p1.T @ p2                                   # sum m d^T
        cr = np.cross(p1, p2).sum(axis=0)                # m^T [d]x = (m x d)^T ; [m]x d = m x d
        C1[0, 0] = np.trace(md)
        C1[0, 1:] = -cr
        C1[1:, 0] = -cr
        C1[1:, 1:] = md + md.T - np.trace(md) * np.eye(3)   # m d^T + [m]x [d]x
        sm, sd = p1.sum(axis=0), p2.sum(axis=0)
        C2[0, 1:] = sm - sd
        C2[1:, 0] = sd - sm
        C2[1:, 1:] = -_skew(sd) - _skew(sm)
        C1 = C1 * (-2); C2 = C2 * 2
        A = (C2.T @ C2 / (2 * n) - C1 - C1.T) * 0.5
        U, D, Vt = np.linalg.svd(A)
        qdot = U[:, 0]
        q = qdot[1:]
        Cq = _skew(q)
        sv = C2 @ qdot * (-1.0) / (2 * n)
        Q = np.zeros((4, 4))
        Q[0, 0] = qdot[0]; Q[0, 1:] = q; Q[1:, 0] = -q; Q[1:, 1:] = np.eye(3) * qdot[0] + Cq
        t = (Q @ sv)[1:]
        R = np.eye(3) * (qdot[0] * qdot[0] - float(q @ q)) + 2 * np.outer(q, q) + 2 * qdot[0] * Cq
        return rms, _rt_to_gl(R, t)
    if algo == 5:   # icp6Dhelix.cc:48-206
        x2, y2, z2 = p2[:, 0], p2[:, 1], p2[:, 2]
        dist = p2 - p1
        B = np.zeros((6, 6))
        B[3, 3] = B[4, 4] = B[5, 5] = n
        B[0, 4] = B[4, 0] = (-z2).sum(); B[1, 3] = B[3, 1] = z2.sum()
        B[0, 5] = B[5, 0] = y2.sum();    B[2, 3] = B[3, 2] = (-y2).sum()
        B[2, 4] = B[4, 2] = x2.sum();    B[1, 5] = B[5, 1] = (-x2).sum()
        B[0, 1] = B[1, 0] = (y2 * -x2).sum(); B[0, 2] = B[2, 0] = (-z2 * x2).sum(); B[1, 2] = B[2, 1] = (z2 * -y2).sum()
        B[0, 0] = (z2 * z2 + y2 * y2).sum(); B[1, 1] = (z2 * z2 + x2 * x2).sum(); B[2, 2] = (x2 * x2 + y2 * y2).sum()
        bd = np.array([(-z2 * dist[:, 1] + y2 * dist[:, 2]).sum(), (z2 * dist[:, 0] - x2 * dist[:, 2]).sum(),
                       (-y2 * dist[:, 0] + x2 * dist[:, 1]).sum(), dist[:, 0].sum(), dist[:, 1].sum(), dist[:, 2].sum()])
        ccs = np.linalg.solve(B, bd)
        c, cs = -ccs[:3], -ccs[3:]
        CLength = math.sqrt(float(c @ c))
        rotationCheck = float(c @ cs)
        angle = math.atan(CLength)
        g = c / CLength
        sinA = math.sin(-angle / 2)
        b0, b1, b2, b3 = math.cos(-angle / 2), g[0] * sinA, g[1] * sinA, g[2] * sinA
        R = np.array([[b0 * b0 + b1 * b1 - b2 * b2 - b3 * b3, 2 * (b1 * b2 + b0 * b3), 2 * (b1 * b3 - b0 * b2)],
                      [2 * (b1 * b2 - b0 * b3), b0 * b0 - b1 * b1 + b2 * b2 - b3 * b3, 2 * (b2 * b3 + b0 * b1)],
                      [2 * (b1 * b3 + b0 * b2), 2 * (b2 * b3 - b0 * b1), b0 * b0 - b1 * b1 - b2 * b2 + b3 * b3]])
        R = R / (b0 * b0 + b1 * b1 + b2 * b2 + b3 * b3)
        skew = rotationCheck / (CLength * CLength)
        gs = (cs - c * skew) / CLength
        pT = np.cross(g, gs)
        t = R @ -pT + g * (skew * angle) + pT
        return rms, _rt_to_gl(R, t)
    if algo == 7:   # icp6Dlumeuler.cc:42-229
        rPosTheta, rPos = matrix4_to_euler(pose)
        u = (p1 + p2) / 2.0
        d = p1 - p2
        x, y, z = u[:, 0], u[:, 1], u[:, 2]
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        MZ = np.array([dx.sum(), dy.sum(), dz.sum(), (-z * dy + y * dz).sum(), (-y * dx + x * dy).sum(),
                       (z * dx - x * dz).sum()])
        MM = np.zeros((6, 6))
        MM[0, 0] = MM[1, 1] = MM[2, 2] = n
        MM[3, 3] = (y * y + z * z).sum(); MM[4, 4] = (x * x + y * y).sum(); MM[5, 5] = (x * x + z * z).sum()
        MM[0, 4] = MM[4, 0] = -y.sum(); MM[0, 5] = MM[5, 0] = z.sum()
        MM[1, 3] = MM[3, 1] = -z.sum(); MM[1, 4] = MM[4, 1] = x.sum()
        MM[2, 3] = MM[3, 2] = y.sum();  MM[2, 5] = MM[5, 2] = -x.sum()
        MM[3, 4] = MM[4, 3] = -(x * z).sum(); MM[3, 5] = MM[5, 3] = -(x * y).sum(); MM[4, 5] = MM[5, 4] = -(y * z).sum()
        Ehat = np.linalg.solve(MM, MZ)
        cx, cy = math.cos(rPosTheta[0]), math.cos(rPosTheta[1])
        sx, sy = math.sin(rPosTheta[0]), math.sin(rPosTheta[1])
        tx, ty, tz = rPos
        T1 = _euler_T(rPos, rPosTheta)
        H = np.eye(6)
        H[0, 4] = -tz * cx + ty * sx; H[0, 5] = ty * cx * cy + tz * cy * sx
        H[1, 3] = tz; H[1, 4] = -tx * sx; H[1, 5] = -tx * cx * cy + tz * sy
        H[2, 3] = -ty; H[2, 4] = tx * cx; H[2, 5] = -tx * cy * sx - ty * sy
        H[3, 5] = sy; H[4, 4] = sx; H[4, 5] = cx * cy; H[5, 4] = cx; H[5, 5] = -cy * sx
        X = np.concatenate([rPos, rPosTheta]) - np.linalg.solve(H, Ehat)
        T2 = _euler_T(X[:3], X[3:])
        Tinc = T1 @ np.linalg.inv(T2)
        return rms, _rt_to_gl(Tinc[:3, :3], Tinc[:3, 3])
    if algo == 8:   # icp6Dlumquat.cc:40-231
        quat, t = matrix4_to_quat(pose)
        x = (p1[:, 0] + p1[:, 0]) / 2.0            # sic: p1.x twice (icp6Dlumquat.cc:90)
        y = (p1[:, 1] + p2[:, 1]) / 2.0
        z = (p1[:, 2] + p2[:, 2]) / 2.0
        d = p1 - p2
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        MZ = np.array([dx.sum(), dy.sum(), dz.sum(), (x * dx + y * dy + z * dz).sum(), (z * dy - y * dz).sum(),
                       (x * dz - z * dx).sum(), (y * dx - x * dy).sum()])
        MM = np.zeros((7, 7))
        MM[0, 0] = MM[1, 1] = MM[2, 2] = n
        MM[3, 3] = (x * x + y * y + z * z).sum(); MM[4, 4] = (y * y + z * z).sum()
        MM[5, 5] = (x * x + z * z).sum(); MM[6, 6] = (x * x + y * y).sum()
        sx, sy, sz = x.sum(), y.sum(), z.sum()
        MM[0, 3] = MM[3, 0] = sx; MM[0, 5] = MM[5, 0] = -sz; MM[0, 6] = MM[6, 0] = sy
        MM[1, 3] = MM[3, 1] = sy; MM[1, 4] = MM[4, 1] = sz;  MM[1, 6] = MM[6, 1] = -sx
        MM[2, 3] = MM[3, 2] = sz; MM[2, 4] = MM[4, 2] = -sy; MM[2, 5] = MM[5, 2] = sx
        MM[4, 5] = MM[5, 4] = -(x * y).sum(); MM[4, 6] = MM[6, 4] = -(x * z).sum(); MM[5, 6] = MM[6, 5] = -(y * z).sum()
        Ehat = np.linalg.solve(MM, MZ)
        p, q, r, sq = quat
        X0, Y0, Z0 = t
        U = np.array([[p, q, r, sq], [q, -p, sq, -r], [r, -sq, -p, q], [sq, r, -q, -p]])
        T = np.array([[p * X0 + sq * Y0 - r * Z0, q * X0 + r * Y0 + sq * Z0, r * X0 - q * Y0 + p * Z0, sq * X0 - p * Y0 - q * Z0],
                      [-sq * X0 + p * Y0 + q * Z0, -r * X0 + q * Y0 - p * Z0, q * X0 + r * Y0 + sq * Z0, p * X0 + sq * Y0 - r * Z0],
                      [r * X0 - q * Y0 + p * Z0, -sq * X0 + p * Y0 + q * Z0, -p * X0 - sq * Y0 + r * Z0, q * X0 + r * Y0 - sq * Z0]])
        H = np.zeros((7, 7))
        H[:3, :3] = np.eye(3); H[:3, 3:] = T * (-2); H[3:, 3:] = U * 2
        Xhat = np.array([X0, Y0, Z0, p, q, r, sq])
        T1 = _quat_T(t, p, np.array([q, r, sq]))
        X = Xhat - np.linalg.solve(H, Ehat)
        T2 = _quat_T(X[:3], X[3], X[4:7])
        Tinc = T1 @ np.linalg.inv(T2)
        return rms, _rt_to_gl(Tinc[:3, :3], Tinc[:3, 3])
    if algo == 9:   # icp6Dquatscale.cc:37-161
        S = (p2.T @ p1) / n - np.outer(cd, cm)
        tr = np.trace(S)
        Q = np.zeros((4, 4))
        Q[0, 0] = tr
        Q[0, 1] = Q[1, 0] = S[1, 2] - S[2, 1]
        Q[0, 2] = Q[2, 0] = S[2, 0] - S[0, 2]
        Q[0, 3] = Q[3, 0] = S[0, 1] - S[1, 0]
        Q[1:, 1:] = S + S.T - tr * np.eye(3)
        w, V = np.linalg.eigh(Q)
        q = V[:, np.argmax(w)]
        q = q / np.linalg.norm(q)
        q0, q1, q2, q3 = q
        R = np.array([[q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
                      [2 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 - q0 * q1)],
                      [2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3]])
        scale = math.sqrt(float(((p1 - cm) ** 2).sum()) / float(((p2 - cd) ** 2).sum()))
        return rms, _rt_to_gl(R * scale, cm - scale * (R @ cd))
    raise ValueError("algo")


def align(algo, p1, p2, cm, cd, pn=None, pose=None):
    """Returns (rms, alignxf).  algo = the -a id: 1 QUAT, 2 SVD, 6 APX, 10 NAPX (these four also exist as
    Align_Parallel) and the serial-only 3 ORTHO, 4 DUAL, 5 HELIX, 7 LUMEULER, 8 LUMQUAT, 9 QUAT_SCALE."""
    n = len(p1)
    cm = np.asarray(cm, float)
    cd = np.asarray(cd, float)
    if algo in (3, 4, 5, 7, 8, 9):
        return _align_serial_only(algo, p1, p2, cm, cd, pose)
    if algo == 1:   # icp6Dquat.cc:38-144
        s = float(((p1 - p2) ** 2).sum())
        S = (p2.T @ p1) / n - np.outer(cd, cm)        # S[i][j] = sum p2_i p1_j / n - cd_i cm_j
        tr = np.trace(S)
        Q = np.zeros((4, 4))
        Q[0, 0] = tr
        Q[0, 1] = Q[1, 0] = S[1, 2] - S[2, 1]
        Q[0, 2] = Q[2, 0] = S[2, 0] - S[0, 2]
        Q[0, 3] = Q[3, 0] = S[0, 1] - S[1, 0]
        Q[1:, 1:] = S + S.T - tr * np.eye(3)
        w, V = np.linalg.eigh(Q)
        q = V[:, np.argmax(w)]
        q = q / np.linalg.norm(q)
        q0, q1, q2, q3 = q
        R = np.array([[q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
                      [2 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 - q0 * q1)],
                      [2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3]])
        return math.sqrt(s / n), _compose(R, cm, cd)
    if algo == 2:   # icp6Dsvd.cc:38-158
        s = float(((p1 - p2) ** 2).sum())
        H = (p2 - cd).T @ (p1 - cm)                    # H(j,k) = sum d_j m_k
        U, L, Vt = np.linalg.svd(H)
        V = Vt.T
        R = V @ U.T
        if np.linalg.det(R) < 0:
            V[:, 2] = -V[:, 2]
            R = V @ U.T
        return math.sqrt(s / n), _compose(R, cm, cd)
    if algo == 6:   # icp6Dapx.cc:35-133
        if n <= 3:
            return 0.0, np.eye(4).reshape(16)
        p12 = p1 - p2
        p2c = p2 - cd
        s = float((p12 ** 2).sum())
        B = np.array([(p12[:, 2] * p2c[:, 1] - p12[:, 1] * p2c[:, 2]).sum(),
                      (p12[:, 0] * p2c[:, 2] - p12[:, 2] * p2c[:, 0]).sum(),
                      (p12[:, 1] * p2c[:, 0] - p12[:, 0] * p2c[:, 1]).sum()])
        A = np.zeros((3, 3))
        A[0, 0] = (p2c[:, 1] ** 2 + p2c[:, 2] ** 2).sum()
        A[0, 1] = -(p2c[:, 0] * p2c[:, 1]).sum()
        A[0, 2] = -(p2c[:, 0] * p2c[:, 2]).sum()
        A[1, 1] = (p2c[:, 0] ** 2 + p2c[:, 2] ** 2).sum()
        A[1, 2] = -(p2c[:, 1] * p2c[:, 2]).sum()
        A[2, 2] = (p2c[:, 0] ** 2 + p2c[:, 1] ** 2).sum()
        x = _choldc_solve(A, B)      # only the upper triangle is read, like choldc
        if x is None:
            return -1.0, np.eye(4).reshape(16)
        return math.sqrt(s / n), _compose(_apx_rotation(x), cm, cd)
    if algo == 10:  # icp6Dnapx.cc:34-149
        d = ((p1 - p2) * pn).sum(axis=1)
        p2c = p2 - cd
        c = np.cross(p2c, pn)
        v = np.hstack([c, pn])
        A = v.T @ v
        B = v.sum(axis=0)            # sic: not weighted by d (icp6Dnapx.cc:68-73)
        x = _choldc_solve(A, B)
        if x is None:
            return -1.0, np.eye(4).reshape(16)
        R = _apx_rotation(x[:3])
        a = _compose(R, x[3:6] + cd, cd)
        return math.sqrt(float((d * d).sum()) / n), a
    raise ValueError("algo")


def align_parallel_quat(n, s, cm, cd, Si):
    """icp6D_QUAT::Align_Parallel (icp6Dquat.cc:515-634) including its un-normalised
    `S -= cd*cm`.  Arrays are per thread chunk."""
    n = np.asarray(n, float)
    N = n.sum()
    cmg = (n[:, None] * cm).sum(axis=0) / N
    cdg = (n[:, None] * cd).sum(axis=0) / N
    ret = math.sqrt(np.sum(s) / N)
    S = np.zeros((3, 3))
    for i in range(len(n)):
        for j in range(3):
            for k in range(3):
                S[j, k] += Si[i][k * 3 + j] + n[i] * ((cd[i][j] - cdg[j]) * (cm[i][k] - cmg[k]))
    S -= np.outer(cdg, cmg)
    tr = np.trace(S)
    Q = np.zeros((4, 4))
    Q[0, 0] = tr
    Q[0, 1] = Q[1, 0] = S[1, 2] - S[2, 1]
    Q[0, 2] = Q[2, 0] = S[2, 0] - S[0, 2]
    Q[0, 3] = Q[3, 0] = S[0, 1] - S[1, 0]
    Q[1:, 1:] = S + S.T - tr * np.eye(3)
    w, V = np.linalg.eigh(Q)
    q0, q1, q2, q3 = V[:, np.argmax(w)]
    R = np.array([[q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
                  [2 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 - q0 * q1)],
                  [2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3]])
    return ret, _compose(R, cmg, cdg)


# ---------------------------------------------------------------------------------------
# Scan model (scan.cc / basicScan.cc, the parts on the path)
# ---------------------------------------------------------------------------------------
class OScan:
    def __init__(self, rPos, rPosTheta, points, normals=None, bucket=20):
        self.rPos = np.array(rPos, float)
        self.rPosTheta = np.array(rPosTheta, float)
        self.transMatOrg = euler_to_matrix4(self.rPos, self.rPosTheta)      # basicScan.cc:184
        self.transMat = np.eye(4).reshape(16).copy()
        self.dalignxf = np.eye(4).reshape(16).copy()
        self._transform_matrix(self.transMatOrg)                           # basicScan.cc:188
        self.dalignxf = np.eye(4).reshape(16).copy()                        # basicScan.cc:192
        self.xyz = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3).copy()
        self.normals = None if normals is None else np.ascontiguousarray(normals, float).reshape(-1, 3).copy()
        orc.transform_points(self.transMatOrg, self.xyz)                   # basicScan.cc:735
        if self.normals is not None:
            orc.transform_normals(self.transMatOrg, self.normals)
        self.xyz_orig = self.xyz.copy()                                    # copyReducedToOriginal
        self.bucket = bucket
        self.kd = None

    def get_rPos(self): return self.rPos
    def get_rPosTheta(self): return self.rPosTheta
    def get_transMat(self): return self.transMat

    def tree(self):
        if self.kd is None:
            self.kd = orc.Tree(self.xyz_orig, self.bucket)
        return self.kd

    def _transform_matrix(self, alignxf):
        """scan.cc:878-898"""
        self.transMat = orc.mmult(alignxf, self.transMat)
        self.rPosTheta, self.rPos = matrix4_to_euler(self.transMat)
        self.dalignxf = orc.mmult(alignxf, self.dalignxf)

    def transform(self, alignxf, *_):
        """scan.cc:918-1009 (points + matrices)"""
        alignxf = np.ascontiguousarray(alignxf, float).reshape(16)
        orc.transform_points(alignxf, self.xyz)
        if self.normals is not None:
            orc.transform_normals(alignxf, self.normals)
        self._transform_matrix(alignxf)

    def transformToEuler(self, rP, rPT, *_):
        """scan.cc:1061-1083"""
        tinv, _ok = orc.m4inv(self.transMat)
        self.transform(tinv)
        self.transform(euler_to_matrix4(rP, rPT))

    def mergeCoordinatesWithRoboterPosition(self, prev):
        """scan.cc:826-833"""
        tmp, _ok = orc.m4inv(prev.transMatOrg)
        self.transform(orc.mmult(prev.transMat, tmp))

    def get_rPosQuat(self):
        """rQuat = Matrix4ToQuat(transMat), kept current by Scan::transformMatrix (scan.cc:886)"""
        return matrix4_to_quat(self.transMat)[0]

    def transformToQuat(self, rP, rPQ, *_):
        """scan.cc:1093-1104"""
        tinv, _ok = orc.m4inv(self.transMat)
        self.transform(tinv)
        self.transform(quat_to_matrix4(rPQ, rP))


def rand_keep_mask(n, rnd):
    """`if (rnd > 1 && rand(rnd) != 0) continue;` (searchTree.cc:118) with rand(int) of
    globals.icc:607-610, one libc rand() per candidate in index order (serial build)."""
    import ctypes
    libc = ctypes.CDLL(None)
    libc.rand.restype = ctypes.c_int
    return np.array([int(float(rnd) * float(libc.rand()) / (2147483647 + 1.0)) == 0 for _ in range(n)], dtype=bool)


class MetaOScan:
    """MetaScan + KDtreeMetaManaged (metaScan.cc:27-107, kdMeta.cc:34-134): tree over the current
    points of the member scans in concatenation order, identity dalignxf."""

    def __init__(self, scans):
        self.scans = list(scans)
        self.dalignxf = np.eye(4).reshape(16).copy()
        self.kd = None

    def tree(self):
        if self.kd is None:
            self._pts = np.ascontiguousarray(np.concatenate([s.xyz for s in self.scans]))
            self.kd = orc.Tree(self._pts, self.scans[0].bucket)
        return self.kd


def get_pt_pairs(source, target, maxdist2, mode=0, rnd=0):
    """Scan::getPtPairs (scan.cc:1220-1260): whole scan, centroids normalised"""
    xyz, nrm = target.xyz, target.normals
    if rnd > 1:
        keep = rand_keep_mask(len(xyz), rnd)
        xyz = np.ascontiguousarray(xyz[keep])
        nrm = None if nrm is None else np.ascontiguousarray(nrm[keep])
    r = source.tree().get_pt_pairs(source.dalignxf, xyz, nrm, 0, None, mode, maxdist2)
    if r["n"]:
        r["cm"] = r["centroid_m"] / r["n"]
        r["cd"] = r["centroid_d"] / r["n"]
    else:
        r["cm"] = r["cd"] = np.zeros(3)
    return r


def match(prev, cur, algo=1, max_dist_match2=625.0, max_num_iterations=50, epsilonICP=1e-7, mode=0,
          align_fn=None, rnd=0):
    """icp6D::match (icp6D.cc:104-285), serial-branch semantics (icp6D.cc:225-246).
    Returns (iter, trace) with trace rows (pairs, rms, alignxf[16])."""
    align_fn = align_fn or align
    trace = []
    if max_num_iterations == 0:
        return 0, trace
    ret = prev_ret = prev_prev_ret = 0.0
    it = 0
    for it in range(max_num_iterations):
        prev_prev_ret, prev_ret = prev_ret, ret
        r = get_pt_pairs(prev, cur, max_dist_match2, mode, rnd)
        if r["n"] > 3:
            if algo in (3, 7, 8):   # getAlgorithmID() 3 / 8: alignxf enters as the scan's transMat (icp6D.cc:237-241)
                ret, alignxf = align_fn(algo, r["p1"], r["p2"], r["cm"], r["cd"], r["pn"], cur.transMat.copy())
            else:
                ret, alignxf = align_fn(algo, r["p1"], r["p2"], r["cm"], r["cd"], r["pn"])
        else:
            break
        trace.append((r["n"], ret, alignxf.copy()))
        cur.transform(alignxf)
        if (abs(ret - prev_ret) < epsilonICP and abs(ret - prev_prev_ret) < epsilonICP) or \
                it == max_num_iterations - 1:
            break
    return it, trace


def point_point_error(prev, cur, max_dist_match, scale_max):
    """icp6D::Point_Point_Error (icp6D.cc:293-367), serial branch -> (error, number of pairs)"""
    scale = math.log(scale_max) / (max_dist_match * max_dist_match)
    r = get_pt_pairs(prev, cur, max_dist_match * max_dist_match)
    d = ((r["p1"] - r["p2"]) ** 2).sum(axis=1)
    error = 0.0
    for v in d:                              # error -= 0.39894228 * exp(dist * scale), in pair order
        error -= 0.39894228 * math.exp(v * scale)
    return error / r["n"], r["n"]


def do_icp(scans, algo=1, max_dist_match2=625.0, max_num_iterations=50, epsilonICP=1e-7, meta=False,
           rnd=0, eP=True, max_num_metascans=-1):
    """icp6D::doICP (icp6D.cc:374-437) -> list of (iter, trace) per matched scan"""
    out = []
    metas, my_meta = [], None
    for i, cur in enumerate(scans):
        if i > 0:
            if eP:
                cur.mergeCoordinatesWithRoboterPosition(scans[i - 1])
            out.append(match(my_meta if meta else scans[i - 1], cur, algo, max_dist_match2, max_num_iterations,
                             epsilonICP, 0, None, rnd))
        if meta and i != len(scans) - 1:
            metas.append(cur)
            if max_num_metascans > 0:
                while len(metas) > max_num_metascans:
                    metas.pop(0)
            my_meta = MetaOScan(metas)
    return out


# ---------------------------------------------------------------------------------------
# graph-SLAM (graph.cc, lum6Deuler.cc, graphSlam6D.cc)
# ---------------------------------------------------------------------------------------
def graph_links(scans, cldist2=None, loopsize=None):
    """Graph(nodes, cldist2, loopsize) (graph.cc:108-131) -> list of (from, to)"""
    n = len(scans)
    links = [(i, i + 1) for i in range(n - 1)]
    if cldist2 is not None:
        for j in range(n):
            for k in range(j + 1, n):
                d = scans[k].get_rPos() - scans[j].get_rPos()
                if abs(k - j) > loopsize and d[0] * d[0] + d[1] * d[1] + d[2] * d[2] < cldist2:
                    links.append((j, k))
    return links


def graph_links_clpairs(scans, clpairs, maxdist2):
    """the graph step of graphSlam6D::matchGraph6Dautomatic(allScans, nrIt, clpairs, loopsize)
    (graphSlam6D.cc:82-133), serial order: link (j, k), j != k, when more than clpairs pairs.
    -> (links, {(j, k): pair count})"""
    links, counts = [], {}
    for j in range(len(scans)):
        for k in range(len(scans)):
            if j == k:
                continue
            m = get_pt_pairs(scans[j], scans[k], maxdist2)["n"]
            counts[(j, k)] = m
            if m > clpairs:
                links.append((j, k))
    return links, counts


def covariance_euler(first, second, maxdist2):
    """lum6DEuler::covarianceEuler (lum6Deuler.cc:94-251) -> (C, CD, m, ss, D)"""
    r = get_pt_pairs(first, second, maxdist2)
    return covariance_euler_from_pairs(r["p1"], r["p2"])


def covariance_euler_from_pairs(a, b):
    """the arithmetic of covarianceEuler after the pair search (lum6Deuler.cc:143-232) on an explicit pair list:
    a = p1 (first scan's points in the world), b = p2 -> (C, CD, m, ss, D)"""
    m = len(a)
    C = np.zeros((6, 6)); CD = np.zeros(6)
    if m <= 2:
        return C, CD, m, 0.0, np.zeros(6)
    u = (a + b) / 2.0
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    d = a - b
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    sx, sy, sz = x.sum(), y.sum(), z.sum()
    xpy = (x * x + y * y).sum(); xpz = (x * x + z * z).sum(); ypz = (y * y + z * z).sum()
    xy = (x * y).sum(); xz = (x * z).sum(); yz = (y * z).sum()
    MZ = np.array([dx.sum(), dy.sum(), dz.sum(), (-z * dy + y * dz).sum(), (-y * dx + x * dy).sum(),
                   (z * dx - x * dz).sum()])
    MM = np.zeros((6, 6))
    MM[0, 0] = MM[1, 1] = MM[2, 2] = m
    MM[3, 3] = ypz; MM[4, 4] = xpy; MM[5, 5] = xpz
    MM[0, 4] = MM[4, 0] = -sy; MM[0, 5] = MM[5, 0] = sz
    MM[1, 3] = MM[3, 1] = -sz; MM[1, 4] = MM[4, 1] = sx
    MM[2, 3] = MM[3, 2] = sy;  MM[2, 5] = MM[5, 2] = -sx
    MM[3, 4] = MM[4, 3] = -xz; MM[3, 5] = MM[5, 3] = -xy; MM[4, 5] = MM[5, 4] = -yz
    D = np.linalg.solve(MM, MZ)                       # MM.i() * MZ
    ss = ((dx - (D[0] - y * D[4] + z * D[5])) ** 2 + (dy - (D[1] - z * D[3] + x * D[4])) ** 2 +
          (dz - (D[2] + y * D[3] - x * D[5])) ** 2).sum()
    ss = ss / (2 * m - 3)
    if ss < 0.0000000000001:
        return C, CD, m, ss, D
    return MM / ss, MZ / ss, m, ss, D


def solve_sparse_cholesky(G, B):
    """graphSlam6D::solveSparseCholesky(GraphMatrix*, B) (graphSlam6D.cc:345-379, 477-503):
    entries with |v| <= 1e-5 are not entered; SPD solve."""
    Gf = np.where(np.abs(G) > 0.00001, G, 0.0)
    L = np.linalg.cholesky(Gf)
    return np.linalg.solve(L.T, np.linalg.solve(L, B))


def lum_pose_update(scan, Xi):
    """lum6Deuler.cc:378-448"""
    xa, ya, za = scan.get_rPos()
    tx, ty = scan.get_rPosTheta()[0], scan.get_rPosTheta()[1]
    ctx, stx, cty, sty = math.cos(tx), math.sin(tx), math.cos(ty), math.sin(ty)
    Ha = np.eye(6)
    Ha[0, 4] = -za * ctx + ya * stx
    Ha[0, 5] = ya * cty * ctx + za * stx * cty
    Ha[1, 3] = za
    Ha[1, 4] = -xa * stx
    Ha[1, 5] = -xa * ctx * cty + za * sty
    Ha[2, 3] = -ya
    Ha[2, 4] = xa * ctx
    Ha[2, 5] = -xa * cty * stx - ya * sty
    Ha[3, 5] = sty
    Ha[4, 4] = stx
    Ha[4, 5] = ctx * cty
    Ha[5, 4] = ctx
    Ha[5, 5] = -stx * cty
    result = np.linalg.inv(Ha) @ Xi
    return scan.get_rPos() - result[:3], scan.get_rPosTheta() - result[3:], float(np.linalg.norm(result[:3]))


def lum_iteration(links, scans, maxdist2):
    """one iteration of lum6DEuler::doGraphSlam6D (lum6Deuler.cc:351-474) -> ret"""
    n = len(scans) - 1
    G = np.zeros((6 * n, 6 * n)); B = np.zeros(6 * n)
    for (fa, fb) in links:
        a, b = fa - 1, fb - 1
        Cab, CDab = covariance_euler(scans[fa], scans[fb], maxdist2)[:2]
        if a >= 0:
            B[a * 6:a * 6 + 6] += CDab; G[a * 6:a * 6 + 6, a * 6:a * 6 + 6] += Cab
        if b >= 0:
            B[b * 6:b * 6 + 6] -= CDab; G[b * 6:b * 6 + 6, b * 6:b * 6 + 6] += Cab
        if a >= 0 and b >= 0:
            G[a * 6:a * 6 + 6, b * 6:b * 6 + 6] -= Cab; G[b * 6:b * 6 + 6, a * 6:a * 6 + 6] -= Cab
    X = solve_sparse_cholesky(G, B)
    tot = 0.0
    for i in range(1, len(scans)):
        rP, rPT, dl = lum_pose_update(scans[i], X[(i - 1) * 6:(i - 1) * 6 + 6])
        scans[i].transformToEuler(rP, rPT)
        tot += dl
    return tot / len(scans), G, B, X


def match_graph6d_automatic(cldist, loopsize, scans, algo, max_dist_match2, max_it, epsilonICP, nrIt, epsilonSLAM,
                            mdml2, eP=True, elch=False, graph_slam=True):
    """matchGraph6Dautomatic (src/slam6d/slam6D.cc:387-548) with my_loopSlam6D == NULL, lum6DEuler as the
    graph back-end, no meta scans: sequential ICP, loop detection by pose distance, rounds of
    { Graph(i+1, cldist^2, loopsize); one LUM iteration } until ret <= epsilonSLAM or nrIt rounds.
    Returns the number of global rounds."""
    cldist2 = cldist * cldist
    n = len(scans)
    loop_detection = 0
    rounds = 0
    g = []
    min_dist, first, last = -1.0, 0, 0
    closed = []

    def global_rounds(nodes):
        nonlocal rounds
        if not graph_slam:
            return 0.0
        j = 0
        while True:
            links = graph_links(scans[:nodes], cldist2, loopsize)
            ret = lum_iteration(links, scans[:nodes], mdml2)[0]
            j += 1
            rounds += 1
            if not (j < nrIt and ret > epsilonSLAM):
                return ret
    for i in range(1, n):
        g.append((i - 1, i))
        if eP:
            scans[i].mergeCoordinatesWithRoboterPosition(scans[i - 1])
        match(scans[i - 1], scans[i], algo, max_dist_match2, max_it, epsilonICP)
        if loop_detection == 1:
            loop_detection = 2
        for j in range(0, i - loopsize):
            d = scans[j].get_rPos() - scans[i].get_rPos()
            dist = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
            if dist < cldist2:
                loop_detection = 1
                if min_dist < 0 or dist < min_dist:
                    min_dist, first, last = dist, j, i
        if loop_detection == 2:
            loop_detection = 0
            min_dist = -1.0
            if elch:
                elch_close_loop(scans, first, last, g, algo, max_dist_match2, max_it, epsilonICP)
                closed.append((first, last))
                g.append((first, last))
            global_rounds(i + 1)
    if loop_detection == 1 and elch:
        elch_close_loop(scans, first, last, g, algo, max_dist_match2, max_it, epsilonICP)
        closed.append((first, last))
        g.append((first, last))
    global_rounds(n)
    if elch:
        return rounds, closed
    return rounds


# ---------------------------------------------------------------------------------------
# ELCH loop closing (-L 1): elch6D::graph_balancer (src/slam6d/elch6D.cc:186-279), elch6Deuler::close_loop
# (src/slam6d/elch6Deuler.cc:44-138).  Parity unpinned: both TUs need Boost.Graph.
# ---------------------------------------------------------------------------------------
def _dijkstra(adj, n, s):
    """boost::dijkstra_shortest_paths: strict '<' relaxation, predecessor[v] == v where unreached"""
    import heapq
    inf = float("inf")
    p = list(range(n)); d = [inf] * n
    d[s] = 0.0
    heap = [(0.0, s)]
    done = [False] * n
    while heap:
        du, u = heapq.heappop(heap)
        if done[u] or du > d[u]:
            continue
        done[u] = True
        for (v, w) in adj[u]:
            nd = d[u] + w
            if nd < d[v]:
                d[v] = nd; p[v] = u
                heapq.heappush(heap, (nd, v))
    return p, d


def graph_balancer(n, edges, ew, f, l):
    """elch6D::graph_balancer on an undirected multigraph [(a, b)] with weights ew -> weights[n] (zeros where the
    balancer assigns nothing)"""
    adj = [[] for _ in range(n)]
    for (a, b), w in zip(edges, ew):
        adj[a].append((b, w))
        if a != b:
            adj[b].append((a, w))

    def remove_edge(a, b):
        adj[a] = [e for e in adj[a] if e[0] != b]
        if a != b:
            adj[b] = [e for e in adj[b] if e[0] != a]
    weights = [0.0] * n
    crossings = [f, l]
    branches = []
    weights[f] = 0.0; weights[l] = 1.0
    p_min = d_min = None
    while crossings:
        dist = -1.0
        s_min = e_min = None
        k = 0
        while k < len(crossings):
            si = crossings[k]
            p, d = _dijkstra(adj, n, si)
            swap = False
            for m in range(k + 1, len(crossings)):
                e = crossings[m]
                if e != p[e] and (dist < 0 or d[e] < dist):
                    dist = d[e]; s_min = k; e_min = m; swap = True
            if swap:
                p_min, d_min = p, d
            if dist < 0:
                branches.append(si)
                del crossings[k]
            else:
                k += 1
        if dist > -1:
            sv, ev = crossings[s_min], crossings[e_min]
            remove_edge(ev, p_min[ev])
            i = p_min[ev]
            while i != sv:
                weights[i] = weights[sv] + (weights[ev] - weights[sv]) * d_min[i] / d_min[ev]
                remove_edge(i, p_min[i])
                if len(adj[i]) > 0:
                    crossings.append(i)
                i = p_min[i]
            # erase by iterator: the positions found above (later erasures do not disturb earlier positions)
            drop = []
            if len(adj[sv]) == 0:
                drop.append(s_min)
            if len(adj[ev]) == 0:
                drop.append(e_min)
            for idx in sorted(drop, reverse=True):
                del crossings[idx]
    while branches:
        s_ = branches.pop(0)
        for (v, w) in list(adj[s_]):
            weights[v] = weights[s_]
            if len(adj[v]) > 1:
                branches.append(v)
        for (v, w) in list(adj[s_]):
            adj[v] = [e for e in adj[v] if e[0] != s_]
        adj[s_] = []
    return np.array(weights)


def match_meta_data(prev, members, algo=1, max_dist_match2=625.0, max_num_iterations=50, epsilonICP=1e-7):
    """icp6D::match with a MetaScan as the data scan (members = its scans): pairs of all members against the model,
    one alignment, every member moved.  Returns (iter, trace)."""
    trace = []
    ret = prev_ret = prev_prev_ret = 0.0
    it = 0
    for it in range(max_num_iterations):
        prev_prev_ret, prev_ret = prev_ret, ret
        rs = [get_pt_pairs(prev, mbr, max_dist_match2) for mbr in members]
        n = sum(r["n"] for r in rs)
        if n > 3:
            p1 = np.concatenate([r["p1"] for r in rs]); p2 = np.concatenate([r["p2"] for r in rs])
            ret, alignxf = align(algo, p1, p2, p1.mean(axis=0), p2.mean(axis=0))
        else:
            break
        trace.append((n, ret, alignxf.copy()))
        for mbr in members:
            mbr.transform(alignxf)
        if (abs(ret - prev_ret) < epsilonICP and abs(ret - prev_prev_ret) < epsilonICP) or it == max_num_iterations - 1:
            break
    return it, trace


def elch_close_loop(scans, first, last, edges, algo, max_dist_match2, max_it, epsilonICP):
    """elch6Deuler::close_loop -> (delta[6], weights[6][n])"""
    n = max(max(a, b) for a, b in edges) + 1
    wts = np.empty((6, len(edges)))
    for e, (a, b) in enumerate(edges):
        Cm = covariance_euler(scans[a], scans[b], max_dist_match2)[0]
        wts[:, e] = np.abs(np.diag(np.linalg.inv(Cm)))
    weights = [graph_balancer(n, edges, wts[j], first, last) for j in range(6)]
    for i in range(last - 2, last + 1):
        for j in range(6):
            weights[j][i] = 0.0
    start = MetaOScan([scans[first], scans[first + 1], scans[first + 2]])
    before = np.concatenate([scans[last].rPos, scans[last].rPosTheta])
    match_meta_data(start, [scans[last - 2], scans[last - 1], scans[last]], algo, max_dist_match2, max_it, epsilonICP)
    delta = np.concatenate([scans[last].rPos, scans[last].rPosTheta]) - before
    for i in range(1, n):
        rP = np.array([scans[i].rPos[k] + delta[k] * (weights[k][i] - weights[k][0]) for k in range(3)])
        rT = np.array([scans[i].rPosTheta[k] + delta[3 + k] * (weights[3 + k][i] - weights[3 + k][0]) for k in range(3)])
        scans[i].transformToEuler(rP, rT)
    return delta, weights


# ---------------------------------------------------------------------------------------
# ELCH loop closing with quaternion poses, -L 2 .. 4: elch6Dquat::close_loop (src/slam6d/elch6Dquat.cc:44-148),
# elch6DunitQuat::close_loop (src/slam6d/elch6DunitQuat.cc:45-199), elch6Dslerp::close_loop
# (src/slam6d/elch6Dslerp.cc:44-184).  PARITY UNPINNED, like -L 1: the three TUs need Boost.Graph and scan.h -> Boost;
# restated by reading, on top of covariance_quat (below), graph_balancer and match_meta_data (above).
# ---------------------------------------------------------------------------------------
def qmult(q1, q2):
    """QMult (globals.icc:1112-1117): q1 * q2, (w, x, y, z)"""
    return np.array([q1[0] * q2[0] - q1[1] * q2[1] - q1[2] * q2[2] - q1[3] * q2[3],
                     q1[0] * q2[1] + q1[1] * q2[0] + q1[2] * q2[3] - q1[3] * q2[2],
                     q1[0] * q2[2] - q1[1] * q2[3] + q1[2] * q2[0] + q1[3] * q2[1],
                     q1[0] * q2[3] + q1[1] * q2[2] - q1[2] * q2[1] + q1[3] * q2[0]])


def normalize4(q):
    """Normalize4 (globals.icc:267-275)"""
    q = np.array(q, dtype=np.float64)
    norm = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return q / norm


def slerp(qa, qb, t):
    """slerp (globals.icc:1123-1166)"""
    cos_half = qa[0] * qb[0] + qa[1] * qb[1] + qa[2] * qb[2] + qa[3] * qb[3]
    if abs(cos_half) >= 1.0:
        return np.array(qa, dtype=np.float64)
    half = math.acos(cos_half)
    sin_half = math.sqrt(1.0 - cos_half * cos_half)
    if abs(sin_half) < 0.001:
        return normalize4([qa[k] * 0.5 + qb[k] * 0.5 for k in range(4)])
    ratio_a = math.sin((1 - t) * half) / sin_half
    ratio_b = math.sin(t * half) / sin_half
    return normalize4([qa[k] * ratio_a + qb[k] * ratio_b for k in range(4)])


def _elch_quat_weights(scans, edges, first, last, maxdist2, combine):
    """The part the three share: one covarianceQuat per edge, C = C.i(), |diag| as edge weights -- seven graphs
    (elch6Dquat.cc:52-66), or three + the sum of the four quaternion entries (elch6DunitQuat.cc:52-69,
    elch6Dslerp.cc:50-84; `abs` there is the floating-point overload) -- and a graph_balancer run per graph."""
    n = max(max(a, b) for a, b in edges) + 1
    nw = 4 if combine else 7
    wts = np.empty((nw, len(edges)))
    for e, (a, b) in enumerate(edges):
        Cm = covariance_quat(scans[a], scans[b], maxdist2)[0]
        d = np.abs(np.diag(np.linalg.inv(Cm)))
        if combine:
            wts[:3, e] = d[:3]
            wts[3, e] = d[3] + d[4] + d[5] + d[6]
        else:
            wts[:, e] = d
    return n, [graph_balancer(n, edges, wts[j], first, last) for j in range(nw)]


def elch_close_loop_quat(scans, first, last, edges, algo, max_dist_match2, max_it, epsilonICP):
    """elch6Dquat::close_loop (-L 2) -> (delta[7], weights[7][n])"""
    n, weights = _elch_quat_weights(scans, edges, first, last, max_dist_match2, False)
    start = MetaOScan([scans[first], scans[first + 1], scans[first + 2]])
    for i in range(last - 2, last + 1):                            # elch6Dquat.cc:85-89
        for j in range(7):
            weights[j][i] = 0.0
    before = np.concatenate([scans[last].rPos, scans[last].get_rPosQuat()])
    match_meta_data(start, [scans[last - 2], scans[last - 1], scans[last]], algo, max_dist_match2, max_it, epsilonICP)
    delta = np.concatenate([scans[last].rPos, scans[last].get_rPosQuat()]) - before
    for i in range(1, n):                                          # elch6Dquat.cc:124-142
        rq = scans[i].get_rPosQuat()
        rP = np.array([scans[i].rPos[k] + delta[k] * (weights[k][i] - weights[k][0]) for k in range(3)])
        rQ = np.array([rq[k] + delta[3 + k] * (weights[3 + k][i] - weights[3 + k][0]) for k in range(4)])
        scans[i].transformToQuat(rP, normalize4(rQ))
    return delta, weights


def elch_close_loop_unitquat(scans, first, last, edges, algo, max_dist_match2, max_it, epsilonICP):
    """elch6DunitQuat::close_loop (-L 3) -> (delta[3], deltaQ[4], weights[4][n])"""
    n, weights = _elch_quat_weights(scans, edges, first, last, max_dist_match2, True)
    start = MetaOScan([scans[first], scans[first + 1], scans[first + 2]])
    ends = [scans[last - 2], scans[last - 1], scans[last]]
    old = [(scans[k].rPos.copy(), scans[k].get_rPosQuat().copy()) for k in (last, last - 1, last - 2)]   # :84-108
    p_before = scans[last].rPos.copy()
    qb = scans[last].get_rPosQuat()
    q1 = np.array([qb[0], -qb[1], -qb[2], -qb[3]])                  # :114-118
    match_meta_data(start, ends, algo, max_dist_match2, max_it, epsilonICP)
    delta = scans[last].rPos - p_before
    deltaQ = qmult(scans[last].get_rPosQuat(), q1)                  # q2 * q1^-1, :135
    for k, (p, q) in zip((last, last - 1, last - 2), old):          # restore poses after ICP matching, :149-152
        scans[k].transformToQuat(p, q)
    q0 = scans[0].get_rPosQuat()                                    # inverse rotation of scan 0, :155-167
    w0 = weights[3][0]
    pd = qmult(deltaQ, q0)
    s0 = np.array([(1 - w0) * q0[0] + pd[0] * w0,
                   -1 * ((1 - w0) * q0[1] + pd[1] * w0),
                   -1 * ((1 - w0) * q0[2] + pd[2] * w0),
                   -1 * ((1 - w0) * q0[3] + pd[3] * w0)])
    scan0Pdelta = qmult(q0, normalize4(s0))
    for i in range(1, n):                                           # :170-192
        rP = np.array([scans[i].rPos[k] + delta[k] * (weights[k][i] - weights[k][0]) for k in range(3)])
        qi = scans[i].get_rPosQuat()
        rot = qmult(deltaQ, qi)
        wi = weights[3][i]
        tmp = normalize4([(1 - wi) * qi[k] + rot[k] * wi for k in range(4)])
        scans[i].transformToQuat(rP, normalize4(qmult(scan0Pdelta, tmp)))
    return delta, deltaQ, weights


def elch_close_loop_slerp(scans, first, last, edges, algo, max_dist_match2, max_it, epsilonICP):
    """elch6Dslerp::close_loop (-L 4) -> (deltaT[3], deltaQ[4], weights[4][n])"""
    n, weights = _elch_quat_weights(scans, edges, first, last, max_dist_match2, True)
    start = MetaOScan([scans[i] for i in range(first - 2, first + 3) if i >= 0])          # :93-98
    ends = [scans[i] for i in range(last - 2, last + 1) if i < n]                          # :100-110 (offsets 2 / 0)
    Pl0 = scans[last].transMat.copy()
    match_meta_data(start, ends, algo, max_dist_match2, max_it, epsilonICP)
    Pp0 = scans[last].transMat.copy()
    Pf0 = scans[first].transMat.copy()
    Pf0_inv = orc.m4inv(Pf0)[0]
    tmp1 = orc.mmult(Pf0_inv, Pl0)                                  # :127-130
    tmp2 = orc.m4inv(tmp1)[0]
    tmp1 = orc.mmult(Pp0, tmp2)
    deltaf = orc.mmult(Pf0_inv, tmp1)
    deltaQ, deltaT = matrix4_to_quat(deltaf)
    idQ = np.array([1.0, 0.0, 0.0, 0.0])

    def share(i):
        rP = np.array([deltaT[k] * weights[k][i] for k in range(3)])
        return quat_to_matrix4(slerp(idQ, deltaQ, weights[3][i]), rP)
    delta0 = orc.mmult(Pf0, orc.m4inv(share(0))[0])                # :151-157
    for i in range(1, n):                                           # :162-175
        if last - 2 <= i <= last:
            M = orc.mmult(delta0, Pf0_inv)
        else:
            M = orc.mmult(orc.mmult(delta0, share(i)), Pf0_inv)
        scans[i].transform(M)
    return deltaT, deltaQ, weights


# ---------------------------------------------------------------------------------------
# lum6DQuat (-G 2), src/slam6d/lum6Dquat.cc   (pinned: tests/test_graph_backends_reference_host.py)
# ---------------------------------------------------------------------------------------
def covariance_quat(first, second, maxdist2):
    """lum6DQuat::covarianceQuat (lum6Dquat.cc:81-248) -> (C 7x7, CD 7, m, ss)"""
    r = get_pt_pairs(first, second, maxdist2)
    m = r["n"]
    C = np.zeros((7, 7)); CD = np.zeros(7)
    if m <= 2:
        return C, CD, m, 0.0
    a, b = r["p1"], r["p2"]
    u = (a + b) / 2.0
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    d = a - b
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    sx, sy, sz = x.sum(), y.sum(), z.sum()
    MZ = np.array([dx.sum(), dy.sum(), dz.sum(), (x * dx + y * dy + z * dz).sum(), (z * dy - y * dz).sum(),
                   (x * dz - z * dx).sum(), (y * dx - x * dy).sum()])
    MM = np.zeros((7, 7))
    MM[0, 0] = MM[1, 1] = MM[2, 2] = m
    MM[3, 3] = (x * x + y * y + z * z).sum(); MM[4, 4] = (y * y + z * z).sum()
    MM[5, 5] = (x * x + z * z).sum(); MM[6, 6] = (x * x + y * y).sum()
    MM[0, 3] = MM[3, 0] = sx; MM[0, 5] = MM[5, 0] = -sz; MM[0, 6] = MM[6, 0] = sy
    MM[1, 3] = MM[3, 1] = sy; MM[1, 4] = MM[4, 1] = sz;  MM[1, 6] = MM[6, 1] = -sx
    MM[2, 3] = MM[3, 2] = sz; MM[2, 4] = MM[4, 2] = -sy; MM[2, 5] = MM[5, 2] = sx
    MM[4, 5] = MM[5, 4] = -(x * y).sum(); MM[4, 6] = MM[6, 4] = -(x * z).sum(); MM[5, 6] = MM[6, 5] = -(y * z).sum()
    D = np.linalg.solve(MM, MZ)
    e0 = dx - (D[0] + x * D[3] - z * D[5] + y * D[6])
    e1 = dy - (D[1] + y * D[3] + z * D[4] - x * D[6])
    e2 = dz - (D[2] + z * D[3] - y * D[4] + x * D[5])
    ss = float((e0 * e0 + e1 * e1 + e2 * e2).sum()) / (2 * m - 3)
    with np.errstate(divide="ignore", invalid="ignore"):      # no guard here (unlike covarianceEuler): ss == 0 gives inf / NaN
        ssi = np.float64(1.0) / np.float64(ss)
        return MM * ssi, MZ * ssi, m, ss


def lumquat_pose_update(scan, Xi):
    """lum6Dquat.cc:347-432 -> (rPos, rPosQuat normalised, |dxyz|)"""
    xa, ya, za = scan.get_rPos()
    p, q, r, s = scan.get_rPosQuat()
    px, py, pz = p * xa, p * ya, p * za
    qx, qy, qz = q * xa, q * ya, q * za
    rx, ry, rz = r * xa, r * ya, r * za
    sx, sy, sz = s * xa, s * ya, s * za
    Ha = np.eye(7)
    Ha[3, 3] = 2 * p; Ha[4, 3] = 2 * q; Ha[5, 3] = 2 * r; Ha[6, 3] = 2 * s
    Ha[3, 4] = 2 * q; Ha[4, 4] = -2 * p; Ha[5, 4] = -2 * s; Ha[6, 4] = 2 * r
    Ha[3, 5] = 2 * r; Ha[4, 5] = 2 * s; Ha[5, 5] = -2 * p; Ha[6, 5] = -2 * q
    Ha[3, 6] = 2 * s; Ha[4, 6] = -2 * r; Ha[5, 6] = 2 * q; Ha[6, 6] = -2 * p
    Ha[0, 3] = -2 * (px + sy - rz); Ha[1, 3] = -2 * (-sx + py + qz); Ha[2, 3] = -2 * (rx - qy + pz)
    Ha[0, 4] = -2 * (qx + ry + sz); Ha[1, 4] = -2 * (-rx + qy - pz); Ha[2, 4] = -2 * (-sx + py + qz)
    Ha[0, 5] = -2 * (rx - qy + pz); Ha[1, 5] = -2 * (qx + ry + sz);  Ha[2, 5] = -2 * (-px - sy + rz)
    Ha[0, 6] = -2 * (sx - py - qz); Ha[1, 6] = -2 * (px + sy - rz);  Ha[2, 6] = -2 * (qx + ry + sz)
    result = np.linalg.solve(Ha, Xi)
    rPos = scan.get_rPos() - result[:3]
    quat = np.array([p, q, r, s]) - result[3:]
    quat = quat / math.sqrt(float(quat @ quat))
    return rPos, quat, float(np.linalg.norm(result[:3]))


def lumquat_iteration(links, scans, maxdist2):
    """one iteration of lum6DQuat::doGraphSlam6D (lum6Dquat.cc:319-481); FillGB3D (:248-276) ASSIGNS the
    off-diagonal blocks (`= -Cab`), so of several links between the same two scans the last one wins there."""
    n = len(scans) - 1
    G = np.zeros((7 * n, 7 * n)); B = np.zeros(7 * n)
    for (fa, fb) in links:
        a, b = fa - 1, fb - 1
        Cab, CDab = covariance_quat(scans[fa], scans[fb], maxdist2)[:2]
        if a >= 0:
            B[a * 7:a * 7 + 7] += CDab; G[a * 7:a * 7 + 7, a * 7:a * 7 + 7] += Cab
        if b >= 0:
            B[b * 7:b * 7 + 7] -= CDab; G[b * 7:b * 7 + 7, b * 7:b * 7 + 7] += Cab
        if a >= 0 and b >= 0:
            G[a * 7:a * 7 + 7, b * 7:b * 7 + 7] = -Cab; G[b * 7:b * 7 + 7, a * 7:a * 7 + 7] = -Cab
    X = solve_sparse_cholesky(G, B)
    tot = 0.0
    for i in range(1, len(scans)):
        rP, rQ, dl = lumquat_pose_update(scans[i], X[(i - 1) * 7:(i - 1) * 7 + 7])
        scans[i].transformToQuat(rP, rQ)
        tot += dl
    return tot / len(scans), G, B, X


# ---------------------------------------------------------------------------------------
# ghelix6DQ2 (-G 3), src/slam6d/ghelix6DQ2.cc   (pinned, as above)
# ---------------------------------------------------------------------------------------
def helix_compute_rt(ccs):
    """icp6D_HELIX::computeRt (icp6Dhelix.cc:144-206) for one 6-vector"""
    c, cs = -ccs[:3], -ccs[3:]
    CLength = math.sqrt(float(c @ c))
    rotationCheck = float(c @ cs)
    angle = math.atan(CLength)
    g = c / CLength
    sinA = math.sin(-angle / 2)
    b0, b1, b2, b3 = math.cos(-angle / 2), g[0] * sinA, g[1] * sinA, g[2] * sinA
    R = np.array([[b0 * b0 + b1 * b1 - b2 * b2 - b3 * b3, 2 * (b1 * b2 + b0 * b3), 2 * (b1 * b3 - b0 * b2)],
                  [2 * (b1 * b2 - b0 * b3), b0 * b0 - b1 * b1 + b2 * b2 - b3 * b3, 2 * (b2 * b3 + b0 * b1)],
                  [2 * (b1 * b3 + b0 * b2), 2 * (b2 * b3 - b0 * b1), b0 * b0 - b1 * b1 - b2 * b2 + b3 * b3]])
    R = R / (b0 * b0 + b1 * b1 + b2 * b2 + b3 * b3)
    skew = rotationCheck / (CLength * CLength)
    gs = (cs - c * skew) / CLength
    pT = np.cross(g, gs)
    t = R @ -pT + g * (skew * angle) + pT
    return _rt_to_gl(R, t)


def ghelix_link_blocks(p1, p2):
    """the per-link sums of ghelix6DQ2::genBBdForLinkedPair (ghelix6DQ2.cc:88-150):
    -> (n, Blk 6x6 symmetric, bd1 6, bd2 6)"""
    n = len(p1)
    x2, y2, z2 = p2[:, 0], p2[:, 1], p2[:, 2]
    b40, b50, b42 = (-z2).sum(), y2.sum(), x2.sum()
    Blk = np.zeros((6, 6))
    Blk[3, 3] = Blk[4, 4] = Blk[5, 5] = n
    Blk[0, 4] = Blk[4, 0] = b40;  Blk[1, 3] = Blk[3, 1] = -b40
    Blk[0, 5] = Blk[5, 0] = b50;  Blk[2, 3] = Blk[3, 2] = -b50
    Blk[2, 4] = Blk[4, 2] = b42;  Blk[1, 5] = Blk[5, 1] = -b42
    Blk[0, 1] = Blk[1, 0] = (y2 * -x2).sum(); Blk[0, 2] = Blk[2, 0] = (-z2 * x2).sum(); Blk[1, 2] = Blk[2, 1] = (z2 * -y2).sum()
    Blk[0, 0] = (z2 * z2 + y2 * y2).sum(); Blk[1, 1] = (z2 * z2 + x2 * x2).sum(); Blk[2, 2] = (x2 * x2 + y2 * y2).sum()
    d = p1 - p2
    bd1 = np.array([(-p1[:, 2] * d[:, 1] + p1[:, 1] * d[:, 2]).sum(), (p1[:, 2] * d[:, 0] - p1[:, 0] * d[:, 2]).sum(),
                    (-p1[:, 1] * d[:, 0] + p1[:, 0] * d[:, 1]).sum(), d[:, 0].sum(), d[:, 1].sum(), d[:, 2].sum()])
    bd2 = np.array([(-z2 * -d[:, 1] + y2 * -d[:, 2]).sum(), (z2 * -d[:, 0] - x2 * -d[:, 2]).sum(),
                    (-y2 * -d[:, 0] + x2 * -d[:, 1]).sum(), -d[:, 0].sum(), -d[:, 1].sum(), -d[:, 2].sum()])
    return n, Blk, bd1, bd2


def ghelix_iteration(links, scans, maxdist2, B=None, bd=None):
    """one iteration of ghelix6DQ2::doGraphSlam6D (ghelix6DQ2.cc:330-449).  B and bd persist across
    the iterations of one call (they are zeroed before the loop only, :329-330): pass them back in."""
    n = len(scans) - 1
    if B is None:
        B = np.zeros((6 * n, 6 * n)); bd = np.zeros(6 * n)
    for (fa, fb) in links:
        r = get_pt_pairs(scans[fa], scans[fb], maxdist2)
        if r["n"] <= 1:
            continue
        m, Blk, bd1, bd2 = ghelix_link_blocks(r["p1"], r["p2"])
        a, b = (fa - 1) * 6, (fb - 1) * 6
        if fa != 0:
            B[a:a + 6, a:a + 6] += Blk; bd[a:a + 6] += bd1
        B[b:b + 6, b:b + 6] += Blk; bd[b:b + 6] += bd2
        if fa != 0:
            B[a:a + 6, b:b + 6] -= Blk; B[b:b + 6, a:a + 6] -= Blk
    ccs = solve_sparse_cholesky(B, bd)
    tot = 0.0
    for i in range(1, len(scans)):
        axf = helix_compute_rt(ccs[(i - 1) * 6:(i - 1) * 6 + 6])
        scans[i].transform(axf)
        tot += math.sqrt(axf[12] ** 2 + axf[13] ** 2 + axf[14] ** 2)
    return tot / len(scans), B, bd, ccs


# ---------------------------------------------------------------------------------------
# gapx6D (-G 4), src/slam6d/gapx6D.cc
# ---------------------------------------------------------------------------------------
def compute_rt(x, dx):
    """icp6D_APX::computeRt (icp6Dapx.cc:310-335)"""
    a = np.zeros(16)
    R = _apx_rotation(x)
    for r in range(3):
        for c in range(3):
            a[c * 4 + r] = R[r, c]
    a[12:15] = dx
    a[15] = 1
    return a


def gapx_link_blocks(p1, p2, cm):
    """gapx6D::genBArotForLinkedPair (gapx6D.cc:153-310): the per-link sums, literally (including
    `p1x*p2x + p1y + p2y`), both points centred on centroids_m."""
    a = p1 - cm
    b = p2 - cm
    p1x, p1y, p1z = a.T
    p2x, p2y, p2z = b.T
    MkMkt = np.array([[(p1y * p1y + p1z * p1z).sum(), -(p1x * p1y).sum(), -(p1x * p1z).sum()],
                      [-(p1x * p1y).sum(), (p1x * p1x + p1z * p1z).sum(), -(p1y * p1z).sum()],
                      [-(p1x * p1z).sum(), -(p1y * p1z).sum(), (p1x * p1x + p1y * p1y).sum()]])
    DkDkt = np.array([[(p2y * p2y + p2z * p2z).sum(), -(p2x * p2y).sum(), -(p2x * p2z).sum()],
                      [-(p2x * p2y).sum(), (p2x * p2x + p2z * p2z).sum(), -(p2y * p2z).sum()],
                      [-(p2x * p2z).sum(), -(p2y * p2z).sum(), (p2x * p2x + p2y * p2y).sum()]])
    d11 = (p1y * p2y + p1z + p2z).sum()       # p1yp2yp1zp2z  (sic)
    d22 = (p1x * p2x + p1z + p2z).sum()       # p1xp2xp1zp2z
    d33 = (p1x * p2x + p1y + p2y).sum()       # p1xp2xp1yp2y
    MkDkt = np.array([[d11, -(p1y * p2x).sum(), -(p1z * p2x).sum()],
                      [-(p1y * p2x).sum(), d22, -(p1z * p2y).sum()],
                      [-(p1z * p2x).sum(), -(p1z * p2y).sum(), d33]])
    DkMkt = np.array([[d11, -(p2y * p1x).sum(), -(p2z * p1x).sum()],
                      [-(p2y * p1x).sum(), d22, -(p2z * p1y).sum()],
                      [-(p2z * p1x).sum(), -(p2z * p1y).sum(), d33]])
    Ak1 = -np.array([((p1z - p2z) * p2y - (p1y - p2y) * p2z).sum(), ((p1x - p2x) * p2z - (p1z - p2z) * p2x).sum(),
                     ((p1y - p2y) * p2x - (p1x - p2x) * p2y).sum()])
    Ak2 = np.array([((p1z - p2z) * p1y - (p1y - p2y) * p1z).sum(), ((p1x - p2x) * p1z - (p1z - p2z) * p1x).sum(),
                    ((p1y - p2y) * p1x - (p1x - p2x) * p1y).sum()])
    return MkMkt, DkDkt, MkDkt, DkMkt, Ak1, Ak2


def solve_chol_upper(G, B):
    """solveSparseCholesky(const Matrix&, B) (graphSlam6D.cc:302-343): entries |v| <= 1e-5 dropped,
    cs_cholsol reads the upper triangle of the (not exactly symmetric) matrix only."""
    U = np.triu(np.where(np.abs(G) > 0.00001, G, 0.0))
    S = U + np.triu(U, 1).T
    L = np.linalg.cholesky(S)
    return np.linalg.solve(L.T, np.linalg.solve(L, B))


def gapx_translate_and_move(links, scans, cms, cds, X, T, A=None):
    """the rest of an iteration of gapx6D::doGraphSlam6D once X is solved (gapx6D.cc:456-529): the translation system
    (genBAtransForLinkedPair, :76-137), T += Bt^-1 A, the pose update.  T is updated in place, and so is A (3n) if given:
    it is left holding the translation system's right hand side, as the reference's is.  -> sum of |T_i|"""
    n = len(scans) - 1
    tot = 0.0
    Bt = np.zeros((n, n))
    A = np.zeros(3 * n) if A is None else A
    A[:] = 0.0
    for (f, sx), cm, cd in zip(links, cms, cds):         # genBAtransForLinkedPair (gapx6D.cc:76-137)
        x = X[(f - 1) * 3:(f - 1) * 3 + 3] if f != 0 else np.zeros(3)
        pm = cm.copy(); orc.transform_points(compute_rt(x, np.zeros(3)), pm.reshape(1, 3))
        pd = cd.copy(); orc.transform_points(compute_rt(X[(sx - 1) * 3:(sx - 1) * 3 + 3], np.zeros(3)), pd.reshape(1, 3))
        Ak1 = pm - pd
        if f != 0:
            A[(f - 1) * 3:(f - 1) * 3 + 3] -= Ak1
            Bt[f - 1, f - 1] += 1
            Bt[f - 1, sx - 1] -= 1; Bt[sx - 1, f - 1] -= 1   # SymmetricMatrix: one stored element
        A[(sx - 1) * 3:(sx - 1) * 3 + 3] += Ak1
        Bt[sx - 1, sx - 1] += 1
    Bti = np.linalg.inv(Bt)
    for i in range(n):
        for j in range(n):
            T[i * 3:i * 3 + 3] += A[j * 3:j * 3 + 3] * Bti[i, j]
    for i in range(1, len(scans)):
        dx = T[(i - 1) * 3:(i - 1) * 3 + 3]
        scans[i].transform(compute_rt(X[(i - 1) * 3:(i - 1) * 3 + 3], dx))
        tot += float(np.sqrt(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2]))
    return tot


class GapxState:
    """what gapx6D::doGraphSlam6D keeps over the iterations of one call: the translations T, the rotation system's
    matrix B and the right hand side A that both systems share"""

    def __init__(self, n, T=None):
        self.T = np.zeros(3 * n) if T is None else np.asarray(T, np.float64)
        self.B = np.zeros((3 * n, 3 * n))
        self.A = np.zeros(3 * n)

    def copy(self):
        c = GapxState(len(self.T) // 3, self.T.copy())
        c.B, c.A = self.B.copy(), self.A.copy()
        return c


def gapx_iteration(links, scans, maxdist2, state=None):
    """one iteration of gapx6D::doGraphSlam6D (gapx6D.cc:323-542).  T (translation vector) keeps
    accumulating across iterations of one call, as the reference's does -- and so does the rotation
    system's matrix B, which is zeroed before the loop only (:359-366).  The vector A serves both
    systems: zeroed after the rotation solve (:458), filled by the translation step and not zeroed
    again, so the next iteration's rotation system starts from it.  Pass the returned GapxState back
    in for the next iteration (None, or a bare T, starts B and A at zero).  Returns (ret, state, X)."""
    n = len(scans) - 1
    if not isinstance(state, GapxState):
        state = GapxState(n, state)
    T, B, A = state.T, state.B, state.A
    cms, cds = [], []
    sum_position_diff = 0.0
    for (f, sx) in links:
        r = get_pt_pairs(scans[f], scans[sx], maxdist2)
        cms.append(r["cm"]); cds.append(r["cd"])
        if r["n"] <= 1:
            continue
        MkMkt, DkDkt, MkDkt, DkMkt, Ak1, Ak2 = gapx_link_blocks(r["p1"], r["p2"], r["cm"])
        a, b = f - 1, sx - 1
        if f != 0:
            A[a * 3:a * 3 + 3] += Ak1
            B[a * 3:a * 3 + 3, a * 3:a * 3 + 3] += MkMkt
            B[a * 3:a * 3 + 3, b * 3:b * 3 + 3] += DkMkt
            B[b * 3:b * 3 + 3, a * 3:a * 3 + 3] += MkDkt
        A[b * 3:b * 3 + 3] += Ak2
        B[b * 3:b * 3 + 3, b * 3:b * 3 + 3] += DkDkt
        sum_position_diff += 1.0                         # genBArotForLinkedPair returns 1.0 (sic)
    X = solve_chol_upper(B, A)
    sum_position_diff += gapx_translate_and_move(links, scans, cms, cds, X, T, A)
    return sum_position_diff / len(scans), state, X


# ---------------------------------------------------------------------------------------
# uos ASCII + .pose readers (src/scanio/helper.cc:192-234, 564-700): fixture generation only
# ---------------------------------------------------------------------------------------
def read_uos(path):
    pts = []
    with open(path) as f:
        for line in f:
            line = line.split("#", 1)[0].split()
            if len(line) == 3:          # "x y z" (an optional first count line has 1 field)
                pts.append((float(line[0]), float(line[1]), float(line[2])))
    return np.array(pts, dtype=np.float64)


def read_pose(path):
    v = [float(t) for t in open(path).read().split()[:6]]
    rPos = np.array(v[:3])
    rPosTheta = np.array([(2 * math.pi * a) / 360 for a in v[3:6]])   # rad(), globals.icc:172-175
    return rPos, rPosTheta
