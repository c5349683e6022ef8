"""Optimizer::BundleAdjustment (src/Optimizer.cc:56-255) restated in numpy: the checker of the
device's orbmi_bundle_adjustment.

g2o cannot be built for the tests and the C++ oracle's local_ba always runs LocalBA's two-stage
schedule, so this file states the reference's formulation once more, after oracle/lba_oracle.cpp:
one SparseOptimizer::optimize(n) of OptimizationAlgorithmLevenberg over BlockSolver_6_3, sequential
in edge order (numpy's ufunc.at and cumsum apply their operands one after another, in order), a
dense Schur complement and a dense Cholesky of S.  It states the formulation, not the device's
blocking.  test_gba_cpu.py anchors it to the C++ oracle.

run(problem, iterations, robust, stop_at_check=-1, solver="chol") -> dict like optimizer.GlobalBA.run.
solver="ldl" solves S by an unpivoted LDL^T instead: the variation a scene must be stable under.
"""
from __future__ import annotations

import numpy as np

TERMINATE, SOLVE_FAILED, REJECTED = 1, 2, 4
MAX_ITERATIONS = 64
DBL_MAX = np.finfo(np.float64).max


# ---- SE3Quat (g2o types/se3quat.h), quaternions as (x, y, z, w) ----------------------------
def _normalize_rotation(q):
    if q[3] < 0:
        q = -q
    return q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])


def _quat_from_matrix(m):
    q = np.zeros(4)
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    if tr > 0:
        t = np.sqrt(tr + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
    return q


def _quat_to_matrix(q):
    """Eigen toRotationMatrix; q (..., 4) -> (..., 3, 3)."""
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = 1 - (tyy + tzz); R[..., 0, 1] = txy - twz; R[..., 0, 2] = txz + twy
    R[..., 1, 0] = txy + twz; R[..., 1, 1] = 1 - (txx + tzz); R[..., 1, 2] = tyz - twx
    R[..., 2, 0] = txz - twy; R[..., 2, 1] = tyz + twx; R[..., 2, 2] = 1 - (txx + tyy)
    return R


def _quat_rotate(q, v):
    """Eigen _transformVector; q (..., 4), v (..., 3)."""
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    u0 = y * v[..., 2] - z * v[..., 1]
    u1 = z * v[..., 0] - x * v[..., 2]
    u2 = x * v[..., 1] - y * v[..., 0]
    u0, u1, u2 = u0 + u0, u1 + u1, u2 + u2
    c0, c1, c2 = y * u2 - z * u1, z * u0 - x * u2, x * u1 - y * u0
    return np.stack([v[..., 0] + w * u0 + c0, v[..., 1] + w * u1 + c1, v[..., 2] + w * u2 + c2], -1)


def _quat_mul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                     a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
                     a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def se3_from_tcw(tcw):
    """Converter::toSE3Quat: float Tcw (16) -> (q, t)."""
    T = np.asarray(tcw, np.float32).reshape(4, 4).astype(np.float64)
    return _normalize_rotation(_quat_from_matrix(T[:3, :3])), T[:3, 3].copy()


def se3_to_tcw(q, t):
    """Converter::toCvMat(SE3Quat): float 4x4."""
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = _quat_to_matrix(np.asarray(q)).astype(np.float32)
    T[:3, 3] = np.asarray(t).astype(np.float32)
    return T


def _se3_exp(u):
    w, up = u[:3], u[3:]
    theta = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    O = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    O2 = O @ O
    if theta < 0.00001:
        R = np.eye(3) + O + O2
        V = R
    else:
        a, b = np.sin(theta) / theta, (1 - np.cos(theta)) / (theta * theta)
        c = (theta - np.sin(theta)) / theta ** 3
        R = np.eye(3) + a * O + b * O2
        V = np.eye(3) + b * O + c * O2
    return _normalize_rotation(_quat_from_matrix(R)), V @ up


def _se3_oplus(u, q, t):
    """exp(u) * T (VertexSE3Expmap::oplusImpl)."""
    qe, te = _se3_exp(u)
    return _normalize_rotation(_quat_mul(qe, q)), te + _quat_rotate(qe, t)


# ---- the graph ------------------------------------------------------------------------------
class _Graph:
    def __init__(self, problem, robust):
        K, P, E = problem.kfs, problem.pts, problem.edges
        self.nkf, self.npt, self.ne = len(K), len(P), len(E)
        qt = [se3_from_tcw(k["tcw"]) for k in K]
        self.q = np.array([a for a, _ in qt], np.float64).reshape(-1, 4)
        self.t = np.array([b for _, b in qt], np.float64).reshape(-1, 3)
        self.X = P["pos"].astype(np.float64).reshape(-1, 3)
        self.pt = E["point"].astype(np.int64)
        self.kf = E["kf"].astype(np.int64)
        self.stereo = ~(E["ur"] < 0)
        self.obs = np.stack([E["u"], E["v"], np.where(self.stereo, E["ur"], 0)], -1).astype(np.float64)
        self.info = E["inv_sigma2"].astype(np.float64)
        self.fx, self.fy, self.cx, self.cy = (K[n][self.kf].astype(np.float64) for n in ("fx", "fy", "cx", "cy"))
        self.bf32 = K["bf"][self.kf].astype(np.float32)
        self.bf = self.bf32.astype(np.float64)
        # src/Optimizer.cc:106-107: const float thHuber2D = sqrt(5.99), thHuber3D = sqrt(7.815)
        self.delta = np.where(self.stereo, np.float64(np.float32(np.sqrt(7.815))), np.float64(np.float32(np.sqrt(5.99))))
        self.robust = bool(robust)
        # the pose blocks: free keyframes that an edge names, in id order; points with an edge
        named = np.zeros(self.nkf, bool)
        named[self.kf] = True
        self.rank = np.full(self.nkf, -1, np.int64)
        order = np.argsort(K["id"], kind="stable")
        free = [int(k) for k in order if not K["fixed"][k] and named[k]]
        self.rank[free] = np.arange(len(free))
        self.free = np.asarray(free, np.int64)
        self.np_ = len(free)
        self.included = np.zeros(self.npt, bool)
        self.included[self.pt] = True
        self.pi = self.rank[self.kf]                     # pose block of each edge, -1 fixed
        self.fe = np.nonzero(self.pi >= 0)[0]            # edges into a free pose, in edge order
        # ordered pairs (a1, a2) of the free edges of one point: landmark, a1, a2 order
        cnt = np.bincount(self.pt[self.fe], minlength=self.npt)
        start = np.concatenate([[0], np.cumsum(cnt)])
        m = cnt[self.pt[self.fe]]                        # per free edge: its point's free edges
        a1 = np.repeat(np.arange(len(self.fe)), m)
        first = np.repeat(start[self.pt[self.fe]], m)
        within = np.arange(len(a1)) - np.repeat(np.concatenate([[0], np.cumsum(m)])[:-1], m)
        self.p1, self.p2 = self.fe[a1], self.fe[first + within]
        self.err = np.zeros((self.ne, 3))

    def compute_errors(self):
        p = _quat_rotate(self.q[self.kf], self.X[self.pt]) + self.t[self.kf]
        with np.errstate(all="ignore"):
            px, py = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
            m0 = self.obs[:, 0] - (px * self.fx + self.cx)
            m1 = self.obs[:, 1] - (py * self.fy + self.cy)
            invz32 = (1.0 / p[:, 2]).astype(np.float32)   # float invz (types_six_dof_expmap.cpp:151)
            invz = invz32.astype(np.float64)
            r0 = p[:, 0] * invz * self.fx + self.cx
            r1 = p[:, 1] * invz * self.fy + self.cy
            r2 = r0 - (self.bf32 * invz32).astype(np.float64)
        s = self.stereo
        self.err = np.stack([np.where(s, self.obs[:, 0] - r0, m0), np.where(s, self.obs[:, 1] - r1, m1),
                             np.where(s, self.obs[:, 2] - r2, 0.0)], -1)

    def chi2_edges(self):
        e, i = self.err, self.info
        c = e[:, 0] * (i * e[:, 0]) + e[:, 1] * (i * e[:, 1])
        return np.where(self.stereo, c + e[:, 2] * (i * e[:, 2]), c)

    def robustify(self, c):
        """RobustKernelHuber: (rho, rho') per edge."""
        if not self.robust:
            return c, np.ones_like(c)
        d, dsqr = self.delta, self.delta * self.delta
        with np.errstate(all="ignore"):
            s = np.sqrt(c)
            big = ~(c <= dsqr)
            return np.where(big, 2 * s * d - dsqr, c), np.where(big, d / s, 1.0)

    def active_robust_chi2(self):
        rho = self.robustify(self.chi2_edges())[0]
        return float(np.cumsum(rho)[-1]) if self.ne else 0.0

    def jacobians(self):
        p = _quat_rotate(self.q[self.kf], self.X[self.pt]) + self.t[self.kf]
        R = _quat_to_matrix(self.q[self.kf])
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        fx, fy, bf, s = self.fx, self.fy, self.bf, self.stereo
        Jl, Jp = np.zeros((self.ne, 3, 3)), np.zeros((self.ne, 3, 6))
        with np.errstate(all="ignore"):
            z2 = z * z
            t02, t12 = -x / z * fx, -y / z * fy
            for c in range(3):
                mono0 = -1. / z * (fx * R[:, 0, c] + 0 * R[:, 1, c] + t02 * R[:, 2, c])
                mono1 = -1. / z * (0 * R[:, 0, c] + fy * R[:, 1, c] + t12 * R[:, 2, c])
                st0 = -fx * R[:, 0, c] / z + fx * x * R[:, 2, c] / z2
                st1 = -fy * R[:, 1, c] / z + fy * y * R[:, 2, c] / z2
                Jl[:, 0, c] = np.where(s, st0, mono0)
                Jl[:, 1, c] = np.where(s, st1, mono1)
                Jl[:, 2, c] = np.where(s, st0 - bf * R[:, 2, c] / z2, 0.0)
            Jp[:, 0, 0] = x * y / z2 * fx; Jp[:, 0, 1] = -(1 + (x * x / z2)) * fx; Jp[:, 0, 2] = y / z * fx
            Jp[:, 0, 3] = -1. / z * fx; Jp[:, 0, 5] = x / z2 * fx
            Jp[:, 1, 0] = (1 + y * y / z2) * fy; Jp[:, 1, 1] = -x * y / z2 * fy; Jp[:, 1, 2] = -x / z * fy
            Jp[:, 1, 4] = -1. / z * fy; Jp[:, 1, 5] = y / z2 * fy
            Jp[:, 2, 0] = np.where(s, Jp[:, 0, 0] - bf * y / z2, 0.0)
            Jp[:, 2, 1] = np.where(s, Jp[:, 0, 1] + bf * x / z2, 0.0)
            Jp[:, 2, 2] = np.where(s, Jp[:, 0, 2], 0.0)
            Jp[:, 2, 3] = np.where(s, Jp[:, 0, 3], 0.0)
            Jp[:, 2, 5] = np.where(s, Jp[:, 0, 5] - bf / z2, 0.0)
        return Jl, Jp

    def build_system(self):
        """BlockSolver::buildSystem: every edge's constructQuadraticForm, in edge order."""
        Jl, Jp = self.jacobians()
        rho1 = self.robustify(self.chi2_edges())[1]
        with np.errstate(all="ignore"):
            w = rho1 * self.info if self.robust else self.info
            om = -(self.info[:, None] * self.err) * (rho1[:, None] if self.robust else 1.0)
            self.bl = np.zeros((self.npt, 3))
            self.Hll = np.zeros((self.npt, 3, 3))
            for r in range(3):
                np.add.at(self.bl[:, r], np.repeat(self.pt, 3), (Jl[:, :, r] * om).reshape(-1))
                for c in range(3):
                    h = Jl[:, 0, r] * w * Jl[:, 0, c] + Jl[:, 1, r] * w * Jl[:, 1, c] + Jl[:, 2, r] * w * Jl[:, 2, c]
                    np.add.at(self.Hll[:, r, c], self.pt, h)
            fe, pi = self.fe, self.pi[self.fe]
            self.bp = np.zeros((self.np_, 6))
            self.Hpp = np.zeros((self.np_, 6, 6))
            self.B = np.zeros((self.ne, 6, 3))
            for r in range(6):
                np.add.at(self.bp[:, r], np.repeat(pi, 3), (Jp[fe, :, r] * om[fe]).reshape(-1))
                for c in range(6):
                    h = Jp[:, 0, r] * w * Jp[:, 0, c] + Jp[:, 1, r] * w * Jp[:, 1, c] + Jp[:, 2, r] * w * Jp[:, 2, c]
                    np.add.at(self.Hpp[:, r, c], pi, h[fe])
                for c in range(3):
                    self.B[:, r, c] = Jp[:, 0, r] * w * Jl[:, 0, c] + Jp[:, 1, r] * w * Jl[:, 1, c] + Jp[:, 2, r] * w * Jl[:, 2, c]

    def lambda_init(self):
        m = 0.0
        if self.np_:
            m = max(m, float(np.nanmax(np.abs(self.Hpp[:, range(6), range(6)]), initial=0.0)))
        inc = self.included
        if inc.any():
            m = max(m, float(np.nanmax(np.abs(self.Hll[inc][:, range(3), range(3)]), initial=0.0)))
        return 1e-5 * m

    def schur(self, lam):
        """S = Hpp + lambda I - sum_p B_ip (Hll_p + lambda I)^-1 B_jp^T, b_S likewise (dense)."""
        N = 6 * self.np_
        with np.errstate(all="ignore"):
            D = self.Hll + lam * np.eye(3)
            c00 = D[:, 1, 1] * D[:, 2, 2] - D[:, 1, 2] * D[:, 2, 1]
            c10 = D[:, 1, 2] * D[:, 2, 0] - D[:, 1, 0] * D[:, 2, 2]
            c20 = D[:, 1, 0] * D[:, 2, 1] - D[:, 1, 1] * D[:, 2, 0]
            det = D[:, 0, 0] * c00 + D[:, 0, 1] * c10 + D[:, 0, 2] * c20
            Di = np.empty_like(D)
            Di[:, 0, 0] = c00 / det; Di[:, 1, 0] = c10 / det; Di[:, 2, 0] = c20 / det
            Di[:, 0, 1] = (D[:, 0, 2] * D[:, 2, 1] - D[:, 0, 1] * D[:, 2, 2]) / det
            Di[:, 1, 1] = (D[:, 0, 0] * D[:, 2, 2] - D[:, 0, 2] * D[:, 2, 0]) / det
            Di[:, 2, 1] = (D[:, 0, 1] * D[:, 2, 0] - D[:, 0, 0] * D[:, 2, 1]) / det
            Di[:, 0, 2] = (D[:, 0, 1] * D[:, 1, 2] - D[:, 0, 2] * D[:, 1, 1]) / det
            Di[:, 1, 2] = (D[:, 0, 2] * D[:, 1, 0] - D[:, 0, 0] * D[:, 1, 2]) / det
            Di[:, 2, 2] = (D[:, 0, 0] * D[:, 1, 1] - D[:, 0, 1] * D[:, 1, 0]) / det
            self.Dinv = Di
            db = Di[:, :, 0] * self.bl[:, 0:1] + Di[:, :, 1] * self.bl[:, 1:2] + Di[:, :, 2] * self.bl[:, 2:3]
            S = np.zeros((N, N))
            bs = np.zeros(N)
            for i in range(self.np_):
                S[6 * i:6 * i + 6, 6 * i:6 * i + 6] = self.Hpp[i] + lam * np.eye(6)
                bs[6 * i:6 * i + 6] = self.bp[i]
            fe = self.fe
            if len(fe):
                B1, d1 = self.B[fe], db[self.pt[fe]]
                v = B1[:, :, 0] * d1[:, 0:1] + B1[:, :, 1] * d1[:, 1:2] + B1[:, :, 2] * d1[:, 2:3]
                np.subtract.at(bs, (6 * self.pi[fe])[:, None] + np.arange(6), v)
                Bp, Dp, B2 = self.B[self.p1], Di[self.pt[self.p1]], self.B[self.p2]
                BD = Bp[:, :, 0:1] * Dp[:, None, 0, :] + Bp[:, :, 1:2] * Dp[:, None, 1, :] + Bp[:, :, 2:3] * Dp[:, None, 2, :]
                v = (BD[:, :, None, 0] * B2[:, None, :, 0] + BD[:, :, None, 1] * B2[:, None, :, 1]
                     + BD[:, :, None, 2] * B2[:, None, :, 2])
                rows = (6 * self.pi[self.p1])[:, None, None] + np.arange(6)[None, :, None] + np.zeros((1, 1, 6), np.int64)
                cols = (6 * self.pi[self.p2])[:, None, None] + np.arange(6)[None, None, :] + np.zeros((1, 6, 1), np.int64)
                np.subtract.at(S, (rows, cols), v)
        return S, bs

    def back_substitute(self, xp):
        """x_l = D^-1 (b_l - sum B^T x_p), the sums in edge order."""
        cl = self.bl.copy()
        fe = self.fe
        with np.errstate(all="ignore"):
            if len(fe):
                xe = xp.reshape(-1, 6)[self.pi[fe]]                        # (nfe, 6)
                v = np.transpose(self.B[fe], (0, 2, 1)) * xe[:, None, :]   # (nfe, c, r)
                idx = (3 * self.pt[fe])[:, None, None] + np.arange(3)[None, :, None] + np.zeros((1, 1, 6), np.int64)
                flat = cl.reshape(-1)
                np.subtract.at(flat, idx.reshape(-1), v.reshape(-1))
                cl = flat.reshape(-1, 3)
            Di = self.Dinv
            return Di[:, :, 0] * cl[:, 0:1] + Di[:, :, 1] * cl[:, 1:2] + Di[:, :, 2] * cl[:, 2:3]


def ldlt_solve(S, b):
    """Unpivoted right-looking LDL^T; None when a pivot is not a positive finite number."""
    A, n = S.copy(), len(b)
    y = b.copy()
    with np.errstate(all="ignore"):
        for j in range(n):
            d = A[j, j]
            if not (d > 0 and np.isfinite(d)):
                return None
            col = A[j + 1:, j] / d
            A[j + 1:, j + 1:] -= np.outer(col, A[j + 1:, j])
            y[j + 1:] -= col * y[j]
            A[j + 1:, j] = col
        y /= np.diag(A)
        for j in range(n - 1, 0, -1):
            y[:j] -= A[j, :j] * y[j]
    return y


def chol_solve(S, b):
    """Dense Cholesky; None when S is not positive definite or not finite."""
    if not np.isfinite(S).all() or not np.isfinite(b).all():
        return None
    try:
        L = np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        return None
    n = len(b)
    y = np.linalg.solve(L, b) if n else b.copy()
    x = np.linalg.solve(L.T, y) if n else y
    return x if np.isfinite(x).all() else None


def run(problem, iterations=10, robust=False, stop_at_check=-1, solver="chol"):
    if not 0 <= iterations <= MAX_ITERATIONS:
        raise ValueError("iterations")
    g = _Graph(problem, robust)
    checks, stop_seen = 0, -1

    def terminate():
        nonlocal checks, stop_seen
        idx = checks
        checks += 1
        s = stop_at_check >= 0 and idx >= stop_at_check
        if s and stop_seen < 0:
            stop_seen = idx
        return s

    solve = chol_solve if solver == "chol" else ldlt_solve
    trials = np.zeros(MAX_ITERATIONS, np.int32)
    status, it, lam, ni, n_bad = 0, 0, 0.0, 2.0, 0
    chi_initial = chi_last = 0.0
    empty = g.ne == 0
    i = 0
    with np.errstate(all="ignore"):
        while not empty and i < iterations and not terminate():
            g.compute_errors()
            current = g.active_robust_chi2()
            ini = current
            g.build_system()
            if i == 0:
                lam, ni, n_bad = g.lambda_init(), 2.0, 0
                chi_initial = current
            rho, qmax = 0.0, 0
            while True:
                q0, t0, X0 = g.q.copy(), g.t.copy(), g.X.copy()
                S, bs = g.schur(lam)
                xp = solve(S, bs) if len(bs) else bs
                ok2 = xp is not None
                if ok2:
                    xl = g.back_substitute(xp)
                    for k, kf in enumerate(g.free):
                        g.q[kf], g.t[kf] = _se3_oplus(xp[6 * k:6 * k + 6], g.q[kf], g.t[kf])
                    g.X[g.included] = g.X[g.included] + xl[g.included]
                else:
                    status |= SOLVE_FAILED
                    xp, xl = np.zeros(6 * g.np_), np.zeros((g.npt, 3))
                g.compute_errors()
                chi_last = g.active_robust_chi2()
                temp = chi_last if ok2 else DBL_MAX
                xs = np.concatenate([xp, xl[g.included].reshape(-1)])
                bb = np.concatenate([g.bp.reshape(-1), g.bl[g.included].reshape(-1)])
                terms = xs * (lam * xs + bb)
                scale = (float(np.cumsum(terms)[-1]) if len(terms) else 0.0) + 1e-3
                rho = (current - temp) / scale
                if rho > 0 and np.isfinite(temp):
                    alpha = min(1. - (2 * rho - 1) ** 3, 2. / 3.)
                    lam *= max(1. / 3., alpha)
                    ni = 2.0
                    current = temp
                else:
                    lam *= ni
                    ni *= 2
                    g.q, g.t, g.X = q0, t0, X0
                    status |= REJECTED
                qmax += 1
                trials[i] = qmax
                if not (rho < 0 and qmax < 10 and not terminate()):
                    break
            it += 1
            i += 1
            if qmax == 10 or rho == 0:
                status |= TERMINATE
                break
            n_bad = n_bad + 1 if (ini - current) * 1e3 < ini else 0
            if n_bad >= 3:
                status |= TERMINATE
                break
    if empty:
        status |= TERMINATE
    tcw = problem.kfs["tcw"].reshape(-1, 4, 4).copy()
    for kf in g.free:
        tcw[kf] = se3_to_tcw(g.q[kf], g.t[kf])
    pos = problem.pts["pos"].reshape(-1, 3).copy()
    pos[g.included] = g.X[g.included].astype(np.float32)
    return {"tcw": tcw, "pos": pos, "included": g.included.copy(), "iterations": it, "trials": trials[:iterations].copy(),
            "chi2_initial": chi_initial, "chi2": chi_last, "stop_check": stop_seen, "checks": checks, "status": status,
            "n_free": g.np_, "pose64": (g.q.copy(), g.t.copy()), "pos64": g.X.copy()}


class ReferenceBackend:
    """The restatement behind loop.global_bundle_adjustment's backend interface."""

    def bundle_adjustment(self, problem, iterations=10, robust=False, stop=None, stop_at_check=None):
        at = -1 if stop_at_check is None else stop_at_check
        if stop is not None and stop.value:
            at = 0
        return run(problem, iterations, robust, at)
