"""Numpy restatement of csrc/sim3_opt.h (Optimizer::OptimizeSim3, src/Optimizer.cc:1145-1347, with
the bundled g2o's semantics), operation for operation after g2o's sources: Sim3(Vector7d), the
Sim3 product, inverse and map (types/sim3.h), the two projection edges
(types/types_seven_dof_expmap.h), BaseBinaryEdge's numeric linearizeOplus and
constructQuadraticForm, the Huber kernel, the dense damped solve and
OptimizationAlgorithmLevenberg::solve with the bundled stop rules.  It is the checker of the host
header (tests/cpp/sim3opt_check.cpp), of the device kernel and of optimizer.Sim3Optimizer.

Two Jacobian modes: "numeric" is g2o's (central differences with delta = 1e-9 through oplus);
"analytic" is the independent check of the restatement, from the left update with generator
G(y) = [-[y]x | I | y]:  J12 = -dpi(y) G(y), y = S x;  J21 = +dpi(y') (1/s) R^T G(x), y' = S^-1 x.

Everything is vectorised over the correspondences: numpy's elementwise +, -, *, /, sqrt round once
per operation like the scalar code; the sums over the edges are sequential (cumsum) in the edge
order e12(0), e21(0), e12(1), ...  Also the seeded two-camera scene and the committed problem list
the tests share."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
DELTA = 1e-9
MAX_TRIALS = 10
TH2 = 10.0  # LoopClosing::ComputeSim3 calls OptimizeSim3(..., 10, mbFixScale)


# ---- quaternions and Sim3 (types/sim3.h) --------------------------------------------------------

def quat_from_R(m):
    """Eigen::Quaternion(const Matrix3&); m row-major (9), q = x y z w, not normalised."""
    m = [F64(v) for v in np.asarray(m, F64).reshape(9)]
    q = [F64(0)] * 4
    tr = (m[0] + m[4]) + m[8]
    if tr > 0:
        t = np.sqrt(tr + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[7] - m[5]) * t
        q[1] = (m[2] - m[6]) * t
        q[2] = (m[3] - m[1]) * t
        return np.array(q, F64)
    i = 0
    if m[4] > m[0]:
        i = 1
    if m[8] > (m[4] if i == 1 else m[0]):
        i = 2
    if i == 0:
        t = np.sqrt(((m[0] - m[4]) - m[8]) + 1.0)
        q[0] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[7] - m[5]) * t
        q[1] = (m[3] + m[1]) * t
        q[2] = (m[6] + m[2]) * t
    elif i == 1:
        t = np.sqrt(((m[4] - m[8]) - m[0]) + 1.0)
        q[1] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[2] - m[6]) * t
        q[2] = (m[7] + m[5]) * t
        q[0] = (m[1] + m[3]) * t
    else:
        t = np.sqrt(((m[8] - m[0]) - m[4]) + 1.0)
        q[2] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[3] - m[1]) * t
        q[0] = (m[2] + m[6]) * t
        q[1] = (m[5] + m[7]) * t
    return np.array(q, F64)


def quat_to_R(q):
    """Eigen toRotationMatrix, row-major 3x3."""
    x, y, z, w = (F64(v) for v in q)
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]], F64)


def quat_mul(a, b):
    a = [F64(v) for v in a]
    b = [F64(v) for v in b]
    x = ((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1]
    y = ((a[3] * b[1] + a[1] * b[3]) + a[2] * b[0]) - a[0] * b[2]
    z = ((a[3] * b[2] + a[2] * b[3]) + a[0] * b[1]) - a[1] * b[0]
    w = ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2]
    return np.array([x, y, z, w], F64)


def rotate(q, v):
    """Eigen's quaternion * vector, v (..., 3)."""
    q = [F64(c) for c in q]
    v = np.asarray(v, F64)
    v0, v1, v2 = v[..., 0], v[..., 1], v[..., 2]
    ux = q[1] * v2 - q[2] * v1
    uy = q[2] * v0 - q[0] * v2
    uz = q[0] * v1 - q[1] * v0
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    cx = q[1] * uz - q[2] * uy
    cy = q[2] * ux - q[0] * uz
    cz = q[0] * uy - q[1] * ux
    return np.stack([(v0 + q[3] * ux) + cx, (v1 + q[3] * uy) + cy, (v2 + q[3] * uz) + cz], -1)


class Sim3:
    __slots__ = ("q", "t", "s")

    def __init__(self, q, t, s):
        self.q = np.asarray(q, F64).copy()
        self.t = np.asarray(t, F64).copy()
        self.s = F64(s)

    @staticmethod
    def from_rts(R, t, s):
        """g2o::Sim3(Matrix3d, Vector3d, double) from the caller's floats."""
        return Sim3(quat_from_R(np.asarray(R, F32).astype(F64)), np.asarray(t, F32).astype(F64), F64(F32(s)))

    def map(self, x):
        return self.s * rotate(self.q, x) + self.t

    def mul(self, o):
        return Sim3(quat_mul(self.q, o.q), self.s * rotate(self.q, o.t) + self.t, self.s * o.s)

    def inverse(self):
        qc = np.array([-self.q[0], -self.q[1], -self.q[2], self.q[3]], F64)
        m = F64(-1.) / self.s
        return Sim3(qc, rotate(qc, m * self.t), F64(1.) / self.s)

    def matrix(self):
        """s R and t in doubles."""
        return self.s * quat_to_R(self.q), self.t.copy()

    def to_float(self):
        """Converter::toCvMat(g2o::Sim3): (float)(s * R), (float)t."""
        return (self.s * quat_to_R(self.q)).astype(F32), self.t.astype(F32)

    def bits(self):
        return np.concatenate([self.q, self.t, [self.s]]).astype(F64).tobytes()


def sim3_exp(u):
    """Sim3(const Vector7d&), types/sim3.h:70-142."""
    u = [F64(v) for v in u]
    w0, w1, w2, sigma = u[0], u[1], u[2], u[6]
    theta = np.sqrt((w0 * w0 + w1 * w1) + w2 * w2)
    z = F64(0)
    Om = [z, -w2, w1, w2, z, -w0, -w1, w0, z]
    Om2 = [(Om[3 * r] * Om[c] + Om[3 * r + 1] * Om[3 + c]) + Om[3 * r + 2] * Om[6 + c] for r in range(3) for c in range(3)]
    s = F64(math.exp(sigma))
    eps = 0.00001
    small = bool(theta < eps)
    sn, cs, ra, rb = F64(0), F64(1), F64(1), F64(1)
    if not small:
        sn, cs = F64(math.sin(theta)), F64(math.cos(theta))
        ra = sn / theta
        rb = (1 - cs) / (theta * theta)
    if abs(sigma) < eps:
        C = F64(1)
        if small:
            A, B = F64(1. / 2.), F64(1. / 6.)
        else:
            theta2 = theta * theta
            A = (1 - cs) / theta2
            B = (theta - sn) / (theta2 * theta)
    else:
        C = (s - 1) / sigma
        if small:
            sigma2 = sigma * sigma
            A = ((sigma - 1) * s + 1) / sigma2
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
        else:
            a, b, theta2, sigma2 = s * sn, s * cs, theta * theta, sigma * sigma
            c = theta2 + sigma2
            A = (a * sigma + (1 - b) * theta) / (theta * c)
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2
    R, W = [], []
    for k in range(9):
        I = F64(1.0 if k in (0, 4, 8) else 0.0)
        R.append((I + Om[k]) + Om2[k] if small else (I + ra * Om[k]) + rb * Om2[k])
        W.append((A * Om[k] + B * Om2[k]) + C * I)
    t = [(W[3 * r] * u[3] + W[3 * r + 1] * u[4]) + W[3 * r + 2] * u[5] for r in range(3)]
    return Sim3(quat_from_R(R), t, s)


def oplus(S, x, fix_scale):
    """VertexSim3Expmap::oplusImpl."""
    u = [F64(v) for v in x]
    if fix_scale:
        u[6] = F64(0)
    return sim3_exp(u).mul(S)


# ---- the edges ----------------------------------------------------------------------------------

def edge_error(T, X, obs, k):
    """obs - cam_map(project(T.map(X))), (n, 2)."""
    y = T.map(X)
    px, py = y[:, 0] / y[:, 2], y[:, 1] / y[:, 2]
    return np.stack([obs[:, 0] - (px * k[0] + k[2]), obs[:, 1] - (py * k[1] + k[3])], -1)


def chi2_of(e, w):
    return e[:, 0] * (w * e[:, 0]) + e[:, 1] * (w * e[:, 1])


def huber(c, delta, dsqr):
    """RobustKernelHuber::robustify: rho[0], rho[1]."""
    inl = c <= dsqr
    with np.errstate(invalid="ignore", divide="ignore"):
        sq = np.sqrt(np.where(inl, F64(1), c))
        rho0 = np.where(inl, c, 2 * sq * delta - dsqr)
        rho1 = np.where(inl, F64(1), delta / sq)
    return rho0, rho1


class Problem:
    """One OptimizeSim3 problem as orbmi_sim3_opt_problem holds it (float32 arrays)."""

    def __init__(self, x3d_c1, x3d_c2, obs1, obs2, inv_sigma2_1, inv_sigma2_2, k1, k2, th2, fix_scale, R12, t12, s12,
                 truth=None):
        self.x3d_c1 = np.ascontiguousarray(x3d_c1, F32).reshape(-1, 3)
        self.x3d_c2 = np.ascontiguousarray(x3d_c2, F32).reshape(-1, 3)
        self.obs1 = np.ascontiguousarray(obs1, F32).reshape(-1, 2)
        self.obs2 = np.ascontiguousarray(obs2, F32).reshape(-1, 2)
        self.inv_sigma2_1 = np.ascontiguousarray(inv_sigma2_1, F32).reshape(-1)
        self.inv_sigma2_2 = np.ascontiguousarray(inv_sigma2_2, F32).reshape(-1)
        self.k1 = np.ascontiguousarray(k1, F32).reshape(4)
        self.k2 = np.ascontiguousarray(k2, F32).reshape(4)
        self.th2 = F32(th2)
        self.fix_scale = int(bool(fix_scale))
        self.R12 = np.ascontiguousarray(R12, F32).reshape(3, 3)
        self.t12 = np.ascontiguousarray(t12, F32).reshape(3)
        self.s12 = F32(s12)
        self.truth = truth
        self.n = len(self.x3d_c1)

    def initial(self):
        return Sim3.from_rts(self.R12.reshape(9), self.t12, self.s12)


class _Opt:
    def __init__(self, P, mode):
        self.P, self.mode = P, mode
        self.X1, self.X2 = P.x3d_c1.astype(F64), P.x3d_c2.astype(F64)
        self.o1, self.o2 = P.obs1.astype(F64), P.obs2.astype(F64)
        self.w1, self.w2 = P.inv_sigma2_1.astype(F64), P.inv_sigma2_2.astype(F64)
        self.k1, self.k2 = P.k1.astype(F64), P.k2.astype(F64)
        self.delta = F64(np.sqrt(P.th2))  # float sqrt of the float th2
        self.dsqr = self.delta * self.delta
        self.th2 = F64(P.th2)
        self.fix = P.fix_scale
        self.alive = np.ones(P.n, bool)
        self.chi2 = np.zeros((P.n, 2), F64)
        self.trace = []

    # computeActiveErrors + activeRobustChi2
    def errors(self, S):
        Si = S.inverse()
        c12 = chi2_of(edge_error(S, self.X2, self.o1, self.k1), self.w1)
        c21 = chi2_of(edge_error(Si, self.X1, self.o2, self.k2), self.w2)
        a = self.alive
        self.chi2[a, 0] = c12[a]
        self.chi2[a, 1] = c21[a]
        r12, _ = huber(c12, self.delta, self.dsqr)
        r21, _ = huber(c21, self.delta, self.dsqr)
        per = (r12 + r21)[a]
        return F64(np.cumsum(per)[-1]) if len(per) else F64(0)

    def jacobians(self, S, mode=None):
        """J12, J21: (n, 2, 7)."""
        mode = mode or self.mode
        n = self.P.n
        J12, J21 = np.zeros((n, 2, 7), F64), np.zeros((n, 2, 7), F64)
        if mode == "numeric":
            scalar = F64(1.0) / (2 * F64(DELTA))
            for d in range(7):
                if d == 6 and self.fix:
                    continue  # both pushed estimates are the same: exactly 0
                u = [F64(0)] * 7
                u[d] = F64(DELTA)
                Pp = oplus(S, u, self.fix)
                u[d] = F64(-DELTA)
                Pm = oplus(S, u, self.fix)
                J12[:, :, d] = scalar * (edge_error(Pp, self.X2, self.o1, self.k1) - edge_error(Pm, self.X2, self.o1, self.k1))
                Ppi, Pmi = Pp.inverse(), Pm.inverse()
                J21[:, :, d] = scalar * (edge_error(Ppi, self.X1, self.o2, self.k2) - edge_error(Pmi, self.X1, self.o2, self.k2))
            return J12, J21

        def G(y):
            g = np.zeros((n, 3, 7), F64)
            g[:, 0, 1], g[:, 0, 2] = y[:, 2], -y[:, 1]
            g[:, 1, 0], g[:, 1, 2] = -y[:, 2], y[:, 0]
            g[:, 2, 0], g[:, 2, 1] = y[:, 1], -y[:, 0]
            g[:, 0, 3] = g[:, 1, 4] = g[:, 2, 5] = 1
            g[:, :, 6] = y
            return g

        def dpi(y, k):
            d = np.zeros((n, 2, 3), F64)
            d[:, 0, 0] = k[0] / y[:, 2]
            d[:, 0, 2] = -k[0] * y[:, 0] / (y[:, 2] * y[:, 2])
            d[:, 1, 1] = k[1] / y[:, 2]
            d[:, 1, 2] = -k[1] * y[:, 1] / (y[:, 2] * y[:, 2])
            return d

        qn = S.q / np.linalg.norm(S.q)
        R = quat_to_R(qn)
        J12 = -np.einsum("nij,njk->nik", dpi(S.map(self.X2), self.k1), G(S.map(self.X2)))
        yi = S.inverse().map(self.X1)
        J21 = np.einsum("nij,jl,nlk->nik", dpi(yi, self.k2), R.T / S.s, G(self.X1))
        if self.fix:
            J12[:, :, 6] = 0
            J21[:, :, 6] = 0
        return J12, J21

    # buildSystem at the estimate the errors were last computed at
    def build(self, S, mode=None):
        Si = S.inverse()
        J12, J21 = self.jacobians(S, mode)
        rows = []
        for J, e, w in ((J12, edge_error(S, self.X2, self.o1, self.k1), self.w1),
                        (J21, edge_error(Si, self.X1, self.o2, self.k2), self.w2)):
            c = chi2_of(e, w)
            rho0, rho1 = huber(c, self.delta, self.dsqr)
            ww = rho1 * w
            r0, r1 = -(w * e[:, 0]) * rho1, -(w * e[:, 1]) * rho1
            nd = 6 if self.fix else 7
            acc = np.zeros((self.P.n, 36), F64)
            q = 0
            for r in range(7):
                for cc in range(r, 7):
                    if cc < nd:
                        acc[:, q] = (J[:, 0, r] * ww) * J[:, 0, cc] + (J[:, 1, r] * ww) * J[:, 1, cc]
                    q += 1
                if r < nd:
                    acc[:, 28 + r] = J[:, 0, r] * r0 + J[:, 1, r] * r1
            acc[:, 35] = rho0
            rows.append(acc)
        inter = np.stack(rows, 1)[self.alive].reshape(-1, 36)  # e12(0), e21(0), e12(1), ...
        tot = np.cumsum(inter, 0)[-1] if len(inter) else np.zeros(36, F64)
        H = np.zeros((7, 7), F64)
        q = 0
        for r in range(7):
            for cc in range(r, 7):
                H[r, cc] = H[cc, r] = tot[q]
                q += 1
        return H, tot[28:35].copy(), F64(tot[35])

    @staticmethod
    def solve7(H, b, lam):
        """The unpivoted LDL^T of csrc/sim3_opt.h s3o_solve7."""
        A = np.array(H, F64)
        for j in range(7):
            A[j, j] = A[j, j] + lam
        D, ok = np.zeros(7, F64), True
        for j in range(7):
            d = A[j, j]
            for k in range(j):
                d = d - (A[j, k] * A[j, k]) * D[k]
            ok = ok and bool(d > 0) and bool(d < np.inf)
            D[j] = d
            with np.errstate(all="ignore"):
                for i in range(j + 1, 7):
                    s = A[i, j]
                    for k in range(j):
                        s = s - (A[i, k] * A[j, k]) * D[k]
                    A[i, j] = s / d
        if not ok:
            return False, np.zeros(7, F64)
        y = np.zeros(7, F64)
        for i in range(7):
            s = b[i]
            for k in range(i):
                s = s - A[i, k] * y[k]
            y[i] = s
        y = y / D
        x = np.zeros(7, F64)
        for i in range(6, -1, -1):
            s = y[i]
            for k in range(i + 1, 7):
                s = s - A[k, i] * x[k]
            x[i] = s
        return True, x

    def optimize(self, S, iterations):
        """SparseOptimizer::optimize with OptimizationAlgorithmLevenberg::solve.  Returns the
        estimate and the iterations run."""
        if not self.alive.any():
            return S, 0
        lam = ni = F64(0)
        nbad = done = 0
        with np.errstate(all="ignore"):
            for it in range(iterations):
                H, b, chi = self.build(S)
                current = ini = chi
                if it == 0:
                    m = F64(0)
                    for j in range(7):
                        a = abs(H[j, j])
                        m = a if a > m else m
                    lam, ni, nbad = F64(1e-5) * m, F64(2), 0
                rho, qmax = F64(0), 0
                while True:
                    ok2, x = self.solve7(H, b, lam)
                    T = oplus(S, x, self.fix) if ok2 else S
                    temp = self.errors(T)
                    if not ok2:
                        temp = F64(np.finfo(F64).max)
                    scale = F64(0)
                    for j in range(7):
                        scale = scale + x[j] * (lam * x[j] + b[j])
                    scale = scale + 1e-3
                    rho = (current - temp) / scale
                    accept = bool(rho > 0) and bool(np.isfinite(temp))
                    self.trace.append("A" if accept else "R")
                    if accept:
                        z = 2 * rho - 1
                        alpha = 1. - z * z * z
                        alpha = alpha if alpha < 2. / 3. else F64(2. / 3.)
                        lam = lam * (F64(1. / 3.) if 1. / 3. > alpha else alpha)
                        ni = F64(2)
                        current = temp
                        S = T
                    else:
                        lam = lam * ni
                        ni = ni * 2
                    qmax += 1
                    if not (rho < 0 and qmax < MAX_TRIALS):
                        break
                self.trace.append("|")
                done += 1
                if qmax == MAX_TRIALS or rho == 0:
                    break
                if (ini - current) * 1e3 < ini:
                    nbad += 1
                else:
                    nbad = 0
                if nbad >= 3:
                    break
        return S, done

    def outliers(self):
        """The chi2 pass over the live pairs: the tested values, then the flags (a NaN is bad)."""
        a = self.alive.copy()
        with np.errstate(invalid="ignore"):
            good = (self.chi2[:, 0] <= self.th2) & (self.chi2[:, 1] <= self.th2)
        tested = self.chi2[a].copy()
        self.alive = a & good
        return int((a & ~good).sum()), int((a & good).sum()), tested


class Result:
    pass


def optimize_sim3(P, mode="numeric"):
    """Optimizer::OptimizeSim3 on one problem."""
    o = _Opt(P, mode)
    r = Result()
    S0 = P.initial()
    S, its0 = o.optimize(S0, 5)
    r.n_bad, _, r.tested1 = o.outliers()
    r.inlier1 = o.alive.copy()
    r.iterations = [its0, 0]
    r.n_in = 0
    r.tested2 = np.zeros((0, 2), F64)
    r.S = S0  # the early return leaves g2oS12 as passed in
    r.more_iterations = 10 if r.n_bad > 0 else 5
    r.early = P.n - r.n_bad < 10
    if not r.early:
        S, its1 = o.optimize(S, r.more_iterations)
        _, r.n_in, r.tested2 = o.outliers()
        r.iterations[1] = its1
        r.S = S
    r.inlier = o.alive.astype(np.uint8)
    r.chi2 = o.chi2.copy()
    r.trace = "".join(o.trace)
    r.sR, r.t = r.S.matrix()
    r.s = r.S.s
    r.sR_f, r.t_f = r.S.to_float()
    return r


def linearize(P, mode="numeric"):
    """One buildSystem pass at the initial estimate: H (7x7), b (7), the robust chi2."""
    o = _Opt(P, mode)
    with np.errstate(all="ignore"):
        return o.build(P.initial())


def transform_vector(r):
    """sR (9), t (3), s of a result: the entries the parity bars compare."""
    return np.concatenate([np.asarray(r.sR, F64).reshape(9), np.asarray(r.t, F64).reshape(3), [F64(r.s)]])


def qualifies(P):
    """The committed-problem rule: on the restatement alone, both Jacobian modes agree on the
    flags after either pass, on n_bad and n_in; every chi2 either pass compares with th2 lies at
    least 1e-3 th2 away from it in both modes; the transforms agree within 5e-5 per entry.
    Returns (ok, the numeric-versus-analytic spread of the transform)."""
    a, b = optimize_sim3(P, "numeric"), optimize_sim3(P, "analytic")
    th2 = float(P.th2)
    ok = (a.n_bad == b.n_bad and a.n_in == b.n_in and (a.inlier1 == b.inlier1).all() and (a.inlier == b.inlier).all())
    for r in (a, b):
        for t in (r.tested1, r.tested2):
            if t.size and not (np.abs(t - th2) >= 1e-3 * th2).all():
                ok = False
    spread = float(np.abs(transform_vector(a) - transform_vector(b)).max()) if P.n else 0.0
    return bool(ok and spread <= 5e-5), spread


# ---- the seeded scene -----------------------------------------------------------------------------

K1 = np.array([500.0, 510.0, 320.0, 240.0], F32)
K2 = np.array([480.0, 470.0, 310.0, 250.0], F32)


def _rodrigues(v):
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3)
    k = v / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def level_tables(nlevels=8, scale_factor=1.2):
    s = [F32(1.0)]
    for _ in range(1, nlevels):
        s.append(F32(s[-1] * F32(scale_factor)))
    s = np.array(s, F32)
    sig2 = (s * s).astype(F32)
    return s, (F32(1.0) / sig2).astype(F32)


def make_problem(seed, n, fix_scale, outlier_fraction, n_outliers=None, pixel_sigma=0.7, point_sigma=0.004,
                 perturb=1.0):
    """Two camera frames with a known Sim3 between them: n points seen by both, point noise in
    either camera frame, pixel noise scaled by the octave, a fraction (or an exact number) of the
    observations shifted by tens of pixels, varying octaves on both sides, and a perturbed initial
    estimate."""
    rng = np.random.default_rng(seed)
    s_true = 1.0 if fix_scale else float(rng.uniform(0.8, 1.3))
    R_true = _rodrigues(rng.normal(0, 0.12, 3))
    t_true = rng.normal(0, 0.25, 3)
    X2 = np.stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4.0, 10.0, n)], -1)
    X1 = s_true * X2 @ R_true.T + t_true
    scales, inv_sigma2 = level_tables()
    oct1, oct2 = rng.integers(0, 8, n), rng.integers(0, 8, n)

    def project(X, k):
        return np.stack([k[0] * X[:, 0] / X[:, 2] + k[2], k[1] * X[:, 1] / X[:, 2] + k[3]], -1)

    obs1 = project(X1, K1.astype(F64)) + rng.normal(0, pixel_sigma, (n, 2)) * scales[oct1, None]
    obs2 = project(X2, K2.astype(F64)) + rng.normal(0, pixel_sigma, (n, 2)) * scales[oct2, None]
    k = int(round(outlier_fraction * n)) if n_outliers is None else n_outliers
    bad = rng.choice(n, k, replace=False) if k else np.zeros(0, int)
    for i in bad:
        shift = rng.uniform(25.0, 60.0, 2) * rng.choice([-1.0, 1.0], 2)
        if rng.random() < 0.5:
            obs1[i] += shift
        else:
            obs2[i] += shift
    x1 = X1 + rng.normal(0, point_sigma, (n, 3))
    x2 = X2 + rng.normal(0, point_sigma, (n, 3))
    R0 = _rodrigues(rng.normal(0, 0.01 * perturb, 3)) @ R_true
    t0 = t_true + rng.normal(0, 0.03 * perturb, 3)
    s0 = 1.0 if fix_scale else s_true * (1 + float(rng.normal(0, 0.02 * perturb)))
    truth = dict(R=R_true, t=t_true, s=s_true, outliers=np.sort(bad))
    return Problem(x1, x2, obs1, obs2, inv_sigma2[oct1], inv_sigma2[oct2], K1, K2, TH2, fix_scale, R0, t0, s0, truth)


# The committed problems: (seed, n, fix_scale, outlier fraction).  Every one qualifies
# (tests/test_sim3opt_cpu.py asserts it); a seed that does not is replaced here, never skipped.
# The sizes are the kernel's edges: 0, 9 / 10 (the early return), 63 / 64 / 65 (one wavefront),
# 257 (more than one pair per lane); both scale modes; with and without outliers (10 or 5 more
# iterations).
PROBLEMS = [
    (1, 0, 0, 0.0),
    (2, 9, 0, 0.0),
    (3, 10, 1, 0.0),
    (4, 63, 0, 0.15),
    (5, 64, 1, 0.15),
    (6, 65, 0, 0.0),
    (7, 65, 1, 0.15),
    (8, 257, 0, 0.15),
    (9, 257, 1, 0.0),
    (10, 80, 0, 0.15),
    (11, 80, 1, 0.15),
    (12, 30, 1, 0.4),
]


def problem(spec):
    seed, n, fix_scale, frac = spec
    return make_problem(seed, n, fix_scale, frac)


# ---- ORBmatcher::SearchByProjection(KF, Scw, vpPoints, vpMatched, th) ---------------------------

_POPC = np.array([bin(i).count("1") for i in range(256)], np.int32)
TH_LOW = 50


def decompose_scw(Scw):
    """:368-374 in float32: scw = sqrt(row0 . row0) (the dot product in double), Rcw = sRcw / scw,
    tcw = t / scw, Ow = -Rcw^T tcw.  -> T (3x4 [Rcw | tcw]), Ow."""
    S = np.asarray(Scw, F32).reshape(-1, 4)[:3]
    r = S[0, :3].astype(F64)
    scw = F32(np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]))
    T = (S / scw).astype(F32)
    Ow = np.array([-((T[0, c] * T[0, 3] + T[1, c] * T[1, 3]) + T[2, c] * T[2, 3]) for c in range(3)], F32)
    return T, Ow


def search_by_projection_sim3(kf, Scw, mps, matched, th, trace=None):
    """src/ORBmatcher.cc:359-479, float32-exact, the loop in list order.  matched as
    orbmi_search_by_projection_sim3 takes it.  -> matched after, nmatches.  trace (a dict) receives
    per point the stage at which it was dropped."""
    from orb_slam2_with_comment_amd.types import MP_BAD
    m = np.asarray(matched, np.int32).copy()
    n = len(mps)
    v = kf.view()
    min_x, max_x, min_y, max_y = F32(v.min_x), F32(v.max_x), F32(v.min_y), F32(v.max_y)
    gwi, ghi = F32(v.grid_w_inv), F32(v.grid_h_inv)
    scale, logsf, nlev = np.asarray(kf.scale_factors, F32), F32(v.log_scale_factor), v.nlevels
    fx, fy, cx, cy = F32(v.fx), F32(v.fy), F32(v.cx), F32(v.cy)
    kx, ky, koct = kf.keys["x"].astype(F32), kf.keys["y"].astype(F32), kf.keys["octave"]
    gx = ((kx - min_x) * gwi).astype(F64)
    gy = ((ky - min_y) * ghi).astype(F64)
    px = (np.sign(gx) * np.floor(np.abs(gx) + 0.5)).astype(np.int64)  # AssignFeaturesToGrid's round
    py = (np.sign(gy) * np.floor(np.abs(gy) + 0.5)).astype(np.int64)
    in_grid = (px >= 0) & (px < 64) & (py >= 0) & (py < 48)
    cell = px * 48 + py
    T, Ow = decompose_scw(Scw)
    found = set(int(x) for x in m if x >= 0)
    th = F32(th)
    nmatches = 0
    why = {}
    for i in range(n):
        if (mps["flags"][i] & MP_BAD) or i in found:
            why[i] = "bad" if mps["flags"][i] & MP_BAD else "found"
            continue
        X = mps["pos"][i].astype(F32)
        with np.errstate(all="ignore"):
            Pc = [F32(F32(F32(F32(T[r, 0] * X[0]) + F32(T[r, 1] * X[1])) + F32(T[r, 2] * X[2])) + T[r, 3]) for r in range(3)]
            if Pc[2] < 0:
                why[i] = "behind"
                continue
            invz = F32(1.0) / Pc[2]
            u = F32(F32(fx * F32(Pc[0] * invz)) + cx)
            w = F32(F32(fy * F32(Pc[1] * invz)) + cy)
        if not (u >= min_x and u < max_x and w >= min_y and w < max_y):
            why[i] = "image"
            continue
        PO = (X - Ow).astype(F32)
        d = PO.astype(F64)
        dist = F32(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
        if dist < F32(0.8) * mps["min_distance"][i] or dist > F32(1.2) * mps["max_distance"][i]:
            why[i] = "distance"
            continue
        nrm = mps["normal"][i].astype(F64)
        if d[0] * nrm[0] + d[1] * nrm[1] + d[2] * nrm[2] < 0.5 * F64(dist):
            why[i] = "normal"
            continue
        ratio = F32(mps["max_distance"][i] / dist)
        level = int(np.ceil(F32(F32(math.log(float(ratio))) / logsf)))
        level = min(max(level, 0), nlev - 1)
        r = F32(th * scale[level])
        x0 = max(0, int(np.floor(F32(F32(F32(u - min_x) - r) * gwi))))
        x1 = min(63, int(np.ceil(F32(F32(F32(u - min_x) + r) * gwi))))
        y0 = max(0, int(np.floor(F32(F32(F32(w - min_y) - r) * ghi))))
        y1 = min(47, int(np.ceil(F32(F32(F32(w - min_y) + r) * ghi))))
        c = in_grid & (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1)
        c &= (np.abs(kx - u) < r) & (np.abs(ky - w) < r)
        c &= (m == -1) & (koct >= level - 1) & (koct <= level)  # vpMatched[idx], the octave window
        idx = np.nonzero(c)[0]
        if len(idx) == 0:
            why[i] = "no candidate"
            continue
        dd = _POPC[kf.desc[idx] ^ mps["desc"][i][None, :]].sum(1)
        best = np.lexsort((idx, cell[idx], dd))[0]  # strict <: ties to the first in grid order
        if dd[best] <= TH_LOW:
            m[idx[best]] = i
            nmatches += 1
            why[i] = "matched"
        else:
            why[i] = "distance > TH_LOW"
    if trace is not None:
        trace.update(why)
    return m, nmatches


def projection_scene(seed=0, nk=600, npts=300, s=1.3, special=True):
    """A keyframe of nk random keypoints (KITTI intrinsics, octaves 0-7, random descriptors) and
    npts world points under a Sim3 Scw of scale s, point i built to match keypoint perm[i]: on its
    ray, at the octave's predicted level, seen head-on, its descriptor a few bits away.  With
    `special`, the first points are the cases the search has to tell apart:
      0, 1   compete for one keypoint; 1 is the closer descriptor but 0 comes first
      5      already in `matched` on entry (its keypoint occupied by it)
      6      behind the camera            7   outside its distance range
      8      its normal fails the 60 degree test
      9      flagged bad                  10  projects outside the image
    and 5 % of the keypoints are occupied on entry by points that are not in the list (-2).
    -> dict(kf, Scw, mps, matched, th, perm)."""
    from orb_slam2_with_comment_amd import synth
    from orb_slam2_with_comment_amd.types import KP_DTYPE, MAPPOINT_DTYPE, MP_BAD, Frame
    rng = np.random.default_rng(seed)
    cam = synth.KITTI
    keys = np.zeros(nk, KP_DTYPE)
    keys["x"] = rng.uniform(20, cam.width - 20, nk)
    keys["y"] = rng.uniform(20, cam.height - 20, nk)
    keys["octave"] = rng.integers(0, 8, nk)
    desc = rng.integers(0, 256, (nk, 32)).astype(np.uint8)
    kf = Frame(keys, desc, np.full(nk, -1, F32), np.eye(4, dtype=F32), cam)
    R = _rodrigues(rng.normal(0, 0.05, 3))
    t = rng.normal(0, 0.5, 3)
    Scw = np.hstack([s * R, (s * t)[:, None]]).astype(F32)
    T, Ow = decompose_scw(Scw)
    Rcw, tcw = T[:, :3].astype(F64), T[:, 3].astype(F64)
    perm = rng.permutation(nk)[:npts]
    mps = np.zeros(npts, MAPPOINT_DTYPE)

    def place(i, k, z, flips):
        Xc = z * np.array([(keys["x"][k] - cam.cx) / cam.fx, (keys["y"][k] - cam.cy) / cam.fy, 1.0])
        Xw = Rcw.T @ (Xc - tcw)
        PO = Xw - Ow.astype(F64)
        dist = np.linalg.norm(PO)
        mps["pos"][i] = Xw
        mps["normal"][i] = PO / dist
        mps["max_distance"][i] = dist * 1.2 ** (int(keys["octave"][k]) - 0.5)
        mps["min_distance"][i] = mps["max_distance"][i] / 1.2 ** 7
        d = desc[k].copy()
        for b in rng.choice(256, flips, replace=False):
            d[b >> 3] ^= np.uint8(1 << (b & 7))
        mps["desc"][i] = d

    for i, k in enumerate(perm):
        place(i, k, rng.uniform(5, 40), int(rng.integers(0, 12)))
    matched = np.full(nk, -1, np.int32)
    if special and npts > 10:
        place(0, perm[0], 12.0, 6)
        place(1, perm[0], 12.0, 0)
        matched[perm[5]] = 5
        mps["pos"][6] = Rcw.T @ (np.array([0.0, 0.0, -5.0]) - tcw)
        mps["max_distance"][7] = 0.5 * np.linalg.norm(mps["pos"][7].astype(F64) - Ow.astype(F64))
        mps["normal"][8] = -mps["normal"][8]
        mps["flags"][9] |= MP_BAD
        mps["pos"][10] = Rcw.T @ (np.array([1000.0, 0.0, 5.0]) - tcw)
        occupied = rng.permutation(nk)[:nk // 20]
        matched[occupied[matched[occupied] == -1]] = -2
    return {"kf": kf, "Scw": Scw, "mps": mps, "matched": matched, "th": 10, "perm": perm}


def projection_overflow_scene(seed=0, nk=130, npts=110):
    """More candidates per point than the device keeps (Matcher::kCandCap = 96): nk keypoints of
    octave 0 within two pixels of one another, all with one descriptor, and npts points of that
    descriptor projecting among them.  Every point takes the first free keypoint in grid order."""
    sc = projection_scene(seed, nk, npts, 1.0, special=False)
    kf, mps = sc["kf"], sc["mps"]
    rng = np.random.default_rng(seed + 1)
    kf.keys["x"] = 600.0 + rng.uniform(-1, 1, nk)
    kf.keys["y"] = 180.0 + rng.uniform(-1, 1, nk)
    kf.keys["octave"] = 0
    kf.desc[:] = kf.desc[0]
    mps[:] = mps[0]
    T, Ow = decompose_scw(sc["Scw"])
    Xc = 10.0 * np.array([(600.0 - kf.cam.cx) / kf.cam.fx, (180.0 - kf.cam.cy) / kf.cam.fy, 1.0])
    Xw = T[:, :3].astype(F64).T @ (Xc - T[:, 3].astype(F64))
    PO = Xw - Ow.astype(F64)
    mps["pos"] = Xw
    mps["normal"] = PO / np.linalg.norm(PO)
    mps["max_distance"] = np.linalg.norm(PO) * 1.2 ** -0.5
    mps["min_distance"] = mps["max_distance"] / 1.2 ** 7
    mps["desc"] = kf.desc[0]
    return sc
