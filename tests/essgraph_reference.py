"""Numpy restatement of csrc/essgraph.h and csrc/essgraph_edges.h (Optimizer::OptimizeEssentialGraph,
src/Optimizer.cc:829-1118, and the two arithmetic loops of LoopClosing::CorrectLoop, with the bundled
g2o's semantics), operation for operation: Sim3::log, EdgeSim3::computeError, BaseBinaryEdge's
numeric linearizeOplus and constructQuadraticForm, OptimizationAlgorithmLevenberg::solve with the
user lambda 1e-16, the edge rule and the point / pose correction.

Everything is vectorised over the edges: numpy's elementwise +, -, *, /, sqrt round once per
operation like the scalar code; branches are both computed and selected.  sin, cos, acos, log and
exp come from `math`, so they are glibc's.  The sums over the edges are sequential, in edge order.
The damped solve is DENSE (Cholesky of H + lambda I): the restatement states the reference's
formulation, the sparse order is the library's own business.

A Sim3 is 8 doubles: q (x y z w), t, s.  Also the drifted-ring problems the tests share."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
DELTA = 1e-9
MAX_TRIALS = 10
TERMINATE, SOLVE_FAILED, REJECTED = 1, 2, 4


def _m(fn, a):
    out = np.empty(len(a), F64)
    for i, v in enumerate(a):
        try:
            out[i] = fn(float(v))
        except (ValueError, OverflowError):
            out[i] = math.nan
    return out


# ---- batched quaternions and Sim3 (types/sim3.h); S = (n, 8) ------------------------------------------

def quat_to_R(q):
    """Eigen toRotationMatrix: 9 arrays, row-major."""
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)]


def quat_from_R(m):
    """Eigen::Quaternion(const Matrix3&), m = 9 arrays; (n, 4), not normalised."""
    with np.errstate(all="ignore"):
        tr = (m[0] + m[4]) + m[8]
        t = np.sqrt(tr + 1.0)
        w0 = 0.5 * t
        t = 0.5 / t
        b0 = [(m[7] - m[5]) * t, (m[2] - m[6]) * t, (m[3] - m[1]) * t, w0]
        t = np.sqrt(((m[0] - m[4]) - m[8]) + 1.0)
        x = 0.5 * t
        t = 0.5 / t
        b1 = [x, (m[3] + m[1]) * t, (m[6] + m[2]) * t, (m[7] - m[5]) * t]
        t = np.sqrt(((m[4] - m[8]) - m[0]) + 1.0)
        y = 0.5 * t
        t = 0.5 / t
        b2 = [(m[1] + m[3]) * t, y, (m[7] + m[5]) * t, (m[2] - m[6]) * t]
        t = np.sqrt(((m[8] - m[0]) - m[4]) + 1.0)
        z = 0.5 * t
        t = 0.5 / t
        b3 = [(m[2] + m[6]) * t, (m[5] + m[7]) * t, z, (m[3] - m[1]) * t]
    i = np.where(m[4] > m[0], 1, 0)
    i = np.where(m[8] > np.where(i == 1, m[4], m[0]), 2, i)
    pos = tr > 0
    out = [np.where(pos, b0[k], np.where(i == 0, b1[k], np.where(i == 1, b2[k], b3[k]))) for k in range(4)]
    return np.stack(out, -1)


def quat_mul(a, b):
    x = ((a[:, 3] * b[:, 0] + a[:, 0] * b[:, 3]) + a[:, 1] * b[:, 2]) - a[:, 2] * b[:, 1]
    y = ((a[:, 3] * b[:, 1] + a[:, 1] * b[:, 3]) + a[:, 2] * b[:, 0]) - a[:, 0] * b[:, 2]
    z = ((a[:, 3] * b[:, 2] + a[:, 2] * b[:, 3]) + a[:, 0] * b[:, 1]) - a[:, 1] * b[:, 0]
    w = ((a[:, 3] * b[:, 3] - a[:, 0] * b[:, 0]) - a[:, 1] * b[:, 1]) - a[:, 2] * b[:, 2]
    return np.stack([x, y, z, w], -1)


def rotate(q, v):
    """Eigen's quaternion * vector."""
    v0, v1, v2 = v[:, 0], v[:, 1], v[:, 2]
    ux = q[:, 1] * v2 - q[:, 2] * v1
    uy = q[:, 2] * v0 - q[:, 0] * v2
    uz = q[:, 0] * v1 - q[:, 1] * v0
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    cx = q[:, 1] * uz - q[:, 2] * uy
    cy = q[:, 2] * ux - q[:, 0] * uz
    cz = q[:, 0] * uy - q[:, 1] * ux
    return np.stack([(v0 + q[:, 3] * ux) + cx, (v1 + q[:, 3] * uy) + cy, (v2 + q[:, 3] * uz) + cz], -1)


def s_map(S, x):
    return S[:, 7:8] * rotate(S[:, :4], x) + S[:, 4:7]


def s_mul(a, b):
    return np.concatenate([quat_mul(a[:, :4], b[:, :4]), a[:, 7:8] * rotate(a[:, :4], b[:, 4:7]) + a[:, 4:7],
                           (a[:, 7] * b[:, 7])[:, None]], -1)


def s_inverse(a):
    qc = a[:, :4] * np.array([-1.0, -1.0, -1.0, 1.0])
    m = F64(-1.) / a[:, 7]
    return np.concatenate([qc, rotate(qc, m[:, None] * a[:, 4:7]), (F64(1.) / a[:, 7])[:, None]], -1)


def _abc(small, sigma, s, theta, sn, cs):
    """A, B, C of Sim3(Vector7d) and of Sim3::log: the four branches."""
    eps = 0.00001
    with np.errstate(all="ignore"):
        theta2 = theta * theta
        sigma2 = sigma * sigma
        A00 = (1 - cs) / theta2
        B00 = (theta - sn) / (theta2 * theta)
        C1 = (s - 1) / sigma
        A10 = ((sigma - 1) * s + 1) / sigma2
        B10 = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
        a, b = s * sn, s * cs
        c = theta2 + sigma2
        A11 = (a * sigma + (1 - b) * theta) / (theta * c)
        B11 = (C1 - ((b - 1) * sigma + a * theta) / c) * 1. / theta2
    ss = np.abs(sigma) < eps
    A = np.where(ss, np.where(small, 1. / 2., A00), np.where(small, A10, A11))
    B = np.where(ss, np.where(small, 1. / 6., B00), np.where(small, B10, B11))
    C = np.where(ss, 1.0, C1)
    return A, B, C


def _skew_sq(Om):
    return [(Om[3 * r] * Om[c] + Om[3 * r + 1] * Om[3 + c]) + Om[3 * r + 2] * Om[6 + c] for r in range(3) for c in range(3)]


def s_exp(u):
    """Sim3(const Vector7d&), types/sim3.h:70-142; u (n, 7)."""
    w0, w1, w2, sigma = u[:, 0], u[:, 1], u[:, 2], u[:, 6]
    theta = np.sqrt((w0 * w0 + w1 * w1) + w2 * w2)
    z = np.zeros_like(w0)
    Om = [z, -w2, w1, w2, z, -w0, -w1, w0, z]
    Om2 = _skew_sq(Om)
    s = _m(math.exp, sigma)
    small = theta < 0.00001
    th = np.where(small, 0.0, theta)
    sn, cs = _m(math.sin, th), _m(math.cos, th)
    with np.errstate(all="ignore"):
        ra = sn / theta
        rb = (1 - cs) / (theta * theta)
    A, B, C = _abc(small, sigma, s, theta, sn, cs)
    R, W = [], []
    for k in range(9):
        I = 1.0 if k in (0, 4, 8) else 0.0
        with np.errstate(all="ignore"):
            R.append(np.where(small, (I + Om[k]) + Om2[k], (I + ra * Om[k]) + rb * Om2[k]))
        W.append((A * Om[k] + B * Om2[k]) + C * I)
    t = [(W[3 * r] * u[:, 3] + W[3 * r + 1] * u[:, 4]) + W[3 * r + 2] * u[:, 5] for r in range(3)]
    return np.concatenate([quat_from_R(R), np.stack(t, -1), s[:, None]], -1)


def s_log(S):
    """Sim3::log, types/sim3.h:148-230, with the 3x3 partial-pivot LU of csrc/essgraph.h."""
    s = S[:, 7]
    sigma = _m(math.log, s)
    R = quat_to_R(S[:, :4])
    d = 0.5 * (((R[0] + R[4]) + R[8]) - 1)
    dR = [R[7] - R[5], R[2] - R[6], R[3] - R[1]]
    small = d > 1 - 0.00001
    theta = _m(math.acos, np.where(small, 1.0, d))
    with np.errstate(all="ignore"):
        f = np.where(small, 0.5, theta / (2 * np.sqrt(1 - d * d)))
    theta = np.where(small, 0.0, theta)
    sn, cs = _m(math.sin, theta), _m(math.cos, theta)
    w0, w1, w2 = f * dR[0], f * dR[1], f * dR[2]
    A, B, C = _abc(small, sigma, s, theta, sn, cs)
    z = np.zeros_like(w0)
    Om = [z, -w2, w1, w2, z, -w0, -w1, w0, z]
    Om2 = _skew_sq(Om)
    W = [[(A * Om[3 * r + c] + B * Om2[3 * r + c]) + C * (1.0 if r == c else 0.0) for c in range(3)] for r in range(3)]
    t = [S[:, 4].copy(), S[:, 5].copy(), S[:, 6].copy()]
    with np.errstate(all="ignore"):
        for k in range(2):
            for r in range(k + 1, 3):
                sw = np.abs(W[r][k]) > np.abs(W[k][k])
                for c in range(3):
                    a, b = W[k][c], W[r][c]
                    W[k][c], W[r][c] = np.where(sw, b, a), np.where(sw, a, b)
                a, b = t[k], t[r]
                t[k], t[r] = np.where(sw, b, a), np.where(sw, a, b)
            for r in range(k + 1, 3):
                m = W[r][k] / W[k][k]
                for c in range(k + 1, 3):
                    W[r][c] = W[r][c] - m * W[k][c]
                t[r] = t[r] - m * t[k]
        u2 = t[2] / W[2][2]
        u1 = (t[1] - W[1][2] * u2) / W[1][1]
        u0 = ((t[0] - W[0][1] * u1) - W[0][2] * u2) / W[0][0]
    return np.stack([w0, w1, w2, u0, u1, u2, sigma], -1)


def oplus(S, x, fix_scale):
    """VertexSim3Expmap::oplusImpl."""
    u = np.array(x, F64)
    if fix_scale:
        u[:, 6] = 0
    return s_mul(s_exp(u), S)


def edge_error(C, S0, S1):
    """EdgeSim3::computeError: log(C * S_v0 * S_v1^-1)."""
    return s_log(s_mul(s_mul(C, S0), s_inverse(S1)))


def chi2_of(e):
    c = np.zeros(len(e), F64)
    for k in range(7):
        c = c + e[:, k] * e[:, k]
    return c


def seq_sum(a):
    t = F64(0)
    for v in a:
        t = t + v
    return t


def from_rts(R, t, s=1.0):
    """g2o::Sim3(Matrix3d, Vector3d, double) from floats; R (n, 3, 3), t (n, 3)."""
    R = np.asarray(R, F32).astype(F64).reshape(-1, 9)
    t = np.asarray(t, F32).astype(F64).reshape(-1, 3)
    return np.concatenate([quat_from_R([R[:, k] for k in range(9)]), t, np.full((len(t), 1), F64(F32(s)))], -1)


def sim3_to_tcw(S):
    """[R | t * (1. / s)] as float 4x4 (src/LoopClosing.cc:620-628)."""
    S = np.asarray(S, F64).reshape(-1, 8)
    R = quat_to_R(S[:, :4])
    inv = F64(1.) / S[:, 7]
    T = np.zeros((len(S), 4, 4), F32)
    for r in range(3):
        for c in range(3):
            T[:, r, c] = R[3 * r + c].astype(F32)
        T[:, r, 3] = (S[:, 4 + r] * inv).astype(F32)
    T[:, 3, 3] = 1
    return T


def correct_points(P, ref_index, Srw, Swr_corrected):
    """correctedSwr.map(Srw.map((double)P)) rounded to float; ref_index (n) picks the pair of Sim3."""
    P = np.asarray(P, F32).reshape(-1, 3)
    if len(P) == 0:
        return P.copy()
    ref_index = np.asarray(ref_index)
    y = s_map(np.asarray(Srw, F64).reshape(-1, 8)[ref_index], P.astype(F64))
    return s_map(np.asarray(Swr_corrected, F64).reshape(-1, 8)[ref_index], y).astype(F32)


# ---- linearisation and the Levenberg loop ----------------------------------------------------------

class Linearisation:
    __slots__ = ("e", "chi2", "J0", "J1", "H00", "H01", "H11", "b0", "b1")


def linearize_edges(est, v0, v1, C, fix_scale, delta=DELTA):
    """Per edge: e (E, 7), chi2, J0 / J1 (E, 7, 7), the three products and -J^T e."""
    S0, S1 = est[v0], est[v1]
    L = Linearisation()
    L.e = edge_error(C, S0, S1)
    L.chi2 = chi2_of(L.e)
    scalar = F64(1.0) / (2 * F64(delta))
    J = [np.zeros((len(v0), 7, 7), F64), np.zeros((len(v0), 7, 7), F64)]
    for v in range(2):
        for d in range(7):
            u = np.zeros((len(v0), 7), F64)
            u[:, d] = delta
            T = oplus(S1 if v else S0, u, fix_scale)
            ep = edge_error(C, S0 if v else T, T if v else S1)
            u[:, d] = -delta
            T = oplus(S1 if v else S0, u, fix_scale)
            em = edge_error(C, S0 if v else T, T if v else S1)
            J[v][:, :, d] = scalar * (ep - em)
    L.J0, L.J1 = J

    def prod(A, B):
        s = np.zeros((len(v0), 7, 7), F64)
        for k in range(7):
            s = s + A[:, k, :, None] * B[:, k, None, :]
        return s

    def rhs(A):
        s = np.zeros((len(v0), 7), F64)
        for k in range(7):
            s = s + A[:, k, :] * (-L.e[:, k, None])
        return s
    L.H00, L.H01, L.H11 = prod(J[0], J[0]), prod(J[0], J[1]), prod(J[1], J[1])
    L.b0, L.b1 = rhs(J[0]), rhs(J[1])
    return L


def free_vertices(nv, fixed, v0, v1):
    """Ascending vertex index: not fixed, and named by an edge."""
    used = np.zeros(nv, bool)
    used[v0] = True
    used[v1] = True
    used[fixed] = False
    return np.nonzero(used)[0]


def assemble(L, nv, fixed, v0, v1):
    """Dense H, b over the free vertices (ascending index), the edges added in edge order."""
    free = free_vertices(nv, fixed, v0, v1)
    pos = np.full(nv, -1)
    pos[free] = np.arange(len(free))
    n = 7 * len(free)
    H, b = np.zeros((n, n), F64), np.zeros(n, F64)
    for e in range(len(v0)):
        a, c = pos[v0[e]], pos[v1[e]]
        if a >= 0:
            H[7 * a:7 * a + 7, 7 * a:7 * a + 7] += L.H00[e]
            b[7 * a:7 * a + 7] += L.b0[e]
        if c >= 0:
            H[7 * c:7 * c + 7, 7 * c:7 * c + 7] += L.H11[e]
            b[7 * c:7 * c + 7] += L.b1[e]
        if a >= 0 and c >= 0:
            H[7 * a:7 * a + 7, 7 * c:7 * c + 7] += L.H01[e]
            H[7 * c:7 * c + 7, 7 * a:7 * a + 7] += L.H01[e].T
    return free, H, b


class Result:
    __slots__ = ("est", "chi2_before", "chi2_after", "iterations", "trials", "status")


def optimize(vertices, fixed, v0, v1, meas, fix_scale, iterations=20, delta=DELTA):
    """OptimizeEssentialGraph's optimize(20) over arrays: vertices (nv, 8), edges (v0, v1, meas)."""
    est = np.array(vertices, F64).reshape(-1, 8)
    v0, v1 = np.asarray(v0, np.int64).reshape(-1), np.asarray(v1, np.int64).reshape(-1)
    C = np.asarray(meas, F64).reshape(-1, 8)
    nv = len(est)
    R = Result()
    R.est, R.chi2_before, R.chi2_after, R.iterations, R.trials, R.status = est, 0.0, 0.0, 0, [], 0
    free = free_vertices(nv, fixed, v0, v1) if len(v0) else np.zeros(0, np.int64)
    if len(free) == 0 or iterations <= 0:
        R.status = TERMINATE
        return R
    lam = ni = F64(0)
    nbad = 0
    cur = F64(0)
    stopped = False
    for it in range(iterations):
        L = linearize_edges(est, v0, v1, C, fix_scale, delta)
        _, H, b = assemble(L, nv, fixed, v0, v1)
        cur = seq_sum(L.chi2)
        ini = cur
        if it == 0:
            R.chi2_before = float(cur)
            lam, ni, nbad = F64(1e-16), F64(2), 0
        rho, qmax = F64(0), 0
        while True:
            ok2 = True
            try:
                with np.errstate(all="ignore"):
                    if not np.isfinite(H).all():
                        raise np.linalg.LinAlgError
                    Lc = np.linalg.cholesky(H + lam * np.eye(len(b)))
                    x = np.linalg.solve(Lc.T, np.linalg.solve(Lc, b))
                    if not np.isfinite(x).all():
                        raise np.linalg.LinAlgError
            except np.linalg.LinAlgError:
                ok2 = False
                x = np.zeros_like(b)
                R.status |= SOLVE_FAILED
            temp, scale = F64(1.7976931348623157e308), F64(0)
            trial = est
            if ok2:
                trial = est.copy()
                trial[free] = oplus(est[free], x.reshape(-1, 7), fix_scale)
                with np.errstate(all="ignore"):
                    temp = seq_sum(chi2_of(edge_error(C, trial[v0], trial[v1])))
                    scale = seq_sum(x * (lam * x + b))
            with np.errstate(all="ignore"):
                rho = (cur - temp) / (scale + 1e-3)
            if rho > 0 and np.isfinite(temp):
                z = 2 * rho - 1
                alpha = min(1. - z * z * z, 2. / 3.)
                lam = lam * max(1. / 3., alpha)
                ni = F64(2)
                cur = temp
                est = trial
            else:
                lam = lam * ni
                ni = ni * 2
                R.status |= REJECTED
            qmax += 1
            if not (rho < 0 and qmax < MAX_TRIALS):
                break
        R.trials.append(qmax)
        R.iterations += 1
        if qmax == MAX_TRIALS or rho == 0:
            stopped = True
            break
        nbad = nbad + 1 if (ini - cur) * 1e3 < ini else 0
        if nbad >= 3:
            stopped = True
            break
    if stopped:
        R.status |= TERMINATE
    R.est, R.chi2_after = est, float(cur)
    return R


def pose_deviation(a, b, extent):
    """max over q (up to sign), s, and t relative to the graph's extent."""
    a, b = np.asarray(a, F64).reshape(-1, 8), np.asarray(b, F64).reshape(-1, 8)
    sign = np.where((a[:, :4] * b[:, :4]).sum(-1) < 0, -1.0, 1.0)[:, None]
    dq = np.abs(a[:, :4] - sign * b[:, :4]).max()
    return float(max(dq, np.abs(a[:, 7] - b[:, 7]).max(), np.abs(a[:, 4:7] - b[:, 4:7]).max() / extent))


# ---- the edge rule (src/Optimizer.cc:862-1053) over a graph dict ------------------------------------
# graph: live (n_ids) bool, Tcw (n_ids, 4, 4) float32, parent (n_ids), loop_edges {id: [ids]},
# covisibles {id: [ids]} (GetCovisiblesByWeight(100), in its order), corrected / noncorrected
# {id: Sim3 (8)}, loop_connections {id: {id: weight}}, loop_id, cur_id

def _one(S):
    return np.asarray(S, F64).reshape(1, 8)


def essential_graph_edges(G):
    """-> v0, v1 (keyframe ids), measurements (E, 8), vScw (n_ids, 8); ascending keyframe id
    wherever the reference iterates in pointer order."""
    n = len(G["live"])
    live = np.asarray(G["live"], bool)
    Tcw = np.asarray(G["Tcw"], F32).reshape(n, 4, 4)
    vScw = np.zeros((n, 8), F64)
    vScw[:, 3] = 1
    vScw[:, 7] = 1
    ids = np.nonzero(live)[0]
    vScw[ids] = from_rts(Tcw[ids, :3, :3], Tcw[ids, :3, 3], 1.0)
    for i, S in G["corrected"].items():
        vScw[i] = np.asarray(S, F64)
    v0, v1, meas = [], [], []

    def push(i, j, Sjw, Swi):
        v0.append(i)
        v1.append(j)
        meas.append(s_mul(_one(Sjw), Swi)[0])
    inserted = set()
    for i in sorted(G["loop_connections"]):
        Swi = s_inverse(_one(vScw[i]))
        row = G["loop_connections"][i]
        for j in sorted(row):
            if (i != G["cur_id"] or j != G["loop_id"]) and row[j] < 100:
                continue
            push(i, j, vScw[j], Swi)
            inserted.add((min(i, j), max(i, j)))
    nonc = G["noncorrected"]

    def Sw_of(j):
        return nonc[j] if j in nonc else vScw[j]
    parent = np.asarray(G["parent"])
    for i in ids:
        i = int(i)
        Swi = s_inverse(_one(Sw_of(i)))
        p = int(parent[i])
        if p >= 0:
            push(i, p, Sw_of(p), Swi)
        loops = sorted(set(G["loop_edges"].get(i, ())))
        for l in loops:
            if l < i:
                push(i, l, Sw_of(l), Swi)
        for j in G["covisibles"].get(i, ()):
            if j == p or parent[j] == i or j in loops:
                continue
            if not j < i or (j, i) in inserted:
                continue
            push(i, j, Sw_of(j), Swi)
    return (np.array(v0, np.int32), np.array(v1, np.int32), np.array(meas, F64).reshape(-1, 8), vScw)


class Backend:
    """The restatement as the backend object of loop.essential_graph_edges / optimize_essential_graph."""

    def essential_graph_edges(self, G):
        return essential_graph_edges(G)

    def optimize_essential_graph(self, vertices, fixed, v0, v1, meas, fix_scale, iterations=20):
        r = optimize(vertices, fixed, v0, v1, meas, fix_scale, iterations)
        return {"vertices": r.est, "chi2_before": r.chi2_before, "chi2_after": r.chi2_after, "iterations": r.iterations,
                "trials": list(r.trials), "status": r.status}

    def correct_points_sim3(self, points, ref_index, Srw, Swr_corrected, poses):
        return correct_points(points, ref_index, Srw, Swr_corrected), sim3_to_tcw(poses)


# ---- the committed problems: drifted rings closed onto keyframe 0 ------------------------------------

def _rot(axis, a):
    axis = np.asarray(axis, F64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)


def ring_graph(seed, N, shape="ring", radius=10.0, rot_noise=0.004, t_noise=0.02, scale_drift=0.0):
    """A graph dict: N keyframes on a circle (shape "ring": parent i - 1, covisible i - 2, the loop
    N - 1 -> 0; "chain": parents and the loop only), their poses drifted step by step, the last three
    corrected by propagation from the loop measurement."""
    rng = np.random.default_rng(seed)
    Ttrue = []
    for i in range(N):
        a = 2 * math.pi * i / N
        Rwc = _rot([0, 0, 1], a + math.pi / 2)
        twc = np.array([radius * math.cos(a), radius * math.sin(a), 0.3 * math.sin(3 * a)])
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = Rwc.T, -Rwc.T @ twc
        Ttrue.append(T)
    Tdrift = [Ttrue[0]]
    for i in range(1, N):
        rel = Ttrue[i] @ np.linalg.inv(Ttrue[i - 1])
        noise = np.eye(4)
        noise[:3, :3] = _rot(rng.normal(0, 1, 3), rng.normal(0, rot_noise))
        noise[:3, 3] = rng.normal(0, t_noise, 3)
        Tdrift.append(noise @ rel @ Tdrift[i - 1])
    Tcw = np.array(Tdrift).astype(F32)
    cur, loop = N - 1, 0
    # the accepted Scw of the current keyframe: the loop keyframe's pose and the true relative motion
    Tcl = Ttrue[cur] @ np.linalg.inv(Ttrue[loop])
    s = math.exp(scale_drift)
    Scl = from_rts(Tcl[None, :3, :3], Tcl[None, :3, 3], 1.0)
    Scl[0, 7] = s
    Scw = s_mul(Scl, from_rts(Tcw[loop:loop + 1, :3, :3], Tcw[loop:loop + 1, :3, 3], 1.0))[0]
    connected = [k for k in (N - 3, N - 2) if 0 < k < cur]
    corrected, nonc = propagate(Tcw, cur, connected, Scw)
    G = {"live": np.ones(N, bool), "Tcw": Tcw, "parent": np.arange(-1, N - 1, dtype=np.int32), "loop_edges": {},
         "covisibles": {}, "corrected": corrected, "noncorrected": nonc, "loop_connections": {cur: {loop: 40}},
         "loop_id": loop, "cur_id": cur}
    if shape == "ring":
        for i in range(N):
            G["covisibles"][i] = [j for j in (i - 1, i + 1, i - 2, i + 2) if 0 <= j < N]
    return G


def propagate(Tcw, cur, connected, Scw):
    """LoopClosing.cc:546-581 over float poses (loop.propagate_corrected_sim3 restates it the same way)."""
    Tcw = np.asarray(Tcw, F32)
    Twc = np.eye(4, dtype=F32)
    Rwc = Tcw[cur, :3, :3].T
    Twc[:3, :3] = Rwc
    t = Tcw[cur, :3, 3]
    for r in range(3):
        Twc[r, 3] = -((Rwc[r, 0] * t[0] + Rwc[r, 1] * t[1]) + Rwc[r, 2] * t[2])
    corrected, nonc = {cur: np.asarray(Scw, F64)}, {}
    for i in list(connected) + [cur]:
        Tiw = Tcw[i]
        if i != cur:
            A, B = Tiw.astype(F64), Twc.astype(F64)
            Tic = np.zeros((4, 4), F64)
            for r in range(4):
                for c in range(4):
                    Tic[r, c] = ((A[r, 0] * B[0, c] + A[r, 1] * B[1, c]) + A[r, 2] * B[2, c]) + A[r, 3] * B[3, c]
            Tic = Tic.astype(F32)
            Sic = from_rts(Tic[None, :3, :3], Tic[None, :3, 3], 1.0)
            corrected[i] = s_mul(Sic, _one(Scw))[0]
        nonc[i] = from_rts(Tiw[None, :3, :3], Tiw[None, :3, 3], 1.0)[0]
    return corrected, nonc


class Problem:
    """vertices (nv, 8), fixed, v0 / v1 (vertex indices), meas (E, 8), fix_scale, extent."""


def problem_from_graph(G, fix_scale):
    v0, v1, meas, vScw = essential_graph_edges(G)
    ids = np.nonzero(np.asarray(G["live"], bool))[0]
    index = np.full(len(G["live"]), -1, np.int32)
    index[ids] = np.arange(len(ids))
    P = Problem()
    P.vertices, P.fixed = vScw[ids], int(index[G["loop_id"]])
    P.v0, P.v1, P.meas, P.fix_scale = index[v0], index[v1], meas, int(fix_scale)
    centres = -rotate(P.vertices[:, :4] * np.array([-1.0, -1.0, -1.0, 1.0]), P.vertices[:, 4:7])
    P.extent = float(np.abs(centres - centres.mean(0)).max())
    return P


# (seed, N, fix_scale, shape)
PROBLEMS = ((1, 24, 1, "ring"), (2, 24, 0, "ring"), (3, 66, 1, "ring"), (4, 257, 1, "chain"))

_cache = {}


def problem(spec):
    if spec not in _cache:
        seed, N, fix_scale, shape = spec
        _cache[spec] = problem_from_graph(ring_graph(seed, N, shape, scale_drift=0.0 if fix_scale else 0.02), fix_scale)
    return _cache[spec]


def solved(spec, delta=DELTA):
    key = ("solved", spec, delta)
    if key not in _cache:
        P = problem(spec)
        _cache[key] = optimize(P.vertices, P.fixed, P.v0, P.v1, P.meas, P.fix_scale, 20, delta)
    return _cache[key]


def qualifies(spec):
    """The restatement ends by a rule of Levenberg's or the 20th iteration, and its results with
    delta = 1e-9 and 1e-8 agree within 1e-5 (a tenth of the pose bar)."""
    P, a, b = problem(spec), solved(spec), solved(spec, 1e-8)
    spread = pose_deviation(a.est, b.est, P.extent)
    ended = bool(a.status & TERMINATE) or a.iterations == 20
    return ended and np.isfinite(a.est).all() and spread <= 1e-5, spread


def linearisation(spec, delta=DELTA):
    """H blocks per free vertex pair as dense H, b and chi2 at the initial estimates."""
    key = ("lin", spec, delta)
    if key not in _cache:
        P = problem(spec)
        L = linearize_edges(P.vertices, P.v0, P.v1, P.meas, P.fix_scale, delta)
        free, H, b = assemble(L, len(P.vertices), P.fixed, P.v0, P.v1)
        _cache[key] = (L, free, H, b, float(seq_sum(L.chi2)))
    return _cache[key]


def synthetic_problem(seed, nv, pairs, fix_scale, fixed, meas_noise=0.0, start_noise=0.02):
    """Random poses a few metres apart, one edge per (v0, v1) of `pairs` measuring S_v1 * S_v0^-1 of
    the true poses (times exp of meas_noise), the estimates starting start_noise away from them."""
    rng = np.random.default_rng(seed)
    u = rng.normal(0, 0.5, (nv, 7))
    u[:, 3:6] = rng.normal(0, 4.0, (nv, 3))
    u[:, 6] = 0 if fix_scale else rng.normal(0, 0.05, nv)
    truth = s_exp(u)
    P = Problem()
    P.truth = truth
    d = rng.normal(0, start_noise, (nv, 7))
    if fix_scale:
        d[:, 6] = 0
    d[fixed] = 0
    P.vertices = s_mul(s_exp(d), truth) if start_noise else truth.copy()
    P.fixed, P.fix_scale = int(fixed), int(fix_scale)
    P.v0 = np.array([p[0] for p in pairs], np.int32)
    P.v1 = np.array([p[1] for p in pairs], np.int32)
    P.meas = s_mul(truth[P.v1], s_inverse(truth[P.v0])) if len(pairs) else np.zeros((0, 8))
    if meas_noise and len(pairs):
        n = rng.normal(0, meas_noise, (len(pairs), 7))
        if fix_scale:
            n[:, 6] = 0
        P.meas = s_mul(s_exp(n), P.meas)
    P.extent = float(np.abs(truth[:, 4:7]).max())
    return P
