"""Numpy restatement of csrc/sim3_horn.h (ORB_SLAM2::Sim3Solver, src/Sim3Solver.cc), operation
for operation: the fp64 Horn step with the same cyclic Jacobi, the float32 projection and inlier
test, the thresholds, the iteration rule, the counter-based sampler and the iterate replay.  It is
the checker of the host header (tests/cpp/sim3_check.cpp), of the device kernel and of
orb_slam2_with_comment_amd.sim3; an independent eigh-based Horn step checks the restatement itself.
Also the seeded Sim3 scene the tests share.

Every function is vectorised over the hypotheses: numpy's elementwise +, -, *, /, sqrt round once
per operation like the scalar code, and nothing here is fused."""
import functools
import math

import numpy as np

F32, F64 = np.float32, np.float64
SWEEPS = 8  # kSim3Sweeps
_M64 = (1 << 64) - 1


# ---- thresholds, iteration rule, sampler -----------------------------------------------------

def level_sigma2(nlevels=8, scale_factor=1.2):
    """mvLevelSigma2 as ORBextractor builds it (src/ORBextractor.cc:422-430), float32."""
    s = [F32(1.0)]
    for _ in range(1, nlevels):
        s.append(F32(s[-1] * F32(scale_factor)))
    return np.array([F32(x * x) for x in s], F32)


def max_error(sigma2):
    """(size_t)(9.210 * sigmaSquare), src/Sim3Solver.cc:87-88 with include/Sim3Solver.h:79-80."""
    return np.trunc(9.210 * np.asarray(sigma2, F32).astype(F64)).astype(np.int32)


def iterations(n, min_inliers, probability=0.99, max_its=300):
    """SetRansacParameters (:114-138); 0 when n < min_inliers (iterate returns at once)."""
    if n < min_inliers:
        return 0
    v = 1.0
    if min_inliers != n:
        eps = float(F32(min_inliers) / F32(n))
        den = math.log(1 - math.pow(eps, 3.0))
        num = math.log(1 - probability)
        v = math.ceil(num / den) if den != 0 else -math.inf
    if v >= max_its:
        return max(max_its, 1)
    return int(v) if v >= 1 else 1


def _mix(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def draw(seed, solver, it, d):
    return _mix((seed & _M64) ^ _mix(((solver & 0xFFFFFFFF) << 40) ^ ((it & 0xFFFFFFFF) << 2) ^ d))


def sample_triples(seed, solver, n, its):
    """:167-185: draw from the available indices, swap with the back, pop; three times."""
    out = np.zeros((its, 3), np.int32)
    for it in range(its):
        avail = list(range(n))
        for d in range(3):
            r = draw(seed, solver, it, d) % len(avail)
            out[it, d] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


# ---- ComputeSim3 -----------------------------------------------------------------------------

def horn(P1, P2, fix_scale):
    """sim3_horn over H triples: P1, P2 (H, 3 points, 3) float32 -> T12, T21 (H, 12) float32, s (H,)."""
    P1 = np.asarray(P1, F32).astype(F64)
    P2 = np.asarray(P2, F32).astype(F64)
    with np.errstate(all="ignore"):
        O1 = ((P1[:, 0] + P1[:, 1]) + P1[:, 2]) / 3.0
        O2 = ((P2[:, 0] + P2[:, 1]) + P2[:, 2]) / 3.0
        Pr1 = P1 - O1[:, None, :]
        Pr2 = P2 - O2[:, None, :]
        M = [[(Pr2[:, 0, r] * Pr1[:, 0, c] + Pr2[:, 1, r] * Pr1[:, 1, c]) + Pr2[:, 2, r] * Pr1[:, 2, c]
              for c in range(3)] for r in range(3)]
        A = [[None] * 4 for _ in range(4)]
        A[0][0] = (M[0][0] + M[1][1]) + M[2][2]
        A[0][1] = M[1][2] - M[2][1]
        A[0][2] = M[2][0] - M[0][2]
        A[0][3] = M[0][1] - M[1][0]
        A[1][1] = (M[0][0] - M[1][1]) - M[2][2]
        A[1][2] = M[0][1] + M[1][0]
        A[1][3] = M[2][0] + M[0][2]
        A[2][2] = (-M[0][0] + M[1][1]) - M[2][2]
        A[2][3] = M[1][2] + M[2][1]
        A[3][3] = (-M[0][0] - M[1][1]) + M[2][2]
        H = len(P1)
        V = [[np.full(H, 1.0 if p == q else 0.0) for q in range(4)] for p in range(4)]
        for p in range(4):
            for q in range(p):
                A[p][q] = A[q][p]
        for _ in range(SWEEPS):
            for p in range(4):
                for q in range(p + 1, 4):
                    rot = A[p][q] != 0
                    theta = (A[q][q] - A[p][p]) / (2 * A[p][q])
                    t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1))
                    c = 1 / np.sqrt(t * t + 1)
                    s = t * c
                    for k in range(4):
                        akp, akq = A[k][p], A[k][q]
                        A[k][p] = np.where(rot, c * akp - s * akq, akp)
                        A[k][q] = np.where(rot, s * akp + c * akq, akq)
                    for k in range(4):
                        apk, aqk = A[p][k], A[q][k]
                        A[p][k] = np.where(rot, c * apk - s * aqk, apk)
                        A[q][k] = np.where(rot, s * apk + c * aqk, aqk)
                    for k in range(4):
                        vkp, vkq = V[k][p], V[k][q]
                        V[k][p] = np.where(rot, c * vkp - s * vkq, vkp)
                        V[k][q] = np.where(rot, s * vkp + c * vkq, vkq)
        best = A[0][0]
        q4 = [V[k][0] for k in range(4)]
        for i in range(1, 4):
            upd = A[i][i] > best
            best = np.where(upd, A[i][i], best)
            q4 = [np.where(upd, V[k][i], q4[k]) for k in range(4)]
        qw, qx, qy, qz = q4
        qn = np.sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz)
        qw, qx, qy, qz = qw / qn, qx / qn, qy / qn, qz / qn
        R = [[1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy)],
             [2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx)],
             [2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)]]
        nom = np.zeros(H)
        den = np.zeros(H)
        for i in range(3):
            for r in range(3):
                p3 = (R[r][0] * Pr2[:, i, 0] + R[r][1] * Pr2[:, i, 1]) + R[r][2] * Pr2[:, i, 2]
                nom = nom + Pr1[:, i, r] * p3
                den = den + p3 * p3
        s = den / den if fix_scale else nom / den
        inv = 1.0 / s
        T12 = np.zeros((H, 12), F32)
        T21 = np.zeros((H, 12), F32)
        sR12 = [[s * R[r][c] for c in range(3)] for r in range(3)]
        sR21 = [[inv * R[c][r] for c in range(3)] for r in range(3)]
        t12 = [O1[:, r] - ((sR12[r][0] * O2[:, 0] + sR12[r][1] * O2[:, 1]) + sR12[r][2] * O2[:, 2]) for r in range(3)]
        t21 = [-((sR21[r][0] * t12[0] + sR21[r][1] * t12[1]) + sR21[r][2] * t12[2]) for r in range(3)]
        for r in range(3):
            for c in range(3):
                T12[:, 4 * r + c] = sR12[r][c].astype(F32)
                T21[:, 4 * r + c] = sR21[r][c].astype(F32)
            T12[:, 4 * r + 3] = t12[r].astype(F32)
            T21[:, 4 * r + 3] = t21[r].astype(F32)
        return T12, T21, s.astype(F32)


def horn_eigh(P1, P2, fix_scale):
    """An independent Horn step: np.linalg.eigh of N, everything in fp64, no shared code with horn().
    -> T12 (H, 3, 4) float64, s."""
    P1 = np.asarray(P1, F32).astype(F64)
    P2 = np.asarray(P2, F32).astype(F64)
    T = np.zeros((len(P1), 3, 4))
    sc = np.zeros(len(P1))
    for h in range(len(P1)):
        o1, o2 = P1[h].mean(0), P2[h].mean(0)
        a, b = P1[h] - o1, P2[h] - o2
        M = b.T @ a
        N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                      [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                      [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                      [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
        N = N + np.triu(N, 1).T
        w, v = np.linalg.eigh(N)
        qw, qx, qy, qz = v[:, -1]
        R = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy)],
                      [2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx)],
                      [2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)]])
        p3 = b @ R.T
        s = 1.0 if fix_scale else (a * p3).sum() / (p3 * p3).sum()
        T[h, :, :3] = s * R
        T[h, :, 3] = o1 - s * R @ o2
        sc[h] = s
    return T, sc


# ---- CheckInliers ----------------------------------------------------------------------------

def _project(T, X, k):
    """sim3_project: T (H, 12) float32, X (N, 3) float32, k = fx fy cx cy float32 -> u, v (H, N)."""
    T = T[:, :, None]
    x, y, z = X[None, :, 0], X[None, :, 1], X[None, :, 2]
    px = ((T[:, 0] * x + T[:, 1] * y) + T[:, 2] * z) + T[:, 3]
    py = ((T[:, 4] * x + T[:, 5] * y) + T[:, 6] * z) + T[:, 7]
    pz = ((T[:, 8] * x + T[:, 9] * y) + T[:, 10] * z) + T[:, 11]
    invz = F32(1.0) / pz
    return k[0] * (px * invz) + k[2], k[1] * (py * invz) + k[3]


def _to_image(X, k):
    invz = F32(1.0) / X[:, 2]
    return k[0] * (X[:, 0] * invz) + k[2], k[1] * (X[:, 1] * invz) + k[3]


def errors(T12, T21, X1, X2, k1, k2):
    """err1, err2 of CheckInliers (:364-368), float32 (H, N)."""
    X1, X2 = np.asarray(X1, F32), np.asarray(X2, F32)
    k1, k2 = np.asarray(k1, F32), np.asarray(k2, F32)
    with np.errstate(all="ignore"):
        u11, v11 = _to_image(X1, k1)
        u21, v21 = _project(T12, X2, k1)
        u12, v12 = _project(T21, X1, k2)
        u22, v22 = _to_image(X2, k2)
        dx1, dy1, dx2, dy2 = u11[None] - u21, v11[None] - v21, u12 - u22[None], v12 - v22[None]
        err1, err2 = dx1 * dx1 + dy1 * dy1, dx2 * dx2 + dy2 * dy2
    assert err1.dtype == F32 and err2.dtype == F32
    return err1, err2


def pack_mask(flags):
    """(H, N) bool -> (H, ceil(N / 64)) uint64, bit i & 63 of word i >> 6."""
    H, N = flags.shape
    words = (N + 63) // 64
    b = np.zeros((H, words * 64), np.uint64)
    b[:, :N] = flags
    b = b.reshape(H, words, 64)
    return (b << np.arange(64, dtype=np.uint64)[None, None, :]).sum(-1, dtype=np.uint64)


def unpack_mask(mask, n):
    mask = np.asarray(mask, np.uint64)
    bits = (mask[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)
    return bits.reshape(len(mask), -1)[:, :n].astype(bool)


def hypotheses(X1, X2, e1, e2, k1, k2, fix_scale, triples):
    """Every hypothesis of one solver, as orbmi_sim3_ransac_batch returns them."""
    X1, X2 = np.asarray(X1, F32).reshape(-1, 3), np.asarray(X2, F32).reshape(-1, 3)
    triples = np.asarray(triples, np.int32).reshape(-1, 3)
    T12, T21, s = horn(X1[triples], X2[triples], fix_scale)
    err1, err2 = errors(T12, T21, X1, X2, k1, k2)
    with np.errstate(invalid="ignore"):
        flags = (err1 < np.asarray(e1, np.int32).astype(F32)[None]) & (err2 < np.asarray(e2, np.int32).astype(F32)[None])
    return {"T12": T12, "T21": T21, "s": s, "count": flags.sum(1).astype(np.int32), "mask": pack_mask(flags),
            "flags": flags, "err1": err1, "err2": err2}


# ---- iterate ---------------------------------------------------------------------------------

def iterate_sequence(hyp, its, n, min_inliers, indices1, n1, chunk, calls):
    """Sim3Solver::iterate (:140-220) called `calls` times with nIterations = chunk, read straight
    off the reference's loop.  -> [(h or None, bNoMore, vbInliers, nInliers)] with h the returned
    hypothesis."""
    out = []
    mn_iterations, best = 0, 0
    flags = unpack_mask(hyp["mask"], n) if its else None
    for _ in range(calls):
        vb = np.zeros(n1, bool)
        if n < min_inliers:
            out.append((None, True, vb, 0))
            continue
        cur, ret = 0, None
        while mn_iterations < its and cur < chunk:
            cur += 1
            h = mn_iterations
            mn_iterations += 1
            c = int(hyp["count"][h])
            if c >= best:
                best = c
                if c > min_inliers:
                    vb[np.asarray(indices1)[flags[h]]] = True
                    ret = (h, False, vb, c)
                    break
        out.append(ret if ret is not None else (None, mn_iterations >= its, vb, 0))
    return out


# ---- the Sim3 scene --------------------------------------------------------------------------

def rodrigues(rv):
    rv = np.asarray(rv, F64)
    th = np.linalg.norm(rv)
    k = rv / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K


def kitti_k():
    from orb_slam2_with_comment_amd import synth
    c = synth.KITTI
    return np.array([c.fx, c.fy, c.cx, c.cy], F32)


def sim3_scene(seed, outlier_fraction, fix_scale, n=120, ntriples=300):
    """KITTI intrinsics, n points in camera 1's frustum (z 5-40 m), X1 = s R X2 + t with rotation
    vector (0.02, -0.15, 0.01), t = (0.8, -0.05, 1.5), s = 1 (fix_scale) or 1.1; Gaussian noise of
    1 cm * z / 10 on X2, a fraction of X2 displaced by uniform +-3 m, octaves uniform in 0-7,
    triples of three distinct indices from default_rng(seed)."""
    rng = np.random.default_rng(seed)
    k = kitti_k()
    z = rng.uniform(5, 40, n)
    u, v = rng.uniform(0, 1241, n), rng.uniform(0, 376, n)
    X1 = np.stack([(u - k[2]) * z / k[0], (v - k[3]) * z / k[1], z], -1)
    R, t, s = rodrigues([0.02, -0.15, 0.01]), np.array([0.8, -0.05, 1.5]), (1.0 if fix_scale else 1.1)
    X2 = (X1 - t) @ R / s  # R^T (X1 - t) / s
    X2 = X2 + rng.normal(size=(n, 3)) * (0.01 * z / 10)[:, None]
    out = rng.permutation(n)[:int(round(outlier_fraction * n))]
    X2[out] += rng.uniform(-3, 3, (len(out), 3))
    table = max_error(level_sigma2())
    e1, e2 = table[rng.integers(0, 8, n)], table[rng.integers(0, 8, n)]
    triples = np.array([rng.permutation(n)[:3] for _ in range(ntriples)], np.int32).reshape(-1, 3) if n >= 3 else \
        np.zeros((0, 3), np.int32)
    return {"X1": X1.astype(F32), "X2": X2.astype(F32), "e1": e1.astype(np.int32), "e2": e2.astype(np.int32),
            "k1": k, "k2": k.copy(), "fix_scale": int(fix_scale), "triples": triples, "n": n,
            "T12_true": np.hstack([s * R, t[:, None]])}


def write_problem(path, sc):
    """One scene as tests/cpp/sim3_check.cpp reads it."""
    with open(path, "wb") as f:
        f.write(np.array([sc["n"], len(sc["triples"]), sc["fix_scale"]], np.int32).tobytes())
        f.write(np.concatenate([sc["k1"], sc["k2"]]).astype(np.float32).tobytes())
        for key, dt in (("X1", np.float32), ("X2", np.float32), ("e1", np.int32), ("e2", np.int32), ("triples", np.int32)):
            f.write(np.ascontiguousarray(sc[key], dt).tobytes())


def canon(a):
    """Bit pattern of a float32 array with every NaN mapped to one pattern (hosts and the device
    produce different NaN payloads; only NaN-ness is pinned)."""
    a = np.ascontiguousarray(a, F32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def assert_hypotheses_equal(got, ref):
    """Bit-equal (every NaN counted as one pattern: its payload differs between processors)."""
    for key in ("T12", "T21", "s"):
        np.testing.assert_array_equal(canon(got[key]), canon(ref[key]), err_msg=key)
    np.testing.assert_array_equal(got["count"], ref["count"])
    np.testing.assert_array_equal(got["mask"], ref["mask"])


_REF = {}


def scene_ref(seed, frac, fix):
    """The scene and the restatement's hypotheses, computed once per case."""
    key = (seed, frac, fix)
    if key not in _REF:
        sc = sim3_scene(seed, frac, fix)
        _REF[key] = (sc, hypotheses(sc["X1"], sc["X2"], sc["e1"], sc["e2"], sc["k1"], sc["k2"], fix, sc["triples"]))
    return _REF[key]


# ---- SearchBySim3 ----------------------------------------------------------------------------

_POPC = np.array([bin(i).count("1") for i in range(256)], np.int32)


def _xform(T, X):
    """R X + t in float32, left to right (T: 3x4 or 4x4 float32, X: (n, 3) float32)."""
    return np.stack([((T[r, 0] * X[:, 0] + T[r, 1] * X[:, 1]) + T[r, 2] * X[:, 2]) + T[r, 3] for r in range(3)], -1)


def sim3_matrices(s12, R12, t12):
    """sR12 = s12 R12, sR21 = (1.0 / s12) R12^T, t21 = -sR21 t12 (src/ORBmatcher.cc:1304-1308):
    the scalar a double, the matrix float32, one rounding per entry.  -> S12, S21 (3x4 float32)."""
    R12, t12 = np.asarray(R12, F32).reshape(3, 3), np.asarray(t12, F32).reshape(3)
    s = F64(F32(s12))
    sR12 = (s * R12.astype(F64)).astype(F32)
    sR21 = ((1.0 / s) * R12.T.astype(F64)).astype(F32)
    t21 = np.array([-((sR21[r, 0] * t12[0] + sR21[r, 1] * t12[1]) + sR21[r, 2] * t12[2]) for r in range(3)], F32)
    return np.hstack([sR12, t12[:, None]]).astype(F32), np.hstack([sR21, t21[:, None]]).astype(F32)


def _search_direction(src_tcw, mps, has, skip, S, k, target, th):
    """One loop of SearchBySim3 (:1338-1421 / :1425-1502): the source keyframe's points searched in
    the target keyframe.  -> vnMatch (len(mps)), best distances."""
    from orb_slam2_with_comment_amd.types import MP_BAD
    v = target.view()
    min_x, max_x, min_y, max_y = F32(v.min_x), F32(v.max_x), F32(v.min_y), F32(v.max_y)
    gwi, ghi = F32(v.grid_w_inv), F32(v.grid_h_inv)
    scale, logsf, nlev = np.asarray(target.scale_factors, F32), F32(v.log_scale_factor), v.nlevels
    kx, ky, koct = target.keys["x"].astype(F32), target.keys["y"].astype(F32), target.keys["octave"]
    # Frame::AssignFeaturesToGrid: round half away from zero
    gx = ((kx - min_x) * gwi).astype(F64)
    gy = ((ky - min_y) * ghi).astype(F64)
    px = (np.sign(gx) * np.floor(np.abs(gx) + 0.5)).astype(np.int64)
    py = (np.sign(gy) * np.floor(np.abs(gy) + 0.5)).astype(np.int64)
    in_grid = (px >= 0) & (px < 64) & (py >= 0) & (py < 48)
    cell = px * 48 + py
    n = len(mps)
    vn, bd = np.full(n, -1, np.int32), np.full(n, 256, np.int32)
    if n == 0 or len(kx) == 0:
        return vn, bd
    th = F32(th)
    with np.errstate(all="ignore"):
        Pc = _xform(S, _xform(np.asarray(src_tcw, F32).reshape(4, 4), mps["pos"].astype(F32)))
        invz = F32(1.0) / Pc[:, 2]
        u = k[0] * (Pc[:, 0] * invz) + k[2]
        w = k[1] * (Pc[:, 1] * invz) + k[3]
        d3 = np.sqrt((Pc[:, 0].astype(F64) ** 2 + Pc[:, 1].astype(F64) ** 2) + Pc[:, 2].astype(F64) ** 2).astype(F32)
    ok = np.asarray(has, bool) & ~np.asarray(skip, bool) & ((mps["flags"] & MP_BAD) == 0)
    ok &= ~(Pc[:, 2] < 0)
    ok &= (u >= min_x) & (u < max_x) & (w >= min_y) & (w < max_y)
    ok &= ~((d3 < F32(0.8) * mps["min_distance"]) | (d3 > F32(1.2) * mps["max_distance"]))
    for i in np.nonzero(ok)[0]:
        ratio = F32(mps["max_distance"][i] / d3[i])
        level = int(np.ceil(F32(F32(math.log(float(ratio))) / logsf)))
        level = min(max(level, 0), nlev - 1)
        r = F32(th * scale[level])
        x0 = max(0, int(np.floor(F32(F32(F32(u[i] - min_x) - r) * gwi))))
        x1 = min(63, int(np.ceil(F32(F32(F32(u[i] - min_x) + r) * gwi))))
        y0 = max(0, int(np.floor(F32(F32(F32(w[i] - min_y) - r) * ghi))))
        y1 = min(47, int(np.ceil(F32(F32(F32(w[i] - min_y) + r) * ghi))))
        c = in_grid & (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1)
        c &= (np.abs(kx - u[i]) < r) & (np.abs(ky - w[i]) < r) & (koct >= level - 1) & (koct <= level)
        idx = np.nonzero(c)[0]
        if len(idx) == 0:
            continue
        dist = _POPC[target.desc[idx] ^ mps["desc"][i][None, :]].sum(1)
        best = np.lexsort((idx, cell[idx], dist))[0]  # least distance, then the first in grid order
        bd[i] = dist[best]
        if dist[best] <= 100:
            vn[i] = idx[best]
    return vn, bd


def search_by_sim3(kf1, mps1, has1, kf2, mps2, has2, s12, R12, t12, th, match12):
    """ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:1285-1525), float32-exact.  match12 as
    orbmi_search_by_sim3 takes it.  -> vnMatch1, vnMatch2, match12 after, nFound, (dist1, dist2)."""
    m12 = np.asarray(match12, np.int32).copy()
    n1, n2 = len(kf1.keys), len(kf2.keys)
    already1 = m12 != -1
    already2 = np.zeros(n2, bool)
    already2[m12[(m12 >= 0) & (m12 < n2)]] = True
    S12, S21 = sim3_matrices(s12, R12, t12)
    k = np.array([kf1.cam.fx, kf1.cam.fy, kf1.cam.cx, kf1.cam.cy], F32)  # KF1's in both directions
    vn1, d1 = _search_direction(kf1.tcw, mps1, has1, already1, S21, k, kf2, th)
    vn2, d2 = _search_direction(kf2.tcw, mps2, has2, already2, S12, k, kf1, th)
    nfound = 0
    for i1 in range(n1):
        if vn1[i1] >= 0 and vn2[vn1[i1]] == i1:
            m12[i1] = vn1[i1]
            nfound += 1
    return vn1, vn2, m12, nfound, (d1, d2)


@functools.lru_cache(maxsize=None)
def sim3_search_scene(f1=4, f2=6, s12=1.0, seed=0):
    """KF1 = frame f1, KF2 = frame f2 of the synthetic KITTI sequence, their own stereo map points
    scattered to the keypoint slots (2 % flagged bad), S12 = T1w Tw2 with t perturbed by 0.02 m,
    20 % of KF1's points pre-matched (to a random KF2 slot, or -2: no index in KF2).  s12 != 1:
    KF2's map (points, pose, distances) lives in a world scaled by 1 / s12."""
    import scenario
    from orb_slam2_with_comment_amd import synth, synth_map as SM
    from orb_slam2_with_comment_amd.types import MAPPOINT_DTYPE
    rng = np.random.default_rng(seed)
    sf = scenario.scale_factors()
    out = []
    for f in (f1, f2):
        kl, dl, u, d, T = scenario.frame_data(f)
        mp, idx = SM.mappoints_from_frame(kl, dl, d, synth.KITTI, T, sf, rng, 0.02)
        slots = np.zeros(len(kl), MAPPOINT_DTYPE)
        slots[idx] = mp
        has = np.zeros(len(kl), np.uint8)
        has[idx] = 1
        out.append((scenario.make_frame(f), slots, has))
    (kf1, mps1, has1), (kf2, mps2, has2) = out
    T12 = kf1.tcw.astype(F64) @ np.linalg.inv(kf2.tcw.astype(F64))
    R12 = T12[:3, :3].astype(F32)
    t12 = (T12[:3, 3] + np.array([0.02, -0.02, 0.02])).astype(F32)
    if s12 != 1.0:
        mps2 = mps2.copy()
        for key in ("pos", "max_distance", "min_distance"):
            mps2[key] = (mps2[key].astype(F64) / s12).astype(F32)
        tcw = kf2.tcw.copy()
        tcw[:3, 3] = (tcw[:3, 3].astype(F64) / s12).astype(F32)
        kf2.tcw = tcw
    m12 = np.full(len(kf1.keys), -1, np.int32)
    pre = np.nonzero(has1)[0]
    pre = pre[rng.random(len(pre)) < 0.2]
    m12[pre] = np.where(rng.random(len(pre)) < 0.8, rng.integers(0, len(kf2.keys), len(pre)), -2)
    return {"kf1": kf1, "mps1": mps1, "has1": has1, "kf2": kf2, "mps2": mps2, "has2": has2, "s12": s12, "R12": R12,
            "t12": t12, "th": 7.5, "match12": m12}
