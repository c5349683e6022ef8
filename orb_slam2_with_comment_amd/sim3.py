"""Python mirror of ORB_SLAM2::Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc) over the C ABI.

The device computes every RANSAC hypothesis of every solver of a batch in one launch
(orbmi_sim3_ransac_batch: ComputeSim3 + CheckInliers per iteration); Sim3Solver.iterate replays
the reference's best / return rule over those arrays on the host.  The replay takes the arrays
from anywhere (Sim3Solver.set_hypotheses), so it can be driven without a GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._capi import check, lib
from .types import MP_BAD


class Sim3Problem(C.Structure):
    """orbmi_sim3_problem (include/orbmi.h)."""
    _fields_ = [("n", C.c_int32), ("x3d_c1", C.c_void_p), ("x3d_c2", C.c_void_p), ("max_err1", C.c_void_p),
                ("max_err2", C.c_void_p), ("k1", C.c_float * 4), ("k2", C.c_float * 4), ("fix_scale", C.c_int32),
                ("probability", C.c_double), ("min_inliers", C.c_int32), ("max_iterations", C.c_int32),
                ("triples", C.c_void_p), ("seed", C.c_uint64)]


class Sim3Hypotheses(C.Structure):
    """orbmi_sim3_hypotheses (include/orbmi.h)."""
    _fields_ = [("iterations", C.c_int32), ("T12", C.c_void_p), ("T21", C.c_void_p), ("s", C.c_void_p),
                ("count", C.c_void_p), ("mask", C.c_void_p)]


def sim3_iterations(n: int, min_inliers: int, probability: float = 0.99, max_iterations: int = 300) -> int:
    """SetRansacParameters' mRansacMaxIts (src/Sim3Solver.cc:125-135); 0 when n < min_inliers."""
    out = C.c_int()
    check("orbmi_sim3_iterations", lib().orbmi_sim3_iterations(n, min_inliers, probability, max_iterations, C.byref(out)))
    return out.value


def sim3_sample_triples(seed: int, solver: int, n: int, iterations: int) -> np.ndarray:
    """The minimal sets of :167-185 from the library's counter-based generator: (iterations, 3)."""
    out = np.zeros((max(iterations, 1), 3), np.int32)
    check("orbmi_sim3_sample_triples", lib().orbmi_sim3_sample_triples(seed, solver, n, iterations, out.ctypes.data))
    return out[:iterations]


def sim3_max_error(sigma2) -> np.ndarray:
    """mvnMaxError per level: (size_t)(9.210 * sigma2), :87-88."""
    out, v = [], C.c_int32()
    for s in np.atleast_1d(np.asarray(sigma2, np.float32)):
        check("orbmi_sim3_max_error", lib().orbmi_sim3_max_error(float(s), C.byref(v)))
        out.append(v.value)
    return np.array(out, np.int32)


def problem(x3d_c1, x3d_c2, max_err1, max_err2, k1, k2, fix_scale, probability=0.99, min_inliers=6,
            max_iterations=300, triples=None, seed=0) -> dict:
    """One solver's inputs as the arrays orbmi_sim3_problem points to."""
    return {"x1": np.ascontiguousarray(x3d_c1, np.float32).reshape(-1, 3),
            "x2": np.ascontiguousarray(x3d_c2, np.float32).reshape(-1, 3),
            "e1": np.ascontiguousarray(max_err1, np.int32), "e2": np.ascontiguousarray(max_err2, np.int32),
            "k1": np.ascontiguousarray(k1, np.float32), "k2": np.ascontiguousarray(k2, np.float32),
            "fix_scale": int(bool(fix_scale)), "probability": float(probability), "min_inliers": int(min_inliers),
            "max_iterations": int(max_iterations), "seed": int(seed),
            "triples": None if triples is None else np.ascontiguousarray(triples, np.int32).reshape(-1, 3)}


class Sim3Ransac:
    """The batched device call.  matcher: an ORBmatcher whose handle and stream are used."""

    def __init__(self, matcher=None, device: int = 0):
        from .matcher import ORBmatcher
        self._own = matcher is None
        self.matcher = ORBmatcher(device=device) if matcher is None else matcher

    def close(self):
        if self._own and self.matcher is not None:
            self.matcher.close()
        self.matcher = None

    def __call__(self, problems: list) -> list:
        """problems: dicts of problem().  -> per solver {"iterations", "T12" (H, 12), "T21", "s",
        "count", "mask" (H, words)} with H = iterations."""
        m = len(problems)
        P, R = (Sim3Problem * max(m, 1))(), (Sim3Hypotheses * max(m, 1))()
        bufs = []
        for k, p in enumerate(problems):
            n = len(p["x1"])
            if len(p["x2"]) != n or len(p["e1"]) != n or len(p["e2"]) != n:
                raise ValueError("sim3 problem arrays differ in length")
            cap = max(sim3_iterations(n, p["min_inliers"], p["probability"], p["max_iterations"]), 1)
            if p["triples"] is not None and len(p["triples"]) < cap:
                raise ValueError("fewer triples than iterations")
            words = max((n + 63) // 64, 1)
            b = {"T12": np.zeros((cap, 12), np.float32), "T21": np.zeros((cap, 12), np.float32),
                 "s": np.zeros(cap, np.float32), "count": np.zeros(cap, np.int32), "mask": np.zeros((cap, words), np.uint64)}
            bufs.append(b)
            P[k].n = n
            P[k].x3d_c1, P[k].x3d_c2 = p["x1"].ctypes.data, p["x2"].ctypes.data
            P[k].max_err1, P[k].max_err2 = p["e1"].ctypes.data, p["e2"].ctypes.data
            P[k].k1, P[k].k2 = (C.c_float * 4)(*p["k1"]), (C.c_float * 4)(*p["k2"])
            P[k].fix_scale, P[k].probability = p["fix_scale"], p["probability"]
            P[k].min_inliers, P[k].max_iterations, P[k].seed = p["min_inliers"], p["max_iterations"], p["seed"]
            P[k].triples = None if p["triples"] is None else p["triples"].ctypes.data
            R[k].T12, R[k].T21, R[k].s = b["T12"].ctypes.data, b["T21"].ctypes.data, b["s"].ctypes.data
            R[k].count, R[k].mask = b["count"].ctypes.data, b["mask"].ctypes.data
        check("orbmi_sim3_ransac_batch", lib().orbmi_sim3_ransac_batch(self.matcher._h, m, P, R))
        out = []
        for k, b in enumerate(bufs):
            H = R[k].iterations
            out.append({"iterations": H, **{key: a[:H] for key, a in b.items()}})
        return out


def unpack_mask(mask: np.ndarray, n: int) -> np.ndarray:
    """One hypothesis' bitmask words -> mvbInliersi (n bools)."""
    bits = (np.asarray(mask, np.uint64)[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)
    return bits.reshape(-1)[:n].astype(bool)


def _to_camera(tcw, xw):
    """Rcw * X3Dw + tcw in float32 (:94-98)."""
    T, X = np.asarray(tcw, np.float32).reshape(4, 4), np.asarray(xw, np.float32).reshape(-1, 3)
    return np.stack([((T[r, 0] * X[:, 0] + T[r, 1] * X[:, 1]) + T[r, 2] * X[:, 2]) + T[r, 3] for r in range(3)], -1)


class Sim3Solver:
    """Sim3Solver(pKF1, pKF2, vpMatched12, bFixScale) (src/Sim3Solver.cc:37-112).

    kf1, kf2: types.Frame (mvKeysUn, pose, intrinsics, scale factors); mps1 / mps2: orbmi_mappoint
    records per keypoint slot of KF1 / KF2 (GetMapPointMatches), has_mp1 / has_mp2 = the slot holds
    a point (default: all); matches12[i1] = the KF2 slot of vpMatched12[i1]
    (GetIndexInKeyFrame(pKF2)), < 0 for none."""

    def __init__(self, kf1, kf2, mps1, mps2, matches12, bFixScale, has_mp1=None, has_mp2=None, seed=0, solver=0):
        m12 = np.asarray(matches12, np.int64)
        self.mN1 = len(m12)
        has1 = np.ones(len(mps1), bool) if has_mp1 is None else np.asarray(has_mp1, bool)
        has2 = np.ones(len(mps2), bool) if has_mp2 is None else np.asarray(has_mp2, bool)
        keep = []
        for i1 in range(self.mN1):  # :62-103
            i2 = int(m12[i1])
            if i2 < 0 or i2 >= len(mps2) or not has2[i2] or i1 >= len(mps1) or not has1[i1]:
                continue
            if (mps1["flags"][i1] & MP_BAD) or (mps2["flags"][i2] & MP_BAD):
                continue
            keep.append((i1, i2))
        keep = np.array(keep, np.int64).reshape(-1, 2)
        self.mvnIndices1 = keep[:, 0].astype(np.int32)
        self.mvnIndices2 = keep[:, 1].astype(np.int32)
        s1 = np.asarray(kf1.scale_factors, np.float32)
        s2 = np.asarray(kf2.scale_factors, np.float32)
        self.mvnMaxError1 = sim3_max_error(s1 * s1)[kf1.keys["octave"][keep[:, 0]]]
        self.mvnMaxError2 = sim3_max_error(s2 * s2)[kf2.keys["octave"][keep[:, 1]]]
        self.mvX3Dc1 = _to_camera(kf1.tcw, mps1["pos"][keep[:, 0]])
        self.mvX3Dc2 = _to_camera(kf2.tcw, mps2["pos"][keep[:, 1]])
        self.mK1 = np.array([kf1.cam.fx, kf1.cam.fy, kf1.cam.cx, kf1.cam.cy], np.float32)
        self.mK2 = np.array([kf2.cam.fx, kf2.cam.fy, kf2.cam.cx, kf2.cam.cy], np.float32)
        self._init(bFixScale, seed, solver)

    @classmethod
    def from_arrays(cls, x3d_c1, x3d_c2, max_err1, max_err2, k1, k2, bFixScale, indices1=None, n1=None, seed=0,
                    solver=0):
        """A solver from the constructor's outputs (the arrays of orbmi_sim3_problem)."""
        self = cls.__new__(cls)
        self.mvX3Dc1 = np.ascontiguousarray(x3d_c1, np.float32).reshape(-1, 3)
        self.mvX3Dc2 = np.ascontiguousarray(x3d_c2, np.float32).reshape(-1, 3)
        self.mvnMaxError1 = np.ascontiguousarray(max_err1, np.int32)
        self.mvnMaxError2 = np.ascontiguousarray(max_err2, np.int32)
        self.mK1, self.mK2 = np.ascontiguousarray(k1, np.float32), np.ascontiguousarray(k2, np.float32)
        n = len(self.mvX3Dc1)
        self.mvnIndices1 = np.arange(n, dtype=np.int32) if indices1 is None else np.asarray(indices1, np.int32)
        self.mN1 = n if n1 is None else int(n1)
        self._init(bFixScale, seed, solver)
        return self

    def _init(self, bFixScale, seed, solver):
        self.N = len(self.mvX3Dc1)
        self.mbFixScale = bool(bFixScale)
        self.seed, self.solver = int(seed), int(solver)
        self.triples = None
        self._auto_triples = False
        self.SetRansacParameters()  # :111

    def SetRansacParameters(self, probability=0.99, minInliers=6, maxIterations=300):
        """:114-138 (the defaults of include/Sim3Solver.h:48)."""
        self.mRansacProb, self.mRansacMinInliers = float(probability), int(minInliers)
        self.mRansacMaxIts = sim3_iterations(self.N, self.mRansacMinInliers, self.mRansacProb, int(maxIterations))
        self._max_iterations = int(maxIterations)
        self.mnIterations = 0
        self.mnBestInliers = 0
        self._best = None
        self._hyp = None
        if self._auto_triples:  # drawn for the previous iteration count
            self.triples, self._auto_triples = None, False

    def problem(self) -> dict:
        return problem(self.mvX3Dc1, self.mvX3Dc2, self.mvnMaxError1, self.mvnMaxError2, self.mK1, self.mK2,
                       self.mbFixScale, self.mRansacProb, self.mRansacMinInliers, self._max_iterations, self.triples,
                       self.seed)

    def set_hypotheses(self, hyp: dict):
        """The per-hypothesis arrays iterate replays: from Sim3Ransac / solve_batch, or from any
        other implementation of the same arithmetic."""
        self._hyp = hyp

    def iterate(self, nIterations, ransac: Sim3Ransac | None = None):
        """:140-220 -> (T12 (4x4) | None, bNoMore, vbInliers (mN1), nInliers)."""
        vb = np.zeros(self.mN1, bool)
        if self.N < self.mRansacMinInliers:
            return None, True, vb, 0
        if self._hyp is None:
            if ransac is None:
                raise RuntimeError("no hypotheses: call solve_batch / set_hypotheses, or pass a Sim3Ransac")
            solve_batch([self], ransac)
        H = self._hyp
        cur = 0
        while self.mnIterations < self.mRansacMaxIts and cur < nIterations:
            cur += 1
            h = self.mnIterations
            self.mnIterations += 1
            c = int(H["count"][h])
            if c >= self.mnBestInliers:
                self.mnBestInliers = c
                self._best = h
                if c > self.mRansacMinInliers:
                    vb[self.mvnIndices1[unpack_mask(H["mask"][h], self.N)]] = True
                    return self._T(H["T12"][h]), False, vb, c
        return None, self.mnIterations >= self.mRansacMaxIts, vb, 0

    def find(self, ransac: Sim3Ransac | None = None):
        """:222-226 -> (T12 | None, vbInliers12, nInliers)."""
        T, _, vb, n = self.iterate(self.mRansacMaxIts, ransac)
        return T, vb, n

    @staticmethod
    def _T(rows):
        T = np.eye(4, dtype=np.float32)
        T[:3] = np.asarray(rows, np.float32).reshape(3, 4)
        return T

    def GetEstimatedScale(self) -> float:
        return float(self._hyp["s"][self._best])

    def GetEstimatedRotation(self) -> np.ndarray:
        """mBestRotation = mR12i: sR12 / s, one float32 division per entry."""
        return (self._T(self._hyp["T12"][self._best])[:3, :3] / np.float32(self._hyp["s"][self._best])).astype(np.float32)

    def GetEstimatedTranslation(self) -> np.ndarray:
        return self._T(self._hyp["T12"][self._best])[:3, 3].copy()


def solve_batch(solvers: list, ransac: Sim3Ransac):
    """Every hypothesis of several solvers in one launch (the candidate loop of
    LoopClosing::ComputeSim3, src/LoopClosing.cc:349-398): each solver's iterate then replays its
    own arrays.  A solver without explicit triples samples as position `solver.solver` of seed."""
    probs = []
    for s in solvers:
        if s.triples is None and s.mRansacMaxIts > 0:
            s.triples = sim3_sample_triples(s.seed, s.solver, s.N, s.mRansacMaxIts)
            s._auto_triples = True
        probs.append(s.problem())
    for s, h in zip(solvers, ransac(probs)):
        s.set_hypotheses(h)


# ---- LoopClosing::ComputeSim3 from the solvers on (src/LoopClosing.cc:331-490) -------------------

def _quat_to_R(q):
    x, y, z, w = (float(v) for v in q)
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    return np.array([[1 - (ty * y + tz * z), ty * x - tz * w, tz * x + ty * w],
                     [ty * x + tz * w, 1 - (tx * x + tz * z), tz * y - tx * w],
                     [tz * x - ty * w, tz * y + tx * w, 1 - (tx * x + ty * y)]], np.float64)


class DeviceBackend:
    """The four device operators compute_sim3 chains, on one matcher handle (one stream, one
    staging arena).  A test drives compute_sim3 with an object of the same four methods."""

    def __init__(self, matcher=None, device: int = 0):
        from .matcher import ORBmatcher
        from .optimizer import Sim3Optimizer
        self._own = matcher is None
        self.matcher = ORBmatcher(device=device) if matcher is None else matcher
        self.ransac = Sim3Ransac(self.matcher)
        self.optimizer = Sim3Optimizer(self.matcher)

    def close(self):
        if self._own and self.matcher is not None:
            self.matcher.close()
        self.matcher = None

    def solve_batch(self, solvers):
        solve_batch(solvers, self.ransac)

    def search_by_sim3(self, cur, cand, match12, s, R, t, th):
        return self.matcher.SearchBySim3(cur["kf"], cur["mps"], cur["has"], cand["kf"], cand["mps"], cand["has"], match12,
                                         s, R, t, th)[0]

    def optimize(self, problems):
        return self.optimizer.run(problems)

    def search_by_projection(self, kf, Scw, mps, matched, th):
        return self.matcher.SearchByProjectionSim3(kf, Scw, mps, matched, th)


def compute_sim3(cur_kf, candidates, bow_matches, loop_points_of, fix_scale, seed=0, backend=None):
    """LoopClosing::ComputeSim3 (src/LoopClosing.cc:331-490) from the Sim3Solvers on, over the
    device operators.  cur_kf and every candidate: {"kf": types.Frame, "mps": orbmi_mappoint
    records per keypoint slot, "has": the slot holds a point} (and optionally "bad": isBad());
    bow_matches[i][j] = the slot in candidate i of SearchByBoW(cur, candidate i)'s match for slot j
    of the current keyframe, -1 for none (SearchByBoW(KF, KF) is the caller's);
    loop_points_of(i) -> (records, slot_to_index): mvpLoopMapPoints of candidate i (:436-455) and,
    per keypoint slot of candidate i, the index of its point in that list (-1: not in it).

    Per round every live candidate runs 5 RANSAC iterations (all hypotheses of all solvers come
    from one solve_batch call); a candidate at its iteration limit is discarded (bNoMore).  Every
    candidate that returned a Sim3 goes through SearchBySim3 (th 7.5) and then all of them through
    one OptimizeSim3 batch (th2 10); the first in candidate order with nIn >= 20 wins, which is the
    candidate the reference's sequential loop stops at.  Then Scw = Scm * Smw,
    SearchByProjection(cur, Scw, loop points, th 10), accepted at >= 40 matches.  No SetErase
    bookkeeping.

    -> {"accepted", "candidate" (index or None), "Scw" (4x4 float32), "scw" {"sR", "t", "s"} in
    doubles, "matches" (per current slot: the candidate's slot, -1 none), "loop_matched" (per
    current slot: index into the loop points, -1 none, -2 a point outside the list), "n_total",
    "log" (per-stage counts)}."""
    from .optimizer import Sim3Optimizer
    own = backend is None
    be = DeviceBackend() if own else backend
    try:
        return _compute_sim3(cur_kf, candidates, bow_matches, loop_points_of, fix_scale, seed, be, Sim3Optimizer)
    finally:
        if own:
            be.close()


def _compute_sim3(cur, candidates, bow_matches, loop_points_of, fix_scale, seed, be, Sim3Optimizer):
    n0 = len(candidates)
    log = []
    out = {"accepted": False, "candidate": None, "Scw": None, "scw": None, "matches": None, "loop_matched": None,
           "n_total": 0, "log": log}
    solvers, discarded = [None] * n0, [False] * n0
    ncand = 0
    for i, c in enumerate(candidates):  # :316-348
        bow = np.asarray(bow_matches[i], np.int32)
        nmatches = int((bow >= 0).sum())
        if c.get("bad", False) or nmatches < 20:
            discarded[i] = True
            log.append(("discarded", i, nmatches))
            continue
        s = Sim3Solver(cur["kf"], c["kf"], cur["mps"], c["mps"], bow, fix_scale, cur["has"], c["has"], seed=seed, solver=i)
        s.SetRansacParameters(0.99, 20, 300)
        solvers[i] = s
        ncand += 1
    rounds = 0
    winner = None
    while ncand > 0 and winner is None:  # :357-423
        rounds += 1
        fresh = [s for i, s in enumerate(solvers) if s is not None and not discarded[i] and s._hyp is None
                 and s.N >= s.mRansacMinInliers]
        if fresh:
            be.solve_batch(fresh)
            log.append(("solve_batch", rounds, len(fresh)))
        returned = []
        for i in range(n0):
            if discarded[i]:
                continue
            T, no_more, vb, nin = solvers[i].iterate(5)
            if no_more:
                discarded[i] = True
                ncand -= 1
            if T is not None:
                returned.append((i, vb, nin))
        problems, kept = [], []
        for i, vb, nin in returned:
            c, s = candidates[i], solvers[i]
            bow = np.asarray(bow_matches[i], np.int32)
            m12 = np.where(vb, bow, -1).astype(np.int32)  # :389-394
            R, t, sc = s.GetEstimatedRotation(), s.GetEstimatedTranslation(), s.GetEstimatedScale()
            m12 = np.array(be.search_by_sim3(cur, c, m12, sc, R, t, 7.5), np.int32)
            p, idx = Sim3Optimizer.assemble(cur["kf"], c["kf"], cur["mps"], c["mps"], m12, R, t, sc, 10, fix_scale, cur["has"])
            problems.append(p)
            kept.append((i, m12, idx, nin))
        if not problems:
            continue
        results = be.optimize(problems)
        log.append(("optimize_batch", rounds, [(i, nin, int((m12 != -1).sum()), r["n_in"]) for (i, m12, _, nin), r in
                                               zip(kept, results)]))
        for (i, m12, idx, _), r in zip(kept, results):
            if r["n_in"] >= 20:  # :408
                m12[idx[np.asarray(r["inlier"]) == 0]] = -1
                winner = (i, m12, r)
                break
    log.append(("rounds", rounds))
    if winner is None:
        return out
    i, m12, r = winner
    c = candidates[i]
    # mg2oScw = gScm * gSmw, gSmw = Sim3(Rmw, tmw, 1.0) (:413-416), then Converter::toCvMat
    Tmw = np.asarray(c["kf"].tcw, np.float32).reshape(4, 4).astype(np.float64)
    sR_cm = float(r["s"]) * _quat_to_R(r["q"])
    sR = sR_cm @ Tmw[:3, :3]
    t = sR_cm @ Tmw[:3, 3] + np.asarray(r["t"], np.float64)
    Scw = np.eye(4, dtype=np.float32)
    Scw[:3, :3], Scw[:3, 3] = sR.astype(np.float32), t.astype(np.float32)
    pts, slot_to_index = loop_points_of(i)
    slot_to_index = np.asarray(slot_to_index, np.int64)
    matched = np.full(len(m12), -1, np.int32)  # mvpCurrentMatchedPoints in the list's indices
    has = m12 >= 0
    where = slot_to_index[m12[has]]
    matched[has] = np.where(where >= 0, where, -2)
    matched[m12 == -2] = -2
    matched, nproj = be.search_by_projection(cur["kf"], Scw, pts, matched, 10)
    n_total = int((np.asarray(matched) != -1).sum())
    log.append(("search_by_projection", i, int(nproj), n_total))
    out.update(candidate=i, Scw=Scw, scw={"sR": sR, "t": t, "s": float(r["s"])}, matches=m12,
               loop_matched=np.asarray(matched, np.int32), n_total=n_total, accepted=n_total >= 40)
    return out
