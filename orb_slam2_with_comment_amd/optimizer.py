"""Python mirror of Optimizer::LocalBundleAdjustment (include/Optimizer.h:62) over the C ABI.

`gather_local_ba` restates the graph assembly of src/Optimizer.cc:486-683 (local keyframes =
pKF + covisible, local points, fixed observer keyframes, one edge per observation) over a
minimal map model; `LocalBA.run` optimises the assembled graph on the GPU."""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from ._capi import check, lib
from .types import BA_EDGE_DTYPE, BA_KF_DTYPE, BA_PT_DTYPE, BAProblem


class LocalBA:
    def __init__(self, device: int = 0):
        h = C.c_void_p()
        check("orbmi_ba_create", lib().orbmi_ba_create(device, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().orbmi_ba_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stop_at_check(self, k: int):
        """The deterministic pbStopFlag (orbmi_ba_set_stop_at_check): later calls read the flag
        raised from their k-th check on; k < 0 turns it off."""
        check("orbmi_ba_set_stop_at_check", lib().orbmi_ba_set_stop_at_check(self._h, int(k)))

    def run(self, problem: BAProblem, stop: C.c_int | None = None, stop_at_check: int | None = None):
        if stop_at_check is not None:
            self.set_stop_at_check(stop_at_check)
        r, tcw, pos, erase = problem.result_buffers()
        v = problem.view()
        check("orbmi_local_bundle_adjustment",
              lib().orbmi_local_bundle_adjustment(self._h, C.addressof(v), C.addressof(r),
                                                  C.addressof(stop) if stop is not None else None))
        return self.result(problem, r, tcw, pos, erase)

    @staticmethod
    def result(problem: BAProblem, r, tcw, pos, erase):
        """run()'s return value from a filled orbmi_ba_result and its buffers (problem.result_buffers())."""
        n = len(problem.kfs), len(problem.pts), len(problem.edges)
        return {"tcw": tcw[:n[0]].reshape(-1, 4, 4), "pos": pos[:n[1]], "erase": erase[:n[2]].astype(bool),
                "iterations": tuple(r.iterations), "chi2": tuple(r.chi2), "aborted": r.aborted,
                "stop_check": r.stop_check, "checks": r.checks}


class GlobalBA(LocalBA):
    """Optimizer::BundleAdjustment (src/Optimizer.cc:56-255) over the C ABI, on an orbmi_ba handle:
    `run` optimises a graph assembled by gather_global_ba (or any BAProblem) on the GPU."""

    TERMINATE, SOLVE_FAILED, REJECTED = 1, 2, 4   # ORBMI_GBA_*

    def run(self, problem: BAProblem, iterations: int = 10, robust: bool = False, stop: C.c_int | None = None,
            stop_at_check: int | None = None):
        from .types import GBAResultView
        if stop_at_check is not None:
            self.set_stop_at_check(stop_at_check)
        n = len(problem.kfs), len(problem.pts)
        tcw = np.zeros((max(n[0], 1), 16), np.float32)
        pos = np.zeros((max(n[1], 1), 3), np.float32)
        inc = np.zeros(max(n[1], 1), np.uint8)
        r = GBAResultView(tcw.ctypes.data, pos.ctypes.data, inc.ctypes.data)
        v = problem.view()
        check("orbmi_bundle_adjustment",
              lib().orbmi_bundle_adjustment(self._h, C.addressof(v), int(iterations), int(bool(robust)), C.addressof(r),
                                            C.addressof(stop) if stop is not None else None))
        return {"tcw": tcw[:n[0]].reshape(-1, 4, 4), "pos": pos[:n[1]], "included": inc[:n[1]].astype(bool),
                "iterations": r.iterations, "trials": np.array(r.trials[:int(iterations)], np.int32),
                "chi2_initial": r.chi2_initial, "chi2": r.chi2, "stop_check": r.stop_check, "checks": r.checks,
                "status": r.status, "n_free": r.n_free, "n_blocks": r.n_blocks, "phase_ms": tuple(r.phase_ms)}


def _ba_keyframes(kfs, fixed):
    """BA_KF_DTYPE records of keyframes; fixed(i, keyframe) -> bool."""
    K = np.zeros(len(kfs), BA_KF_DTYPE)
    for i, k in enumerate(kfs):
        K[i]["tcw"] = np.asarray(k.tcw, np.float32).reshape(-1)
        K[i]["id"] = k.id
        K[i]["fixed"] = 1 if fixed(i, k) else 0
        K[i]["fx"], K[i]["fy"], K[i]["cx"], K[i]["cy"], K[i]["bf"] = k.cam.fx, k.cam.fy, k.cam.cx, k.cam.cy, k.cam.bf
    return K


def _ba_points_edges(mps, kfs):
    """BA_PT_DTYPE records of points and the BA_EDGE_DTYPE rows of their observations: per point in
    ascending keyframe id, bad keyframes and keyframes outside `kfs` skipped."""
    kidx = {id(k): i for i, k in enumerate(kfs)}
    P = np.zeros(len(mps), BA_PT_DTYPE)
    if mps:
        P["pos"] = np.array([mp.pos for mp in mps], np.float32).reshape(-1, 3)
        P["id"] = [mp.id for mp in mps]
        P["bad"] = [int(mp.bad) for mp in mps]
    e_pt, e_kf, e_kp = [], [], []
    for pi, mp in enumerate(mps):
        for kf in sorted(mp.observations, key=lambda k: k.id):
            ki = kidx.get(id(kf))
            if kf.bad or ki is None:
                continue
            e_pt.append(pi)
            e_kf.append(ki)
            e_kp.append(mp.observations[kf])
    E = np.zeros(len(e_pt), BA_EDGE_DTYPE)
    if e_pt:
        E["point"], E["kf"] = e_pt, e_kf
        e_kf, e_kp = np.asarray(e_kf), np.asarray(e_kp)
        for ki in np.unique(e_kf):   # one gather per keyframe
            sel = e_kf == ki
            k, j = kfs[ki], e_kp[sel]
            kp = k.keys_un[j]
            E["u"][sel] = kp["x"]
            E["v"][sel] = kp["y"]
            E["ur"][sel] = np.asarray(k.u_right, np.float32)[j]
            E[E.dtype.names[5]][sel] = np.asarray(k.inv_level_sigma2, np.float32)[kp["octave"]]
    return P, E


def gather_global_ba(keyframes, map_points):
    """The graph of Optimizer::BundleAdjustment (src/Optimizer.cc:78-200) over the minimal map
    model: every keyframe and point that is not bad, one edge per observation in ascending keyframe
    id (the build's replacement of pointer order), observations of bad keyframes and of keyframes
    outside `keyframes` skipped, fixed = (id == 0).  A point left without an edge stays in the
    arrays and comes back with included = 0.  -> (BAProblem, keyframes kept, points kept)."""
    kfs = [k for k in keyframes if not k.bad]
    mps = [mp for mp in map_points if not mp.bad]
    K = _ba_keyframes(kfs, lambda i, k: k.id == 0)
    P, E = _ba_points_edges(mps, kfs)
    return BAProblem(K, P, E), kfs, mps


class PoseOptimizer:
    """Optimizer::PoseOptimization(Frame*) (include/Optimizer.h:58) on the GPU, batched: one
    workgroup per frame.  `run(frames, obs)` updates the POSE_FRAME_DTYPE records in place
    (tcw, inliers = the reference's return value, iterations) and returns mvbOutlier per obs."""

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        check("orbmi_pose_create", lib().orbmi_pose_create(device, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().orbmi_pose_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, frames: np.ndarray, obs: np.ndarray) -> np.ndarray:
        from .types import POSE_FRAME_DTYPE, POSE_OBS_DTYPE
        assert frames.dtype == POSE_FRAME_DTYPE and obs.dtype == POSE_OBS_DTYPE
        assert frames.flags.c_contiguous and obs.flags.c_contiguous
        out = np.zeros(len(obs), np.uint8)
        check("orbmi_pose_optimization",
              lib().orbmi_pose_optimization(self._h, frames.ctypes.data, len(frames), obs.ctypes.data, len(obs),
                                            out.ctypes.data))
        return out.astype(bool)

    def run_device(self, frames_ptr: int, nframes: int, obs_ptr: int, nobs: int, outlier_ptr: int):
        """Device-resident frames / observations / flags: enqueued on the handle's stream."""
        check("orbmi_pose_optimization",
              lib().orbmi_pose_optimization(self._h, frames_ptr, nframes, obs_ptr, nobs, outlier_ptr))

    def synchronize(self):
        check("orbmi_pose_synchronize", lib().orbmi_pose_synchronize(self._h))

    def share_stream(self, extractor_handle):
        check("orbmi_pose_share_stream", lib().orbmi_pose_share_stream(self._h, extractor_handle))

    def PoseOptimization(self, view, inv_level_sigma2: np.ndarray, mappoints, rec, outlier):
        """Optimizer::PoseOptimization(Frame*) with its edge assembly: `view` = FrameView
        (initial tcw), `mappoints` = FrameMapPoints, rec = POSE_FRAME_DTYPE record (numpy, or a
        device address), outlier = per-keypoint mvbOutlier (numpy u8, or a device address).
        Returns the inlier count for host records, None when enqueued on the device."""
        sig = np.ascontiguousarray(inv_level_sigma2, np.float32)
        host = isinstance(rec, np.ndarray)
        rp = rec.ctypes.data if host else rec
        op = outlier.ctypes.data if isinstance(outlier, np.ndarray) else outlier
        check("orbmi_pose_optimization_frame",
              lib().orbmi_pose_optimization_frame(self._h, C.addressof(view), sig.ctypes.data, C.addressof(mappoints),
                                                  rp, op))
        return int(np.asarray(rec["inliers"]).reshape(-1)[0]) if host else None

    def PoseOptimizationTrack(self, view, inv_level_sigma2: np.ndarray, mappoints, rec: int, outlier: int, stage: int,
                              occupied_out, counts: int):
        """PoseOptimization followed by Tracking's pass over mvpMapPoints (orbmi_track_update_matches
        `stage`: 0 = TrackWithMotionModel's outlier discard, 1 = TrackLocalMap's statistics) in one
        launch; every address is device memory, enqueued on the handle's stream."""
        sig = np.ascontiguousarray(inv_level_sigma2, np.float32)
        check("orbmi_pose_optimization_frame_track",
              lib().orbmi_pose_optimization_frame_track(self._h, C.addressof(view), sig.ctypes.data,
                                                        C.addressof(mappoints), rec, outlier, int(stage),
                                                        occupied_out, counts))


# ---- minimal map model for the graph assembly (src/Optimizer.cc:486-534) ------------------
@dataclasses.dataclass(eq=False)
class KeyFrame:
    id: int
    tcw: np.ndarray                     # 4x4 float32
    keys_un: np.ndarray                 # KP_DTYPE
    u_right: np.ndarray                 # float32 (-1 = mono)
    inv_level_sigma2: np.ndarray        # mvInvLevelSigma2
    cam: object
    map_points: list = dataclasses.field(default_factory=list)   # MapPoint or None per keypoint
    covisible: list = dataclasses.field(default_factory=list)    # GetVectorCovisibleKeyFrames order
    bad: bool = False
    tcw_gba: np.ndarray = None          # mTcwGBA (loop.global_bundle_adjustment)
    ba_global_for_kf: int = 0           # mnBAGlobalForKF


@dataclasses.dataclass(eq=False)
class MapPoint:
    id: int
    pos: np.ndarray
    observations: dict = dataclasses.field(default_factory=dict)  # KeyFrame -> keypoint index
    bad: bool = False
    pos_gba: np.ndarray = None          # mPosGBA
    ba_global_for_kf: int = 0           # mnBAGlobalForKF


def gather_local_ba(pKF: KeyFrame):
    """Assemble the LocalBundleAdjustment graph around pKF exactly like the reference
    (local KFs, local MPs in first-seen order, fixed cameras, edges per observation in KF-id
    order -- the build's deterministic replacement of std::map<KeyFrame*> pointer order)."""
    local_kfs = [pKF] + [k for k in pKF.covisible if not k.bad]
    local_set = {id(k) for k in [pKF] + pKF.covisible}
    local_mps, seen = [], set()
    for kf in local_kfs:
        for mp in kf.map_points:
            if mp is not None and not mp.bad and id(mp) not in seen:
                seen.add(id(mp))
                local_mps.append(mp)
    fixed, fixed_set = [], set()
    for mp in local_mps:
        for kf in sorted(mp.observations, key=lambda k: k.id):
            if id(kf) not in local_set and id(kf) not in fixed_set:
                fixed_set.add(id(kf))
                if not kf.bad:
                    fixed.append(kf)
    kfs = local_kfs + fixed
    K = _ba_keyframes(kfs, lambda i, k: i >= len(local_kfs) or k.id == 0)
    P, E = _ba_points_edges(local_mps, kfs)
    return BAProblem(K, P, E), kfs, local_mps


class Sim3OptProblem(C.Structure):
    """orbmi_sim3_opt_problem (include/orbmi.h)."""
    _fields_ = [("n", C.c_int32), ("x3d_c1", C.c_void_p), ("x3d_c2", C.c_void_p), ("obs1", C.c_void_p),
                ("obs2", C.c_void_p), ("inv_sigma2_1", C.c_void_p), ("inv_sigma2_2", C.c_void_p),
                ("k1", C.c_float * 4), ("k2", C.c_float * 4), ("th2", C.c_float), ("fix_scale", C.c_int32),
                ("R12", C.c_float * 9), ("t12", C.c_float * 3), ("s12", C.c_float)]


class Sim3OptResult(C.Structure):
    """orbmi_sim3_opt_result (include/orbmi.h)."""
    _fields_ = [("q", C.c_double * 4), ("t", C.c_double * 3), ("s", C.c_double), ("sR", C.c_float * 9),
                ("t_f", C.c_float * 3), ("n_in", C.c_int32), ("n_bad", C.c_int32), ("iterations", C.c_int32 * 2),
                ("inlier", C.c_void_p), ("chi2", C.c_void_p)]


def sim3_opt_problem(x3d_c1, x3d_c2, obs1, obs2, inv_sigma2_1, inv_sigma2_2, k1, k2, th2, fix_scale, R12, t12, s12) -> dict:
    """One OptimizeSim3 problem as the arrays orbmi_sim3_opt_problem points to."""
    f = np.float32
    return {"x1": np.ascontiguousarray(x3d_c1, f).reshape(-1, 3), "x2": np.ascontiguousarray(x3d_c2, f).reshape(-1, 3),
            "o1": np.ascontiguousarray(obs1, f).reshape(-1, 2), "o2": np.ascontiguousarray(obs2, f).reshape(-1, 2),
            "w1": np.ascontiguousarray(inv_sigma2_1, f).reshape(-1), "w2": np.ascontiguousarray(inv_sigma2_2, f).reshape(-1),
            "k1": np.ascontiguousarray(k1, f).reshape(4), "k2": np.ascontiguousarray(k2, f).reshape(4),
            "th2": float(f(th2)), "fix_scale": int(bool(fix_scale)), "R12": np.ascontiguousarray(R12, f).reshape(9),
            "t12": np.ascontiguousarray(t12, f).reshape(3), "s12": float(f(s12))}


def _inv_level_sigma2(scale_factors):
    """mvInvLevelSigma2 (src/ORBextractor.cc:422-436): 1.0f / (scale * scale), float32."""
    s = np.asarray(scale_factors, np.float32)
    return (np.float32(1.0) / (s * s).astype(np.float32)).astype(np.float32)


class Sim3Optimizer:
    """Optimizer::OptimizeSim3 (src/Optimizer.cc:1145-1347) on the GPU, batched: one workgroup per
    problem, every (candidate, hypothesis) pair of LoopClosing::ComputeSim3 in one launch.
    matcher: an ORBmatcher whose handle, stream and staging arena are used."""

    def __init__(self, matcher=None, device: int = 0):
        from .matcher import ORBmatcher
        self._own = matcher is None
        self.matcher = ORBmatcher(device=device) if matcher is None else matcher
        self.last = None

    def close(self):
        if self._own and self.matcher is not None:
            self.matcher.close()
        self.matcher = None

    @staticmethod
    def _fill(P, p):
        n = len(p["x1"])
        if any(len(p[k]) != n for k in ("x2", "o1", "o2", "w1", "w2")):
            raise ValueError("sim3 optimisation arrays differ in length")
        P.n = n
        for name, key in (("x3d_c1", "x1"), ("x3d_c2", "x2"), ("obs1", "o1"), ("obs2", "o2"), ("inv_sigma2_1", "w1"),
                          ("inv_sigma2_2", "w2")):
            setattr(P, name, p[key].ctypes.data if n else None)
        P.k1, P.k2 = (C.c_float * 4)(*p["k1"]), (C.c_float * 4)(*p["k2"])
        P.th2, P.fix_scale = p["th2"], p["fix_scale"]
        P.R12, P.t12, P.s12 = (C.c_float * 9)(*p["R12"]), (C.c_float * 3)(*p["t12"]), p["s12"]
        return n

    def run(self, problems: list) -> list:
        """problems: dicts of sim3_opt_problem().  -> per problem {"q" (x y z w), "t", "s" (doubles),
        "sR" (3x3), "t_f" (float32, as Converter::toCvMat rounds them), "n_in", "n_bad", "iterations",
        "inlier" (n, 0 where the reference nulls the match), "chi2" (n, 2)}."""
        m = len(problems)
        P, R = (Sim3OptProblem * max(m, 1))(), (Sim3OptResult * max(m, 1))()
        bufs = []
        for k, p in enumerate(problems):
            n = self._fill(P[k], p)
            b = (np.zeros(max(n, 1), np.uint8), np.zeros((max(n, 1), 2), np.float64))
            bufs.append(b)
            R[k].inlier, R[k].chi2 = b[0].ctypes.data, b[1].ctypes.data
        check("orbmi_optimize_sim3_batch", lib().orbmi_optimize_sim3_batch(self.matcher._h, m, P if m else None, R if m else None))
        out = []
        for k, p in enumerate(problems):
            n = len(p["x1"])
            out.append({"q": np.array(R[k].q), "t": np.array(R[k].t), "s": float(R[k].s),
                        "sR": np.array(R[k].sR, np.float32).reshape(3, 3), "t_f": np.array(R[k].t_f, np.float32),
                        "n_in": R[k].n_in, "n_bad": R[k].n_bad, "iterations": tuple(R[k].iterations),
                        "inlier": bufs[k][0][:n], "chi2": bufs[k][1][:n]})
        return out

    def linearize(self, p: dict):
        """One buildSystem pass at the initial estimate (orbmi_debug_sim3_opt_linearize): H (7x7),
        b (7), the robust chi2."""
        P = Sim3OptProblem()
        self._fill(P, p)
        H, b, c = np.zeros((7, 7)), np.zeros(7), C.c_double()
        check("orbmi_debug_sim3_opt_linearize",
              lib().orbmi_debug_sim3_opt_linearize(self.matcher._h, C.addressof(P), H.ctypes.data, b.ctypes.data, C.byref(c)))
        return H, b, c.value

    @staticmethod
    def assemble(kf1, kf2, mps1, mps2, matches1, R12, t12, s12, th2, fix_scale, has_mp1=None):
        """The reference's assembly loop (:1198-1281) -> (problem dict, vnIndexEdge).  kf1 / kf2:
        types.Frame; mps1 / mps2: orbmi_mappoint records per keypoint slot; matches1[i] = the KF2
        slot of vpMatches1[i] (GetIndexInKeyFrame(pKF2)), -1 for a null match, -2 for a point
        without an index in KF2.  Skipped: a null match, a null or bad pMP1, a bad pMP2, i2 < 0."""
        from .sim3 import _to_camera
        from .types import MP_BAD
        m1 = np.asarray(matches1, np.int64)
        has1 = np.ones(len(mps1), bool) if has_mp1 is None else np.asarray(has_mp1, bool)
        keep = []
        for i in range(len(m1)):
            i2 = int(m1[i])
            if i2 == -1:  # !vpMatches1[i]
                continue
            if i >= len(mps1) or not has1[i]:  # !pMP1
                continue
            if i2 < 0 or i2 >= len(mps2):  # i2 < 0
                continue
            if (mps1["flags"][i] & MP_BAD) or (mps2["flags"][i2] & MP_BAD):
                continue
            keep.append((i, i2))
        keep = np.array(keep, np.int64).reshape(-1, 2)
        i1, i2 = keep[:, 0], keep[:, 1]
        p = sim3_opt_problem(
            _to_camera(kf1.tcw, mps1["pos"][i1]), _to_camera(kf2.tcw, mps2["pos"][i2]),
            np.stack([kf1.keys["x"][i1], kf1.keys["y"][i1]], -1), np.stack([kf2.keys["x"][i2], kf2.keys["y"][i2]], -1),
            _inv_level_sigma2(kf1.scale_factors)[kf1.keys["octave"][i1]],
            _inv_level_sigma2(kf2.scale_factors)[kf2.keys["octave"][i2]],
            [kf1.cam.fx, kf1.cam.fy, kf1.cam.cx, kf1.cam.cy], [kf2.cam.fx, kf2.cam.fy, kf2.cam.cx, kf2.cam.cy],
            th2, fix_scale, R12, t12, s12)
        return p, i1.astype(np.int64)

    def OptimizeSim3(self, kf1, kf2, mps1, mps2, matches1, R12, t12, s12, th2, fix_scale, has_mp1=None) -> int:
        """Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale): nulls matches1
        (an integer array, -1 = null) in place where the reference nulls vpMatches1 and returns nIn.
        The refined g2oS12 and the other outputs of run() are left in self.last."""
        p, idx = self.assemble(kf1, kf2, mps1, mps2, matches1, R12, t12, s12, th2, fix_scale, has_mp1)
        r = self.run([p])[0]
        matches1[idx[r["inlier"] == 0]] = -1
        self.last = r
        return r["n_in"]


class EssGraphProblem(C.Structure):
    """orbmi_essgraph_problem (include/orbmi.h)."""
    _fields_ = [("n_vertices", C.c_int32), ("vertices", C.c_void_p), ("fixed", C.c_int32), ("n_edges", C.c_int32),
                ("v0", C.c_void_p), ("v1", C.c_void_p), ("measurements", C.c_void_p), ("fix_scale", C.c_int32),
                ("iterations", C.c_int32), ("profile", C.c_int32)]


class EssGraphResult(C.Structure):
    """orbmi_essgraph_result (include/orbmi.h)."""
    _fields_ = [("vertices", C.c_void_p), ("chi2_before", C.c_double), ("chi2_after", C.c_double), ("iterations", C.c_int32),
                ("status", C.c_int32), ("trials", C.c_int32 * 32), ("phase_ms", C.c_float * 4)]


EG_TERMINATE, EG_SOLVE_FAILED, EG_REJECTED = 1, 2, 4


class EssentialGraphOptimizer:
    """optimizer.optimize(20) of Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:829-1118) on the
    GPU over arrays: vertices (n, 8) Sim3 as q (x y z w), t, s; edges as vertex indices v0 / v1 and
    measurements (E, 8).  matcher: an ORBmatcher whose handle, stream and staging arena are used."""

    def __init__(self, matcher=None, device: int = 0):
        from .matcher import ORBmatcher
        self._own = matcher is None
        self.matcher = ORBmatcher(device=device) if matcher is None else matcher

    def close(self):
        if self._own and self.matcher is not None:
            self.matcher.close()
        self.matcher = None

    @staticmethod
    def _problem(vertices, fixed, v0, v1, meas, fix_scale, iterations, profile=False):
        keep = (np.ascontiguousarray(vertices, np.float64).reshape(-1, 8), np.ascontiguousarray(v0, np.int32).reshape(-1),
                np.ascontiguousarray(v1, np.int32).reshape(-1), np.ascontiguousarray(meas, np.float64).reshape(-1, 8))
        if not (len(keep[1]) == len(keep[2]) == len(keep[3])):
            raise ValueError("essential-graph edge arrays differ in length")
        P = EssGraphProblem()
        P.n_vertices, P.vertices, P.fixed = len(keep[0]), keep[0].ctypes.data if len(keep[0]) else None, int(fixed)
        ne = len(keep[1])
        P.n_edges = ne
        P.v0, P.v1, P.measurements = (keep[1].ctypes.data, keep[2].ctypes.data, keep[3].ctypes.data) if ne else (None, None, None)
        P.fix_scale, P.iterations, P.profile = int(bool(fix_scale)), int(iterations), int(bool(profile))
        return P, keep

    def run(self, vertices, fixed, v0, v1, meas, fix_scale, iterations=20, profile=False) -> dict:
        """-> {"vertices" (n, 8), "chi2_before", "chi2_after", "iterations", "trials" (per iteration),
        "status" (EG_* or'ed), "phase_ms" (linearise, assemble, factor + solve, update; profile only)}."""
        P, keep = self._problem(vertices, fixed, v0, v1, meas, fix_scale, iterations, profile)
        out = np.zeros((max(len(keep[0]), 1), 8), np.float64)
        R = EssGraphResult()
        R.vertices = out.ctypes.data
        check("orbmi_optimize_essential_graph",
              lib().orbmi_optimize_essential_graph(self.matcher._h, C.addressof(P), C.addressof(R)))
        return {"vertices": out[:len(keep[0])], "chi2_before": float(R.chi2_before), "chi2_after": float(R.chi2_after),
                "iterations": int(R.iterations), "trials": [int(t) for t in R.trials[:R.iterations]], "status": int(R.status),
                "phase_ms": [float(t) for t in R.phase_ms]}

    def linearize(self, vertices, fixed, v0, v1, meas, fix_scale) -> dict:
        """One buildSystem pass at the given estimates (orbmi_debug_essgraph_linearize), in the
        library's block storage: {"vert_of", "col_ptr", "row_of", "Hd" (nf, 7, 7), "Ho" (nl, 7, 7),
        "b" (nf, 7), "chi2"}; `dense()` below spreads it over the free vertices."""
        P, keep = self._problem(vertices, fixed, v0, v1, meas, fix_scale, 0)
        dims = np.zeros(2, np.int32)
        f = lib().orbmi_debug_essgraph_linearize
        check("orbmi_debug_essgraph_linearize", f(self.matcher._h, C.addressof(P), dims.ctypes.data, None, None, None, None, None, None, None))
        nf, nl = int(dims[0]), int(dims[1])
        vert_of, col_ptr, row_of = np.zeros(max(nf, 1), np.int32), np.zeros(nf + 1, np.int32), np.zeros(max(nl, 1), np.int32)
        Hd, Ho, b, c = np.zeros((max(nf, 1), 7, 7)), np.zeros((max(nl, 1), 7, 7)), np.zeros((max(nf, 1), 7)), C.c_double()
        check("orbmi_debug_essgraph_linearize",
              f(self.matcher._h, C.addressof(P), dims.ctypes.data, vert_of.ctypes.data, col_ptr.ctypes.data, row_of.ctypes.data,
                Hd.ctypes.data, Ho.ctypes.data, b.ctypes.data, C.byref(c)))
        return {"vert_of": vert_of[:nf], "col_ptr": col_ptr, "row_of": row_of[:nl], "Hd": Hd[:nf], "Ho": Ho[:nl], "b": b[:nf],
                "chi2": float(c.value)}

    @staticmethod
    def dense(lin: dict):
        """The block storage of linearize() as (free vertices ascending, dense H, b)."""
        free = np.sort(lin["vert_of"])
        pos = {int(v): k for k, v in enumerate(free)}
        n = 7 * len(free)
        H, b = np.zeros((n, n)), np.zeros(n)
        for c, v in enumerate(lin["vert_of"]):
            p = pos[int(v)]
            H[7 * p:7 * p + 7, 7 * p:7 * p + 7] = lin["Hd"][c]
            b[7 * p:7 * p + 7] = lin["b"][c]
            for a in range(lin["col_ptr"][c], lin["col_ptr"][c + 1]):
                q = pos[int(lin["vert_of"][lin["row_of"][a]])]
                H[7 * q:7 * q + 7, 7 * p:7 * p + 7] = lin["Ho"][a]
                H[7 * p:7 * p + 7, 7 * q:7 * q + 7] = lin["Ho"][a].T
        return free, H, b

    def correct_points_sim3(self, points, ref_index, Srw, Swr_corrected, poses):
        """orbmi_correct_points_sim3: (corrected points (n, 3) float32, Tcw (k, 4, 4) float32 of poses)."""
        P = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        r = np.ascontiguousarray(ref_index, np.int32).reshape(-1)
        A = np.ascontiguousarray(Srw, np.float64).reshape(-1, 8)
        B = np.ascontiguousarray(Swr_corrected, np.float64).reshape(-1, 8)
        S = np.ascontiguousarray(poses, np.float64).reshape(-1, 8)
        if len(r) != len(P) or len(A) != len(B):
            raise ValueError("point correction arrays differ in length")
        out, T = np.zeros((max(len(P), 1), 3), np.float32), np.zeros((max(len(S), 1), 4, 4), np.float32)
        check("orbmi_correct_points_sim3",
              lib().orbmi_correct_points_sim3(self.matcher._h, len(P), P.ctypes.data if len(P) else None, r.ctypes.data if len(P) else None,
                                              len(A), A.ctypes.data if len(A) else None, B.ctypes.data if len(B) else None,
                                              out.ctypes.data, len(S), S.ctypes.data if len(S) else None, T.ctypes.data))
        return out[:len(P)], T[:len(S)]
