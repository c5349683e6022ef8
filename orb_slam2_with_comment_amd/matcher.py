"""Python mirror of ORB_SLAM2::ORBmatcher (include/ORBmatcher.h:37-102) over the C ABI.

The map/frame state crosses the boundary as flat arrays (types.py): keypoints, descriptors,
mvuRight and the pose of a Frame; MapPoint state as orbmi_mappoint records.  Results are the
reference's side effects as index arrays (see include/orbmi.h for the codes)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._capi import check, lib
from .types import TRACK_DTYPE, FrameView


class ORBmatcher:
    TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30  # src/ORBmatcher.cc:37-39

    def __init__(self, nnratio: float = 0.6, checkOri: bool = True, device: int = 0):
        h = C.c_void_p()
        check("orbmi_matcher_create", lib().orbmi_matcher_create(device, C.byref(h)))
        self._h = h
        self.mfNNratio = nnratio
        self.mbCheckOrientation = checkOri

    def close(self):
        if getattr(self, "_h", None):
            lib().orbmi_matcher_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def IsInFrustum(self, frame, mps, viewing_cos_limit=0.5):
        """Frame::isInFrustum over all points (src/Frame.cc:274-342)."""
        mps = np.ascontiguousarray(mps)
        tr = np.zeros(max(len(mps), 1), TRACK_DTYPE)
        v = frame.view()
        check("orbmi_is_in_frustum", lib().orbmi_is_in_frustum(self._h, C.addressof(v), mps.ctypes.data, len(mps),
                                                               viewing_cos_limit, tr.ctypes.data))
        return tr[:len(mps)]

    def SearchByProjection(self, frame, occupied, mps, track, th=3.0):
        """SearchByProjection(Frame&, vector<MapPoint*>, th) (src/ORBmatcher.cc:59-155)."""
        occ = np.ascontiguousarray(occupied, np.uint8)
        mps = np.ascontiguousarray(mps)
        track = np.ascontiguousarray(track)
        out = np.zeros(max(len(frame.keys), 1), np.int32)
        n = C.c_int()
        v = frame.view()
        check("orbmi_search_by_projection_local",
              lib().orbmi_search_by_projection_local(self._h, C.addressof(v), occ.ctypes.data, mps.ctypes.data,
                                                     track.ctypes.data, len(mps), th, self.mfNNratio,
                                                     out.ctypes.data, C.byref(n)))
        return out[:len(frame.keys)], n.value

    def SearchLocalPoints(self, frame, occupied, mps, th=1.0):
        """Tracking::SearchLocalPoints (src/Tracking.cc:1345-1403) fused on the GPU."""
        occ = np.ascontiguousarray(occupied, np.uint8)
        mps = np.ascontiguousarray(mps)
        out = np.zeros(max(len(frame.keys), 1), np.int32)
        n, ntm = C.c_int(), C.c_int()
        v = frame.view()
        check("orbmi_search_local_points",
              lib().orbmi_search_local_points(self._h, C.addressof(v), occ.ctypes.data, mps.ctypes.data, len(mps), th,
                                              out.ctypes.data, C.byref(n), C.byref(ntm)))
        return out[:len(frame.keys)], n.value, ntm.value

    def SearchByProjectionLastFrame(self, cf, occupied, lf, lf_points, th, bMono=False):
        """SearchByProjection(Frame& CF, const Frame& LF, th, bMono) (src/ORBmatcher.cc:1540-1695)."""
        occ = np.ascontiguousarray(occupied, np.uint8)
        lfp = np.ascontiguousarray(lf_points)
        out = np.zeros(max(len(cf.keys), 1), np.int32)
        n = C.c_int()
        vc, vl = cf.view(), lf.view()
        check("orbmi_search_by_projection_last_frame",
              lib().orbmi_search_by_projection_last_frame(self._h, C.addressof(vc), occ.ctypes.data, C.addressof(vl),
                                                          lfp.ctypes.data, th, int(bMono),
                                                          int(self.mbCheckOrientation), out.ctypes.data, C.byref(n)))
        return out[:len(cf.keys)], n.value

    def SearchForTriangulation(self, kf1, has_mp1, fv1, kf2, has_mp2, fv2, F12, bOnlyStereo=False):
        """SearchForTriangulation(KeyFrame*, KeyFrame*, cv::Mat F12, vector<pair<size_t,size_t>>&,
        bool) (src/ORBmatcher.cc:783-975): kf1 / kf2 are types.Frame (keys_un, u_right, desc, tcw),
        has_mp = GetMapPoint(i) != NULL, fv = mFeatVec.  Returns (match12, nmatches); the matched
        pairs are (i, match12[i]) for match12[i] >= 0."""
        m1 = np.ascontiguousarray(has_mp1, np.uint8)
        m2 = np.ascontiguousarray(has_mp2, np.uint8)
        F = np.ascontiguousarray(F12, np.float32).reshape(3, 3)
        out = np.zeros(max(len(kf1.keys), 1), np.int32)
        n = C.c_int()
        v1, v2, f1, f2 = kf1.view(), kf2.view(), fv1.view(), fv2.view()
        check("orbmi_search_for_triangulation", lib().orbmi_search_for_triangulation(
            self._h, C.addressof(v1), m1.ctypes.data, C.addressof(f1), C.addressof(v2), m2.ctypes.data,
            C.addressof(f2), F.ctypes.data, int(bOnlyStereo), int(self.mbCheckOrientation), out.ctypes.data,
            C.byref(n)))
        return out[:len(kf1.keys)], n.value

    def FuseSearch(self, kf, mps, in_kf=None, th=3.0):
        """The search of Fuse(KeyFrame*, const vector<MapPoint*>&, th) (src/ORBmatcher.cc:977-1127):
        -> (best_idx, best_dist, ncandidates); the Replace / AddObservation replay in list order
        is the caller's (include/orbmi.h)."""
        mps = np.ascontiguousarray(mps)
        n = len(mps)
        ink = None if in_kf is None else np.ascontiguousarray(in_kf, np.uint8)
        bi, bd = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        c = C.c_int()
        v = kf.view()
        check("orbmi_fuse_search", lib().orbmi_fuse_search(
            self._h, C.addressof(v), mps.ctypes.data if n else None, None if ink is None else ink.ctypes.data, n,
            th, bi.ctypes.data, bd.ctypes.data, C.byref(c)))
        return bi[:n], bd[:n], c.value

    def FuseSim3Search(self, kfs, Scws, mps, in_kf=None, th=4.0):
        """The search of Fuse(KeyFrame*, cv::Mat Scw, vpPoints, th, vpReplacePoint)
        (src/ORBmatcher.cc:1139-1269) for several keyframes in one launch: kfs are types.Frame,
        Scws one 3x4 or 4x4 float matrix [sRcw | t] per keyframe, mps the loop map points
        (orbmi_mappoint records), in_kf (nkf, n) IsInKeyFrame flags or None.
        -> (best_idx, best_dist) of shape (nkf, n) and nfused (nkf); the Replace / AddObservation
        replay in list order is the caller's (loop.fuse_sim3_replay)."""
        mps = np.ascontiguousarray(mps)
        nkf, n = len(kfs), len(mps)
        S = np.zeros((max(nkf, 1), 12), np.float32)
        if len(Scws) != nkf:
            raise ValueError("FuseSim3Search takes one Scw per keyframe")
        for k in range(nkf):
            S[k] = np.asarray(Scws[k], np.float32).reshape(-1, 4)[:3].reshape(12)
        ink = None
        if in_kf is not None:
            ink = np.ascontiguousarray(in_kf, np.uint8)
            if ink.size != nkf * n:
                raise ValueError("FuseSim3Search takes one in_kf flag per keyframe and point")
        bi = np.full(max(nkf * n, 1), -1, np.int32)
        bd = np.full(max(nkf * n, 1), 256, np.int32)
        nf = np.zeros(max(nkf, 1), np.int32)
        views = (FrameView * max(nkf, 1))()
        for k in range(nkf):
            views[k] = kfs[k].view()
        check("orbmi_fuse_sim3_search_batch", lib().orbmi_fuse_sim3_search_batch(
            self._h, nkf, C.addressof(views) if nkf else None, S.ctypes.data, mps.ctypes.data if n else None,
            None if ink is None or not ink.size else ink.ctypes.data, n, float(th), bi.ctypes.data, bd.ctypes.data,
            nf.ctypes.data))
        return bi[:nkf * n].reshape(nkf, n), bd[:nkf * n].reshape(nkf, n), nf[:nkf]

    def SearchBySim3(self, kf1, mps1, has_mp1, kf2, mps2, has_mp2, match12, s12, R12, t12, th=7.5):
        """SearchBySim3(KeyFrame*, KeyFrame*, vector<MapPoint*>& vpMatches12, s12, R12, t12, th)
        (src/ORBmatcher.cc:1285-1525): kf1 / kf2 are types.Frame, mps / has_mp one orbmi_mappoint
        and one flag per keypoint slot, match12 as include/orbmi.h codes it (-1 none, >= 0 the KF2
        slot, -2 a point without an index in KF2).  Returns (match12 with the new matches, nFound,
        vnMatch1, vnMatch2)."""
        n1, n2 = len(kf1.keys), len(kf2.keys)
        mps1, mps2 = np.ascontiguousarray(mps1), np.ascontiguousarray(mps2)
        h1, h2 = np.ascontiguousarray(has_mp1, np.uint8), np.ascontiguousarray(has_mp2, np.uint8)
        if len(mps1) != n1 or len(h1) != n1 or len(mps2) != n2 or len(h2) != n2 or len(match12) != n1:
            raise ValueError("SearchBySim3 takes one map point record, flag and match per keypoint slot")
        m12 = np.zeros(max(n1, 1), np.int32)
        m12[:n1] = match12
        R = np.ascontiguousarray(R12, np.float32).reshape(3, 3)
        t = np.ascontiguousarray(t12, np.float32).reshape(3)
        vn1, vn2 = np.zeros(max(n1, 1), np.int32), np.zeros(max(n2, 1), np.int32)
        n = C.c_int()
        v1, v2 = kf1.view(), kf2.view()
        check("orbmi_search_by_sim3", lib().orbmi_search_by_sim3(
            self._h, C.addressof(v1), mps1.ctypes.data if n1 else None, h1.ctypes.data if n1 else None,
            C.addressof(v2), mps2.ctypes.data if n2 else None, h2.ctypes.data if n2 else None, float(s12),
            R.ctypes.data, t.ctypes.data, th, m12.ctypes.data, C.byref(n), vn1.ctypes.data, vn2.ctypes.data))
        return m12[:n1], n.value, vn1[:n1], vn2[:n2]

    def SearchByProjectionSim3(self, kf, Scw, mps, matched, th=10):
        """SearchByProjection(KeyFrame*, cv::Mat Scw, vpPoints, vpMatched, th)
        (src/ORBmatcher.cc:359-479): kf is a types.Frame, Scw a 3x4 or 4x4 float matrix [sRcw | t],
        mps the candidate points (orbmi_mappoint records), matched one entry per keypoint slot of
        kf as include/orbmi.h codes vpMatched (-1 none, >= 0 the index in mps, -2 a point that is
        not in mps).  Returns (matched with the new matches, nmatches)."""
        nk = len(kf.keys)
        mps = np.ascontiguousarray(mps)
        if len(matched) != nk:
            raise ValueError("SearchByProjectionSim3 takes one match per keypoint slot")
        m = np.zeros(max(nk, 1), np.int32)
        m[:nk] = matched
        S = np.ascontiguousarray(np.asarray(Scw, np.float32).reshape(-1, 4)[:3])
        n = C.c_int()
        v = kf.view()
        check("orbmi_search_by_projection_sim3", lib().orbmi_search_by_projection_sim3(
            self._h, C.addressof(v), S.ctypes.data, mps.ctypes.data if len(mps) else None, len(mps),
            m.ctypes.data, float(th), C.byref(n)))
        return m[:nk], n.value

    def ComputeDistinctiveDescriptors(self, obs_desc: np.ndarray, obs_off: np.ndarray, desc_out=None):
        """MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:247-316) for a batch of map
        points: rows obs_off[p]..obs_off[p+1] of obs_desc are point p's observation descriptors.
        Returns (best row per point, -1 without observations; np x 32 mDescriptor)."""
        d = np.ascontiguousarray(obs_desc, np.uint8).reshape(-1, 32)
        off = np.ascontiguousarray(obs_off, np.int32)
        n = len(off) - 1
        best = np.zeros(max(n, 1), np.int32)
        out = np.zeros((max(n, 1), 32), np.uint8) if desc_out is None else np.ascontiguousarray(desc_out, np.uint8)
        check("orbmi_compute_distinctive_descriptors", lib().orbmi_compute_distinctive_descriptors(
            self._h, d.ctypes.data if len(d) else None, off.ctypes.data, n, best.ctypes.data, out.ctypes.data))
        return best[:n], out[:n]

    def SearchByBoW(self, kf, kf_mp_ok, kf_fv, f, f_fv):
        """SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&) (src/ORBmatcher.cc:211-344)."""
        ok = np.ascontiguousarray(kf_mp_ok, np.uint8)
        out = np.zeros(max(len(f.keys), 1), np.int32)
        n = C.c_int()
        vk, vf, fk, ff = kf.view(), f.view(), kf_fv.view(), f_fv.view()
        check("orbmi_search_by_bow",
              lib().orbmi_search_by_bow(self._h, C.addressof(vk), ok.ctypes.data, C.addressof(fk), C.addressof(vf),
                                        C.addressof(ff), self.mfNNratio, int(self.mbCheckOrientation),
                                        out.ctypes.data, C.byref(n)))
        return out[:len(f.keys)], n.value

    def SearchByBoWKF(self, kf1, ok1, fv1, kf2, ok2, fv2, nnratio=None, checkOri=None):
        """SearchByBoW(KeyFrame*, KeyFrame*, vector<MapPoint*>& vpMatches12)
        (src/ORBmatcher.cc:635-768): ok = the slot holds a map point that is not bad, fv = mFeatVec.
        Returns (match12, nmatches): match12[i1] = the KF2 keypoint matched to KF1 keypoint i1, -1
        for none -- the bow_matches row compute_sim3 takes.  nnratio / checkOri override the
        matcher's own (ComputeSim3 builds an ORBmatcher(0.75, true) for this call)."""
        n1, n2 = len(kf1.keys), len(kf2.keys)
        o1, o2 = np.ascontiguousarray(ok1, np.uint8), np.ascontiguousarray(ok2, np.uint8)
        if len(o1) != n1 or len(o2) != n2:
            raise ValueError("SearchByBoWKF takes one flag per keypoint slot")
        out = np.zeros(max(n1, 1), np.int32)
        n = C.c_int()
        v1, v2, f1, f2 = kf1.view(), kf2.view(), fv1.view(), fv2.view()
        check("orbmi_search_by_bow_kf", lib().orbmi_search_by_bow_kf(
            self._h, C.addressof(v1), o1.ctypes.data if n1 else None, C.addressof(f1), C.addressof(v2),
            o2.ctypes.data if n2 else None, C.addressof(f2), self.mfNNratio if nnratio is None else nnratio,
            int(self.mbCheckOrientation if checkOri is None else checkOri), out.ctypes.data, C.byref(n)))
        return out[:n1], n.value
