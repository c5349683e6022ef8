"""Loop detection: ORB_SLAM2::KeyFrameDatabase (src/KeyFrameDatabase.cc:33-197) on the device and
LoopClosing::DetectLoop (src/LoopClosing.cc:105-264) on top of it.

KeyFrameDatabase          orbmi_kfdb_*: the keyframes' BowVectors stored forward in one device
                          arena; a query intersects the query vector with every indexed slot.
LoopDetector              DetectLoop: the early add, minScore over the covisibles, the database
                          query and the covisibility-consistency groups.
detect_and_compute_sim3   DetectLoop, SearchByBoW(KF, KF) per enough-consistent candidate, then
                          sim3.compute_sim3: LoopClosing::Run up to CorrectLoop.

essential_graph_edges     the edge list of Optimizer::OptimizeEssentialGraph (host only).
propagate_corrected_sim3  CorrectLoop's pose propagation: CorrectedSim3 and NonCorrectedSim3.
optimize_essential_graph  the edge list, the device pose-graph Levenberg and the correction of
                          poses and map points: the arithmetic of LoopClosing::CorrectLoop.


fuse_sim3_replay          the map updates of ORBmatcher::Fuse(KF, Scw) in list order.
search_and_fuse           LoopClosing::SearchAndFuse: one batched search, the replay per keyframe.
loop_connections          the new covisibility links of CorrectLoop (LoopConnections).
current_matched_points    mvpCurrentMatchedPoints as objects, from compute_sim3's result.
correct_loop              LoopClosing::CorrectLoop on system.KeyFrame / system.MapPoint, from the
                          accepted Scw to the corrected poses and points.

global_bundle_adjustment      Optimizer::GlobalBundleAdjustemnt: the whole map's graph, the device
                              bundle adjustment and the write-back of src/Optimizer.cc:206-253.
run_global_bundle_adjustment  LoopClosing::RunGlobalBundleAdjustment: that, then the spanning-tree
                              propagation and the map points' carry-over.

For detection the covisibility graph stays the caller's: it comes in as callables (or mappings)
from a keyframe id to ids.  Monocular mode, DetectRelocalizationCandidates, the GBA thread and the
call from the SLAM loops are not here.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._capi import check, lib
from .sim3 import DeviceBackend, _quat_to_R, compute_sim3
from .types import MAPPOINT_DTYPE, MP_BAD, MP_HAS_OBS, Frame
from .vocabulary import L1_NORM


class KfdbQueryResult(C.Structure):
    """orbmi_kfdb_query_result (include/orbmi.h)."""
    _fields_ = [("n_slots", C.c_int32), ("max_common", C.c_int32), ("min_common", C.c_int32), ("kf_id", C.c_void_p),
                ("common", C.c_void_p), ("first_word", C.c_void_p), ("add_seq", C.c_void_p), ("score", C.c_void_p)]


def _fn(x):
    """A graph accessor given as a callable, or as a mapping / sequence indexed by keyframe id."""
    if callable(x):
        return x
    if hasattr(x, "get"):
        return lambda i: x.get(i, ())
    return lambda i: x[i] if 0 <= i < len(x) else ()


def _query_arrays(word, value):
    w = np.ascontiguousarray(word, np.uint32).reshape(-1)
    v = np.ascontiguousarray(value, np.float64).reshape(-1)
    if len(w) != len(v):
        raise ValueError("a BowVector takes one value per word")
    return w, v


def _ids(ids):
    return np.ascontiguousarray(list(ids) if not isinstance(ids, np.ndarray) else ids, np.int32).reshape(-1)


class KeyFrameDatabase:
    """Device KeyFrameDatabase.  A keyframe's mBowVec is stored once (store); add / erase are
    KeyFrameDatabase::add / erase and only switch its `indexed` flag; the vector stays for score()
    (DetectLoop scores covisibles that were erased or never added)."""

    def __init__(self, scoring: int = L1_NORM, max_keyframes: int = 4096, max_words_total: int | None = None,
                 device: int = 0):
        if max_words_total is None:
            max_words_total = max_keyframes * 2048
        h = C.c_void_p()
        check("orbmi_kfdb_create", lib().orbmi_kfdb_create(device, int(scoring), int(max_keyframes),
                                                           int(max_words_total), C.byref(h)))
        self._h = h
        self.max_keyframes = int(max_keyframes)
        self._stored = set()  # GetBestCovisibilityKeyFrames is tabulated over the stored ids

    def close(self):
        if getattr(self, "_h", None):
            lib().orbmi_kfdb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear(self):
        check("orbmi_kfdb_clear", lib().orbmi_kfdb_clear(self._h))
        self._stored = set()

    def store(self, kf_id: int, word, value):
        """pKF->mBowVec (host arrays, word ids strictly ascending)."""
        w, v = _query_arrays(word, value)
        check("orbmi_kfdb_store", lib().orbmi_kfdb_store(self._h, int(kf_id), w.ctypes.data if len(w) else None,
                                                         v.ctypes.data if len(w) else None, len(w)))
        self._stored.add(int(kf_id))

    def store_device(self, kf_id: int, d_word: int, d_value: int, n: int):
        """The same from device addresses (ORBVocabulary.transform_device's outputs, finished on
        the device: synchronize() the vocabulary first); n = the word count."""
        check("orbmi_kfdb_store", lib().orbmi_kfdb_store(self._h, int(kf_id), d_word, d_value, int(n)))
        self._stored.add(int(kf_id))

    def add(self, kf_id: int):
        check("orbmi_kfdb_add", lib().orbmi_kfdb_add(self._h, int(kf_id)))

    def erase(self, kf_id: int):
        check("orbmi_kfdb_erase", lib().orbmi_kfdb_erase(self._h, int(kf_id)))

    def score(self, word, value, kf_ids) -> np.ndarray:
        """mpVoc->score(query, mBowVec of each id) as doubles."""
        w, v = _query_arrays(word, value)
        ids = _ids(kf_ids)
        out = np.zeros(max(len(ids), 1), np.float64)
        check("orbmi_kfdb_score", lib().orbmi_kfdb_score(self._h, w.ctypes.data if len(w) else None,
                                                         v.ctypes.data if len(w) else None, len(w),
                                                         ids.ctypes.data if len(ids) else None, len(ids),
                                                         out.ctypes.data))
        return out[:len(ids)]

    def query(self, word, value, connected_ids=()) -> dict:
        """The per-slot half of DetectLoopCandidates (:76-139) -> {"kf_id", "common", "first_word",
        "add_seq", "score" (per slot), "max_common", "min_common"}."""
        w, v = _query_arrays(word, value)
        conn = _ids(connected_ids)
        n = self.max_keyframes
        a = {"kf_id": np.zeros(n, np.int32), "common": np.zeros(n, np.int32), "first_word": np.zeros(n, np.uint32),
             "add_seq": np.zeros(n, np.uint64), "score": np.zeros(n, np.float64)}
        r = KfdbQueryResult(0, 0, 0, *(a[k].ctypes.data for k in ("kf_id", "common", "first_word", "add_seq", "score")))
        check("orbmi_kfdb_query", lib().orbmi_kfdb_query(self._h, w.ctypes.data if len(w) else None,
                                                         v.ctypes.data if len(w) else None, len(w),
                                                         conn.ctypes.data if len(conn) else None, len(conn),
                                                         C.addressof(r)))
        out = {k: x[:r.n_slots] for k, x in a.items()}
        out.update(max_common=int(r.max_common), min_common=int(r.min_common))
        return out

    def DetectLoopCandidates(self, word, value, min_score: float, connected_ids=(), best_covis=()) -> list:
        """KeyFrameDatabase::DetectLoopCandidates(pKF, minScore): word / value = pKF->mBowVec,
        connected_ids = pKF->GetConnectedKeyFrames(), best_covis(id) = GetBestCovisibilityKeyFrames(10)
        of a stored keyframe.  -> vpLoopCandidates as keyframe ids, in the reference's order."""
        w, v = _query_arrays(word, value)
        conn = _ids(connected_ids)
        get = _fn(best_covis)
        nkf = max(self._stored) + 1 if self._stored else 0
        none = np.zeros(0, np.int32)
        rows = [_ids(get(i)) if i in self._stored else none for i in range(nkf)]
        off = np.zeros(nkf + 1, np.int32)
        if nkf:
            off[1:] = np.cumsum([len(r) for r in rows])
        ids = np.concatenate(rows).astype(np.int32) if nkf and off[-1] else np.zeros(1, np.int32)
        out = np.zeros(self.max_keyframes, np.int32)
        n = C.c_int()
        check("orbmi_detect_loop_candidates", lib().orbmi_detect_loop_candidates(
            self._h, w.ctypes.data if len(w) else None, v.ctypes.data if len(w) else None, len(w),
            C.c_float(np.float32(min_score)), conn.ctypes.data if len(conn) else None, len(conn), off.ctypes.data,
            ids.ctypes.data, nkf, out.ctypes.data, len(out), C.byref(n)))
        return [int(x) for x in out[:n.value]]


class LoopBackend(DeviceBackend):
    """compute_sim3's device operators plus the two DetectLoop needs: a KeyFrameDatabase and
    SearchByBoW(KF, KF).  A test drives LoopDetector / detect_and_compute_sim3 with an object of
    the same methods over the numpy restatement."""

    def __init__(self, db: KeyFrameDatabase | None = None, matcher=None, device: int = 0, **db_args):
        super().__init__(matcher, device)
        self._own_db = db is None
        self.db = KeyFrameDatabase(device=device, **db_args) if db is None else db

    def close(self):
        if self._own_db and self.db is not None:
            self.db.close()
        self.db = None
        if getattr(self, "_gba", None) is not None:
            self._gba.close()
            self._gba = None
        super().close()

    def search_by_bow_kf(self, cur, cand):
        """ORBmatcher matcher(0.75, true); matcher.SearchByBoW(mpCurrentKF, pKF, ...) (:299, :330)."""
        return self.matcher.SearchByBoWKF(cur["kf"], cur["ok"], cur["fv"], cand["kf"], cand["ok"], cand["fv"],
                                          nnratio=0.75, checkOri=True)

    # CorrectLoop's operators: the batched Fuse(KF, Scw) search, ComputeDistinctiveDescriptors and
    # the essential graph's three, all on this backend's matcher handle
    def fuse_sim3_search(self, kfs, Scws, mps, in_kf, th):
        return self.matcher.FuseSim3Search(kfs, Scws, mps, in_kf, th)

    def distinctive(self, obs_desc, obs_off):
        return self.matcher.ComputeDistinctiveDescriptors(obs_desc, obs_off)[1]

    def _essgraph(self):
        if getattr(self, "_eg", None) is None:
            self._eg = EssGraphBackend(matcher=self.matcher)
        return self._eg

    def essential_graph_edges(self, G):
        return self._essgraph().essential_graph_edges(G)

    def optimize_essential_graph(self, vertices, fixed, v0, v1, meas, fix_scale, iterations=20):
        return self._essgraph().optimize_essential_graph(vertices, fixed, v0, v1, meas, fix_scale, iterations)

    def correct_points_sim3(self, points, ref_index, Srw, Swr_corrected, poses):
        return self._essgraph().correct_points_sim3(points, ref_index, Srw, Swr_corrected, poses)

    def bundle_adjustment(self, problem, iterations=10, robust=False, stop=None, stop_at_check=None):
        """Optimizer::BundleAdjustment on the assembled graph (optimizer.GlobalBA.run)."""
        if getattr(self, "_gba", None) is None:
            from .optimizer import GlobalBA
            self._gba = GlobalBA()
        return self._gba.run(problem, iterations, robust, stop, -1 if stop_at_check is None else stop_at_check)


class LoopDetector:
    """LoopClosing::DetectLoop with its members.  db: a KeyFrameDatabase (or an object with its
    store / add / score / DetectLoopCandidates).  The graph: GetVectorCovisibleKeyFrames(id) (all
    covisibles, for minScore), GetConnectedKeyFrames(id) (the same set, for the query's exclusion
    and the consistency groups), GetBestCovisibilityKeyFrames(id) (the best 10, for the score
    accumulation), isBad(id); each a callable or a mapping by keyframe id."""

    def __init__(self, db, GetVectorCovisibleKeyFrames, GetConnectedKeyFrames, GetBestCovisibilityKeyFrames,
                 isBad=None, consistency_th: int = 3):
        self.db = db
        self.GetVectorCovisibleKeyFrames = _fn(GetVectorCovisibleKeyFrames)
        self.GetConnectedKeyFrames = _fn(GetConnectedKeyFrames)
        self.GetBestCovisibilityKeyFrames = _fn(GetBestCovisibilityKeyFrames)
        self.isBad = (lambda i: False) if isBad is None else _fn(isBad)
        self.mnCovisibilityConsistencyTh = consistency_th
        self.mLastLoopKFid = 0            # CorrectLoop would set it
        self.mvConsistentGroups = []      # [(set of ids, consistency)]
        self.mvpEnoughConsistentCandidates = []
        self.mlpLoopKeyFrameQueue = []
        self.mpCurrentKF = None
        self.mBowVec = {}                 # id -> (word, value): the queued keyframes' vectors
        self.last_candidates = []         # vpCandidateKFs of the last DetectLoop
        self.last_min_score = None

    def InsertKeyFrame(self, kf_id: int, word, value):
        """LoopClosing::InsertKeyFrame (:91-97): queue the keyframe; its mBowVec goes into the
        database's store (not indexed until DetectLoop adds it)."""
        w, v = _query_arrays(word, value)
        self.db.store(int(kf_id), w, v)
        self.mBowVec[int(kf_id)] = (w, v)
        if int(kf_id) != 0:  # :93
            self.mlpLoopKeyFrameQueue.append(int(kf_id))

    def CheckNewKeyFrames(self) -> bool:
        return bool(self.mlpLoopKeyFrameQueue)

    def DetectLoop(self) -> bool:
        cur = self.mpCurrentKF = self.mlpLoopKeyFrameQueue.pop(0)
        self.last_candidates, self.last_min_score = [], None
        if cur < self.mLastLoopKFid + 10:  # :116-121
            self.db.add(cur)
            return False
        w, v = self.mBowVec[cur]
        covis = [int(i) for i in self.GetVectorCovisibleKeyFrames(cur) if not self.isBad(int(i))]
        min_score = np.float32(1)
        if covis:  # :126-140, float score = mpORBVocabulary->score(...)
            for s in np.asarray(self.db.score(w, v, covis), np.float64).astype(np.float32):
                if s < min_score:
                    min_score = s
        self.last_min_score = min_score
        connected = [int(i) for i in self.GetConnectedKeyFrames(cur)]
        cands = self.db.DetectLoopCandidates(w, v, min_score, connected, self.GetBestCovisibilityKeyFrames)
        self.last_candidates = list(cands)
        if not cands:  # :147-153
            self.db.add(cur)
            self.mvConsistentGroups = []
            return False
        self.mvpEnoughConsistentCandidates = []
        current_groups = []
        consistent_group = [False] * len(self.mvConsistentGroups)
        for cand in cands:  # :173-240
            group = {int(i) for i in self.GetConnectedKeyFrames(cand)}
            group.add(cand)
            enough = False
            for_some = False
            for ig, (prev, nprev) in enumerate(self.mvConsistentGroups):
                if group & prev:
                    for_some = True
                    ncur = nprev + 1
                    if not consistent_group[ig]:
                        current_groups.append((group, ncur))
                        consistent_group[ig] = True
                    if ncur >= self.mnCovisibilityConsistencyTh and not enough:
                        self.mvpEnoughConsistentCandidates.append(cand)
                        enough = True
            if not for_some:
                current_groups.append((group, 0))
        self.mvConsistentGroups = current_groups
        self.db.add(cur)
        return bool(self.mvpEnoughConsistentCandidates)


def detect_and_compute_sim3(detector: LoopDetector, keyframes, loop_points_of, fix_scale, seed=0, backend=None):
    """One LoopClosing::Run iteration up to CorrectLoop (src/LoopClosing.cc:63-77): DetectLoop on
    the next queued keyframe, SearchByBoW(mpCurrentKF, pKF) for every enough-consistent candidate
    (:330; a candidate with fewer than 20 matches is discarded, :333-337), then compute_sim3.

    keyframes[id] -> {"kf": types.Frame, "mps", "has" (compute_sim3's), "ok": the slot holds a point
    that is not bad, "fv": mFeatVec, optionally "bad"}; loop_points_of(id) as compute_sim3's, by
    keyframe id; backend: a LoopBackend (or its restatement) whose db the detector uses.

    -> {"detected", "current", "candidates" (vpCandidateKFs), "consistent"
    (mvpEnoughConsistentCandidates), "bow_matches" (one row per consistent candidate), "sim3"
    (compute_sim3's result or None), "loop_kf" (the accepted candidate's id or None)}."""
    get = _fn(keyframes)
    detected = detector.DetectLoop()
    cur_id = detector.mpCurrentKF
    out = {"detected": detected, "current": cur_id, "candidates": list(detector.last_candidates),
           "consistent": list(detector.mvpEnoughConsistentCandidates) if detected else [], "bow_matches": [],
           "sim3": None, "loop_kf": None}
    if not detected:
        return out
    cur = get(cur_id)
    ids = out["consistent"]
    cands = [get(i) for i in ids]
    bow = []
    for c in cands:
        if c.get("bad", False):  # :324-328
            bow.append(np.full(len(cur["kf"].keys), -1, np.int32))
            continue
        bow.append(np.array(backend.search_by_bow_kf(cur, c)[0], np.int32))
    out["bow_matches"] = bow
    r = compute_sim3(cur, cands, bow, lambda i: loop_points_of(ids[i]), fix_scale, seed=seed, backend=backend)
    out["sim3"] = r
    if r["candidate"] is not None and r["accepted"]:
        out["loop_kf"] = ids[r["candidate"]]
    return out


# ---- LoopClosing::CorrectLoop: the essential graph -----------------------------------
# A Sim3 is 8 doubles: q (x y z w), t, s.  A graph is a dict over keyframe ids:
#   live (n_ids) bool, Tcw (n_ids, 4, 4) float32, parent (n_ids, -1: none),
#   loop_edges {id: [ids]}, covisibles {id: [ids]} (GetCovisiblesByWeight(100), in its order),
#   corrected / noncorrected {id: Sim3}, loop_connections {id: {id: weight}}, loop_id, cur_id

class EssGraphInput(C.Structure):
    """orbmi_essgraph_input (include/orbmi.h)."""
    _fields_ = [("n_ids", C.c_int32), ("live", C.c_void_p), ("Tcw", C.c_void_p), ("parent", C.c_void_p),
                ("loop_off", C.c_void_p), ("loop_ids", C.c_void_p), ("cov_off", C.c_void_p), ("cov_ids", C.c_void_p),
                ("n_corrected", C.c_int32), ("corrected_ids", C.c_void_p), ("corrected", C.c_void_p),
                ("n_noncorrected", C.c_int32), ("noncorrected_ids", C.c_void_p), ("noncorrected", C.c_void_p),
                ("lc_off", C.c_void_p), ("lc_ids", C.c_void_p), ("lc_weight", C.c_void_p), ("loop_id", C.c_int32),
                ("cur_id", C.c_int32)]


def _csr(rows, n, weights=False):
    off, ids, w = [0], [], []
    for i in range(n):
        row = rows.get(i, ())
        for j in row:
            ids.append(int(j))
            if weights:
                w.append(int(row[j]))
        off.append(len(ids))
    pad = [0] if not ids else []  # never a NULL array
    return np.array(off, np.int32), np.array(ids + pad, np.int32), np.array(w + pad, np.int32)


def _sim3_table(d):
    ids = np.array(sorted(d), np.int32)
    S = np.array([np.asarray(d[int(i)], np.float64).reshape(8) for i in ids], np.float64).reshape(-1, 8)
    return ids, S


def _sim3_from_float_pose(T, backend=None):
    """g2o::Sim3(Matrix3d, Vector3d, 1.0) of a float 4x4 pose, through the edge rule's vScw."""
    G = {"live": np.ones(1, bool), "Tcw": np.asarray(T, np.float32).reshape(1, 4, 4), "parent": np.full(1, -1, np.int32),
         "loop_edges": {}, "covisibles": {}, "corrected": {}, "noncorrected": {}, "loop_connections": {}, "loop_id": 0, "cur_id": 0}
    return essential_graph_edges(G, backend)[3][0]


def _device_edges(G):
    n = len(G["live"])
    live = np.ascontiguousarray(np.asarray(G["live"], bool).astype(np.uint8))
    Tcw = np.ascontiguousarray(G["Tcw"], np.float32).reshape(n, 16)
    parent = np.ascontiguousarray(G["parent"], np.int32)
    lo, li, _ = _csr(G["loop_edges"], n)
    co, ci, _ = _csr(G["covisibles"], n)
    xo, xi, xw = _csr(G["loop_connections"], n, True)
    cid, cs = _sim3_table(G["corrected"])
    nid, ns = _sim3_table(G["noncorrected"])
    I = EssGraphInput()
    I.n_ids, I.live, I.Tcw, I.parent = n, live.ctypes.data, Tcw.ctypes.data, parent.ctypes.data
    I.loop_off, I.loop_ids, I.cov_off, I.cov_ids = lo.ctypes.data, li.ctypes.data, co.ctypes.data, ci.ctypes.data
    I.n_corrected, I.n_noncorrected = len(cid), len(nid)
    if len(cid):
        I.corrected_ids, I.corrected = cid.ctypes.data, cs.ctypes.data
    if len(nid):
        I.noncorrected_ids, I.noncorrected = nid.ctypes.data, ns.ctypes.data
    I.lc_off, I.lc_ids, I.lc_weight = xo.ctypes.data, xi.ctypes.data, xw.ctypes.data
    I.loop_id, I.cur_id = int(G["loop_id"]), int(G["cur_id"])
    cap = int(live.sum()) + int(lo[-1]) + int(co[-1]) + int(xo[-1])
    v0, v1 = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32)
    meas, vScw, ne = np.zeros((max(cap, 1), 8)), np.zeros((n, 8)), C.c_int()
    check("orbmi_essential_graph_edges",
          lib().orbmi_essential_graph_edges(C.addressof(I), cap, v0.ctypes.data, v1.ctypes.data, meas.ctypes.data,
                                            vScw.ctypes.data, C.byref(ne)))
    return v0[:ne.value].copy(), v1[:ne.value].copy(), meas[:ne.value].copy(), vScw


class EssGraphBackend:
    """The library's operators behind essential_graph_edges / optimize_essential_graph.  A test
    drives both with an object of the same three methods over the numpy restatement."""

    def __init__(self, matcher=None, device: int = 0):
        from .optimizer import EssentialGraphOptimizer
        self.optimizer = EssentialGraphOptimizer(matcher, device)

    def close(self):
        self.optimizer.close()

    def essential_graph_edges(self, G):
        return _device_edges(G)

    def optimize_essential_graph(self, vertices, fixed, v0, v1, meas, fix_scale, iterations=20):
        return self.optimizer.run(vertices, fixed, v0, v1, meas, fix_scale, iterations)

    def correct_points_sim3(self, points, ref_index, Srw, Swr_corrected, poses):
        return self.optimizer.correct_points_sim3(points, ref_index, Srw, Swr_corrected, poses)


def essential_graph_edges(graph, backend=None):
    """The edge list of Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:862-1053), host only:
    -> (v0, v1 as keyframe ids, measurements (E, 8), vScw (n_ids, 8)).  Ascending keyframe id
    wherever the reference iterates in pointer order."""
    if backend is None:
        return _device_edges(graph)
    return backend.essential_graph_edges(graph)


def propagate_corrected_sim3(Tcw, cur_id, connected_ids, Scw, backend=None):
    """LoopClosing::CorrectLoop's pose propagation (src/LoopClosing.cc:546-581): for the current
    keyframe and every keyframe connected to it, Sic = Tiw * Twc as a Sim3 of scale 1 and
    CorrectedSiw = Sic * Scw; NonCorrectedSim3 = the poses as they are.  Tcw: (n_ids, 4, 4) float32;
    Scw: the accepted Sim3 (8) of the current keyframe.  Twc = [Rcw^T | -Rcw^T tcw] in float, the
    product Tiw * Twc with double accumulators rounded to float once (cv::gemm's for CV_32F).
    backend: as essential_graph_edges takes it (the Sim3 of a float pose comes from its vScw).
    -> (corrected {id: Sim3}, noncorrected {id: Sim3})."""
    Tcw = np.asarray(Tcw, np.float32)
    Scw = np.asarray(Scw, np.float64).reshape(8)
    Twc = np.eye(4, dtype=np.float32)
    Rwc = Tcw[cur_id, :3, :3].T
    t = Tcw[cur_id, :3, 3]
    Twc[:3, :3] = Rwc
    for r in range(3):
        Twc[r, 3] = -((Rwc[r, 0] * t[0] + Rwc[r, 1] * t[1]) + Rwc[r, 2] * t[2])
    corrected, nonc = {int(cur_id): Scw.copy()}, {}
    for i in [int(k) for k in connected_ids if int(k) != int(cur_id)] + [int(cur_id)]:
        Tiw = Tcw[i]
        if i != cur_id:
            A, B = Tiw.astype(np.float64), Twc.astype(np.float64)
            Tic = np.zeros((4, 4), np.float64)
            for r in range(4):
                for c in range(4):
                    Tic[r, c] = ((A[r, 0] * B[0, c] + A[r, 1] * B[1, c]) + A[r, 2] * B[2, c]) + A[r, 3] * B[3, c]
            corrected[i] = _sim3_mul(_sim3_from_float_pose(Tic.astype(np.float32), backend), Scw)
        nonc[i] = _sim3_from_float_pose(Tiw, backend)
    return corrected, nonc


def _sim3_rotate(q, v):
    """Eigen's quaternion * vector, one rounding per operation in csrc/sim3_opt.h's order."""
    q = [np.float64(c) for c in q]
    v = [np.float64(c) for c in v]
    ux, uy, uz = q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    cx, cy, cz = q[1] * uz - q[2] * uy, q[2] * ux - q[0] * uz, q[0] * uy - q[1] * ux
    return np.array([(v[0] + q[3] * ux) + cx, (v[1] + q[3] * uy) + cy, (v[2] + q[3] * uz) + cz], np.float64)


def _sim3_mul(a, b):
    """Sim3::operator* in csrc/sim3_opt.h's order."""
    a, b = [np.float64(c) for c in a], [np.float64(c) for c in b]
    q = [((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1], ((a[3] * b[1] + a[1] * b[3]) + a[2] * b[0]) - a[0] * b[2],
         ((a[3] * b[2] + a[2] * b[3]) + a[0] * b[1]) - a[1] * b[0], ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2]]
    t = a[7] * _sim3_rotate(a[:4], b[4:7]) + np.array(a[4:7], np.float64)
    return np.array(q + list(t) + [a[7] * b[7]], np.float64)


def _sim3_inverse(a):
    a = [np.float64(c) for c in a]
    qc = [-a[0], -a[1], -a[2], a[3]]
    m = np.float64(-1.) / a[7]
    return np.array(qc + list(_sim3_rotate(qc, [m * a[4], m * a[5], m * a[6]])) + [np.float64(1.) / a[7]], np.float64)


def optimize_essential_graph(graph, fix_scale, points=None, point_ref=None, backend=None, iterations=20):
    """Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:829-1118) over a graph dict: the edge list,
    the Levenberg optimisation with the loop keyframe fixed, the SE3 poses [R | t / s] of every live
    keyframe and the correction of the map points.  points (n, 3) float32 with point_ref (n): the
    keyframe id each point is corrected through (mnCorrectedReference where CorrectLoop corrected it,
    else its reference keyframe).  UpdateNormalAndDepth and the map surgery stay the caller's.
    -> {"Tcw" (n_ids, 4, 4) float32 (live ids replaced), "vertices" (n_ids, 8), "points", "edges":
    (v0, v1, meas), "vScw", "chi2_before", "chi2_after", "iterations", "trials", "status"}."""
    own = backend is None
    be = EssGraphBackend() if own else backend
    try:
        v0, v1, meas, vScw = be.essential_graph_edges(graph)
        live = np.asarray(graph["live"], bool)
        ids = np.nonzero(live)[0]
        index = np.full(len(live), -1, np.int32)
        index[ids] = np.arange(len(ids), dtype=np.int32)
        r = be.optimize_essential_graph(vScw[ids], int(index[graph["loop_id"]]), index[v0], index[v1], meas, fix_scale, iterations)
        opt = np.asarray(r["vertices"], np.float64).reshape(-1, 8)
        Swc = np.array([_sim3_inverse(S) for S in opt], np.float64).reshape(-1, 8)  # vCorrectedSwc
        P = np.zeros((0, 3), np.float32) if points is None else np.asarray(points, np.float32).reshape(-1, 3)
        ref = np.zeros(0, np.int32) if points is None else index[np.asarray(point_ref, np.int64)]
        if len(ref) and (ref < 0).any():
            raise ValueError("a point's reference keyframe does not live")
        new_points, T = be.correct_points_sim3(P, ref, vScw[ids], Swc, opt)
        Tcw = np.array(graph["Tcw"], np.float32).reshape(len(live), 4, 4)
        Tcw[ids] = T
        vertices = vScw.copy()
        vertices[ids] = opt
        return {"Tcw": Tcw, "vertices": vertices, "points": new_points, "edges": (v0, v1, meas), "vScw": vScw,
                "chi2_before": r["chi2_before"], "chi2_after": r["chi2_after"], "iterations": r["iterations"],
                "trials": r["trials"], "status": r["status"]}
    finally:
        if own:
            be.close()


# ---- LoopClosing::CorrectLoop: the map surgery --------------------------------------
# On system.KeyFrame / system.MapPoint.  `backend`: LoopBackend, or an object of the same methods
# over a restatement (fuse_sim3_search, distinctive and the essential graph's three).

def _kf_frame(kf) -> Frame:
    return Frame(kf.keys_un, kf.desc, kf.u_right, kf.tcw, kf.cam, kf.scale_factors, bounds=getattr(kf, "bounds", None))


def _fuse_records(mps) -> np.ndarray:
    rec = np.zeros(len(mps), MAPPOINT_DTYPE)
    for j, mp in enumerate(mps):
        rec["pos"][j], rec["normal"][j], rec["desc"][j] = mp.pos, mp.normal, mp.desc
        rec["max_distance"][j], rec["min_distance"][j] = mp.max_distance, mp.min_distance
        rec["flags"][j] = (MP_BAD if mp.bad else 0) | (MP_HAS_OBS if mp.nobs > 0 else 0)
    return rec


def sim3_to_cv_scw(S) -> np.ndarray:
    """Converter::toCvMat(g2o::Sim3): rows 0-2 of [s R | t], computed in double and rounded to
    float once."""
    S = np.asarray(S, np.float64).reshape(8)
    out = np.zeros((3, 4), np.float32)
    out[:, :3] = (S[7] * _quat_to_R(S[:4])).astype(np.float32)
    out[:, 3] = S[4:7].astype(np.float32)
    return out


def _distinctive(mps, backend):
    """MapPoint::ComputeDistinctiveDescriptors of the points that live, through the backend: the
    descriptors of the observing keyframes that are not bad, in keyframe-id order."""
    mps = [m for m in mps if not m.bad]
    rows, off = [], [0]
    for mp in mps:
        for kf in sorted(mp.observations, key=lambda k: k.id):
            if not kf.bad:
                rows.append(kf.desc[mp.observations[kf]])
        off.append(len(rows))
    if not rows:
        return
    d = backend.distinctive(np.asarray(rows, np.uint8).reshape(-1, 32), np.asarray(off, np.int32))
    for j, mp in enumerate(mps):
        if off[j + 1] > off[j]:
            mp.desc = np.asarray(d[j], np.uint8).copy()


def fuse_sim3_replay(kf, pts, best_idx):
    """The map updates of ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)
    (src/ORBmatcher.cc:1247-1266) from the search's best_idx, in list order: a point that is bad or
    in kf by now is skipped; best_idx < 0 does nothing; else nFused counts, and the keypoint's
    slot, read as it is at that moment, decides: a point that is not bad becomes replace[i], a bad
    one changes nothing, an empty slot takes the point (AddObservation + AddMapPoint).
    -> (replace: vpReplacePoint, nfused)."""
    replace, nfused = [None] * len(pts), 0
    for i, mp in enumerate(pts):
        b = int(best_idx[i])
        if mp.bad or kf in mp.observations or b < 0:
            continue
        nfused += 1
        in_kf = kf.map_points[b]
        if in_kf is not None:
            if not in_kf.bad:
                replace[i] = in_kf
        else:
            mp.add_observation(kf, b)
            kf.map_points[b] = mp
    return replace, nfused


def search_and_fuse(corrected, loop_points, backend, th=4.0):
    """LoopClosing::SearchAndFuse (src/LoopClosing.cc:725-754): corrected = CorrectedPosesMap as
    {KeyFrame: Sim3}, taken in ascending keyframe id; loop_points = mvpLoopMapPoints.  Per keyframe:
    Fuse(pKF, cvScw, loop points, 4, vpReplacePoints), then vpReplacePoints[i]->Replace(loop point
    i) in index order, then the descriptors Replace owes its targets, once per keyframe.

    The search of all keyframes runs in one launch up front on the records as they are.  Between
    two keyframes a loop point's record changes only in its descriptor (a Replace onto it) and in
    its bad flag; bad and in-keyframe are re-checked by the replay, and a live point whose record
    differs from the one searched is searched again against the keyframes still to come, so the map
    after the call is the one the keyframe-by-keyframe loop leaves.
    -> one dict per keyframe: {"kf", "nfused", "added", "replaced", "researched"}."""
    kfs = sorted(corrected, key=lambda k: k.id)
    pts = list(loop_points)
    nkf, n = len(kfs), len(pts)
    if nkf == 0 or n == 0:
        return [{"kf": k.id, "nfused": 0, "added": 0, "replaced": 0, "researched": 0} for k in kfs]
    frames = [_kf_frame(k) for k in kfs]
    Scws = [sim3_to_cv_scw(corrected[k]) for k in kfs]
    rec0 = _fuse_records(pts)
    in0 = np.array([[k in mp.observations for mp in pts] for k in kfs], np.uint8)
    best = np.array(backend.fuse_sim3_search(frames, Scws, rec0, in0, th)[0], np.int32).reshape(nkf, n)
    out = []
    for t, kf in enumerate(kfs):
        rec = _fuse_records(pts)
        redo = [j for j, m in enumerate(pts) if not m.bad and rec[j].tobytes() != rec0[j].tobytes()]
        if redo:
            rin = np.array([[k in pts[j].observations for j in redo] for k in kfs[t:]], np.uint8)
            bi = backend.fuse_sim3_search(frames[t:], Scws[t:], rec[redo], rin, th)[0]
            best[t:, redo] = np.asarray(bi, np.int32).reshape(nkf - t, len(redo))
            rec0[redo] = rec[redo]
        had = [kf in m.observations for m in pts]
        replace, nfused = fuse_sim3_replay(kf, pts, best[t])
        added = sum(1 for j, m in enumerate(pts) if not had[j] and kf in m.observations)
        owed, replaced = [], 0
        for i, rep in enumerate(replace):
            if rep is not None and rep.replace(pts[i]):
                replaced += 1
                if pts[i] not in owed:
                    owed.append(pts[i])
        _distinctive(owed, backend)
        out.append({"kf": kf.id, "nfused": nfused, "added": added, "replaced": replaced, "researched": len(redo)})
    return out


def loop_connections(connected):
    """LoopConnections of CorrectLoop (src/LoopClosing.cc:665-692): per keyframe of
    mvpCurrentConnectedKFs (in the given order), UpdateConnections, then its connected keyframes
    minus its covisibles of before minus mvpCurrentConnectedKFs.
    -> {id: {id: weight}}, the weight GetWeight's after the update (essential_graph_edges' format)."""
    connected = list(connected)
    own = set(connected)
    out = {}
    for kf in connected:
        previous = set(kf.covisible)
        kf.update_connections()
        out[kf.id] = {k.id: int(kf.get_weight(k)) for k in sorted(kf.conn, key=lambda k: k.id)
                      if k not in previous and k not in own}
    return out


def current_matched_points(sim3_result, matched_kf, loop_points):
    """mvpCurrentMatchedPoints (src/LoopClosing.cc:430-470) as objects, one per keypoint slot of the
    current keyframe, from compute_sim3's result: loop_matched >= 0 is an index into loop_points
    (the list compute_sim3 searched, in its order), -2 a point of the matched keyframe outside that
    list (its slot in `matches`), -1 none."""
    lm, m12 = np.asarray(sim3_result["loop_matched"]), np.asarray(sim3_result["matches"])
    out = [None] * len(lm)
    for j in range(len(lm)):
        if lm[j] >= 0:
            out[j] = loop_points[int(lm[j])]
        elif lm[j] == -2 and m12[j] >= 0:
            out[j] = matched_kf.map_points[int(m12[j])]
    return out


def correct_loop(cur, matched_kf, Scw, current_matched, loop_points, keyframes, map_points, fix_scale, backend,
                 iterations=20):
    """LoopClosing::CorrectLoop (src/LoopClosing.cc:509-719) without the thread handshakes and
    without the global bundle adjustment.  cur / matched_kf: mpCurrentKF / mpMatchedKF; Scw: mg2oScw
    (8 doubles: q, t, s); current_matched: mvpCurrentMatchedPoints (current_matched_points);
    loop_points: mvpLoopMapPoints; keyframes / map_points: the map's.  Keyframe-keyed maps are
    walked in ascending id.
    -> {"corrected_points" {kf id: count}, "loop_fusion" {"replaced", "added"}, "search_and_fuse",
    "loop_connections", "graph", "essential_graph" (optimize_essential_graph's result)}."""
    from .system import update_normals_and_depths
    cur.update_connections()  # :540
    connected = list(cur.covisible) + [cur]  # mvpCurrentConnectedKFs
    n_ids = max(k.id for k in keyframes) + 1
    Tcw = np.zeros((n_ids, 4, 4), np.float32)
    Tcw[:] = np.eye(4, dtype=np.float32)
    for k in keyframes:
        Tcw[k.id] = np.asarray(k.tcw, np.float32).reshape(4, 4)
    Scw = np.asarray(Scw, np.float64).reshape(8)
    corrected, nonc = propagate_corrected_sim3(Tcw, cur.id, [k.id for k in cur.covisible], Scw, backend)  # :546-582
    by_id = {k.id: k for k in connected}
    order = sorted(corrected)
    # :586-633.  A point is corrected through the first keyframe (ascending id) that holds it; the
    # positions and the poses [R | t / s] of all of them come from one correct_points_sim3 call
    todo, ref = [], []
    seen = set()
    per_kf = {}
    for q, i in enumerate(order):
        mine = []
        for mp in by_id[i].map_points:
            if mp is None or mp.bad or mp.corrected_by_kf == cur.id or mp in seen:
                continue
            seen.add(mp)
            mine.append(mp)
        per_kf[i] = mine
        todo += mine
        ref += [q] * len(mine)
    Srw = np.array([nonc[i] for i in order], np.float64).reshape(-1, 8)
    Sc = np.array([corrected[i] for i in order], np.float64).reshape(-1, 8)
    Swr = np.array([_sim3_inverse(S) for S in Sc], np.float64).reshape(-1, 8)
    P = np.array([mp.pos for mp in todo], np.float32).reshape(-1, 3)
    newP, newT = backend.correct_points_sim3(P, np.asarray(ref, np.int32), Srw, Swr, Sc)
    at = 0
    for q, i in enumerate(order):
        kf = by_id[i]
        for mp in per_kf[i]:
            mp.pos = np.asarray(newP[at], np.float32).copy()
            mp.corrected_by_kf, mp.corrected_reference = cur.id, i
            at += 1
        # UpdateNormalAndDepth reads the centres of all observing keyframes as they are now: the
        # earlier ones corrected, this one and the later ones not yet
        update_normals_and_depths(per_kf[i])
        kf.tcw = np.asarray(newT[q], np.float32).reshape(4, 4).copy()
        kf.update_connections()
    # :638-653, the loop fusion
    fusion = {"replaced": 0, "added": 0}
    for i, lp in enumerate(current_matched):
        if lp is None:
            continue
        cm = cur.map_points[i]
        if cm is not None:
            if cm.replace(lp):
                fusion["replaced"] += 1
                _distinctive([lp], backend)
        else:
            cur.map_points[i] = lp
            lp.add_observation(cur, i)
            _distinctive([lp], backend)
            fusion["added"] += 1
    saf = search_and_fuse({by_id[i]: corrected[i] for i in order}, loop_points, backend)  # :661
    lc = loop_connections(connected)  # :665-692
    # Optimizer::OptimizeEssentialGraph over the map as it is now
    live = np.zeros(n_ids, bool)
    parent = np.full(n_ids, -1, np.int32)
    for k in keyframes:
        live[k.id] = not k.bad
        Tcw[k.id] = np.asarray(k.tcw, np.float32).reshape(4, 4)
        if k.parent is not None:
            parent[k.id] = k.parent.id
    G = {"live": live, "Tcw": Tcw, "parent": parent,
         "loop_edges": {k.id: [e.id for e in k.loop_edges] for k in keyframes if k.loop_edges},
         "covisibles": {k.id: [c.id for c in k.covisible if k.get_weight(c) >= 100] for k in keyframes if not k.bad},
         "corrected": corrected, "noncorrected": nonc, "loop_connections": lc, "loop_id": matched_kf.id, "cur_id": cur.id}
    pts = [mp for mp in map_points if not mp.bad]
    refs = [mp.corrected_reference if mp.corrected_by_kf == cur.id else mp.ref_kf.id for mp in pts]
    r = optimize_essential_graph(G, fix_scale, np.array([mp.pos for mp in pts], np.float32).reshape(-1, 3), refs,
                                 backend=backend, iterations=iterations)
    for k in keyframes:
        if not k.bad:
            k.tcw = np.asarray(r["Tcw"][k.id], np.float32).reshape(4, 4).copy()
    for j, mp in enumerate(pts):
        mp.pos = np.asarray(r["points"][j], np.float32).copy()
    update_normals_and_depths(pts)
    matched_kf.loop_edges.append(cur)  # :702-703
    cur.loop_edges.append(matched_kf)
    return {"corrected_points": {i: len(per_kf[i]) for i in order}, "loop_fusion": fusion, "search_and_fuse": saf,
            "loop_connections": lc, "graph": G, "essential_graph": r}


def global_bundle_adjustment(keyframes, map_points, loop_kf_id, backend, iterations=10, robust=False, stop=None,
                             stop_at_check=None):
    """Optimizer::GlobalBundleAdjustemnt (src/Optimizer.cc:47-53) = BundleAdjustment (:56-255) over
    the map: optimizer.gather_global_ba, backend.bundle_adjustment, then the write-back of :206-253.
    loop_kf_id == 0: straight into the poses and positions, with UpdateNormalAndDepth; otherwise
    into tcw_gba / pos_gba with ba_global_for_kf = loop_kf_id.  The estimate is written back even
    when the stop flag was seen, as the reference does.  -> the backend's result with "keyframes"
    and "map_points" (the vertices, in array order) added."""
    from .optimizer import gather_global_ba
    from .system import update_normals_and_depths
    problem, kfs, mps = gather_global_ba(keyframes, map_points)
    r = dict(backend.bundle_adjustment(problem, iterations, robust, stop, stop_at_check))
    for i, kf in enumerate(kfs):
        T = np.asarray(r["tcw"][i], np.float32).reshape(4, 4).copy()
        if loop_kf_id == 0:
            kf.tcw = T
        else:
            kf.tcw_gba, kf.ba_global_for_kf = T, loop_kf_id
    moved = []
    for j, mp in enumerate(mps):
        if not r["included"][j]:
            continue
        X = np.asarray(r["pos"][j], np.float32).copy()
        if loop_kf_id == 0:
            mp.pos = X
            moved.append(mp)
        else:
            mp.pos_gba, mp.ba_global_for_kf = X, loop_kf_id
    if moved:
        update_normals_and_depths(moved)
    r["keyframes"], r["map_points"] = kfs, mps
    return r


def run_global_bundle_adjustment(keyframes, map_points, origins, loop_kf_id, backend, iterations=10, robust=False,
                                 stop=None, stop_at_check=None):
    """LoopClosing::RunGlobalBundleAdjustment (src/LoopClosing.cc:790-901) without the thread
    handshakes: the bundle adjustment, then, unless the stop flag was seen, the map update of
    :812-891.  The spanning tree is walked breadth-first from `origins` (mvpKeyFrameOrigins), children
    in ascending id: a child the bundle adjustment did not optimise takes (Tchild * Twc_parent) *
    tcw_gba_parent; every keyframe reached keeps its pose in tcw_bef_gba and takes tcw_gba.  A point
    that was optimised takes pos_gba; another is carried through its reference keyframe,
    Rwc (Rcw_before X + tcw_before) + twc, unless that keyframe was not reached.  The products are
    float with double accumulators (cv::gemm's convention here; not pinned against OpenCV).
    loop_kf_id == 0 is BundleAdjustment's direct write-back: nothing is left to propagate.
    -> {"ba", "applied", "optimised", "propagated", "carried", "skipped"}."""
    from .system import _mul, pose_inverse
    ba = global_bundle_adjustment(keyframes, map_points, loop_kf_id, backend, iterations, robust, stop, stop_at_check)
    out = {"ba": ba, "applied": False, "optimised": 0, "propagated": 0, "carried": 0, "skipped": 0}
    if ba["stop_check"] >= 0 or (stop is not None and stop.value):  # if(!mbStopGBA)
        return out
    out["applied"] = True
    out["optimised"] = len(ba["keyframes"])
    if loop_kf_id == 0:
        return out
    queue = list(origins)
    at = 0
    while at < len(queue):
        kf = queue[at]
        at += 1
        Twc = pose_inverse(kf.tcw)
        for child in sorted(kf.children, key=lambda k: k.id):
            if child.ba_global_for_kf != loop_kf_id:
                child.tcw_gba = _mul(_mul(child.tcw, Twc), kf.tcw_gba)
                child.ba_global_for_kf = loop_kf_id
                out["propagated"] += 1
            queue.append(child)
        kf.tcw_bef_gba = kf.tcw
        kf.tcw = np.asarray(kf.tcw_gba, np.float32).reshape(4, 4).copy()
    for mp in map_points:
        if mp.bad:
            continue
        if mp.ba_global_for_kf == loop_kf_id:
            mp.pos = np.asarray(mp.pos_gba, np.float32).copy()
            continue
        ref = mp.ref_kf
        if ref is None or ref.ba_global_for_kf != loop_kf_id or ref.tcw_bef_gba is None:
            out["skipped"] += 1
            continue
        Tb = np.asarray(ref.tcw_bef_gba, np.float32).reshape(4, 4)
        Xc = (_mul(Tb[:3, :3], np.asarray(mp.pos, np.float32).reshape(3, 1)) + Tb[:3, 3:4]).astype(np.float32)
        Twc = pose_inverse(ref.tcw)
        mp.pos = (_mul(Twc[:3, :3], Xc) + Twc[:3, 3:4]).astype(np.float32)[:, 0].copy()
        out["carried"] += 1
    return out
