"""Loop detection: ORB_SLAM2::KeyFrameDatabase (src/KeyFrameDatabase.cc:33-197) on the device and
LoopClosing::DetectLoop (src/LoopClosing.cc:105-264) on top of it.

KeyFrameDatabase          orbmi_kfdb_*: the keyframes' BowVectors stored forward in one device
                          arena; a query intersects the query vector with every indexed slot.
LoopDetector              DetectLoop: the early add, minScore over the covisibles, the database
                          query and the covisibility-consistency groups.
detect_and_compute_sim3   DetectLoop, SearchByBoW(KF, KF) per enough-consistent candidate, then
                          sim3.compute_sim3: LoopClosing::Run up to CorrectLoop.

The covisibility graph stays the caller's: it comes in as callables (or mappings) from a keyframe
id to ids.  CorrectLoop and DetectRelocalizationCandidates are not here.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._capi import check, lib
from .sim3 import DeviceBackend, compute_sim3
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
        super().close()

    def search_by_bow_kf(self, cur, cand):
        """ORBmatcher matcher(0.75, true); matcher.SearchByBoW(mpCurrentKF, pKF, ...) (:299, :330)."""
        return self.matcher.SearchByBoWKF(cur["kf"], cur["ok"], cur["fv"], cand["kf"], cand["ok"], cand["fv"],
                                          nnratio=0.75, checkOri=True)


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
