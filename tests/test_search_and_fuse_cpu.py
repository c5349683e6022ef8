"""CorrectLoop's map surgery without a GPU, over the numpy restatement (tests/fuse_sim3_reference.py):
the search of Fuse(KF, Scw) clause by clause, loop.fuse_sim3_replay, loop.search_and_fuse against a
plain keyframe-by-keyframe loop, loop.loop_connections and loop.correct_loop on a map built from
the loop scene.  The scenes and the map builders are shared with tests/test_search_and_fuse_gpu.py."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_sim3_reference as ref  # noqa: E402
import sim3opt_reference as so  # noqa: E402

F32, F64 = np.float32, np.float64


# ---- the search, clause by clause ------------------------------------------------------------------

@pytest.mark.parametrize("s", [1.0, 1.3])
def test_search_restatement_names_every_clause(s):
    sc = ref.clause_scene(0, s)
    why = {}
    bi, bd = ref.fuse_sim3_search(sc["kf"], sc["Scw"], sc["mps"], sc["in_kf"], sc["th"], why)
    perm = sc["perm"]
    for i, clause in ((ref.BAD, "bad"), (ref.IN_KF, "in_kf"), (ref.BEHIND, "behind"), (ref.IMAGE, "image"),
                      (ref.DISTANCE, "distance"), (ref.NORMAL, "normal"), (ref.EMPTY, "empty window"),
                      (ref.OCT_M2, "octave"), (ref.OCT_P1, "octave")):
        assert why[i] == clause and bi[i] == -1 and bd[i] == 256, (i, clause, why[i])
    for i in (ref.OCT_M1, ref.OCT_0):
        assert why[i] == "fused" and bi[i] == perm[i]
    assert (bi[ref.DIST_50], bd[ref.DIST_50]) == (perm[ref.DIST_50], 50)
    assert (bi[ref.DIST_51], bd[ref.DIST_51]) == (-1, 51) and why[ref.DIST_51] == "distance > TH_LOW"
    # equal distances: the first keypoint in grid order, here the one of higher index
    k1, k2 = sc["tie_keys"]
    assert ref.grid_order_first(sc["kf"], k1, k2) == k2 > k1
    assert bi[ref.TIE] == k2 and bd[ref.TIE] == 3
    # two points on one keypoint: both get it
    assert bi[ref.SHARE_A] == bi[ref.SHARE_B] == perm[ref.SHARE_A]
    assert (bd[ref.SHARE_A], bd[ref.SHARE_B]) == (6, 0)
    # a keypoint that holds a point is still chosen; SearchByProjection(KF, Scw) would pass it by
    k = perm[ref.OCCUPIED]
    assert sc["occupied"][k] and bi[ref.OCCUPIED] == k
    matched = np.where(sc["occupied"] == 1, -2, -1).astype(np.int32)
    m, _ = so.search_by_projection_sim3(sc["kf"], sc["Scw"], sc["mps"], matched, sc["th"])
    assert m[k] == -2 and ref.OCCUPIED not in m
    # 3 scale[level] px off: inside the window of 4 scale[level], chi2 = 9 above 5.99 and 7.8
    k = perm[ref.FAR]
    assert bi[ref.FAR] == k and bd[ref.FAR] == 2
    lev = int(sc["kf"].keys["octave"][k])
    T, _ = so.decompose_scw(sc["Scw"])
    Pc = T[:, :3].astype(F64) @ sc["mps"]["pos"][ref.FAR].astype(F64) + T[:, 3]
    cam = sc["kf"].cam
    e = np.hypot(cam.fx * Pc[0] / Pc[2] + cam.cx - sc["kf"].keys["x"][k], cam.fy * Pc[1] / Pc[2] + cam.cy - sc["kf"].keys["y"][k])
    assert (e / sc["kf"].scale_factors[lev]) ** 2 > 7.8
    # the unnamed points land on their keypoints
    assert (bi[21:] == perm[21:]).all()


def test_search_restatement_batch_rows_are_the_single_calls():
    kfs, Scws, mps, in_kf = ref.batch_case(3, 33)
    bi, bd, nf = ref.fuse_sim3_search_batch(kfs, Scws, mps, in_kf, 4.0)
    for k in range(3):
        b1, d1 = ref.fuse_sim3_search(kfs[k], Scws[k], mps, in_kf[k], 4.0)
        assert np.array_equal(bi[k], b1) and np.array_equal(bd[k], d1) and nf[k] == (b1 >= 0).sum()
    assert nf[0] > 10 and nf[1] == 0 and (bd[1] == 256).all()


# ---- a small map of system.KeyFrame / system.MapPoint objects ---------------------------------------

def _scale_factors():
    s, out = F32(1), []
    for _ in range(8):
        out.append(s)
        s = F32(F64(s) * F64(F32(1.2)))
    return np.array(out, F32)


class MapBuilder:
    """Keyframes whose keypoints are added one by one, then frozen into system.KeyFrame arrays."""

    def __init__(self, seed):
        from orb_slam2_with_comment_amd import synth
        self.rng = np.random.default_rng(seed)
        self.cam = synth.KITTI
        self.sf = _scale_factors()
        self.rows = {}    # kf id -> [(x, y, octave, desc, occupant)]
        self.pose = {}    # kf id -> 4x4
        self.next_id = 0

    def keyframe(self, i, Tcw, clutter=0):
        self.rows[i], self.pose[i] = [], np.asarray(Tcw, F64)
        for _ in range(clutter):
            self.keypoint(i, self.rng.uniform(20, self.cam.width - 20), self.rng.uniform(20, self.cam.height - 20),
                          int(self.rng.integers(0, 8)), self.random_desc())

    def random_desc(self):
        return self.rng.integers(0, 256, 32).astype(np.uint8)

    def flipped(self, d, flips):
        d = d.copy()
        for b in self.rng.choice(256, flips, replace=False):
            d[b >> 3] ^= np.uint8(1 << (b & 7))
        return d

    def keypoint(self, i, x, y, octave, desc, occupant=None):
        self.rows[i].append((x, y, octave, desc, occupant))
        return len(self.rows[i]) - 1

    def project(self, i, X):
        T = self.pose[i]
        Pc = T[:3, :3] @ X + T[:3, 3]
        return self.cam.fx * Pc[0] / Pc[2] + self.cam.cx, self.cam.fy * Pc[1] / Pc[2] + self.cam.cy

    def point(self, X, octave, desc, ref_id, view_from):
        """A map point record without observations yet (observe() adds them after freeze)."""
        from orb_slam2_with_comment_amd.system import MapPoint
        Ow = -self.pose[view_from][:3, :3].T @ self.pose[view_from][:3, 3]
        PO = np.asarray(X, F64) - Ow
        dist = np.linalg.norm(PO)
        mp = MapPoint(self.next_id, np.asarray(X, F32), ref_id, desc.copy(), (PO / dist).astype(F32),
                      F32(dist * 1.2 ** (octave - 0.5)), F32(dist * 1.2 ** (octave - 0.5) / 1.2 ** 7))
        self.next_id += 1
        return mp

    def freeze(self):
        from orb_slam2_with_comment_amd.system import KeyFrame
        from orb_slam2_with_comment_amd.types import KP_DTYPE
        kfs = {}
        for i, rows in self.rows.items():
            keys = np.zeros(len(rows), KP_DTYPE)
            keys["x"], keys["y"] = [r[0] for r in rows], [r[1] for r in rows]
            keys["octave"] = [r[2] for r in rows]
            desc = np.array([r[3] for r in rows], np.uint8).reshape(-1, 32)
            kfs[i] = KeyFrame(i, i, float(i), self.pose[i].astype(F32), keys, desc, np.full(len(rows), -1, F32),
                              np.full(len(rows), -1, F32), (1.0 / self.sf ** 2).astype(F32), self.sf, self.cam,
                              [None] * len(rows))
        points = {}
        for i, rows in self.rows.items():
            for idx, r in enumerate(rows):
                mp = r[4]
                if mp is None:
                    continue
                points[mp.id] = mp
                if isinstance(mp.ref_kf, int):
                    mp.ref_kf = kfs[mp.ref_kf]
                kfs[i].map_points[idx] = mp
                mp.add_observation(kfs[i], idx)
        return kfs, points


def _sim3(rng, s):
    """A Sim3 (q, t, s) near the identity, and its SE3 pose [R | t / s]."""
    import essgraph_reference as eg
    R = so._rodrigues(rng.normal(0, 0.01, 3))
    t = rng.normal(0, 0.05, 3)
    S = eg.from_rts(R[None], (s * t)[None], 1.0)[0]
    S[7] = s
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return S, T


LOOP_KF, SIDE_X, SIDE_Y = 0, 30, 31     # the loop side's keyframe and two helpers of the current side
CORRECTED = (10, 11, 12, 13)            # the corrected keyframes, searched in this order
N_RANDOM = 40
# hand-built loop points (indices into the list)
TWO_ON_ONE_A, TWO_ON_ONE_B, CHAIN_P, CHAIN_Q, REDESC, SHARED = 40, 41, 42, 43, 44, 45
N_LOOP = 46


def fuse_map(seed=3):
    """A map in which every event of SearchAndFuse happens.  Loop points 0 .. N_LOOP - 1, each
    observed by keyframe LOOP_KF; the corrected keyframes CORRECTED, each with its own Sim3 (scales
    1, 1.1, 0.9, 1.05) and 60 keypoints of clutter.  Points 0 .. 39 get, per corrected keyframe with
    probability 0.6, a keypoint at their projection (0 .. 20 bits away), empty or (0.4) holding a
    point of the current side that keyframe SIDE_X observes too.  By hand:
      TWO_ON_ONE_A / _B  one position; their keypoint in keyframe 10 holds a point: both name it
      CHAIN_P / CHAIN_Q  one position; their keypoint in 10 is empty: P is added, then replaced by
                         Q and turns bad; keyframe 11 has a keypoint for them too
      REDESC     replaces in 10 a point that SIDE_X and SIDE_Y observe with two close descriptors
                 far from its own, so its distinctive descriptor changes; keyframe 11 has one
                 keypoint near the old descriptor (redesc_old) and one near the new (redesc_new)
      SHARED     its keypoints in 10 and 11 hold one and the same point: after 10 it is in 11
    -> (kfs {id: KeyFrame}, corrected {KeyFrame: Sim3}, loop_points, info)."""
    B = MapBuilder(seed)
    rng = B.rng
    B.keyframe(LOOP_KF, np.eye(4))
    B.keyframe(SIDE_X, np.eye(4))
    B.keyframe(SIDE_Y, np.eye(4))
    sims = {}
    for i, s in zip(CORRECTED, (1.0, 1.1, 0.9, 1.05)):
        sims[i], T = _sim3(rng, s)
        B.keyframe(i, T, clutter=60)
    z = rng.uniform(8, 30, N_LOOP)
    X = np.stack([rng.uniform(-0.6, 0.6, N_LOOP) * z, rng.uniform(-0.15, 0.15, N_LOOP) * z, z], -1)  # all inside the image
    X[TWO_ON_ONE_B], X[CHAIN_Q] = X[TWO_ON_ONE_A], X[CHAIN_P]
    octave = rng.integers(1, 7, N_LOOP)
    octave[TWO_ON_ONE_B], octave[CHAIN_Q] = octave[TWO_ON_ONE_A], octave[CHAIN_P]
    d0 = [B.random_desc() for _ in range(N_LOOP)]
    d0[TWO_ON_ONE_B] = B.flipped(d0[TWO_ON_ONE_A], 4)
    d0[CHAIN_Q] = B.flipped(d0[CHAIN_P], 4)
    loop_points = []
    for i in range(N_LOOP):
        mp = B.point(X[i], int(octave[i]), d0[i], LOOP_KF, CORRECTED[0])
        B.keypoint(LOOP_KF, 100.0 + 20 * i, 100.0, int(octave[i]), d0[i], mp)
        loop_points.append(mp)

    def side_point(i, k, desc):
        return B.point(X[i], int(octave[i]), desc, k, k)

    def target(i, k, desc, occupant=None, dx=0.0):
        u, v = B.project(k, X[i])
        return B.keypoint(k, u + dx + rng.uniform(-0.3, 0.3), v + rng.uniform(-0.3, 0.3), int(octave[i]), desc, occupant)
    for i in range(N_RANDOM):
        for k in CORRECTED:
            if rng.random() >= 0.6:
                continue
            d = B.flipped(d0[i], int(rng.integers(0, 21)))
            occ = None
            if rng.random() < 0.4:
                occ = side_point(i, k, d)
                B.keypoint(SIDE_X, rng.uniform(20, 1200), rng.uniform(20, 350), int(octave[i]), B.random_desc(), occ)
            target(i, k, d, occ)
    k0, k1 = CORRECTED[0], CORRECTED[1]
    d = B.flipped(d0[TWO_ON_ONE_A], 2)
    target(TWO_ON_ONE_A, k0, d, side_point(TWO_ON_ONE_A, k0, d))
    target(CHAIN_P, k0, B.flipped(d0[CHAIN_P], 2))
    target(CHAIN_P, k1, B.flipped(d0[CHAIN_P], 1))
    dA, dB = B.flipped(d0[REDESC], 5), B.random_desc()
    c = side_point(REDESC, k0, dA)
    target(REDESC, k0, dA, c)
    B.keypoint(SIDE_X, 50.0, 50.0, int(octave[REDESC]), dB, c)
    B.keypoint(SIDE_Y, 50.0, 50.0, int(octave[REDESC]), B.flipped(dB, 2), c)
    old = target(REDESC, k1, B.flipped(d0[REDESC], 3), dx=-1.0)
    new = target(REDESC, k1, B.flipped(dB, 1), dx=1.0)
    d = B.flipped(d0[SHARED], 2)
    c = side_point(SHARED, k0, d)
    target(SHARED, k0, d, c)
    target(SHARED, k1, B.flipped(d0[SHARED], 3), c)
    kfs, _ = B.freeze()
    corrected = {kfs[i]: sims[i] for i in CORRECTED}
    return kfs, corrected, loop_points, {"redesc_old": old, "redesc_new": new}


def snapshot(kfs, points):
    """Everything the surgery can change, by id."""
    seen, todo = {}, list(points)
    for kf in kfs.values():
        todo += [m for m in kf.map_points if m is not None]
    while todo:
        m = todo.pop()
        if m.id in seen:
            continue
        seen[m.id] = m
        if m.replaced is not None:
            todo.append(m.replaced)
    return {
        "observations": {i: sorted((k.id, idx) for k, idx in m.observations.items()) for i, m in sorted(seen.items())},
        "slots": {i: [None if m is None else m.id for m in kf.map_points] for i, kf in sorted(kfs.items())},
        "bad": {i: m.bad for i, m in sorted(seen.items())},
        "replaced": {i: None if m.replaced is None else m.replaced.id for i, m in sorted(seen.items())},
        "nobs": {i: m.nobs for i, m in sorted(seen.items())},
        "found": {i: (m.found, m.visible) for i, m in sorted(seen.items())},
        "desc": {i: bytes(np.asarray(m.desc, np.uint8)) for i, m in sorted(seen.items())},
    }


def plain_search_and_fuse(corrected, loop_points, events=None):
    """LoopClosing::SearchAndFuse as the reference runs it, from the restatement: per keyframe in
    ascending id the search on the map as it is, the map updates of :1247-1266 in list order, the
    Replace calls in index order, ComputeDistinctiveDescriptors after every Replace."""
    from orb_slam2_with_comment_amd import loop
    events = {} if events is None else events
    for k in ("added", "replaced", "named_twice", "bad_before_later", "stale_differs"):
        events.setdefault(k, 0)
    kfs = sorted(corrected, key=lambda k: k.id)
    for t, kf in enumerate(kfs):
        rec = loop._fuse_records(loop_points)
        in_kf = np.array([kf in m.observations for m in loop_points], np.uint8)
        Scw = loop.sim3_to_cv_scw(corrected[kf])
        bi, _ = ref.fuse_sim3_search(loop._kf_frame(kf), Scw, rec, in_kf, 4.0)
        events["bad_before_later"] += sum(1 for m in loop_points if m.bad and t > 0 and not getattr(m, "_was_bad", False))
        for m in loop_points:
            m._was_bad = m.bad
        replace = [None] * len(loop_points)
        for i, m in enumerate(loop_points):
            if rec["flags"][i] & 1 or in_kf[i] or bi[i] < 0:
                continue
            holder = kf.map_points[bi[i]]
            if holder is None:
                m.add_observation(kf, int(bi[i]))
                kf.map_points[bi[i]] = m
                events["added"] += 1
            elif not holder.bad:
                replace[i] = holder
        named = [r.id for r in replace if r is not None]
        events["named_twice"] += len(named) - len(set(named))
        for i, r in enumerate(replace):
            if r is not None and r.replace(loop_points[i]):
                events["replaced"] += 1
                m = loop_points[i]
                if not m.bad:
                    rows = [k.desc[m.observations[k]] for k in sorted(m.observations, key=lambda k: k.id) if not k.bad]
                    m.desc = ref.distinctive(np.array(rows, np.uint8), np.array([0, len(rows)], np.int32))[0].copy()
    return events


# ---- fuse_sim3_replay ------------------------------------------------------------------------------

def _replay_map():
    """One keyframe with five keypoints: 0 empty, 1 held by a live point, 2 held by a bad point,
    3 empty; four loop points."""
    B = MapBuilder(1)
    B.keyframe(0, np.eye(4))
    B.keyframe(1, np.eye(4))
    X = np.array([0.0, 0.0, 10.0])
    live, dead = B.point(X, 2, B.random_desc(), 1, 1), B.point(X, 2, B.random_desc(), 1, 1)
    for occ in (None, live, dead, None, None):
        B.keypoint(1, 100.0, 100.0, 2, B.random_desc(), occ)
    pts = [B.point(X, 2, B.random_desc(), 0, 1) for _ in range(5)]
    for p in pts:
        B.keypoint(0, 50.0, 50.0, 2, p.desc, p)
    kfs, _ = B.freeze()
    dead.bad = True
    return kfs[1], pts, live, dead


def test_replay_empty_live_and_bad_slots():
    from orb_slam2_with_comment_amd.loop import fuse_sim3_replay
    kf, pts, live, dead = _replay_map()
    replace, nfused = fuse_sim3_replay(kf, pts, [0, 1, 2, -1, -1])
    assert nfused == 3
    assert replace == [None, live, None, None, None]
    assert kf.map_points[0] is pts[0] and pts[0].observations[kf] == 0 and pts[0].nobs == 2
    assert kf.map_points[1] is live and kf.map_points[2] is dead and kf not in pts[2].observations
    assert kf not in pts[3].observations and kf.map_points[3] is None


def test_replay_two_points_on_one_empty_slot():
    """The loop reads the slot as it is at that moment: the second point finds the first."""
    from orb_slam2_with_comment_amd.loop import fuse_sim3_replay
    kf, pts, _, _ = _replay_map()
    replace, nfused = fuse_sim3_replay(kf, pts, [3, 3, -1, -1, -1])
    assert nfused == 2 and replace[0] is None and replace[1] is pts[0]
    assert kf.map_points[3] is pts[0] and kf not in pts[1].observations


def test_replay_rechecks_bad_and_in_keyframe():
    """A point that turned bad or entered the keyframe between the search and the replay."""
    from orb_slam2_with_comment_amd.loop import fuse_sim3_replay
    kf, pts, live, _ = _replay_map()
    pts[0].bad = True
    pts[1].add_observation(kf, 4)
    kf.map_points[4] = pts[1]
    replace, nfused = fuse_sim3_replay(kf, pts, [0, 1, 3, -1, -1])
    assert nfused == 1 and replace == [None] * 5
    assert kf.map_points[0] is None and kf.map_points[1] is live and kf.map_points[3] is pts[2]
    assert pts[1].observations[kf] == 4


# ---- search_and_fuse ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def plain_fuse_result():
    kfs, corrected, loop_points, info = fuse_map()
    events = plain_search_and_fuse(corrected, loop_points)
    return snapshot(kfs, loop_points), events, info


def test_fuse_map_makes_every_event_happen_in_the_plain_loop():
    from orb_slam2_with_comment_amd import loop
    snap, events, info = plain_fuse_result()
    print("plain loop events", events)
    assert events["added"] >= 10 and events["replaced"] >= 10
    assert events["named_twice"] >= 1 and events["bad_before_later"] >= 1
    k0, k1 = CORRECTED[0], CORRECTED[1]
    # one replace[i] named by two list entries
    assert snap["bad"][CHAIN_P] and snap["replaced"][CHAIN_P] == CHAIN_Q
    assert (k1, snap["slots"][k1].index(CHAIN_Q)) in snap["observations"][CHAIN_Q]
    # the point whose descriptor changed after keyframe 10 chose, in 11, the keypoint of its new
    # descriptor; with the descriptor it had before, the search picks the other one
    kfs, corrected, loop_points, _ = fuse_map()
    kf = kfs[k1]
    rec = loop._fuse_records(loop_points)
    old, _ = ref.fuse_sim3_search(loop._kf_frame(kf), loop.sim3_to_cv_scw(corrected[kf]), rec, None, 4.0)
    assert old[REDESC] == info["redesc_old"]
    assert (k1, info["redesc_new"]) in snap["observations"][REDESC]
    assert snap["desc"][REDESC] != bytes(loop_points[REDESC].desc)
    # the shared occupant: after keyframe 10 the loop point is in 11 already
    assert {k for k, _ in snap["observations"][SHARED]} >= {LOOP_KF, k0, k1}


def test_search_and_fuse_leaves_the_plain_loops_map():
    from orb_slam2_with_comment_amd import loop
    want, _, _ = plain_fuse_result()
    kfs, corrected, loop_points, _ = fuse_map()
    be = ref.RestatementBackend()
    counts = loop.search_and_fuse(corrected, loop_points, be)
    got = snapshot(kfs, loop_points)
    for key in want:
        assert got[key] == want[key], key
    print("search_and_fuse counts", counts, "searches", be.calls)
    assert [c["kf"] for c in counts] == list(CORRECTED)
    assert be.calls[0] == (len(CORRECTED), N_LOOP)           # one batch up front
    assert sum(c["researched"] for c in counts) >= 1 and len(be.calls) >= 2
    assert all(n < N_LOOP for _, n in be.calls[1:])          # afterwards only the changed records
    assert sum(c["added"] for c in counts) >= 10 and sum(c["replaced"] for c in counts) >= 10


def test_search_and_fuse_without_the_research_differs():
    """The re-search is what makes the batch equal the loop: a backend that answers every later call
    with 'nothing found' leaves another map."""
    from orb_slam2_with_comment_amd import loop
    want, _, _ = plain_fuse_result()
    kfs, corrected, loop_points, _ = fuse_map()

    class Stale(ref.RestatementBackend):
        def fuse_sim3_search(self, kfs_, Scws, mps, in_kf, th):
            if self.calls:
                self.calls.append((len(kfs_), len(mps)))
                n = (len(kfs_), len(mps))
                return np.full(n, -1, np.int32), np.full(n, 256, np.int32), np.zeros(len(kfs_), np.int32)
            return super().fuse_sim3_search(kfs_, Scws, mps, in_kf, th)
    loop.search_and_fuse(corrected, loop_points, Stale())
    assert snapshot(kfs, loop_points)["observations"] != want["observations"]


def test_search_and_fuse_empty_inputs():
    from orb_slam2_with_comment_amd import loop
    kfs, corrected, loop_points, _ = fuse_map()
    be = ref.RestatementBackend()
    assert loop.search_and_fuse({}, loop_points, be) == []
    assert [c["nfused"] for c in loop.search_and_fuse(corrected, [], be)] == [0] * len(CORRECTED)
    assert be.calls == []


def test_sim3_to_cv_scw_rounds_once():
    from orb_slam2_with_comment_amd import loop
    import essgraph_reference as eg
    R = so._rodrigues(np.array([0.1, -0.2, 0.3]))
    t = np.array([1.0, -2.0, 0.5])
    S = eg.from_rts(R[None], t[None], 1.0)[0]
    S[7] = 1.25
    want = np.hstack([1.25 * np.asarray(eg.quat_to_R(S[None, :4]), F64).reshape(3, 3), t[:, None]])
    got = loop.sim3_to_cv_scw(S)
    assert got.dtype == np.float32 and got.shape == (3, 4)
    assert np.abs(got.astype(F64) - want).max() <= 2.0 ** -24 * np.abs(want).max()
    T, _ = so.decompose_scw(got)
    assert np.abs(T[:, :3] - R).max() < 1e-6 and np.abs(T[:, 3] - t / 1.25).max() < 1e-6


# ---- loop_connections --------------------------------------------------------------------------------

def test_loop_connections_keeps_only_the_new_links():
    """A is connected to B (both in the connected set) and to its previous covisible P; after the
    fusion it also shares 17 points with M, a member of the connected set it was not linked to, and
    16 with N, outside the set.  Only N is a loop connection.  B and M gain nothing."""
    from orb_slam2_with_comment_amd import loop
    B = MapBuilder(2)
    for i in (1, 2, 3, 4, 5):
        B.keyframe(i, np.eye(4))
    A_, B_, P_, N_, M_ = 1, 2, 3, 4, 5
    X = np.array([0.0, 0.0, 10.0])
    for other, count in ((B_, 20), (P_, 18), (N_, 16), (M_, 17)):
        for _ in range(count):
            mp = B.point(X, 2, B.random_desc(), A_, A_)
            B.keypoint(A_, 10.0, 10.0, 2, mp.desc, mp)
            B.keypoint(other, 10.0, 10.0, 2, mp.desc, mp)
    kfs, _ = B.freeze()
    A, Bk, P, N, M = kfs[A_], kfs[B_], kfs[P_], kfs[N_], kfs[M_]
    for a, b, w in ((A, Bk, 20), (A, P, 18)):
        a.add_connection(b, w)
        b.add_connection(a, w)
    for k in kfs.values():
        k.first_connection = False
    got = loop.loop_connections([Bk, M, A])
    assert got == {B_: {}, M_: {}, A_: {N_: 16}}
    assert list(got) == [B_, M_, A_]
    assert A.get_weight(N) == 16 and N.get_weight(A) == 16      # the new link, with UpdateConnections' weight
    assert A.get_weight(P) == 18 and A.get_weight(M) == 17      # a previous covisible and a member: linked, not listed


# ---- correct_loop on the loop scene ----------------------------------------------------------------

DRIFT_T, DRIFT_R = [0.3, -0.05, 0.1], 0.01   # tests/test_essgraph_gpu.py's end-to-end drift
N_SHARED = 40                                 # points every recent keyframe shares with each covisible


def loop_scene_map():
    """The loop scene as a map of objects: keyframes 0 .. 11, 15 and 20 .. 23 as system.KeyFrame, the
    points in their slots as system.MapPoint (a record flagged bad: a bad point outside its slot).
    Connections weigh as tests/test_essgraph_gpu.py's end-to-end test weighs them (the points of i
    projecting into j), the spanning tree is the chain in id order, the keyframes from 12 on and
    their points are drifted by 0.3 m / 0.01 rad.  So that the recent keyframes are connected
    through real observations too, each shares N_SHARED of its points with each of its covisibles
    (in keypoint slots that held nothing).  -> (kfs {id: KeyFrame}, points (list), by_slot)."""
    import essgraph_reference as eg
    import loop_reference as lref
    from orb_slam2_with_comment_amd import synth
    from orb_slam2_with_comment_amd.system import KeyFrame, MapPoint
    sc = lref.loop_scene()
    src, covis = sc["keyframes"], sc["covisible"]
    cam = synth.KITTI
    D = np.eye(4)
    D[:3, :3] = eg._rot([0.2, 1.0, 0.1], DRIFT_R)
    D[:3, 3] = DRIFT_T
    Dinv = np.linalg.inv(D)
    kfs, points, by_slot = {}, [], {}
    for i in sorted(src):
        F = src[i]["kf"]
        T = np.asarray(F.tcw, F64).reshape(4, 4)
        if i >= 12:
            T = T @ D
        sf = np.asarray(F.scale_factors, F32)
        kfs[i] = KeyFrame(i, i, float(i), T.astype(F32), F.keys, F.desc, F.u_right, np.full(len(F.keys), -1, F32),
                          (1.0 / sf ** 2).astype(F32), sf, cam, [None] * len(F.keys), first_connection=False)
    for i in sorted(src):
        kf, rec, has = kfs[i], src[i]["mps"], src[i]["has"]
        by_slot[i] = {}
        for idx in np.nonzero(has == 1)[0]:
            r = rec[idx]
            pos = r["pos"].astype(F64)
            if i >= 12:
                pos = Dinv[:3, :3] @ pos + Dinv[:3, 3]
            mp = MapPoint(len(points), pos.astype(F32), kf, r["desc"].copy(), r["normal"].copy(), r["max_distance"],
                          r["min_distance"])
            points.append(mp)
            by_slot[i][int(idx)] = mp
            if r["flags"] & 1:
                mp.bad = True
                continue
            kf.map_points[idx] = mp
            mp.add_observation(kf, int(idx))

    def shared(i, j):
        mp = src[i]["mps"][src[i]["has"] == 1]["pos"].astype(F64)
        T = np.asarray(src[j]["kf"].tcw, F64).reshape(4, 4)
        c = mp @ T[:3, :3].T + T[:3, 3]
        z = c[:, 2]
        ok = z > 0.1
        u, v = cam.fx * c[:, 0] / np.where(ok, z, 1) + cam.cx, cam.fy * c[:, 1] / np.where(ok, z, 1) + cam.cy
        return int((ok & (u >= 0) & (u < cam.width) & (v >= 0) & (v < cam.height)).sum())
    for i in sorted(src):
        for j in covis[i]:
            kfs[i].add_connection(kfs[j], shared(i, j))
    order = sorted(src)
    for a, b in zip(order[1:], order[:-1]):
        kfs[a].parent = kfs[b]
        kfs[b].children.append(kfs[a])
    for i in sorted(src):
        if i < 12:
            continue
        own = [m for m in kfs[i].map_points if m is not None and m.ref_kf is kfs[i]]
        for q, j in enumerate(covis[i]):
            free = [s for s, m in enumerate(kfs[j].map_points) if m is None and s not in by_slot[j]]
            for mp, s in zip(own[q * N_SHARED:(q + 1) * N_SHARED], free):
                kfs[j].map_points[s] = mp
                mp.add_observation(kfs[j], s)
    return kfs, points, by_slot


@functools.lru_cache(maxsize=None)
def restatement_sim3():
    import loop_reference as lref
    res = lref.run_loop_scene(lref.RestatementLoopBackend())[-1]
    assert res["detected"] and res["sim3"]["accepted"]
    return res


def run_correct_loop(res, backend):
    """correct_loop on a fresh loop_scene_map with the Sim3 result `res`.
    -> (kfs, points, before {id: Tcw}, out)."""
    import essgraph_reference as eg
    import loop_reference as lref
    from orb_slam2_with_comment_amd import loop
    kfs, points, by_slot = loop_scene_map()
    cur, matched = kfs[res["current"]], kfs[res["loop_kf"]]
    src = lref.loop_scene()["keyframes"][matched.id]
    first = [by_slot[matched.id][int(s)] for s in np.nonzero(src["has"] == 1)[0]]  # compute_sim3's list, in its order
    loop_points = first + [m for j in (matched.id - 1, matched.id + 1) for m in kfs[j].map_points if m is not None]
    cm = loop.current_matched_points(res["sim3"], matched, loop_points)
    scw = res["sim3"]["scw"]
    Scw = eg.from_rts((np.asarray(scw["sR"], F64) / scw["s"])[None], np.asarray(scw["t"])[None], 1.0)[0]
    Scw[7] = F64(scw["s"])
    before = {i: k.tcw.copy() for i, k in kfs.items()}
    out = loop.correct_loop(cur, matched, Scw, cm, loop_points, list(kfs.values()), points, True, backend)
    return kfs, points, before, out


@functools.lru_cache(maxsize=None)
def restatement_correct_loop():
    return run_correct_loop(restatement_sim3(), ref.RestatementBackend())


def test_current_matched_points(oracle):
    from orb_slam2_with_comment_amd import loop
    res = restatement_sim3()
    kfs, points, by_slot = loop_scene_map()
    matched = kfs[res["loop_kf"]]
    lst = [m for m in matched.map_points if m is not None]
    r = {"loop_matched": np.array([0, -1, -2, -2, 2]), "matches": np.array([5, -1, 7, -1, 9])}
    slot7 = matched.map_points[7]
    assert loop.current_matched_points(r, matched, lst) == [lst[0], None, slot7, None, lst[2]]


def test_correct_loop_on_the_loop_scene(oracle):
    res = restatement_sim3()
    kfs, points, before, out = restatement_correct_loop()
    cur, matched = kfs[res["current"]], kfs[res["loop_kf"]]
    corrected_ids = sorted(out["graph"]["corrected"])
    assert corrected_ids == [15, 20, 21, 22, 23] and cur.id == 23 and matched.id == 3
    # a point is corrected exactly once, through the lowest-id corrected keyframe that holds it
    held = {}
    fresh = loop_scene_map()[0]
    n_corrected = 0
    for i in corrected_ids:
        for m in fresh[i].map_points:
            if m is not None:
                held.setdefault(m.id, i)
    by_id = {m.id: m for m in points}
    for pid, i in held.items():
        m = by_id[pid]
        assert m.corrected_by_kf == cur.id and m.corrected_reference == i
        n_corrected += 1
    assert sum(out["corrected_points"].values()) == n_corrected
    assert any(by_id[p].ref_kf.id != i for p, i in held.items())   # first come, first served did bind
    assert all(m.corrected_by_kf == -1 for m in points if m.id not in held)
    saf = out["search_and_fuse"]
    print("correct_loop: corrected", out["corrected_points"], "loop fusion", out["loop_fusion"], "search_and_fuse", saf)
    assert sum(c["replaced"] for c in saf) >= 1 and sum(c["added"] for c in saf) >= 1
    assert out["loop_fusion"]["replaced"] + out["loop_fusion"]["added"] >= 40
    lc = out["loop_connections"]
    print("loop connections", lc)
    assert sorted(lc) == corrected_ids and any(lc.values())
    assert matched.id in lc[cur.id] and lc[cur.id][matched.id] == cur.get_weight(matched) >= 15
    assert all(j < 12 for row in lc.values() for j in row)
    eg_out = out["essential_graph"]
    pairs = list(zip(eg_out["edges"][0].tolist(), eg_out["edges"][1].tolist()))
    assert (cur.id, matched.id) in pairs
    print("chi2 %.3e -> %.3e, %d edges" % (eg_out["chi2_before"], eg_out["chi2_after"], len(pairs)))
    assert eg_out["chi2_after"] < eg_out["chi2_before"]
    assert matched in cur.loop_edges and cur in matched.loop_edges
    for kf in kfs.values():
        for idx, m in enumerate(kf.map_points):
            assert m is None or not m.bad
    for m in points:
        for kf, idx in m.observations.items():
            assert kf.map_points[idx] is m
    # the drift is gone: the recent keyframes end near the poses the scene rendered them from
    import loop_reference as lref
    src = lref.loop_scene()["keyframes"]
    for i in corrected_ids:
        true = np.asarray(src[i]["kf"].tcw, F64).reshape(4, 4)
        assert np.abs(before[i][:3, 3] - true[:3, 3]).max() > 0.05
        assert np.abs(kfs[i].tcw[:3, 3] - true[:3, 3]).max() < 0.05
