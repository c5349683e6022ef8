"""ORBmatcher::Fuse(KF, Scw, vpPoints, th, vpReplacePoint) (src/ORBmatcher.cc:1139-1269) restated in
numpy, float32-exact: the search as orbmi_fuse_sim3_search_batch returns it, the scene that names
one point per clause of that search, and a restatement backend for loop.search_and_fuse /
loop.correct_loop.  The map updates (:1247-1266) are loop.fuse_sim3_replay's; the plain
keyframe-by-keyframe loop the tests compare against is written in the tests.

Built on sim3opt_reference: decompose_scw and the grid arithmetic of search_by_projection_sim3
(the same projection, gates, level prediction and window; no occupancy, and the decision is
per point, so nothing here depends on the order of the list)."""
from __future__ import annotations

import math

import numpy as np

import sim3opt_reference as so

F32, F64 = np.float32, np.float64
TH_LOW = so.TH_LOW
_POPC = so._POPC


def _grid(kf):
    """AssignFeaturesToGrid of a keyframe: (in_grid, px, py, cell) per keypoint."""
    v = kf.view()
    kx, ky = kf.keys["x"].astype(F32), kf.keys["y"].astype(F32)
    gx = ((kx - F32(v.min_x)) * F32(v.grid_w_inv)).astype(F64)
    gy = ((ky - F32(v.min_y)) * F32(v.grid_h_inv)).astype(F64)
    px = (np.sign(gx) * np.floor(np.abs(gx) + 0.5)).astype(np.int64)
    py = (np.sign(gy) * np.floor(np.abs(gy) + 0.5)).astype(np.int64)
    return (px >= 0) & (px < 64) & (py >= 0) & (py < 48), px, py, px * 48 + py


def fuse_sim3_search(kf, Scw, mps, in_kf=None, th=4.0, trace=None):
    """The search of :1164-1246 for one keyframe.  -> best_idx (the keypoint when bestDist <=
    TH_LOW, else -1), best_dist (the least distance in the window, 256 without a candidate).
    trace (a dict) receives per point the clause that decided it."""
    from orb_slam2_with_comment_amd.types import MP_BAD
    n = len(mps)
    best_idx, best_dist = np.full(n, -1, np.int32), np.full(n, 256, np.int32)
    v = kf.view()
    min_x, max_x, min_y, max_y = F32(v.min_x), F32(v.max_x), F32(v.min_y), F32(v.max_y)
    gwi, ghi = F32(v.grid_w_inv), F32(v.grid_h_inv)
    scale, logsf, nlev = np.asarray(kf.scale_factors, F32), F32(v.log_scale_factor), v.nlevels
    fx, fy, cx, cy = F32(v.fx), F32(v.fy), F32(v.cx), F32(v.cy)
    kx, ky, koct = kf.keys["x"].astype(F32), kf.keys["y"].astype(F32), kf.keys["octave"]
    in_grid, px, py, cell = _grid(kf)
    T, Ow = so.decompose_scw(Scw)
    th = F32(th)
    why = {}
    for i in range(n):
        if mps["flags"][i] & MP_BAD:
            why[i] = "bad"
            continue
        if in_kf is not None and in_kf[i]:
            why[i] = "in_kf"
            continue
        X = mps["pos"][i].astype(F32)
        with np.errstate(all="ignore"):
            Pc = [F32(F32(F32(F32(T[r, 0] * X[0]) + F32(T[r, 1] * X[1])) + F32(T[r, 2] * X[2])) + T[r, 3])
                  for r in range(3)]
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
        if not c.any():
            why[i] = "empty window"
            continue
        c &= (koct >= level - 1) & (koct <= level)
        idx = np.nonzero(c)[0]
        if len(idx) == 0:
            why[i] = "octave"
            continue
        dd = _POPC[kf.desc[idx] ^ mps["desc"][i][None, :]].sum(1)
        b = np.lexsort((idx, cell[idx], dd))[0]  # strict <: ties to the first in grid order
        best_dist[i] = dd[b]
        if dd[b] <= TH_LOW:
            best_idx[i] = idx[b]
            why[i] = "fused"
        else:
            why[i] = "distance > TH_LOW"
    if trace is not None:
        trace.update(why)
    return best_idx, best_dist


def fuse_sim3_search_batch(kfs, Scws, mps, in_kf=None, th=4.0):
    """orbmi_fuse_sim3_search_batch: -> best_idx, best_dist of shape (nkf, n), nfused (nkf)."""
    nkf, n = len(kfs), len(mps)
    bi, bd = np.full((nkf, n), -1, np.int32), np.full((nkf, n), 256, np.int32)
    ink = None if in_kf is None else np.asarray(in_kf, np.uint8).reshape(nkf, n)
    for k in range(nkf):
        bi[k], bd[k] = fuse_sim3_search(kfs[k], Scws[k], mps, None if ink is None else ink[k], th)
    return bi, bd, (bi >= 0).sum(1).astype(np.int32)


# ---- the clause scene ------------------------------------------------------------------------

# the named points of clause_scene
BAD, IN_KF, BEHIND, IMAGE, DISTANCE, NORMAL, EMPTY = 9, 5, 6, 10, 7, 8, 11
OCT_M2, OCT_P1, OCT_M1, OCT_0 = 12, 13, 14, 15
DIST_50, DIST_51, TIE, SHARE_A, SHARE_B, OCCUPIED, FAR = 16, 17, 18, 0, 1, 19, 20
CLAUSE_LEVEL = 3  # the predicted level of the octave-window points


def clause_scene(seed=0, s=1.3, nk=600, npts=300):
    """so.projection_scene without its own special points (point i lands on keypoint perm[i]), then
    one named point per clause of the search:
      BAD, IN_KF (flagged in in_kf), BEHIND, IMAGE, DISTANCE, NORMAL: dropped by that gate
      EMPTY        projects where no keypoint lies within the window
      OCT_M2 / OCT_P1 / OCT_M1 / OCT_0   predicted level 3, its keypoint at octave 1 / 4 / 2 / 3
      DIST_50 / DIST_51   descriptor 50 / 51 bits from its keypoint's
      TIE          two keypoints 1.5 px apart with one descriptor (tie_keys), the point 3 bits away
      SHARE_A / SHARE_B   both on keypoint perm[SHARE_A]
      OCCUPIED     its keypoint holds a point already (occupied[perm[OCCUPIED]] = 1)
      FAR          its keypoint 3 scale[level] px from the projection (chi2 = 9: Fuse(KF, MPs)'s
                   5.99 / 7.8 gate would drop it)
    -> dict(kf, Scw, mps, in_kf, occupied, th, perm, tie_keys)."""
    from orb_slam2_with_comment_amd.types import MP_BAD
    sc = so.projection_scene(seed, nk, npts, s, special=False)
    kf, mps, perm, Scw = sc["kf"], sc["mps"], sc["perm"], sc["Scw"]
    rng = np.random.default_rng(seed + 1000)
    cam, keys, desc = kf.cam, kf.keys, kf.desc
    T, Ow = so.decompose_scw(Scw)
    Rcw, tcw = T[:, :3].astype(F64), T[:, 3].astype(F64)
    scale = np.asarray(kf.scale_factors, F64)
    free = np.setdiff1d(np.arange(nk), perm)  # keypoints no point was built for

    def place(i, x, y, z, level, d):
        Xc = z * np.array([(x - cam.cx) / cam.fx, (y - cam.cy) / cam.fy, 1.0])
        Xw = Rcw.T @ (Xc - tcw)
        PO = Xw - Ow.astype(F64)
        dist = np.linalg.norm(PO)
        mps["pos"][i] = Xw
        mps["normal"][i] = PO / dist
        mps["max_distance"][i] = dist * 1.2 ** (level - 0.5)
        mps["min_distance"][i] = mps["max_distance"][i] / 1.2 ** 7
        mps["desc"][i] = d
        mps["flags"][i] = 0

    def flipped(d, flips):
        d = d.copy()
        for b in rng.choice(256, flips, replace=False):
            d[b >> 3] ^= np.uint8(1 << (b & 7))
        return d

    def on_key(i, k, flips, level=None, du=0.0):
        place(i, float(keys["x"][k]) + du, float(keys["y"][k]), 12.0, int(keys["octave"][k]) if level is None else level,
              flipped(desc[k], flips))

    in_kf = np.zeros(npts, np.uint8)
    occupied = np.zeros(nk, np.uint8)
    mps["flags"][BAD] |= MP_BAD
    in_kf[IN_KF] = 1
    mps["pos"][BEHIND] = Rcw.T @ (np.array([0.0, 0.0, -5.0]) - tcw)
    mps["pos"][IMAGE] = Rcw.T @ (np.array([1000.0, 0.0, 5.0]) - tcw)
    mps["max_distance"][DISTANCE] = 0.5 * np.linalg.norm(mps["pos"][DISTANCE].astype(F64) - Ow.astype(F64))
    mps["normal"][NORMAL] = -mps["normal"][NORMAL]
    # EMPTY: the pixel farthest from every keypoint on a coarse lattice, window of level 0 (4 px)
    gx, gy = np.meshgrid(np.arange(30.0, cam.width - 30, 7), np.arange(30.0, cam.height - 30, 7))
    clear = np.minimum.reduce([np.maximum(np.abs(gx - x), np.abs(gy - y)) for x, y in zip(keys["x"], keys["y"])])
    j = np.unravel_index(np.argmax(clear), clear.shape)
    assert clear[j] > 8
    place(EMPTY, gx[j], gy[j], 12.0, 0, desc[perm[EMPTY]])
    for i, o in ((OCT_M2, -2), (OCT_P1, 1), (OCT_M1, -1), (OCT_0, 0)):
        keys["octave"][perm[i]] = CLAUSE_LEVEL + o
        on_key(i, perm[i], 4, level=CLAUSE_LEVEL)
    on_key(DIST_50, perm[DIST_50], 50)
    on_key(DIST_51, perm[DIST_51], 51)
    # TIE: the keypoint of higher index in the earlier grid column, so that neither "lowest index"
    # nor "last seen" gives the reference's answer
    k1, k2 = sorted((int(perm[TIE]), int(free[0])))
    v = kf.view()
    col = int(np.clip(round(float(keys["x"][k2] - v.min_x) * v.grid_w_inv), 2, 61))
    xb = (col + 0.5) / float(v.grid_w_inv) + float(v.min_x)  # columns col | col + 1 meet here
    keys["x"][k2], keys["x"][k1] = xb - 0.75, xb + 0.75
    keys["y"][k1], keys["octave"][k1] = keys["y"][k2], keys["octave"][k2]
    desc[k1] = desc[k2]
    on_key(TIE, k2, 3)
    on_key(SHARE_A, perm[SHARE_A], 6)
    on_key(SHARE_B, perm[SHARE_A], 0)
    occupied[perm[OCCUPIED]] = 1
    on_key(OCCUPIED, perm[OCCUPIED], 2)
    lev = int(keys["octave"][perm[FAR]])
    on_key(FAR, perm[FAR], 2, du=3.0 * scale[lev])
    return {"kf": kf, "Scw": Scw, "mps": mps, "in_kf": in_kf, "occupied": occupied, "th": 4.0, "perm": perm,
            "tie_keys": (k1, k2)}


def grid_order_first(kf, a, b):
    """Which of keypoints a, b GetFeaturesInArea visits first: by cell (ix * 48 + iy), then index."""
    cell = _grid(kf)[3]
    return min((a, b), key=lambda k: (int(cell[k]), k))


# ---- the restatement backend of loop.search_and_fuse / loop.correct_loop ---------------------------

def distinctive(obs_desc, obs_off):
    """MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:247-316): per point the observation
    whose median distance to the point's observations (itself included; the element at
    int(0.5 (N - 1)) of the sorted row) is least, the first on ties.  -> (np, 32) descriptors."""
    D = np.asarray(obs_desc, np.uint8).reshape(-1, 32)
    out = np.zeros((len(obs_off) - 1, 32), np.uint8)
    for p in range(len(obs_off) - 1):
        d = D[obs_off[p]:obs_off[p + 1]]
        if len(d) == 0:
            continue
        dist = _POPC[d[:, None, :] ^ d[None, :, :]].sum(-1)
        med = np.sort(dist, axis=1)[:, int(0.5 * (len(d) - 1))]
        out[p] = d[int(np.argmin(med))]
    return out


class RestatementBackend:
    """loop.LoopBackend's CorrectLoop operators over the restatements: the search above,
    distinctive, and essgraph_reference.Backend's three."""

    def __init__(self):
        import essgraph_reference as eg
        self._eg = eg.Backend()
        self.calls = []  # (nkf, n) of every fuse_sim3_search
        for name in ("essential_graph_edges", "optimize_essential_graph", "correct_points_sim3"):
            setattr(self, name, getattr(self._eg, name))

    def fuse_sim3_search(self, kfs, Scws, mps, in_kf, th):
        self.calls.append((len(kfs), len(mps)))
        return fuse_sim3_search_batch(kfs, Scws, mps, in_kf, th)

    def distinctive(self, obs_desc, obs_off):
        return distinctive(obs_desc, obs_off)


def batch_case(nkf, n, s=1.3, seed=0):
    """Keyframes of different sizes for one batched call, from clause_scene(seed, s): A its keyframe
    (600 keypoints), A2 the same keypoints under an Scw shifted by 2 cm (some points still land in
    their windows, some do not), K0 without keypoints, K1 the one keypoint a point was built for.
    nkf = 1: [A]; 2: [A2, A]; 3: [A, K0, K1].  The first n points of the scene; in_kf: the scene's
    row for A, a different random row for every other keyframe.
    -> (kfs, Scws, mps, in_kf (nkf, n))."""
    from orb_slam2_with_comment_amd.types import KP_DTYPE, Frame
    sc = clause_scene(seed, s)
    A, Scw = sc["kf"], sc["Scw"]
    one = [int(sc["perm"][min(21, len(sc["perm"]) - 1)])]
    K0 = Frame(np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8), np.zeros(0, F32), np.eye(4), A.cam)
    K1 = Frame(A.keys[one], A.desc[one], np.full(1, -1, F32), np.eye(4), A.cam)
    Scw2 = Scw.copy()
    Scw2[:, 3] += F32(0.02)
    kfs, Scws = {1: ([A], [Scw]), 2: ([A, A], [Scw2, Scw]), 3: ([A, K0, K1], [Scw, Scw2, Scw])}[nkf]
    rng = np.random.default_rng(seed + 7)
    in_kf = (rng.random((nkf, n)) < 0.1).astype(np.uint8)
    in_kf[kfs.index(A) if nkf != 2 else 1] = sc["in_kf"][:n]
    return kfs, Scws, sc["mps"][:n].copy(), in_kf
