"""Crafted inputs for Optimizer::PoseOptimization's device code (k_pose_opt, csrc/pose.hip): the
Levenberg trial chain, the four-round outlier schedule, the frame sizes at the kernel's strides
and the in-kernel edge assembly with Tracking's update pass as its tail.  No GPU here: the scenes
are numpy arrays, and the census helpers run the oracle (oracle/pose_oracle.cpp) alone.
tests/test_pose_edges_cpu.py asserts each scene's census (that the oracle really goes where the
scene is aimed, with margins rounding cannot cross); tests/test_pose_edges_gpu.py runs the kernel
on the same arrays.

Every scene is a Scene: `name`, `aim` (the branch of the kernel it is built for), its inputs
(`frames` / `obs` for the batched call, or `gather` = a GatherInput for the per-frame call) and
`census`, the predicate over the oracle's run that proves the scene reaches its aim.
"""
import functools

import numpy as np

f32 = np.float32
CHI2_TH = (5.991, 7.815)  # mono, stereo (src/Optimizer.cc:258-259, compared in float)

# the margins of a decisive scene (requirements, tests/test_pose_edges_cpu.py)
TRIAL_MARGIN = 1e-4   # every trial's |currentChi - tempChi| / currentChi
STOP_MARGIN = 1e-2    # every 3-bad-iterations test, relative
FLAG_MARGIN = 1e-3    # every classified chi2 from 5.991 / 7.815, relative
ULP_MOVE = 1e-5       # the result under a one-ulp move of one initial pose element


class Scene:
    def __init__(self, name, aim, census, frames=None, obs=None, gather=None, **extra):
        self.name, self.aim, self.census = name, aim, census
        self.frames, self.obs, self.gather = frames, obs, gather
        self.__dict__.update(extra)


def _kitti():
    from orb_slam2_with_comment_amd import synth
    return synth.KITTI


def _second_cam():
    from orb_slam2_with_comment_amd import synth
    return synth.EUROC  # another intrinsic matrix and baseline


def rodrigues(a):
    th = np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]]) / max(th, 1e-300)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def perturbed(seed, n_obs, stereo_frac, rn, tn):
    """An outlier-free frame whose initial pose is far off: pose_problem at a 1e-6 pose noise, then
    tcw <- dT * tcw with dT drawn from default_rng(100 + seed): rotation vector uniform(-1, 1, 3) * rn,
    then translation uniform(-1, 1, 3) * tn."""
    from orb_slam2_with_comment_amd import synth_map as SM
    fr, ob, gt = SM.pose_problem(seed=seed, n_obs=n_obs, stereo_frac=stereo_frac, outlier_frac=0.0,
                                 pose_noise=(1e-6, 1e-6))
    rng = np.random.default_rng(100 + seed)
    rv = rng.uniform(-1, 1, 3) * rn
    tv = rng.uniform(-1, 1, 3) * tn
    dT = np.eye(4)
    dT[:3, :3] = rodrigues(rv)
    dT[:3, 3] = tv
    T = dT @ fr[0]["tcw"].reshape(4, 4).astype(np.float64)
    fr[0]["tcw"] = T.astype(f32).reshape(-1)
    return fr, ob


# ---------------------------------------------------------------- census helpers (oracle only)
def sequence(trials):
    """'A|RRA|...' of one frame's trial record: A accepted, R rejected, '|' between iterations and
    '/' between rounds."""
    s, last = "", None
    for t in trials:
        key = (int(t["round"]), int(t["iteration"]))
        if last is not None and key != last:
            s += "/" if key[0] != last[0] else "|"
        s += "A" if t["accepted"] else "R"
        last = key
    return s


def flag_margin(chi2_rounds, stereo):
    """Smallest relative distance of a classified chi2 from its threshold, per round that ran
    (inf for a round that did not)."""
    th = np.where(stereo, CHI2_TH[1], CHI2_TH[0])
    out = []
    for r in range(4):
        c = chi2_rounds[r].astype(np.float64)
        out.append(float(np.min(np.abs(c - th) / th)) if len(c) and not np.isnan(c).all() else np.inf)
    return out


def oracle_run(oracle, fr, ob):
    """The oracle on one batch -> per frame dict(tcw, inliers, iterations, flags, chi2 (4 x n),
    stop (4 margins), tie (4 margins), trials, seq)."""
    ref = fr.copy()
    out, chi2, margins, trials = oracle.pose_optimization(ref, ob, diag=True, trials=True)
    res = []
    for f in range(len(fr)):
        b, n = int(fr[f]["obs_begin"]), int(fr[f]["n_obs"])
        s = slice(b, b + n)
        res.append(dict(tcw=ref[f]["tcw"].copy(), inliers=int(ref[f]["inliers"]), iterations=int(ref[f]["iterations"]),
                        flags=out[s].copy(), chi2=chi2[:, s].copy(), stop=margins[f][:4].copy(), tie=margins[f][4:].copy(),
                        trials=trials[f], seq=sequence(trials[f]), stereo=~(ob["ur"][s] < 0)))
    return res


def ulp_moves(oracle, fr, ob):
    """The 24 one-ulp moves of the 12 pose elements of frame 0's initial tcw (rows 0-2): the
    largest change of the resulting pose, and whether flags, inliers or iterations moved."""
    base = fr.copy()
    out0 = oracle.pose_optimization(base, ob)
    worst, moved = 0.0, False
    for q in range(12):
        for d in (np.inf, -np.inf):
            g = fr.copy()
            g[0]["tcw"][q] = np.nextafter(fr[0]["tcw"][q], f32(d), dtype=f32)
            out = oracle.pose_optimization(g, ob)
            worst = max(worst, float(np.abs(g[0]["tcw"].astype(np.float64) - base[0]["tcw"]).max()))
            moved |= bool((out != out0).any()) or int(g[0]["inliers"]) != int(base[0]["inliers"]) or \
                int(g[0]["iterations"]) != int(base[0]["iterations"])
    return worst, moved


def decisive_figures(oracle, fr, ob):
    r = oracle_run(oracle, fr, ob)[0]
    rel = r["trials"]["rel"]
    last = max(int(t) for t in r["trials"]["round"]) if len(rel) else 0
    worst, moved = ulp_moves(oracle, fr, ob)
    return dict(seq=r["seq"], iterations=r["iterations"], inliers=r["inliers"], trial_margin=float(rel.min()),
                stop_margin=float(np.min(r["stop"])), flag_margin=flag_margin(r["chi2"], r["stereo"])[last],
                ulp_move=worst, ulp_flips=moved, run=r)


def assert_decisive(fig):
    assert fig["trial_margin"] >= TRIAL_MARGIN, fig["trial_margin"]
    assert fig["stop_margin"] >= STOP_MARGIN, fig["stop_margin"]
    assert fig["flag_margin"] >= FLAG_MARGIN, fig["flag_margin"]
    assert fig["ulp_move"] <= ULP_MOVE and not fig["ulp_flips"], (fig["ulp_move"], fig["ulp_flips"])


# ---------------------------------------------------------------- decisive LM scenes
def _rounds(seq):
    return seq.split("/")


def _has_chain3(seq):
    return "RRRA" in seq


DECISIVE = {
    # name: (n_obs, stereo_frac, seed, rn, tn), aim, predicate over the trial sequence
    "robust_rounds_start_RRA": ((40, 0.7, 8, 0.7, 3.0),
                                "candidate 2 of a fresh chain in rounds 0, 1 and 2 (fresh lambda per round) and a "
                                "rejection in the non-robust round 3; mixed stereo; four rounds of 10 iterations",
                                lambda f: all(r.startswith("RRA") for r in _rounds(f["seq"])[:3]) and f["iterations"] == 40 and
                                _rounds(f["seq"])[3].startswith("RA")),
    "mono9_chain4": ((9, 0.0, 18, 0.5, 2.0),
                     "candidates 3 and 4 of a chain (RRRRA, RRRA); monocular; one round, the 10-iteration cap",
                     lambda f: "RRRRA" in f["seq"] and f["iterations"] == 10 and "/" not in f["seq"]),
    "stereo9_RA": ((9, 0.7, 6, 0.7, 3.0),
                   "candidate 1 of a chain in a mixed-stereo single round (n < 10)",
                   lambda f: "|RA" in f["seq"] and "/" not in f["seq"] and f["iterations"] == 10),
    "mono40_chain3": ((40, 0.0, 15, 0.7, 3.0),
                      "candidate 3 of a chain (RRRA) in a four-round monocular frame with one outlier",
                      lambda f: _has_chain3(f["seq"]) and f["seq"].count("/") == 3),
}


@functools.lru_cache(maxsize=None)
def decisive_scene(name):
    args, aim, pred = DECISIVE[name]
    n, sf, seed, rn, tn = args
    fr, ob = perturbed(seed, n, sf, rn, tn)

    def census(fig):
        assert_decisive(fig)
        assert pred(fig), fig["seq"]
    return Scene(name, aim, census, frames=fr, obs=ob, args=args)


# ---------------------------------------------------------------- round structure
@functools.lru_cache(maxsize=None)
def all_outlier_scene():
    """Every edge an outlier after round 0: rounds 1-3 have no active edge (nact == 0), run no
    trial, and the pose handed back is the initial one."""
    from orb_slam2_with_comment_amd import synth_map as SM
    fr, ob, _ = SM.pose_problem(seed=3, n_obs=300, pose_noise=(0.4, 3.0))

    def census(r):
        th = np.where(r["stereo"], CHI2_TH[1], CHI2_TH[0])
        for rd in range(4):
            c = r["chi2"][rd].astype(np.float64)
            assert (c > th * (1 + FLAG_MARGIN)).all(), rd
        assert r["inliers"] == 0 and r["flags"].all()
        assert r["iterations"] == 10 and set(int(t) for t in r["trials"]["round"]) == {0}
    return Scene("all_outlier", "nact == 0 in rounds 1-3: the rounds skip optimize() and classify at the initial pose",
                 census, frames=fr, obs=ob)


def well_spread(ob, inl):
    """At least 6 inliers that span the image and the depth range: the 6x6 system they leave is
    well conditioned (a quarter of the image each way)."""
    cam = _kitti()
    u, v = ob["u"][inl], ob["v"][inl]
    return int(inl.sum()) >= 6 and np.ptp(u) >= cam.width / 4 and np.ptp(v) >= cam.height / 4


def readmitted(r):
    """Per round r -> r + 1: observations that were outliers after round r and inliers after r + 1."""
    th = np.where(r["stereo"], CHI2_TH[1], CHI2_TH[0])
    out = []
    for rd in range(3):
        a, b = r["chi2"][rd].astype(np.float64), r["chi2"][rd + 1].astype(np.float64)
        out.append(np.nonzero((a > th) & (b <= th))[0])
    return out


READMIT_ARGS = dict(seed=33, n_obs=60, stereo_frac=0.6, outlier_frac=0.4)  # 7 observations come back after round 1


@functools.lru_cache(maxsize=None)
def readmission_scene():
    """Gross outliers bias round 0's robust estimate, so some good observations classify as
    outliers; round 1 runs without the gross ones, and the classification recomputes the
    outliers' errors at the new pose (the quaternion-form pose_error) and takes them back."""
    from orb_slam2_with_comment_amd import synth_map as SM
    fr, ob, _ = SM.pose_problem(**READMIT_ARGS)

    def census(r):
        th = np.where(r["stereo"], CHI2_TH[1], CHI2_TH[0])
        back = readmitted(r)
        best = 0
        for rd in range(3):
            k = back[rd]
            m = np.minimum(np.abs(r["chi2"][rd][k] - th[k]) / th[k], np.abs(r["chi2"][rd + 1][k] - th[k]) / th[k])
            best = max(best, int((m >= FLAG_MARGIN).sum()))
        assert best >= 3, [len(b) for b in back]
        assert well_spread(ob, ~(r["chi2"][0] > th)), "round 0 leaves too few inliers"
        assert min(flag_margin(r["chi2"], r["stereo"])) >= FLAG_MARGIN
    return Scene("readmission", "outl[k] set: the classification's fresh pose_error and the flag going back to 0",
                 census, frames=fr, obs=ob)


N_BEHIND, N_NEAR = 4, 4


@functools.lru_cache(maxsize=None)
def behind_camera_scene():
    """A few map points behind the camera (z = -5 m) and a few nearer than 0.1 m, each 2 m / 0.1 m
    off its ray so its projection is hundreds of pixels away: gross outliers in every round,
    through 1 / z < 0 and 1 / z > 10; the other observations converge."""
    from orb_slam2_with_comment_amd import synth_map as SM
    n = 300
    fr, ob, gt = SM.pose_problem(seed=29, n_obs=n, stereo_frac=0.6, outlier_frac=0.0, pose_noise=(0.005, 0.02))
    cam, T = _kitti(), gt[0]
    Twc = np.linalg.inv(T)
    idx = np.arange(N_BEHIND + N_NEAR) * 9 + 2
    for j, k in enumerate(idx):
        z, off = (-5.0, 2.0) if j < N_BEHIND else (0.05, 0.1)
        Xc = np.array([(ob["u"][k] - cam.cx) * z / cam.fx + off, (ob["v"][k] - cam.cy) * z / cam.fy, z, 1.0])
        ob["Xw"][k] = (Twc @ Xc)[:3].astype(f32)
    ob["ur"][idx[::2]] = -1.0  # both kinds of edge among them
    ob["ur"][idx[1::2]] = ob["u"][idx[1::2]] - 3.0

    def census(r):
        th = np.where(r["stereo"], CHI2_TH[1], CHI2_TH[0])
        for rd in range(4):
            assert (r["chi2"][rd][idx] > 100 * th[idx]).all(), rd
        assert r["flags"][idx].all() and r["inliers"] >= 0.85 * n  # ~5% of good ones exceed the 95% quantile
        assert well_spread(ob, ~(r["chi2"][0] > th))
        assert np.abs(r["tcw"].reshape(4, 4) - T).max() < 0.01
        assert min(flag_margin(r["chi2"], r["stereo"])) >= FLAG_MARGIN
        Xc = ob["Xw"][idx].astype(np.float64) @ r["tcw"].reshape(4, 4)[:3, :3].T + r["tcw"].reshape(4, 4)[:3, 3]
        assert (Xc[:N_BEHIND, 2] < 0).all() and ((Xc[N_BEHIND:, 2] > 0) & (Xc[N_BEHIND:, 2] < 0.1)).all()
    return Scene("behind_camera", "1 / z negative and 1 / z > 10 in the error, the Huber weight and the Jacobian",
                 census, frames=fr, obs=ob, idx=idx)


# ---------------------------------------------------------------- the size set
SIZES = (0, 1, 2, 3, 4, 9, 10, 11, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4095, 4096)
GAP_SENTINEL = 0xA5


@functools.lru_cache(maxsize=None)
def size_scene():
    """One batch, one frame per size at and around the kernel's strides (64 lanes, 256 threads of
    buildSystem, 512 of a trial, 4096 edges of LDS), ~10% outliers so skipped edges straddle each
    stride; the observation ranges lie in shuffled order with unused gaps between them, and the
    frames alternate between two cameras.  `gaps` = mask of observations no frame owns."""
    from orb_slam2_with_comment_amd import synth_map as SM
    from orb_slam2_with_comment_amd.types import POSE_FRAME_DTYPE, POSE_OBS_DTYPE
    rng = np.random.default_rng(77)
    order = rng.permutation(len(SIZES))
    gap = rng.integers(1, 40, len(SIZES) + 1)
    total = int(sum(SIZES) + gap.sum())
    frames = np.zeros(len(SIZES), POSE_FRAME_DTYPE)
    obs = np.zeros(total, POSE_OBS_DTYPE)
    owned = np.zeros(total, bool)
    pos = int(gap[0])
    for slot, f in enumerate(order):
        n = SIZES[f]
        cam = _kitti() if f % 2 == 0 else _second_cam()
        fr, ob, _ = SM.pose_problem(seed=300 + int(f), n_obs=max(n, 1), stereo_frac=0.7, outlier_frac=0.1, cam=cam)
        frames[f] = fr[0]
        frames[f]["obs_begin"], frames[f]["n_obs"] = pos, n
        obs[pos:pos + n] = ob[:n]
        owned[pos:pos + n] = True
        pos += n + int(gap[slot + 1])
    assert pos == total

    def census(runs):
        assert tuple(int(n) for n in frames["n_obs"]) == SIZES
        b = frames["obs_begin"].astype(np.int64)
        assert (np.diff(b) < 0).any() and (np.diff(b) > 0).any()          # shuffled
        ends = sorted((int(b[f]), int(b[f] + frames[f]["n_obs"])) for f in range(len(SIZES)))
        assert ends[0][0] > 0 and all(e0[1] < e1[0] for e0, e1 in zip(ends, ends[1:])) and ends[-1][1] < total
        assert int(owned.sum()) == sum(SIZES) and len({(float(x["fx"]), float(x["bf"])) for x in frames}) == 2
        for f, r in enumerate(runs):
            n = SIZES[f]
            nr = len(set(int(t) for t in r["trials"]["round"]))
            assert nr == (0 if n < 3 else 1 if n < 10 else 4), (n, nr)
            if n >= 63:
                assert 0.03 * n <= r["flags"].sum() <= 0.2 * n, (n, int(r["flags"].sum()))
    return Scene("sizes", "every loop stride of the edge passes and reductions; obs_begin of any order", census,
                 frames=frames, obs=obs, gaps=~owned)


# ---------------------------------------------------------------- gather scenes
class GatherInput:
    """A crafted Frame with its match arrays, as PoseOptimization(Frame*) takes it.  `clamped` is
    the frame the oracle gets (octaves clamped into [0, nlevels - 1] as the device clamps them);
    `n_device` < len(keys) truncates the frame on the device path."""

    def __init__(self, frame, sig, match_lf, lfp, match_mp, mps, clamped=None, n_device=None, cats=None):
        self.frame, self.sig, self.match_lf, self.lfp, self.match_mp, self.mps = frame, sig, match_lf, lfp, match_mp, mps
        self.clamped = clamped or frame
        self.n_device = n_device
        self.cats = cats or {}


def _sigma(nlevels):
    s, out = f32(1), []
    for _ in range(nlevels):
        out.append(s)
        s = f32(np.float64(s) * np.float64(f32(1.2)))
    s = np.array(out, f32)
    return s, (f32(1.0) / (s * s).astype(f32)).astype(f32)


def point_of(match_lf, n_lf, match_mp, n_mp, i):
    """'mp' / 'lf' / None: where keypoint i's point comes from (the map point wins)."""
    if match_mp is not None and 0 <= match_mp[i] < n_mp:
        return "mp"
    if match_lf is not None and 0 <= match_lf[i] < n_lf:
        return "lf"
    return None


BAD_INDEX = (-5, None, 1 << 30)  # None = the array's own length (the first index out of range)


def build_gather(nk, source, seed, stereo=True, nlevels=8, wild_octaves=False, share=0.5, n_device=None):
    """nk keypoints, `share` of them holding a point.  source: 'lf', 'mp', 'both' or 'neither'.
    With 'both', a third of the points sit in each array alone and a third of the keypoints hold
    both (the last-frame entry then points at a decoy 3 m off: the map point must win), a share of
    the lf-only ones carry an out-of-range match_mp, and keypoints without a point carry -1 or an
    out-of-range index in either array."""
    from orb_slam2_with_comment_amd import synth_map as SM
    from orb_slam2_with_comment_amd.types import KP_DTYPE, LFPOINT_DTYPE, MAPPOINT_DTYPE, MP_HAS_OBS, Frame
    rng = np.random.default_rng(seed)
    cam = _kitti()
    scale, sig = _sigma(nlevels)
    fr, ob, _ = SM.pose_problem(seed=seed, n_obs=max(nk, 1), stereo_frac=0.7, outlier_frac=0.1)
    ob = ob[:nk]
    keys = np.zeros(nk, KP_DTYPE)
    keys["x"], keys["y"], keys["size"], keys["angle"], keys["response"] = ob["u"], ob["v"], 31.0, 0.0, 1.0
    # the level whose sigma the observation's noise was drawn with (pose_problem: by depth)
    octave = np.rint(-np.log(ob["inv_sigma2"].astype(np.float64)) / (2 * np.log(1.2))).astype(np.int64) % nlevels
    keys["octave"] = octave
    keys["class_id"] = -1
    ur = ob["ur"].copy() if stereo else None
    holds = rng.random(nk) < share if source != "neither" else np.zeros(nk, bool)
    if source == "both":
        kind = rng.integers(0, 3, nk)  # 0 = lf only, 1 = mp only, 2 = both
    else:
        kind = np.full(nk, 0 if source == "lf" else 1)
    use_lf, use_mp = source in ("lf", "both", "neither"), source in ("mp", "both", "neither")
    n_lf = max(int((holds & (kind != 1)).sum()), 1) + 3 if use_lf else 0
    n_mp = max(int((holds & (kind != 0)).sum()), 1) + 3 if use_mp else 0
    lfp, mps = np.zeros(n_lf, LFPOINT_DTYPE), np.zeros(n_mp, MAPPOINT_DTYPE)
    match_lf = np.full(max(nk, 1), -1, np.int32) if use_lf else None
    match_mp = np.full(max(nk, 1), -1, np.int32) if use_mp else None
    slots_lf, slots_mp = list(rng.permutation(n_lf)), list(rng.permutation(n_mp))
    cats = dict(lf=0, mp=0, both=0, none=0, mp_bad_lf_ok=0, bad_index=0, has_obs_lf=0, has_obs_mp=0, no_obs_lf=0,
                no_obs_mp=0, mono_edges=0, stereo_edges=0)
    for i in range(nk):
        bad = BAD_INDEX[int(rng.integers(0, 3))]
        if not holds[i]:
            cats["none"] += 1
            if rng.random() < 0.5:  # out-of-range indices on a keypoint without a point
                cats["bad_index"] += 1
                if use_lf:
                    match_lf[i] = n_lf if bad is None else bad
                if use_mp and rng.random() < 0.5:
                    match_mp[i] = n_mp if bad is None else bad
            continue
        obs_flag = MP_HAS_OBS if rng.random() < 0.6 else 0
        if kind[i] != 1:  # a last-frame point
            j = slots_lf.pop()
            match_lf[i] = j
            lfp[j]["pos"] = ob["Xw"][i]
            lfp[j]["flags"] = 1 | obs_flag
        if kind[i] != 0:  # a map point
            j = slots_mp.pop()
            match_mp[i] = j
            mps[j]["pos"] = ob["Xw"][i]
            mps[j]["flags"] = obs_flag
        if kind[i] == 2:  # both: the last-frame point is a decoy with the opposite flag
            cats["both"] += 1
            lfp[match_lf[i]]["pos"] = ob["Xw"][i] + f32(3.0)
            lfp[match_lf[i]]["flags"] = 1 | (MP_HAS_OBS ^ obs_flag)
        elif kind[i] == 0 and use_mp and rng.random() < 0.4:
            match_mp[i] = n_mp if bad is None else bad  # match_mp out of range, match_lf valid
            cats["mp_bad_lf_ok"] += 1
        src = "mp" if kind[i] != 0 else "lf"
        cats[src] += 1
        cats[("has_obs_" if obs_flag else "no_obs_") + src] += 1
        cats["stereo_edges" if (stereo and ur[i] >= 0) else "mono_edges"] += 1
    frame = Frame(keys, np.zeros((nk, 32), np.uint8), ur, fr[0]["tcw"].reshape(4, 4), cam, scale_factors=scale)
    clamped = None
    if wild_octaves:  # the device clamps kp.octave into [0, nlevels - 1]; the oracle indexes with it
        wild = keys.copy()
        wild["octave"] = np.where(np.arange(nk) % 3 == 0, -1, np.where(np.arange(nk) % 3 == 1, 9, keys["octave"]))
        ck = wild.copy()
        ck["octave"] = np.clip(wild["octave"], 0, nlevels - 1)
        clamped = Frame(ck, frame.desc, ur, frame.tcw, cam, scale_factors=scale)
        frame = Frame(wild, frame.desc, ur, frame.tcw, cam, scale_factors=scale)
    cats["edges"] = cats["lf"] + cats["mp"]
    return GatherInput(frame, sig, match_lf, lfp, match_mp, mps, clamped=clamped, n_device=n_device, cats=cats)


def build_overflow():
    """5000 keypoints, every one matched: more edges than the kernel's LDS holds (4096)."""
    g = build_gather(5000, "both", 55, share=1.1)
    return g


GATHER = {
    # name: (builder arguments, aim)
    "k0": (dict(nk=0, source="both", seed=40), "no keypoint: per == 0"),
    "k1": (dict(nk=1, source="both", seed=41, share=1.1), "one edge: n < 3, pose untouched"),
    "k2": (dict(nk=2, source="both", seed=42, share=1.1), "two edges: n < 3"),
    "k3": (dict(nk=3, source="both", seed=43, share=1.1), "three edges: the smallest frame that optimises"),
    "k511_lf": (dict(nk=511, source="lf", seed=44), "per = 1 with an idle last thread; match_mp NULL"),
    "k512_mp": (dict(nk=512, source="mp", seed=45), "per = 1, every thread one keypoint; match_lf NULL"),
    "k513_both": (dict(nk=513, source="both", seed=46), "per = 2: first count past one keypoint per thread"),
    "k4096_both": (dict(nk=4096, source="both", seed=47), "per = 8: the last count on the batched-load branch"),
    "k4097_both": (dict(nk=4097, source="both", seed=48), "per = 9: the first count on the one-at-a-time branch"),
    "k6000_both": (dict(nk=6000, source="both", seed=49), "per = 12, one-at-a-time branch, ~3000 edges"),
    "neither": (dict(nk=200, source="neither", seed=50), "match arrays present, no index in range: zero edges"),
    "mono": (dict(nk=300, source="both", seed=51, stereo=False), "u_right NULL: monocular edges, stage 1 keeps outliers' slots"),
    "one_level": (dict(nk=300, source="both", seed=52, nlevels=1), "nlevels = 1"),
    "wild_octaves": (dict(nk=300, source="both", seed=53, wild_octaves=True), "octaves -1 and 9: the clamp"),
    "n_device": (dict(nk=600, source="both", seed=54, n_device=389), "n_device < n: the device count truncates"),
}


@functools.lru_cache(maxsize=None)
def gather_scene(name):
    if name == "overflow":
        g = build_overflow()
        aim = "more than 4096 edges: inliers = -1, the tail's keypoint form"
    else:
        kw, aim = GATHER[name]
        g = build_gather(**kw)

    def census(counted):
        """counted: dict from count_gather (the independent walk over the match arrays)."""
        for k in ("edges", "lf", "mp", "both", "mp_bad_lf_ok", "stereo_edges", "mono_edges"):
            assert counted[k] == g.cats[k], (k, counted[k], g.cats[k])
    return Scene(name, aim, census, gather=g)


def count_gather(g, n=None):
    """An independent walk over the match arrays: edges and their categories among the first n
    keypoints."""
    from orb_slam2_with_comment_amd.types import MP_HAS_OBS
    nk = len(g.frame.keys) if n is None else n
    c = dict(edges=0, lf=0, mp=0, both=0, mp_bad_lf_ok=0, stereo_edges=0, mono_edges=0, has_obs=0, index=[])
    for i in range(nk):
        src = point_of(g.match_lf, len(g.lfp), g.match_mp, len(g.mps), i)
        if src is None:
            continue
        c["edges"] += 1
        c[src] += 1
        c["index"].append(i)
        lf_ok = g.match_lf is not None and 0 <= g.match_lf[i] < len(g.lfp)
        if src == "mp" and lf_ok:
            c["both"] += 1
        if src == "lf" and g.match_mp is not None and g.match_mp[i] != -1:
            c["mp_bad_lf_ok"] += 1
        fl = g.mps[g.match_mp[i]]["flags"] if src == "mp" else g.lfp[g.match_lf[i]]["flags"]
        c["has_obs"] += bool(fl & MP_HAS_OBS)
        st = g.frame.u_right is not None and g.frame.u_right[i] >= 0
        c["stereo_edges" if st else "mono_edges"] += 1
    return c
