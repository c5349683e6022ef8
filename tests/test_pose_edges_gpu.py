"""GPU parity of k_pose_opt (csrc/pose.hip) on the crafted scenes of tests/pose_scenes.py, whose
census tests/test_pose_edges_cpu.py proves on the oracle alone.

  * decisive LM scenes: no decision of the oracle's run is within rounding of a tie, so LM
    iterations, outlier flags and the inlier count are compared EXACTLY (plain assertions, no
    lenient branch) and the pose within POSE_TOL = 1e-4;
  * round-structure and size scenes: the bars of tests/test_pose_gpu.py (check_flags /
    check_iterations), plus what each scene is about (all flags set, pose untouched, bytes of the
    flag array no frame owns);
  * the API's edges: range checks of the host path, inliers = -1 of the device path;
  * gather scenes through PoseOptimization (host arrays) against oracle.pose_optimization_frame,
    and through PoseOptimizationTrack (device arrays, stages 0 and 1) against
    oracle.track_update_matches on the GPU's own flags, byte for byte against the unfused pair of
    calls and against the same call with the initial pose in device memory.

No call here hands the device path a range that leaves its buffer.

Measured on an MI355X: the float pose record equals the oracle's in every scene (largest
difference 0.0, decisive scenes included; the double results round to the same floats); the
readmission scene runs 20 iterations against the oracle's 19 on a trial with a chi2 change of 0
(the lenient branch of check_iterations, as in tests/test_pose_gpu.py).  Every test's call takes
0.02 s or less; the first one also pays ~5 s of library and device start-up.

What bites (each mutation of csrc/pose.hip applied alone, this file run against it):
  1. pose_candidates without `nn *= 2`       test_decisive_scene_exact[mono9_chain4] (6 iterations
                                             for 10), [mono40_chain3] (10 for 40); also behind_camera
                                             and wild_octaves by their iteration counts
  2. pose_reduce28_w0 sums one wave fewer    test_size_set_one_launch, test_size_set_device_arrays_keep_the_gaps,
                                             all_outlier, behind_camera, every gather scene >= 511
  3. no fresh error for outl[k]              test_round_structure_scene[readmission_scene], behind_camera,
                                             the size set, the gather scenes
  4. point_ref prefers the last-frame point  every `both` gather scene, host and fused (k513_both, ...)
  5. stage 1 drops `if (stereo)`             test_gather_scene_fused_track_update[mono-1], and only it"""
import ctypes as C

import numpy as np
import pytest

import pose_scenes as S
from test_pose_gpu import check_flags, check_iterations

pytestmark = pytest.mark.gpu
POSE_TOL = 1e-4
SENTINEL = S.GAP_SENTINEL


@pytest.fixture(scope="module")
def PO():
    from orb_slam2_with_comment_amd.optimizer import PoseOptimizer
    return PoseOptimizer()


@pytest.fixture(scope="module")
def matcher():
    from orb_slam2_with_comment_amd.matcher import ORBmatcher
    m = ORBmatcher(device=0)
    yield m
    m.close()


def dev(a):
    """A device copy of a numpy array's bytes (torch uint8 tensor; at least one byte)."""
    import torch
    b = np.frombuffer(np.ascontiguousarray(a).tobytes() or b"\0", np.uint8).copy()
    return torch.from_numpy(b).cuda()


def host(t, dtype, n=None):
    a = t.cpu().numpy().view(dtype)
    return a.copy() if n is None else a[:n].copy()


def sync():
    import torch
    torch.cuda.synchronize()


def run_on_device(PO, fr, ob, flags_fill=SENTINEL):
    """orbmi_pose_optimization on device arrays -> (frames, flag bytes) read back."""
    from orb_slam2_with_comment_amd.types import POSE_FRAME_DTYPE
    dF, dO = dev(fr), dev(ob)
    dX = dev(np.full(max(len(ob), 1), flags_fill, np.uint8))
    PO.run_device(dF.data_ptr(), len(fr), dO.data_ptr(), len(ob), dX.data_ptr())
    PO.synchronize()
    sync()
    return host(dF, POSE_FRAME_DTYPE, len(fr)), host(dX, np.uint8, len(ob))


# ---------------------------------------------------------------- decisive LM scenes
def _exact(fr, out, ref, tag):
    d = float(np.abs(fr[0]["tcw"].astype(np.float64) - ref["tcw"]).max())
    print(f"{tag}: pose difference {d:.3e}, iterations {int(fr[0]['iterations'])} (oracle {ref['iterations']}), "
          f"inliers {int(fr[0]['inliers'])} (oracle {ref['inliers']}), oracle trials {ref['seq']}")
    assert int(fr[0]["iterations"]) == ref["iterations"], tag
    np.testing.assert_array_equal(np.asarray(out, bool), ref["flags"], err_msg=tag)
    assert int(fr[0]["inliers"]) == ref["inliers"], tag
    assert d <= POSE_TOL, (tag, d)


@pytest.mark.parametrize("name", list(S.DECISIVE))
def test_decisive_scene_exact(oracle, PO, name):
    sc = S.decisive_scene(name)
    ref = S.oracle_run(oracle, sc.frames, sc.obs)[0]
    fr = sc.frames.copy()
    out = PO.run(fr, sc.obs)
    _exact(fr, out, ref, name)


def test_decisive_scene_exact_device_path(oracle, PO):
    sc = S.decisive_scene("robust_rounds_start_RRA")
    ref = S.oracle_run(oracle, sc.frames, sc.obs)[0]
    fr, out = run_on_device(PO, sc.frames, sc.obs)
    _exact(fr, out, ref, "robust_rounds_start_RRA (device arrays)")


# ---------------------------------------------------------------- round structure, sizes
def _usual(fr, out, ob, refs, tag=""):
    """The bars of tests/test_pose_gpu.py, frame by frame; returns the largest pose difference."""
    worst = 0.0
    for f, ref in enumerate(refs):
        d = float(np.abs(fr[f]["tcw"].astype(np.float64) - ref["tcw"]).max())
        worst = max(worst, d)
        assert d <= POSE_TOL, (tag, f, d)
        b, n = int(fr[f]["obs_begin"]), int(fr[f]["n_obs"])
        s = slice(b, b + n)
        nd = check_flags(out[s], ref["flags"], ref["chi2"], ref["stereo"], tag=f"{tag} frame {f}")
        if n >= 3:
            assert int(fr[f]["inliers"]) == n - int(np.asarray(out[s], bool).sum())
        assert abs(int(fr[f]["inliers"]) - ref["inliers"]) <= nd
        check_iterations(fr[f]["iterations"], ref["iterations"], np.concatenate([ref["stop"], ref["tie"]]),
                         tag=f"{tag} frame {f}")
    print(f"{tag}: largest pose difference {worst:.3e}")
    return worst


def test_all_outlier_rounds_skip_the_optimisation(oracle, PO):
    sc = S.all_outlier_scene()
    refs = S.oracle_run(oracle, sc.frames, sc.obs)
    fr = sc.frames.copy()
    out = PO.run(fr, sc.obs)
    _usual(fr, out, sc.obs, refs, "all_outlier")
    assert out.all() and int(fr[0]["inliers"]) == 0 and int(fr[0]["iterations"]) == refs[0]["iterations"] == 10
    # rounds 1-3 optimise nothing: the pose handed back is the initial one (float -> quaternion -> float)
    assert np.abs(fr[0]["tcw"].astype(np.float64) - sc.frames[0]["tcw"]).max() <= 1e-6


@pytest.mark.parametrize("scene", ["readmission_scene", "behind_camera_scene"])
def test_round_structure_scene(oracle, PO, scene):
    sc = getattr(S, scene)()
    refs = S.oracle_run(oracle, sc.frames, sc.obs)
    fr = sc.frames.copy()
    out = PO.run(fr, sc.obs)
    _usual(fr, out, sc.obs, refs, sc.name)
    if scene == "readmission_scene":  # the observations round 1 took back are inliers here too
        back = S.readmitted(refs[0])[0]
        assert len(back) >= 3 and not out[back][~refs[0]["flags"][back]].any()
    else:
        assert out[sc.idx].all()


@pytest.fixture(scope="module")
def size_refs(oracle):
    sc = S.size_scene()
    return S.oracle_run(oracle, sc.frames, sc.obs)


def _small_frames_untouched(fr, out, sc):
    for f, n in enumerate(S.SIZES):
        if n < 3:
            assert fr[f]["tcw"].tobytes() == sc.frames[f]["tcw"].tobytes()
            assert int(fr[f]["inliers"]) == 0 and int(fr[f]["iterations"]) == 0
            b = int(fr[f]["obs_begin"])
            assert not np.asarray(out[b:b + n]).any()


def test_size_set_one_launch(PO, size_refs):
    sc = S.size_scene()
    fr = sc.frames.copy()
    out = PO.run(fr, sc.obs)
    _usual(fr, out, sc.obs, size_refs, "sizes")
    _small_frames_untouched(fr, out, sc)


def test_size_set_device_arrays_keep_the_gaps(PO, size_refs):
    sc = S.size_scene()
    fr, out = run_on_device(PO, sc.frames, sc.obs)
    assert (out[sc.gaps] == SENTINEL).all(), "a flag byte no frame owns was written"
    assert set(np.unique(out[~sc.gaps]).tolist()) <= {0, 1}
    _usual(fr, out.astype(bool) & ~sc.gaps, sc.obs, size_refs, "sizes (device arrays)")
    _small_frames_untouched(fr, out * ~sc.gaps, sc)
    # the same kernel on the same bytes: the staged host path gives the same answer
    fr_h = sc.frames.copy()
    out_h = PO.run(fr_h, sc.obs)
    assert fr_h.tobytes() == fr.tobytes()
    np.testing.assert_array_equal(out_h[~sc.gaps], out[~sc.gaps].astype(bool))


# ---------------------------------------------------------------- API edges
def _call(PO, frames, nframes, obs, nobs, out):
    from orb_slam2_with_comment_amd._capi import lib
    p = lambda a: a if isinstance(a, int) or a is None else a.ctypes.data  # noqa: E731
    return lib().orbmi_pose_optimization(PO._h, p(frames), nframes, p(obs), nobs, p(out))


def test_host_path_checks_its_ranges(PO):
    from orb_slam2_with_comment_amd import _capi
    from orb_slam2_with_comment_amd import synth_map as SM
    fr, ob, _ = SM.pose_problem(seed=60, n_obs=4097, outlier_frac=0.0)
    out = np.zeros(len(ob), np.uint8)
    f0 = fr.copy()
    assert _call(PO, fr, 1, ob, len(ob), out) == _capi.ORBMI_E_UNSUPPORTED  # 4097 observations
    for begin, n in ((0, -1), (-1, 5), (4090, 8), (4097, 1)):                # negative, past nobs
        g = f0.copy()
        g[0]["obs_begin"], g[0]["n_obs"] = begin, n
        assert _call(PO, g, 1, ob, len(ob), out) == _capi.ORBMI_E_ARG, (begin, n)
    assert fr.tobytes() == f0.tobytes() and not out.any()
    g = f0.copy()
    g[0]["n_obs"] = 100
    d_ob = dev(ob)
    assert _call(PO, g, 1, d_ob.data_ptr(), len(ob), out) == _capi.ORBMI_E_ARG   # host frames, device obs
    d_out = dev(out)
    assert _call(PO, g, 1, ob, len(ob), d_out.data_ptr()) == _capi.ORBMI_E_ARG   # host frames, device flags
    assert _call(PO, None, 0, None, 0, None) == _capi.ORBMI_OK
    h = g.copy()
    assert _call(PO, g, 0, ob, len(ob), out) == _capi.ORBMI_OK and g.tobytes() == h.tobytes() and not out.any()
    assert _call(PO, g, 1, ob, len(ob), out) == _capi.ORBMI_OK and int(g[0]["iterations"]) > 0


def test_device_path_reports_too_many_observations(PO):
    """n_obs = 4097 in a buffer that holds 4097 observations: inliers = -1, nothing else written."""
    from orb_slam2_with_comment_amd import synth_map as SM
    fr, ob, _ = SM.pose_problem(seed=61, n_obs=4097, outlier_frac=0.0)
    got, flags = run_on_device(PO, fr, ob)
    assert int(got[0]["inliers"]) == -1 and int(got[0]["iterations"]) == 0
    assert got[0]["tcw"].tobytes() == fr[0]["tcw"].tobytes()
    assert (flags == SENTINEL).all()


# ---------------------------------------------------------------- gather scenes, host arrays
def _mp_struct(g, match_lf, match_mp, lfp, mps):
    """orbmi_frame_mappoints over addresses or arrays (None = the array is absent)."""
    from orb_slam2_with_comment_amd.types import FrameMapPoints
    p = lambda a: a if isinstance(a, int) else a.ctypes.data  # noqa: E731
    mp = FrameMapPoints()
    if g.match_lf is not None:
        mp.match_lf, mp.lf_points, mp.n_lf_points = p(match_lf), p(lfp), len(g.lfp)
    if g.match_mp is not None:
        mp.match_mp, mp.mps, mp.n_mps = p(match_mp), p(mps), len(g.mps)
    return mp


def _copy(a):
    return None if a is None else a.copy()


def _oracle_frame(oracle, g, n=None):
    """oracle.pose_optimization_frame on the first n keypoints of the scene's (clamped) frame."""
    from orb_slam2_with_comment_amd.types import Frame
    fr = g.clamped
    if n is not None:
        fr = Frame(fr.keys[:n], fr.desc[:n], None if fr.u_right is None else fr.u_right[:n], fr.tcw, fr.cam,
                   scale_factors=fr.scale_factors)
    cut = (lambda a: None if a is None else a[:max(len(fr.keys), 1)].copy())
    return fr, oracle.pose_optimization_frame(fr, g.sig, cut(g.match_lf), g.lfp, cut(g.match_mp), g.mps, diag=True)


def _cmp_frame(rec, flags, ref, u_right, nk, tag, with_point):
    """The record and the per-keypoint flags of the first nk keypoints against the oracle's, at the
    usual bars; with_point = the keypoints that hold a point (every other flag is 0)."""
    ref_rec, ref_out, chi2, margins = ref
    d = float(np.abs(rec["tcw"].astype(np.float64) - ref_rec["tcw"]).max())
    print(f"{tag}: {int(ref_rec['n_obs'])} edges, pose difference {d:.3e}")
    assert d <= POSE_TOL, (tag, d)
    assert int(rec["n_obs"]) == int(ref_rec["n_obs"])
    stereo = np.zeros(nk, bool) if u_right is None else np.asarray(u_right[:nk]) >= 0
    nd = check_flags(flags[:nk], ref_out, chi2, stereo, tag=tag)
    assert abs(int(rec["inliers"]) - int(ref_rec["inliers"])) <= nd
    check_iterations(rec["iterations"], ref_rec["iterations"], margins, tag=tag)
    assert int(ref_rec["n_obs"]) == len(with_point)
    assert not np.asarray(flags[:nk])[np.setdiff1d(np.arange(nk), with_point)].any(), "flag on a keypoint without a point"
    assert set(np.unique(flags[:nk]).tolist()) <= {0, 1}
    if len(with_point) < 3:
        assert not np.asarray(flags[:nk]).any()


@pytest.mark.parametrize("name", [n for n in S.GATHER if n != "n_device"])
def test_gather_scene_host_arrays(oracle, PO, name):
    from orb_slam2_with_comment_amd.types import POSE_FRAME_DTYPE
    g = S.gather_scene(name).gather
    nk = len(g.frame.keys)
    _, ref = _oracle_frame(oracle, g)
    lf, mpm = _copy(g.match_lf), _copy(g.match_mp)
    mp = _mp_struct(g, lf, mpm, g.lfp, g.mps)
    rec = np.zeros(1, POSE_FRAME_DTYPE)
    out = np.full(max(nk, 1), 1, np.uint8)  # every keypoint's flag is written: none stays 1 without a reason
    v = g.frame.view()
    PO.PoseOptimization(v, g.sig, mp, rec, out)
    _cmp_frame(rec[0], out, ref, g.frame.u_right, nk, name, S.count_gather(g)["index"])
    if int(ref[0]["n_obs"]) < 3:
        assert rec[0]["tcw"].tobytes() == g.frame.tcw.astype(np.float32).tobytes()
        assert int(rec[0]["inliers"]) == 0 and int(rec[0]["iterations"]) == 0
    for a, b in ((lf, g.match_lf), (mpm, g.match_mp)):  # no update pass here: the match arrays are inputs
        if a is not None:
            np.testing.assert_array_equal(a, b)


def test_gather_overflow_host_arrays_is_unsupported(PO):
    from orb_slam2_with_comment_amd import _capi
    from orb_slam2_with_comment_amd.types import POSE_FRAME_DTYPE
    g = S.gather_scene("overflow").gather
    mp = _mp_struct(g, g.match_lf.copy(), g.match_mp.copy(), g.lfp, g.mps)
    rec, out = np.zeros(1, POSE_FRAME_DTYPE), np.zeros(len(g.frame.keys), np.uint8)
    v = g.frame.view()
    with pytest.raises(_capi.OrbmiError) as e:
        PO.PoseOptimization(v, g.sig, mp, rec, out)
    assert e.value.code == _capi.ORBMI_E_UNSUPPORTED


# ---------------------------------------------------------------- gather scenes, device arrays + the fused tail
TAIL = 64  # sentinel elements behind every per-keypoint device array


class DeviceFrame:
    """The scene's arrays in device memory, each with TAIL sentinel elements behind the keypoints."""

    def __init__(self, g, tcw_on_device=False):
        from orb_slam2_with_comment_amd.types import KP_DTYPE
        f = g.frame
        nk = self.nk = len(f.keys)
        self.g = g
        self.keys = dev(np.concatenate([f.keys, np.zeros(1, KP_DTYPE)]))
        self.ur = None if f.u_right is None else dev(np.concatenate([f.u_right, np.zeros(1, np.float32)]))
        self.desc = dev(np.zeros((max(nk, 1), 32), np.uint8))
        pad = lambda a: None if a is None else dev(np.concatenate([a[:nk], np.full(TAIL, -77, np.int32)]))  # noqa: E731
        self.lf, self.mpm = pad(g.match_lf), pad(g.match_mp)
        self.lfp, self.mps = dev(g.lfp), dev(g.mps)
        self.rec = dev(np.full(128, SENTINEL, np.uint8))
        self.outlier = dev(np.full(nk + TAIL, SENTINEL, np.uint8))
        self.occ = dev(np.full(nk + TAIL, SENTINEL, np.uint8))
        self.counts = dev(np.full(2, -9, np.int32))
        self.tcw = dev(f.tcw.astype(np.float32)) if tcw_on_device else None
        self.n_dev = None if g.n_device is None else dev(np.array([g.n_device], np.int32))
        v = f.view()
        v.keys_un = self.keys.data_ptr()
        v.u_right = None if self.ur is None else self.ur.data_ptr()
        v.desc = self.desc.data_ptr()
        if self.tcw is not None:
            v.tcw = self.tcw.data_ptr()
        if self.n_dev is not None:
            v.n_device = self.n_dev.data_ptr()
        self.view = v
        ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
        self.mp = _mp_struct(g, ptr(self.lf), ptr(self.mpm), self.lfp.data_ptr(), self.mps.data_ptr())

    def results(self):
        from orb_slam2_with_comment_amd.types import POSE_FRAME_DTYPE
        sync()
        r = dict(rec=host(self.rec, np.uint8), outlier=host(self.outlier, np.uint8), occ=host(self.occ, np.uint8),
                 counts=host(self.counts, np.int32))
        r["lf"] = None if self.lf is None else host(self.lf, np.int32)
        r["mpm"] = None if self.mpm is None else host(self.mpm, np.int32)
        r["frame"] = r["rec"][:POSE_FRAME_DTYPE.itemsize].view(POSE_FRAME_DTYPE)[0]
        return r


def _fused(PO, g, stage, tcw_on_device=False):
    D = DeviceFrame(g, tcw_on_device)
    PO.PoseOptimizationTrack(D.view, g.sig, D.mp, D.rec.data_ptr(), D.outlier.data_ptr(), stage, D.occ.data_ptr(),
                             D.counts.data_ptr())
    PO.synchronize()
    return D.results()


def _unfused(PO, matcher, g, stage):
    from orb_slam2_with_comment_amd._capi import check, lib
    D = DeviceFrame(g)
    PO.PoseOptimization(D.view, g.sig, D.mp, D.rec.data_ptr(), D.outlier.data_ptr())
    PO.synchronize()
    check("orbmi_track_update_matches",
          lib().orbmi_track_update_matches(matcher._h, C.addressof(D.view), stage, D.outlier.data_ptr(), C.addressof(D.mp),
                                           D.occ.data_ptr(), D.counts.data_ptr()))
    return D.results()  # (synchronises the device)


def _same(a, b, what):
    for k in ("rec", "outlier", "occ", "counts", "lf", "mpm"):
        if a[k] is None:
            assert b[k] is None
            continue
        assert a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs"


@pytest.mark.parametrize("stage", [0, 1])
@pytest.mark.parametrize("name", list(S.GATHER))
def test_gather_scene_fused_track_update(oracle, PO, matcher, name, stage):
    g = S.gather_scene(name).gather
    nk = len(g.frame.keys)
    m = nk if g.n_device is None else g.n_device  # the keypoints the device sees
    got = _fused(PO, g, stage)
    fr, ref = _oracle_frame(oracle, g, m)
    flags = got["outlier"][:m]
    _cmp_frame(got["frame"], flags, ref, g.frame.u_right, m, f"{name} stage {stage}", S.count_gather(g, m)["index"])
    # Tracking's pass on the GPU's own flags: exact
    cut = (lambda a: None if a is None else a[:max(m, 1)].copy())
    up_lf, up_mp = cut(g.match_lf), cut(g.match_mp)
    occ, cnt = oracle.track_update_matches(fr, stage, flags if m else np.zeros(1, np.uint8), up_lf, g.lfp, up_mp, g.mps)
    for mine, theirs in ((got["lf"], up_lf), (got["mpm"], up_mp)):
        if theirs is not None:
            np.testing.assert_array_equal(mine[:m], theirs[:m])
    np.testing.assert_array_equal(got["occ"][:m], occ[:m])
    assert got["counts"].tolist() == cnt.tolist()
    # nothing behind the keypoints the device sees is written
    assert (got["outlier"][m:] == SENTINEL).all() and (got["occ"][m:] == SENTINEL).all()
    for mine, orig in ((got["lf"], g.match_lf), (got["mpm"], g.match_mp)):
        if orig is not None:
            np.testing.assert_array_equal(mine[m:nk], orig[m:nk])
            assert (mine[nk:] == -77).all()
    if g.frame.u_right is None and stage == 1:  # monocular: TrackLocalMap keeps the outliers' points
        held = np.array([i for i in range(m) if flags[i]])
        assert len(held) >= 5
        for mine, orig in ((got["lf"], g.match_lf), (got["mpm"], g.match_mp)):
            np.testing.assert_array_equal(mine[held], orig[held])
    _same(got, _unfused(PO, matcher, g, stage), "fused vs PoseOptimization + track update")
    _same(got, _fused(PO, g, stage, tcw_on_device=True), "initial pose on the host vs on the device")


@pytest.mark.parametrize("stage", [0, 1])
def test_gather_overflow_takes_the_keypoint_form(oracle, PO, stage):
    """More than 4096 edges: the record says inliers = -1 at the initial pose, every flag is 0 and
    the tail runs its keypoint form on those flags."""
    g = S.gather_scene("overflow").gather
    nk = len(g.frame.keys)
    got = _fused(PO, g, stage)
    rec = got["frame"]
    assert int(rec["inliers"]) == -1 and int(rec["iterations"]) == 0 and int(rec["n_obs"]) == 5000
    assert rec["tcw"].tobytes() == g.frame.tcw.astype(np.float32).tobytes()
    assert not got["outlier"][:nk].any() and (got["outlier"][nk:] == SENTINEL).all()
    up_lf, up_mp = g.match_lf.copy(), g.match_mp.copy()
    occ, cnt = oracle.track_update_matches(g.frame, stage, np.zeros(nk, np.uint8), up_lf, g.lfp, up_mp, g.mps)
    np.testing.assert_array_equal(got["lf"][:nk], up_lf)
    np.testing.assert_array_equal(got["mpm"][:nk], up_mp)
    np.testing.assert_array_equal(got["occ"][:nk], occ)
    assert got["counts"].tolist() == cnt.tolist()
    assert (got["occ"][nk:] == SENTINEL).all() and (got["lf"][nk:] == -77).all() and (got["mpm"][nk:] == -77).all()
