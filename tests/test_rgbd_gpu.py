"""The RGB-D sensor mode on MI355X: the device stage (csrc/rgbd.hip: UndistortKeyPoints +
ComputeStereoFromRGBD, cvtColor) bit for bit against the numpy restatement
(tests/rgbd_reference.py), the image bounds through the matcher against the oracle, and the native
RGB-D loop (orbmi_slam_track_rgbd) against system.StereoSLAM.TrackRGBD over the oracle backend."""
import ctypes as C
import functools

import numpy as np
import pytest

import rgbd_backends as B
import rgbd_reference as R
from orb_slam2_with_comment_amd import synth, synth_map as SM
from orb_slam2_with_comment_amd.types import KP_DTYPE, Frame

pytestmark = pytest.mark.gpu

_DECISIONS = ("n", "init", "track", "bow_matches", "lf_matches", "nmatches_map", "local_map_points",
              "local_matches", "inliers", "need_kf", "state", "keyframes", "mappoints")


@functools.lru_cache(maxsize=None)
def _frames(n):
    return B.render_rgbd_sequence(n)


@pytest.fixture(scope="module")
def S():
    return B.tum1_settings()


@pytest.fixture(scope="module")
def frame0(S):
    """Frame 0 (640 x 480, TUM1): the image, its gray form, the u16 and float32 depth maps, and the
    GPU extractor holding the extraction of the gray image (raw keypoints on the device)."""
    from orb_slam2_with_comment_amd.orb import ORBextractor
    rgb, depth, _ = _frames(1)[0]
    gray = R.cvt_gray(rgb, True)
    ex = ORBextractor(S.n_features, float(S.scale_factor), S.n_levels, S.ini_th_fast, S.min_th_fast, device=0)
    keys, desc = ex(gray)
    assert len(keys) > 900
    depth_f = depth.astype(np.float32) * np.float32(S.depth_map_factor)
    yield {"rgb": rgb, "gray": gray, "depth": depth, "depth_f": depth_f, "ex": ex, "keys": keys, "desc": desc}
    ex.close()


def _same(got, ref):
    ku, ur, dep = got
    rku, rur, rdep = ref
    assert len(ku) == len(rku)
    assert ku.tobytes() == np.ascontiguousarray(rku, KP_DTYPE).tobytes()   # every field, bit for bit
    np.testing.assert_array_equal(ur.view(np.uint32), rur.view(np.uint32))
    np.testing.assert_array_equal(dep.view(np.uint32), rdep.view(np.uint32))


def _ref(S, keys, depth, factor, dist=None):
    return R.stereo_from_rgbd(keys, depth, factor, S.fx, S.fy, S.cx, S.cy, S.dist_coef if dist is None else dist, S.bf)


def _padded(a, pad):
    buf = np.zeros((a.shape[0], a.shape[1] + pad), a.dtype)
    buf[:, :a.shape[1]] = a
    buf[:, a.shape[1]:] = 7   # the padding holds values a wrong pitch would pick up
    return buf[:, :a.shape[1]]


@pytest.mark.parametrize("case", ["u16", "f32", "u16_pitch", "f32_pitch", "f32_factor"])
def test_stereo_from_rgbd_matches_restatement(S, frame0, case):
    from orb_slam2_with_comment_amd.orb import compute_stereo_from_rgbd
    f = frame0
    depth, factor = {"u16": (f["depth"], S.depth_map_factor), "f32": (f["depth_f"], 1.0),
                     "u16_pitch": (_padded(f["depth"], 13), S.depth_map_factor),
                     "f32_pitch": (_padded(f["depth_f"], 5), 1.0),
                     "f32_factor": (f["depth"].astype(np.float32), S.depth_map_factor)}[case]
    got = compute_stereo_from_rgbd(f["ex"], depth, factor, S, S.dist_coef, float(S.bf), len(f["keys"]))
    ref = _ref(S, f["keys"], depth, factor)
    assert (ref[2] > 0).sum() > 500 and (ref[2] < 0).sum() > 50   # depth and dropouts both present
    assert np.abs(ref[0]["x"] - f["keys"]["x"]).max() > 1            # the undistortion moves keypoints
    _same(got, ref)


def test_stereo_from_rgbd_zero_negative_nan_depth(S, frame0):
    """0, negative, NaN and infinite depth under known keypoints: -1 / -1 for all but +inf (d > 0)."""
    from orb_slam2_with_comment_amd.orb import compute_stereo_from_rgbd
    f = frame0
    depth = f["depth_f"].copy()
    bad = np.array([0.0, -1.5, np.nan, -0.0, np.inf, -np.inf], np.float32)
    k = f["keys"][:120]
    depth[k["y"].astype(np.int64), k["x"].astype(np.int64)] = np.tile(bad, 20)
    got = compute_stereo_from_rgbd(f["ex"], depth, 1.0, S, S.dist_coef, float(S.bf), len(f["keys"]))
    ref = _ref(S, f["keys"], depth, 1.0)
    seeded = ref[2][:120]
    assert (seeded == -1).sum() >= 80 and np.isinf(seeded).sum() >= 1   # (keys of two octaves may share a pixel)
    _same(got, ref)


def test_stereo_from_rgbd_no_keypoints_and_capacity(S, frame0):
    from orb_slam2_with_comment_amd import _capi
    from orb_slam2_with_comment_amd.orb import ORBextractor, camera_view, compute_stereo_from_rgbd
    f = frame0
    ex = ORBextractor(S.n_features, float(S.scale_factor), S.n_levels, S.ini_th_fast, S.min_th_fast, device=0)
    k, d = ex(np.full((480, 640), 97, np.uint8))   # a flat image: no keypoints
    assert len(k) == 0 and d is None
    ku, ur, dep = compute_stereo_from_rgbd(ex, f["depth"], S.depth_map_factor, S, S.dist_coef, float(S.bf), 0)
    assert len(ku) == len(ur) == len(dep) == 0
    ex.close()
    ku, ur, dep = compute_stereo_from_rgbd(None, f["depth"], S.depth_map_factor, S, S.dist_coef, float(S.bf),
                                           keys=np.zeros(0, KP_DTYPE))
    assert len(ku) == len(ur) == len(dep) == 0
    # fewer output slots than keypoints: ORBMI_E_CAP, nothing written
    c = camera_view(S, S.dist_coef)
    n = len(f["keys"]) - 1
    ku, ur, dep = np.zeros(n, KP_DTYPE), np.zeros(n, np.float32), np.zeros(n, np.float32)
    rc = _capi.lib().orbmi_compute_stereo_from_rgbd(f["ex"].handle, 0, f["depth"].ctypes.data, 1, f["depth"].strides[0],
                                                    float(S.depth_map_factor), 480, 640, C.addressof(c), float(S.bf),
                                                    ku.ctypes.data, ur.ctypes.data, dep.ctypes.data, n)
    assert rc == _capi.ORBMI_E_CAP and not ur.any()


def test_stereo_from_rgbd_caller_keys(S, frame0):
    """The caller-keypoints form: keys on the last row and column, and a few outside the image,
    which get -1 / -1 and are copied (nothing is read out of bounds)."""
    from orb_slam2_with_comment_amd.orb import compute_stereo_from_rgbd
    f = frame0
    keys = np.concatenate([f["keys"][:300], np.zeros(12, KP_DTYPE)])
    edge = [(639.0, 10.0), (639.96875, 479.96875), (0.0, 479.0), (12.5, 479.5), (-0.5, -0.5),   # inside after truncation
            (640.0, 10.0), (10.0, 480.0), (-1.0, 5.0), (5.0, -1.0), (1e9, 1e9), (-3e9, 7.0), (700.25, 500.5)]  # outside
    for i, (x, y) in enumerate(edge):
        keys[300 + i] = (x, y, 31.0, 12.5, 40.0, 1, -1)
    depth = f["depth_f"].copy()
    depth[479, :] = 2.0
    depth[:, 639] = 1.5
    depth[0, 0] = 0.75
    for dm, factor in ((depth, 1.0), (_padded(f["depth"], 3), S.depth_map_factor)):
        got = compute_stereo_from_rgbd(None, dm, factor, S, S.dist_coef, float(S.bf), keys=keys)
        ref = _ref(S, keys, dm, factor)
        _same(got, ref)
    ref = _ref(S, keys, depth, 1.0)
    assert np.all(ref[2][300:305] > 0) and np.all(ref[2][305:] == -1) and np.all(ref[1][305:] == -1)
    assert ref[0][305:].tobytes() == keys[305:].tobytes()


def test_stereo_from_rgbd_zero_distortion_copies_keys(S, frame0):
    """k1 = 0 (the reference tests only k1): mvKeysUn = mvKeys bit for bit, whatever k2.. hold."""
    from orb_slam2_with_comment_amd.orb import compute_stereo_from_rgbd
    f = frame0
    for dist in (np.zeros(4, np.float32), np.array([0, -0.9, 0.01, 0.002, 1.1], np.float32)):
        got = compute_stereo_from_rgbd(f["ex"], f["depth"], S.depth_map_factor, S, dist, float(S.bf), len(f["keys"]))
        assert got[0].tobytes() == f["keys"].tobytes()
        _same(got, _ref(S, f["keys"], f["depth"], S.depth_map_factor, dist))


def test_stereo_from_rgbd_device_pointers(S, frame0):
    """Depth map and outputs in HBM (torch tensors), and a mix of host and device outputs."""
    import torch
    from orb_slam2_with_comment_amd import _capi
    from orb_slam2_with_comment_amd.orb import camera_view
    f = frame0
    n = len(f["keys"])
    ref = _ref(S, f["keys"], f["depth"], S.depth_map_factor)
    c = camera_view(S, S.dist_coef)
    d_depth = torch.from_numpy(f["depth"].view(np.int16)).cuda()
    for mixed in (False, True):
        d_ku = torch.zeros(n * KP_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_ur = torch.zeros(n, dtype=torch.float32, device="cuda")
        d_dep = torch.zeros(n, dtype=torch.float32, device="cuda")
        h_ur = np.zeros(n, np.float32)
        rc = _capi.lib().orbmi_compute_stereo_from_rgbd(
            f["ex"].handle, 0, d_depth.data_ptr(), 1, 640 * 2, float(S.depth_map_factor), 480, 640, C.addressof(c),
            float(S.bf), d_ku.data_ptr(), h_ur.ctypes.data if mixed else d_ur.data_ptr(), d_dep.data_ptr(), n)
        assert rc == 0
        torch.cuda.synchronize()
        ku = d_ku.cpu().numpy().view(KP_DTYPE)
        ur = h_ur if mixed else d_ur.cpu().numpy()
        _same((ku, ur, d_dep.cpu().numpy()), ref)


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("rgb", [True, False])
def test_cvt_gray_matches_integer_formula(channels, rgb):
    """37 x 19 with a padded pitch; every channel takes all 256 values."""
    from orb_slam2_with_comment_amd.orb import cvt_gray
    rng = np.random.default_rng(channels * 2 + rgb)
    rows, cols = 19, 37
    buf = rng.integers(0, 256, (rows, cols + 3, channels), dtype=np.uint8)
    for ch in range(channels):
        buf[:, :cols, ch].flat[2:258] = rng.permutation(256)   # (pixels 0 and 1 are set below)
    buf[0, 0, :3], buf[0, 1, :3] = 255, 0
    im = buf[:, :cols]
    assert im.strides[0] == (cols + 3) * channels
    for ch in range(3):
        assert len(np.unique(im[..., ch])) == 256
    got = cvt_gray(im, rgb)
    ref = R.cvt_gray(im, rgb)
    assert ref[0, 0] == 255 and ref[0, 1] == 0
    np.testing.assert_array_equal(got, ref)
    if channels == 3:
        assert not np.array_equal(ref, R.cvt_gray(im, not rgb))   # the channel order matters


def test_cvt_gray_device_image_640x480(frame0):
    import torch
    from orb_slam2_with_comment_amd import _capi
    rgb = frame0["rgb"]
    d_im = torch.from_numpy(rgb).cuda()
    d_g = torch.zeros((480, 640), dtype=torch.uint8, device="cuda")
    assert _capi.lib().orbmi_cvt_gray(0, d_im.data_ptr(), 640 * 3, 3, 1, 480, 640, d_g.data_ptr(), 640) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d_g.cpu().numpy(), frame0["gray"])


@pytest.fixture(scope="module")
def bounded(S, oracle):
    """A TUM1 frame with the distorted camera's bounds, seen from a pose moved sideways so that map
    points project between the bounds and the sensor's edges, and the local map of frames 0..2."""
    frames = _frames(4)
    be = B.OracleRGBDBackend(S)
    sf = be.scale_factors
    rng = np.random.default_rng(3)
    parts = []
    for f in range(3):
        ku, d, ur, dep = be.extract_rgbd(frames[f][0], frames[f][1])
        mp, _ = SM.mappoints_from_frame(ku, d, dep, synth.TUM1, frames[f][2], sf, rng, 0.02, 0.02, 0.02)
        parts.append(mp)
    mps = np.concatenate(parts)
    ku, d, ur, dep = be.extract_rgbd(frames[3][0], frames[3][1])
    T = frames[3][2].copy()
    T[:3, 3] += (0.12, 0.08, -0.1)
    bounds = be.image_bounds(S)
    tcw = SM.tcw_from_twc(T)
    return (Frame(ku, d, ur, tcw, synth.TUM1, scale_factors=sf, bounds=bounds),
            Frame(ku, d, ur, tcw, synth.TUM1, scale_factors=sf), mps)


def test_bounds_through_the_matcher(oracle, bounded):
    """isInFrustum and the local SearchByProjection with TUM1's image bounds agree with the oracle
    given the same bounds; and the bounds matter (points in view of the full sensor area only)."""
    from orb_slam2_with_comment_amd import ORBmatcher
    F, F_full, mps = bounded
    v = F.view()
    assert 0 < v.min_x and v.max_x < 640 and 0 < v.min_y and v.max_y < 480
    t_ref = oracle.is_in_frustum(F, mps, 0.5)
    t_full = oracle.is_in_frustum(F_full, mps, 0.5)
    assert t_ref["in_view"].sum() > 500
    assert t_full["in_view"].sum() > t_ref["in_view"].sum()
    m = ORBmatcher(0.8)
    t = m.IsInFrustum(F, mps, 0.5)
    np.testing.assert_array_equal(t.view(np.uint8), t_ref.view(np.uint8))
    occ = np.zeros(len(F.keys), np.uint8)
    for th in (1.0, 5.0):
        m_ref, n_ref = oracle.search_by_projection_local(F, occ, mps, t_ref, th, 0.8)
        got, n = m.SearchByProjection(F, occ, mps, t_ref, th)
        assert n == n_ref and n > 15   # (the pose is moved off the true one: 21 matches at th 1, 441 at th 5)
        np.testing.assert_array_equal(got, m_ref)
    m.close()


def test_native_rgbd_matches_oracle_30_frames(S):
    """orbmi_slam_track_rgbd (synchronous LocalMapping) over 30 synthetic frames against the Python
    loop over the oracle backend: the comparisons and bars of test_native_matches_oracle_200_frames."""
    from orb_slam2_with_comment_amd import _capi
    from orb_slam2_with_comment_amd.native_slam import NativeStereoSLAM
    from orb_slam2_with_comment_amd.system import OK, StereoSLAM, ate_rmse
    from slam_backends import small_vocabulary
    n = 30
    frames = _frames(n)
    voc = small_vocabulary()
    gpu = NativeStereoSLAM(S, device=0, vocabulary=voc, record=True, sensor="rgbd")
    for f, (rgb, depth, _) in enumerate(frames):
        gpu.TrackRGBD(rgb, depth, f / 30.0)
    ref = StereoSLAM(S, backend=B.OracleRGBDBackend(S, voc), sensor="rgbd")
    for f, (rgb, depth, _) in enumerate(frames):
        ref.TrackRGBD(rgb, depth, f / 30.0)
    a_all, b_all = gpu.stats, ref.stats
    assert len(a_all) == len(b_all) == n
    for a, b in zip(a_all, b_all):
        assert {k: a.get(k) for k in _DECISIONS} == {k: b.get(k) for k in _DECISIONS}, (a, b)
    assert all(st["state"] == OK for st in a_all) and a_all[0]["init"]
    tg, tr = gpu.trajectory_twc(), ref.trajectory_twc()
    np.testing.assert_allclose(tg[:, :3, 3], tr[:, :3, 3], atol=1e-3)
    np.testing.assert_allclose(tg[:, :3, :3], tr[:, :3, :3], atol=1e-4)
    gt = np.array([fr[2] for fr in frames])
    assert abs(ate_rmse(tg, gt) - ate_rmse(tr, gt)) < 1e-3
    assert gpu.counts()["local_ba_calls"] == sum(1 for _ in ref.ba_log)
    assert gpu.counts()["keyframes"] >= 2
    np.testing.assert_array_equal(gpu.keyframe_state_log(), np.array(ref.kf_state, np.int32).reshape(-1, 6))
    # a stereo call on the RGB-D handle, and an RGB-D call on a stereo handle: ORBMI_E_STATE
    g = np.ascontiguousarray(frames[0][0][..., 1])
    tcw, has = np.zeros(16, np.float32), C.c_int()
    L = _capi.lib()
    assert L.orbmi_slam_track_stereo(gpu._h, g.ctypes.data, g.ctypes.data, 480, 640, 640, 1.0, tcw.ctypes.data,
                                     C.byref(has)) == _capi.ORBMI_E_STATE
    assert L.orbmi_slam_track_stereo_ahead(gpu._h, g.ctypes.data, g.ctypes.data, 480, 640, 640, 1.0, None, None,
                                           tcw.ctypes.data, C.byref(has)) == _capi.ORBMI_E_STATE
    assert gpu.counts()["frames"] == n
    gpu.Shutdown()
    stereo = NativeStereoSLAM(S, device=0, vocabulary=None)
    d = frames[0][1]
    assert L.orbmi_slam_track_rgbd(stereo._h, g.ctypes.data, 1, 640, d.ctypes.data, 1, 1280, 480, 640, 0.0,
                                   tcw.ctypes.data, C.byref(has)) == _capi.ORBMI_E_STATE
    stereo.Shutdown()


def test_gpu_backend_tracks_rgbd(S):
    """system.StereoSLAM(sensor="rgbd") over GpuBackend.extract_rgbd (cvt_gray + extraction + the
    RGB-D stage through the operator entries): the oracle-backed loop's first frames, a gray and a
    colour image alike."""
    from orb_slam2_with_comment_amd.system import GpuBackend
    frames = _frames(4)
    gb = GpuBackend(S, 0, None)
    gb.bind_camera(S.camera)
    ob = B.OracleRGBDBackend(S)
    for rgb, depth, _ in frames[:2]:
        for im in (rgb, R.cvt_gray(rgb, True)):
            got, ref = gb.extract_rgbd(im, depth), ob.extract_rgbd(im, depth)
            _same((got[0], got[2], got[3]), (ref[0], ref[2], ref[3]))
            np.testing.assert_array_equal(got[1], ref[1])
    gb.close()
