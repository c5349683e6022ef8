"""The RGB-D sensor mode on the CPU: the C ABI exports, the shared undistortion header
(csrc/undistort.h) against the numpy restatement (tests/rgbd_reference.py), the restatement
against the forward distortion model, the synthetic TUM-shaped sequence, and system.StereoSLAM's
TrackRGBD over the oracle backend (tests/rgbd_backends.py)."""
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

import rgbd_backends as B
import rgbd_reference as R

ROOT = pathlib.Path(__file__).resolve().parents[1]
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

_NEW_SYMBOLS = ("orbmi_compute_image_bounds", "orbmi_compute_stereo_from_rgbd", "orbmi_compute_stereo_from_rgbd_keys",
                "orbmi_cvt_gray", "orbmi_slam_create_rgbd", "orbmi_slam_track_rgbd")


def test_rgbd_symbols_exported():
    from orb_slam2_with_comment_amd import _capi
    from orb_slam2_with_comment_amd.build import LIB, build
    build()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(_NEW_SYMBOLS) <= exported, set(_NEW_SYMBOLS) - exported
    assert set(_NEW_SYMBOLS) <= set(_capi.declared_symbols())
    assert set(_NEW_SYMBOLS) <= set(_capi._PROTOS)


@pytest.fixture(scope="module")
def tum1():
    return B.tum1_settings()


@pytest.fixture(scope="module")
def undistort_exe(tmp_path_factory):
    if not pathlib.Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    exe = tmp_path_factory.mktemp("undistort") / "undistort_check"
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-ffp-contract=off", "-I",
                    str(ROOT / "orb_slam2_with_comment_amd" / "csrc"), str(ROOT / "tests" / "cpp" / "undistort_check.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, timeout=600)
    return exe


def _run_header(exe, tmp_path, s, dist, rows, cols, u, v):
    d5 = np.zeros(5, np.float32)
    d5[:len(dist)] = dist
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(np.array([s.fx, s.fy, s.cx, s.cy, *d5], np.float32).tobytes())
        f.write(np.array([rows, cols, len(u)], np.int32).tobytes())
        f.write(np.stack([u, v], -1).astype(np.float32).tobytes())
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    out = np.fromfile(fout, np.float32)
    return out[:-4].reshape(-1, 2), out[-4:]


@pytest.mark.parametrize("case", ["tum1", "four", "zero"])
def test_shared_header_matches_numpy_restatement(undistort_exe, tmp_path, tum1, case):
    """10^4 points and the four corners through csrc/undistort.h on the host: bit-equal to the numpy
    restatement for the TUM1 coefficients, a 4-coefficient set and zero distortion (output = input,
    bounds = 0, cols, 0, rows)."""
    s = tum1
    dist = {"tum1": s.dist_coef, "four": np.array([-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05], np.float32),
            "zero": np.zeros(4, np.float32)}[case]
    assert len(s.dist_coef) == 5
    rng = np.random.default_rng(11)
    u = rng.uniform(-20, 660, 10000).astype(np.float32)
    v = rng.uniform(-20, 500, 10000).astype(np.float32)
    u[:4], v[:4] = [0, 640, 0, 640], [0, 0, 480, 480]
    got, bounds = _run_header(undistort_exe, tmp_path, s, dist, 480, 640, u, v)
    ref_b = R.image_bounds(s.fx, s.fy, s.cx, s.cy, dist, 480, 640)
    if case == "zero":
        np.testing.assert_array_equal(got.view(np.uint32), np.stack([u, v], -1).view(np.uint32))
        np.testing.assert_array_equal(bounds, np.array([0, 640, 0, 480], np.float32))
        np.testing.assert_array_equal(ref_b, bounds)
        return
    xu, yu = R.undistort_points(u, v, s.fx, s.fy, s.cx, s.cy, dist)
    np.testing.assert_array_equal(got.view(np.uint32), np.stack([xu, yu], -1).view(np.uint32))
    np.testing.assert_array_equal(bounds.view(np.uint32), ref_b.view(np.uint32))
    if case == "tum1":  # the undistorted image is smaller than the sensor on every side
        assert 0 < bounds[0] < 40 and 600 < bounds[1] < 640 and 0 < bounds[2] < 40 and 440 < bounds[3] < 480


def test_host_bounds_entry_matches_restatement(tum1):
    """orbmi_compute_image_bounds (host only, no GPU) = the restatement, and 0, cols, 0, rows for k1 = 0."""
    from orb_slam2_with_comment_amd.orb import compute_image_bounds
    s = tum1
    got = compute_image_bounds(s, s.dist_coef, 480, 640)
    np.testing.assert_array_equal(got.view(np.uint32),
                                  R.image_bounds(s.fx, s.fy, s.cx, s.cy, s.dist_coef, 480, 640).view(np.uint32))
    np.testing.assert_array_equal(compute_image_bounds(s, np.array([0, 0.1, 0.01, 0.01], np.float32), 480, 640),
                                  np.array([0, 640, 0, 480], np.float32))


def test_undistortion_inverts_the_forward_model(tum1):
    """Independent of the restatement's iteration: the undistorted points, re-distorted with the
    closed-form forward model in float64, return to the input.  Measured for TUM1 over every
    integer pixel position 0..640 x 0..480: maximum 0.1103 px (at the corner (640, 0), where five
    iterations have not converged; the median is 8e-6 px); asserted at twice that."""
    s = tum1
    uu, vv = np.meshgrid(np.arange(0, 641, dtype=np.float32), np.arange(0, 481, dtype=np.float32))
    u, v = uu.ravel(), vv.ravel()
    xu, yu = R.undistort_points(u, v, s.fx, s.fy, s.cx, s.cy, s.dist_coef)
    ud, vd = R.distort_points(xu, yu, s.fx, s.fy, s.cx, s.cy, s.dist_coef)
    err = np.maximum(np.abs(ud - u), np.abs(vd - v))
    print(f"round trip: max {err.max():.6f} px, median {np.median(err):.2e} px")
    assert err.max() < 2 * 0.1103
    # and the undistortion is not the identity: the corners move by several pixels
    assert np.abs(xu - u).max() > 5


@pytest.fixture(scope="module")
def rgbd_frames():
    return B.render_rgbd_sequence(12)


def test_synthetic_frame_meets_stereo_initialization(tum1, rgbd_frames, oracle):
    """Frame 0 of the synthetic TUM-shaped sequence: more than 500 keypoints with depth
    (StereoInitialization, src/Tracking.cc:586), some closer than mThDepth, and dropouts (depth 0)."""
    s = tum1
    rgb, depth, _ = rgbd_frames[0]
    assert rgb.shape == (480, 640, 3) and rgb.dtype == np.uint8 and depth.shape == (480, 640) and depth.dtype == np.uint16
    assert (depth == 0).any() and (depth > 0).mean() > 0.5
    be = B.OracleRGBDBackend(s)
    ku, _, ur, dep = be.extract_rgbd(rgb, depth)
    valid = dep > 0
    assert valid.sum() > 500
    assert ((dep < s.th_depth) & valid).sum() > 50
    assert (~valid).sum() > 0 and np.all(ur[~valid] == -1)
    # u_right = x_un - bf / d, to the left of the keypoint
    assert np.all(ur[valid] < ku["x"][valid])


def test_existing_synthetic_output_unchanged():
    """render / stereo_pair / mono are untouched by the RGB-D additions (digests of frame 0,
    recorded from the parent revision)."""
    import hashlib
    from orb_slam2_with_comment_amd import synth
    L, Rr, _ = synth.stereo_pair(synth.KITTI, 0)
    m = synth.mono(synth.EUROC, 0)
    assert hashlib.sha256(L.tobytes()).hexdigest() == _DIGESTS["L"]
    assert hashlib.sha256(Rr.tobytes()).hexdigest() == _DIGESTS["R"]
    assert hashlib.sha256(m.tobytes()).hexdigest() == _DIGESTS["mono"]


_DIGESTS = {"L": "d721d3f2588452cffe4b4e25ef2bbc80060538a495e3af5d66527eae6524674e",
            "R": "cf6bbbb447a36a7375a526d9c7a0fd9c961b171ccff222ad526fc0416d40b45d",
            "mono": "cf5ff93be99396f328c75e8a277380182e5c1e7dcefeff40a88e84ca5afb72ca"}


def test_python_loop_tracks_rgbd_on_the_oracle(tum1, rgbd_frames):
    """system.StereoSLAM(sensor="rgbd").TrackRGBD over the oracle backend on 12 synthetic frames:
    initialisation on frame 0, every later state OK, at least 2 keyframes, no extract_stereo call.
    ATE against ground truth measured here: 0.00447 m; asserted at twice that (a gross-error guard,
    e.g. against a sign error in u_right)."""
    from orb_slam2_with_comment_amd.system import OK, StereoSLAM, ate_rmse
    from slam_backends import small_vocabulary
    s = tum1
    slam = StereoSLAM(s, backend=B.OracleRGBDBackend(s, small_vocabulary()), sensor="rgbd")
    poses = [slam.TrackRGBD(rgb, depth, f / 30.0) for f, (rgb, depth, _) in enumerate(rgbd_frames)]
    assert slam.stats[0]["init"] is True and slam.stats[0]["state"] == OK
    assert all(st["state"] == OK for st in slam.stats[1:]) and all(p is not None for p in poses)
    assert len(slam.keyframes) >= 2
    assert "extract_stereo" not in slam.backend.calls and slam.backend.calls["extract_rgbd"] == 12
    gt = np.array([fr[2] for fr in rgbd_frames])
    ate = ate_rmse(slam.trajectory_twc(), gt)
    print(f"ATE {ate:.6f} m")
    assert ate < 2 * 0.00447
    with pytest.raises(RuntimeError):
        slam.TrackStereo(rgbd_frames[0][0][..., 0], rgbd_frames[0][0][..., 0], 1.0)


def test_frame_bounds_default_and_given():
    """types.Frame.view(): today's values by default, the given bounds and their grid otherwise."""
    from orb_slam2_with_comment_amd import synth
    from orb_slam2_with_comment_amd.types import KP_DTYPE, Frame
    k, d = np.zeros(1, KP_DTYPE), np.zeros((1, 32), np.uint8)
    v = Frame(k, d, cam=synth.KITTI).view()
    assert (v.min_x, v.max_x, v.min_y, v.max_y) == (0.0, 1241.0, 0.0, 376.0)
    assert v.grid_w_inv == np.float32(np.float32(64) / np.float32(1241))
    b = (np.float32(10.5), np.float32(626.25), np.float32(14.5), np.float32(473.0))
    v = Frame(k, d, cam=synth.TUM1, bounds=b).view()
    assert (v.min_x, v.max_x, v.min_y, v.max_y) == tuple(float(x) for x in b)
    assert v.grid_w_inv == np.float32(np.float32(64) / np.float32(b[1] - b[0]))
    assert v.grid_h_inv == np.float32(np.float32(48) / np.float32(b[3] - b[2]))
