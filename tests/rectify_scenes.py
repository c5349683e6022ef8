"""Test infrastructure shared by tests/test_rectify_cpu.py and tests/test_rectify_gpu.py: the
EuRoC rig of tests/golden/settings/EuRoC.yaml, small cameras for the map builder, the raw
EuRoC-shaped sequence (synth.raw_stereo_pair) and its rectification by the numpy restatement."""
from __future__ import annotations

import functools
import os

import numpy as np

import rectify_reference as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EUROC_YAML = os.path.join(ROOT, "tests", "golden", "settings", "EuRoC.yaml")
N_FRAMES = 12


@functools.lru_cache(maxsize=None)
def euroc_settings():
    from orb_slam2_with_comment_amd.settings import load_settings
    return load_settings(EUROC_YAML)


def small_camera(nd, rows, cols, seed=0):
    """A camera of rows x cols with nd distortion coefficients, a small rotation and a new
    projection: intrinsics scaled to the size so that the maps cross the image border."""
    from orb_slam2_with_comment_amd.settings import RectifyCamera
    rng = np.random.default_rng(1000 * nd + 31 * rows + cols + seed)
    f = 0.9 * max(cols, rows, 4)
    K = np.array([[f, 0, 0.5 * cols + 0.3], [0, 0.97 * f, 0.5 * rows - 0.2], [0, 0, 1]], np.float64)
    D = np.array([-0.283, 0.074, 1.9e-4, 1.8e-5, 0.013, 0.021, -0.008, 0.004], np.float64)[:nd]
    w = rng.uniform(-0.02, 0.02, 3)  # Rodrigues, first order re-orthonormalised by QR
    A = np.array([[1, -w[2], w[1]], [w[2], 1, -w[0]], [-w[1], w[0], 1]])
    Q, Rr = np.linalg.qr(A)
    R = Q * np.sign(np.diag(Rr))
    P = np.array([[0.93 * f, 0, 0.5 * cols, -3.1], [0, 0.93 * f, 0.5 * rows, 0], [0, 0, 1, 0]], np.float64)
    return RectifyCamera(K, D, R, P, rows, cols)


def _raw(f):
    from orb_slam2_with_comment_amd import synth
    return synth.raw_stereo_pair(euroc_settings().rectification, f)


@functools.lru_cache(maxsize=None)
def raw_frames():
    """[(left, right, Twc)] of frames 0..11 of the raw EuRoC-shaped sequence, rendered once per
    process and in this process (~0.3 s per pair: a pool would fork after the GPU tests have
    initialised the device)."""
    return [_raw(f) for f in range(N_FRAMES)]


@functools.lru_cache(maxsize=None)
def euroc_maps():
    """((map1, map2) left, (map1, map2) right) of the EuRoC rig by the numpy restatement."""
    return tuple(RR.init_undistort_rectify_map(c.K, c.D, c.R, c.P, c.rows, c.cols)
                 for c in euroc_settings().rectification)


@functools.lru_cache(maxsize=None)
def rectified_frames():
    """[(left, right)] of raw_frames() rectified by the numpy restatement."""
    (l1, l2), (r1, r2) = euroc_maps()
    return [(RR.remap(L, l1, l2), RR.remap(R, r1, r2)) for L, R, _ in raw_frames()]
