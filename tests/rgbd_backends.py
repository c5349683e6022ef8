"""Test infrastructure: slam_backends.OracleBackend with the RGB-D Frame constructor -- the oracle's
extraction followed by the numpy restatement (tests/rgbd_reference.py) -- so system.StereoSLAM's
TrackRGBD runs on the CPU and the native RGB-D loop can be compared with it."""
from __future__ import annotations

import os

import numpy as np

import rgbd_reference as R
from slam_backends import OracleBackend

TUM1_YAML = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "settings", "TUM1.yaml")


class OracleRGBDBackend(OracleBackend):
    def __init__(self, settings, vocabulary=None):
        super().__init__(settings, vocabulary)
        self.settings = settings

    def image_bounds(self, s):
        return R.image_bounds(s.fx, s.fy, s.cx, s.cy, s.dist_coef, s.height, s.width)

    def extract_rgbd(self, im, depth):
        self._count("extract_rgbd")
        s = self.settings
        im = np.asarray(im)
        gray = R.cvt_gray(im, s.rgb) if im.ndim == 3 else im
        k, d = self.O.extract(self.p, np.ascontiguousarray(gray))
        ku, ur, dep = R.stereo_from_rgbd(k, depth, s.depth_map_factor, s.fx, s.fy, s.cx, s.cy, s.dist_coef, s.bf)
        return ku, np.asarray(d, np.uint8).reshape(-1, 32), ur, dep


def tum1_settings():
    from orb_slam2_with_comment_amd.settings import load_settings
    return load_settings(TUM1_YAML)


def _render(f):
    from orb_slam2_with_comment_amd import synth
    return synth.rgbd_frame(synth.TUM1, f)


def render_rgbd_sequence(n, workers=None):
    """Frames 0..n-1 of the synthetic TUM-shaped sequence (synth.rgbd_frame), by a process pool."""
    import multiprocessing as mp
    workers = workers or max(1, min(16, (os.cpu_count() or 1), n))
    if workers == 1:
        return [_render(f) for f in range(n)]
    with mp.get_context("fork").Pool(workers) as pool:
        return pool.map(_render, range(n))
