"""orb_slam2_with_comment_amd — MI355X-native ORB front-end and local BA for ORB-SLAM2.

The hot path of AHzZ123/orb_slam2_with_comment as hand-written HIP kernels
for gfx950 behind a C ABI (include/orbmi.h, liborbmi.so).  This package holds the kernels
(csrc/), their build (build.py), the ctypes binding (_capi.py) and a Python mirror of the
reference interface (orb.py) used by tests and bench.py.
"""
from .loop import KeyFrameDatabase, LoopBackend, LoopDetector, detect_and_compute_sim3  # noqa: F401
from .matcher import ORBmatcher  # noqa: F401
from .orb import ORBextractor, compute_stereo_matches  # noqa: F401
from .sim3 import Sim3Ransac, Sim3Solver, compute_sim3, solve_batch  # noqa: F401

__all__ = ["KeyFrameDatabase", "LoopBackend", "LoopDetector", "ORBextractor", "ORBmatcher", "Sim3Ransac",
           "Sim3Solver", "compute_sim3", "compute_stereo_matches", "detect_and_compute_sim3", "solve_batch"]
