"""Test infrastructure: a plain numpy restatement of the RGB-D Frame stages, the normative
checker of csrc/undistort.h and csrc/rgbd.hip.

  undistort_points      cv::undistortPoints(pts, pts, K, distCoef, Mat(), K) as
                        Frame::UndistortKeyPoints calls it (src/Frame.cc:456): OpenCV 3.x
                        cvUndistortPoints with R = I, P = K, five fixed iterations, fp64 from the
                        float32 K and mDistCoef, each line evaluated as written
  image_bounds          Frame::ComputeImageBounds (src/Frame.cc:471-499)
  stereo_from_rgbd      Frame::UndistortKeyPoints + Frame::ComputeStereoFromRGBD (:434-469, :678-699)
                        behind Tracking::GrabImageRGBD's convertTo (src/Tracking.cc:226-227)
  cvt_gray              cvtColor's 8-bit fixed-point formula (14 fractional bits)
  distort_points        the forward distortion model (closed form), for the geometric check

numpy evaluates every float64 / float32 operation with one IEEE rounding, as the library does
under -ffp-contract=off.
"""
from __future__ import annotations

import numpy as np


def _coeffs(dist):
    d = np.asarray(dist, np.float32).ravel()
    assert len(d) in (4, 5)
    k1, k2, p1, p2 = (np.float64(v) for v in d[:4])
    k3 = np.float64(d[4]) if len(d) == 5 else np.float64(0.0)
    return k1, k2, p1, p2, k3


def undistort_points(u, v, fx, fy, cx, cy, dist):
    """float32 (u, v) arrays -> float32 (xu, yu); no k1 test here (the callers apply it)."""
    u = np.asarray(u, np.float32).astype(np.float64)
    v = np.asarray(v, np.float32).astype(np.float64)
    fx, fy, cx, cy = (np.float64(np.float32(a)) for a in (fx, fy, cx, cy))
    k1, k2, p1, p2, k3 = _coeffs(dist)
    ifx = 1.0 / fx
    ify = 1.0 / fy
    x0 = (u - cx) * ifx
    y0 = (v - cy) * ify
    x, y = x0, y0
    for _ in range(5):
        r2 = x * x + y * y
        icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x = (x0 - dx) * icdist
        y = (y0 - dy) * icdist
    return (fx * x + cx).astype(np.float32), (fy * y + cy).astype(np.float32)


def distort_points(xu, yu, fx, fy, cx, cy, dist):
    """The forward model in float64: undistorted pixel -> distorted pixel (closed form)."""
    fx, fy, cx, cy = (np.float64(np.float32(a)) for a in (fx, fy, cx, cy))
    k1, k2, p1, p2, k3 = _coeffs(dist)
    x = (np.asarray(xu, np.float64) - cx) / fx
    y = (np.asarray(yu, np.float64) - cy) / fy
    r2 = x * x + y * y
    cdist = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = x * cdist + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * cdist + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return fx * xd + cx, fy * yd + cy


def image_bounds(fx, fy, cx, cy, dist, rows, cols):
    """float32 (mnMinX, mnMaxX, mnMinY, mnMaxY)."""
    d = np.asarray(dist, np.float32).ravel()
    if len(d) == 0 or d[0] == 0.0:
        return np.array([0.0, cols, 0.0, rows], np.float32)
    x, y = undistort_points(np.array([0, cols, 0, cols], np.float32), np.array([0, 0, rows, rows], np.float32),
                            fx, fy, cx, cy, d)
    return np.array([min(x[0], x[2]), max(x[1], x[3]), min(y[0], y[1]), max(y[2], y[3])], np.float32)


def stereo_from_rgbd(keys, depth, factor, fx, fy, cx, cy, dist, bf):
    """keys: structured keypoints (x, y, ...); depth: float32 or uint16 map -> (keys_un, u_right,
    depth) with a key whose truncated position is outside the map copied and given -1 / -1."""
    keys = np.asarray(keys)
    n = len(keys)
    ku = keys.copy()
    ur = np.full(n, -1, np.float32)
    dep = np.full(n, -1, np.float32)
    if n == 0:
        return ku, ur, dep
    depth = np.asarray(depth)
    rows, cols = depth.shape
    factor = np.float32(factor)
    u, v = keys["x"].astype(np.float32), keys["y"].astype(np.float32)
    with np.errstate(invalid="ignore"):
        iu, iv = np.trunc(u).astype(np.int64), np.trunc(v).astype(np.int64)   # C truncation of (int)u
    inside = (iu >= 0) & (iu < cols) & (iv >= 0) & (iv < rows)
    raw = depth[np.where(inside, iv, 0), np.where(inside, iu, 0)]
    if depth.dtype == np.float32 and factor == np.float32(1.0):
        d = raw.astype(np.float32)
    else:
        with np.errstate(invalid="ignore"):
            d = raw.astype(np.float32) * factor   # one float32 multiply
    dist = np.asarray(dist, np.float32).ravel()
    if dist[0] != 0.0:
        xu, yu = undistort_points(u, v, fx, fy, cx, cy, dist)
        ku["x"] = np.where(inside, xu, u)
        ku["y"] = np.where(inside, yu, v)
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = inside & (d > 0)   # false for NaN
        q = np.float32(bf) / d  # float32 division, correctly rounded
        ur = np.where(ok, ku["x"] - q, np.float32(-1)).astype(np.float32)
    dep = np.where(ok, d, np.float32(-1)).astype(np.float32)
    return ku, ur, dep


def cvt_gray(image, rgb):
    """H x W x 3|4 u8 -> H x W u8; rgb: R is channel 0, else B is."""
    im = np.asarray(image).astype(np.int64)
    c0, g, c2 = im[..., 0], im[..., 1], im[..., 2]
    r, b = (c0, c2) if rgb else (c2, c0)
    return ((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8)
