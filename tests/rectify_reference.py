"""numpy restatement of stereo rectification: cv::initUndistortRectifyMap as OpenCV
3.x documents it, cv::remap's fixed-point conversion of float maps, and the bilinear remap of
8-bit images with BORDER_CONSTANT 0.  Written from the documented algorithm, in fp64 with one
IEEE operation per step (numpy's elementwise operations are single operations; the column sums
use np.add.accumulate, which adds sequentially).  Test infrastructure only."""
from __future__ import annotations

import numpy as np

INTER_BITS = 5
INTER_TAB = 1 << INTER_BITS


def inverse_projection(P, R):
    """inverse(P[0:3, 0:3] R): dot products summed in index order, cofactors times 1 / det."""
    P = np.asarray(P, np.float64).reshape(3, -1)
    R = np.asarray(R, np.float64).reshape(3, 3)
    S = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            s = float(P[i, 0]) * float(R[0, j])
            s = s + float(P[i, 1]) * float(R[1, j])
            s = s + float(P[i, 2]) * float(R[2, j])
            S[i][j] = s
    (a, b, c), (d, e, f), (g, h, k) = S
    det = a * (e * k - f * h) - b * (d * k - f * g) + c * (d * h - e * g)
    det = 1.0 / det
    return np.array([(e * k - f * h) * det, (c * h - b * k) * det, (b * f - c * e) * det,
                     (f * g - d * k) * det, (a * k - c * g) * det, (c * d - a * f) * det,
                     (d * h - e * g) * det, (b * g - a * h) * det, (a * e - b * d) * det], np.float64)


def normalised(K, D, R, P, rows, cols):
    """(x, y) of every rectified pixel in the raw camera's normalised plane, before distortion."""
    iR = inverse_projection(P, R)
    i = np.arange(rows, dtype=np.float64)[:, None]

    def run(c0, c1, c2):  # row start i * c1 + c2, then one addition of c0 per column
        inc = np.full((rows, cols), c0, np.float64)
        inc[:, 0:1] = i * c1 + c2
        return np.add.accumulate(inc, axis=1)

    _x, _y, _w = run(iR[0], iR[1], iR[2]), run(iR[3], iR[4], iR[5]), run(iR[6], iR[7], iR[8])
    w = 1.0 / _w
    return _x * w, _y * w


def init_undistort_rectify_map(K, D, R, P, rows, cols):
    """(map1, map2) float32 rows x cols.  D: 4, 5 or 8 coefficients k1 k2 p1 p2 [k3 [k4 k5 k6]]."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    D = np.asarray(D, np.float64).ravel()
    if len(D) not in (4, 5, 8):
        raise ValueError("D has 4, 5 or 8 coefficients")
    k1, k2, p1, p2, k3, k4, k5, k6 = list(D) + [0.0] * (8 - len(D))
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    x, y = normalised(K, D, R, P, rows, cols)
    x2, y2 = x * x, y * y
    r2 = x2 + y2
    _2xy = 2 * x * y
    kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
    xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)
    yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy
    return (fx * xd + cx).astype(np.float32), (fy * yd + cy).astype(np.float32)


def fixed_point(m):
    """round-half-even(m * 32) as int64 and the mask of NaNs and values beyond int32."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.asarray(m, np.float32).astype(np.float64) * INTER_TAB
        bad = ~(np.abs(s) < 2147483648.0)
        return np.rint(np.where(bad, 0.0, s)).astype(np.int64), bad


def records(map1, map2):
    """x0, y0, a, b (int64) and the outside mask of every destination pixel."""
    sx, bx = fixed_point(map1)
    sy, by = fixed_point(map2)
    return sx >> INTER_BITS, sy >> INTER_BITS, sx & (INTER_TAB - 1), sy & (INTER_TAB - 1), bx | by


def remap(src, map1, map2):
    """cv::remap(src, dst, map1, map2, INTER_LINEAR, BORDER_CONSTANT, 0) for a u8 image."""
    src = np.asarray(src, np.uint8)
    rows, cols = src.shape
    x0, y0, a, b, out = records(map1, map2)

    def tap(y, x):
        ok = ~out & (x >= 0) & (x < cols) & (y >= 0) & (y < rows)
        return np.where(ok, src[np.clip(y, 0, rows - 1), np.clip(x, 0, cols - 1)].astype(np.int64), 0)

    v = ((INTER_TAB - a) * (INTER_TAB - b) * tap(y0, x0) + a * (INTER_TAB - b) * tap(y0, x0 + 1)
         + (INTER_TAB - a) * b * tap(y0 + 1, x0) + a * b * tap(y0 + 1, x0 + 1))
    return ((v + 512) >> 10).astype(np.uint8)


def rectify_pair(rect, left, right):
    """Both images of a raw pair through the maps of settings.Settings.rectification."""
    out = []
    for cam, im in zip(rect, (left, right)):
        m1, m2 = init_undistort_rectify_map(cam.K, cam.D, cam.R, cam.P, cam.rows, cam.cols)
        out.append(remap(im, m1, m2))
    return out
