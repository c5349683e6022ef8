"""Synthetic KITTI- / EuRoC-shaped input.

KITTI-00 and EuRoC are not available offline, so every benchmark and parity test runs on
ray-cast textured planes with exact ground truth: a ground plane at y=+1.65 m, side walls at
x=+-8 m, a canopy at y=-4 m and a far wall, camera moving forward 1 m/frame with 0.2 deg/frame
yaw.  Intrinsics come from the reference's own settings files
(Examples/Stereo/KITTI00-02.yaml, Examples/Monocular/EuRoC.yaml).  The texture is a blocky
multi-scale hash pattern on a smooth gradient plus +-4 uniform noise, seeded per frame, which
gives FAST corners at every pyramid level.  `rgbd_frame` renders the same scene at indoor size
through the distortion model of Examples/RGB-D/TUM1.yaml, with a uint16 depth map.
"""
from __future__ import annotations

import dataclasses

import numpy as np


@dataclasses.dataclass(frozen=True)
class Camera:
    width: int
    height: int
    fx: float
    fy: float
    cx: float
    cy: float
    bf: float  # stereo baseline x fx

    @property
    def baseline(self) -> float:
        return self.bf / self.fx


# Examples/Stereo/KITTI00-02.yaml
KITTI = Camera(1241, 376, 718.856, 718.856, 607.1928, 185.2157, 386.1448)
# Examples/Monocular/EuRoC.yaml (bf from Examples/Stereo/EuRoC.yaml)
EUROC = Camera(752, 480, 458.654, 457.296, 367.215, 248.375, 47.90639384423901)



@dataclasses.dataclass(frozen=True)
class RGBDCamera(Camera):
    """A distorted RGB-D camera: mDistCoef (k1 k2 p1 p2 k3), ThDepth and DepthMapFactor as the
    settings file gives them."""
    dist_coef: tuple = (0.0, 0.0, 0.0, 0.0)
    th_depth: float = 40.0
    depth_map_factor: float = 5000.0
    n_features: int = 1000


# Examples/RGB-D/TUM1.yaml (bf 40, ThDepth 40, DepthMapFactor 5000, 1000 features)
TUM1 = RGBDCamera(640, 480, 517.306408, 516.469215, 318.643040, 255.313989, 40.0,
                  (0.262383, -0.953104, -0.005358, 0.002628, 1.163314), 40.0, 5000.0, 1000)

_PLANES = (  # (axis, offset): plane axis == offset in world coordinates
    (1, 1.65),    # ground
    (1, -4.0),    # canopy
    (0, -8.0),    # left wall
    (0, 8.0),     # right wall
    (2, 400.0),   # far wall
)


def _hash01(i: np.ndarray, j: np.ndarray, salt: int) -> np.ndarray:
    h = (i.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ \
        (j.astype(np.uint64) * np.uint64(0xC2B2AE3D27D4EB4F)) ^ np.uint64(salt * 0x165667B19E3779F9 & (2**64 - 1))
    h ^= h >> np.uint64(29)
    h *= np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(32)
    return (h >> np.uint64(40)).astype(np.float64) / float(1 << 24)


def pose(frame: int, step: float = 1.0, yaw_deg: float = 0.2) -> np.ndarray:
    """Twc (4x4 float64) of the left camera at `frame`."""
    a = np.deg2rad(yaw_deg * frame)
    T = np.eye(4)
    T[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    T[2, 3] = step * frame
    return T


def render(cam: Camera, Twc: np.ndarray, seed: int, noise: float = 4.0,
           return_depth: bool = False):
    """Ray-cast one u8 image (H x W) from camera pose Twc."""
    u = np.arange(cam.width, dtype=np.float64)
    v = np.arange(cam.height, dtype=np.float64)
    uu, vv = np.meshgrid(u, v)
    dc = np.stack([(uu - cam.cx) / cam.fx, (vv - cam.cy) / cam.fy, np.ones_like(uu)], -1)
    dw = dc @ Twc[:3, :3].T
    o = Twc[:3, 3]
    best_t = np.full(uu.shape, np.inf)
    img = np.zeros(uu.shape)
    for pid, (axis, off) in enumerate(_PLANES):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (off - o[axis]) / dw[..., axis]
        hit = (t > 0) & (t < best_t)
        if not hit.any():
            continue
        p = o + dw[hit] * t[hit][:, None]
        ax = [k for k in range(3) if k != axis]
        a, b = p[:, ax[0]], p[:, ax[1]]
        val = 128.0 + 50.0 * np.sin(0.11 * a + pid) * np.cos(0.07 * b)
        val += 80.0 * (_hash01(np.floor(a / 0.6), np.floor(b / 0.6), 11 + pid) - 0.5)
        val += 50.0 * (_hash01(np.floor(a / 0.17), np.floor(b / 0.17), 23 + pid) - 0.5)
        img[hit] = val
        best_t[hit] = t[hit]
    rng = np.random.default_rng(seed)
    img += rng.uniform(-noise, noise, img.shape)
    out = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    if return_depth:
        return out, best_t  # t along dc (z=1) is the depth
    return out


def stereo_pair(cam: Camera, frame: int, seed_base: int = 1000):
    """(left, right, Twc_left) for frame `frame` of the KITTI-shaped sequence."""
    T = pose(frame)
    TR = T.copy()
    TR[:3, 3] = T[:3, 3] + T[:3, :3] @ np.array([cam.baseline, 0.0, 0.0])
    seed = seed_base + frame
    return render(cam, T, seed), render(cam, TR, seed + 7919), T


def mono(cam: Camera, frame: int, seed_base: int = 5000):
    return render(cam, pose(frame, step=0.05, yaw_deg=0.5), seed_base + frame)


# ---- RGB-D (TUM-shaped) ---------------------------------------------------------------------
_ROOM = (  # (axis, offset) in metres: an indoor corridor around a camera 1 m above the floor
    (1, 1.0),     # floor
    (1, -1.2),    # ceiling
    (0, -1.5),    # left wall
    (0, 1.5),     # right wall
    (2, 10.0),    # end wall (beyond the sensor range until the camera gets close)
)
_ROOM_TEXTURE_SCALE = 0.25   # the KITTI-shaped texture shrunk 4x: 15 cm and 4 cm blocks
_RGBD_STEP = 0.05            # metres per frame
_RGBD_RANGE = 6.0            # metres; farther surfaces read 0 (a dropout)


def _undistorted_rays(cam) -> np.ndarray:
    """Per pixel of the distorted image, the undistorted normalised point (x, y, 1): the
    distortion model inverted by the five fixed-point iterations cv::undistortPoints runs."""
    k1, k2, p1, p2 = cam.dist_coef[:4]
    k3 = cam.dist_coef[4] if len(cam.dist_coef) > 4 else 0.0
    u = np.arange(cam.width, dtype=np.float64)
    v = np.arange(cam.height, dtype=np.float64)
    uu, vv = np.meshgrid(u, v)
    x0, y0 = (uu - cam.cx) / cam.fx, (vv - cam.cy) / cam.fy
    x, y = x0, y0
    for _ in range(5):
        r2 = x * x + y * y
        icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (x0 - dx) * icdist, (y0 - dy) * icdist
    return np.stack([x, y, np.ones_like(x)], -1)


def _cast_room(dw: np.ndarray, o: np.ndarray):
    """(image before noise, ray parameter t of the nearest hit) of rays o + t dw in _ROOM."""
    best_t = np.full(dw.shape[:2], np.inf)
    img = np.zeros(dw.shape[:2])
    for pid, (axis, off) in enumerate(_ROOM):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (off - o[axis]) / dw[..., axis]
        hit = (t > 0) & (t < best_t)
        if not hit.any():
            continue
        p = (o + dw[hit] * t[hit][:, None]) / _ROOM_TEXTURE_SCALE
        ax = [k for k in range(3) if k != axis]
        a, b = p[:, ax[0]], p[:, ax[1]]
        val = 128.0 + 50.0 * np.sin(0.11 * a + pid) * np.cos(0.07 * b)
        val += 80.0 * (_hash01(np.floor(a / 0.6), np.floor(b / 0.6), 11 + pid) - 0.5)
        val += 50.0 * (_hash01(np.floor(a / 0.17), np.floor(b / 0.17), 23 + pid) - 0.5)
        img[hit] = val
        best_t[hit] = t[hit]
    return img, best_t


def rgbd_frame(cam: RGBDCamera, frame: int, seed_base: int = 9000, noise: float = 4.0):
    """(rgb u8 H x W x 3, depth u16 H x W, Twc) of frame `frame` of the TUM-shaped sequence.

    The scene is the KITTI-shaped one at indoor size: a corridor 3 m wide and 2.2 m high (_ROOM)
    with the texture at scale 0.25, the camera moving 0.05 m/frame forward with 0.2 deg/frame yaw.
    Rendering goes through the distortion model: the ray of a pixel is its undistorted normalised
    point, so undistorted keypoints obey the pinhole model of K.  depth = z * DepthMapFactor as
    uint16, 0 beyond 6 m (sensor dropouts: the end wall at the start).  The chosen scale: walls
    1.5 m to either side, floor 1.0 m below, ceiling 1.2 m above, end wall 10 m ahead, texture
    blocks of 15 cm and 4 cm.  With TUM1 frame 0 gives 1,004 keypoints, 711 of them with depth
    (more than the 500 StereoInitialization asks for, src/Tracking.cc:586) and 104 closer than
    mThDepth = bf ThDepth / fx = 3.09 m (tests/test_rgbd_cpu.py checks both conditions)."""
    Twc = pose(frame, step=_RGBD_STEP)
    dc = _undistorted_rays(cam)
    dw = dc @ Twc[:3, :3].T
    o = Twc[:3, 3]
    img, best_t = _cast_room(dw, o)
    rng = np.random.default_rng(seed_base + frame)
    img += rng.uniform(-noise, noise, img.shape)
    g = np.rint(img)
    rgb = np.clip(np.stack([g + 6, g, g - 9], -1), 0, 255).astype(np.uint8)  # a slight tint: R, G, B differ
    z = np.where(np.isfinite(best_t) & (best_t <= _RGBD_RANGE), best_t, 0.0)  # t along (x, y, 1) is the depth
    depth = np.clip(np.rint(z * cam.depth_map_factor), 0, 65535).astype(np.uint16)
    return rgb, depth, Twc


# ---- raw stereo (EuRoC-shaped: not rectified) -----------------------------------------------
def raw_stereo_pair(rig, frame: int, seed_base: int = 12000, noise: float = 4.0):
    """(left, right, Twc) raw u8 images of frame `frame` as a rig that is not factory-rectified
    sees the RGB-D corridor (_ROOM, texture scale 0.25, 0.05 m/frame): rig = (left, right)
    settings.RectifyCamera, Twc the pose of the rectified left camera.  The ray of a raw pixel is
    R_c (its undistorted normalised point, the five iterations of _undistorted_rays with that
    camera's K and D) in the rectified frame -- R_c takes raw camera coordinates to rectified ones,
    so rectifying the pair (cv::initUndistortRectifyMap with R_c, P_c + cv::remap) gives the
    pinhole views of LEFT.P / RIGHT.P.  The right camera sits bf / fx = -RIGHT.P[0,3] / RIGHT.P[0,0]
    along the rectified x axis.  D has 4 or 5 coefficients (more raise: the inverse model here has
    no k4..k6)."""
    Twc = pose(frame, step=_RGBD_STEP)
    baseline = -float(rig[1].P[0, 3]) / float(rig[1].P[0, 0])
    out = []
    for side, cam in enumerate(rig):
        if len(np.asarray(cam.D).ravel()) > 5:  # _undistorted_rays inverts k1 k2 p1 p2 k3 only
            raise ValueError("raw_stereo_pair renders cameras with at most 5 distortion coefficients")
        K, D = np.asarray(cam.K, np.float64), tuple(float(v) for v in np.asarray(cam.D).ravel())
        c = RGBDCamera(int(cam.cols), int(cam.rows), K[0, 0], K[1, 1], K[0, 2], K[1, 2], 0.0, D)
        dw = (_undistorted_rays(c) @ np.asarray(cam.R, np.float64).T) @ Twc[:3, :3].T  # rows: d_rect = R d_raw
        o = Twc[:3, 3] + Twc[:3, :3] @ np.array([baseline * side, 0.0, 0.0])
        img, _ = _cast_room(dw, o)
        rng = np.random.default_rng(seed_base + frame + 7919 * side)
        img += rng.uniform(-noise, noise, img.shape)
        out.append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
    return out[0], out[1], Twc
