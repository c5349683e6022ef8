"""Python mirror of the reference's ORB front-end interface, over the C ABI (liborbmi.so).

`ORBextractor` mirrors include/ORBextractor.h:45-111 (constructor arguments, operator(),
getters, mvImagePyramid); `compute_stereo_matches` mirrors Frame::ComputeStereoMatches
(src/Frame.cc:501-675); `compute_stereo_from_rgbd`, `compute_image_bounds` and `cvt_gray` mirror the
RGB-D Frame constructor's stages (src/Frame.cc:434-499, 678-699).  Every call runs the hand-written HIP kernels; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import KP_DTYPE, check, lib, ptr


class ORBextractor:
    """ORB_SLAM2::ORBextractor on one MI355X (include/ORBextractor.h:58-59)."""

    def __init__(self, nfeatures: int, scaleFactor: float, nlevels: int, iniThFAST: int,
                 minThFAST: int, device: int = 0):
        h = C.c_void_p()
        check("orbmi_extractor_create",
              lib().orbmi_extractor_create(device, nfeatures, scaleFactor, nlevels, iniThFAST,
                                           minThFAST, C.byref(h)))
        self._h = h
        self.nfeatures = nfeatures
        self.nlevels = nlevels
        self.device = device
        self._shape = None

    def close(self):
        if getattr(self, "_h", None):
            lib().orbmi_extractor_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    # ORBextractor::operator()(image, mask, keypoints, descriptors)  src/ORBextractor.cc:1043
    def __call__(self, image: np.ndarray, mask=None):
        """Returns (keypoints [structured KP_DTYPE], descriptors [n x 32 u8] or None).

        The mask is ignored, as in the reference (include/ORBextractor.h:62-63)."""
        image = np.asarray(image)
        if image.size == 0:
            return np.zeros(0, KP_DTYPE), None
        if image.dtype != np.uint8 or image.ndim != 2:
            raise TypeError("ORBextractor expects a CV_8UC1 image (src/ORBextractor.cc:1050)")
        image = np.ascontiguousarray(image)
        cap = self.nfeatures + 16 * self.nlevels + 64
        while True:
            kps = np.zeros(cap, KP_DTYPE)
            desc = np.zeros((cap, 32), np.uint8)
            n = C.c_int()
            rc = lib().orbmi_extract(self._h, ptr(image), image.shape[0], image.shape[1],
                                     image.strides[0], ptr(kps), ptr(desc), cap, C.byref(n))
            if rc == _capi.ORBMI_E_CAP:
                cap = n.value
                continue
            check("orbmi_extract", rc)
            break
        self._shape = image.shape
        n = n.value
        if n == 0:
            return kps[:0].copy(), None  # descriptors.release() (src/ORBextractor.cc:1063-1064)
        return kps[:n].copy(), desc[:n].copy()

    def _levels_f(self, fn):
        out = np.zeros(self.nlevels, np.float32)
        check(fn, getattr(lib(), fn)(self._h, ptr(out)))
        return out

    def GetLevels(self) -> int:
        return lib().orbmi_extractor_get_levels(self._h)

    def GetScaleFactor(self) -> float:
        return lib().orbmi_extractor_get_scale_factor(self._h)

    def GetScaleFactors(self):
        return self._levels_f("orbmi_extractor_get_scale_factors")

    def GetInverseScaleFactors(self):
        return self._levels_f("orbmi_extractor_get_inverse_scale_factors")

    def GetScaleSigmaSquares(self):
        return self._levels_f("orbmi_extractor_get_scale_sigma_squares")

    def GetInverseScaleSigmaSquares(self):
        return self._levels_f("orbmi_extractor_get_inverse_scale_sigma_squares")

    def features_per_level(self):
        out = np.zeros(self.nlevels, np.int32)
        check("orbmi_extractor_get_features_per_level",
              lib().orbmi_extractor_get_features_per_level(self._h, ptr(out)))
        return out

    def pyramid_level(self, level: int, padded: bool = False, item: int = 0) -> np.ndarray:
        """mvImagePyramid[level] of the last extraction (padded: with the 19-px border)."""
        rows, cols = self._shape if self._shape else (4096, 4096)
        cap_w, cap_h = cols + 64, rows + 64
        out = np.zeros((cap_h, cap_w), np.uint8)
        w, h = C.c_int(), C.c_int()
        check("orbmi_extractor_get_pyramid_level",
              lib().orbmi_extractor_get_pyramid_level(self._h, item, level, int(padded), ptr(out),
                                                      cap_w, C.byref(w), C.byref(h)))
        return out[:h.value, :w.value].copy()

    @property
    def mvImagePyramid(self):
        return [self.pyramid_level(l) for l in range(self.nlevels)]


class CameraView(C.Structure):
    """orbmi_camera (include/orbmi.h): mK and mDistCoef (k1 k2 p1 p2 [k3])."""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("dist", C.c_float * 5), ("ndist", C.c_int)]


DEPTH_F32, DEPTH_U16 = 0, 1


def camera_view(cam, dist_coef=None) -> CameraView:
    """cam: anything with fx, fy, cx, cy; dist_coef: 4 or 5 coefficients (default: cam.dist_coef
    when it has one, else no distortion)."""
    if dist_coef is None:
        dist_coef = getattr(cam, "dist_coef", None)
    d = np.zeros(4, np.float32) if dist_coef is None else np.asarray(dist_coef, np.float32).ravel()
    if len(d) not in (4, 5):
        raise ValueError("mDistCoef has 4 or 5 entries (src/Tracking.cc:68-80)")
    c = CameraView(float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy))
    for k, v in enumerate(d):
        c.dist[k] = float(v)
    c.ndist = len(d)
    return c


def _depth_args(depth: np.ndarray):
    """(array kept alive, type, row pitch): a float32 or uint16 map, rows contiguous."""
    depth = np.asarray(depth)
    if depth.ndim != 2 or depth.dtype not in (np.float32, np.uint16):
        raise TypeError("the depth map is a 2-D float32 (CV_32F) or uint16 (CV_16U) array")
    if depth.strides[1] != depth.itemsize or depth.strides[0] < depth.shape[1] * depth.itemsize:
        depth = np.ascontiguousarray(depth)
    return depth, (DEPTH_U16 if depth.dtype == np.uint16 else DEPTH_F32), depth.strides[0]


def compute_image_bounds(cam, dist_coef, rows: int, cols: int) -> np.ndarray:
    """Frame::ComputeImageBounds (src/Frame.cc:471-499) -> float32 (mnMinX, mnMaxX, mnMinY, mnMaxY).
    Runs on the host (no GPU)."""
    d = np.ascontiguousarray(dist_coef, np.float32).ravel()
    out = np.zeros(4, np.float32)
    check("orbmi_compute_image_bounds",
          lib().orbmi_compute_image_bounds(float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy), ptr(d), len(d),
                                           int(rows), int(cols), ptr(out)))
    return out


def compute_stereo_from_rgbd(extractor: "ORBextractor | None", depth: np.ndarray, depth_factor: float, cam,
                             dist_coef, bf: float, n: int | None = None, item: int = 0, keys=None, device: int = 0):
    """Frame::UndistortKeyPoints + Frame::ComputeStereoFromRGBD (src/Frame.cc:434-469, 678-699)
    on the keypoints of `extractor`'s last extraction (n = their count), or on the caller's raw
    `keys` (KP_DTYPE; extractor = None).  depth: float32 or uint16 map (its row pitch is kept);
    depth_factor = mDepthMapFactor (already inverted).  Returns (mvKeysUn, mvuRight, mvDepth)."""
    depth, dtype, step = _depth_args(depth)
    c = camera_view(cam, dist_coef)
    if keys is not None:
        keys = np.ascontiguousarray(keys, KP_DTYPE)
        n = len(keys)
    m = max(int(n), 1)
    ku, u, d = np.zeros(m, KP_DTYPE), np.full(m, -1, np.float32), np.full(m, -1, np.float32)
    rows, cols = depth.shape
    if keys is not None:
        check("orbmi_compute_stereo_from_rgbd_keys",
              lib().orbmi_compute_stereo_from_rgbd_keys(device, ptr(keys), n, ptr(depth), dtype, step, float(depth_factor),
                                                        rows, cols, C.addressof(c), float(bf), ptr(ku), ptr(u), ptr(d)))
    else:
        check("orbmi_compute_stereo_from_rgbd",
              lib().orbmi_compute_stereo_from_rgbd(extractor.handle, item, ptr(depth), dtype, step, float(depth_factor),
                                                   rows, cols, C.addressof(c), float(bf), ptr(ku), ptr(u), ptr(d), int(n)))
    return ku[:n], u[:n], d[:n]


def cvt_gray(image: np.ndarray, rgb: bool, device: int = 0) -> np.ndarray:
    """cvtColor(im, gray, CV_RGB2GRAY | CV_BGR2GRAY | CV_RGBA2GRAY | CV_BGRA2GRAY) as
    Tracking::GrabImageRGBD applies it (src/Tracking.cc:208-224): H x W x 3|4 u8 -> H x W u8, on the
    GPU.  The image's row pitch is kept."""
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] not in (3, 4):
        raise TypeError("cvt_gray expects an H x W x 3 or H x W x 4 uint8 image")
    ch = image.shape[2]
    if image.strides[2] != 1 or image.strides[1] != ch or image.strides[0] < image.shape[1] * ch:
        image = np.ascontiguousarray(image)
    rows, cols = image.shape[:2]
    gray = np.zeros((rows, cols), np.uint8)
    check("orbmi_cvt_gray", lib().orbmi_cvt_gray(device, ptr(image), image.strides[0], ch, 1 if rgb else 0, rows, cols,
                                                 ptr(gray), gray.strides[0]))
    return gray


def compute_stereo_matches(left: ORBextractor, right: ORBextractor, bf: float, fx: float,
                           n_left: int, item_left: int = 0, item_right: int = 0):
    """Frame::ComputeStereoMatches (src/Frame.cc:501-675) on the last extractions of
    `left` and `right`; returns (mvuRight, mvDepth) float32 arrays of n_left entries."""
    u = np.full(max(n_left, 1), -1, np.float32)
    d = np.full(max(n_left, 1), -1, np.float32)
    check("orbmi_compute_stereo_matches",
          lib().orbmi_compute_stereo_matches(left.handle, item_left, right.handle, item_right, bf, fx,
                                             ptr(u), ptr(d), n_left))
    return u[:n_left], d[:n_left]
