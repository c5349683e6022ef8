"""Stereo rectification on the device (orbmi_rectifier_* / orbmi_remap* in include/orbmi.h): what
Examples/Stereo/stereo_euroc.cc:55-137 does with cv::initUndistortRectifyMap and cv::remap in
front of TrackStereo.  The maps are built once on the host, the remap of each pair is one launch
of the HIP kernel in csrc/rectify.hip."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._capi import check, lib
from .settings import RectifyCamera, Settings  # noqa: F401


class RectifyCameraStruct(C.Structure):
    """orbmi_rectify_camera (include/orbmi.h)."""
    _fields_ = [("K", C.c_double * 9), ("D", C.c_double * 8), ("nd", C.c_int), ("R", C.c_double * 9),
                ("P", C.c_double * 12), ("rows", C.c_int), ("cols", C.c_int)]


def camera_struct(cam: RectifyCamera) -> RectifyCameraStruct:
    c = RectifyCameraStruct()
    D = np.asarray(cam.D, np.float64).ravel()
    if len(D) > 8:
        raise ValueError("D has at most 8 coefficients here (thin-prism and tilt terms are not built)")
    c.K[:] = np.asarray(cam.K, np.float64).ravel().tolist()
    c.D[:] = D.tolist() + [0.0] * (8 - len(D))
    c.nd = len(D)
    c.R[:] = np.asarray(cam.R, np.float64).ravel().tolist()
    c.P[:] = np.asarray(cam.P, np.float64).ravel().tolist()
    c.rows, c.cols = int(cam.rows), int(cam.cols)
    return c


def init_undistort_rectify_map(cam: RectifyCamera):
    """cv::initUndistortRectifyMap(K, D, R, P[0:3, 0:3], size, CV_32F): (map1, map2), host only."""
    c = camera_struct(cam)
    m1 = np.empty((max(c.rows, 0), max(c.cols, 0)), np.float32)
    m2 = np.empty_like(m1)
    check("orbmi_init_undistort_rectify_map",
          lib().orbmi_init_undistort_rectify_map(C.addressof(c), m1.ctypes.data, m2.ctypes.data))
    return m1, m2


class Rectifier:
    """One camera's maps on the device (orbmi_rectifier): cv::remap(src, dst, map1, map2,
    INTER_LINEAR) of u8 gray images, numpy arrays or torch tensors of that device."""

    def __init__(self, map1, map2, device: int = 0):
        m1 = np.ascontiguousarray(map1, np.float32)
        m2 = np.ascontiguousarray(map2, np.float32)
        if m1.ndim != 2 or m1.shape != m2.shape:
            raise ValueError("map1 and map2 are two float images of one size")
        self.shape = m1.shape
        self.device = device
        h = C.c_void_p()
        check("orbmi_rectifier_create", lib().orbmi_rectifier_create(device, m1.ctypes.data, m2.ctypes.data,
                                                                      m1.shape[0], m1.shape[1], C.byref(h)))
        self._h = h

    def __call__(self, src, out=None):
        s, dst = _image(src, self.device), _output(src, out, self.shape, self.device)
        stream = _call_stream(self.device, s.array, dst.array)
        check("orbmi_remap", lib().orbmi_remap(self._h, s.ptr, s.rows, s.cols, s.step, dst.ptr, dst.step, stream))
        return dst.array

    def close(self):
        if getattr(self, "_h", None):
            lib().orbmi_rectifier_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _View:
    """Pointer, size and pitch of a 2-D u8 image."""

    def __init__(self, array, ptr, rows, cols, step):
        self.array, self.ptr, self.rows, self.cols, self.step = array, ptr, rows, cols, step


def _call_stream(device, *arrays):
    """The `stream` argument of a call on these images.  All of them tensors and the current torch
    stream a stream of its own: that stream's handle -- the call is ordered on it and does not
    block the host.  Otherwise NULL, which makes the call return with its outputs complete; the
    handle's stream does not wait for torch's default stream by itself (it is a non-blocking
    stream and the default stream has no handle to pass), so when a tensor is involved the current
    torch stream is synchronised first: a source still being written by an earlier torch kernel is
    then finished before it is read."""
    if not any(_is_tensor(a) for a in arrays):
        return None
    import torch
    cur = torch.cuda.current_stream(device)
    if cur.cuda_stream and all(_is_tensor(a) for a in arrays):
        return C.c_void_p(cur.cuda_stream)
    cur.synchronize()
    return None


def _is_tensor(a) -> bool:
    return type(a).__module__.startswith("torch")


def _image(a, device) -> _View:
    if _is_tensor(a):
        import torch
        if a.dtype != torch.uint8 or a.dim() != 2 or a.stride(1) != 1 or not a.is_cuda or a.device.index != device:
            raise ValueError("a device image is a 2-D uint8 tensor of the rectifier's device with contiguous rows")
        return _View(a, a.data_ptr(), a.shape[0], a.shape[1], a.stride(0))
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise ValueError("an image is a 2-D uint8 array")
    if a.strides[1] != 1:
        a = np.ascontiguousarray(a)
    return _View(a, a.ctypes.data, a.shape[0], a.shape[1], a.strides[0])


def _output(src, out, shape, device) -> _View:
    if out is None:
        if _is_tensor(src):
            import torch
            out = torch.empty(shape, dtype=torch.uint8, device=src.device)
        else:
            out = np.empty(shape, np.uint8)
    v = _image(out, device)
    if v.array is not out or (v.rows, v.cols) != tuple(shape):
        raise ValueError("out is a uint8 image of the maps' size with contiguous rows")
    return v


class StereoRectifier:
    """Both cameras of a rig: StereoRectifier(settings | (left, right) RectifyCamera, device).
    rect(left, right) remaps a raw pair in one launch (orbmi_remap_pair) and returns the rectified
    pair: numpy arrays for numpy input, device tensors for torch tensors.  Under a torch stream of
    its own (torch.cuda.stream(...)) the call is ordered on that stream and does not block the
    host; on torch's default stream it waits for that stream first and returns with the outputs
    complete (_call_stream)."""

    def __init__(self, settings_or_cameras, device: int = 0):
        cams = settings_or_cameras
        if isinstance(cams, str):
            from .settings import load_settings
            cams = load_settings(cams)
        if isinstance(cams, Settings):
            if cams.rectification is None:
                raise ValueError("the settings file has no LEFT / RIGHT rectification parameters")
            cams = cams.rectification
        self.cameras = tuple(cams)
        if len(self.cameras) != 2:
            raise ValueError("a left and a right camera")
        self.device = device
        self._maps = tuple(init_undistort_rectify_map(c) for c in self.cameras)
        self.left, self.right = (Rectifier(m1, m2, device) for m1, m2 in self._maps)

    def maps(self):
        """((M1l, M2l), (M1r, M2r)) as stereo_euroc.cc:92-93 builds them."""
        return self._maps

    def __call__(self, left, right, out=None):
        L, R = _image(left, self.device), _image(right, self.device)
        if (L.rows, L.cols, L.step) != (R.rows, R.cols, R.step) or _is_tensor(left) != _is_tensor(right):
            return self.left(left, out and out[0]), self.right(right, out and out[1])
        oL = _output(left, out and out[0], self.left.shape, self.device)
        oR = _output(right, out and out[1], self.right.shape, self.device)
        if oL.step != oR.step:
            return self.left(left, oL.array), self.right(right, oR.array)
        stream = _call_stream(self.device, L.array, R.array, oL.array, oR.array)
        check("orbmi_remap_pair", lib().orbmi_remap_pair(self.left._h, self.right._h, L.ptr, R.ptr, L.rows, L.cols, L.step,
                                                         oL.ptr, oR.ptr, oL.step, stream))
        return oL.array, oR.array

    def close(self):
        self.left.close()
        self.right.close()
