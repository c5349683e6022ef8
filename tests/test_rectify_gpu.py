"""Stereo rectification on the MI355X: the remap kernel (csrc/rectify.hip) through the C ABI and
the Python and C++ layers, bit for bit against the numpy restatement (tests/rectify_reference.py);
the rectified pair through extraction and stereo matching against the oracle; and the native loop
on raw frames against a plain handle on the reference-rectified frames."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import rectify_reference as RR
import rectify_scenes as SC

pytestmark = pytest.mark.gpu

PAD = 0xA5


def _lib():
    from orb_slam2_with_comment_amd import _capi
    return _capi.lib()


class Handle:
    """orbmi_rectifier over a pair of float maps."""

    def __init__(self, m1, m2):
        self.m1, self.m2 = np.ascontiguousarray(m1, np.float32), np.ascontiguousarray(m2, np.float32)
        self.rows, self.cols = self.m1.shape
        self.h = C.c_void_p()
        assert _lib().orbmi_rectifier_create(0, self.m1.ctypes.data, self.m2.ctypes.data, self.rows, self.cols,
                                             C.byref(self.h)) == 0

    def close(self):
        _lib().orbmi_rectifier_destroy(self.h)

    def remap(self, src, where="host", dst_step=None, status=False):
        """src: a 2-D u8 array (its row stride is the pitch).  Returns the dst_step-wide buffer,
        pre-filled with PAD."""
        import torch
        dst_step = dst_step or self.cols
        dst = np.full((self.rows, dst_step), PAD, np.uint8)
        step = src.strides[0]
        if where == "device":
            base = src.base if src.base is not None else src  # the whole pitched block goes up
            t_src = torch.from_numpy(np.ascontiguousarray(base)).cuda()
            t_dst = torch.from_numpy(dst).cuda()
            torch.cuda.synchronize()
            rc = _lib().orbmi_remap(self.h, t_src.data_ptr(), src.shape[0], src.shape[1], step, t_dst.data_ptr(), dst_step,
                                    None)
            dst = t_dst.cpu().numpy()
        else:
            rc = _lib().orbmi_remap(self.h, src.ctypes.data, src.shape[0], src.shape[1], step, dst.ctypes.data, dst_step, None)
        if status:
            return rc, dst
        assert rc == 0
        return dst

    def reference(self, src):
        return RR.remap(src, self.m1, self.m2)


def _source(rows, cols, seed=0, pitch=None):
    rng = np.random.default_rng(100 * rows + cols + seed)
    return rng.integers(0, 256, (rows, pitch or cols), dtype=np.uint8)[:, :cols]


def _border_map(rows, cols, src_rows, src_cols, seed=0):
    """Random coordinates from -1.5 to src_cols + 0.5 / src_rows + 0.5: taps on every side of the border."""
    rng = np.random.default_rng(7 * rows + cols + seed)
    return (rng.uniform(-1.5, src_cols + 0.5, (rows, cols)).astype(np.float32),
            rng.uniform(-1.5, src_rows + 0.5, (rows, cols)).astype(np.float32))


def _tap_patterns(m1, m2, src_rows, src_cols):
    """The set of (x class, y class) with a tap inside: 0 = only the second tap inside, 1 = both, 2 = only the first."""
    x0, y0, _, _, out = RR.records(m1, m2)

    def cls(v, n):
        return np.where(v == -1, 0, np.where((v >= 0) & (v < n - 1), 1, np.where(v == n - 1, 2, -1)))
    cx, cy = cls(x0, src_cols), cls(y0, src_rows)
    ok = ~out & (cx >= 0) & (cy >= 0)
    return set(zip(cx[ok].tolist(), cy[ok].tolist()))


# dst cols x rows, src cols x rows
SHAPES = [((1, 1), (41, 29)), ((1, 7), (41, 29)), ((5, 3), (41, 29)), ((37, 23), (41, 29)), ((64, 64), (41, 29)),
          ((65, 33), (16, 16)), ((752, 480), (752, 480))]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("dst,src", SHAPES, ids=[f"{d[0]}x{d[1]}" for d, _ in SHAPES])
def test_remap_shapes(dst, src, where):
    """Every destination size (one pixel, a column, sizes that are no multiple of the 4-pixel store
    or the 256 x 4 block, more than one block, the EuRoC size) over a source larger and smaller than
    it, host and device pointers, a map that crosses every border: bit-equal to the restatement."""
    (cols, rows), (sc, sr) = dst, src
    m1, m2 = _border_map(rows, cols, sr, sc)
    image = _source(sr, sc)
    h = Handle(m1, m2)
    np.testing.assert_array_equal(h.remap(image, where), h.reference(image))
    h.close()


def test_remap_every_phase_and_tap_pattern():
    """752 x 480 random coordinates over a 41 x 29 source: all 1,024 phases and each of the nine
    inside/outside tap patterns occur, and the result is the restatement's."""
    m1, m2 = _border_map(480, 752, 29, 41, seed=3)
    _, _, a, b, out = RR.records(m1, m2)
    assert len(np.unique((a * 32 + b)[~out])) == 1024
    assert _tap_patterns(m1, m2, 29, 41) == {(i, j) for i in range(3) for j in range(3)}
    image = _source(29, 41, seed=3)
    h = Handle(m1, m2)
    ref = h.reference(image)
    assert len(np.unique(ref)) > 200
    np.testing.assert_array_equal(h.remap(image, "device"), ref)
    h.close()


@pytest.mark.parametrize("where", ["host", "device"])
def test_remap_pitches(where):
    """src_step > cols, and dst_step > cols with the padding pre-filled and left untouched (steps
    that are and are not multiples of the 4-byte store)."""
    m1, m2 = _border_map(23, 37, 29, 41, seed=1)
    h = Handle(m1, m2)
    image = _source(29, 41, seed=1, pitch=53)
    assert image.strides[0] == 53
    ref = h.reference(image)
    np.testing.assert_array_equal(h.remap(image, where), ref)
    for step in (40, 43, 64):
        got = h.remap(image, where, dst_step=step)
        np.testing.assert_array_equal(got[:, :37], ref)
        assert (got[:, 37:] == PAD).all()
    h.close()


def test_remap_special_maps():
    """Integral coordinates on the last row and column, ties of the half-even rounding in both
    directions, a wholly outside map, NaN / infinities / 1e30, and an all-255 source."""
    sr, sc = 29, 41
    image = _source(sr, sc, seed=2)
    t = 0.5 / 32
    # integral coordinates: the image itself, last row and column included (their second taps are outside with weight 0)
    uu, vv = np.meshgrid(np.arange(sc, dtype=np.float32), np.arange(sr, dtype=np.float32))
    h = Handle(uu, vv)
    got = h.remap(image)
    np.testing.assert_array_equal(got, image)
    np.testing.assert_array_equal(got, h.reference(image))
    h.close()
    # ties: 10 + 0.5/32 and 11 + 0.5/32 round down to the even 320 and 352, 10 + 1.5/32 up to 322, -0.5/32 to 0
    xs = np.array([10 + t, 11 + t, 10 + 3 * t, 12 - t, -t, 5 + 31 * t], np.float32)
    m1, m2 = np.meshgrid(xs, xs)
    _, _, a, _, _ = RR.records(m1, m2)
    assert a[0].tolist() == [0, 0, 2, 0, 0, 16]
    h = Handle(m1, m2)
    np.testing.assert_array_equal(h.remap(image), h.reference(image))
    h.close()
    # wholly outside, and values that are no coordinates: all 0
    bad = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, -2.0, 1e6, 67108864.0], np.float32)
    m1 = np.tile(bad, (5, 1))
    for a_, b_ in ((m1, np.full_like(m1, 3.0)), (np.full_like(m1, 3.0), m1), (np.full((5, 8), -5.0, np.float32),) * 2):
        h = Handle(a_, b_)
        got = h.remap(image, "device")
        assert (got == 0).all()
        np.testing.assert_array_equal(got, h.reference(image))
        h.close()
    # an interior map over a source of all 255: the weights sum to 1024 at every phase
    rng = np.random.default_rng(9)
    m1 = rng.uniform(0, sc - 1.001, (64, 96)).astype(np.float32)
    m2 = rng.uniform(0, sr - 1.001, (64, 96)).astype(np.float32)
    h = Handle(m1, m2)
    assert (h.remap(np.full((sr, sc), 255, np.uint8)) == 255).all()
    h.close()


def test_remap_pair_equals_two_single_calls():
    """orbmi_remap_pair with handles of two sizes, host and device pointers, a padded destination."""
    import torch
    hl, hr = Handle(*_border_map(23, 37, 29, 41, seed=4)), Handle(*_border_map(19, 37, 29, 41, seed=5))
    sl, sr_ = _source(29, 41, seed=4, pitch=48), _source(29, 41, seed=5, pitch=48)
    ref_l, ref_r = hl.reference(sl), hr.reference(sr_)
    np.testing.assert_array_equal(hl.remap(sl), ref_l)
    np.testing.assert_array_equal(hr.remap(sr_), ref_r)
    dl, dr = np.full((23, 40), PAD, np.uint8), np.full((19, 40), PAD, np.uint8)
    assert _lib().orbmi_remap_pair(hl.h, hr.h, sl.ctypes.data, sr_.ctypes.data, 29, 41, 48, dl.ctypes.data, dr.ctypes.data,
                                   40, None) == 0
    np.testing.assert_array_equal(dl[:, :37], ref_l)
    np.testing.assert_array_equal(dr[:, :37], ref_r)
    assert (dl[:, 37:] == PAD).all() and (dr[:, 37:] == PAD).all()
    tl, tr = torch.from_numpy(sl.base.copy()).cuda(), torch.from_numpy(sr_.base.copy()).cuda()
    ol, orr = torch.zeros((23, 37), dtype=torch.uint8, device="cuda"), torch.zeros((19, 37), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # a NULL stream: device inputs complete on entry, outputs complete on return
    assert _lib().orbmi_remap_pair(hl.h, hr.h, tl.data_ptr(), tr.data_ptr(), 29, 41, 48, ol.data_ptr(), orr.data_ptr(), 37,
                                   None) == 0
    np.testing.assert_array_equal(ol.cpu().numpy(), ref_l)
    np.testing.assert_array_equal(orr.cpu().numpy(), ref_r)
    hl.close()
    hr.close()


SPIN = 5_000_000  # torch.cuda._sleep cycles: the stream stays busy for milliseconds, the host calls take microseconds


def test_callers_stream_orders_the_call_without_a_host_wait():
    """The `stream` argument (a stream of the caller's, not NULL): the source is written on that
    stream behind a spin, by a copy enqueued just before the call, and the destination is read
    after a wait on that stream alone.  The result is right only if the handle's stream waited for
    the caller's and the caller's for the handle's; the caller's stream is still busy when the call
    returns, so the host did not wait.  A single image and a pair."""
    import torch
    hl, hr = Handle(*_border_map(23, 37, 29, 41, seed=8)), Handle(*_border_map(23, 37, 29, 41, seed=9))
    il, ir = np.ascontiguousarray(_source(29, 41, seed=8)), np.ascontiguousarray(_source(29, 41, seed=9))
    pl, pr = torch.from_numpy(il).pin_memory(), torch.from_numpy(ir).pin_memory()
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    vp = C.c_void_p
    for pair in (False, True):
        with torch.cuda.stream(side):
            sl = torch.zeros((29, 41), dtype=torch.uint8, device="cuda")
            sr = torch.zeros((29, 41), dtype=torch.uint8, device="cuda")
            dl = torch.full((23, 37), PAD, dtype=torch.uint8, device="cuda")
            dr = torch.full((23, 37), PAD, dtype=torch.uint8, device="cuda")
            side.synchronize()
            torch.cuda._sleep(SPIN)
            sl.copy_(pl, non_blocking=True)
            sr.copy_(pr, non_blocking=True)
            if pair:
                rc = _lib().orbmi_remap_pair(hl.h, hr.h, vp(sl.data_ptr()), vp(sr.data_ptr()), 29, 41, 41, vp(dl.data_ptr()),
                                             vp(dr.data_ptr()), 37, vp(side.cuda_stream))
            else:
                rc = _lib().orbmi_remap(hl.h, vp(sl.data_ptr()), 29, 41, 41, vp(dl.data_ptr()), 37, vp(side.cuda_stream))
            busy = not side.query()
            assert rc == 0
            assert busy, "the call returned after the caller's stream had drained: it waited on the host"
            side.synchronize()
        np.testing.assert_array_equal(dl.cpu().numpy(), hl.reference(il))
        if pair:
            np.testing.assert_array_equal(dr.cpu().numpy(), hr.reference(ir))
    hl.close()
    hr.close()


def test_handles_reused_alternated_and_refused():
    """One handle with three sources of different sizes; two handles of different sizes used
    alternately; a refused source size or pitch returns ORBMI_E_ARG, writes nothing, and the
    next valid call is correct."""
    from orb_slam2_with_comment_amd._capi import ORBMI_E_ARG
    a, b = Handle(*_border_map(23, 37, 29, 41, seed=6)), Handle(*_border_map(33, 65, 16, 16, seed=7))
    for k, (sr, sc) in enumerate([(29, 41), (16, 16), (50, 70), (29, 41)]):
        image = _source(sr, sc, seed=10 + k)
        for h in (a, b, a):
            np.testing.assert_array_equal(h.remap(image, "host" if k % 2 else "device"), h.reference(image))
    image = _source(29, 41, seed=20)
    dst = np.full((23, 37), PAD, np.uint8)
    L = _lib()
    assert L.orbmi_remap(a.h, image.ctypes.data, 29, 32768, 32768, dst.ctypes.data, 37, None) == ORBMI_E_ARG  # too wide
    assert L.orbmi_remap(a.h, image.ctypes.data, 32768, 41, 41, dst.ctypes.data, 37, None) == ORBMI_E_ARG     # too tall
    assert L.orbmi_remap(a.h, image.ctypes.data, 29, 41, 40, dst.ctypes.data, 37, None) == ORBMI_E_ARG        # src_step < cols
    assert L.orbmi_remap(a.h, image.ctypes.data, 29, 41, 41, dst.ctypes.data, 36, None) == ORBMI_E_ARG        # dst_step < cols
    assert L.orbmi_remap(a.h, None, 29, 41, 41, dst.ctypes.data, 37, None) == ORBMI_E_ARG
    assert L.orbmi_remap(None, image.ctypes.data, 29, 41, 41, dst.ctypes.data, 37, None) == ORBMI_E_ARG
    assert (dst == PAD).all()
    np.testing.assert_array_equal(a.remap(image), a.reference(image))
    h = C.c_void_p(1)
    m = np.zeros((2, 2), np.float32)
    assert L.orbmi_rectifier_create(0, m.ctypes.data, m.ctypes.data, 0, 2, C.byref(h)) == ORBMI_E_ARG and not h.value
    a.close()
    b.close()


# ---- the EuRoC rig: Python layer, chain, loop, C++ layer --------------------------------------------
@pytest.fixture(scope="module")
def rectifier():
    from orb_slam2_with_comment_amd.rectify import StereoRectifier
    r = StereoRectifier(SC.euroc_settings(), 0)
    yield r
    r.close()


def test_python_stereo_rectifier(rectifier):
    """StereoRectifier: maps() are the restatement's, numpy pairs and device tensors give the
    reference-rectified pair, `out` is filled in place."""
    import torch
    for got, ref in zip(rectifier.maps(), SC.euroc_maps()):
        np.testing.assert_array_equal(got[0].view(np.uint32), ref[0].view(np.uint32))
        np.testing.assert_array_equal(got[1].view(np.uint32), ref[1].view(np.uint32))
    L, R, _ = SC.raw_frames()[3]
    ref_l, ref_r = SC.rectified_frames()[3]
    gl, gr = rectifier(L, R)
    np.testing.assert_array_equal(gl, ref_l)
    np.testing.assert_array_equal(gr, ref_r)
    tl, tr = rectifier(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda())
    assert tl.is_cuda and tr.is_cuda
    np.testing.assert_array_equal(tl.cpu().numpy(), ref_l)
    np.testing.assert_array_equal(tr.cpu().numpy(), ref_r)
    out = (np.zeros_like(L), np.zeros_like(R))
    rectifier(L, R, out=out)
    np.testing.assert_array_equal(out[0], ref_l)
    np.testing.assert_array_equal(rectifier.left(L), ref_l)
    np.testing.assert_array_equal(rectifier.right(torch.from_numpy(R).cuda()).cpu().numpy(), ref_r)
    # sources still being written when the call is made, by an asynchronous copy behind a spin: on
    # torch's default stream the call waits for it first; under a stream of its own it is ordered on
    # that stream and returns while the stream is busy
    pl, pr = torch.from_numpy(L).pin_memory(), torch.from_numpy(R).pin_memory()
    for side in (None, torch.cuda.Stream()):
        with torch.cuda.stream(side):
            tl, tr = torch.zeros_like(pl, device="cuda"), torch.zeros_like(pr, device="cuda")
            torch.cuda.current_stream().synchronize()
            torch.cuda._sleep(SPIN)
            tl.copy_(pl, non_blocking=True)
            tr.copy_(pr, non_blocking=True)
            gl, gr = rectifier(tl, tr)
            if side is not None:
                assert not side.query(), "the call waited on the host"
                side.synchronize()
        np.testing.assert_array_equal(gl.cpu().numpy(), ref_l)
        np.testing.assert_array_equal(gr.cpu().numpy(), ref_r)


def test_rectified_pair_through_extraction_and_stereo(rectifier, oracle):
    """The raw pair rectified into one device buffer, then orbmi_extract_batch_device and
    orbmi_compute_stereo_matches_batch_device on it: the oracle's keypoints, descriptors and stereo
    matches on the reference-rectified pair."""
    import torch
    import orb_slam2_with_comment_amd as orb
    from orb_slam2_with_comment_amd import _capi
    s = SC.euroc_settings()
    L, R, _ = SC.raw_frames()[0]
    ref_l, ref_r = SC.rectified_frames()[0]
    rows, cols = ref_l.shape
    pair = torch.zeros((2, rows, cols), dtype=torch.uint8, device="cuda")
    rectifier(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), out=(pair[0], pair[1]))
    torch.cuda.synchronize()
    cap = s.n_features + 16 * s.n_levels + 64
    ex = orb.ORBextractor(s.n_features, float(s.scale_factor), s.n_levels, s.ini_th_fast, s.min_th_fast)
    d_kps = torch.zeros(2 * cap * 28, dtype=torch.uint8, device="cuda")
    d_desc = torch.zeros(2 * cap * 32, dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    d_u = torch.zeros(2 * cap, dtype=torch.float32, device="cuda")
    d_d = torch.zeros(2 * cap, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    vp, lib = C.c_void_p, _capi.lib()
    _capi.check("orbmi_extract_batch_device", lib.orbmi_extract_batch_device(
        ex.handle, vp(pair.data_ptr()), 2, rows, cols, cols, rows * cols, vp(d_kps.data_ptr()), vp(d_desc.data_ptr()),
        vp(d_cnt.data_ptr()), cap))
    _capi.check("orbmi_compute_stereo_matches_batch_device", lib.orbmi_compute_stereo_matches_batch_device(
        ex.handle, float(s.bf), float(s.fx), vp(d_u.data_ptr()), vp(d_d.data_ptr())))
    _capi.check("orbmi_extractor_synchronize", lib.orbmi_extractor_synchronize(ex.handle))
    p = oracle.params(s.n_features, float(s.scale_factor), s.n_levels, s.ini_th_fast, s.min_th_fast)
    kl, dl = oracle.extract(p, ref_l)
    kr, dr = oracle.extract(p, ref_r)
    ru, rd = oracle.stereo(p, ref_l, ref_r, float(s.bf), float(s.fx), kl, dl, kr, dr)
    n = len(kl)
    assert d_cnt.cpu().tolist() == [n, len(kr)] and n > 500
    np.testing.assert_array_equal(d_kps.cpu().numpy()[:28 * n].view(_capi.KP_DTYPE), kl)
    np.testing.assert_array_equal(d_desc.cpu().numpy()[:32 * n].reshape(n, 32), np.asarray(dl).reshape(n, 32))
    np.testing.assert_array_equal(d_u.cpu().numpy()[:n], ru)
    np.testing.assert_array_equal(d_d.cpu().numpy()[:n], rd)
    assert (rd > 0).sum() >= 500


_STAT_KEYS = ("frame", "n", "state", "init", "track", "lf_matches", "bow_matches", "nmatches_map", "local_map_points",
              "local_matches", "inliers", "need_kf", "keyframes", "mappoints", "reset")


@pytest.mark.parametrize("ahead", [False, True], ids=["plain", "next_pair"])
def test_native_loop_on_raw_frames_equals_plain_on_rectified(ahead):
    """NativeStereoSLAM(rectify=True) on the 12 raw frames (synchronous LocalMapping) against a plain
    handle on the reference-rectified frames: every Tcw, every stats record and the counts bit for
    bit, also with next_pair.  A raw frame of the wrong size returns ORBMI_E_ARG and the next
    frame tracks."""
    from orb_slam2_with_comment_amd import _capi
    from orb_slam2_with_comment_amd.native_slam import NativeStereoSLAM
    from orb_slam2_with_comment_amd.system import OK
    from slam_backends import small_vocabulary
    s, voc = SC.euroc_settings(), small_vocabulary()
    raw = [(L, R) for L, R, _ in SC.raw_frames()]
    rect = SC.rectified_frames()

    def drive(slam, frames, bad_at=None):
        poses = []
        for f, (L, R) in enumerate(frames):
            if f == bad_at:
                with pytest.raises(_capi.OrbmiError) as e:
                    slam.TrackStereo(L[:-1], R[:-1], f / 20.0)
                assert e.value.code == _capi.ORBMI_E_ARG
            nxt = frames[f + 1] if ahead and f + 1 < len(frames) else None
            poses.append(slam.TrackStereo(L, R, f / 20.0, next_pair=nxt) if ahead else slam.TrackStereo(L, R, f / 20.0))
        return poses

    gpu = NativeStereoSLAM(s, device=0, vocabulary=voc, rectify=True)
    ref = NativeStereoSLAM(s, device=0, vocabulary=voc)
    pa, pb = drive(gpu, raw, bad_at=5), drive(ref, rect)
    for f, (a, b) in enumerate(zip(pa, pb)):
        assert a is not None and b is not None, f
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=f"Tcw of frame {f}")
    sa, sb = gpu.stats, ref.stats
    assert len(sa) == len(sb) == len(raw)
    for a, b in zip(sa, sb):
        assert {k: a.get(k) for k in _STAT_KEYS} == {k: b.get(k) for k in _STAT_KEYS}, (a, b)
    assert sa[0]["init"] is True and all(st["state"] == OK for st in sa)
    assert gpu.counts() == ref.counts() and gpu.counts()["keyframes"] >= 2
    np.testing.assert_array_equal(gpu.trajectory_twc(), ref.trajectory_twc())
    gpu.Shutdown()
    ref.Shutdown()


def test_rectifying_handle_refuses_other_cameras():
    """The cameras' sizes must be the settings': ORBMI_E_ARG and no handle; rectify=True without
    LEFT / RIGHT parameters raises."""
    import dataclasses
    from orb_slam2_with_comment_amd import _capi
    from orb_slam2_with_comment_amd.native_slam import NativeStereoSLAM
    s = SC.euroc_settings()
    for change in ({"LEFT.height": 479}, {"RIGHT.width": 751}, {"LEFT.D": np.zeros((1, 6))}):
        with pytest.raises(_capi.OrbmiError) as e:
            NativeStereoSLAM(dataclasses.replace(s, raw={**s.raw, **change}), device=0, rectify=True)
        assert e.value.code == _capi.ORBMI_E_ARG
    plain = {k: v for k, v in s.raw.items() if not k.startswith(("LEFT.", "RIGHT."))}
    with pytest.raises(ValueError):
        NativeStereoSLAM(dataclasses.replace(s, raw=plain), device=0, rectify=True)


def test_cpp_dropin_rectify(tmp_path):
    """orbmi::StereoRectifier from C++ (tests/cpp/dropin_rectify.cpp) on a raw pair: the
    reference-rectified pair."""
    from test_cpp_dropin import build_dropin
    exe = build_dropin(str(tmp_path), "dropin_rectify")
    L, R, _ = SC.raw_frames()[7]
    cams = []
    for c in SC.euroc_settings().rectification:
        D = np.zeros(8)
        D[:len(c.D)] = c.D
        cams.append(np.concatenate([c.K.ravel(), D, [len(c.D)], c.R.ravel(), c.P.ravel(), [c.rows, c.cols]]))
    np.concatenate(cams).astype(np.float64).tofile(tmp_path / "cams.bin")
    L.tofile(tmp_path / "l.raw")
    R.tofile(tmp_path / "r.raw")
    subprocess.run([exe, str(tmp_path / "cams.bin"), str(tmp_path / "l.raw"), str(tmp_path / "r.raw"), "480", "752",
                    str(tmp_path / "out.bin")], check=True, timeout=120)
    out = np.fromfile(tmp_path / "out.bin", np.uint8).reshape(2, 480, 752)
    ref_l, ref_r = SC.rectified_frames()[7]
    np.testing.assert_array_equal(out[0], ref_l)
    np.testing.assert_array_equal(out[1], ref_r)
