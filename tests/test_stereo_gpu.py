"""GPU parity: Frame::ComputeStereoMatches on MI355X vs the CPU restatement (bit-exact)."""
import ctypes as C
import os

import numpy as np
import pytest

import stereo_reference as SR
import stereo_scenes as SC
from orb_slam2_with_comment_amd import synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _pair(orb, p):
    mk = lambda: orb.ORBextractor(p.nfeatures, p.scale_factor, p.nlevels, p.ini_th_fast, p.min_th_fast)
    return mk(), mk()


@pytest.mark.parametrize("frame", [0, 5, 23])
def test_stereo_parity(oracle, frame):
    import orb_slam2_with_comment_amd as orb
    p = oracle.params(2000)
    exL, exR = _pair(orb, p)
    L, R, _ = synth.stereo_pair(synth.KITTI, frame)
    kl, dl = exL(L)
    kr, dr = exR(R)
    u, d = orb.compute_stereo_matches(exL, exR, synth.KITTI.bf, synth.KITTI.fx, len(kl))
    u_ref, d_ref = oracle.stereo(p, L, R, synth.KITTI.bf, synth.KITTI.fx, kl, dl, kr, dr)
    bad = np.nonzero((u != u_ref) | (d != d_ref))[0]
    assert len(bad) == 0, f"{len(bad)} mismatches, first {bad[:5]}: gpu {u[bad[:3]]} ref {u_ref[bad[:3]]}"
    assert (d > 0).sum() > 300


def test_stereo_golden(oracle):
    import orb_slam2_with_comment_amd as orb
    g = np.load(os.path.join(GOLD, "kitti_stereo_f0.npz"), allow_pickle=False)
    exL, exR = _pair(orb, oracle.params(2000))
    kl, _ = exL(g["left"])
    exR(g["right"])
    u, d = orb.compute_stereo_matches(exL, exR, float(g["bf"]), float(g["fx"]), len(kl))
    np.testing.assert_array_equal(u, g["u_right"])
    np.testing.assert_array_equal(d, g["depth"])


def test_stereo_no_matches(oracle):
    """Right image unrelated to the left: few/no matches; empty-median case defined."""
    import orb_slam2_with_comment_amd as orb
    p = oracle.params(2000)
    exL, exR = _pair(orb, p)
    L, _, _ = synth.stereo_pair(synth.KITTI, 0)
    R = np.full_like(L, 128)
    R[::7, ::5] = 255
    kl, dl = exL(L)
    kr, dr = exR(R)
    u, d = orb.compute_stereo_matches(exL, exR, synth.KITTI.bf, synth.KITTI.fx, len(kl))
    if dr is None:
        kr, dr = kr[:0], np.zeros((0, 32), np.uint8)
    u_ref, d_ref = oracle.stereo(p, L, R, synth.KITTI.bf, synth.KITTI.fx, kl, dl, kr, dr)
    np.testing.assert_array_equal(u, u_ref)
    np.testing.assert_array_equal(d, d_ref)


# ---- every branch, size and pyramid setting (tests/stereo_scenes.py) ---------------------
# The kernels against the numpy restatement of tests/stereo_reference.py, bit for bit.


def _extract(ex, image, capacity=None):
    """orbmi_extract with a chosen capacity (the Python mirror picks its own)."""
    from orb_slam2_with_comment_amd import _capi
    if capacity is None:
        return ex(image)
    image = np.ascontiguousarray(image)
    kps = np.zeros(capacity, _capi.KP_DTYPE)
    desc = np.zeros((capacity, 32), np.uint8)
    n = C.c_int()
    _capi.check("orbmi_extract", _capi.lib().orbmi_extract(ex.handle, _capi.ptr(image), image.shape[0], image.shape[1],
                                                           image.strides[0], _capi.ptr(kps), _capi.ptr(desc), capacity,
                                                           C.byref(n)))
    return kps[:n.value].copy(), desc[:n.value].copy()


def _set_keypoints(ex, item, kps, desc):
    from orb_slam2_with_comment_amd import _capi
    kps = np.ascontiguousarray(kps, _capi.KP_DTYPE)
    desc = np.ascontiguousarray(desc, np.uint8)
    return _capi.lib().orbmi_debug_set_keypoints(ex.handle, item, _capi.ptr(kps), _capi.ptr(desc), len(kps))


def _assert_bit_equal(u, d, res, what):
    bad = np.nonzero((u.view(np.uint32) != res.u_right.view(np.uint32))
                     | (d.view(np.uint32) != res.depth.view(np.uint32)))[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(u)} keypoints differ, first {bad[0]} "
                           f"({SR.OUTCOME_NAMES[res.outcome[bad[0]]]}): gpu {u[bad[0]]!r} {d[bad[0]]!r}, "
                           f"restatement {res.u_right[bad[0]]!r} {res.depth[bad[0]]!r}")


def _run_scene(oracle, scene):
    import orb_slam2_with_comment_amd as orb
    mk = lambda: orb.ORBextractor(scene.nfeatures, scene.scale_factor, scene.nlevels, 20, 7)
    exL, exR = mk(), mk()
    own = _extract(exL, scene.left, scene.capacity) + _extract(exR, scene.right, scene.capacity)
    for v in scene.variants:
        kps = v.kps or own
        if v.kps is not None:
            assert _set_keypoints(exL, 0, kps[0], kps[1]) == 0 and _set_keypoints(exR, 0, kps[2], kps[3]) == 0
        res = SC.reference(oracle, scene, v, kps=None if v.kps else own)
        u, d = orb.compute_stereo_matches(exL, exR, scene.bf, scene.fx, len(kps[0]))
        _assert_bit_equal(u, d, res, f"{scene.name}/{v.name}")


@pytest.mark.parametrize("scene", ["branches", "identical", "median_ranks", "counts"])
def test_stereo_scene(oracle, scene):
    _run_scene(oracle, SC.scene(scene))


@pytest.mark.parametrize("which", ["above", "bin255"])
def test_stereo_high_sad(oracle, which):
    """SADs beyond 2^15 (both patches lose their centre pixel: up to 121 * 510)."""
    _run_scene(oracle, SC.scene(f"high_sad_{which}"))


@pytest.mark.parametrize("key", list(SC.PYRAMIDS))
@pytest.mark.parametrize("kind", ["own", "top"])
def test_stereo_pyramids(oracle, kind, key):
    """Other pyramids than 1.2 x 8; `top` fills the row list to its bound (a parity test of the
    sizing in stereo_run, ceil(4 * max scale) + 2 rows per right keypoint)."""
    _run_scene(oracle, SC.scene(f"pyramid_{kind}_{key}"))


@pytest.mark.parametrize("sf,nl,rows,cols", SC.PYRAMIDS_REFUSED)
def test_stereo_pyramid_below_one_cell_is_refused(sf, nl, rows, cols):
    import orb_slam2_with_comment_amd as orb
    from orb_slam2_with_comment_amd import _capi
    ex = orb.ORBextractor(500, sf, nl, 20, 7)
    with pytest.raises(_capi.OrbmiError) as e:
        ex(np.zeros((rows, cols), np.uint8))
    assert e.value.code == _capi.ORBMI_E_UNSUPPORTED


def test_stereo_tall(oracle):
    """A portrait image near the tallest the extractor takes, with crafted keypoints down to the
    last rows the reference allows."""
    _run_scene(oracle, SC.scene("tall"))


@pytest.mark.parametrize("rows,cols", SC.TALL_REFUSED)
def test_stereo_row_table_bound_is_out_of_reach(rows, cols):
    """Images at k_stereo_rows' bound (4,095 rows) and past it are refused at extraction, before
    any stereo launch; a stereo call on the handle then reports an error and leaves its outputs
    alone."""
    import orb_slam2_with_comment_amd as orb
    from orb_slam2_with_comment_amd import _capi
    ex = orb.ORBextractor(500, 1.2, 8, 20, 7)
    with pytest.raises(_capi.OrbmiError) as e:
        ex(np.zeros((rows, cols), np.uint8))
    assert e.value.code == _capi.ORBMI_E_UNSUPPORTED
    u = np.full(8, 7.5, np.float32)
    d = np.full(8, 7.5, np.float32)
    rc = _capi.lib().orbmi_compute_stereo_matches(ex.handle, 0, ex.handle, 0, 10.0, 40.0, _capi.ptr(u), _capi.ptr(d), 8)
    # E_STATE, and only because the refused extraction left the handle without a batch: this is no
    # test of stereo_run's own `rows + 1 > 4,096` refusal, which no reachable image gets to (nor of
    # the row scan with a row count near 4,096)
    assert rc == _capi.ORBMI_E_STATE
    assert (u == 7.5).all() and (d == 7.5).all()


def test_stereo_batch(oracle):
    """Three pairs in one handle (caller's device buffers, different counts, one pair without
    right keypoints) through the batch entry, then the same items through the single entry."""
    import torch
    import orb_slam2_with_comment_amd as orb
    from orb_slam2_with_comment_amd import _capi
    L = _capi.lib()
    scenes = SC.batch()
    rows, cols = scenes[0].left.shape
    cap, nb = 600, 2 * len(scenes)
    ex = orb.ORBextractor(500, 1.2, 8, 20, 7)
    imgs = torch.from_numpy(np.stack([im for s in scenes for im in (s.left, s.right)])).cuda()
    d_kps = torch.zeros(nb * cap * 28, dtype=torch.uint8, device="cuda")
    d_desc = torch.zeros(nb * cap * 32, dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros(nb, dtype=torch.int32, device="cuda")
    d_u = torch.full((nb * cap,), 7.5, dtype=torch.float32, device="cuda")
    d_d = torch.full((nb * cap,), 7.5, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    vp = C.c_void_p
    _capi.check("orbmi_extract_batch_device", L.orbmi_extract_batch_device(
        ex.handle, vp(imgs.data_ptr()), nb, rows, cols, cols, rows * cols, vp(d_kps.data_ptr()), vp(d_desc.data_ptr()),
        vp(d_cnt.data_ptr()), cap))
    for p, s in enumerate(scenes):
        kl, dl, kr, dr = s.variants[0].kps
        assert _set_keypoints(ex, 2 * p, kl, dl) == 0 and _set_keypoints(ex, 2 * p + 1, kr, dr) == 0
    assert _set_keypoints(ex, nb, kl, dl) == _capi.ORBMI_E_STATE
    assert _set_keypoints(ex, 0, np.zeros(cap + 1, _capi.KP_DTYPE), np.zeros((cap + 1, 32), np.uint8)) == _capi.ORBMI_E_CAP
    _capi.check("orbmi_compute_stereo_matches_batch_device", L.orbmi_compute_stereo_matches_batch_device(
        ex.handle, scenes[0].bf, scenes[0].fx, vp(d_u.data_ptr()), vp(d_d.data_ptr())))
    _capi.check("orbmi_extractor_synchronize", L.orbmi_extractor_synchronize(ex.handle))
    u_all, d_all = d_u.cpu().numpy(), d_d.cpu().numpy()
    assert d_cnt.cpu().tolist() == [n for s in scenes for n in (len(s.variants[0].kps[0]), len(s.variants[0].kps[2]))]
    for p, s in enumerate(scenes):
        res = SC.reference(oracle, s, s.variants[0])
        n = len(res.u_right)
        at = 2 * p * cap
        _assert_bit_equal(u_all[at:at + n].copy(), d_all[at:at + n].copy(), res, f"batch entry, pair {p}")
        assert (u_all[at + n:at + 2 * cap] == 7.5).all()  # nothing past the count, nothing in the right item's slots
        u, d = orb.compute_stereo_matches(ex, ex, s.bf, s.fx, n, item_left=2 * p, item_right=2 * p + 1)
        _assert_bit_equal(u, d, res, f"single entry, items {2 * p}, {2 * p + 1}")
    with pytest.raises(_capi.OrbmiError) as e:  # n_left short of the item's count
        orb.compute_stereo_matches(ex, ex, 10.0, 40.0, len(scenes[2].variants[0].kps[0]) - 1, item_left=4, item_right=5)
    assert e.value.code == _capi.ORBMI_E_CAP


def test_stereo_status_codes():
    import orb_slam2_with_comment_amd as orb
    from orb_slam2_with_comment_amd import _capi
    img = SC.branches().left

    def code(left, right, n=4096):
        with pytest.raises(_capi.OrbmiError) as e:
            orb.compute_stereo_matches(left, right, 10.0, 40.0, n)
        return e.value.code

    a, b = orb.ORBextractor(500, 1.2, 8, 20, 7), orb.ORBextractor(500, 1.2, 8, 20, 7)
    assert code(a, b) == _capi.ORBMI_E_STATE  # before any extraction
    assert _set_keypoints(a, 0, np.zeros(1, _capi.KP_DTYPE), np.zeros((1, 32), np.uint8)) == _capi.ORBMI_E_STATE
    a(img)
    assert code(a, b) == _capi.ORBMI_E_STATE  # the right handle still has none
    # the hook takes only keypoints the kernels can index: octave inside the pyramid, x and y inside the image
    one = SC.make_kps([10.0], [10.0], [0], SC.scale_tables(1.2, 8)[0])
    for field, value in (("octave", 8), ("octave", -1), ("y", 300.0), ("y", -1.0), ("x", 400.0), ("x", np.nan)):
        bad = one.copy()
        bad[field] = value
        assert _set_keypoints(a, 0, bad, np.zeros((1, 32), np.uint8)) == _capi.ORBMI_E_ARG, (field, value)
    assert _set_keypoints(a, 0, one, np.zeros((1, 32), np.uint8)) == 0
    b(img[:240, :320])
    assert code(a, b) == _capi.ORBMI_E_ARG    # another shape
    c = orb.ORBextractor(500, 1.2, 4, 20, 7)
    c(img)
    assert code(a, c) == _capi.ORBMI_E_ARG    # another level count
