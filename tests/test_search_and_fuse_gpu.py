"""GPU parity of CorrectLoop's SearchAndFuse: orbmi_fuse_sim3_search_batch (k_fuse_sim3) against the
numpy restatement tests/fuse_sim3_reference.py with no tolerance, at the group, wave and block edges
of eight lanes per point, with keyframes of different sizes in one batch; the candidate-overflow
scene, bad arguments and determinism; then loop.search_and_fuse and loop.correct_loop over the
library against the same code over the restatement."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_sim3_reference as ref  # noqa: E402
import sim3opt_reference as so  # noqa: E402
import test_search_and_fuse_cpu as cpu  # noqa: E402
from test_essgraph_gpu import POSE_TOL  # noqa: E402

pytestmark = pytest.mark.gpu

ORBMI_OK, ORBMI_E_ARG = 0, -1
F32, F64 = np.float32, np.float64
MAXIMA = {}


@pytest.fixture(scope="module")
def matcher():
    from orb_slam2_with_comment_amd.matcher import ORBmatcher
    m = ORBmatcher()
    yield m
    m.close()


def raw_call(matcher, kfs, Scws, mps, in_kf, th=4.0, want_nfused=True, fill=-7, override=None):
    """orbmi_fuse_sim3_search_batch through ctypes with every argument replaceable (override: h, nkf,
    kfs, Scw, mps, in_kf, n_mp, best_idx, best_dist, nfused as raw values).
    -> (rc, best_idx, best_dist, nfused), the arrays pre-filled with `fill`."""
    from orb_slam2_with_comment_amd._capi import lib
    from orb_slam2_with_comment_amd.types import FrameView
    nkf, n = len(kfs), len(mps)
    views = (FrameView * max(nkf, 1))()
    for k in range(nkf):
        views[k] = kfs[k].view()
    S = np.ascontiguousarray([np.asarray(s, F32).reshape(-1, 4)[:3].reshape(12) for s in Scws], F32).reshape(-1, 12)
    mps = np.ascontiguousarray(mps)
    ink = None if in_kf is None else np.ascontiguousarray(in_kf, np.uint8)
    bi, bd = np.full(max(nkf * n, 1), fill, np.int32), np.full(max(nkf * n, 1), fill, np.int32)
    nf = np.full(max(nkf, 1), fill, np.int32)
    a = dict(h=matcher._h, nkf=nkf, kfs=C.addressof(views), Scw=S.ctypes.data if nkf else None,
             mps=mps.ctypes.data if n else None, in_kf=None if ink is None or not ink.size else ink.ctypes.data, n_mp=n,
             best_idx=bi.ctypes.data, best_dist=bd.ctypes.data, nfused=nf.ctypes.data if want_nfused else None)
    a.update(override or {})
    rc = lib().orbmi_fuse_sim3_search_batch(a["h"], a["nkf"], a["kfs"], a["Scw"], a["mps"], a["in_kf"], a["n_mp"], float(th),
                                            a["best_idx"], a["best_dist"], a["nfused"])
    return rc, bi[:nkf * n].reshape(nkf, n), bd[:nkf * n].reshape(nkf, n), nf[:nkf]


# ---- the search, with no tolerance ---------------------------------------------------------------------

@pytest.mark.parametrize("s", [1.0, 1.3])
def test_clause_scene_equals_the_restatement(matcher, s):
    sc = ref.clause_scene(0, s)
    want_i, want_d = ref.fuse_sim3_search(sc["kf"], sc["Scw"], sc["mps"], sc["in_kf"], sc["th"])
    bi, bd, nf = matcher.FuseSim3Search([sc["kf"]], [sc["Scw"]], sc["mps"], sc["in_kf"][None], sc["th"])
    np.testing.assert_array_equal(bi[0], want_i)
    np.testing.assert_array_equal(bd[0], want_d)
    assert nf[0] == (want_i >= 0).sum() >= 250
    # the named differences from the two existing searches, on the device
    perm = sc["perm"]
    assert bi[0][ref.FAR] == perm[ref.FAR]                          # no chi2 gate
    fi, _, _ = matcher.FuseSearch(_with_pose(sc), sc["mps"], sc["in_kf"], sc["th"])
    assert fi[ref.FAR] == -1 and fi[ref.OCT_0] == perm[ref.OCT_0]   # ... which Fuse(KF, MPs) has
    assert bi[0][ref.OCCUPIED] == perm[ref.OCCUPIED]                # no occupancy
    assert bi[0][ref.SHARE_A] == bi[0][ref.SHARE_B] == perm[ref.SHARE_A]
    assert bi[0][ref.TIE] == ref.grid_order_first(sc["kf"], *sc["tie_keys"])
    assert (bi[0][ref.DIST_50], bd[0][ref.DIST_50], bi[0][ref.DIST_51], bd[0][ref.DIST_51]) == (perm[ref.DIST_50], 50, -1, 51)


def _with_pose(sc):
    """The clause scene's keyframe posed at the decomposed Scw, for Fuse(KF, MPs)."""
    from orb_slam2_with_comment_amd.types import Frame
    T, _ = so.decompose_scw(sc["Scw"])
    tcw = np.eye(4, dtype=F32)
    tcw[:3] = T
    kf = sc["kf"]
    return Frame(kf.keys, kf.desc, kf.u_right, tcw, kf.cam)


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 31, 32, 33, 300])
@pytest.mark.parametrize("s", [1.0, 1.3])
def test_point_counts_and_batches_equal_the_restatement(matcher, s, n):
    """n at the edges of a group (8 lanes), a wave (8 points) and a block (32 points); 1, 2 and 3
    keyframes of 600, 1 and 0 keypoints; in_kf NULL and given, a different row per keyframe;
    nfused NULL and given."""
    for nkf in (1, 2, 3):
        kfs, Scws, mps, in_kf = ref.batch_case(nkf, n, s)
        for ink in (None, in_kf):
            want_i, want_d, want_n = ref.fuse_sim3_search_batch(kfs, Scws, mps, ink, 4.0)
            bi, bd, nf = matcher.FuseSim3Search(kfs, Scws, mps, ink, 4.0)
            assert bi.shape == bd.shape == (nkf, n) and nf.shape == (nkf,)
            np.testing.assert_array_equal(bi, want_i)
            np.testing.assert_array_equal(bd, want_d)
            np.testing.assert_array_equal(nf, want_n if n else 0)
            rc, bi2, bd2, nf2 = raw_call(matcher, kfs, Scws, mps, ink, want_nfused=False)
            assert rc == ORBMI_OK and (nf2 == -7).all()
            if n:
                np.testing.assert_array_equal(bi2, want_i)
                np.testing.assert_array_equal(bd2, want_d)
    if n >= 31:
        assert want_n[0] >= 10 and (ink[0] != ink[-1]).any()


def test_overflow_scene_returns_the_first_keypoint_in_grid_order(matcher):
    """130 coincident keypoints of one descriptor: more candidates per point than kCandCap, all at
    distance 0.  Every point gets the first keypoint of the reference's visit order."""
    sc = so.projection_overflow_scene()
    kf = sc["kf"]
    want_i, want_d = ref.fuse_sim3_search(kf, sc["Scw"], sc["mps"], None, 4.0)
    bi, bd, nf = matcher.FuseSim3Search([kf], [sc["Scw"]], sc["mps"], None, 4.0)
    np.testing.assert_array_equal(bi[0], want_i)
    np.testing.assert_array_equal(bd[0], want_d)
    cell = ref._grid(kf)[3]
    first = min(range(len(kf.keys)), key=lambda k: (int(cell[k]), k))
    assert (bi[0] == first).all() and (bd[0] == 0).all() and nf[0] == len(sc["mps"]) == 110


def test_bad_arguments_leave_the_outputs_untouched(matcher):
    import torch
    kfs, Scws, mps, in_kf = ref.batch_case(2, 33)
    S = np.ascontiguousarray([np.asarray(s, F32)[:3].reshape(12) for s in Scws], F32)
    d_scw = torch.from_numpy(S).cuda()
    zero, nan, inf = S.copy(), S.copy(), S.copy()
    zero[1, :3] = 0
    nan[0, 1] = np.nan
    inf[1, 0] = np.inf
    cases = [dict(h=None), dict(nkf=-1), dict(n_mp=-1), dict(kfs=None), dict(Scw=None), dict(mps=None), dict(best_idx=None),
             dict(best_dist=None), dict(Scw=d_scw.data_ptr()), dict(Scw=zero.ctypes.data), dict(Scw=nan.ctypes.data),
             dict(Scw=inf.ctypes.data)]
    for o in cases:
        rc, bi, bd, nf = raw_call(matcher, kfs, Scws, mps, in_kf, override=o)
        assert rc == ORBMI_E_ARG, o
        assert (bi == -7).all() and (bd == -7).all() and (nf == -7).all(), o
    # nothing to do is not an error, and nothing is written
    for o in (dict(nkf=0), dict(n_mp=0), dict(nkf=0, kfs=None, Scw=None), dict(n_mp=0, mps=None, best_idx=None, best_dist=None)):
        rc, bi, bd, nf = raw_call(matcher, kfs, Scws, mps, in_kf, override=o)
        assert rc == ORBMI_OK, o
        assert (bi == -7).all() and (bd == -7).all() and (nf == -7).all(), o
    # the handle still works
    rc, bi, _, _ = raw_call(matcher, kfs, Scws, mps, in_kf)
    assert rc == ORBMI_OK and (bi >= 0).sum() >= 40


def test_two_calls_give_the_same_bytes(matcher):
    kfs, Scws, mps, in_kf = ref.batch_case(3, 300)
    a = matcher.FuseSim3Search(kfs, Scws, mps, in_kf, 4.0)
    b = matcher.FuseSim3Search(kfs, Scws, mps, in_kf, 4.0)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- search_and_fuse and correct_loop over the library ---------------------------------------------------

@pytest.fixture(scope="module")
def backend(matcher):
    from orb_slam2_with_comment_amd.loop import LoopBackend
    be = LoopBackend(matcher=matcher, max_keyframes=32, max_words_total=32 * 2100)
    yield be
    be.db.close()


def test_search_and_fuse_on_the_device_leaves_the_plain_loops_map(backend):
    from orb_slam2_with_comment_amd import loop
    want, _, _ = cpu.plain_fuse_result()
    kfs, corrected, loop_points, _ = cpu.fuse_map()
    counts = loop.search_and_fuse(corrected, loop_points, backend)
    got = cpu.snapshot(kfs, loop_points)
    for key in want:
        assert got[key] == want[key], key
    kfs, corrected, loop_points, _ = cpu.fuse_map()
    assert counts == loop.search_and_fuse(corrected, loop_points, ref.RestatementBackend())
    assert sum(c["researched"] for c in counts) >= 1


def test_correct_loop_on_the_device_equals_the_restatement(oracle, backend):
    """Both backends from the restatement's accepted Sim3.  Exact through the map surgery, the loop
    connections and the edge list; the optimised poses and the corrected points within POSE_TOL, as
    tests/test_essgraph_gpu.py's end-to-end test applies it."""
    import essgraph_reference as eg
    res = cpu.restatement_sim3()
    kfs_w, pts_w, _, want = cpu.restatement_correct_loop()
    kfs_g, pts_g, before, got = cpu.run_correct_loop(res, backend)
    assert got["corrected_points"] == want["corrected_points"] and got["loop_fusion"] == want["loop_fusion"]
    assert got["search_and_fuse"] == want["search_and_fuse"]
    assert got["loop_connections"] == want["loop_connections"]
    sg, sw = cpu.snapshot(kfs_g, pts_g), cpu.snapshot(kfs_w, pts_w)
    for key in sw:
        assert sg[key] == sw[key], key
    eg_g, eg_w = got["essential_graph"], want["essential_graph"]
    for a, b in zip(eg_g["edges"], eg_w["edges"]):
        assert a.tobytes() == b.tobytes()
    assert eg_g["vScw"].tobytes() == eg_w["vScw"].tobytes()
    assert got["graph"]["Tcw"].tobytes() == want["graph"]["Tcw"].tobytes()
    live = np.asarray(got["graph"]["live"], bool)
    ids = np.nonzero(live)[0]
    Tcw = got["graph"]["Tcw"]
    centres = np.array([-(Tcw[i, :3, :3].T @ Tcw[i, :3, 3]) for i in ids])
    extent = float(np.abs(centres - centres.mean(0)).max())
    dev = eg.pose_deviation(eg_g["vertices"][ids], eg_w["vertices"][ids], extent)
    dT = np.abs(eg_g["Tcw"].astype(F64) - eg_w["Tcw"].astype(F64))
    dP = np.abs(eg_g["points"].astype(F64) - eg_w["points"].astype(F64)).max()
    scale = extent + np.abs(eg_w["points"]).max()
    MAXIMA.update(vertices=dev, Tcw_R=dT[:, :3, :3].max(), Tcw_t=dT[:, :3, 3].max(), points=dP)
    print("correct_loop on the device: %d edges, chi2 %.3e -> %.3e (restatement %.3e); max deviation vertices %.2e, "
          "Tcw R %.2e t %.2e, points %.2e (extent %.1f, %d points)" % (
              len(eg_g["edges"][0]), eg_g["chi2_before"], eg_g["chi2_after"], eg_w["chi2_after"], dev, dT[:, :3, :3].max(),
              dT[:, :3, 3].max(), dP, extent, len(eg_g["points"])))
    assert eg_g["chi2_after"] < eg_g["chi2_before"]
    assert dev <= POSE_TOL
    assert dT[:, :3, :3].max() <= 2 * POSE_TOL and dT[:, :3, 3].max() <= POSE_TOL * extent + 1e-6
    assert dP <= POSE_TOL * scale
    dK = max(np.abs(kfs_g[i].tcw.astype(F64) - kfs_w[i].tcw.astype(F64)).max() for i in kfs_w)
    dX = max(np.abs(a.pos.astype(F64) - b.pos.astype(F64)).max() for a, b in zip(pts_g, pts_w) if not b.bad)
    assert dK <= max(2 * POSE_TOL, POSE_TOL * extent + 1e-6) and dX <= POSE_TOL * scale
    assert all(a.bad == b.bad for a, b in zip(pts_g, pts_w))
