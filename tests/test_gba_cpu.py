"""Global bundle adjustment without a GPU: the numpy restatement (tests/gba_reference.py) anchored
to the C++ oracle, the qualification of every device-parity scene, optimizer.gather_global_ba
clause by clause, and loop.run_global_bundle_adjustment over the restatement backend."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gba_reference as GR  # noqa: E402
import gba_scenes as GS  # noqa: E402
from orb_slam2_with_comment_amd import loop, synth  # noqa: E402
from orb_slam2_with_comment_amd.optimizer import gather_global_ba  # noqa: E402
from orb_slam2_with_comment_amd.system import KeyFrame, MapPoint, pose_inverse  # noqa: E402
from orb_slam2_with_comment_amd.types import KP_DTYPE  # noqa: E402


# ---- the anchor ---------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,free,fixed,npts", [(3, 6, 2, 300), (11, 12, 2, 500)])
def test_restatement_anchored_to_oracle(oracle, seed, free, fixed, npts):
    """On a stereo-only problem BundleAdjustment(robust, 5 iterations) and LocalBundleAdjustment's
    first stage are the same computation (the stereo Huber deltas coincide), so the restatement
    must repeat the C++ oracle stopped at the src/Optimizer.cc:689 check: the same iteration
    count, chi2 within rtol 1e-9, poses and points within 1e-9.  Measured: chi2 1.2e-15, outputs
    bit-equal.  (With the generator's few negative-ur observations left in, which the ABI reads as
    mono, chi2 differs by 1.6e-7: the mono deltas sqrt(5.99) / sqrt(5.991) differ.  gba_scenes.
    anchor_problem drops those edges.)"""
    prob = GS.anchor_problem(seed, free, fixed, npts)
    assert not (prob.edges["ur"] < 0).any()
    n5 = oracle.local_ba(prob)["iterations"][0]
    ref = None
    for k in range(1, 200):
        r = oracle.local_ba(prob, stop_at_check=k)
        if r["iterations"] == (n5, 0):
            ref = r
            break
    assert ref is not None
    g = GR.run(prob, 5, True)
    print("chi2", ref["chi2"][0], g["chi2"], "dT", np.abs(ref["tcw"] - g["tcw"]).max(), "dP", np.abs(ref["pos"] - g["pos"]).max())
    assert g["iterations"] == n5
    np.testing.assert_allclose(g["chi2"], ref["chi2"][0], rtol=1e-9)
    assert np.abs(ref["tcw"] - g["tcw"]).max() <= 1e-9
    assert np.abs(ref["pos"] - g["pos"]).max() <= 1e-9


@pytest.mark.parametrize("name", sorted(GS.CASES))
def test_scene_qualifies(name):
    """A device-parity problem qualifies when the restatement ends by a rule of Levenberg's or by
    its count and is stable under its own variation: a dense LDL^T of S instead of the Cholesky
    gives the same trial sequence and agrees within 1e-7 of the scene's extent.  No seed had to be
    replaced."""
    problem, iterations, robust, a = GS.case(name)
    assert a["iterations"] == iterations or a["status"] & GR.TERMINATE
    assert not a["status"] & GR.SOLVE_FAILED
    b = GR.run(problem, iterations, robust, solver="ldl")
    assert (a["iterations"], a["trials"].tolist(), a["status"]) == (b["iterations"], b["trials"].tolist(), b["status"])
    ext = GS.extent(problem)
    d = max(np.abs(a["pose64"][1] - b["pose64"][1]).max(initial=0.0), np.abs(a["pose64"][0] - b["pose64"][0]).max(initial=0.0),
            np.abs(a["pos64"] - b["pos64"]).max(initial=0.0))
    assert d <= 1e-7 * ext, (d, ext)


def test_restatement_huber_deltas():
    """BundleAdjustment's mono delta is sqrt(5.99), not LocalBA's sqrt(5.991)."""
    problem = GS.case("mono_only")[0]
    g = GR._Graph(problem, True)
    assert (g.delta == np.float64(np.float32(np.sqrt(5.99)))).all()
    g = GR._Graph(GS.case("stereo_only")[0], True)
    assert (g.delta == np.float64(np.float32(np.sqrt(7.815)))).all()


# ---- a small map over system.KeyFrame / system.MapPoint -----------------------------------------
def _map(seed=150, n_kf=6, n_points=80, ids=None):
    """Keyframes in a parent -> child chain and points whose reference keyframe is their first
    observer, from a sliding-window problem."""
    problem = GS.sliding_window_problem(seed=seed, n_kf=n_kf, n_points=n_points)[0]
    ids = list(range(n_kf)) if ids is None else ids
    sf = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
    inv = (np.float32(1.0) / (sf * sf)).astype(np.float32)
    kfs = []
    for k in range(n_kf):
        e = problem.edges[problem.edges["kf"] == k]
        keys = np.zeros(len(e), KP_DTYPE)
        keys["x"], keys["y"] = e["u"], e["v"]
        keys["octave"] = np.rint(np.log(1.0 / e["inv_sigma2"]) / np.log(1.44)).astype(np.int32)
        kfs.append(KeyFrame(ids[k], ids[k], float(k), problem.kfs["tcw"][k].reshape(4, 4).copy(), keys,
                            np.zeros((len(e), 32), np.uint8), e["ur"].copy(), np.zeros(len(e), np.float32), inv, sf,
                            synth.KITTI, [None] * len(e)))
    mps = [MapPoint(1000 + p, problem.pts["pos"][p].copy(), None) for p in range(len(problem.pts))]
    for k, kf in enumerate(kfs):
        for j, ei in enumerate(np.nonzero(problem.edges["kf"] == k)[0]):
            mp = mps[problem.edges["point"][ei]]
            kf.map_points[j] = mp
            mp.observations[kf] = j
            if mp.ref_kf is None:
                mp.ref_kf = kf
    for a, b in zip(kfs[:-1], kfs[1:]):
        b.parent = a
        a.children.append(b)
    return kfs, mps


def _edges_of(problem, kept_kfs, kept_mps):
    return {(kept_mps[e["point"]].id, kept_kfs[e["kf"]].id) for e in problem.edges}


def test_gather_everything():
    kfs, mps = _map()
    problem, kk, mm = gather_global_ba(kfs, mps)
    assert [k.id for k in kk] == [k.id for k in kfs] and [m.id for m in mm] == [m.id for m in mps]
    assert problem.kfs["fixed"].tolist() == [1] + [0] * (len(kfs) - 1)          # fixed = (id == 0)
    assert len(problem.edges) == sum(len(m.observations) for m in mps)
    pt = problem.edges["point"]
    assert (np.diff(pt) >= 0).all()                                              # grouped by point
    for p in np.unique(pt):                                                      # ascending keyframe id within a point
        ids = problem.kfs["id"][problem.edges["kf"][pt == p]]
        assert (np.diff(ids.astype(np.int64)) > 0).all()
    e = problem.edges[0]
    kf, mp = kk[e["kf"]], mm[e["point"]]
    j = mp.observations[kf]
    assert (e["u"], e["v"], e["ur"]) == (kf.keys_un[j]["x"], kf.keys_un[j]["y"], kf.u_right[j])
    assert e["inv_sigma2"] == kf.inv_level_sigma2[kf.keys_un[j]["octave"]]


def test_gather_bad_keyframe_and_its_observations():
    kfs, mps = _map()
    kfs[2].bad = True
    problem, kk, mm = gather_global_ba(kfs, mps)
    assert kfs[2] not in kk and len(problem.kfs) == len(kfs) - 1
    assert all(kid != kfs[2].id for _, kid in _edges_of(problem, kk, mm))
    assert len(problem.edges) == sum(1 for m in mps for k in m.observations if k is not kfs[2])


def test_gather_bad_point():
    kfs, mps = _map()
    mps[3].bad = True
    problem, kk, mm = gather_global_ba(kfs, mps)
    assert mps[3] not in mm and len(problem.pts) == len(mps) - 1
    assert all(pid != mps[3].id for pid, _ in _edges_of(problem, kk, mm))


def test_gather_point_left_without_an_edge():
    """A point seen only by a bad keyframe stays in the arrays; the optimisation reports
    included = 0 and returns its position untouched."""
    kfs, mps = _map()
    lone = MapPoint(5000, np.array([0.3, 0.1, 12.0], np.float32), kfs[2])
    lone.observations[kfs[2]] = 0
    kfs[2].bad = True
    mps = mps[:10] + [lone] + mps[10:]
    problem, kk, mm = gather_global_ba(kfs, mps)
    at = mm.index(lone)
    assert not (problem.edges["point"] == at).any()
    r = GR.run(problem, 3, False)
    assert not r["included"][at] and r["included"].sum() == len(mm) - 1 - sum(
        1 for m in mm if m is not lone and all(k.bad for k in m.observations))
    np.testing.assert_array_equal(r["pos"][at], lone.pos)


def test_gather_ids_with_gaps_in_any_list_order():
    ids = [0, 3, 4, 9, 20, 21]
    kfs, mps = _map(ids=ids)
    shuffled = [kfs[i] for i in (4, 0, 5, 2, 1, 3)]
    problem, kk, mm = gather_global_ba(shuffled, mps)
    assert [k.id for k in kk] == [k.id for k in shuffled]
    assert problem.kfs["fixed"].tolist() == [int(k.id == 0) for k in shuffled]
    pt = problem.edges["point"]
    for p in np.unique(pt):
        got = problem.kfs["id"][problem.edges["kf"][pt == p]].astype(np.int64)
        assert got.tolist() == sorted(k.id for k in mm[p].observations)


# ---- run_global_bundle_adjustment over the restatement ------------------------------------------
LOOP_ID = 7


def _f64(T):
    return np.asarray(T, np.float64).reshape(4, 4)


def test_run_gba_propagates_and_carries():
    """Two keyframes added after the bundle adjustment (a chain: parent -> new1 -> new2) are
    propagated through the spanning tree; a point that only they see is carried through its
    reference keyframe; a point whose reference keyframe the walk does not reach is left alone."""
    kfs, mps = _map(n_kf=8, n_points=120)
    old, new1, new2 = kfs[:6], kfs[6], kfs[7]
    late = [m for m in mps if all(k in (new1, new2) for k in m.observations)]
    assert late, "the scene has points that only the late keyframes see"
    stray_kf = KeyFrame(99, 99, 0.0, np.eye(4, dtype=np.float32), kfs[0].keys_un[:1], None, kfs[0].u_right[:1], None,
                        kfs[0].inv_level_sigma2, kfs[0].scale_factors, synth.KITTI, [None])
    stray = MapPoint(6000, np.array([1.0, 2.0, 30.0], np.float32), stray_kf)
    stray.observations[stray_kf] = 0
    before = {k.id: k.tcw.copy() for k in kfs}
    pos_before = {m.id: m.pos.copy() for m in mps + [stray]}
    out = loop.run_global_bundle_adjustment(old, mps + [stray], [kfs[0]], LOOP_ID, GR.ReferenceBackend())
    assert out["applied"] and out["optimised"] == 6 and out["propagated"] == 2
    assert out["carried"] == len(late) and out["skipped"] == 1
    ba = out["ba"]
    for i, k in enumerate(old):
        np.testing.assert_array_equal(k.tcw, ba["tcw"][i])
        np.testing.assert_array_equal(k.tcw_bef_gba, before[k.id])
        assert k.ba_global_for_kf == LOOP_ID
    # child = (Tchild * Twc_parent) * TcwGBA_parent, the parent's poses as they were / as they are
    exp1 = _f64(before[new1.id]) @ np.linalg.inv(_f64(before[old[-1].id])) @ _f64(old[-1].tcw)
    exp2 = _f64(before[new2.id]) @ np.linalg.inv(_f64(before[new1.id])) @ exp1
    assert np.abs(new1.tcw - exp1).max() <= 1e-5 and np.abs(new2.tcw - exp2).max() <= 1e-5
    np.testing.assert_array_equal(new1.tcw_bef_gba, before[new1.id])
    for m in late:
        ref = m.ref_kf
        Xc = _f64(before[ref.id])[:3, :3] @ pos_before[m.id] + _f64(before[ref.id])[:3, 3]
        Twc = _f64(pose_inverse(ref.tcw))
        assert np.abs(m.pos - (Twc[:3, :3] @ Xc + Twc[:3, 3])).max() <= 1e-4
    np.testing.assert_array_equal(stray.pos, pos_before[stray.id])
    j = ba["map_points"].index(mps[0])
    if ba["included"][j]:
        np.testing.assert_array_equal(mps[0].pos, ba["pos"][j])


def test_run_gba_stop_flag_applies_nothing():
    kfs, mps = _map()
    before = [k.tcw.copy() for k in kfs]
    pos = [m.pos.copy() for m in mps]
    out = loop.run_global_bundle_adjustment(kfs, mps, [kfs[0]], LOOP_ID, GR.ReferenceBackend(), stop_at_check=1)
    assert not out["applied"] and out["ba"]["stop_check"] == 1 and out["ba"]["iterations"] == 1
    for k, T in zip(kfs, before):
        np.testing.assert_array_equal(k.tcw, T)
        assert k.tcw_bef_gba is None
        assert k.tcw_gba is not None      # BundleAdjustment itself writes its estimate back
    for m, X in zip(mps, pos):
        np.testing.assert_array_equal(m.pos, X)


def test_run_gba_loop_kf_zero_writes_poses_directly():
    kfs, mps = _map()
    normals = [None if m.normal is None else m.normal.copy() for m in mps]
    out = loop.run_global_bundle_adjustment(kfs, mps, [kfs[0]], 0, GR.ReferenceBackend())
    ba = out["ba"]
    assert out["applied"] and out["propagated"] == out["carried"] == out["skipped"] == 0
    for i, k in enumerate(kfs):
        np.testing.assert_array_equal(k.tcw, ba["tcw"][i])
        assert k.tcw_gba is None
    for j, m in enumerate(mps):
        if ba["included"][j]:
            np.testing.assert_array_equal(m.pos, ba["pos"][j])
            assert m.pos_gba is None and m.normal is not None and normals[j] is None   # UpdateNormalAndDepth ran
