"""GPU parity: Optimizer::BundleAdjustment on MI355X (orbmi_bundle_adjustment) against the numpy
restatement tests/gba_reference.py.  The bars are the project's own for bundle adjustment
(test_lba_gpu.py): poses 1e-4, points 1e-3 relative to max(1, |x|), chi2 rtol 1e-6, and
iterations, trials, stop_check and checks equal."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gba_reference as GR  # noqa: E402
import gba_scenes as GS  # noqa: E402
from orb_slam2_with_comment_amd.types import BAProblem  # noqa: E402

pytestmark = pytest.mark.gpu
POSE_TOL, POINT_TOL, CHI_RTOL = 1e-4, 1e-3, 1e-6


@pytest.fixture(scope="module")
def GBA():
    from orb_slam2_with_comment_amd.optimizer import GlobalBA
    g = GlobalBA()
    yield g
    g.close()


def _compare(r, ref, chi=True):
    assert (r["stop_check"], r["checks"]) == (ref["stop_check"], ref["checks"]), \
        ((r["stop_check"], r["checks"]), (ref["stop_check"], ref["checks"]))
    assert r["iterations"] == ref["iterations"], (r["iterations"], ref["iterations"])
    assert r["trials"].tolist() == ref["trials"].tolist(), (r["trials"], ref["trials"])
    assert r["status"] == ref["status"], (r["status"], ref["status"])
    np.testing.assert_array_equal(r["included"], ref["included"])
    dT = np.abs(r["tcw"] - ref["tcw"]).max(initial=0.0)
    dP = (np.abs(r["pos"] - ref["pos"]) / np.maximum(1.0, np.abs(ref["pos"]))).max(initial=0.0)
    print(f"dT {dT:.3g} dP {dP:.3g} chi2 {r['chi2']!r} / {ref['chi2']!r} initial {r['chi2_initial']!r} / {ref['chi2_initial']!r}")
    assert dT <= POSE_TOL, dT
    assert dP <= POINT_TOL, dP
    if chi:
        np.testing.assert_allclose(r["chi2_initial"], ref["chi2_initial"], rtol=CHI_RTOL)
        np.testing.assert_allclose(r["chi2"], ref["chi2"], rtol=CHI_RTOL)


@pytest.mark.parametrize("name", sorted(GS.CASES))
def test_gba_parity(GBA, name):
    """Every size at which the device takes another path (gba_scenes.CASES): no free pose, below and
    across the MFMA tile, around the panel width, two panels and one pose, the first size LocalBA
    cannot take, ~130 poses with a sparse S; robust on and off, 10 iterations and 1; the shapes."""
    problem, iterations, robust, ref = GS.case(name)
    r = GBA.run(problem, iterations, robust)
    assert r["n_free"] == ref["n_free"]
    _compare(r, ref)
    # what the optimisation does not hold comes back bit for bit
    rank_free = (problem.kfs["fixed"] == 0) & np.isin(np.arange(len(problem.kfs)), problem.edges["kf"])
    np.testing.assert_array_equal(r["tcw"][~rank_free].reshape(-1, 16), problem.kfs["tcw"][~rank_free])
    np.testing.assert_array_equal(r["pos"][~r["included"]], problem.pts["pos"][~r["included"]])
    if name == "edgeless_points":
        assert 0 < (~r["included"]).sum() < len(r["included"])
    if name == "free130":
        fill = r["n_blocks"] / (r["n_free"] * (r["n_free"] + 1) / 2)
        print("block fill of S before elimination:", fill)
        assert fill < 0.5


def test_gba_deterministic(GBA):
    """Two calls give the same 64 bits in every output."""
    problem, iterations, robust, _ = GS.case("free17_robust")
    a, b = GBA.run(problem, iterations, robust), GBA.run(problem, iterations, robust)
    for k in ("tcw", "pos", "included", "trials"):
        np.testing.assert_array_equal(a[k], b[k])
    for k in ("chi2", "chi2_initial"):
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes()
    assert (a["iterations"], a["status"], a["checks"]) == (b["iterations"], b["status"], b["checks"])


def _same_bits(a, b):
    assert set(a) == set(b)
    for k in set(a) - {"phase_ms"}:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
        elif isinstance(a[k], (float, tuple)):
            assert np.asarray(a[k], np.float64).tobytes() == np.asarray(b[k], np.float64).tobytes(), k
        else:
            assert a[k] == b[k], k


def test_both_entries_on_one_handle():
    """Global BA and LocalBA share a handle's device arena (and its stream): a large global problem,
    LocalBA, a small global problem and LocalBA again on one handle give, array for array and bit
    for bit, what each call gives on a fresh handle -- nothing one entry leaves in the arena or in
    the pinned buffers reaches the other."""
    from orb_slam2_with_comment_amd import synth_map as SM
    from orb_slam2_with_comment_amd.optimizer import GlobalBA, LocalBA
    (big, big_it, big_rob), (small, small_it, small_rob) = [(b(), it, rob) for b, it, rob in
                                                            (GS.CASES["free17_robust"], GS.CASES["free3"])]
    local = SM.local_ba_problem(seed=3, n_free=6, n_fixed=2, n_points=300)[0]
    calls = [lambda g: g.run(big, big_it, big_rob), lambda g: LocalBA.run(g, local),
             lambda g: g.run(small, small_it, small_rob), lambda g: LocalBA.run(g, local)]

    def fresh(call):
        g = GlobalBA()
        try:
            return call(g)
        finally:
            g.close()
    want = [fresh(c) for c in calls[:3]]
    want.append(want[1])  # the same LocalBA call
    g = GlobalBA()
    try:
        got = [c(g) for c in calls]
    finally:
        g.close()
    assert want[0]["n_free"] == 17 and want[2]["n_free"] == 3 and want[1]["iterations"][0] > 0
    for a, b in zip(got, want):
        _same_bits(a, b)


def _check_689(oracle, prob):
    """The index of the src/Optimizer.cc:689 check: the first k at which LocalBA's oracle stops
    after the robust optimize(5) alone."""
    n5 = oracle.local_ba(prob)["iterations"][0]
    for k in range(1, 200):
        r = oracle.local_ba(prob, stop_at_check=k)
        if r["iterations"] == (n5, 0):
            return k, r
    raise AssertionError("no such check")


def test_gba_three_way(oracle, GBA):
    """Below 31 poses, stereo only (the Huber deltas coincide): orbmi_bundle_adjustment(robust,
    5 iterations), orbmi_local_bundle_adjustment stopped at the :689 check and the C++ oracle agree."""
    from orb_slam2_with_comment_amd.optimizer import LocalBA
    prob = GS.anchor_problem()
    k, ref = _check_689(oracle, prob)
    g = GBA.run(prob, 5, True)
    L = LocalBA()
    try:
        loc = L.run(prob, stop=C.c_int(0), stop_at_check=k)
    finally:
        L.close()
    assert g["iterations"] == ref["iterations"][0] == loc["iterations"][0]
    for other in (ref, loc):
        assert np.abs(g["tcw"] - other["tcw"]).max() <= POSE_TOL
        assert (np.abs(g["pos"] - other["pos"]) / np.maximum(1.0, np.abs(other["pos"]))).max() <= POINT_TOL
        np.testing.assert_allclose(g["chi2"], other["chi2"][0], rtol=CHI_RTOL)


def test_gba_stop_at_every_check(GBA):
    """The flag raised at every check index of one small run, by index only: stop_check, checks,
    iterations and the write-back match the restatement stopped at the same check."""
    problem, iterations, robust, base = GS.case("free7_robust")
    n = base["checks"]
    try:
        for k in range(n + 1):
            ref = GR.run(problem, iterations, robust, stop_at_check=k)
            r = GBA.run(problem, iterations, robust, stop=C.c_int(0), stop_at_check=k)
            assert r["stop_check"] == (k if k < n else -1)
            _compare(r, ref, chi=ref["iterations"] > 0)
    finally:
        GBA.set_stop_at_check(-1)
    r = GBA.run(problem, iterations, robust, stop=C.c_int(1))  # the caller's flag, raised before the call
    assert (r["stop_check"], r["checks"], r["iterations"]) == (0, 1, 0)


def _run_guarded(GBA, problem, iterations, robust):
    """The C call with its output arrays inside guard bands; -> (result dict, guards intact)."""
    from orb_slam2_with_comment_amd._capi import check, lib
    from orb_slam2_with_comment_amd.types import GBAResultView
    nk, npt, G = len(problem.kfs), len(problem.pts), 64
    tcw = np.full(nk * 16 + 2 * G, 777.0, np.float32)
    pos = np.full(npt * 3 + 2 * G, 777.0, np.float32)
    inc = np.full(npt + 2 * G, 77, np.uint8)
    r = GBAResultView(tcw.ctypes.data + 4 * G, pos.ctypes.data + 4 * G, inc.ctypes.data + G)
    v = problem.view()
    check("orbmi_bundle_adjustment", lib().orbmi_bundle_adjustment(GBA._h, C.addressof(v), iterations, int(robust),
                                                                  C.addressof(r), None))
    intact = all((a[:G] == g).all() and (a[-G:] == g).all() for a, g in ((tcw, 777.0), (pos, 777.0), (inc, 77)))
    return {"tcw": tcw[G:-G].reshape(-1, 16), "pos": pos[G:-G].reshape(-1, 3), "included": inc[G:-G].astype(bool),
            "iterations": r.iterations, "status": r.status, "chi2": r.chi2}, intact


def _finite_or_flagged(r):
    return bool(np.isfinite(r["tcw"]).all() and np.isfinite(r["pos"]).all()) or bool(r["status"] & 2) or bool(r["status"] & 4)


@pytest.mark.parametrize("what", ["nan_pose", "inf_pose", "single_mono_observation", "no_fixed_keyframe"])
def test_gba_terminates(GBA, what):
    """Bounded loops on valid memory: NaN and infinite input poses, a mono point with one
    observation, and a gauge-free problem end, with finite outputs or the status saying so, and
    leave the memory around the output arrays untouched."""
    problem = GS.sliding_window_problem(seed=140, n_kf=8, n_points=250, fixed=() if what == "no_fixed_keyframe" else (0,))[0]
    K, P, E = problem.kfs.copy(), problem.pts, problem.edges.copy()
    if what == "nan_pose":
        K["tcw"][3][5] = np.nan
    elif what == "inf_pose":
        K["tcw"][3][3] = np.inf
    elif what == "single_mono_observation":
        first = np.nonzero(E["point"] == 5)[0]
        E = np.delete(E, first[1:])
        E["ur"][first[0]] = -1.0
    r, intact = _run_guarded(GBA, BAProblem(K, P, E), 10, False)
    assert intact
    assert 0 <= r["iterations"] <= 10
    assert _finite_or_flagged(r), r["status"]
    if what == "no_fixed_keyframe":
        assert np.isfinite(r["tcw"]).all() and np.isfinite(r["pos"]).all()


def test_gba_consistent_problem_stays(GBA):
    """Zero noise: the observations are the projections of the initial estimate (rounded to float),
    so Levenberg ends by a rule of its own and nothing moves beyond rounding."""
    problem = GS.sliding_window_problem(seed=141, n_kf=8, n_points=250, pose_noise=(0, 0), point_noise=0)[0]
    g = GR._Graph(problem, False)
    g.compute_errors()
    E = problem.edges.copy()
    E["u"] -= g.err[:, 0].astype(np.float32)
    E["v"] -= g.err[:, 1].astype(np.float32)
    E["ur"] = np.where(E["ur"] < 0, E["ur"], E["ur"] - g.err[:, 2].astype(np.float32))
    r = GBA.run(BAProblem(problem.kfs, problem.pts, E), 10, False)
    assert r["status"] & 1 and r["iterations"] < 10, (r["status"], r["iterations"])
    assert np.abs(r["tcw"].reshape(-1, 16) - problem.kfs["tcw"]).max() <= 1e-5
    assert np.abs(r["pos"] - problem.pts["pos"]).max() <= 1e-4


def test_gba_argument_checks(GBA):
    """Refused before anything is launched: duplicate (point, keyframe) edges, edges not grouped by
    point, indices out of range (ORBMI_E_ARG); more free poses than the documented cap
    (ORBMI_E_UNSUPPORTED)."""
    from orb_slam2_with_comment_amd._capi import ORBMI_E_ARG, OrbmiError
    from orb_slam2_with_comment_amd.types import BA_EDGE_DTYPE, BA_KF_DTYPE, BA_PT_DTYPE, GBA_MAX_FREE_POSES
    problem = GS.case("free2")[0]
    e = problem.edges

    def code(edges, kfs=problem.kfs, pts=problem.pts, iterations=10):
        with pytest.raises(OrbmiError) as err:
            GBA.run(BAProblem(kfs, pts, edges), iterations)
        return err.value.code

    assert code(np.concatenate([e[:1], e])) == ORBMI_E_ARG
    assert code(np.concatenate([e[5:], e[:5]])) == ORBMI_E_ARG
    for field, value in (("point", len(problem.pts)), ("point", -1), ("kf", len(problem.kfs)), ("kf", -1)):
        bad = e.copy()
        bad[field][len(bad) // 2] = value
        assert code(bad) == ORBMI_E_ARG
    assert code(e, iterations=65) == ORBMI_E_ARG
    n = GBA_MAX_FREE_POSES + 1
    K = np.zeros(n, BA_KF_DTYPE)
    K["tcw"] = np.eye(4, dtype=np.float32).reshape(-1)
    K["id"] = np.arange(n)
    K["fx"] = K["fy"] = 500
    P = np.zeros(n, BA_PT_DTYPE)
    P["pos"][:, 2] = 10
    E = np.zeros(n, BA_EDGE_DTYPE)
    E["point"] = E["kf"] = np.arange(n)
    E["ur"], E["inv_sigma2"] = -1, 1
    assert code(E, K, P) == -4  # ORBMI_E_UNSUPPORTED


def test_run_global_bundle_adjustment_on_the_loop_scene(oracle):
    """End to end: the loop scene after loop.correct_loop (both maps corrected by the restatement's
    operators, so they start equal), then run_global_bundle_adjustment with the device backend and
    with the restatement backend: the same included flags and counts, poses within 1e-4, points
    within 1e-3."""
    import fuse_sim3_reference as fref
    import test_search_and_fuse_cpu as cpu
    from orb_slam2_with_comment_amd import loop
    res = cpu.restatement_sim3()
    outs = []
    be = loop.LoopBackend(max_keyframes=32, max_words_total=32 * 2100)
    try:
        for backend in (be, GR.ReferenceBackend()):
            kfs, points, _, _ = cpu.run_correct_loop(res, fref.RestatementBackend())
            cur = kfs[res["current"]]
            o = loop.run_global_bundle_adjustment(list(kfs.values()), points, [kfs[min(kfs)]], cur.id, backend)
            outs.append((kfs, points, o))
    finally:
        be.close()
    (kg, pg, og), (kw, pw, ow) = outs
    for key in ("applied", "optimised", "propagated", "carried", "skipped"):
        assert og[key] == ow[key], key
    assert og["applied"] and og["optimised"] == len(kg)
    np.testing.assert_array_equal(og["ba"]["included"], ow["ba"]["included"])
    dT = max(np.abs(kg[i].tcw - kw[i].tcw).max() for i in kw)
    dP = max((np.abs(a.pos - b.pos) / np.maximum(1.0, np.abs(b.pos))).max() for a, b in zip(pg, pw) if not b.bad)
    print("loop scene: trials", og["ba"]["trials"], ow["ba"]["trials"], "chi2", og["ba"]["chi2"], ow["ba"]["chi2"], "dT", dT, "dP", dP)
    assert dT <= POSE_TOL and dP <= POINT_TOL
    for i in kw:
        np.testing.assert_array_equal(kg[i].tcw_bef_gba, kw[i].tcw_bef_gba)
