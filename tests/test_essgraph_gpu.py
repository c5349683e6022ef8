"""GPU parity of the essential-graph optimisation (orbmi_optimize_essential_graph,
orbmi_correct_points_sim3; src/Optimizer.cc:829-1118, src/LoopClosing.cc:546-628) against the numpy
restatement tests/essgraph_reference.py, on the shapes where the kernels can go wrong."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import essgraph_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-4  # q, s, and t relative to the graph's extent: the bar of the fp64 optimisers
ORBMI_E_ARG = -1


@pytest.fixture(scope="module")
def opt():
    from orb_slam2_with_comment_amd.optimizer import EssentialGraphOptimizer
    o = EssentialGraphOptimizer()
    yield o
    o.close()


def run(opt, P, iterations=20):
    return opt.run(P.vertices, P.fixed, P.v0, P.v1, P.meas, P.fix_scale, iterations)


@functools.lru_cache(maxsize=None)
def restated(key):
    P = SHAPES[key]()
    return P, ref.optimize(P.vertices, P.fixed, P.v0, P.v1, P.meas, P.fix_scale)


def star(n_leaves, fixed, seed):
    return ref.synthetic_problem(seed, n_leaves + 1, [(k, 0) if k % 2 else (0, k) for k in range(1, n_leaves + 1)], 1, fixed, 0.01)


def ring_pairs(n):
    return [(i, i - 1) for i in range(1, n)] + [(n - 1, 0)]


SHAPES = {
    "two_vertices": lambda: ref.synthetic_problem(1, 2, [(0, 1)], 1, 1, 0.0),
    "two_vertices_free_scale": lambda: ref.synthetic_problem(2, 2, [(1, 0)], 0, 0, 0.0),
    "hub_65": lambda: star(65, 3, 3),
    "hub_130": lambda: star(130, 130, 4),
    "hub_fixed": lambda: star(65, 0, 5),
    "opposite_pair": lambda: ref.synthetic_problem(6, 5, ring_pairs(5) + [(2, 3), (3, 2)], 1, 0, 0.01),
    "fixed_first": lambda: ref.synthetic_problem(7, 9, ring_pairs(9) + [(0, 4)], 1, 0, 0.01),
    "fixed_middle": lambda: ref.synthetic_problem(7, 9, ring_pairs(9) + [(0, 4)], 1, 4, 0.01),
    "fixed_last": lambda: ref.synthetic_problem(7, 9, ring_pairs(9) + [(0, 4)], 0, 8, 0.01),
    "isolated_vertex": lambda: ref.synthetic_problem(8, 8, [(i, i - 1) for i in range(1, 7)] + [(6, 0)], 1, 2, 0.01),
}

MAXIMA = {}


def compare(opt, P, want, name):
    got = run(opt, P)
    dev = ref.pose_deviation(got["vertices"], want.est, P.extent)
    MAXIMA[name] = dev
    print("%s: device versus restatement max deviation %.2e; device iterations %d trials %s status %d chi2 %.3e -> %.3e; "
          "restatement iterations %d trials %s status %d chi2 %.3e" % (
              name, dev, got["iterations"], got["trials"], got["status"], got["chi2_before"], got["chi2_after"],
              want.iterations, want.trials, want.status, want.chi2_after))
    assert np.isfinite(got["vertices"]).all()
    assert dev <= POSE_TOL
    assert abs(got["chi2_before"] - want.chi2_before) <= 1e-9 * want.chi2_before
    assert got["chi2_after"] <= got["chi2_before"]
    assert got["vertices"][P.fixed].tobytes() == np.asarray(P.vertices[P.fixed], np.float64).tobytes()
    if P.fix_scale:
        assert (got["vertices"][:, 7] == P.vertices[:, 7]).all()  # s comes back exactly as given
    assert 1 <= got["iterations"] <= 20 and all(1 <= t <= 10 for t in got["trials"])
    assert (got["status"] & 1) or got["iterations"] == 20
    return got


@pytest.mark.parametrize("key", sorted(SHAPES))
def test_small_shapes_against_the_restatement(opt, key):
    P, want = restated(key)
    got = compare(opt, P, want, key)
    if key == "isolated_vertex":  # vertex 7 has no edge: bit for bit
        assert got["vertices"][7].tobytes() == P.vertices[7].tobytes()
        assert got["vertices"][0].tobytes() != P.vertices[0].tobytes()
    if key.startswith("two_vertices"):
        assert got["chi2_after"] < 1e-12 * got["chi2_before"]


@pytest.mark.parametrize("spec", ref.PROBLEMS, ids=lambda s: "%s%d_%s" % (s[3], s[1], "fixed" if s[2] else "free"))
def test_committed_problems_against_the_restatement(opt, spec):
    """Rings of 24 in both scale modes, a ring of 66 (more than 64 vertices and edges), a chain of
    257 with one loop edge (fill and the update table)."""
    P, want = ref.problem(spec), ref.solved(spec)
    _, spread = ref.qualifies(spec)
    compare(opt, P, want, str(spec))
    print("    the restatement's own delta 1e-9 versus 1e-8 spread: %.2e" % spread)


@pytest.mark.parametrize("spec", ref.PROBLEMS[:3], ids=lambda s: "%s%d_%s" % (s[3], s[1], "fixed" if s[2] else "free"))
def test_linearisation_at_the_initial_estimates(opt, spec):
    P = ref.problem(spec)
    _, free, H, b, chi = ref.linearisation(spec)
    _, _, H8, b8, _ = ref.linearisation(spec, 1e-8)
    spread_H = np.abs(H - H8).max() / np.abs(H).max()
    spread_b = np.abs(b - b8).max() / np.abs(b).max()
    lin = opt.linearize(P.vertices, P.fixed, P.v0, P.v1, P.meas, P.fix_scale)
    gfree, gH, gb = opt.dense(lin)
    assert (gfree == free).all()
    dH, db = np.abs(gH - H).max() / np.abs(H).max(), np.abs(gb - b).max() / np.abs(b).max()
    print("%s: max|dH|/max|H| %.2e (restatement delta spread %.2e), max|db|/max|b| %.2e (%.2e), chi2 rel %.1e" % (
        spec, dH, spread_H, db, spread_b, abs(lin["chi2"] - chi) / chi))
    assert abs(lin["chi2"] - chi) <= 1e-9 * chi
    assert dH <= 2 * spread_H
    assert db <= 2 * spread_b
    if P.fix_scale:
        assert (gH[6::7, :] == 0).all() and (gH[:, 6::7] == 0).all() and (gb[6::7] == 0).all()
    # fill blocks of the factor's layout stay exactly 0
    pairs = {(min(int(a), int(c)), max(int(a), int(c))) for a, c in zip(P.v0, P.v1)}
    for c, v in enumerate(lin["vert_of"]):
        for a in range(lin["col_ptr"][c], lin["col_ptr"][c + 1]):
            w = int(lin["vert_of"][lin["row_of"][a]])
            if (min(int(v), w), max(int(v), w)) not in pairs:
                assert (lin["Ho"][a] == 0).all()


def test_only_the_fixed_vertex(opt):
    P = ref.synthetic_problem(1, 1, [], 1, 0)
    got = run(opt, P)
    assert got["vertices"].tobytes() == P.vertices.tobytes()
    assert got["iterations"] == 0 and got["trials"] == []


def test_consistent_graph_terminates_by_rule(opt):
    P = ref.synthetic_problem(11, 30, ring_pairs(30) + [(i, i - 2) for i in range(2, 30)], 1, 0, 0.0, start_noise=0.0)
    got = run(opt, P)
    print("consistent graph: chi2 %.3e -> %.3e, iterations %d trials %s status %d" % (
        got["chi2_before"], got["chi2_after"], got["iterations"], got["trials"], got["status"]))
    assert got["chi2_before"] < 1e-20
    assert got["status"] & 1
    assert ref.pose_deviation(got["vertices"], P.vertices, P.extent) <= POSE_TOL


def test_component_not_connected_to_the_fixed_vertex(opt):
    pairs = ring_pairs(6) + [(6 + a, 6 + b) for a, b in ring_pairs(6)]
    P = ref.synthetic_problem(12, 12, pairs, 1, 0, 0.01)
    got = run(opt, P)
    print("floating component: iterations %d trials %s status %d chi2 %.3e -> %.3e" % (
        got["iterations"], got["trials"], got["status"], got["chi2_before"], got["chi2_after"]))
    assert np.isfinite(got["vertices"]).all()
    assert got["status"] & 6  # a solve failed or a trial was rejected, and the status says so
    assert got["iterations"] <= 20 and all(1 <= t <= 10 for t in got["trials"])
    # the estimates are the last accepted ones: their chi2 is the one reported
    chi = float(ref.seq_sum(ref.chi2_of(ref.edge_error(P.meas, got["vertices"][P.v0], got["vertices"][P.v1]))))
    assert abs(chi - got["chi2_after"]) <= 1e-9 * max(chi, 1e-30)
    assert got["chi2_after"] <= got["chi2_before"]


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_input_pose_terminates(opt, bad):
    P = ref.synthetic_problem(13, 10, ring_pairs(10), 1, 0, 0.01)
    guard = np.full((12, 8), 7.25)
    guard[1:11] = P.vertices
    guard[4, 5] = bad
    verts = guard[1:11]  # a view: the call must leave the rows around it alone
    got = opt.run(verts, P.fixed, P.v0, P.v1, P.meas, 1)
    assert (guard[0] == 7.25).all() and (guard[11] == 7.25).all()
    assert got["status"] & 2  # not a success: every solve met a pivot that is not a positive finite number
    assert got["iterations"] <= 20 and all(1 <= t <= 10 for t in got["trials"])
    assert got["vertices"].shape == (10, 8)


def test_bad_arguments_return_before_a_launch(opt):
    import ctypes as C
    from orb_slam2_with_comment_amd._capi import lib
    from orb_slam2_with_comment_amd.optimizer import EssGraphResult
    P = ref.synthetic_problem(14, 6, ring_pairs(6), 1, 0, 0.01)
    h = opt.matcher._h
    out = np.zeros((6, 8))

    def call(vertices=P.vertices, fixed=0, v0=P.v0, v1=P.v1, iterations=20, result=True, handle=h):
        Q, keep = opt._problem(vertices, fixed, v0, v1, P.meas[:len(v0)], 1, iterations)
        R = EssGraphResult()
        R.vertices = out.ctypes.data
        return lib().orbmi_optimize_essential_graph(handle, C.addressof(Q), C.addressof(R) if result else None)
    assert call() == 0
    bad = P.v0.copy()
    bad[2] = 6
    assert call(v0=bad) == ORBMI_E_ARG          # a vertex out of range
    bad[2] = -1
    assert call(v1=bad) == ORBMI_E_ARG
    same = P.v1.copy()
    same[3] = P.v0[3]
    assert call(v1=same) == ORBMI_E_ARG         # v0 == v1
    assert call(fixed=6) == ORBMI_E_ARG         # a missing fixed vertex
    assert call(fixed=-1) == ORBMI_E_ARG
    assert call(iterations=33) == ORBMI_E_ARG
    assert call(result=False) == ORBMI_E_ARG
    assert call(handle=None) == ORBMI_E_ARG
    assert lib().orbmi_optimize_essential_graph(h, None, None) == ORBMI_E_ARG
    # the point correction: a reference outside the tables
    pts, S = np.zeros((2, 3), np.float32), P.vertices[:2].copy()
    f = lib().orbmi_correct_points_sim3
    ref_bad = np.array([0, 2], np.int32)
    o = np.zeros((2, 3), np.float32)
    assert f(h, 2, pts.ctypes.data, ref_bad.ctypes.data, 2, S.ctypes.data, S.ctypes.data, o.ctypes.data, 0, None, None) == ORBMI_E_ARG
    assert f(h, 2, pts.ctypes.data, None, 2, S.ctypes.data, S.ctypes.data, o.ctypes.data, 0, None, None) == ORBMI_E_ARG
    assert f(h, 0, None, None, 0, None, None, None, 0, None, None) == 0


def test_two_calls_give_the_same_bits(opt):
    for P in (ref.problem(ref.PROBLEMS[2]), SHAPES["hub_130"]()):
        a, b = run(opt, P), run(opt, P)
        assert a["vertices"].tobytes() == b["vertices"].tobytes()
        assert (a["chi2_before"], a["chi2_after"], a["iterations"], a["trials"], a["status"]) == (
            b["chi2_before"], b["chi2_after"], b["iterations"], b["trials"], b["status"])
        la = opt.linearize(P.vertices, P.fixed, P.v0, P.v1, P.meas, P.fix_scale)
        lb = opt.linearize(P.vertices, P.fixed, P.v0, P.v1, P.meas, P.fix_scale)
        assert all(np.asarray(la[k]).tobytes() == np.asarray(lb[k]).tobytes() for k in la)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_correct_points_sim3_is_bit_equal(opt, n):
    rng = np.random.default_rng(n)
    Srw = ref.s_exp(np.concatenate([rng.normal(0, 0.5, (5, 3)), rng.normal(0, 4, (5, 3)), np.zeros((5, 1))], 1))
    upd = rng.normal(0, 0.05, (5, 7))
    upd[:2, 6] = 0           # scale 1 and scale != 1
    corrected = ref.s_mul(ref.s_exp(upd), Srw)
    corrected[4] = Srw[4]    # a reference keyframe that was not corrected: its points stay to rounding
    Swr = ref.s_inverse(corrected)
    pts = rng.normal(0, 6, (n, 3)).astype(np.float32)
    refs = rng.integers(0, 5, n).astype(np.int32)
    got_p, got_T = opt.correct_points_sim3(pts, refs, Srw, Swr, corrected)
    want_p, want_T = ref.correct_points(pts, refs, Srw, Swr), ref.sim3_to_tcw(corrected)
    assert got_p.shape == (n, 3) and got_p.tobytes() == want_p.tobytes()
    assert got_T.tobytes() == want_T.tobytes()
    if n:
        still = refs == 4
        assert np.abs(got_p[still] - pts[still]).max(initial=0) < 1e-5
        moved = refs == 2
        assert n < 10 or np.abs(got_p[moved] - pts[moved]).max() > 1e-3


def test_optimize_essential_graph_end_to_end(oracle, opt):
    """From the loop scene of DESIGN.md §6i (keyframes 0 .. 11, the current keyframes re-rendering
    frame 3, the accepted Scw): propagation, the edge list, the optimisation and the correction, on
    the device backend and on the restatement backend."""
    import loop_reference as lref
    from orb_slam2_with_comment_amd import loop, synth
    from orb_slam2_with_comment_amd.loop import LoopBackend
    be = LoopBackend(matcher=opt.matcher, max_keyframes=32, max_words_total=32 * 2100)
    res = lref.run_loop_scene(be)[-1]
    be.db.close()
    assert res["detected"] and res["sim3"]["accepted"]
    sc = lref.loop_scene()
    kfs, covis = sc["keyframes"], sc["covisible"]
    cur, loop_kf = res["current"], res["loop_kf"]
    n_ids = max(kfs) + 1
    live = np.zeros(n_ids, bool)
    live[list(kfs)] = True  # ids with gaps: 12, 13, 14, 16 .. 19 do not live
    Tcw = np.zeros((n_ids, 4, 4), np.float32)
    Tcw[:] = np.eye(4, dtype=np.float32)
    for i, k in kfs.items():
        Tcw[i] = np.asarray(k["kf"].tcw, np.float32).reshape(4, 4)
    # the drift the loop closes: the keyframes since the revisit sit 0.3 m and 0.01 rad off
    D = np.eye(4)
    D[:3, :3] = ref._rot([0.2, 1.0, 0.1], 0.01)
    D[:3, 3] = [0.3, -0.05, 0.1]
    recent = [i for i in kfs if i >= 12]
    for i in recent:
        Tcw[i] = (Tcw[i].astype(np.float64) @ D).astype(np.float32)
    order = sorted(kfs)
    parent = np.full(n_ids, -1, np.int32)
    for a, b in zip(order[1:], order[:-1]):
        parent[a] = b
    cam = synth.KITTI

    def shared(i, j):
        """Map points of keyframe i that project into keyframe j's image: the weight of the pair."""
        mp = kfs[i]["mps"][kfs[i]["has"] == 1]["pos"].astype(np.float64)
        T = np.asarray(kfs[j]["kf"].tcw, np.float64).reshape(4, 4)
        c = mp @ T[:3, :3].T + T[:3, 3]
        z = c[:, 2]
        ok = z > 0.1
        u, v = cam.fx * c[:, 0] / np.where(ok, z, 1) + cam.cx, cam.fy * c[:, 1] / np.where(ok, z, 1) + cam.cy
        return int((ok & (u >= 0) & (u < cam.width) & (v >= 0) & (v < cam.height)).sum())
    covisibles = {i: [j for j in covis[i] if shared(i, j) >= 100] for i in kfs}
    scw = res["sim3"]["scw"]
    Scw = ref.from_rts((np.asarray(scw["sR"], np.float64) / scw["s"])[None], np.asarray(scw["t"])[None], 1.0)[0]
    Scw[7] = np.float64(scw["s"])
    corrected, nonc = loop.propagate_corrected_sim3(Tcw, cur, covis[cur], Scw)
    # LoopConnections: what the corrected keyframes see after the fusion and did not before
    near = [j for j in (loop_kf - 1, loop_kf, loop_kf + 1) if j in kfs]
    lc = {i: {j: shared(i, j) for j in near} for i in corrected if i in lref.SCENE_CURRENT}
    G = {"live": live, "Tcw": Tcw, "parent": parent, "loop_edges": {}, "covisibles": covisibles, "corrected": corrected,
         "noncorrected": nonc, "loop_connections": lc, "loop_id": loop_kf, "cur_id": cur}
    pts, refs = [], []
    for i in (loop_kf, 8, cur, lref.SCENE_RECENT):
        p = kfs[i]["mps"][kfs[i]["has"] == 1]["pos"][:40]
        pts.append(p)
        refs += [i] * len(p)
    pts = np.concatenate(pts).astype(np.float32)
    dev_be = loop.EssGraphBackend(matcher=opt.matcher)
    got = loop.optimize_essential_graph(G, True, pts, refs, backend=dev_be)
    want = loop.optimize_essential_graph(G, True, pts, refs, backend=ref.Backend())
    for a, b in zip(got["edges"], want["edges"]):
        assert a.tobytes() == b.tobytes()
    assert got["vScw"].tobytes() == want["vScw"].tobytes()
    pairs = list(zip(got["edges"][0].tolist(), got["edges"][1].tolist()))
    assert (cur, loop_kf) in pairs and len(pairs) >= len(kfs) - 1
    ids = np.nonzero(live)[0]
    centres = np.array([-(Tcw[i, :3, :3].T @ Tcw[i, :3, 3]) for i in ids])
    extent = float(np.abs(centres - centres.mean(0)).max())
    dev = ref.pose_deviation(got["vertices"][ids], want["vertices"][ids], extent)
    dT = np.abs(got["Tcw"].astype(np.float64) - want["Tcw"].astype(np.float64))
    dP = np.abs(got["points"].astype(np.float64) - want["points"].astype(np.float64)).max()
    print("end to end: %d edges, chi2 %.3e -> %.3e (restatement %.3e), iterations %d trials %s; max deviation %.2e, "
          "Tcw %.2e, points %.2e (extent %.1f)" % (len(pairs), got["chi2_before"], got["chi2_after"], want["chi2_after"],
                                                  got["iterations"], got["trials"], dev, dT.max(), dP, extent))
    assert got["chi2_after"] < got["chi2_before"]
    assert dev <= POSE_TOL
    assert dT[:, :3, :3].max() <= 2 * POSE_TOL and dT[:, :3, 3].max() <= POSE_TOL * extent + 1e-6
    assert dP <= POSE_TOL * (extent + np.abs(pts).max())
    assert (got["Tcw"][~live] == Tcw[~live]).all()
    # the current keyframe ends near its accepted Scw, and the drifted keyframes moved
    assert np.abs(got["Tcw"][cur] - ref.sim3_to_tcw(Scw[None])[0]).max() < 0.05
    assert np.abs(got["Tcw"][cur, :3, 3] - Tcw[cur, :3, 3]).max() > 0.05


def test_zz_report_maxima():
    """The measured maxima of this run, for profiles/essgraph/essgraph_bench.txt and DESIGN.md §6j."""
    for k, v in MAXIMA.items():
        print("max deviation %-40s %.2e" % (k, v))
    assert all(v <= POSE_TOL for v in MAXIMA.values())
