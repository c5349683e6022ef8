"""OptimizeEssentialGraph without a GPU: the numpy restatement's self-checks
(tests/essgraph_reference.py), the host build of csrc/essgraph.h and csrc/essgraph_edges.h against it
bit for bit (tests/cpp/essgraph_check.cpp, once more under the sanitizers), the edge rule case by
case, and loop.optimize_essential_graph over the restatement as its backend."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import essgraph_io as io  # noqa: E402
import essgraph_reference as ref  # noqa: E402

POSE_TOL = 1e-4  # q, s, and t relative to the graph's extent: the bar of the fp64 optimisers


# ---- the restatement's self-checks ----------------------------------------------------------------

def test_log_inverts_exp_in_all_four_branches():
    rng = np.random.default_rng(0)
    u = rng.normal(0, 0.4, (40, 7))
    u[:10, :3] *= 1e-7   # theta < eps
    u[5:15, 6] *= 1e-7   # |sigma| < eps (5..9: both)
    u[20, :] = 0
    S = ref.s_exp(u)
    back = ref.s_log(S)
    assert np.abs(back - u).max() < 1e-9, np.abs(back - u).max()
    # log of a product with the inverse is 0
    assert np.abs(ref.s_log(ref.s_mul(S, ref.s_inverse(S)))).max() < 1e-12


def test_numeric_jacobians_match_a_wider_difference():
    P = ref.problem(ref.PROBLEMS[1])
    a = ref.linearize_edges(P.vertices, P.v0, P.v1, P.meas, 0, 1e-9)
    b = ref.linearize_edges(P.vertices, P.v0, P.v1, P.meas, 0, 1e-6)
    for Ja, Jb in ((a.J0, b.J0), (a.J1, b.J1)):
        assert np.abs(Ja - Jb).max() / np.abs(Jb).max() < 1e-5
    # a common right-multiplication leaves e unchanged, e(S0 G, S1 G) = e(S0, S1), as far as the
    # quaternions are unit: those of g2o::Sim3(Matrix3d, ...) from float poses are to ~1e-7
    G = ref.s_exp(np.array([[0.1, -0.2, 0.05, 1.0, 2.0, -1.0, 0.1]]))
    e0 = ref.edge_error(P.meas, P.vertices[P.v0], P.vertices[P.v1])
    Gn = np.repeat(G, len(P.v0), 0)
    e1 = ref.edge_error(P.meas, ref.s_mul(P.vertices[P.v0], Gn), ref.s_mul(P.vertices[P.v1], Gn))
    assert np.abs(e0 - e1).max() < 1e-5


def test_fix_scale_zeroes_row_and_column_six():
    L, free, H, b, _ = ref.linearisation(ref.PROBLEMS[0])
    assert (H[6::7, :] == 0).all() and (H[:, 6::7] == 0).all() and (b[6::7] == 0).all()
    r = ref.solved(ref.PROBLEMS[0])
    assert (r.est[:, 7] == ref.problem(ref.PROBLEMS[0]).vertices[:, 7]).all()
    _, _, H, b, _ = ref.linearisation(ref.PROBLEMS[1])
    assert (np.diag(H)[6::7] > 0).all() and (b[6::7] != 0).any()


def test_every_committed_problem_qualifies():
    for spec in ref.PROBLEMS:
        ok, spread = ref.qualifies(spec)
        r = ref.solved(spec)
        print(spec, "delta 1e-9 versus 1e-8 spread %.2e" % spread, "iterations", r.iterations, "trials", r.trials, "status",
              r.status, "chi2 %.3e -> %.3e" % (r.chi2_before, r.chi2_after))
        assert ok, (spec, spread)
        assert r.chi2_after < r.chi2_before


def test_optimisation_closes_the_ring():
    """The drift that the loop measurement exposes is spread over the ring: the residual of the
    loop edge falls by orders of magnitude and no keyframe ends far from where it started."""
    for spec in ref.PROBLEMS[:3]:
        P, r = ref.problem(spec), ref.solved(spec)
        assert r.chi2_after < 0.05 * r.chi2_before
        assert ref.pose_deviation(r.est, P.vertices, P.extent) < 0.2


# ---- the host build of the headers against the restatement ---------------------------------------

@pytest.mark.parametrize("spec", ref.PROBLEMS)
def test_host_header_is_bit_equal_at_the_initial_estimates(spec):
    P = ref.problem(spec)
    g = io.run_opt(P)
    L, free, H, b, chi = ref.linearisation(spec)
    assert g["e"].tobytes() == L.e.tobytes()
    assert g["J"].tobytes() == np.stack([L.J0, L.J1], 1).tobytes()
    assert g["rec"][:, 7].tobytes() == L.chi2.tobytes()
    assert g["chi2"][0] == chi
    Hh, bh = io.dense_from_blocks(free, g["vert_of"], g["col_ptr"], g["row_of"], g["Hd"], g["Ho"], g["b"])
    assert Hh.tobytes() == H.tobytes()
    assert bh.tobytes() == b.tobytes()
    # the final estimates: the sparse LDL^T and the dense Cholesky round differently
    r = ref.solved(spec)
    dev = ref.pose_deviation(g["vertices"], r.est, P.extent)
    print(spec, "host header versus restatement: max deviation %.2e;" % dev, g["stdout"].strip(), "| restatement trials", r.trials)
    assert dev <= POSE_TOL
    assert g["chi"][0] == r.chi2_before
    assert abs(g["chi"][1] - r.chi2_after) <= 1e-6 * r.chi2_before
    if P.fix_scale:
        assert (g["vertices"][:, 7] == P.vertices[:, 7]).all()


def test_host_header_under_sanitizers():
    """The stand-alone check program with -fsanitize=address,undefined, on its own."""
    for spec in (ref.PROBLEMS[0], ref.PROBLEMS[1]):
        P = ref.problem(spec)
        g = io.run_opt(P, sanitize=True)
        assert g["iterations"] == io.run_opt(P)["iterations"]
    G = ref.ring_graph(5, 12)
    got = io.run_edges(G, sanitize=True)
    want = ref.essential_graph_edges(G)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))


def test_host_optimiser_handles_the_corner_graphs():
    P = ref.Problem()
    P.vertices, P.fixed, P.fix_scale = ref.problem(ref.PROBLEMS[0]).vertices[:1], 0, 1
    P.v0, P.v1, P.meas = np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 8))
    g = io.run_opt(P)
    assert g["iterations"] == 0 and g["status"] == ref.TERMINATE and g["vertices"].tobytes() == P.vertices.tobytes()
    # two vertices, one edge: the free one moves onto the measurement
    Q = ref.problem(ref.PROBLEMS[0])
    P.vertices, P.fixed = Q.vertices[:2].copy(), 1
    P.v0, P.v1 = np.array([0], np.int32), np.array([1], np.int32)
    P.meas = ref.s_mul(ref.s_exp(np.array([[0.01, 0.02, -0.01, 0.1, 0.0, -0.1, 0.0]])),
                       ref.s_mul(Q.vertices[1:2], ref.s_inverse(Q.vertices[0:1])))
    g = io.run_opt(P)
    r = ref.optimize(P.vertices, P.fixed, P.v0, P.v1, P.meas, 1)
    assert g["chi"][1] < 1e-12 * g["chi"][0]
    assert ref.pose_deviation(g["vertices"], r.est, 1.0) <= POSE_TOL
    assert g["vertices"][1].tobytes() == P.vertices[1].tobytes()


# ---- the edge rule, case by case (src/Optimizer.cc:862-1053) ----------------------------------------

def small_graph(n=8, seed=0, live=None):
    G = ref.ring_graph(seed, n, "chain")
    G["loop_connections"], G["corrected"], G["noncorrected"] = {}, {}, {}
    G["loop_id"], G["cur_id"] = 0, n - 1
    if live is not None:
        G["live"] = np.asarray(live, bool)
    return G


def edges_both_ways(G):
    """The library's host header (through the check program) and the restatement agree exactly."""
    got = io.run_edges(G)
    want = ref.essential_graph_edges(G)
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
    return [(int(a), int(b)) for a, b in zip(got[0], got[1])], got[2], got[3]


def test_edges_spanning_tree_only():
    G = small_graph()
    pairs, meas, vScw = edges_both_ways(G)
    assert pairs == [(i, i - 1) for i in range(1, 8)]
    # Sji = Sjw * Swi
    want = ref.s_mul(vScw[0:1], ref.s_inverse(vScw[1:2]))[0]
    assert meas[0].tobytes() == want.tobytes()


def test_edges_loop_connection_weight_99_and_100():
    G = small_graph()
    G["loop_connections"] = {5: {1: 99, 2: 100}}
    pairs, _, _ = edges_both_ways(G)
    assert (5, 2) in pairs and (5, 1) not in pairs
    assert pairs[0] == (5, 2)  # the loop connections come first


def test_edges_cur_loop_pair_is_exempt_from_the_weight_rule():
    G = small_graph()
    G["loop_connections"] = {7: {0: 3, 1: 3}, 6: {0: 3}}
    pairs, _, _ = edges_both_ways(G)
    assert (7, 0) in pairs and (7, 1) not in pairs and (6, 0) not in pairs
    G["loop_connections"] = {0: {7: 3}}  # only (cur, loop) in that direction is exempt
    pairs, _, _ = edges_both_ways(G)
    assert (0, 7) not in pairs


def test_edges_pair_listed_from_both_sides_gives_two_edges():
    G = small_graph()
    G["loop_connections"] = {5: {2: 150}, 2: {5: 150}}
    pairs, meas, _ = edges_both_ways(G)
    assert pairs[:2] == [(2, 5), (5, 2)]  # ascending id of the key
    # the two measurements are each other's inverse as far as the float poses' quaternions are unit
    assert np.abs(ref.s_log(ref.s_mul(meas[0:1], meas[1:2]))).max() < 1e-5


def test_edges_covisibility_exclusions():
    G = small_graph()
    G["loop_edges"] = {6: [2], 2: [6]}
    G["covisibles"] = {6: [5, 7, 2, 3, 4], 3: [6, 2, 1]}
    pairs, _, _ = edges_both_ways(G)
    of6 = [p for p in pairs if p[0] == 6]
    # parent 5 (once, as the tree edge), loop edge 2 (once, as the loop edge), child 7 and the
    # larger id never; 3 and 4 as covisibility edges in the listed order
    assert of6 == [(6, 5), (6, 2), (6, 3), (6, 4)]
    of3 = [p for p in pairs if p[0] == 3]
    assert of3 == [(3, 2), (3, 1)]  # 6 is the larger id: not emitted from 3; 2 is the parent


def test_edges_loop_edges_emit_from_the_larger_id_only():
    G = small_graph()
    G["loop_edges"] = {6: [2, 1], 2: [6], 1: [6]}
    pairs, _, _ = edges_both_ways(G)
    assert [p for p in pairs if p[0] == 6] == [(6, 5), (6, 1), (6, 2)]  # ascending id
    assert [p for p in pairs if p[0] == 2] == [(2, 1)]


def test_edges_pair_already_inserted_is_skipped():
    G = small_graph()
    G["loop_connections"] = {3: {6: 120}}
    G["covisibles"] = {6: [3, 4]}
    pairs, _, _ = edges_both_ways(G)
    assert pairs.count((6, 3)) == 0 and pairs.count((3, 6)) == 1 and (6, 4) in pairs


def test_edges_noncorrected_sim3_takes_precedence_on_normal_edges():
    G = small_graph()
    rng = np.random.default_rng(3)
    other = {k: ref.s_exp(rng.normal(0, 0.1, (1, 7)))[0] for k in (5, 6)}
    corr = {k: ref.s_exp(rng.normal(0, 0.1, (1, 7)))[0] for k in (5, 6)}
    G["noncorrected"], G["corrected"] = other, corr
    G["loop_connections"] = {6: {0: 500}}
    pairs, meas, vScw = edges_both_ways(G)
    assert vScw[5].tobytes() == corr[5].tobytes() and vScw[6].tobytes() == corr[6].tobytes()
    S = lambda a: np.asarray(a).reshape(1, 8)
    # the loop connection uses vScw (the corrected pose)
    k = pairs.index((6, 0))
    assert meas[k].tobytes() == ref.s_mul(vScw[0:1], ref.s_inverse(S(corr[6])))[0].tobytes()
    # the tree edge 6 -> 5 uses NonCorrectedSim3 at both ends, 5 -> 4 at the near end only
    k = pairs.index((6, 5))
    assert meas[k].tobytes() == ref.s_mul(S(other[5]), ref.s_inverse(S(other[6])))[0].tobytes()
    k = pairs.index((5, 4))
    assert meas[k].tobytes() == ref.s_mul(vScw[4:5], ref.s_inverse(S(other[5])))[0].tobytes()
    k = pairs.index((7, 6))
    assert meas[k].tobytes() == ref.s_mul(S(other[6]), ref.s_inverse(vScw[7:8]))[0].tobytes()


def test_edges_id_gaps_and_ascending_order():
    live = np.ones(10, bool)
    live[[2, 5]] = False
    G = small_graph(10, live=live)
    G["parent"] = np.array([-1, 0, -1, 1, 3, -1, 4, 6, 7, 8], np.int32)
    G["cur_id"] = 9
    G["loop_connections"] = {9: {0: 10}, 4: {1: 200, 0: 300}}
    pairs, _, vScw = edges_both_ways(G)
    assert pairs[:3] == [(4, 0), (4, 1), (9, 0)]
    assert [p for p in pairs[3:]] == [(1, 0), (3, 1), (4, 3), (6, 4), (7, 6), (8, 7), (9, 8)]
    ident = np.array([0, 0, 0, 1, 0, 0, 0, 1.0])
    assert (vScw[2] == ident).all() and (vScw[5] == ident).all()


def test_edges_bad_arguments():
    G = small_graph()
    G["loop_edges"] = {3: [9]}  # out of range
    io.run_edges(G, expect=3)
    live = np.ones(8, bool)
    live[4] = False
    G = small_graph(live=live)  # 5's parent does not live
    io.run_edges(G, expect=3)


# ---- the Python layer over the restatement ---------------------------------------------------------

def test_library_edge_rule_equals_the_restatement():
    """orbmi_essential_graph_edges (host only: no GPU is touched) against the restatement."""
    from orb_slam2_with_comment_amd import loop
    for G in (ref.ring_graph(1, 24), ref.ring_graph(4, 40, "chain")):
        got, want = loop.essential_graph_edges(G), ref.essential_graph_edges(G)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
        again = loop.essential_graph_edges(G, backend=ref.Backend())
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, want))


def test_propagation_gives_the_two_pose_maps():
    from orb_slam2_with_comment_amd import loop
    G = ref.ring_graph(1, 24)
    Scw = G["corrected"][23]
    corrected, nonc = loop.propagate_corrected_sim3(G["Tcw"], 23, [21, 22], Scw)
    want_c, want_n = ref.propagate(G["Tcw"], 23, [21, 22], Scw)
    assert sorted(corrected) == [21, 22, 23] and sorted(nonc) == [21, 22, 23]
    assert all(corrected[k].tobytes() == want_c[k].tobytes() for k in corrected)
    assert all(nonc[k].tobytes() == want_n[k].tobytes() for k in nonc)
    assert corrected[23].tobytes() == np.asarray(Scw).tobytes()
    again, _ = loop.propagate_corrected_sim3(G["Tcw"], 23, [21, 22], Scw, backend=ref.Backend())
    assert all(again[k].tobytes() == want_c[k].tobytes() for k in again)
    # the relative pose of a neighbour to the current keyframe is kept: Siw Swc before = after
    S = lambda a: np.asarray(a).reshape(1, 8)
    before = ref.s_mul(S(nonc[22]), ref.s_inverse(S(nonc[23])))
    after = ref.s_mul(S(corrected[22]), ref.s_inverse(S(corrected[23])))
    assert np.abs(ref.s_log(ref.s_mul(before, ref.s_inverse(after)))).max() < 1e-5


def test_optimize_essential_graph_over_the_restatement():
    from orb_slam2_with_comment_amd import loop
    live = np.ones(14, bool)
    live[[3, 9]] = False  # id gaps
    G = ref.ring_graph(7, 14)
    G["live"] = live
    G["parent"] = np.array([-1, 0, 1, -1, 2, 4, 5, 6, 7, -1, 8, 10, 11, 12], np.int32)
    G["covisibles"] = {i: [j for j in G["covisibles"][i] if live[j]] for i in range(14) if live[i]}
    rng = np.random.default_rng(1)
    pts = rng.normal(0, 5, (30, 3)).astype(np.float32)
    refs = rng.choice(np.nonzero(live)[0], 30)
    out = loop.optimize_essential_graph(G, 1, pts, refs, backend=ref.Backend())
    assert out["chi2_after"] < out["chi2_before"]
    assert (out["Tcw"][~live] == G["Tcw"][~live]).all()
    # the loop keyframe is fixed: its pose comes back as [R | t] of its Sim3, a float rounding away
    assert np.abs(out["Tcw"][0] - G["Tcw"][0]).max() < 1e-6
    # a point moves with its reference keyframe: its coordinates in that camera are kept
    for k in (0, 7, 19):
        i = refs[k]
        cam_before = G["Tcw"][i, :3, :3].astype(np.float64) @ pts[k] + G["Tcw"][i, :3, 3]
        S = out["vertices"][i]
        cam_after = (out["Tcw"][i, :3, :3].astype(np.float64) @ out["points"][k] + out["Tcw"][i, :3, 3]) * S[7]
        if i not in G["corrected"]:
            assert np.abs(cam_before - cam_after).max() < 1e-4
