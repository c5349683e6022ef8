"""The census of the crafted CreateNewMapPoints scenes (tests/tri_scenes.py), on the CPU: two
independent restatements of SearchForTriangulation (the C++ oracle and tests/tri_reference.py)
agree on every scene index for index, every path a scene was built for is reached (non-zero census
entries, the designed winners), every floating-point decision of a search scene clears its
threshold by SEARCH_MARGIN and every geometry match clears tri_oracle's by GEOM_MARGIN -- so
tests/test_tri_edges_gpu.py can compare the kernels exactly, with no exclusion list -- and the
launch plan (orbmi_debug_tri_plan, the functions the launchers call) puts every scene on the
kernel path it names.  For comparison, the natural scenes of test_triangulation_gpu.py score 0
tie-decided matches, 0 epipole rejections and a largest slice of 61.

The host product geometry (orbmi_triangulate_matches, tri_geom.h compiled for the host) is
checked here too: against tri_oracle on every match of `geometry`, and the classifier names every
exit taken."""
import ctypes as C

import numpy as np
import pytest

import tri_reference as R
import tri_scenes as S

SEARCH_MARGIN = 1e-3  # relative, every float decision of a search scene
GEOM_MARGIN = 1e-4    # tri_oracle's relative margin (test_create_points_gpu.py's bar)
X3D_RTOL = 2e-5


def plan(kf1_n, nnodes, npairs, nf):
    from orb_slam2_with_comment_amd._capi import check, lib
    out = np.zeros(3, np.int32)
    check("orbmi_debug_tri_plan", lib().orbmi_debug_tri_plan(kf1_n, nnodes, npairs, nf, out.ctypes.data))
    return [int(v) for v in out]


def run_both(oracle, sc, nb, only_stereo, check_ori):
    kf2, has2, fv2, F12 = sc.nbs[nb]
    om, on = oracle.search_for_triangulation(sc.kf1, sc.has1, sc.fv1, kf2, has2, fv2, F12, only_stereo, check_ori)
    rm, rn, census = R.search_for_triangulation(sc.kf1, sc.has1, sc.fv1, kf2, has2, fv2, F12, only_stereo, check_ori)
    np.testing.assert_array_equal(om, rm, err_msg=f"{sc.name} neighbour {nb}: oracle vs tri_reference")
    assert on == rn == int((rm >= 0).sum())
    assert census["min_margin"] >= SEARCH_MARGIN, (sc.name, nb, census["min_margin"])
    return rm, census


def show(name, census):
    print(f"census {name}: " + ", ".join(f"{k}={v}" for k, v in census.items() if k != "winners"))


def node_paths(sc, nb=0):
    fv2 = sc.nbs[nb][2]
    common = set(int(i) for i in sc.fv1.node_id)
    sizes = [int(fv2.off[k + 1] - fv2.off[k]) for k in range(len(fv2.node_id)) if int(fv2.node_id[k]) in common]
    return {nf: plan(len(sc.kf1.keys), len(sc.fv1.node_id), 1, nf)[1] for nf in sizes}


@pytest.mark.parametrize("name", [f.__name__ for f in S.SEARCH_SCENES])
def test_search_scene_restatements_agree_with_margins(oracle, name):
    """Oracle and tri_reference agree on every neighbour and setting of every scene, with every
    float decision at least SEARCH_MARGIN from its threshold."""
    sc = S.search_scene(name)
    for nb in range(len(sc.nbs)):
        for only_stereo, check_ori in sc.settings:
            _, census = run_both(oracle, sc, nb, only_stereo, check_ori)
            show(f"{name}[{nb}] only_stereo={int(only_stereo)} check_ori={int(check_ori)}", census)


def test_node_sizes_census(oracle):
    sc = S.search_scene("node_sizes")
    m, census = run_both(oracle, sc, 0, False, False)
    assert census["winners"] == sc.designed["winners"]
    # every placed candidate and nothing else lies within TH_LOW: best + worse per KF1 feature
    # (the swept nodes have no free position for a worse one)
    swept = 128 + 256
    assert census["cand_le50"] == 2 * (len(sc.designed["winners"]) - swept) + swept - 1  # the node of 1 has no other
    paths = node_paths(sc)
    assert {nf: paths[nf] for nf in S.NODE_SIZES} == {nf: (0 if nf <= 128 else 1 if nf <= 256 else 2)
                                                      for nf in S.NODE_SIZES}
    pos = {}
    for node, p in census["winners"].values():
        pos.setdefault(node, set()).add(p)
    for k, nf in enumerate(S.NODE_SIZES):
        want = set(range(nf)) if nf in (128, 256) else {p for p in S.NODE_TARGETS + (nf - 1,) if p < nf}
        assert pos[10 + k] == want, (nf, pos[10 + k])
    # every lane and register slot of both tri_node_regs instances wins, and both ends of
    # tri_node_mem's strided loop
    assert {(p & 63, p >> 6) for p in pos[10 + S.NODE_SIZES.index(128)]} == {(l, h) for l in range(64) for h in range(2)}
    assert {(p & 63, p >> 6) for p in pos[10 + S.NODE_SIZES.index(256)]} == {(l, h) for l in range(64) for h in range(4)}
    assert {0, 399} <= pos[10 + S.NODE_SIZES.index(400)]
    assert census["largest_slice"] == 256 and census["multi_pass"] > 0


def test_ties_census(oracle):
    sc = S.search_scene("ties")
    m, census = run_both(oracle, sc, 0, False, False)
    d = sc.designed
    assert census["winners"] == d["winners"]
    assert all(m[i] < 0 for i in d["unmatched"])
    assert census["tie_decided"] == len(d["tied"]) == 12
    assert census["rej_line"] == 6 and census["rej_flag2"] == 3 and census["skip_flag1"] == 3
    assert census["cand_le50"] == 3 * 16  # distance 51 is not one of them
    assert sorted(node_paths(sc).items()) == [(100, 0), (200, 1), (300, 2)]


def test_slices_census(oracle):
    for name, nodes_largest in (("slices_one", 200), ("slices_cap", 1030), ("slices_small", 157)):
        sc = S.search_scene(name)
        m, census = run_both(oracle, sc, 0, False, False)
        assert census["winners"] == sc.designed["winners"]
        assert census["largest_slice"] == nodes_largest
        splits = plan(len(sc.kf1.keys), len(sc.fv1.node_id), 1, 1)[0]
        assert splits == sc.designed["splits"], (name, splits)
    one = S.search_scene("slices_one")
    _, census = run_both(oracle, one, 0, False, False)
    assert census["skip_flag1"] == 1 + 1 + 43 + 64 + 57 and census["nodes_skipped1"] == 20
    small = S.search_scene("slices_small")
    sizes1 = np.diff(small.fv1.off)
    assert sizes1.min() < small.designed["splits"] and sizes1.max() % small.designed["splits"]
    assert len(S.search_scene("slices_cap").kf1.keys) % 64
    # the batch: the slice count changes with the number of pairs, the data does not
    sc = S.search_scene("slices_batch")
    n1, nn = len(sc.kf1.keys), len(sc.fv1.node_id)
    assert (plan(n1, nn, 1, 4)[0], plan(n1, nn, 12, 4)[0]) == sc.designed["splits"]
    _, census = run_both(oracle, sc, 3, False, False)
    assert census["tie_decided"] > 0 and census["rej_flag2"] > 0


def test_gates_census(oracle):
    sc = S.search_scene("gates")
    for only_stereo in (False, True):
        m, census = run_both(oracle, sc, 0, only_stereo, False)
        assert sorted(np.nonzero(m >= 0)[0].tolist()) == sorted(sc.designed["match"][only_stereo])
        assert census["rej_line"] == 4
        if only_stereo:
            assert census["skip_only_stereo1"] == 8 and census["rej_only_stereo2"] == 4 and census["rej_epipole"] == 0
        else:
            assert census["rej_epipole"] == 2  # mono/mono inside the radius, octaves 0 and 3
        m0, c0 = run_both(oracle, sc, 1, only_stereo, False)
        assert (m0 < 0).all() and c0["rej_den0"] > 0 and c0["rej_line"] == 0


def test_merge_census(oracle):
    a, b = S.search_scene("merge_a"), S.search_scene("merge_b")
    for sc, skipped in ((a, (5, 2)), (b, (2, 5))):
        m, census = run_both(oracle, sc, 0, False, False)
        assert census["winners"] == sc.designed["winners"] and len(census["winners"]) == 5
        assert (census["nodes_skipped1"], census["nodes_skipped2"]) == skipped
        m0, c0 = run_both(oracle, sc, 1, False, False)
        assert (m0 < 0).all() and c0["cand_le50"] == 0
    e = S.search_scene("merge_empty1")
    m, census = run_both(oracle, e, 0, False, False)
    assert (m < 0).all() and len(e.fv1.node_id) == 0 and len(e.kf1.keys) == 5


def test_rotation_census(oracle):
    sc = S.search_scene("rotation")
    for nb in range(3):
        m, census = run_both(oracle, sc, nb, False, True)
        assert sorted(np.nonzero(m >= 0)[0].tolist()) == sorted(sc.designed["kept"][nb])
        assert census["rot_removed"] == sc.designed["removed"][nb] > 0
        m_off, _ = run_both(oracle, sc, nb, False, False)
        assert int((m_off >= 0).sum()) == sum(S.ROT_HISTS[nb].values())


def tri_host(K1, K2, idx1, idx2):
    from orb_slam2_with_comment_amd._capi import check, lib
    idx1, idx2 = np.ascontiguousarray(idx1, np.int32), np.ascontiguousarray(idx2, np.int32)
    x = np.zeros((max(len(idx1), 1), 3), np.float32)
    ok = np.zeros(max(len(idx1), 1), np.uint8)
    if len(idx1):
        check("tri", lib().orbmi_triangulate_matches(C.addressof(K1.tri), C.addressof(K2.tri), idx1.ctypes.data,
                                                     idx2.ctypes.data, len(idx1), x.ctypes.data, ok.ctypes.data))
    return ok[:len(idx1)], x[:len(idx1)]


def test_geometry_every_exit_and_margin(oracle):
    """`geometry`: the search pairs every designed match; the classifier names the designed exit
    for each; tri_oracle clears GEOM_MARGIN on each; the host product code gives tri_oracle's flag
    on every match and its points within X3D_RTOL; the two bf matches flip under K2's bf."""
    g = S.geometry()
    K1, K2 = g["K1"], g["K2"]
    assert K1.cam.bf != K2.cam.bf
    m, n = oracle.search_for_triangulation(K1.frame, K1.has, K1.fv, K2.frame, K2.has, K2.fv, g["F12"], False, False)
    rm, rn, census = R.search_for_triangulation(K1.frame, K1.has, K1.fv, K2.frame, K2.has, K2.fv, g["F12"], False,
                                                False)
    np.testing.assert_array_equal(m, rm)
    assert census["min_margin"] >= SEARCH_MARGIN
    idx1 = np.array([d[0] for d in g["designed"]], np.int32)
    idx2 = np.array([d[1] for d in g["designed"]], np.int32)
    np.testing.assert_array_equal(m[idx1], idx2)
    ok_o, x_o, mg = oracle.triangulate_matches(K1.oracle_kf(oracle), K2.oracle_kf(oracle), idx1, idx2)
    ok_p, x_p = tri_host(K1, K2, idx1, idx2)
    taken = {}
    for k, (i1, i2, want) in enumerate(g["designed"]):
        acc, ex, info = R.classify_triangulation(K1, K2, i1, i2)
        print(f"geometry match {k}: designed {want}, classifier {ex}, oracle ok={ok_o[k]} margin={mg[k]:.3g}")
        assert ex == want and acc == bool(ok_o[k]) == want.startswith(("tri_", "unproj")), (k, want, ex, acc, info)
        if ex == "gate1_stereo":
            assert info["right_only"]
        taken[ex] = taken.get(ex, 0) + 1
    print(f"geometry: smallest tri_oracle margin {mg.min():.3g}; exits {taken}")
    assert mg.min() >= GEOM_MARGIN
    reachable = set(R.EXITS) - {"v3_zero", "dist_zero", "no_branch"}
    assert set(taken) == reachable, reachable ^ set(taken)
    np.testing.assert_array_equal(ok_p, ok_o)
    both = ok_o == 1
    scale = np.maximum(1.0, np.linalg.norm(x_o[both].astype(np.float64), axis=1))
    assert (np.abs(x_p[both].astype(np.float64) - x_o[both]).max(axis=1) / scale <= X3D_RTOL).all()
    # the rule of :530 decides these two, one in each direction
    for tag, with_bf1 in (("accepted_by_bf1_only", True), ("accepted_by_bf2_only", False)):
        i1, i2, _ = g["designed"][g["tags"][tag]]
        assert R.classify_triangulation(K1, K2, i1, i2)[0] == with_bf1
        assert R.classify_triangulation(K1, K2, i1, i2, bf2_in_gate2=True)[0] != with_bf1
    for tag in ("inside_below", "inside_above"):
        assert ok_o[g["tags"][tag]] == 1


def claims_expected(oracle, c):
    """The reference's loop on the host: the oracle search with KF1's flags as the earlier pairs
    left them, then orbmi_triangulate_matches -> (match, ok, x3d) rows per pair, and the same
    pairs' matches on the entry flags."""
    K1 = c["K1"]
    npairs, n1 = len(c["nbs"]), K1.n
    has1 = K1.has.copy()
    exp_m = np.full((npairs, n1), -1, np.int32)
    exp_ok = np.zeros((npairs, n1), np.uint8)
    exp_x = np.zeros((npairs, n1, 3), np.float32)
    free = np.full((npairs, n1), -1, np.int32)
    for j, nb in enumerate(c["nbs"]):
        m12, _ = oracle.search_for_triangulation(K1.frame, has1, K1.fv, nb.frame, nb.has, nb.fv, c["F12"][j], False,
                                                 False)
        i1 = np.nonzero(m12 >= 0)[0]
        ok, x = tri_host(K1, nb, i1, m12[i1])
        exp_m[j] = m12
        exp_ok[j, i1], exp_x[j, i1] = ok, x
        free[j], _ = oracle.search_for_triangulation(K1.frame, K1.has, K1.fv, nb.frame, nb.has, nb.fv, c["F12"][j],
                                                     False, False)
        has1[i1[ok == 1]] = 1
    return exp_m, exp_ok, exp_x, free


@pytest.mark.parametrize("npairs", S.CLAIM_NPAIRS)
def test_claims_ownership_as_designed(oracle, npairs):
    c = S.claims(npairs)
    K1 = c["K1"]
    assert K1.n == S.CLAIM_N1 == 70
    exp_m, exp_ok, _, free = claims_expected(oracle, c)
    owner = np.array([np.nonzero(exp_ok[:, i])[0][0] if exp_ok[:, i].any() else -1 for i in range(K1.n)])
    np.testing.assert_array_equal(owner, c["owner"])
    assert (exp_ok.sum(axis=0) <= 1).all()
    want = {0, -1} if npairs == 1 else {0, npairs // 2, npairs - 1, -1}
    assert set(owner.tolist()) == want
    rejected_before = sum(int(((exp_m[j] >= 0) & (exp_ok[j] == 0) & ((owner > j) | (owner < 0))).sum())
                          for j in range(npairs))
    dropped_after = sum(int(((free[j] >= 0) & (exp_m[j] < 0)).sum()) for j in range(npairs))
    print(f"claims npairs={npairs}: owners {np.unique(owner, return_counts=True)}, rejected earlier matches "
          f"{rejected_before}, dropped later matches {dropped_after}")
    assert rejected_before > 0
    assert dropped_after > 0 or npairs == 1
    # every match's geometry is decided clearly, so the device's flags can be compared with
    # tri_oracle's with no exclusion
    k1o = K1.oracle_kf(oracle)
    worst = 1.0
    for j, nb in enumerate(c["nbs"]):
        i1 = np.nonzero(free[j] >= 0)[0]
        ok_o, _, mg = oracle.triangulate_matches(k1o, nb.oracle_kf(oracle), i1, free[j][i1])
        worst = min(worst, float(mg.min()))
        sel = exp_m[j][i1] >= 0
        np.testing.assert_array_equal(exp_ok[j][i1][sel], ok_o[sel])
    print(f"claims npairs={npairs}: smallest tri_oracle margin {worst:.3g}")
    assert worst >= GEOM_MARGIN
    G = plan(K1.n, len(K1.fv.node_id), npairs, 1)[2]
    assert G == (0 if npairs > 64 else next(g for g in (4, 8, 16, 32, 64) if npairs <= g))
    # 70 keypoints: the last wave is partial for G <= 16 (70 is no multiple of 64 / G), and the
    # last workgroup for every G (whole waves past the keyframe for G = 32 and 64)
    assert G == 0 or ((K1.n * G) % 64 if G <= 16 else (K1.n * G) % 256)


def test_plan_thresholds():
    """The three decisions at their boundaries, through the functions the launchers call."""
    assert [plan(100, 4, 1, nf)[1] for nf in (0, 1, 128, 129, 256, 257, 5000)] == [0, 0, 0, 1, 1, 2, 2]
    assert [plan(70, 70, p, 1)[2] for p in (1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 200)] == \
        [4, 4, 8, 8, 16, 16, 32, 32, 64, 64, 0, 0]
    assert plan(2000, 500, 9, 1)[0] == 1 and plan(1030, 1, 1, 1)[0] == 64 and plan(0, 0, 1, 1)[0] == 1
