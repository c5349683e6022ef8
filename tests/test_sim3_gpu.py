"""GPU parity of the batched Sim3Solver (orbmi_sim3_ransac_batch, src/Sim3Solver.cc) with the
numpy restatement (tests/sim3_reference.py): every hypothesis' T12, T21, s, inlier count and
inlier mask bit for bit, over the Sim3 scene, the shapes where the kernel can go wrong, a ragged
batch and the edge cases; then sim3.Sim3Solver end to end under the ComputeSim3 schedule."""
import numpy as np
import pytest

import sim3_reference as R
from sim3_reference import assert_hypotheses_equal, scene_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ransac():
    from orb_slam2_with_comment_amd.sim3 import Sim3Ransac
    r = Sim3Ransac()
    yield r
    r.close()


def _problem(sc, min_inliers=20, max_iterations=300, triples="scene", seed=0):
    from orb_slam2_with_comment_amd.sim3 import problem
    tri = sc["triples"] if isinstance(triples, str) else triples
    return problem(sc["X1"], sc["X2"], sc["e1"], sc["e2"], sc["k1"], sc["k2"], sc["fix_scale"], 0.99, min_inliers,
                   max_iterations, tri, seed)


def _ref(sc, triples):
    return R.hypotheses(sc["X1"], sc["X2"], sc["e1"], sc["e2"], sc["k1"], sc["k2"], sc["fix_scale"], triples)


@pytest.mark.parametrize("fix", [0, 1])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_hypotheses_match_restatement(ransac, seed, fix):
    """H = 300 hypotheses of the scene at 30 % and 75 % outliers (one batch of two solvers): all
    arrays bit-equal to the restatement."""
    cases = [scene_ref(seed, frac, fix) for frac in (0.3, 0.75)]
    got = ransac([_problem(sc) for sc, _ in cases])
    for g, (sc, ref) in zip(got, cases):
        assert g["iterations"] == 300
        assert_hypotheses_equal(g, ref)
        assert ref["count"].max() > 20


@pytest.mark.parametrize("n", [3, 20, 63, 64, 65, 1000])
def test_shapes_single_hypothesis(ransac, n):
    """H = 1 and N at, below and above the wave size (tail lanes must not set mask bits) and
    N = 1000 (16 mask words).  N == min_inliers gives exactly one iteration."""
    sc = R.sim3_scene(10 + n, 0.3, 0, n=n, ntriples=1)
    g = ransac([_problem(sc, min_inliers=n)])[0]
    assert g["iterations"] == 1 and g["mask"].shape == (1, (n + 63) // 64)
    assert_hypotheses_equal(g, _ref(sc, sc["triples"]))
    if n % 64:
        assert not (g["mask"][:, -1] >> np.uint64(n % 64)).any()


def test_ragged_batch(ransac):
    """Three solvers of different N and iteration counts in one call: N = 65 (300 iterations),
    120 (35) and 3 (1)."""
    a, b, c = R.sim3_scene(20, 0.3, 0, n=65), R.sim3_scene(21, 0.6, 1), R.sim3_scene(22, 0.0, 0, n=3, ntriples=1)
    got = ransac([_problem(a, 12), _problem(b, 60), _problem(c, 3)])
    assert [g["iterations"] for g in got] == [300, 35, 1]
    assert_hypotheses_equal(got[0], _ref(a, a["triples"]))
    assert_hypotheses_equal(got[1], _ref(b, b["triples"][:35]))
    assert_hypotheses_equal(got[2], _ref(c, c["triples"]))


def test_library_sampler_on_null_triples(ransac):
    """triples = NULL: solver k of the batch draws orbmi_sim3_sample_triples(seed, k, ...)."""
    a, b = R.sim3_scene(30, 0.3, 0), R.sim3_scene(31, 0.3, 1, n=40)
    got = ransac([_problem(a, 20, triples=None, seed=11), _problem(b, 20, triples=None, seed=12)])
    assert [g["iterations"] for g in got] == [300, 35]
    assert_hypotheses_equal(got[0], _ref(a, R.sample_triples(11, 0, 120, 300)))
    assert_hypotheses_equal(got[1], _ref(b, R.sample_triples(12, 1, 40, 35)))


def test_edge_cases(ransac):
    from orb_slam2_with_comment_amd._capi import ORBMI_E_ARG, OrbmiError
    sc, _ = scene_ref(0, 0.3, 0)
    # a degenerate triple: count 0 and an all-zero mask, in both scale modes
    for fix in (0, 1):
        d = dict(sc, fix_scale=fix)
        tri = np.array([[5, 5, 5], [1, 2, 3]], np.int32)
        g = ransac([_problem(d, min_inliers=118, triples=tri)])[0]
        assert g["iterations"] == 2
        assert g["count"][0] == 0 and not g["mask"][0].any()
        assert_hypotheses_equal(g, _ref(d, tri))
    # n < min_inliers: 0 iterations, nothing written
    small = R.sim3_scene(1, 0.3, 0, n=12, ntriples=1)
    g = ransac([_problem(small, 20), _problem(sc, 20)])
    assert g[0]["iterations"] == 0 and len(g[0]["count"]) == 0 and g[1]["iterations"] == 300
    assert ransac([_problem(R.sim3_scene(1, 0.3, 0, n=2, ntriples=0), 20, triples=None)])[0]["iterations"] == 0
    # a bad triple index, n < 3 with iterations to run: ORBMI_E_ARG before anything is launched
    for bad in (120, -1):
        tri = sc["triples"].copy()
        tri[299, 2] = bad
        with pytest.raises(OrbmiError) as e:
            ransac([_problem(sc, 20, triples=tri)])
        assert e.value.code == ORBMI_E_ARG
    with pytest.raises(OrbmiError) as e:
        ransac([_problem(R.sim3_scene(1, 0.3, 0, n=2, ntriples=0), 2, triples=None)])
    assert e.value.code == ORBMI_E_ARG
    assert ransac([]) == []


@pytest.mark.parametrize("frac,min_inliers", [(0.3, 20), (0.6, 20), (0.75, 20), (0.3, 60), (0.6, 60), (0.75, 60)])
def test_solver_end_to_end(ransac, frac, min_inliers):
    """Sim3Solver on the GPU under the ComputeSim3 schedule (SetRansacParameters(0.99, min, 300),
    iterate(5) until bNoMore, continuing after a success), four candidates sharing one launch: the
    same return sequence -- which call returns, T12, vbInliers, nInliers, bNoMore -- as the solver
    driven from the restatement's arrays."""
    from orb_slam2_with_comment_amd.sim3 import Sim3Solver, solve_batch
    idx1 = np.arange(0, 240, 2)

    def make(seed):
        sc, hyp = scene_ref(seed, frac, 0)
        s = Sim3Solver.from_arrays(sc["X1"], sc["X2"], sc["e1"], sc["e2"], sc["k1"], sc["k2"], 0, idx1, 240)
        s.SetRansacParameters(0.99, min_inliers, 300)
        s.triples = sc["triples"][:s.mRansacMaxIts]
        return s, hyp

    gpu = [make(seed)[0] for seed in range(4)]
    solve_batch(gpu, ransac)
    successes = 0
    for seed, g in enumerate(gpu):
        c, hyp = make(seed)
        c.set_hypotheses({k: v[:c.mRansacMaxIts] for k, v in hyp.items()})
        for call in range(c.mRansacMaxIts + 2):  # every call runs at least one iteration until bNoMore
            (Tg, bg, vg, ng), (Tc, bc, vc, nc) = g.iterate(5), c.iterate(5)
            assert (Tg is None) == (Tc is None) and bg == bc and ng == nc, (seed, call)
            np.testing.assert_array_equal(vg, vc)
            if Tc is not None:
                successes += 1
                np.testing.assert_array_equal(Tg, Tc)
                assert g.GetEstimatedScale() == c.GetEstimatedScale()
            if bc:
                break
        assert bc
    if min_inliers == 60 and frac >= 0.6:
        assert successes == 0  # at most 48 / 30 points are left in place
    elif min_inliers == 20:
        assert successes >= 4  # every seed's best count is above 20 (test_scene_statistics)


@pytest.mark.parametrize("frac,min_inliers", [(0.3, 20), (0.75, 20), (0.6, 60)])
def test_cpp_dropin_sim3(tmp_path, ransac, frac, min_inliers):
    """orbmi::Sim3Solver from C++ (tests/cpp/dropin_sim3.cpp) under the ComputeSim3 schedule on one
    scene: iterations, the number of iterate(5) calls, success, bNoMore, nInliers, T12, the
    estimated scale / translation / rotation and vbInliers equal to the Python path's."""
    import subprocess
    from orb_slam2_with_comment_amd.sim3 import Sim3Solver
    from test_cpp_dropin import build_dropin
    from sim3_reference import write_problem
    sc, _ = scene_ref(2, frac, 0)
    idx1 = np.arange(0, 240, 2).astype(np.int32)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    write_problem(fin, sc)
    with open(fin, "ab") as f:
        f.write(np.array([240], np.int32).tobytes() + idx1.tobytes())
    exe = build_dropin(str(tmp_path), "dropin_sim3")
    subprocess.run([exe, str(fin), str(fout), str(min_inliers)], check=True, timeout=120)
    raw = fout.read_bytes()
    head = np.frombuffer(raw, np.int32, 5)
    T12 = np.frombuffer(raw, np.float32, 16, 20).reshape(4, 4)
    st = np.frombuffer(raw, np.float32, 13, 84)
    vb = np.frombuffer(raw, np.uint8, 240, 136).astype(bool)
    s = Sim3Solver.from_arrays(sc["X1"], sc["X2"], sc["e1"], sc["e2"], sc["k1"], sc["k2"], 0, idx1, 240)
    s.SetRansacParameters(0.99, min_inliers, 300)
    s.triples = sc["triples"][:s.mRansacMaxIts]
    calls, T, no_more = 0, None, False
    while T is None and not no_more:
        T, no_more, v, n = s.iterate(5, ransac)
        calls += 1
    assert head.tolist() == [s.mRansacMaxIts, calls, int(T is not None), int(no_more), n]
    np.testing.assert_array_equal(vb, v)
    assert (T is not None) == (min_inliers == 20)
    if T is not None:
        np.testing.assert_array_equal(T12, T)
        assert st[0] == np.float32(s.GetEstimatedScale())
        np.testing.assert_array_equal(st[1:4], s.GetEstimatedTranslation())
        np.testing.assert_array_equal(st[4:].reshape(3, 3), s.GetEstimatedRotation())


# ---- SearchBySim3 ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def matcher():
    from orb_slam2_with_comment_amd.matcher import ORBmatcher
    m = ORBmatcher()
    yield m
    m.close()


_SEARCH_REF = {}


def _border_search_scene():
    """scenario.border_scene as both keyframes of SearchBySim3 (one pose, t12 a few millimetres),
    its points in their keypoints' slots: both directions search windows that overlap the borders."""
    from scenario import border_scene
    from orb_slam2_with_comment_amd.types import MAPPOINT_DTYPE
    b = border_scene()
    kf, n = b["kf"], len(b["kf"].keys)
    mps, has = np.zeros(n, MAPPOINT_DTYPE), np.zeros(n, np.uint8)
    mps[b["slot"]], has[b["slot"]] = b["mps"], 1
    return {"kf1": kf, "mps1": mps, "has1": has, "kf2": kf, "mps2": mps, "has2": has, "s12": 1.0,
            "R12": np.eye(3, dtype=np.float32), "t12": np.array([0.002, -0.002, 0.002], np.float32), "th": 7.5,
            "match12": np.full(n, -1, np.int32)}


def _search_ref(f2, s12):
    if (f2, s12) not in _SEARCH_REF:
        sc = _border_search_scene() if f2 == "border" else R.sim3_search_scene(4, f2, s12)
        _SEARCH_REF[f2, s12] = (sc, R.search_by_sim3(sc["kf1"], sc["mps1"], sc["has1"], sc["kf2"], sc["mps2"], sc["has2"],
                                                     sc["s12"], sc["R12"], sc["t12"], sc["th"], sc["match12"]))
    return _SEARCH_REF[f2, s12]


def _gpu_search(matcher, sc, kf2=None):
    return matcher.SearchBySim3(sc["kf1"], sc["mps1"], sc["has1"], kf2 or sc["kf2"], sc["mps2"], sc["has2"], sc["match12"],
                                sc["s12"], sc["R12"], sc["t12"], sc["th"])


@pytest.mark.parametrize("f2,s12", [(6, 1.0), (5, 1.0), (6, 1.1), ("border", 1.0)])
def test_search_by_sim3_matches_restatement(oracle, matcher, f2, s12):
    """orbmi_search_by_sim3 on keyframes 4 and 6 / 5 (and with s12 = 1.1, KF2's map scaled to
    match): vnMatch1, vnMatch2, match12 and nFound exactly the restatement's.  f2 = "border": the
    windows of both directions overlap the four image borders and a corner (the restatement finds
    a point at each)."""
    sc, (vn1, vn2, m12, nfound, _) = _search_ref(f2, s12)
    g12, gn, g1, g2 = _gpu_search(matcher, sc)
    np.testing.assert_array_equal(g1, vn1)
    np.testing.assert_array_equal(g2, vn2)
    np.testing.assert_array_equal(g12, m12)
    if f2 == "border":
        from scenario import assert_every_border_matched, border_scene
        b = border_scene()
        assert gn == nfound
        assert_every_border_matched(b, m12[b["slot"]] == b["slot"])
    else:
        assert gn == nfound >= 100


def test_search_by_sim3_projects_with_kf1_intrinsics(oracle, matcher):
    """Both directions use KF1's fx, fy, cx, cy (src/ORBmatcher.cc:1289-1292): a KF2 view whose fx
    is 5 % off changes nothing."""
    import dataclasses
    from orb_slam2_with_comment_amd.types import Frame
    sc, (vn1, vn2, m12, nfound, _) = _search_ref(6, 1.0)
    k = sc["kf2"]
    off = Frame(k.keys, k.desc, k.u_right, k.tcw, dataclasses.replace(k.cam, fx=k.cam.fx * 1.05))
    g12, gn, g1, g2 = _gpu_search(matcher, sc, off)
    np.testing.assert_array_equal(g1, vn1)
    np.testing.assert_array_equal(g2, vn2)
    np.testing.assert_array_equal(g12, m12)
    assert gn == nfound


def test_search_by_sim3_empty_inputs(oracle, matcher):
    """n = 0 on either side, and keyframes without map points: nFound 0, nothing matched."""
    from orb_slam2_with_comment_amd.types import KP_DTYPE, MAPPOINT_DTYPE, Frame
    sc, _ = _search_ref(6, 1.0)
    empty = Frame(np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8), np.zeros(0, np.float32), sc["kf2"].tcw, sc["kf2"].cam)
    nomp, nohas = np.zeros(0, MAPPOINT_DTYPE), np.zeros(0, np.uint8)
    n1 = len(sc["kf1"].keys)
    m12, n, vn1, vn2 = matcher.SearchBySim3(sc["kf1"], sc["mps1"], sc["has1"], empty, nomp, nohas, sc["match12"], 1.0,
                                            sc["R12"], sc["t12"])
    assert n == 0 and np.array_equal(m12, sc["match12"]) and (vn1 == -1).all() and len(vn2) == 0
    m12, n, vn1, vn2 = matcher.SearchBySim3(empty, nomp, nohas, sc["kf2"], sc["mps2"], sc["has2"], np.zeros(0, np.int32), 1.0,
                                            sc["R12"], sc["t12"])
    assert n == 0 and len(m12) == 0 and len(vn1) == 0 and (vn2 == -1).all()
    none = np.full(n1, -1, np.int32)
    m12, n, vn1, vn2 = matcher.SearchBySim3(sc["kf1"], sc["mps1"], np.zeros(n1, np.uint8), sc["kf2"], sc["mps2"],
                                            np.zeros(len(sc["kf2"].keys), np.uint8), none, 1.0, sc["R12"], sc["t12"])
    assert n == 0 and (m12 == -1).all() and (vn1 == -1).all() and (vn2 == -1).all()


def test_cpp_dropin_search_by_sim3(tmp_path, oracle, matcher):
    """orbmi::ORBmatcher::SearchBySim3 from C++ (tests/cpp/dropin_sim3.cpp search) on the keyframe
    scene: match12 and nFound equal to the Python path's."""
    import subprocess
    from test_cpp_dropin import build_dropin
    sc, _ = _search_ref(6, 1.0)
    d = tmp_path
    v = sc["kf1"].view()
    np.array([v.fx, v.fy, v.cx, v.cy, v.bf, v.mb, v.max_x, v.max_y, v.grid_w_inv, v.grid_h_inv, v.log_scale_factor],
             np.float32).tofile(d / "in_cam.bin")
    sc["kf1"].scale_factors.tofile(d / "in_scale_factors.bin")
    for tag, F in (("kf1", sc["kf1"]), ("kf2", sc["kf2"])):
        F.keys.tofile(d / f"in_{tag}_keys.bin")
        F.desc.tofile(d / f"in_{tag}_desc.bin")
        np.ascontiguousarray(F.u_right, np.float32).tofile(d / f"in_{tag}_ur.bin")
        F.tcw.tofile(d / f"in_{tag}_tcw.bin")
    for k in ("mps1", "mps2", "has1", "has2", "match12"):
        np.ascontiguousarray(sc[k]).tofile(d / f"in_{k}.bin")
    np.concatenate([[sc["s12"]], sc["R12"].ravel(), sc["t12"], [sc["th"]]]).astype(np.float32).tofile(d / "in_sim3.bin")
    exe = build_dropin(str(d), "dropin_sim3")
    subprocess.run([exe, "search", str(d)], check=True, timeout=120)
    g12, gn, _, _ = _gpu_search(matcher, sc)
    np.testing.assert_array_equal(np.fromfile(d / "out_match12.bin", np.int32), g12)
    assert np.fromfile(d / "out_nfound.bin", np.int32).tolist() == [gn] and gn >= 100
