"""The census of tests/matcher_scenes.py, without a GPU: on every scene the sequential oracle lands
where the scene says it does, so that tests/test_matcher_edges_gpu.py compares the kernels with it on
the path each scene was built for.  The numbers asserted here are conditions on the scenes, not
measurements: a scene that stops reaching its branch fails here."""
import numpy as np
import pytest

import matcher_scenes as S


def oracle_agrees(oracle, sc):
    """the oracle's output is the one the scene's `want` / `rejected` amount to; -> that output"""
    out, n = S.run_oracle(oracle, sc)
    exp, n_exp = S.expected_out(sc)
    np.testing.assert_array_equal(out, exp, err_msg=sc.name)
    assert n == n_exp, sc.name
    return out


def sorted_candidates(sc, q):
    """query q's candidates in the reference's preference order: distance, then visit order"""
    idx = S.candidates(sc, q)
    desc = sc.mps["desc"][q] if sc.mode == 0 else sc.lfp["desc"][q]
    d = np.array([S.hamming(desc, sc.frame.desc[i]) for i in idx])
    order = np.lexsort((S.visit_key(sc.frame, idx), d))
    return idx[order], d[order]


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
def test_depth(oracle, mode, big):
    sc = S.depth(mode, big)
    cases, pos = sc.info["cases"], sc.info["pos"]
    nc = sc.nc
    assert [c[0] for c in cases] == list(nc[pos]) and nc.sum() == nc[pos].sum()
    assert (sc.nq > S.REG_QUERIES and pos[0] < S.REG_QUERIES < pos[-1]) if big else sc.nq <= S.REG_QUERIES
    nc = nc[pos]
    assert set(nc) == set(S.DEPTH_NC) and {0, 3, 4, 148, 149, 150} == {k for c, k in cases if c == 150}
    # each side of every boundary of k_greedy's sources: prefix | top | list | list's second wave step | re-enumeration
    for lo in (S.GREEDY_PRE, S.TOP_K, 64, S.CAND_CAP):
        assert lo in nc and lo + 1 in nc
    oracle_agrees(oracle, sc)
    ties = 0
    for q, (n, k) in zip(pos, cases):
        idx, d = sorted_candidates(sc, q)
        assert sc.occ[idx[:k]].all() and not sc.occ[idx[k:]].any()
        assert sc.want[q] == (idx[k] if k < n else -1)         # the answer sits at depth k of the sorted list
        if k + 1 < n:                                            # and no ratio test stands in its way
            assert sc.frame.keys["octave"][idx[k]] != sc.frame.keys["octave"][idx[k + 1]]
            ties += d[k] == d[k + 1]
        if n >= 64:                                              # all 16 lanes of a group have cells to walk
            assert len(np.unique(S.visit_key(sc.frame, idx) >> 20)) > 16
    assert ties >= 10                                            # answers that win on the visit order alone
    assert sc.frame.u_right[sc.want[sc.want >= 0]].max() > 0 > sc.frame.u_right[sc.want[sc.want >= 0]].min()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("length", [S.CHAIN_SHORT, S.CHAIN_LONG])
def test_chain(oracle, mode, length):
    assert S.CHAIN_SHORT + 1 < S.GREEDY_ROUNDS < S.CHAIN_LONG   # one link per round: either side of the bound
    sc = S.chain(mode, length)
    np.testing.assert_array_equal(sc.nc, [1] + [2] * (length - 1))
    out = oracle_agrees(oracle, sc)
    np.testing.assert_array_equal(out, np.arange(length))       # query i ends on keypoint i
    for q in range(1, length):                                  # its second choice: keypoint i - 1 is nearer
        idx, d = sorted_candidates(sc, q)
        assert list(idx) == [q - 1, q] and list(d) == [10, 20]
    # without query 0 every query keeps its first choice: the chain is a dependency on query 0
    out = oracle_agrees(oracle, S.chain(mode, length, "headless"))
    np.testing.assert_array_equal(out, list(range(1, length)) + [-1])
    # keypoint 0 occupied on entry: query 0 finds nothing, query 1 loses keypoint 0 all the same
    out = oracle_agrees(oracle, S.chain(mode, length, "occupied"))
    np.testing.assert_array_equal(out, [-1] + list(range(1, length)))
    # a query that matches and claims nothing: the two halves differ, its own match is overwritten
    for variant, m in (("noobs", length // 2), ("noobs_late", length - 5)):
        sc = S.chain(mode, length, variant)
        out = oracle_agrees(oracle, sc)
        np.testing.assert_array_equal(out, list(range(m)) + list(range(m + 1, length)) + [-1])
        assert sc.info["mid"] == m and sc.want[m] == sc.want[m + 1] == m
    assert S.CHAIN_LONG - 5 > S.GREEDY_ROUNDS                   # the late one sits behind a fallback-long chain


@pytest.mark.parametrize("variant", ["plain", "noobs", "noobs_late"])
@pytest.mark.parametrize("mode", [0, 1])
def test_chain_past_the_register_path(oracle, mode, variant):
    sc = S.chain(mode, S.CHAIN_LONG, variant, True)
    at = sc.info["at"]
    assert sc.nq > S.REG_QUERIES and at < S.REG_QUERIES < at + S.CHAIN_LONG
    nc = sc.nc
    assert nc.sum() == 2 * S.CHAIN_LONG - 1 and (nc[:at] == 0).all() and (nc[at + S.CHAIN_LONG:] == 0).all()
    out = oracle_agrees(oracle, sc)
    if variant == "plain":
        np.testing.assert_array_equal(out, at + np.arange(S.CHAIN_LONG))
    else:
        assert out[sc.info["mid"]] == at + sc.info["mid"] + 1 and out[S.CHAIN_LONG - 1] == -1


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("nnratio", [0.8, 0.6])
def test_decide(oracle, nnratio, big):
    sc = S.decide(nnratio, big)
    out = oracle_agrees(oracle, sc)
    names, pos = [n for n, _ in sc.info["cases"]], sc.info["pos"]
    assert (sc.nq > S.REG_QUERIES and pos[0] < S.REG_QUERIES < pos[-1]) if big else sc.nq <= S.REG_QUERIES
    for q, (name, ok) in zip(pos, sc.info["cases"]):
        assert ((out == q).sum() == 1) == ok, name
    for a, b in sc.info["pairs"]:
        assert sc.info["cases"][a][1] and not sc.info["cases"][b][1], (names[a], names[b])
    assert sum(n.endswith("_exact") for n in names) >= 1          # d1 == nnratio * d2 in float, accepted
    nc = sc.nc
    assert [nc[pos[names.index(n)]] for n in ("second_real_256_slow_path", "levels_same_slow_path")] == [6, 6]
    idx, d = sorted_candidates(sc, pos[names.index("second_real_256_same_level")])
    assert list(d) == [50, 256] and len(set(sc.frame.keys["octave"][idx])) == 1
    idx, d = sorted_candidates(sc, pos[names.index("best_eq_TH_HIGH")])
    assert list(d) == [S.TH_HIGH]


def test_pairs(oracle):
    sc = S.pairs()
    first = sc.info["first_accept"]
    assert first == S.PAIRS_KP * (S.PAIRS_KP - 1) // 2 and sc.nq <= S.REG_QUERIES
    nc = sc.nc
    assert (nc == S.PAIRS_KP + 4).all() and 64 < nc[0] <= S.CAND_CAP
    out = oracle_agrees(oracle, sc)
    assert (sc.want[:first] == -1).all() and sorted(out[out >= 0]) == list(range(first, sc.nq))
    assert len(set(sc.frame.keys["octave"])) == 1 and not (sc.mps["flags"] & S.MP_HAS_OBS).any()
    for q in list(range(0, first, 97)) + [first - 1]:            # occupied prefix, then A, B, the rest
        idx, d = sorted_candidates(sc, q)
        assert list(d) == [5, 6, 7, 8, 21, 25] + [27] * (S.PAIRS_KP - 2) and sc.occ[idx[:4]].all() and not sc.occ[idx[4:]].any()
        assert d[4] > np.float32(0.8) * np.float32(d[5]) and not d[4] > np.float32(0.8) * np.float32(d[6])
    idx, d = sorted_candidates(sc, first)
    assert list(d) == [4, 5, 6, 7, 20] + [26] * (S.PAIRS_KP - 1) and not d[4] > np.float32(0.8) * np.float32(d[5])


def test_window(oracle):
    sc = S.window()
    out = oracle_agrees(oracle, sc)
    nc = sc.nc
    for q, (name, ok) in enumerate(sc.info["cases"]):
        assert ((out == q).sum() == 1) == ok == (nc[q] == 1), name
    for a, b in sc.info["pairs"]:
        assert sc.info["cases"][a][1] and not sc.info["cases"][b][1]
    x, y, r, ur, minL, maxL, valid = S.windows(sc)
    k = sc.frame.keys
    assert (r[:13] == 4.0).all() and minL[0] == -1
    assert (np.abs(k["x"][:4] - x[:4])[[0, 2]] == r[0]).all() and (np.abs(k["y"][4:8] - y[4:8])[[0, 2]] == r[0]).all()
    q = [n for n, _ in sc.info["cases"]].index("stereo_at_r")
    assert abs(ur[q] - sc.frame.u_right[q]) == r[q]


def test_window_directions(oracle):
    got = {}
    for d in S.WINDOW1_SHIFTS:
        sc = S.window1(d)
        out = oracle_agrees(oracle, sc)
        np.testing.assert_array_equal(sc.nc, sc.want >= 0)
        got[d] = tuple(out >= 0)
    assert len(set(got.values())) == 3                           # the direction flags took effect
    lo0 = [q for q, (lo, o) in enumerate(S.window1("forward").info["cases"]) if lo == 0]
    assert all(got["forward"][q] for q in lo0) and sum(got["backward"][q] for q in lo0) == 1
    mono = oracle_agrees(oracle, S.window1("forward", True))     # bMono switches them off
    assert tuple(mono >= 0) == got["still"]


KEEP = {"tie4": {2, 5, 9}, "20_2_2_1": {7, 3, 11}, "20_2_1": {0, 6}, "20_1": {4}, "7": {8}, "30_3_2": {1, 10}}


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("name", list(S.ROTATIONS))
def test_rotation(oracle, name, big):
    sc = S.rotation(name, big)
    out = oracle_agrees(oracle, sc)
    q = np.nonzero(sc.want >= 0)[0]
    a0, a1 = sc.lf.keys["angle"][q], sc.frame.keys["angle"][sc.want[q]]
    bins = np.array([S.rot_bin(u, v) for u, v in zip(a0, a1)])
    np.testing.assert_array_equal(bins, sc.info["bins"][q])
    counts = np.bincount(bins, minlength=30)
    assert {b: int(c) for b, c in enumerate(counts) if c} == S.ROTATIONS[name]
    assert sc.info["keep"] == KEEP[name] == S.three_maxima(counts)
    np.testing.assert_array_equal(out[sc.want[q]] == -2, ~np.isin(bins, sorted(KEEP[name])))
    d = a0.astype(np.float64) - a1
    if 12 in S.ROTATIONS[name]:
        assert np.isclose(d, 359.9).any()
    if 11 in S.ROTATIONS[name]:
        assert (d[bins == 11] < 0).any()
    if 0 in S.ROTATIONS[name]:
        assert (d[bins == 0] >= 885).any()                       # rounds to bin 30, wraps to 0
    assert (sc.nq > S.REG_QUERIES and q.min() < S.REG_QUERIES < q.max()) if big else sc.nq <= S.REG_QUERIES


@pytest.mark.parametrize("mode", [0, 1])
def test_many_keypoints(oracle, mode):
    sc = S.many_keypoints(mode)
    assert len(sc.frame.keys) == S.MAX_KP
    out = oracle_agrees(oracle, sc)
    nc = sc.nc
    assert set(nc) == {4, 6}
    ng = len(S.MANY_GROUPS)
    for g, (As, B, C, D, octD) in enumerate(S.MANY_GROUPS):
        assert sc.occ[list(As)].all() and out[B] == g            # the contested keypoint goes to the first query
        idx, d = sorted_candidates(sc, ng + g)
        assert set(idx[:len(As)]) == set(As) and list(idx[len(As):]) == [B, C, D] and list(d) == [5] * len(As) + [20, 60, 70]
        assert out[C] == (ng + g if mode == 1 or octD == 0 else -1)
    for group in ([g[1] for g in S.MANY_GROUPS], [g[2] for g in S.MANY_GROUPS], [g[3] for g in S.MANY_GROUPS],
                  [a for g in S.MANY_GROUPS for a in g[0]]):     # contested, runner-up, its second, occupied
        assert any(4096 < i <= 12288 for i in group) and any(i > 12288 for i in group), group
    assert S.MANY_GROUPS[2][1] == S.MAX_KP - 1
    if mode == 0:
        assert (out[[g[2] for g in S.MANY_GROUPS]] >= 0).tolist() == [False, False, False, True, True]


def test_census_file(oracle):
    """profiles/matcher_edges/census.txt is the table of this tree (python tests/matcher_scenes.py
    rewrites it; the MI355X's round counts follow below the mark)"""
    text = S.census_text(oracle)
    assert " NO " not in text
    with open(S.CENSUS) as f:
        old = f.read()
    assert old.split(S.GPU_MARK)[0] == text
