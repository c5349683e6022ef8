"""Loop detection without a GPU: the restatement (tests/loop_reference.py) on hand-written cases,
the host tail header csrc/kfdb_select.h through tests/cpp/loop_check.cpp against it,
LoopDetector's consistency groups on scripted candidate sequences, and SearchByBoW(KF, KF)
restated."""
import functools
import os
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_reference as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---- the restatement on known answers -------------------------------------------------------------

def test_l1_and_l2_scores_known_answers():
    a = ref.BowVector([1, 3], [0.5, 0.5])
    b = ref.BowVector([3, 4], [0.25, 0.75])
    # the only shared word is 3: |0.5 - 0.25| - 0.5 - 0.25 = -0.5, score 0.25
    assert ref.score(ref.L1_NORM, a, b) == 0.25
    assert ref.score(ref.L1_NORM, a, a) == 1.0
    none = ref.score(ref.L1_NORM, a, ref.BowVector([2, 5], [0.5, 0.5]))
    assert none == 0.0 and np.signbit(none)  # -0.0 / 2.0
    h = ref.BowVector([1, 2, 3, 4], [0.5, 0.5, 0.5, 0.5])
    assert ref.score(ref.L2_NORM, h, h) == 1.0  # the sum is 1: the >= 1 branch
    assert ref.score(ref.L2_NORM, h, ref.BowVector([7], [1.0])) == 0.0
    # one shared word, 0.5 * 0.5: 1 - sqrt(0.75)
    assert ref.score(ref.L2_NORM, h, ref.BowVector([2, 9], [0.5, 0.5])) == 1.0 - np.sqrt(0.75)
    assert ref.score(ref.L1_NORM, ref.BowVector([], []), a) == 0.0


def _hand_db():
    """Keyframes 7, 3, 5 (added in that order) share the query's word 10, keyframe 9 (added last)
    shares word 4 as well, keyframe 2 shares nothing, keyframe 8 is stored but never added."""
    db = ref.KeyFrameDatabase()
    q = ([4, 10, 20, 30], [0.25, 0.25, 0.25, 0.25])
    db.store(7, [10, 20, 41], [0.5, 0.25, 0.25])
    db.store(3, [10, 20, 30], [0.25, 0.5, 0.25])
    db.store(5, [10, 42], [0.5, 0.5])
    db.store(9, [4, 10, 20], [0.625, 0.1875, 0.1875])
    db.store(2, [50, 51], [0.5, 0.5])
    db.store(8, [4, 10, 20, 30], [0.25, 0.25, 0.25, 0.25])
    for i in (7, 3, 5, 9, 2):
        db.add(i)
    return db, q


def test_sharing_list_order_is_first_word_then_add_order():
    db, q = _hand_db()
    r = db.query(*q)
    assert r["order"] == [9, 7, 3, 5]  # 9 is met at word 4; then word 10's list in add order
    assert r["common"] == {9: 3, 7: 2, 3: 3, 5: 1}
    assert r["max_common"] == 3 and r["min_common"] == 2  # (int)(3 * 0.8f) = 2
    assert sorted(r["score"]) == [3, 9]  # > 2 is strict: keyframe 7 (2 words) is not scored
    db.erase(3)
    db.add(3)
    assert db.query(*q)["order"] == [9, 7, 5, 3]  # erased and added again: at the back
    assert db.query(*q, connected_ids=[9])["order"] == [7, 5, 3]


def test_detect_loop_candidates_known_answers():
    db, q = _hand_db()
    s = db.query(*q)["score"]
    assert s[3] == 0.75 and s[9] == 0.625  # L1: the sum of min(vi, wi)
    assert db.DetectLoopCandidates(*q, 0.1) == [9, 3]
    assert db.DetectLoopCandidates(*q, 0.7) == [3]
    assert db.DetectLoopCandidates(*q, 0.8) == []
    # 9's best covisible 3 scores higher: 9's entry names 3 with accScore 1.375; 3's own entry
    # (0.75) falls under 0.75 * 1.375
    assert db.DetectLoopCandidates(*q, 0.1, best_covis={9: [3]}) == [3]
    # a neighbour that was not scored in this query (7: too few words; 8: never added) adds nothing
    assert db.DetectLoopCandidates(*q, 0.1, best_covis={9: [7, 8, 2]}) == [9, 3]
    # a connected keyframe is neither a candidate nor a neighbour nor part of max_common
    assert db.DetectLoopCandidates(*q, 0.1, connected_ids=[3], best_covis={9: [3]}) == [9]
    assert db.query(*q, connected_ids=[3, 9])["max_common"] == 2
    assert db.DetectLoopCandidates([60], [1.0], 0.0) == []


@pytest.mark.parametrize("maxc,minc", [(5, 4), (6, 4), (10, 8), (15, 12)])
def test_min_common_words_truncation(maxc, minc):
    """(int)(max * 0.8f): keyframes sitting exactly at the threshold are not scored."""
    db = ref.KeyFrameDatabase()
    qw = list(range(100, 100 + maxc))
    q = (qw, [1.0 / maxc] * maxc)
    db.store(0, qw, q[1])
    for k in (1, 2, 3):  # minc - 1, minc, minc + 1 shared words
        n = minc - 2 + k
        w = qw[:n] + [900 + k]
        db.store(k, w, [1.0 / len(w)] * len(w))
    for k in range(4):
        db.add(k)
    r = db.query(*q)
    assert (r["max_common"], r["min_common"]) == (maxc, minc)
    assert r["common"][2] == minc and sorted(r["score"]) == [0, 3]


# ---- csrc/kfdb_select.h through the stand-alone program ---------------------------------------------

@functools.lru_cache(maxsize=None)
def check_program(sanitize=False):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.fail("no host C++ compiler")
    d = tempfile.mkdtemp(prefix="loop_check_")
    exe = os.path.join(d, "loop_check")
    cmd = [cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "orb_slam2_with_comment_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "loop_check.cpp"), "-o", exe]
    if sanitize:
        cmd[1:1] = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(cmd, check=True)
    return exe


def slot_arrays(case, rq):
    """The per-slot arrays a database query returns, put together from the restatement's per-id
    result: the smallest shared word from a set intersection, add_seq from replaying the ops."""
    qset = {int(w) for w in case["query"][0]}
    seq, counter = {}, 0
    for op, i in case["ops"]:
        if op == "add":
            counter += 1
            seq[i] = counter
    n = len(case["store"])
    a = {"kf_id": np.zeros(n, np.int32), "common": np.zeros(n, np.int32), "first_word": np.full(n, 0xFFFFFFFF, np.uint32),
         "add_seq": np.zeros(n, np.uint64), "score": np.zeros(n, np.float64)}
    for s, (i, w, _) in enumerate(case["store"]):
        a["kf_id"][s] = i
        a["add_seq"][s] = seq.get(i, 0)
        a["common"][s] = rq["common"].get(i, 0)
        a["score"][s] = rq["score"].get(i, 0.0)
        shared = qset & {int(x) for x in w}
        if a["common"][s]:
            assert len(shared) == a["common"][s]
            a["first_word"][s] = min(shared)
    return a


def run_select(case, a, min_common, min_score, sanitize=False):
    exe = check_program(sanitize)
    d = tempfile.mkdtemp(prefix="loop_case_")
    ids = a["kf_id"]
    n_ids = int(ids.max()) + 1 if len(ids) else 0
    slot_of_id = np.full(n_ids, -1, np.int32)
    slot_of_id[ids] = np.arange(len(ids), dtype=np.int32)
    rows = [np.asarray(case["best_covis"].get(i, ()), np.int32) for i in range(n_ids)]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    cov = np.concatenate(rows).astype(np.int32) if n_ids and off[-1] else np.zeros(0, np.int32)
    with open(os.path.join(d, "in.bin"), "wb") as f:
        f.write(struct.pack("<5if", len(ids), min_common, n_ids, n_ids, len(cov), float(min_score)))
        for x in (a["kf_id"], a["common"], a["first_word"], a["add_seq"], a["score"], slot_of_id, off, cov):
            f.write(np.ascontiguousarray(x).tobytes())
    subprocess.run([exe, "select", os.path.join(d, "in.bin"), os.path.join(d, "out.bin")], check=True, capture_output=True)
    o = np.fromfile(os.path.join(d, "out.bin"), np.int32)
    shutil.rmtree(d)
    nc = int(o[0])
    return o[1:1 + nc].tolist(), o[2 + nc:2 + nc + int(o[1 + nc])].tolist()


SELECT_CASES = [(0, 1, 1), (1, 5, 63), (2, 65, 64), (3, 65, 257), (4, 300, 65), (5, 40, 0)]


def _select_case(spec, frac=0.6):
    seed, ndb, nq = spec
    case = ref.database_case(seed, ndb, nq, scoring=seed % 2)
    db = ref.fill(ref.KeyFrameDatabase(case["scoring"]), case)
    rq = db.query(*case["query"], case["connected"])
    ms = ref.min_score_for(case, frac)
    want = db.DetectLoopCandidates(*case["query"], ms, case["connected"], case["best_covis"])
    return case, rq, ms, want


@pytest.mark.parametrize("spec", SELECT_CASES, ids=lambda s: "seed%d-db%d-q%d" % s)
def test_host_tail_equals_the_restatement(spec):
    """kfdb_select.h from per-slot arrays: the list order as ascending (first_word, add_seq) and
    the candidates equal the inverted-file restatement's."""
    for frac in (0.0, 0.6, 2.0):  # minScore below everything, in the middle, above everything
        case, rq, ms, want = _select_case(spec, frac) if frac <= 1 else (*_select_case(spec)[:2], F32(2.0), [])
        got, order = run_select(case, slot_arrays(case, rq), rq["min_common"], ms)
        assert order == rq["order"]
        assert got == want
    if spec[1] >= 65 and spec[2] > 0:
        assert len(rq["order"]) > 20 and len(rq["score"]) > 3 and len(_select_case(spec, 0.0)[3]) >= 1  # not trivial


def test_host_tail_under_sanitizers():
    """The stand-alone program with -fsanitize=address,undefined, on its own."""
    for spec in ((3, 65, 257), (0, 1, 1), (5, 40, 0)):
        case, rq, ms, want = _select_case(spec)
        got, order = run_select(case, slot_arrays(case, rq), rq["min_common"], ms, sanitize=True)
        assert got == want and order == rq["order"]


def test_score_tails_of_the_header():
    sums = np.array([0.0, -0.5, -2.0, -1.2345678901234567, 0.3, 0.9999999999999999, 1.0, 1.0000000000000002, 0.75])
    d = tempfile.mkdtemp(prefix="loop_tail_")
    sums.tofile(os.path.join(d, "in.bin"))
    subprocess.run([check_program(), "tail", os.path.join(d, "in.bin"), os.path.join(d, "out.bin")], check=True)
    out = np.fromfile(os.path.join(d, "out.bin"), np.float64).reshape(2, -1)
    shutil.rmtree(d)
    l1 = -sums / 2.0
    l2 = np.array([1.0 if s >= 1 else 1.0 - np.sqrt(1.0 - s) for s in sums])
    assert out[0].tobytes() == l1.tobytes() and out[1].tobytes() == l2.tobytes()


def test_scalar_inverted_file_of_the_check_program(tmp_path):
    """loop_check's scalar inverted-file DetectLoopCandidates (what tools/loop_bench.py times on
    the host) returns the restatement's candidates."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import loop_bench
    case = loop_bench.bench_case(48, 120, seed=3)
    path = tmp_path / "db.bin"
    loop_bench.write_invfile_case(case, path)
    out = subprocess.run([check_program(), "invfile", str(path), "3"], check=True, capture_output=True, text=True).stdout
    got = [int(x) for x in out.splitlines()[0].split()[1:]]
    db = ref.fill(ref.KeyFrameDatabase(case["scoring"]), case)
    want = db.DetectLoopCandidates(*case["query"], case["min_score"], case["connected"], case["best_covis"])
    assert got == want and len(want) >= 1


# ---- LoopDetector: the consistency groups ---------------------------------------------------------------

class ScriptedDB:
    """A database whose DetectLoopCandidates answers come from a script, by current keyframe."""

    def __init__(self, script, scores=None):
        self.script, self.scores = script, scores or {}
        self.added, self.stored, self.min_scores, self.calls = [], [], [], 0

    def store(self, i, w, v):
        self.stored.append(i)

    def add(self, i):
        self.added.append(i)

    def score(self, w, v, ids):
        return np.array([self.scores.get(i, 0.5) for i in ids], np.float64)

    def DetectLoopCandidates(self, w, v, min_score, connected, best_covis):
        self.min_scores.append(min_score)
        self.calls += 1
        return list(self.script.get(self.cur, []))


def _detector(script, scores=None, covis=None, bad=None):
    from orb_slam2_with_comment_amd.loop import LoopDetector
    db = ScriptedDB(script, scores)
    covis = covis or {}
    det = LoopDetector(db, covis, covis, covis, isBad=bad)

    def step(i):
        det.InsertKeyFrame(i, [1], [1.0])
        db.cur = i
        return det.DetectLoop()
    return det, db, step


def test_consistency_reaches_three_on_the_fourth_query():
    # chain covisibility among the old keyframes 0..5: a candidate's group is itself + neighbours
    covis = {i: [j for j in (i - 1, i + 1) if 0 <= j <= 5] for i in range(6)}
    det, db, step = _detector({20: [2], 21: [3], 22: [2], 23: [3]}, covis=covis)
    assert [step(i) for i in (20, 21, 22)] == [False, False, False]  # consistency 0, 1, 2
    assert [n for _, n in det.mvConsistentGroups] == [2]
    assert step(23) and det.mvpEnoughConsistentCandidates == [3]  # the one that reaches 3
    assert db.added == [20, 21, 22, 23]  # the add happens on every path


def test_query_without_candidates_clears_the_groups():
    covis = {i: [j for j in (i - 1, i + 1) if 0 <= j <= 5] for i in range(6)}
    det, db, step = _detector({20: [2], 21: [2], 22: [], 23: [2], 24: [2]}, covis=covis)
    step(20), step(21)
    assert [n for _, n in det.mvConsistentGroups] == [1]
    assert not step(22) and det.mvConsistentGroups == []
    assert not step(23) and not step(24)
    assert [n for _, n in det.mvConsistentGroups] == [1] and db.added == [20, 21, 22, 23, 24]


def test_one_previous_group_is_counted_once_per_query():
    """Two candidates consistent with the same previous group: the group is carried once
    (vbConsistentGroup), with the first candidate's members; both candidates may still become
    enough-consistent."""
    covis = {i: [j for j in (i - 1, i + 1) if 0 <= j <= 5] for i in range(6)}
    det, db, step = _detector({20: [2], 21: [2, 3], 22: [2, 3], 23: [2, 3]}, covis=covis)
    step(20)
    step(21)
    assert [(sorted(g), n) for g, n in det.mvConsistentGroups] == [([1, 2, 3], 1)]
    step(22)
    assert [(sorted(g), n) for g, n in det.mvConsistentGroups] == [([1, 2, 3], 2)]
    assert step(23) and det.mvpEnoughConsistentCandidates == [2, 3]
    # an unrelated candidate starts a group of its own at 0
    det2, _, step2 = _detector({20: [0], 21: [0, 5]}, covis=covis)
    step2(20), step2(21)
    assert [(sorted(g), n) for g, n in det2.mvConsistentGroups] == [([0, 1], 1), ([4, 5], 0)]


def test_early_add_before_last_loop_plus_ten():
    det, db, step = _detector({5: [1], 12: [1]})
    assert not step(5) and db.calls == 0 and db.added == [5]  # mnId < mLastLoopKFid + 10
    det.mLastLoopKFid = 3
    assert not step(12) and db.calls == 0 and db.added == [5, 12]  # 12 < 13
    assert not step(13) and db.calls == 1 and db.added == [5, 12, 13]
    det.InsertKeyFrame(0, [1], [1.0])  # keyframe 0 is stored (DetectLoop scores it) but never queued
    assert 0 in db.stored and not det.CheckNewKeyFrames()


def test_min_score_over_the_covisibles_that_are_not_bad():
    covis = {30: [1, 2, 3], 31: []}
    det, db, step = _detector({}, scores={1: 0.4, 2: 0.1, 3: 0.25}, covis=covis, bad={2: True})
    step(30)
    assert db.min_scores == [F32(0.25)]  # 2 is bad
    step(31)
    assert db.min_scores[1] == F32(1)  # no covisibles: minScore stays 1


# ---- SearchByBoW(KF, KF) restated ------------------------------------------------------------------

def _masks(kf1, kf2, seed=1):
    rng = np.random.default_rng(seed)
    return (rng.random(len(kf1.keys)) < 0.85).astype(np.uint8), (rng.random(len(kf2.keys)) < 0.85).astype(np.uint8)


def test_search_by_bow_kf_restated_finds_the_true_pairs():
    kf1, fv1, kf2, fv2, perm = ref.bow_pair(0)
    ok1, ok2 = _masks(kf1, kf2)
    for ori in (False, True):
        m, n = ref.search_by_bow_kf(kf1, ok1, fv1, kf2, ok2, fv2, 0.75, ori)
        assert n == int((m >= 0).sum()) >= 40
        hit = m >= 0
        assert (m[hit] == perm[hit]).all()          # 12 flipped bits of 256: only the true pair is near
        assert ok1[hit].all() and ok2[m[hit]].all()  # both sides hold a live point
        assert len(set(m[hit].tolist())) == n       # vbMatched2: a KF2 keypoint is taken once
    m0, _ = ref.search_by_bow_kf(kf1, ok1, fv1, kf2, ok2, fv2, 0.75, False)
    m1, n1 = ref.search_by_bow_kf(kf1, ok1, fv1, kf2, ok2, fv2, 0.75, True)
    assert 0 < n1 < int((m0 >= 0).sum())            # the histogram removes the angle outliers
    z1, z2 = np.zeros_like(ok1), np.zeros_like(ok2)
    assert ref.search_by_bow_kf(kf1, z1, fv1, kf2, ok2, fv2)[1] == 0
    assert ref.search_by_bow_kf(kf1, ok1, fv1, kf2, z2, fv2)[1] == 0


def th_low_pair(dist):
    """One feature per side in one node, `dist` bits apart."""
    from orb_slam2_with_comment_amd import synth
    from orb_slam2_with_comment_amd.types import KP_DTYPE, FeatureVector, Frame
    d1 = np.zeros((1, 32), np.uint8)
    bits = np.zeros(256, np.uint8)
    bits[:dist] = 1
    d2 = np.packbits(bits).reshape(1, 32)
    k = np.zeros(1, KP_DTYPE)
    fv = FeatureVector(np.array([5]))
    return Frame(k, d1, None, None, synth.KITTI), fv, Frame(k.copy(), d2, None, None, synth.KITTI), FeatureVector(np.array([5]))


def test_search_by_bow_kf_th_low_is_strict():
    one = np.ones(1, np.uint8)
    for dist, want in ((49, 0), (50, -1), (51, -1)):
        kf1, fv1, kf2, fv2 = th_low_pair(dist)
        m, n = ref.search_by_bow_kf(kf1, one, fv1, kf2, one, fv2, 0.75, True)
        assert m.tolist() == [want] and n == (want >= 0)


def test_search_by_bow_kf_first_feature_wins_ties():
    from orb_slam2_with_comment_amd import synth
    from orb_slam2_with_comment_amd.types import KP_DTYPE, FeatureVector, Frame
    d1 = np.zeros((1, 32), np.uint8)
    d2 = np.zeros((3, 32), np.uint8)
    d2[0, 0], d2[1, 0], d2[2, 0] = 0x0F, 0x03, 0x30  # distances 4, 2, 2: the first at 2 is slot 1
    kf1 = Frame(np.zeros(1, KP_DTYPE), d1, None, None, synth.KITTI)
    kf2 = Frame(np.zeros(3, KP_DTYPE), d2, None, None, synth.KITTI)
    fv1, fv2 = FeatureVector(np.array([5])), FeatureVector(np.array([5, 5, 5]))
    m, n = ref.search_by_bow_kf(kf1, np.ones(1, np.uint8), fv1, kf2, np.ones(3, np.uint8), fv2, 0.75, False)
    assert n == 0  # 2 < 0.75 * 2 fails: the tie is also the second best
    m, n = ref.search_by_bow_kf(kf1, np.ones(1, np.uint8), fv1, kf2, np.ones(3, np.uint8), fv2, 1.01, False)
    assert m.tolist() == [1]


# ---- the end-to-end scene over the restatements (what the GPU case is compared with) ----------------------

def test_scene_restatement_names_the_revisited_keyframe(oracle):
    """The property of the scene, on the restatement alone: with the first vocabulary shape tried
    (loop_reference.SCENE_VOCAB) every query of a re-render of frame 3's pose names keyframe 3 or a
    direct neighbour, the fourth consecutive query reaches consistency 3, SearchByBoW(KF, KF) keeps
    at least 20 matches and compute_sim3 accepts the loop."""
    res = ref.run_loop_scene(ref.RestatementLoopBackend())
    near = {ref.SCENE_REVISITED - 1, ref.SCENE_REVISITED, ref.SCENE_REVISITED + 1}
    print([(r["current"], r["candidates"], r["consistent"]) for r in res])
    assert [r["detected"] for r in res] == [False, False, False, True]
    assert all(near & set(r["candidates"]) for r in res)
    last = res[-1]
    assert last["loop_kf"] in near and int((last["bow_matches"][0] >= 0).sum()) >= 20
    assert last["sim3"]["accepted"] and last["sim3"]["n_total"] >= 40
    T = np.asarray(ref.loop_scene()["keyframes"][last["current"]]["kf"].tcw, np.float64).reshape(4, 4)
    assert np.abs(last["sim3"]["Scw"][:3, :3] - T[:3, :3]).max() < 5e-3
    assert np.abs(last["sim3"]["Scw"][:3, 3] - T[:3, 3]).max() < 0.1
