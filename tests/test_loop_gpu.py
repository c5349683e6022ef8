"""GPU parity of loop detection with the restatement (tests/loop_reference.py): the device
KeyFrameDatabase (csrc/kfdb.hip) -- per-slot counts, scores bit for bit, list order, candidates --
SearchByBoW(KF, KF) (k_bow_match_kf), the C++ adapters and detect_and_compute_sim3 end to end.
Everything is compared for equality; only Scw of the end-to-end case has a bound, the one
test_compute_sim3_end_to_end derives."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_reference as ref  # noqa: E402
from test_loop_cpu import _hand_db, _masks, th_low_pair  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


def device_db(scoring=0, max_keyframes=320, max_words_total=None):
    from orb_slam2_with_comment_amd.loop import KeyFrameDatabase
    return KeyFrameDatabase(scoring, max_keyframes, max_words_total or max_keyframes * 320)


def bits(a):
    return np.asarray(a, np.float64).tobytes()


def sharing_order(q):
    """lKFsSharingWords from a device query: ascending (first_word, add_seq) of the slots with common > 0."""
    s = [k for k in range(len(q["kf_id"])) if q["common"][k] > 0]
    s.sort(key=lambda k: (int(q["first_word"][k]), int(q["add_seq"][k])))
    return [int(q["kf_id"][k]) for k in s]


def compare_query(db, rdb, word, value, connected=()):
    """One query on both databases: every per-slot figure equal, scores bit for bit."""
    q, r = db.query(word, value, connected), rdb.query(word, value, connected)
    assert (q["max_common"], q["min_common"]) == (r["max_common"], r["min_common"])
    ids = [int(i) for i in q["kf_id"]]
    assert [int(c) for c in q["common"]] == [r["common"].get(i, 0) for i in ids]
    assert sharing_order(q) == r["order"]
    want = np.array([r["score"].get(i, 0.0) for i in ids], np.float64)
    assert bits(q["score"]) == bits(want), (q["score"], want)
    return q, r


# ---- synthetic sparse vectors: sizes ---------------------------------------------------------------

SIZE_CASES = [(seed, ndb, nq) for seed, (ndb, nq) in enumerate(
    [(ndb, nq) for ndb in (0, 1, 5, 65, 300) for nq in (0, 1, 63, 64, 65, 257)])]


@pytest.mark.parametrize("seed,ndb,nq", SIZE_CASES, ids=lambda v: str(v))
def test_database_equals_the_inverted_file(seed, ndb, nq):
    """Query lengths 0 .. 257, stored lengths 0 .. 300, 0 .. 300 slots (65 and 300: more than one
    workgroup's waves), L1 and L2 alternating: counts, order, scores, candidates and
    orbmi_kfdb_score on every stored id, indexed or not."""
    case = ref.database_case(seed, ndb, nq, scoring=seed % 2)
    db, rdb = ref.fill(device_db(case["scoring"]), case), ref.fill(ref.KeyFrameDatabase(case["scoring"]), case)
    qw, qv = case["query"]
    q, r = compare_query(db, rdb, qw, qv, case["connected"])
    ids = [i for i, _, _ in case["store"]]
    assert bits(db.score(qw, qv, ids)) == bits(rdb.score(qw, qv, ids))
    for ms in (F32(0), ref.min_score_for(case), F32(2)):
        got = db.DetectLoopCandidates(qw, qv, ms, case["connected"], case["best_covis"])
        assert got == rdb.DetectLoopCandidates(qw, qv, ms, case["connected"], case["best_covis"])
    if ndb == 0 or nq == 0:
        assert db.DetectLoopCandidates(qw, qv, 0.0, (), {}) == []
    db.close()


# ---- overlap positions and content -------------------------------------------------------------------

def _vec(words, rng, l2=False):
    w = np.array(sorted(words), np.uint32)
    v = rng.uniform(0.1, 1.0, len(w))
    v = v / (np.sqrt((v * v).sum()) if l2 else v.sum())
    return w, v


@pytest.mark.parametrize("scoring", [0, 1])
def test_overlap_positions(scoring):
    rng = np.random.default_rng(4 + scoring)
    l2 = scoring == 1
    base = list(range(1000, 1000 + 2 * 130, 2))  # 130 even words: the query
    q = _vec(base, rng, l2)
    odd = list(range(1001, 1001 + 2 * 140, 2))   # never in the query
    stored = {
        1: [base[0]] + odd[:99],                 # the only shared word first in both
        2: odd[:99] + [base[-1]],                # last in both
        3: [5] + odd[:70] + [base[0]],           # first of the query, last of the keyframe
        4: [base[-1]] + [w + 5000 for w in odd[:80]],  # last of the query, first of the keyframe
        5: list(range(100, 162)) + base[10:14] + [w + 5000 for w in odd[:20]],  # shared words at positions 62 .. 65: a chunk boundary
        6: base,                                 # identical words (and, below, identical values)
        7: odd,                                  # disjoint
        8: [],                                   # empty
        9: base[60:70],                          # the query's own chunk boundary
    }
    db, rdb = device_db(scoring), ref.KeyFrameDatabase(scoring)
    for i, words in stored.items():
        w, v = (q if i == 6 else _vec(words, rng, l2))
        for d in (db, rdb):
            d.store(i, w, v)
            d.add(i)
    qq, r = compare_query(db, rdb, *q)
    assert r["order"][:3] == [1, 3, 6]  # word base[0] is met first, its list is in add order
    assert 7 not in r["order"] and 8 not in r["order"]
    ids = list(stored)
    got, want = db.score(*q, ids), rdb.score(*q, ids)
    assert bits(got) == bits(want)
    if l2:
        assert want[ids.index(6)] == 1.0 or abs(want[ids.index(6)] - 1.0) < 1e-7  # the sum is 1 up to rounding
    assert want[ids.index(7)] == 0.0
    # L2's score >= 1 branch for certain: values whose squares sum to exactly 1
    if l2:
        h = (np.array([1, 2, 3, 4], np.uint32), np.full(4, 0.5))
        for d in (db, rdb):
            d.store(20, *h)
        assert db.score(*h, [20]).tolist() == rdb.score(*h, [20]).tolist() == [1.0]
    # nothing shares a word: empty
    lone = (np.array([7], np.uint32), np.array([1.0]))
    assert db.DetectLoopCandidates(*lone, 0.0) == rdb.DetectLoopCandidates(*lone, 0.0) == []
    assert db.query(*lone)["max_common"] == 0
    db.close()


@pytest.mark.parametrize("maxc,minc", [(5, 4), (6, 4), (10, 8), (15, 12)])
def test_min_common_words_truncation(maxc, minc):
    qw = list(range(100, 100 + maxc))
    q = (qw, [1.0 / maxc] * maxc)
    db, rdb = device_db(), ref.KeyFrameDatabase()
    for d in (db, rdb):
        d.store(0, *q)
        for k in (1, 2, 3):  # minc - 1, minc (exactly at the threshold: not scored), minc + 1 shared words
            w = qw[:minc - 2 + k] + [900 + k]
            d.store(k, w, [1.0 / len(w)] * len(w))
        for k in range(4):
            d.add(k)
    g, r = compare_query(db, rdb, *q)
    assert (g["max_common"], g["min_common"]) == (maxc, minc)
    assert [bool(s) for s in g["score"]] == [True, False, False, True]
    assert db.DetectLoopCandidates(*q, 0.0) == rdb.DetectLoopCandidates(*q, 0.0)
    db.close()


# ---- order, the connected list, the accumulation -------------------------------------------------------

def _hand_pair():
    rdb, q = _hand_db()
    db = device_db()
    for i, kf in rdb.kfs.items():
        db.store(i, kf.mBowVec.word, kf.mBowVec.value)
    for i in (7, 3, 5, 9, 2):
        db.add(i)
    return db, rdb, q


def test_list_order():
    db, rdb, q = _hand_pair()
    assert sharing_order(db.query(*q)) == [9, 7, 3, 5]  # 9's first shared word is smaller; then add order 7, 3, 5
    for d in (db, rdb):
        d.erase(3)
    compare_query(db, rdb, *q)
    for d in (db, rdb):
        d.add(3)
    assert sharing_order(compare_query(db, rdb, *q)[0]) == [9, 7, 5, 3]  # erased and added again: at the back
    assert db.DetectLoopCandidates(*q, 0.1) == rdb.DetectLoopCandidates(*q, 0.1) == [9, 3]
    db.close()


def test_connected_list_and_accumulation():
    db, rdb, q = _hand_pair()
    calls = [
        (0.1, (), {}, [9, 3]),
        (0.7, (), {}, [3]),
        (0.8, (), {}, []),                       # a minScore that removes everything
        (0.1, (), {9: [3]}, [3]),                # replaced by a better-scoring neighbour
        (0.1, (), {9: [3], 3: [9]}, [3]),        # two entries naming the same keyframe: listed once
        (0.1, (), {9: [7, 8, 2]}, [9, 3]),       # neighbours that were not scored add nothing
        (0.1, [3], {9: [3]}, [9]),               # a connected keyframe: absent, and no neighbour
        (0.1, [3, 9, 40], {}, [7]),              # ... and no part of max_common: 7's two words now suffice (40: unknown, ignored)
    ]
    for ms, conn, covis, want in calls:
        got = db.DetectLoopCandidates(*q, ms, conn, covis)
        assert got == rdb.DetectLoopCandidates(*q, ms, conn, covis) == want, (ms, conn, covis, got)
    g, _ = compare_query(db, rdb, *q, connected=[3, 9])
    assert g["max_common"] == 2
    # stored but not indexed (8), indexed (3), and the stored-only id after an erase
    assert bits(db.score(*q, [8, 3, 2])) == bits(rdb.score(*q, [8, 3, 2]))
    assert db.score(*q, [8]).tolist() == [1.0]
    db.close()


def test_status_codes():
    from orb_slam2_with_comment_amd._capi import (ORBMI_E_ARG, ORBMI_E_CAP, ORBMI_E_STATE, ORBMI_E_UNSUPPORTED,
                                                  OrbmiError)
    from orb_slam2_with_comment_amd.loop import KeyFrameDatabase

    def code(fn, *a):
        with pytest.raises(OrbmiError) as e:
            fn(*a)
        return e.value.code
    for scoring in (2, 3, 4, 5):
        assert code(KeyFrameDatabase, scoring, 4, 64) == ORBMI_E_UNSUPPORTED
    db = KeyFrameDatabase(0, 2, 10)
    db.store(4, [1, 2, 3], [0.2, 0.3, 0.5])
    assert code(db.store, 4, [1], [1.0]) == ORBMI_E_STATE          # stored twice
    assert code(db.store, 5, [3, 2], [0.5, 0.5]) == ORBMI_E_ARG    # not ascending
    assert code(db.store, 5, [2, 2], [0.5, 0.5]) == ORBMI_E_ARG    # not strictly
    assert code(db.store, 5, list(range(8)), [0.125] * 8) == ORBMI_E_CAP  # 3 + 8 > 10 words
    db.store(5, [7], [1.0])
    assert code(db.store, 6, [7], [1.0]) == ORBMI_E_CAP            # a third slot
    assert code(db.add, 9) == ORBMI_E_ARG and code(db.erase, 9) == ORBMI_E_ARG  # unknown id
    assert code(db.score, [1], [1.0], [4, 9]) == ORBMI_E_ARG
    db.add(4)
    assert code(db.add, 4) == ORBMI_E_STATE
    db.clear()
    db.store(4, [1], [1.0])  # cleared: the id and the capacity are free again
    assert db.query([1], [1.0])["max_common"] == 0  # stored, not added
    db.close()


def test_device_pointer_store_from_transform_device(oracle):
    """orbmi_transform's device outputs go into the arena without a host round trip: the same
    query result as the host path."""
    import torch
    from scenario import frame_data
    from orb_slam2_with_comment_amd.vocabulary import ORBVocabulary, Vocabulary
    v = Vocabulary.synthetic(k=10, L=4, seed=9)
    gv = ORBVocabulary(v, device=0)
    host, dev = device_db(0, 8, 8 * 2100), device_db(0, 8, 8 * 2100)
    cap = 2048
    for f in (3, 4):
        dl = frame_data(f)[1]
        w, val, _ = gv.transform(dl, 4)
        host.store(f, w, val)
        host.add(f)
        d_desc = torch.zeros((cap, 32), dtype=torch.uint8, device="cuda")
        d_desc[:len(dl)] = torch.from_numpy(dl).cuda()
        outs = dict(word=torch.zeros(cap, dtype=torch.int32, device="cuda"), value=torch.zeros(cap, dtype=torch.float64, device="cuda"),
                    node=torch.zeros(cap, dtype=torch.int32, device="cuda"), off=torch.zeros(cap + 1, dtype=torch.int32, device="cuda"),
                    feat=torch.zeros(cap, dtype=torch.int32, device="cuda"), counts=torch.zeros(2, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        gv.transform_device(d_desc.data_ptr(), len(dl), None, 4, *(outs[k].data_ptr() for k in
                            ("word", "value", "node", "off", "feat", "counts")))
        gv.synchronize()
        nw = int(outs["counts"].cpu()[0])
        assert nw == len(w)
        dev.store_device(f, outs["word"].data_ptr(), outs["value"].data_ptr(), nw)
        dev.add(f)
    qw, qv, _ = gv.transform(frame_data(5)[1], 4)
    a, b = host.query(qw, qv), dev.query(qw, qv)
    for k in ("kf_id", "common", "first_word", "add_seq"):
        np.testing.assert_array_equal(a[k], b[k])
    print("max_common", a["max_common"])
    assert bits(a["score"]) == bits(b["score"]) and a["max_common"] == b["max_common"] > 0
    host.close(), dev.close(), gv.close()


# ---- SearchByBoW(KF, KF) -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def matcher():
    from orb_slam2_with_comment_amd.matcher import ORBmatcher
    m = ORBmatcher(0.75, True)
    yield m
    m.close()


@pytest.fixture(scope="module")
def stereo_pair_kfs(oracle):
    """Frames 3 and 4 of the synthetic sequence, synth_map.bow_nodes as the vocabulary, masks from
    stereo depth; and their restated matches for both orientation settings."""
    import scenario
    from orb_slam2_with_comment_amd import synth_map as SM
    from orb_slam2_with_comment_amd.types import FeatureVector
    kf1, kf2 = scenario.make_frame(3), scenario.make_frame(4)
    ok1 = (scenario.frame_data(3)[3] > 0).astype(np.uint8)
    ok2 = (scenario.frame_data(4)[3] > 0).astype(np.uint8)
    fv1, fv2 = FeatureVector(SM.bow_nodes(kf1.desc)), FeatureVector(SM.bow_nodes(kf2.desc))
    want = {ori: ref.search_by_bow_kf(kf1, ok1, fv1, kf2, ok2, fv2, 0.75, ori) for ori in (False, True)}
    return kf1, ok1, fv1, kf2, ok2, fv2, want


@pytest.mark.parametrize("ori", [False, True])
def test_search_by_bow_kf_on_two_keyframes(matcher, stereo_pair_kfs, ori):
    kf1, ok1, fv1, kf2, ok2, fv2, want = stereo_pair_kfs
    m, n = matcher.SearchByBoWKF(kf1, ok1, fv1, kf2, ok2, fv2, checkOri=ori)
    np.testing.assert_array_equal(m, want[ori][0])
    assert n == want[ori][1] >= 50
    assert want[True][1] < want[False][1]  # the histogram removes something


def test_search_by_bow_kf_masks_th_low_and_ties(matcher, stereo_pair_kfs):
    kf1, ok1, fv1, kf2, ok2, fv2, _ = stereo_pair_kfs
    for o1, o2 in ((np.zeros_like(ok1), ok2), (ok1, np.zeros_like(ok2))):  # a mask that empties one side
        m, n = matcher.SearchByBoWKF(kf1, o1, fv1, kf2, o2, fv2)
        assert n == 0 and (m == -1).all()
    # half of either side masked: both gates matter
    h1, h2 = ok1 & (np.arange(len(ok1)) % 2 == 0), ok2 & (np.arange(len(ok2)) % 3 != 0)
    m, n = matcher.SearchByBoWKF(kf1, h1, fv1, kf2, h2, fv2)
    w, wn = ref.search_by_bow_kf(kf1, h1, fv1, kf2, h2, fv2, 0.75, True)
    np.testing.assert_array_equal(m, w)
    assert n == wn > 20 and h1[m >= 0].all() and h2[m[m >= 0]].all()
    # a pair at distance exactly TH_LOW: rejected here, accepted by the (KF, Frame) form
    one = np.ones(1, np.uint8)
    for dist, want in ((49, 0), (50, -1), (51, -1)):
        a, fa, b, fb = th_low_pair(dist)
        m, n = matcher.SearchByBoWKF(a, one, fa, b, one, fb)
        assert m.tolist() == [want] and n == (want >= 0)
    a, fa, b, fb = th_low_pair(50)
    assert matcher.SearchByBoW(a, one, fa, b, fb)[0].tolist() == [0]
    # the small synthetic pairs (outlier angles, a node KF1 lacks, ties in node order)
    for seed in (0, 1):
        k1, f1, k2, f2, _ = ref.bow_pair(seed)
        o1, o2 = _masks(k1, k2, seed)
        for ori in (False, True):
            m, n = matcher.SearchByBoWKF(k1, o1, f1, k2, o2, f2, checkOri=ori)
            w, wn = ref.search_by_bow_kf(k1, o1, f1, k2, o2, f2, 0.75, ori)
            np.testing.assert_array_equal(m, w)
            assert n == wn > 20
    # empty keyframes
    from orb_slam2_with_comment_amd import synth
    from orb_slam2_with_comment_amd.types import KP_DTYPE, FeatureVector, Frame
    e = Frame(np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8), None, None, synth.KITTI)
    efv = FeatureVector(np.zeros(0, np.int64))
    assert matcher.SearchByBoWKF(e, np.zeros(0, np.uint8), efv, kf2, ok2, fv2)[1] == 0
    assert matcher.SearchByBoWKF(kf1, ok1, fv1, e, np.zeros(0, np.uint8), efv)[1] == 0


def test_search_by_bow_kf_node_beyond_the_register_window(matcher):
    """One node with 700 KF2 features (the kernel keeps vbMatched2 of the first 512 in registers,
    the rest is re-read from memory): the true partners sit on both sides of the window."""
    k1, f1, k2, f2, perm = ref.bow_pair(5, n1=90, n2=700, nnodes=1, flip=10)
    from orb_slam2_with_comment_amd.types import FeatureVector
    f1, f2 = FeatureVector(np.zeros(90, np.int64)), FeatureVector(np.zeros(700, np.int64))
    # duplicate descriptors in KF1: the second of a pair must find its partner taken (vbMatched2)
    k1.desc[45:90] = k1.desc[0:45]
    o1, o2 = np.ones(90, np.uint8), np.ones(700, np.uint8)
    w, wn = ref.search_by_bow_kf(k1, o1, f1, k2, o2, f2, 0.75, False)
    m, n = matcher.SearchByBoWKF(k1, o1, f1, k2, o2, f2, checkOri=False)
    np.testing.assert_array_equal(m, w)
    hit = w[:45][w[:45] >= 0]
    assert n == wn and (hit < 512).any() and (hit >= 512).any()
    assert (w[45:90] != w[0:45])[w[0:45] >= 0].all()  # the duplicates did not take the same keypoint


def test_cpp_dropin_search_by_bow_kf(tmp_path, matcher, stereo_pair_kfs):
    from test_cpp_dropin import build_dropin
    kf1, ok1, fv1, kf2, ok2, fv2, want = stereo_pair_kfs
    d = tmp_path
    v = kf1.view()
    np.array([v.fx, v.fy, v.cx, v.cy, v.bf, v.mb, v.max_x, v.max_y, v.grid_w_inv, v.grid_h_inv, v.log_scale_factor],
             np.float32).tofile(d / "in_cam.bin")
    kf1.scale_factors.tofile(d / "in_scale_factors.bin")
    np.array([0.75, 1], np.float32).tofile(d / "in_param.bin")
    for name, kf, ok, fv in (("kf1", kf1, ok1, fv1), ("kf2", kf2, ok2, fv2)):
        kf.keys.tofile(d / f"in_{name}_keys.bin")
        kf.desc.tofile(d / f"in_{name}_desc.bin")
        ok.tofile(d / f"in_{name}_ok.bin")
        fv.node_id.tofile(d / f"in_{name}_fv_node.bin")
        fv.off.tofile(d / f"in_{name}_fv_off.bin")
        fv.feat.tofile(d / f"in_{name}_fv_feat.bin")
    exe = build_dropin(str(d), "dropin_loop")
    subprocess.run([exe, "bow", str(d)], check=True, timeout=120)
    np.testing.assert_array_equal(np.fromfile(d / "out_match12.bin", np.int32), want[True][0])
    assert np.fromfile(d / "out_nmatches.bin", np.int32).tolist() == [want[True][1]]


def test_cpp_dropin_detect_loop_candidates(tmp_path):
    """orbmi::KeyFrameDatabase from C++ with DetectLoop's call shape: the minScore loop over the
    covisibles, then DetectLoopCandidates: the restatement's scores (bit for bit) and candidates."""
    from test_cpp_dropin import build_dropin
    case = ref.database_case(3, 65, 257)
    d = tmp_path
    ids = [i for i, _, _ in case["store"]]
    np.array([case["scoring"], len(ids)], np.int32).tofile(d / "in_db_head.bin")
    np.array(ids, np.int32).tofile(d / "in_db_ids.bin")
    np.array([len(w) for _, w, _ in case["store"]], np.int32).tofile(d / "in_db_len.bin")
    np.concatenate([w for _, w, _ in case["store"]]).astype(np.uint32).tofile(d / "in_db_word.bin")
    np.concatenate([v for _, _, v in case["store"]]).astype(np.float64).tofile(d / "in_db_value.bin")
    np.array([[1 if op == "add" else 0, i] for op, i in case["ops"]], np.int32).tofile(d / "in_ops.bin")
    qw, qv = case["query"]
    qw.tofile(d / "in_q_word.bin")
    qv.tofile(d / "in_q_value.bin")
    np.array(case["connected"], np.int32).tofile(d / "in_connected.bin")
    rdb = ref.fill(ref.KeyFrameDatabase(case["scoring"]), case)
    # covisibles for minScore: the connected keyframes and the three that score best
    sc = rdb.query(qw, qv, case["connected"])["score"]
    covisible = list(case["connected"]) + sorted(sc, key=sc.get)[-3:]
    np.array(covisible, np.int32).tofile(d / "in_covisible.bin")
    n_ids = max(ids) + 1
    rows = [np.asarray(case["best_covis"].get(i, ()), np.int32) for i in range(n_ids)]
    np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32).tofile(d / "in_covis_off.bin")
    np.concatenate(rows).astype(np.int32).tofile(d / "in_covis_ids.bin")
    exe = build_dropin(str(d), "dropin_loop")
    subprocess.run([exe, "detect", str(d)], check=True, timeout=120)
    want_scores = rdb.score(qw, qv, covisible)
    assert (d / "out_scores.bin").read_bytes() == bits(want_scores)
    ms = want_scores.astype(np.float32).min()
    assert np.fromfile(d / "out_min_score.bin", np.float32).tolist() == [ms]
    want = rdb.DetectLoopCandidates(qw, qv, ms, case["connected"], case["best_covis"])
    assert np.fromfile(d / "out_candidates.bin", np.int32).tolist() == want and len(want) >= 1


# ---- one scene, end to end --------------------------------------------------------------------------------

def test_detect_and_compute_sim3_end_to_end(oracle, matcher):
    """Keyframes 0 .. 11 of the synthetic sequence in the database, the current keyframes fresh
    renders of frame 3's pose: the device backend and the restatement backend give the same
    candidates in the same order, the same BoW matches, the same accepted candidate and matches;
    Scw within the bound test_compute_sim3_end_to_end derives.  DetectLoop counts a group's
    consistency from 0, so the threshold 3 is reached by the fourth consecutive query."""
    from orb_slam2_with_comment_amd.loop import LoopBackend
    want = ref.run_loop_scene(ref.RestatementLoopBackend())
    be = LoopBackend(matcher=matcher, max_keyframes=32, max_words_total=32 * 2100)
    got = ref.run_loop_scene(be)
    sc = ref.loop_scene()
    near = {ref.SCENE_REVISITED - 1, ref.SCENE_REVISITED, ref.SCENE_REVISITED + 1}
    assert [r["detected"] for r in want] == [False, False, False, True]
    for g, w in zip(got, want):
        assert near & set(w["candidates"])  # the revisited keyframe or a direct neighbour: the scene's property
        assert g["candidates"] == w["candidates"] and g["consistent"] == w["consistent"]
        assert g["detected"] == w["detected"] and g["current"] == w["current"] and g["loop_kf"] == w["loop_kf"]
        assert len(g["bow_matches"]) == len(w["bow_matches"])
        for a, b in zip(g["bow_matches"], w["bow_matches"]):
            np.testing.assert_array_equal(a, b)
    g, w = got[-1]["sim3"], want[-1]["sim3"]
    print("driver log", g["log"])
    assert g["accepted"] and w["accepted"] and g["candidate"] == w["candidate"]
    assert got[-1]["loop_kf"] in near
    np.testing.assert_array_equal(g["matches"], w["matches"])
    np.testing.assert_array_equal(g["loop_matched"], w["loop_matched"])
    assert g["n_total"] == w["n_total"] >= 40
    cand = sc["keyframes"][got[-1]["loop_kf"]]
    tmw = np.abs(np.asarray(cand["kf"].tcw, np.float64).reshape(4, 4)[:3, 3]).max()
    tol = 1e-4 * (3 * tmw + 1)
    dev = np.abs(g["Scw"].astype(np.float64) - w["Scw"].astype(np.float64)).max()
    print("max |Scw gpu - Scw restatement| %.3e (bound %.3e)" % (dev, tol))
    assert dev <= tol
    be.close()
