"""GPU parity on the crafted scenes of tests/matcher_scenes.py: k_candidates and k_greedy against the
sequential oracle, index-exact on every keypoint and on the match count, on the paths the census
(tests/test_matcher_edges_cpu.py) shows each scene to reach in the reference; and, from
orbmi_debug_greedy_stats, what the kernel itself did on them: the bounded-rounds fallback on the
long chain and not on the short one, the slow path on the clusters whose prefix runs out."""
import ctypes as C

import numpy as np
import pytest

import matcher_scenes as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    from orb_slam2_with_comment_amd import ORBmatcher
    return ORBmatcher


_REF = {}


def reference(oracle, sc):
    """the oracle's output on a scene, computed once and left unchanged"""
    key = (sc.name, sc.mode)
    if key not in _REF:
        out, n = S.run_oracle(oracle, sc)
        out.setflags(write=False)
        _REF[key] = (out, n)
    return _REF[key]


def search(m, sc, frame=None):
    frame = frame or sc.frame
    if sc.mode == 0:
        return m.SearchByProjection(frame, sc.occ, sc.mps, sc.track, sc.th)
    return m.SearchByProjectionLastFrame(frame, sc.occ, sc.lf, sc.lfp, sc.th, sc.mono)


def matcher(M, sc):
    return M(sc.nnratio) if sc.mode == 0 else M(0.9, sc.ori)


def parity(oracle, M, sc):
    ref, n_ref = reference(oracle, sc)
    m = matcher(M, sc)
    got, n = search(m, sc)
    m.close()
    np.testing.assert_array_equal(got, ref, err_msg=sc.name)
    assert n == n_ref, sc.name


def greedy_stats(reset=1):
    """{calls, rounds, largest round count, slow-path evaluations, fallbacks} since the last
    call; the first call switches the collection on, reset = -1 off"""
    from orb_slam2_with_comment_amd._capi import lib
    st = (C.c_ulonglong * 5)()
    assert lib().orbmi_debug_greedy_stats(st, reset) == 0
    return dict(zip(("calls", "rounds", "max_rounds", "slow", "fallbacks"), (int(v) for v in st)))


@pytest.fixture(scope="module", autouse=True)
def collection_off_afterwards():
    """the tests after this module run k_greedy as the ones before it did: not collecting"""
    yield
    greedy_stats(-1)


def parity_with_stats(oracle, M, sc):
    greedy_stats()
    parity(oracle, M, sc)
    st = greedy_stats()
    print(f"GREEDY {sc.name} mode {sc.mode}: {st}")
    assert st["calls"] == 1
    return st


def device_frame(F):
    """F with its keypoints, descriptors and u_right in HBM (used in place: such a frame's grid can be pinned)"""
    import torch
    d = (torch.from_numpy(F.keys.view(np.uint8)).cuda(), torch.from_numpy(F.desc).cuda(),
         torch.from_numpy(F.u_right).cuda())

    class P:
        keys = F.keys
        _keep = d

        def view(self):
            v = F.view()
            v.keys_un, v.desc, v.u_right = d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr()
            self._v = v
            return v
    return P()


def parity_pinned(oracle, M, sc):
    """device-resident frame arrays, the grid built once (Frame::AssignFeaturesToGrid) and pinned:
    two searches on it, neither rebuilding"""
    from orb_slam2_with_comment_amd._capi import lib
    ref, n_ref = reference(oracle, sc)
    P, m = device_frame(sc.frame), matcher(M, sc)
    v = P.view()
    assert lib().orbmi_matcher_assign_features_to_grid(m._h, C.addressof(v)) == 0
    for _ in range(2):
        got, n = search(m, sc, P)
        np.testing.assert_array_equal(got, ref, err_msg=sc.name)
        assert n == n_ref
    assert lib().orbmi_matcher_release_grid(m._h) == 0
    m.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_depth(oracle, M, mode):
    """every candidate count either side of 4/5, 8/9, 64/65 and 96/97, the answer behind 0, 3, 4,
    nc - 2, nc - 1 and nc occupied candidates: the prefix, the sorted top, the list and, for 97, 98
    and 150 candidates, the owning lane's walk over the window again"""
    st = parity_with_stats(oracle, M, S.depth(mode))
    assert st["slow"] > 0 and st["fallbacks"] == 0
    parity_pinned(oracle, M, S.depth(mode))


@pytest.mark.parametrize("variant", ["plain", "headless", "occupied", "noobs", "noobs_late"])
@pytest.mark.parametrize("length", [S.CHAIN_SHORT, S.CHAIN_LONG])
@pytest.mark.parametrize("mode", [0, 1])
def test_chain(oracle, M, mode, length, variant):
    """one link per round: the short chain converges inside kGreedyRounds, the long one does not
    and thread 0 replays it sequentially (and hands the results back to the register copies)"""
    st = parity_with_stats(oracle, M, S.chain(mode, length, variant))
    if variant == "plain" and length == S.CHAIN_SHORT:
        assert st["fallbacks"] == 0 and st["max_rounds"] >= 32
    if variant in ("plain", "noobs_late") and length == S.CHAIN_LONG:
        assert st["fallbacks"] == 1                                # noobs_late: replayed with a query that claims nothing
    if variant == "headless":
        assert st["fallbacks"] == 0 and st["max_rounds"] <= 3      # no dependency, no rounds
    if variant == "plain":
        parity_pinned(oracle, M, S.chain(mode, length, variant))


@pytest.mark.parametrize("variant", ["plain", "noobs", "noobs_late"])
@pytest.mark.parametrize("mode", [0, 1])
def test_chain_past_the_register_path(oracle, M, mode, variant):
    """the same fallback with more than 4,096 queries (results in memory, not in registers); the
    early query without MP_HAS_OBS cuts the chain short of it, so the rounds' own claims decide"""
    st = parity_with_stats(oracle, M, S.chain(mode, S.CHAIN_LONG, variant, True))
    assert st["fallbacks"] == (variant != "noobs")


@pytest.mark.parametrize("mode", [0, 1])
def test_depth_past_the_register_path(oracle, M, mode):
    """the same clusters among more than 4,096 queries: greedy_eval's own walk over the sorted top,
    the list in chunks of 16 and the window again"""
    st = parity_with_stats(oracle, M, S.depth(mode, True))
    assert st["fallbacks"] == 0


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("nnratio", [0.8, 0.6])
def test_decide(oracle, M, nnratio, big):
    """big: among more than 4,096 queries, where greedy_eval decides"""
    parity(oracle, M, S.decide(nnratio, big))


def test_pairs(oracle, M):
    """the wave-wide slow path's runner-up for every pair of candidates, so also for the pairs
    that one lane holds, wherever the list's arrival order put them"""
    sc = S.pairs()
    st = parity_with_stats(oracle, M, sc)
    assert st["slow"] >= sc.nq and st["fallbacks"] == 0


def test_window(oracle, M):
    parity(oracle, M, S.window())


@pytest.mark.parametrize("direction,mono", [("still", False), ("forward", False), ("backward", False), ("forward", True)])
def test_window_directions(oracle, M, direction, mono):
    parity(oracle, M, S.window1(direction, mono))


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("name", list(S.ROTATIONS))
def test_rotation(oracle, M, name, big):
    parity(oracle, M, S.rotation(name, big))


@pytest.mark.parametrize("mode", [0, 1])
def test_many_keypoints(oracle, M, mode):
    """kGreedyMaxKp keypoints: the later passes of the occupancy / octave load, prefix entries and
    claims on keypoint indices above 12 bits, up to 16,383"""
    st = parity_with_stats(oracle, M, S.many_keypoints(mode))
    assert st["slow"] > 0 and st["fallbacks"] == 0


@pytest.mark.parametrize("mode", [0, 1])
def test_one_keypoint_too_many(M, mode):
    from orb_slam2_with_comment_amd._capi import ORBMI_E_UNSUPPORTED, OrbmiError
    sc = S.many_keypoints(mode, S.MAX_KP + 1)
    assert len(sc.frame.keys) == S.MAX_KP + 1
    m = matcher(M, sc)
    with pytest.raises(OrbmiError) as e:
        search(m, sc)
    assert e.value.code == ORBMI_E_UNSUPPORTED and "ORBMI_E_UNSUPPORTED" in str(e.value)
    m.close()
