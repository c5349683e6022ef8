"""Frame::ComputeStereoMatches without a GPU: the numpy restatement (tests/stereo_reference.py)
equals the oracle bit for bit on every scene of tests/stereo_scenes.py, and every scene reaches the
branches it was built for.  The census numbers are conditions on the scenes, not measurements: a
scene that stops covering its branch fails here."""
import numpy as np
import pytest

import stereo_reference as SR
import stereo_scenes as SC

CASES = SC.CASES  # names only: a scene is generated inside the first test that uses it
IDS = [f"{s}-{v}" for s, v in CASES]


def _keypoints(oracle, scene, variant):
    return variant.kps or SC.own_keypoints(oracle, scene)


@pytest.mark.parametrize("scene,variant", CASES, ids=IDS)
def test_restatement_equals_oracle(oracle, scene, variant):
    scene = SC.scene(scene)
    variant = SC.variant(scene, variant)
    res = SC.reference(oracle, scene, variant)
    p = oracle.params(scene.nfeatures, scene.scale_factor, scene.nlevels)
    u, d = oracle.stereo(p, scene.left, scene.right, scene.bf, scene.fx, *_keypoints(oracle, scene, variant))
    bad = np.nonzero((u.view(np.uint32) != res.u_right.view(np.uint32))
                     | (d.view(np.uint32) != res.depth.view(np.uint32)))[0]
    assert len(bad) == 0, (f"{len(bad)} keypoints differ, first {bad[0]} "
                           f"({SR.OUTCOME_NAMES[res.outcome[bad[0]]]}): oracle {u[bad[0]]} {d[bad[0]]}, "
                           f"restatement {res.u_right[bad[0]]} {res.depth[bad[0]]}")


@pytest.mark.parametrize("scene,variant", CASES, ids=IDS)
def test_scene_census(oracle, scene, variant):
    scene = SC.scene(scene)
    variant = SC.variant(scene, variant)
    res = SC.reference(oracle, scene, variant)
    c = SR.census(res)
    print(scene.name, variant.name, c)
    for code, least in variant.need.items():
        assert c[SR.OUTCOME_NAMES[code]] >= least, (SR.OUTCOME_NAMES[code], c)
    for i, r in variant.chosen.items():
        assert res.idx_r[i] == r, f"left keypoint {i} chose {res.idx_r[i]}, built for {r}"
    for i, ok in variant.allowed.items():
        assert res.outcome[i] in ok, f"left keypoint {i}: {SR.OUTCOME_NAMES[res.outcome[i]]}"
    if variant.median is not None:
        assert variant.median[0] <= res.median <= variant.median[1], c
    if variant.tail_from is not None:
        # the left keypoints past k_stereo_filter's registers carry SADs: one the median culls,
        # and (where there are several) ones whose loss from the histogram would move the median
        tail = res.outcome[variant.tail_from:]
        assert np.isin(tail, (SR.ACCEPTED, SR.CULLED)).all() and (tail == SR.CULLED).any(), tail
        if len(tail) > 1:
            assert (tail == SR.ACCEPTED).any(), tail
            # ... which the outputs show: with the median of the SADs below tail_from alone, the
            # cull set would be another one
            took = np.isin(res.outcome, (SR.ACCEPTED, SR.ACCEPTED_CLAMP, SR.CULLED))
            head = np.sort(res.sad[:variant.tail_from][took[:variant.tail_from]])
            th_head = np.float32(1.5) * np.float32(1.4) * np.float32(head[len(head) // 2])
            assert th_head != res.th_dist, (th_head, res.th_dist)
            cull_head = took & ~(res.sad.astype(np.float32) < th_head)
            assert (cull_head != (res.outcome == SR.CULLED)).any(), (th_head, res.th_dist)
    # an accepted match is a finite depth and a column left of the keypoint's own
    ok = res.depth > 0
    assert (ok == np.isin(res.outcome, (SR.ACCEPTED, SR.ACCEPTED_CLAMP))).all()
    kl = _keypoints(oracle, scene, variant)[0]
    assert np.isfinite(res.depth[ok]).all() and (res.u_right[ok] < kl["x"][ok]).all()


def test_high_sad_defeats_a_15_bit_select(oracle):
    """The select k_stereo_filter used before (256 bins of x >> 7 clamped to 255, then 128 bins of
    x & 127 over the values with x >> 7 == bin exactly), restated on the scene's accepted SADs:
    it does not find the median of `above`, which is what made the scene necessary."""
    def select15(sads):
        sads = np.sort(sads)
        rank = len(sads) // 2
        h1 = np.bincount(np.minimum(sads >> 7, 255), minlength=256)
        b1 = int(np.searchsorted(np.cumsum(h1), rank, side="right"))
        rest = rank - int(h1[:b1].sum())
        h2 = np.bincount(sads[(sads >> 7) == b1] & 127, minlength=128)
        cum = np.cumsum(h2)
        if rest >= cum[-1]:
            return b1  # no bin found: the bin number is left in place
        return (b1 << 7) | int(np.searchsorted(cum, rest, side="right"))

    above, bin255 = SC.high_sad()
    res = SC.reference(oracle, above, above.variants[0])
    sads = res.sad[res.depth > 0]
    assert res.median > 32767 and len(sads) >= 1
    assert select15(sads) == 255 != int(res.median)
    res = SC.reference(oracle, bin255, bin255.variants[0])
    assert select15(res.sad[res.sad >= 0]) == int(res.median) == 32736  # the old select still held here
    assert (res.sad > 32767).sum() >= 3


def test_row_list_bound_is_reached(oracle):
    """pyramid_top fills ceil(4 * scale) + 2 rows with every right keypoint, which is the bound
    stereo_run sizes the row list by; 24 rows per keypoint fall short of it."""
    for key in SC.PYRAMIDS:
        s = SC.pyramid_top(key)
        v = s.variants[0]
        kr = v.kps[2]
        scale, _ = SC.scale_tables(s.scale_factor, s.nlevels)
        r = np.float32(2.0) * scale[kr["octave"]]
        n = np.ceil(kr["y"] + r).astype(int) - np.floor(kr["y"] - r).astype(int) + 1
        assert len(kr) == s.capacity == 256 and (n == v.rows_per_keypoint).all()
        assert v.rows_per_keypoint == int(np.ceil(np.float32(4.0) * scale.max())) + 2 > 24
