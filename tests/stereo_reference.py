"""Frame::ComputeStereoMatches (reference src/Frame.cc:501-675) restated in plain numpy.

A second restatement, written from the reference's text and independent of both
oracle/orb_stereo_oracle.cpp and csrc/stereo.hip: the CPU tests hold it against the oracle, the GPU
tests hold the kernels against it.  Beyond mvuRight / mvDepth it reports, per left keypoint, which
way out of the reference's loop the keypoint took, so a scene can assert that it reaches the branch
it was built for and a mismatch can be named by branch.

Arithmetic: every quantity the reference holds in a `float` is an np.float32 here and every
operation on them rounds once (no contraction); `round()` is C's (halves away from zero); the
float -> int conversions truncate.  The SADs are cv::norm(IL, IR, NORM_L1) of two 11 x 11 float
patches with their centre pixels subtracted: integers, at most 121 * 510 = 61,710, so every partial
sum is exact in float and the order of summation does not matter.

Pinned semantics: Frame::mb is read at :531 before the constructor assigns it, and
mb = bf / fx is used; when no match is accepted the reference indexes an empty vector at :662, and
no filtering is done.

The way out `deltaR < -1 || deltaR > 1` (:639) cannot be taken and has no outcome code.  The best
shift is the first strict minimum of the 11 SADs and lies strictly inside the range when :633 is
reached, so dist1 > dist2 and dist3 >= dist2 (integers, exact in float).  With a = dist1 - dist2
>= 1 and b = dist3 - dist2 >= 0, deltaR = (a - b) / (2 (a + b)): the denominator is at least 2,
so the quotient is finite, and |a - b| <= a + b bounds it by 1/2.  Each float operation rounds
monotonically and 1/2 is representable, so the computed deltaR lies in [-1/2, 1/2] too.

The image pyramids are inputs (oracle.pyramid's padded levels, 19 px of border), as are the scale
tables: both have parity tests of their own.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

NO_CANDIDATES = 0     # :548 the keypoint's row holds no right keypoint (or :554, maxU < 0)
HAMMING_REJECT = 1    # :587 best descriptor distance >= (TH_HIGH + TH_LOW) / 2 = 75
WINDOW_OFF_LEVEL = 2  # :610 the sliding window leaves the level
SHIFT_AT_END = 3      # :629 the best shift is -L or +L
DISPARITY_NEG = 4     # :647 disparity < minD = 0
DISPARITY_MAX = 5     # :647 disparity >= maxD
ACCEPTED = 6          # :654-656, survives the median cull
ACCEPTED_CLAMP = 7    # :649-653 disparity <= 0 replaced by 0.01, survives the cull
CULLED = 8            # :665-674 SAD >= 2.1 * median
OUTCOME_NAMES = ["no candidates", "Hamming reject", "window off the level", "best shift at +-L",
                 "disparity negative", "disparity >= maxD", "accepted", "accepted through the 0.01 clamp",
                 "culled by the median"]

EDGE = 19  # EDGE_THRESHOLD: the border of every padded pyramid level
TH_HIGH, TH_LOW = 100, 50
_POPC = np.array([bin(i).count("1") for i in range(256)], np.int32)
_F = np.float32

StereoResult = namedtuple("StereoResult", "u_right depth outcome idx_r shift sad median th_dist clamped")


def c_round(x) -> float:
    """round(float): nearest integer, halves away from zero (exact: x + 0.5 in double)."""
    x = float(x)
    return math.floor(x + 0.5) if x >= 0 else -math.floor(-x + 0.5)


def compute_stereo_matches(pyr_left, pyr_right, scale, inv_scale, bf, fx, kps_l, desc_l, kps_r, desc_r):
    """-> StereoResult: u_right, depth (float32, N); per left keypoint outcome (codes above), idx_r
    (chosen right keypoint, -1 before :587 passes), shift (best incR, 0 when no SAD ran), sad (best
    SAD, -1 when none) and clamped (the 0.01 clamp fired); median and th_dist (float32 scalars, NaN
    when nothing was accepted)."""
    scale = np.asarray(scale, _F)
    inv_scale = np.asarray(inv_scale, _F)
    desc_l = np.asarray(desc_l, np.uint8).reshape(-1, 32)
    desc_r = np.asarray(desc_r, np.uint8).reshape(-1, 32)
    N, Nr = len(kps_l), len(kps_r)
    u_right = np.full(N, -1, _F)
    depth = np.full(N, -1, _F)
    outcome = np.full(N, NO_CANDIDATES, np.int32)
    idx_r = np.full(N, -1, np.int32)
    shift = np.zeros(N, np.int32)
    sad = np.full(N, -1, np.int32)
    clamped = np.zeros(N, bool)
    th_orb_dist = (TH_HIGH + TH_LOW) // 2
    n_rows = pyr_left[0].shape[0] - 2 * EDGE

    # :510-528 row table
    x_r = np.asarray(kps_r["x"], _F) if Nr else np.zeros(0, _F)
    oct_r = np.asarray(kps_r["octave"], np.int32) if Nr else np.zeros(0, np.int32)
    rows = [[] for _ in range(n_rows)]
    for i_r in range(Nr):
        kp_y = _F(kps_r["y"][i_r])
        r = _F(2.0) * scale[oct_r[i_r]]
        maxr = int(math.ceil(float(kp_y + r)))
        minr = int(math.floor(float(kp_y - r)))
        for yi in range(minr, maxr + 1):
            rows[yi].append(i_r)  # (an IndexError here: the keypoint is illegal for the reference)
    rows = [np.asarray(v, np.int64) for v in rows]

    # :531-533
    bf = _F(bf)
    mb = bf / _F(fx)
    min_z = mb
    min_d = _F(0)
    max_d = bf / min_z

    w, L = 5, 5
    accepted = []  # vDistIdx
    for i_l in range(N):
        level_l = int(kps_l["octave"][i_l])
        v_l = _F(kps_l["y"][i_l])
        u_l = _F(kps_l["x"][i_l])
        cand = rows[int(v_l)]
        if len(cand) == 0:
            continue
        min_u = u_l - max_d
        max_u = u_l - min_d
        if max_u < 0:
            continue
        # :563-584 ascending iR, strict '<' from TH_HIGH: the first of the smallest distances
        best_dist, best_idx_r = TH_HIGH, 0
        o = oct_r[cand]
        xr = x_r[cand]
        sel = cand[(o >= level_l - 1) & (o <= level_l + 1) & (xr >= min_u) & (xr <= max_u)]
        if len(sel):
            d = _POPC[np.bitwise_xor(desc_r[sel], desc_l[i_l])].sum(1)
            k = int(np.argmin(d))  # first occurrence of the minimum
            if d[k] < best_dist:
                best_dist, best_idx_r = int(d[k]), int(sel[k])
        if not best_dist < th_orb_dist:
            outcome[i_l] = HAMMING_REJECT
            continue
        idx_r[i_l] = best_idx_r
        # :590-594
        u_r0 = x_r[best_idx_r]
        sf = inv_scale[level_l]
        scaled_ul = _F(c_round(u_l * sf))
        scaled_vl = _F(c_round(v_l * sf))
        scaled_ur0 = _F(c_round(u_r0 * sf))
        pl, pr = pyr_left[level_l], pyr_right[level_l]
        cols = pr.shape[1] - 2 * EDGE
        # :598-600 (the patch is cut before the window test, as in the reference)
        y0 = int(scaled_vl) - w + EDGE
        xl0 = int(scaled_ul) - w + EDGE
        assert 0 <= y0 and y0 + 2 * w + 1 <= pl.shape[0] and 0 <= xl0 and xl0 + 2 * w + 1 <= pl.shape[1], \
            f"left keypoint {i_l}: patch outside the padded level"
        il = pl[y0:y0 + 2 * w + 1, xl0:xl0 + 2 * w + 1].astype(np.int32)
        il = il - il[w, w]
        # :608-611
        iniu = scaled_ur0 + _F(L) - _F(w)
        endu = scaled_ur0 + _F(L) + _F(w) + _F(1)
        if iniu < 0 or endu >= cols:
            outcome[i_l] = WINDOW_OFF_LEVEL
            continue
        # :613-627
        xr0 = int(scaled_ur0) - L - w + EDGE
        strip = pr[y0:y0 + 2 * w + 1, xr0:xr0 + 2 * (L + w) + 1].astype(np.int32)
        best_sad, best_inc = 2147483647, 0
        v_dists = np.zeros(2 * L + 1, _F)
        for inc in range(-L, L + 1):
            ir = strip[:, L + inc:L + inc + 2 * w + 1]
            ir = ir - ir[w, w]
            dist = _F(np.abs(il - ir).sum())
            if dist < _F(best_sad):
                best_sad, best_inc = int(dist), inc
            v_dists[L + inc] = dist
        shift[i_l], sad[i_l] = best_inc, best_sad
        if best_inc == -L or best_inc == L:
            outcome[i_l] = SHIFT_AT_END
            continue
        # :633-640
        dist1, dist2, dist3 = v_dists[L + best_inc - 1], v_dists[L + best_inc], v_dists[L + best_inc + 1]
        delta_r = (dist1 - dist3) / (_F(2.0) * (dist1 + dist3 - _F(2.0) * dist2))
        assert -1 <= delta_r <= 1, "see the module docstring"
        # :643-657
        best_ur = scale[level_l] * (scaled_ur0 + _F(best_inc) + delta_r)
        disparity = u_l - best_ur
        if disparity >= min_d and disparity < max_d:
            if disparity <= 0:
                disparity = _F(0.01)
                best_ur = _F(float(u_l) - 0.01)
                clamped[i_l] = True
            depth[i_l] = bf / disparity
            u_right[i_l] = best_ur
            accepted.append((best_sad, i_l))
            outcome[i_l] = ACCEPTED_CLAMP if clamped[i_l] else ACCEPTED
        else:
            outcome[i_l] = DISPARITY_NEG if disparity < min_d else DISPARITY_MAX

    median = th_dist = _F(np.nan)
    if accepted:  # P9: nothing accepted -> no filtering
        accepted.sort()
        median = _F(accepted[len(accepted) // 2][0])
        th_dist = _F(1.5) * _F(1.4) * median
        for s, i_l in reversed(accepted):
            if _F(s) < th_dist:
                break
            u_right[i_l] = -1
            depth[i_l] = -1
            outcome[i_l] = CULLED
    return StereoResult(u_right, depth, outcome, idx_r, shift, sad, median, th_dist, clamped)


def census(res: StereoResult) -> dict:
    """Keypoints per outcome name, plus the median, thDist and the largest SAD."""
    out = {OUTCOME_NAMES[c]: int((res.outcome == c).sum()) for c in range(len(OUTCOME_NAMES))}
    out["median"] = float(res.median)
    out["th_dist"] = float(res.th_dist)
    out["max_sad"] = int(res.sad.max()) if len(res.sad) else -1
    return out
