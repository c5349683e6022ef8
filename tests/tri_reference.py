"""A plain sequential restatement of ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:783-975)
with CheckDistEpipolarLine (:173-196) and ComputeThreeMaxima (:1854-1895), written from the
reference text, that also counts what it went through, and a classifier that names the exit
CreateNewMapPoints' per-match geometry (src/LocalMapping.cc:385-557) takes.

The search restatement keeps the reference's loop (`if(dist>TH_LOW || dist>bestDist) continue;
... if(CheckDistEpipolarLine(...)) {bestIdx2=idx2; bestDist=dist;}`) and float arithmetic
(numpy float32 scalars, one rounding per operation; the epipole's small matrix products
accumulate in double as a cv::Mat gemm does).  Beside match12 and the count it returns a census:

  cand_le50          candidates (KF1 feature, KF2 feature of the same node) at distance <= 50, flags aside
  rej_epipole        ... of them rejected by the mono/mono epipole test
  rej_line           ... by the epipolar-line distance
  rej_den0           ... by den == 0
  rej_flag2          ... skipped because the KF2 keypoint has a map point
  rej_only_stereo2   ... skipped by bOnlyStereo on the KF2 side
  skip_flag1         KF1 features of common nodes skipped because they have a map point
  skip_only_stereo1  KF1 features of common nodes skipped by bOnlyStereo
  multi_pass         KF1 features with more than one candidate passing every test
  tie_decided        KF1 features whose smallest passing distance is shared (the last one wins)
  winners            {idx1: (node id, position of the winner in the KF2 node's list)} before the
                     rotation filter
  rot_removed        matches removed by the three-maxima rule
  nodes_skipped1/2   nodes of either FeatureVector the merge passed over
  largest_slice      the largest number of KF1 features of a common node (one slice, unsplit)
  min_margin         the smallest relative distance of a floating-point decision to its threshold
"""
import numpy as np

f32 = np.float32
TH_LOW = 50
HISTO_LENGTH = 30


def _bits(desc):
    return np.unpackbits(np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), axis=1).astype(np.float32)


def hamming_matrix(d1, d2):
    b1, b2 = _bits(d1), _bits(d2)
    return (b1 @ (1 - b2).T + (1 - b1) @ b2.T).astype(np.int32)


def _rel(v, th):
    v, th = float(v), float(th)
    m = max(abs(v), abs(th))
    return abs(v - th) / m if m > 0 else 1.0


def epipole(kf1, kf2):
    """ex, ey of :790-799 (Cw = -R1w^T t1w, C2 = R2w Cw + t2w, each a float matrix product)."""
    T1, T2 = np.asarray(kf1.tcw, np.float64), np.asarray(kf2.tcw, np.float64)
    Cw = (-(T1[:3, :3].T @ T1[:3, 3])).astype(f32).astype(np.float64)
    C2 = (T2[:3, :3] @ Cw + T2[:3, 3]).astype(f32)
    with np.errstate(all="ignore"):
        invz = f32(1.0) / C2[2]
        ex = f32(kf2.cam.fx) * C2[0] * invz + f32(kf2.cam.cx)
        ey = f32(kf2.cam.fy) * C2[1] * invz + f32(kf2.cam.cy)
    return ex, ey


def three_maxima(sizes):
    """ComputeThreeMaxima on the bin sizes -> (ind1, ind2, ind3, margins)."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    margins = []
    th = f32(0.1) * f32(max1)
    if max1 > 0:
        margins.append(_rel(max2, th))
    if f32(max2) < th:
        ind2 = ind3 = -1
    else:
        if max1 > 0:
            margins.append(_rel(max3, th))
        if f32(max3) < th:
            ind3 = -1
    return ind1, ind2, ind3, margins


def search_for_triangulation(kf1, has_mp1, fv1, kf2, has_mp2, fv2, F12, only_stereo=False, check_ori=True):
    F = np.asarray(F12, f32).reshape(3, 3)
    n1 = len(kf1.keys)
    match12 = np.full(n1, -1, np.int32)
    census = dict(cand_le50=0, rej_epipole=0, rej_line=0, rej_den0=0, rej_flag2=0, rej_only_stereo2=0, skip_flag1=0,
                  skip_only_stereo1=0, multi_pass=0, tie_decided=0, winners={}, rot_removed=0, nodes_skipped1=0,
                  nodes_skipped2=0, largest_slice=0, min_margin=1.0)
    margins = []
    ex, ey = epipole(kf1, kf2)
    sf2 = np.asarray(kf2.scale_factors, f32)
    sigma2 = (sf2 * sf2).astype(f32)  # mvLevelSigma2
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    factor = f32(1.0) / f32(HISTO_LENGTH)
    nmatches = 0
    k1, k2 = kf1.keys, kf2.keys
    a = b = 0
    na, nb = len(fv1.node_id), len(fv2.node_id)
    while a < na and b < nb:
        ida, idb = int(fv1.node_id[a]), int(fv2.node_id[b])
        if ida < idb:
            census["nodes_skipped1"] += 1
            a += 1
            continue
        if ida > idb:
            census["nodes_skipped2"] += 1
            b += 1
            continue
        feat1 = fv1.feat[fv1.off[a]:fv1.off[a + 1]]
        feat2 = fv2.feat[fv2.off[b]:fv2.off[b + 1]]
        census["largest_slice"] = max(census["largest_slice"], len(feat1))
        D = hamming_matrix(kf1.desc[feat1], kf2.desc[feat2]) if len(feat1) and len(feat2) else np.zeros((0, 0), int)
        close = [np.nonzero(row <= TH_LOW)[0] for row in D]
        for p1, idx1 in enumerate(feat1):
            idx1 = int(idx1)
            if has_mp1[idx1]:
                census["skip_flag1"] += 1
                continue
            st1 = kf1.u_right[idx1] >= 0
            if only_stereo and not st1:
                census["skip_only_stereo1"] += 1
                continue
            kp1 = k1[idx1]
            la = kp1["x"] * F[0, 0] + kp1["y"] * F[1, 0] + F[2, 0]
            lb = kp1["x"] * F[0, 1] + kp1["y"] * F[1, 1] + F[2, 1]
            lc = kp1["x"] * F[0, 2] + kp1["y"] * F[1, 2] + F[2, 2]
            best_dist, best_idx2, best_pos = TH_LOW, -1, -1
            passing = []
            for p2 in close[p1]:
                idx2 = int(feat2[p2])
                dist = int(D[p1, p2])
                census["cand_le50"] += 1
                if has_mp2[idx2]:
                    census["rej_flag2"] += 1
                    continue
                st2 = kf2.u_right[idx2] >= 0
                if only_stereo and not st2:
                    census["rej_only_stereo2"] += 1
                    continue
                kp2 = k2[idx2]
                ok = True
                if not st1 and not st2:
                    dx, dy = ex - kp2["x"], ey - kp2["y"]
                    with np.errstate(all="ignore"):
                        d2 = dx * dx + dy * dy
                    th = f32(100) * sf2[kp2["octave"]]
                    if np.isfinite(d2):
                        margins.append(_rel(d2, th))
                    if d2 < th:
                        census["rej_epipole"] += 1
                        ok = False
                if ok:
                    num = la * kp2["x"] + lb * kp2["y"] + lc
                    den = la * la + lb * lb
                    if den == 0:
                        census["rej_den0"] += 1
                        ok = False
                    else:
                        dsqr = num * num / den
                        th = 3.84 * float(sigma2[kp2["octave"]])
                        margins.append(_rel(dsqr, th))
                        if not float(dsqr) < th:
                            census["rej_line"] += 1
                            ok = False
                if ok:
                    passing.append((dist, int(p2)))
                # the reference's scan: a candidate above bestDist is not looked at; one that
                # passes becomes the best, ties included
                if dist > TH_LOW or dist > best_dist:
                    continue
                if ok:
                    best_idx2, best_dist, best_pos = idx2, dist, int(p2)
            if len(passing) > 1:
                census["multi_pass"] += 1
                dmin = min(d for d, _ in passing)
                if sum(d == dmin for d, _ in passing) > 1:
                    census["tie_decided"] += 1
            if best_idx2 >= 0:
                match12[idx1] = best_idx2
                census["winners"][idx1] = (ida, best_pos)
                nmatches += 1
                if check_ori:
                    rot = kp1["angle"] - k2[best_idx2]["angle"]
                    if rot < 0.0:
                        rot = rot + f32(360.0)
                    v = float(rot * factor)
                    margins.append(min(1.0, abs(abs(v - np.floor(v)) - 0.5)))
                    bn = int(np.floor(v + 0.5))  # round(), v >= 0
                    if bn == HISTO_LENGTH:
                        bn = 0
                    rot_hist[bn].append(idx1)
        a += 1
        b += 1
    census["nodes_skipped1"] += na - a
    census["nodes_skipped2"] += nb - b
    if check_ori:
        i1, i2, i3, mg = three_maxima([len(h) for h in rot_hist])
        margins += mg
        for i in range(HISTO_LENGTH):
            if i in (i1, i2, i3):
                continue
            for idx1 in rot_hist[i]:
                match12[idx1] = -1
                nmatches -= 1
                census["rot_removed"] += 1
    census["min_margin"] = min(margins) if margins else 1.0
    return match12, nmatches, census


# ---- CreateNewMapPoints' geometry: which exit a match takes ------------------------------------
EXITS = ("tri_mm", "tri_ms", "tri_sm", "tri_ss", "unproj1", "unproj2", "low_parallax_mono", "cos_nonpositive",
         "no_branch", "v3_zero", "z1", "z2", "gate1_mono", "gate1_stereo", "gate2_mono", "gate2_stereo", "dist_zero",
         "scale_below", "scale_above")


def _mm(A, B):
    return (np.asarray(A, np.float64) @ np.asarray(B, np.float64)).astype(f32)


def classify_triangulation(K1, K2, i1, i2, bf2_in_gate2=False):
    """src/LocalMapping.cc:385-557 for the match (i1 of K1, i2 of K2) -> (accepted, exit, info).
    K: an object with tcw (4x4 float32), cam (fx fy cx cy bf), keys, ur, depth, sf (scale factors)
    and sig2 (level sigma^2).  exit names the branch that produced the point when accepted, else
    the test that rejected it.  info: gate1 / gate2 = (error, threshold) where reached, and
    right_only = the first gate failed through the right coordinate alone.  bf2_in_gate2 = True
    evaluates the second keyframe's right coordinate with ITS mbf (what the reference does not
    do, :530) to tell which matches that rule decides."""
    c1, c2 = K1.cam, K2.cam
    info = {}
    Rcw1, tcw1 = K1.tcw[:3, :3], K1.tcw[:3, 3]
    Rcw2, tcw2 = K2.tcw[:3, :3], K2.tcw[:3, 3]
    Rwc1, Rwc2 = Rcw1.T.copy(), Rcw2.T.copy()
    Ow1, Ow2 = -_mm(Rwc1, tcw1), -_mm(Rwc2, tcw2)
    kp1, kp2 = K1.keys[i1], K2.keys[i2]
    ur1, ur2 = K1.ur[i1], K2.ur[i2]
    st1, st2 = bool(ur1 >= 0), bool(ur2 >= 0)
    inv = lambda x: f32(f32(1.0) / f32(x))  # noqa: E731
    xn1 = np.array([(kp1["x"] - f32(c1.cx)) * inv(c1.fx), (kp1["y"] - f32(c1.cy)) * inv(c1.fy), 1], f32)
    xn2 = np.array([(kp2["x"] - f32(c2.cx)) * inv(c2.fx), (kp2["y"] - f32(c2.cy)) * inv(c2.fy), 1], f32)
    r1, r2 = _mm(Rwc1, xn1).astype(np.float64), _mm(Rwc2, xn2).astype(np.float64)
    cpr = f32(r1 @ r2 / (np.sqrt(r1 @ r1) * np.sqrt(r2 @ r2)))
    cps1 = cps2 = f32(cpr + f32(1))
    if st1:
        mb = f32(f32(c1.bf) / f32(c1.fx))
        cps1 = f32(np.cos(2 * np.arctan2(np.float64(mb) / 2, np.float64(K1.depth[i1]))))
    elif st2:
        mb = f32(f32(c2.bf) / f32(c2.fx))
        cps2 = f32(np.cos(2 * np.arctan2(np.float64(mb) / 2, np.float64(K2.depth[i2]))))
    cps = min(cps1, cps2)
    if cpr < cps and cpr > 0 and (st1 or st2 or cpr < 0.9998):
        T1, T2 = K1.tcw, K2.tcw
        A = np.stack([xn1[0] * T1[2] - T1[0], xn1[1] * T1[2] - T1[1],
                      xn2[0] * T2[2] - T2[0], xn2[1] * T2[2] - T2[1]]).astype(f32)
        _, _, vt = np.linalg.svd(A.astype(np.float64))
        x = vt[3].astype(f32)
        if x[3] == 0:
            return False, "v3_zero", info
        x = (x[:3] / x[3]).astype(f32)
        src = "tri_" + "ms"[st1] + "ms"[st2]
    elif st1 and cps1 < cps2:
        zz = K1.depth[i1]
        xc = np.array([(kp1["x"] - f32(c1.cx)) * zz * inv(c1.fx), (kp1["y"] - f32(c1.cy)) * zz * inv(c1.fy), zz], f32)
        x = (Rwc1.astype(np.float64) @ xc.astype(np.float64) + Ow1.astype(np.float64)).astype(f32)
        src = "unproj1"
    elif st2 and cps2 < cps1:
        zz = K2.depth[i2]
        xc = np.array([(kp2["x"] - f32(c2.cx)) * zz * inv(c2.fx), (kp2["y"] - f32(c2.cy)) * zz * inv(c2.fy), zz], f32)
        x = (Rwc2.astype(np.float64) @ xc.astype(np.float64) + Ow2.astype(np.float64)).astype(f32)
        src = "unproj2"
    else:
        if not (cpr > 0):
            return False, "cos_nonpositive", info
        if not st1 and not st2:
            return False, "low_parallax_mono", info
        return False, "no_branch", info
    info["x"] = x
    xd = x.astype(np.float64)
    z1 = f32(Rcw1[2].astype(np.float64) @ xd + np.float64(tcw1[2]))
    if z1 <= 0:
        return False, "z1", info
    z2 = f32(Rcw2[2].astype(np.float64) @ xd + np.float64(tcw2[2]))
    if z2 <= 0:
        return False, "z2", info
    for g, (K, R, t, z, kp, ur, st) in enumerate(((K1, Rcw1, tcw1, z1, kp1, ur1, st1),
                                                  (K2, Rcw2, tcw2, z2, kp2, ur2, st2))):
        cam = K.cam
        s2 = K.sig2[kp["octave"]]
        xx = f32(R[0].astype(np.float64) @ xd + np.float64(t[0]))
        yy = f32(R[1].astype(np.float64) @ xd + np.float64(t[1]))
        iz = f32(1.0 / np.float64(z))
        uu = f32(cam.fx) * xx * iz + f32(cam.cx)
        vv = f32(cam.fy) * yy * iz + f32(cam.cy)
        ex, ey = uu - kp["x"], vv - kp["y"]
        e2 = ex * ex + ey * ey
        if not st:
            th = 5.991 * float(s2)
            info[f"gate{g + 1}"] = (float(e2), th)
            if float(e2) > th:
                return False, f"gate{g + 1}_mono", info
        else:
            # the right coordinate uses the FIRST keyframe's mbf in both gates (:500, :530)
            bf = K2.cam.bf if (g == 1 and bf2_in_gate2) else K1.cam.bf
            er = (uu - f32(bf) * iz) - ur
            th = 7.8 * float(s2)
            info[f"gate{g + 1}"] = (float(e2 + er * er), th)
            if float(e2 + er * er) > th:
                info["right_only"] = not float(e2) > th
                return False, f"gate{g + 1}_stereo", info
    n1, n2 = (x - Ow1).astype(np.float64), (x - Ow2).astype(np.float64)
    d1, d2 = f32(np.sqrt(n1 @ n1)), f32(np.sqrt(n2 @ n2))
    if d1 == 0 or d2 == 0:
        return False, "dist_zero", info
    rd = d2 / d1
    ro = K1.sf[kp1["octave"]] / K2.sf[kp2["octave"]]
    rf = f32(1.5) * K1.sf[1]
    info["scale"] = (float(rd * rf), float(ro), float(rd), float(ro * rf))
    if rd * rf < ro:
        return False, "scale_below", info
    if rd > ro * rf:
        return False, "scale_above", info
    return True, src, info
