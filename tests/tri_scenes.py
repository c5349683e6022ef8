"""Crafted keyframe pairs for CreateNewMapPoints' device code (k_tri_match, k_triangulate[_par],
tri_geom.h), built array by array: no image, no extraction.

Descriptors: a random 256-bit base per cluster and candidates made by flipping an exact number of
its bits, so every Hamming distance <= 50 in a scene is one the scene placed (random 256-bit
strings lie around 128 apart; the census of tests/test_tri_edges_cpu.py counts the candidates).

Search scenes: keyframe 2 stands one metre ahead of keyframe 1 with the same orientation, so the
epipole is the principal point and the epipolar line of a keypoint on the row y = cy is that row:
a candidate on the row passes CheckDistEpipolarLine with distance 0, one `d` pixels off it has
squared distance d^2 against 3.84 * scale[octave]^2.  Keypoints are stereo (the mono/mono epipole
test does not apply) and sit at (cx + 200, cy) unless a scene says otherwise.

Every scene is a Scene: kf1 / has1 / fv1, the neighbours nbs = [(kf2, has2, fv2, F12), ...], the
(only_stereo, check_ori) settings to run, and `designed`: what the scene was built to produce.
"""
import functools

import numpy as np

f32 = np.float32


def _cam():
    from orb_slam2_with_comment_amd import synth
    return synth.KITTI


def _tcw(x=0.0, z=0.0, yaw=0.0):
    """Tcw of a camera at (x, 0, z) turned by yaw about the vertical axis."""
    c, s = np.cos(yaw), np.sin(yaw)
    Twc = np.eye(4)
    Twc[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    Twc[:3, 3] = (x, 0.0, z)
    return np.linalg.inv(Twc).astype(f32)


def compute_f12(T1, T2, cam):
    from tri_scenario import compute_f12 as f
    return f(T1, T2, cam)


def flip(rng, base, k, among=None):
    """base with exactly k of its 256 bits flipped (chosen among the bit indices `among`)."""
    bits = np.unpackbits(np.asarray(base, np.uint8))
    where = rng.choice(256 if among is None else np.asarray(among), size=k, replace=False)
    bits[where] ^= 1
    return np.packbits(bits)


def rand_desc(rng):
    return rng.integers(0, 256, 32, dtype=np.uint8)


class Builder:
    """One keyframe, keypoint by keypoint; a keypoint's vocabulary node is given with it and the
    FeatureVector lists each node's keypoints in the order they were added."""

    def __init__(self, tcw, cam=None):
        self.cam = cam or _cam()
        self.tcw = tcw
        self.rows, self.desc, self.ur, self.has, self.nodes = [], [], [], [], {}

    def add(self, node, desc, x=None, y=None, octave=0, angle=0.0, stereo=True, has_mp=0, ur=None):
        x = self.cam.cx + 200.0 if x is None else x
        y = self.cam.cy if y is None else y
        i = len(self.rows)
        self.rows.append((x, y, 31.0, angle, 1.0, octave, -1))
        self.desc.append(np.asarray(desc, np.uint8))
        self.ur.append((x - 20.0 if stereo else -1.0) if ur is None else ur)
        self.has.append(has_mp)
        if node is not None:
            self.nodes.setdefault(int(node), []).append(i)
        return i

    def finish(self):
        from orb_slam2_with_comment_amd.types import KP_DTYPE, FeatureVector, Frame
        keys = np.array(self.rows, KP_DTYPE) if self.rows else np.zeros(0, KP_DTYPE)
        desc = np.array(self.desc, np.uint8).reshape(-1, 32)
        fr = Frame(keys, desc, np.array(self.ur, f32), self.tcw, self.cam)
        ids = sorted(self.nodes)
        off = np.concatenate([[0], np.cumsum([len(self.nodes[k]) for k in ids])]).astype(np.int32)
        feat = np.array([i for k in ids for i in self.nodes[k]], np.int32)
        fv = FeatureVector.from_csr(np.array(ids, np.uint32), off, feat)
        return fr, np.array(self.has, np.uint8), fv


class Scene:
    def __init__(self, name, kf1, nbs, settings, designed, doc):
        self.name, self.doc = name, doc
        self.kf1, self.has1, self.fv1 = kf1
        self.nbs = nbs  # [(kf2, has2, fv2, F12)]
        self.settings = settings  # [(only_stereo, check_ori)]
        self.designed = designed


T1 = _tcw()
T2 = _tcw(z=1.0)


def _F():
    return compute_f12(T1, T2, _cam())


def _fill(rng, B, node, slots, nf):
    """Adds a KF2 node of nf keypoints in position order: slots[pos] = dict of Builder.add
    arguments, every other position a random descriptor."""
    for p in range(nf):
        kw = slots.get(p) or dict(desc=rand_desc(rng))
        B.add(node, **kw)


NODE_SIZES = (1, 63, 64, 65, 127, 128, 129, 192, 255, 256, 257, 320, 400)
NODE_TARGETS = (0, 63, 64, 127, 128, 191, 192, 255, 256)


def node_sizes():
    """Every KF2 node size around the 128 / 256 thresholds of k_tri_match's three paths.  Each
    node has one KF1 feature per target position (0, 63, 64, 127, 128, 191, 192, 255, 256, nf - 1
    where they exist) whose unique best candidate (distance 10) sits there, beside a worse one
    (distance 30) elsewhere; the nodes of 128 and of 256 have one KF1 feature for EVERY position,
    so every lane and every register slot of tri_node_regs<2> and <4> wins once, and their KF1
    lists (128, 256 features) need the second and later 64-feature chunks.  The memory path's
    strided loop wins at its first and last position."""
    rng = np.random.default_rng(101)
    A, B = Builder(T1), Builder(T2)
    winners = {}
    for k, nf in enumerate(NODE_SIZES):
        node = 10 + k
        sweep = nf in (128, 256)
        targets = list(range(nf)) if sweep else sorted({p for p in NODE_TARGETS + (nf - 1,) if p < nf})
        free = [p for p in range(nf) if p not in targets]
        slots = {}
        for p in targets:
            base = rand_desc(rng)
            i1 = A.add(node, base)
            slots[p] = dict(desc=flip(rng, base, 10))
            if free:
                slots[free.pop(len(free) // 2)] = dict(desc=flip(rng, base, 30))
            winners[i1] = (node, p)
        _fill(rng, B, node, slots, nf)
    fr2, has2, fv2 = B.finish()
    return Scene("node_sizes", A.finish(), [(fr2, has2, fv2, _F())], [(False, False), (False, True)],
                 dict(winners=winners), node_sizes.__doc__)


TIE_NODES = ((100, 1), (200, 2), (300, 4))  # (KF2 node size, slots between the two tied lanes)


def ties():
    """The tie rule (the LAST candidate of equal distance that passes wins; key dist << 32 | ~pos)
    in a node of each path (100, 200 and 300 KF2 features).  Per node: (a) two tied candidates in
    the same lane, different register slots (positions 5 and 5 + 64 k); (b) three in different
    lanes of one slot (10, 20, 30); (c) three at the first, a middle and the last position;
    (d) tied at 12, 50 and 80 where 80 fails the epipolar-line test: 50 wins; (e) a smaller
    distance at 15 that fails the line test must not block 33; (f) a lone candidate at distance
    exactly 50 is accepted, (g) one at 51 is not; (h) the best candidate (position 7) has a map
    point: 44 wins; (i) a KF1 feature with a map point is not matched."""
    rng = np.random.default_rng(202)
    cam = _cam()
    A, B = Builder(T1), Builder(T2)
    winners, unmatched, tied = {}, [], []
    off_line = cam.cy + 3.0
    for k, (nf, step) in enumerate(TIE_NODES):
        node = 40 + k
        slots = {}

        def query(cands, win, has_mp=0, is_tie=False):
            base = rand_desc(rng)
            i1 = A.add(node, base, has_mp=has_mp)
            for pos, dist, kw in cands:
                assert pos not in slots
                slots[pos] = dict(desc=flip(rng, base, dist), **kw)
            if win is None:
                unmatched.append(i1)
            else:
                winners[i1] = (node, win)
                if is_tie:
                    tied.append(i1)

        far = 5 + 64 * step
        query([(5, 20, {}), (far, 20, {})], far, is_tie=True)
        query([(10, 20, {}), (20, 20, {}), (30, 20, {})], 30, is_tie=True)
        query([(0, 18, {}), (40, 18, {}), (nf - 1, 18, {})], nf - 1, is_tie=True)
        query([(12, 22, {}), (50, 22, {}), (80, 22, dict(y=off_line))], 50, is_tie=True)
        query([(15, 10, dict(y=off_line)), (33, 25, {})], 33)
        query([(60, 50, {})], 60)
        query([(61, 51, {})], None)
        query([(7, 5, dict(has_mp=1)), (44, 30, {})], 44)
        query([(62, 8, {})], None, has_mp=1)
        _fill(rng, B, node, slots, nf)
    fr2, has2, fv2 = B.finish()
    return Scene("ties", A.finish(), [(fr2, has2, fv2, _F())], [(False, False), (False, True)],
                 dict(winners=winners, unmatched=unmatched, tied=tied), ties.__doc__)


def _mirror_nodes(rng, A, B, sizes2, n1_of, flag):
    """KF1 node k with n1_of[k] features against a KF2 node of sizes2[k]: KF1 feature i is KF2
    position (i % nf)'s descriptor with 10 bits flipped, positions counted from the node's end."""
    winners = {}
    for k, nf in enumerate(sizes2):
        node = 1 + k
        bases = [rand_desc(rng) for _ in range(nf)]
        for b in bases:
            B.add(node, b)
        for i in range(n1_of[k]):
            p = nf - 1 - (i % nf)
            h = flag(k, i)
            i1 = A.add(node, flip(rng, bases[p], 10), has_mp=h)
            if not h:
                winners[i1] = (node, p)
    return winners


def slices_one():
    """splits == 1: KF1 nodes of 64, 65, 128, 129 and 200 features are one slice each, visited in
    chunks of 64 (the second and later passes of tri_node_regs' chunk loop).  Map-point flags are
    scattered inside chunks (a sparse ballot), one whole chunk (features 64..127 of the 129 node)
    is excluded, and 20 one-feature nodes KF2 lacks keep KF1.n / nodes / 16 below 2."""
    rng = np.random.default_rng(303)
    A, B = Builder(T1), Builder(T2)
    sizes = (64, 65, 128, 129, 200)

    def flag(k, i):
        n = sizes[k]
        return int((n == 64 and i == 63) or (n == 65 and i == 64) or (n == 128 and i % 3 == 0) or
                   (n == 129 and 64 <= i < 128) or (n == 200 and i % 7 in (1, 4)))
    winners = _mirror_nodes(rng, A, B, sizes, sizes, flag)
    for k in range(20):
        A.add(100 + k, rand_desc(rng))
    fr2, has2, fv2 = B.finish()
    return Scene("slices_one", A.finish(), [(fr2, has2, fv2, _F())], [(False, False)],
                 dict(winners=winners, splits=1), slices_one.__doc__)


def slices_cap():
    """splits at its cap of 64: one KF1 node of 1030 features (1030 / 1 / 16 = 64) against a KF2
    node of 40; the slices hold 16 or 17 features (1030 is no multiple of 64)."""
    rng = np.random.default_rng(304)
    A, B = Builder(T1), Builder(T2)
    winners = _mirror_nodes(rng, A, B, (40,), (1030,), lambda k, i: int(i % 11 == 0))
    fr2, has2, fv2 = B.finish()
    return Scene("slices_cap", A.finish(), [(fr2, has2, fv2, _F())], [(False, False)],
                 dict(winners=winners, splits=64), slices_cap.__doc__)


def slices_small():
    """splits (5) above a node's size: KF1 nodes of 3 and 157 features give empty slices in the
    first and slices of 31 or 32 in the second (157 is no multiple of 5)."""
    rng = np.random.default_rng(305)
    A, B = Builder(T1), Builder(T2)
    winners = _mirror_nodes(rng, A, B, (10, 140), (3, 157), lambda k, i: 0)
    fr2, has2, fv2 = B.finish()
    return Scene("slices_small", A.finish(), [(fr2, has2, fv2, _F())], [(False, False)],
                 dict(winners=winners, splits=5), slices_small.__doc__)


def slices_batch():
    """The same KF1 (6144 keypoints in 32 nodes of 192) against 1 and against 12 neighbours in one
    batch call: the by-chip term of the slice count (4096 / (nodes * npairs)) gives 12 slices for
    one pair and 10 for twelve, and a pair's matches must not depend on it.  The neighbours share
    their keypoints (4 per node, 24 bits apart; a KF1 feature lies 6 from one and 30 from the
    other three) and differ in their map-point flags, so per pair some features fall back to the
    last of three tied candidates."""
    rng = np.random.default_rng(306)
    A, B = Builder(T1), Builder(T2)
    for k in range(32):
        node = 1 + k
        perm = rng.permutation(256)
        nodebase = rand_desc(rng)
        bases = [flip(rng, nodebase, 12, among=perm[12 * q:12 * q + 12]) for q in range(4)]
        for b in bases:
            B.add(node, b)
        for i in range(192):
            A.add(node, flip(rng, bases[i % 4], 6, among=perm[48:]))
    fr2, _, fv2 = B.finish()
    idx = np.arange(len(fr2.keys))
    nbs = [(fr2, ((idx + j) % 5 == 0).astype(np.uint8), fv2, _F()) for j in range(12)]
    return Scene("slices_batch", A.finish(), nbs, [(False, False)], dict(splits=(12, 10)), slices_batch.__doc__)


def gates():
    """The floating-point gates, one KF1 feature and one candidate per vocabulary node.
    Epipole: a candidate whose squared distance to the epipole (the principal point) is 2 % below
    or above 100 * scale[octave], at octaves 0 and 3, as mono/mono (rejected when below) and as
    mono/stereo, stereo/mono and stereo/stereo (the test must not apply).  bOnlyStereo: the same
    keypoints give a mono keypoint on either side.  Epipolar line: a stereo candidate 1.9 and 2.0
    scale[octave] pixels off the line (3.61 and 4.0 against 3.84 sigma^2) at octaves 0 and 7.  A
    second neighbour is the same keyframe with an F12 whose first two columns are zero
    (den == 0: no match at all)."""
    rng = np.random.default_rng(404)
    cam = _cam()
    A, B = Builder(T1), Builder(T2)
    sf = [float(f32(1.2) ** k) for k in range(8)]
    match = {False: [], True: []}  # designed matches by only_stereo
    node = 0
    for octave in (0, 3):
        for side, inside in ((0.99, True), (1.01, False)):
            d = side * np.sqrt(100 * sf[octave])
            for st1 in (False, True):
                for st2 in (False, True):
                    base = rand_desc(rng)
                    i1 = A.add(node, base, x=cam.cx + d, stereo=st1)
                    B.add(node, flip(rng, base, 12), x=cam.cx + d, octave=octave, stereo=st2)
                    node += 1
                    if st1 or st2 or not inside:
                        match[False].append(i1)
                    if st1 and st2:
                        match[True].append(i1)
    for octave in (0, 7):
        for off, ok in ((1.9, True), (-1.9, True), (2.0, False), (-2.0, False)):
            base = rand_desc(rng)
            i1 = A.add(node, base)
            B.add(node, flip(rng, base, 12), y=cam.cy + off * sf[octave], octave=octave)
            node += 1
            if ok:
                match[False].append(i1)
                match[True].append(i1)
    fr2, has2, fv2 = B.finish()
    F0 = _F().copy()
    F0[:, :2] = 0
    return Scene("gates", A.finish(), [(fr2, has2, fv2, _F()), (fr2, has2, fv2, F0)],
                 [(False, False), (True, False)], dict(match=match, no_match_nb=1), gates.__doc__)


def _merge(name, ids1, ids2, doc):
    rng = np.random.default_rng(505)
    A, B = Builder(T1), Builder(T2)
    winners = {}
    for node in sorted(set(ids1) | set(ids2)):
        base = rand_desc(rng)
        if node in ids1:
            i1 = A.add(node, base)
            if node in ids2:
                winners[i1] = (node, 1)
        if node in ids2:
            B.add(node, rand_desc(rng))
            B.add(node, flip(rng, base, 9))
    kf1, (fr2, has2, fv2) = A.finish(), B.finish()
    E = Builder(T2)
    for i in range(len(fr2.keys)):
        E.add(None, fr2.desc[i])
    fre, hase, fve = E.finish()  # the same keypoints, a FeatureVector without nodes
    return Scene(name, kf1, [(fr2, has2, fv2, _F()), (fre, hase, fve, _F())], [(False, False)],
                 dict(winners=winners, no_match_nb=1), doc)


MERGE_A = ((1, 2, 3, 5, 6, 8, 9, 10, 20, 21), (3, 4, 5, 6, 7, 8, 10))


def merge_a():
    """The FeatureVector merge: KF1 nodes KF2 lacks at the start (1, 2), in the middle (9) and at
    the end (20, 21) of the id range, KF2 nodes KF1 lacks in the middle (4, 7); a second neighbour
    whose fv2 has no nodes."""
    return _merge("merge_a", *MERGE_A, merge_a.__doc__)


def merge_b():
    """The converse of merge_a: KF2 nodes KF1 lacks at the start, in the middle and at the end."""
    return _merge("merge_b", MERGE_A[1], MERGE_A[0], merge_b.__doc__)


def merge_empty1():
    """fv1 without nodes (keypoints, but no FeatureVector entries): no match, no launch."""
    rng = np.random.default_rng(506)
    A, B = Builder(T1), Builder(T2)
    for k in range(5):
        base = rand_desc(rng)
        A.add(None, base)
        B.add(k, flip(rng, base, 9))
    fr2, has2, fv2 = B.finish()
    return Scene("merge_empty1", A.finish(), [(fr2, has2, fv2, _F())], [(False, False)], dict(winners={}),
                 merge_empty1.__doc__)


ROT_HISTS = ({0: 20, 3: 3, 6: 1, 9: 1}, {0: 20, 3: 3, 6: 3, 9: 1}, {0: 30, 3: 2, 6: 2, 9: 1})
ROT_KEPT = ((0, 3), (0, 3, 6), (0,))


def rotation():
    """check_ori = 1: three neighbours whose matches' angle differences fill the rotation histogram
    as {bin: matches} = ROT_HISTS, so the three-maxima rule (second and third maximum only above
    0.1 x the first) keeps bins ROT_KEPT and drops the rest.  Run singly and as pairs 0, 1, 2 of
    one batch call (the per-pair hist / bin_of rows).  One KF1 feature per vocabulary node."""
    rng = np.random.default_rng(606)
    A = Builder(T1)
    nq = max(sum(h.values()) for h in ROT_HISTS)
    bases = [rand_desc(rng) for _ in range(nq)]
    for q in range(nq):
        A.add(q, bases[q], angle=200.0)
    nbs, kept = [], []
    for h, keep in zip(ROT_HISTS, ROT_KEPT):
        B = Builder(T2)
        q, kept_q = 0, []
        for bn, cnt in h.items():
            for _ in range(cnt):
                B.add(q, flip(rng, bases[q], 11), angle=200.0 - (30.0 * bn + 5.0))
                if bn in keep:
                    kept_q.append(q)
                q += 1
        fr2, has2, fv2 = B.finish()
        nbs.append((fr2, has2, fv2, _F()))
        kept.append(kept_q)
    return Scene("rotation", A.finish(), nbs, [(False, True), (False, False)],
                 dict(kept=kept, removed=[sum(h.values()) - len(k) for h, k in zip(ROT_HISTS, kept)]),
                 rotation.__doc__)


SEARCH_SCENES = (node_sizes, ties, slices_one, slices_cap, slices_small, slices_batch, gates, merge_a, merge_b,
                 merge_empty1, rotation)


@functools.lru_cache(maxsize=None)
def search_scene(name):
    return {f.__name__: f for f in SEARCH_SCENES}[name]()


# ---- geometry and ownership ---------------------------------------------------------------------
class TriKF:
    """A keyframe for orbmi_create_new_map_points / orbmi_triangulate_matches: the Frame, its
    FeatureVector and flags, the orbmi_tri_keyframe view and the fields the reference classifier
    (tri_reference.classify_triangulation) reads."""

    def __init__(self, frame, has, fv, depth):
        from orb_slam2_with_comment_amd.types import TriKeyFrame
        self.frame, self.has, self.fv = frame, has, fv
        self.cam, self.tcw, self.keys, self.ur = frame.cam, frame.tcw, frame.keys, frame.u_right
        self.depth = np.ascontiguousarray(depth, f32)
        self.sf = frame.scale_factors
        self.sig2 = (self.sf * self.sf).astype(f32)
        c = self.cam
        self.mb = f32(f32(c.bf) / f32(c.fx))
        self.tri = TriKeyFrame(self.tcw.ctypes.data, self.keys.ctypes.data, self.ur.ctypes.data,
                               self.depth.ctypes.data, c.fx, c.fy, c.cx, c.cy, c.bf, self.mb, self.sig2.ctypes.data,
                               self.sf.ctypes.data)
        self.view = frame.view()
        self.fvv = fv.view()
        self.n = len(self.keys)

    def oracle_kf(self, O):
        c = self.cam
        return O.tri_keyframe(self.tcw, self.keys, self.ur, self.depth, c.fx, c.fy, c.cx, c.cy, c.bf, self.mb,
                              self.sig2, self.sf)


def _project(tcw, cam, X, Z):
    """Pixel column and depth of the world point (X, 0, Z) (every point lies in the plane of the
    cameras' motion, so its row is cy in every keyframe and its epipolar line is that row)."""
    p = np.asarray(tcw, np.float64) @ np.array([X, 0.0, Z, 1.0])
    return cam.fx * p[0] / p[2] + cam.cx, p[2]


class _TriBuilder(Builder):
    def __init__(self, tcw, cam):
        super().__init__(tcw, cam)
        self.depth = []

    def kp(self, node, desc, u, octave=0, stereo_z=None, dur=0.0):
        """A keypoint at column u; stereo_z = the depth its right coordinate encodes with this
        camera's bf (None: monocular), dur = an offset added to that right coordinate."""
        ur = -1.0 if stereo_z is None else u - self.cam.bf / stereo_z + dur
        i = self.add(node, desc, x=u, octave=octave, ur=ur)
        self.depth.append(-1.0 if stereo_z is None else float(f32(self.cam.bf) / (f32(u) - f32(ur))))
        return i

    def finish_tri(self):
        fr, has, fv = self.finish()
        return TriKF(fr, has, fv, self.depth)


GEOM_T2 = dict(x=-0.42, z=0.9, yaw=0.01)  # no parallax along 25 degrees left, the most at the right edge


@functools.lru_cache(maxsize=None)
def geometry():
    """One pair with K1.bf != K2.bf (K2's is 2 % smaller) in which every match is built to take one
    exit of tri::triangulate_one (names as tri_reference.EXITS).  All points lie in the plane of
    the cameras' motion (row cy everywhere), so each match passes the search's epipolar test
    whatever its columns are, and a column or right-coordinate offset steers the geometry (a
    stereo keypoint needs a right coordinate >= 0, so the stereo cases stay inside the image):
    accepted by triangulation as mono/mono, mono/stereo, stereo/mono and stereo/stereo (a point
    5 m ahead on the far side of the baseline); accepted by unprojection from KF1 (stereo/mono, a
    point one degree off the baseline's direction) and from KF2 (mono/stereo); rejected by the
    0.9998 rule (mono/mono 1.5 degrees off the baseline's direction), by cosParallaxRays <= 0 (rays more than 90 degrees apart), by
    z1 <= 0 (rays that meet behind both cameras), by z2 <= 0 (a point between the cameras), by the
    first gate as mono (unprojected from KF2, column off by 4 px) and as stereo through the right
    coordinate alone, by the second gate as mono (unprojected from KF1) and as stereo; two stereo
    second-gate matches are decided by WHICH bf the right coordinate uses (the reference's, K1's:
    one accepted that K2's would reject, one rejected that K2's would accept); scale consistency
    just outside and just inside either bound.  Not reachable from finite inputs, and so absent:
    v3 == 0 (the null vector's last component vanishes only for a point at infinity) and
    dist == 0 (a point on a camera centre has z <= 0 there)."""
    import dataclasses
    rng = np.random.default_rng(707)
    cam1 = _cam()
    cam2 = dataclasses.replace(cam1, bf=cam1.bf * 0.98)
    Ta, Tb = _tcw(), _tcw(**GEOM_T2)
    A, B = _TriBuilder(Ta, cam1), _TriBuilder(Tb, cam2)
    designed = []  # (idx1, idx2, exit)
    flips = {}

    def match(exit_, P=None, u1=None, u2=None, st1=False, st2=False, du1=0.0, du2=0.0, dur1=0.0, dur2=0.0, o1=0,
              o2=0, z2_from_bf1=True, tag=None):
        node = len(designed)
        base = rand_desc(rng)
        z1 = z2 = None
        if P is not None:
            u1, z1 = _project(Ta, cam1, *P)
            u2, z2 = _project(Tb, cam2, *P)
        # a stereo KF2 keypoint's right coordinate is consistent with the bf the second gate uses
        # (K1's) unless the case is about that difference
        s2z = None if not st2 else (z2 * cam2.bf / cam1.bf if z2_from_bf1 else z2)
        i1 = A.kp(node, base, u1 + du1, octave=o1, stereo_z=z1 if st1 else None, dur=dur1)
        i2 = B.kp(node, flip(rng, base, 10), u2 + du2, octave=o2, stereo_z=s2z, dur=dur2)
        designed.append((i1, i2, exit_))
        if tag:
            flips[tag] = len(designed) - 1

    edge, centre = (3.5, 5.0), (-2.442, 5.480)  # world (X, Z): far off the baseline / 1 degree off it
    match("tri_mm", P=edge)
    match("tri_ms", P=edge, st2=True)
    match("tri_sm", P=edge, st1=True)
    match("tri_ss", P=edge, st1=True, st2=True)
    match("unproj1", P=centre, st1=True)
    match("unproj2", P=centre, st2=True, z2_from_bf1=False)
    match("low_parallax_mono", P=(-2.791, 6.419))  # 1.5 degrees off the baseline: clear of the search's epipole test
    match("cos_nonpositive", u1=cam1.cx - 1200.0, u2=cam1.cx + 1200.0)
    match("z1", u1=cam1.cx + 127.0, u2=cam1.cx - 127.0)
    match("z2", P=(-0.1, 0.3))
    match("gate1_mono", P=centre, st2=True, z2_from_bf1=False, du1=4.0)
    match("gate1_stereo", P=edge, st1=True, dur1=4.0)
    match("gate2_mono", P=centre, st1=True, du2=4.0)
    match("gate2_stereo", P=edge, st2=True, dur2=6.0)
    # the bf rule: at 4.1 m K1's and K2's bf put the right coordinate 1.9 px apart
    match("tri_ms", P=edge, st2=True, dur2=-2.0, tag="accepted_by_bf1_only")
    match("gate2_stereo", P=edge, st2=True, dur2=3.3, tag="accepted_by_bf2_only")
    # scale consistency: dist2 / dist1 is 0.93 at `edge`; ratioFactor = 1.8
    match("scale_below", P=edge, o1=3, o2=0)
    match("tri_mm", P=edge, o1=2, o2=0, tag="inside_below")
    match("scale_above", P=edge, o1=0, o2=4)
    match("tri_mm", P=edge, o1=0, o2=3, tag="inside_above")
    K1, K2 = A.finish_tri(), B.finish_tri()
    F12 = compute_f12(Ta, Tb, cam1)
    return dict(K1=K1, K2=K2, F12=F12, designed=designed, tags=flips, doc=geometry.__doc__)


CLAIM_NPAIRS = (1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65)
CLAIM_N1 = 70


def _owner(i, npairs):
    """The pair built to own KF1 keypoint i: pair 0, a middle pair, the last pair or none (-1)."""
    return (0, npairs // 2, npairs - 1, -1)[i % 4]


@functools.lru_cache(maxsize=None)
def claims(npairs):
    """Ownership of a KF1 keypoint by the FIRST pair whose geometry accepts it
    (k_triangulate_par<G>'s ballot, k_triangulate's loop).  KF1 has 70 keypoints (no multiple of
    64 / G for any G: the last wave is partial), one per vocabulary node, every third one stereo;
    neighbour j stands at its own pose and matches keypoint i unless (i + 2 j) % 7 == 0.  By
    construction the owner of keypoint i is pair 0, pair npairs / 2, pair npairs - 1 or nobody
    (i % 4): in the pairs before the owner's the matched KF2 keypoint lies where the rays meet
    behind the cameras (rejected: match12 stays, ok = 0), from the owner on it is the point's true
    projection (accepted if it came first; later ones are dropped: match12 -> -1, ok = 0)."""
    rng = np.random.default_rng(808 + npairs)
    cam = _cam()
    Ta = _tcw()
    A = _TriBuilder(Ta, cam)
    pts, bases = [], []
    for i in range(CLAIM_N1):
        P = (-3.0 + 6.0 * i / (CLAIM_N1 - 1), 5.0 + (i % 5))
        u1, z1 = _project(Ta, cam, *P)
        bases.append(rand_desc(rng))
        A.kp(i, bases[i], u1, stereo_z=z1 if i % 3 == 0 else None)
        pts.append((P, u1))
    K1 = A.finish_tri()
    nbs, F12 = [], []
    for j in range(npairs):
        Tj = _tcw(x=0.9 + 0.02 * j, z=0.1 * (j % 3), yaw=0.004 * (j % 4))
        B = _TriBuilder(Tj, cam)
        for i in range(CLAIM_N1):
            own = _owner(i, npairs)
            if (i + 2 * j) % 7 == 0 and j != own:
                continue
            P, u1 = pts[i]
            good = own >= 0 and j >= own
            u2 = _project(Tj, cam, *P)[0] if good else u1 + 150.0
            B.kp(i, flip(rng, bases[i], 10), u2)
        nbs.append(B.finish_tri())
        F12.append(compute_f12(Ta, Tj, cam))
    return dict(K1=K1, nbs=nbs, F12=F12, owner=[_owner(i, npairs) for i in range(CLAIM_N1)])
