"""Seeded scenes for Frame::ComputeStereoMatches (tests/test_stereo_cpu.py, test_stereo_gpu.py).

A scene is an image pair, a pyramid setting, bf / fx and one or more keypoint sets ("variants"):
either the extractor's own keypoints or crafted ones, which the GPU tests put in front of the
stereo kernels with orbmi_debug_set_keypoints after extracting the images once.  Everything is
generated; nothing is read from disk.

Crafted keypoints are legal for the reference: the octave lies inside the level count, x and y lie
inside the image and y +- 2 * scale[octave] lies inside [0, rows - 1] (`check_legal`).

Each variant carries the census it must meet on the numpy restatement's outcome codes
(`need`: outcome -> least count) and, where the construction fixes them, the right keypoint a
left keypoint must choose (`chosen`) and the outcomes it may end in (`allowed`).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import stereo_reference as SR

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
_F = np.float32


@dataclass
class Variant:
    name: str
    kps: tuple | None            # (kps_l, desc_l, kps_r, desc_r), or None: the extractor's own keypoints
    need: dict = field(default_factory=dict)      # outcome code -> least number of keypoints
    chosen: dict = field(default_factory=dict)    # left index -> right index it must choose
    allowed: dict = field(default_factory=dict)   # left index -> set of outcomes it may end in
    median: tuple | None = None  # (lo, hi): the median must lie in [lo, hi]
    rows_per_keypoint: int | None = None  # pyramid_top: rows every right keypoint enters
    tail_from: int | None = None  # counts: first left index beyond k_stereo_filter's registers


@dataclass
class Scene:
    name: str
    left: np.ndarray
    right: np.ndarray
    bf: float
    fx: float
    variants: list
    nfeatures: int = 500
    scale_factor: float = 1.2
    nlevels: int = 8
    capacity: int | None = None  # orbmi_extract capacity (default: the Python mirror's)


def scale_tables(scale_factor, nlevels):
    """mvScaleFactor / mvInvScaleFactor (src/ORBextractor.cc:418-432), for placing keypoints; the
    tests read the tables they compute with from the oracle and assert they equal these."""
    s = np.ones(nlevels, _F)
    for i in range(1, nlevels):
        s[i] = _F(float(s[i - 1]) * float(_F(scale_factor)))
    return s, (_F(1.0) / s).astype(_F)


def level_width(cols, inv_scale_l):
    """cvRound(cols * inv_scale) (src/ORBextractor.cc:1111): round half to even."""
    return int(np.rint(_F(cols) * _F(inv_scale_l)))


def texture(rng, rows, cols, lo=40, hi=150):
    """Noise at several scales, values in [lo, hi]: every 11 x 11 patch of every level has a
    distinct SAD minimum, and a bump of up to 100 grey levels does not clip."""
    t = np.zeros((rows, cols))
    for cell, wgt in ((1, 1.0), (2, 1.0), (4, 1.5), (8, 2.0), (16, 2.0)):
        n = rng.uniform(-1, 1, (rows // cell + 2, cols // cell + 2))
        t += wgt * np.kron(n, np.ones((cell, cell)))[:rows, :cols]
    t = (t - t.min()) / (t.max() - t.min())
    return (lo + t * (hi - lo)).astype(np.uint8)


def shifted(left, d):
    """right[y, x] = left[y, x + d] (wrapping): a left point at u appears at u - d."""
    return np.roll(left, -d, axis=1)


def make_kps(xs, ys, octs, scale):
    k = np.zeros(len(xs), KP_DTYPE)
    k["x"], k["y"], k["octave"] = xs, ys, octs
    k["size"] = _F(31.0) * scale[np.asarray(octs, int)] if len(xs) else 0
    k["angle"], k["response"], k["class_id"] = 0, 1, -1
    return k


def flip_bits(desc, k, rng):
    """A copy of a 32-byte descriptor at Hamming distance exactly k."""
    bits = np.unpackbits(np.asarray(desc, np.uint8))
    bits[rng.choice(256, k, replace=False)] ^= 1
    return np.packbits(bits)


def check_legal(kps, rows, cols, scale):
    o = kps["octave"]
    assert ((o >= 0) & (o < len(scale))).all()
    assert ((kps["x"] >= 0) & (kps["x"] <= cols - 1) & (kps["y"] >= 0) & (kps["y"] <= rows - 1)).all()
    r = _F(2.0) * scale[o]
    assert ((kps["y"] - r >= 0) & (kps["y"] + r <= rows - 1)).all()


class _Builder:
    """Left / right keypoint lists in index order."""

    def __init__(self, rng, scale):
        self.rng, self.scale = rng, scale
        self.l, self.r, self.dl, self.dr = [], [], [], []

    def left(self, x, y, o=0, desc=None):
        self.l.append((x, y, o))
        self.dl.append(self.rng.integers(0, 256, 32, dtype=np.uint8) if desc is None else desc)
        return len(self.l) - 1

    def right(self, x, y, o=0, desc=None, of=None, ham=0):
        """desc, or a copy of left keypoint `of`'s descriptor at Hamming distance `ham`."""
        if desc is None:
            desc = (flip_bits(self.dl[of], ham, self.rng) if of is not None
                    else self.rng.integers(0, 256, 32, dtype=np.uint8))
        self.r.append((x, y, o))
        self.dr.append(desc)
        return len(self.r) - 1

    def arrays(self, rows, cols):
        out = []
        for pts, ds in ((self.l, self.dl), (self.r, self.dr)):
            a = np.asarray(pts, np.float64).reshape(-1, 3)
            k = make_kps(a[:, 0].astype(_F), a[:, 1].astype(_F), a[:, 2].astype(np.int32), self.scale)
            check_legal(k, rows, cols, self.scale)
            out += [k, np.asarray(ds, np.uint8).reshape(-1, 32)]
        return tuple(out)


# ---- 1. branches ------------------------------------------------------------------------
@functools.lru_cache(None)
def branches(seed=3):
    """Every way out of the per-keypoint loop, the inclusive search bounds, the octave window,
    the Hamming threshold, ties, a crowded row, the level's right edge, the 0.01 clamp and the
    disparity bounds; maxD = 40.  Rows 0-129 have a true disparity of 20, rows 130-189 of 40,
    rows 190-299 of 0; the right image carries noise of +-2 so that the SADs and their median
    are positive, except on the mirror-symmetric patches."""
    rng = np.random.default_rng(seed)
    rows, cols = 300, 400
    scale, inv = scale_tables(1.2, 8)
    L = texture(rng, rows, cols)
    sym = []  # (x, y) of the mirror-symmetric patches, painted before the right image is cut
    b = _Builder(rng, scale)
    v = Variant("crafted", None)
    A = lambda k: (60 + 60 * (k % 5), 12 + 12 * (k // 5))    # rows 12..96, d = 20
    B = lambda k: (60 + 60 * (k % 5), 142 + 12 * (k // 5))   # rows 142..178, d = 40
    C = lambda k: (60 + 60 * (k % 5), 204 + 12 * (k // 5))   # rows 204..264, d = 0
    past_hamming = {SR.WINDOW_OFF_LEVEL, SR.SHIFT_AT_END, SR.DISPARITY_NEG, SR.DISPARITY_MAX, SR.ACCEPTED,
                    SR.ACCEPTED_CLAMP, SR.CULLED}
    k = 0
    # plain matches: they carry the median
    for _ in range(10):
        x, y = A(k); k += 1
        i = b.left(x, y)
        v.chosen[i] = b.right(x - 20, y, of=i, ham=10)
    # best Hamming distance exactly 74 (passes), 75 and 110 (rejected)
    for ham in (74, 75, 110) * 3:
        x, y = A(k); k += 1
        i = b.left(x, y)
        b.right(x - 20, y, of=i, ham=ham)
        v.allowed[i] = past_hamming if ham == 74 else {SR.HAMMING_REJECT}
    # Hamming ties: the lowest right index wins; the other one sits 6 px off the match
    for first_true in (True, False, True, False):
        x, y = A(k); k += 1
        i = b.left(x, y)
        r0 = b.right(x - 20 if first_true else x - 26, y, of=i, ham=30)
        b.right(x - 26 if first_true else x - 20, y, of=i, ham=30)
        v.chosen[i] = r0
    # octaves: candidates two levels away are skipped although their descriptors are closest
    for near in (1, 3, 1, 3, 1, 3):
        x, y = A(k); k += 1
        i = b.left(x, y, 2)
        b.right(x - 26, y, 0, of=i, ham=5)
        b.right(x - 14, y, 4, of=i, ham=5)
        v.chosen[i] = b.right(x - 20, y, near, of=i, ham=20)
    for far in (2, 2, 3):
        x, y = A(k); k += 1
        i = b.left(x, y, 0)
        b.right(x - 20, y, far, of=i, ham=5)
        v.allowed[i] = {SR.HAMMING_REJECT}
    # the right keypoint 5 px off the match: the best shift is -L / +L
    for off in (5, -5, 5, -5):
        x, y = A(k); k += 1
        i = b.left(x, y)
        b.right(x - 20 + off, y, of=i, ham=10)
        v.allowed[i] = {SR.SHIFT_AT_END}
    heavy = []
    for _ in range(4):  # a heavily disturbed right patch: accepted, then culled
        x, y = A(k); k += 1
        i = b.left(x, y)
        b.right(x - 20, y, of=i, ham=10)
        heavy.append((x - 20, y))
        v.allowed[i] = {SR.CULLED}
    assert k <= 40
    # a crowded row: 100 right keypoints in range of one left keypoint, four of them tied at the
    # smallest distance, more than 64 list positions apart
    for y, true_first in ((112, True), (124, False)):
        i = b.left(200, y)
        for j in range(100):
            xj = 160 + 40 * j / 99
            if j == 3:
                xj = 180 if true_first else 173
            if j in (40, 70, 95):
                xj = 173 if true_first else 180
            r = b.right(xj, y, of=i, ham=12 if j in (3, 40, 70, 95) else 60 + j % 40)
            if j == 3:
                v.chosen[i] = r
        if true_first:
            v.allowed[i] = past_hamming - {SR.SHIFT_AT_END}
    # uR exactly uL - maxD: inside the search range; the parabola puts the disparity just under
    # or just at / over maxD
    k = 0
    for _ in range(20):
        x, y = B(k); k += 1
        i = b.left(x, y)
        v.chosen[i] = b.right(x - 40, y, of=i, ham=10)
        v.allowed[i] = {SR.DISPARITY_MAX, SR.ACCEPTED, SR.CULLED}
    # uR exactly uL: the disparity falls just under or just over 0 ...
    k = 0
    for _ in range(16):
        x, y = C(k); k += 1
        i = b.left(x, y)
        v.chosen[i] = b.right(x, y, of=i, ham=10)
        v.allowed[i] = {SR.DISPARITY_NEG, SR.ACCEPTED, SR.CULLED}
    # ... or is exactly 0 on a patch that is mirror-symmetric about the keypoint's column
    for _ in range(4):
        x, y = C(k); k += 1
        sym.append((x, y))
        i = b.left(x, y)
        v.chosen[i] = b.right(x, y, of=i, ham=10)
        v.allowed[i] = {SR.ACCEPTED_CLAMP}
    # the level's right edge: round(uR * inv) = W - 12, W - 11, W - 10 puts endu at W - 1, W, W + 1
    y = 196
    for o in (0, 1, 2):
        W = level_width(cols, inv[o])
        for j, t in enumerate((W - 12, W - 11, W - 10)):
            ur = _F(t) * scale[o]
            assert SR.c_round(ur * inv[o]) == t
            i = b.left(float(ur + _F(2.0) * scale[o]), y, o)
            v.chosen[i] = b.right(float(ur), y, o, of=i, ham=10)
            v.allowed[i] = past_hamming - {SR.WINDOW_OFF_LEVEL} if j == 0 else {SR.WINDOW_OFF_LEVEL}
            y += 8
    # rows that no right band covers
    for j in range(4):
        v.allowed[b.left(100 + 50 * j, 284 + 3 * j)] = {SR.NO_CANDIDATES}

    for x, y in sym:
        L[y - 6:y + 7, x + 1:x + 14] = L[y - 6:y + 7, x - 13:x][:, ::-1]
    R = np.empty_like(L)
    R[:130], R[130:190], R[190:] = shifted(L[:130], 20), shifted(L[130:190], 40), L[190:]
    noise = rng.integers(-2, 3, R.shape)
    for x, y in sym:
        noise[y - 6:y + 7, x - 13:x + 14] = 0
    for x, y in heavy:
        noise[y - 5:y + 6, x - 5:x + 6] = rng.integers(-12, 13, (11, 11))
        noise[y, x - 5:x + 6] = 0
    R = np.clip(R.astype(int) + noise, 0, 255).astype(np.uint8)
    v.kps = b.arrays(rows, cols)
    v.need = {c: 3 for c in range(len(SR.OUTCOME_NAMES))}
    return Scene("branches", L, R, 10.0, 40.0, [v])


# ---- 2. identical -----------------------------------------------------------------------
@functools.lru_cache(None)
def identical(seed=5):
    """L == R with the extractor's own keypoints: every accepted SAD is 0, so the median and
    thDist are 0 and every accepted match is culled (x < 0 never holds)."""
    L = texture(np.random.default_rng(seed), 300, 400, 20, 230)
    v = Variant("own", None, need={SR.CULLED: 100, SR.DISPARITY_NEG: 3}, median=(0, 0))
    return Scene("identical", L, L.copy(), 10.0, 40.0, [v], nfeatures=1000)


# ---- 3. median ranks --------------------------------------------------------------------
def _bump(img, x, y, total):
    """Raise pixels of the 11 x 11 patch around (x, y), off its centre row, by `total` in all:
    with an otherwise exact copy the SAD at the matching shift is exactly `total`."""
    cells = [(dy, dx) for dy in (-4, -2, 2, 4) for dx in (-3, -1, 1, 3)]
    for dy, dx in cells:
        step = min(total, 60)
        img[y + dy, x + dx] += step
        total -= step
    assert total == 0


@functools.lru_cache(None)
def median_ranks(seed=7):
    """Exact copies at a disparity of 20 with dialled SADs m - 1, m - 1, m, m, m, m + 1, m + 1,
    floor(2.1 m), floor(2.1 m) + 1 for m = 128 and m = 256 (the SADs repeat on both sides of a
    histogram bin edge, and two sit on either side of thDist = 2.1 m), taken 0, 1, 2, 3, 8 and 9
    at a time: size/2 is the upper middle of an even count."""
    rng = np.random.default_rng(seed)
    rows, cols = 300, 400
    scale, _ = scale_tables(1.2, 8)
    L = texture(rng, rows, cols)
    R = shifted(L, 20).astype(int)
    pts = {}
    k = 0
    for m in (128, 256):
        th = int(2.1 * m)
        assert _F(th) < _F(1.5) * _F(1.4) * _F(m) <= _F(th + 1)
        for s in (m - 1, m - 1, m, m, m, m + 1, m + 1, th, th + 1):
            x, y = 60 + 60 * (k % 5), 20 + 24 * (k // 5)
            k += 1
            _bump(R, x - 20, y, s)
            pts.setdefault(m, []).append((x, y, s))
    R = R.astype(np.uint8)

    def variant(name, m, picks, need, med):
        b = _Builder(np.random.default_rng(seed + 1), scale)
        for j in picks:
            x, y, _ = pts[m][j]
            i = b.left(x, y)
            b.right(x - 20, y, of=i, ham=10)
        if not picks:  # nothing accepted: three pairs that fail the Hamming threshold
            for j in range(3):
                x, y, _ = pts[m][j]
                i = b.left(x, y)
                b.right(x - 20, y, of=i, ham=110)
        return Variant(name, b.arrays(rows, cols), need=need, median=med)

    # pts order:        0      1     2  3  4   5      6     7    8
    vs = [variant("n0", 128, [], {SR.HAMMING_REJECT: 3}, None),
          variant("n1", 128, [2], {SR.ACCEPTED: 1}, (128, 128)),
          variant("n2", 128, [0, 2], {SR.ACCEPTED: 2}, (128, 128)),
          variant("n3", 128, [0, 2, 8], {SR.ACCEPTED: 2, SR.CULLED: 1}, (128, 128)),
          variant("n8_m128", 128, [8, 7, 0, 1, 2, 3, 4, 5], {SR.ACCEPTED: 7, SR.CULLED: 1}, (128, 128)),
          variant("n9_m128", 128, [8, 7, 6, 5, 4, 3, 2, 1, 0], {SR.ACCEPTED: 8, SR.CULLED: 1}, (128, 128)),
          variant("n8_m256", 256, [8, 7, 0, 1, 2, 3, 4, 5], {SR.ACCEPTED: 7, SR.CULLED: 1}, (256, 256)),
          variant("n9_m256", 256, [8, 7, 6, 5, 4, 3, 2, 1, 0], {SR.ACCEPTED: 8, SR.CULLED: 1}, (256, 256))]
    return Scene("median_ranks", L, R, 10.0, 40.0, vs)


# ---- 4. high SAD ------------------------------------------------------------------------
@functools.lru_cache(None)
def high_sad(seed=9):
    """One-pixel horizontal stripes (lo / lo + A) on the left, the inverted stripes on the right
    at a disparity of 20, and a texture of amplitude 2 on both that fixes the minimum's shift (the
    keypoints' own rows carry none: the centre pixels' difference would enter all 66 terms alike).
    Both patches lose their centre pixel, so the six rows of the other parity contribute 2 A per
    pixel: SAD = 66 * 2 A = 132 A exactly.  Each band of 16 rows has its own A, 230 .. 251.
    `above`: A = 249 .. 251, every SAD above 32,767 (median 132 * 250 = 33,000).  `bin255`: the median at 132 * 248 = 32,736 (inside
    [32,640, 32,767]) with SADs above and below it."""
    rng = np.random.default_rng(seed)
    rows, cols = 300, 400
    scale, _ = scale_tables(1.2, 8)
    tex = rng.integers(0, 3, (rows, cols + 20))
    tex[8::16] = 1  # the keypoints' own rows: the centre pixels' difference would add to 66 terms alike

    def images(amps):
        amp = np.zeros(rows, int)
        amp[:16 * len(amps)] = np.repeat(amps, 16)
        on = (np.arange(rows) % 2)[:, None]
        left = on * amp[:, None] + tex[:, :cols]
        right = (1 - on) * amp[:, None] + tex[:, 20:]
        return left.astype(np.uint8), right.astype(np.uint8)

    def variant(name, amps, med):
        b = _Builder(np.random.default_rng(seed + 1), scale)
        d = rng.integers(0, 256, 32, dtype=np.uint8)
        for bnd in range(len(amps)):
            for x in (100, 300):
                i = b.left(x, 16 * bnd + 8, desc=d)
                b.right(x - 20, 16 * bnd + 8, desc=d)
        return Variant(name, b.arrays(rows, cols), need={SR.ACCEPTED: 2 * len(amps)}, median=med)

    a1 = [251, 250, 249, 251, 250, 249, 251, 250, 249, 251, 250, 249, 251, 250, 249, 251, 250, 249]
    a2 = [248, 240, 251, 248, 236, 250, 248, 244, 251, 248, 230, 250, 248, 248, 249, 240, 249, 248]
    L1, R1 = images(a1)
    L2, R2 = images(a2)
    return (Scene("high_sad_above", L1, R1, 10.0, 40.0, [variant("above", a1, (32768, 61710))]),
            Scene("high_sad_bin255", L2, R2, 10.0, 40.0, [variant("bin255", a2, (32736, 32736))]))


# ---- 5. counts --------------------------------------------------------------------------
BETWEEN = 624  # counts: left 4,001's SAD, between thDist with and without the filter's tail values


@functools.lru_cache(None)
def counts(seed=11):
    """More right keypoints than k_stereo_rows keeps in registers (4,096) and more left
    keypoints than k_stereo_filter does (8,192), and the sizes just below: 8,200 random left and
    4,097 random right keypoints on all octaves.  300 of the right keypoints are partners: a left
    keypoint moved by the disparity of 20, with a copy of its descriptor at a few flipped bits;
    the others have descriptors of their own, so the accepted SADs are few enough that some ranks
    matter to the median.  The partners' left keypoints are spread over every index, so every
    register slot of k_stereo_filter holds real SADs, and they include
    - left 8,192 .. 8,199, the values only the filter's tail loop sees (octave 0, whole
      coordinates): 8,192 on a heavily disturbed right patch, which the median culls, the others
      on exact copies (SAD 0), which pull the median down;
    - left 4,001 with a dialled SAD of BETWEEN, which lies between thDist with the seven zeros
      counted (it is culled) and without them (it would be kept): the outputs show whether the
      tail values entered the histograms;
    - right 4,096, the keypoint k_stereo_rows reloads, as the partner of an octave-0 left keypoint.
    Variants: 8,192 / 4,096, 8,193 / 4,097 and 8,200 / 4,097 keypoints."""
    rng = np.random.default_rng(seed)
    rows, cols = 300, 400
    scale, _ = scale_tables(1.2, 8)
    L = texture(rng, rows, cols)
    nl, nr, tail, npart = 8200, 4097, 8192, 300
    octs = rng.integers(0, 8, nl)
    r = 2.0 * scale[octs] + 1e-3
    ys = (r + rng.uniform(0, 1, nl) * (rows - 1 - 2 * r)).astype(_F)
    xs = rng.uniform(45, 380, nl).astype(_F)
    # the tail and right 4,096's partner: octave 0 at whole coordinates, in rows of their own
    special = list(range(tail, nl)) + [4000, 4001]
    for j, i in enumerate(special):
        octs[i], xs[i], ys[i] = 0, 70 + 30 * j, 20 + 27 * j
    kl = make_kps(xs, ys, octs.astype(np.int32), scale)
    dl = rng.integers(0, 256, (nl, 32), dtype=np.uint8)
    # right j's partner (or -1): the tail first, right 4,096 <-> left 4,000, the rest anywhere
    partner = np.full(nr, -1)
    partner[:nl - tail] = np.arange(tail, nl)
    partner[nr - 1], partner[nr - 2] = 4000, 4001
    rest = rng.choice(np.setdiff1d(np.arange(tail), [4000, 4001]), npart - (nl - tail) - 2, replace=False)
    partner[rng.choice(np.arange(nl - tail, nr - 2), len(rest), replace=False)] = rest
    free = partner < 0
    kr = make_kps(rng.uniform(25, 360, nr).astype(_F), np.zeros(nr, _F), np.zeros(nr, np.int32), scale)
    o = rng.integers(0, 8, nr)
    rr = 2.0 * scale[o] + 1e-3
    kr["octave"], kr["y"] = o, (rr + rng.uniform(0, 1, nr) * (rows - 1 - 2 * rr)).astype(_F)
    kr["size"] = _F(31.0) * scale[o]
    dr = rng.integers(0, 256, (nr, 32), dtype=np.uint8)
    for j in np.nonzero(~free)[0]:
        kr[j] = kl[partner[j]]
        kr["x"][j] = kl["x"][partner[j]] - _F(20)
        dr[j] = flip_bits(dl[partner[j]], int(rng.integers(0, 12)), rng)
    check_legal(kl, rows, cols, scale)
    check_legal(kr, rows, cols, scale)
    noise = rng.integers(-2, 3, L.shape)
    for i in special:
        x, y = int(xs[i]) - 20, int(ys[i])
        noise[y - 5:y + 6, x - 10:x + 11] = 0
    x, y = int(xs[tail]) - 20, int(ys[tail])
    noise[y - 5:y + 6, x - 5:x + 6] = rng.integers(-12, 13, (11, 11))
    noise[y, x - 5:x + 6] = 0
    R = shifted(L, 20).astype(int) + noise
    _bump(R, int(xs[4001]) - 20, int(ys[4001]), BETWEEN)
    R = np.clip(R, 0, 255).astype(np.uint8)
    need = {SR.ACCEPTED: 100, SR.HAMMING_REJECT: 1000}
    r4096 = {4000: nr - 1}
    vs = [Variant("r4096_l8192", (kl[:8192], dl[:8192], kr[:4096], dr[:4096]), need=need),
          Variant("r4097_l8193", (kl[:8193], dl[:8193], kr, dr), need=need, chosen=r4096, tail_from=tail,
                  allowed={4001: {SR.ACCEPTED}}),
          Variant("r4097_l8200", (kl, dl, kr, dr), need=need, chosen=r4096, tail_from=tail,
                  allowed={4001: {SR.CULLED}})]
    return Scene("counts", L, R, 10.0, 40.0, vs, nfeatures=1000, capacity=8320)


# ---- 6. pyramids ------------------------------------------------------------------------
PYRAMIDS = {"1.2x12": (1.2, 12, 480, 640), "1.5x6": (1.5, 6, 480, 640), "2.0x4": (2.0, 4, 496, 640)}
# The extractor needs at least one 30-px FAST cell inside the 16-px border of every level, 62 px a
# side (the reference divides by a cell count of 0 below that): 1.5^5 and 2^3 leave 300 x 400 below
# it, so those two pyramids run at the smallest height that keeps their top level legal.
PYRAMIDS_REFUSED = [(1.5, 6, 300, 400), (2.0, 4, 300, 400)]


@functools.lru_cache(None)
def pyramid_own(key, seed=13):
    sf, nl, rows, cols = PYRAMIDS[key]
    rng = np.random.default_rng(seed)
    L = texture(rng, rows, cols, 20, 230)
    R = np.clip(shifted(L, 12).astype(int) + rng.integers(-2, 3, L.shape), 0, 255).astype(np.uint8)
    v = Variant("own", None, need={SR.ACCEPTED: 50})
    return Scene(f"pyramid_own_{key}", L, R, 10.0, 40.0, [v], nfeatures=1000, scale_factor=sf, nlevels=nl)


@functools.lru_cache(None)
def pyramid_top(key, seed=15):
    """256 right keypoints, all on the top octave and each in ceil(4 * scale) + 2 rows, with a
    capacity of 256: the row list is exactly full."""
    sf, nl, rows, cols = PYRAMIDS[key]
    rng = np.random.default_rng(seed)
    scale, _ = scale_tables(sf, nl)
    top = nl - 1
    L = texture(rng, rows, cols, 20, 230)
    R = np.clip(shifted(L, 12).astype(int) + rng.integers(-2, 3, L.shape), 0, 255).astype(np.uint8)
    r = _F(2.0) * scale[top]
    per = int(np.ceil(_F(4.0) * scale[top])) + 2
    ys = []
    for y in np.arange(np.ceil(float(r)) + 0.25, rows - 1 - float(r), 0.25, dtype=np.float64):
        y = _F(y)
        if int(np.ceil(y + r)) - int(np.floor(y - r)) + 1 == per and y - r >= 0 and y + r <= rows - 1:
            ys.append(y)
    ys = rng.choice(np.asarray(ys, _F), 256)
    xs = rng.uniform(100, cols - 100, 256).astype(_F)
    b = _Builder(rng, scale)
    for j in range(256):
        i = b.left(float(xs[j]), float(ys[j]), top - (j % 2))
        b.right(float(xs[j] - _F(12)), float(ys[j]), top, of=i, ham=int(rng.integers(0, 12)))
    v = Variant("top", b.arrays(rows, cols), need={SR.ACCEPTED: 3}, rows_per_keypoint=per)
    return Scene(f"pyramid_top_{key}", L, R, 10.0, 40.0, [v], nfeatures=192, scale_factor=sf, nlevels=nl,
                 capacity=256)


# ---- 7. tall ----------------------------------------------------------------------------
# k_stereo_rows' table holds 4,095 rows, but no image that tall reaches it: the extractor needs
# round(width / height) >= 1 inside the border on every level (DistributeOctTree's nIni; the
# reference indexes an empty vector below that) and at most 2^20 candidate slots on level 0, which
# together end a little under 2,800 rows.  The scene is a portrait image close to that.
TALL_REFUSED = [(4095, 640), (4096, 640), (4095, 2048)]


@functools.lru_cache(None)
def tall(seed=19):
    """2,400 x 1,300: the row table's scan runs over 600 threads instead of 94.  300 crafted
    pairs; the last 40 sit at y = rows - 7 .. rows - 3, the lowest an octave-0 keypoint may
    (y + 2 <= rows - 1), so the right bands reach the image's last row."""
    rng = np.random.default_rng(seed)
    rows, cols = 2400, 1300
    scale, _ = scale_tables(1.2, 8)
    L = texture(rng, rows, cols)
    R = np.clip(shifted(L, 20).astype(int) + rng.integers(-2, 3, L.shape), 0, 255).astype(np.uint8)
    b = _Builder(rng, scale)
    v = Variant("crafted", None, need={SR.ACCEPTED: 150})
    for j in range(260):
        o = j % 3
        r = 2.0 * float(scale[o]) + 0.01
        x, y = float(rng.uniform(60, cols - 40)), float(rng.uniform(r, rows - 1 - r))
        b.right(x - 20, y, o, of=b.left(x, y, o), ham=8)
    for j in range(40):
        x, y = 60.0 + 25 * j, rows - 7.0 + 4.0 * j / 39
        i = b.left(x, y)
        b.right(x - 20, y, of=i, ham=8)
        v.allowed[i] = {SR.ACCEPTED, SR.CULLED}
    v.kps = b.arrays(rows, cols)
    assert int(v.kps[0]["y"].max()) == rows - 3 and int(np.ceil(v.kps[2]["y"].max() + 2)) == rows - 1
    return Scene("tall", L, R, 10.0, 40.0, [v])


# ---- 8. batch ---------------------------------------------------------------------------
@functools.lru_cache(None)
def batch(seed=17):
    """Three pairs for one handle, with 40, 0 and 90 right keypoints."""
    rows, cols = 300, 400
    scale, _ = scale_tables(1.2, 8)
    out = []
    for p, (nl, nr) in enumerate(((60, 40), (30, 0), (90, 90))):
        rng = np.random.default_rng(seed + p)
        L = texture(rng, rows, cols)
        R = np.clip(shifted(L, 20).astype(int) + rng.integers(-2, 3, L.shape), 0, 255).astype(np.uint8)
        b = _Builder(rng, scale)
        for j in range(nl):
            o = int(rng.integers(0, 3))
            i = b.left(float(rng.uniform(60, 380)), float(rng.uniform(12, 287)), o)
            if j < nr:
                b.right(b.l[i][0] - 20, b.l[i][1], o, of=i, ham=8)
        need = {SR.ACCEPTED: 10} if nr else {SR.NO_CANDIDATES: nl}
        out.append(Scene(f"batch_{p}", L, R, 10.0, 40.0, [Variant("crafted", b.arrays(rows, cols), need=need)]))
    return tuple(out)


# Every scene by name with its variants' names, so that the tests can be parametrised without
# generating anything at collection time; `scene(name)` generates (once) on first use.
_MEDIAN_VARIANTS = ["n0", "n1", "n2", "n3", "n8_m128", "n9_m128", "n8_m256", "n9_m256"]
CATALOG = {"branches": (branches, ["crafted"]), "identical": (identical, ["own"]),
           "median_ranks": (median_ranks, _MEDIAN_VARIANTS),
           "high_sad_above": (lambda: high_sad()[0], ["above"]), "high_sad_bin255": (lambda: high_sad()[1], ["bin255"]),
           "counts": (counts, ["r4096_l8192", "r4097_l8193", "r4097_l8200"]),
           **{f"pyramid_own_{k}": (functools.partial(pyramid_own, k), ["own"]) for k in PYRAMIDS},
           **{f"pyramid_top_{k}": (functools.partial(pyramid_top, k), ["top"]) for k in PYRAMIDS},
           "tall": (tall, ["crafted"]),
           **{f"batch_{p}": (functools.partial(lambda p: batch()[p], p), ["crafted"]) for p in range(3)}}
CASES = [(name, v) for name, (_, variants) in CATALOG.items() for v in variants]


def scene(name):
    s = CATALOG[name][0]()
    assert s.name == name and [v.name for v in s.variants] == CATALOG[name][1]
    return s


def variant(s, name):
    return next(v for v in s.variants if v.name == name)


# ---- the restatement on a scene (CPU) ---------------------------------------------------
_REF = {}


def reference(oracle, scene, variant, kps=None):
    """The numpy restatement's StereoResult for a variant, on oracle.pyramid's levels; cached, so
    the tests share one computation (the arrays are read-only).  kps: the keypoint arrays to use
    for an `own` variant (default: oracle.extract's)."""
    key = (scene.name, variant.name)
    if kps is None and key in _REF:
        return _REF[key]
    p = oracle.params(scene.nfeatures, scene.scale_factor, scene.nlevels)
    tab = oracle.tables(p)
    s, inv = scale_tables(scene.scale_factor, scene.nlevels)
    assert (tab["scale"] == s).all() and (tab["inv_scale"] == inv).all()
    pl, pr = _pyramids(oracle, scene)
    use = kps or variant.kps or own_keypoints(oracle, scene)
    res = SR.compute_stereo_matches(pl, pr, tab["scale"], tab["inv_scale"], scene.bf, scene.fx, *use)
    for a in res[:6]:
        a.setflags(write=False)
    if kps is None:
        _REF[key] = res
    return res


_PYR = {}


def _pyramids(oracle, scene):
    if scene.name not in _PYR:
        p = oracle.params(scene.nfeatures, scene.scale_factor, scene.nlevels)
        _PYR[scene.name] = (oracle.pyramid(p, scene.left), oracle.pyramid(p, scene.right))
    return _PYR[scene.name]


def own_keypoints(oracle, scene):
    p = oracle.params(scene.nfeatures, scene.scale_factor, scene.nlevels)
    kl, dl = oracle.extract(p, scene.left)
    kr, dr = oracle.extract(p, scene.right)
    return kl, dl, kr, dr
