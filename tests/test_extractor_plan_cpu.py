"""The extractor's host plan (csrc/extractor_plan.h, HIP-free) without a GPU:
tests/cpp/extractor_plan_check.cpp builds the extractor's tables and the plan of each image size below
and writes every table, and builds the padded pyramid on the CPU twice -- level by level from the
resize taps (what k_pyr_level0 / k_pyr_resize consume) and tile by tile from k_pyramid's parameter
blocks with the kernel's loop structure, aborting when a tile reads outside what it staged.  Here the
tables and both pyramids are compared with the CPU oracle, and the cell grid, the candidate regions,
the octree capacities, the IC table and the blur tiles with restatements by brute force.

A refused size must return ORBMI_E_UNSUPPORTED and leave the plan it was given bytewise as it was:
each refused case starts from the plan of the accepted case before it."""
import functools
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ORBMI_E_ARG, ORBMI_E_UNSUPPORTED = -1, -4
EDGE, HALF_PATCH, REGIONS, TILE, IC_ITEMS = 19, 15, 16, 64, 224  # kEdge, kHalfPatch, kFastRegions, kTile, kIcItems

# name: rows, cols, nlevels, nfeatures
ACCEPTED = {
    "62x62": (62, 62, 1, 300),            # the smallest accepted
    "96x128": (96, 128, 2, 300),
    "97x131": (97, 131, 2, 300),          # odd sizes
    "150x201": (150, 201, 3, 300),
    "283x397": (283, 397, 4, 500),        # the golden crop's size
    "480x640": (480, 640, 8, 2000),
    "480x752": (480, 752, 8, 2000),
    "376x1241": (376, 1241, 8, 2000),
    "70x90": (70, 90, 1, 300),            # the widest cell k_fast2 takes: wCell + 6 == kTile
    "1080x1920": (1080, 1920, 8, 2000),   # k_pyramid's tile grid grows past 16 x 8
}
REFUSED = {
    "120x160": (120, 160, 8, 2000),       # a high level under 30 pixels
    "70x128": (70, 128, 2, 300),          # level 0 fits, level 1 does not: the partial build
    "300x100": (300, 100, 1, 300),        # nIni == 0: the reference indexes an empty vector
    "70x91": (70, 91, 1, 300),            # wCell + 6 > kTile
}
# the order of the run: every refused case behind an accepted one, whose plan it must leave alone
ORDER = ["62x62", "120x160", "96x128", "70x128", "97x131", "300x100", "150x201", "70x91", "283x397", "480x640", "480x752",
         "376x1241", "70x90", "1080x1920"]


def image(name):
    r, c = ACCEPTED[name][:2]
    if name == "283x397":
        return np.ascontiguousarray(np.load(os.path.join(GOLD, "crop_283x397_l4.npz"), allow_pickle=False)["image"])
    return np.random.default_rng(r * 10007 + c).integers(0, 256, (r, c), dtype=np.uint8)


def check_program(sanitize=False):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.fail("no host C++ compiler")
    d = tempfile.mkdtemp(prefix="extractor_plan_check_")
    exe = os.path.join(d, "extractor_plan_check")
    cmd = [cxx, "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "orb_slam2_with_comment_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "extractor_plan_check.cpp"), "-o", exe]
    if sanitize:
        cmd[1:1] = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(cmd, check=True)
    return exe


@functools.lru_cache(maxsize=None)
def native(sanitize=False):
    """Every case through the check program once: {case: (rc, {key: [words]})}, {case: (a, b) pyramid bytes}."""
    exe = check_program(sanitize)
    d = os.path.dirname(exe)
    inp, out = os.path.join(d, "in.txt"), os.path.join(d, "out.txt")
    with open(inp, "w") as f:
        for name in ORDER:
            img = "-"
            if name in ACCEPTED:
                img = os.path.join(d, name + ".img")
                image(name).tofile(img)
            f.write("case %s %d %d %d %d %s\n" % ((name,) + (ACCEPTED.get(name) or REFUSED[name]) + (img,)))
        f.write("end\n")
    subprocess.run([exe, inp, out], check=True, capture_output=True)
    got, cur = {}, None
    for line in open(out).read().splitlines():
        w = line.split()
        if w[0] == "case":
            cur = got.setdefault(w[1], (int(w[2]), {}))[1]
        elif w[0] == "describe_overflow":
            got[w[0]] = (int(w[1]), {})
        elif w[0] in ("level", "ic"):
            cur.setdefault(w[0], []).append(w[1:])
        elif w[0] != "plan_us":
            cur[w[0]] = w[1:]
    pyr = {n: tuple(np.fromfile(os.path.join(d, n + ".img." + k), np.uint8) for k in "ab") for n in ACCEPTED}
    shutil.rmtree(d)
    return got, pyr


def ints(words, width=None):
    a = np.array([int(v) for v in words], np.int64)
    return a.reshape(-1, width) if width else a


def floats(words):
    return np.array([int(v) for v in words], np.uint32).view(np.float32)


LEVEL = ("W H stride ph off cell_begin cell_end nfeat out_base out_cap key_base key_cap width height nIni hX scale size "
         "blur_xv resize_xv xtab_off ytab_off boff bstride").split()
CELL = "x0 y0 w h sx sy slot_base level roi_off stride lcell".split()
SCALARS = "pimg bimg keys_cap out_cap fast_maxw fast_maxh kx ky hx hy blob_words lds0 lds_half blob_size blob_fnv".split()


def plan_of(name):
    rc, t = native()[0][name]
    assert rc == 0
    levels = [dict(zip(LEVEL, (int(v) for v in row))) for row in t["level"]]
    for g in levels:
        for k in ("hX", "scale", "size"):
            g[k] = np.array([g[k]], np.uint32).view(np.float32)[0]
    cells = [dict(zip(CELL, (int(v) for v in row))) for row in ints(t["cells"], len(CELL))]
    return t, levels, cells, dict(zip(SCALARS, (int(v) for v in t["scalars"])))


def params(oracle, name):
    r, c, nl, nf = ACCEPTED[name]
    return oracle.params(nf, 1.2, nl, 20, 7)


@pytest.mark.parametrize("name", list(ACCEPTED))
def test_tables_equal_oracle(oracle, name):
    t = native()[0][name][1]
    want = oracle.tables(params(oracle, name))
    for k in ("scale", "inv_scale", "sigma2", "inv_sigma2"):
        np.testing.assert_array_equal(floats(t[k]), want[k], err_msg=k)
    np.testing.assert_array_equal(ints(t["nfeat"]), want["features_per_level"])
    np.testing.assert_array_equal(ints(t["umax"]), want["umax"])


@pytest.mark.parametrize("name", list(ACCEPTED))
def test_pyramids_equal_oracle(oracle, name):
    """Level by level and tile by tile, every padded byte; and every padded byte is some tile's."""
    ref = np.concatenate([l.reshape(-1) for l in oracle.pyramid(params(oracle, name), image(name))])
    a, b = native()[1][name]
    np.testing.assert_array_equal(a, ref)
    np.testing.assert_array_equal(b, ref)
    assert native()[0][name][1]["unwritten"] == ["0"]


def cell_grid(W, H):
    """ComputeKeyPointsOctTree's cell loop (src/ORBextractor.cc:778-829) for one level, cell by cell: the ROI of
    every cell it runs FAST on and the shift it adds, in loop order; and nCols * nRows, wCell, hCell."""
    minB, maxBX, maxBY = EDGE - 3, W - EDGE + 3, H - EDGE + 3
    width, height = np.float32(maxBX - minB), np.float32(maxBY - minB)
    nCols, nRows = int(width / np.float32(30)), int(height / np.float32(30))
    wCell, hCell = math.ceil(width / np.float32(nCols)), math.ceil(height / np.float32(nRows))
    out = []
    for i in range(nRows):
        iniY = minB + i * hCell
        if iniY >= maxBY - 3:
            continue
        maxY = min(iniY + hCell + 6, maxBY)
        for j in range(nCols):
            iniX = minB + j * wCell
            if iniX >= maxBX - 6:
                continue
            maxX = min(iniX + wCell + 6, maxBX)
            out.append((iniX, iniY, maxX - iniX, maxY - iniY, j * wCell, i * hCell))
    return out, nCols * nRows, wCell, hCell


@pytest.mark.parametrize("name", list(ACCEPTED))
def test_plan_equals_brute_force(oracle, name):
    p = params(oracle, name)
    rows, cols = ACCEPTED[name][:2]
    t, levels, cells, s = plan_of(name)
    Wo, Ho = oracle.level_sizes(p, rows, cols)
    nfeat = oracle.tables(p)["features_per_level"]
    assert [g["W"] for g in levels] == Wo.tolist() and [g["H"] for g in levels] == Ho.tolist()
    key = outb = off = boff = ncell = 0
    for l, g in enumerate(levels):
        want, ngrid, wCell, hCell = cell_grid(g["W"], g["H"])
        mine = cells[g["cell_begin"]:g["cell_end"]]
        assert g["cell_begin"] == ncell and len(mine) == ngrid
        ncell += ngrid
        # the cells FAST runs on, in the reference's order; the skipped ones keep their place with w == 0
        assert [tuple(c[k] for k in CELL[:6]) for c in mine if c["w"]] == want
        assert [c["lcell"] for c in mine] == list(range(ngrid)) and all(c["level"] == l for c in mine)
        assert all(c["stride"] == g["stride"] and
                   c["roi_off"] == g["off"] + (EDGE + c["y0"]) * g["stride"] + EDGE + c["x0"] for c in mine)
        assert all(0 <= c["x0"] and c["x0"] + c["w"] <= g["W"] and 0 <= c["y0"] and c["y0"] + c["h"] <= g["H"] and
                   c["w"] <= TILE and c["h"] <= TILE for c in mine)
        # a cell's candidates: FAST's non-maximum suppression keeps at most one of two neighbours per axis
        cap = ((wCell + 1) // 2) * ((hCell + 1) // 2)
        assert (g["key_base"], g["key_cap"]) == (key, cap * len(want))
        key += cap * len(want)
        # DistributeOctTree (:539-560) and its output slots: at most max(N, 4 nIni) + 3 nodes
        width, height = g["W"] - 2 * EDGE + 6, g["H"] - 2 * EDGE + 6
        ratio = np.float32(width) / np.float32(height)
        nIni = int(np.floor(ratio + np.float32(0.5)))  # round(): half away from zero
        assert (g["width"], g["height"], g["nIni"]) == (width, height, nIni) and nIni >= 1
        assert g["hX"] == np.float32(width) / np.float32(nIni)
        assert g["nfeat"] == nfeat[l]
        assert (g["out_base"], g["out_cap"]) == (outb, max(int(nfeat[l]) + 3, 4 * nIni) + 1)
        outb += g["out_cap"]
        # the padded and the blurred planes lie behind one another
        assert g["stride"] % 64 == 0 and 0 <= g["stride"] - (g["W"] + 2 * EDGE) < 64 and g["ph"] == g["H"] + 2 * EDGE
        assert g["bstride"] % 128 == 0 and 0 <= g["bstride"] - g["W"] < 128
        assert (g["off"], g["boff"]) == (off, boff)
        off, boff = off + g["stride"] * g["ph"], boff + g["bstride"] * g["H"]
        assert g["scale"] == oracle.tables(p)["scale"][l] and g["size"] == np.float32(int(np.float32(31) * g["scale"]))
        assert g["blur_xv"] == g["W"] // 4 * 4
        if name == "70x90":
            assert wCell + 6 == TILE
    assert (s["keys_cap"], s["out_cap"], s["pimg"], s["bimg"]) == (key, outb, off, boff)
    assert s["fast_maxw"] == max(c["w"] for c in cells) and s["fast_maxh"] == max(c["h"] for c in cells)
    assert s["blob_size"] == s["kx"] * s["ky"] * s["blob_words"]
    assert 4 * s["blob_words"] + s["lds0"] + 2 * s["lds_half"] <= 64 * 1024
    assert (s["kx"] * s["ky"] > 16 * 8) == (name == "1080x1920")


@pytest.mark.parametrize("name", list(ACCEPTED))
def test_regions_partition_the_candidates(name):
    t, levels, cells, s = plan_of(name)
    regbase = ints(t["regbase"], REGIONS)
    assert len(regbase) == len(levels)
    for l, g in enumerate(levels):
        ends = np.append(regbase[l], g["key_base"] + g["key_cap"])
        assert ends[0] == g["key_base"] and (np.diff(ends) >= 0).all()
        _, _, wCell, hCell = cell_grid(g["W"], g["H"])
        need = np.zeros(REGIONS, np.int64)
        for c in cells[g["cell_begin"]:g["cell_end"]]:
            assert c["slot_base"] == regbase[l][c["lcell"] % REGIONS]
            if c["w"]:
                need[c["lcell"] % REGIONS] += ((wCell + 1) // 2) * ((hCell + 1) // 2)
        assert (np.diff(ends) >= need).all()


def test_ic_table_covers_the_circle_once():
    t = native()[0]["62x62"][1]
    assert t["describe"] == ["0"] and native()[0]["describe_overflow"][0] == ORBMI_E_ARG
    umax = ints(t["umax"])
    circle = sorted((u, v) for v in range(-HALF_PATCH, HALF_PATCH + 1) for u in range(-umax[abs(v)], umax[abs(v)] + 1))
    assert [int(r[0]) for r in t["ic"]] == [0, 1, 2, 3]
    for ou, row in enumerate(t["ic"]):
        items = ints(row[1:], 4)
        assert len(items) <= IC_ITEMS
        px = []
        for wa, wm, r, off in items:
            assert off % 4 == 0 and wm != 0
            for b in range(4):
                m = wm >> (8 * b) & 255
                assert m in (0, 1)
                if m:
                    u = off + b - ou - HALF_PATCH
                    assert (wa >> (8 * b) & 255) == u + 16
                    px.append((u, r - HALF_PATCH))
                else:
                    assert (wa >> (8 * b) & 255) == 0
        assert sorted(px) == circle, ou


def test_pattern_table_is_the_transposed_pairs():
    have = ints(native()[0]["62x62"][1]["pattern"], 4)
    pat = (4 * np.arange(256)[:, None] + np.arange(4)[None, :]) % 251 - 125  # the check program's stand-in
    for pair in range(256):
        x0, y0, x1, y1 = pat[pair]
        assert have[16 * (pair & 15) + (pair >> 4)].tolist() == [x0, x1, y0, y1]


@pytest.mark.parametrize("name", list(ACCEPTED))
def test_blur_tiles_tile_every_level(name):
    t, levels, cells, s = plan_of(name)
    cover = [np.zeros((g["H"], g["W"]), np.int32) for g in levels]
    for l, x0, y0 in ints(t["btiles"], 3):
        assert x0 % 128 == 0 and y0 % 32 == 0 and x0 < levels[l]["W"] and y0 < levels[l]["H"]
        cover[l][y0:y0 + 32, x0:x0 + 128] += 1
    assert all((c == 1).all() for c in cover)


@pytest.mark.parametrize("name", list(REFUSED))
def test_refused_sizes_leave_the_plan_alone(name):
    rc, t = native()[0][name]
    assert rc == ORBMI_E_UNSUPPORTED and t == {"untouched": ["1"]}


def test_host_header_under_sanitizers():
    """The stand-alone check program with -fsanitize=address,undefined, on its own, over all cases."""
    (ga, pa), (gb, pb) = native(sanitize=True), native()
    assert ga == gb
    assert all(np.array_equal(pa[n][k], pb[n][k]) for n in ACCEPTED for k in (0, 1))
