"""The bundle-adjustment graphs' host plan (csrc/ba_graph.h, HIP-free) without a GPU:
tests/cpp/ba_graph_check.cpp builds LocalBA's and global BA's index tables for small graphs and
writes every table; the same tables are restated here by brute force in numpy -- counting for the
CSRs, a stable argsort by id, all co-observing edge pairs of a point keyed by r1 (r1 + 1) / 2 + r2
and stably sorted -- and every line must be equal.  The two plan checks must accept every plan as
built and reject each corruption of it.

What LocalBA's entry itself calls is ba_tables_ok(..., per_edge=False): the pass over the edges is
left out there because ba_graph_index tests, while it fills, that each edge lands inside its keyframe's
segment (`j >= kf_start[kf + 1]`), which with its paired stores makes kf_pos / kf_edges in range and
inverse.  That test cannot be made to fire from outside -- the counts it compares against come from
the same edges -- so no case here reaches it; the `lba_entry` lines pin what the entry's call does
cover (the CSR ends, rank / free_kf, blk_kf) and that a corrupted kf_edges entry is NOT among it."""
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORBMI_E_ARG = -1
BA_MAX_POSES = 30  # kBaMaxPoses


class Scene:
    def __init__(self, name, kfs, npt, edges):
        """kfs: (id, fixed) in list order; edges: (point, keyframe index) in edge order."""
        self.name, self.kfs, self.npt, self.edges = name, kfs, npt, edges
        assert len(kfs) <= 8 and npt <= 12 and len(edges) <= 40

    def text(self):
        out = ["scene %s %d %d %d" % (self.name, len(self.kfs), self.npt, len(self.edges))]
        out += ["kf %d %d" % k for k in self.kfs]
        out += ["e %d %d" % e for e in self.edges]
        return "\n".join(out) + "\n"

    # ---- the brute-force restatement ----------------------------------------------------------
    def tables(self, drop_unseen, blktab=None):
        nkf, npt, ne = len(self.kfs), self.npt, len(self.edges)
        pt = np.array([e[0] for e in self.edges], np.int64).reshape(-1)
        kf = np.array([e[1] for e in self.edges], np.int64).reshape(-1)
        t = {}
        t["pt_start"] = [int((pt < p).sum()) for p in range(npt + 1)]
        t["kf_start"] = [int((kf < k).sum()) for k in range(nkf + 1)]
        kf_edges = np.argsort(kf, kind="stable")
        kf_pos = np.empty(ne, np.int64)
        kf_pos[kf_edges] = np.arange(ne)
        t["kf_edges"], t["kf_pos"] = kf_edges.tolist(), kf_pos.tolist()
        if not drop_unseen:
            t["kf_pt"] = pt[kf_edges].tolist()
        order = np.argsort(np.array([k[0] for k in self.kfs], np.int64), kind="stable").tolist() if nkf else []
        free = [k for k in order if not self.kfs[k][1] and (not drop_unseen or (kf == k).any())]
        rank = [free.index(k) if k in free else -1 for k in range(nkf)]
        t["order"], t["rank"], t["free_kf"], nf = order, rank, free, len(free)
        if not drop_unseen:
            blk_kf = [None] * (nf * (nf + 1))
            pairs = [(ra, rb) for ra in range(nf) for rb in range(ra, nf)]
            for l, (ra, rb) in enumerate(pairs):
                blk_kf[2 * blktab[nf][l]], blk_kf[2 * blktab[nf][l] + 1] = free[ra], free[rb]
            t["blk_kf"] = blk_kf
            t["npair_cap"] = [sum(sum(rank[kf[e]] >= 0 for e in range(ne) if pt[e] == p) ** 2 for p in range(npt))]
        else:
            keyed = []
            for p in range(npt):
                es = [e for e in range(ne) if pt[e] == p]
                for e1 in es:
                    for e2 in es:
                        r1, r2 = rank[kf[e1]], rank[kf[e2]]
                        if r1 >= 0 and 0 <= r2 <= r1:
                            keyed.append((r1 * (r1 + 1) // 2 + r2, r1, r2, e1, e2))
            idx = np.argsort(np.array([k[0] for k in keyed], np.int64), kind="stable").tolist() if keyed else []
            keyed = [keyed[i] for i in idx]
            firsts = [i for i in range(len(keyed)) if i == 0 or keyed[i][0] != keyed[i - 1][0]]
            t["blk_ij"] = [v for i in firsts for v in keyed[i][1:3]]
            t["blk_start"] = firsts + [len(keyed)]
            t["pairs"] = [v for k in keyed for v in k[3:5]]
            t["npair"] = [len(keyed)]
        t["nf"] = [nf]
        return t


def scenes():
    # ids with gaps in non-ascending list order; keyframe 2 (id 9, fixed) lies between the free ids 4 and 30;
    # keyframe 4 (id 12) is free and no edge names it; point 3 has no edge; point 4 is seen by fixed
    # keyframes only; point 0 is seen by every keyframe but the unseen one; point 5 by keyframe 1 twice over
    # two points; edges of one point are not in keyframe order
    mixed = Scene("mixed", [(30, 0), (4, 0), (9, 1), (0, 1), (12, 0), (21, 0)], 7,
                  [(0, 5), (0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 5), (2, 0), (2, 2), (2, 5), (4, 3), (4, 2),
                   (5, 1), (5, 0), (6, 5), (6, 1), (6, 0)])
    every = Scene("every", [(3, 1), (1, 0), (2, 0), (7, 0)], 3,
                  [(0, 0), (0, 1), (0, 2), (0, 3), (1, 3), (1, 1), (2, 2)])        # point 0: every keyframe
    one_free = Scene("one_free", [(5, 1), (2, 0), (8, 1)], 3, [(0, 0), (0, 1), (1, 1), (1, 2), (2, 0), (2, 2)])
    none_free = Scene("none_free", [(1, 1), (0, 1)], 2, [(0, 0), (0, 1), (1, 1)])
    no_edges = Scene("no_edges", [(2, 0), (1, 0), (0, 1)], 2, [])
    empty = Scene("empty", [], 0, [])
    full = Scene("full", [(7 - k, int(k == 7)) for k in range(8)], 12,
                 [(p, k) for p in range(12) for k in range(8) if (p + k) % 3 != 1][:40])
    return [mixed, every, one_free, none_free, no_edges, empty, full]


REFUSED = [Scene("bad_index", [(0, 0), (1, 0)], 2, [(0, 0), (1, 2)]),
           Scene("bad_point", [(0, 0), (1, 0)], 2, [(0, 0), (2, 1)]),
           Scene("point_goes_down", [(0, 0), (1, 0)], 3, [(1, 0), (0, 1)]),
           Scene("edge_twice", [(0, 0), (1, 0)], 2, [(0, 0), (0, 1), (0, 0)])]


def check_program(sanitize=False):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.fail("no host C++ compiler")
    d = tempfile.mkdtemp(prefix="ba_graph_check_")
    exe = os.path.join(d, "ba_graph_check")
    cmd = [cxx, "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "orb_slam2_with_comment_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "ba_graph_check.cpp"), "-o", exe]
    if sanitize:
        cmd[1:1] = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(cmd, check=True)
    return exe


@functools.lru_cache(maxsize=None)
def native(sanitize=False):
    """Every scene through the check program once: {scene: lines}, {nf: block table line}."""
    exe = check_program(sanitize)
    d = os.path.dirname(exe)
    inp, out = os.path.join(d, "in.txt"), os.path.join(d, "out.txt")
    with open(inp, "w") as f:
        f.write("".join(s.text() for s in scenes() + REFUSED) + "end\n")
    subprocess.run([exe, inp, out], check=True, capture_output=True)
    got, blktab, cur = {}, {}, None
    for line in open(out).read().splitlines():
        w = line.split()
        if w[0] == "scene":
            cur = got.setdefault(w[1], [])
        elif w[0] == "blktab":
            blktab[int(w[1])] = (int(w[2]), [int(v) for v in w[3:]])
        else:
            cur.append(line)
    return got, blktab


def rows(lines, plan):
    return {w[1]: w[2:] for w in (l.split() for l in lines) if w[0] == plan and w[1] != "corrupt"}


@pytest.mark.parametrize("scene", scenes(), ids=lambda s: s.name)
def test_tables_match_brute_force(scene):
    got, blktab = native()
    lines = got[scene.name]
    assert lines[0] == "validate 0"
    tab = {nf: ids for nf, (ok, ids) in blktab.items()}
    for plan, drop in (("lba", False), ("gba", True)):
        have, want = rows(lines, plan), scene.tables(drop, tab)
        assert have.pop("ok") == ["1"]
        assert set(have) == set(want)
        for name in want:
            assert [int(v) for v in have[name]] == [int(v) for v in want[name]], (plan, name)


def test_scenes_cover_the_cases():
    """What the scenes are built to show, read off the restated tables."""
    seen = set()
    for s in scenes():
        lba, gba = s.tables(False, {nf: list(range(nf * (nf + 1) // 2)) for nf in range(9)}), s.tables(True)
        ids, fixed = [k[0] for k in s.kfs], [k[1] for k in s.kfs]
        nkf, nf = len(s.kfs), lba["nf"][0]
        if nkf and nf == 0:
            seen.add("no_free")
        if nf == 1:
            seen.add("one_free")
        free_ids = [ids[k] for k in lba["free_kf"]]
        if any(fixed[k] and any(a < ids[k] < b for a in free_ids for b in free_ids) for k in range(nkf)):
            seen.add("fixed_between_free")
        if ids != sorted(ids) and any(b - a > 1 for a, b in zip(sorted(ids), sorted(ids)[1:])):
            seen.add("gaps_unsorted")
        if any(lba["rank"][k] >= 0 and gba["rank"][k] < 0 for k in range(nkf)):
            seen.add("free_unseen")
            assert gba["nf"][0] < nf
        for p in range(s.npt):
            obs = [e[1] for e in s.edges if e[0] == p]
            if not obs:
                seen.add("point_no_edge")
            elif all(fixed[k] for k in obs):
                seen.add("point_fixed_only")
            if nkf and sorted(obs) == list(range(nkf)):
                seen.add("point_every_kf")
    assert seen == {"no_free", "one_free", "fixed_between_free", "gaps_unsorted", "free_unseen", "point_no_edge",
                    "point_fixed_only", "point_every_kf"}


@pytest.mark.parametrize("scene", REFUSED, ids=lambda s: s.name)
def test_refusals(scene):
    assert native()[0][scene.name] == ["validate %d" % ORBMI_E_ARG]


def test_block_table_is_a_permutation():
    blktab = native()[1]
    assert sorted(blktab) == list(range(BA_MAX_POSES + 1))
    for nf, (ok, ids) in blktab.items():
        assert ok == 1 and sorted(ids) == list(range(nf * (nf + 1) // 2)), nf


def test_plan_checks_reject_corruptions():
    """Each corruption is applied at least once per plan that has the table, and always rejected."""
    got = native()[0]
    applied = {}
    for s in scenes():
        for w in (l.split() for l in got[s.name]):
            if len(w) == 4 and w[1] == "corrupt" and w[3] != "na":
                # (the entry's form of LocalBA's check leaves the per-edge part to ba_graph_index's fill)
                assert w[3] == ("1" if w[0] == "lba_entry" and w[2] == "kf_edges_ne" else "0"), (s.name, w)
                applied[(w[0], w[2])] = applied.get((w[0], w[2]), 0) + 1
    common = ["kf_edges_ne", "pt_start_end", "free_kf_swap"]
    assert all(l != "lba_entry ok 0" for s in scenes() for l in got[s.name])
    assert set(applied) == {(plan, c) for plan in ("lba", "lba_entry") for c in common + ["blk_kf_nkf"]} | \
        {("gba", c) for c in common + ["blk_start_down", "pair_minus1"]}


def test_host_header_under_sanitizers():
    """The stand-alone check program with -fsanitize=address,undefined, on its own, over all scenes."""
    assert native(sanitize=True) == native()
