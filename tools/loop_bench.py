"""Time loop detection on the GPU.  orbmi_detect_loop_candidates at 64, 512 and 4096 stored
keyframes of about 1500 words each (a synthetic 100000-word vocabulary; a cluster of keyframes
shares 40 % of the query's words, the rest share what chance gives), HIP events around windows of
back-to-back calls after a warm-up, beside the wall time per call and -- with --check-exe, a build
of tests/cpp/loop_check.cpp -- the host loop of a scalar inverted-file DetectLoopCandidates over
the same data (one CPU thread; a port of the algorithm for comparison, not the reference program).
orbmi_search_by_bow_kf: frames 3 and 4 of the synthetic sequence, timed the same way.

    python tools/loop_bench.py [--check-exe PATH] [--windows 7] [--calls 50] [--out FILE]
"""
import argparse
import ctypes as C
import os
import statistics
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

NWORDS = 100000


def bench_case(nkf, nwords_kf=1500, seed=0, scoring=0):
    """-> the case format of tests/loop_reference.database_case, keyframe ids 0 .. nkf - 1 added in
    order, plus "min_score" and "nwords"."""
    rng = np.random.default_rng(seed)

    def vec(n, must=()):
        w = np.unique(np.concatenate([np.asarray(must, np.int64), rng.integers(0, NWORDS, max(n - len(must), 0))]))
        v = rng.uniform(0.1, 1.0, len(w))
        return w.astype(np.uint32), (v / v.sum()).astype(np.float64)

    qw, qv = vec(nwords_kf)
    centre = nkf // 3
    store = []
    for i in range(nkf):
        near = abs(i - centre) <= 3
        must = rng.choice(qw, int(0.4 * len(qw)), replace=False) if near else ()
        store.append((i, *vec(nwords_kf, must)))
    best = {i: [j for j in (i - 1, i + 1, i - 2, i + 2, i - 3, i + 3, i - 4, i + 4, i - 5, i + 5) if 0 <= j < nkf]
            for i in range(nkf)}
    return {"scoring": scoring, "store": store, "ops": [("add", i) for i in range(nkf)], "query": (qw, qv),
            "connected": list(range(max(nkf - 5, 0), nkf)), "best_covis": best, "min_score": np.float32(0.02),
            "nwords": NWORDS}


def write_invfile_case(case, path):
    """The input of `loop_check invfile`."""
    nkf = len(case["store"])
    rows = [np.asarray(case["best_covis"].get(i, ()), np.int32) for i in range(nkf)]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    cov = np.concatenate(rows).astype(np.int32) if nkf and off[-1] else np.zeros(0, np.int32)
    qw, qv = case["query"]
    with open(path, "wb") as f:
        f.write(struct.pack("<6if", case["scoring"], nkf, case["nwords"], len(qw), len(case["connected"]), len(cov),
                            float(case["min_score"])))
        for i, w, v in case["store"]:
            f.write(struct.pack("<i", len(w)))
            f.write(np.ascontiguousarray(w, np.uint32).tobytes())
            f.write(np.ascontiguousarray(v, np.float64).tobytes())
        f.write(np.ascontiguousarray(qw, np.uint32).tobytes())
        f.write(np.ascontiguousarray(qv, np.float64).tobytes())
        f.write(np.asarray(case["connected"], np.int32).tobytes())
        f.write(off.tobytes())
        f.write(cov.tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check-exe")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--sizes", default="64,512,4096")
    ap.add_argument("--out")
    a = ap.parse_args()

    import loop_reference as ref
    from orb_slam2_with_comment_amd import _hip
    from orb_slam2_with_comment_amd._capi import check, lib
    from orb_slam2_with_comment_amd.loop import KeyFrameDatabase

    rt = _hip.runtime()
    rt.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    rt.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    rt.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert rt.hipEventCreate(C.byref(e0)) == 0 and rt.hipEventCreate(C.byref(e1)) == 0

    def timed(fn, calls, stream=None):
        for _ in range(20):
            fn()
        dev_us, wall_us = [], []
        for _ in range(a.windows):
            assert rt.hipEventRecord(e0, stream) == 0
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            wall = time.perf_counter() - t0
            assert rt.hipEventRecord(e1, stream) == 0 and rt.hipEventSynchronize(e1) == 0
            ms = C.c_float()
            assert rt.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
            dev_us.append(ms.value * 1e3 / calls)
            wall_us.append(wall * 1e6 / calls)
        return dev_us, wall_us

    def fmt(v):
        return f"median {statistics.median(v):.1f} us, min {min(v):.1f}, max {max(v):.1f}"

    lines = [f"windows of {a.calls} back-to-back calls after 20 warm-up calls, {a.windows} windows; host arrays in and out; "
             "every call waits for its result, so the event time of a window is its wall time seen from the device"]
    for nkf in [int(s) for s in a.sizes.split(",")]:
        case = bench_case(nkf)
        db = KeyFrameDatabase(case["scoring"], max_keyframes=nkf, max_words_total=nkf * 1600)
        ref.fill(db, case)
        qw, qv = case["query"]
        nk = nkf
        off = np.zeros(nk + 1, np.int32)
        rows = [np.asarray(case["best_covis"][i], np.int32) for i in range(nk)]
        off[1:] = np.cumsum([len(r) for r in rows])
        cov = np.concatenate(rows).astype(np.int32)
        conn = np.asarray(case["connected"], np.int32)
        out = np.zeros(nkf, np.int32)
        n = C.c_int()
        L = lib()

        def call():
            check("orbmi_detect_loop_candidates", L.orbmi_detect_loop_candidates(
                db._h, qw.ctypes.data, qv.ctypes.data, len(qw), C.c_float(case["min_score"]), conn.ctypes.data, len(conn),
                off.ctypes.data, cov.ctypes.data, nk, out.ctypes.data, len(out), C.byref(n)))
        call()
        got = out[:n.value].tolist()
        r = db.query(qw, qv, conn)
        nscored = int((r["common"] > r["min_common"]).sum())
        dev_us, wall_us = timed(call, a.calls)
        words = sum(len(w) for _, w, _ in case["store"])
        lines += [f"orbmi_detect_loop_candidates: {nkf} keyframes, {words} stored words ({words * 12 / 1e6:.1f} MB), query of "
                  f"{len(qw)} words; max_common {r['max_common']}, {nscored} slots scored, candidates {got}",
                  f"  time per call between HIP events: {fmt(dev_us)}",
                  f"  wall time per call (ctypes call only): {fmt(wall_us)}"]
        if a.check_exe:
            with tempfile.TemporaryDirectory() as d:
                path = os.path.join(d, "db.bin")
                write_invfile_case(case, path)
                per = []
                for _ in range(a.windows):
                    o = subprocess.run([a.check_exe, "invfile", path, "200"], capture_output=True, text=True, check=True,
                                       timeout=300).stdout.splitlines()
                    host = [int(x) for x in o[0].split()[1:]]
                    assert host == got, (host, got)
                    per.append(float(o[1].split()[1]))
                lines.append("  loop_check invfile on the same data (one CPU thread, a scalar inverted-file port, not the "
                             f"reference; the same candidates): {fmt(per)}")
        db.close()

    # orbmi_search_by_bow_kf on two neighbouring keyframes of the synthetic sequence
    import scenario
    from orb_slam2_with_comment_amd import ORBmatcher, synth_map as SM
    from orb_slam2_with_comment_amd.types import FeatureVector
    kf1, kf2 = scenario.make_frame(3), scenario.make_frame(4)
    ok1 = (scenario.frame_data(3)[3] > 0).astype(np.uint8)
    ok2 = (scenario.frame_data(4)[3] > 0).astype(np.uint8)
    fv1, fv2 = FeatureVector(SM.bow_nodes(kf1.desc)), FeatureVector(SM.bow_nodes(kf2.desc))
    m = ORBmatcher(0.75, True)
    stream = C.c_void_p()
    check("orbmi_matcher_get_stream", lib().orbmi_matcher_get_stream(m._h, C.byref(stream)))
    nm = m.SearchByBoWKF(kf1, ok1, fv1, kf2, ok2, fv2)[1]
    dev_us, wall_us = timed(lambda: m.SearchByBoWKF(kf1, ok1, fv1, kf2, ok2, fv2), a.calls, stream)
    lines += [f"orbmi_search_by_bow_kf: frames 3 and 4 ({len(kf1.keys)} / {len(kf2.keys)} keypoints, {len(fv1.node_id)} nodes, "
              f"nmatches {nm})",
              f"  stream time per call (HIP events, staging copies and the host's gaps included): {fmt(dev_us)}",
              f"  wall time per call (Python binding included): {fmt(wall_us)}"]
    t0 = time.perf_counter()
    ref.search_by_bow_kf(kf1, ok1, fv1, kf2, ok2, fv2)
    lines.append(f"  (the Python restatement of the same search, for scale only: {(time.perf_counter() - t0) * 1e3:.0f} ms)")
    m.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
