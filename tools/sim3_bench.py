"""Time the loop-closure operators on the GPU.  orbmi_sim3_ransac_batch: 4 solvers x 300
hypotheses x N = 200 (the Sim3 scene of tests/sim3_reference.py), HIP events on the matcher's stream around windows of back-to-back calls
after a warm-up, beside the wall time per call and -- with --check-exe, a build of
tests/cpp/sim3_check.cpp -- the host loop of the same header over the same problems (a scalar
port of the library's arithmetic, not the reference program).  orbmi_search_by_sim3: the keyframe
scene of tests/test_sim3_gpu.py, timed the same way.

    python tools/sim3_bench.py [--check-exe PATH] [--windows 7] [--calls 200] [--out FILE]
"""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check-exe")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--solvers", type=int, default=4)
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--out")
    a = ap.parse_args()

    import sim3_reference as R
    from orb_slam2_with_comment_amd import _hip
    from orb_slam2_with_comment_amd._capi import check, lib
    from orb_slam2_with_comment_amd.sim3 import Sim3Ransac, problem

    scenes = [R.sim3_scene(k, 0.6, 0, n=a.n) for k in range(a.solvers)]
    probs = [problem(s["X1"], s["X2"], s["e1"], s["e2"], s["k1"], s["k2"], 0, 0.99, 20, 300, s["triples"]) for s in scenes]
    ransac = Sim3Ransac()
    got = ransac(probs)
    assert all(g["iterations"] == 300 for g in got)
    ref = R.hypotheses(scenes[0]["X1"], scenes[0]["X2"], scenes[0]["e1"], scenes[0]["e2"], scenes[0]["k1"],
                       scenes[0]["k2"], 0, scenes[0]["triples"])
    R.assert_hypotheses_equal(got[0], ref)

    rt = _hip.runtime()
    rt.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    rt.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    stream = C.c_void_p()
    check("orbmi_matcher_get_stream", lib().orbmi_matcher_get_stream(ransac.matcher._h, C.byref(stream)))
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert rt.hipEventCreate(C.byref(e0)) == 0 and rt.hipEventCreate(C.byref(e1)) == 0
    for _ in range(50):
        ransac(probs)
    dev_us, wall_us = [], []
    for _ in range(a.windows):
        assert rt.hipEventRecord(e0, stream) == 0
        t0 = time.perf_counter()
        for _ in range(a.calls):
            ransac(probs)
        wall = time.perf_counter() - t0
        assert rt.hipEventRecord(e1, stream) == 0 and rt.hipEventSynchronize(e1) == 0
        ms = C.c_float()
        assert rt.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        dev_us.append(ms.value * 1e3 / a.calls)
        wall_us.append(wall * 1e6 / a.calls)
    lines = [f"orbmi_sim3_ransac_batch: {a.solvers} solvers x 300 hypotheses x N = {a.n}, host arrays in and out",
             f"  windows of {a.calls} back-to-back calls after 50 warm-up calls, {a.windows} windows",
             f"  stream time per call (HIP events, staging copies and the host's gaps included): "
             f"median {statistics.median(dev_us):.1f} us, min {min(dev_us):.1f}, max {max(dev_us):.1f}",
             f"  wall time per call (Python binding included): median {statistics.median(wall_us):.1f} us, "
             f"min {min(wall_us):.1f}, max {max(wall_us):.1f}"]
    if a.check_exe:
        from sim3_reference import write_problem
        per = []
        with tempfile.TemporaryDirectory() as d:
            for _ in range(a.windows):
                tot = 0.0
                for k, s in enumerate(scenes):
                    fin = os.path.join(d, f"p{k}.bin")
                    write_problem(fin, s)
                    r = subprocess.run([a.check_exe, fin, os.path.join(d, "o.bin"), "200"], capture_output=True, text=True,
                                       check=True, timeout=300)
                    tot += float(r.stdout.split("host_loop_ms")[1].split()[0]) * 1e3
                per.append(tot)
        lines.append(f"  sim3_check host loop over the same {a.solvers} problems (one CPU thread, a scalar port of the same "
                     f"header, not the reference): median {statistics.median(per):.1f} us, min {min(per):.1f}, "
                     f"max {max(per):.1f}")
    # orbmi_search_by_sim3 on the keyframe scene of tests/test_sim3_gpu.py (frames 4 and 6)
    sc = R.sim3_search_scene(4, 6, 1.0)
    m = ransac.matcher

    def search():
        return m.SearchBySim3(sc["kf1"], sc["mps1"], sc["has1"], sc["kf2"], sc["mps2"], sc["has2"], sc["match12"], sc["s12"],
                              sc["R12"], sc["t12"], sc["th"])

    nfound = search()[1]
    for _ in range(50):
        search()
    dev_us, wall_us = [], []
    for _ in range(a.windows):
        assert rt.hipEventRecord(e0, stream) == 0
        t0 = time.perf_counter()
        for _ in range(a.calls):
            search()
        wall = time.perf_counter() - t0
        assert rt.hipEventRecord(e1, stream) == 0 and rt.hipEventSynchronize(e1) == 0
        ms = C.c_float()
        assert rt.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        dev_us.append(ms.value * 1e3 / a.calls)
        wall_us.append(wall * 1e6 / a.calls)
    lines += [f"orbmi_search_by_sim3: keyframes 4 and 6 ({len(sc['kf1'].keys)} and {len(sc['kf2'].keys)} keypoints, "
              f"{int(sc['has1'].sum())} and {int(sc['has2'].sum())} map points, th 7.5, nFound {nfound}), host arrays in and out",
              f"  stream time per call: median {statistics.median(dev_us):.1f} us, min {min(dev_us):.1f}, max {max(dev_us):.1f}",
              f"  wall time per call (Python binding included): median {statistics.median(wall_us):.1f} us, "
              f"min {min(wall_us):.1f}, max {max(wall_us):.1f}"]
    t0 = time.perf_counter()
    R.search_by_sim3(sc["kf1"], sc["mps1"], sc["has1"], sc["kf2"], sc["mps2"], sc["has2"], sc["s12"], sc["R12"], sc["t12"],
                     sc["th"], sc["match12"])
    lines.append(f"  (the numpy restatement of the same search, for scale only: {(time.perf_counter() - t0) * 1e3:.0f} ms)")
    ransac.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
