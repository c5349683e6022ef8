"""Time the second half of LoopClosing::ComputeSim3 on the GPU.  orbmi_optimize_sim3_batch: 1 and
4 problems x n = 100 and n = 300 (the two-camera scene of tests/sim3opt_reference.py, 15 %
outliers, free scale), HIP events on the matcher's stream around windows of back-to-back calls
after a warm-up, beside the wall time per call and -- with --check-exe, a build of
tests/cpp/sim3opt_check.cpp -- the host loop of the same header over the same problems (a scalar
port of the library's arithmetic, not the reference program).  orbmi_search_by_projection_sim3:
keyframes 4 and 6 of the synthetic sequence (KF2's map points searched in KF1), timed the same way.

    python tools/sim3opt_bench.py [--check-exe PATH] [--windows 7] [--calls 100] [--out FILE]
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
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--out")
    a = ap.parse_args()

    import sim3_reference as R
    import sim3opt_reference as ref
    from test_sim3opt_cpu import write_problem
    from orb_slam2_with_comment_amd import _hip
    from orb_slam2_with_comment_amd._capi import check, lib
    from orb_slam2_with_comment_amd.optimizer import Sim3Optimizer, sim3_opt_problem

    opt = Sim3Optimizer()
    rt = _hip.runtime()
    rt.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    rt.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    stream = C.c_void_p()
    check("orbmi_matcher_get_stream", lib().orbmi_matcher_get_stream(opt.matcher._h, C.byref(stream)))
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert rt.hipEventCreate(C.byref(e0)) == 0 and rt.hipEventCreate(C.byref(e1)) == 0

    def timed(fn, calls):
        for _ in range(30):
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

    lines = [f"windows of {a.calls} back-to-back calls after 30 warm-up calls, {a.windows} windows; host arrays in and out"]
    for n in (100, 300):
        scenes = [ref.make_problem(500 + k, n, 0, 0.15) for k in range(4)]
        probs = [sim3_opt_problem(P.x3d_c1, P.x3d_c2, P.obs1, P.obs2, P.inv_sigma2_1, P.inv_sigma2_2, P.k1, P.k2, P.th2,
                                  P.fix_scale, P.R12, P.t12, P.s12) for P in scenes]
        got = opt.run(probs)
        want = ref.optimize_sim3(scenes[0])
        assert got[0]["n_in"] == want.n_in and (got[0]["inlier"] == want.inlier).all()
        host = None
        if a.check_exe:
            host = []
            with tempfile.TemporaryDirectory() as d:
                for k, P in enumerate(scenes):
                    fin = os.path.join(d, f"p{k}.bin")
                    write_problem(P, fin)
                    per = []
                    for _ in range(a.windows):
                        r = subprocess.run([a.check_exe, fin, os.path.join(d, "o.bin"), "200"], capture_output=True,
                                           text=True, check=True, timeout=300)
                        per.append(float(r.stdout.split("host_loop_ms")[1].split()[0]) * 1e3)
                    host.append(per)
        for batch in (1, 4):
            dev_us, wall_us = timed(lambda: opt.run(probs[:batch]), a.calls)
            its = [g["iterations"] for g in got[:batch]]
            lines += [f"orbmi_optimize_sim3_batch: {batch} problem(s) x n = {n} (15 % outliers, free scale; Levenberg "
                      f"iterations {its}, n_in {[g['n_in'] for g in got[:batch]]})",
                      f"  stream time per call (HIP events, staging copies and the host's gaps included): {fmt(dev_us)}",
                      f"  wall time per call (Python binding included): {fmt(wall_us)}"]
            if host:
                tot = [sum(host[k][w] for k in range(batch)) for w in range(a.windows)]
                lines.append(f"  sim3opt_check host loop over the same {batch} problem(s) (one CPU thread, a scalar port of "
                             f"the same header, not the reference): {fmt(tot)}")
    # orbmi_search_by_projection_sim3: KF2's map points searched in KF1 under KF1's pose
    sc = R.sim3_search_scene(4, 6, 1.0)
    mps = sc["mps2"][sc["has2"] == 1]
    matched = np.full(len(sc["kf1"].keys), -1, np.int32)
    Scw = np.ascontiguousarray(sc["kf1"].tcw[:3], np.float32)
    m = opt.matcher
    nm = m.SearchByProjectionSim3(sc["kf1"], Scw, mps, matched, 10)[1]
    dev_us, wall_us = timed(lambda: m.SearchByProjectionSim3(sc["kf1"], Scw, mps, matched, 10), a.calls)
    lines += [f"orbmi_search_by_projection_sim3: keyframes 4 and 6 ({len(sc['kf1'].keys)} keypoints, {len(mps)} points, th 10, "
              f"nmatches {nm}); the host replay of the claims is part of the call",
              f"  stream time per call: {fmt(dev_us)}",
              f"  wall time per call (Python binding included): {fmt(wall_us)}"]
    t0 = time.perf_counter()
    ref.search_by_projection_sim3(sc["kf1"], Scw, mps, matched, 10)
    lines.append(f"  (the numpy restatement of the same search, for scale only: {(time.perf_counter() - t0) * 1e3:.0f} ms)")
    opt.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
