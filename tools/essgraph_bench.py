"""Time Optimizer::OptimizeEssentialGraph's optimisation on the GPU.  orbmi_optimize_essential_graph
on drifted rings of 200, 1,000 and 4,000 keyframes (tests/essgraph_reference.py: the parent edge and
two covisibility edges per keyframe, one loop, fixed scale), the whole call with host arrays in and
out: HIP events on the matcher's stream around windows of back-to-back calls after a warm-up, beside
the wall time per call; one profiled call for how the time splits between linearisation, assembly,
factor + solve and update; and -- with --check-exe, a build of tests/cpp/essgraph_check.cpp -- the
host loop eg_optimize_host of the same header over the same problem on one CPU thread (this
library's host port, not the reference program).

    python tools/essgraph_bench.py [--check-exe PATH] [--windows 5] [--sizes 200,1000,4000] [--out FILE]
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


def ring(ref, loop, n):
    """A ring of n keyframes whose drift adds up to about the same total at every size."""
    G = ref.ring_graph(9, n, "chain", rot_noise=0.02 / np.sqrt(n), t_noise=0.1 / np.sqrt(n))
    G["covisibles"] = {i: [j for j in (i - 2, i - 3) if j >= 0] for i in range(n)}
    v0, v1, meas, vScw = loop.essential_graph_edges(G)
    return vScw, int(G["loop_id"]), v0, v1, meas


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check-exe")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--sizes", default="200,1000,4000")
    ap.add_argument("--out")
    a = ap.parse_args()

    import essgraph_reference as ref
    from orb_slam2_with_comment_amd import _hip, loop
    from orb_slam2_with_comment_amd._capi import check, lib
    from orb_slam2_with_comment_amd.optimizer import EssentialGraphOptimizer

    opt = EssentialGraphOptimizer()
    rt = _hip.runtime()
    rt.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    rt.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    stream = C.c_void_p()
    check("orbmi_matcher_get_stream", lib().orbmi_matcher_get_stream(opt.matcher._h, C.byref(stream)))
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert rt.hipEventCreate(C.byref(e0)) == 0 and rt.hipEventCreate(C.byref(e1)) == 0

    def fmt(v):
        return f"median {statistics.median(v):.2f} ms, min {min(v):.2f}, max {max(v):.2f}"

    lines = [f"{a.windows} windows of back-to-back calls after 2 warm-up calls; host arrays in and out; fixed scale, 20 iterations allowed"]
    for n in [int(s) for s in a.sizes.split(",")]:
        verts, fixed, v0, v1, meas = ring(ref, loop, n)
        call = lambda profile=False: opt.run(verts, fixed, v0, v1, meas, 1, 20, profile)  # noqa: E731
        t0 = time.perf_counter()
        first = call()
        once = time.perf_counter() - t0
        call()
        calls = max(1, min(50, int(0.5 / max(once, 1e-4))))
        dev_ms, wall_ms = [], []
        for _ in range(a.windows):
            assert rt.hipEventRecord(e0, stream) == 0
            t0 = time.perf_counter()
            for _ in range(calls):
                call()
            wall = time.perf_counter() - t0
            assert rt.hipEventRecord(e1, stream) == 0 and rt.hipEventSynchronize(e1) == 0
            ms = C.c_float()
            assert rt.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
            dev_ms.append(ms.value / calls)
            wall_ms.append(wall * 1e3 / calls)
        prof = call(True)
        ph = prof["phase_ms"]
        lines += [f"orbmi_optimize_essential_graph: ring of {n} keyframes, {len(v0)} edges; chi2 {first['chi2_before']:.3e} -> "
                  f"{first['chi2_after']:.3e}, {first['iterations']} iterations, trials {first['trials']} "
                  f"({sum(first['trials'])} solves), status {first['status']}",
                  f"  stream time per call (HIP events; staging, read-backs and the host's symbolic plan included), "
                  f"{calls} call(s) per window: {fmt(dev_ms)}",
                  f"  wall time per call (Python binding included): {fmt(wall_ms)}",
                  f"  one profiled call, summed over its iterations and trials: linearisation {ph[0]:.2f} ms, assembly {ph[1]:.2f} ms, "
                  f"factor + solve {ph[2]:.2f} ms, update {ph[3]:.2f} ms"]
        if a.check_exe:
            with tempfile.TemporaryDirectory() as d:
                fin = os.path.join(d, "p.bin")
                with open(fin, "wb") as f:
                    f.write(np.array([n, fixed, len(v0), 1, 20], "<i4").tobytes())
                    f.write(np.ascontiguousarray(verts, "<f8").tobytes())
                    f.write(np.ascontiguousarray(v0, "<i4").tobytes())
                    f.write(np.ascontiguousarray(v1, "<i4").tobytes())
                    f.write(np.ascontiguousarray(meas, "<f8").tobytes())
                reps = max(1, min(20, 4000 // n))
                per = []
                for _ in range(a.windows):
                    r = subprocess.run([a.check_exe, "opt", fin, os.path.join(d, "o.bin"), str(reps)], capture_output=True,
                                       text=True, check=True, timeout=600)
                    per.append(float(r.stdout.split("host_loop_ms")[1].split()[0]))
                tail = r.stdout.strip().splitlines()[-1]
            lines.append(f"  eg_optimize_host over the same problem (one CPU thread; this library's host port of the same header, "
                         f"not the reference), {reps} run(s) per window: {fmt(per)}  [{tail}]")
    opt.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
