"""Time Optimizer::BundleAdjustment on the GPU.  orbmi_bundle_adjustment on sliding-window
trajectories of about 100, 500 and 1,500 keyframes (tests/gba_scenes.py: every point seen by 2..8
neighbouring keyframes, 15 points per keyframe), 10 iterations, no robust kernel, the whole call
with host arrays in and out: HIP events on the handle's stream around windows of back-to-back calls
after a warm-up, beside the wall time per call; one profiled call (ORBMI_GBA_PROFILE) for how the
time splits between linearisation, Schur complement, factor + solve and update + chi2; and the block
fill of S before elimination.

    python tools/gba_bench.py [--windows 5] [--sizes 100,500,1500] [--out FILE]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--sizes", default="100,500,1500")
    ap.add_argument("--out")
    a = ap.parse_args()

    import gba_scenes as GS
    from orb_slam2_with_comment_amd import _hip
    from orb_slam2_with_comment_amd._capi import check, lib
    from orb_slam2_with_comment_amd.optimizer import GlobalBA

    ba = GlobalBA()
    rt = _hip.runtime()
    rt.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    rt.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    rt.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    rt.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    stream = C.c_void_p()
    assert rt.hipStreamCreate(C.byref(stream)) == 0
    check("orbmi_ba_set_stream", lib().orbmi_ba_set_stream(ba._h, stream))
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert rt.hipEventCreate(C.byref(e0)) == 0 and rt.hipEventCreate(C.byref(e1)) == 0

    def fmt(v):
        return f"median {statistics.median(v):.2f} ms, min {min(v):.2f}, max {max(v):.2f}"

    lines = [f"{a.windows} windows of back-to-back calls after 2 warm-up calls; host arrays in and out; 10 iterations, not robust"]
    for n in [int(s) for s in a.sizes.split(",")]:
        problem = GS.sliding_window_problem(seed=200 + n, n_kf=n + 1, n_points=15 * n)[0]
        call = lambda: ba.run(problem, 10, False)  # noqa: E731
        t0 = time.perf_counter()
        first = call()
        once = time.perf_counter() - t0
        call()
        calls = max(1, min(20, int(0.5 / max(once, 1e-4))))
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
        os.environ["ORBMI_GBA_PROFILE"] = "1"
        try:
            ph = call()["phase_ms"]
        finally:
            del os.environ["ORBMI_GBA_PROFILE"]
        nf = first["n_free"]
        fill = first["n_blocks"] / max(1, nf * (nf + 1) // 2)
        solves = int(first["trials"].sum())
        tot = sum(ph)
        lines += [f"orbmi_bundle_adjustment: {nf} free keyframes ({6 * nf} unknowns), {len(problem.pts)} points, "
                  f"{len(problem.edges)} edges; chi2 {first['chi2_initial']:.3e} -> {first['chi2']:.3e}, "
                  f"{first['iterations']} iterations, {solves} solves, status {first['status']}",
                  f"  block fill of S before elimination (i >= j): {first['n_blocks']} of {nf * (nf + 1) // 2} = {fill:.4f}",
                  f"  stream time per call (HIP events; uploads, read-backs and the host's index tables included), "
                  f"{calls} call(s) per window: {fmt(dev_ms)}",
                  f"  wall time per call (Python binding included): {fmt(wall_ms)}",
                  f"  one profiled call, summed over its iterations and trials: linearise {ph[0]:.2f} ms, Schur {ph[1]:.2f} ms, "
                  f"factor + solve {ph[2]:.2f} ms ({100 * ph[2] / max(tot, 1e-9):.0f} %), update + chi2 {ph[3]:.2f} ms"]
    ba.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
