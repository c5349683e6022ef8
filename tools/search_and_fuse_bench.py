"""Time orbmi_fuse_sim3_search_batch, the search of LoopClosing::SearchAndFuse, on one GPU: one
batched call over nkf keyframes against nkf single-keyframe calls of the same entry.  Keyframes of
2,000 keypoints (tests/sim3opt_reference.projection_scene; every keyframe its own arrays and its own
Scw, a few centimetres apart), nkf = 1, 8, 24, lists of 500 and 4,000 points (the 4,000 are the
scene's 2,000 twice, the second copy 2 cm off with 8 descriptor bits flipped).  HIP events on the
matcher's stream around windows of back-to-back calls after a warm-up; host arrays in and out.

    python tools/search_and_fuse_bench.py [--windows 7] [--calls 50] [--out FILE]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out")
    a = ap.parse_args()

    import fuse_sim3_reference as fref
    import sim3opt_reference as so
    from orb_slam2_with_comment_amd import _hip
    from orb_slam2_with_comment_amd._capi import check, lib
    from orb_slam2_with_comment_amd.matcher import ORBmatcher
    from orb_slam2_with_comment_amd.types import Frame, FrameView

    m = ORBmatcher()
    L = lib()
    rt = _hip.runtime()
    rt.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    rt.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    stream = C.c_void_p()
    check("orbmi_matcher_get_stream", L.orbmi_matcher_get_stream(m._h, C.byref(stream)))
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert rt.hipEventCreate(C.byref(e0)) == 0 and rt.hipEventCreate(C.byref(e1)) == 0

    def timed(fn):
        for _ in range(10):
            fn()
        dev_us, wall_us = [], []
        for _ in range(a.windows):
            assert rt.hipEventRecord(e0, stream) == 0
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn()
            wall = time.perf_counter() - t0
            assert rt.hipEventRecord(e1, stream) == 0 and rt.hipEventSynchronize(e1) == 0
            ms = C.c_float()
            assert rt.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
            dev_us.append(ms.value * 1e3 / a.calls)
            wall_us.append(wall * 1e6 / a.calls)
        return dev_us, wall_us

    def fmt(v):
        return f"median {statistics.median(v):.1f} us, min {min(v):.1f}, max {max(v):.1f}"

    sc = so.projection_scene(0, 2000, 2000, 1.1, special=False)
    base = sc["kf"]
    rng = np.random.default_rng(1)
    twice = np.concatenate([sc["mps"], sc["mps"]])
    twice["pos"][2000:] += np.float32(0.02)
    for i in range(2000, 4000):
        for b in rng.choice(256, 8, replace=False):
            twice["desc"][i][b >> 3] ^= np.uint8(1 << (b & 7))
    max_kf = 24
    kfs = [Frame(base.keys.copy(), base.desc.copy(), base.u_right.copy(), np.eye(4), base.cam) for _ in range(max_kf)]
    Scw = np.zeros((max_kf, 12), np.float32)
    for k in range(max_kf):
        S = sc["Scw"].copy()
        S[:, 3] += rng.normal(0, 0.01, 3).astype(np.float32)
        Scw[k] = S.reshape(12)
    views = (FrameView * max_kf)()
    for k in range(max_kf):
        views[k] = kfs[k].view()
    vsize = C.sizeof(FrameView)

    lines = [f"orbmi_fuse_sim3_search_batch, th 4, keyframes of {len(base.keys)} keypoints; windows of {a.calls} back-to-back "
             f"calls after 10 warm-up calls, {a.windows} windows; host arrays in and out, nfused read back",
             "every figure below is measured by this run (HIP events on the matcher's stream: the staging copies, both "
             "launches, the read-back and the host's gaps between calls are inside; wall: perf_counter around the same "
             "calls, ctypes included); nothing here is an estimate, and no other program was timed on these sizes"]
    for n in (500, 4000):
        mps = np.ascontiguousarray(twice[:n] if n > 2000 else sc["mps"][:n])
        want = fref.fuse_sim3_search(kfs[0], Scw[0].reshape(3, 4), mps, None, 4.0)[0]
        for nkf in (1, 8, 24):
            bi, bd = np.zeros(nkf * n, np.int32), np.zeros(nkf * n, np.int32)
            nf = np.zeros(nkf, np.int32)

            def batched():
                rc = L.orbmi_fuse_sim3_search_batch(m._h, nkf, C.addressof(views), Scw.ctypes.data, mps.ctypes.data, None, n,
                                                    4.0, bi.ctypes.data, bd.ctypes.data, nf.ctypes.data)
                assert rc == 0

            def singles():
                for k in range(nkf):
                    rc = L.orbmi_fuse_sim3_search_batch(m._h, 1, C.addressof(views) + k * vsize, Scw.ctypes.data + 48 * k,
                                                        mps.ctypes.data, None, n, 4.0, bi.ctypes.data + 4 * k * n,
                                                        bd.ctypes.data + 4 * k * n, nf.ctypes.data + 4 * k)
                    assert rc == 0
            batched()
            ref_bi, ref_nf = bi.copy(), nf.copy()
            assert np.array_equal(ref_bi[:n], want)
            singles()
            assert np.array_equal(bi, ref_bi) and np.array_equal(nf, ref_nf)
            db, wb = timed(batched)
            lines += [f"{n} points x {nkf} keyframe(s) (fused per keyframe: {int(nf.min())} .. {int(nf.max())})",
                      f"  one batched call      stream {fmt(db)}", f"                        wall   {fmt(wb)}"]
            if nkf > 1:
                ds, ws = timed(singles)
                lines += [f"  {nkf} single calls       stream {fmt(ds)}", f"                        wall   {fmt(ws)}",
                          f"  batched / singles (medians): stream {statistics.median(db) / statistics.median(ds):.2f}, "
                          f"wall {statistics.median(wb) / statistics.median(ws):.2f}"]
    m.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
