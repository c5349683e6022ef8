"""Time stereo rectification on the GPU.  orbmi_remap_pair at 752 x 480 (the EuRoC rig of
tests/golden/settings/EuRoC.yaml, device images in and out, the caller's stream): HIP events around
windows of back-to-back calls after a warm-up, beside the wall time per call; the algorithmic bytes
of a pair over that time.  With --loop, the native loop on the 12 raw frames of
synth.raw_stereo_pair (NativeStereoSLAM(rectify=True)) beside a plain handle on the same frames
rectified beforehand, alternating, in frames per second.

    python tools/rectify_bench.py [--windows 7] [--calls 500] [--loop] [--repeats 5] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def pair_bytes(rows, cols):
    """Algorithmic traffic of one pair: per destination pixel an 8-byte record and one byte
    stored, and each source image read once."""
    return 2 * (rows * cols * (8 + 1) + rows * cols)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch
    import rectify_reference as RR
    import rectify_scenes as SC
    from orb_slam2_with_comment_amd.rectify import StereoRectifier

    s = SC.euroc_settings()
    L, R, _ = SC._raw(0)
    rect = StereoRectifier(s, 0)
    tl, tr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    out = (torch.empty_like(tl), torch.empty_like(tr))
    # a stream of the caller's: the handle's stream waits for it and it waits for the handle's, and
    # no call blocks the host (torch's default stream has no handle to pass: rectify._call_stream)
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    with torch.cuda.stream(side):
        rect(tl, tr, out=out)
        side.synchronize()
        (l1, l2), (r1, r2) = rect.maps()
        assert np.array_equal(out[0].cpu().numpy(), RR.remap(L, l1, l2)) and np.array_equal(out[1].cpu().numpy(), RR.remap(R, r1, r2))
        for _ in range(100):
            rect(tl, tr, out=out)
        side.synchronize()
        dev_us, wall_us, busy = [], [], 0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(a.windows):
            e0.record(side)
            t0 = time.perf_counter()
            for _ in range(a.calls):
                rect(tl, tr, out=out)
            wall = time.perf_counter() - t0
            busy += not side.query()  # work still pending when the last call returned: the calls did not wait
            e1.record(side)
            e1.synchronize()
            dev_us.append(e0.elapsed_time(e1) * 1e3 / a.calls)
            wall_us.append(wall * 1e6 / a.calls)
    rows, cols = L.shape
    nbytes = pair_bytes(rows, cols)
    med = statistics.median(dev_us)
    lines = [f"orbmi_remap_pair: {cols} x {rows} pair, device images in and out on the caller's stream (a torch side stream; "
             f"it was still busy when the last call of {busy} of {a.windows} windows returned)",
             f"  windows of {a.calls} back-to-back calls after 100 warm-up calls, {a.windows} windows",
             f"  stream time per pair (HIP events; the launch, the two stream hand-overs and the host's gaps included): "
             f"median {med:.1f} us, min {min(dev_us):.1f}, max {max(dev_us):.1f}",
             f"  wall time per call (Python binding included): median {statistics.median(wall_us):.1f} us, "
             f"min {min(wall_us):.1f}, max {max(wall_us):.1f}",
             f"  algorithmic bytes per pair {nbytes} ({nbytes / 1e6:.2f} MB): {nbytes / med / 1e3:.1f} GB/s over the median stream time"]
    rect.close()
    if a.loop:
        from orb_slam2_with_comment_amd.native_slam import NativeStereoSLAM
        from slam_backends import small_vocabulary
        raw = [(fr[0], fr[1]) for fr in SC.raw_frames()]
        pre = SC.rectified_frames()
        voc = small_vocabulary()

        def run(frames, rectify):
            slam = NativeStereoSLAM(s, device=0, vocabulary=voc, rectify=rectify)
            t0 = time.perf_counter()
            for f, (iL, iR) in enumerate(frames):
                slam.TrackStereo(iL, iR, f / 20.0, next_pair=frames[f + 1] if f + 1 < len(frames) else None)
            dt = time.perf_counter() - t0
            kf = slam.counts()["keyframes"]
            slam.Shutdown()
            return len(frames) / dt, kf
        run(raw, True), run(pre, False)  # warm-up: code objects, buffers
        fa, fb = [], []
        for _ in range(a.repeats):
            fa.append(run(raw, True)[0])
            fb.append(run(pre, False)[0])
        lines += [f"native loop, {len(raw)} frames of the raw EuRoC-shaped sequence, next_pair driver, synchronous LocalMapping, "
                  f"{a.repeats} alternating repeats after one warm-up run each (handle creation excluded)",
                  f"  rectify=True on raw frames: median {statistics.median(fa):.1f} frames/s, min {min(fa):.1f}, max {max(fa):.1f}",
                  f"  plain handle on frames rectified beforehand: median {statistics.median(fb):.1f} frames/s, "
                  f"min {min(fb):.1f}, max {max(fb):.1f}"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
