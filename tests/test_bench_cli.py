"""bench.py's command line and its --dump-outputs writer (host code only, no GPU)."""
import sys

import numpy as np
import pytest


@pytest.fixture()
def bench(monkeypatch):
    import bench as B
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    return B


def test_plain_run_is_the_default(bench, monkeypatch):
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.mode == "track" and a.gpus == 1
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3", "--full",
                                      "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d" and a.steps == 7 and a.warmup == 3


def test_keypoints_as_float32(bench):
    from orb_slam2_with_comment_amd.types import KP_DTYPE
    k = np.zeros(3, KP_DTYPE)
    k["x"], k["y"], k["size"] = [1.5, 2.25, 1240.0], [0.0, 375.0, 7.125], 31.0
    k["angle"], k["response"] = [0.0, 359.99, 12.5], [20.0, 255.0, 7.0]
    k["octave"], k["class_id"] = [0, 7, 3], -1
    f = bench.keypoints_f32(k.view(np.int32).reshape(3, 7))
    assert f.dtype == np.float32 and f.shape == (3, 7)
    for j, name in enumerate(KP_DTYPE.names):
        np.testing.assert_array_equal(f[:, j], k[name].astype(np.float32))


def test_dump_outputs_writes_float_arrays(bench, tmp_path):
    arrays = {"idx": np.array([-1, 0, 2063], np.int32), "desc": np.arange(64, dtype=np.uint8).reshape(2, 32),
              "flag": np.array([True, False]), "pose": np.eye(4, dtype=np.float32),
              "chi2": np.array([1.0 / 3.0, 2e300]), "counts": [3, 4]}
    d = tmp_path / "out" / "dir"
    bench.dump_outputs(str(d), arrays)
    assert sorted(p.name for p in d.iterdir()) == sorted(n + ".npy" for n in arrays)
    for n, v in arrays.items():
        got = np.load(d / (n + ".npy"))
        assert got.dtype == (np.float64 if n == "chi2" else np.float32)
        np.testing.assert_array_equal(got, np.asarray(v).astype(got.dtype))


def test_dump_outputs_refuses_more_than_64_mb(bench, tmp_path, monkeypatch):
    assert bench.DUMP_LIMIT_BYTES == 64 << 20
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1024)
    with pytest.raises(RuntimeError):
        bench.dump_outputs(str(tmp_path), {"a": np.zeros(200, np.float32), "b": np.zeros(100, np.float32)})


@pytest.mark.gpu
def test_plain_run_dumps_its_last_step(tmp_path, oracle):
    """A plain `bench.py --steps 6 --warmup 2 --dump-outputs DIR`: one line with the headline
    fields and none of --full's, six timed steps, and float arrays whose features are those of
    the last timed step's frame (step 5 of 4 resident frames = frame 3 of the sequence),
    bit-exact with the oracle's like every extraction."""
    import json
    import os
    import subprocess
    from orb_slam2_with_comment_amd import synth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2",
                        "--frames", "4", "--dump-outputs", str(d)], cwd=root, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 6 and out["warmup"] == 2 and out["full"] is False and out["n_gpus"] == 1
    assert out["unit"] == "frames/s" and out["higher_is_better"] is True and out["dtype"] == "u8"
    assert out["ms_per_step"] > 0 and abs(out["value"] * out["ms_per_step"] / 1e3 - 1) < 1e-3
    for moved in ("cpu_baseline", "pcie_inclusive", "roofline", "stage_ms_per_step", "phase_ms_per_frame"):
        assert moved not in out
    arrays = {f.name[:-4]: np.load(f) for f in d.iterdir()}
    assert all(v.dtype in (np.float32, np.float64) for v in arrays.values())
    assert sum(v.nbytes for v in arrays.values()) <= 64 << 20
    L, R, _ = synth.stereo_pair(synth.KITTI, 3, seed_base=1000)
    par = oracle.params(2000)
    for side, img in (("left", L), ("right", R)):
        k, desc = oracle.extract(par, img)
        ref = np.stack([k[name].astype(np.float32) for name in k.dtype.names], axis=1)
        np.testing.assert_array_equal(arrays[side + "_keypoints"], ref)
        np.testing.assert_array_equal(arrays[side + "_descriptors"], desc.astype(np.float32))
    n = len(arrays["left_keypoints"])
    for name in ("u_right", "depth", "match_last_frame", "match_local_map", "outlier"):
        assert arrays[name].shape == (n,)
    c = arrays["track_counts"]
    assert c[0] >= 20 and c[2] >= 10 and c[3] >= 30   # the frame tracked (results()'s ok)
    assert int((arrays["match_last_frame"] >= 0).sum()) + int((arrays["match_local_map"] >= 0).sum()) >= c[3]
    np.testing.assert_array_equal(arrays["tcw"][3], [0, 0, 0, 1])
    assert arrays["local_ba_tcw"].shape == (24, 4, 4) and arrays["local_ba_points"].shape == (3000, 3)
    # the last keyframe among steps 0..5 is step 4's (every 4th step) = frame 2 of the sequence; its
    # neighbours are the other resident frames (4 + 2 frames are resident, so 5 of the up to 9)
    n_kf = len(oracle.extract(par, synth.stereo_pair(synth.KITTI, 2, seed_base=1000)[0])[0])
    assert arrays["triangulation_ok"].shape == arrays["triangulation_match"].shape == (5, n_kf)
    assert arrays["new_points"].shape == (5, n_kf, 3)
    assert (arrays["new_points"][arrays["triangulation_ok"] == 0] == 0).all()
