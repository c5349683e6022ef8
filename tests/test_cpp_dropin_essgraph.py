"""orbmi::Optimizer::OptimizeEssentialGraph of include/orbmi.hpp: tests/cpp/dropin_essgraph.cpp builds
against liborbmi.so (CPU: compile + link only) and, on the GPU, gives the arrays of the C call bit
for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import essgraph_reference as ref  # noqa: E402
from test_cpp_dropin import build_dropin  # noqa: E402


def test_cpp_essgraph_layer_compiles_and_links(tmp_path):
    from orb_slam2_with_comment_amd import build
    build.build()
    assert os.path.exists(build_dropin(str(tmp_path), "dropin_essgraph"))


@pytest.mark.gpu
def test_cpp_dropin_optimize_essential_graph(tmp_path):
    from orb_slam2_with_comment_amd.optimizer import EssentialGraphOptimizer
    exe = build_dropin(str(tmp_path), "dropin_essgraph")
    P = ref.problem(ref.PROBLEMS[0])
    nv = len(P.vertices)
    rng = np.random.default_rng(2)
    pts = rng.normal(0, 5, (65, 3)).astype(np.float32)
    refs = rng.integers(0, nv, 65).astype(np.int32)
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.array([nv, P.fixed, len(P.v0), P.fix_scale, 20], "<i4").tobytes())
        f.write(np.ascontiguousarray(P.vertices, "<f8").tobytes())
        f.write(np.ascontiguousarray(P.v0, "<i4").tobytes())
        f.write(np.ascontiguousarray(P.v1, "<i4").tobytes())
        f.write(np.ascontiguousarray(P.meas, "<f8").tobytes())
        f.write(np.array([len(pts)], "<i4").tobytes())
        f.write(pts.tobytes())
        f.write(refs.tobytes())
    subprocess.run([exe, str(inp), str(out)], check=True, timeout=120)
    b = out.read_bytes()
    opt = EssentialGraphOptimizer()
    r = opt.run(P.vertices, P.fixed, P.v0, P.v1, P.meas, P.fix_scale)
    Swc = ref.s_inverse(r["vertices"])
    moved, T = opt.correct_points_sim3(pts, refs, P.vertices, Swc, r["vertices"])
    opt.close()
    want = (r["vertices"].tobytes() + T.tobytes() + np.array([r["chi2_before"], r["chi2_after"]]).tobytes() +
            np.array([r["iterations"], r["status"]], "<i4").tobytes() + moved.tobytes())
    assert b == want
    assert r["chi2_after"] < r["chi2_before"]
