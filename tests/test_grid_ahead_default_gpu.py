"""The pipelined tracker builds each frame's keypoint grid on the extraction stream by default
(ORBMI_GRID_AHEAD unset = 1); ORBMI_GRID_AHEAD=0 builds it on the tracking stream.  The bench's
frames tracked at both settings leave the same outputs, array for array (bench.track_outputs)."""
import argparse

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


class _NoMapper:  # bench.track_outputs reads the LocalMapping results too; none here
    last = None

    def last_job_outputs(self):
        return None


def test_grid_ahead_default_equals_tracking_stream_grid(monkeypatch):
    import bench
    got = {}
    for setting in (None, "0"):
        if setting is None:
            monkeypatch.delenv("ORBMI_GRID_AHEAD", raising=False)
        else:
            monkeypatch.setenv("ORBMI_GRID_AHEAD", setting)
        S = bench.setup_track(argparse.Namespace(frames=4, nfeatures=500), 0, 0)
        tr, cam, F = S["tr"], S["cam"], 4
        try:
            assert tr.grid_ahead == (setting is None)
            img_bytes = cam.height * cam.width
            outs = []
            for i in range(5):  # both frame slots, each reused (a slot's grid rebuilt behind its searches)
                f = 2 + i % F
                tr.track(S["imgs"].data_ptr() + f * 2 * img_bytes, cam.height, cam.width, S["tcws"][f],
                         S["lf_views"][f - 1], S["lf_pts"][f - 1].data_ptr(), S["mps"][f].data_ptr(), S["n_mp"][f])
                if i >= 3:
                    outs.append(bench.track_outputs(tr, _NoMapper()))
            got[setting] = outs
        finally:
            tr.close()
    for a, b in zip(got[None], got["0"]):
        assert a.keys() == b.keys()
        for k in a:
            np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=k)
        assert a["track_counts"][0] >= 20  # the searches found the frame
