#!/usr/bin/env python
"""bench.py — MI355X Track+LocalMap throughput (BASELINE.json metric).

Default workload (`--mode track`, SURVEY.md §8(d) config 2 + amortised config 3): one step =
one KITTI-shaped 1241x376 stereo frame through the GPU hot path, in Tracking's order:
ORBextractor(left) + ORBextractor(right) (2000 features, 1.2, 8 levels, FAST 20/7; one batched
launch sequence) + Frame::ComputeStereoMatches + TrackWithMotionModel (SearchByProjection(CF, LF,
th=7) against the previous frame's stereo points, device-side retry test, PoseOptimization,
outlier discard) + TrackLocalMap (SearchLocalPoints (isInFrustum + SearchByProjection, th=1)
against ~2000 local map points at the optimised pose, PoseOptimization, inlier count); every 4th
frame is a keyframe whose LocalBundleAdjustment
(config 3: 20 free + 4 fixed KFs, 3000 points, ~15k edges) runs concurrently on the
LocalMapping thread, as in the reference.  All LocalBAs started inside the timed region finish
inside it.  Inputs (images, last-frame points, local map) are resident in HBM before timing.

N > 1 (torchrun, one rank per GPU, config 4): every rank tracks its own stereo stream (weak
scaling) and each step all-gathers the streams' left descriptors + keypoints over RCCL and
matches its descriptors against the other streams' (build-defined cross-stream matching).

Other modes: `--mode extract` (extraction + stereo only), `--mode lba` (config 3 alone),
`--mode batch` (config 5: EuRoC-shaped 752x480 mono, 5000 features, 64 frames per launch),
`--mode system` (the whole StereoSLAM host loop -- System::TrackStereo
with the map, keyframes and synchronous LocalMapping + LocalBA on the host around the GPU
operators -- over a rendered sequence with exact ground truth; reports frames/s and ATE).

A plain run sets up, warms up, times `--steps` steps and prints the headline line.  `--full` adds
everything measured beside it, each in runs of its own: the CPU baselines, the per-stage, phase and
roofline profiles, the PCIe-inclusive pass, the idle-GPU keyframe latency (`--mode system`: the
synchronous loop and the Python host loop).  `--dump-outputs DIR` writes what the last timed step
computed as DIR/<name>.npy (float32 / float64); the inputs are seeded, so two builds run with the
same arguments can be compared array for array.

Prints ONE JSON line on rank 0 (contract: task statement; fields documented in DESIGN.md).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import platform
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# One HIP hardware queue per stream of the pipeline (the null stream, extraction E, tracking T,
# the LocalMapping chain, and the native loop's handles): with HIP's default of 4 queues a fifth
# stream shares a queue and its kernels wait behind unrelated work (1,235 -> 1,519
# frames/s measured).  Set before the HIP runtime starts; a larger explicit setting wins.
if int(os.environ.get("GPU_MAX_HW_QUEUES", "4") or 4) < 8:
    os.environ["GPU_MAX_HW_QUEUES"] = "8"

import numpy as np  # noqa: E402
import torch  # noqa: E402  (loaded before liborbmi.so: one HIP runtime in the process)

METRIC = json.load(open(os.path.join(ROOT, "BASELINE.json")))["metric"]
HBM_PEAK_GBS = 8000.0   # MI355X HBM3E (MI355X_MICROARCH.md)
FP64_PEAK_TFS = 78.6    # MI355X FP64 vector
KF_EVERY = 4            # harness keyframe policy (SURVEY.md §8(d) "CPU baseline timing")
_vp = C.c_void_p


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200,
                    help="timed steps.  --mode track / extract time exactly this many; --mode lba times "
                         "max(STEPS // 10, 3) LocalBAs, --mode batch max(STEPS // 10, 5) launches of --batch frames, "
                         "--mode system tracks max(STEPS, 12) frames and times all but the first 10; the line's "
                         "'steps' is the number timed")
    ap.add_argument("--warmup", type=int, default=20,
                    help="untimed steps before them (--mode lba: max(WARMUP // 10, 1) LocalBAs, --mode batch: "
                         "max(WARMUP // 4, 2) launches, --mode system: its first 10 frames)")
    ap.add_argument("--mode", choices=["track", "extract", "lba", "batch", "system"], default="track")
    ap.add_argument("--frames", type=int, default=8, help="distinct stereo frames resident per rank")
    ap.add_argument("--nfeatures", type=int, default=2000)
    ap.add_argument("--batch", type=int, default=64, help="frames per launch in --mode batch")
    ap.add_argument("--cpu-sample-s", type=float, default=15.0)
    ap.add_argument("--no-cpu-baseline", action="store_true",
                    help="with --full: leave the CPU baselines out (a plain run has none)")
    ap.add_argument("--lm-chain", choices=["full", "bow-ba"], default="full",
                    help="per-keyframe LocalMapping work: the whole LocalMapping::Run body, or ComputeBoW + LocalBA")
    ap.add_argument("--dist-backend", default="nccl",
                    help="nccl (= RCCL, one GPU per rank); gloo only to rehearse N > 1 on a 1-GPU box")
    ap.add_argument("--traffic", default=os.path.join(ROOT, "profiles", "r06", "traffic_track.json"),
                    help="per-kernel PMC HBM bytes per launch (tools/pmc_traffic.py)")
    ap.add_argument("--traffic-lba", default=os.path.join(ROOT, "profiles", "r06", "traffic_lba.json"),
                    help="per-kernel PMC HBM bytes per launch of --mode lba (tools/pmc_traffic.py)")
    ap.add_argument("--traffic-batch", default=os.path.join(ROOT, "profiles", "r06", "traffic_batch.json"),
                    help="the same for --mode batch (tools/gpu.sh pmc_batch)")
    ap.add_argument("--frame-events", action="store_true",
                    help="track mode: HIP events around every timed frame's extraction and tracking (their "
                         "overlap in the JSON line's 'overlap'; diagnostics, adds four events per frame)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beside the headline figure: the CPU baselines, the per-stage, phase "
                         "and roofline profiles, the PCIe-inclusive pass, the other configurations of a mode")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy "
                         "(float32 / float64).  Reproducible run to run in every mode but --mode system, whose "
                         "concurrent LocalMapping makes the trajectory depend on timing")
    ap.add_argument("--print-traffic-config", action="store_true",
                    help="print the workload key tools/pmc_traffic.py stores with a traffic summary, and exit")
    return ap.parse_args()


def traffic_config(a):
    """The workload a PMC traffic summary was measured on (stored in it by tools/pmc_traffic.py):
    a summary is reported as roofline.traffic only for the same workload, null otherwise."""
    c = {"mode": a.mode, "nfeatures": a.nfeatures}
    if a.mode == "batch":  # (run_batch: 5000 features whatever --nfeatures says)
        c.update({"nfeatures": 5000, "rows": 480, "cols": 752, "batch": a.batch, "nlevels": 8})
    else:
        c.update({"rows": 376, "cols": 1241, "nlevels": 8})
    if a.mode == "track":
        c["lm_chain"] = a.lm_chain
    return c


def level_geometry(rows, cols, nlevels=8, sf=1.2):
    """Pyramid sizes exactly as ComputePyramid (cvRound((float)cols * invScale))."""
    s = np.float32(1.0)
    W, H = [], []
    for _ in range(nlevels):
        inv = np.float32(1.0) / s
        W.append(int(np.rint(np.float32(cols) * inv)))
        H.append(int(np.rint(np.float32(rows) * inv)))
        s = np.float32(np.float64(s) * np.float64(np.float32(sf)))
    return W, H


def _traffic_summary(path, config):
    """The per-kernel bytes of a tools/pmc_traffic.py summary when it was measured on `config`
    (its stored "config"; a summary without one is not trusted either), else None."""
    if not os.path.exists(path):
        return None
    try:
        d = json.load(open(path))
    except Exception:
        return None
    if config is not None and d.get("config") != config:
        return None
    return d.get("per_launch_bytes", {})


def batch_traffic(path, config, nlevels=8):
    """HBM bytes of one config-5 launch sequence from a tools/pmc_traffic.py summary of the batch
    mode (calibrated FETCH_SIZE / WRITE_SIZE per kernel launch): every stage once, the resize once
    per level above 0; None without the file or when it was measured on another workload."""
    per = _traffic_summary(path, config)
    if per is None:
        return None
    return int(sum(v * (nlevels - 1 if k == "pyr_resize" else 1) for k, v in per.items()))


def frame_overlap(evs):
    """Per-frame timeline from the tracker's events (--frame-events): the tracking stream's idle
    gap before each frame, when the next frame's extraction started relative to this frame's
    tracking start, the extraction span and the wait of tracking on it (µs, median / p90)."""
    base = evs[0][0]
    t = np.array([[base.elapsed_time(e) * 1e3 for e in ev] for ev in evs])  # µs from the first event
    stats = {}

    def put(name, v):
        v = np.sort(np.asarray(v))
        stats[name] = {"median": round(float(v[len(v) // 2]), 1), "p90": round(float(v[int(0.9 * (len(v) - 1))]), 1)}
    put("track_span_us", t[:, 3] - t[:, 2])
    put("track_idle_gap_us", t[1:, 2] - t[:-1, 3])
    put("next_extract_start_after_track_start_us", t[1:, 0] - t[:-1, 2])
    put("extract_span_us", t[:, 1] - t[:, 0])
    put("track_start_after_extract_end_us", t[:, 2] - t[:, 1])
    stats["frames"] = len(evs)
    return stats


def job_overlap(jobs):
    """The LocalMapping jobs' timeline (--frame-events): each job's span on the mapper's stream
    (the first packet to LocalBA's return), the stream's gap between two jobs, and the host's gap
    from one job's LocalBA return to the next job's start (µs, median / p90)."""
    base = jobs[0][0]
    t = np.array([[base.elapsed_time(e0) * 1e3, base.elapsed_time(e1) * 1e3] for e0, e1, _, _, _ in jobs])
    h = np.array([[h0, h1] for _, _, h0, h1, _ in jobs]) * 1e6
    out = {}

    def put(name, v):
        v = np.sort(np.asarray(v))
        if len(v):
            out[name] = {"median": round(float(v[len(v) // 2]), 1), "p90": round(float(v[int(0.9 * (len(v) - 1))]), 1)}
    put("lm_job_span_us", t[:, 1] - t[:, 0])
    put("lm_stream_gap_between_jobs_us", t[1:, 0] - t[:-1, 1])
    put("lm_host_gap_between_jobs_us", h[1:, 0] - h[:-1, 1])
    # the job's stages on the stream: each from the previous boundary (LocalBA: to the job's end)
    names = [n for n, _ in jobs[0][4]]
    if names and all([n for n, _ in j[4]] == names for j in jobs):
        for k, n in enumerate(names + ["local_ba"]):
            v = []
            for e0, e1, _, _, mk in jobs:
                a = e0 if k == 0 else mk[k - 1][1]
                b = e1 if k == len(names) else mk[k][1]
                v.append(a.elapsed_time(b) * 1e3)
            put(f"lm_stage_{n}_us", v)
    out["lm_jobs"] = len(jobs)
    return out


def lba_trial_traffic(a):
    """HBM bytes of one LocalBA LM trial (its three launches) from the --mode lba PMC summary,
    None without it or when it was measured on another workload."""
    per = _traffic_summary(a.traffic_lba, traffic_config(a))
    if not per:
        return None
    ks = ("k_ba_schur", "k_ba_solve_mfma", "k_ba_update_errors")
    return int(sum(per[k] for k in ks)) if all(k in per for k in ks) else None


def read_traffic(path, name, config=None):
    per = _traffic_summary(path, config)
    return None if per is None else per.get(name)


DUMP_LIMIT_BYTES = 64 << 20


def keypoints_f32(kps):
    """cv::KeyPoint records (n x 7 int32 words: x, y, size, angle, response as float bits, octave,
    class_id) as n x 7 float32 values."""
    kps = np.ascontiguousarray(kps, np.int32).reshape(-1, 7)
    out = np.empty(kps.shape, np.float32)
    out[:, :5] = kps[:, :5].view(np.float32)
    out[:, 5:] = kps[:, 5:]
    return out


def dump_outputs(path, arrays):
    """--dump-outputs: each array as DIR/<name>.npy, float64 as it is and everything else as
    float32 (indices, counts, flags, descriptor bytes and octaves are all below 2^24: exact)."""
    os.makedirs(path, exist_ok=True)
    total = 0
    for name, v in arrays.items():
        v = np.asarray(v)
        v = np.ascontiguousarray(v, np.float64 if v.dtype == np.float64 else np.float32)
        total += v.nbytes
        if total > DUMP_LIMIT_BYTES:
            raise RuntimeError(f"--dump-outputs: {name} takes the dump past {DUMP_LIMIT_BYTES} bytes")
        np.save(os.path.join(path, name + ".npy"), v)


# --------------------------------------------------------------------------------- track
def setup_track(a, rank, local):
    """Resident inputs for `frames` tracked steps: frames 2..F+1 of the rank's sequence."""
    from orb_slam2_with_comment_amd import synth, synth_map as SM
    from orb_slam2_with_comment_amd.orb import compute_stereo_matches
    from orb_slam2_with_comment_amd.pipeline import StereoTracker, frame_view
    cam = synth.KITTI
    F = a.frames
    seq = [synth.stereo_pair(cam, f, seed_base=1000 * (rank + 1)) for f in range(F + 2)]
    tr = StereoTracker(cam, a.nfeatures, device=local, pipelined=True)
    sf = tr.scale_factors
    # per-frame features through the host API (bit-exact with the oracle, tests/); stereo needs
    # both pyramids resident, so the right images go through a second extractor
    from orb_slam2_with_comment_amd.orb import ORBextractor
    right = ORBextractor(a.nfeatures, 1.2, 8, 20, 7, device=local)
    feats2 = []
    for L, R, T in seq:
        kl, dl = tr.extractor(L)
        right(R)
        u, d = compute_stereo_matches(tr.extractor, right, cam.bf, cam.fx, len(kl))
        feats2.append((L, R, T, kl, dl, u, d))
    right.close()
    rng = np.random.default_rng(7 + rank)
    cap = tr.cap
    dev = torch.device("cuda", local)
    nF = F + 2
    lf_keys = torch.zeros((nF, cap, 7), dtype=torch.int32, device=dev)
    lf_desc = torch.zeros((nF, cap, 32), dtype=torch.uint8, device=dev)
    lf_u = torch.full((nF, cap), -1.0, dtype=torch.float32, device=dev)
    from orb_slam2_with_comment_amd.types import LFPOINT_DTYPE, MAPPOINT_DTYPE
    lf_pts = torch.zeros((nF, cap * LFPOINT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    n_lf, tcws = [], []
    for f, (L, R, T, kl, dl, u, d) in enumerate(feats2):
        n = len(kl)
        n_lf.append(n)
        lf_keys[f, :n] = torch.from_numpy(np.ascontiguousarray(kl).view(np.int32).reshape(n, 7)).to(dev)
        lf_desc[f, :n] = torch.from_numpy(dl).to(dev)
        lf_u[f, :n] = torch.from_numpy(u).to(dev)
        lfp = SM.lastframe_points(kl, dl, d, cam, T, rng, outlier_frac=0.05)
        lf_pts[f, :n * LFPOINT_DTYPE.itemsize] = torch.from_numpy(lfp.view(np.uint8)).to(dev)
        Tn = T.copy()
        Tn[:3, 3] += rng.normal(0, 0.02, 3)  # motion-model pose estimate, a few cm off
        tcws.append(SM.tcw_from_twc(Tn))
    lf_tcw = [SM.tcw_from_twc(x[2]) for x in feats2]
    lf_views = [frame_view(n_lf[f], lf_keys[f].data_ptr(), lf_u[f].data_ptr(), lf_desc[f].data_ptr(), lf_tcw[f], cam,
                           sf, cam.width, cam.height) for f in range(nF)]
    # local map of frame f: points created from frames f-1 and f-2 (~3000)
    mps, n_mp = [], []
    for f in range(nF):
        if f < 2:
            mps.append(None)
            n_mp.append(0)
            continue
        parts = []
        for g in (f - 1, f - 2):
            _, _, T, kl, dl, u, d = feats2[g]
            mp, _ = SM.mappoints_from_frame(kl, dl, d, cam, T, sf, rng, bad_frac=0.02, noobs_frac=0.02)
            parts.append(mp)
        m = np.concatenate(parts)
        mps.append(torch.from_numpy(m.view(np.uint8).copy()).to(dev))
        n_mp.append(len(m))
    imgs = torch.from_numpy(np.stack([np.stack([x[0], x[1]]) for x in feats2])).to(dev)  # nF x 2 x H x W
    torch.cuda.synchronize()
    return dict(cam=cam, tr=tr, imgs=imgs, tcws=tcws, lf_views=lf_views, lf_pts=lf_pts, n_lf=n_lf, mps=mps,
                n_mp=n_mp, feats=feats2, keep=(lf_keys, lf_desc, lf_u, lf_tcw, sf), nF=nF)


def setup_local_mapping(S, voc, vocab, rank, problem, n_neighbours=9, n_target_maps=4):
    """LocalMapping jobs (pipeline.LocalMappingJob) for the resident frames: keyframe f's
    neighbours are the other resident frames (their FeatureVectors computed once), its map points
    the back-projected local map of frame f, the fuse targets' points the local maps of its
    n_target_maps nearest neighbours, and its points' observation descriptors bit-flipped copies
    of the point descriptor (2-6 per point).  Host mirrors ride along for the CPU baseline."""
    from orb_slam2_with_comment_amd.pipeline import KeyFrameData, LocalMappingJob
    from orb_slam2_with_comment_amd.types import MAPPOINT_DTYPE, Frame
    tr, cam = S["tr"], S["cam"]
    dev = tr.kps.device
    sf = np.ascontiguousarray(tr.scale_factors, np.float32)
    sig2 = np.ascontiguousarray(tr.extractor.GetScaleSigmaSquares(), np.float32)
    lf_keys, lf_desc, lf_u, lf_tcw, _ = S["keep"]
    nF, cap = S["nF"], tr.cap
    rng = np.random.default_rng(11 + rank)
    has_mp_h = (rng.random((nF, cap)) < 0.4).astype(np.uint8)  # GetMapPoint(i) != NULL
    has_mp = torch.from_numpy(has_mp_h).to(dev)
    kfd, host = [], []
    for f in range(nF):
        _, _, _, kl, dl, u, d = S["feats"][f]
        _, _, fv = voc.transform(dl, 4)
        kfd.append(KeyFrameData(cam, sf, sig2, len(kl), lf_keys[f].data_ptr(), lf_desc[f].data_ptr(),
                                lf_u[f].data_ptr(), has_mp[f].data_ptr(), kl, u, d, lf_tcw[f], fv=fv))
        host.append(dict(frame=Frame(kl, dl, u, lf_tcw[f], cam), has_mp=has_mp_h[f, :len(kl)].copy(), fv=fv))
    jobs, keep = {}, [has_mp]
    for f in range(2, nF):
        nbrs = sorted((g for g in range(nF) if g != f), key=lambda g: (abs(g - f), g))[:n_neighbours]
        mp_h = S["mps"][f].cpu().numpy().view(MAPPOINT_DTYPE)
        tgt = [g for g in nbrs if S["mps"][g] is not None][:n_target_maps]
        tp_h = np.concatenate([S["mps"][g].cpu().numpy().view(MAPPOINT_DTYPE) for g in tgt])
        d_tp = torch.from_numpy(tp_h.view(np.uint8).copy()).to(dev)
        nobs = rng.integers(2, 7, len(mp_h))
        off = np.concatenate([[0], np.cumsum(nobs)]).astype(np.int32)
        obs = np.repeat(mp_h["desc"], nobs, axis=0)
        flip = (rng.random(obs.shape) < 0.08) * (1 << rng.integers(0, 8, obs.shape))  # one bit in ~8 % of bytes
        obs = (obs ^ flip.astype(np.uint8)).astype(np.uint8)
        d_obs, d_off = torch.from_numpy(obs.copy()).to(dev), torch.from_numpy(off).to(dev)
        keep += [d_tp, d_obs, d_off]
        job = LocalMappingJob(kfd[f], lf_desc[f].data_ptr(), [kfd[g] for g in nbrs],
                              (S["mps"][f].data_ptr(), len(mp_h)), (d_tp.data_ptr(), len(tp_h)),
                              (d_obs.data_ptr(), d_off.data_ptr(), len(mp_h)), problem)
        job.host = dict(kf=host[f], neighbours=[host[g] for g in nbrs], kf_points=mp_h, target_points=tp_h,
                        obs_desc=obs, obs_off=off, desc=S["feats"][f][4])
        jobs[f] = job
    torch.cuda.synchronize()
    return jobs, (kfd, keep)


def cpu_local_mapping(O, vocab, job):
    """The same LocalMapping::Run iteration as pipeline.LocalMapper.run_job on the oracle
    (the host triangulation geometry is liborbmi.so's host code, shared with the GPU loop)."""
    import ctypes as C_
    from orb_slam2_with_comment_amd._capi import check, lib
    from orb_slam2_with_comment_amd.types import FeatureVector
    h = job.host
    _, _, node, off, feat = O.transform(vocab, h["desc"], 4)
    fv = FeatureVector.from_csr(node, off, feat)
    O.compute_distinctive_descriptors(h["obs_desc"], h["obs_off"])
    n_new = 0
    has1 = h["kf"]["has_mp"].copy()  # KF1's map points as the earlier pairs leave them
    for j, nb in enumerate(h["neighbours"]):
        m12, _ = O.search_for_triangulation(h["kf"]["frame"], has1, fv, nb["frame"], nb["has_mp"], nb["fv"],
                                            job.F12[j].reshape(3, 3), False, False)
        idx1 = np.nonzero(m12 >= 0)[0].astype(np.int32)
        if len(idx1):
            idx2 = np.ascontiguousarray(m12[idx1], np.int32)
            x3d = np.zeros((len(idx1), 3), np.float32)
            ok = np.zeros(len(idx1), np.uint8)
            check("orbmi_triangulate_matches", lib().orbmi_triangulate_matches(
                C_.addressof(job.kf.tri), C_.addressof(job.neighbours[j].tri), idx1.ctypes.data, idx2.ctypes.data,
                len(idx1), x3d.ctypes.data, ok.ctypes.data))
            has1[idx1[ok == 1]] = 1
            n_new += int(ok.sum())
    for nb in h["neighbours"]:
        O.fuse_search(nb["frame"], h["kf_points"], None, 3.0)
    O.fuse_search(h["kf"]["frame"], h["target_points"], None, 3.0)
    O.compute_distinctive_descriptors(h["obs_desc"], h["obs_off"])
    O.local_ba(job.problem)
    return n_new


def track_outputs(tr, mapper):
    """What a caller of the timed path holds after its last step (--dump-outputs): the last
    tracked frame's features and stereo matches, its matches, outlier flags, poses and counts, and
    what the last keyframe's LocalMapping chain found and its LocalBA returned."""
    r = tr.results()
    nl, nr = (int(x) for x in tr.counts.cpu().numpy())
    kps, desc = tr.kps.cpu().numpy(), tr.desc.cpu().numpy()
    out = {"left_keypoints": keypoints_f32(kps[0, :nl]), "right_keypoints": keypoints_f32(kps[1, :nr]),
           "left_descriptors": desc[0, :nl], "right_descriptors": desc[1, :nr],
           "u_right": tr.u_right[0, :nl].cpu().numpy(), "depth": tr.depth[0, :nl].cpu().numpy(),
           "match_last_frame": tr.match_lf[:nl].cpu().numpy(), "match_local_map": tr.match_mp[:nl].cpu().numpy(),
           "outlier": tr.outlier[:nl].cpu().numpy(), "tcw_motion_model": r["tcw_mm"], "tcw": r["tcw"],
           "track_counts": [r["search_matches"], r["outliers_mm"], r["nmatches_map"], r["inliers"], r["outliers"]]}
    ba = mapper.last
    if ba is not None:
        out.update({"local_ba_tcw": ba["tcw"], "local_ba_points": ba["pos"], "local_ba_erase": ba["erase"],
                    "local_ba_chi2": np.array(ba["chi2"], np.float64), "local_ba_iterations": ba["iterations"]})
    o = mapper.last_job_outputs()
    if o is not None:  # CreateNewMapPoints' pairs and accepted points, the Fuse searches' candidates
        out.update({"triangulation_match": o["tri"], "triangulation_ok": o["tri_ok"], "new_points": o["x3d"],
                    "fuse_match": o["fuse_match"]})
    return out


def pcie_inclusive_pass(a, S, tr, step, sync, ext, h_imgs, dist, world):
    """The PCIe-inclusive pass (not `value`: the contract's value has the inputs resident in HBM):
    the same steps with each stereo pair DMA'd from pinned host memory, overlapped with the
    previous frame's tracking; and the DMA alone, synchronised, per pair."""
    rows, cols, F = S["cam"].height, S["cam"].width, a.frames
    img_bytes = rows * cols
    ext_ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    sync()
    ext_ev[0].record(ext)
    for i in range(16):
        tr.extract_stereo(S["imgs"].data_ptr() + (2 + i % F) * 2 * img_bytes, rows, cols)
    ext_ev[1].record(ext)
    for i in range(16):
        tr.extract_stereo(h_imgs.ptr + (2 + i % F) * 2 * img_bytes, rows, cols, host=True)
    ext_ev[2].record(ext)
    sync()
    upload_ms = (ext_ev[1].elapsed_time(ext_ev[2]) - ext_ev[0].elapsed_time(ext_ev[1])) / 16
    if dist:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    host_up = 0.0
    for i in range(a.steps):
        th = time.perf_counter()
        step(i, host=True)
        host_up += time.perf_counter() - th
    t_enq_up = time.perf_counter() - t0
    sync()
    if dist:
        dist.barrier()
    dt_up = max_over_ranks(time.perf_counter() - t0, dist)
    return {"value": round(a.steps * world / dt_up, 3), "unit": "frames/s", "ms_per_step": round(dt_up / a.steps * 1e3, 4),
            "upload_bytes_per_frame": 2 * img_bytes,
            "host_enqueue_ms_per_step": round(host_up / a.steps * 1e3, 4),
            "host_enqueued_all_ms": round(t_enq_up * 1e3, 3), "upload_ms_per_frame_alone": round(upload_ms, 4),
            "upload_GBps_alone": round(2 * img_bytes / (upload_ms * 1e-3) / 1e9, 2),
            "how": "each step's stereo pair read from pinned host memory by a copy kernel on the extraction stream "
                   "(orbmi_extract_batch_host), ahead of its extraction and overlapped with the previous frame's "
                   "tracking; upload_ms_per_frame_alone = extraction from host minus from HBM, back to back"}


def run_track(a, rank, world, local, dist):
    from orb_slam2_with_comment_amd import synth_map as SM
    from orb_slam2_with_comment_amd.pipeline import LocalMapper, StreamExchange
    S = setup_track(a, rank, local)
    cam, tr = S["cam"], S["tr"]
    rows, cols = cam.height, cam.width
    img_bytes = rows * cols
    F = a.frames
    problem, _ = SM.local_ba_problem(seed=42)
    # KeyFrame::ComputeBoW on the LocalMapping thread needs an ORB vocabulary: synthetic, of the
    # ORB vocabulary's shape (k = 10, L = 6, 1.1 M nodes; the file is not available offline)
    from orb_slam2_with_comment_amd.vocabulary import ORBVocabulary, Vocabulary
    vocab = Vocabulary.synthetic(k=10, L=6, seed=7)
    S["vocab"] = vocab
    voc = ORBVocabulary(vocab, device=local)
    # (ComputeBoW on the extraction stream, orbmi_vocabulary_share_stream, was measured slower:
    # 1,489 vs 2,517 frames/s -- the transform then queues behind the frames the host enqueued
    # ahead, and the LocalMapping thread waits for it)
    # ComputeBoW ahead takes one more stream (the vocabulary's); with N > 1 the exchange stream and
    # RCCL's add theirs, so there it stays off unless ORBMI_LM_PREBOW says otherwise (the streams
    # then stay within the 4 hardware queues the gloo rehearsal ran with)
    prebow = os.environ.get("ORBMI_LM_PREBOW", "1" if world == 1 else "0") == "1"
    mapper = LocalMapper(local, vocabulary=voc, prebow=prebow)
    kf_desc = lambda f: (S["keep"][1][f].data_ptr(), S["n_lf"][f])  # noqa: E731  (the keyframe's descriptors)
    # the whole LocalMapping::Run body per keyframe (ProcessNewKeyFrame, CreateNewMapPoints,
    # SearchInNeighbors, LocalBundleAdjustment); --lm-chain bow-ba keeps round 2's ComputeBoW + LocalBA
    jobs, S["lm_keep"] = setup_local_mapping(S, voc, vocab, rank, problem)
    S["jobs"] = jobs
    full_chain = a.lm_chain == "full"
    keyframe = (lambda f: mapper.insert_keyframe(jobs[f])) if full_chain else \
        (lambda f: mapper.insert_keyframe(problem, kf_desc(f)))
    xch = StreamExchange(tr, dist, local) if dist is not None else None  # config 4
    ext = torch.cuda.ExternalStream(tr.stream_handle, device=tr.kps.device)        # extraction (E)
    trk = torch.cuda.ExternalStream(tr.track_stream_handle, device=tr.kps.device)  # tracking (T)

    # the same frames in pinned host memory: the PCIe-inclusive pass DMAs each step's stereo pair
    # to HBM on the extraction stream (stereo_kitti.cc:81-97 times TrackStereo from a host image)
    h_imgs = None
    if a.full:
        from orb_slam2_with_comment_amd import _hip
        h_imgs = _hip.PinnedBytes(S["imgs"].numel())
        h_imgs.array[:] = S["imgs"].cpu().numpy().reshape(-1)

    def step(i, host=False):
        f = 2 + i % F
        src = (h_imgs.ptr if host else S["imgs"].data_ptr()) + f * 2 * img_bytes
        tr.track(src, rows, cols, S["tcws"][f], S["lf_views"][f - 1], S["lf_pts"][f - 1].data_ptr(),
                 S["mps"][f].data_ptr(), S["n_mp"][f], host=host)
        if xch is not None:  # config 4: exchange left features, match against the other streams
            xch.exchange()
        if i % KF_EVERY == 0:
            keyframe(f)

    def sync():
        tr.synchronize()
        if xch is not None:
            xch.synchronize()
        mapper.wait()
        torch.cuda.synchronize()

    for i in range(a.warmup):
        step(i)
    sync()
    full = a.full  # everything beside the headline figure (a plain run only times the steps)
    if full:
        # one keyframe alone (the LocalMapping chain): its latency on an otherwise idle GPU
        t0 = time.perf_counter()
        keyframe(2)
        mapper.wait()
        lba_ms = (time.perf_counter() - t0) * 1e3
        lba_info = mapper.last
        chain_info = dict(mapper.last_chain.materialize()) if full_chain else None
        t0 = time.perf_counter()
        for _ in range(10):
            b = mapper.bow
            voc.transform_device(kf_desc(2)[0], kf_desc(2)[1], None, 4, b["word"].data_ptr(), b["value"].data_ptr(),
                                 b["node"].data_ptr(), b["off"].data_ptr(), b["feat"].data_ptr(),
                                 b["counts"].data_ptr())
            voc.synchronize()
        bow_us = (time.perf_counter() - t0) / 10 * 1e6
        bow_words = int(mapper.bow["counts"][0])

        # per-stage profile (untimed): extractor stages via the library's event brackets
        stage = profile_stages(tr.extractor.handle, lambda i: (tr.extract_stereo(
            S["imgs"].data_ptr() + (2 + i % F) * 2 * img_bytes, rows, cols), tr.synchronize()), max(F, 16))
        # phase profile (untimed): HIP events on the tracking stream around each phase
        n_tr = max(F, 32)
        phases = {"extract_stereo": 0.0, "track_motion_model": 0.0, "track_local_map": 0.0}
        tr.synchronize()
        t0 = time.perf_counter()
        for i in range(n_tr):
            f = 2 + i % F
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record(ext)
            tr.extract_stereo(S["imgs"].data_ptr() + f * 2 * img_bytes, rows, cols)
            ev[1].record(ext)
            trk.wait_event(ev[1])
            tr.track_with_motion_model(S["tcws"][f], S["lf_views"][f - 1], S["lf_pts"][f - 1].data_ptr())
            ev[2].record(trk)
            tr.track_local_map(S["lf_views"][f - 1], S["lf_pts"][f - 1].data_ptr(), S["mps"][f].data_ptr(),
                               S["n_mp"][f])
            ev[3].record(trk)
            tr.synchronize()
            for k, name in enumerate(phases):
                phases[name] += ev[k].elapsed_time(ev[k + 1]) / n_tr
        track_only_ms = (time.perf_counter() - t0) / n_tr * 1e3  # includes a host sync per frame
        # tracking alone, back to back (no LocalBA): host enqueue time vs GPU-bound time per frame
        tr.synchronize()
        t0 = time.perf_counter()
        for i in range(n_tr):
            f = 2 + i % F
            tr.track(S["imgs"].data_ptr() + f * 2 * img_bytes, rows, cols, S["tcws"][f], S["lf_views"][f - 1],
                     S["lf_pts"][f - 1].data_ptr(), S["mps"][f].data_ptr(), S["n_mp"][f])
        enqueue_ms = (time.perf_counter() - t0) / n_tr * 1e3
        tr.synchronize()
        track_async_ms = (time.perf_counter() - t0) / n_tr * 1e3
        outcome = tr.results()
        nm_lf = int((tr.match_lf[:int(tr.counts[0])] >= 0).sum())
        nm_mp = int((tr.match_mp[:int(tr.counts[0])] >= 0).sum())
        kp_per_frame = float(stage["kp_per_step"])

    # ---- timed region
    lib = __import__("orb_slam2_with_comment_amd._capi", fromlist=["lib"]).lib()
    if full:
        dom = stage["dominant"]
        lib.orbmi_set_profiling(tr.extractor.handle, 1 << stage["dominant_id"])
        reset_profile(tr.extractor.handle)
        # the path's dominant kernel (rocprofv3, profiles/): PoseOptimization, bracketed with HIP
        # events on the tracking stream it is launched on
        # (every POSE_PROF_STRIDE-th launch: a timed event pair is two queue packets of ~6 µs each on
        # the tracking stream; an odd stride alternates TrackWithMotionModel's and TrackLocalMap's)
        lib.orbmi_pose_set_profiling(tr.pose._h, POSE_PROF_STRIDE)
        pose_prof = read_pose_profile(lib, tr.pose._h)
    sync()
    if dist:
        dist.barrier()
    sync()
    if a.frame_events:
        tr.frame_events = []
        mapper.job_events = []
    t0 = time.perf_counter()
    host_s = 0.0  # time the host spends enqueueing (a host-bound step shows host ~ wall)
    for i in range(a.steps):
        th = time.perf_counter()
        step(i)
        host_s += time.perf_counter() - th
    t_enq = time.perf_counter()
    if a.frame_events:  # which chain ends the timed region: tracking or the LocalMapping jobs
        tr.synchronize()
        t_trk = time.perf_counter()
        mapper.wait()
        t_map = time.perf_counter()
    sync()
    if dist:
        dist.barrier()
    dt = time.perf_counter() - t0
    if full:
        ms, nl = read_profile(tr.extractor.handle)
        lib.orbmi_set_profiling(tr.extractor.handle, 0)
        pose_prof = read_pose_profile(lib, tr.pose._h)
        lib.orbmi_pose_set_profiling(tr.pose._h, 0)
    dt = max_over_ranks(dt, dist)
    if a.dump_outputs and rank == 0:  # the last timed step's results, before anything else runs
        dump_outputs(a.dump_outputs, track_outputs(tr, mapper))
    overlap = frame_overlap(tr.frame_events) if tr.frame_events else None
    if overlap:
        overlap.update({"host_enqueued_ms": round((t_enq - t0) * 1e3, 3), "tracking_done_ms": round((t_trk - t0) * 1e3, 3),
                        "mapping_done_ms": round((t_map - t0) * 1e3, 3)})
    if overlap and mapper.job_events:
        overlap.update(job_overlap(mapper.job_events))
    tr.frame_events = None
    mapper.job_events = None
    if full:
        pcie = pcie_inclusive_pass(a, S, tr, step, sync, ext, h_imgs, dist, world)
    n_lba = (a.steps + KF_EVERY - 1) // KF_EVERY
    x_matches = None
    if xch is not None:
        xch.synchronize()
        x_matches = int((xch.xmatch[:int(tr.counts[0])] >= 0).sum())
    value = a.steps * world / dt
    if full:
        ext_roof = roofline_entry(dom, stage, ms[stage["dominant_id"]], nl[stage["dominant_id"]], a.traffic,
                                  traffic_config(a))
        roof = pose_roofline(pose_prof, outcome["recs"], a.traffic, traffic_config(a))
    out = None
    if rank == 0:
        cpu = None
        cpu_tp = None
        if full and not a.no_cpu_baseline and world == 1:
            cpu = cpu_baseline_track(S, problem, a)
            O = oracle_native()
            imgs = [x for fr in S["feats"] for x in fr[:2]]
            cpu_tp = cpu_throughput_extract(O, O.params(a.nfeatures), imgs, min(a.cpu_sample_s, 5))
        out = {
            "metric": METRIC, "value": round(value, 3), "unit": "frames/s", "n_gpus": world, "steps": a.steps,
            "warmup": a.warmup, "ms_per_step": round(dt / a.steps * 1e3, 4), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "u8",
            "data": "synthetic: ray-cast KITTI-shaped 1241x376 stereo sequence + back-projected local map + "
                    "config-3 LocalBA graph, resident in HBM",
            "config": {
                "workload": "Track+LocalMap per stereo frame: ORBextractor(L,R) [2000 feat, 1.2, 8 lv, FAST 20/7] "
                            "+ ComputeStereoMatches + TrackWithMotionModel [SearchByProjection(CF,LF,th=7), "
                            "PoseOptimization] + TrackLocalMap [SearchLocalPoints(th=1, "
                            f"~{int(np.mean([n for n in S['n_mp'] if n]))} MPs), PoseOptimization] "
                            + (f"+ LocalMapping::Run every {KF_EVERY}th frame on the concurrent LocalMapping thread "
                               "[ProcessNewKeyFrame: KeyFrame::ComputeBoW"
                               + (" (a queued keyframe's issued beside the previous LocalBA, on the vocabulary's stream)"
                                  if getattr(mapper, "_prebow", False) else "")
                               + " + ComputeDistinctiveDescriptors; "
                               "CreateNewMapPoints: SearchForTriangulation x9 neighbours + triangulation geometry, all on the device; "
                               "SearchInNeighbors: Fuse x9 targets + Fuse(KF, targets' points) + "
                               "ComputeDistinctiveDescriptors; LocalBundleAdjustment(config 3)]" if full_chain else
                               "+ KeyFrame::ComputeBoW + LocalBundleAdjustment(config 3) "
                               f"every {KF_EVERY}th frame on the concurrent LocalMapping thread")
                            + ("; + RCCL all-gather of left desc/kps and cross-stream matching (config 4)"
                               if world > 1 else ""),
                "frames_resident": F, "parallelism": f"one stereo stream per GPU x{world}",
            },
            "full": full,
            "host_enqueue_ms_per_step_timed": round(host_s / a.steps * 1e3, 4),
            **({"overlap": overlap} if overlap else {}),
            "cross_stream_matches_last_frame": x_matches,
            "host": host_info(),
        }
        if full:
            out.update({
                "kpts_desc_per_s": round(value * kp_per_frame, 1),
                "keypoints_per_frame": round(kp_per_frame, 1),
                "pcie_inclusive": pcie,
                "matches_per_frame": {"last_frame": nm_lf, "local_map": nm_mp, "inliers": outcome["inliers"],
                                      "tracking_ok": outcome["ok"]},
                "phase_ms_per_frame": {k: round(v, 4) for k, v in phases.items()},
                "track_only_ms_per_frame_synced": round(track_only_ms, 4),
                "track_only_ms_per_frame_back_to_back": round(track_async_ms, 4),
                "host_enqueue_ms_per_frame": round(enqueue_ms, 4),
                "compute_bow": {"us_per_keyframe_synced": round(bow_us, 1), "words": bow_words,
                                "vocabulary": "synthetic k=10 L=6 (1,111,111 nodes), L1 / TF-IDF, levelsup 4"},
                "local_mapping": {"ms_per_keyframe_idle_gpu": round(lba_ms, 3), "chain": a.lm_chain,
                                  "keyframes_in_timed_region": n_lba, "last_keyframe": chain_info,
                                  "compute_bow_issued_ahead": getattr(mapper, "bow_ahead", 0)},
                "local_ba": {"calls_in_timed_region": n_lba,
                             "iterations": list(lba_info["iterations"]) if lba_info else None,
                             "edges": int(len(problem.edges)), "points": int(len(problem.pts)),
                             "keyframes": int(len(problem.kfs))},
                "stage_ms_per_step": stage["stage_ms"],
                "roofline": roof,
                "extractor_roofline": ext_roof,
                "pipeline_roofline": pipeline_roofline(stage, rows, cols),
                "cpu_baseline": cpu,
                "cpu_baseline_throughput": cpu_tp,
            })
    if xch is not None:
        xch.close()
    mapper.close()
    tr.close()
    if h_imgs is not None:
        h_imgs.close()
    return out


# --------------------------------------------------------------------------------- helpers
def profile_stages(handle, run_step, n):
    """Per-stage GPU time of the extractor/stereo kernels (library event brackets) and the
    algorithmic bytes of each stage's launch."""
    from orb_slam2_with_comment_amd import _capi
    lib = _capi.lib()
    NS = _capi.NUM_STAGES
    lib.orbmi_set_profiling(handle, 0x1FF)
    reset_profile(handle)
    kp = 0
    cand = 0
    W, H = level_geometry(376, 1241)
    for i in range(n):
        run_step(i)
    ms, nl = read_profile(handle)
    lib.orbmi_set_profiling(handle, 0)
    # keypoints and FAST candidates of the last step (debug views)
    cnt = np.zeros(2, np.int32)
    for item in range(2):
        buf = np.zeros((1 << 16, 3), np.int32)
        for l in range(8):
            c = C.c_int()
            lib.orbmi_debug_fast_candidates(handle, item, l, _capi.ptr(buf), 1 << 16, C.byref(c))
            cand += c.value
    lvl = np.zeros((1 << 14, 3), np.int32)
    for item in range(2):
        for l in range(8):
            c = C.c_int()
            lib.orbmi_debug_octree_level(handle, item, l, _capi.ptr(lvl), 1 << 14, C.byref(c))
            kp += c.value
    stage_ms = {_capi.STAGES[s]: round(ms[s] / n, 5) for s in range(NS) if nl[s] and s < len(_capi.STAGES)}
    dom = int(np.argmax(ms))
    P = sum(w * h for w, h in zip(W, H))
    padded = [(w + 38) * (h + 38) for w, h in zip(W, H)]
    cand_img, kp_img = cand / 2, kp / 2
    alg = {
        # k_pyramid builds every level in one launch (stage pyr_level0): the image in, padded levels out
        "pyr_level0": 2 * (W[0] * H[0] + sum(padded)),
        "pyr_resize": 2 * sum(W[l - 1] * H[l - 1] + padded[l] for l in range(1, 8)) / 7,
        "fast": 2 * (P + 4 * cand_img),
        # k_octree also blurs every level (the blur tiles run as extra workgroups of the launch)
        "octree": 2 * (4 * cand_img + 8 * kp_img) + 2 * (2 * P),
        "describe": 2 * kp_img * (37 * 37 + 31 * 31 + 60),
        "blur": 2 * (2 * P),
        "stereo_rows": kp_img * 28 * 2,
        "stereo_match": kp_img * (28 + 32 + 8) + kp_img * 1452,
        "stereo_filter": kp_img * 16,
    }
    return {"stage_ms": stage_ms, "dominant_id": dom, "dominant": _capi.STAGES[dom], "alg": alg, "P": P,
            "kp_per_step": kp, "launch_counts": {_capi.STAGES[s]: int(nl[s]) / n for s in range(NS)
                                                 if nl[s] and s < len(_capi.STAGES)}}


def reset_profile(handle):
    read_profile(handle)


def read_profile(handle):
    from orb_slam2_with_comment_amd import _capi
    NS = _capi.NUM_STAGES
    ms = np.zeros(NS)
    nl = np.zeros(NS, np.int64)
    _capi.check("orbmi_read_profile", _capi.lib().orbmi_read_profile(handle, _capi.ptr(ms), _capi.ptr(nl)))
    return ms, nl


def roofline_entry(name, stage, ms_total, launches, traffic_path, config):
    avg_s = ms_total / max(int(launches), 1) / 1e3
    alg = float(stage["alg"].get(name, 0.0))
    achieved = alg / avg_s / 1e9 if avg_s > 0 else 0.0
    return {"kernel": name, "bound": "hbm", "achieved": round(achieved, 3), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 6), "traffic": read_traffic(traffic_path, name, config),
            "alg_bytes_per_launch": round(alg), "avg_launch_us": round(avg_s * 1e6, 3), "launches": int(launches)}


def read_pose_profile(lib, handle):
    ms, nl = C.c_double(), C.c_longlong()
    rc = lib.orbmi_pose_read_profile(handle, C.byref(ms), C.byref(nl))
    if rc:
        raise RuntimeError(f"orbmi_pose_read_profile returned {rc}")
    return ms.value, nl.value


# algorithmic fp64 flops of PoseOptimization: per edge and edge pass
# (computeActiveErrors + linearizeOplus + J^T W J + b) and per Levenberg trial (damped 6x6 LDL^T
# + exponential map + step control)
POSE_PROF_STRIDE = int(os.environ.get("ORBMI_POSE_PROF_STRIDE", "7"))  # (A/B: 1 = every launch)
POSE_FLOPS_PER_EDGE_PASS = 300
POSE_FLOPS_PER_TRIAL = 600


def pose_roofline(prof, recs, traffic_path, config):
    """k_pose_opt against the FP64 peak: edge passes counted as (iterations + 4 rounds) x edges
    of the frame's two PoseOptimizations (a lower bound: rejected trials add passes)."""
    ms_total, launches = prof
    avg_s = ms_total / max(int(launches), 1) / 1e3
    flops = np.mean([int(r["n_obs"]) * POSE_FLOPS_PER_EDGE_PASS * (int(r["iterations"]) + 4)
                     + int(r["iterations"]) * POSE_FLOPS_PER_TRIAL for r in recs])
    achieved = flops / avg_s / 1e12 if avg_s > 0 else 0.0
    # the kernel issues fp64 VALU instructions only (no MFMA: a 6x6 system per frame, DESIGN.md
    # §4 and the MFMA A/B in §4b); the peak is the fp64 vector peak, equal to the fp64 MFMA peak
    return {"kernel": "k_pose_opt", "bound": "fp64-valu", "achieved": round(achieved, 6), "peak": FP64_PEAK_TFS,
            "unit": "TFLOP/s", "frac": round(achieved / FP64_PEAK_TFS, 8),
            "traffic": read_traffic(traffic_path, "k_pose_opt", config), "alg_flops_per_launch": round(float(flops)),
            "avg_launch_us": round(avg_s * 1e6, 3), "launches": int(launches),
            "note": "fp64 Levenberg on one workgroup per frame: serial-latency-bound (DESIGN.md)"}


def pipeline_roofline(stage, rows, cols):
    kp_img = stage["kp_per_step"] / 2
    B = 7 * stage["P"] + 60 * kp_img  # B = 7P + 60N per image
    ext_ms = sum(v for k, v in stage["stage_ms"].items() if k in ("pyr_level0", "pyr_resize", "fast", "octree",
                                                                   "blur", "describe"))
    out = {"alg_bytes_per_image": round(B), "extract_ms_per_step": round(ext_ms, 5)}
    if ext_ms > 0:
        gbs = 2 * B / (ext_ms / 1e3) / 1e9
        out["achieved_GBs"] = round(gbs, 3)
        out["frac"] = round(gbs / HBM_PEAK_GBS, 6)
    return out


def max_over_ranks(dt, dist):
    if not dist:
        return dt
    t = torch.tensor([dt], dtype=torch.float64, device="cuda")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def host_info():
    return {"cpu": cpu_model(), "nproc": os.cpu_count(), "cpu_share_threads": cpu_threads(), "hip": torch.version.hip}


def cpu_baseline_track(S, problem, a):
    """The oracle (C++ restatement of the reference path) on host cores with the reference's
    threading: L/R extraction on two threads (src/Frame.cc:78-81), stereo + TrackWithMotionModel +
    TrackLocalMap serial, LocalBundleAdjustment on a third thread (LocalMapping) every 4th frame."""
    from concurrent.futures import ThreadPoolExecutor
    from orb_slam2_with_comment_amd.types import Frame, LFPOINT_DTYPE, MAPPOINT_DTYPE
    O = oracle_native()
    cam = S["cam"]
    p = O.params(a.nfeatures)
    inv_sigma2 = O.tables(p)["inv_sigma2"]
    pool = ThreadPoolExecutor(2)
    lm = ThreadPoolExecutor(1)
    F = a.frames
    lf_frames = {}
    for f in range(S["nF"]):
        L, R, T, kl, dl, u, d = S["feats"][f]
        lf_frames[f] = Frame(kl, dl, u, S["keep"][3][f], cam)
    lf_points = [S["lf_pts"][f][:S["n_lf"][f] * LFPOINT_DTYPE.itemsize].cpu().numpy().view(LFPOINT_DTYPE)
                 for f in range(S["nF"])]
    mps = [None if m is None else m.cpu().numpy().view(MAPPOINT_DTYPE) for m in S["mps"]]
    futs = []
    n = 0
    t0 = time.perf_counter()
    while True:
        f = 2 + n % F
        L, R, T, _, _, _, _ = S["feats"][f]
        fl = pool.submit(O.extract, p, L)
        fr = pool.submit(O.extract, p, R)
        (kl, dl), (kr, dr) = fl.result(), fr.result()
        u, d = O.stereo(p, L, R, cam.bf, cam.fx, kl, dl, kr, dr)
        cf = Frame(kl, dl, u, S["tcws"][f], cam)
        O.track_frame(cf, lf_frames[f - 1], lf_points[f - 1], mps[f], inv_sigma2, 7.0)
        if n % KF_EVERY == 0:  # LocalMapping::Run for the new keyframe (the GPU bench's chain)
            if a.lm_chain == "full":
                futs.append(lm.submit(cpu_local_mapping, O, S["vocab"], S["jobs"][f]))
            else:
                futs.append(lm.submit(lambda dl_=dl: (O.transform(S["vocab"], dl_, 4), O.local_ba(problem))))
        n += 1
        el = time.perf_counter() - t0
        if (el >= a.cpu_sample_s and n >= KF_EVERY) or n >= 10000:
            break
    for fu in futs:
        fu.result()
    el = time.perf_counter() - t0
    pool.shutdown()
    lm.shutdown()
    return {"value": round(n / el, 4), "unit": "frames/s", "cores": 3, "kind": "port",
            "sample": f"{n} tracked frames (same synthetic frames, local maps and BA graph), oracle (-O3 "
                      f"-march=native) extract L||R (2 threads) + stereo + TrackWithMotionModel + TrackLocalMap "
                      f"(both PoseOptimizations) serial, {len(futs)} LocalMapping keyframes "
                      f"({'full LocalMapping::Run chain' if a.lm_chain == 'full' else 'ComputeBoW + LocalBA'}) "
                      f"on a 3rd thread; {el:.1f} s",
            "cpu": O.cpu_model()}


# --------------------------------------------------------------------------------- extract
def run_extract(a, rank, world, local, dist):
    from orb_slam2_with_comment_amd import synth
    from orb_slam2_with_comment_amd.pipeline import StereoTracker
    cam = synth.KITTI
    rows, cols = cam.height, cam.width
    frames = [synth.stereo_pair(cam, f, seed_base=1000 * (rank + 1))[:2] for f in range(a.frames)]
    imgs = torch.from_numpy(np.stack([np.stack(p) for p in frames])).cuda()
    tr = StereoTracker(cam, a.nfeatures, device=local, pipelined=True)
    img_bytes = rows * cols

    def step(i):
        tr.extract_stereo(imgs.data_ptr() + (i % a.frames) * 2 * img_bytes, rows, cols)

    for i in range(a.warmup):
        step(i)
    tr.synchronize()
    from orb_slam2_with_comment_amd import _capi
    lib = _capi.lib()
    if a.full:
        stage = profile_stages(tr.extractor.handle, lambda i: (step(i), tr.synchronize()), max(a.frames, 16))
        lib.orbmi_set_profiling(tr.extractor.handle, 1 << stage["dominant_id"])
        reset_profile(tr.extractor.handle)
    tr.synchronize()
    if dist:
        dist.barrier()
    t0 = time.perf_counter()
    for i in range(a.steps):
        step(i)
    tr.synchronize()
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    dt = max_over_ranks(time.perf_counter() - t0, dist)
    if a.full:
        ms, nl = read_profile(tr.extractor.handle)
        lib.orbmi_set_profiling(tr.extractor.handle, 0)
    if a.dump_outputs and rank == 0:
        nl_, nr_ = (int(x) for x in tr.counts.cpu().numpy())
        kps, desc = tr.kps.cpu().numpy(), tr.desc.cpu().numpy()
        dump_outputs(a.dump_outputs, {
            "left_keypoints": keypoints_f32(kps[0, :nl_]), "right_keypoints": keypoints_f32(kps[1, :nr_]),
            "left_descriptors": desc[0, :nl_], "right_descriptors": desc[1, :nr_],
            "u_right": tr.u_right[0, :nl_].cpu().numpy(), "depth": tr.depth[0, :nl_].cpu().numpy()})
    value = a.steps * world / dt
    out = None
    if rank == 0:
        cpu = None if (not a.full or a.no_cpu_baseline or world > 1) else cpu_baseline_extract(frames, cam, a)
        out = {
            "metric": METRIC, "value": round(value, 3), "unit": "frames/s", "n_gpus": world, "steps": a.steps,
            "warmup": a.warmup, "ms_per_step": round(dt / a.steps * 1e3, 4), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "u8",
            "data": "synthetic: ray-cast KITTI-shaped 1241x376 stereo sequence, resident in HBM",
            "config": {"workload": "extraction only: ORBextractor(L,R) [2000 feat] + ComputeStereoMatches",
                       "frames_resident": a.frames, "parallelism": f"one stereo stream per GPU x{world}"},
            "full": a.full, "host": host_info(),
        }
        if a.full:
            out.update({
                "kpts_desc_per_s": round(value * stage["kp_per_step"], 1),
                "keypoints_per_frame": stage["kp_per_step"],
                "stage_ms_per_step": stage["stage_ms"],
                "roofline": roofline_entry(stage["dominant"], stage, ms[stage["dominant_id"]],
                                           nl[stage["dominant_id"]], a.traffic, traffic_config(a)),
                "pipeline_roofline": pipeline_roofline(stage, rows, cols),
                "cpu_baseline": cpu,
            })
    tr.close()
    return out


def cpu_baseline_extract(frames, cam, a):
    from concurrent.futures import ThreadPoolExecutor
    O = oracle_native()
    p = O.params(a.nfeatures)
    pool = ThreadPoolExecutor(2)
    n = 0
    t0 = time.perf_counter()
    while True:
        L, R = frames[n % len(frames)]
        fl, fr = pool.submit(O.extract, p, L), pool.submit(O.extract, p, R)
        (kl, dl), (kr, dr) = fl.result(), fr.result()
        O.stereo(p, L, R, cam.bf, cam.fx, kl, dl, kr, dr)
        n += 1
        el = time.perf_counter() - t0
        if (el >= a.cpu_sample_s and n >= 3) or n >= 10000:
            break
    pool.shutdown()
    return {"value": round(n / el, 4), "unit": "frames/s", "cores": 2, "kind": "port",
            "sample": f"{n} stereo frames, oracle (-O3 -march=native) extract L||R (2 threads) + stereo, {el:.1f} s",
            "cpu": O.cpu_model()}


# --------------------------------------------------------------------------------- lba
def run_lba(a, rank, world, local, dist):
    from orb_slam2_with_comment_amd import synth_map as SM
    from orb_slam2_with_comment_amd.optimizer import LocalBA
    problem, _ = SM.local_ba_problem(seed=42 + rank)
    ba = LocalBA(local)
    for _ in range(max(a.warmup // 10, 1)):
        res = ba.run(problem)
    steps = max(a.steps // 10, 3)
    if dist:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        res = ba.run(problem)
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    dt = max_over_ranks(time.perf_counter() - t0, dist)
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, {"local_ba_tcw": res["tcw"], "local_ba_points": res["pos"],
                                      "local_ba_erase": res["erase"], "local_ba_iterations": res["iterations"],
                                      "local_ba_chi2": np.array(res["chi2"], np.float64)})
    out = None
    if rank == 0:
        cpu = None
        if a.full and not a.no_cpu_baseline and world == 1:
            O = oracle_native()
            n, t0 = 0, time.perf_counter()
            while True:
                O.local_ba(problem)
                n += 1
                if time.perf_counter() - t0 > min(a.cpu_sample_s, 10) and n >= 3:
                    break
            el = time.perf_counter() - t0
            cpu = {"value": round(n / el, 4), "unit": "LocalBA/s", "cores": 1, "kind": "port",
                   "sample": f"{n} config-3 LocalBAs on the oracle (g2o restatement, 1 thread), {el:.1f} s"}
        it = res["iterations"]
        E, M, K = len(problem.edges), len(problem.pts), int((problem.kfs["fixed"] == 0).sum())
        # flops per LM iteration ~ E*600 + Schur + (6K)^3/3
        obs = np.bincount(problem.edges["point"], minlength=M)
        flops_it = E * 600 + 2 * np.sum(72 * obs + 108 * obs * (obs + 1) / 2) + (6 * K) ** 3 / 3
        per_call_s = dt / steps
        achieved = flops_it * (it[0] + it[1]) / per_call_s / 1e12
        out = {
            "metric": "LocalBundleAdjustment/s (config 3)", "value": round(steps * world / dt, 3), "unit": "LocalBA/s",
            "n_gpus": world, "steps": steps, "warmup": a.warmup, "ms_per_step": round(per_call_s * 1e3, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64",
            "data": "synthetic config-3 graph (seed 42): 20 free + 4 fixed KFs, 3000 points",
            "config": {"workload": "config3: Optimizer::LocalBundleAdjustment, 5+10 LM iterations, Huber",
                       "edges": E, "points": M, "free_keyframes": K},
            "iterations": list(it), "chi2": list(res["chi2"]),
            "roofline": {"kernel": "LocalBA kernel chain", "bound": "latency (3 dependent launches per LM trial: Schur, solve, update + device-side LM decision)",
                         "achieved": round(achieved, 6), "peak": FP64_PEAK_TFS, "unit": "TFLOP/s",
                         "frac": round(achieved / FP64_PEAK_TFS, 8), "traffic": lba_trial_traffic(a),
                         "traffic_scope": "HBM bytes of one LM trial's launches (k_ba_schur + k_ba_solve_mfma + "
                                          "k_ba_update_errors), " + os.path.relpath(a.traffic_lba, ROOT)},
            "cpu_baseline": cpu, "host": host_info(),
        }
    ba.close()
    return out


# --------------------------------------------------------------------------------- system
def run_system(a, rank, world, local, dist):
    """Config 1: System::TrackStereo over the first `steps` (200) frames of the
    rendered KITTI-shaped sequence, on the native host loop (orbmi_slam: map, Tracking and the
    synchronous LocalMapping in C++ around the MI355X operators).  Host images in, poses out,
    like Examples/Stereo/stereo_kitti.cc:81-122: every frame timed with steady_clock, median and
    mean after 10 warm-up frames (the pacing usleep excluded).  cpu_baseline = the same host logic
    on the oracle backend (CPU restatement), a bounded sample of the same frames."""
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from orb_slam2_with_comment_amd.native_slam import NativeStereoSLAM
    from orb_slam2_with_comment_amd.settings import load_settings, write_settings
    from orb_slam2_with_comment_amd.system import StereoSLAM, ate_rmse
    from orb_slam2_with_comment_amd.vocabulary import Vocabulary
    from slam_backends import render_sequence
    N, W = max(a.steps, 12), 10
    frames = render_sequence(N)
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "KITTI_synth.yaml")
    write_settings(path, __import__("orb_slam2_with_comment_amd.synth", fromlist=["KITTI"]).KITTI,
                   n_features=a.nfeatures)
    s = load_settings(path)
    voc = Vocabulary.synthetic(k=10, L=5, seed=3)

    def drive(slam, ahead=False):
        """stereo_kitti's loop; ahead: the next pair handed over with each frame (its Frame
        constructor runs on the GPU while the frame is tracked, orbmi_slam_track_stereo_ahead)."""
        times = []
        for f, (L, R, _) in enumerate(frames):
            t0 = time.perf_counter()
            if ahead:
                slam.TrackStereo(L, R, 0.1 * f, next_pair=frames[f + 1][:2] if f + 1 < len(frames) else None)
            else:
                slam.TrackStereo(L, R, 0.1 * f)
            times.append(time.perf_counter() - t0)
        return np.array(times)

    def run_native(async_lm):
        slam = NativeStereoSLAM(s, device=local, vocabulary=voc, async_local_mapping=async_lm)
        if dist:
            dist.barrier()
        times = drive(slam, ahead=True)
        t0 = time.perf_counter()
        slam.WaitLocalMapping()  # the mapping thread's queue drains inside the measurement
        wait_s = time.perf_counter() - t0
        torch.cuda.synchronize()
        gt = np.array([fr[2] for fr in frames])
        traj = np.array(slam.trajectory_twc())
        ate = ate_rmse(traj, gt)
        st = slam.stats
        ok = sum(1 for x in st if x.get("state") == 2)
        counts = slam.counts()
        counts["local_mapping_outcomes"] = slam.local_mapping_counts()
        ph = slam.phase_ms()
        counts["phase_ms_per_frame"] = {k: v for k, v in ph.items() if not k.startswith("lm_")}
        per_kf = len(st) / max(counts["keyframes"] - 1, 1)  # the first keyframe is not mapped
        counts["local_mapping_ms_per_keyframe"] = {k[3:]: round(v * per_kf, 4) for k, v in ph.items()
                                                   if k.startswith("lm_")}
        slam.Shutdown()
        return times, wait_s, ate, ok, counts, traj, np.array([x.get("state", -1) for x in st])

    # the product configuration: LocalMapping on its own thread, concurrent with Tracking as in
    # the reference (System::System starts it, src/System.cc:84-92); then (--full) the synchronous
    # form (deterministic, what the parity tests drive) for comparison
    times, wait_s, ate, ok, counts, traj, states = run_native(True)
    dt = max_over_ranks(float(times[W:].sum()) + wait_s, dist)
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, {"trajectory_twc": traj, "frame_state": states})
    if a.full:
        s_times, s_wait, s_ate, s_ok, s_counts, _, _ = run_native(False)
    out = None
    if rank == 0:
        cpu = py = None
        if a.full and not a.no_cpu_baseline and world == 1:
            from slam_backends import OracleBackend
            O = oracle_native()  # the -O3 -march=native build, loaded before the backend binds it
            ref = StereoSLAM(s, backend=OracleBackend(s, voc))
            n, t1, ct = 0, time.perf_counter(), []
            while n < N:
                L, R, _ = frames[n]
                t0 = time.perf_counter()
                ref.TrackStereo(L, R, 0.1 * n)
                ct.append(time.perf_counter() - t0)
                n += 1
                if time.perf_counter() - t1 > a.cpu_sample_s and n >= W + 3:
                    break
            el = float(np.sum(ct[W:]))
            cpu = {"value": round((n - W) / el, 4), "unit": "frames/s", "cores": 1, "kind": "port",
                   "median_ms": round(float(np.median(ct[W:])) * 1e3, 2),
                   "sample": f"frames {W}..{n - 1} of the same sequence through the same host logic (system.py) "
                             f"on the oracle backend (1 thread), {el:.1f} s", "cpu": O.cpu_model()}
            # the same loop in Python over the GPU operators (system.StereoSLAM): the host-code share
            pyslam = StereoSLAM(s, device=local, vocabulary=voc)
            pt = drive(pyslam)
            pyslam.Shutdown()
            py = {"frames_per_s": round((N - W) / float(pt[W:].sum()), 3),
                  "median_ms": round(float(np.median(pt[W:])) * 1e3, 3)}
        out = {
            "metric": "frames/sec (System::TrackStereo, native host loop + concurrent LocalMapping)",
            "value": round((N - W) * world / dt, 3), "unit": "frames/s", "n_gpus": world, "steps": N - W,
            "warmup": W, "ms_per_step": round(dt / (N - W) * 1e3, 4), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "u8",
            "data": "synthetic: ray-cast KITTI-shaped 1241x376 stereo sequence with exact ground truth",
            "config": {"workload": "config 1: System::TrackStereo over the first 200 frames (Frame ctor + Track "
                                   "(motion model / reference KF) + TrackLocalMap + keyframe insertion + "
                                   "LocalMapping::Run [ProcessNewKeyFrame, MapPointCulling, CreateNewMapPoints, "
                                   "SearchInNeighbors, LocalBA, KeyFrameCulling]), 2000 features", "frames": N,
                       "parallelism": "one stream per GPU"},
            "frame_ms": {"median": round(float(np.median(times[W:])) * 1e3, 3),
                         "mean": round(float(np.mean(times[W:])) * 1e3, 3),
                         "p90": round(float(np.percentile(times[W:], 90)) * 1e3, 3)},
            "ate_rmse_m": round(ate, 5),
            "ate_note": "frames handed over back to back (no stereo_kitti.cc:95-107 timestamp wait): the mapping "
                        "thread lags Tracking by a timing-dependent amount and this ATE varies run to run "
                        "(0.4-3 m on this sequence, tools/concur_probe.py); with frames 3 ms apart it is "
                        "0.25-0.29 m (tests/test_native_slam_gpu.py), the synchronous loop's below is exact",
            "frames_tracked": ok, "keyframes": counts["keyframes"],
            "local_ba_calls": counts["local_ba_calls"], "mappoints": counts["mappoints"],
            "ba_skipped": counts["local_mapping_outcomes"]["ba_skipped"],
            "ba_interrupted": counts["local_mapping_outcomes"]["ba_interrupted"],
            "local_mapping_outcomes": counts["local_mapping_outcomes"],
            "local_mapping": "own thread, concurrent with Tracking (the reference's threading)",
            "phase_ms_per_frame": counts["phase_ms_per_frame"],
            "local_mapping_ms_per_keyframe": counts["local_mapping_ms_per_keyframe"],
            "final_local_mapping_wait_ms": round(wait_s * 1e3, 3),
            "full": a.full, "host": host_info(),
        }
        if a.full:
            out.update({"synchronous_local_mapping": {
                "frames_per_s": round((N - W) / (float(s_times[W:].sum()) + s_wait), 3),
                "frame_ms": {"median": round(float(np.median(s_times[W:])) * 1e3, 3),
                             "mean": round(float(np.mean(s_times[W:])) * 1e3, 3),
                             "p90": round(float(np.percentile(s_times[W:], 90)) * 1e3, 3)},
                "ate_rmse_m": round(s_ate, 5), "frames_tracked": s_ok, "keyframes": s_counts["keyframes"],
                "local_ba_calls": s_counts["local_ba_calls"], "phase_ms_per_frame": s_counts["phase_ms_per_frame"],
                "local_mapping_outcomes": s_counts["local_mapping_outcomes"],
                "local_mapping_ms_per_keyframe": s_counts["local_mapping_ms_per_keyframe"]},
                "python_host_loop_on_gpu": py, "cpu_baseline": cpu})
    return out


# --------------------------------------------------------------------------------- batch
def run_batch(a, rank, world, local, dist):
    """Config 5: EuRoC-shaped 752x480 mono, 8 levels, 5000 features, `batch` frames per launch.
    Frames shard across ranks with no collective: rank r extracts frames
    [64r, 64r+63] of the sequence (seed 5000 + frame), all distinct."""
    from orb_slam2_with_comment_amd import _capi, synth
    from orb_slam2_with_comment_amd.orb import ORBextractor
    cam = synth.EUROC
    rows, cols = cam.height, cam.width
    nb = a.batch
    base = [synth.mono(cam, nb * rank + f, seed_base=5000) for f in range(nb)]
    imgs = torch.from_numpy(np.stack(base)).cuda()
    ex = ORBextractor(5000, 1.2, 8, 20, 7, device=local)
    cap = 5000 + 64
    kps = torch.zeros((nb, cap, 7), dtype=torch.int32, device="cuda")
    desc = torch.zeros((nb, cap, 32), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(nb, dtype=torch.int32, device="cuda")
    lib = _capi.lib()

    def step(i):
        _capi.check("extract", lib.orbmi_extract_batch_device(
            ex.handle, _vp(imgs.data_ptr()), nb, rows, cols, cols, rows * cols, _vp(kps.data_ptr()),
            _vp(desc.data_ptr()), _vp(cnt.data_ptr()), cap))

    def sync():
        lib.orbmi_extractor_synchronize(ex.handle)
        torch.cuda.synchronize()

    for i in range(max(a.warmup // 4, 2)):
        step(i)
    sync()
    stage_ms = None
    if a.full:
        # per-stage GPU time of one launch (library event brackets; untimed)
        lib.orbmi_set_profiling(ex.handle, 0x1FF)
        reset_profile(ex.handle)
        for i in range(4):
            step(i)
        sync()
        st_ms, st_n = read_profile(ex.handle)
        lib.orbmi_set_profiling(ex.handle, 0)
        stage_ms = {_capi.STAGES[s]: round(st_ms[s] / 4, 5) for s in range(_capi.NUM_STAGES)
                    if st_n[s] and s < len(_capi.STAGES)}
    steps = max(a.steps // 10, 5)
    if dist:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    for i in range(steps):
        step(i)
    sync()
    if dist:
        dist.barrier()
    dt = max_over_ranks(time.perf_counter() - t0, dist)
    kp = float(cnt.float().mean().item())
    W, H = level_geometry(rows, cols)
    P = sum(w * h for w, h in zip(W, H))
    B = (7 * P + 60 * kp) * nb
    if a.dump_outputs and rank == 0:  # every frame's count, the first 16 frames' keypoints and descriptors
        n = cnt.cpu().numpy()
        k, d = kps[:16].cpu().numpy(), desc[:16].cpu().numpy()
        live = np.arange(cap)[None, :] < n[:16, None]  # rows past a frame's count are not outputs
        dump_outputs(a.dump_outputs, {
            "counts": n, "keypoints": np.where(live[..., None], keypoints_f32(k).reshape(k.shape), np.float32(0)),
            "descriptors": np.where(live[..., None], d, np.uint8(0))})
    out = None
    if rank == 0:
        cpu = None
        cpu_tp = None
        if a.full and not a.no_cpu_baseline and world == 1:
            O = oracle_native()
            p = O.params(5000)
            n, t0 = 0, time.perf_counter()
            while True:
                O.extract(p, base[n % nb])
                n += 1
                if time.perf_counter() - t0 > min(a.cpu_sample_s, 10) and n >= 3:
                    break
            el = time.perf_counter() - t0
            cpu = {"value": round(n / el, 4), "unit": "frames/s", "cores": 1, "kind": "port",
                   "sample": f"{n} EuRoC-shaped frames on the oracle extractor (-O3 -march=native, 1 thread), "
                             f"{el:.1f} s", "cpu": O.cpu_model()}
            cpu_tp = cpu_throughput_extract(O, p, base, min(a.cpu_sample_s, 10))
        gbs = B / (dt / steps) / 1e9
        out = {
            "metric": "frames/s (config 5 batched mono extraction)", "value": round(steps * nb * world / dt, 3),
            "unit": "frames/s", "n_gpus": world, "steps": steps, "warmup": a.warmup,
            "ms_per_step": round(dt / steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "u8",
            "data": "synthetic EuRoC-shaped 752x480 mono frames (64 distinct per rank), resident in HBM",
            "config": {"workload": f"config5: ORBextractor 5000 feat, 8 levels, {nb} frames per launch",
                       "parallelism": f"frames sharded {nb} per GPU x{world}, no collective"},
            "kpts_desc_per_s": round(steps * nb * world * kp / dt, 1), "keypoints_per_frame": round(kp, 1),
            "stage_ms_per_launch": stage_ms,
            "roofline": {"kernel": "pipeline", "bound": "hbm", "achieved": round(gbs, 3), "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 6),
                         "traffic": batch_traffic(a.traffic_batch, traffic_config(a)),
                         "traffic_source": os.path.relpath(a.traffic_batch, ROOT),
                         "alg_bytes_per_launch": round(B)},
            "cpu_baseline": cpu, "cpu_baseline_throughput": cpu_tp, "host": host_info(),
        }
    ex.close()
    return out


def oracle_native():
    """The oracle built -O3 -march=native on this host (bench's cpu_baseline legs only)."""
    from oracle import oracle_ctypes as O
    if O._lib is None:
        O.use_native()
    return O


def cpu_threads():
    """Host threads for throughput baselines: the job's CPU share (OMP_NUM_THREADS, 16 on the
    GPU box) bounded by the affinity mask."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    return max(1, min(n, int(os.environ.get("OMP_NUM_THREADS", "16"))))


def cpu_throughput_extract(O, p, frames, sample_s):
    """Throughput mode: one oracle extractor per host thread, each on its own
    frames, for kpts+desc/s."""
    from concurrent.futures import ThreadPoolExecutor
    T = cpu_threads()
    stop = time.perf_counter() + sample_s

    def worker(t):
        n = kp = 0
        while True:
            k, _ = O.extract(p, frames[(t + n * T) % len(frames)])
            n += 1
            kp += len(k)
            if time.perf_counter() > stop:
                return n, kp
    t0 = time.perf_counter()
    with ThreadPoolExecutor(T) as pool:
        res = list(pool.map(worker, range(T)))
    el = time.perf_counter() - t0
    n = sum(r[0] for r in res)
    kp = sum(r[1] for r in res)
    return {"value": round(kp / el, 1), "unit": "kpts+desc/s", "frames_per_s": round(n / el, 3), "cores": T,
            "kind": "port", "sample": f"{n} frames on {T} oracle extractors (one per thread, -O3 -march=native), "
                                      f"{el:.1f} s", "cpu": O.cpu_model()}


def spawn_ranks(a):
    """`--gpus N` (N > 1) outside torchrun: run the same command as N ranks of one torchrun job
    (one process per GPU, RCCL over xGMI) as a CHILD process started before this process makes
    any GPU call, and return its exit code (rank 0 prints the JSON line)."""
    import socket
    import subprocess
    n_dev = torch.cuda.device_count()  # does not initialise the GPU
    if a.gpus > n_dev and a.dist_backend == "nccl":
        raise SystemExit(f"bench.py: --gpus {a.gpus} but only {n_dev} GPU(s) visible")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]
    return subprocess.call(cmd, env=env)


def main():
    a = parse()
    if a.print_traffic_config:
        print(json.dumps(traffic_config(a)))
        return
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(a))
    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    if world != a.gpus:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={world}; launch one rank per GPU")
    if a.dist_backend != "nccl":  # rehearsal: ranks may share a GPU
        local = local % torch.cuda.device_count()
    torch.cuda.set_device(local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        if a.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(a.dist_backend)
    run = {"track": run_track, "extract": run_extract, "lba": run_lba, "batch": run_batch,
           "system": run_system}[a.mode]
    out = run(a, rank, world, local, dist)
    if rank == 0 and out is not None:
        print(json.dumps(out), flush=True)
    if dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
