"""orbmi_local_mapping_job (one native call per LocalMapping::Run iteration, the default of
pipeline.LocalMapper.run_job) against the call-by-call chain over the per-operator entries
(ORBMI_LM_NATIVE=0) on the same jobs, two mappers: every output bit for bit -- SearchForTriangulation
matches, accepted pairs and their points, the distinctive descriptors, both Fuse directions, the
keyframe's FeatureVector and LocalBA's poses, positions, erase list, chi2 and iteration counts.
(tests/test_local_mapping_gpu.py checks the native default against the oracle.)"""
import argparse

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    import bench
    from orb_slam2_with_comment_amd import synth_map as SM
    from orb_slam2_with_comment_amd.vocabulary import ORBVocabulary, Vocabulary
    S = bench.setup_track(argparse.Namespace(frames=4, nfeatures=500), 0, 0)
    vocab = Vocabulary.synthetic(k=10, L=3)
    voc = ORBVocabulary(vocab, device=0)
    problem, _ = SM.local_ba_problem(seed=3, n_free=3, n_fixed=1, n_points=60)
    jobs, keep = bench.setup_local_mapping(S, voc, vocab, 0, problem)
    yield dict(S=S, voc=voc, problem=problem, jobs=jobs, keep=keep)
    voc.close()
    S["tr"].close()


def _mapper(monkeypatch, voc, native, prebow):
    from orb_slam2_with_comment_amd.pipeline import LocalMapper
    monkeypatch.setenv("ORBMI_LM_NATIVE", "1" if native else "0")
    m = LocalMapper(0, vocabulary=voc, prebow=prebow)
    assert m._native == native
    return m


def _outputs(mapper, job, out):
    """Everything a finished job left behind, read back to the host."""
    o = mapper._out
    mapper._ms.synchronize()
    npts = job.obs[2]
    ok = o["tri_ok"]()
    fv = o["fv"]()
    last = mapper.last
    return dict(tri=o["tri"](), tri_ok=ok, x3d=np.where(ok[..., None] > 0, o["x3d"](), np.float32(0)).view(np.uint32),
                best=o["best"][:npts].cpu().numpy(), dsc=o["dsc"][:32 * npts].cpu().numpy(),
                bi=o["bi"][:o["n_fuse"]].cpu().numpy(), bd=o["bd"][:o["n_fuse"]].cpu().numpy(),
                fv_node=fv.node_id, fv_off=fv.off, fv_feat=fv.feat, bow_words=np.int64(out["bow_words"]),
                tcw=last["tcw"].view(np.uint32), pos=last["pos"].view(np.uint32), erase=last["erase"],
                chi2=np.asarray(last["chi2"]).view(np.uint64), iterations=np.asarray(last["iterations"]),
                stop_check=np.int64(last["stop_check"]))


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def _hand_jobs(jobs):
    """Jobs bench.setup_local_mapping cannot produce: a keyframe without neighbours and target
    points, and a keyframe without map points (no candidates for the targets, nothing for
    ComputeDistinctiveDescriptors)."""
    from orb_slam2_with_comment_amd.pipeline import LocalMappingJob
    j = jobs[sorted(jobs)[0]]
    alone = LocalMappingJob(j.kf, j.d_desc, [], j.kf_points, (None, 0), j.obs, j.problem)
    empty = LocalMappingJob(j.kf, j.d_desc, j.neighbours, (j.kf_points[0], 0), j.target_points,
                            (j.obs[0], j.obs[1], 0), j.problem)
    return {"no_neighbours": alone, "no_map_points": empty}


@pytest.mark.parametrize("prebow", [True, False])
def test_native_job_equals_call_by_call(setup, monkeypatch, prebow):
    jobs = dict(setup["jobs"])
    order = sorted(jobs)[:2]
    jobs.update(_hand_jobs(jobs))
    order += ["no_neighbours", "no_map_points"]
    got = {}
    for native in (True, False):  # one mapper after the other: without prebow they share the vocabulary's stream
        mapper = _mapper(monkeypatch, setup["voc"], native, prebow)
        try:
            got[native] = {f: _outputs(mapper, jobs[f], mapper.run_job(jobs[f])) for f in order}
        finally:
            mapper.close()
    for f in order:
        _same(got[True][f], got[False][f], f"job {f}")
    ref = got[False]
    assert (ref[order[0]]["tri"] >= 0).any() and ref[order[0]]["tri_ok"].any() and (ref[order[0]]["bi"] >= 0).any()
    assert ref["no_neighbours"]["tri"].size == 0 and ref["no_neighbours"]["bi"].size == 0
    assert ref["no_map_points"]["best"].size == 0 and (ref["no_map_points"]["tri"] >= 0).any()


def test_three_queued_jobs_alternate_bow_sets(setup, monkeypatch):
    """Three jobs through insert_keyframe / wait(): the next keyframe's ComputeBoW is issued from
    inside the native call (LocalBA's enqueued hook) into the other BowVector / FeatureVector set."""
    jobs = setup["jobs"]
    a, b = sorted(jobs)[:2]
    got = {}
    for native in (True, False):
        mapper = _mapper(monkeypatch, setup["voc"], native, True)
        try:
            for f in (a, b, a):
                mapper.insert_keyframe(jobs[f])
            mapper.wait()
            assert mapper.done == 3 and mapper.bow_ahead >= 1
            got[native] = _outputs(mapper, jobs[a], mapper.last_chain)
            for slot, bw in enumerate(mapper.bows):
                got[native].update({f"set{slot}_{k}": v.cpu().numpy() for k, v in bw.items() if k == "counts"})
                nn = int(bw["counts"][1].item())
                got[native][f"set{slot}_node"] = bw["node"][:nn].cpu().numpy()
                got[native][f"set{slot}_off"] = bw["off"][:nn + 1].cpu().numpy()
        finally:
            mapper.close()
    _same(got[True], got[False], "third queued job")


def test_null_job_is_an_argument_error(setup, monkeypatch):
    import ctypes as C
    from orb_slam2_with_comment_amd._capi import ORBMI_E_ARG, lib
    from orb_slam2_with_comment_amd.types import LMJobResult
    mapper = _mapper(monkeypatch, setup["voc"], True, True)
    try:
        res = LMJobResult()
        assert lib().orbmi_local_mapping_job(mapper.matcher._h, mapper.ba._h, None, C.addressof(res)) == ORBMI_E_ARG
        assert lib().orbmi_local_mapping_job(mapper.matcher._h, mapper.ba._h, None, None) == ORBMI_E_ARG
    finally:
        mapper.close()
