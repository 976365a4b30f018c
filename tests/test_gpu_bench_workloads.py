"""Every workload bench.py times, at full length, against the CPU oracle (tests/golden/bench_oracle.json).

The inputs are regenerated through bench.py's own functions (tests/bench_workloads.py) and checked against the
fixture's digests before anything is compared; the Forwarders are built as the bench builds them (a fresh pair
dictionary per workload, recompressed over all of its chunks).  One workload's Forwarders are alive at a time.
Beyond the bench's own numbers: all 64 proposals of the populations (the bench records only proposal 0), the rank-1
hand-off off as well as on, one-column mutants of the headline, and the headline / config[2] shapes on data at the
P(different) of the reference's example pairs (1 % and 3.3 %).
"""
import json
import math

import numpy as np
import pytest

import bench_workloads as bw
from conftest import rel_err
from imcoalhmm_amd import Forwarder, _capi
from imcoalhmm_amd.hmm import forward_chunks, forward_chunks_batch, recompress

pytestmark = pytest.mark.gpu
TOL = 1e-11

with open(bw.ORACLE_JSON) as _fh:
    ORACLE = json.load(_fh)["workloads"]


def _build(chunks):
    _capi.check(_capi.lib().imc_dictionary_reset())   # as bench.py: every workload compresses with its own dictionary
    fw = [Forwarder.from_array(c, 3) for c in chunks]
    recompress(fw)                                      # what bench.py / DistributedLikelihood do (no-op for one chunk)
    return fw


@pytest.fixture(scope="module")
def workload():
    """workload(name) -> (Workload, chunks, Forwarders); building one frees the previous workload's Forwarders."""
    cur = {}

    def release():
        for f in cur.get("fw", ()):
            f.close()
        cur.clear()

    def get(name):
        if cur.get("name") != name:
            release()
            w = bw.WORKLOADS[name]
            chunks = bw.generate(w)
            assert [bw.digest(c) for c in chunks] == ORACLE[name]["sha256"], "inputs changed: rerun make_bench_oracle.py"
            cur.update(name=name, w=w, chunks=chunks, fw=_build(chunks))
        return cur["w"], cur["chunks"], cur["fw"]

    yield get
    release()


def _report(name, errs):
    print("\n[bench oracle] %-13s worst rel err %.2e over %d values" % (name, max(errs), len(errs)))


def _single(workload, name, reference=("zip",)):
    w, _, fw = workload(name)
    rec = ORACLE[name]
    pi, T, E = bw.hmm(w)
    got = fw[0].forward(pi, T, E)
    wants = [rec["zip"]["total"][0]] + ([rec["textbook"]] if "textbook" in reference else [])
    errs = [rel_err(got, want) for want in wants]
    assert math.isfinite(got) and max(errs) < TOL, (name, got, wants)
    return got, errs


def test_headline_against_oracle_and_one_column_mutants(workload):
    """BASELINE config[1] (iso20_t0, 1 x 1e8, bench seed 20240001) through the bench's kernel, against the compressed
    and the textbook oracle; then each one-column mutant against its own oracle value - a dropped, doubled or misread
    column moves the value by far more than the tolerance."""
    got, errs = _single(workload, "headline", ("zip", "textbook"))
    kernels = _capi.last_plan()["kernels"]
    assert "k_zpropagate4<5" in kernels, kernels
    _report("headline", errs)
    w, chunks, _ = workload("headline")
    pi, T, E = bw.hmm(w)
    for m in ORACLE["headline"]["mutants"]:
        mutant = bw.mutate(chunks[0], m["column"])
        assert bw.digest(mutant) == m["sha256"], "inputs changed: rerun make_bench_oracle.py"
        _capi.check(_capi.lib().imc_dictionary_reset())
        f = Forwarder.from_array(mutant, 3)
        try:
            v = f.forward(pi, T, E)
        finally:
            f.close()
        shift = rel_err(v, got)
        print("[bench oracle] headline mutant at column %d: shift %.2e = %.0f x TOL, rel err %.2e" % (
            m["column"], shift, shift / TOL, rel_err(v, m["zip"])))
        assert rel_err(v, m["zip"]) < TOL, (m["column"], v, m["zip"])
        assert shift > 100 * TOL, (m["column"], v, got)


def _handoff_on_off(workload, name, must_fire, forced_segment=0):
    """The value with the rank-1 hand-off allowed (the default) and switched off, both against the oracle; with
    `forced_segment` also with the segment length forced, where the planner always schedules the hand-off test (one
    checkpoint at a quarter of the segment) - so the hand-off runs on these data even where the planner's estimate
    would not choose it at the natural segmentation."""
    w, _, fw = workload(name)
    want = ORACLE[name]["zip"]["total"][0]
    pi, T, E = bw.hmm(w)
    L = _capi.lib()
    runs = []
    try:
        for handoff, seg in ((1, 0), (0, 0)) + (((1, forced_segment),) if forced_segment else ()):
            _capi.check(L.imc_set_rank1_handoff(handoff))
            _capi.check(L.imc_set_segment_length(seg))
            v = fw[0].forward(pi, T, E)
            runs.append({"handoff": handoff, "segment": seg, "value": v, "kernels": _capi.last_plan()["kernels"],
                         "rank1 tested/collapsed": _capi.last_rank1()})
    finally:
        L.imc_set_segment_length(0)
        _capi.check(L.imc_set_rank1_handoff(1))
    msg = (name, want, runs)
    if must_fire:
        assert "rank1-handoff" in runs[0]["kernels"] and runs[0]["rank1 tested/collapsed"][1] > 0, msg
    assert "rank1" not in runs[1]["kernels"], msg
    if forced_segment:
        assert "rank1-handoff" in runs[2]["kernels"] and runs[2]["rank1 tested/collapsed"][0] > 0, msg
    errs = [rel_err(r["value"], want) for r in runs]
    assert all(math.isfinite(r["value"]) for r in runs) and max(errs) < TOL, msg
    _report(name, errs)
    for r in runs:
        print("[bench oracle] %s hand-off %d, segment %d: %s, rank-1 segments tested/collapsed %r" % (
            name, r["handoff"], r["segment"], r["kernels"], r["rank1 tested/collapsed"]))


def test_config2_handoff_on_and_off(workload):
    """BASELINE config[2] (im150_t0, 1 x 1e8, seed 20240002): the value with the certified rank-1 hand-off (default;
    it must have fired) and without it both match the oracle."""
    _handoff_on_off(workload, "config2", must_fire=True)


def test_config3_slice_per_chunk_and_total(workload):
    """Per-GPU slice of BASELINE config[3] (iso20_t0, 32 x 1e7, seeds 20240100 + i): every chunk, the total as the
    left-to-right sum of the chunks, and the total against the oracle's."""
    w, _, fw = workload("config3_slice")
    rec = ORACLE["config3_slice"]
    pi, T, E = bw.hmm(w)
    h = [f.handle for f in fw]
    per = forward_chunks_batch(h, pi[None], T[None], E[None], per_chunk=True)[0]
    tot = forward_chunks(h, pi, T, E)
    errs = [rel_err(g, o) for g, o in zip(per, rec["zip"]["per_chunk"]["0"])]
    bad = [(i, per[i], rec["zip"]["per_chunk"]["0"][i]) for i, e in enumerate(errs) if not e < TOL]
    assert not bad, bad
    s = 0.0
    for v in per:
        s += v
    assert tot == s, (tot, s)
    errs.append(rel_err(tot, rec["zip"]["total"][0]))
    assert errs[-1] < TOL, (tot, rec["zip"]["total"][0])
    _report("config3_slice", errs)


@pytest.mark.parametrize("name", ["pop150", "pop20", "pop10"])
def test_population_all_proposals_and_permuted_order(workload, name):
    """The populations of bench.py's extra_configs (64 proposals x 32 x 1e6 at 150 and 20 states, 64 x 100 x 1e6 at
    10 states): the totals of all 64 proposals and the per-chunk values of five of them against the oracle; the same
    64 proposals in another order give every proposal the same bits (consecutive evaluations with different
    parameters share nothing)."""
    w, _, fw = workload(name)
    rec = ORACLE[name]
    pis, Ts, Es = bw.proposals(w)
    h = [f.handle for f in fw]
    per = forward_chunks_batch(h, pis, Ts, Es, per_chunk=True)
    tot = forward_chunks_batch(h, pis, Ts, Es)
    errs = []
    for b in range(w.batch):
        e = rel_err(tot[b], rec["zip"]["total"][b])
        assert e < TOL, (name, b, tot[b], rec["zip"]["total"][b])
        errs.append(e)
    for b, want in rec["zip"]["per_chunk"].items():
        b = int(b)
        for i, (g, o) in enumerate(zip(per[b], want)):
            e = rel_err(g, o)
            assert e < TOL, (name, b, i, g, o)
            errs.append(e)
    perm = np.random.default_rng(20241016).permutation(w.batch)
    per_p = forward_chunks_batch(h, pis[perm], Ts[perm], Es[perm], per_chunk=True)
    tot_p = forward_chunks_batch(h, pis[perm], Ts[perm], Es[perm])
    for k, b in enumerate(perm):
        assert per_p[k].tobytes() == per[b].tobytes(), (name, b, k)
        assert tot_p[k] == tot[b], (name, b, k, tot_p[k], tot[b])
    _report(name, errs)


@pytest.mark.parametrize("name", ["div20_1pc", "div20_3pc"])
def test_headline_shape_at_higher_divergence(workload, name):
    """20 states, 1 x 1e8 columns at P(different) ~ 1 % and ~ 3.3 %: a different pair dictionary and columns per
    token than the benchmark data's 0.4 %."""
    _, errs = _single(workload, name, ("zip", "textbook"))
    _report(name, errs)


def test_150_states_at_higher_divergence_handoff_on_and_off(workload):
    """150 states, 1 x 1e7 columns at P(different) ~ 3.3 %: the rank-1 hand-off point moves with the data.  At this
    length the planner may keep the plain GEMM chain, so the hand-off is also run at a forced segmentation."""
    _handoff_on_off(workload, "div150_3pc", must_fire=False, forced_segment=50_000)
