"""Keeps tests/golden/bench_oracle.json honest (CPU only): the registry of benchmarked workloads still generates the
inputs the fixture was made from, a sample of its values is recomputed live with the oracle, and the divergence
variants' data sit at their target P(different)."""
import json

import numpy as np
import pytest

import bench_workloads as bw
from conftest import rel_err

LIVE_TOL = 1e-13


@pytest.fixture(scope="module")
def fixture():
    with open(bw.ORACLE_JSON) as fh:
        return json.load(fh)["workloads"]


def _check_digests(rec, chunks, index):
    got = [bw.digest(c) for c in chunks]
    want = [rec["sha256"][i] for i in index]
    assert got == want, "inputs changed: rerun make_bench_oracle.py"


def test_fixture_matches_the_registry(fixture):
    assert list(fixture) == list(bw.WORKLOADS)
    for name, w in bw.WORKLOADS.items():
        rec = fixture[name]
        assert (rec["states"], rec["columns"], rec["chunks"], rec["batch"]) == (w.states, w.columns, len(w.seeds),
                                                                                w.batch), name
        assert len(rec["sha256"]) == len(w.seeds) and len(rec["zip"]["total"]) == w.batch, name
        assert sorted(int(b) for b in rec["zip"]["per_chunk"]) == [b for b in bw.FIXTURE_PROPOSALS if b < w.batch]
        for b, per in rec["zip"]["per_chunk"].items():     # totals are the left-to-right sums of the per-chunk values
            s = 0.0
            for v in per:
                s += v
            assert len(per) == len(w.seeds) and s == rec["zip"]["total"][int(b)], (name, b)
        assert np.all(np.isfinite(rec["zip"]["total"])) and len(set(rec["zip"]["total"])) == w.batch, name
        if w.theta is not None:
            assert rec["theta"] == list(w.theta)
    assert fixture["headline_b64"]["sha256"] == fixture["headline"]["sha256"]
    # proposal 0 is the fixture's theta rebuilt by the model layer: (pi, T, E) equal to ~1e-12, not bit for bit
    assert rel_err(fixture["headline_b64"]["zip"]["total"][0], fixture["headline"]["zip"]["total"][0]) < 1e-12


def test_headline_inputs_and_value_live(fixture, oracle, hmm_params):
    w, rec = bw.WORKLOADS["headline"], fixture["headline"]
    chunks = bw.generate(w)
    _check_digests(rec, chunks, [0])
    pi, T, E = hmm_params("iso20_t0")
    got = oracle.Zip(chunks[0], 3).forward(pi, T, E)
    assert rel_err(got, rec["zip"]["total"][0]) < LIVE_TOL, (got, rec["zip"]["total"][0])
    assert rel_err(rec["textbook"], rec["zip"]["total"][0]) < 1e-12
    for m in rec["mutants"]:
        assert bw.digest(bw.mutate(chunks[0], m["column"])) == m["sha256"]
        assert rel_err(m["zip"], rec["zip"]["total"][0]) > 100 * 1e-11, m


def test_config3_chunk_live(fixture, oracle, hmm_params):
    w, rec = bw.WORKLOADS["config3_slice"], fixture["config3_slice"]
    i = 17
    chunk = bw.generate(w, [i])[0]
    _check_digests(rec, [chunk], [i])
    pi, T, E = hmm_params("iso20_t0")
    got = oracle.Zip(chunk, 3).forward(pi, T, E)
    assert rel_err(got, rec["zip"]["per_chunk"]["0"][i]) < LIVE_TOL, (got, rec["zip"]["per_chunk"]["0"][i])


def test_150_state_population_chunk_and_proposal_live(fixture, oracle):
    w, rec = bw.WORKLOADS["pop150"], fixture["pop150"]
    i, b = 9, 31
    chunk = bw.generate(w, [i])[0]
    _check_digests(rec, [chunk], [i])
    pis, Ts, Es = bw.proposals(w)
    assert not np.array_equal(Ts[b], Ts[0])
    got = oracle.Zip(chunk, 3).forward(pis[b], Ts[b], Es[b])
    assert rel_err(got, rec["zip"]["per_chunk"][str(b)][i]) < LIVE_TOL, (got, rec["zip"]["per_chunk"][str(b)][i])


@pytest.mark.parametrize("name", sorted(bw.DIVERGENCE_TARGET))
def test_divergence_variants_hit_their_rate(fixture, name):
    w, target = bw.WORKLOADS[name], bw.DIVERGENCE_TARGET[name]
    p = bw.p_different(bw.first_piece(w))
    assert abs(p - target) < 0.05 * target, (name, p, target)
    assert abs(fixture[name]["p_different"] - target) < 0.05 * target, (name, fixture[name]["p_different"])
    base = bw.p_different(bw.first_piece(bw.WORKLOADS["headline" if w.states == 20 else "config2"]))
    assert p > 2 * base, (name, p, base)                  # the benchmark data themselves sit at about 0.4 %
