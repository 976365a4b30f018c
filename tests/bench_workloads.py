"""Registry of the workloads bench.py times, for the tests that pin them to the CPU oracle (not a test module).

One entry per workload: where its (pi, T, E) come from (a fixture key of tests/golden/hmm_params.npz, or a model and
theta), the number of states, the columns per chunk, the chunk seeds, the number of parameter sets per evaluation and
the bench.py flags that select it (None: only measured under --full, in bench.extra_configs).  The data and the
proposals are produced by bench.py's own functions (bench.generate, bench.proposals), so a change to the bench's
rules shows up as a changed input digest, never as a silent divergence of the tests from the timed run.

The two "divergence" families are not benchmarked: they are the headline's and config[2]'s shapes on data sampled at
the P(different) of the reference's example pairs (1 % and 3.3 %; the benchmark data sit at about 0.4 %), where the
pair dictionary, the columns per token and the rank-1 hand-off point all differ.

tests/golden/make_bench_oracle.py writes the oracle values of every entry to tests/golden/bench_oracle.json.
"""
import collections
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import bench  # noqa: E402

# Serial generation: a fork pool is unsafe in a process that has touched the GPU (bench.generate's docstring), and
# pytest runs these after other GPU tests.  Every piece has its own seed, so the data do not depend on this.
bench.GEN_WORKERS = 1

ORACLE_JSON = os.path.join(REPO, "tests", "golden", "bench_oracle.json")
BATCH = 64
FIXTURE_PROPOSALS = (0, 1, 31, 32, 63)      # proposals whose per-chunk values the fixture records

Workload = collections.namedtuple("Workload", "name key model theta states columns seeds batch flags")


def _model(kind, states):
    from imcoalhmm_amd import models
    if kind == "iso":
        return models.IsolationModel(states)
    return models.IsolationMigrationModel(states // 2, states - states // 2)


WORKLOADS = collections.OrderedDict((w.name, w) for w in (
    # bench.main: --gpus 1 -> config2 on iso20_t0, one 1e8-column chain, seed 20240001
    Workload("headline", "iso20_t0", "iso", None, 20, 100_000_000, (20240001,), 1, ()),
    # bench.main with --batch 64: the same chain, bench.proposals' 64 parameter sets
    Workload("headline_b64", "iso20_t0", "iso", None, 20, 100_000_000, (20240001,), BATCH, ("--batch", "64")),
    # BASELINE config[2]: bench.main --fixture im150_t0 (seed 20240001 + 1) and extra_configs "c3"
    Workload("config2", "im150_t0", "im", None, 150, 100_000_000, (20240002,), 1, ("--fixture", "im150_t0")),
    # per-GPU slice of BASELINE config[3]: bench.main --workload config4-slice and extra_configs "c4_*"
    Workload("config3_slice", "iso20_t0", "iso", None, 20, 10_000_000, tuple(20240100 + i for i in range(32)), 1,
             ("--workload", "config4-slice")),
    # populations of extra_configs: "c5_*", "c5n20_*", "a10_*"
    Workload("pop150", "im150_t0", "im", None, 150, 1_000_000, tuple(20240600 + i for i in range(32)), BATCH, None),
    Workload("pop20", "iso20_t0", "iso", None, 20, 1_000_000, tuple(20240700 + i for i in range(32)), BATCH, None),
    Workload("pop10", "iso10_t0", "iso", None, 10, 1_000_000, tuple(20240800 + i for i in range(100)), BATCH, None),
    # per-GPU slice of BASELINE config[4] through bench.main
    Workload("pop150_slice", "im150_t0", "im", None, 150, 1_000_000, tuple(20240100 + i for i in range(32)), BATCH,
             ("--fixture", "im150_t0", "--workload", "config4-slice", "--columns", "1000000", "--batch", "64")),
    # divergence variants (theta = split time, coal rate, recomb rate / isolation time, migration time, coal rate,
    # recomb rate, migration rate): P(different) about 1.0 %, 3.3 % and 3.3 %
    Workload("div20_1pc", None, "iso", (0.004, 1000.0, 0.4), 20, 100_000_000, (20240901,), 1, None),
    Workload("div20_3pc", None, "iso", (0.0157, 1000.0, 0.4), 20, 100_000_000, (20240902,), 1, None),
    Workload("div150_3pc", None, "im", (0.0125, 0.0125, 1000.0, 0.4, 200.0), 150, 10_000_000, (20240903,), 1, None),
))

DIVERGENCE_TARGET = {"div20_1pc": 0.010, "div20_3pc": 0.033, "div150_3pc": 0.033}


def _params_file():
    return np.load(os.path.join(REPO, "tests", "golden", "hmm_params.npz"))


def hmm(w):
    """(pi, T, E) of the workload's unperturbed parameter set."""
    if w.key is not None:
        d = _params_file()
        return d[w.key + "_pi"], d[w.key + "_T"], d[w.key + "_E"]
    return _model(w.model, w.states).build_hidden_markov_model(np.array(w.theta, dtype=np.float64))


def proposals(w):
    """(pis, Ts, Es) of the batch, exactly as bench.py builds them (row 0 is the unperturbed set)."""
    pi, T, E = hmm(w)
    if w.batch == 1:
        return pi[None], T[None], E[None]
    pis, Ts, Es, _ = bench.proposals(_params_file(), w.key, w.states, w.batch, T)
    return pis, Ts, Es


def generate(w, chunks=None):
    """The workload's chunks (uint8 arrays) in chunk order; `chunks`: indices of a subset."""
    idx = range(len(w.seeds)) if chunks is None else chunks
    if w.key is not None:
        data = bench.generate([(i, w.key, w.columns, w.seeds[i]) for i in idx])
        return [data[i] for i in idx]
    # bench.generate's rule (pieces of bench.PIECE columns, piece k seeded seed * 1000 + k) with the model's (pi, T, E)
    from imcoalhmm_amd import synth
    pi, T, E = hmm(w)
    out = []
    for i in idx:
        pieces = [synth.sample_alignment(pi, T, E, min(bench.PIECE, w.columns - off), seed=w.seeds[i] * 1000 + k)
                  for k, off in enumerate(range(0, w.columns, bench.PIECE))]
        out.append(pieces[0] if len(pieces) == 1 else np.concatenate(pieces))
    return out


def first_piece(w):
    """The first bench.PIECE columns of chunk 0 (for a cheap check of a divergence variant's rate)."""
    if w.key is not None:
        return bench.generate([(0, w.key, min(bench.PIECE, w.columns), w.seeds[0])])[0]
    from imcoalhmm_amd import synth
    pi, T, E = hmm(w)
    return synth.sample_alignment(pi, T, E, min(bench.PIECE, w.columns), seed=w.seeds[0] * 1000)


def digest(chunk):
    return hashlib.sha256(np.ascontiguousarray(chunk, dtype=np.uint8).tobytes()).hexdigest()


def p_different(chunk):
    """Fraction of differing columns among the columns with both bases present (symbol 1 over symbols 0 and 1)."""
    c = np.bincount(chunk, minlength=3)
    return float(c[1]) / float(c[0] + c[1])


def mutant_columns(columns):
    return (0, columns // 2, columns - 1)


def mutate(chunk, column):
    """Copy of `chunk` with the symbol s at `column` replaced by (s + 1) % 3."""
    m = chunk.copy()
    m[column] = (int(m[column]) + 1) % 3
    return m
