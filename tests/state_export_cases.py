"""Shared by tests/test_state_export_cpu.py and tests/test_gpu_state_export.py: the cases of the state-level check of
imc_forward_state (forward vectors and transfer operators compared ENTRY BY ENTRY with the long-double reference of
oracle/forward_oracle.c), the one comparer, and the measured fp64 deviations the shape tolerances come from.

A state is compared in two parts that cannot compensate each other:
  shape  every column normalised to sum 1 (in long double), max over entries of |got / ref - 1|: the column exponents
         drop out, so this sees mantissas only - a permuted row, a wrong lane, one entry off in the ninth digit;
  scale  log(sum_i values[i][c]) + exps[c] ln 2 against the reference's log mass of the column, relative to |log mass|
         (absolute below 1): each column mass is a log-likelihood from a basis start, held to the suite's 1e-11.

Shape tolerance of a family = 16 x the largest d64 over the family's cases, d64 = the worst shape deviation of the
oracle's fp64 variant (the same statements in double) from its long-double variant: measured on the CPU, never on the
device.  `python tests/state_export_cases.py` prints the table that D64 below records.

D64 is a record, not a measurement of every run.  The suite re-measures it only for the cases up to 24 states
(tests/test_state_export_cpu.py, within a factor of two either way): blocked-valu, blocked-mfma-lds and blocked-global
in full, percolumn up to 17 states, alphabet65 at 10 states.  chain-lds, wide-blocked, gemm-chain, gemm-chain-150,
gemm-chain-handoff, percolumn at 33 and 64 states and alphabet65 at 40 states are NOT re-checked by the suite (their
references cost seconds each); they are re-measured only by running this file by hand."""
import collections
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:            # (run as a script: pytest gets the path from conftest.py)
    sys.path.insert(0, REPO)
from imcoalhmm_amd import synth    # noqa: E402

R1_TOL = 2.0 ** -42          # kernels_big.hpp: the rank-one hand-off's component-wise claim, per certified segment
SCALE_TOL = 1e-11            # the suite's tolerance on a log-likelihood
SHAPE_FACTOR = 16.0          # device association (tokens, 16-step blocks, tree folds) against one sequential chain
STAYS = (0.9, 0.93, 0.97)    # random_hmm's stay probability of parameter set b
RAW_LENGTHS = (1, 2, 15, 16, 17, 464, 647)     # 464 = 29 units of 16: a last level-1 run of length 1; 647: ragged, two chain levels
TOKEN_LENGTHS = (4096, 4099, 6000)             # zip_min_columns is 4096
TRAINER_LENGTH = 40_000                        # created first: trains the dictionary the token chunks share; not exported
GLOBAL_TRAINER_LENGTH = 800_000                # ... of the global-table scan's cases: a dictionary with levels beyond LDS
HANDOFF_LENGTH = 3 * 4096 + 133                # three forced 4096-column segments and a ragged tail
_LN2 = np.log(np.longdouble(2.0))

# family -> worst d64 over its cases (measured here: python tests/state_export_cases.py); tolerance = SHAPE_FACTOR x
D64 = {
    "percolumn": 4.61e-15,             # tolerance 7.38e-14
    "chain-lds": 4.45e-15,             # tolerance 7.12e-14
    "blocked-valu": 2.9e-15,           # tolerance 4.64e-14
    "blocked-mfma-lds": 2.66e-15,      # tolerance 4.26e-14
    "blocked-global": 1.92e-15,        # tolerance 3.07e-14
    "wide-blocked": 1.93e-15,          # tolerance 3.09e-14
    "gemm-chain": 4.65e-15,            # tolerance 7.44e-14
    "gemm-chain-150": 2.06e-14,        # tolerance 3.3e-13   (150 states: kept apart, so that it does not widen 25-70)
    "gemm-chain-handoff": 1.15e-15,    # tolerance 1.84e-14  (+ R1_TOL per operator segment)
    "alphabet65": 1.77e-15,            # tolerance 2.83e-14
}

Case = collections.namedtuple("Case", "family n nsym tokens lengths segs zip blocked streaming wide expect reject trainer level")


def _case(family, n, tokens, zip_mode, expect, nsym=3, lengths=None, segs=None, blocked=4, streaming=-1, wide=-1, reject=(),
          trainer=TRAINER_LENGTH, level=None):
    if lengths is None:
        lengths = TOKEN_LENGTHS if tokens else RAW_LENGTHS
    if segs is None:
        segs = (0, 48, 52) if tokens else (0, 16)
    return Case(family, n, nsym, tokens, tuple(lengths), tuple(segs), zip_mode, blocked, streaming, wide,
                tuple(expect) + (("[tokens]",) if tokens else ("[columns]",)), tuple(reject), trainer if tokens else 0, level)


def cases():
    """Every row of the table in tests/test_gpu_state_export.py.  zip / blocked / streaming / wide are the arguments of
    imc_set_compression, imc_set_blocked_kernel, imc_set_table_streaming and imc_set_wide_blocked that pin the family, as
    the other GPU modules pin it; expect: substrings of imc_last_kernels() that say the family ran."""
    out = []
    for n in (1, 3, 4, 16, 17, 33, 64):
        out.append(_case("percolumn", n, False, 4, ("k_propagate<",)))
    out.append(_case("chain-lds", 72, False, 0, ("k_big_propagate",)))
    for n in (10, 20):
        out.append(_case("blocked-valu", n, True, 3, ("k_zpropagate2<",), blocked=2))
        out.append(_case("blocked-valu", n, False, 5, ("k_zpropagate2<",), blocked=2))
    for n in (4, 13, 20, 24):
        out.append(_case("blocked-mfma-lds", n, True, 3, ("k_zpropagate3<",), blocked=3))
    for n in (10, 16, 20):
        for streaming in (0, 1):
            # a level beyond LDS needs a larger dictionary than 40 000 columns train (36 tokens: every level fits LDS, the
            # planner runs k_zpropagate3): 800 000 columns train 2727 tokens.  Once automatic (a byte level), once pinned
            # to the 384-token level (IMC_FORCE_LEVEL=11: 16-bit tokens).
            how = dict(blocked=5, streaming=streaming, trainer=GLOBAL_TRAINER_LENGTH, reject=() if streaming else ("streamed",))
            streamed = ("streamed",) if streaming else ()
            out.append(_case("blocked-global", n, True, 3, ("k_zpropagate4<",) + streamed, **how))
            out.append(_case("blocked-global", n, True, 3, ("k_zpropagate4<", ",16") + streamed, level=11, **how))
    for n in (25, 28, 32):
        out.append(_case("wide-blocked", n, True, 1, ("k_zpropagate4<%d" % ((n + 3) // 4),), wide=1))
    for n in (25, 33, 48, 64, 70):
        out.append(_case("gemm-chain", n, True, 3, ("k_big_propagate",)))
        out.append(_case("gemm-chain", n, False, 5, ("k_big_propagate",)))
    out.append(_case("gemm-chain-150", 150, False, 5, ("k_big_propagate",), lengths=(1, 16, 17, 464, 647)))
    for n in (28, 70):
        out.append(_case("gemm-chain-handoff", n, False, 5, ("k_big_propagate", "rank1-handoff"), lengths=(HANDOFF_LENGTH,), segs=(4096,)))
    # (the blocked MFMA scan with its table in LDS, not the per-vector token kernel k_zpropagate<R,G> the planner falls back to)
    out.append(_case("alphabet65", 10, True, 3, ("k_zpropagate3<",), nsym=65, reject=("k_zpropagate<",)))
    out.append(_case("alphabet65", 40, True, 3, ("k_big_propagate",), nsym=65))
    return out


def case_id(case):
    return "%s-n%d-%s%s%s" % (case.family, case.n, "tokens" if case.tokens else "raw",
                              "-stream%d" % case.streaming if case.streaming >= 0 else "",
                              "-level%d" % case.level if case.level is not None else "")


def families():
    return sorted({c.family for c in cases()})


def hmms_of(case):
    """The three parameter sets of a case (B = 1 takes the first)."""
    return [synth.random_hmm(case.n, case.nsym, seed=8300 + 3 * case.n + b, stay=STAYS[b]) for b in range(3)]


def compressible(n, seed, nsym=3):
    rng = np.random.default_rng(seed)
    p = np.full(nsym, 0.1 / max(nsym - 1, 1)); p[0] = 0.9
    return rng.choice(nsym, size=n, p=p / p.sum()).astype(np.uint8)


def skewed_symbols(n, nsym, seed):
    """A compressible stream over a large alphabet: three frequent symbols (one of them the last), the rest rare."""
    rng = np.random.default_rng(seed)
    hot = np.array([0, nsym // 2, nsym - 1])
    obs = np.where(rng.random(n) < 0.9, hot[rng.integers(0, 3, size=n)], rng.integers(0, nsym, size=n))
    return obs.astype(np.int32)


def _symbols(case, m, seed):
    return compressible(m, seed) if case.nsym == 3 else skewed_symbols(m, case.nsym, seed)


def trainer_of(case):
    """The chunk that is created first and trains the dictionary (token cases), or None."""
    return _symbols(case, case.trainer, 7010) if case.tokens else None     # (one seed: the dictionary's size follows the symbols)


def chunks_of(case):
    """The exported chunks of a case, the same symbols whatever the family (the seed follows N and the position)."""
    return [_symbols(case, m, 7100 + 10 * case.n + k) for k, m in enumerate(case.lengths)]


_refs = {}


def reference(oracle, case, b, k, as_operator, fp64=False):
    """(shape, logmass) of chunk k under parameter set b, computed once per process and shared (never modified)."""
    key = (case.n, case.nsym, case.lengths[k], k, b, bool(as_operator), bool(fp64))
    if key not in _refs:
        pi, T, E = hmms_of(case)[b]
        obs = chunks_of(case)[k]
        shape, logmass = oracle.operator_ld(T, E, obs, fp64=fp64) if as_operator else oracle.vector_ld(pi, T, E, obs, fp64=fp64)
        shape.setflags(write=False)
        if as_operator:
            logmass.setflags(write=False)
        _refs[key] = (shape, logmass)
    return _refs[key]


def _columns(values, exps, ref_shape, ref_logmass):
    v = np.asarray(values, dtype=np.float64)
    n = v.shape[0]
    v = v.reshape(n, -1)
    e = np.asarray(exps, dtype=np.int64).reshape(-1)
    ref = np.asarray(ref_shape, dtype=np.float64).reshape(n, -1)
    lm = np.asarray(ref_logmass, dtype=np.float64).reshape(-1)
    assert v.shape == ref.shape and e.shape == lm.shape == (v.shape[1],), (v.shape, ref.shape, e.shape, lm.shape)
    return v, e, ref, lm


def _errors(values, exps, ref_shape, ref_logmass):
    """Per-entry shape errors [N, columns] and per-column scale errors [columns], in long double."""
    v, e, ref, lm = _columns(values, exps, ref_shape, ref_logmass)
    # no exclusions: the test HMMs are dense and positive, so no reference entry is zero and nothing is masked
    assert np.all(np.isfinite(ref)) and np.all(ref > 0) and np.all(np.isfinite(lm)), "the reference has a zero or non-finite entry"
    assert np.all(np.isfinite(v)), "non-finite exported value at %r" % (np.argwhere(~np.isfinite(v))[:4].tolist(),)
    assert np.all(v >= 0), "negative exported value at %r" % (np.argwhere(v < 0)[:4].tolist(),)
    vl = v.astype(np.longdouble)
    mass = vl.sum(axis=0)
    assert np.all(mass > 0), "exported column without mass: %r" % (np.argwhere(~(mass > 0))[:4].tolist(),)
    shape_err = np.abs(vl / mass[None, :] / ref.astype(np.longdouble) - 1)
    got_log = np.log(mass) + e.astype(np.longdouble) * _LN2
    scale_err = np.abs(got_log - lm.astype(np.longdouble)) / np.maximum(np.abs(lm), 1.0)
    return shape_err, scale_err


def compare_state(values, exps, ref_shape, ref_logmass):
    """(worst shape error, worst scale error) of one exported state - a vector ``values[N]`` with one exponent or an
    operator ``values[N, N]`` with one exponent per column, true value ``values * 2**exps`` - against the reference's
    ``(shape, logmass)``.  Raises AssertionError for a non-finite or negative exported value."""
    shape_err, scale_err = _errors(values, exps, ref_shape, ref_logmass)
    return float(shape_err.max()), float(scale_err.max())


def describe_state(values, exps, ref_shape, ref_logmass):
    """Where the worst errors of compare_state are: row and column of the shape error, column of the scale error."""
    shape_err, scale_err = _errors(values, exps, ref_shape, ref_logmass)
    i, c = np.unravel_index(int(np.argmax(shape_err)), shape_err.shape)
    s = int(np.argmax(scale_err))
    return "shape %.3g at row %d column %d, scale %.3g at column %d" % (float(shape_err[i, c]), i, c, float(scale_err[s]), s)


def states_from_reference(shape, logmass):
    """(values, exps) in the exported format from a reference (shape, logmass): per column the exponent
    e = ceil(logmass / ln 2) and values = shape * exp(logmass - e ln 2), computed in long double and rounded once."""
    shape = np.asarray(shape, dtype=np.float64)
    lm = np.asarray(logmass, dtype=np.float64).astype(np.longdouble)
    e = np.ceil(lm / _LN2)
    frac = np.exp(lm - e * _LN2)
    values = (shape.astype(np.longdouble) * (frac[None, :] if shape.ndim == 2 else frac)).astype(np.float64)
    return values, (e.astype(np.int64) if shape.ndim == 2 else int(e))


def shape_tolerance(family):
    return SHAPE_FACTOR * D64[family]


def d64_of(oracle, case):
    """Worst shape deviation of the fp64 variant from the long-double reference over every (parameter set, chunk, mode) of a case."""
    worst = 0.0
    for b in range(3):
        for k in range(len(case.lengths)):
            for as_operator in (True, False):
                shape, logmass = reference(oracle, case, b, k, as_operator)
                s64, l64 = reference(oracle, case, b, k, as_operator, fp64=True)
                zero = np.zeros(np.size(l64))            # (s64's columns sum to 1: exponent 0, log mass 0; only the shape is read)
                worst = max(worst, compare_state(s64, zero, shape, zero)[0])
    return worst


if __name__ == "__main__":
    import time
    from oracle import oracle_lib
    oracle_lib.build()
    table = collections.OrderedDict()
    for case in cases():
        t0 = time.time()
        d = d64_of(oracle_lib, case)
        table[case.family] = max(table.get(case.family, 0.0), d)
        print("%-40s d64 %.3g   (%.1f s)" % (case_id(case), d, time.time() - t0), flush=True)
    for family, d in table.items():
        print("    %r: %.3g,      # tolerance %.3g" % (family, float("%.3g" % d), SHAPE_FACTOR * float("%.3g" % d)))
