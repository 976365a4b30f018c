"""The long-double state reference (orc_operator_ld / orc_vector_ld) and the state comparer, on the CPU.

First the reference against itself and against independent statements of the same objects; then four faults of the
kind a kernel's lane mapping or a fold can commit, each of which today's scalar check (the recombined log-likelihood
at 1e-11 relative) lets through and state_export_cases.compare_state does not."""
import numpy as np
import pytest

from conftest import rel_err
from imcoalhmm_amd import synth
from imcoalhmm_amd.hmm import combine_states
from state_export_cases import (SCALE_TOL, SHAPE_FACTOR, compare_state, compressible, describe_state, states_from_reference)

pytestmark = pytest.mark.skipif(np.finfo(np.longdouble).eps >= 1e-18,
                                reason="numpy's long double is no wider than double here: the comparer needs the extended type")
TOL = 1e-11                          # the suite's tolerance on a log-likelihood
CUTS = (0, 1000, 2000, 3000)         # three slices, each several mixing times long (stay 0.95: a few hundred columns)


@pytest.fixture(scope="module")
def split(oracle):
    """A three-slice alignment under a mixed 20-state HMM: per slice the long-double reference, the fp64 variant's
    states in the exported format, and d64 - the fp64 variant's own worst shape deviation."""
    pi, T, E = synth.random_hmm(20, 3, seed=8160, stay=0.95)
    whole = compressible(CUTS[-1], seed=21)
    pieces = [whole[a:b] for a, b in zip(CUTS[:-1], CUTS[1:])]
    ref = [oracle.vector_ld(pi, T, E, pieces[0])] + [oracle.operator_ld(T, E, p) for p in pieces[1:]]
    f64 = [oracle.vector_ld(pi, T, E, pieces[0], fp64=True)] + [oracle.operator_ld(T, E, p, fp64=True) for p in pieces[1:]]
    states = [states_from_reference(*s) for s in f64]
    d64 = max(compare_state(v, e, *r)[0] for (v, e), r in zip(states, ref))
    return dict(hmm=(pi, T, E), whole=whole, pieces=pieces, ref=ref, states=states, d64=d64)


def recombined(states):
    (vec, vexp), ops = states[0], states[1:]
    return combine_states(vec, vexp, [v for v, _ in ops], [e for _, e in ops])


def test_reference_states_recombine_to_the_whole_alignment(oracle, split):
    """Vector of the first slice, operators of the others, all from the long-double reference: combine_states gives
    forward_scaled_ld of the whole alignment.  (1e-12: a log mass rounded to double is off by up to 1e-13 absolute.)"""
    pi, T, E = split["hmm"]
    got = recombined([states_from_reference(*s) for s in split["ref"]])
    want = oracle.forward_scaled_ld(pi, T, E, split["whole"])
    assert rel_err(got, want) < 1e-12, (got, want)
    # ... and the vector's log mass alone is the first slice's log-likelihood
    assert rel_err(split["ref"][0][1], oracle.forward_scaled_ld(pi, T, E, split["pieces"][0])) < 1e-15
    for shape, _ in split["ref"]:
        assert np.allclose(shape.sum(axis=0), 1.0, rtol=0, atol=1e-15) and np.all(shape > 0)


def test_reference_agrees_with_numpy_state(oracle, hmm_params):
    """The plain-numpy states of test_dist_gloo.py (fp64, a different rescaling rule) on a small case: within the shape
    tolerance rule (16 x the fp64 variant's own deviation) and the scale tolerance."""
    from test_dist_gloo import _numpy_state
    pi, T, E = hmm_params("iso10_t0")
    obs = synth.sample_alignment(pi, T, E, 300, seed=12)
    for as_operator in (True, False):
        ref = oracle.operator_ld(T, E, obs) if as_operator else oracle.vector_ld(pi, T, E, obs)
        f64 = oracle.operator_ld(T, E, obs, fp64=True) if as_operator else oracle.vector_ld(pi, T, E, obs, fp64=True)
        d64 = compare_state(*states_from_reference(*f64), *ref)[0]
        values, exps = _numpy_state(pi, T, E, obs, as_operator)
        shape_err, scale_err = compare_state(values, exps, *ref)
        print("operator" if as_operator else "vector", "d64 %.3g numpy shape %.3g scale %.3g" % (d64, shape_err, scale_err))
        assert 0 < d64 < 1e-13
        assert shape_err <= SHAPE_FACTOR * d64 and scale_err <= SCALE_TOL, describe_state(values, exps, *ref)


def test_one_column_operator_is_the_definition(oracle):
    """L = 1: P = diag(E[:,o]) T' (the first column acts as an operator too), to rounding of the reference's output."""
    pi, T, E = synth.random_hmm(13, 3, seed=5, stay=0.9)
    for o in range(3):
        shape, logmass = oracle.operator_ld(T, E, np.array([o], dtype=np.uint8))
        assert np.allclose(shape * np.exp(logmass)[None, :], E[:, o][:, None] * T.T, rtol=1e-15, atol=0)
        vshape, vmass = oracle.vector_ld(pi, T, E, np.array([o], dtype=np.uint8))
        assert np.allclose(vshape * np.exp(vmass), pi * E[:, o], rtol=1e-15, atol=0)


def test_sixteen_bit_observations_are_the_same_function(oracle):
    """Alphabets beyond 256 symbols take 16-bit observations: on symbols that both forms can carry, bit-equal results;
    and symbol 256 is read (a one-column operator again)."""
    pi, T, E = synth.random_hmm(7, 257, seed=9, stay=0.9)
    obs = np.random.default_rng(3).integers(0, 256, size=200)
    E8 = np.ascontiguousarray(E[:, :256])
    for fp64 in (False, True):
        a, b = oracle.operator_ld(T, E, obs, fp64=fp64), oracle.operator_ld(T, E8, obs, fp64=fp64)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        a, b = oracle.vector_ld(pi, T, E, obs, fp64=fp64), oracle.vector_ld(pi, T, E8, obs, fp64=fp64)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    shape, logmass = oracle.operator_ld(T, E, np.array([256]))
    assert np.allclose(shape * np.exp(logmass)[None, :], E[:, 256][:, None] * T.T, rtol=1e-15, atol=0)


def test_unfaulted_fp64_states_pass_both_checks(oracle, split):
    pi, T, E = split["hmm"]
    assert rel_err(recombined(split["states"]), oracle.forward_scaled_ld(pi, T, E, split["whole"])) < TOL
    assert 0 < split["d64"] < 1e-13, split["d64"]
    for (v, e), r in zip(split["states"], split["ref"]):
        shape_err, scale_err = compare_state(v, e, *r)
        assert shape_err <= SHAPE_FACTOR * split["d64"] and scale_err <= SCALE_TOL


def faulted(split, which, fault):
    states = [(v.copy(), np.array(e).copy()) for v, e in split["states"]]
    fault(*states[which])
    return states


def swap_rows(values, exps):
    values[[3, 11]] = values[[11, 3]]


def scale_one_entry(values, exps):
    values[5, 7] *= 1.0 + 1e-9


def swap_entries(values, exps):
    values[[2, 17]] = values[[17, 2]]


@pytest.mark.parametrize("name,which,fault", [("rows of the last operator swapped", 2, swap_rows),
                                              ("one entry of a middle operator scaled by 1 + 1e-9", 1, scale_one_entry)])
def test_scalar_passes_comparer_fails(oracle, split, name, which, fault):
    """(a), (b): the recombined log-likelihood moves by less than the suite's tolerance - today's check passes - while
    the comparer reports a shape error beyond its tolerance, on the faulted state and on no other; the scale stays."""
    pi, T, E = split["hmm"]
    want = oracle.forward_scaled_ld(pi, T, E, split["whole"])
    states = faulted(split, which, fault)
    moved = rel_err(recombined(states), recombined(split["states"]))
    tol = SHAPE_FACTOR * split["d64"]
    errs = [compare_state(v, e, *r) for (v, e), r in zip(states, split["ref"])]
    print("%s: log-likelihood moved %.3g relative; shape errors %r against %.3g" % (name, moved, [x[0] for x in errs], tol))
    assert moved < TOL and rel_err(recombined(states), want) < TOL                      # scalar passes
    assert errs[which][0] > tol, describe_state(*states[which], *split["ref"][which])   # comparer fails
    assert all(x[0] <= tol for k, x in enumerate(errs) if k != which)
    assert all(x[1] <= SCALE_TOL for x in errs)


def test_permuted_vector_passes_the_first_slice_check(oracle, split):
    """(c): the exported vector alone, as the "first slice" check reads it - only its sum enters."""
    pi, T, E = split["hmm"]
    (v, e), = faulted(split, 0, swap_entries)[:1]
    first = combine_states(v, e, [], [])
    assert rel_err(first, oracle.forward_scaled_ld(pi, T, E, split["pieces"][0])) < TOL
    shape_err, scale_err = compare_state(v, e, *split["ref"][0])
    print("vector entries swapped: shape error %.3g, scale error %.3g" % (shape_err, scale_err))
    assert shape_err > SHAPE_FACTOR * split["d64"] and scale_err <= SCALE_TOL


def test_swapped_exponents_show_in_the_scale_alone(split):
    """(d): two columns of the last operator exchange their exponents: the mantissas are untouched, so the shape
    passes and the scale fails - a wrong exponent and a wrong mantissa are told apart."""
    values, exps = split["states"][2]
    c0 = 0
    differ = np.flatnonzero(exps != exps[c0])
    assert differ.size, "the case needs two columns with different exponents: %r" % (exps,)
    c1 = int(differ[0])

    def swap_exponents(values, exps):
        exps[[c0, c1]] = exps[[c1, c0]]
    v, e = faulted(split, 2, swap_exponents)[2]
    shape_err, scale_err = compare_state(v, e, *split["ref"][2])
    print("exponents of columns %d and %d swapped (%d, %d): shape error %.3g, scale error %.3g" % (c0, c1, exps[c0], exps[c1], shape_err, scale_err))
    assert shape_err <= SHAPE_FACTOR * split["d64"]
    assert scale_err > SCALE_TOL


def test_recorded_tolerances_come_from_the_reference(oracle):
    """Every family of the GPU module has a recorded d64 (no tolerance is a default), both streams appear where the
    table says so, and the record is reproduced here, from the reference alone, for the cases that cost nothing (up to
    24 states): no case deviates by more than its family's record."""
    import state_export_cases as sx
    cases = sx.cases()
    assert sorted(sx.D64) == sx.families()
    assert all(0 < d < 1e-12 for d in sx.D64.values()), sx.D64
    for family in ("blocked-valu", "gemm-chain"):
        assert {c.tokens for c in cases if c.family == family} == {True, False}
    measured = {}
    for case in cases:
        if case.n <= 24 and case.level is None and case.streaming <= 0:
            d = sx.d64_of(oracle, case)
            measured[case.family] = max(measured.get(case.family, 0.0), d)
            # (within 2 x: how the compiler contracts the fp64 variant's multiply-adds is the host's, and d64 is a maximum of rounding noise)
            assert d <= 2.0 * sx.D64[case.family], (sx.case_id(case), d, sx.D64[case.family])
    print({k: "%.3g of %.3g" % (v, sx.D64[k]) for k, v in measured.items()})
    # ... and where every case of a family is cheap, the record is that maximum itself: it is not overstated either
    for family in ("blocked-valu", "blocked-mfma-lds", "blocked-global"):
        assert measured[family] >= 0.5 * sx.D64[family], (family, measured[family], sx.D64[family])


def test_comparer_refuses_what_it_must_not_skip(split):
    values, exps = split["states"][1]
    bad = values.copy(); bad[4, 4] = np.nan
    with pytest.raises(AssertionError):
        compare_state(bad, exps, *split["ref"][1])
    bad = values.copy(); bad[4, 4] = -bad[4, 4]
    with pytest.raises(AssertionError):
        compare_state(bad, exps, *split["ref"][1])
    shape, logmass = split["ref"][1]
    zero = shape.copy(); zero[0, 0] = 0.0
    with pytest.raises(AssertionError):
        compare_state(values, exps, zero, logmass)
