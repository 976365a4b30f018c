"""A cached plan is replayed only under the options it was built under (csrc/options_host.hpp: same_plan_options is
the plan key's comparison, and a plan's launches read the record the plan keeps, not the live context).

For each pair of settings the same chunks are evaluated under A, B, A, B in one process.  Each call must name its
setting's kernel family in imc_last_kernels() - a stale plan served under the other setting names the other one - calls
1 and 3 and calls 2 and 4 must agree bit for bit, and all four must be within the suite's 1e-11 relative of
oracle.forward_scaled, chunk by chunk - a plan rebuilt wrongly is not.

Shapes are the smallest at which the families differ (tests/state_export_cases.py): chunks of 4096, 4099 and 6000
columns of three symbols behind a 40 000-column chunk that trains their dictionary - 800 000 columns where the global
table is needed - and for the rank-one hand-off one raw chunk of 3 x 4096 + 133 columns in forced 4096-column segments."""
import numpy as np
import pytest

import state_export_cases as sx
from conftest import rel_err
from imcoalhmm_amd import Forwarder, _capi
from imcoalhmm_amd.hmm import forward_chunks_batch

pytestmark = pytest.mark.gpu
TOL = 1e-11


def restore():
    L = _capi.lib()
    L.imc_set_segment_length(0)
    L.imc_set_blocked_kernel(4)
    L.imc_set_table_streaming(-1)
    L.imc_set_wide_blocked(-1)
    L.imc_set_rank1_handoff(1)
    L.imc_set_compression(1)
    L.imc_dictionary_reset()


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    assert _capi.lib().imc_device_count() >= 1, "gpu tests need a device"
    yield
    restore()


def _case(family, n, tokens=True, streaming=-1):
    return next(c for c in sx.cases() if (c.family, c.n, c.tokens, c.streaming, c.level) == (family, n, tokens, streaming, None))


_refs = {}


def reference(oracle, case):
    """Per-chunk log-likelihoods of the case's chunks under its first parameter set: computed once, shared, read-only."""
    key = (case.n, case.nsym, case.lengths)
    if key not in _refs:
        pi, T, E = sx.hmms_of(case)[0]
        ref = np.array([oracle.forward_scaled(pi, T, E, obs) for obs in sx.chunks_of(case)])
        ref.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


def setter(name):
    return lambda value: _capi.check(getattr(_capi.lib(), name)(value))


def alternate(oracle, case, base, flip, a, b, expect_a, expect_b, reject_a=(), reject_b=(), look=None):
    """base: (setter name, value) pairs that hold for all four calls; flip: the setter under test; a / b: its two values;
    expect / reject: substrings of imc_last_kernels() that must / must not appear under each.  look(plan, value):
    further assertions on imc_last_plan()."""
    ref = reference(oracle, case)
    pi, T, E = sx.hmms_of(case)[0]
    try:
        restore()
        for name, value in base:
            setter(name)(value)
        trainer = Forwarder.from_array(sx.trainer_of(case), case.nsym) if case.tokens else None   # created first: trains the dictionary
        fw = [Forwarder.from_array(c, case.nsym) for c in sx.chunks_of(case)]
        handles = [f.handle for f in fw]
        got, names, plans = [], [], []
        for value in (a, b, a, b):
            setter(flip)(value)
            got.append(forward_chunks_batch(handles, pi[None], T[None], E[None], per_chunk=True)[0].copy())
            plans.append(_capi.last_plan())
            names.append(plans[-1]["kernels"])
        print(flip, (a, b), names, [float(np.max(np.abs(g / ref - 1))) for g in got])
        for call, value in enumerate((a, b, a, b)):
            expect, reject = (expect_a, reject_a) if value == a else (expect_b, reject_b)
            assert all(s in names[call] for s in expect), (flip, call, value, expect, names)
            assert not any(s in names[call] for s in reject), (flip, call, value, reject, names)
            if look:
                look(plans[call], value)
        assert names[0] == names[2] and names[1] == names[3], names
        assert np.array_equal(got[0], got[2]) and np.array_equal(got[1], got[3]), (flip, got)
        for call in range(4):
            for k in range(len(ref)):
                assert rel_err(float(got[call][k]), float(ref[k])) < TOL, (flip, call, k, got[call][k], ref[k])
        del trainer, fw
    finally:
        restore()


def test_blocked_kernel_variant(oracle):
    alternate(oracle, _case("blocked-valu", 10), [("imc_set_compression", 3)], "imc_set_blocked_kernel", 3, 2,
              ("k_zpropagate3<",), ("k_zpropagate2<",), reject_a=("k_zpropagate2<",), reject_b=("k_zpropagate3<",))


def test_compression(oracle):
    alternate(oracle, _case("blocked-valu", 10), [], "imc_set_compression", 1, 0, ("[tokens]",), ("[columns]",),
              reject_a=("[columns]",), reject_b=("[tokens]",))


def test_segment_length(oracle):
    first = []       # the propagate kernel of each call: the first entry of the list (what follows says how the chunks were stitched)

    def look(plan, value):
        first.append(plan["kernels"].split("+")[0])
        if value:
            assert plan["token_segment_len"] == value, plan

    alternate(oracle, _case("blocked-valu", 10), [("imc_set_compression", 3)], "imc_set_segment_length", 0, 48,
              ("k_zpropagate3<", "[tokens]"), ("k_zpropagate3<", "[tokens]"), look=look)
    assert len(set(first)) == 1, first


def test_table_streaming(oracle):
    alternate(oracle, _case("blocked-global", 10, streaming=1), [("imc_set_compression", 3), ("imc_set_blocked_kernel", 5)], "imc_set_table_streaming", 1, 0,
              ("k_zpropagate4<", "streamed"), ("k_zpropagate4<",), reject_b=("streamed",))


def test_wide_blocked(oracle):
    alternate(oracle, _case("wide-blocked", 28), [], "imc_set_wide_blocked", 1, 0, ("k_zpropagate4<7",), (), reject_b=("k_zpropagate4<7",))


def test_rank1_handoff(oracle):
    alternate(oracle, _case("gemm-chain-handoff", 28, tokens=False), [("imc_set_compression", 5), ("imc_set_segment_length", 4096)],
              "imc_set_rank1_handoff", 1, 0, ("k_big_propagate", "rank1-handoff"), ("k_big_propagate",), reject_b=("rank1-handoff",))
