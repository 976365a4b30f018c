"""imc_forward_state, entry by entry: every exported forward vector and transfer operator against the long-double
reference of oracle/forward_oracle.c (orc_vector_ld / orc_operator_ld), through state_export_cases.compare_state.

The other GPU modules reduce a chunk to one log-likelihood; operators that have mixed are rank one by then, the last
operator enters only through its column sums, and one entry off by 1e-9 moves the scalar by 1e-13
(tests/test_state_export_cpu.py shows each of these passing the scalar check).  Here every (parameter set, chunk) state
of every case is compared - shape (mantissas, column exponents dropped out) and scale (the column's log mass) apart -
for both export modes, B = 1 and B = 3, several chunks per call, automatic and forced short segments.

Families (state_export_cases.cases() pins them as the other modules do; each call asserts its family in the plan):

  family               kernels                                      N                       stream
  percolumn            k_propagate                                   1 3 4 16 17 33 64       raw
  chain-lds            k_big_propagate + k_chain<NP,0> fold          72                      raw
  blocked-valu         k_zpropagate2 (imc_set_blocked_kernel(2))     10 20                   tokens, raw
  blocked-mfma-lds     k_zpropagate3 (variant 3)                     4 13 20 24              tokens
  blocked-global       k_zpropagate4 (variant 5), hybrid / streamed  10 16 20                tokens (byte level, 16-bit level)
  wide-blocked         k_zpropagate4<7 | 8> (imc_set_wide_blocked)   25 28 32                tokens
  gemm-chain           k_big_propagate                               25 33 48 64 70          tokens, raw
  gemm-chain-150       k_big_propagate                               150                     raw
  gemm-chain-handoff   k_big_propagate + rank-one hand-off           28 70                   raw, 4096-column segments
  alphabet65           k_zpropagate3 (never the per-vector           10                      tokens, 65 symbols
                       k_zpropagate<R,G>) / k_big_propagate          40                      tokens, 65 symbols

Every family of the table exists in operator mode; none was dropped.

Raw chunks: 1, 2, 15, 16, 17, 464 (29 units of 16: a last level-1 run of length 1) and 647 columns (ragged, two chain
levels) in one call, segments automatic and 16.  Token chunks: 4096, 4099 and 6000 columns in one call behind a
40 000-column chunk that trains their dictionary, segments automatic, 48 and 52 tokens (52 is rounded to 64 by the GEMM
chain, taken as it is by the blocked scans).  Hand-off: 3 x 4096 + 133 columns, segments of 4096.
blocked-global only: a 40 000-column chunk trains 36 tokens, every level of which fits LDS at 10 to 20 states, and the
planner then runs k_zpropagate3 whatever the variant; its dictionary is trained by 800 000 columns instead (2727
tokens), and each case runs on the level the planner picks (a byte level) and pinned to the 384-token level
(IMC_FORCE_LEVEL=11: 16-bit tokens).  The exported chunks are the same.

Tolerances (none taken from the device):
  shape  16 x the family's worst d64 - the deviation of the oracle's fp64 variant from its long-double variant over the
         family's cases (state_export_cases.D64, measured on the CPU) - plus, where the plan ran the rank-one hand-off,
         R1_TOL = 2^-42 per operator segment of the chunk (kernels_big.hpp's own component-wise claim);
  scale  1e-11 relative to |log mass|, absolute below 1.

d64 per case (`python tests/state_export_cases.py`; worst over the three parameter sets, the chunks and both modes):
  percolumn           n1 0, n3 9.4e-16, n4 7.6e-16, n16 2.9e-15, n17 1.7e-15, n33 4.5e-15, n64 4.6e-15   -> tolerance 7.4e-14
  chain-lds           n72 4.5e-15                                                                         -> 7.1e-14
  blocked-valu        n10 1.3e-15 (tokens) 1.4e-15 (raw), n20 1.9e-15 (tokens) 2.9e-15 (raw)              -> 4.6e-14
  blocked-mfma-lds    n4 3.2e-16, n13 9.2e-16, n20 1.9e-15, n24 2.7e-15                                   -> 4.3e-14
  blocked-global      n10 1.3e-15, n16 1.4e-15, n20 1.9e-15                                               -> 3.1e-14
  wide-blocked        n25 1.5e-15, n28 1.5e-15, n32 1.9e-15                                               -> 3.1e-14
  gemm-chain          tokens: n25 1.5e-15, n33 1.2e-15, n48 2.9e-15, n64 4.1e-15, n70 1.9e-15;
                      raw: n25 2.3e-15, n33 4.5e-15, n48 4.2e-15, n64 4.6e-15, n70 4.7e-15                -> 7.4e-14
  gemm-chain-150      n150 2.1e-14 (kept apart so that it does not widen the tolerance of 25 to 70 states) -> 3.3e-13
  gemm-chain-handoff  n28 1.2e-15, n70 1.1e-15                       -> 1.8e-14 + 2^-42 per operator segment (<= 7.0e-13)
  alphabet65          n10 9.0e-16, n40 1.8e-15                                                            -> 2.8e-14
Measured on the MI355X, worst shape error per family (beside its d64): percolumn 4.7e-15 (4.6e-15), chain-lds 6.9e-15
(4.5e-15), blocked-valu 7.8e-15 (2.9e-15), blocked-mfma-lds 1.4e-14 (2.7e-15), blocked-global 1.1e-14 (1.9e-15),
wide-blocked 2.2e-14 (1.9e-15; 32 states, 48-token segments: 0.7 x the tolerance, the closest of all), gemm-chain 1.3e-14
(4.7e-15), gemm-chain-150 3.8e-14 (2.1e-14), gemm-chain-handoff 2.4e-15 (1.2e-15), alphabet65 3.8e-15 (1.8e-15); worst
scale error 8.9e-16.  Each case prints its own figures.
"""
import math
import os

import numpy as np
import pytest

import state_export_cases as sx
from imcoalhmm_amd import Forwarder, _capi
from imcoalhmm_amd.hmm import forward_states

pytestmark = pytest.mark.gpu
CASES = sx.cases()


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    assert _capi.lib().imc_device_count() >= 1, "gpu tests need a device"
    yield
    restore()


def restore():
    L = _capi.lib()
    L.imc_set_segment_length(0)
    L.imc_set_blocked_kernel(4)
    L.imc_set_table_streaming(-1)
    L.imc_set_wide_blocked(-1)
    L.imc_set_compression(1)
    L.imc_dictionary_reset()


def pin(case):
    L = _capi.lib()
    _capi.check(L.imc_set_blocked_kernel(case.blocked))
    _capi.check(L.imc_set_table_streaming(case.streaming))
    _capi.set_wide_blocked(case.wide)
    _capi.check(L.imc_set_compression(case.zip))
    _capi.check(L.imc_dictionary_reset())


def run_case(oracle, case):
    """Every state of a case: one record per (segment length, B, export mode, parameter set, chunk).  A call that did
    not run the case's family is an error."""
    hmms = sx.hmms_of(case)
    chunks = sx.chunks_of(case)
    records = []
    try:
        pin(case)
        if case.level is not None:
            os.environ["IMC_FORCE_LEVEL"] = str(case.level)      # (read when a plan is built)
        trainer = Forwarder.from_array(sx.trainer_of(case), case.nsym) if case.tokens else None     # created first; not exported
        fw = [Forwarder.from_array(c, case.nsym) for c in chunks]
        handles = [f.handle for f in fw]
        for seg in case.segs:
            _capi.check(_capi.lib().imc_set_segment_length(seg))
            for B in (1, 3):
                pis, Ts, Es = (np.stack([h[k] for h in hmms[:B]]) for k in range(3))
                for as_operator in (True, False):
                    values, exps = forward_states(handles, pis, Ts, Es, as_operator)
                    plan = _capi.last_plan()
                    what = (sx.case_id(case), "seg %d" % seg, "B %d" % B, "operator" if as_operator else "vector")
                    assert all(s in plan["kernels"] for s in case.expect), (what, case.expect, plan)
                    assert not any(s in plan["kernels"] for s in case.reject), (what, case.reject, plan)
                    handoff = "rank1-handoff" in plan["kernels"]
                    seglen = plan["token_segment_len"] if case.tokens else plan["column_segment_len"]
                    for b in range(B):
                        for k, c in enumerate(chunks):
                            ref = sx.reference(oracle, case, b, k, as_operator)
                            shape_err, scale_err = sx.compare_state(values[b, k], exps[b, k], *ref)
                            tol = sx.shape_tolerance(case.family)
                            if handoff:      # one component-wise 2^-42 per operator segment of this chunk
                                tol += sx.R1_TOL * (math.ceil(c.size / seglen) - (0 if as_operator else 1))
                            records.append(dict(what=what + ("set %d" % b, "chunk %d (%d columns)" % (k, c.size)), kernels=plan["kernels"],
                                                shape=shape_err, scale=scale_err, tol=tol,
                                                where=sx.describe_state(values[b, k], exps[b, k], *ref)))
        del trainer, fw
    finally:
        os.environ.pop("IMC_FORCE_LEVEL", None)
        restore()
    return records


@pytest.mark.parametrize("case", CASES, ids=sx.case_id)
def test_exported_states_entry_by_entry(oracle, case):
    records = run_case(oracle, case)
    assert len(records) == len(case.segs) * (1 + 3) * 2 * len(case.lengths)       # no state left out
    worst_shape = max(records, key=lambda r: r["shape"] / r["tol"])
    worst_scale = max(records, key=lambda r: r["scale"])
    print("%s: worst shape error %.3g (tolerance %.3g) at %s; worst scale error %.3g at %s; kernels %s" % (
        sx.case_id(case), worst_shape["shape"], worst_shape["tol"], "/".join(worst_shape["what"][1:]), worst_scale["scale"],
        "/".join(worst_scale["what"][1:]), sorted({r["kernels"] for r in records})))
    bad = [r for r in records if not (r["shape"] <= r["tol"] and r["scale"] <= sx.SCALE_TOL)]
    assert not bad, (len(bad), len(records), [(r["what"], r["where"], r["tol"], r["kernels"]) for r in bad[:6]])
