"""The stitch's chain step (k_chain<NP, D > 0>): the rescaled vector handed from lane to lane in registers (the default)
against the step that sends it through LDS (IMC_CHAIN_LDS=1).

Both forms apply the same FMAs and adds to the same operands in the same order, so the switch must change nothing but
the schedule: per-chunk log-likelihoods bit-equal between a process with the default environment and one with
IMC_CHAIN_LDS=1, and every value of the default process within the suite's 1e-11 of the CPU oracle.

State counts where the lane layout can go wrong: 4, 10, 16 (exactly one 16-lane row), 17 (one lane in the second row),
20, 24, 32, 33, 64 (a full wavefront), and 72 (the LDS-only k_chain<NP, 0>, which the switch does not touch).  Raw
column stream on the per-column kernel (imc_set_compression(4): a stitch unit is a segment; 72 states: mode 0, the
kernels of that size), 16-column segments: the 40 000-column chunk is 2500 stitch units, deep enough for three chain
levels with ragged last runs; beside it, in the same call, a chunk of a single unit (no chain), a 464-column chunk of
29 units (its level-1 runs are 14 + 14 + 1: a run of length 1 at the end) and an empty chunk (k_finish writes its 0.0).
One parameter set and three (blockIdx.y).  One more case at 20 states on the blocked fp64-MFMA scan with short token
segments, where a stitch unit is a workgroup's folded operator.  (Own processes: the switch is read when the library's
context is created.)"""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-11
STATES = (4, 10, 16, 17, 20, 24, 32, 33, 64, 72)
LENGTHS = (40_000, 10, 464, 0)
BLOCKED_STATES, BLOCKED_LENGTHS = 20, (600_000, 150_000)
BATCHES = (1, 3)


def hmms_of(n):
    from imcoalhmm_amd import synth
    return [synth.random_hmm(n, 3, seed=8200 + n + b, stay=0.9) for b in range(3)]


def chunks_of(n):
    rng = np.random.default_rng(77 + n)
    return [rng.integers(0, 3, size=m).astype(np.uint8) for m in LENGTHS]


def blocked_chunks(hmms):
    from imcoalhmm_amd import synth
    return [synth.sample_alignment(*hmms[0], m, seed=91 + k) for k, m in enumerate(BLOCKED_LENGTHS)]


CHILD = textwrap.dedent('''
    import json, os, sys
    import numpy as np
    sys.path.insert(0, %r)
    sys.path.insert(0, os.path.join(%r, "tests"))
    from imcoalhmm_amd import Forwarder, _capi
    from imcoalhmm_amd.hmm import forward_chunks_batch
    import test_gpu_chain_step as T
    L = _capi.lib()
    out = {}

    def run(key, chunks, hmms):
        fw = [Forwarder.from_array(c, 3) for c in chunks]
        for B in T.BATCHES:
            v = forward_chunks_batch([f.handle for f in fw], *(np.stack([h[k] for h in hmms[:B]]) for k in range(3)), per_chunk=True)
            plan = _capi.last_plan()
            out["%%s/%%d" %% (key, B)] = {"kernels": plan["kernels"], "segments": plan["segments"], "vectors": plan["vectors"],
                                        "values": [float(x).hex() for x in v.ravel()]}

    _capi.check(L.imc_set_segment_length(16))
    for n in T.STATES:
        _capi.check(L.imc_set_compression(4 if n <= 64 else 0))
        run("raw%%d" %% n, T.chunks_of(n), T.hmms_of(n))
    _capi.check(L.imc_set_compression(3)); _capi.check(L.imc_set_segment_length(64))
    hmms = T.hmms_of(T.BLOCKED_STATES)
    run("blocked%%d" %% T.BLOCKED_STATES, T.blocked_chunks(hmms), hmms)
    print(json.dumps(out))
''') % (REPO, REPO)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    script = tmp_path_factory.mktemp("chain_step") / "chain.py"
    script.write_text(CHILD)
    outs = {}
    for lds in (False, True):
        env = dict(os.environ)
        env.pop("IMC_CHAIN_LDS", None)
        if lds:
            env["IMC_CHAIN_LDS"] = "1"
        r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, (lds, r.stdout[-500:], r.stderr[-2000:])
        outs[lds] = json.loads(r.stdout.strip().splitlines()[-1])
    return outs


def units_of(rec, n, nonempty):
    # every non-empty chunk starts with one vector; each further unit is an operator of n vectors
    return (rec["vectors"] - nonempty) // n + nonempty


def test_cases_reach_the_chain(runs):
    """The shapes are what the docstring says: three chain levels on the raw stream (more than 16 x 12 units in one chunk);
    on the token stream workgroup operators of the blocked scan, more than a last level holds, and no fused tail."""
    for n in STATES:
        for B in BATCHES:
            rec = runs[False]["raw%d/%d" % (n, B)]
            print(n, B, rec["kernels"], rec["segments"], rec["vectors"])
            if n <= 64:
                assert "k_propagate" in rec["kernels"] and units_of(rec, n, 3) == 2500 + 1 + 29, (n, B, rec)
    for B in BATCHES:
        rec = runs[False]["blocked%d/%d" % (BLOCKED_STATES, B)]
        print("blocked", B, rec["kernels"], rec["segments"], rec["vectors"])
        assert "k_zpropagate" in rec["kernels"] and "fused-tail" not in rec["kernels"], rec["kernels"]
        assert units_of(rec, BLOCKED_STATES, 2) > 32, rec


def test_lds_switch_changes_no_bit(runs):
    assert runs[False].keys() == runs[True].keys()
    for key, rec in runs[False].items():
        print(key, rec["values"], runs[True][key]["values"] == rec["values"])
        assert runs[True][key]["values"] == rec["values"], (key, rec["values"], runs[True][key]["values"])
        assert runs[True][key]["kernels"] == rec["kernels"], (key, rec["kernels"], runs[True][key]["kernels"])


def test_default_step_agrees_with_the_oracle(runs, oracle):
    worst = 0.0
    cases = [("raw%d" % n, hmms_of(n), chunks_of(n)) for n in STATES]
    hb = hmms_of(BLOCKED_STATES)
    cases.append(("blocked%d" % BLOCKED_STATES, hb, blocked_chunks(hb)))
    for key, hmms, chunks in cases:
        want = [[oracle.forward_scaled(*hmms[b], c) if len(c) else 0.0 for c in chunks] for b in range(max(BATCHES))]
        for B in BATCHES:
            got = [float.fromhex(x) for x in runs[False]["%s/%d" % (key, B)]["values"]]
            assert len(got) == B * len(chunks)
            for b in range(B):
                for k in range(len(chunks)):
                    g, w = got[b * len(chunks) + k], want[b][k]
                    if w == 0.0:
                        assert g == 0.0, (key, B, b, k, g)
                        continue
                    err = abs(g - w) / abs(w)
                    worst = max(worst, err)
                    assert err <= TOL, (key, B, b, k, g, w, err)
    print("worst relative error against the oracle: %.3g" % worst)
