"""The column-split form of the two-depth table kernel (k_z4_level2<NT, FIRST, W>: one token per wavefront, the four
blocks of the matrix instruction hold four column tiles of that token) against the four-tokens-per-wavefront form.

Every output tile is accumulated by the same MFMA sequence on the same operands and the rescale picks the same power of
two, so IMC_TABLE_SPLIT must change nothing but the schedule: log-likelihoods bit-equal with the switch off, on (the
launches of at most about one wavefront per SIMD) and on for every launch (IMC_TABLE_SPLIT_MAX), with the first launch
fetching the parameters itself (IMC_FUSE_HEAD=1: the FIRST instantiations) or not; and every value within the suite's
1e-11 of the CPU oracle.  States 4 .. 24 cover every NT = 1 .. 6, i.e. both pass counts (one pass of column tiles up to
16 states, two at 20 and 24) and the padding tiles of NT = 1, 2, 3, 5, 6; three dictionary levels each (byte and 16-bit
token streams); one parameter set and three.  IMC_TABLE_TRIPLES=0 throughout: up to 12 states the three-depth kernel
would otherwise build the table.  (Own processes: the switches are read when the library's context is created.)"""
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
STATES = (4, 8, 10, 12, 16, 20, 24)
LEVELS = (9, 11, 13)
LENGTHS = (1_000_000, 4099, 150_000)


def hmms_of(n):
    from imcoalhmm_amd import synth
    return [synth.random_hmm(n, 3, seed=7100 + n + b, stay=0.995) for b in range(3)]


def chunks_of(n, hmms):
    from imcoalhmm_amd import synth
    return [synth.sample_alignment(*hmms[0], m, seed=31 + n + k) for k, m in enumerate(LENGTHS)]


CHILD = textwrap.dedent('''
    import json, os, sys
    import numpy as np
    sys.path.insert(0, %r)
    sys.path.insert(0, os.path.join(%r, "tests"))
    from imcoalhmm_amd import Forwarder, _capi
    from imcoalhmm_amd.hmm import forward_chunks_batch
    import test_gpu_table_split as T
    L = _capi.lib()
    _capi.check(L.imc_set_compression(3)); _capi.check(L.imc_set_blocked_kernel(5))
    out = {}
    for n in T.STATES:
        hmms = T.hmms_of(n)
        fw = [Forwarder.from_array(c, 3) for c in T.chunks_of(n, hmms)]
        for lvl in T.LEVELS:
            os.environ["IMC_FORCE_LEVEL"] = str(lvl)
            for B in (1, 3):
                v = forward_chunks_batch([f.handle for f in fw], *(np.stack([h[k] for h in hmms[:B]]) for k in range(3)), per_chunk=True)
                out["%%d/%%d/%%d" %% (n, lvl, B)] = {"kernels": _capi.last_plan()["kernels"], "values": [float(x).hex() for x in v.ravel()]}
            del os.environ["IMC_FORCE_LEVEL"]
        del fw
        _capi.check(L.imc_dictionary_reset())
    print(json.dumps(out))
''') % (REPO, REPO)


def test_table_split_changes_nothing_but_the_schedule(tmp_path, oracle):
    script = tmp_path / "split.py"
    script.write_text(CHILD)
    outs = {}
    for split in ("0", "1", "all"):
        for fuse in ("1", "0"):
            env = dict(os.environ, IMC_TABLE_TRIPLES="0", IMC_FUSE_HEAD=fuse, IMC_TABLE_SPLIT="0" if split == "0" else "1")
            env.pop("IMC_TABLE_SPLIT_MAX", None)
            if split == "all":
                env["IMC_TABLE_SPLIT_MAX"] = str(1 << 30)
            r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=900, env=env)
            assert r.returncode == 0, (split, fuse, r.stdout[-500:], r.stderr[-2000:])
            outs[(split, fuse)] = json.loads(r.stdout.strip().splitlines()[-1])
    base = outs[("0", "1")]
    # the routes: the global-table kernel at every level beyond 8 states and at one level at least below (up to 8 states a
    # byte level's table fits LDS); the split form only - and then always - where the switch allows it
    for n in STATES:
        on_table = [k for k in base if k.startswith("%d/" % n) and "k_zpropagate4" in base[k]["kernels"]]
        assert len(on_table) == 2 * len(LEVELS) if n > 8 else len(on_table) >= 2, (n, {k: base[k]["kernels"] for k in base})
    for (split, fuse), res in outs.items():
        for key, rec in res.items():
            want = split != "0" and "k_zpropagate4" in rec["kernels"]
            assert ("table-split" in rec["kernels"]) == want, (split, fuse, key, rec["kernels"])
    # (a) bit-equal whatever the form
    for setting, res in outs.items():
        for key in base:
            print(setting, key, res[key]["kernels"], res[key]["values"] == base[key]["values"])
            assert res[key]["values"] == base[key]["values"], (setting, key, res[key], base[key])
    # (b) the CPU oracle
    worst = 0.0
    for n in STATES:
        hmms = hmms_of(n)
        chunks = chunks_of(n, hmms)
        want = [[oracle.forward_scaled(*hmms[b], c) for c in chunks] for b in range(3)]
        for lvl in LEVELS:
            for B in (1, 3):
                got = [float.fromhex(x) for x in base["%d/%d/%d" % (n, lvl, B)]["values"]]
                for b in range(B):
                    for k in range(len(chunks)):
                        err = abs(got[b * len(chunks) + k] - want[b][k]) / abs(want[b][k])
                        worst = max(worst, err)
                        assert err <= TOL, (n, lvl, B, b, k, got[b * len(chunks) + k], want[b][k])
    print("worst relative error against the oracle: %.3g" % worst)
