"""A plan owns its device memory (DevBuf in csrc/engine_core.hpp): erasing it from the plan list - eviction of the least
recently used plan, the chunk filters of imc_obs_free and imc_obs_recompress - gives back every buffer it allocated.
Pinned here with something other than the code under test: the device's own free-memory figure, read through torch.

One cycle evaluates five distinct plans (10, 20, 28, 48 and 100 states, three parameter sets) on one long chunk, on a
set of three ragged chunks (70 001 / 0 / 4 099 columns) or on all four - one more plan than the library caches, in an
order in which every eviction takes a plan that holds an operator table in global memory.  It then frees the shortest
ragged chunk and creates it again (imc_obs_free drops the plans that use it, the 100-state one on all four chunks among
them), evaluates the 28-state plan on all four chunks once more so that such a plan is cached again, and calls
hmm.recompress on the ragged set (imc_obs_recompress drops that plan).  recompress returns early, before its plan
filter, when the chunks already share one dictionary trained on at least their columns; the dictionary registry is
therefore reset before the chunk is re-created: 4 099 columns train no dictionary of their own, the new chunk stays
uncompressed and the set is mixed when recompress sees it.  The same steps run once before the first cycle, so every
cycle starts from the same dictionaries and encodings, and the log-likelihoods of the last cycle must equal those of
the first bit for bit.

Free memory after cycles 2-4 may fall below the figure after cycle 1 by no more than ALLOWANCE, and every plan's
operator table must be at least ten times that, so that one leaked plan cannot hide in it.  The long chunk has
8 000 000 columns for that reason: at 200 000 columns the 28-state table is 2.1 MiB, at 1e6 / 2e6 columns the 20-state
table 14.1 / 18.8 MiB, from 4e6 on every table is above 20 MiB, and at 8e6 the 100-state plan takes the rank-one
hand-off and with it the packed table (measured: 4 096 tokens at 20 and 28 states, 7 213 at 48 and 100).  The 10-state
plan stays on the ragged set, where it runs the LDS-table scan and allocates no table (its global table could not
exceed 3 x 4097 x 100 x 8 bytes = 9.4 MiB).
"""
import json
import os
import re
import subprocess
import sys
import textwrap

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARAMETER_SETS = 3
# The largest drift of this script on the parent commit's library (whose release() calls, by reading, free everything
# on these paths) was PARENT_DRIFT bytes - after cycles 2-4 the figure was never below the one after cycle 1 (once 2 MiB
# above it, on either build): profiles/plan_ownership_ab.txt, which also has the test's wall time (3.6-3.7 s).
# Allowed: twice that plus one allocation granule of the device (GRANULE: hipMalloc of 16 bytes ... 1 MiB moves the
# free-memory figure by 2 MiB, larger requests by multiples of it; measured in the same session).
PARENT_DRIFT = 0
GRANULE = 2 << 20
ALLOWANCE = 2 * PARENT_DRIFT + GRANULE

SCRIPT = textwrap.dedent('''
    import json, os, sys
    import numpy as np
    sys.path.insert(0, %r)
    import torch
    from imcoalhmm_amd import Forwarder, _capi, synth, hmm
    from imcoalhmm_amd.hmm import forward_chunks_batch
    L = _capi.lib()
    B = %d
    gen = synth.random_hmm(6, 3, seed=11, stay=0.995)

    def chunk(m, seed):
        return Forwarder.from_array(synth.sample_alignment(*gen, m, seed=seed), 3)

    sets = {"one": [chunk(8_000_000, 0)], "ragged": [chunk(m, 200 + q) for q, m in enumerate((70_001, 0, 4_099))]}
    # (cached at the start of a cycle: 20 and 48 states on the long chunk.  28 and 100 are added, 10 evicts 20, 20 evicts
    # 48, 48 evicts 28; the freed chunk then takes 100 and 10 with it, and recompress the 28-state plan of churn().)
    PLANS = ((28, "all"), (100, "all"), (10, "ragged"), (20, "one"), (48, "one"))
    params = {}
    for n, _ in PLANS:
        hmms = [synth.random_hmm(n, 3, seed=1000 + 10 * n + q, stay=0.995) for q in range(B)]
        params[n] = [np.stack([h[k] for h in hmms]) for k in range(3)]

    def evaluate(n, name):
        chunks = sets["one"] + sets["ragged"] if name == "all" else sets[name]
        v = forward_chunks_batch([f.handle for f in chunks], *params[n], per_chunk=True)
        plan = _capi.last_plan()
        return [float(x).hex() for x in v.ravel()], plan["kernels"], plan["token_alphabet"]

    def churn():
        _capi.check(L.imc_dictionary_reset())
        sets["ragged"][2].close()                                  # imc_obs_free: every cached plan that uses the chunk goes
        sets["ragged"][2] = chunk(4_099, 202)                      # (too short to train a dictionary: uncompressed)
        evaluate(28, "all")                                        # a plan that uses the set is cached again ...
        hmm.recompress(sets["ragged"])                             # ... and imc_obs_recompress drops it

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    free_bytes()                                                   # (torch's own context exists from here on)
    churn()
    report = {"free": [], "values": [], "plans": []}
    for cycle in range(4):
        got = [evaluate(n, name) for n, name in PLANS]
        report["values"].append([g[0] for g in got])
        churn()
        report["free"].append(free_bytes())
        if cycle == 0:
            report["plans"] = [[n, name, g[1], g[2]] for (n, name), g in zip(PLANS, got)]
    print("REPORT " + json.dumps(report), flush=True)
''') % (REPO, PARAMETER_SETS)


def test_free_memory_does_not_drift_over_plan_churn(tmp_path):
    script = tmp_path / "plan_churn.py"
    script.write_text(SCRIPT)
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    report = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("REPORT ")][-1][7:])
    free = report["free"]
    drift = [free[0] - f for f in free[1:]]
    # what the cycle is meant to cover: the LDS-table scan, the global-table scan, the wide scan, the GEMM chain without
    # and (rank-one hand-off) with a packed table - so that a planner change cannot quietly shrink the test
    expected = {10: ("k_zpropagate3<3>",), 20: ("k_zpropagate4<5,",), 28: ("k_zpropagate4<7,",), 48: ("k_big_propagate<3>",),
                100: ("k_big_propagate", "rank1-handoff")}
    # the smallest operator table in global memory a plan of the cycle allocates (the global-table scan and the chains;
    # the LDS-table scan allocates none; of a plan on all four chunks, the table of its largest alphabet): parameter
    # sets x (alphabet + 1) entries x table doubles, the padded order squared - 4 x NT for k_zpropagate4<NT,...> (its
    # entries carry a few doubles of bank padding on top, not counted), 16 x NT for k_big_propagate<NT>
    tables = []
    for n, _, kernels, alphabet in report["plans"]:
        scan, chain = re.match(r"k_zpropagate4<(\d+)", kernels), re.match(r"k_big_propagate(?:_s)?<(\d+)>", kernels)
        if scan or chain:
            order = 4 * int(scan.group(1)) if scan else 16 * int(chain.group(1))
            assert order >= n
            tables.append(PARAMETER_SETS * (alphabet + 1) * order * order * 8)
    print("plans:", report["plans"])
    print("free bytes after cycles 1-4:", free, "drift below cycle 1:", drift, "allowance:", ALLOWANCE,
          "smallest operator table:", min(tables) if tables else None)
    for n, _, kernels, _ in report["plans"]:
        assert all(part in kernels for part in expected[n]), (n, kernels)
    assert len(tables) == 4, report["plans"]
    assert report["values"][3] == report["values"][0]
    assert tables and min(tables) >= 10 * ALLOWANCE, (tables, ALLOWANCE)      # one leaked plan cannot hide in the allowance
    assert max(drift) <= ALLOWANCE, (free, drift, ALLOWANCE)
