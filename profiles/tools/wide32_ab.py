"""A/B leg for 32 states (the wide blocked scan, four-wavefront workgroups).  bench.py has no (pi, T, E) fixture between 20
and 150 states, so: synth.random_hmm(32, 3, seed=1320, stay=0.995) on one 1e8-column chunk, 20 warm-up and 300 timed
forward_chunks_batch calls, one JSON line (wall time per evaluation, log-likelihood, kernel names; no per-kernel time).
IMCOAL_FWD_LIB selects the library, one fresh process per run.

    python profiles/tools/wide32_ab.py
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from imcoalhmm_amd import Forwarder, _capi, synth                     # noqa: E402
from imcoalhmm_amd.hmm import forward_chunks_batch                    # noqa: E402

gen = synth.random_hmm(6, 3, seed=11, stay=0.995)
f = Forwarder.from_array(synth.sample_alignment(*gen, 100_000_000, seed=5), 3)
h = synth.random_hmm(32, 3, seed=1320, stay=0.995)
params = [np.stack([h[k]]) for k in range(3)]
for _ in range(20):
    v = forward_chunks_batch([f.handle], *params, per_chunk=True)
t0 = time.perf_counter()
for _ in range(300):
    v = forward_chunks_batch([f.handle], *params, per_chunk=True)
dt = time.perf_counter() - t0
print(json.dumps({"ms_per_step": dt / 300 * 1e3, "loglik": float(v.ravel()[0]), "kernel": _capi.last_plan()["kernels"]}), flush=True)
