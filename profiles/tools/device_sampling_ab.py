"""profiles/device_sampling_ab.txt: the HMM sampler (imcoalhmm_amd/simulate.py, csrc/kernels_sample.hpp) on one MI355X.
Per configuration 60 ms of untimed calls (the device conditioning of bench.py), one warm-up call, then the median of 5:
the whole simulate.sample(where="device") call by the host clock and its three kernels by HIP events (the library's
IMC_DEBUG_HOST=1 lines); the tile-length sweep; tables in LDS against global memory (IMC_SAMPLE_LDS=0); the sequential
specification imc_sample_host; synth.sample_alignment, the generator of the bench harness.

    python profiles/tools/device_sampling_ab.py > profiles/device_sampling_ab.txt"""
import os
import re
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
os.environ["IMC_DEBUG_HOST"] = "1"          # the library prints its three kernels' HIP-event times to stderr
import torch
import numpy as np
from imcoalhmm_amd import simulate, synth, _capi

err = tempfile.TemporaryFile(mode="w+")
os.dup2(err.fileno(), 2)

d = np.load(os.path.join(REPO, "tests", "golden", "hmm_params.npz"))
iso20 = (d["iso20_t0_pi"], d["iso20_t0_T"], d["iso20_t0_E"])
big150 = synth.random_hmm(150, 3, seed=150, stay=0.98)
big128 = synth.random_hmm(128, 3, seed=128, stay=0.98)


def kernel_times(n):
    err.flush(); err.seek(0)
    rows = [[float(x) for x in m] for m in re.findall(r"summary ([0-9.]+) ms.*scan ([0-9.]+) ms, emit ([0-9.]+) ms", err.read())]
    err.seek(0); err.truncate()
    return np.median(np.array(rows[-n:]), axis=0)


def device(name, hmm, L, tile=None, lds=None, states=False):
    for key, v in (("IMC_SAMPLE_TILE", tile), ("IMC_SAMPLE_LDS", lds)):
        if v is None:
            os.environ.pop(key, None)
        else:
            os.environ[key] = str(v)
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < 60.0:
        simulate.sample(*hmm, L, 1, emit_symbols=2)
    simulate.sample(*hmm, L, 1, emit_symbols=2, return_states=states)
    wall = []
    for k in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = simulate.sample(*hmm, L, 1 + k, emit_symbols=2, return_states=states)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        del out
    s, c, e = kernel_times(5)
    print("%-46s L=%-10d whole call %9.3f ms | summary %9.3f  scan %8.3f  emit %8.3f ms" % (name, L, np.median(wall), s, c, e), flush=True)


print("device: simulate.sample(where=\"device\"), median of 5", flush=True)
device("20 states, default tile", iso20, 10_000_000)
device("20 states, default tile", iso20, 100_000_000)
device("20 states, default tile, with states", iso20, 100_000_000, states=True)
device("150 states, default tile (global table)", big150, 10_000_000)
device("128 states, default tile (LDS table)", big128, 10_000_000)
device("128 states, IMC_SAMPLE_LDS=0", big128, 10_000_000, lds=0)
device("20 states, IMC_SAMPLE_LDS=0", iso20, 100_000_000, lds=0)
for tile in (64, 128, 256, 512, 1024, 2048, 4096):
    device("20 states, tile %d" % tile, iso20, 100_000_000, tile=tile)
for tile in (128, 512, 2048):
    device("150 states, tile %d" % tile, big150, 10_000_000, tile=tile)
os.environ.pop("IMC_SAMPLE_TILE", None)

print("host: imc_sample_host", flush=True)
for hmm, n, L in ((iso20, 20, 10_000_000), (iso20, 20, 100_000_000), (big150, 150, 10_000_000)):
    times = []
    for k in range(5 if L <= 10_000_000 else 1):
        t0 = time.perf_counter()
        simulate.sample(*hmm, L, 1 + k, emit_symbols=2, where="host")
        times.append(time.perf_counter() - t0)
    print("%d states L=%d: %.3f s (median of %d)" % (n, L, np.median(times), len(times)), flush=True)

print("parent's generator: synth.sample_alignment", flush=True)
for hmm, n, L in ((iso20, 20, 10_000_000), (big150, 150, 10_000_000)):
    t0 = time.perf_counter()
    synth.sample_alignment(*hmm, L, seed=1)
    print("%d states L=%d: %.3f s (one run)" % (n, L, time.perf_counter() - t0), flush=True)
