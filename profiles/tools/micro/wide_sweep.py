"""Time per evaluation at 24, 28 and 32 states with the blocked scan off / on / automatic (imc_set_wide_blocked), for the
shapes the records use: 30 x 1e6 columns with one and with 16 parameter sets, one 1e7-column chunk, 100 x 1e5 columns.

    python profiles/tools/micro/wide_sweep.py TAG [--steps K] [--states 24,28,32] [--data FILE.npy]

One process per library build: IMCOAL_FWD_LIB selects another build (a parent build has no switch and is timed as it
is, reported as mode "-").  Run the builds alternately, several rounds each; one line per (states, shape, mode) and
round: median and minimum of K evaluations in microseconds (host wall time around the synchronous call), the kernels.
Data: coalescent columns sampled from the 20-state isolation fixture (as bench.py does), the same symbols for every
state count; the HMMs come from the host-side model layer, 16 log-normal proposals around the fixture's theta."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("tag")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--states", default="24,28,32")
    ap.add_argument("--data", default="")
    ap.add_argument("--shapes", default="30x1e6,30x1e6x16,1x1e7,100x1e5")
    args = ap.parse_args()
    from imcoalhmm_amd import _capi, models, synth
    d = np.load(os.path.join(REPO, "tests", "golden", "hmm_params.npz"))
    if args.data and os.path.exists(args.data):
        cols = np.load(args.data)
    else:
        cols = np.concatenate([synth.sample_alignment(d["iso20_t0_pi"], d["iso20_t0_T"], d["iso20_t0_E"], 1_000_000, seed=20240100 + k)
                               for k in range(30)])
        if args.data:
            np.save(args.data, cols)
    has_switch = hasattr(ctypes.CDLL(_capi.LIB_PATH), "imc_set_wide_blocked")
    if not has_switch:
        _capi.SIGNATURES = [s for s in _capi.SIGNATURES if s[0] != "imc_set_wide_blocked"]
    from imcoalhmm_amd import Forwarder
    from imcoalhmm_amd.hmm import forward_chunks_batch
    L = _capi.lib()
    _capi.check(L.imc_set_compression(1))
    shapes = {}
    for name in args.shapes.split(","):
        parts = name.split("x")
        n_chunks, length, B = int(parts[0]), int(float(parts[1])), int(parts[2]) if len(parts) > 2 else 1
        _capi.check(L.imc_dictionary_reset())                   # every shape trains its dictionary on its own first chunk
        shapes[name] = ([Forwarder.from_array(cols[k * length:(k + 1) * length], 3) for k in range(n_chunks)], B)
    theta0 = d["iso20_t0_theta"]
    thetas = theta0 * np.exp(0.1 * np.random.default_rng(20240500).standard_normal((16, len(theta0))))
    thetas[0] = theta0
    for n in [int(x) for x in args.states.split(",")]:
        pis, Ts, Es = models.IsolationModel(n).build_batch(thetas)
        for name, (fw, B) in shapes.items():
            handles = [f.handle for f in fw]
            for mode in ((0, 1, -1) if has_switch else (None,)):
                if mode is not None:
                    _capi.set_wide_blocked(mode)
                for _ in range(3):
                    forward_chunks_batch(handles, pis[:B], Ts[:B], Es[:B])
                ts = []
                for _ in range(args.steps):
                    t0 = time.perf_counter()
                    v = forward_chunks_batch(handles, pis[:B], Ts[:B], Es[:B])
                    ts.append(time.perf_counter() - t0)
                plan = _capi.last_plan()
                print("%s states %d shape %s mode %s: median %.1f us min %.1f us  value %.17g  seg %d alphabet %d  %s" % (
                    args.tag, n, name, "-" if mode is None else mode, np.median(ts) * 1e6, min(ts) * 1e6, float(v[0]),
                    plan["token_segment_len"], plan["token_alphabet"], plan["kernels"]), flush=True)
        if has_switch:
            _capi.set_wide_blocked(-1)


if __name__ == "__main__":
    main()
