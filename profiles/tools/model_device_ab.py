"""A/B of the model layer's device route (models.set_device_transitions, csrc/kernels_model.hpp) against the numpy path
the parent takes for every model with a migration epoch.  Both legs in this one process and run, interleaved; an untimed
warm-up of each leg first; the median of the repeated steps is reported with the spread.

    python profiles/tools/model_device_ab.py [--reps 9] [--columns 1000000] [--chunks 32] > profiles/model_device_ab.txt

Per model: build_batch(64) off / on, and one whole Likelihood.batch(64) step (build + device pass) off / on."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from imcoalhmm_amd import Forwarder, Likelihood, _capi, synth  # noqa: E402
from imcoalhmm_amd import models as M  # noqa: E402

IM_THETA = np.array([0.001, 0.001, 1000.0, 0.4, 200.0])
MODELS = [
    ("IM(10,10)", lambda: M.IsolationMigrationModel(10, 10), IM_THETA),
    ("IM(75,75)", lambda: M.IsolationMigrationModel(75, 75), IM_THETA),
    # (isolation time, migration time, recombination rate, 5 coalescence rates, 2 migration rates)
    ("IMEpochs(2,10,10)", lambda: M.IsolationMigrationEpochsModel(2, 10, 10),
     np.array([0.001, 0.001, 0.4, 1000.0, 900.0, 1100.0, 1000.0, 950.0, 200.0, 150.0])),
]


def timed(fn, reps, switch):
    """Median, min, max of ``reps`` timed calls of fn under each setting of the switch, interleaved off / on."""
    times = {False: [], True: []}
    for on in (False, True):                       # untimed warm-up of each leg
        M.set_device_transitions(on)
        fn()
    for _ in range(reps):
        for on in switch:
            M.set_device_transitions(on)
            t0 = time.perf_counter()
            fn()
            times[on].append(time.perf_counter() - t0)
    M.set_device_transitions(False)
    return {on: (np.median(v) * 1e3, min(v) * 1e3, max(v) * 1e3) for on, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--population", type=int, default=64)
    ap.add_argument("--columns", type=int, default=1_000_000)
    ap.add_argument("--chunks", type=int, default=32)
    ap.add_argument("--skip-likelihood", action="store_true")
    args = ap.parse_args()
    lib = _capi.lib()
    assert lib.imc_device_count() >= 1, "needs a GPU"
    print("# model_device_ab: population %d, %d reps (median [min .. max], ms), %d chunks x %d columns" % (
        args.population, args.reps, args.chunks, args.columns))
    print("# off = numpy path (the parent's), on = imc_model_transitions_device; both legs in one process, interleaved")
    for name, make, theta in MODELS:
        model = make()
        thetas = [theta * (1.0 + 0.002 * k) for k in range(args.population)]
        calls = M._native["device_calls"]
        res = timed(lambda: model.build_batch(thetas), args.reps, (False, True))
        routed = M._native["device_calls"] - calls
        off, on = res[False], res[True]
        M.set_device_transitions(False)
        a = model.build_batch(thetas)
        M.set_device_transitions(True)
        b = model.build_batch(thetas)
        M.set_device_transitions(False)
        print("%-18s N=%3d build_batch     off %8.2f [%8.2f .. %8.2f]   on %8.2f [%8.2f .. %8.2f]   off/on %5.2fx   routed calls %d   max|dT| %.1e"
              % (name, a[0].shape[1], off[0], off[1], off[2], on[0], on[1], on[2], off[0] / on[0], routed, np.abs(a[1] - b[1]).max()), flush=True)
        if args.skip_likelihood:
            continue
        pi, T, E = model.build_hidden_markov_model(theta)
        chunks = [Forwarder.from_array(synth.sample_alignment(pi, T, E, args.columns, seed=100 + k), 3) for k in range(args.chunks)]
        lik = Likelihood(model, chunks)
        res = timed(lambda: lik.batch(thetas), args.reps, (False, True))
        off, on = res[False], res[True]
        print("%-18s N=%3d Likelihood.batch off %8.2f [%8.2f .. %8.2f]   on %8.2f [%8.2f .. %8.2f]   off/on %5.2fx"
              % (name, a[0].shape[1], off[0], off[1], off[2], on[0], on[1], on[2], off[0] / on[0]), flush=True)
        del lik, chunks


if __name__ == "__main__":
    main()
