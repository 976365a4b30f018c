"""Set-up time with the host trainer against the device trainer (imc_set_device_training, csrc/kernels_train.hpp), and
against a build of the parent commit.

    python profiles/tools/device_training_ab.py --parent-tree DIR [--runs 5] [--out profiles/device_training_ab.txt]

(DIR: a checkout of the parent commit with its library built, `python -m imcoalhmm_amd.build` there; the parent leg
imports the package from it, so the parent's Python and the parent's library run together)

Workloads, generator, seeds and method are those of device_encode_ab.py (one1e8: create 1 x 1e8 columns; c32: create
32 x 1e7 columns, then recompress; a100: create 100 x 1e6 columns, then recompress; every measurement one fresh child
process under its own `timeout`, legs interleaved, the device context created untimed, median [min .. max]).
Legs: parent (the parent commit's package and library; parent1, with --parent-device: the same with its device trainer,
for a parent that has one; the summary then ends with switch1 against parent1 per workload), switch0 (this tree, imc_set_device_training(0): the default),
switch1 (this tree, imc_set_device_training(1)); all three with imc_set_device_encoding(1) and imc_set_device_ingest(1),
so that what differs between switch0 and switch1 is the trainer alone.  Compared across legs and runs: the dictionary
(alphabet, crc32 of its left / right lists), the token total and the crc32 of the first and last chunk's deepest stream.
The phase split is the library's own IMC_DEBUG_HOST=1 report; "train" is the phase the device trainer replaces.  A child
that fails ends the whole run."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from device_encode_ab import WORKLOADS, phases  # noqa: E402

LEGS = ("parent", "switch0", "switch1")


def child(workload, leg, data_dir, tree):
    sys.path.insert(0, tree)
    from imcoalhmm_amd import Forwarder, _capi
    from imcoalhmm_amd.hmm import recompress
    spec = WORKLOADS[workload]
    arrays = [np.load(os.path.join(data_dir, tag + ".npy")) for tag, _, _, _ in spec["requests"]]
    lib = _capi.lib()
    _capi.check(lib.imc_set_device(0))                         # context creation, untimed
    _capi.check(lib.imc_set_device_encoding(1))
    _capi.check(lib.imc_set_device_ingest(1))
    if leg != "parent":
        _capi.check(lib.imc_set_device_training(1 if leg.endswith("1") else 0))
    t0 = time.perf_counter()
    fw = [Forwarder.from_array(a, 3) for a in arrays]
    t1 = time.perf_counter()
    if spec["recompress"]:
        recompress(fw)
    t2 = time.perf_counter()
    tokens = sum(f.compressed_length(16384)[0] for f in fw)
    crc = 0
    for f in (fw[0], fw[-1]):
        crc = zlib.crc32(f.new_obs.astype(np.uint16).tobytes(), crc)
    pairs = fw[0].sym2pair
    dict_crc = zlib.crc32(np.array([pairs[z] for z in sorted(pairs)], dtype=np.uint16).tobytes())
    how = _capi.last_training() if leg != "parent" else {"path": 0}
    print("RESULT " + json.dumps({"create_s": t1 - t0, "recompress_s": t2 - t1, "alphabet": fw[0].compressed_length(16384)[1],
                                  "tokens": tokens, "crc32_first_last": crc, "crc32_dictionary": dict_crc, "trainer": how["path"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree")
    ap.add_argument("--parent-device", action="store_true", help="also run the parent with its device trainer (leg parent1)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "device_training_ab.txt"))
    ap.add_argument("--workloads", default="one1e8,c32,a100")
    ap.add_argument("--child", nargs=4, metavar=("WORKLOAD", "LEG", "DATA_DIR", "TREE"))
    args = ap.parse_args()
    if args.child:
        return child(*args.child)
    if not args.parent_tree or not os.path.exists(os.path.join(args.parent_tree, "imcoalhmm_amd", "libimcoal_fwd.so")):
        ap.error("--parent-tree: a checkout of the parent commit with imcoalhmm_amd/libimcoal_fwd.so built")
    sys.path.insert(0, REPO)
    import bench
    names = [w for w in args.workloads.split(",") if w]
    legs = ("parent", "parent1", "switch0", "switch1") if args.parent_device else LEGS
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("# device_training_ab: %d runs per leg, every run a fresh child process, legs interleaved; seconds, median [min .. max]" % args.runs)
    say("# parent = the parent commit's package and library; switch0 / switch1 = this tree with imc_set_device_training(0 / 1); "
        "device encoding and device ingest on in all legs")
    results = {}
    with tempfile.TemporaryDirectory() as data_dir:
        t0 = time.time()
        for w in names:
            for tag, a in bench.generate(WORKLOADS[w]["requests"]).items():
                np.save(os.path.join(data_dir, tag + ".npy"), a)
        say("# data generated in %.0f s (bench.py's generator and seeds)" % (time.time() - t0))
        for run in range(args.runs):
            for w in names:
                for leg in legs:
                    env = dict(os.environ, IMC_DEBUG_HOST="1")
                    for name in ("IMC_DEVICE_ENCODE", "IMC_DEVICE_INGEST", "IMC_DEVICE_TRAIN", "IMCOAL_FWD_LIB"):
                        env.pop(name, None)
                    tree = os.path.abspath(args.parent_tree) if leg.startswith("parent") else REPO
                    cmd = ["timeout", "-k", "10", str(WORKLOADS[w]["limit"]), sys.executable, os.path.abspath(__file__), "--child", w, leg, data_dir, tree]
                    out = subprocess.run(cmd, capture_output=True, text=True, env=env)
                    res = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
                    if out.returncode != 0 or not res:
                        say("# FAILED: %s %s run %d, exit status %d; nothing more is started\n%s" % (w, leg, run, out.returncode, out.stderr[-3000:]))
                        return 1
                    r = json.loads(res[0][7:])
                    r["phases"] = phases(out.stderr)
                    if r["trainer"] != (1 if leg.endswith("1") else 0):
                        say("# FAILED: %s %s run %d trained on path %d" % (w, leg, run, r["trainer"]))
                        return 1
                    results.setdefault((w, leg), []).append(r)
                    say("run %d  %-7s %-8s create %8.3f s  recompress %7.3f s  alphabet %5d  tokens %9d  crc %08x  dictionary %08x" % (
                        run, w, leg, r["create_s"], r["recompress_s"], r["alphabet"], r["tokens"], r["crc32_first_last"], r["crc32_dictionary"]))

    def stat(values):
        return "%8.3f [%7.3f .. %7.3f]" % (float(np.median(values)), min(values), max(values))

    say("#\n# summary (seconds)")
    for w in names:
        same = {(r["alphabet"], r["tokens"], r["crc32_first_last"], r["crc32_dictionary"]) for leg in legs for r in results[(w, leg)]}
        say("# %s: dictionaries and token streams of all legs and runs %s" % (
            w, "IDENTICAL (alphabet, crc32 of the dictionary, token total, crc32 of the first and last chunk's deepest stream)"
            if len(same) == 1 else "DIFFER: %r" % sorted(same)))
        for leg in legs:
            rs = results[(w, leg)]
            say("%-7s %-8s create %s   recompress %s   total %s" % (
                w, leg, stat([r["create_s"] for r in rs]), stat([r["recompress_s"] for r in rs]), stat([r["create_s"] + r["recompress_s"] for r in rs])))
            keys = sorted({k for r in rs for k in r["phases"]})
            if keys:
                say("#        %-8s phases, ms, median over runs (summed over the chunks of a run): %s" % (
                    leg, "; ".join("%s %.0f" % (k, float(np.median([r["phases"].get(k, 0.0) for r in rs]))) for k in keys)))
    say("#\n# switch0 against the parent, total seconds: difference of medians | spread (max - min) of the parent's own runs")
    for w in names:
        tot = {leg: [r["create_s"] + r["recompress_s"] for r in results[(w, leg)]] for leg in ("switch0", "parent")}
        diff, spread = float(np.median(tot["switch0"]) - np.median(tot["parent"])), max(tot["parent"]) - min(tot["parent"])
        say("%-7s switch0 - parent %+8.3f | %7.3f   %s" % (w, diff, spread, "inside" if abs(diff) <= spread else "OUTSIDE"))
    if args.parent_device:
        say("#\n# this tree against the parent, device path in both, total seconds: difference of medians | spread (max - min) of the parent's own runs")
        for w in names:
            tot = {leg: [r["create_s"] + r["recompress_s"] for r in results[(w, leg)]] for leg in ("switch1", "parent1")}
            diff, spread = float(np.median(tot["switch1"]) - np.median(tot["parent1"])), max(tot["parent1"]) - min(tot["parent1"])
            say("%-7s switch1 - parent1 %+8.3f | %7.3f   %s" % (w, diff, spread, "inside" if diff <= spread else "OUTSIDE"))
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
