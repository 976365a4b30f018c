"""Set-up time with the host encoder against the device encoder (imc_set_device_encoding, csrc/kernels_encode.hpp), and
against a build of the parent commit.

    python profiles/tools/device_encode_ab.py --parent-tree DIR [--runs 5] [--out profiles/device_encode_ab.txt]

(DIR: a checkout of the parent commit with its library built, `python -m imcoalhmm_amd.build` there; the parent leg
imports the package from it, so the parent's Python and the parent's library run together)

Workloads (3 symbols, bench.py's generator and seeds):
    one1e8   create 1 x 1e8 columns                         (bench.py's default workload)
    c32      create 32 x 1e7 columns, then recompress       (the per-GPU slice of BASELINE config[3])
    a100     create 100 x 1e6 columns, then recompress      (the reference authors' data scale)
Legs: parent (the parent commit's package and library, its default encoder: the host's), parent1 (the same with its device
encoder; --parent-device, for a parent that has one), switch0 (this tree, host encoder: the default), switch1 (this tree,
device encoder).  Every measurement is one fresh child process under its own `timeout`; the legs are interleaved (parent,
switch0, switch1, parent, ...); the data is generated once by this driver, which never touches the GPU, and handed over
as .npy files.  A child creates the device context with an untimed imc_set_device(0) first, so the figures are the
chunk work alone (bench.py's setup_s also holds the context creation).  Reported: median [min .. max] over the runs.
The phase split is the library's own IMC_DEBUG_HOST=1 report.  With --parent-device the summary ends with this tree
against the parent per workload and encoder: the difference of the medians beside the min .. max spread of the parent's
own runs.  A child that fails ends the whole run."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = {
    "one1e8": dict(requests=[("one1e8_0", "iso20_t0", 100_000_000, 20240001)], recompress=False, limit=240),
    "c32": dict(requests=[("c32_%d" % i, "iso20_t0", 10_000_000, 20240100 + i) for i in range(32)], recompress=True, limit=300),
    "a100": dict(requests=[("a100_%d" % i, "iso10_t0", 1_000_000, 20240800 + i) for i in range(100)], recompress=True, limit=240),
}
LEGS = ("parent", "switch0", "switch1")


def child(workload, leg, data_dir, tree):
    sys.path.insert(0, tree)
    from imcoalhmm_amd import Forwarder, _capi
    from imcoalhmm_amd.hmm import recompress
    spec = WORKLOADS[workload]
    arrays = [np.load(os.path.join(data_dir, tag + ".npy")) for tag, _, _, _ in spec["requests"]]
    lib = _capi.lib()
    _capi.check(lib.imc_set_device(0))                         # context creation, untimed
    if leg != "parent":
        _capi.check(lib.imc_set_device_encoding(1 if leg.endswith("1") else 0))
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
    print("RESULT " + json.dumps({"create_s": t1 - t0, "recompress_s": t2 - t1, "alphabet": fw[0].compressed_length(16384)[1],
                                  "tokens": tokens, "crc32_first_last": crc}), flush=True)


def phases(stderr):
    """Sums of the library's '[imc host]' lines: milliseconds per phase of creation and of recompress."""
    out = {}
    for line in stderr.splitlines():
        if not line.startswith("[imc host] "):
            continue
        what = "recompress" if "recompress" in line else "create"
        for part in line.split(":", 1)[1].split(","):
            words = part.split()
            if "ms" in words[2:]:
                i = words.index("ms", 2)
                key = what + " " + " ".join(words[:i - 1])
                out[key] = out.get(key, 0.0) + float(words[i - 1])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree")
    ap.add_argument("--parent-device", action="store_true", help="also run the parent with its device encoder (leg parent1)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "device_encode_ab.txt"))
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

    say("# device_encode_ab: %d runs per leg, every run a fresh child process, legs interleaved; seconds, median [min .. max]" % args.runs)
    say("# parent = the parent commit's package and library; switch0 / switch1 = this tree with imc_set_device_encoding(0 / 1)")
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
                    env.pop("IMC_DEVICE_ENCODE", None)
                    env.pop("IMCOAL_FWD_LIB", None)
                    tree = os.path.abspath(args.parent_tree) if leg.startswith("parent") else REPO
                    cmd = ["timeout", "-k", "10", str(WORKLOADS[w]["limit"]), sys.executable, os.path.abspath(__file__), "--child", w, leg, data_dir, tree]
                    out = subprocess.run(cmd, capture_output=True, text=True, env=env)
                    res = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
                    if out.returncode != 0 or not res:
                        say("# FAILED: %s %s run %d, exit status %d; nothing more is started\n%s" % (w, leg, run, out.returncode, out.stderr[-3000:]))
                        return 1
                    r = json.loads(res[0][7:])
                    r["phases"] = phases(out.stderr)
                    results.setdefault((w, leg), []).append(r)
                    say("run %d  %-7s %-8s create %8.3f s  recompress %7.3f s  alphabet %5d  tokens %9d  crc %08x" % (
                        run, w, leg, r["create_s"], r["recompress_s"], r["alphabet"], r["tokens"], r["crc32_first_last"]))

    def stat(values):
        return "%8.3f [%7.3f .. %7.3f]" % (float(np.median(values)), min(values), max(values))

    say("#\n# summary (seconds)")
    for w in names:
        same = {(r["alphabet"], r["tokens"], r["crc32_first_last"]) for leg in legs for r in results[(w, leg)]}
        say("# %s: token streams of all legs and runs %s" % (w, "IDENTICAL (alphabet, token total, crc32 of the first and last chunk's deepest stream)"
                                                              if len(same) == 1 else "DIFFER: %r" % sorted(same)))
        for leg in legs:
            rs = results[(w, leg)]
            say("%-7s %-8s create %s   recompress %s   total %s" % (
                w, leg, stat([r["create_s"] for r in rs]), stat([r["recompress_s"] for r in rs]), stat([r["create_s"] + r["recompress_s"] for r in rs])))
            keys = sorted({k for r in rs for k in r["phases"]})
            if keys:
                say("#        %-8s phases, ms, median over runs (summed over the chunks of a run): %s" % (
                    leg, "; ".join("%s %.0f" % (k, float(np.median([r["phases"].get(k, 0.0) for r in rs]))) for k in keys)))
    if args.parent_device:
        say("#\n# this tree against the parent, total seconds: difference of medians | spread (max - min) of the parent's own runs")
        for w in names:
            for mine, theirs in (("switch0", "parent"), ("switch1", "parent1")):
                tot = {leg: [r["create_s"] + r["recompress_s"] for r in results[(w, leg)]] for leg in (mine, theirs)}
                diff, spread = float(np.median(tot[mine]) - np.median(tot[theirs])), max(tot[theirs]) - min(tot[theirs])
                say("%-7s %-8s - %-8s %+8.3f | %7.3f   %s" % (w, mine, theirs, diff, spread, "inside" if abs(diff) <= spread else "OUTSIDE"))
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
