"""Creation time with the host parser against device ingestion (imc_set_device_ingest, csrc/kernels_ingest.hpp), and
against a build of the parent commit.

    python profiles/tools/device_ingest_ab.py --parent-tree DIR [--runs 5] [--out profiles/device_ingest_ab.txt]

(DIR: a checkout of the parent commit with its library built, `python -m imcoalhmm_amd.build` there; the parent leg
imports the package from it, so the parent's Python and the parent's library run together)

Workloads (3 symbols, bench.py's generator and seeds):
    text1e8   Forwarder(path, 3) on a text file of 1e8 columns (200 MB: BASELINE config[1])
    cache1e8  the same on its 2-bit cache (25 MB)
    a100      Forwarder(path, 3) on 100 text files of 1e6 columns, then recompress
    pair1e8   two aligned sequences of 1e8 bases -> chunk: prepare.encode_pairwise + Forwarder.from_array against
              Forwarder.from_sequences (the parent and switch0 legs run the first, switch1 the second)
    sweep     text1e8 with the switch on at IMC_INGEST_SLAB_BYTES = 1, 4, 16, 64 and 256 MiB (--sweep-runs per size)
Legs: parent (the parent commit's package and library; parent1, with --parent-device: the same with its device ingestion,
for a parent that has one; the summary then ends with switch1 against parent1 per workload: the difference of the medians
beside the min .. max spread of the parent's own runs), switch0 (this tree, imc_set_device_ingest(0)), switch1 (this
tree, imc_set_device_ingest(1)); all three with imc_set_device_encoding(1), so that what differs between switch0 and
switch1 is where the file becomes symbols.  Every measurement is one fresh child process under its own `timeout`; the legs
are interleaved (parent, switch0, switch1, parent, ...).  The files are written once by this driver, which never touches
the GPU, and read once before the first child, so every child finds them in the page cache.  A child creates the device
context with an untimed imc_set_device(0) first.  Reported: median [min .. max] over the runs, and per run the token
total and a crc32 of the first and last chunk's deepest stream: all legs must agree.  A child that fails ends the run."""
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
LEGS = ("parent", "switch0", "switch1")
SWEEP_MIB = (1, 4, 16, 64, 256)
WORKLOADS = {
    "text1e8": dict(requests=[("one1e8_0", "iso20_t0", 100_000_000, 20240001)], recompress=False, limit=240),
    "cache1e8": dict(requests=[("one1e8_0", "iso20_t0", 100_000_000, 20240001)], recompress=False, limit=240),
    "a100": dict(requests=[("a100_%d" % i, "iso10_t0", 1_000_000, 20240800 + i) for i in range(100)], recompress=True, limit=240),
    "pair1e8": dict(requests=[("one1e8_0", "iso20_t0", 100_000_000, 20240001)], recompress=False, limit=240),
}


def write_text(path, obs):
    """prepare.write_text's bytes for symbols below 10 ("%d " per column), written with two strided stores."""
    out = np.empty(2 * obs.size, dtype=np.uint8)
    out[0::2] = obs + ord("0")
    out[1::2] = ord(" ")
    out.tofile(path)


def sequences_for(obs, seed):
    """Two aligned sequences whose pairwise symbols are obs: equal bases, a substitution where obs is 1, an N where it is 2."""
    rng = np.random.default_rng(seed)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    k = rng.integers(0, 4, size=obs.size, dtype=np.uint8)
    s1 = bases[k]
    s2 = bases[(k + (obs == 1)) & 3]
    s2[obs == 2] = ord("N")
    return s1, s2


def child(workload, leg, data_dir, tree):
    sys.path.insert(0, tree)
    from imcoalhmm_amd import Forwarder, _capi, prepare
    from imcoalhmm_amd.hmm import recompress
    spec = WORKLOADS[workload]
    lib = _capi.lib()
    _capi.check(lib.imc_set_device(0))                         # context creation, untimed
    _capi.check(lib.imc_set_device_encoding(1))
    if leg != "parent":
        _capi.check(lib.imc_set_device_ingest(1 if leg.endswith("1") else 0))
    ext = ".imc" if workload == "cache1e8" else ".ziphmm"
    if workload == "pair1e8":
        s1, s2 = (open(os.path.join(data_dir, "pair_%d.seq" % k), "rb").read() for k in (1, 2))
        t0 = time.perf_counter()
        if leg.endswith("1"):
            fw = [Forwarder.from_sequences(s1, s2)]
        else:
            obs = np.empty(len(s1), dtype=np.uint8)
            _capi.check(lib.imc_encode_pairwise(s1, s2, len(s1), obs.ctypes.data_as(_capi._u8p)))
            fw = [Forwarder.from_array(obs, 3)]
    else:
        paths = [os.path.join(data_dir, tag + ext) for tag, _, _, _ in spec["requests"]]
        t0 = time.perf_counter()
        fw = [Forwarder(p, 3) for p in paths]
    t1 = time.perf_counter()
    how = _capi.last_ingest() if leg != "parent" else {"path": "host", "slabs": 0}
    if spec["recompress"]:
        recompress(fw)
    t2 = time.perf_counter()
    tokens = sum(f.compressed_length(16384)[0] for f in fw)
    crc = 0
    for f in (fw[0], fw[-1]):
        crc = zlib.crc32(f.new_obs.astype(np.uint16).tobytes(), crc)
    print("RESULT " + json.dumps({"create_s": t1 - t0, "recompress_s": t2 - t1, "alphabet": fw[0].compressed_length(16384)[1], "tokens": tokens,
                                  "crc32_first_last": crc, "path": how["path"], "slabs": how["slabs"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree")
    ap.add_argument("--parent-device", action="store_true", help="also run the parent with its device ingestion (leg parent1)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sweep-runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "device_ingest_ab.txt"))
    ap.add_argument("--workloads", default="text1e8,cache1e8,a100,pair1e8")
    ap.add_argument("--child", nargs=4, metavar=("WORKLOAD", "LEG", "DATA_DIR", "TREE"))
    args = ap.parse_args()
    if args.child:
        return child(*args.child)
    if not args.parent_tree or not os.path.exists(os.path.join(args.parent_tree, "imcoalhmm_amd", "libimcoal_fwd.so")):
        ap.error("--parent-tree: a checkout of the parent commit with imcoalhmm_amd/libimcoal_fwd.so built")
    sys.path.insert(0, REPO)
    import bench
    from imcoalhmm_amd import prepare
    names = [w for w in args.workloads.split(",") if w]
    legs = ("parent", "parent1", "switch0", "switch1") if args.parent_device else LEGS
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def run_child(w, leg, data_dir, slab=None):
        env = dict(os.environ)
        for k in ("IMC_DEVICE_ENCODE", "IMC_DEVICE_INGEST", "IMCOAL_FWD_LIB", "IMC_INGEST_SLAB_BYTES"):
            env.pop(k, None)
        if slab:
            env["IMC_INGEST_SLAB_BYTES"] = str(slab)
        tree = os.path.abspath(args.parent_tree) if leg.startswith("parent") else REPO
        cmd = ["timeout", "-k", "10", str(WORKLOADS[w]["limit"]), sys.executable, os.path.abspath(__file__), "--child", w, leg, data_dir, tree]
        out = subprocess.run(cmd, capture_output=True, text=True, env=env)
        res = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
        if out.returncode != 0 or not res:
            say("# FAILED: %s %s, exit status %d; nothing more is started\n%s" % (w, leg, out.returncode, out.stderr[-3000:]))
            return None
        return json.loads(res[0][7:])

    def stat(values):
        return "%8.3f [%7.3f .. %7.3f]" % (float(np.median(values)), min(values), max(values))

    say("# device_ingest_ab: %d runs per leg, every run a fresh child process, legs interleaved; seconds, median [min .. max]" % args.runs)
    say("# parent = the parent commit's package and library; switch0 / switch1 = this tree with imc_set_device_ingest(0 / 1); device encoding on in all legs")
    results, sweep = {}, {}
    with tempfile.TemporaryDirectory() as data_dir:
        t0 = time.time()
        done = set()
        for w in names:
            for tag, a in bench.generate(WORKLOADS[w]["requests"]).items():
                if tag in done:
                    continue
                done.add(tag)
                a = np.ascontiguousarray(a, dtype=np.uint8)
                write_text(os.path.join(data_dir, tag + ".ziphmm"), a)
                if "cache1e8" in names and tag == "one1e8_0":
                    prepare.write_cache(os.path.join(data_dir, tag + ".imc"), a, 3)
                if "pair1e8" in names and tag == "one1e8_0":
                    for k, s in enumerate(sequences_for(a, 7), 1):
                        s.tofile(os.path.join(data_dir, "pair_%d.seq" % k))
        total = 0
        for name in sorted(os.listdir(data_dir)):                 # read once: the page cache holds every file
            with open(os.path.join(data_dir, name), "rb") as fh:
                while True:
                    block = fh.read(1 << 24)
                    if not block:
                        break
                    total += len(block)
        say("# files written and read back in %.0f s (bench.py's generator and seeds; %.0f MB)" % (time.time() - t0, total / 1e6))
        for run in range(args.runs):
            for w in names:
                for leg in legs:
                    r = run_child(w, leg, data_dir)
                    if r is None:
                        return 1
                    results.setdefault((w, leg), []).append(r)
                    say("run %d  %-8s %-8s create %8.3f s  recompress %7.3f s  path %-8s slabs %3d  alphabet %5d  tokens %9d  crc %08x" % (
                        run, w, leg, r["create_s"], r["recompress_s"], r["path"], r["slabs"], r["alphabet"], r["tokens"], r["crc32_first_last"]))
        if "text1e8" in names:
            for run in range(args.sweep_runs):
                for mib in SWEEP_MIB:
                    r = run_child("text1e8", "switch1", data_dir, slab=mib << 20)
                    if r is None:
                        return 1
                    sweep.setdefault(mib, []).append(r)
                    say("sweep run %d  slab %4d MiB  create %8.3f s  slabs %3d  crc %08x" % (run, mib, r["create_s"], r["slabs"], r["crc32_first_last"]))
    say("#\n# summary (seconds)")
    for w in names:
        same = {(r["alphabet"], r["tokens"], r["crc32_first_last"]) for leg in legs for r in results[(w, leg)]}
        say("# %s: token streams of all legs and runs %s" % (w, "IDENTICAL (alphabet, token total, crc32 of the first and last chunk's deepest stream)"
                                                              if len(same) == 1 else "DIFFER: %r" % sorted(same)))
        for leg in legs:
            rs = results[(w, leg)]
            say("%-8s %-8s create %s   recompress %s   total %s   (path %s)" % (
                w, leg, stat([r["create_s"] for r in rs]), stat([r["recompress_s"] for r in rs]), stat([r["create_s"] + r["recompress_s"] for r in rs]),
                rs[0]["path"]))
    if args.parent_device:
        say("#\n# this tree against the parent, device path in both, total seconds: difference of medians | spread (max - min) of the parent's own runs")
        for w in names:
            tot = {leg: [r["create_s"] + r["recompress_s"] for r in results[(w, leg)]] for leg in ("switch1", "parent1")}
            diff, spread = float(np.median(tot["switch1"]) - np.median(tot["parent1"])), max(tot["parent1"]) - min(tot["parent1"])
            say("%-8s switch1 - parent1 %+8.3f | %7.3f   %s" % (w, diff, spread, "inside" if diff <= spread else "OUTSIDE"))
    if sweep:
        say("#\n# slab size sweep, text1e8 with the switch on (seconds to create)")
        for mib in SWEEP_MIB:
            say("slab %4d MiB  create %s   slabs %d" % (mib, stat([r["create_s"] for r in sweep[mib]]), sweep[mib][0]["slabs"]))
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
