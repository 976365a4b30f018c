"""Chunks of all pairs of an alignment file: prepare.pairwise_forwarders (a Python pass over the file, two uploads per
pair) at the parent commit against imcoalhmm_amd.Alignment (the file opened once on the device, csrc/kernels_align.hpp).

    python profiles/tools/device_alignment_ab.py --parent-tree DIR [--runs 5] [--sizes 10000000,100000000] [--out profiles/device_alignment_ab.txt]

(DIR: a checkout of the parent commit with its library built, `python -m imcoalhmm_amd.build` there; the parent leg
imports the package from it, so the parent's Python and the parent's library run together)

Input: 4 records x n bases wrapped at 60 (a random root sequence; record k differs from it in 0.4 (k + 1) % of the
columns, a few of them N or gaps), written once by this driver, which never touches the GPU, and read once before the first
child, so every child finds it in the page cache.
Legs, each one child process per size under its own `timeout`, with imc_set_device_encoding(1) and
imc_set_device_training(1), an untimed imc_set_device(0) first, then one warm-up round and --runs timed rounds:
    parent   the parent commit's package and library:  read_fasta(path);  (a) pairwise_forwarders(path), all six pairs
    branch   this tree:  the same two (pairwise_forwarders is unchanged: the leg shows the spread between two builds);
             (b) Alignment(path);  (c) Alignment(path).pairs();  pairs() of an open alignment;  (d) one triplet chunk of an
             open alignment
With --parent-device (a parent that has the device path) the two trees are compared on that path instead: legs parent1
and branch1, --runs fresh child processes each, interleaved, every child one round of (b) and of pairs() of the open
alignment; the summary ends with the difference of the medians beside the min .. max spread of the parent's own runs.
Reported: median [min .. max] over the timed rounds, and the crc32 of the six chunks' deepest token streams, which all legs
must agree on.  A child that fails ends the run."""
import argparse
import gc
import json
import os
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def write_alignment(path, n, seed):
    rng = np.random.default_rng(seed)
    root = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n)
    with open(path, "wb") as fh:
        for k in range(4):
            s = root.copy()
            flip = rng.random(n) < 0.004 * (k + 1)
            s[flip] = rng.choice(np.frombuffer(b"ACGTN-", dtype=np.uint8), size=int(flip.sum()))
            fh.write(b">species%d some description\n" % k)
            rows = n // 60
            block = np.full((rows, 61), 10, dtype=np.uint8)
            block[:, :60] = s[:rows * 60].reshape(rows, 60)
            block.tofile(fh)
            if n % 60:
                fh.write(bytes(s[rows * 60:]) + b"\n")


def child(leg, path, tree, runs):
    sys.path.insert(0, tree)
    from imcoalhmm_amd import _capi, prepare
    lib = _capi.lib()
    _capi.check(lib.imc_set_device(0))                         # context creation, untimed
    _capi.check(lib.imc_set_device_encoding(1))
    _capi.check(lib.imc_set_device_training(1))
    times, crcs, info = {}, None, {}

    def timed(name, fn, keep):
        gc.collect()
        t0 = time.perf_counter()
        out = fn()
        if keep:
            times.setdefault(name, []).append(time.perf_counter() - t0)
        return out

    def crc_of(fw):
        return ["%08x" % (zlib.crc32(fw[k].new_obs.astype(np.uint16).tobytes()) & 0xffffffff) for k in sorted(fw)]

    if leg.endswith("1"):                                      # --parent-device: one round of the device path alone
        from imcoalhmm_amd import Alignment
        aln = timed("b Alignment(path)", lambda: Alignment(path), True)
        fw = timed("  pairs() of an open alignment", aln.pairs, True)
        print("RESULT " + json.dumps({"times": times, "crcs": crc_of(fw), "info": aln.info}), flush=True)
        return
    for run in range(-1, runs):
        keep = run >= 0
        names = list(timed("read_fasta", lambda: prepare.read_fasta(path), keep))
        fw = timed("a pairwise_forwarders", lambda: prepare.pairwise_forwarders(path), keep)
        if run < 0:
            crcs = crc_of(fw)
        del fw
        if leg == "branch":
            from imcoalhmm_amd import Alignment
            aln = timed("b Alignment(path)", lambda: Alignment(path), keep)
            info = aln.info
            fw = timed("  pairs() of an open alignment", aln.pairs, keep)
            if run < 0:
                assert crc_of(fw) == crcs, "pairs() and pairwise_forwarders disagree"
            del fw
            trip = timed("d one triplet chunk of an open alignment", lambda: aln.forwarder(*names[:3]), keep)
            del trip
            aln.close()

            def open_and_pairs():
                with Alignment(path) as a:
                    return a.pairs()
            fw = timed("c Alignment(path).pairs()", open_and_pairs, keep)
            del fw
    print("RESULT " + json.dumps({"times": times, "crcs": crcs, "info": info}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree")
    ap.add_argument("--parent-device", action="store_true", help="compare the device path of the two trees (legs parent1, branch1)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sizes", default="10000000,100000000")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "device_alignment_ab.txt"))
    ap.add_argument("--child", nargs=4, metavar=("LEG", "PATH", "TREE", "RUNS"))
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], args.child[2], int(args.child[3]))
    if not args.parent_tree or not os.path.exists(os.path.join(args.parent_tree, "imcoalhmm_amd", "libimcoal_fwd.so")):
        ap.error("--parent-tree: a checkout of the parent commit with imcoalhmm_amd/libimcoal_fwd.so built")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def run_child(leg, path):
        env = dict(os.environ)
        for k in ("IMC_DEVICE_ENCODE", "IMC_DEVICE_INGEST", "IMC_DEVICE_TRAIN", "IMCOAL_FWD_LIB", "IMC_INGEST_SLAB_BYTES"):
            env.pop(k, None)
        tree = os.path.abspath(args.parent_tree) if leg.startswith("parent") else REPO
        cmd = ["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--child", leg, path, tree, str(args.runs)]
        out = subprocess.run(cmd, capture_output=True, text=True, env=env)
        res = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
        if out.returncode != 0 or not res:
            say("# FAILED: %s, exit status %d; nothing more is started\n%s" % (leg, out.returncode, out.stderr[-3000:]))
            return None
        return json.loads(res[0][7:])

    if args.parent_device:
        say("# device_alignment_ab --parent-device: per leg and size %d fresh child processes, legs interleaved, one round each; seconds, median [min .. max]" % args.runs)
    else:
        say("# device_alignment_ab: per leg and size one child process: a warm-up round, then %d timed rounds; seconds, median [min .. max]" % args.runs)
    say("# command: python profiles/tools/device_alignment_ab.py --parent-tree DIR%s --runs %d --sizes %s" % (" --parent-device" if args.parent_device else "", args.runs, args.sizes))
    say("# parent = the parent commit's package and library; branch = this tree; imc_set_device_encoding(1) and imc_set_device_training(1) in both; default slab size")
    with tempfile.TemporaryDirectory() as data_dir:
        for n in [int(s) for s in args.sizes.split(",") if s]:
            path = os.path.join(data_dir, "aln%d.fa" % n)
            t0 = time.time()
            write_alignment(path, n, seed=n % 1000)
            with open(path, "rb") as fh:                              # read once: the page cache holds the file
                while fh.read(1 << 24):
                    pass
            say("#\n# 4 records x %d bases wrapped at 60: %d bytes, written and read back in %.1f s" % (n, os.path.getsize(path), time.time() - t0))
            if args.parent_device:
                rounds = {"parent1": [], "branch1": []}
                for run in range(args.runs):
                    for leg in rounds:
                        r = run_child(leg, path)
                        if r is None:
                            return 1
                        rounds[leg].append(r)
                        say("run %d  n %-10d %-8s %s   crc32 %s" % (run, n, leg, "  ".join("%s %.3f" % (k.strip(), v[0]) for k, v in r["times"].items()), " ".join(r["crcs"])))
                same = len({tuple(r["crcs"]) for rs in rounds.values() for r in rs}) == 1
                say("# n %d: the six chunks' deepest token streams of all legs and runs %s" % (n, "IDENTICAL" if same else "DIFFER"))
                say("# n %d: Alignment.info %s" % (n, json.dumps(rounds["branch1"][0]["info"], sort_keys=True)))
                say("# this tree against the parent: difference of medians | spread (max - min) of the parent's own runs")
                for name in list(rounds["parent1"][0]["times"]) + ["total"]:
                    ts = {leg: [sum(v[0] for v in r["times"].values()) if name == "total" else r["times"][name][0] for r in rs] for leg, rs in rounds.items()}
                    for leg in rounds:
                        say("n %-10d %-8s %-32s %8.3f [%7.3f .. %7.3f]" % (n, leg, name, float(np.median(ts[leg])), min(ts[leg]), max(ts[leg])))
                    diff, spread = float(np.median(ts["branch1"]) - np.median(ts["parent1"])), max(ts["parent1"]) - min(ts["parent1"])
                    say("n %-10d branch1 - parent1 %-23s %+8.3f | %7.3f   %s" % (n, name, diff, spread, "inside" if diff <= spread else "OUTSIDE"))
                continue
            got = {}
            for leg in ("parent", "branch"):
                got[leg] = run_child(leg, path)
                if got[leg] is None:
                    return 1
            same = got["parent"]["crcs"] == got["branch"]["crcs"]
            say("# n %d: the six chunks' deepest token streams %s in the parent's (a), the branch's (a) and pairs(): crc32 %s" % (
                n, "IDENTICAL" if same else "DIFFER", " ".join(got["branch"]["crcs"])))
            say("# n %d: Alignment.info %s" % (n, json.dumps(got["branch"]["info"], sort_keys=True)))
            for leg in ("parent", "branch"):
                for name, ts in got[leg]["times"].items():
                    say("n %-10d %-7s %-42s %8.3f [%7.3f .. %7.3f]   runs %s" % (n, leg, name, float(np.median(ts)), min(ts), max(ts), " ".join("%.3f" % t for t in ts)))
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
