"""Opening a PHYLIP alignment: prepare.read_phylip / prepare.pairwise_forwarders(in_format="phylip") (a Python pass over
the file, two uploads per pair; both functions are the parent commit's, unchanged in this tree) against
imcoalhmm_amd.Alignment(path, in_format="phylip") (the file opened once on the device, csrc/kernels_phylip.hpp), with
Alignment(fasta_path) on the same sequences beside it.

    python profiles/tools/phylip_ab.py [--runs 5] [--sizes 10000000,100000000] [--host-interleaved 300000] [--out profiles/device_phylip_ab.txt]

Input: 4 records x n bases (a random root sequence; record k differs from it in 0.4 (k + 1) % of the columns, a few of them
N or gaps), written once by this driver, which never touches the GPU, in three files - PHYLIP with one line per record
(seq-gen's shape), PHYLIP interleaved at 60, FASTA wrapped at 60 - and read once before the first child, so every child
finds them in the page cache.
Legs, one child process per size and shape under its own `timeout`, with imc_set_device_encoding(1) and
imc_set_device_training(1), an untimed imc_set_device(0) first, then one warm-up round and --runs timed rounds:
    host     read_phylip(path);  pairwise_forwarders(path, in_format="phylip"), all six pairs
    device   Alignment(path, in_format="phylip");  pairs() of the open alignment;  one triplet chunk of the open alignment;
             Alignment(fasta_path)
read_phylip appends every line of an interleaved file to a string held in a list (`seqs[k % n] += ...`), which copies the
record so far: its time grows with the square of the record's length, so the host legs of the interleaved shape run at
--host-interleaved bases per record only (0: never) and are marked so.
Reported: median [min .. max] over the timed rounds, and the crc32 of the six chunks' deepest token streams, which the host
leg and the device leg must agree on.  A child that fails ends the run."""
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


def write_alignments(stem, n, seed):
    """stem.seq.phy, stem.int.phy and stem.fa with the same four records."""
    rng = np.random.default_rng(seed)
    root = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n)
    seqs = []
    for k in range(4):
        s = root.copy()
        flip = rng.random(n) < 0.004 * (k + 1)
        s[flip] = rng.choice(np.frombuffer(b"ACGTN-", dtype=np.uint8), size=int(flip.sum()))
        seqs.append(s)
    rows = n // 60

    def wrapped(fh, s, first_row, last_row):
        block = np.full((last_row - first_row, 61), 10, dtype=np.uint8)
        block[:, :60] = s[first_row * 60:last_row * 60].reshape(last_row - first_row, 60)
        block.tofile(fh)

    with open(stem + ".seq.phy", "wb") as fh:
        fh.write(b" 4 %d\n" % n)
        for k, s in enumerate(seqs):
            fh.write(b"%-10d" % (k + 1))
            s.tofile(fh)
            fh.write(b"\n")
    with open(stem + ".int.phy", "wb") as fh:                         # block b: row b of every record
        fh.write(b" 4 %d\n" % n)
        for k, s in enumerate(seqs):
            fh.write(b"%-10d" % (k + 1) + bytes(s[:60]) + b"\n")
        if rows > 1:
            block = np.full((rows - 1, 4, 61), 10, dtype=np.uint8)
            for k, s in enumerate(seqs):
                block[:, k, :60] = s[60:rows * 60].reshape(rows - 1, 60)
            block.tofile(fh)
        if n % 60 and rows:
            for s in seqs:
                fh.write(bytes(s[rows * 60:]) + b"\n")
    with open(stem + ".fa", "wb") as fh:
        for k, s in enumerate(seqs):
            fh.write(b">%d\n" % (k + 1))
            wrapped(fh, s, 0, rows)
            if n % 60:
                fh.write(bytes(s[rows * 60:]) + b"\n")


def child(path, fasta_path, host_legs, runs):
    sys.path.insert(0, REPO)
    from imcoalhmm_amd import Alignment, _capi, prepare
    lib = _capi.lib()
    _capi.check(lib.imc_set_device(0))                         # context creation, untimed
    _capi.check(lib.imc_set_device_encoding(1))
    _capi.check(lib.imc_set_device_training(1))
    times, crcs, info = {}, {}, {}

    def timed(name, fn, keep):
        gc.collect()
        t0 = time.perf_counter()
        out = fn()
        if keep:
            times.setdefault(name, []).append(time.perf_counter() - t0)
        return out

    def crc_of(fw):
        return ["%08x" % (zlib.crc32(fw[k].new_obs.astype(np.uint16).tobytes()) & 0xffffffff) for k in sorted(fw)]

    for run in range(-1, runs):
        keep = run >= 0
        if host_legs:
            timed("host    read_phylip", lambda: prepare.read_phylip(path), keep)
            fw = timed("host    pairwise_forwarders, six pairs", lambda: prepare.pairwise_forwarders(path, in_format="phylip"), keep)
            if run < 0:
                crcs["host"] = crc_of(fw)
            del fw
        aln = timed("device  Alignment(path, in_format='phylip')", lambda: Alignment(path, in_format="phylip"), keep)
        info = aln.info
        fw = timed("device    pairs() of the open alignment", aln.pairs, keep)
        if run < 0:
            crcs["device"] = crc_of(fw)
        del fw
        trip = timed("device    one triplet chunk of the open alignment", lambda: aln.forwarder(*aln.names[:3]), keep)
        del trip
        aln.close()
        if fasta_path:
            fa = timed("device  Alignment(fasta_path), same sequences", lambda: Alignment(fasta_path), keep)
            if run < 0:
                crcs["fasta"] = crc_of(fa.pairs())
                info = dict(info, fasta=fa.info)
            fa.close()
    print("RESULT " + json.dumps({"times": times, "crcs": crcs, "info": info}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sizes", default="10000000,100000000")
    ap.add_argument("--host-interleaved", type=int, default=300000, help="bases per record at which the interleaved shape's host legs run (0: never)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "device_phylip_ab.txt"))
    ap.add_argument("--child", nargs=4, metavar=("PATH", "FASTA", "HOST", "RUNS"))
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], args.child[2] == "1", int(args.child[3]))
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def run_child(path, fasta_path, host_legs):
        env = dict(os.environ)
        for k in ("IMC_DEVICE_ENCODE", "IMC_DEVICE_INGEST", "IMC_DEVICE_TRAIN", "IMCOAL_FWD_LIB", "IMC_INGEST_SLAB_BYTES"):
            env.pop(k, None)
        cmd = ["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--child", path, fasta_path, "1" if host_legs else "0", str(args.runs)]
        out = subprocess.run(cmd, capture_output=True, text=True, env=env)
        res = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
        if out.returncode != 0 or not res:
            say("# FAILED: %s, exit status %d; nothing more is started\n%s" % (os.path.basename(path), out.returncode, out.stderr[-3000:]))
            return None
        return json.loads(res[0][7:])

    say("# phylip_ab: per size and shape one child process: a warm-up round, then %d timed rounds; seconds, median [min .. max]" % args.runs)
    say("# command: python profiles/tools/phylip_ab.py --runs %d --sizes %s --host-interleaved %d" % (args.runs, args.sizes, args.host_interleaved))
    say("# host = prepare.read_phylip / prepare.pairwise_forwarders, the parent commit's functions (unchanged here); device = Alignment;")
    say("# imc_set_device_encoding(1) and imc_set_device_training(1) in all legs; default slab size")
    sizes = [int(s) for s in args.sizes.split(",") if s]
    plan = [(n, shape, shape == "seq") for n in sizes for shape in ("seq", "int")]
    if args.host_interleaved:
        plan.insert(0, (args.host_interleaved, "int", True))
    with tempfile.TemporaryDirectory() as data_dir:
        written = set()
        for n, shape, host_legs in plan:
            stem = os.path.join(data_dir, "aln%d" % n)
            if n not in written:
                t0 = time.time()
                write_alignments(stem, n, seed=n % 1000)
                for ext in (".seq.phy", ".int.phy", ".fa"):
                    with open(stem + ext, "rb") as fh:                # read once: the page cache holds the file
                        while fh.read(1 << 24):
                            pass
                written.add(n)
                say("#\n# 4 records x %d bases: one line per record %d bytes, interleaved at 60 %d bytes, FASTA wrapped at 60 %d bytes; written and read back in %.1f s" % (
                    n, os.path.getsize(stem + ".seq.phy"), os.path.getsize(stem + ".int.phy"), os.path.getsize(stem + ".fa"), time.time() - t0))
            path = stem + "." + shape + ".phy"
            got = run_child(path, stem + ".fa", host_legs)
            if got is None:
                return 1
            what = "one line per record" if shape == "seq" else "interleaved at 60"
            crcs = got["crcs"]
            same = len({tuple(v) for v in crcs.values()}) == 1
            say("# n %d, %s: the six chunks' deepest token streams %s in %s: crc32 %s" % (n, what, "IDENTICAL" if same else "DIFFER", ", ".join(sorted(crcs)), " ".join(crcs["device"])))
            say("# n %d, %s: Alignment.info %s" % (n, what, json.dumps(got["info"], sort_keys=True)))
            if not host_legs:
                say("# n %d, %s: host legs not run (read_phylip is quadratic in the record length on interleaved files; see n %d)" % (n, what, args.host_interleaved))
            for name, ts in got["times"].items():
                say("n %-10d %-4s %-50s %8.3f [%7.3f .. %7.3f]   runs %s" % (n, shape, name, float(np.median(ts)), min(ts), max(ts), " ".join("%.3f" % t for t in ts)))
            if not same:
                return 1
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
