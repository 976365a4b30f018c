#!/usr/bin/env python3
"""Generate tests/golden/bench_oracle.json: CPU-oracle log-likelihoods of every workload bench.py times.

For each entry of tests/bench_workloads.py the inputs are regenerated through bench.py's own functions and evaluated
with the oracle's compressed forward (oracle_lib.Zip, the zipHMM-style restatement).  Recorded per workload:

* the sha256 of every generated chunk (the GPU tests refuse to compare against changed inputs);
* the log-likelihood of every proposal (total), and per chunk for the proposals FIXTURE_PROPOSALS;
* the 1e8-column single chains at 20 states: the textbook scaled forward of the whole chain (asserted to agree with the
  compressed forward within 1e-12) and the long-double forward of its first 2e6 columns;
* the headline: the value after one symbol s is replaced by (s + 1) % 3 at the first, middle and last column (asserted
  to move the value by more than 100 x the tests' 1e-11 tolerance);
* the divergence variants: theta and the realised P(different).

No alignment is stored.  CPU only; deterministic (per-chunk values do not depend on the thread schedule, totals are
left-to-right sums), so a rerun on the same machine reproduces the file byte for byte.

Run once:  python tests/golden/make_bench_oracle.py
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)

import bench_workloads as bw  # noqa: E402
from oracle import oracle_lib  # noqa: E402

TOL = 1e-11
HEAD = 2_000_000
THREADS = max(1, min(16, os.cpu_count() or 1))


def rel(a, b):
    return abs(a - b) / abs(b)


def evaluate(w, chunks):
    zips = [oracle_lib.Zip(c, 3) for c in chunks]
    pis, Ts, Es = bw.proposals(w)
    totals, per = [], {}
    for b in range(w.batch):
        tot, pc = oracle_lib.forward_chunks_mt(pis[b], Ts[b], Es[b], chunks, threads=THREADS, zips=zips)
        totals.append(float(tot))
        if b in bw.FIXTURE_PROPOSALS:
            per[str(b)] = [float(v) for v in pc]
    return {"total": totals, "per_chunk": per}


def main():
    oracle_lib.build()
    t_all = time.time()
    out = {"tolerance": TOL, "oracle": "oracle_lib.Zip (compressed forward), per chunk; totals left to right",
           "fixture_proposals": list(bw.FIXTURE_PROPOSALS), "workloads": {}}
    for name, w in bw.WORKLOADS.items():
        t0 = time.time()
        chunks = bw.generate(w)
        rec = {"states": w.states, "columns": w.columns, "chunks": len(chunks), "batch": w.batch,
               "sha256": [bw.digest(c) for c in chunks]}
        if w.theta is not None:
            rec["theta"] = list(w.theta)
            rec["p_different"] = bw.p_different(chunks[0])
        rec["zip"] = evaluate(w, chunks)
        zip0 = rec["zip"]["total"][0]
        if w.states == 20 and len(chunks) == 1 and w.columns == 100_000_000 and w.batch == 1:
            pi, T, E = bw.hmm(w)
            textbook = float(oracle_lib.forward_scaled(pi, T, E, chunks[0]))
            assert rel(textbook, zip0) < 1e-12, (name, textbook, zip0)
            head = chunks[0][:HEAD]
            head_ld = float(oracle_lib.forward_scaled_ld(pi, T, E, head))
            head_zip = float(oracle_lib.Zip(head, 3).forward(pi, T, E))
            assert rel(head_zip, head_ld) < 1e-12, (name, head_zip, head_ld)
            rec["textbook"] = textbook
            rec["head"] = {"columns": HEAD, "forward_scaled_ld": head_ld}
        if name == "headline":
            pi, T, E = bw.hmm(w)
            rec["mutants"] = []
            for col in bw.mutant_columns(w.columns):
                m = bw.mutate(chunks[0], col)
                v = float(oracle_lib.Zip(m, 3).forward(pi, T, E))
                assert rel(v, zip0) > 100 * TOL, (col, v, zip0)
                rec["mutants"].append({"column": col, "sha256": bw.digest(m), "zip": v, "rel_shift": rel(v, zip0)})
        out["workloads"][name] = rec
        print("%-14s %3d x %9d columns, batch %2d: %.16g  (%.1f s)" % (name, len(chunks), w.columns, w.batch, zip0,
                                                                       time.time() - t0), flush=True)
        del chunks
    path = os.path.join(HERE, "bench_oracle.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote %s (%d bytes) in %.0f s on %d threads" % (path, os.path.getsize(path), time.time() - t_all, THREADS))


if __name__ == "__main__":
    main()
