"""What chunk creation and re-compression produce, as digests, for this tree and for a build of the parent commit side by side.

    python profiles/tools/chunk_digests.py --parent-tree DIR [--out profiles/chunk_paths_digests.txt]

(DIR: a checkout of the parent commit with its library built, `python -m imcoalhmm_amd.build` there; its legs import the
package and tests/device_encode_cases.py from it)

Per chunk one sha256 over the dictionary (left, right of every merged token) and, for every level of
device_encode_cases.K_LEVELS, the alphabet, the length, the tokens and the token counts; for the 3-symbol chunks also the
per-chunk log-likelihood of one 20-state HMM as a hex float.  The cases are the test modules' own small ones:
    three        the 3-symbol trainer compressible(3_000_000, seed=5), then chunks of 4096, 4097 and 65 537 columns under
                 imc_set_device_encoding(0) and (1)
    large        skewed_symbols(60_000, nsym) for 65 and 257 symbols, the creation that trains, under both switches
    recompress   the five arrays of test_recompress_batched_on_the_device, created and recompressed under both switches
    from_device  Forwarder.from_device (torch imported first): a 3-symbol chunk with a published dictionary, and the
                 257-symbol creation that trains on the head copied back
    min_count    `three` (trainer and the 65 537-column chunk) with IMC_DICT_MIN_COUNT=2
    max_depth    ... with IMC_DICT_MAX_DEPTH=6
Every case is one fresh child process under its own `timeout`; a child that fails ends the run.  The driver never touches
the GPU."""
import argparse
import hashlib
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CASES = (("three", {}), ("large", {}), ("recompress", {}), ("from_device", {}), ("min_count", {"IMC_DICT_MIN_COUNT": "2"}),
         ("max_depth", {"IMC_DICT_MAX_DEPTH": "6"}))


def child(case, tree):
    sys.path.insert(0, os.path.join(tree, "tests"))
    sys.path.insert(0, tree)
    if case == "from_device":
        import torch                                  # torch first: its bundled HIP runtime must be the one that initialises
    import device_encode_cases as dc
    from imcoalhmm_amd import Forwarder, _capi, synth
    from imcoalhmm_amd.hmm import forward_chunks_batch, recompress, set_device_encoding
    lib = _capi.lib()
    pi, T, E = synth.random_hmm(20, 3, seed=2020, stay=0.97)

    def digest(f):
        h = hashlib.sha256()
        pairs = f.sym2pair
        h.update(np.array([(t,) + tuple(pairs[t]) for t in sorted(pairs)], dtype=np.int64).tobytes())
        for limit in dc.K_LEVELS:
            n, used = f.compressed_length(limit)
            tok, used2 = dc.tokens(f, limit)
            assert used2 == used and tok.size == n
            h.update(np.array([limit, used, n], dtype=np.int64).tobytes())
            h.update(tok.astype(np.uint16).tobytes())
            h.update(f.token_counts(limit).astype(np.uint32).tobytes())
        return h.hexdigest()

    def say(name, f, loglik=None):
        print("DIGEST %-40s alphabet %5d  %s%s" % (name, f.compressed_length(16384)[1], digest(f),
                                                    "" if loglik is None else "  loglik " + float(loglik).hex()), flush=True)

    def logliks(fw):
        return forward_chunks_batch([f.handle for f in fw], pi[None], T[None], E[None], per_chunk=True)[0]

    try:
        if case in ("three", "min_count", "max_depth"):
            trainer, _ = dc.train3()
            say(case + " trainer", trainer)
            for n in ((4096, 4097, 65537) if case == "three" else (65537,)):
                fw = dc.host_and_device(dc.compressible(n, seed=1000 + n), 3)
                for switch, (f, ll) in enumerate(zip(fw, logliks(fw))):
                    say("%s %d switch %d" % (case, n, switch), f, ll)
        elif case == "large":
            for nsym in (65, 257):
                for switch in (0, 1):
                    _capi.check(lib.imc_dictionary_reset())
                    set_device_encoding(switch)
                    say("large %d switch %d" % (nsym, switch), Forwarder.from_array(dc.skewed_symbols(60_000, nsym, seed=nsym), nsym))
        elif case == "recompress":
            arrays = [dc.compressible(n, seed=40 + k) for k, n in enumerate((40_000, 4096, 100, 7, 70_000))]
            for switch in (0, 1):
                _capi.check(lib.imc_dictionary_reset())
                set_device_encoding(switch)
                fw = [Forwarder.from_array(a, 3) for a in arrays]
                recompress(fw)
                for k, (f, ll) in enumerate(zip(fw, logliks(fw))):
                    say("recompress chunk %d switch %d" % (k, switch), f, ll)
        elif case == "from_device":
            dc.train3()
            f = Forwarder.from_device(torch.from_numpy(dc.compressible(70_001, seed=21)).to("cuda"), 3)
            say("from_device uint8 3", f, logliks([f])[0])
            _capi.check(lib.imc_dictionary_reset())
            obs257 = dc.skewed_symbols(60_000, 257, seed=33)
            say("from_device int16 257 (trains)", Forwarder.from_device(torch.from_numpy(obs257.astype(np.int16)).to("cuda"), 257))
    finally:
        set_device_encoding(0)
    print("CASE OK", flush=True)


def run_tree(tree, say):
    out = []
    for case, extra in CASES:
        env = dict(os.environ, **extra)
        for name in ("IMC_DEVICE_ENCODE", "IMCOAL_FWD_LIB") + tuple(k for k in ("IMC_DICT_MIN_COUNT", "IMC_DICT_MAX_DEPTH") if k not in extra):
            env.pop(name, None)
        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", case, tree]
        run = subprocess.run(cmd, capture_output=True, text=True, env=env)
        if run.returncode != 0 or "CASE OK" not in run.stdout:
            say("# FAILED: %s in %s, exit status %d; nothing more is started\n%s" % (case, tree, run.returncode, (run.stdout + run.stderr)[-3000:]))
            return None
        out += [ln[7:] for ln in run.stdout.splitlines() if ln.startswith("DIGEST ")]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "chunk_paths_digests.txt"))
    ap.add_argument("--child", nargs=2, metavar=("CASE", "TREE"))
    args = ap.parse_args()
    if args.child:
        return child(*args.child)
    if not args.parent_tree or not os.path.exists(os.path.join(args.parent_tree, "imcoalhmm_amd", "libimcoal_fwd.so")):
        ap.error("--parent-tree: a checkout of the parent commit with imcoalhmm_amd/libimcoal_fwd.so built")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("# chunk_digests: sha256 per chunk over the dictionary and, per level, alphabet, length, tokens and token counts;")
    say("# per-chunk log-likelihood of one 20-state HMM as a hex float.  parent = the parent commit's package and library.")
    rows = {}
    for leg, tree in (("parent", os.path.abspath(args.parent_tree)), ("branch", REPO)):
        rows[leg] = run_tree(tree, say)
        if rows[leg] is None:
            return 1
    differ = 0
    for i in range(max(len(rows["parent"]), len(rows["branch"]))):
        p = rows["parent"][i] if i < len(rows["parent"]) else "(missing)"
        b = rows["branch"][i] if i < len(rows["branch"]) else "(missing)"
        differ += p != b
        say("parent %s\nbranch %s   %s" % (p, b, "same" if p == b else "DIFFERENT"))
    say("# %d rows, %s" % (len(rows["branch"]), "parent and branch IDENTICAL" if not differ else "%d rows DIFFER" % differ))
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
