"""Launch sequence and results of a fixed list of small calls, one line per case: imc_last_kernels(), the eight numbers
of imc_last_plan() and every log-likelihood as float.hex() ([parameter set][chunk]).  A case of more than three chunks
prints per parameter set the sum over the chunks and one sha256 over the per-chunk values' hex strings instead, which
keeps a line short at 40 chunks x 9 sets; imc_forward_state cases print a digest of the returned state.  The last cases
run on a dictionary trained on a 2.4e7-column chunk (16-bit token levels, segments long enough for the rank-one hand-off);
behind them come shapes on which the planner's decisions are not trivial (PLANNER_SETS: the shapes of
tests/test_gpu_planner.py at half the columns, populations of parameter sets over 30 chunks, one long chunk beside 200
short ones, and a forced segment length).

A change of the host side that is meant to leave every launch alone is run through this on the build before and the
build after it (IMCOAL_FWD_LIB selects the library), once per launch-schedule switch of the environment - the switches
are read when the library's context is created, so every setting is a process of its own (profiles/README.md).  The
two outputs must be byte-identical.

    python profiles/tools/launch_sequence.py > out.txt
"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from imcoalhmm_amd import Forwarder, _capi, synth                     # noqa: E402
from imcoalhmm_amd.hmm import forward_chunks_batch, forward_states    # noqa: E402

STATES = (4, 10, 20, 24, 28, 32, 40, 48, 100, 150)
BATCHES = (1, 3, 9)
CHUNK_SETS = ("one", "ragged", "many")


def cases():
    """(N, chunk set, B, compression, blocked kernel, table streaming, wide blocked, state mode or None)."""
    out = []
    for i, n in enumerate(STATES):                                 # every size on every chunk set, automatic modes
        for j, cs in enumerate(CHUNK_SETS):
            out.append((n, cs, BATCHES[(i + j) % 3], 1, 4, -1, -1, None))
    for mode in range(6):                                          # imc_set_compression
        for i, n in enumerate((10, 20, 28, 48, 150)):
            out.append((n, CHUNK_SETS[(mode + i) % 3], BATCHES[(mode + 2 * i) % 3], mode, 4, -1, -1, None))
    for variant in (2, 3, 4, 5):                                   # imc_set_blocked_kernel, pinned to the blocked family
        for i, n in enumerate((10, 20, 24)):
            out.append((n, CHUNK_SETS[(variant + i) % 3], BATCHES[(variant + i) % 3], 3, variant, -1, -1, None))
    for streaming in (0, 1):                                       # imc_set_table_streaming, hybrid table wherever possible
        for i, n in enumerate((10, 20)):
            for b in BATCHES:
                out.append((n, CHUNK_SETS[i], b, 3, 5, streaming, -1, None))
    for wide in (0, 1):                                            # imc_set_wide_blocked
        for i, n in enumerate((28, 32)):
            for j, cs in enumerate(("one", "many")):
                out.append((n, cs, BATCHES[(wide + i + j) % 3], 1, 4, -1, wide, None))
    for as_operator in (0, 1):                                     # imc_forward_state
        for i, n in enumerate((4, 20, 28, 48, 100)):
            out.append((n, CHUNK_SETS[i % 3], BATCHES[(as_operator + i) % 3], 1, 4, -1, -1, as_operator))
    return out


# chunk sets of the planner cases: (chunks, columns of the first, columns of the others); chunk k is 37 k columns longer
PLANNER_SETS = {"gemm-or-matvec": (10, 50_000, 50_000), "many-short": (100, 5_000, 5_000), "mid": (32, 30_000, 30_000),
                "slots": (3, 150_000, 150_000), "population": (30, 300_000, 300_000), "long-and-short": (201, 2_400_000, 20_000)}
# (N, chunk set, B, segment length): automatic modes
PLANNER_CASES = [(32, "gemm-or-matvec", 4, 0), (48, "many-short", 1, 0), (64, "mid", 4, 0), (100, "slots", 1, 0),
                 (10, "population", 16, 0), (20, "population", 8, 0), (20, "long-and-short", 8, 0), (32, "gemm-or-matvec", 4, 64)]


def main():
    L = _capi.lib()
    gen = synth.random_hmm(6, 3, seed=11, stay=0.995)
    lengths = {"one": (200_000,), "one-capped": (50_000,), "ragged": (70_001, 0, 4_099), "many": (5_000,) * 40}
    chunks = {}
    for k, (name, lens) in enumerate(lengths.items()):             # (the long chunk first: it trains the dictionary)
        chunks[name] = [Forwarder.from_array(synth.sample_alignment(*gen, m, seed=100 * k + q), 3) for q, m in enumerate(lens)]
    long_cases = [(150, "long", 1, 1, 4, -1, -1, None), (20, "long", 3, 3, 5, -1, -1, None), (20, "long", 1, 3, 5, 0, -1, None)]
    planner_cases = [(n, cs, b, 1, 4, -1, -1, None, seg) for n, cs, b, seg in PLANNER_CASES]
    for n, cs, b, mode, variant, streaming, wide, state, seg in [c + (0,) for c in cases() + long_cases] + planner_cases:
        if cs == "one" and n >= 100:
            cs = "one-capped"
        if cs == "long" and cs not in chunks:                      # a new dictionary, trained on the long chunk
            _capi.check(L.imc_dictionary_reset())
            chunks[cs] = [Forwarder.from_array(synth.sample_alignment(*gen, 24_000_000, seed=77), 3)]
        if cs in PLANNER_SETS and cs not in chunks:                # (encoded with the long chunk's dictionary)
            count, first, rest = PLANNER_SETS[cs]
            chunks[cs] = [Forwarder.from_array(synth.sample_alignment(*gen, (rest if q else first) + 37 * q, seed=9200 + q), 3)
                          for q in range(count)]
        tag = "N=%d %s B=%d c=%d k=%d s=%d w=%d %s" % (n, cs, b, mode, variant, streaming, wide,
                                                      "loglik" if state is None else "state%d" % state)
        if seg:
            tag += " seg=%d" % seg
        try:
            _capi.check(L.imc_set_compression(mode))
            _capi.check(L.imc_set_blocked_kernel(variant))
            _capi.check(L.imc_set_table_streaming(streaming))
            _capi.check(L.imc_set_wide_blocked(wide))
            _capi.check(L.imc_set_segment_length(seg))
            hmms = [synth.random_hmm(n, 3, seed=1000 + 10 * n + q, stay=0.995) for q in range(b)]
            params = [np.stack([h[k] for h in hmms]) for k in range(3)]
            handles = [f.handle for f in chunks[cs] if state is None or len(f)]    # (imc_forward_state takes no empty chunk)
            if state is None:
                v = forward_chunks_batch(handles, *params, per_chunk=True)
                values = " ".join(float(x).hex() for x in v.ravel())
                if len(handles) > 3:
                    sums = [sum((float(x) for x in row), 0.0) for row in v]            # (left to right, as imc_forward_batch sums)
                    values = " ".join(x.hex() for x in sums) + " | chunks " + hashlib.sha256(values.encode()).hexdigest()
            else:
                st, ex = forward_states(handles, *params, as_operator=bool(state))
                values = hashlib.sha256(st.tobytes() + ex.tobytes()).hexdigest()
            plan = _capi.last_plan()
            keys = [k for k in plan if k != "kernels"]
            print(tag, "|", plan["kernels"], "|", " ".join(str(plan[k]) for k in keys), "|", values, flush=True)
        except (ValueError, MemoryError, RuntimeError) as e:
            print(tag, "| error:", e, flush=True)


if __name__ == "__main__":
    main()
