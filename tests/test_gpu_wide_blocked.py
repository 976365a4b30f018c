"""25 to 32 states on the register-blocked fp64-MFMA scan (k_zpropagate4<7> / <8>: workgroups of four wavefronts and 16
segments, streamed operator table built one dictionary depth per launch; imc_set_wide_blocked), against the CPU oracle.

Tolerance: the suite's 1e-11 relative (the engine only re-associates fp64 arithmetic, rescaling by exact powers of two).
"""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import rel_err
from imcoalhmm_amd import Forwarder, _capi, synth
from imcoalhmm_amd.hmm import forward_chunks_batch

pytestmark = pytest.mark.gpu
TOL = 1e-11
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED = [0, 1, 2, 15, 16, 17, 31, 32, 33, 1000, 4097, 65255, 0, 20000]


def scan_name(n):
    return "k_zpropagate4<%d" % ((n + 3) // 4)


@pytest.fixture(autouse=True)
def _defaults():
    L = _capi.lib()
    assert L.imc_device_count() >= 1, "gpu tests need a device"
    _capi.check(L.imc_set_compression(1))
    _capi.check(L.imc_set_segment_length(0))
    _capi.check(L.imc_dictionary_reset())
    yield
    L.imc_set_segment_length(0)
    L.imc_set_compression(1)
    if hasattr(L, "imc_set_wide_blocked"):
        L.imc_set_wide_blocked(-1)


def compressible(n, seed, nsym=3):
    rng = np.random.default_rng(seed)
    p = np.full(nsym, 0.1 / max(nsym - 1, 1)); p[0] = 0.9
    return rng.choice(nsym, size=n, p=p / p.sum()).astype(np.uint8)


def forwarders(chunks, first):
    """One Forwarder per chunk, chunk `first` created first: it trains the dictionary the others are encoded with."""
    fw = [None] * len(chunks)
    for k in [first] + [k for k in range(len(chunks)) if k != first]:
        fw[k] = Forwarder.from_array(chunks[k], 3)
    return fw


_want = {}


def oracle_values(oracle, key, hmms, chunks):
    """[b][chunk] oracle log-likelihoods, computed once per key and shared by the tests (never modified)."""
    if key not in _want:
        _want[key] = [[oracle.forward_scaled(pi, T, E, c) if c.size else 0.0 for c in chunks] for pi, T, E in hmms]
    return _want[key]


def close(g, w):
    return (g == 0.0 and w == 0.0) or rel_err(g, w) < TOL


def run(fw, hmms, per_chunk=True):
    pis, Ts, Es = (np.stack([h[k] for h in hmms]) for k in range(3))
    got = forward_chunks_batch([f.handle for f in fw], pis, Ts, Es, per_chunk=per_chunk)
    return got, _capi.last_plan()


@pytest.mark.parametrize("n", [25, 28, 29, 32])
def test_parity_batches_and_repeats(oracle, n):
    """Padding inside the last tile at odd and even tile counts (25, 29), exact fits (28, 32), the odd count's EXTRA
    part of the table layout (25, 28); compressible chunks beside one too short to be compressed; stitching forced
    (48-token segments) and automatic; one and three parameter sets."""
    _capi.set_wide_blocked(1)
    hmms = [synth.random_hmm(n, 3, seed=300 + n + 1000 * b, stay=0.97) for b in range(3)]
    chunks = [compressible(L, seed=n * 10 + k) for k, L in enumerate((40_000, 5000, 4096, 100, 33_000))]
    want = oracle_values(oracle, ("parity", n), hmms, chunks)
    fw = forwarders(chunks, 0)
    for seg in (48, 0):
        _capi.check(_capi.lib().imc_set_segment_length(seg))
        got3, plan = run(fw, hmms)
        assert scan_name(n) in plan["kernels"], plan["kernels"]
        assert plan["vector_tokens"] > 0 and plan["vector_columns"] > 0, plan      # the 100-column chunk stays on its per-column kernel
        again, _ = run(fw, hmms)
        assert np.array_equal(got3, again), (n, seg)
        for b in range(3):
            got1, plan1 = run(fw, hmms[b:b + 1])
            assert scan_name(n) in plan1["kernels"], plan1["kernels"]
            print("n=%d seg=%d b=%d batch %r single %r" % (n, seg, b, got3[b].tolist(), got1[0].tolist()))
            for k in range(len(chunks)):
                assert close(got1[0][k], want[b][k]), (n, seg, b, k, got1[0][k], want[b][k])
                assert close(got3[b][k], want[b][k]), (n, seg, b, k, got3[b][k], want[b][k])
            # the bits follow the cut: forced, it is the same for one set and for three; automatic, the planner's segment
            # length depends on the number of sets (as up to 24 states), and the rows are compared where it came out equal
            if seg or (plan1["token_segment_len"], plan1["token_alphabet"]) == (plan["token_segment_len"], plan["token_alphabet"]):
                assert np.array_equal(got3[b], got1[0]), (n, seg, b, got3[b], got1[0], plan, plan1)


def segs_for(ntok, k):
    """Forced segment lengths (the library rounds them to 16 tokens) that cut ntok tokens into about k segments."""
    return [seg for seg in range(16, ntok + 32, 16) if abs(-(-ntok // seg) - k) <= 1]


@pytest.mark.parametrize("n", [28, 32])
def test_ragged_shapes(oracle, n):
    """Empty, one-column and short chunks beside compressed ones in one call (forced and automatic segment length, two
    parameter sets); then single chunks cut into 1, 2, 4, 5, 16 and 17 segments - a packed block, the fold's stage A
    alone, stage B with two to four wavefronts, two workgroups - into more than 16 workgroups (stitch launches) and
    into at most four (fused tail)."""
    _capi.set_wide_blocked(1)
    L = _capi.lib()
    hmms = [synth.random_hmm(n, 3, seed=4100 + n + 1000 * b, stay=0.97) for b in range(2)]
    chunks = [compressible(m, seed=n * 31 + k) for k, m in enumerate(RAGGED)] + [compressible(200_000, seed=n * 31 + 99)]
    want = oracle_values(oracle, ("ragged", n), hmms, chunks)
    fw = forwarders(chunks, RAGGED.index(65255))
    for seg in (48, 0, 4096):
        _capi.check(L.imc_set_segment_length(seg))
        got, plan = run(fw[:len(RAGGED)], hmms)
        assert scan_name(n) in plan["kernels"], plan["kernels"]
        for b in range(2):
            for k in range(len(RAGGED)):
                assert close(got[b][k], want[b][k]), (n, seg, b, k, RAGGED[k], got[b][k], want[b][k])
    # single chunks by number of segments
    _capi.check(L.imc_set_segment_length(0))
    cand = [k for k in range(len(chunks)) if chunks[k].size > 4096]
    ntoks = {}
    for k in cand:
        _, plan = run([fw[k]], hmms)
        assert scan_name(n) in plan["kernels"], (k, plan["kernels"])
        ntoks[k] = plan["tokens"]
    seen = {}
    for k in cand:
        for seg in sorted({16} | {s for nseg in (1, 2, 4, 5, 16, 17) for s in segs_for(ntoks[k], nseg)}):
            _capi.check(L.imc_set_segment_length(seg))
            got, plan = run([fw[k]], hmms)
            assert scan_name(n) in plan["kernels"], (k, seg, plan)
            for b in range(2):
                assert close(got[b][0], want[b][k]), (n, k, seg, plan["segments"], b, got[b][0], want[b][k])
            fused = "fused-tail" in plan["kernels"]
            assert fused == (plan["segments"] <= 64), (seg, plan)      # at most four workgroups of 16 segments (IMC_FUSE_TAIL's default)
            seen[plan["segments"]] = fused
    print("n=%d tokens %r, segment counts run: %r" % (n, ntoks, sorted(seen)))
    assert all(nseg in seen for nseg in (1, 2, 4, 5, 16, 17)), sorted(seen)
    assert any(nseg > 256 for nseg in seen), sorted(seen)              # more than 16 workgroups: the stitch launches
    assert any(16 < nseg <= 64 and f for nseg, f in seen.items())      # several workgroups meeting in the fused tail


def smallest_wide_training_length(nsym=3):
    """Shortest first chunk (in steps of 100 000 columns) whose dictionary has more than 256 tokens."""
    for m in range(100_000, 3_000_001, 100_000):
        _capi.check(_capi.lib().imc_dictionary_reset())
        f = Forwarder.from_array(compressible(m, seed=5), nsym)
        if f.compressed_length(16384)[1] > 256:
            return m
    return None


def test_sixteen_bit_tokens(oracle):
    """A dictionary beyond 256 tokens: the scan on a 16-bit token stream (k_zpropagate4<8,16,...>).  The training chunk
    is the shortest that gives such a dictionary; where the planner's estimate prefers a byte level for so little data,
    the level is pinned (IMC_FORCE_LEVEL, read when a plan is built)."""
    n = 32
    _capi.set_wide_blocked(1)
    m = smallest_wide_training_length()
    assert m is not None
    print("smallest training chunk with more than 256 tokens: %d columns" % m)
    pi, T, E = synth.random_hmm(n, 3, seed=5000 + n, stay=0.97)
    chunks = [compressible(m, seed=5), compressible(50_000, seed=6), compressible(7, seed=7)]
    want = oracle_values(oracle, ("wide16", m), [(pi, T, E)], chunks)[0]
    _capi.check(_capi.lib().imc_dictionary_reset())
    fw = [Forwarder.from_array(c, 3) for c in chunks]
    assert fw[0].compressed_length(16384)[1] > 256
    try:
        _, plan = run(fw, [(pi, T, E)])
        level = 23
        while plan["token_alphabet"] <= 256 and level > 0:
            level -= 1
            os.environ["IMC_FORCE_LEVEL"] = str(level)
            _, plan = run(fw, [(pi, T, E)])
        print("level %s: %r" % (os.environ.get("IMC_FORCE_LEVEL", "automatic"), plan))
        for seg in (0, 4096, 48):
            _capi.check(_capi.lib().imc_set_segment_length(seg))
            got, plan = run(fw, [(pi, T, E)])
            assert scan_name(n) + ",16" in plan["kernels"], plan["kernels"]
            assert plan["token_alphabet"] > 256, plan
            for k in range(len(chunks)):
                assert close(got[0][k], want[k]), (seg, k, got[0][k], want[k])
    finally:
        os.environ.pop("IMC_FORCE_LEVEL", None)


@pytest.mark.parametrize("n", [28, 32])
def test_against_the_present_kernels(oracle, n):
    """Mode 0 (the kernels of before) and mode 1 agree within the tolerance; the automatic mode returns the bits of one
    of them."""
    hmms = [synth.random_hmm(n, 3, seed=6100 + n + b, stay=0.97) for b in range(2)]
    chunks = [compressible(m, seed=n * 7 + k) for k, m in enumerate((120_000, 30_000, 9_000))]
    fw = forwarders(chunks, 0)
    res = {}
    for mode in (0, 1, -1):
        _capi.set_wide_blocked(mode)
        res[mode], plan = run(fw, hmms)
        print("n=%d wide_blocked=%d: %s" % (n, mode, plan["kernels"]))
        assert (scan_name(n) in plan["kernels"]) == (mode == 1) or mode == -1, (mode, plan["kernels"])
    assert np.max(np.abs(res[0] / res[1] - 1.0)) < TOL, (res[0], res[1])
    assert np.array_equal(res[-1], res[0]) or np.array_equal(res[-1], res[1])
    want = oracle_values(oracle, ("old", n), hmms, chunks)
    for b in range(2):
        for k in range(len(chunks)):
            assert close(res[1][b][k], want[b][k]) and close(res[0][b][k], want[b][k]), (n, b, k)


@pytest.mark.parametrize("n", [25, 32])
def test_edge_values(n):
    """A symbol no state can emit gives -inf; a NaN in T gives NaN."""
    _capi.set_wide_blocked(1)
    pi, T, E = synth.random_hmm(n, 3, seed=7100 + n, stay=0.97)
    chunk = compressible(40_000, seed=n)
    fw = [Forwarder.from_array(chunk, 3)]
    E0 = E.copy(); E0[:, 2] = 0.0; E0 /= E0.sum(axis=1, keepdims=True)
    with np.errstate(all="ignore"):
        got, plan = run(fw, [(pi, T, E0)])
    assert scan_name(n) in plan["kernels"], plan["kernels"]
    assert (chunk == 2).any() and got[0][0] == -np.inf, got
    Tn = T.copy(); Tn[3, 5] = np.nan
    with np.errstate(all="ignore"):
        got, plan = run(fw, [(pi, Tn, E)])
    assert scan_name(n) in plan["kernels"] and np.isnan(got[0][0]), (plan["kernels"], got)


def test_split_alignment_operators(oracle):
    """imc_forward_state(as_operator=1): an alignment in three slices - the vector of the first, the exact transfer
    operators of the others from the blocked scan - recombines to the log-likelihood of the whole alignment."""
    from imcoalhmm_amd.hmm import combine_states, forward_states
    n = 28
    _capi.set_wide_blocked(1)
    hmms = [synth.random_hmm(n, 3, seed=8100 + 3 * n + b, stay=0.95) for b in range(2)]
    pis, Ts, Es = (np.stack([h[k] for h in hmms]) for k in range(3))
    whole = compressible(130_000, seed=n + 1)
    cuts = [0, 50_000, 90_000, whole.size]
    fw = [Forwarder.from_array(whole[a:b], 3) for a, b in zip(cuts[:-1], cuts[1:])]
    fw_whole = Forwarder.from_array(whole, 3)
    want = oracle_values(oracle, ("split", n), hmms, [whole])
    for seg in (0, 48):
        _capi.check(_capi.lib().imc_set_segment_length(seg))
        vec, vexp = forward_states([fw[0].handle], pis, Ts, Es, as_operator=False)
        assert scan_name(n) in _capi.last_plan()["kernels"], _capi.last_plan()["kernels"]
        ops, oexp = forward_states([f.handle for f in fw[1:]], pis, Ts, Es, as_operator=True)
        assert scan_name(n) in _capi.last_plan()["kernels"], _capi.last_plan()["kernels"]
        one = forward_chunks_batch([fw_whole.handle], pis, Ts, Es)
        for b in range(2):
            got = combine_states(vec[b, 0], vexp[b, 0], ops[b], oexp[b])
            assert rel_err(got, want[b][0]) < TOL, (seg, b, got, want[b][0])
            assert rel_err(one[b], want[b][0]) < TOL, (seg, b, one[b], want[b][0])
            assert rel_err(got, one[b]) < TOL


GUARD_SCRIPT = textwrap.dedent('''
    import os, sys
    import numpy as np
    sys.path.insert(0, %r)
    from imcoalhmm_amd import Forwarder, _capi, synth
    from imcoalhmm_amd.hmm import forward_chunks_batch
    from oracle import oracle_lib
    oracle_lib.build()
    L = _capi.lib()
    _capi.set_wide_blocked(1)
    ragged = %r

    def compressible(n, seed):
        rng = np.random.default_rng(seed)
        return rng.choice(3, size=n, p=[0.9, 0.05, 0.05]).astype(np.uint8)

    tails = 0
    for n in (28, 32):
        hmms = [synth.random_hmm(n, 3, seed=4100 + n + 1000 * b, stay=0.97) for b in range(2)]
        pis, Ts, Es = (np.stack([h[k] for h in hmms]) for k in range(3))
        chunks = [compressible(m, seed=n * 31 + k) for k, m in enumerate(ragged)]
        L.imc_dictionary_reset()
        order = sorted(range(len(chunks)), key=lambda k: -chunks[k].size)       # the longest chunk trains the dictionary
        fw = {k: Forwarder.from_array(chunks[k], 3) for k in order}
        want = [[oracle_lib.forward_scaled(pis[b], Ts[b], Es[b], c) if c.size else 0.0 for c in chunks] for b in range(2)]
        for seg in (48, 0, 4096):
            L.imc_set_segment_length(seg)
            per = forward_chunks_batch([fw[k].handle for k in range(len(chunks))], pis, Ts, Es, per_chunk=True)
            assert "k_zpropagate4<%%d" %% (n // 4) in _capi.last_plan()["kernels"], _capi.last_plan()["kernels"]
            for b in range(2):
                for k in range(len(chunks)):
                    w = want[b][k]
                    assert (per[b][k] == 0.0 and w == 0.0) or abs(per[b][k] - w) <= 1e-11 * abs(w), (n, seg, b, k, per[b][k], w)
        # the fused tail with up to 16 workgroups of a chunk (IMC_FUSE_TAIL=2), twice: the arrival counters must be back at zero
        k = ragged.index(65255)
        for seg in (16, 32, 64, 128):
            L.imc_set_segment_length(seg)
            for rep in range(2):
                per = forward_chunks_batch([fw[k].handle], pis, Ts, Es, per_chunk=True)
                tails += "fused-tail" in _capi.last_plan()["kernels"]
                for b in range(2):
                    assert abs(per[b][0] - want[b][k]) <= 1e-11 * abs(want[b][k]), (n, seg, rep, b, per[b][0], want[b][k], _capi.last_plan())
        L.imc_set_segment_length(0)
        del fw
    assert tails >= 4, tails
    print("wide guard ok", tails, flush=True)
''') % (REPO, RAGGED)


def test_ragged_under_guard_pages(tmp_path):
    """The ragged call once more with every device buffer flush against an unmapped page (IMC_GUARD=1), and the fused
    tail forced on for chunks of up to 16 workgroups (IMC_FUSE_TAIL=2), in a child process."""
    script = tmp_path / "wide_guard.py"
    script.write_text(GUARD_SCRIPT)
    env = dict(os.environ, IMC_GUARD="1", IMC_FUSE_TAIL="2")
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300, env=env)
    tail = (out.stdout[-1500:], out.stderr[-3000:])
    if "hipMemAddressReserve" in out.stderr or "hipMemCreate" in out.stderr or "hipMemGetAllocationGranularity" in out.stderr:
        pytest.skip("HIP virtual-memory management is unavailable on this box: %r" % (tail,))
    assert out.returncode == 0 and "wide guard ok" in out.stdout, tail
