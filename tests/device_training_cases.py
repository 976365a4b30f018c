"""Shared by tests/test_gpu_device_training.py and the child processes it starts: one training with the host trainer and
one with the device trainer (imc_set_device_training) from the same symbols, and what is compared - the dictionary entry
for entry, the chunk at every level (device_encode_cases.assert_same_chunk), what imc_last_training reports."""
import os

import numpy as np

from device_encode_cases import assert_same_chunk, compressible, skewed_symbols
from imcoalhmm_amd import Forwarder, _capi
from imcoalhmm_amd.hmm import recompress, set_device_encoding, set_device_training

RETRY_RECIPE = (40_000, 190, 190)      # skewed_symbols(n, nsym, seed): the host's byte phase stops at 192..255 tokens and runs again


def periodic(n, period):
    obs = np.zeros(n, dtype=np.uint8)
    if period > 1:
        obs[period - 1::period] = 1
    return obs


def trained_both_ways(make, what, device_encoding=0):
    """make() -> Forwarder, called as the creation that trains its alphabet's dictionary: once with the host trainer,
    once with the device trainer.  Asserts the same dictionary, the same chunk and the same training statistics;
    returns (host-trained chunk, device-trained chunk, statistics)."""
    L = _capi.lib()
    try:
        set_device_encoding(device_encoding)
        _capi.check(L.imc_set_compression(1))
        _capi.check(L.imc_dictionary_reset())
        set_device_training(0)
        a = make()
        how_a = _capi.last_training()
        _capi.check(L.imc_dictionary_reset())
        set_device_training(1)
        b = make()
        how_b = _capi.last_training()
    finally:
        set_device_training(0)
        set_device_encoding(0)
        _capi.check(L.imc_dictionary_reset())
    assert how_a["path"] == 0 and how_b["path"] == 1, (what, how_a, how_b)
    sa, sb = a.sym2pair, b.sym2pair
    assert len(sa) == len(sb), (what, len(sa), len(sb), how_a, how_b)
    assert sa == sb, (what, [(z, sa[z], sb[z]) for z in sorted(sa) if sa[z] != sb[z]][:4])
    assert {k: how_a[k] for k in ("symbols", "attempts", "rounds")} == {k: how_b[k] for k in ("symbols", "attempts", "rounds")}, (what, how_a, how_b)
    assert_same_chunk(a, b, what)
    return a, b, how_b


def small_cases():
    """(name, symbols, nsym) of the cases the guard-mode child runs too: a byte phase that stops below 256 tokens, streams
    that collapse to a handful of elements, and a 16-bit raw alphabet."""
    yield "40000 compressible", compressible(40_000, seed=5), 3
    for period in (1, 2, 3):
        yield "period %d" % period, periodic(40_000, period), 3
    yield "1000 symbols", skewed_symbols(100_000, 1000, seed=1000), 1000


def recompressed_both_ways(arrays, nsym, what):
    """The chunks of `arrays`, created and then recompressed, with the host trainer and with the device trainer (device
    encoding on in both): the same dictionary and the same chunks."""
    L = _capi.lib()
    seen = []
    try:
        set_device_encoding(1)
        for switch in (0, 1):
            _capi.check(L.imc_dictionary_reset())
            set_device_training(switch)
            fw = [Forwarder.from_array(a, nsym) for a in arrays]
            recompress(fw)
            seen.append((fw, _capi.last_training()))
    finally:
        set_device_training(0)
        set_device_encoding(0)
        _capi.check(L.imc_dictionary_reset())
    (fw0, how0), (fw1, how1) = seen
    assert how0["path"] == 0 and how1["path"] == 1, (what, how0, how1)
    assert how0["symbols"] == how1["symbols"] and how0["attempts"] == how1["attempts"] and how0["rounds"] == how1["rounds"], (what, how0, how1)
    for k, (a, b) in enumerate(zip(fw0, fw1)):
        assert a.sym2pair == b.sym2pair, (what, k)
        assert_same_chunk(a, b, (what, k))
    return fw0, fw1, how1


def ragged_arrays():
    """Seven chunks of 3 000 to 400 000 columns (one below the 4096 columns a chunk needs to be compressed at all)."""
    return [compressible(n, seed=60 + k) for k, n in enumerate((40_000, 5_000, 400_000, 3_000, 33_333, 120_001, 8_191))]


def many_small_arrays():
    """70 chunks of 5000 columns: none trains a dictionary on its own, the sample is 70 heads."""
    return [compressible(5_000, seed=200 + k) for k in range(70)]


def guard_cases():
    """What the guard-mode child runs (IMC_GUARD=1: every buffer flush against an unmapped range)."""
    for name, obs, nsym in small_cases():
        trained_both_ways(lambda: Forwarder.from_array(obs, nsym), name)
        print("ok", name, flush=True)
    fw0, fw1, how = recompressed_both_ways(many_small_arrays(), 3, "70 chunks")
    assert len(fw1[0].sym2pair) > 8 and how["symbols"] == 70 * 5000
    print("recompress ok", flush=True)


def device_path_cases(torch, oracle, tol=1e-11):
    """The creations whose symbols are on the device already - Forwarder.from_device (uint8; int16 with 257 symbols) and
    Forwarder.from_sequences - as the training creation with the device trainer, against the host path from the same
    symbols; then one evaluation at 10 states of a host-trained and a device-trained chunk: bit-equal, and within `tol`
    relative of the CPU oracle.  Called from a process that imported torch before the library."""
    from imcoalhmm_amd import prepare, synth
    from imcoalhmm_amd.hmm import forward_chunks_batch
    L = _capi.lib()
    dev = torch.device("cuda")

    def other_way(reference, make, what):
        try:
            _capi.check(L.imc_dictionary_reset())
            set_device_training(1)
            f = make()
            how = _capi.last_training()
        finally:
            set_device_training(0)
            _capi.check(L.imc_dictionary_reset())
        assert how["path"] == 1, (what, how)
        assert f.sym2pair == reference.sym2pair and len(f.sym2pair) > 8, what
        assert_same_chunk(reference, f, what)
        return f

    def host_trained(obs, nsym):
        _capi.check(L.imc_dictionary_reset())
        set_device_training(0)
        f = Forwarder.from_array(obs, nsym)
        assert _capi.last_training()["path"] == 0
        return f

    obs3 = compressible(70_001, seed=21)
    host3 = host_trained(obs3, 3)
    f8 = other_way(host3, lambda: Forwarder.from_device(torch.from_numpy(obs3).to(dev), 3), "uint8 tensor")
    pi, T, E = synth.random_hmm(10, 3, seed=310, stay=0.97)
    got = forward_chunks_batch([host3.handle, f8.handle], pi[None], T[None], E[None], per_chunk=True)[0]
    want = oracle.forward_scaled(pi, T, E, obs3)
    assert got[0] == got[1] and abs(got[1] - want) / abs(want) < tol, (got, want)
    print("uint8 ok", flush=True)

    obs257 = skewed_symbols(60_000, 257, seed=33)
    host257 = host_trained(obs257, 257)
    other_way(host257, lambda: Forwarder.from_device(torch.from_numpy(obs257.astype(np.int16)).to(dev), 257), "int16 tensor")
    print("int16 ok", flush=True)

    rng = np.random.default_rng(8)
    s1 = rng.choice(list(b"ACGT"), size=50_000).astype(np.uint8)
    s2 = s1.copy()
    change = rng.random(s1.size) < 0.08
    s2[change] = rng.choice(list(b"ACGT"), size=int(change.sum())).astype(np.uint8)
    s2[rng.random(s1.size) < 0.02] = ord("N")
    a, b = s1.tobytes().decode("ascii"), s2.tobytes().decode("ascii")
    host_pair = host_trained(prepare.encode_pairwise(a, b), 3)
    other_way(host_pair, lambda: Forwarder.from_sequences(a, b), "sequence pair")
    print("pairwise ok", flush=True)
