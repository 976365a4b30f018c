"""The device trainer (csrc/kernels_train.hpp, imc_set_device_training) against the host trainer (imc::train_dictionary)
on the GPU: from the same symbols the same dictionary, entry for entry - and therefore the same chunk at every level -
for the byte phase (to 256 entries and short of them, on streams that collapse to a handful of elements, with near-ties
throughout, with the retry loop firing), the 16-bit rounds (on byte-level tokens and on 16-bit raw symbols), under
IMC_DICT_MAX_DEPTH and IMC_DICT_MIN_COUNT, for the joint sample of imc_obs_recompress, and for the creations whose symbols
never were on the host.  The oracle of the dictionary comparisons is the host trainer itself; log-likelihoods are
additionally held to the CPU oracle at the suite's 1e-11."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from device_encode_cases import compressible, skewed_symbols
from device_training_cases import (RETRY_RECIPE, many_small_arrays, periodic, ragged_arrays, recompressed_both_ways, small_cases,
                                   trained_both_ways)
from imcoalhmm_amd import Forwarder, _capi
from imcoalhmm_amd.hmm import set_device_encoding, set_device_training

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _restore_switches():
    L = _capi.lib()
    assert L.imc_device_count() >= 1, "gpu tests need a device"
    try:
        yield
    finally:
        set_device_training(0)
        set_device_encoding(0)
        _capi.check(L.imc_set_compression(1))
        _capi.check(L.imc_dictionary_reset())


def _both(obs, nsym, what, device_encoding=0):
    return trained_both_ways(lambda: Forwarder.from_array(obs, nsym), what, device_encoding)


def test_byte_phase_fills_and_rounds_run():
    a, b, how = _both(compressible(3_000_000, seed=5), 3, "3e6 columns", device_encoding=1)
    assert b.compressed_length(16384)[1] > 1024                          # (as device_encode_cases.train3)
    assert how["attempts"] == 1 and how["rounds"] >= 13 and how["symbols"] == 3_000_000


@pytest.mark.parametrize("name", [c[0] for c in small_cases()])
def test_small_samples(name):
    """40 000 columns: the byte phase stops on its threshold below 256 entries and no round runs; all-equal, alternating
    and period-3 streams collapse to a handful of elements (shorter than a tile, then too short for any pair to reach
    the threshold); 1000 symbols: no byte phase, rounds on the raw 16-bit stream."""
    (obs, nsym), = [(c[1], c[2]) for c in small_cases() if c[0] == name]
    a, b, how = _both(obs, nsym, name)
    alphabet = b.compressed_length(16384)[1]
    if nsym == 1000:
        assert how["attempts"] == 0 and how["rounds"] >= 1 and alphabet > 1000
    else:
        assert how["attempts"] == 1 and how["rounds"] == 0 and nsym < alphabet < 192


def test_exactly_the_training_minimum():
    obs = compressible(32_768, seed=5)
    a, b, how = _both(obs, 3, "32768 columns")
    assert how["symbols"] == 32_768 and b.compressed_length(16384)[1] > 3
    try:                                                                 # one column fewer trains nothing, on either path
        set_device_training(1)
        f = Forwarder.from_array(obs[:-1], 3)
    finally:
        set_device_training(0)
    assert f.compressed_length(16384) == (32_767, 3)


def test_near_ties():
    obs = np.random.default_rng(4).integers(0, 4, size=200_000).astype(np.uint8)
    _both(obs, 4, "uniform over 4 symbols")


@pytest.mark.parametrize("nsym", [65, 257])
def test_large_alphabets(nsym):
    a, b, how = _both(skewed_symbols(60_000, nsym, seed=nsym), nsym, "nsym %d" % nsym)
    assert (how["attempts"] == 0) == (nsym > 256)


def test_retry_loop():
    """RETRY_RECIPE = skewed_symbols(40 000, 190, seed=190): 190 raw symbols leave the byte phase 66 entries, and with
    threshold 64 it stops inside 192..255 (found on the CPU with a stand-alone program around train_dictionary: 2
    attempts, 862 tokens after 10 rounds), so the host trains again with threshold 8; the device continues its run."""
    n, nsym, seed = RETRY_RECIPE
    a, b, how = _both(skewed_symbols(n, nsym, seed=seed), nsym, "retry")
    assert how["attempts"] > 1 and how["rounds"] >= 1, how


@pytest.mark.parametrize("variable,value,data", [("IMC_DICT_MAX_DEPTH", "3", "400000 columns"), ("IMC_DICT_MIN_COUNT", "2", "400000 columns"),
                                                 ("IMC_DICT_MIN_COUNT", "2", "retry recipe")])
def test_experiment_variables_are_read_at_every_training(variable, value, data):
    """(The forced count only bears on the 16-bit rounds, and 400 000 of these columns end inside the byte phase - the
    host trainer gives 99 tokens - so it is also set on the retry recipe, whose training runs 10 rounds.)"""
    if data == "retry recipe":
        n, nsym, seed = RETRY_RECIPE
        obs = skewed_symbols(n, nsym, seed=seed)
    else:
        obs, nsym = compressible(3_000_000, seed=5)[:400_000], 3
    plain = _both(obs, nsym, data)[0].sym2pair
    old = os.environ.get(variable)
    try:
        os.environ[variable] = value
        a, b, how = _both(obs, nsym, "%s=%s, %s" % (variable, value, data))
    finally:
        if old is None:
            del os.environ[variable]
        else:
            os.environ[variable] = old
    if variable == "IMC_DICT_MAX_DEPTH" or data == "retry recipe":
        assert b.sym2pair != plain                                       # the variable did change the training


def test_recompress_ragged_chunks():
    arrays = ragged_arrays()
    fw0, fw1, how = recompressed_both_ways(arrays, 3, "ragged")
    assert how["symbols"] == sum(a.size for a in arrays if a.size >= 4096)   # every chunk is shorter than its share: the sample is all of them
    assert fw1[3].compressed_length(16384) == (3_000, 3)                 # under 4096 columns: left alone
    assert len(fw1[0].sym2pair) > 100                                    # (the joint dictionary: 145 tokens)


def test_recompress_many_small_chunks():
    fw0, fw1, how = recompressed_both_ways(many_small_arrays(), 3, "70 chunks")
    assert how["symbols"] == 70 * 5000 and len(fw1[0].sym2pair) > 8


DEVICE_PATHS_SCRIPT = textwrap.dedent('''
    import sys
    sys.path.insert(0, %r)
    sys.path.insert(0, %r)
    import torch                                   # torch first: its bundled HIP runtime must be the one that initialises
    from device_training_cases import device_path_cases
    from oracle import oracle_lib
    oracle_lib.build()
    device_path_cases(torch, oracle_lib)
    print("device paths ok", flush=True)
''') % (REPO, os.path.join(REPO, "tests"))


def test_device_resident_and_ingest_paths(tmp_path):
    """Forwarder.from_device (uint8; int16 with 257 symbols) and Forwarder.from_sequences as the training creation:
    device_training_cases.device_path_cases, in a child process that imports torch before the library."""
    script = tmp_path / "device_paths.py"
    script.write_text(DEVICE_PATHS_SCRIPT)
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "device paths ok" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])


GUARD_SCRIPT = textwrap.dedent('''
    import sys
    sys.path.insert(0, %r)
    sys.path.insert(0, %r)
    from device_training_cases import guard_cases
    guard_cases()
    print("guard ok", flush=True)
''') % (REPO, os.path.join(REPO, "tests"))


def test_device_trainer_under_guard_pages(tmp_path):
    """Every buffer of the trainer - streams, tile tables, pair bins, the counting table, the candidate list, the device
    dictionary - flush against an unmapped range; IMC_DEBUG_HOST shows that the recompression with both switches on
    copied no symbols back."""
    script = tmp_path / "guard_training.py"
    script.write_text(GUARD_SCRIPT)
    env = dict(os.environ, IMC_GUARD="1", IMC_DEBUG_HOST="1")
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    tail = (out.stdout[-1500:], out.stderr[-3000:])
    if "hipMemAddressReserve" in out.stderr or "hipMemCreate" in out.stderr or "hipMemGetAllocationGranularity" in out.stderr:
        pytest.skip("HIP virtual-memory management is unavailable on this box: %r" % (tail,))
    assert out.returncode == 0 and "guard ok" in out.stdout and "recompress ok" in out.stdout, tail
    lines = [l for l in out.stderr.splitlines() if l.startswith("[imc host] recompress 70 chunks")]
    assert len(lines) == 2, tail
    assert "host trainer" in lines[0] and " 0 symbol bytes to the host" not in lines[0], lines
    assert "device trainer, 0 symbol bytes to the host" in lines[1], lines
