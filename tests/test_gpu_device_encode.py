"""The device encoder (csrc/kernels_encode.hpp) against the host encoder (imc::encode_levels) on the GPU: the same tokens,
token counts and lengths at every level of the dictionary, exactly - across tile boundaries (4096 elements), for runs far
longer than a tile and than the 1024 tiles one thread each of the scan takes, for byte merges, 16-bit rounds and 16-bit
raw streams - and the entry points built on it:
Forwarder.from_device, imc_obs_token_counts, the batched imc_obs_recompress.  The oracle of the token comparisons is the
host encoder itself; log-likelihoods are additionally held to the CPU oracle at the suite's 1e-11."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from device_encode_cases import CONTENTS, LENGTHS, assert_same_chunk, compressible, content, host_and_device, skewed_symbols, train3
from imcoalhmm_amd import Forwarder, _capi, synth
from imcoalhmm_amd.hmm import forward_chunks_batch, recompress, set_device_encoding

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_state = {}


@pytest.fixture(autouse=True)
def _restore_switches():
    L = _capi.lib()
    assert L.imc_device_count() >= 1, "gpu tests need a device"
    try:
        yield
    finally:
        set_device_encoding(0)
        _capi.check(L.imc_set_compression(1))
        _capi.check(L.imc_set_table_streaming(-1))
        _capi.check(L.imc_set_blocked_kernel(4))


def _dictionary(nsym):
    """One host-trained dictionary per alphabet for the module; trained again only if another test has reset it."""
    L = _capi.lib()
    set_device_encoding(0)
    _capi.check(L.imc_set_compression(1))
    if nsym in _state:
        probe = Forwarder.from_array(np.zeros(4096, dtype=np.uint8 if nsym <= 256 else np.int32), nsym)
        if probe.sym2pair == _state[nsym][0].sym2pair:
            return _state[nsym]
    if nsym == 3:
        _state[3] = train3()
    else:
        _capi.check(L.imc_dictionary_reset())
        _state.pop(3, None)
        f = Forwarder.from_array(skewed_symbols(60_000, nsym, seed=nsym), nsym)
        alpha = f.compressed_length(16384)[1]
        assert alpha > nsym, alpha                                        # the sample did compress
        _state[nsym] = (f, alpha)
    return _state[nsym]


@pytest.mark.parametrize("kind", CONTENTS)
def test_same_tokens_three_symbols(kind):
    _, alpha = _dictionary(3)
    for n in LENGTHS:
        obs = content(kind, n)
        if obs is None:                                                   # (a single 1 at a column this length does not have)
            continue
        a, b = host_and_device(obs, 3)
        assert a.compressed_length(16384)[1] == alpha, (kind, n)          # the chunks did go through the whole dictionary
        assert_same_chunk(a, b, (kind, n))


SCAN_SHARES_N = 2 * 1024 * 4096 + 4097       # 2050 tiles: three per thread of the one-workgroup scan, a ragged last share, idle threads behind it


@pytest.mark.parametrize("kind", ["compressible", "zeros"])
def test_same_tokens_several_tiles_per_scan_thread(kind):
    """Beyond 1024 tiles a thread of k_enc_scan owns several consecutive tiles; with zeros the carry crosses every tile
    and every share boundary."""
    _, alpha = _dictionary(3)
    a, b = host_and_device(content(kind, SCAN_SHARES_N), 3)
    assert a.compressed_length(16384)[1] == alpha
    assert_same_chunk(a, b, (kind, SCAN_SHARES_N))


@pytest.mark.parametrize("nsym", [65, 257])
def test_same_tokens_large_alphabets(nsym):
    """65 symbols: byte merges on a byte stream (a 60000-column sample ends this dictionary inside the byte phase, at 125
    tokens; byte merges followed by rounds are the 3-symbol cases); 257 symbols: rounds on a 16-bit raw stream."""
    L = _capi.lib()
    trainer, alpha = _dictionary(nsym)
    for n, seed in ((60_000, nsym), (4099, 7)):
        obs = skewed_symbols(n, nsym, seed=seed)
        a, b = host_and_device(obs, nsym)
        assert a.compressed_length(16384)[1] == alpha
        assert_same_chunk(a, b, (nsym, n))
    # the creation that trains the dictionary, with the device encoding the chunk: same dictionary, same streams
    try:
        _capi.check(L.imc_dictionary_reset())
        _state.clear()
        set_device_encoding(1)
        again = Forwarder.from_array(skewed_symbols(60_000, nsym, seed=nsym), nsym)
    finally:
        set_device_encoding(0)
    assert again.sym2pair == trainer.sym2pair
    assert_same_chunk(trainer, again, (nsym, "trained with the switch on"))


FROM_DEVICE_SCRIPT = textwrap.dedent('''
    import sys
    sys.path.insert(0, %r)
    sys.path.insert(0, %r)
    import torch                                   # torch first: its bundled HIP runtime must be the one that initialises
    from device_encode_cases import from_device_cases
    from oracle import oracle_lib
    oracle_lib.build()
    from_device_cases(torch, oracle_lib)
    print("from_device ok", flush=True)
''') % (REPO, os.path.join(REPO, "tests"))


def test_from_device(tmp_path):
    """Forwarder.from_device on torch tensors (uint8 and int32 with 3 symbols, int16 with 257): device_encode_cases.
    from_device_cases, in a child process that imports torch before the library (one HIP runtime per process)."""
    script = tmp_path / "from_device.py"
    script.write_text(FROM_DEVICE_SCRIPT)
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "from_device ok" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])


def test_recompress_batched_on_the_device():
    L = _capi.lib()
    arrays = [compressible(n, seed=40 + k) for k, n in enumerate((40_000, 4096, 100, 7, 70_000))]
    pi, T, E = synth.random_hmm(20, 3, seed=2020, stay=0.97)
    seen = []
    try:
        for switch in (0, 1):
            _capi.check(L.imc_dictionary_reset())
            _state.clear()
            set_device_encoding(switch)
            fw = [Forwarder.from_array(a, 3) for a in arrays]
            recompress(fw)
            per = forward_chunks_batch([f.handle for f in fw], pi[None], T[None], E[None], per_chunk=True)[0]
            seen.append((fw, per))
    finally:
        set_device_encoding(0)
        _capi.check(L.imc_dictionary_reset())
    (fw0, per0), (fw1, per1) = seen
    assert fw0[0].sym2pair == fw1[0].sym2pair and len(fw0[0].sym2pair) > 8
    for k, (a, b) in enumerate(zip(fw0, fw1)):
        assert a.sym2pair == b.sym2pair, k
        assert_same_chunk(a, b, ("recompress", k))
        assert per0[k] == per1[k], (k, per0[k], per1[k])
    for k in (2, 3):
        assert fw1[k].compressed_length(16384) == (arrays[k].size, 3)     # the two short chunks are still raw
    assert fw1[0].compressed_length(16384)[0] < 40_000 // 4


def test_recompress_batched_several_tiles_per_scan_thread():
    """Three chunks in one run of passes, 2052 tiles at the start: the chunk-start scan (k_enc_mark_*) and the passes'
    scan both give a thread several tiles."""
    L = _capi.lib()
    arrays = [compressible(n, seed=60 + k) for k, n in enumerate((4_200_000, 4096, 4_200_000))]
    seen = []
    try:
        for switch in (0, 1):
            _capi.check(L.imc_dictionary_reset())
            _state.clear()
            set_device_encoding(switch)
            fw = [Forwarder.from_array(a, 3) for a in arrays]
            recompress(fw)
            seen.append(fw)
    finally:
        set_device_encoding(0)
        _capi.check(L.imc_dictionary_reset())
    for k, (a, b) in enumerate(zip(*seen)):
        assert a.sym2pair == b.sym2pair and len(a.sym2pair) > 8, k
        assert_same_chunk(a, b, ("recompress", k))
    assert seen[1][0].compressed_length(16384)[0] < 4_200_000 // 4


GUARD_SCRIPT = textwrap.dedent('''
    import sys
    sys.path.insert(0, %r)
    sys.path.insert(0, %r)
    import numpy as np
    import torch
    from device_encode_cases import CONTENTS, assert_same_chunk, compressible, content, host_and_device, train3
    from imcoalhmm_amd import Forwarder
    _, alpha = train3()
    for kind in CONTENTS:
        for n in (4096, 4097, 8193):
            obs = content(kind, n)
            if obs is None:
                continue
            a, b = host_and_device(obs, 3)
            assert a.compressed_length(16384)[1] == alpha
            assert_same_chunk(a, b, (kind, n))
    print("encode ok", flush=True)
    obs = compressible(8193, seed=3)
    f = Forwarder.from_device(torch.from_numpy(obs).to("cuda"), 3)
    assert_same_chunk(Forwarder.from_array(obs, 3), f, "from_device")
    print("from_device ok", flush=True)
''') % (REPO, os.path.join(REPO, "tests"))


def test_device_encoder_under_guard_pages(tmp_path):
    """Every buffer of the encoder - scratch streams, tile tables, level buffers - flush against an unmapped page."""
    script = tmp_path / "guard_encode.py"
    script.write_text(GUARD_SCRIPT)
    env = dict(os.environ, IMC_GUARD="1")
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    tail = (out.stdout[-1500:], out.stderr[-3000:])
    if "hipMemAddressReserve" in out.stderr or "hipMemCreate" in out.stderr or "hipMemGetAllocationGranularity" in out.stderr:
        pytest.skip("HIP virtual-memory management is unavailable on this box: %r" % (tail,))
    assert out.returncode == 0 and "encode ok" in out.stdout and "from_device ok" in out.stdout, tail
