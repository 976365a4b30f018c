"""Device ingestion (csrc/kernels_ingest.hpp) against the host parser (csrc/obs_io.hpp) on the GPU: the same file opened
with imc_set_device_ingest(0) and (1) gives the same length, the same raw symbols and the same chunk at every level, and
imc_last_ingest proves that the device path ran, in the slabs the slab rule gives - for text across tile (4096 bytes) and
slab boundaries, for the three cache layouts, and for the pairwise rule of Forwarder.from_sequences.  Every error has the
host parser's code and message.  The oracle of the symbol comparisons is the host parser itself; log-likelihoods are
additionally held to the CPU oracle at the suite's 1e-11."""
import ctypes
import os
import struct
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from device_encode_cases import assert_same_chunk, compressible, skewed_symbols, train3
from device_ingest_cases import (assert_same_error, assert_same_file, open_both, raw_symbols, slab_bytes, small_cases, text_of)
from imcoalhmm_amd import Forwarder, _capi, prepare, synth
from imcoalhmm_amd.hmm import forward_chunks_batch, set_device_encoding, set_device_ingest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-11
MAGIC = b"IMCOBS1\n"
_state = {}


@pytest.fixture(autouse=True)
def _restore_switches():
    L = _capi.lib()
    assert L.imc_device_count() >= 1, "gpu tests need a device"
    try:
        yield
    finally:
        set_device_ingest(0)
        set_device_encoding(0)
        _capi.check(L.imc_set_compression(1))
        os.environ.pop("IMC_INGEST_SLAB_BYTES", None)


@pytest.fixture
def dictionary3():
    """The 3-symbol dictionary of device_encode_cases.train3, so that chunks of every length get token streams; trained
    again only if another test has reset it."""
    if "f" in _state:
        probe = Forwarder.from_array(np.zeros(4096, dtype=np.uint8), 3)
        if probe.sym2pair == _state["f"].sym2pair:
            return _state["alpha"]
    _state["f"], _state["alpha"] = train3()
    return _state["alpha"]


def _write(tmp_path, name, data):
    path = tmp_path / name
    path.write_bytes(data)
    return str(path)


# ---- text ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slab", [None, 4096, 4097, 10000])
def test_reference_format_three_symbols(tmp_path, dictionary3, slab):
    for n in (1, 2, 4095, 4096, 4097, 8193, 65537):
        obs = compressible(n, seed=100 + n)
        path = _write(tmp_path, "t%d.ziphmm" % n, text_of(obs))
        a, b = assert_same_file(path, 3, slab, "text", obs)
        if n >= 4096:
            assert b.compressed_length(16384)[1] == dictionary3, n      # the chunk went through the whole dictionary


@pytest.mark.parametrize("nsym", [65, 257])
def test_tokens_of_one_to_three_digits_across_tiles(tmp_path, nsym):
    """65 and 257 symbols: tokens of 1 to 3 digits, so token starts, digit runs and separators fall on every offset of a
    tile boundary; 257 symbols are 16-bit symbols on the device.  The first file trains the alphabet's dictionary."""
    L = _capi.lib()
    _capi.check(L.imc_dictionary_reset())
    _state.clear()
    trainer = skewed_symbols(60_000, nsym, seed=nsym)
    path = _write(tmp_path, "train.ziphmm", text_of(trainer))
    a, b = assert_same_file(path, nsym, None, "text", trainer)
    assert b.compressed_length(16384)[1] > nsym
    for n, slab in ((9001, None), (9001, 4096), (4099, 4097)):
        obs = skewed_symbols(n, nsym, seed=7 + n)
        path = _write(tmp_path, "w%d.ziphmm" % n, text_of(obs))
        assert_same_file(path, nsym, slab, "text", obs)
    _capi.check(L.imc_dictionary_reset())


@pytest.mark.parametrize("slab", [None, 4096])
def test_separators_and_edges(tmp_path, dictionary3, slab):
    rng = np.random.default_rng(11)
    seps = [b" ", b"\n", b"\t", b"\r\n", b"  ", b" \n\t\r\n", b"\f", b"\v ", b"\n" * 9]
    obs = compressible(9000, seed=12)
    mixed = b"".join(b"%d" % int(v) + seps[k] for v, k in zip(obs, rng.integers(0, len(seps), size=obs.size)))
    files = {
        "mixed": (mixed, obs),
        "leading": (b" \n\t  " + text_of(obs[:5000]), obs[:5000]),
        "no_trailing": (text_of(obs[:4097]).rstrip(), obs[:4097]),
        "no_trailing_one": (b"2", [2]),
        "zeros_in_front": (b"007 0 01 002", None),
        "empty": (b"", []),
        "whitespace_only": (b" \n\t\r\n  " * 700, []),
    }
    for name, (data, want) in files.items():
        assert_same_file(_write(tmp_path, name + ".ziphmm", data), 20 if name == "zeros_in_front" else 3, slab, "text", want, what=(name, slab))
    a, _, _ = open_both(_write(tmp_path, "seven.ziphmm", b"007 0 01 002"), 20)
    assert raw_symbols(a).tolist() == [7, 0, 1, 2]


def test_a_twenty_digit_token_is_declined(tmp_path, dictionary3):
    """The device parser does not evaluate digit runs beyond 16: the file is parsed by the host parser from its start
    (path "host"), with the same symbols - also when the run lies in a later slab than symbols already parsed."""
    obs = compressible(6000, seed=3)
    data = text_of(obs) + b"00000000000000000002 1 " + text_of(obs[:100])
    want = np.concatenate([obs, [2, 1], obs[:100]])
    for slab in (None, 4096):
        a, b, how = open_both(_write(tmp_path, "long.ziphmm", data), 3, slab)
        assert how == {"path": "host", "bytes": 0, "slabs": 0, "columns": want.size}, how
        assert (raw_symbols(a) == want).all() and (raw_symbols(b) == want).all()
        assert_same_chunk(a, b, ("declined", slab))
    # sixteen digits are parsed on the device
    _, b16, how = open_both(_write(tmp_path, "sixteen.ziphmm", b"0 0000000000000002 1"), 3)
    assert how["path"] == "text" and raw_symbols(b16).tolist() == [0, 2, 1]
    # a slab without any whitespace is declined as well
    solid = b"1 " * 100 + b"0" * 5000 + b" 2"
    a, b, how = open_both(_write(tmp_path, "solid.ziphmm", solid), 3, 4096)
    assert how["path"] == "host" and (raw_symbols(a) == raw_symbols(b)).all() and len(b) == 102


def test_errors_are_the_host_parsers(tmp_path):
    E_IO, E_SYM = _capi.IMC_ERR_IO, _capi.IMC_ERR_SYMBOL
    for k, (data, code) in enumerate([(b"0 1 x 2", E_IO), (b"9", E_SYM), (b"0 1 9", E_SYM), (b"9x", E_IO), (b"x 9", E_IO), (b"9 x", E_SYM),
                                      (b"-1", E_IO), (b"0 1 2 1 7", E_SYM), (b"0 9999999 1", E_SYM), (b"0 12345678901234", E_SYM)]):
        rc, msg, _ = assert_same_error(_write(tmp_path, "e%d.ziphmm" % k, data), 3, None, code)
        if data == b"9 x":
            assert msg == b"symbol 9 at column 0 >= nsym"
        if data in (b"9", b"0 1 9"):
            assert msg == b"symbol 9 >= nsym"                                # at the end of the file: no column
        if data == b"0 9999999 1":
            assert msg == b"symbol 1000000 at column 1 >= nsym"               # the host parser's cap
    base = text_of(compressible(7000, seed=4))                              # 14000 bytes: digits at even offsets, spaces at odd ones
    for offset in (4095, 4096):
        data = bytearray(base)
        data[offset] = ord("x")
        for slab in (None, 4096):
            assert_same_error(_write(tmp_path, "bad%d.ziphmm" % offset, bytes(data)), 3, slab, E_IO)
    third = bytearray(base)
    third[2 * 4096 + 100] = ord("9")                                        # column 4146, in the third slab of 4096 bytes
    rc, msg, _ = assert_same_error(_write(tmp_path, "third.ziphmm", bytes(third)), 3, 4096, E_SYM)
    assert msg == b"symbol 9 at column 4146 >= nsym"
    # file order: the bad byte of the second slab comes before the symbol of the third, and a symbol before a later bad byte
    both = bytearray(third)
    both[4096 + 51] = ord("?")
    assert_same_error(_write(tmp_path, "both.ziphmm", bytes(both)), 3, 4096, E_IO)
    both = bytearray(third)
    both[2 * 4096 + 103] = ord("?")
    assert_same_error(_write(tmp_path, "both2.ziphmm", bytes(both)), 3, 4096, E_SYM)
    both[2 * 4096 + 101] = ord("?")                                         # "9?": the bad byte ends the digit run and wins
    assert_same_error(_write(tmp_path, "both3.ziphmm", bytes(both)), 3, 4096, E_IO)
    # 257 symbols: 16-bit symbols, a three-digit token that is too large
    assert_same_error(_write(tmp_path, "wide.ziphmm", b"256 0 257 1"), 257, None, E_SYM)


# The slab is cut behind its last whitespace byte, at 8 392 704 bytes here: 2049 tiles, three for each of the threads 0 .. 682
# of the one-workgroup scan, idle threads behind them.
SCAN_SHARES_SLAB = 2 * 1024 * 4096 + 4097


def test_a_slab_of_several_tiles_per_scan_thread(tmp_path, dictionary3):
    """12 MB of text in two slabs: in the first a thread of k_ing_scan owns three consecutive tiles (12288 bytes), in the
    second one.  Then two faults in different threads' shares of the first slab, in both orders: the first one in file
    order is reported, as by the host parser."""
    obs = compressible(6_000_000, seed=77)
    data = np.stack([obs + ord("0"), np.full(obs.size, ord(" "), dtype=np.uint8)], axis=1).tobytes()     # text_of(obs): digits at even offsets
    assert data[:8] == text_of(obs[:4])
    path = _write(tmp_path, "big.ziphmm", data)
    a, b = assert_same_file(path, 3, SCAN_SHARES_SLAB, "text", obs)
    assert _capi.last_ingest()["slabs"] == 2
    assert b.compressed_length(16384)[1] == dictionary3
    share = 3 * 4096
    early, late = 100 * share + 5000, 600 * share + 7000                   # digits in the shares of threads 100 and 600 ...
    assert early < late < SCAN_SHARES_SLAB - 1 and early // share != late // share    # ... both in front of the first slab's cut
    for first, second, code in ((b"9", b"x", _capi.IMC_ERR_SYMBOL), (b"x", b"9", _capi.IMC_ERR_IO)):
        bad = bytearray(data)
        bad[early:early + 1], bad[late:late + 1] = first, second
        rc, msg, _ = assert_same_error(_write(tmp_path, "bad.ziphmm", bytes(bad)), 3, SCAN_SHARES_SLAB, code)
        if first == b"9":
            assert msg == b"symbol 9 at column %d >= nsym" % (early // 2)


# ---- cache --------------------------------------------------------------------------------------------------
def _cache(nsym_file, bits, L, payload):
    return MAGIC + struct.pack("<IIQ", nsym_file, bits, L) + payload


@pytest.mark.parametrize("slab", [None, 4096])
def test_cache_files(tmp_path, dictionary3, slab):
    for n in (1, 3, 4, 5, 4097, 16385):
        obs = compressible(n, seed=200 + n)
        path = str(tmp_path / ("c%d.imc" % n))
        prepare.write_cache(path, obs, 3)
        assert_same_file(path, 3, slab, "cache", obs)
        assert_same_file(path, 300, slab, "cache", obs)                     # a 2-bit payload into 16-bit symbols
    obs65 = skewed_symbols(5000, 65, seed=1).astype(np.uint8)
    path = str(tmp_path / "c65.imc")
    prepare.write_cache(path, obs65, 65)
    assert_same_file(path, 65, slab, "cache", obs65)
    obs257 = skewed_symbols(5000, 257, seed=2)
    path = _write(tmp_path, "c257.imc", _cache(257, 16, obs257.size, obs257.astype("<u2").tobytes()))
    assert_same_file(path, 257, slab, "cache", obs257)
    assert_same_file(_write(tmp_path, "c0.imc", _cache(3, 2, 0, b"")), 3, slab, "cache", [])


def test_cache_errors_are_the_host_parsers(tmp_path):
    obs = compressible(16385, seed=9)
    path = str(tmp_path / "four.imc")
    prepare.write_cache(path, obs, 4)
    assert_same_error(path, 3, None, _capi.IMC_ERR_SYMBOL)                   # an alphabet above nsym
    whole = open(path, "rb").read()
    for slab in (None, 4096):
        assert_same_error(_write(tmp_path, "cut.imc", whole[:-1]), 4, slab, _capi.IMC_ERR_IO)
        assert_same_error(_write(tmp_path, "cut2.imc", whole[:24 + 4096]), 4, slab, _capi.IMC_ERR_IO)
    assert_same_error(_write(tmp_path, "head.imc", whole[:20]), 4, None, _capi.IMC_ERR_IO)
    # symbols that the header's alphabet allows to be written but nsym does not
    pk = bytearray((16385 + 3) // 4)
    pk[4100 // 4] = 3 << (2 * (4100 % 4))
    rc, msg, _ = assert_same_error(_write(tmp_path, "three.imc", _cache(3, 2, 16385, bytes(pk))), 3, 4096, _capi.IMC_ERR_SYMBOL)
    assert msg == b"symbol 3 at column 4100 >= nsym"
    wide = np.zeros(5000, dtype="<u2")
    wide[4999] = 300
    assert_same_error(_write(tmp_path, "wide.imc", _cache(257, 16, 5000, wide.tobytes())), 257, None, _capi.IMC_ERR_SYMBOL)
    bytes65 = np.zeros(5000, dtype=np.uint8)
    bytes65[17] = 65
    assert_same_error(_write(tmp_path, "b65.imc", _cache(65, 8, 5000, bytes65.tobytes())), 65, None, _capi.IMC_ERR_SYMBOL)


# ---- the chunk behind the symbols -----------------------------------------------------------------------------
def test_training_through_the_device_path(tmp_path):
    """The creation that trains the alphabet's dictionary, with the file parsed on the device: only the training head
    travels back; the dictionary and the streams are the host path's."""
    L = _capi.lib()
    obs = compressible(300_000, seed=5)
    path = str(tmp_path / "train.ziphmm")
    prepare.write_text(path, obs)
    try:
        _capi.check(L.imc_dictionary_reset())
        _state.clear()
        host = Forwarder(path, 3)
        _capi.check(L.imc_dictionary_reset())
        set_device_ingest(1)
        with slab_bytes(1 << 18):
            dev = Forwarder(path, 3)
        how = _capi.last_ingest()
    finally:
        set_device_ingest(0)
        _capi.check(L.imc_dictionary_reset())
    assert how == {"path": "text", "bytes": 600_000, "slabs": 3, "columns": 300_000}, how
    assert len(host.sym2pair) > 8 and dev.sym2pair == host.sym2pair
    assert_same_chunk(host, dev, "trained through the device path")


def test_values(tmp_path, dictionary3, example_pairs):
    from oracle import oracle_lib
    oracle_lib.build()
    pi, T, E = synth.random_hmm(10, 3, seed=41, stay=0.97)
    for key, obs in example_pairs.items():
        path = str(tmp_path / (key + ".ziphmm"))
        prepare.write_text(path, obs)
        a, b = assert_same_file(path, 3, 1 << 16, "text", obs, what=key)
        got = forward_chunks_batch([a.handle, b.handle], pi[None], T[None], E[None], per_chunk=True)[0]
        assert got[0] == got[1], (key, got)
        want = oracle_lib.forward_scaled(pi, T, E, obs)
        assert abs(got[1] - want) / abs(want) < TOL, (key, got[1], want)


# ---- pairwise -------------------------------------------------------------------------------------------------
def _sequences(n, seed):
    """Mostly bases of both cases, some gaps and Ns, and every byte value now and then."""
    rng = np.random.default_rng(seed)
    common = np.frombuffer(b"ACGTacgtACGTacgt-Nn", dtype=np.uint8)
    out = []
    for _ in range(2):
        s = rng.choice(common, size=n)
        anything = rng.random(n) < 0.05
        s[anything] = rng.integers(0, 256, size=int(anything.sum()), dtype=np.uint8)
        out.append(bytes(s))
    return out


def test_pairwise_from_sequences(dictionary3):
    L = _capi.lib()
    every = bytes(range(256))
    cases = [_sequences(n, seed=n) for n in (1, 4096, 4097, 70001)]
    cases.append((b"".join(bytes([x]) * 256 for x in range(256)), every * 256))     # all 256 x 256 byte pairs
    for s1, s2 in cases:
        n = len(s1)
        want = np.empty(n, dtype=np.uint8)
        _capi.check(L.imc_encode_pairwise(s1, s2, n, want.ctypes.data_as(_capi._u8p)))
        host = Forwarder.from_array(want, 3)
        for slab in (None, 8192):
            with slab_bytes(slab):
                dev = Forwarder.from_sequences(s1, s2)
                how = _capi.last_ingest()
            pieces = 1 if slab is None else (n + 4095) // 4096
            assert how == {"path": "pairwise", "bytes": 2 * n, "slabs": pieces, "columns": n}, (n, slab, how)
            assert dev.NSYM == 3 and (raw_symbols(dev) == want).all(), (n, slab)
            assert_same_chunk(host, dev, ("pairwise", n, slab))
    text = Forwarder.from_sequences("ACGTN-acgt", "ACCTNAaggt")
    assert raw_symbols(text).tolist() == [0, 0, 1, 0, 2, 2, 0, 1, 0, 0]
    with pytest.raises(ValueError, match="differ in length"):
        Forwarder.from_sequences(b"ACGT", b"ACG")


def test_pairwise_forwarders_from_an_alignment(tmp_path, dictionary3):
    seqs = {"a": "ACGTACGTNN--ACGT" * 300, "b": "ACGTACCTNNA-ACGA" * 300, "c": "acgtacgtnnccacgt" * 300}
    fa = tmp_path / "three.fa"
    fa.write_text("".join(">%s\n%s\n" % kv for kv in seqs.items()))
    before = sorted(os.listdir(str(tmp_path)))
    every = prepare.pairwise_forwarders(str(fa))
    assert list(every) == [("a", "b"), ("a", "c"), ("b", "c")]
    for (x, y), f in every.items():
        assert (raw_symbols(f) == prepare.encode_pairwise(seqs[x], seqs[y])).all(), (x, y)
    only = prepare.pairwise_forwarders(str(fa), pairs=[("c", "a")])
    assert list(only) == [("c", "a")] and len(only[("c", "a")]) == 4800
    assert sorted(os.listdir(str(tmp_path))) == before                      # no intermediate file


ENV_SCRIPT = textwrap.dedent('''
    import sys
    sys.path.insert(0, %r)
    from imcoalhmm_amd import Forwarder, _capi
    f = Forwarder(sys.argv[1], 3)
    print("path", _capi.last_ingest()["path"], len(f), flush=True)
''') % (REPO,)


def test_the_environment_sets_the_switch_at_start_up(tmp_path):
    path = _write(tmp_path, "env.ziphmm", text_of(compressible(5000, seed=8)))
    script = tmp_path / "env_switch.py"
    script.write_text(ENV_SCRIPT)
    for value, want in (("1", "text"), ("0", "host")):
        env = dict(os.environ, IMC_DEVICE_INGEST=value)
        out = subprocess.run([sys.executable, str(script), path], capture_output=True, text=True, timeout=300, env=env)
        assert out.returncode == 0 and "path %s 5000" % want in out.stdout, (value, out.stdout[-500:], out.stderr[-2000:])


# ---- guard pages ----------------------------------------------------------------------------------------------
GUARD_SCRIPT = textwrap.dedent('''
    import sys, tempfile
    sys.path.insert(0, %r)
    sys.path.insert(0, %r)
    from device_encode_cases import train3
    from device_ingest_cases import small_cases
    train3()
    with tempfile.TemporaryDirectory() as tmp:
        small_cases(tmp)
    print("ingest ok", flush=True)
''') % (REPO, os.path.join(REPO, "tests"))


def test_device_ingest_under_guard_pages(tmp_path, dictionary3):
    """Slabs, tile tables, the symbol buffer and the chunk's own buffer flush against an unmapped page: the cases run here
    first, then once more in a process with IMC_GUARD=1."""
    small_cases(str(tmp_path))
    script = tmp_path / "guard_ingest.py"
    script.write_text(GUARD_SCRIPT)
    env = dict(os.environ, IMC_GUARD="1")
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    tail = (out.stdout[-1500:], out.stderr[-3000:])
    if "hipMemAddressReserve" in out.stderr or "hipMemCreate" in out.stderr or "hipMemGetAllocationGranularity" in out.stderr:
        pytest.skip("HIP virtual-memory management is unavailable on this box: %r" % (tail,))
    assert out.returncode == 0 and "ingest ok" in out.stdout, tail
