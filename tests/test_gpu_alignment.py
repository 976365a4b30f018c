"""Resident alignments (csrc/kernels_align.hpp) on the GPU.  An Alignment opened on the device holds the names and
sequences prepare.read_fasta gives, in the slabs the slab rule gives, across tile (4096 bytes) and slab boundaries, wrapped
and unwrapped, with "\n" and "\r\n"; every file the device parser declines goes through the host reader with the same
result, and the two error files with the host reader's code and message.  A chunk built from resident sequences - pairs and
triplets, record starts at every residue mod 4 - has the host encoders' symbols and is, at every level, the chunk
Forwarder.from_array builds from them.  Every comparison is exact."""
import ctypes
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from alignment_cases import assert_chunk, assert_parsed, bases, fasta, host_symbols, small_cases
from device_encode_cases import assert_same_chunk, train3
from device_ingest_cases import raw_symbols, slab_bytes
from imcoalhmm_amd import Alignment, Forwarder, _capi, prepare, synth
from imcoalhmm_amd.hmm import forward_chunks_batch, set_device_encoding, set_device_ingest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLABS = (None, 4096)
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


@pytest.fixture
def dictionary65():
    """A 65-symbol dictionary trained on the triplet symbols of three related sequences, so that triplet chunks get token
    streams; trained again only if another test has reset it."""
    if "f65" in _state:
        probe = Forwarder.from_array(np.zeros(4096, dtype=np.uint8), 65)
        if probe.sym2pair == _state["f65"].sym2pair:
            return _state["alpha65"]
    rng = np.random.default_rng(65)
    a = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=200_000)
    b, c = a.copy(), a.copy()
    for s, rate in ((b, 0.02), (c, 0.05)):
        flip = rng.random(s.size) < rate
        s[flip] = rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=int(flip.sum()))
    _capi.check(_capi.lib().imc_dictionary_reset())
    _state.pop("f", None)                                               # (the reset forgets every alphabet's dictionary)
    f = Forwarder.from_array(host_symbols([bytes(a), bytes(b), bytes(c)]), 65)
    _state["f65"], _state["alpha65"] = f, f.compressed_length(16384)[1]
    assert _state["alpha65"] > 65
    return _state["alpha65"]


def _write(tmp_path, name, data):
    path = tmp_path / name
    path.write_bytes(data)
    return str(path)


# ---- parse equals specification -------------------------------------------------------------------------------
def _three(n=4097):
    return [(b"s%d" % k, bases(n, seed=40 + k)) for k in range(3)]


def _second_header_at(offset, header=b"b"):
    """Two records; the '>' of the second one stands at byte `offset` of the file."""
    first = bases(offset - 4, seed=offset)
    data = fasta([(b"a", first)], wrap=None) + fasta([(header, bases(300, seed=offset + 1))], wrap=70)
    assert data[offset:offset + 1] == b">" and data.count(b">") == 2
    return data


PARSE_FILES = {
    "wrapped at 60": lambda: fasta(_three(), wrap=60),
    "wrapped at 61": lambda: fasta(_three(), wrap=61),
    "unwrapped": lambda: fasta(_three(), wrap=None),
    "unwrapped, longer than two slabs": lambda: fasta(_three(9001), wrap=None),
    "crlf wrapped at 60": lambda: fasta(_three(), wrap=60, eol=b"\r\n"),
    "crlf wrapped at 61": lambda: fasta(_three(), wrap=61, eol=b"\r\n"),
    "crlf unwrapped": lambda: fasta(_three(), wrap=None, eol=b"\r\n"),
    "second header at 4095": lambda: _second_header_at(4095),
    "second header at 4096": lambda: _second_header_at(4096),
    "second header at 4097": lambda: _second_header_at(4097),
    "header line straddles 4096": lambda: _second_header_at(4090, b"b a description that crosses the boundary"),
    "empty lines between records": lambda: b"\n" + fasta(_three(500)[:1], wrap=60) + b"\n\n" + fasta(_three(500)[1:2], wrap=60) + b"\r\n\n" + fasta(_three(500)[2:]),
    "no final newline": lambda: fasta(_three(5000), wrap=60, final=False),
    "no final newline, header last": lambda: fasta(_three(100), wrap=60) + b">last",
    "one-base record": lambda: fasta([(b"a", b"A"), (b"b", bases(4200, seed=3)), (b"c", b"g")], wrap=60),
    "empty record": lambda: fasta([(b"a", b""), (b"b", bases(4200, seed=4)), (b"c", b""), (b"d", b"")], wrap=60),
    "lines in front of the first header": lambda: b"#comment\nACGT\n\n" + fasta(_three(4097), wrap=60),
    "descriptions": lambda: fasta([(b"a\tdesc one", bases(50, 1)), (b"b  two words", bases(50, 2))], wrap=20),
    "empty file": lambda: b"",
}


@pytest.mark.parametrize("slab", SLABS)
@pytest.mark.parametrize("name", sorted(PARSE_FILES))
def test_device_parse_is_read_fasta(tmp_path, name, slab):
    path = _write(tmp_path, "p.fa", PARSE_FILES[name]())
    assert_parsed(path, slab, "device").close()


def test_device_parse_with_several_tiles_per_scan_thread(tmp_path):
    """12 MB in two slabs: the first is cut at its last line end (2049 tiles, the last one short), so each of the threads
    0 .. 682 of k_aln_scan owns three consecutive tiles, the threads behind them none, and record boundaries fall inside
    such shares."""
    data = fasta([(b"s%d" % k, bases(2_950_000, seed=60 + k)) for k in range(4)], wrap=60)
    aln = assert_parsed(_write(tmp_path, "big.fa", data), 2 * 1024 * 4096 + 4097, "device")
    assert aln.info["slabs"] == 2 and aln.info["records"] == 4
    aln.close()


# ---- declines fall back, identically -----------------------------------------------------------------------------
def _spoiled(at, byte):
    data = bytearray(fasta(_three(3000), wrap=60))
    assert chr(data[at]) not in ">\n"
    data[at:at + 1] = byte
    return bytes(data)


DECLINED = {
    "a blank in a sequence line": lambda: _spoiled(5000, b" "),
    "a tab at the end of a sequence line": lambda: fasta(_three(3000), wrap=60).replace(b"\n", b"\t\n", 3),
    "a control byte in a sequence line": lambda: _spoiled(7000, b"\x01"),
    "a lone carriage return": lambda: _spoiled(4500, b"\r"),
    "whitespace in front of a header": lambda: fasta(_three(3000), wrap=60).replace(b">s1", b" >s1"),
    "more records than the cap": lambda: fasta([(b"r%d" % k, b"ACGT") for k in range(4097)]),
    "a repeated name": lambda: fasta(_three(3000) + [(b"s1", bases(3000, seed=9))], wrap=60),
    "a header line longer than a slab": lambda: fasta([(b"a " + b"d" * 5000, bases(100, 1)), (b"b", bases(100, 2))]),
}


@pytest.mark.parametrize("name", sorted(DECLINED))
def test_declined_files_go_through_the_host_reader(tmp_path, name):
    slab = 4096 if name == "a header line longer than a slab" else None
    path = _write(tmp_path, "d.fa", DECLINED[name]())
    assert_parsed(path, slab, "host").close()
    if slab:                                                             # ... and fits a slab of the default size
        assert_parsed(path, None, "device").close()


@pytest.mark.parametrize("data, needle", [(fasta(_three(3000), wrap=60).replace(b">s2", b">"), b"header without a name"),
                                          (fasta(_three(3000), wrap=60)[:6000] + b"\xe9" + fasta(_three(3000), wrap=60)[6001:], b"non-ASCII byte")])
def test_error_files_have_the_host_readers_code_and_message(tmp_path, data, needle):
    L = _capi.lib()
    path = os.fsencode(_write(tmp_path, "e.fa", data))
    count, length, h = ctypes.c_int(0), ctypes.c_size_t(0), ctypes.c_void_p()
    want = (L.imc_read_fasta(path, -1, None, 0, None, 0, ctypes.byref(length), ctypes.byref(count)), L.imc_last_error())
    for slab in SLABS:
        with slab_bytes(slab):
            got = (L.imc_aln_open_fasta(path, ctypes.byref(h)), L.imc_last_error())
        assert got == want and want[0] == _capi.IMC_ERR_IO and needle in want[1] and h.value is None, (slab, got, want)


# ---- chunks ------------------------------------------------------------------------------------------------------
@pytest.fixture
def five(tmp_path):
    """Five records of 4097 bases, unwrapped or wrapped alike back to back on the device: their starts are 0, 4097, 8194,
    12291 and 16388, so every residue mod 4 occurs."""
    seqs = {"r%d" % k: bases(4097, seed=70 + k) for k in range(5)}
    path = _write(tmp_path, "five.fa", fasta([(k.encode(), v) for k, v in seqs.items()], wrap=60))
    aln = assert_parsed(path, None, "device")
    assert sorted(np.cumsum([0] + aln.lengths[:-1]) % 4) == [0, 0, 1, 2, 3]
    yield aln, seqs
    aln.close()


def test_every_pair_of_five_records(five, dictionary3):
    aln, seqs = five
    names = aln.names
    for i, a in enumerate(names):
        for b in names[i:]:                                              # (a, a) included
            dev, _ = assert_chunk(aln, (a, b), seqs, ("pair", a, b))
            assert dev.compressed_length(16384)[1] == dictionary3
    assert_chunk(aln, (names[4], names[1]), seqs, "pair in reverse order")


def test_triplets_of_five_records(five, dictionary65):
    aln, seqs = five
    names = aln.names
    for members in ((0, 1, 2), (4, 2, 0), (1, 1, 3)):
        assert_chunk(aln, tuple(names[m] for m in members), seqs, ("triplet", members))


@pytest.mark.parametrize("n", [1, 3, 4096, 70001])
def test_lengths(tmp_path, dictionary3, n):
    """One pair and one triplet per length; at 70001 columns the column kernel runs more than one workgroup, and the
    triplet chunk (no 65-symbol dictionary is asked for here) is compared as raw symbols at every level."""
    seqs = {"x%d" % k: bases(n, seed=n + k) for k in range(3)}
    path = _write(tmp_path, "n.fa", fasta([(k.encode(), v) for k, v in seqs.items()], wrap=60))
    with assert_parsed(path, None, "device") as aln:
        assert_chunk(aln, ("x0", "x2"), seqs, ("pair", n))
        assert_chunk(aln, ("x2", "x0", "x1"), seqs, ("triplet", n))


def _closed_then_evaluated(aln, seqs, names, nsym):
    dev, host = assert_chunk(aln, names, seqs, names)
    aln.close()                                                          # the chunk keeps no reference to the alignment
    with pytest.raises(ValueError, match="closed"):
        aln.forwarder(*names)
    pi, T, E = synth.random_hmm(10, nsym, seed=nsym, stay=0.97)
    got = forward_chunks_batch([host.handle, dev.handle], pi[None], T[None], E[None], per_chunk=True)[0]
    assert got[0] == got[1] and np.isfinite(got[0]), (nsym, got)


def test_a_pair_outlives_its_alignment_and_evaluates_to_the_same_bits(five, dictionary3):
    _closed_then_evaluated(five[0], five[1], ("r1", "r3"), 3)


def test_a_triplet_outlives_its_alignment_and_evaluates_to_the_same_bits(five, dictionary65):
    _closed_then_evaluated(five[0], five[1], ("r0", "r2", "r4"), 65)


def test_argument_errors_that_need_an_alignment(tmp_path):
    L = _capi.lib()
    path = _write(tmp_path, "u.fa", b">a\nACGT\n>bb\nACGTA\n>c\nACGT\n")
    with Alignment(path) as aln:
        h = ctypes.c_void_p()
        for members, k, needle in (((0, 3), 2, b"not a record"), ((-1, 0), 2, b"not a record"), ((0, 2, 5), 3, b"not a record"),
                                   ((0, 1), 2, b"a has 4 bases, bb has 5"), ((2, 0, 1), 3, b"c has 4 bases, bb has 5")):
            rc = L.imc_obs_create_from_alignment(aln.handle, (ctypes.c_int32 * 3)(*members), k, ctypes.byref(h))
            assert rc == _capi.IMC_ERR_ARG and needle in L.imc_last_error() and h.value is None, (members, rc, L.imc_last_error())
        with pytest.raises(KeyError):
            aln.forwarder("a", "nobody")
        with pytest.raises(ValueError):
            aln.forwarder("a")
        with pytest.raises(ValueError, match="differ in length"):
            aln.forwarder("a", "bb")
        assert raw_symbols(aln.forwarder("a", "c")).tolist() == [0, 0, 0, 0]
        assert aln.sequence("bb") == b"ACGTA" and len(aln) == 3


def test_pairs_are_pairwise_forwarders(tmp_path, dictionary3):
    seqs = {"a": "ACGTACGTNN--ACGT" * 300, "b": "ACGTACCTNNA-ACGA" * 300, "c": "acgtacgtnnccacgt" * 300}   # test_pairwise_forwarders_from_an_alignment
    fa = tmp_path / "three.fa"
    fa.write_text("".join(">%s\n%s\n" % kv for kv in seqs.items()))
    want = prepare.pairwise_forwarders(str(fa))
    with Alignment(str(fa)) as aln:
        assert aln.parser == "device"
        got = aln.pairs()
        only = aln.pairs([("c", "a")])
        with pytest.raises(KeyError):
            aln.pairs([("a", "nobody")])
        assert aln.pairs([]) == {}
    assert list(got) == list(want) == [("a", "b"), ("a", "c"), ("b", "c")]
    for key in want:
        assert (raw_symbols(got[key]) == raw_symbols(want[key])).all(), key
        assert_same_chunk(want[key], got[key], key)
    assert list(only) == [("c", "a")] and len(only[("c", "a")]) == 4800


# ---- guard pages ----------------------------------------------------------------------------------------------
GUARD_SCRIPT = textwrap.dedent('''
    import sys, tempfile
    sys.path.insert(0, %r)
    sys.path.insert(0, %r)
    from device_encode_cases import train3
    from alignment_cases import small_cases
    train3()
    with tempfile.TemporaryDirectory() as tmp:
        small_cases(tmp)
    print("alignment ok", flush=True)
''') % (REPO, os.path.join(REPO, "tests"))


def test_alignments_under_guard_pages(tmp_path, dictionary3):
    """Slabs, tile tables, the record table, the resident buffer and the chunk's own buffer flush against an unmapped
    page: the cases run here first, then once more in a process with IMC_GUARD=1."""
    small_cases(str(tmp_path))
    script = tmp_path / "guard_alignment.py"
    script.write_text(GUARD_SCRIPT)
    env = dict(os.environ, IMC_GUARD="1")
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    tail = (out.stdout[-1500:], out.stderr[-3000:])
    if "hipMemAddressReserve" in out.stderr or "hipMemCreate" in out.stderr or "hipMemGetAllocationGranularity" in out.stderr:
        pytest.skip("HIP virtual-memory management is unavailable on this box: %r" % (tail,))
    assert out.returncode == 0 and "alignment ok" in out.stdout, tail
