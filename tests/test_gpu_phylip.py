"""PHYLIP alignments (csrc/kernels_phylip.hpp) on the GPU.  An Alignment opened with in_format="phylip" holds the names and
sequences prepare.read_phylip gives - sequential files whose lines span tiles and slabs, interleaved files at widths 60 and
1 and at unequal widths, names that straddle a tile and a slab boundary - in ceil(bytes / slab) slabs; every file the
device parser declines goes through the host reader with the same result, and the error files with the host reader's code
and message.  Chunks built from the resident sequences have the host encoders' symbols, are the chunks
Forwarder.from_array builds, and are the chunks a FASTA alignment of the same sequences gives.  Every comparison is exact."""
import ctypes
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from alignment_cases import assert_chunk, assert_parsed, bases, fasta
from device_encode_cases import assert_same_chunk, train3
from device_ingest_cases import raw_symbols, slab_bytes
from imcoalhmm_amd import Alignment, Forwarder, _capi, synth
from imcoalhmm_amd.hmm import forward_chunks_batch, set_device_encoding, set_device_ingest
from phylip_cases import assert_parsed_phylip, phylip, small_cases

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
    """The 3-symbol dictionary of device_encode_cases.train3, so that pair chunks get token streams; trained again only if
    another test has reset it."""
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


def _records(n, length, seed=0):
    return [(b"%d" % (k + 1), bases(length, seed=1000 * seed + 17 * length + k)) for k in range(n)]


# ---- parse equals specification: sequential -----------------------------------------------------------------------
@pytest.mark.parametrize("slab", SLABS)
@pytest.mark.parametrize("length", [1, 4095, 4096, 4097, 8193, 3 * 4096 + 5])
@pytest.mark.parametrize("n", [2, 4])
def test_sequential_files(tmp_path, n, length, slab):
    """seq-gen's shape: one line per record, names padded to 10 columns; with n = 4 and length = 4097 the four regions start
    at all four residues mod 4."""
    path = _write(tmp_path, "s.phy", phylip(_records(n, length), None, pad=10))
    aln = assert_parsed_phylip(path, slab, "device")
    if length > 4096 and slab:
        assert aln.info["slabs"] >= n
    aln.close()


# ---- parse equals specification: interleaved ----------------------------------------------------------------------
def _unequal_records(seed):
    """Three records whose lines differ in width within every block; every record totals 900."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(3):
        w = rng.integers(1, 120, size=14).tolist()
        out.append(w + [1])                                              # (the last block takes what is left)
    return out


INTERLEAVED = {
    "width 60": lambda: phylip(_records(3, 4300, 1), 60),
    "width 60, blank lines": lambda: phylip(_records(3, 4300, 2), 60, blank=True),
    "width 60, crlf": lambda: phylip(_records(3, 4300, 3), 60, eol=b"\r\n"),
    "width 60, crlf, blank lines": lambda: phylip(_records(3, 4300, 4), 60, blank=True, eol=b"\r\n"),
    "width 60, groups of 10": lambda: phylip(_records(3, 4300, 5), 60, group=10),
    "width 60, no final newline": lambda: phylip(_records(3, 4300, 6), 60, final=False),
    "width 60, groups, blank lines, crlf, no final newline": lambda: phylip(_records(4, 4097, 7), 60, group=10, blank=True, eol=b"\r\n", final=False),
    "width 1": lambda: phylip(_records(3, 2100, 8), 1),
    "width 1, blank lines": lambda: phylip(_records(2, 2100, 9), 1, blank=True),
    "width 1, crlf, no final newline": lambda: phylip(_records(2, 2100, 10), 1, eol=b"\r\n", final=False),
    "blocks of different widths": lambda: phylip(_records(3, 9000, 11), [50, 70, 3, 1, 4096, 60, 4097, 2, 200, 1]),
    "records of different widths in a block": lambda: phylip(_records(3, 900 + 700, 12), _unequal_records(12), blank=True),
    "name-only name lines": lambda: phylip(_records(3, 4300, 13), [0, 60, 4100, 70]),
    "spaces-only lines": lambda: phylip(_records(3, 4300, 14), 60, blank=True).replace(b"\n\n", b"\n    \n"),
    "leading blank lines": lambda: b"\n   \n\r\n" + phylip(_records(2, 4300, 15), 61),
    "zero length": lambda: b"3 0\na\nb\nc\n",
}


@pytest.mark.parametrize("slab", SLABS)
@pytest.mark.parametrize("name", sorted(INTERLEAVED))
def test_interleaved_files(tmp_path, name, slab):
    path = _write(tmp_path, "i.phy", INTERLEAVED[name]())
    assert_parsed_phylip(path, slab, "device").close()


# ---- names across tile and slab boundaries ------------------------------------------------------------------------
def _second_name_at(offset, name, long_header):
    """Two records; the second name starts at byte `offset` of the file.  long_header: the first record is name-only and
    the header line is long (leading spaces); else the first name line carries the bases in front of it."""
    total = 600
    a, b = bases(total, seed=offset + len(name)), bases(total, seed=offset + len(name) + 1)
    if long_header:
        head = b"2 %d\n" % total
        head = b" " * (offset - len(head) - 2) + head
        data = head + b"a\n" + name + b" " + b[:60] + b"\n" + a[:540] + b"\n" + b[60:] + b"\n" + a[540:] + b"\n"
    else:
        total = offset + 100
        a, b = bases(total, seed=offset + len(name)), bases(total, seed=offset + len(name) + 1)
        head = b"2 %d\n" % total
        first = offset - len(head) - 3
        data = head + b"a " + a[:first] + b"\n" + name + b"  " + b[:7] + b"\n" + a[first:] + b"\n" + b[7:] + b"\n"
    assert data[offset:offset + len(name)] == name and data[offset - 1:offset] == b"\n"
    return data


@pytest.mark.parametrize("slab", SLABS)
@pytest.mark.parametrize("long_header", [False, True])
@pytest.mark.parametrize("size", [1, 6, 7, 100, 255])
def test_a_name_across_a_tile_and_a_slab_boundary(tmp_path, size, long_header, slab):
    """The second name starts at byte 4090: from 7 bytes on it crosses byte 4096, a tile boundary, and with the smallest
    slab a slab boundary."""
    name = bytes(0x21 + (7 * k) % 0x5e for k in range(size))
    path = _write(tmp_path, "n.phy", _second_name_at(4090, name, long_header))
    aln = assert_parsed_phylip(path, slab, "device")
    assert aln.names == ["a", name.decode("ascii")]
    aln.close()


def test_one_record_and_4096_records(tmp_path):
    for slab in SLABS:
        assert_parsed_phylip(_write(tmp_path, "one.phy", phylip(_records(1, 5000), 61)), slab, "device").close()
        assert_parsed_phylip(_write(tmp_path, "one.phy", phylip(_records(1, 5000), None)), slab, "device").close()
    many = [(b"r%d" % k, bytes(b"ACGT"[(k + j) % 4] for j in range(3))) for k in range(4096)]
    for slab in SLABS:
        aln = assert_parsed_phylip(_write(tmp_path, "many.phy", phylip(many, None, pad=0)), slab, "device")
        assert aln.info["records"] == 4096
        aln.close()
        assert_parsed_phylip(_write(tmp_path, "many.phy", phylip(many, 1, pad=0)), slab, "device").close()


# ---- declines fall back, identically -----------------------------------------------------------------------------
def _three(length=3000):
    return _records(3, length, 20)


def _one_break_as_cr(data, k):
    """The k-th line ends with a lone '\\r': the same lines for universal newlines."""
    lines = data.split(b"\n")
    return b"\n".join(lines[:k]) + b"\r" + b"\n".join(lines[k:])


DECLINED = {
    "a tab separator": lambda: phylip(_three(), 60).replace(b"2         ", b"2\t", 1),
    "a leading space in front of a name": lambda: phylip(_three(), 60).replace(b"\n2 ", b"\n 2 ", 1),
    "a lone carriage return": lambda: _one_break_as_cr(phylip(_three(), 60), 100),
    "a third header token": lambda: phylip(_three(), 60, header=b"3 3000 I"),
    "a 256-byte name": lambda: phylip([(b"n" * 256, bases(500, 1)), (b"m", bases(500, 2))], 60),
    "4097 records": lambda: phylip([(b"r%d" % k, b"ACG") for k in range(4097)], None, pad=0),
}


@pytest.mark.parametrize("name", sorted(DECLINED))
def test_declined_files_go_through_the_host_reader(tmp_path, name):
    data = DECLINED[name]()
    assert {"a tab separator": b"\n2\t", "a leading space in front of a name": b"\n 2 ", "a lone carriage return": b"\r",
            "a third header token": b" I\n", "a 256-byte name": b"n" * 256, "4097 records": b"\nr4096 "}[name] in data
    path = _write(tmp_path, "d.phy", data)
    for slab in SLABS:
        assert_parsed_phylip(path, slab, "host").close()


def test_a_header_line_longer_than_the_slab_declines(tmp_path):
    data = phylip(_three(), 60, header=b" " * 4200 + b"3 3000")
    path = _write(tmp_path, "h.phy", data)
    assert_parsed_phylip(path, 4096, "host").close()
    assert_parsed_phylip(path, None, "device").close()                  # ... and fits a slab of the default size


def _error_files():
    good = phylip(_three(3000), 60)
    short_last = phylip(_three(3000), 60, final=False)[:-1]
    fewer = phylip(_three(3000)[:2], None, header=b"3 3000")
    repeated = phylip([(b"x", bases(3000, 1)), (b"y", bases(3000, 2)), (b"x", bases(3000, 3))], 60)
    high = good[:-20] + b"\xe9" + good[-19:]
    return {"a length mismatch in the last record only": (short_last, b"PHYLIP sequence 3 has 2999 columns, header says 3000"),
            "fewer name lines than n": (fewer, b"says 3 sequences, 2 name lines"),
            "a repeated name": (repeated, b"name x is repeated"),
            "a byte >= 0x80 in the last slab": (high, b"non-ASCII byte")}


@pytest.mark.parametrize("name", sorted(_error_files()))
def test_error_files_have_the_host_readers_code_and_message(tmp_path, name):
    data, needle = _error_files()[name]
    L = _capi.lib()
    text = _write(tmp_path, "e.phy", data)
    path = os.fsencode(text)
    count, length, h = ctypes.c_int(0), ctypes.c_size_t(0), ctypes.c_void_p()
    want = (L.imc_read_phylip(path, -1, None, 0, None, 0, ctypes.byref(length), ctypes.byref(count)), L.imc_last_error())
    for slab in SLABS:
        with slab_bytes(slab):
            got = (L.imc_aln_open_phylip(path, ctypes.byref(h)), L.imc_last_error())
            assert got == want and want[0] == _capi.IMC_ERR_IO and needle in want[1] and h.value is None, (slab, got, want)
            with pytest.raises(IOError):
                Alignment(text, in_format="phylip")


# ---- chunks ------------------------------------------------------------------------------------------------------
@pytest.fixture(params=["sequential", "interleaved"])
def four(tmp_path, request):
    """Four records of 4097 bases: their regions start at 0, 4097, 8194 and 12291, every residue mod 4."""
    seqs = {"r%d" % k: bases(4097, seed=170 + k) for k in range(4)}
    data = phylip([(k.encode(), v) for k, v in seqs.items()], None if request.param == "sequential" else 60)
    aln = assert_parsed_phylip(_write(tmp_path, "four.phy", data), None, "device")
    yield aln, seqs
    aln.close()


def test_pairs_and_triplets_from_resident_sequences(four, dictionary3):
    aln, seqs = four
    for names in (("r0", "r1"), ("r3", "r2"), ("r1", "r1"), ("r2", "r0")):
        dev, _ = assert_chunk(aln, names, seqs, ("pair", names))
        assert dev.compressed_length(16384)[1] == dictionary3
    for names in (("r0", "r1", "r2"), ("r3", "r1", "r0")):
        assert_chunk(aln, names, seqs, ("triplet", names))
    assert list(aln.pairs()) == [(a, b) for i, a in enumerate(aln.names) for b in aln.names[i + 1:]]


def test_phylip_and_fasta_alignments_give_the_same_chunks_and_bits(tmp_path, dictionary3):
    seqs = {"r%d" % k: bases(5000, seed=270 + k) for k in range(3)}
    records = [(k.encode(), v) for k, v in seqs.items()]
    pi, T, E = synth.random_hmm(10, 3, seed=3, stay=0.97)
    with assert_parsed(_write(tmp_path, "s.fa", fasta(records, wrap=60)), None, "device") as fa:
        for shape, widths in (("seq", None), ("int", 60)):
            with assert_parsed_phylip(_write(tmp_path, shape + ".phy", phylip(records, widths)), 4096, "device") as ph:
                for names in (("r0", "r2"), ("r1", "r0", "r2")):
                    a, b = fa.forwarder(*names), ph.forwarder(*names)
                    assert (raw_symbols(a) == raw_symbols(b)).all(), (shape, names)
                    assert_same_chunk(a, b, (shape, names))
                    if len(names) == 2:
                        got = forward_chunks_batch([a.handle, b.handle], pi[None], T[None], E[None], per_chunk=True)[0]
                        assert got[0] == got[1] and np.isfinite(got[0]), (shape, got)


def test_chunks_outlive_the_alignment_and_close_twice_is_fine(four, dictionary3):
    aln, seqs = four
    dev, host = assert_chunk(aln, ("r1", "r3"), seqs, "lifetime")
    aln.close()
    aln.close()
    with pytest.raises(ValueError, match="closed"):
        aln.forwarder("r1", "r3")
    pi, T, E = synth.random_hmm(10, 3, seed=5, stay=0.97)
    got = forward_chunks_batch([host.handle, dev.handle], pi[None], T[None], E[None], per_chunk=True)[0]
    assert got[0] == got[1] and np.isfinite(got[0]), got


# ---- guard pages ----------------------------------------------------------------------------------------------
GUARD_SCRIPT = textwrap.dedent('''
    import sys, tempfile
    sys.path.insert(0, %r)
    sys.path.insert(0, %r)
    from phylip_cases import small_cases
    with tempfile.TemporaryDirectory() as tmp:
        small_cases(tmp)
    print("phylip ok", flush=True)
''') % (REPO, os.path.join(REPO, "tests"))


def test_phylip_under_guard_pages(tmp_path):
    """Slabs, tile tables, the line table, the name table, the resident buffer and the chunk's own buffer flush against an
    unmapped page: once, in a process with IMC_GUARD=1."""
    script = tmp_path / "guard_phylip.py"
    script.write_text(GUARD_SCRIPT)
    env = dict(os.environ, IMC_GUARD="1")
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    tail = (out.stdout[-1500:], out.stderr[-3000:])
    if "hipMemAddressReserve" in out.stderr or "hipMemCreate" in out.stderr or "hipMemGetAllocationGranularity" in out.stderr:
        pytest.skip("HIP virtual-memory management is unavailable on this box: %r" % (tail,))
    assert out.returncode == 0 and "phylip ok" in out.stdout, tail
