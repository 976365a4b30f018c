"""Shared by tests/test_gpu_alignment.py and the guard-mode script it starts: how FASTA files are written, the slab count
the slab rule of csrc/align_tiles.hpp gives for a file, what is compared after an alignment is opened (names, order and
every sequence against prepare.read_fasta; what imc_aln_info says), what is compared for a chunk built from resident
sequences (raw symbols against the host encoders, every level against the chunk Forwarder.from_array builds from them,
what imc_last_ingest says), and the small cases that also run under IMC_GUARD=1."""
import os

import numpy as np

from device_encode_cases import assert_same_chunk
from device_ingest_cases import DEFAULT_SLAB, MIN_SLAB, raw_symbols, slab_bytes
from imcoalhmm_amd import Alignment, Forwarder, _capi, prepare

COMMON = np.frombuffer(b"ACGTacgtNn-", dtype=np.uint8)
# every printable byte but '>', which starts a header wherever a line happens to begin with it
PRINTABLE = np.array([c for c in range(0x21, 0x7f) if c != ord(">")], dtype=np.uint8)


def bases(n, seed):
    """n bases from "ACGTacgtNn-", 5 % of them replaced by arbitrary printable bytes."""
    rng = np.random.default_rng(seed)
    s = rng.choice(COMMON, size=n)
    other = rng.random(n) < 0.05
    s[other] = rng.choice(PRINTABLE, size=int(other.sum()))
    return bytes(s)


def fasta(records, wrap=60, eol=b"\n", final=True):
    """FASTA bytes of [(header text behind '>', bases)]; wrap None: one line per record."""
    out = []
    for header, seq in records:
        out.append(b">" + header + eol)
        width = wrap or max(len(seq), 1)
        for at in range(0, len(seq), width):
            out.append(seq[at:at + width] + eol)
    data = b"".join(out)
    return data if final or not data.endswith(eol) else data[:-len(eol)]


def fasta_slabs(data, slab):
    """Slabs a FASTA file of these bytes goes up in: a slab ends where the buffer ends unless the buffer's last line is a
    header line, which is carried into the next slab - or None where a header line is longer than a slab (declined)."""
    slab = min(slab or DEFAULT_SLAB, max(len(data), MIN_SLAB))
    buf, pos, slabs, at_line_start = b"", 0, 0, True
    while True:
        take = min(slab - len(buf), len(data) - pos)
        buf += data[pos:pos + take]
        pos += take
        eof = pos == len(data)
        line = buf.rfind(b"\n") + 1
        if eof or line == len(buf) or (line == 0 and not at_line_start) or buf[line:line + 1] != b">":
            cut = len(buf)
        else:
            cut = line
        if cut == 0:
            return slabs if eof else None
        slabs += 1
        at_line_start = buf[cut - 1:cut] == b"\n"
        buf = buf[cut:]
        if eof:
            return slabs


def assert_parsed(path, slab=None, parser="device"):
    """Open the file as an Alignment: the parser that ran, the names in order, every sequence and imc_aln_info against
    prepare.read_fasta and the slab rule.  Returns the open alignment."""
    data = open(path, "rb").read()
    want = prepare.read_fasta(path)
    with slab_bytes(slab):
        aln = Alignment(path)
    what = (os.path.basename(path), slab)
    assert aln.parser == parser, (what, aln.info)
    assert aln.names == list(want), (what, aln.names[:8], list(want)[:8])
    assert aln.lengths == [len(v) for v in want.values()], (what, aln.lengths[:8])
    for name, seq in want.items():
        got = aln.sequence(name)
        assert got == seq.encode("latin-1"), (what, name, len(got), len(seq))
    if parser == "device":
        assert aln.info == {"parser": "device", "bytes": len(data), "slabs": fasta_slabs(data, slab), "records": len(want)}, (what, aln.info, fasta_slabs(data, slab))
    else:
        assert aln.info == {"parser": "host", "bytes": 0, "slabs": 0, "records": len(want)}, (what, aln.info)
    return aln


def host_symbols(seqs):
    """The host encoders on two or three sequences (bytes)."""
    text = [s.decode("latin-1") for s in seqs]
    return prepare.encode_pairwise(*text) if len(seqs) == 2 else prepare.encode_triplet(*text)


def assert_chunk(aln, names, seqs, what):
    """The chunk of these records from the resident sequences against the host encoder's symbols and the chunk
    Forwarder.from_array builds from them; returns (from the alignment, from the array)."""
    want = host_symbols([seqs[n] for n in names])
    nsym = 3 if len(names) == 2 else 65
    dev = aln.forwarder(*names)
    how = _capi.last_ingest()
    assert how == {"path": "alignment", "bytes": 0, "slabs": 0, "columns": want.size}, (what, how)
    assert dev.NSYM == nsym and len(dev) == want.size, what
    got = raw_symbols(dev)
    assert got.size == want.size and (got == want).all(), (what, np.flatnonzero(got != want)[:8])
    host = Forwarder.from_array(want, nsym)
    assert_same_chunk(host, dev, what)
    return dev, host


def small_cases(tmp, sizes=(4096, 4097, 8193), slab=4096):
    """Three records at sizes around a tile and a slab, with the smallest slab, parsed on the device, and one pair and one
    triplet from them: the cases that run once more with every device buffer flush against an unmapped page."""
    for n in sizes:
        seqs = {b"s%d" % k: bases(n, seed=900 + 10 * n + k) for k in range(3)}
        path = os.path.join(tmp, "g%d.fa" % n)
        with open(path, "wb") as fh:
            fh.write(fasta([(k, v) for k, v in seqs.items()], wrap=61))
        aln = assert_parsed(path, slab)
        named = {k.decode(): v for k, v in seqs.items()}
        assert_chunk(aln, ("s0", "s1"), named, ("guard pair", n))
        assert_chunk(aln, ("s2", "s0", "s1"), named, ("guard triplet", n))
        aln.close()
