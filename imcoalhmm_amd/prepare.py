"""Pairwise or triplet alignment -> observation file, the counterpart of the pairwise and triplet branches of the
reference's scripts/prepare-alignments.py:77-146 (which needs BioPython; this does not).

    python -m imcoalhmm_amd.prepare examples/example_data.fa out.ziphmm --names hg18,pantro2
    python -m imcoalhmm_amd.prepare in.fa out.imc --names a,b --cache     # packed 2-bit cache
    python -m imcoalhmm_amd.prepare in.fa out.ziphmm --names a,b,c        # triplet: 65 symbols

The text output is byte-compatible with the reference's ("%d " per column, prepare-alignments.py:99-105 and 142-146)
and the outputs are accepted by ``Forwarder(input_filename, NSYM=3)`` (pairs) and ``Forwarder(input_filename, NSYM=65)``
(triplets).  To build chunks straight from an alignment, without a file in between, open it with
``imcoalhmm_amd.Alignment``.  Quartet alignments are out of scope: the script's own formula (``... + 32*i4``, missing =
128, lines 186-190) collides with valid codes and disagrees with ILS.py:414-433, which decodes base 4.
"""
import argparse
import ctypes
import os

import numpy as np

from . import _capi


def read_fasta(path):
    """{name: sequence} in file order (name = first word of the header)."""
    seqs, name, parts = {}, None, []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            if line.startswith(">"):
                if name is not None:
                    seqs[name] = "".join(parts)
                name, parts = line[1:].split()[0], []
            else:
                parts.append(line)
    if name is not None:
        seqs[name] = "".join(parts)
    return seqs


def read_phylip(path):
    """Sequential or interleaved PHYLIP with names in the first 10 characters / first word."""
    with open(path) as f:
        lines = [l.rstrip("\n") for l in f if l.strip()]
    n, length = (int(x) for x in lines[0].split()[:2])
    names, seqs = [], []
    for l in lines[1:1 + n]:
        parts = l.split(None, 1)
        names.append(parts[0])
        seqs.append(parts[1].replace(" ", "") if len(parts) > 1 else "")
    rest = lines[1 + n:]
    for k, l in enumerate(rest):
        seqs[k % n] += l.replace(" ", "")
    out = dict(zip(names, seqs))
    for k, v in out.items():
        if len(v) != length:
            raise ValueError("PHYLIP sequence %s has %d columns, header says %d" % (k, len(v), length))
    return out


def encode_pairwise(seq1, seq2):
    """uint8 symbols per column: 2 = either base not in ACGT, 0 = equal, 1 = different
    (scripts/prepare-alignments.py:99-105)."""
    if len(seq1) != len(seq2):
        raise ValueError("sequences differ in length: %d vs %d" % (len(seq1), len(seq2)))
    a, b = seq1.encode("ascii"), seq2.encode("ascii")
    out = np.empty(len(a), dtype=np.uint8)
    _capi.check(_capi.lib().imc_encode_pairwise(a, b, len(a), out.ctypes.data_as(_capi._u8p)))
    return out


def encode_triplet(seq1, seq2, seq3):
    """uint8 symbols per column: i1 + 4*i2 + 16*i3 with A, C, G, T -> 0..3 (either case), 64 = any of the three bases not
    in ACGT (scripts/prepare-alignments.py:134-146).  65 symbols."""
    if not len(seq1) == len(seq2) == len(seq3):
        raise ValueError("sequences differ in length: %d, %d and %d" % (len(seq1), len(seq2), len(seq3)))
    a, b, c = seq1.encode("ascii"), seq2.encode("ascii"), seq3.encode("ascii")
    out = np.empty(len(a), dtype=np.uint8)
    _capi.check(_capi.lib().imc_encode_triplet(a, b, c, len(a), out.ctypes.data_as(_capi._u8p)))
    return out


def read_fasta_native(path):
    """``read_fasta`` by the library's host reader (``imc_read_fasta``, csrc/fasta_io.hpp): {name: bytes} in file order
    for ASCII files; IOError for a header without a name and for a byte >= 0x80."""
    return _read_native(_capi.lib().imc_read_fasta, path)


def read_phylip_native(path):
    """``read_phylip`` by the library's host reader (``imc_read_phylip``, csrc/phylip_io.hpp): {name: bytes} in file order
    for ASCII files; IOError for what that header lists - a bad header, too few name lines, a repeated name, a record whose
    length differs from the header's, a byte >= 0x80."""
    return _read_native(_capi.lib().imc_read_phylip, path)


def _read_native(read, path):
    count, length = ctypes.c_int(0), ctypes.c_size_t(0)
    _capi.check(read(os.fsencode(path), -1, None, 0, None, 0, ctypes.byref(length), ctypes.byref(count)))
    out = {}
    for k in range(count.value):
        _capi.check(read(os.fsencode(path), k, None, 0, None, 0, ctypes.byref(length), ctypes.byref(count)))
        room = 4096
        while True:                                     # (a name is never empty: grow the buffer until it fits)
            name, seq = ctypes.create_string_buffer(room), ctypes.create_string_buffer(max(length.value, 1))
            _capi.check(read(os.fsencode(path), k, name, len(name), seq, length.value, ctypes.byref(length), ctypes.byref(count)))
            if name.value:
                break
            room *= 16
        out[name.value.decode("ascii")] = seq.raw[:length.value]
    return out


def pairwise_forwarders(path, pairs=None, in_format="fasta"):
    """{(a, b): Forwarder} for the given pairs of sequence names of an alignment file - or for all pairs, in file order -
    with the pairwise rule applied on the device (``Forwarder.from_sequences``): no intermediate observation file is
    written and no symbol array is built on the host."""
    from .hmm import Forwarder
    if in_format not in ("fasta", "phylip"):
        raise ValueError("in_format must be 'fasta' or 'phylip', got %r" % (in_format,))
    seqs = read_fasta(path) if in_format == "fasta" else read_phylip(path)
    names = list(seqs.keys())
    if pairs is None:
        pairs = [(a, b) for i, a in enumerate(names) for b in names[i + 1:]]
    out = {}
    for a, b in pairs:
        for name in (a, b):
            if name not in seqs:
                raise KeyError("no sequence named %r in %s" % (name, path))
        out[(a, b)] = Forwarder.from_sequences(seqs[a], seqs[b])
    return out


def write_text(path, obs):
    """The reference's own file format: one decimal token per column, each followed by a space."""
    obs = np.ascontiguousarray(obs, dtype=np.uint8)
    lut = np.array([b"%d " % k for k in range(256)], dtype="S4")
    with open(path, "wb", 64 * 1024) as f:
        for off in range(0, obs.size, 1 << 22):
            f.write(b"".join(lut[obs[off:off + (1 << 22)]].tolist()))


def write_cache(path, obs, nsym=3):
    obs = np.ascontiguousarray(obs, dtype=np.uint8)
    _capi.check(_capi.lib().imc_write_cache(os.fsencode(path), obs.ctypes.data_as(_capi._u8p), obs.size, int(nsym)))


def read_observations(path, nsym=3):
    """Parse a text or cache observation file on the host (what Forwarder.__init__ does before the upload)."""
    n = ctypes.c_size_t(0)
    L = _capi.lib()
    _capi.check(L.imc_read_observations(os.fsencode(path), int(nsym), None, 0, ctypes.byref(n)))
    out = np.empty(n.value, dtype=np.uint8)
    _capi.check(L.imc_read_observations(os.fsencode(path), int(nsym), out.ctypes.data_as(_capi._u8p), out.size, ctypes.byref(n)))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="pairwise or triplet alignment -> IMCoalHMM observation file")
    ap.add_argument("in_filename")
    ap.add_argument("output_filename")
    ap.add_argument("--names", default=None, help="comma-separated sequence names: two (pairwise) or three (triplet); default: the first two")
    ap.add_argument("--in-format", default="fasta", choices=["fasta", "phylip"])
    ap.add_argument("--cache", action="store_true", help="write the packed cache instead of text (2 bits per column for a pair, a byte for a triplet)")
    ap.add_argument("--verbose", action="store_true")
    args = ap.parse_args(argv)
    seqs = read_fasta(args.in_filename) if args.in_format == "fasta" else read_phylip(args.in_filename)
    names = args.names.split(",") if args.names else list(seqs.keys())[:2]
    if len(names) not in (2, 3):
        ap.error("two sequence names are needed for a pairwise alignment, three for a triplet")
    nsym = 3 if len(names) == 2 else 65
    obs = encode_pairwise(*(seqs[n] for n in names)) if len(names) == 2 else encode_triplet(*(seqs[n] for n in names))
    if args.cache:
        write_cache(args.output_filename, obs, nsym)
    else:
        write_text(args.output_filename, obs)
    if args.verbose:
        print("%s: %d columns, symbol counts %s" % (" vs ".join(names), obs.size, np.bincount(obs, minlength=nsym).tolist()))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
