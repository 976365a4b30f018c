"""Shared by tests/test_gpu_phylip.py, tests/test_phylip_cpu.py and the guard-mode script: how PHYLIP files are written
(sequential or interleaved, block widths, name padding, groups separated by spaces, blank lines between blocks, the line
break), what is compared after one is opened as an Alignment (names, order, every sequence, the parser that ran and what
imc_aln_info says, against prepare.read_phylip - the specification), and the small cases that also run under IMC_GUARD=1."""
import os

from alignment_cases import assert_chunk, bases
from device_ingest_cases import DEFAULT_SLAB, MIN_SLAB, slab_bytes
from imcoalhmm_amd import Alignment, prepare


def phylip(records, widths=None, pad=10, group=0, blank=False, eol=b"\n", final=True, header=None):
    """PHYLIP bytes of [(name, bases)].  widths None: sequential, one line per record (seq-gen's shape); an int: interleaved
    blocks of that width; a list: the widths of the blocks (the last block takes what is left); a list of lists: the widths
    per record.  pad: names are padded with spaces to that many columns (at least one space when bases follow); group:
    bases in groups of that many, separated by one space; blank: an empty line between blocks."""
    n, length = len(records), len(records[0][1])
    if widths is None:
        widths = [length]
    elif isinstance(widths, int):
        widths = [widths] * max(1, -(-length // widths))
    per_record = widths if isinstance(widths[0], (list, tuple)) else [widths] * n

    def grouped(s):
        return s if not group else b" ".join(s[at:at + group] for at in range(0, len(s), group))

    out = [header if header is not None else b" %d %d" % (n, length)]
    done = [0] * n
    for block in range(len(per_record[0])):
        if block and blank:
            out.append(b"")
        for r, (name, seq) in enumerate(records):
            last = block == len(per_record[r]) - 1
            piece = seq[done[r]:] if last else seq[done[r]:done[r] + per_record[r][block]]
            done[r] += len(piece)
            if block == 0:
                out.append((name.ljust(pad) + (b"" if name.ljust(pad).endswith(b" ") else b" ") + grouped(piece)) if piece else name)
            else:
                assert piece, "a line behind the name lines must hold a base"
                out.append(grouped(piece))
    data = eol.join(out) + eol
    return data if final else data[:-len(eol)]


def phylip_slabs(data, slab):
    """Slabs a PHYLIP file of these bytes goes up in: it is cut anywhere."""
    slab = min(slab or DEFAULT_SLAB, max(len(data), MIN_SLAB))
    return -(-len(data) // slab)


def assert_parsed_phylip(path, slab=None, parser="device"):
    """Open the file as an Alignment: the parser that ran, the names in order, every sequence and imc_aln_info against
    prepare.read_phylip.  Returns the open alignment."""
    data = open(path, "rb").read()
    want = prepare.read_phylip(path)
    with slab_bytes(slab):
        aln = Alignment(path, in_format="phylip")
    what = (os.path.basename(path), slab)
    assert aln.in_format == "phylip"
    assert aln.parser == parser, (what, aln.info)
    assert aln.names == list(want), (what, aln.names[:8], list(want)[:8])
    assert aln.lengths == [len(v) for v in want.values()], (what, aln.lengths[:8])
    for name, seq in want.items():
        got = aln.sequence(name)
        assert got == seq.encode("latin-1"), (what, name, len(got), len(seq), [k for k in range(min(len(got), len(seq))) if got[k] != ord(seq[k])][:4])
    if parser == "device":
        assert aln.info == {"parser": "device", "bytes": len(data), "slabs": phylip_slabs(data, slab), "records": len(want)}, (what, aln.info)
    else:
        assert aln.info == {"parser": "host", "bytes": 0, "slabs": 0, "records": len(want)}, (what, aln.info)
    return aln


def small_cases(tmp, sizes=(4095, 4096, 4097), slab=4096):
    """The smallest sequential and interleaved files around a tile and a slab, with the smallest slab, parsed on the
    device, and one pair from each: the cases that run once with every device buffer flush against an unmapped page."""
    for n in sizes:
        seqs = {b"s%d" % k: bases(n, seed=700 + 10 * n + k) for k in range(3)}
        named = {k.decode(): v for k, v in seqs.items()}
        for shape, widths in (("seq", None), ("int", 61)):
            path = os.path.join(tmp, "g%d.%s.phy" % (n, shape))
            with open(path, "wb") as fh:
                fh.write(phylip(list(seqs.items()), widths))
            aln = assert_parsed_phylip(path, slab)
            assert_chunk(aln, ("s2", "s0"), named, ("guard pair", n, shape))
            aln.close()
