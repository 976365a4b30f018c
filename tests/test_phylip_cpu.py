"""PHYLIP alignments (csrc/phylip_io.hpp, csrc/phylip_tiles.hpp, csrc/kernels_phylip.hpp) and their entry points -
imc_read_phylip, imc_aln_open_phylip, Alignment(path, in_format="phylip"), prepare.read_phylip_native - as far as a machine
without a GPU can see them.  tests/phylip_tiles_check.cpp drives the functions the kernels call, tile by tile and slab by
slab, against the host reader under AddressSanitizer + UBSan; the host reader itself is held to prepare.read_phylip - the
specification - here; the rest are the symbols, the argument checks, the errors that need no device, and the kernels'
register budget.  Parsed sequences and chunks are compared on the device in tests/test_gpu_phylip.py."""
import ctypes
import os
import re
import subprocess

import pytest

from imcoalhmm_amd import Alignment, _capi, build, prepare
from test_encode_tiles_cpu import run_check_under_asan_ubsan
from kernel_scratch_cases import scratch_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "imcoalhmm_amd", "csrc")
NEW = ("imc_read_phylip", "imc_aln_open_phylip")


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _capi.lib()


def test_phylip_tiles_under_asan_ubsan(tmp_path):
    run_check_under_asan_ubsan(tmp_path, "phylip_tiles_check", "phylip_tiles ok")


# ---- the host reader against prepare.read_phylip ----------------------------------------------------------------
PHYLIP_CASES = {
    "seq-gen shape": b" 2 8\n1         ACGTACGT\n2         ACGTACGA\n",
    "interleaved, blank line between blocks": b"2 8\na ACGT\nb ACGA\n\nACGT\nTTTT\n",
    "unequal block widths": b"2 9\na ACG\nb ACGTA\nACGTAC\nACGT\n",
    "groups of four": b"2 12\nalpha      ACGT ACGT ACGT\nbeta       ACGT ACGA ACGT\n",
    "groups of four, interleaved": b"2 12\nalpha ACGT ACGT\nbeta ACGT ACGA\nACGT\nAC GT\n",
    "name-only name lines": b"2 4\na\nb\nACGT\nACGA\n",
    "name-only first record": b"2 4\na\nb AC\nACGT\nGA\n",
    "crlf": b"2 8\r\na ACGT\r\nb ACGA\r\n\r\nACGT\r\nTTTT\r\n",
    "lone cr": b"2 8\ra ACGT\rb ACGA\r\rACGT\rTTTT\r",
    "no final newline": b"2 8\na ACGT\nb ACGA\nACGT\nTTTT",
    "a line of spaces between blocks": b"2 8\na ACGT\nb ACGA\n   \nACGT\nTTTT\n",
    "trailing spaces": b"2 8  \na ACGT  \nb ACGA \nACGT   \nTTTT \n",
    "leading spaces": b"2 8\n  a ACGT\nb ACGA\n  ACGT\n TTTT\n",
    "a tab as separator": b"2 4\na\tACGT\nb \t ACGA\n",
    "leading blank lines": b"\n  \n\r\n2 4\na ACGT\nb ACGA\n",
    "one record": b"1 6\nonly ACG\nTGA\n",
    "a third header token": b"2 4 I\na ACGT\nb ACGA\n",
    "interior control bytes stay": b"2 5\na AC\x01GT\nb A\tCGA\n",
    "zero length": b"2 0\na\nb\n",
    "long name, no blank": b"2 4\nabcdefghijklmnop ACGT\nq ACGT\n",
}


@pytest.mark.parametrize("case", sorted(PHYLIP_CASES))
def test_read_phylip_is_prepares(lib, tmp_path, case):
    path = tmp_path / "x.phy"
    path.write_bytes(PHYLIP_CASES[case])
    want = prepare.read_phylip(str(path))
    got = prepare.read_phylip_native(str(path))
    assert list(got) == list(want), case
    assert {k: v.decode("ascii") for k, v in got.items()} == want, case


ERRORS = {
    "a trailing tab counts": (b"2 4\na ACGT\t\nb ACGA\n", b"PHYLIP sequence a has 5 columns, header says 4"),
    "a plain mismatch": (b"2 4\na ACGT\nb ACG\n", b"PHYLIP sequence b has 3 columns, header says 4"),
    "an empty file": (b"", b"no PHYLIP header"),
    "blank lines only": (b"\n  \n", b"no PHYLIP header"),
    "one header token": (b"2\na ACGT\n", b"needs two numbers"),
    "n = 0": (b"0 4\n", b"0 sequences"),
    "1_0 as length": (b"2 1_0\na ACGTACGTAC\nb ACGTACGTAC\n", b"'1_0' is not a decimal number"),
    "+2 as count": (b"+2 4\na ACGT\nb ACGA\n", b"'+2' is not a decimal number"),
    "a count that does not fit": (b"4294967296 1\na A\n", b"does not fit"),
    "a length that does not fit": (b"1 99999999999999999999\na A\n", b"does not fit"),
    "fewer name lines than n": (b"3 4\na ACGT\nb ACGA\n", b"says 3 sequences, 2 name lines"),
    "a repeated name": (b"2 4\na ACGT\na ACGA\n", b"name a is repeated"),
    "a byte >= 0x80": (b"2 4\na AC\xc3\xa9\nb ACGA\n", b"non-ASCII byte"),
}


@pytest.mark.parametrize("case", sorted(ERRORS))
def test_read_phylip_deviations_are_io_errors(lib, tmp_path, case):
    data, needle = ERRORS[case]
    path = tmp_path / "bad.phy"
    path.write_bytes(data)
    count, length = ctypes.c_int(-1), ctypes.c_size_t(0)
    rc = lib.imc_read_phylip(os.fsencode(str(path)), -1, None, 0, None, 0, ctypes.byref(length), ctypes.byref(count))
    assert rc == _capi.IMC_ERR_IO and needle in lib.imc_last_error() and b"bad.phy" in lib.imc_last_error(), (rc, lib.imc_last_error())
    with pytest.raises(IOError):
        prepare.read_phylip_native(str(path))


def test_the_length_mismatches_are_pythons_too(tmp_path):
    for case in ("a trailing tab counts", "a plain mismatch"):
        path = tmp_path / "m.phy"
        path.write_bytes(ERRORS[case][0])
        with pytest.raises(ValueError) as ei:
            prepare.read_phylip(str(path))
        assert ERRORS[case][1].decode() in str(ei.value)


def test_read_phylip_missing_file_and_null_path(lib, tmp_path):
    count, length = ctypes.c_int(-1), ctypes.c_size_t(0)
    assert lib.imc_read_phylip(os.fsencode(str(tmp_path / "missing.phy")), -1, None, 0, None, 0, ctypes.byref(length), ctypes.byref(count)) == _capi.IMC_ERR_IO
    assert b"cannot open" in lib.imc_last_error()
    assert lib.imc_read_phylip(None, -1, None, 0, None, 0, ctypes.byref(length), ctypes.byref(count)) == _capi.IMC_ERR_ARG
    path = tmp_path / "two.phy"
    path.write_bytes(PHYLIP_CASES["seq-gen shape"])
    name, seq = ctypes.create_string_buffer(16), ctypes.create_string_buffer(8)
    assert lib.imc_read_phylip(os.fsencode(str(path)), 1, name, 16, seq, 8, ctypes.byref(length), ctypes.byref(count)) == _capi.IMC_OK
    assert (name.value, seq.raw, length.value, count.value) == (b"2", b"ACGTACGA", 8, 2)
    assert lib.imc_read_phylip(os.fsencode(str(path)), 2, name, 16, seq, 8, ctypes.byref(length), ctypes.byref(count)) == _capi.IMC_ERR_ARG


# ---- the boundary -----------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_declared_and_bound(lib):
    header = open(os.path.join(REPO, "include", "imcoal_fwd.h")).read()
    source = open(os.path.join(CSRC, "imcoal_fwd.hip")).read()
    names = [sig[0] for sig in _capi.SIGNATURES]
    for name in NEW:
        assert hasattr(lib, name)
        assert len(re.findall(r"^int %s\(" % name, header, flags=re.M)) == 1, name
        assert len(re.findall(r"^int %s\(" % name, source, flags=re.M)) == 1, name
        assert names.count(name) == 1
    by_name = {sig[0]: sig for sig in _capi.SIGNATURES}
    assert by_name["imc_read_phylip"][1:] == by_name["imc_read_fasta"][1:]
    assert by_name["imc_aln_open_phylip"][1:] == by_name["imc_aln_open_fasta"][1:]
    assert callable(prepare.read_phylip_native)


def test_header_exports_and_signatures_name_the_same_set(lib):
    header = open(os.path.join(REPO, "include", "imcoal_fwd.h")).read()
    declared = set(re.findall(r"^[A-Za-z_][A-Za-z0-9_ \*]*?\b(imc_[a-z0-9_]+)\(", header, flags=re.M))
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(REPO, "imcoalhmm_amd", "libimcoal_fwd.so")], capture_output=True, text=True)
    if out.returncode != 0:
        pytest.skip("nm not available")
    exported = set(re.findall(r" T (imc_[a-z0-9_]+)$", out.stdout, flags=re.M))
    for name in NEW:
        assert name in declared and name in exported
    bound = {sig[0] for sig in _capi.SIGNATURES}
    assert {n for n in declared if "phylip" in n} == {n for n in exported if "phylip" in n} == {n for n in bound if "phylip" in n} == set(NEW)


@pytest.mark.parametrize("what", ["null out", "null path"])
def test_argument_errors_before_any_device_call(lib, what):
    h = ctypes.c_void_p()
    rc = lib.imc_aln_open_phylip(b"x.phy", None) if what == "null out" else lib.imc_aln_open_phylip(None, ctypes.byref(h))
    assert rc == _capi.IMC_ERR_ARG and lib.imc_last_error() and h.value is None, (what, rc)


def test_a_missing_file_is_an_io_error_before_the_device_is_asked(lib, tmp_path):
    h = ctypes.c_void_p()
    assert lib.imc_aln_open_phylip(os.fsencode(str(tmp_path / "missing.phy")), ctypes.byref(h)) == _capi.IMC_ERR_IO
    assert b"cannot open" in lib.imc_last_error() and h.value is None
    with pytest.raises(IOError):
        Alignment(str(tmp_path / "missing.phy"), in_format="phylip")


def test_no_phylip_alignment_without_a_device(lib, tmp_path):
    if lib.imc_device_count() > 0:
        pytest.skip("a device is present")
    path = tmp_path / "two.phy"
    path.write_bytes(PHYLIP_CASES["seq-gen shape"])
    with pytest.raises(_capi.ImcError) as ei:
        Alignment(str(path), in_format="phylip")
    assert ei.value.code == _capi.IMC_ERR_NODEVICE


def test_an_unknown_format_is_a_value_error_before_any_library_call(tmp_path):
    with pytest.raises(ValueError, match="in_format"):
        Alignment(str(tmp_path / "missing.nex"), in_format="nexus")         # (a library call would say IOError: cannot open)


# ---- device code hygiene ------------------------------------------------------------------------------------------
def test_phylip_headers_hold_no_device_code_of_their_own():
    for name in ("phylip_io.hpp", "phylip_tiles.hpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert "#include <hip" not in text and "__global__" not in text and "threadIdx" not in text, name
    assert "k_phy_" not in open(os.path.join(CSRC, "kernels_align.hpp")).read()
    assert "kernels_phylip" not in open(os.path.join(CSRC, "kernels_align.hpp")).read()
    assert '#include "kernels_phylip.hpp"' in open(os.path.join(CSRC, "imcoal_fwd.hip")).read()


def test_phylip_kernels_use_no_scratch():
    src = '#include <hip/hip_runtime.h>\n#include "kernels_phylip.hpp"\n'
    seen = scratch_bytes(src, "k_phy_")
    kernels = ("k_phy_summary", "k_phy_scan", "k_phy_count", "k_phy_partial", "k_phy_offsets", "k_phy_scatter")
    for k in kernels:
        assert any(re.match(r"_Z\d+%s[A-Z]" % k, n) for n in seen), (k, sorted(seen))
    assert len(seen) == len(kernels) and all(v == 0 for v in seen.values()), seen
