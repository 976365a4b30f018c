"""Resident alignments (csrc/fasta_io.hpp, csrc/align_tiles.hpp, csrc/kernels_align.hpp) and their entry points -
imc_aln_*, imc_obs_create_from_alignment, imc_read_fasta, imc_encode_triplet, Alignment, Forwarder.from_alignment, the
triplet branch of prepare - as far as a machine without a GPU can see them.  tests/align_tiles_check.cpp drives the
functions the kernels call, tile by tile and slab by slab, against the host reader under AddressSanitizer + UBSan; the host
reader itself is held to prepare.read_fasta here; the rest are the symbols, the argument checks that need no alignment,
the errors that need no device, and the kernels' register budget.  Parsed sequences and chunks are compared on the device
in tests/test_gpu_alignment.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import imcoalhmm_amd
from imcoalhmm_amd import Alignment, Forwarder, _capi, build, prepare
from test_encode_tiles_cpu import run_check_under_asan_ubsan
from kernel_scratch_cases import scratch_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NEW = {"imc_read_fasta": "int", "imc_encode_triplet": "int", "imc_aln_open_fasta": "int", "imc_aln_count": "int",
       "imc_aln_name": r"const char \*", "imc_aln_length": "size_t ", "imc_aln_sequence": "int", "imc_aln_info": "int",
       "imc_aln_free": "int", "imc_obs_create_from_alignment": "int"}


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _capi.lib()


def test_align_tiles_under_asan_ubsan(tmp_path):
    run_check_under_asan_ubsan(tmp_path, "align_tiles_check", "align_tiles ok")


# ---- the host reader against prepare.read_fasta ---------------------------------------------------------------
FASTA_CASES = {
    "plain": b">a\nACGT\nAC\n>b\nTTTTGG\n",
    "crlf": b">a\r\nACGT\r\nAC\r\n>b\r\nTTTTGG\r\n",
    "lone cr": b">a\rACGT\rAC\r>b\rTTTTGG\r",
    "mixed breaks": b">a\nAC\rGT\r\nAC\n\r>b\r\r\nTT\n",
    "trailing blanks": b">a  \nACGT \t\nAC\x1c\n>b\t\nTTTTGG\x0b\x0c\n",
    "interior blanks": b">a\nAC GT\nA\tC\n>b\nTT TT GG\n",
    "leading blanks": b"  >a\n  ACGT\n\t>b\nTT\n",
    "blank lines": b"\n\n>a\n\nACGT\n   \n\nAC\n>b\n\n\n",
    "text before the first header": b"; a comment\nACGT\n>a\nAC\n",
    "description": b">a some description here\nACGT\n>b\tdesc\nTT\n> c spaced\nGG\n",
    "duplicate name": b">a\nAC\n>b\nGG\n>a\nTTT\n>c\nA\n",
    "duplicate name, last empty": b">a\nAC\n>b\nGG\n>a\n",
    "no final newline": b">a\nACGT\n>b\nTT",
    "header at the end": b">a\nACGT\n>b",
    "empty record": b">a\n>b\nACGT\n>c\n\n>d\nA\n",
    "no record": b"ACGT\nAC\n",
    "empty file": b"",
    "greater-than inside a line": b">a\nAC>GT\nA>\n",
    "control bytes": b">a\x1fx\nAC\x01GT\n\x1d\n>b\x01\nA\x7f\n",
}


@pytest.mark.parametrize("case", sorted(FASTA_CASES))
def test_read_fasta_is_prepares(lib, tmp_path, case):
    path = tmp_path / "x.fa"
    path.write_bytes(FASTA_CASES[case])
    want = prepare.read_fasta(str(path))
    got = prepare.read_fasta_native(str(path))
    assert list(got) == list(want), case
    assert {k: v.decode("ascii") for k, v in got.items()} == want, case


@pytest.mark.parametrize("data, needle", [(b">a\nAC\n>\nGG\n", b"header without a name"), (b">a\nAC\n>   \n", b"header without a name"),
                                          (b">a\nAC\xc3\xa9\n", b"non-ASCII byte"), (b">a\xff\nAC\n", b"non-ASCII byte")])
def test_read_fasta_deviations_are_io_errors(lib, tmp_path, data, needle):
    path = tmp_path / "bad.fa"
    path.write_bytes(data)
    count, length = ctypes.c_int(-1), ctypes.c_size_t(0)
    rc = lib.imc_read_fasta(os.fsencode(str(path)), -1, None, 0, None, 0, ctypes.byref(length), ctypes.byref(count))
    assert rc == _capi.IMC_ERR_IO and needle in lib.imc_last_error(), (rc, lib.imc_last_error())
    with pytest.raises(IOError):
        prepare.read_fasta_native(str(path))
    assert lib.imc_read_fasta(os.fsencode(str(tmp_path / "missing.fa")), -1, None, 0, None, 0, ctypes.byref(length), ctypes.byref(count)) == _capi.IMC_ERR_IO
    assert b"cannot open" in lib.imc_last_error()
    assert lib.imc_read_fasta(None, -1, None, 0, None, 0, ctypes.byref(length), ctypes.byref(count)) == _capi.IMC_ERR_ARG


# ---- triplets ---------------------------------------------------------------------------------------------------
def test_encode_triplet_by_hand(lib):
    s1, s2, s3 = "ACGTacgtAN-A", "AAAAccccTAAx", "AAAAAAAAGAAA"
    want = [0, 1, 2, 3, 4, 5, 6, 7, 0 + 4 * 3 + 16 * 2, 64, 64, 64]
    assert prepare.encode_triplet(s1, s2, s3).tolist() == want
    out = np.full(12, 255, dtype=np.uint8)
    assert lib.imc_encode_triplet(s1.encode(), s2.encode(), s3.encode(), 12, out.ctypes.data_as(_capi._u8p)) == _capi.IMC_OK
    assert out.tolist() == want
    assert prepare.encode_triplet("TTT", "TTT", "TTT").tolist() == [63, 63, 63]
    assert lib.imc_encode_triplet(None, b"A", b"A", 1, out.ctypes.data_as(_capi._u8p)) == _capi.IMC_ERR_ARG
    with pytest.raises(ValueError):
        prepare.encode_triplet("ACG", "AC", "ACG")


def test_prepare_cli_writes_triplets_and_keeps_pairs(lib, tmp_path):
    fa = tmp_path / "x.fa"
    fa.write_text(">a desc\nACGTNAC\nGT\n>b\nACCTAAC\nGA\n>c\nAAAAAAAAA\n")       # the file of test_prepare_cli_on_fasta_and_phylip
    out = tmp_path / "abc.txt"
    assert prepare.main([str(fa), str(out), "--names", "a,b,c"]) == 0
    assert out.read_text() == "0 5 6 15 64 0 5 10 3 "
    cache = tmp_path / "abc.imc"
    assert prepare.main([str(fa), str(cache), "--names", "c,b,a", "--cache"]) == 0
    assert prepare.read_observations(str(cache), 65).tolist() == [0, 20, 36, 60, 64, 0, 20, 40, 48]
    pair = tmp_path / "ab.txt"
    assert prepare.main([str(fa), str(pair), "--names", "a,b"]) == 0
    assert pair.read_text() == "0 0 1 0 2 0 0 0 1 "
    first_two = tmp_path / "first.txt"
    assert prepare.main([str(fa), str(first_two)]) == 0
    assert first_two.read_text() == "0 0 1 0 2 0 0 0 1 "
    with pytest.raises(SystemExit):
        prepare.main([str(fa), str(out), "--names", "a,b,c,a"])


# ---- the boundary -----------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_declared_and_bound(lib):
    header = open(os.path.join(REPO, "include", "imcoal_fwd.h")).read()
    source = open(os.path.join(REPO, "imcoalhmm_amd", "csrc", "imcoal_fwd.hip")).read()
    names = [sig[0] for sig in _capi.SIGNATURES]
    for name, returns in NEW.items():
        assert hasattr(lib, name)
        assert len(re.findall(r"^%s ?%s\(" % (returns, name), header, flags=re.M)) == 1, name
        assert len(re.findall(r"^%s ?%s\(" % (returns, name), source, flags=re.M)) == 1, name
        assert names.count(name) == 1
    assert "typedef struct imc_aln imc_aln;" in header
    by_name = {sig[0]: sig for sig in _capi.SIGNATURES}
    assert len(by_name["imc_obs_create_from_alignment"][2]) == 4 and len(by_name["imc_read_fasta"][2]) == 8
    assert imcoalhmm_amd.Alignment is Alignment and "Alignment" in imcoalhmm_amd.__all__
    assert callable(Forwarder.from_alignment) and callable(prepare.encode_triplet)
    for method in ("sequence", "forwarder", "pairs", "close", "__enter__", "__exit__"):
        assert callable(getattr(Alignment, method))


@pytest.mark.parametrize("what", ["null out", "null out of open", "null path", "k 1", "k 4", "null alignment", "null members"])
def test_argument_errors_before_any_device_call(lib, what):
    h = ctypes.c_void_p()
    members = (ctypes.c_int32 * 3)(0, 1, 2)
    fake = ctypes.c_void_p(0)                                              # no alignment can exist without a device
    if what == "null out of open":
        rc = lib.imc_aln_open_fasta(b"x.fa", None)
    elif what == "null path":
        rc = lib.imc_aln_open_fasta(None, ctypes.byref(h))
    elif what == "null out":
        rc = lib.imc_obs_create_from_alignment(fake, members, 2, None)
    elif what in ("k 1", "k 4"):
        rc = lib.imc_obs_create_from_alignment(fake, members, int(what[2:]), ctypes.byref(h))
    elif what == "null alignment":
        rc = lib.imc_obs_create_from_alignment(None, members, 3, ctypes.byref(h))
    else:
        somewhere = ctypes.create_string_buffer(4096)                      # never looked at: the null check comes first
        rc = lib.imc_obs_create_from_alignment(ctypes.addressof(somewhere), None, 2, ctypes.byref(h))
    assert rc == _capi.IMC_ERR_ARG, (what, rc, lib.imc_last_error())
    assert lib.imc_last_error()
    assert h.value is None


def test_handles_that_are_null(lib):
    assert lib.imc_aln_free(None) == _capi.IMC_OK
    assert lib.imc_aln_count(None) == 0 and lib.imc_aln_length(None, 0) == 0 and lib.imc_aln_name(None, 0) is None
    out = (ctypes.c_uint64 * 4)()
    assert lib.imc_aln_info(None, out) == _capi.IMC_ERR_ARG
    assert lib.imc_aln_sequence(None, 0, None, 0) == _capi.IMC_ERR_ARG


def test_a_missing_file_is_an_io_error_before_the_device_is_asked(lib, tmp_path):
    h = ctypes.c_void_p()
    assert lib.imc_aln_open_fasta(os.fsencode(str(tmp_path / "missing.fa")), ctypes.byref(h)) == _capi.IMC_ERR_IO
    assert b"cannot open" in lib.imc_last_error() and h.value is None
    with pytest.raises(IOError):
        Alignment(str(tmp_path / "missing.fa"))


def test_no_alignment_without_a_device(lib, tmp_path):
    if lib.imc_device_count() > 0:
        pytest.skip("a device is present")
    fa = tmp_path / "two.fa"
    fa.write_text(">a\nACGT\n>b\nACGA\n")
    with pytest.raises(_capi.ImcError) as ei:
        Alignment(str(fa))
    assert ei.value.code == _capi.IMC_ERR_NODEVICE


def test_last_ingest_names_the_alignment_path(lib):
    text = open(os.path.join(REPO, "imcoalhmm_amd", "_capi.py")).read()
    assert '("host", "text", "cache", "pairwise", "alignment")' in text
    assert set(_capi.last_ingest()) == {"path", "bytes", "slabs", "columns"}


# ---- device code hygiene ------------------------------------------------------------------------------------------
def test_alignment_headers_hold_no_device_code_of_their_own():
    for name in ("align_tiles.hpp", "fasta_io.hpp"):
        text = open(os.path.join(REPO, "imcoalhmm_amd", "csrc", name)).read()
        assert "#include <hip" not in text and "__global__" not in text and "threadIdx" not in text, name
    kernels = open(os.path.join(REPO, "imcoalhmm_amd", "csrc", "kernels_align.hpp")).read()
    assert "k_ing_" not in kernels.replace("k_ing_scan's", "") and "k_enc_" not in kernels
    assert "k_aln_" not in open(os.path.join(REPO, "imcoalhmm_amd", "csrc", "kernels_ingest.hpp")).read()


def test_alignment_kernels_use_no_scratch():
    src = ('#include <hip/hip_runtime.h>\n#include "kernels_align.hpp"\n'
           'template __global__ void k_aln_columns<2>(const uint8_t *, uint64_t, uint64_t, uint64_t, uint32_t, uint8_t *);\n'
           'template __global__ void k_aln_columns<3>(const uint8_t *, uint64_t, uint64_t, uint64_t, uint32_t, uint8_t *);\n')
    seen = scratch_bytes(src, "k_aln_")
    kernels = ("k_aln_summary", "k_aln_scan", "k_aln_scatter", "k_aln_columnsILi2E", "k_aln_columnsILi3E")
    for k in kernels:
        assert any(re.match(r"_Z\d+%s[A-Z]" % k, n) for n in seen), (k, sorted(seen))
    assert len(seen) == len(kernels) and all(v == 0 for v in seen.values()), seen
