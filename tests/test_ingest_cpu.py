"""Device ingestion (csrc/ingest_tiles.hpp, csrc/kernels_ingest.hpp) and its entry points - imc_set_device_ingest,
imc_obs_create_pairwise, imc_last_ingest, Forwarder.from_sequences, prepare.pairwise_forwarders - as far as a machine
without a GPU can see them.  tests/ingest_tiles_check.cpp drives the functions the kernels call, tile by tile and slab by
slab, against the host parser's own loop under AddressSanitizer + UBSan; the rest are the symbols, the argument checks (they
run before any HIP call), the errors that need no device, and the kernels' register budget.  The symbols themselves are
compared with the host parser's on the device in tests/test_gpu_device_ingest.py."""
import ctypes
import os
import re

import pytest

from imcoalhmm_amd import Forwarder, _capi, build, hmm, prepare
from test_encode_tiles_cpu import run_check_under_asan_ubsan
from kernel_scratch_cases import scratch_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NEW = ("imc_set_device_ingest", "imc_obs_create_pairwise", "imc_last_ingest")


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _capi.lib()


def test_ingest_tiles_under_asan_ubsan(tmp_path):
    run_check_under_asan_ubsan(tmp_path, "ingest_tiles_check", "ingest_tiles ok")


def test_new_symbols_are_exported_declared_and_bound(lib):
    header = open(os.path.join(REPO, "include", "imcoal_fwd.h")).read()
    source = open(os.path.join(REPO, "imcoalhmm_amd", "csrc", "imcoal_fwd.hip")).read()
    names = [sig[0] for sig in _capi.SIGNATURES]
    for name in NEW:
        assert hasattr(lib, name)
        assert len(re.findall(r"^int %s\(" % name, header, flags=re.M)) == 1, name
        assert len(re.findall(r"^int %s\(" % name, source, flags=re.M)) == 1, name
        assert names.count(name) == 1
    by_name = {sig[0]: sig for sig in _capi.SIGNATURES}
    assert len(by_name["imc_obs_create_pairwise"][2]) == 4 and len(by_name["imc_last_ingest"][2]) == 1
    assert callable(hmm.set_device_ingest) and callable(Forwarder.from_sequences) and callable(prepare.pairwise_forwarders)
    assert callable(_capi.last_ingest)


def test_ingest_headers_hold_no_device_code_of_their_own():
    text = open(os.path.join(REPO, "imcoalhmm_amd", "csrc", "ingest_tiles.hpp")).read()
    assert "#include <hip" not in text and "__global__" not in text
    kernels = open(os.path.join(REPO, "imcoalhmm_amd", "csrc", "kernels_ingest.hpp")).read()
    assert "k_enc_" not in kernels
    assert "k_ing_" not in open(os.path.join(REPO, "imcoalhmm_amd", "csrc", "kernels_encode.hpp")).read()


@pytest.mark.parametrize("what", ["null out", "null seq1", "null seq2", "L 2^31"])
def test_create_pairwise_refuses_bad_arguments_before_any_device_call(lib, what):
    h = ctypes.c_void_p()
    args = dict(a=b"ACGT", b=b"ACGA", L=4, out=ctypes.byref(h))
    if what == "null out":
        args["out"] = None
    elif what == "null seq1":
        args["a"] = None
    elif what == "null seq2":
        args["b"] = None
    elif what == "L 2^31":
        args["L"] = 1 << 31                                                # (the length is refused before a byte is read)
    rc = lib.imc_obs_create_pairwise(args["a"], args["b"], args["L"], args["out"])
    assert rc == _capi.IMC_ERR_ARG, (what, rc, lib.imc_last_error())
    assert lib.imc_last_error()
    assert h.value is None


def test_switch_and_read_out_need_no_device(lib):
    for mode in (-1, 2, 7):
        assert lib.imc_set_device_ingest(mode) == _capi.IMC_ERR_ARG
        with pytest.raises(ValueError):
            hmm.set_device_ingest(mode)
    assert lib.imc_last_ingest(None) == _capi.IMC_ERR_ARG
    out = (ctypes.c_uint64 * 4)()
    assert lib.imc_last_ingest(out) == _capi.IMC_OK
    assert set(_capi.last_ingest()) == {"path", "bytes", "slabs", "columns"}
    assert lib.imc_set_device_ingest(1) == _capi.IMC_OK
    assert lib.imc_set_device_ingest(0) == _capi.IMC_OK                        # back to the default


def test_from_sequences_refuses_unequal_lengths_before_any_device_call(lib):
    with pytest.raises(ValueError, match="differ in length"):
        Forwarder.from_sequences("ACGT", "ACG")
    with pytest.raises(ValueError, match="differ in length"):
        Forwarder.from_sequences(b"ACGT", b"ACGTA")


def test_pairwise_forwarders_checks_its_arguments_first(lib, tmp_path):
    fa = tmp_path / "three.fa"
    fa.write_text(">a\nACGT\n>b\nACGA\n>c\nAC-T\n")
    with pytest.raises(KeyError):
        prepare.pairwise_forwarders(str(fa), pairs=[("a", "nobody")])
    with pytest.raises(ValueError):
        prepare.pairwise_forwarders(str(fa), in_format="nexus")
    assert prepare.pairwise_forwarders(str(fa), pairs=[]) == {}


@pytest.mark.parametrize("mode", [0, 1])
def test_errors_that_need_no_device_are_the_same_in_both_modes(lib, tmp_path, mode):
    """A path that does not exist, and what a cache header can get wrong, are found before the device is asked for."""
    magic = b"IMCOBS1\n"
    files = {
        "short header": magic + b"\x03\x00\x00\x00",
        "bad bits": magic + (3).to_bytes(4, "little") + (4).to_bytes(4, "little") + (8).to_bytes(8, "little") + b"\x00" * 8,
        "alphabet above nsym": magic + (4).to_bytes(4, "little") + (2).to_bytes(4, "little") + (8).to_bytes(8, "little") + b"\x00" * 2,
    }
    want = {"short header": (_capi.IMC_ERR_IO, b"truncated cache header"), "bad bits": (_capi.IMC_ERR_IO, b"bad cache header"),
            "alphabet above nsym": (_capi.IMC_ERR_SYMBOL, b"alphabet of 4 symbols")}
    try:
        assert lib.imc_set_device_ingest(mode) == _capi.IMC_OK
        h = ctypes.c_void_p()
        missing = os.fsencode(str(tmp_path / "missing.ziphmm"))
        assert lib.imc_obs_create_from_text(missing, 3, ctypes.byref(h)) == _capi.IMC_ERR_IO
        assert b"cannot open" in lib.imc_last_error() and h.value is None
        for name, data in files.items():
            path = tmp_path / (name.replace(" ", "_") + ".imc")
            path.write_bytes(data)
            rc = lib.imc_obs_create_from_text(os.fsencode(str(path)), 3, ctypes.byref(h))
            assert (rc, want[name][1] in lib.imc_last_error()) == (want[name][0], True), (name, rc, lib.imc_last_error())
            assert h.value is None
    finally:
        assert lib.imc_set_device_ingest(0) == _capi.IMC_OK


def test_ingest_kernels_use_no_scratch():
    src = '#include <hip/hip_runtime.h>\n#include "kernels_ingest.hpp"\n'
    seen = scratch_bytes(src, "k_ing_")
    kernels = ("k_ing_text_summary", "k_ing_scan", "k_ing_text_scatter", "k_ing_unpack2", "k_ing_pairwise")
    for k in kernels:
        assert any(re.match(r"_Z\d+%s[A-Z]" % k, n) for n in seen), (k, sorted(seen))
    assert len(seen) == len(kernels) and all(v == 0 for v in seen.values()), seen
