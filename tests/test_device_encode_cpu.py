"""The device encoder (csrc/kernels_encode.hpp) and the entry points around it - imc_obs_create_device,
imc_obs_token_counts, imc_set_device_encoding, Forwarder.from_device - as far as a machine without a GPU can see them:
the symbols, the argument checks (they run before any HIP call), the input checks of from_device, and the kernels'
register budget.  The tokens are compared with the host encoder's on the device in tests/test_gpu_device_encode.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from imcoalhmm_amd import Forwarder, _capi, build, hmm
from kernel_scratch_cases import scratch_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NEW = ("imc_obs_create_device", "imc_obs_token_counts", "imc_set_device_encoding")


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _capi.lib()


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
    assert len(by_name["imc_obs_create_device"][2]) == 6 and len(by_name["imc_obs_token_counts"][2]) == 5
    assert callable(hmm.set_device_encoding) and callable(Forwarder.from_device) and callable(Forwarder.token_counts)


@pytest.mark.parametrize("what", ["null out", "null symbols", "sym_bytes 3", "sym_bytes 0", "sym_bytes 8", "nsym 0", "nsym 4097",
                                  "bytes with nsym 257", "L 2^31"])
def test_create_device_refuses_bad_arguments_before_any_device_call(lib, what):
    h = ctypes.c_void_p()
    args = dict(ptr=0x1000, L=100, nsym=3, size=1, out=ctypes.byref(h))       # (the address is never dereferenced)
    if what == "null out":
        args["out"] = None
    elif what == "null symbols":
        args["ptr"] = None
    elif what.startswith("sym_bytes"):
        args["size"] = int(what.split()[1])
    elif what.startswith("nsym"):
        args.update(nsym=int(what.split()[1]), size=4)
    elif what == "bytes with nsym 257":
        args["nsym"] = 257
    elif what == "L 2^31":
        args["L"] = 1 << 31
    rc = lib.imc_obs_create_device(args["ptr"], args["L"], args["nsym"], args["size"], None, args["out"])
    assert rc == _capi.IMC_ERR_ARG, (what, rc, lib.imc_last_error())
    assert lib.imc_last_error()
    assert h.value is None


def test_other_argument_errors_need_no_device(lib):
    used = ctypes.c_int(0)
    assert lib.imc_obs_token_counts(None, 256, None, 0, ctypes.byref(used)) == _capi.IMC_ERR_ARG
    for mode in (-1, 2, 7):
        assert lib.imc_set_device_encoding(mode) == _capi.IMC_ERR_ARG
        with pytest.raises(ValueError):
            hmm.set_device_encoding(mode)
    assert lib.imc_set_device_encoding(1) == _capi.IMC_OK
    assert lib.imc_set_device_encoding(0) == _capi.IMC_OK                      # back to the default


def test_valid_create_device_without_a_device_says_so(lib):
    if lib.imc_device_count() > 0:
        pytest.skip("a device is present: tests/test_gpu_device_encode.py runs the call")
    h = ctypes.c_void_p()
    assert lib.imc_obs_create_device(0x1000, 100, 3, 1, None, ctypes.byref(h)) == _capi.IMC_ERR_NODEVICE


class _FakeDeviceArray(object):
    """Only the interface dictionary: from_device must refuse these inputs before it looks at the address."""

    def __init__(self, shape, typestr, strides=None):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "strides": strides, "data": (0x1000, False), "version": 2}


@pytest.mark.parametrize("arr", [_FakeDeviceArray((50,), "|u1", (2,)), _FakeDeviceArray((50,), "<i4", (8,)),
                                 _FakeDeviceArray((10, 5), "|u1"), _FakeDeviceArray((), "|u1"),
                                 _FakeDeviceArray((50,), "<f4"), _FakeDeviceArray((50,), "<f8"), _FakeDeviceArray((50,), "<i8")],
                         ids=["strided-u1", "strided-i4", "2-D", "0-D", "float32", "float64", "int64"])
def test_from_device_refuses_what_it_cannot_take(lib, arr):
    with pytest.raises(ValueError):
        Forwarder.from_device(arr, 3)
    with pytest.raises(ValueError):
        Forwarder.from_device(np.zeros(8, dtype=np.uint8), 3)                   # host arrays have no device interface


def test_encoder_kernels_use_no_scratch():
    src = '#include <hip/hip_runtime.h>\n#include "kernels_encode.hpp"\n'
    seen = scratch_bytes(src, "k_enc_")
    kernels = ("k_enc_summary", "k_enc_scan", "k_enc_scatter", "k_enc_mark_summary", "k_enc_mark_scatter", "k_enc_snapshot",
               "k_enc_histogram", "k_enc_load", "k_enc_validate", "k_enc_narrow")
    for k in kernels:
        assert any(re.match(r"_Z\d+%s[A-Z]" % k, n) for n in seen), (k, sorted(seen))
    assert len(seen) == len(kernels) and all(v == 0 for v in seen.values()), seen
