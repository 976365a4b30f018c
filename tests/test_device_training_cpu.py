"""The device trainer (csrc/kernels_train.hpp) and the entry points around it - imc_set_device_training,
imc_last_training, hmm.set_device_training, _capi.last_training - as far as a machine without a GPU can see them: the
symbols, the argument checks (they need no device) and the kernels' register budget.  The dictionaries are compared with
the host trainer's on the CPU in tests/test_train_tiles_cpu.py (the rules) and on the device in
tests/test_gpu_device_training.py (the kernels)."""
import ctypes
import os
import re

import pytest

from imcoalhmm_amd import _capi, build, hmm
from kernel_scratch_cases import scratch_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NEW = ("imc_set_device_training", "imc_last_training")


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
    assert len(by_name["imc_set_device_training"][2]) == 1 and len(by_name["imc_last_training"][2]) == 1
    assert callable(hmm.set_device_training) and callable(_capi.last_training)
    assert "training stays on the host" not in header and "training is the host's" not in header


def test_argument_errors_need_no_device(lib):
    for mode in (-1, 2, 7):
        assert lib.imc_set_device_training(mode) == _capi.IMC_ERR_ARG
        assert lib.imc_last_error()
        with pytest.raises(ValueError):
            hmm.set_device_training(mode)
    assert lib.imc_last_training(None) == _capi.IMC_ERR_ARG
    out = (ctypes.c_uint64 * 4)()
    assert lib.imc_last_training(out) == _capi.IMC_OK
    assert set(_capi.last_training()) == {"path", "symbols", "attempts", "rounds"}
    try:
        assert lib.imc_set_device_training(1) == _capi.IMC_OK
        hmm.set_device_training(1)
    finally:
        assert lib.imc_set_device_training(0) == _capi.IMC_OK                  # back to the default


def test_trainer_kernels_use_no_scratch():
    """The method of test_device_encode_cpu.py::test_encoder_kernels_use_no_scratch; kernels_train.hpp includes
    kernels_encode.hpp, whose kernels that test covers, so only the k_trn_ ones are looked at here."""
    src = ('#include <hip/hip_runtime.h>\n#include "kernels_train.hpp"\n'
           'template __global__ void k_trn_pair_hist<true>(const uint16_t *, uint32_t, uint32_t, uint32_t *);\n'
           'template __global__ void k_trn_pair_hist<false>(const uint16_t *, uint32_t, uint32_t, uint32_t *);\n')
    seen = scratch_bytes(src, "k_trn_")
    kernels = ("k_trn_load", "k_trn_pair_histILb1E", "k_trn_pair_histILb0E", "k_trn_argmax", "k_trn_pair_count", "k_trn_candidates")
    for k in kernels:
        assert any(re.match(r"_Z\d+%s[A-Z]" % k, n) for n in seen), (k, sorted(seen))
    assert len(seen) == len(kernels) and all(v == 0 for v in seen.values()), seen
