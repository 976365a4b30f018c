"""Record what the host routine imc_model_expm returns for the matrices of
tests/test_models_cpu.py::test_native_expm_matches_scipy -> tests/golden/expm_host_golden.npz.

The file pins the host path bit for bit: it was written by the library as it stood BEFORE the Pade degree / squaring
choice moved into imc_model::expm_plan (shared with the device path), and tests/test_model_device_cpu.py compares the
current library's bytes with it.  Run it again only when the host algorithm is changed on purpose:

    python tests/golden/make_expm_host_golden.py
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

SIZES = (1, 2, 4, 15, 31)
SCALES = (1e-4, 1e-2, 0.2, 0.9, 2.0, 2.2, 4.5, 5.3, 6.0, 40.0, 900.0)


def matrices():
    """(n, scale, Q) in the order and with the generator of test_native_expm_matches_scipy."""
    rng = np.random.default_rng(5)
    for n in SIZES:
        for scale in SCALES:
            Q = rng.random((n, n)) * scale / n
            np.fill_diagonal(Q, 0.0)
            np.fill_diagonal(Q, -Q.sum(axis=1))
            yield n, scale, Q


def host_expm(lib, Q):
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    out = np.empty_like(Q)
    dp = ctypes.POINTER(ctypes.c_double)
    rc = lib.imc_model_expm(Q.shape[0], Q.ctypes.data_as(dp), out.ctypes.data_as(dp))
    assert rc == 0, lib.imc_last_error()
    return out


if __name__ == "__main__":
    from imcoalhmm_amd import _capi
    lib = _capi.lib()
    out = {}
    for n, scale, Q in matrices():
        out["n%d_s%g" % (n, scale)] = host_expm(lib, Q)
    np.savez_compressed(os.path.join(HERE, "expm_host_golden.npz"), **out)
    print("wrote %d matrices" % len(out))
