"""Alignments drawn from an HMM (pi, T, E) on the device: simulated replicates for the simulate -> prepare -> estimate loop
(the reference's simulations/*/simulate.sh) and for parametric bootstraps of ``maximum_likelihood_estimate``.

``sample`` is ``imc_sample_device`` / ``imc_sample_host`` (include/imcoal_sample.h): hidden paths and symbols from counter
based uniforms, exactly reproducible from ``(seed, tag)`` and the same bytes on both paths.  ``forwarders`` hands the
device symbols to ``Forwarder.from_device``, so a replicate becomes a chunk without a symbol on the host.
"""
import ctypes

import numpy as np

from . import _capi
from .hmm import Forwarder

MISSING_TAG = 1          # the uniforms of the missing-data overlay: the same seed, another stream


def _tables(pi, T, E, emit_symbols):
    pi = _capi.as_f64(np.asarray(pi)).reshape(-1)
    n = pi.shape[0]
    T = _capi.as_f64(np.asarray(T), (n, n))
    E = _capi.as_f64(np.asarray(E))
    if E.ndim != 2 or E.shape[0] != n:
        raise ValueError("E must be (%d,S), got %r" % (n, E.shape))
    emit = E.shape[1] if emit_symbols is None else int(emit_symbols)
    return pi, T, E, emit


def last_sampling():
    """Dict view of imc_last_sampling(): ``path`` 0 (host) or 1 (device), ``tiles``, ``tile`` (length) and ``columns`` of
    the last call."""
    arr = (ctypes.c_uint64 * 4)()
    _capi.check(_capi.lib().imc_last_sampling(arr))
    return dict(zip(("path", "tiles", "tile", "columns"), [int(x) for x in arr]))


def sample(pi, T, E, length, seed, replicates=1, emit_symbols=None, tag=0, return_states=False, where="device", stream=None):
    """``replicates`` independent paths of ``length`` columns from (pi, T, E); only the first ``emit_symbols`` columns of
    ``E`` are drawn from (default: all; pairwise models keep missing data in column 2 and sample with 2).

    ``where="device"``: torch tensors of shape ``(replicates, length)`` on the library's device - uint8 symbols, int16 beyond
    256 symbols - written by the kernels on ``stream`` (a handle or an object with ``cuda_stream``; default: torch's current
    stream), which is synchronised before the call returns.  ``where="host"``: numpy arrays (uint8 / uint16) from the
    sequential specification, the same values.  With ``return_states`` the result is ``(symbols, states)``."""
    pi, T, E, emit = _tables(pi, T, E, emit_symbols)
    n, S = pi.shape[0], E.shape[1]
    R, L = int(replicates), int(length)
    wide = emit > 256
    lib = _capi.lib()
    head = (n, S, emit, _capi.dptr(pi), _capi.dptr(T), _capi.dptr(E), int(seed) & 0xFFFFFFFFFFFFFFFF, int(tag) & 0xFFFFFFFF, R, max(L, 0))
    shape = (max(R, 0), max(L, 0))
    if where == "host":
        sym = np.zeros(shape, dtype=np.uint16 if wide else np.uint8)
        states = np.zeros(shape, dtype=np.uint8) if return_states else None
        _capi.check(lib.imc_sample_host(*head, sym.ctypes.data, 2 if wide else 1, states.ctypes.data if return_states else None))
        return (sym, states) if return_states else sym
    if where != "device":
        raise ValueError("where must be \"device\" or \"host\", got %r" % (where,))
    import torch
    if stream is None:
        stream = torch.cuda.current_stream()
    handle = stream if isinstance(stream, int) else stream.cuda_stream
    dev = torch.device("cuda", torch.cuda.current_device())
    sym = torch.empty(shape, dtype=torch.int16 if wide else torch.uint8, device=dev)
    states = torch.empty(shape, dtype=torch.uint8, device=dev) if return_states else None
    _capi.check(lib.imc_sample_device(*head, sym.data_ptr() or None, 2 if wide else 1, states.data_ptr() if return_states else None,
                                      handle or None))
    return (sym, states) if return_states else sym


def missing_chain(fraction, mean_run):
    """(pi, T, E) of the two-state chain behind ``missing=``: state 1 = missing, runs of mean length ``mean_run``, a
    stationary share ``fraction`` of the columns, started from the stationary distribution; identity emissions."""
    fraction, mean_run = float(fraction), float(mean_run)
    if not 0.0 < fraction < 1.0 or not mean_run >= 1.0:
        raise ValueError("missing needs 0 < fraction < 1 and mean_run >= 1, got %r, %r" % (fraction, mean_run))
    leave = 1.0 / mean_run
    enter = fraction * leave / (1.0 - fraction)
    if enter > 1.0:
        raise ValueError("missing: fraction %r cannot be reached with runs of mean length %r" % (fraction, mean_run))
    return (np.array([1.0 - fraction, fraction]), np.array([[1.0 - enter, enter], [leave, 1.0 - leave]]), np.eye(2))


def sample_with_missing(pi, T, E, length, seed, replicates=1, emit_symbols=None, missing=None):
    """``sample(..., where="device")`` with the missing-data overlay ``missing=(symbol, fraction, mean_run)``: a second
    chain (``missing_chain``, tag 1 of the same seed) through the same entry point marks the columns that read ``symbol``."""
    sym = sample(pi, T, E, length, seed, replicates=replicates, emit_symbols=emit_symbols)
    if missing is None:
        return sym
    import torch
    symbol, fraction, mean_run = missing
    mask = sample(*missing_chain(fraction, mean_run), length, seed, replicates=replicates, tag=MISSING_TAG)
    return torch.where(mask != 0, torch.full_like(sym, int(symbol)), sym)


def forwarders(pi, T, E, length, seed, replicates=1, emit_symbols=None, missing=None):
    """One ``Forwarder`` per simulated replicate, ``NSYM = E.shape[1]``, through ``Forwarder.from_device``: no symbol visits
    the host."""
    sym = sample_with_missing(pi, T, E, length, seed, replicates=replicates, emit_symbols=emit_symbols, missing=missing)
    import torch
    nsym = int(np.asarray(E).shape[1])
    return [Forwarder.from_device(sym[r], nsym, stream=torch.cuda.current_stream()) for r in range(sym.shape[0])]
