"""Shared by tests/test_sample_cpu.py, tests/test_gpu_sample.py and the scripts the latter starts: the HMM recipes, an
independent numpy implementation of the sampler's specification (include/imcoal_sample.h: uint64 Philox, np.cumsum tables)
and thin ctypes wrappers of imc_sample_host / imc_sample_device."""
import ctypes

import numpy as np

from imcoalhmm_amd import _capi

KINDS = ("sticky", "fast-mixing", "sparse", "cyclic", "absorbing", "banded", "unnormalised")
MASK = np.uint64(0xFFFFFFFF)


def transitions(kind, n, rng):
    T = np.zeros((n, n))
    if kind == "sticky":
        T = 0.001 * rng.random((n, n)) / n + 0.999 * np.eye(n)
    elif kind == "fast-mixing":
        T = rng.random((n, n)) + 1e-3
    elif kind == "sparse":
        for i in range(n):
            for j in rng.integers(0, n, size=3):
                T[i, j] += rng.random() + 0.05
    elif kind == "cyclic":                                   # every column's map is a bijection
        T[np.arange(n), (np.arange(n) + 1) % n] = 1.0
    elif kind == "absorbing":
        T = rng.random((n, n)) + 1e-3
        T[n // 2] = 0.0
        T[n // 2, n // 2] = 1.0
    elif kind == "banded":                                   # leading and trailing zeros in every row
        lo, hi = n // 4, max(n // 4 + 1, 3 * n // 4)
        T[:, lo:hi] = rng.random((n, hi - lo)) + 1e-3
    elif kind == "unnormalised":
        T = (rng.random((n, n)) + 1e-3) * (0.1 + 50.0 * rng.random((n, 1)))
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(T)


def hmm(kind, n, S, seed):
    rng = np.random.default_rng([seed, n, KINDS.index(kind)])
    T = transitions(kind, n, rng)
    pi = rng.random(n) + 1e-3
    if n > 2:
        pi[0] = pi[-1] = 0.0
    E = rng.random((n, S)) + 0.05
    return pi, T, E


# ---- the independent implementation -------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """uint64 arrays (or scalars) holding 32-bit words -> the four output words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    m0, m1, w0, w1, s32 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & MASK, (p0 >> s32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + w0) & MASK, (k1 + w1) & MASK
    return c0, c1, c2, c3


def uniforms(seed, tag, replicate, L):
    t = np.arange(L, dtype=np.uint64)
    ones = np.ones(L, dtype=np.uint64)
    w = philox4x32_10(t & MASK, t >> np.uint64(32), ones * np.uint64(replicate), ones * np.uint64(tag), seed & 0xFFFFFFFF, seed >> 32)
    to_unit = lambda lo, hi: (((hi << np.uint64(32)) | lo) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return to_unit(w[0], w[1]), to_unit(w[2], w[3])


def thresholds(row):
    c = np.cumsum(np.asarray(row, dtype=np.float64))
    cdf = c / c[-1]                                            # the LAST running sum, not np.sum (pairwise)
    cdf[np.flatnonzero(np.asarray(row) > 0)[-1]:] = 1.0
    return cdf


def reference_sample(pi, T, E, emit, seed, tag, R, L, first_replicate=0):
    """Replicates first_replicate .. first_replicate + R - 1."""
    n = len(pi)
    cpi = thresholds(pi)
    cT = [thresholds(T[i]) for i in range(n)]
    cE = [thresholds(E[i, :emit]) for i in range(n)]
    sym = np.zeros((R, L), dtype=np.int64)
    states = np.zeros((R, L), dtype=np.int64)
    for r in range(R):
        us, uy = uniforms(seed, tag, first_replicate + r, L)
        us = us.tolist()
        x = states[r]
        s = x[0] = int(np.searchsorted(cpi, us[0], side="right"))
        for t in range(1, L):
            s = x[t] = int(np.searchsorted(cT[s], us[t], side="right"))
        for i in range(n):
            at = np.flatnonzero(x == i)
            sym[r, at] = np.searchsorted(cE[i], uy[at], side="right")
    return sym, states


# ---- the library -----------------------------------------------------------------------------------
def _head(pi, T, E, emit, seed, tag, R, L):
    pi, T, E = _capi.as_f64(pi), _capi.as_f64(T), _capi.as_f64(E)
    return (pi, T, E), (len(pi), E.shape[1], emit, _capi.dptr(pi), _capi.dptr(T), _capi.dptr(E), seed, tag, R, L)


def host_sample(pi, T, E, emit, seed, tag, R, L, states=True):
    keep, head = _head(pi, T, E, emit, seed, tag, R, L)
    wide = emit > 256
    sym = np.full((R, L), 0xEE, dtype=np.uint16 if wide else np.uint8)
    st = np.full((R, L), 0xEE, dtype=np.uint8) if states else None
    _capi.check(_capi.lib().imc_sample_host(*head, sym.ctypes.data, 2 if wide else 1, st.ctypes.data if states else None))
    return sym, st


def device_sample(torch, pi, T, E, emit, seed, tag, R, L, states=True, stream=None):
    """imc_sample_device into poisoned torch tensors with a guard band behind them -> numpy (symbols, states or None)."""
    keep, head = _head(pi, T, E, emit, seed, tag, R, L)
    wide = emit > 256
    pad = 64
    sym = torch.full((R * L + pad,), 0x6E, dtype=torch.int16 if wide else torch.uint8, device="cuda")
    st = torch.full((R * L + pad,), 0x6E, dtype=torch.uint8, device="cuda") if states else None
    torch.cuda.synchronize()
    _capi.check(_capi.lib().imc_sample_device(*head, sym.data_ptr(), 2 if wide else 1, st.data_ptr() if states else None, stream))
    sym, st = sym.cpu().numpy(), st.cpu().numpy() if states else None
    assert (sym[R * L:] == 0x6E).all() and (st is None or (st[R * L:] == 0x6E).all()), "written past the end of the output"
    sym = sym[:R * L].reshape(R, L)
    return (sym.view(np.uint16) if wide else sym), (st[:R * L].reshape(R, L) if states else None)


def last_sampling():
    arr = (ctypes.c_uint64 * 4)()
    _capi.check(_capi.lib().imc_last_sampling(arr))
    return [int(x) for x in arr]
