"""Shared by tests/test_gpu_device_encode.py and the guard-mode script it starts: the data recipes, the level list of
csrc/pair_dict.hpp and the chunk-against-chunk comparison (lengths, tokens and token counts at every level, exact)."""
import ctypes

import numpy as np

from imcoalhmm_amd import Forwarder, _capi
from imcoalhmm_amd.hmm import set_device_encoding

K_LEVELS = (8, 12, 16, 24, 32, 44, 64, 96, 128, 192, 256, 384, 512, 768, 1024, 1536, 2048, 3072, 4096, 6144, 8192, 12288, 16384)
LENGTHS = (4096, 4097, 8191, 8192, 8193, 12289, 65537, 300000)
CONTENTS = ("compressible", "zeros", "one-at-4095", "one-at-4096", "one-at-4097", "alternating", "period-3")
_u16p = ctypes.POINTER(ctypes.c_uint16)


def compressible(n, seed, nsym=3):
    """The recipe of tests/test_gpu_parity.py (test_wide_token_levels)."""
    rng = np.random.default_rng(seed)
    p = np.full(nsym, 0.1 / max(nsym - 1, 1)); p[0] = 0.9
    return rng.choice(nsym, size=n, p=p / p.sum()).astype(np.uint8)


def skewed_symbols(n, nsym, seed):
    """The recipe of tests/test_gpu_parity.py (_skewed_symbols): three frequent symbols, the rest rare."""
    rng = np.random.default_rng(seed)
    hot = np.array([0, nsym // 2, nsym - 1])
    obs = np.where(rng.random(n) < 0.9, hot[rng.integers(0, 3, size=n)], rng.integers(0, nsym, size=n))
    return obs.astype(np.int32)


def content(kind, n):
    """One of CONTENTS at length n, or None where the case does not exist (a single 1 at a column the chunk lacks)."""
    if kind == "compressible":
        return compressible(n, seed=1000 + n)
    obs = np.zeros(n, dtype=np.uint8)
    if kind.startswith("one-at-"):
        col = int(kind.split("-")[-1])
        if col >= n:
            return None
        obs[col] = 1
    elif kind == "alternating":
        obs[1::2] = 1
    elif kind == "period-3":
        obs[2::3] = 1                                                  # 0 0 1 0 0 1 ...
    return obs


def tokens(f, limit):
    L = _capi.lib()
    n, used = ctypes.c_size_t(0), ctypes.c_int(0)
    _capi.check(L.imc_obs_tokens(f.handle, limit, None, 0, ctypes.byref(n), ctypes.byref(used)))
    out = np.zeros(max(n.value, 1), dtype=np.uint16)
    _capi.check(L.imc_obs_tokens(f.handle, limit, out.ctypes.data_as(_u16p), n.value, ctypes.byref(n), ctypes.byref(used)))
    return out[:n.value], used.value


def assert_same_chunk(a, b, what):
    """Every level: equal compressed_length, equal imc_obs_tokens, equal token_counts."""
    assert len(a) == len(b), what
    for limit in K_LEVELS:
        assert a.compressed_length(limit) == b.compressed_length(limit), (what, limit, a.compressed_length(limit), b.compressed_length(limit))
        ta, ua = tokens(a, limit)
        tb, ub = tokens(b, limit)
        assert ua == ub and ta.size == tb.size, (what, limit, ua, ub, ta.size, tb.size)
        diff = np.flatnonzero(ta != tb)
        assert diff.size == 0, (what, limit, int(diff[0]), ta[diff[0]:diff[0] + 8], tb[diff[0]:diff[0] + 8])
        ca, cb = a.token_counts(limit), b.token_counts(limit)
        assert ca.size == cb.size == ua and (ca == cb).all(), (what, limit, np.flatnonzero(ca != cb)[:8])


def train3():
    """The 3-symbol dictionary of test_wide_token_levels, trained by the host path; returns (forwarder, alphabet)."""
    L = _capi.lib()
    set_device_encoding(0)
    _capi.check(L.imc_set_compression(1))
    _capi.check(L.imc_dictionary_reset())
    f = Forwarder.from_array(compressible(3_000_000, seed=5), 3)
    alpha = f.compressed_length(16384)[1]
    assert alpha > 1024, alpha                                           # the 16-bit rounds run
    return f, alpha


def host_and_device(obs, nsym):
    """The same symbols as a chunk encoded on the host (switch 0) and one encoded on the device (switch 1)."""
    try:
        set_device_encoding(0)
        a = Forwarder.from_array(obs, nsym)
        set_device_encoding(1)
        b = Forwarder.from_array(obs, nsym)
    finally:
        set_device_encoding(0)
    return a, b


def _raises_value_error(fn, needle):
    try:
        fn()
    except ValueError as e:
        assert needle in str(e), (needle, str(e))
        return
    raise AssertionError("no ValueError (%s)" % needle)


def from_device_cases(torch, oracle, tol=1e-11):
    """Forwarder.from_device on torch tensors against chunks built from the same symbols on the host: tokens and counts at
    every level, per-chunk log-likelihoods bit for bit (automatic mode at 10, 20 and 40 states; the hybrid-table kernel
    pinned at 20) and within `tol` relative of the CPU oracle, then the error cases.  Called from a process that
    imported torch before the library."""
    from imcoalhmm_amd import synth
    from imcoalhmm_amd.hmm import forward_chunks_batch
    L = _capi.lib()
    dev = torch.device("cuda")

    def logliks(fw, n, nsym, seed):
        pi, T, E = synth.random_hmm(n, nsym, seed=seed, stay=0.97)
        return (pi, T, E), forward_chunks_batch([f.handle for f in fw], pi[None], T[None], E[None], per_chunk=True)[0]

    def rel(a, b):
        return abs(a - b) / abs(b)

    _, alpha3 = train3()
    obs3 = compressible(70_001, seed=21)
    # ---- uint8 and int32, 3 symbols ----
    host = Forwarder.from_array(obs3, 3)
    t8 = torch.from_numpy(obs3).to(dev)
    f8 = Forwarder.from_device(t8, 3)
    t8.zero_()                                                           # the forwarder keeps its own copy
    torch.cuda.synchronize()
    del t8
    assert f8.compressed_length(16384)[1] == alpha3
    assert_same_chunk(host, f8, "uint8 tensor")
    t32 = torch.from_numpy(obs3.astype(np.int32)).to(dev)
    f32 = Forwarder.from_device(t32, 3, stream=torch.cuda.current_stream())
    assert_same_chunk(host, f32, "int32 tensor")
    for n in (10, 20, 40):
        (pi, T, E), got = logliks([host, f8, f32], n, 3, seed=300 + n)
        assert got[0] == got[1] == got[2], (n, got)
        assert rel(got[1], oracle.forward_scaled(pi, T, E, obs3)) < tol, (n, got)
    try:
        _capi.check(L.imc_set_table_streaming(0))
        _capi.check(L.imc_set_blocked_kernel(5))
        (pi, T, E), got = logliks([host, f8], 20, 3, seed=77)
        kernels = _capi.last_plan()["kernels"]
    finally:
        _capi.check(L.imc_set_table_streaming(-1))
        _capi.check(L.imc_set_blocked_kernel(4))
    assert got[0] == got[1], (got, kernels)
    assert rel(got[1], oracle.forward_scaled(pi, T, E, obs3)) < tol
    # ---- errors ----
    bad = obs3.copy()
    bad[5000] = 3
    _raises_value_error(lambda: Forwarder.from_device(torch.from_numpy(bad).to(dev), 3), "column 5000")

    class HostArray(object):                                             # a host address behind the device interface
        def __init__(self, a):
            self.a = a
            self.__cuda_array_interface__ = {"shape": a.shape, "typestr": "|u1", "strides": None, "data": (a.ctypes.data, False), "version": 2}
    h = ctypes.c_void_p()
    assert L.imc_obs_create_device(obs3.ctypes.data, obs3.size, 3, 1, None, ctypes.byref(h)) == _capi.IMC_ERR_ARG
    assert b"device memory" in L.imc_last_error()
    _raises_value_error(lambda: Forwarder.from_device(HostArray(obs3), 3), "device memory")
    short = Forwarder.from_device(torch.from_numpy(obs3[:100].copy()).to(dev), 3)
    assert short.compressed_length(16384) == (100, 3)                    # too short to compress: stays raw
    assert (tokens(short, 16384)[0] == obs3[:100]).all()
    (pi, T, E), got = logliks([short], 10, 3, seed=5)
    assert rel(got[0], oracle.forward_scaled(pi, T, E, obs3[:100])) < tol
    # ---- int16, 257 symbols ----
    obs257 = skewed_symbols(60_000, 257, seed=33)
    host257 = Forwarder.from_array(obs257, 257)                          # trains the 257-symbol dictionary (host path)
    assert host257.compressed_length(16384)[1] > 257
    f16 = Forwarder.from_device(torch.from_numpy(obs257.astype(np.int16)).to(dev), 257)
    assert_same_chunk(host257, f16, "int16 tensor")
    (pi, T, E), got = logliks([host257, f16], 10, 257, seed=9)
    assert got[0] == got[1]
    assert rel(got[1], oracle.forward_scaled(pi, T, E, obs257)) < tol
    # the creation that trains the dictionary, from device memory: only the training head travels to the host
    _capi.check(L.imc_dictionary_reset())
    first = Forwarder.from_device(torch.from_numpy(obs257.astype(np.int16)).to(dev), 257)
    assert first.sym2pair == host257.sym2pair
    assert_same_chunk(host257, first, "int16 tensor, trains the dictionary")
