"""imc_sample_host (include/imcoal_sample.h) without a device: exact agreement with an independent numpy implementation of
the specification (sample_cases.reference_sample: uint64 Philox, np.cumsum tables), every refusal of both entry points
with its code and message before any HIP call, and a statistical check of the drawn chain."""
import ctypes

import numpy as np
import pytest

from imcoalhmm_amd import _capi, build
from sample_cases import KINDS, hmm, host_sample, last_sampling, philox4x32_10, reference_sample


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _capi.lib()


def test_philox_known_answers():
    for ctr, key, want in (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
                            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        assert tuple(int(w) for w in philox4x32_10(*ctr, *key)) == want


@pytest.mark.parametrize("n", (1, 2, 3, 20, 65, 256))
def test_host_equals_independent_numpy(lib, n):
    for k, kind in enumerate(KINDS):
        for R, L, S, emit, tag in ((1, 2500 if n < 65 else 1201, 3, 2, 0), (3, 701, 5, 5, 1)):
            pi, T, E = hmm(kind, n, S, seed=11 + k)
            seed = 20240917 + (k << 40)                                   # both key words in use
            sym, st = host_sample(pi, T, E, emit, seed, tag, R, L)
            want_sym, want_st = reference_sample(pi, T, E, emit, seed, tag, R, L)
            assert (st == want_st).all(), (kind, n, R, int(np.flatnonzero((st != want_st).ravel())[0]))
            assert (sym == want_sym).all(), (kind, n, R, int(np.flatnonzero((sym != want_sym).ravel())[0]))
            assert last_sampling() == [0, 0, 0, R * L]
            only_sym, none = host_sample(pi, T, E, emit, seed, tag, R, L, states=False)
            assert none is None and (only_sym == sym).all()
    if n == 20:                                                            # 16-bit symbols, L = 5000
        pi, T, E = hmm("fast-mixing", n, 300, seed=3)
        sym, st = host_sample(pi, T, E, 300, 5, 2, 1, 5000)
        want_sym, want_st = reference_sample(pi, T, E, 300, 5, 2, 1, 5000)
        assert sym.dtype == np.uint16 and sym.max() > 256 and (sym == want_sym).all() and (st == want_st).all()


def _call(lib, which, N=4, S=3, emit=3, pi="ok", T="ok", E="ok", R=1, L=10, out="ok", sym_bytes=1, edit=None):
    rng = np.random.default_rng(0)
    arrays = {"pi": rng.random(max(N, 1)) + 0.1, "T": rng.random((max(N, 1), max(N, 1))) + 0.1, "E": rng.random((max(N, 1), max(S, 1))) + 0.1}
    if edit:
        edit(arrays)
    ptr = lambda name, flag: _capi.dptr(arrays[name]) if flag == "ok" else None
    buf = np.zeros(64, dtype=np.uint8)                                    # (never written: every call here is refused first)
    args = [N, S, emit, ptr("pi", pi), ptr("T", T), ptr("E", E), 1, 0, R, L, buf.ctypes.data if out == "ok" else None, sym_bytes, None]
    if which == "imc_sample_device":
        args.append(None)
    rc = getattr(lib, which)(*args)
    return rc, lib.imc_last_error().decode()


REFUSALS = [
    (dict(N=0), "N must be in [1,256]"), (dict(N=257), "N must be in [1,256]"),
    (dict(S=0, emit=0), "S must be in [1,4096]"), (dict(S=4097), "S must be in [1,4096]"),
    (dict(emit=0), "emit_symbols must be in [1,S]"), (dict(emit=4), "emit_symbols must be in [1,S]"),
    (dict(S=257, emit=257, sym_bytes=1), "byte symbols cannot carry more than 256 symbols"),
    (dict(sym_bytes=3), "sym_bytes must be 1 or 2"), (dict(sym_bytes=0), "sym_bytes must be 1 or 2"),
    (dict(L=0), "L must be in [1,2^31)"), (dict(L=1 << 31), "L must be in [1,2^31)"),
    (dict(R=0), "n_replicates must be in [1,65536]"), (dict(R=65537), "n_replicates must be in [1,65536]"),
    (dict(pi=None), "pi, T or E is null"), (dict(T=None), "pi, T or E is null"), (dict(E=None), "pi, T or E is null"),
    (dict(out=None), "the symbol output is null"),
    (dict(edit=lambda a: a["T"].__setitem__((2, 1), -0.25)), "T row 2: an entry is negative or not finite"),
    (dict(edit=lambda a: a["T"].__setitem__((3, 0), np.inf)), "T row 3: an entry is negative or not finite"),
    (dict(edit=lambda a: a["E"].__setitem__((1, 2), np.nan)), "E row 1: an entry is negative or not finite"),
    (dict(edit=lambda a: a["pi"].__setitem__(slice(None), 0.0)), "pi row 0: the total is not positive"),
    (dict(emit=2, edit=lambda a: a["E"].__setitem__((3, slice(0, 2)), 0.0)), "E row 3: the total is not positive"),
]


@pytest.mark.parametrize("which", ("imc_sample_host", "imc_sample_device"))
def test_refusals_name_their_reason_and_touch_no_device(lib, which):
    """IMC_ERR_ARG with its message from both entry points.  The device entry point decides all of them before its first
    HIP call: on a machine without a device it would answer IMC_ERR_NODEVICE otherwise (last test of this file)."""
    for kwargs, message in REFUSALS:
        rc, err = _call(lib, which, **kwargs)
        assert rc == _capi.IMC_ERR_ARG and err == which + ": " + message, (kwargs, rc, err)
    with pytest.raises(ValueError, match="T row 2"):
        _capi.check(_call(lib, which, edit=lambda a: a["T"].__setitem__((2, 1), -0.25))[0])
    assert lib.imc_last_sampling(None) == _capi.IMC_ERR_ARG


def test_tile_setting_is_refused_before_any_device_call(lib, monkeypatch):
    for bad in ("0", "65537", "abc", "-1", "12x"):
        monkeypatch.setenv("IMC_SAMPLE_TILE", bad)
        rc, err = _call(lib, "imc_sample_device")
        assert rc == _capi.IMC_ERR_ARG and "IMC_SAMPLE_TILE" in err, (bad, rc, err)
    monkeypatch.setenv("IMC_SAMPLE_TILE", "1")
    rc, err = _call(lib, "imc_sample_device", R=65536, L=(1 << 31) - 1)
    assert rc == _capi.IMC_ERR_ARG and "2^31 tiles" in err, (rc, err)


def test_statistics_of_the_drawn_chain(lib):
    """Every empirical transition and emission frequency within 5 binomial standard deviations of its probability (the
    worst deviation on exactly these inputs is 1.8, printed below): deterministic, a condition with margin."""
    rng = np.random.default_rng(1)
    Rm = rng.random((4, 4)) + 1e-3
    E = rng.random((4, 3)) + 0.05
    T = 0.05 * Rm + 0.95 * np.eye(4)
    T /= T.sum(axis=1, keepdims=True)
    pi = np.full(4, 0.25)
    sym, st = host_sample(pi, T, E, 3, 20240917, 0, 1, 200000)
    x, o = st[0].astype(np.int64), sym[0].astype(np.int64)
    worst = 0.0
    pairs = np.bincount(x[:-1] * 4 + x[1:], minlength=16).reshape(4, 4)
    emis = np.bincount(x * 3 + o, minlength=12).reshape(4, 3)
    for counts, probs in ((pairs, T), (emis, E / E.sum(axis=1, keepdims=True))):
        n = counts.sum(axis=1, keepdims=True)
        assert (n > 1000).all()
        z = np.abs(counts / n - probs) / np.sqrt(probs * (1 - probs) / n)
        worst = max(worst, float(z.max()))
    print("worst deviation: %.2f binomial standard deviations" % worst)
    assert worst < 5.0, worst


def test_device_entry_point_without_a_device(lib):
    if lib.imc_device_count() > 0:
        pytest.skip("a device is present")
    rc, err = _call(lib, "imc_sample_device")
    assert rc == _capi.IMC_ERR_NODEVICE and "no HIP device" in err, (rc, err)
