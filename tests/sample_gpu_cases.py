"""The device cases of tests/test_gpu_sample.py, run by the scripts it starts in child processes that import torch before the
library (one HIP runtime per process): imc_sample_device against imc_sample_host, exactly."""
import os

import numpy as np

from imcoalhmm_amd import Forwarder, _capi, models, simulate
from sample_cases import device_sample, hmm, host_sample, last_sampling, reference_sample

STATES = (1, 2, 3, 20, 63, 64, 65, 128, 150, 256)
L_ODD = 3 * 64 + 5
DEFAULT_TILE = 512

# (kind, N, S, emit, replicates, L, states output)
EQUALITY = [("cyclic", n, 3, 2, 3, L_ODD, True) for n in STATES] + [
    ("sticky", 20, 3, 2, 1, 20011, True),
    ("fast-mixing", 20, 3, 3, 3, 20011, False),
    ("fast-mixing", 20, 257, 257, 1, 20011, True),                  # 16-bit output
    ("fast-mixing", 20, 257, 257, 3, 65, False),
    ("fast-mixing", 2, 65, 65, 3, L_ODD, True),
    ("sparse", 63, 3, 2, 3, 20011, True),
    ("fast-mixing", 64, 3, 3, 1, 20011, False),
    ("sparse", 65, 3, 2, 3, 64, True),
    ("sticky", 128, 3, 3, 1, 63, True),
    ("absorbing", 150, 3, 2, 1, 20011, True),
    ("fast-mixing", 256, 65, 65, 3, 65, True),
    ("absorbing", 20, 3, 2, 3, L_ODD, False),
    ("fast-mixing", 3, 3, 2, 1, 1, True),
    ("fast-mixing", 3, 3, 2, 3, 1, True),
    ("sticky", 3, 3, 3, 3, 2, True),
    ("fast-mixing", 1, 3, 2, 1, 64, True),
    ("banded", 150, 3, 3, 3, L_ODD, True),
    ("unnormalised", 256, 3, 2, 1, 20011, True),
]


def assert_equal(got, want, what):
    if want is None:
        assert got is None, what
        return
    diff = np.flatnonzero((got != want).ravel())
    assert got.shape == want.shape and diff.size == 0, (what, diff.size, int(diff[0]), got.ravel()[diff[:6]], want.ravel()[diff[:6]])


def equality_case(torch, case, seed=20240917):
    kind, n, S, emit, R, L, states = case
    pi, T, E = hmm(kind, n, S, seed=5)
    want_sym, want_st = host_sample(pi, T, E, emit, seed, 0, R, L, states=states)
    sym, st = device_sample(torch, pi, T, E, emit, seed, 0, R, L, states=states)     # (last: imc_last_sampling describes it)
    assert_equal(sym, want_sym, (case, "symbols"))
    assert_equal(st, want_st, (case, "states"))


def equality(torch):
    for case in EQUALITY:
        equality_case(torch, case)
        tile = int(os.environ["IMC_SAMPLE_TILE"])
        R, L = case[4], case[5]
        assert last_sampling() == [1, (R * L + tile - 1) // tile, tile, R * L], (case, last_sampling())


def tile_lengths(torch):
    """No result depends on the tile length; L lies above the default tile, and at tile 1 the scan takes two passes."""
    R, L = 1, 70001
    for kind, n in (("sticky", 20), ("cyclic", 20), ("fast-mixing", 150)):
        pi, T, E = hmm(kind, n, 3, seed=8)
        want = host_sample(pi, T, E, 2, 99, 0, R, L)
        for tile in (1, 7, 64, 4096, None):
            if tile is None:
                os.environ.pop("IMC_SAMPLE_TILE", None)
            else:
                os.environ["IMC_SAMPLE_TILE"] = str(tile)
            got = device_sample(torch, pi, T, E, 2, 99, 0, R, L)
            assert_equal(got[0], want[0], (kind, n, tile, "symbols"))
            assert_equal(got[1], want[1], (kind, n, tile, "states"))
            used = tile or DEFAULT_TILE
            assert last_sampling() == [1, (L + used - 1) // used, used, L], (tile, last_sampling())
    os.environ.pop("IMC_SAMPLE_TILE", None)


def determinism(torch):
    pi, T, E = hmm("fast-mixing", 20, 3, seed=2)
    R, L, seed = 3, 5003, 77
    a = device_sample(torch, pi, T, E, 2, seed, 0, R, L)
    b = device_sample(torch, pi, T, E, 2, seed, 0, R, L)
    assert_equal(a[0], b[0], "repeated call, symbols")
    assert_equal(a[1], b[1], "repeated call, states")
    other_tag = device_sample(torch, pi, T, E, 2, seed, 1, R, L)
    other_seed = device_sample(torch, pi, T, E, 2, seed + (1 << 32), 0, R, L)
    assert (a[1] != other_tag[1]).mean() > 0.5 and (a[1] != other_seed[1]).mean() > 0.5    # 20 fast-mixing states: ~95 % differ
    assert (a[1][0] != a[1][1]).mean() > 0.5 and (a[1][1] != a[1][2]).mean() > 0.5
    alone = host_sample(pi, T, E, 2, seed, 0, 1, L)
    assert_equal(a[0][:1], alone[0], "replicate 0 alone")
    for r in range(R):                                       # the specification for that replicate alone (numpy)
        want_sym, want_st = reference_sample(pi, T, E, 2, seed, 0, 1, L, first_replicate=r)
        assert_equal(a[0][r:r + 1].astype(np.int64), want_sym, ("replicate alone, symbols", r))
        assert_equal(a[1][r:r + 1].astype(np.int64), want_st, ("replicate alone, states", r))


def stream_ordering(torch):
    pi, T, E = hmm("sticky", 20, 3, seed=4)
    R, L = 2, 300007
    want = host_sample(pi, T, E, 2, 5, 0, R, L, states=False)[0]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        big = torch.zeros(1 << 28, dtype=torch.uint8, device="cuda")     # the side stream is busy ...
        sym = torch.full((R, L), 0x6E, dtype=torch.uint8, device="cuda")  # ... when the output is written on it
        keep = (_capi.as_f64(pi), _capi.as_f64(T), _capi.as_f64(E))
        _capi.check(_capi.lib().imc_sample_device(20, 3, 2, _capi.dptr(keep[0]), _capi.dptr(keep[1]), _capi.dptr(keep[2]), 5, 0, R, L,
                                                  sym.data_ptr(), 1, None, side.cuda_stream))
        got = sym.cpu().numpy()
    assert_equal(got, want, "output written on a side stream")
    del big
    via_module = simulate.sample(pi, T, E, L, 5, replicates=R, emit_symbols=2, stream=side)
    assert via_module.shape == (R, L) and via_module.dtype == torch.uint8 and via_module.is_cuda
    assert_equal(via_module.cpu().numpy(), want, "simulate.sample on a side stream")
    sym_h, st_h = simulate.sample(pi, T, E, L, 5, replicates=R, emit_symbols=2, where="host", return_states=True)
    sym_d, st_d = simulate.sample(pi, T, E, L, 5, replicates=R, emit_symbols=2, return_states=True)
    assert_equal(sym_d.cpu().numpy(), sym_h, "simulate.sample host and device")
    assert_equal(st_d.cpu().numpy(), st_h, "simulate.sample host and device, states")
    wide = simulate.sample(*hmm("fast-mixing", 5, 300, seed=1), 1000, 3)
    assert wide.dtype == torch.int16 and int(wide.max()) > 256
    # a host pointer as output: an error, never a fault
    lib = _capi.lib()
    host = np.zeros(R * L, dtype=np.uint8)
    dev = torch.zeros(R * L, dtype=torch.uint8, device="cuda")
    head = (20, 3, 2, _capi.dptr(keep[0]), _capi.dptr(keep[1]), _capi.dptr(keep[2]), 5, 0, R, L)
    assert lib.imc_sample_device(*head, host.ctypes.data, 1, None, None) == _capi.IMC_ERR_ARG
    assert b"d_sym_out is not device memory" in lib.imc_last_error()
    assert lib.imc_sample_device(*head, dev.data_ptr(), 1, host.ctypes.data, None) == _capi.IMC_ERR_ARG
    assert b"d_states_out is not device memory" in lib.imc_last_error()
    assert not host.any() and not dev.any()


def forwarders(torch):
    from device_encode_cases import assert_same_chunk
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hmm_params.npz"))
    pi, T, E = d["iso20_t0_pi"], d["iso20_t0_T"], d["iso20_t0_E"]
    R, L, seed = 2, 70001, 31
    fw = simulate.forwarders(pi, T, E, L, seed, replicates=R, emit_symbols=2)
    want = host_sample(pi, T, E, 2, seed, 0, R, L, states=False)[0]
    assert want.max() == 1 and len(fw) == R
    for r in range(R):
        ref = Forwarder.from_array(want[r], 3)
        assert fw[r].NSYM == 3 and len(fw[r]) == L
        assert_same_chunk(ref, fw[r], ("simulated replicate", r))
        assert fw[r].forward(pi, T, E) == ref.forward(pi, T, E), r
        assert np.isfinite(fw[r].forward(pi, T, E))


def model_simulate(torch):
    from device_encode_cases import assert_same_chunk
    model, theta = models.IsolationModel(10), np.array([0.001, 1000.0, 0.4])
    R, L, seed = 2, 50001, 9
    pi, T, E = model.build_hidden_markov_model(theta)
    sym = host_sample(pi, T, E, 2, seed, 0, R, L, states=False)[0]
    mask = host_sample(*simulate.missing_chain(0.04, 25), 2, seed, simulate.MISSING_TAG, R, L, states=False)[0]
    assert 0.02 < mask.mean() < 0.06 and set(np.unique(mask)) == {0, 1}
    want = np.where(mask != 0, 2, sym).astype(np.uint8)
    got = simulate.sample_with_missing(pi, T, E, L, seed, replicates=R, emit_symbols=2, missing=(2, 0.04, 25)).cpu().numpy()
    assert set(np.unique(got)) == {0, 1, 2}
    assert_equal(got == 2, mask != 0, "missing positions")
    assert_equal(got, want, "symbols under the overlay")
    fw = model.simulate(theta, L, seed, replicates=R, missing=(2, 0.04, 25))
    for r in range(R):
        assert_same_chunk(Forwarder.from_array(want[r], 3), fw[r], ("Model.simulate", r))
    plain = model.simulate(theta, L, seed, replicates=1)
    assert_same_chunk(Forwarder.from_array(sym[0], 3), plain[0], "Model.simulate without missing data")


def guard(torch):
    for case in EQUALITY:
        if case[1] in (20, 150, 256) or case[5] == 1:
            equality_case(torch, case)
