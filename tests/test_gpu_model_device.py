"""(pi, T) of migration-model populations on the GPU (csrc/kernels_model.hpp behind imc_model_transitions_device and
imc_model_expm_batch_device) against the host function imc_model_transitions / imc_model_expm - the CPU reference,
which takes any space size - and against the reference-derived goldens.

Tolerances are the project's existing ones and none is new: 1e-13 absolute on pi and T between two paths
(test_native_and_numpy_paths_agree), check_hmm's 1e-12 absolute / 1e-11 relative against the goldens, 5e-13 and row sums
within 1e-12 for expm (test_native_expm_matches_scipy), 1e-11 relative on log-likelihoods (the parity suite).  The host
path sits 9e-16 / 9e-15 from numpy and 9e-16 absolute / 6e-15 relative from the goldens, so a changed summation order
(fp64 MFMA products, FMA contraction) has three orders of margin."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from imcoalhmm_amd import Forwarder, Likelihood, _capi, synth
from imcoalhmm_amd import models as M
from model_device_cases import _dp, _i32, call_transitions, one_space_case

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = np.load(os.path.join(HERE, "golden", "model_golden.npz"))
PARAMS = np.load(os.path.join(HERE, "golden", "hmm_params.npz"))
ISO_THETA = np.array([0.001, 1000.0, 0.4])

MODELS = {
    "iso2": (lambda: M.IsolationModel(2), lambda: ISO_THETA),
    "iso7": (lambda: M.IsolationModel(7), lambda: ISO_THETA),
    "im_2_2": (lambda: M.IsolationMigrationModel(2, 2), lambda: GOLD["im_2_2_theta"]),
    "im_3_4": (lambda: M.IsolationMigrationModel(3, 4), lambda: GOLD["im_3_4_theta"]),
    "epochs_2_3_2": (lambda: M.IsolationMigrationEpochsModel(2, 3, 2), lambda: GOLD["epochs_2_3_2_theta"]),
    "vmig_12": (lambda: M.VariableCoalAndMigrationRateModel(1, [2, 3]), lambda: GOLD["vmig_12_theta"]),
}
_cases = {}


def model_case(name, batch=9):
    """The arrays of the transitions entry points for ``batch`` perturbed points of a model (models._native_structure /
    _native_pack, what the Python route passes), built once per model."""
    key = (name, batch)
    if key not in _cases:
        make, theta = MODELS[name]
        model, theta = make(), np.asarray(theta(), dtype=np.float64)
        systems = [model.build_ctmc_system(*(theta * (1.0 + 0.03 * k))) for k in range(batch)]
        st, q_index = M._native_structure(systems[0], M.DEVICE_MAX_SPACE)
        assert st
        q_size, Qs, dts, starts = M._native_pack(systems, st, q_index)
        _cases[key] = dict(n_systems=batch, n_intervals=st["n"], space_size=st["space_size"], cls_off=st["cls_off"], cls_idx=st["cls_idx"],
                           piece_q=st["piece_q"], piece_proj=st["piece_proj"], n_q=st["n_q"], q_size=q_size, n_proj=len(st["proj_off"]),
                           proj_off=st["proj_off"] if len(st["proj_off"]) else _i32([0]), proj=st["proj"] if len(st["proj"]) else np.zeros(1),
                           Q=Qs, dt=dts, start=starts)
    return _cases[key]


def take(case, idx):
    """The systems ``idx`` of a case as a case of their own."""
    out = dict(case, n_systems=len(idx))
    for k in ("Q", "dt", "start"):
        out[k] = np.ascontiguousarray(case[k][idx])
    return out


def both(case):
    lib = _capi.lib()
    rc_h, pi_h, T_h = call_transitions(lib, case, device=False)
    assert rc_h == 0, lib.imc_last_error()
    rc_d, pi_d, T_d = call_transitions(lib, case, device=True)
    assert rc_d == 0, lib.imc_last_error()
    return pi_h, T_h, pi_d, T_d


@pytest.mark.parametrize("name", sorted(MODELS))
def test_transitions_match_the_host_function(name):
    case = model_case(name)
    if name == "im_3_4":
        assert 94 in case["space_size"] and 15 in case["space_size"] and (case["piece_proj"] >= 0).sum() == 1
    if name == "epochs_2_3_2":
        assert case["n_q"] >= 2
    pi_h, T_h, pi_d, T_d = both(case)
    print(name, "max |pi - host|", np.abs(pi_d - pi_h).max(), "max |T - host|", np.abs(T_d - T_h).max())
    assert np.abs(pi_d - pi_h).max() < 1e-13 and np.abs(T_d - T_h).max() < 1e-13


@pytest.mark.parametrize("order,n_intervals", [(128, 5), (97, 4), (33, 1)])
def test_transitions_at_orders_no_model_has(order, n_intervals):
    """Padded orders 128 and 112 (97 states), where the solve leaves LDS; one interval alone is accepted."""
    case = one_space_case(order, n_intervals, n_systems=3, seed=order)
    pi_h, T_h, pi_d, T_d = both(case)
    print(order, "max |pi - host|", np.abs(pi_d - pi_h).max(), "max |T - host|", np.abs(T_d - T_h).max())
    assert np.abs(pi_d - pi_h).max() < 1e-13 and np.abs(T_d - T_h).max() < 1e-13
    assert np.abs(pi_d.sum(axis=1) - 1).max() < 1e-12


class _switched_on(object):
    def __enter__(self):
        self.was = M.set_device_transitions(True)
        self.calls = M._native["device_calls"]
        return self

    def routed(self):
        return M._native["device_calls"] - self.calls

    def __exit__(self, *exc):
        M.set_device_transitions(self.was)


@pytest.mark.parametrize("key,make", [
    ("im_2_2", lambda: M.IsolationMigrationModel(2, 2)), ("im_3_4", lambda: M.IsolationMigrationModel(3, 4)),
    ("im_5_2", lambda: M.IsolationMigrationModel(5, 2)), ("im_4_6_scaled", lambda: M.IsolationMigrationModel(4, 6)),
    ("im20_t0", lambda: M.IsolationMigrationModel(10, 10)), ("epochs_2_3_2", lambda: M.IsolationMigrationEpochsModel(2, 3, 2)),
    ("vmig_11", lambda: M.VariableCoalAndMigrationRateModel(0, [2, 3])), ("vmig_12", lambda: M.VariableCoalAndMigrationRateModel(1, [2, 3])),
    ("vmig_22", lambda: M.VariableCoalAndMigrationRateModel(2, [2, 3])),
])
def test_models_match_the_goldens_through_the_switch(key, make):
    gold = PARAMS if key == "im20_t0" else GOLD
    with _switched_on() as sw:
        pi, T, E = make().build_hidden_markov_model(gold[key + "_theta"])
        assert sw.routed() >= 1
    want_pi, want_T, want_E = gold[key + "_pi"], gold[key + "_T"], gold[key + "_E"]
    assert pi.shape == want_pi.shape and T.shape == want_T.shape and pi.dtype == np.float64 and T.dtype == np.float64
    nz = want_T > 1e-200
    print(key, "pi", np.abs(pi - want_pi).max(), "T", np.abs(T - want_T).max(), "T rel", np.abs(T[nz] / want_T[nz] - 1).max())
    assert np.abs(pi - want_pi).max() < 1e-12
    assert np.abs(T - want_T).max() < 1e-12
    assert np.abs(T[nz] / want_T[nz] - 1).max() < 1e-11
    assert np.abs(E - want_E).max() < 1e-12
    assert abs(pi.sum() - 1) < 1e-12 and np.abs(T.sum(axis=1) - 1).max() < 1e-12


def test_small_spaces_stay_on_the_host_path_with_the_switch_on():
    with _switched_on() as sw:
        M.IsolationModel(5).build_hidden_markov_model(ISO_THETA)
        assert sw.routed() == 0


@pytest.mark.parametrize("n", [1, 2, 4, 15, 16, 17, 31, 94, 96, 128])
def test_expm_batch_matches_the_host_routine(n):
    lib = _capi.lib()
    rng = np.random.default_rng(5 + n)
    scales = (1e-4, 1e-2, 0.2, 0.9, 2.0, 2.2, 4.5, 5.3, 6.0, 40.0, 900.0)      # every Pade degree, s = 0 and s > 0
    A = np.empty((len(scales), n, n))
    for k, scale in enumerate(scales):
        Q = rng.random((n, n)) * scale / n
        np.fill_diagonal(Q, 0.0)
        np.fill_diagonal(Q, -Q.sum(axis=1))
        A[k] = Q
    want = np.empty_like(A)
    for k in range(len(scales)):
        assert lib.imc_model_expm(n, A[k].ctypes.data_as(_dp), want[k].ctypes.data_as(_dp)) == 0
    got = np.full_like(A, np.nan)
    assert lib.imc_model_expm_batch_device(n, len(scales), A.ctypes.data_as(_dp), got.ctypes.data_as(_dp)) == 0, lib.imc_last_error()
    print(n, "max |device - host| per scale", np.abs(got - want).max(axis=(1, 2)))
    assert np.abs(got - want).max() < 5e-13
    assert np.abs(got.sum(axis=2) - 1).max() < 1e-12
    again = np.full_like(A, np.nan)
    assert lib.imc_model_expm_batch_device(n, len(scales), A.ctypes.data_as(_dp), again.ctypes.data_as(_dp)) == 0
    assert again.tobytes() == got.tobytes()


def test_results_do_not_depend_on_the_call():
    lib = _capi.lib()
    case = model_case("im_3_4")
    _, pi9, T9 = call_transitions(lib, case, device=True)
    _, pi9b, T9b = call_transitions(lib, case, device=True)
    assert pi9.tobytes() == pi9b.tobytes() and T9.tobytes() == T9b.tobytes()
    rc, pi1, T1 = call_transitions(lib, take(case, [0]), device=True)
    assert rc == 0 and pi1[0].tobytes() == pi9[0].tobytes() and T1[0].tobytes() == T9[0].tobytes()
    # 257 systems: more work matrices than one launch's workspace takes, so the last system runs in a later round
    many = take(case, [1 + k % 8 for k in range(256)] + [0])
    # (precondition: nine padded work matrices per distinct (rate matrix, dt) of every system, against the 256 MiB a launch
    #  may take - MODEL_WORK_CAP in csrc/engine_model.hpp - so that systems are read and written at a non-zero round offset)
    padded = [16 * ((int(q) + 15) // 16) for q in case["q_size"]]
    work_bytes = sum(9 * 8 * padded[q] ** 2 for b in range(257)
                     for q, _ in {(int(q), float(d)) for q, d in zip(case["piece_q"], many["dt"][b])})
    assert work_bytes > (256 << 20), work_bytes
    rc, pim, Tm = call_transitions(lib, many, device=True)
    assert rc == 0, lib.imc_last_error()
    assert pim[256].tobytes() == pi9[0].tobytes() and Tm[256].tobytes() == T9[0].tobytes()
    assert pim[3].tobytes() == pi9[4].tobytes() and Tm[3].tobytes() == T9[4].tobytes()


def test_errors():
    lib = _capi.lib()
    rc, _, _ = call_transitions(lib, one_space_case(129, 3), device=True)
    assert rc == _capi.IMC_ERR_ARG
    # a "rate matrix" whose rows do not sum to 0, in system 3 of 5
    case = take(model_case("im_2_2"), [0, 1, 2, 3, 4])
    off = 0
    for order in case["q_size"]:
        block = case["Q"][3, off:off + order * order].reshape(order, order)
        block[np.arange(order), np.arange(order)] *= 0.9
        off += order * order
    rc, _, _ = call_transitions(lib, case, device=True)
    msg = lib.imc_last_error().decode()
    assert rc == _capi.IMC_ERR_ARG and "joint probabilities sum to" in msg and "not 1" in msg and "system 3" in msg, (rc, msg)
    rc_h, _, _ = call_transitions(lib, case, device=False)
    assert rc_h == _capi.IMC_ERR_ARG and lib.imc_last_error().decode().split(",")[0] == msg.split(",")[0]      # the same sum, to 6 decimals
    # start mass outside the B class: the host route's ValueError through Python
    sp = M.migration_space()
    Q = sp.rate_matrix(M.migration_rates(1000.0, 1000.0, 0.4, 200.0, 200.0))
    bad = np.zeros(sp.size)
    bad[sp.end_states[0]] = 1.0
    system = M.PiecewiseCTMC(bad, [sp] * 3, [(Q, 1e-3, None), (Q, 2e-3, None)])
    with _switched_on() as sw:
        with pytest.raises(ValueError, match="must be supported on the B class"):
            M.hmm_transitions(system)
        assert sw.routed() == 1


def test_likelihood_batch_is_the_same_through_the_switch():
    model = M.IsolationMigrationModel(3, 3)
    theta = np.array([0.001, 0.001, 1000.0, 0.4, 200.0])
    thetas = [theta * (1.0 + 0.02 * k) for k in range(8)]
    pi, T, E = model.build_hidden_markov_model(theta)
    chunks = [Forwarder.from_array(synth.sample_alignment(pi, T, E, 20_000, seed=11 + k), 3) for k in range(2)]
    lik = Likelihood(model, chunks)
    off = lik.batch(thetas)
    with _switched_on() as sw:
        on = lik.batch(thetas)
        assert sw.routed() == 1
    print("log-likelihoods off", off, "relative difference", np.abs(on / off - 1))
    assert np.all(np.isfinite(off)) and np.abs(on / off - 1).max() <= 1e-11


GUARD_SCRIPT = textwrap.dedent('''
    import sys
    import numpy as np
    sys.path.insert(0, %r)
    sys.path.insert(0, %r)
    import test_gpu_model_device as t
    from imcoalhmm_amd import _capi
    lib = _capi.lib()
    pi_h, T_h, pi_d, T_d = t.both(t.model_case("im_3_4"))
    assert np.abs(pi_d - pi_h).max() < 1e-13 and np.abs(T_d - T_h).max() < 1e-13
    print("transitions ok", flush=True)
    t.test_expm_batch_matches_the_host_routine(17)
    t.test_expm_batch_matches_the_host_routine(94)
    print("expm ok", flush=True)
''') % (REPO, HERE)


def test_under_guard_pages(tmp_path):
    """IM(3,4) transitions and expm at n = 17 and 94 with every device buffer flush against an unmapped range."""
    script = tmp_path / "model_guard.py"
    script.write_text(GUARD_SCRIPT)
    env = dict(os.environ, IMC_GUARD="1")
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    tail = (out.stdout[-1500:], out.stderr[-3000:])
    if "hipMemAddressReserve" in out.stderr or "hipMemCreate" in out.stderr or "hipMemGetAllocationGranularity" in out.stderr:
        pytest.skip("HIP virtual-memory management is unavailable on this box: %r" % (tail,))
    assert out.returncode == 0 and "transitions ok" in out.stdout and "expm ok" in out.stdout, tail
