"""Shared by tests/test_model_device_cpu.py and tests/test_gpu_model_device.py: a synthetic model structure of any order
and one way of calling imc_model_transitions / imc_model_transitions_device on the same arrays."""
import ctypes

import numpy as np

_i32p = ctypes.POINTER(ctypes.c_int32)
_dp = ctypes.POINTER(ctypes.c_double)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def one_space_case(order, n_intervals, n_systems=1, seed=0):
    """A synthetic structure over ONE state space of ``order`` states, numbered class by class B, L, R, E as
    models.StateSpace does, with one random rate matrix per system and no projection.  Mass only moves forward
    (B -> L | R -> E) and the R class mirrors the L class rate for rate, which is what makes the symmetrised joint
    matrix sum to 1.  Returns the keyword arrays of the two transitions entry points."""
    rng = np.random.default_rng(seed)
    nl = max(order // 4, 1)
    ne = max(order // 4, 1)
    nb = max(order - 2 * nl - ne, 1)
    Bc, Lc, Rc, Ec = (np.arange(a, min(b, order)) for a, b in ((0, nb), (nb, nb + nl), (nb + nl, nb + 2 * nl), (nb + 2 * nl, order)))
    classes = [Bc, Lc, Ec]
    cls_idx = np.concatenate(classes * n_intervals)
    cls_off = np.concatenate([[0], np.cumsum([len(c) for c in classes] * n_intervals)])
    Q = np.zeros((n_systems, order, order))
    if len(Rc) == nl and len(Ec):
        for b in range(n_systems):
            q = Q[b]
            q[np.ix_(Bc, Bc)] = np.triu(rng.random((nb, nb)), 1)
            q[np.ix_(Bc, Lc)] = q[np.ix_(Bc, Rc)] = rng.random((nb, nl))
            q[np.ix_(Bc, Ec)] = rng.random((nb, len(Ec)))
            q[np.ix_(Lc, Lc)] = q[np.ix_(Rc, Rc)] = np.triu(rng.random((nl, nl)), 1)
            q[np.ix_(Lc, Ec)] = q[np.ix_(Rc, Ec)] = rng.random((nl, len(Ec)))
            q[np.ix_(Ec, Ec)] = np.triu(rng.random((len(Ec), len(Ec))), 1)
            q *= (1.0 + 0.1 * b) * 8.0 / order
            np.fill_diagonal(q, -q.sum(axis=1))
    start = np.zeros((n_systems, order))
    start[:, 0] = 1.0
    return dict(n_systems=n_systems, n_intervals=n_intervals, space_size=_i32([order] * n_intervals), cls_off=_i32(cls_off),
                cls_idx=_i32(cls_idx), piece_q=_i32([0] * max(n_intervals - 1, 1)), piece_proj=_i32([-1] * max(n_intervals - 1, 1)),
                n_q=1, q_size=_i32([order]), n_proj=0, proj_off=_i32([0]), proj=np.zeros(1), Q=Q,
                dt=0.3 + 0.1 * rng.random((n_systems, max(n_intervals - 1, 1))), start=start)


def call_transitions(lib, case, device, null=None):
    """(rc, pi, T) of imc_model_transitions(_device) on the arrays of ``case``; ``null`` names one pointer passed as NULL."""
    n, nb = case["n_intervals"], case["n_systems"]
    pi, T = np.full((nb, n), np.nan), np.full((nb, n, n), np.nan)

    def ptr(name, kind):
        return None if name == null else case[name].ctypes.data_as(kind)
    args = [nb, n, ptr("space_size", _i32p), ptr("cls_off", _i32p), ptr("cls_idx", _i32p), ptr("piece_q", _i32p),
            ptr("piece_proj", _i32p), case["n_q"], ptr("q_size", _i32p), case["n_proj"], ptr("proj_off", _i32p), ptr("proj", _dp),
            ptr("Q", _dp), ptr("dt", _dp), ptr("start", _dp), None if null == "pi" else pi.ctypes.data_as(_dp), T.ctypes.data_as(_dp)]
    rc = lib.imc_model_transitions_device(*args) if device else lib.imc_model_transitions(*(args + [1]))
    return rc, pi, T
