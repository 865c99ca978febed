"""The Huang-Carter kernel table w(eta): the initial-value problem of the reference's ``generate_kernel``
(functionals.py:1204-1230, :1303-1329), solved here in plain numpy.

    w'(eta) = -[(5/3) (L(eta) - 3 eta^2 - 1) - (5 - 3 beta) beta w] / (beta eta),   L = 1 / G^-1_Lindhard,
    w(eta_max) = -(8/3) / ((5 - 3 beta) beta),

integrated downwards with the classical fourth-order Runge-Kutta scheme on the table's own nodes; w(0) = 0 is prepended as in
the reference.  The reference hands the same problem to xitorch's ``solve_ivp``; this table is the project's own RK4 solution
of it, not xitorch's -- the two agree to the truncation error of either integrator, not to rounding.
"""
import functools
import math

import numpy as np


def _lindhard(eta):
    """1 / G^-1(eta) with the two special cases of the reference (functionals.py:1214-1220)"""
    if eta == 0.0:
        return 1.0
    if eta == 1.0:
        return 2.0
    return 1.0 / (0.5 + ((1.0 - eta * eta) / (4.0 * eta)) * math.log(abs((1.0 + eta) / (1.0 - eta))))


@functools.lru_cache(maxsize=16)
def _solve(beta, eta_max, n_eta):
    eta = np.linspace(0.0, eta_max, n_eta)
    bb = (5.0 - 3.0 * beta) * beta

    def f(e, w):
        return -((5.0 / 3.0) * (_lindhard(e) - 3.0 * e * e - 1.0) - bb * w) / beta / e

    ts = [float(t) for t in eta[:0:-1]]            # eta_max down to eta[1]
    y = -(8.0 / 3.0) / bb
    out = [y]
    for i in range(len(ts) - 1):
        t0, t1 = ts[i], ts[i + 1]
        h = t1 - t0
        tm = t0 + h / 2
        k1 = f(t0, y)
        k2 = f(tm, y + h / 2 * k1)
        k3 = f(tm, y + h / 2 * k2)
        k4 = f(t1, y + h * k3)
        y = y + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
        out.append(y)
    w = np.concatenate(([0.0], np.array(out[::-1], dtype=np.float64)))
    eta.setflags(write=False)
    w.setflags(write=False)
    return eta, w


def solve_kernel(beta, eta_max=50.0, n_eta=10000):
    """-> (eta, w): two read-only float64 arrays of ``n_eta`` entries, cached per argument tuple."""
    beta, eta_max, n_eta = float(beta), float(eta_max), int(n_eta)
    if not 0.0 < beta < 5.0 / 3.0:
        raise ValueError('solve_kernel: beta must lie in (0, 5/3), got %r' % (beta,))
    if n_eta < 4 or not eta_max > 0.0:
        raise ValueError('solve_kernel: needs n_eta >= 4 and eta_max > 0')
    return _solve(beta, eta_max, n_eta)
