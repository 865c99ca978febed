"""numpy double of the preconditioned conjugate gradients (ofdft_cg_direction and the preconditioned mode of ofdft_cg_start /
ofdft_cg_step: professad_amd/csrc/cg_abi.h, cg_kernels.h; ofdft_precondition: engine_hvp.inc.h) on top of
tests/tn_double.py, with HipCgBackend's methods, so that optimize.solve_projected, density_response and TruncatedNewton run the
preconditioned recurrence without a device (tests/test_pcg_cpu.py) and the device sweeps and solves have a yardstick
(tests/test_pcg_gpu.py).  Not the product: nothing in professad_amd imports it.

The recurrence, for P H P x = b with P = I - phi phi^T / S and a symmetric positive definite M^-1:
    start       x = 0, r = P b, phi.r = 0
    direction   z = M^-1 r;  rho = r.z - (phi.r)(phi.z) / S;  beta = rho / rho_old (0 the first time);  p = (z - phi (phi.z) / S) + beta p
    step        alpha = rho / p.q;  x += alpha p;  r -= alpha (q - phi (phi.q) / S);  r.r and phi.r;  the stopping rules on r.r
"""
import math

import numpy as np

import hvp_double as D
import tn_double as T
from tn_double import CG_CONVERGED, CG_CURVATURE, CG_MAXITER, CG_RUNNING  # noqa: F401


def kappa2_auto(n_elec, volume):
    """(4/3) k_F^2 of the mean density"""
    return (4.0 / 3.0) * (3.0 * math.pi ** 2 * n_elec / volume) ** (2.0 / 3.0)


def precondition(box, r, kappa2):
    """z = irfftn(rfftn(r) / (k^2 + kappa2)), k of hvp_double.k_squared"""
    return np.fft.irfftn(np.fft.rfftn(r) / (D.k_squared(box, r.shape) + kappa2), s=r.shape, axes=(0, 1, 2))


class _Pcg:
    """the preconditioned recurrence over NumpyCgBackend's state; `apply(r, n_elec) -> z` is the subclass's"""
    preconditioned = True

    def start(self, phi, b, rtol, maxiter):
        super().start(phi, b, rtol, maxiter)
        self.phir, self.rho, self.first, self.ready, self.z = 0.0, 0.0, True, False, None

    def pre_direction(self, phi, n_elec):
        assert self.reason == CG_RUNNING and not self.ready
        self.z = self.apply(self.r, n_elec)
        self.direction_sweeps(phi)
        return self.reason

    def direction_sweeps(self, phi):
        """the two sweeps of ofdft_cg_direction on the z in place"""
        z = self.z
        phiz = float((phi * z).sum())
        rho = float((self.r * z).sum()) - self.phir * phiz / self.S
        if not rho > 0:
            self.reason = CG_CURVATURE
            return
        pz = z - phi * (phiz / self.S)
        self.p = pz if self.first else pz + (rho / self.rho) * self.p
        self.rho, self.first, self.ready = rho, False, True

    def step(self, phi, pq, phiq):
        assert self.reason == CG_RUNNING and self.ready
        if not pq > 0:
            if self.iters == 0:
                self.x = self.p.copy()
            self.reason = CG_CURVATURE
            return self.reason
        alpha = self.rho / pq
        self.x = self.x + alpha * self.p
        self.r = self.r - alpha * (self.q - phi * (phiq / self.S))
        self.iters += 1
        self.rr = float((self.r * self.r).sum())
        self.phir = float((phi * self.r).sum())
        self.ready = False
        if not self.rr > self.rtol ** 2 * self.bb:
            self.reason = CG_CONVERGED
        elif self.iters >= self.maxiter:
            self.reason = CG_MAXITER
        return self.reason


class PcgBackend(_Pcg, T.NumpyCgBackend):
    """NumpyCgBackend preconditioned by the kinetic operator; kappa2 'auto' = (4/3) k_F^2 from the n_elec of the solve"""

    def __init__(self, box, shape, terms, kappa2='auto', alpha=5 / 6, beta=5 / 6):
        T.NumpyCgBackend.__init__(self, box, shape, terms, alpha, beta)
        self.kappa2 = kappa2

    def apply(self, r, n_elec):
        k2 = kappa2_auto(n_elec, abs(np.linalg.det(self.box))) if self.kappa2 == 'auto' else self.kappa2
        return precondition(self.box, r, k2)


def diag_precond(n, seed=0):
    """m of the made-up diagonal preconditioner z = r / m: uniform in [0.5, 1.5], independent of tn_double.diag_inputs"""
    return 0.5 + np.random.default_rng(7000003 * seed + n + 11).random(n)


class DiagPcgBackend(_Pcg, T.DiagCgBackend):
    """the preconditioned sweeps around the made-up operator q = h * p and the diagonal preconditioner z = r / m: any vector
    length, no grid (tests/test_pcg_gpu.py drives ofdft_cg_* with the same pair)"""

    def __init__(self, diag, m):
        T.DiagCgBackend.__init__(self, diag)
        self.m = m

    def apply(self, r, n_elec):
        return r / self.m

    def seed_pre(self, x, r, p, q, z, S, bb, rr, iters, rho, phir, first, ready, rtol=0.0, maxiter=1 << 30):
        """the state in front of one sweep, taken from elsewhere (a device solver's): that sweep is then judged alone"""
        self.seed(x, r, p, q, S, bb, rr, iters, rtol, maxiter)
        self.z, self.rho, self.phir, self.first, self.ready = z, rho, phir, first, ready
        return self
