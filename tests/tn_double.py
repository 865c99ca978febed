"""numpy double of the chi-space Hessian-vector product (ofdft_hessian_vector_chi: professad_amd/csrc/hvp_kernels.h,
engine_hvp.inc.h) on top of tests/hvp_double.py, and a numpy backend with HipCgBackend's methods
(professad_amd/csrc/cg_abi.h restated), so that the host logic of optimize.TruncatedNewton, optimize.solve_projected and
optimize.density_response runs without a device (tests/test_tn_cpu.py) and the device product can be compared on grids that
have no golden (tests/test_tn_gpu.py, tests/test_second_order_extents_gpu.py); DiagCgBackend puts the same sweeps around a made-up
diagonal operator, the yardstick of the solver's own test (tests/test_cg_sweeps_gpu.py).  Not the product: nothing in professad_amd
imports it.
"""
import numpy as np

import hvp_double as D

CG_RUNNING, CG_CONVERGED, CG_MAXITER, CG_CURVATURE = 0, 1, 2, 3


def density(box, phi, n_elec):
    """-> S, c, n of the closure (system.py:846-847)"""
    dV = abs(np.linalg.det(box)) / phi.size
    S = float((phi * phi).sum())
    c = n_elec / (S * dV)
    return S, c, c * phi * phi


def hessian_vector_chi(box, phi, d, g, n_elec, terms, alpha=5 / 6, beta=5 / 6):
    """-> (dict dHd, phiHd, a, S, dmu; H d) as Engine.hessian_vector_chi(..., want_scalars=True) returns them; g None = zeros"""
    dV = abs(np.linalg.det(box)) / phi.size
    S, c, n = density(box, phi, n_elec)
    g = np.zeros_like(phi) if g is None else g
    a = float((phi * d).sum())
    dn = 2 * c * phi * d - (2 * a / S) * n
    dv = D.hessian_vector(box, n, dn, terms, alpha, beta)[1]
    dmu = (float((dv * n).sum()) * dV + float((g * d).sum())) / n_elec
    with np.errstate(divide='ignore', invalid='ignore'):
        quot = np.where(phi != 0, d * g / phi, 0.0)
    Hd = -(2 * a / S) * g + quot + 2 * c * phi * (dv - dmu) * dV
    return dict(dHd=float((d * Hd).sum()), phiHd=float((phi * Hd).sum()), a=a, S=S, dmu=dmu), Hd


class NumpyCgBackend:
    """the solver state and sweeps of ofdft_cg_* in numpy; the product is hessian_vector_chi above"""

    def __init__(self, box, shape, terms, alpha=5 / 6, beta=5 / 6):
        self.box, self.terms, self.al, self.be = box, terms, alpha, beta
        self.dV = abs(np.linalg.det(box)) / int(np.prod(shape))
        self.products = 0

    def start(self, phi, b, rtol, maxiter):
        self.S = float((phi * phi).sum())
        self.r = b - phi * (float((phi * b).sum()) / self.S)
        self.p = self.r.copy()
        self.x = np.zeros_like(phi)
        self.q = None
        self.rr = self.bb = float((self.r * self.r).sum())
        self.rtol, self.maxiter, self.iters = rtol, maxiter, 0
        self.reason = CG_RUNNING if self.rr > 0 else CG_CONVERGED

    def product(self, phi, g, n_elec, reuse):
        s, self.q = hessian_vector_chi(self.box, phi, self.p, g, n_elec, self.terms, self.al, self.be)
        self.products += 1
        return s['dHd'], s['phiHd']

    def step(self, phi, pq, phiq):
        assert self.reason == CG_RUNNING
        if not pq > 0:
            if self.iters == 0:
                self.x = self.p.copy()
            self.reason = CG_CURVATURE
            return self.reason
        alpha = self.rr / pq
        self.x = self.x + alpha * self.p
        self.r = self.r - alpha * (self.q - phi * (phiq / self.S))
        self.iters += 1
        rr_old, self.rr = self.rr, float((self.r * self.r).sum())
        if not self.rr > self.rtol ** 2 * self.bb:
            self.reason = CG_CONVERGED
        elif self.iters >= self.maxiter:
            self.reason = CG_MAXITER
        else:
            self.direction(phi, rr_old)
        return self.reason

    def direction(self, phi, rr_old):
        """the direction sweep of a step, alone: p = P r + (r.r / r.r of the iteration before) p"""
        self.p = (self.r - phi * (float((phi * self.r).sum()) / self.S)) + (self.rr / rr_old) * self.p

    def status(self):
        return self.iters, self.reason, (np.sqrt(self.rr / self.bb) if self.bb > 0 else 0.0)

    def solution(self):
        return self.x.copy()

    def hv(self, den, w):
        return D.hessian_vector(self.box, den, w, self.terms, self.al, self.be)[1]


def diag_inputs(n, seed=0):
    """phi, b, h of the made-up diagonal problem: magnitudes uniform in [0.5, 1.5], random signs for b, positive phi and h"""
    rng = np.random.default_rng(1000003 * seed + n)
    phi, h = 0.5 + rng.random(n), 0.5 + rng.random(n)
    b = (0.5 + rng.random(n)) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    return phi, b, h


class DiagCgBackend(NumpyCgBackend):
    """the same sweeps around a made-up operator q = h * p with a fixed diagonal h: any vector length, no grid
    (tests/test_cg_sweeps_gpu.py drives ofdft_cg_* with the same operator)"""

    def __init__(self, diag):
        self.h, self.dV, self.products = diag, 1.0, 0

    def product(self, phi, g, n_elec, reuse):
        assert reuse == (self.products > 0)
        self.q = self.h * self.p
        self.products += 1
        return float((self.p * self.q).sum()), float((phi * self.q).sum())

    def seed(self, x, r, p, q, S, bb, rr, iters, rtol=0.0, maxiter=1 << 30):
        """the state in front of one `step`, taken from elsewhere (a device solver's): that step is then judged alone"""
        self.x, self.r, self.p, self.q = x, r, p, q
        self.S, self.bb, self.rr, self.iters = S, bb, rr, iters
        self.rtol, self.maxiter, self.reason = rtol, maxiter, CG_RUNNING
        return self

    def hv(self, den, w):
        raise NotImplementedError('a made-up operator has no density')
