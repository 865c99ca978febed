"""numpy double of the lockstep multi-column solver (ofdft_cgm_*: professad_amd/csrc/cg_abi.h, cg_kernels.h) with
optimize.HipCgMultiBackend's methods: one solo numpy backend per column (tests/tn_double.py, tests/pcg_double.py), so that a
column of optimize.solve_projected_multi is by construction the recurrence optimize.solve_projected runs on that backend, and
the host logic of the batched drivers runs without a device (tests/test_response_multi_cpu.py).  The device sweeps and solves are
judged against the same solo backends, column by column (tests/test_response_multi_gpu.py).  Not the product: nothing in professad_amd
imports it.
"""
import numpy as np

from tn_double import CG_RUNNING


class MultiCgDouble:
    """`make(j)` -> the solo backend of column j (NumpyCgBackend, DiagCgBackend or their preconditioned variants)"""

    def __init__(self, make):
        self.make = make
        self.proto = make(0)          # dV, hv and the mode, before any start
        self.dV = self.proto.dV
        self.cols = []
        self.products = 0

    @property
    def preconditioned(self):
        return bool(getattr(self.proto, 'preconditioned', False))

    def _running(self):
        return [j for j, c in enumerate(self.cols) if c.reason == CG_RUNNING]

    def _reasons(self):
        return [c.reason for c in self.cols]

    def start(self, phi, bs, rtol, maxiter):
        self.cols = [self.make(j) for j in range(len(bs))]
        for c, b in zip(self.cols, bs):
            c.start(phi, b, rtol, maxiter)

    def pre_direction(self, phi, n_elec):
        for j in self._running():
            self.cols[j].pre_direction(phi, n_elec)
        return self._reasons()

    def product(self, phi, n_elec, reuse):
        """the sums of an ended column are not defined (NaN here): nothing may read them"""
        pq, phiq = [float('nan')] * len(self.cols), [float('nan')] * len(self.cols)
        for j in self._running():
            pq[j], phiq[j] = self.cols[j].product(phi, None, n_elec, reuse)
        self.products += 1
        return pq, phiq

    def step(self, phi, pq, phiq):
        for j in self._running():
            self.cols[j].step(phi, pq[j], phiq[j])
        return self._reasons()

    def status(self):
        return [c.status() for c in self.cols]

    def solution(self):
        return np.stack([c.solution() for c in self.cols])

    def hv(self, den, w):
        return self.proto.hv(den, w)


def with_batch(backend, batch, make):
    """a driver double (fc_double.NumpyFcBackend, elastic_double.NumpyElasticBackend) that asks for batched solves of `batch`
    columns, as a caller's backend does: the `batch` attribute and `cgm(ncols)`"""
    backend.batch = batch
    backend.cgm = lambda ncols: MultiCgDouble(make)
    return backend
