"""GPU test: the single-column solver (ofdft_cg_*) is the one-column case of the lockstep solver (ofdft_cgm_*), bit for bit.

ofdft_cg_* are wrappers round ofdft_cgm_* with ncols_max = 1 (professad_amd/csrc/cg_abi.h): they pass the scalars p.q and phi.q as
one-element arrays and report column 0's reason.  For the same phi, b, h and m three handles run side by side, around q = h * p and
z = r / m as tests/test_cg_sweeps_gpu.py and tests/test_response_multi_gpu.py drive them:
    an ofdft_cg handle;  an ofdft_cgm handle for one column;  an ofdft_cgm handle for three columns with b in column 2
(columns 0 and 1 carry another right-hand side and b = 0, which ends at the start).  x, r, p, every info_host and every status are
equal, not close: a column's sweeps and sums do not depend on how many columns run beside it, nor on the entry that started them.

Lengths: 45 (an odd count: the tail element, and an odd column stride in the caller's stack of right-hand sides), 16^3, and one
element past 2 * kRedThreads * kRedBlocks (csrc/pointwise_kernels.h), where the grid is at its cap and the tail makes a second trip.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import pcg_double as P
import test_cg_sweeps_gpu as S
import test_response_multi_gpu as M
import tn_double as T
from professad_amd import _native as N

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
STEPS = 6


def reduction_constants():
    src = open(os.path.join(os.path.dirname(os.path.abspath(N.__file__)), 'csrc', 'pointwise_kernels.h')).read()
    return [int(re.search(r'constexpr int %s = (\d+);' % k, src).group(1)) for k in ('kRedThreads', 'kRedBlocks')]


LENGTHS = [45, 16 * 16 * 16, 2 * int(np.prod(reduction_constants())) + 1]
dev = M.dev


class One(S.Solver):
    """tests/test_cg_sweeps_gpu.Solver with the calls of the preconditioned mode"""

    def __init__(self, n, hdiag):
        super().__init__(n, hdiag)
        zp = C.c_void_p(0)
        assert self.lib.ofdft_cg_z(self._h, C.byref(zp)) == N.OK
        self.z = torch.as_tensor(S._Raw(zp.value, self.n, '<f8'), device=DEV)
        self.z.fill_(float('nan'))
        self.dinfo = (C.c_double * 4)()

    def set_pre(self, on):
        assert self.lib.ofdft_cg_set_preconditioned(self._h, 1 if on else 0) == N.OK

    def direction(self, phi):
        reason = C.c_int(-1)
        rc = self.lib.ofdft_cg_direction(self._h, C.c_void_p(phi.data_ptr()), self.dinfo, C.byref(reason), self._stream())
        assert rc == N.OK, self.err()
        return reason.value

    def close(self):
        self.z = None
        super().close()


class Trio:
    """the three handles on one problem; `same` asserts that what the single-column handle holds is what column 0 of the
    one-column handle and column 2 of the three-column handle hold"""

    def __init__(self, n, pre):
        self.n, self.pre = n, pre
        phi, b, h = T.diag_inputs(n, seed=31)
        _phi, b0, h0 = T.diag_inputs(n, seed=32)
        m, m0 = P.diag_precond(n, seed=31), P.diag_precond(n, seed=32)
        self.phi = dev(phi)
        self.bs = dev(np.stack([b0, np.zeros(n), b]))          # (3, n): column 1 starts at an odd element when n is odd
        self.hs, self.ms = dev(np.stack([h0, h, h])), dev(np.stack([m0, m, m]))
        self.one, self.m1, self.m3 = One(n, self.hs[2]), M.MSolver(n, 1), M.MSolver(n, 3)
        for s in (self.one, self.m1, self.m3):
            s.set_pre(pre)

    def close(self):
        for s in (self.one, self.m1, self.m3):
            s.close()

    def same(self, what):
        one, m1, m3 = self.one, self.m1, self.m3
        for name in ('x', 'r', 'p'):
            a = getattr(one, name)
            assert torch.equal(a, getattr(m1, name)[0]) and torch.equal(a, getattr(m3, name)[2]), (what, name)
        st = one.status()
        assert st == m1.status(0) == m3.status(2), what
        return st

    def start(self, rtol, maxiter):
        self.one.start(self.phi, self.bs[2], rtol, maxiter)
        assert self.m1.start_rc(self.phi, self.bs[2:], rtol, maxiter) == N.OK, self.m1.err()
        assert self.m3.start_rc(self.phi, self.bs, rtol, maxiter) == N.OK, self.m3.err()
        assert tuple(self.one.info) == tuple(self.m1.info) == tuple(self.m3.info[6:9])
        assert self.m3.status(1) == (0, N.CG_CONVERGED, 0.0) and self.m3.status(0)[:2] == (0, N.CG_RUNNING)
        assert self.same('start')[:2] == (0, N.CG_RUNNING)

    def direction(self):
        one, m1, m3 = self.one, self.m1, self.m3
        torch.div(one.r, self.ms[2], out=one.z)
        m1.z[0].copy_(m1.r[0] / self.ms[2])
        m3.z.copy_(m3.r / self.ms)
        reason = one.direction(self.phi)
        for s in (m1, m3):
            rc, _running = s.direction_rc(self.phi)
            assert rc == N.OK, s.err()
        assert tuple(one.dinfo) == tuple(m1.dinfo) == tuple(m3.dinfo[8:12])
        assert self.same('direction')[1] == reason
        return reason

    def step(self, pq=None):
        """one step of all three; `pq` replaces p.q of the shared column (the curvature exit)"""
        one, m1, m3 = self.one, self.m1, self.m3
        torch.mul(one.hd, one.p, out=one.q)
        m1.q[0].copy_(self.hs[2] * m1.p[0])
        m3.q.copy_(self.hs * m3.p)
        assert torch.equal(one.q, m1.q[0]) and torch.equal(one.q, m3.q[2])
        pq = float(torch.dot(one.p, one.q)) if pq is None else pq
        phiq = float(torch.dot(self.phi, one.q))
        pq0, phiq0 = float(torch.dot(m3.p[0], m3.q[0])), float(torch.dot(self.phi, m3.q[0]))
        reason = one.step(self.phi, pq, phiq)
        rc, _running = m1.step_rc(self.phi, [pq], [phiq])
        assert rc == N.OK, m1.err()
        rc, _running = m3.step_rc(self.phi, [pq0, float('nan'), pq], [phiq0, float('nan'), phiq])
        assert rc == N.OK, m3.err()
        assert self.same('step')[1] == reason
        return reason


@pytest.fixture
def trio():
    made = []

    def factory(*args):
        made.append(Trio(*args))
        return made[-1]
    yield factory
    for t in made:
        t.close()


@pytest.mark.parametrize('pre', [False, True], ids=['plain', 'preconditioned'])
@pytest.mark.parametrize('n', LENGTHS)
def test_one_column_is_the_single_solver_bit_for_bit(trio, n, pre):
    """start and six steps (with the direction call in front of each in preconditioned mode) up to the iteration cap, then a
    second solve on the same handles driven into the first-step curvature exit, where x = p"""
    t = trio(n, pre)
    t.start(0.0, STEPS)
    for k in range(STEPS):
        if pre:
            assert t.direction() == N.CG_RUNNING
        assert t.step() == (N.CG_RUNNING if k + 1 < STEPS else N.CG_MAXITER)
    it, reason, rel = t.same('end')
    assert (it, reason) == (STEPS, N.CG_MAXITER) and 0.0 < rel < 1.0
    sol = t.one.solution()
    assert torch.equal(sol, t.one.x) and torch.equal(sol, t.m1.solution(1)[0]) and torch.equal(sol, t.m3.solution(3)[2])
    # non-positive curvature in front of the first update
    t.start(1e-8, 50)
    if pre:
        assert t.direction() == N.CG_RUNNING
    p0 = t.one.p.clone()
    assert t.step(pq=-1.0) == N.CG_CURVATURE
    assert t.same('curvature')[:2] == (0, N.CG_CURVATURE)
    assert torch.equal(t.one.x, p0) and torch.equal(t.one.p, p0) and torch.equal(t.one.solution(), p0)
    assert t.m3.status(0)[:2] == (1, N.CG_RUNNING)          # the column beside it went on
