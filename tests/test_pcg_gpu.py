"""GPU tests of the preconditioned conjugate gradients: the operator ofdft_precondition (Engine.precondition)
against numpy, the new solver entries (ofdft_cg_set_preconditioned, ofdft_cg_z, ofdft_cg_direction and the preconditioned mode of
ofdft_cg_start / ofdft_cg_step) sweep by sweep against tests/pcg_double.py, the golden response of tests/golden/tn_g16r.npz with
`precondition='auto'`, and force_constants / elastic_constants / bulk_modulus / optimize_density end to end on the fcc-Al 16^3
case with and without the option.

Bounds.
  operator: 10 x the largest max|z - z_numpy| / max|z| measured on an MI355X over the grids, both pipelines and both kappa^2
      (MEASURED['operator']); the same bound for sum z = sum r / kappa^2, relative to sum|z|.
  sweeps: those of tests/test_cg_sweeps_gpu.py -- elementwise 128 eps of the magnitudes of the element's terms, sums 64 eps of
      sum|terms| against math.fsum -- each sweep judged alone from the device's state in front of it.
  solve and end to end: the bounds the existing tests use for the plain solver at the same rtol (tests/test_tn_gpu.py:
      10 x MEASURED_DN, MEASURED_DMU; tests/test_force_constants_gpu.py: SOLVE_BOUND; tests/test_elastic_gpu.py: SOLVE_BOUND).
Every test prints its figures as `MEASURE ...` before it asserts.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import cases
import elastic_double as ED
import fc_cases
import fc_double as FD
import pcg_double as P
import test_cg_sweeps_gpu as S
import tn_cases
import tn_double as T
from professad_amd import _native as N
from professad_amd import elastic, ions, optimize, synth
from professad_amd.engine import Engine
from professad_amd.force_constants import force_constants

pytestmark = pytest.mark.gpu
GOLDEN = os.path.dirname(os.path.abspath(cases.__file__))
DEV = 'cuda:0'
TERMS = list(tn_cases.TERMS)
EPS = 2.0 ** -52

# measured on an MI355X (per-case figures in the tests' docstrings)
# operator: 5.9e-16 / 1.0e-15 / 1.3e-15 / 6.8e-16 / 1.1e-15 on 16^3 / 17^3 / (18, 20, 16) / 48^3 / (128, 128, 64), the same to two digits in
# both pipelines; sum z at most 4.2e-16 of sum|z|.  Sweeps: elementwise at most 1.96 eps, sums at most 1.76 eps.  Golden response: 16
# iterations (numpy 16, plain 153), dn 2.72e-12, dmu 1.33e-10.  a16: TN 26 products (plain 98); force constants row 1 1.5e-11 of
# max|Phi| in 22-23 iterations (plain 101-102); K 1.6e-11, C 2.1e-11 in 22-23 iterations (plain 100).
MEASURED = dict(operator=1.31e-15, golden_iters=16, dn=2.72e-12, dmu=1.33e-10)
DN_BOUND, DMU_BOUND = 10 * 2.64e-12, 10 * 1.33e-10            # tests/test_tn_gpu.py: 10 x MEASURED_DN, 10 x MEASURED_DMU
FC_SOLVE_BOUND, FC_RTOL = 1e-8, 1e-11                           # tests/test_force_constants_gpu.py: SOLVE_BOUND, RTOL
EL_SOLVE_BOUND, EL_RTOL = min(60 * 1e-11 * 0.3, 1e-10), 1e-11   # tests/test_elastic_gpu.py: SOLVE_BOUND, RTOL
E_BOUND_HA = 1e-10


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.double, device=DEV)


# ------------------------------------------------------------------------------- 1: the operator
GRIDS = {
    'p16': ((16, 16, 16), lambda: synth.cubic_cell(16)),                  # powers of two
    'o17': ((17, 17, 17), lambda: synth.cubic_cell(17)),                  # odd: chirp-z
    't18': ((18, 20, 16), lambda: synth.triclinic_cell(1.0)),             # triclinic, chirp-z
    'm48': ((48, 48, 48), lambda: synth.cubic_cell(48)),                  # mixed radix
    'x128': ((128, 128, 64), lambda: synth.triclinic_cell(4.0)),          # the cross-wave x pass; more than one trip of the sweeps
}
KAPPA2 = (0.3, 1.1)
_OP = {}


def operator_reference(name):
    """box, r and the numpy z per kappa^2 of a grid; computed once and shared by the two pipelines"""
    if name not in _OP:
        shape, box = GRIDS[name]
        box = box()
        r = np.random.default_rng(20250 + sum(shape)).standard_normal(shape)
        _OP[name] = (box, r, {k2: P.precondition(box, r, k2) for k2 in KAPPA2})
    return _OP[name]


@pytest.mark.parametrize('pipeline', [0, 1])
@pytest.mark.parametrize('name', list(GRIDS))
def test_operator_matches_numpy(name, pipeline):
    """Engine.precondition against irfftn(rfftn(r) / (k^2 + kappa^2)) for a seeded normal field, kappa^2 = 0.3 and 1.1, with the
    default pipeline (fused x pass or chirp-z x-mix) and with OFDFT_OPT_PIPELINE = 1 (forward, multiply, inverse).
    Measured on an MI355X: see MEASURED['operator'] (the largest) and the per-grid figures printed."""
    shape = GRIDS[name][0]
    box, r, want = operator_reference(name)
    eng = Engine(shape, DEV).set_cell(box)
    eng.set_option(N.OPT_PIPELINE, pipeline)
    tr = dev(r)
    worst = worst_sum = 0.0
    for k2 in KAPPA2:
        tz = eng.precondition(tr, k2)
        assert torch.equal(tr, dev(r))                         # the input is left alone
        z = tz.cpu().numpy()
        worst = max(worst, float(np.abs(z - want[k2]).max() / np.abs(want[k2]).max()))
        worst_sum = max(worst_sum, abs(math.fsum(z.ravel().tolist()) - math.fsum(r.ravel().tolist()) / k2) / float(np.abs(z).sum()))
        out = torch.full_like(tr, float('nan'))
        assert eng.precondition(tr, k2, out=out) is out and torch.equal(out, tz)      # bitwise reproducible, every element written
    fast = eng.query(N.Q_FAST_PATH)
    eng.close()
    print('MEASURE pcg operator %s %s pipeline %d (fast path %d): z %.2e  sum z %.2e' % (name, shape, pipeline, fast, worst, worst_sum))
    assert worst <= 10 * MEASURED['operator'] and worst_sum <= 10 * MEASURED['operator']


# ------------------------------------------------------------------------------- 2: the retained fields
@pytest.mark.parametrize('name,pipeline', [('g16r', 0), ('g16r', 1), ('g17r', 0), ('g18t', 0)])
def test_precondition_leaves_the_retained_fields(name, pipeline):
    """hessian_vector_chi(reuse_density=False), precondition, hessian_vector_chi(reuse_density=True): bitwise the product without the
    call in between, and still with the smaller transform count"""
    g = np.load(os.path.join(GOLDEN, 'tn_%s.npz' % name))
    box, phi, d, _vext, n_elec = tn_cases.make_inputs(name)
    eng = Engine(phi.shape, DEV).set_cell(box).set_terms(TERMS)
    eng.set_option(N.OPT_PIPELINE, pipeline)
    tphi, td, tg = dev(phi), dev(d), dev(g['g'])
    eng.hessian_vector_chi(tphi, td, tg, n_elec)
    s0, H0 = eng.hessian_vector_chi(tphi, td, tg, n_elec, reuse_density=True, want_scalars=True)
    count = eng.query(N.Q_FFT_COUNT)
    eng.hessian_vector_chi(tphi, td, tg, n_elec)
    z = eng.precondition(td, 0.7)
    s1, H1 = eng.hessian_vector_chi(tphi, td, tg, n_elec, reuse_density=True, want_scalars=True)
    assert torch.equal(H0, H1) and s0 == s1
    z2 = eng.precondition(td, 0.7)
    assert torch.equal(eng.hessian_vector_chi(tphi, td, tg, n_elec, reuse_density=True), H0) and torch.equal(z, z2)
    assert eng.query(N.Q_FFT_COUNT) == count
    eng.close()


# ------------------------------------------------------------------------------- 3: the sweeps alone
LENGTHS = [1, 2, 255, 257, 262145, 1048577]
ITERATIONS = 3


class PSolver(S.Solver):
    """tests/test_cg_sweeps_gpu.Solver with the preconditioned entries around z = r / m"""

    def __init__(self, n, hdiag, mdiag):
        super().__init__(n, hdiag)
        self.md = mdiag
        ptr = C.c_void_p(0)
        assert self.lib.ofdft_cg_z(self._h, C.byref(ptr)) == N.OK and ptr.value
        again = C.c_void_p(0)
        assert self.lib.ofdft_cg_z(self._h, C.byref(again)) == N.OK and again.value == ptr.value
        self.z = torch.as_tensor(S._Raw(ptr.value, self.n, '<f8'), device=DEV)
        self.z.fill_(float('nan'))
        self.dinfo = (C.c_double * 4)()
        self.preconditioned = False

    def set_pre(self, on):
        assert self.lib.ofdft_cg_set_preconditioned(self._h, 1 if on else 0) == N.OK
        self.preconditioned = bool(on)

    def direction_rc(self, phi):
        reason = C.c_int(-1)
        rc = self.lib.ofdft_cg_direction(self._h, C.c_void_p(phi.data_ptr()), self.dinfo, C.byref(reason), self._stream())
        return rc, reason.value

    def pre_direction(self, phi, n_elec):
        torch.div(self.r, self.md, out=self.z)
        rc, reason = self.direction_rc(phi)
        assert rc == N.OK, self.err()
        return reason

    def close(self):
        self.z = None
        super().close()


@pytest.fixture
def pmake():
    made = []

    def factory(*args):
        made.append(PSolver(*args))
        return made[-1]
    yield factory
    for s in made:
        s.close()


host, fsum, ratio = S.host, S.fsum, S.ratio


def sum_dev(got, terms):
    scale = fsum(np.abs(terms))
    return abs(got - fsum(terms)) / (EPS * scale) if scale else abs(got)


@pytest.mark.parametrize('n', LENGTHS)
def test_preconditioned_sweeps_match_the_numpy_statement(pmake, n):
    """ofdft_cg_start in preconditioned mode, then three times: z = r / m written by the test, ofdft_cg_direction, q = h p,
    ofdft_cg_step -- x, r, p elementwise and r.z, phi.z, rho, r.r as sums, each against pcg_double.DiagPcgBackend seeded with the
    device's state in front of the sweep.  The solver's vectors are NaN beforehand.  At n = 1 the projected b is rounding noise or zero:
    that length pins the launches with no pair at all and the tail element."""
    phi, b, h = T.diag_inputs(n)
    m = P.diag_precond(n)
    tphi, tb = dev(phi), dev(b)
    s = pmake(n, dev(h), dev(m))
    s.set_pre(1)
    s.start(tphi, tb, 0.0, 1 << 20)
    rr0, Sd = s.info[0], s.info[1]
    ref = P.DiagPcgBackend(h, m)
    ref.start(phi, b, 0.0, 1 << 20)
    x, r = host(s.x), host(s.r)
    worst_e = ratio(r, ref.r, np.abs(b) + np.abs(ref.r - b)) / EPS
    worst_s = sum_dev(rr0, r * r)
    assert not x.any()
    it, reason, rel = s.status()
    assert (it, reason) == (0, N.CG_RUNNING if rr0 > 0.0 else N.CG_CONVERGED)
    if reason != N.CG_RUNNING:
        rc, _reason = s.direction_rc(tphi)
        assert rc == N.ESTATE and 'the solve has ended' in s.err()
    p = host(s.p)
    rr, rho, phir, steps = rr0, 0.0, 0.0, 0
    while reason == N.CG_RUNNING and steps < ITERATIONS:
        # ---- the direction: two sums, one sweep
        torch.div(s.r, s.md, out=s.z)
        z = host(s.z)
        rc, reason = s.direction_rc(tphi)
        assert rc == N.OK, s.err()
        rz, phiz, rho1, beta = tuple(s.dinfo)
        worst_s = max(worst_s, sum_dev(rz, r * z), sum_dev(phiz, phi * z))
        terms = np.concatenate([r * z, [-phir * fsum(phi * z) / Sd]])
        worst_s = max(worst_s, sum_dev(rho1, terms))
        if reason != N.CG_RUNNING:               # (n = 1: nothing is left of r in the complement of phi)
            assert reason == N.CG_CURVATURE and not rho1 > 0.0 and np.array_equal(host(s.p), p, equal_nan=True)
            break
        assert beta == (0.0 if steps == 0 else rho1 / rho)
        ref.seed_pre(x, r, p, None, z, Sd, rr0, rr, steps, rho, phir, steps == 0, False)
        ref.direction_sweeps(phi)
        p1 = host(s.p)
        sd = phiz / Sd
        mag = np.abs(z) + np.abs(sd * phi) + (np.abs(beta * p) if steps else 0.0)
        worst_e = max(worst_e, ratio(p1, ref.p, mag) / EPS)
        rc, _reason = s.direction_rc(tphi)
        assert rc == N.ESTATE and 'already formed' in s.err()
        # ---- the product and the update sweep
        torch.mul(s.hd, s.p, out=s.q)
        q = host(s.q)
        pq, phiq = float(np.dot(p1, q)), float(np.dot(phi, q))
        if not pq > 0.0:                         # (n = 1: p = z - phi (phi.z) / S may vanish altogether)
            assert n == 1 and s.step(tphi, pq, phiq) == N.CG_CURVATURE
            break
        reason = s.step(tphi, pq, phiq)
        steps += 1
        x1, r1 = host(s.x), host(s.r)
        assert np.array_equal(host(s.p), p1)                       # no direction sweep inside the step
        ref.seed_pre(x, r, p1, q, z, Sd, rr0, rr, steps - 1, rho1, phir, False, True, maxiter=1 << 30)
        ref.step(phi, pq, phiq)
        alpha, su = rho1 / pq, phiq / Sd
        worst_e = max(worst_e, ratio(x1, ref.x, np.abs(x) + np.abs(alpha * p1)) / EPS)
        worst_e = max(worst_e, ratio(r1, ref.r, np.abs(r) + np.abs(alpha * q) + np.abs(alpha * su * phi)) / EPS)
        it, reason2, rel = s.status()
        assert (it, reason2) == (steps, reason)
        rr1 = rel * rel * rr0
        worst_s = max(worst_s, sum_dev(rr1, r1 * r1))
        x, r, p, rr, rho, phir = x1, r1, p1, rr1, rho1, fsum(phi * r1)
    assert steps == ITERATIONS or n <= 2
    if s.status()[1] != N.CG_CURVATURE or steps:
        assert np.array_equal(host(s.solution()), host(s.x))
    print('MEASURE pcg sweeps n=%d: %d iterations, elementwise %.2f eps of the terms (bound %g), sums %.2f eps of sum|terms| (bound %g)'
          % (n, steps, worst_e, S.ELEMENT_BOUND, worst_s, S.SUMS_BOUND[N.F64]))
    assert worst_e <= S.ELEMENT_BOUND and worst_s <= S.SUMS_BOUND[N.F64]


def pre_running(s, tphi, tb, updates, rtol=0.0, maxiter=50):
    """a started preconditioned solve after `updates` whole iterations"""
    s.set_pre(1)
    s.start(tphi, tb, rtol, maxiter)
    for _ in range(updates):
        assert s.pre_direction(tphi, 1.0) == N.CG_RUNNING
        assert s.step(tphi, *s.product(tphi, None, 1.0, s.products > 0)) == N.CG_RUNNING


@pytest.mark.parametrize('n', [257, 262145])
def test_exits_states_and_the_plain_mode_afterwards(pmake, n):
    """every exit reason of the preconditioned mode, the OFDFT_ESTATE refusals, two handles bit for bit, and a plain solve on a handle
    that has run preconditioned against a fresh handle, bit for bit"""
    phi, b, h = T.diag_inputs(n, seed=2)
    m = P.diag_precond(n, seed=2)
    tphi, tb, th, tm = dev(phi), dev(b), dev(h), dev(m)
    s = pmake(n, th, tm)
    # before any start; plain mode
    rc, _r = s.direction_rc(tphi)
    assert rc == N.ESTATE and 'ofdft_cg_start has not been called' in s.err()
    s.start(tphi, tb, 0.0, 50)
    rc, _r = s.direction_rc(tphi)
    assert rc == N.ESTATE and 'plain mode' in s.err()
    s.set_pre(1)                                       # takes effect at the next start: the running solve stays plain
    rc, _r = s.direction_rc(tphi)
    assert rc == N.ESTATE and 'plain mode' in s.err()
    assert s.step(tphi, *s.product(tphi, None, 1.0, False)) == N.CG_RUNNING
    reason = C.c_int(0)
    assert s.lib.ofdft_cg_direction(s._h, None, None, C.byref(reason), None) == N.EINVAL
    assert s.lib.ofdft_cg_z(s._h, None) == N.EINVAL
    # a step before its direction
    pre_running(s, tphi, tb, 0)
    rc, _r = s.step_rc(tphi, 1.0, 0.0)
    assert rc == N.ESTATE and 'ofdft_cg_direction has not formed' in s.err()
    pre_running(s, tphi, tb, 1)
    rc, _r = s.step_rc(tphi, 1.0, 0.0)
    assert rc == N.ESTATE and 'ofdft_cg_direction has not formed' in s.err()
    # the iteration cap
    pre_running(s, tphi, tb, 1, maxiter=2)
    assert s.pre_direction(tphi, 1.0) == N.CG_RUNNING
    assert s.step(tphi, *s.product(tphi, None, 1.0, True)) == N.CG_MAXITER
    it, reason, rel = s.status()
    assert (it, reason) == (2, N.CG_MAXITER) and 0.0 < rel < 1.0
    for rc in (s.direction_rc(tphi)[0], s.step_rc(tphi, 1.0, 0.0)[0]):
        assert rc == N.ESTATE and 'the solve has ended' in s.err()
    assert torch.equal(s.solution(), s.x)
    # convergence: against the numpy recurrence through optimize.solve_projected, the same count
    s.products = 0
    xs, it, reason, rel, nprod = optimize.solve_projected(s, tphi, None, tb, 1.0, 1e-10, 200)
    x_np, it_np, reason_np, _rel, _n = optimize.solve_projected(P.DiagPcgBackend(h, m), phi, None, b, 1.0, 1e-10, 200)
    bp = b - phi * (fsum(phi * b) / fsum(phi * phi))
    apart = float(np.linalg.norm(host(xs) - x_np) / np.linalg.norm(bp))
    print('MEASURE pcg solve n=%d: iterations %d (numpy %d) residual %.2e |x - numpy|_2 / |b_p|_2 %.2e' % (n, it, it_np, rel, apart))
    assert (reason, nprod) == (N.CG_CONVERGED, it) and rel <= 1e-10 and (it, reason) == (it_np, reason_np)
    assert apart <= 4.0 * (1e-10 + 64 * EPS * it)               # tests/test_cg_sweeps_gpu.py: twice 2 (rtol + 64 eps per iteration)
    # non-positive curvature in front of the first update: x = p = P z
    for pq in (-1.0, 0.0, float('nan')):
        pre_running(s, tphi, tb, 0)
        assert s.pre_direction(tphi, 1.0) == N.CG_RUNNING
        p0 = s.p.clone()
        assert s.step(tphi, pq, 0.0) == N.CG_CURVATURE and s.status()[:2] == (0, N.CG_CURVATURE)
        assert torch.equal(s.x, p0) and torch.equal(s.solution(), p0)
    # ... and after one update: x stays
    pre_running(s, tphi, tb, 1)
    assert s.pre_direction(tphi, 1.0) == N.CG_RUNNING
    x1 = s.x.clone()
    assert s.step(tphi, -1.0, 0.0) == N.CG_CURVATURE and torch.equal(s.x, x1) and bool(x1.any())
    # a preconditioner that is not positive definite, or a NaN in z (the odd tail element): the direction ends the solve, x and p stay
    for spoil in ('negative', 'nan'):
        pre_running(s, tphi, tb, 1)
        x1, p1 = s.x.clone(), s.p.clone()
        torch.div(s.r, s.md, out=s.z)
        if spoil == 'negative':
            s.z.neg_()
        else:
            s.z[n - 1] = float('nan')
        rc, reason = s.direction_rc(tphi)
        assert (rc, reason) == (N.OK, N.CG_CURVATURE) and s.status()[:2] == (1, N.CG_CURVATURE)
        assert torch.equal(s.x, x1) and torch.equal(s.p, p1)
    # b = 0
    s.set_pre(1)
    s.start(tphi, torch.zeros_like(tb), 1e-12, 50)
    assert s.status() == (0, N.CG_CONVERGED, 0.0)
    # two handles, the same bits, every scalar included
    c = pmake(n, th, tm)
    logs = []
    for t in (s, c):
        t.products = 0
        t.set_pre(1)
        t.start(tphi, tb, 0.0, 50)
        rec = [tuple(t.info)]
        for _ in range(ITERATIONS):
            rec += [t.pre_direction(tphi, 1.0), tuple(t.dinfo)]
            pq, phiq = t.product(tphi, None, 1.0, t.products > 0)
            rec += [pq, phiq, t.step(tphi, pq, phiq), t.status()]
        logs.append(rec)
    assert logs[0] == logs[1]
    assert all(torch.equal(getattr(s, v), getattr(c, v)) for v in 'xrpqz')
    # plain mode on the used handle against a fresh one
    fresh = pmake(n, th, tm)
    logs = []
    for t in (s, fresh):
        t.products = 0
        t.set_pre(0)
        t.start(tphi, tb, 0.0, 50)
        rec = [tuple(t.info), t.status()]
        for _ in range(ITERATIONS):
            pq, phiq = t.product(tphi, None, 1.0, t.products > 0)
            rec += [pq, phiq, t.step(tphi, pq, phiq), t.status()]
        logs.append(rec)
    assert logs[0] == logs[1]
    assert all(torch.equal(getattr(s, v), getattr(fresh, v)) for v in 'xrpq')


# ------------------------------------------------------------------------------- 4: the solve
def test_golden_response_with_the_preconditioner_and_a_plain_solve_afterwards():
    """the golden tn_g16r response at rtol 1e-12 with precondition='auto': the numpy double's iteration count to +-1 (16), dn and dmu
    within the plain solve's bounds; then a plain solve on the same handle, bitwise a fresh handle's, in the golden's 153 iterations"""
    g = np.load(os.path.join(GOLDEN, 'tn_g16r.npz'))
    box, phi, _d, _vext, n_elec = tn_cases.make_inputs('g16r')
    dv = tn_cases.response_dv(phi.shape)
    ref = optimize.density_response(None, g['chi_gs'], n_elec, dv, rtol=1e-12, maxiter=500, backend=P.PcgBackend(box, phi.shape, TERMS))
    eng = Engine(phi.shape, DEV).set_cell(box).set_terms(TERMS)
    chi, tdv = dev(g['chi_gs']), dev(dv)
    b = optimize.HipCgBackend(eng, precondition='auto')
    r = optimize.density_response(eng, chi, n_elec, tdv, rtol=1e-12, maxiter=500, backend=b)
    dn = r['dn'].cpu().numpy()
    ddn = float(np.abs(dn - g['dn']).max() / np.abs(g['dn']).max())
    dmu = abs(r['dmu'] - float(g['dmu'])) / abs(float(g['dmu']))
    again = optimize.density_response(eng, chi, n_elec, tdv, rtol=1e-12, maxiter=500, precondition='auto')
    fixed = optimize.density_response(eng, chi, n_elec, tdv, rtol=1e-12, maxiter=500,
                                      precondition=optimize.kinetic_kappa2(n_elec, abs(np.linalg.det(box))))
    b.set_precondition(None)
    plain = optimize.density_response(eng, chi, n_elec, tdv, rtol=1e-12, maxiter=500, backend=b)
    fresh = optimize.density_response(eng, chi, n_elec, tdv, rtol=1e-12, maxiter=500)
    b.close()
    eng.close()
    print('MEASURE pcg response g16r: dn %.2e dmu %.2e iterations %d (numpy %d, plain %d) products %d residual %.2e'
          % (ddn, dmu, r['iterations'], ref['iterations'], plain['iterations'], r['hvp_count'], r['rel_residual']))
    assert r['reason'] == optimize.CG_CONVERGED and r['rel_residual'] <= 1e-12
    assert abs(r['iterations'] - ref['iterations']) <= 1 and r['hvp_count'] == r['iterations']
    assert ddn <= DN_BOUND and dmu <= DMU_BOUND
    assert abs(dn.sum()) <= 64 * EPS * np.abs(dn).sum()
    for other in (again, fixed):                                  # a handle of its own, 'auto' spelled out: the same bits
        assert torch.equal(other['dn'], r['dn']) and other['iterations'] == r['iterations'] and other['dmu'] == r['dmu']
    assert plain['iterations'] == fresh['iterations'] and abs(plain['iterations'] - int(g['cg_iters'])) <= 1
    assert torch.equal(plain['dn'], fresh['dn']) and plain['dmu'] == fresh['dmu'] and plain['rel_residual'] == fresh['rel_residual']


# ------------------------------------------------------------------------------- 5: end to end
_RUN = {}


def a16():
    box, shape, frac, _den, raw, k_max = fc_cases.make_inputs('a16')
    tab = ions.recpot_table(raw, k_max)
    return box, shape, frac, tab, np.full(frac.shape[0], float(tab[2]))


def run():
    """truncated-Newton ground states of the a16 case with and without tn_precondition; run once and shared"""
    if not _RUN:
        box, shape, frac, tab, z = a16()
        eng = Engine(shape, DEV).set_cell(box)
        vext = ions.ionic_potential(eng, box, [(frac, tab)])
        eng.set_terms(TERMS)
        kw = dict(volume=abs(np.linalg.det(box)), n_method='TN')
        _RUN['plain'] = optimize.optimize_density(eng, float(z.sum()), vext, **kw)
        _RUN['pre'] = optimize.optimize_density(eng, float(z.sum()), vext, tn_precondition='auto', **kw)
        _RUN['eng'] = eng
    return _RUN


def test_truncated_newton_with_the_preconditioner():
    """optimize_density(n_method='TN', tn_precondition='auto') from the uniform density: the plain run's energy within 1e-10 Ha in
    at most 40 products and at most half the plain run's (the numpy double: 26 against 98)"""
    s = run()
    plain, pre = s['plain'], s['pre']
    dE = pre['E_Ha'] - plain['E_Ha']
    print('MEASURE pcg TN a16: products %d (plain %d) outer %d (plain %d) E - E_plain %.2e Ha' %
          (pre['hvp_count'], plain['hvp_count'], pre['iterations'], plain['iterations'], dE))
    assert plain['converged'] and pre['converged']
    assert abs(dE) <= E_BOUND_HA
    assert pre['hvp_count'] <= 40 and 2 * pre['hvp_count'] <= plain['hvp_count']


def test_force_constants_with_the_preconditioner():
    """force_constants(primitive_ion_indices=[1], precondition='auto') at rtol 1e-11 against the numpy-driven plain matrix within the
    bound of the plain end-to-end test (1e-8 of max|Phi|); the three solves take at most half the plain run's iterations"""
    box, shape, frac, tab, _z = a16()
    s = run()
    chi, eng = s['plain']['chi'], s['eng']
    kw = dict(primitive_ion_indices=[1], rtol=FC_RTOL)
    plain = force_constants(eng, box, [(frac, tab)], chi, **kw)
    pre = force_constants(eng, box, [(frac, tab)], chi, precondition='auto', **kw)
    ref = force_constants(None, box, [(frac, tab)], chi.cpu().numpy(), backend=FD.NumpyFcBackend(box, shape, [(frac, tab)], TERMS), **kw)
    scale = float(np.abs(ref['phi']).max())
    d, dp = float(np.abs(pre['phi'] - ref['phi']).max() / scale), float(np.abs(plain['phi'] - ref['phi']).max() / scale)
    print('MEASURE pcg fc a16 row 1: Phi - numpy %.2e (plain %.2e) of max|Phi| %.4e  iterations %s (plain %s) products %d (plain %d)'
          % (d, dp, scale, pre['iterations'], plain['iterations'], pre['hvp_count'], plain['hvp_count']))
    assert all(x == optimize.CG_CONVERGED for x in pre['reason']) and max(pre['rel_residual']) <= FC_RTOL
    assert d <= FC_SOLVE_BOUND
    assert 2 * sum(pre['iterations']) <= sum(plain['iterations'])
    for k in ('ion_ion', 'direct'):                               # the parts without a solve do not see the option
        assert np.array_equal(pre['parts'][k], plain['parts'][k])


def test_bulk_modulus_with_the_preconditioner():
    """elastic_constants / bulk_modulus(precondition='auto') at rtol 1e-11 against the numpy-driven plain run within the bound of the
    plain end-to-end test; the six solves take at most half the plain run's iterations"""
    box, shape, frac, tab, _z = a16()
    s = run()
    chi, eng = s['plain']['chi'], s['eng']
    plain = elastic.elastic_constants(eng, box, [(frac, tab)], chi, rtol=EL_RTOL)
    pre = elastic.elastic_constants(eng, box, [(frac, tab)], chi, rtol=EL_RTOL, precondition='auto')
    K = elastic.bulk_modulus(eng, box, [(frac, tab)], chi, rtol=EL_RTOL, precondition='auto')
    ref = elastic.elastic_constants(None, box, [(frac, tab)], chi.cpu().numpy(), rtol=EL_RTOL,
                                    backend=ED.NumpyElasticBackend(box, shape, [(frac, tab)], TERMS))
    dK = abs(K - ref['bulk_modulus']) / abs(ref['bulk_modulus'])
    dC = float(np.abs(pre['C'] - ref['C']).max() / np.abs(ref['C']).max())
    print('MEASURE pcg elastic a16: K %.10e - numpy %.2e  C - numpy %.2e  iterations %s (plain %s)'
          % (K, dK, dC, pre['iterations'], plain['iterations']))
    assert K == pre['bulk_modulus']
    assert all(x == optimize.CG_CONVERGED for x in pre['reason']) and max(pre['rel_residual']) <= EL_RTOL
    assert dK <= EL_SOLVE_BOUND and dC <= EL_SOLVE_BOUND
    assert 2 * sum(pre['iterations']) <= sum(plain['iterations'])


# ------------------------------------------------------------------------------- 6: refusals
def test_refusals_by_name():
    from professad_amd.distributed import DistEngine
    box, shape, frac, tab, _z = a16()
    r = torch.ones(shape, dtype=torch.double, device=DEV)
    eng = Engine(shape, DEV).set_cell(box).set_terms(TERMS)
    for bad in (0.0, -0.5, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='kappa2'):
            eng.precondition(r, bad)
        rc = eng.lib.ofdft_precondition(eng._ctx, C.c_void_p(r.data_ptr()), C.c_void_p(torch.empty_like(r).data_ptr()), bad, eng._stream())
        assert rc == N.EINVAL and 'kappa2' in eng.lib.ofdft_last_error(eng._ctx).decode()
    with pytest.raises(ValueError, match='z is r'):
        eng.precondition(r, 1.0, out=r)
    rc = eng.lib.ofdft_precondition(eng._ctx, C.c_void_p(r.data_ptr()), C.c_void_p(r.data_ptr()), 1.0, eng._stream())
    assert rc == N.EINVAL and 'z_dev must not be r_dev' in eng.lib.ofdft_last_error(eng._ctx).decode()
    for bad in (0.0, 'yes'):
        with pytest.raises(ValueError, match='precondition'):
            optimize.HipCgBackend(eng, precondition=bad)
        with pytest.raises(ValueError, match='precondition'):
            force_constants(eng, box, [(frac, tab)], r, precondition=bad)
    with pytest.raises(ValueError, match='tn_precondition'):
        optimize.optimize_density(eng, 12.0, None, volume=abs(np.linalg.det(box)), tn_precondition='auto')
    eng.close()
    e32 = Engine(shape, DEV, dtype=torch.float32).set_cell(box).set_terms(['ion_electron', 'tf'])
    with pytest.raises(NotImplementedError, match='fp64'):
        e32.precondition(r.float(), 1.0)
    rc = e32.lib.ofdft_precondition(e32._ctx, C.c_void_p(r.data_ptr()), C.c_void_p(torch.empty_like(r).data_ptr()), 1.0, e32._stream())
    assert rc == N.EINVAL and 'fp64 library' in e32.lib.ofdft_last_error(e32._ctx).decode()
    with pytest.raises(NotImplementedError, match='fp64'):
        optimize.HipCgBackend(e32, precondition='auto')
    with pytest.raises(NotImplementedError, match='fp64'):
        force_constants(e32, box, [(frac, tab)], r.float(), precondition='auto')
    e32.close()
    de = DistEngine(shape, DEV).set_cell(torch.as_tensor(box)).set_terms(['ion_electron', 'tf'])
    with pytest.raises(NotImplementedError, match='single-GPU'):
        de.precondition(r, 1.0)
    with pytest.raises(NotImplementedError, match='single-GPU'):
        optimize.HipCgBackend(de, precondition='auto')
    with pytest.raises(NotImplementedError, match='single-GPU'):
        elastic.bulk_modulus(de, box, [(frac, tab)], r, precondition='auto')
    with pytest.raises(NotImplementedError, match='single-GPU'):
        optimize.optimize_density(de, 12.0, volume=abs(np.linalg.det(box)), n_method='TN', tn_precondition='auto')
    de.close()
