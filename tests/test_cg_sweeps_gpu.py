"""GPU tests of the device conjugate-gradient solver on its own (ofdft_cg_*: professad_amd/csrc/cg_kernels.h, cg_abi.h), without
an engine: the ABI is driven directly, as optimize.HipCgBackend drives it, on torch's current stream, around a made-up operator
q = h * p with a fixed diagonal h formed in torch from the solver's own p and written into its own q (ofdft_cg_vectors), so that
any vector length is possible.  The yardstick is tests/tn_double.py: NumpyCgBackend's statement of each sweep (DiagCgBackend).

Lengths: around one block of pairs (511, 512, 513), the smallest (1, 2, 3; at n = 1 the projected b is rounding noise, so that
length pins the launch with no pair at all, n2 = 0, and the tail element, and little else), 17^3, and the lengths at which the grid-stride loops
under the cap of 1024 blocks x 256 threads of pairs make a second trip: 524 288 is exactly one full trip, 524 289 sends the odd
tail element alone into the second, 786 433 makes a partial second trip, 1 048 577 two full trips plus the tail.

Bounds.  Both are derived, not measured; every test prints what it observed as `MEASURE ...` before it asserts (MEASURED_* below
hold the figures of an MI355X run, for the record only).
  elementwise: 128 eps times the sum of the magnitudes of the terms of that element's expression (r = b - s phi; x + alpha p;
      r - alpha q + alpha s phi; r - s phi + beta p): FMA contraction on the device, and alpha, beta, s formed on the host from
      device sums on one side and numpy sums on the other.
  sums: 64 eps sum|terms| against math.fsum.  A thread adds at most 3 terms serially (n <= 1 048 577), then 6 shuffle levels, 4
      waves, and a second stage of 4 serial adds and 8 tree levels: under 32 roundings; 64 leaves a factor of two.
  fp32 library (float vectors, double accumulators): 128 * 2^-23 elementwise; 4 * 2^-23 sum|terms| for the sums, whose products
      are rounded in fp32 and whose accumulation is fp64.
Each sweep is judged alone: the numpy backend is re-seeded from the device's state in front of the sweep, so rounding does not
compound over the iterations.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import tn_double as T
from professad_amd import _native as N
from professad_amd import optimize

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LENGTHS = [1, 2, 3, 511, 512, 513, 4913, 524288, 524289, 786433, 1048577]
EPS = {N.F64: 2.0 ** -52, N.F32: 2.0 ** -23}
ELEMENT_BOUND = 128.0                                  # x eps x the magnitudes of the element's terms
SUMS_BOUND = {N.F64: 64.0, N.F32: 4.0}                 # x eps x sum|terms|
STEPS = 6

# observed on an MI355X, in units of the bounds' eps (largest over the lengths): elementwise ratio, sums ratio
MEASURED_F64 = dict(element=3.60, sums=1.84)             # both at n = 786 433; 0.55 .. 3.6 and 0.89 .. 1.84 over the lengths
MEASURED_F32 = dict(element=1.28, sums=0.046)            # n = 524 289 and n = 513
# whole solve on a general phi, device against numpy: |x - x_numpy|_2 / |b_p|_2 per length.  Asserted at 10 x (the project's rule for
# a comparison with the numpy double); a figure below one rounding of a double counts as that rounding
MEASURED_SOLVE = {513: 1.71e-16, 524289: 1.66e-16}


class _Raw:
    """zero-copy view of solver-owned device memory for torch"""

    def __init__(self, ptr, count, typestr):
        self.__cuda_array_interface__ = {'shape': (int(count),), 'typestr': typestr, 'data': (int(ptr), False), 'version': 2}


class Solver:
    """ofdft_cg_* of one library around q = h * p, with HipCgBackend's methods (optimize.solve_projected drives it) and the raw
    return codes where a test needs them"""

    def __init__(self, n, hdiag=None, code=N.F64):
        self.lib, self.n, self.hd = N.load(code), int(n), hdiag
        self.dtype = torch.double if code == N.F64 else torch.float32
        self._h = C.c_void_p(0)
        assert self.lib.ofdft_cg_create(C.byref(self._h), self.n, torch.device(DEV).index) == N.OK
        ptrs = [C.c_void_p(0) for _ in range(4)]
        assert self.lib.ofdft_cg_vectors(self._h, *[C.byref(p) for p in ptrs]) == N.OK
        ts = '<f8' if code == N.F64 else '<f4'
        self.x, self.r, self.p, self.q = [torch.as_tensor(_Raw(p.value, self.n, ts), device=DEV) for p in ptrs]
        assert all(v.dtype == self.dtype and v.numel() == self.n for v in (self.x, self.r, self.p, self.q))
        for v in (self.x, self.r, self.p, self.q):          # whatever a sweep fails to write stays visible
            v.fill_(float('nan'))
        self.info = (C.c_double * 3)()
        self.products = 0

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)

    def err(self):
        return self.lib.ofdft_cg_last_error(self._h).decode()

    # ---- raw calls -> return code
    def start_rc(self, phi, b, rtol, maxiter):
        self.products = 0
        return self.lib.ofdft_cg_start(self._h, C.c_void_p(phi.data_ptr()), C.c_void_p(b.data_ptr()), float(rtol), int(maxiter),
                                       self.info, self._stream())

    def step_rc(self, phi, pq, phiq):
        reason = C.c_int(-1)
        rc = self.lib.ofdft_cg_step(self._h, C.c_void_p(phi.data_ptr()), float(pq), float(phiq), C.byref(reason), self._stream())
        return rc, reason.value

    def solution_rc(self, out):
        return self.lib.ofdft_cg_solution(self._h, C.c_void_p(out.data_ptr()), self._stream())

    # ---- HipCgBackend's methods
    def start(self, phi, b, rtol, maxiter):
        assert self.start_rc(phi, b, rtol, maxiter) == N.OK, self.err()

    def product(self, phi, g, n_elec, reuse):
        assert reuse == (self.products > 0)
        torch.mul(self.hd, self.p, out=self.q)
        self.products += 1
        return float(torch.dot(self.p, self.q)), float(torch.dot(phi, self.q))

    def step(self, phi, pq, phiq):
        rc, reason = self.step_rc(phi, pq, phiq)
        assert rc == N.OK, self.err()
        return reason

    def status(self):
        it, reason, rel = C.c_int(-1), C.c_int(-1), C.c_double(-1.0)
        assert self.lib.ofdft_cg_status(self._h, C.byref(it), C.byref(reason), C.byref(rel)) == N.OK
        return it.value, reason.value, rel.value

    def solution(self):
        out = torch.empty(self.n, dtype=self.dtype, device=DEV)
        assert self.solution_rc(out) == N.OK, self.err()
        return out

    def close(self):
        if self._h:
            self.x = self.r = self.p = self.q = None
            self.lib.ofdft_cg_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@pytest.fixture
def make():
    """Solver(...) whose handle and device vectors are released when the test ends, passed or failed"""
    made = []

    def factory(*args, **kw):
        made.append(Solver(*args, **kw))
        return made[-1]
    yield factory
    for s in made:
        s.close()


inputs = T.diag_inputs          # magnitudes uniform in [0.5, 1.5]: random signs for b, positive phi and h


def dev(a, code=N.F64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.double if code == N.F64 else torch.float32, device=DEV)


def host(t):
    """a device vector as float64 (exact for float vectors)"""
    return t.cpu().numpy().astype(np.float64)


def fsum(a):
    return math.fsum(a.tolist())


def ratio(got, want, mag):
    """max |got - want| / mag over the elements; an element without magnitude must be met exactly"""
    d = np.abs(got - want)
    assert not np.isnan(d).any()
    zero = mag == 0.0
    assert not d[zero].any()
    return float((d[~zero] / mag[~zero]).max()) if (~zero).any() else 0.0


def sweeps(make, n, code):
    """ofdft_cg_start and STEPS x ofdft_cg_step against the numpy statement of each sweep -> (largest elementwise ratio, largest
    sums ratio), both in units of eps"""
    eps = EPS[code]
    phi, b, h = inputs(n)
    tphi, tb = dev(phi, code), dev(b, code)
    phi, b, h = host(tphi), host(tb), host(dev(h, code))          # what the device holds (rounded to float for the fp32 library)
    s = make(n, dev(h, code), code)
    worst_e = worst_s = 0.0

    # ---- start: b.b is not returned; phi.phi, phi.b and the r.r of the projected b are
    s.start(tphi, tb, 0.0, 1 << 20)
    rr0, S, phib = s.info[0], s.info[1], s.info[2]
    ref = T.DiagCgBackend(h)
    ref.start(phi, b, 0.0, 1 << 20)
    x, r, p = host(s.x), host(s.r), host(s.p)
    sc = ref.r - b                                                 # -s phi as numpy formed it
    worst_e = max(worst_e, ratio(r, ref.r, np.abs(b) + np.abs(sc)) / eps)
    assert not x.any() and np.array_equal(p, r)
    for got, terms in ((S, phi * phi), (phib, phi * b), (rr0, r * r)):
        scale = fsum(np.abs(terms))
        worst_s = max(worst_s, abs(got - fsum(terms)) / (eps * scale) if scale else abs(got))
    it, reason, rel = s.status()
    assert (it, reason) == (0, N.CG_RUNNING if rr0 > 0.0 else N.CG_CONVERGED) and rel == (1.0 if rr0 > 0.0 else 0.0)

    # ---- steps
    rr, steps = rr0, 0
    while reason == N.CG_RUNNING and steps < STEPS:
        torch.mul(s.hd, s.p, out=s.q)
        q = host(s.q)
        pq, phiq = float(np.dot(p, q)), float(np.dot(phi, q))
        assert pq > 0.0
        reason = s.step(tphi, pq, phiq)
        steps += 1
        x1, r1, p1 = host(s.x), host(s.r), host(s.p)
        # the update sweep, from the device's state in front of it (an iteration cap of one more keeps numpy from the direction sweep)
        ref.seed(x, r, p, q, S, rr0, rr, steps - 1, maxiter=steps)
        ref.step(phi, pq, phiq)
        alpha, su = rr / pq, phiq / S
        worst_e = max(worst_e, ratio(x1, ref.x, np.abs(x) + np.abs(alpha * p)) / eps)
        worst_e = max(worst_e, ratio(r1, ref.r, np.abs(r) + np.abs(alpha * q) + np.abs(alpha * su * phi)) / eps)
        it, reason2, rel = s.status()
        assert (it, reason2) == (steps, reason)
        rr1 = rel * rel * rr0                                      # the device's r.r, a rounding or two apart
        scale = fsum(r1 * r1)
        worst_s = max(worst_s, abs(rr1 - scale) / (eps * scale) if scale else abs(rr1))
        if reason == N.CG_RUNNING:
            # the direction sweep, from the device's new residual and its sum
            ref.seed(x1, r1, p, q, S, rr0, rr1, steps)
            ref.direction(phi, rr)
            beta, sd = rr1 / rr, float((phi * r1).sum()) / S
            worst_e = max(worst_e, ratio(p1, ref.p, np.abs(r1) + np.abs(sd * phi) + np.abs(beta * p)) / eps)
        else:                                                      # (rtol = 0: only a residual of exactly zero ends the solve)
            assert reason == N.CG_CONVERGED and rel == 0.0 and np.array_equal(p1, p)
        x, r, p, rr = x1, r1, p1, rr1
    assert steps == STEPS or reason == N.CG_CONVERGED
    assert np.array_equal(host(s.solution()), x)
    return worst_e, worst_s


# ------------------------------------------------------------------------------- 1: every sweep against its numpy statement
@pytest.mark.parametrize('n', LENGTHS)
def test_sweeps_match_the_numpy_statement(make, n):
    """x, r, p after ofdft_cg_start and after each of six ofdft_cg_step calls, elementwise within 128 eps of the magnitudes of
    their terms; info_host of the start and the relative residual of ofdft_cg_status within 64 eps sum|terms| of math.fsum over
    the downloaded vectors.  The solver's vectors are filled with NaN beforehand: an element a sweep does not reach fails.
    Observed on an MI355X over the eleven lengths: elementwise at most 3.6 eps, sums at most 1.84 eps (MEASURED_F64)."""
    e, sm = sweeps(make, n, N.F64)
    print('MEASURE cg sweeps f64 n=%d: elementwise %.2f eps of the terms (bound %g), sums %.2f eps of sum|terms| (bound %g)'
          % (n, e, ELEMENT_BOUND, sm, SUMS_BOUND[N.F64]))
    assert e <= ELEMENT_BOUND and sm <= SUMS_BOUND[N.F64]


@pytest.mark.parametrize('n', [513, 524289])
def test_sweeps_of_the_fp32_library_match_the_numpy_statement(make, n):
    """libofdft_hip_f32.so exports the same entries with float vectors (double accumulators and scalars): the same comparison
    against numpy in double at 128 * 2^-23 elementwise and 4 * 2^-23 sum|terms|.
    Observed on an MI355X: elementwise 1.07 / 1.28, sums 0.046 / 0.001 (in units of 2^-23) at n = 513 / 524 289."""
    e, sm = sweeps(make, n, N.F32)
    print('MEASURE cg sweeps f32 n=%d: elementwise %.2f eps32 of the terms (bound %g), sums %.3f eps32 of sum|terms| (bound %g)'
          % (n, e, ELEMENT_BOUND, sm, SUMS_BOUND[N.F32]))
    assert e <= ELEMENT_BOUND and sm <= SUMS_BOUND[N.F32]


# ------------------------------------------------------------------------------- 2: whole solves
RTOL, MAXITER = 1e-10, 200


@pytest.mark.parametrize('n', [513, 524289])
def test_whole_solves_on_the_diagonal_operator(make, n):
    """(a) phi an eigenvector of the operator: phi lives on the first half of the vector, where h is constant, so P and H
    commute and x = (projected b) / h exactly.  (b) a general positive phi: against optimize.solve_projected on the numpy
    backend, with the same iteration count.
    Bounds: the spectrum of P H P on the complement of phi lies in [0.5, 1.5], so |x - x*|_2 <= 2 |r|_2, and |r|_2 <= rtol |b|_2
    for the recurrence's residual, which drifts from the true one by a few eps |H| |x| per iteration (64 eps per iteration
    allowed).  (b) runs the same iterations on both sides, which differ by rounding only: 10 x the figure measured on an MI355X
    (MEASURED_SOLVE), as for every comparison with the numpy double; twice the bound of (a) stays as a ceiling.
    Measured on an MI355X, n = 513 / 524 289: (a) 4.3e-11 / 5.6e-11 of |b_p|_2 (bound 2.0e-10), (b) 1.71e-16 / 1.66e-16 of |b_p|_2; 18
    iterations in every run, device and numpy."""
    phi, b, h = inputs(n, seed=1)
    m = (n + 1) // 2
    # (a)
    phi_a, h_a = phi.copy(), h.copy()
    phi_a[m:] = 0.0
    h_a[:m] = 0.8125
    s = make(n, dev(h_a))
    x, it, reason, rel, nprod = optimize.solve_projected(s, dev(phi_a), None, dev(b), 1.0, RTOL, MAXITER)
    bp = b - phi_a * (math.fsum((phi_a * b).tolist()) / math.fsum((phi_a * phi_a).tolist()))
    want = bp / h_a
    da = float(np.linalg.norm(host(x) - want) / np.linalg.norm(bp))
    bound_a = 2.0 * (RTOL + 64 * EPS[N.F64] * it)
    ref = T.DiagCgBackend(h_a)
    _x, it_np, reason_np, _rel, _np = optimize.solve_projected(ref, phi_a, None, b, 1.0, RTOL, MAXITER)
    print('MEASURE cg solve n=%d eigenvector phi: |x - b_p / h|_2 / |b_p|_2 %.2e (bound %.2e)  iterations %d (numpy %d) residual %.2e'
          % (n, da, bound_a, it, it_np, rel))
    assert (reason, nprod) == (N.CG_CONVERGED, it) and rel <= RTOL and 1 < it < MAXITER
    assert (it, reason) == (it_np, reason_np)
    assert da <= bound_a
    # (b) on the same handle: a second start behaves as the first
    s.hd = dev(h)
    x, it, reason, rel, nprod = optimize.solve_projected(s, dev(phi), None, dev(b), 1.0, RTOL, MAXITER)
    ref = T.DiagCgBackend(h)
    x_np, it_np, reason_np, rel_np, nprod_np = optimize.solve_projected(ref, phi, None, b, 1.0, RTOL, MAXITER)
    bp = b - phi * (math.fsum((phi * b).tolist()) / math.fsum((phi * phi).tolist()))
    db = float(np.linalg.norm(host(x) - x_np) / np.linalg.norm(bp))
    bound_b = 10 * max(MEASURED_SOLVE[n], EPS[N.F64])
    print('MEASURE cg solve n=%d general phi: |x - numpy|_2 / |b_p|_2 %.2e (bound %.2e)  iterations %d (numpy %d) residual %.2e (numpy %.2e)'
          % (n, db, bound_b, it, it_np, rel, rel_np))
    assert (it, reason, nprod) == (it_np, reason_np, nprod_np) and reason == N.CG_CONVERGED and rel <= RTOL
    assert db <= bound_b <= 4.0 * (RTOL + 64 * EPS[N.F64] * it)


# ------------------------------------------------------------------------------- 3: exits and state
def running(s, tphi, tb, updates, maxiter=50):
    """a started solve after `updates` genuine iterations"""
    s.start(tphi, tb, 0.0, maxiter)
    for _ in range(updates):
        assert s.step(tphi, *s.product(tphi, None, 1.0, s.products > 0)) == N.CG_RUNNING


@pytest.mark.parametrize('n', [513, 524289])
def test_exit_reasons_and_what_they_leave_behind(make, n):
    phi, b, h = inputs(n, seed=2)
    tphi, tb = dev(phi), dev(b)
    s = make(n, dev(h))
    # the iteration cap: exactly two updates, no direction sweep after the second
    running(s, tphi, tb, 1, maxiter=2)
    x1, p1 = s.x.clone(), s.p.clone()
    assert s.step(tphi, *s.product(tphi, None, 1.0, True)) == N.CG_MAXITER
    it, reason, rel = s.status()
    assert (it, reason) == (2, N.CG_MAXITER) and 0.0 < rel < 1.0
    assert torch.equal(s.p, p1) and not torch.equal(s.x, x1)
    rc, _reason = s.step_rc(tphi, 1.0, 0.0)
    assert rc == N.ESTATE and 'the solve has ended' in s.err()
    assert torch.equal(s.solution(), s.x)
    # non-positive curvature, or a NaN in its place, in front of the first update: x = p, the steepest-descent step
    for pq in (-1.0, 0.0, float('nan')):
        running(s, tphi, tb, 0)
        p0 = s.p.clone()
        assert s.step(tphi, pq, 0.0) == N.CG_CURVATURE
        assert s.status()[:2] == (0, N.CG_CURVATURE)
        assert torch.equal(s.x, p0) and torch.equal(s.p, p0) and torch.equal(s.solution(), p0)
        rc, _reason = s.step_rc(tphi, 1.0, 0.0)
        assert rc == N.ESTATE and 'the solve has ended' in s.err()
    # the same after two updates: x stays what it was
    for pq in (-1.0, 0.0, float('nan')):
        running(s, tphi, tb, 2)
        x2, r2, p2 = s.x.clone(), s.r.clone(), s.p.clone()
        rel2 = s.status()[2]
        assert s.step(tphi, pq, 0.0) == N.CG_CURVATURE
        assert s.status() == (2, N.CG_CURVATURE, rel2)
        assert torch.equal(s.x, x2) and torch.equal(s.r, r2) and torch.equal(s.p, p2) and bool(x2.any())
    # a NaN inside q (here in the last element: the odd tail) ends the solve through the residual sum
    running(s, tphi, tb, 1)
    pq, phiq = s.product(tphi, None, 1.0, True)
    s.q[n - 1] = float('nan')
    assert s.step(tphi, pq, phiq) == N.CG_CURVATURE
    it, reason, rel = s.status()
    assert (it, reason) == (2, N.CG_CURVATURE) and math.isnan(rel)
    # b = 0: x = 0 solves it at the start
    s.start(tphi, torch.zeros_like(tb), 1e-12, 50)
    assert s.status() == (0, N.CG_CONVERGED, 0.0) and s.info[0] == 0.0 and s.info[2] == 0.0 and s.info[1] > 0.0
    assert not bool(s.x.any()) and not bool(s.solution().any())
    rc, _reason = s.step_rc(tphi, 1.0, 0.0)
    assert rc == N.ESTATE and 'the solve has ended' in s.err()


@pytest.mark.parametrize('n', [513, 524289])
def test_refusals_and_a_second_start(make, n):
    phi, b, h = inputs(n, seed=3)
    tphi, tb, out = dev(phi), dev(b), torch.empty(n, dtype=torch.double, device=DEV)
    s = make(n, dev(h))
    # nothing started yet
    rc, _reason = s.step_rc(tphi, 1.0, 0.0)
    assert rc == N.ESTATE and 'ofdft_cg_step: ofdft_cg_start has not been called' in s.err()
    assert s.solution_rc(out) == N.ESTATE and 'ofdft_cg_solution: ofdft_cg_start has not been called' in s.err()
    # arguments
    for rtol, maxiter in ((-1e-3, 10), (float('nan'), 10), (1e-3, 0)):
        assert s.start_rc(tphi, tb, rtol, maxiter) == N.EINVAL
    assert s.start_rc(torch.zeros_like(tphi), tb, 1e-3, 10) == N.EINVAL and 'phi is zero everywhere' in s.err()
    rc, _reason = s.step_rc(tphi, 1.0, 0.0)                        # a refused start leaves nothing started
    assert rc == N.ESTATE and 'has not been called' in s.err()
    # a used handle against a fresh one: the same bits and scalars
    phi2, b2, _h = inputs(n, seed=4)
    running(s, dev(phi2), dev(b2), 3)
    fresh = make(n, s.hd)
    log = []
    for t in (s, fresh):
        t.start(tphi, tb, 0.0, 50)
        rec = [tuple(t.info), t.status()]
        for _ in range(3):
            pq, phiq = t.product(tphi, None, 1.0, t.products > 0)
            rec += [pq, phiq, t.step(tphi, pq, phiq), t.status()]
        log.append(rec)
    assert log[0] == log[1]
    assert torch.equal(s.x, fresh.x) and torch.equal(s.r, fresh.r) and torch.equal(s.p, fresh.p) and torch.equal(s.q, fresh.q)


# ------------------------------------------------------------------------------- 4: reproducibility
def test_two_handles_give_the_same_bits(make):
    """n = 1 048 577 (two full trips of every loop plus the tail): x, r, p after the start and after each of six steps, and every
    scalar the calls return, are identical between two handles given the same inputs."""
    n = 1048577
    phi, b, h = inputs(n, seed=5)
    tphi, tb, th = dev(phi), dev(b), dev(h)
    a, c = make(n, th), make(n, th)
    for t in (a, c):
        t.start(tphi, tb, 0.0, 50)
    assert tuple(a.info) == tuple(c.info) and a.status() == c.status()
    assert torch.equal(a.x, c.x) and torch.equal(a.r, c.r) and torch.equal(a.p, c.p)
    for _ in range(STEPS):
        sa, sc = a.product(tphi, None, 1.0, a.products > 0), c.product(tphi, None, 1.0, c.products > 0)
        assert sa == sc
        assert a.step(tphi, *sa) == c.step(tphi, *sc) == N.CG_RUNNING
        assert a.status() == c.status()
        assert torch.equal(a.x, c.x) and torch.equal(a.r, c.r) and torch.equal(a.p, c.p)
    assert a.status()[0] == STEPS
