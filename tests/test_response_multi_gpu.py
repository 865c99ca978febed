"""GPU tests of the batched response solves: ofdft_hessian_vector_chi_multi (Engine.hessian_vector_chi_multi)
against tests/tn_double.py, ofdft_precondition_multi against tests/pcg_double.py, the lockstep solver ofdft_cgm_* sweep by sweep
against the solo numpy backends of tests/tn_double.py and tests/pcg_double.py, optimize.density_response_multi on the golden response
of tests/golden/tn_g16r.npz, and force_constants / elastic_constants / bulk_modulus with `batch` end to end on the fcc-Al 16^3 case.

Bounds.
  product: 10 x the largest max|H d_j - double| / max|double| measured on an MI355X per grid, over the columns, both term sets and
      B = 1, 3, 8 (MEASURED['product']); the scalars at the same bound relative to the sum of the magnitudes of their terms
      (sum|d H d|, sum|phi H d|, sum|dv n| dV / N).  The same bound for a column against the single-column entry.
  preconditioner: 10 x MEASURED['operator'] of tests/test_pcg_gpu.py -- the same operator.
  sweeps: those of tests/test_cg_sweeps_gpu.py -- elementwise 128 eps of the magnitudes of the element's terms, sums 64 eps of
      sum|terms| against math.fsum -- each sweep judged alone from the device's state in front of it.
  solve and end to end: the bounds the existing tests hold (tests/test_tn_gpu.py: 10 x MEASURED_DN, MEASURED_DMU;
      tests/test_force_constants_gpu.py and tests/test_elastic_gpu.py: SOLVE_BOUND), taken from tests/test_pcg_gpu.py's restatement.
Every test prints its figures as `MEASURE ...` before it asserts.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cases
import elastic_double as ED
import fc_double as FD
import hvp_cases
import hvp_double as D
import pcg_double as P
import test_cg_sweeps_gpu as S
import test_pcg_gpu as PG
import test_response_multi_cpu as MC
import tn_cases
import tn_double as T
from professad_amd import _native as N
from professad_amd import elastic, optimize, synth
from professad_amd.engine import Engine
from professad_amd.force_constants import force_constants

pytestmark = pytest.mark.gpu
GOLDEN = os.path.dirname(os.path.abspath(cases.__file__))
DEV = 'cuda:0'
TERMS = list(tn_cases.TERMS)
EPS = 2.0 ** -52

# measured on an MI355X: the largest max|H d_j - double| / max|double| per grid (columns, both term sets, B = 1, 3, 8); the single-column
# entry sits at 3.5e-14 .. 4.9e-14 against the goldens of the first three (tests/test_tn_gpu.py).  For the record: the scalars at most
# 6.9e-15 of the sum of their terms, a column against the single-column entry at most 5.0e-16 of max|H d|; preconditioner 4.3e-16 ..
# 1.4e-15 (a column bitwise the single-column entry's); sweeps elementwise at most 3.5 eps, sums 2.1 eps; golden response dn 2.64e-12 /
# 2.72e-12, dmu 1.33e-10 plain / preconditioned in 153 / 16 iterations, the solo solves' counts; fcc-Al 16^3: two rows of Phi 3.2e-13
# from the numpy-driven matrix with 204 (batch 3) and 102 (batch 8) products instead of 611, K 1.5e-11, C 2.1e-11 with 100 instead of 600
MEASURED = {
    'product': {'g16r': 3.39e-14, 'g17r': 3.11e-14, 'g18t': 3.24e-14, 'm48': 2.85e-14, 'x128': 2.15e-14, 'odd45': 1.15e-14},
}
OPERATOR_BOUND = 10 * PG.MEASURED['operator']
host, fsum, ratio, sum_dev = S.host, S.fsum, S.ratio, PG.sum_dev


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.double, device=DEV)


@pytest.fixture(autouse=True)
def no_gpu_work_after_a_device_error():
    """a test that left the device in an error state ends the session: nothing more is started on that GPU"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit('device error, no further GPU work: %s' % e, returncode=3)


# ------------------------------------------------------------------------------- 1, 2: the product
def synth_inputs(shape, box, seed):
    den = synth.random_density(shape, seed=seed)
    phi = 0.6 * np.sqrt(den)
    return box, phi, float(den.sum() * abs(np.linalg.det(box)) / den.size)


PRODUCT_CASES = {
    'g16r': lambda: tn_cases.make_inputs('g16r'),          # powers of two: fused transforms
    'g17r': lambda: tn_cases.make_inputs('g17r'),          # odd: chirp-z
    'g18t': lambda: tn_cases.make_inputs('g18t'),          # triclinic, chirp-z
    'm48': lambda: synth_inputs((48, 48, 48), synth.cubic_cell(48), 21),                       # mixed radix
    'x128': lambda: synth_inputs((128, 128, 64), synth.triclinic_cell(4.0), 22),               # reductions: more than one trip, the block cap
    'odd45': lambda: synth_inputs((5, 3, 3), synth.cubic_cell(5), 23),                         # odd npts: the tail element; odd column stride
}
EXPONENTS = {'wt': (5 / 6, 5 / 6), 'wgc98': D.WGC98}
_PROD = {}


def product_reference(case, expo):
    """box, phi, n_elec, eight seeded directions and the numpy double's (scalars, H d) per direction; computed once and shared"""
    if (case, expo) not in _PROD:
        inp = PRODUCT_CASES[case]()
        box, phi, n_elec = (inp[0], inp[1], inp[4]) if len(inp) == 5 else inp
        dirs = np.stack([hvp_cases.direction(phi.shape, seed=300 + j) for j in range(8)])
        al, be = EXPONENTS[expo]
        _PROD[(case, expo)] = (box, phi, n_elec, dirs, [T.hessian_vector_chi(box, phi, dirs[j], None, n_elec, TERMS, al, be) for j in range(8)])
    return _PROD[(case, expo)]


@pytest.mark.parametrize('expo', list(EXPONENTS))
@pytest.mark.parametrize('case', list(PRODUCT_CASES))
def test_product_matches_the_double_and_the_single_column_entry(case, expo):
    """Engine.hessian_vector_chi_multi for B = 1, 3, 8 seeded directions against tests/tn_double.hessian_vector_chi (g = None) per
    column, its scalars against the double's sums, each column against Engine.hessian_vector_chi, and the transform counts
    2 (D + B W), with reuse 2 B W.  Measured on an MI355X: MEASURED['product'] and the per-case figures printed."""
    box, phi, n_elec, dirs, ref = product_reference(case, expo)
    al, be = EXPONENTS[expo]
    eng = Engine(phi.shape, DEV).set_cell(box).set_terms(TERMS, dict(wt_alpha=al, wt_beta=be))
    dV = abs(np.linalg.det(box)) / phi.size
    _S, cn, den = T.density(box, phi, n_elec)
    tphi, tdirs = dev(phi), dev(dirs)
    single = []
    for j in range(8):
        single.append(eng.hessian_vector_chi(tphi, tdirs[j].clone(), None, n_elec, reuse_density=j > 0))
        if j < 2:
            count = eng.query(N.Q_FFT_COUNT)
            n0, n1 = (count, None) if j == 0 else (n0, count)
    assert (n0, n1) == ((14, 8) if al != be else (10, 6))
    Dn, W = (n0 - n1) // 2, n1 // 2
    worst = worst_s = worst_1 = 0.0
    for B in (1, 3, 8):
        stack = tdirs[:B].contiguous()
        keep = stack.clone()
        out = torch.full_like(stack, float('nan'))
        s, H = eng.hessian_vector_chi_multi(tphi, stack, n_elec, want_scalars=True, out=out)
        assert H is out and torch.equal(stack, keep)
        assert eng.query(N.Q_FFT_COUNT) == 2 * (Dn + B * W)
        H2 = eng.hessian_vector_chi_multi(tphi, stack, n_elec, reuse_density=True)
        assert eng.query(N.Q_FFT_COUNT) == 2 * B * W
        assert torch.equal(H2, H)
        Hh = H.cpu().numpy()
        assert not np.isnan(Hh).any()
        for j in range(B):
            sd, Hd = ref[j]
            scale = float(np.abs(Hd).max())
            worst = max(worst, float(np.abs(Hh[j] - Hd).max()) / scale)
            worst_1 = max(worst_1, float((H[j] - single[j]).abs().max()) / scale)
            mag = float(np.abs(dirs[j] * Hd).sum())
            dv = Hd / (2 * cn * phi * dV) + sd['dmu']                 # H d = 2 c phi (dv - dmu) dV: dmu = sum dv n dV / N is a sum of these terms
            worst_s = max(worst_s, abs(s[j]['dHd'] - sd['dHd']) / mag, abs(s[j]['phiHd'] - sd['phiHd']) / float(np.abs(phi * Hd).sum()),
                          abs(s[j]['dmu'] - sd['dmu']) / (float(np.abs(dv * den).sum()) * dV / n_elec))
            assert s[j]['a'] == pytest.approx(sd['a'], rel=1e-12, abs=1e-12 * float(np.abs(phi * dirs[j]).sum()))
            assert s[j]['S'] == pytest.approx(sd['S'], rel=1e-13)
    eng.close()
    print('MEASURE multi product %s %s %s: H d %.2e  scalars %.2e  against the single-column entry %.2e  (D, W) = (%d, %d)'
          % (case, phi.shape, expo, worst, worst_s, worst_1, Dn, W))
    bound = 10 * MEASURED['product'][case]
    assert worst <= bound and worst_s <= bound and worst_1 <= bound


# ------------------------------------------------------------------------------- 3: reuse across the entries
@pytest.mark.parametrize('case', ['g16r', 'g17r'])
def test_reuse_across_the_entries_is_bitwise_and_is_invalidated_together(case):
    box, phi, n_elec, dirs, _ref = product_reference(case, 'wt')
    eng = Engine(phi.shape, DEV).set_cell(box).set_terms(TERMS)
    tphi, stack, d0 = dev(phi), dev(dirs[:3]), dev(dirs[0])
    with pytest.raises(RuntimeError, match=r'\(-3\)'):            # nothing retained yet: OFDFT_ESTATE
        eng.hessian_vector_chi_multi(tphi, stack, n_elec, reuse_density=True)
    Hm = eng.hessian_vector_chi_multi(tphi, stack, n_elec)
    s_m, Hm1 = eng.hessian_vector_chi_multi(tphi, stack, n_elec, reuse_density=True, want_scalars=True)
    # single after multi
    Hs1 = eng.hessian_vector_chi(tphi, d0, None, n_elec, reuse_density=True)
    Hs = eng.hessian_vector_chi(tphi, d0, None, n_elec)
    # multi after single, with the preconditioner in between
    z = eng.precondition_multi(stack, 0.7)
    s_m2, Hm2 = eng.hessian_vector_chi_multi(tphi, stack, n_elec, reuse_density=True, want_scalars=True)
    print('MEASURE multi reuse %s: max|difference| multi with reuse %.1e, single after multi %.1e, multi after single and the preconditioner %.1e'
          % (case, float((Hm1 - Hm).abs().max()), float((Hs1 - Hs).abs().max()), float((Hm2 - Hm).abs().max())))
    assert torch.equal(Hm1, Hm)
    assert torch.equal(Hs1, Hs)
    assert torch.equal(Hm2, Hm) and s_m2 == s_m
    assert torch.equal(eng.precondition_multi(stack, 0.7), z)
    assert torch.equal(eng.hessian_vector_chi(tphi, d0, None, n_elec, reuse_density=True), Hs)
    # set_terms, an energy call and set_cell invalidate the fields for both entries
    den = dev(T.density(box, phi, n_elec)[2])
    vext = torch.zeros_like(den)
    scales = iter((1.01, 1.02))                                  # (another cell each time: Engine.set_cell passes an unchanged box by)
    for spoil in (lambda: (eng.set_terms(['tf']), eng.set_terms(TERMS)), lambda: eng.energy_potential(den, vext),
                  lambda: eng.set_cell(box * next(scales))):
        eng.hessian_vector_chi(tphi, d0, None, n_elec)
        spoil()
        with pytest.raises(RuntimeError, match=r'\(-3\)'):
            eng.hessian_vector_chi_multi(tphi, stack, n_elec, reuse_density=True)
        eng.hessian_vector_chi_multi(tphi, stack, n_elec)
        spoil()
        with pytest.raises(RuntimeError, match=r'\(-3\)'):
            eng.hessian_vector_chi(tphi, d0, None, n_elec, reuse_density=True)
    eng.close()


# ------------------------------------------------------------------------------- 4: the preconditioner
_OPM = {}


def operator_reference(name):
    """box, five seeded fields (column 0: that of tests/test_pcg_gpu.py) and the numpy z per column at kappa^2 = 0.3"""
    if name not in _OPM:
        box, r0, _want = PG.operator_reference(name)
        rng = np.random.default_rng(977 + sum(r0.shape))
        r = np.stack([r0] + [rng.standard_normal(r0.shape) for _ in range(4)])
        _OPM[name] = (box, r, np.stack([P.precondition(box, r[j], 0.3) for j in range(5)]))
    return _OPM[name]


@pytest.mark.parametrize('pipeline', [0, 1])
@pytest.mark.parametrize('name', list(PG.GRIDS))
def test_preconditioner_matches_numpy_per_column(name, pipeline):
    """Engine.precondition_multi on five columns (one more than a transform batch) against pcg_double.precondition per column;
    the inputs stay, every output element is written, and a column is bitwise the single-column entry's"""
    box, r, want = operator_reference(name)
    eng = Engine(r.shape[1:], DEV).set_cell(box)
    eng.set_option(N.OPT_PIPELINE, pipeline)
    tr = dev(r)
    out = torch.full_like(tr, float('nan'))
    assert eng.precondition_multi(tr, 0.3, out=out) is out
    assert torch.equal(tr, dev(r))
    z = out.cpu().numpy()
    assert not np.isnan(z).any()
    worst = max(float(np.abs(z[j] - want[j]).max() / np.abs(want[j]).max()) for j in range(5))
    one = eng.precondition(tr[4].clone(), 0.3)
    same = torch.equal(one, out[4])
    eng.close()
    print('MEASURE multi preconditioner %s pipeline %d: z %.2e (bound %.2e)  column 4 bitwise the single entry: %s'
          % (name, pipeline, worst, OPERATOR_BOUND, same))
    assert worst <= OPERATOR_BOUND and same


# ------------------------------------------------------------------------------- 5: the sweeps
class MSolver:
    """ofdft_cgm_* driven directly around q_j = h_j * p_j (and z_j = r_j / m_j), with the raw return codes"""

    def __init__(self, n, ncols_max):
        self.lib, self.n, self.B = N.load(N.F64), int(n), int(ncols_max)
        self._h = C.c_void_p(0)
        assert self.lib.ofdft_cgm_create(C.byref(self._h), self.n, self.B, torch.device(DEV).index) == N.OK
        ptrs = [C.c_void_p(0) for _ in range(5)]
        ld = C.c_longlong(0)
        assert self.lib.ofdft_cgm_vectors(self._h, *[C.byref(p) for p in ptrs[:4]], C.byref(ld)) == N.OK
        assert self.lib.ofdft_cgm_z(self._h, C.byref(ptrs[4])) == N.OK
        self.ld = ld.value
        assert self.ld >= self.n and self.ld % 2 == 0
        self.full = [torch.as_tensor(S._Raw(p.value, self.B * self.ld, '<f8'), device=DEV).view(self.B, self.ld) for p in ptrs]
        for v in self.full:
            v.fill_(float('nan'))
        self.x, self.r, self.p, self.q, self.z = [v[:, :self.n] for v in self.full]
        self.info, self.dinfo = (C.c_double * (3 * self.B))(), (C.c_double * (4 * self.B))()

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)

    def err(self):
        return self.lib.ofdft_cgm_last_error(self._h).decode()

    def set_pre(self, on):
        assert self.lib.ofdft_cgm_set_preconditioned(self._h, 1 if on else 0) == N.OK

    def start_rc(self, phi, bs, rtol, maxiter, ncols=None, stride=None):
        return self.lib.ofdft_cgm_start(self._h, C.c_void_p(phi.data_ptr()), C.c_void_p(bs.data_ptr()), self.n if stride is None else stride,
                                        bs.shape[0] if ncols is None else ncols, float(rtol), int(maxiter), self.info, self._stream())

    def step_rc(self, phi, pq, phiq):
        run = C.c_int(-1)
        a, b = (C.c_double * len(pq))(*pq), (C.c_double * len(phiq))(*phiq)
        return self.lib.ofdft_cgm_step(self._h, C.c_void_p(phi.data_ptr()), a, b, C.byref(run), self._stream()), run.value

    def direction_rc(self, phi):
        run = C.c_int(-1)
        return self.lib.ofdft_cgm_direction(self._h, C.c_void_p(phi.data_ptr()), self.dinfo, C.byref(run), self._stream()), run.value

    def status(self, j):
        it, reason, rel = C.c_int(-1), C.c_int(-1), C.c_double(-1.0)
        assert self.lib.ofdft_cgm_status(self._h, j, C.byref(it), C.byref(reason), C.byref(rel)) == N.OK
        return it.value, reason.value, rel.value

    def solution(self, B):
        out = torch.full((B, self.n), float('nan'), dtype=torch.double, device=DEV)
        assert self.lib.ofdft_cgm_solution(self._h, C.c_void_p(out.data_ptr()), self.n, self._stream()) == N.OK, self.err()
        return out

    def close(self):
        if self._h:
            self.full = self.x = self.r = self.p = self.q = self.z = None
            self.lib.ofdft_cgm_destroy(self._h)
            self._h = C.c_void_p(0)


@pytest.fixture
def mmake():
    made = []

    def factory(*args):
        made.append(MSolver(*args))
        return made[-1]
    yield factory
    for s in made:
        s.close()


def column_inputs(n, B):
    """phi and, per column, b, h, m of the made-up diagonal problems"""
    phi = T.diag_inputs(n, seed=0)[0]
    cols = [T.diag_inputs(n, seed=10 + j)[1:] + (P.diag_precond(n, seed=10 + j),) for j in range(B)]
    return phi, np.stack([c[0] for c in cols]), np.stack([c[1] for c in cols]), np.stack([c[2] for c in cols])


ITERATIONS = 3


@pytest.mark.parametrize('pre', [False, True], ids=['plain', 'preconditioned'])
@pytest.mark.parametrize('B', [3, 8])
@pytest.mark.parametrize('n', [1, 2, 255, 257, 262145])
def test_sweeps_match_the_numpy_statement_per_column(mmake, n, B, pre):
    """ofdft_cgm_start, then three times ([z_j = r_j / m_j, ofdft_cgm_direction,] q_j = h_j p_j, ofdft_cgm_step) on B columns of
    a handle built for 8: every column's x, r, p elementwise and its sums against the solo numpy backend seeded with the device's
    state in front of the sweep.  The vectors are NaN beforehand, the unused columns and the padding stay NaN."""
    phi, bs, hs, ms = column_inputs(n, B)
    tphi, tbs, ths, tms = dev(phi), dev(bs), dev(hs), dev(ms)
    s = mmake(n, 8)
    s.set_pre(pre)
    assert s.start_rc(tphi, tbs, 0.0, 1 << 20) == N.OK, s.err()
    worst_e = worst_s = 0.0
    st = []
    for j in range(B):
        ref = P.DiagPcgBackend(hs[j], ms[j]) if pre else T.DiagCgBackend(hs[j])
        ref.start(phi, bs[j], 0.0, 1 << 20)
        x, r, p = host(s.x[j]), host(s.r[j]), host(s.p[j])
        rr0, Sd, phib = s.info[3 * j], s.info[3 * j + 1], s.info[3 * j + 2]
        worst_e = max(worst_e, ratio(r, ref.r, np.abs(bs[j]) + np.abs(ref.r - bs[j])) / EPS)
        worst_s = max(worst_s, sum_dev(rr0, r * r), sum_dev(Sd, phi * phi), sum_dev(phib, phi * bs[j]))
        assert not x.any() and np.array_equal(p, r)
        it, reason, rel = s.status(j)
        assert (it, reason) == (0, N.CG_RUNNING if rr0 > 0.0 else N.CG_CONVERGED)
        st.append(dict(ref=ref, x=x, r=r, p=p, rr0=rr0, rr=rr0, S=Sd, rho=0.0, phir=0.0, reason=reason, steps=0))
    for k in range(ITERATIONS):
        run = [j for j in range(B) if st[j]['reason'] == N.CG_RUNNING]
        if not run:
            break
        frozen = {j: (s.x[j].clone(), s.r[j].clone()) for j in range(B) if j not in run}
        if pre:
            s.z[:B].copy_(s.r[:B] / tms)
            rc, _running = s.direction_rc(tphi)
            assert rc == N.OK, s.err()
            for j in run:
                c = st[j]
                z = host(s.z[j])
                rz, phiz, rho1, beta = s.dinfo[4 * j:4 * j + 4]
                worst_s = max(worst_s, sum_dev(rz, c['r'] * z), sum_dev(phiz, phi * z),
                              sum_dev(rho1, np.concatenate([c['r'] * z, [-c['phir'] * fsum(phi * z) / c['S']]])))
                c['reason'] = s.status(j)[1]
                if c['reason'] != N.CG_RUNNING:          # (n = 1: nothing is left of r in the complement of phi)
                    assert c['reason'] == N.CG_CURVATURE and not rho1 > 0.0 and np.array_equal(host(s.p[j]), c['p'], equal_nan=True)
                    continue
                assert beta == (0.0 if k == 0 else rho1 / c['rho'])
                c['ref'].seed_pre(c['x'], c['r'], c['p'], None, z, c['S'], c['rr0'], c['rr'], c['steps'], c['rho'], c['phir'], k == 0, False)
                c['ref'].direction_sweeps(phi)
                p1 = host(s.p[j])
                mag = np.abs(z) + np.abs(phiz / c['S'] * phi) + (np.abs(beta * c['p']) if k else 0.0)
                worst_e = max(worst_e, ratio(p1, c['ref'].p, mag) / EPS)
                c.update(p=p1, rho_new=rho1, z=z)
            run = [j for j in run if st[j]['reason'] == N.CG_RUNNING]
            if not run:
                break
        s.q[:B].copy_(ths * s.p[:B])
        pq, phiq = [float('nan')] * B, [float('nan')] * B
        for j in run:
            st[j]['q'] = host(s.q[j])
            pq[j], phiq[j] = float(np.dot(st[j]['p'], st[j]['q'])), float(np.dot(phi, st[j]['q']))
        rc, _running = s.step_rc(tphi, pq, phiq)
        assert rc == N.OK, s.err()
        for j in run:
            c = st[j]
            it, reason, rel = s.status(j)
            x1, r1, p1 = host(s.x[j]), host(s.r[j]), host(s.p[j])
            if not pq[j] > 0.0:                      # (n = 1: the direction may vanish altogether)
                assert n == 1 and reason == N.CG_CURVATURE
                c['reason'] = reason
                continue
            c['steps'] += 1
            assert it == c['steps']
            if pre:
                assert np.array_equal(p1, c['p'])                   # no direction sweep inside the step
                c['ref'].seed_pre(c['x'], c['r'], c['p'], c['q'], c['z'], c['S'], c['rr0'], c['rr'], c['steps'] - 1, c['rho_new'], c['phir'],
                                  False, True, maxiter=1 << 30)
                alpha = c['rho_new'] / pq[j]
            else:
                c['ref'].seed(c['x'], c['r'], c['p'], c['q'], c['S'], c['rr0'], c['rr'], c['steps'] - 1, maxiter=c['steps'])
                alpha = c['rr'] / pq[j]
            c['ref'].step(phi, pq[j], phiq[j])
            su = phiq[j] / c['S']
            worst_e = max(worst_e, ratio(x1, c['ref'].x, np.abs(c['x']) + np.abs(alpha * c['p'])) / EPS)
            worst_e = max(worst_e, ratio(r1, c['ref'].r, np.abs(c['r']) + np.abs(alpha * c['q']) + np.abs(alpha * su * phi)) / EPS)
            rr1 = rel * rel * c['rr0']
            worst_s = max(worst_s, sum_dev(rr1, r1 * r1))
            if not pre and reason == N.CG_RUNNING:
                c['ref'].seed(x1, r1, c['p'], c['q'], c['S'], c['rr0'], rr1, c['steps'])
                c['ref'].direction(phi, c['rr'])
                beta, sd = rr1 / c['rr'], float((phi * r1).sum()) / c['S']
                worst_e = max(worst_e, ratio(p1, c['ref'].p, np.abs(r1) + np.abs(sd * phi) + np.abs(beta * c['p'])) / EPS)
            c.update(x=x1, r=r1, p=p1, rr=rr1, reason=reason, phir=fsum(phi * r1))
            if pre:
                c['rho'] = c['rho_new']
        for j, (fx, fr) in frozen.items():
            assert torch.equal(s.x[j], fx, ) and torch.equal(s.r[j], fr)
    assert n <= 2 or all(c['steps'] == ITERATIONS for c in st)
    sol = s.solution(B)
    assert torch.equal(sol, s.x[:B])
    for v in s.full[:4]:                               # the columns nobody started and the padding are untouched
        assert bool(torch.isnan(v[B:]).all()) and bool(torch.isnan(v[:, n:]).all())
    print('MEASURE multi sweeps %s n=%d B=%d: elementwise %.2f eps of the terms (bound %g), sums %.2f eps of sum|terms| (bound %g)'
          % ('pcg' if pre else 'cg', n, B, worst_e, S.ELEMENT_BOUND, worst_s, S.SUMS_BOUND[N.F64]))
    assert worst_e <= S.ELEMENT_BOUND and worst_s <= S.SUMS_BOUND[N.F64]


class MDiag:
    """HipCgMultiBackend's methods on an MSolver around the diagonal operators; records that ended columns stay as they ended"""

    def __init__(self, s, ths, tms, pre):
        self.s, self.ths, self.tms, self.preconditioned = s, ths, tms, pre
        self.dV, self.ended = 1.0, {}

    def _freeze_check(self):
        for j in range(self.B):
            if self.s.status(j)[1] != N.CG_RUNNING:
                now = (self.s.x[j].clone(), self.s.r[j].clone(), self.s.status(j))
                if j in self.ended:
                    assert torch.equal(now[0], self.ended[j][0]) and torch.equal(now[1], self.ended[j][1]) and now[2] == self.ended[j][2]
                self.ended[j] = now

    def _reasons(self):
        self._freeze_check()
        return [self.s.status(j)[1] for j in range(self.B)]

    def start(self, phi, bs, rtol, maxiter):
        self.B = bs.shape[0]
        self.s.set_pre(self.preconditioned)
        assert self.s.start_rc(phi, bs, rtol, maxiter) == N.OK, self.s.err()

    def pre_direction(self, phi, n_elec):
        self.s.z[:self.B].copy_(self.s.r[:self.B] / self.tms)
        rc, _run = self.s.direction_rc(phi)
        assert rc == N.OK, self.s.err()
        return self._reasons()

    def product(self, phi, n_elec, reuse):
        self.s.q[:self.B].copy_(self.ths * self.s.p[:self.B])
        return ([float(torch.dot(self.s.p[j], self.s.q[j])) for j in range(self.B)],
                [float(torch.dot(phi, self.s.q[j])) for j in range(self.B)])

    def step(self, phi, pq, phiq):
        rc, _run = self.s.step_rc(phi, pq, phiq)
        assert rc == N.OK, self.s.err()
        return self._reasons()

    def status(self):
        return [self.s.status(j) for j in range(self.B)]

    def solution(self):
        return self.s.solution(self.B)


@pytest.mark.parametrize('pre', [False, True], ids=['plain', 'preconditioned'])
@pytest.mark.parametrize('n', [48, 257])
def test_the_four_endings_inside_one_batch(mmake, n, pre):
    """the five columns of tests/test_response_multi_cpu.exits_problem in one batch: every column's reason and iteration count are
    the solo numpy solve's, an ended column's x, r, reason and count are bitwise unchanged by every later sweep, the curvature
    column's x is its first direction"""
    phi, bs, hs, ms = MC.exits_problem(n)
    tphi, tbs = dev(phi), dev(bs)
    b = MDiag(mmake(n, 5), dev(np.stack(hs)), dev(np.stack(ms)), pre)
    x, iters, reasons, rels, nprod = optimize.solve_projected_multi(b, tphi, tbs, 1.0, 1e-10, MC.MAXITER)
    solo = [optimize.solve_projected(P.DiagPcgBackend(hs[j], ms[j]) if pre else T.DiagCgBackend(hs[j]), phi, None, bs[j], 1.0, 1e-10, MC.MAXITER)
            for j in range(5)]
    apart = [float(np.abs(host(x[j]) - solo[j][0]).max() / max(np.abs(solo[j][0]).max(), 1e-300)) for j in range(5)]
    print('MEASURE multi endings %s n=%d: iterations %s reasons %s (numpy %s %s) products %d max|x - numpy|/max|x| %s'
          % ('pcg' if pre else 'cg', n, iters, reasons, [s_[1] for s_ in solo], [s_[2] for s_ in solo], nprod, ['%.1e' % a for a in apart]))
    assert iters == [s_[1] for s_ in solo] and reasons == [s_[2] for s_ in solo]
    assert sorted(set(reasons)) == [N.CG_CONVERGED, N.CG_MAXITER, N.CG_CURVATURE] and nprod == MC.MAXITER
    assert not bool(x[0].any()) and rels[0] == 0.0
    assert len(b.ended) == 5
    assert max(apart[j] for j in (1, 2, 4)) <= 1e-9          # (converged to rtol 1e-10, or the first direction itself)


def test_solver_states_and_limits(mmake):
    n = 257
    phi, bs, hs, ms = column_inputs(n, 3)
    tphi, tbs = dev(phi), dev(bs)
    s = mmake(n, 3)
    rc, _run = s.step_rc(tphi, [1.0] * 3, [0.0] * 3)
    print('MEASURE multi solver states: step before start -> %d (%s)' % (rc, s.err()))
    assert rc == N.ESTATE and 'ofdft_cgm_start has not been called' in s.err()
    rc = s.start_rc(tphi, tbs, 0.0, 10, ncols=4)
    print('MEASURE multi solver states: four columns on a handle for three -> %d (%s)' % (rc, s.err()))
    assert rc == N.EINVAL and '1 .. 3' in s.err() and 'OFDFT_MULTI_MAX = 8' in s.err()
    assert s.start_rc(tphi, tbs, 0.0, 10, ncols=0) == N.EINVAL
    assert s.start_rc(tphi, tbs, 0.0, 10, stride=n - 1) == N.EINVAL and 'b_stride' in s.err()
    assert s.start_rc(tphi, tbs, 0.0, 10) == N.OK
    rc, _run = s.direction_rc(tphi)
    assert rc == N.ESTATE and 'plain mode' in s.err()
    s.set_pre(1)
    assert s.start_rc(tphi, tbs, 0.0, 10) == N.OK
    rc, _run = s.step_rc(tphi, [1.0] * 3, [0.0] * 3)
    assert rc == N.ESTATE and 'ofdft_cgm_direction has not formed' in s.err()
    s.z[:3].copy_(s.r[:3] / dev(ms))
    rc, run = s.direction_rc(tphi)
    assert (rc, run) == (N.OK, 3)
    rc, _run = s.direction_rc(tphi)
    assert rc == N.ESTATE and 'already formed' in s.err()
    rc, run = s.step_rc(tphi, [-1.0, float('nan'), 0.0], [0.0] * 3)          # every column ends on curvature: x_j = p_j
    assert (rc, run) == (N.OK, 0) and torch.equal(s.x[:3], s.p[:3])
    rc, _run = s.step_rc(tphi, [1.0] * 3, [0.0] * 3)
    assert rc == N.ESTATE and 'every column has ended' in s.err()
    assert s.start_rc(tphi, torch.zeros_like(tbs), 1e-12, 10) == N.OK
    assert [s.status(j) for j in range(3)] == [(0, N.CG_CONVERGED, 0.0)] * 3


# ------------------------------------------------------------------------------- 6: the golden response
@pytest.mark.parametrize('pre', [None, 'auto'], ids=['plain', 'preconditioned'])
def test_golden_response_in_three_columns(pre):
    """density_response_multi on tn_g16r at rtol 1e-12 with three columns: the golden's dv against tests/golden/tn_g16r.npz within
    the bounds of the solo solve; dv = 0, which gives dn = 0 exactly in 0 iterations; a seeded dv against the numpy double.  Each
    column's iteration count is within 1 of the solo device solve's."""
    g = np.load(os.path.join(GOLDEN, 'tn_g16r.npz'))
    box, phi, _d, _vext, n_elec = tn_cases.make_inputs('g16r')
    dv = tn_cases.response_dv(phi.shape)
    seeded = 0.05 * hvp_cases.direction(phi.shape, seed=411)
    ref = optimize.density_response(None, g['chi_gs'], n_elec, seeded, rtol=1e-12, maxiter=500,
                                    backend=P.PcgBackend(box, phi.shape, TERMS) if pre else T.NumpyCgBackend(box, phi.shape, TERMS))
    eng = Engine(phi.shape, DEV).set_cell(box).set_terms(TERMS)
    chi = dev(g['chi_gs'])
    dvs = dev(np.stack([dv, np.zeros_like(dv), seeded]))
    r = optimize.density_response_multi(eng, chi, n_elec, dvs, rtol=1e-12, maxiter=500, precondition=pre)
    solo = [optimize.density_response(eng, chi, n_elec, dvs[j].clone(), rtol=1e-12, maxiter=500, precondition=pre) for j in (0, 2)]
    eng.close()
    dn = r['dn'].cpu().numpy()
    ddn = float(np.abs(dn[0] - g['dn']).max() / np.abs(g['dn']).max())
    dmu = abs(r['dmu'][0] - float(g['dmu'])) / abs(float(g['dmu']))
    ddn2 = float(np.abs(dn[2] - ref['dn']).max() / np.abs(ref['dn']).max())
    dmu2 = abs(r['dmu'][2] - ref['dmu']) / abs(ref['dmu'])
    dsolo = [float((r['dn'][j] - s_['dn']).abs().max() / s_['dn'].abs().max()) for j, s_ in zip((0, 2), solo)]
    print('MEASURE multi response g16r %s: golden dn %.2e dmu %.2e; seeded against numpy dn %.2e dmu %.2e; against the solo device solve %s; '
          'iterations %s (solo %s, numpy %d) products %d residuals %s'
          % (pre, ddn, dmu, ddn2, dmu2, ['%.1e' % x for x in dsolo], r['iterations'], [s_['iterations'] for s_ in solo], ref['iterations'],
             r['hvp_count'], ['%.1e' % x for x in r['rel_residual']]))
    assert r['reason'] == [optimize.CG_CONVERGED] * 3 and max(r['rel_residual']) <= 1e-12
    assert ddn <= PG.DN_BOUND and dmu <= PG.DMU_BOUND
    assert ddn2 <= PG.DN_BOUND and dmu2 <= PG.DMU_BOUND
    assert r['iterations'][1] == 0 and not dn[1].any() and r['dmu'][1] == 0.0 and r['rel_residual'][1] == 0.0
    for j, s_ in zip((0, 2), solo):
        assert abs(r['iterations'][j] - s_['iterations']) <= 1
    assert r['hvp_count'] == max(r['iterations'])
    assert abs(dn[0].sum()) <= 64 * EPS * np.abs(dn[0]).sum()


# ------------------------------------------------------------------------------- 7: end to end
def same_shape(a, b):
    return all(len(a[k]) == len(b[k]) for k in ('iterations', 'rel_residual', 'reason'))


def test_force_constants_in_batches():
    """force_constants(primitive_ion_indices=[1, 2]) at rtol 1e-11 with batch 3, batch 8 (six columns across the two ions in one
    solve) and batch 3 with precondition='auto', against the numpy-driven matrix within SOLVE_BOUND and against batch=None"""
    box, shape, frac, tab, _z = PG.a16()
    s = PG.run()
    chi, eng = s['plain']['chi'], s['eng']
    kw = dict(primitive_ion_indices=[1, 2], rtol=PG.FC_RTOL)
    plain = force_constants(eng, box, [(frac, tab)], chi, **kw)
    ref = force_constants(None, box, [(frac, tab)], chi.cpu().numpy(), backend=FD.NumpyFcBackend(box, shape, [(frac, tab)], TERMS), **kw)
    scale = float(np.abs(ref['phi']).max())
    for batch, pre in ((3, None), (8, None), (3, 'auto')):
        r = force_constants(eng, box, [(frac, tab)], chi, batch=batch, precondition=pre, **kw)
        d, dp = float(np.abs(r['phi'] - ref['phi']).max() / scale), float(np.abs(r['phi'] - plain['phi']).max() / scale)
        print('MEASURE multi fc a16 rows 1, 2 batch %d %s: Phi - numpy %.2e  Phi - unbatched %.2e of max|Phi| %.4e  iterations %s (unbatched %s) '
              'products %d (unbatched %d)' % (batch, pre, d, dp, scale, r['iterations'], plain['iterations'], r['hvp_count'], plain['hvp_count']))
        assert all(x == optimize.CG_CONVERGED for x in r['reason']) and max(r['rel_residual']) <= PG.FC_RTOL
        assert d <= PG.FC_SOLVE_BOUND and dp <= PG.FC_SOLVE_BOUND
        assert same_shape(r, plain) and r['phi'].shape == plain['phi'].shape and abs(r['asr_residual'] - plain['asr_residual']) <= PG.FC_SOLVE_BOUND
        for k in ('ion_ion', 'direct'):                           # the parts without a solve do not see the option
            assert np.array_equal(r['parts'][k], plain['parts'][k])
        assert set(r['parts']) == set(plain['parts'])
        if pre is None:
            assert all(abs(a - b) <= 1 for a, b in zip(r['iterations'], plain['iterations']))
            assert r['hvp_count'] < plain['hvp_count']


def test_elastic_constants_and_bulk_modulus_in_batches():
    """elastic_constants(batch=6) and bulk_modulus(batch=6) at rtol 1e-11, plain and once with precondition='auto', against the
    numpy-driven run within SOLVE_BOUND and against batch=None"""
    box, shape, frac, tab, _z = PG.a16()
    s = PG.run()
    chi, eng = s['plain']['chi'], s['eng']
    plain = elastic.elastic_constants(eng, box, [(frac, tab)], chi, rtol=PG.EL_RTOL)
    ref = elastic.elastic_constants(None, box, [(frac, tab)], chi.cpu().numpy(), rtol=PG.EL_RTOL,
                                    backend=ED.NumpyElasticBackend(box, shape, [(frac, tab)], TERMS))
    for pre in (None, 'auto'):
        r = elastic.elastic_constants(eng, box, [(frac, tab)], chi, rtol=PG.EL_RTOL, batch=6, precondition=pre)
        K = elastic.bulk_modulus(eng, box, [(frac, tab)], chi, rtol=PG.EL_RTOL, batch=6, precondition=pre)
        dK = abs(K - ref['bulk_modulus']) / abs(ref['bulk_modulus'])
        dC = float(np.abs(r['C'] - ref['C']).max() / np.abs(ref['C']).max())
        dP = float(np.abs(r['C'] - plain['C']).max() / np.abs(plain['C']).max())
        print('MEASURE multi elastic a16 batch 6 %s: K - numpy %.2e  C - numpy %.2e  C - unbatched %.2e  iterations %s (unbatched %s) products %d (unbatched %d)'
              % (pre, dK, dC, dP, r['iterations'], plain['iterations'], r['hvp_count'], plain['hvp_count']))
        assert K == r['bulk_modulus']
        assert all(x == optimize.CG_CONVERGED for x in r['reason']) and max(r['rel_residual']) <= PG.EL_RTOL
        assert dK <= PG.EL_SOLVE_BOUND and dC <= PG.EL_SOLVE_BOUND and dP <= PG.EL_SOLVE_BOUND
        assert same_shape(r, plain) and set(r['parts']) == set(plain['parts'])
        assert r['hvp_count'] == max(r['iterations'])


# ------------------------------------------------------------------------------- 8: refusals
def test_refusals_by_name():
    from professad_amd.distributed import DistEngine
    box, phi, n_elec, dirs, _ref = product_reference('g16r', 'wt')
    shape = phi.shape
    eng = Engine(shape, DEV).set_cell(box).set_terms(TERMS)
    tphi = dev(phi)
    lib, npts = eng.lib, phi.size

    def raw(ncols, dstride=npts, ostride=npts, out=None, reuse=0):
        big = torch.zeros((9,) + shape, dtype=torch.double, device=DEV)
        o = torch.empty_like(big) if out is None else out(big)
        rc = lib.ofdft_hessian_vector_chi_multi(eng._ctx, C.c_void_p(tphi.data_ptr()), C.c_void_p(big.data_ptr()), dstride, ncols, n_elec,
                                                C.c_void_p(o.data_ptr()), ostride, None, reuse, eng._stream())
        return rc, lib.ofdft_last_error(eng._ctx).decode()
    for B in (0, 9):
        rc, msg = raw(B)
        print('MEASURE multi refusals: ncols = %d -> %d (%s)' % (B, rc, msg))
        assert rc == N.EINVAL and '1 .. 8' in msg and 'OFDFT_MULTI_MAX' in msg
        with pytest.raises(ValueError, match='1 .. 8'):
            eng.hessian_vector_chi_multi(tphi, torch.zeros((B,) + shape, dtype=torch.double, device=DEV), n_elec)
        with pytest.raises(ValueError, match='1 .. 8'):
            eng.precondition_multi(torch.zeros((B,) + shape, dtype=torch.double, device=DEV), 1.0)
        with pytest.raises(ValueError, match='1 .. 8'):
            optimize.HipCgMultiBackend(eng, B)
        big = torch.zeros((9,) + shape, dtype=torch.double, device=DEV)
        rc = lib.ofdft_precondition_multi(eng._ctx, C.c_void_p(big.data_ptr()), npts, C.c_void_p(torch.empty_like(big).data_ptr()), npts, B, 1.0,
                                          eng._stream())
        assert rc == N.EINVAL and '1 .. 8' in lib.ofdft_last_error(eng._ctx).decode()
    rc, msg = raw(3, dstride=npts - 1)
    assert rc == N.EINVAL and 'stride' in msg
    rc, msg = raw(3, ostride=npts - 1)
    assert rc == N.EINVAL and 'stride' in msg
    rc, msg = raw(3, out=lambda big: big[2])              # the third column of the input stack
    assert rc == N.EINVAL and 'overlaps' in msg
    rc, msg = raw(3, reuse=1)
    assert rc == N.ESTATE and 'reuse_density = 1' in msg
    stack = dev(dirs[:3])
    with pytest.raises(ValueError, match='aliases'):
        eng.hessian_vector_chi_multi(tphi, stack, n_elec, out=stack)
    with pytest.raises(ValueError, match='aliases'):
        eng.precondition_multi(stack, 1.0, out=stack)
    for bad in (stack.float(), stack.cpu(), stack.transpose(1, 2), stack[0]):
        with pytest.raises(ValueError):
            eng.hessian_vector_chi_multi(tphi, bad, n_elec)
    with pytest.raises(ValueError, match='kappa2'):
        eng.precondition_multi(stack, 0.0)
    eng.set_terms(TERMS, dict(wts_kind=1))
    with pytest.raises(NotImplementedError, match='wts_kind'):
        eng.hessian_vector_chi_multi(tphi, stack, n_elec)
    rc, msg = raw(3)
    assert rc == N.EINVAL and 'wts_kind' in msg
    for names, word in ((('pbe_x', 'pbe_c'), 'pbe_x'), (('tf', 'vw', 'wgc99_nl'), 'wgc99_nl')):
        eng.set_terms(list(names))
        with pytest.raises(NotImplementedError, match=word):
            eng.hessian_vector_chi_multi(tphi, stack, n_elec)
        with pytest.raises(NotImplementedError, match=word):
            optimize.density_response_multi(eng, tphi, n_elec, stack)
        rc, msg = raw(3)
        assert rc == N.EINVAL and word in msg
    eng.close()
    e32 = Engine(shape, DEV, dtype=torch.float32).set_cell(box).set_terms(['tf'])
    with pytest.raises(NotImplementedError, match='fp64'):
        e32.hessian_vector_chi_multi(tphi.float(), stack.float(), n_elec)
    with pytest.raises(NotImplementedError, match='fp64'):
        e32.precondition_multi(stack.float(), 1.0)
    with pytest.raises(NotImplementedError, match='fp64'):
        optimize.HipCgMultiBackend(e32, 3)
    rc = e32.lib.ofdft_hessian_vector_chi_multi(e32._ctx, C.c_void_p(tphi.data_ptr()), C.c_void_p(stack.data_ptr()), npts, 3, n_elec,
                                                C.c_void_p(torch.empty_like(stack).data_ptr()), npts, None, 0, e32._stream())
    assert rc == N.EINVAL and 'fp64 library' in e32.lib.ofdft_last_error(e32._ctx).decode()
    e32.close()
    de = DistEngine(shape, DEV).set_cell(torch.as_tensor(box)).set_terms(['ion_electron', 'tf'])
    with pytest.raises(NotImplementedError, match='single-GPU'):
        de.hessian_vector_chi_multi(tphi, stack, n_elec)
    with pytest.raises(NotImplementedError, match='single-GPU'):
        de.precondition_multi(stack, 1.0)
    with pytest.raises(NotImplementedError, match='single-GPU'):
        optimize.density_response_multi(de, tphi, n_elec, stack)
    de.close()
