"""Batched response solves without a device: optimize.solve_projected_multi on the numpy multi backend of
tests/multi_double.py against optimize.solve_projected on the same solo backends, the `batch` grouping of force_constants and
elastic_constants on the numpy doubles against `batch=None`, and the argument refusals that need no device.  Every test prints its
figures as `MEASURE ...` before it asserts.

Bounds.  A column of the multi double is one solo backend driven by the same calls in the same order, so 1. asks for equality.
The drivers with `batch` run the same numpy arithmetic per column as without (the columns of the double share nothing), so 2. asks
for equality too, which is "the doubles' own rounding" at its sharpest.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (the oracle closure)

from professad_amd import _native as N
from professad_amd import elastic, optimize, synth
from professad_amd.force_constants import force_constants

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import elastic_cases as EC  # noqa: E402
import elastic_double as ED  # noqa: E402
import fc_double as FD  # noqa: E402
import multi_double as M  # noqa: E402
import pcg_double as P  # noqa: E402
import tn_cases  # noqa: E402
import tn_double as T  # noqa: E402
from oracle import ions as O  # noqa: E402

TERMS = list(tn_cases.TERMS)
NAMES = ('zero', 'eigen', 'curvature', 'capped', 'easy')
MAXITER = 5


def exits_problem(n=48):
    """phi, the right-hand sides and the diagonal operators / preconditioners of five columns that end at different iterations for
    all four reasons within MAXITER: b = 0 (converged at 0); b an eigenvector of P H P -- supported where phi is zero and h, m are
    constant -- (converged at 1); a negative diagonal (curvature at once); a spread diagonal (capped by maxiter); h within 1e-3 of
    a constant (converged before the cap)"""
    phi, b, h = T.diag_inputs(n, seed=3)
    m = P.diag_precond(n, seed=3)
    half = n // 2
    phi = phi.copy()
    phi[half:] = 0.0
    bs, hs, ms = [], [], []
    bs.append(np.zeros(n)), hs.append(h), ms.append(m)                                          # zero
    e = np.zeros(n)
    e[half:] = b[half:]
    he, me = h.copy(), m.copy()
    he[half:], me[half:] = 2.0, 3.0
    bs.append(e), hs.append(he), ms.append(me)                                                  # eigen
    bs.append(b), hs.append(-h), ms.append(m)                                                   # curvature
    bs.append(b), hs.append(h * np.linspace(1.0, 400.0, n)), ms.append(m)                       # capped
    bs.append(b[::-1].copy()), hs.append(1.0 + 1e-3 * h), ms.append(np.ones(n))                 # easy
    return phi, np.stack(bs), hs, ms


@pytest.mark.parametrize('pre', [False, True], ids=['plain', 'preconditioned'])
def test_each_column_is_the_solo_solve(pre):
    phi, bs, hs, ms = exits_problem()

    def make(j):
        return P.DiagPcgBackend(hs[j], ms[j]) if pre else T.DiagCgBackend(hs[j])
    multi = M.MultiCgDouble(make)
    x, iters, reasons, rels, nprod = optimize.solve_projected_multi(multi, phi, bs, 1.0, 1e-10, MAXITER)
    solo = [optimize.solve_projected(make(j), phi, None, bs[j], 1.0, 1e-10, MAXITER) for j in range(len(bs))]
    for j, nm in enumerate(NAMES):
        print('MEASURE multi cpu %s %-9s: iterations %d (solo %d) reason %d (solo %d) |r|/|b| %.3e products %d (solo %d) max|dx| %.1e'
              % ('pcg' if pre else 'cg', nm, iters[j], solo[j][1], reasons[j], solo[j][2], rels[j], nprod, solo[j][4],
                 np.abs(x[j] - solo[j][0]).max()))
    for j in range(len(bs)):
        assert np.array_equal(x[j], solo[j][0])
        assert (iters[j], reasons[j], rels[j]) == solo[j][1:4]
    assert nprod == max(s[4] for s in solo) == multi.products
    want = dict(zero=(0, optimize.CG_CONVERGED), eigen=(1, optimize.CG_CONVERGED), curvature=(0, optimize.CG_CURVATURE),
                capped=(MAXITER, optimize.CG_MAXITER))
    for j, nm in enumerate(NAMES[:4]):
        assert (iters[j], reasons[j]) == want[nm], nm
    assert reasons[4] == optimize.CG_CONVERGED and 1 < iters[4] < MAXITER
    assert not x[0].any()


def relax(backend, chi, n_elec, steps):
    tn = optimize.TruncatedNewton(chi, backend.cg, n_elec)
    for _outer in range(steps):
        before = tn.total_iter
        tn.step(lambda: backend.closure(chi, n_elec))
        if tn.total_iter == before:
            break


def small_cell(nions):
    """Al ions in the triclinic cell of 203 bohr^3 on a 6 x 8 x 6 grid (the cell of tests/test_elastic_cpu.py), the seven-term set"""
    shape = (6, 8, 6)
    box = synth.triclinic_cell(0.75)
    tab = O.recpot_table(*EC.recpot())
    frac = np.array([[0.1, 0.2, 0.15], [0.6, 0.55, 0.7], [0.35, 0.8, 0.4], [0.85, 0.3, 0.9]])[:nions]
    n_elec = nions * float(tab[2])
    chi = np.full(shape, np.sqrt(n_elec / abs(np.linalg.det(box))))
    return box, shape, [(frac, tab)], n_elec, chi


def same_log(a, b):
    return a['iterations'] == b['iterations'] and a['reason'] == b['reason'] and a['rel_residual'] == b['rel_residual']


def test_force_constants_batch_groups_the_same_solves():
    """four ions: 3 P = 12 right-hand sides; batch 8 (groups of 8 + 4, across ions), 3 and 1 against batch=None"""
    box, shape, species, n_elec, chi = small_cell(4)
    b = FD.NumpyFcBackend(box, shape, species, TERMS)
    relax(b, chi, n_elec, 14)
    ref = force_constants(None, box, species, chi, backend=b, rtol=1e-11)
    assert len(ref['iterations']) == 12
    for batch in (8, 3, 1):
        bb = M.with_batch(FD.NumpyFcBackend(box, shape, species, TERMS), batch, lambda j: T.NumpyCgBackend(box, shape, TERMS))
        r = force_constants(None, box, species, chi, backend=bb, rtol=1e-11)
        dev = float(np.abs(r['phi'] - ref['phi']).max() / np.abs(ref['phi']).max())
        print('MEASURE multi cpu force_constants batch %d: max|dPhi|/max|Phi| %.2e iterations %s (unbatched %s) products %d (unbatched %d)'
              % (batch, dev, r['iterations'], ref['iterations'], r['hvp_count'], ref['hvp_count']))
        assert np.array_equal(r['phi'], ref['phi']) and same_log(r, ref)
        for k in ref['parts']:
            assert np.array_equal(r['parts'][k], ref['parts'][k])
        assert r['asr_residual'] == ref['asr_residual']
        groups = [ref['iterations'][j0:j0 + batch] for j0 in range(0, 12, batch)]
        assert r['hvp_count'] == sum(max(g) for g in groups)
    sub = force_constants(None, box, species, chi, primitive_ion_indices=[2, 0],
                          backend=M.with_batch(FD.NumpyFcBackend(box, shape, species, TERMS), 4, lambda j: T.NumpyCgBackend(box, shape, TERMS)),
                          rtol=1e-11)
    assert np.array_equal(sub['phi'][0], ref['phi'][2]) and np.array_equal(sub['phi'][1], ref['phi'][0])
    assert sub['iterations'] == ref['iterations'][6:9] + ref['iterations'][0:3]


def test_elastic_constants_batch_groups_the_same_solves():
    """six right-hand sides; batch 4 (4 + 2) and 6 against batch=None, plain and preconditioned; bulk_modulus likewise"""
    box, shape, species, n_elec, chi = small_cell(2)
    for pre in (False, True):
        def solo():
            return P.PcgBackend(box, shape, TERMS) if pre else T.NumpyCgBackend(box, shape, TERMS)
        b = ED.NumpyElasticBackend(box, shape, species, TERMS)
        if not pre:
            relax(b, chi, n_elec, 14)
        b.cg = solo()
        ref = elastic.elastic_constants(None, box, species, chi, backend=b, rtol=1e-11)
        for batch in (4, 6):
            bb = M.with_batch(ED.NumpyElasticBackend(box, shape, species, TERMS), batch, lambda j: solo())
            r = elastic.elastic_constants(None, box, species, chi, backend=bb, rtol=1e-11)
            dev = float(np.abs(r['C'] - ref['C']).max() / np.abs(ref['C']).max())
            print('MEASURE multi cpu elastic_constants %s batch %d: max|dC|/max|C| %.2e iterations %s (unbatched %s) products %d (unbatched %d)'
                  % ('pcg' if pre else 'cg', batch, dev, r['iterations'], ref['iterations'], r['hvp_count'], ref['hvp_count']))
            assert np.array_equal(r['C'], ref['C']) and np.array_equal(r['W2'], ref['W2']) and same_log(r, ref)
            assert r['bulk_modulus'] == ref['bulk_modulus']
            assert r['hvp_count'] == sum(max(ref['iterations'][j0:j0 + batch]) for j0 in range(0, 6, batch))
        bb = M.with_batch(ED.NumpyElasticBackend(box, shape, species, TERMS), 6, lambda j: solo())
        assert elastic.bulk_modulus(None, box, species, chi, backend=bb, rtol=1e-11) == ref['bulk_modulus']


class _FakeEngine:
    def __init__(self, names, comm=None, dtype=torch.double):
        self.comm, self.dtype = comm, dtype
        mask = 0
        for nm in names:
            mask |= N.TERM_BITS[nm]
        self._terms_key = (mask, np.zeros(N.NPARAMS).tobytes())

    def _mask(self):
        return self._terms_key[0]


def test_arguments_are_refused_before_any_device_work():
    print('MEASURE multi cpu refusals: batch limit %d, bad values 0, 9, -1, 2.0, "3", True' % optimize.MULTI_MAX)
    for bad in (0, 9, -1, 2.0, '3', True):
        with pytest.raises(ValueError, match='batch'):
            optimize.check_batch(bad)
    assert optimize.check_batch(None) is None and optimize.check_batch(8) == 8 and optimize.check_batch(np.int64(3)) == 3
    assert optimize.MULTI_MAX == N.MULTI_MAX == 8
    sp = [(np.zeros((1, 3)), (None, None, 3))]
    for driver in (force_constants, elastic.elastic_constants, elastic.bulk_modulus):
        with pytest.raises(ValueError, match='backend'):          # the rule of `precondition`
            driver(None, np.eye(3), sp, None, backend=object(), batch=3)
        with pytest.raises(ValueError, match='batch'):
            driver(_FakeEngine(['ion_electron', 'tf']), np.eye(3), sp, None, batch=9)
        with pytest.raises(NotImplementedError, match='single-GPU'):
            driver(_FakeEngine(['ion_electron', 'tf'], comm=object()), np.eye(3), sp, None, batch=3)
        with pytest.raises(NotImplementedError, match='fp64'):
            driver(_FakeEngine(['ion_electron', 'tf'], dtype=torch.float32), np.eye(3), sp, None, batch=3)
        with pytest.raises(NotImplementedError, match='pbe_x'):
            driver(_FakeEngine(['ion_electron', 'tf', 'pbe_x']), np.eye(3), sp, None, batch=3)
    with pytest.raises(ValueError, match='backend'):
        optimize.density_response_multi(None, None, 8.0, [None], backend=object(), precondition='auto')
    for B in (0, 9):
        with pytest.raises(ValueError, match='1 .. 8'):
            optimize.density_response_multi(None, None, 8.0, [None] * B, backend=object())
    for make in (lambda e: optimize.HipCgMultiBackend(e, 3), lambda e: optimize.density_response_multi(e, None, 8.0, [None] * 3)):
        with pytest.raises(NotImplementedError, match='fp64'):
            make(_FakeEngine(['tf'], dtype=torch.float32))
        with pytest.raises(NotImplementedError, match='single-GPU'):
            make(_FakeEngine(['tf'], comm=object()))
        with pytest.raises(NotImplementedError, match='wgc99_nl'):
            make(_FakeEngine(['tf', 'vw', 'wgc99_nl']))
    from professad_amd.distributed import DistEngine
    for name in ('hessian_vector_chi_multi', 'precondition_multi'):
        with pytest.raises(NotImplementedError, match='single-GPU'):
            getattr(DistEngine, name)(None, None, None, 1.0)


@pytest.mark.parametrize('dtype', [N.F64, N.F32])
def test_entry_points_are_exported_and_refuse_null_handles_and_limits(dtype):
    lib = N.load(dtype)
    new = ['ofdft_hessian_vector_chi_multi', 'ofdft_precondition_multi'] + ['ofdft_cgm_' + s for s in (
        'create', 'destroy', 'last_error', 'vectors', 'z', 'set_preconditioned', 'start', 'step', 'direction', 'status', 'solution')]
    print('MEASURE multi cpu exports: %d new entries, %d in all' % (len(new), len(N.EXPORTS)))
    for sym in new:
        assert sym in N.EXPORTS and hasattr(lib, sym)
    assert lib.ofdft_hessian_vector_chi_multi(None, None, None, 8, 1, 1.0, None, 8, None, 0, None) == N.EINVAL
    assert lib.ofdft_precondition_multi(None, None, 8, None, 8, 1, 1.0, None) == N.EINVAL
    h, run, z = ctypes.c_void_p(0), ctypes.c_int(0), ctypes.c_void_p(0)
    for ncols_max in (0, 9):
        assert lib.ofdft_cgm_create(ctypes.byref(h), 8, ncols_max, 0) == N.EINVAL and not h.value
    assert lib.ofdft_cgm_create(None, 8, 3, 0) == N.EINVAL
    one = (ctypes.c_double * 1)()
    assert lib.ofdft_cgm_start(None, None, None, 8, 1, 0.0, 1, None, None) == N.EINVAL
    assert lib.ofdft_cgm_step(None, None, one, one, ctypes.byref(run), None) == N.EINVAL
    assert lib.ofdft_cgm_direction(None, None, None, ctypes.byref(run), None) == N.EINVAL
    assert lib.ofdft_cgm_z(None, ctypes.byref(z)) == N.EINVAL
    assert lib.ofdft_cgm_set_preconditioned(None, 1) == N.EINVAL
    assert lib.ofdft_cgm_status(None, 0, None, None, None) == N.EINVAL
    assert lib.ofdft_cgm_solution(None, None, 8, None) == N.EINVAL
    assert lib.ofdft_cgm_last_error(None) == b'null handle'
