"""Truncated Newton and the density response without a device: the chi-space product's closed form (tests/tn_double.py on
tests/hvp_double.py) against the reference's double autograd (tests/golden/tn_<case>.npz; generator make_golden_tn.py), the host
logic of optimize.TruncatedNewton / solve_projected / density_response driven by the numpy backend, and the entry points' error
paths.

Tolerance rule (that of tests/test_hvp_cpu.py): 10 x the largest deviation from the reference's golden measured with
numpy 2 / torch 2 on x86-64 (MEASURED; every test prints its figure before it asserts).  The ground-state energy takes the
bound the goldens' description sets instead: 1e-10 Ha.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from professad_amd import _native as N
from professad_amd import optimize

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import cases  # noqa: E402
import tn_cases  # noqa: E402
import tn_double as T  # noqa: E402
from oracle import refpath  # noqa: E402

# largest figures over the cases they cover (see each test's docstring)
MEASURED = dict(Hd=4.25e-14, dHd=8.66e-15, identity=1.16e-16, den_gs=5.86e-12, dn=2.64e-12, dmu=1.33e-10)
E_BOUND_HA = 1e-10
MAX_OUTER, MAX_PRODUCTS = 8, 200


def gold(case):
    g = np.load(os.path.join(HERE, 'golden', 'tn_%s.npz' % case))
    box, phi, d, vext, n_elec = tn_cases.make_inputs(case)
    assert cases.checksum(box, phi, d, vext) == pytest.approx(float(g['checksum']), rel=1e-12)       # generator drift
    return g, box, phi, d, vext, n_elec


def cpu_closure(box, vext, n_elec):
    """E[chi] and its gradient from the pinned oracle (oracle/refpath.py), numpy in and out"""
    tb, table = torch.as_tensor(box), refpath.term_table(torch.as_tensor(vext))
    fns = [table[k] for k in tn_cases.TERMS]

    def closure(chi):
        E, g = refpath.closure(tb, torch.as_tensor(chi), n_elec, fns)
        return float(E), g.numpy()
    return closure


@pytest.mark.parametrize('case', tn_cases.CASES)
def test_closed_form_matches_the_reference_double_autograd(case):
    """H d and d.H d of tn_double.hessian_vector_chi at phi = 1.7 sqrt(den) with the golden gradient, relative to max|H d|.
    Measured g16r / g17r / g18t: H d 8.1e-16 / 3.7e-14 / 4.3e-14, d.H d 1.2e-16 / 8.7e-15 / 7.9e-16; H phi = -g to 1.2e-16 of max|g|."""
    g, box, phi, d, _vext, n_elec = gold(case)
    s, Hd = T.hessian_vector_chi(box, phi, d, g['g'], n_elec, tn_cases.TERMS)
    dev = float(np.abs(Hd - g['Hd']).max() / np.abs(g['Hd']).max())
    ddev = abs(s['dHd'] - float(g['dHd'])) / abs(float(g['dHd']))
    _s, Hphi = T.hessian_vector_chi(box, phi, phi, g['g'], n_elec, tn_cases.TERMS)
    ident = float(np.abs(Hphi + g['g']).max() / np.abs(g['g']).max())
    print('MEASURE tn double %s: Hd %.2e dHd %.2e  H phi + g %.2e' % (case, dev, ddev, ident))
    assert dev <= 10 * MEASURED['Hd'] and ddev <= 10 * MEASURED['dHd'] and ident <= 10 * MEASURED['identity']
    assert s['a'] == pytest.approx(float((phi * d).sum()), rel=1e-14) and s['S'] == pytest.approx(float((phi * phi).sum()), rel=1e-14)
    assert abs(s['phiHd'] - float((phi * Hd).sum())) <= 1e-12 * np.abs(phi).max() * np.abs(Hd).sum()


@pytest.fixture(scope='module')
def ground_state():
    """TruncatedNewton from the uniform density on g16r: numpy backend, oracle closure; run once for the tests below"""
    g, box, phi, _d, vext, n_elec = gold('g16r')
    closure = cpu_closure(box, vext, n_elec)
    chi = np.full(phi.shape, np.sqrt(n_elec / abs(np.linalg.det(box))))
    backend = T.NumpyCgBackend(box, phi.shape, tn_cases.TERMS)
    tn = optimize.TruncatedNewton(chi, backend, n_elec)
    outer = 0
    while outer < 12:
        before = tn.total_iter
        tn.step(lambda: closure(chi))
        if tn.total_iter == before:          # |g|_2 <= tolerance_grad: the step did nothing
            break
        outer += 1
    return g, box, n_elec, chi, tn, backend


def test_truncated_newton_reaches_the_golden_ground_state(ground_state):
    """Energy within 1e-10 Ha of the reference run's, density within 10 x the measured 5.9e-12 of max n (measured E - E_gs: 1.6e-16 Ha;
    the run stops at |g|_2 <= 1e-10, the golden at 3e-12), inside the caps on outer iterations and products (the reference-driven run: 5 and 150)."""
    g, box, n_elec, chi, tn, _b = ground_state
    E, grad = tn._at
    n = T.density(box, chi, n_elec)[2]
    n_ref = T.density(box, g['chi_gs'], n_elec)[2]
    dden = float(np.abs(n - n_ref).max() / n_ref.max())
    print('MEASURE tn cpu g16r: E - E_gs %.2e Ha  density %.2e  |g|_2 %.2e  outer %d evals %d products %d (golden %s)'
          % (E - float(g['E_gs']), dden, np.linalg.norm(grad), tn.total_iter, tn.func_evals, tn.hvp_count, g['counts']))
    assert np.linalg.norm(grad) <= 1e-10
    assert abs(E - float(g['E_gs'])) <= E_BOUND_HA
    assert dden <= 10 * MEASURED['den_gs']
    assert tn.total_iter <= MAX_OUTER and tn.hvp_count <= MAX_PRODUCTS
    assert [c[1] for c in tn.cg_log][:3] == [optimize.CG_CONVERGED] * 3          # the early solves end on the forcing term


def test_density_response_matches_the_golden(ground_state):
    """dn and dmu at the golden ground state for tn_cases.response_dv, conjugate gradients to 1e-12 as in the golden.
    Measured: dn 2.6e-12 of max|dn|, dmu 1.3e-10 relative (dmu = 2.5e-6 is what is left of two sums of ~1e-3); the same 153
    iterations; sum dn = 0 to rounding."""
    g, box, n_elec, _chi, _tn, backend = ground_state
    dv = tn_cases.response_dv(g['dn'].shape)
    r = optimize.density_response(None, g['chi_gs'], n_elec, dv, rtol=1e-12, maxiter=500, backend=backend)
    ddn = float(np.abs(r['dn'] - g['dn']).max() / np.abs(g['dn']).max())
    dmu = abs(r['dmu'] - float(g['dmu'])) / abs(float(g['dmu']))
    print('MEASURE response cpu g16r: dn %.2e dmu %.2e iterations %d (golden %d)' % (ddn, dmu, r['iterations'], int(g['cg_iters'])))
    assert r['reason'] == optimize.CG_CONVERGED and r['rel_residual'] <= 1e-12
    assert ddn <= 10 * MEASURED['dn'] and dmu <= 10 * MEASURED['dmu']
    assert abs(r['dn'].sum()) <= 1e-14 * np.abs(r['dn']).sum()


def test_solver_exit_reasons():
    """iteration cap and non-positive curvature as solve_projected reports them (a 2 x 2 x 2 grid with a made-up operator)"""
    Diag = T.DiagCgBackend
    phi = np.ones((2, 2, 2))
    b = np.arange(8.0).reshape(2, 2, 2) - 3.5
    x, it, reason, rel, nprod = optimize.solve_projected(Diag(np.linspace(1, 2, 8).reshape(2, 2, 2)), phi, None, b, 1.0, 1e-12, 2)
    assert (it, reason, nprod) == (2, optimize.CG_MAXITER, 2) and rel > 1e-12
    x, it, reason, rel, nprod = optimize.solve_projected(Diag(-np.ones((2, 2, 2))), phi, None, b, 1.0, 1e-12, 50)
    assert (it, reason, nprod) == (0, optimize.CG_CURVATURE, 1) and np.array_equal(x, b)       # x = p = the projected b
    x, it, reason, rel, nprod = optimize.solve_projected(Diag(np.ones((2, 2, 2))), phi, None, b, 1.0, 1e-12, 50)
    assert (it, reason) == (1, optimize.CG_CONVERGED) and np.allclose(x, b, rtol=0, atol=1e-15)


@pytest.mark.parametrize('dtype', [N.F64, N.F32])
def test_entry_points_are_exported_and_refuse_null_handles(dtype):
    lib = N.load(dtype)
    for sym in ('ofdft_hessian_vector_chi', 'ofdft_cg_create', 'ofdft_cg_start', 'ofdft_cg_step', 'ofdft_cg_status', 'ofdft_cg_solution'):
        assert sym in N.EXPORTS and hasattr(lib, sym)
    s = (ctypes.c_double * N.HVC_NSCALARS)()
    assert lib.ofdft_hessian_vector_chi(None, None, None, None, 1.0, None, s, 0, None) == N.EINVAL
    reason = ctypes.c_int(0)
    assert lib.ofdft_cg_step(None, None, 1.0, 0.0, ctypes.byref(reason), None) == N.EINVAL
    assert lib.ofdft_cg_create(None, 8, 0) == N.EINVAL
    assert lib.ofdft_cg_status(None, None, None, None) == N.EINVAL


def test_unknown_method_is_still_a_value_error():
    with pytest.raises(ValueError, match='n_method'):
        optimize.optimize_density(None, 8.0, n_method='SD')
