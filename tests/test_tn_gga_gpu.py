"""GPU tests of the second-order stack on Wang-Teter + PBE (cfg3 of tests/golden/hvp_gga_cases.py) under OFDFT_OPT_HVP_GGA = 1
(DESIGN.md §9k): Engine.hessian_vector_chi, optimize_density(n_method='TN') and optimize.density_response against the reference's
double autograd (tests/golden/tn_gga_<case>.npz; generator tests/golden/make_golden_tn_gga.py), and one column of
force_constants against finite differences of forces between re-relaxed ground states.

Tolerance rule (that of tests/test_tn_gpu.py): 10 x the largest deviation from the reference's golden measured on an MI355X over the
cases (MEASURED_* below; every test prints its figures as `MEASURE ...` before it asserts and lists them in its docstring).
"""
import os

import numpy as np
import pytest
import torch

import cases
import fc_cases
import hvp_gga_cases as G
import tn_cases
import tn_double as T
from professad_amd import _native as N
from professad_amd import ions, optimize
from professad_amd.engine import Engine
from professad_amd.force_constants import force_constants

pytestmark = pytest.mark.gpu
GOLDEN = os.path.dirname(os.path.abspath(cases.__file__))
DEV = 'cuda:0'
CFG3, AL, BE = G.CFG3
TERMS = list(CFG3)
EPS = 2.0 ** -52

# largest figures measured on an MI355X (per-case values in the docstrings of the tests that use them)
MEASURED_HD = 2.77e-14                # max|Hd - golden| / max|golden|, three cases
MEASURED_DHD = 5.78e-15               # |d.Hd - golden| / |golden|
MEASURED_E_GS = 2.91e-16              # |E - E_gs| [Ha], g16r (a figure below one rounding of E_gs counts as that rounding)
MEASURED_DEN_GS = 8.12e-12            # max|n - n_gs| / max n_gs, g16r
MEASURED_DN = 5.61e-13                # max|dn - golden| / max|golden|, three cases, plain and preconditioned
MEASURED_DMU = 2.81e-12               # |dmu - golden| / |golden|
MEASURED_FD_COLUMN = 1.975e-7         # force-constant column against the central difference, of max|Phi|
# the LDA figure of tests/test_force_constants_gpu.py: same eps, cell and grid, and XC is a small part of Phi -- more than ten times
# it would be a finding
FD_COLUMN_LDA = 2.65e-7
FD_EPS = 1e-3
FD_COLUMN = (2, 1)
RTOL = 1e-11
MAX_OUTER, MAX_PRODUCTS = 10, 300      # the reference-driven run on g16r: 6 Newton steps, 204 products


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.double, device=DEV)


_GOLD = {}


def gold(case):
    """golden file and inputs of a case, loaded once and shared"""
    if case not in _GOLD:
        g = np.load(os.path.join(GOLDEN, 'tn_gga_%s.npz' % case))
        box, phi, d, vext, n_elec = tn_cases.make_inputs(case)
        assert abs(cases.checksum(box, phi, d, vext) - float(g['checksum'])) < 1e-9
        _GOLD[case] = (g, box, phi, d, vext, n_elec)
    return _GOLD[case]


def engine(shape, box):
    return Engine(shape, DEV).set_cell(box).set_terms(TERMS, dict(wt_alpha=AL, wt_beta=BE)).set_option(N.OPT_HVP_GGA, 1)


# ------------------------------------------------------------------------------- 1: H d against the goldens
@pytest.mark.parametrize('case', G.TN_CASES)
def test_product_matches_the_reference_goldens(case):
    """Engine.hessian_vector_chi at phi = 1.7 sqrt(den) with the gradient of the engine's own closure, against the reference's
    grad((g d).sum(), chi); the reuse call is bitwise the same and runs 14 transforms for the 22 of the first.
    Measured on an MI355X, g16r / g17r / g18t: H d 2.8e-14 / 2.6e-14 / 2.6e-14 of max|H d| (cfg2: 4.5e-14 / 4.4e-14 / 4.9e-14,
    tests/test_tn_gpu.py), d.H d 3.7e-15 / 5.8e-15 / 1.7e-15; the closure gradient itself is within 4.5e-14 / 4.6e-14 / 4.1e-14 of the golden's."""
    g, box, phi, d, vext, n_elec = gold(case)
    eng = engine(phi.shape, box)
    tphi, td = dev(phi), dev(d)
    _E, _mu, grad = eng.energy_grad_chi(tphi, n_elec, dev(vext))
    dg = float(np.abs(grad.cpu().numpy() - g['g']).max() / np.abs(g['g']).max())
    s, Hd = eng.hessian_vector_chi(tphi, td, grad, n_elec, want_scalars=True)
    n0 = eng.query(N.Q_FFT_COUNT)
    s1, Hd1 = eng.hessian_vector_chi(tphi, td, grad, n_elec, reuse_density=True, want_scalars=True)
    n1 = eng.query(N.Q_FFT_COUNT)
    eng.close()
    same = torch.equal(Hd, Hd1) and s == s1
    Hd = Hd.cpu().numpy()
    dH = float(np.abs(Hd - g['Hd']).max() / np.abs(g['Hd']).max())
    dq = abs(s['dHd'] - float(g['dHd'])) / abs(float(g['dHd']))
    print('MEASURE tn_gga %s: Hd %.2e dHd %.2e (gradient %.2e)  transforms %d / %d' % (case, dH, dq, dg, n0, n1))
    assert dH <= 10 * MEASURED_HD and dq <= 10 * MEASURED_DHD
    assert same and (n0, n1) == (22, 14)
    assert abs(s['dHd'] - float((d * Hd).sum())) <= 1e-12 * float(np.abs(d * Hd).sum())
    assert abs(s['phiHd'] - float((phi * Hd).sum())) <= 1e-12 * float(np.abs(phi * Hd).sum())


# ------------------------------------------------------------------------------- 2: truncated Newton
def test_truncated_newton_from_the_uniform_density():
    """g16r: optimize_density(n_method='TN') reaches the golden ground-state energy and density within 10 x the figures measured on
    an MI355X: E 2.9e-16 Ha, density 8.1e-12 of max n (the run stops at |g|_2 <= 1e-10, the golden at 5.7e-15; 6 evaluations, 154 products,
    8 outer iterations of optimize_density); the reference-driven run takes 6 Newton steps and 204 products to |g|_2 = 5.7e-15."""
    g, box, phi, _d, vext, n_elec = gold('g16r')
    eng = engine(phi.shape, box)
    r = optimize.optimize_density(eng, n_elec, dev(vext), volume=abs(np.linalg.det(box)), n_method='TN')
    eng.close()
    n_ref = T.density(box, g['chi_gs'], n_elec)[2]
    dE = r['E_Ha'] - float(g['E_gs'])
    dden = float(np.abs(r['den'].cpu().numpy() - n_ref).max() / n_ref.max())
    print('MEASURE tn_gga g16r: E - E_gs %.2e Ha  density %.2e  outer %d evals %d products %d  max|g|/dV %.2e'
          % (dE, dden, r['iterations'], r['func_evals'], r['hvp_count'], r['history'][-1][3]))
    assert r['converged']
    assert abs(dE) <= 10 * max(MEASURED_E_GS, EPS * abs(float(g['E_gs']))) and dden <= 10 * MEASURED_DEN_GS
    assert r['iterations'] <= MAX_OUTER and 0 < r['hvp_count'] <= MAX_PRODUCTS


# ------------------------------------------------------------------------------- 3: density response
@pytest.mark.parametrize('case', G.TN_CASES)
def test_density_response_matches_the_goldens(case):
    """dn and dmu at the golden ground state against the golden's (conjugate gradients to 1e-12 in both), plain and with
    precondition='auto' (the same solution in fewer iterations).  Measured on an MI355X, g16r / g17r / g18t: plain dn 4.0e-15 / 1.8e-14 / 4.6e-13 of max|dn|,
    dmu 2.0e-13 / 2.4e-14 / 1.2e-14, in 155 / 156 / 193 iterations, the goldens' counts; preconditioned dn 1.3e-13 / 2.6e-13 / 5.6e-13,
    dmu 2.8e-12 / 6.3e-15 / 1.8e-14 in 16 / 16 / 17 (g16r's dmu, 2.4e-6, is what is left of two sums of ~1e-3)."""
    g, box, _phi, _d, _vext, n_elec = gold(case)
    shape = g['dn'].shape
    dv = tn_cases.response_dv(shape)
    eng = engine(shape, box)
    chi = dev(g['chi_gs'])
    figs = []
    for pre in (None, 'auto'):
        r = optimize.density_response(eng, chi, n_elec, dev(dv), rtol=1e-12, maxiter=500, precondition=pre)
        dn = r['dn'].cpu().numpy()
        ddn = float(np.abs(dn - g['dn']).max() / np.abs(g['dn']).max())
        dmu = abs(r['dmu'] - float(g['dmu'])) / abs(float(g['dmu']))
        print('MEASURE response_gga %s precondition=%s: dn %.2e dmu %.2e  iterations %d (golden %d) residual %.2e'
              % (case, pre, ddn, dmu, r['iterations'], int(g['cg_iters']), r['rel_residual']))
        figs.append((pre, r, ddn, dmu, dn))
    eng.close()
    for pre, r, ddn, dmu, dn in figs:
        assert r['reason'] == optimize.CG_CONVERGED and r['rel_residual'] <= 1e-12, pre
        assert ddn <= 10 * MEASURED_DN and dmu <= 10 * MEASURED_DMU, pre
        assert abs(dn.sum()) <= 64 * EPS * np.abs(dn).sum()
    assert figs[1][1]['iterations'] < figs[0][1]['iterations']


# ------------------------------------------------------------------------------- 4: one column of the force constants
def a16():
    box, shape, frac, _den, raw, k_max = fc_cases.make_inputs('a16')
    tab = ions.recpot_table(raw, k_max)
    return box, shape, frac, tab, np.full(frac.shape[0], float(tab[2]))


def relaxed(frac, chi0=None):
    """truncated-Newton ground state of the a16 cell with the ions at `frac` for Wang-Teter + PBE -> chi, density"""
    box, shape, _frac, tab, z = a16()
    eng = Engine(shape, DEV).set_cell(box)
    vext = ions.ionic_potential(eng, box, [(frac, tab)])
    eng.set_terms(TERMS, dict(wt_alpha=AL, wt_beta=BE)).set_option(N.OPT_HVP_GGA, 1)
    r = optimize.optimize_density(eng, float(z.sum()), vext, chi0=chi0, volume=abs(np.linalg.det(box)), n_method='TN')
    eng.close()
    assert r['converged']
    return r['chi'], r['den']


def test_a_column_is_the_central_difference_of_forces_between_relaxed_ground_states():
    """fcc Al, 16^3, Wang-Teter + PBE: Phi[:, b, :, j] from force_constants(batch=None) against -(F(R + eps) - F(R - eps)) / (2 eps), F the
    ion-electron plus ion-ion forces at truncated-Newton ground states re-relaxed at both displaced geometries, eps = 1e-3 bohr,
    for the column (ion 2, y) of tests/test_force_constants_gpu.py.  Bound: 10 x the figure measured on an MI355X, 1.98e-7 of max|Phi| = 4.517e-2 Ha/bohr^2 (the eps^2 truncation; twelve solves of 103-104
    iterations, 1242 products, max|g|/dV 1.2e-11);
    more than ten times the LDA figure of that file (2.65e-7 of max|Phi|) would be a finding."""
    box, shape, frac, tab, z = a16()
    chi, _den = relaxed(frac)
    eng = engine(shape, box)
    r = force_constants(eng, box, [(frac, tab)], chi, rtol=RTOL)
    ib, j = FD_COLUMN
    F = {}
    for sign in (+1, -1):
        cart = frac @ box
        cart[ib, j] += sign * FD_EPS
        f = cart @ np.linalg.inv(box)
        _chi, den = relaxed(f, chi0=chi)
        F[sign] = ions.ion_electron_forces(eng, box, den, [(f, tab)])[0] + ions.ion_ion(eng, box, f, z)[1]
    eng.close()
    fd = -(F[+1] - F[-1]) / (2 * FD_EPS)
    phi = r['phi']
    d = float(np.abs(phi[:, ib, :, j] - fd).max() / np.abs(phi).max())
    print('MEASURE fc_gga a16 finite difference column (%d, %d): %.3e  max|Phi| %.4e  iterations %d..%d products %d  max|g|/dV %.2e'
          % (ib, j, d, np.abs(phi).max(), min(r['iterations']), max(r['iterations']), r['hvp_count'], r['ground_state_gradient']))
    assert all(x == optimize.CG_CONVERGED for x in r['reason'])
    assert MEASURED_FD_COLUMN <= 10 * FD_COLUMN_LDA
    assert d <= 10 * MEASURED_FD_COLUMN
