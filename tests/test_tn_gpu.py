"""GPU tests of the chi-space Hessian-vector product (ofdft_hessian_vector_chi, Engine.hessian_vector_chi), the device
conjugate-gradient solver (ofdft_cg_*), optimize_density(n_method='TN') and optimize.density_response, against the reference's
double autograd (tests/golden/tn_<case>.npz; generator tests/golden/make_golden_tn.py) and, on grids without goldens, the numpy
double (tests/tn_double.py).

Tolerance rule (that of tests/test_hvp_gpu.py): 10 x the largest deviation from the reference's golden -- or from the numpy
double where no golden exists -- measured on an MI355X over the cases (MEASURED_* below; every test prints its figures as
`MEASURE ...` before it asserts and lists them in its docstring).  The yardstick is always the reference's output.
"""
import os

import numpy as np
import pytest
import torch

import cases
import hvp_cases
import hvp_double as D
import tn_cases
import tn_double as T
from professad_amd import _native as N
from professad_amd import optimize
from professad_amd.engine import Engine

pytestmark = pytest.mark.gpu
GOLDEN = os.path.dirname(os.path.abspath(cases.__file__))
DEV = 'cuda:0'
TERMS = list(tn_cases.TERMS)
SIX = ('hartree', 'tf', 'vw', 'wt_nl', 'lda_x', 'pz_c')
EPS = 2.0 ** -52

# largest figures measured on an MI355X (per-case values in the docstrings of the tests that use them)
MEASURED_HD = 4.88e-14           # max|Hd - golden| / max|golden|, three cases
MEASURED_DHD = 4.33e-15          # |d.Hd - golden| / |golden|
MEASURED_DOUBLE = {(48, 96, 32): 2.63e-15, (32, 16, 64): 1.20e-13}      # max|Hd - double| / max|double|
MEASURED_E_GS = 2.78e-16         # |E - E_gs| [Ha], g16r (a figure below one rounding of E_gs counts as that rounding)
MEASURED_DEN_GS = 5.86e-12       # max|n - n_gs| / max n_gs, g16r
MEASURED_DN = 2.64e-12           # max|dn - golden| / max|golden|, three cases
MEASURED_DMU = 1.33e-10          # |dmu - golden| / |golden|
MEASURED_EULER = 1.93e-12        # max|hv(n, dn) + dv - mean| / max|dv|
FD_BOUND = 10 * 9.2e-9           # central difference of two ground states at eps = 1e-2: 10 x the reference-only figure
MAX_OUTER, MAX_PRODUCTS = 8, 200


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.double, device=DEV)


_GOLD = {}


def gold(case):
    """golden file and inputs of a case, loaded once and shared"""
    if case not in _GOLD:
        g = np.load(os.path.join(GOLDEN, 'tn_%s.npz' % case))
        box, phi, d, vext, n_elec = tn_cases.make_inputs(case)
        assert abs(cases.checksum(box, phi, d, vext) - float(g['checksum'])) < 1e-9
        _GOLD[case] = (g, box, phi, d, vext, n_elec)
    return _GOLD[case]


def engine(shape, box, names=TERMS, al=None, be=None):
    return Engine(shape, DEV).set_cell(box).set_terms(list(names), None if al is None else dict(wt_alpha=al, wt_beta=be))


# ------------------------------------------------------------------------------- 1: H d against the goldens
@pytest.mark.parametrize('case', tn_cases.CASES)
def test_product_matches_the_reference_goldens(case):
    """Engine.hessian_vector_chi at phi = 1.7 sqrt(den) with the gradient of the engine's own closure, against the reference's
    grad((g d).sum(), chi).  Measured on an MI355X, g16r / g17r / g18t: H d 4.5e-14 / 4.4e-14 / 4.9e-14 of max|H d| (the n-space
    product of the same set sits at 3.5e-14 / 5.5e-14 / 4.1e-14, tests/test_hvp_gpu.py), d.H d 2.7e-15 / 4.3e-15 / 2.2e-15; the closure
    gradient itself is within 6.3e-14 / 7.2e-14 / 6.4e-14 of the golden's."""
    g, box, phi, d, vext, n_elec = gold(case)
    eng = engine(phi.shape, box)
    tphi, td = dev(phi), dev(d)
    _E, _mu, grad = eng.energy_grad_chi(tphi, n_elec, dev(vext))
    dg = float(np.abs(grad.cpu().numpy() - g['g']).max() / np.abs(g['g']).max())
    s, Hd = eng.hessian_vector_chi(tphi, td, grad, n_elec, want_scalars=True)
    eng.close()
    Hd = Hd.cpu().numpy()
    dH = float(np.abs(Hd - g['Hd']).max() / np.abs(g['Hd']).max())
    dq = abs(s['dHd'] - float(g['dHd'])) / abs(float(g['dHd']))
    print('MEASURE tn %s: Hd %.2e dHd %.2e (gradient %.2e)' % (case, dH, dq, dg))
    assert dH <= 10 * MEASURED_HD and dq <= 10 * MEASURED_DHD
    # the returned scalars belong to the returned field
    assert abs(s['dHd'] - float((d * Hd).sum())) <= 1e-12 * float(np.abs(d * Hd).sum())
    assert abs(s['phiHd'] - float((phi * Hd).sum())) <= 1e-12 * float(np.abs(phi * Hd).sum())
    assert s['a'] == pytest.approx(float((phi * d).sum()), rel=1e-12) and s['S'] == pytest.approx(float((phi * phi).sum()), rel=1e-13)


# ------------------------------------------------------------------------------- 2: identities
def test_identities_on_g18t():
    """H phi = -g; <u, H d> = <d, H u>; the implied dn sums to zero; g=None is the call with a zero array, bit for bit.
    Bounds: those of the product (MEASURED_HD) times the scale of the quantity.  Measured on an MI355X: H phi + g 1.5e-15 of max|g|,
    symmetry 3.6e-18 of |u| |H d|, sum dn 1.6e-18 of sum |dn|."""
    g, box, phi, d, vext, n_elec = gold('g18t')
    eng = engine(phi.shape, box)
    tphi, td = dev(phi), dev(d)
    u = hvp_cases.direction(phi.shape, seed=82)
    tu = dev(u)
    _E, _mu, grad = eng.energy_grad_chi(tphi, n_elec, dev(vext))
    Hphi = eng.hessian_vector_chi(tphi, tphi, grad, n_elec)
    ident = float((Hphi + grad).abs().max() / grad.abs().max())
    s, Hd = eng.hessian_vector_chi(tphi, td, grad, n_elec, reuse_density=True, want_scalars=True)
    Hu = eng.hessian_vector_chi(tphi, tu, grad, n_elec, reuse_density=True)
    a, b = float((tu * Hd).sum()), float((td * Hu).sum())
    scale = float(tu.norm() * Hd.norm())
    # the density variation the call forms: dn = 2 c phi d - (2 a / S) n
    S, c, n = T.density(box, phi, n_elec)
    dn = 2 * c * phi * d - (2 * s['a'] / s['S']) * n
    dsum = abs(dn.sum()) / np.abs(dn).sum()
    print('MEASURE tn identities g18t: H phi + g %.2e  symmetry %.2e  sum dn %.2e' % (ident, abs(a - b) / scale, dsum))
    assert ident <= 10 * MEASURED_HD
    assert abs(a - b) <= 10 * MEASURED_HD * scale
    assert dsum <= 64 * EPS
    H0 = eng.hessian_vector_chi(tphi, td, None, n_elec, reuse_density=True)
    Hz = eng.hessian_vector_chi(tphi, td, torch.zeros_like(tphi), n_elec, reuse_density=True)
    assert torch.equal(H0, Hz) and not torch.equal(H0, Hd)
    eng.close()


# ------------------------------------------------------------------------------- 3: reuse
def test_reuse_density_is_bitwise_and_skips_the_density_transforms():
    g, box, phi, d, _vext, n_elec = gold('g16r')
    eng = engine(phi.shape, box, SIX)
    tphi, td, tg = dev(phi), dev(d), dev(g['g'])

    def call(reuse, **kw):
        return eng.hessian_vector_chi(tphi, td, tg, n_elec, reuse_density=reuse, **kw)
    with pytest.raises(RuntimeError, match=r'\(-3\)'):          # nothing retained yet: OFDFT_ESTATE
        call(True)
    s0, H0 = call(False, want_scalars=True)
    assert eng.query(N.Q_FFT_COUNT) == 10 and eng.query(N.Q_LAUNCH_COUNT) > 0
    s1, H1 = call(True, want_scalars=True)
    assert eng.query(N.Q_FFT_COUNT) == 6
    assert torch.equal(H0, H1) and s0 == s1
    assert torch.equal(call(True), H0)                            # without the host read of the scalars
    # the n-space product's retained fields are its own: neither entry reuses the other's
    den = dev(T.density(box, phi, n_elec)[2])
    with pytest.raises(RuntimeError, match=r'\(-3\)'):
        eng.hessian_vector(den, td, reuse_density=True)
    eng.hessian_vector(den, td)
    with pytest.raises(RuntimeError, match=r'\(-3\)'):
        call(True)
    assert torch.equal(call(False), H0)
    # set_terms, an energy call and set_cell invalidate
    eng.set_terms(['tf'])
    eng.set_terms(list(SIX))
    with pytest.raises(RuntimeError, match=r'\(-3\)'):
        call(True)
    assert torch.equal(call(False), H0)
    eng.energy_potential(den)
    with pytest.raises(RuntimeError, match=r'\(-3\)'):
        call(True)
    assert torch.equal(call(False), H0)
    eng.set_cell(box * 1.01)
    with pytest.raises(RuntimeError, match=r'\(-3\)'):
        call(True)
    eng.close()


# ------------------------------------------------------------------------------- 4: other transform families
@pytest.mark.parametrize('shape,triclinic', [((48, 96, 32), True), ((32, 16, 64), False)])
def test_mixed_radix_and_unequal_powers_of_two_match_the_double(shape, triclinic):
    """cfg2's terms with the Wang-Teter exponents of WGC98 (alpha != beta) against tests/tn_double.py with a made-up gradient
    perpendicular to phi.  Measured on an MI355X: 2.6e-15 on (48, 96, 32), 1.2e-13 on (32, 16, 64) of max|H d| (the n-space product sits
    at 2.4e-15 and 1.3e-13 there: the nonlocal kernel's conditioning, tests/test_hvp_gpu.py)."""
    from professad_amd import synth
    box = synth.triclinic_cell(shape[0] / 8.0) if triclinic else synth.cubic_cell(32)
    den = synth.random_density(shape, seed=11)
    phi = 0.6 * np.sqrt(den)
    d = hvp_cases.direction(shape, seed=83)
    gr = hvp_cases.direction(shape, seed=84)
    gr -= phi * (phi * gr).sum() / (phi * phi).sum()
    n_elec = float(den.sum() * abs(np.linalg.det(box)) / den.size)
    al, be = D.WGC98
    sd, Hdd = T.hessian_vector_chi(box, phi, d, gr, n_elec, TERMS, al, be)
    eng = engine(shape, box, TERMS, al, be)
    s, Hd = eng.hessian_vector_chi(dev(phi), dev(d), dev(gr), n_elec, want_scalars=True)
    assert eng.query(N.Q_FFT_COUNT) == 14
    eng.close()
    dH = float(np.abs(Hd.cpu().numpy() - Hdd).max() / np.abs(Hdd).max())
    print('MEASURE tn double %s: Hd %.2e dHd %.2e dmu %.2e' % (shape, dH, abs(s['dHd'] - sd['dHd']) / abs(sd['dHd']),
                                                             abs(s['dmu'] - sd['dmu']) / abs(sd['dmu'])))
    assert dH <= 10 * MEASURED_DOUBLE[shape]
    assert abs(s['dHd'] - sd['dHd']) <= 10 * MEASURED_DOUBLE[shape] * float(np.abs(d * Hdd).sum())


# ------------------------------------------------------------------------------- 5: truncated Newton
_GS = {}


def ground_state(shift=0.0):
    """optimize_density(n_method='TN') from the uniform density on g16r in vext + shift * response_dv; run once per shift"""
    if shift not in _GS:
        _g, box, phi, _d, vext, n_elec = gold('g16r')
        eng = engine(phi.shape, box)
        v = dev(vext + shift * tn_cases.response_dv(phi.shape))
        _GS[shift] = optimize.optimize_density(eng, n_elec, v, volume=abs(np.linalg.det(box)), n_method='TN')
        eng.close()
    return _GS[shift]


def test_truncated_newton_from_the_uniform_density():
    """g16r: the golden ground-state energy and density within 10 x the figures measured on an MI355X (E 2.8e-16 Ha, density 5.9e-12
    of max n: the run stops at |g|_2 = 5e-12, the golden at 2.5e-12; 5 Newton steps, 6 evaluations, 150 products, 8 outer
    iterations of optimize_density of which the last three do nothing), in at most 8 outer iterations and 200 products (the reference-driven run: 5 and 150 to |g|_2 = 5e-12)."""
    g, box, _phi, _d, _vext, n_elec = gold('g16r')
    r = ground_state()
    n_ref = T.density(box, g['chi_gs'], n_elec)[2]
    dE = r['E_Ha'] - float(g['E_gs'])
    dden = float(np.abs(r['den'].cpu().numpy() - n_ref).max() / n_ref.max())
    print('MEASURE tn g16r: E - E_gs %.2e Ha  density %.2e  outer %d evals %d products %d  max|g|/dV %.2e'
          % (dE, dden, r['iterations'], r['func_evals'], r['hvp_count'], r['history'][-1][3]))
    assert r['converged']
    assert abs(dE) <= 10 * max(MEASURED_E_GS, EPS * abs(float(g['E_gs']))) and dden <= 10 * MEASURED_DEN_GS
    assert r['iterations'] <= MAX_OUTER and 0 < r['hvp_count'] <= MAX_PRODUCTS


# ------------------------------------------------------------------------------- 6: density response
@pytest.mark.parametrize('case', tn_cases.CASES)
def test_density_response_matches_the_goldens(case):
    """dn and dmu at the golden ground state against the golden's (conjugate gradients to 1e-12 in both), and the Euler
    residual max|hv(n, dn) + dv - mean| / max|dv| with Engine.hessian_vector as the judge (reference-only: 1.9e-12).
    Measured on an MI355X, g16r / g17r / g18t: dn 2.6e-12 / 3.1e-14 / 3.2e-13 of max|dn|, dmu 1.3e-10 / 1.4e-14 / 5.3e-14 (g16r's dmu,
    2.5e-6, is what is left of two sums of ~1e-3), Euler 1.5e-12 / 1.6e-12 / 1.9e-12; 153 / 154 / 193 iterations, the goldens' counts."""
    g, box, _phi, _d, _vext, n_elec = gold(case)
    shape = g['dn'].shape
    dv = tn_cases.response_dv(shape)
    eng = engine(shape, box)
    chi = dev(g['chi_gs'])
    r = optimize.density_response(eng, chi, n_elec, dev(dv), rtol=1e-12, maxiter=500)
    dn = r['dn'].cpu().numpy()
    n = dev(T.density(box, g['chi_gs'], n_elec)[2])
    res = (eng.hessian_vector(n, r['dn']) + dev(dv)).cpu().numpy()
    eng.close()
    euler = float(np.abs(res - res.mean()).max() / np.abs(dv).max())
    ddn = float(np.abs(dn - g['dn']).max() / np.abs(g['dn']).max())
    dmu = abs(r['dmu'] - float(g['dmu'])) / abs(float(g['dmu']))
    print('MEASURE response %s: dn %.2e dmu %.2e euler %.2e  iterations %d (golden %d) residual %.2e'
          % (case, ddn, dmu, euler, r['iterations'], int(g['cg_iters']), r['rel_residual']))
    assert r['reason'] == optimize.CG_CONVERGED and r['rel_residual'] <= 1e-12
    assert ddn <= 10 * MEASURED_DN and dmu <= 10 * MEASURED_DMU and euler <= 10 * MEASURED_EULER
    assert abs(dn.sum()) <= 64 * EPS * np.abs(dn).sum()


def test_density_response_is_the_derivative_of_the_ground_state():
    """g16r: dn against the central difference of two truncated-Newton ground states at v +- eps dv, eps = 1e-2.  The bound is
    10 x the reference-only 9.2e-9 of max|dn|: the eps^2 truncation dominates and does not depend on the device.
    Measured on an MI355X: 1.55e-8."""
    g, box, _phi, _d, _vext, n_elec = gold('g16r')
    dv = tn_cases.response_dv(g['dn'].shape)
    eps = 1e-2
    plus, minus = ground_state(eps), ground_state(-eps)
    fd = ((plus['den'] - minus['den']) / (2 * eps)).cpu().numpy()
    eng = engine(g['dn'].shape, box)
    r = optimize.density_response(eng, ground_state()['chi'], n_elec, dev(dv), rtol=1e-12, maxiter=500)
    eng.close()
    d = float(np.abs(r['dn'].cpu().numpy() - fd).max() / np.abs(fd).max())
    print('MEASURE response finite difference g16r: %.2e' % d)
    assert d <= FD_BOUND


# ------------------------------------------------------------------------------- 7: fcc-Al end to end
def test_truncated_newton_and_lbfgs_agree_on_fcc_al():
    """fcc-Al primitive cell, 20^3, ion-electron + Hartree + Wang-Teter + Perdew-Zunger with the recpot of ions.npz: truncated
    Newton and the fused L-BFGS (ntol 1e-7) agree within 5e-4 eV, the bound between optimisers of tests/test_gpu_parity.py.
    Measured on an MI355X: -1.5e-7 eV (L-BFGS 22 outer iterations, 120 evaluations; truncated Newton 7 evaluations, 177 products)."""
    from professad_amd.ions import ionic_potential, recpot_table
    g = np.load(os.path.join(GOLDEN, 'ions.npz'))
    tab = recpot_table(g['recpot_raw'], float(g['recpot_kmax']))
    box = 4.050 / 0.529177210903 * np.array([[0.5, 0.5, 0.0], [0.0, 0.5, 0.5], [0.5, 0.0, 0.5]])
    vol = abs(np.linalg.det(box))
    eng = Engine((20, 20, 20), DEV).set_cell(dev(box))
    vext = ionic_potential(eng, box, [(np.zeros((1, 3)), tab)])
    eng.set_terms(TERMS)
    n_el = float(tab[2])
    r1 = optimize.optimize_density(eng, n_el, vext, volume=vol, ntol=1e-7)
    r2 = optimize.optimize_density(eng, n_el, vext, volume=vol, ntol=1e-7, n_method='TN')
    eng.close()
    d = (r2['E_Ha'] - r1['E_Ha']) * optimize.EV_PER_HA
    print('MEASURE fcc-Al: E(TN) - E(L-BFGS) %.3e eV; L-BFGS %d iterations %d evaluations; TN %d iterations %d evaluations %d products'
          % (d, r1['iterations'], r1['func_evals'], r2['iterations'], r2['func_evals'], r2['hvp_count']))
    assert r1['converged'] and r2['converged'] and r1['hvp_count'] == 0 and r2['hvp_count'] > 0
    assert abs(d) < 5e-4


# ------------------------------------------------------------------------------- 8: refusals
@pytest.mark.parametrize('names,word', [(('tf', 'vw', 'wgc99_nl'), 'wgc99_nl'), (('pbe_x', 'pbe_c'), 'pbe_x')])
def test_unserved_term_sets_are_refused_by_name(names, word):
    _g, box, phi, d, _vext, n_elec = gold('g16r')
    eng = Engine(phi.shape, DEV).set_cell(box).set_terms(list(names))
    with pytest.raises(RuntimeError, match=r'\(-1\).*\b%s\b' % word):
        eng.hessian_vector_chi(dev(phi), dev(d), None, n_elec)
    with pytest.raises(NotImplementedError, match=word):
        optimize.optimize_density(eng, n_elec, volume=abs(np.linalg.det(box)), n_method='TN')
    with pytest.raises(NotImplementedError, match=word):
        optimize.density_response(eng, dev(phi), n_elec, dev(d))
    eng.close()


def test_slab_and_fp32_engines_refuse_and_unknown_methods_stay_value_errors():
    from professad_amd.distributed import DistEngine
    _g, box, phi, d, _vext, n_elec = gold('g16r')
    vol = abs(np.linalg.det(box))
    de = DistEngine(phi.shape, DEV).set_cell(torch.as_tensor(box)).set_terms(['tf'])
    with pytest.raises(NotImplementedError, match='single-GPU'):
        de.hessian_vector_chi(dev(phi), dev(d), None, n_elec)
    with pytest.raises(NotImplementedError, match='single-GPU'):
        optimize.optimize_density(de, n_elec, volume=vol, n_method='TN')
    de.close()
    e32 = Engine(phi.shape, DEV, dtype=torch.float32).set_cell(box).set_terms(['tf'])
    with pytest.raises(NotImplementedError, match='fp64'):
        e32.hessian_vector_chi(dev(phi).float(), dev(d).float(), None, n_elec)
    with pytest.raises(NotImplementedError, match='fp64'):
        optimize.optimize_density(e32, n_elec, volume=vol, n_method='TN')
    with pytest.raises(ValueError):
        optimize.optimize_density(e32, n_elec, volume=vol, n_method='SD')
    e32.close()
