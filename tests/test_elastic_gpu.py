"""GPU tests of the elastic constants: the strain-gradient entries (Engine.potential_strain_gradient,
ions.ionic_potential_strain_gradient) and the fixed-chi second strain derivatives (Engine.strain_hessian,
ions.ion_electron_strain_hessian, ions.ion_ion_strain_hessian) against the reference's own autograd
(tests/golden/elastic_<case>.npz; generator tests/golden/make_golden_elastic.py) and, on grids without goldens, the numpy double
(tests/elastic_double.py); professad_amd.elastic end to end on the fcc-Al 16^3 case against the numpy-driven tensor and against
finite differences of the native stress between re-relaxed ground states.

Tolerance rule: against a golden or the double, ten times the deviation of the numpy double from the same golden, measured on
the CPU (DOUBLE_DEV below, the figures of tests/test_elastic_cpu.py), capped at 1e-10 of the maximum; a finite difference, ten
times the deviation of the reference-only (numpy-driven) run of the same difference.  Every test prints its figures as
`MEASURE ...` before it asserts; the MI355X figures stand in MEASURED.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cases
import elastic_cases as EC
import elastic_double as ED
import tn_cases
from professad_amd import _native as N
from professad_amd import elastic, ions, optimize, synth
from professad_amd.engine import Engine

pytestmark = pytest.mark.gpu
GOLDEN = os.path.dirname(os.path.abspath(cases.__file__))
DEV = 'cuda:0'
TERMS = list(tn_cases.TERMS)
assert tuple(TERMS) == EC.SUMMED
CAP = 1e-10
# deviation of the numpy double from each golden, per case, relative to the maximum of the quantity
# (tests/test_elastic_cpu.py measures and pins them)
DOUBLE_DEV = {
    'w2': {'b': {'ion_electron': 9.31e-13, 'hartree': 9.23e-16, 'tf': 5.07e-16, 'vw': 8.74e-16, 'wt_nl': 7.53e-15, 'nl_0709': 9.86e-15,
                 'lda_x': 2.13e-15, 'pz_c': 3.38e-15, 'pw_c': 3.34e-15, 'chachiyo_c': 5.54e-15},
           'a16': {'ion_electron': 1.97e-12, 'hartree': 1.28e-15, 'tf': 4.20e-16, 'vw': 1.10e-15, 'wt_nl': 5.42e-15, 'nl_0709': 5.99e-15,
                   'lda_x': 1.28e-15, 'pz_c': 2.74e-15, 'pw_c': 5.64e-15, 'chachiyo_c': 1.31e-15}},
    'b_sum': {'b': 7.47e-14, 'a16': 6.43e-14},
    'b': {'ion_electron': 6.81e-14, 'hartree': 8.29e-16, 'vw': 1.63e-14, 'wt_nl': 3.47e-15, 'nl_0709': 2.87e-15},      # a16
}
# figures measured on an MI355X (per-case values in the tests' docstrings)
MEASURED = {
    'w2_golden': {'ion_electron': 1.14e-12, 'hartree': 1.34e-15, 'tf': 5.77e-16, 'vw': 6.72e-16, 'wt_nl': 2.84e-15, 'nl_0709': 3.78e-15,
                  'lda_x': 1.59e-15, 'pz_c': 2.74e-15, 'pw_c': 5.50e-15, 'chachiyo_c': 3.32e-15},        # the larger of b and a16
    'b_sum': 9.60e-14, 'b': {'ion_electron': 5.78e-14, 'hartree': 1.07e-15, 'vw': 1.67e-14, 'wt_nl': 3.28e-15},
    'w2_grids': {'ion_electron': 6.40e-12, 'hartree': 2.80e-15, 'tf': 6.52e-16, 'vw': 9.65e-16, 'wt_nl': 3.53e-14, 'lda_x': 1.96e-15,
                 'pw_c': 3.51e-15},                                                                        # the largest of the five grids
    'v_eps_double': 1.28e-13, 'ionic_double': 1.02e-13, 'b_nl_0709': 2.84e-15, 'v_eps_double_two_families': 7.72e-14,
    'ion_ion_double': {'b': 8.56e-14, 'a16': 4.03e-13},
    'a16': dict(C_numpy=2.05e-11, W2_pair_asymmetry=1.51e-12, symmetry_residual=8.870e-3, iterations=100, products=600,
                K=2.832627e-3, P=5.166e-5, fd_column_yz=5.955e-5, fd_K=2.532e-4),
}
RTOL = 1e-11


def bound(dev):
    return min(10 * dev, CAP)


def dev_t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.double, device=DEV)


def rel(a, ref):
    return float(np.abs(np.asarray(a) - ref).max() / np.abs(ref).max())


_GOLD = {}


def gold(case):
    """golden file and inputs of a case, loaded once and shared"""
    if case not in _GOLD:
        g = np.load(os.path.join(GOLDEN, 'elastic_%s.npz' % case))
        box, shape, frac, den, raw, k_max = EC.make_inputs(case)
        assert abs(cases.checksum(box, frac, den, raw) - float(g['checksum'])) < 1e-9
        _GOLD[case] = (g, box, shape, frac, den, ions.recpot_table(raw, k_max))
    return _GOLD[case]


def closure_jacobian(V, den, box):
    """B_kl = 2 c phi dV (V_kl - sum V_kl n dV / N) with phi = sqrt(den): what the goldens store"""
    dV = abs(np.linalg.det(box)) / den.size
    n_elec = den.sum() * dV
    chi = np.sqrt(den)
    c = n_elec / ((chi * chi).sum() * dV)
    return np.stack([2 * c * chi * dV * (v - (v * den).sum() * dV / n_elec) for v in V])


def engine_for_key(shape, box, key):
    term, ab = EC.TERMS[key]
    params = dict(wt_alpha=ab[0], wt_beta=ab[1]) if ab else None
    return Engine(shape, DEV).set_cell(box).set_terms([term], params), term, ab


# ------------------------------------------------------------------------------- 1: the entries against the goldens
@pytest.mark.parametrize('case', EC.CASES)
def test_fixed_chi_strain_hessians_match_the_reference_goldens(case):
    """every W2^0_t against torch.autograd.functional.hessian of the reference functional in eps at the seeded chi.  Measured on
    an MI355X, b / a16: ion_electron 9.9e-13 / 1.1e-12, hartree 8.0e-16 / 1.3e-15, tf 3.4e-16 / 5.8e-16, vw 6.7e-16 / 4.0e-16,
    wt_nl 1.9e-15 / 2.8e-15, non_local_KEF(0.7, 0.9) 3.3e-15 / 3.8e-15, lda_x 1.4e-15 / 1.6e-15, pz_c 1.8e-15 / 2.7e-15,
    pw_c 2.2e-15 / 5.5e-15, chachiyo_c 3.3e-15 / 5.8e-16 of max|W2|."""
    g, box, shape, frac, den, tab = gold(case)
    d = {}
    for key in EC.TERMS:
        eng, term, _ab = engine_for_key(shape, box, key)
        if term == 'ion_electron':
            w = ions.ion_electron_strain_hessian(eng, box, dev_t(den), [(frac, tab)])
        else:
            w = eng.strain_hessian(dev_t(den))[term]
        eng.close()
        d[key] = rel(w, g['w2_' + key])
    print('MEASURE elastic %s W2: %s' % (case, ' '.join('%s %.2e' % kv for kv in d.items())))
    for key, v in d.items():
        assert v <= bound(DOUBLE_DEV['w2'][case][key]), key


@pytest.mark.parametrize('case', EC.CASES)
def test_strain_gradient_fields_match_the_reference_goldens(case):
    """the six fields V_kl = v_eps,kl - delta_kl hv(n, n), as the Jacobian B_kl of the closure gradient in eps: the summed
    seven-term set on both cases, and on a16 each term with an explicit part on its own; the transform count"""
    g, box, shape, frac, den, tab = gold(case)
    eng = Engine(shape, DEV).set_cell(box).set_terms(TERMS)
    b = elastic.HipElasticBackend(eng, box, [(frac, tab)])
    V = b.potential_strain_gradient(dev_t(den)).cpu().numpy()
    eng.potential_strain_gradient(dev_t(den))
    ffts = int(eng.query(N.Q_FFT_COUNT))
    b.close()
    eng.close()
    d = {'sum': rel(closure_jacobian(V, den, box), g['b_sum'])}
    if case == 'a16':
        gb = np.load(os.path.join(GOLDEN, 'elastic_a16_b.npz'))
        for t in EC.EXPLICIT:
            e1 = Engine(shape, DEV).set_cell(box).set_terms([t])
            if t == 'ion_electron':
                V = ions.ionic_potential_strain_gradient(e1, box, [(frac, tab)])
            else:
                V = e1.potential_strain_gradient(dev_t(den))
                V[:3] -= e1.hessian_vector(dev_t(den), dev_t(den))
            e1.close()
            d[t] = rel(closure_jacobian(V.cpu().numpy(), den, box), gb['b_' + t])
    print('MEASURE elastic %s B: %s  transforms %d' % (case, ' '.join('%s %.2e' % kv for kv in d.items()), ffts))
    assert ffts == 3 + 18                      # hartree + vw + wt_nl with alpha = beta
    assert d.pop('sum') <= bound(DOUBLE_DEV['b_sum'][case])
    for t, v in d.items():
        assert v <= bound(DOUBLE_DEV['b'][t]), t


def test_strain_gradient_with_two_convolution_families_and_the_transform_counts():
    """alpha != beta (0.7, 0.9): the second power in the head kernel, the fourth family of spectra, both coefficients of the
    combine.  The nonlocal term alone as B_kl against the reference's Jacobian on a16 (bound: ten times the double's 2.87e-15),
    hartree + vw + wt_nl against tests/elastic_double.py on the (20, 18, 33) triclinic grid, and the transform counts: 4 + 24
    for the three terms, 6 inverse for the ionic entry.  Measured on an MI355X: B 2.84e-15 of max|B|, fields 7.72e-14 of their
    maximum; 14, 28 and 6 transforms."""
    g, box, shape, frac, den, tab = gold('a16')
    al, be = EC.AB2
    par = dict(wt_alpha=al, wt_beta=be)
    eng = Engine(shape, DEV).set_cell(box).set_terms(['wt_nl'], par)
    V = eng.potential_strain_gradient(dev_t(den))
    ffts1 = int(eng.query(N.Q_FFT_COUNT))
    V[:3] -= eng.hessian_vector(dev_t(den), dev_t(den))
    eng.close()
    d = rel(closure_jacobian(V.cpu().numpy(), den, box), g['b_nl_0709'])
    box2, shape2, den2, ions_ = EC.grid_inputs('g20t')
    terms = ['hartree', 'vw', 'wt_nl']
    eng = Engine(shape2, DEV).set_cell(box2).set_terms(terms, par)
    V2 = eng.potential_strain_gradient(dev_t(den2))
    ffts3 = int(eng.query(N.Q_FFT_COUNT))
    _g, tab2 = grid_gold()
    species = [(fr, (tab2[0], s * tab2[1], s * tab2[2])) for fr, s in ions_]
    ions.ionic_potential_strain_gradient(eng, box2, species[:1])
    ffts_ion = int(eng.query(N.Q_FFT_COUNT)) - ffts3
    eng.close()
    d2 = rel(V2.cpu().numpy(), ED.potential_strain_gradient(box2, den2, terms, al, be))
    print('MEASURE elastic alpha != beta: B a16 %.2e  v_eps - double on (20, 18, 33) %.2e  transforms %d / %d / ionic %d' % (d, d2, ffts1, ffts3, ffts_ion))
    assert ffts1 == 2 + 12 and ffts3 == 4 + 24 and ffts_ion == 6
    assert d <= bound(DOUBLE_DEV['b']['nl_0709']) and d2 <= bound(FIELD_DEV)


# deviation of the numpy double from the goldens of the further grids (tests/golden/elastic_grids.npz), per grid and term
GRID_DEV = {
    'g17': {'ion_electron': 1.9e-12, 'hartree': 3.29e-15, 'tf': 6.52e-16, 'vw': 1.48e-15, 'wt_nl': 3.76e-14, 'lda_x': 3.63e-16, 'pw_c': 3.23e-15},
    'g48t': {'ion_electron': 2.82e-12, 'hartree': 1.13e-15, 'tf': 8e-16, 'vw': 7.52e-15, 'wt_nl': 1.21e-14, 'lda_x': 1.13e-15, 'pw_c': 2.36e-15},
    'g32x': {'ion_electron': 7.87e-12, 'hartree': 3.06e-15, 'tf': 3.91e-16, 'vw': 1.69e-14, 'wt_nl': 5.96e-15, 'lda_x': 9.79e-16, 'pw_c': 3.53e-15},
    'g20t': {'ion_electron': 3.16e-12, 'hartree': 8.47e-16, 'tf': 1.23e-16, 'vw': 1.16e-14, 'wt_nl': 2.02e-14, 'lda_x': 2.26e-15, 'pw_c': 2.55e-15},
    'g33': {'ion_electron': 4.35e-12, 'hartree': 2.55e-15, 'tf': 6.51e-16, 'vw': 2.36e-14, 'wt_nl': 4.53e-15, 'lda_x': 1.52e-15, 'pw_c': 2.5e-15},
}
# the fields have no golden on these grids: the larger of the two cases' figures for the summed field stands in
FIELD_DEV = max(DOUBLE_DEV['b_sum'].values())
_GRIDS = {}


def grid_gold():
    if not _GRIDS:
        _GRIDS['g'] = np.load(os.path.join(GOLDEN, 'elastic_grids.npz'))
        raw, k_max = EC.recpot()
        _GRIDS['tab'] = ions.recpot_table(raw, k_max)
    return _GRIDS['g'], _GRIDS['tab']


@pytest.mark.parametrize('name', list(EC.GRIDS))
def test_entries_on_other_grids(name):
    """a chirp-z extent (17^3), a mixed-radix extent in a triclinic cell (48, 16, 16), unequal powers of two (32, 16, 64), and two
    grids with an odd last extent and more k-points than one trip of the moment kernels' block loops, (20, 18, 33) and (32, 32, 33);
    ions of two species.  Every W2^0_t against the reference's autograd (tests/golden/elastic_grids.npz), bound per grid and term;
    the fields against tests/elastic_double.py; the reduction entries twice: bitwise equal.  Measured on an MI355X, in the order
    of the grids: ion_electron 2.7 / 1.5 / 6.4 / 1.8 / 2.9 e-12, hartree 1.3 / 1.5 / 2.8 / 1.2 / 1.4 e-15, tf 6.5 / 4.3 / 6.5 / 2.5 / 3.9 e-16,
    vw 6.3 / 9.7 / 3.4 / 5.8 / 3.8 e-16, wt_nl 35 / 1.7 / 4.8 / 1.9 / 2.9 e-15, lda_x 0.5 / 0.8 / 0.9 / 1.3 / 2.0 e-15, pw_c 1.6 / 2.0 / 3.1 / 2.4 / 3.5 e-15;
    v_eps against the double 5.3 / 8.1 / 2.6 / 7.6 / 13 e-14, the ionic field 10 / 4.5 / 5.3 / 5.1 / 5.7 e-14."""
    g, tab = grid_gold()
    box, shape, den, ions_ = EC.grid_inputs(name)
    assert abs(cases.checksum(box, den, *[fr for fr, _s in ions_]) - float(g['checksum_' + name])) < 1e-9
    species = [(fr, (tab[0], s * tab[1], s * tab[2])) for fr, s in ions_]
    terms = list(EC.GRID_TERMS)
    eng = Engine(shape, DEV).set_cell(box).set_terms(terms)
    n = dev_t(den)
    W = eng.strain_hessian(n)
    W['ion_electron'] = ions.ion_electron_strain_hessian(eng, box, n, species)
    again = eng.strain_hessian(n)
    again['ion_electron'] = ions.ion_electron_strain_hessian(eng, box, n, species)
    V = eng.potential_strain_gradient(n)
    Vi = ions.ionic_potential_strain_gradient(eng, box, species)
    V2 = eng.potential_strain_gradient(n)
    eng.close()
    d = {t: rel(W[t], g['w2_%s_%s' % (name, t)]) for t in terms}
    dv = rel(V.cpu().numpy(), ED.potential_strain_gradient(box, den, terms[1:]))
    dvi = rel(Vi.cpu().numpy(), sum(ED.ionic_potential_strain_gradient(box, shape, f, tb) for f, tb in species))
    print('MEASURE elastic grid %s %s: W2 %s  v_eps - double %.2e  ionic - double %.2e'
          % (name, shape, ' '.join('%s %.2e' % kv for kv in d.items()), dv, dvi))
    for t, v in d.items():
        assert v <= bound(GRID_DEV[name][t]), t
    assert dv <= bound(FIELD_DEV) and dvi <= bound(DOUBLE_DEV['b']['ion_electron'])
    assert all(np.array_equal(W[t], again[t]) for t in W) and torch.equal(V, V2)


def test_table_derivatives_beyond_the_table_end():
    """the first and second derivative of the table interpolant (csrc/kpoint.h: recpot<1>, recpot<2>) on both sides of the table
    end, where they change from the Hermite forms to zero slope and curvature plus the Coulomb tail: the (18, 20, 16) triclinic
    cell of tools/geometry_entries_digest.py with its thinned table (every other point, half the charge) and one species of 2
    ions.  That table ends at |k| = 30 and the cell's largest |k| is 13.4, so a prefix of 1251 points (|k| <= 7.5) is used: 47 %
    of the half spectrum lies beyond it and 53 % inside, asserted here.  Against tests/elastic_double.py with the bounds of
    test_entries_on_other_grids for these two entries; the W2 bound there is per grid, and the smallest of them (17^3, the grid
    nearest in size) is taken.  Measured on an MI355X: W2 2.56e-13 of max|W2|, the field 1.79e-14 of its maximum."""
    g = np.load(os.path.join(GOLDEN, 'ions.npz'))
    full = ions.recpot_table(g['recpot_raw'], float(g['recpot_kmax']))
    tab = (full[0][::2][:1251], 0.5 * full[1][::2][:1251], 0.5 * full[2])
    shape = (18, 20, 16)
    box = g['a_box'][0, 0] * np.array([[1.0, 0.0, 0.0], [0.1, 1.1, 0.0], [0.05, -0.1, 0.9]])
    rng = np.random.default_rng(17)
    rng.random((1, 3))
    frac = rng.random((2, 3)) * 1.5 - 0.25
    kabs = np.sqrt(ED._half_spectrum(box, shape)[1])
    beyond, inside = float((kabs > tab[0][-1]).mean()), float((kabs < tab[0][-1]).mean())
    den = synth.smooth_density(shape, seed=10, n0=0.03, amp=0.5)
    eng = Engine(shape, DEV).set_cell(box).set_terms(['ion_electron'])
    W = ions.ion_electron_strain_hessian(eng, box, dev_t(den), [(frac, tab)])
    V = ions.ionic_potential_strain_gradient(eng, box, [(frac, tab)])
    eng.close()
    dw = rel(W, ED.ion_electron(box, den, frac, tab))
    dv = rel(V.cpu().numpy(), ED.ionic_potential_strain_gradient(box, shape, frac, tab))
    print('MEASURE elastic table end: beyond %.3f inside %.3f  W2 - double %.2e  ionic field - double %.2e' % (beyond, inside, dw, dv))
    assert beyond >= 0.25 and inside >= 0.25
    assert dw <= bound(min(d['ion_electron'] for d in GRID_DEV.values()))
    assert dv <= bound(DOUBLE_DEV['b']['ion_electron'])


@pytest.mark.parametrize('case', EC.CASES)
def test_ion_ion_strain_hessian_matches_the_double_and_is_bitwise_reproducible(case):
    """against tests/elastic_double.ion_ion (itself pinned to central differences of the oracle stress, tests/test_elastic_cpu.py),
    at the default cutoff and at Rc = 40 bohr.  The device sums the same M <= 2e4 pair tensors per block as the double in another
    order, with the device's erfc and exp: M eps of the maximum in the worst case (the bound of the ion-ion Hessian test).
    Measured on an MI355X, b / a16: 8.6e-14 / 4.0e-13 of max|W2| at the default cutoff (Rc = 40 bohr: 1.2e-14 / 2.6e-14)."""
    _g, box, shape, frac, _den, tab = gold(case)
    z = np.full(frac.shape[0], float(tab[2]))
    eng = Engine(shape, DEV).set_cell(box)
    W = ions.ion_ion_strain_hessian(eng, box, frac, z)
    again = ions.ion_ion_strain_hessian(eng, box, frac, z)
    Wc = ions.ion_ion_strain_hessian(eng, box, frac, z, Rc=40.0)
    eng.close()
    d, dc = rel(W, ED.ion_ion(box, frac, z)), rel(Wc, ED.ion_ion(box, frac, z, Rc=40.0))
    asym = float(np.abs(W - W.transpose(2, 3, 0, 1)).max() / np.abs(W).max())
    print('MEASURE elastic ion-ion %s: double %.2e (Rc = 40: %.2e) pair asymmetry %.2e' % (case, d, dc, asym))
    assert np.array_equal(W, again)
    assert d <= 2e4 * 2.0 ** -52 and dc <= 2e4 * 2.0 ** -52 and asym == 0.0


# ------------------------------------------------------------------------------- 3: end to end
# Solves stopped at |r| <= rtol |b| leave |dx| / |x| <= kappa rtol with kappa ~ (2 * 100 / ln(2 / rtol))^2 = 60 for ~100 iterations
# to rtol = 1e-11 (the argument of tests/test_force_constants_gpu.py), on a response part of 2.9 Ha against max|W2| of 10 Ha:
# 60 * 1e-11 * 0.3 = 2e-10 of max|W2|, and the same of max|C| (C is W2 / vol plus stress terms both drivers share).  Every
# comparison with the double is capped at 1e-10, so that is the bound.
SOLVE_BOUND = min(60 * RTOL * 0.3, CAP)
FD_EPS = 1e-3
FD_COLUMN = (1, 2)
# ten times the reference-only (numpy-driven, tests/elastic_double.NumpyElasticBackend) figures of the same differences at the same
# step: 5.96e-5 of max|C| for the column yz, 2.53e-4 of K: truncation of the difference, whose coefficient is large here
# (tests/test_elastic_cpu.py scans the step of the corresponding energy difference: 230 - 710 h^2 of max|W2|).
FD_COLUMN_BOUND = 10 * 5.96e-5
FD_BULK_BOUND = 10 * 2.53e-4
_RUN = {}


def a16():
    box, shape, frac, _den, raw, k_max = EC.make_inputs('a16')
    tab = ions.recpot_table(raw, k_max)
    return box, shape, frac, tab, np.full(frac.shape[0], float(tab[2]))


def relaxed(box, chi0=None):
    """truncated-Newton ground state of the a16 ions (fixed fractional coordinates) in the cell `box` -> chi, density"""
    _box, shape, frac, tab, z = a16()
    eng = Engine(shape, DEV).set_cell(box)
    vext = ions.ionic_potential(eng, box, [(frac, tab)])
    eng.set_terms(TERMS)
    r = optimize.optimize_density(eng, float(z.sum()), vext, chi0=chi0, volume=abs(np.linalg.det(box)), n_method='TN')
    eng.close()
    assert r['converged']
    return r['chi'], r['den']


def native_stress(box, den):
    """Engine.stress + ion_electron_stress + the ion-ion stress, on the device"""
    _box, shape, frac, tab, z = a16()
    eng = Engine(shape, DEV).set_cell(box).set_terms(TERMS)
    sig = sum(eng.stress(den).values()) + ions.ion_electron_stress(eng, box, den, [(frac, tab)]) + ions.ion_ion(eng, box, frac, z)[2]
    eng.close()
    return sig


def run():
    """ground state and elastic constants of the a16 case; run once and shared"""
    if not _RUN:
        box, shape, frac, tab, _z = a16()
        chi, _den = relaxed(box)
        eng = Engine(shape, DEV).set_cell(box).set_terms(TERMS)
        _RUN.update(chi=chi, eng=eng, r=elastic.elastic_constants(eng, box, [(frac, tab)], chi, rtol=RTOL))
    return _RUN


def test_elastic_constants_match_the_numpy_driven_tensor():
    """the same driver on tests/elastic_double.NumpyElasticBackend at the device's ground state: C, W2 and its parts; every solve
    converged; W2 is symmetric under (mn) <-> (pq) as a second derivative is.  The 6 x 6 matrix itself is NOT symmetric to the
    solve bound here, and is not meant to be: the cell is not at equilibrium, and Birch coefficients C_ijkl = d sigma_ij / d eps_kl
    under an anisotropic stress differ from C_klij by terms of the size of the stress differences (C_1122 - C_2211 =
    sigma_22 - sigma_11 already) -- 8.9e-3 of max|C| here, in the reference's own recipe applied at fixed chi
    (tests/golden/elastic_a16.npz, cfix4) as in this driver.  `symmetry_residual` is therefore compared with the numpy-driven
    run, like C, and the symmetry that a second derivative has is asserted on W2.
    Measured on an MI355X: max|C| 3.9159e-3 Ha/b3; C - numpy 2.05e-11, W2 - numpy 2.05e-11 of max|W2| (fixed chi 1.97e-11, ion-ion 9.9e-13,
    response 2.2e-14); W2 pair asymmetry 1.51e-12; symmetry_residual 8.870e-3 (numpy: the same); six solves of 100 iterations (numpy: the
    same), 600 products; max|g|/dV 2.3e-11; K 2.832627e-3 Ha/b3 at P 5.17e-5."""
    box, shape, frac, tab, _z = a16()
    r = run()['r']
    ref = elastic.elastic_constants(None, box, [(frac, tab)], run()['chi'].cpu().numpy(), rtol=RTOL,
                                    backend=ED.NumpyElasticBackend(box, shape, [(frac, tab)], TERMS))
    dC, dC4 = rel(r['C'], ref['C']), rel(r['C4'], ref['C4'])
    scale = float(np.abs(ref['W2']).max())
    dW = float(np.abs(r['W2'] - ref['W2']).max() / scale)
    dparts = {'ion_ion': float(np.abs(r['parts']['ion_ion'] - ref['parts']['ion_ion']).max() / scale),
              'response': float(np.abs(r['parts']['response'] - ref['parts']['response']).max() / scale),
              'fixed_chi': max(float(np.abs(r['parts']['fixed_chi'][t] - ref['parts']['fixed_chi'][t]).max()) for t in TERMS) / scale}
    pair = float(np.abs(r['W2'] - r['W2'].transpose(2, 3, 0, 1)).max() / scale)
    print('MEASURE elastic a16: max|C| %.4e Ha/b3  C - numpy %.2e (C4 %.2e)  W2 - numpy %.2e (%s)  W2 pair asymmetry %.2e  '
          'symmetry_residual %.3e (numpy %.3e)  iterations %d..%d (numpy %d..%d) products %d  max|g|/dV %.2e  K %.6e P %.3e'
          % (np.abs(ref['C']).max(), dC, dC4, dW, ' '.join('%s %.2e' % kv for kv in dparts.items()), pair, r['symmetry_residual'],
             ref['symmetry_residual'], min(r['iterations']), max(r['iterations']), min(ref['iterations']), max(ref['iterations']),
             r['hvp_count'], r['ground_state_gradient'], r['bulk_modulus'], r['pressure']))
    assert r['C'].shape == (6, 6) and r['C4'].shape == (3, 3, 3, 3) and len(r['reason']) == 6
    assert all(x == optimize.CG_CONVERGED for x in r['reason']) and max(r['rel_residual']) <= RTOL
    assert r['ground_state_gradient'] < 1e-8 and r['hvp_count'] >= sum(r['iterations'])
    assert dC <= SOLVE_BOUND and dC4 <= SOLVE_BOUND and dW <= SOLVE_BOUND and pair <= SOLVE_BOUND
    assert abs(r['symmetry_residual'] - ref['symmetry_residual']) <= SOLVE_BOUND
    assert np.array_equal(r['C'], r['C'].T)
    assert np.array_equal(sum(r['parts']['fixed_chi'].values()) + r['parts']['ion_ion'] + r['parts']['response'], r['W2'])


def test_bulk_modulus_is_the_tensor_identity_and_the_wrapper():
    """K = (sum_ik W2[i,i,k,k] + 6 vol P) / (9 vol), P = -tr(W1) / (3 vol), to rounding; GPa by the reference's factor"""
    box, _shape, frac, tab, _z = a16()
    s = run()
    r = s['r']
    vol = abs(np.linalg.det(box))
    P = -np.trace(r['stress']) / 3.0
    K = (np.einsum('iikk->', r['W2']) + 6.0 * vol * P) / (9.0 * vol)
    print('MEASURE elastic a16 bulk: K %.10e identity %.10e P %.6e' % (r['bulk_modulus'], K, r['pressure']))
    assert abs(K - r['bulk_modulus']) <= 64 * 2.0 ** -52 * abs(K) and abs(P - r['pressure']) <= 64 * 2.0 ** -52 * abs(P)
    gpa = elastic.bulk_modulus(s['eng'], box, [(frac, tab)], s['chi'], units='GPa', rtol=RTOL)
    assert gpa == r['bulk_modulus'] * (4.3597447222071e-18 / 5.29177210903e-11 ** 3 * 1e-9)


def test_a_column_and_the_bulk_modulus_are_central_differences_between_relaxed_ground_states():
    """C4[:, :, k, l] against (sigma(+) - sigma(-)) / (2 eps) of the total native stress at truncated-Newton ground states
    re-relaxed on the device in the cells h (I +- eps sym(e_kl)), and K against -dP / d ln vol under isotropic scaling,
    eps = 1e-3; bounds: ten times the numpy-driven figures of the same differences.  Measured on an MI355X: column yz 5.955e-5 of
    max|C|, K 2.532e-4 (the numpy-driven run: 5.955e-5 and 2.532e-4)."""
    box, _shape, _frac, _tab, _z = a16()
    s = run()
    r = s['r']
    k, l = FD_COLUMN
    e = np.zeros((3, 3))
    e[k, l] += 0.5
    e[l, k] += 0.5
    sig = {}
    for name, bx in (('c+', box @ (np.eye(3) + FD_EPS * e)), ('c-', box @ (np.eye(3) - FD_EPS * e)), ('v+', box * (1 + FD_EPS)),
                     ('v-', box * (1 - FD_EPS))):
        sig[name] = native_stress(bx, relaxed(bx, chi0=s['chi'])[1])
    d = float(np.abs((sig['c+'] - sig['c-']) / (2 * FD_EPS) - r['C4'][:, :, k, l]).max() / np.abs(r['C4']).max())
    Kfd = (np.trace(sig['v+']) - np.trace(sig['v-'])) / 3.0 / (3.0 * np.log((1 + FD_EPS) / (1 - FD_EPS)))
    dK = abs(Kfd - r['bulk_modulus']) / abs(r['bulk_modulus'])
    print('MEASURE elastic a16 finite differences: column %s %.3e  K %.3e (K %.6e, difference %.6e)' % (FD_COLUMN, d, dK, r['bulk_modulus'], Kfd))
    assert d <= FD_COLUMN_BOUND and dK <= FD_BULK_BOUND


# ------------------------------------------------------------------------------- 4: refusals
def test_pme_unserved_terms_slab_and_fp32_engines_are_refused_by_name():
    from professad_amd.distributed import DistEngine
    box, shape, frac, tab, z = a16()
    chi = torch.ones(shape, dtype=torch.double, device=DEV)
    eng = Engine(shape, DEV).set_cell(box).set_terms(TERMS)
    before = eng.query(N.Q_LAUNCH_COUNT)
    with pytest.raises(NotImplementedError, match='PME'):
        elastic.elastic_constants(eng, box, [(frac, tab)], chi, pme_order=4)
    with pytest.raises(NotImplementedError, match='PME'):
        ions.ionic_potential_strain_gradient(eng, box, [(frac, tab)], pme_order=4)
    with pytest.raises(NotImplementedError, match='PME'):
        ions.ion_electron_strain_hessian(eng, box, chi, [(frac, tab)], pme_order=4)
    assert eng.query(N.Q_LAUNCH_COUNT) == before
    dp = C.POINTER(C.c_double)
    f, ks, v = np.ascontiguousarray(frac), np.ascontiguousarray(tab[0]), np.ascontiguousarray(tab[1])
    out = torch.empty((6,) + tuple(shape), dtype=torch.double, device=DEV)
    w = np.zeros(81)
    rc = eng.lib.ofdft_ionic_potential_strain_gradient(eng._ctx, f.ctypes.data_as(dp), 4, ks.ctypes.data_as(dp), v.ctypes.data_as(dp), ks.size,
                                                       float(tab[2]), 4, C.c_void_p(out.data_ptr()), eng._stream())
    assert rc == N.EINVAL
    with pytest.raises(RuntimeError, match=r'\(-1\).*PME'):
        eng._check(rc, 'ofdft_ionic_potential_strain_gradient')
    rc = eng.lib.ofdft_ion_electron_strain_hessian(eng._ctx, C.c_void_p(chi.data_ptr()), f.ctypes.data_as(dp), 4, ks.ctypes.data_as(dp),
                                                   v.ctypes.data_as(dp), ks.size, float(tab[2]), 4, w.ctypes.data_as(dp), eng._stream())
    assert rc == N.EINVAL
    with pytest.raises(RuntimeError, match=r'\(-1\).*PME'):
        eng._check(rc, 'ofdft_ion_electron_strain_hessian')
    eng.close()
    for name in ('wgc99_nl', 'pbe_x', 'pbe_c', 'gga_k', 'vwgtf', 'nlk'):
        params = dict(nlk_kind=N.NLK_XWM, nlk_p0=0.0) if name == 'nlk' else None
        eng = Engine(shape, DEV).set_cell(box).set_terms(['ion_electron', 'hartree', 'tf', name], params)
        with pytest.raises(NotImplementedError, match=r'\b%s\b' % name):
            elastic.elastic_constants(eng, box, [(frac, tab)], chi)
        with pytest.raises(RuntimeError, match=r'\b%s\b' % name):
            eng.strain_hessian(chi)
        with pytest.raises(RuntimeError, match=r'\b%s\b' % name):
            eng.potential_strain_gradient(chi)
        eng.close()
    de = DistEngine(shape, DEV).set_cell(torch.as_tensor(box)).set_terms(['ion_electron', 'tf'])
    with pytest.raises(NotImplementedError, match='single-GPU'):
        elastic.elastic_constants(de, box, [(frac, tab)], chi)
    de.close()
    e32 = Engine(shape, DEV, dtype=torch.float32).set_cell(box).set_terms(['ion_electron', 'tf'])
    with pytest.raises(NotImplementedError, match='fp64'):
        elastic.elastic_constants(e32, box, [(frac, tab)], chi.float())
    for call in (lambda: e32.strain_hessian(chi.float()), lambda: e32.potential_strain_gradient(chi.float()),
                 lambda: ions.ion_electron_strain_hessian(e32, box, chi.float(), [(frac, tab)])):
        with pytest.raises(NotImplementedError, match='fp64'):
            call()
    # the fp32 library's own entries are stubs that name the fp64 library
    x = np.zeros(81)
    for rc, what in ((e32.lib.ofdft_strain_hessian(e32._ctx, None, x.ctypes.data_as(dp), None), 'ofdft_strain_hessian'),
                     (e32.lib.ofdft_potential_strain_gradient(e32._ctx, None, None, None), 'ofdft_potential_strain_gradient'),
                     (e32.lib.ofdft_ion_ion_strain_hessian(e32._ctx, x.ctypes.data_as(dp), x.ctypes.data_as(dp), 1, 0.0, x.ctypes.data_as(dp), None),
                      'ofdft_ion_ion_strain_hessian')):
        assert rc == N.EINVAL
        with pytest.raises(RuntimeError, match='fp64 library'):
            e32._check(rc, what)
    # plain fp64 work goes to the fp64 sibling
    from professad_amd.engine import engine_for
    e64 = engine_for(shape, e32.device)
    assert np.array_equal(ions.ion_ion_strain_hessian(e32, box, frac, z), ions.ion_ion_strain_hessian(e64, box, frac, z))
    e32.close()
