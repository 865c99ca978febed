"""CPU tests of the elastic constants: the closed forms behind the strain entries (tests/elastic_double.py restates
them in numpy) against the reference's own autograd (tests/golden/elastic_*.npz; generator tests/golden/make_golden_elastic.py),
the Lindhard shape function and its two derivatives against an extended-precision evaluation, the ion-ion strain Hessian against
central differences of the oracle stress, and the host logic of professad_amd.elastic on the numpy backend, end to end against
second differences of re-relaxed energies.  No GPU anywhere; every test prints its figures as `MEASURE ...` before it asserts.

The deviations of the double from the goldens recorded here (DOUBLE_DEV, GRID_DEV) are the reference-only numbers the bounds of
tests/test_elastic_gpu.py derive from (ten times each, capped at 1e-10).
"""
import ctypes
import os
import sys

import mpmath
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import cases  # noqa: E402
import elastic_cases as EC  # noqa: E402
import elastic_double as ED  # noqa: E402
import hvp_double as HD  # noqa: E402
import tn_cases  # noqa: E402
from oracle import ionion  # noqa: E402
from oracle import ions as O  # noqa: E402
from professad_amd import _native as N  # noqa: E402
from professad_amd import elastic, optimize, synth  # noqa: E402

EPS = 2.0 ** -52
CAP = 1e-10
TERMS = list(tn_cases.TERMS)
# measured deviations of the double from the goldens, relative to the maximum of the quantity: per case
DOUBLE_DEV = {
    'w2': {'b': {'ion_electron': 9.31e-13, 'hartree': 9.23e-16, 'tf': 5.07e-16, 'vw': 8.74e-16, 'wt_nl': 7.53e-15, 'nl_0709': 9.86e-15,
                 'lda_x': 2.13e-15, 'pz_c': 3.38e-15, 'pw_c': 3.34e-15, 'chachiyo_c': 5.54e-15},
           'a16': {'ion_electron': 1.97e-12, 'hartree': 1.28e-15, 'tf': 4.20e-16, 'vw': 1.10e-15, 'wt_nl': 5.42e-15, 'nl_0709': 5.99e-15,
                   'lda_x': 1.28e-15, 'pz_c': 2.74e-15, 'pw_c': 5.64e-15, 'chachiyo_c': 1.31e-15}},
    'b_sum': {'b': 7.47e-14, 'a16': 6.43e-14},
    'b': {'ion_electron': 6.81e-14, 'hartree': 8.29e-16, 'vw': 1.63e-14, 'wt_nl': 3.47e-15, 'nl_0709': 2.87e-15},      # a16
}
GRID_DEV = {
    'g17': {'ion_electron': 1.9e-12, 'hartree': 3.29e-15, 'tf': 6.52e-16, 'vw': 1.48e-15, 'wt_nl': 3.76e-14, 'lda_x': 3.63e-16, 'pw_c': 3.23e-15},
    'g48t': {'ion_electron': 2.82e-12, 'hartree': 1.13e-15, 'tf': 8e-16, 'vw': 7.52e-15, 'wt_nl': 1.21e-14, 'lda_x': 1.13e-15, 'pw_c': 2.36e-15},
    'g32x': {'ion_electron': 7.87e-12, 'hartree': 3.06e-15, 'tf': 3.91e-16, 'vw': 1.69e-14, 'wt_nl': 5.96e-15, 'lda_x': 9.79e-16, 'pw_c': 3.53e-15},
    'g20t': {'ion_electron': 3.16e-12, 'hartree': 8.47e-16, 'tf': 1.23e-16, 'vw': 1.16e-14, 'wt_nl': 2.02e-14, 'lda_x': 2.26e-15, 'pw_c': 2.55e-15},
    'g33': {'ion_electron': 4.35e-12, 'hartree': 2.55e-15, 'tf': 6.51e-16, 'vw': 2.36e-14, 'wt_nl': 4.53e-15, 'lda_x': 1.52e-15, 'pw_c': 2.5e-15},
}
# A recorded deviation is a handful of roundings of one FFT library and one BLAS; another build of either may move it.  The double
# is held to four times the record and to the cap of the GPU bounds, so that ten times the record stays a bound the double meets.
SLACK = 4.0


def rel(a, ref):
    return float(np.abs(np.asarray(a) - ref).max() / np.abs(ref).max())


def gold(case):
    g = np.load(os.path.join(HERE, 'golden', 'elastic_%s.npz' % case))
    box, shape, frac, den, raw, k_max = EC.make_inputs(case)
    assert cases.checksum(box, frac, den, raw) == pytest.approx(float(g['checksum']), rel=1e-12)       # generator drift
    return g, box, shape, frac, den, O.recpot_table(raw, k_max)


def closure_jacobian(V, den, box):
    """B_kl = 2 c phi dV (V_kl - sum V_kl n dV / N) with phi = sqrt(den)"""
    dV = abs(np.linalg.det(box)) / den.size
    n_elec = den.sum() * dV
    chi = np.sqrt(den)
    c = n_elec / ((chi * chi).sum() * dV)
    return np.stack([2 * c * chi * dV * (v - (v * den).sum() * dV / n_elec) for v in V])


# ------------------------------------------------------------------------------- 1: the double against the reference's autograd
@pytest.mark.parametrize('case', EC.CASES)
def test_fixed_chi_strain_hessians_match_the_reference_autograd(case):
    """W2^0_t of every term against torch.autograd.functional.hessian of the reference functional in eps.  Measured b / a16:
    ion_electron 9.3e-13 / 2.0e-12, hartree 9.2e-16 / 1.3e-15, tf 5.1e-16 / 4.2e-16, vw 8.7e-16 / 1.1e-15, wt_nl 7.5e-15 / 5.4e-15,
    non_local_KEF(0.7, 0.9) 9.9e-15 / 6.0e-15, lda_x 2.1e-15 / 1.3e-15, pz_c 3.4e-15 / 2.7e-15, pw_c 3.3e-15 / 5.6e-15,
    chachiyo_c 5.5e-15 / 1.3e-15.  (The ion-electron figure carries the second derivative of the cubic-Hermite table: 1 / dk^2.)"""
    g, box, _shape, frac, den, tab = gold(case)
    d = {}
    for key, (term, ab) in EC.TERMS.items():
        if term == 'ion_electron':
            w = ED.ion_electron(box, den, frac, tab)
        else:
            w = ED.term(box, den, term, *(ab or ()))
        d[key] = rel(w, g['w2_' + key])
        assert rel(w, w.transpose(2, 3, 0, 1)) <= 64 * EPS
    print('MEASURE elastic double %s W2: %s' % (case, ' '.join('%s %.2e' % kv for kv in d.items())))
    for key, v in d.items():
        assert v <= min(SLACK * DOUBLE_DEV['w2'][case][key], CAP), key


@pytest.mark.parametrize('name', list(EC.GRIDS))
def test_fixed_chi_strain_hessians_on_the_further_grids(name):
    """the grids of the GPU suite that have no full golden, ions of two species: the figures stand in GRID_DEV"""
    g = np.load(os.path.join(HERE, 'golden', 'elastic_grids.npz'))
    tab = O.recpot_table(*EC.recpot())
    box, _shape, den, ions_ = EC.grid_inputs(name)
    assert cases.checksum(box, den, *[fr for fr, _s in ions_]) == pytest.approx(float(g['checksum_' + name]), rel=1e-12)
    species = [(fr, (tab[0], s * tab[1], s * tab[2])) for fr, s in ions_]
    d = {}
    for t in EC.GRID_TERMS:
        w = sum(ED.ion_electron(box, den, f, tb) for f, tb in species) if t == 'ion_electron' else ED.term(box, den, t)
        d[t] = rel(w, g['w2_%s_%s' % (name, t)])
    print('MEASURE elastic double grid %s W2: %s' % (name, ' '.join('%s %.2e' % kv for kv in d.items())))
    for t, v in d.items():
        assert v <= min(SLACK * GRID_DEV[name][t], CAP), t


@pytest.mark.parametrize('case', EC.CASES)
def test_strain_gradient_fields_match_the_reference_autograd(case):
    """V_kl = v_eps,kl - delta_kl hv(n, n) as the Jacobian of the closure gradient in eps, for the summed seven-term set and, on
    a16, for each term with an explicit part.  Measured b / a16: sum 7.5e-14 / 6.4e-14; a16 per term: ion_electron 6.8e-14,
    hartree 8.3e-16, vw 1.6e-14, wt_nl 3.5e-15, non_local_KEF(0.7, 0.9) 2.9e-15."""
    g, box, shape, frac, den, tab = gold(case)
    be = ED.NumpyElasticBackend(box, shape, [(frac, tab)], TERMS)
    d = {'sum': rel(closure_jacobian(be.potential_strain_gradient(den), den, box), g['b_sum'])}
    if case == 'a16':
        gb = np.load(os.path.join(HERE, 'golden', 'elastic_a16_b.npz'))
        for t in EC.EXPLICIT:
            if t == 'ion_electron':
                V = ED.ionic_potential_strain_gradient(box, shape, frac, tab)
            else:
                V = ED.potential_strain_gradient(box, den, [t])
                V[:3] -= HD.term_hv(box, den, den, t)
            d[t] = rel(closure_jacobian(V, den, box), gb['b_' + t])
        al, be = EC.AB2                      # the alpha != beta instance of the nonlocal term alone
        V = ED.potential_strain_gradient(box, den, ['wt_nl'], al, be)
        V[:3] -= HD.term_hv(box, den, den, 'wt_nl', al, be)
        d['nl_0709'] = rel(closure_jacobian(V, den, box), g['b_nl_0709'])
    print('MEASURE elastic double %s B: %s' % (case, ' '.join('%s %.2e' % kv for kv in d.items())))
    assert d.pop('sum') <= min(SLACK * DOUBLE_DEV['b_sum'][case], CAP)
    for t, v in d.items():
        assert v <= min(SLACK * DOUBLE_DEV['b'][t], CAP), t


# ------------------------------------------------------------------------------- 2: the two conversion identities
@pytest.mark.parametrize('case', EC.CASES)
def test_the_reference_recipe_and_the_bulk_modulus_follow_from_w2_and_w1(case):
    """D[i,j,k,l] = W2[j,i,l,k] + W1[l,i] delta_jk, C = (D_ijkl + D_ijlk) / (2 vol) - sigma_ij delta_kl against the reference's own
    recipe (system.py:1281-1337) applied by autograd at fixed chi, from the reference's W2 and W1 alone: 2.0e-15 / 9.8e-16 of max|C|
    (b / a16).  K = vol d2E/dvol2 against the second derivative of E along the isotropic strain, which is sum_ik W2[i,i,k,k] by
    the chain rule: the identity is exact in exact arithmetic, here to a few roundings of the sums."""
    g, box, _shape, _frac, _den, _tab = gold(case)
    vol = abs(np.linalg.det(box))
    W2 = sum(g['w2_' + t] for t in EC.SUMMED)
    W1 = g['w1_sum']
    C4 = elastic.tensor_from_w2(W2, W1, vol)
    d = rel(C4, g['cfix4'])
    ds = float(np.abs(W1.T / vol - g['stress_sum']).max() / np.abs(g['stress_sum']).max())
    K, P = elastic.bulk_from_w2(W2, W1, vol)
    # E(vol (1 + e)^3): d2E/de2 = 9 vol^2 E'' + 6 vol E', dE/de = 3 vol E'
    d2e, d1e = np.einsum('iikk->', W2), np.trace(W1)
    K_direct = vol * (d2e - 2.0 * d1e) / (9.0 * vol * vol)
    dK = abs(K - K_direct) / abs(K_direct)
    C, sym = elastic.voigt_matrix(C4)
    print('MEASURE elastic conversion %s: C recipe %.2e  stress %.2e  K identity %.2e  asymmetry of the 6 x 6 matrix %.3e' % (case, d, ds, dK, sym))
    assert d <= 64 * EPS and ds <= 64 * EPS and dK <= 64 * EPS
    assert P == pytest.approx(-np.trace(g['stress_sum']) / 3.0, rel=1e-13)
    assert np.array_equal(C, C.T) and C[0, 3] == C4[0, 0, 1, 2] and C[3, 5] == C4[1, 2, 0, 1] and C[4, 4] == C4[0, 2, 0, 2]


def test_moduli_and_units_follow_the_reference_formulas():
    """Voigt / Reuss / Poisson on an isotropic matrix, where every average is the input; the unit factors of system.py:27-33"""
    K0, G0 = 0.003, 0.001
    lam = K0 - 2.0 * G0 / 3.0
    C = np.zeros((6, 6))
    C[:3, :3] = lam
    C[np.arange(3), np.arange(3)] = lam + 2.0 * G0
    C[np.arange(3, 6), np.arange(3, 6)] = G0
    assert elastic.voigt_moduli(C) == pytest.approx((K0, G0), rel=1e-14)
    assert elastic.reuss_moduli(C) == pytest.approx((K0, G0), rel=1e-13)
    assert elastic.shear_average(C) == pytest.approx(G0, rel=1e-13) and elastic.shear_average(C, 'geometric') == pytest.approx(G0, rel=1e-13)
    assert elastic.poissons_ratio(K0, G0) == pytest.approx((3 * K0 - 2 * G0) / (2 * (3 * K0 + G0)), rel=1e-14)
    with pytest.raises(ValueError, match='mean_type'):
        elastic.shear_average(C, 'harmonic')
    assert elastic.unit_factor('Ha/b3') == 1.0
    assert elastic.unit_factor('GPa') == pytest.approx(4.3597447222071e-18 / 5.29177210903e-11 ** 3 * 1e-9, rel=1e-14)      # 29421.0157
    assert elastic.unit_factor('eV/a3') == pytest.approx(27.211386245988 / 0.529177210903 ** 3, rel=1e-12)                # 183.631
    with pytest.raises(ValueError, match='units'):
        elastic.unit_factor('Pa')


# ------------------------------------------------------------------------------- 3: the Lindhard shape function twice differentiated
def test_lindhard_shape_and_its_derivatives_against_extended_precision():
    """F = 1/G - 3 eta^2 - 1, P = eta F', Q = eta^2 F'' as the double and strain2_kernels.h::lindhard_shape_d2 form them (direct
    below eta = 3, the eta^-2 series from 3 on) against 50-digit arithmetic.  Measured absolute errors: eta >= 3 (to 14): F 2.2e-16,
    P 6.9e-18, Q 5.6e-17 -- where the direct form, whose double cancellation is differentiated twice, is off by 4.5e-10 in Q at
    eta = 12; 0.02 <= eta < 3 away from the logarithmic singularity of F' at eta = 1: F 4.3e-14, P 1.8e-13, Q 5.6e-13 of max(1, |Q|)."""
    mpmath.mp.dps = 50

    def Fmp(e):
        e = mpmath.mpf(e)
        return 1 / (mpmath.mpf(1) / 2 + (1 - e * e) / (4 * e) * mpmath.log(abs((1 + e) / (1 - e)))) - 3 * e * e - 1
    lo = np.concatenate([np.linspace(0.02, 0.98, 25), np.linspace(1.02, 2.99, 25)])
    hi = np.linspace(3.0, 14.0, 30)
    err = {}
    for name, etas in (('lo', lo), ('hi', hi)):
        F, P, Q = ED.lindhard_shape_d2(etas)
        ref = np.array([[float(Fmp(e)), float(e * mpmath.diff(Fmp, e)), float(e * e * mpmath.diff(Fmp, e, 2))] for e in etas])
        err[name] = (np.abs(F - ref[:, 0]).max(), np.abs(P - ref[:, 1]).max(), (np.abs(Q - ref[:, 2]) / np.maximum(1.0, np.abs(ref[:, 2]))).max())
    e = np.array([12.0])
    lg = np.log(np.abs((1 + e) / (1 - e)))
    G, Dg = 0.5 + (1 - e * e) / (4 * e) * lg, 0.5 - 0.25 * (e + 1 / e) * lg
    De = -0.25 * (1 - 1 / (e * e)) * lg - 0.5 * (e + 1 / e) / (1 - e * e)
    direct = float(abs((-(e * De - Dg) / G ** 2 + 2 * Dg ** 2 / G ** 3 - 6 * e * e)[0] - float(144 * mpmath.diff(Fmp, 12.0, 2))))
    print('MEASURE elastic lindhard: eta < 3 F %.2e P %.2e Q %.2e;  eta >= 3 F %.2e P %.2e Q %.2e  (direct form, Q at 12: %.2e)'
          % (err['lo'] + err['hi'] + (direct,)))
    assert max(err['hi']) <= 64 * EPS          # no cancellation: a few roundings of numbers of order one
    assert max(err['lo']) <= 5e-12             # the direct form: (1 - eta^2)^-1 amplifies a rounding up to 50 times on this scan
    F1, P1, Q1 = ED.lindhard_shape_d2(np.array([1.0]))
    assert (F1[0], P1[0], Q1[0]) == (-2.0, -6.0, -6.0)          # G is the constant 1/2 of the reference's masked assignment


# ------------------------------------------------------------------------------- 4: ion-ion
@pytest.mark.parametrize('case', EC.CASES)
def test_ion_ion_strain_hessian_matches_central_differences_of_the_oracle_stress(case):
    """three columns of W2 against central differences in eps_pq of dE/d eps = (I + eps)^-T vol(eps) sigma(eps), sigma the oracle
    ion-ion stress at the strained cell with Rd and Rc held at their unstrained values (a pair crossing Rc weighs erfc(6) / Rc ~
    2e-17).  Measured b / a16: 2.7e-4 / 1.6e-4 at 1e-2 falling as the square of the step to 2.7e-8 / 1.6e-8 at 1e-4."""
    box, _shape, frac, _den, raw, k_max = EC.make_inputs(case)
    z = np.full(frac.shape[0], float(O.recpot_table(raw, k_max)[2]))
    W = ED.ion_ion(box, frac, z)
    Rc, Rd = ionion.heuristics(box)

    def grad(eps):
        b = box @ (np.eye(3) + eps)
        return np.linalg.inv(np.eye(3) + eps).T @ (abs(np.linalg.det(b)) * ionion.forces_stress(b, frac @ b, z, Rc, Rd)[1])
    devs = []
    for h in (1e-2, 1e-3, 1e-4):
        dev = 0.0
        for p, q in ((0, 0), (1, 2), (2, 0)):
            e = np.zeros((3, 3))
            e[p, q] = h
            dev = max(dev, float(np.abs((grad(e) - grad(-e)) / (2 * h) - W[:, :, p, q]).max()))
        devs.append(dev / float(np.abs(W).max()))
        print('MEASURE elastic ion-ion fd %s: step %.0e deviation %.2e' % (case, h, devs[-1]))
    # truncation h^2 |W''''| / 6: 2.7 h^2 of max|W2| measured at every step; rounding eps |W1| / h stays below 1e-11
    assert devs[-1] <= 1e-7 and 50 < devs[0] / devs[1] < 200 and 50 < devs[1] / devs[2] < 200
    assert rel(W, W.transpose(2, 3, 0, 1)) <= 64 * EPS


# ------------------------------------------------------------------------------- 5: the driver on the numpy backend
def relax(backend, chi, n_elec):
    tn = optimize.TruncatedNewton(chi, backend.cg, n_elec)
    for _outer in range(14):
        before = tn.total_iter
        tn.step(lambda: backend.closure(chi, n_elec))
        if tn.total_iter == before:
            break
    return tn


@pytest.fixture(scope='module')
def driven():
    """two Al ions in a triclinic cell of 203 bohr^3 on a 6 x 8 x 6 grid, the seven-term set, relaxed by truncated Newton"""
    shape = (6, 8, 6)
    box = synth.triclinic_cell(0.75)
    tab = O.recpot_table(*EC.recpot())
    frac = np.array([[0.1, 0.2, 0.15], [0.6, 0.55, 0.7]])
    species = [(frac, tab)]
    n_elec = 2 * float(tab[2])
    b = ED.NumpyElasticBackend(box, shape, species, TERMS)
    chi = np.full(shape, np.sqrt(n_elec / abs(np.linalg.det(box))))
    relax(b, chi, n_elec)
    r = elastic.elastic_constants(None, box, species, chi, backend=b, rtol=1e-11)
    return dict(box=box, shape=shape, species=species, n_elec=n_elec, chi=chi, backend=b, r=r)


def test_driver_parts_add_up_and_w2_is_a_symmetric_second_derivative(driven):
    """Measured: max|g|/dV 1.5e-15, six solves of 51-52 iterations, W2 (mn) <-> (pq) asymmetry 1e-12 of max|W2| = 3.1 Ha (response
    2.3); the 6 x 6 matrix is 0.10 of max|C| away from symmetric: the cell is far from equilibrium (P = 1.1e-3 Ha/b3, K = 6.0e-3)."""
    r = driven['r']
    W2 = r['W2']
    pair = float(np.abs(W2 - W2.transpose(2, 3, 0, 1)).max() / np.abs(W2).max())
    print('MEASURE elastic driver: max|g|/dV %.2e iterations %d..%d products %d  W2 pair asymmetry %.2e  symmetry_residual %.3e  K %.4e P %.4e'
          % (r['ground_state_gradient'], min(r['iterations']), max(r['iterations']), r['hvp_count'], pair, r['symmetry_residual'],
             r['bulk_modulus'], r['pressure']))
    assert r['ground_state_gradient'] < 1e-7
    assert all(x == optimize.CG_CONVERGED for x in r['reason']) and max(r['rel_residual']) <= 1e-11 and len(r['iterations']) == 6
    # solves stopped at |r| <= rtol |b|: |dx| / |x| <= kappa rtol, kappa ~ (2 * 52 / ln(2 / rtol))^2 = 16 for 52 iterations to 1e-11, on a
    # response part of 2.3 Ha out of max|W2| = 3.1 Ha: 16 * 1e-11 * 0.7 = 1.1e-10, capped like every comparison at 1e-10
    assert pair <= min(16 * 1e-11 * 0.7, CAP)
    assert np.array_equal(sum(r['parts']['fixed_chi'].values()) + r['parts']['ion_ion'] + r['parts']['response'], W2)
    assert set(r['parts']['fixed_chi']) == set(TERMS) and r['hvp_count'] >= sum(r['iterations'])
    vol = abs(np.linalg.det(driven['box']))
    K, P = elastic.bulk_from_w2(W2, vol * r['stress'].T, vol)
    assert K == r['bulk_modulus'] and P == r['pressure']
    assert np.array_equal(r['C'], elastic.voigt_matrix(r['C4'])[0])


def test_w2_is_the_second_difference_of_re_relaxed_energies(driven):
    """A : W2 : A without the ion-ion part against (E(+h A) - 2 E(0) + E(-h A)) / h^2 of the energies re-relaxed in the cells
    box (I +- h A), for three general (non-symmetric) unit directions A over a scan of steps.  Bound: ten times the 3e-5 of
    max|W2| measured with the reference alone (issue).  Measured, worst direction: 2.1e-3 at h = 2e-3, 3.1e-4 at 1e-3, 1.8e-4 at
    5e-4, 1.5e-5 at 2.5e-4, 9.5e-6 at 1.25e-4: the difference falls with the step, as 230 - 710 h^2 -- truncation with a
    coefficient that is large on this cell (a rough density on a 6 x 8 x 6 grid, and a pseudopotential table that is a C1
    interpolant; which of the two makes it large has not been isolated).  At the step 2e-3 it stands seven times above the bound, so
    the two smallest steps are held to the bound and the deviation must not grow as the step shrinks."""
    d = driven
    r = d['r']
    W2e = r['W2'] - r['parts']['ion_ion']
    rng = np.random.default_rng(3)
    dirs = [a / np.linalg.norm(a) for a in rng.standard_normal((3, 3, 3))]

    def energy(bx):
        b = ED.NumpyElasticBackend(bx, d['shape'], d['species'], TERMS)
        chi = d['chi'].copy()
        relax(b, chi, d['n_elec'])
        return b.closure(chi, d['n_elec'])[0]
    E0 = energy(d['box'])
    devs = []
    for h in (2e-3, 1e-3, 5e-4, 2.5e-4, 1.25e-4):
        dev = 0.0
        for A in dirs:
            fd = (energy(d['box'] @ (np.eye(3) + h * A)) - 2 * E0 + energy(d['box'] @ (np.eye(3) - h * A))) / h ** 2
            dev = max(dev, abs(fd - np.einsum('mn,mnpq,pq', A, W2e, A)) / float(np.abs(W2e).max()))
        print('MEASURE elastic driver second difference: step %.3g deviation %.2e  (%.0f h^2)' % (h, dev, dev / h ** 2))
        devs.append(dev)
    assert devs[-1] <= 10 * 3e-5 and devs[-2] <= 10 * 3e-5
    assert all(b <= a for a, b in zip(devs, devs[1:]))


def test_driver_options_units_and_warning(driven):
    d = driven
    gpa = elastic.elastic_constants(None, d['box'], d['species'], d['chi'], backend=d['backend'], rtol=1e-11, units='GPa')
    f = 4.3597447222071e-18 / 5.29177210903e-11 ** 3 * 1e-9                     # system.py:33
    assert np.allclose(gpa['C'], d['r']['C'] * f, rtol=1e-14, atol=0) and gpa['bulk_modulus'] == pytest.approx(d['r']['bulk_modulus'] * f, rel=1e-14)
    assert np.array_equal(gpa['W2'], d['r']['W2'])                               # Ha, never converted
    K = elastic.bulk_modulus(None, d['box'], d['species'], d['chi'], backend=d['backend'], rtol=1e-11)
    assert K == d['r']['bulk_modulus']
    with pytest.warns(UserWarning, match='did not converge'):
        cut = elastic.elastic_constants(None, d['box'], d['species'], d['chi'], backend=d['backend'], maxiter=3)
    assert cut['reason'] == [optimize.CG_MAXITER] * 6
    with pytest.raises(ValueError, match='units'):
        elastic.elastic_constants(None, d['box'], d['species'], d['chi'], backend=d['backend'], units='Pa')


# ------------------------------------------------------------------------------- 6: refusals and the ABI
class _FakeEngine:
    """what elastic.refusal reads of an engine"""

    def __init__(self, terms, dtype=None, comm=None, wts=0.0):
        import torch
        self.dtype = dtype or torch.double
        self.comm = comm
        vals = np.zeros(N.NPARAMS)
        vals[12] = wts
        self._terms_key = (sum(N.TERM_BITS[t] for t in terms), vals.tobytes())

    def _mask(self):
        return self._terms_key[0]


@pytest.mark.parametrize('name', ['wgc99_nl', 'pbe_x', 'pbe_c', 'gga_k', 'vwgtf', 'nlk'])
def test_unserved_terms_are_refused_by_name(name):
    with pytest.raises(NotImplementedError, match=r'\b%s\b' % name):
        elastic.elastic_constants(_FakeEngine(['ion_electron', 'hartree', 'tf', name]), np.eye(3), [(np.zeros((1, 3)), (None, None, 3))], None)


def test_pme_slabs_fp32_and_missing_ion_electron_are_refused_by_name():
    import torch
    sp = [(np.zeros((1, 3)), (None, None, 3))]
    with pytest.raises(NotImplementedError, match='PME'):
        elastic.elastic_constants(_FakeEngine(['ion_electron', 'tf']), np.eye(3), sp, None, pme_order=4)
    with pytest.raises(NotImplementedError, match='single-GPU'):
        elastic.elastic_constants(_FakeEngine(['ion_electron', 'tf'], comm=object()), np.eye(3), sp, None)
    with pytest.raises(NotImplementedError, match='fp64'):
        elastic.elastic_constants(_FakeEngine(['ion_electron', 'tf'], dtype=torch.float32), np.eye(3), sp, None)
    with pytest.raises(NotImplementedError, match='wts_kind'):
        elastic.elastic_constants(_FakeEngine(['ion_electron', 'tf', 'wt_nl'], wts=1.0), np.eye(3), sp, None)
    with pytest.raises(NotImplementedError, match='ion_electron'):
        elastic.elastic_constants(_FakeEngine(['hartree', 'tf']), np.eye(3), sp, None)


@pytest.mark.parametrize('dtype', [N.F64, N.F32])
def test_entry_points_are_exported_and_refuse_null_arguments(dtype):
    """both libraries export the five symbols; a null context is OFDFT_EINVAL in both"""
    lib = N.load(dtype)
    names = ('ofdft_potential_strain_gradient', 'ofdft_ionic_potential_strain_gradient', 'ofdft_strain_hessian',
             'ofdft_ion_electron_strain_hessian', 'ofdft_ion_ion_strain_hessian')
    for name in names:
        assert name in N.EXPORTS and hasattr(lib, name)
    x = (ctypes.c_double * 81)()
    assert lib.ofdft_potential_strain_gradient(None, None, None, None) == N.EINVAL
    assert lib.ofdft_ionic_potential_strain_gradient(None, x, 1, x, x, 2, 3.0, 0, None, None) == N.EINVAL
    assert lib.ofdft_strain_hessian(None, None, x, None) == N.EINVAL
    assert lib.ofdft_ion_electron_strain_hessian(None, None, x, 1, x, x, 2, 3.0, 0, x, None) == N.EINVAL
    assert lib.ofdft_ion_ion_strain_hessian(None, x, x, 1, 0.0, x, None) == N.EINVAL
