"""CPU tests of the force constants: the closed forms behind ofdft_ionic_potential_gradient, ofdft_ion_electron_curvature and
ofdft_ion_ion_hessian (tests/fc_double.py restates them in numpy) against the reference's own autograd
(tests/golden/fc_<case>.npz; generator tests/golden/make_golden_fc.py) and against central differences of the pinned oracle
forces, and the host logic of professad_amd.force_constants on the numpy backend.  No GPU anywhere; every test prints its figures
as `MEASURE ...` before it asserts.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import cases  # noqa: E402
import fc_cases  # noqa: E402
import fc_double as FD  # noqa: E402
import tn_cases  # noqa: E402
import tn_double as T  # noqa: E402
from oracle import ionion  # noqa: E402
from professad_amd import _native as N  # noqa: E402
from professad_amd import optimize  # noqa: E402
from professad_amd.force_constants import force_constants  # noqa: E402
from professad_amd.ions import recpot_table  # noqa: E402

EPS = 2.0 ** -52
# Both sides are fp64 sums over the grid's N_k k-points of terms of one size, transformed by two different FFT libraries:
# between the random-walk sqrt(N_k) eps (2e-14 at 7 680 points) and the worst case N_k eps (1.7e-12).  1e-12 of the maximum.
CLOSED_FORM_BOUND = 1e-12
# Central difference of the oracle forces at step h [bohr]: truncation h^2 |F'''| / 6 against rounding eps max|F| / h.  The pair
# function's derivatives grow by about 1 / r ~ 0.2 / bohr per order at the nearest-neighbour distance, so at h = 1e-3..1e-4 the
# truncation is 1e-8..1e-10 of max|H| and the rounding 1e-12..1e-11: the best step of the scan lies below 1e-8, and an error in the
# closed forms is of order one at every step.
ION_ION_FD_BOUND = 1e-8
# Row sums: the diagonal block adds the very tensors the off-diagonal blocks subtract, so only the order of the additions differs:
# a few roundings of the sum of magnitudes.
SUM_RULE_BOUND = 64 * EPS
# Symmetry: block (p, b) sums T(R_b + s - R_p) and block (b, p) sums T(R_p - s - R_b), the same M <= 2e4 pairs in another order
# with separations rounded at the size of the coordinates: M eps of max|H| in the worst case.
ION_ION_SYMMETRY_BOUND = 2e4 * EPS
# issue: ten times the 2.65e-7 of max|Phi| of the reference-only run at eps = 1e-3 bohr (eps^2 truncation, device independent)
FD_COLUMN_BOUND = 10 * 2.65e-7
FD_EPS = 1e-3
# Symmetry of the assembled matrix: the three parts are symmetric to rounding by themselves but for the response, whose error
# is that of the 12 solves: conjugate gradients stopped at |r| <= rtol |b| leave |dx| / |x| <= kappa rtol, and ~100 iterations to
# rtol = 1e-10 mean kappa ~ (2 * 100 / ln(2 / rtol))^2 = 70.  With the response part ten times max|Phi| (0.456 against 4.6e-2 Ha/bohr^2)
# that is 70 * 1e-10 * 10 = 7e-8 of max|Phi|; the ground state's own residual gradient adds less.
SYMMETRY_BOUND = 1e-7
FD_COLUMN = (2, 1)               # (ion b, direction j) of the finite-difference column
TERMS = list(tn_cases.TERMS)


def gold(case):
    g = np.load(os.path.join(HERE, 'golden', 'fc_%s.npz' % case))
    box, shape, frac, den, raw, k_max = fc_cases.make_inputs(case)
    assert cases.checksum(box, frac, den, raw) == pytest.approx(float(g['checksum']), rel=1e-12)       # generator drift
    return g, box, shape, frac, den, recpot_table(raw, k_max)


# ------------------------------------------------------------------------------- 1: closed forms against the reference's autograd
@pytest.mark.parametrize('case', fc_cases.CASES)
def test_potential_gradient_and_curvature_match_the_reference_autograd(case):
    """the Jacobian of lattice_sum for one ion and the Hessian of IonElectron over it, relative to their maxima.
    Measured b / a16: gradient 3.6e-15 / 5.7e-16, curvature 6.7e-15 / 1.2e-15."""
    g, box, shape, frac, den, tab = gold(case)
    a = int(g['ion'])
    dv = FD.potential_gradient(box, shape, (frac @ box)[a], tab)
    D = FD.ion_electron_curvature(box, den, frac, tab)
    ref = np.stack([g['hess'][p, :, p, :] for p in range(frac.shape[0])])
    d1 = float(np.abs(dv - g['dv']).max() / np.abs(g['dv']).max())
    d2 = float(np.abs(D - ref).max() / np.abs(ref).max())
    print('MEASURE fc double %s: gradient %.2e curvature %.2e' % (case, d1, d2))
    assert d1 <= CLOSED_FORM_BOUND and d2 <= CLOSED_FORM_BOUND
    # the forces the same sums give are the first derivative the golden ions.npz pins elsewhere; here: linear in the density
    F1 = FD.ion_electron_forces(box, den, frac, tab)
    assert np.allclose(FD.ion_electron_forces(box, -2.0 * den, frac, tab), -2.0 * F1, rtol=1e-13, atol=0)


# ------------------------------------------------------------------------------- 2: ion-ion Hessian
def ion_sets():
    out = {}
    for case in fc_cases.CASES:
        box, _shape, frac, _den, raw, k_max = fc_cases.make_inputs(case)
        out[case] = (box, frac, np.full(frac.shape[0], float(recpot_table(raw, k_max)[2])))
    return out


@pytest.mark.parametrize('case', fc_cases.CASES)
def test_ion_ion_hessian_matches_central_differences_of_the_oracle_forces(case):
    """one column (ion 1, every direction) of -dF/dR by central differences of oracle.ionion.forces_stress at fixed Rc, Rd, over a
    scan of steps; the best step is asserted.  Measured b / a16: 4.7e-6 / 5.6e-6 at 1e-2 falling as the square of the step to 4.7e-10 / 5.9e-10 at 1e-4 and 4.6e-11 / 2.1e-10 at 3e-5."""
    box, frac, z = ion_sets()[case]
    n = frac.shape[0]
    H = FD.ion_ion_hessian(box, frac, z, range(n))
    Rc, Rd = ionion.heuristics(box)
    coords = frac @ box
    best = None
    for h in (1e-2, 3e-3, 1e-3, 3e-4, 1e-4, 3e-5):
        dev = 0.0
        for j in range(3):
            step = np.zeros_like(coords)
            step[1, j] = h
            Fp = ionion.forces_stress(box, coords + step, z, Rc, Rd)[0]
            Fm = ionion.forces_stress(box, coords - step, z, Rc, Rd)[0]
            dev = max(dev, float(np.abs(-(Fp - Fm) / (2 * h) - H[:, 1, :, j]).max()))
        dev /= float(np.abs(H).max())
        print('MEASURE fc ion-ion fd %s: step %.0e deviation %.2e' % (case, h, dev))
        best = dev if best is None else min(best, dev)
    assert best <= ION_ION_FD_BOUND


@pytest.mark.parametrize('case', fc_cases.CASES)
def test_ion_ion_hessian_is_symmetric_and_its_rows_sum_to_zero(case):
    """a rigid translation costs nothing at a fixed pair list.  Measured b / a16: row sums 2.2e-17 / 1.3e-18 of the sum of magnitudes
    (each pair's tensor enters the diagonal and the off-diagonal block alike), asymmetry 4.3e-15 / 1.3e-14 of max|H|."""
    box, frac, z = ion_sets()[case]
    n = frac.shape[0]
    H = FD.ion_ion_hessian(box, frac, z, range(n))
    rows = float(np.abs(H.sum(axis=1)).max() / np.abs(H).sum(axis=1).max())
    asym = float(np.abs(H - H.transpose(1, 0, 3, 2)).max() / np.abs(H).max())
    print('MEASURE fc ion-ion %s: row sums %.2e asymmetry %.2e' % (case, rows, asym))
    assert rows <= SUM_RULE_BOUND and asym <= ION_ION_SYMMETRY_BOUND
    assert np.array_equal(FD.ion_ion_hessian(box, frac, z, [2, 0]), H[[2, 0]])
    one = FD.ion_ion_hessian(box, frac[:1], z[:1], [0])
    assert one.shape == (1, 1, 3, 3) and not one.any()


# ------------------------------------------------------------------------------- 3: the driver on the numpy backend
def relax(backend, chi, n_elec):
    """truncated Newton on the numpy backend with the oracle closure, in place; -> the optimiser"""
    tn = optimize.TruncatedNewton(chi, backend.cg, n_elec)
    for _outer in range(12):
        before = tn.total_iter
        tn.step(lambda: backend.closure(chi, n_elec))
        if tn.total_iter == before:          # |g|_2 <= tolerance_grad: the step did nothing
            break
    return tn


def total_forces(backend, box, frac, z, chi, n_elec):
    """F = -dE_tot/dR: ion-electron forces of the density of chi plus the oracle's ion-ion forces"""
    n = T.density(box, chi, n_elec)[2]
    Rc, Rd = ionion.heuristics(box)
    return backend.ion_electron_forces(n) + ionion.forces_stress(box, frac @ box, z, Rc, Rd)[0]


@pytest.fixture(scope='module')
def driven():
    """ground state and force constants of the a16 case on the numpy backend; run once for the tests below"""
    box, shape, frac, _den, raw, k_max = fc_cases.make_inputs('a16')
    tab = recpot_table(raw, k_max)
    z = np.full(frac.shape[0], float(tab[2]))
    n_elec = float(z.sum())
    b = FD.NumpyFcBackend(box, shape, [(frac, tab)], TERMS)
    chi = np.full(shape, np.sqrt(n_elec / abs(np.linalg.det(box))))
    relax(b, chi, n_elec)
    r = force_constants(None, box, [(frac, tab)], chi, backend=b, rtol=1e-11)
    return dict(box=box, shape=shape, frac=frac, tab=tab, z=z, n_elec=n_elec, chi=chi, backend=b, r=r)


def test_driver_returns_a_symmetric_matrix_whose_parts_add_up(driven):
    """Measured: asymmetry 5.1e-12 of max|Phi| = 4.63e-2 Ha/bohr^2 (parts 0.260 ion-ion, 0.255 direct, 0.456 response), twelve solves
    of 101-103 iterations, acoustic sum rule residual 9.7e-4 (the egg-box effect: reported, not asserted), max|g|/dV 2.3e-11."""
    r = driven['r']
    phi, parts = r['phi'], r['parts']
    n = phi.shape[0]
    M = phi.transpose(0, 2, 1, 3).reshape(3 * n, 3 * n)
    asym = float(np.abs(M - M.T).max() / np.abs(M).max())
    print('MEASURE fc driver a16: max|Phi| %.4e parts %s asymmetry %.2e asr %.2e iterations %d..%d products %d max|g|/dV %.2e'
          % (np.abs(phi).max(), {k: '%.3f' % np.abs(v).max() for k, v in parts.items()}, asym, r['asr_residual'],
             min(r['iterations']), max(r['iterations']), r['hvp_count'], r['ground_state_gradient']))
    assert phi.shape == (4, 4, 3, 3) and len(r['iterations']) == 12
    assert all(x == optimize.CG_CONVERGED for x in r['reason']) and max(r['rel_residual']) <= 1e-11
    assert asym <= SYMMETRY_BOUND
    assert np.array_equal(parts['ion_ion'] + parts['direct'] + parts['response'], phi)
    assert r['hvp_count'] >= sum(r['iterations'])
    assert r['asr_residual'] == pytest.approx(float(np.abs(phi.sum(axis=1)).max() / np.abs(phi).max()), rel=1e-12)


def test_driver_options_rows_units_and_sum_rule(driven):
    d, r = driven, driven['r']
    b = d['backend']
    one = force_constants(None, d['box'], [(d['frac'], d['tab'])], d['chi'], primitive_ion_indices=[1], backend=b, rtol=1e-11)
    assert one['phi'].shape == (1, 4, 3, 3) and np.array_equal(one['phi'][0], r['phi'][1]) and len(one['iterations']) == 3
    ev = force_constants(None, d['box'], [(d['frac'], d['tab'])], d['chi'], primitive_ion_indices=[1], backend=b, rtol=1e-11,
                         units='eV/a2', impose_asr=True)
    f = (4.3597447222071e-18 / 1.602176634e-19) / (5.29177210903e-11 * 1e10) ** 2                       # system.py:27-33, 715
    fixed = one['phi'].copy()
    fixed[0, 1] -= one['phi'].sum(axis=1)[0]
    assert np.allclose(ev['phi'], fixed * f, rtol=1e-14, atol=0)
    assert np.abs(ev['phi'].sum(axis=1)).max() <= 64 * EPS * np.abs(ev['phi']).sum(axis=1).max()
    assert ev['asr_residual'] == one['asr_residual']               # the residual reported is that of the uncorrected matrix
    with pytest.warns(UserWarning, match='did not converge'):            # a solve cut short is said aloud
        cut = force_constants(None, d['box'], [(d['frac'], d['tab'])], d['chi'], primitive_ion_indices=[0], backend=b, maxiter=3)
    assert cut['reason'] == [optimize.CG_MAXITER] * 3 and cut['iterations'] == [3, 3, 3]
    with pytest.raises(ValueError, match='units'):
        force_constants(None, d['box'], [(d['frac'], d['tab'])], d['chi'], backend=b, units='GPa')
    with pytest.raises(ValueError, match='primitive_ion_indices'):
        force_constants(None, d['box'], [(d['frac'], d['tab'])], d['chi'], primitive_ion_indices=[4], backend=b)


def test_a_column_is_the_central_difference_of_forces_between_relaxed_ground_states(driven):
    """Phi[:, b, :, j] against -(F(R + eps) - F(R - eps)) / (2 eps) with the density re-relaxed at both displaced geometries,
    eps = 1e-3 bohr.  The bound is ten times the 2.65e-7 of max|Phi| measured with the reference-only pieces: eps^2 truncation.
    Measured for the column (ion 2, y): 2.20e-7."""
    d = driven
    ib, j = FD_COLUMN
    F = {}
    for sign in (+1, -1):
        cart = d['frac'] @ d['box']
        cart[ib, j] += sign * FD_EPS
        frac = cart @ np.linalg.inv(d['box'])
        b = FD.NumpyFcBackend(d['box'], d['shape'], [(frac, d['tab'])], TERMS)
        chi = d['chi'].copy()
        relax(b, chi, d['n_elec'])
        F[sign] = total_forces(b, d['box'], frac, d['z'], chi, d['n_elec'])
    fd = -(F[+1] - F[-1]) / (2 * FD_EPS)
    phi = d['r']['phi']
    dev = float(np.abs(phi[:, ib, :, j] - fd).max() / np.abs(phi).max())
    print('MEASURE fc driver a16 finite difference column (%d, %d): %.3e' % (ib, j, dev))
    assert dev <= FD_COLUMN_BOUND


# ------------------------------------------------------------------------------- 4: the ABI
@pytest.mark.parametrize('dtype', [N.F64, N.F32])
def test_entry_points_are_exported_and_refuse_null_arguments(dtype):
    """both libraries export the three symbols; a null context is OFDFT_EINVAL in both (the fp32 library's f64-only code)"""
    lib = N.load(dtype)
    for name in ('ofdft_ionic_potential_gradient', 'ofdft_ion_electron_curvature', 'ofdft_ion_ion_hessian'):
        assert name in N.EXPORTS and hasattr(lib, name)
    x = (ctypes.c_double * 9)()
    rows = (ctypes.c_int * 1)(0)
    assert lib.ofdft_ionic_potential_gradient(None, x, 1, x, x, 2, 3.0, 0, 0, None, None) == N.EINVAL
    assert lib.ofdft_ion_electron_curvature(None, None, x, 1, x, x, 2, 3.0, 0, x, None) == N.EINVAL
    assert lib.ofdft_ion_ion_hessian(None, x, x, 1, 0.0, rows, 1, x, None) == N.EINVAL


# ------------------------------------------------------------------------------- 5: the driver code shared with elastic.py
def test_the_device_backend_is_closed_when_a_piece_raises(monkeypatch):
    """force_constants owns the backend it makes: a piece that raises leaves no conjugate-gradient handle behind"""
    from professad_amd import force_constants as fc_mod

    class Fake:
        dV = 1.0
        closed = 0

        def __init__(self, engine, box_vecs, species):
            Fake.made = self

        def ground_state_gradient(self, chi, n_elec):
            return 0.0

        def ion_ion_hessian(self, frac, charges, rows, Rc):
            return np.zeros((len(rows), frac.shape[0], 3, 3))

        def ion_electron_curvature(self, den):
            raise RuntimeError('curvature failed')

        def close(self):
            self.closed += 1

    monkeypatch.setattr(fc_mod, 'HipFcBackend', Fake)
    monkeypatch.setattr(fc_mod, 'refusal', lambda engine, pme_order=None: None)
    tab = (np.linspace(0.0, 4.0, 9), np.ones(9), 3.0)
    with pytest.raises(RuntimeError, match='curvature failed'):
        force_constants(None, np.eye(3), [(np.zeros((2, 3)), tab)], np.ones((2, 2, 2)))
    assert Fake.made.closed == 1


def test_both_drivers_normalise_a_species_list_the_same_way(monkeypatch):
    """one normalisation (optimize.normalise_species) behind force_constants and elastic_constants: the backends of both see the
    same (frac, charges, n_elec) for a two-species list"""
    from professad_amd import elastic as el_mod
    from professad_amd import force_constants as fc_mod
    tab_a, tab_b = (np.linspace(0.0, 4.0, 9), np.ones(9), 3.0), (np.linspace(0.0, 4.0, 5), np.ones(5), 1.0)
    species = [([[0.0, 0.0, 0.0], [0.5, 0.5, 0.5]], tab_a), (np.array([0.25, 0.25, 0.75]), tab_b)]
    want_frac = np.array([[0.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.25, 0.25, 0.75]])
    want_z = np.array([3.0, 3.0, 1.0])
    norm, frac, z = optimize.normalise_species(species)
    assert np.array_equal(frac, want_frac) and np.array_equal(z, want_z) and frac.dtype == np.float64
    assert [f.shape for f, _t in norm] == [(2, 3), (1, 3)] and norm[1][1] is tab_b
    seen = {}

    class Stop(Exception):
        pass

    class Spy:
        dV, volume = 1.0, 1.0

        def __init__(self, who):
            self.who = who

        def ground_state_gradient(self, chi, n_elec):
            seen[self.who] = [n_elec]
            return 0.0

        def ion_ion_hessian(self, frac, charges, rows, Rc):
            seen[self.who] += [frac, charges]
            raise Stop

        def strain_hessian(self, den):
            return {}

        def ion_ion_strain_hessian(self, frac, charges, Rc):
            seen[self.who] += [frac, charges]
            raise Stop

    chi = np.ones((2, 2, 2))
    with pytest.raises(Stop):
        fc_mod.force_constants(None, np.eye(3), species, chi, backend=Spy('fc'))
    with pytest.raises(Stop):
        el_mod.elastic_constants(None, np.eye(3), species, chi, backend=Spy('el'))
    for who in ('fc', 'el'):
        n_elec, frac, z = seen[who]
        assert n_elec == 7.0 and np.array_equal(frac, want_frac) and np.array_equal(z, want_z)


def test_species_arrays_rejects_unequal_and_two_dimensional_tables():
    from professad_amd.ions import _species_arrays
    ks = np.linspace(0.0, 4.0, 9)
    frac, k, v, z = _species_arrays([0.1, 0.2, 0.3], (ks, np.ones(9), 3))
    assert frac.shape == (1, 3) and frac.flags.c_contiguous and k.dtype == v.dtype == np.float64 and z == 3.0 and isinstance(z, float)
    with pytest.raises(ValueError, match='equal length'):
        _species_arrays(np.zeros((1, 3)), (ks, np.ones(8), 3.0))
    with pytest.raises(ValueError, match='1-D'):
        _species_arrays(np.zeros((1, 3)), (ks.reshape(3, 3), np.ones((3, 3)), 3.0))
