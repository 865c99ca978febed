"""GPU tests of the force constants: ofdft_ionic_potential_gradient, ofdft_ion_electron_curvature and ofdft_ion_ion_hessian
(professad_amd.ions) against the reference's own autograd (tests/golden/fc_<case>.npz; generator tests/golden/make_golden_fc.py)
and, on grids without goldens, the numpy double (tests/fc_double.py); professad_amd.force_constants end to end on the fcc-Al 16^3
case against the numpy-driven matrix and against finite differences of forces between re-relaxed ground states.

Tolerance rule (that of tests/test_hvp_gpu.py) for the gradient and curvature entries: 10 x the largest deviation from the golden
-- or from the numpy double where no golden exists -- measured on an MI355X (MEASURED below; every test prints its figures as
`MEASURE ...` before it asserts).  The other bounds are reasoned where they stand.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cases
import fc_cases
import fc_double as FD
import tn_cases
from professad_amd import _native as N
from professad_amd import ions, optimize
from professad_amd.engine import Engine, engine_for
from professad_amd.force_constants import force_constants

pytestmark = pytest.mark.gpu
GOLDEN = os.path.dirname(os.path.abspath(cases.__file__))
DEV = 'cuda:0'
TERMS = list(tn_cases.TERMS)
EPS = 2.0 ** -52

# largest figures measured on an MI355X, relative to the maximum of the quantity (per-case values in the tests' docstrings)
MEASURED = {
    'gradient_golden': 1.17e-14,                 # max|dv - golden| / max|golden|, cases b and a16
    'curvature_golden': 1.94e-14,                 # max|D - golden| / max|golden|
    'gradient_double': {(17, 17, 17): 1.00e-15, (48, 16, 16): 1.41e-15, (32, 16, 64): 1.37e-15},
}
# The device sums the same M <= 2e4 pair tensors per block as the double, in another order and with the device's erfc and exp
# (a few units in the last place each): M eps of max|H| in the worst case (the bound of the double's own symmetry test).
ION_ION_BOUND = 2e4 * EPS
# issue: ten times the 2.65e-7 of max|Phi| of the reference-only run at eps = 1e-3 bohr (eps^2 truncation, device independent)
FD_COLUMN_BOUND = 10 * 2.65e-7
FD_EPS = 1e-3
FD_COLUMN = (2, 1)
# The response part is the error of twelve conjugate-gradient solves stopped at |r| <= rtol |b|: |dx| / |x| <= kappa rtol with
# kappa ~ (2 * 100 / ln(2 / rtol))^2 = 60 for ~100 iterations to rtol = 1e-11, on a part ten times max|Phi| (0.456 against 4.6e-2
# Ha/bohr^2): 60 * 1e-11 * 10 = 6e-9 of max|Phi|, for the symmetry as for the difference between two drivers at one chi.
SOLVE_BOUND = 1e-8
RTOL = 1e-11
# issue: ten times the 9.7e-4 seen on the CPU; an aliasing effect of the fixed grid, not an accuracy measure
ASR_BOUND = 1e-2


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.double, device=DEV)


_GOLD = {}


def gold(case):
    """golden file and inputs of a case, loaded once and shared"""
    if case not in _GOLD:
        g = np.load(os.path.join(GOLDEN, 'fc_%s.npz' % case))
        box, shape, frac, den, raw, k_max = fc_cases.make_inputs(case)
        assert abs(cases.checksum(box, frac, den, raw) - float(g['checksum'])) < 1e-9
        _GOLD[case] = (g, box, shape, frac, den, ions.recpot_table(raw, k_max))
    return _GOLD[case]


# ------------------------------------------------------------------------------- 1: the entries against the goldens
@pytest.mark.parametrize('case', fc_cases.CASES)
def test_gradient_and_curvature_entries_match_the_reference_goldens(case):
    """d v_ext / dR of one ion against the reference's Jacobian of lattice_sum, D against the diagonal blocks of its Hessian of
    IonElectron.  Measured on an MI355X, b / a16: gradient 1.2e-14 / 1.7e-15 of max|dv|, curvature 1.9e-14 / 3.0e-15 of max|D| (the numpy
    double of the same forms sits at 3.6e-15 / 5.7e-16 and 6.7e-15 / 1.2e-15, tests/test_force_constants_cpu.py)."""
    g, box, shape, frac, den, tab = gold(case)
    eng = Engine(shape, DEV).set_cell(box)
    dv = ions.ionic_potential_gradient(eng, box, [(frac, tab)], int(g['ion'])).cpu().numpy()
    D = ions.ion_electron_curvature(eng, box, dev(den), [(frac, tab)])[0]
    eng.close()
    ref = np.stack([g['hess'][p, :, p, :] for p in range(frac.shape[0])])
    d1 = float(np.abs(dv - g['dv']).max() / np.abs(g['dv']).max())
    d2 = float(np.abs(D - ref).max() / np.abs(ref).max())
    print('MEASURE fc %s: gradient %.2e curvature %.2e' % (case, d1, d2))
    assert dv.shape == (3,) + tuple(shape) and D.shape == (frac.shape[0], 3, 3)
    assert d1 <= 10 * MEASURED['gradient_golden'] and d2 <= 10 * MEASURED['curvature_golden']
    assert np.array_equal(D, D.transpose(0, 2, 1))


@pytest.mark.parametrize('shape,cell', [((17, 17, 17), ('cubic', 17)), ((48, 16, 16), ('tri', 1.0)), ((32, 16, 64), ('cubic', 32))])
def test_gradient_entry_matches_the_double_on_other_transform_families(shape, cell):
    """a chirp-z extent, a mixed-radix fused extent in a triclinic cell and unequal powers of two: the second of three ions of
    two species, against tests/fc_double.py.  Two species with different tables make the species and ion indexing visible.
    Measured on an MI355X: 1.0e-15 on 17^3, 1.4e-15 on (48, 16, 16), 1.4e-15 on (32, 16, 64) of max|dv|."""
    g = np.load(os.path.join(GOLDEN, 'ions.npz'))
    tab = ions.recpot_table(g['recpot_raw'], float(g['recpot_kmax']))
    tab2 = (tab[0], 0.5 * tab[1], 0.5 * tab[2])                       # a second, made-up species: half the potential
    box = cases.make_cell(cell)
    rng = np.random.default_rng(17)
    species = [(rng.random((1, 3)), tab), (rng.random((2, 3)) * 1.5 - 0.25, tab2)]      # (also coordinates outside [0, 1))
    ref = FD.potential_gradient(box, shape, (species[1][0] @ box)[0], tab2)
    eng = Engine(shape, DEV).set_cell(box)
    dv = ions.ionic_potential_gradient(eng, box, species, 1)
    again = ions.ionic_potential_gradient(eng, box, species, 1)
    eng.close()
    d = float(np.abs(dv.cpu().numpy() - ref).max() / np.abs(ref).max())
    print('MEASURE fc double %s: gradient %.2e' % (shape, d))
    assert d <= 10 * MEASURED['gradient_double'][shape]
    assert torch.equal(dv, again)


# ------------------------------------------------------------------------------- 2: ion-ion Hessian
@pytest.mark.parametrize('case', fc_cases.CASES + ['one'])
def test_ion_ion_hessian_matches_the_double_and_is_bitwise_reproducible(case):
    """against tests/fc_double.ion_ion_hessian (itself pinned to central differences of the oracle forces); subsets of rows and
    repeated calls return the same bits; a cell with one ion has no second derivative at all.
    Measured on an MI355X, b / a16: 2.7e-14 / 5.7e-14 of max|H| at the default cutoff (Rc = 40 bohr: 1.6e-15 / 2.9e-15), row sums
    4.2e-17 / 4.0e-17 of the sum of magnitudes, asymmetry 1.2e-16 / 1.6e-16."""
    _g, box, shape, frac, _den, tab = gold('a16' if case == 'one' else case)
    if case == 'one':
        frac = frac[:1]
    z = np.full(frac.shape[0], float(tab[2]))
    n = frac.shape[0]
    eng = Engine(shape, DEV).set_cell(box)
    H = ions.ion_ion_hessian(eng, box, frac, z, range(n))
    again = ions.ion_ion_hessian(eng, box, frac, z, range(n))
    sub = ions.ion_ion_hessian(eng, box, frac, z, [n - 1, 0]) if n > 1 else H
    Hc = ions.ion_ion_hessian(eng, box, frac, z, [0], Rc=40.0)
    eng.close()
    assert H.shape == (n, n, 3, 3) and np.array_equal(H, again)
    if case == 'one':
        assert not H.any() and not Hc.any()
        return
    assert np.array_equal(sub, H[[n - 1, 0]])
    ref = FD.ion_ion_hessian(box, frac, z, range(n))
    refc = FD.ion_ion_hessian(box, frac, z, [0], Rc=40.0)
    scale = float(np.abs(ref).max())
    d, dc = float(np.abs(H - ref).max() / scale), float(np.abs(Hc - refc).max() / scale)
    rows = float(np.abs(H.sum(axis=1)).max() / np.abs(H).sum(axis=1).max())
    asym = float(np.abs(H - H.transpose(1, 0, 3, 2)).max() / scale)
    print('MEASURE fc ion-ion %s: double %.2e (Rc = 40: %.2e) row sums %.2e asymmetry %.2e' % (case, d, dc, rows, asym))
    assert d <= ION_ION_BOUND and dc <= ION_ION_BOUND and asym <= ION_ION_BOUND
    assert rows <= 64 * EPS          # the diagonal block is the host's sum of the very numbers the other blocks negate


# ------------------------------------------------------------------------------- 3: end to end
_RUN = {}


def a16():
    box, shape, frac, _den, raw, k_max = fc_cases.make_inputs('a16')
    tab = ions.recpot_table(raw, k_max)
    return box, shape, frac, tab, np.full(frac.shape[0], float(tab[2]))


def relaxed(frac, chi0=None):
    """truncated-Newton ground state of the a16 cell with the ions at `frac` -> chi, density (device tensors)"""
    box, shape, _frac, tab, z = a16()
    eng = Engine(shape, DEV).set_cell(box)
    vext = ions.ionic_potential(eng, box, [(frac, tab)])
    eng.set_terms(TERMS)
    r = optimize.optimize_density(eng, float(z.sum()), vext, chi0=chi0, volume=abs(np.linalg.det(box)), n_method='TN')
    eng.close()
    assert r['converged']
    return r['chi'], r['den']


def run():
    """ground state and force constants of the a16 case, all four ions as rows; run once and shared"""
    if not _RUN:
        box, shape, frac, tab, _z = a16()
        chi, _den = relaxed(frac)
        eng = Engine(shape, DEV).set_cell(box).set_terms(TERMS)
        _RUN.update(chi=chi, eng=eng, r=force_constants(eng, box, [(frac, tab)], chi, rtol=RTOL))
    return _RUN


def test_force_constants_match_the_numpy_driven_matrix():
    """the same driver on tests/fc_double.NumpyFcBackend at the device's ground state; symmetry of the 12 x 12 matrix; the parts;
    every solve converged; the acoustic sum rule residual (the egg-box effect: an aliasing figure, bounded loosely).
    Measured on an MI355X: max|Phi| 4.6265e-2 Ha/bohr^2; Phi - numpy 3.2e-13 of it (ion-ion 3.2e-13, direct 2.4e-15, response 6.0e-15);
    asymmetry 5.2e-12; sum rule residual 9.72e-4; twelve solves of 101-103 iterations (numpy: the same), 1224 products; max|g|/dV 2.3e-11."""
    box, shape, frac, tab, _z = a16()
    r = run()['r']
    phi, parts = r['phi'], r['parts']
    ref = force_constants(None, box, [(frac, tab)], run()['chi'].cpu().numpy(), rtol=RTOL,
                          backend=FD.NumpyFcBackend(box, shape, [(frac, tab)], TERMS))
    scale = float(np.abs(ref['phi']).max())
    M = phi.transpose(0, 2, 1, 3).reshape(12, 12)
    asym = float(np.abs(M - M.T).max() / scale)
    d = float(np.abs(phi - ref['phi']).max() / scale)
    dparts = {k: float(np.abs(parts[k] - ref['parts'][k]).max() / scale) for k in parts}
    print('MEASURE fc a16: max|Phi| %.4e  Phi - numpy %.2e (%s)  asymmetry %.2e  asr %.2e  iterations %d..%d (numpy %d..%d) products %d  '
          'max|g|/dV %.2e' % (scale, d, ' '.join('%s %.2e' % kv for kv in dparts.items()), asym, r['asr_residual'], min(r['iterations']),
                              max(r['iterations']), min(ref['iterations']), max(ref['iterations']), r['hvp_count'],
                              r['ground_state_gradient']))
    assert phi.shape == (4, 4, 3, 3) and len(r['reason']) == 12
    assert all(x == optimize.CG_CONVERGED for x in r['reason']) and max(r['rel_residual']) <= RTOL
    assert d <= SOLVE_BOUND and asym <= SOLVE_BOUND
    assert np.array_equal(parts['ion_ion'] + parts['direct'] + parts['response'], phi)
    assert 0.0 < r['asr_residual'] < ASR_BOUND
    assert r['hvp_count'] >= sum(r['iterations']) and r['ground_state_gradient'] < 1e-8


def test_one_primitive_ion_is_a_row_of_the_full_call():
    box, _shape, frac, tab, _z = a16()
    s = run()
    one = force_constants(s['eng'], box, [(frac, tab)], s['chi'], primitive_ion_indices=[1], rtol=RTOL)
    assert one['phi'].shape == (1, 4, 3, 3) and len(one['iterations']) == 3
    assert np.array_equal(one['phi'][0], s['r']['phi'][1])
    for k in one['parts']:
        assert np.array_equal(one['parts'][k][0], s['r']['parts'][k][1])


def test_a_column_is_the_central_difference_of_forces_between_relaxed_ground_states():
    """Phi[:, b, :, j] against -(F(R + eps) - F(R - eps)) / (2 eps), F the ion-electron plus ion-ion forces at truncated-Newton
    ground states re-relaxed on the device at both displaced geometries, eps = 1e-3 bohr.  Bound: ten times the 2.65e-7 of
    max|Phi| of the reference-only run (eps^2 truncation).  Measured on an MI355X for the column (ion 2, y): 2.20e-7 (the numpy-driven
    run: 2.20e-7)."""
    box, shape, frac, tab, z = a16()
    s = run()
    ib, j = FD_COLUMN
    F = {}
    eng = Engine(shape, DEV).set_cell(box)
    for sign in (+1, -1):
        cart = frac @ box
        cart[ib, j] += sign * FD_EPS
        f = cart @ np.linalg.inv(box)
        _chi, den = relaxed(f, chi0=s['chi'])
        F[sign] = ions.ion_electron_forces(eng, box, den, [(f, tab)])[0] + ions.ion_ion(eng, box, f, z)[1]
    eng.close()
    fd = -(F[+1] - F[-1]) / (2 * FD_EPS)
    phi = s['r']['phi']
    d = float(np.abs(phi[:, ib, :, j] - fd).max() / np.abs(phi).max())
    print('MEASURE fc a16 finite difference column (%d, %d): %.3e' % (ib, j, d))
    assert d <= FD_COLUMN_BOUND


# ------------------------------------------------------------------------------- 4: refusals
def test_pme_is_refused_by_name():
    box, shape, frac, tab, _z = a16()
    eng = Engine(shape, DEV).set_cell(box).set_terms(TERMS)
    chi = torch.ones(shape, dtype=torch.double, device=DEV)
    with pytest.raises(NotImplementedError, match='PME'):
        force_constants(eng, box, [(frac, tab)], chi, pme_order=4)
    with pytest.raises(NotImplementedError, match='PME'):
        ions.ionic_potential_gradient(eng, box, [(frac, tab)], 0, pme_order=4)
    with pytest.raises(NotImplementedError, match='PME'):
        ions.ion_electron_curvature(eng, box, chi, [(frac, tab)], pme_order=4)
    # the raw entries answer OFDFT_EINVAL, the message naming PME
    dp = C.POINTER(C.c_double)
    f = np.ascontiguousarray(frac)
    ks, v = np.ascontiguousarray(tab[0]), np.ascontiguousarray(tab[1])
    out = torch.empty((3,) + tuple(shape), dtype=torch.double, device=DEV)
    c6 = np.zeros((4, 6))
    rc = eng.lib.ofdft_ionic_potential_gradient(eng._ctx, f.ctypes.data_as(dp), 4, ks.ctypes.data_as(dp), v.ctypes.data_as(dp), ks.size,
                                                float(tab[2]), 4, 0, C.c_void_p(out.data_ptr()), eng._stream())
    assert rc == N.EINVAL
    with pytest.raises(RuntimeError, match=r'\(-1\).*PME'):
        eng._check(rc, 'ofdft_ionic_potential_gradient')
    rc = eng.lib.ofdft_ion_electron_curvature(eng._ctx, C.c_void_p(chi.data_ptr()), f.ctypes.data_as(dp), 4, ks.ctypes.data_as(dp),
                                              v.ctypes.data_as(dp), ks.size, float(tab[2]), 4, c6.ctypes.data_as(dp), eng._stream())
    assert rc == N.EINVAL
    with pytest.raises(RuntimeError, match=r'\(-1\).*PME'):
        eng._check(rc, 'ofdft_ion_electron_curvature')
    eng.close()


def test_unserved_terms_slab_and_fp32_engines_are_refused_by_name():
    from professad_amd.distributed import DistEngine
    box, shape, frac, tab, z = a16()
    chi = torch.ones(shape, dtype=torch.double, device=DEV)
    eng = Engine(shape, DEV).set_cell(box).set_terms(['ion_electron', 'hartree', 'tf', 'pbe_x'])
    with pytest.raises(NotImplementedError, match=r'\bpbe_x\b'):
        force_constants(eng, box, [(frac, tab)], chi)
    eng.close()
    de = DistEngine(shape, DEV).set_cell(torch.as_tensor(box)).set_terms(['ion_electron', 'tf'])
    with pytest.raises(NotImplementedError, match='single-GPU'):
        force_constants(de, box, [(frac, tab)], chi)
    de.close()
    e32 = Engine(shape, DEV, dtype=torch.float32).set_cell(box).set_terms(['ion_electron', 'tf'])
    with pytest.raises(NotImplementedError, match='fp64'):
        force_constants(e32, box, [(frac, tab)], chi.float())
    with pytest.raises(NotImplementedError, match='fp64'):
        ions.ion_electron_curvature(e32, box, chi.float(), [(frac, tab)])
    # the fp32 library's own entries are stubs that name the fp64 library
    x = np.zeros(12)
    dp = C.POINTER(C.c_double)
    rows = (C.c_int * 1)(0)
    rc = e32.lib.ofdft_ion_ion_hessian(e32._ctx, x.ctypes.data_as(dp), x.ctypes.data_as(dp), 1, 0.0, rows, 1, x.ctypes.data_as(dp), None)
    assert rc == N.EINVAL
    with pytest.raises(RuntimeError, match='fp64 library'):
        e32._check(rc, 'ofdft_ion_ion_hessian')
    # plain fp64 work goes to the fp64 sibling: the ion-ion Hessian as it is, the potential gradient narrowed
    e64 = engine_for(shape, e32.device)
    assert np.array_equal(ions.ion_ion_hessian(e32, box, frac, z, [0]), ions.ion_ion_hessian(e64, box, frac, z, [0]))
    g32 = ions.ionic_potential_gradient(e32, box, [(frac, tab)], 2)
    assert g32.dtype == torch.float32 and torch.equal(g32, ions.ionic_potential_gradient(e64, box, [(frac, tab)], 2).float())
    e32.close()
