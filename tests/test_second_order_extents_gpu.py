"""GPU tests of the second-order entries on grids past the block caps of their grid-stride kernels (hvp_kernels.h, fc_kernels.h,
cg_kernels.h through the engine's product), against the numpy doubles (tests/hvp_double.py, tn_double.py, fc_double.py):

  A = (128, 128, 64) in synth.cubic_cell(128): the fused transforms; npts / 2 + 1 = 524 289 is one element past 2048 blocks x 256
      threads and twice the 1024-block cap of the reducing kernels; the half spectrum has 540 672 points, past 524 288.
  B = (81, 81, 81) in synth.cubic_cell(81): the chirp-z transforms; 531 441 points, odd, past the 1024-block cap.
Both keep eta_max (9.9 and 11.3) inside the 11 .. 15 of the grids measured before, so the conditioning of the Lindhard kernel
(tests/test_hvp_gpu.py) does not move the yardstick.  Terms: cfg2's with the exponents of WGC98 (14 transforms), as in
test_mixed_radix_and_unequal_powers_of_two_match_the_double of tests/test_hvp_gpu.py and tests/test_tn_gpu.py.

Also here: a chi of mixed sign (every chi of the other chi-space tests is positive), and the ion-electron curvature entry on
grids with an odd last extent, unequal extents, more k-points than its 64-block cap covers in one trip, and two species.

Tolerance rule (that of tests/test_hvp_gpu.py): 10 x the largest deviation from the numpy double measured on an MI355X (MEASURED*
below; every test prints its figures as `MEASURE ...` before it asserts).  On top of it no figure may reach the size that
would be a finding: 1e-11 of the quantity's maximum (the threshold the docstring of test_terms_and_sets_match_the_reference_goldens
names), or 100 x the figure of the same key on (32, 16, 64).  The numpy doubles of A and B are computed once and shared.
"""
import math

import numpy as np
import pytest
import torch

import cases
import fc_double as FD
import hvp_cases
import hvp_double as D
import tn_cases
import tn_double as T
from professad_amd import _native as N
from professad_amd import ions, optimize, synth
from professad_amd.engine import Engine

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TERMS = list(tn_cases.TERMS)
AL, BE = D.WGC98
EPS = 2.0 ** -52
SHAPES = {'A': (128, 128, 64), 'B': (81, 81, 81)}
FINDING = 1e-11
# the figures of (32, 16, 64) for the keys that have one (tests/test_hvp_gpu.py: MEASURED_DOUBLE; tests/test_tn_gpu.py)
AT_32_16_64 = dict(hv=1.27e-13, q_hartree=6.90e-16, q_tf=1.22e-16, q_vw=0.0, q_wt_nl=9.69e-13, q_lda_x=1.91e-16, q_pz_c=5.29e-16,
                   Hd=1.20e-13)

# measured on an MI355X.  hv, Hd, cg_x: max|. - double| / max|double|; q_<term>: |q_t - double| / |double|; q_field: |sum_t q_t -
# sum(w hv) dV| / sum|w hv| dV; dHd, phiHd: |. - double| / sum|d Hd|, sum|phi Hd|; dmu: |dmu - double| / |double|
# (a figure below one rounding of a double -- q_vw on A: equal bits -- counts as that rounding)
MEASURED = {
    'A': dict(hv=3.18e-14, q_hartree=3.70e-16, q_tf=3.68e-16, q_vw=0.0, q_wt_nl=1.04e-14, q_lda_x=5.73e-16, q_pz_c=8.85e-16,
              q_field=7.81e-16, Hd=3.96e-14, dHd=6.42e-16, phiHd=1.67e-17, dmu=9.86e-14, cg_x=9.06e-15, gradient=1.12e-14,
              curvature=1.65e-15),
    'B': dict(hv=4.29e-14, q_hartree=1.64e-15, q_tf=1.33e-15, q_vw=1.66e-15, q_wt_nl=4.33e-14, q_lda_x=1.32e-15, q_pz_c=5.24e-16,
              q_field=8.13e-16, Hd=4.18e-14, dHd=1.28e-15, phiHd=1.47e-17, dmu=2.78e-14, cg_x=3.36e-14),
    'g17r': dict(Hd=4.45e-14),
}
# max|D - double| / max|double| of ions.ion_electron_curvature
MEASURED_CURVATURE = {(17, 17, 17): 2.79e-15, (20, 18, 33): 1.54e-15, (32, 32, 33): 1.05e-14, (48, 16, 16): 3.65e-15}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.double, device=DEV)


def check(key, name, figure):
    """the 10 x rule for one printed figure, and the finding thresholds"""
    assert figure <= 10 * max(MEASURED[key][name], EPS), (key, name, figure)
    assert figure <= FINDING, (key, name, figure)
    if name in AT_32_16_64:
        assert figure <= 100 * max(AT_32_16_64[name], EPS), (key, name, figure)


_IN, _REF = {}, {}


def inputs(key):
    """box, density, directions and the made-up gradient perpendicular to phi of a shape, made once"""
    if key not in _IN:
        if key == 'g17r':
            box, phi, _d, _vext, n_elec = tn_cases.make_inputs(key)
            shape, den, al, be = phi.shape, None, tn_cases.ALPHA, tn_cases.BETA
        else:
            shape = SHAPES[key]
            box = synth.cubic_cell(shape[0])
            den = synth.random_density(shape, seed=11)
            phi = 0.6 * np.sqrt(den)
            n_elec = float(den.sum() * abs(np.linalg.det(box)) / den.size)
            al, be = AL, BE
        gr = hvp_cases.direction(shape, seed=84)
        gr -= phi * (phi * gr).sum() / (phi * phi).sum()
        _IN[key] = dict(box=box, shape=shape, den=den, phi=phi, n_elec=n_elec, al=al, be=be, dV=abs(np.linalg.det(box)) / phi.size,
                        w=hvp_cases.direction(shape, seed=78), d=hvp_cases.direction(shape, seed=83), gr=gr)
    return _IN[key]


def double(key, which):
    """the numpy double of the n-space ('hv') or chi-space ('chi') product of a shape, computed once"""
    if (key, which) not in _REF:
        i = inputs(key)
        if which == 'hv':
            _REF[key, which] = D.hessian_vector(i['box'], i['den'], i['w'], TERMS, i['al'], i['be'])
        else:
            _REF[key, which] = T.hessian_vector_chi(i['box'], i['phi'], i['d'], i['gr'], i['n_elec'], TERMS, i['al'], i['be'])
    return _REF[key, which]


def engine(key):
    i = inputs(key)
    eng = Engine(i['shape'], DEV).set_cell(i['box']).set_terms(TERMS, dict(wt_alpha=i['al'], wt_beta=i['be']))
    if key == 'A':
        assert eng.fast_path
    else:
        assert eng.query(N.Q_FAST_PATH) == 0
    return eng


def signs(shape):
    """+-1 per point, about half of them negative"""
    return np.where(np.random.default_rng(85).random(shape) < 0.5, -1.0, 1.0)


# ------------------------------------------------------------------------------- 1: the n-space product
@pytest.mark.parametrize('key', ['A', 'B'])
def test_hessian_vector_past_the_caps(key):
    """Engine.hessian_vector(want_terms=True) against tests/hvp_double.py: hv, every q_t, and the sums against the returned field;
    reuse_density is bitwise and drops the transform count from 14 to 8.
    Measured on an MI355X, A / B: hv 3.2e-14 / 4.3e-14 of max|hv|; q_t hartree 3.7e-16 / 1.6e-15, tf 3.7e-16 / 1.3e-15, vw 0 / 1.7e-15,
    wt_nl 1.0e-14 / 4.3e-14, lda_x 5.7e-16 / 1.3e-15, pz_c 8.9e-16 / 5.2e-16; the sums against the field 7.8e-16 / 8.1e-16."""
    i = inputs(key)
    qd, hvd = double(key, 'hv')
    eng = engine(key)
    tden, tw = dev(i['den']), dev(i['w'])
    q, hv = eng.hessian_vector(tden, tw, want_terms=True)
    assert eng.query(N.Q_FFT_COUNT) == 14
    q1, hv1 = eng.hessian_vector(tden, tw, reuse_density=True, want_terms=True)
    assert eng.query(N.Q_FFT_COUNT) == 8
    eng.close()
    assert torch.equal(hv, hv1) and q == q1
    hv = hv.cpu().numpy()
    fig = dict(hv=float(np.abs(hv - hvd).max() / np.abs(hvd).max()))
    for t in TERMS:
        if t != 'ion_electron':
            fig['q_' + t] = abs(q[t] - qd[t]) / abs(qd[t])
    wh = i['w'] * hv
    fig['q_field'] = abs(sum(q.values()) - math.fsum(wh.ravel().tolist()) * i['dV']) / (float(np.abs(wh).sum()) * i['dV'])
    print('MEASURE extents hvp %s: %s' % (key, ' '.join('%s %.2e' % kv for kv in fig.items())))
    for name, v in fig.items():
        check(key, name, v)
    assert q['ion_electron'] == 0.0 and all(v == 0.0 for t, v in q.items() if t not in TERMS)


# ------------------------------------------------------------------------------- 2: the chi-space product
def chi_figures(s, Hd, sd, Hdd, phi, d):
    return dict(Hd=float(np.abs(Hd - Hdd).max() / np.abs(Hdd).max()),
                dHd=abs(s['dHd'] - sd['dHd']) / float(np.abs(d * Hdd).sum()),
                phiHd=abs(s['phiHd'] - sd['phiHd']) / float(np.abs(phi * Hdd).sum()),
                dmu=abs(s['dmu'] - sd['dmu']) / abs(sd['dmu']))


@pytest.mark.parametrize('key', ['A', 'B'])
def test_hessian_vector_chi_past_the_caps(key):
    """Engine.hessian_vector_chi(want_scalars=True) with a made-up gradient perpendicular to phi against tests/tn_double.py: H d,
    d.H d, phi.H d, d mu; a = phi.d and S = phi.phi against math.fsum at 64 eps sum|terms| (the depth of the device's sums, see
    tests/test_cg_sweeps_gpu.py); reuse_density is bitwise.
    Measured on an MI355X, A / B: H d 4.0e-14 / 4.2e-14 of max|H d|, d.H d 6.4e-16 / 1.3e-15 of sum|d H d|, phi.H d 1.7e-17 / 1.5e-17 of
    sum|phi H d|, d mu 9.9e-14 / 2.8e-14 of itself; a and S equal math.fsum to the last bit."""
    i = inputs(key)
    sd, Hdd = double(key, 'chi')
    eng = engine(key)
    tphi, td, tg = dev(i['phi']), dev(i['d']), dev(i['gr'])
    s, Hd = eng.hessian_vector_chi(tphi, td, tg, i['n_elec'], want_scalars=True)
    assert eng.query(N.Q_FFT_COUNT) == 14
    s1, Hd1 = eng.hessian_vector_chi(tphi, td, tg, i['n_elec'], reuse_density=True, want_scalars=True)
    assert eng.query(N.Q_FFT_COUNT) == 8
    eng.close()
    assert torch.equal(Hd, Hd1) and s == s1
    fig = chi_figures(s, Hd.cpu().numpy(), sd, Hdd, i['phi'], i['d'])
    pd, pp = i['phi'] * i['d'], i['phi'] * i['phi']
    da = abs(s['a'] - math.fsum(pd.ravel().tolist())) / float(np.abs(pd).sum())
    dS = abs(s['S'] - math.fsum(pp.ravel().tolist())) / float(pp.sum())
    print('MEASURE extents chi %s: %s  a %.2f eps S %.2f eps of sum|terms|' % (key, ' '.join('%s %.2e' % kv for kv in fig.items()), da / EPS, dS / EPS))
    for name, v in fig.items():
        check(key, name, v)
    assert da <= 64 * EPS and dS <= 64 * EPS


# ------------------------------------------------------------------------------- 3: chi of mixed sign
@pytest.mark.parametrize('key', ['A', 'B', 'g17r'])
def test_a_chi_of_mixed_sign_is_the_positive_one_with_the_signs_put_back(key):
    """The closure is even in every chi_j, so with s = +-1 per point hessian_vector_chi(s phi, s d, s g) = s * hessian_vector_chi(phi,
    d, g) *bitwise*, scalars included: every sign cancels exactly in n, dn, k and in the three terms of P (the numpy double gives a
    difference of exactly 0.0, tests/test_second_order_doubles_cpu.py).  The flipped call against the double of the flipped
    inputs takes the bound of the unflipped one.
    Measured on an MI355X, A / B / g17r: H d 4.0e-14 / 4.2e-14 / 4.4e-14 of max|H d|, flipped and unflipped alike (equal bits)."""
    i = inputs(key)
    sg = signs(i['shape'])
    phi, d, gr = sg * i['phi'], sg * i['d'], sg * i['gr']
    assert 0.4 < (sg < 0).mean() < 0.6
    eng = engine(key)
    s0, H0 = eng.hessian_vector_chi(dev(i['phi']), dev(i['d']), dev(i['gr']), i['n_elec'], want_scalars=True)
    s1, H1 = eng.hessian_vector_chi(dev(phi), dev(d), dev(gr), i['n_elec'], want_scalars=True)
    eng.close()
    assert s0 == s1
    assert torch.equal(H1, dev(sg) * H0)
    sd, Hdd = T.hessian_vector_chi(i['box'], phi, d, gr, i['n_elec'], TERMS, i['al'], i['be'])
    sd0, Hdd0 = double(key, 'chi')
    f0 = float(np.abs(H0.cpu().numpy() - Hdd0).max() / np.abs(Hdd0).max())
    f1 = float(np.abs(H1.cpu().numpy() - Hdd).max() / np.abs(Hdd).max())
    print('MEASURE extents mixed-sign chi %s: Hd %.2e (unflipped %.2e)  double flipped - s * unflipped %.1e' % (key, f1, f0, np.abs(Hdd - sg * Hdd0).max()))
    check(key, 'Hd', f0)
    check(key, 'Hd', f1)
    assert sd['S'] == sd0['S'] and sd['a'] == sd0['a']


# ------------------------------------------------------------------------------- 4: the solver's hand-off to the product
@pytest.mark.parametrize('key', ['A', 'B'])
def test_three_cg_iterations_through_the_engines_product(key):
    """optimize.solve_projected(HipCgBackend(eng), phi, None, rhs, N, 1e-30, 3) against the same call on tests/tn_double.NumpyCgBackend,
    rhs as optimize.density_response forms it from tn_cases.response_dv: both end with (3, CG_MAXITER, 3 products); x by max|dx| /
    max|x|.  The only place where the in-place p -> q hand-off between the solver and the product runs past the caps.
    Measured on an MI355X, A / B: 9.1e-15 / 3.4e-14 of max|x|; residuals 1.209000e-2 / 1.548223e-1 on both sides."""
    i = inputs(key)
    phi, dV, n_elec = i['phi'], i['dV'], i['n_elec']
    dv = tn_cases.response_dv(i['shape'])
    S, c, n = T.density(i['box'], phi, n_elec)
    rhs = (-2.0 * c * dV) * phi * (dv - float((dv * n).sum()) * dV / n_elec)
    ref = T.NumpyCgBackend(i['box'], i['shape'], TERMS, i['al'], i['be'])
    x_np, it_np, reason_np, rel_np, nprod_np = optimize.solve_projected(ref, phi, None, rhs, n_elec, 1e-30, 3)
    eng = engine(key)
    backend = optimize.HipCgBackend(eng)
    x, it, reason, rel, nprod = optimize.solve_projected(backend, dev(phi), None, dev(rhs), n_elec, 1e-30, 3)
    x = x.cpu().numpy()
    backend.close()
    eng.close()
    fig = float(np.abs(x - x_np).max() / np.abs(x_np).max())
    print('MEASURE extents cg %s: x %.2e  residual %.6e (numpy %.6e)' % (key, fig, rel, rel_np))
    assert (it, reason, nprod) == (3, optimize.CG_MAXITER, 3) == (it_np, reason_np, nprod_np)
    check(key, 'cg_x', fig)


# ------------------------------------------------------------------------------- 5: the ion entries
def curvature_checks(eng, box, den, species):
    """-> max|D - double| / max|double| over the ions of both species, after the exact properties: symmetric blocks, a repeated
    call and each species on its own return the same bits"""
    tden = dev(den)
    Ds = ions.ion_electron_curvature(eng, box, tden, species)
    again = ions.ion_electron_curvature(eng, box, tden, species)
    alone = [ions.ion_electron_curvature(eng, box, tden, [sp])[0] for sp in species]
    assert [D_.shape for D_ in Ds] == [(1, 3, 3), (2, 3, 3)]
    for D_, D2, D1 in zip(Ds, again, alone):
        assert np.array_equal(D_, D_.transpose(0, 2, 1)) and np.array_equal(D_, D2) and np.array_equal(D_, D1)
    got = np.concatenate(Ds)
    ref = np.concatenate([FD.ion_electron_curvature(box, den, f, tab) for f, tab in species])
    assert np.abs(ref[1:]).max() > 0.1 * np.abs(ref).max()          # the halved species is not lost in the first one's scale
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def test_ion_entries_on_shape_A():
    """ions.ionic_potential_gradient (its spectral kernel past 2048 x 256 k-points) and ions.ion_electron_curvature (64 blocks: 33
    trips) on (128, 128, 64) against tests/fc_double.py.
    Measured on an MI355X: gradient 1.1e-14 of max|dv|, curvature 1.7e-15 of max|D|."""
    shape = SHAPES['A']
    box = synth.cubic_cell(shape[0])
    species = FD.two_species(17)
    den = synth.smooth_density(shape, seed=7, n0=0.05, amp=0.5)
    ref = FD.potential_gradient(box, shape, (species[1][0] @ box)[1], species[1][1])
    eng = Engine(shape, DEV).set_cell(box)
    assert eng.fast_path
    dv = ions.ionic_potential_gradient(eng, box, species, 2)
    again = ions.ionic_potential_gradient(eng, box, species, 2)
    fc = curvature_checks(eng, box, den, species)
    eng.close()
    fg = float(np.abs(dv.cpu().numpy() - ref).max() / np.abs(ref).max())
    print('MEASURE extents ions A: gradient %.2e curvature %.2e' % (fg, fc))
    assert torch.equal(dv, again)
    check('A', 'gradient', fg)
    check('A', 'curvature', fc)


@pytest.mark.parametrize('shape,cell', [((17, 17, 17), ('cubic', 17)), ((20, 18, 33), ('tri', 1.0)), ((32, 32, 33), ('tri', 1.0)),
                                        ((48, 16, 16), ('tri', 1.0))])
def test_curvature_entry_on_odd_and_mixed_radix_grids(shape, cell):
    """ions.ion_electron_curvature against tests/fc_double.py (itself pinned to central differences of the forces on the odd grids,
    tests/test_second_order_doubles_cpu.py) where the entry had not run: an odd last extent (the half-spectrum weight is 1 at
    z = 0 only), unequal extents, 17 408 k-points (just past one trip of its 64 blocks) and a mixed-radix extent; two species.
    Measured on an MI355X: 2.8e-15 on (17, 17, 17), 1.5e-15 on (20, 18, 33), 1.1e-14 on (32, 32, 33), 3.7e-15 on (48, 16, 16) of max|D|."""
    box = cases.make_cell(cell)
    den = synth.smooth_density(shape, seed=7, n0=0.05, amp=0.5)
    eng = Engine(shape, DEV).set_cell(box)
    fig = curvature_checks(eng, box, den, FD.two_species(sum(shape)))
    eng.close()
    print('MEASURE extents curvature %s: %.2e' % (shape, fig))
    assert fig <= 10 * max(MEASURED_CURVATURE[shape], EPS) and fig <= FINDING
