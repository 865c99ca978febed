"""GPU tests of the stages that OFDFT_OPT_HVP_WGC = 1 and OFDFT_OPT_HVP_GGA = 1 add to the Hessian-vector product (hvp_gga_mid_kernel,
hvp_wgc_head_kernel, hvp_wgc_tail_kernel and the kGga / kWgc instantiations of hvp_combine_kernel, each in its n-space and chi-space
form) on grids past the block caps of their grid-stride loops.  tests/test_second_order_extents_gpu.py runs these
grids with cfg2's terms only, which launch none of them; the largest grid the options had run on is (48, 96, 32): 288 blocks, one trip.

  A = (128, 128, 64): 524 288 pairs = 2048 x 256, the cap of the WGC99 head exactly, and twice the 1024-block cap of the mid, tail
      and combine kernels: every loop takes a second trip, every reduction has blocks that carry two trips.
  B = (81, 81, 81): 531 441 points, odd: block 0 / thread 0 patches the last point after its own trips; the chirp-z transforms.
Inputs, doubles and figures: tests/hvp_options_extents.py (the inputs of that test unchanged; terms cfg3w, the bench set).  A wrong
stride, a reduction that drops the blocks above the cap, an odd tail applied twice or left out, or a retained U / G / grad n short by
the second trip would each pass every other test; the last one matters most, since every CG iteration after the first is a
reuse_density product.

Tolerance rule: 10 x YARDSTICK, the deviation of the numpy double from the same formulas in long double, a copy of
MEASURED_EXTENTS of tests/test_hvp_vacuum_cpu.py (computed without a device).  A sum may deviate by no less than ten roundings of
its own terms (hvp_options_extents.q_floor; 10 eps for the figures already relative to sum|terms|); a and S against
math.fsum at 64 eps of sum|terms|, as in tests/test_second_order_extents_gpu.py.  Nothing may reach 1e-11 (FINDING).  The numpy doubles
are computed once per shape and shared.  Every test prints its figures as `MEASURE ...` before it asserts; the MI355X figures are in
MEASURED_DEVICE.
"""
import math

import numpy as np
import pytest
import torch

import hvp_options_extents as X
from professad_amd import _native as N
from professad_amd import optimize
from professad_amd.engine import Engine

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS = 2.0 ** -52
FINDING = 1e-11
SUM_FLOOR = 10 * EPS
# copy of MEASURED_EXTENTS of tests/test_hvp_vacuum_cpu.py: the numpy double against long double
YARDSTICK = {
    'A': dict(cfg3w=dict(hv=7.92e-16, q_hartree=5.55e-16, q_tf=2.45e-16, q_vw=3.20e-16, q_wgc99_nl=7.62e-16, q_pbe_x=2.00e-16, q_pbe_c=6.10e-16),
              wgc99_nl=dict(hv=5.45e-16, q_wgc99_nl=7.62e-16), pbe=dict(hv=4.53e-15, q_pbe_x=2.00e-16, q_pbe_c=6.10e-16),
              chi=dict(Hd=8.74e-16, dHd=3.26e-16, phiHd=1.86e-17, dmu=9.11e-15)),
    'B': dict(cfg3w=dict(hv=1.17e-15, q_hartree=2.73e-16, q_tf=3.63e-16, q_vw=3.55e-16, q_wgc99_nl=3.01e-16, q_pbe_x=9.08e-16, q_pbe_c=7.56e-16),
              wgc99_nl=dict(hv=1.00e-15, q_wgc99_nl=3.01e-16), pbe=dict(hv=3.71e-15, q_pbe_x=9.08e-16, q_pbe_c=7.56e-16),
              chi=dict(Hd=1.15e-15, dHd=4.87e-16, phiHd=4.59e-17, dmu=3.71e-14),
              cg=dict(x=8.73e-15)),          # three CG iterations: max|x - long double| / max|long double|
}
# transforms of a product and of its reuse call (tests/test_hvp_wgc_gpu.py, tests/test_hvp_gga_gpu.py)
FFT = {'cfg3w': (42, 24), 'wgc99_nl': (24, 12), 'pbe': (12, 8)}
# measured on an MI355X against the numpy double, the figures of YARDSTICK (for the record: the bounds come from YARDSTICK alone).
# q_field: |sum_t q_t - sum(w hv) dV| / sum|w hv| dV; a and S equal math.fsum to the last bit; mixed-sign chi: equal bits
MEASURED_DEVICE = {
    'A': dict(cfg3w=dict(hv=1.14e-15, q_hartree=3.70e-16, q_tf=3.68e-16, q_vw=0.0, q_wgc99_nl=1.22e-15, q_pbe_x=2.00e-16, q_pbe_c=1.10e-15, q_field=7.92e-16),
              wgc99_nl=dict(hv=1.51e-15, q_wgc99_nl=1.22e-15, q_field=9.15e-16), pbe=dict(hv=4.14e-15, q_pbe_x=2.00e-16, q_pbe_c=1.10e-15, q_field=1.33e-15),
              chi=dict(Hd=1.72e-15, dHd=7.60e-16, phiHd=1.84e-17, dmu=1.13e-14)),
    'B': dict(cfg3w=dict(hv=2.04e-15, q_hartree=1.64e-15, q_tf=1.33e-15, q_vw=1.66e-15, q_wgc99_nl=1.81e-15, q_pbe_x=2.87e-15, q_pbe_c=1.89e-15, q_field=8.27e-16),
              wgc99_nl=dict(hv=2.22e-15, q_wgc99_nl=1.81e-15, q_field=9.04e-16), pbe=dict(hv=8.97e-15, q_pbe_x=2.87e-15, q_pbe_c=1.89e-15, q_field=1.83e-15),
              chi=dict(Hd=2.16e-15, dHd=8.12e-16, phiHd=4.61e-17, dmu=1.11e-14), cg=dict(x=1.38e-14)),
}

_REF = {}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.double, device=DEV)


def double(key, which):
    """the numpy doubles of a shape, computed once: 'terms' (hvp_options_extents.per_term) or 'chi' (chi_product)"""
    if (key, which) not in _REF:
        _REF[key, which] = X.per_term(key) if which == 'terms' else X.chi_product(key)
    return _REF[key, which]


def engine(key, names=X.CFG3W):
    i = X.inputs(key)
    eng = Engine(i['shape'], DEV).set_cell(i['box']).set_terms(list(names)).set_option(N.OPT_HVP_WGC, 1).set_option(N.OPT_HVP_GGA, 1)
    if key == 'A':
        assert eng.fast_path
    else:
        assert eng.query(N.Q_FAST_PATH) == 0
    return eng


def bound(key, name, fig, floor=0.0):
    y = YARDSTICK[key][name]
    return {k: max(10 * max(y[k], EPS), floor if np.isscalar(floor) else floor.get(k, 0.0)) for k in fig}


def check(key, name, fig, floor=0.0):
    """10 x the yardstick per printed figure, or the floor of a sum; nothing at the size of a finding"""
    for k, b in bound(key, name, fig, floor).items():
        assert fig[k] <= b <= FINDING, (key, name, k, fig[k], b)


# ------------------------------------------------------------------------------- 1: the n-space product
@pytest.mark.parametrize('name', list(X.SETS))
@pytest.mark.parametrize('key', ['A', 'B'])
def test_hessian_vector_past_the_caps(key, name):
    """Engine.hessian_vector(want_terms=True) for cfg3w, for wgc99_nl alone and for pbe_x + pbe_c alone -- each stage's own field and
    sum, not only the total in which one stage could hide in another's rounding -- against tests/hvp_wgc_double.py: hv, every q_t,
    sum_t q_t against the returned field; 42 / 24, 24 / 12 and 12 / 8 transforms; reuse_density is bitwise in hv and q.
    Measured on an MI355X: MEASURED_DEVICE."""
    i = X.inputs(key)
    names = X.SETS[name]
    terms = double(key, 'terms')
    qd, hvd = X.set_product(terms, names)
    eng = engine(key, names)
    tden, tw = dev(i['den']), dev(i['w'])
    q, hv = eng.hessian_vector(tden, tw, want_terms=True)
    c0 = eng.query(N.Q_FFT_COUNT)
    q1, hv1 = eng.hessian_vector(tden, tw, reuse_density=True, want_terms=True)
    c1 = eng.query(N.Q_FFT_COUNT)
    eng.close()
    assert (c0, c1) == FFT[name]
    assert torch.equal(hv, hv1) and q == q1
    hv = hv.cpu().numpy()
    fig = X.hv_figures(q, hv, qd, hvd)
    floors = {'q_' + t: X.q_floor(i['w'], terms[t][1], i['dV'], qd[t]) for t in names if t != 'ion_electron'}
    wh = i['w'] * hv
    q_field = abs(sum(q.values()) - math.fsum(wh.ravel().tolist()) * i['dV']) / (float(np.abs(wh).sum()) * i['dV'])
    print('MEASURE hvp options extents %s %s: %s  q_field %.2e' % (key, name, ' '.join('%s %.2e' % kv for kv in fig.items()), q_field))
    print('MEASURE hvp options extents %s %s bounds: %s' % (key, name, ' '.join('%s %.2e' % kv for kv in bound(key, name, fig, floors).items())))
    assert np.isfinite(hv).all()
    check(key, name, fig, floors)
    assert q_field <= SUM_FLOOR
    assert all(v == 0.0 for t, v in q.items() if t not in names or t == 'ion_electron')


# ------------------------------------------------------------------------------- 2: the chi-space product
@pytest.mark.parametrize('key', ['A', 'B'])
def test_hessian_vector_chi_past_the_caps(key):
    """Engine.hessian_vector_chi(want_scalars=True) for cfg3w with a made-up gradient perpendicular to phi against
    hvp_wgc_double.hessian_vector_chi: H d, d.H d, phi.H d, d mu; a = phi.d and S = phi.phi against math.fsum at 64 eps sum|terms|;
    42 / 24 transforms; reuse_density is bitwise.
    Measured on an MI355X: MEASURED_DEVICE."""
    i = X.inputs(key)
    sd, Hdd = double(key, 'chi')
    eng = engine(key)
    tphi, td, tg = dev(i['phi']), dev(i['d']), dev(i['gr'])
    s, Hd = eng.hessian_vector_chi(tphi, td, tg, i['n_elec'], want_scalars=True)
    c0 = eng.query(N.Q_FFT_COUNT)
    s1, Hd1 = eng.hessian_vector_chi(tphi, td, tg, i['n_elec'], reuse_density=True, want_scalars=True)
    c1 = eng.query(N.Q_FFT_COUNT)
    eng.close()
    assert (c0, c1) == FFT['cfg3w']
    assert torch.equal(Hd, Hd1) and s == s1
    fig = X.chi_figures(s, Hd.cpu().numpy(), sd, Hdd, i['phi'], i['d'])
    floors = dict(dHd=SUM_FLOOR, phiHd=SUM_FLOOR)
    pd, pp = i['phi'] * i['d'], i['phi'] * i['phi']
    da = abs(s['a'] - math.fsum(pd.ravel().tolist())) / float(np.abs(pd).sum())
    dS = abs(s['S'] - math.fsum(pp.ravel().tolist())) / float(pp.sum())
    print('MEASURE hvp options extents chi %s: %s  a %.2f eps S %.2f eps of sum|terms|' % (key, ' '.join('%s %.2e' % kv for kv in fig.items()), da / EPS, dS / EPS))
    check(key, 'chi', fig, floors)
    assert da <= 64 * EPS and dS <= 64 * EPS


# ------------------------------------------------------------------------------- 3: chi of mixed sign
def test_a_chi_of_mixed_sign_is_the_positive_one_with_the_signs_put_back():
    """B: the chi-space mid, head and tail kernels form n and dn on the fly, even in every phi_j, in their loops and in the odd-tail
    patch alike: hessian_vector_chi(s phi, s d, s g) = s * hessian_vector_chi(phi, d, g) *bitwise*, scalars included (the double gives
    a difference of exactly 0.0 on v16s, tests/test_hvp_vacuum_cpu.py)."""
    key = 'B'
    i = X.inputs(key)
    sg = X.signs(i['shape'])
    assert 0.4 < (sg < 0).mean() < 0.6 and sg.ravel()[-1] in (-1.0, 1.0)
    eng = engine(key)
    s0, H0 = eng.hessian_vector_chi(dev(i['phi']), dev(i['d']), dev(i['gr']), i['n_elec'], want_scalars=True)
    s1, H1 = eng.hessian_vector_chi(dev(sg * i['phi']), dev(sg * i['d']), dev(sg * i['gr']), i['n_elec'], want_scalars=True)
    eng.close()
    sd, Hdd = double(key, 'chi')
    f0 = float(np.abs(H0.cpu().numpy() - Hdd).max() / np.abs(Hdd).max())
    print('MEASURE hvp options extents mixed-sign chi B: max|H(s phi, s d, s g) - s H(phi, d, g)| = %.1e  Hd %.2e'
          % (float((H1 - dev(sg) * H0).abs().max()), f0))
    assert s0 == s1
    assert torch.equal(H1, dev(sg) * H0)
    check(key, 'chi', dict(Hd=f0))


# ------------------------------------------------------------------------------- 4: the solver's hand-off to the product
def test_three_cg_iterations_through_the_engines_product():
    """B: optimize.solve_projected(HipCgBackend(eng), phi, None, rhs, N, 1e-30, 3) against the same call on
    hvp_wgc_double.NumpyCgBackend, rhs as optimize.density_response forms it from tn_cases.response_dv: both end with (3, CG_MAXITER,
    3 products); x by max|dx| / max|x| within 10 x its own yardstick (the same three iterations in long double).  Iterations 2 and 3 are reuse products: the only place where
    the retained U, G and grad n are read past the caps and across the solver's in-place p -> q hand-off.
    Measured on an MI355X: MEASURED_DEVICE."""
    key = 'B'
    x_np, it_np, reason_np, rel_np, nprod_np = X.numpy_cg(key)
    eng = engine(key)
    backend = optimize.HipCgBackend(eng)
    x, it, reason, rel, nprod = X.cg_solve(key, backend, dev)
    x = x.cpu().numpy()
    backend.close()
    eng.close()
    fig = float(np.abs(x - x_np).max() / np.abs(x_np).max())
    print('MEASURE hvp options extents cg B: x %.2e  residual %.6e (numpy %.6e)' % (fig, rel, rel_np))
    assert (it, reason, nprod) == (3, optimize.CG_MAXITER, 3) == (it_np, reason_np, nprod_np)
    check(key, 'cg', dict(x=fig))
