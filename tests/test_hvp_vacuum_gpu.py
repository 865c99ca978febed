"""GPU tests of the second derivatives of WGC99 and PBE (OFDFT_OPT_HVP_WGC = OFDFT_OPT_HVP_GGA = 1) where the
density runs from bulk into vacuum: the case v16s of tests/golden/hvp_vacuum_cases.py, den 3.7e-2 .. 1.6e-6, reduced gradient up to
6e2, r_s up to 53.  Every other Hessian test feeds densities of 0.02 .. 0.4; pbe_second builds its jets through n^(-8/3), n^(-7/3)
and r_s with lean rcp / log / exp, and wgc_triple uses n^(beta - 2).  n space against the reference's double autograd
(tests/golden/hvp_vacuum_v16s.npz; generator tests/golden/make_golden_hvp_vacuum.py), chi space against the numpy double
(tests/hvp_wgc_double.py).  The density floor of these tests is 1e-6 (hvp_vacuum_cases.DENSITY_FLOOR says why); lower densities
are out of scope.

Tolerance rule: all figures are taken per density decade, max|x - y| over the decade / max|y| over the decade, so that the bulk's
scale does not hide the vacuum (and the other way round).  The yardsticks below are copies of the tables of
tests/test_hvp_vacuum_cpu.py, computed without a device: per (key, decade) the largest mutual deviation of the numpy double, the
same formulas in long double and the golden.  The device may deviate by 10 x the yardstick -- ten is the factor every Hessian test
here uses -- sums by no less than ten roundings of their own terms (10 eps of sum|terms|), and nothing may reach 1e-11 (FINDING).
pbe_x and pbe_c alone are not compared as fields: their yardstick is already above 1e-12 (hvp_vacuum_cases.GPU_KEYS); their sums
and their part in cfg3w are.  Every test prints its figures as `MEASURE ...` before it asserts; the MI355X figures are in the
docstrings.
"""
import os

import numpy as np
import pytest
import torch

import cases
import hvp_options_extents as X
import hvp_vacuum_cases as V
import hvp_wgc_double as W
from professad_amd import _native as N
from professad_amd.engine import Engine

pytestmark = pytest.mark.gpu
GOLDEN = os.path.dirname(os.path.abspath(cases.__file__))
DEV = 'cuda:0'
FINDING = 1e-11
EPS = 2.0 ** -52
DECADES = [-6, -5, -4, -3, -2]
CHI_DECADES = [-6, -5, -4, -3, -2, -1]
# copies of MEASURED, MEASURED_Q and MEASURED_CHI of tests/test_hvp_vacuum_cpu.py (hv per decade of den; q relative to sum|w hv| dV;
# H d per decade of phi^2, d.H d and phi.H d relative to the sums of their terms' moduli, d mu relative to itself)
YARDSTICK = {
    'wgc99_nl': [3.15e-15, 6.18e-15, 9.31e-15, 3.94e-15, 2.90e-15],
    'cfg3w': [3.27e-14, 2.94e-14, 3.39e-14, 5.47e-14, 6.06e-14],
}
YARDSTICK_Q = {'wgc99_nl': 2.42e-15, 'pbe_x': 1.11e-14, 'pbe_c': 1.75e-14, 'cfg3w': 2.69e-16}
YARDSTICK_CHI = {
    'cfg3w': dict(Hd=[6.18e-15, 1.55e-14, 7.42e-14, 9.37e-14, 1.44e-13, 9.47e-14], dHd=1.36e-16, phiHd=2.13e-17, dmu=2.34e-15),
    'wgc99_nl_zero': dict(Hd=[1.84e-16, 1.14e-16, 1.20e-16, 9.64e-17, 4.55e-16, 6.08e-16], dHd=1.91e-17, phiHd=3.75e-18, dmu=3.35e-16),
}
# transforms of a product and of its reuse call (tests/test_hvp_wgc_gpu.py)
FFT = {'wgc99_nl': (24, 12), 'cfg3w': (42, 24)}
SUM_FLOOR = 10 * EPS          # ten roundings of a sum's terms, relative to the sum of their moduli


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.double, device=DEV)


def fmt(v):
    return '[' + ', '.join('%.2e' % f for f in v) + ']'


def per_decade(x, y, dec, decs):
    return [float(np.abs(x - y)[dec == k].max() / np.abs(y)[dec == k].max()) for k in decs]


_GOLD = []


def gold():
    """golden file and inputs, loaded once and shared"""
    if not _GOLD:
        g = np.load(os.path.join(GOLDEN, 'hvp_vacuum_v16s.npz'))
        box, den, _vext = V.make_inputs('v16s')
        w = V.direction(den)
        assert abs(cases.checksum(box, den, w) - float(g['checksum'])) < 1e-9
        _GOLD.append((g, box, den, w))
    return _GOLD[0]


def engine(shape, box, names):
    return Engine(shape, DEV).set_cell(box).set_terms(list(names)).set_option(N.OPT_HVP_WGC, 1).set_option(N.OPT_HVP_GGA, 1)


def check_decades(fig, yard):
    assert max(yard) <= FINDING / 10
    assert all(f <= 10 * y for f, y in zip(fig, yard)), fig


# ------------------------------------------------------------------------------- 1: n space against the goldens
@pytest.mark.parametrize('key', V.GPU_KEYS)
def test_vacuum_to_bulk_matches_the_reference_goldens(key):
    """Engine.hessian_vector(want_terms=True) on v16s for wgc99_nl alone and for cfg3w: hv per decade of den within 10 x the yardstick;
    sum_t q_t, and for cfg3w the entries of wgc99_nl, pbe_x and pbe_c against their single-term goldens, within 10 x theirs or ten
    roundings of sum|w hv_t| dV; sum_t q_t against the returned field within those ten roundings; everything finite; 24 / 12 and
    42 / 24 transforms; the reuse call returns the same bits.
    Measured on an MI355X, decades -6 .. -2 (yardstick in brackets):
        wgc99_nl hv 2.9e-15 4.3e-15 8.1e-15 3.8e-15 1.8e-15  (3.2e-15 6.2e-15 9.3e-15 3.9e-15 2.9e-15)
        cfg3w    hv 1.8e-14 3.0e-14 4.7e-14 4.9e-14 6.3e-14  (3.3e-14 2.9e-14 3.4e-14 5.5e-14 6.1e-14)
        q: wgc99_nl 8.1e-16 (2.4e-15), cfg3w 1.1e-15 (2.7e-16), and inside cfg3w pbe_x 9.6e-15 (1.1e-14), pbe_c 1.2e-14 (1.8e-14);
        sum q against the returned field 8.1e-16 for both.  The device is where the double is."""
    g, box, den, w = gold()
    dV = abs(np.linalg.det(box)) / den.size
    dec, decs = V.decades(den)
    assert decs == DECADES
    td, tw = dev(den), dev(w)
    eng = engine(den.shape, box, V.KEYS[key])
    q, hv = eng.hessian_vector(td, tw, want_terms=True)
    c0 = eng.query(N.Q_FFT_COUNT)
    q1, hv1 = eng.hessian_vector(td, tw, reuse_density=True, want_terms=True)
    c1 = eng.query(N.Q_FFT_COUNT)
    eng.close()
    hv_t = hv
    hv = hv.cpu().numpy()
    ref = g['hv_' + key]
    fig = per_decade(hv, ref, dec, decs)
    scale = lambda k: float(np.abs(w * g['hv_' + k]).sum() * dV)      # noqa: E731
    dq = {key: abs(sum(q.values()) - float(g['q_' + key])) / scale(key)}
    if key == 'cfg3w':
        for t in ('wgc99_nl', 'pbe_x', 'pbe_c'):
            dq[t] = abs(q[t] - float(g['q_' + t])) / scale(t)
    wh = w * hv
    dfield = abs(sum(q.values()) - float(wh.sum() * dV)) / float(np.abs(wh).sum() * dV)
    print('MEASURE hvp_vacuum %s: hv %s (yardstick %s)' % (key, fmt(fig), fmt(YARDSTICK[key])))
    print('MEASURE hvp_vacuum %s: q %s  sum q against the field %.2e  transforms %d / %d'
          % (key, ' '.join('%s %.2e (yardstick %.2e)' % (k, v, YARDSTICK_Q[k]) for k, v in dq.items()), dfield, c0, c1))
    assert np.isfinite(hv).all() and all(np.isfinite(v) for v in q.values())
    assert (c0, c1) == FFT[key]
    assert torch.equal(hv_t, hv1) and q == q1
    assert all(v == 0.0 for k, v in q.items() if k not in V.KEYS[key])
    check_decades(fig, YARDSTICK[key])
    for k, v in dq.items():
        assert v <= max(10 * YARDSTICK_Q[k], SUM_FLOOR) <= FINDING, (k, v)
    assert dfield <= SUM_FLOOR


# ------------------------------------------------------------------------------- 2: chi space against the double
def chi_call(eng, phi, d, gr, n_elec, reuse=False):
    return eng.hessian_vector_chi(dev(phi), dev(d), dev(gr), n_elec, reuse_density=reuse, want_scalars=True)


def chi_check(name, phi, d, s, Hd, sd, Hdd):
    dec, decs = V.decades(phi * phi)
    assert decs == CHI_DECADES
    fig = X.chi_figures(s, Hd, sd, Hdd, phi, d)
    fig['Hd'] = per_decade(Hd, Hdd, dec, decs)
    y = YARDSTICK_CHI[name]
    print('MEASURE hvp_vacuum chi %s: Hd %s (yardstick %s)  dHd %.2e  phiHd %.2e  dmu %.2e'
          % (name, fmt(fig['Hd']), fmt(y['Hd']), fig['dHd'], fig['phiHd'], fig['dmu']))
    assert np.isfinite(Hd).all() and all(np.isfinite(v) for v in s.values())
    check_decades(fig['Hd'], y['Hd'])
    assert fig['dHd'] <= max(10 * y['dHd'], SUM_FLOOR) and fig['phiHd'] <= max(10 * y['phiHd'], SUM_FLOOR)
    assert fig['dmu'] <= 10 * y['dmu'] <= FINDING


def test_chi_space_product_on_the_slab():
    """Engine.hessian_vector_chi at phi = 1.7 sqrt(den) for cfg3w with the unweighted direction (seed 83) and a made-up gradient made
    perpendicular to phi, against hvp_wgc_double.hessian_vector_chi: H d per decade of phi^2, d.H d, phi.H d, d mu; reuse is bitwise.
    Measured on an MI355X, decades -6 .. -1 of phi^2: H d 9.4e-15 2.7e-14 9.3e-14 1.2e-13 1.8e-13 2.0e-13 (yardstick 6.2e-15 1.6e-14
    7.4e-14 9.4e-14 1.4e-13 9.5e-14); d.H d 1.4e-16, phi.H d 2.3e-17, d mu 6.1e-15 (1.4e-16, 2.1e-17, 2.3e-15)."""
    _g, box, den, _w = gold()
    phi, d, gr, n_elec = V.chi_inputs(box, den)
    sd, Hdd = W.hessian_vector_chi(box, phi, d, gr, n_elec, V.CFG3W)
    eng = engine(den.shape, box, V.CFG3W)
    s, Hd = chi_call(eng, phi, d, gr, n_elec)
    c0 = eng.query(N.Q_FFT_COUNT)
    s1, Hd1 = chi_call(eng, phi, d, gr, n_elec, reuse=True)
    c1 = eng.query(N.Q_FFT_COUNT)
    eng.close()
    assert (c0, c1) == FFT['cfg3w']
    assert torch.equal(Hd, Hd1) and s == s1
    chi_check('cfg3w', phi, d, s, Hd.cpu().numpy(), sd, Hdd)


# ------------------------------------------------------------------------------- 3: chi of mixed sign
def test_a_chi_of_mixed_sign_is_the_positive_one_with_the_signs_put_back():
    """HvpChiGgaMidArgs and HvpChiWgcArgs form n = cs phi^2 and dn = 2 cs phi d - k n on the fly, even in every phi_j: with s = +-1 per
    point hessian_vector_chi(s phi, s d, s g) = s * hessian_vector_chi(phi, d, g) *bitwise*, scalars included (the numpy double gives a
    difference of exactly 0.0, tests/test_hvp_vacuum_cpu.py).  Measured on an MI355X: equal bits."""
    _g, box, den, _w = gold()
    phi, d, gr, n_elec = V.chi_inputs(box, den)
    sg = X.signs(phi.shape)
    assert 0.4 < (sg < 0).mean() < 0.6
    eng = engine(den.shape, box, V.CFG3W)
    s0, H0 = chi_call(eng, phi, d, gr, n_elec)
    s1, H1 = chi_call(eng, sg * phi, sg * d, sg * gr, n_elec)
    eng.close()
    print('MEASURE hvp_vacuum mixed-sign chi: max|H(s phi, s d, s g) - s H(phi, d, g)| = %.1e' % float((H1 - dev(sg) * H0).abs().max()))
    assert s0 == s1
    assert torch.equal(H1, dev(sg) * H0)


# ------------------------------------------------------------------------------- 4: a zero of chi
def test_a_zero_of_chi_with_wgc99_alone():
    """phi = 0 at one point (n = 0 there), term set ('wgc99_nl',): wgc_triple returns zeros where n is not positive -- n^(beta - 2) and
    n^(alpha - 2) are infinite at 0 -- and hvp_wgc_double.triple states the same rule; without it the transforms would spread NaN
    over the grid.  Finite everywhere, and within the bound of wgc99_nl against the double of the same inputs.
    A zero of phi with OFDFT_OPT_HVP_GGA = 1 and pbe_x / pbe_c in the term set is outside the contract (pbe_second documents n > 0)
    and untested.
    Measured on an MI355X, decades -6 .. -1 of phi^2: H d 4.2e-16 1.4e-16 1.9e-16 2.2e-16 1.3e-15 5.0e-16 (yardstick 1.8e-16 1.1e-16
    1.2e-16 9.6e-17 4.6e-16 6.1e-16); d.H d 9.5e-17, phi.H d 8.2e-18, d mu 8.9e-16; H d at the zero 1.6e-16 from the double's."""
    _g, box, den, _w = gold()
    phi, d, gr, n_elec = V.chi_inputs(box, den, zero=True)
    assert phi[V.ZERO_AT] == 0.0 and (phi == 0).sum() == 1
    sd, Hdd = W.hessian_vector_chi(box, phi, d, gr, n_elec, ('wgc99_nl',))
    assert np.isfinite(Hdd).all()
    eng = engine(den.shape, box, ('wgc99_nl',))
    s, Hd = chi_call(eng, phi, d, gr, n_elec)
    c0 = eng.query(N.Q_FFT_COUNT)
    eng.close()
    Hd = Hd.cpu().numpy()
    assert c0 == FFT['wgc99_nl'][0]
    chi_check('wgc99_nl_zero', phi, d, s, Hd, sd, Hdd)
    at = abs(Hd[V.ZERO_AT] - Hdd[V.ZERO_AT]) / abs(Hdd[V.ZERO_AT])
    print('MEASURE hvp_vacuum zero of chi: H d at the zero %.6e (double %.6e, %.2e apart)' % (Hd[V.ZERO_AT], Hdd[V.ZERO_AT], at))
    # -(2 a / S) g there and nothing else: the device's sums a = phi.d (which cancels) and S at 64 eps of sum|terms| (tests/test_cg_sweeps_gpu.py)
    assert at <= 64 * EPS * (float(np.abs(phi * d).sum()) / abs(sd['a']) + 1.0)
