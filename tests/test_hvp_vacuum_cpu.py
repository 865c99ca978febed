"""The yardsticks of tests/test_hvp_vacuum_gpu.py and tests/test_hvp_options_extents_gpu.py, without a device:

  * v16s (tests/golden/hvp_vacuum_cases.py: a slab whose density runs from 3.7e-2 to 1.6e-6): the numpy double
    (tests/hvp_wgc_double.py), the same formulas in long double (the doubles are generic in dtype and numpy's FFT keeps
    longdouble: a 64-bit-mantissa evaluation, no new maths) and the reference's double autograd (tests/golden/hvp_vacuum_v16s.npz),
    each against each, per key and per density decade floor(log10 den): max|x - y| over the decade / max|y| over the decade.
    The yardstick of a (key, decade) is the largest of the three figures.  q is a cancelling sum, so its figures are
    |q_x - q_y| / sum|w hv| dV.
  * a pointwise sweep of hvp_gga_double.second_partials in double against long double, n from 1e-6 to 1 and s from 0 to 31.6.
  * the chi-space double on v16s against long double, the sign-flip identity (a difference of exactly 0.0, as
    tests/test_second_order_doubles_cpu.py has it for cfg2) and what the double does at a zero of chi.
  * the doubles of the two grids past the block caps (tests/hvp_options_extents.py) against long double.

Every yardstick a GPU test uses must stay at or under 1e-12 (CAP), so that ten times it stays inside the 1e-11 that counts as a
finding; pbe_x and pbe_c alone on v16s do not (hvp_vacuum_cases.GPU_KEYS says why) and the GPU test leaves their fields out.
Every test prints its figures as `MEASURE ...` and asserts 10 x the tables below, measured with numpy 2 / torch 2 on x86-64 (long
double: the 80-bit format).  The tables of the two GPU files are copies; test_the_gpu_files_hold_copies_of_the_tables checks it.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import cases  # noqa: E402
import hvp_gga_double as H  # noqa: E402
import hvp_options_extents as X  # noqa: E402
import hvp_vacuum_cases as V  # noqa: E402
import hvp_wgc_double as W  # noqa: E402

LD = np.longdouble
CAP = 1e-12
EPS = 2.0 ** -52
DECADES = [-6, -5, -4, -3, -2]
# v16s, hv: per key the yardstick of the decades -6 .. -2 of den (the largest of double - long double, double - golden, golden - long double)
MEASURED = {
    'wgc99_nl': [3.15e-15, 6.18e-15, 9.31e-15, 3.94e-15, 2.90e-15],
    'pbe_x': [5.10e-12, 1.43e-12, 1.37e-12, 1.24e-12, 8.94e-13],
    'pbe_c': [1.68e-12, 1.73e-12, 1.59e-12, 1.51e-12, 1.38e-12],
    'cfg3w': [3.27e-14, 2.94e-14, 3.39e-14, 5.47e-14, 6.06e-14],
}
# ... q: the largest of the three |q_x - q_y| / sum|w hv| dV
MEASURED_Q = {'wgc99_nl': 2.42e-15, 'pbe_x': 1.11e-14, 'pbe_c': 1.75e-14, 'cfg3w': 2.69e-16}
# v16s in chi space, double against long double: H d per decade -6 .. -1 of phi^2, then d.H d and phi.H d relative to sum|d H d| and
# sum|phi H d|, d mu relative to itself.  cfg3w at phi = 1.7 sqrt(den); wgc99_nl alone with phi = 0 at one point
CHI_DECADES = [-6, -5, -4, -3, -2, -1]
MEASURED_CHI = {
    'cfg3w': dict(Hd=[6.18e-15, 1.55e-14, 7.42e-14, 9.37e-14, 1.44e-13, 9.47e-14], dHd=1.36e-16, phiHd=2.13e-17, dmu=2.34e-15),
    'wgc99_nl_zero': dict(Hd=[1.84e-16, 1.14e-16, 1.20e-16, 9.64e-17, 4.55e-16, 6.08e-16], dHd=1.91e-17, phiHd=3.75e-18, dmu=3.35e-16),
}
# pointwise sweep, max|double - long double| / |long double| of f_s, f_nn, f_ns, f_ss.  Exchange: 9e-14 is f_nn near its change of
# sign at s = 1.6, the others stay under 5e-15.  Correlation at s > 10 is the figure of H -> -eps_c: f and its partials are what is
# left of a cancellation (f_s = 1e-10 where exchange has 60); at s <= 10 it stays under 1.6e-11 (f_nn; the others under 6.7e-13)
MEASURED_POINTWISE = {'pbe_x': [7.72e-16, 9.02e-14, 5.03e-15, 1.02e-15], 'pbe_c': [9.58e-11, 1.61e-10, 2.02e-10, 2.24e-10]}
# the grids past the caps, double against long double: the figures of hvp_options_extents.hv_figures per term set, chi_figures
MEASURED_EXTENTS = {
    'A': dict(cfg3w=dict(hv=7.92e-16, q_hartree=5.55e-16, q_tf=2.45e-16, q_vw=3.20e-16, q_wgc99_nl=7.62e-16, q_pbe_x=2.00e-16, q_pbe_c=6.10e-16),
              wgc99_nl=dict(hv=5.45e-16, q_wgc99_nl=7.62e-16), pbe=dict(hv=4.53e-15, q_pbe_x=2.00e-16, q_pbe_c=6.10e-16),
              chi=dict(Hd=8.74e-16, dHd=3.26e-16, phiHd=1.86e-17, dmu=9.11e-15)),
    'B': dict(cfg3w=dict(hv=1.17e-15, q_hartree=2.73e-16, q_tf=3.63e-16, q_vw=3.55e-16, q_wgc99_nl=3.01e-16, q_pbe_x=9.08e-16, q_pbe_c=7.56e-16),
              wgc99_nl=dict(hv=1.00e-15, q_wgc99_nl=3.01e-16), pbe=dict(hv=3.71e-15, q_pbe_x=9.08e-16, q_pbe_c=7.56e-16),
              chi=dict(Hd=1.15e-15, dHd=4.87e-16, phiHd=4.59e-17, dmu=3.71e-14),
              cg=dict(x=8.73e-15)),          # three CG iterations: max|x - long double| / max|long double|
}


def per_decade(x, y, dec, decs):
    return [float(np.abs(x - y)[dec == k].max() / np.abs(y)[dec == k].max()) for k in decs]


def fmt(v):
    return '[' + ', '.join('%.2e' % f for f in v) + ']'


def within(fig, measured):
    """the 10 x rule against a recorded figure (a recorded 0 counts as one rounding)"""
    return fig <= 10 * max(measured, EPS)


@pytest.fixture(scope='module')
def v16s():
    g = np.load(os.path.join(HERE, 'golden', 'hvp_vacuum_v16s.npz'))
    box, den, _vext = V.make_inputs('v16s')
    w = V.direction(den)
    assert cases.checksum(box, den, w) == pytest.approx(float(g['checksum']), rel=1e-12)       # generator drift
    assert np.array_equal(w, g['w'])
    return g, box, den, w


def test_case_is_the_slab_it_is_meant_to_be(v16s):
    """the density range, the floor, about 1 500 points per decade, s from 1e-2 to 1e3, and N clear of the jumps of round(N)"""
    _g, box, den, _w = v16s
    nel = float(den.mean() * abs(np.linalg.det(box)))
    dec, decs = V.decades(den)
    k = H.k_vectors(box, den.shape)
    s = np.sqrt(sum(a * a for a in H.grad(k, den))) / (2 * (3 * np.pi ** 2) ** (1 / 3) * den ** (4 / 3))
    rs = (3 / (4 * np.pi * den)) ** (1 / 3)
    print('MEASURE hvp_vacuum cpu v16s: den %.3e .. %.3e  N %.4f  s %.1e .. %.1e  r_s %.2f .. %.1f  points per decade %s'
          % (den.min(), den.max(), nel, s.min(), s.max(), rs.min(), rs.max(), [int((dec == d).sum()) for d in decs]))
    assert den.min() >= V.DENSITY_FLOOR and 1.6e-6 < den.min() < 1.7e-6 and 3.7e-2 < den.max() < 3.8e-2
    assert decs == DECADES and min((dec == d).sum() for d in decs) > 1000
    assert abs(nel - 5.9003) < 1e-4 and abs(nel % 1.0 - 0.5) >= V.HALF_INTEGER_MARGIN
    assert s.min() < 2e-2 and s.max() > 5e2


@pytest.mark.parametrize('key', list(V.KEYS))
def test_yardsticks_of_v16s(v16s, key):
    """hv per decade and q: double, long double and golden, each against each; the largest is the yardstick.  Kept keys stay under CAP."""
    g, box, den, w = v16s
    dV = abs(np.linalg.det(box)) / den.size
    dec, decs = V.decades(den)
    q, hv = W.hessian_vector(box, den, w, V.KEYS[key])
    ql, hvl = W.hessian_vector(box, den.astype(LD), w.astype(LD), V.KEYS[key])
    assert hvl.dtype == LD
    gold, qg = g['hv_' + key], float(g['q_' + key])
    three = [per_decade(hv, hvl, dec, decs), per_decade(hv, gold, dec, decs), per_decade(gold, hvl, dec, decs)]
    yard = [max(col) for col in zip(*three)]
    scale = float(np.abs(w * gold).sum() * dV)
    qd, qld = sum(q.values()), float(sum(ql.values()))
    yq = max(abs(qd - qld), abs(qd - qg), abs(qg - qld)) / scale
    print('MEASURE hvp_vacuum cpu v16s %s: double - long double %s  double - golden %s  golden - long double %s' % ((key,) + tuple(fmt(t) for t in three)))
    print('MEASURE hvp_vacuum cpu v16s %s: yardstick hv %s  q %.2e  (q %.6e, |q| / sum|w hv| dV %.2f; max|hv| per decade %s)'
          % (key, fmt(yard), yq, qg, abs(qg) / scale, fmt([np.abs(gold)[dec == k].max() for k in decs])))
    assert all(within(f, m) for f, m in zip(yard, MEASURED[key])), yard
    assert within(yq, MEASURED_Q[key])
    assert yq <= CAP and MEASURED_Q[key] <= CAP            # the sums of every key are compared on the device
    # the keys whose fields the GPU test compares are exactly those under the cap
    assert (max(MEASURED[key]) <= CAP) == (key in V.GPU_KEYS)
    if key in V.GPU_KEYS:
        assert max(yard) <= CAP


def test_pointwise_second_partials_against_long_double():
    """hvp_gga_double.second_partials on n in logspace(-6, 0), s in {0} + logspace(-3, 1.5), sigma = (2 k_F n s)^2: every partial finite,
    and its largest relative deviation from long double per term"""
    n = np.logspace(-6, 0, 61)[:, None]
    s = np.concatenate([[0.0], np.logspace(-3, 1.5, 46)])[None, :]
    sigma = (2 * (3 * np.pi ** 2 * n) ** (1 / 3) * n * s) ** 2
    n = n * np.ones_like(sigma)
    for term in ('pbe_x', 'pbe_c'):
        pd = H.second_partials(n, sigma, term)
        pl = H.second_partials(n.astype(LD), sigma.astype(LD), term)
        assert all(np.isfinite(a).all() for a in pd) and pl[0].dtype == LD
        rel = [np.abs(a - b) / np.abs(b) for a, b in zip(pd, pl)]
        fig = [float(r.max()) for r in rel]
        low = [float(r[:, s[0] <= 10].max()) for r in rel]
        print('MEASURE hvp_vacuum cpu pointwise %s: f_s, f_nn, f_ns, f_ss %s  (s <= 10: %s)' % (term, fmt(fig), fmt(low)))
        assert all(within(f, m) for f, m in zip(fig, MEASURED_POINTWISE[term])), fig


def chi_yardstick(box, phi, d, gr, n_elec, names):
    sd, Hd = W.hessian_vector_chi(box, phi, d, gr, n_elec, names)
    sl, Hl = W.hessian_vector_chi(box, phi.astype(LD), d.astype(LD), gr.astype(LD), n_elec, names)
    assert Hl.dtype == LD
    dec, decs = V.decades(phi * phi)
    assert decs == CHI_DECADES
    fig = X.chi_figures(sd, Hd, sl, Hl, phi, d)
    fig['Hd'] = per_decade(Hd, Hl, dec, decs)
    return sd, Hd, fig


def check_chi(name, fig):
    m = MEASURED_CHI[name]
    print('MEASURE hvp_vacuum cpu v16s chi %s: Hd %s  dHd %.2e  phiHd %.2e  dmu %.2e' % (name, fmt(fig['Hd']), fig['dHd'], fig['phiHd'], fig['dmu']))
    assert all(within(f, y) for f, y in zip(fig['Hd'], m['Hd'])) and max(fig['Hd']) <= CAP and max(m['Hd']) <= CAP
    for k in ('dHd', 'phiHd', 'dmu'):
        assert within(fig[k], m[k]) and fig[k] <= CAP and m[k] <= CAP, (k, fig[k])


def test_chi_space_double_on_v16s_and_the_sign_flip_identity(v16s):
    """cfg3w at phi = 1.7 sqrt(den) with the unweighted direction: the double against long double per decade of phi^2; with s = +-1
    per point hessian_vector_chi(s phi, s d, s g) - s hessian_vector_chi(phi, d, g) is exactly 0.0 and the scalars are the same numbers"""
    _g, box, den, _w = v16s
    phi, d, gr, n_elec = V.chi_inputs(box, den)
    s0, H0, fig = chi_yardstick(box, phi, d, gr, n_elec, V.CFG3W)
    check_chi('cfg3w', fig)
    sg = X.signs(phi.shape)
    assert 0.4 < (sg < 0).mean() < 0.6
    s1, H1 = W.hessian_vector_chi(box, sg * phi, sg * d, sg * gr, n_elec, V.CFG3W)
    diff = float(np.abs(H1 - sg * H0).max())
    print('MEASURE hvp_vacuum cpu v16s sign flip: max|H(s phi, s d, s g) - s H(phi, d, g)| = %.1e' % diff)
    assert diff == 0.0 and s0 == s1


def test_double_at_a_zero_of_chi(v16s):
    """phi = 0 at one point, wgc99_nl alone: the double states the device's rule (f = f' = f'' = 0 where n is not positive), so it is
    finite everywhere, H d at the zero is -(2 a / S) g to the bit, and the rest sits where the case without the zero does.  Without
    the rule n ** (e - 2) is infinite there and the transforms spread NaN over the whole grid."""
    _g, box, den, _w = v16s
    phi, d, gr, n_elec = V.chi_inputs(box, den, zero=True)
    assert phi[V.ZERO_AT] == 0.0 and (phi == 0).sum() == 1
    sd, Hd, fig = chi_yardstick(box, phi, d, gr, n_elec, ('wgc99_nl',))
    check_chi('wgc99_nl_zero', fig)
    assert np.isfinite(Hd).all() and all(np.isfinite(v) for v in sd.values())
    assert Hd[V.ZERO_AT] == -(2 * sd['a'] / sd['S']) * gr[V.ZERO_AT]
    for e in W.PARAMS[:2]:                  # the rule itself: all nine entries are 0 at n = 0 and at n < 0
        for n0 in (0.0, -1e-3):
            assert all(float(x[0]) == 0.0 for part in W.triple(np.array([n0]), np.array([n0 - 0.01]), e) for x in part)


@pytest.fixture(scope='module', params=['A', 'B'])
def extents(request):
    key = request.param
    return key, X.inputs(key), X.per_term(key), X.per_term(key, LD)


@pytest.mark.parametrize('name', list(X.SETS))
def test_n_space_doubles_past_the_caps_against_long_double(extents, name):
    """cfg3w, wgc99_nl alone and pbe_x + pbe_c alone on (128, 128, 64) and (81, 81, 81): hv and every q_t"""
    key, i, td, tl = extents
    nel = float(i['den'].mean() * abs(np.linalg.det(i['box'])))
    assert abs(nel - {'A': 957.81, 'B': 242.73}[key]) < 0.01
    (q, hv), (ql, hvl) = X.set_product(td, X.SETS[name]), X.set_product(tl, X.SETS[name])
    assert hvl.dtype == LD
    fig = X.hv_figures(q, hv, ql, hvl)
    print('MEASURE hvp_vacuum cpu extents %s %s: %s' % (key, name, ' '.join('%s %.2e' % kv for kv in fig.items())))
    m = MEASURED_EXTENTS[key][name]
    assert set(fig) == set(m)
    assert all(within(v, m[k]) and v <= CAP and m[k] <= CAP for k, v in fig.items()), fig


def test_chi_space_doubles_past_the_caps_against_long_double(extents):
    key, i, _td, _tl = extents
    (sd, Hd), (sl, Hl) = X.chi_product(key), X.chi_product(key, LD)
    assert Hl.dtype == LD
    fig = X.chi_figures(sd, Hd, sl, Hl, i['phi'], i['d'])
    print('MEASURE hvp_vacuum cpu extents %s chi: %s' % (key, ' '.join('%s %.2e' % kv for kv in fig.items())))
    m = MEASURED_EXTENTS[key]['chi']
    assert set(fig) == set(m)
    assert all(within(v, m[k]) and v <= CAP and m[k] <= CAP for k, v in fig.items()), fig


def test_three_cg_iterations_past_the_caps_against_long_double():
    """B: three iterations of optimize.solve_projected on hvp_wgc_double.NumpyCgBackend in double and in long double (its scalars stay
    doubles: one rounding each, below what is measured).  The iterations amplify the deviation of a product about eight times."""
    x, it, reason, _rel, nprod = X.numpy_cg('B')
    xl, itl, reasonl, _rell, nprodl = X.numpy_cg('B', LD)
    assert xl.dtype == LD and (it, reason, nprod) == (itl, reasonl, nprodl) == (3, W.T.CG_MAXITER, 3)
    fig = float(np.abs(x - xl).max() / np.abs(xl).max())
    print('MEASURE hvp_vacuum cpu extents B cg: x %.2e' % fig)
    m = MEASURED_EXTENTS['B']['cg']['x']
    assert within(fig, m) and fig <= CAP and m <= CAP


def test_the_gpu_files_hold_copies_of_the_tables():
    import test_hvp_options_extents_gpu as GX
    import test_hvp_vacuum_gpu as GV
    assert GV.YARDSTICK == {k: MEASURED[k] for k in V.GPU_KEYS} and GV.YARDSTICK_Q == MEASURED_Q and GV.YARDSTICK_CHI == MEASURED_CHI
    assert GV.DECADES == DECADES and GV.CHI_DECADES == CHI_DECADES
    assert GX.YARDSTICK == MEASURED_EXTENTS
