"""CPU-side checks of the Huang-Carter kinds of OFDFT_NLK (HuangCarter, RevisedHuangCarter): the numpy double of the closed form
the engine evaluates (tests/hc_double.py) against the reference's forward + autograd (tests/golden/hc_<case>.npz; generator
tests/golden/make_golden_hc.py), the kernel table of professad_amd.hc_kernel, and the host side (slots, kinds, exports, the
drop-in classes' refusal of a differentiable cell)."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import cases
import hc_cases
import hc_double
from professad_amd import _native as N
from professad_amd import functionals as F
from professad_amd import hc_kernel

GOLDEN = os.path.dirname(os.path.abspath(cases.__file__))
# the bounds of the GPU parity test (tests/spectral_check.py: E_TOL['f64'], V_TOL['f64']), which this double has to meet as well
E_TOL, V_TOL = 1e-13, 1.5e-12


def table(key):
    return hc_kernel.solve_kernel(hc_cases.beta_of(key), hc_cases.ETA_MAX, hc_cases.N_ETA)


# ------------------------------------------------------------------------------- 1: the numpy double against the reference
@pytest.mark.parametrize('case', hc_cases.CASES)
@pytest.mark.parametrize('key', list(hc_cases.KINDS))
def test_numpy_double_matches_reference_golden(case, key):
    """Measured (this double against the reference's autograd): dE_nl / |E_total| <= 7.7e-17, dv_nl / max|v_nl| <= 3.6e-14
    over the eight (case, kind) pairs (1.1e-14 without g16w); the node sets agree."""
    gold = np.load(os.path.join(GOLDEN, 'hc_%s.npz' % case))
    box, den = hc_cases.make_inputs(case)
    assert abs(cases.checksum(box, den) - float(gold['checksum'])) < 1e-9
    eta, w = table(key)
    r = hc_double.hc_energy_potential(key, hc_cases.KINDS[key][1], box, den, eta, w)
    E_tot = float(gold[key + '_E'])
    v_ref = gold[key + '_v_nl']
    err_E = abs(r['E_nl'] - float(gold[key + '_E_nl'])) / abs(E_tot)
    err_v = float(np.abs(r['v_nl'] - v_ref).max() / np.abs(v_ref).max())
    print('%s %s: dE %.2e dv %.2e M %d intervals %d' % (case, key, err_E, err_v, r['M'], r['touched']))
    assert err_E <= E_TOL and err_v <= V_TOL
    assert r['M'] == int(gold[key + '_M'])
    assert r['xi_min'] == pytest.approx(float(gold[key + '_xi_min']), rel=1e-13)
    assert r['xi_max'] == pytest.approx(float(gold[key + '_xi_max']), rel=1e-13)
    assert r['lower'] == pytest.approx(float(gold[key + '_lower']), rel=1e-13)
    # the functional's total: vW + TF restated as well
    E_rest, v_rest = hc_double.tf_vw(box, den)
    assert abs(E_rest + r['E_nl'] - E_tot) <= E_TOL * abs(E_tot)
    assert np.abs(v_rest + r['v_nl'] - gold[key + '_v']).max() <= V_TOL * np.abs(gold[key + '_v']).max()


def test_wide_case_touches_many_intervals_and_plain_cases_three():
    for key, want in (('hc', 34), ('revhc', 14)):
        box, den = hc_cases.make_inputs('g16w')
        r = hc_double.hc_energy_potential(key, hc_cases.KINDS[key][1], box, den, *table(key))
        assert r['touched'] == want and r['M'] == {'hc': 40, 'revhc': 21}[key]
    box, den = hc_cases.make_inputs('g16r')
    assert hc_double.hc_energy_potential('hc', hc_cases.HC_ARGS, box, den, *table('hc'))['touched'] == 3


def test_node_set_margin_of_the_fixtures():
    """neither ceil argument of the node formulas within 1e-6 of an integer: rounding in xi_min / xi_max cannot move the node set"""
    for case in hc_cases.CASES:
        gold = np.load(os.path.join(GOLDEN, 'hc_%s.npz' % case))
        for key in hc_cases.KINDS:
            _lower, M, a, b = hc_cases.node_set(float(gold[key + '_xi_min']), float(gold[key + '_xi_max']), hc_cases.kappa_of(key))
            assert M == int(gold[key + '_M'])
            assert min(abs(a - round(a)), abs(b - round(b))) > 1e-6, (case, key)


EDGE = [(case, key) for case, spec in hc_cases.EDGE_CASES.items() for key in spec['keys']]
_EDGE_DOUBLE = {}


def edge_double(case, key):
    """the numpy double of an edge case (hc_cases.EDGE_CASES) with the case's table and kappa, computed once and shared"""
    if (case, key) not in _EDGE_DOUBLE:
        box, den = hc_cases.make_inputs(hc_cases.EDGE_CASES[case]['grid'])
        eta, w = hc_kernel.solve_kernel(hc_cases.beta_of(key), *hc_cases.edge_table(case))
        _EDGE_DOUBLE[case, key] = (box, den, eta, hc_double.hc_energy_potential(key, hc_cases.edge_args(case, key), box, den, eta, w))
    return _EDGE_DOUBLE[case, key]


@pytest.mark.parametrize('case,key', EDGE)
def test_numpy_double_matches_edge_golden(case, key):
    """The short-table, M = 64 and (20, 18, 33) goldens, at the bounds of the test above.  Measured (dE_nl / |E_total|, dv_nl /
    max|v_nl|): g16r_t8 hc 2.6e-17 8.0e-15, revhc 6.5e-17 1.0e-14; g18t_t8 hc 5.8e-17 1.1e-14, revhc 4.4e-17 1.2e-14;
    g16w_m64 hc 3.4e-17 2.9e-14; g20x33 hc 7.3e-18 9.8e-15, revhc 2.8e-17 1.2e-14 -- all below a tenth of the bounds, so the GPU
    tests of these goldens (tests/test_hc_edges_gpu.py) keep the parity bounds as they are."""
    gold = np.load(os.path.join(GOLDEN, 'hc_%s.npz' % case))
    box, den, _eta, r = edge_double(case, key)
    assert abs(cases.checksum(box, den) - float(gold['checksum'])) < 1e-9
    assert sorted(gold.files) == sorted(['checksum'] + [k + s for k in hc_cases.EDGE_CASES[case]['keys']
                                                        for s in ('_E', '_E_nl', '_v_nl', '_xi_min', '_xi_max', '_lower', '_M')])
    E_tot = float(gold[key + '_E'])
    v_ref = gold[key + '_v_nl']
    err_E = abs(r['E_nl'] - float(gold[key + '_E_nl'])) / abs(E_tot)
    err_v = float(np.abs(r['v_nl'] - v_ref).max() / np.abs(v_ref).max())
    print('%s %s: dE %.2e dv %.2e M %d intervals %d' % (case, key, err_E, err_v, r['M'], r['touched']))
    assert err_E <= E_TOL and err_v <= V_TOL
    assert r['M'] == int(gold[key + '_M'])
    for k in ('xi_min', 'xi_max', 'lower'):
        assert r[k] == pytest.approx(float(gold[key + '_' + k]), rel=1e-13)
    assert abs(hc_double.tf_vw(box, den)[0] + r['E_nl'] - E_tot) <= E_TOL * abs(E_tot)
    kappa = hc_cases.edge_args(case, key)[-1]
    _lower, M, a, b = hc_cases.node_set(float(gold[key + '_xi_min']), float(gold[key + '_xi_max']), kappa)
    assert M == r['M'] and min(abs(a - round(a)), abs(b - round(b))) > 1e-6


@pytest.mark.parametrize('case,key', [(c, k) for c, k in EDGE if hc_cases.EDGE_CASES[c]['table']])
def test_short_table_clamps_a_share_of_the_pairs_and_moves_the_potential(case, key):
    """The condition that makes the short-table goldens a test of hc_table_interp's clamp, from numpy alone: of the (k-point, node)
    pairs over the nodes some point's spline reads, at least a tenth lie past the table's end (q / xi_j > eta_max) and at least a
    tenth inside it.  Measured: g16r_t8 20.7 % (hc), 20.7 % (revhc); g18t_t8 20.7 %, 20.9 %.  With the default table the same
    pairs are all inside (largest q / xi_j 17.1), and v_nl differs by 5.8e-4 .. 6.9e-4 of its maximum: eight orders above the
    parity bound."""
    box, den, eta, r = edge_double(case, key)
    eta_max = float(eta[-1])
    assert eta_max == hc_cases.edge_table(case)[0] and len(eta) == hc_cases.edge_table(case)[1]
    first, last = r['used']
    assert 0 <= first < last < r['M']
    ratio = r['q'][..., None] / r['nodes'][first:last + 1]
    above, below = float(np.mean(ratio > eta_max)), float(np.mean(ratio < eta_max))
    default = hc_double.hc_energy_potential(key, hc_cases.edge_args(case, key), box, den, *table(key))
    moved = float(np.abs(default['v_nl'] - r['v_nl']).max() / np.abs(r['v_nl']).max())
    print('%s %s: %.1f %% of %d pairs clamped, %.1f %% inside, largest q / xi_j %.1f, v_nl moves by %.2e' % (
        case, key, 100 * above, ratio.size, 100 * below, ratio.max(), moved))
    assert above >= 0.10 and below >= 0.10
    assert ratio.max() < hc_cases.ETA_MAX and moved > 1e-5


def test_m64_case_fills_the_node_cap_and_its_neighbour_exceeds_it():
    """g16w at hc_cases.KAPPA_M64 needs exactly the 64 nodes an evaluation carries (M + 3 = 67 transforms forward: no multiple of the
    batch of 4), at KAPPA_M65 one more; both with ceil margins far above rounding"""
    _box, _den, _eta, r = edge_double('g16w_m64', 'hc')
    assert r['M'] == 64 and (r['M'] + 3) % 4 != 0
    for kappa, want in ((hc_cases.KAPPA_M64, 64), (hc_cases.KAPPA_M65, 65)):
        _lower, M, a, b = hc_cases.node_set(r['xi_min'], r['xi_max'], kappa)
        assert M == want and min(abs(a - round(a)), abs(b - round(b))) > 0.1


# ------------------------------------------------------------------------------- 2: the kernel table
@pytest.mark.parametrize('key', list(hc_cases.KINDS))
def test_table_matches_fixture_and_boundary_values(key):
    gold = np.load(os.path.join(GOLDEN, 'hc_g16r.npz'))
    beta = hc_cases.beta_of(key)
    eta, w = table(key)
    w_inf = -(8 / 3) / ((5 - 3 * beta) * beta)
    assert eta.shape == w.shape == (hc_cases.N_ETA,) and eta[0] == 0.0 and eta[-1] == hc_cases.ETA_MAX
    assert w[0] == 0.0 and w[-1] == w_inf
    assert np.abs(w - gold[key + '_table']).max() <= 1e-14 * abs(w_inf)
    assert hc_kernel.solve_kernel(beta, hc_cases.ETA_MAX, hc_cases.N_ETA)[1] is w             # cached per argument tuple
    assert not w.flags.writeable


@pytest.mark.parametrize('key', list(hc_cases.KINDS))
def test_table_converges_with_the_node_count(key):
    """N_eta against 2 N_eta - 1 on the shared nodes: an RK4 truncation estimate.  Measured max |dw| / |w_inf|: 3.93e-5 (hc,
    beta = 0.7143) and 4.14e-5 (revhc, beta = 2/3), both at the first node above 0, where the ODE's 1 / eta is largest; the bound is
    the larger figure with a margin of 4.  (The logarithmic point of the Lindhard function at eta = 1 lowers the local order, so
    the bound is measured, not derived.)"""
    beta = hc_cases.beta_of(key)
    n = hc_cases.N_ETA
    _e1, w1 = hc_kernel.solve_kernel(beta, hc_cases.ETA_MAX, n)
    _e2, w2 = hc_kernel.solve_kernel(beta, hc_cases.ETA_MAX, 2 * n - 1)
    w_inf = -(8 / 3) / ((5 - 3 * beta) * beta)
    d = np.abs(w1 - w2[::2]) / abs(w_inf)
    print(key, 'max |dw| / |w_inf| %.3e at node %d' % (d.max(), int(d.argmax())))
    assert d.max() <= TABLE_STEP_BOUND


TABLE_STEP_BOUND = 4 * 4.14e-5


def test_solve_kernel_refuses_bad_arguments():
    for bad in (0.0, 5 / 3, -0.1):
        with pytest.raises(ValueError, match='beta'):
            hc_kernel.solve_kernel(bad)
    with pytest.raises(ValueError, match='n_eta'):
        hc_kernel.solve_kernel(0.7, 50.0, 3)


# ------------------------------------------------------------------------------- 3: host side
def test_slots_and_kinds_agree_with_the_header():
    header = open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'ofdft_hip.h')).read()
    defs = dict(re.findall(r'#define\s+(OFDFT_\w+)\s+(-?\d+)\b', header))
    assert int(defs['OFDFT_P_NLK_P3']) == N.P_NLK_P3 == 17 and int(defs['OFDFT_NPARAMS']) == N.NPARAMS == 18
    assert int(defs['OFDFT_P_NLK_P2']) == N.P_NLK_P2 == 16 and int(defs['OFDFT_P_NLK_KIND']) == N.P_NLK_KIND == 13
    assert (N.NLK_HC, N.NLK_REVHC) == (4, 5) and N.NTERMS == int(defs['OFDFT_NTERMS']) == 15
    assert 'ofdft_set_nlk_table' in header and 'ofdft_set_nlk_table' in N.EXPORTS
    kernels = open(os.path.join(os.path.dirname(GOLDEN), '..', 'professad_amd', 'csrc', 'hc_kernels.h')).read()
    assert re.search(r'NLK_HC = 4, NLK_REVHC = 5', kernels) and re.search(r'kHcMaxNodes = 64', kernels)


def test_both_libraries_export_the_table_entry():
    import __graft_entry__
    __graft_entry__.build()
    for dtype in (N.F64, N.F32):
        assert hasattr(N.load(dtype), 'ofdft_set_nlk_table')


def test_drop_in_classes_names_tables_and_refusal_of_a_differentiable_cell():
    hc, rhc = F.HuangCarter(hc_cases.HC_ARGS), F.RevisedHuangCarter(hc_cases.REVHC_ARGS)
    assert hc.__qualname__ == hc.__name__ == 'HuangCarter' and rhc.__qualname__ == rhc.__name__ == 'RevisedHuangCarter'
    assert (hc.lamb, hc.beta, hc.kappa) == hc_cases.HC_ARGS and (rhc.a, rhc.b, rhc.beta, rhc.kappa) == hc_cases.REVHC_ARGS
    for f in (hc, rhc):
        assert list(inspect.signature(f.forward).parameters) == ['box_vecs', 'den'] and callable(f)
        assert list(inspect.signature(f.generate_kernel).parameters) == ['eta_max', 'N_eta']
        assert f.kernel.shape == (2, 10000) and f.kernel.dtype == torch.double
        eta, w = hc_kernel.solve_kernel(f.beta)
        assert np.array_equal(f.kernel[0].numpy(), eta) and np.array_equal(f.kernel[1].numpy(), w)
        box = torch.eye(3, dtype=torch.double).requires_grad_()
        with pytest.raises(NotImplementedError, match='no stress'):
            f(box, torch.ones(4, 4, 4, dtype=torch.double))
    hc.generate_kernel(eta_max=20, N_eta=500)
    assert hc.kernel.shape == (2, 500) and float(hc.kernel[0, -1]) == 20.0
    assert dict(hc._params())['nlk_kind'] == 4.0 and dict(rhc._params())['nlk_p3'] == hc_cases.REVHC_ARGS[3]
