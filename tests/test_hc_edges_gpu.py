"""GPU tests of the branches of the Huang-Carter chain (OFDFT_NLK kinds 4 and 5; csrc/hc_kernels.h, csrc/engine_hc.inc.h) that
tests/test_hc_gpu.py does not reach: the end of the kernel table, the node cap from both sides, a grid of three unequal extents
with an odd last one, second and ragged trips of every grid-stride loop, where the extrema of xi lie, densities that are not
positive, the parameter edges and the state around the chain.  Each test states next to it, or asserts from numpy, the
condition on its inputs that makes the branch reached.

References: the reference's forward + autograd (tests/golden/hc_<case>.npz of hc_cases.EDGE_CASES; generator
tests/golden/make_golden_hc.py) and the numpy double of the closed form (tests/hc_double.py).  Bounds are the project's fp64
parity bounds (tests/spectral_check.py): energies E_TOL['f64'] of |E_total|, fields V_TOL['f64'] of their maximum.  The numpy
double deviates from every new golden by less than a tenth of these (tests/test_hc_cpu.py::test_numpy_double_matches_edge_golden:
at most 6.5e-17 and 2.9e-14), so no case has a bound of its own.  Every test prints its figures before it asserts; the figures
measured on an MI355X stand in the docstrings.
"""
import os
import re

import numpy as np
import pytest
import torch

import cases
import hc_cases
import hc_double
from spectral_check import E_TOL, V_TOL
from professad_amd import _native as N
from professad_amd import functionals as F
from professad_amd import hc_kernel
from professad_amd import synth
from professad_amd.engine import Engine

pytestmark = pytest.mark.gpu
GOLDEN = os.path.dirname(os.path.abspath(cases.__file__))
DEV = 'cuda:0'
ETOL, VTOL = E_TOL['f64'], V_TOL['f64']
KEYS = list(hc_cases.KINDS)
EDGE = [(case, key) for case, spec in hc_cases.EDGE_CASES.items() for key in spec['keys']]
NAMES = ('tf', 'vw', 'nlk')
CLOSURE_NAMES = ('ion_electron', 'hartree', 'tf', 'vw', 'nlk', 'lda_x')
NOT_POSITIVE = r'xi\(r\) must be positive and finite'
# launch geometry of the chain (csrc/engine_ctx.h grid_for, csrc/pointwise_kernels.h kRedBlocks / kRedThreads)
SPEC_TRIP = 2048 * 256            # threads of the spectral kernels, the maps and the epilogue
RED_TRIP = 1024 * 256             # threads of the reducing kernels (min / max, gather, tail)


def dev(a, dtype=torch.double):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def maxerr(a, b):
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b)) / np.abs(b).max())


def params(key, **over):
    p = dict(hc_cases.KINDS[key][2])
    p.update(over)
    return p


def chain_transforms(eng, td, p):
    """transforms of the term's own chain: OFDFT_Q_FFT_COUNT of (tf, vw, nlk) minus that of (tf, vw); 2 M + 10"""
    eng.set_terms(NAMES, p)
    eng.energy_potential(td)
    full = eng.query(N.Q_FFT_COUNT)
    eng.set_terms(('tf', 'vw'))
    eng.energy_potential(td)
    return int(full - eng.query(N.Q_FFT_COUNT))


def margins(xi_min, xi_max, kappa):
    """(M, the smaller distance of the two ceil arguments of the node formulas to an integer)"""
    _lower, M, a, b = hc_cases.node_set(xi_min, xi_max, kappa)
    return M, min(abs(a - round(a)), abs(b - round(b)))


def two_kf(n):
    return 2.0 * (3.0 * np.pi ** 2 * n) ** (1.0 / 3.0)


# ------------------------------------------------------------------------------- 1 - 3: the new goldens
@pytest.mark.parametrize('case,key', EDGE)
def test_engine_and_drop_in_match_edge_golden(case, key):
    """g16r_t8, g18t_t8: a table of 1601 nodes up to eta_max = 8, past whose end 20.7 .. 21.0 % of the (k-point, node) pairs lie
    (asserted from numpy in tests/test_hc_cpu.py): hc_table_interp's clamp of eta and of the last interval.  The engine takes the
    table through the nlk_eta_max / nlk_n_eta keys of set_terms, the drop-in classes through generate_kernel(8, 1601); the result
    with the default table on the same context differs by more than 1e-5 of max|v_nl| (3e-4 .. 7e-4 in the double).
    g16w_m64: 64 nodes, the most an evaluation carries (67 forward transforms: a last batch of 3).
    g20x33: (20, 18, 33) in a triclinic cell: three unequal extents with an odd last one.
    Measured on an MI355X over the seven pairs, engine and drop-in: dE_nl <= 6.5e-17 and dE <= 5.9e-16 of |E_total|, dv_nl <= 2.9e-14
    (g16w_m64) and dv <= 5.4e-14 (g20x33) of the maximum; the default table moves v_nl by 5.8e-4 .. 6.9e-4 (per case: MEASURED)."""
    spec = hc_cases.EDGE_CASES[case]
    gold = np.load(os.path.join(GOLDEN, 'hc_%s.npz' % case))
    box, den = hc_cases.make_inputs(spec['grid'])
    assert abs(cases.checksum(box, den) - float(gold['checksum'])) < 1e-9
    tb, td = dev(box), dev(den)
    E_ref, E_nl_ref, v_nl_ref = float(gold[key + '_E']), float(gold[key + '_E_nl']), gold[key + '_v_nl']
    v_ref = hc_double.tf_vw(box, den)[1] + v_nl_ref            # (the new goldens store the nonlocal part only)
    p = hc_cases.edge_params(case, key)
    eng = Engine(den.shape, DEV).set_cell(box)
    eng.set_terms(NAMES, p)
    E_terms, v = eng.energy_potential(td)
    eng.set_terms(('nlk',), p)
    E_only, v_nl = eng.energy_potential(td)
    E = sum(E_terms.values())
    figs = (abs(E_terms['nlk'] - E_nl_ref) / abs(E_ref), abs(E - E_ref) / abs(E_ref), maxerr(v_nl.cpu().numpy(), v_nl_ref),
            maxerr(v.cpu().numpy(), v_ref))
    print('%s %s engine: dE_nl %.2e dE %.2e dv_nl %.2e dv %.2e' % ((case, key) + figs))
    assert figs[0] <= ETOL and figs[1] <= ETOL, (case, key, E_terms, E_ref, E_nl_ref)
    assert figs[2] <= VTOL and figs[3] <= VTOL, (case, key)
    assert E_only['nlk'] == E_terms['nlk']
    if spec['table']:
        p_default = {k: x for k, x in p.items() if k not in ('nlk_eta_max', 'nlk_n_eta')}
        eng.set_terms(('nlk',), p_default)
        _E, v_default = eng.energy_potential(td)
        moved = maxerr(v_default.cpu().numpy(), v_nl_ref)
        print('%s %s: the default table moves v_nl by %.2e of its maximum' % (case, key, moved))
        assert moved > 1e-5
        eng.set_terms(('nlk',), p)              # and back: the short table again, the same bits
        _E, v_back = eng.energy_potential(td)
        assert torch.equal(v_back, v_nl)
    assert chain_transforms(eng, td, p) == 2 * int(gold[key + '_M']) + 10
    eng.close()
    # the drop-in class
    f = getattr(F, hc_cases.KINDS[key][0])(hc_cases.edge_args(case, key))
    if spec['table']:
        v_default = F.get_functional_derivative(tb, td, f).cpu().numpy()
        f.generate_kernel(*spec['table'])
    Ef = float(f(tb, td))
    vf = F.get_functional_derivative(tb, td, f).cpu().numpy()
    print('%s %s drop-in: dE %.2e dv %.2e' % (case, key, abs(Ef - E_ref) / abs(E_ref), maxerr(vf, v_ref)))
    assert abs(Ef - E_ref) <= ETOL * abs(E_ref) and float(f.forward(tb, td)) == Ef
    assert maxerr(vf, v_ref) <= VTOL
    if spec['table']:
        assert np.abs(v_default - vf).max() > 1e-5 * np.abs(v_nl_ref).max()


def test_sixty_four_nodes_are_served_and_sixty_five_refused():
    """g16w at hc_cases.KAPPA_M64 (64 nodes; parity in the test above) and at KAPPA_M65 (65: ceil margins of both above 0.29,
    tests/test_hc_cpu.py): the 65-node evaluation is refused by name with the counters of the served one left as they were, through
    both entry points, and the 64-node evaluation afterwards returns the bits it returned before"""
    box, den = hc_cases.make_inputs('g16w')
    gold = np.load(os.path.join(GOLDEN, 'hc_g16w_m64.npz'))
    assert int(gold['hc_M']) == 64
    assert margins(float(gold['hc_xi_min']), float(gold['hc_xi_max']), hc_cases.KAPPA_M65)[0] == 65
    td = dev(den)
    p64, p65 = hc_cases.edge_params('g16w_m64', 'hc'), params('hc', nlk_p2=hc_cases.KAPPA_M65)
    eng = Engine(den.shape, DEV).set_cell(box)
    assert chain_transforms(eng, td, p64) == 2 * 64 + 10
    eng.set_terms(NAMES, p64)
    E, v = eng.energy_potential(td)
    launches, ffts = eng.query(N.Q_LAUNCH_COUNT), eng.query(N.Q_FFT_COUNT)
    eng.set_terms(NAMES, p65)
    with pytest.raises(RuntimeError, match=r'xi_min = .*xi_max = .*kappa = 1\.1095.*M = 65 spline nodes, more than the 64'):
        eng.energy_potential(td)
    assert eng.query(N.Q_LAUNCH_COUNT) == launches and eng.query(N.Q_FFT_COUNT) == ffts
    with pytest.raises(RuntimeError, match='M = 65'):
        eng.energy_grad_chi(dev(np.sqrt(den)), float(den.mean() * abs(np.linalg.det(box))))
    assert eng.query(N.Q_LAUNCH_COUNT) == launches and eng.query(N.Q_FFT_COUNT) == ffts
    eng.set_terms(NAMES, p64)
    E2, v2 = eng.energy_potential(td)
    assert E2 == E and torch.equal(v2, v)
    assert eng.query(N.Q_LAUNCH_COUNT) == launches and eng.query(N.Q_FFT_COUNT) == ffts
    eng.close()


# ------------------------------------------------------------------------------- 4: past one trip of every loop
BIG = (128, 128, 66)
BIG_POINTS = BIG[0] * BIG[1] * BIG[2]                       # 1 081 344
BIG_KPOINTS = BIG[0] * BIG[1] * (BIG[2] // 2 + 1)           # 557 056
# the spectral kernels and the epilogue take a second, ragged trip; the maps (two points per thread) a second one as well; the
# reducing kernels four full trips and a ragged fifth
assert BIG_KPOINTS > SPEC_TRIP and BIG_KPOINTS % SPEC_TRIP != 0 and BIG_POINTS // 2 > SPEC_TRIP
assert BIG_POINTS % RED_TRIP != 0 and BIG_POINTS // RED_TRIP == 4
_BIG = {}


def big_inputs():
    if 'in' not in _BIG:
        _BIG['in'] = (np.diag([2.0, 2.0, 1.0]) @ synth.cubic_cell(64), synth.smooth_density(BIG, seed=41))
    return _BIG['in']


def big_double(key):
    """the numpy double on the big grid, once per kind"""
    if key not in _BIG:
        box, den = big_inputs()
        eta, w = hc_kernel.solve_kernel(hc_cases.beta_of(key), hc_cases.ETA_MAX, hc_cases.N_ETA)
        r = hc_double.hc_energy_potential(key, hc_cases.KINDS[key][1], box, den, eta, w)
        _BIG[key] = {k: r[k] for k in ('E_nl', 'v_nl', 'M')}
    return _BIG[key]


@pytest.mark.parametrize('key', KEYS)
def test_second_and_ragged_trips_match_numpy_double(key):
    """(128, 128, 66): 557 056 k-points (above the 524 288 threads of hc_spec_kernel, hc_adjoint_kernel, spec_grad_kernel and the
    epilogue: a second trip of 32 768) and 1 081 344 points (4.125 trips of the reducing kernels); the j * total + i node stride
    with i beyond one trip.  Measured on an MI355X (hc, revhc): dE_nl 1.4e-18, 9.2e-19 and dE 3.5e-16 of |E_total|, dv_nl 1.43e-13,
    1.40e-13 and dv 2.89e-13 of the maximum; M = 10, 12."""
    box, den = big_inputs()
    ref = big_double(key)
    E_rest, v_rest = hc_double.tf_vw(box, den)
    E_ref = E_rest + ref['E_nl']
    eng = Engine(BIG, DEV).set_cell(box)
    p = params(key)
    td = dev(den)
    eng.set_terms(NAMES, p)
    E_terms, v = eng.energy_potential(td)
    eng.set_terms(('nlk',), p)
    _E, v_nl = eng.energy_potential(td)
    figs = (abs(E_terms['nlk'] - ref['E_nl']) / abs(E_ref), abs(sum(E_terms.values()) - E_ref) / abs(E_ref),
            maxerr(v_nl.cpu().numpy(), ref['v_nl']), maxerr(v.cpu().numpy(), v_rest + ref['v_nl']))
    print('%s %s: dE_nl %.2e dE %.2e dv_nl %.2e dv %.2e M %d' % ((BIG, key) + figs + (ref['M'],)))
    assert figs[0] <= ETOL and figs[1] <= ETOL
    assert figs[2] <= VTOL and figs[3] <= VTOL
    assert ref['M'] > 8 and chain_transforms(eng, td, p) == 2 * ref['M'] + 10
    eng.close()


@pytest.mark.parametrize('key', KEYS)
def test_closure_matches_chain_rule_past_one_trip(key):
    """the form of tests/test_hc_gpu.py::test_closure_matches_chain_rule (1e-11), on the big grid: the closure's map, the epilogue's
    chi branch and the device-side share of mu beyond one trip.  Device against device.  Measured on an MI355X (both kinds): energies
    2.6e-15, mu 4.2e-16, chi.grad 3.1e-14."""
    box, den = big_inputs()
    rng = np.random.default_rng(1041)
    chi = np.sqrt(den) * (1.0 + 0.05 * rng.random(BIG))
    vext = synth.random_potential(BIG, seed=141)
    vol = abs(np.linalg.det(box))
    dV = vol / chi.size
    n_elec = float(np.floor(den.mean() * vol) + 0.3)
    p = params(key)
    eng = Engine(BIG, DEV).set_cell(box).set_terms(CLOSURE_NAMES, p)
    tc, tv = dev(chi), dev(vext)
    Ec, mu, g = eng.energy_grad_chi(tc, n_elec, tv)
    Ec2, mu2, g2 = eng.energy_grad_chi(tc, n_elec, tv)
    assert Ec2 == Ec and mu2 == mu and torch.equal(g2, g)
    cfac = n_elec / (np.mean(chi * chi) * vol)
    n = cfac * chi * chi
    E, v = eng.energy_potential(dev(n), tv)
    v = v.cpu().numpy()
    mu_ref = float((v * n).sum() * dV / n_elec)
    g_ref = cfac * 2.0 * chi * (v - mu_ref) * dV
    figs = (max(abs(Ec[k] - E[k]) / max(1.0, abs(E[k])) for k in E), abs(mu - mu_ref) / max(1.0, abs(mu_ref)),
            maxerr(g.cpu().numpy(), g_ref))
    print('%s %s closure: dE %.2e dmu %.2e dgrad %.2e' % ((BIG, key) + figs))
    assert figs[0] <= 1e-11 and figs[1] <= 1e-11 and figs[2] < 1e-11
    assert Ec['nlk'] != 0.0 and sorted(k for k in Ec if Ec[k] != 0.0) == sorted(CLOSURE_NAMES)
    eng.set_terms(('nlk',), p)
    E1, mu1, g1 = eng.energy_grad_chi(tc, n_elec)
    _E, v1 = eng.energy_potential(dev(n))
    v1 = v1.cpu().numpy()
    mu1_ref = float((v1 * n).sum() * dV / n_elec)
    assert E1['nlk'] == Ec['nlk']
    assert abs(mu1 - mu1_ref) <= 1e-11 * max(1.0, abs(mu1_ref))
    assert maxerr(g1.cpu().numpy(), cfac * 2.0 * chi * (v1 - mu1_ref) * dV) < 1e-11
    eng.close()


# ------------------------------------------------------------------------------- 5: where the extrema lie
LAST, THIRD_TRIP = BIG_POINTS - 1, 600000
assert 2 * RED_TRIP <= THIRD_TRIP < 3 * RED_TRIP and LAST >= 4 * RED_TRIP            # the third and the ragged fifth trip


@pytest.mark.parametrize('at_min,at_max', [(LAST, THIRD_TRIP), (THIRD_TRIP, LAST)])
def test_extrema_in_later_trips_reach_the_node_set(at_min, at_max):
    """HC with lambda = 0: xi = 2 k_F(n) depends on n(r) alone.  Half the density's minimum and twice its maximum are planted at
    the last grid point (the ragged fifth trip of hc_minmax_kernel) and at flat index 600 000 (its third trip), then swapped.  With
    kappa = 1.01 the node set needs more than 64 nodes, so the evaluation is refused after the head alone, and the message carries
    what the head found: xi_min and xi_max (%g: six significant digits) and M.  Measured on an MI355X, both placements: xi_min = 1.38294
    and xi_max = 2.64029 (2 k_F of the planted values: 1.3829409, 2.6402913), M = 104 as node_set gives."""
    box, den = big_inputs()
    den = den.copy()
    n_lo, n_hi = 0.5 * den.min(), 2.0 * den.max()
    den.reshape(-1)[at_min], den.reshape(-1)[at_max] = n_lo, n_hi
    kappa = 1.01
    M, margin = margins(two_kf(n_lo), two_kf(n_hi), kappa)
    assert margin > 1e-3 and M > 64
    eng = Engine(BIG, DEV).set_cell(box).set_terms(NAMES, params('hc', nlk_p0=0.0, nlk_p2=kappa))
    with pytest.raises(RuntimeError) as err:
        eng.energy_potential(dev(den))
    m = re.search(r'xi_min = (\S+), xi_max = (\S+) and kappa = (\S+) need M = (\d+) spline nodes', str(err.value))
    assert m, str(err.value)
    xi_min, xi_max, M_dev = float(m.group(1)), float(m.group(2)), int(m.group(4))
    print('planted %d / %d: xi_min %s (2 k_F %.8g) xi_max %s (2 k_F %.8g) M %d (%d)' % (at_min, at_max, m.group(1), two_kf(n_lo),
                                                                                     m.group(2), two_kf(n_hi), M_dev, M))
    # (%g rounds to six significant digits: at most 5e-6 of the value)
    assert abs(xi_min - two_kf(n_lo)) <= 5e-6 * two_kf(n_lo) and abs(xi_max - two_kf(n_hi)) <= 5e-6 * two_kf(n_hi)
    assert M_dev == M
    eng.close()


# ------------------------------------------------------------------------------- 6: densities that are not positive
@pytest.mark.parametrize('key', KEYS)
def test_density_that_is_not_positive_is_refused_and_leaves_no_trace(key):
    """One bad value (0, a negative one, NaN) at the last grid point and at flat index 300 000 (the second trip of hc_minmax_kernel),
    through ofdft_energy_potential; a NaN in chi through ofdft_energy_grad_chi (c chi^2 cannot be negative).  Every call is
    refused by the host with its message, the launch and transform counts stay, and the next evaluation of the good density
    returns the bits of the one before: the NaN left in the hc:* workspaces does no harm.  On an MI355X: eight refusals per kind, all
    by that message; E_nl = -2.702798009064e-01 (hc), -2.707538972504e-01 (revhc) before and after."""
    box, den = big_inputs()
    vol = abs(np.linalg.det(box))
    n_elec = float(den.mean() * vol)
    eng = Engine(BIG, DEV).set_cell(box).set_terms(NAMES, params(key))
    td, tc = dev(den), dev(np.sqrt(den))
    assert RED_TRIP <= 300000 < 2 * RED_TRIP
    E0, v0 = eng.energy_potential(td)
    counts = (eng.query(N.Q_LAUNCH_COUNT), eng.query(N.Q_FFT_COUNT))
    refused = 0
    for at in (LAST, 300000):
        for bad in (0.0, -0.01, float('nan')):
            tbad = td.clone()
            tbad.view(-1)[at] = bad
            with pytest.raises(RuntimeError, match=NOT_POSITIVE):
                eng.energy_potential(tbad)
            refused += 1
            assert (eng.query(N.Q_LAUNCH_COUNT), eng.query(N.Q_FFT_COUNT)) == counts, (at, bad)
            E1, v1 = eng.energy_potential(td)
            assert E1 == E0 and torch.equal(v1, v0), (at, bad)
            assert (eng.query(N.Q_LAUNCH_COUNT), eng.query(N.Q_FFT_COUNT)) == counts
    Ec0, mu0, g0 = eng.energy_grad_chi(tc, n_elec)
    counts = (eng.query(N.Q_LAUNCH_COUNT), eng.query(N.Q_FFT_COUNT))
    for at in (LAST, 300000):
        cbad = tc.clone()
        cbad.view(-1)[at] = float('nan')
        with pytest.raises(RuntimeError, match=NOT_POSITIVE):
            eng.energy_grad_chi(cbad, n_elec)
        refused += 1
        assert (eng.query(N.Q_LAUNCH_COUNT), eng.query(N.Q_FFT_COUNT)) == counts, at
        Ec1, mu1, g1 = eng.energy_grad_chi(tc, n_elec)
        assert Ec1 == Ec0 and mu1 == mu0 and torch.equal(g1, g0), at
    print('%s %s: %d refusals, E_nl %.12e unchanged' % (BIG, key, refused, E0['nlk']))
    assert refused == 8 and np.isfinite(E0['nlk']) and E0['nlk'] != 0.0
    eng.close()


# ------------------------------------------------------------------------------- 7: parameter edges
def _double(key, args, box, den):
    beta = args[1] if key == 'hc' else args[2]
    eta, w = hc_kernel.solve_kernel(beta, hc_cases.ETA_MAX, hc_cases.N_ETA)
    return hc_double.hc_energy_potential(key, args, box, den, eta, w)


def _against_double(eng, td, p, ref, E_rest, what):
    eng.set_terms(NAMES, p)
    E_terms, _v = eng.energy_potential(td)
    eng.set_terms(('nlk',), p)
    _E, v_nl = eng.energy_potential(td)
    E_ref = E_rest + ref['E_nl']
    figs = (abs(E_terms['nlk'] - ref['E_nl']) / abs(E_ref), maxerr(v_nl.cpu().numpy(), ref['v_nl']))
    print('%s: dE_nl %.2e dv_nl %.2e M %d' % ((what,) + figs + (ref['M'],)))
    assert figs[0] <= ETOL and figs[1] <= VTOL, what
    return E_terms['nlk'], v_nl


def test_lambda_zero_and_a_zero_are_one_functional_and_b_zero_matches_the_double():
    """HC with lambda = 0 and revHC with a = 0 at one beta and kappa: in hc_xi_point both branches give F = 1 exactly and zero
    derivatives, and the two parameter layouts of hc_par land in the same fields, so energy and potential are bit-equal; each
    against the numpy double, and revHC with b = 0 as well.  Measured on an MI355X: lambda = 0 against a = 0 bit-equal (differences 0);
    against the double dE_nl 9.8e-19 in all three, dv_nl 9.3e-15 (lambda = 0, a = 0) and 3.6e-15 (b = 0)."""
    box, den = hc_cases.make_inputs('g16r')
    td = dev(den)
    E_rest = hc_double.tf_vw(box, den)[0]
    beta, kappa = 0.7, 1.2
    eng = Engine(den.shape, DEV).set_cell(box)
    hc_args, rev_args = (0.0, beta, kappa), (0.0, 0.10, beta, kappa)
    E_hc, v_hc = _against_double(eng, td, dict(nlk_kind=4, nlk_p0=0.0, nlk_p1=beta, nlk_p2=kappa), _double('hc', hc_args, box, den),
                                 E_rest, 'hc lambda = 0')
    E_rev, v_rev = _against_double(eng, td, dict(nlk_kind=5, nlk_p0=0.0, nlk_p1=0.10, nlk_p2=beta, nlk_p3=kappa),
                                   _double('revhc', rev_args, box, den), E_rest, 'revhc a = 0')
    print('lambda = 0 against a = 0: dE %.2e dv %.2e' % (abs(E_hc - E_rev), float((v_hc - v_rev).abs().max())))
    assert E_hc == E_rev and torch.equal(v_hc, v_rev)
    b0 = hc_cases.REVHC_ARGS[:1] + (0.0,) + hc_cases.REVHC_ARGS[2:]
    _against_double(eng, td, params('revhc', nlk_p1=0.0), _double('revhc', b0, box, den), E_rest, 'revhc b = 0')
    eng.close()


@pytest.mark.parametrize('key', KEYS)
def test_uniform_density_is_served_and_its_nonlocal_term_vanishes(key):
    """n(r) = n0, the start point of every optimisation: xi_min = xi_max, the kernel vanishes at eta = 0, so T_NL and its
    potential are zero up to rounding (|E_nl| <= E_TOL |E_TF|, max|v_nl| <= V_TOL max|v_TF|), the node set is that of
    node_set(xi, xi, kappa) (ceil margins above 1e-3 asserted), and chi.grad of the uniform chi is zero within 1e-11 of
    2 chi v_TF dV.  Measured on an MI355X, both kinds: E_nl, v_nl and chi.grad exactly 0 (the spectrum of a uniform grid has its one
    entry at q = 0, where w = 0), mu / v_TF = 1.000000000000001; M = 9 (hc), 10 (revhc)."""
    box, _den = hc_cases.make_inputs('g16r')
    shape = (16, 16, 16)
    n0 = 0.03
    vol = abs(np.linalg.det(box))
    dV = vol / 4096
    kappa = hc_cases.kappa_of(key)
    M, margin = margins(two_kf(n0), two_kf(n0), kappa)
    assert margin > 1e-3 and 4 <= M <= 64
    td = torch.full(shape, n0, dtype=torch.double, device=DEV)
    p = params(key)
    eng = Engine(shape, DEV).set_cell(box).set_terms(NAMES, p)
    E, _v = eng.energy_potential(td)
    eng.set_terms(('nlk',), p)
    _E, v_nl = eng.energy_potential(td)
    v_tf = (5 / 3) * 0.3 * (3 * np.pi ** 2) ** (2 / 3) * n0 ** (2 / 3)
    figs = (abs(E['nlk']) / abs(E['tf']), float(v_nl.abs().max()) / v_tf)
    print('uniform %s: |E_nl| / |E_tf| %.2e max|v_nl| / v_tf %.2e M %d' % ((key,) + figs + (M,)))
    assert E['tf'] == pytest.approx(0.3 * (3 * np.pi ** 2) ** (2 / 3) * n0 ** (5 / 3) * vol, rel=1e-12)
    assert figs[0] <= ETOL and figs[1] <= VTOL
    assert chain_transforms(eng, td, p) == 2 * M + 10
    eng.set_terms(NAMES, p)
    chi = torch.full(shape, np.sqrt(n0), dtype=torch.double, device=DEV)
    Ec, mu, g = eng.energy_grad_chi(chi, n0 * vol)
    scale = 2.0 * np.sqrt(n0) * v_tf * dV
    print('uniform %s closure: max|chi.grad| / (2 chi v_tf dV) %.2e mu / v_tf %.15f' % (key, float(g.abs().max()) / scale, mu / v_tf))
    assert float(g.abs().max()) <= 1e-11 * scale
    assert abs(Ec['nlk']) <= ETOL * abs(Ec['tf']) and abs(mu - v_tf) <= 1e-11 * v_tf
    eng.close()


# ------------------------------------------------------------------------------- 8: state around the chain
def test_kind_switches_and_a_refusal_leave_the_other_pipelines_bitwise():
    """One context on g16r: a closure evaluation of the Wang-Teter set (repeated until the persistent small-grid kernel or the graph
    replay serves it) and an evaluation of OFDFT_NLK kind 1 (KGAP) are recorded; then kinds 4 and 5 are evaluated through both
    entry points, one call refused (a NaN in the density); then the two recorded evaluations return their bits again, the
    replay / resident counters advance again, and kind 4 returns the bits a fresh context gives.  A fresh context gives the
    recorded bits as well."""
    box, den, vext, chi, n_elec = cases.make_inputs('g16r')
    wt_names = ('ion_electron', 'hartree', 'tf', 'vw', 'wt_nl', 'lda_x')
    kgap = dict(nlk_kind=1, nlk_p0=2.0)
    td, tc, tv = dev(den), dev(chi), dev(vext)

    def served(eng):
        return eng.query(N.Q_GRAPH_REPLAYS) + eng.query(N.Q_RESIDENT_EVALS)

    def wt_pass(eng):
        """five closure calls of the Wang-Teter set (tests/test_nlk_gpu.py: the replay serves from the second call on)"""
        eng.set_terms(wt_names)
        s0 = served(eng)
        Ec, mu, g = eng.energy_grad_chi(tc, n_elec, tv)
        out = (dict(Ec), mu, g.clone())
        for _ in range(4):
            Ec, mu, g = eng.energy_grad_chi(tc, n_elec, tv)
            assert Ec == out[0] and mu == out[1] and torch.equal(g, out[2])
        assert served(eng) > s0
        return out

    def kgap_pass(eng):
        eng.set_terms(NAMES, kgap)
        E, v = eng.energy_potential(td)
        Ec, mu, g = eng.energy_grad_chi(tc, n_elec)
        return (dict(E), v.clone(), dict(Ec), mu, g.clone())

    def hc_pass(eng, key):
        eng.set_terms(NAMES, params(key))
        E, v = eng.energy_potential(td)
        Ec, mu, g = eng.energy_grad_chi(tc, n_elec)
        return (dict(E), v.clone(), dict(Ec), mu, g.clone())

    def same(a, b):
        return len(a) == len(b) and all(torch.equal(x, y) if torch.is_tensor(x) else x == y for x, y in zip(a, b))

    eng = Engine(den.shape, DEV).set_cell(box)
    wt0, kg0 = wt_pass(eng), kgap_pass(eng)
    assert kg0[0]['nlk'] != 0.0 and wt0[0]['wt_nl'] != 0.0
    hc0, rev0 = hc_pass(eng, 'hc'), hc_pass(eng, 'revhc')
    assert hc0[0]['nlk'] != rev0[0]['nlk'] and hc0[0]['nlk'] != kg0[0]['nlk']
    tbad = td.clone()
    tbad.view(-1)[-1] = float('nan')
    with pytest.raises(RuntimeError, match=NOT_POSITIVE):
        eng.energy_potential(tbad)
    wt1, kg1 = wt_pass(eng), kgap_pass(eng)
    assert same(wt1, wt0) and same(kg1, kg0)
    hc1 = hc_pass(eng, 'hc')
    assert same(hc1, hc0)
    fresh = Engine(den.shape, DEV).set_cell(box)
    assert same(hc_pass(fresh, 'hc'), hc0)
    fresh.close()
    fresh = Engine(den.shape, DEV).set_cell(box)
    assert same(wt_pass(fresh), wt0) and same(kgap_pass(fresh), kg0) and same(hc_pass(fresh, 'revhc'), rev0)
    fresh.close()
    eng.close()


# figures measured on an MI355X, against the bounds 1e-13 (energies) and 1.5e-12 (fields); the closure's against 1e-11
MEASURED = {
    # engine: (dE_nl, dE, dv_nl, dv); the drop-in classes give the same dE and dv to two digits
    'golden': {('g16r_t8', 'hc'): (2.75e-17, 3.35e-16, 8.29e-15, 2.56e-15), ('g16r_t8', 'revhc'): (6.50e-17, 3.35e-16, 1.01e-14, 2.43e-15),
               ('g18t_t8', 'hc'): (5.76e-17, 5.90e-16, 1.09e-14, 1.08e-14), ('g18t_t8', 'revhc'): (4.56e-17, 5.90e-16, 1.17e-14, 1.09e-14),
               ('g16w_m64', 'hc'): (3.22e-17, 4.12e-16, 2.88e-14, 1.00e-15),
               ('g20x33', 'hc'): (3.67e-18, 4.69e-16, 1.07e-14, 5.38e-14), ('g20x33', 'revhc'): (2.66e-17, 4.69e-16, 1.21e-14, 5.39e-14)},
    # the default table against the short-table golden, of max|v_nl|
    'table_moves_v_nl': {('g16r_t8', 'hc'): 6.78e-4, ('g16r_t8', 'revhc'): 6.94e-4, ('g18t_t8', 'hc'): 5.76e-4, ('g18t_t8', 'revhc'): 6.09e-4},
    'big': {'hc': (1.37e-18, 3.52e-16, 1.43e-13, 2.89e-13), 'revhc': (9.15e-19, 3.52e-16, 1.40e-13, 2.89e-13)},
    'big_closure': {'hc': dict(dE=2.60e-15, dmu=4.16e-16, dgrad=3.09e-14), 'revhc': dict(dE=2.60e-15, dmu=4.16e-16, dgrad=3.12e-14)},
    'extrema': dict(xi_min='1.38294', xi_max='2.64029', M=104),            # both placements; 2 k_F = 1.3829409, 2.6402913
    # (dE_nl, dv_nl); lambda = 0 against a = 0: both differences exactly 0
    'edges': {'hc lambda = 0': (9.80e-19, 9.33e-15), 'revhc a = 0': (9.80e-19, 9.33e-15), 'revhc b = 0': (9.80e-19, 3.55e-15)},
    # E_nl, v_nl and chi.grad are exactly 0 for both kinds (the spectrum of a uniform grid has its one entry at q = 0, where w = 0)
    'uniform': dict(E_nl=0.0, v_nl=0.0, chi_grad=0.0, mu_over_v_tf=1.000000000000001),
}
