"""GPU tests of the Huang-Carter kinds of OFDFT_NLK (kinds 4 and 5: HuangCarter, RevisedHuangCarter) against the reference's
forward + autograd (tests/golden/hc_<case>.npz; generator tests/golden/make_golden_hc.py) and the numpy double of the closed
form (tests/hc_double.py).

Bounds are the project's fp64 parity bounds (tests/spectral_check.py): energies E_TOL['f64'] of |E_total|, potentials
V_TOL['f64'] of the field's maximum.  Two independent fp64 evaluations on the CPU (the reference's autograd and the numpy
double) sit at 8e-17 and 3.6e-14 (tests/test_hc_cpu.py).  Measured on an MI355X over the eight (case, kind) pairs and the
128 x 64 x 64 grid: dE_nl <= 7.7e-17 and dE <= 5.9e-16 of |E_total|, dv_nl <= 3.6e-14 (g16w), dv <= 8.3e-14 (128 x 64 x 64).

The closure test follows tests/test_nlk_gpu.py::test_closure_matches_chain_rule_and_graph_replay_is_bitwise: chain rule at 1e-11,
repeated calls bitwise.  The per-term energies of the two entry points are compared at that bound as well: the closure forms
n = c chi^2 on the device and the chain rule forms it in numpy, so the two evaluations do not see the same bits of the density.
"""
import ctypes as C
import os

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
from professad_amd.optimize import optimize_density

pytestmark = pytest.mark.gpu
GOLDEN = os.path.dirname(os.path.abspath(cases.__file__))
DEV = 'cuda:0'
ETOL, VTOL = E_TOL['f64'], V_TOL['f64']
KEYS = list(hc_cases.KINDS)


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
    eng.set_terms(('tf', 'vw', 'nlk'), p)
    eng.energy_potential(td)
    full = eng.query(N.Q_FFT_COUNT)
    eng.set_terms(('tf', 'vw'))
    eng.energy_potential(td)
    return int(full - eng.query(N.Q_FFT_COUNT))


# ------------------------------------------------------------------------------- 1: golden parity
@pytest.mark.parametrize('case', hc_cases.CASES)
@pytest.mark.parametrize('key', KEYS)
def test_engine_and_drop_in_match_reference_golden(case, key):
    gold = np.load(os.path.join(GOLDEN, 'hc_%s.npz' % case))
    box, den = hc_cases.make_inputs(case)
    assert abs(cases.checksum(box, den) - float(gold['checksum'])) < 1e-9
    tb, td = dev(box), dev(den)
    E_ref, v_ref = float(gold[key + '_E']), gold[key + '_v']
    E_nl_ref, v_nl_ref = float(gold[key + '_E_nl']), gold[key + '_v_nl']
    p = params(key)
    eng = Engine(den.shape, DEV).set_cell(box)
    eng.set_terms(('tf', 'vw', 'nlk'), p)
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
    # the node set is the reference's: the chain's transform count is 2 M + 10
    assert chain_transforms(eng, td, p) == 2 * int(gold[key + '_M']) + 10
    eng.close()
    # the drop-in class
    f = getattr(F, hc_cases.KINDS[key][0])(hc_cases.KINDS[key][1])
    Ef = float(f(tb, td))
    vf = F.get_functional_derivative(tb, td, f).cpu().numpy()
    Ef2 = float(f.forward(tb, td))
    print('%s %s drop-in: dE %.2e dv %.2e' % (case, key, abs(Ef - E_ref) / abs(E_ref), maxerr(vf, v_ref)))
    assert abs(Ef - E_ref) <= ETOL * abs(E_ref) and Ef2 == Ef
    assert maxerr(vf, v_ref) <= VTOL


# ------------------------------------------------------------------------------- 2: past one trip of the grid-stride loops
BIG = (128, 64, 64)


@pytest.mark.parametrize('key', KEYS)
def test_big_grid_matches_numpy_double(key):
    """524 288 points: twice the 1024 x 256 threads of the reducing kernels' grid cap, and three batches of inverse transforms"""
    box = np.diag([2.0, 1.0, 1.0]) @ synth.cubic_cell(64)
    den = synth.smooth_density(BIG, seed=41)
    eta, w = hc_kernel.solve_kernel(hc_cases.beta_of(key), hc_cases.ETA_MAX, hc_cases.N_ETA)
    ref = hc_double.hc_energy_potential(key, hc_cases.KINDS[key][1], box, den, eta, w)
    E_rest, v_rest = hc_double.tf_vw(box, den)
    E_ref = E_rest + ref['E_nl']
    eng = Engine(BIG, DEV).set_cell(box)
    p = params(key)
    td = dev(den)
    eng.set_terms(('tf', 'vw', 'nlk'), p)
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


# ------------------------------------------------------------------------------- 3: closure form
@pytest.mark.parametrize('case,key', [('g16r', 'hc'), ('g17r', 'revhc'), ('g18t', 'hc')])
def test_closure_matches_chain_rule(case, key):
    """ofdft_energy_grad_chi against the chain rule on ofdft_energy_potential's outputs, in the form of
    tests/test_nlk_gpu.py::test_closure_matches_chain_rule_and_graph_replay_is_bitwise (same bounds); a repeated call returns the
    same bits, and neither the persistent small-grid kernel nor the graph replay serves a term set with these kinds"""
    box, _den, vext, chi, n_elec = cases.make_inputs(case)
    shape = chi.shape
    vol = abs(np.linalg.det(box))
    dV = vol / chi.size
    names = ('ion_electron', 'hartree', 'tf', 'vw', 'nlk', 'lda_x')
    p = params(key)
    eng = Engine(shape, DEV).set_cell(box).set_terms(names, p)
    tc, tv = dev(chi), dev(vext)
    r0, g0 = eng.query(N.Q_RESIDENT_EVALS), eng.query(N.Q_GRAPH_REPLAYS)
    Ec, mu, g = eng.energy_grad_chi(tc, n_elec, tv)
    first = (dict(Ec), mu, g.clone())
    for _ in range(3):
        Ec2, mu2, g2 = eng.energy_grad_chi(tc, n_elec, tv)
        assert Ec2 == first[0] and mu2 == first[1] and torch.equal(g2, first[2])
    assert eng.query(N.Q_RESIDENT_EVALS) == r0 and eng.query(N.Q_GRAPH_REPLAYS) == g0
    cfac = n_elec / (np.mean(chi * chi) * vol)
    n = cfac * chi * chi
    E, v = eng.energy_potential(dev(n), tv)
    v = v.cpu().numpy()
    mu_ref = float((v * n).sum() * dV / n_elec)
    g_ref = cfac * 2.0 * chi * (v - mu_ref) * dV
    for k in E:
        assert abs(Ec[k] - E[k]) <= 1e-11 * max(1.0, abs(E[k])), (k, Ec[k], E[k])
    assert Ec['nlk'] != 0.0 and sorted(k for k in Ec if Ec[k] != 0.0) == sorted(names)
    assert abs(mu - mu_ref) <= 1e-11 * max(1.0, abs(mu_ref))
    assert maxerr(g.cpu().numpy(), g_ref) < 1e-11
    # the term alone: its share of mu and chi.grad
    eng.set_terms(('nlk',), p)
    E1, mu1, g1 = eng.energy_grad_chi(tc, n_elec)
    _E, v1 = eng.energy_potential(dev(n))
    v1 = v1.cpu().numpy()
    mu1_ref = float((v1 * n).sum() * dV / n_elec)
    assert E1['nlk'] == Ec['nlk']
    assert abs(mu1 - mu1_ref) <= 1e-11 * max(1.0, abs(mu1_ref))
    assert maxerr(g1.cpu().numpy(), cfac * 2.0 * chi * (v1 - mu1_ref) * dV) < 1e-11
    eng.close()


# ------------------------------------------------------------------------------- 4: density optimisation
def test_optimize_density_with_revhc_converges_below_the_uniform_density():
    box, _den, vext, _chi, n_elec = cases.make_inputs('g16r')
    vol = abs(np.linalg.det(box))
    names = ('ion_electron', 'hartree', 'tf', 'vw', 'nlk', 'lda_x')
    eng = Engine((16, 16, 16), DEV).set_cell(box).set_terms(names, params('revhc'))
    tv = dev(0.1 * vext)
    chi_u = torch.full((16, 16, 16), np.sqrt(n_elec / vol), dtype=torch.double, device=DEV)
    E_u, _mu, _g = eng.energy_grad_chi(chi_u, n_elec, tv)
    res = optimize_density(eng, n_elec, vext=tv, volume=vol, n_maxiter=400)
    print('revHC optimisation: %d iterations, E %.10f (uniform %.10f)' % (res['iterations'], res['E_Ha'], sum(E_u.values())))
    assert res['converged']
    assert res['E_Ha'] < sum(E_u.values())
    assert res['E_terms']['nlk'] != 0.0 and float(res['den'].min()) > 0.0
    eng.close()


# ------------------------------------------------------------------------------- 5: reproducibility and what invalidates
def test_two_calls_are_bitwise_and_changes_invalidate():
    box, den = hc_cases.make_inputs('g16r')
    td = dev(den)
    p = params('revhc')
    eng = Engine(den.shape, DEV).set_cell(box).set_terms(('tf', 'vw', 'nlk'), p)

    def run():
        E, v = eng.energy_potential(td)
        return E['nlk'], v.clone()
    E_a, v_a = run()
    E_a2, v_a2 = run()
    assert E_a2 == E_a and torch.equal(v_a2, v_a)
    changes = {
        'kappa': lambda: eng.set_terms(('tf', 'vw', 'nlk'), params('revhc', nlk_p3=1.25)),
        'beta': lambda: eng.set_terms(('tf', 'vw', 'nlk'), params('revhc', nlk_p2=0.7)),
        'cell': lambda: eng.set_cell(box * 1.05),
        'table': lambda: eng.set_nlk_table(*hc_kernel.solve_kernel(hc_cases.beta_of('revhc'), 40.0, 4001)),
    }
    for what, change in changes.items():
        change()
        E_b, v_b = run()
        assert E_b != E_a and not torch.equal(v_b, v_a), what
        eng.set_cell(box).set_terms(('tf', 'vw', 'nlk'), p)
        if what == 'table':
            eng.set_nlk_table(*hc_kernel.solve_kernel(hc_cases.beta_of('revhc'), hc_cases.ETA_MAX, hc_cases.N_ETA))
        E_c, v_c = run()
        assert E_c == E_a and torch.equal(v_c, v_a), what
    fresh = Engine(den.shape, DEV).set_cell(box).set_terms(('tf', 'vw', 'nlk'), p)
    E_f, v_f = fresh.energy_potential(td)
    assert E_f['nlk'] == E_a and torch.equal(v_f, v_a)
    fresh.close()
    eng.close()


# ------------------------------------------------------------------------------- 6: refusals
def test_refusals_by_message():
    box, den = hc_cases.make_inputs('g16r')
    td = dev(den)
    f32 = Engine(den.shape, DEV, dtype=torch.float32).set_cell(box)
    with pytest.raises(RuntimeError, match=r'libofdft_hip\.so'):
        f32.set_terms(('tf', 'vw', 'nlk'), params('hc'))
    f32.close()
    eng = Engine(den.shape, DEV).set_cell(box)
    with pytest.raises(RuntimeError, match='OFDFT_P_NLK_KIND.*4 \\(HC\\) or 5 \\(revHC\\)'):
        eng.set_terms(('tf', 'vw', 'nlk'))
    with pytest.raises(RuntimeError, match='kappa must exceed 1'):
        eng.set_terms(('tf', 'vw', 'nlk'), params('hc', nlk_p2=1.0))
    with pytest.raises(RuntimeError, match='kappa must exceed 1'):
        eng.set_terms(('tf', 'vw', 'nlk'), params('revhc', nlk_p3=0.9))
    for bad in (0.0, 5 / 3, -0.2):
        with pytest.raises(RuntimeError, match=r'beta must lie in \(0, 5/3\)'):
            eng.set_terms(('tf', 'vw', 'nlk'), params('hc', nlk_p1=bad))
        with pytest.raises(RuntimeError, match=r'beta must lie in \(0, 5/3\)'):
            eng.set_terms(('tf', 'vw', 'nlk'), params('revhc', nlk_p2=bad))
    with pytest.raises(RuntimeError, match='lambda must be >= 0'):
        eng.set_terms(('tf', 'vw', 'nlk'), params('hc', nlk_p0=-1e-3))
    with pytest.raises(RuntimeError, match='b must be >= 0'):
        eng.set_terms(('tf', 'vw', 'nlk'), params('revhc', nlk_p1=-0.1))
    with pytest.raises(RuntimeError, match='OFDFT_P_WTS_KIND'):
        eng.set_terms(('tf', 'vw', 'nlk'), params('hc', wts_kind=1))
    eng.set_terms(('tf', 'vw', 'nlk'), params('hc'))
    with pytest.raises(RuntimeError, match='no stress'):
        eng.stress(td)
    with pytest.raises(RuntimeError, match='no second derivative of the term nlk'):
        eng.hessian_vector(td, td)
    E, _v = eng.energy_potential(td)            # the context still serves evaluations
    assert E['nlk'] != 0.0
    eng.close()
    slab = Engine(den.shape, DEV, nranks=2, rank=0).set_cell(box)
    with pytest.raises(RuntimeError, match='single-GPU contexts'):
        slab.set_terms(('tf', 'vw', 'nlk'), params('hc'))
    slab.close()


def test_missing_table_through_the_raw_abi():
    box, den = hc_cases.make_inputs('g16r')
    td = dev(den)
    eng = Engine(den.shape, DEV).set_cell(box)
    vals = np.zeros(N.NPARAMS)
    vals[:13] = [5 / 6, 5 / 6, 0.9, 0.4, 2.7, 1.0, 0.0, 40 / 27, 0.0, 0.0, 0.0, 1.0, 0.0]
    vals[N.P_NLK_KIND:N.P_NLK_P2 + 1] = (4.0,) + hc_cases.HC_ARGS
    mask = N.TERM_BITS['tf'] | N.TERM_BITS['vw'] | N.TERM_BITS['nlk']
    dp = C.POINTER(C.c_double)
    assert eng.lib.ofdft_set_terms(eng._ctx, mask, vals.ctypes.data_as(dp), len(vals)) == 0
    E = (C.c_double * N.NTERMS)()
    out = torch.empty_like(td)
    rc = eng.lib.ofdft_energy_potential(eng._ctx, C.c_void_p(td.data_ptr()), None, E, C.c_void_p(out.data_ptr()), eng._stream())
    assert rc == N.ESTATE and b'ofdft_set_nlk_table' in eng.lib.ofdft_last_error(eng._ctx)
    # a table that is not uniform, or too short, is refused; a good one makes the context serve
    eta, w = hc_kernel.solve_kernel(hc_cases.HC_ARGS[1])
    bad = np.array(eta)
    bad[5] *= 1.01
    assert eng.lib.ofdft_set_nlk_table(eng._ctx, bad.ctypes.data_as(dp), w.ctypes.data_as(dp), len(w)) == N.EINVAL
    assert eng.lib.ofdft_set_nlk_table(eng._ctx, eta.ctypes.data_as(dp), w.ctypes.data_as(dp), 3) == N.EINVAL
    eng.set_nlk_table(eta, w)
    rc = eng.lib.ofdft_energy_potential(eng._ctx, C.c_void_p(td.data_ptr()), None, E, C.c_void_p(out.data_ptr()), eng._stream())
    assert rc == 0 and E[14] != 0.0
    eng.close()


def test_more_nodes_than_the_cap_is_refused_and_counters_stay():
    """a density whose xi_max / xi_min exceeds kappa^64 at kappa = 1.01 (checked on the CPU first): OFDFT_EINVAL naming xi_min,
    xi_max, kappa and M; the launch and transform counts of the last served evaluation stay as they were"""
    box, den = hc_cases.make_inputs('g16w')
    kappa = 1.01
    args = hc_cases.REVHC_ARGS[:3] + (kappa,)
    kx, ky, kz, _k2 = hc_double.wavevecs(box, den.shape)
    nk = np.fft.rfftn(den)
    gg = sum(np.fft.irfftn(1j * k * nk, den.shape, axes=(0, 1, 2)) ** 2 for k in (kx, ky, kz))
    xi = hc_double.xi_field('revhc', args, den, gg)[0]
    assert xi.max() / xi.min() > kappa ** 64
    _lower, M, _a, _b = hc_cases.node_set(float(xi.min()), float(xi.max()), kappa)
    assert M > 64
    td = dev(den)
    eng = Engine(den.shape, DEV).set_cell(box).set_terms(('tf', 'vw', 'nlk'), params('revhc'))
    E, v = eng.energy_potential(td)
    launches, ffts = eng.query(N.Q_LAUNCH_COUNT), eng.query(N.Q_FFT_COUNT)
    eng.set_terms(('tf', 'vw', 'nlk'), params('revhc', nlk_p3=kappa))
    with pytest.raises(RuntimeError, match=r'xi_min = .*xi_max = .*kappa = 1\.01.*M = %d' % M):
        eng.energy_potential(td)
    assert eng.query(N.Q_LAUNCH_COUNT) == launches and eng.query(N.Q_FFT_COUNT) == ffts
    chi = dev(np.sqrt(den))
    with pytest.raises(RuntimeError, match='M = %d' % M):
        eng.energy_grad_chi(chi, float(den.mean() * abs(np.linalg.det(box))))
    assert eng.query(N.Q_LAUNCH_COUNT) == launches
    eng.set_terms(('tf', 'vw', 'nlk'), params('revhc'))
    E2, v2 = eng.energy_potential(td)
    assert E2 == E and torch.equal(v2, v)
    eng.close()


@pytest.mark.parametrize('key', KEYS)
def test_staged_entries_refuse_the_kinds_on_one_gpu(key):
    """ofdft_dist_begin (HipStages, whose default is one rank) carries the Wang-Teter stages, which serve kinds 1 .. 3: kinds 4 / 5
    are refused by name before anything is reset or launched, and the context still serves the single-GPU entries"""
    from professad_amd.distributed import HipStages
    box, den = hc_cases.make_inputs('g16r')
    td = dev(den)
    st = HipStages(den.shape, DEV)
    st.set_cell(box).set_terms(('tf', 'vw', 'nlk'), params(key))
    E, v = st.energy_potential(td)
    launches, ffts = st.query(N.Q_LAUNCH_COUNT), st.query(N.Q_FFT_COUNT)
    assert launches > 0
    out = torch.empty_like(td)
    for from_chi, src, cscale in ((False, td, 0.0), (True, dev(np.sqrt(den)), 1.0)):
        with pytest.raises(RuntimeError, match=r'OFDFT_NLK of kind %d .*ofdft_dist_' % hc_cases.KINDS[key][2]['nlk_kind']):
            st.begin(src, from_chi, cscale, float(den.mean() * abs(np.linalg.det(box))), None, out)
        assert st.query(N.Q_LAUNCH_COUNT) == launches and st.query(N.Q_FFT_COUNT) == ffts
    E2, v2 = st.energy_potential(td)
    assert E2 == E and torch.equal(v2, v)
    st.close()


def test_a_table_of_the_callers_own_stays_through_set_terms():
    """Engine.set_nlk_table after set_terms: later set_terms calls with the same beta (the drop-in classes make one per evaluation)
    keep the caller's table; another beta brings solve_kernel's table for it, and so does going back"""
    box, den = hc_cases.make_inputs('g16r')
    td = dev(den)
    p = params('revhc')
    names = ('tf', 'vw', 'nlk')
    eng = Engine(den.shape, DEV).set_cell(box).set_terms(names, p)
    E_default = eng.energy_potential(td)[0]['nlk']
    eng.set_nlk_table(*hc_kernel.solve_kernel(hc_cases.beta_of('revhc'), 40.0, 4001))
    E_own = eng.energy_potential(td)[0]['nlk']
    assert E_own != E_default
    eng.set_terms(names, p)
    assert eng.energy_potential(td)[0]['nlk'] == E_own
    eng.set_terms(names, params('revhc', nlk_p3=1.25)).set_terms(names, p)           # (kappa is no argument of the table)
    assert eng.energy_potential(td)[0]['nlk'] == E_own
    eng.set_terms(names, params('revhc', nlk_p2=0.7)).set_terms(names, p)
    assert eng.energy_potential(td)[0]['nlk'] == E_default
    eng.close()
