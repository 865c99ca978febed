"""GPU tests of the Hessian-vector product (ofdft_hessian_vector, Engine.hessian_vector, the twice-differentiable drop-in terms
and get_inv_G) against the reference's double autograd (tests/golden/hvp_<case>.npz; generator tests/golden/make_golden_hvp.py),
the numpy double (tests/hvp_double.py) on grids without goldens, and the Lindhard function in closed form.

Tolerance rule: per key, 10 x the largest max|hv - golden| / max|golden| measured on an MI355X over the four golden cases
(MEASURED below; the docstring of the first test lists them); q_t takes the same bound relative to |q_t|.  The grids without
goldens, the symmetry check, the double backward and get_inv_G use the bound of the key they exercise.
"""
import os

import numpy as np
import pytest
import torch

import cases
import hvp_cases
import hvp_double as D
from professad_amd import _native as N
from professad_amd import functionals as F
from professad_amd import synth
from professad_amd.engine import Engine

pytestmark = pytest.mark.gpu
GOLDEN = os.path.dirname(os.path.abspath(cases.__file__))
DEV = 'cuda:0'
KEYS = {**hvp_cases.TERMS, **hvp_cases.SETS}
# largest measured deviation per key, MI355X (see test_terms_and_sets_match_the_reference_goldens)
MEASURED = {
    'hartree': 1.14e-15, 'tf': 5.26e-16, 'vw': 1.10e-15, 'wt_nl': 4.93e-12, 'lda_x': 5.87e-16, 'pz_c': 8.34e-16, 'pw_c': 2.36e-15,
    'chachiyo_c': 1.02e-15, 'wgc98_nl': 4.93e-12, 'cfg1': 1.22e-15, 'cfg2': 5.45e-14,
}
MEASURED_GINV = 1.21e-13   # get_inv_G against the closed forms, relative to G_inv (test_get_inv_G_closed_forms)
SIX = ('hartree', 'tf', 'vw', 'wt_nl', 'lda_x', 'pz_c')


def bound(key):
    return 10 * MEASURED[key]


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.double, device=DEV)


def params_of(al, be):
    return None if al is None else dict(wt_alpha=al, wt_beta=be)


_GOLD = {}


def gold(case):
    """golden file and inputs of a case, loaded once and shared"""
    if case not in _GOLD:
        g = np.load(os.path.join(GOLDEN, 'hvp_%s.npz' % case))
        box, den, _vext = hvp_cases.make_inputs(case)
        w = hvp_cases.direction(den.shape)
        assert abs(cases.checksum(box, den, w) - float(g['checksum'])) < 1e-9
        _GOLD[case] = (g, box, den, w)
    return _GOLD[case]


def engine(shape, box, names, al=None, be=None):
    return Engine(shape, DEV).set_cell(box).set_terms(list(names), params_of(al, be))


# ------------------------------------------------------------------------------- 1: per term and per term set, goldens
@pytest.mark.parametrize('case', hvp_cases.CASES)
def test_terms_and_sets_match_the_reference_goldens(case):
    """hv and q_t through Engine.hessian_vector for the nine served terms, the alpha != beta member and the cfg1 / cfg2 sums.

    Measured max|hv - golden| / max|golden| on an MI355X, g16r / g17r / g18t / g16d (the test prints every figure before it asserts):
        hartree 4.0e-16 / 8.4e-16 / 1.1e-15 / 4.0e-16      tf 5.3e-16 / 4.1e-16 / 5.2e-16 / 4.3e-16      vw 6.0e-16 / 1.1e-15 / 9.7e-16 / 5.0e-16
        lda_x 3.0e-16 / 5.5e-16 / 3.0e-16 / 5.9e-16        pz_c 8.3e-16 / 8.2e-16 / 8.1e-16 / 8.0e-16    pw_c 2.4e-15 / 1.4e-15 / 1.2e-15 / 1.0e-15
        chachiyo_c 6.5e-16 / 1.0e-15 / 8.2e-16 / 7.0e-16   cfg1 6.0e-16 / 1.2e-15 / 1.0e-15 / 4.9e-16    cfg2 3.5e-14 / 5.5e-14 / 4.1e-14 / 3.4e-15
        wt_nl and wgc98_nl 3.6e-12 / 4.9e-12 / 3.7e-12 / 7.3e-14          q_t: at most 4.2e-13 (wt_nl), 5.6e-15 (cfg2), 5.3e-16 elsewhere
    The nonlocal term alone stands out, below the 1e-11 that would be a finding: its kernel 1 / G^-1(eta) - 3 eta^2 - 1 cancels twice
    at large eta, so one rounding in eta, the logarithm or the reciprocal comes out ~4.5 eta^4 times larger (eta reaches 11 .. 12
    on the r_s = 2 grids, 5.3 on g16d; a random direction has full power there).  The numpy double against the same goldens is at
    4.2e-13 (tests/test_hvp_cpu.py) with library log and division; the device kernel is the evaluation's own (lindhard_shape,
    lean log and reciprocal), a few roundings more.  Inside cfg2 the term is a hundredth of vW's share, hence 5e-14 there."""
    g, box, den, w = gold(case)
    dV = abs(np.linalg.det(box)) / den.size
    td, tw = dev(den), dev(w)
    eng = Engine(den.shape, DEV).set_cell(box)
    for key, (names, al, be) in KEYS.items():
        q, hv = eng.set_terms(list(names), params_of(al, be)).hessian_vector(td, tw, want_terms=True)
        hv = hv.cpu().numpy()
        ref, qref = g['hv_' + key], float(g['q_' + key])
        if key == 'ion_electron':        # accepted without vext; contributes nothing
            assert not hv.any() and q['ion_electron'] == 0.0 and not ref.any()
            continue
        d = float(np.abs(hv - ref).max() / np.abs(ref).max())
        dq = abs(sum(q.values()) - qref) / abs(qref)
        dsum = abs(sum(q.values()) - float((w * hv).sum() * dV)) / abs(qref)      # the kernel's sums against the returned field
        print('MEASURE hvp %s %s: hv %.2e q %.2e (q vs field %.2e)' % (case, key, d, dq, dsum))
        assert d <= bound(key), (case, key, d)
        assert dq <= bound(key) and dsum <= bound(key), (case, key, dq, dsum)
        assert all(v == 0.0 for k, v in q.items() if k not in names)
    eng.close()


# ------------------------------------------------------------------------------- 2: transform families without goldens
# measured on an MI355X against tests/hvp_double.py, per shape: max|hv - double| / max|double| and |q_t - double| / |double| per term
MEASURED_DOUBLE = {
    (48, 96, 32): dict(hv=2.36e-15, hartree=5.85e-16, tf=1.37e-16, vw=3.24e-16, wt_nl=1.68e-16, lda_x=2.14e-16, pz_c=3.96e-16),
    (32, 16, 64): dict(hv=1.27e-13, hartree=6.90e-16, tf=1.22e-16, vw=0.0, wt_nl=9.69e-13, lda_x=1.91e-16, pz_c=5.29e-16),
}
EPS = 2.0 ** -52      # a q_t measured below one rounding of a double (vw on (32, 16, 64): equal bits) takes this as its figure


@pytest.mark.parametrize('shape,triclinic', [((48, 96, 32), True), ((32, 16, 64), False)])
def test_mixed_radix_and_unequal_powers_of_two_match_the_double(shape, triclinic):
    """cfg2's terms with the Wang-Teter exponents of WGC98 (alpha != beta: four nonlocal spectra) against tests/hvp_double.py, the
    same rule as for the goldens: 10 x the figure measured for this shape (MEASURED_DOUBLE), for hv and for every q_t.  The
    nonlocal q_t and hv of (32, 16, 64) carry the kernel's conditioning (see the first test): eta reaches 15.1 there, 4.0 on (48, 96, 32)."""
    box = synth.triclinic_cell(shape[0] / 8.0) if triclinic else synth.cubic_cell(32)
    den = synth.random_density(shape, seed=11)
    w = hvp_cases.direction(shape, seed=78)
    names = hvp_cases.SETS['cfg2'][0]
    al, be = D.WGC98
    qd, hvd = D.hessian_vector(box, den, w, names, al, be)
    eng = engine(shape, box, names, al, be)
    assert eng.fast_path
    q, hv = eng.hessian_vector(dev(den), dev(w), want_terms=True)
    assert eng.query(N.Q_FFT_COUNT) == 14
    eng.close()
    m = MEASURED_DOUBLE[shape]
    d = float(np.abs(hv.cpu().numpy() - hvd).max() / np.abs(hvd).max())
    dq = {t: abs(q[t] - qd[t]) / abs(qd[t]) for t in names if t != 'ion_electron'}
    print('MEASURE hvp double %s: hv %.2e  q %s' % (shape, d, ' '.join('%s %.2e' % kv for kv in dq.items())))
    assert d <= 10 * m['hv']
    for t, v in dq.items():
        assert v <= 10 * max(m[t], EPS), (t, v)
    assert q['ion_electron'] == 0.0


# ------------------------------------------------------------------------------- 3: symmetry
def test_hessian_is_symmetric():
    """<u, H w> = <w, H u> for two independent directions on g18t with the cfg2 set, to the tolerance of cfg2 times |u| |H w|
    (measured on an MI355X: 1.0e-17 of it)"""
    _g, box, den, w = gold('g18t')
    u = hvp_cases.direction(den.shape, seed=79)
    names, al, be = hvp_cases.SETS['cfg2']
    eng = engine(den.shape, box, names, al, be)
    td = dev(den)
    Hw = eng.hessian_vector(td, dev(w)).cpu().numpy()
    Hu = eng.hessian_vector(td, dev(u), reuse_density=True).cpu().numpy()
    eng.close()
    a, b = float((u * Hw).sum()), float((w * Hu).sum())
    scale = np.linalg.norm(u) * np.linalg.norm(Hw)
    print('MEASURE hvp symmetry: %.2e' % (abs(a - b) / scale))
    assert abs(a - b) <= bound('cfg2') * scale


# ------------------------------------------------------------------------------- 4: reuse
@pytest.mark.parametrize('case,al,be,counts', [('g16r', 5 / 6, 5 / 6, (10, 6)), ('g17r', 5 / 6, 5 / 6, (10, 6)),
                                               ('g18t', D.WGC98[0], D.WGC98[1], (14, 8))])
def test_reuse_density_is_bitwise_and_skips_the_density_transforms(case, al, be, counts):
    _g, box, den, w = gold(case)
    eng = engine(den.shape, box, SIX, al, be)
    td, tw = dev(den), dev(w)
    with pytest.raises(RuntimeError, match=r'\(-3\)'):          # nothing retained yet: OFDFT_ESTATE
        eng.hessian_vector(td, tw, reuse_density=True)
    q0, hv0 = eng.hessian_vector(td, tw, want_terms=True)
    assert eng.query(N.Q_FFT_COUNT) == counts[0] and eng.query(N.Q_LAUNCH_COUNT) > 0 and eng.query(N.Q_KERNEL_MS) > 0
    q1, hv1 = eng.hessian_vector(td, tw, reuse_density=True, want_terms=True)
    assert eng.query(N.Q_FFT_COUNT) == counts[1]
    assert torch.equal(hv0, hv1) and q0 == q1
    hv2 = eng.hessian_vector(td, tw, reuse_density=True)                      # without the host read of the sums
    assert torch.equal(hv0, hv2)
    # set_terms invalidates
    eng.set_terms(['tf'])
    eng.set_terms(list(SIX), params_of(al, be))
    with pytest.raises(RuntimeError, match=r'\(-3\)'):
        eng.hessian_vector(td, tw, reuse_density=True)
    assert torch.equal(eng.hessian_vector(td, tw), hv0)
    # an energy call invalidates
    eng.energy_potential(td)
    with pytest.raises(RuntimeError, match=r'\(-3\)'):
        eng.hessian_vector(td, tw, reuse_density=True)
    # set_cell invalidates
    assert torch.equal(eng.hessian_vector(td, tw), hv0)
    eng.set_cell(box * 1.01)
    with pytest.raises(RuntimeError, match=r'\(-3\)'):
        eng.hessian_vector(td, tw, reuse_density=True)
    eng.close()


# ------------------------------------------------------------------------------- 5: refusals
@pytest.mark.parametrize('names,params,word', [
    (('tf', 'vw', 'wgc99_nl'), None, 'wgc99_nl'), (('pbe_x', 'pbe_c'), None, 'pbe_x'), (('pbe_c',), None, 'pbe_c'),
    (('vw', 'gga_k'), None, 'gga_k'), (('vw', 'vwgtf'), None, 'vwgtf'), (('tf', 'vw', 'nlk'), dict(nlk_kind=1, nlk_p0=2.0), 'nlk'),
    (('tf', 'vw', 'wt_nl'), dict(wts_kind=1.0), 'wts_kind')])
def test_unserved_term_sets_are_refused_by_name(names, params, word):
    _g, box, den, w = gold('g16r')
    eng = Engine(den.shape, DEV).set_cell(box).set_terms(list(names), params)
    with pytest.raises(RuntimeError, match=r'\(-1\).*\b%s\b' % word):
        eng.hessian_vector(dev(den), dev(w))
    eng.close()
    f = F.NativeTerms(list(names), **(params or {}))
    n = dev(den).requires_grad_()
    v = torch.autograd.grad(f(dev(box), n), n, create_graph=True)[0]
    with pytest.raises(NotImplementedError, match=word):
        torch.autograd.grad((v * dev(w)).sum(), n)


def test_slab_and_fp32_engines_refuse():
    from professad_amd.distributed import DistEngine
    _g, box, den, w = gold('g16r')
    de = DistEngine(den.shape, DEV).set_cell(torch.as_tensor(box)).set_terms(['tf'])
    with pytest.raises(NotImplementedError, match='single-GPU'):
        de.hessian_vector(dev(den), dev(w))
    de.close()
    e32 = Engine(den.shape, DEV, dtype=torch.float32).set_cell(box).set_terms(['tf'])
    with pytest.raises(NotImplementedError, match='fp64'):
        e32.hessian_vector(dev(den).float(), dev(w).float())
    e32.close()


# ------------------------------------------------------------------------------- 6: linear response in closed form
def lindhard(eta):
    with np.errstate(divide='ignore', invalid='ignore'):
        return 0.5 + (1 - eta ** 2) / (4 * eta) * np.log(np.abs((1 + eta) / (1 - eta)))


@pytest.mark.parametrize('name', ['WangTeter', 'Perrot', 'SmargiassiMadden', 'WangGovindCarter98', 'tf+vw', 'ThomasFermi'])
def test_get_inv_G_closed_forms(name):
    """functionals.get_inv_G on the 16^3 cubic grid: the Wang-Teter family reproduces the Lindhard function at every k != 0,
    TF + vW gives 1 / (1 + 3 eta^2), TF gives 1.  Relative to G_inv, 10 x the largest deviation measured on an MI355X
    (MEASURED_GINV; the reference's own get_inv_G(WangTeter) is within 2e-14 of Lindhard on g16r).  Measured: 1.21e-13 for the four
    Wang-Teter members (and for a user's stabiliser below), 2.1e-14 for TF + vW, 0 for TF."""
    _g, box, den, _w = gold('g16r')
    f = {'tf+vw': F.NativeTerms(['tf', 'vw'])}.get(name) or getattr(F, name)
    eta, G = F.get_inv_G(dev(box), dev(den), f)
    eta, G = eta.cpu().numpy(), G.cpu().numpy()
    assert eta.shape == G.shape == (16, 16, 9) and eta[0, 0, 0] == 0.0
    want = np.ones_like(eta) if name == 'ThomasFermi' else (1 / (1 + 3 * eta ** 2) if name == 'tf+vw' else lindhard(eta))
    m = eta != 0
    d = float(np.max(np.abs(G[m] - want[m]) / np.abs(want[m])))
    print('MEASURE get_inv_G %s: %.2e' % (name, d))
    assert d <= 10 * MEASURED_GINV
    assert abs(G[0, 0, 0] - 1.0) <= 10 * MEASURED_GINV          # k = 0: the Thomas-Fermi response alone


def test_get_inv_G_with_a_user_stabiliser_goes_through_autograd():
    """WangTeterStyleFunctional with a user's f composes three native energies in torch.  At the uniform density T_NL and its
    first derivative vanish, so the second derivative of T_TF f(T_NL / T_TF) is T_TF'' + f'(0) T_NL'' / f'(0) for every f with
    f(0) = 1: the response is WangTeter's, the Lindhard function"""
    _g, box, den, _w = gold('g16r')
    f = F.WangTeterStyleFunctional((5 / 6, 5 / 6, lambda x: 1 + x + x ** 2))
    assert f._kind is None
    eta, G = F.get_inv_G(dev(box), dev(den), f)
    eta, G = eta.cpu().numpy(), G.cpu().numpy()
    m = eta != 0
    d = float(np.max(np.abs(G[m] - lindhard(eta[m])) / lindhard(eta[m])))
    print('MEASURE get_inv_G user f: %.2e' % d)
    assert d <= 10 * MEASURED_GINV


# ------------------------------------------------------------------------------- 7: double backward through the drop-in terms
@pytest.mark.parametrize('case', hvp_cases.CASES)
def test_double_backward_through_the_drop_in_terms(case):
    """E = WangTeter + Hartree + PerdewZunger; v = grad(E, den, create_graph=True) is dE/dn_i = (potential) dV, so
    grad((v w).sum(), den) = H w and (H w) / dV is the golden's hv of cfg2 (whose ion-electron part is zero).
    Measured on an MI355X: 3.5e-14 / 5.4e-14 / 4.1e-14 / 3.4e-15 of max|hv| (g16r / g17r / g18t / g16d): the fused call's figures."""
    g, box, den, w = gold(case)
    tb, tw = dev(box), dev(w)
    dV = abs(np.linalg.det(box)) / den.size
    n = dev(den).requires_grad_()
    E = F.WangTeter(tb, n) + F.Hartree(tb, n) + F.PerdewZunger(tb, n)
    v = torch.autograd.grad(E, n, create_graph=True)[0]
    assert v.requires_grad
    hv = (torch.autograd.grad((v * tw).sum(), n)[0] / dV).cpu().numpy()
    ref = g['hv_cfg2'] - g['hv_ion_electron']
    d = float(np.abs(hv - ref).max() / np.abs(ref).max())
    print('MEASURE double backward %s: %.2e' % (case, d))
    assert d <= bound('cfg2')
    # the first derivative under create_graph is the one a plain backward returns, bit for bit
    n1 = dev(den).requires_grad_()
    v1 = torch.autograd.grad(F.WangTeter(tb, n1) + F.Hartree(tb, n1) + F.PerdewZunger(tb, n1), n1)[0]
    assert torch.equal(v.detach(), v1) and not v1.requires_grad
    # get_functional_derivative(requires_grad=True) is the same potential, differentiable
    n2 = dev(den)
    fd = F.get_functional_derivative(tb, n2, F.Hartree, requires_grad=True)
    assert fd.requires_grad
    hvh = torch.autograd.grad((fd * tw).sum(), n2)[0].cpu().numpy()
    assert float(np.abs(hvh - g['hv_hartree']).max() / np.abs(g['hv_hartree']).max()) <= bound('hartree')


MEASURED_WTS_USER = 5.40e-14  # 3.5e-14 / 5.4e-14 / 4.1e-14 / 3.4e-15 on g16r / g17r / g18t / g16d: largest of the four cases, MI355X (test_double_backward_through_a_user_stabiliser)


@pytest.mark.parametrize('case', hvp_cases.CASES)
def test_double_backward_through_a_user_stabiliser(case):
    """WangTeterStyleFunctional with a stabilisation function the engine does not know composes the native vW, TF and nonlocal
    energies in torch: T = vW + T_TF f(T_NL / T_TF).  On a non-uniform density the scalar factors in front of the native
    potentials depend on the density, so the second backward also needs the derivative of each potential node with respect to
    its incoming factor, sum(u v) dV -- 5e-5 of max|hv| here.  Against the reference's double autograd of the same composite
    (golden key wts_user), 10 x the largest deviation measured on an MI355X (MEASURED_WTS_USER)."""
    g, box, den, w = gold(case)
    tb, tw = dev(box), dev(w)
    dV = abs(np.linalg.det(box)) / den.size
    f = F.WangTeterStyleFunctional((5 / 6, 5 / 6, hvp_cases.user_stabiliser))
    assert f._kind is None
    n = dev(den).requires_grad_()
    v = torch.autograd.grad(f(tb, n), n, create_graph=True)[0]
    hv = (torch.autograd.grad((v * tw).sum(), n)[0] / dV).cpu().numpy()
    ref = g['hv_wts_user']
    plain = g['hv_vw'] + g['hv_tf'] + g['hv_wt_nl']
    assert np.abs(ref - plain).max() > 1e-5 * np.abs(ref).max()          # the composite differs from the plain sum: the factor path counts
    d = float(np.abs(hv - ref).max() / np.abs(ref).max())
    print('MEASURE double backward user f %s: %.2e' % (case, d))
    assert d <= 10 * MEASURED_WTS_USER


def test_mixed_cell_derivative_is_refused():
    _g, box, den, _w = gold('g16r')
    tb = dev(box).requires_grad_()
    n = dev(den).requires_grad_()
    with pytest.raises(NotImplementedError, match='box_vecs'):
        torch.autograd.grad(F.ThomasFermi(tb, n), n, create_graph=True)
