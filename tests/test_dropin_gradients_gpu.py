"""The layer professad's System calls -- professad_amd/functionals.py: _NativeEnergy, _NativePotential, NativeTerms, engine_for --
against the numpy double of tests/system_double.py, on one grid per transform family with full-spectrum densities
(tests/spectral_check.py) and the cells of tests/test_extent_matrix_gpu.py:

  (16, 8, 32) orthorhombic   fused power-of-two pipeline, unequal extents
  (27, 35, 33) triclinic     chirp-z (the smallest odd shape of tests/test_geometry_step_extents_gpu.py)
  (48, 16, 32) triclinic     mixed-radix line transform along x, fused pipeline (asserted: Engine.fast_path)

Per grid and per public callable with an oracle (system_double.CALLABLES; the tabulated-kernel terms keep tests/test_nlk_gpu.py):
  a. E and dE/dn from (2.5 f(box, n)).backward() at spectral_check's fp64 bounds (E_TOL, V_TOL, and its per-k-point criterion);
     n.grad / (2.5 dV) against get_functional_derivative;
  b. dE/dbox through the reference's get_stress recipe (functional_tools.py:94-99) with an upstream factor of 1.7, at 2e-10 of
     max|sigma|; under create_graph=True the call raises NotImplementedError;
  c. with nothing requiring grad E is bitwise the E of the call that also forms the potential.
Per grid, IonElectron and NativeTerms with 'ion_electron' (d-f), the way System strings the terms together (g-i) and inputs at the
edge (j); see the tests' docstrings.

a, second clause.  The backward returns (gE v) dV, so n.grad / (2.5 dV) is fl(fl(fl(2.5 v) dV) / fl(2.5 dV')) and
get_functional_derivative fl(fl(v dV) / dV'): the same potential v of the same deterministic engine call behind four and two
roundings (dV' the volume element get_functional_derivative forms on the device; the test divides by the same number).  2.5 v is
not exact in binary, so the two are equal bit for bit only where the roundings happen to agree -- 40 to 80 % of the grid points --
and no implementation of the backward can make them agree everywhere (a power of two as upstream factor would).  What is asserted
is what the roundings allow: six roundings of at most 2^-53 each, |difference| <= 3 * 2^-52 |v| at every grid point (the
user-lambda WangTeterStyleFunctional, whose three native potentials autograd sums: 16 * 2^-52 max|v|); the share of points that
agree bit for bit is recorded.

Measured on an MI355X, worst over the three grids and the 32 callables (per case: test_extent_matrix_gpu._record):
  a  E 1.1e-15 (bound 1e-13), dE/dn 4.9e-14 of max|v| (1.5e-12), per k-point 2.1e-11 (1e-9); against get_functional_derivative
     2.0 * 2^-52
  b  sigma 2.4e-13 of max|sigma| (non_local_KEF; every other callable <= 1.2e-14; bound 2e-10)
  d  dE/dv_ext 7.3e-16 (1e-15)       e  dE/dbox of IonElectron 1.1e-15 of |E| max|B^-T|, of the fused set 1.9e-15 (2e-10)
  f  contraction with dv_ext/dR 1.4e-14 of max|F| (2e-11)
  g  dispatch loop: E 3.4e-15, dE/dn 1.3e-14, per k-point 2.2e-12, against the fused call 3.7e-16 (1e-12)
  i  closure: E 1.7e-15, chi.grad 7.3e-15 (1.5e-12), per k-point 7.9e-13, against energy_grad_chi 8.9e-15 (1e-12)

The Wang-Teter nonlocal term on its own (non_local_KEF) is the case that found something: with the Lindhard factor in the
reference's direct form at every eta, dE/dn was 4.9e-12, 8.3e-12 and 6.7e-12 of max|v| on the three grids, above V_TOL -- the form
cancels twice for large eta (6.5e-11 absolute at eta = 12, where these grids reach; system_double.Evaluator evaluates the same
formula in extended precision).  lindhard_shape(double) now takes the cancellation-free series from eta = 3 on
(pointwise_kernels.h): 1.3e-14, 2.1e-14, 1.4e-14.
"""
import numpy as np
import pytest
import torch

import spectral_check as sc
import system_double as SD
import test_extent_matrix_gpu as M
from oracle import refpath
from professad_amd import functionals as F
from professad_amd.engine import Engine, engine_for
from professad_amd.ions import ion_electron_forces, ionic_potential_gradient

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GRIDS = [((16, 8, 32), 'ortho'), ((27, 35, 33), 'tri'), ((48, 16, 32), 'tri')]
GRID_IDS = ['%dx%dx%d-%s' % (s + (c,)) for s, c in GRIDS]
G_UP = 2.5                  # upstream factor of the density gradients
G_BOX = 1.7                 # ... of the lattice-vector gradients
ULP = 2.0 ** -52
SYSTEM_TERMS = ['ion_electron', 'hartree', 'wgc99', 'pbe']
SYSTEM_IDS = ['Hartree', 'WGC99', 'PerdewBurkeErnzerhof']

_CASES = {}
_CALLABLES = {}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.double, device=DEV)


def case(shape, cell):
    """inputs and the double of one grid, computed once per (shape, cell) and left unchanged; the per-callable (E, dE/dn, sigma)
    join the cache when first asked for"""
    key = (shape, cell)
    if key not in _CASES:
        box = M.make_cell(shape, cell)
        den, vext, chi = M.inputs(shape, cell)
        _CASES[key] = dict(box=box, den=den, vext=vext, chi=chi, d=SD.D(box, den), dV=abs(np.linalg.det(box)) / den.size,
                           tb=dev(box), doubles={})
    return _CASES[key]


def double(shape, cell, cid):
    o = case(shape, cell)
    if cid not in o['doubles']:
        o['doubles'][cid] = SD.DOUBLES[cid](o['d'])
    return o['doubles'][cid]


def fn(cid):
    if cid not in _CALLABLES:
        _CALLABLES[cid] = SD.FACTORIES[cid](F)
    return _CALLABLES[cid]


def maxrel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize('shape,cell', GRIDS, ids=GRID_IDS)
def test_grids_take_the_transform_family_they_stand_for(shape, cell):
    o = case(shape, cell)
    eng = engine_for(shape, DEV).set_cell(o['box'])
    assert eng.fast_path == (shape != (27, 35, 33)), (shape, eng.fast_path)
    assert round(float(o['den'].mean()) * abs(np.linalg.det(o['box']))) >= 1          # round(N_e) of WGC99 / vWGTF is not zero


# ------------------------------------------------------------------------------------------------ a-c: per grid and callable
@pytest.mark.parametrize('cid', SD.IDS)
@pytest.mark.parametrize('shape,cell', GRIDS, ids=GRID_IDS)
def test_energy_and_density_gradient_under_an_upstream_factor(shape, cell, cid):
    """a."""
    o, f = case(shape, cell), fn(cid)
    Eo, vo, _ = double(shape, cell, cid)
    n = dev(o['den']).requires_grad_()
    E = f(o['tb'], n)
    (G_UP * E).backward()
    v_np = (n.grad / (G_UP * o['dV'])).cpu().numpy()
    ev, ek = sc.errors(v_np, vo, 'f64')
    eE = abs(float(E) - Eo) / max(1.0, abs(Eo))
    # dV as get_functional_derivative forms it (functional_tools.py:31): determinants from numpy, torch on the host and torch on the
    # device differ by up to three units in the last place on these cells
    v = n.grad / (G_UP * (torch.abs(torch.linalg.det(o['tb'])) / n.numel()))
    gfd = F.get_functional_derivative(o['tb'], dev(o['den']), f)
    diff = (v - gfd).abs()
    same = float((diff == 0).double().mean())
    if cid == 'WTS-user':
        ulps, bound = float(diff.max() / gfd.abs().max()) / ULP, 16.0
    else:
        ulps, bound = float((diff / gfd.abs()).max()) / ULP, 3.0
    M._record(test='dropin', shape=shape, cell=cell, callable=cid, deriv='dE/dn', err_E=eE, err_v=ev, err_vk=ek,
              gfd_ulps=ulps, gfd_bitwise_share=same)
    print('MEASURE a %s %s %s: E %.1e v %.1e per-k %.1e; against get_functional_derivative %.2f ulp, %.3f of the points bitwise'
          % (shape, cell, cid, eE, ev, ek, ulps, same))
    assert ulps <= bound, (shape, cell, cid, ulps)
    assert eE <= sc.E_TOL['f64'], (shape, cell, cid, float(E), Eo)
    SD.check_field(v_np, vo, (shape, cell, cid), float(E), Eo)


def _get_stress(f, o, create_graph=False):
    """functional_tools.py:94-99 with an upstream factor"""
    b = o['tb'].clone().requires_grad_(True)
    vol = torch.abs(torch.linalg.det(b))
    E = f(b, dev(o['den']) * vol.detach() / vol)
    dEdcell = torch.autograd.grad(G_BOX * E, b, create_graph=create_graph)[0].T / G_BOX
    return (dEdcell @ b.detach() / vol.detach()).detach().cpu().numpy()


@pytest.mark.parametrize('cid', SD.IDS)
@pytest.mark.parametrize('shape,cell', GRIDS, ids=GRID_IDS)
def test_lattice_vector_gradient_through_the_get_stress_recipe(shape, cell, cid):
    """b."""
    o, f = case(shape, cell), fn(cid)
    sig = _get_stress(f, o)
    e = SD.rel(sig, double(shape, cell, cid)[2])
    M._record(test='dropin', shape=shape, cell=cell, callable=cid, deriv='dE/dbox', err_sigma=e)
    print('MEASURE b %s %s %s: sigma %.1e' % (shape, cell, cid, e))
    SD.check_stress(sig, double(shape, cell, cid)[2], SD.SIG_RTOL, (shape, cell, cid))
    with pytest.raises(NotImplementedError):
        _get_stress(f, o, create_graph=True)


@pytest.mark.parametrize('cid', SD.IDS)
@pytest.mark.parametrize('shape,cell', GRIDS, ids=GRID_IDS)
def test_energy_only_call_returns_the_bits_of_the_call_with_a_potential(shape, cell, cid):
    """c."""
    o, f = case(shape, cell), fn(cid)
    E_plain = f(o['tb'], dev(o['den']))
    E_grad = f(o['tb'], dev(o['den']).requires_grad_())
    assert not E_plain.requires_grad and E_grad.requires_grad
    assert torch.equal(E_plain, E_grad.detach()), (shape, cell, cid, float(E_plain), float(E_grad))


# ------------------------------------------------------------------------------------------- d-f: IonElectron, once per grid
def _ion_terms():
    return [('IonElectron', F.IonElectron, []), ('NativeTerms', F.NativeTerms(SYSTEM_TERMS), SYSTEM_IDS)]


@pytest.mark.parametrize('shape,cell', GRIDS, ids=GRID_IDS)
def test_gradient_with_respect_to_the_external_potential(shape, cell):
    """d. dE/dv_ext = gE n dV elementwise to 1e-15 relative (two fp64 multiplications), with n requiring grad or not, plain and
    under create_graph=True (both branches of _NativeEnergy.backward)"""
    o = case(shape, cell)
    want = dev((G_BOX * o['den']) * o['dV'])
    worst = 0.0
    for name, f, _ids in _ion_terms():
        for n_grad in (True, False):
            for cg in (False, True):
                n = dev(o['den']).requires_grad_(n_grad)
                vx = dev(o['vext']).requires_grad_()
                E = f(o['tb'], n, vx)
                (g,) = torch.autograd.grad(G_BOX * E, vx, create_graph=cg)
                e = float(((g.detach() - want).abs() / want).max())
                worst = max(worst, e)
                assert e <= 1e-15, (shape, name, n_grad, cg, e)
    M._record(test='dropin', shape=shape, cell=cell, callable='IonElectron', deriv='dE/dv_ext', err=worst)
    print('MEASURE d %s %s: %.2e' % (shape, cell, worst))


@pytest.mark.parametrize('shape,cell', GRIDS, ids=GRID_IDS)
def test_lattice_vector_gradient_at_a_fixed_external_potential(shape, cell):
    """e. IonElectron with box_vecs.requires_grad: dE/dbox = E B^-T (the documented partial derivative at fixed grid values of n and
    v_ext), E at E_TOL.  With further terms in one NativeTerms: B^T dE/dbox = vol sigma + (int v n) 1 with the double's sigma and
    potential (v_ext included), at the stress bound."""
    o = case(shape, cell)
    binvT = np.linalg.inv(o['box']).T
    Eo = o['d'].ev.ion_electron(o['den'], o['vext'])[0]
    for n_grad in (False, True):
        b = o['tb'].clone().requires_grad_()
        E = F.IonElectron(b, dev(o['den']).requires_grad_(n_grad), dev(o['vext']))
        (g,) = torch.autograd.grad(G_BOX * E, b)
        err = np.abs(g.cpu().numpy() / G_BOX - Eo * binvT).max()
        tol = (sc.E_TOL['f64'] * max(1.0, abs(Eo)) + 4 * ULP * abs(Eo)) * np.abs(binvT).max()
        M._record(test='dropin', shape=shape, cell=cell, callable='IonElectron', deriv='dE/dbox', n_grad=n_grad,
                  err=err / (abs(Eo) * np.abs(binvT).max()))
        print('MEASURE e %s %s IonElectron (n.requires_grad %s): %.2e (bound %.2e)' % (shape, cell, n_grad, err, tol))
        assert abs(float(E) - Eo) <= sc.E_TOL['f64'] * max(1.0, abs(Eo))
        assert err <= tol, (shape, n_grad, err, tol)
    ev = SD.evaluate(o['box'], o['den'], SYSTEM_IDS, o['vext'])['sum']
    vol = abs(np.linalg.det(o['box']))
    want = vol * ev[2] + float(np.sum(ev[1] * o['den']) * o['dV']) * np.eye(3)
    b = o['tb'].clone().requires_grad_()
    (g,) = torch.autograd.grad(G_BOX * F.NativeTerms(SYSTEM_TERMS)(b, dev(o['den']), dev(o['vext'])), b)
    got = o['box'].T @ (g.cpu().numpy() / G_BOX)
    e = SD.rel(got, want)
    M._record(test='dropin', shape=shape, cell=cell, callable='NativeTerms+ion_electron', deriv='dE/dbox', err=e)
    print('MEASURE e %s %s NativeTerms: %.2e' % (shape, cell, e))
    assert e <= SD.SIG_RTOL, (shape, e)


@pytest.mark.parametrize('shape,cell', GRIDS, ids=GRID_IDS)
def test_external_potential_gradient_contracts_to_the_ion_forces(shape, cell):
    """f. sum_r (dE/dv_ext)(r) (dv_ext/dR_a)(r) = dU/dR_a = -F_a for one ion of each species, to 2e-11 of max|F|: the sum of the two
    1e-11 bounds under which ionic_potential_gradient and ion_electron_forces are pinned"""
    o = case(shape, cell)
    rng = np.random.default_rng(sum(shape))
    species = SD.tables([(rng.random((2, 3)) * 1.6 - 0.3, SD.golden_recpot()), (rng.random((3, 3)) * 1.6 - 0.3, SD.second_recpot()[:2])])
    eng = engine_for(shape, DEV)
    vx = dev(o['vext']).requires_grad_()
    (g,) = torch.autograd.grad(G_BOX * F.IonElectron(o['tb'], dev(o['den']), vx), vx)
    Fs = np.concatenate(ion_electron_forces(eng, o['box'], dev(o['den']), species))
    worst = 0.0
    for ion in (1, 3):
        dv = ionic_potential_gradient(eng, o['box'], species, ion)
        dU = (dv * g[None]).sum(dim=(1, 2, 3)).cpu().numpy() / G_BOX
        worst = max(worst, float(np.abs(dU + Fs[ion]).max() / np.abs(Fs).max()))
    M._record(test='dropin', shape=shape, cell=cell, callable='IonElectron', deriv='dE/dv_ext . dv_ext/dR', err=worst)
    print('MEASURE f %s %s: %.2e of max|F|' % (shape, cell, worst))
    assert worst <= 2e-11, (shape, worst)


# ----------------------------------------------------------------------------------------------------- g-i: the way System uses it
def test_dispatch_loop_over_several_systems_with_one_backward():
    """g. System.__compute_energy's dispatch (system.py:759-772) over IonElectron, Hartree, WGC99, PBE for three systems at once --
    two shapes, and the first shape again in another cell (one shared engine: a set_cell / set_terms switch on every call) --
    alternating term by term, then ONE backward for the three sums.  Each n.grad is the double's (every term's saved potential is
    its own, no cell or parameter slot leaks) and the fused NativeTerms result to 1e-12."""
    systems = [((16, 8, 32), 'ortho'), ((27, 35, 33), 'tri'), ((16, 8, 32), 'tri')]
    terms = [F.IonIon, F.IonElectron, F.Hartree, F.WangGovindCarter99().forward, F.PerdewBurkeErnzerhof]
    os_ = [case(*s) for s in systems]
    ns = [dev(o['den']).requires_grad_() for o in os_]
    vxs = [dev(o['vext']) for o in os_]
    Es = [torch.zeros((1,), dtype=torch.double, device=DEV) for _ in systems]
    for f in terms:
        for i, o in enumerate(os_):
            if f.__qualname__ == 'IonElectron':
                Es[i] = Es[i] + f(o['tb'], ns[i], vxs[i])
            elif f.__qualname__ == 'IonIon':
                continue
            else:
                Es[i] = Es[i] + f(o['tb'], ns[i])
    (Es[0] + Es[1] + Es[2]).backward()
    fused = F.NativeTerms(SYSTEM_TERMS)
    for i, (s, o) in enumerate(zip(systems, os_)):
        Eo, vo, _ = SD.evaluate(o['box'], o['den'], SYSTEM_IDS, o['vext'])['sum']
        ev, ek, eE = SD.check_field((ns[i].grad / o['dV']).cpu().numpy(), vo, ('dispatch', s), float(Es[i]), Eo)
        n2 = dev(o['den']).requires_grad_()
        E2 = fused(o['tb'], n2, vxs[i])
        E2.backward()
        ef = maxrel(ns[i].grad, n2.grad)
        M._record(test='dropin', shape=s[0], cell=s[1], callable='dispatch loop', deriv='dE/dn', err_E=eE, err_v=ev, err_vk=ek,
                  err_fused=ef)
        print('MEASURE g %s: E %.1e v %.1e per-k %.1e, against the fused call %.1e' % (s, eE, ev, ek, ef))
        assert ef <= 1e-12 and abs(float(Es[i]) - float(E2)) <= 1e-12 * abs(float(E2)), (s, ef)


@pytest.mark.parametrize('shape,cell', GRIDS, ids=GRID_IDS)
def test_parameters_of_other_terms_do_not_leak(shape, cell):
    """h. f1, then terms that set the same parameter slots to other values, then f1 again: the same bits"""
    o = case(shape, cell)
    others = [F.WangGovindCarter99(init_args=(SD.WGC98[0], SD.WGC98[1], 3.2, 1.0)), fn('PG1'), fn('non_local_KEF'), fn('PGSLr'),
              fn('vWGTF2'), fn('WTS-exp')]

    def run(f):
        n = dev(o['den']).requires_grad_()
        E = f(o['tb'], n)
        E.backward()
        return E.detach(), n.grad

    for cid in ('WGC99', 'PGSL025', 'WangTeter', 'vWGTF1'):
        first = run(fn(cid))
        for g in others:
            run(g)
        again = run(fn(cid))
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1]), (shape, cid)


@pytest.mark.parametrize('shape,cell', GRIDS, ids=GRID_IDS)
def test_closure_through_autograd(shape, cell):
    """i. n = N chi^2 / (sum chi^2 dV) formed in torch, E.backward(): chi.grad is Engine.energy_grad_chi's gradient to 1e-12 and
    refpath.closure's (the reference's own closure, system.py:830-838) at V_TOL; chi of mixed sign"""
    o = case(shape, cell)
    sign = np.where(np.random.default_rng(sum(shape)).random(shape) < 0.5, -1.0, 1.0)
    chi_np = o['chi'] * sign
    assert 0.4 < (chi_np < 0).mean() < 0.6
    n_elec = float(np.floor(o['den'].mean() * abs(np.linalg.det(o['box']))) + 0.3)
    chi = dev(chi_np).requires_grad_()
    n = n_elec * chi ** 2 / ((chi ** 2).sum() * o['dV'])
    vx = dev(o['vext'])
    E = F.IonElectron(o['tb'], n, vx) + F.Hartree(o['tb'], n) + F.WangGovindCarter99()(o['tb'], n) + F.PerdewBurkeErnzerhof(o['tb'], n)
    E.backward()
    fused = F.NativeTerms(SYSTEM_TERMS)
    eng = Engine(shape, DEV).set_cell(o['box']).set_terms(fused.names, fused.params)
    Ee, _mu, ge = eng.energy_grad_chi(dev(chi_np), n_elec, vx)
    eng.close()
    e_eng = maxrel(chi.grad, ge)
    tab = refpath.term_table(torch.as_tensor(o['vext']))
    Er, gr = refpath.closure(torch.as_tensor(o['box']), torch.as_tensor(chi_np), n_elec,
                             [tab[k] for k in ('ion_electron', 'hartree', 'wgc99', 'pbe_x', 'pbe_c')])
    ev, ek, eE = SD.check_field(chi.grad.cpu().numpy(), gr.numpy(), ('closure', shape), float(E), float(Er))
    M._record(test='dropin', shape=shape, cell=cell, callable='closure', deriv='dE/dchi', err_E=eE, err_v=ev, err_vk=ek,
              err_engine=e_eng)
    print('MEASURE i %s %s: E %.1e chi.grad %.1e per-k %.1e, against energy_grad_chi %.1e' % (shape, cell, eE, ev, ek, e_eng))
    assert e_eng <= 1e-12 and abs(float(E) - sum(Ee.values())) <= 1e-12 * abs(float(E)), (shape, e_eng)


# ------------------------------------------------------------------------------------------------------- j: inputs at the edge
@pytest.mark.parametrize('shape,cell', GRIDS, ids=GRID_IDS)
def test_inputs_at_the_edge(shape, cell):
    """j."""
    o = case(shape, cell)
    f = F.NativeTerms(['hartree', 'wt', 'pbe'])
    base = dev(o['den']).permute(2, 1, 0).contiguous()
    view = base.permute(2, 1, 0)                          # the density's values behind other strides
    assert not view.is_contiguous() and torch.equal(view, dev(o['den']))
    res = []
    for n in (view.detach().requires_grad_(), dev(o['den']).requires_grad_()):
        E = f(o['tb'], n)
        E.backward()
        res.append((E.detach(), n.grad))
    assert not view.is_contiguous()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    with pytest.raises(TypeError):
        f(o['tb'], dev(o['den']).float())
    with pytest.raises(ValueError):
        f(o['tb'], torch.as_tensor(o['den']))
    n = dev(o['den']).requires_grad_()
    E = f(o['tb'], n)
    with torch.no_grad():
        n.mul_(1.5)
    with pytest.raises(RuntimeError, match='modified by an inplace operation'):
        E.backward()
