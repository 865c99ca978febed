"""Pin the oracle: both CPU restatements must reproduce the reference's own outputs
(fixtures made by tests/golden/make_golden.py running profess-ad itself)."""
import os

import numpy as np
import pytest
import torch

import cases
from oracle import closed_form as cf
from oracle import refpath as rp

GOLDEN = os.path.dirname(os.path.abspath(cases.__file__))


def load(name):
    return np.load(os.path.join(GOLDEN, name))


def relerr(a, b):
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-300))


def test_recip_grid_matches_reference_wavevecs():
    gold = load('wavevecs.npz')
    box = cases.make_cell(('tri', 0.3))
    for shape in [(4, 4, 4), (5, 5, 5), (6, 6, 6), (4, 5, 6)]:
        tag = 'x'.join(map(str, shape))
        got_np = cf.recip(box, shape)
        got_t = rp.recip_grid(torch.as_tensor(box), shape)
        for comp, a, b in zip(('kx', 'ky', 'kz', 'k2'), got_np, got_t):
            ref = gold['%s_%s' % (tag, comp)]
            assert relerr(a, ref) < 1e-14
            assert relerr(b.numpy(), ref) < 1e-14


def test_wgc99_kernel_matches_reference():
    gold = load('wgc99_kernel_g16r.npz')
    w0, w1, w2 = cf.wgc_kernel(gold['eta'])
    for got, ref in zip((w0, w1, w2), gold['kernel']):
        assert relerr(got, ref) < 1e-12
    k = rp.Wgc99().build_kernel(torch.as_tensor(gold['eta'])).numpy()
    assert relerr(k, gold['kernel']) < 1e-13


def test_wgc99_fourth_table_is_a_combination_of_two_others():
    """the engine stores (w0, K1 | K2) and forms K3 = K2 + ((3 - gamma) / (3 n_ref)) K1 in registers (csrc/pointwise_kernels.h: MixWgc,
    wgc_table_kernel): the identity on the REFERENCE's own kernel derivatives (functionals.py:968-972 on the golden w, w', w'')"""
    gold = load('wgc99_kernel_g16r.npz')
    eta = gold['eta']
    w0, w1, w2 = gold['kernel']
    for ga, nref in ((2.7, 0.03), (2.2, 0.17), (4.2, 1.3)):
        K1 = -eta * w1 / (6 * nref)
        K2 = (eta ** 2 * w2 + (7 - ga) * eta * w1) / (36 * nref ** 2)
        K3 = (eta ** 2 * w2 + (1 + ga) * eta * w1) / (36 * nref ** 2)
        ck = (3 - ga) / (3 * nref)
        assert np.abs(K3 - (K2 + ck * K1)).max() <= 1e-14 * max(np.abs(K3).max(), np.abs(K2).max(), np.abs(ck * K1).max())


@pytest.mark.parametrize('case', cases.PER_TERM_CASES)
def test_per_term_energy_and_potential(case):
    gold = load('terms_%s.npz' % case)
    box, den, vext, chi, n_elec = cases.make_inputs(case)
    assert abs(cases.checksum(den, vext, chi) - float(gold['input_checksum'])) < 1e-9
    ev = cf.Evaluator(cf.Grid(box, den.shape))
    table = rp.term_table(torch.as_tensor(vext))
    tb, td = torch.as_tensor(box), torch.as_tensor(den)
    for nm in cases.SINGLE_TERMS:
        Eref, vref = float(gold['E_' + nm]), gold['v_' + nm]
        # closed form
        E, v = ev.term(nm, den, vext)
        assert abs(E - Eref) <= 1e-12 * max(1.0, abs(Eref)), (nm, E, Eref)
        assert relerr(v, vref) < 2e-11, (nm, relerr(v, vref))
        # op-for-op autograd restatement
        E2, v2 = rp.energy_and_potential(tb, td, table[nm])
        assert abs(float(E2) - Eref) <= 1e-13 * max(1.0, abs(Eref)), (nm, float(E2), Eref)
        assert relerr(v2.numpy(), vref) < 1e-12, (nm, relerr(v2.numpy(), vref))


@pytest.mark.parametrize('case', cases.FUSED_CASES)
def test_fused_configs_and_closure(case):
    gold = load('fused_%s.npz' % case)
    box, den, vext, chi, n_elec = cases.make_inputs(case)
    assert abs(cases.checksum(den, vext, chi) - float(gold['input_checksum'])) < 1e-9
    assert n_elec == float(gold['n_elec'])
    ev = cf.Evaluator(cf.Grid(box, den.shape))
    for cfg, names in cases.CONFIGS.items():
        E, Es, v = ev.terms(names, den, vext)
        Eref = float(gold['E_' + cfg])
        assert abs(E - Eref) <= 1e-12 * max(1.0, abs(Eref))
        assert relerr(v, gold['v_' + cfg]) < 2e-11
        Ec, g, mu = ev.closure(names, chi, n_elec, vext)
        assert abs(Ec - float(gold['Ec_' + cfg])) <= 1e-12 * max(1.0, abs(Ec))
        assert relerr(g, gold['g_' + cfg]) < 2e-11
    if case in ('g16r', 'g17r'):
        table = rp.term_table(torch.as_tensor(vext))
        for cfg, names in cases.CONFIGS.items():
            Ec, g = rp.closure(torch.as_tensor(box), torch.as_tensor(chi), n_elec, [table[n] for n in names])
            assert abs(float(Ec) - float(gold['Ec_' + cfg])) <= 1e-13 * max(1.0, abs(float(Ec)))
            assert relerr(g.numpy(), gold['g_' + cfg]) < 1e-12


def test_ionic_potential_oracle():
    from oracle import ions as oi
    g = load('ions.npz')
    raw, kmax = g['recpot_raw'], float(g['recpot_kmax'])
    assert oi.recpot_table(raw, kmax)[2] == int(g['z']) == 3
    for order in (2, 3, 6, 10):
        assert relerr(oi.cardinal_b_spline(g['bspline_x'], order), g['bspline_%d' % order]) < 1e-14
    for tag, shape, orders in (('a', (32, 32, 32), (4, 10)), ('b', (16, 20, 24), (6,))):
        box, frac = g[tag + '_box'], g[tag + '_frac']
        k2 = cf.recip(box, shape)[3]
        assert relerr(oi.recpot_on_grid(raw, kmax, np.sqrt(k2)), g[tag + '_vk']) < 1e-13
        assert relerr(oi.structure_factor_exact(box, shape, frac), g[tag + '_S_exact']) < 1e-12
        assert relerr(oi.ionic_potential(box, shape, frac, raw, kmax, None), g[tag + '_v_exact']) < 1e-12
        for o in orders:
            assert relerr(oi.structure_factor_pme(shape, frac, o), g['%s_S_pme%d' % (tag, o)]) < 1e-11
            assert relerr(oi.ionic_potential(box, shape, frac, raw, kmax, o), g['%s_v_pme%d' % (tag, o)]) < 1e-11
    # the config-1 fixture's v_ext is this potential (reference System, exact structure factor)
    c1 = load('cfg1_fccAl_32.npz')
    assert relerr(oi.ionic_potential(c1['box'], (32, 32, 32), g['a_frac'], raw, kmax, None), c1['vext']) < 1e-10


def test_ion_electron_forces_oracle():
    """analytic force restatement against the reference's autograd forces (exact and PME structure factors)"""
    from oracle import ions as oi
    from professad_amd import synth
    g = load('ions.npz')
    raw, kmax = g['recpot_raw'], float(g['recpot_kmax'])
    for tag, shape, order, dk in (('a', (32, 32, 32), 10, dict(seed=8, n0=0.03, amp=0.5)),
                                  ('b', (16, 20, 24), 6, dict(seed=7, n0=0.05, amp=0.5))):
        den = synth.smooth_density(shape, **dk)
        for o in (None, order):
            F = oi.ion_electron_forces(g[tag + '_box'], shape, g[tag + '_frac'], den, raw, kmax, o)
            ref = g[tag + '_force_exact'] if o is None else g['%s_force_pme%d' % (tag, o)]
            assert np.abs(F - ref).max() < 1e-13, (tag, o)


def test_stress_oracle():
    """closed-form / derived stress restatements against the reference's get_stress (autograd) outputs"""
    from oracle import stress as st
    from professad_amd import synth
    g = load('stress.npz')
    for case in ('g16r', 'gmix', 'g18t'):
        box, den, vext, chi, n_elec = cases.make_inputs(case)
        got = {'hartree': st.hartree(box, den), 'tf': st.tf(box, den), 'vw': st.vw(box, den), 'wt_nl': st.wt_nl(box, den),
               'lda_x': st.lda(box, den, 'lda_x'), 'pz_c': st.lda(box, den, 'pz_c'), 'pw_c': st.lda(box, den, 'pw_c'),
               'chachiyo_c': st.lda(box, den, 'chachiyo_c'), 'pbe_x': st.pbe(box, den, True, False),
               'pbe_c': st.pbe(box, den, False, True),
               'wgc99': st.tf(box, den) + st.vw(box, den) + st.wgc99_nl(box, den),
               'pgsl025': st.vw(box, den) + st.pauli_gaussian(box, den),
               'pgslr': st.vw(box, den) + st.pauli_gaussian(box, den, 40 / 27, 0.25, 0.4, 0.2),
               'wts_exp': st.wang_teter_style(box, den),
               'lkt': st.vw(box, den) + st.ggak(box, den, 'lkt'),
               'pgs': st.vw(box, den) + st.pauli_gaussian(box, den, 40 / 27, beta=0.0),
               'vwgtf1': st.vw(box, den) + st.vwgtf(box, den, 1), 'vwgtf2': st.vw(box, den) + st.vwgtf(box, den, 2)}
        for k, v in got.items():
            ref = g['%s_%s' % (case, k)]
            assert np.abs(v - ref).max() <= 1e-11 * np.abs(ref).max(), (case, k)
    ions = load('ions.npz')
    raw, kmax = ions['recpot_raw'], float(ions['recpot_kmax'])
    for tag, shape, order, dk in (('a', (32, 32, 32), 10, dict(seed=8, n0=0.03, amp=0.5)),
                                  ('b', (16, 20, 24), 6, dict(seed=7, n0=0.05, amp=0.5))):
        den = synth.smooth_density(shape, **dk)
        for o in (None, order):
            s = st.ion_electron(ions[tag + '_box'], den, ions[tag + '_frac'], raw, kmax, o)
            ref = g['%s_ion_electron_%s' % (tag, 'exact' if o is None else 'pme%d' % o)]
            assert np.abs(s - ref).max() <= 1e-12 * np.abs(ref).max(), (tag, o)


def _ion_ion_cases():
    import json
    doc = json.load(open(os.path.join(GOLDEN, 'ion_ion_known_answers.json')))
    out = {}
    for c in doc['cases']:
        box = np.array(c['box'], dtype=np.float64)
        cart = np.array(c['cart'], dtype=np.float64) if c['cart'] is not None else np.array(c['frac'], dtype=np.float64) @ box
        out[c['name']] = (box, cart, np.array(c['charges'], dtype=np.float64), c['h_max'], c['expected'])
    return out, doc['madelung']


def test_ion_ion_oracle_known_answers_and_derivatives():
    """energies against the reference's own known-answer values; forces / stress formulas against finite differences of
    that energy (fixed Rc, Rd: the quantities autograd holds constant)"""
    from oracle import ionion as ii
    cs, madelung = _ion_ion_cases()
    E = {}
    for name in ('Al', 'Si', 'SiO2', 'NaCl_fcc', 'NaCl_two'):
        box, cart, z, h, want = cs[name]
        E[name] = ii.energy(box, cart, z, 12 * h, 2 * h)
        if want is not None:
            assert abs(E[name] - want) / len(z) < 1e-10, name
    assert abs(4 * E['NaCl_fcc'] - E['NaCl_two'] - madelung) < 1e-10
    # derivatives on a small low-symmetry case (the reference's FD-stress cell, tests/test_ion_utils.py:151-155)
    box = np.array([[6.5, -0.13, 0.25], [-0.33, 7.21, 0.24], [0.55, 0.04, 6.78]])
    frac = np.array([[0, 0, 0], [0.35, 0.65, 0.45]])
    z = np.array([1.0, 1.0])
    Rc, Rd = ii.heuristics(box)
    Rc *= 0.5                                            # keep the CPU test short; still converged to ~1e-9
    F, sig = ii.forces_stress(box, frac @ box, z, Rc, Rd)
    h = 1e-5
    for a, d in ((0, 0), (1, 2)):
        cp, cm = (frac @ box).copy(), (frac @ box).copy()
        cp[a, d] += h
        cm[a, d] -= h
        fd = -(ii.energy(box, cp, z, Rc, Rd) - ii.energy(box, cm, z, Rc, Rd)) / (2 * h)
        assert abs(fd - F[a, d]) < 1e-8
    vol = abs(np.linalg.det(box))
    for i, j in ((0, 0), (1, 2)):
        eps = np.zeros((3, 3))
        eps[i, j] += 0.5 * h
        eps[j, i] += 0.5 * h
        bp, bm = box + box @ eps, box - box @ eps
        fd = (ii.energy(bp, frac @ bp, z, Rc, Rd) - ii.energy(bm, frac @ bm, z, Rc, Rd)) / (2 * h * vol)
        assert abs(fd - sig[i, j]) < 1e-8, (i, j, fd, sig[i, j])
