"""GPU tests of the second derivatives of PBE exchange and correlation under OFDFT_OPT_HVP_GGA = 1: the second
transform stage of ofdft_hessian_vector / Engine.hessian_vector against the reference's double autograd
(tests/golden/hvp_gga_<case>.npz; generator tests/golden/make_golden_hvp_gga.py), the numpy double (tests/hvp_gga_double.py) on
grids without goldens, symmetry, reuse, and the switch itself.

Tolerance rule (that of tests/test_hvp_gpu.py): per key, 10 x the largest max|hv - golden| / max|golden| measured on an MI355X over
the four golden cases (MEASURED below; the tests' docstrings list the figures per case); q takes the same bound relative to |q|.
A figure above 1e-11 would be a finding (FINDING), not a number to record.  Every test prints its figures as `MEASURE ...` before it
asserts.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cases
import hvp_cases
import hvp_gga_cases as G
import hvp_gga_double as H
from professad_amd import _native as N
from professad_amd import synth
from professad_amd.engine import Engine

pytestmark = pytest.mark.gpu
GOLDEN = os.path.dirname(os.path.abspath(cases.__file__))
DEV = 'cuda:0'
KEYS = {**{k: (v, None, None) for k, v in G.TERMS.items()}, **G.SETS}
CFG3, AL, BE = G.CFG3
CFG2 = hvp_cases.SETS['cfg2'][0]
FINDING = 1e-11
# largest measured deviation per key over g16r, g17r, g18t, g16d, MI355X (test_pbe_terms_and_cfg3_match_the_reference_goldens)
MEASURED = {'pbe_x': 2.10e-15, 'pbe_c': 2.56e-15, 'pbe': 6.05e-15, 'cfg3': 2.70e-14}
# ... of |q_t - sum w hv_t dV| / |q_t| for the single-term keys: the mid kernel's sums (adjoint identity) against the returned field
MEASURED_Q_FIELD = 3.41e-16
# measured on an MI355X against tests/hvp_gga_double.py, per shape: max|hv - double| / max|double|, and the largest |q_t - double| / |double|
MEASURED_DOUBLE = {(48, 96, 32): dict(hv=2.12e-15, q=1.03e-15), (32, 16, 64): dict(hv=7.38e-14, q=4.33e-13)}
# transforms of a product and of its reuse call: pbe_x + pbe_c alone 2 + 6 + 3 + 1 = 12 and 1 + 3 + 3 + 1 = 8; cfg3 adds hartree's 2,
# vw's 4 / 2 and wt_nl's 4 / 2 (alpha = beta); cfg2 is 10 / 6 (tests/test_hvp_gpu.py)
FFT_PBE, FFT_CFG3, FFT_CFG2 = (12, 8), (22, 14), (10, 6)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.double, device=DEV)


def params_of(al, be):
    return None if al is None else dict(wt_alpha=al, wt_beta=be)


_GOLD = {}


def gold(case):
    """golden file and inputs of a case, loaded once and shared"""
    if case not in _GOLD:
        g = np.load(os.path.join(GOLDEN, 'hvp_gga_%s.npz' % case))
        box, den, _vext = G.make_inputs(case)
        w = G.direction(den.shape)
        assert abs(cases.checksum(box, den, w) - float(g['checksum'])) < 1e-9
        _GOLD[case] = (g, box, den, w)
    return _GOLD[case]


def engine(shape, box, names, al=None, be=None, gga=1):
    eng = Engine(shape, DEV).set_cell(box).set_terms(list(names), params_of(al, be))
    return eng.set_option(N.OPT_HVP_GGA, gga) if gga is not None else eng


# ------------------------------------------------------------------------------- 1: goldens
@pytest.mark.parametrize('case', G.CASES)
def test_pbe_terms_and_cfg3_match_the_reference_goldens(case):
    """hv and q through Engine.hessian_vector for pbe_x, pbe_c, both and cfg3 (g16r: the power-of-two plan, g17r: chirp-z, g18t:
    18 x 20 x 16 triclinic, g16d: r_s < 1); for the single-term keys q_t also against sum w hv_t dV of the returned field.

    Measured max|hv - golden| / max|golden| on an MI355X, g16r / g17r / g18t / g16d (the test prints every figure before it asserts):
        pbe_x 7.0e-16 / 1.8e-15 / 2.1e-15 / 8.3e-16      pbe_c 4.9e-16 / 2.5e-15 / 2.6e-15 / 5.0e-16
        pbe   4.0e-15 / 5.0e-15 / 6.1e-15 / 2.7e-15      cfg3  1.9e-14 / 2.2e-14 / 2.7e-14 / 2.1e-15
        q: at most 4.9e-16 (pbe_x), 4.7e-16 (pbe_c), 3.3e-15 (pbe), 2.4e-15 (cfg3); q_t against the returned field at most 3.4e-16.
    The numpy double sits at 7.9e-16 / 1.3e-15 / 3.9e-15 / 4.8e-15 against the same goldens (tests/test_hvp_gga_cpu.py).  `pbe` stands
    above its parts because exchange and correlation cancel to a fifth of either; cfg3 carries the Wang-Teter kernel's conditioning
    as cfg2 does (5.5e-14 there, tests/test_hvp_gpu.py).  All far below the 1e-11 that would be a finding."""
    g, box, den, w = gold(case)
    dV = abs(np.linalg.det(box)) / den.size
    td, tw = dev(den), dev(w)
    eng = Engine(den.shape, DEV).set_cell(box).set_option(N.OPT_HVP_GGA, 1)
    figs = []
    for key, (names, al, be) in KEYS.items():
        q, hv = eng.set_terms(list(names), params_of(al, be)).hessian_vector(td, tw, want_terms=True)      # (the option outlives set_terms)
        hv = hv.cpu().numpy()
        ref, qref = g['hv_' + key], float(g['q_' + key])
        d = float(np.abs(hv - ref).max() / np.abs(ref).max())
        dq = abs(sum(q.values()) - qref) / abs(qref)
        dfield = abs(sum(q.values()) - float((w * hv).sum() * dV)) / abs(qref)
        print('MEASURE hvp_gga %s %s: hv %.2e q %.2e (q vs field %.2e)' % (case, key, d, dq, dfield))
        figs.append((key, d, dq, dfield))
        assert all(v == 0.0 for k, v in q.items() if k not in names)
        if key == 'cfg3':                # the per-term entries of the sum are those of the single-term calls
            qt = {t: abs(q[t] - float(g['q_' + t])) / abs(float(g['q_' + t])) for t in ('pbe_x', 'pbe_c')}
            print('MEASURE hvp_gga %s cfg3 per term: q_pbe_x %.2e q_pbe_c %.2e' % (case, qt['pbe_x'], qt['pbe_c']))
    eng.close()
    assert all(v <= FINDING for v in MEASURED.values())
    for key, d, dq, dfield in figs:
        assert d <= 10 * MEASURED[key], (case, key, d)
        assert dq <= 10 * MEASURED[key], (case, key, dq)
        if key in ('pbe_x', 'pbe_c'):
            assert dfield <= 10 * MEASURED_Q_FIELD, (case, key, dfield)
            assert qt[key] <= 10 * MEASURED[key], (case, key, qt)         # (measured: equal to the single-term call's q_t)


# ------------------------------------------------------------------------------- 2: transform families without goldens
@pytest.mark.parametrize('shape,triclinic', [((48, 96, 32), True), ((32, 16, 64), False)])
def test_mixed_radix_and_unequal_powers_of_two_match_the_double(shape, triclinic):
    """cfg3 against tests/hvp_gga_double.py on a mixed-radix triclinic grid and on unequal powers of two: 10 x the figure measured
    for this shape (MEASURED_DOUBLE), for hv and for every q_t (`q`: the largest of them).  Measured on an MI355X: hv 2.1e-15 and 7.4e-14; q_t at most 1.0e-15 (pbe_c) on
    (48, 96, 32), and 4.3e-13 on (32, 16, 64), which is wt_nl's -- the kernel's conditioning at eta up to 15.1, as in tests/test_hvp_gpu.py --
    with pbe_x equal to the last bit and pbe_c at 5.9e-16 there."""
    box = synth.triclinic_cell(shape[0] / 8.0) if triclinic else synth.cubic_cell(32)
    den = synth.random_density(shape, seed=11)
    w = hvp_cases.direction(shape, seed=78)
    qd, hvd = H.hessian_vector(box, den, w, CFG3, AL, BE)
    eng = engine(shape, box, CFG3, AL, BE)
    assert eng.fast_path
    q, hv = eng.hessian_vector(dev(den), dev(w), want_terms=True)
    nfft = eng.query(N.Q_FFT_COUNT)
    eng.close()
    m = MEASURED_DOUBLE[shape]
    d = float(np.abs(hv.cpu().numpy() - hvd).max() / np.abs(hvd).max())
    dq = {t: abs(q[t] - qd[t]) / abs(qd[t]) for t in CFG3 if t != 'ion_electron'}
    print('MEASURE hvp_gga double %s: hv %.2e  q %s' % (shape, d, ' '.join('%s %.2e' % kv for kv in dq.items())))
    assert nfft == FFT_CFG3[0]
    assert m['hv'] <= FINDING and d <= 10 * m['hv']
    assert max(dq.values()) <= 10 * m['q'], dq
    assert q['ion_electron'] == 0.0


# ------------------------------------------------------------------------------- 3: symmetry
def test_hessian_is_symmetric():
    """<u, H w> = <w, H u> for two independent directions on g18t with cfg3, to the tolerance of cfg3 times |u| |H w|
    (measured on an MI355X: 1.3e-17 of it)"""
    _g, box, den, w = gold('g18t')
    u = hvp_cases.direction(den.shape, seed=79)
    eng = engine(den.shape, box, CFG3, AL, BE)
    td = dev(den)
    Hw = eng.hessian_vector(td, dev(w)).cpu().numpy()
    Hu = eng.hessian_vector(td, dev(u), reuse_density=True).cpu().numpy()
    eng.close()
    a, b = float((u * Hw).sum()), float((w * Hu).sum())
    scale = np.linalg.norm(u) * np.linalg.norm(Hw)
    print('MEASURE hvp_gga symmetry: %.2e' % (abs(a - b) / scale))
    assert abs(a - b) <= 10 * MEASURED['cfg3'] * scale


# ------------------------------------------------------------------------------- 4: reuse
@pytest.mark.parametrize('case', ['g16r', 'g17r'])
def test_reuse_density_is_bitwise_and_skips_four_more_transforms(case):
    """grad n joins the retained fields: a reuse call returns the same bits and sums, skips one forward and three inverse
    transforms more than cfg2's reuse does, and is invalidated by what invalidates cfg2's -- set_option included;
    Engine.precondition between two reuse calls changes nothing.  Counts: pbe_x + pbe_c alone 12 / 8, cfg3 22 / 14."""
    _g, box, den, w = gold(case)
    td, tw = dev(den), dev(w)
    e2 = engine(den.shape, box, CFG2, AL, BE, gga=None)
    e2.hessian_vector(td, tw)
    c2 = [e2.query(N.Q_FFT_COUNT)]
    e2.hessian_vector(td, tw, reuse_density=True)
    c2.append(e2.query(N.Q_FFT_COUNT))
    e2.close()
    assert tuple(c2) == FFT_CFG2
    ep = engine(den.shape, box, ('pbe_x', 'pbe_c'))
    hp = ep.hessian_vector(td, tw)
    cp = [ep.query(N.Q_FFT_COUNT)]
    assert torch.equal(ep.hessian_vector(td, tw, reuse_density=True), hp)
    cp.append(ep.query(N.Q_FFT_COUNT))
    ep.close()
    assert tuple(cp) == FFT_PBE

    eng = engine(den.shape, box, CFG3, AL, BE)
    with pytest.raises(RuntimeError, match=r'\(-3\)'):          # nothing retained yet: OFDFT_ESTATE
        eng.hessian_vector(td, tw, reuse_density=True)
    q0, hv0 = eng.hessian_vector(td, tw, want_terms=True)
    c3 = [eng.query(N.Q_FFT_COUNT)]
    q1, hv1 = eng.hessian_vector(td, tw, reuse_density=True, want_terms=True)
    c3.append(eng.query(N.Q_FFT_COUNT))
    print('MEASURE hvp_gga reuse %s: transforms cfg2 %s  pbe %s  cfg3 %s' % (case, c2, cp, c3))
    assert tuple(c3) == FFT_CFG3 and (c3[0] - c3[1]) - (c2[0] - c2[1]) == 4
    assert torch.equal(hv0, hv1) and q0 == q1
    assert torch.equal(eng.hessian_vector(td, tw, reuse_density=True), hv0)          # without the host read of the sums
    # the preconditioner between two reuse calls leaves the retained fields alone
    eng.precondition(tw, 1.3)
    assert torch.equal(eng.hessian_vector(td, tw, reuse_density=True), hv0)
    # set_terms, an energy call, set_option and set_cell invalidate
    eng.set_terms(['tf'])
    eng.set_terms(list(CFG3), params_of(AL, BE))
    with pytest.raises(RuntimeError, match=r'\(-3\)'):
        eng.hessian_vector(td, tw, reuse_density=True)
    assert torch.equal(eng.hessian_vector(td, tw), hv0)
    eng.energy_potential(td, dev(np.zeros(den.shape)))
    with pytest.raises(RuntimeError, match=r'\(-3\)'):
        eng.hessian_vector(td, tw, reuse_density=True)
    assert torch.equal(eng.hessian_vector(td, tw), hv0)
    eng.set_option(N.OPT_HVP_GGA, 1)
    with pytest.raises(RuntimeError, match=r'\(-3\)'):
        eng.hessian_vector(td, tw, reuse_density=True)
    assert torch.equal(eng.hessian_vector(td, tw), hv0)
    eng.set_cell(box * 1.01)
    with pytest.raises(RuntimeError, match=r'\(-3\)'):
        eng.hessian_vector(td, tw, reuse_density=True)
    eng.close()


# ------------------------------------------------------------------------------- 5: the switch
def test_the_switch_and_what_stays_refused():
    """off (never set, or 0): today's (-1) message naming pbe_x; on: the products run, the multi and strain entries still name it --
    at the C ABI, under Engine's own refusals -- wgc99_nl next to PBE is refused as wgc99_nl; values other than 0 and 1 are
    OFDFT_EINVAL; the fp32 library accepts the option"""
    _g, box, den, w = gold('g16r')
    td, tw = dev(den), dev(w)
    n_elec = float(den.sum() * abs(np.linalg.det(box)) / den.size)
    eng = engine(den.shape, box, CFG3, AL, BE, gga=None)
    assert eng.option(N.OPT_HVP_GGA) is None
    for value in (None, 0):
        if value is not None:
            eng.set_option(N.OPT_HVP_GGA, value)
        with pytest.raises(RuntimeError, match=r'\(-1\).*ofdft_hessian_vector: no second derivative of the term pbe_x$'):
            eng.hessian_vector(td, tw)
        with pytest.raises(RuntimeError, match=r'\(-1\).*ofdft_hessian_vector_chi: no second derivative of the term pbe_x$'):
            eng.hessian_vector_chi(td, tw, None, n_elec)
    for bad in (2, -1, 0.5):
        with pytest.raises(RuntimeError, match=r'\(-1\).*OFDFT_OPT_HVP_GGA'):
            eng.set_option(N.OPT_HVP_GGA, bad)
    assert eng.option(N.OPT_HVP_GGA) == 0.0                    # a refused value is not recorded
    eng.set_option(N.OPT_HVP_GGA, 1)
    assert eng.option(N.OPT_HVP_GGA) == 1.0
    eng.hessian_vector(td, tw)
    eng.hessian_vector_chi(td, tw, None, n_elec)
    # the library's multi and strain entries, called past Engine's own refusals
    lib, ctx, st = eng.lib, eng._ctx, eng._stream()
    out = torch.empty((6,) + tuple(td.shape), dtype=td.dtype, device=td.device)
    ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    w2 = (C.c_double * (N.NTERMS * 81))()
    for name, call in (('ofdft_hessian_vector_chi_multi',
                        lambda: lib.ofdft_hessian_vector_chi_multi(ctx, ptr(td), ptr(tw), eng.npts, 1, n_elec, ptr(out), eng.npts, None, 0, st)),
                       ('ofdft_potential_strain_gradient', lambda: lib.ofdft_potential_strain_gradient(ctx, ptr(td), ptr(out), st)),
                       ('ofdft_strain_hessian', lambda: lib.ofdft_strain_hessian(ctx, ptr(td), w2, st))):
        rc = call()
        msg = lib.ofdft_last_error(ctx).decode()
        print('MEASURE hvp_gga switch %s: %d %s' % (name, rc, msg))
        assert rc == N.EINVAL and msg == '%s: no second derivative of the term pbe_x' % name
    with pytest.raises(NotImplementedError, match='hessian_vector_chi_multi: .*pbe_x.*batching is what is missing'):
        eng.hessian_vector_chi_multi(td, tw[None], n_elec)
    for call in (eng.strain_hessian, eng.potential_strain_gradient):
        with pytest.raises(NotImplementedError, match='pbe_x.*strain derivative of PBE'):
            call(td)
    eng.set_terms(['tf', 'vw', 'wgc99_nl', 'pbe_x', 'pbe_c'])
    with pytest.raises(RuntimeError, match=r'\(-1\).*no second derivative of the term wgc99_nl$'):
        eng.hessian_vector(td, tw)
    eng.set_terms(['pbe_c']).set_option(N.OPT_HVP_GGA, 0)
    with pytest.raises(RuntimeError, match=r'\(-1\).*no second derivative of the term pbe_c$'):
        eng.hessian_vector(td, tw)
    eng.close()
    e32 = Engine(den.shape, DEV, dtype=torch.float32).set_cell(box).set_terms(['tf'])
    assert e32.set_option(N.OPT_HVP_GGA, 1).option(N.OPT_HVP_GGA) == 1.0
    with pytest.raises(RuntimeError, match=r'\(-1\).*OFDFT_OPT_HVP_GGA'):
        e32.set_option(N.OPT_HVP_GGA, 3)
    e32.close()
