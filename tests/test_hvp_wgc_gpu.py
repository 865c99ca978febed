"""GPU tests of the second derivatives of WGC99 under OFDFT_OPT_HVP_WGC = 1: the WGC99 stage of
ofdft_hessian_vector / Engine.hessian_vector against the reference's double autograd (tests/golden/hvp_wgc_<case>.npz; generator
tests/golden/make_golden_hvp_wgc.py), the numpy double (tests/hvp_wgc_double.py) on grids without goldens, a uniform density,
symmetry, reuse, and the switch itself.

Tolerance rule: the yardstick is the numpy double's own deviation from the reference's goldens, YARDSTICK below, computed without a
device by tests/test_hvp_wgc_cpu.py (its MEASURED; the table is a copy).  Per key hv (relative to max|golden|) and q (relative to
|q|) may deviate by 10 x that figure -- the device's transforms and fm:: functions round differently from numpy's; ten is the
factor every Hessian test here uses -- and q, a sum with cancellation, by no less than ten roundings of its own terms
(10 eps sum|w hv| dV / |q|).  A figure above 1e-11 would be a finding (FINDING).  The reuse test is bitwise.  Every test prints its
figures as `MEASURE ...` before it asserts; the MI355X figures are in the docstrings.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cases
import hvp_cases
import hvp_wgc_cases as G
import hvp_wgc_double as W
from professad_amd import _native as N
from professad_amd import synth
from professad_amd.engine import Engine

pytestmark = pytest.mark.gpu
GOLDEN = os.path.dirname(os.path.abspath(cases.__file__))
DEV = 'cuda:0'
FINDING = 1e-11
EPS = 2.0 ** -52
# tests/test_hvp_wgc_cpu.py: the numpy double against the goldens, the larger of the hv and q figures over g16r, g17r, g18t, g16d
YARDSTICK = {'wgc99_nl': 9.72e-15, 'wgc99': 7.39e-16, 'cfg3w': 8.82e-16, 'cfg2w': 7.43e-16}
# transforms of a product and of its reuse call: wgc99_nl alone 6 + 6 + 6 + 6 = 24 and 12; the LDA set adds hartree's 2 and vw's
# 4 / 2; the bench set adds PBE's 12 / 8 to that
FFT_WGC, FFT_CFG2W, FFT_CFG3W = (24, 12), (30, 16), (42, 24)
CFG2_PLAIN = hvp_cases.SETS['cfg2']


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.double, device=DEV)


_GOLD = {}


def gold(case):
    """golden file and inputs of a case, loaded once and shared"""
    if case not in _GOLD:
        g = np.load(os.path.join(GOLDEN, 'hvp_wgc_%s.npz' % case))
        box, den, _vext = G.make_inputs(case)
        w = G.direction(den.shape)
        assert abs(cases.checksum(box, den, w) - float(g['checksum'])) < 1e-9
        _GOLD[case] = (g, box, den, w)
    return _GOLD[case]


def engine(shape, box, names, wgc=1, gga=1):
    eng = Engine(shape, DEV).set_cell(box).set_terms(list(names))
    if wgc is not None:
        eng.set_option(N.OPT_HVP_WGC, wgc)
    if gga is not None:
        eng.set_option(N.OPT_HVP_GGA, gga)
    return eng


def q_floor(w, hv, dV, q):
    """ten roundings of the terms of q = sum w hv dV, relative to |q|"""
    return 10 * EPS * float(np.abs(w * hv).sum() * dV) / abs(q)


# ------------------------------------------------------------------------------- 1: goldens
@pytest.mark.parametrize('case', G.CASES)
def test_wgc99_terms_and_sets_match_the_reference_goldens(case):
    """hv and q through Engine.hessian_vector for wgc99_nl, the whole functional, cfg3w and cfg2w (g16r: the power-of-two plan, g17r:
    chirp-z, g18t: 18 x 20 x 16 triclinic, g16d: ten times the density); q_5 also against sum w hv dV of the returned field.

    Measured max|hv - golden| / max|golden| on an MI355X, g16r / g17r / g18t / g16d (the test prints every figure before it asserts):
        wgc99_nl 9.6e-15 / 6.0e-15 / 5.4e-15 / 1.7e-15      wgc99 6.0e-16 / 1.1e-15 / 9.7e-16 / 6.3e-16
        cfg3w    6.1e-16 / 1.1e-15 / 9.9e-16 / 5.1e-16      cfg2w 7.0e-16 / 1.2e-15 / 1.0e-15 / 5.1e-16
        q at most 4.7e-16; q_5 of a set equal to the single-term call's (at most 2.1e-16 from its golden); q_5 against the returned
        field at most 4.3e-16.
    The numpy double sits at 9.7e-15 / 7.4e-16 / 8.8e-16 / 7.4e-16 against the same goldens: the device is where the double is, and every
    figure is inside ten times that."""
    g, box, den, w = gold(case)
    dV = abs(np.linalg.det(box)) / den.size
    td, tw = dev(den), dev(w)
    eng = Engine(den.shape, DEV).set_cell(box).set_option(N.OPT_HVP_WGC, 1).set_option(N.OPT_HVP_GGA, 1)
    figs = []
    for key, names in G.KEYS.items():
        q, hv = eng.set_terms(list(names)).hessian_vector(td, tw, want_terms=True)      # (the options outlive set_terms)
        hv = hv.cpu().numpy()
        ref, qref = g['hv_' + key], float(g['q_' + key])
        d = float(np.abs(hv - ref).max() / np.abs(ref).max())
        dq = abs(sum(q.values()) - qref) / abs(qref)
        print('MEASURE hvp_wgc %s %s: hv %.2e q %.2e (bound %.2e, q floor %.2e)' % (case, key, d, dq, 10 * YARDSTICK[key], q_floor(w, ref, dV, qref)))
        figs.append((key, d, dq, q_floor(w, ref, dV, qref)))
        assert all(v == 0.0 for k, v in q.items() if k not in names)
        if key == 'wgc99_nl':            # the tail kernel's sum against the returned field
            qf = float((w * hv).sum() * dV)
            dfield = abs(q['wgc99_nl'] - qf) / abs(qf)
            print('MEASURE hvp_wgc %s q_5 against the field: %.2e' % (case, dfield))
        else:                            # the per-term entry of a sum is that of the single-term call
            dterm = abs(q['wgc99_nl'] - float(g['q_wgc99_nl'])) / abs(float(g['q_wgc99_nl']))
            print('MEASURE hvp_wgc %s %s q_5 against the single-term golden: %.2e' % (case, key, dterm))
            figs.append(('wgc99_nl', 0.0, dterm, q_floor(w, g['hv_wgc99_nl'], dV, float(g['q_wgc99_nl']))))
    eng.close()
    assert all(v <= FINDING for v in YARDSTICK.values())
    assert dfield <= q_floor(w, g['hv_wgc99_nl'], dV, float(g['q_wgc99_nl']))
    for key, d, dq, floor in figs:
        assert d <= 10 * YARDSTICK[key], (case, key, d)
        assert dq <= max(10 * YARDSTICK[key], floor), (case, key, dq)


# ------------------------------------------------------------------------------- 2: transform families without goldens
@pytest.mark.parametrize('shape,triclinic', [((48, 96, 32), True), ((32, 16, 64), False)])
def test_mixed_radix_and_unequal_powers_of_two_match_the_double(shape, triclinic):
    """cfg3w against tests/hvp_wgc_double.py on a mixed-radix triclinic grid and on unequal powers of two: hv within 10 x the cfg3w
    yardstick, q_5 within 10 x the wgc99_nl one.  Measured on an MI355X: hv 1.0e-15 and 8.5e-16, q_5 1.7e-16 and 1.5e-16 (N = 3422.62
    and 14.96)."""
    box = synth.triclinic_cell(shape[0] / 8.0) if triclinic else synth.cubic_cell(32)
    den = synth.random_density(shape, seed=11)
    w = hvp_cases.direction(shape, seed=78)
    nel = float(den.mean() * abs(np.linalg.det(box)))
    assert abs(nel % 1.0 - 0.5) >= G.HALF_INTEGER_MARGIN, nel
    dV = abs(np.linalg.det(box)) / den.size
    qd, hvd = W.hessian_vector(box, den, w, G.CFG3W)
    eng = engine(shape, box, G.CFG3W)
    assert eng.fast_path
    q, hv = eng.hessian_vector(dev(den), dev(w), want_terms=True)
    nfft = eng.query(N.Q_FFT_COUNT)
    eng.close()
    d = float(np.abs(hv.cpu().numpy() - hvd).max() / np.abs(hvd).max())
    dq = abs(q['wgc99_nl'] - qd['wgc99_nl']) / abs(qd['wgc99_nl'])
    floor = q_floor(w, W.wgc_hv(box, den, w), dV, qd['wgc99_nl'])
    print('MEASURE hvp_wgc double %s: hv %.2e  q_5 %.2e (floor %.2e)  N %.3f' % (shape, d, dq, floor, nel))
    assert nfft == FFT_CFG3W[0]
    assert d <= 10 * YARDSTICK['cfg3w']
    assert dq <= max(10 * YARDSTICK['wgc99_nl'], floor)


def test_uniform_density_with_integer_n():
    """n = 3 / 512 on an 8 bohr cube, kappa = 1: every step from the box to n_ref is exact in binary on the device (the volume by
    cofactors, the sum of 4096 equal values, 3 / 512), so theta = 0 exactly and B, C, Q, S are fields of zeros (their transforms run
    all the same: 24).  numpy's determinant is 512 (1 - 1e-15), so the double's theta is a few roundings of n instead.  hv of wgc99_nl
    against the double, relative to max|hv|: 10 x the yardstick.  Measured on an MI355X: 1.0e-15 of max|hv| = 1.10."""
    shape, box = (16, 16, 16), np.eye(3) * 8.0
    den = np.full(shape, 3.0 / 512.0)
    w = hvp_cases.direction(shape, seed=80)
    hvd = W.wgc_hv(box, den, w)
    eng = engine(shape, box, ('wgc99_nl',))
    q, hv = eng.hessian_vector(dev(den), dev(w), want_terms=True)
    nfft = eng.query(N.Q_FFT_COUNT)
    eng.close()
    hv = hv.cpu().numpy()
    d = float(np.abs(hv - hvd).max() / np.abs(hvd).max())
    print('MEASURE hvp_wgc uniform: hv %.2e  max|hv| %.3e  q_5 %.6e' % (d, np.abs(hvd).max(), q['wgc99_nl']))
    assert nfft == FFT_WGC[0] and np.isfinite(hv).all()
    assert d <= 10 * YARDSTICK['wgc99_nl']


# ------------------------------------------------------------------------------- 3: symmetry
def test_hessian_is_symmetric():
    """<u, H w> = <w, H u> for two independent directions on g18t with cfg3w, to the tolerance of cfg3w times |u| |H w|
    (measured on an MI355X: 8.4e-18 of it)"""
    _g, box, den, w = gold('g18t')
    u = hvp_cases.direction(den.shape, seed=79)
    eng = engine(den.shape, box, G.CFG3W)
    td = dev(den)
    Hw = eng.hessian_vector(td, dev(w)).cpu().numpy()
    Hu = eng.hessian_vector(td, dev(u), reuse_density=True).cpu().numpy()
    eng.close()
    a, b = float((u * Hw).sum()), float((w * Hu).sum())
    scale = np.linalg.norm(u) * np.linalg.norm(Hw)
    print('MEASURE hvp_wgc symmetry: %.2e' % (abs(a - b) / scale))
    assert abs(a - b) <= 10 * YARDSTICK['cfg3w'] * scale


# ------------------------------------------------------------------------------- 4: reuse
@pytest.mark.parametrize('case', ['g16r', 'g17r'])
def test_reuse_density_is_bitwise_and_skips_twelve_transforms(case):
    """U = M a and G = M p join the retained fields: a reuse call returns the same bits and sums and skips their twelve transforms;
    set_terms, an evaluation, set_option and set_cell invalidate; Engine.precondition between two reuse calls changes nothing.
    Counts: wgc99_nl alone 24 / 12, the LDA set 30 / 16, the bench set 42 / 24."""
    _g, box, den, w = gold(case)
    td, tw = dev(den), dev(w)
    counts = {}
    for name, names in (('wgc', ('wgc99_nl',)), ('cfg2w', G.CFG2W)):
        e = engine(den.shape, box, names, gga=None)
        q0, h0 = e.hessian_vector(td, tw, want_terms=True)
        c = [e.query(N.Q_FFT_COUNT)]
        q1, h1 = e.hessian_vector(td, tw, reuse_density=True, want_terms=True)
        c.append(e.query(N.Q_FFT_COUNT))
        e.close()
        assert torch.equal(h0, h1) and q0 == q1
        counts[name] = tuple(c)

    eng = engine(den.shape, box, G.CFG3W)
    with pytest.raises(RuntimeError, match=r'\(-3\)'):          # nothing retained yet: OFDFT_ESTATE
        eng.hessian_vector(td, tw, reuse_density=True)
    q0, hv0 = eng.hessian_vector(td, tw, want_terms=True)
    c3 = [eng.query(N.Q_FFT_COUNT)]
    q1, hv1 = eng.hessian_vector(td, tw, reuse_density=True, want_terms=True)
    c3.append(eng.query(N.Q_FFT_COUNT))
    print('MEASURE hvp_wgc reuse %s: transforms wgc %s  cfg2w %s  cfg3w %s' % (case, counts['wgc'], counts['cfg2w'], c3))
    assert counts['wgc'] == FFT_WGC and counts['cfg2w'] == FFT_CFG2W and tuple(c3) == FFT_CFG3W
    assert torch.equal(hv0, hv1) and q0 == q1
    assert torch.equal(eng.hessian_vector(td, tw, reuse_density=True), hv0)          # without the host read of the sums
    # the preconditioner between two reuse calls leaves the retained fields alone
    eng.precondition(tw, 1.3)
    assert torch.equal(eng.hessian_vector(td, tw, reuse_density=True), hv0)
    # set_terms, an energy call, set_option and set_cell invalidate
    eng.set_terms(['tf'])
    eng.set_terms(list(G.CFG3W))
    with pytest.raises(RuntimeError, match=r'\(-3\)'):
        eng.hessian_vector(td, tw, reuse_density=True)
    assert torch.equal(eng.hessian_vector(td, tw), hv0)
    eng.energy_potential(td, dev(np.zeros(den.shape)))
    with pytest.raises(RuntimeError, match=r'\(-3\)'):
        eng.hessian_vector(td, tw, reuse_density=True)
    assert torch.equal(eng.hessian_vector(td, tw), hv0)
    eng.set_option(N.OPT_HVP_WGC, 1)
    with pytest.raises(RuntimeError, match=r'\(-3\)'):
        eng.hessian_vector(td, tw, reuse_density=True)
    assert torch.equal(eng.hessian_vector(td, tw), hv0)
    eng.set_cell(box * 1.01)
    with pytest.raises(RuntimeError, match=r'\(-3\)'):
        eng.hessian_vector(td, tw, reuse_density=True)
    eng.close()


# ------------------------------------------------------------------------------- 5: the switch
def test_the_switch_and_what_stays_refused():
    """off (never set, 0, or only OPT_HVP_GGA = 1): today's (-1) message naming wgc99_nl; on: the products run, the multi and strain
    entries still name it -- at the C ABI, under Engine's own refusals; OPT_HVP_WGC = 1 alone still refuses pbe_x; values other than
    0 and 1 are OFDFT_EINVAL; the fp32 library accepts the option; term sets without wgc99_nl are bitwise unchanged by it"""
    _g, box, den, w = gold('g16r')
    td, tw = dev(den), dev(w)
    n_elec = float(den.sum() * abs(np.linalg.det(box)) / den.size)
    eng = engine(den.shape, box, G.CFG2W, wgc=None, gga=None)
    assert eng.option(N.OPT_HVP_WGC) is None

    def refused(term):
        with pytest.raises(RuntimeError, match=r'\(-1\).*ofdft_hessian_vector: no second derivative of the term %s$' % term):
            eng.hessian_vector(td, tw)
        with pytest.raises(RuntimeError, match=r'\(-1\).*ofdft_hessian_vector_chi: no second derivative of the term %s$' % term):
            eng.hessian_vector_chi(td, tw, None, n_elec)

    refused('wgc99_nl')
    eng.set_option(N.OPT_HVP_WGC, 0)
    refused('wgc99_nl')
    eng.set_option(N.OPT_HVP_GGA, 1)
    refused('wgc99_nl')
    for bad in (2, -1, 0.5):
        with pytest.raises(RuntimeError, match=r'\(-1\).*OFDFT_OPT_HVP_WGC takes 0 or 1'):
            eng.set_option(N.OPT_HVP_WGC, bad)
    assert eng.option(N.OPT_HVP_WGC) == 0.0                    # a refused value is not recorded
    eng.set_option(N.OPT_HVP_GGA, 0).set_option(N.OPT_HVP_WGC, 1)
    assert eng.option(N.OPT_HVP_WGC) == 1.0
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
        print('MEASURE hvp_wgc switch %s: %d %s' % (name, rc, msg))
        assert rc == N.EINVAL and msg == '%s: no second derivative of the term wgc99_nl' % name
    with pytest.raises(NotImplementedError, match='hessian_vector_chi_multi: .*wgc99_nl.*batching is what is missing'):
        eng.hessian_vector_chi_multi(td, tw[None], n_elec)
    for call in (eng.strain_hessian, eng.potential_strain_gradient):
        with pytest.raises(NotImplementedError, match='wgc99_nl.*strain derivative of WGC99'):
            call(td)
    # OPT_HVP_WGC = 1 alone: PBE stays refused
    eng.set_terms(list(G.CFG3W))
    refused('pbe_x')
    eng.close()
    # a term set without wgc99_nl: the same bits with the option off and on
    names, al, be = CFG2_PLAIN
    hv = {}
    for value in (0, 1):
        e = Engine(den.shape, DEV).set_cell(box).set_terms(list(names), dict(wt_alpha=al, wt_beta=be)).set_option(N.OPT_HVP_WGC, value)
        hv[value] = e.hessian_vector(td, tw, want_terms=True)
        e.close()
    assert torch.equal(hv[0][1], hv[1][1]) and hv[0][0] == hv[1][0]
    e32 = Engine(den.shape, DEV, dtype=torch.float32).set_cell(box).set_terms(['tf'])
    assert e32.set_option(N.OPT_HVP_WGC, 1).option(N.OPT_HVP_WGC) == 1.0
    with pytest.raises(RuntimeError, match=r'\(-1\).*OFDFT_OPT_HVP_WGC'):
        e32.set_option(N.OPT_HVP_WGC, 3)
    e32.close()
