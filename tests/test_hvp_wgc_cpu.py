"""Second derivatives of WGC99 without a device: the numpy double (tests/hvp_wgc_double.py) against the reference's
double autograd (tests/golden/hvp_wgc_<case>.npz, tn_wgc_<case>.npz), the option's Python name, and who refuses wgc99_nl when the
option is off, on, and on the batched and elastic paths -- on fake engines, before any device work.  Every test prints its figures
as `MEASURE ...` before it asserts.  The figures of MEASURED and MEASURED_CHI are the yardstick of the GPU tests
(tests/test_hvp_wgc_gpu.py, tests/test_tn_wgc_gpu.py): they owe nothing to the HIP code."""
import os
import sys

import numpy as np
import pytest
import torch

from professad_amd import _native as N
from professad_amd import elastic, force_constants, optimize

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
sys.path.insert(0, HERE)
import cases  # noqa: E402
import hvp_wgc_cases as G  # noqa: E402
import hvp_wgc_double as W  # noqa: E402
import tn_cases  # noqa: E402

# Largest of max|hv - golden| / max|golden| and |q - golden| / |q| over g16r, g17r, g18t, g16d, measured with numpy 2 / torch 2 on
# x86-64: numpy.fft against torch.fft, the oracle's Horner series against the reference's, and the order of the pointwise
# arithmetic are the only sources.  wgc99_nl alone stands above the sets because its max|hv| is 0.3 .. 0.7 where theirs is 7 .. 70
# (the von Weizsaecker term): the same absolute deviation.  Per case, hv: wgc99_nl 9.7e-15 / 5.9e-15 / 5.4e-15 / 1.6e-15,
# wgc99 6.0e-16 / 7.4e-16 / 6.9e-16 / 5.7e-16, cfg3w 6.1e-16 / 8.8e-16 / 8.2e-16 / 5.1e-16, cfg2w 5.0e-16 / 7.4e-16 / 7.4e-16 / 5.1e-16;
# q at most 4.0e-16.
MEASURED = {'wgc99_nl': 9.72e-15, 'wgc99': 7.39e-16, 'cfg3w': 8.82e-16, 'cfg2w': 7.43e-16}
# ... and of max|H d - golden| / max|golden| and |d.H d - golden| / |golden| in chi space over g16r, g17r, g18t (cfg3w):
# 8.2e-16 / 9.0e-16 / 1.3e-15 and 0 / 1.4e-16 / 2.7e-16
MEASURED_CHI = dict(Hd=1.27e-15, dHd=2.67e-16)
FINDING = 1e-13          # a figure above this is a finding, not a number to record


@pytest.fixture(scope='module', params=G.CASES)
def case(request):
    g = np.load(os.path.join(HERE, 'golden', 'hvp_wgc_%s.npz' % request.param))
    box, den, _vext = G.make_inputs(request.param)
    w = G.direction(den.shape)
    assert cases.checksum(box, den, w) == pytest.approx(float(g['checksum']), rel=1e-12)       # generator drift
    assert np.array_equal(w, g['w'])
    return request.param, g, box, den, w


def test_cases_stay_clear_of_the_jumps_of_round_n():
    """round(N) is a constant of the differentiation only away from its jumps: every case at least 0.1 from a half-integer"""
    for name in G.CASES:
        box, den, _vext = G.make_inputs(name)
        frac = float(den.mean() * abs(np.linalg.det(box))) % 1.0
        print('MEASURE hvp_wgc cpu %s: fractional part of N %.2f' % (name, frac))
        assert abs(frac - 0.5) >= G.HALF_INTEGER_MARGIN


@pytest.mark.parametrize('key', list(G.KEYS))
def test_double_matches_the_reference_double_autograd(case, key):
    """hv and q of wgc99_nl, the whole functional, cfg3w and cfg2w.  Asserted: 10 x MEASURED per key, for hv relative to max|golden|
    and for q relative to |q|."""
    name, g, box, den, w = case
    assert all(v <= FINDING for v in MEASURED.values())
    q, hv = W.hessian_vector(box, den, w, G.KEYS[key])
    ref, qref = g['hv_' + key], float(g['q_' + key])
    dev = np.abs(hv - ref).max() / np.abs(ref).max()
    qdev = abs(sum(q.values()) - qref) / abs(qref)
    print('MEASURE hvp_wgc cpu %s %s: hv %.2e  q %.2e  max|hv| %.3e' % (name, key, dev, qdev, np.abs(ref).max()))
    assert dev <= 10 * MEASURED[key]
    assert qdev <= 10 * MEASURED[key]


def test_first_derivative_in_the_same_notation_is_the_oracle_s():
    """E_NL = c dV sum p . U and v = c sum p' U + a' G against the oracle's WGC99 (oracle/refpath.py: its energy and autograd potential
    minus TF and vW): the notation the Hessian form is written in is the evaluation's"""
    from oracle import refpath
    box, den, _vext = G.make_inputs('g18t')
    E, v = W.energy_potential(box, den)
    tb, td = torch.as_tensor(box), torch.as_tensor(den)
    wgc = refpath.Wgc99()
    Er, vr = refpath.energy_and_potential(tb, td, lambda b, d: wgc(b, d) - refpath.thomas_fermi(b, d) - refpath.weizsaecker(b, d))
    dE, dv = abs(E - float(Er)) / abs(float(Er)), float(np.abs(v - vr.numpy()).max() / np.abs(vr.numpy()).max())
    print('MEASURE hvp_wgc cpu first derivative g18t: E %.2e v %.2e' % (dE, dv))
    assert dE <= 1e-13 and dv <= 1e-12


@pytest.mark.parametrize('name', G.TN_CASES)
def test_chi_space_double_matches_the_reference(name):
    """H d of the closure for cfg3w at phi = 1.7 sqrt(den) with the reference's own gradient g, against grad((g d).sum(), chi); N is
    the caller's n_elec (1.3 and 2.3: rounded to 1 and 2)"""
    g = np.load(os.path.join(HERE, 'golden', 'tn_wgc_%s.npz' % name))
    box, phi, d, vext, n_elec = tn_cases.make_inputs(name)
    assert cases.checksum(box, phi, d, vext) == pytest.approx(float(g['checksum']), rel=1e-12)
    assert abs(n_elec % 1.0 - 0.5) >= G.HALF_INTEGER_MARGIN
    s, Hd = W.hessian_vector_chi(box, phi, d, g['g'], n_elec, G.CFG3W)
    dev = np.abs(Hd - g['Hd']).max() / np.abs(g['Hd']).max()
    qdev = abs(s['dHd'] - float(g['dHd'])) / abs(float(g['dHd']))
    print('MEASURE hvp_wgc cpu chi %s: Hd %.2e  dHd %.2e' % (name, dev, qdev))
    assert all(v <= FINDING for v in MEASURED_CHI.values())
    assert dev <= 10 * MEASURED_CHI['Hd'] and qdev <= 10 * MEASURED_CHI['dHd']
    assert ('chi_gs' in g) == (name in G.GS_CASES)


def test_option_is_exported():
    header = open(os.path.join(os.path.dirname(HERE), 'include', 'ofdft_hip.h')).read()
    assert '#define OFDFT_OPT_HVP_WGC %d ' % N.OPT_HVP_WGC in header
    taken = [getattr(N, nm) for nm in dir(N) if nm.startswith('OPT_') and nm != 'OPT_HVP_WGC']
    assert N.OPT_HVP_WGC == 19 and N.OPT_HVP_WGC not in taken


class _FakeEngine:
    """what the refusals read of an engine; `options`: None = an engine without the accessor, else option number -> value"""

    def __init__(self, names, options=None):
        self.comm, self.dtype = None, torch.double
        mask = 0
        for nm in names:
            mask |= N.TERM_BITS[nm]
        self._terms_key = (mask, np.zeros(N.NPARAMS).tobytes())
        if options is not None:
            self.option = lambda opt: options.get(int(opt))

    def _mask(self):
        return self._terms_key[0]


BENCH = ['ion_electron', 'hartree', 'tf', 'vw', 'wgc99_nl', 'pbe_x', 'pbe_c']
WGC_LDA = ['ion_electron', 'hartree', 'tf', 'vw', 'wgc99_nl', 'lda_x', 'pz_c']
SPECIES = [(np.zeros((1, 3)), (None, None, 3))]
WGC_ON, GGA_ON = {N.OPT_HVP_WGC: 1.0}, {N.OPT_HVP_GGA: 1.0}
BOTH_ON = {**WGC_ON, **GGA_ON}


@pytest.mark.parametrize('options', [None, {}, {N.OPT_HVP_WGC: 0.0}, GGA_ON])
def test_option_off_refuses_as_before(options):
    """no accessor, never set, set to 0, only OPT_HVP_GGA = 1: today's message, on every path"""
    e = _FakeEngine(BENCH, options)
    print('MEASURE hvp_wgc cpu refusal off (%r): %s' % (options, optimize.second_order_refusal(e)))
    assert not optimize.hvp_wgc_enabled(e)
    assert optimize.second_order_refusal(e) == 'no second derivative of the term wgc99_nl'
    assert optimize.response_refusal(e) == 'no second derivative of the term wgc99_nl'
    assert force_constants.refusal(e) == elastic.refusal(e) == 'no second derivative of the term wgc99_nl'
    assert force_constants.batch_refusal(e) == 'no second derivative of the term wgc99_nl'
    with pytest.raises(NotImplementedError, match='no second derivative of the term wgc99_nl$'):
        optimize.HipCgBackend(e)
    with pytest.raises(NotImplementedError, match="n_method='TN': no second derivative of the term wgc99_nl$"):
        optimize.optimize_density(e, 3.0, n_method='TN', volume=1.0)


def test_option_on_serves_the_single_column_paths_and_names_what_is_missing_elsewhere():
    e = _FakeEngine(WGC_LDA, WGC_ON)
    assert optimize.hvp_wgc_enabled(e) and not optimize.hvp_gga_enabled(e)
    assert optimize.second_order_refusal(e) is None and optimize.response_refusal(e) is None and force_constants.refusal(e) is None
    # OPT_HVP_WGC alone still refuses PBE; both options open the bench set
    assert optimize.second_order_refusal(_FakeEngine(BENCH, WGC_ON)) == 'no second derivative of the term pbe_x'
    both = _FakeEngine(BENCH, BOTH_ON)
    assert optimize.second_order_refusal(both) is None and force_constants.refusal(both) is None
    assert optimize.second_order_refusal(_FakeEngine(WGC_LDA + ['gga_k'], WGC_ON)) == 'no second derivative of the term gga_k'
    # batched paths: batching is what is missing
    for eng in (e, both):
        for why in (optimize.second_order_refusal(eng, gga_missing='batch'), force_constants.batch_refusal(eng)):
            print('MEASURE hvp_wgc cpu refusal batch: %s' % why)
            assert 'term wgc99_nl' in why and 'batching is what is missing' in why and 'no WGC99 stage' in why
        for make in (lambda: optimize.HipCgMultiBackend(eng, 3), lambda: optimize.density_response_multi(eng, None, 8.0, [None] * 3),
                     lambda: force_constants.force_constants(eng, np.eye(3), SPECIES, None, batch=3)):
            with pytest.raises(NotImplementedError, match='wgc99_nl.*batching is what is missing'):
                make()
    # elastic paths: the strain derivative
    why = elastic.refusal(e)
    print('MEASURE hvp_wgc cpu refusal strain: %s' % why)
    assert 'term wgc99_nl' in why and 'strain derivative of WGC99' in why
    for driver in (elastic.elastic_constants, elastic.bulk_modulus):
        for batch in (None, 3):
            with pytest.raises(NotImplementedError, match='wgc99_nl.*strain derivative of WGC99'):
                driver(e, np.eye(3), SPECIES, None, batch=batch)
    # Engine's own strain entries, before any device work (no context is touched); option off: they go to the library as before
    from professad_amd.engine import Engine
    for call in (lambda: Engine.strain_hessian(e, None), lambda: Engine.potential_strain_gradient(e, None)):
        with pytest.raises(NotImplementedError, match='Engine.*wgc99_nl.*strain derivative of WGC99'):
            call()
    assert optimize.gga_strain_refusal(_FakeEngine(WGC_LDA, {N.OPT_HVP_WGC: 0.0})) is None and optimize.gga_strain_refusal(_FakeEngine(WGC_LDA)) is None
    assert optimize.gga_strain_refusal(_FakeEngine(['tf', 'vw'], WGC_ON)) is None
    assert 'term wgc99_nl' in optimize.gga_strain_refusal(both)
    assert 'term pbe_x' in optimize.gga_strain_refusal(_FakeEngine(BENCH, GGA_ON))          # (wgc99_nl: the library's own refusal there)
    assert force_constants.batch_refusal(_FakeEngine(['ion_electron', 'tf', 'vw'], WGC_ON)) is None
