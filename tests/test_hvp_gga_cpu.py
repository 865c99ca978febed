"""Second derivatives of PBE without a device: the numpy double (tests/hvp_gga_double.py) against the reference's
double autograd (tests/golden/hvp_gga_<case>.npz, tn_gga_<case>.npz), the option's Python name, and who refuses pbe_x / pbe_c when
the option is off, on, and on the batched and elastic paths -- on fake engines, before any device work.  Every test prints its
figures as `MEASURE ...` before it asserts."""
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
import hvp_gga_cases as G  # noqa: E402
import hvp_gga_double as H  # noqa: E402
import tn_cases  # noqa: E402

# Largest max|hv - golden| / max|golden| over g16r, g17r, g18t, g16d, measured with numpy 2 / torch 2 on x86-64: numpy.fft against
# torch.fft and the order of the pointwise arithmetic are the only sources.  `pbe` stands above its two parts because the exchange
# and correlation products cancel to a fifth of either (max|hv| 1.0 .. 1.4 against 4.2 .. 6.3 on the r_s = 2 grids).
MEASURED = {'pbe_x': 7.9e-16, 'pbe_c': 1.3e-15, 'pbe': 3.9e-15, 'cfg3': 4.8e-15}
# ... and of max|H d - golden| / max|golden| and |d.H d - golden| / |golden| in chi space over g16r, g17r, g18t (cfg3): 8.9e-16 /
# 3.8e-14 / 4.3e-14 and 1.2e-16 / 8.7e-15 / 9.4e-16 -- the figures of cfg2 in test_tn_cpu.py (4.25e-14, 8.66e-15), which the
# Wang-Teter kernel at large eta sets (test_hvp_cpu.py), not PBE
MEASURED_CHI = dict(Hd=4.4e-14, dHd=8.7e-15)
FINDING = 1e-13          # a figure above this is a finding, not a number to record


@pytest.fixture(scope='module', params=G.CASES)
def case(request):
    g = np.load(os.path.join(HERE, 'golden', 'hvp_gga_%s.npz' % request.param))
    box, den, _vext = G.make_inputs(request.param)
    w = G.direction(den.shape)
    assert cases.checksum(box, den, w) == pytest.approx(float(g['checksum']), rel=1e-12)       # generator drift
    assert np.array_equal(w, g['w'])
    return request.param, g, box, den, w


@pytest.mark.parametrize('key', list(G.TERMS) + list(G.SETS))
def test_double_matches_the_reference_double_autograd(case, key):
    """hv and q of pbe_x, pbe_c, both, and cfg3.  q of the double comes from the adjoint identity
    sum f_nn w^2 + 2 f_ns w dsigma + f_ss dsigma^2 + 2 f_s |grad w|^2, the golden's from sum w hv: the identity itself is checked.
    Asserted: 10 x MEASURED per key, for hv relative to max|golden| and for q relative to |q|."""
    name, g, box, den, w = case
    assert all(v <= FINDING for v in MEASURED.values())
    names, al, be = G.SETS[key] if key in G.SETS else (G.TERMS[key], 5 / 6, 5 / 6)
    q, hv = H.hessian_vector(box, den, w, names, al, be)
    ref, qref = g['hv_' + key], float(g['q_' + key])
    dev = np.abs(hv - ref).max() / np.abs(ref).max()
    qdev = abs(sum(q.values()) - qref) / abs(qref)
    print('MEASURE hvp_gga cpu %s %s: hv %.2e  q %.2e  max|hv| %.3e' % (name, key, dev, qdev, np.abs(ref).max()))
    assert dev <= 10 * MEASURED[key]
    assert qdev <= 10 * MEASURED[key]


@pytest.mark.parametrize('name', G.TN_CASES)
def test_chi_space_double_matches_the_reference(name):
    """H d of the closure for cfg3 at phi = 1.7 sqrt(den) with the reference's own gradient g, against grad((g d).sum(), chi)"""
    g = np.load(os.path.join(HERE, 'golden', 'tn_gga_%s.npz' % name))
    box, phi, d, vext, n_elec = tn_cases.make_inputs(name)
    assert cases.checksum(box, phi, d, vext) == pytest.approx(float(g['checksum']), rel=1e-12)
    names, al, be = G.CFG3
    s, Hd = H.hessian_vector_chi(box, phi, d, g['g'], n_elec, names, al, be)
    dev = np.abs(Hd - g['Hd']).max() / np.abs(g['Hd']).max()
    qdev = abs(s['dHd'] - float(g['dHd'])) / abs(float(g['dHd']))
    print('MEASURE hvp_gga cpu chi %s: Hd %.2e  dHd %.2e' % (name, dev, qdev))
    assert all(v <= FINDING for v in MEASURED_CHI.values())
    assert dev <= 10 * MEASURED_CHI['Hd'] and qdev <= 10 * MEASURED_CHI['dHd']


def test_option_is_exported():
    header = open(os.path.join(os.path.dirname(HERE), 'include', 'ofdft_hip.h')).read()
    assert '#define OFDFT_OPT_HVP_GGA %d ' % N.OPT_HVP_GGA in header
    taken = [getattr(N, nm) for nm in dir(N) if nm.startswith('OPT_') and nm != 'OPT_HVP_GGA']
    assert N.OPT_HVP_GGA not in taken and N.OPT_HVP_GGA not in (2, 3)           # (2 and 3 are retired numbers)


class _FakeEngine:
    """what the refusals read of an engine; `gga`: None = an engine without the accessor, else the value Engine.option returns"""

    def __init__(self, names, gga=None):
        self.comm, self.dtype = None, torch.double
        mask = 0
        for nm in names:
            mask |= N.TERM_BITS[nm]
        self._terms_key = (mask, np.zeros(N.NPARAMS).tobytes())
        if gga is not None:
            self.option = lambda opt: {N.OPT_HVP_GGA: float(gga)}.get(int(opt)) if gga != 'unset' else None

    def _mask(self):
        return self._terms_key[0]


WT_PBE = ['ion_electron', 'hartree', 'tf', 'vw', 'wt_nl', 'pbe_x', 'pbe_c']
SPECIES = [(np.zeros((1, 3)), (None, None, 3))]


@pytest.mark.parametrize('gga', [None, 'unset', 0])
def test_option_off_refuses_as_before(gga):
    """no accessor (the other tests' fakes), never set, set to 0: today's message, on every path"""
    e = _FakeEngine(WT_PBE, gga)
    print('MEASURE hvp_gga cpu refusal off (%r): %s' % (gga, optimize.second_order_refusal(e)))
    assert optimize.second_order_refusal(e) == 'no second derivative of the term pbe_x'
    assert optimize.second_order_refusal(_FakeEngine(['tf', 'pbe_c'], gga)) == 'no second derivative of the term pbe_c'
    assert optimize.response_refusal(e) == 'no second derivative of the term pbe_x'
    assert force_constants.refusal(e) == elastic.refusal(e) == 'no second derivative of the term pbe_x'
    with pytest.raises(NotImplementedError, match='no second derivative of the term pbe_x$'):
        optimize.HipCgBackend(e)
    with pytest.raises(NotImplementedError, match="n_method='TN': no second derivative of the term pbe_x$"):
        optimize.optimize_density(e, 3.0, n_method='TN', volume=1.0)


def test_option_on_serves_the_single_column_paths_and_names_what_is_missing_elsewhere():
    e = _FakeEngine(WT_PBE, 1)
    assert optimize.hvp_gga_enabled(e) and not optimize.hvp_gga_enabled(_FakeEngine(WT_PBE)) and not optimize.hvp_gga_enabled(_FakeEngine(WT_PBE, 0))
    assert optimize.second_order_refusal(e) is None and optimize.response_refusal(e) is None
    assert force_constants.refusal(e) is None
    # the terms the option does not touch stay refused, in the order of the engine's own list
    assert optimize.second_order_refusal(_FakeEngine(WT_PBE + ['wgc99_nl'], 1)) == 'no second derivative of the term wgc99_nl'
    assert optimize.second_order_refusal(_FakeEngine(['tf', 'pbe_x', 'gga_k'], 1)) == 'no second derivative of the term gga_k'
    # batched paths: batching is what is missing
    for why in (optimize.second_order_refusal(e, gga_missing='batch'), force_constants.batch_refusal(e)):
        print('MEASURE hvp_gga cpu refusal batch: %s' % why)
        assert 'term pbe_x' in why and 'batching is what is missing' in why
    assert 'term pbe_c' in optimize.second_order_refusal(_FakeEngine(['tf', 'pbe_c'], 1), gga_missing='batch')
    for make in (lambda: optimize.HipCgMultiBackend(e, 3), lambda: optimize.density_response_multi(e, None, 8.0, [None] * 3),
                 lambda: force_constants.force_constants(e, np.eye(3), SPECIES, None, batch=3)):
        with pytest.raises(NotImplementedError, match='pbe_x.*batching is what is missing'):
            make()
    # elastic paths: the strain derivative of PBE
    why = elastic.refusal(e)
    print('MEASURE hvp_gga cpu refusal strain: %s' % why)
    assert 'term pbe_x' in why and 'strain derivative of PBE' in why
    for driver in (elastic.elastic_constants, elastic.bulk_modulus):
        for batch in (None, 3):
            with pytest.raises(NotImplementedError, match='pbe_x.*strain derivative of PBE'):
                driver(e, np.eye(3), SPECIES, None, batch=batch)
    # Engine's own strain entries, before any device work (no context is touched); option off: they go to the library as before
    from professad_amd.engine import Engine
    for call in (lambda: Engine.strain_hessian(e, None), lambda: Engine.potential_strain_gradient(e, None)):
        with pytest.raises(NotImplementedError, match='Engine.*pbe_x.*strain derivative of PBE'):
            call()
    assert optimize.gga_strain_refusal(_FakeEngine(WT_PBE, 0)) is None and optimize.gga_strain_refusal(_FakeEngine(WT_PBE)) is None
    assert optimize.gga_strain_refusal(_FakeEngine(['tf', 'vw'], 1)) is None
    assert force_constants.batch_refusal(_FakeEngine(['ion_electron', 'tf', 'vw'], 1)) is None


def test_engine_records_the_options_it_was_given():
    """Engine.set_option / Engine.option on an object that stands in for the context (no device)"""
    from professad_amd.engine import Engine

    class Lib:
        def ofdft_set_option(self, ctx, opt, value):
            return 0
    e = Engine.__new__(Engine)
    e.lib, e._ctx, e._options = Lib(), None, {}
    assert e.option(N.OPT_HVP_GGA) is None
    assert e.set_option(N.OPT_HVP_GGA, 1) is e and e.option(N.OPT_HVP_GGA) == 1.0 and e.option(N.OPT_PIPELINE) is None
    e.set_option(N.OPT_HVP_GGA, 0)
    assert e.option(N.OPT_HVP_GGA) == 0.0
