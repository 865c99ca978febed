"""OFDFT_OPT_AXIS_PASSES: one-axis operators as one-axis passes of the z-fused pipeline on one GPU.
Bit 1: D_a n of the split-derivative GGA chain from an x pass on the z spectrum (no y round trip: one y pass less, every cell).
Bit 2: the von Weizsaecker Laplacian on cells with orthogonal axes as one x pass with -(k_a^2 + k_c^2) plus one y pass with
-k_b^2 between its transforms that adds the x pass' result (two y passes and a launch less; fp64 library only).
Option 3 (default) against option 0 -- the sequence without either -- on the same engine inputs, tolerances of
test_potential_spectrum_gpu.py (both routes are the same transforms with the multiplies regrouped: fp64 1e-13 on the energies and
mu, 1e-12 of the max-norm on the gradient; fp32 5e-6)."""
import numpy as np
import pytest
import torch

from professad_amd import _native as N
from professad_amd import functionals as F
from professad_amd import synth
from professad_amd.engine import Engine

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CFG3 = ['ion_electron', 'hartree', 'wgc99', 'pbe']
PGSLR = {'ggak_kind': 1.0, 'ggak_mu': 40 / 27, 'ggak_beta': 0.25, 'ggak_lambda': 0.4, 'ggak_sigma': 0.2}


def _box(shape, cell):
    if cell == 'tri':
        return synth.triclinic_cell(shape[0] / 4.0)
    if cell == 'cubic':
        return synth.cubic_cell(shape[0])
    # orthorhombic with three different grid spacings AND three different edges: a swapped k_a, k_b or k_c cannot cancel
    return np.diag([0.25 * shape[0], 0.31 * shape[1], 0.22 * shape[2]])


def _inputs(shape, dtype, cell, seed=3, rough=False):
    den = synth.random_density(shape, seed=seed) if rough else synth.smooth_density(shape, seed=seed)
    vext = synth.random_potential(shape, seed=seed + 1)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)  # noqa: E731
    return torch.as_tensor(_box(shape, cell)), t(np.sqrt(den)), t(den), t(vext)


def _pair(shape, dtype, box, names, params=None, values=(3, 0), extra=()):
    """the same context twice: OFDFT_OPT_AXIS_PASSES = values[0] and values[1]"""
    def mk(v):
        e = Engine(shape, DEV, dtype=dtype).set_cell(box).set_terms(F.NativeTerms(names).names, params)
        e.set_option(N.OPT_RESIDENT, 0)
        for opt, val in extra:
            e.set_option(opt, val)
        return e.set_option(N.OPT_AXIS_PASSES, v)
    return mk(values[0]), mk(values[1])


def _close(Ea, mua, ga, Eb, mub, gb, rtol_e, rtol_g):
    assert set(Ea) == set(Eb)
    err_e = max(abs(Ea[k] - Eb[k]) / max(abs(Eb[k]), 1e-6) for k in Eb)
    err_mu = abs(mua - mub) / max(abs(mub), 1e-6)
    err_g = float((ga.double() - gb.double()).abs().max()) / float(gb.double().abs().max())
    print('max rel dE %.3e  dmu %.3e  dgrad %.3e' % (err_e, err_mu, err_g))
    for k in Eb:
        assert abs(Ea[k] - Eb[k]) <= rtol_e * max(abs(Eb[k]), 1e-6), (k, Ea[k], Eb[k])
    assert err_mu <= rtol_e, (mua, mub)
    assert err_g <= rtol_g, err_g


def _closure_pair(new, old, chi, vext, rtol_e, rtol_g, dy, dl, graph):
    """dy / dl: y passes / launches the first engine saves"""
    for rep in range(3):          # (grids of <= 2^19 points replay a hipGraph from the third call on)
        Ea, mua, ga = new.energy_grad_chi(chi, 12.0, vext)
        Eb, mub, gb = old.energy_grad_chi(chi, 12.0, vext)
        _close(Ea, mua, ga, Eb, mub, gb, rtol_e, rtol_g)
        del ga, gb                # the same gradient buffer again: the captured graph applies
    if graph:
        assert new.query(N.Q_GRAPH_REPLAYS) >= 1 and old.query(N.Q_GRAPH_REPLAYS) >= 1
    assert new.query(N.Q_YPASS_COUNT) == old.query(N.Q_YPASS_COUNT) - dy
    assert new.query(N.Q_FFT_COUNT) == old.query(N.Q_FFT_COUNT)
    assert new.query(N.Q_LAUNCH_COUNT) == old.query(N.Q_LAUNCH_COUNT) - dl
    new.close()
    old.close()


# launches: the Laplacian's three become two; D_a n saves its y-inverse, and in the potential-spectrum form (extents the
# energy-integrating x pass serves: powers of two up to 512) stage 2 has no density pass left, else one with an output less
# x-pass kernel family of the two moved passes (both 1 -> 1): group-parallel below 256-point lines by default, cross-wave at 256;
# OFDFT_OPT_XWAVE 2 / 5 put the wave-local / the cross-wave kernel under the same shapes.  48 x 96 x 120: mixed-radix plans (the y
# kernel re-patterns its registers between the two transforms); 32^3 with the full-spectrum density: every Nyquist plane carries weight
@pytest.mark.parametrize('shape,cell,xwave,rough,dy,dl', [
    ((32, 32, 32), 'tri', 1, False, 1, 1),
    ((64, 64, 64), 'cubic', 1, False, 3, 2),
    ((64, 64, 64), 'cubic', 2, False, 3, 2),
    ((128, 64, 32), 'ortho', 1, False, 3, 2),
    ((128, 64, 32), 'ortho', 5, False, 3, 2),
    ((256, 32, 32), 'ortho', 1, False, 3, 2),
    ((48, 96, 120), 'ortho', 1, False, 3, 1),
    ((32, 32, 32), 'cubic', 1, True, 3, 2),
])
def test_cfg3_fp64_axis_passes_match_the_y_round_trips(shape, cell, xwave, rough, dy, dl):
    """cfg3 closure (the bench's evaluation): triclinic cells lose one y pass (D_a n), cells with orthogonal axes three"""
    box, chi, _, vext = _inputs(shape, torch.double, cell, rough=rough)
    new, old = _pair(shape, torch.double, box, CFG3, extra=((N.OPT_XWAVE, xwave),))
    _closure_pair(new, old, chi, vext, 1e-13, 1e-12, dy, dl, graph=shape[0] * shape[1] * shape[2] <= 1 << 19)


def test_cfg3_fp32_axis_passes_match_the_y_round_trips():
    """fp32 at 64^3, option 3 against option 0, 5e-6 on energies, mu and the gradient.  The fp32 library serves bit 1 only (one y
    pass and one launch less): there the two-pass Laplacian measured 1.0 % slower per evaluation than the three-pass one in every
    alternation at 256^3, and, -k^2 weighing the fp32 transforms' rounding with k_max^2, either grouping of its multiplies is
    ~2e-5 of the gradient's max-norm from the other (measured 1.68e-5 here while the library still served bit 2, against 1.8e-7
    for bit 1), so the two could not have met this bound"""
    shape = (64, 64, 64)
    box, chi, _, vext = _inputs(shape, torch.float32, 'cubic')
    new, old = _pair(shape, torch.float32, box, CFG3)
    _closure_pair(new, old, chi, vext, 5e-6, 5e-6, 1, 1, graph=True)


def test_fp32_library_accepts_bit_2_and_keeps_the_three_pass_laplacian():
    """option 3 and option 1 enqueue the same sequence in the fp32 library: bitwise equal, equal counts"""
    shape = (64, 64, 64)
    box, chi, _, vext = _inputs(shape, torch.float32, 'cubic')
    new, old = _pair(shape, torch.float32, box, CFG3, values=(3, 1))
    Ea, mua, ga = new.energy_grad_chi(chi, 12.0, vext)
    Eb, mub, gb = old.energy_grad_chi(chi, 12.0, vext)
    assert Ea == Eb and mua == mub and torch.equal(ga, gb)
    assert new.query(N.Q_LAUNCH_COUNT) == old.query(N.Q_LAUNCH_COUNT) and new.query(N.Q_YPASS_COUNT) == old.query(N.Q_YPASS_COUNT)
    new.close()
    old.close()


@pytest.mark.parametrize('shape,cell', [((64, 64, 64), 'cubic'), ((128, 64, 32), 'ortho')])
def test_cfg3_fp32_axis_passes_against_the_fp64_engine(shape, cell):
    """the fp32 build with the new sequence against the fp64 engine with the old one, at the bounds the suite holds the fp32 build
    to everywhere (energies 5e-6, gradient 5e-4 of its max-norm: the smoke run's)"""
    box, chi, _, vext = _inputs(shape, torch.double, cell)
    e32, e64 = _pair(shape, torch.float32, box, CFG3)
    e64.close()
    e64 = Engine(shape, DEV).set_cell(box).set_terms(F.NativeTerms(CFG3).names).set_option(N.OPT_RESIDENT, 0).set_option(N.OPT_AXIS_PASSES, 0)
    Ea, mua, ga = e32.energy_grad_chi(chi.float(), 12.0, vext.float())
    Eb, mub, gb = e64.energy_grad_chi(chi, 12.0, vext)
    _close(Ea, mua, ga, Eb, mub, gb, 5e-6, 5e-4)
    e32.close()
    e64.close()


def test_separate_spectra_form_keeps_its_hartree_pass():
    """OFDFT_OPT_POT_SPECTRUM 0: the density x pass is left with the Hartree potential alone; still three y passes less"""
    shape = (64, 64, 64)
    box, chi, _, vext = _inputs(shape, torch.double, 'cubic')
    new, old = _pair(shape, torch.double, box, CFG3, extra=((N.OPT_POT_SPECTRUM, 0),))
    _closure_pair(new, old, chi, vext, 1e-13, 1e-12, 3, 1, graph=True)


@pytest.mark.parametrize('shape,cell', [((32, 32, 32), 'tri'), ((64, 64, 64), 'cubic')])
@pytest.mark.parametrize('pspec', [1, 0])
def test_laplacian_pauli_gaussian_keeps_lap_n_in_the_density_pass(shape, cell, pspec):
    """the Laplacian-dependent Pauli-Gaussian member: -k^2 n^ still comes from the y-forwarded spectrum (it depends on all three
    axes), D_a n no longer does"""
    box, _, den, _ = _inputs(shape, torch.double, cell)
    new, old = _pair(shape, torch.double, box, ['hartree', 'vw', 'gga_k', 'pbe_x', 'pbe_c'], PGSLR, extra=((N.OPT_POT_SPECTRUM, pspec),))
    Ea, va = new.energy_potential(den)
    Eb, vb = old.energy_potential(den)
    err_v = float((va - vb).abs().max()) / float(vb.abs().max())
    print('max rel dE %.3e  dv %.3e' % (max(abs(Ea[k] - Eb[k]) / max(abs(Eb[k]), 1e-6) for k in Eb), err_v))
    for k in Eb:
        assert abs(Ea[k] - Eb[k]) <= 1e-13 * max(abs(Eb[k]), 1e-6), (k, Ea[k], Eb[k])
    assert err_v <= 1e-12
    assert new.query(N.Q_YPASS_COUNT) == old.query(N.Q_YPASS_COUNT) - (1 if cell == 'tri' else 3)
    assert new.query(N.Q_FFT_COUNT) == old.query(N.Q_FFT_COUNT)
    new.close()
    old.close()


def _bitwise(names, cell, shape, values=(3, 0)):
    box, chi, _, vext = _inputs(shape, torch.double, cell)
    new, old = _pair(shape, torch.double, box, names, values=values)
    for rep in range(3):
        Ea, mua, ga = new.energy_grad_chi(chi, 12.0, vext)
        Eb, mub, gb = old.energy_grad_chi(chi, 12.0, vext)
        assert Ea == Eb and mua == mub and torch.equal(ga, gb), rep
    assert new.query(N.Q_LAUNCH_COUNT) == old.query(N.Q_LAUNCH_COUNT)
    assert new.query(N.Q_YPASS_COUNT) == old.query(N.Q_YPASS_COUNT)
    new.close()
    old.close()


def test_wang_teter_set_is_untouched_by_bit_1_and_differs_by_the_laplacian_only():
    """['ion_electron', 'hartree', 'wt', 'pz'] at 64^3 cubic.  'wt' expands to tf + vw + wt_nl (NativeTerms), so the set HAS the von
    Weizsaecker Laplacian and bit 2 applies to it as to tf + vw + pz below: it cannot be bitwise equal under option 3.  What holds bitwise, with equal launch counts, is bit 1 -- there is no GGA chain; option 3
    differs from option 0 by the Laplacian's two y passes and one launch, within the fp64 bounds."""
    names, shape = ['ion_electron', 'hartree', 'wt', 'pz'], (64, 64, 64)
    _bitwise(names, 'cubic', shape, values=(1, 0))
    box, chi, _, vext = _inputs(shape, torch.double, 'cubic')
    new, old = _pair(shape, torch.double, box, names)
    _closure_pair(new, old, chi, vext, 1e-13, 1e-12, 2, 1, graph=True)


def test_term_set_without_gradient_or_laplacian_is_bitwise_unchanged():
    _bitwise(['ion_electron', 'hartree', 'tf', 'pz'], 'cubic', (64, 64, 64))


def test_von_weizsaecker_without_gga_differs_by_the_laplacian_only():
    shape = (64, 64, 64)
    box, chi, _, vext = _inputs(shape, torch.double, 'cubic')
    new, old = _pair(shape, torch.double, box, ['ion_electron', 'hartree', 'tf', 'vw', 'pz'])
    _closure_pair(new, old, chi, vext, 1e-13, 1e-12, 2, 1, graph=True)


def test_triclinic_cell_without_gga_is_bitwise_unchanged():
    """neither part applies: no split GGA chain, axes not orthogonal"""
    _bitwise(['ion_electron', 'hartree', 'tf', 'vw', 'pz'], 'tri', (32, 32, 32))


@pytest.mark.parametrize('value,dy', [(1, 1), (2, 2)])
def test_each_bit_alone(value, dy):
    shape = (64, 64, 64)
    box, chi, _, vext = _inputs(shape, torch.double, 'cubic')
    new, old = _pair(shape, torch.double, box, CFG3, values=(value, 0))
    _closure_pair(new, old, chi, vext, 1e-13, 1e-12, dy, 1, graph=True)


def test_option_value_is_checked():
    eng = Engine((32, 32, 32), DEV).set_cell(torch.as_tensor(synth.cubic_cell(32)))
    with pytest.raises(Exception):
        eng.set_option(N.OPT_AXIS_PASSES, 4)
    eng.close()
