"""OFDFT_OPT_POT_SPECTRUM: the Hartree potential folded into the divergence spectrum of the split-derivative GGA chain
(E_H by Parseval in the divergence x pass, D_b G_b and the y-inverse of that spectrum in one y pass, one spectrum read by
the combine kernel) against the separate spectra of option 0, on the same engine inputs."""
import numpy as np
import pytest
import torch

from professad_amd import _native as N
from professad_amd import functionals as F
from professad_amd import synth
from professad_amd.engine import Engine

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
OPT_POT_SPECTRUM = 16
CFG3 = ['ion_electron', 'hartree', 'wgc99', 'pbe']
PGSLR = {'ggak_kind': 1.0, 'ggak_mu': 40 / 27, 'ggak_beta': 0.25, 'ggak_lambda': 0.4, 'ggak_sigma': 0.2}


def _inputs(shape, dtype, triclinic=False, seed=3):
    box = synth.triclinic_cell(shape[0] / 4.0) if triclinic else synth.cubic_cell(shape[0])
    den = synth.smooth_density(shape, seed=seed)
    vext = synth.random_potential(shape, seed=seed + 1)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)  # noqa: E731
    return torch.as_tensor(box), t(np.sqrt(den)), t(den), t(vext)


def _pair(shape, dtype, box, names, params=None):
    """the same context twice: the new form (default) and option 0"""
    mk = lambda v: (Engine(shape, DEV, dtype=dtype).set_cell(box).set_terms(F.NativeTerms(names).names, params)  # noqa: E731
                    .set_option(N.OPT_RESIDENT, 0).set_option(OPT_POT_SPECTRUM, v))
    return mk(1), mk(0)


def _close(Ea, mua, ga, Eb, mub, gb, rtol_e, rtol_g):
    assert set(Ea) == set(Eb)
    for k in Eb:
        assert abs(Ea[k] - Eb[k]) <= rtol_e * max(abs(Eb[k]), 1e-6), (k, Ea[k], Eb[k])
    assert abs(mua - mub) <= rtol_e * max(abs(mub), 1e-6), (mua, mub)
    err = float((ga.double() - gb.double()).abs().max()) / float(gb.double().abs().max())
    assert err <= rtol_g, err


@pytest.mark.parametrize('shape,triclinic', [((64, 64, 64), False), ((64, 64, 64), True), ((128, 128, 128), False),
                                             ((256, 256, 256), False)])
def test_cfg3_fp64_potential_spectrum_matches_separate_spectra(shape, triclinic):
    """cfg3 closure (the bench's evaluation): per-term energies and mu within 1e-13, gradient within 1e-12; the 64^3 grids
    run as hipGraph replays from the third call on.  Two y passes and at least two launches fewer."""
    box, chi, _, vext = _inputs(shape, torch.double, triclinic)
    new, old = _pair(shape, torch.double, box, CFG3)
    for rep in range(3):
        Ea, mua, ga = new.energy_grad_chi(chi, 12.0, vext)
        Eb, mub, gb = old.energy_grad_chi(chi, 12.0, vext)
        _close(Ea, mua, ga, Eb, mub, gb, 1e-13, 1e-12)
        del ga, gb          # the same gradient buffer again: the captured graph applies
    if shape[0] == 64:
        assert new.query(N.Q_GRAPH_REPLAYS) >= 1 and old.query(N.Q_GRAPH_REPLAYS) >= 1
    assert new.query(N.Q_YPASS_COUNT) == old.query(N.Q_YPASS_COUNT) - 2
    assert new.query(N.Q_LAUNCH_COUNT) < old.query(N.Q_LAUNCH_COUNT)
    new.close()
    old.close()


@pytest.mark.parametrize('shape', [(64, 64, 64), (256, 256, 256)])
def test_cfg3_fp32_potential_spectrum_matches_separate_spectra(shape):
    box, chi, _, vext = _inputs(shape, torch.float32)
    new, old = _pair(shape, torch.float32, box, CFG3)
    for rep in range(3):
        Ea, mua, ga = new.energy_grad_chi(chi, 12.0, vext)
        Eb, mub, gb = old.energy_grad_chi(chi, 12.0, vext)
        _close(Ea, mua, ga, Eb, mub, gb, 5e-6, 5e-6)
    assert new.query(N.Q_YPASS_COUNT) == old.query(N.Q_YPASS_COUNT) - 2
    new.close()
    old.close()


@pytest.mark.parametrize('shape,triclinic', [((32, 32, 32), True), ((128, 128, 128), False)])
def test_laplacian_pauli_gaussian_with_hartree_and_pbe(shape, triclinic):
    """the Laplacian-dependent Pauli-Gaussian member: (df/dL)^ is the third input of the same divergence x pass"""
    box, _, den, _ = _inputs(shape, torch.double, triclinic)
    new, old = _pair(shape, torch.double, box, ['hartree', 'vw', 'gga_k', 'pbe_x', 'pbe_c'], PGSLR)
    Ea, va = new.energy_potential(den)
    Eb, vb = old.energy_potential(den)
    for k in Eb:
        assert abs(Ea[k] - Eb[k]) <= 1e-13 * max(abs(Eb[k]), 1e-6), (k, Ea[k], Eb[k])
    assert float((va - vb).abs().max()) <= 1e-12 * float(vb.abs().max())
    assert new.query(N.Q_YPASS_COUNT) == old.query(N.Q_YPASS_COUNT) - 2
    new.close()
    old.close()


@pytest.mark.parametrize('names', [['ion_electron', 'wgc99', 'pbe'], ['ion_electron', 'hartree', 'wt', 'pz'],
                                   ['ion_electron', 'hartree', 'tf', 'vw', 'pz']])
def test_term_sets_without_hartree_or_gga_are_bitwise_unchanged(names):
    shape = (64, 64, 64)
    box, chi, _, vext = _inputs(shape, torch.double)
    new, old = _pair(shape, torch.double, box, names)
    for rep in range(3):
        Ea, mua, ga = new.energy_grad_chi(chi, 12.0, vext)
        Eb, mub, gb = old.energy_grad_chi(chi, 12.0, vext)
        assert Ea == Eb and mua == mub and torch.equal(ga, gb), rep
    assert new.query(N.Q_LAUNCH_COUNT) == old.query(N.Q_LAUNCH_COUNT)
    new.close()
    old.close()
