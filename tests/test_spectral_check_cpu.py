"""The comparison of tests/spectral_check.py is tight enough to matter: a change of one k-point (and its Hermitian partner) of an
oracle potential / closure gradient by 1e-6 (fp64 thresholds) or 1e-2 (fp32 thresholds) of its size there -- in the measure
of the check, |Vo^_k| + tau rms|Vo^| -- is rejected at every location where x-pass kernels go wrong, round-off of the
precision is accepted, and the inputs of the extent matrix carry spectral weight at all of those locations (a smooth or
32^3-tiled input would not)."""
import numpy as np
import pytest

import spectral_check as sc
import test_extent_matrix_gpu as M

SHAPE, CELL = (128, 32, 64), 'ortho'
REL = {'f64': 1e-6, 'f32': 1e-2}


@pytest.fixture(scope='module')
def oracle_fields():
    o = M.oracle(SHAPE, CELL, 'wgc99_pbe')
    return {'potential': (o['v'], o['vk']), 'closure_gradient': (o['g'], o['gk'])}


def _rejected(v, vo, p, vok):
    try:
        sc.check(v, vo, p, vok=vok)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize('p', ['f64', 'f32'])
@pytest.mark.parametrize('field', ['potential', 'closure_gradient'])
def test_single_k_point_errors_are_rejected_and_round_off_is_not(oracle_fields, field, p):
    vo, vok = oracle_fields[field]
    sc.check(vo, vo, p, vok=vok)
    # round-off of the precision at hand is accepted: fp32 storage of the oracle value, fp64 noise of a few ulp
    if p == 'f32':
        noisy = vo.astype(np.float32).astype(np.float64)
    else:
        noisy = vo + 4e-16 * np.max(np.abs(vo)) * np.random.default_rng(3).standard_normal(vo.shape)
    sc.check(noisy, vo, p, vok=vok)
    for name, k in sc.probe_points(SHAPE).items():
        bad = sc.perturb(vo, k, REL[p], sc.TAU[p], vok)
        dk = sc.spectrum(bad) - vok
        assert np.count_nonzero(np.abs(dk) > 1e-3 * np.abs(dk).max()) in (1, 2), name       # one k-point (+ its partner)
        assert _rejected(bad, vo, p, vok), (field, p, name, sc.errors(bad, vo, p, vok))


def test_probe_points_are_the_locations_they_name():
    n0, n1, n2 = SHAPE
    pts = sc.probe_points(SHAPE)
    assert pts['x_nyquist'][0] == n0 // 2
    assert pts['x_folded_half'][0] == n0 // 2 + 1
    assert pts['y_nyquist'][1] == n1 // 2
    assert pts['z_nyquist_plane'][2] == n2 // 2
    assert pts['kz0_plane_kx_upper_half'][2] == 0 and pts['kz0_plane_kx_upper_half'][0] > n0 // 2
    assert all(k % 32 for k in pts['off_the_32_tiling'])


def _shapes():
    return [(s, c) for s, c in M.MATRIX] + [((256, 256, 256), 'ortho'), ((512, 256, 128), 'tri')]


@pytest.mark.parametrize('shape,cell', _shapes(), ids=['%dx%dx%d-%s' % (s + (c,)) for s, c in _shapes()])
def test_matrix_inputs_have_spectral_weight_at_every_probe_point(shape, cell):
    den, vext, chi = M.inputs(shape, cell)
    for name, a in (('den', den), ('vext', vext), ('chi', chi)):
        ak = sc.spectrum(a)
        rms = sc.rms_amplitude(ak)
        for where, k in sc.probe_points(shape).items():
            assert abs(ak[k]) >= 0.1 * rms, (shape, cell, name, where, abs(ak[k]) / rms)
