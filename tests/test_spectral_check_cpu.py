"""The comparison of tests/spectral_check.py is tight enough to matter: a change of one k-point (and its Hermitian partner) of an
oracle potential / closure gradient by 1e-6 (fp64 thresholds) or 1e-2 (fp32 thresholds) of its size there -- in the measure
of the check, |Vo^_k| + tau rms|Vo^| -- is rejected at every location where x-pass kernels go wrong, round-off of the
precision is accepted, and the inputs of the extent matrix carry spectral weight at all of those locations (a smooth or
32^3-tiled input would not)."""
import numpy as np
import pytest

import spectral_check as sc
import test_chirpz_matrix_gpu as C
import test_extent_matrix_gpu as M
import test_slab_matrix_gpu as S
from oracle import ions as oi

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
    return ([(s, c) for s, c in M.MATRIX] + [((256, 256, 256), 'ortho'), ((512, 256, 128), 'tri')]
            + [(s, c) for s, c in C.MATRIX] + [((255, 255, 255), 'ortho')])


# chirp-z shapes with odd extents on every axis in turn (x odd / y even, n2 odd, n0 small enough that n0 // 2 + 5 wraps)
ODD = [((15, 17, 19), 'tri'), ((255, 14, 26), 'ortho'), ((10, 383, 14), 'ortho'), ((12, 10, 509), 'tri'), ((515, 6, 8), 'ortho')]


@pytest.mark.parametrize('shape', [s for s, _ in ODD] + [(53, 53, 53), (65, 30, 67), (257, 9, 20)])
def test_probe_points_on_odd_extents(shape):
    """on an odd extent the 'Nyquist' probes are the highest positive frequency ((n - 1) / 2) and the folded half starts at the
    most negative one (-(n - 1) / 2); for odd n2 the last kz plane of the half spectrum has full weight (its partner -kz is
    not stored) and is the z probe.  Every probe lies inside the half spectrum and names the location it stands for."""
    n0, n1, n2 = shape
    pts = sc.probe_points(shape)
    f0, f1 = np.fft.fftfreq(n0, 1.0 / n0), np.fft.fftfreq(n1, 1.0 / n1)
    for k in pts.values():
        assert 0 <= k[0] < n0 and 0 <= k[1] < n1 and 0 <= k[2] <= n2 // 2, (shape, pts)
    assert abs(f0[pts['x_nyquist'][0]]) == n0 // 2                   # the largest |kx| (the Nyquist index when n0 is even)
    assert f0[pts['x_folded_half'][0]] == -((n0 - 1) // 2)           # the most negative kx that is not the Nyquist index
    assert abs(f1[pts['y_nyquist'][1]]) == n1 // 2
    assert pts['z_nyquist_plane'][2] == n2 // 2 == np.fft.rfftfreq(n2).size - 1          # the last stored kz plane
    assert oi.half_weights(shape)[pts['z_nyquist_plane'][2]] == (1.0 if n2 % 2 == 0 else 2.0)
    assert pts['kz0_plane_kx_upper_half'][2] == 0 and f0[pts['kz0_plane_kx_upper_half'][0]] < 0
    assert all(k % 32 for k in pts['off_the_32_tiling'])


@pytest.mark.parametrize('shape,cell', ODD, ids=['%dx%dx%d-%s' % (s + (c,)) for s, c in ODD])
def test_single_k_point_errors_are_rejected_on_odd_extents(shape, cell):
    """perturb on odd extents: a probe is its own Hermitian partner only at k = 0 along an odd axis, so every probe here gets
    one partner (kz = 0 plane) or none (kz > 0: the partner is not in the half spectrum, irfftn supplies it) and the change
    reaches the full spectrum unscaled; the check rejects it at both precisions and accepts round-off"""
    o = M.oracle(shape, cell, 'wgc99_pbe')
    for vo, vok in ((o['v'], o['vk']), (o['g'], o['gk'])):
        for p in ('f64', 'f32'):
            noisy = vo.astype(np.float32).astype(np.float64) if p == 'f32' else vo * (1 + 4e-16)
            sc.check(noisy, vo, p, vok=vok)
            for name, k in sc.probe_points(shape).items():
                bad = sc.perturb(vo, k, REL[p], sc.TAU[p], vok)
                dk = sc.spectrum(bad) - vok
                big = np.abs(dk) > 1e-3 * np.abs(dk).max()
                partner = ((-k[0]) % shape[0], (-k[1]) % shape[1], k[2])
                assert big[k] and np.count_nonzero(big) == (2 if k[2] == 0 or 2 * k[2] == shape[2] else 1), (name, k)
                if k[2] == 0:
                    assert big[partner] and np.isclose(dk[partner], np.conj(dk[k]))
                # the measured per-k error is the requested one: the change is neither halved by symmetrisation nor doubled
                got = sc.kspace_error(bad, vo, sc.TAU[p], vok)
                assert abs(got - REL[p]) <= 1e-3 * REL[p], (shape, name, p, got)
                assert _rejected(bad, vo, p, vok), (shape, name, p, sc.errors(bad, vo, p, vok))


def slab_boundary_points(shape, P):
    """{name: (kx, ky, kz)} of the k-points where the exchange layout of P slab ranks changes record (engine_ctx.h: XchgGeom):
    the first and the last x plane of a rank's slab, the first y line of a rank's slab -- each once in a remainder kz plane
    (kz >= nzm = 8 (nzc / 8)) and once in the last full 8-plane block -- and both kz locations at a (kx, ky) inside a slab.
    Without remainder planes (nzc a multiple of 8) the last plane of the last block stands in."""
    n0, n1, n2 = shape
    nxl, nyl, nzc = n0 // P, n1 // P, n2 // 2 + 1
    nzm = nzc // 8 * 8
    kz_rem = nzm + 1 if nzc - nzm > 1 else nzc - 1          # (one remainder plane: it is the Nyquist plane)
    kz_blk = nzm - 3
    inner = (n0 // 2 + nxl // 2) % n0, nyl // 2          # inside a slab wherever a slab has an inside (nxl >= 3, nyl >= 2)
    pts = {'kz_remainder_plane': (inner[0], inner[1], kz_rem), 'kz_last_full_block': (inner[0], inner[1], kz_blk)}
    for r in range(1, P):
        kz = (kz_rem, kz_blk) if r % 2 else (kz_blk, kz_rem)
        pts['kx_first_plane_of_rank_%d' % r] = (r * nxl, inner[1], kz[0])
        pts['kx_last_plane_of_rank_%d' % (r - 1)] = (r * nxl - 1, inner[1], kz[1])
        pts['ky_first_line_of_rank_%d' % r] = (inner[0], r * nyl, kz[0])
    return pts


@pytest.mark.parametrize('shape,P,cell', S.GEOMETRIES + [g[:3] for g in S.CHUNKED], ids=[S._gid(g) for g in S.GEOMETRIES + S.CHUNKED])
def test_single_k_point_errors_on_slab_boundaries_are_rejected(shape, P, cell):
    """what shows that the rows of tests/test_slab_matrix_gpu.py can fail: a single-k-point error at a slab boundary of its
    geometries is rejected at the sizes of the sensitivity test above (1e-6 with the fp64 bounds, 1e-2 with the fp32 ones), and
    accepted at a tenth of what the bounds admit there.  (Not at a tenth of the rejected size: with the fp64 bounds 1e-7 is
    still a hundred times the per-k bound of 1e-9; and on the smallest grids here, 2048 and 4096 points, one k-point is so
    large a share of the field that the real-space bound is the tighter of the two.)"""
    n0, n1, n2 = shape
    nzc = n2 // 2 + 1
    pts = slab_boundary_points(shape, P)
    assert len(pts) == 3 * (P - 1) + 2
    for name, k in pts.items():
        assert 0 <= k[0] < n0 and 0 <= k[1] < n1 and 0 < k[2] < nzc, (name, k)
    assert all(k[0] % (n0 // P) == 0 for nm, k in pts.items() if nm.startswith('kx_first'))
    assert all((k[0] + 1) % (n0 // P) == 0 for nm, k in pts.items() if nm.startswith('kx_last'))
    assert all(k[1] % (n1 // P) == 0 and k[1] for nm, k in pts.items() if nm.startswith('ky_first'))
    nzm = nzc // 8 * 8
    assert pts['kz_last_full_block'][2] // 8 == nzm // 8 - 1
    assert pts['kz_remainder_plane'][2] >= nzm or nzc == nzm
    o = M.oracle(shape, cell, 'vwgtf1_h')
    try:
        for vo, vok in ((o['v'], o['vk']), (o['g'], o['gk'])):
            for p in ('f64', 'f32'):
                for name, k in pts.items():
                    bad = sc.perturb(vo, k, REL[p], sc.TAU[p], vok)
                    assert _rejected(bad, vo, p, vok), (shape, P, name, k, p, sc.errors(bad, vo, p, vok))
                    # the errors are linear in the size of the change: a tenth of what the tighter criterion admits is accepted
                    ev, ek = sc.errors(bad, vo, p, vok)
                    assert abs(ek - REL[p]) <= 1e-3 * REL[p], (shape, P, name, p, ek)
                    ok = 0.1 * REL[p] * min(sc.V_TOL[p] / ev, sc.K_TOL[p] / ek)
                    sc.check(sc.perturb(vo, k, ok, sc.TAU[p], vok), vo, p, vok=vok)
    finally:
        M._ORACLE.pop((shape, cell, 'vwgtf1_h'), None)


@pytest.mark.parametrize('shape,cell', _shapes(), ids=['%dx%dx%d-%s' % (s + (c,)) for s, c in _shapes()])
def test_matrix_inputs_have_spectral_weight_at_every_probe_point(shape, cell):
    den, vext, chi = M.inputs(shape, cell)
    for name, a in (('den', den), ('vext', vext), ('chi', chi)):
        ak = sc.spectrum(a)
        rms = sc.rms_amplitude(ak)
        for where, k in sc.probe_points(shape).items():
            assert abs(ak[k]) >= 0.1 * rms, (shape, cell, name, where, abs(ak[k]) / rms)
