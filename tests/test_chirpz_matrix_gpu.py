"""The chirp-z (Bluestein) path -- the extents without a line-transform plan, i.e. every grid the reference's System.ecut2shape
(system.py:74-89) gives, since its extents are odd -- against the fp64 oracle (oracle/closed_form.py) on full-spectrum inputs
(tests/spectral_check.py), in real space and per k-point, for every term set of the extent matrix (tests/test_extent_matrix_gpu.py:
TERM_SETS reaches every mix functor), both builds, OFDFT_OPT_BS_FUSED 1 and 0.

What runs (lines.hip, engine.hip: the unfused pipeline):
  * OFDFT_OPT_BS_FUSED 1 and every extent <= 256 along x (padded length M <= 512): bluestein_xmix_kernel -- forward-x, the mix and
    inverse-x in one kernel -- for MixScale HARTREE / LAPLACE / LINDHARD, MixDensity<false, true>, MixDensity<true, true>, MixDiv
    and MixWgc; the Laplacian-dependent GGA members (pgslr_h, pgsl025) keep the three-pass form.  Both padded lengths of y and z
    equal and <= 128: the fused z + y kernel (bluestein_zy_kernel), else separate z and y passes.
  * OFDFT_OPT_BS_FUSED 0, or x > 256: the three-pass form (chirp-z line passes, padded lengths up to 1024, and the spectral
    kernels between them).
  * an extent > 512, or OFDFT_OPT_BLUESTEIN 0: the plain O(N^2) DFT kernels for the whole grid.
ofdft_query(OFDFT_Q_XPASS_KINDS) is exactly XPASS_CHIRPZ where bluestein_xmix_ok holds and the GGA has no Laplacian
(engine.hip: xm), 0 elsewhere; OFDFT_Q_FAST_PATH is 0 throughout.

OFDFT_OPT_GGA_SPLIT does not change what runs on this path: the unfused pipeline always builds the three Cartesian gradient
components (engine.hip, phase B / D).  The matrix therefore runs the default only, and every case with a GGA checks that
OFDFT_OPT_GGA_SPLIT 0 gives the same launch count (OFDFT_Q_LAUNCH_COUNT) and a bitwise equal potential.

Bounds: those of the extent matrix (tests/spectral_check.py, where the maxima measured here are recorded).
"""
import time

import numpy as np
import pytest
import torch

import spectral_check as sc
import test_extent_matrix_gpu as M
from professad_amd import _native as N
from professad_amd.engine import Engine

pytestmark = pytest.mark.gpu
DEV = M.DEV
GGA = {'wgc99_pbe', 'wgc98_lkt_pbe', 'perrot_pg1_pz', 'sm_pgs_chach', 'pgslr_h', 'pgsl025'}

# (shape, cell): why each is here
MATRIX = [
    ((15, 17, 19), 'tri'),      # fused z + y at M = 64, x at M = 32; odd row count (the z rows go in pairs)
    ((27, 35, 33), 'tri'),      # the anchor shape of tests/test_gpu_parity.py, fused z + y at M = 128
    ((53, 53, 53), 'ortho'),    # the reference's own small case (its 20-bohr box)
    ((64, 53, 32), 'ortho'),    # power-of-two lines on a grid without a plan
    ((65, 30, 67), 'ortho'),    # M1 != M2 (separate z and y passes), even n1 without a plan, x at M = 256
    ((129, 22, 45), 'tri'),     # xmix at M = 512
    ((255, 14, 26), 'ortho'),   # xmix at the largest x it serves; even n2 (kz Nyquist plane); nzc = 14 (remainder planes)
    ((257, 9, 20), 'tri'),      # x > 256: the three-pass form, a generic pass at M = 1024
    ((10, 383, 14), 'ortho'),   # y pass at M = 1024
    ((12, 10, 509), 'tri'),     # z r2c / c2r at M = 1024, odd n2
    ((515, 6, 8), 'ortho'),     # an extent > 512: the plain DFT kernels for the whole grid
]
# shapes also run with OFDFT_OPT_BLUESTEIN 0 (the plain DFT kernels at extents the chirp-z path would serve)
PLAIN_DFT = [((15, 17, 19), 'tri'), ((65, 30, 67), 'ortho'), ((257, 9, 20), 'tri')]


def expected_kinds(shape, ts, bs_fused, bluestein=1):
    """OFDFT_Q_XPASS_KINDS of an evaluation: bluestein_xmix_ok (bs_fused, every extent <= 512, x <= 256) and no Laplacian GGA"""
    xm = bs_fused and bluestein and max(shape) <= 512 and shape[0] <= 256 and ts not in M.LAPLACIAN_GGA
    return N.XPASS_CHIRPZ if xm else 0


def measure(o, p, E, v, Ec, mu, g):
    """errors of one energy_potential (E, v) and one closure (Ec, mu, g) against the oracle o, in the measures of spectral_check"""
    ev, ek = sc.errors(v.cpu().numpy() if torch.is_tensor(v) else v, o['v'], p, o['vk'])
    gv, gk = sc.errors(g.cpu().numpy(), o['g'], p, o['gk'])
    return dict(err_E=abs(sum(E.values()) - o['E']) / max(1.0, abs(o['E'])), err_v=ev, err_vk=ek,
                err_Ec=abs(sum(Ec.values()) - o['Ec']) / max(1.0, abs(o['Ec'])), err_g=gv, err_gk=gk,
                err_mu=abs(mu - o['mu']) / max(1.0, abs(o['mu'])))


def over_bounds(rec, p):
    """[(error name, value, bound)] of the errors of `rec` above the bounds of precision p (spectral_check: the extent matrix's
    bounds hold on this path too)"""
    bounds = (('err_E', sc.E_TOL), ('err_Ec', sc.E_TOL), ('err_v', sc.V_TOL), ('err_g', sc.V_TOL), ('err_vk', sc.K_TOL),
              ('err_gk', sc.K_TOL), ('err_mu', sc.MU_TOL))
    return [(key, rec[key], b[p]) for key, b in bounds if not rec[key] <= b[p]]


def run_case(shape, cell, ts, fused=(1, 0), dtypes=('f64', 'f32'), bluestein=1):
    """every (dtype, OFDFT_OPT_BS_FUSED) of one (shape, cell, term set) against the oracle; every error is recorded before the
    first assertion so that one report covers the whole case -> {(dtype, bs_fused): kinds}"""
    o = M.oracle(shape, cell, ts)
    names, params, _ = M.TERM_SETS[ts]
    seen, bad = {}, []
    for p in dtypes:
        dt = M.DTYPES[p]
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=DEV)  # noqa: E731
        den, vext, chi = t(o['den']), t(o['vext']), t(o['chi'])
        eng = Engine(shape, DEV, dtype=dt).set_cell(torch.as_tensor(o['box'])).set_terms(names, params)
        eng.set_option(N.OPT_GRAPH, 0).set_option(N.OPT_RESIDENT, 0).set_option(N.OPT_BLUESTEIN, bluestein)
        assert int(eng.query(N.Q_FAST_PATH)) == 0, shape
        for bs in fused:
            eng.set_option(N.OPT_BS_FUSED, bs)
            what = (shape, cell, ts, p, 'bs_fused=%d' % bs, 'bluestein=%d' % bluestein)
            want = expected_kinds(shape, ts, bs, bluestein)
            E, v = eng.energy_potential(den, vext)
            k1 = int(eng.query(N.Q_XPASS_KINDS))
            v = v.cpu().numpy()
            if ts in GGA:          # OFDFT_OPT_GGA_SPLIT changes nothing on this path (module docstring)
                eng.set_option(N.OPT_GGA_SPLIT, 0)
                E0, v0 = eng.energy_potential(den, vext)
                n0 = int(eng.query(N.Q_LAUNCH_COUNT))
                eng.set_option(N.OPT_GGA_SPLIT, 1)
                # (against a repeat: the first call also builds tables, e.g. WGC99's, which adds launches)
                eng.energy_potential(den, vext)
                n1 = int(eng.query(N.Q_LAUNCH_COUNT))
                assert n0 == n1 and np.array_equal(v0.cpu().numpy(), v) and E0 == E, (what, n0, n1)
            Ec, mu, g = eng.energy_grad_chi(chi, o['n_elec'], vext)
            k2 = int(eng.query(N.Q_XPASS_KINDS))
            rec = measure(o, p, E, v, Ec, mu, g)
            M._record(shape=shape, cell=cell, ts=ts, dtype=p, bs_fused=bs, bluestein=bluestein, kinds=[k1, k2], **rec)
            seen[(p, bs)] = k1 | k2
            if (k1, k2) != (want, want):
                bad.append((what, 'kinds', k1, k2, want))
            bad += [what + b for b in over_bounds(rec, p)]
        eng.close()
    assert not bad, bad
    return seen


@pytest.mark.parametrize('ts', list(M.TERM_SETS))
@pytest.mark.parametrize('shape,cell', MATRIX, ids=['%dx%dx%d-%s' % (s + (c,)) for s, c in MATRIX])
def test_chirpz_path_matches_the_oracle(shape, cell, ts):
    t0 = time.time()
    seen = run_case(shape, cell, ts)
    if shape[0] <= 256 and max(shape) <= 512 and ts not in M.LAPLACIAN_GGA:
        assert seen[('f64', 1)] == seen[('f32', 1)] == N.XPASS_CHIRPZ, seen        # the fused chirp-z x pass ran
    M._record(shape=shape, cell=cell, ts=ts, seconds=time.time() - t0)


@pytest.mark.parametrize('ts', ['wgc99_pbe', 'wgc98_lkt_pbe', 'pgslr_h', 'vwgtf1_h', 'wts_exp'])
@pytest.mark.parametrize('shape,cell', PLAIN_DFT, ids=['%dx%dx%d-%s' % (s + (c,)) for s, c in PLAIN_DFT])
def test_plain_dft_kernels_match_the_oracle(shape, cell, ts):
    """OFDFT_OPT_BLUESTEIN 0: the same grids on the O(N^2) DFT kernels (no fused x pass)"""
    t0 = time.time()
    seen = run_case(shape, cell, ts, fused=(1,), bluestein=0)
    assert not any(seen.values()), seen
    M._record(shape=shape, cell=cell, ts=ts, bluestein=0, seconds=time.time() - t0)


def test_full_size_odd_grid_without_tiling_matches_the_oracle():
    """255^3 (the largest x the fused chirp-z x pass serves, M = 512 on every axis) on a full-spectrum input, default options
    (graph capture and the resident kernel as they come), both builds"""
    shape, cell, ts = (255, 255, 255), 'ortho', 'wgc98_lkt_pbe'
    t0 = time.time()
    o = M.oracle(shape, cell, ts)
    names, params, _ = M.TERM_SETS[ts]
    bad = []
    for p in ('f64', 'f32'):
        dt = M.DTYPES[p]
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=DEV)  # noqa: E731
        den, vext, chi = t(o['den']), t(o['vext']), t(o['chi'])
        eng = Engine(shape, DEV, dtype=dt).set_cell(torch.as_tensor(o['box'])).set_terms(names, params)
        E, v = eng.energy_potential(den, vext)
        k1 = int(eng.query(N.Q_XPASS_KINDS))
        for _ in range(2):             # the second closure call may replay a captured graph
            Ec, mu, g = eng.energy_grad_chi(chi, o['n_elec'], vext)
        k2 = int(eng.query(N.Q_XPASS_KINDS))
        rec = measure(o, p, E, v, Ec, mu, g)
        eng.close()
        M._record(shape=shape, cell=cell, ts=ts, dtype=p, kinds=[k1, k2], **rec)
        if (k1, k2) != (N.XPASS_CHIRPZ, N.XPASS_CHIRPZ):
            bad.append((p, 'kinds', k1, k2))
        bad += [(p,) + b for b in over_bounds(rec, p)]
    M._ORACLE.pop((shape, cell, ts), None)
    M._record(shape=shape, cell=cell, ts=ts, seconds=time.time() - t0)
    assert not bad, bad
