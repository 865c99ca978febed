"""The fused x-pass kernels at the line lengths they are instantiated for (128, 256, 512, 1024, mixed-radix 480), the fused z
kernels at rows of 256 / 512 / 1024 / 480 points, and both builds -- each run against the fp64 oracle (oracle/closed_form.py)
on inputs whose spectrum is full (tests/spectral_check.py), in real space and per k-point.

Every x-pass kernel family is compared with the oracle on its own (OFDFT_OPT_XWAVE 1 default, 0 group-parallel, 2 wave-local,
5 cross-wave wherever it exists), with the split and the three-component GGA chain (OFDFT_OPT_GGA_SPLIT 1 / 0), and
ofdft_query(OFDFT_Q_XPASS_KINDS) tells which family ran.  Which term set reaches which mix functor (xpass_a.hip, xpass_b.hip):

  wgc99_pbe      MixWgc (MixWgcFold on orthogonal cells), MixDensityA<true, false> / MixDensity<true, true>, MixDerivA / MixDiv,
                 MixScale<SPEC_LAPLACE>
  wgc98_lkt_pbe  MixScale<SPEC_LINDHARD> (two spectra: alpha != beta), the same density / divergence mixes with the LKT kinetic GGA
  perrot_pg1_pz  MixScale<SPEC_LINDHARD> (alpha = beta = 1), PG1 through the density / divergence mixes with Hartree
  sm_pgs_chach   MixDensityA<false, false> / MixDensity<false, true> (GGA without Hartree), MixScale<SPEC_LINDHARD> (alpha = beta = 1/2)
  pgslr_h        MixDensityA<true, true>, MixDerivAL (split chain only: the three-component form of a Laplacian-dependent GGA
                 is the unfused pipeline, no fused x pass)
  pgsl025        MixDensityA<false, true>, MixDerivAL
  vwgtf1_h       MixDensity<true, false> (Hartree, no GGA), MixScale<SPEC_LAPLACE>
  vwgtf2_pw      MixScale<SPEC_LAPLACE> alone, PW92
  wts_exp        MixScale<SPEC_LINDHARD> (Wang-Teter, one spectrum), the two-pass stabilised combine
"""
import json
import math
import os
import time

import numpy as np
import pytest
import torch

import spectral_check as sc
from oracle import closed_form as cf
from professad_amd import _native as N
from professad_amd import synth
from professad_amd.engine import Engine

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = {'f64': torch.double, 'f32': torch.float32}
S5 = math.sqrt(5.0)
WGC98 = {'wt_alpha': (5 + S5) / 6, 'wt_beta': (5 - S5) / 6}
PGS = {'ggak_kind': 1.0, 'ggak_mu': 40 / 27}

# name: (engine terms, engine params, oracle pieces).  A piece is a method of oracle.closed_form.Evaluator with its extra
# arguments, or ('term', name) for Evaluator.term (the composite reference functionals, vW included where they carry it)
TERM_SETS = {
    'wgc99_pbe': (['ion_electron', 'hartree', 'tf', 'vw', 'wgc99_nl', 'pbe_x', 'pbe_c'], {},
                  [('ion_electron',), ('hartree',), ('term', 'wgc99'), ('pbe',)]),
    'wgc98_lkt_pbe': (['ion_electron', 'hartree', 'tf', 'vw', 'wt_nl', 'gga_k', 'pbe_x', 'pbe_c'], dict(WGC98, ggak_kind=0.0),
                      [('ion_electron',), ('hartree',), ('term', 'wgc98'), ('ggak', 'lkt'), ('pbe',)]),
    'perrot_pg1_pz': (['hartree', 'tf', 'vw', 'wt_nl', 'gga_k', 'lda_x', 'pz_c'],
                      {'wt_alpha': 1.0, 'wt_beta': 1.0, 'ggak_kind': 1.0, 'ggak_mu': 1.0},
                      [('hartree',), ('term', 'perrot'), ('ggak', 'pg', 1.0), ('lda_x',), ('pz_c',)]),
    'sm_pgs_chach': (['tf', 'vw', 'wt_nl', 'gga_k', 'lda_x', 'chachiyo_c'], dict(PGS, wt_alpha=0.5, wt_beta=0.5),
                     [('term', 'sm'), ('ggak', 'pg', 40 / 27), ('lda_x',), ('chachiyo_c',)]),
    'pgslr_h': (['hartree', 'vw', 'gga_k'], dict(PGS, ggak_beta=0.25, ggak_lambda=0.4, ggak_sigma=0.2),
                [('hartree',), ('term', 'pgslr')]),
    'pgsl025': (['vw', 'gga_k'], dict(PGS, ggak_beta=0.25), [('term', 'pgsl025')]),
    'vwgtf1_h': (['ion_electron', 'hartree', 'vw', 'vwgtf'], {'vwgtf_kind': 1.0},
                 [('ion_electron',), ('hartree',), ('term', 'vwgtf1')]),
    'vwgtf2_pw': (['vw', 'vwgtf', 'lda_x', 'pw_c'], {'vwgtf_kind': 2.0}, [('term', 'vwgtf2'), ('lda_x',), ('pw_c',)]),
    'wts_exp': (['tf', 'vw', 'wt_nl'], {'wts_kind': 1.0}, [('term', 'wts_exp')]),
}
LAPLACIAN_GGA = {'pgslr_h', 'pgsl025'}

# (shape, cell).  fp32 cross-wave kernel (two lines per lane) runs where every line count is even; n2 = 270 leaves no kz
# remainder planes (n2 / 2 + 1 = 136 = 17 x 8), the remainder map is empty and the launcher falls back (xpass_impl.h)
MATRIX = [
    ((128, 32, 64), 'ortho'),
    ((256, 16, 64), 'tri'),
    ((256, 32, 32), 'ortho'),
    ((512, 16, 32), 'ortho'),
    ((1024, 16, 16), 'ortho'),
    ((1024, 8, 32), 'tri'),
    ((480, 16, 32), 'tri'),          # mixed-radix x
    ((32, 32, 256), 'ortho'),        # z rows of 128 / 256 / 512 points and a mixed-radix row (240)
    ((16, 32, 512), 'tri'),
    ((16, 16, 1024), 'ortho'),
    ((32, 16, 480), 'ortho'),
    ((128, 8, 270), 'ortho'),        # the fp32 NL = 2 fallback at every cross-wave line length
    ((256, 8, 270), 'tri'),
    ((512, 8, 270), 'ortho'),
    ((1024, 8, 270), 'ortho'),
]
XWAVES = (1, 0, 2, 5)
XC_LINES = (128, 256, 512, 1024)

_ORACLE = {}
_REPORT = os.environ.get('OFDFT_MATRIX_REPORT')


def make_cell(shape, kind):
    """orthogonal non-cubic (the WGC99 table fold runs) or triclinic (it does not), ~0.24 bohr per grid step"""
    if kind == 'ortho':
        return np.diag([7.6 * s / 32.0 * (1.0 + 0.1 * i) for i, s in enumerate(shape)])
    return synth.triclinic_cell(1.0) * (np.asarray(shape, dtype=float)[:, None] / 32.0)


def inputs(shape, cell):
    seed = 1000 + sum(shape) + (7 if cell == 'tri' else 0)
    return sc.full_spectrum_inputs(shape, seed)


def _oracle_sum(ev, pieces, n, vext):
    E, v = 0.0, np.zeros_like(n)
    for p in pieces:
        if p[0] == 'term':
            e, vt = ev.term(p[1], n, vext)
        elif p[0] == 'ion_electron':
            e, vt = ev.ion_electron(n, vext)
        else:
            e, vt = getattr(ev, p[0])(n, *p[1:])
        E, v = E + e, v + vt
    return E, v


def oracle(shape, cell, ts):
    """fp64 oracle of energy_potential and of the closure (E, mu, chi.grad; system.py:830-853), once per (shape, cell, term set)"""
    key = (shape, cell, ts)
    if key not in _ORACLE:
        box = make_cell(shape, cell)
        den, vext, chi = inputs(shape, cell)
        n_elec = float(np.floor(den.mean() * abs(np.linalg.det(box))) + 0.3)
        ev = cf.Evaluator(cf.Grid(box, shape))
        pieces = TERM_SETS[ts][2]
        E, v = _oracle_sum(ev, pieces, den, vext)
        c = n_elec / float(np.mean(chi * chi) * ev.g.vol)
        n = c * chi * chi
        Ec, vc = _oracle_sum(ev, pieces, n, vext)
        mu = float(np.mean(vc * n) * ev.g.vol / n_elec)
        g = c * 2 * chi * (vc - mu) * ev.g.dV
        _ORACLE[key] = dict(box=box, den=den, vext=vext, chi=chi, n_elec=n_elec, E=E, v=v, vk=sc.spectrum(v),
                            Ec=Ec, mu=mu, g=g, gk=sc.spectrum(g))
    return _ORACLE[key]


def expected_kinds(shape, p, xwave, fused=True):
    """the exact OFDFT_Q_XPASS_KINDS of an evaluation, or None where only 'some fused x pass ran' is fixed (OFDFT_OPT_XWAVE 1,
    and 5 on lines without a cross-wave kernel: wave-local for passes over >= 3 spectra, group-parallel for the rest)"""
    if not fused:
        return 0
    n0, n2 = shape[0], shape[2]
    pow2_le512 = n0 in (8, 16, 32, 64, 128, 256, 512)
    if xwave == 0:
        return N.XPASS_GROUP
    if xwave == 2:
        return N.XPASS_WAVE if pow2_le512 else N.XPASS_GROUP
    if xwave == 5 and n0 in XC_LINES:
        if p == 'f64':
            return N.XPASS_CROSS1
        if (n2 // 2 + 1) % 8 == 0:       # no remainder planes: a line group would straddle the (empty) remainder map
            return N.XPASS_WAVE if n0 <= 512 else N.XPASS_GROUP
        return N.XPASS_CROSS2
    return None


def _record(**kw):
    if _REPORT:
        with open(_REPORT, 'a') as f:
            f.write(json.dumps(kw) + '\n')


def run_case(shape, cell, ts, xwaves=XWAVES, gsplits=(1, 0), dtypes=('f64', 'f32')):
    o = oracle(shape, cell, ts)
    names, params, _ = TERM_SETS[ts]
    kinds_seen = {}
    for p in dtypes:
        dt = DTYPES[p]
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=DEV)  # noqa: E731
        den, vext, chi = t(o['den']), t(o['vext']), t(o['chi'])
        eng = Engine(shape, DEV, dtype=dt).set_cell(torch.as_tensor(o['box'])).set_terms(names, params)
        eng.set_option(N.OPT_GRAPH, 0).set_option(N.OPT_RESIDENT, 0)
        for xw in xwaves:
            for gs in gsplits:
                eng.set_option(N.OPT_XWAVE, xw).set_option(6, gs)
                fused = not (ts in LAPLACIAN_GGA and gs == 0)
                want = expected_kinds(shape, p, xw, fused)
                what = (shape, cell, ts, p, xw, gs)
                E, v = eng.energy_potential(den, vext)
                k1 = int(eng.query(N.Q_XPASS_KINDS))
                ev, ek = sc.check(v.cpu().numpy(), o['v'], p, what + ('potential',), o['vk'], sum(E.values()), o['E'])
                Ec, mu, g = eng.energy_grad_chi(chi, o['n_elec'], vext)
                k2 = int(eng.query(N.Q_XPASS_KINDS))
                gv, gk = sc.check(g.cpu().numpy(), o['g'], p, what + ('closure',), o['gk'], sum(Ec.values()), o['Ec'])
                assert abs(mu - o['mu']) <= sc.MU_TOL[p] * max(1.0, abs(o['mu'])), (what, mu, o['mu'])
                _record(shape=shape, cell=cell, ts=ts, dtype=p, xwave=xw, gsplit=gs, kinds=[k1, k2],
                        err_E=abs(sum(E.values()) - o['E']) / max(1.0, abs(o['E'])), err_v=ev, err_vk=ek,
                        err_Ec=abs(sum(Ec.values()) - o['Ec']) / max(1.0, abs(o['Ec'])), err_g=gv, err_gk=gk,
                        err_mu=abs(mu - o['mu']) / max(1.0, abs(o['mu'])))
                for k in (k1, k2):
                    if want is None:
                        assert k and not k & N.XPASS_CHIRPZ, (what, k)
                    else:
                        assert k == want, (what, k, want)
                kinds_seen[(p, xw)] = kinds_seen.get((p, xw), 0) | k1 | k2
        eng.close()
    return kinds_seen


@pytest.mark.parametrize('ts', list(TERM_SETS))
@pytest.mark.parametrize('shape,cell', MATRIX, ids=['%dx%dx%d-%s' % (s + (c,)) for s, c in MATRIX])
def test_fused_kernels_match_the_oracle_at_every_extent(shape, cell, ts):
    fallback = (shape[2] // 2 + 1) % 8 == 0
    t0 = time.time()
    seen = run_case(shape, cell, ts, xwaves=(1, 5) if fallback else XWAVES)
    if shape[0] in XC_LINES:
        # the kernel the case is there for ran: cross-wave, in fp32 with two lines per lane unless the shape forces the fallback
        assert seen[('f64', 5)] == N.XPASS_CROSS1
        assert bool(seen[('f32', 5)] & N.XPASS_CROSS2) != fallback, seen
    _record(shape=shape, cell=cell, ts=ts, seconds=time.time() - t0)


@pytest.mark.parametrize('shape,cell', [((256, 256, 256), 'ortho'), ((512, 256, 128), 'tri')])
def test_full_size_grid_without_tiling_matches_the_oracle(shape, cell):
    """the launch geometry of the benchmark sizes, remainder tiles included, on a full-spectrum input (no 32^3 tiling) with a
    term set outside configs 1-3 (WGC98 + LKT + PBE), default kernel choice, both builds"""
    t0 = time.time()
    seen = run_case(shape, cell, 'wgc98_lkt_pbe', xwaves=(1,), gsplits=(1,))
    assert seen[('f64', 1)] & N.XPASS_CROSS1 and seen[('f32', 1)] & N.XPASS_CROSS2, seen
    _ORACLE.pop((shape, cell, 'wgc98_lkt_pbe'), None)
    _record(shape=shape, cell=cell, ts='wgc98_lkt_pbe', seconds=time.time() - t0)
