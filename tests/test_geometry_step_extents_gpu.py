"""The routines called once per geometry step -- ofdft_stress, ofdft_ionic_potential, ofdft_ion_electron_forces and
ofdft_ion_electron_stress -- at odd, large and mixed-radix extents, against the fp64 oracle (oracle/stress.py, oracle/ions.py)
on full-spectrum densities (tests/spectral_check.py).

The reference goldens of these routines are all on even extents, and larger grids are reached elsewhere only by periodic
tiling, whose spectrum is empty off the tile frequencies.  Here:
  * odd n2 (33, 53, 67): the last kz plane of the half spectrum has weight 2 (half_weight, stress_kernels.h / ion_kernels.h);
  * odd grids run their transforms on the chirp-z path (x <= 256) or the three-pass chirp-z form (257 along x); 48 x 96 x 120 the
    mixed-radix fast path;
  * every term with a stress branch in ofdft_stress, one LDA correlation per term set (with several active each entry gets the
    mean of their shared reduction);
  * ions at awkward positions -- fractional coordinate exactly 0, on a grid point, negative, >= 1, 1 - 1e-16, two ions on one
    point -- with the exact structure factor and PME orders below the smallest extent (the oracle's numpy += does not
    accumulate repeated stencil indices).
Tolerances are those of the golden tests (test_gpu_parity.py): 2e-10 of max |sigma| per term, 1e-10 for the ion-electron stress,
1e-11 relative for the potential and the forces.
"""
import math
import os
import time

import numpy as np
import pytest
import torch

import spectral_check as sc
import test_extent_matrix_gpu as M
from oracle import ions as oi
from oracle import stress as st
from professad_amd import _native as N
from professad_amd.engine import Engine
from professad_amd.ions import ion_electron_forces, ion_electron_stress, ionic_potential, recpot_table

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
S5 = math.sqrt(5.0)
WGC98 = ((5 + S5) / 6, (5 - S5) / 6)

SHAPES = [
    ((27, 35, 33), 'tri'),       # odd everywhere, chirp-z with the fused z + y pass
    ((53, 53, 53), 'cubic'),     # the reference's own small grid
    ((65, 30, 67), 'ortho'),     # separate chirp-z z and y passes, x at M = 256
    ((257, 9, 20), 'tri'),       # x > 256 (chirp-z at M = 1024), even n2
    ((48, 96, 120), 'tri'),      # mixed-radix fast path
]

# name: (engine terms, engine params, {term: oracle stress of that term}) -- every term with a stress branch in ofdft_stress
STRESS_SETS = {
    'hartree_tf_vw': (['hartree', 'tf', 'vw'], {}, {'hartree': st.hartree, 'tf': st.tf, 'vw': st.vw}),
    'wt_56': (['wt_nl'], {}, {'wt_nl': st.wt_nl}),
    'wt_wgc98': (['wt_nl'], {'wt_alpha': WGC98[0], 'wt_beta': WGC98[1]},
                 {'wt_nl': lambda b, n: st.wt_nl(b, n, *WGC98)}),
    'wgc99': (['tf', 'vw', 'wgc99_nl'], {}, {'tf': st.tf, 'vw': st.vw, 'wgc99_nl': st.wgc99_nl}),
    'lda_pz': (['lda_x', 'pz_c'], {}, {'lda_x': lambda b, n: st.lda(b, n, 'lda_x'), 'pz_c': lambda b, n: st.lda(b, n, 'pz_c')}),
    'lda_pw': (['lda_x', 'pw_c'], {}, {'lda_x': lambda b, n: st.lda(b, n, 'lda_x'), 'pw_c': lambda b, n: st.lda(b, n, 'pw_c')}),
    'lda_chachiyo': (['lda_x', 'chachiyo_c'], {},
                     {'lda_x': lambda b, n: st.lda(b, n, 'lda_x'), 'chachiyo_c': lambda b, n: st.lda(b, n, 'chachiyo_c')}),
    'pbe': (['pbe_x', 'pbe_c'], {}, {'pbe_x': lambda b, n: st.pbe(b, n, True, False), 'pbe_c': lambda b, n: st.pbe(b, n, False, True)}),
    'lkt': (['vw', 'gga_k'], {'ggak_kind': 0.0}, {'vw': st.vw, 'gga_k': lambda b, n: st.ggak(b, n, 'lkt')}),
    'pg1': (['vw', 'gga_k'], {'ggak_kind': 1.0, 'ggak_mu': 1.0}, {'gga_k': lambda b, n: st.pauli_gaussian(b, n, 1.0, beta=0.0)}),
    'pgs': (['vw', 'gga_k'], {'ggak_kind': 1.0}, {'gga_k': lambda b, n: st.pauli_gaussian(b, n, 40 / 27, beta=0.0)}),
    'pgsl025': (['vw', 'gga_k'], {'ggak_kind': 1.0, 'ggak_beta': 0.25},          # Laplacian members: STRESS_HESS
                {'gga_k': lambda b, n: st.pauli_gaussian(b, n, 40 / 27, 0.25)}),
    'pgslr': (['vw', 'gga_k'], {'ggak_kind': 1.0, 'ggak_beta': 0.25, 'ggak_lambda': 0.4, 'ggak_sigma': 0.2},
              {'gga_k': lambda b, n: st.pauli_gaussian(b, n, 40 / 27, 0.25, 0.4, 0.2)}),
    'vwgtf1': (['vw', 'vwgtf'], {'vwgtf_kind': 1.0}, {'vwgtf': lambda b, n: st.vwgtf(b, n, 1)}),
    'vwgtf2': (['vw', 'vwgtf'], {'vwgtf_kind': 2.0}, {'vwgtf': lambda b, n: st.vwgtf(b, n, 2)}),
    # the stabilised Wang-Teter style functional splits its stress over tf / vw / wt_nl with native weights: the sum is pinned
    'wts_exp': (['tf', 'vw', 'wt_nl'], {'wts_kind': 1.0}, {'sum': st.wang_teter_style}),
}
PME_ORDERS = (4, 6, 10)
SIG_RTOL, ION_SIG_RTOL, ION_RTOL = 2e-10, 1e-10, 1e-11


def make_cell(shape, kind):
    if kind == 'cubic':
        return np.eye(3) * 0.24 * shape[0]
    return M.make_cell(shape, kind)


def density(shape, kind):
    """full-spectrum density (synth.random_density white noise on a constant: every k-point carries weight)"""
    return sc.full_spectrum_inputs(shape, 2000 + sum(shape) + (7 if kind == 'tri' else 0))[0]


def awkward_ions(shape):
    """fractional coordinates where wrapping and stencil indexing go wrong"""
    n0, n1, n2 = shape
    return np.array([[0.0, 0.0, 0.0],                              # exactly 0
                     [3 / n0, 5 / n1, (n2 - 1) / n2],                 # on a grid point (the last z plane)
                     [-0.3, -0.05, -1.71],                            # negative
                     [1.0, 1.7, 2.25],                                # >= 1
                     [1 - 1e-16, 1 - 1e-16, 1 - 1e-16],               # just below 1: f n may round up to n
                     [0.37, 0.61, 0.13], [0.37, 0.61, 0.13],          # two ions on one point
                     [0.5, -1e-17, 0.999]])                          # -1e-17 wraps to 1.0, then to 0


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - b)) / np.max(np.abs(b)))


@pytest.fixture(scope='module')
def recpot():
    g = np.load(os.path.join(GOLDEN, 'ions.npz'))
    raw, kmax = g['recpot_raw'], float(g['recpot_kmax'])
    return raw, kmax, recpot_table(raw, kmax)


@pytest.mark.parametrize('shape,cell', SHAPES, ids=['%dx%dx%d-%s' % (s + (c,)) for s, c in SHAPES])
def test_stress_of_every_term_matches_the_oracle(shape, cell):
    t0 = time.time()
    box, den = make_cell(shape, cell), density(shape, cell)
    eng = Engine(shape, DEV).set_cell(torch.as_tensor(box))
    assert bool(eng.query(N.Q_FAST_PATH)) == (shape == (48, 96, 120))
    d = torch.as_tensor(den, device=DEV)
    worst, bad = {}, []
    for name, (terms, params, want) in STRESS_SETS.items():
        sig = eng.set_terms(terms, params).stress(d)
        for term, f in want.items():
            ref = f(box, den)
            got = sum(sig[t] for t in terms) if term == 'sum' else sig[term]
            e = _rel(got, ref)
            worst[name + ':' + term] = e
            if not e <= SIG_RTOL:
                bad.append((name, term, e))
    eng.close()
    M._record(shape=shape, cell=cell, test='stress', worst=max(worst.values()), seconds=time.time() - t0)
    assert not bad, (shape, bad)


@pytest.mark.parametrize('shape,cell', SHAPES, ids=['%dx%dx%d-%s' % (s + (c,)) for s, c in SHAPES])
def test_ion_routines_at_awkward_positions_match_the_oracle(shape, cell, recpot):
    t0 = time.time()
    raw, kmax, tab = recpot
    box, den = make_cell(shape, cell), density(shape, cell)
    frac = awkward_ions(shape)
    eng = Engine(shape, DEV).set_cell(torch.as_tensor(box))
    d = torch.as_tensor(den, device=DEV)
    errs, bad = {}, []
    for o in (None,) + tuple(p for p in PME_ORDERS if p < min(shape)):
        v = ionic_potential(eng, box, [(frac, tab)], pme_order=o).cpu().numpy()
        F = ion_electron_forces(eng, box, d, [(frac, tab)], pme_order=o)[0]
        s = ion_electron_stress(eng, box, d, [(frac, tab)], pme_order=o)
        e = dict(v=_rel(v, oi.ionic_potential(box, shape, frac, raw, kmax, o)),
                 F=_rel(F, oi.ion_electron_forces(box, shape, frac, den, raw, kmax, o)),
                 s=_rel(s, st.ion_electron(box, den, frac, raw, kmax, o)))
        errs[o] = e
        bad += [(o, k, x) for k, x in e.items() if not x <= (ION_SIG_RTOL if k == 's' else ION_RTOL)]
        assert np.abs(F[5] - F[6]).max() <= 1e-14 * np.abs(F).max(), (o, F[5], F[6])      # two ions on one point: one force
    # the two coincident ions as one species each accumulate to the same potential
    v2 = ionic_potential(eng, box, [(frac[:6], tab), (frac[6:], tab)], pme_order=4).cpu().numpy()
    e2 = _rel(v2, oi.ionic_potential(box, shape, frac, raw, kmax, 4))
    eng.close()
    M._record(shape=shape, cell=cell, test='ions', errs={str(k): e for k, e in errs.items()}, species=e2,
              seconds=time.time() - t0)
    assert not bad and e2 <= ION_RTOL, (shape, bad, e2)


def test_fp32_engine_hands_the_geometry_step_to_its_fp64_sibling(recpot):
    """an fp32 engine on an odd grid: stress, forces and ion-electron stress are fp64 work on the widened density, the
    ionic potential is narrowed on the way out"""
    raw, kmax, tab = recpot
    shape, cell = (27, 35, 33), 'tri'
    box = make_cell(shape, cell)
    d32 = torch.as_tensor(density(shape, cell), dtype=torch.float32, device=DEV)
    den = d32.double().cpu().numpy()
    frac = awkward_ions(shape)
    eng = Engine(shape, DEV, dtype=torch.float32).set_cell(torch.as_tensor(box))
    for name in ('wgc99', 'pbe', 'pgslr'):
        terms, params, want = STRESS_SETS[name]
        sig = eng.set_terms(terms, params).stress(d32)
        for term, f in want.items():
            assert _rel(sig[term], f(box, den)) <= SIG_RTOL, (name, term)
    for o in (None, 6):
        v = ionic_potential(eng, box, [(frac, tab)], pme_order=o)
        assert v.dtype == torch.float32
        assert _rel(v.cpu().numpy(), oi.ionic_potential(box, shape, frac, raw, kmax, o)) <= 1e-7, o
        F = ion_electron_forces(eng, box, d32, [(frac, tab)], pme_order=o)[0]
        assert _rel(F, oi.ion_electron_forces(box, shape, frac, den, raw, kmax, o)) <= ION_RTOL, o
        s = ion_electron_stress(eng, box, d32, [(frac, tab)], pme_order=o)
        assert _rel(s, st.ion_electron(box, den, frac, raw, kmax, o)) <= ION_SIG_RTOL, o
    eng.close()
