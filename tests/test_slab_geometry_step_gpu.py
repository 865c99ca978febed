"""The routines called once per geometry step -- ofdft_stress, ofdft_ionic_potential, ofdft_ion_electron_forces and
ofdft_ion_electron_stress -- on slab-decomposed contexts (nranks 2 to 8), against the fp64 oracle (oracle/stress.py,
oracle/ions.py) and against one engine on the full grid.

On slabs these routines take a path of their own (engine_ions_stress.inc.h, lines.hip): PME spreading / gathering on the rank's
own x planes, the b1 factors offset by the y-slab origin, every k-space kernel on the rank's y-slab, every reduced number through
global_sums, normalisations by the global grid, every transform through the all-to-all callback.  The P ranks are P contexts in
one process, each on its own thread, with the collectives of tests/local_ranks.py (ThreadCollectives; its logic is tested on
the CPU in tests/test_local_collectives_cpu.py).

Term sets, PME orders, awkward ions, densities, cells and the three oracle tolerances are those of
tests/test_geometry_step_extents_gpu.py, unchanged; the geometries are the smallest of tests/test_slab_matrix_gpu.py with each
layout property:
  16 x 16 x 16, 8, tri      nxl = nyl = 2: a stencil of order 4 / 6 / 10 spans up to 5 ranks and wraps from rank 7 to rank 0
  8 x 8 x 32, 8, ortho      nxl = nyl = 1 (orders 4, 6)
  64 x 32 x 48, 4, ortho    mixed-radix z
  96 x 48 x 120, 4, tri     mixed radix on all axes, 61 kz planes (7 blocks + 5 remainder planes)
  32 x 64 x 270, 8, ortho   no remainder planes
  1024 x 8 x 16, 8, ortho   128 planes per rank, nyl = 1 (orders 4, 6)
  64 x 64 x 32, 2, tri      two kz blocks
The ions are awkward_ions(shape) plus four on the slab boundaries: x fraction exactly on the first plane of rank 1 and of rank
P - 1, the last double below the first plane of rank 1, and half a grid step below 1 (the stencil wraps from the last rank into
rank 0); y and z generic.

Bounds.  Against the oracle: SIG_RTOL, ION_SIG_RTOL, ION_RTOL of the single-engine file.  Against one engine, relative to
max |.| of the one-engine result (per term for the stress): the project's 1e-12 (tests/test_dist_gpu.py:
_check_worker_results) for every quantity -- ONE_TOL below; no measured maximum exceeds it, so none is widened.  The ranks'
partial sums add up in another order than one GPU's.  Maxima over all cases, measured on an MI355X (OFDFT_MATRIX_REPORT
records them per case, the tests print every figure):
                          slabs - oracle   one engine - oracle   slabs - one engine   bound (oracle / one engine)
  stress, per term           3.3e-13            3.3e-13               8.4e-16            2e-10 / 1e-12
  ionic potential            8.2e-15            8.2e-15               4.4e-16            1e-11 / 1e-12   (bitwise equal in most cases)
  ion-electron forces        7.5e-13            7.5e-13               2.8e-13            1e-11 / 1e-12   (PME; exact sum 5.0e-14 / 4.2e-16)
  ion-electron stress        1.7e-15            1.7e-15               5.8e-16            1e-10 / 1e-12
Seconds per case (own process; oracle included): stress 0.4 - 0.7, 1.7 / 1.8 on the two 553k-point grids; ion routines
0.3 - 0.5, 1.1 / 1.0 on those; the untouched-hot-path cases 0.4 -- so the oracle is not cached beyond a case.
"""
import re
import time

import numpy as np
import pytest
import torch

import test_extent_matrix_gpu as M
import test_geometry_step_extents_gpu as G
import test_slab_matrix_gpu as S
from local_ranks import LocalRanks, _identical
from oracle import ions as oi
from oracle import stress as st
from professad_amd.engine import Engine
from professad_amd.ions import ion_electron_forces, ion_electron_stress, ionic_potential

pytestmark = pytest.mark.gpu
DEV = G.DEV
recpot = G.recpot          # (the module-scoped fixture of the single-engine file)

GEOMETRIES = [
    ((16, 16, 16), 8, 'tri'),
    ((8, 8, 32), 8, 'ortho'),
    ((64, 32, 48), 4, 'ortho'),
    ((96, 48, 120), 4, 'tri'),
    ((32, 64, 270), 8, 'ortho'),
    ((1024, 8, 16), 8, 'ortho'),
    ((64, 64, 32), 2, 'tri'),
]
UNTOUCHED = [((16, 16, 16), 8, 'tri'), ((64, 64, 32), 2, 'tri')]
SERVED = [name for name in G.STRESS_SETS if name != 'wts_exp']
# slabs against one engine, relative to max |one engine| (per term for the stress): stress of a term, ionic potential, forces,
# ion-electron stress
ONE_TOL = dict(sig=1e-12, v=1e-12, F=1e-12, s=1e-12)


def slab_ions(shape, P):
    """G.awkward_ions plus ions on the slab boundaries (x); the two coincident ions stay at rows 5 and 6"""
    n0 = shape[0]
    nxl = n0 // P
    edge = np.array([[nxl * 1 / n0, 0.23, 0.71],                          # exactly on the first plane of rank 1
                     [nxl * (P - 1) / n0, 0.58, 0.34],                    # ... and of the last rank
                     [np.nextafter(nxl * 1 / n0, 0), 0.81, 0.09],         # the last double below rank 1's first plane
                     [(nxl * P - 0.5) / n0, 0.44, 0.92]])                 # the stencil wraps from the last rank into rank 0
    return np.concatenate([G.awkward_ions(shape), edge])


def _setup(shape, P, cell):
    box, den = G.make_cell(shape, cell), G.density(shape, cell)
    bt = torch.as_tensor(box)
    return box, den, torch.as_tensor(den, device=DEV), LocalRanks(shape, DEV, P).set_cell(bt), Engine(shape, DEV).set_cell(bt)


def _stress_errors(name, sig, one, refs, bad, worst):
    """one term set's slab stress `sig` against the oracle `refs` and the one-engine stress `one`, per term"""
    terms = G.STRESS_SETS[name][0]
    for term, ref in refs.items():
        e, e1 = G._rel(sig[term], ref), G._rel(one[term], ref)
        worst['oracle'] = max(worst['oracle'], e)
        worst['one_oracle'] = max(worst['one_oracle'], e1)
        print('stress %s:%s slab-oracle %.3g one-oracle %.3g' % (name, term, e, e1))
        if not e <= G.SIG_RTOL:
            bad.append((name, term, 'slab vs oracle', e))
        if not e1 <= G.SIG_RTOL:
            bad.append((name, term, 'one engine vs oracle', e1))
    for term in terms:
        e = G._rel(sig[term], one[term])
        worst['one'] = max(worst['one'], e)
        print('stress %s:%s slab-one %.3g' % (name, term, e))
        if not e <= ONE_TOL['sig']:
            bad.append((name, term, 'slab vs one engine', e))


@pytest.mark.parametrize('shape,P,cell', GEOMETRIES, ids=[S._gid(g) for g in GEOMETRIES])
def test_slab_stress_of_every_term_matches_the_oracle_and_one_engine(shape, P, cell):
    t0 = time.time()
    box, den, d, loc, eng = _setup(shape, P, cell)
    worst, bad, refs = dict(oracle=0.0, one_oracle=0.0, one=0.0), [], {}
    try:
        for name in SERVED:
            terms, params, want = G.STRESS_SETS[name]
            sig = loc.set_terms(terms, params).stress(d)
            one = eng.set_terms(terms, params).stress(d)
            refs[name] = {term: f(box, den) for term, f in want.items()}
            _stress_errors(name, sig, one, refs[name], bad, worst)
        # the stabilised Wang-Teter style functional: refused by ofdft_stress on every rank, and nobody is left waiting
        terms, params, _ = G.STRESS_SETS['wts_exp']
        loc.set_terms(terms, params)
        t1 = time.time()
        with pytest.raises(RuntimeError, match=S.REFUSED_WTS):
            loc.stress(d)
        assert time.time() - t1 < 0.5 * loc.COLLECTIVE_TIMEOUT
        errs = loc.coll.rank_errors
        assert len(errs) == P and all(isinstance(e, RuntimeError) and re.search(S.REFUSED_WTS, str(e)) for e in errs), errs
        # ... and the same contexts go on serving
        name = 'hartree_tf_vw'
        terms, params, _ = G.STRESS_SETS[name]
        _stress_errors(name, loc.set_terms(terms, params).stress(d), eng.set_terms(terms, params).stress(d), refs[name], bad, worst)
    finally:
        loc.close()
        eng.close()
    M._record(shape=shape, P=P, cell=cell, test='slab stress', seconds=time.time() - t0, **worst)
    assert not bad, (shape, P, bad)


@pytest.mark.parametrize('shape,P,cell', GEOMETRIES, ids=[S._gid(g) for g in GEOMETRIES])
def test_slab_ion_routines_match_the_oracle_and_one_engine(shape, P, cell, recpot):
    t0 = time.time()
    raw, kmax, tab = recpot
    box, den, d, loc, eng = _setup(shape, P, cell)
    frac = slab_ions(shape, P)
    sp = [(frac, tab)]
    orders = (None,) + tuple(p for p in G.PME_ORDERS if p < min(shape))
    assert len(orders) >= 3
    errs, bad = {}, []
    try:
        for o in orders:
            got = dict(v=loc.ionic_potential(sp, o).cpu().numpy(), F=loc.ion_electron_forces(d, sp, o)[0],
                       s=loc.ion_electron_stress(d, sp, o))
            one = dict(v=ionic_potential(eng, box, sp, pme_order=o).cpu().numpy(), F=ion_electron_forces(eng, box, d, sp, pme_order=o)[0],
                       s=ion_electron_stress(eng, box, d, sp, pme_order=o))
            ref = dict(v=oi.ionic_potential(box, shape, frac, raw, kmax, o), F=oi.ion_electron_forces(box, shape, frac, den, raw, kmax, o),
                       s=st.ion_electron(box, den, frac, raw, kmax, o))
            assert got['v'].shape == tuple(shape)
            e = {}
            for k in ('v', 'F', 's'):
                tol = G.ION_SIG_RTOL if k == 's' else G.ION_RTOL
                e[k], e[k + '_one_oracle'], e[k + '_one'] = G._rel(got[k], ref[k]), G._rel(one[k], ref[k]), G._rel(got[k], one[k])
                bad += [(o, k, what, x, bound) for what, x, bound in (('slab vs oracle', e[k], tol), ('one engine vs oracle', e[k + '_one_oracle'], tol),
                                                                      ('slab vs one engine', e[k + '_one'], ONE_TOL[k])) if not x <= bound]
            errs[str(o)] = e
            print('ions order %s: %s' % (o, ' '.join('%s %.3g' % kv for kv in e.items())))
            F = got['F']
            assert np.abs(F[5] - F[6]).max() <= 1e-14 * np.abs(F).max(), (o, F[5], F[6])      # two ions on one point: one force
        # the ions split over two species (the coincident pair apart) accumulate to the same potential
        sp2 = [(frac[:6], tab), (frac[6:], tab)]
        v2, v2_one = loc.ionic_potential(sp2, 4).cpu().numpy(), ionic_potential(eng, box, sp2, pme_order=4).cpu().numpy()
        e2 = G._rel(v2, oi.ionic_potential(box, shape, frac, raw, kmax, 4))
        e2_one = G._rel(v2, v2_one)
        print('ions two species: slab-oracle %.3g slab-one %.3g' % (e2, e2_one))
    finally:
        loc.close()
        eng.close()
    M._record(shape=shape, P=P, cell=cell, test='slab ions', errs=errs, species=e2, species_one=e2_one, seconds=time.time() - t0)
    assert not bad and e2 <= G.ION_RTOL and e2_one <= ONE_TOL['v'], (shape, P, bad, e2, e2_one)


def _geometry_step(loc, d, sp):
    return [loc.stress(d), loc.ionic_potential(sp, 4), loc.ion_electron_forces(d, sp, 4), loc.ion_electron_stress(d, sp, 4)]


def _bitwise(a, b):
    return all(torch.equal(x, y) if torch.is_tensor(x) else _identical(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('shape,P,cell', UNTOUCHED, ids=[S._gid(g) for g in UNTOUCHED])
def test_geometry_step_leaves_the_hot_path_untouched(shape, P, cell, recpot):
    """energy_potential and the closure before and after the four geometry-step routines: they share workspaces with the hot
    path, and dist_rfftn / dist_irfftn use its exchange buffers (and their receive parity) between evaluations"""
    t0 = time.time()
    tab = recpot[2]
    names, params, _ = M.TERM_SETS['wgc99_pbe']
    fields = M.inputs(shape, cell)
    box = M.make_cell(shape, cell)
    n_elec = float(np.floor(fields[0].mean() * abs(np.linalg.det(box))) + 0.3)
    den, vext, chi = S._tensors(fields, torch.double)
    n0, nxl = shape[0], shape[0] // P
    # at most two of these order-4 stencils share a grid point, so the spread's atomic sums do not depend on their order
    sp = [(np.array([[nxl / n0, 0.3, 0.7], [(n0 - 0.5) / n0, 0.8, 0.2], [0.37, 0.61, 0.13]]), tab)]
    loc = LocalRanks(shape, DEV, P).set_cell(torch.as_tensor(box)).set_terms(names, params)
    try:
        hot1 = [loc.energy_potential(den, vext), loc.closure(chi, n_elec, vext)]
        g1 = _geometry_step(loc, den, sp)
        hot2 = [loc.energy_potential(den, vext), loc.closure(chi, n_elec, vext)]
        g2 = _geometry_step(loc, den, sp)
        hot3 = [loc.energy_potential(den, vext), loc.closure(chi, n_elec, vext)]
    finally:
        loc.close()
    M._record(shape=shape, P=P, cell=cell, test='slab untouched', seconds=time.time() - t0)
    for i, (a, b, c) in enumerate(zip(hot1, hot2, hot3)):
        assert S._same(a, b) and S._same(a, c), (shape, P, 'hot-path evaluation %d changed after the geometry step' % i)
    assert _bitwise(g1, g2), (shape, P, 'the geometry step is not reproducible')
    assert loc.coll.calls[0] > 0 and loc.coll.calls[1] > 0
