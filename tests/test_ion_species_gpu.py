"""professad_amd/ions.py with a real species list: 320 ions of two species whose recpot tables differ in length, k_max and charge --
200 on the table of tests/golden/ions.npz (10002 points, k_max = 30, z = 3) and 120 on system_double.second_recpot (1537 points,
k_max = 9, z = 5: most k-points of these grids lie beyond its end, where recpot_value clamps) -- against the numpy double of
tests/system_double.py, on (16, 16, 32) orthorhombic and (27, 35, 33) triclinic (chirp-z) with full-spectrum densities.

The ions are a 4 x 4 x 5 tiling of a four-ion basis, jittered with a fixed seed, with coordinates below 0 and above 1 and one
coincident pair (system_double.tiled_ions): more ions than a workgroup has threads, in every routine.  ionic_potential,
ion_electron_forces and ion_electron_stress run with the exact structure factor and PME orders 4, 6 and 10; the species in the other
order give the same potential and stress to 1e-13 and the forces move with their species; one ion per species, drawn by seed, is
also compared for ionic_potential_gradient and ion_electron_curvature against tests/fc_double.py.

Bounds.  The project's: 1e-11 of the maximum for potential and forces, 1e-10 for the stress, 1e-11 for the second-order entries.
With hundreds of ions the sums are longer and the PME spread accumulates atomically, so the double's own spread is measured on the
CPU -- the double evaluated with the ions of each species in reversed order -- and where it exceeds a quarter of the default bound
the bound becomes four times the spread (`bounds`); never sized from the engine's output.  Spread of the double (forces are sums
per ion and do not depend on the order at all: 0 everywhere) against a quarter of the default bound (2.5e-12 / 2.5e-11):
    (16, 16, 32) ortho   potential 5.2e-16 exact, 2.7e-16 / 4.8e-16 / 5.2e-14 PME 4 / 6 / 10;  stress <= 1.6e-16
    (27, 35, 33) tri     potential 5.0e-16 exact, 0 / 5.3e-16 / 4.9e-14 PME 4 / 6 / 10;        stress <= 1.0e-18
so no bound is re-derived: the defaults hold.  Both numbers (spread, bound) of every case go through
test_extent_matrix_gpu._record.

Measured on an MI355X, worst over both grids: potential 1.4e-14 exact and up to 9.8e-14 at PME order 10 (1.8e-15 / 3.1e-15 at orders
4 / 6), forces 2.2e-14 exact and 1.8e-13 PME, stress 8.7e-16; the species in the other order move the potential by at most 7.2e-14
(PME 10; 0 exact) and the stress by 1.8e-18, the forces not at all; gradient 5.8e-15 and curvature 3.6e-14 of the drawn ions.
At PME order 10 the spline factors b(m) are large near the Nyquist planes, which these densities and tables populate: the double's own
reorder spread there (5e-14) is as large as the engine's figure under the species swap, 2.8e-14 to 7.2e-14 over five runs (the spread
kernel accumulates atomically, so it moves from run to run) -- less than a factor of two below the 1e-13 bound.  (The two species'
potentials are added by one commutative sum: the figure is the run-to-run spread of the atomics, not an effect of the order.)
"""
import numpy as np
import pytest
import torch

import fc_double as FD
import system_double as SD
import test_extent_matrix_gpu as M
from professad_amd.engine import Engine
from professad_amd.ions import (ion_electron_curvature, ion_electron_forces, ion_electron_stress, ionic_potential,
                                ionic_potential_gradient)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GRIDS = [((16, 16, 32), 'ortho'), ((27, 35, 33), 'tri')]
GRID_IDS = ['%dx%dx%d-%s' % (s + (c,)) for s, c in GRIDS]
ORDERS = (None, 4, 6, 10)
DEFAULT = {'v': SD.ION_RTOL, 'F': SD.ION_RTOL, 's': SD.ION_SIG_RTOL}
SECOND_ORDER_BOUND = 1e-11          # tests/test_second_order_extents_gpu.py (FINDING)

_DOUBLE = {}


def species_list():
    """[(frac [200, 3], (raw, k_max)), (frac [120, 3], (raw, k_max))]"""
    fa, fb = SD.tiled_ions()
    return [(fa, SD.golden_recpot()), (fb, SD.second_recpot()[:2])]


def inputs(shape, cell):
    return M.make_cell(shape, cell), M.inputs(shape, cell)[0]


def _evaluate(box, den, species, order):
    return dict(v=SD.species_potential(box, den.shape, species, order), F=SD.species_forces(box, den, species, order),
                s=SD.species_stress(box, den, species, order))


def double(shape, cell, order):
    """the double of one case, its spread under a reordering of the ions and the bounds that follow; once per (shape, cell, order)"""
    key = (shape, cell, order)
    if key not in _DOUBLE:
        box, den = inputs(shape, cell)
        species = species_list()
        a = _evaluate(box, den, species, order)
        b = _evaluate(box, den, [(f[::-1].copy(), tab) for f, tab in species], order)
        fscale = max(np.abs(f).max() for f in a['F'])
        spread = dict(v=SD.rel(b['v'], a['v']), s=SD.rel(b['s'], a['s']),
                      F=max(np.abs(fb[::-1] - fa).max() for fa, fb in zip(a['F'], b['F'])) / fscale)
        a['spread'] = spread
        a['bound'] = bounds(spread)
        _DOUBLE[key] = a
    return _DOUBLE[key]


def bounds(spread):
    """the default bound, or four times the double's own spread where that spread exceeds a quarter of the default"""
    return {k: (DEFAULT[k] if spread[k] <= DEFAULT[k] / 4 else 4 * spread[k]) for k in DEFAULT}


def test_bounds_follow_the_spread_of_the_double():
    assert bounds(dict(v=2.4e-12, F=0.0, s=2.6e-11)) == dict(v=1e-11, F=1e-11, s=4 * 2.6e-11)
    assert bounds(dict(v=2.6e-12, F=1e-11, s=0.0)) == dict(v=4 * 2.6e-12, F=4e-11, s=1e-10)


@pytest.mark.parametrize('order', ORDERS, ids=lambda o: 'exact' if o is None else 'pme%d' % o)
@pytest.mark.parametrize('shape,cell', GRIDS, ids=GRID_IDS)
def test_ion_routines_with_two_species_match_the_double(shape, cell, order):
    box, den = inputs(shape, cell)
    o = double(shape, cell, order)
    species = SD.tables(species_list())
    assert sum(f.shape[0] for f, _ in species) == 320 and species[0][1][0].size != species[1][1][0].size
    assert order is None or order < min(shape)          # (the oracle's numpy += does not accumulate repeated stencil indices)
    eng = Engine(shape, DEV)
    d = torch.as_tensor(den, device=DEV)
    v = ionic_potential(eng, box, species, pme_order=order).cpu().numpy()
    Fs = ion_electron_forces(eng, box, d, species, pme_order=order)
    s = ion_electron_stress(eng, box, d, species, pme_order=order)
    # the species in the other order: the same potential and stress, the forces move with their species
    v2 = ionic_potential(eng, box, species[::-1], pme_order=order).cpu().numpy()
    F2 = ion_electron_forces(eng, box, d, species[::-1], pme_order=order)
    s2 = ion_electron_stress(eng, box, d, species[::-1], pme_order=order)
    eng.close()
    fscale = max(np.abs(f).max() for f in o['F'])
    err = dict(v=SD.rel(v, o['v']), s=SD.rel(s, o['s']), F=max(np.abs(a - b).max() for a, b in zip(Fs, o['F'])) / fscale)
    swap = dict(v=SD.rel(v2, v), s=SD.rel(s2, s), F=max(np.abs(a - b).max() for a, b in zip(F2[::-1], Fs)) / fscale)
    M._record(test='ion_species', shape=shape, cell=cell, order=order, err=err, swap=swap, spread=o['spread'], bound=o['bound'])
    print('MEASURE ions %s %s %s: err %s swapped %s spread %s bound %s' % (shape, cell, order, err, swap, o['spread'], o['bound']))
    SD.check_ion_potential(v, o['v'], o['bound']['v'], (shape, order))
    SD.check_forces(Fs, o['F'], o['bound']['F'], (shape, order))
    SD.check_stress(s, o['s'], o['bound']['s'], (shape, order))
    assert [f.shape for f in F2] == [f.shape for f in Fs[::-1]]
    assert swap['v'] <= 1e-13 and swap['s'] <= 1e-13 and swap['F'] <= 1e-13, swap
    assert np.array_equal(species[0][0][7], species[1][0][1])          # the coincident pair: one ion of each species


@pytest.mark.parametrize('shape,cell', GRIDS, ids=GRID_IDS)
def test_second_order_entries_of_one_ion_per_species(shape, cell):
    """ionic_potential_gradient and ion_electron_curvature of one ion per species, drawn by seed, against fc_double"""
    box, den = inputs(shape, cell)
    species = SD.tables(species_list())
    rng = np.random.default_rng(sum(shape))
    picks = [int(rng.integers(0, species[0][0].shape[0])), int(rng.integers(0, species[1][0].shape[0]))]
    eng = Engine(shape, DEV)
    d = torch.as_tensor(den, device=DEV)
    Dc = ion_electron_curvature(eng, box, d, species)
    errs = {}
    for s, a in enumerate(picks):
        frac, tab = species[s]
        ion = a + (0 if s == 0 else species[0][0].shape[0])
        dv = ionic_potential_gradient(eng, box, species, ion).cpu().numpy()
        errs['gradient%d' % s] = SD.rel(dv, FD.potential_gradient(box, shape, (frac @ box)[a], tab))
        errs['curvature%d' % s] = SD.rel(Dc[s][a], FD.ion_electron_curvature(box, den, frac[[a]], tab)[0])
    eng.close()
    M._record(test='ion_species', shape=shape, cell=cell, picks=picks, err=errs)
    print('MEASURE second order %s %s ions %s: %s' % (shape, cell, picks, errs))
    assert max(errs.values()) <= SECOND_ORDER_BOUND, errs
