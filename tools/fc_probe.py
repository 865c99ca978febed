#!/usr/bin/env python3
"""Time the force-constant pipeline and its entries on the fcc-Al conventional cell (4 ions, the al.gga table of
tests/golden/ions.npz, ions shifted off their sites as in tests/golden/fc_cases.py), fp64, one process.

Per grid: a truncated-Newton ground state of ion_electron + hartree + tf + vw + wt_nl + lda_x + pz_c, then
    column                    force_constants(primitive_ion_indices=[0]): three solves; wall time / 3, iterations and products
    potential_gradient        ofdft_ionic_potential_gradient (one spectral pass, three inverse transforms)
    potential_one_ion         ofdft_ionic_potential for ONE ion on the same grid (one spectral pass, one inverse transform): the
                              natural comparison of the entry above
    curvature                 ofdft_ion_electron_curvature (one transform, one reduction over 4 ions)
    ion_electron_forces       ofdft_ion_electron_forces (the same shape of work, three sums instead of six)
    ion_ion_hessian           ofdft_ion_ion_hessian, all four rows
Per round and entry `steps` timed calls after `warmup` untimed ones (every call ends in a stream synchronisation, so the host
clock around the block is the time of the work).  Writes one JSON row per (grid, round, entry) and one summary row per grid
(medians over the rounds) to --out (profiles/force_constants.jsonl).
usage: fc_probe.py [--grids 64,128] [--steps 10] [--warmup 3] [--rounds 3] [--maxiter 3000] [--out profiles/force_constants.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from professad_amd import ions, optimize  # noqa: E402
from professad_amd.engine import Engine  # noqa: E402
from professad_amd.force_constants import force_constants  # noqa: E402

TERMS = ['ion_electron', 'hartree', 'tf', 'vw', 'wt_nl', 'lda_x', 'pz_c']
ENTRIES = ['potential_gradient', 'potential_one_ion', 'curvature', 'ion_electron_forces', 'ion_ion_hessian']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grids', default='64,128')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--maxiter', type=int, default=3000, help='of the response solves (unpreconditioned: 400 iterations at 64^3)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'force_constants.jsonl'))
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'ions.npz'))
    tab = ions.recpot_table(g['recpot_raw'], float(g['recpot_kmax']))
    box = g['a_box']
    frac = g['a_frac'] + 0.02 * np.random.default_rng(5).standard_normal((4, 3))
    species, one = [(frac, tab)], [(frac[:1], tab)]
    z = np.full(4, float(tab[2]))
    rows = []
    for n in (int(s) for s in a.grids.split(',')):
        shape = (n, n, n)
        eng = Engine(shape, dev).set_cell(box)
        vext = ions.ionic_potential(eng, box, species)
        eng.set_terms(TERMS)
        t0 = time.perf_counter()
        gs = optimize.optimize_density(eng, float(z.sum()), vext, volume=abs(np.linalg.det(box)), n_method='TN')
        rows.append(dict(grid=n, entry='ground_state', seconds=round(time.perf_counter() - t0, 4), converged=bool(gs['converged']),
                         evaluations=gs['func_evals'], products=gs['hvp_count']))
        print(json.dumps(rows[-1]), flush=True)
        chi, den = gs['chi'], gs['den']
        calls = {
            'potential_gradient': lambda: ions.ionic_potential_gradient(eng, box, species, 0),
            'potential_one_ion': lambda: ions.ionic_potential(eng, box, one),
            'curvature': lambda: ions.ion_electron_curvature(eng, box, den, species),
            'ion_electron_forces': lambda: ions.ion_electron_forces(eng, box, den, species),
            'ion_ion_hessian': lambda: ions.ion_ion_hessian(eng, box, frac, z, range(4)),
        }
        times = {v: [] for v in ENTRIES + ['column']}
        col = None
        for rnd in range(1, a.rounds + 1):
            for v in ENTRIES:
                for _ in range(a.warmup):
                    calls[v]()
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    calls[v]()
                torch.cuda.synchronize(dev)
                times[v].append((time.perf_counter() - t0) / a.steps * 1e3)
                rows.append(dict(grid=n, round=rnd, entry=v, ms_per_call=round(times[v][-1], 4), steps=a.steps, warmup=a.warmup))
                print(json.dumps(rows[-1]), flush=True)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            col = force_constants(eng, box, species, chi, primitive_ion_indices=[0], maxiter=a.maxiter)
            times['column'].append((time.perf_counter() - t0) / 3 * 1e3)
            rows.append(dict(grid=n, round=rnd, entry='column', ms_per_column=round(times['column'][-1], 3), iterations=col['iterations'],
                             products=col['hvp_count'], reasons=col['reason'], maxiter=a.maxiter, rel_residual=col['rel_residual'], asr_residual=col['asr_residual']))
            print(json.dumps(rows[-1]), flush=True)
        med = {v: statistics.median(times[v]) for v in times}
        rows.append(dict(grid=n, dtype='f64', terms='+'.join(TERMS), summary='median over %d rounds' % a.rounds,
                         ms={v: round(med[v], 4) for v in med},
                         spread={v: [round(min(times[v]), 4), round(max(times[v]), 4)] for v in times},
                         ms_per_product_in_a_column=round(med['column'] * 3 / col['hvp_count'], 4),
                         ratio_gradient_to_one_ion_potential=round(med['potential_gradient'] / med['potential_one_ion'], 3)))
        print(json.dumps(rows[-1]), flush=True)
        eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        for r in rows:
            fh.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
