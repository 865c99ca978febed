#!/usr/bin/env python3
"""Time the elastic-constant pipeline and its entries on the fcc-Al conventional cell (4 ions, the al.gga table of
tests/golden/ions.npz, ions shifted off their sites as in tests/golden/fc_cases.py), fp64, one process.

Per grid: a truncated-Newton ground state of ion_electron + hartree + tf + vw + wt_nl + lda_x + pz_c, then
    strain_gradient           ofdft_potential_strain_gradient (3 forward + 18 inverse transforms)
    hessian_vector            ofdft_hessian_vector without reuse of the same terms (10 transforms): its natural comparison
    ionic_strain_gradient     ofdft_ionic_potential_strain_gradient (one spectral pass, six inverse transforms)
    strain_hessian            ofdft_strain_hessian alone (three transforms, three moment reductions)
    stress                    ofdft_stress of the same terms: the natural comparison of the entry above
    ion_electron_strain_hessian, ion_electron_stress      one transform and one reduction each
    ion_ion_strain_hessian, ion_ion                        the pair scans
    elastic                   one full elastic_constants: six solves; wall time, iterations and products
The entries alternate within a round; per round and entry `steps` timed calls after `warmup` untimed ones (every call ends in a
stream synchronisation, so the host clock around the block is the time of the work).  Writes one JSON row per (grid, round, entry)
and one summary row per grid (medians over the rounds) to --out (profiles/elastic.jsonl).
usage: elastic_probe.py [--grids 64,128] [--steps 10] [--warmup 3] [--rounds 3] [--maxiter 3000] [--out profiles/elastic.jsonl]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from professad_amd import _native as N  # noqa: E402
from professad_amd import elastic, ions, optimize  # noqa: E402
from professad_amd.engine import Engine  # noqa: E402

TERMS = ['ion_electron', 'hartree', 'tf', 'vw', 'wt_nl', 'lda_x', 'pz_c']
ENTRIES = ['strain_gradient', 'hessian_vector', 'ionic_strain_gradient', 'strain_hessian', 'stress', 'ion_electron_strain_hessian',
           'ion_electron_stress', 'ion_ion_strain_hessian', 'ion_ion']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grids', default='64,128')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--maxiter', type=int, default=3000, help='of the response solves (unpreconditioned: 400 iterations at 64^3)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'elastic.jsonl'))
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'ions.npz'))
    tab = ions.recpot_table(g['recpot_raw'], float(g['recpot_kmax']))
    box = g['a_box']
    frac = g['a_frac'] + 0.02 * np.random.default_rng(5).standard_normal((4, 3))
    species = [(frac, tab)]
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
        buf = (C.c_double * (N.NTERMS * 81))()

        def strain_hessian_entry():          # the native entry alone (Engine.strain_hessian adds a stress and a product for the local terms)
            eng._check(eng.lib.ofdft_strain_hessian(eng._ctx, C.c_void_p(den.data_ptr()), buf, eng._stream()), 'ofdft_strain_hessian')
        calls = {
            'strain_gradient': lambda: eng.potential_strain_gradient(den),
            'hessian_vector': lambda: eng.hessian_vector(den, den),
            'ionic_strain_gradient': lambda: ions.ionic_potential_strain_gradient(eng, box, species),
            'strain_hessian': strain_hessian_entry,
            'stress': lambda: eng.stress(den),
            'ion_electron_strain_hessian': lambda: ions.ion_electron_strain_hessian(eng, box, den, species),
            'ion_electron_stress': lambda: ions.ion_electron_stress(eng, box, den, species),
            'ion_ion_strain_hessian': lambda: ions.ion_ion_strain_hessian(eng, box, frac, z),
            'ion_ion': lambda: ions.ion_ion(eng, box, frac, z),
        }
        times = {v: [] for v in ENTRIES + ['elastic']}
        full = None
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
            full = elastic.elastic_constants(eng, box, species, chi, maxiter=a.maxiter)
            times['elastic'].append((time.perf_counter() - t0) * 1e3)
            rows.append(dict(grid=n, round=rnd, entry='elastic', ms=round(times['elastic'][-1], 3), iterations=full['iterations'],
                             products=full['hvp_count'], reasons=full['reason'], maxiter=a.maxiter, rel_residual=full['rel_residual'],
                             bulk_modulus_GPa=full['bulk_modulus'] * elastic.GPA_PER_ATOMIC, symmetry_residual=full['symmetry_residual']))
            print(json.dumps(rows[-1]), flush=True)
        med = {v: statistics.median(times[v]) for v in times}
        rows.append(dict(grid=n, dtype='f64', terms='+'.join(TERMS), summary='median over %d rounds' % a.rounds,
                         ms={v: round(med[v], 4) for v in med},
                         spread={v: [round(min(times[v]), 4), round(max(times[v]), 4)] for v in times},
                         ms_per_product_in_the_call=round(med['elastic'] / full['hvp_count'], 4),
                         ratio_strain_gradient_to_hessian_vector=round(med['strain_gradient'] / med['hessian_vector'], 3),
                         ratio_strain_hessian_to_stress=round(med['strain_hessian'] / med['stress'], 3),
                         ratio_ion_electron=round(med['ion_electron_strain_hessian'] / med['ion_electron_stress'], 3),
                         ratio_ion_ion=round(med['ion_ion_strain_hessian'] / med['ion_ion'], 3)))
        print(json.dumps(rows[-1]), flush=True)
        eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        for r in rows:
            fh.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
