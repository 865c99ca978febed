#!/usr/bin/env python3
"""Time the batched response solves against the solo path, inside ONE process, on the fcc-Al conventional cell of
tools/pcg_probe.py at its truncated-Newton ground state, with precondition='auto' and rtol 1e-10.  The solo path is the code the
batched one does not touch; no ratio is fixed in advance.

(a) solves: for B = 3, 6, 8 right-hand sides (d v_ext / d R of the ions, x, y, z of ion 0, then ion 1, ...), one
    optimize.density_response_multi of the B columns against B optimize.density_response calls on the same right-hand sides;
    wall time and iteration counts.
(b) drivers: one force_constants row (primitive_ion_indices=[1]) with batch=None and batch=3, and one elastic_constants call with
    batch=None and batch=6.
Both sides alternate inside a round, after one untimed run each; the figures are medians over `rounds` rounds.
usage: multi_probe.py [--grids 64,128] [--rounds 5] [--out profiles/response_multi.jsonl]"""
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
from professad_amd import elastic, ions, optimize  # noqa: E402
from professad_amd.engine import Engine  # noqa: E402
from professad_amd.force_constants import force_constants  # noqa: E402

TERMS = ['ion_electron', 'hartree', 'tf', 'vw', 'wt_nl', 'lda_x', 'pz_c']
RTOL = 1e-10


def emit(rows, **row):
    rows.append(row)
    print(json.dumps(row), flush=True)


def timed(dev, f):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize(dev)
    return r, (time.perf_counter() - t0) * 1e3


def alternate(dev, variants, rounds):
    """variants: {name: callable}; one untimed run each, then `rounds` alternating rounds -> ({name: [ms]}, {name: last result})"""
    t, last = {v: [] for v in variants}, {}
    for f in variants.values():
        f()
    for _rnd in range(rounds):
        for v, f in variants.items():
            last[v], ms = timed(dev, f)
            t[v].append(ms)
    return t, last


def grid(n, a, dev, rows):
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'ions.npz'))
    tab = ions.recpot_table(g['recpot_raw'], float(g['recpot_kmax']))
    box = g['a_box']
    frac = g['a_frac'] + 0.02 * np.random.default_rng(5).standard_normal((4, 3))
    species = [(frac, tab)]
    n_elec = 4 * float(tab[2])
    eng = Engine((n, n, n), dev).set_cell(box)
    vext = ions.ionic_potential(eng, box, species)
    eng.set_terms(TERMS)
    gs = optimize.optimize_density(eng, n_elec, vext, volume=abs(np.linalg.det(box)), n_method='TN', tn_precondition='auto')
    emit(rows, part='ground_state', grid=n, converged=bool(gs['converged']), evaluations=gs['func_evals'], products=gs['hvp_count'],
         max_g_over_dV=gs['history'][-1][3])
    chi = gs['chi']
    dvs = torch.cat([ions.ionic_potential_gradient(eng, box, species, p) for p in range(3)])[:8].contiguous()      # [8, n, n, n]
    solo = optimize.HipCgBackend(eng, precondition='auto')
    multi = optimize.HipCgMultiBackend(eng, 8, precondition='auto')
    kw = dict(rtol=RTOL, maxiter=a.maxiter)
    for B in (3, 6, 8):
        stack = dvs[:B].contiguous()
        t, last = alternate(dev, {
            'solo': lambda: [optimize.density_response(eng, chi, n_elec, stack[j], backend=solo, **kw) for j in range(B)],
            'batched': lambda: optimize.density_response_multi(eng, chi, n_elec, stack, backend=multi, **kw)}, a.rounds)
        med = {v: statistics.median(t[v]) for v in t}
        apart = max(float((last['batched']['dn'][j] - last['solo'][j]['dn']).abs().max() / last['solo'][j]['dn'].abs().max()) for j in range(B))
        emit(rows, part='solves', grid=n, dtype='f64', columns=B, rtol=RTOL, precondition='auto', summary='median over %d rounds' % a.rounds,
             ms={v: round(med[v], 3) for v in med}, spread={v: [round(min(t[v]), 3), round(max(t[v]), 3)] for v in t},
             ms_per_column={v: round(med[v] / B, 3) for v in med}, ratio_batched_to_solo=round(med['batched'] / med['solo'], 4),
             iterations=dict(solo=[r['iterations'] for r in last['solo']], batched=last['batched']['iterations']),
             products=dict(solo=sum(r['hvp_count'] for r in last['solo']), batched=last['batched']['hvp_count']), dn_apart=apart)
    solo.close()
    multi.close()
    drivers = {
        'force_constants_row': (lambda batch: force_constants(eng, box, species, chi, primitive_ion_indices=[1], rtol=RTOL, maxiter=a.maxiter,
                                                              precondition='auto', batch=batch), 3, 'phi'),
        'elastic_constants': (lambda batch: elastic.elastic_constants(eng, box, species, chi, rtol=RTOL, maxiter=a.maxiter, precondition='auto',
                                                                      batch=batch), 6, 'C'),
    }
    for name, (call, batch, key) in drivers.items():
        t, last = alternate(dev, {'solo': lambda: call(None), 'batched': lambda: call(batch)}, a.rounds)
        med = {v: statistics.median(t[v]) for v in t}
        apart = float(np.abs(last['batched'][key] - last['solo'][key]).max() / np.abs(last['solo'][key]).max())
        emit(rows, part='drivers', grid=n, dtype='f64', driver=name, batch=batch, rtol=RTOL, precondition='auto',
             summary='median over %d rounds' % a.rounds, ms={v: round(med[v], 3) for v in med},
             spread={v: [round(min(t[v]), 3), round(max(t[v]), 3)] for v in t}, ratio_batched_to_solo=round(med['batched'] / med['solo'], 4),
             iterations={v: last[v]['iterations'] for v in last}, products={v: last[v]['hvp_count'] for v in last}, result_apart=apart)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grids', default='64,128')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--maxiter', type=int, default=500)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'response_multi.jsonl'))
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    rows = []
    for n in (int(g) for g in a.grids.split(',') if g):
        grid(n, a, dev, rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        for r in rows:
            fh.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
