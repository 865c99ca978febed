#!/usr/bin/env python3
"""Time the kinetic preconditioner and the preconditioned conjugate gradients against the plain solver, inside
ONE process.  Every time is reported beside the unpreconditioned run of the same process.

(a) operator: one Engine.precondition (ofdft_precondition) on an n^3 grid with the default pipeline (fused x pass) and with
    OFDFT_OPT_PIPELINE = 1 (forward, multiply, inverse), alternating, beside Engine.hessian_vector_chi with reuse_density -- the
    product an iteration of the solve runs -- on hartree + tf + vw + wt_nl + lda_x + pz_c.  Per round and variant `steps` timed
    calls after `warmup` untimed ones (every call ends in a stream synchronisation); medians over the rounds.
(b) response: on the fcc-Al cell of tools/fc_probe.py at its truncated-Newton ground state, one optimize.density_response to
    d v_ext / d R_x of ion 1 at rtol 1e-10 without and with precondition='auto', alternating; iterations and wall time.
(c) optimisers: tools/tn_probe.py's set-up -- the fused L-BFGS to its default stop, then truncated Newton without and with
    tn_precondition='auto' until max|g| / dV is below what L-BFGS reached; evaluations, products and wall time (each after one
    untimed run, median of `opt_rounds` alternating rounds).
usage: pcg_probe.py [--grids 128,256] [--response-grids 64,128] [--steps 100] [--warmup 5] [--rounds 5] [--opt-rounds 3]
                    [--out profiles/pcg.jsonl]"""
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
from professad_amd import _native as N  # noqa: E402
from professad_amd import ions, optimize, synth  # noqa: E402
from professad_amd.engine import Engine  # noqa: E402

SIX = ['hartree', 'tf', 'vw', 'wt_nl', 'lda_x', 'pz_c']
OPERATOR = ['precondition_fused', 'precondition_unfused', 'product_reuse']


def emit(rows, **row):
    rows.append(row)
    print(json.dumps(row), flush=True)


def operator(n, a, dev, rows):
    shape = (n, n, n)
    box = synth.cubic_cell(n)
    den_np = synth.smooth_density(shape, seed=1234)
    chi = torch.as_tensor(den_np, device=dev).sqrt()
    n_elec = float(den_np.sum() * abs(np.linalg.det(box)) / den_np.size)
    kappa2 = optimize.kinetic_kappa2(n_elec, abs(np.linalg.det(box)))
    d = torch.as_tensor(synth.random_density(shape, seed=77) - 0.033, device=dev)
    eng = Engine(shape, dev).set_cell(box).set_terms(SIX)
    g = eng.energy_grad_chi(chi, n_elec)[2]
    out, z = torch.empty_like(chi), torch.empty_like(chi)

    def prepare(v):
        eng.set_option(N.OPT_PIPELINE, 1 if v == 'precondition_unfused' else 0)
        if v == 'product_reuse':
            eng.hessian_vector_chi(chi, d, g, n_elec, out=out)

    def call(v):
        if v == 'product_reuse':
            return eng.hessian_vector_chi(chi, d, g, n_elec, reuse_density=True, out=out)
        return eng.precondition(d, kappa2, out=z)

    times = {v: [] for v in OPERATOR}
    for rnd in range(1, a.rounds + 1):
        for v in OPERATOR:
            prepare(v)
            for _ in range(a.warmup):
                call(v)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(a.steps):
                call(v)
            torch.cuda.synchronize(dev)
            times[v].append((time.perf_counter() - t0) / a.steps * 1e3)
            emit(rows, part='operator', grid=n, dtype='f64', round=rnd, variant=v, ms_per_call=round(times[v][-1], 4), steps=a.steps,
                 warmup=a.warmup)
    eng.set_option(N.OPT_PIPELINE, 0)
    med = {v: statistics.median(times[v]) for v in OPERATOR}
    emit(rows, part='operator', grid=n, dtype='f64', kappa2=kappa2, summary='median over %d rounds' % a.rounds,
         ms_per_call={v: round(med[v], 4) for v in OPERATOR},
         spread={v: [round(min(times[v]), 4), round(max(times[v]), 4)] for v in OPERATOR},
         ratio_fused_to_unfused=round(med['precondition_fused'] / med['precondition_unfused'], 3),
         ratio_fused_to_product_reuse=round(med['precondition_fused'] / med['product_reuse'], 3))
    eng.close()


def response(n, a, dev, rows):
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'ions.npz'))
    tab = ions.recpot_table(g['recpot_raw'], float(g['recpot_kmax']))
    box = g['a_box']
    frac = g['a_frac'] + 0.02 * np.random.default_rng(5).standard_normal((4, 3))
    species = [(frac, tab)]
    n_elec = 4 * float(tab[2])
    shape = (n, n, n)
    eng = Engine(shape, dev).set_cell(box)
    vext = ions.ionic_potential(eng, box, species)
    eng.set_terms(['ion_electron'] + SIX)
    gs = optimize.optimize_density(eng, n_elec, vext, volume=abs(np.linalg.det(box)), n_method='TN', tn_precondition='auto')
    emit(rows, part='response', grid=n, entry='ground_state', converged=bool(gs['converged']), evaluations=gs['func_evals'],
         products=gs['hvp_count'], max_g_over_dV=gs['history'][-1][3])
    chi = gs['chi']
    dv = ions.ionic_potential_gradient(eng, box, species, 1)[0]
    backends = {'plain': optimize.HipCgBackend(eng), 'preconditioned': optimize.HipCgBackend(eng, precondition='auto')}
    t, last = {v: [] for v in backends}, {}

    def solve(v):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        r = optimize.density_response(eng, chi, n_elec, dv, rtol=1e-10, maxiter=a.maxiter, backend=backends[v])
        torch.cuda.synchronize(dev)
        return r, (time.perf_counter() - t0) * 1e3
    for v in backends:
        solve(v)                                   # untimed
    for rnd in range(1, a.opt_rounds + 1):
        for v in backends:
            last[v], ms = solve(v)
            t[v].append(ms)
            emit(rows, part='response', grid=n, round=rnd, variant=v, ms=round(ms, 3), iterations=last[v]['iterations'],
                 products=last[v]['hvp_count'], reason=last[v]['reason'], rel_residual=last[v]['rel_residual'])
    med = {v: statistics.median(t[v]) for v in backends}
    apart = float((last['plain']['dn'] - last['preconditioned']['dn']).abs().max() / last['plain']['dn'].abs().max())
    emit(rows, part='response', grid=n, dtype='f64', rtol=1e-10, summary='median over %d rounds' % a.opt_rounds,
         ms={v: round(med[v], 3) for v in med}, spread={v: [round(min(t[v]), 3), round(max(t[v]), 3)] for v in t},
         iterations={v: last[v]['iterations'] for v in last},
         ms_per_iteration={v: round(med[v] / max(1, last[v]['iterations']), 4) for v in med},
         ratio_time_preconditioned_to_plain=round(med['preconditioned'] / med['plain'], 4), dn_apart=apart)
    for b in backends.values():
        b.close()
    eng.close()


def optimisers(n, a, dev, rows):
    shape = (n, n, n)
    box = synth.cubic_cell(n)
    vol = abs(np.linalg.det(box))
    den_np = synth.smooth_density(shape, seed=1234)
    n_elec = float(den_np.sum() * vol / den_np.size)
    vext = torch.as_tensor(0.2 * (den_np / den_np.mean() - 1.0), device=dev)      # tools/tn_probe.py's
    eng = Engine(shape, dev).set_cell(box).set_terms(['ion_electron'] + SIX)

    def run(method, **kw):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        r = optimize.optimize_density(eng, n_elec, vext, volume=vol, n_method=method, **kw)
        torch.cuda.synchronize(dev)
        return r, (time.perf_counter() - t0) * 1e3

    ref, _ = run('LBFGS')                          # untimed: also fixes the gradient level truncated Newton has to reach
    target = ref['history'][-1][3]
    tn_kw = dict(conv_target='dEdchi', ntol=target, n_conv_cond_count=1)
    variants = (('LBFGS', 'LBFGS', {}), ('TN', 'TN', tn_kw), ('TN_preconditioned', 'TN', dict(tn_kw, tn_precondition='auto')))
    for _name, m, kw in variants[1:]:
        run(m, **kw)
    t, last = {v[0]: [] for v in variants}, {}
    for _rnd in range(a.opt_rounds):
        for name, m, kw in variants:
            last[name], ms = run(m, **kw)
            t[name].append(ms)
    for name, _m, _kw in variants:
        r = last[name]
        emit(rows, part='optimisers', grid=n, dtype='f64', terms='ion_electron+' + '+'.join(SIX), method=name,
             ms=round(statistics.median(t[name]), 2), spread=[round(min(t[name]), 2), round(max(t[name]), 2)],
             ratio_to_TN=round(statistics.median(t[name]) / statistics.median(t['TN']), 3),
             ratio_to_LBFGS=round(statistics.median(t[name]) / statistics.median(t['LBFGS']), 3),
             iterations=r['iterations'], evaluations=r['func_evals'], products=r['hvp_count'], converged=bool(r['converged']),
             E_Ha=r['E_Ha'], max_g_over_dV=r['history'][-1][3], target_max_g_over_dV=target)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grids', default='128,256')
    ap.add_argument('--response-grids', default='64,128')
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--opt-rounds', type=int, default=3)
    ap.add_argument('--maxiter', type=int, default=3000, help='of the response solves (plain: about 780 iterations at 128^3)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pcg.jsonl'))
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    rows = []
    for n in (int(g) for g in a.grids.split(',') if g):
        operator(n, a, dev, rows)
    for n in (int(g) for g in a.response_grids.split(',') if g):
        response(n, a, dev, rows)
    for n in (int(g) for g in a.grids.split(',') if g):
        optimisers(n, a, dev, rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        for r in rows:
            fh.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
