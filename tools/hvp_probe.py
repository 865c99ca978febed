#!/usr/bin/env python3
"""Time the Hessian-vector product against the energy evaluation of the same term set, inside ONE process, alternating.

Four variants per grid on the set hartree + tf + vw + wt_nl + lda_x + pz_c (fp64):
    hvp            Engine.hessian_vector, everything computed (10 transforms)
    hvp_reuse      ... with reuse_density=True (6 transforms)
    eval_unfused   Engine.energy_potential with OFDFT_OPT_PIPELINE = 1: the same batched transforms and separate pointwise /
                   spectral kernels (6 transforms)
    eval_default   Engine.energy_potential with the default pipeline
Per round and variant `steps` timed calls after `warmup` untimed ones (every call ends in a stream synchronisation, so the host
clock around the block is the time of the work); the profiling switch stays off.  Writes one JSON row per (grid, round, variant)
and one summary row per grid -- medians over the rounds and the three ratios hvp / eval_unfused, hvp_reuse / eval_unfused,
hvp / eval_default -- to --out (profiles/hvp.jsonl).
usage: hvp_probe.py [--grids 128,256] [--steps 20] [--warmup 5] [--rounds 5] [--out profiles/hvp.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from professad_amd import _native as N  # noqa: E402
from professad_amd import synth  # noqa: E402
from professad_amd.engine import Engine  # noqa: E402

TERMS = ['hartree', 'tf', 'vw', 'wt_nl', 'lda_x', 'pz_c']
VARIANTS = ['hvp', 'hvp_reuse', 'eval_unfused', 'eval_default']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grids', default='128,256')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hvp.jsonl'))
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    rows = []
    for n in (int(g) for g in a.grids.split(',')):
        shape = (n, n, n)
        box = synth.cubic_cell(n)
        den = torch.as_tensor(synth.random_density(shape, seed=1234), device=dev)
        w = torch.as_tensor(synth.random_density(shape, seed=77) - 0.033, device=dev)
        # one engine per pipeline: a change of OFDFT_OPT_PIPELINE would drop the retained fields and the captured state
        engs = {'hvp': Engine(shape, dev).set_cell(box).set_terms(TERMS)}
        engs['hvp_reuse'] = engs['hvp']
        engs['eval_unfused'] = Engine(shape, dev).set_cell(box).set_terms(TERMS).set_option(N.OPT_PIPELINE, 1)
        engs['eval_default'] = Engine(shape, dev).set_cell(box).set_terms(TERMS)

        def call(v):
            e = engs[v]
            if v == 'hvp':
                return e.hessian_vector(den, w)
            if v == 'hvp_reuse':
                return e.hessian_vector(den, w, reuse_density=True)
            return e.energy_potential(den)[1]

        times = {v: [] for v in VARIANTS}
        meta = {}
        for rnd in range(1, a.rounds + 1):
            for v in VARIANTS:
                if v == 'hvp_reuse':
                    engs[v].hessian_vector(den, w)          # the call whose density fields the timed ones reuse
                for _ in range(a.warmup):
                    call(v)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    call(v)
                torch.cuda.synchronize(dev)
                ms = (time.perf_counter() - t0) / a.steps * 1e3
                times[v].append(ms)
                meta[v] = {'transforms': int(engs[v].query(N.Q_FFT_COUNT)), 'launches': int(engs[v].query(N.Q_LAUNCH_COUNT)),
                           'device_ms_last_call': round(engs[v].query(N.Q_KERNEL_MS), 4)}
                rows.append(dict(grid=n, dtype='f64', terms='+'.join(TERMS), round=rnd, variant=v, ms_per_call=round(ms, 4),
                                 steps=a.steps, warmup=a.warmup, **meta[v]))
                print(json.dumps(rows[-1]), flush=True)
        med = {v: statistics.median(times[v]) for v in VARIANTS}
        rows.append(dict(grid=n, dtype='f64', terms='+'.join(TERMS), summary='median over %d rounds' % a.rounds,
                         ms_per_call={v: round(med[v], 4) for v in VARIANTS},
                         spread={v: [round(min(times[v]), 4), round(max(times[v]), 4)] for v in VARIANTS},
                         ms_per_transform={v: round(med[v] / meta[v]['transforms'], 4) for v in VARIANTS},
                         transforms={v: meta[v]['transforms'] for v in VARIANTS},
                         ratio_hvp_to_eval_unfused=round(med['hvp'] / med['eval_unfused'], 3),
                         ratio_hvp_reuse_to_eval_unfused=round(med['hvp_reuse'] / med['eval_unfused'], 3),
                         ratio_hvp_to_eval_default=round(med['hvp'] / med['eval_default'], 3)))
        print(json.dumps(rows[-1]), flush=True)
        for e in {id(e): e for e in engs.values()}.values():
            e.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        for r in rows:
            fh.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
