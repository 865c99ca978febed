#!/usr/bin/env python3
"""Time the closure evaluation of the Huang-Carter kinds against WGC99 and against the unfused pipeline's transforms, inside ONE
process, alternating.

Variants per grid (fp64, smooth density, closure form ofdft_energy_grad_chi):
    hc          TF + vW + HuangCarter(0.01177, 0.7143, 1.2)
    revhc       TF + vW + RevisedHuangCarter(0.45, 0.10, 2/3, 1.15)
    wgc99       TF + vW + WGC99 (the default, fused pipeline: what profiles/nlk_256.jsonl records)
    wgc99_unf   TF + vW + WGC99 with OFDFT_OPT_PIPELINE = 1: the unfused pipeline, whose whole-grid transforms are the ones the
                Huang-Carter chain runs; its time / its transform count is the per-transform yardstick of this run
Per round and variant `steps` timed calls after `warmup` untimed ones (every call ends in a stream synchronisation, so the host
clock around the block is the time of the work); the profiling switch stays off.  Writes one JSON row per (grid, round, variant)
and one summary row per (grid, variant) -- the median over the rounds, M, the transform count, the launch count, the workspace
bytes and, for hc / revhc, ratio_to_transforms = median / (transform count x the unfused per-transform time) -- to --out
(profiles/hc.jsonl).
usage: hc_probe.py [--grids 128,256] [--steps 20] [--warmup 3] [--rounds 5] [--out profiles/hc.jsonl]"""
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
from professad_amd import synth  # noqa: E402
from professad_amd.engine import Engine  # noqa: E402

VARIANTS = {
    'hc': (('tf', 'vw', 'nlk'), dict(nlk_kind=4, nlk_p0=0.01177, nlk_p1=0.7143, nlk_p2=1.2), None),
    'revhc': (('tf', 'vw', 'nlk'), dict(nlk_kind=5, nlk_p0=0.45, nlk_p1=0.10, nlk_p2=2 / 3, nlk_p3=1.15), None),
    'wgc99': (('tf', 'vw', 'wgc99_nl'), None, None),
    'wgc99_unf': (('tf', 'vw', 'wgc99_nl'), None, 1),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grids', default='128,256')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hc.jsonl'))
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    rows = []
    for n in (int(g) for g in a.grids.split(',')):
        shape = (n, n, n)
        box = synth.cubic_cell(n)
        den = synth.smooth_density(shape, seed=20240601)
        n_elec = float(den.mean() * abs(np.linalg.det(box)))
        chi = torch.as_tensor(np.sqrt(den), device=dev)
        engs = {}
        for v, (names, p, pipeline) in VARIANTS.items():
            engs[v] = Engine(shape, dev).set_cell(box).set_terms(names, p)
            if pipeline is not None:
                engs[v].set_option(N.OPT_PIPELINE, pipeline)
        rest = Engine(shape, dev).set_cell(box).set_terms(('tf', 'vw'))          # the transforms of the rest of the hc / revhc term sets
        rest.energy_grad_chi(chi, n_elec)
        rest_transforms = int(rest.query(N.Q_FFT_COUNT))
        rest.close()
        times = {v: [] for v in VARIANTS}
        meta = {}
        for rnd in range(1, a.rounds + 1):
            for v, e in engs.items():
                for _ in range(a.warmup):
                    e.energy_grad_chi(chi, n_elec)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    e.energy_grad_chi(chi, n_elec)
                torch.cuda.synchronize(dev)
                ms = (time.perf_counter() - t0) / a.steps * 1e3
                times[v].append(ms)
                meta[v] = dict(transforms=int(e.query(N.Q_FFT_COUNT)), launches=int(e.query(N.Q_LAUNCH_COUNT)),
                               workspace_bytes=int(e.query(N.Q_WORKSPACE_BYTES)))
                rows.append(dict(grid=n, dtype='f64', round=rnd, variant=v, ms_per_call=round(ms, 4)))
        per_transform = statistics.median(times['wgc99_unf']) / meta['wgc99_unf']['transforms']
        for v in VARIANTS:
            s = dict(grid=n, dtype='f64', variant=v, summary=True, median_ms=round(statistics.median(times[v]), 4), rounds=a.rounds,
                     steps=a.steps, **meta[v])
            if v in ('hc', 'revhc'):
                s['M'] = (meta[v]['transforms'] - rest_transforms - 10) // 2          # the chain runs 2 M + 10 transforms
                s['unfused_ms_per_transform'] = round(per_transform, 5)
                s['ratio_to_transforms'] = round(statistics.median(times[v]) / (meta[v]['transforms'] * per_transform), 3)
                s['ratio_to_wgc99'] = round(statistics.median(times[v]) / statistics.median(times['wgc99']), 2)
            rows.append(s)
            print(json.dumps(s), flush=True)
        for e in engs.values():
            e.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        for r in rows:
            fh.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
