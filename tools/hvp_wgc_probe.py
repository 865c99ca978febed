#!/usr/bin/env python3
"""Time the Hessian-vector product of WGC99 + PBE (the bench set; OFDFT_OPT_HVP_WGC = 1, OFDFT_OPT_HVP_GGA = 1), of WGC99 + Perdew-Zunger
and their reuse calls against those of Wang-Teter + PBE (cfg3), inside ONE process, alternating (the method of hvp_gga_probe.py).

Six variants per grid, fp64, ion_electron + hartree + tf + vw and
    bench / bench_reuse    + wgc99_nl + pbe_x + pbe_c: 42 / 24 transforms
    wlda / wlda_reuse      + wgc99_nl + lda_x + pz_c:  30 / 16 transforms
    cfg3 / cfg3_reuse      + wt_nl + pbe_x + pbe_c:    22 / 14 transforms
Per round and variant `steps` timed calls after `warmup` untimed ones (every call ends in a stream synchronisation, so the host
clock around the block is the time of the work); the profiling switch stays off while the clock runs.  After the timed rounds one
profiled pass of `steps` calls per variant records the time per kernel class (Engine.profile).
Writes one JSON row per (grid, round, variant), one per (grid, variant) with the kernel classes, and one summary row per grid --
medians over the rounds, ms per transform and its ratio to cfg3's, the two WGC99 kernels' time per call, and the workspace bytes each
engine holds (OFDFT_Q_WORKSPACE_BYTES) -- to --out (profiles/hvp_wgc.jsonl).
usage: hvp_wgc_probe.py [--grids 128,256] [--steps 20] [--warmup 5] [--rounds 5] [--out profiles/hvp_wgc.jsonl]"""
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

BASE = ['ion_electron', 'hartree', 'tf', 'vw']
SETS = {'bench': BASE + ['wgc99_nl', 'pbe_x', 'pbe_c'], 'wlda': BASE + ['wgc99_nl', 'lda_x', 'pz_c'], 'cfg3': BASE + ['wt_nl', 'pbe_x', 'pbe_c']}
VARIANTS = ['bench', 'bench_reuse', 'wlda', 'wlda_reuse', 'cfg3', 'cfg3_reuse']


def key(v):
    return v.split('_')[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grids', default='128,256')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hvp_wgc.jsonl'))
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    rows = []
    for n in (int(g) for g in a.grids.split(',')):
        shape = (n, n, n)
        box = synth.cubic_cell(n)
        den = torch.as_tensor(synth.random_density(shape, seed=1234), device=dev)
        w = torch.as_tensor(synth.random_density(shape, seed=77) - 0.033, device=dev)
        engs = {k: Engine(shape, dev).set_cell(box).set_terms(names).set_option(N.OPT_HVP_GGA, 1).set_option(N.OPT_HVP_WGC, 1)
                for k, names in SETS.items()}

        def call(v):
            return engs[key(v)].hessian_vector(den, w, reuse_density=v.endswith('_reuse'))

        def block(v, count):
            if v.endswith('_reuse'):
                engs[key(v)].hessian_vector(den, w)          # the call whose density fields the following ones reuse
            for _ in range(count):
                call(v)

        times = {v: [] for v in VARIANTS}
        meta = {}
        for rnd in range(1, a.rounds + 1):
            for v in VARIANTS:
                e = engs[key(v)]
                block(v, a.warmup)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    call(v)
                torch.cuda.synchronize(dev)
                ms = (time.perf_counter() - t0) / a.steps * 1e3
                times[v].append(ms)
                meta[v] = {'transforms': int(e.query(N.Q_FFT_COUNT)), 'launches': int(e.query(N.Q_LAUNCH_COUNT)),
                           'device_ms_last_call': round(e.query(N.Q_KERNEL_MS), 4)}
                rows.append(dict(grid=n, dtype='f64', terms='+'.join(SETS[key(v)]), round=rnd, variant=v, ms_per_call=round(ms, 4),
                                 steps=a.steps, warmup=a.warmup, **meta[v]))
                print(json.dumps(rows[-1]), flush=True)
        kernels = {}
        for v in VARIANTS:                                  # per kernel class, outside the timed rounds
            e = engs[key(v)]
            block(v, 1)
            e.set_profiling(True)
            for _ in range(a.steps):
                call(v)
            kernels[v] = {k: round(ms / a.steps, 4) for k, (ms, _cnt) in sorted(e.profile().items())}
            e.set_profiling(False)
            rows.append(dict(grid=n, dtype='f64', variant=v, profiled='ms per call by kernel class over %d calls' % a.steps,
                             kernels=kernels[v], kernel_ms_last_call=round(e.query(N.Q_KERNEL_MS), 4)))
            print(json.dumps(rows[-1]), flush=True)
        med = {v: statistics.median(times[v]) for v in VARIANTS}
        per_fft = {v: med[v] / meta[v]['transforms'] for v in VARIANTS}
        rows.append(dict(grid=n, dtype='f64', summary='median over %d rounds' % a.rounds,
                         ms_per_call={v: round(med[v], 4) for v in VARIANTS},
                         spread={v: [round(min(times[v]), 4), round(max(times[v]), 4)] for v in VARIANTS},
                         transforms={v: meta[v]['transforms'] for v in VARIANTS},
                         ms_per_transform={v: round(per_fft[v], 4) for v in VARIANTS},
                         ms_per_transform_over_cfg3={v: round(per_fft[v] / per_fft['cfg3_reuse' if v.endswith('_reuse') else 'cfg3'], 3)
                                                     for v in VARIANTS},
                         wgc_head_ms=kernels['bench'].get('hvp_wgc_head', 0.0), wgc_tail_ms=kernels['bench'].get('hvp_wgc_tail', 0.0),
                         wgc_mix_ms=kernels['bench'].get('spec_wgc_mix', 0.0),
                         workspace_bytes={k: int(e.query(N.Q_WORKSPACE_BYTES)) for k, e in engs.items()}))
        print(json.dumps(rows[-1]), flush=True)
        for e in engs.values():
            e.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        for r in rows:
            fh.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
