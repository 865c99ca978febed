#!/usr/bin/env python3
"""Time the Hessian-vector product of Wang-Teter + PBE (cfg3, OFDFT_OPT_HVP_GGA = 1) and its reuse call against those of
Wang-Teter + Perdew-Zunger (cfg2), inside ONE process, alternating (the method of hvp_probe.py).

Four variants per grid, fp64, ion_electron + hartree + tf + vw + wt_nl and
    cfg3 / cfg3_reuse    + pbe_x + pbe_c: 22 / 14 transforms, two transform stages around hvp_gga_mid_kernel
    cfg2 / cfg2_reuse    + lda_x + pz_c:  10 / 6 transforms
Per round and variant `steps` timed calls after `warmup` untimed ones (every call ends in a stream synchronisation, so the host
clock around the block is the time of the work); the profiling switch stays off while the clock runs.  After the timed rounds one
profiled pass of `steps` calls per variant records the time per kernel class (Engine.profile) and OFDFT_Q_KERNEL_MS of its last call.
Writes one JSON row per (grid, round, variant), one per (grid, variant) with the kernel classes, and one summary row per grid --
medians over the rounds, ms per transform, the mid kernel's time per call and that time in units of one transform of cfg2 -- to
--out (profiles/hvp_gga.jsonl).
usage: hvp_gga_probe.py [--grids 128,256] [--steps 20] [--warmup 5] [--rounds 5] [--out profiles/hvp_gga.jsonl]"""
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

BASE = ['ion_electron', 'hartree', 'tf', 'vw', 'wt_nl']
SETS = {'cfg3': BASE + ['pbe_x', 'pbe_c'], 'cfg2': BASE + ['lda_x', 'pz_c']}
VARIANTS = ['cfg3', 'cfg3_reuse', 'cfg2', 'cfg2_reuse']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grids', default='128,256')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hvp_gga.jsonl'))
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    rows = []
    for n in (int(g) for g in a.grids.split(',')):
        shape = (n, n, n)
        box = synth.cubic_cell(n)
        den = torch.as_tensor(synth.random_density(shape, seed=1234), device=dev)
        w = torch.as_tensor(synth.random_density(shape, seed=77) - 0.033, device=dev)
        engs = {k: Engine(shape, dev).set_cell(box).set_terms(names) for k, names in SETS.items()}
        engs['cfg3'].set_option(N.OPT_HVP_GGA, 1)

        def call(v):
            return engs[v[:4]].hessian_vector(den, w, reuse_density=v.endswith('_reuse'))

        def block(v, count):
            if v.endswith('_reuse'):
                engs[v[:4]].hessian_vector(den, w)          # the call whose density fields the following ones reuse
            for _ in range(count):
                call(v)

        times = {v: [] for v in VARIANTS}
        meta = {}
        for rnd in range(1, a.rounds + 1):
            for v in VARIANTS:
                e = engs[v[:4]]
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
                rows.append(dict(grid=n, dtype='f64', terms='+'.join(SETS[v[:4]]), round=rnd, variant=v, ms_per_call=round(ms, 4),
                                 steps=a.steps, warmup=a.warmup, **meta[v]))
                print(json.dumps(rows[-1]), flush=True)
        kernels = {}
        for v in VARIANTS:                                  # per kernel class, outside the timed rounds
            e = engs[v[:4]]
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
        mid = kernels['cfg3'].get('hvp_gga_mid', 0.0)
        rows.append(dict(grid=n, dtype='f64', summary='median over %d rounds' % a.rounds,
                         ms_per_call={v: round(med[v], 4) for v in VARIANTS},
                         spread={v: [round(min(times[v]), 4), round(max(times[v]), 4)] for v in VARIANTS},
                         transforms={v: meta[v]['transforms'] for v in VARIANTS},
                         ms_per_transform={v: round(per_fft[v], 4) for v in VARIANTS},
                         ratio_cfg3_to_cfg2=round(med['cfg3'] / med['cfg2'], 3),
                         ratio_cfg3_reuse_to_cfg2_reuse=round(med['cfg3_reuse'] / med['cfg2_reuse'], 3),
                         mid_kernel_ms=mid, mid_kernel_in_cfg2_transforms=round(mid / per_fft['cfg2'], 3)))
        print(json.dumps(rows[-1]), flush=True)
        for e in engs.values():
            e.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        for r in rows:
            fh.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
