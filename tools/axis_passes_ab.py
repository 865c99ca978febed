#!/usr/bin/env python3
"""OFDFT_OPT_AXIS_PASSES values against each other on the bench's workload, inside ONE process and on one engine, alternating:
per round and value `steps` timed closure evaluations after `warmup` untimed ones (a change of the option drops the captured
state, so every block warms up again).  One JSON row per (round, value) on stdout.
usage: axis_passes_ab.py [--grid 256] [--dtype f64|f32] [--steps 20] [--warmup 5] [--rounds 3] [--values 3,1,0]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from professad_amd import _native as N  # noqa: E402
from professad_amd.engine import Engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grid', type=int, default=256)
    ap.add_argument('--dtype', default='f64', choices=['f64', 'f32'])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--values', default='3,1,0')
    a = ap.parse_args()
    n = a.grid
    dev = torch.device('cuda', 0)
    tdtype = torch.double if a.dtype == 'f64' else torch.float32
    box, chi_h, vext_h, n_elec, _ = bench.make_inputs(n, 0)
    eng = Engine((n, n, n), dev, dtype=tdtype).set_cell(torch.as_tensor(box)).set_terms(bench.CFG3)
    chi = torch.as_tensor(chi_h, dtype=tdtype, device=dev)
    vext = torch.as_tensor(vext_h, dtype=tdtype, device=dev)
    for rnd in range(1, a.rounds + 1):
        for val in (int(v) for v in a.values.split(',')):
            eng.set_option(N.OPT_AXIS_PASSES, val)
            for _ in range(a.warmup):
                E, mu, g = eng.energy_grad_chi(chi, n_elec, vext)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(a.steps):
                E, mu, g = eng.energy_grad_chi(chi, n_elec, vext)
            torch.cuda.synchronize(dev)
            ms = (time.perf_counter() - t0) / a.steps * 1e3
            print(json.dumps({'workload': '%d^3 %s cfg3 closure, %d steps after %d' % (n, a.dtype, a.steps, a.warmup), 'round': rnd,
                              'axis_passes': val, 'ms_per_step': round(ms, 4), 'y_passes': eng.query(N.Q_YPASS_COUNT),
                              'launches': int(eng.query(N.Q_LAUNCH_COUNT)), 'energy_Ha': sum(E.values()), 'mu': mu}), flush=True)
    eng.close()


if __name__ == '__main__':
    main()
