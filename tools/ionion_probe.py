"""Cell-list ion-ion sum against the direct kernel on fcc Al supercells with small random displacements: one JSON line per
case (appended to profiles/ionion_cells.jsonl, or --out).

    python tools/ionion_probe.py --ions 4096 --rc 40            # 8^3 / 16^3 / 32^3 primitive cells: 512, 4 096, 32 768 ions
    python tools/ionion_probe.py --ions 131072 --rc 250 --no-direct      # 32^3 conventional cells, a = 244.8 bohr (BASELINE config 5)

Each line: ions, Rc, Rd, cells m, mean / max occupancy, tile T, the ordered pair count (nions^2 (4/3) pi Rc^3 / vol, each pair
from both ends: exact up to the surface term for a near-uniform crystal), the median of --reps wall times of the whole call
(sort, upload, kernel, read-back) per method, pairs/s, and the differences between the methods in E/N, forces and stress.  The direct kernel runs only where
direct_candidates <= 2e11.  One process per case: run each under its own `timeout -k 10 <s>` and chain them with `&&`.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import ionion_cells_double as cd  # noqa: E402
from professad_amd.engine import Engine  # noqa: E402
from professad_amd.ions import ion_ion, ion_ion_cost  # noqa: E402

A_AL = 7.65


def supercell(nions, seed=1, amp=0.02):
    prim = {512: 8, 4096: 16, 32768: 32}
    if nions in prim:
        n = prim[nions]
        box = n * 0.5 * A_AL * np.array([[0.0, 1.0, 1.0], [1.0, 0.0, 1.0], [1.0, 1.0, 0.0]])
        g = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing='ij'), -1).reshape(-1, 3).astype(np.float64)
    else:
        n = round((nions / 4) ** (1.0 / 3.0))
        if 4 * n ** 3 != nions:
            raise SystemExit('ions must be 512, 4096, 32768 or 4 n^3')
        box = n * A_AL * np.eye(3)
        basis = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
        g = (np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing='ij'), -1).reshape(-1, 1, 3) + basis).reshape(-1, 3)
    frac = (g + 0.25 + np.random.default_rng(seed).uniform(-amp, amp, g.shape)) / n
    return box, frac, np.full(g.shape[0], 3.0)


def timed(fn, reps):
    fn()                                   # warm-up: workspaces, first launch
    ts, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ions', type=int, required=True)
    ap.add_argument('--rc', type=float, required=True)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--no-direct', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ionion_cells.jsonl'))
    a = ap.parse_args()
    box, frac, z = supercell(a.ions)
    cost = ion_ion_cost(box, a.ions, a.rc, frac)
    m = cd.choose_cells(box, a.ions)
    counts = np.diff(cd.bin_ions(frac, m)[3])
    rec = dict(ions=a.ions, Rc=cost['Rc'], Rd=cost['Rd'], pairs_estimate=cost['pairs_estimate'],
               direct_candidates=cost['direct_candidates'], cells=list(m), occupancy_mean=float(counts.mean()),
               occupancy_max=int(counts.max()), tile_targets=cd.tile_targets(counts), reps=a.reps)
    eng = Engine((16, 16, 16), 'cuda:0')
    ms, (Ec, Fc, Sc) = timed(lambda: ion_ion(eng, box, frac, z, Rc=a.rc, method='cells', max_pairs=float('inf')), a.reps)
    rec.update(cells_ms=ms, E_per_ion=Ec / a.ions)
    rec.update(cells_pairs_per_s=cost['pairs_estimate'] / (ms * 1e-3))
    if not a.no_direct and cost['direct_candidates'] <= 2e11:
        msd, (Ed, Fd, Sd) = timed(lambda: ion_ion(eng, box, frac, z, Rc=a.rc), a.reps)
        rec.update(direct_ms=msd, direct_pairs_per_s=cost['pairs_estimate'] / (msd * 1e-3),
                   direct_candidates_per_s=cost['direct_candidates'] / (msd * 1e-3),
                   dE_per_ion=abs(Ec - Ed) / a.ions, dF_max=float(np.abs(Fc - Fd).max()), dS_max=float(np.abs(Sc - Sd).max()))
    eng.close()
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'a') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
