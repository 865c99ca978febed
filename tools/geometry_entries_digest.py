#!/usr/bin/env python3
"""Digest of every per-geometry-step entry, for a bitwise A/B between two builds of the library.

Loads whichever library OFDFT_LIB selects (default: the tree's own) and prints one JSON line per (case, entry): the SHA-256 of
every output array, OFDFT_Q_LAUNCH_COUNT / OFDFT_Q_FFT_COUNT as a query returns them after the call and, with --profile, the
launches per kernel name the call added (ofdft_profile_get).  Two builds agree when their outputs are equal line for line
(`diff`); the `lib` field is left out of the lines for that reason and goes to the header line alone.

Cases (fp64, the al.gga table of tests/golden/ions.npz, seeded densities):
    c16      16^3 cubic fcc-Al cell, 4 ions shifted off their sites                               (fused pipeline)
    c17      17^3, the same cell                                                                  (chirp-z transforms)
    t18      (18, 20, 16) triclinic cell, two species (1 + 2 ions) whose tables differ in length  (mixed radix)
    c16pme   the three PME-capable entries with pme_order = 4 on c16
    c16ab    ofdft_stress, ofdft_strain_hessian and ofdft_potential_strain_gradient with alpha != beta on c16
    c16wgc   ofdft_stress of hartree + tf + vw + wgc99_nl + pbe_x + pbe_c on c16
    c16nlk   ofdft_stress of hartree + tf + vw + nlk (KGAP, which has a stress) on c16
usage: [OFDFT_LIB=path/to/libofdft_hip.so] geometry_entries_digest.py [--profile] [--out FILE]"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from professad_amd import _native as N  # noqa: E402
from professad_amd import ions, synth  # noqa: E402
from professad_amd.engine import Engine  # noqa: E402

TERMS = ['ion_electron', 'hartree', 'tf', 'vw', 'wt_nl', 'lda_x', 'pz_c']
DEV = 'cuda:0'


def sha(a):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digest(x):
    """SHA-256 of every array in a result: arrays, tensors, floats, and lists / tuples / dicts of them"""
    if isinstance(x, dict):
        return {k: digest(v) for k, v in sorted(x.items())}
    if isinstance(x, (list, tuple)):
        return [digest(v) for v in x]
    return sha(np.float64(x) if isinstance(x, float) else x)


class Run:
    def __init__(self, out, profile):
        self.out, self.profile = out, profile

    def entry(self, case, eng, name, call):
        before = {k: v[1] for k, v in eng.profile().items()} if self.profile else None
        result = call()
        row = dict(case=case, entry=name, sha256=digest(result), launch_count=int(eng.query(N.Q_LAUNCH_COUNT)),
                   fft_count=int(eng.query(N.Q_FFT_COUNT)))
        if self.profile:
            row['launches'] = {k: v[1] - before.get(k, 0) for k, v in sorted(eng.profile().items()) if v[1] != before.get(k, 0)}
        line = json.dumps(row, sort_keys=True)
        print(line, flush=True)
        self.out.write(line + '\n')

    def engine(self, shape, box, names, params=None):
        eng = Engine(shape, DEV).set_cell(box).set_terms(list(names), params)
        if self.profile:
            eng.set_profiling(True)
        return eng


def strain_hessian_entry(eng, den):
    """ofdft_strain_hessian alone (Engine.strain_hessian adds a stress and a product for the pointwise terms)"""
    buf = (C.c_double * (N.NTERMS * 81))()
    eng._check(eng.lib.ofdft_strain_hessian(eng._ctx, C.c_void_p(den.data_ptr()), buf, eng._stream()), 'ofdft_strain_hessian')
    return np.array(list(buf), dtype=np.float64)


def all_entries(run, case, shape, box, species, seed):
    frac = np.concatenate([np.asarray(f, dtype=np.float64).reshape(-1, 3) for f, _t in species])
    z = np.concatenate([np.full(np.asarray(f).reshape(-1, 3).shape[0], float(t[2])) for f, t in species])
    eng = run.engine(shape, box, TERMS)
    den = torch.as_tensor(synth.smooth_density(shape, seed=seed, n0=0.03, amp=0.5), dtype=torch.double, device=DEV)
    for name, call in [
        ('ionic_potential', lambda: ions.ionic_potential(eng, box, species)),
        ('ion_electron_forces', lambda: ions.ion_electron_forces(eng, box, den, species)),
        ('ion_electron_stress', lambda: ions.ion_electron_stress(eng, box, den, species)),
        ('ion_ion', lambda: ions.ion_ion(eng, box, frac, z)),
        ('ion_ion_cells', lambda: ions.ion_ion(eng, box, frac, z, method='cells')),
        ('stress', lambda: eng.stress(den)),
        ('ionic_potential_gradient', lambda: ions.ionic_potential_gradient(eng, box, species, frac.shape[0] - 1)),
        ('ion_electron_curvature', lambda: ions.ion_electron_curvature(eng, box, den, species)),
        ('ion_ion_hessian', lambda: ions.ion_ion_hessian(eng, box, frac, z, range(frac.shape[0]))),
        ('potential_strain_gradient', lambda: eng.potential_strain_gradient(den)),
        ('ionic_potential_strain_gradient', lambda: ions.ionic_potential_strain_gradient(eng, box, species)),
        ('strain_hessian', lambda: strain_hessian_entry(eng, den)),
        ('ion_electron_strain_hessian', lambda: ions.ion_electron_strain_hessian(eng, box, den, species)),
        ('ion_ion_strain_hessian', lambda: ions.ion_ion_strain_hessian(eng, box, frac, z)),
    ]:
        run.entry(case, eng, name, call)
    eng.close()
    return den


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--profile', action='store_true', help='also the launches per kernel name each call added')
    ap.add_argument('--out', default=os.devnull)
    a = ap.parse_args()
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'ions.npz'))
    tab = ions.recpot_table(g['recpot_raw'], float(g['recpot_kmax']))
    tab_short = (tab[0][::2], 0.5 * tab[1][::2], 0.5 * tab[2])       # a second, made-up species: every other table point
    cubic = g['a_box']
    frac4 = g['a_frac'] + 0.02 * np.random.default_rng(5).standard_normal((4, 3))
    tri = cubic[0, 0] * np.array([[1.0, 0.0, 0.0], [0.1, 1.1, 0.0], [0.05, -0.1, 0.9]])
    rng = np.random.default_rng(17)
    two = [(rng.random((1, 3)), tab), (rng.random((2, 3)) * 1.5 - 0.25, tab_short)]      # (also coordinates outside [0, 1))
    one = [(frac4, tab)]
    with open(a.out, 'w') as out:
        print(json.dumps(dict(header='geometry_entries_digest', lib=os.environ.get('OFDFT_LIB') or N.lib_path(), profile=a.profile)),
              flush=True)
        run = Run(out, a.profile)
        den16 = all_entries(run, 'c16', (16, 16, 16), cubic, one, 8)
        all_entries(run, 'c17', (17, 17, 17), cubic, one, 9)
        all_entries(run, 't18', (18, 20, 16), tri, two, 10)
        shape = (16, 16, 16)
        eng = run.engine(shape, cubic, TERMS)
        run.entry('c16pme', eng, 'ionic_potential', lambda: ions.ionic_potential(eng, cubic, one, pme_order=4))
        run.entry('c16pme', eng, 'ion_electron_forces', lambda: ions.ion_electron_forces(eng, cubic, den16, one, pme_order=4))
        run.entry('c16pme', eng, 'ion_electron_stress', lambda: ions.ion_electron_stress(eng, cubic, den16, one, pme_order=4))
        eng.close()
        eng = run.engine(shape, cubic, TERMS, dict(wt_alpha=1.0, wt_beta=2.0 / 3.0))
        run.entry('c16ab', eng, 'stress', lambda: eng.stress(den16))
        run.entry('c16ab', eng, 'strain_hessian', lambda: strain_hessian_entry(eng, den16))
        run.entry('c16ab', eng, 'potential_strain_gradient', lambda: eng.potential_strain_gradient(den16))
        eng.close()
        eng = run.engine(shape, cubic, ['hartree', 'tf', 'vw', 'wgc99_nl', 'pbe_x', 'pbe_c'])
        run.entry('c16wgc', eng, 'stress', lambda: eng.stress(den16))
        eng.close()
        eng = run.engine(shape, cubic, ['hartree', 'tf', 'vw', 'nlk'], dict(nlk_kind=N.NLK_KGAP, nlk_p0=2.0))
        run.entry('c16nlk', eng, 'stress', lambda: eng.stress(den16))
        eng.close()


if __name__ == '__main__':
    main()
