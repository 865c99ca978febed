"""Cases of the force-constant goldens (make_golden_fc.py writes them, tests/test_force_constants_cpu.py and
tests/test_force_constants_gpu.py read them): the two ion sets of ions.npz with its al.gga recpot table.
  b    the triclinic cell, 16 x 20 x 24, 7 random ions
  a16  the fcc-Al conventional cell, 16^3, its four ions each shifted by 0.02 standard normals in fractional coordinates, so that
       no symmetry hides an error -- also the end-to-end case of the force-constant tests
"""
import os

import numpy as np

from professad_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ['b', 'a16']
ION = {'b': 3, 'a16': 1}                       # the ion whose potential gradient is stored
SHAPE = {'b': (16, 20, 24), 'a16': (16, 16, 16)}
DEN = {'b': dict(seed=7, n0=0.05, amp=0.5), 'a16': dict(seed=8, n0=0.03, amp=0.5)}


def make_inputs(case):
    """-> box, shape, frac, den (a seeded positive density), raw recpot table, k_max"""
    g = np.load(os.path.join(HERE, 'ions.npz'))
    shape = SHAPE[case]
    if case == 'b':
        box, frac = g['b_box'], g['b_frac']
    else:
        box = g['a_box']
        frac = g['a_frac'] + 0.02 * np.random.default_rng(5).standard_normal((4, 3))
    den = synth.smooth_density(shape, **DEN[case])
    return box, shape, frac, den, g['recpot_raw'], float(g['recpot_kmax'])
