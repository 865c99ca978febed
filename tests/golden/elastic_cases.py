"""Cases of the strain-Hessian goldens (make_golden_elastic.py writes them, tests/test_elastic_cpu.py and
tests/test_elastic_gpu.py read them): the inputs of fc_cases.make_inputs --
  b    the triclinic cell, 16 x 20 x 24, 7 random ions
  a16  the fcc-Al conventional cell, 16^3, its four ions off their sites
with chi = sqrt(den) of the seeded density as the fixed grid values, N = mean(den) vol.
Stored per case: w2_<term> [3, 3, 3, 3] for the TERMS below, b_sum / w1_sum / cfix4 / stress_sum of the SUMMED set, the input checksum;
for a16 also b_<term> of the EXPLICIT terms (elastic_a16_b.npz); and w2_<grid>_<term> on the GRIDS at the end (elastic_grids.npz).
"""
import os

import numpy as np

import cases
import fc_cases
from professad_amd import synth

CASES = fc_cases.CASES
make_inputs = fc_cases.make_inputs
AB2 = (0.7, 0.9)                     # the alpha != beta instance of non_local_KEF
# golden key -> (engine term, (alpha, beta) or None)
TERMS = {'ion_electron': ('ion_electron', None), 'hartree': ('hartree', None), 'tf': ('tf', None), 'vw': ('vw', None),
         'wt_nl': ('wt_nl', (5 / 6, 5 / 6)), 'nl_0709': ('wt_nl', AB2), 'lda_x': ('lda_x', None), 'pz_c': ('pz_c', None),
         'pw_c': ('pw_c', None), 'chachiyo_c': ('chachiyo_c', None)}
VOIGT = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))
SUMMED = ('ion_electron', 'hartree', 'tf', 'vw', 'wt_nl', 'lda_x', 'pz_c')      # the seven-term set of the end-to-end tests
EXPLICIT = ('ion_electron', 'hartree', 'vw', 'wt_nl')                          # terms whose potential depends on the cell explicitly


# grids without a full golden: the chirp-z, mixed-radix and power-of-two transform families, and two grids with an odd last extent
# and more k-points than one trip of the moment kernels' block loops.  Stored in elastic_grids.npz: w2_<grid>_<term>.
GRIDS = {'g17': ((17, 17, 17), ('cubic', 17)), 'g48t': ((48, 16, 16), ('tri', 1.0)), 'g32x': ((32, 16, 64), ('cubic', 32)),
         'g20t': ((20, 18, 33), ('tri', 1.0)), 'g33': ((32, 32, 33), ('cubic', 32))}
GRID_TERMS = ('ion_electron', 'hartree', 'tf', 'vw', 'wt_nl', 'lda_x', 'pw_c')
SPECIES_SEED = 17


def grid_inputs(name):
    """-> box, shape, den, [(frac, potential scale)]: three ions of two species, the second with half the potential of the
    recpot table of ions.npz (the ions of tests/fc_double.two_species), coordinates partly outside [0, 1)"""
    shape, cell = GRIDS[name]
    rng = np.random.default_rng(SPECIES_SEED)
    ions_ = [(rng.random((1, 3)), 1.0), (rng.random((2, 3)) * 1.5 - 0.25, 0.5)]
    return cases.make_cell(cell), shape, synth.smooth_density(shape, seed=23, n0=0.04, amp=0.4), ions_


def recpot():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'ions.npz'))
    return g['recpot_raw'], float(g['recpot_kmax'])
