"""Cases of the truncated-Newton / density-response goldens (make_golden_tn.py writes them, tests/test_tn_cpu.py and
tests/test_tn_gpu.py read them): grids of cases.py, the cfg2 term set of hvp_cases.py with the case's vext."""
import numpy as np

import cases
import hvp_cases

CASES = ['g16r', 'g17r', 'g18t']
TERMS, ALPHA, BETA = hvp_cases.SETS['cfg2']
CHI_SCALE = 1.7          # phi = 1.7 sqrt(den): a scale != 1, so the normalisation path is exercised
DIR_SEED = 81


def make_inputs(case):
    """-> box, phi, d, vext, n_elec"""
    box, den, vext, _chi, n_elec = cases.make_inputs(case)
    return box, CHI_SCALE * np.sqrt(den), hvp_cases.direction(den.shape, seed=DIR_SEED), vext, n_elec


def response_dv(shape):
    """the perturbation of the response goldens: 0.01 cos(2 pi i / n0) + 0.005 sin(2 pi (j / n1 + 2 k / n2)) in grid indices"""
    i, j, k = np.meshgrid(*[np.arange(s) / s for s in shape], indexing='ij')
    return 0.01 * np.cos(2 * np.pi * i) + 0.005 * np.sin(2 * np.pi * (j + 2 * k))
