"""Cases, direction and term sets of the Hessian-vector goldens (make_golden_hvp.py writes them, tests/test_hvp_cpu.py and
tests/test_hvp_gpu.py read them).  The grid cases are those of cases.py plus `g16d`: g16r's density times 10, whose r_s is
0.87 .. 0.93 -- the r_s < 1 branch of Perdew-Zunger correlation (every case of cases.py sits at r_s = 1.9 .. 2.0, the other one)."""
import numpy as np

import cases

CASES = ['g16r', 'g17r', 'g18t', 'g16d']
S5 = np.sqrt(5.0)
# golden key -> (engine term names, alpha, beta)
TERMS = {
    'ion_electron': (('ion_electron',), None, None), 'hartree': (('hartree',), None, None), 'tf': (('tf',), None, None),
    'vw': (('vw',), None, None), 'wt_nl': (('wt_nl',), 5 / 6, 5 / 6), 'lda_x': (('lda_x',), None, None), 'pz_c': (('pz_c',), None, None),
    'pw_c': (('pw_c',), None, None), 'chachiyo_c': (('chachiyo_c',), None, None),
    'wgc98_nl': (('wt_nl',), (5 + S5) / 6, (5 - S5) / 6),
}
SETS = {
    'cfg1': (('ion_electron', 'hartree', 'tf', 'vw', 'lda_x', 'pz_c'), None, None),
    'cfg2': (('ion_electron', 'hartree', 'tf', 'vw', 'wt_nl', 'lda_x', 'pz_c'), 5 / 6, 5 / 6),
}


def user_stabiliser(x):
    """a Pauli-positivity stabilisation function that is neither 1 + x nor exp (f(0) = 1, f'(0) = 1): golden key `wts_user`,
    WangTeterStyleFunctional((5/6, 5/6, user_stabiliser)) -- T_TF f(T_NL / T_TF) makes the energies' scalar factors depend on the density"""
    return 1 + x + x ** 2


def make_inputs(name):
    """-> box, den, vext (numpy fp64)"""
    box, den, vext, _chi, _n = cases.make_inputs('g16r' if name == 'g16d' else name)
    return box, (den * 10.0 if name == 'g16d' else den), vext


def direction(shape, seed=77):
    return np.random.default_rng(seed).standard_normal(shape) * 0.01


def rs_range(den):
    rs = (3 / (4 * np.pi * den)) ** (1 / 3)
    return float(rs.min()), float(rs.max())
