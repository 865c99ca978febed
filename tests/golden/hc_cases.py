"""Cases and parameters of the Huang-Carter goldens (make_golden_hc.py writes them, tests/test_hc_cpu.py and
tests/test_hc_gpu.py read them).  The grid cases are those of cases.py plus `g16w`: g16r's density made wide,
n_mean exp(2 u) with u = (n - n_mean) / (max n - min n), rescaled to g16r's mean -- its xi spans many spline intervals
(HC: 1.74 .. 723, 40 nodes, 34 intervals touched) where the plain cases touch three."""
import numpy as np

import cases

CASES = ['g16r', 'g17r', 'g18t', 'g16w']
# golden key -> (reference class name, init_args, engine parameters of the nonlocal term)
HC_ARGS = (0.01177, 0.7143, 1.2)
REVHC_ARGS = (0.45, 0.10, 2 / 3, 1.15)
KINDS = {
    'hc': ('HuangCarter', HC_ARGS, dict(nlk_kind=4, nlk_p0=HC_ARGS[0], nlk_p1=HC_ARGS[1], nlk_p2=HC_ARGS[2])),
    'revhc': ('RevisedHuangCarter', REVHC_ARGS,
              dict(nlk_kind=5, nlk_p0=REVHC_ARGS[0], nlk_p1=REVHC_ARGS[1], nlk_p2=REVHC_ARGS[2], nlk_p3=REVHC_ARGS[3])),
}
ETA_MAX, N_ETA = 50.0, 10000


def beta_of(key):
    return KINDS[key][1][1] if key == 'hc' else KINDS[key][1][2]


def kappa_of(key):
    return KINDS[key][1][-1]


def make_inputs(name):
    """-> box, den (numpy fp64)"""
    box, den, _vext, _chi, _n = cases.make_inputs('g16r' if name == 'g16w' else name)
    if name == 'g16w':
        u = (den - den.mean()) / (den.max() - den.min())
        wide = den.mean() * np.exp(2.0 * u)
        den = wide * (den.mean() / wide.mean())
    return box, den


def node_set(xi_min, xi_max, kappa):
    """(lower, M, the two ceil arguments) of field_dependent_convolution's geometric mode (functional_tools.py:415-417)"""
    a = -np.log(xi_min) / np.log(kappa)
    lower = kappa ** (-(np.ceil(a) + 3))
    b = np.log((xi_max + 1) / lower) / np.log(kappa)
    return float(lower), int(np.ceil(b) + 3), float(a), float(b)
