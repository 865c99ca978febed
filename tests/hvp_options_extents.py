"""Inputs and numpy doubles of the Hessian-vector products of WGC99 + PBE (OFDFT_OPT_HVP_WGC = OFDFT_OPT_HVP_GGA = 1) on the two
grids past the block caps of tests/test_second_order_extents_gpu.py, shared by tests/test_hvp_options_extents_gpu.py (the device
against the double) and tests/test_hvp_vacuum_cpu.py (the double against itself in long double: the yardstick):

  A = (128, 128, 64) in synth.cubic_cell(128): 524 288 pairs, exactly the 2048 x 256 of the WGC99 head and twice the 1024-block cap
      of the reducing kernels (hvp_gga_mid_kernel, hvp_wgc_tail_kernel, hvp_combine_kernel).  N = 957.81.
  B = (81, 81, 81) in synth.cubic_cell(81): 531 441 points, odd (block 0 / thread 0 patches the last one), the chirp-z transforms.
      N = 242.73.
The inputs are those of that test unchanged: synth.random_density(seed=11), hvp_cases.direction with seeds 78 / 83 / 84, phi = 0.6
sqrt(den), the made-up gradient made perpendicular to phi.  The doubles are tests/hvp_wgc_double.py's, which is generic in dtype
(numpy's FFT keeps longdouble).  Not the product: nothing in professad_amd imports it.
"""
import numpy as np

import hvp_cases
import hvp_wgc_cases as G
import hvp_wgc_double as W
from professad_amd import synth

SHAPES = {'A': (128, 128, 64), 'B': (81, 81, 81)}
CFG3W = G.CFG3W
# the term sets the n-space test runs: the bench set, and each new stage alone (its own field and sum, not hidden in the other's rounding)
SETS = {'cfg3w': CFG3W, 'wgc99_nl': ('wgc99_nl',), 'pbe': ('pbe_x', 'pbe_c')}
_IN = {}


def inputs(key):
    """box, density, directions and the made-up gradient perpendicular to phi of a shape, made once"""
    if key not in _IN:
        shape = SHAPES[key]
        box = synth.cubic_cell(shape[0])
        den = synth.random_density(shape, seed=11)
        phi = 0.6 * np.sqrt(den)
        vol = abs(np.linalg.det(box))
        nel = float(den.mean() * vol)
        assert abs(nel % 1.0 - 0.5) >= G.HALF_INTEGER_MARGIN, nel          # round(N) is a constant of the differentiation
        gr = hvp_cases.direction(shape, seed=84)
        gr -= phi * (phi * gr).sum() / (phi * phi).sum()
        _IN[key] = dict(box=box, shape=shape, den=den, phi=phi, n_elec=float(den.sum() * vol / den.size), dV=vol / den.size,
                        w=hvp_cases.direction(shape, seed=78), d=hvp_cases.direction(shape, seed=83), gr=gr)
    return _IN[key]


def per_term(key, dtype=np.float64):
    """-> {term: (q_t, hv_t)} of cfg3w's terms in n space, each computed once, in `dtype`"""
    i = inputs(key)
    den, w = i['den'].astype(dtype), i['w'].astype(dtype)
    out = {}
    for t in CFG3W:
        q, hv = W.hessian_vector(i['box'], den, w, (t,))
        out[t] = (q[t], hv)
    return out


def set_product(terms, names):
    """(dict term -> q_t, hv) of a term set from per_term's result, summed in the order hvp_wgc_double.hessian_vector sums"""
    order = [t for t in names if t != 'wgc99_nl'] + [t for t in names if t == 'wgc99_nl']
    hv = np.zeros_like(terms[order[0]][1])
    for t in order:
        hv = hv + terms[t][1]
    return {t: terms[t][0] for t in names}, hv


def chi_product(key, dtype=np.float64, sign=None):
    """hvp_wgc_double.hessian_vector_chi of cfg3w in `dtype`; `sign`: +-1 per point on phi, d and g"""
    i = inputs(key)
    s = 1.0 if sign is None else sign
    return W.hessian_vector_chi(i['box'], (s * i['phi']).astype(dtype), (s * i['d']).astype(dtype), (s * i['gr']).astype(dtype), i['n_elec'], CFG3W)


def signs(shape):
    """+-1 per point, about half of them negative (those of tests/test_second_order_extents_gpu.py)"""
    return np.where(np.random.default_rng(85).random(shape) < 0.5, -1.0, 1.0)


def q_floor(w, hv_t, dV, q_t):
    """ten roundings of the terms of q_t = sum w hv_t dV, relative to |q_t| (tests/test_hvp_wgc_gpu.py)"""
    return 10 * 2.0 ** -52 * float(np.abs(w * hv_t).sum() * dV) / abs(q_t)


def hv_figures(q, hv, qd, hvd):
    """hv by max|. - double| / max|double|; every q_t by |q_t - double| / |double| (tests/test_second_order_extents_gpu.py)"""
    fig = dict(hv=float(np.abs(hv - hvd).max() / np.abs(hvd).max()))
    for t, v in qd.items():
        if t != 'ion_electron':
            fig['q_' + t] = float(abs(q[t] - v) / abs(v))
    return fig


def chi_figures(s, Hd, sd, Hdd, phi, d):
    """H d by max|.| / max|double|, d.H d and phi.H d relative to sum|d H d| and sum|phi H d|, d mu relative to itself"""
    return dict(Hd=float(np.abs(Hd - Hdd).max() / np.abs(Hdd).max()),
                dHd=float(abs(s['dHd'] - sd['dHd']) / np.abs(d * Hdd).sum()),
                phiHd=float(abs(s['phiHd'] - sd['phiHd']) / np.abs(phi * Hdd).sum()),
                dmu=float(abs(s['dmu'] - sd['dmu']) / abs(sd['dmu'])))



def cg_solve(key, backend, cast=lambda a: a, maxiter=3):
    """optimize.solve_projected(backend, phi, None, rhs, N, 1e-30, maxiter) with rhs as optimize.density_response forms it from
    tn_cases.response_dv; `cast` takes the numpy inputs to what the backend works on -> (x, iterations, reason, residual, products)"""
    import tn_cases
    import tn_double as T
    from professad_amd import optimize
    i = inputs(key)
    phi, dV, n_elec = i['phi'], i['dV'], i['n_elec']
    dv = tn_cases.response_dv(i['shape'])
    S, c, n = T.density(i['box'], phi, n_elec)
    rhs = (-2.0 * c * dV) * phi * (dv - float((dv * n).sum()) * dV / n_elec)
    return optimize.solve_projected(backend, cast(phi), None, cast(rhs), n_elec, 1e-30, maxiter)


def numpy_cg(key, dtype=np.float64):
    """cg_solve on hvp_wgc_double.NumpyCgBackend in `dtype`"""
    i = inputs(key)
    return cg_solve(key, W.NumpyCgBackend(i['box'], i['shape'], CFG3W), lambda a: a.astype(dtype))
