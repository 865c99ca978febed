"""Preconditioned conjugate gradients without a device: the recurrence of tests/pcg_double.py, driven by
optimize.solve_projected / density_response / TruncatedNewton exactly as the device backend is, against the golden response of
tests/golden/tn_g16r.npz and against the plain solver of tests/tn_double.py on the fcc-Al cell of tests/golden/fc_cases.py; and
the host side of the new entry points.

Bounds.  The golden response takes the bounds of tests/test_tn_cpu.py for the plain solve (10 x its MEASURED).  The iteration
counts are bounded by what the preconditioner is for: a quarter of the plain count on the golden, no growth with the grid beyond
three iterations, at most half the plain count of the same problem.  Every test prints its figures before it asserts.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (the oracle closure)

from professad_amd import _native as N
from professad_amd import optimize
from professad_amd.ions import recpot_table

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import cases  # noqa: E402
import fc_cases  # noqa: E402
import fc_double as FD  # noqa: E402
import pcg_double as P  # noqa: E402
import tn_cases  # noqa: E402
import tn_double as T  # noqa: E402

TERMS = list(tn_cases.TERMS)
PLAIN_GOLDEN_ITERS = 153                              # the plain solve of the golden response (tests/test_tn_cpu.py)
BOUND = dict(dn=10 * 2.64e-12, dmu=10 * 1.33e-10)    # tests/test_tn_cpu.py: 10 x MEASURED['dn'], MEASURED['dmu']
E_BOUND_HA = 1e-10
# measured with numpy 2 on x86-64, for the record: golden response 16 iterations, dn 2.7e-12, dmu 1.1e-10;
# Al cell, d v / d R_x of ion 1, rtol 1e-10: 16^3 20 against 92 plain, 24^3 21 against 139; truncated Newton 26 products against 98
MEASURED = dict(golden_iters=16, al16=(20, 92), al24=(21, 139), tn=(26, 98))


def test_golden_response_in_a_quarter_of_the_iterations():
    """dn and dmu of the golden tn_g16r response at rtol 1e-12 within the plain solve's bounds; iterations <= 153 / 4 (measured 16)"""
    g = np.load(os.path.join(HERE, 'golden', 'tn_g16r.npz'))
    box, phi, d, vext, n_elec = tn_cases.make_inputs('g16r')
    assert cases.checksum(box, phi, d, vext) == pytest.approx(float(g['checksum']), rel=1e-12)
    b = P.PcgBackend(box, phi.shape, TERMS)
    r = optimize.density_response(None, g['chi_gs'], n_elec, tn_cases.response_dv(phi.shape), rtol=1e-12, maxiter=500, backend=b)
    ddn = float(np.abs(r['dn'] - g['dn']).max() / np.abs(g['dn']).max())
    dmu = abs(r['dmu'] - float(g['dmu'])) / abs(float(g['dmu']))
    print('MEASURE pcg cpu golden g16r: dn %.2e dmu %.2e iterations %d products %d (plain %d)'
          % (ddn, dmu, r['iterations'], r['hvp_count'], PLAIN_GOLDEN_ITERS))
    assert r['reason'] == optimize.CG_CONVERGED and r['rel_residual'] <= 1e-12
    assert ddn <= BOUND['dn'] and dmu <= BOUND['dmu']
    assert r['iterations'] <= PLAIN_GOLDEN_ITERS // 4 and r['hvp_count'] == r['iterations']
    assert abs(r['dn'].sum()) <= 1e-14 * np.abs(r['dn']).sum()


def al_cell(n):
    """the fcc-Al cell with the a16 ions of fc_cases and the real recpot on an n^3 grid -> backend pieces"""
    box, _shape, frac, _den, raw, k_max = fc_cases.make_inputs('a16')
    tab = recpot_table(raw, k_max)
    n_elec = 4 * float(tab[2])
    return box, (n, n, n), frac, tab, n_elec


def relax(fc, cg, chi, n_elec):
    """truncated Newton with the oracle closure of `fc` and the solver `cg`, in place -> the optimiser"""
    tn = optimize.TruncatedNewton(chi, cg, n_elec)
    for _outer in range(12):
        before = tn.total_iter
        tn.step(lambda: fc.closure(chi, n_elec))
        if tn.total_iter == before:
            break
    return tn


@pytest.fixture(scope='module')
def al16():
    """plain and preconditioned truncated Newton from the uniform density at 16^3; run once"""
    box, shape, frac, tab, n_elec = al_cell(16)
    fc = FD.NumpyFcBackend(box, shape, [(frac, tab)], TERMS)
    out = {}
    for name, cg in (('plain', fc.cg), ('pre', P.PcgBackend(box, shape, TERMS))):
        chi = np.full(shape, np.sqrt(n_elec / abs(np.linalg.det(box))))
        tn = relax(fc, cg, chi, n_elec)
        out[name] = (chi, tn)
    return box, shape, frac, tab, n_elec, fc, out


def response_counts(box, shape, frac, tab, n_elec, chi):
    dv = FD.potential_gradient(box, shape, (frac @ box)[1], tab)[0]
    res = {}
    for name, cg in (('plain', T.NumpyCgBackend(box, shape, TERMS)), ('pre', P.PcgBackend(box, shape, TERMS))):
        res[name] = optimize.density_response(None, chi, n_elec, dv, rtol=1e-10, maxiter=500, backend=cg)
        assert res[name]['reason'] == optimize.CG_CONVERGED and res[name]['rel_residual'] <= 1e-10
    scale = np.abs(res['plain']['dn']).max()
    return res['pre']['iterations'], res['plain']['iterations'], float(np.abs(res['pre']['dn'] - res['plain']['dn']).max() / scale)


def test_iteration_count_does_not_grow_with_the_grid(al16):
    """the response to d v / d R_x of ion 1 at the ground states of 16^3 and 24^3, rtol 1e-10: the preconditioned count at 24^3 is at
    most that at 16^3 + 3, and both are at most half the plain count of the same problem (measured 20 and 21 against 92 and 139)"""
    box, shape, frac, tab, n_elec, _fc, out = al16
    it16, plain16, d16 = response_counts(box, shape, frac, tab, n_elec, out['plain'][0])
    box, shape24, frac, tab, n_elec = al_cell(24)
    fc = FD.NumpyFcBackend(box, shape24, [(frac, tab)], TERMS)
    chi = np.full(shape24, np.sqrt(n_elec / abs(np.linalg.det(box))))
    relax(fc, fc.cg, chi, n_elec)
    it24, plain24, d24 = response_counts(box, shape24, frac, tab, n_elec, chi)
    print('MEASURE pcg cpu Al response: 16^3 %d (plain %d, dn apart %.1e)  24^3 %d (plain %d, dn apart %.1e)'
          % (it16, plain16, d16, it24, plain24, d24))
    assert it24 <= it16 + 3
    assert 2 * it16 <= plain16 and 2 * it24 <= plain24
    # two solves of one system, each to |r| <= 1e-10 |b|: apart by at most 2 rtol cond(H), and cond(H) < 1e3 here (plain CG needs
    # ~ sqrt(cond) ln(2 / rtol) / 2 iterations: 139 gives cond ~ 140)
    assert max(d16, d24) <= 2e-7


def test_truncated_newton_takes_fewer_products_to_the_same_energy(al16):
    """from the uniform density at 16^3: the same energy within 1e-10 Ha, at most 40 products and at most half the plain run's
    (measured 26 against 98)"""
    _box, _shape, _frac, _tab, _n_elec, _fc, out = al16
    (_c0, plain), (_c1, pre) = out['plain'], out['pre']
    dE = pre._at[0] - plain._at[0]
    print('MEASURE pcg cpu Al TN 16^3: products %d (plain %d) outer %d (plain %d) E - E_plain %.2e Ha |g|_2 %.1e (plain %.1e)'
          % (pre.hvp_count, plain.hvp_count, pre.total_iter, plain.total_iter, dE, np.linalg.norm(pre._at[1]), np.linalg.norm(plain._at[1])))
    assert np.linalg.norm(pre._at[1]) <= 1e-10 and np.linalg.norm(plain._at[1]) <= 1e-10
    assert abs(dE) <= E_BOUND_HA
    assert pre.hvp_count <= 40 and 2 * pre.hvp_count <= plain.hvp_count


def test_recurrence_exits():
    """the exits of the preconditioned recurrence as solve_projected reports them (a 2 x 2 x 2 grid, made-up operator and preconditioner)"""
    phi = np.ones((2, 2, 2))
    b = np.arange(8.0).reshape(2, 2, 2) - 3.5
    m = np.linspace(2, 1, 8).reshape(2, 2, 2)
    x, it, reason, rel, nprod = optimize.solve_projected(P.DiagPcgBackend(np.linspace(1, 2, 8).reshape(2, 2, 2), m), phi, None, b, 1.0, 1e-12, 2)
    assert (it, reason, nprod) == (2, optimize.CG_MAXITER, 2) and rel > 1e-12
    x, it, reason, rel, nprod = optimize.solve_projected(P.DiagPcgBackend(-np.ones((2, 2, 2)), m), phi, None, b, 1.0, 1e-12, 50)
    z = b / m
    assert (it, reason, nprod) == (0, optimize.CG_CURVATURE, 1) and np.allclose(x, z - z.mean(), rtol=0, atol=1e-15)      # x = p = P z
    x, it, reason, rel, nprod = optimize.solve_projected(P.DiagPcgBackend(np.ones((2, 2, 2)), np.ones((2, 2, 2))), phi, None, b, 1.0, 1e-12, 50)
    assert (it, reason) == (1, optimize.CG_CONVERGED) and np.allclose(x, b, rtol=0, atol=1e-15)
    # the plain numpy backend is driven as before
    x, it, reason, rel, nprod = optimize.solve_projected(T.DiagCgBackend(np.ones((2, 2, 2))), phi, None, b, 1.0, 1e-12, 50)
    assert (it, reason) == (1, optimize.CG_CONVERGED)


def test_precondition_argument_is_checked_before_any_device_work():
    for bad in (0.0, -1.0, float('nan'), float('inf'), 'on', True):
        with pytest.raises(ValueError, match='precondition'):
            optimize.check_precondition(bad)
    assert optimize.check_precondition(None) is None and optimize.check_precondition('auto') == 'auto'
    assert optimize.check_precondition(2) == 2.0
    assert optimize.kinetic_kappa2(12.0, 500.0) == pytest.approx(P.kappa2_auto(12.0, 500.0), rel=1e-15)
    with pytest.raises(ValueError, match='tn_precondition'):
        optimize.optimize_density(None, 8.0, n_method='LBFGS', tn_precondition='auto')
    with pytest.raises(ValueError, match='backend'):
        optimize.density_response(None, None, 8.0, None, backend=object(), precondition='auto')


@pytest.mark.parametrize('dtype', [N.F64, N.F32])
def test_entry_points_are_exported_and_refuse_null_handles(dtype):
    """both libraries export the four entries and refuse null handles; where this machine has a device, ofdft_cg_direction on a handle
    in plain mode is OFDFT_ESTATE (tests/test_pcg_gpu.py asserts that unconditionally)"""
    lib = N.load(dtype)
    for sym in ('ofdft_precondition', 'ofdft_cg_set_preconditioned', 'ofdft_cg_z', 'ofdft_cg_direction'):
        assert sym in N.EXPORTS and hasattr(lib, sym)
    reason, z = ctypes.c_int(0), ctypes.c_void_p(0)
    assert lib.ofdft_precondition(None, None, None, 1.0, None) == N.EINVAL
    assert lib.ofdft_cg_set_preconditioned(None, 1) == N.EINVAL
    assert lib.ofdft_cg_z(None, ctypes.byref(z)) == N.EINVAL
    assert lib.ofdft_cg_direction(None, None, None, ctypes.byref(reason), None) == N.EINVAL
    h = ctypes.c_void_p(0)
    if lib.ofdft_cg_create(ctypes.byref(h), 8, 0) == N.OK:          # (needs a device for its vectors)
        try:
            x = (ctypes.c_double * 8)()
            assert lib.ofdft_cg_direction(h, x, None, ctypes.byref(reason), None) == N.ESTATE
        finally:
            lib.ofdft_cg_destroy(h)
