"""CPU tests of the numpy doubles where tests/test_second_order_extents_gpu.py and tests/test_cg_sweeps_gpu.py lean on them without a
golden: fc_double.ion_electron_curvature on grids with an odd last extent (against central differences of
fc_double.ion_electron_forces), the sign-flip identity of tn_double.hessian_vector_chi, and tn_double.DiagCgBackend (the made-up
diagonal operator and the re-seeding of one step).  No GPU anywhere; every test prints its figures as `MEASURE ...` before it asserts.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import cases  # noqa: E402
import fc_double as FD  # noqa: E402
import hvp_cases  # noqa: E402
import tn_cases  # noqa: E402
import tn_double as T  # noqa: E402
from professad_amd import optimize, synth  # noqa: E402

# Central difference of the forces at step h = 1e-4 bohr: truncation h^2 |F'''| / 6, independent of any device; measured 4.8e-9, 4.5e-9
# and 1.2e-8 of max|D| on (17, 17, 17), (20, 18, 33) and (32, 32, 33).  An error in the closed form is of order one.
CURVATURE_FD_BOUND = 1e-7
FD_STEP = 1e-4


@pytest.mark.parametrize('shape,cell', [((17, 17, 17), ('cubic', 17)), ((20, 18, 33), ('tri', 1.0)), ((32, 32, 33), ('tri', 1.0))])
def test_curvature_double_is_the_derivative_of_the_forces_on_odd_grids(shape, cell):
    """D[a][:, j] against -(F_a(R + h e_j) - F_a(R - h e_j)) / (2 h) for every ion and Cartesian direction, with the two species of
    tests/test_second_order_extents_gpu.py (fc_double.two_species)."""
    box = cases.make_cell(cell)
    inv = np.linalg.inv(box)
    den = synth.smooth_density(shape, seed=7, n0=0.05, amp=0.5)
    worst = scale = 0.0
    for frac, tab in FD.two_species(sum(shape)):
        D = FD.ion_electron_curvature(box, den, frac, tab)
        assert np.allclose(D, D.transpose(0, 2, 1), rtol=0, atol=1e-15 * np.abs(D).max())
        scale = max(scale, float(np.abs(D).max()))
        for a in range(frac.shape[0]):
            for j in range(3):
                F = {}
                for sign in (+1, -1):
                    cart = frac @ box
                    cart[a, j] += sign * FD_STEP
                    F[sign] = FD.ion_electron_forces(box, den, cart @ inv, tab)
                fd = -(F[+1] - F[-1]) / (2 * FD_STEP)
                worst = max(worst, float(np.abs(fd[a] - D[a, :, j]).max()))
    print('MEASURE curvature double %s: central difference %.2e of max|D| = %.3e' % (shape, worst / scale, scale))
    assert worst <= CURVATURE_FD_BOUND * scale


def test_sign_flip_identity_is_exact_in_the_double():
    """g17r: the closure is even in every chi_j, so with s = +-1 per point hessian_vector_chi(s phi, s d, s g) - s * hessian_vector_chi(phi,
    d, g) is exactly 0.0 and the scalars are the same numbers: every sign cancels in n, dn, a, S and in the three terms of H d."""
    box, phi, d, _vext, n_elec = tn_cases.make_inputs('g17r')
    gr = hvp_cases.direction(phi.shape, seed=84)
    gr -= phi * (phi * gr).sum() / (phi * phi).sum()
    s = np.where(np.random.default_rng(85).random(phi.shape) < 0.5, -1.0, 1.0)
    assert 0.4 < (s < 0).mean() < 0.6
    s0, H0 = T.hessian_vector_chi(box, phi, d, gr, n_elec, tn_cases.TERMS)
    s1, H1 = T.hessian_vector_chi(box, s * phi, s * d, s * gr, n_elec, tn_cases.TERMS)
    diff = float(np.abs(H1 - s * H0).max())
    print('MEASURE sign flip g17r: max|H(s phi, s d, s g) - s H(phi, d, g)| = %.1e' % diff)
    assert diff == 0.0
    assert s0 == s1


def test_diagonal_backend_solves_and_reseeds():
    """tn_double.DiagCgBackend: with phi an eigenvector of the operator (h constant where phi lives) the solution is the
    projected b over h, within 2 (rtol + 64 eps per iteration) |b_p|_2 (the spectrum of P H P on the complement of phi lies in
    [0.5, 1.5]); a step taken after `seed` with the state of a running solve is that solve's own step, bit for bit."""
    n, rtol = 513, 1e-10
    phi, b, h = T.diag_inputs(n, 1)
    m = (n + 1) // 2
    phi[m:] = 0.0
    h[:m] = 0.8125
    x, it, reason, rel, nprod = optimize.solve_projected(T.DiagCgBackend(h), phi, None, b, 1.0, rtol, 200)
    bp = b - phi * ((phi * b).sum() / (phi * phi).sum())
    dev = float(np.linalg.norm(x - bp / h) / np.linalg.norm(bp))
    print('MEASURE diagonal backend: |x - b_p / h|_2 / |b_p|_2 %.2e after %d iterations' % (dev, it))
    assert (reason, nprod) == (T.CG_CONVERGED, it) and rel <= rtol and 1 < it < 200
    assert dev <= 2.0 * (rtol + 64 * 2.0 ** -52 * it)
    phi, b, h = T.diag_inputs(n, 2)
    run, twin = T.DiagCgBackend(h), T.DiagCgBackend(h)
    run.start(phi, b, 0.0, 50)
    for k in range(3):
        pq, phiq = run.product(phi, None, 1.0, k > 0)
        twin.seed(run.x, run.r, run.p, run.q, run.S, run.bb, run.rr, run.iters)
        assert run.step(phi, pq, phiq) == twin.step(phi, pq, phiq) == T.CG_RUNNING
        assert np.array_equal(run.x, twin.x) and np.array_equal(run.r, twin.r) and np.array_equal(run.p, twin.p)
        assert (run.rr, run.iters) == (twin.rr, twin.iters)
