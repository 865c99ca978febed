"""Interatomic force constants from the ground-state density response.

`force_constants` stands behind the reference's `System.force_constants(primitive_ion_indices)` (src/professad/system.py:695-717,
1340-1367), which differentiates the forces at the relaxed density once more by autograd through xitorch's minimiser.  Here the
implicit derivative is explicit: with F = -dE_tot/dR at the ground state and E_tot = E[n] + E_ion-ion,

    Phi[p, b, i, j] = -dF[p, i] / dR[b, j] = Phi_ii[p, b, i, j] + delta_pb D[p, i, j] - F_ie[dn_(p, i)][b, j]

where dn_(p, i) is `optimize.density_response` to dv = d v_ext / d R_{p, i} (`ofdft_ionic_potential_gradient`), F_ie the
ion-electron force entry (linear in the density: it takes dn as it is), D the ion-electron curvature at fixed density
(`ofdft_ion_electron_curvature`) and Phi_ii the ion-ion Hessian (`ofdft_ion_ion_hessian`).  Phi is symmetric, so the 3 P solves
for the displaced primitive ions give every requested row.  Single GPU, fp64, exact structure factor.
"""
import numpy as np

from . import ions, optimize
from .optimize import A_PER_BOHR


class HipFcBackend(optimize.HipResponseBackend):
    """What `force_constants` needs, on the device: the pieces from professad_amd.ions on top of optimize.HipResponseBackend
    (the conjugate gradients, the ground-state check).  The small per-ion results are numpy arrays."""

    def potential_gradient(self, ion):
        return ions.ionic_potential_gradient(self.eng, self.box, self.species, ion)

    def ion_electron_forces(self, den):
        return np.concatenate(ions.ion_electron_forces(self.eng, self.box, den, self.species), axis=0)

    def ion_electron_curvature(self, den):
        return np.concatenate(ions.ion_electron_curvature(self.eng, self.box, den, self.species), axis=0)

    def ion_ion_hessian(self, frac, charges, rows, Rc):
        return ions.ion_ion_hessian(self.eng, self.box, frac, charges, rows, Rc)


def refusal(engine, pme_order=None):
    """None, or why `force_constants` cannot run on this engine (raised before any device work)"""
    return optimize.response_refusal(engine, pme_order)


def batch_refusal(engine):
    """None, or why `force_constants(batch=k)` cannot run where `batch=None` can: with the engine's OPT_HVP_GGA at 1 pbe_x / pbe_c pass
    the single-column solves (with its OPT_HVP_WGC at 1, wgc99_nl), and the batched ones keep refusing them by name"""
    return optimize.second_order_refusal(engine, gga_missing='batch')


def force_constants(engine, box_vecs, species, chi, primitive_ion_indices=None, Rc=None, rtol=1e-10, maxiter=500, units='Ha/b2',
                    impose_asr=False, backend=None, pme_order=None, precondition=None, batch=None):
    """Phi[p, b, i, j] = -dF[p, i] / dR[b, j] for p in `primitive_ion_indices` (default: every ion) and all ions b.

    engine: a single-GPU fp64 `Engine` with the caller's term set (it includes ion_electron) on the cell `box_vecs`.
    species: iterable of (frac_coords [n, 3], (ks, v, z)) per ion type, as `ions.ionic_potential` takes it; the global ion index
    is the position in the concatenation of the species, and n_elec = sum z.  chi: a ground state of these terms in the
    potential of these ions, e.g. `optimize_density(..., n_method='TN')['chi']` (any scale).  Rc: the ion-ion cutoff (`ions.ion_ion`).
    rtol, maxiter: of the 3 P conjugate-gradient solves.  units: 'Ha/b2' or 'eV/a2' (system.py:712-717).

    Returns a dict: `phi` [P, N, 3, 3]; `parts` with `ion_ion`, `direct` and `response` (they sum to `phi` before `impose_asr`);
    `iterations`, `rel_residual`, `reason` (lists over the 3 P solves, p-major) and `hvp_count`; `asr_residual` =
    max|sum_b Phi[p, b]| / max|Phi| -- the acoustic sum rule holds only as far as the fixed grid is translation invariant (the
    pointwise nonlinear terms alias: about 1e-3 at 16^3 for fcc Al), so this is reported, and `impose_asr=True` restores it by
    correcting the diagonal block with the row sum; `ground_state_gradient` = max|g| / dV of the closure at `chi`.
    A solve that ends for another reason than convergence raises a warning: unpreconditioned, the iteration count of the conjugate
    gradients grows with the grid (about 100 at 16^3, 400 at 64^3 for fcc Al), so larger grids need a larger `maxiter` -- or
    `precondition`: None, 'auto' or kappa^2 > 0 (`optimize.HipCgBackend`), the kinetic preconditioner, about 20 iterations at any grid.
    `batch`: None, or 1 .. 8: the 3 P right-hand sides, in the same p-major order, go `batch` columns at a time through batched
    solves (`optimize.density_response_multi`).  The returned dict is the same, `hvp_count` then counting batched
    products.  With `backend` given, `batch` is that backend's own attribute, as `precondition` is.

    NotImplementedError, before any device work and naming the cause: PME, a slab-decomposed engine, an fp32 engine, a term
    without a second derivative.  (`backend`: an object with HipFcBackend's methods -- the tests' numpy double.)"""
    if units not in ('Ha/b2', 'eV/a2'):
        raise ValueError("Parameter 'units' can only be 'Ha/b2' or 'eV/a2'")                       # system.py:717
    species, frac, charges = optimize.normalise_species(species)
    nions = frac.shape[0]
    rows = list(range(nions)) if primitive_ion_indices is None else [int(p) for p in primitive_ion_indices]
    if not rows or min(rows) < 0 or max(rows) >= nions:
        raise ValueError('primitive_ion_indices must name at least one ion, each in [0, %d)' % nions)
    optimize._own_backend_only('force_constants', backend, precondition)
    optimize.check_precondition(precondition)
    batch = optimize.resolve_batch('force_constants', backend, batch)
    if backend is None:
        why = refusal(engine, pme_order) or (batch_refusal(engine) if batch is not None else None)
        if why:
            raise NotImplementedError('force_constants: ' + why)
    b = backend if backend is not None else HipFcBackend(engine, box_vecs, species)
    try:
        if precondition is not None:
            b.cg.set_precondition(precondition)
        n_elec = float(charges.sum())
        S = float((chi * chi).sum())
        n = (n_elec / (S * b.dV)) * chi * chi
        gsg = b.ground_state_gradient(chi, n_elec)
        ion_ion = b.ion_ion_hessian(frac, charges, rows, Rc)
        D = b.ion_electron_curvature(n)
        direct = np.zeros_like(ion_ion)
        response = np.zeros_like(ion_ion)
        log = optimize.new_solve_log()
        if batch is None:
            for q, p in enumerate(rows):
                direct[q, p] = D[p]
                dv = b.potential_gradient(p)
                for i in range(3):
                    r = optimize.density_response(engine, chi, n_elec, dv[i], rtol=rtol, maxiter=maxiter, backend=b.cg)
                    response[q, :, i, :] = -b.ion_electron_forces(r['dn'])
                    optimize.log_solve(log, r)
        else:               # the same 3 P right-hand sides in the same order, `batch` columns per solve, across ions
            dvs = []
            for q, p in enumerate(rows):
                direct[q, p] = D[p]
                dv = b.potential_gradient(p)
                dvs.extend(dv[i] for i in range(3))
            for k, r in enumerate(optimize.batched_responses(b, engine, chi, n_elec, dvs, batch, rtol, maxiter)):
                response[k // 3, :, k % 3, :] = -b.ion_electron_forces(r['dn'])
                optimize.log_solve(log, r)
    finally:
        if backend is None:
            b.close()
    optimize.warn_unconverged('force_constants', log, maxiter, 'the matrix is not accurate')
    parts = dict(ion_ion=ion_ion, direct=direct, response=response)
    phi = ion_ion + direct + response
    row_sum = phi.sum(axis=1)
    asr = float(np.abs(row_sum).max() / np.abs(phi).max())
    if impose_asr:
        for q, p in enumerate(rows):
            phi[q, p] -= row_sum[q]
    if units == 'eV/a2':
        f = optimize.EV_PER_HA / A_PER_BOHR ** 2
        phi = phi * f
        parts = {k: v * f for k, v in parts.items()}
    return dict(phi=phi, parts=parts, asr_residual=asr, ground_state_gradient=gsg, **log)
