"""Elastic constants and the bulk modulus from the ground-state strain response.

`elastic_constants` stands behind the reference's `System.elastic_constants` and `System.bulk_modulus` (src/professad/system.py:
542-566, 670-693, 1225-1338), which differentiate the relaxed energy twice by autograd through xitorch's minimiser.  Here the
implicit derivative is explicit.  The strain is h -> h (I + eps) with a general eps at fixed fractional ion coordinates, fixed grid
values of chi and fixed N (the reference's closure, system.py:1266-1273), so n ~ 1 / det(I + eps).  With W1[m, n] = dE / d eps_mn
= vol sigma^T and V_kl = v_eps,kl - delta_kl hv(n, n) the total strain derivative of the potential at fixed chi,

    W2[m, n, p, q] = d2 E_gs / d eps_mn d eps_pq = W2^0 (fixed chi) + sum_r V_mn(r) dn_pq(r) dV

where dn_pq is `optimize.density_response` to dv = V_pq (six solves: V is symmetric in its indices).  The reference's convention:

    D[i, j, k, l] = W2[j, i, l, k] + W1[l, i] delta_jk,    C_ijkl = (D_ijkl + D_ijlk) / (2 vol) - sigma_ij delta_kl,

the 6 x 6 matrix in its order 11, 22, 33, 23, 13, 12, and K = vol d2E/dvol2 = (sum_ik W2[i, i, k, k] + 6 vol P) / (9 vol) with
P = -tr(W1) / (3 vol).  Single GPU, fp64, exact structure factor.
"""
import numpy as np

from . import ions, optimize
from .optimize import A_PER_BOHR

GPA_PER_ATOMIC = 4.3597447222071e-18 / 5.29177210903e-11 ** 3 * 1e-9
VOIGT = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))    # the reference's order (system.py:1330-1336) and that of the six fields


def unit_factor(units):
    if units == 'Ha/b3':
        return 1.0
    if units == 'eV/a3':
        return optimize.EV_PER_HA / A_PER_BOHR ** 3
    if units == 'GPa':
        return GPA_PER_ATOMIC
    raise ValueError("units must be one of 'Ha/b3', 'eV/a3', 'GPa', not %r" % (units,))


class HipElasticBackend(optimize.HipResponseBackend):
    """What `elastic_constants` needs, on the device: the strain entries of professad_amd.ions and Engine on top of
    optimize.HipResponseBackend (the conjugate gradients, the ground-state check).  Tensors in the strain are numpy arrays."""

    def strain_hessian(self, den):
        """{term: W2^0_t}, the ion_electron entry filled from the ions"""
        out = self.eng.strain_hessian(den)
        out['ion_electron'] = ions.ion_electron_strain_hessian(self.eng, self.box, den, self.species)
        return out

    def ion_ion_strain_hessian(self, frac, charges, Rc):
        return ions.ion_ion_strain_hessian(self.eng, self.box, frac, charges, Rc)

    def stress(self, den, frac, charges, Rc):
        """total stress [3, 3]: the functional's terms, ion-electron and ion-ion"""
        sig = sum(self.eng.stress(den).values()) + ions.ion_electron_stress(self.eng, self.box, den, self.species)
        return sig + ions.ion_ion(self.eng, self.box, frac, charges, Rc)[2]

    def potential_strain_gradient(self, den):
        """V_kl [6, grid]: v_eps,kl of the terms and of v_ext, minus delta_kl hv(n, n)"""
        V = self.eng.potential_strain_gradient(den) + ions.ionic_potential_strain_gradient(self.eng, self.box, self.species)
        V[:3] -= self.eng.hessian_vector(den, den)
        return V


def refusal(engine, pme_order=None):
    """None, or why `elastic_constants` cannot run on this engine (raised before any device work).  pbe_x / pbe_c are refused
    whatever the engine's OPT_HVP_GGA says, and wgc99_nl whatever its OPT_HVP_WGC says: their strain derivative is not built."""
    return optimize.response_refusal(engine, pme_order, 'strain')


def tensor_from_w2(W2, W1, volume):
    """C4 [3, 3, 3, 3] of the reference's recipe (system.py:1281-1337) from W2[m, n, p, q] and W1[m, n] = vol sigma^T"""
    eye = np.eye(3)
    D = np.einsum('jilk->ijkl', W2) + np.einsum('li,jk->ijkl', W1, eye)
    return 0.5 * (D + np.einsum('ijlk->ijkl', D)) / volume - np.einsum('ij,kl->ijkl', W1.T / volume, eye)


def voigt_matrix(C4):
    """-> (C [6, 6] as the reference assembles it: its upper triangle, mirrored; max|C - C^T| / max|C| of the full matrix)"""
    full = np.array([[C4[i, j, k, l] for (k, l) in VOIGT] for (i, j) in VOIGT])
    C = np.triu(full) + np.triu(full, 1).T
    return C, float(np.abs(full - full.T).max() / np.abs(full).max())


def bulk_from_w2(W2, W1, volume):
    """-> (K, P): K = vol d2E/dvol2 and P = -dE/dvol of the isotropic strain"""
    P = -np.trace(W1) / (3.0 * volume)
    return (np.einsum('iikk->', W2) + 6.0 * volume * P) / (9.0 * volume), P


def elastic_constants(engine, box_vecs, species, chi, Rc=None, rtol=1e-10, maxiter=500, units='Ha/b3', backend=None, pme_order=None,
                      precondition=None, batch=None):
    """Elastic constants (Birch coefficients) C_ijkl = d sigma_ij / d eps_kl at the ground state `chi`, with the relaxation of the
    density under the strain included.

    engine: a single-GPU fp64 `Engine` with the caller's term set (it includes ion_electron) on the cell `box_vecs`.
    species: iterable of (frac_coords [n, 3], (ks, v, z)) per ion type, as `ions.ionic_potential` takes it; n_elec = sum z.
    chi: a ground state of these terms in the potential of these ions, e.g. `optimize_density(..., n_method='TN')['chi']`.
    Rc: the ion-ion cutoff (`ions.ion_ion`).  rtol, maxiter: of the six conjugate-gradient solves.  units: 'Ha/b3', 'eV/a3', 'GPa'.

    Returns a dict: `C` [6, 6] in the reference's order 11, 22, 33, 23, 13, 12 and `C4` [3, 3, 3, 3]; `W2` [3, 3, 3, 3] (Ha, never
    converted) and its `parts`: `fixed_chi` {term: W2^0_t}, `ion_ion`, `response`; `stress` [3, 3], `pressure`, `bulk_modulus`;
    `symmetry_residual` = max|C - C^T| / max|C| of the 6 x 6 matrix before the reference's mirroring; `iterations`,
    `rel_residual`, `reason` (lists over the six solves, in the order xx, yy, zz, yz, xz, xy), `hvp_count`, and
    `ground_state_gradient` = max|g| / dV of the closure at `chi`.  A solve that ends for another reason than convergence raises
    a warning: unpreconditioned, the iteration count of the conjugate gradients grows with the grid; `precondition` (None, 'auto'
    or kappa^2 > 0, `optimize.HipCgBackend`) takes the grid out of it.  `batch`: None, or 1 .. 8: the six right-hand sides, in the
    same order, go `batch` columns at a time through batched solves (`optimize.density_response_multi`); the
    returned dict is the same, `hvp_count` then counting batched products.  With `backend` given, `batch` is that backend's own
    attribute, as `precondition` is.

    NotImplementedError, before any device work and naming the cause: PME, a slab-decomposed engine, an fp32 engine, a term
    without a second derivative.  (`backend`: an object with HipElasticBackend's methods -- the tests' numpy double.)"""
    f = unit_factor(units)
    species, frac, charges = optimize.normalise_species(species)
    optimize._own_backend_only('elastic_constants', backend, precondition)
    optimize.check_precondition(precondition)
    batch = optimize.resolve_batch('elastic_constants', backend, batch)
    if backend is None:
        why = refusal(engine, pme_order)
        if why:
            raise NotImplementedError('elastic_constants: ' + why)
    b = backend if backend is not None else HipElasticBackend(engine, box_vecs, species)
    try:
        if precondition is not None:
            b.cg.set_precondition(precondition)
        vol = b.volume
        n_elec = float(charges.sum())
        S = float((chi * chi).sum())
        n = (n_elec / (S * b.dV)) * chi * chi
        gsg = b.ground_state_gradient(chi, n_elec)
        fixed = b.strain_hessian(n)
        ion_ion = b.ion_ion_strain_hessian(frac, charges, Rc)
        sigma = np.asarray(b.stress(n, frac, charges, Rc), dtype=np.float64)
        V = b.potential_strain_gradient(n)
        log = optimize.new_solve_log()
        R6 = np.zeros((6, 6))
        if batch is None:
            for c in range(6):
                r = optimize.density_response(engine, chi, n_elec, V[c], rtol=rtol, maxiter=maxiter, backend=b.cg)
                for a in range(6):
                    R6[a, c] = float((V[a] * r['dn']).sum()) * b.dV
                optimize.log_solve(log, r)
        else:               # the same six right-hand sides in the same order, `batch` columns per solve
            for c, r in enumerate(optimize.batched_responses(b, engine, chi, n_elec, [V[c] for c in range(6)], batch, rtol, maxiter)):
                for a in range(6):
                    R6[a, c] = float((V[a] * r['dn']).sum()) * b.dV
                optimize.log_solve(log, r)
    finally:
        if backend is None:
            b.close()
    optimize.warn_unconverged('elastic_constants', log, maxiter, 'the constants are not accurate')
    response = np.zeros((3, 3, 3, 3))
    for a, (i, j) in enumerate(VOIGT):
        for c, (k, l) in enumerate(VOIGT):
            response[i, j, k, l] = response[j, i, k, l] = response[i, j, l, k] = response[j, i, l, k] = R6[a, c]
    W2 = sum(fixed.values()) + ion_ion + response
    W1 = vol * sigma.T
    C4 = tensor_from_w2(W2, W1, vol)
    C, sym = voigt_matrix(C4)
    K, P = bulk_from_w2(W2, W1, vol)
    return dict(C=C * f, C4=C4 * f, W2=W2, parts=dict(fixed_chi=fixed, ion_ion=ion_ion, response=response), stress=sigma * f,
                pressure=P * f, bulk_modulus=K * f, symmetry_residual=sym, ground_state_gradient=gsg, **log)


def bulk_modulus(engine, box_vecs, species, chi, units='Ha/b3', **kwargs):
    """K = vol d2E/dvol2 at the ground state `chi` (System.bulk_modulus, system.py:542-566): the `bulk_modulus` entry of
    `elastic_constants`, whose arguments it takes"""
    return elastic_constants(engine, box_vecs, species, chi, units=units, **kwargs)['bulk_modulus']


def voigt_moduli(C):
    """Voigt bulk and shear moduli of a 6 x 6 matrix of elastic constants"""
    C = np.asarray(C, dtype=np.float64)
    d, o, s = C[0, 0] + C[1, 1] + C[2, 2], C[0, 1] + C[1, 2] + C[0, 2], C[3, 3] + C[4, 4] + C[5, 5]
    return (d + 2.0 * o) / 9.0, (d - o + 3.0 * s) / 15.0


def reuss_moduli(C):
    """Reuss bulk and shear moduli: the same combinations of the compliances S = C^-1, inverted"""
    S = np.linalg.inv(np.asarray(C, dtype=np.float64))
    d, o, s = S[0, 0] + S[1, 1] + S[2, 2], S[0, 1] + S[1, 2] + S[0, 2], S[3, 3] + S[4, 4] + S[5, 5]
    return 1.0 / (d + 2.0 * o), 15.0 / (4.0 * d - 4.0 * o + 3.0 * s)


def shear_average(C, mean_type='arithmetic'):
    """Shear modulus as the arithmetic or geometric mean of the Voigt and Reuss shear moduli"""
    Gv, Gr = voigt_moduli(C)[1], reuss_moduli(C)[1]
    if mean_type == 'arithmetic':
        return 0.5 * (Gv + Gr)
    if mean_type == 'geometric':
        return (Gv * Gr) ** 0.5
    raise ValueError("mean_type must be 'arithmetic' or 'geometric', not %r" % (mean_type,))


def poissons_ratio(K, G):
    """nu = (1 - 3 G / (3 K + G)) / 2 from the bulk and shear moduli"""
    return 0.5 * (1.0 - 3.0 * G / (3.0 * K + G))
