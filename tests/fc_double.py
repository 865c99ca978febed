"""numpy double of the force-constant pieces (professad_amd/csrc/fc_kernels.h, engine_force_constants.inc.h) and a
numpy backend with force_constants.HipFcBackend's methods, so that the closed forms are pinned to the reference's autograd
without a GPU (tests/test_force_constants_cpu.py), the host logic of professad_amd.force_constants runs without a device, and the
device results can be compared on grids that have no golden (tests/test_force_constants_gpu.py).  Not the product: nothing in
professad_amd imports it.
"""
import math
import os

import numpy as np
import torch
from scipy.special import erfc

import tn_double as T
from oracle import ionion, refpath
from oracle import ions as O
from oracle.closed_form import recip

PAIRS6 = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def two_species(seed):
    """three ions of two species -- the recpot of tests/golden/ions.npz and a made-up second one with half the potential, as in
    tests/test_force_constants_gpu.py -- with fractional coordinates partly outside [0, 1)"""
    from professad_amd.ions import recpot_table
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ions.npz'))
    tab = recpot_table(g['recpot_raw'], float(g['recpot_kmax']))
    tab2 = (tab[0], 0.5 * tab[1], 0.5 * tab[2])
    rng = np.random.default_rng(seed)
    return [(rng.random((1, 3)), tab), (rng.random((2, 3)) * 1.5 - 0.25, tab2)]


def table_on_grid(tab, kabs):
    """interpolate_recpot (ion_utils.py:74-81) from the prepared table (ks, v with the Coulomb tail added, z)"""
    ks, v, z = tab
    y = O.hermite_interp(ks, v, np.minimum(kabs, ks[-1]))
    with np.errstate(divide='ignore'):
        return np.where(kabs != 0, y - 4 * math.pi * z / np.where(kabs != 0, kabs, 1.0) ** 2, y)


def _spectral(box, shape, tab):
    kx, ky, kz, k2 = recip(box, shape)
    return (kx, ky, kz), table_on_grid(tab, np.sqrt(k2)), abs(np.linalg.det(box))


def potential_gradient(box, shape, R, tab):
    """d v_ext / d R_j of one ion at the Cartesian position R -> [3, n0, n1, n2]"""
    k, vk, vol = _spectral(box, shape, tab)
    ph = np.exp(-1j * (k[0] * R[0] + k[1] * R[1] + k[2] * R[2]))
    return np.stack([np.fft.irfftn(-1j * kj * ph * vk, s=shape, axes=(0, 1, 2), norm='forward') / vol for kj in k])


def ionic_potential(box, shape, frac, tab):
    _k, vk, vol = _spectral(box, shape, tab)
    return np.fft.irfftn(O.structure_factor_exact(box, shape, frac) * vk, s=shape, axes=(0, 1, 2), norm='forward') / vol


def _ion_sums(box, den, frac, tab, weight):
    """sum_k w_k v~ weight(k, phase conj(n^)) per ion"""
    shape = den.shape
    k, vk, vol = _spectral(box, shape, tab)
    w = O.half_weights(shape)[None, None, :] * vk
    nk = np.conj(np.fft.rfftn(den))
    cart = frac @ box
    dV = vol / den.size
    return [weight(k, w * np.exp(-1j * (k[0] * R[0] + k[1] * R[1] + k[2] * R[2])) * nk) for R in cart], dV / vol


def ion_electron_forces(box, den, frac, tab):
    """F_a = -d/dR_a dV sum_r den v_ext -> [n, 3]; linear in den, any sign"""
    out, pref = _ion_sums(box, den, frac, tab, lambda k, c: [np.sum((kj * 1j * c).real) for kj in k])
    return pref * np.array(out)


def ion_electron_curvature(box, den, frac, tab):
    """D[a] = d^2 (dV sum_r den v_ext) / dR_a dR_a -> [n, 3, 3]"""
    out, pref = _ion_sums(box, den, frac, tab, lambda k, c: [[np.sum((ki * kj * c).real) for kj in k] for ki in k])
    return -pref * np.array(out)


def ion_ion_hessian(box, frac, charges, rows, Rc=None):
    """d^2 E_ion-ion / dR_p dR_b at a fixed pair list (oracle.ionion.pairs), p in rows -> [len(rows), n, 3, 3]"""
    Rc, Rd = ionion.heuristics(box, Rc)
    coords = frac @ box
    n = coords.shape[0]
    H = np.zeros((n, n, 3, 3))
    spi = math.sqrt(math.pi)
    for i, j, d, r in ionion.pairs(box, coords, Rc):
        if i == j:
            continue
        zz = charges[i] * charges[j]
        e = np.exp(-(r / Rd) ** 2)
        fp = zz * (-2 * e / (spi * Rd * r) - erfc(r / Rd) / r ** 2)
        fpp = zz * (4 * e / (spi * Rd ** 3) + 4 * e / (spi * Rd * r ** 2) + 2 * erfc(r / Rd) / r ** 3)
        Tm = np.einsum('p,pa,pb->ab', (fpp - fp / r) / r ** 2, d, d) + np.sum(fp / r) * np.eye(3)
        H[i, j] -= Tm
        H[i, i] += Tm
    return H[list(rows)]


class NumpyFcBackend:
    """force_constants.HipFcBackend in numpy: the pieces above, the pinned oracle closure (oracle/refpath.py) for the gradient at
    the ground state, tests/tn_double.NumpyCgBackend for the solves"""

    def __init__(self, box, shape, species, terms):
        self.box, self.shape, self.species, self.terms = box, tuple(shape), species, list(terms)
        self.dV = abs(np.linalg.det(box)) / int(np.prod(shape))
        self.cg = T.NumpyCgBackend(box, shape, terms)

    def vext(self):
        return sum(ionic_potential(self.box, self.shape, f, tab) for f, tab in self.species)

    def closure(self, chi, n_elec):
        table = refpath.term_table(torch.as_tensor(self.vext()))
        E, g = refpath.closure(torch.as_tensor(self.box), torch.as_tensor(chi), n_elec, [table[k] for k in self.terms])
        return float(E), g.numpy()

    def ground_state_gradient(self, chi, n_elec):
        return float(np.abs(self.closure(chi, n_elec)[1]).max()) / self.dV

    def potential_gradient(self, ion):
        for f, tab in self.species:
            if ion < f.shape[0]:
                return potential_gradient(self.box, self.shape, (f @ self.box)[ion], tab)
            ion -= f.shape[0]
        raise IndexError(ion)

    def ion_electron_forces(self, den):
        return np.concatenate([ion_electron_forces(self.box, den, f, tab) for f, tab in self.species])

    def ion_electron_curvature(self, den):
        return np.concatenate([ion_electron_curvature(self.box, den, f, tab) for f, tab in self.species])

    def ion_ion_hessian(self, frac, charges, rows, Rc):
        return ion_ion_hessian(self.box, frac, charges, rows, Rc)

    def close(self):
        pass
