"""numpy double of the second strain derivative at fixed chi (professad_amd/csrc/strain2_kernels.h, engine_strain.inc.h;
DESIGN.md §9e), so that the closed forms are pinned to the reference's autograd without a GPU (tests/test_elastic_cpu.py) and the
device results can be compared on grids that have no golden (tests/test_elastic_gpu.py).  Built from oracle/ and library
functions.  Not the product: nothing in professad_amd imports it, and it imports nothing from professad_amd.

The strain is h -> h (I + eps), eps general; fractional ion coordinates, the grid values of chi and N are fixed, so n ~ 1/J,
J = det(I + eps).  W2[m, n, p, q] = d^2 E / d eps_mn d eps_pq at eps = 0.  A reciprocal-space term E = sum_k X_k f(s_k, J),
s = |k|^2, k -> (I + eps)^-1 k, gives (ds/d eps_mn = -2 k_m k_n, d2s = 2 (k_m k_q d_np + k_p k_n d_qm + k_n k_q d_mp),
d2J = d_mn d_pq - d_mq d_np)

    W2 = sum_k X [4 f_ss k k k k + 2 f_s (k_m k_q d_np + k_p k_n d_qm + k_n k_q d_mp) - 2 f_sJ (k_m k_n d_pq + d_mn k_p k_q)
                  + f_JJ d_mn d_pq + f_J (d_mn d_pq - d_mq d_np)].

Here every coefficient is formed from the derivatives of f on their own (the device code takes the f_sJ moments from the others).
"""
import math

import numpy as np
from scipy.special import erf, erfc

import hvp_double as D
from oracle import ionion
from oracle import ions as O
from oracle import stress as OS
from oracle.closed_form import recip

EYE = np.eye(3)
DD_MN_PQ = np.einsum('mn,pq->mnpq', EYE, EYE)
DD_MQ_NP = np.einsum('mq,np->mnpq', EYE, EYE)
LOCAL = ('tf', 'lda_x', 'pz_c', 'pw_c', 'chachiyo_c')
SPECTRAL = ('hartree', 'vw', 'wt_nl')


def volume_tensor(E_J, E_JJ):
    """W2 of an energy that depends on the cell through J alone"""
    return E_J * (DD_MN_PQ - DD_MQ_NP) + E_JJ * DD_MN_PQ


def spectral_tensor(K, X, f_s, f_ss, f_sJ, f_J, f_JJ):
    """K [3, nk] wave vectors, X [nk] weights, the derivatives of f per k-point (scalars broadcast)"""
    one = np.ones_like(X)
    M4 = np.einsum('k,mk,nk,pk,qk->mnpq', 4 * X * f_ss * one, K, K, K, K, optimize=True)
    M2 = np.einsum('k,ik,jk->ij', 2 * X * f_s * one, K, K)
    M2b = np.einsum('k,ik,jk->ij', -2 * X * f_sJ * one, K, K)
    return (M4 + np.einsum('mq,np->mnpq', M2, EYE) + np.einsum('pn,qm->mnpq', M2, EYE) + np.einsum('nq,mp->mnpq', M2, EYE)
            + np.einsum('mn,pq->mnpq', M2b, EYE) + np.einsum('mn,pq->mnpq', EYE, M2b)
            + volume_tensor(np.sum(X * f_J * one), np.sum(X * f_JJ * one)))


def _half_spectrum(box, shape):
    """wave vectors [3, nk], |k|^2 [nk] and multiplicities [nk] of the half spectrum without k = 0"""
    kx, ky, kz, k2 = recip(box, shape)
    w = np.broadcast_to(O.half_weights(shape)[None, None, :], k2.shape)
    m = k2 != 0
    return np.stack([kx[m], ky[m], kz[m]]), k2[m], w[m], m


def lindhard_shape_d2(eta):
    """F = 1/G - 3 eta^2 - 1 of the Lindhard response (functionals.py:617-628, 648), P = eta F', Q = eta^2 F'' for eta > 0.
    eta >= 3: the series in z = eta^-2 (c_j = 1 / (4 j^2 - 1), G = z R, R = sum c_(j+1) z^j, V = sum c_(j+2) z^j, F = -3 V / R - 1,
    eta d/d eta = -2 z d/dz), 18 terms; below, the direct form; eta == 1: G is the constant 1/2 of the reference's masked
    assignment."""
    eta = np.asarray(eta, dtype=np.float64)
    F, P, Q = np.empty_like(eta), np.empty_like(eta), np.empty_like(eta)
    big = eta >= 3.0
    z = 1.0 / eta[big] ** 2
    c = 1.0 / (4.0 * np.arange(1, 20) ** 2 - 1.0)                # c_1 .. c_19
    R, V = np.polynomial.Polynomial(c[:18]), np.polynomial.Polynomial(c[1:19])
    r, r1, r2, v, v1, v2 = R(z), R.deriv(1)(z), R.deriv(2)(z), V(z), V.deriv(1)(z), V.deriv(2)(z)
    u1 = (v1 * r - v * r1) / r ** 2
    u2 = (v2 * r - v * r2) / r ** 2 - 2 * r1 * u1 / r
    F[big], P[big], Q[big] = -3 * v / r - 1, 6 * z * u1, -18 * z * u1 - 12 * z * z * u2
    one = eta == 1.0
    F[one], P[one], Q[one] = -2.0, -6.0, -6.0
    m = ~big & ~one
    e = eta[m]
    lg = np.log(np.abs((1 + e) / (1 - e)))
    G = 0.5 + (1 - e * e) / (4 * e) * lg
    Dg = 0.5 - 0.25 * (e + 1 / e) * lg
    De = -0.25 * (1 - 1 / (e * e)) * lg - 0.5 * (e + 1 / e) / (1 - e * e)
    F[m] = 1 / G - 3 * e * e - 1
    P[m] = -Dg / G ** 2 - 6 * e * e
    Q[m] = -(e * De - Dg) / G ** 2 + 2 * Dg ** 2 / G ** 3 - 6 * e * e
    return F, P, Q


def hartree(box, den):
    """E = (vol / 2) sum_k w 4 pi |n^_k|^2 / (J s)"""
    K, s, w, m = _half_spectrum(box, den.shape)
    X = 0.5 * abs(np.linalg.det(box)) * w * 4 * math.pi * np.abs(np.fft.rfftn(den, norm='forward')[m]) ** 2
    return spectral_tensor(K, X, -1 / s ** 2, 2 / s ** 3, 1 / s ** 2, -1 / s, 2 / s)


def vw(box, den):
    """E = (vol / 2) sum_k w s |F[sqrt n]_k|^2, the spectrum forward-normalised: vol |.|^2 is strain-invariant"""
    K, s, w, m = _half_spectrum(box, den.shape)
    X = 0.5 * abs(np.linalg.det(box)) * w * np.abs(np.fft.rfftn(np.sqrt(den), norm='forward')[m]) ** 2
    return spectral_tensor(K, X, 1.0, 0.0, 0.0, 0.0, 0.0)


def wt_nl(box, den, alpha=5 / 6, beta=5 / 6):
    """E = vol c_TF pref sum_k w Re(a^ b^*) J^(-2/3) F(eta), eta = sqrt(s) J^(1/3) / (2 k_F), n0 = N / vol (functionals.py:644-652)"""
    K, s, w, m = _half_spectrum(box, den.shape)
    vol = abs(np.linalg.det(box))
    n0 = (den.mean() * vol) / vol
    kf = (3 * math.pi ** 2 * n0) ** (1 / 3)
    a = np.fft.rfftn(den ** alpha, norm='forward')[m]
    b = np.fft.rfftn(den ** beta, norm='forward')[m]
    X = vol * D.CTF * 5 / (9 * alpha * beta * n0 ** (alpha + beta - 5 / 3)) * w * (a * np.conj(b)).real
    F, P, Q = lindhard_shape_d2(np.sqrt(s) / (2 * kf))
    return spectral_tensor(K, X, P / (2 * s), (Q - P) / (4 * s * s), (Q - P) / (6 * s), -2 / 3 * F + P / 3,
                           10 / 9 * F - 2 / 3 * P + Q / 9)


def hermite_second(x, y, xs):
    """d^2/dxs^2 of oracle.ions.hermite_interp inside an interval"""
    mm = O.hermite_slopes(x, y)
    idx = np.searchsorted(x[1:], xs)
    dx = x[idx + 1] - x[idx]
    t = (xs - x[idx]) / dx
    return ((12 * t - 6) * y[idx] + (6 * t - 4) * mm[idx] * dx + (-12 * t + 6) * y[idx + 1] + (6 * t - 2) * mm[idx + 1] * dx) / dx ** 2


def ion_electron(box, den, frac, tab):
    """E = (1 / N J) sum_k w Re(S_k conj(n~_k)) v~(sqrt s) of one species; tab = (ks, v with the Coulomb tail added, z)"""
    ks, y, z = tab
    shape = den.shape
    K, s, w, m = _half_spectrum(box, shape)
    core = O.half_weights(shape)[None, None, :] * (O.structure_factor_exact(box, shape, frac) * np.conj(np.fft.rfftn(den))).real / den.size
    kabs = np.sqrt(s)
    inside = kabs < ks[-1]
    xs = np.minimum(kabs, ks[-1])
    v = O.hermite_interp(ks, y, xs) - 4 * math.pi * z / s
    dv = np.where(inside, OS.hermite_derivative(ks, y, xs), 0.0) + 8 * math.pi * z / kabs ** 3
    d2v = np.where(inside, hermite_second(ks, y, xs), 0.0) - 24 * math.pi * z / s ** 2
    out = spectral_tensor(K, core[m], dv / (2 * kabs), d2v / (4 * s) - dv / (4 * kabs ** 3), -dv / (2 * kabs), -v, 2 * v)
    v0 = float(y[0])                                            # k = 0: f = v~(0) / J
    return out + volume_tensor(-core[0, 0, 0] * v0, 2 * core[0, 0, 0] * v0)


def local(box, den, term):
    """a pointwise term E = vol J mean(e(n / J)): E_J from the stress trace, E_JJ = int n (H_t n)"""
    vol = abs(np.linalg.det(box))
    sig = OS.tf(box, den) if term == 'tf' else OS.lda(box, den, term)
    E_JJ = float((den * D.term_hv(box, den, den, term)).sum()) * vol / den.size
    return volume_tensor(vol * np.trace(sig) / 3, E_JJ)


def term(box, den, name, alpha=5 / 6, beta=5 / 6):
    if name == 'hartree':
        return hartree(box, den)
    if name == 'vw':
        return vw(box, den)
    if name == 'wt_nl':
        return wt_nl(box, den, alpha, beta)
    return local(box, den, name)


def ion_ion(box, frac, charges, Rc=None):
    """the pair sum over the fixed pair list (oracle.ionion.pairs) with Rd, Rc held, r^2 = d (I + eps)(I + eps)^T d^T, plus the
    background term through rho ~ 1/J and R_a ~ J^(1/3)"""
    Rc, Rd = ionion.heuristics(box, Rc)
    coords = frac @ box
    charges = np.asarray(charges, dtype=np.float64)
    vol = abs(np.linalg.det(box))
    rho = charges.sum() / vol
    spi = math.sqrt(math.pi)
    W = np.zeros((3, 3, 3, 3))
    Q = charges.copy()
    for i, j, d, r in ionion.pairs(box, coords, Rc):
        Q[i] += charges[j] * r.size
        zz = charges[i] * charges[j]
        e = np.exp(-(r / Rd) ** 2)
        fp = zz * (-2 * e / (spi * Rd * r) - erfc(r / Rd) / r ** 2)
        fpp = zz * (4 * e / (spi * Rd ** 3) + 4 * e / (spi * Rd * r ** 2) + 2 * erfc(r / Rd) / r ** 3)
        W += 0.5 * np.einsum('k,km,kn,kp,kq->mnpq', (fpp - fp / r) / r ** 2, d, d, d, d, optimize=True)
        W += 0.5 * np.einsum('mp,nq->mnpq', np.einsum('k,km,kp->mp', fp / r, d, d), EYE)
    Ra = np.cbrt(0.75 / math.pi * Q / rho)
    Z = charges
    ex, er = np.exp(-Ra ** 2 / Rd ** 2), erf(Ra / Rd)
    h = -math.pi * Z * Ra ** 2 + math.pi * Z * (Ra ** 2 - 0.5 * Rd * Rd) * er + spi * Z * Ra * Rd * ex
    h1 = -2 * math.pi * Z * Ra * erfc(Ra / Rd)
    h2 = -2 * math.pi * Z * erfc(Ra / Rd) + 4 * spi * Z * Ra * ex / Rd
    return W + volume_tensor(np.sum(rho * (h1 * Ra / 3 - h)), np.sum(rho * (2 * h - 8 / 9 * h1 * Ra + h2 * Ra ** 2 / 9)))


# ------------------------------------------------------------------------------------------- strain gradient of the potential
VOIGT = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))          # xx, yy, zz, yz, xz, xy


def potential_strain_gradient(box, den, terms, alpha=5 / 6, beta=5 / 6):
    """v_eps,kl [6, grid] of a term set: the derivative of dE/dn with respect to eps_kl at fixed grid values of den, n0 = N / vol
    following the cell.  d(1/s) = 2 k_k k_l / s^2, d(-s) = 2 k_k k_l, d ln n0 = -delta_kl, d ln eta = delta_kl / 3 - k_k k_l / s."""
    shape = den.shape
    kx, ky, kz, k2 = recip(box, shape)
    k = (kx, ky, kz)
    with np.errstate(divide='ignore', invalid='ignore'):
        inv = np.where(k2 != 0, 1.0 / np.where(k2 != 0, k2, 1.0), 0.0)
    out = np.zeros((6,) + shape)

    def conv(f, x):
        return np.fft.irfftn(f * np.fft.rfftn(x), s=shape, axes=(0, 1, 2))
    if 'hartree' in terms:
        for c, (i, j) in enumerate(VOIGT):
            out[c] += conv(8 * math.pi * k[i] * k[j] * inv * inv, den)
    if 'vw' in terms:
        chi = np.sqrt(den)
        for c, (i, j) in enumerate(VOIGT):
            out[c] -= conv(k[i] * k[j], chi) / chi
    if 'wt_nl' in terms:
        vol = abs(np.linalg.det(box))
        n0 = (den.mean() * vol) / vol
        kf = (3 * math.pi ** 2 * n0) ** (1 / 3)
        pref = 5 / (9 * alpha * beta * n0 ** (alpha + beta - 5 / 3))
        F, P = np.zeros(k2.shape), np.zeros(k2.shape)
        m = k2 != 0
        F[m], P[m], _Q = lindhard_shape_d2(np.sqrt(k2[m]) / (2 * kf))
        for c, (i, j) in enumerate(VOIGT):
            Kp = pref * ((i == j) * ((alpha + beta - 5 / 3) * F + P / 3) - P * k[i] * k[j] * inv)
            out[c] += D.CTF * (alpha * den ** (alpha - 1) * conv(Kp, den ** beta) + beta * den ** (beta - 1) * conv(Kp, den ** alpha))
    return out


def _table(tab, kabs):
    """v~, v~' on |k| from the prepared table (ks, v with the Coulomb tail added, z); zero slope past the table end"""
    ks, y, z = tab
    xs = np.minimum(kabs, ks[-1])
    safe = np.where(kabs != 0, kabs, 1.0)
    v = O.hermite_interp(ks, y, xs) - np.where(kabs != 0, 4 * math.pi * z / safe ** 2, 0.0)
    dv = np.where(kabs < ks[-1], OS.hermite_derivative(ks, y, xs), 0.0) + 8 * math.pi * z / safe ** 3
    return v, np.where(kabs != 0, dv, 0.0)


def ionic_potential_strain_gradient(box, shape, frac, tab):
    """d v_ext / d eps_kl [6, grid] of one species: -delta_kl v_ext + F^-1[S v~' (-k_k k_l / |k|)] / vol"""
    kx, ky, kz, k2 = recip(box, shape)
    k = (kx, ky, kz)
    kabs = np.sqrt(k2)
    v, dv = _table(tab, kabs)
    S = O.structure_factor_exact(box, shape, frac)
    vol = abs(np.linalg.det(box))
    safe = np.where(kabs != 0, kabs, 1.0)
    return np.stack([np.fft.irfftn(S * (-dv * k[i] * k[j] / safe - (i == j) * v), s=shape, axes=(0, 1, 2), norm='forward') / vol
                     for i, j in VOIGT])


def ion_electron_stress(box, den, frac, tab):
    """oracle.stress.ion_electron from the prepared table"""
    shape = den.shape
    kx, ky, kz, k2 = recip(box, shape)
    k = (kx, ky, kz)
    kabs = np.sqrt(k2)
    v, dv = _table(tab, kabs)
    core = O.half_weights(shape)[None, None, :] * (O.structure_factor_exact(box, shape, frac) * np.conj(np.fft.rfftn(den))).real / den.size
    safe = np.where(kabs != 0, kabs, 1.0)
    sig = -np.sum(core * v) * np.eye(3)
    for i in range(3):
        for j in range(3):
            sig[i, j] -= np.sum(core * dv * k[i] * k[j] / safe)
    return sig / abs(np.linalg.det(box))


def term_stress(box, den, name, alpha=5 / 6, beta=5 / 6):
    if name in ('hartree', 'tf', 'vw'):
        return getattr(OS, name)(box, den)
    if name == 'wt_nl':
        return OS.wt_nl(box, den, alpha, beta)
    return OS.lda(box, den, name)


class NumpyElasticBackend:
    """elastic.HipElasticBackend in numpy: the pieces above, the pinned oracle closure (oracle/refpath.py) for the gradient at
    the ground state, tests/tn_double.NumpyCgBackend for the solves.  species: [(frac, (ks, v, z))]; terms include ion_electron."""

    def __init__(self, box, shape, species, terms):
        import fc_double
        import tn_double
        self.box, self.shape, self.species, self.terms = box, tuple(shape), species, list(terms)
        self.volume = abs(np.linalg.det(box))
        self.dV = self.volume / int(np.prod(shape))
        self.cg = tn_double.NumpyCgBackend(box, shape, terms)
        self._fc = fc_double.NumpyFcBackend(box, shape, species, terms)

    def closure(self, chi, n_elec):
        return self._fc.closure(chi, n_elec)

    def ground_state_gradient(self, chi, n_elec):
        return self._fc.ground_state_gradient(chi, n_elec)

    def _functional(self):
        return [t for t in self.terms if t != 'ion_electron']

    def strain_hessian(self, den):
        out = {t: term(self.box, den, t) for t in self._functional()}
        out['ion_electron'] = sum(ion_electron(self.box, den, f, tab) for f, tab in self.species)
        return out

    def ion_ion_strain_hessian(self, frac, charges, Rc):
        return ion_ion(self.box, frac, charges, Rc)

    def stress(self, den, frac, charges, Rc):
        sig = sum(term_stress(self.box, den, t) for t in self._functional())
        sig = sig + sum(ion_electron_stress(self.box, den, f, tab) for f, tab in self.species)
        Rc_, Rd = ionion.heuristics(self.box, Rc)
        return sig + ionion.forces_stress(self.box, frac @ self.box, np.asarray(charges, dtype=np.float64), Rc_, Rd)[1]

    def potential_strain_gradient(self, den):
        V = potential_strain_gradient(self.box, den, self._functional())
        V = V + sum(ionic_potential_strain_gradient(self.box, self.shape, f, tab) for f, tab in self.species)
        V[:3] -= D.hessian_vector(self.box, den, den, self._functional())[1]
        return V

    def close(self):
        pass
