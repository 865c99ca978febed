"""numpy double of the Hessian-vector product of the nonlocal part of WGC99 (professad_amd/csrc/hvp_kernels.h: hvp_wgc_head_kernel,
hvp_wgc_tail_kernel), on top of tests/hvp_gga_double.py:

    n_ref = kappa round(N) / vol, a constant of the differentiation (functionals.py:952-954);  theta = n - n_ref
    a = (A, A theta, A theta^2 / 2), A = n^beta;     p = (P, P theta, P theta^2 / 2), P = n^alpha
    M = [[w0, K1, K2], [K1, K3, 0], [K2, 0, 0]], each entry F^-1 table F  (functionals.py:968-981)
    E  = C_TF dV sum p . (M a);     U = M a,  G = M p
    hv = C_TF sum_i [ p_i'' w U_i + p_i' (M (a' w))_i + a_i'' w G_i + a_i' (M (p' w))_i ]        (' = d/dn, d theta / dn = 1)

The kernel tables are those of the oracle's WGC99 (oracle/closed_form.py: wgc_kernel, as oracle/stress.py forms K1, K2, K3 from it);
numpy.fft does the transforms.  `term_hv`, `hessian_vector` and `hessian_vector_chi` extend those of hvp_gga_double to the name
wgc99_nl; N is mean(den) vol of the density passed in, or `n_elec` where the caller has it (chi space).
Not the product: nothing in professad_amd imports it.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hvp_double as D  # noqa: E402
import hvp_gga_double as H  # noqa: E402
import tn_double as T  # noqa: E402
from oracle.closed_form import WGC_ALPHA, WGC_BETA, wgc_kernel  # noqa: E402

CTF = D.CTF
PARAMS = (WGC_ALPHA, WGC_BETA, 2.7, 1.0)          # alpha, beta, gamma, kappa


def tables(box, shape, nel_rounded, params=PARAMS):
    """-> n_ref and (w0, K1, K2, K3) on the half spectrum for round(N) = nel_rounded (functionals.py:952-972)"""
    al, be, ga, ka = params
    vol = abs(np.linalg.det(box))
    nref = ka * (nel_rounded / vol)
    k2 = D.k_squared(box, shape)
    eta = np.where(k2 != 0, np.sqrt(k2) / (2 * (3 * np.pi * np.pi * nref) ** (1 / 3)), 0.0)
    w0, w1, w2 = wgc_kernel(eta, al, be, ga)
    T_ = 20 * nref ** (5 / 3 - al - be)
    w0, w1, w2 = T_ * w0, T_ * w1, T_ * w2
    K1 = -eta * w1 / (6 * nref)
    K2 = (eta ** 2 * w2 + (7 - ga) * eta * w1) / (36 * nref ** 2)
    K3 = (eta ** 2 * w2 + (1 + ga) * eta * w1) / (36 * nref ** 2)
    return nref, (w0, K1, K2, K3)


def mix(tab, x):
    """M x for a triple of real fields"""
    w0, K1, K2, K3 = tab
    xk = [np.fft.rfftn(f) for f in x]
    yk = (w0 * xk[0] + K1 * xk[1] + K2 * xk[2], K1 * xk[0] + K3 * xk[1], K2 * xk[0])
    return [np.fft.irfftn(f, s=x[0].shape, axes=(0, 1, 2)) for f in yk]


def triple(n, th, e):
    """(f, f theta, f theta^2 / 2) for f = n^e with its first and second derivatives in n.  Where n is not positive f, f' and f'' count
    as 0, the rule of the device's wgc_triple (hvp_kernels.h): n^(e - 2) is infinite at n = 0 for both exponents, and the point is a
    zero of chi, which takes no part in the chi-space product."""
    pos = n > 0
    with np.errstate(divide='ignore', invalid='ignore'):
        f, f1, f2 = (np.where(pos, x, 0) for x in (n ** e, e * n ** (e - 1), e * (e - 1) * n ** (e - 2)))
    h = th * th / 2
    return ([f, f * th, f * h], [f1, f1 * th + f, f1 * h + f * th], [f2, f2 * th + 2 * f1, f2 * h + 2 * f1 * th + f])


def fields(box, den, n_elec=None, params=PARAMS):
    """the density side of a product: theta, the jets of a and p, the table, U = M a and G = M p"""
    vol = abs(np.linalg.det(box))
    nel = round(float(den.mean() * vol) if n_elec is None else n_elec)
    nref, tab = tables(box, den.shape, nel, params)
    th = den - nref
    a, p = triple(den, th, params[1]), triple(den, th, params[0])
    return dict(nref=nref, tab=tab, a=a, p=p, U=mix(tab, a[0]), G=mix(tab, p[0]))


def energy_potential(box, den, n_elec=None, params=PARAMS):
    """E_NL and its first derivative in the same notation (checked against the evaluation's closed form by the CPU test)"""
    f = fields(box, den, n_elec, params)
    dV = abs(np.linalg.det(box)) / den.size
    E = CTF * dV * sum(float((pi * ui).sum()) for pi, ui in zip(f['p'][0], f['U']))
    v = CTF * sum(pd * ui + ad * gi for pd, ui, ad, gi in zip(f['p'][1], f['U'], f['a'][1], f['G']))
    return E, v


def wgc_hv(box, den, w, n_elec=None, params=PARAMS):
    f = fields(box, den, n_elec, params)
    (_a, ad, add), (_p, pd, pdd) = f['a'], f['p']
    Ma = mix(f['tab'], [x * w for x in ad])
    Mp = mix(f['tab'], [x * w for x in pd])
    return CTF * sum(pdd[i] * w * f['U'][i] + pd[i] * Ma[i] + add[i] * w * f['G'][i] + ad[i] * Mp[i] for i in range(3))


def term_hv(box, den, w, term, alpha=5 / 6, beta=5 / 6, n_elec=None):
    """hvp_gga_double.term_hv, and wgc99_nl"""
    if term == 'wgc99_nl':
        return wgc_hv(box, den, w, n_elec)
    return H.term_hv(box, den, w, term, alpha, beta)


def hessian_vector(box, den, w, terms, alpha=5 / 6, beta=5 / 6, n_elec=None):
    """hvp_gga_double.hessian_vector for term sets that may hold wgc99_nl (its q_t is sum w hv_t dV, as the device forms it)"""
    dV = abs(np.linalg.det(box)) / den.size
    rest = [t for t in terms if t != 'wgc99_nl']
    q, hv = H.hessian_vector(box, den, w, rest, alpha, beta)
    if 'wgc99_nl' in terms:
        h = wgc_hv(box, den, w, n_elec)
        q['wgc99_nl'] = float((w * h).sum() * dV)
        hv = hv + h
    return q, hv


def hessian_vector_chi(box, phi, d, g, n_elec, terms, alpha=5 / 6, beta=5 / 6):
    """tn_double.hessian_vector_chi (the same chain from dv to H d) over this module's products; N is the caller's n_elec"""
    dV = abs(np.linalg.det(box)) / phi.size
    S, c, n = T.density(box, phi, n_elec)
    g = np.zeros_like(phi) if g is None else g
    a = float((phi * d).sum())
    dn = 2 * c * phi * d - (2 * a / S) * n
    dv = hessian_vector(box, n, dn, terms, alpha, beta, n_elec)[1]
    dmu = (float((dv * n).sum()) * dV + float((g * d).sum())) / n_elec
    with np.errstate(divide='ignore', invalid='ignore'):
        quot = np.where(phi != 0, d * g / phi, 0.0)
    Hd = -(2 * a / S) * g + quot + 2 * c * phi * (dv - dmu) * dV
    return dict(dHd=float((d * Hd).sum()), phiHd=float((phi * Hd).sum()), a=a, S=S, dmu=dmu), Hd


class NumpyCgBackend(H.NumpyCgBackend):
    """hvp_gga_double.NumpyCgBackend over this module's products"""

    def product(self, phi, g, n_elec, reuse):
        s, self.q = hessian_vector_chi(self.box, phi, self.p, g, n_elec, self.terms, self.al, self.be)
        self.products += 1
        return s['dHd'], s['phiHd']

    def hv(self, den, w):
        return hessian_vector(self.box, den, w, self.terms, self.al, self.be)[1]
