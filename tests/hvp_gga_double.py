"""numpy double of the Hessian-vector product of PBE exchange and correlation (professad_amd/csrc/hvp_kernels.h:
hvp_gga_mid_kernel, pointwise_kernels.h: pbe_second), on top of tests/hvp_double.py and tests/tn_double.py:

    E = dV sum f(n, sigma),  sigma = sum_a (D_a n)^2,  D_a = F^-1 i k_a F  (the reference's grad_i, functional_tools.py:166-183)
    dsigma = 2 sum_a D_a n D_a w
    hv     = f_nn w + f_ns dsigma - 2 sum_a D_a [(f_ns w + f_ss dsigma) D_a n + f_s D_a w]

with the second partials of f in closed form (`second_partials`): the pointwise f(n, sigma) of functionals.py:1597-1618, its two
1e-30 guards kept as constants, pushed through second-order Taylor arithmetic in (n, sigma) -- every elementary step
(sum, product, reciprocal, log, exp, power of n) carries its exact first and second derivatives.  numpy.fft does the transforms,
k is built as hvp_double.k_squared builds it.  `term_hv`, `hessian_vector`, `hessian_vector_chi` and `NumpyCgBackend` extend those
of hvp_double / tn_double to the names pbe_x and pbe_c by import.  Not the product: nothing in professad_amd imports it.
"""
import numpy as np

import hvp_double as D
import tn_double as T

GGA = ('pbe_x', 'pbe_c')


def k_vectors(box, shape):
    """(kx, ky, kz) on the half spectrum (functional_tools.py:135-162), as hvp_double.k_squared builds |k|^2"""
    b = 2 * np.pi * np.linalg.inv(np.asarray(box, dtype=np.float64).T)
    f = [np.fft.fftfreq(s) * s for s in shape[:2]] + [np.fft.rfftfreq(shape[2]) * shape[2]]
    for a in (0, 1):                       # the Nyquist frequency of an even extent counts as positive (:152-154)
        if shape[a] % 2 == 0:
            f[a][shape[a] // 2] = shape[a] // 2
    fa, fb, fc = np.meshgrid(*f, indexing='ij')
    return [fa * b[0, j] + fb * b[1, j] + fc * b[2, j] for j in range(3)]


def grad(k, x):
    """D_a x for a = 0, 1, 2"""
    xk = np.fft.rfftn(x)
    return [np.fft.irfftn(1j * ka * xk, s=x.shape, axes=(0, 1, 2)) for ka in k]


class Jet:
    """value and the partials (n, s, nn, ns, ss) of a function of (n, sigma) on the grid"""

    def __init__(self, v, n=0.0, s=0.0, nn=0.0, ns=0.0, ss=0.0):
        self.c = (v, n, s, nn, ns, ss)

    @staticmethod
    def lift(x):
        return x if isinstance(x, Jet) else Jet(x)

    def __add__(self, o):
        o = Jet.lift(o)
        return Jet(*[a + b for a, b in zip(self.c, o.c)])

    __radd__ = __add__

    def __neg__(self):
        return Jet(*[-a for a in self.c])

    def __sub__(self, o):
        return self + (-Jet.lift(o))

    def __rsub__(self, o):
        return Jet.lift(o) + (-self)

    def __mul__(self, o):
        o = Jet.lift(o)
        a, an, as_, ann, ans, ass = self.c
        b, bn, bs, bnn, bns, bss = o.c
        return Jet(a * b, an * b + a * bn, as_ * b + a * bs, ann * b + 2 * an * bn + a * bnn,
                   ans * b + an * bs + as_ * bn + a * bns, ass * b + 2 * as_ * bs + a * bss)

    __rmul__ = __mul__

    def chain(self, g0, g1, g2):
        """g(self) from g, g', g'' at the value"""
        _a, an, as_, ann, ans, ass = self.c
        return Jet(g0, g1 * an, g1 * as_, g2 * an * an + g1 * ann, g2 * an * as_ + g1 * ans, g2 * as_ * as_ + g1 * ass)

    def recip(self):
        r = 1.0 / self.c[0]
        return self.chain(r, -r * r, 2 * r ** 3)

    def __truediv__(self, o):
        return self * Jet.lift(o).recip()

    def __rtruediv__(self, o):
        return Jet.lift(o) * self.recip()

    def log(self):
        r = 1.0 / self.c[0]
        return self.chain(np.log(self.c[0]), r, -r * r)

    def exp(self):
        e = np.exp(self.c[0])
        return self.chain(e, e, e)

    def pow(self, p):
        v = self.c[0]
        return self.chain(v ** p, p * v ** (p - 1), p * (p - 1) * v ** (p - 2))


def energy_density(n, sigma, term):
    """f(n, sigma) of functionals.py:1597-1618 for numbers, arrays or Jets (n, sigma as Jets: its Taylor expansion)"""
    lift = isinstance(n, Jet)
    log = (lambda x: x.log()) if lift else np.log
    exp = (lambda x: x.exp()) if lift else np.exp
    pw = (lambda x, p: x.pow(p)) if lift else (lambda x, p: x ** p)
    if term == 'pbe_x':
        ex = -(3 / 4) * (3 / np.pi) ** (1 / 3) * pw(n, 4 / 3)
        s2 = 0.25 * (3 * np.pi * np.pi) ** (-2 / 3) * sigma / pw(n, 8 / 3)
        kappa, mu = 0.804, 0.066725 * np.pi * np.pi / 3
        return (1 + kappa - kappa / (1 + mu / kappa * s2)) * ex
    if term == 'pbe_c':
        A1, alpha = 0.0310907, 0.2137
        b1, b2, b3, b4 = 7.5957, 3.5876, 1.6382, 0.49294
        rs = pw(3 / 4 / np.pi / n, 1 / 3)
        eps = -2 * A1 * (1 + alpha * rs) * log(1 + 1 / (2 * A1 * (b1 * pw(rs, 0.5) + b2 * rs + b3 * pw(rs, 1.5) + b4 * pw(rs, 2))))
        beta, gamma = 0.066725, (1 - np.log(2)) / np.pi / np.pi
        A = beta / gamma / (exp(-1 * eps / gamma) - 1 + 1e-30)
        t2 = (1 / 16) * (np.pi / 3) ** (1 / 3) * sigma / (pw(n, 7 / 3) + 1e-30)
        At2 = A * t2
        H = gamma * log(1 + beta / gamma * t2 * ((1 + At2) / (1 + At2 + At2 * At2)))
        return (eps + H) * n
    raise KeyError(term)


def second_partials(n, sigma, term):
    """-> f_s, f_nn, f_ns, f_ss of the term on the grid"""
    f = energy_density(Jet(n, n=1.0), Jet(sigma, s=1.0), term)
    _v, _fn, fs, fnn, fns, fss = f.c
    return fs, fnn, fns, fss


def gga_hv(box, den, w, terms):
    """-> (dict term -> q_t by the adjoint identity, hv summed over `terms`) for terms among pbe_x, pbe_c"""
    k = k_vectors(box, den.shape)
    dV = abs(np.linalg.det(box)) / den.size
    gn, gw = grad(k, den), grad(k, w)
    sigma = sum(a * a for a in gn)
    ds = 2 * sum(a * b for a, b in zip(gn, gw))
    gw2 = sum(b * b for b in gw)
    tot, q = np.zeros((4,) + den.shape), {}
    for t in terms:
        p = np.array(second_partials(den, sigma, t))
        fs, fnn, fns, fss = p
        q[t] = float((fnn * w * w + 2 * fns * w * ds + fss * ds * ds + 2 * fs * gw2).sum() * dV)
        tot += p
    fs, fnn, fns, fss = tot
    c = fns * w + fss * ds
    div = sum(d for d in (grad([ka], c * a + fs * b)[0] for ka, a, b in zip(k, gn, gw)))
    return q, fnn * w + fns * ds - 2 * div


def term_hv(box, den, w, term, alpha=5 / 6, beta=5 / 6):
    """hvp_double.term_hv, and pbe_x / pbe_c"""
    if term in GGA:
        return gga_hv(box, den, w, (term,))[1]
    return D.term_hv(box, den, w, term, alpha, beta)


def hessian_vector(box, den, w, terms, alpha=5 / 6, beta=5 / 6):
    """hvp_double.hessian_vector for term sets that may hold pbe_x / pbe_c (their q_t from the adjoint identity, as the device forms it)"""
    dV = abs(np.linalg.det(box)) / den.size
    hv, q = np.zeros_like(den), {}
    for t in terms:
        if t in GGA:
            qt, h = gga_hv(box, den, w, (t,))
            q[t] = qt[t]
        else:
            h = D.term_hv(box, den, w, t, alpha, beta)
            q[t] = float((w * h).sum() * dV)
        hv += h
    return q, hv


def hessian_vector_chi(box, phi, d, g, n_elec, terms, alpha=5 / 6, beta=5 / 6):
    """tn_double.hessian_vector_chi (the same chain from dv to H d) over this module's products"""
    dV = abs(np.linalg.det(box)) / phi.size
    S, c, n = T.density(box, phi, n_elec)
    g = np.zeros_like(phi) if g is None else g
    a = float((phi * d).sum())
    dn = 2 * c * phi * d - (2 * a / S) * n
    dv = hessian_vector(box, n, dn, terms, alpha, beta)[1]
    dmu = (float((dv * n).sum()) * dV + float((g * d).sum())) / n_elec
    with np.errstate(divide='ignore', invalid='ignore'):
        quot = np.where(phi != 0, d * g / phi, 0.0)
    Hd = -(2 * a / S) * g + quot + 2 * c * phi * (dv - dmu) * dV
    return dict(dHd=float((d * Hd).sum()), phiHd=float((phi * Hd).sum()), a=a, S=S, dmu=dmu), Hd


class NumpyCgBackend(T.NumpyCgBackend):
    """tn_double.NumpyCgBackend over this module's products"""

    def product(self, phi, g, n_elec, reuse):
        s, self.q = hessian_vector_chi(self.box, phi, self.p, g, n_elec, self.terms, self.al, self.be)
        self.products += 1
        return s['dHd'], s['phiHd']

    def hv(self, den, w):
        return hessian_vector(self.box, den, w, self.terms, self.al, self.be)[1]
