"""numpy double of the Hessian-vector product (professad_amd/csrc/hvp_kernels.h, engine_hvp.inc.h; DESIGN.md "Hessian-vector
products"): hv = d/d eps v[n + eps w] at eps = 0 per term, in closed form, with numpy.fft for the transforms -- so that the
operator forms are pinned to the reference's double autograd without a GPU (tests/test_hvp_cpu.py) and the device result can be
compared on grids that have no golden (tests/test_hvp_gpu.py).  Not the product: nothing in professad_amd imports it.
"""
import numpy as np

CTF = 0.3 * (3 * np.pi ** 2) ** (2 / 3)
S5 = np.sqrt(5.0)
WGC98 = ((5 + S5) / 6, (5 - S5) / 6)


def k_squared(box, shape):
    """|k|^2 on the half spectrum (functional_tools.py:135-162)"""
    b = 2 * np.pi * np.linalg.inv(np.asarray(box, dtype=np.float64).T)
    f = [np.fft.fftfreq(s) * s for s in shape[:2]] + [np.fft.rfftfreq(shape[2]) * shape[2]]
    for a in (0, 1):                       # the Nyquist frequency of an even extent counts as positive (:152-154)
        if shape[a] % 2 == 0:
            f[a][shape[a] // 2] = shape[a] // 2
    fa, fb, fc = np.meshgrid(*f, indexing='ij')
    k = [fa * b[0, j] + fb * b[1, j] + fc * b[2, j] for j in range(3)]
    return k[0] ** 2 + k[1] ** 2 + k[2] ** 2


def lindhard(eta):
    """G^-1(eta) (functionals.py:617-628)"""
    g = np.ones_like(eta)
    m = (eta != 0.0) & (eta != 1.0)
    e = eta[m]
    g[m] = 0.5 + (1 - e * e) / (4 * e) * np.log(np.abs((1 + e) / (1 - e)))
    g[eta == 1.0] = 0.5
    return g


def wt_kernel(box, den, alpha, beta):
    """the kernel of non_local_KEF (functionals.py:644-652) with n0 = mean(den): a constant of the differentiation"""
    vol = abs(np.linalg.det(box))
    n0 = (den.mean() * vol) / vol          # as the reference forms it: the kernel at large eta amplifies the last bit of n0 ~100 times
    eta = np.sqrt(k_squared(box, den.shape)) / (2 * (3 * np.pi ** 2 * n0) ** (1 / 3))
    return 5 / (9 * alpha * beta * n0 ** (alpha + beta - 5 / 3)) * (1 / lindhard(eta) - 3 * eta ** 2 - 1)


def _conv(kern, x):
    return np.fft.irfftn(kern * np.fft.rfftn(x), s=x.shape, axes=(0, 1, 2))


def corr_second(n, kind):
    """d^2 (n eps_c) / dn^2 = rs (rs eps'' - 2 eps') / (9 n) of functionals.py:1515-1537"""
    rs = (3 / (4 * np.pi * n)) ** (1 / 3)
    if kind == 'pz_c':
        gm, b1, b2, A, C, D = -0.1423, 1.0529, 0.3334, 0.0311, 0.002, -0.0116
        sr = np.sqrt(rs)
        den = 1 + b1 * sr + b2 * rs
        dd, d2d = 0.5 * b1 / sr + b2, -0.25 * b1 / (rs * sr)
        d1 = np.where(rs < 1, A / rs + C * np.log(rs) + C + D, -gm * dd / den ** 2)
        d2 = np.where(rs < 1, -A / rs ** 2 + C / rs, -gm * d2d / den ** 2 + 2 * gm * dd ** 2 / den ** 3)
    elif kind == 'pw_c':
        A, a1, b1, b2, b3, b4 = 0.0310907, 0.2137, 7.5957, 3.5876, 1.6382, 0.49294
        sr = np.sqrt(rs)
        z = 2 * A * (b1 * sr + b2 * rs + b3 * rs * sr + b4 * rs ** 2)
        dz = 2 * A * (0.5 * b1 / sr + b2 + 1.5 * b3 * sr + 2 * b4 * rs)
        d2z = 2 * A * (-0.25 * b1 / (rs * sr) + 0.75 * b3 / sr + 2 * b4)
        q = z * (z + 1)
        L, dL, d2L = np.log(1 + 1 / z), -dz / q, -d2z / q + dz ** 2 * (2 * z + 1) / q ** 2
        pre = 2 * A * (1 + a1 * rs)
        d1 = -2 * A * a1 * L - pre * dL
        d2 = -4 * A * a1 * dL - pre * d2L
    elif kind == 'chachiyo_c':
        a, b = (np.log(2) - 1) / 2 / np.pi ** 2, 20.4562557
        arg = 1 + b / rs + b / rs ** 2
        da, d2a = -b / rs ** 2 - 2 * b / rs ** 3, 2 * b / rs ** 3 + 6 * b / rs ** 4
        d1 = a * da / arg
        d2 = a * (d2a / arg - da ** 2 / arg ** 2)
    else:
        raise KeyError(kind)
    return rs * (rs * d2 - 2 * d1) / (9 * n)


def term_hv(box, den, w, term, alpha=5 / 6, beta=5 / 6):
    """hv of one served term"""
    n = den
    if term == 'ion_electron':
        return np.zeros_like(n)
    if term == 'hartree':
        k2 = k_squared(box, n.shape)
        with np.errstate(divide='ignore'):
            coul = np.where(k2 != 0, 4 * np.pi / k2, 0.0)
        return _conv(coul, w)
    if term == 'tf':
        return (10 / 9) * CTF * n ** (-1 / 3) * w
    if term == 'vw':
        k2 = k_squared(box, n.shape)
        chi = np.sqrt(n)
        dchi = w / (2 * chi)
        return -0.5 * (_conv(-k2, dchi) / chi - _conv(-k2, chi) * dchi / chi ** 2)
    if term == 'wt_nl':
        K = wt_kernel(box, n, alpha, beta)
        A, B = _conv(K, n ** beta), _conv(K, n ** alpha)
        return CTF * (alpha * (alpha - 1) * n ** (alpha - 2) * w * A + alpha * n ** (alpha - 1) * _conv(K, beta * n ** (beta - 1) * w)
                      + beta * (beta - 1) * n ** (beta - 2) * w * B + beta * n ** (beta - 1) * _conv(K, alpha * n ** (alpha - 1) * w))
    if term == 'lda_x':
        return -(1 / 3) * (3 / np.pi) ** (1 / 3) * n ** (-2 / 3) * w
    return corr_second(n, term) * w


def hessian_vector(box, den, w, terms, alpha=5 / 6, beta=5 / 6):
    """-> (dict term -> int w (H_t w), hv) of a term set, as Engine.hessian_vector(..., want_terms=True) returns them"""
    dV = abs(np.linalg.det(box)) / den.size
    hv, q = np.zeros_like(den), {}
    for t in terms:
        h = term_hv(box, den, w, t, alpha, beta)
        q[t] = float((w * h).sum() * dV)
        hv += h
    return q, hv
