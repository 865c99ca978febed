"""Numpy double of the Huang-Carter kinds of OFDFT_NLK (kinds 4 and 5): the closed form the engine evaluates, restated on the CPU.

    hc_energy_potential(kind, args, box, den, eta, w) -> dict(E_nl, v_nl, xi_min, xi_max, lower, M, touched, nodes, used, q)

kind 'hc' with args (lambda, beta, kappa) or 'revhc' with (a, b, beta, kappa); (eta, w) the kernel table.  E_nl = T_NL [Ha] and
v_nl = dT_NL/dn on the grid.  With p = 8/3 - beta, C = 0.3 (3 pi^2)^(2/3) 8 (3 pi^2), gamma = |grad n|^2 (spectral gradient,
the Nyquist row of an even extent counted as positive, functional_tools.py:150-156):
    xi = 2 k_F (1 + lambda gamma / (n^(8/3) + 1e-30))      |      2 k_F (1 + a s^2 / (1 + b s^2))
    nodes xi_j = lower kappa^j (functional_tools.py:415-417), f_j = F^-1[w(min(q / xi_j, eta_max)) F[n^beta]]
    K = sum_o c_o f_(i+o), K_xi = sum_o c'_o f_(i+o) over the four nodes of the spline interval i of xi(r) (functional_tools.py:337-378)
    E = dV sum A K,  A = C n^p / xi^3,   Q = C n^p (K_xi / xi^3 - 3 K / xi^4)
    v = C p n^(p-1) K / xi^3 + Q dxi/dn - div(2 Q dxi/dgamma grad n) + beta n^(beta-1) F^-1[sum_j w_j F[W_j]]
W_j(r) = A c_o where j = i(r) + o.  The node set is a constant of the differentiation.

Measured against the reference's own forward + autograd on the fixtures (tests/test_hc_cpu.py prints the figures):
E_nl within 8e-17 of |E_total|, v_nl within 3.6e-14 of max |v_nl| over the eight (case, kind) pairs (the largest on g16w).
"""
import numpy as np

C_HC = 0.3 * (3 * np.pi ** 2) ** (2 / 3) * 8 * (3 * np.pi ** 2)


def wavevecs(box, shape):
    b = 2 * np.pi * np.linalg.inv(np.asarray(box, dtype=np.float64).T)
    f = [np.fft.fftfreq(shape[i]) * shape[i] for i in range(2)]
    for a in f:
        a[len(a) // 2] = abs(a[len(a) // 2])
    f.append(np.fft.rfftfreq(shape[2]) * shape[2])
    nA, nB, nC = np.meshgrid(*f, indexing='ij')
    k = [nA * b[0, j] + nB * b[1, j] + nC * b[2, j] for j in range(3)]
    return k[0], k[1], k[2], k[0] ** 2 + k[1] ** 2 + k[2] ** 2


def interpolate(x, y, xs):
    """functional_tools.py:292-334"""
    m = (y[1:] - y[:-1]) / (x[1:] - x[:-1])
    m = np.concatenate([m[:1], (m[1:] + m[:-1]) / 2, m[-1:]])
    idx = np.searchsorted(x[1:], xs)
    dx = x[idx + 1] - x[idx]
    t = (xs - x[idx]) / dx
    return ((1 - 3 * t ** 2 + 2 * t ** 3) * y[idx] + (t - 2 * t ** 2 + t ** 3) * m[idx] * dx + (3 * t ** 2 - 2 * t ** 3) * y[idx + 1]
            + (t ** 3 - t ** 2) * m[idx + 1] * dx)


def xi_field(kind, args, n, gg):
    """xi, dxi/dn, dxi/dgamma"""
    kF = (3 * np.pi ** 2 * n) ** (1 / 3)
    n83 = n ** (8 / 3)
    if kind == 'hc':
        lam = args[0]
        d = n83 + 1e-30
        Fs, dF_dn, dF_dgg = 1 + lam * gg / d, lam * (-(8 / 3) * n ** (5 / 3) * gg / d ** 2), lam / d
    else:
        a, b = args[0], args[1]
        cs = 0.25 * (3 * np.pi ** 2) ** (-2 / 3)
        s2 = cs * gg / n83
        dFds2 = a / (1 + b * s2) ** 2
        Fs, dF_dn, dF_dgg = 1 + a * s2 / (1 + b * s2), dFds2 * (-(8 / 3) * s2 / n), dFds2 * cs / n83
    return 2 * kF * Fs, 2 * kF / (3 * n) * Fs + 2 * kF * dF_dn, 2 * kF * dF_dgg


def hc_energy_potential(kind, args, box, den, eta, w):
    n = np.asarray(den, dtype=np.float64)
    shape = n.shape
    beta, kappa = (args[1], args[2]) if kind == 'hc' else (args[2], args[3])
    p = 8 / 3 - beta
    kx, ky, kz, k2 = wavevecs(box, shape)
    dV = abs(np.linalg.det(box)) / n.size
    nk = np.fft.rfftn(n)
    g = [np.fft.irfftn(1j * k * nk, shape, axes=(0, 1, 2)) for k in (kx, ky, kz)]
    xi, dxi_dn, dxi_dgg = xi_field(kind, args, n, g[0] ** 2 + g[1] ** 2 + g[2] ** 2)
    xi_min, xi_max = float(xi.min()), float(xi.max())
    lower = kappa ** (-(np.ceil(-np.log(xi_min) / np.log(kappa)) + 3))
    M = int(np.ceil(np.log((xi_max + 1) / lower) / np.log(kappa)) + 3)
    xs = lower * kappa ** np.arange(M, dtype=np.float64)
    q = np.sqrt(k2)
    wt = interpolate(eta, w, np.minimum(q[..., None] / xs, eta[-1]))
    conv = np.fft.irfftn(wt * np.fft.rfftn(n ** beta)[..., None], s=shape, axes=(0, 1, 2))
    idx = np.searchsorted(xs[1:], xi)
    assert idx.min() >= 1 and idx.max() <= M - 3
    dx, dm, dp = xs[idx + 1] - xs[idx], xs[idx] - xs[idx - 1], xs[idx + 2] - xs[idx + 1]
    t = (xi - xs[idx]) / dx
    h = [1 - 3 * t ** 2 + 2 * t ** 3, t - 2 * t ** 2 + t ** 3, 3 * t ** 2 - 2 * t ** 3, -t ** 2 + t ** 3]
    dh = [(-6 * t + 6 * t ** 2) / dx, (1 - 4 * t + 3 * t ** 2) / dx, (6 * t - 6 * t ** 2) / dx, (-2 * t + 3 * t ** 2) / dx]

    def weights(h):
        a1, a2 = h[1] * dx / 2, h[3] * dx / 2
        return [-a1 / dm, h[0] + a1 / dm - a1 / dx - a2 / dx, h[2] + a1 / dx + a2 / dx - a2 / dp, a2 / dp]
    cw, dcw = weights(h), weights(dh)
    fj = [np.take_along_axis(conv, (idx + o)[..., None], 3)[..., 0] for o in (-1, 0, 1, 2)]
    K = sum(c * f for c, f in zip(cw, fj))
    Kxi = sum(c * f for c, f in zip(dcw, fj))
    A = C_HC * n ** p / xi ** 3
    Q = C_HC * n ** p * (Kxi / xi ** 3 - 3 * K / xi ** 4)
    E = float((A * K).sum() * dV)
    v = C_HC * p * n ** (p - 1) * K / xi ** 3 + Q * dxi_dn
    u = 2 * Q * dxi_dgg
    v = v - sum(np.fft.irfftn(1j * k * np.fft.rfftn(u * gi), shape, axes=(0, 1, 2)) for k, gi in zip((kx, ky, kz), g))
    W = np.zeros(shape + (M,))
    for o, c in zip((-1, 0, 1, 2), cw):
        np.put_along_axis(W, (idx + o)[..., None], (A * c)[..., None], 3)
    v = v + beta * n ** (beta - 1) * np.fft.irfftn((wt * np.fft.rfftn(W, axes=(0, 1, 2))).sum(3), s=shape, axes=(0, 1, 2))
    # touched: spline intervals from the lowest to the highest one used; nodes, used: the node set and the first and last node
    # that some point's spline reads; q: |k| on the half spectrum
    return dict(E_nl=E, v_nl=v, xi_min=xi_min, xi_max=xi_max, lower=float(lower), M=M, touched=int(idx.max() - idx.min() + 1),
                nodes=xs, used=(int(idx.min()) - 1, int(idx.max()) + 2), q=q)


def tf_vw(box, den):
    """(E, v) of Thomas-Fermi + von Weizsaecker (functionals.py:207-246), for the functionals' totals"""
    n = np.asarray(den, dtype=np.float64)
    dV = abs(np.linalg.det(box)) / n.size
    ctf = 0.3 * (3 * np.pi ** 2) ** (2 / 3)
    _kx, _ky, _kz, k2 = wavevecs(box, n.shape)
    s = np.sqrt(n)
    lap = np.fft.irfftn(-k2 * np.fft.rfftn(s), n.shape, axes=(0, 1, 2))
    E = float((ctf * n ** (5 / 3)).sum() * dV + (-0.5 * s * lap).sum() * dV)
    return E, (5 / 3) * ctf * n ** (2 / 3) - 0.5 * lap / s
