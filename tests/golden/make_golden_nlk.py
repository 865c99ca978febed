#!/usr/bin/env python3
"""Golden vectors of the tabulated-kernel nonlocal functionals (KGAP, Mi-Genova-Pavanello, Xu-Wang-Ma), from the *reference*.

Run from the repo root where the reference is present (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_nlk.py [--big | --stress]

Same in-memory stubs for the reference's absent third-party modules as make_golden.py; only OUTPUTS of the reference are
written.  Fixtures (tests/golden/):
  nlk_<case>.npz         g16s, g17r, g18t, g20t: per functional E, v = get_functional_derivative, and the nonlocal part alone
                         E_nl = E - E_vW - E_TF, v_nl = v - v_vW - v_TF (the stabilised KGAP: totals only); MGP's rounding noise;
                         for g16s also the kernel arrays the CPU test restates (kgap_kernel, xwm_kernel1, mgp_table)
  nlk_big_scalars.json   (--big) 64^3, 128^3, 96^3, 53^3: E, E_nl and cases.probe_stats of v / v_nl
  nlk_stress.npz         (--stress) get_stress of KGAP(2.0), KGAP(1.1, exp), XWM(0), XWM(0.5) on g16s, g18t, g20t ('<case>_<key>')

MGP's rounding noise: the reference's 1-D quadrature evaluates 1/G - 3 eta^2 - 1 at eta up to ~290, where it cancels about
eleven digits; the reference is evaluated a second time with its table replaced by the np.longdouble evaluation of the same sum
on the same nodes, and mgp_noise_E = |E - E'|, mgp_noise_v = max|v_nl - v_nl'| / max|v_nl| are stored: how far the reference
is from the exact value of its own formula.
"""
import argparse
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True


def _import_reference():
    def _absent(*a, **k):
        raise NotImplementedError('stubbed third-party dependency (not on the hot path)')

    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m

    stub('xitorch')
    stub('xitorch.integrate', solve_ivp=_absent)
    stub('xitorch.optimize', minimize=_absent)
    stub('torch_nl', compute_neighborlist=_absent)
    sys.path.insert(0, '/root/reference/src')
    import professad.functionals as F
    import professad.functional_tools as T
    return F, T


import torch  # noqa: E402
import cases  # noqa: E402
from professad_amd import synth  # noqa: E402

F, T = _import_reference()
DT = torch.double
SMALL_CASES = ['g16s', 'g17r', 'g18t', 'g20t']
BIG_GRIDS = [64, 128, 96, 53]
STRESS_CASES = ['g16s', 'g18t', 'g20t']
STRESS_KEYS = ['kgap_2.0', 'kgap_1.1_exp', 'xwm_0', 'xwm_0.5']       # (MGP: the reference's get_stress raises on it)
MGP_ARGS = (0.2, 0.01)
ROUNDING_MARGIN = 0.05      # |N_e - (k + 1/2)| must exceed this: round(N_e) is then the same number for every evaluator


def t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=DT)


def functionals():
    """name -> (callable, has a nonlocal part of its own); MGP a fresh instance per call of this function"""
    return {
        'kgap_2.0': (lambda b, d: F.KGAP(b, d, 2.0), True),
        'kgap_1.1_exp': (lambda b, d: F.KGAP(b, d, 1.1, torch.exp), False),
        'kgap_0.0': (lambda b, d: F.KGAP(b, d, 0.0), True),
        'xwm_0': (lambda b, d: F.XuWangMa(b, d, 0), True),
        'xwm_0.5': (lambda b, d: F.XuWangMa(b, d, 0.5), True),
        'mgp': (F.MiGenovaPavanello(MGP_ARGS), True),
    }


def e_and_pot(f, box, den):
    E = float(f(box, den.clone()).item())
    v = T.get_functional_derivative(box, den.clone(), f)
    return E, v.detach().numpy()


def longdouble_table(etas_1d, n_int=10000):
    """the sum of MiGenovaPavanello.generate_kernel on the same nodes and quadrature points, in np.longdouble"""
    ts64 = torch.linspace(1e-4, 1, n_int, dtype=DT).numpy()
    ts = ts64.astype(np.longdouble)
    dt = np.longdouble(ts64[1] - ts64[0])
    out = np.empty(len(etas_1d), dtype=np.float64)
    t13, t16 = ts ** (np.longdouble(1) / 3), ts ** (np.longdouble(1) / 6)
    for i0 in range(0, len(etas_1d), 100):
        e = etas_1d[i0:i0 + 100].astype(np.longdouble)[:, None] / t13[None, :]
        with np.errstate(divide='ignore', invalid='ignore'):
            g = np.longdouble(0.5) + ((1 - e * e) / (4 * e)) * np.log(np.abs((1 + e) / (1 - e)))
        g[e == 0] = 1
        g[e == 1] = 0.5
        w = np.longdouble(0.2) * (3 * np.pi ** 2) ** (np.longdouble(2) / 3) * np.sum((1 / g - 3 * e * e - 1) / t16[None, :], axis=1) * dt
        out[i0:i0 + 100] = w.astype(np.float64)
    return out


def check_margin(name, box, den):
    nel = float(den.mean() * abs(np.linalg.det(box)))
    assert abs(nel - np.floor(nel) - 0.5) > ROUNDING_MARGIN, '%s: N_e = %.4f is within %.2f of a rounding edge' % (name, nel, ROUNDING_MARGIN)
    return nel


def evaluate_all(name, box_np, den_np, full):
    """-> dict of results for one input (full: keep the potentials; else probe statistics)"""
    nel = check_margin(name, box_np, den_np)
    box, den = t(box_np), t(den_np)
    E_vw, v_vw = e_and_pot(F.Weizsaecker, box, den)
    E_tf, v_tf = e_and_pot(F.ThomasFermi, box, den)
    res = {'n_elec': nel}
    fs = functionals()
    for key, (f, has_nl) in fs.items():
        E, v = e_and_pot(f, box, den)
        res[key + '_E'] = E
        res[key + '_v'] = v if full else cases.probe_stats(v)
        if has_nl:
            res[key + '_E_nl'] = E - E_vw - E_tf
            v_nl = v - v_vw - v_tf
            res[key + '_v_nl'] = v_nl if full else cases.probe_stats(v_nl)
            res[key + '_v_nl_max'] = float(np.abs(v_nl).max())
        if key == 'mgp':
            mgp = f
            table_ref = mgp.kernel.detach().numpy().copy()
            exact = longdouble_table(table_ref[0])
            mgp.kernel = torch.cat([mgp.kernel[0].unsqueeze(0), t(exact).unsqueeze(0)])
            E2, v2 = e_and_pot(mgp, box, den)
            res['mgp_noise_E'] = abs(E - E2)
            res['mgp_noise_v'] = float(np.abs(v - v2).max() / np.abs(v_nl).max())
            res['mgp_table_noise'] = float(np.abs(table_ref[1] - exact).max() / np.abs(table_ref[1]).max())
            if full:
                res['mgp_table'] = table_ref
    return res


def kernel_arrays(box_np, den_np):
    """the k-space arrays behind the g16s goldens, for the CPU restatement test"""
    box, den = t(box_np), t(den_np)
    eta_g, ginv_gap = F.G_inv_gap(box, den, 2.0)
    kg = torch.zeros_like(eta_g)
    nz = eta_g != 0
    kg[nz] = 1 / ginv_gap[nz] - 3 * eta_g[nz] ** 2 - 1
    eta, ginv = F.G_inv_lindhard(box, den)
    vol = abs(np.linalg.det(box_np))
    n0 = round(float(den_np.mean() * vol)) / vol
    gder = torch.zeros_like(eta)
    nz = eta != 0
    gder[nz] = 0.5 - 0.25 * (eta[nz] + 1 / eta[nz]) * torch.log(torch.abs((1 + eta[nz]) / (1 - eta[nz])))
    k1 = np.pi ** 2 / (3 * np.pi ** 2) ** (1 / 3) / (6 * n0) * (gder * ginv ** -2 + 6 * eta ** 2)      # kappa = 0
    return dict(kgap_eta=eta_g.numpy(), kgap_kernel=kg.numpy(), xwm_eta=eta.numpy(), xwm_kernel1=k1.numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--big', action='store_true')
    ap.add_argument('--stress', action='store_true')
    ap.add_argument('--only', default=None)
    args = ap.parse_args()
    if args.stress:
        out = {}
        for case in STRESS_CASES:
            box, den, _vext, _chi, _n = cases.make_inputs(case)
            check_margin(case, box, den)
            fs = functionals()
            for key in STRESS_KEYS:
                out['%s_%s' % (case, key)] = T.get_stress(t(box), t(den), fs[key][0]).detach().numpy()
                print(case, key, out['%s_%s' % (case, key)].diagonal(), flush=True)
            out[case + '_checksum'] = cases.checksum(box, den)
        np.savez_compressed(os.path.join(HERE, 'nlk_stress.npz'), **out)
        return
    if not args.big:
        for case in SMALL_CASES:
            if args.only and case != args.only:
                continue
            box, den, _vext, _chi, _n = cases.make_inputs(case)
            res = evaluate_all(case, box, den, True)
            res['checksum'] = cases.checksum(box, den)
            if case == 'g16s':
                res.update(kernel_arrays(box, den))
            path = os.path.join(HERE, 'nlk_%s.npz' % case)
            np.savez_compressed(path, **res)
            print(case, 'N_e = %.4f' % res['n_elec'], 'mgp noise E %.2e v %.2e table %.2e' % (res['mgp_noise_E'], res['mgp_noise_v'], res['mgp_table_noise']),
                  os.path.getsize(path), 'bytes', flush=True)
        return
    path = os.path.join(HERE, 'nlk_big_scalars.json')
    out = json.load(open(path)) if os.path.exists(path) else {}
    for n in BIG_GRIDS:
        if args.only and str(n) != args.only:
            continue
        box = synth.cubic_cell(n)
        seed = 1234
        den = synth.random_density((n, n, n), seed=seed)
        res = evaluate_all('big_%d' % n, box, den, False)
        res['seed'] = seed
        res['checksum'] = cases.checksum(box, den)
        out[str(n)] = res
        print(n, 'N_e = %.4f' % res['n_elec'], 'mgp noise E %.2e v %.2e' % (res['mgp_noise_E'], res['mgp_noise_v']), flush=True)
        json.dump(out, open(path, 'w'), indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
