#!/usr/bin/env python3
"""Golden vectors of the Hessian-vector product on the vacuum-to-bulk case v16s (hvp_vacuum_cases.py), from the *reference*'s own
double autograd.

Run from the repo root where the reference is present (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_hvp_vacuum.py

Same in-memory stubs for the reference's absent third-party modules as make_golden_hvp.py; only OUTPUTS of the reference are
written.  Fixture (tests/golden/hvp_vacuum_v16s.npz): the direction w, an input checksum, and per key wgc99_nl
(F.WangGovindCarter99() minus Weizsaecker and ThomasFermi), pbe_x (F.pbe_exchange), pbe_c (F.pbe_correlation) and cfg3w
(IonElectron + Hartree + WGC99 + PBE)
    hv_<key> = grad((v w).sum(), n),  v = grad(E, n, create_graph=True) / dV        and        q_<key> = sum(w hv) dV
The reference takes round(mean(den) vol) with .item() (functionals.py:952-954), a constant of the differentiation; the generator
asserts that the case sits at least hvp_vacuum_cases.HALF_INTEGER_MARGIN from a jump of that rounding.
"""
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
    return F


import torch  # noqa: E402
import cases  # noqa: E402
import hvp_vacuum_cases  # noqa: E402

F = _import_reference()
DT = torch.double


def t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=DT)


def reference_terms(vext):
    wgc = F.WangGovindCarter99()
    return {
        'wgc99_nl': lambda b, d: wgc(b, d) - F.Weizsaecker(b, d) - F.ThomasFermi(b, d),
        'pbe_x': F.pbe_exchange, 'pbe_c': F.pbe_correlation,
        'cfg3w': lambda b, d: F.IonElectron(b, d, vext) + F.Hartree(b, d) + wgc(b, d) + F.PerdewBurkeErnzerhof(b, d),
    }


def hessian_vector(f, box, den, w):
    n = den.clone().requires_grad_()
    dV = torch.abs(torch.linalg.det(box)) / n.numel()
    v = torch.autograd.grad(f(box, n), n, create_graph=True)[0] / dV
    return torch.autograd.grad((v * w).sum(), n)[0].detach().numpy()


def main():
    for case in hvp_vacuum_cases.CASES:
        box, den, vext = hvp_vacuum_cases.make_inputs(case)
        w = hvp_vacuum_cases.direction(den)
        vol = abs(np.linalg.det(box))
        dV = vol / den.size
        frac = (den.mean() * vol) % 1.0
        print(case, 'mean(den) vol = %.4f' % (den.mean() * vol), 'den %.3e .. %.3e' % (den.min(), den.max()), flush=True)
        assert abs(frac - 0.5) >= hvp_vacuum_cases.HALF_INTEGER_MARGIN, (case, frac)
        res = {'w': w, 'checksum': cases.checksum(box, den, w)}
        terms = reference_terms(t(vext))
        assert set(terms) == set(hvp_vacuum_cases.KEYS)
        for key, f in terms.items():
            hv = hessian_vector(f, t(box), t(den), t(w))
            res['hv_' + key] = hv
            res['q_' + key] = float((w * hv).sum() * dV)
        path = os.path.join(HERE, 'hvp_vacuum_%s.npz' % case)
        np.savez_compressed(path, **res)
        print(case, os.path.getsize(path), 'bytes', flush=True)
        assert os.path.getsize(path) < (1 << 20)


if __name__ == '__main__':
    main()
