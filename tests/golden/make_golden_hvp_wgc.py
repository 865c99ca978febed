#!/usr/bin/env python3
"""Golden vectors of the Hessian-vector product of the WGC99 kinetic functional, from the *reference*'s own double autograd.

Run from the repo root where the reference is present (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_hvp_wgc.py

Same in-memory stubs for the reference's absent third-party modules as make_golden_hvp.py; only OUTPUTS of the reference are
written.  Fixtures (tests/golden/hvp_wgc_<case>.npz, cases of hvp_wgc_cases.py): the direction w, an input checksum, and per key
wgc99_nl (F.WangGovindCarter99() minus Weizsaecker and ThomasFermi), wgc99 (the whole functional), cfg3w (IonElectron + Hartree +
WGC99 + PBE) and cfg2w (the same with PerdewZunger)
    hv_<key> = grad((v w).sum(), n),  v = grad(E, n, create_graph=True) / dV        and        q_<key> = sum(w hv) dV
The reference takes round(mean(den) vol) with .item() (functionals.py:952-954), a constant of the differentiation; the generator
asserts that every case sits at least hvp_wgc_cases.HALF_INTEGER_MARGIN from a jump of that rounding.
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
import hvp_wgc_cases  # noqa: E402

F = _import_reference()
DT = torch.double


def t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=DT)


def reference_terms(vext):
    wgc = F.WangGovindCarter99()
    return {
        'wgc99_nl': lambda b, d: wgc(b, d) - F.Weizsaecker(b, d) - F.ThomasFermi(b, d),
        'wgc99': wgc,
        'cfg3w': lambda b, d: F.IonElectron(b, d, vext) + F.Hartree(b, d) + wgc(b, d) + F.PerdewBurkeErnzerhof(b, d),
        'cfg2w': lambda b, d: F.IonElectron(b, d, vext) + F.Hartree(b, d) + wgc(b, d) + F.PerdewZunger(b, d),
    }


def hessian_vector(f, box, den, w):
    n = den.clone().requires_grad_()
    dV = torch.abs(torch.linalg.det(box)) / n.numel()
    v = torch.autograd.grad(f(box, n), n, create_graph=True)[0] / dV
    return torch.autograd.grad((v * w).sum(), n)[0].detach().numpy()


def main():
    for case in hvp_wgc_cases.CASES:
        box, den, vext = hvp_wgc_cases.make_inputs(case)
        w = hvp_wgc_cases.direction(den.shape)
        vol = abs(np.linalg.det(box))
        dV = vol / den.size
        frac = (den.mean() * vol) % 1.0
        print(case, 'mean(den) vol = %.4f' % (den.mean() * vol), flush=True)
        assert abs(frac - 0.5) >= hvp_wgc_cases.HALF_INTEGER_MARGIN, (case, frac)
        res = {'w': w, 'checksum': cases.checksum(box, den, w)}
        for key, f in reference_terms(t(vext)).items():
            hv = hessian_vector(f, t(box), t(den), t(w))
            res['hv_' + key] = hv
            res['q_' + key] = float((w * hv).sum() * dV)
        path = os.path.join(HERE, 'hvp_wgc_%s.npz' % case)
        np.savez_compressed(path, **res)
        print(case, os.path.getsize(path), 'bytes', flush=True)


if __name__ == '__main__':
    main()
