#!/usr/bin/env python3
"""Golden vectors of the Hessian-vector product of PBE exchange and correlation, from the *reference*'s own double autograd.

Run from the repo root where the reference is present (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_hvp_gga.py

Same in-memory stubs for the reference's absent third-party modules as make_golden_hvp.py; only OUTPUTS of the reference are
written.  Fixtures (tests/golden/hvp_gga_<case>.npz, cases of hvp_gga_cases.py): the direction w, an input checksum, and per key
pbe_x (F.pbe_exchange), pbe_c (F.pbe_correlation), pbe (F.PerdewBurkeErnzerhof) and cfg3 (IonElectron + Hartree + WangTeter + PBE)
    hv_<key> = grad((v w).sum(), n),  v = grad(E, n, create_graph=True) / dV        and        q_<key> = sum(w hv) dV
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
import hvp_gga_cases  # noqa: E402

F = _import_reference()
DT = torch.double


def t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=DT)


def reference_terms(vext):
    return {
        'pbe_x': F.pbe_exchange, 'pbe_c': F.pbe_correlation, 'pbe': F.PerdewBurkeErnzerhof,
        'cfg3': lambda b, d: F.IonElectron(b, d, vext) + F.Hartree(b, d) + F.WangTeter(b, d) + F.PerdewBurkeErnzerhof(b, d),
    }


def hessian_vector(f, box, den, w):
    n = den.clone().requires_grad_()
    dV = torch.abs(torch.linalg.det(box)) / n.numel()
    v = torch.autograd.grad(f(box, n), n, create_graph=True)[0] / dV
    return torch.autograd.grad((v * w).sum(), n)[0].detach().numpy()


def main():
    for case in hvp_gga_cases.CASES:
        box, den, vext = hvp_gga_cases.make_inputs(case)
        w = hvp_gga_cases.direction(den.shape)
        dV = abs(np.linalg.det(box)) / den.size
        res = {'w': w, 'checksum': cases.checksum(box, den, w)}
        for key, f in reference_terms(t(vext)).items():
            hv = hessian_vector(f, t(box), t(den), t(w))
            res['hv_' + key] = hv
            res['q_' + key] = float((w * hv).sum() * dV)
        path = os.path.join(HERE, 'hvp_gga_%s.npz' % case)
        np.savez_compressed(path, **res)
        print(case, os.path.getsize(path), 'bytes', flush=True)


if __name__ == '__main__':
    main()
