#!/usr/bin/env python3
"""Golden vectors of the Hessian-vector product, from the *reference*'s own double autograd.

Run from the repo root where the reference is present (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_hvp.py

Same in-memory stubs for the reference's absent third-party modules as make_golden_nlk.py; only OUTPUTS of the reference are
written.  Fixtures (tests/golden/hvp_<case>.npz, cases of hvp_cases.py): the direction w, an input checksum, and per key of
hvp_cases.TERMS / SETS and for `wts_user` (WangTeterStyleFunctional with hvp_cases.user_stabiliser)
    hv_<key> = grad((v w).sum(), n),  v = grad(E, n, create_graph=True) / dV        and        q_<key> = sum(w hv) dV
i.e. hv = (H w) / dV with H the Hessian of the energy in the grid values.
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
import hvp_cases  # noqa: E402

F = _import_reference()
DT = torch.double


def t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=DT)


def reference_terms(vext):
    return {
        'ion_electron': lambda b, d: F.IonElectron(b, d, vext), 'hartree': F.Hartree, 'tf': F.ThomasFermi, 'vw': F.Weizsaecker,
        'wt_nl': lambda b, d: F.non_local_KEF(b, d, 5 / 6, 5 / 6), 'lda_x': F.lda_exchange, 'pz_c': F.perdew_zunger_correlation,
        'pw_c': F.perdew_wang_correlation, 'chachiyo_c': F.chachiyo_correlation,
        'wgc98_nl': lambda b, d: F.non_local_KEF(b, d, (5 + hvp_cases.S5) / 6, (5 - hvp_cases.S5) / 6),
        'cfg1': lambda b, d: F.IonElectron(b, d, vext) + F.Hartree(b, d) + F.ThomasFermi(b, d) + F.Weizsaecker(b, d) + F.PerdewZunger(b, d),
        'cfg2': lambda b, d: F.IonElectron(b, d, vext) + F.Hartree(b, d) + F.WangTeter(b, d) + F.PerdewZunger(b, d),
        'wts_user': F.WangTeterStyleFunctional((5 / 6, 5 / 6, hvp_cases.user_stabiliser)),
    }


def hessian_vector(f, box, den, w):
    n = den.clone().requires_grad_()
    dV = torch.abs(torch.linalg.det(box)) / n.numel()
    v = torch.autograd.grad(f(box, n), n, create_graph=True)[0] / dV
    if not v.requires_grad:            # a functional linear in n: no second derivative
        return np.zeros(tuple(n.shape))
    return torch.autograd.grad((v * w).sum(), n)[0].detach().numpy()


def main():
    for case in hvp_cases.CASES:
        box, den, vext = hvp_cases.make_inputs(case)
        w = hvp_cases.direction(den.shape)
        dV = abs(np.linalg.det(box)) / den.size
        res = {'w': w, 'checksum': cases.checksum(box, den, w), 'rs_range': np.array(hvp_cases.rs_range(den))}
        for key, f in reference_terms(t(vext)).items():
            hv = hessian_vector(f, t(box), t(den), t(w))
            res['hv_' + key] = hv
            res['q_' + key] = float((w * hv).sum() * dV)
        path = os.path.join(HERE, 'hvp_%s.npz' % case)
        np.savez_compressed(path, **res)
        print(case, 'r_s %.3f .. %.3f' % tuple(res['rs_range']), os.path.getsize(path), 'bytes', flush=True)


if __name__ == '__main__':
    main()
