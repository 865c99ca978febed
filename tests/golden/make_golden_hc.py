#!/usr/bin/env python3
"""Golden vectors of the Huang-Carter and revised Huang-Carter functionals, from the *reference*.

Run from the repo root where the reference is present (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_hc.py [case ...]

(no argument: every case of hc_cases.CASES and hc_cases.EDGE_CASES; otherwise only the cases named.)

Same in-memory stubs for the reference's absent third-party modules as make_golden.py, with one difference: the stand-in for
``xitorch.integrate.solve_ivp`` returns the values of professad_amd.hc_kernel.solve_kernel (xitorch is not installed where the
goldens are made), so the reference's own ``forward`` and autograd run on the table the engine gets.  The kernel table is
therefore the project's RK4 solution of the reference's initial-value problem, not xitorch's.  ``debug = False`` is set on the
HuangCarter instance: the reference's class never defines the attribute its ``forward`` reads (functionals.py:1247).
Only OUTPUTS of the reference are written.  Fixtures (tests/golden/hc_<case>.npz), per kind key k in hc_cases.KINDS:
  k_E, k_v          the functional's total (vW + TF + T_NL) and its functional derivative
  k_E_nl, k_v_nl    T_NL = E - E_vW - E_TF and its derivative
  k_xi_min, k_xi_max, k_lower, k_M     the spline's node set as field_dependent_convolution formed it
  k_table           w(eta) on linspace(0, ETA_MAX, N_ETA) (the table depends on beta only: in the first case's file)
  checksum          of the inputs
The cases of hc_cases.EDGE_CASES store k_E, k_E_nl, k_v_nl, the node set and the checksum only.  One that names a table gets it
from the reference's own generate_kernel(eta_max, N_eta) (through the stand-in above); one that names a kappa gets an instance
with that kappa in its init_args.

Node-set margin: neither ceil argument of the node formulas may lie within 1e-6 of an integer, so that a rounding-level
difference in xi_min / xi_max cannot change the node set (asserted; if a case ever fails, scale its density by 1.01).
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

import torch  # noqa: E402

from professad_amd import hc_kernel  # noqa: E402


def _solve_ivp(fcn, ts, y0, params=()):
    """the values of hc_kernel.solve_kernel on the reference's nodes `ts` (eta_max down to eta[1]), as [len(ts), 1]"""
    beta = float(params[0])
    n_eta = len(ts) + 1
    eta, w = hc_kernel.solve_kernel(beta, float(ts[0]), n_eta)
    assert np.allclose(eta[:0:-1], ts.numpy(), rtol=0, atol=1e-12)
    return torch.from_numpy(np.ascontiguousarray(w[:0:-1])).unsqueeze(1)


def _import_reference():
    def _absent(*a, **k):
        raise NotImplementedError('stubbed third-party dependency (not on the hot path)')

    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m

    stub('xitorch')
    stub('xitorch.integrate', solve_ivp=_solve_ivp)
    stub('xitorch.optimize', minimize=_absent)
    stub('torch_nl', compute_neighborlist=_absent)
    sys.path.insert(0, '/root/reference/src')
    import professad.functionals as F
    import professad.functional_tools as T
    return F, T


import hc_cases  # noqa: E402
import cases  # noqa: E402

F, T = _import_reference()


def evaluate(f, box, den):
    """-> E, v, E_nl, v_nl (per volume element) of the reference instance f"""
    b = torch.as_tensor(box)
    dV = abs(np.linalg.det(box)) / den.size
    d = torch.as_tensor(den).clone().requires_grad_()
    E = f.forward(b, d)
    E_rest = F.Weizsaecker(b, d) + F.ThomasFermi(b, d)
    (v,) = torch.autograd.grad(E, d, retain_graph=True)
    (v_rest,) = torch.autograd.grad(E_rest, d)
    return E.item(), v.numpy() / dV, (E - E_rest).item(), (v - v_rest).numpy() / dV


def instance(cls, args, table=None):
    with torch.no_grad():
        f = getattr(F, cls)(args)
        f.debug = False
        if table:
            f.generate_kernel(*table)
    return f


def main():
    only = sys.argv[1:]
    funcs = {key: instance(cls, args) for key, (cls, args, _p) in hc_cases.KINDS.items()}
    seen = {}
    orig = T.field_dependent_convolution

    def spy(k, f, g, xis, kappa, mode='arithmetic'):
        seen['xi'] = (xis.min().item(), xis.max().item())
        return orig(k, f, g, xis, kappa, mode)
    F.field_dependent_convolution = spy
    margin = 1.0

    def node_fields(case, key, kappa):
        nonlocal margin
        xi_min, xi_max = seen['xi']
        lower, M, a, bb = hc_cases.node_set(xi_min, xi_max, kappa)
        dist = min(abs(a - round(a)), abs(bb - round(bb)))
        assert dist > 1e-6, (case, key, a, bb)
        margin = min(margin, dist)
        return {key + '_xi_min': xi_min, key + '_xi_max': xi_max, key + '_lower': lower, key + '_M': M}

    for case in hc_cases.CASES:
        if only and case not in only:
            continue
        box, den = hc_cases.make_inputs(case)
        out = dict(checksum=cases.checksum(box, den))
        for key, f in funcs.items():
            E, v, E_nl, v_nl = evaluate(f, box, den)
            out.update({key + '_E': E, key + '_v': v, key + '_E_nl': E_nl, key + '_v_nl': v_nl})
            out.update(node_fields(case, key, hc_cases.kappa_of(key)))
            if case == hc_cases.CASES[0]:          # the table depends on beta only: stored once
                out[key + '_table'] = f.kernel[1].numpy()
            print('%s %-5s E %.12e E_nl %.6e max|v_nl| %.3e xi %.4f .. %.4f M %d' % (case, key, E, E_nl, np.abs(v_nl).max(),
                                                                                 out[key + '_xi_min'], out[key + '_xi_max'], out[key + '_M']))
        np.savez_compressed(os.path.join(HERE, 'hc_%s.npz' % case), **out)
    for case, spec in hc_cases.EDGE_CASES.items():
        if only and case not in only:
            continue
        box, den = hc_cases.make_inputs(spec['grid'])
        out = dict(checksum=cases.checksum(box, den))
        for key in spec['keys']:
            args = hc_cases.edge_args(case, key)
            f = instance(hc_cases.KINDS[key][0], args, spec['table'])
            assert tuple(f.kernel.shape) == (2, hc_cases.edge_table(case)[1]) and float(f.kernel[0, -1]) == hc_cases.edge_table(case)[0]
            E, _v, E_nl, v_nl = evaluate(f, box, den)
            out.update({key + '_E': E, key + '_E_nl': E_nl, key + '_v_nl': v_nl})
            out.update(node_fields(case, key, args[-1]))
            print('%s %-5s E %.12e E_nl %.6e max|v_nl| %.3e xi %.4f .. %.4f M %d' % (case, key, E, E_nl, np.abs(v_nl).max(),
                                                                                 out[key + '_xi_min'], out[key + '_xi_max'], out[key + '_M']))
        np.savez_compressed(os.path.join(HERE, 'hc_%s.npz' % case), **out)
    print('smallest distance of a ceil argument to an integer: %.4f' % margin)


if __name__ == '__main__':
    main()
