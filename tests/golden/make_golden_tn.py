#!/usr/bin/env python3
"""Golden vectors of the chi-space Hessian-vector product, the truncated-Newton ground state and the density response, from
the *reference*'s own double autograd.

Run from the repo root where the reference is present (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_tn.py

Same in-memory stubs for the reference's absent third-party modules as make_golden_hvp.py; only OUTPUTS of the reference are
written.  Every derivative below is the reference's: E[chi] is its closure energy (system.py:846-848) of cfg2's functionals,
g = grad(E, chi) and H d = grad((g d).sum(), chi).  The outer iteration (optimize.TruncatedNewton), the conjugate-gradient
sweeps (tn_double.NumpyCgBackend) and optimize.density_response are this project's host logic driven by those derivatives.
Fixtures (tests/golden/tn_<case>.npz, cases of tn_cases.py):
    g, Hd, dHd           at phi = 1.7 sqrt(den) along d = hvp_cases.direction(shape, seed=81)
    chi_gs, E_gs, gnorm  the ground state from the uniform density, run to |g|_2 < 3e-12
    dn, dmu, cg_iters    the response to tn_cases.response_dv at that ground state, conjugate gradients to 1e-12
    counts (g16r)        outer iterations, energy evaluations, products of the run at the first |g|_2 <= 1e-10, and per solve
    checksum             of the inputs
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
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
import tn_cases  # noqa: E402
import tn_double  # noqa: E402
from professad_amd import optimize  # noqa: E402

F = _import_reference()
DT = torch.double


def t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=DT)


class Reference:
    """E[chi], its gradient and Hessian-vector products by the reference's autograd"""

    def __init__(self, box, vext, n_elec):
        self.box, self.vext, self.n_elec = t(box), t(vext), n_elec
        self.vol = torch.abs(torch.linalg.det(self.box))

    def functional(self, den):
        b = self.box
        return F.IonElectron(b, den, self.vext) + F.Hartree(b, den) + F.WangTeter(b, den) + F.PerdewZunger(b, den)

    def energy(self, chi):
        den = (self.n_elec / (torch.mean(chi.pow(2)) * self.vol)) * chi.pow(2)          # system.py:846-847
        return self.functional(den)

    def closure(self, chi):
        x = t(chi).requires_grad_()
        E = self.energy(x)
        return float(E), torch.autograd.grad(E, x)[0].numpy()

    def hessian_vector_chi(self, chi, d):
        x = t(chi).requires_grad_()
        g = torch.autograd.grad(self.energy(x), x, create_graph=True)[0]
        return torch.autograd.grad((g * t(d)).sum(), x)[0].numpy()

    def hessian_vector(self, den, w):
        n = t(den).requires_grad_()
        dV = self.vol / n.numel()
        v = torch.autograd.grad(self.functional(n), n, create_graph=True)[0] / dV
        return torch.autograd.grad((v * t(w)).sum(), n)[0].numpy()


class ReferenceBackend(tn_double.NumpyCgBackend):
    """the numpy sweeps around the reference's products"""

    def __init__(self, ref, box, shape):
        super().__init__(box, shape, tn_cases.TERMS)
        self.ref = ref

    def product(self, phi, g, n_elec, reuse):
        self.q = self.ref.hessian_vector_chi(phi, self.p)
        self.products += 1
        return float((self.p * self.q).sum()), float((phi * self.q).sum())

    def hv(self, den, w):
        return self.ref.hessian_vector(den, w)


def main():
    for case in tn_cases.CASES:
        box, phi, d, vext, n_elec = tn_cases.make_inputs(case)
        ref = Reference(box, vext, n_elec)
        res = {'checksum': cases.checksum(box, phi, d, vext)}
        _E, g = ref.closure(phi)
        Hd = ref.hessian_vector_chi(phi, d)
        res.update(g=g, Hd=Hd, dHd=float((d * Hd).sum()))
        # ground state from the uniform density
        vol = abs(np.linalg.det(box))
        chi = np.full(phi.shape, np.sqrt(n_elec / vol))
        backend = ReferenceBackend(ref, box, phi.shape)
        tn = optimize.TruncatedNewton(chi, backend, n_elec, cg_maxiter=50, tolerance_grad=3e-12)
        counts = None
        for _outer in range(30):
            tn.step(lambda: ref.closure(chi))
            gn = float(np.linalg.norm(tn._at[1]))
            print(case, 'outer', tn.total_iter, 'evals', tn.func_evals, 'products', tn.hvp_count, '|g|_2 %.2e' % gn, flush=True)
            if counts is None and gn <= 1e-10:
                counts = (tn.total_iter, tn.func_evals, tn.hvp_count)
            if gn < 3e-12:
                break
        assert gn < 3e-12
        res.update(chi_gs=chi.copy(), E_gs=tn._at[0], gnorm=gn)
        if case == 'g16r':
            res.update(counts=np.array(counts), cg_products=np.array([c[0] for c in tn.cg_log]))
        # response
        dv = tn_cases.response_dv(phi.shape)
        r = optimize.density_response(None, chi, n_elec, dv, rtol=1e-12, maxiter=500, backend=backend)
        print(case, 'response: iterations', r['iterations'], 'residual %.2e' % r['rel_residual'], 'dmu %.6e' % r['dmu'],
              'sum dn / sum |dn| %.1e' % (r['dn'].sum() / np.abs(r['dn']).sum()), flush=True)
        res.update(dn=r['dn'], dmu=r['dmu'], cg_iters=r['iterations'])
        path = os.path.join(HERE, 'tn_%s.npz' % case)
        np.savez_compressed(path, **res)
        print(case, os.path.getsize(path), 'bytes', flush=True)


if __name__ == '__main__':
    main()
