#!/usr/bin/env python3
"""Golden vectors of the chi-space Hessian-vector product, the truncated-Newton ground state and the density response for
WGC99 + PBE (cfg3w of hvp_wgc_cases.py), from the *reference*'s own double autograd.

Run from the repo root where the reference is present (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_tn_wgc.py

make_golden_tn_gga.py with F.WangGovindCarter99() in place of F.WangTeter: same stubs, same inputs (tn_cases.make_inputs), same
host logic (optimize.TruncatedNewton, tn_double.NumpyCgBackend's sweeps, optimize.density_response) around the reference's
derivatives; only OUTPUTS of the reference are written.  Fixtures (tests/golden/tn_wgc_<case>.npz, cases of tn_cases.py):
    g, Hd, dHd           at phi = 1.7 sqrt(den) along d = hvp_cases.direction(shape, seed=81)
    checksum             of the inputs
and for hvp_wgc_cases.GS_CASES (g16r, g18t; on g17r the line search of this driver stalls at |g|_2 = 9.8e-9)
    chi_gs, E_gs, gnorm  the ground state from the uniform density, run to |g|_2 < 3e-12
    dn, dmu, cg_iters    the response to tn_cases.response_dv at that ground state, conjugate gradients to 1e-12
    counts               outer iterations, energy evaluations, products of the run at the first |g|_2 <= 1e-10
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden_tn as M  # noqa: E402  (the stubs, the reference import, Reference and ReferenceBackend)
import cases  # noqa: E402
import hvp_wgc_cases  # noqa: E402
import tn_cases  # noqa: E402
from professad_amd import optimize  # noqa: E402

F = M.F


class ReferenceWgc(M.Reference):
    def __init__(self, box, vext, n_elec):
        super().__init__(box, vext, n_elec)
        self.wgc = F.WangGovindCarter99()

    def functional(self, den):
        b = self.box
        return F.IonElectron(b, den, self.vext) + F.Hartree(b, den) + self.wgc(b, den) + F.PerdewBurkeErnzerhof(b, den)


def main():
    for case in hvp_wgc_cases.TN_CASES:
        box, phi, d, vext, n_elec = tn_cases.make_inputs(case)
        assert abs(n_elec % 1.0 - 0.5) >= hvp_wgc_cases.HALF_INTEGER_MARGIN, (case, n_elec)
        ref = ReferenceWgc(box, vext, n_elec)
        res = {'checksum': cases.checksum(box, phi, d, vext)}
        _E, g = ref.closure(phi)
        Hd = ref.hessian_vector_chi(phi, d)
        res.update(g=g, Hd=Hd, dHd=float((d * Hd).sum()))
        if case in hvp_wgc_cases.GS_CASES:
            vol = abs(np.linalg.det(box))
            chi = np.full(phi.shape, np.sqrt(n_elec / vol))
            backend = M.ReferenceBackend(ref, box, phi.shape)
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
            res.update(chi_gs=chi.copy(), E_gs=tn._at[0], gnorm=gn, counts=np.array(counts))
            dv = tn_cases.response_dv(phi.shape)
            r = optimize.density_response(None, chi, n_elec, dv, rtol=1e-12, maxiter=500, backend=backend)
            print(case, 'response: iterations', r['iterations'], 'residual %.2e' % r['rel_residual'], 'dmu %.6e' % r['dmu'], flush=True)
            res.update(dn=r['dn'], dmu=r['dmu'], cg_iters=r['iterations'])
        path = os.path.join(HERE, 'tn_wgc_%s.npz' % case)
        np.savez_compressed(path, **res)
        print(case, os.path.getsize(path), 'bytes', flush=True)


if __name__ == '__main__':
    main()
