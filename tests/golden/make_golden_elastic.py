#!/usr/bin/env python3
"""Golden vectors of the second strain derivative at fixed chi, from the *reference*'s own double autograd.

Run from the repo root where the reference is present (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_elastic.py

Same in-memory stubs for the reference's absent third-party modules as make_golden_fc.py; only OUTPUTS of the reference are
written.  Fixtures (tests/golden/elastic_<case>.npz, cases of elastic_cases.py):
    w2_<term> [3, 3, 3, 3]  torch.autograd.functional.hessian in eps of E_t(chi, box (I + eps)), the closure of
                            System.__compute_elastic_constants (system.py:1266-1273) restricted to one term: the density is
                            N chi^2 / (mean(chi^2) vol(eps)) at fixed grid values of chi = sqrt(den), and for ion_electron the
                            potential is rebuilt by lattice_sum from the fixed fractional coordinates, with the reference's
                            interpolation of its al.gga.recpot on |k|(eps) (system.py:183-194)
    b_sum [6, n0, n1, n2]   the Jacobian of the closure gradient g = dE/dchi in eps_kl (kl = xx, yy, zz, yz, xz, xy; asserted
                            symmetric in kl) for the summed set elastic_cases.SUMMED; w1_sum [3, 3] = dE / d eps of that set
    cfix4 [3, 3, 3, 3]      the reference's own C recipe (system.py:1281-1337) applied to the summed set with chi held fixed, and
                            stress_sum [3, 3], the stress it forms on the way
    checksum                of the inputs
    b_nl_0709               (a16 only) the same Jacobian for non_local_KEF(0.7, 0.9) alone
and for a16, in elastic_a16_b.npz, b_<term> for the four terms with an explicit part (elastic_cases.EXPLICIT); in
elastic_grids.npz, w2_<grid>_<term> on the five further grids of elastic_cases.GRIDS with ions of two species.
The ion-ion energy is not here: the reference takes its pair list from torch-nl, which is absent (oracle/ionion.py).
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
    import professad.ion_utils as IU
    import professad.functional_tools as T
    return F, IU, T


import torch  # noqa: E402
import cases  # noqa: E402
import elastic_cases  # noqa: E402

F, IU, T = _import_reference()
DT = torch.double
RECPOT = '/root/reference/tests/potentials/al.gga.recpot'


def t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=DT)


def eps_hessian(tb, chi, n_elec, f):
    def energy(eps):
        b = tb @ (torch.eye(3, dtype=DT) + eps)
        vol = torch.abs(torch.linalg.det(b))
        d = (n_elec / (torch.mean(chi.pow(2)) * vol)) * chi.pow(2)
        return f(b, d).reshape(())
    return torch.autograd.functional.hessian(energy, torch.zeros(3, 3, dtype=DT)).numpy()


def grids():
    """W2^0_t on the grids of elastic_cases.GRIDS (two species: the second with half the table) -> elastic_grids.npz"""
    out = {}
    for name in elastic_cases.GRIDS:
        box, shape, den, ions_ = elastic_cases.grid_inputs(name)
        tb = t(box)
        chi = torch.sqrt(t(den))
        n_elec = float(den.mean() * abs(np.linalg.det(box)))

        def ion_electron(b, d):
            _kx, _ky, _kz, k2 = T.wavevecs(b, shape)
            k = torch.zeros(k2.shape, dtype=DT)
            k[k2 != 0] = torch.sqrt(k2[k2 != 0])
            vk = IU.interpolate_recpot(RECPOT, k)
            vext = sum(IU.lattice_sum(b, shape, t(fr) @ b, scale * vk, None) for fr, scale in ions_)
            return F.IonElectron(b, d, vext)

        fun = {'ion_electron': ion_electron, 'hartree': F.Hartree, 'tf': F.ThomasFermi, 'vw': F.Weizsaecker,
               'wt_nl': lambda b, d: F.non_local_KEF(b, d, 5 / 6, 5 / 6), 'lda_x': F.lda_exchange, 'pw_c': F.perdew_wang_correlation}
        for term in elastic_cases.GRID_TERMS:
            out['w2_%s_%s' % (name, term)] = eps_hessian(tb, chi, n_elec, fun[term])
        out['checksum_' + name] = cases.checksum(box, den, *[fr for fr, _s in ions_])
        print(name, {k.split('_', 2)[2]: '%.3e' % np.abs(v).max() for k, v in out.items() if k.startswith('w2_' + name)}, flush=True)
    path = os.path.join(HERE, 'elastic_grids.npz')
    np.savez_compressed(path, **out)
    print('grids', os.path.getsize(path), 'bytes', flush=True)


def main():
    if '--grids-only' not in sys.argv:
        full()
    grids()


def full():
    for case in elastic_cases.CASES:
        box, shape, frac, den, raw, k_max = elastic_cases.make_inputs(case)
        tb, tfrac = t(box), t(frac)
        chi = torch.sqrt(t(den))
        n_elec = float(den.mean() * abs(np.linalg.det(box)))

        def ion_electron(b, d):
            _kx, _ky, _kz, k2 = T.wavevecs(b, shape)
            k = torch.zeros(k2.shape, dtype=DT)
            k[k2 != 0] = torch.sqrt(k2[k2 != 0])
            vext = IU.lattice_sum(b, shape, tfrac @ b, IU.interpolate_recpot(RECPOT, k), None)
            return F.IonElectron(b, d, vext)

        fun = {'ion_electron': ion_electron, 'hartree': F.Hartree, 'tf': F.ThomasFermi, 'vw': F.Weizsaecker,
               'wt_nl': lambda b, d: F.non_local_KEF(b, d, 5 / 6, 5 / 6),
               'nl_0709': lambda b, d: F.non_local_KEF(b, d, *elastic_cases.AB2),
               'lda_x': F.lda_exchange, 'pz_c': F.perdew_zunger_correlation, 'pw_c': F.perdew_wang_correlation,
               'chachiyo_c': F.chachiyo_correlation}
        out = {}
        for key in elastic_cases.TERMS:
            def energy(eps, f=fun[key]):
                b = tb @ (torch.eye(3, dtype=DT) + eps)
                vol = torch.abs(torch.linalg.det(b))
                d = (n_elec / (torch.mean(chi.pow(2)) * vol)) * chi.pow(2)
                return f(b, d).reshape(())

            w2 = torch.autograd.functional.hessian(energy, torch.zeros(3, 3, dtype=DT)).numpy()
            out['w2_' + key] = w2
            print(case, key, 'max|W2| %.6e  asym(mn<->pq) %.1e' % (np.abs(w2).max(), np.abs(w2 - w2.transpose(2, 3, 0, 1)).max()), flush=True)
        # the summed set: first derivative, the Jacobian of the closure gradient in eps and the reference's own C recipe at fixed chi
        eye = torch.eye(3, dtype=DT)

        def closure_energy(x, eps, names):
            b = tb @ (eye + eps)
            vol = torch.abs(torch.linalg.det(b))
            d = (n_elec / (torch.mean(x.pow(2)) * vol)) * x.pow(2)
            return sum(fun[k](b, d).reshape(()) for k in names)

        def jacobian6(names):
            x = chi.clone().requires_grad_()
            eps = torch.zeros(3, 3, dtype=DT, requires_grad=True)
            dE = torch.autograd.grad(closure_energy(x, eps, names), eps, create_graph=True)[0]
            B = torch.stack([torch.stack([torch.autograd.grad(dE[i, j], x, retain_graph=True)[0] for j in range(3)]) for i in range(3)])
            asym = float((B - B.transpose(0, 1)).abs().max() / B.abs().max())
            assert asym < 1e-12, asym
            return torch.stack([B[i, j] for i, j in elastic_cases.VOIGT]).numpy(), dE.detach().numpy()

        out['b_sum'], out['w1_sum'] = jacobian6(elastic_cases.SUMMED)
        # the Birch coefficients of system.py:1281-1337 with chi held fixed: the stress as a function of the lattice vectors, its
        # Jacobian, contracted with the lattice vectors and symmetrised in the strain indices
        vol0 = torch.abs(torch.linalg.det(tb))

        def sigma(h):
            d = (n_elec / (torch.mean(chi.pow(2)) * torch.abs(torch.linalg.det(h)))) * chi.pow(2)
            E = sum(fun[k](h, d).reshape(()) for k in elastic_cases.SUMMED)
            g = torch.autograd.grad(E, h, create_graph=True)[0]
            return torch.einsum('ai,aj->ij', g, h) / torch.abs(torch.linalg.det(h))

        J = torch.autograd.functional.jacobian(sigma, tb.clone())                   # [i, j, a, b] = d sigma_ij / d h_ab
        C4 = torch.einsum('ijak,al->ijkl', J, tb)
        C4 = (0.5 * (C4 + C4.transpose(2, 3))).numpy()
        out['cfix4'] = C4
        out['stress_sum'] = sigma(tb.clone().requires_grad_()).detach().numpy()
        if case == 'a16':       # the alpha != beta instance alone: the second convolution family of the strain gradient
            out['b_nl_0709'] = jacobian6(['nl_0709'])[0]
        print(case, 'summed: max|B| %.3e max|Cfix| %.3e vol %.6f' % (np.abs(out['b_sum']).max(), np.abs(C4).max(), float(vol0)), flush=True)
        path = os.path.join(HERE, 'elastic_%s.npz' % case)
        np.savez_compressed(path, checksum=cases.checksum(box, frac, den, raw), **out)
        print(case, os.path.getsize(path), 'bytes', flush=True)
        if case == 'a16':       # per term, for the four terms with an explicit part
            per = {'b_' + k: jacobian6([k])[0] for k in elastic_cases.EXPLICIT}
            path = os.path.join(HERE, 'elastic_%s_b.npz' % case)
            np.savez_compressed(path, checksum=cases.checksum(box, frac, den, raw), **per)
            print(case, 'per-term B', os.path.getsize(path), 'bytes', flush=True)


if __name__ == '__main__':
    main()
