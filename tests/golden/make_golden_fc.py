#!/usr/bin/env python3
"""Golden vectors of the force-constant pieces, from the *reference*'s own double autograd.

Run from the repo root where the reference is present (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fc.py

Same in-memory stubs for the reference's absent third-party modules as make_golden_hvp.py; only OUTPUTS of the reference are
written.  Fixtures (tests/golden/fc_<case>.npz, cases of fc_cases.py):
    dv     [3, n0, n1, n2]  the Jacobian of lattice_sum(box, shape, cart, v~, None) with respect to the Cartesian coordinates of
                            the ONE ion fc_cases.ION[case] (ion_utils.py:88-137)
    hess   [N, 3, N, 3]     torch.autograd.functional.hessian of U(R) = IonElectron(box, den, lattice_sum(R)) at the seeded density
                            (its off-diagonal blocks are asserted to vanish)
    checksum                of the inputs
The reciprocal-space potential is the reference's own interpolation of its al.gga.recpot (make_golden.py:272-320 does the same).
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
import fc_cases  # noqa: E402

F, IU, T = _import_reference()
DT = torch.double
RECPOT = '/root/reference/tests/potentials/al.gga.recpot'


def t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=DT)


def main():
    for case in fc_cases.CASES:
        box, shape, frac, den, raw, k_max = fc_cases.make_inputs(case)
        tb, tden = t(box), t(den)
        _kx, _ky, _kz, k2 = T.wavevecs(tb, shape)
        k = torch.zeros(k2.shape, dtype=DT)
        k[k2 != 0] = torch.sqrt(k2[k2 != 0])
        vk = IU.interpolate_recpot(RECPOT, k)
        cart = t(frac) @ tb
        a = fc_cases.ION[case]

        def potential(ra):
            full = torch.cat([cart[:a], ra[None, :], cart[a + 1:]], dim=0)
            return IU.lattice_sum(tb, shape, full, vk, None)

        dv = torch.autograd.functional.jacobian(potential, cart[a].clone())          # [n0, n1, n2, 3]
        dv = dv.permute(3, 0, 1, 2).contiguous().numpy()
        hess = torch.autograd.functional.hessian(lambda R: F.IonElectron(tb, tden, IU.lattice_sum(tb, shape, R, vk, None)), cart.clone())
        hess = hess.numpy()
        n = frac.shape[0]
        off = max(np.abs(hess[p, :, b, :]).max() for p in range(n) for b in range(n) if p != b)
        assert off == 0.0 or off < 1e-14 * np.abs(hess).max(), off
        path = os.path.join(HERE, 'fc_%s.npz' % case)
        np.savez_compressed(path, dv=dv, hess=hess, ion=np.int64(a), checksum=cases.checksum(box, frac, den, raw))
        print(case, 'max|dv| %.3e max|hess| %.3e off-diagonal %.1e' % (np.abs(dv).max(), np.abs(hess).max(), off),
              os.path.getsize(path), 'bytes', flush=True)


if __name__ == '__main__':
    main()
