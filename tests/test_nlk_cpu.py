"""CPU-side checks of the tabulated-kernel nonlocal functionals (KGAP, Mi-Genova-Pavanello, Xu-Wang-Ma): the drop-in names and
signatures, the term bit, both libraries' ABI, and a numpy restatement of the three kernel formulas the device's table builder
implements (csrc/pointwise_kernels.h: nlk_table_kernel, nlk_mgp_table_kernel) against the arrays the reference produced for
g16s (tests/golden/nlk_g16s.npz)."""
import inspect
import os

import numpy as np
import pytest
import torch

import cases
from professad_amd import _native as N
from professad_amd import functionals as F

GOLDEN = os.path.dirname(os.path.abspath(cases.__file__))
EV_PER_HA = 4.3597447222071e-18 / 1.602176634e-19


def test_names_signatures_and_qualnames():
    assert list(inspect.signature(F.KGAP).parameters) == ['box_vecs', 'den', 'E_gap', 'f']
    assert list(inspect.signature(F.XuWangMa).parameters) == ['box_vecs', 'den', 'kappa']
    assert inspect.signature(F.XuWangMa).parameters['kappa'].default == 0
    assert F.KGAP.__qualname__ == 'KGAP' and F.XuWangMa.__qualname__ == 'XuWangMa'
    assert list(inspect.signature(F.MiGenovaPavanello.__init__).parameters) == ['self', 'init_args']
    mgp = F.MiGenovaPavanello((0.2, 0.01))
    assert mgp.__qualname__ == mgp.__name__ == 'MiGenovaPavanello' and (mgp.a, mgp.b) == (0.2, 0.01)
    assert list(inspect.signature(mgp.forward).parameters) == ['box_vecs', 'den'] and callable(mgp)
    x = torch.linspace(-1, 1, 5, dtype=torch.double)
    assert torch.equal(inspect.signature(F.KGAP).parameters['f'].default(x), 1 + x)      # the reference's default f(x) = 1 + x


def test_stabiliser_detection_needs_no_device():
    assert F._stabiliser(lambda x: 1 + x) == (1.0, 0.0)
    assert F._stabiliser(torch.exp) == (1.0, 1.0)
    fp0, kind = F._stabiliser(lambda x: 1 + 2 * x + x * x)
    assert fp0 == 2.0 and kind is None
    with pytest.raises(ValueError):
        F._stabiliser(lambda x: 2 + x)
    # WangTeterStyleFunctional shares the detection
    assert F.WangTeterStyleFunctional((5 / 6, 5 / 6, torch.exp))._kind == 1.0
    assert F.WangTeterStyleFunctional()._kind == 0.0


def test_term_bit_and_slots():
    assert N.TERM_BITS['nlk'] == 1 << 14 and N.TERM_ORDER[14] == 'nlk' and N.NTERMS == 15
    assert (N.NLK_KGAP, N.NLK_MGP, N.NLK_XWM) == (1, 2, 3)
    assert F.NativeTerms(['tf', 'vw', 'nlk'], nlk_kind=3, nlk_p0=0.5).names == ('tf', 'vw', 'nlk')
    assert 'nlk' not in F.NativeTerms.ALIASES            # the kinds need parameters


def test_per_term_dicts_keep_their_entries_for_term_sets_without_nlk():
    """a term set without the new bit gets the fourteen entries it always got; 'nlk' appears only while it is set"""
    vals = list(range(N.NTERMS))
    assert list(N.per_term(vals, N.TERM_BITS['tf'] | N.TERM_BITS['wgc99_nl'])) == N.TERM_ORDER[:14]
    with_nlk = N.per_term(vals, N.TERM_BITS['tf'] | N.TERM_BITS['nlk'])
    assert list(with_nlk) == N.TERM_ORDER and with_nlk['nlk'] == 14


def test_both_libraries_build_and_export_the_abi():
    import __graft_entry__
    __graft_entry__.build()
    for dtype in (N.F64, N.F32):
        lib = N.load(dtype)
        for sym in N.EXPORTS:
            assert hasattr(lib, sym), sym
    header = open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'ofdft_hip.h')).read()
    for d in ('OFDFT_NLK ', 'OFDFT_P_NLK_KIND', 'OFDFT_P_NLK_P0', 'OFDFT_P_NLK_P1'):
        assert d in header


# ---- the kernel formulas, restated in numpy (what the device builder evaluates per k-point, in fp64)
def ginv_lind(eta):
    with np.errstate(divide='ignore', invalid='ignore'):
        g = 0.5 + ((1 - eta * eta) / (4 * eta)) * np.log(np.abs((1 + eta) / (1 - eta)))
    g = np.where(eta == 0, 1.0, g)
    return np.where(eta == 1, 0.5, g)


def ginv_gap(eta, delta):
    ap, am, d2 = 4 * (eta + eta * eta), 4 * (eta - eta * eta), delta * delta
    return 0.5 - delta * (np.arctan(ap / delta) + np.arctan(am / delta)) / (8 * eta) \
        + (d2 / 128 / eta ** 3 + 1 / 8 / eta - eta / 8) * np.log((d2 + ap * ap) / (d2 + am * am))


def torch_linspace(lo, hi, n):
    """torch.linspace in fp64: from the low end in the first half, from the high end in the second"""
    i = np.arange(n)
    step = (hi - lo) / (n - 1)
    return np.where(i < n // 2, lo + step * i, hi - step * (n - 1 - i))


def mgp_table(eta_hi, n_eta=2000, n_int=10000):
    ts = torch_linspace(1e-4, 1.0, n_int)
    dt = ts[1] - ts[0]
    etas = torch_linspace(0.0, eta_hi, n_eta)
    w = np.empty(n_eta)
    for i0 in range(0, n_eta, 200):
        e = etas[i0:i0 + 200, None] / ts[None, :] ** (1 / 3)
        w[i0:i0 + 200] = 0.2 * (3 * np.pi ** 2) ** (2 / 3) * np.sum((1 / ginv_lind(e) - 3 * e * e - 1) / ts[None, :] ** (1 / 6), axis=1) * dt
    return etas, w


@pytest.fixture(scope='module')
def g16s():
    gold = np.load(os.path.join(GOLDEN, 'nlk_g16s.npz'))
    box, den, _vext, _chi, _n = cases.make_inputs('g16s')
    assert abs(cases.checksum(box, den) - float(gold['checksum'])) < 1e-9
    vol = abs(np.linalg.det(box))
    return gold, vol, round(den.mean() * vol) / vol


def test_gap_kernel_restatement(g16s):
    gold, vol, n0 = g16s
    eta = gold['kgap_eta']
    kf = (3 * np.pi ** 2 * n0) ** (1 / 3)
    delta = 2 * (2.0 / EV_PER_HA) / kf ** 2
    nz = eta != 0
    k = np.zeros_like(eta)
    k[nz] = 1 / ginv_gap(eta[nz], delta) - 3 * eta[nz] ** 2 - 1
    err = np.abs(k - gold['kgap_kernel']).max() / np.abs(gold['kgap_kernel']).max()
    print('gap kernel: %.2e of the largest entry' % err)
    assert err <= KGAP_BOUND


def test_xwm_kernel1_restatement(g16s):
    gold, vol, n0 = g16s
    eta = gold['xwm_eta']
    g = ginv_lind(eta)
    nz = eta != 0
    gder = np.zeros_like(eta)
    gder[nz] = 0.5 - 0.25 * (eta[nz] + 1 / eta[nz]) * np.log(np.abs((1 + eta[nz]) / (1 - eta[nz])))
    k1 = np.pi ** 2 / (3 * np.pi ** 2) ** (1 / 3) / (6 * n0) * (gder / g ** 2 + 6 * eta ** 2)
    err = np.abs(k1 - gold['xwm_kernel1']).max() / np.abs(gold['xwm_kernel1']).max()
    print('XWM kernel1: %.2e of the largest entry' % err)
    assert err <= XWM_BOUND


def test_mgp_table_restatement(g16s):
    gold, vol, n0 = g16s
    nodes, w_ref = gold['mgp_table']
    etas, w = mgp_table(nodes[-1])
    assert np.abs(etas - nodes).max() <= 4e-16 * nodes[-1]
    err = np.abs(w - w_ref).max() / np.abs(w_ref).max()
    print('MGP table: %.2e of the largest entry' % err)
    assert err <= MGP_BOUND


# Bounds: ten times the difference between these numpy restatements and the reference's own (torch) arrays measured when the
# test was written -- another library's log / atan / pow, not another formula:
#   XWM kernel1  4.09e-14 of the largest entry                                  -> 4.1e-13
#   MGP table    3.6e-9 of the largest entry for a fp64 restatement on the reference's nodes (2.5e-8 with the pow of this one;
#                the sum cancels about eleven digits at eta / t^(1/3) ~ 300, and the reference's table differs from an 80-bit
#                evaluation of the same sum by 1.2e-7)                                                   -> 3.6e-8
#   gap kernel   0.0: numpy and torch gave the same bits here.  Ten times nothing is no bound for another libm, so this one is
#                the rounding error of the formula itself: 3 eta^2 (up to 540 at eta = 13.4) against an O(1) result loses
#                540 x 2^-52 = 1.2e-13 per operation, a handful of operations                              -> 1e-12
KGAP_BOUND = 1e-12
XWM_BOUND = 4.1e-13
MGP_BOUND = 3.6e-8
