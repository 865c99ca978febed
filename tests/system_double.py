"""numpy double of what professad's System differentiates, assembled only from oracle/ (closed_form, stress, ions; refpath stands
behind the closure of tests/test_dropin_gradients_gpu.py), so that the drop-in layer -- professad_amd/functionals.py and
professad_amd/ions.py with real species lists -- can be compared with one object per (cell, density):

  * `CALLABLES`: every public callable of professad_amd.functionals that has an oracle, as (id, factory(F) -> callable,
    double(D) -> (E, dE/dn, sigma)); `evaluate` returns the three per term and their sum;
  * `species_potential`, `species_forces`, `species_stress`: v_ext, the ion-electron forces and the ion-electron stress of a
    species list, summed species by species (each is linear in the species);
  * `second_recpot`: a synthetic raw table whose length, k_max and charge all differ from tests/golden/ions.npz;
  * the comparison helpers the GPU files assert with (`check_field`, `check_stress`, `check_forces`), so that
    tests/test_system_double_cpu.py can show on the CPU that each of them rejects a perturbed double.

Not the product: nothing in professad_amd imports it.
"""
import math
import os

import numpy as np

import spectral_check as sc
from oracle import closed_form as cf
from oracle import ions as oi
from oracle import stress as st

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
S5 = math.sqrt(5.0)
WGC98 = ((5 + S5) / 6, (5 - S5) / 6)
WGC99_OTHER = (1.1, 0.7, 3.2, 0.9)              # non-default init_args: u = 3.8, v = u^2 - 36 alpha beta = -13.28 (not degenerate)
NLKEF_AB = (0.7, 0.9)                           # non_local_KEF with alpha != beta

# the project's bounds (tests/test_gpu_parity.py, tests/test_geometry_step_extents_gpu.py)
SIG_RTOL, ION_SIG_RTOL, ION_RTOL = 2e-10, 1e-10, 1e-11


# ------------------------------------------------------------------------------------------------------------- recpot tables
def golden_recpot():
    """(raw, k_max) of the reference's al.gga.recpot as stored in tests/golden/ions.npz (10002 points, k_max = 30, z = 3)"""
    g = np.load(os.path.join(GOLDEN, 'ions.npz'))
    return g['recpot_raw'], float(g['recpot_kmax'])


SECOND_Z, SECOND_KMAX, SECOND_LEN = 5, 9.0, 1537


def second_recpot():
    """(raw, k_max, z): a smooth analytic local pseudopotential in k, in the raw layout recpot_table expects (the Coulomb part
    -4 pi z / k^2 included for k > 0, the finite k -> 0 limit of the remainder at index 0):

        raw(k) = -4 pi z / k^2 exp(-(k rc)^2 / 4) + A (1 - (k rb)^2) exp(-(k rb)^2 / 4),   raw(0) = pi z rc^2 + A

    (a Gaussian-screened Coulomb attraction plus a short-ranged repulsive core).  1537 points up to k_max = 9 bohr^-1, z = 5: the
    grids of the tests (about 0.24 bohr per step, |k| up to ~22 bohr^-1) reach far beyond this table's end, where
    interpolate_recpot (ion_utils.py:74-81) clamps, and stay inside the golden table (k_max = 30)."""
    z, rc, A, rb = SECOND_Z, 0.55, 3.0, 0.8
    k = np.linspace(0.0, SECOND_KMAX, SECOND_LEN)
    raw = np.empty(SECOND_LEN)
    raw[1:] = (-4 * math.pi * z / k[1:] ** 2 * np.exp(-(k[1:] * rc) ** 2 / 4)
               + A * (1 - (k[1:] * rb) ** 2) * np.exp(-(k[1:] * rb) ** 2 / 4))
    raw[0] = math.pi * z * rc * rc + A
    return raw, SECOND_KMAX, z


def charge_off_by_one(raw, k_max):
    """the raw table of the same pseudopotential with one more unit of charge in its Coulomb part"""
    ks = np.linspace(0.0, k_max, raw.size)
    out = raw.copy()
    out[1:] -= 4 * math.pi / ks[1:] ** 2
    return out


def clamp_census(box, shape, k_max):
    """(k-points with 0 < |k| < k_max, k-points with |k| > k_max) of the half grid: the two branches of the table clamp"""
    kabs = np.sqrt(cf.recip(np.asarray(box, dtype=np.float64), shape)[3])
    return int(((kabs > 0) & (kabs < k_max)).sum()), int((kabs > k_max).sum())


# --------------------------------------------------------------------------------------------------------------- ion routines
# species: list of (frac [n, 3], (raw, k_max)); `order`: None (exact structure factor) or the PME order
def species_potential(box, shape, species, order=None):
    return sum(oi.ionic_potential(box, shape, f, raw, km, order) for f, (raw, km) in species)


def species_forces(box, den, species, order=None):
    """list of [n, 3], one per species (a force belongs to its ion: nothing to sum)"""
    return [oi.ion_electron_forces(box, den.shape, f, den, raw, km, order) for f, (raw, km) in species]


def species_stress(box, den, species, order=None):
    return sum(st.ion_electron(box, den, f, raw, km, order) for f, (raw, km) in species)


def species_energy(box, den, species, order=None):
    return float(np.mean(den * species_potential(box, den.shape, species, order)) * abs(np.linalg.det(box)))


def tables(species):
    """the species list as professad_amd.ions takes it: (frac, (ks, v, z))"""
    return [(f, oi.recpot_table(raw, km)) for f, (raw, km) in species]


# ------------------------------------------------------------------------------------------------------------------ functionals
class Evaluator(cf.Evaluator):
    """oracle.closed_form.Evaluator with the Lindhard factor of the Wang-Teter kernel, 1 / G^-1(eta) - 3 eta^2 - 1
    (functionals.py:617-628,648), evaluated in extended precision.  The formula cancels twice for large eta (G^-1 = 0.5 - 0.5 +
    O(eta^-2), then 1 / G^-1 against 3 eta^2): in fp64 it carries an absolute error of up to 6.5e-11 at eta = 12, where the
    full-spectrum grids of these tests reach -- next to TF and vW that is nothing, in the potential of non_local_KEF alone it
    is 1e-11 of the maximum, above spectral_check.V_TOL (the engine's fp64 factor takes a series from eta = 3 on).  x87 long double
    (eps 1.1e-19) leaves 3e-14; where long double is fp64 the class is the oracle's own."""

    def _wt_kernel(self, nbar, alpha, beta):
        L = np.longdouble
        kf = (3 * cf.PI * cf.PI * nbar) ** (1 / 3)
        eta = np.where(self.g.k2 != 0, np.sqrt(self.g.k2.astype(L)) / L(2 * kf), L(0))
        with np.errstate(divide='ignore', invalid='ignore'):
            g = L(0.5) + ((1 - eta ** 2) / (4 * eta)) * np.log(np.abs((1 + eta) / (1 - eta)))
        g = np.where(eta == 0, L(1), np.where(eta == 1, L(0.5), g))
        return (5 / (9 * alpha * beta * nbar ** (alpha + beta - 5 / 3)) * (1 / g - 3 * eta ** 2 - 1)).astype(np.float64)


class D:
    """the oracle pieces of one (cell, density): every method returns (E, dE/dn, sigma)"""

    def __init__(self, box, n):
        self.box, self.n = np.asarray(box, dtype=np.float64), np.asarray(n, dtype=np.float64)
        self.g = cf.Grid(self.box, self.n.shape)
        self.ev = Evaluator(self.g)

    def hartree(self):
        return self.ev.hartree(self.n) + (st.hartree(self.box, self.n),)

    def tf(self):
        return self.ev.tf(self.n) + (st.tf(self.box, self.n),)

    def vw(self):
        return self.ev.vw(self.n) + (st.vw(self.box, self.n),)

    def wt_nl(self, a, b):
        return self.ev.wt_nl(self.n, a, b) + (st.wt_nl(self.box, self.n, a, b),)

    def wt_family(self, a, b):
        return add(self.tf(), self.vw(), self.wt_nl(a, b))

    def wgc99(self, params=None):
        ev = self.ev if params is None else Evaluator(self.g, params)
        return add(self.tf(), self.vw(), ev.wgc99_nl(self.n) + (st.wgc99_nl(self.box, self.n, params),))

    def lda(self, name):
        return getattr(self.ev, name)(self.n) + (st.lda(self.box, self.n, name),)

    def pbe(self, x, c):
        return self.ev.pbe(self.n, do_x=x, do_c=c) + (st.pbe(self.box, self.n, x, c),)

    def vwgtf(self, kind):
        return self.ev.term('vwgtf%d' % kind, self.n) + (st.vw(self.box, self.n) + st.vwgtf(self.box, self.n, kind),)

    def lkt(self):
        return self.ev.term('lkt', self.n) + (st.vw(self.box, self.n) + st.ggak(self.box, self.n, 'lkt'),)

    def pauli_gaussian(self, name, mu, beta, lam, sigma):
        return self.ev.term(name, self.n) + (st.vw(self.box, self.n) + st.pauli_gaussian(self.box, self.n, mu, beta, lam, sigma),)

    def wt_style(self, a, b, f, df, fprime0):
        """functionals.py:728-782: T = vW + T_TF f(X), X = T_NL / (f'(0) T_TF)
        -> v = v_vW + v_TF (f - f' X) + v_NL f'(X) / f'(0), and the same weights on the stresses (tools_for_tests.py:310-364)"""
        (Ev, vv, sv), (Et, vt, s_t), (En, vn, sn) = self.vw(), self.tf(), self.wt_nl(a, b)
        X = En / (fprime0 * Et)
        fx, dfx = f(X), df(X)
        w_t, w_n = fx - dfx * X, dfx / fprime0
        return Ev + Et * fx, vv + vt * w_t + vn * w_n, sv + s_t * w_t + sn * w_n


def add(*parts):
    return sum(p[0] for p in parts), sum(p[1] for p in parts), sum(p[2] for p in parts)


def user_f(t):
    """the user's stabilisation function of the WangTeterStyleFunctional case: f(0) = 1, f'(0) = 2, neither 1 + x nor exp (works on
    torch tensors and on floats alike)"""
    return 1 + 2 * t + t * t


def _wgc99(F, init_args=None, forward=False):
    o = F.WangGovindCarter99() if init_args is None else F.WangGovindCarter99(init_args=init_args)
    return o.forward if forward else o


def _pg(F, setter):
    o = F.PauliGaussian()
    getattr(o, setter)()
    return o


def _wts(F, f):
    return F.WangTeterStyleFunctional(init_args=(5 / 6, 5 / 6, f))


def _torch_exp(F):
    import torch
    return torch.exp


# (id, factory(F = professad_amd.functionals) -> callable f(box_vecs, den), double(D) -> (E, dE/dn, sigma))
CALLABLES = [
    ('Hartree', lambda F: F.Hartree, lambda d: d.hartree()),
    ('ThomasFermi', lambda F: F.ThomasFermi, lambda d: d.tf()),
    ('Weizsaecker', lambda F: F.Weizsaecker, lambda d: d.vw()),
    ('non_local_KEF', lambda F: (lambda b, n: F.non_local_KEF(b, n, *NLKEF_AB)), lambda d: d.wt_nl(*NLKEF_AB)),
    ('WangTeter', lambda F: F.WangTeter, lambda d: d.wt_family(5 / 6, 5 / 6)),
    ('Perrot', lambda F: F.Perrot, lambda d: d.wt_family(1.0, 1.0)),
    ('SmargiassiMadden', lambda F: F.SmargiassiMadden, lambda d: d.wt_family(0.5, 0.5)),
    ('WangGovindCarter98', lambda F: F.WangGovindCarter98, lambda d: d.wt_family(*WGC98)),
    ('WGC99', lambda F: _wgc99(F), lambda d: d.wgc99()),
    ('WGC99.forward', lambda F: _wgc99(F, forward=True), lambda d: d.wgc99()),
    ('WGC99-other', lambda F: _wgc99(F, WGC99_OTHER), lambda d: d.wgc99(WGC99_OTHER)),
    ('WGC99-other.forward', lambda F: _wgc99(F, WGC99_OTHER, forward=True), lambda d: d.wgc99(WGC99_OTHER)),
    ('lda_exchange', lambda F: F.lda_exchange, lambda d: d.lda('lda_x')),
    ('perdew_zunger_correlation', lambda F: F.perdew_zunger_correlation, lambda d: d.lda('pz_c')),
    ('perdew_wang_correlation', lambda F: F.perdew_wang_correlation, lambda d: d.lda('pw_c')),
    ('chachiyo_correlation', lambda F: F.chachiyo_correlation, lambda d: d.lda('chachiyo_c')),
    ('PerdewZunger', lambda F: F.PerdewZunger, lambda d: add(d.lda('lda_x'), d.lda('pz_c'))),
    ('PerdewWang', lambda F: F.PerdewWang, lambda d: add(d.lda('lda_x'), d.lda('pw_c'))),
    ('Chachiyo', lambda F: F.Chachiyo, lambda d: add(d.lda('lda_x'), d.lda('chachiyo_c'))),
    ('pbe_exchange', lambda F: F.pbe_exchange, lambda d: d.pbe(True, False)),
    ('pbe_correlation', lambda F: F.pbe_correlation, lambda d: d.pbe(False, True)),
    ('PerdewBurkeErnzerhof', lambda F: F.PerdewBurkeErnzerhof, lambda d: d.pbe(True, True)),
    ('vWGTF1', lambda F: F.vWGTF1, lambda d: d.vwgtf(1)),
    ('vWGTF2', lambda F: F.vWGTF2, lambda d: d.vwgtf(2)),
    ('LuoKarasievTrickey', lambda F: F.LuoKarasievTrickey, lambda d: d.lkt()),
    ('PG1', lambda F: _pg(F, 'set_PG1'), lambda d: d.pauli_gaussian('pg1', 1.0, 0.0, 0.0, 0.0)),
    ('PGS', lambda F: _pg(F, 'set_PGS'), lambda d: d.pauli_gaussian('pgs', 40 / 27, 0.0, 0.0, 0.0)),
    ('PGSL025', lambda F: _pg(F, 'set_PGSL025'), lambda d: d.pauli_gaussian('pgsl025', 40 / 27, 0.25, 0.0, 0.0)),
    ('PGSLr', lambda F: _pg(F, 'set_PGSLr'), lambda d: d.pauli_gaussian('pgslr', 40 / 27, 0.25, 0.4, 0.2)),
    ('WTS-linear', lambda F: _wts(F, lambda t: 1 + t), lambda d: d.wt_style(5 / 6, 5 / 6, lambda x: 1 + x, lambda x: 1.0, 1.0)),
    ('WTS-exp', lambda F: _wts(F, _torch_exp(F)), lambda d: d.wt_style(5 / 6, 5 / 6, math.exp, math.exp, 1.0)),
    ('WTS-user', lambda F: _wts(F, user_f), lambda d: d.wt_style(5 / 6, 5 / 6, user_f, lambda x: 2 + 2 * x, 2.0)),
]
IDS = [c[0] for c in CALLABLES]
DOUBLES = {c[0]: c[2] for c in CALLABLES}
FACTORIES = {c[0]: c[1] for c in CALLABLES}


def evaluate(box, n, ids=IDS, vext=None):
    """{id: (E, dE/dn, sigma)} for the drop-in callables `ids`, plus 'sum'; with `vext` the IonElectron term at that fixed
    potential joins under 'IonElectron' (E = int n v_ext, dE/dn = v_ext; its sigma is the partial one at fixed grid values of
    v_ext, zero in the convention of Engine.stress: the dependence of v_ext on the cell is species_stress's)"""
    d = D(box, n)
    out = {i: DOUBLES[i](d) for i in ids}
    if vext is not None:
        out['IonElectron'] = d.ev.ion_electron(d.n, vext) + (np.zeros((3, 3)),)
    out['sum'] = add(*out.values())
    return out


# ----------------------------------------------------------------------------------------------------------- comparison helpers
def rel(a, b):
    """max |a - b| / max |b|"""
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b)) / np.max(np.abs(b)))


def check_field(v, vo, what='', E=None, Eo=None, vok=None):
    """a potential / gradient grid and its energy against the double at the fp64 bounds of the oracle matrices
    (spectral_check: V_TOL in real space, K_TOL per k-point, E_TOL); returns (err_v, err_k, err_E)"""
    ev, ek = sc.check(v, vo, 'f64', what, vok, E, Eo)
    return ev, ek, (abs(E - Eo) / max(1.0, abs(Eo)) if E is not None else None)


def check_stress(sig, sigo, rtol=SIG_RTOL, what=''):
    e = rel(sig, sigo)
    assert e <= rtol, ('stress', what, e, rtol)
    return e


def check_forces(F, Fo, rtol=ION_RTOL, what=''):
    """every species' forces against the double's, relative to the largest force of the whole list"""
    scale = max(float(np.abs(f).max()) for f in Fo)
    assert [np.shape(a) for a in F] == [np.shape(b) for b in Fo], ('forces', what, [np.shape(a) for a in F])
    e = max(float(np.abs(np.asarray(a) - b).max()) for a, b in zip(F, Fo)) / scale
    assert e <= rtol, ('forces', what, e, rtol)
    return e


def check_ion_potential(v, vo, rtol=ION_RTOL, what=''):
    e = rel(v, vo)
    assert e <= rtol, ('ionic potential', what, e, rtol)
    return e


# ------------------------------------------------------------------------------------------------- the ions of the species test
def tiled_ions(seed=320):
    """320 ions: a 4 x 4 x 5 tiling of a four-ion basis, jittered with a fixed seed, shifted so that some coordinates lie
    outside [0, 1) (below 0 and above 1), with one coincident pair (ion 201 sits on ion 7: one of each species)
    -> ([200, 3], [120, 3])"""
    basis = np.array([[0.0, 0.0, 0.0], [0.5, 0.5, 0.0], [0.5, 0.0, 0.5], [0.0, 0.5, 0.5]])
    reps = np.array([4.0, 4.0, 5.0])
    cells = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(5), indexing='ij'), -1).reshape(-1, 1, 3)
    frac = ((cells + basis[None]) / reps).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    frac = frac + 0.02 * (rng.random(frac.shape) - 0.5) + np.array([-0.1, 0.15, 0.0])
    frac = frac[rng.permutation(frac.shape[0])]
    frac[201] = frac[7]
    assert frac.shape == (320, 3) and frac.min() < 0.0 and frac.max() >= 1.0
    return frac[:200].copy(), frac[200:].copy()
