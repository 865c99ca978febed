"""Drop-in energy terms with the reference's names and call signatures, backed by the HIP engine.

Every callable here has the reference protocol ``f(box_vecs, den) -> torch scalar`` (``IonElectron``
takes ``v_ext`` as a third argument) of src/professad/functionals.py, keeps the reference's
``__name__``/``__qualname__`` (professad's System dispatches on them, system.py:199-203,761-771,
917-921) and supports ``E.backward()`` / ``torch.autograd.grad`` w.r.t. ``den``, with the analytic functional
derivative computed by the engine (no autograd through FFTs).  Under ``create_graph=True`` that derivative is itself
differentiable in ``den``: its backward is the engine's Hessian-vector product (``Engine.hessian_vector``), for the terms
that have one (Hartree, TF, vW, the Wang-Teter family, the local XC terms); the others raise ``NotImplementedError`` there.
PBE and WGC99 stay among the others here: their second derivatives are options of an ``Engine`` of one's own (``OPT_HVP_GGA``,
``OPT_HVP_WGC``), and the engines behind these terms are shared and keep the default.
``get_inv_G`` (functional_tools.py:34-70) rests on it.

So ``terms=[IonElectron, Hartree, WangTeter, PerdewBurkeErnzerhof]`` built from THIS module can be
handed to professad's ``System`` unchanged, and ``get_functional_derivative(box_vecs, den, f)``
(functional_tools.py:9-31) works on them.  ``NativeTerms`` fuses several terms into one engine call
(shared spectra; System only sums its terms, system.py:771).

Gradients w.r.t. ``box_vecs`` come from the engine's analytic per-term stress (ofdft_stress), so the reference's
``get_stress(box_vecs, den, f)`` (functional_tools.py:73-101) works on these terms too.
"""
import weakref

import numpy as np
import torch

from . import _native as N
from .engine import engine_for

_S5 = np.sqrt(5.0)


_BOX_CACHE = {}       # id(tensor) -> (weakref, version counter, data_ptr, host copy (3x3 float64), cell volume); a few Systems
_BOX_CACHE_MAX = 8


def _host_box(box_vecs):
    """Lattice vectors on the host + the cell volume.  professad's System hands its own ``box_vecs`` attribute to every term of
    every iteration (system.py:771): when the caller passes a tensor object it passed before, unmodified (same version
    counter, same storage), nothing crosses the device boundary -- a device->host copy of 72 bytes is a stream
    synchronisation, as long as a small-grid evaluation itself.  The cache holds weak references only (no device tensor is
    kept alive), tensors that require grad (stress paths) or have no version counter (inference mode) are never cached."""
    try:
        ver = box_vecs._version
    except Exception:  # noqa: BLE001  (inference-mode tensors have no version counter)
        ver = None
    key = id(box_vecs)
    if ver is not None:
        hit = _BOX_CACHE.get(key)
        if hit is not None and hit[0]() is box_vecs and hit[1] == ver and hit[2] == box_vecs.data_ptr():
            return hit[3], hit[4]
    box = np.ascontiguousarray(box_vecs.detach().double().cpu().numpy()).reshape(3, 3)
    vol = float(torch.abs(torch.linalg.det(torch.from_numpy(box))))
    if ver is not None and not box_vecs.requires_grad:
        if len(_BOX_CACHE) >= _BOX_CACHE_MAX:
            for k in [k for k, h in _BOX_CACHE.items() if h[0]() is None] or list(_BOX_CACHE)[:1]:
                del _BOX_CACHE[k]
        _BOX_CACHE[key] = (weakref.ref(box_vecs), ver, box_vecs.data_ptr(), box, vol)
    return box, vol


class _NativeEnergy(torch.autograd.Function):
    """forward: C-ABI call (energy + dE/dn); backward: gE * dE/dn * dV  (functional_tools.py:31).

    When ``box_vecs.requires_grad`` (the reference's get_stress / System.stress differentiate the energy with respect
    to the lattice vectors, functional_tools.py:94-99) the engine's analytic stress supplies the PARTIAL derivative at
    fixed density grid values: with sigma the stress at fixed electron number (density ~ 1/volume),
        dE/dB |_n = B^-T (vol * sigma + (int v n) * 1),
    because the density path -- which torch differentiates itself through ``den * vol.detach() / vol`` -- contributes
    -(int v n) B^-T.  For IonElectron (fixed v_ext array) sigma = 0 and the formula reduces to E B^-T; the dependence
    of v_ext on the cell is differentiated by whoever built v_ext."""

    @staticmethod
    def forward(ctx, box_vecs, den, v_ext, term_names, params):
        eng = engine_for(den.shape, den.device)
        box_np, vol = _host_box(box_vecs)
        eng.set_cell(box_np)
        eng.set_terms(term_names, params)          # (hashable tuples: memoised in the engine)
        need_box = box_vecs.requires_grad
        need_v = den.requires_grad or need_box
        E_terms, v = eng.energy_potential(den, v_ext, want_potential=need_v)
        dV = vol / den.numel()
        ctx.dV = dV
        ctx.has_vext = v_ext is not None
        ctx.g_box = None
        if need_box:
            sig = sum(eng.stress(den).values())                              # total over the active terms (3x3)
            vn = float((v * den.detach()).sum()) * dV
            g = torch.linalg.inv(torch.from_numpy(box_np)).T @ torch.as_tensor(vol * sig + vn * np.eye(3))
            ctx.g_box = g.to(box_vecs.device)
        # The third entry is the input itself: whether a backward will run under create_graph is not known here, and that one
        # differentiates with respect to it again.  A reference, no copy and no work -- but autograd's version check now covers
        # den: an in-place change of den between this call and its backward raises instead of being ignored.
        ctx.save_for_backward(v if den.requires_grad else None,
                              den.detach() if (v_ext is not None and v_ext.requires_grad) else None,
                              den if den.requires_grad else None)
        ctx.E_terms = E_terms
        ctx.hvp_key = (box_np, term_names, params, need_box)
        return torch.tensor(sum(E_terms.values()), dtype=torch.double, device=den.device)

    @staticmethod
    def backward(ctx, gE):
        v, den, den_in = ctx.saved_tensors
        if v is not None and torch.is_grad_enabled():       # create_graph=True: the potential stays differentiable in den
            box_np, term_names, params, need_box = ctx.hvp_key
            if need_box:
                raise NotImplementedError('mixed second derivatives with respect to box_vecs are not served: the native terms '
                                          'are twice differentiable in the density only')
            g_den = _NativePotential.apply(den_in, gE, v, ctx.dV, box_np, term_names, params)
            g_vext = gE * den * ctx.dV if den is not None else None
            return None, g_den, g_vext, None, None
        g_den = gE * v * ctx.dV if v is not None else None
        g_vext = gE * den * ctx.dV if den is not None else None       # d/dv_ext of mean(n v) vol
        g_box = gE.to(ctx.g_box.device) * ctx.g_box if ctx.g_box is not None else None
        return g_box, g_den, g_vext, None, None


class _NativePotential(torch.autograd.Function):
    """The first derivative as a differentiable node (only built by a backward under ``create_graph=True``): forward returns
    what ``_NativeEnergy.backward`` returns, gE * dE/dn * dV; its backward for an incoming ``u`` is the Hessian-vector product
    gE * dV * hessian_vector(den, u) (ofdft_hessian_vector) -- what the reference's double autograd gives get_inv_G
    (functional_tools.py:34-70) and the second-order derivative terms of System (system.py:1204-1367)."""

    @staticmethod
    def forward(ctx, den, gE, v, dV, box_np, term_names, params):
        ctx.save_for_backward(den, gE, v)
        ctx.key = (dV, box_np, term_names, params)
        return gE * v * dV

    @staticmethod
    def backward(ctx, u):
        den, gE, v = ctx.saved_tensors
        dV, box_np, term_names, params = ctx.key
        if torch.is_grad_enabled():
            raise NotImplementedError('native terms are twice differentiable in the density: no third derivative')
        eng = engine_for(den.shape, den.device)
        eng.set_cell(box_np)                       # the shared engine may have served another term since the forward pass
        eng.set_terms(term_names, params)
        try:
            hv = eng.hessian_vector(den, u.detach().contiguous())
        except RuntimeError as e:
            if 'no second derivative' in str(e):
                raise NotImplementedError(str(e)) from None
            raise
        return gE * dV * hv, (u * v).sum() * dV, None, None, None, None, None


def _evaluate(box_vecs, den, names, params=(), v_ext=None):
    return _NativeEnergy.apply(box_vecs, den, v_ext, tuple(names), tuple(params))


class NativeTerms:
    """Several reference terms fused into ONE engine evaluation.

    ``NativeTerms(['hartree', 'wgc99', 'pbe'])`` behaves like a single reference functional
    f(box_vecs, den); with ``'ion_electron'`` in the list it takes the reference's IonElectron
    signature f(box_vecs, den, v_ext) and carries ``__qualname__ == 'IonElectron'`` so that professad's
    System passes v_ext (system.py:762-763)."""

    ALIASES = {
        'wt': ('tf', 'vw', 'wt_nl'), 'wgc99': ('tf', 'vw', 'wgc99_nl'),
        'pz': ('lda_x', 'pz_c'), 'pw': ('lda_x', 'pw_c'), 'chachiyo': ('lda_x', 'chachiyo_c'),
        'pbe': ('pbe_x', 'pbe_c'), 'lkt': ('vw', 'gga_k'),
    }

    def __init__(self, names, **params):
        flat = []
        for nm in names:
            for t in self.ALIASES.get(nm, (nm,)):
                if t not in N.TERM_BITS:
                    raise KeyError('unknown term %r' % (t,))
                if t not in flat:
                    flat.append(t)
        self.names = tuple(flat)
        self.params = tuple(sorted(params.items()))
        self.needs_vext = 'ion_electron' in flat
        self.__name__ = self.__qualname__ = 'IonElectron' if self.needs_vext else 'NativeTerms'
        self.last_energies = None

    def __call__(self, box_vecs, den, v_ext=None):
        if self.needs_vext and v_ext is None:
            raise TypeError('this NativeTerms includes ion_electron and needs v_ext')
        return _evaluate(box_vecs, den, self.names, self.params, v_ext if self.needs_vext else None)

    def potential(self, box_vecs, den, v_ext=None):
        """dE/dn grid -- the reference's ``potentials=`` hook signature f(box_vecs, den) (system.py:849)."""
        eng = engine_for(den.shape, den.device)
        eng.set_cell(_host_box(box_vecs)[0])
        eng.set_terms(self.names, self.params)
        self.last_energies, v = eng.energy_potential(den, v_ext if self.needs_vext else None)
        return v


# ----------------------------------------------------------------- reference-named functionals
def IonIon():
    """Marker term, handled by System (functionals.py:21-28)."""
    return None


def IonElectron(box_vecs, den, v_ext):
    """functionals.py:31-46"""
    return _evaluate(box_vecs, den, ('ion_electron',), v_ext=v_ext)


def Hartree(box_vecs, den):
    """functionals.py:49-72"""
    return _evaluate(box_vecs, den, ('hartree',))


def ThomasFermi(box_vecs, den):
    """functionals.py:207-224"""
    return _evaluate(box_vecs, den, ('tf',))


def Weizsaecker(box_vecs, den):
    """functionals.py:227-246"""
    return _evaluate(box_vecs, den, ('vw',))


def non_local_KEF(box_vecs, den, alpha, beta):
    """functionals.py:644-652"""
    return _evaluate(box_vecs, den, ('wt_nl',), (('wt_alpha', float(alpha)), ('wt_beta', float(beta))))


def _wt_style(alpha, beta):
    p = (('wt_alpha', float(alpha)), ('wt_beta', float(beta)))

    def f(box_vecs, den):
        return _evaluate(box_vecs, den, ('tf', 'vw', 'wt_nl'), p)
    return f


WangTeter = _wt_style(5 / 6, 5 / 6)                        # functionals.py:655-670
Perrot = _wt_style(1.0, 1.0)                               # functionals.py:673-689
SmargiassiMadden = _wt_style(0.5, 0.5)                     # functionals.py:692-707
WangGovindCarter98 = _wt_style((5 + _S5) / 6, (5 - _S5) / 6)   # functionals.py:710-725
for _f, _n in ((WangTeter, 'WangTeter'), (Perrot, 'Perrot'), (SmargiassiMadden, 'SmargiassiMadden'),
               (WangGovindCarter98, 'WangGovindCarter98')):
    _f.__name__ = _f.__qualname__ = _n


class WangGovindCarter99:
    """functionals.py:787-985.  ``init_args=(alpha, beta, gamma, kappa)`` as in the reference (:795-815);
    call the instance or its ``forward``.  The kernel tables are generated on the GPU and cached in the
    engine while the cell and the rounded electron count are unchanged (reference rule :961-966)."""

    def __init__(self, init_args=None):
        if init_args is None:
            init_args = ((5 + _S5) / 6, (5 - _S5) / 6, 2.7, 1.0)
        self.alpha, self.beta, self.gamma, self.kappa = (float(x) for x in init_args)
        self.__name__ = self.__qualname__ = 'WangGovindCarter99'

    def _params(self):
        return (('wgc_alpha', self.alpha), ('wgc_beta', self.beta), ('wgc_gamma', self.gamma), ('wgc_kappa', self.kappa))

    def forward(self, box_vecs, den):
        return _evaluate(box_vecs, den, ('tf', 'vw', 'wgc99_nl'), self._params())

    __call__ = forward


def lda_exchange(box_vecs, den):
    """functionals.py:1510-1512"""
    return _evaluate(box_vecs, den, ('lda_x',))


def perdew_zunger_correlation(box_vecs, den):
    """functionals.py:1515-1521"""
    return _evaluate(box_vecs, den, ('pz_c',))


def perdew_wang_correlation(box_vecs, den):
    """functionals.py:1524-1530"""
    return _evaluate(box_vecs, den, ('pw_c',))


def chachiyo_correlation(box_vecs, den):
    """functionals.py:1533-1537"""
    return _evaluate(box_vecs, den, ('chachiyo_c',))


def PerdewZunger(box_vecs, den):
    """functionals.py:1540-1554"""
    return _evaluate(box_vecs, den, ('lda_x', 'pz_c'))


def PerdewWang(box_vecs, den):
    """functionals.py:1557-1571"""
    return _evaluate(box_vecs, den, ('lda_x', 'pw_c'))


def Chachiyo(box_vecs, den):
    """functionals.py:1574-1588"""
    return _evaluate(box_vecs, den, ('lda_x', 'chachiyo_c'))


def pbe_exchange(box_vecs, den):
    """functionals.py:1597-1603"""
    return _evaluate(box_vecs, den, ('pbe_x',))


def pbe_correlation(box_vecs, den):
    """functionals.py:1606-1618"""
    return _evaluate(box_vecs, den, ('pbe_c',))


def PerdewBurkeErnzerhof(box_vecs, den):
    """functionals.py:1621-1635"""
    return _evaluate(box_vecs, den, ('pbe_x', 'pbe_c'))


def get_functional_derivative(box_vecs, den, functional, requires_grad=False):
    """functional_tools.py:9-31 for native terms (same result as autograd on them, one engine call).  With
    ``requires_grad=True`` the derivative returned can be differentiated once more with respect to ``den`` (which then is
    the tensor passed in, as in the reference): its backward is a Hessian-vector product of the engine.  Unlike the
    reference (functional_tools.py:28-30), which sets ``den.requires_grad`` back to False, ``den`` then keeps
    ``requires_grad=True``: it is the leaf the caller differentiates the result with respect to."""
    if requires_grad:
        den.requires_grad_()
    else:
        den = den.detach().requires_grad_()
    E = functional(box_vecs, den)
    (g,) = torch.autograd.grad(E, den, create_graph=requires_grad)
    return g / (torch.abs(torch.linalg.det(box_vecs)) / den.numel())


def get_inv_G(box_vecs, den, kinetic_functional, requires_grad=False):
    """functional_tools.py:34-70: the linear-response function G^-1(eta) = pi^2 / (k_F F[d^2 T / dn dn']) of a kinetic
    functional at the uniform density n0 = round(mean(den) vol) / vol -> (eta, G_inv) on the half spectrum.  One
    Hessian-vector product of every native term inside ``kinetic_functional`` (composites -- sums, a user's stabilisation
    function -- go through autograd as in the reference); the transform of the response row is the engine's."""
    if requires_grad or box_vecs.requires_grad:
        raise NotImplementedError('get_inv_G: derivatives of the response function (third derivatives of the functional, or '
                                  'mixed density-cell ones) are not served')
    vol = float(torch.abs(torch.linalg.det(box_vecs.detach().double())))
    n_elec = round(float(torch.mean(den)) * vol)
    n0 = torch.full(den.shape, n_elec / vol, dtype=torch.double, device=den.device).requires_grad_()
    k_F = (3 * np.pi * np.pi * n_elec / vol) ** (1 / 3)
    dV = vol / den.numel()
    dTdn = torch.autograd.grad(kinetic_functional(box_vecs, n0), n0, create_graph=True)[0] / dV
    row = torch.autograd.grad(dTdn[0, 0, 0], n0)[0]
    G_inv = np.pi * np.pi / k_F / engine_for(den.shape, den.device).rfftn(row.contiguous()).real
    # |k| as functional_tools.py:135-162 (wavevecs) gives it
    b = 2 * np.pi * torch.linalg.inv(box_vecs.detach().double().T).to(den.device)
    f = [torch.fft.fftfreq(s, dtype=torch.double, device=den.device) * s for s in den.shape[:2]]
    for a in (0, 1):                       # the Nyquist frequency of an even extent counts as positive (:152-154)
        if den.shape[a] % 2 == 0:
            f[a][den.shape[a] // 2] = den.shape[a] // 2
    f.append(torch.fft.rfftfreq(den.shape[2], dtype=torch.double, device=den.device) * den.shape[2])
    fa, fb, fc = torch.meshgrid(*f, indexing='ij')
    k = [fa * b[0, j] + fb * b[1, j] + fc * b[2, j] for j in range(3)]
    eta = torch.sqrt(k[0] ** 2 + k[1] ** 2 + k[2] ** 2) / (2 * k_F)
    return eta, G_inv


def vWGTF1(box_vecs, den):
    """functionals.py:251-274"""
    return _evaluate(box_vecs, den, ('vw', 'vwgtf'), (('vwgtf_kind', 1.0),))


def vWGTF2(box_vecs, den):
    """functionals.py:277-306"""
    return _evaluate(box_vecs, den, ('vw', 'vwgtf'), (('vwgtf_kind', 2.0),))


def LuoKarasievTrickey(box_vecs, den):
    """functionals.py:309-333 (vW + int tau_TF / cosh(1.3 s))"""
    return _evaluate(box_vecs, den, ('vw', 'gga_k'), (('ggak_kind', 0.0),))


class PauliGaussian:
    """functionals.py:336-403: vW + int tau_TF (exp(-mu s^2) + beta q^2 - lambda q s^2 + sigma s^4); default = PGSL0.25.
    Every member shares the gradient / flux / divergence passes of the fused pipelines with PBE (``OFDFT_GGA_K``); the
    Laplacian-dependent ones (PGSL0.25 -- the default --, PGSLr) carry two more spectra through the same chain (lap n in,
    lap(df/dL) out).  Fused, slab-decomposed and stress paths all serve them (tests: term + ``get_stress`` goldens)."""

    def __init__(self, init_args=None):
        self.mu, self.beta, self.lamb, self.sigma = (40 / 27, 0.25, 0.0, 0.0) if init_args is None else init_args
        self.__name__ = self.__qualname__ = 'PauliGaussian'

    def set_PG1(self):
        self.mu, self.beta, self.lamb, self.sigma = 1.0, 0.0, 0.0, 0.0

    def set_PGS(self):
        self.mu, self.beta, self.lamb, self.sigma = 40 / 27, 0.0, 0.0, 0.0

    def set_PGSL025(self):
        self.mu, self.beta, self.lamb, self.sigma = 40 / 27, 0.25, 0.0, 0.0

    def set_PGSLr(self):
        self.mu, self.beta, self.lamb, self.sigma = 40 / 27, 0.25, 0.4, 0.2

    def forward(self, box_vecs, den):
        p = (('ggak_kind', 1.0), ('ggak_mu', abs(float(self.mu))), ('ggak_beta', abs(float(self.beta))),
             ('ggak_lambda', abs(float(self.lamb))), ('ggak_sigma', abs(float(self.sigma))))
        return _evaluate(box_vecs, den, ('vw', 'gga_k'), p)

    __call__ = forward


def _stabiliser(f):
    """(f'(0), OFDFT_P_WTS_KIND or None) of a Pauli-positivity stabilisation function f (f(0) = 1): kind 0.0 for f(x) = 1 + x,
    1.0 for exp -- the two the engine evaluates itself -- else None (the caller composes the native energies in torch)."""
    zero = torch.zeros((1,), dtype=torch.double, requires_grad=True)
    if float(f(zero).detach()) != 1.0:
        raise ValueError('Requires f(0) = 1')
    fprime0 = float(torch.autograd.grad(f(zero), zero)[0])
    probe = torch.tensor([-0.7, 0.25, 1.0], dtype=torch.double)
    got = f(probe)
    kind = None
    if torch.allclose(got, 1 + probe, rtol=1e-14, atol=0):
        kind = 0.0
    elif torch.allclose(got, torch.exp(probe), rtol=1e-14, atol=0):
        kind = 1.0
    return fprime0, kind


class WangTeterStyleFunctional:
    """functionals.py:728-782: T = vW + T_TF f(T_NL / (f'(0) T_TF)) with a Pauli-positivity stabilisation function f
    (f(0) = 1; default f(x) = 1 + x, i.e. a plain Wang-Teter style functional).

    The two stabilisation functions the reference's papers and tests use are served by ONE engine evaluation
    (``OFDFT_P_WTS_KIND``): f(x) = 1 + x is the plain sum T_TF + T_NL, f = exp runs the combine stage twice (energies, then
    the potential with the weights f - f' X and f'(X) / f'(0) they determine); the stress carries the same weights
    (tests/tools_for_tests.py:310-364).  Any other callable f -- a user lambda cannot cross the C ABI -- composes the three
    native energies in torch, its derivative reaching the native potentials and stresses through autograd."""

    def __init__(self, init_args=None):
        self.alpha, self.beta, self.f = (5 / 6, 5 / 6, (lambda t: 1 + t)) if init_args is None else init_args
        self.fprime0, self._kind = _stabiliser(self.f)
        self.__name__ = self.__qualname__ = 'WangTeterStyleFunctional'

    def forward(self, box_vecs, den):
        if self._kind is not None:
            return _evaluate(box_vecs, den, ('tf', 'vw', 'wt_nl'),
                             (('wt_alpha', float(self.alpha)), ('wt_beta', float(self.beta)), ('wts_kind', self._kind)))
        vW, TF = Weizsaecker(box_vecs, den), ThomasFermi(box_vecs, den)
        T_NL = non_local_KEF(box_vecs, den, float(self.alpha), float(self.beta)) / self.fprime0
        return vW + TF * self.f(T_NL / TF)

    __call__ = forward


# ------------------------------------------- nonlocal functionals with a tabulated, density-independent kernel (OFDFT_NLK)
def _nlk_params(kind, p0=0.0, p1=0.0):
    return (('nlk_kind', float(kind)), ('nlk_p0', float(p0)), ('nlk_p1', float(p1)))


def _linear(x):
    return 1 + x


_STABILISERS = {_linear: (1.0, 0.0), torch.exp: (1.0, 1.0)}      # f -> _stabiliser(f)


def KGAP(box_vecs, den, E_gap, f=_linear):
    """functionals.py:1106-1171: vW + T_TF f(T_NL / (f'(0) T_TF)) with the gapped-jellium kernel for a band gap ``E_gap`` [eV].
    The kernel is tabulated on the device once per (cell, round(N_e), E_gap); f(x) = 1 + x (the default) and exp are ONE engine
    evaluation, any other f composes the native vW, TF and nonlocal energies in torch (as WangTeterStyleFunctional does).
    ``get_stress`` works on it (analytic stress of the tabulated kernel, f = exp included)."""
    hit = _STABILISERS.get(f)               # (detected once per function object: KGAP sits inside optimisation loops)
    if hit is None:
        if len(_STABILISERS) >= 16:
            _STABILISERS.clear()
        hit = _STABILISERS[f] = _stabiliser(f)
    fprime0, kind = hit
    p = _nlk_params(N.NLK_KGAP, E_gap)
    if kind is not None:
        return _evaluate(box_vecs, den, ('tf', 'vw', 'nlk'), p + (('wts_kind', kind),))
    vW, TF = Weizsaecker(box_vecs, den), ThomasFermi(box_vecs, den)
    T_NL = _evaluate(box_vecs, den, ('nlk',), p)
    return vW + TF * f(T_NL / fprime0 / TF)


class MiGenovaPavanello:
    """functionals.py:1370-1451.  ``init_args=(a, b)``; call the instance or its ``forward``.  The 1-D line-integral table
    (2000 nodes x 10000 quadrature points) and the per-k-point kernel are built on the device and rebuilt when the cell,
    round(N_e) or (a, b) change -- which is what a FRESH instance of the reference computes (a reference instance keeps the
    table of an earlier call while it still covers eta_max)."""

    def __init__(self, init_args):
        self.a, self.b = (float(x) for x in init_args)
        self.__name__ = self.__qualname__ = 'MiGenovaPavanello'

    def forward(self, box_vecs, den):
        if box_vecs.requires_grad:
            raise NotImplementedError("MiGenovaPavanello has no stress: the reference's own get_stress raises on it "
                                      "(torch.unique, which builds its kernel, has no derivative)")
        return _evaluate(box_vecs, den, ('tf', 'vw', 'nlk'), _nlk_params(N.NLK_MGP, self.a, self.b))

    __call__ = forward


def XuWangMa(box_vecs, den, kappa=0):
    """functionals.py:1456-1498: vW + TF + the Taylor-expanded line-integral kernel (two powers of the density, a 2 x 2 kernel
    matrix mixed inside one x pass); ``get_stress`` works on it."""
    return _evaluate(box_vecs, den, ('tf', 'vw', 'nlk'), _nlk_params(N.NLK_XWM, kappa))


# ------------------------------------------- nonlocal functionals with a density-dependent kernel (OFDFT_NLK kinds 4 and 5)
class _HuangCarterBase:
    """What HuangCarter and RevisedHuangCarter share: the kernel table w(eta) (``.kernel``, [2, N_eta]: eta; w) and the call.
    The table is the project's own classical Runge-Kutta solution of the reference's initial-value problem
    (professad_amd.hc_kernel), not xitorch's ``solve_ivp`` -- the two differ by the truncation error of the integrators."""

    def generate_kernel(self, eta_max=50, N_eta=10000):
        from . import hc_kernel
        self._table = (float(eta_max), int(N_eta))
        eta, w = hc_kernel.solve_kernel(self.beta, *self._table)
        self.kernel = torch.from_numpy(np.stack([eta, w]))

    def _params(self):
        raise NotImplementedError

    def forward(self, box_vecs, den):
        if box_vecs.requires_grad:
            raise NotImplementedError('%s has no stress: the strain derivative of its density-dependent kernel is not built '
                                      '(differentiate in the density only)' % self.__name__)
        p = self._params() + (('nlk_eta_max', self._table[0]), ('nlk_n_eta', float(self._table[1])))
        return _evaluate(box_vecs, den, ('tf', 'vw', 'nlk'), p)

    __call__ = forward


class HuangCarter(_HuangCarterBase):
    """functionals.py:1176-1269: vW + TF + the Huang-Carter term with the single-point density-dependent kernel
    w(|r - r'|, xi(r)), xi = 2 k_F (1 + lambda |grad n|^2 / n^(8/3)).  ``init_args=(lamb, beta, kappa)``; kappa > 1 is the ratio
    of the geometric spline nodes in xi.  Differentiable once in ``den``; single GPU, fp64."""

    def __init__(self, init_args):
        self.lamb, self.beta, self.kappa = (float(x) for x in init_args)
        self.__name__ = self.__qualname__ = 'HuangCarter'
        self.generate_kernel()

    def _params(self):
        return (('nlk_kind', float(N.NLK_HC)), ('nlk_p0', self.lamb), ('nlk_p1', self.beta), ('nlk_p2', self.kappa))


class RevisedHuangCarter(_HuangCarterBase):
    """functionals.py:1272-1365: as HuangCarter with xi = 2 k_F (1 + a s^2 / (1 + b s^2)), s the reduced gradient.
    ``init_args=(a, b, beta, kappa)``."""

    def __init__(self, init_args):
        self.a, self.b, self.beta, self.kappa = (float(x) for x in init_args)
        self.__name__ = self.__qualname__ = 'RevisedHuangCarter'
        self.generate_kernel()

    def _params(self):
        return (('nlk_kind', float(N.NLK_REVHC)), ('nlk_p0', self.a), ('nlk_p1', self.b), ('nlk_p2', self.beta), ('nlk_p3', self.kappa))
