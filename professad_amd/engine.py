"""Python host object over one ofdft_ctx (one grid shape on one GPU).

PyTorch is used only as plumbing: it owns the device tensors and the HIP stream; every number is
produced by the HIP library behind the C ABI.  There is no CPU path: construction raises when the
library or a GPU is missing.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _native as N
from . import hc_kernel


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class Engine:
    """energy + functional derivative of a set of OFDFT terms on a fixed grid shape."""

    def __init__(self, shape, device=None, nranks=1, rank=0, dtype=torch.double):
        """dtype: torch.double (the reference's precision; libofdft_hip.so) or torch.float32 (the fp32 build of the
        same kernels, libofdft_hip_f32.so: hot path and L-BFGS only; energy sums stay fp64)."""
        if dtype not in (torch.double, torch.float32):
            raise TypeError('dtype must be torch.double or torch.float32')
        self.dtype = dtype
        self.cdtype = torch.complex128 if dtype == torch.double else torch.complex64
        self._code = N.F64 if dtype == torch.double else N.F32
        if not torch.cuda.is_available():
            raise N.NativeLibraryError('professad_amd needs a ROCm GPU (torch.cuda.is_available() is False); '
                                       'there is no CPU fallback')
        self.lib = N.load(self._code)
        self.device = torch.device(device if device is not None else 'cuda:0')
        if self.device.type != 'cuda':
            raise ValueError('Engine tensors must live on a GPU device, got %s' % self.device)
        self.global_shape = tuple(int(s) for s in shape)
        if len(self.global_shape) != 3:
            raise ValueError('shape must be (n0, n1, n2)')
        # `shape` of the tensors this engine takes: the rank's x-slab (the whole grid on one GPU)
        self.shape = (self.global_shape[0] // int(nranks),) + self.global_shape[1:]
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self._ctx = C.c_void_p(0)
        rc = self.lib.ofdft_create_dist(C.byref(self._ctx), *self.global_shape, self._code, idx, int(nranks), int(rank))
        if rc != 0:
            raise RuntimeError('ofdft_create failed (%d): %s' % (rc, self.lib.ofdft_last_error(None).decode()))
        self._box_key = None
        self._terms_key = None
        self._terms_memo = {}
        self._nlk_table_key = None
        self._options = {}           # option number -> the value last given to set_option (Engine.option)
        self.npts = int(np.prod(self.shape))
        self._dev_index = idx
        self._dev_exact = torch.device('cuda', idx)
        # (a private torch entry point, ~1.5 microseconds cheaper per call than torch.cuda.current_stream(); optional)
        self._raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)

    def close(self):
        if getattr(self, '_ctx', None) is not None and self._ctx.value:
            self.lib.ofdft_destroy(self._ctx)
            self._ctx = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    # -- helpers
    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError('%s failed (%d): %s' % (what, rc, self.lib.ofdft_last_error(self._ctx).decode()))

    def _grid_tensor(self, t, name):
        if t is None:
            return None
        if not isinstance(t, torch.Tensor):
            raise TypeError('%s must be a torch.Tensor' % name)
        if t.device == self._dev_exact and t.dtype == self.dtype and t.shape == self.shape and not t.requires_grad and t.is_contiguous():
            return t                                      # the hot path's case: nothing to convert
        if t.device != self.device and not (t.device.type == 'cuda' and self.device.type == 'cuda'
                                            and (t.device.index or 0) == (self.device.index or 0)):
            raise ValueError('%s is on %s, engine is on %s' % (name, t.device, self.device))
        if t.dtype != self.dtype:
            raise TypeError('%s must be %s for this engine (the reference is fp64 throughout; an fp32 engine takes '
                            'torch.float32 only)' % (name, self.dtype))
        if tuple(t.shape) != self.shape:
            raise ValueError('%s has shape %s, engine grid is %s' % (name, tuple(t.shape), self.shape))
        if t.requires_grad or not t.is_contiguous():
            t = t.detach().contiguous()
        return t

    def _stream(self):
        if self._raw_stream is not None:
            return C.c_void_p(self._raw_stream(self._dev_index))
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # -- configuration
    def set_cell(self, box_vecs):
        # a host array is compared by its 72 bytes (no device sync; a caller may rescale its box array IN PLACE between
        # calls, so object identity says nothing); anything else goes through torch first
        if isinstance(box_vecs, np.ndarray):
            box = np.ascontiguousarray(box_vecs, dtype=np.float64).reshape(9)
        else:
            box = np.ascontiguousarray(torch.as_tensor(box_vecs).detach().cpu().numpy(), dtype=np.float64).reshape(9)
        key = box.tobytes()
        if key != self._box_key:
            self._check(self.lib.ofdft_set_cell(self._ctx, box.ctypes.data_as(C.POINTER(C.c_double))), 'ofdft_set_cell')
            self._box_key = key
        return self

    def set_terms(self, names, params=None):
        """names: iterable of keys of _native.TERM_BITS; params: dict slot->value
        (wt_alpha, wt_beta, wgc_alpha, wgc_beta, wgc_gamma, wgc_kappa, ggak_kind, ggak_mu, ggak_beta, ggak_lambda, ggak_sigma, vwgtf_kind,
        wts_kind, nlk_kind, nlk_p0, nlk_p1, nlk_p2, nlk_p3).  For nlk_kind 4 / 5 (HuangCarter: nlk_p0..2 = lambda, beta, kappa;
        RevisedHuangCarter: nlk_p0..3 = a, b, beta, kappa) the kernel table of hc_kernel.solve_kernel(beta, nlk_eta_max, nlk_n_eta)
        goes to the library with the call; the two table arguments are keys of ``params`` too (defaults 50, 10000)."""
        memo = None
        if isinstance(names, tuple) and (params is None or isinstance(params, tuple)):      # hashable call (the drop-in terms): memoised
            memo = (names, params)
            key = self._terms_memo.get(memo)
            if key is not None:
                if key != self._terms_key:
                    vals = np.frombuffer(key[1], dtype=np.float64)
                    self._check(self.lib.ofdft_set_terms(self._ctx, key[0], vals.ctypes.data_as(C.POINTER(C.c_double)), len(vals)),
                                'ofdft_set_terms')
                    self._terms_key = key
                self._hc_table(key[1], self._terms_memo[(memo, 'table')])
                return self
            params = dict(params) if params else None
        mask = 0
        for nm in names:
            mask |= N.TERM_BITS[nm]
        slots = ['wt_alpha', 'wt_beta', 'wgc_alpha', 'wgc_beta', 'wgc_gamma', 'wgc_kappa', 'ggak_kind', 'ggak_mu', 'ggak_beta',
                 'ggak_lambda', 'ggak_sigma', 'vwgtf_kind', 'wts_kind', 'nlk_kind', 'nlk_p0', 'nlk_p1', 'nlk_p2', 'nlk_p3']
        s5 = np.sqrt(5.0)
        vals = np.array([5 / 6, 5 / 6, (5 + s5) / 6, (5 - s5) / 6, 2.7, 1.0, 0.0, 40 / 27, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                        dtype=np.float64)
        params = dict(params or {})
        table = (float(params.pop('nlk_eta_max', 50.0)), int(params.pop('nlk_n_eta', 10000)))
        for k, v in params.items():
            vals[slots.index(k)] = float(v)
        key = (mask, vals.tobytes())
        if key != self._terms_key:
            self._check(self.lib.ofdft_set_terms(self._ctx, mask, vals.ctypes.data_as(C.POINTER(C.c_double)), len(vals)),
                        'ofdft_set_terms')
            self._terms_key = key
        if memo is not None:
            self._terms_memo[memo] = key
            self._terms_memo[(memo, 'table')] = table
        self._hc_table(key[1], table)
        return self

    def _hc_table(self, vals_bytes, table):
        """the Huang-Carter kernel table of the term set just selected goes to the library, once per (beta, eta_max, n_eta)"""
        vals = np.frombuffer(vals_bytes, dtype=np.float64)
        kind = int(vals[N.P_NLK_KIND])
        if kind not in (N.NLK_HC, N.NLK_REVHC) or not (self._terms_key[0] & N.TERM_BITS['nlk']):
            return
        beta = float(vals[N.P_NLK_P1 if kind == N.NLK_HC else N.P_NLK_P2])
        if self._nlk_table_key == ('custom', beta):       # the caller's own table for this beta (set_nlk_table) stays
            return
        tkey = (beta,) + tuple(table)
        if tkey != self._nlk_table_key:
            eta, w = hc_kernel.solve_kernel(*tkey)
            self.set_nlk_table(eta, w)
            self._nlk_table_key = tkey

    def set_nlk_table(self, eta, w):
        """The 1-D kernel table w(eta) of the Huang-Carter kinds (ofdft_set_nlk_table): uniform eta grid from 0, >= 4 nodes.
        ``set_terms`` calls it by itself with the table of hc_kernel.solve_kernel.  A caller with a table of its own calls it after
        the ``set_terms`` that selects kind 4 / 5: the table then belongs to that term set's beta and stays through later
        ``set_terms`` calls (those of the drop-in classes included) until one selects another beta, which brings solve_kernel's
        table for the new beta back.  Called before such a ``set_terms``, it is replaced by that call."""
        eta = np.ascontiguousarray(eta, dtype=np.float64)
        w = np.ascontiguousarray(w, dtype=np.float64)
        if eta.ndim != 1 or eta.shape != w.shape:
            raise ValueError('eta and w must be one-dimensional arrays of one length')
        dp = C.POINTER(C.c_double)
        self._check(self.lib.ofdft_set_nlk_table(self._ctx, eta.ctypes.data_as(dp), w.ctypes.data_as(dp), len(eta)), 'ofdft_set_nlk_table')
        self._nlk_table_key = None
        if self._terms_key is not None and (self._terms_key[0] & N.TERM_BITS['nlk']):
            vals = np.frombuffer(self._terms_key[1], dtype=np.float64)
            kind = int(vals[N.P_NLK_KIND])
            if kind in (N.NLK_HC, N.NLK_REVHC):
                self._nlk_table_key = ('custom', float(vals[N.P_NLK_P1 if kind == N.NLK_HC else N.P_NLK_P2]))
        return self

    def _mask(self):
        """term mask of the last set_terms (0 before the first)"""
        return self._terms_key[0] if self._terms_key is not None else 0

    # -- hot path
    def energy_potential(self, den, vext=None, want_potential=True):
        """-> (dict term -> E [Ha], dE/dn tensor or None)."""
        den = self._grid_tensor(den, 'den')
        vext = self._grid_tensor(vext, 'v_ext')
        out = torch.empty_like(den) if want_potential else None
        E = (C.c_double * N.NTERMS)()
        self._check(self.lib.ofdft_energy_potential(self._ctx, _ptr(den), _ptr(vext), E, _ptr(out), self._stream()),
                    'ofdft_energy_potential')
        return N.per_term(E, self._mask()), out

    def energy_grad_chi(self, chi, n_elec, vext=None, want_grad=True):
        """The optimize_density closure: -> (dict term -> E, mu, chi.grad tensor or None)."""
        chi = self._grid_tensor(chi, 'chi')
        vext = self._grid_tensor(vext, 'v_ext')
        out = torch.empty_like(chi) if want_grad else None
        E = (C.c_double * N.NTERMS)()
        mu = C.c_double(0.0)
        self._check(self.lib.ofdft_energy_grad_chi(self._ctx, _ptr(chi), _ptr(vext), float(n_elec), E, C.byref(mu),
                                                   _ptr(out), self._stream()), 'ofdft_energy_grad_chi')
        return N.per_term(E, self._mask()), mu.value, out

    def hessian_vector(self, den, w, reuse_density=False, want_terms=False):
        """Second functional derivative of the active terms applied to the direction ``w``: hv = d/d eps v[den + eps w] at
        eps = 0 = (H w) / dV (ofdft_hessian_vector; what the reference gets from a second autograd pass, functional_tools.py:34-70).
        -> hv, or with ``want_terms`` (dict term -> int w (H_t w), hv).  ``reuse_density=True``: ``den`` holds the values of the
        previous call made without it; the density-only transforms are skipped and the result is bitwise the same."""
        if self.dtype != torch.double:
            raise NotImplementedError('Engine.hessian_vector: the Hessian-vector product is fp64 work (libofdft_hip.so); '
                                      'an fp32 engine does not serve it')
        den = self._grid_tensor(den, 'den')
        w = self._grid_tensor(w, 'w')
        out = torch.empty_like(den)
        q = (C.c_double * N.NTERMS)() if want_terms else None
        self._check(self.lib.ofdft_hessian_vector(self._ctx, _ptr(den), _ptr(w), _ptr(out), q, 1 if reuse_density else 0,
                                                  self._stream()), 'ofdft_hessian_vector')
        return (N.per_term(q, self._mask()), out) if want_terms else out

    def hessian_vector_chi(self, chi, d, g, n_elec, reuse_density=False, want_scalars=False, out=None):
        """The Hessian of the closure's E[chi] applied to the direction ``d``: the derivative of the gradient ``g`` that
        ``energy_grad_chi`` returns, along ``d`` (ofdft_hessian_vector_chi).  ``chi`` at any scale; ``g`` is that
        gradient or None at a stationary point (g = 0).  Where chi is exactly zero the term d g / chi counts as zero.
        -> H d, or with ``want_scalars`` (dict with dHd = d.Hd, phiHd = chi.Hd, a = chi.d, S = chi.chi, dmu; H d).
        ``reuse_density=True``: ``chi`` holds the values of the previous call made without it; the density-only transforms are
        skipped and the result is bitwise the same.  Single GPU and fp64, the terms of ``hessian_vector``."""
        if self.dtype != torch.double:
            raise NotImplementedError('Engine.hessian_vector_chi: the Hessian-vector product is fp64 work (libofdft_hip.so); '
                                      'an fp32 engine does not serve it')
        chi = self._grid_tensor(chi, 'chi')
        d = self._grid_tensor(d, 'd')
        g = self._grid_tensor(g, 'g')
        if out is None:
            out = torch.empty_like(chi)
        elif self._grid_tensor(out, 'out') is not out:
            raise ValueError('out must be a contiguous grid tensor of this engine')
        s = (C.c_double * N.HVC_NSCALARS)() if want_scalars else None
        self._check(self.lib.ofdft_hessian_vector_chi(self._ctx, _ptr(chi), _ptr(d), _ptr(g), float(n_elec), _ptr(out), s,
                                                      1 if reuse_density else 0, self._stream()), 'ofdft_hessian_vector_chi')
        return (dict(zip(N.HVC_NAMES, s)), out) if want_scalars else out

    def precondition(self, r, kappa2, out=None):
        """The kinetic preconditioner of the conjugate gradients (ofdft_precondition):
        z = irfftn(rfftn(r) / (k^2 + kappa2)) with kappa2 > 0 [1/bohr^2] -> z (``out`` if given; never ``r`` itself).
        Needs the cell only, not the terms; leaves what ``hessian_vector[_chi]`` retains for ``reuse_density=True`` valid.
        Single GPU and fp64."""
        if self.dtype != torch.double:
            raise NotImplementedError('Engine.precondition: the kinetic preconditioner is fp64 work (libofdft_hip.so); '
                                      'an fp32 engine does not serve it')
        if self.shape != self.global_shape:
            raise NotImplementedError('Engine.precondition: the kinetic preconditioner is served by single-GPU contexts')
        kappa2 = float(kappa2)
        if not (kappa2 > 0.0 and math.isfinite(kappa2)):
            raise ValueError('Engine.precondition: kappa2 must be positive and finite, got %r' % kappa2)
        r = self._grid_tensor(r, 'r')
        if out is None:
            out = torch.empty_like(r)
        elif self._grid_tensor(out, 'out') is not out:
            raise ValueError('out must be a contiguous grid tensor of this engine')
        if out.data_ptr() == r.data_ptr():
            raise ValueError('Engine.precondition: z is r -- the transform is not in place, give another `out`')
        self._check(self.lib.ofdft_precondition(self._ctx, _ptr(r), _ptr(out), kappa2, self._stream()), 'ofdft_precondition')
        return out

    # -- several columns per call (ofdft_*_multi)
    def _multi_refusal(self, who, what):
        """NotImplementedError, before any device work, where the multi entries are not served"""
        if self.dtype != torch.double:
            raise NotImplementedError('Engine.%s: %s is fp64 work (libofdft_hip.so); an fp32 engine does not serve it' % (who, what))
        if self.shape != self.global_shape:
            raise NotImplementedError('Engine.%s: %s is served by single-GPU contexts' % (who, what))

    def _grid_stack(self, t, name):
        """a stack [B, *shape] of 1 .. MULTI_MAX grid fields as the multi entries take it: contiguous fp64 on this device -> B"""
        if not isinstance(t, torch.Tensor):
            raise TypeError('%s must be a torch.Tensor' % name)
        if t.dim() != 4 or tuple(t.shape[1:]) != self.shape:
            raise ValueError('%s has shape %s; a stack [B, %d, %d, %d] of grid fields is needed' % ((name, tuple(t.shape)) + self.shape))
        if not 1 <= t.shape[0] <= N.MULTI_MAX:
            raise ValueError('%s stacks %d columns; the multi entries take 1 .. %d (OFDFT_MULTI_MAX)' % (name, t.shape[0], N.MULTI_MAX))
        if t.device != self._dev_exact or t.dtype != self.dtype or not t.is_contiguous() or t.requires_grad:
            raise ValueError('%s must be a contiguous %s stack on %s without requires_grad' % (name, self.dtype, self._dev_exact))
        return int(t.shape[0])

    def _stack_out(self, out, src, who):
        if out is None:
            return torch.empty_like(src)
        if self._grid_stack(out, 'out') != src.shape[0]:
            raise ValueError('Engine.%s: out stacks %d columns, the input %d' % (who, out.shape[0], src.shape[0]))
        nbytes = src.numel() * src.element_size()
        if out.data_ptr() < src.data_ptr() + nbytes and src.data_ptr() < out.data_ptr() + nbytes:
            raise ValueError('Engine.%s: out aliases the input stack -- the call is not in place, give another `out`' % who)
        return out

    def hessian_vector_chi_multi(self, chi, dirs, n_elec, reuse_density=False, want_scalars=False, out=None):
        """``hessian_vector_chi`` at a stationary point (g = 0) for a stack ``dirs`` [B, *shape] of B = 1 .. 8 directions in one call
        (ofdft_hessian_vector_chi_multi): chi, the density-side fields and the density-only factors are read or
        formed once for all columns.  -> H dirs [B, *shape], or with ``want_scalars`` (list of B dicts as ``hessian_vector_chi``
        returns them; H dirs).  Each column agrees with the single-column entry to rounding.  ``reuse_density=True`` may follow a
        call of either entry made without it on the same chi.  Single GPU and fp64, the terms of ``hessian_vector``."""
        self._multi_refusal('hessian_vector_chi_multi', 'the Hessian-vector product')
        from . import optimize
        why = optimize.second_order_refusal(self, gga_missing='batch')
        if why:
            raise NotImplementedError('Engine.hessian_vector_chi_multi: ' + why)
        B = self._grid_stack(dirs, 'dirs')
        chi = self._grid_tensor(chi, 'chi')
        out = self._stack_out(out, dirs, 'hessian_vector_chi_multi')
        s = (C.c_double * (N.HVC_NSCALARS * B))() if want_scalars else None
        self._check(self.lib.ofdft_hessian_vector_chi_multi(self._ctx, _ptr(chi), _ptr(dirs), self.npts, B, float(n_elec), _ptr(out), self.npts,
                                                            s, 1 if reuse_density else 0, self._stream()), 'ofdft_hessian_vector_chi_multi')
        if not want_scalars:
            return out
        return [dict(zip(N.HVC_NAMES, s[N.HVC_NSCALARS * j:N.HVC_NSCALARS * (j + 1)])) for j in range(B)], out

    def precondition_multi(self, r, kappa2, out=None):
        """``precondition`` for a stack ``r`` [B, *shape] of B = 1 .. 8 fields in one call with one synchronisation
        (ofdft_precondition_multi) -> z [B, *shape] (``out`` if given; it must not overlap ``r``)."""
        self._multi_refusal('precondition_multi', 'the kinetic preconditioner')
        kappa2 = float(kappa2)
        if not (kappa2 > 0.0 and math.isfinite(kappa2)):
            raise ValueError('Engine.precondition_multi: kappa2 must be positive and finite, got %r' % kappa2)
        B = self._grid_stack(r, 'r')
        out = self._stack_out(out, r, 'precondition_multi')
        self._check(self.lib.ofdft_precondition_multi(self._ctx, _ptr(r), self.npts, _ptr(out), self.npts, B, kappa2, self._stream()),
                    'ofdft_precondition_multi')
        return out

    @property
    def volume(self):
        """cell volume of the last set_cell"""
        if self._box_key is None:
            raise RuntimeError('set_cell has not been called')
        return abs(float(np.linalg.det(np.frombuffer(self._box_key, dtype=np.float64).reshape(3, 3))))

    # -- validation entry points
    def rfftn(self, x):
        x = self._grid_tensor(x, 'x')
        out = torch.empty(self.shape[0], self.shape[1], self.shape[2] // 2 + 1, dtype=self.cdtype, device=self.device)
        self._check(self.lib.ofdft_rfftn(self._ctx, _ptr(x), _ptr(out), self._stream()), 'ofdft_rfftn')
        return out

    def irfftn(self, xk):
        want = (self.shape[0], self.shape[1], self.shape[2] // 2 + 1)
        if tuple(xk.shape) != want or xk.dtype != self.cdtype:
            raise ValueError('spectrum must be %s of shape %s' % (self.cdtype, want))
        xk = xk.detach().contiguous()
        out = torch.empty(self.shape, dtype=self.dtype, device=self.device)
        self._check(self.lib.ofdft_irfftn(self._ctx, _ptr(xk), _ptr(out), self._stream()), 'ofdft_irfftn')
        return out

    def debug_math(self, kind, x):
        """the lean transcendentals of csrc/fastmath.h applied elementwise (validation only)"""
        x = x.detach().contiguous()
        if x.dtype != self.dtype or not x.is_cuda:
            raise TypeError('x must be a %s device tensor' % self.dtype)
        out = torch.empty_like(x)
        kinds = {'rcp': 0, 'log': 1, 'exp': 2, 'rsixth': 3, 'cbrt': 4, 'inv': 5}
        self._check(self.lib.ofdft_debug_math(self._ctx, kinds[kind], _ptr(x), _ptr(out), x.numel(), self._stream()), 'ofdft_debug_math')
        return out

    def query(self, what):
        v = C.c_double(0.0)
        self._check(self.lib.ofdft_query(self._ctx, int(what), C.byref(v)), 'ofdft_query')
        return v.value

    def set_option(self, option, value):
        self._check(self.lib.ofdft_set_option(self._ctx, int(option), float(value)), 'ofdft_set_option')
        self._options[int(option)] = float(value)
        return self

    def option(self, option):
        """the value last given to ``set_option`` for this option on this engine, or None if it was never set (the library's default holds)"""
        return self._options.get(int(option))


    def stress(self, den):
        """per-term stress tensors {term name: 3x3 numpy array, Ha/bohr^3} for the active terms at fixed electron number
        (get_stress semantics, functional_tools.py:73-101); the ion-electron entry is zero (see ions.ion_electron_stress)"""
        den = self._grid_tensor(den, 'den')
        if self.dtype != torch.double:       # stress is fp64 work: widen the density and use the fp64 sibling engine
            if self._box_key is None or self._terms_key is None:
                raise RuntimeError('Engine.stress: set_cell and set_terms must be called first')
            sib = engine_for(self.global_shape, self.device)
            sib._box_key, sib._terms_key = None, None          # the sibling is shared: always (re)configure it
            sib._check(sib.lib.ofdft_set_cell(sib._ctx, np.frombuffer(self._box_key, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))),
                       'ofdft_set_cell')
            sib._check(sib.lib.ofdft_set_terms(sib._ctx, self._terms_key[0],
                                               np.frombuffer(self._terms_key[1], dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double)),
                                               N.NPARAMS), 'ofdft_set_terms')
            return sib.stress(den.double())
        buf = (C.c_double * (N.NTERMS * 9))()
        self._check(self.lib.ofdft_stress(self._ctx, C.c_void_p(den.data_ptr()), buf, self._stream()), 'ofdft_stress')
        a = np.array(list(buf), dtype=np.float64).reshape(N.NTERMS, 3, 3)
        return N.per_term(a, self._mask())

    def potential_strain_gradient(self, den):
        """v_eps,kl, kl = xx, yy, zz, yz, xz, xy -> [6, n0, n1, n2]: the derivative of the potential dE/dn of the active terms
        with respect to the strain eps_kl (h -> h (I + eps)) at fixed grid values of ``den``, the mean density of the
        Wang-Teter kernel following the cell (ofdft_potential_strain_gradient).  ion_electron contributes
        nothing here (ions.ionic_potential_strain_gradient).  Single GPU and fp64, the terms of ``hessian_vector``."""
        if self.dtype != torch.double:
            raise NotImplementedError('Engine.potential_strain_gradient is fp64 work (libofdft_hip.so); an fp32 engine does not serve it')
        from . import optimize
        why = optimize.gga_strain_refusal(self)
        if why:
            raise NotImplementedError('Engine.potential_strain_gradient: ' + why)
        den = self._grid_tensor(den, 'den')
        out = torch.empty((6,) + tuple(den.shape), dtype=den.dtype, device=den.device)
        self._check(self.lib.ofdft_potential_strain_gradient(self._ctx, _ptr(den), _ptr(out), self._stream()),
                    'ofdft_potential_strain_gradient')
        return out

    def strain_hessian(self, den):
        """{term name: [3, 3, 3, 3] numpy array, Ha}: d^2 E_t / d eps_mn d eps_pq at eps = 0 under h -> h (I + eps) at fixed grid
        values of chi and fixed N, so that the density scales as 1 / det(I + eps).  hartree, vw and wt_nl come
        from ofdft_strain_hessian; tf, lda_x and the LDA correlations depend on J = det(I + eps) alone:
        E_J (d_mn d_pq - d_mq d_np) + E_JJ d_mn d_pq with E_J = vol tr(sigma_t) / 3 (``stress``) and E_JJ = int n (H_t n)
        (``hessian_vector``); with several correlation terms active their entries carry the shares ``stress`` gives them, and only
        their sum is meaningful.  The ion_electron entry is zero (ions.ion_electron_strain_hessian).  Single GPU and fp64."""
        if self.dtype != torch.double:
            raise NotImplementedError('Engine.strain_hessian is fp64 work (libofdft_hip.so); an fp32 engine does not serve it')
        from . import optimize
        why = optimize.gga_strain_refusal(self)
        if why:
            raise NotImplementedError('Engine.strain_hessian: ' + why)
        den = self._grid_tensor(den, 'den')
        buf = (C.c_double * (N.NTERMS * 81))()
        self._check(self.lib.ofdft_strain_hessian(self._ctx, _ptr(den), buf, self._stream()), 'ofdft_strain_hessian')
        out = N.per_term(np.array(list(buf), dtype=np.float64).reshape(N.NTERMS, 3, 3, 3, 3), self._mask())
        local = [t for t in ('tf', 'lda_x', 'pz_c', 'pw_c', 'chachiyo_c') if self._mask() & N.TERM_BITS[t]]
        if local:
            sig = self.stress(den)
            q, _hv = self.hessian_vector(den, den, want_terms=True)
            eye = np.eye(3)
            dd, dx = np.einsum('mn,pq->mnpq', eye, eye), np.einsum('mq,np->mnpq', eye, eye)
            for t in local:
                E_J = self.volume * float(np.trace(sig[t])) / 3.0
                out[t] = E_J * (dd - dx) + float(q[t]) * dd
        return out

    def set_profiling(self, on):
        self._check(self.lib.ofdft_set_profiling(self._ctx, 1 if on else 0), 'ofdft_set_profiling')

    def profile(self):
        """-> {kernel class: (total ms, launches)} accumulated since set_profiling(True)."""
        out = {}
        buf = C.create_string_buffer(64)
        for i in range(self.lib.ofdft_profile_count(self._ctx)):
            ms, n = C.c_double(0.0), C.c_longlong(0)
            self._check(self.lib.ofdft_profile_get(self._ctx, i, buf, 64, C.byref(ms), C.byref(n)), 'ofdft_profile_get')
            out[buf.value.decode()] = (ms.value, n.value)
        return out

    @property
    def fast_path(self):
        return bool(self.query(N.Q_FAST_PATH))


_ENGINES = {}


# extents whose line transforms run in registers / LDS, i.e. grids that take the fused pipelines (csrc/engine_ctx.h:
# line_extent_ok / row_extent_ok); every other extent works too, through chirp-z line transforms and the unfused pipeline
FUSED_EXTENTS_MIXED = (48, 96, 120, 144, 160, 192, 240, 250, 270, 288, 320, 384, 480)       # both builds (fp32 since round 3)


def fused_extents(axis=0, dtype=torch.double, nranks=1):
    """sorted extents along `axis` (0, 1: lines; 2: the real-to-complex rows) served by the fused pipelines"""
    lo, hi = (16, 2048) if axis == 2 else (8, 1024)
    out = {1 << k for k in range(3, 12) if lo <= (1 << k) <= hi}
    out |= set(FUSED_EXTENTS_MIXED)
    if nranks > 1 and axis < 2:                       # slabs: axes 0 and 1 are cut into nranks pieces
        out = {e for e in out if e % nranks == 0}
    return sorted(out)


def next_fast_extent(n, axis=0, dtype=torch.double, nranks=1):
    """smallest fused-pipeline extent >= n along `axis` (ValueError beyond the largest one)"""
    for e in fused_extents(axis, dtype, nranks):
        if e >= n:
            return e
    raise ValueError('no fused-pipeline extent >= %d along axis %d' % (n, axis))


def ecut2shape_fast(energy_cutoff, box_vecs, dtype=torch.double, nranks=1):
    """Grid shape for an energy cutoff (eV) and lattice vectors (Angstrom): the reference's rule (system.py:74-89,
    1 + 2 ceil(k_cut / |b_i|) points per axis -- always odd) rounded UP per axis to the next extent the fused pipelines
    serve, so the cutoff is never lowered.  Returns (shape, reference_shape)."""
    import numpy as np
    A_per_b, eV_per_Ha = 5.29177210903e-11 * 1e10, 4.3597447222071e-18 / 1.602176634e-19       # CODATA 2018, as system.py:27-31
    bvs = np.asarray(box_vecs, dtype=float) / A_per_b
    kcut = np.sqrt(2.0 * float(energy_cutoff) / eV_per_Ha)
    ref = tuple(int(1 + 2 * np.ceil(kcut / (2 * np.pi / np.sqrt((bvs[i] ** 2).sum())))) for i in range(3))
    return tuple(next_fast_extent(r, i, dtype, nranks) for i, r in enumerate(ref)), ref


def engine_for(shape, device, dtype=torch.double):
    """One cached Engine per (shape, device, dtype)."""
    dev = torch.device(device)
    key = (tuple(int(s) for s in shape), dev.type, dev.index if dev.index is not None else 0, dtype)
    e = _ENGINES.get(key)
    if e is None:
        e = _ENGINES[key] = Engine(shape, dev, dtype=dtype)
    return e
