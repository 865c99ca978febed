"""Density optimisation on top of the engine's closure: the caller side of the hot path.

`optimize_density` mirrors the control flow and stopping rules of the reference's
`System.optimize_density` (src/professad/system.py:774-908) for its default method: chi = sqrt(n) as the
unconstrained variable, a fixed-step limited-memory BFGS (history 8, at most 6 inner iterations / 7 closure calls
per outer step, step 0.1; the reference instantiates its vendored optimiser that way, system.py:822), energy
differences in eV against `ntol`, convergence only counted after the 5th outer iteration.

`FixedStepLBFGS` is a from-scratch implementation of that algorithm (standard two-loop recursion with the
y.s > 1e-10 |s|^2 curvature test and gamma = y.s / y.y scaling, reference semantics
_optimizers/lbfgs/lbfgsnew.py:512-769) that keeps the (s, y) history as two [m, N] device matrices so the
two-loop dot products and updates are batched tensor ops on the GPU.

`VectorFreeLBFGS` is the same algorithm arranged for the GPU: the history lives behind the
`ofdft_lbfgs_*` C ABI and every inner iteration is ONE multi-dot sweep (all inner products of {s, y, g} with the
stored pairs) plus ONE multi-axpy sweep (direction, chi update, gradient copy) -- about 40 grid-sized reads/writes
instead of the ~135 of the op-by-op form -- while the two-loop recursion itself runs here on the (2m+1) coefficients
of the direction in the basis {S_j, Y_j, g}.  On several ranks the sweep's local sums need one small all-reduce.

`TruncatedNewton` (`n_method='TN'`, the optimiser PROFESS itself defaults to) and `density_response` are the second-order
consumers: both solve with the Hessian of E[chi] by conjugate gradients whose vectors live behind `ofdft_cg_*` and whose
products are `ofdft_hessian_vector_chi` (`HipCgBackend`, `solve_projected`).  Single GPU, fp64.  With
`precondition` (off by default) the solve is preconditioned by the kinetic operator 1 / (k^2 + kappa^2) (`ofdft_precondition`;
DESIGN.md §9i), which takes the grid out of its iteration count.  `density_response_multi` (and `batch=` of the drivers in
force_constants.py and elastic.py) runs up to eight such solves in lockstep on `HipCgMultiBackend` (`ofdft_cgm_*`,
`ofdft_hessian_vector_chi_multi`, `ofdft_precondition_multi`): one product, one preconditioner call and one launch
per sweep for all right-hand sides.
"""
import ctypes as C
import math

import numpy as np
import torch

EV_PER_HA = 4.3597447222071e-18 / 1.602176634e-19      # system.py:27-33


class FixedStepLBFGS:
    def __init__(self, x, lr=0.1, history_size=8, max_iter=6, tolerance_grad=1e-5, tolerance_change=1e-9):
        self.x = x                                   # flat view is taken lazily; updated in place
        self.lr, self.m, self.max_iter = float(lr), int(history_size), int(max_iter)
        self.max_eval = self.max_iter * 5 // 4       # lbfgsnew.py:69-70
        self.tol_g, self.tol_c = tolerance_grad, tolerance_change
        n = x.numel()
        self.S = torch.zeros(self.m, n, dtype=x.dtype, device=x.device)
        self.Y = torch.zeros(self.m, n, dtype=x.dtype, device=x.device)
        self.count = 0                                # valid pairs (oldest first in rows 0..count-1)
        self.gamma = 1.0
        self.total_iter = 0
        self.d = None
        self.t = None
        self.g_prev = None
        self.func_evals = 0

    def _push(self, s, y):
        if self.count == self.m:
            self.S = torch.roll(self.S, -1, 0)
            self.Y = torch.roll(self.Y, -1, 0)
            self.count -= 1
        self.S[self.count].copy_(s)
        self.Y[self.count].copy_(y)
        self.count += 1

    def _direction(self, g):
        """-H g by the two-loop recursion over the stored pairs."""
        k = self.count
        q = g.neg()
        if k == 0:
            return q * self.gamma
        S, Y = self.S[:k], self.Y[:k]
        rho = 1.0 / (S * Y).sum(1)
        al = torch.empty(k, dtype=g.dtype, device=g.device)
        for i in range(k - 1, -1, -1):
            al[i] = torch.dot(S[i], q) * rho[i]
            q.add_(Y[i], alpha=-float(al[i]))
        r = q * self.gamma
        for i in range(k):
            be = torch.dot(Y[i], r) * rho[i]
            r.add_(S[i], alpha=float(al[i] - be))
        return r

    def step(self, closure):
        """One outer step: closure() -> (loss float, flat gradient tensor); x is updated in place.
        Returns the loss of the first closure call (as the reference's optimiser does)."""
        x = self.x.view(-1)
        loss0, g = closure()
        loss = loss0
        evals = 1
        self.func_evals += 1
        g = g.reshape(-1)
        g1 = float(g.abs().sum())
        if g1 <= self.tol_g:
            return loss0
        n_iter = 0
        while n_iter < self.max_iter and not math.isnan(float(g.norm())):
            n_iter += 1
            self.total_iter += 1
            if self.total_iter == 1:
                d = g.neg()
                self.count = 0
                self.gamma = 1.0
            else:
                y = g - self.g_prev
                s = self.d * self.t
                ys = float(torch.dot(y, s))
                sn = float(s.norm())
                if ys > 1e-10 * sn * sn:                          # lbfgsnew.py:622
                    self._push(s, y)
                    self.gamma = ys / float(torch.dot(y, y))
                d = self._direction(g)
            self.g_prev = g.clone()
            prev_loss = loss
            t = min(1.0, 1.0 / g1) * self.lr if self.total_iter == 1 else self.lr
            gtd = float(torch.dot(g, d))
            x.add_(d, alpha=t)                                     # fixed step, no line search
            self.d, self.t = d, t
            if n_iter != self.max_iter:
                loss, g = closure()
                g = g.reshape(-1)
                g1 = float(g.abs().sum())
                evals += 1
                self.func_evals += 1
                if math.isnan(g1):
                    break
            if n_iter == self.max_iter or evals >= self.max_eval:
                break
            if g1 <= self.tol_g or gtd > -self.tol_c:
                break
            if float((d * t).abs().sum()) <= self.tol_c or abs(loss - prev_loss) < self.tol_c:
                break
        return loss0


class HipLbfgsBackend:
    """History and sweeps on the device (ofdft_lbfgs_* in libofdft_hip.so; no CPU fallback)."""

    def __init__(self, n, history, device, dtype=torch.double):
        from . import _native as N
        self.dtype = dtype
        self.lib = N.load(N.F64 if dtype == torch.double else N.F32)      # the vectors take the library's precision
        self.device = torch.device(device)
        # the device index is resolved exactly as Engine does: a bare 'cuda' means torch's current device
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device('cuda', idx)
        self._h = C.c_void_p(0)
        rc = self.lib.ofdft_lbfgs_create(C.byref(self._h), int(n), int(history), idx)
        if rc != 0:
            raise RuntimeError('ofdft_lbfgs_create failed with code %d' % rc)
        self._buf = (C.c_double * (6 * 8 + 7))()
        self._cs, self._cy, self._cg = (C.c_double * 8)(), (C.c_double * 8)(), 0.0
        self.n = int(n)

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError('%s: %s' % (what, self.lib.ofdft_lbfgs_last_error(self._h).decode()))

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _vec(self, t, name):
        if not (t.is_cuda and t.dtype == self.dtype and t.is_contiguous() and t.numel() == self.n):
            raise ValueError('%s must be a contiguous %s device tensor of %d elements' % (name, self.dtype, self.n))
        return C.c_void_p(t.data_ptr())

    def dots(self, g):
        k = C.c_int(0)
        self._check(self.lib.ofdft_lbfgs_dots(self._h, self._vec(g, 'g'), self._buf, C.byref(k), self._stream()), 'ofdft_lbfgs_dots')
        return np.array(self._buf[:6 * k.value + 7], dtype=np.float64), k.value

    def dots_raw(self, g):
        """the sums left in the backend's own buffer (for `direction`): -> (number of pairs, tail = s.s, s.y, y.y, g.s, g.y, g.g, |g|_1)"""
        k = C.c_int(0)
        self._check(self.lib.ofdft_lbfgs_dots(self._h, self._vec(g, 'g'), self._buf, C.byref(k), self._stream()), 'ofdft_lbfgs_dots')
        kv = k.value
        return kv, self._buf[6 * kv:6 * kv + 7]

    def set_dots(self, vals):
        """put all-reduced sums back into the buffer `direction` reads"""
        for i, v in enumerate(vals):
            self._buf[i] = v

    def direction(self, k, first):
        """curvature test + commit + Gram blocks + two-loop recursion, natively (ofdft_lbfgs_direction) -> g.d; the coefficients
        stay in the backend for `update_direct`"""
        cg, gtd = C.c_double(0.0), C.c_double(0.0)
        self._check(self.lib.ofdft_lbfgs_direction(self._h, self._buf, int(k), 1 if first else 0, self._cs, self._cy, C.byref(cg),
                                                   C.byref(gtd), None, None), 'ofdft_lbfgs_direction')
        self._cg = cg.value
        return gtd.value

    def update_direct(self, t, x, g):
        """x += t d with the coefficients of the last `direction`; nothing waits for the stream (`abs_step` reads the sum later)"""
        self._check(self.lib.ofdft_lbfgs_update(self._h, self._cs, self._cy, self._cg, float(t), self._vec(x, 'x'), self._vec(g, 'g'),
                                                None, self._stream()), 'ofdft_lbfgs_update')

    def abs_step(self):
        out = C.c_double(0.0)
        self._check(self.lib.ofdft_lbfgs_abs_step(self._h, C.byref(out)), 'ofdft_lbfgs_abs_step')
        return out.value

    def commit(self, push):
        self._check(self.lib.ofdft_lbfgs_commit(self._h, 1 if push else 0), 'ofdft_lbfgs_commit')

    def update(self, cs, cy, cg, t, x, g):
        dp = C.POINTER(C.c_double)
        cs = np.ascontiguousarray(cs, dtype=np.float64)
        cy = np.ascontiguousarray(cy, dtype=np.float64)
        out = C.c_double(0.0)
        self._check(self.lib.ofdft_lbfgs_update(self._h, cs.ctypes.data_as(dp), cy.ctypes.data_as(dp), float(cg), float(t),
                                                self._vec(x, 'x'), self._vec(g, 'g'), C.byref(out), self._stream()),
                    'ofdft_lbfgs_update')
        return out.value

    def reset(self):
        self._check(self.lib.ofdft_lbfgs_reset(self._h), 'ofdft_lbfgs_reset')

    def close(self):
        if self._h:
            self.lib.ofdft_lbfgs_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VectorFreeLBFGS:
    """FixedStepLBFGS with the vectors behind a backend (`dots`, `commit`, `update`) and the recursion on coefficients.

    Gram blocks kept on the host for the stored pairs (oldest first): SS[i,j] = S_i.S_j, SY[i,j] = S_i.Y_j,
    YY[i,j] = Y_i.Y_j.  `all_reduce(vec) -> vec` sums the sweeps' local scalars over ranks (None on one GPU)."""

    def __init__(self, x, backend, lr=0.1, history_size=8, max_iter=6, tolerance_grad=1e-5, tolerance_change=1e-9,
                 all_reduce=None):
        self.x, self.b = x, backend
        self.lr, self.m, self.max_iter = float(lr), int(history_size), int(max_iter)
        self.max_eval = self.max_iter * 5 // 4       # lbfgsnew.py:69-70
        self.tol_g, self.tol_c = tolerance_grad, tolerance_change
        self.all_reduce = all_reduce
        self.SS = np.zeros((0, 0))
        self.SY = np.zeros((0, 0))
        self.YY = np.zeros((0, 0))
        self.gamma = 1.0
        self.total_iter = 0
        self.func_evals = 0
        self.info = None

    # ---- sweep 1: everything the iteration needs to know about the new gradient
    def _analyse(self, g):
        vals, k = self.b.dots(g.view(-1))
        if self.all_reduce is not None:
            vals = self.all_reduce(vals)
        v = vals[:6 * k].reshape(2, k, 3)        # [S|Y][j][s,y,g]
        tail = vals[6 * k:]
        self.info = dict(k=k, sS=v[0, :, 0], yS=v[0, :, 1], gS=v[0, :, 2], sY=v[1, :, 0], yY=v[1, :, 1], gY=v[1, :, 2],
                         ss=tail[0], sy=tail[1], yy=tail[2], gs=tail[3], gy=tail[4], gg=tail[5], g1=tail[6])
        return self.info

    def _push(self, f):
        """append the candidate pair's row / column to the Gram blocks (dropping the oldest pair when full)"""
        k = f['k']
        sS, yS, sY, yY, gS, gY = f['sS'], f['yS'], f['sY'], f['yY'], f['gS'], f['gY']
        SS, SY, YY = self.SS, self.SY, self.YY
        if k == self.m:
            SS, SY, YY = SS[1:, 1:], SY[1:, 1:], YY[1:, 1:]
            sS, yS, sY, yY, gS, gY = sS[1:], yS[1:], sY[1:], yY[1:], gS[1:], gY[1:]
            k -= 1
        n = k + 1
        nSS, nSY, nYY = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
        nSS[:k, :k], nSY[:k, :k], nYY[:k, :k] = SS, SY, YY
        nSS[k, :k] = nSS[:k, k] = sS
        nSS[k, k] = f['ss']
        nYY[k, :k] = nYY[:k, k] = yY
        nYY[k, k] = f['yy']
        nSY[k, :k] = sY              # s_new . Y_j
        nSY[:k, k] = yS              # S_j . y_new
        nSY[k, k] = f['sy']
        self.SS, self.SY, self.YY = nSS, nSY, nYY
        return np.append(gS, f['gs']), np.append(gY, f['gy'])

    def _coefficients(self, gS, gY, gg):
        """two-loop recursion (lbfgsnew.py:649-663) on the coefficients of the direction in {S_j, Y_j, g}"""
        k = self.SS.shape[0]
        dS, dY, dg = np.zeros(k), np.zeros(k), -1.0
        rho = 1.0 / np.diag(self.SY) if k else np.zeros(0)
        al = np.zeros(k)
        for i in range(k - 1, -1, -1):
            al[i] = (dS @ self.SS[:, i] + dY @ self.SY[i, :] + dg * gS[i]) * rho[i]
            dY[i] -= al[i]
        dS *= self.gamma
        dY *= self.gamma
        dg *= self.gamma
        for i in range(k):
            be = (dS @ self.SY[:, i] + dY @ self.YY[:, i] + dg * gY[i]) * rho[i]
            dS[i] += al[i] - be
        gtd = dS @ gS + dY @ gY + dg * gg
        return dS, dY, dg, gtd

    def step(self, closure):
        """Same contract as FixedStepLBFGS.step."""
        if hasattr(self.b, 'direction'):
            return self._step_native(closure)
        loss0, g = closure()
        loss = loss0
        evals = 1
        self.func_evals += 1
        f = self._analyse(g)
        g1 = f['g1']
        if g1 <= self.tol_g:
            return loss0
        n_iter = 0
        while n_iter < self.max_iter and not math.isnan(f['gg']):
            n_iter += 1
            self.total_iter += 1
            if self.total_iter == 1:
                self.b.commit(False)
                self.SS = self.SY = self.YY = np.zeros((0, 0))
                self.gamma = 1.0
                gS, gY = np.zeros(0), np.zeros(0)
            else:
                push = f['sy'] > 1e-10 * f['ss']                      # lbfgsnew.py:622 (sn*sn = s.s)
                self.b.commit(push)
                if push:
                    gS, gY = self._push(f)
                    self.gamma = f['sy'] / f['yy']
                else:
                    gS, gY = f['gS'], f['gY']
            cs, cy, cg, gtd = self._coefficients(gS, gY, f['gg'])
            prev_loss = loss
            t = min(1.0, 1.0 / g1) * self.lr if self.total_iter == 1 else self.lr
            abs_step = self.b.update(cs, cy, cg, t, self.x.view(-1), g.view(-1))       # x += t d, g_prev = g
            if self.all_reduce is not None:
                abs_step = float(self.all_reduce(np.array([abs_step]))[0])
            if n_iter != self.max_iter:
                loss, g = closure()
                f = self._analyse(g)
                g1 = f['g1']
                evals += 1
                self.func_evals += 1
                if math.isnan(g1):
                    break
            if n_iter == self.max_iter or evals >= self.max_eval:
                break
            if g1 <= self.tol_g or gtd > -self.tol_c:
                break
            if abs_step <= self.tol_c or abs(loss - prev_loss) < self.tol_c:
                break
        return loss0

    # ---- the same iteration with the host side of the recursion inside the library (ofdft_lbfgs_direction): per inner
    # iteration two ctypes calls and no numpy between the sweeps; the update does not wait for its stream (the closure
    # evaluation that follows synchronises, the |step| sum is read after it)
    def _dots_native(self, g):
        k, tail = self.b.dots_raw(g.view(-1))
        if self.all_reduce is not None:
            vals = self.all_reduce(np.array(self.b._buf[:6 * k + 7], dtype=np.float64))
            self.b.set_dots(vals)
            tail = [float(v) for v in vals[6 * k:]]
        return k, tail           # tail = s.s, s.y, y.y, g.s, g.y, g.g, |g|_1

    def _step_native(self, closure):
        loss0, g = closure()
        loss = loss0
        evals = 1
        self.func_evals += 1
        k, tail = self._dots_native(g)
        g1 = tail[6]
        if g1 <= self.tol_g:
            return loss0
        n_iter = 0
        while n_iter < self.max_iter and not math.isnan(tail[5]):
            n_iter += 1
            self.total_iter += 1
            gtd = self.b.direction(k, self.total_iter == 1)
            prev_loss = loss
            t = min(1.0, 1.0 / g1) * self.lr if self.total_iter == 1 else self.lr
            self.b.update_direct(t, self.x.view(-1), g.view(-1))                       # x += t d, g_prev = g
            last = n_iter == self.max_iter
            if not last:
                loss, g = closure()                                                   # (synchronises the stream)
                k, tail = self._dots_native(g)
                g1 = tail[6]
                evals += 1
                self.func_evals += 1
                if math.isnan(g1):
                    break
            if last or evals >= self.max_eval:
                break
            if g1 <= self.tol_g or gtd > -self.tol_c:
                break
            abs_step = self.b.abs_step()
            if self.all_reduce is not None:
                abs_step = float(self.all_reduce(np.array([abs_step]))[0])
            if abs_step <= self.tol_c or abs(loss - prev_loss) < self.tol_c:
                break
        return loss0


class TwoPointGradientDescent:
    """Barzilai-Borwein two-point gradient descent on one flat variable -- the reference's alternative density optimiser
    (`n_method='TPGD'`, system.py:823-824; _optimizers/tpgd/two_point_gradient_descent.py:25-65): one closure call per step,
    step length (dx . dx) / (dx . dg) from the previous point, the fixed `lr` on the first step or when the quotient is not
    positive.  `all_reduce(vec) -> vec` sums the two local dot products over ranks (None on one GPU)."""

    def __init__(self, x, lr=0.1, all_reduce=None):
        if lr <= 0.0:
            raise ValueError('lr must be positive')
        self.x, self.lr, self.all_reduce = x, float(lr), all_reduce
        self.x_prev = self.g_prev = None
        self.func_evals = 0
        self.total_iter = 0

    def step(self, closure):
        loss, g = closure()
        self.func_evals += 1
        alpha = self.lr
        if self.x_prev is not None:
            dx, dg = self.x - self.x_prev, g - self.g_prev
            dots = torch.stack(((dx * dx).sum(dtype=torch.double), (dx * dg).sum(dtype=torch.double))).cpu().numpy()
            if self.all_reduce is not None:
                dots = self.all_reduce(dots)
            if dots[1] != 0.0 and dots[0] / dots[1] > 0.0:
                alpha = float(dots[0] / dots[1])
        self.x_prev, self.g_prev = self.x.clone(), g.clone()
        self.x.add_(g, alpha=-alpha)
        self.total_iter += 1
        return loss


# ------------------------------------------------------------------------------------------------ second order
CG_RUNNING, CG_CONVERGED, CG_MAXITER, CG_CURVATURE = 0, 1, 2, 3      # exit reasons of a solve (OFDFT_CG_*; _native.CG_REASONS)
_UNSERVED = ('wgc99_nl', 'pbe_x', 'pbe_c', 'gga_k', 'vwgtf', 'nlk')    # terms without a second derivative (ofdft_hessian_vector)
_GGA_OPT_IN = ('pbe_x', 'pbe_c')           # ... served by the single-column products once the engine's OPT_HVP_GGA is 1
_WGC_OPT_IN = ('wgc99_nl',)                # ... once its OPT_HVP_WGC is 1
_GGA_MISSING = {
    'batch': 'batching is what is missing -- the multi-column product has no PBE stage; use the single-column path (batch=None, '
             'density_response, Engine.hessian_vector_chi)',
    'strain': 'the strain derivative of PBE is not built (elastic constants, bulk modulus, Engine.strain_hessian, '
              'Engine.potential_strain_gradient)',
}
_WGC_MISSING = {
    'batch': 'batching is what is missing -- the multi-column product has no WGC99 stage; use the single-column path (batch=None, '
             'density_response, Engine.hessian_vector_chi)',
    'strain': 'the strain derivative of WGC99 is not built (elastic constants, bulk modulus, Engine.strain_hessian, '
              'Engine.potential_strain_gradient)',
}


def hvp_gga_enabled(engine):
    """the engine's OPT_HVP_GGA is 1 (an engine without `Engine.option`, such as a test's fake, counts as off)"""
    from . import _native as N
    option = getattr(engine, 'option', None)
    return option is not None and option(N.OPT_HVP_GGA) == 1


def hvp_wgc_enabled(engine):
    """the engine's OPT_HVP_WGC is 1 (as `hvp_gga_enabled`)"""
    from . import _native as N
    option = getattr(engine, 'option', None)
    return option is not None and option(N.OPT_HVP_WGC) == 1


def _opted_in(engine):
    """term name -> what the batched and strain paths lack for it, for the terms the engine's options open to the single-column products"""
    opened = {}
    if hvp_wgc_enabled(engine):
        opened.update((name, _WGC_MISSING) for name in _WGC_OPT_IN)
    if hvp_gga_enabled(engine):
        opened.update((name, _GGA_MISSING) for name in _GGA_OPT_IN)
    return opened


def gga_strain_refusal(engine):
    """None, or -- with the engine's OPT_HVP_GGA (OPT_HVP_WGC) at 1 and pbe_x / pbe_c (wgc99_nl) among its terms -- why its strain
    entries do not serve them: the products then let these terms through, the strain entries say so before any device work"""
    from . import _native as N
    opened = _opted_in(engine)
    if opened and engine._terms_key is not None:
        for name in _UNSERVED:
            if name in opened and engine._mask() & N.TERM_BITS[name]:
                return 'no second derivative of the term %s here: %s' % (name, opened[name]['strain'])
    return None


def second_order_refusal(engine, gga_missing=None):
    """None, or why the engine cannot serve Hessian-vector products in chi (what ofdft_hessian_vector_chi itself refuses).
    pbe_x / pbe_c pass when the engine's OPT_HVP_GGA is 1 and wgc99_nl when its OPT_HVP_WGC is 1 -- unless `gga_missing` names what
    the asking path lacks for them ('batch': the multi-column entries, 'strain': the elastic entries), which keep refusing them by
    name."""
    from . import _native as N
    if getattr(engine, 'comm', None) is not None:
        return 'the Hessian-vector product is served by single-GPU contexts; a slab-decomposed DistEngine has no second derivative'
    if engine.dtype != torch.double:
        return 'the Hessian-vector product is fp64 work (libofdft_hip.so); an fp32 engine does not serve it'
    mask = engine._mask()
    opened = _opted_in(engine)
    for name in _UNSERVED:
        if mask & N.TERM_BITS[name]:
            if name in opened:
                if gga_missing is None:
                    continue
                return 'no second derivative of the term %s here: %s' % (name, opened[name][gga_missing])
            return 'no second derivative of the term %s' % name
    if mask & N.TERM_BITS['wt_nl'] and np.frombuffer(engine._terms_key[1], dtype=np.float64)[12] != 0.0:
        return 'no second derivative of the stabilised Wang-Teter style functional (wts_kind)'
    return None


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def check_precondition(value):
    """the `precondition` argument of the second-order entries: None (plain conjugate gradients), 'auto' or kappa^2 > 0"""
    if value is None or value == 'auto':
        return value
    if isinstance(value, (int, float)) and not isinstance(value, bool) and value > 0.0 and math.isfinite(value):
        return float(value)
    raise ValueError("precondition must be None, 'auto' or a positive finite kappa^2 [1/bohr^2], got %r" % (value,))


def kinetic_kappa2(n_elec, volume):
    """kappa^2 = (4/3) k_F^2 of the mean density: the Thomas-Fermi part of the shift the Hessian adds to c dV (-lap)"""
    return (4.0 / 3.0) * (3.0 * math.pi ** 2 * n_elec / volume) ** (2.0 / 3.0)


class _HipCgBase:
    """What the device backends for one column and for several share: the preconditioner setting and its kappa^2, the error check
    and the release of the handle `_h`.  `_abi` is the prefix of the solver's entries (ofdft_cg or ofdft_cgm)."""
    _abi = None

    @property
    def preconditioned(self):
        return self.precondition is not None

    def set_precondition(self, precondition):
        """takes effect at the next `start`"""
        self.precondition = check_precondition(precondition)

    def _kappa2(self, n_elec):
        return kinetic_kappa2(n_elec, self.eng.volume) if self.precondition == 'auto' else self.precondition

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError('%s failed (%d): %s' % (what, rc, getattr(self.lib, self._abi + '_last_error')(self._h).decode()))

    def hv(self, den, w):
        return self.eng.hessian_vector(den, w)

    def close(self):
        if self._h:
            getattr(self.lib, self._abi + '_destroy')(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipCgBackend(_HipCgBase):
    """Conjugate gradients for P H P x = b on the device (ofdft_cg_* and ofdft_hessian_vector_chi in libofdft_hip.so; no CPU
    fallback): x, r, p, q live behind the handle, the engine's product reads p and writes q in place.
    `precondition`: None (plain), 'auto' (kappa^2 = (4/3) (3 pi^2 N / vol)^(2/3) from the `n_elec` of each solve) or kappa^2 > 0:
    every iteration then opens with z = F^-1[r^ / (k^2 + kappa^2)] (`ofdft_precondition`) and `ofdft_cg_direction`; `set_precondition`
    changes it between solves."""
    _abi = 'ofdft_cg'

    def __init__(self, engine, precondition=None):
        why = second_order_refusal(engine)
        if why:
            raise NotImplementedError(why)
        self.precondition = check_precondition(precondition)
        self.eng, self.lib = engine, engine.lib
        self.dV = engine.volume / engine.npts
        self._h = C.c_void_p(0)
        rc = self.lib.ofdft_cg_create(C.byref(self._h), engine.npts, engine._dev_index)
        if rc != 0:
            raise RuntimeError('ofdft_cg_create failed with code %d' % rc)
        self._p, self._q = C.c_void_p(0), C.c_void_p(0)
        self._check(self.lib.ofdft_cg_vectors(self._h, None, None, C.byref(self._p), C.byref(self._q)), 'ofdft_cg_vectors')
        self._scal = (C.c_double * 5)()
        self._r, self._z = C.c_void_p(0), C.c_void_p(0)

    def start(self, phi, b, rtol, maxiter):
        e = self.eng
        phi, b = e._grid_tensor(phi, 'chi'), e._grid_tensor(b, 'b')          # (held until the call returns)
        self._check(self.lib.ofdft_cg_set_preconditioned(self._h, 1 if self.preconditioned else 0), 'ofdft_cg_set_preconditioned')
        if self.preconditioned and not self._z:
            self._check(self.lib.ofdft_cg_vectors(self._h, None, C.byref(self._r), None, None), 'ofdft_cg_vectors')
            self._check(self.lib.ofdft_cg_z(self._h, C.byref(self._z)), 'ofdft_cg_z')
        self._check(self.lib.ofdft_cg_start(self._h, _vp(phi), _vp(b), float(rtol), int(maxiter), None, e._stream()), 'ofdft_cg_start')

    def product(self, phi, g, n_elec, reuse):
        """q = H p -> (p.q, phi.q)"""
        e = self.eng
        phi, g = e._grid_tensor(phi, 'chi'), e._grid_tensor(g, 'g')
        e._check(self.lib.ofdft_hessian_vector_chi(e._ctx, _vp(phi), self._p, _vp(g), float(n_elec), self._q, self._scal,
                                                   1 if reuse else 0, e._stream()), 'ofdft_hessian_vector_chi')
        return self._scal[0], self._scal[1]

    def pre_direction(self, phi, n_elec):
        """preconditioned mode, in front of every product: z = M^-1 r, then p = P z + beta p -> exit reason"""
        e = self.eng
        e._check(self.lib.ofdft_precondition(e._ctx, self._r, self._z, float(self._kappa2(n_elec)), e._stream()), 'ofdft_precondition')
        reason = C.c_int(0)
        phi = e._grid_tensor(phi, 'chi')
        self._check(self.lib.ofdft_cg_direction(self._h, _vp(phi), None, C.byref(reason), e._stream()), 'ofdft_cg_direction')
        return reason.value

    def step(self, phi, p_dot_q, phi_dot_q):
        reason = C.c_int(0)
        phi = self.eng._grid_tensor(phi, 'chi')
        self._check(self.lib.ofdft_cg_step(self._h, _vp(phi), float(p_dot_q), float(phi_dot_q), C.byref(reason), self.eng._stream()),
                    'ofdft_cg_step')
        return reason.value

    def status(self):
        it, reason, rel = C.c_int(0), C.c_int(0), C.c_double(0.0)
        self._check(self.lib.ofdft_cg_status(self._h, C.byref(it), C.byref(reason), C.byref(rel)), 'ofdft_cg_status')
        return it.value, reason.value, rel.value

    def solution(self):
        x = torch.empty(self.eng.shape, dtype=self.eng.dtype, device=self.eng._dev_exact)
        self._check(self.lib.ofdft_cg_solution(self._h, C.c_void_p(x.data_ptr()), self.eng._stream()), 'ofdft_cg_solution')
        return x


def solve_projected(backend, phi, g, b, n_elec, rtol, maxiter):
    """Conjugate gradients for P H P x = b at phi (P = I - phi phi^T / phi.phi; g: the closure gradient there, None at a stationary
    point) until |r| <= rtol |b|, `maxiter` iterations or non-positive curvature.  The first product runs with reuse_density = 0,
    the others with 1.  A backend whose `preconditioned` is true forms its direction in `pre_direction` before every product
    (z = M^-1 r, p = P z + beta p); the stopping rule is the same, on the unpreconditioned residual.
    -> (x, iterations, exit reason CG_*, |r| / |b|, products)"""
    backend.start(phi, b, rtol, maxiter)
    _it, reason, _rel = backend.status()
    pre = bool(getattr(backend, 'preconditioned', False))
    products = 0
    while reason == CG_RUNNING:
        if pre and backend.pre_direction(phi, n_elec) != CG_RUNNING:
            break
        pq, phiq = backend.product(phi, g, n_elec, products > 0)
        products += 1
        reason = backend.step(phi, pq, phiq)
    iters, reason, rel = backend.status()
    return backend.solution(), iters, reason, rel, products


class TruncatedNewton:
    """Line-search truncated Newton on chi (the optimiser PROFESS itself defaults to), on a backend that solves the projected
    Newton equation (`HipCgBackend`).  Per outer step: conjugate gradients for P H P x = -g down to the forcing term
    |r| < min(0.5, sqrt|g|) |g| or `cg_maxiter` iterations, leaving at non-positive curvature with the current x (the steepest
    descent direction if that happens at once); then Armijo backtracking on the closure energy from t = 1 (halving, c1 = 1e-4,
    at most 20 trials; an energy within a few roundings of the bound passes, so that the last, tiny steps are not lost to the
    noise of the energy sum).  The accepted trial's energy and gradient open the next step: one evaluation per step when the full
    step is taken.  A step at |g|_2 <= `tolerance_grad` does nothing."""

    def __init__(self, x, backend, n_elec, cg_maxiter=50, tolerance_grad=1e-10, c1=1e-4, max_trials=20):
        self.x, self.b, self.n_elec = x, backend, float(n_elec)
        self.cg_maxiter, self.tol_g, self.c1, self.max_trials = int(cg_maxiter), float(tolerance_grad), float(c1), int(max_trials)
        self.func_evals = self.hvp_count = self.total_iter = 0
        self.cg_log = []                 # per solve: (products, exit reason, |g|_2 before it)
        self._at = None                  # (E, g) at the current x

    def step(self, closure):
        """closure() -> (E, gradient) at the current x, which is updated in place.  Returns the energy before the step."""
        if self._at is None:
            self._at = closure()
            self.func_evals += 1
        E, g = self._at
        gnorm = math.sqrt(float((g * g).sum()))
        if not gnorm > self.tol_g:
            return E
        dx, _it, reason, _rel, nprod = solve_projected(self.b, self.x, g, -g, self.n_elec, min(0.5, math.sqrt(gnorm)), self.cg_maxiter)
        self.hvp_count += nprod
        self.cg_log.append((nprod, reason, gnorm))
        gtd = float((g * dx).sum())
        if not gtd < 0.0:                # (cannot happen with a positive definite projected Hessian; never walk uphill)
            dx, gtd = -g, -gnorm * gnorm
        x0 = self.x + 0.0
        slack = 4.0 * np.finfo(np.float64).eps * abs(E)
        t = 1.0
        for _trial in range(self.max_trials):
            self.x[...] = x0 + t * dx
            Et, gt = closure()
            self.func_evals += 1
            if Et <= E + self.c1 * t * gtd + slack:
                self._at = (Et, gt)
                break
            t *= 0.5
        else:                            # no acceptable step: stay where the step began; the closure's last call belongs to that point
            self.x[...] = x0
            self._at = closure()
            self.func_evals += 1
        self.total_iter += 1
        return E


def _own_backend_only(who, backend, precondition):
    if backend is not None and precondition is not None:
        raise ValueError('%s: `precondition` configures the backend the call builds; with `backend` given, set it on that backend' % who)


def _response_density(chi, n_elec, dV):
    """-> (c, n) with n = c chi^2 the density of chi (any scale), sum n dV = n_elec"""
    c = n_elec / (float((chi * chi).sum()) * dV)
    return c, c * chi * chi


def _response_rhs(chi, c, n, n_elec, dV, dv):
    """the right-hand side -2 c chi (dv - sum(dv n) dV / N) dV of the response to the perturbation dv"""
    shift = float((dv * n).sum()) * dV / n_elec
    return (-2.0 * c * dV) * chi * (dv - shift)


def _response_result(b, chi, c, n, n_elec, dV, dv, dchi):
    """-> (dn, dmu) of the perturbation dv from the solution dchi"""
    dn = 2.0 * c * chi * dchi
    return dn, float((n * (b.hv(n, dn) + dv)).sum()) * dV / n_elec


def density_response(engine, chi, n_elec, dv, rtol=1e-10, maxiter=500, backend=None, precondition=None):
    """First-order change of the ground-state density under a perturbation `dv` of the external potential, at the ground state
    `chi` (any scale) of the engine's terms: the implicit derivative of the minimiser, one conjugate-gradient solve with the
    Hessian of E[chi],  P H P dchi = -2 c chi (dv - sum(dv n) dV / N) dV  with g = 0.  Returns a dict with dn = 2 c chi dchi
    (sum dn = 0), dmu = sum n (hv(n, dn) + dv) dV / N, the iteration count, the relative residual and the exit reason.
    Single GPU, fp64 and the terms `Engine.hessian_vector` serves; anything else raises NotImplementedError.  (`backend`: another
    solver with HipCgBackend's methods -- the tests' numpy double.)  `precondition`: None, 'auto' or kappa^2 > 0, as `HipCgBackend`
    takes it: the kinetic preconditioner, which makes the iteration count independent of the grid; the result is the same
    solution to `rtol`."""
    _own_backend_only('density_response', backend, precondition)
    b = backend if backend is not None else HipCgBackend(engine, precondition)
    dV = b.dV
    c, n = _response_density(chi, n_elec, dV)
    rhs = _response_rhs(chi, c, n, n_elec, dV, dv)
    dchi, iters, reason, rel, nprod = solve_projected(b, chi, None, rhs, n_elec, rtol, maxiter)
    dn, dmu = _response_result(b, chi, c, n, n_elec, dV, dv, dchi)
    if backend is None:
        b.close()
    return dict(dn=dn, dmu=dmu, iterations=iters, rel_residual=rel, reason=reason, hvp_count=nprod)


# ---- several right-hand sides per solve
MULTI_MAX = 8      # OFDFT_MULTI_MAX


def check_batch(value):
    """the `batch` argument of the response drivers: None (one solve per right-hand side) or an integer 1 .. 8 columns per solve"""
    if value is None:
        return None
    if isinstance(value, (int, np.integer)) and not isinstance(value, bool) and 1 <= int(value) <= MULTI_MAX:
        return int(value)
    raise ValueError('batch must be None or an integer in 1 .. %d (OFDFT_MULTI_MAX), got %r' % (MULTI_MAX, value))


def _stack(fields):
    return torch.stack(list(fields)) if isinstance(fields[0], torch.Tensor) else np.stack(list(fields))


class HipCgMultiBackend(_HipCgBase):
    """`HipCgBackend` for up to `ncols` right-hand sides in lockstep (ofdft_cgm_*, ofdft_hessian_vector_chi_multi and
    ofdft_precondition_multi in libofdft_hip.so; no CPU fallback): the columns of x, r, p, q, z live behind the
    handle, one product call forms q_j = H p_j for all of them.  The methods of `HipCgBackend`, taking a stack `bs` [B, *shape]
    and returning per-column lists.  Not block Krylov: each column is the recurrence a solo solve runs, with its own
    coefficients, exit reason and iteration count; a column that has ended is frozen while the others go on."""
    _abi = 'ofdft_cgm'

    def __init__(self, engine, ncols, precondition=None):
        why = second_order_refusal(engine, gga_missing='batch')
        if why:
            raise NotImplementedError(why)
        if check_batch(ncols) is None:
            raise ValueError('ncols must be an integer in 1 .. %d' % MULTI_MAX)
        self.precondition = check_precondition(precondition)
        self.eng, self.lib, self.ncols_max = engine, engine.lib, int(ncols)
        self.dV = engine.volume / engine.npts
        self._h = C.c_void_p(0)
        rc = self.lib.ofdft_cgm_create(C.byref(self._h), engine.npts, self.ncols_max, engine._dev_index)
        if rc != 0:
            raise RuntimeError('ofdft_cgm_create failed with code %d' % rc)
        self._r, self._p, self._q, self._z = C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0)
        ld = C.c_longlong(0)
        self._check(self.lib.ofdft_cgm_vectors(self._h, None, C.byref(self._r), C.byref(self._p), C.byref(self._q), C.byref(ld)),
                    'ofdft_cgm_vectors')
        self._ld = ld.value
        self._scal = (C.c_double * (5 * MULTI_MAX))()
        self._pq, self._phiq = (C.c_double * MULTI_MAX)(), (C.c_double * MULTI_MAX)()
        self.ncols = 0

    def start(self, phi, bs, rtol, maxiter):
        e = self.eng
        phi = e._grid_tensor(phi, 'chi')
        B = e._grid_stack(bs, 'bs')
        if B > self.ncols_max:
            raise ValueError('bs stacks %d columns, this backend was built for %d' % (B, self.ncols_max))
        self._check(self.lib.ofdft_cgm_set_preconditioned(self._h, 1 if self.preconditioned else 0), 'ofdft_cgm_set_preconditioned')
        if self.preconditioned and not self._z:
            self._check(self.lib.ofdft_cgm_z(self._h, C.byref(self._z)), 'ofdft_cgm_z')
        self._check(self.lib.ofdft_cgm_start(self._h, _vp(phi), _vp(bs), e.npts, B, float(rtol), int(maxiter), None, e._stream()),
                    'ofdft_cgm_start')
        self.ncols = B

    def product(self, phi, n_elec, reuse):
        """q_j = H p_j for every column -> (p_j.q_j, phi.q_j) as two lists"""
        e = self.eng
        phi = e._grid_tensor(phi, 'chi')
        e._check(self.lib.ofdft_hessian_vector_chi_multi(e._ctx, _vp(phi), self._p, self._ld, self.ncols, float(n_elec), self._q, self._ld,
                                                         self._scal, 1 if reuse else 0, e._stream()), 'ofdft_hessian_vector_chi_multi')
        return [self._scal[5 * j] for j in range(self.ncols)], [self._scal[5 * j + 1] for j in range(self.ncols)]

    def _reasons(self):
        return [s[1] for s in self.status()]

    def pre_direction(self, phi, n_elec):
        """preconditioned mode, in front of every product: z_j = M^-1 r_j, then p_j = P z_j + beta_j p_j -> exit reasons"""
        e = self.eng
        e._check(self.lib.ofdft_precondition_multi(e._ctx, self._r, self._ld, self._z, self._ld, self.ncols, float(self._kappa2(n_elec)),
                                                   e._stream()), 'ofdft_precondition_multi')
        running = C.c_int(0)
        phi = e._grid_tensor(phi, 'chi')
        self._check(self.lib.ofdft_cgm_direction(self._h, _vp(phi), None, C.byref(running), e._stream()), 'ofdft_cgm_direction')
        return self._reasons()

    def step(self, phi, p_dot_q, phi_dot_q):
        running = C.c_int(0)
        phi = self.eng._grid_tensor(phi, 'chi')
        for j in range(self.ncols):
            self._pq[j], self._phiq[j] = float(p_dot_q[j]), float(phi_dot_q[j])
        self._check(self.lib.ofdft_cgm_step(self._h, _vp(phi), self._pq, self._phiq, C.byref(running), self.eng._stream()), 'ofdft_cgm_step')
        return self._reasons()

    def status(self):
        """-> [(iterations, reason, |r| / |b|)] per column"""
        out = []
        it, reason, rel = C.c_int(0), C.c_int(0), C.c_double(0.0)
        for j in range(self.ncols):
            self._check(self.lib.ofdft_cgm_status(self._h, j, C.byref(it), C.byref(reason), C.byref(rel)), 'ofdft_cgm_status')
            out.append((it.value, reason.value, rel.value))
        return out

    def solution(self):
        x = torch.empty((self.ncols,) + tuple(self.eng.shape), dtype=self.eng.dtype, device=self.eng._dev_exact)
        self._check(self.lib.ofdft_cgm_solution(self._h, C.c_void_p(x.data_ptr()), self.eng.npts, self.eng._stream()), 'ofdft_cgm_solution')
        return x


def solve_projected_multi(backend, phi, bs, n_elec, rtol, maxiter):
    """`solve_projected` at a stationary point (g = 0) for the stack `bs` [B, ...] of right-hand sides, the B recurrences in
    lockstep on a backend with `HipCgMultiBackend`'s methods: one product call per iteration serves every column, a column that
    has ended stays as it ended, and the run ends when every column has.
    -> (x [B, ...], iterations [B], exit reasons [B], |r| / |b| [B], batched products)"""
    backend.start(phi, bs, rtol, maxiter)
    reasons = [s[1] for s in backend.status()]
    pre = bool(getattr(backend, 'preconditioned', False))
    products = 0
    while any(r == CG_RUNNING for r in reasons):
        if pre:
            reasons = backend.pre_direction(phi, n_elec)
            if not any(r == CG_RUNNING for r in reasons):
                break
        pq, phiq = backend.product(phi, n_elec, products > 0)
        products += 1
        reasons = backend.step(phi, pq, phiq)
    st = backend.status()
    return backend.solution(), [s[0] for s in st], [s[1] for s in st], [s[2] for s in st], products


def density_response_multi(engine, chi, n_elec, dvs, rtol=1e-10, maxiter=500, backend=None, precondition=None):
    """`density_response` to the B = 1 .. 8 perturbations stacked in `dvs` [B, ...] by one batched solve (`solve_projected_multi`).
    Returns the keys of `density_response`: `dn` as [B, ...]; `dmu`, `iterations`, `rel_residual` and `reason` as lists over the
    columns; `hvp_count` counts batched products.  Column j is the result `density_response` gives for dvs[j], to rounding; each
    dmu_j is defined exactly as there.  (`backend`: another solver with HipCgMultiBackend's methods -- the tests' numpy double.)"""
    _own_backend_only('density_response_multi', backend, precondition)
    B = len(dvs)
    if check_batch(B) is None:
        raise ValueError('dvs must stack 1 .. %d perturbations' % MULTI_MAX)
    b = backend if backend is not None else HipCgMultiBackend(engine, B, precondition)
    try:
        dV = b.dV
        c, n = _response_density(chi, n_elec, dV)
        rhs = [_response_rhs(chi, c, n, n_elec, dV, dvs[j]) for j in range(B)]
        dchi, iters, reasons, rels, nprod = solve_projected_multi(b, chi, _stack(rhs), n_elec, rtol, maxiter)
        dn, dmu = zip(*[_response_result(b, chi, c, n, n_elec, dV, dvs[j], dchi[j]) for j in range(B)])
    finally:
        if backend is None:
            b.close()
    return dict(dn=_stack(dn), dmu=list(dmu), iterations=iters, rel_residual=rels, reason=reasons, hvp_count=nprod)


def resolve_batch(who, backend, batch):
    """the `batch` argument of a driver: it configures the backend the call builds; a caller's backend carries its own (`batch`
    attribute, None without one), as it carries its own preconditioner"""
    if backend is not None and batch is not None:
        raise ValueError('%s: `batch` configures the backend the call builds; with `backend` given, set it on that backend' % who)
    return check_batch(batch if backend is None else getattr(backend, 'batch', None))


def batched_responses(b, engine, chi, n_elec, dvs, batch, rtol, maxiter):
    """the results `density_response` would give for each of the perturbations `dvs` (a list), in their order, from batched solves
    of `batch` columns on the driver backend's multi solver `b.cgm(batch)`; `hvp_count` of the first of a group carries the group's
    batched products, the others 0"""
    out = []
    for j0 in range(0, len(dvs), batch):
        group = dvs[j0:j0 + batch]
        r = density_response_multi(engine, chi, n_elec, _stack(group), rtol=rtol, maxiter=maxiter, backend=b.cgm(batch))
        for j in range(len(group)):      # (dn: a field of its own, not a view into the stack)
            out.append(dict(dn=r['dn'][j].clone() if isinstance(r['dn'], torch.Tensor) else r['dn'][j].copy(), dmu=r['dmu'][j], iterations=r['iterations'][j], rel_residual=r['rel_residual'][j],
                            reason=r['reason'][j], hvp_count=r['hvp_count'] if j == 0 else 0))
    return out


# ---- what the drivers over `density_response` share (force_constants.py, elastic.py)
A_PER_BOHR = 5.29177210903e-11 * 1e10      # system.py:27-33 (CODATA 2018)


def normalise_species(species):
    """-> (species with fp64 [n, 3] coordinates, frac [N, 3] and charges [N] of all ions).  The global ion index is the position
    in the concatenation of the species, and n_elec = charges.sum()."""
    species = [(np.asarray(torch.as_tensor(f).detach().cpu().numpy(), dtype=np.float64).reshape(-1, 3), tab) for f, tab in species]
    frac = np.concatenate([f for f, _t in species], axis=0)
    charges = np.concatenate([np.full(f.shape[0], float(tab[2])) for f, tab in species])
    return species, frac, charges


def response_refusal(engine, pme_order=None, gga_missing=None):
    """None, or why a driver over `density_response` with ions cannot run on this engine (raised before any device work);
    `gga_missing` as `second_order_refusal` takes it"""
    from . import _native as N
    if pme_order:
        return ('particle-mesh Ewald (PME, pme_order=%r) is not served: the derivative of the B-spline spread is not built; '
                'use the exact structure factor' % (pme_order,))
    why = second_order_refusal(engine, gga_missing)
    if why:
        return why
    if not engine._mask() & N.TERM_BITS['ion_electron']:
        return 'the term set has no ion_electron term: nothing couples the density to the ions'
    return None


class HipResponseBackend:
    """Base of the drivers' device backends: the engine on its cell, dV, the conjugate gradients (`cg`, closed by `close`) and the
    check of the ground state.  Grids are torch tensors of the engine; the small results are numpy arrays."""

    def __init__(self, engine, box_vecs, species):
        self.eng, self.box, self.species = engine, box_vecs, species
        engine.set_cell(box_vecs)
        self.volume = engine.volume
        self.dV = engine.volume / engine.npts
        self.cg = HipCgBackend(engine)
        self._cgm = None

    def cgm(self, ncols):
        """the solver of the batched solves (`batch`), built on first use for `ncols` columns with the preconditioner of `cg`"""
        if self._cgm is None or self._cgm.ncols_max < ncols:
            if self._cgm is not None:
                self._cgm.close()
            self._cgm = HipCgMultiBackend(self.eng, ncols)
        self._cgm.set_precondition(self.cg.precondition)
        return self._cgm

    def ground_state_gradient(self, chi, n_elec):
        """max|g| / dV of the closure at chi with v_ext rebuilt from the ions"""
        from . import ions
        vext = ions.ionic_potential(self.eng, self.box, self.species)
        _E, _mu, g = self.eng.energy_grad_chi(chi, n_elec, vext)
        return float(g.abs().max()) / self.dV

    def close(self):
        self.cg.close()
        if self._cgm is not None:
            self._cgm.close()


def new_solve_log():
    """what a driver reports of its response solves, in solve order"""
    return dict(iterations=[], rel_residual=[], reason=[], hvp_count=0)


def log_solve(log, r):
    """append the result `r` of one `density_response` call"""
    for k in ('iterations', 'rel_residual', 'reason'):
        log[k].append(r[k])
    log['hvp_count'] += r['hvp_count']


def warn_unconverged(who, log, maxiter, what):
    """Without `precondition` the iteration count of the conjugate gradients grows with the grid, so a solve
    may end at maxiter.  `what`: what is then not accurate."""
    import warnings
    bad = sum(x != CG_CONVERGED for x in log['reason'])
    if bad:
        warnings.warn('%s: %d of %d response solves did not converge within maxiter=%d (see `reason`, `rel_residual`); %s'
                      % (who, bad, len(log['reason']), maxiter, what))


def optimize_density(engine, n_elec, vext=None, chi0=None, ntol=1e-7, n_conv_cond_count=3, n_step_size=0.1,
                     n_maxiter=1000, conv_target='dE', verbose=False, volume=None, optimizer='fused', n_method='LBFGS',
                     tn_cg_maxiter=50, tn_gtol=1e-10, tn_precondition=None):
    """Minimise E[n = N_e chi^2 / int chi^2] with the engine's terms.  Returns a dict with the converged density,
    chi, energy [Ha], iteration count and the convergence history.

    engine: an `Engine` (cell and terms already set) or a `DistEngine` (slab-decomposed: chi / vext / the results are
    this rank's x-slabs and every rank runs this function; the optimiser's scalars are all-reduced, so all ranks take
    identical decisions); `volume` = cell volume (needed when chi0 is None to start from the uniform density, as
    System.optimize_density does after System.__init__).  `optimizer`: 'fused' (HIP sweeps, `VectorFreeLBFGS`) or
    'torch' (`FixedStepLBFGS` on torch tensors; single GPU only).
    With an fp32 engine the energies carry ~1e-6 relative round-off: choose `ntol` above that noise (the default 1e-7 eV
    suits fp64) or the loop runs to `n_maxiter`.
    `n_method`: 'LBFGS', 'TPGD' (the reference's two) or 'TN', truncated Newton (`TruncatedNewton`: at most `tn_cg_maxiter`
    Hessian-vector products per Newton equation, no step once |g|_2 <= `tn_gtol`); 'TN' needs a single-GPU fp64 `Engine` whose
    terms all have a second derivative, and raises NotImplementedError otherwise.  The result's `hvp_count` is the number of
    Hessian-vector products taken (0 for the other methods).  `tn_precondition`: None, 'auto' or kappa^2 > 0, the kinetic
    preconditioner of the Newton equations (`HipCgBackend`); ValueError with another method."""
    if conv_target not in ('dE', 'dEdchi', 'euler'):
        raise ValueError("Only 'dE', 'dEdchi' or 'euler' recognized as 'conv_target' argument")       # system.py:889-890
    if n_method not in ('LBFGS', 'TPGD', 'TN'):
        raise ValueError("Only 'LBFGS', 'TPGD' or 'TN' recognized for 'n_method' argument")           # system.py:826
    if tn_precondition is not None and n_method != 'TN':
        raise ValueError("tn_precondition belongs to n_method='TN'")
    check_precondition(tn_precondition)
    if n_method == 'TN':
        why = second_order_refusal(engine)
        if why:
            raise NotImplementedError("n_method='TN': " + why)
    if conv_target != 'dE' and volume is None:
        raise ValueError("conv_target=%r needs `volume` (the cell volume fixes dV)" % conv_target)
    comm = getattr(engine, 'comm', None)                    # DistEngine
    multi = comm is not None and comm.active
    if comm is not None:
        shape, dev, dtype = engine.plan.local_shape, engine.stages.device, engine.stages.dtype
        npts_global = engine.npts_global
    else:
        shape, dev, dtype = engine.shape, engine.device, engine.dtype
        npts_global = int(np.prod(shape))

    def gsum(x):                                            # sum over ranks of a python float
        return float(comm.all_reduce_sum(np.array([x]), dev)[0]) if multi else x

    def gmax(x):
        if not multi:
            return x
        import torch.distributed as dist
        t = torch.tensor([x], dtype=torch.double, device=dev if comm.backend == 'nccl' else 'cpu')
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=comm.group)
        return float(t[0])
    if chi0 is None:
        if volume is None:
            raise ValueError('volume is needed for the uniform start')
        chi = torch.full(shape, math.sqrt(n_elec / volume), dtype=dtype, device=dev)
    else:
        chi = chi0.detach().clone().to(device=dev, dtype=dtype)
    state = {}

    def closure():
        E_terms, mu, g = engine.energy_grad_chi(chi, n_elec, vext)
        state.update(E=sum(E_terms.values()), mu=mu, g=g, E_terms=E_terms)
        if conv_target == 'euler':          # the Euler residual belongs to the density of THIS call (see below): keep its chi
            if 'chi_c' not in state:
                state['chi_c'] = torch.empty_like(chi)
            state['chi_c'].copy_(chi)
        return state['E'], g

    if n_method == 'TN':
        opt = TruncatedNewton(chi, HipCgBackend(engine, tn_precondition), n_elec, cg_maxiter=tn_cg_maxiter, tolerance_grad=tn_gtol)
    elif n_method == 'TPGD':        # system.py:823-824
        hook = (lambda v: comm.all_reduce_sum(np.ascontiguousarray(v, dtype=np.float64), dev)) if multi else None
        opt = TwoPointGradientDescent(chi, lr=n_step_size, all_reduce=hook)
    elif optimizer == 'fused':      # device-resident history, two sweeps per inner iteration
        hook = (lambda v: comm.all_reduce_sum(np.ascontiguousarray(v, dtype=np.float64), dev)) if multi else None
        opt = VectorFreeLBFGS(chi, HipLbfgsBackend(chi.numel(), 8, dev, dtype), lr=n_step_size, history_size=8, max_iter=6,
                              all_reduce=hook)
    elif optimizer == 'torch' and not multi:      # op-by-op form on torch tensors
        opt = FixedStepLBFGS(chi, lr=n_step_size, history_size=8, max_iter=6)
    else:
        raise ValueError("optimizer must be 'fused' or 'torch'")
    E_prev = closure()[0] * EV_PER_HA
    history, conv = [], 0
    dV = None
    for it in range(1, int(round(n_maxiter)) + 1):
        opt.step(closure)
        # like the reference, energy / gradient are those of the LAST closure call of the step (system.py:869-871)
        E = state['E'] * EV_PER_HA
        dE = E - E_prev
        E_prev = E
        if dV is None and volume is not None:
            dV = volume / npts_global
        dEdchi = gmax(float(state['g'].abs().max())) / dV if dV else float('nan')
        history.append((it, E, dE, dEdchi))
        if verbose:
            print('%5d %16.8f %12.4e %12.4e' % history[-1])
        if conv_target == 'euler':
            # max |mu - dE/dn| (system.py:377-412) at the density of the step's LAST closure call -- the reference's System keeps
            # that density (system.py:833-834) and check_density_convergence differentiates at it, not at the chi the optimiser
            # moved to afterwards.  No extra evaluation: the closure's gradient is chi.grad = 2 c chi (dE/dn - mu) dV
            # (system.py:850-853), so mu - dE/dn = -chi.grad / (2 c chi dV) wherever chi != 0.
            chi_c = state['chi_c'].double()
            c2 = n_elec / (gsum(float((chi_c * chi_c).sum())) / npts_global * volume)
            res = torch.where(chi_c != 0, state['g'].double() / (2.0 * c2 * dV * chi_c), torch.zeros_like(chi_c))
            stop = gmax(float(res.abs().max()))
        else:
            stop = abs(dE) if conv_target == 'dE' else dEdchi
        if it > 5:
            conv = conv + 1 if stop < ntol else 0
        if conv == n_conv_cond_count:
            break
    E_terms, mu, g = engine.energy_grad_chi(chi, n_elec, vext)
    ntilde = gsum(float((chi.double() * chi.double()).sum())) / npts_global * (volume if volume is not None else 1.0)
    den = (n_elec / ntilde) * chi * chi if volume is not None else None
    if n_method == 'TN':
        opt.b.close()
    return dict(chi=chi, den=den, E_Ha=sum(E_terms.values()), E_terms=E_terms, mu=mu, iterations=it,
                converged=conv == n_conv_cond_count, history=history, func_evals=opt.func_evals,
                hvp_count=getattr(opt, 'hvp_count', 0))
