// C ABI of the device-resident conjugate-gradient solver (cg_kernels.h, include/ofdft_hip.h).  Included once, at the end of
// engine.hip, behind lbfgs_abi.h whose helpers (lfail's pattern, DeviceScope) it follows.
// One solver: ofdft_cgm_* below run ncols recurrences in lockstep behind one handle, every sweep one launch and one fetch for all
// columns.  The columns share nothing but phi and S: each keeps its own alpha, beta, rho, phi.r, exit reason and
// iteration count, and ends on its own; the run ends when every column has.  ofdft_cg_*, at the end of this file, are that solver
// with ncols_max = 1: wrappers that pass the scalars as one-element arrays and report column 0.
#pragma once
#include <cstdarg>
#include <new>

#include "cg_kernels.h"

// the words in which the messages of the two families of entries differ
struct CgWords {
    const char *pfx, *all_have, *directions, *are;
};
static const CgWords kCgOne = {"ofdft_cg", "the solve has", "direction", "is"};
static const CgWords kCgMulti = {"ofdft_cgm", "every column has", "directions", "are"};

struct ofdft_cgm {
    const CgWords* w = &kCgMulti;
    long long n = 0, ld = 0;         // points per column; column stride of the handle's vectors (n rounded up to even)
    int ncols_max = 0, ncols = 0, device = 0;
    real *x = nullptr, *r = nullptr, *p = nullptr, *q = nullptr, *z = nullptr;      // [ncols_max][ld]; z on first use
    bool pre_next = false, pre = false, dir_ready = false, dir_first = false, started = false;
    double *d_partial = nullptr, *d_out = nullptr, *h_out = nullptr;
    int maxiter = 0;
    double S = 0.0, rtol = 0.0;
    struct Col {
        double rho = 0.0, phir = 0.0, rr = 0.0, bb = 0.0;
        int iters = 0, reason = OFDFT_CG_RUNNING;
    } col[kCgmMax];
    char err[256] = "";
};

namespace {

int mfail(ofdft_cgm* o, int code, const char* fmt, ...) {
    if (o) {
        va_list ap;
        va_start(ap, fmt);
        std::vsnprintf(o->err, sizeof(o->err), fmt, ap);
        va_end(ap);
    }
    return code;
}
#define CGM_TRY(o, expr)                                                                \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess) return mfail(o, OFDFT_EHIP, "%s", hipGetErrorString(e_)); \
    } while (0)

int cgm_blocks(const ofdft_cgm* o) {
    long long want = (o->n / 2 + kRedThreads) / kRedThreads;
    return (int)(want < 1 ? 1 : (want > kRedBlocks ? kRedBlocks : want));
}
int cgm_ensure_z(ofdft_cgm* o) {
    if (!o->z) CGM_TRY(o, hipMalloc((void**)&o->z, sizeof(real) * (size_t)o->ld * o->ncols_max));
    return OFDFT_OK;
}
// second-level sums of `ns` scalars per column, all columns in one launch, to the host (one synchronisation): out[col * ns + s].
// The sums of a column the sweep skipped are not defined; the caller reads those of the columns it ran.
int cgm_fetch(ofdft_cgm* o, int blocks, int ns, hipStream_t st) {
    hipLaunchKernelGGL(cgm_reduce_kernel, dim3(ns, o->ncols), dim3(kRedThreads), 0, st, (const double*)o->d_partial, blocks, ns, o->d_out);
    CGM_TRY(o, hipMemcpyAsync(o->h_out, o->d_out, sizeof(double) * ns * o->ncols, hipMemcpyDeviceToHost, st));
    CGM_TRY(o, hipStreamSynchronize(st));
    CGM_TRY(o, hipGetLastError());
    return OFDFT_OK;
}
int cgm_running(const ofdft_cgm* o) {
    int k = 0;
    for (int c = 0; c < o->ncols; ++c) k += o->col[c].reason == OFDFT_CG_RUNNING;
    return k;
}

template <class H>
void cgm_destroy(H* o) {
    if (!o) return;
    DeviceScope device_scope_(o->device);
    for (real* v : {o->x, o->r, o->p, o->q, o->z})
        if (v) (void)hipFree(v);
    if (o->d_partial) (void)hipFree(o->d_partial);
    if (o->d_out) (void)hipFree(o->d_out);
    if (o->h_out) (void)hipHostFree(o->h_out);
    delete o;
}

template <class H>
int cgm_create(H** out, long long n, int ncols_max, int device_id, const CgWords* w) {
    if (!out || n < 1 || ncols_max < 1 || ncols_max > kCgmMax) return OFDFT_EINVAL;
    *out = nullptr;
    H* o = new (std::nothrow) H();
    if (!o) return OFDFT_ENOMEM;
    o->w = w;
    o->n = n;
    o->ld = (n + 1) & ~1LL;
    o->ncols_max = ncols_max;
    o->device = device_id;
    DeviceScope device_scope_(device_id);
    hipError_t e = device_scope_.err;
    const size_t vb = sizeof(real) * (size_t)o->ld * ncols_max;
    for (real** v : {&o->x, &o->r, &o->p, &o->q})
        if (e == hipSuccess) e = hipMalloc((void**)v, vb);
    if (e == hipSuccess) e = hipMalloc((void**)&o->d_partial, sizeof(double) * kRedBlocks * 3 * ncols_max);
    if (e == hipSuccess) e = hipMalloc((void**)&o->d_out, sizeof(double) * 3 * ncols_max);
    if (e == hipSuccess) e = hipHostMalloc((void**)&o->h_out, sizeof(double) * 3 * ncols_max);
    if (e != hipSuccess) {
        cgm_destroy(o);
        return e == hipErrorOutOfMemory ? OFDFT_ENOMEM : OFDFT_EHIP;
    }
    *out = o;
    return OFDFT_OK;
}

}  // namespace

extern "C" {

int ofdft_cgm_create(ofdft_cgm** out, long long n, int ncols_max, int device_id) { return cgm_create(out, n, ncols_max, device_id, &kCgMulti); }

void ofdft_cgm_destroy(ofdft_cgm* o) { cgm_destroy(o); }

const char* ofdft_cgm_last_error(const ofdft_cgm* o) { return o ? o->err : "null handle"; }

int ofdft_cgm_vectors(ofdft_cgm* o, void** x_dev, void** r_dev, void** p_dev, void** q_dev, long long* stride) {
    if (!o) return OFDFT_EINVAL;
    if (x_dev) *x_dev = o->x;
    if (r_dev) *r_dev = o->r;
    if (p_dev) *p_dev = o->p;
    if (q_dev) *q_dev = o->q;
    if (stride) *stride = o->ld;
    return OFDFT_OK;
}

int ofdft_cgm_set_preconditioned(ofdft_cgm* o, int on) {
    if (!o) return OFDFT_EINVAL;
    o->pre_next = on != 0;
    return OFDFT_OK;
}

int ofdft_cgm_z(ofdft_cgm* o, void** z_dev) {
    if (!o || !z_dev) return OFDFT_EINVAL;
    DeviceScope device_scope_(o->device);
    CGM_TRY(o, device_scope_.err);
    if (int rc = cgm_ensure_z(o)) return rc;
    *z_dev = o->z;
    return OFDFT_OK;
}

int ofdft_cgm_start(ofdft_cgm* o, const void* phi_dev, const void* b_dev, long long b_stride, int ncols, double rtol, int maxiter,
                    double* info_host, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!o) return OFDFT_EINVAL;
    if (!phi_dev || !b_dev || !(rtol >= 0.0) || maxiter < 1) return mfail(o, OFDFT_EINVAL, "ofdft_cgm_start: null argument, negative rtol or maxiter < 1");
    if (ncols < 1 || ncols > o->ncols_max)
        return mfail(o, OFDFT_EINVAL, "ofdft_cgm_start: ncols = %d is outside 1 .. %d, the ncols_max of this handle (at most OFDFT_MULTI_MAX = %d)",
                     ncols, o->ncols_max, kCgmMax);
    if (b_stride < o->n) return mfail(o, OFDFT_EINVAL, "ofdft_cgm_start: b_stride is below the points of a column");
    DeviceScope device_scope_(o->device);
    CGM_TRY(o, device_scope_.err);
    o->started = false;
    o->pre = o->pre_next;
    if (o->pre)
        if (int rc = cgm_ensure_z(o)) return rc;
    o->ncols = ncols;
    const real* phi = (const real*)phi_dev;
    const real* b = (const real*)b_dev;
    const int blocks = cgm_blocks(o);
    hipLaunchKernelGGL(cgm_start_dots_kernel, dim3(blocks, ncols), dim3(kRedThreads), 0, st, phi, b, b_stride, o->n, o->d_partial);
    if (int rc = cgm_fetch(o, blocks, 3, st)) return rc;
    double s3[kCgmMax][3];
    for (int c = 0; c < ncols; ++c)
        for (int s = 0; s < 3; ++s) s3[c][s] = o->h_out[3 * c + s];
    const double S = s3[0][1];
    if (!(S > 0.0)) return mfail(o, OFDFT_EINVAL, "%s_start: phi is zero everywhere", o->w->pfx);
    CgmCols cols{};
    for (int c = 0; c < ncols; ++c) cols.a[c] = (real)(s3[c][2] / S);
    cols.active = (1u << ncols) - 1u;
    hipLaunchKernelGGL(cgm_start_kernel, dim3(blocks, ncols), dim3(kRedThreads), 0, st, phi, b, b_stride, cols, o->x, o->r, o->p, o->ld, o->n,
                       o->d_partial);
    if (int rc = cgm_fetch(o, blocks, 1, st)) return rc;
    o->S = S;
    o->rtol = rtol;
    o->maxiter = maxiter;
    o->dir_ready = false;
    o->dir_first = true;
    for (int c = 0; c < ncols; ++c) {
        ofdft_cgm::Col& k = o->col[c];
        k.rr = k.bb = o->h_out[c];
        k.rho = k.phir = 0.0;
        k.iters = 0;
        k.reason = k.rr > 0.0 ? OFDFT_CG_RUNNING : OFDFT_CG_CONVERGED;      // b = 0: x = 0 solves it
        if (info_host) {
            info_host[3 * c] = k.rr;
            info_host[3 * c + 1] = S;
            info_host[3 * c + 2] = s3[c][2];
        }
    }
    o->started = true;
    return OFDFT_OK;
}

int ofdft_cgm_step(ofdft_cgm* o, const void* phi_dev, const double* p_dot_q, const double* phi_dot_q, int* running, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!o) return OFDFT_EINVAL;
    if (!phi_dev || !p_dot_q || !phi_dot_q || !running) return mfail(o, OFDFT_EINVAL, "ofdft_cgm_step: null argument");
    const CgWords& w = *o->w;
    if (!o->started) return mfail(o, OFDFT_ESTATE, "%s_step: %s_start has not been called", w.pfx, w.pfx);
    if (!cgm_running(o)) return mfail(o, OFDFT_ESTATE, "%s_step: %s ended (%s_status)", w.pfx, w.all_have, w.pfx);
    if (o->pre && !o->dir_ready)
        return mfail(o, OFDFT_ESTATE, "%s_step: preconditioned mode, and %s_direction has not formed the %s of this step", w.pfx, w.pfx, w.directions);
    DeviceScope device_scope_(o->device);
    CGM_TRY(o, device_scope_.err);
    const real* phi = (const real*)phi_dev;
    const int blocks = cgm_blocks(o);
    CgmCols up{};
    bool copied = false;
    for (int c = 0; c < o->ncols; ++c) {
        ofdft_cgm::Col& k = o->col[c];
        if (k.reason != OFDFT_CG_RUNNING) continue;
        if (!(p_dot_q[c] > 0.0)) {          // non-positive curvature (or NaN): x stays; before the first update x = p, the steepest descent step
            if (k.iters == 0) {
                CGM_TRY(o, hipMemcpyAsync(o->x + c * o->ld, o->p + c * o->ld, sizeof(real) * (size_t)o->n, hipMemcpyDeviceToDevice, st));
                copied = true;
            }
            k.reason = OFDFT_CG_CURVATURE;
            continue;
        }
        up.a[c] = (real)((o->pre ? k.rho : k.rr) / p_dot_q[c]);
        up.b[c] = (real)(phi_dot_q[c] / o->S);
        up.active |= 1u << c;
    }
    o->dir_ready = false;
    if (up.active) {
        hipLaunchKernelGGL(cgm_update_kernel, dim3(blocks, o->ncols), dim3(kRedThreads), 0, st, phi, (const real*)o->p, (const real*)o->q, up, o->x,
                           o->r, o->ld, o->n, o->d_partial);
        if (int rc = cgm_fetch(o, blocks, 2, st)) return rc;
        CgmCols dir{};
        for (int c = 0; c < o->ncols; ++c) {
            if (!((up.active >> c) & 1u)) continue;
            ofdft_cgm::Col& k = o->col[c];
            k.iters++;
            const double rr_old = k.rr;
            k.rr = o->h_out[2 * c];
            k.phir = o->h_out[2 * c + 1];
            if (k.rr != k.rr) k.reason = OFDFT_CG_CURVATURE;      // a NaN in the product: nothing more to gain from this column
            else if (!(k.rr > o->rtol * o->rtol * k.bb)) k.reason = OFDFT_CG_CONVERGED;
            else if (k.iters >= o->maxiter) k.reason = OFDFT_CG_MAXITER;
            else if (!o->pre) {
                dir.a[c] = (real)(k.phir / o->S);
                dir.b[c] = (real)(k.rr / rr_old);
                dir.active |= 1u << c;
            }
        }
        if (dir.active)
            hipLaunchKernelGGL(cgm_direction_kernel, dim3(blocks, o->ncols), dim3(256), 0, st, phi, (const real*)o->r, dir, o->p, o->ld, o->n);
    } else if (copied) {
        CGM_TRY(o, hipStreamSynchronize(st));      // (only first-step copies x = p were queued)
    }
    CGM_TRY(o, hipGetLastError());
    *running = cgm_running(o);
    return OFDFT_OK;
}

// preconditioned mode, between the update sweep of one step and the product of the next: with z_c = M^-1 r_c in place for every
// running column, rho_c = r_c.P z_c = r_c.z_c - (phi.r_c)(phi.z_c) / S, beta_c = rho_c / rho_c_old (0 after the start) and
// p_c = P z_c + beta_c p_c.  One synchronisation.
int ofdft_cgm_direction(ofdft_cgm* o, const void* phi_dev, double* info_host, int* running, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!o) return OFDFT_EINVAL;
    if (!phi_dev || !running) return mfail(o, OFDFT_EINVAL, "ofdft_cgm_direction: null argument");
    const CgWords& w = *o->w;
    if (!o->started) return mfail(o, OFDFT_ESTATE, "%s_direction: %s_start has not been called", w.pfx, w.pfx);
    if (!o->pre)
        return mfail(o, OFDFT_ESTATE, "%s_direction: the solve runs in plain mode (%s_set_preconditioned before %s_start)", w.pfx, w.pfx, w.pfx);
    if (!cgm_running(o)) return mfail(o, OFDFT_ESTATE, "%s_direction: %s ended (%s_status)", w.pfx, w.all_have, w.pfx);
    if (o->dir_ready)
        return mfail(o, OFDFT_ESTATE, "%s_direction: the %s of this step %s already formed (%s_step)", w.pfx, w.directions, w.are, w.pfx);
    DeviceScope device_scope_(o->device);
    CGM_TRY(o, device_scope_.err);
    const real* phi = (const real*)phi_dev;
    const int blocks = cgm_blocks(o);
    CgmCols run{};
    for (int c = 0; c < o->ncols; ++c)
        if (o->col[c].reason == OFDFT_CG_RUNNING) run.active |= 1u << c;
    hipLaunchKernelGGL(cgm_pre_dots_kernel, dim3(blocks, o->ncols), dim3(kRedThreads), 0, st, phi, (const real*)o->r, (const real*)o->z, run, o->ld,
                       o->n, o->d_partial);
    if (int rc = cgm_fetch(o, blocks, 2, st)) return rc;
    CgmCols dir{};
    for (int c = 0; c < o->ncols; ++c) {
        if (info_host)
            for (int s = 0; s < 4; ++s) info_host[4 * c + s] = 0.0;
        if (!((run.active >> c) & 1u)) continue;
        ofdft_cgm::Col& k = o->col[c];
        const double rz = o->h_out[2 * c], phiz = o->h_out[2 * c + 1];
        const double rho = rz - k.phir * phiz / o->S;
        const double beta = o->dir_first ? 0.0 : rho / k.rho;
        if (info_host) {
            info_host[4 * c] = rz;
            info_host[4 * c + 1] = phiz;
            info_host[4 * c + 2] = rho;
            info_host[4 * c + 3] = beta;
        }
        if (!(rho > 0.0)) {                // M is positive definite: only a NaN or a vanished residual comes here; x stays
            k.reason = OFDFT_CG_CURVATURE;
            continue;
        }
        dir.a[c] = (real)(phiz / o->S);
        dir.b[c] = (real)beta;
        dir.active |= 1u << c;
        k.rho = rho;
    }
    if (dir.active) {
        if (o->dir_first)
            hipLaunchKernelGGL(cgm_pre_direction_kernel<true>, dim3(blocks, o->ncols), dim3(kRedThreads), 0, st, phi, (const real*)o->z, dir, o->p,
                               o->ld, o->n);
        else
            hipLaunchKernelGGL(cgm_pre_direction_kernel<false>, dim3(blocks, o->ncols), dim3(kRedThreads), 0, st, phi, (const real*)o->z, dir, o->p,
                               o->ld, o->n);
    }
    CGM_TRY(o, hipGetLastError());
    o->dir_first = false;
    o->dir_ready = true;
    *running = cgm_running(o);
    return OFDFT_OK;
}

// x of every column of the solve, copied to the caller's stack at its stride (the stream's order; no wait)
int ofdft_cgm_solution(ofdft_cgm* o, void* x_out_dev, long long stride, void* stream) {
    if (!o) return OFDFT_EINVAL;
    if (!x_out_dev) return mfail(o, OFDFT_EINVAL, "ofdft_cgm_solution: null argument");
    if (!o->started) return mfail(o, OFDFT_ESTATE, "%s_solution: %s_start has not been called", o->w->pfx, o->w->pfx);
    if (stride < o->n) return mfail(o, OFDFT_EINVAL, "ofdft_cgm_solution: stride is below the points of a column");
    DeviceScope device_scope_(o->device);
    CGM_TRY(o, device_scope_.err);
    CGM_TRY(o, hipMemcpy2DAsync(x_out_dev, sizeof(real) * (size_t)stride, o->x, sizeof(real) * (size_t)o->ld, sizeof(real) * (size_t)o->n,
                                (size_t)o->ncols, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return OFDFT_OK;
}

int ofdft_cgm_status(const ofdft_cgm* o, int col, int* iterations, int* reason, double* rel_residual) {
    if (!o || col < 0 || col >= o->ncols_max) return OFDFT_EINVAL;
    const ofdft_cgm::Col& k = o->col[col];
    if (iterations) *iterations = k.iters;
    if (reason) *reason = k.reason;
    if (rel_residual) *rel_residual = k.bb > 0.0 ? std::sqrt(k.rr / k.bb) : 0.0;
    return OFDFT_OK;
}

}  // extern "C"

// ================================================================================================================================
// One solve (include/ofdft_hip.h): the handle is the solver above with ncols_max = 1, the entries translate the arguments.  The
// argument checks stay here: OFDFT_EINVAL before any device work, and without a message.
struct ofdft_cg : ofdft_cgm {};

extern "C" {

int ofdft_cg_create(ofdft_cg** out, long long n, int device_id) { return cgm_create(out, n, 1, device_id, &kCgOne); }

void ofdft_cg_destroy(ofdft_cg* o) { cgm_destroy(o); }

const char* ofdft_cg_last_error(const ofdft_cg* o) { return ofdft_cgm_last_error(o); }

int ofdft_cg_start(ofdft_cg* o, const void* phi_dev, const void* b_dev, double rtol, int maxiter, double* info_host, void* stream) {
    if (!o || !phi_dev || !b_dev || !(rtol >= 0.0) || maxiter < 1) return OFDFT_EINVAL;
    return ofdft_cgm_start(o, phi_dev, b_dev, o->n, 1, rtol, maxiter, info_host, stream);
}

int ofdft_cg_vectors(ofdft_cg* o, void** x_dev, void** r_dev, void** p_dev, void** q_dev) {
    return ofdft_cgm_vectors(o, x_dev, r_dev, p_dev, q_dev, nullptr);
}

int ofdft_cg_step(ofdft_cg* o, const void* phi_dev, double p_dot_q, double phi_dot_q, int* reason, void* stream) {
    if (!o || !phi_dev || !reason) return OFDFT_EINVAL;
    int running;
    const int rc = ofdft_cgm_step(o, phi_dev, &p_dot_q, &phi_dot_q, &running, stream);
    if (rc == OFDFT_OK) *reason = o->col[0].reason;
    return rc;
}

int ofdft_cg_set_preconditioned(ofdft_cg* o, int on) { return ofdft_cgm_set_preconditioned(o, on); }

int ofdft_cg_z(ofdft_cg* o, void** z_dev) { return ofdft_cgm_z(o, z_dev); }

int ofdft_cg_direction(ofdft_cg* o, const void* phi_dev, double* info_host, int* reason, void* stream) {
    if (!o || !phi_dev || !reason) return OFDFT_EINVAL;
    int running;
    const int rc = ofdft_cgm_direction(o, phi_dev, info_host, &running, stream);
    if (rc == OFDFT_OK) *reason = o->col[0].reason;
    return rc;
}

// x of the solve, copied to the caller's array (the stream's order; no wait)
int ofdft_cg_solution(ofdft_cg* o, void* x_out_dev, void* stream) {
    if (!o || !x_out_dev) return OFDFT_EINVAL;
    return ofdft_cgm_solution(o, x_out_dev, o->n, stream);
}

int ofdft_cg_status(const ofdft_cg* o, int* iterations, int* reason, double* rel_residual) {
    return ofdft_cgm_status(o, 0, iterations, reason, rel_residual);
}

}  // extern "C"
