// C ABI of the device-resident conjugate-gradient solver (cg_kernels.h, include/ofdft_hip.h).  Included once, at the end of
// engine.hip, behind lbfgs_abi.h whose helpers (lfail's pattern, DeviceScope) it follows.
#pragma once
#include <new>

#include "cg_kernels.h"

struct ofdft_cg {
    long long n = 0;
    int device = 0;
    real *x = nullptr, *r = nullptr, *p = nullptr, *q = nullptr;
    real* z = nullptr;               // preconditioned mode: z = M^-1 r, written by the caller (allocated on first use)
    bool pre_next = false;           // ofdft_cg_set_preconditioned: the mode of the next ofdft_cg_start
    bool pre = false;                // the mode of the running solve
    bool dir_ready = false;          // preconditioned mode: ofdft_cg_direction has formed p for the coming step
    bool dir_first = false;          // ... and none has run since ofdft_cg_start (beta = 0)
    double rho = 0.0, phir = 0.0;    // r.Pz of the last direction; phi.r of the last update sweep
    double *d_partial = nullptr, *d_out = nullptr, *h_out = nullptr;
    bool started = false;
    int iters = 0, maxiter = 0, reason = OFDFT_CG_RUNNING;
    double bb = 0.0, S = 0.0, rr = 0.0, rtol = 0.0;
    char err[256] = "";
};

namespace {

int cfail(ofdft_cg* o, int code, const char* msg) {
    if (o) std::snprintf(o->err, sizeof(o->err), "%s", msg);
    return code;
}
#define CG_TRY(o, expr)                                                           \
    do {                                                                          \
        hipError_t e_ = (expr);                                                   \
        if (e_ != hipSuccess) return cfail(o, OFDFT_EHIP, hipGetErrorString(e_)); \
    } while (0)

int cg_blocks(const ofdft_cg* o) {
    long long want = (o->n / 2 + kRedThreads) / kRedThreads;
    return (int)(want < 1 ? 1 : (want > kRedBlocks ? kRedBlocks : want));
}
int cg_ensure_z(ofdft_cg* o) {
    if (!o->z) CG_TRY(o, hipMalloc((void**)&o->z, sizeof(real) * (size_t)o->n));
    return OFDFT_OK;
}
// second-level sum of `ns` scalars, to the host (one synchronisation)
int cg_fetch(ofdft_cg* o, int blocks, int ns, double* out, hipStream_t st) {
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(ns), dim3(kRedThreads), 0, st, (const double*)o->d_partial, blocks, ns, o->d_out);
    CG_TRY(o, hipMemcpyAsync(o->h_out, o->d_out, sizeof(double) * ns, hipMemcpyDeviceToHost, st));
    CG_TRY(o, hipStreamSynchronize(st));
    CG_TRY(o, hipGetLastError());
    for (int s = 0; s < ns; ++s) out[s] = o->h_out[s];
    return OFDFT_OK;
}

}  // namespace

extern "C" {

int ofdft_cg_create(ofdft_cg** out, long long n, int device_id) {
    if (!out || n < 1) return OFDFT_EINVAL;
    *out = nullptr;
    ofdft_cg* o = new (std::nothrow) ofdft_cg();
    if (!o) return OFDFT_ENOMEM;
    o->n = n;
    o->device = device_id;
    DeviceScope device_scope_(device_id);
    hipError_t e = device_scope_.err;
    const size_t vb = sizeof(real) * (size_t)n;
    for (real** v : {&o->x, &o->r, &o->p, &o->q})
        if (e == hipSuccess) e = hipMalloc((void**)v, vb);
    if (e == hipSuccess) e = hipMalloc((void**)&o->d_partial, sizeof(double) * kRedBlocks * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&o->d_out, sizeof(double) * 4);
    if (e == hipSuccess) e = hipHostMalloc((void**)&o->h_out, sizeof(double) * 4);
    if (e != hipSuccess) {
        ofdft_cg_destroy(o);
        return e == hipErrorOutOfMemory ? OFDFT_ENOMEM : OFDFT_EHIP;
    }
    *out = o;
    return OFDFT_OK;
}

void ofdft_cg_destroy(ofdft_cg* o) {
    if (!o) return;
    DeviceScope device_scope_(o->device);
    for (real* v : {o->x, o->r, o->p, o->q, o->z})
        if (v) (void)hipFree(v);
    if (o->d_partial) (void)hipFree(o->d_partial);
    if (o->d_out) (void)hipFree(o->d_out);
    if (o->h_out) (void)hipHostFree(o->h_out);
    delete o;
}

const char* ofdft_cg_last_error(const ofdft_cg* o) { return o ? o->err : "null handle"; }

int ofdft_cg_start(ofdft_cg* o, const void* phi_dev, const void* b_dev, double rtol, int maxiter, double* info_host, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!o || !phi_dev || !b_dev || !(rtol >= 0.0) || maxiter < 1) return OFDFT_EINVAL;
    DeviceScope device_scope_(o->device);
    CG_TRY(o, device_scope_.err);
    o->started = false;
    o->pre = o->pre_next;
    if (o->pre)
        if (int rc = cg_ensure_z(o)) return rc;
    const real* phi = (const real*)phi_dev;
    const real* b = (const real*)b_dev;
    const int blocks = cg_blocks(o);
    hipLaunchKernelGGL(cg_start_dots_kernel, dim3(blocks), dim3(kRedThreads), 0, st, phi, b, o->n, o->d_partial);
    double s3[3];
    if (int rc = cg_fetch(o, blocks, 3, s3, st)) return rc;
    if (!(s3[1] > 0.0)) return cfail(o, OFDFT_EINVAL, "ofdft_cg_start: phi is zero everywhere");
    hipLaunchKernelGGL(cg_start_kernel, dim3(blocks), dim3(kRedThreads), 0, st, phi, b, (real)(s3[2] / s3[1]), o->x, o->r, o->p, o->n,
                       o->d_partial);
    double rr;
    if (int rc = cg_fetch(o, blocks, 1, &rr, st)) return rc;
    o->bb = rr;              // the norm of the projected right-hand side is the yardstick of the relative residual
    o->S = s3[1];
    o->rr = rr;
    o->rtol = rtol;
    o->maxiter = maxiter;
    o->iters = 0;
    o->dir_ready = false;      // preconditioned mode: p = r of the sweep above is not a direction yet (ofdft_cg_direction forms it)
    o->dir_first = true;
    o->rho = 0.0;
    o->phir = 0.0;             // r = P b
    o->reason = rr > 0.0 ? OFDFT_CG_RUNNING : OFDFT_CG_CONVERGED;      // b = 0: x = 0 solves it
    o->started = true;
    if (info_host) {
        info_host[0] = rr;
        info_host[1] = s3[1];
        info_host[2] = s3[2];
    }
    return OFDFT_OK;
}

int ofdft_cg_vectors(ofdft_cg* o, void** x_dev, void** r_dev, void** p_dev, void** q_dev) {
    if (!o) return OFDFT_EINVAL;
    if (x_dev) *x_dev = o->x;
    if (r_dev) *r_dev = o->r;
    if (p_dev) *p_dev = o->p;
    if (q_dev) *q_dev = o->q;
    return OFDFT_OK;
}

int ofdft_cg_step(ofdft_cg* o, const void* phi_dev, double p_dot_q, double phi_dot_q, int* reason, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!o || !phi_dev || !reason) return OFDFT_EINVAL;
    if (!o->started) return cfail(o, OFDFT_ESTATE, "ofdft_cg_step: ofdft_cg_start has not been called");
    if (o->reason != OFDFT_CG_RUNNING) return cfail(o, OFDFT_ESTATE, "ofdft_cg_step: the solve has ended (ofdft_cg_status)");
    if (o->pre && !o->dir_ready)
        return cfail(o, OFDFT_ESTATE, "ofdft_cg_step: preconditioned mode, and ofdft_cg_direction has not formed the direction of this step");
    DeviceScope device_scope_(o->device);
    CG_TRY(o, device_scope_.err);
    const real* phi = (const real*)phi_dev;
    if (!(p_dot_q > 0.0)) {            // non-positive curvature (or NaN): x stays; before the first update x = p, the steepest descent step
        if (o->iters == 0) {
            CG_TRY(o, hipMemcpyAsync(o->x, o->p, sizeof(real) * (size_t)o->n, hipMemcpyDeviceToDevice, st));
            CG_TRY(o, hipStreamSynchronize(st));
        }
        *reason = o->reason = OFDFT_CG_CURVATURE;
        return OFDFT_OK;
    }
    const int blocks = cg_blocks(o);
    const double alpha = (o->pre ? o->rho : o->rr) / p_dot_q;
    hipLaunchKernelGGL(cg_update_kernel, dim3(blocks), dim3(kRedThreads), 0, st, phi, (const real*)o->p, (const real*)o->q, (real)alpha,
                       (real)(phi_dot_q / o->S), o->x, o->r, o->n, o->d_partial);
    double s2[2];
    if (int rc = cg_fetch(o, blocks, 2, s2, st)) return rc;
    o->iters++;
    const double rr_old = o->rr;
    o->rr = s2[0];
    o->phir = s2[1];
    o->dir_ready = false;
    if (o->rr != o->rr) o->reason = OFDFT_CG_CURVATURE;      // a NaN in the product: nothing more to gain from this solve
    else if (!(o->rr > o->rtol * o->rtol * o->bb)) o->reason = OFDFT_CG_CONVERGED;      // |r| <= rtol |b|
    else if (o->iters >= o->maxiter) o->reason = OFDFT_CG_MAXITER;
    else if (!o->pre)
        hipLaunchKernelGGL(cg_direction_kernel, dim3(blocks), dim3(256), 0, st, phi, (const real*)o->r, (real)(o->rr / rr_old),
                           (real)(s2[1] / o->S), o->p, o->n);
    *reason = o->reason;
    return OFDFT_OK;
}

int ofdft_cg_set_preconditioned(ofdft_cg* o, int on) {
    if (!o) return OFDFT_EINVAL;
    o->pre_next = on != 0;
    return OFDFT_OK;
}

int ofdft_cg_z(ofdft_cg* o, void** z_dev) {
    if (!o || !z_dev) return OFDFT_EINVAL;
    DeviceScope device_scope_(o->device);
    CG_TRY(o, device_scope_.err);
    if (int rc = cg_ensure_z(o)) return rc;
    *z_dev = o->z;
    return OFDFT_OK;
}

// preconditioned mode, between the update sweep of one step and the product of the next: with z = M^-1 r in place,
// rho = r.Pz = r.z - (phi.r)(phi.z) / S, beta = rho / rho_old (0 after ofdft_cg_start), p = Pz + beta p.  One synchronisation.
int ofdft_cg_direction(ofdft_cg* o, const void* phi_dev, double* info_host, int* reason, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!o || !phi_dev || !reason) return OFDFT_EINVAL;
    if (!o->started) return cfail(o, OFDFT_ESTATE, "ofdft_cg_direction: ofdft_cg_start has not been called");
    if (!o->pre) return cfail(o, OFDFT_ESTATE, "ofdft_cg_direction: the solve runs in plain mode (ofdft_cg_set_preconditioned before ofdft_cg_start)");
    if (o->reason != OFDFT_CG_RUNNING) return cfail(o, OFDFT_ESTATE, "ofdft_cg_direction: the solve has ended (ofdft_cg_status)");
    if (o->dir_ready) return cfail(o, OFDFT_ESTATE, "ofdft_cg_direction: the direction of this step is already formed (ofdft_cg_step)");
    DeviceScope device_scope_(o->device);
    CG_TRY(o, device_scope_.err);
    const real* phi = (const real*)phi_dev;
    const int blocks = cg_blocks(o);
    hipLaunchKernelGGL(cg_pre_dots_kernel, dim3(blocks), dim3(kRedThreads), 0, st, phi, (const real*)o->r, (const real*)o->z, o->n, o->d_partial);
    double s2[2];
    if (int rc = cg_fetch(o, blocks, 2, s2, st)) return rc;
    const double rho = s2[0] - o->phir * s2[1] / o->S;
    if (info_host) {
        info_host[0] = s2[0];
        info_host[1] = s2[1];
        info_host[2] = rho;
        info_host[3] = o->dir_first ? 0.0 : rho / o->rho;
    }
    if (!(rho > 0.0)) {                // M is positive definite: only a NaN or a vanished residual comes here; x stays
        *reason = o->reason = OFDFT_CG_CURVATURE;
        return OFDFT_OK;
    }
    const real s = (real)(s2[1] / o->S);
    if (o->dir_first)
        hipLaunchKernelGGL(cg_pre_direction_kernel<true>, dim3(blocks), dim3(kRedThreads), 0, st, phi, (const real*)o->z, (real)0.0, s, o->p, o->n);
    else
        hipLaunchKernelGGL(cg_pre_direction_kernel<false>, dim3(blocks), dim3(kRedThreads), 0, st, phi, (const real*)o->z, (real)(rho / o->rho), s,
                           o->p, o->n);
    CG_TRY(o, hipGetLastError());
    o->rho = rho;
    o->dir_first = false;
    o->dir_ready = true;
    *reason = o->reason;
    return OFDFT_OK;
}

// x of the solve, copied to the caller's array (the stream's order; no wait)
int ofdft_cg_solution(ofdft_cg* o, void* x_out_dev, void* stream) {
    if (!o || !x_out_dev) return OFDFT_EINVAL;
    if (!o->started) return cfail(o, OFDFT_ESTATE, "ofdft_cg_solution: ofdft_cg_start has not been called");
    DeviceScope device_scope_(o->device);
    CG_TRY(o, device_scope_.err);
    CG_TRY(o, hipMemcpyAsync(x_out_dev, o->x, sizeof(real) * (size_t)o->n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return OFDFT_OK;
}

int ofdft_cg_status(const ofdft_cg* o, int* iterations, int* reason, double* rel_residual) {
    if (!o) return OFDFT_EINVAL;
    if (iterations) *iterations = o->iters;
    if (reason) *reason = o->reason;
    if (rel_residual) *rel_residual = o->bb > 0.0 ? std::sqrt(o->rr / o->bb) : 0.0;
    return OFDFT_OK;
}

}  // extern "C"
