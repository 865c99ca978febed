// Conjugate gradients for the projected operator P H P x = b, P = I - phi phi^T / S (S = phi.phi), b perpendicular to phi: the
// linear solve behind truncated Newton and the ground-state density response (professad_amd/optimize.py).  The product
// q = H p is the caller's (ofdft_hessian_vector_chi, which also returns p.q and phi.q); per iteration the solver adds two
// sweeps over its own vectors:
//   update     x += alpha p;  r -= alpha (q - phi (phi.q) / S);  sums r.r and phi.r
//   direction  p = (r - phi (phi.r) / S) + beta p                (the projection is applied here, so p stays in the subspace)
// Preconditioned mode (opt-in): the direction is formed from z = M^-1 r, which the caller writes, by two sweeps in
// front of the product (sums r.z, phi.z; p = (z - phi (phi.z) / S) + beta p), and the update sweep is followed by none.
// Reductions as in lbfgs_kernels.h: fixed order, wavefront shuffles, no atomics -- bitwise reproducible.
#pragma once
#include "pointwise_kernels.h"

namespace ofdft {

// pairs of reals per step, the odd last element alone (i == n2)
#define CG_FOR_PAIRS(n)                                                                                                   \
    const long long n2 = (n) >> 1;                                                                                       \
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n2 + ((n) & 1); i += (long long)gridDim.x * blockDim.x)
__device__ __forceinline__ cplx cg_ld(const real* p, long long i, long long n2, long long n) {
    return i < n2 ? reinterpret_cast<const cplx*>(p)[i] : mkc(p[n - 1], 0.0);
}
__device__ __forceinline__ void cg_st(real* p, long long i, long long n2, long long n, cplx v) {
    if (i < n2) reinterpret_cast<cplx*>(p)[i] = v;
    else p[n - 1] = v.x;
}

// start, first sweep: b.b, phi.phi, phi.b
static __global__ __launch_bounds__(kRedThreads) void cg_start_dots_kernel(const real* __restrict__ phi, const real* __restrict__ b,
                                                                           long long n, acc_t* __restrict__ partial) {
    acc_t acc[3] = {0.0, 0.0, 0.0};
    CG_FOR_PAIRS(n) {
        const cplx f = cg_ld(phi, i, n2, n), v = cg_ld(b, i, n2, n);
        acc[0] += v.x * v.x + v.y * v.y;
        acc[1] += f.x * f.x + f.y * f.y;
        acc[2] += f.x * v.x + f.y * v.y;
    }
    block_reduce_store<3>(acc, partial);
}

// start, second sweep: x = 0, r = p = b - s phi (s = phi.b / S); sum r.r
static __global__ __launch_bounds__(kRedThreads) void cg_start_kernel(const real* __restrict__ phi, const real* __restrict__ b, real s,
                                                                      real* __restrict__ x, real* __restrict__ r, real* __restrict__ p,
                                                                      long long n, acc_t* __restrict__ partial) {
    acc_t acc[1] = {0.0};
    CG_FOR_PAIRS(n) {
        const cplx f = cg_ld(phi, i, n2, n), v = cg_ld(b, i, n2, n);
        const cplx ri = mkc(v.x - s * f.x, v.y - s * f.y);
        cg_st(x, i, n2, n, mkc(0.0, 0.0));
        cg_st(r, i, n2, n, ri);
        cg_st(p, i, n2, n, ri);
        acc[0] += ri.x * ri.x + ri.y * ri.y;
    }
    block_reduce_store<1>(acc, partial);
}

// update sweep (s = phi.q / S); sums r.r and phi.r of the new residual
static __global__ __launch_bounds__(kRedThreads) void cg_update_kernel(const real* __restrict__ phi, const real* __restrict__ p,
                                                                       const real* __restrict__ q, real alpha, real s, real* __restrict__ x,
                                                                       real* __restrict__ r, long long n, acc_t* __restrict__ partial) {
    acc_t acc[2] = {0.0, 0.0};
    CG_FOR_PAIRS(n) {
        const cplx f = cg_ld(phi, i, n2, n), pi = cg_ld(p, i, n2, n), qi = cg_ld(q, i, n2, n);
        cplx xi = cg_ld(x, i, n2, n), ri = cg_ld(r, i, n2, n);
        xi.x += alpha * pi.x;
        xi.y += alpha * pi.y;
        ri.x -= alpha * (qi.x - s * f.x);
        ri.y -= alpha * (qi.y - s * f.y);
        cg_st(x, i, n2, n, xi);
        cg_st(r, i, n2, n, ri);
        acc[0] += ri.x * ri.x + ri.y * ri.y;
        acc[1] += f.x * ri.x + f.y * ri.y;
    }
    block_reduce_store<2>(acc, partial);
}

// direction sweep (s = phi.r / S)
static __global__ __launch_bounds__(kRedThreads) void cg_direction_kernel(const real* __restrict__ phi, const real* __restrict__ r,
                                                                          real beta, real s, real* __restrict__ p, long long n) {
    CG_FOR_PAIRS(n) {
        const cplx f = cg_ld(phi, i, n2, n), ri = cg_ld(r, i, n2, n);
        cplx pi = cg_ld(p, i, n2, n);
        pi.x = (ri.x - s * f.x) + beta * pi.x;
        pi.y = (ri.y - s * f.y) + beta * pi.y;
        cg_st(p, i, n2, n, pi);
    }
}

// ---- preconditioned mode: the caller writes z = M^-1 r between the update sweep and these two
// sums r.z and phi.z
static __global__ __launch_bounds__(kRedThreads) void cg_pre_dots_kernel(const real* __restrict__ phi, const real* __restrict__ r,
                                                                         const real* __restrict__ z, long long n, acc_t* __restrict__ partial) {
    acc_t acc[2] = {0.0, 0.0};
    CG_FOR_PAIRS(n) {
        const cplx f = cg_ld(phi, i, n2, n), ri = cg_ld(r, i, n2, n), zi = cg_ld(z, i, n2, n);
        acc[0] += ri.x * zi.x + ri.y * zi.y;
        acc[1] += f.x * zi.x + f.y * zi.y;
    }
    block_reduce_store<2>(acc, partial);
}

// direction sweep (s = phi.z / S): p = (z - s phi) + beta p; FIRST: p = z - s phi (beta = 0, whatever p holds)
template <bool FIRST>
static __global__ __launch_bounds__(kRedThreads) void cg_pre_direction_kernel(const real* __restrict__ phi, const real* __restrict__ z,
                                                                              real beta, real s, real* __restrict__ p, long long n) {
    CG_FOR_PAIRS(n) {
        const cplx f = cg_ld(phi, i, n2, n), zi = cg_ld(z, i, n2, n);
        cplx pi = mkc(zi.x - s * f.x, zi.y - s * f.y);
        if (!FIRST) {
            const cplx po = cg_ld(p, i, n2, n);
            pi.x += beta * po.x;
            pi.y += beta * po.y;
        }
        cg_st(p, i, n2, n, pi);
    }
}
#undef CG_FOR_PAIRS

}  // namespace ofdft
