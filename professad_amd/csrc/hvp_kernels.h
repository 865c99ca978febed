// Kernels of the Hessian-vector product hv = d/d eps v[n + eps w] at eps = 0 (ofdft_hessian_vector and, in chi space,
// ofdft_hessian_vector_chi; fp64, gfx950): one head
// kernel that writes every real field to be transformed, one spectral kernel over all spectra of the call, one combine kernel
// that adds the pointwise terms, writes hv once and reduces the per-term w . hv_t.  The operator forms are those of DESIGN.md
// ("Hessian-vector products"); the reference obtains them by a second autograd pass (functional_tools.py:34-70).
#pragma once
#include "pointwise_kernels.h"

namespace ofdft {

constexpr int kHvpMaxSpectra = 7;      // w | sqrt n, d sqrt n | n^beta, n^(beta-1) w | n^alpha, n^(alpha-1) w
constexpr int kHvpScalars = 10;        // per-term sums of w hv_t, indexed by the term's bit position (ion_electron .. chachiyo_c)
enum { HVP_VW = 1, HVP_WT = 2, HVP_WT2 = 4, HVP_REUSE = 8 };

// ---- head: n, w -> the real fields of the active terms (with HVP_REUSE only those that depend on w)
struct HvpHeadArgs {
    static constexpr bool kChi = false;
    const real* n;
    const real* w;
    real* chi;  real* dchi;      // sqrt n, w / (2 sqrt n)
    real* pb;   real* pbw;       // n^beta, n^(beta - 1) w
    real* pa;   real* paw;       // n^alpha, n^(alpha - 1) w   (HVP_WT2: alpha != beta)
    long long npts;
    real al, be;
    unsigned flags;
};
struct HvpHeadPoint { real chi, dchi, pb, pbw, pa, paw; };
__device__ __forceinline__ HvpHeadPoint hvp_head_point(const HvpHeadArgs& a, real n, real w) {
    HvpHeadPoint p{};
    if (a.flags & HVP_VW) {
        p.chi = sqrt(n);
        p.dchi = w / (2.0 * p.chi);
    }
    if (a.flags & HVP_WT) {
        const real b1 = pow(n, a.be - 1.0);
        p.pb = b1 * n;
        p.pbw = b1 * w;
        if (a.flags & HVP_WT2) {
            const real a1 = pow(n, a.al - 1.0);
            p.pa = a1 * n;
            p.paw = a1 * w;
        }
    }
    return p;
}
// chi-space variant (ofdft_hessian_vector_chi): `n` holds phi and `w` the direction d; the density and its variation are formed
// on the fly, n = cs phi^2 and dn = 2 cs phi d - k n (k = 2 phi.d / phi.phi, so sum dn = 0), and dn is written once where a
// transform reads it as it stands (Hartree).  The n-space instantiation carries none of this.
struct HvpChiHeadArgs : HvpHeadArgs {
    static constexpr bool kChi = true;
    real cs, k;
    real* dn;                    // nullptr: no transform takes dn itself
};
__device__ __forceinline__ void hvp_chi_density(real cs, real k, real phi, real d, real& n, real& dn) {
    n = cs * phi * phi;
    dn = 2.0 * cs * phi * d - k * n;
}
template <class Args>
static __global__ void hvp_head_kernel(Args a) {
    const bool vw = a.flags & HVP_VW, wt = a.flags & HVP_WT, wt2 = a.flags & HVP_WT2, dens = !(a.flags & HVP_REUSE);
    const long long n2 = a.npts >> 1;
#define ST2(ptr, u, v) reinterpret_cast<cplx*>(ptr)[i] = mkc(u, v)
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (long long)gridDim.x * blockDim.x) {
        cplx n = reinterpret_cast<const cplx*>(a.n)[i], w = reinterpret_cast<const cplx*>(a.w)[i];
        if constexpr (Args::kChi) {
            const cplx phi = n, d = w;
            hvp_chi_density(a.cs, a.k, phi.x, d.x, n.x, w.x);
            hvp_chi_density(a.cs, a.k, phi.y, d.y, n.y, w.y);
            if (a.dn) ST2(a.dn, w.x, w.y);
        }
        const HvpHeadPoint p0 = hvp_head_point(a, n.x, w.x), p1 = hvp_head_point(a, n.y, w.y);
        if (vw) {
            if (dens) ST2(a.chi, p0.chi, p1.chi);
            ST2(a.dchi, p0.dchi, p1.dchi);
        }
        if (wt) {
            if (dens) ST2(a.pb, p0.pb, p1.pb);
            ST2(a.pbw, p0.pbw, p1.pbw);
        }
        if (wt2) {
            if (dens) ST2(a.pa, p0.pa, p1.pa);
            ST2(a.paw, p0.paw, p1.paw);
        }
    }
#undef ST2
    if ((a.npts & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const long long i = a.npts - 1;
        real n = a.n[i], w = a.w[i];
        if constexpr (Args::kChi) {
            hvp_chi_density(a.cs, a.k, a.n[i], a.w[i], n, w);
            if (a.dn) a.dn[i] = w;
        }
        const HvpHeadPoint p = hvp_head_point(a, n, w);
        if (vw) {
            if (dens) a.chi[i] = p.chi;
            a.dchi[i] = p.dchi;
        }
        if (wt) {
            if (dens) a.pb[i] = p.pb;
            a.pbw[i] = p.pbw;
        }
        if (wt2) {
            if (dens) a.pa[i] = p.pa;
            a.paw[i] = p.paw;
        }
    }
}

// ---- spectral: every spectrum of the call times its operator, in place; k, eta and the Lindhard kernel once per k-point
struct HvpSpecArgs {
    cplx* s[kHvpMaxSpectra];
    int op[kHvpMaxSpectra];      // SPEC_HARTREE: 4 pi / k^2 (0 at k = 0), SPEC_LAPLACE: -k^2, SPEC_LINDHARD: pref (1 / G^-1(eta) - 3 eta^2 - 1)
    int ns, lindhard;            // lindhard: some spectrum takes the kernel
    KGeom kg;
    real pref, inv2kf;           // term_scalars: wt_pref, wt_inv2kf
};
static __global__ void hvp_spec_kernel(HvpSpecArgs a) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.kg.g.total; i += (long long)gridDim.x * blockDim.x) {
        real kx, ky, kz, k2;
        kvec(a.kg, i, kx, ky, kz, k2);
        real f[3];
        f[SPEC_HARTREE] = (k2 != 0.0) ? 4.0 * kPiR / k2 : 0.0;                                    // functionals.py:67-70
        f[SPEC_LAPLACE] = -k2;                                                                    // functional_tools.py:227
        f[SPEC_LINDHARD] = a.lindhard ? a.pref * lindhard_shape((k2 != 0.0) ? sqrt(k2) * a.inv2kf : 0.0) : 0.0;   // functionals.py:637-638,648
#pragma unroll
        for (int j = 0; j < kHvpMaxSpectra; ++j) {
            if (j < a.ns) {
                const real fj = a.op[j] == SPEC_HARTREE ? f[SPEC_HARTREE] : (a.op[j] == SPEC_LAPLACE ? f[SPEC_LAPLACE] : f[SPEC_LINDHARD]);
                const cplx v = a.s[j][i];
                a.s[j][i] = mkc(v.x * fj, v.y * fj);
            }
        }
    }
}

// ---- local correlation: d^2 (n eps_c) / dn^2 = rs (rs eps'' - 2 eps') / (9 n), from the parametrisations of lda_point
__device__ __forceinline__ real hvp_corr_second(real n, unsigned mask) {
    const real rs = kCrs / cbrt(n);
    real d1 = 0.0, d2 = 0.0;         // eps', eps'' with respect to rs, summed over the flavours set
    if (mask & OFDFT_PZ_C) {          // functionals.py:1515-1521
        const real gm = -0.1423, b1 = 1.0529, b2 = 0.3334, A = 0.0311, C = 0.002, D = -0.0116;
        if (rs < 1.0) {
            const real lr = log(rs);
            d1 += A / rs + C * lr + C + D;
            d2 += -A / (rs * rs) + C / rs;
        } else {
            const real sr = sqrt(rs), den = 1.0 + b1 * sr + b2 * rs;
            const real dd = 0.5 * b1 / sr + b2, d2d = -0.25 * b1 / (rs * sr);
            d1 += -gm * dd / (den * den);
            d2 += -gm * d2d / (den * den) + 2.0 * gm * dd * dd / (den * den * den);
        }
    }
    if (mask & OFDFT_PW_C) {          // functionals.py:1524-1530
        const real A = 0.0310907, a1 = 0.2137, b1 = 7.5957, b2 = 3.5876, b3 = 1.6382, b4 = 0.49294;
        const real sr = sqrt(rs);
        const real z = 2.0 * A * (sr * (b1 + sr * (b2 + sr * (b3 + sr * b4))));
        const real dz = 2.0 * A * (0.5 * b1 / sr + b2 + 1.5 * b3 * sr + 2.0 * b4 * rs);
        const real d2z = 2.0 * A * (-0.25 * b1 / (rs * sr) + 0.75 * b3 / sr + 2.0 * b4);
        const real q = z * (z + 1.0);
        const real L = log(1.0 + 1.0 / z), dL = -dz / q, d2L = -d2z / q + dz * dz * (2.0 * z + 1.0) / (q * q);
        const real pre = 2.0 * A * (1.0 + a1 * rs);
        d1 += -2.0 * A * a1 * L - pre * dL;
        d2 += -4.0 * A * a1 * dL - pre * d2L;
    }
    if (mask & OFDFT_CHACHIYO_C) {    // functionals.py:1533-1537
        const real a = (kLn2 - 1.0) / (2.0 * kPiR * kPiR), b = 20.4562557;
        const real ir = 1.0 / rs, ir2 = ir * ir;
        const real arg = 1.0 + b * ir + b * ir2;
        const real da = -b * ir2 - 2.0 * b * ir2 * ir, d2a = 2.0 * b * ir2 * ir + 6.0 * b * ir2 * ir2;
        d1 += a * da / arg;
        d2 += a * (d2a / arg - da * da / (arg * arg));
    }
    return rs * (rs * d2 - 2.0 * d1) / (9.0 * n);
}

// ---- combine: n, w and the inverse-transformed fields -> hv, and the per-term sums of w hv_t
struct HvpCombineArgs {
    static constexpr bool kChi = false;
    const real* n;
    const real* w;
    const real* vh;                       // F^-1[4 pi w^ / k^2]
    const real* lap;  const real* dlap;   // lap sqrt n, lap (w / 2 sqrt n)
    const real* A;    const real* Cb;     // K * n^beta, K * (n^(beta-1) w)
    const real* B;    const real* Ca;     // K * n^alpha, K * (n^(alpha-1) w)      (two: alpha != beta)
    real* hv;
    long long npts;
    unsigned mask;
    int two;
    real al, be;
};
struct HvpPoint { real n, w, vh, lap, dlap, A, Cb, B, Ca; };
__device__ __forceinline__ real hvp_combine_point(const HvpCombineArgs& a, const HvpPoint& p, acc_t (&acc)[kHvpScalars]) {
    const real n = p.n, w = p.w;
    real hv = 0.0;
    if (a.mask & OFDFT_HARTREE) {
        acc[1] += w * p.vh;
        hv += p.vh;
    }
    const real n13 = cbrt(n);
    if (a.mask & OFDFT_TF) {                    // (10/9) c_TF n^(-1/3) w
        const real t = (10.0 / 9.0) * kCtf * w / n13;
        acc[2] += w * t;
        hv += t;
    }
    if (a.mask & OFDFT_VW) {                    // -1/2 [lap(d chi) / chi - lap(chi) d chi / chi^2]
        const real chi = sqrt(n), dchi = w / (2.0 * chi);
        const real t = -0.5 * (p.dlap - p.lap * dchi / chi) / chi;
        acc[3] += w * t;
        hv += t;
    }
    if (a.mask & OFDFT_WT_NL) {
        const real a2 = pow(n, a.al - 2.0), a1 = a2 * n;
        real t;
        if (a.two) {
            const real b2 = pow(n, a.be - 2.0), b1 = b2 * n;
            t = kCtf * (a.al * (a.al - 1.0) * a2 * w * p.A + a.al * a.be * a1 * p.Cb + a.be * (a.be - 1.0) * b2 * w * p.B +
                        a.al * a.be * b1 * p.Ca);
        } else {
            t = kCtf * 2.0 * a.al * ((a.al - 1.0) * a2 * w * p.A + a.al * a1 * p.Cb);
        }
        acc[4] += w * t;
        hv += t;
    }
    if (a.mask & OFDFT_LDA_X) {                 // (4/9) kCx n^(-2/3) w = -(1/3) (3/pi)^(1/3) n^(-2/3) w
        const real t = (4.0 / 9.0) * kCx * w / (n13 * n13);
        acc[6] += w * t;
        hv += t;
    }
    if (a.mask & OFDFT_PZ_C) {
        const real t = hvp_corr_second(n, OFDFT_PZ_C) * w;
        acc[7] += w * t;
        hv += t;
    }
    if (a.mask & OFDFT_PW_C) {
        const real t = hvp_corr_second(n, OFDFT_PW_C) * w;
        acc[8] += w * t;
        hv += t;
    }
    if (a.mask & OFDFT_CHACHIYO_C) {
        const real t = hvp_corr_second(n, OFDFT_CHACHIYO_C) * w;
        acc[9] += w * t;
        hv += t;
    }
    return hv;
}
// chi-space variant: `n` holds phi, `w` the direction d, `hv` the output; per point dv = hv(n, dn) as above, then
//   P_j = -k g_j + d_j g_j / phi_j + c2 phi_j dv_j        (c2 = 2 cs dV; the quotient counts as 0 where phi_j = 0)
// is written, and sum dv n, g.d, d.P, phi.P are reduced (kHvpChiScalars, in this order): the constant d mu that still has to
// come off dv is known only after this sum (hvp_chi_shift_kernel).  g = nullptr stands for a gradient of zeros.
constexpr int kHvpChiScalars = 4;
struct HvpChiCombineArgs : HvpCombineArgs {
    static constexpr bool kChi = true;
    const real* g;
    real cs, k, c2;
};
__device__ __forceinline__ real hvp_chi_point(const HvpChiCombineArgs& a, real phi, real d, real g, real n, real dv,
                                              acc_t (&acc)[kHvpChiScalars]) {
    const real P = (phi != 0.0 ? d * g / phi : 0.0) - a.k * g + a.c2 * phi * dv;
    acc[0] += dv * n;
    acc[1] += g * d;
    acc[2] += d * P;
    acc[3] += phi * P;
    return P;
}
// (every array pointer is valid: the host points the fields of absent terms at `n`, as for combine_kernel)
template <class Args>
static __global__ __launch_bounds__(kRedThreads) void hvp_combine_kernel(Args a, acc_t* __restrict__ partial) {
    acc_t acc[kHvpScalars];
#pragma unroll
    for (int s = 0; s < kHvpScalars; ++s) acc[s] = 0.0;
    acc_t cacc[kHvpChiScalars] = {0.0, 0.0, 0.0, 0.0};
    (void)cacc;
    const long long n2 = a.npts >> 1;
#define LD2(ptr) reinterpret_cast<const cplx*>(ptr)[i]
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (long long)gridDim.x * blockDim.x) {
        cplx n = LD2(a.n), w = LD2(a.w);
        const cplx vh = LD2(a.vh), lp = LD2(a.lap), dl = LD2(a.dlap), A = LD2(a.A), Cb = LD2(a.Cb), B = LD2(a.B), Ca = LD2(a.Ca);
        if constexpr (Args::kChi) {
            const cplx phi = n, d = w, g = a.g ? LD2(a.g) : mkc(0.0, 0.0);
            hvp_chi_density(a.cs, a.k, phi.x, d.x, n.x, w.x);
            hvp_chi_density(a.cs, a.k, phi.y, d.y, n.y, w.y);
            const real v0 = hvp_combine_point(a, HvpPoint{n.x, w.x, vh.x, lp.x, dl.x, A.x, Cb.x, B.x, Ca.x}, acc);
            const real v1 = hvp_combine_point(a, HvpPoint{n.y, w.y, vh.y, lp.y, dl.y, A.y, Cb.y, B.y, Ca.y}, acc);
            const real h0 = hvp_chi_point(a, phi.x, d.x, g.x, n.x, v0, cacc);
            const real h1 = hvp_chi_point(a, phi.y, d.y, g.y, n.y, v1, cacc);
            reinterpret_cast<cplx*>(a.hv)[i] = mkc(h0, h1);
        } else {
            const real h0 = hvp_combine_point(a, HvpPoint{n.x, w.x, vh.x, lp.x, dl.x, A.x, Cb.x, B.x, Ca.x}, acc);
            const real h1 = hvp_combine_point(a, HvpPoint{n.y, w.y, vh.y, lp.y, dl.y, A.y, Cb.y, B.y, Ca.y}, acc);
            reinterpret_cast<cplx*>(a.hv)[i] = mkc(h0, h1);
        }
    }
#undef LD2
    if ((a.npts & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const long long i = a.npts - 1;
        if constexpr (Args::kChi) {
            real n, w;
            hvp_chi_density(a.cs, a.k, a.n[i], a.w[i], n, w);
            const real dv = hvp_combine_point(a, HvpPoint{n, w, a.vh[i], a.lap[i], a.dlap[i], a.A[i], a.Cb[i], a.B[i], a.Ca[i]}, acc);
            a.hv[i] = hvp_chi_point(a, a.n[i], a.w[i], a.g ? a.g[i] : (real)0.0, n, dv, cacc);
        } else {
            a.hv[i] = hvp_combine_point(a, HvpPoint{a.n[i], a.w[i], a.vh[i], a.lap[i], a.dlap[i], a.A[i], a.Cb[i], a.B[i], a.Ca[i]}, acc);
        }
    }
    if constexpr (Args::kChi) block_reduce_store<kHvpChiScalars>(cacc, partial);      // (the per-term sums are not kept: dead code here)
    else block_reduce_store<kHvpScalars>(acc, partial);
}

// ---- chi space, before the head: phi.d and phi.phi (fixed order, as every reduction here)
static __global__ __launch_bounds__(kRedThreads) void hvp_chi_dots_kernel(const real* __restrict__ phi, const real* __restrict__ d,
                                                                          long long npts, acc_t* __restrict__ partial) {
    acc_t acc[2] = {0.0, 0.0};
    const long long n2 = npts >> 1;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (long long)gridDim.x * blockDim.x) {
        const cplx p = reinterpret_cast<const cplx*>(phi)[i], q = reinterpret_cast<const cplx*>(d)[i];
        acc[0] += p.x * q.x + p.y * q.y;
        acc[1] += p.x * p.x + p.y * p.y;
    }
    if ((npts & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        acc[0] += phi[npts - 1] * d[npts - 1];
        acc[1] += phi[npts - 1] * phi[npts - 1];
    }
    block_reduce_store<2>(acc, partial);
}

// ---- chi space, after the combine: out_j -= c2 phi_j d mu with d mu = (sums[0] dV + sums[1]) / N from the reduced sums of
// the combine kernel (on the device: the call does not wait for the host in between)
static __global__ void hvp_chi_shift_kernel(const real* __restrict__ phi, real* __restrict__ out, long long npts,
                                            const acc_t* __restrict__ sums, real dV, real inv_nel, real c2) {
    const real s = c2 * ((sums[0] * dV + sums[1]) * inv_nel);
    const long long n2 = npts >> 1;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (long long)gridDim.x * blockDim.x) {
        const cplx p = reinterpret_cast<const cplx*>(phi)[i];
        cplx o = reinterpret_cast<cplx*>(out)[i];
        o.x -= s * p.x;
        o.y -= s * p.y;
        reinterpret_cast<cplx*>(out)[i] = o;
    }
    if ((npts & 1) && blockIdx.x == 0 && threadIdx.x == 0) out[npts - 1] -= s * phi[npts - 1];
}

}  // namespace ofdft
