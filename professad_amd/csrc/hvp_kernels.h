// Kernels of the Hessian-vector product hv = d/d eps v[n + eps w] at eps = 0 (ofdft_hessian_vector and, in chi space,
// ofdft_hessian_vector_chi; fp64, gfx950): one head
// kernel that writes every real field to be transformed, one spectral kernel over all spectra of the call, one combine kernel
// that adds the pointwise terms, writes hv once and reduces the per-term w . hv_t.  The operator forms are those of DESIGN.md
// ("Hessian-vector products"); the reference obtains them by a second autograd pass (functional_tools.py:34-70).
#pragma once
#include "pointwise_kernels.h"

namespace ofdft {

constexpr int kHvpScalars = 12;        // per-term sums of w hv_t, indexed by the term's bit position (ion_electron .. pbe_c)
constexpr int kHvpCombineScalars = 10; // ... of which the combine kernel reduces ion_electron .. chachiyo_c; pbe_x, pbe_c: the GGA mid kernel
constexpr int kHvpGgaScalars = 2;
static_assert(kHvpCombineScalars + kHvpGgaScalars == kHvpScalars, "bits 10 and 11 follow the combine kernel's sums");
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
    real* nout;                  // nullptr: no transform takes n itself (the GGA gradient does; not written with HVP_REUSE)
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
            if (a.nout && dens) ST2(a.nout, n.x, n.y);
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
            if (a.nout && dens) a.nout[i] = n;
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
    const real* gpw;  const real* gdiv;   // GGA (kGga instantiations): the mid kernel's pointwise part, div flux
    const real* whv;                      // WGC99 without PBE (kWgc instantiations): the tail kernel's field (with PBE it is inside gpw)
};
struct HvpPoint { real n, w, vh, lap, dlap, A, Cb, B, Ca; };
__device__ __forceinline__ real hvp_combine_point(const HvpCombineArgs& a, const HvpPoint& p, acc_t (&acc)[kHvpCombineScalars], real hv0 = 0.0) {
    const real n = p.n, w = p.w;
    real hv = hv0;                               // PBE: f_nn w + f_nsigma dsigma - 2 div flux; WGC99: the tail's field (their w hv_t come from those kernels)
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
// hv0, the start value of hv: kGga: gpw - 2 gdiv (the WGC99 tail has added its field to gpw where both run); kWgc: whv
template <class Args, bool kGga = false, bool kWgc = false>
static __global__ __launch_bounds__(kRedThreads) void hvp_combine_kernel(Args a, acc_t* __restrict__ partial) {
    acc_t acc[kHvpCombineScalars];
#pragma unroll
    for (int s = 0; s < kHvpCombineScalars; ++s) acc[s] = 0.0;
    acc_t cacc[kHvpChiScalars] = {0.0, 0.0, 0.0, 0.0};
    (void)cacc;
    const long long n2 = a.npts >> 1;
#define LD2(ptr) reinterpret_cast<const cplx*>(ptr)[i]
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (long long)gridDim.x * blockDim.x) {
        cplx n = LD2(a.n), w = LD2(a.w);
        const cplx vh = LD2(a.vh), lp = LD2(a.lap), dl = LD2(a.dlap), A = LD2(a.A), Cb = LD2(a.Cb), B = LD2(a.B), Ca = LD2(a.Ca);
        cplx g0 = mkc(0.0, 0.0);
        if constexpr (kGga) {
            const cplx pw = LD2(a.gpw), dv = LD2(a.gdiv);
            g0 = mkc(pw.x - 2.0 * dv.x, pw.y - 2.0 * dv.y);
        } else if constexpr (kWgc) {
            g0 = LD2(a.whv);
        }
        if constexpr (Args::kChi) {
            const cplx phi = n, d = w, g = a.g ? LD2(a.g) : mkc(0.0, 0.0);
            hvp_chi_density(a.cs, a.k, phi.x, d.x, n.x, w.x);
            hvp_chi_density(a.cs, a.k, phi.y, d.y, n.y, w.y);
            const real v0 = hvp_combine_point(a, HvpPoint{n.x, w.x, vh.x, lp.x, dl.x, A.x, Cb.x, B.x, Ca.x}, acc, g0.x);
            const real v1 = hvp_combine_point(a, HvpPoint{n.y, w.y, vh.y, lp.y, dl.y, A.y, Cb.y, B.y, Ca.y}, acc, g0.y);
            const real h0 = hvp_chi_point(a, phi.x, d.x, g.x, n.x, v0, cacc);
            const real h1 = hvp_chi_point(a, phi.y, d.y, g.y, n.y, v1, cacc);
            reinterpret_cast<cplx*>(a.hv)[i] = mkc(h0, h1);
        } else {
            const real h0 = hvp_combine_point(a, HvpPoint{n.x, w.x, vh.x, lp.x, dl.x, A.x, Cb.x, B.x, Ca.x}, acc, g0.x);
            const real h1 = hvp_combine_point(a, HvpPoint{n.y, w.y, vh.y, lp.y, dl.y, A.y, Cb.y, B.y, Ca.y}, acc, g0.y);
            reinterpret_cast<cplx*>(a.hv)[i] = mkc(h0, h1);
        }
    }
#undef LD2
    if ((a.npts & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const long long i = a.npts - 1;
        real g0 = 0.0;
        if constexpr (kGga) g0 = a.gpw[i] - 2.0 * a.gdiv[i];
        else if constexpr (kWgc) g0 = a.whv[i];
        if constexpr (Args::kChi) {
            real n, w;
            hvp_chi_density(a.cs, a.k, a.n[i], a.w[i], n, w);
            const real dv = hvp_combine_point(a, HvpPoint{n, w, a.vh[i], a.lap[i], a.dlap[i], a.A[i], a.Cb[i], a.B[i], a.Ca[i]}, acc, g0);
            a.hv[i] = hvp_chi_point(a, a.n[i], a.w[i], a.g ? a.g[i] : (real)0.0, n, dv, cacc);
        } else {
            a.hv[i] = hvp_combine_point(a, HvpPoint{a.n[i], a.w[i], a.vh[i], a.lap[i], a.dlap[i], a.A[i], a.Cb[i], a.B[i], a.Ca[i]}, acc, g0);
        }
    }
    if constexpr (Args::kChi) block_reduce_store<kHvpChiScalars>(cacc, partial);      // (the per-term sums are not kept: dead code here)
    else block_reduce_store<kHvpCombineScalars>(acc, partial);
}

// ---- GGA mid stage (PBE exchange / correlation): between the two transform stages of a product with pbe_x or pbe_c.
// With sigma = |grad n|^2, dsigma = 2 grad n . grad w and the second partials of f(n, sigma) summed over the terms set,
//   c = f_sn w + f_ss dsigma,     flux = c grad n + f_s grad w   (over grad w, in place),     pw = f_nn w + f_ns dsigma,
// and per term  q_t = sum f_nn w^2 + 2 f_ns w dsigma + f_ss dsigma^2 + 2 f_s |grad w|^2  (= sum w hv_t by D_a^T = -D_a; slots 0: x, 1: c).
// The chi-space instantiation forms n and w = dn from (phi, d) on the fly, as head and combine do, and reduces nothing.
struct HvpGgaMidArgs {
    static constexpr bool kChi = false;
    const real* n;
    const real* w;
    const real* gn[3];          // grad n ("hv:gn0..2": density-only, retained)
    real* gw[3];                // grad w in, flux out
    real* pw;
    long long npts;
    int x, c;                   // pbe_x, pbe_c set
};
struct HvpChiGgaMidArgs : HvpGgaMidArgs {
    static constexpr bool kChi = true;
    real cs, k;
};
struct HvpGgaPoint { real pw, f0, f1, f2; };
__device__ __forceinline__ HvpGgaPoint hvp_gga_point(const HvpGgaMidArgs& a, real n, real w, real a0, real a1, real a2, real b0, real b1, real b2,
                                                     acc_t (&acc)[kHvpGgaScalars]) {
    const real sigma = a0 * a0 + a1 * a1 + a2 * a2, ds = 2.0 * (a0 * b0 + a1 * b1 + a2 * b2), gw2 = b0 * b0 + b1 * b1 + b2 * b2;
    PbeSecond x, c;
    pbe_second(n, sigma, a.x != 0, a.c != 0, x, c);
    acc[0] += x.fnn * w * w + 2.0 * x.fns * w * ds + x.fss * ds * ds + 2.0 * x.fs * gw2;
    acc[1] += c.fnn * w * w + 2.0 * c.fns * w * ds + c.fss * ds * ds + 2.0 * c.fs * gw2;
    const real fs = x.fs + c.fs, fnn = x.fnn + c.fnn, fns = x.fns + c.fns, fss = x.fss + c.fss;
    const real cc = fns * w + fss * ds;
    return HvpGgaPoint{fnn * w + fns * ds, cc * a0 + fs * b0, cc * a1 + fs * b1, cc * a2 + fs * b2};
}
template <class Args>
static __global__ __launch_bounds__(kRedThreads) void hvp_gga_mid_kernel(Args a, acc_t* __restrict__ partial) {
    acc_t acc[kHvpGgaScalars] = {0.0, 0.0};
    const long long n2 = a.npts >> 1;
#define LD2(ptr) reinterpret_cast<const cplx*>(ptr)[i]
#define ST2(ptr, u, v) reinterpret_cast<cplx*>(ptr)[i] = mkc(u, v)
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (long long)gridDim.x * blockDim.x) {
        cplx n = LD2(a.n), w = LD2(a.w);
        const cplx a0 = LD2(a.gn[0]), a1 = LD2(a.gn[1]), a2 = LD2(a.gn[2]), b0 = LD2(a.gw[0]), b1 = LD2(a.gw[1]), b2 = LD2(a.gw[2]);
        if constexpr (Args::kChi) {
            const cplx phi = n, d = w;
            hvp_chi_density(a.cs, a.k, phi.x, d.x, n.x, w.x);
            hvp_chi_density(a.cs, a.k, phi.y, d.y, n.y, w.y);
        }
        const HvpGgaPoint p0 = hvp_gga_point(a, n.x, w.x, a0.x, a1.x, a2.x, b0.x, b1.x, b2.x, acc);
        const HvpGgaPoint p1 = hvp_gga_point(a, n.y, w.y, a0.y, a1.y, a2.y, b0.y, b1.y, b2.y, acc);
        ST2(a.pw, p0.pw, p1.pw);
        ST2(a.gw[0], p0.f0, p1.f0);
        ST2(a.gw[1], p0.f1, p1.f1);
        ST2(a.gw[2], p0.f2, p1.f2);
    }
#undef LD2
#undef ST2
    if ((a.npts & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const long long i = a.npts - 1;
        real n = a.n[i], w = a.w[i];
        if constexpr (Args::kChi) hvp_chi_density(a.cs, a.k, a.n[i], a.w[i], n, w);
        const HvpGgaPoint p = hvp_gga_point(a, n, w, a.gn[0][i], a.gn[1][i], a.gn[2][i], a.gw[0][i], a.gw[1][i], a.gw[2][i], acc);
        a.pw[i] = p.pw;
        a.gw[0][i] = p.f0;
        a.gw[1][i] = p.f1;
        a.gw[2][i] = p.f2;
    }
    if constexpr (!Args::kChi) block_reduce_store<kHvpGgaScalars>(acc, partial);
}

// ---- WGC99 stage (OFDFT_OPT_HVP_WGC = 1).  n_ref is a constant of the differentiation (functionals.py:952-954 take
// round(N) with .item()), so the nonlocal energy is E = c dV sum p . (M a) with a fixed symmetric 3 x 3 block M of real convolution
// kernels (spec_wgc_mix_kernel) between pointwise functions of n: with theta = n - n_ref,
//   a = (A, A theta, A theta^2 / 2), A = n^beta;      p = (P, P theta, P theta^2 / 2), P = n^alpha;      U = M a,  G = M p,
//   hv = c sum_i [ p_i'' w U_i + p_i' (M (a' w))_i + a_i'' w G_i + a_i' (M (p' w))_i ]           (' = d/dn, d theta / dn = 1).
// The head writes a, p (density-only: not with HVP_REUSE) and a' w, p' w; the host runs each triple through M in place; the tail forms
// hv, adds it to `add` (the PBE stage's pointwise field) where given, and reduces sum w hv.  Both kernels take the chi-space pair
// (phi, d) as head and combine do, forming n and w = dn on the fly; the chi-space tail reduces nothing.
constexpr int kHvpWgcScalars = 1;
struct HvpWgcArgs {
    static constexpr bool kChi = false;
    const real* n;
    const real* w;
    real* a[3];   real* p[3];    // head: a, p out;            tail: U, G in       ("hv:wU0..2", "hv:wG0..2": retained)
    real* da[3];  real* dp[3];   // head: a' w, p' w out;      tail: M (a' w), M (p' w) in
    const real* add;             // tail: nullptr or a field hv is added to (may be `out`)
    real* out;                   // tail: hv (may be da[0]: every thread reads its own elements before it writes them)
    long long npts;
    real al, be, nref;
    unsigned flags;              // HVP_REUSE
};
struct HvpChiWgcArgs : HvpWgcArgs {
    static constexpr bool kChi = true;
    real cs, k;
};
// (f, f theta, f theta^2 / 2) for f = n^e, with its first and second derivative in n; the power is the evaluation's (fm::pow_pos:
// bluestein.h bs_prep, zpass.h), 0 where n is not positive
struct WgcTriple { real v[3], d[3], dd[3]; };
__device__ __forceinline__ WgcTriple wgc_triple(real n, real th, real e) {
    const real f2 = n > 0.0 ? fm::pow_pos(n, e - (real)2.0) : (real)0.0;
    const real f1 = f2 * n, f = f1 * n, h = 0.5 * th * th;
    const real g1 = e * f1, g2 = e * (e - 1.0) * f2;
    WgcTriple t;
    t.v[0] = f;    t.v[1] = f * th;                  t.v[2] = f * h;
    t.d[0] = g1;   t.d[1] = g1 * th + f;             t.d[2] = g1 * h + f * th;
    t.dd[0] = g2;  t.dd[1] = g2 * th + 2.0 * g1;     t.dd[2] = g2 * h + 2.0 * g1 * th + f;
    return t;
}
template <class Args>
static __global__ void hvp_wgc_head_kernel(Args a) {
    const bool dens = !(a.flags & HVP_REUSE);
    const long long n2 = a.npts >> 1;
#define ST2(ptr, u, v) reinterpret_cast<cplx*>(ptr)[i] = mkc(u, v)
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (long long)gridDim.x * blockDim.x) {
        cplx n = reinterpret_cast<const cplx*>(a.n)[i], w = reinterpret_cast<const cplx*>(a.w)[i];
        if constexpr (Args::kChi) {
            const cplx phi = n, d = w;
            hvp_chi_density(a.cs, a.k, phi.x, d.x, n.x, w.x);
            hvp_chi_density(a.cs, a.k, phi.y, d.y, n.y, w.y);
        }
        const WgcTriple b0 = wgc_triple(n.x, n.x - a.nref, a.be), b1 = wgc_triple(n.y, n.y - a.nref, a.be);
        const WgcTriple p0 = wgc_triple(n.x, n.x - a.nref, a.al), p1 = wgc_triple(n.y, n.y - a.nref, a.al);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (dens) {
                ST2(a.a[j], b0.v[j], b1.v[j]);
                ST2(a.p[j], p0.v[j], p1.v[j]);
            }
            ST2(a.da[j], b0.d[j] * w.x, b1.d[j] * w.y);
            ST2(a.dp[j], p0.d[j] * w.x, p1.d[j] * w.y);
        }
    }
#undef ST2
    if ((a.npts & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const long long i = a.npts - 1;
        real n = a.n[i], w = a.w[i];
        if constexpr (Args::kChi) hvp_chi_density(a.cs, a.k, a.n[i], a.w[i], n, w);
        const WgcTriple b = wgc_triple(n, n - a.nref, a.be), p = wgc_triple(n, n - a.nref, a.al);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (dens) {
                a.a[j][i] = b.v[j];
                a.p[j][i] = p.v[j];
            }
            a.da[j][i] = b.d[j] * w;
            a.dp[j][i] = p.d[j] * w;
        }
    }
}
struct HvpWgcPoint { real U[3], G[3], Ma[3], Mp[3]; };
__device__ __forceinline__ real hvp_wgc_point(const HvpWgcArgs& a, real n, real w, const HvpWgcPoint& q, acc_t (&acc)[kHvpWgcScalars]) {
    const WgcTriple b = wgc_triple(n, n - a.nref, a.be), p = wgc_triple(n, n - a.nref, a.al);
    real s = 0.0, t = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        s += p.dd[j] * q.U[j] + b.dd[j] * q.G[j];
        t += p.d[j] * q.Ma[j] + b.d[j] * q.Mp[j];
    }
    const real hv = kCtf * (s * w + t);
    acc[0] += w * hv;
    return hv;
}
template <class Args>
static __global__ __launch_bounds__(kRedThreads) void hvp_wgc_tail_kernel(Args a, acc_t* __restrict__ partial) {
    acc_t acc[kHvpWgcScalars] = {0.0};
    const long long n2 = a.npts >> 1;
#define LD2(ptr) reinterpret_cast<const cplx*>(ptr)[i]
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (long long)gridDim.x * blockDim.x) {
        cplx n = LD2(a.n), w = LD2(a.w);
        if constexpr (Args::kChi) {
            const cplx phi = n, d = w;
            hvp_chi_density(a.cs, a.k, phi.x, d.x, n.x, w.x);
            hvp_chi_density(a.cs, a.k, phi.y, d.y, n.y, w.y);
        }
        HvpWgcPoint q0, q1;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const cplx U = LD2(a.a[j]), G = LD2(a.p[j]), Ma = LD2(a.da[j]), Mp = LD2(a.dp[j]);
            q0.U[j] = U.x;    q1.U[j] = U.y;
            q0.G[j] = G.x;    q1.G[j] = G.y;
            q0.Ma[j] = Ma.x;  q1.Ma[j] = Ma.y;
            q0.Mp[j] = Mp.x;  q1.Mp[j] = Mp.y;
        }
        const cplx h0 = a.add ? LD2(a.add) : mkc(0.0, 0.0);
        const real v0 = hvp_wgc_point(a, n.x, w.x, q0, acc), v1 = hvp_wgc_point(a, n.y, w.y, q1, acc);
        reinterpret_cast<cplx*>(a.out)[i] = mkc(h0.x + v0, h0.y + v1);
    }
#undef LD2
    if ((a.npts & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const long long i = a.npts - 1;
        real n = a.n[i], w = a.w[i];
        if constexpr (Args::kChi) hvp_chi_density(a.cs, a.k, a.n[i], a.w[i], n, w);
        HvpWgcPoint q;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            q.U[j] = a.a[j][i];
            q.G[j] = a.p[j][i];
            q.Ma[j] = a.da[j][i];
            q.Mp[j] = a.dp[j][i];
        }
        const real h0 = a.add ? a.add[i] : (real)0.0;
        a.out[i] = h0 + hvp_wgc_point(a, n, w, q, acc);
    }
    if constexpr (!Args::kChi) block_reduce_store<kHvpWgcScalars>(acc, partial);
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

// ================================================================================================================================
// Several directions per call (ofdft_hessian_vector_chi_multi): the chi-space product at a stationary point (g = 0)
// for NC <= kMultiMax directions d_j at once.  Same schedule, the column count a dimension: phi, the density-side fields and
// every density-only factor (n, its roots and powers, the second derivatives of the local terms) are read or formed once per
// point and serve all columns.  NC is a template parameter, so the per-column accumulators and pointers stay in registers.
constexpr int kMultiMax = 8;                                   // OFDFT_MULTI_MAX
constexpr int kHvpMultiScalars = 3;                            // per column: sum dv n, d.P, phi.P  (g.d = 0)
constexpr int kHvpMultiSpectra = 3 + 4 * kMultiMax;            // density-only spectra + four per column
static_assert(kHvpMultiScalars * kMultiMax <= kMaxScalars && kMultiMax + 1 <= kMaxScalars, "the multi sums use the context's partial buffers");

// pair i of an array of n reals (n2 = n / 2 pairs, then the odd last element alone with a zero partner).  A column of a caller's
// stack may start at an odd element (odd stride): such a base takes two scalar accesses per pair.
__device__ __forceinline__ bool hvm_pair_aligned(const real* p) { return (reinterpret_cast<unsigned long long>(p) & (2 * sizeof(real) - 1)) == 0; }
__device__ __forceinline__ cplx hvm_ld(const real* p, long long i, long long n2, long long n) {
    if (i >= n2) return mkc(p[n - 1], 0.0);
    if (hvm_pair_aligned(p)) return reinterpret_cast<const cplx*>(p)[i];
    return mkc(p[2 * i], p[2 * i + 1]);
}
__device__ __forceinline__ void hvm_st(real* p, long long i, long long n2, long long n, cplx v) {
    if (i >= n2) {
        p[n - 1] = v.x;
    } else if (hvm_pair_aligned(p)) {
        reinterpret_cast<cplx*>(p)[i] = v;
    } else {
        p[2 * i] = v.x;
        p[2 * i + 1] = v.y;
    }
}
#define HVM_FOR_PAIRS(n)                                                                                                  \
    const long long n2 = (n) >> 1;                                                                                       \
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n2 + ((n) & 1); i += (long long)gridDim.x * blockDim.x)

// ---- before the head: a_j = phi.d_j for every column and S = phi.phi (slot NC), the latter summed exactly as hvp_chi_dots_kernel
// sums it, so that either entry may reuse the other's density fields
template <int NC>
static __global__ __launch_bounds__(kRedThreads) void hvm_dots_kernel(const real* __restrict__ phi, const real* __restrict__ d, long long stride,
                                                                      long long npts, acc_t* __restrict__ partial) {
    acc_t acc[NC + 1];
#pragma unroll
    for (int s = 0; s <= NC; ++s) acc[s] = 0.0;
    const long long n2 = npts >> 1;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (long long)gridDim.x * blockDim.x) {
        const cplx p = hvm_ld(phi, i, n2, npts);
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const cplx q = hvm_ld(d + j * stride, i, n2, npts);
            acc[j] += p.x * q.x + p.y * q.y;
        }
        acc[NC] += p.x * p.x + p.y * p.y;
    }
    if ((npts & 1) && blockIdx.x == 0 && threadIdx.x == 0) {      // (the odd last element where hvp_chi_dots_kernel adds it)
#pragma unroll
        for (int j = 0; j < NC; ++j) acc[j] += phi[npts - 1] * d[j * stride + npts - 1];
        acc[NC] += phi[npts - 1] * phi[npts - 1];
    }
    block_reduce_store<NC + 1>(acc, partial);
}

// ---- head: phi once, the density-only fields once (not with HVP_REUSE), then dn_j, d chi_j, n^(beta-1) dn_j, n^(alpha-1) dn_j per column
struct HvmHeadArgs {
    const real* phi;
    const real* d;               // column j at d + j * stride
    long long stride, npts;
    real* chi;  real* pb;  real* pa;                                   // sqrt n, n^beta, n^alpha ("hv:lap", "hv:A", "hv:B")
    real* dn[kMultiMax];                                                // nullptr: no transform takes dn itself
    real* dchi[kMultiMax];  real* pbw[kMultiMax];  real* paw[kMultiMax];
    real k[kMultiMax];                                                  // 2 a_j / S
    real cs, al, be;
    unsigned flags;
};
template <int NC>
static __global__ void hvm_head_kernel(HvmHeadArgs a) {
    const bool vw = a.flags & HVP_VW, wt = a.flags & HVP_WT, wt2 = a.flags & HVP_WT2, dens = !(a.flags & HVP_REUSE);
    HVM_FOR_PAIRS(a.npts) {
        const cplx phi = hvm_ld(a.phi, i, n2, a.npts);
        const bool pair = i < n2;                       // the odd last element has no partner: its y lane is not formed
        const real n0 = a.cs * phi.x * phi.x, n1 = pair ? a.cs * phi.y * phi.y : (real)1.0;
        real c0 = 0.0, c1 = 0.0, b0 = 0.0, b1 = 0.0, a0 = 0.0, a1 = 0.0;
        if (vw) {
            c0 = sqrt(n0);
            c1 = sqrt(n1);
            if (dens) hvm_st(a.chi, i, n2, a.npts, mkc(c0, c1));
        }
        if (wt) {
            b0 = pow(n0, a.be - 1.0);
            b1 = pow(n1, a.be - 1.0);
            if (dens) hvm_st(a.pb, i, n2, a.npts, mkc(b0 * n0, b1 * n1));
        }
        if (wt2) {
            a0 = pow(n0, a.al - 1.0);
            a1 = pow(n1, a.al - 1.0);
            if (dens) hvm_st(a.pa, i, n2, a.npts, mkc(a0 * n0, a1 * n1));
        }
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const cplx d = hvm_ld(a.d + j * a.stride, i, n2, a.npts);
            const real w0 = 2.0 * a.cs * phi.x * d.x - a.k[j] * n0, w1 = pair ? 2.0 * a.cs * phi.y * d.y - a.k[j] * n1 : (real)0.0;
            if (a.dn[j]) hvm_st(a.dn[j], i, n2, a.npts, mkc(w0, w1));
            if (vw) hvm_st(a.dchi[j], i, n2, a.npts, mkc(w0 / (2.0 * c0), w1 / (2.0 * c1)));
            if (wt) hvm_st(a.pbw[j], i, n2, a.npts, mkc(b0 * w0, b1 * w1));
            if (wt2) hvm_st(a.paw[j], i, n2, a.npts, mkc(a0 * w0, a1 * w1));
        }
    }
}

// ---- spectral: every spectrum of the call (single-column products too: engine_hvp.inc.h, SpecStage) times its operator, in place;
// k, eta and the Lindhard kernel once per k-point
struct HvmSpecArgs {
    cplx* s[kHvpMultiSpectra];
    unsigned char op[kHvpMultiSpectra + 1];      // SPEC_HARTREE: 4 pi / k^2 (0 at k = 0), SPEC_LAPLACE: -k^2, SPEC_LINDHARD: pref (1 / G^-1(eta) - 3 eta^2 - 1)
    int ns, lindhard;                            // lindhard: some spectrum takes the kernel
    KGeom kg;
    real pref, inv2kf;                           // term_scalars: wt_pref, wt_inv2kf
};
static __global__ void hvm_spec_kernel(HvmSpecArgs a) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.kg.g.total; i += (long long)gridDim.x * blockDim.x) {
        real kx, ky, kz, k2;
        kvec(a.kg, i, kx, ky, kz, k2);
        const real fh = (k2 != 0.0) ? 4.0 * kPiR / k2 : 0.0;
        const real fl = -k2;
        const real fk = a.lindhard ? a.pref * lindhard_shape((k2 != 0.0) ? sqrt(k2) * a.inv2kf : 0.0) : 0.0;
        for (int j = 0; j < a.ns; ++j) {                  // (uniform index into the kernel arguments: scalar loads)
            const int o = a.op[j];
            const real fj = o == SPEC_HARTREE ? fh : (o == SPEC_LAPLACE ? fl : fk);
            cplx* s = a.s[j];
            const cplx v = s[i];
            s[i] = mkc(v.x * fj, v.y * fj);
        }
    }
}

// ---- combine: the density-only factors of a point once, then out_j = c2 phi dv_j and the three sums per column
struct HvmCombineArgs {
    const real* phi;
    const real* d;
    long long dstride;
    const real* lap;  const real* A;  const real* B;                   // density side, shared by the columns
    const real* vh[kMultiMax];  const real* dlap[kMultiMax];  const real* Cb[kMultiMax];  const real* Ca[kMultiMax];
    real* out;
    long long ostride, npts;
    real k[kMultiMax];
    unsigned mask;
    int two;
    real al, be, cs, c2;
};
// what a point contributes to every column: dv = vh + w g0 + v1 (dlap - w v2) + wb Cb + wa Ca   (w = dn_j)
struct HvmFactors { real n, g0, v1, v2, wb, wa; };
__device__ __forceinline__ HvmFactors hvm_factors(const HvmCombineArgs& a, real n, real lap, real A, real B) {
    HvmFactors f{};
    f.n = n;
    const real n13 = cbrt(n);
    if (a.mask & OFDFT_TF) f.g0 += (10.0 / 9.0) * kCtf / n13;
    if (a.mask & OFDFT_LDA_X) f.g0 += (4.0 / 9.0) * kCx / (n13 * n13);
    if (a.mask & (OFDFT_PZ_C | OFDFT_PW_C | OFDFT_CHACHIYO_C)) f.g0 += hvp_corr_second(n, a.mask);      // (linear in the flavours set)
    if (a.mask & OFDFT_VW) {                       // -1/2 [lap(d chi) - lap(chi) w / (2 n)] / chi
        f.v1 = -0.5 / sqrt(n);
        f.v2 = lap / (2.0 * n);
    }
    if (a.mask & OFDFT_WT_NL) {
        const real a2 = pow(n, a.al - 2.0), a1 = a2 * n;
        if (a.two) {
            const real b2 = pow(n, a.be - 2.0), b1 = b2 * n;
            f.g0 += kCtf * (a.al * (a.al - 1.0) * a2 * A + a.be * (a.be - 1.0) * b2 * B);
            f.wb = kCtf * a.al * a.be * a1;
            f.wa = kCtf * a.al * a.be * b1;
        } else {
            f.g0 += kCtf * 2.0 * a.al * (a.al - 1.0) * a2 * A;
            f.wb = kCtf * 2.0 * a.al * a.al * a1;
        }
    }
    return f;
}
__device__ __forceinline__ real hvm_point(const HvmCombineArgs& a, const HvmFactors& f, real phi, real d, real k, real vh, real dlap, real Cb,
                                          real Ca, acc_t* acc) {
    const real w = 2.0 * a.cs * phi * d - k * f.n;
    real dv = w * f.g0;
    if (a.mask & OFDFT_HARTREE) dv += vh;
    if (a.mask & OFDFT_VW) dv += f.v1 * (dlap - w * f.v2);
    if (a.mask & OFDFT_WT_NL) {
        dv += f.wb * Cb;
        if (a.two) dv += f.wa * Ca;
    }
    const real P = a.c2 * phi * dv;
    acc[0] += dv * f.n;
    acc[1] += d * P;
    acc[2] += phi * P;
    return P;
}
template <int NC>
static __global__ __launch_bounds__(kRedThreads) void hvm_combine_kernel(HvmCombineArgs a, acc_t* __restrict__ partial) {
    acc_t acc[kHvpMultiScalars * NC];
#pragma unroll
    for (int s = 0; s < kHvpMultiScalars * NC; ++s) acc[s] = 0.0;
    const bool has_h = a.mask & OFDFT_HARTREE, has_vw = a.mask & OFDFT_VW, has_wt = a.mask & OFDFT_WT_NL;
    const cplx zero = mkc(0.0, 0.0);
    HVM_FOR_PAIRS(a.npts) {
        const cplx phi = hvm_ld(a.phi, i, n2, a.npts);
        const bool pair = i < n2;
        const cplx lp = has_vw ? hvm_ld(a.lap, i, n2, a.npts) : zero, A = has_wt ? hvm_ld(a.A, i, n2, a.npts) : zero;
        const cplx B = (has_wt && a.two) ? hvm_ld(a.B, i, n2, a.npts) : zero;
        const HvmFactors f0 = hvm_factors(a, a.cs * phi.x * phi.x, lp.x, A.x, B.x);
        const HvmFactors f1 = hvm_factors(a, pair ? a.cs * phi.y * phi.y : (real)1.0, lp.y, A.y, B.y);
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const cplx d = hvm_ld(a.d + j * a.dstride, i, n2, a.npts);
            const cplx vh = has_h ? hvm_ld(a.vh[j], i, n2, a.npts) : zero, dl = has_vw ? hvm_ld(a.dlap[j], i, n2, a.npts) : zero;
            const cplx Cb = has_wt ? hvm_ld(a.Cb[j], i, n2, a.npts) : zero, Ca = (has_wt && a.two) ? hvm_ld(a.Ca[j], i, n2, a.npts) : zero;
            const real h0 = hvm_point(a, f0, phi.x, d.x, a.k[j], vh.x, dl.x, Cb.x, Ca.x, acc + kHvpMultiScalars * j);
            real h1 = 0.0;
            if (pair) h1 = hvm_point(a, f1, phi.y, d.y, a.k[j], vh.y, dl.y, Cb.y, Ca.y, acc + kHvpMultiScalars * j);
            hvm_st(a.out + j * a.ostride, i, n2, a.npts, mkc(h0, h1));
        }
    }
    block_reduce_store<kHvpMultiScalars * NC>(acc, partial);
}

// ---- after the combine: out_j -= c2 phi d mu_j with d mu_j = sums[3 j] dV / N from the reduced sums, phi read once for all columns
static __global__ void hvm_shift_kernel(const real* __restrict__ phi, real* __restrict__ out, long long ostride, int ncols, long long npts,
                                        const acc_t* __restrict__ sums, real dV, real inv_nel, real c2) {
    HVM_FOR_PAIRS(npts) {
        const cplx p = hvm_ld(phi, i, n2, npts);
        for (int j = 0; j < ncols; ++j) {
            const real s = c2 * ((sums[kHvpMultiScalars * j] * dV) * inv_nel);
            cplx o = hvm_ld(out + j * ostride, i, n2, npts);
            o.x -= s * p.x;
            o.y -= s * p.y;
            hvm_st(out + j * ostride, i, n2, npts, o);
        }
    }
}
#undef HVM_FOR_PAIRS

}  // namespace ofdft
