// Per-term stress tensors sigma_ij = (1/Omega) dE/d eps_ij at fixed electron number (density ~ 1/volume): what the
// reference's get_stress (functional_tools.py:73-101) / System.__compute_stress (system.py:925-935) return by autograd.
// Closed forms: Hartree, TF, WT, LDA, PBE as in the reference's analytic test forms (tests/tools_for_tests.py:212-307,
// 367-472); vW, WGC99 and ion-electron in the exact discrete forms derived in oracle/stress.py.  Every kernel is a
// reduction to 7 numbers (xx, yy, zz, xy, xz, yz, + an energy-like scalar) over the half spectrum, or to 19 over the grid.
#pragma once
#include "ion_kernels.h"

namespace ofdft {

constexpr int kStressSpecScalars = 7;
constexpr int kStressRealScalars = 28;

enum { STRESS_HARTREE = 0, STRESS_VW = 1, STRESS_WT = 2, STRESS_HESS = 3 };

// a, b: UNNORMALISED spectra (b only for WT); scale = 1/N^2.
//   HARTREE: acc_ij += w 4 pi |n~|^2 k_i k_j / k^4,              acc[6] += w 4 pi |n~|^2 / k^2        (tools_for_tests.py:212-238)
//   VW:      acc_ij += -w |s~|^2 k_i k_j                                                              (oracle/stress.py)
//   WT:      acc_ij += w Re(a~ b~*) aux3(eta) (k_i k_j / k^2 - delta_ij / 3),  acc[6] += w Re(a~ b~*) shape(eta)   (:262-307)
//   HESS:    acc_ij += w Re(a~ b~*) k_i k_j     = -N^2 mean(b F^-1[-k_i k_j a~])    (Hessian term of a Laplacian-dependent GGA)
template <int OP>
__global__ __launch_bounds__(kRedThreads) void stress_spec_kernel(const cplx* __restrict__ a, const cplx* __restrict__ b,
                                                                  KGeom kg, double scale, double inv2kf,
                                                                  double* __restrict__ partial) {
    double acc[kStressSpecScalars] = {0, 0, 0, 0, 0, 0, 0};
    for_each_kpoint(kg, [&](const KPoint& p) {
        if (p.k2 == 0.0) return;
        const double w = half_weight(kg.g, p.z) * scale;
        const cplx av = a[p.i];
        if (OP == STRESS_HARTREE) {
            const double f = w * 4.0 * kPi * (av.x * av.x + av.y * av.y) / (p.k2 * p.k2);
            add_k2(acc, f, p.kx, p.ky, p.kz);
            acc[6] += f * p.k2;
        } else if (OP == STRESS_VW) {
            add_k2(acc, -w * (av.x * av.x + av.y * av.y), p.kx, p.ky, p.kz);
        } else if (OP == STRESS_HESS) {
            const cplx bv = b[p.i];
            add_k2(acc, w * (av.x * bv.x + av.y * bv.y), p.kx, p.ky, p.kz);
        } else {
            const cplx bv = b[p.i];
            const double re = w * (av.x * bv.x + av.y * bv.y);
            const double eta = sqrt(p.k2) * inv2kf;
            const double lg = log(fabs((1.0 + eta) / (1.0 - eta)));
            const double lind = 0.5 + (1.0 - eta * eta) / (4.0 * eta) * lg;
            const double aux3 = eta / (lind * lind) * (0.5 / eta - 0.25 * (1.0 + 1.0 / (eta * eta)) * lg) + 6.0 * eta * eta;
            const double f = re * aux3 / p.k2;
            add_k2(acc, f, p.kx, p.ky, p.kz);
            const double third = re * aux3 / 3.0;
            acc[0] -= third;
            acc[1] -= third;
            acc[2] -= third;
            acc[6] += re * lindhard_shape(eta);
        }
    });
    block_reduce_store<kStressSpecScalars>(acc, partial);
}

// Tabulated-kernel nonlocal term (OFDFT_NLK), kinds KGAP and XWM.  Derived as oracle/stress.py documents the Wang-Teter and WGC99
// forms.  With unnormalised spectra a~, b~ of the powers n^(e_a), n^(e_b), one pair term is
//     T = vol / N^2  sum_k w K(k; vol) Re(a~ b~*),
// and under a homogeneous strain eps at fixed N_e the grid values scale as n -> n / J, the wave vectors as
// d ln|k| / d eps_ij = -k_i k_j / k^2, and vol -> J vol.  Hence
//     (1 / vol) dT / d eps_ij = delta_ij (1 - e_a - e_b) T / vol
//                               + 1 / N^2 sum_k w Re(a~ b~*) [ dK/dln|k| (-k_i k_j / k^2) + dK/dln vol |_k delta_ij ].
// Every kernel here is K = c vol^q F(eta [, delta]) with eta = |k| / (2 k_F), k_F ~ vol^(-1/3) (n0 = round(N_e) / vol, and the
// un-rounded N_e / vol of XWM's eta, scale alike at fixed N_e) and, for KGAP, delta = 2 E_gap / k_F^2 ~ vol^(2/3):
//     dK/dln|k| = eta K_eta,     dK/dln vol |_k = q K + eta K_eta / 3 + (2/3) delta K_delta,
// and q = e_a + e_b - 5/3 for each pair (KGAP: c ~ n0^-(alpha+beta-5/3); XWM: kernel0, kernel1b ~ n0^(-2 kappa) with powers
// 2 kappa + 5/3, kernel1a ~ n0^(-1 - 2 kappa) with powers 2 kappa + 8/3), so the diagonal collects to -2/3 T / vol:
//     sigma_ij = sum_pairs 1 / N^2 sum_k w Re(a~ b~*) [ eta K_eta (delta_ij / 3 - k_i k_j / k^2) + (2/3) delta K_delta delta_ij ]
//                - (2/3) T / vol delta_ij.
// Closed forms: F = 1/G - 3 eta^2 - 1, F_eta = -G_eta / G^2 - 6 eta, F_delta = -G_delta / G^2, with G the gapped response
// (nlk_ginv_gap; its eta and delta derivatives below) or the Lindhard one, for which eta G_eta = D = 1/2 - (eta + 1/eta) lg / 4;
// XWM's kernel1 shape is H = D / G^2 + 6 eta^2 (= -eta F_eta), H_eta = D_eta / G^2 - 2 D^2 / (eta G^3) + 12 eta.
//   KGAP: K = c0 F(eta, delta) on Re(a~ b~*), a = n^alpha, b = n^beta
//   XWM:  K_AA = c0 F + c1 H on |A~|^2, K_AB = c2 H on Re(A~ B~*)  (c1 = -(n0 / p^2) k1, c2 = k1 / (p r): functionals.py:1478-1496)
// acc_ij: the bracket; acc[6]: sum_k w K Re(.) = T / vol.
struct NlkStress { int kind; double inv2kf, c0, c1, c2, delta; };
__device__ __forceinline__ void nlk_gap_derivs(double e, double d, double& G, double& Ge, double& Gd) {
    const double lg0 = log(fabs((1.0 + e) / (1.0 - e)));
    if (d == 0.0) {
        G = e == 1.0 ? 0.5 : 0.5 + (1.0 - e * e) / (4.0 * e) * lg0;
        Ge = 0.5 / e - 0.25 * (1.0 + 1.0 / (e * e)) * lg0;
        Gd = 0.0;
        return;
    }
    const double p = 4.0 * (e + e * e), m = 4.0 * (e - e * e), pp = 4.0 * (1.0 + 2.0 * e), mp = 4.0 * (1.0 - 2.0 * e), d2 = d * d;
    const double at = atan(p / d) + atan(m / d), dp = d2 + p * p, dm = d2 + m * m;
    const double Q = d2 / (128.0 * e * e * e) + 1.0 / (8.0 * e) - e / 8.0, L = log(dp / dm);
    const double Qe = -3.0 * d2 / (128.0 * e * e * e * e) - 1.0 / (8.0 * e * e) - 0.125, Le = 2.0 * p * pp / dp - 2.0 * m * mp / dm;
    G = 0.5 - d * at / (8.0 * e) + Q * L;
    Ge = -d * (d * pp / dp + d * mp / dm) / (8.0 * e) + d * at / (8.0 * e * e) + Qe * L + Q * Le;
    Gd = -(at - d * p / dp - d * m / dm) / (8.0 * e) + (2.0 * d / (128.0 * e * e * e)) * L + Q * (2.0 * d / dp - 2.0 * d / dm);
}
__global__ __launch_bounds__(kRedThreads) void stress_nlk_kernel(const cplx* __restrict__ a, const cplx* __restrict__ b, KGeom kg,
                                                                 double scale, NlkStress t, double* __restrict__ partial) {
    double acc[kStressSpecScalars] = {0, 0, 0, 0, 0, 0, 0};
    for_each_kpoint(kg, [&](const KPoint& p) {
        if (p.k2 == 0.0) return;
        const double w = half_weight(kg.g, p.z) * scale;
        const cplx av = a[p.i], bv = b[p.i];
        const double eta = sqrt(p.k2) * t.inv2kf;
        double G, Ge, Gd;
        nlk_gap_derivs(eta, t.kind == NLK_KGAP ? t.delta : 0.0, G, Ge, Gd);
        const double F = 1.0 / G - 3.0 * eta * eta - 1.0, Fe = -Ge / (G * G) - 6.0 * eta;
        double g, diag = 0.0, en;          // g = sum X eta K_eta, diag = sum X (2/3) delta K_delta, en = sum X K
        if (t.kind == NLK_KGAP) {
            const double X = w * (av.x * bv.x + av.y * bv.y);
            g = X * t.c0 * eta * Fe;
            diag = X * t.c0 * (2.0 / 3.0) * t.delta * (-Gd / (G * G));
            en = X * t.c0 * F;
        } else {
            const double Xaa = w * (av.x * av.x + av.y * av.y), Xab = w * (av.x * bv.x + av.y * bv.y);
            const double lg = log(fabs((1.0 + eta) / (1.0 - eta)));
            const double D = eta * Ge, De = -0.25 * (1.0 - 1.0 / (eta * eta)) * lg - 0.5 * (eta + 1.0 / eta) / (1.0 - eta * eta);
            const double H = D / (G * G) + 6.0 * eta * eta, He = De / (G * G) - 2.0 * D * D / (eta * G * G * G) + 12.0 * eta;
            g = eta * (Xaa * (t.c0 * Fe + t.c1 * He) + Xab * t.c2 * He);
            en = Xaa * (t.c0 * F + t.c1 * H) + Xab * t.c2 * H;
        }
        add_k2(acc, -g / p.k2, p.kx, p.ky, p.kz);
        acc[0] += g / 3.0 + diag;
        acc[1] += g / 3.0 + diag;
        acc[2] += g / 3.0 + diag;
        acc[6] += en;
    });
    block_reduce_store<kStressSpecScalars>(acc, partial);
}

// WGC99 nonlocal part (oracle/stress.py::wgc99_nl): spectra of A, B, C, P, Q, S (unnormalised), scale = 1/N^2
//   acc_ij += G (delta_ij / 3 - k_i k_j / k^2),  G = (w0' X0 + K1' X1 + K2' X2 + K3' X3) eta;   acc[6] += w0 X0 + K1 X1 + K2 X2 + K3 X3
struct WgcSpectra { const cplx* s[6]; };
__global__ __launch_bounds__(kRedThreads) void stress_wgc_kernel(WgcSpectra sp, KGeom kg, WgcSeries s, double scale,
                                                                 double* __restrict__ partial) {
    double acc[kStressSpecScalars] = {0, 0, 0, 0, 0, 0, 0};
    for_each_kpoint(kg, [&](const KPoint& p) {
        if (p.k2 == 0.0) return;
        const double w = half_weight(kg.g, p.z) * scale;
        const double eta = sqrt(p.k2) * s.inv2kf;
        double w0, w1, w2, w3;
        wgc_series<true>(eta, s, w0, w1, w2, w3);
        w0 *= s.pref;
        w1 *= s.pref;
        w2 *= s.pref;
        w3 *= s.pref;
        const double i6 = 1.0 / (6.0 * s.nref), i36 = 1.0 / (36.0 * s.nref * s.nref);
        const double K1 = -eta * w1 * i6;
        const double K2 = (eta * eta * w2 + (7.0 - s.gamma) * eta * w1) * i36;
        const double K3 = (eta * eta * w2 + (1.0 + s.gamma) * eta * w1) * i36;
        const double dK1 = -(w1 + eta * w2) * i6;
        const double common = 2.0 * eta * w2 + eta * eta * w3;
        const double dK2 = (common + (7.0 - s.gamma) * (w1 + eta * w2)) * i36;
        const double dK3 = (common + (1.0 + s.gamma) * (w1 + eta * w2)) * i36;
        const cplx A = sp.s[0][p.i], B = sp.s[1][p.i], C = sp.s[2][p.i], P = sp.s[3][p.i], Q = sp.s[4][p.i], S = sp.s[5][p.i];
        const double X0 = w * (P.x * A.x + P.y * A.y);
        const double X1 = w * (P.x * B.x + P.y * B.y + Q.x * A.x + Q.y * A.y);
        const double X2 = w * (P.x * C.x + P.y * C.y + S.x * A.x + S.y * A.y);
        const double X3 = w * (Q.x * B.x + Q.y * B.y);
        const double G = (w1 * X0 + dK1 * X1 + dK2 * X2 + dK3 * X3) * eta;
        add_k2(acc, -G / p.k2, p.kx, p.ky, p.kz);
        acc[0] += G / 3.0;
        acc[1] += G / 3.0;
        acc[2] += G / 3.0;
        acc[6] += w0 * X0 + K1 * X1 + K2 * X2 + K3 * X3;
    });
    block_reduce_store<kStressSpecScalars>(acc, partial);
}

// ion-electron: acc_ij += core v~'(k) k_i k_j / |k|,  acc[6] += core v~(k),  core = w Re(S_k conj(n^_k)) (oracle/stress.py)
// S exact (cart != nullptr) or PME (conj(b Q^)); nk unnormalised.
__global__ __launch_bounds__(kRedThreads) void stress_ion_kernel(const cplx* __restrict__ nk, const cplx* __restrict__ Qk,
                                                                 KGeom kg, const cplx* __restrict__ b0,
                                                                 const cplx* __restrict__ b1, const cplx* __restrict__ b2,
                                                                 const double* __restrict__ cart, int nion, RecpotTable tab,
                                                                 double* __restrict__ partial) {
    double acc[kStressSpecScalars] = {0, 0, 0, 0, 0, 0, 0};
    for_each_kpoint(kg, [&](const KPoint& p) {
        const cplx S = cart ? structure_factor(cart, nion, p.kx, p.ky, p.kz) : pme_structure_factor(b0, b1, b2, Qk, p);
        const cplx n = nk[p.i];
        const double core = half_weight(kg.g, p.z) * (S.x * n.x + S.y * n.y);
        const double kabs = (p.k2 != 0.0) ? sqrt(p.k2) : 0.0;
        const RecpotValue t = recpot<1>(tab, kabs);
        acc[6] += core * t.v;
        if (p.k2 != 0.0) add_k2(acc, core * t.dv / kabs, p.kx, p.ky, p.kz);
    });
    block_reduce_store<kStressSpecScalars>(acc, partial);
}

// real-space sums: [0] n^(5/3); [1] LDA-x (e - v n); [2] LDA-c (e - v n); PBE-x: [3..8] d_i n d_j n df/dg, [9] |grad n|^2 df/dg,
// [10] f - n df/dn; PBE-c: [11..16], [17], [18]; GGA kinetic (Pauli part): [19..24], [25], [26]
// (tools_for_tests.py:241-243, 367-472; the kinetic GGA has the same form, :46-118); [27] G tau_TF of vWGTF
__global__ __launch_bounds__(kRedThreads) void stress_real_kernel(const double* __restrict__ n, const double* __restrict__ gx,
                                                                  const double* __restrict__ gy, const double* __restrict__ gz,
                                                                  long long npts, unsigned mask, GgaSel sel,
                                                                  double gtf_inv_n0, int gtf_kind, double* __restrict__ partial,
                                                                  double* __restrict__ lapn = nullptr) {
    double acc[kStressRealScalars];
#pragma unroll
    for (int i = 0; i < kStressRealScalars; ++i) acc[i] = 0.0;
    const bool do_px = mask & OFDFT_PBE_X, do_pc = mask & OFDFT_PBE_C, do_pk = mask & OFDFT_GGA_K;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < npts; i += (long long)gridDim.x * blockDim.x) {
        const double d = n[i];
        if (mask & OFDFT_TF) acc[0] += cbrt(d * d) * d;
        if (mask & OFDFT_VWGTF) {
            double e, v;
            vwgtf_point(d, cbrt(d), 0.3 * cbrt(9.0 * kPi * kPi * kPi * kPi), gtf_inv_n0, gtf_kind, e, v);
            acc[27] += e;
        }
        if (mask & (OFDFT_LDA_X | OFDFT_PZ_C | OFDFT_PW_C | OFDFT_CHACHIYO_C)) {
            const XcLocal r = lda_point(d, mask);
            acc[1] += r.ex - r.vx * d;
            acc[2] += r.ec - r.vc * d;
        }
        if (do_px || do_pc || do_pk) {
            const double a = gx[i], b = gy[i], c = gz[i];
            const double g2 = a * a + b * b + c * c;
            for (int which = 0; which < 3; ++which) {
                if (which == 0 ? !do_px : (which == 1 ? !do_pc : !do_pk)) continue;
                const GgaSel one{which == 0, which == 1, which == 2, sel.kkind, sel.kmu, 0.0, 0.0, 0.0};
                PbePoint p = {0.0, 0.0, 0.0, 0.0, 0.0};
                double* o = acc + 3 + 8 * which;
                if (which == 2 && lapn) {
                    // f(n, g, l = lap n):  sigma_ij = delta_ij mean(f - n f_n - 2 g f_g - l f_l) - 2 mean(f_g d_i n d_j n)
                    //                                 - 2 mean(f_l d_i d_j n); the last term is reduced in k-space
                    //                                 (stress_spec_kernel<STRESS_HESS>) from the spectrum of f_l, left in lapn
                    GgaSel full = sel;
                    full.x = full.c = 0;
                    full.k = 1;
                    double dfdl;
                    const double l = lapn[i];
                    pg_laplacian_point(d, g2, l, full, p, dfdl);
                    o[7] -= l * dfdl;
                    lapn[i] = dfdl;
                } else {
                    p = pbe_point(d, g2, one);
                }
                o[0] += a * a * p.dfdg;
                o[1] += b * b * p.dfdg;
                o[2] += c * c * p.dfdg;
                o[3] += a * b * p.dfdg;
                o[4] += a * c * p.dfdg;
                o[5] += b * c * p.dfdg;
                o[6] += g2 * p.dfdg;
                o[7] += (which == 0 ? p.fx : (which == 1 ? p.fc : p.fk)) - d * p.dfdn;
            }
        }
    }
    block_reduce_store<kStressRealScalars>(acc, partial);
}

}  // namespace ofdft
