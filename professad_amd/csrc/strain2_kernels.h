// Second strain derivative of the energy at fixed grid values of chi: the fixed-chi part W2^0 of the elastic
// constants.  The strain is h -> h (I + eps) with a general (non-symmetric) eps; fractional ion coordinates, the grid values of
// chi and N are fixed, so n ~ 1/J, J = det(I + eps).  Reference: what torch.autograd.functional.hessian gives in eps through the
// closure of System.__compute_elastic_constants (src/professad/system.py:1266-1273).
//
// Reciprocal-space terms.  A wave vector moves as k -> (I + eps)^-1 k, so with s = |k|^2
//     ds / d eps_mn            = -2 k_m k_n
//     d2s / d eps_mn d eps_pq  =  2 (k_m k_q delta_np + k_p k_n delta_qm + k_n k_q delta_mp)
//     dJ / d eps_mn = delta_mn,     d2J / d eps_mn d eps_pq = delta_mn delta_pq - delta_mq delta_np
// and a term E = sum_k X_k f(s_k, J) (X_k: strain-invariant products of unnormalised spectra) has
//     W2[m,n,p,q] = sum_k X [ c4 k_m k_n k_p k_q + c2 (k_m k_q delta_np + k_p k_n delta_qm + k_n k_q delta_mp)
//                             + c2b (k_m k_n delta_pq + delta_mn k_p k_q) + c0a delta_mn delta_pq
//                             + c0b (delta_mn delta_pq - delta_mq delta_np) ]
//     c4 = 4 f_ss,  c2 = 2 f_s,  c2b = -2 f_sJ,  c0a = f_JJ,  c0b = f_J.
// The kernels reduce 15 + 6 + 2 sums: X c4 k k k k (sorted index quadruples), X c2 k k (xx, yy, zz, xy, xz, yz), X c0a, X c0b.
// The c2b moments need no sums of their own: for every term here c2b is c2 (Hartree, ion-electron), zero (vW) or -(s/3) c4
// (Wang-Teter: the trace of the quartic moments), which the host uses.
//   Hartree       f = 1 / (J s):                c4 = 8 / s^3, c2 = c2b = -2 / s^2, c0a = 2 / s, c0b = -1 / s
//   vW            f = s:                        c2 = 2
//   Wang-Teter    f = J^(-2/3) F(eta), eta = sqrt(s) J^(1/3) / (2 k_F):  with P = eta F', Q = eta^2 F''
//                 c4 = (Q - P) / s^2, c2 = P / s, c2b = -(Q - P) / (3 s), c0a = 10/9 F - 2/3 P + Q / 9, c0b = -2/3 F + P / 3
//   ion-electron  f = v~(sqrt s) / J:           c4 = v~'' / s - v~' / |k|^3, c2 = c2b = v~' / |k|, c0a = 2 v~, c0b = -v~
// Pair sum of the ion-ion energy: r^2 = d (I + eps)(I + eps)^T d^T, so with f(r) = Z_i Z_j erfc(r / Rd) / r
//     W2[m,n,p,q] = 1/2 sum_pairs [ (f'' - f'/r) d_m d_n d_p d_q / r^2 + (f'/r) d_m d_p delta_nq ].
// Every reduction: wavefront shuffles (block_reduce_store), fixed-order sum of the block partials on the host; no atomics.
#pragma once
#include "stress_kernels.h"

namespace ofdft {

constexpr int kStrain2Scalars = 23;      // 15 quartic + 6 quadratic + c0a + c0b
static_assert(kStrain2Scalars <= kMaxScalars, "a row of c->d_partial holds kMaxScalars doubles");

// F = 1/G - 3 eta^2 - 1 of the Lindhard response G (functionals.py:617-628,648) with P = eta F' and Q = eta^2 F''.
// eta >= 3: with z = eta^-2 and c_j = 1 / (4 j^2 - 1), G = z R, R = sum_{j>=0} c_(j+1) z^j, V = sum_{j>=0} c_(j+2) z^j, F = -3 u - 1,
// u = V / R (lindhard_shape's series); eta d/d eta = -2 z d/dz gives P = 6 z u', Q = -18 z u' - 12 z^2 u'': 18 terms (tail 9^-18),
// no cancellation -- the direct form cancels twice there, and its derivatives lose eta^4 times a rounding as F itself does.
// eta < 3: direct, with lg = log|(1 + eta) / (1 - eta)|, D = eta G' = 1/2 - (eta + 1/eta) lg / 4,
// D' = -(1 - 1/eta^2) lg / 4 - (eta + 1/eta) / (2 (1 - eta^2)):  P = -D / G^2 - 6 eta^2,  Q = -(eta D' - D) / G^2 + 2 D^2 / G^3 - 6 eta^2.
// eta == 1: the reference assigns G = 1/2 there as a constant (no derivative): P = Q = -6.
__device__ __forceinline__ void lindhard_shape_d2(double eta, double& F, double& P, double& Q) {
    if (eta >= 3.0) {
        const double z = 1.0 / (eta * eta);
        double r = 1.0 / (4.0 * 18 * 18 - 1.0), r1 = 0.0, r2 = 0.0, v = 1.0 / (4.0 * 19 * 19 - 1.0), v1 = 0.0, v2 = 0.0;
#pragma unroll
        for (int j = 17; j >= 1; --j) {       // Horner with the first derivative and half the second
            r2 = __builtin_fma(r2, z, r1);
            r1 = __builtin_fma(r1, z, r);
            r = __builtin_fma(r, z, 1.0 / (4.0 * j * j - 1.0));
            v2 = __builtin_fma(v2, z, v1);
            v1 = __builtin_fma(v1, z, v);
            v = __builtin_fma(v, z, 1.0 / (4.0 * (j + 1) * (j + 1) - 1.0));
        }
        r2 *= 2.0;
        v2 *= 2.0;
        const double ir = 1.0 / r;
        const double u1 = (v1 * r - v * r1) * ir * ir;
        const double u2 = (v2 * r - v * r2) * ir * ir - 2.0 * r1 * u1 * ir;
        F = -3.0 * v * ir - 1.0;
        P = 6.0 * z * u1;
        Q = -18.0 * z * u1 - 12.0 * z * z * u2;
        return;
    }
    const double e2 = eta * eta;
    if (eta == 1.0) {
        F = -2.0;
        P = Q = -6.0;
        return;
    }
    const double lg = log(fabs((1.0 + eta) / (1.0 - eta)));
    const double G = 0.5 + (1.0 - e2) / (4.0 * eta) * lg;
    const double D = 0.5 - 0.25 * (eta + 1.0 / eta) * lg;
    const double De = -0.25 * (1.0 - 1.0 / e2) * lg - 0.5 * (eta + 1.0 / eta) / (1.0 - e2);
    const double iG = 1.0 / G, iG2 = iG * iG;
    F = iG - 3.0 * e2 - 1.0;
    P = -D * iG2 - 6.0 * e2;
    Q = -(eta * De - D) * iG2 + 2.0 * D * D * iG2 * iG - 6.0 * e2;
}

enum { STRAIN2_HARTREE = 0, STRAIN2_VW = 1, STRAIN2_WT = 2 };

// a, b: UNNORMALISED spectra (b only for WT); scale = 1/N^2.  X = w 4 pi |n~|^2 (Hartree), w |s~|^2 (vW), w Re(a~ b~*) (WT).
template <int OP>
__global__ __launch_bounds__(kRedThreads) void strain2_spec_kernel(const cplx* __restrict__ a, const cplx* __restrict__ b, KGeom kg,
                                                                   double scale, double inv2kf, double* __restrict__ partial) {
    double acc[kStrain2Scalars];
#pragma unroll
    for (int s = 0; s < kStrain2Scalars; ++s) acc[s] = 0.0;
    for_each_kpoint(kg, [&](const KPoint& p) {
        if (p.k2 == 0.0) return;
        const double w = half_weight(kg.g, p.z) * scale;
        const cplx av = a[p.i];
        if (OP == STRAIN2_HARTREE) {
            const double is = 1.0 / p.k2, X = w * 4.0 * kPi * (av.x * av.x + av.y * av.y) * is;
            add_k4(acc, 8.0 * X * is * is, p.kx, p.ky, p.kz);
            add_k2(acc + 15, -2.0 * X * is, p.kx, p.ky, p.kz);
            acc[21] += 2.0 * X;
            acc[22] -= X;
        } else if (OP == STRAIN2_VW) {
            add_k2(acc + 15, 2.0 * w * (av.x * av.x + av.y * av.y), p.kx, p.ky, p.kz);
        } else {
            const cplx bv = b[p.i];
            const double X = w * (av.x * bv.x + av.y * bv.y), is = 1.0 / p.k2;
            double F, P, Q;
            lindhard_shape_d2(sqrt(p.k2) * inv2kf, F, P, Q);
            add_k4(acc, X * (Q - P) * is * is, p.kx, p.ky, p.kz);
            add_k2(acc + 15, X * P * is, p.kx, p.ky, p.kz);
            acc[21] += X * (10.0 / 9.0 * F - 2.0 / 3.0 * P + Q / 9.0);
            acc[22] += X * (-2.0 / 3.0 * F + P / 3.0);
        }
    });
    block_reduce_store<kStrain2Scalars>(acc, partial);
}

// ion-electron, exact structure factor: X = w Re(S_k conj(n^_k)), nk unnormalised; k = 0 contributes to c0a, c0b only
__global__ __launch_bounds__(kRedThreads) void strain2_ion_kernel(const cplx* __restrict__ nk, KGeom kg, const double* __restrict__ cart,
                                                                  int nion, RecpotTable tab, double* __restrict__ partial) {
    double acc[kStrain2Scalars];
#pragma unroll
    for (int s = 0; s < kStrain2Scalars; ++s) acc[s] = 0.0;
    for_each_kpoint(kg, [&](const KPoint& p) {
        const cplx S = structure_factor(cart, nion, p.kx, p.ky, p.kz), n = nk[p.i];
        const double X = half_weight(kg.g, p.z) * (S.x * n.x + S.y * n.y);
        const double kabs = (p.k2 != 0.0) ? sqrt(p.k2) : 0.0;
        const RecpotValue t = recpot<2>(tab, kabs);
        acc[21] += 2.0 * X * t.v;
        acc[22] -= X * t.v;
        if (p.k2 != 0.0) {
            const double ik = 1.0 / kabs;
            add_k4(acc, X * (t.d2v - t.dv * ik) / p.k2, p.kx, p.ky, p.kz);
            add_k2(acc + 15, X * t.dv * ik, p.kx, p.ky, p.kz);
        }
    });
    block_reduce_store<kStrain2Scalars>(acc, partial);
}

// ---- strain gradient of the potential: v_eps,kl = the explicit cell dependence of v = dE/dn at fixed grid values of n, with
// n0 = N / vol following the cell.  Six fields in the order xx, yy, zz, yz, xz, xy.  With unnormalised spectra and a 1/N inverse:
//   Hartree   F^-1[ (8 pi k_k k_l / s^2) n^ ]                                        (d(4 pi / s) = 8 pi k_k k_l / s^2)
//   vW        -F^-1[ k_k k_l chi^ ] / chi                                            (d(-s) = 2 k_k k_l in -1/2 F^-1[-s chi^] / chi)
//   wt_nl     c_TF [ alpha n^(alpha-1) F^-1[K'_kl F[n^beta]] + beta n^(beta-1) F^-1[K'_kl F[n^alpha]] ],
//             K'_kl = pref [ delta_kl ((alpha + beta - 5/3) F + P / 3) - P k_k k_l / s ]   (K = pref(n0) F(eta): d ln n0 = -delta_kl,
//             d ln eta = delta_kl / 3 - k_k k_l / s), K'(0) = 0
// The pointwise terms have no explicit part.  Three kernels around one batch of forward and one of inverse transforms.
constexpr int kStrainGradFamilies = 4;      // Hartree, vW, K' * n^beta, K' * n^alpha (the last only for alpha != beta)
enum { SG_HARTREE = 1, SG_VW = 2, SG_WT = 4, SG_WT2 = 8 };

// head: n -> sqrt n, n^beta [, n^alpha], n read once
static __global__ void strain_grad_head_kernel(const double* __restrict__ n, double* __restrict__ chi, double* __restrict__ pb,
                                               double* __restrict__ pa, long long npts, double al, double be, unsigned flags) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < npts; i += (long long)gridDim.x * blockDim.x) {
        const double d = n[i];
        if (flags & SG_VW) chi[i] = sqrt(d);
        if (flags & SG_WT) pb[i] = pow(d, be);
        if (flags & SG_WT2) pa[i] = pow(d, al);
    }
}

struct StrainGradSpecArgs {
    const cplx* in[kStrainGradFamilies];          // spectra of n, sqrt n, n^beta, n^alpha
    cplx* out[kStrainGradFamilies * 6];           // [family * 6 + component]
    KGeom kg;
    unsigned flags;
    double pref, inv2kf, q;                       // Lindhard prefactor, 1 / (2 k_F), alpha + beta - 5/3
};
// spectral: k, eta, F and P once per k-point; six spectra per active family
static __global__ void strain_grad_spec_kernel(StrainGradSpecArgs a) {
    for_each_kpoint(a.kg, [&](const KPoint& p) {
        const long long i = p.i;
        const double is = (p.k2 != 0.0) ? 1.0 / p.k2 : 0.0;
        const double kk[6] = {p.kx * p.kx, p.ky * p.ky, p.kz * p.kz, p.ky * p.kz, p.kx * p.kz, p.kx * p.ky};
        if (a.flags & SG_HARTREE) {
            const cplx v = a.in[0][i];
            const double f = 8.0 * kPi * is * is;
#pragma unroll
            for (int c = 0; c < 6; ++c) a.out[c][i] = make_double2(v.x * f * kk[c], v.y * f * kk[c]);
        }
        if (a.flags & SG_VW) {
            const cplx v = a.in[1][i];
#pragma unroll
            for (int c = 0; c < 6; ++c) a.out[6 + c][i] = make_double2(v.x * kk[c], v.y * kk[c]);
        }
        if (a.flags & SG_WT) {
            double F = 0.0, P = 0.0, Q = 0.0;
            if (p.k2 != 0.0) lindhard_shape_d2(sqrt(p.k2) * a.inv2kf, F, P, Q);      // (Q is unused here: inlined, its arithmetic is dead code)
            const double iso = (p.k2 != 0.0) ? a.pref * (a.q * F + P / 3.0) : 0.0, an = -a.pref * P * is;
            double f[6];
            voigt6(an, iso, p, f);
            const cplx v = a.in[2][i];
#pragma unroll
            for (int c = 0; c < 6; ++c) a.out[12 + c][i] = make_double2(v.x * f[c], v.y * f[c]);
            if (a.flags & SG_WT2) {
                const cplx u = a.in[3][i];
#pragma unroll
                for (int c = 0; c < 6; ++c) a.out[18 + c][i] = make_double2(u.x * f[c], u.y * f[c]);
            }
        }
    });
}

struct StrainGradCombineArgs {
    const double* n;
    const double* f[kStrainGradFamilies * 6];     // the inverse-transformed fields
    double* out;                                  // [6][npts]
    long long npts;
    unsigned flags;
    double al, be;
};
// combine: n and the fields once, the six outputs once
static __global__ void strain_grad_combine_kernel(StrainGradCombineArgs a) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.npts; i += (long long)gridDim.x * blockDim.x) {
        const double d = a.n[i];
        double cvw = 0.0, cb = 0.0, ca = 0.0;
        if (a.flags & SG_VW) cvw = -1.0 / sqrt(d);
        if (a.flags & SG_WT) {
            // 0.3 (3 pi^2)^(2/3) as a product of doubles: one ulp below kCtf (the rounded long-double product), so it stays
            const double ctf = 0.3 * 9.570780000627306053141655531512398907;
            cb = ctf * a.al * pow(d, a.al - 1.0);
            ca = ctf * a.be * pow(d, a.be - 1.0);
            if (!(a.flags & SG_WT2)) cb += ca;                                    // alpha = beta: one convolution counts twice
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            double v = 0.0;
            if (a.flags & SG_HARTREE) v += a.f[c][i];
            if (a.flags & SG_VW) v += cvw * a.f[6 + c][i];
            if (a.flags & SG_WT) v += cb * a.f[12 + c][i];
            if (a.flags & SG_WT2) v += ca * a.f[18 + c][i];
            a.out[(long long)c * a.npts + i] = v;
        }
    }
}

// d v_ext / d eps_kl of one species at fixed fractional coordinates (the phase k.R is strain-invariant):
//   S_k [ -v~'(|k|) k_k k_l / |k| - delta_kl v~(|k|) ] / vol,  k = 0: -delta_kl S v~(0) / vol;   inverse with norm = 'forward'
struct IonStrainGradOut { cplx* s[6]; };
static __global__ void ion_strain_grad_spec_kernel(IonStrainGradOut out, KGeom kg, const double* __restrict__ cart, int nion, RecpotTable tab,
                                                   double inv_vol) {
    for_each_kpoint(kg, [&](const KPoint& p) {
        const cplx S = structure_factor(cart, nion, p.kx, p.ky, p.kz);
        const double kabs = (p.k2 != 0.0) ? sqrt(p.k2) : 0.0;
        const RecpotValue t = recpot<1>(tab, kabs);
        const double an = (p.k2 != 0.0) ? -t.dv / kabs * inv_vol : 0.0, iso = -t.v * inv_vol;
        double f[6];
        voigt6(an, iso, p, f);
#pragma unroll
        for (int c = 0; c < 6; ++c) out.s[c][p.i] = make_double2(S.x * f[c], S.y * f[c]);
    });
}

// Pair sum of the ion-ion energy, the geometry and pair set of ion_ion_kernel (0 < r <= Rc at the unstrained cell, Rd and Rc
// constants of the differentiation).  grid = (chunks, ions); for ion i over (j, lattice shift):
//   [0..14] (f'' - f'/r) d d d d / r^2   [15..20] (f'/r) d d   [21] sum Z_j (the neighbour charge of the background term)
constexpr int kIonStrain2Scalars = 22;
__global__ __launch_bounds__(kRedThreads) void ion_ion_strain2_kernel(const double* __restrict__ cart, const double* __restrict__ Z,
                                                                      int nion, IonIonGeom g, double* __restrict__ partial) {
    const int i = blockIdx.y;
    const double xi = cart[3 * i], yi = cart[3 * i + 1], zi = cart[3 * i + 2], Zi = Z[i];
    const int w0 = 2 * g.nmax[0] + 1, w1 = 2 * g.nmax[1] + 1, w2 = 2 * g.nmax[2] + 1;
    const long long total = (long long)nion * w0 * w1 * w2;
    const double inv_rd = 1.0 / g.Rd, two_over = 2.0 / (sqrt(kPi) * g.Rd);
    double acc[kIonStrain2Scalars];
#pragma unroll
    for (int s = 0; s < kIonStrain2Scalars; ++s) acc[s] = 0.0;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(t % nion);
        int s0, s1, s2;
        lattice_shift(g, t / nion, s0, s1, s2);
        const double dx = cart[3 * j] + s0 * g.box[0] + s1 * g.box[3] + s2 * g.box[6] - xi;
        const double dy = cart[3 * j + 1] + s0 * g.box[1] + s1 * g.box[4] + s2 * g.box[7] - yi;
        const double dz = cart[3 * j + 2] + s0 * g.box[2] + s1 * g.box[5] + s2 * g.box[8] - zi;
        const double r2 = dx * dx + dy * dy + dz * dz;
        if (in_cutoff(r2, g)) {
            double fpr, q;
            damped_pair_d2(r2, Zi * Z[j], inv_rd, two_over, fpr, q);
            add_k4(acc, q, dx, dy, dz);
            add_k2(acc + 15, fpr, dx, dy, dz);
            acc[21] += Z[j];
        }
    }
    block_reduce_store<kIonStrain2Scalars>(acc, partial + (long long)i * gridDim.x * kIonStrain2Scalars);
}

}  // namespace ofdft
