// Second derivatives with respect to ion positions, the pieces of the interatomic force constants (reference:
// System.force_constants, src/professad/system.py:695-717, 1340-1367, which differentiates lattice_sum, ion_utils.py:88-137,
// and ion_interaction_sum, ion_utils.py:293-333, a second time by autograd).  fp64, gfx950; exact structure factor only.
// Every reduction is a wavefront-shuffle reduction (block_reduce_store) plus a fixed-order second stage on the host: no atomics.
#pragma once
#include "ion_kernels.h"

namespace ofdft {

// d v_ext / d R_{a,j} in reciprocal space for ONE ion at (rx, ry, rz): out_j = -i k_j exp(-i k.R_a) v~(|k|) / vol, j = x, y, z.
// Phase and table value are formed once per k-point (k = 0: all three vanish with k_j).
__global__ void ion_potential_grad_spec_kernel(cplx* __restrict__ out0, cplx* __restrict__ out1, cplx* __restrict__ out2, KGeom kg,
                                               double rx, double ry, double rz, RecpotTable tab, double inv_vol) {
    for_each_kpoint(kg, [&](const KPoint& p) {
        double sn, cs;
        sincos(p.kx * rx + p.ky * ry + p.kz * rz, &sn, &cs);
        const double f = recpot<0>(tab, (p.k2 != 0.0) ? sqrt(p.k2) : 0.0).v * inv_vol;
        const double re = -f * sn, im = -f * cs;               // -i (cs - i sn) f
        out0[p.i] = make_double2(p.kx * re, p.kx * im);
        out1[p.i] = make_double2(p.ky * re, p.ky * im);
        out2[p.i] = make_double2(p.kz * re, p.kz * im);
    });
}

// sum_k w_k v~(|k|) k_i k_j Re(exp(-i k.R_a) conj(n^_k)) for every ion a: xx, yy, zz, xy, xz, yz.  grid = (k chunks, ions);
// partial[(a * gridDim.x + blockIdx.x) * 6 + s].  (The host scales by -dV / vol: the second derivative of dV sum_r n v_ext.)
constexpr int kIonCurvScalars = 6;
__global__ __launch_bounds__(kRedThreads) void ion_curvature_kernel(const cplx* __restrict__ nk, KGeom kg, const double* __restrict__ cart,
                                                                    RecpotTable tab, double* __restrict__ partial) {
    const int a = blockIdx.y;
    const double rx = cart[3 * a], ry = cart[3 * a + 1], rz = cart[3 * a + 2];
    double acc[kIonCurvScalars] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for_each_kpoint(kg, [&](const KPoint& p) {
        if (p.k2 == 0.0) return;
        const double w = half_weight(kg.g, p.z);
        double sn, cs;
        sincos(p.kx * rx + p.ky * ry + p.kz * rz, &sn, &cs);
        const cplx n = nk[p.i];
        add_k2(acc, w * recpot<0>(tab, sqrt(p.k2)).v * (cs * n.x - sn * n.y), p.kx, p.ky, p.kz);
    });
    block_reduce_store<kIonCurvScalars>(acc, partial + (long long)a * gridDim.x * kIonCurvScalars);
}

// Second derivative of the damped pair sum at a fixed pair list.  grid = (chunks, ions, rows): block (c, b, q) scans its share of
// the lattice shifts of the pair (p = rows[q], b) and accumulates
//   T(d) = (f'' - f'/r) d d^T / r^2 + (f'/r) I,   f(r) = Z_p Z_b erfc(r/Rd)/r,   d = R_b + shift - R_p,   0 < r <= Rc
// as xx, yy, zz, xy, xz, yz into partial[((q * nion + b) * gridDim.x + c) * 6 + s].  Blocks with b == p store zeros: the images of
// an ion itself move with it.  A block's sums depend on (p, b) and the geometry only, never on which rows were asked for.
constexpr int kIonHessScalars = 6;
__global__ __launch_bounds__(kRedThreads) void ion_ion_hessian_kernel(const double* __restrict__ cart, const double* __restrict__ Z, int nion,
                                                                      IonIonGeom g, const int* __restrict__ rows,
                                                                      double* __restrict__ partial) {
    const int b = blockIdx.y, p = rows[blockIdx.z];
    const double xp = cart[3 * p], yp = cart[3 * p + 1], zp = cart[3 * p + 2];
    const double xb = cart[3 * b] - xp, yb = cart[3 * b + 1] - yp, zb = cart[3 * b + 2] - zp, zz = Z[p] * Z[b];
    const int w0 = 2 * g.nmax[0] + 1, w1 = 2 * g.nmax[1] + 1, w2 = 2 * g.nmax[2] + 1;
    const long long total = (b == p) ? 0 : (long long)w0 * w1 * w2;
    const double inv_rd = 1.0 / g.Rd, two_over = 2.0 / (sqrt(kPi) * g.Rd);
    double acc[kIonHessScalars] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        int s0, s1, s2;
        lattice_shift(g, t, s0, s1, s2);
        const double dx = xb + s0 * g.box[0] + s1 * g.box[3] + s2 * g.box[6];
        const double dy = yb + s0 * g.box[1] + s1 * g.box[4] + s2 * g.box[7];
        const double dz = zb + s0 * g.box[2] + s1 * g.box[5] + s2 * g.box[8];
        const double r2 = dx * dx + dy * dy + dz * dz;
        if (in_cutoff(r2, g)) {
            double fpr, q;
            damped_pair_d2(r2, zz, inv_rd, two_over, fpr, q);
            acc[0] += q * dx * dx + fpr;
            acc[1] += q * dy * dy + fpr;
            acc[2] += q * dz * dz + fpr;
            acc[3] += q * dx * dy;
            acc[4] += q * dx * dz;
            acc[5] += q * dy * dz;
        }
    }
    block_reduce_store<kIonHessScalars>(acc, partial + ((long long)blockIdx.z * nion + b) * gridDim.x * kIonHessScalars);
}

}  // namespace ofdft
