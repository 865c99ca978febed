// The device-side frame of the per-geometry-step spectral kernels (ion_kernels.h, stress_kernels.h, fc_kernels.h,
// strain2_kernels.h): the walk over the half spectrum, its weights, the structure factors, the pseudopotential
// table with its derivatives and the tensor moments of k, each stated once.  fp64 library only, as those kernels are.
// Every piece is inlined, and a statement moved here is the statement it was: -ffp-contract=on contracts per source expression,
// so the kernels round as they did when they spelled these lines out themselves.
#pragma once
#include "pointwise_kernels.h"

namespace ofdft {

// One point of the half spectrum: its index in the engine's spectrum layout, its grid indices and its wave vector.
struct KPoint {
    long long i;
    int x, y, z;
    double kx, ky, kz, k2;
};

// Grid-stride walk over the spectrum of kg: f(p) for every k-point p.  A kernel's body is a lambda that captures its
// accumulators by reference; `return` inside it goes on to the next point.
template <class F>
__device__ __forceinline__ void for_each_kpoint(const KGeom& kg, F&& f) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < kg.g.total; i += (long long)gridDim.x * blockDim.x) {
        KPoint p;
        p.i = i;
        spec_decode(kg.g, i, p.x, p.y, p.z);
        kvec_xyz(kg, p.x, p.y, p.z, p.kx, p.ky, p.kz, p.k2);
        f(p);
    }
}

// weight of a kz plane in a sum over the full spectrum: the planes kz = 0 and (n2 even) kz = n2 / 2 are their own mirror images
__device__ __forceinline__ double half_weight(const SpecGeom& g, int z) {
    return (z == 0 || ((g.n2 & 1) == 0 && z == g.n2 / 2)) ? 1.0 : 2.0;
}

// exact structure factor sum_a exp(-i k.R_a) (ion_utils.py:121-137)
__device__ __forceinline__ cplx structure_factor(const double* __restrict__ cart, int nion, double kx, double ky, double kz) {
    double sr = 0.0, si = 0.0;
    for (int a = 0; a < nion; ++a) {
        double sn, cs;
        sincos(kx * cart[3 * a] + ky * cart[3 * a + 1] + kz * cart[3 * a + 2], &sn, &cs);
        sr += cs;
        si -= sn;
    }
    return make_double2(sr, si);
}

// particle-mesh-Ewald structure factor conj(b0 b1 b2 Q^) (ion_utils.py:275-286); with the density's spectrum for Q^, its adjoint
__device__ __forceinline__ cplx pme_structure_factor(const cplx* __restrict__ b0, const cplx* __restrict__ b1,
                                                     const cplx* __restrict__ b2, const cplx* __restrict__ Qk, const KPoint& p) {
    return cconj(cmul(cmul(cmul(b0[p.x], b1[p.y]), b2[p.z]), Qk[p.i]));
}

struct RecpotTable {
    const double* ks;    // [n] uniform grid from 0
    const double* y;     // [n] table with the Coulomb tail 4 pi z/k^2 added for k > 0 (ion_utils.py:67-68)
    const double* m;     // [n] Hermite slopes (functional_tools.py:309-310)
    int n;
    double z;
    double inv_dk;
};
struct RecpotValue { double v, dv, d2v; };

// interpolate_recpot at |k| (ion_utils.py:74-81; functional_tools.py:311-334) with its first ORDER derivatives in |k|: the cubic
// Hermite interpolant inside an interval, the end value with zero slope and curvature beyond the table end (torch.minimum
// clamp), the Coulomb tail -4 pi z / k^2 taken off.  Derivatives above ORDER are returned as zero.
template <int ORDER>
__device__ __forceinline__ RecpotValue recpot(const RecpotTable& t, double kabs) {
    const double xs = fmin(kabs, t.ks[t.n - 1]);
    int idx = (int)ceil(xs * t.inv_dk) - 1;
    idx = max(0, min(idx, t.n - 2));
    while (idx > 0 && t.ks[idx] >= xs) --idx;            // searchsorted(x[1:], xs): #entries of x[1:] below xs
    while (idx < t.n - 2 && t.ks[idx + 1] < xs) ++idx;
    const double dx = t.ks[idx + 1] - t.ks[idx];
    const double u = (xs - t.ks[idx]) / dx, u2 = u * u, u3 = u2 * u;
    const bool inside = kabs < t.ks[t.n - 1];
    RecpotValue r = {0.0, 0.0, 0.0};
    r.v = (1.0 - 3.0 * u2 + 2.0 * u3) * t.y[idx] + (u - 2.0 * u2 + u3) * t.m[idx] * dx +
          (3.0 * u2 - 2.0 * u3) * t.y[idx + 1] + (-u2 + u3) * t.m[idx + 1] * dx;
    if constexpr (ORDER >= 1) {
        const double d = ((6.0 * u2 - 6.0 * u) * t.y[idx] + (3.0 * u2 - 4.0 * u + 1.0) * t.m[idx] * dx +
                          (-6.0 * u2 + 6.0 * u) * t.y[idx + 1] + (3.0 * u2 - 2.0 * u) * t.m[idx + 1] * dx) / dx;
        r.dv = inside ? d : 0.0;
    }
    if constexpr (ORDER >= 2) {
        const double d2 = ((12.0 * u - 6.0) * t.y[idx] + (6.0 * u - 4.0) * t.m[idx] * dx +
                           (-12.0 * u + 6.0) * t.y[idx + 1] + (6.0 * u - 2.0) * t.m[idx + 1] * dx) / (dx * dx);
        r.d2v = inside ? d2 : 0.0;
    }
    if (kabs != 0.0) {
        if constexpr (ORDER >= 1) r.dv += 8.0 * kPi * t.z / (kabs * kabs * kabs);
        if constexpr (ORDER >= 2) r.d2v -= 24.0 * kPi * t.z / (kabs * kabs * kabs * kabs);
        r.v = r.v - 4.0 * kPi * t.z / (kabs * kabs);
    } else {
        r.dv = r.d2v = 0.0;
    }
    return r;
}

// acc[0..5] += f k_a k_b: xx, yy, zz, xy, xz, yz
__device__ __forceinline__ void add_k2(double* acc, double f, double x, double y, double z) {
    acc[0] += f * x * x;
    acc[1] += f * y * y;
    acc[2] += f * z * z;
    acc[3] += f * x * y;
    acc[4] += f * x * z;
    acc[5] += f * y * z;
}
// acc[0..14] += f k_a k_b k_c k_d over the sorted quadruples xxxx xxxy xxxz xxyy xxyz xxzz xyyy xyyz xyzz xzzz yyyy yyyz yyzz yzzz zzzz
__device__ __forceinline__ void add_k4(double* acc, double f, double x, double y, double z) {
    const double xx = f * x * x, xy = f * x * y, xz = f * x * z, yy = f * y * y, yz = f * y * z, zz = f * z * z;
    acc[0] += xx * x * x;
    acc[1] += xx * x * y;
    acc[2] += xx * x * z;
    acc[3] += xx * y * y;
    acc[4] += xx * y * z;
    acc[5] += xx * z * z;
    acc[6] += xy * y * y;
    acc[7] += xy * y * z;
    acc[8] += xy * z * z;
    acc[9] += xz * z * z;
    acc[10] += yy * y * y;
    acc[11] += yy * y * z;
    acc[12] += yy * z * z;
    acc[13] += yz * z * z;
    acc[14] += zz * z * z;
}

// f[c] = an k_k k_l + delta_kl iso, the six factors of a strain gradient in the order xx, yy, zz, yz, xz, xy
__device__ __forceinline__ void voigt6(double an, double iso, const KPoint& p, double (&f)[6]) {
    const double kk[6] = {p.kx * p.kx, p.ky * p.ky, p.kz * p.kz, p.ky * p.kz, p.kx * p.kz, p.kx * p.ky};
#pragma unroll
    for (int c = 0; c < 6; ++c) f[c] = an * kk[c] + (c < 3 ? iso : 0.0);
}

}  // namespace ofdft
