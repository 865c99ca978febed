// Kernels of the Huang-Carter kinds of OFDFT_NLK (OFDFT_P_NLK_KIND = 4: HuangCarter, 5: RevisedHuangCarter; functionals.py:1176-1365;
// fp64, gfx950).  The kernel w(|r - r'|, xi(r)) depends on the density at r, so the term is evaluated as the reference's
// field_dependent_convolution does (functional_tools.py:381-423): one convolution of g = n^beta per node xi_j of a geometric
// node set, and a cubic Hermite spline over the nodes at every point.  With p = 8/3 - beta, C = 0.3 (3 pi^2)^(2/3) 8 (3 pi^2),
// gamma = |grad n|^2 and f_j = F^-1[w(q / xi_j) g^]:
//     K = sum_o c_o f_(i+o),  K_xi = sum_o c'_o f_(i+o)   (o = -1 .. 2, i the spline interval of xi(r), c_o the Hermite weights)
//     E = dV sum A K,  A = C n^p / xi^3,    Q = C n^p (K_xi / xi^3 - 3 K / xi^4)
//     v = C p n^(p-1) K / xi^3 + Q dxi/dn - div(2 Q dxi/dgamma grad n) + beta n^(beta-1) F^-1[sum_j w(q / xi_j) F[W_j]]
// with W_j(r) = A(r) c_o(r) where j = i(r) + o and 0 elsewhere.  The node set is a constant of the differentiation (the reference
// takes xi_min and xi_max with .item()).  Host sequence: engine_hc.inc.h; derivation and stage list: DESIGN.md 9g.
// No atomics; every sum in a fixed order (wavefront shuffles, then rows): bitwise reproducible.
#pragma once
#include "pointwise_kernels.h"

namespace ofdft {

enum { NLK_HC = 4, NLK_REVHC = 5 };
constexpr int kHcMaxNodes = 64;        // most spline nodes of one evaluation (the node list travels as a kernel argument)
// slots of c->d_reduced beyond the published block (kReducedLen .. kMaxScalars)
constexpr int kHcRedE = 20, kHcRedBad = 21, kHcRedVn = 22, kHcRedMin = 24, kHcRedMax = 25;
static_assert(kHcRedE >= kReducedLen && kHcRedMax < kMaxScalars, "the chain's sums lie behind the evaluation's");

struct HcPar {
    int kind;
    double p0, p1;         // HC: lambda, -;  revHC: a, b
    double beta, kappa;
};
struct HcNodes {
    int M;
    double xi[kHcMaxNodes];
};
struct HcTable {           // w(eta) on the uniform grid eta_k = k h, with the node slopes of functional_tools.interpolate
    const double* w;
    const double* m;
    int n;
    double h, eta_max;
};

// xi(r) and its derivatives with respect to n and gamma = |grad n|^2
//   HC     xi = 2 k_F (1 + lambda gamma / (n^(8/3) + 1e-30))                 functionals.py:1243-1245
//   revHC  xi = 2 k_F (1 + a s^2 / (1 + b s^2)), s^2 = gamma / (4 (3 pi^2)^(2/3) n^(8/3))      :1342-1345, functional_tools.py:268
struct HcXi { double xi, dn, dg; };
__device__ __forceinline__ HcXi hc_xi_point(const HcPar& p, double n, double gam) {
    const double kf2 = 2.0 * cbrt(3.0 * kPi * kPi * n);
    const double n83 = pow(n, 8.0 / 3.0);
    double F, dFdn, dFdg;
    if (p.kind == NLK_HC) {
        const double d = n83 + 1e-30;
        F = 1.0 + p.p0 * gam / d;
        dFdg = p.p0 / d;
        dFdn = -p.p0 * gam * (8.0 / 3.0) * (n83 / n) / (d * d);
    } else {
        const double cs = 0.25 / (double)kCbrt9Pi4;
        const double s2 = cs * gam / n83, den = 1.0 + p.p1 * s2, dFds2 = p.p0 / (den * den);
        F = 1.0 + p.p0 * s2 / den;
        dFdg = dFds2 * cs / n83;
        dFdn = dFds2 * (-(8.0 / 3.0) * s2 / n);
    }
    HcXi r;
    r.xi = kf2 * F;
    r.dn = kf2 / (3.0 * n) * F + kf2 * dFdn;
    r.dg = kf2 * dFdg;
    return r;
}

// ---- head: min / max of xi over the grid (two stages: per workgroup, then one workgroup over the rows; fixed order)
__device__ __forceinline__ void hc_block_minmax(double mn, double mx, double* __restrict__ out2) {
    __shared__ double red[2][kRedThreads / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mn = fmin(mn, __shfl_down(mn, off, 64));
        mx = fmax(mx, __shfl_down(mx, off, 64));
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        red[0][w] = mn;
        red[1][w] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int ww = 1; ww < kRedThreads / 64; ++ww) {
            mn = fmin(mn, red[0][ww]);
            mx = fmax(mx, red[1][ww]);
        }
        out2[0] = mn;
        out2[1] = mx;
    }
}
static __global__ __launch_bounds__(kRedThreads) void hc_minmax_kernel(const double* __restrict__ n, const double* __restrict__ gx,
                                                                       const double* __restrict__ gy, const double* __restrict__ gz,
                                                                       long long npts, HcPar par, double* __restrict__ partial) {
    double mn = INFINITY, mx = -INFINITY;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < npts; i += (long long)gridDim.x * blockDim.x) {
        const double a = gx[i], b = gy[i], c = gz[i];
        const double xi = hc_xi_point(par, n[i], a * a + b * b + c * c).xi;
        // (a density that is not positive gives NaN here; fmin / fmax would drop it, so it is carried as -inf / +inf for the host to refuse)
        mn = (xi == xi) ? fmin(mn, xi) : -INFINITY;
        mx = (xi == xi) ? fmax(mx, xi) : INFINITY;
    }
    hc_block_minmax(mn, mx, partial + 2 * (long long)blockIdx.x);
}
static __global__ __launch_bounds__(kRedThreads) void hc_minmax_rows_kernel(const double* __restrict__ partial, int rows,
                                                                            double* __restrict__ out2) {
    double mn = INFINITY, mx = -INFINITY;
    for (int r = threadIdx.x; r < rows; r += kRedThreads) {
        mn = fmin(mn, partial[2 * r]);
        mx = fmax(mx, partial[2 * r + 1]);
    }
    hc_block_minmax(mn, mx, out2);
}

// ---- the table: w at eta (clamped to the last node; functionals.py:1257), cubic Hermite as functional_tools.py:309-334.  The grid
// is uniform, so the interval comes from arithmetic.  (searchsorted puts a value that sits ON node k into interval k - 1, the
// floor into interval k: the spline is continuous there, both give w_k.)
__device__ __forceinline__ double hc_table_interp(const HcTable& t, double eta) {
    eta = fmin(eta, t.eta_max);
    int idx = (int)(eta / t.h);
    idx = idx > t.n - 2 ? t.n - 2 : (idx < 0 ? 0 : idx);
    const double u = (eta - (double)idx * t.h) / t.h, u2 = u * u, u3 = u2 * u;
    const double h0 = 1.0 - 3.0 * u2 + 2.0 * u3, h1 = u - 2.0 * u2 + u3, h2 = 3.0 * u2 - 2.0 * u3, h3 = u3 - u2;
    return h0 * t.w[idx] + h1 * t.m[idx] * t.h + h2 * t.w[idx + 1] + h3 * t.m[idx + 1] * t.h;
}

// ---- spectral: f^_j = w(q / xi_j) g^ for every node, g^ read once per k-point; out = [M][total]
static __global__ void hc_spec_kernel(const cplx* __restrict__ g, cplx* __restrict__ out, KGeom kg, HcNodes nd, HcTable t) {
    const long long total = kg.g.total;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        real kx, ky, kz, k2;
        kvec(kg, i, kx, ky, kz, k2);
        const double q = (k2 != 0.0) ? sqrt(k2) : 0.0;                   // functionals.py:1262-1263
        const cplx a = g[i];
        for (int j = 0; j < nd.M; ++j) {
            const double w = hc_table_interp(t, q / nd.xi[j]);
            out[(long long)j * total + i] = mkc(a.x * w, a.y * w);
        }
    }
}

// ---- gather: spline over the nodes at every point (functional_tools.py:337-378, with the derivative in xi), the local part of
// the potential, the vector 2 Q dxi/dgamma grad n (over grad n, in place) and the node weights W_j (over f_j, in place: all M
// entries of a point are written, zeros included).  partial[][2]: sum A K, and the count of points whose interval had to be
// clamped (the three guard nodes on either side make that unreachable: the host refuses the evaluation if it is not 0).
// Under the 1024-thread bound of the reducing kernels (128 VGPRs per lane) the compiler's resource report for gfx950
// (-Rpass-analysis=kernel-resource-usage) gives 127 VGPRs, no scratch and no VGPR spill, 6 SGPRs kept in VGPR lanes, 4 waves per SIMD.
static __global__ __launch_bounds__(kRedThreads) void hc_gather_kernel(const double* __restrict__ n, double* __restrict__ gx,
                                                                       double* __restrict__ gy, double* __restrict__ gz,
                                                                       double* __restrict__ f, double* __restrict__ vloc,
                                                                       long long npts, HcPar par, HcNodes nd, double C,
                                                                       acc_t* __restrict__ partial) {
    __shared__ double sx[kHcMaxNodes];
    const int M = nd.M;
    if (threadIdx.x == 0)
        for (int j = 0; j < M; ++j) sx[j] = nd.xi[j];
    __syncthreads();
    acc_t acc[2] = {0.0, 0.0};
    const double p = 8.0 / 3.0 - par.beta;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < npts; r += (long long)gridDim.x * blockDim.x) {
        const double den = n[r], a = gx[r], b = gy[r], c = gz[r];
        const HcXi x = hc_xi_point(par, den, a * a + b * b + c * c);
        // i = searchsorted(xs[1:], xi): the number of nodes j >= 1 below xi
        int lo = 1, hi = M;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sx[mid] < x.xi) lo = mid + 1;
            else hi = mid;
        }
        int i = lo - 1;
        if (i < 1 || i > M - 3) {
            acc[1] += 1.0;
            i = i < 1 ? 1 : M - 3;
        }
        const double x0 = sx[i], D = sx[i + 1] - x0, Dm = x0 - sx[i - 1], Dp = sx[i + 2] - sx[i + 1];
        const double u = (x.xi - x0) / D, u2 = u * u, u3 = u2 * u;
        const double h0 = 1.0 - 3.0 * u2 + 2.0 * u3, h1 = u - 2.0 * u2 + u3, h2 = 3.0 * u2 - 2.0 * u3, h3 = u3 - u2;
        const double d0 = (6.0 * u2 - 6.0 * u) / D, d1 = (1.0 - 4.0 * u + 3.0 * u2) / D, d2 = (6.0 * u - 6.0 * u2) / D,
                     d3 = (3.0 * u2 - 2.0 * u) / D;
        // node slopes m_j = (s_j + s_(j-1)) / 2, s_j = (f_(j+1) - f_j) / (xi_(j+1) - xi_j): weights of the nodes i-1 .. i+2
        const double a1 = h1 * D * 0.5, a2 = h3 * D * 0.5, e1 = d1 * D * 0.5, e2 = d3 * D * 0.5;
        const double c0 = -a1 / Dm, c1 = h0 + a1 / Dm - a1 / D - a2 / D, c2 = h2 + a1 / D + a2 / D - a2 / Dp, c3 = a2 / Dp;
        const double g0 = -e1 / Dm, g1 = d0 + e1 / Dm - e1 / D - e2 / D, g2 = d2 + e1 / D + e2 / D - e2 / Dp, g3 = e2 / Dp;
        double* fr = f + r;
        const double f0 = fr[(long long)(i - 1) * npts], f1 = fr[(long long)i * npts], f2 = fr[(long long)(i + 1) * npts],
                     f3 = fr[(long long)(i + 2) * npts];
        const double K = c0 * f0 + c1 * f1 + c2 * f2 + c3 * f3, Kx = g0 * f0 + g1 * f1 + g2 * f2 + g3 * f3;
        const double np1 = pow(den, p - 1.0), xi3 = x.xi * x.xi * x.xi;
        const double A = C * np1 * den / xi3;
        const double Q = C * np1 * den * (Kx / xi3 - 3.0 * K / (xi3 * x.xi));
        acc[0] += A * K;
        vloc[r] = C * p * np1 * K / xi3 + Q * x.dn;
        const double uq = 2.0 * Q * x.dg;
        gx[r] = uq * a;
        gy[r] = uq * b;
        gz[r] = uq * c;
        for (int j = 0; j < M; ++j) {
            const int o = j - i;
            fr[(long long)j * npts] = o == -1 ? A * c0 : (o == 0 ? A * c1 : (o == 1 ? A * c2 : (o == 2 ? A * c3 : 0.0)));
        }
    }
    block_reduce_store<2>(acc, partial);
}

// ---- adjoint: adj^ = sum_j w(q / xi_j) W^_j and div^ = i k . u^ (div may be ux: every k-point reads before it writes)
static __global__ void hc_adjoint_kernel(const cplx* __restrict__ W, const cplx* ux, const cplx* __restrict__ uy,
                                         const cplx* __restrict__ uz, cplx* __restrict__ adj, cplx* div, KGeom kg, HcNodes nd,
                                         HcTable t) {
    const long long total = kg.g.total;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        real kx, ky, kz, k2;
        kvec(kg, i, kx, ky, kz, k2);
        const double q = (k2 != 0.0) ? sqrt(k2) : 0.0;
        double re = 0.0, im = 0.0;
        for (int j = 0; j < nd.M; ++j) {
            const double w = hc_table_interp(t, q / nd.xi[j]);
            const cplx a = W[(long long)j * total + i];
            re += w * a.x;
            im += w * a.y;
        }
        adj[i] = mkc(re, im);
        const cplx a = ux[i], b = uy[i], c = uz[i];
        div[i] = mkc(-(kx * a.y + ky * b.y + kz * c.y), kx * a.x + ky * b.x + kz * c.x);
    }
}

// ---- tail: v_NL = local - div + beta n^(beta-1) adj (over the local part, in place); partial[] = sum n v_NL
static __global__ __launch_bounds__(kRedThreads) void hc_tail_kernel(const double* __restrict__ n, double* __restrict__ v,
                                                                     const double* __restrict__ div, const double* __restrict__ adj,
                                                                     long long npts, double beta, acc_t* __restrict__ partial) {
    acc_t acc[1] = {0.0};
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < npts; r += (long long)gridDim.x * blockDim.x) {
        const double den = n[r];
        const double val = v[r] - div[r] + beta * pow(den, beta - 1.0) * adj[r];
        v[r] = val;
        acc[0] += den * val;
    }
    block_reduce_store<1>(acc, partial);
}

// ---- epilogue: the term joins the rest of the evaluation.  chi == nullptr (ofdft_energy_potential): out (+)= v_NL.  Otherwise
// (ofdft_energy_grad_chi): out (+)= 2 c chi (v_NL - s) dV with s = sum(n v_NL) dV / N_e from the device-side reduction -- the
// term's share of mu -- and c the closure scale (system.py:833-837, 850-853)
static __global__ void hc_epilogue_kernel(const double* __restrict__ v, double* __restrict__ out, long long npts, int accumulate,
                                          const double* __restrict__ chi, const acc_t* __restrict__ cscale, double two_dV,
                                          const acc_t* __restrict__ vn, double dV_over_nel) {
    const double s = chi ? vn[0] * dV_over_nel : 0.0, cs = chi ? cscale[0] * two_dV : 0.0;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < npts; r += (long long)gridDim.x * blockDim.x) {
        const double t = chi ? cs * chi[r] * (v[r] - s) : v[r];
        out[r] = accumulate ? out[r] + t : t;
    }
}

}  // namespace ofdft
