// Ion-ion real-space damped pair sum over a cell list (ion_utils.py:293-333; the reference takes its pairs from a cell-list
// neighbour list, ion_utils.py:313-316).  Same eleven per-ion sums and the same pair expression as ion_ion_kernel
// (ion_kernels.h), but the candidates of a target ion are the ions of the cells within Rc of its own cell, not every
// (j, lattice shift).
//
// Layout: ions sorted by cell (cell index = (c0 m1 + c1) m2 + c2 of the wrapped fractional coordinates), coordinates and
// charges as four arrays, cell_start[ncells + 1].  The neighbour cells of EVERY target cell are the same list of offsets
// (o0, o1, o2), kept as runs (o0, o1, lo..hi along the last axis) whose cells can hold an ion within Rc of the target cell.
// An offset that leaves [0, m_d) wraps and contributes the lattice shift floor_div(c_d + o_d, m_d); a run is cut where it
// wraps, and each piece is one contiguous range of sorted ions with one shift.
//
// One workgroup per (target cell, tile of T = 256 / L target ions); L lanes share a target ion (L divides 64, so they sit in
// one wavefront).  The workgroup stages 256 shifted neighbours at a time in LDS (two buffers, one barrier per stage); lane l
// of a target takes neighbours l, l + L, ...: within a wavefront the lanes read L consecutive doubles (distinct banks for
// 64-bit reads) and lanes of different targets read the same addresses (broadcast).  The L lanes combine with wave shuffles
// in a fixed order, lane 0 runs the per-ion epilogue (Q_i -> Ra -> background terms and their strain derivative), and the
// block's eight sums go to partial[block][8].  Every pair is visited from both ends and nothing is accumulated atomically:
// the result is bitwise reproducible from call to call.
#pragma once
#include "pointwise_kernels.h"

namespace ofdft {

constexpr int kIonCellScalars = 8;      // E, pair stress xx yy zz xy xz yz (x vol), background strain trace (x vol)
constexpr int kIonCellThreads = kRedThreads;
struct IonCellGeom {
    double box[9];       // rows = lattice vectors
    int m[3];            // cells per axis
    double Rc, Rd, rho;  // rho = sum Z / vol
    int cell_lo;         // first target cell of this call's part
    int ntiles;          // tiles of T target ions per cell (grid = owned cells x ntiles)
    int nruns;
};

__device__ __forceinline__ int ion_cells_floor_div(int a, int m) { return (a >= 0) ? a / m : -((-a + m - 1) / m); }

template <int L>
__global__ __launch_bounds__(kIonCellThreads) void ion_cells_kernel(const double* __restrict__ xs, const double* __restrict__ ys,
                                                                    const double* __restrict__ zs, const double* __restrict__ qs,
                                                                    const int* __restrict__ cell_start,
                                                                    const int4* __restrict__ runs, IonCellGeom g,
                                                                    double* __restrict__ forces_sorted,
                                                                    double* __restrict__ partial) {
    constexpr int T = kIonCellThreads / L;
    __shared__ double sx[2][kIonCellThreads], sy[2][kIonCellThreads], sz[2][kIonCellThreads], sq[2][kIonCellThreads];
    const int tid = threadIdx.x;
    const int cell = g.cell_lo + (int)blockIdx.x / g.ntiles, tile = (int)blockIdx.x % g.ntiles;
    const int t_begin = cell_start[cell] + tile * T, t_end = cell_start[cell + 1];
    if (t_begin >= t_end) {      // a cell with fewer tiles than the fullest one: nothing to add (uniform over the block)
        if (tid < kIonCellScalars) partial[(long long)blockIdx.x * kIonCellScalars + tid] = 0.0;
        return;
    }
    const int l = tid % L, it = t_begin + tid / L;
    const bool valid = it < t_end;
    const int ir = valid ? it : t_begin;
    const double xi = xs[ir], yi = ys[ir], zi = zs[ir], Zi = qs[ir];
    const int m0 = g.m[0], m1 = g.m[1], m2 = g.m[2];
    const int c0 = cell / (m1 * m2), c1 = (cell / m2) % m1, c2 = cell % m2;
    const double inv_rd = 1.0 / g.Rd, two_over = 2.0 / (sqrt(kPi) * g.Rd), rc2 = g.Rc * g.Rc;
    double acc[kIonIonScalars];
#pragma unroll
    for (int s = 0; s < kIonIonScalars; ++s) acc[s] = 0.0;
    int buf = 0;
    for (int r = 0; r < g.nruns; ++r) {
        const int4 run = runs[r];
        const int n0 = c0 + run.x, n1 = c1 + run.y;
        const int q0 = ion_cells_floor_div(n0, m0), q1 = ion_cells_floor_div(n1, m1);
        const int rowbase = ((n0 - q0 * m0) * m1 + (n1 - q1 * m1)) * m2;
        const int a = c2 + run.z, b = c2 + run.w;
        const int qa = ion_cells_floor_div(a, m2), qb = ion_cells_floor_div(b, m2);
        for (int q = qa; q <= qb; ++q) {
            const int s = max(a, q * m2) - q * m2, e = min(b, q * m2 + m2 - 1) - q * m2;
            const int j0 = cell_start[rowbase + s], j1 = cell_start[rowbase + e + 1];
            const double shx = q0 * g.box[0] + q1 * g.box[3] + q * g.box[6];
            const double shy = q0 * g.box[1] + q1 * g.box[4] + q * g.box[7];
            const double shz = q0 * g.box[2] + q1 * g.box[5] + q * g.box[8];
            for (int base = j0; base < j1; base += kIonCellThreads) {
                // two buffers: a lane still reading stage k never meets a store of stage k + 1, and the barrier of stage k + 1
                // separates the reads of stage k from the stores of stage k + 2
                const int j = base + tid;
                if (j < j1) {
                    sx[buf][tid] = xs[j] + shx;
                    sy[buf][tid] = ys[j] + shy;
                    sz[buf][tid] = zs[j] + shz;
                    sq[buf][tid] = qs[j];
                }
                __syncthreads();
                const int cnt = min(kIonCellThreads, j1 - base);
                if (valid) {
                    for (int jj = l; jj < cnt; jj += L) {
                        const double dx = sx[buf][jj] - xi, dy = sy[buf][jj] - yi, dz = sz[buf][jj] - zi;
                        const double r2 = dx * dx + dy * dy + dz * dz;
                        if (r2 > 1e-24 && r2 <= rc2) {
                            const double Zj = sq[buf][jj];
                            const double rr = sqrt(r2), ir1 = 1.0 / rr, zz = Zi * Zj;
                            const double ec = erfc(rr * inv_rd) * ir1;
                            acc[0] += zz * ec;
                            acc[1] += Zj;
                            const double fpr = zz * (-two_over * exp(-r2 * inv_rd * inv_rd) * ir1 - ec * ir1) * ir1;     // f'(r) / r
                            acc[2] += fpr * dx;
                            acc[3] += fpr * dy;
                            acc[4] += fpr * dz;
                            acc[5] += fpr * dx * dx;
                            acc[6] += fpr * dy * dy;
                            acc[7] += fpr * dz * dz;
                            acc[8] += fpr * dx * dy;
                            acc[9] += fpr * dx * dz;
                            acc[10] += fpr * dy * dz;
                        }
                    }
                }
                buf ^= 1;
            }
        }
    }
    // the L lanes of a target: butterfly in a fixed order (every lane ends with the same sum)
#pragma unroll
    for (int s = 0; s < kIonIonScalars; ++s) {
#pragma unroll
        for (int off = L / 2; off > 0; off >>= 1) acc[s] += __shfl_xor(acc[s], off, 64);
    }
    double out[kIonCellScalars];
#pragma unroll
    for (int s = 0; s < kIonCellScalars; ++s) out[s] = 0.0;
    if (valid && l == 0) {
        // per-ion epilogue (ion_utils.py:318-331 and its strain derivative at fixed pair list: d rho / d eps_aa = -rho,
        // d Ra / d eps_aa = Ra / 3)
        const double Rd = g.Rd, rho = g.rho, spi = sqrt(kPi);
        const double Q = Zi + acc[1];
        const double Ra = cbrt(0.75 / kPi * Q / rho);
        const double ex = exp(-Ra * Ra / (Rd * Rd)), er = erf(Ra / Rd);
        out[0] = 0.5 * acc[0] - kPi * Zi * rho * Ra * Ra + kPi * Zi * rho * (Ra * Ra - 0.5 * Rd * Rd) * er +
                 spi * Zi * rho * Ra * Rd * ex - Zi * Zi / spi / Rd;
#pragma unroll
        for (int k = 0; k < 6; ++k) out[1 + k] = 0.5 * acc[5 + k];
        const double e_rho = -kPi * Zi * Ra * Ra + kPi * Zi * (Ra * Ra - 0.5 * Rd * Rd) * er + spi * Zi * Ra * Rd * ex;
        const double dE_dRa = -2.0 * kPi * Zi * rho * Ra + 2.0 * kPi * Zi * rho * Ra * er +
                              kPi * Zi * rho * (Ra * Ra - 0.5 * Rd * Rd) * 2.0 / (spi * Rd) * ex +
                              spi * Zi * rho * Rd * ex * (1.0 - 2.0 * Ra * Ra / (Rd * Rd));
        out[7] = -rho * e_rho + dE_dRa * Ra / 3.0;
        forces_sorted[3 * (long long)it] = acc[2];
        forces_sorted[3 * (long long)it + 1] = acc[3];
        forces_sorted[3 * (long long)it + 2] = acc[4];
    }
    block_reduce_store<kIonCellScalars>(out, partial);
}

}  // namespace ofdft
