// C ABI of the cell-list ion-ion sum (ion_cells.h).  Included once by engine.hip inside its extern "C" block, after
// engine_ions_stress.inc.h (sym_store, ion_ion_radii).  A first-order entry: it leaves the retained Hessian fields (hvp_valid).
namespace {

// Smallest |sum_d v_d u_d| over the box v_d in [o_d - 1, o_d + 1]: the distance between the closest points of two cells whose
// indices differ by o (u_d = lattice vector d / m_d; G = Gram matrix of the u_d).  Every choice of {free, at the lower bound, at
// the upper bound} per axis is solved; the feasible stationary points contain the minimiser and none lies below it.
double cell_pair_min_dist2(const double G[3][3], const int o[3]) {
    double best = 1e300;
    for (int code = 0; code < 27; ++code) {
        int st[3] = {code % 3, (code / 3) % 3, code / 9};      // 0 free, 1 lower, 2 upper
        double v[3];
        int fr[3], nf = 0;
        for (int d = 0; d < 3; ++d) {
            if (st[d] == 0) {
                fr[nf++] = d;
                v[d] = 0.0;
            } else {
                v[d] = o[d] + (st[d] == 1 ? -1.0 : 1.0);
            }
        }
        if (nf) {      // G_FF v_F = -G_FB v_B by elimination (G is positive definite, so is every principal block)
            double A[3][4];
            for (int i = 0; i < nf; ++i) {
                for (int j = 0; j < nf; ++j) A[i][j] = G[fr[i]][fr[j]];
                double rhs = 0.0;
                for (int d = 0; d < 3; ++d)
                    if (st[d] != 0) rhs -= G[fr[i]][d] * v[d];
                A[i][nf] = rhs;
            }
            for (int i = 0; i < nf; ++i)
                for (int k = i + 1; k < nf; ++k) {
                    const double f = A[k][i] / A[i][i];
                    for (int j = i; j <= nf; ++j) A[k][j] -= f * A[i][j];
                }
            bool ok = true;
            for (int i = nf - 1; i >= 0; --i) {
                double s = A[i][nf];
                for (int j = i + 1; j < nf; ++j) s -= A[i][j] * v[fr[j]];
                v[fr[i]] = s / A[i][i];
            }
            for (int i = 0; i < nf; ++i)
                if (std::fabs(v[fr[i]] - o[fr[i]]) > 1.0 + 1e-9) ok = false;
            if (!ok) continue;
        }
        double f = 0.0;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) f += v[i] * G[i][j] * v[j];
        best = std::min(best, f);
    }
    return std::max(best, 0.0);
}

}  // namespace

// Ion-ion interaction energy, forces and stress through a cell list (ion_utils.py:293-333 with the parameter heuristics of
// System.__ion_ion_interaction, system.py:733-754; forces / stress = what autograd yields, system.py:913-935).
// Rc <= 0: the reference's default (Rd = 2 h_max, Rc = 3 Rd^2 / h_max); Rc > 0, Rd <= 0: Rd = sqrt(h_max Rc / 3); both > 0: as
// given.  The call returns the share of the target cells [part ncells / nparts, (part + 1) ncells / nparts): their ions' energy
// and stress terms, and force rows of those ions only (zero elsewhere); the sum over parts is the whole result.
int ofdft_ion_ion_cells(ofdft_ctx* c, const double* frac_host, const double* charges_host, int nions, double Rc, double Rd,
                        int part, int nparts, double* E_host, double* forces_host, double* stress_host, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!c || !frac_host || !charges_host || !E_host || nions < 1) return OFDFT_EINVAL;
    if (nparts < 1 || part < 0 || part >= nparts) return fail(c, OFDFT_EINVAL, "need 0 <= part < nparts (got %d of %d)", part, nparts);
    if (!c->cell_set) return fail(c, OFDFT_ESTATE, "ofdft_set_cell has not been called");
    OFDFT_ON_DEVICE(c, c->device);
    const double* B = c->box;
    double h[3];
    ion_ion_radii(c, h, Rc, Rd);
    // Cells per axis: roughly cubic cells of kIonCellOccupancy ions on average, m_d = round(h_d / edge) with
    // edge = cbrt(occupancy vol / nions), at least one.  32 ions per cell keep a tile of target ions (below) mostly full while
    // the cells stay small against Rc, so the cells kept by the distance test hug the cutoff sphere; a cell with few ions
    // (m = (1, 1, 1) for a primitive cell) degenerates to the scan over lattice shifts.
    constexpr double kIonCellOccupancy = 32.0;
    const double edge = std::cbrt(kIonCellOccupancy * c->vol / (double)nions);
    IonCellGeom g{};
    std::memcpy(g.box, B, sizeof(g.box));
    long long ncells_ll = 1;
    for (int d = 0; d < 3; ++d) {
        g.m[d] = (int)std::min(1024.0, std::max(1.0, std::floor(h[d] / edge + 0.5)));
        ncells_ll *= g.m[d];
    }
    const int ncells = (int)ncells_ll;
    g.Rc = Rc;
    g.Rd = Rd;
    // wrap into [0, 1) (the pair set {R_j + shift - R_i} does not change), bin, counting sort by cell
    std::vector<double> fw(3 * (size_t)nions);
    std::vector<int> cell_of(nions), cell_start((size_t)ncells + 1, 0);
    double ztot = 0.0;
    for (int a = 0; a < nions; ++a) {
        int ci[3];
        for (int d = 0; d < 3; ++d) {
            double f = frac_host[3 * a + d];
            if (!std::isfinite(f)) return fail(c, OFDFT_EINVAL, "fractional coordinate %d of ion %d is not finite", d, a);
            f -= std::floor(f);
            f -= std::floor(f);
            if (f >= 1.0) f = 0.0;
            fw[3 * (size_t)a + d] = f;
            ci[d] = std::min(g.m[d] - 1, (int)(f * g.m[d]));
        }
        cell_of[a] = (ci[0] * g.m[1] + ci[1]) * g.m[2] + ci[2];
        cell_start[cell_of[a] + 1]++;
        ztot += charges_host[a];
    }
    int max_occ = 0;
    for (int k = 0; k < ncells; ++k) {
        max_occ = std::max(max_occ, cell_start[k + 1]);
        cell_start[k + 1] += cell_start[k];
    }
    std::vector<int> order(nions), fill(cell_start.begin(), cell_start.end() - 1);
    for (int a = 0; a < nions; ++a) order[fill[cell_of[a]]++] = a;       // stable: input order within a cell
    std::vector<double> soa(4 * (size_t)nions);
    for (int k = 0; k < nions; ++k) {
        const int a = order[k];
        const double* f = &fw[3 * (size_t)a];
        for (int d = 0; d < 3; ++d) soa[(size_t)d * nions + k] = f[0] * B[d] + f[1] * B[3 + d] + f[2] * B[6 + d];
        soa[3 * (size_t)nions + k] = charges_host[a];
    }
    g.rho = ztot / c->vol;
    // Target ions per tile T (lanes per target L = 256 / T, at most one wavefront): the T in {4 .. 256} with the fewest lane
    // slots sum_cells ceil(n_c / T) (T + 2); the 2 stands for a tile's share of staging a neighbour tile, which T targets
    // share.  A full tile per cell where the cells are evenly filled, several tiles per cell where one cell holds many ions.
    int T = 4;
    {
        long long best = -1;
        for (int t = 4; t <= kIonCellThreads; t *= 2) {
            long long cost = 0;
            for (int k = 0; k < ncells; ++k) cost += (long long)((cell_start[k + 1] - cell_start[k] + t - 1) / t) * (t + 2);
            if (best < 0 || cost <= best) {
                best = cost;
                T = t;
            }
        }
    }
    g.ntiles = std::max(1, (max_occ + T - 1) / T);
    // neighbour runs: offsets |o_d| <= floor(Rc m_d / h_d) + 1, kept where the two cells can hold a pair within Rc
    double G[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            G[i][j] = (B[3 * i] * B[3 * j] + B[3 * i + 1] * B[3 * j + 1] + B[3 * i + 2] * B[3 * j + 2]) / ((double)g.m[i] * g.m[j]);
    int R[3];
    for (int d = 0; d < 3; ++d) {
        const double r = std::floor(Rc * g.m[d] / h[d]) + 1.0;
        if (r > 4096.0) return fail(c, OFDFT_EINVAL, "Rc = %g spans more than 4096 cells along axis %d", Rc, d);
        R[d] = (int)r;
    }
    const double keep2 = Rc * Rc * (1.0 + 1e-9);
    std::vector<int4> runs;
    for (int o0 = -R[0]; o0 <= R[0]; ++o0)
        for (int o1 = -R[1]; o1 <= R[1]; ++o1) {
            int lo = 1, hi = 0;
            for (int o2 = -R[2]; o2 <= R[2]; ++o2) {
                const int o[3] = {o0, o1, o2};
                if (cell_pair_min_dist2(G, o) <= keep2) {
                    if (lo > hi) lo = o2;
                    hi = o2;
                }
            }
            if (lo <= hi) runs.push_back(make_int4(o0, o1, lo, hi));
        }
    g.nruns = (int)runs.size();
    const int c_lo = (int)((long long)part * ncells / nparts), c_hi = (int)((long long)(part + 1) * ncells / nparts);
    g.cell_lo = c_lo;
    const int own_lo = cell_start[c_lo], own_hi = cell_start[c_hi];
    *E_host = 0.0;
    if (forces_host) std::fill(forces_host, forces_host + 3 * (size_t)nions, 0.0);
    if (stress_host) std::fill(stress_host, stress_host + 9, 0.0);
    if (own_hi == own_lo) return OFDFT_OK;         // this part owns no ion
    const int blocks = (c_hi - c_lo) * g.ntiles;
    double *d_soa, *d_f, *d_part, *d_out;
    int* d_cs;
    int4* d_runs;
    if (int rc = get_ws(c, "ic:soa", sizeof(double) * soa.size(), (void**)&d_soa)) return rc;
    if (int rc = get_ws(c, "ic:f", sizeof(double) * 3 * (size_t)nions, (void**)&d_f)) return rc;
    if (int rc = get_ws(c, "ic:part", sizeof(double) * (size_t)blocks * kIonCellScalars, (void**)&d_part)) return rc;
    if (int rc = get_ws(c, "ic:out", sizeof(double) * kIonCellScalars, (void**)&d_out)) return rc;
    if (int rc = get_ws(c, "ic:cs", sizeof(int) * cell_start.size(), (void**)&d_cs)) return rc;
    if (int rc = get_ws(c, "ic:runs", sizeof(int4) * runs.size(), (void**)&d_runs)) return rc;
    HIP_TRY(c, hipMemcpyAsync(d_soa, soa.data(), sizeof(double) * soa.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_cs, cell_start.data(), sizeof(int) * cell_start.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_runs, runs.data(), sizeof(int4) * runs.size(), hipMemcpyHostToDevice, st));
    const double *xs = d_soa, *ys = d_soa + nions, *zs = d_soa + 2 * (size_t)nions, *qs = d_soa + 3 * (size_t)nions;
#define OFDFT_ION_CELLS_CASE(L)                                                                                                \
    case L:                                                                                                                   \
        OFDFT_LAUNCH(c, st, "ion_cells", (ion_cells_kernel<L>), dim3(blocks), dim3(kIonCellThreads), 0, xs, ys, zs, qs,        \
                     (const int*)d_cs, (const int4*)d_runs, g, d_f, d_part);                                                   \
        break
    switch (kIonCellThreads / T) {
        OFDFT_ION_CELLS_CASE(1);
        OFDFT_ION_CELLS_CASE(2);
        OFDFT_ION_CELLS_CASE(4);
        OFDFT_ION_CELLS_CASE(8);
        OFDFT_ION_CELLS_CASE(16);
        OFDFT_ION_CELLS_CASE(32);
        OFDFT_ION_CELLS_CASE(64);
    }
#undef OFDFT_ION_CELLS_CASE
    // block partials -> E, six pair-stress sums, the background trace term (fixed order: bitwise reproducible)
    OFDFT_LAUNCH(c, st, "ion_cells_reduce", reduce_partials_kernel, dim3(kIonCellScalars), dim3(kRedThreads), 0,
                 (const double*)d_part, blocks, kIonCellScalars, d_out, (double*)nullptr);
    double s[kIonCellScalars];
    std::vector<double> fs;
    HIP_TRY(c, hipMemcpyAsync(s, d_out, sizeof(s), hipMemcpyDeviceToHost, st));
    if (forces_host) {
        fs.resize(3 * (size_t)(own_hi - own_lo));
        HIP_TRY(c, hipMemcpyAsync(fs.data(), d_f + 3 * (size_t)own_lo, sizeof(double) * fs.size(), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(c, hipStreamSynchronize(st));
    HIP_TRY(c, hipGetLastError());
    *E_host = s[0];
    if (forces_host)
        for (int k = own_lo; k < own_hi; ++k)
            for (int d = 0; d < 3; ++d) forces_host[3 * (size_t)order[k] + d] = fs[3 * (size_t)(k - own_lo) + d];
    if (stress_host) {
        double c6[6];
        for (int k = 0; k < 6; ++k) c6[k] = s[1 + k] / c->vol;
        sym_store(stress_host, c6, s[7] / c->vol);
    }
    if (c->profiling) prof_collect(c);
    return OFDFT_OK;
}
