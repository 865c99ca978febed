// C ABI of the ion-position second derivatives behind the interatomic force constants (fc_kernels.h): the gradient
// of the ionic potential with respect to one ion, the ion-electron curvature at fixed density and the ion-ion Hessian.  Included
// once by engine.hip inside its extern "C" block (fp64 library), after engine_ions_stress.inc.h (the frames of the ion entries).
// Single GPU, exact structure factor.  Each entry clears hvp_valid, the fields ofdft_hessian_vector retains for reuse_density = 1,
// as every second-order entry does: the ABI's convention, not a need (none writes an "hv:*" workspace; table in DESIGN.md §9f).

// d v_ext / d R_{a,j}, j = x, y, z, of the ion a = ion_index of one species (what autograd through lattice_sum yields,
// ion_utils.py:88-137): one spectral kernel, one batched inverse transform.
int ofdft_ionic_potential_gradient(ofdft_ctx* c, const double* frac_host, int nions, const double* tab_k, const double* tab_v, int ntab,
                                   double z_ion, int pme_order, int ion_index, void* dv_dev, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!c || !frac_host || !tab_k || !tab_v || !dv_dev) return OFDFT_EINVAL;
    IonPrep p(c);
    if (int rc = ion_begin(c, p, "ofdft_ionic_potential_gradient", true, frac_host, nions, tab_k, tab_v, ntab, z_ion, pme_order, st, &ion_index))
        return rc;
    cplx* spec[3];
    real* out[3];
    const char* names[3] = {"fc:g0", "fc:g1", "fc:g2"};
    for (int j = 0; j < 3; ++j) {
        if (int rc = spec_ws(c, names[j], &spec[j])) return rc;
        out[j] = (real*)dv_dev + (size_t)j * c->npts;
    }
    const double* R = p.cart.data() + 3 * (size_t)ion_index;
    OFDFT_LAUNCH(c, st, "ion_grad_spec", ion_potential_grad_spec_kernel, dim3(grid_for(c->g.total)), dim3(256), 0, spec[0], spec[1], spec[2],
                 c->kg, R[0], R[1], R[2], p.tab, 1.0 / c->vol);
    if (int rc = irfftn_internal_multi(c, spec, out, 3, 1.0, st)) return rc;      // norm='forward': no 1/N  (ion_utils.py:118)
    return ion_finish(c, st);
}

// D[a] = d^2 (dV sum_r n v_ext) / dR_a dR_a at fixed n for every ion of one species: one transform of the density, one reduction
// kernel with six sums per ion.  curv_host [nions][6]: xx, yy, zz, xy, xz, yz (Ha/bohr^2).
int ofdft_ion_electron_curvature(ofdft_ctx* c, const void* den_dev, const double* frac_host, int nions, const double* tab_k,
                                 const double* tab_v, int ntab, double z_ion, int pme_order, double* curv_host, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!c || !den_dev || !frac_host || !tab_k || !tab_v || !curv_host) return OFDFT_EINVAL;
    IonPrep p(c);
    if (int rc = ion_begin(c, p, "ofdft_ion_electron_curvature", true, frac_host, nions, tab_k, tab_v, ntab, z_ion, pme_order, st)) return rc;
    cplx* sN;
    if (int rc = spec_ws(c, "i:Q", &sN)) return rc;
    if (int rc = rfftn_internal(c, (const double*)den_dev, sN, st)) return rc;
    const int kb = grid_for(c->g.total, kRedThreads, 64);
    double* d_part;
    std::vector<double> h((size_t)nions * kb * kIonCurvScalars);
    if (int rc = get_ws(c, "fc:cpart", sizeof(double) * h.size(), (void**)&d_part)) return rc;
    OFDFT_LAUNCH(c, st, "ion_curvature", ion_curvature_kernel, dim3(kb, nions), dim3(kRedThreads), 0, (const cplx*)sN, c->kg,
                 (const double*)p.d_cart, p.tab, d_part);
    HIP_TRY(c, hipMemcpyAsync(h.data(), d_part, sizeof(double) * h.size(), hipMemcpyDeviceToHost, st));
    if (int rc = ion_finish(c, st)) return rc;
    const double pref = -c->dV / c->vol;
    for (int a = 0; a < nions; ++a)
        for (int s = 0; s < kIonCurvScalars; ++s) curv_host[kIonCurvScalars * a + s] = pref * (double)chunk_sum(h.data(), a, kb, kIonCurvScalars, s);
    return OFDFT_OK;
}

// d^2 E_ion-ion / dR_p dR_b for the ions p of rows_host at a fixed pair list: what a second autograd pass over
// ion_interaction_sum (ion_utils.py:293-333) gives; Rd / Rc and the pair set are those of ofdft_ion_ion.  The background term
// depends on the neighbour charge counts only and has no second derivative.  hess_host [nrows][nions][3][3], Ha/bohr^2.
int ofdft_ion_ion_hessian(ofdft_ctx* c, const double* frac_host, const double* charges_host, int nions, double Rc, const int* rows_host,
                          int nrows, double* hess_host, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!c || !frac_host || !charges_host || !rows_host || !hess_host || nions < 1 || nrows < 1) return OFDFT_EINVAL;
    c->hvp_valid = false;
    IonIonCall ii;
    if (int rc = ion_ion_begin(c, ii, frac_host, nions, Rc)) return rc;
    for (int k = 0; k < nrows; ++k)
        if (rows_host[k] < 0 || rows_host[k] >= nions) return fail(c, OFDFT_EINVAL, "ofdft_ion_ion_hessian: row %d outside [0, %d)", rows_host[k], nions);
    if (nrows > 65535) return fail(c, OFDFT_EINVAL, "ofdft_ion_ion_hessian: at most 65535 rows per call");
    OFDFT_ON_DEVICE(c, c->device);
    const int chunks = ion_ion_chunks(ii.nshift);       // one (row, ion) pair per (grid.z, grid.y): the chunks split the shifts alone
    int* d_rows;
    if (int rc = get_ws(c, "fc:rows", sizeof(int) * nrows, (void**)&d_rows)) return rc;
    if (int rc = ion_ion_upload(c, ii, charges_host, nions, "fc:hpart", (size_t)nrows * nions, chunks, kIonHessScalars, st)) return rc;
    HIP_TRY(c, hipMemcpyAsync(d_rows, rows_host, sizeof(int) * nrows, hipMemcpyHostToDevice, st));
    OFDFT_LAUNCH(c, st, "ion_ion_hessian", ion_ion_hessian_kernel, dim3(chunks, nions, nrows), dim3(kRedThreads), 0, (const double*)ii.d_cart,
                 (const double*)ii.d_z, nions, ii.g, (const int*)d_rows, ii.d_part);
    if (int rc = ion_ion_fetch(c, ii, st)) return rc;
    for (int k = 0; k < nrows; ++k) {
        const int p = rows_host[k];
        double* row = hess_host + (size_t)k * nions * 9;
        long double diag[kIonHessScalars] = {0, 0, 0, 0, 0, 0};
        for (int b = 0; b < nions; ++b) {
            double t6[kIonHessScalars];
            for (int s = 0; s < kIonHessScalars; ++s) {
                const long double t = chunk_sum(ii.part.data(), (size_t)k * nions + b, chunks, kIonHessScalars, s);
                diag[s] += t;                       // (b == p: zeros)
                t6[s] = -(double)t;                 // off-diagonal block: -sum over shifts of T
            }
            sym_store(row + 9 * (size_t)b, t6, 0.0);
        }
        double d6[kIonHessScalars];
        for (int s = 0; s < kIonHessScalars; ++s) d6[s] = (double)diag[s];
        sym_store(row + 9 * (size_t)p, d6, 0.0);    // diagonal block: +sum over b != p and shifts
    }
    if (c->profiling) prof_collect(c);
    return OFDFT_OK;
}
