// C ABI of the Hessian-vector product (hvp_kernels.h).  Included once by engine.hip inside its extern "C" block (fp64 library).
//
// The call is three kernels around the batched whole-grid transforms of the unfused pipeline (rfftn_internal_multi /
// irfftn_internal_multi: powers of two, mixed-radix plans and chirp-z extents alike):
//   head     n, w -> sqrt n, w / 2 sqrt n, n^beta, n^(beta-1) w [, n^alpha, n^(alpha-1) w]      (w itself is transformed from the caller's array)
//   forward batch, one spectral kernel over every spectrum, inverse batch
//   combine  n, w, the inverse-transformed fields -> hv, per-term sums of w hv_t
// Density-only fields (lap sqrt n, K * n^beta, K * n^alpha) stay in "hv:lap", "hv:A", "hv:B" for calls with reuse_density = 1.
int ofdft_hessian_vector(ofdft_ctx* c, const void* den_dev, const void* dir_dev, void* hv_dev, double* quad_terms, int reuse_density,
                         void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!c) return OFDFT_EINVAL;
    OFDFT_ON_DEVICE(c, c->device);
    const bool retained = c->hvp_valid;
    if (int rc = begin_call(c, st)) return rc;         // (clears hvp_valid: a failed call leaves nothing to reuse)
    if (!den_dev || !dir_dev || !hv_dev) return fail(c, OFDFT_EINVAL, "null argument");
    if (!c->mask) return fail(c, OFDFT_ESTATE, "ofdft_set_terms has not been called");
    if (c->nranks > 1) return fail(c, OFDFT_EINVAL, "ofdft_hessian_vector is served by single-GPU contexts: slab-decomposed contexts have no second derivative");
    const unsigned mask = c->mask;
    static const struct { unsigned bit; const char* name; } refused[] = {
        {OFDFT_WGC99_NL, "wgc99_nl"}, {OFDFT_PBE_X, "pbe_x"}, {OFDFT_PBE_C, "pbe_c"}, {OFDFT_GGA_K, "gga_k"}, {OFDFT_VWGTF, "vwgtf"}, {OFDFT_NLK, "nlk"}};
    for (const auto& r : refused)
        if (mask & r.bit) return fail(c, OFDFT_EINVAL, "ofdft_hessian_vector: no second derivative of the term %s", r.name);
    if (wts_active(c))
        return fail(c, OFDFT_EINVAL, "ofdft_hessian_vector: no second derivative of the stabilised Wang-Teter style functional (OFDFT_P_WTS_KIND = 1, wts_kind)");
    if (reuse_density && !retained)
        return fail(c, OFDFT_ESTATE, "ofdft_hessian_vector: reuse_density = 1 without a preceding call with reuse_density = 0 on this cell and term set");
    const bool reuse = reuse_density != 0;
    const real* den = (const real*)den_dev;
    const real* w = (const real*)dir_dev;
    const long long npts = c->npts;
    const double inv_n = 1.0 / (double)npts;
    const bool has_h = mask & OFDFT_HARTREE, has_vw = mask & OFDFT_VW, has_wt = mask & OFDFT_WT_NL;

    double nel = c->hvp_nel;
    if (has_wt && !reuse) {                // n0 = mean(den) vol of THIS density: a constant of the differentiation (functionals.py:646-647)
        double nsum;
        if (int rc = device_sum(c, den, false, &nsum, st)) return rc;
        nel = nsum * inv_n * c->vol;
    }
    const TermScalars ts = term_scalars(c, nel);
    const bool two = has_wt && ts.nlp.two;

    // one item per transform: real input (also the head kernel's output), spectrum, operator, real output
    const real* fin[kHvpMaxSpectra];
    cplx* spec[kHvpMaxSpectra];
    real* fout[kHvpMaxSpectra];
    int op[kHvpMaxSpectra];
    int ns = 0;
    real *vh = nullptr, *lap = nullptr, *dlap = nullptr, *A = nullptr, *Cb = nullptr, *B = nullptr, *Ca = nullptr;
    auto item = [&](const real* in, const char* sname, int o, real* out) -> int {
        if (int rc = spec_ws(c, sname, &spec[ns])) return rc;
        fin[ns] = in;
        fout[ns] = out;
        op[ns++] = o;
        return 0;
    };
    if (has_h) {
        if (int rc = real_ws(c, "hv:vh", &vh)) return rc;
        if (int rc = item(w, "s0", SPEC_HARTREE, vh)) return rc;
    }
    if (has_vw) {
        if (int rc = real_ws(c, "hv:lap", &lap)) return rc;
        if (int rc = real_ws(c, "hv:dlap", &dlap)) return rc;
        if (!reuse)
            if (int rc = item(lap, "svw", SPEC_LAPLACE, lap)) return rc;
        if (int rc = item(dlap, "s1", SPEC_LAPLACE, dlap)) return rc;
    }
    if (has_wt) {
        if (int rc = real_ws(c, "hv:A", &A)) return rc;
        if (int rc = real_ws(c, "hv:Cb", &Cb)) return rc;
        if (!reuse)
            if (int rc = item(A, "swb", SPEC_LINDHARD, A)) return rc;
        if (int rc = item(Cb, "s2", SPEC_LINDHARD, Cb)) return rc;
        if (two) {
            if (int rc = real_ws(c, "hv:B", &B)) return rc;
            if (int rc = real_ws(c, "hv:Ca", &Ca)) return rc;
            if (!reuse)
                if (int rc = item(B, "swa", SPEC_LINDHARD, B)) return rc;
            if (int rc = item(Ca, "s3", SPEC_LINDHARD, Ca)) return rc;
        }
    }
    if (has_vw || has_wt) {
        HvpHeadArgs ha{};
        ha.n = den;
        ha.w = w;
        ha.chi = lap;  ha.dchi = dlap;
        ha.pb = A;     ha.pbw = Cb;
        ha.pa = B;     ha.paw = Ca;
        ha.npts = npts;
        ha.al = ts.nlp.al;
        ha.be = ts.nlp.be;
        ha.flags = (has_vw ? HVP_VW : 0) | (has_wt ? HVP_WT : 0) | (two ? HVP_WT2 : 0) | (reuse ? HVP_REUSE : 0);
        OFDFT_LAUNCH(c, st, "hvp_head", hvp_head_kernel, dim3(grid_for(npts / 2 + 1)), dim3(256), 0, ha);
    }
    if (ns) {
        for (int b0 = 0; b0 < ns; b0 += kBsBatch)
            if (int rc = rfftn_internal_multi(c, fin + b0, spec + b0, std::min(kBsBatch, ns - b0), st)) return rc;
        HvpSpecArgs sa{};
        for (int j = 0; j < ns; ++j) {
            sa.s[j] = spec[j];
            sa.op[j] = op[j];
        }
        sa.ns = ns;
        sa.lindhard = has_wt ? 1 : 0;
        sa.kg = c->kg;
        sa.pref = ts.wt_pref;
        sa.inv2kf = ts.wt_inv2kf;
        OFDFT_LAUNCH(c, st, "hvp_spec", hvp_spec_kernel, dim3(grid_for(c->g.total)), dim3(256), 0, sa);
        for (int b0 = 0; b0 < ns; b0 += kBsBatch)
            if (int rc = irfftn_internal_multi(c, spec + b0, fout + b0, std::min(kBsBatch, ns - b0), inv_n, st)) return rc;
    }
    HvpCombineArgs ca{};
    ca.n = den;
    ca.w = w;
    ca.vh = vh ? vh : den;
    ca.lap = lap ? lap : den;
    ca.dlap = dlap ? dlap : den;
    ca.A = A ? A : den;
    ca.Cb = Cb ? Cb : den;
    ca.B = B ? B : den;
    ca.Ca = Ca ? Ca : den;
    ca.hv = (real*)hv_dev;
    ca.npts = npts;
    ca.mask = mask;
    ca.two = two ? 1 : 0;
    ca.al = ts.nlp.al;
    ca.be = ts.nlp.be;
    const int blocks = grid_for(npts / 2 + 1, kRedThreads, kRedBlocks);
    OFDFT_LAUNCH(c, st, "hvp_combine", hvp_combine_kernel, dim3(blocks), dim3(kRedThreads), 0, ca, c->d_partial);
    if (quad_terms) {
        double sums[kHvpScalars];
        if (int rc = fetch_partials(c, blocks, kHvpScalars, sums, st)) return rc;
        for (int t = 0; t < OFDFT_NTERMS; ++t) quad_terms[t] = (t < kHvpScalars && ((mask >> t) & 1)) ? sums[t] * c->dV : 0.0;
    }
    if (int rc = end_call(c, st)) return rc;
    c->hvp_valid = true;
    c->hvp_nel = nel;
    return OFDFT_OK;
}
