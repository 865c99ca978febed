// C ABI of the Hessian-vector products (hvp_kernels.h).  Included once by engine.hip inside its extern "C" block (fp64 library).
//
// A product is three kernels around the batched whole-grid transforms of the unfused pipeline (rfftn_internal_multi /
// irfftn_internal_multi: powers of two, mixed-radix plans and chirp-z extents alike):
//   head     n, w -> sqrt n, w / 2 sqrt n, n^beta, n^(beta-1) w [, n^alpha, n^(alpha-1) w]      (w itself is transformed from the caller's array)
//   forward batch, one spectral kernel over every spectrum, inverse batch
//   combine  n, w, the inverse-transformed fields -> hv, per-term sums of w hv_t
// Density-only fields (lap sqrt n, K * n^beta, K * n^alpha) stay in "hv:lap", "hv:A", "hv:B" for calls with reuse_density = 1.
// With pbe_x or pbe_c in the term set (OFDFT_OPT_HVP_GGA = 1) a second stage runs in front of that batch:
//   forward n, w | spec_grad | inverse -> grad n ("hv:gn0..2", density-only: retained too), grad w
//   mid      n, w, grad n, grad w -> f_nn w + f_ns dsigma ("hv:gpw"), the flux over grad w, the sums of pbe_x and pbe_c
//   forward flux | spec_div | inverse -> "hv:gdiv";   the combine kernel then starts hv from gpw - 2 gdiv
// With wgc99_nl in the term set (OFDFT_OPT_HVP_WGC = 1) a stage of its own runs behind that one:
//   wgc head  n, w -> a, p (density-only) and a' w, p' w, three fields each
//   per triple: forward | spec_wgc_mix | inverse, in place -> U = M a, G = M p ("hv:wU0..2", "hv:wG0..2": retained), M (a' w), M (p' w)
//   wgc tail  -> its hv, the sum of wgc99_nl; the combine kernel starts hv from that field (added to "hv:gpw" where PBE runs too)
//
// hvp_core schedules this once for both entries.  ofdft_hessian_vector hands it (n, w); ofdft_hessian_vector_chi hands it
// (phi, d) with HvpChi set: head and combine then run their chi-space instantiations, which form n and dn on the fly, and the
// call adds one two-sum sweep over (phi, d) in front and one shift of the output by the constant d mu behind.
// ofdft_hessian_vector_chi_multi and ofdft_precondition_multi (end of the file) run the chi-space schedule and the preconditioner
// for up to OFDFT_MULTI_MAX columns per call, sharing the density-side fields with the entries above.
namespace {

// the retained fields belong to the entry that made them: hvp_valid is kHvpNone, kHvpDensity or kHvpChi (every `= false` elsewhere clears it)
enum { kHvpNone = 0, kHvpDensity = 1, kHvpChi = 2 };

struct HvpChi {                  // chi-space call: nullptr for the n-space product
    const real* g;               // closure gradient or nullptr (stationary point)
    double nel;                  // electron number N
    double a, S, cs;             // phi.d, phi.phi, cs = N / (S dV)
    double sums[kHvpChiScalars]; // out: sum dv n, g.d, d.P, phi.P (hvp_kernels.h), when `want`
    bool want;
};

// which entry asks: the two single-column products serve pbe_x / pbe_c under OFDFT_OPT_HVP_GGA = 1 and wgc99_nl under OFDFT_OPT_HVP_WGC = 1
// (the stages of hvp_core); the multi-column product and the strain entries have no kernels for them and keep refusing them whatever
// the options say
enum HvpCaller { kHvpNoGga = 0, kHvpGga = 1 };

const char* hvp_refusal(ofdft_ctx* c, HvpCaller caller) {
    static const struct { unsigned bit; const char* name; } refused[] = {
        {OFDFT_WGC99_NL, "wgc99_nl"}, {OFDFT_PBE_X, "pbe_x"}, {OFDFT_PBE_C, "pbe_c"}, {OFDFT_GGA_K, "gga_k"}, {OFDFT_VWGTF, "vwgtf"}, {OFDFT_NLK, "nlk"}};
    unsigned served = 0u;
    if (caller == kHvpGga && c->hvp_gga) served |= OFDFT_PBE_X | OFDFT_PBE_C;
    if (caller == kHvpGga && c->hvp_wgc) served |= OFDFT_WGC99_NL;
    for (const auto& r : refused)
        if (c->mask & r.bit & ~served) return r.name;
    return nullptr;
}

// The spectral stage of a product, single- or multi-column: one item per transform -- real input (also the head kernel's output),
// spectrum, operator, real output -- run in the order added.
struct SpecStage {
    const real* fin[kHvpMultiSpectra];
    cplx* spec[kHvpMultiSpectra];
    real* fout[kHvpMultiSpectra];
    int op[kHvpMultiSpectra];
    int ns = 0;
    void add(const real* in, cplx* s, int o, real* out) {
        fin[ns] = in;
        spec[ns] = s;
        fout[ns] = out;
        op[ns++] = o;
    }
    // forward batches of kBsBatch, every spectrum times its operator in one launch (`name` in the profile), inverse batches
    int run(ofdft_ctx* c, const TermScalars& ts, const char* name, hipStream_t st) {
        if (!ns) return 0;
        for (int b0 = 0; b0 < ns; b0 += kBsBatch)
            if (int rc = rfftn_internal_multi(c, fin + b0, spec + b0, std::min(kBsBatch, ns - b0), st)) return rc;
        HvmSpecArgs sa{};
        for (int j = 0; j < ns; ++j) {
            sa.s[j] = spec[j];
            sa.op[j] = (unsigned char)op[j];
            if (op[j] == SPEC_LINDHARD) sa.lindhard = 1;
        }
        sa.ns = ns;
        sa.kg = c->kg;
        sa.pref = ts.wt_pref;
        sa.inv2kf = ts.wt_inv2kf;
        OFDFT_LAUNCH(c, st, name, hvm_spec_kernel, dim3(grid_for(c->g.total)), dim3(256), 0, sa);
        const double inv_n = 1.0 / (double)c->npts;
        for (int b0 = 0; b0 < ns; b0 += kBsBatch)
            if (int rc = irfftn_internal_multi(c, spec + b0, fout + b0, std::min(kBsBatch, ns - b0), inv_n, st)) return rc;
        return 0;
    }
};

// `first` = n (or phi), `dir` = w (or d), `out` = hv (or H d before the shift).  The caller has run begin_call and the argument checks.
int hvp_core(ofdft_ctx* c, const real* first, const real* dir, real* out, double* quad_terms, bool reuse, HvpChi* chi, hipStream_t st) {
    const unsigned mask = c->mask;
    const real* den = first;
    const real* w = dir;
    const long long npts = c->npts;
    const double inv_n = 1.0 / (double)npts;
    const bool has_h = mask & OFDFT_HARTREE, has_vw = mask & OFDFT_VW, has_wt = mask & OFDFT_WT_NL;
    const bool has_gga = mask & (OFDFT_PBE_X | OFDFT_PBE_C);         // (hvp_checks let it through: OFDFT_OPT_HVP_GGA = 1)
    const bool has_wgc = mask & OFDFT_WGC99_NL;                      // (... OFDFT_OPT_HVP_WGC = 1)

    double nel = c->hvp_nel;
    if (chi) {
        nel = chi->nel;                    // sum n dV = N by construction
    } else if ((has_wt || has_wgc) && !reuse) {      // n0 = mean(den) vol of THIS density: a constant of the differentiation
                                                     // (functionals.py:646-647; WGC99 rounds it, :952-954)
        double nsum;
        if (int rc = device_sum(c, den, false, &nsum, st)) return rc;
        nel = nsum * inv_n * c->vol;
    }
    const TermScalars ts = term_scalars(c, nel);
    const bool two = has_wt && ts.nlp.two;

    SpecStage stage;
    real *vh = nullptr, *lap = nullptr, *dlap = nullptr, *A = nullptr, *Cb = nullptr, *B = nullptr, *Ca = nullptr;
    auto item = [&](const real* in, const char* sname, int o, real* out_) -> int {
        cplx* s;
        if (int rc = spec_ws(c, sname, &s)) return rc;
        stage.add(in, s, o, out_);
        return 0;
    };
    if (has_h || (chi && has_gga))
        if (int rc = real_ws(c, "hv:vh", &vh)) return rc;
    if (has_h)
        if (int rc = item(chi ? vh : w, "s0", SPEC_HARTREE, vh)) return rc;      // chi space: the head writes dn into "hv:vh"; transformed in place
    // PBE: grad n ("hv:gn0..2", density-only: retained), grad w -> flux ("hv:gw0..2"), the mid kernel's pointwise part and div flux
    real *gn[3] = {}, *gw[3] = {}, *gpw = nullptr, *gdiv = nullptr, *nfield = nullptr;
    if (has_gga) {
        static const char* const gn_name[3] = {"hv:gn0", "hv:gn1", "hv:gn2"};
        static const char* const gw_name[3] = {"hv:gw0", "hv:gw1", "hv:gw2"};
        for (int a = 0; a < 3; ++a) {
            if (int rc = real_ws(c, gn_name[a], &gn[a])) return rc;
            if (int rc = real_ws(c, gw_name[a], &gw[a])) return rc;
        }
        if (int rc = real_ws(c, "hv:gpw", &gpw)) return rc;
        if (int rc = real_ws(c, "hv:gdiv", &gdiv)) return rc;
        if (chi)
            if (int rc = real_ws(c, "hv:gn", &nfield)) return rc;                // chi space: the head writes n here for its transform
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
    if (has_vw || has_wt || (chi && (has_h || has_gga))) {
        HvpChiHeadArgs ha{};
        ha.n = den;
        ha.w = w;
        ha.chi = lap;  ha.dchi = dlap;
        ha.pb = A;     ha.pbw = Cb;
        ha.pa = B;     ha.paw = Ca;
        ha.npts = npts;
        ha.al = ts.nlp.al;
        ha.be = ts.nlp.be;
        ha.flags = (has_vw ? HVP_VW : 0) | (has_wt ? HVP_WT : 0) | (two ? HVP_WT2 : 0) | (reuse ? HVP_REUSE : 0);
        if (chi) {
            ha.cs = chi->cs;
            ha.k = 2.0 * chi->a / chi->S;
            ha.dn = vh;
            ha.nout = nfield;
            OFDFT_LAUNCH(c, st, "hvp_head", hvp_head_kernel<HvpChiHeadArgs>, dim3(grid_for(npts / 2 + 1)), dim3(256), 0, ha);
        } else {
            OFDFT_LAUNCH(c, st, "hvp_head", hvp_head_kernel<HvpHeadArgs>, dim3(grid_for(npts / 2 + 1)), dim3(256), 0, (HvpHeadArgs)ha);
        }
    }
    double gga_sums[kHvpGgaScalars] = {0.0, 0.0};
    if (has_gga) {
        // stage 1: n^ (not with reuse) and w^ -> their gradients; stage 2 behind the mid kernel: the three flux fields -> div flux.
        // It runs in front of the batch below: in chi space that batch transforms "hv:vh" (dn) in place, and this one reads it.
        const real* wsrc = chi ? vh : w;
        const real* nsrc = chi ? nfield : den;
        cplx *sw[4], *sn[4];
        static const char* const sw_name[4] = {"sg:w", "s1", "s2", "s3"};
        static const char* const sn_name[4] = {"sg:n", "sg:n0", "sg:n1", "sg:n2"};
        for (int a = 0; a < 4; ++a) {
            if (int rc = spec_ws(c, sw_name[a], &sw[a])) return rc;
            if (!reuse)
                if (int rc = spec_ws(c, sn_name[a], &sn[a])) return rc;
        }
        const real* gin[2] = {wsrc, nsrc};
        cplx* gsp[2] = {sw[0], reuse ? nullptr : sn[0]};
        if (int rc = rfftn_internal_multi(c, gin, gsp, reuse ? 1 : 2, st)) return rc;
        const int sp_grid = grid_for(c->g.total);
        OFDFT_LAUNCH(c, st, "spec_grad", spec_grad_kernel, dim3(sp_grid), dim3(256), 0, (const cplx*)sw[0], sw[1], sw[2], sw[3], c->kg);
        cplx* isp[6] = {sw[1], sw[2], sw[3], nullptr, nullptr, nullptr};
        real* iout[6] = {gw[0], gw[1], gw[2], gn[0], gn[1], gn[2]};
        int ni = 3;
        if (!reuse) {
            OFDFT_LAUNCH(c, st, "spec_grad", spec_grad_kernel, dim3(sp_grid), dim3(256), 0, (const cplx*)sn[0], sn[1], sn[2], sn[3], c->kg);
            for (int a = 0; a < 3; ++a) isp[ni++] = sn[1 + a];
        }
        for (int b0 = 0; b0 < ni; b0 += kBsBatch)
            if (int rc = irfftn_internal_multi(c, isp + b0, iout + b0, std::min(kBsBatch, ni - b0), inv_n, st)) return rc;
        HvpChiGgaMidArgs ma{};
        ma.n = den;
        ma.w = w;
        for (int a = 0; a < 3; ++a) {
            ma.gn[a] = gn[a];
            ma.gw[a] = gw[a];
        }
        ma.pw = gpw;
        ma.npts = npts;
        ma.x = (mask & OFDFT_PBE_X) ? 1 : 0;
        ma.c = (mask & OFDFT_PBE_C) ? 1 : 0;
        const int mblocks = grid_for(npts / 2 + 1, kRedThreads, kRedBlocks);
        if (chi) {
            ma.cs = chi->cs;
            ma.k = 2.0 * chi->a / chi->S;
            OFDFT_LAUNCH(c, st, "hvp_gga_mid", hvp_gga_mid_kernel<HvpChiGgaMidArgs>, dim3(mblocks), dim3(kRedThreads), 0, ma, c->d_partial);
        } else {
            OFDFT_LAUNCH(c, st, "hvp_gga_mid", hvp_gga_mid_kernel<HvpGgaMidArgs>, dim3(mblocks), dim3(kRedThreads), 0, (HvpGgaMidArgs)ma, c->d_partial);
            if (quad_terms)            // (before the combine kernel takes the partial buffer)
                if (int rc = fetch_partials(c, mblocks, kHvpGgaScalars, gga_sums, st)) return rc;
        }
        const real* fl[3] = {gw[0], gw[1], gw[2]};
        if (int rc = rfftn_internal_multi(c, fl, sw + 1, 3, st)) return rc;
        OFDFT_LAUNCH(c, st, "spec_div", spec_div_kernel, dim3(sp_grid), dim3(256), 0, (const cplx*)sw[1], (const cplx*)sw[2], (const cplx*)sw[3], sw[0],
                     c->kg);
        if (int rc = irfftn_internal_multi(c, sw, &gdiv, 1, inv_n, st)) return rc;
    }
    // WGC99: four triples through the evaluation's tables and mix, each in place; U and G (density-only) are retained.  Behind the PBE
    // stage, whose pointwise field the tail adds to; the spectra are transient and leave "s0" to ofdft_precondition.
    double wgc_sum[kHvpWgcScalars] = {0.0};
    real* whv = nullptr;
    if (has_wgc) {
        static const char* const fname[4][3] = {{"hv:wU0", "hv:wU1", "hv:wU2"}, {"hv:wG0", "hv:wG1", "hv:wG2"},
                                                {"hv:wa0", "hv:wa1", "hv:wa2"}, {"hv:wp0", "hv:wp1", "hv:wp2"}};
        static const char* const sname[3] = {"s1", "s2", "s3"};
        real* f[4][3];
        cplx* sp[3];
        for (int t = 0; t < 4; ++t)
            for (int j = 0; j < 3; ++j)
                if (int rc = real_ws(c, fname[t][j], &f[t][j])) return rc;
        for (int j = 0; j < 3; ++j)
            if (int rc = spec_ws(c, sname[j], &sp[j])) return rc;
        double nref;
        if (int rc = ensure_wgc_tables(c, ts.nel_r, st, &nref)) return rc;
        HvpChiWgcArgs wa{};
        wa.n = den;
        wa.w = w;
        for (int j = 0; j < 3; ++j) {
            wa.a[j] = f[0][j];
            wa.p[j] = f[1][j];
            wa.da[j] = f[2][j];
            wa.dp[j] = f[3][j];
        }
        whv = has_gga ? gpw : f[2][0];       // without PBE the tail writes over its first direction field
        wa.add = has_gga ? gpw : nullptr;
        wa.out = whv;
        wa.npts = npts;
        wa.al = c->params[OFDFT_P_WGC_ALPHA];
        wa.be = c->params[OFDFT_P_WGC_BETA];
        wa.nref = nref;
        wa.flags = reuse ? HVP_REUSE : 0;
        if (chi) {
            wa.cs = chi->cs;
            wa.k = 2.0 * chi->a / chi->S;
            OFDFT_LAUNCH(c, st, "hvp_wgc_head", hvp_wgc_head_kernel<HvpChiWgcArgs>, dim3(grid_for(npts / 2 + 1)), dim3(256), 0, wa);
        } else {
            OFDFT_LAUNCH(c, st, "hvp_wgc_head", hvp_wgc_head_kernel<HvpWgcArgs>, dim3(grid_for(npts / 2 + 1)), dim3(256), 0, (HvpWgcArgs)wa);
        }
        const MixWgc mix = wgc_tab(c);
        for (int t = reuse ? 2 : 0; t < 4; ++t) {
            if (int rc = rfftn_internal_multi(c, f[t], sp, 3, st)) return rc;
            OFDFT_LAUNCH(c, st, "spec_wgc_mix", spec_wgc_mix_kernel, dim3(grid_for(c->g.total)), dim3(256), 0, sp[0], sp[1], sp[2], mix.t01, mix.t2,
                         mix.ck, c->g.total);
            if (int rc = irfftn_internal_multi(c, sp, f[t], 3, inv_n, st)) return rc;
        }
        const int wblocks = grid_for(npts / 2 + 1, kRedThreads, kRedBlocks);
        if (chi) {
            OFDFT_LAUNCH(c, st, "hvp_wgc_tail", hvp_wgc_tail_kernel<HvpChiWgcArgs>, dim3(wblocks), dim3(kRedThreads), 0, wa, c->d_partial);
        } else {
            OFDFT_LAUNCH(c, st, "hvp_wgc_tail", hvp_wgc_tail_kernel<HvpWgcArgs>, dim3(wblocks), dim3(kRedThreads), 0, (HvpWgcArgs)wa, c->d_partial);
            if (quad_terms)            // (before the combine kernel takes the partial buffer)
                if (int rc = fetch_partials(c, wblocks, kHvpWgcScalars, wgc_sum, st)) return rc;
        }
    }
    if (int rc = stage.run(c, ts, "hvp_spec", st)) return rc;
    HvpChiCombineArgs ca{};
    ca.n = den;
    ca.w = w;
    ca.vh = vh ? vh : den;
    ca.lap = lap ? lap : den;
    ca.dlap = dlap ? dlap : den;
    ca.A = A ? A : den;
    ca.Cb = Cb ? Cb : den;
    ca.B = B ? B : den;
    ca.Ca = Ca ? Ca : den;
    ca.hv = out;
    ca.npts = npts;
    ca.mask = mask;
    ca.two = two ? 1 : 0;
    ca.al = ts.nlp.al;
    ca.be = ts.nlp.be;
    ca.gpw = gpw;
    ca.gdiv = gdiv;
    ca.whv = whv;
    const int blocks = grid_for(npts / 2 + 1, kRedThreads, kRedBlocks);
    if (chi) {
        ca.g = chi->g;
        ca.cs = chi->cs;
        ca.k = 2.0 * chi->a / chi->S;
        ca.c2 = 2.0 * chi->cs * c->dV;
        if (has_gga)
            OFDFT_LAUNCH(c, st, "hvp_combine", (hvp_combine_kernel<HvpChiCombineArgs, true>), dim3(blocks), dim3(kRedThreads), 0, ca, c->d_partial);
        else if (has_wgc)
            OFDFT_LAUNCH(c, st, "hvp_combine", (hvp_combine_kernel<HvpChiCombineArgs, false, true>), dim3(blocks), dim3(kRedThreads), 0, ca,
                         c->d_partial);
        else
            OFDFT_LAUNCH(c, st, "hvp_combine", hvp_combine_kernel<HvpChiCombineArgs>, dim3(blocks), dim3(kRedThreads), 0, ca, c->d_partial);
        OFDFT_REDUCE(c, st, c->d_partial, blocks, kHvpChiScalars, c->d_reduced);
        OFDFT_LAUNCH(c, st, "hvp_chi_shift", hvp_chi_shift_kernel, dim3(grid_for(npts / 2 + 1)), dim3(256), 0, first, out, npts,
                     (const acc_t*)c->d_reduced, (real)c->dV, (real)(1.0 / chi->nel), ca.c2);
        if (chi->want) HIP_TRY(c, hipMemcpyAsync(c->h_partial, c->d_reduced, sizeof(double) * kHvpChiScalars, hipMemcpyDeviceToHost, st));
    } else {
        if (has_gga)
            OFDFT_LAUNCH(c, st, "hvp_combine", (hvp_combine_kernel<HvpCombineArgs, true>), dim3(blocks), dim3(kRedThreads), 0, (HvpCombineArgs)ca,
                         c->d_partial);
        else if (has_wgc)
            OFDFT_LAUNCH(c, st, "hvp_combine", (hvp_combine_kernel<HvpCombineArgs, false, true>), dim3(blocks), dim3(kRedThreads), 0,
                         (HvpCombineArgs)ca, c->d_partial);
        else
            OFDFT_LAUNCH(c, st, "hvp_combine", hvp_combine_kernel<HvpCombineArgs>, dim3(blocks), dim3(kRedThreads), 0, (HvpCombineArgs)ca, c->d_partial);
        if (quad_terms) {
            double sums[kHvpScalars];
            if (int rc = fetch_partials(c, blocks, kHvpCombineScalars, sums, st)) return rc;
            for (int s = 0; s < kHvpGgaScalars; ++s) sums[kHvpCombineScalars + s] = gga_sums[s];       // bits 10, 11: pbe_x, pbe_c
            sums[5] = wgc_sum[0];                                                                      // bit 5: wgc99_nl (the tail kernel)
            for (int t = 0; t < OFDFT_NTERMS; ++t) quad_terms[t] = (t < kHvpScalars && ((mask >> t) & 1)) ? sums[t] * c->dV : 0.0;
        }
    }
    if (int rc = end_call(c, st)) return rc;
    if (chi && chi->want)
        for (int s = 0; s < kHvpChiScalars; ++s) chi->sums[s] = c->h_partial[s];
    c->hvp_valid = chi ? kHvpChi : kHvpDensity;
    c->hvp_nel = nel;
    return OFDFT_OK;
}

// the checks both entries share, after begin_call; `who` names the entry in the messages
int hvp_checks(ofdft_ctx* c, const char* who, HvpCaller caller) {
    if (!c->mask) return fail(c, OFDFT_ESTATE, "ofdft_set_terms has not been called");
    if (c->nranks > 1) return fail(c, OFDFT_EINVAL, "%s is served by single-GPU contexts: slab-decomposed contexts have no second derivative", who);
    if (const char* name = hvp_refusal(c, caller)) return fail(c, OFDFT_EINVAL, "%s: no second derivative of the term %s", who, name);
    if (wts_active(c))
        return fail(c, OFDFT_EINVAL, "%s: no second derivative of the stabilised Wang-Teter style functional (OFDFT_P_WTS_KIND = 1, wts_kind)", who);
    return 0;
}

}  // namespace

int ofdft_hessian_vector(ofdft_ctx* c, const void* den_dev, const void* dir_dev, void* hv_dev, double* quad_terms, int reuse_density,
                         void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!c) return OFDFT_EINVAL;
    OFDFT_ON_DEVICE(c, c->device);
    const bool retained = c->hvp_valid == kHvpDensity;
    if (int rc = begin_call(c, st)) return rc;         // (clears hvp_valid: a failed call leaves nothing to reuse)
    if (!den_dev || !dir_dev || !hv_dev) return fail(c, OFDFT_EINVAL, "null argument");
    if (int rc = hvp_checks(c, "ofdft_hessian_vector", kHvpGga)) return rc;
    if (reuse_density && !retained)
        return fail(c, OFDFT_ESTATE, "ofdft_hessian_vector: reuse_density = 1 without a preceding call with reuse_density = 0 on this cell and term set");
    return hvp_core(c, (const real*)den_dev, (const real*)dir_dev, (real*)hv_dev, quad_terms, reuse_density != 0, nullptr, st);
}

// H d in chi space (include/ofdft_hip.h): the derivative of the closure gradient g = 2 c phi (v - mu) dV along d.
int ofdft_hessian_vector_chi(ofdft_ctx* c, const void* chi_dev, const void* dir_dev, const void* g_dev, double n_electrons, void* out_dev,
                             double* scalars_host, int reuse_density, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!c) return OFDFT_EINVAL;
    OFDFT_ON_DEVICE(c, c->device);
    const bool retained = c->hvp_valid == kHvpChi;
    const double S_kept = c->hvp_chi_S;
    if (int rc = begin_call(c, st)) return rc;
    if (!chi_dev || !dir_dev || !out_dev) return fail(c, OFDFT_EINVAL, "null argument");
    if (!(n_electrons > 0.0)) return fail(c, OFDFT_EINVAL, "ofdft_hessian_vector_chi: n_electrons must be positive");
    if (int rc = hvp_checks(c, "ofdft_hessian_vector_chi", kHvpGga)) return rc;
    if (reuse_density && !retained)
        return fail(c, OFDFT_ESTATE, "ofdft_hessian_vector_chi: reuse_density = 1 without a preceding call with reuse_density = 0 on this cell and term set");
    const real* phi = (const real*)chi_dev;
    const real* d = (const real*)dir_dev;
    // a = phi.d (and S = phi.phi of a new phi): the head kernel needs both before it can form dn
    const int blocks = grid_for(c->npts / 2 + 1, kRedThreads, kRedBlocks);
    OFDFT_LAUNCH(c, st, "hvp_chi_dots", hvp_chi_dots_kernel, dim3(blocks), dim3(kRedThreads), 0, phi, d, c->npts, c->d_partial);
    double pre[2];
    if (int rc = fetch_partials(c, blocks, 2, pre, st)) return rc;
    HvpChi x{};
    x.g = (const real*)g_dev;
    x.nel = n_electrons;
    x.a = pre[0];
    x.S = reuse_density ? S_kept : pre[1];
    if (!(x.S > 0.0)) return fail(c, OFDFT_EINVAL, "ofdft_hessian_vector_chi: chi is zero everywhere");
    x.cs = n_electrons / (x.S * c->dV);
    x.want = scalars_host != nullptr;
    if (int rc = hvp_core(c, phi, d, (real*)out_dev, nullptr, reuse_density != 0, &x, st)) return rc;
    c->hvp_chi_S = x.S;
    if (scalars_host) {
        const double dmu = (x.sums[0] * c->dV + x.sums[1]) / n_electrons, c2 = 2.0 * x.cs * c->dV;
        scalars_host[0] = x.sums[2] - c2 * dmu * x.a;      // d . H d
        scalars_host[1] = x.sums[3] - c2 * dmu * x.S;      // phi . H d
        scalars_host[2] = x.a;
        scalars_host[3] = x.S;
        scalars_host[4] = dmu;
    }
    return OFDFT_OK;
}

// ---- several columns per call (include/ofdft_hip.h) ------------------------------------------------------------
namespace {

// Workspaces of the multi entries.  The density-side fields ("hv:lap", "hv:A", "hv:B" and their spectra) are the ones the
// single-column entries write: that is what lets either entry reuse the other's.  The per-direction fields are per column: column
// 0 takes the single-column workspaces under their own names ("hv:vh", "s0", ...), column j > 0 the same name with "#j" appended.
void col_name(char (&name)[32], const char* base, int j) {
    if (j) std::snprintf(name, sizeof(name), "%s#%d", base, j);
    else std::snprintf(name, sizeof(name), "%s", base);
}
int real_ws_col(ofdft_ctx* c, const char* base, int j, real** out) {
    char name[32];
    col_name(name, base, j);
    return real_ws(c, name, out);
}
int spec_ws_col(ofdft_ctx* c, const char* base, int j, cplx** out) {
    char name[32];
    col_name(name, base, j);
    return spec_ws(c, name, out);
}

#define HVM_CASE(NC, ...) \
    case NC: {            \
        constexpr int kNC = NC; \
        __VA_ARGS__;      \
    } break;
// runs the statement with kNC = nc as a compile-time constant (1 .. kMultiMax)
#define HVM_DISPATCH(nc, ...)                                                                                                       \
    switch (nc) {                                                                                                                   \
        HVM_CASE(1, __VA_ARGS__) HVM_CASE(2, __VA_ARGS__) HVM_CASE(3, __VA_ARGS__) HVM_CASE(4, __VA_ARGS__) HVM_CASE(5, __VA_ARGS__) \
        HVM_CASE(6, __VA_ARGS__) HVM_CASE(7, __VA_ARGS__) HVM_CASE(8, __VA_ARGS__)                                                  \
    }
static_assert(kMultiMax == 8 && OFDFT_MULTI_MAX == kMultiMax, "HVM_DISPATCH lists the column counts");

// [a, a + na) and [b, b + nb) share an element
bool ranges_overlap(const real* a, long long na, const real* b, long long nb) { return a < b + nb && b < a + na; }

// the argument checks the two multi entries share; `who` names the entry
int multi_checks(ofdft_ctx* c, const char* who, int ncols, long long in_stride, long long out_stride) {
    if (ncols < 1 || ncols > kMultiMax)
        return fail(c, OFDFT_EINVAL, "%s: ncols = %d is outside 1 .. %d (OFDFT_MULTI_MAX)", who, ncols, kMultiMax);
    if (in_stride < c->npts || out_stride < c->npts)
        return fail(c, OFDFT_EINVAL, "%s: a column stride (%lld in, %lld out) is below the %lld points of a column", who, in_stride, out_stride,
                    c->npts);
    return 0;
}

}  // namespace

int ofdft_hessian_vector_chi_multi(ofdft_ctx* c, const void* chi_dev, const void* dirs_dev, long long dir_stride, int ncols, double n_electrons,
                                   void* out_dev, long long out_stride, double* scalars_host, int reuse_density, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!c) return OFDFT_EINVAL;
    OFDFT_ON_DEVICE(c, c->device);
    const char* who = "ofdft_hessian_vector_chi_multi";
    const bool retained = c->hvp_valid == kHvpChi;         // (the chi-space fields of either entry)
    const double S_kept = c->hvp_chi_S;
    if (int rc = begin_call(c, st)) return rc;
    if (!chi_dev || !dirs_dev || !out_dev) return fail(c, OFDFT_EINVAL, "null argument");
    if (int rc = multi_checks(c, who, ncols, dir_stride, out_stride)) return rc;
    if (!(n_electrons > 0.0)) return fail(c, OFDFT_EINVAL, "%s: n_electrons must be positive", who);
    if (int rc = hvp_checks(c, who, kHvpNoGga)) return rc;
    const long long npts = c->npts;
    const real* phi = (const real*)chi_dev;
    const real* d = (const real*)dirs_dev;
    real* out = (real*)out_dev;
    if (ranges_overlap(d, (ncols - 1) * dir_stride + npts, out, (ncols - 1) * out_stride + npts))
        return fail(c, OFDFT_EINVAL, "%s: out_dev overlaps dirs_dev (the product is not in place)", who);
    if (reuse_density && !retained)
        return fail(c, OFDFT_ESTATE, "%s: reuse_density = 1 without a preceding call with reuse_density = 0 on this cell and term set", who);
    const bool reuse = reuse_density != 0;
    const unsigned mask = c->mask;
    const bool has_h = mask & OFDFT_HARTREE, has_vw = mask & OFDFT_VW, has_wt = mask & OFDFT_WT_NL;
    const TermScalars ts = term_scalars(c, n_electrons);
    const bool two = has_wt && ts.nlp.two;

    // a_j = phi.d_j of every column and S: one sweep, one fetch
    const int blocks = grid_for(npts / 2 + 1, kRedThreads, kRedBlocks);
    HVM_DISPATCH(ncols, OFDFT_LAUNCH(c, st, "hvm_dots", hvm_dots_kernel<kNC>, dim3(blocks), dim3(kRedThreads), 0, phi, d, dir_stride, npts, c->d_partial));
    double pre[kMultiMax + 1];
    if (int rc = fetch_partials(c, blocks, ncols + 1, pre, st)) return rc;
    const double S = reuse ? S_kept : pre[ncols];
    if (!(S > 0.0)) return fail(c, OFDFT_EINVAL, "%s: chi is zero everywhere", who);
    const double cs = n_electrons / (S * c->dV), c2 = 2.0 * cs * c->dV;

    // the density-only items first; every field is transformed in place
    SpecStage stage;
    auto item = [&](real* field, cplx* s, int o) { stage.add(field, s, o, field); };
    real *lap = nullptr, *A = nullptr, *B = nullptr;
    real *vh[kMultiMax] = {}, *dlap[kMultiMax] = {}, *Cb[kMultiMax] = {}, *Ca[kMultiMax] = {};
    cplx* s;
    if (has_vw) {
        if (int rc = real_ws(c, "hv:lap", &lap)) return rc;
        if (!reuse) {
            if (int rc = spec_ws(c, "svw", &s)) return rc;
            item(lap, s, SPEC_LAPLACE);
        }
    }
    if (has_wt) {
        if (int rc = real_ws(c, "hv:A", &A)) return rc;
        if (!reuse) {
            if (int rc = spec_ws(c, "swb", &s)) return rc;
            item(A, s, SPEC_LINDHARD);
        }
        if (two) {
            if (int rc = real_ws(c, "hv:B", &B)) return rc;
            if (!reuse) {
                if (int rc = spec_ws(c, "swa", &s)) return rc;
                item(B, s, SPEC_LINDHARD);
            }
        }
    }
    for (int j = 0; j < ncols; ++j) {
        if (has_h) {            // the head writes dn_j into "hv:vh"; transformed in place
            if (int rc = real_ws_col(c, "hv:vh", j, &vh[j])) return rc;
            if (int rc = spec_ws_col(c, "s0", j, &s)) return rc;
            item(vh[j], s, SPEC_HARTREE);
        }
        if (has_vw) {
            if (int rc = real_ws_col(c, "hv:dlap", j, &dlap[j])) return rc;
            if (int rc = spec_ws_col(c, "s1", j, &s)) return rc;
            item(dlap[j], s, SPEC_LAPLACE);
        }
        if (has_wt) {
            if (int rc = real_ws_col(c, "hv:Cb", j, &Cb[j])) return rc;
            if (int rc = spec_ws_col(c, "s2", j, &s)) return rc;
            item(Cb[j], s, SPEC_LINDHARD);
            if (two) {
                if (int rc = real_ws_col(c, "hv:Ca", j, &Ca[j])) return rc;
                if (int rc = spec_ws_col(c, "s3", j, &s)) return rc;
                item(Ca[j], s, SPEC_LINDHARD);
            }
        }
    }
    if (stage.ns) {
        HvmHeadArgs ha{};
        ha.phi = phi;
        ha.d = d;
        ha.stride = dir_stride;
        ha.npts = npts;
        ha.chi = lap;
        ha.pb = A;
        ha.pa = B;
        for (int j = 0; j < ncols; ++j) {
            ha.dn[j] = vh[j];
            ha.dchi[j] = dlap[j];
            ha.pbw[j] = Cb[j];
            ha.paw[j] = Ca[j];
            ha.k[j] = 2.0 * pre[j] / S;
        }
        ha.cs = cs;
        ha.al = ts.nlp.al;
        ha.be = ts.nlp.be;
        ha.flags = (has_vw ? HVP_VW : 0) | (has_wt ? HVP_WT : 0) | (two ? HVP_WT2 : 0) | (reuse ? HVP_REUSE : 0);
        HVM_DISPATCH(ncols, OFDFT_LAUNCH(c, st, "hvm_head", hvm_head_kernel<kNC>, dim3(grid_for(npts / 2 + 1)), dim3(256), 0, ha));
    }
    if (int rc = stage.run(c, ts, "hvm_spec", st)) return rc;
    HvmCombineArgs ca{};
    ca.phi = phi;
    ca.d = d;
    ca.dstride = dir_stride;
    ca.lap = lap;
    ca.A = A;
    ca.B = B;
    for (int j = 0; j < ncols; ++j) {
        ca.vh[j] = vh[j];
        ca.dlap[j] = dlap[j];
        ca.Cb[j] = Cb[j];
        ca.Ca[j] = Ca[j];
        ca.k[j] = 2.0 * pre[j] / S;
    }
    ca.out = out;
    ca.ostride = out_stride;
    ca.npts = npts;
    ca.mask = mask;
    ca.two = two ? 1 : 0;
    ca.al = ts.nlp.al;
    ca.be = ts.nlp.be;
    ca.cs = cs;
    ca.c2 = c2;
    const int nsum = kHvpMultiScalars * ncols;
    HVM_DISPATCH(ncols, OFDFT_LAUNCH(c, st, "hvm_combine", hvm_combine_kernel<kNC>, dim3(blocks), dim3(kRedThreads), 0, ca, c->d_partial));
    OFDFT_REDUCE(c, st, c->d_partial, blocks, nsum, c->d_reduced);
    OFDFT_LAUNCH(c, st, "hvm_shift", hvm_shift_kernel, dim3(grid_for(npts / 2 + 1)), dim3(256), 0, phi, out, out_stride, ncols, npts,
                 (const acc_t*)c->d_reduced, (real)c->dV, (real)(1.0 / n_electrons), (real)c2);
    if (scalars_host) HIP_TRY(c, hipMemcpyAsync(c->h_partial, c->d_reduced, sizeof(double) * nsum, hipMemcpyDeviceToHost, st));
    if (int rc = end_call(c, st)) return rc;
    c->hvp_valid = kHvpChi;
    c->hvp_nel = n_electrons;
    c->hvp_chi_S = S;
    if (scalars_host)
        for (int j = 0; j < ncols; ++j) {
            const double* sums = c->h_partial + kHvpMultiScalars * j;
            const double dmu = sums[0] * c->dV / n_electrons;
            double* o = scalars_host + OFDFT_HVC_NSCALARS * j;
            o[OFDFT_HVC_DHD] = sums[1] - c2 * dmu * pre[j];
            o[OFDFT_HVC_PHIHD] = sums[2] - c2 * dmu * S;
            o[OFDFT_HVC_A] = pre[j];
            o[OFDFT_HVC_S] = S;
            o[OFDFT_HVC_DMU] = dmu;
        }
    return OFDFT_OK;
}

// z_j = irfftn(rfftn(r_j) / (k^2 + kappa2)) for ncols columns: the kinetic preconditioner of the conjugate gradients
// (include/ofdft_hip.h).  The solver calls it between products that run with reuse_density = 1, so the entries go
// round begin_call, like the first-order ion entries (engine_ions_stress.inc.h): hvp_valid and hvp_chi_S stay, which is sound
// because the workspaces it takes are the spectra "s0", "s0#1", ..., transient in every product, and no "hv:*" field.
namespace {

// the checks both entries share; `who` names the entry
int precondition_checks(ofdft_ctx* c, const char* who, const void* r_dev, const void* z_dev) {
    if (c->nranks > 1) return fail(c, OFDFT_EINVAL, "%s is served by single-GPU contexts: slab-decomposed contexts have no preconditioner", who);
    if (!c->cell_set) return fail(c, OFDFT_ESTATE, "ofdft_set_cell has not been called");
    if (!r_dev || !z_dev) return fail(c, OFDFT_EINVAL, "null argument");
    return 0;
}
bool kappa2_ok(double kappa2) { return kappa2 > 0.0 && std::isfinite(kappa2); }

// The three pipelines, `kBsBatch` columns at a time where a pass takes several fields (the chirp-z helpers), one column per launch
// through the fused radix passes; one synchronisation at the end.  One column enqueues one transform's launches.
int precondition_columns(ofdft_ctx* c, const real* r, long long r_stride, real* z, long long z_stride, int ncols, double kappa2, hipStream_t st) {
    const double inv_n = 1.0 / (double)c->npts;
    const MixScale<SPEC_SCREENED> mix{c->kg, (real)kappa2, (real)0.0};
    cplx* sp[kBsBatch];
    for (int a = 0; a < std::min(kBsBatch, ncols); ++a)
        if (int rc = spec_ws_col(c, "s0", a, &sp[a])) return rc;
    for (int j0 = 0; j0 < ncols; j0 += kBsBatch) {
        const int nb = std::min(kBsBatch, ncols - j0);
        const real* in[kBsBatch];
        real* out[kBsBatch];
        for (int a = 0; a < nb; ++a) {
            in[a] = r + (j0 + a) * r_stride;
            out[a] = z + (j0 + a) * z_stride;
        }
        if (c->fast && !c->force_unfused) {            // z + y | x with the multiply inside | y + z: five spectrum passes
            for (int a = 0; a < nb; ++a) {
                if (int rc = fwd_zy(c, in[a], sp[a], st)) return rc;
                XfIo io{};
                io.in[0] = sp[a];
                io.out[0] = sp[a];
                if (int rc = xfused<1, 1>(c, io, mix, st, "xfused_pre")) return rc;
                if (int rc = inv_yz(c, sp[a], out[a], inv_n, st)) return rc;
            }
        } else if (bluestein_xmix_ok(c) && !c->force_unfused) {      // chirp-z extents: the same shape around the x-mix kernel
            if (int rc = bluestein_fwd_zy_multi(c, in, sp, nb, st)) return rc;
            for (int a = 0; a < nb; ++a)
                if (int rc = bluestein_xmix<1, 1>(c, sp + a, sp + a, mix, st)) return rc;
            if (int rc = bluestein_inv_yz_multi(c, sp, out, nb, inv_n, st)) return rc;
        } else {                                       // forward, multiply, inverse: seven passes
            if (int rc = rfftn_internal_multi(c, in, sp, nb, st)) return rc;
            for (int a = 0; a < nb; ++a)
                OFDFT_LAUNCH(c, st, "spec_scale", (spec_scale_kernel<SPEC_SCREENED>), dim3(grid_for(c->g.total)), dim3(256), 0, (const cplx*)sp[a],
                             sp[a], c->kg, (real)kappa2, (real)0.0);
            if (int rc = irfftn_internal_multi(c, sp, out, nb, inv_n, st)) return rc;
        }
    }
    HIP_TRY(c, hipStreamSynchronize(st));
    HIP_TRY(c, hipGetLastError());
    if (c->profiling) prof_collect(c);
    return OFDFT_OK;
}

}  // namespace

int ofdft_precondition(ofdft_ctx* c, const void* r_dev, void* z_dev, double kappa2, void* stream) {
    if (!c) return OFDFT_EINVAL;
    OFDFT_ON_DEVICE(c, c->device);
    if (int rc = precondition_checks(c, "ofdft_precondition", r_dev, z_dev)) return rc;
    if (!kappa2_ok(kappa2)) return fail(c, OFDFT_EINVAL, "ofdft_precondition: kappa2 must be positive and finite");
    if (z_dev == r_dev) return fail(c, OFDFT_EINVAL, "ofdft_precondition: z_dev must not be r_dev (the transform is not in place)");
    return precondition_columns(c, (const real*)r_dev, c->npts, (real*)z_dev, c->npts, 1, kappa2, (hipStream_t)stream);
}

int ofdft_precondition_multi(ofdft_ctx* c, const void* r_dev, long long r_stride, void* z_dev, long long z_stride, int ncols, double kappa2,
                             void* stream) {
    if (!c) return OFDFT_EINVAL;
    OFDFT_ON_DEVICE(c, c->device);
    const char* who = "ofdft_precondition_multi";
    const real* r = (const real*)r_dev;
    real* z = (real*)z_dev;
    if (int rc = precondition_checks(c, who, r_dev, z_dev)) return rc;
    if (int rc = multi_checks(c, who, ncols, r_stride, z_stride)) return rc;
    if (!kappa2_ok(kappa2)) return fail(c, OFDFT_EINVAL, "%s: kappa2 must be positive and finite", who);
    if (ranges_overlap(r, (ncols - 1) * r_stride + c->npts, z, (ncols - 1) * z_stride + c->npts))
        return fail(c, OFDFT_EINVAL, "%s: z_dev overlaps r_dev (the transform is not in place)", who);
    return precondition_columns(c, r, r_stride, z, z_stride, ncols, kappa2, (hipStream_t)stream);
}
