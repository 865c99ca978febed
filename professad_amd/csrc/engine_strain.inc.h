// C ABI of the second strain derivative at fixed chi (strain2_kernels.h): the reciprocal-space terms of the
// functional, the ion-electron term and the ion-ion sum.  Included once by engine.hip inside its extern "C" block (fp64 library),
// after engine_ions_stress.inc.h (the frames of the ion entries, moment_sums, density_power_spectrum) and engine_hvp.inc.h
// (hvp_checks).  Single GPU, exact structure factor.  Each entry clears hvp_valid, the fields ofdft_hessian_vector retains for
// reuse_density = 1: the two functional entries through begin_call, the three ion entries by the second-order convention (they
// write no "hv:*" workspace; DESIGN.md §9f has the table).  Tensors are [3][3][3][3] row-major in (m, n, p, q) =
// d2 E / d eps_mn d eps_pq, Ha.
namespace {

const int kK2Index[3][3] = {{0, 3, 4}, {3, 1, 5}, {4, 5, 2}};
int k4_index(int a, int b, int c, int d) {
    const int idx[4] = {a, b, c, d}, base[5] = {10, 6, 3, 1, 0};
    int nx = 0, ny = 0;
    for (int i : idx) {
        nx += i == 0;
        ny += i == 1;
    }
    return base[nx] + (4 - nx - ny);
}

enum { kC2bSame = 0, kC2bNone = 1, kC2bTrace = 2 };
// out[m][n][p][q] += pref * (the tensor of the 23 sums of a reciprocal-space kernel); how c2b follows from them: strain2_kernels.h
void strain2_assemble(const double* s, int c2b_kind, double pref, double* out) {
    const double *m4 = s, *m2 = s + 15, c0a = s[21], c0b = s[22];
    double m2b[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) {
            double v = 0.0;
            if (c2b_kind == kC2bSame) v = m2[kK2Index[i][j]];
            if (c2b_kind == kC2bTrace) v = -(m4[k4_index(i, j, 0, 0)] + m4[k4_index(i, j, 1, 1)] + m4[k4_index(i, j, 2, 2)]) / 3.0;
            m2b[kK2Index[i][j]] = v;
        }
    for (int m = 0; m < 3; ++m)
        for (int n = 0; n < 3; ++n)
            for (int p = 0; p < 3; ++p)
                for (int q = 0; q < 3; ++q) {
                    double v = m4[k4_index(m, n, p, q)];
                    if (n == p) v += m2[kK2Index[m][q]];
                    if (q == m) v += m2[kK2Index[p][n]];
                    if (m == p) v += m2[kK2Index[n][q]];
                    if (p == q) v += m2b[kK2Index[m][n]];
                    if (m == n) v += m2b[kK2Index[p][q]];
                    if (m == n && p == q) v += c0a + c0b;
                    if (m == q && n == p) v -= c0b;
                    out[((m * 3 + n) * 3 + p) * 3 + q] += pref * v;
                }
}

}  // namespace

// v_eps,kl (xx, yy, zz, yz, xz, xy) of the active terms at the density den: the explicit cell dependence of the potential at fixed
// grid values of the density, n0 = N / vol following the cell (strain2_kernels.h).  out6_dev [6][n0][n1][n2].  Transforms
// (OFDFT_Q_FFT_COUNT): one forward and six inverse per family -- hartree, vw, wt_nl (two families when alpha != beta).
int ofdft_potential_strain_gradient(ofdft_ctx* c, const void* den_dev, void* out6_dev, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!c) return OFDFT_EINVAL;
    OFDFT_ON_DEVICE(c, c->device);
    if (int rc = begin_call(c, st)) return rc;         // (clears hvp_valid)
    if (!den_dev || !out6_dev) return fail(c, OFDFT_EINVAL, "null argument");
    if (int rc = hvp_checks(c, "ofdft_potential_strain_gradient", kHvpNoGga)) return rc;
    const double* den = (const double*)den_dev;
    const unsigned mask = c->mask;
    const long long npts = c->npts;
    const double invN = 1.0 / (double)npts;
    unsigned flags = ((mask & OFDFT_HARTREE) ? SG_HARTREE : 0) | ((mask & OFDFT_VW) ? SG_VW : 0) | ((mask & OFDFT_WT_NL) ? SG_WT : 0);
    StrainGradSpecArgs sa{};
    sa.kg = c->kg;
    StrainGradCombineArgs ca{};
    ca.n = den;
    ca.out = (double*)out6_dev;
    ca.npts = npts;
    if (flags & SG_WT) {
        double nsum;
        if (int rc = device_sum(c, den, false, &nsum, st)) return rc;
        const TermScalars ts = term_scalars(c, nsum * c->dV);
        const WtMoment wt = wt_moment(ts, nsum * invN);
        ca.al = ts.nlp.al;
        ca.be = ts.nlp.be;
        if (ca.al != ca.be) flags |= SG_WT2;
        sa.pref = wt.pref;
        sa.inv2kf = wt.inv2kf;
        sa.q = wt.q;
    }
    sa.flags = ca.flags = flags;
    static const char* const in_names[kStrainGradFamilies] = {"sg:i0", "sg:i1", "sg:i2", "sg:i3"};
    const real* fin[kStrainGradFamilies];
    cplx* fspec[kStrainGradFamilies];
    cplx* ospec[kStrainGradFamilies * 6];
    real* ofld[kStrainGradFamilies * 6];
    real* head[kStrainGradFamilies] = {nullptr, nullptr, nullptr, nullptr};
    int nf = 0, no = 0;
    for (int f = 0; f < kStrainGradFamilies; ++f) {
        if (!(flags & (1u << f))) continue;
        cplx* s;
        if (int rc = spec_ws(c, in_names[f], &s)) return rc;
        if (f > 0)
            if (int rc = real_ws(c, in_names[f], &head[f])) return rc;
        fin[nf] = f == 0 ? den : head[f];
        fspec[nf++] = s;
        sa.in[f] = s;
        for (int k = 0; k < 6; ++k) {
            char name[16];
            snprintf(name, sizeof(name), "sg:o%d", 6 * f + k);
            if (int rc = spec_ws(c, name, &ospec[no])) return rc;
            if (int rc = real_ws(c, name, &ofld[no])) return rc;
            sa.out[6 * f + k] = ospec[no];
            ca.f[6 * f + k] = ofld[no];
            ++no;
        }
    }
    if (flags & (SG_VW | SG_WT))
        OFDFT_LAUNCH(c, st, "strain_grad_head", strain_grad_head_kernel, dim3(grid_for(npts)), dim3(256), 0, den, head[1], head[2], head[3], npts,
                     ca.al, ca.be, flags);
    if (nf) {
        if (int rc = rfftn_internal_multi(c, fin, fspec, nf, st)) return rc;                  // nf <= kBsBatch
        OFDFT_LAUNCH(c, st, "strain_grad_spec", strain_grad_spec_kernel, dim3(grid_for(c->g.total)), dim3(256), 0, sa);
        for (int b0 = 0; b0 < no; b0 += kBsBatch)
            if (int rc = irfftn_internal_multi(c, ospec + b0, ofld + b0, std::min(kBsBatch, no - b0), invN, st)) return rc;
    }
    OFDFT_LAUNCH(c, st, "strain_grad_combine", strain_grad_combine_kernel, dim3(grid_for(npts)), dim3(256), 0, ca);
    return end_call(c, st);
}

// d v_ext / d eps_kl (xx, yy, zz, yz, xz, xy) of one species at fixed fractional coordinates, with the c2r semantics of
// ofdft_ionic_potential: one spectral kernel, one batch of six inverse transforms.  out6_dev [6][n0][n1][n2].
int ofdft_ionic_potential_strain_gradient(ofdft_ctx* c, const double* frac_host, int nions, const double* tab_k, const double* tab_v,
                                          int ntab, double z_ion, int pme_order, void* out6_dev, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!c || !frac_host || !tab_k || !tab_v || !out6_dev) return OFDFT_EINVAL;
    IonPrep p(c);
    if (int rc = ion_begin(c, p, "ofdft_ionic_potential_strain_gradient", true, frac_host, nions, tab_k, tab_v, ntab, z_ion, pme_order, st))
        return rc;
    IonStrainGradOut so{};
    cplx* spec[6];
    real* out[6];
    for (int k = 0; k < 6; ++k) {
        char name[16];
        snprintf(name, sizeof(name), "sg:o%d", k);
        if (int rc = spec_ws(c, name, &spec[k])) return rc;
        so.s[k] = spec[k];
        out[k] = (real*)out6_dev + (size_t)k * c->npts;
    }
    OFDFT_LAUNCH(c, st, "ion_strain_grad_spec", ion_strain_grad_spec_kernel, dim3(grid_for(c->g.total)), dim3(256), 0, so, c->kg,
                 (const double*)p.d_cart, nions, p.tab, 1.0 / c->vol);
    for (int b0 = 0; b0 < 6; b0 += kBsBatch)
        if (int rc = irfftn_internal_multi(c, spec + b0, out + b0, std::min(kBsBatch, 6 - b0), 1.0, st)) return rc;      // norm='forward'
    return ion_finish(c, st);
}

// W2^0 of the reciprocal-space terms of the active set at the density den (n ~ 1/J under the strain): hartree, vw, wt_nl; every
// other entry of w2_terms_host [OFDFT_NTERMS][81] is zero (the pointwise terms depend on J alone and follow on the host from
// the stress trace and n.H_t n; ion_electron: ofdft_ion_electron_strain_hessian).  The refusals are ofdft_hessian_vector's.
int ofdft_strain_hessian(ofdft_ctx* c, const void* den_dev, double* w2, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!c) return OFDFT_EINVAL;
    OFDFT_ON_DEVICE(c, c->device);
    if (int rc = begin_call(c, st)) return rc;         // (clears hvp_valid)
    if (!den_dev || !w2) return fail(c, OFDFT_EINVAL, "null argument");
    if (int rc = hvp_checks(c, "ofdft_strain_hessian", kHvpNoGga)) return rc;
    const double* den = (const double*)den_dev;
    const unsigned mask = c->mask;
    const double invN = 1.0 / (double)c->npts, invN2 = invN * invN;
    for (int i = 0; i < OFDFT_NTERMS * 81; ++i) w2[i] = 0.0;
    const int sp_blocks = grid_for(c->g.total, kRedThreads, kRedBlocks);
    double s23[kStrain2Scalars];
    cplx *s0 = nullptr, *s1 = nullptr;
    if (int rc = spec_ws(c, "s0", &s0)) return rc;
    if (int rc = spec_ws(c, "s1", &s1)) return rc;
    if (mask & OFDFT_HARTREE) {         // E = (vol / 2) sum_k w 4 pi |n~ / N|^2 / (J s)
        if (int rc = rfftn_internal(c, den, s0, st)) return rc;
        OFDFT_LAUNCH(c, st, "strain2_spec", (strain2_spec_kernel<STRAIN2_HARTREE>), dim3(sp_blocks), dim3(kRedThreads), 0, (const cplx*)s0,
                     (const cplx*)nullptr, c->kg, invN2, 0.0, c->d_partial);
        if (int rc = moment_sums(c, sp_blocks, kStrain2Scalars, s23, st)) return rc;
        strain2_assemble(s23, kC2bSame, 0.5 * c->vol, w2 + 81 * 1);
    }
    if (mask & OFDFT_VW) {              // E = (vol / 2) sum_k w s |F[sqrt n] / N|^2: no J left
        if (int rc = density_power_spectrum(c, den, MAP_SQRT, 0.0, s0, st)) return rc;
        OFDFT_LAUNCH(c, st, "strain2_spec", (strain2_spec_kernel<STRAIN2_VW>), dim3(sp_blocks), dim3(kRedThreads), 0, (const cplx*)s0,
                     (const cplx*)nullptr, c->kg, invN2, 0.0, c->d_partial);
        if (int rc = moment_sums(c, sp_blocks, kStrain2Scalars, s23, st)) return rc;
        strain2_assemble(s23, kC2bNone, 0.5 * c->vol, w2 + 81 * 3);
    }
    if (mask & OFDFT_WT_NL) {           // E = vol c_TF pref sum_k w Re(a~ b~*) / N^2 J^(-2/3) F(eta); n0 = N_e / vol as ofdft_stress forms it
        double nsum;
        if (int rc = device_sum(c, den, false, &nsum, st)) return rc;
        const TermScalars ts = term_scalars(c, nsum * c->dV);
        const double al = ts.nlp.al, be = ts.nlp.be;
        const WtMoment wt = wt_moment(ts, nsum * invN);
        if (int rc = density_power_spectrum(c, den, MAP_POW, be, s0, st)) return rc;      // n^beta first, n^alpha second
        cplx* sa = s0;
        if (al != be) {
            if (int rc = density_power_spectrum(c, den, MAP_POW, al, s1, st)) return rc;
            sa = s1;
        }
        OFDFT_LAUNCH(c, st, "strain2_spec", (strain2_spec_kernel<STRAIN2_WT>), dim3(sp_blocks), dim3(kRedThreads), 0, (const cplx*)sa,
                     (const cplx*)s0, c->kg, invN2, wt.inv2kf, c->d_partial);
        if (int rc = moment_sums(c, sp_blocks, kStrain2Scalars, s23, st)) return rc;
        strain2_assemble(s23, kC2bTrace, c->vol * wt.pref_ctf, w2 + 81 * 4);
    }
    return end_call(c, st);
}

// W2^0 of the ion-electron energy of one species at fixed grid values of the density and fixed fractional coordinates, the
// potential rebuilt from the ions in the strained cell: E = (1 / N J) sum_k w Re(S_k conj(n~_k)) v~(|k|); w2_host [81].
int ofdft_ion_electron_strain_hessian(ofdft_ctx* c, const void* den_dev, const double* frac_host, int nions, const double* tab_k,
                                      const double* tab_v, int ntab, double z_ion, int pme_order, double* w2_host, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!c || !den_dev || !frac_host || !tab_k || !tab_v || !w2_host) return OFDFT_EINVAL;
    IonPrep p(c);
    if (int rc = ion_begin(c, p, "ofdft_ion_electron_strain_hessian", true, frac_host, nions, tab_k, tab_v, ntab, z_ion, pme_order, st))
        return rc;
    cplx* sN;
    if (int rc = spec_ws(c, "i:F", &sN)) return rc;
    if (int rc = rfftn_internal(c, (const double*)den_dev, sN, st)) return rc;
    const int blocks = grid_for(c->g.total, kRedThreads, kRedBlocks);
    OFDFT_LAUNCH(c, st, "strain2_ion", strain2_ion_kernel, dim3(blocks), dim3(kRedThreads), 0, (const cplx*)sN, c->kg,
                 (const double*)p.d_cart, nions, p.tab, c->d_partial);
    double s23[kStrain2Scalars];
    if (int rc = moment_sums(c, blocks, kStrain2Scalars, s23, st)) return rc;
    for (int i = 0; i < 81; ++i) w2_host[i] = 0.0;
    strain2_assemble(s23, kC2bSame, 1.0 / (double)c->npts, w2_host);
    return ion_finish(c, st);
}

// W2^0 of the ion-ion energy (ion_utils.py:293-333 with the heuristics of system.py:733-754) at fixed fractional coordinates:
// the pair sum over the fixed pair list of ofdft_ion_ion, Rd and Rc constants of the differentiation (the reference takes h_max
// from box_vecs.detach()), plus the background term, which depends on the cell through rho ~ 1/J and R_a ~ J^(1/3) alone:
// with e_a(J) = (rho / J) h(R_a J^(1/3)), h' = -2 pi Z R erfc(R / Rd), h'' = -2 pi Z erfc(R / Rd) + 4 sqrt(pi) Z R exp(-R^2 / Rd^2) / Rd,
//     E_J = rho (h' R / 3 - h),   E_JJ = rho (2 h - 8/9 h' R + h'' R^2 / 9)
// and W2 = E_J (delta_mn delta_pq - delta_mq delta_np) + E_JJ delta_mn delta_pq.  w2_host [81].
int ofdft_ion_ion_strain_hessian(ofdft_ctx* c, const double* frac_host, const double* charges_host, int nions, double Rc, double* w2_host,
                                 void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!c || !frac_host || !charges_host || !w2_host || nions < 1) return OFDFT_EINVAL;
    c->hvp_valid = false;
    IonIonCall ii;
    if (int rc = ion_ion_begin(c, ii, frac_host, nions, Rc)) return rc;
    if (c->nranks > 1) return fail(c, OFDFT_EINVAL, "ofdft_ion_ion_strain_hessian is served by single-GPU contexts");
    if (nions > 65535) return fail(c, OFDFT_EINVAL, "ofdft_ion_ion_strain_hessian: at most 65535 ions (the direct pair scan)");
    OFDFT_ON_DEVICE(c, c->device);
    const double Rd = ii.g.Rd;
    const int chunks = ion_ion_chunks(ii.nshift * nions);
    if (int rc = ion_ion_upload(c, ii, charges_host, nions, "ii:s2part", nions, chunks, kIonStrain2Scalars, st)) return rc;
    OFDFT_LAUNCH(c, st, "ion_ion_strain2", ion_ion_strain2_kernel, dim3(chunks, nions), dim3(kRedThreads), 0, (const double*)ii.d_cart,
                 (const double*)ii.d_z, nions, ii.g, ii.d_part);
    if (int rc = ion_ion_fetch(c, ii, st)) return rc;
    double ztot = 0.0;
    for (int a = 0; a < nions; ++a) ztot += charges_host[a];
    const double rho = ztot / c->vol, spi = std::sqrt(kPi);
    long double m[21], EJ = 0.0L, EJJ = 0.0L;
    for (int k = 0; k < 21; ++k) m[k] = 0.0L;
    for (int a = 0; a < nions; ++a) {
        long double s[kIonStrain2Scalars];
        for (int k = 0; k < kIonStrain2Scalars; ++k) s[k] = chunk_sum(ii.part.data(), a, chunks, kIonStrain2Scalars, k);
        for (int k = 0; k < 21; ++k) m[k] += 0.5L * s[k];
        const double Z = charges_host[a];
        const IonBackground bg = ion_background(Z, Z + (double)s[21], rho, Rd);
        const double Ra = bg.Ra, ex = bg.ex, h = bg.h, erc = std::erfc(Ra / Rd);
        const double h1 = -2.0 * kPi * Z * Ra * erc, h2 = -2.0 * kPi * Z * erc + 4.0 * spi * Z * Ra * ex / Rd;
        EJ += rho * (h1 * Ra / 3.0 - h);
        EJJ += rho * (2.0 * h - 8.0 / 9.0 * h1 * Ra + h2 * Ra * Ra / 9.0);
    }
    double m4[15], m2[6];
    for (int k = 0; k < 15; ++k) m4[k] = (double)m[k];
    for (int k = 0; k < 6; ++k) m2[k] = (double)m[15 + k];
    for (int mm = 0; mm < 3; ++mm)
        for (int n = 0; n < 3; ++n)
            for (int p = 0; p < 3; ++p)
                for (int q = 0; q < 3; ++q) {
                    double v = m4[k4_index(mm, n, p, q)];
                    if (n == q) v += m2[kK2Index[mm][p]];
                    if (mm == n && p == q) v += (double)EJ + (double)EJJ;
                    if (mm == q && n == p) v -= (double)EJ;
                    w2_host[((mm * 3 + n) * 3 + p) * 3 + q] = v;
                }
    if (c->profiling) prof_collect(c);
    return OFDFT_OK;
}
