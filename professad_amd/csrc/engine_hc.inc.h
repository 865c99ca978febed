// Host side of the Huang-Carter kinds of OFDFT_NLK (hc_kernels.h).  Included once by engine.hip inside its extern "C"
// block (fp64 library).
//
// The rest of the term set runs through the existing pipelines, untouched, with an effective mask without OFDFT_NLK (the persistent
// small-grid kernel and the hipGraph replay decline it: c->hc_inner); the term's own chain runs around it on the caller's stream:
//   head      g = n^beta; forward n, g; grad n = F^-1[i k n^] (3 inverses); min / max of xi -> host (one synchronisation)
//   host      the geometric node set xi_j = lower kappa^j, j < M, of field_dependent_convolution (functional_tools.py:412-417)
//   [the rest of the term set]
//   spectral  f^_j = w(q / xi_j) g^ for the M nodes; M inverses in batches of kBsBatch
//   gather    spline at every point: sum A K, the local part of v, u = 2 Q dxi/dgamma grad n, the node weights W_j over f_j
//   forward   M + 3 transforms; adjoint kernel: sum_j w(q / xi_j) W^_j and i k . u^; 2 inverses
//   tail      v_NL = local - div + beta n^(beta-1) adjoint, sum n v_NL; epilogue: v_NL joins dE/dn (or chi.grad and mu)
// Transforms: 2 + 3 + M + (M + 3) + 2 = 2 M + 10.  Workspace per node: one spectrum and one real grid.
// The head runs BEFORE the rest of the term set so that a refusal (M above kHcMaxNodes, a density that is not positive) comes before
// the bulk of the device work; every failing call leaves the counters of the last evaluation as they were (HcRestore).
namespace {

struct HcCounters { int fft, launch, yfwd; unsigned xk; double yp; };
HcCounters hc_counters(const ofdft_ctx* c) { return HcCounters{c->fft_count, c->launch_count, c->yfwd_fused, c->xpass_kinds, c->ypass_count}; }
void hc_counters_put(ofdft_ctx* c, const HcCounters& k) {
    c->fft_count = k.fft;
    c->launch_count = k.launch;
    c->yfwd_fused = k.yfwd;
    c->xpass_kinds = k.xk;
    c->ypass_count = k.yp;
}
// A call that fails at any point -- a refusal of the head, a HIP error, a failure of the rest of the term set or of the chain --
// leaves the counters and the time of the last evaluation as they were: the one place that puts them back.
struct HcRestore {
    ofdft_ctx* c;
    HcCounters before;
    float ms;
    bool armed = true;
    explicit HcRestore(ofdft_ctx* ctx) : c(ctx), before(hc_counters(ctx)), ms(ctx->last_ms) {}
    HcRestore(const HcRestore&) = delete;
    HcRestore& operator=(const HcRestore&) = delete;
    ~HcRestore() {
        if (!armed) return;
        hc_counters_put(c, before);
        c->last_ms = ms;
    }
};
constexpr int kNlkTerm = __builtin_ctz(OFDFT_NLK);       // the term's entry of E_terms: its bit position, as everywhere (report_energies)

HcPar hc_par(const ofdft_ctx* c) {
    HcPar p{};
    p.kind = (int)c->params[OFDFT_P_NLK_KIND];
    p.p0 = c->params[OFDFT_P_NLK_P0];
    if (p.kind == NLK_HC) {
        p.beta = c->params[OFDFT_P_NLK_P1];
        p.kappa = c->params[OFDFT_P_NLK_P2];
    } else {
        p.p1 = c->params[OFDFT_P_NLK_P1];
        p.beta = c->params[OFDFT_P_NLK_P2];
        p.kappa = c->params[OFDFT_P_NLK_P3];
    }
    return p;
}

struct HcWork {
    real *g = nullptr, *gx = nullptr, *gy = nullptr, *gz = nullptr, *v = nullptr;
    cplx *sn = nullptr, *sg = nullptr, *sx = nullptr, *sy = nullptr, *sz = nullptr;
    HcNodes nd{};
    HcTable tab{};
};

// head: everything up to the node set.  den: the density on the device
int hc_head(ofdft_ctx* c, const real* den, const HcPar& par, HcWork& w, hipStream_t st) {
    const long long npts = c->npts;
    const double inv_n = 1.0 / (double)npts;
    int rc;
    if ((rc = real_ws(c, "hc:g", &w.g)) || (rc = real_ws(c, "hc:gx", &w.gx)) || (rc = real_ws(c, "hc:gy", &w.gy)) ||
        (rc = real_ws(c, "hc:gz", &w.gz)) || (rc = real_ws(c, "hc:v", &w.v)) || (rc = spec_ws(c, "hc:sn", &w.sn)) ||
        (rc = spec_ws(c, "hc:sg", &w.sg)) || (rc = spec_ws(c, "hc:sx", &w.sx)) || (rc = spec_ws(c, "hc:sy", &w.sy)) ||
        (rc = spec_ws(c, "hc:sz", &w.sz)))
        return rc;
    const double* tabp = (const double*)c->ws["t:hc"].p;
    w.tab = HcTable{tabp, tabp + c->hc_tab_n, c->hc_tab_n, c->hc_tab_h, c->hc_tab_h * (double)(c->hc_tab_n - 1)};
    OFDFT_LAUNCH(c, st, "map", (map_kernel<MAP_POW>), dim3(grid_for(npts / 2 + 1)), dim3(256), 0, den, w.g, npts, (real)par.beta,
                 (const acc_t*)nullptr);
    const real* fin[2] = {den, w.g};
    cplx* fs[2] = {w.sn, w.sg};
    if ((rc = rfftn_internal_multi(c, fin, fs, 2, st))) return rc;
    OFDFT_LAUNCH(c, st, "spec_grad", spec_grad_kernel, dim3(grid_for(c->g.total)), dim3(256), 0, (const cplx*)w.sn, w.sx, w.sy, w.sz, c->kg);
    cplx* gs[3] = {w.sx, w.sy, w.sz};
    real* gr[3] = {w.gx, w.gy, w.gz};
    if ((rc = irfftn_internal_multi(c, gs, gr, 3, inv_n, st))) return rc;
    const int blocks = grid_for(npts, kRedThreads, kRedBlocks);
    OFDFT_LAUNCH(c, st, "hc_minmax", hc_minmax_kernel, dim3(blocks), dim3(kRedThreads), 0, den, (const real*)w.gx, (const real*)w.gy,
                 (const real*)w.gz, npts, par, c->d_partial);
    OFDFT_LAUNCH(c, st, "hc_minmax", hc_minmax_rows_kernel, dim3(1), dim3(kRedThreads), 0, (const double*)c->d_partial, blocks,
                 c->d_reduced + kHcRedMin);
    HIP_TRY(c, hipMemcpyAsync(c->h_partial + kHcRedMin, c->d_reduced + kHcRedMin, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    HIP_TRY(c, hipGetLastError());
    const double xi_min = c->h_partial[kHcRedMin], xi_max = c->h_partial[kHcRedMax];
    if (!(xi_min > 0.0) || !std::isfinite(xi_min) || !std::isfinite(xi_max))
        return fail(c, OFDFT_EINVAL, "OFDFT_NLK (Huang-Carter): xi(r) must be positive and finite everywhere, got xi_min = %g, xi_max = %g (a density that is not positive?)",
                    xi_min, xi_max);
    // functional_tools.py:415-417
    const double lk = std::log(par.kappa);
    const double lower = std::pow(par.kappa, -(std::ceil(-std::log(xi_min) / lk) + 3.0));
    const double Md = std::ceil(std::log((xi_max + 1.0) / lower) / lk) + 3.0;
    if (!(Md >= 4.0) || Md > (double)kHcMaxNodes)
        return fail(c, OFDFT_EINVAL, "OFDFT_NLK (Huang-Carter): xi_min = %g, xi_max = %g and kappa = %g need M = %.0f spline nodes, more than the %d an evaluation carries (raise kappa)",
                    xi_min, xi_max, par.kappa, Md, kHcMaxNodes);
    w.nd.M = (int)Md;
    for (int j = 0; j < w.nd.M; ++j) w.nd.xi[j] = lower * std::pow(par.kappa, (double)j);
    return 0;
}

// the chain behind the node set: v_NL into w.v, sum A K and sum n v_NL into c->d_reduced (kHcRedE, kHcRedVn)
int hc_chain(ofdft_ctx* c, const real* den, const HcPar& par, HcWork& w, hipStream_t st) {
    const long long npts = c->npts, total = c->g.total;
    const double inv_n = 1.0 / (double)npts;
    const int M = w.nd.M;
    int rc;
    cplx* sf;
    real* f;
    if ((rc = get_ws(c, "hc:sf", sizeof(cplx) * (size_t)total * M, (void**)&sf))) return rc;
    if ((rc = get_ws(c, "hc:f", sizeof(real) * (size_t)npts * M, (void**)&f))) return rc;
    cplx* specs[kHcMaxNodes + 3];
    real* reals[kHcMaxNodes + 3];
    for (int j = 0; j < M; ++j) {
        specs[j] = sf + (size_t)j * total;
        reals[j] = f + (size_t)j * npts;
    }
    specs[M] = w.sx; specs[M + 1] = w.sy; specs[M + 2] = w.sz;
    reals[M] = w.gx; reals[M + 1] = w.gy; reals[M + 2] = w.gz;
    OFDFT_LAUNCH(c, st, "hc_spec", hc_spec_kernel, dim3(grid_for(total)), dim3(256), 0, (const cplx*)w.sg, sf, c->kg, w.nd, w.tab);
    for (int b0 = 0; b0 < M; b0 += kBsBatch)
        if ((rc = irfftn_internal_multi(c, specs + b0, reals + b0, std::min(kBsBatch, M - b0), inv_n, st))) return rc;
    const double C = 0.3 * std::pow(3.0 * kPi * kPi, 2.0 / 3.0) * 8.0 * (3.0 * kPi * kPi);       // functionals.py:1266
    const int blocks = grid_for(npts, kRedThreads, kRedBlocks);
    OFDFT_LAUNCH(c, st, "hc_gather", hc_gather_kernel, dim3(blocks), dim3(kRedThreads), 0, den, w.gx, w.gy, w.gz, f, w.v, npts, par, w.nd, C,
                 c->d_partial);
    OFDFT_REDUCE(c, st, c->d_partial, blocks, 2, c->d_reduced + kHcRedE);
    for (int b0 = 0; b0 < M + 3; b0 += kBsBatch)
        if ((rc = rfftn_internal_multi(c, (const real* const*)reals + b0, specs + b0, std::min(kBsBatch, M + 3 - b0), st))) return rc;
    OFDFT_LAUNCH(c, st, "hc_adjoint", hc_adjoint_kernel, dim3(grid_for(total)), dim3(256), 0, (const cplx*)sf, (const cplx*)w.sx,
                 (const cplx*)w.sy, (const cplx*)w.sz, w.sg, w.sx, c->kg, w.nd, w.tab);
    cplx* bs[2] = {w.sg, w.sx};
    real* br[2] = {w.g, w.gx};
    if ((rc = irfftn_internal_multi(c, bs, br, 2, inv_n, st))) return rc;
    OFDFT_LAUNCH(c, st, "hc_tail", hc_tail_kernel, dim3(blocks), dim3(kRedThreads), 0, den, w.v, (const real*)w.gx, (const real*)w.g, npts,
                 par.beta, c->d_partial);
    OFDFT_REDUCE(c, st, c->d_partial, blocks, 1, c->d_reduced + kHcRedVn);
    return 0;
}

// One evaluation of a term set whose OFDFT_NLK is of kind 4 / 5.  closure = false: ofdft_energy_potential (src = the density, out =
// dE/dn or NULL); closure = true: ofdft_energy_grad_chi (src = chi, out = chi.grad or NULL).
int hc_evaluate(ofdft_ctx* c, const void* src, bool closure, const void* vext, double n_electrons, double* E_terms, double* mu_host, void* out,
                void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!c->cell_set) return fail(c, OFDFT_ESTATE, "ofdft_set_cell has not been called");
    if (!src || !E_terms) return fail(c, OFDFT_EINVAL, "null argument");
    if (closure && !(n_electrons > 0.0)) return fail(c, OFDFT_EINVAL, "n_electrons must be positive");
    if ((c->mask & OFDFT_ION_ELECTRON) && !vext) return fail(c, OFDFT_EINVAL, "IonElectron term needs vext");
    if (c->hc_tab_n < 4)
        return fail(c, OFDFT_ESTATE, "OFDFT_NLK of kind 4 / 5 (Huang-Carter) needs its kernel table: call ofdft_set_nlk_table first");
    const HcPar par = hc_par(c);
    const unsigned full = c->mask, rest = full & ~OFDFT_NLK;
    HcRestore restore(c);
    c->hvp_valid = false;
    hc_counters_put(c, HcCounters{0, 0, 0, 0u, 0.0});
    if (!c->hc_ev[0])
        for (auto& e : c->hc_ev) HIP_TRY(c, hipEventCreate(&e));
    HIP_TRY(c, hipEventRecord(c->hc_ev[0], st));

    const real* den = (const real*)src;
    if (closure) {          // n = c chi^2 with the closure scale formed on the device (system.py:833-834)
        real* d;
        if (int rc = real_ws(c, "hc:den", &d)) return rc;
        enqueue_closure_scale(c, (const real*)src, n_electrons, st);
        OFDFT_LAUNCH(c, st, "map", (map_kernel<MAP_SCALE_SQ>), dim3(grid_for(c->npts / 2 + 1)), dim3(256), 0, (const real*)src, d, c->npts, 0.0,
                     (const acc_t*)(c->d_scal + kScalClosure));
        den = d;
    }
    HcWork w;
    if (int rc = hc_head(c, den, par, w, st)) return rc;
    HIP_TRY(c, hipEventRecord(c->hc_ev[1], st));
    const HcCounters head = hc_counters(c);

    double mu_rest = 0.0;
    float ms_rest = 0.f;
    if (rest) {
        c->mask = rest;
        c->hc_inner = true;
        const int rc = closure ? ofdft_energy_grad_chi(c, src, vext, n_electrons, E_terms, &mu_rest, out, stream)
                               : ofdft_energy_potential(c, src, vext, E_terms, out, stream);
        c->mask = full;
        c->hc_inner = false;
        if (rc) return rc;
        ms_rest = c->last_ms;
    } else {
        hc_counters_put(c, HcCounters{0, 0, 0, 0u, 0.0});
        for (int i = 0; i < OFDFT_NTERMS; ++i) E_terms[i] = 0.0;
    }
    c->hvp_valid = false;
    c->fft_count += head.fft;
    c->launch_count += head.launch;

    HIP_TRY(c, hipEventRecord(c->hc_ev[2], st));
    if (int rc = hc_chain(c, den, par, w, st)) return rc;
    if (out)
        OFDFT_LAUNCH(c, st, "hc_epilogue", hc_epilogue_kernel, dim3(grid_for(c->npts)), dim3(256), 0, (const real*)w.v, (real*)out, c->npts,
                     rest ? 1 : 0, closure ? (const real*)src : (const real*)nullptr, (const acc_t*)(c->d_scal + kScalClosure), 2.0 * c->dV,
                     (const acc_t*)(c->d_reduced + kHcRedVn), c->dV / (closure ? n_electrons : 1.0));
    HIP_TRY(c, hipMemcpyAsync(c->h_partial + kHcRedE, c->d_reduced + kHcRedE, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipEventRecord(c->hc_ev[3], st));
    HIP_TRY(c, hipStreamSynchronize(st));
    HIP_TRY(c, hipGetLastError());
    float ms_head = 0.f, ms_tail = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms_head, c->hc_ev[0], c->hc_ev[1]));
    HIP_TRY(c, hipEventElapsedTime(&ms_tail, c->hc_ev[2], c->hc_ev[3]));
    c->last_ms = ms_head + ms_rest + ms_tail;
    c->ms_pending = false;
    if (c->profiling) prof_collect(c);
    if (c->h_partial[kHcRedBad] != 0.0)
        return fail(c, OFDFT_EINVAL, "OFDFT_NLK (Huang-Carter): %.0f points fell outside the spline intervals 1 .. M - 3 of the node set (M = %d)",
                    c->h_partial[kHcRedBad], w.nd.M);
    E_terms[kNlkTerm] = c->h_partial[kHcRedE] * c->dV;
    if (closure && mu_host) *mu_host = mu_rest + c->h_partial[kHcRedVn] * c->dV / n_electrons;
    restore.armed = false;
    return OFDFT_OK;
}

}  // namespace

int ofdft_set_nlk_table(ofdft_ctx* c, const double* eta, const double* wv, int n) {
    if (!c) return OFDFT_EINVAL;
    OFDFT_ON_DEVICE(c, c->device);
    if (!eta || !wv) return fail(c, OFDFT_EINVAL, "ofdft_set_nlk_table: null argument");
    if (n < 4 || n > (1 << 24)) return fail(c, OFDFT_EINVAL, "ofdft_set_nlk_table: the table needs 4 .. 2^24 nodes, got %d", n);
    const double h = (eta[n - 1] - eta[0]) / (double)(n - 1);
    if (eta[0] != 0.0 || !(h > 0.0) || !std::isfinite(h)) return fail(c, OFDFT_EINVAL, "ofdft_set_nlk_table: the eta grid must start at 0 and increase");
    for (int k = 0; k < n; ++k) {
        if (!(std::fabs(eta[k] - (double)k * h) <= 1e-9 * h)) return fail(c, OFDFT_EINVAL, "ofdft_set_nlk_table: the eta grid must be uniform (node %d)", k);
        if (!std::isfinite(wv[k])) return fail(c, OFDFT_EINVAL, "ofdft_set_nlk_table: w is not finite at node %d", k);
    }
    // functional_tools.py:309-310
    std::vector<double> up(2 * (size_t)n);
    for (int k = 0; k < n; ++k) up[k] = wv[k];
    double* m = up.data() + n;
    auto sec = [&](int k) { return (wv[k + 1] - wv[k]) / (eta[k + 1] - eta[k]); };
    m[0] = sec(0);
    for (int k = 1; k < n - 1; ++k) m[k] = (sec(k) + sec(k - 1)) / 2.0;
    m[n - 1] = sec(n - 2);
    void* dev;
    if (int rc = get_ws(c, "t:hc", sizeof(double) * 2 * (size_t)n, &dev)) return rc;
    HIP_TRY(c, hipDeviceSynchronize());          // (an evaluation on another stream may still read the table this replaces)
    HIP_TRY(c, hipMemcpy(dev, up.data(), sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice));
    c->hc_tab_n = n;
    c->hc_tab_h = h;
    c->nlk_valid = false;
    c->hvp_valid = false;
    c->version++;
    return OFDFT_OK;
}
