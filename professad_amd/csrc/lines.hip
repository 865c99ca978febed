// Line-transform drivers of the engine (see engine_ctx.h for the split of the sources).  gfx950 only.
#include "engine_ctx.h"

namespace eng {

// ---------------------------------------------------------------------------------- FFT drivers
template <int LEN, bool INV>
int launch_cpass_t(ofdft_ctx* c, const ArrList& arrs, int narr, const LineMap& main, const LineMap& rem, hipStream_t st,
                   const char* nm) {
    cplx* tw;
    if (int rc = get_twiddle(c, LEN, &tw)) return rc;
    using Cfg = PassCfg<LEN>;
    // (tiles of the main part rounded up to whole groups of OFDFT_CPASS_TILES: a workgroup's tiles never straddle the two parts)
    constexpr int T = OFDFT_CPASS_TILES;
    const int mb = ((main.nlines + Cfg::LPW - 1) / Cfg::LPW + T - 1) / T * T, rb = (rem.nlines + Cfg::LPW - 1) / Cfg::LPW;
    OFDFT_LAUNCH(c, st, nm, (cpass_kernel<LEN, INV>), dim3((mb + rb + T - 1) / T, narr), dim3(Cfg::TPB), Cfg::LDS, arrs, main, rem, mb,
                 c->g.main_count, tw);
    return 0;
}

// line maps of the block-8 layout (see fft_kernels.h)
void pass_maps(const ofdft_ctx* c, int axis, LineMap& main, LineMap& rem) {
    const SpecGeom& g = axis == 0 ? c->gx : c->g;
    const int nb = g.nzm / 8, nrem = g.nzc - g.nzm;
    if (axis == 0) {   // x lines: base = b*n0*n1*8 + (y*8+kin), stride n1*8
        main.d = g.n1 * 8; main.sb = (long long)g.n0 * g.n1 * 8; main.sl = 1; main.se = (long long)g.n1 * 8;
        main.nlines = nb * g.n1 * 8; main.lf = 0;  // lf filled by caller (LPW)
        rem.d = g.n1; rem.sb = (long long)g.n0 * g.n1; rem.sl = 1; rem.se = g.n1; rem.nlines = nrem * g.n1; rem.lf = 0;
    } else {           // y lines: base = (b*n0+x)*n1*8 + kin, stride 8
        main.d = 8; main.sb = (long long)g.n1 * 8; main.sl = 1; main.se = 8; main.nlines = nb * g.n0 * 8; main.lf = 8;
        rem.d = 1; rem.sb = g.n1; rem.sl = 0; rem.se = 1; rem.nlines = nrem * g.n0; rem.lf = 1;
    }
    if (main.nlines == 0) { main.d = 1; main.lf = 1; }
    if (rem.nlines == 0) { rem.d = 1; rem.lf = 1; }
}

// line pass over `narr` spectra in ONE launch
template <bool INV>
int fast_axis_pass_multi(ofdft_ctx* c, int axis, cplx* const* specs, int narr, hipStream_t st) {
    LineMap main, rem;
    pass_maps(c, axis, main, rem);
    ArrList arrs{};
    for (int a = 0; a < narr; ++a) arrs.p[a] = specs[a];
    if (axis == 1) c->ypass_count += narr;
    const int len = axis == 0 ? c->n0g : c->n1;
    const char* nm = axis == 0 ? "cpass_x" : "cpass_y";
    return for_len(kLineLens, len, [&](auto L) {
        if (axis == 0) main.lf = rem.lf = PassCfg<L()>::LPW;
        return launch_cpass_t<L(), INV>(c, arrs, narr, main, rem, st, nm);
    }, [&] { return fail(c, OFDFT_EINVAL, "unsupported fast FFT length %d", len); });
}

template <bool INV>
int fast_axis_pass(ofdft_ctx* c, int axis, cplx* spec, hipStream_t st) {
    return fast_axis_pass_multi<INV>(c, axis, &spec, 1, st);
}
// y pass of `narr` x-slab spectra straight into (forward) / out of (inverse) an all-to-all buffer
template <int LEN, bool INV>
int launch_ypass_xchg_t(ofdft_ctx* c, const ArrList& arrs, int narr, cplx* buf, hipStream_t st, int xk) {
    cplx* tw;
    if (int rc = get_twiddle(c, LEN, &tw)) return rc;
    using Cfg = PassCfg<LEN>;
    LineMap main, rem;
    pass_maps(c, 1, main, rem);
    // the chunk's kz blocks [kb0, kb1) of the x-slab spectra <-> its region of the chunk-major exchange buffer
    const XcView v = xc_view(c, xk);
    XchgGeom xg = c->xg;
    xg.nb = v.nb;
    xg.nrem = v.nrem;
    xg.kb0 = v.kb0;
    xg.arr_sz = v.arr_sz;
    xg.rec = narr * xg.arr_sz;
    xg.chunk = xg.nxl * xg.rec;
    const int per_block = c->g.n0 * 8;                  // y lines per kz block
    int line0 = 0;
    if (v.nb != c->xg.nb) {
        if (per_block % Cfg::LPW) return fail(c, OFDFT_EINVAL, "kz-chunked exchange needs whole y-pass workgroups per kz block");
        line0 = v.kb0 * per_block;
        main.nlines = v.kb1 * per_block;
        if (!v.nrem) rem.nlines = 0;
    }
    main.blk0 = line0 / Cfg::LPW;
    const int mb = (main.nlines - line0 + Cfg::LPW - 1) / Cfg::LPW, rb = (rem.nlines + Cfg::LPW - 1) / Cfg::LPW;
    if (mb + rb == 0) return 0;
    c->ypass_count += narr * (double)(v.nb * 8 + v.nrem) / c->g.nzc;
    OFDFT_LAUNCH(c, st, INV ? "ypass_recv" : "ypass_send", (ypass_xchg_kernel<LEN, INV>), dim3(mb + rb, narr), dim3(Cfg::TPB),
                 Cfg::LDS, arrs, buf + (long long)narr * v.base1, xg, main, rem, mb, c->g.main_count, tw);
    return 0;
}
template <bool INV>
int ypass_xchg(ofdft_ctx* c, const std::vector<cplx*>& list, cplx* buf, hipStream_t st, int xk) {
    const int narr = (int)list.size();
    if (narr == 0) return 0;
    if (narr > 16) return fail(c, OFDFT_EINVAL, "too many spectra in one exchange (%d)", narr);
    ArrList arrs{};
    for (int a = 0; a < narr; ++a) arrs.p[a] = list[a];
    return for_len(kLineLens, c->n1, [&](auto L) { return launch_ypass_xchg_t<L(), INV>(c, arrs, narr, buf, st, xk); },
                   [&] { return fail(c, OFDFT_EINVAL, "unsupported fast FFT length %d", c->n1); });
}

template <int M>
int launch_zfwd_t(ofdft_ctx* c, const real* in, cplx* spec, hipStream_t st) {
    cplx *twM, *twN;
    if (int rc = get_twiddle(c, M, &twM)) return rc;
    if (int rc = get_twiddle(c, 2 * M, &twN)) return rc;
    if constexpr ((M & (M - 1)) == 0) {
        using Cfg = ZCfg<M>;
        const int blocks = (int)((c->g.nrows + Cfg::RPW - 1) / Cfg::RPW);
        OFDFT_LAUNCH(c, st, "zfwd", (zfwd_kernel<M, PreIdentity>), dim3(blocks), dim3(Cfg::TPB), Cfg::LDS, in, spec, c->g, twM,
                           twN, PreIdentity());
    } else {          // rows with factors 3 / 5: the wave-local z pass (zpass.h)
        using W = ZW<M, ZPick<M, 8>::E>;
        const int blocks = (int)((c->g.nrows + W::RPB - 1) / W::RPB);
        OFDFT_LAUNCH(c, st, "zfwd", (zfwd_w_kernel<M, W::E>), dim3(blocks), dim3(256), W::LDS, in, spec, c->g, (const cplx*)twM,
                     (const cplx*)twN);
    }
    return 0;
}
template <int M>
int launch_zinv_t(ofdft_ctx* c, const cplx* spec, real* out, double scale, hipStream_t st) {
    cplx *twM, *twN;
    if (int rc = get_twiddle(c, M, &twM)) return rc;
    if (int rc = get_twiddle(c, 2 * M, &twN)) return rc;
    if constexpr ((M & (M - 1)) == 0) {
        using Cfg = ZCfg<M>;
        const int blocks = (int)((c->g.nrows + Cfg::RPW - 1) / Cfg::RPW);
        PostScale post{(real)scale};
        OFDFT_LAUNCH(c, st, "zinv", (zinv_kernel<M, PostScale>), dim3(blocks), dim3(Cfg::TPB), Cfg::LDS, spec, out, c->g, twM,
                           twN, post);
    } else {
        using W = ZW<M, ZPick<M, 8>::E>;
        const int blocks = (int)((c->g.nrows + W::RPB - 1) / W::RPB);
        OFDFT_LAUNCH(c, st, "zinv", (zinv_w_kernel<M, W::E>), dim3(blocks), dim3(256), W::LDS, spec, out, c->g, (const cplx*)twM,
                     (const cplx*)twN, (real)scale);
    }
    return 0;
}
// dispatch on the half length of the z rows
int zfwd_any(ofdft_ctx* c, const real* in, cplx* spec, hipStream_t st) {
    return for_len(kZRowLens, c->n2 / 2, [&](auto M) { return launch_zfwd_t<M()>(c, in, spec, st); },
                   [&] { return fail(c, OFDFT_EINVAL, "bad n2"); });
}
int zinv_any(ofdft_ctx* c, const cplx* spec, real* out, double scale, hipStream_t st) {
    return for_len(kZRowLens, c->n2 / 2, [&](auto M) { return launch_zinv_t<M()>(c, spec, out, scale, st); },
                   [&] { return fail(c, OFDFT_EINVAL, "bad n2"); });
}

int gen_axis(ofdft_ctx* c, int axis, int inv, cplx*& cur, cplx*& other, hipStream_t st) {
    cplx* tw;
    if (int rc = get_twiddle(c, axis == 0 ? c->n0 : c->n1, &tw)) return rc;
    OFDFT_LAUNCH(c, st, "gen_c2c", gen_c2c_kernel, dim3((unsigned)((c->g.total + 255) / 256)), dim3(256), 0, cur, other, c->g,
                       axis, inv, tw);
    std::swap(cur, other);
    return 0;
}

// ---- Bluestein tables (bluestein.h): chirp w_n = exp(-i pi n^2 / N) and the filter spectrum FFT_M(conj w, wrapped) / M
struct BsTables { cplx *chirp = nullptr, *filt = nullptr; int M = 0; };

int bluestein_pad(int N) {
    int M = 8;
    while (M < 2 * N - 1) M *= 2;
    return M;
}

int get_bluestein(ofdft_ctx* c, int N, BsTables* out) {
    const std::string key = "bs:" + std::to_string(N);
    const int M = bluestein_pad(N);
    out->M = M;
    auto it = c->ws.find(key);
    if (it != c->ws.end()) {
        out->chirp = (cplx*)it->second.p;
        out->filt = out->chirp + N;
        return 0;
    }
    const long double pi = 3.14159265358979323846264338327950288L;
    std::vector<cplx> h((size_t)N + M);
    std::vector<long double> br(M, 0.0L), bi(M, 0.0L);
    for (int n = 0; n < N; ++n) {
        const long long r = ((long long)n * n) % (2LL * N);          // n^2 mod 2N keeps the angle small and exact
        const long double ph = -pi * (long double)r / (long double)N;
        const long double cr = cosl(ph), ci = sinl(ph);
        h[n] = mkc((double)cr, (double)ci);
        br[n] = cr;
        bi[n] = -ci;                                                   // b_n = conj(w_n), b_{-n} = b_n
        if (n) {
            br[M - n] = cr;
            bi[M - n] = -ci;
        }
    }
    // FFT_M(b) / M by a direct O(M^2) sum in extended precision (once per length; M <= 1024)
    std::vector<long double> cs(M), sn(M);
    for (int m = 0; m < M; ++m) {
        cs[m] = cosl(-2.0L * pi * m / M);
        sn[m] = sinl(-2.0L * pi * m / M);
    }
    for (int k = 0; k < M; ++k) {
        long double sr = 0.0L, si = 0.0L;
        for (int n = 0; n < M; ++n) {
            if (br[n] == 0.0L && bi[n] == 0.0L) continue;
            const int t = (int)(((long long)k * n) % M);
            sr += br[n] * cs[t] - bi[n] * sn[t];
            si += br[n] * sn[t] + bi[n] * cs[t];
        }
        h[N + k] = mkc((double)(sr / M), (double)(si / M));
    }
    cplx* d;
    if (int rc = get_ws(c, key.c_str(), sizeof(cplx) * h.size(), (void**)&d)) return rc;
    HIP_TRY(c, hipMemcpy(d, h.data(), sizeof(cplx) * h.size(), hipMemcpyHostToDevice));
    out->chirp = d;
    out->filt = d + N;
    return 0;
}

static int device_cus(const ofdft_ctx* c) {
    static int cus[64] = {0};
    const int d = c->device >= 0 && c->device < 64 ? c->device : 0;
    if (!cus[d]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || n <= 0) n = 256;
        cus[d] = n;
    }
    return cus[d];
}

template <int M>
int launch_bluestein_t(ofdft_ctx* c, const BsIo& io, int narr, const BsArgs& b, const BsTables& t, hipStream_t st) {
    cplx* tw;
    if (int rc = get_twiddle(c, M, &tw)) return rc;
    const char* nm = b.mode ? "bluestein_z" : (b.axis ? "bluestein_y" : "bluestein_x");
    // persistent workgroups (the tables are staged once per workgroup): at most OFDFT_BS_WGS per CU and array
#define OFDFT_BS(KIND_, INV_)                                                                                                       \
    do {                                                                                                                            \
        using Cfg = BsCfg<M, (KIND_ != BS_CPLX ? 1 : 0)>;                                                                                     \
        const long long tiles = (b.nlines + Cfg::LPW - 1) / Cfg::LPW;                                                               \
        const int blocks = (int)std::min<long long>(tiles, (long long)device_cus(c) * OFDFT_BS_WGS);                                \
        OFDFT_LAUNCH(c, st, nm, (bluestein_kernel<M, KIND_, INV_>), dim3(blocks, narr), dim3(Cfg::TPB), Cfg::LDS, io, c->g, b,      \
                     (const cplx*)t.chirp, (const cplx*)t.filt, (const cplx*)tw);                                                   \
    } while (0)
    if (b.mode == 1) OFDFT_BS(BS_R2C, false);
    else if (b.mode == 2) OFDFT_BS(BS_C2R, true);
    else if (b.inv) OFDFT_BS(BS_CPLX, true);
    else OFDFT_BS(BS_CPLX, false);
#undef OFDFT_BS
    return 0;
}

int bluestein_pass_multi(ofdft_ctx* c, int mode, int axis, int inv, const BsIo& io, int narr, double scale, hipStream_t st);
bool bluestein_ok(const ofdft_ctx* c);
// forward-x, mix, inverse-x in one chirp-z kernel (bluestein.h: bluestein_xmix_kernel); x extents up to 256 (M <= 512)
template <int M, int NIN, int NOUT, class Mix>
static int launch_xmix_t(ofdft_ctx* c, const BsMixIo& io, const Mix& mix, const BsTables& t, hipStream_t st) {
    cplx* tw;
    if (int rc = get_twiddle(c, M, &tw)) return rc;
    using Cfg = BsCfg<M, 2>;
    const long long nlines = (long long)c->n1 * c->g.nzc;
    const long long tiles = (nlines + Cfg::LPW - 1) / Cfg::LPW;
    const int blocks = (int)std::min<long long>(tiles, (long long)device_cus(c) * OFDFT_BS_WGS);
    c->xpass_kinds |= OFDFT_XPASS_CHIRPZ;
    OFDFT_LAUNCH(c, st, "bluestein_xmix", (bluestein_xmix_kernel<M, NIN, NOUT, Mix>), dim3(blocks), dim3(Cfg::TPB), Cfg::LDS, io, c->g,
                 c->n0, nlines, (const cplx*)t.chirp, (const cplx*)t.filt, (const cplx*)tw, mix);
    return 0;
}
bool bluestein_xmix_ok(const ofdft_ctx* c) {
    return c->bs_fused && bluestein_ok(c) && c->nranks == 1 && !c->fast && has_len(kChirpXmixLens, bluestein_pad(c->n0));
}
template <int NIN, int NOUT, class Mix>
int bluestein_xmix(ofdft_ctx* c, const cplx* const* in, cplx* const* out, const Mix& mix, hipStream_t st) {
    BsTables t;
    if (int rc = get_bluestein(c, c->n0, &t)) return rc;
    BsMixIo io{};
    for (int i = 0; i < NIN; ++i) io.in[i] = in[i];
    for (int o = 0; o < NOUT; ++o) io.out[o] = out[o];
    return for_len(kChirpXmixLens, t.M, [&](auto M) { return launch_xmix_t<M(), NIN, NOUT, Mix>(c, io, mix, t, st); },
                   [&] { return fail(c, OFDFT_EINVAL, "no fused chirp-z x pass for length %d", c->n0); });
}
template int bluestein_xmix<1, 1, MixScale<SPEC_HARTREE>>(ofdft_ctx*, const cplx* const*, cplx* const*, const MixScale<SPEC_HARTREE>&, hipStream_t);
template int bluestein_xmix<1, 1, MixScale<SPEC_LAPLACE>>(ofdft_ctx*, const cplx* const*, cplx* const*, const MixScale<SPEC_LAPLACE>&, hipStream_t);
template int bluestein_xmix<1, 1, MixScale<SPEC_LINDHARD>>(ofdft_ctx*, const cplx* const*, cplx* const*, const MixScale<SPEC_LINDHARD>&, hipStream_t);
#ifndef OFDFT_REAL_F32      // ofdft_precondition: fp64 library only
template int bluestein_xmix<1, 1, MixScale<SPEC_SCREENED>>(ofdft_ctx*, const cplx* const*, cplx* const*, const MixScale<SPEC_SCREENED>&, hipStream_t);
#endif
template int bluestein_xmix<1, 3, MixDensity<false, true>>(ofdft_ctx*, const cplx* const*, cplx* const*, const MixDensity<false, true>&, hipStream_t);
template int bluestein_xmix<1, 4, MixDensity<true, true>>(ofdft_ctx*, const cplx* const*, cplx* const*, const MixDensity<true, true>&, hipStream_t);
template int bluestein_xmix<3, 1, MixDiv>(ofdft_ctx*, const cplx* const*, cplx* const*, const MixDiv&, hipStream_t);
template int bluestein_xmix<1, 1, MixNlk<1>>(ofdft_ctx*, const cplx* const*, cplx* const*, const MixNlk<1>&, hipStream_t);
template int bluestein_xmix<2, 2, MixNlk<2>>(ofdft_ctx*, const cplx* const*, cplx* const*, const MixNlk<2>&, hipStream_t);
template int bluestein_xmix<3, 3, MixWgc>(ofdft_ctx*, const cplx* const*, cplx* const*, const MixWgc&, hipStream_t);

// small grids: z rows and y lines of an x plane in one kernel (bluestein.h: bluestein_zy_kernel) -- both padded lengths equal and
// <= 128, the (y, kz) plane in LDS
static bool bluestein_zy_ok(const ofdft_ctx* c, int* M_out) {
    if (!c->bs_fused) return false;
    const int M1 = bluestein_pad(c->n1), M2 = bluestein_pad(c->n2);
    if (M1 != M2 || !has_len(kChirpZyLens, M1)) return false;
    *M_out = M1;
    return true;
}
template <int M, bool INV>
static int launch_zy_t(ofdft_ctx* c, const BsIo& io, int narr, double scale, hipStream_t st) {
    cplx* tw;
    if (int rc = get_twiddle(c, M, &tw)) return rc;
    BsTables ty, tz;
    if (int rc = get_bluestein(c, c->n1, &ty)) return rc;
    if (int rc = get_bluestein(c, c->n2, &tz)) return rc;
    const size_t lds = BsZyCfg<M>::lds_bytes(c->n1, c->g.nzc);
    if (lds > 160 * 1024) return fail(c, OFDFT_EINVAL, "fused z / y chirp-z pass: plane too large for LDS");
    OFDFT_LAUNCH(c, st, INV ? "bluestein_yz" : "bluestein_zy", (bluestein_zy_kernel<M, INV>), dim3(c->n0, narr), dim3(BsZyCfg<M>::TPB), lds, io,
                 c->g, (real)scale, (const cplx*)tz.chirp, (const cplx*)tz.filt, (const cplx*)ty.chirp, (const cplx*)ty.filt, (const cplx*)tw);
    return 0;
}
template <bool INV>
static int bluestein_zy(ofdft_ctx* c, int M, const BsIo& io, int narr, double scale, hipStream_t st) {
    return for_len(kChirpZyLens, M, [&](auto L) { return launch_zy_t<L(), INV>(c, io, narr, scale, st); },
                   [&] { return fail(c, OFDFT_EINVAL, "no fused z / y chirp-z pass for padded length %d", M); });
}

// the z and y passes of `n` (<= kBsBatch) transforms, one launch per pass (small grids: ONE launch for both): the halves of a 3-D
// transform around the fused x pass
int bluestein_fwd_zy_multi(ofdft_ctx* c, const real* const* in, cplx* const* spec, int n, hipStream_t st, const BsPrep* prep) {
    BsIo io{};
    for (int a = 0; a < n; ++a) {
        io.spec[a] = spec[a];
        io.rin[a] = in[a];
        if (prep) {
            io.prep[a] = prep->kind[a];
            io.pe[a] = (real)prep->e[a];
        }
    }
    if (prep) io.pnref = (real)prep->nref;
    c->fft_count += n;
    int M;
    if (bluestein_zy_ok(c, &M)) return bluestein_zy<false>(c, M, io, n, 1.0, st);
    if (int rc = bluestein_pass_multi(c, 1, 2, 0, io, n, 1.0, st)) return rc;
    return bluestein_pass_multi(c, 0, 1, 0, io, n, 1.0, st);
}
int bluestein_inv_yz_multi(ofdft_ctx* c, cplx* const* spec, real* const* out, int n, double scale, hipStream_t st) {
    BsIo io{};
    for (int a = 0; a < n; ++a) {
        io.spec[a] = spec[a];
        io.rout[a] = out[a];
    }
    c->fft_count += n;
    int M;
    if (bluestein_zy_ok(c, &M)) return bluestein_zy<true>(c, M, io, n, scale, st);
    if (int rc = bluestein_pass_multi(c, 0, 1, 1, io, n, 1.0, st)) return rc;
    return bluestein_pass_multi(c, 2, 2, 1, io, n, scale, st);
}

// one generic-length pass over `narr` (<= kBsBatch) arrays: mode 0 (complex, axis 0/1), 1 (r2c along z), 2 (c2r along z)
int bluestein_pass_multi(ofdft_ctx* c, int mode, int axis, int inv, const BsIo& io, int narr, double scale, hipStream_t st) {
    const int N = mode == 0 ? (axis == 0 ? c->n0 : c->n1) : c->n2;
    BsTables t;
    if (int rc = get_bluestein(c, N, &t)) return rc;
    BsArgs b{};
    b.N = N;
    b.mode = mode;
    b.axis = axis;
    b.inv = inv;
    b.scale = scale;
    b.nlines = mode == 0 ? (long long)(axis == 0 ? c->n1 : c->n0) * c->g.nzc : (c->g.nrows + 1) / 2;      // (z rows go in pairs)
    return for_len(kChirpLens, t.M, [&](auto M) { return launch_bluestein_t<M()>(c, io, narr, b, t, st); },
                   [&] { return fail(c, OFDFT_EINVAL, "no Bluestein plan for length %d", N); });
}

int bluestein_pass(ofdft_ctx* c, int mode, int axis, int inv, cplx* spec, const real* rin, real* rout, double scale,
                   hipStream_t st) {
    BsIo io{};
    io.spec[0] = spec;
    io.rin[0] = rin;
    io.rout[0] = rout;
    return bluestein_pass_multi(c, mode, axis, inv, io, 1, scale, st);
}

// (extents up to 512: a padded length with a plan)
bool bluestein_ok(const ofdft_ctx* c) {
    return c->use_bluestein && has_len(kChirpLens, bluestein_pad(c->n0)) && has_len(kChirpLens, bluestein_pad(c->n1)) &&
           has_len(kChirpLens, bluestein_pad(c->n2));
}
static bool bluestein_ok_fwd(const ofdft_ctx* c) { return bluestein_ok(c); }

// ---- slab-decomposed 3-D transforms for the per-geometry-step routines (stress, ionic potential, forces): a real x-slab
// [n0/P][n1][n2] <-> the y-slab of the half spectrum in the block-8 layout of the x-pass geometry (c->gx: all of x, n1/P of
// y), which is what every k-space kernel of those routines indexes (kvec / spec_decode with kg.g = gx, kg.y0).  One
// all-to-all per transform through the host's collective (ofdft_set_collectives); the y pass reads / writes the exchange
// layout directly, a small kernel converts between it and the block-8 y-slab array.
static __global__ void xchg_unpack_kernel(const cplx* __restrict__ buf, cplx* __restrict__ spec, SpecGeom gx, XchgGeom xg, int pack) {
    // record of x: [ main (b, yl, kin) | planes (plane, yl) ], one array per record
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < gx.total; i += (long long)gridDim.x * blockDim.x) {
        int x, yl, kz;
        spec_decode(gx, i, x, yl, kz);
        const long long r = (long long)x * xg.arr_sz +
                            (kz < gx.nzm ? (((long long)(kz >> 3) * xg.nyl + yl) * 8 + (kz & 7))
                                         : ((long long)xg.nb * xg.nyl * 8 + (long long)(kz - gx.nzm) * xg.nyl + yl));
        if (pack) const_cast<cplx*>(buf)[r] = spec[i];
        else spec[i] = buf[r];
    }
}
static int dist_rfftn(ofdft_ctx* c, const real* in, cplx* spec, hipStream_t st);
static int dist_irfftn(ofdft_ctx* c, cplx* spec, real* out, double scale, hipStream_t st);

static bool bluestein_ok_fwd(const ofdft_ctx* c);
// `n` (<= kBsBatch) transforms at once: on the chirp-z path every pass covers all of them in ONE launch (small odd grids -- the
// reference's ecut2shape gives 30..100 points per axis -- are bound by their launch count: 69 chirp-z launches for the bench's
// term set); every other path transforms them one by one
int rfftn_internal_multi(ofdft_ctx* c, const real* const* in, cplx* const* spec, int n, hipStream_t st) {
    if (n > 1 && n <= kBsBatch && c->nranks == 1 && !c->fast && bluestein_ok_fwd(c)) {
        BsIo io{};
        for (int a = 0; a < n; ++a) {
            io.spec[a] = spec[a];
            io.rin[a] = in[a];
        }
        c->fft_count += n;
        if (int rc = bluestein_pass_multi(c, 1, 2, 0, io, n, 1.0, st)) return rc;
        if (int rc = bluestein_pass_multi(c, 0, 1, 0, io, n, 1.0, st)) return rc;
        return bluestein_pass_multi(c, 0, 0, 0, io, n, 1.0, st);
    }
    for (int a = 0; a < n; ++a)
        if (int rc = rfftn_internal(c, in[a], spec[a], st)) return rc;
    return 0;
}
int irfftn_internal_multi(ofdft_ctx* c, cplx* const* spec, real* const* out, int n, double scale, hipStream_t st) {
    if (n > 1 && n <= kBsBatch && c->nranks == 1 && !c->fast && bluestein_ok_fwd(c)) {
        BsIo io{};
        for (int a = 0; a < n; ++a) {
            io.spec[a] = spec[a];
            io.rout[a] = out[a];
        }
        c->fft_count += n;
        if (int rc = bluestein_pass_multi(c, 0, 0, 1, io, n, 1.0, st)) return rc;
        if (int rc = bluestein_pass_multi(c, 0, 1, 1, io, n, 1.0, st)) return rc;
        return bluestein_pass_multi(c, 2, 2, 1, io, n, scale, st);
    }
    for (int a = 0; a < n; ++a)
        if (int rc = irfftn_internal(c, spec[a], out[a], scale, st)) return rc;
    return 0;
}

// real [n0][n1][n2] -> internal half spectrum (unnormalised, like torch.fft.rfftn)
int rfftn_internal(ofdft_ctx* c, const real* in, cplx* spec, hipStream_t st) {
    c->fft_count++;
    if (c->nranks > 1) return dist_rfftn(c, in, spec, st);
    if (c->fast) {
        int rc = zfwd_any(c, in, spec, st);
        if (rc) return rc;
        if ((rc = fast_axis_pass<false>(c, 1, spec, st))) return rc;
        return fast_axis_pass<false>(c, 0, spec, st);
    }
    if (bluestein_ok(c)) {        // arbitrary extents: chirp-z line transforms, in place
        if (int rc = bluestein_pass(c, 1, 2, 0, spec, in, nullptr, 1.0, st)) return rc;
        if (int rc = bluestein_pass(c, 0, 1, 0, spec, nullptr, nullptr, 1.0, st)) return rc;
        return bluestein_pass(c, 0, 0, 0, spec, nullptr, nullptr, 1.0, st);
    }
    cplx *tw2, *tmp;
    if (int rc = get_twiddle(c, c->n2, &tw2)) return rc;
    if (int rc = spec_ws(c, "gen_tmp", &tmp)) return rc;
    // z into tmp, y: tmp -> spec, x: spec -> tmp, then copy back (two swaps leave the result in tmp)
    OFDFT_LAUNCH(c, st, "gen_r2c_z", gen_r2c_z_kernel, dim3((unsigned)((c->g.total + 255) / 256)), dim3(256), 0, in, spec, c->g, tw2);
    cplx *cur = spec, *other = tmp;
    if (int rc = gen_axis(c, 1, 0, cur, other, st)) return rc;
    if (int rc = gen_axis(c, 0, 0, cur, other, st)) return rc;
    if (cur != spec) HIP_TRY(c, hipMemcpyAsync(spec, cur, sizeof(cplx) * c->g.total, hipMemcpyDeviceToDevice, st));
    return 0;
}

// internal half spectrum (destroyed) -> real, scaled by `scale` (1/N for irfftn semantics)
int irfftn_internal(ofdft_ctx* c, cplx* spec, real* out, double scale, hipStream_t st) {
    c->fft_count++;
    if (c->nranks > 1) return dist_irfftn(c, spec, out, scale, st);
    if (c->fast) {
        int rc;
        if ((rc = fast_axis_pass<true>(c, 0, spec, st))) return rc;
        if ((rc = fast_axis_pass<true>(c, 1, spec, st))) return rc;
        return zinv_any(c, spec, out, scale, st);
    }
    if (bluestein_ok(c)) {
        if (int rc = bluestein_pass(c, 0, 0, 1, spec, nullptr, nullptr, 1.0, st)) return rc;
        if (int rc = bluestein_pass(c, 0, 1, 1, spec, nullptr, nullptr, 1.0, st)) return rc;
        return bluestein_pass(c, 2, 2, 1, spec, nullptr, out, scale, st);
    }
    cplx *tw2, *tmp;
    if (int rc = get_twiddle(c, c->n2, &tw2)) return rc;
    if (int rc = spec_ws(c, "gen_tmp", &tmp)) return rc;
    cplx *cur = spec, *other = tmp;
    if (int rc = gen_axis(c, 0, 1, cur, other, st)) return rc;
    if (int rc = gen_axis(c, 1, 1, cur, other, st)) return rc;
    PostScale post{(real)scale};
    OFDFT_LAUNCH(c, st, "gen_c2r_z", (gen_c2r_z_kernel<PostScale>), dim3((unsigned)((c->npts + 255) / 256)), dim3(256), 0, cur, out,
                       c->g, tw2, post);
    return 0;
}


// ---------------------------------------------------------------------------------- fused-pipeline pieces
// z-forward + y-forward (the x transform is left to the fused x pass)
int fwd_zy(ofdft_ctx* c, const real* in, cplx* spec, hipStream_t st) {
    c->fft_count++;
    int rc = zfwd_any(c, in, spec, st);
    if (rc) return rc;
    return fast_axis_pass<false>(c, 1, spec, st);
}

// y-inverse + z-inverse (c2r) of a spectrum whose x axis is already back in real space
int inv_yz(ofdft_ctx* c, cplx* spec, real* out, double scale, hipStream_t st) {
    c->fft_count++;
    if (int rc = fast_axis_pass<true>(c, 1, spec, st)) return rc;
    return zinv_any(c, spec, out, scale, st);
}

static int dist_rfftn(ofdft_ctx* c, const real* in, cplx* spec, hipStream_t st) {
    cplx *send, *recv, *tmp;
    if (int rc = dist_buffers(c, 0, &send, &recv)) return rc;
    if (int rc = spec_ws(c, "x:tmp", &tmp)) return rc;
    int rc = zfwd_any(c, in, tmp, st);          // z-forward of the local rows into the x-slab layout
    if (rc) return rc;
    if ((rc = ypass_xchg<false>(c, {tmp}, send, st, kWholeXchg))) return rc;   // y-forward, written in the (unchunked) exchange layout
    if ((rc = dist_exchange(c, send, recv, st))) return rc;
    XchgGeom xg = c->xg;
    xg.rec = xg.arr_sz;
    OFDFT_LAUNCH(c, st, "xchg_unpack", xchg_unpack_kernel, dim3(grid_for(c->gx.total)), dim3(256), 0, (const cplx*)recv, spec, c->gx, xg, 0);
    return fast_axis_pass<false>(c, 0, spec, st);                           // x-forward on the y-slab
}

static int dist_irfftn(ofdft_ctx* c, cplx* spec, real* out, double scale, hipStream_t st) {
    cplx *send, *recv, *tmp;
    if (int rc = dist_buffers(c, 0, &send, &recv)) return rc;
    if (int rc = spec_ws(c, "x:tmp", &tmp)) return rc;
    int rc;
    if ((rc = fast_axis_pass<true>(c, 0, spec, st))) return rc;             // x-inverse on the y-slab
    XchgGeom xg = c->xg;
    xg.rec = xg.arr_sz;
    OFDFT_LAUNCH(c, st, "xchg_pack", xchg_unpack_kernel, dim3(grid_for(c->gx.total)), dim3(256), 0, (const cplx*)send, spec, c->gx, xg, 1);
    if ((rc = dist_exchange(c, send, recv, st))) return rc;
    if ((rc = ypass_xchg<true>(c, {tmp}, recv, st, kWholeXchg))) return rc; // y-inverse out of the (unchunked) exchange layout
    return zinv_any(c, tmp, out, scale, st);
}


// The one-pass y operators on an x-slab spectrum in (kz; y, x) form (fft_kernels.h: yderiv_kernel<LEN, ADD, LAP>); `tail`: the
// kernel's trailing arguments
template <bool ADD, bool LAP, class... Tail>
static int yline_op(ofdft_ctx* c, const char* nm, const cplx* in, cplx* out, double scale, hipStream_t st, Tail... tail) {
    return for_len(kLineLens, c->n1, [&](auto L) {
        cplx* tw;
        if (int rc = get_twiddle(c, L(), &tw)) return rc;
        using Cfg = PassCfg<L()>;
        LineMap main, rem;
        pass_maps(c, 1, main, rem);
        const int mb = (main.nlines + Cfg::LPW - 1) / Cfg::LPW, rb = (rem.nlines + Cfg::LPW - 1) / Cfg::LPW;
        OFDFT_LAUNCH(c, st, nm, (yderiv_kernel<L(), ADD, LAP>), dim3(mb + rb), dim3(Cfg::TPB), Cfg::LDS, in, out, main, rem, mb,
                     c->g.main_count, (const cplx*)tw, (real)scale, tail...);
        return 0;
    }, [&] { return fail(c, OFDFT_EINVAL, "unsupported fast FFT length %d", c->n1); });
}
// index derivative along y
int yderiv(ofdft_ctx* c, const cplx* in, cplx* out, double scale, hipStream_t st, cplx* fwd) {
    if (int rc = yline_op<false, false>(c, "yderiv", in, out, scale, st, fwd)) return rc;
    if (fwd) c->fft_passes_fused++, c->yfwd_fused++;
    return 0;
}
// ... plus a y-forwarded spectrum added before the inverse
int yderiv_add(ofdft_ctx* c, const cplx* in, const cplx* add, cplx* out, double scale, hipStream_t st) {
    return yline_op<true, false>(c, "yderiv", in, out, scale, st, (cplx*)nullptr, add);
}
// y part of the Laplacian plus a finished spectrum of the output's layout
int ylap(ofdft_ctx* c, const cplx* in, const cplx* add, cplx* out, double scale, hipStream_t st) {
    return yline_op<false, true>(c, "ylap", in, out, scale, st, (cplx*)nullptr, add);
}


template int fast_axis_pass_multi<false>(ofdft_ctx*, int, cplx* const*, int, hipStream_t);
template int fast_axis_pass_multi<true>(ofdft_ctx*, int, cplx* const*, int, hipStream_t);
template int fast_axis_pass<false>(ofdft_ctx*, int, cplx*, hipStream_t);
template int fast_axis_pass<true>(ofdft_ctx*, int, cplx*, hipStream_t);
template int ypass_xchg<false>(ofdft_ctx*, const std::vector<cplx*>&, cplx*, hipStream_t, int);
template int ypass_xchg<true>(ofdft_ctx*, const std::vector<cplx*>&, cplx*, hipStream_t, int);

}  // namespace eng
