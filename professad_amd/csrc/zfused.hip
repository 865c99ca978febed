// Launchers of the wave-local z kernels with fused real-space physics (zpass.h).  gfx950 only.
// (fp32 build: this unit's kernels -- the wave-local z kernels -- use the packed complex arithmetic of fft_radix.h: zf_density -9 %,
// zi_combine -5 %, zpbe -6 %, zi_wgc +8 % at their sizes of BASELINE configs 3 / 5, profiles/r05_ab_f32_packed.jsonl; every other
// unit keeps the component-wise forms, which the chirp-z kernels of lines.hip need)
#if defined(OFDFT_REAL_F32) && !defined(OFDFT_F32_PK)
#define OFDFT_F32_PK 1
#endif
#include "engine_ctx.h"

namespace eng {

#ifndef OFDFT_EZ
#define OFDFT_EZ 4
#endif
constexpr int EZ = OFDFT_EZ;   // points per lane wanted by the register-hungry fused z kernels
#ifndef OFDFT_EZ_POWERS
#define OFDFT_EZ_POWERS OFDFT_EZ
#endif
constexpr int EZP = OFDFT_EZ_POWERS;   // ... and by zf_powers (one input row, up to six output spectra)

// One frame for the launchers: the twiddle tables of the rows, the ZW<M, ZPick<M, EW>::E> pick for the rows' half length M (EW =
// points per lane wanted), the block count (also to *blocks_out, if given) and the launch, which `launch` makes as
// launch(M tag, E tag, blocks, LDS bytes of the pick, twM, twN)
template <int EW, class F>
static int z_launch(ofdft_ctx* c, int* blocks_out, F&& launch) {
    cplx *twM, *twN;
    if (int rc = get_twiddle(c, c->n2 / 2, &twM)) return rc;
    if (int rc = get_twiddle(c, c->n2, &twN)) return rc;
    return for_len(kZFusedLens, c->n2 / 2, [&](auto M) {
        using W = ZW<M(), ZPick<M(), EW>::E>;
        const int nb = (int)((c->g.nrows + W::RPB - 1) / W::RPB);
        if (blocks_out) *blocks_out = nb;
        launch(M, std::integral_constant<int, W::E>{}, nb, (size_t)W::LDS, twM, twN);
        return 0;
    }, [&] { return fail(c, OFDFT_EINVAL, "bad n2"); });
}

int launch_zf_density(ofdft_ctx* c, const DenSrc& ds, cplx* out_n, cplx* out_s, hipStream_t st, real* dzn) {
    c->fft_count += (out_n ? 1 : 0) + (out_s ? 1 : 0);
    return z_launch<8>(c, nullptr, [&](auto M, auto E, int nb, size_t lds, cplx* twM, cplx* twN) {
        OFDFT_LAUNCH(c, st, "zf_density", (zf_density_kernel<M(), E()>), dim3(nb), dim3(256), lds, ds, out_n, out_s, c->g, twM, twN, dzn);
    });
}

int launch_zf_powers(ofdft_ctx* c, const DenSrc& ds, const PowersArgs& pa, hipStream_t st) {
    for (int i = 0; i < 6; ++i) c->fft_count += pa.out[i] ? 1 : 0;
    const bool one = pa.out[0] && !pa.out[1] && !pa.out[2] && !pa.out[3] && !pa.out[4] && !pa.out[5];
    return z_launch<EZP>(c, nullptr, [&](auto M, auto E, int nb, size_t lds, cplx* twM, cplx* twN) {
        if (one) OFDFT_LAUNCH(c, st, "zf_powers", (zf_powers_kernel<M(), E(), true>), dim3(nb), dim3(256), lds, ds, pa, c->g, twM, twN);
        else OFDFT_LAUNCH(c, st, "zf_powers", (zf_powers_kernel<M(), E()>), dim3(nb), dim3(256), lds, ds, pa, c->g, twM, twN);
    });
}

int launch_zpbe(ofdft_ctx* c, const DenSrc& ds, cplx* gx, cplx* gy, cplx* gz, real* dfdn, double inv_n,
                int* blocks_out, hipStream_t st) {
    c->fft_count += 6;    // three c2r finished + three r2c started on chip
    return z_launch<EZ>(c, blocks_out, [&](auto M, auto E, int nb, size_t lds, cplx* twM, cplx* twN) {
        OFDFT_LAUNCH(c, st, "zpbe", (zpbe_kernel<M(), E()>), dim3(nb), dim3(256), lds, ds, gx, gy, gz, dfdn, inv_n, gga_sel(c), c->g,
                     twM, twN, c->d_partial);
    });
}

// split-derivative GGA mid stage (zpass.h: zpbe2_kernel); L != nullptr: the Laplacian-dependent Pauli-Gaussian form
int launch_zpbe2(ofdft_ctx* c, const DenSrc& ds, cplx* A, cplx* B, const real* dzn, real* dfdn, double inv_n,
                 int* blocks_out, hipStream_t st, cplx* L) {
    c->fft_count += L ? 8 : 6;    // same six 3-D transforms as the plain form (three c2r finished, three r2c started); + lap n, df/dL
    Bmat bm{};
    std::memcpy(bm.b, c->kg.b, sizeof(bm.b));
    return z_launch<EZ>(c, blocks_out, [&](auto M, auto E, int nb, size_t lds, cplx* twM, cplx* twN) {
        if (L)
            OFDFT_LAUNCH(c, st, "zpbe", (zpbe2_kernel<M(), E(), true>), dim3(nb), dim3(256), lds, ds, A, B, dzn, dfdn, inv_n,
                         1.0 / (double)c->n2, gga_sel(c), bm, c->g, twM, twN, c->d_partial, L);
        else
            OFDFT_LAUNCH(c, st, "zpbe", (zpbe2_kernel<M(), E(), false>), dim3(nb), dim3(256), lds, ds, A, B, dzn, dfdn, inv_n,
                         1.0 / (double)c->n2, gga_sel(c), bm, c->g, twM, twN, c->d_partial, L);
    });
}

int launch_zi_combine(ofdft_ctx* c, const ZCombineArgs& a, int* blocks_out, hipStream_t st) {
    const size_t park = sizeof(real) * 256 * kParkSlots;
    const bool lean = a.v_part || !(a.mask & OFDFT_WGC99_NL);     // no inline WGC99 section needed: the lean instantiation
    return z_launch<EZ>(c, blocks_out, [&](auto M, auto E, int nb, size_t lds, cplx* twM, cplx* twN) {
        if (lean)
            OFDFT_LAUNCH(c, st, "zi_combine", (zi_combine_kernel<M(), E(), false>), dim3(nb), dim3(256), lds + park, a, c->g, twM, twN,
                         c->d_partial);
        else
            OFDFT_LAUNCH(c, st, "zi_combine", (zi_combine_kernel<M(), E(), true>), dim3(nb), dim3(256), lds + park, a, c->g, twM, twN,
                         c->d_partial);
    });
}

// split form: the WGC99 part of the combine on the nonlocal chain's stream -> v_part rows + one energy partial per block
int launch_zi_wgc(ofdft_ctx* c, const ZCombineArgs& a, real* v_part, double* partial, int* blocks_out, hipStream_t st) {
    return z_launch<EZ>(c, blocks_out, [&](auto M, auto E, int nb, size_t lds, cplx* twM, cplx* twN) {
        OFDFT_LAUNCH(c, st, "zi_wgc", (zi_wgc_kernel<M(), E()>), dim3(nb), dim3(256), lds, a, v_part, c->g, twM, twN, partial);
    });
}


}  // namespace eng
