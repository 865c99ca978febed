// Launchers of the fused x passes (xfused_kernel in fft_kernels.h, xw_kernel in xwave.h, xc_kernel in xcross.h): included by
// xpass_a.hip and xpass_b.hip, which instantiate them for the mix functors of the pipelines.
#pragma once
#include "engine_ctx.h"
#include "xcross.h"

namespace eng {

// line maps of a fused x pass and the geometry its kernel sees: the block-8 arrays (one GPU), or the records of the chunk of an
// exchange buffer that `lay` addresses
inline void xpass_maps(const ofdft_ctx* c, const XfLayout& lay, LineMap& main, LineMap& rem, SpecGeom& gk) {
    if (!lay.se_in) return pass_maps(c, 0, main, rem);
    const int nyl = c->xg.nyl;
    const int xnb = lay.xnb >= 0 ? lay.xnb : c->xg.nb, xnrem = lay.xnb >= 0 ? lay.xnrem : c->xg.nrem;   // this chunk's share
    main.d = nyl * 8; main.sb = nyl * 8; main.sl = 1; main.se = lay.se_in; main.nlines = xnb * nyl * 8;
    main.kz0 = lay.kz0;
    rem.d = nyl; rem.sb = nyl; rem.sl = 1; rem.se = lay.se_in; rem.nlines = xnrem * nyl;
    if (main.nlines == 0) main.d = 1;
    if (rem.nlines == 0) rem.d = 1;
    gk.main_count = (long long)xnb * nyl * 8;          // offset of the plane part inside a record
}

// ---- which kernel family takes a pass (OFDFT_OPT_XWAVE: the kXw* values of engine_ctx.h).  The one place that decides.
// measured at 256^3 (A/B on one box): 3 -> 3 (WGC99) 0.55 -> 0.53 ms, 1 -> 2 0.112 -> 0.097 ms, but 1 -> 1 0.062 -> 0.079 ms
// (at 512 points per line the wave-local kernel -- one line per wave: 16 useful bytes per cache line and load -- costs 1.5 x its
// 256-point self per grid point, tools/shape_probe.py, and the group-parallel kernel is faster ALONE, 5.4 vs 6.3 ms for the WGC99
// pair at 512^3; with the two chains overlapped the evaluation is nevertheless 3-4 % faster with the wave-local one, 24.6-25.0 vs
// 25.8-25.9 ms in two alternations on one box: option value 4 selects the group-parallel kernel at 512 for A/B)
// cross-wave kernel (xcross.h; round 4).  Measured on one box, WGC99 pair / 1 -> 2 / 1 -> 1 passes, us per evaluation:
//   256^3: 537 -> 405 / 103 -> 92 / 61-69 -> 58-62;  512^3: 6200 -> 3800 / 1180 -> 920 / 570-600 -> 535-560;
//   1024 x 128 x 128: 920 -> 670 / 197 -> 140 but 90-94 -> 101-106 for the 1 -> 1 passes;  128^3: neutral to 3 % slower.
// option 1 (default): 256- and 512-point lines always, 1024-point lines for passes over >= 3 spectra;
// 5 = wherever it exists (128..1024), 6 = passes over >= 3 spectra only, 7 = the round-3 choice (no cross-wave kernel)
// (fp32 build, 256-point lines: the 1 -> 1 passes measured 36-37 us in the group-parallel kernel against 39-40 here)
// (fp32 build, 1024-point lines -- config 5 -- with two lines per lane: every pass, 1 -> 1 included: 205-220 us against 264-272 in
// the group-parallel kernel at 1024 x 256 x 256, the Lindhard mix 5.8 against 5.9 ms at 1024^3; profiles/r04_x_stride_probe.jsonl)

// does the option want the cross-wave kernel for a pass over nspec = NIN + NOUT spectra?
inline bool xcross_wanted(const ofdft_ctx* c, int nspec) {
    constexpr bool f32 = sizeof(real) == 4;
    const int n = c->n0g, u = c->use_xwave;
    if (!has_len(kXcrossLens, n)) return false;
    if (u == kXwCrossAll) return true;
    if (u == kXwCross3) return nspec >= 3;
    if (u != kXwMeasured) return false;
    if (n == 256) return !(f32 && nspec == 2);
    return n == 512 || (n == 1024 && (nspec >= 3 || f32));
}
// ... the wave-local one?
inline bool xwave_wanted(const ofdft_ctx* c, int nspec) {
    const int u = c->use_xwave;
    return u == kXwWaveAll || ((u == kXwMeasured || u >= kXwCrossAll || (u == kXwGroupAt512 && c->n0g < 512)) && nspec >= 3);
}
// A pass the option gives to the cross-wave kernel leaves it again where lanes own NL > 1 memory-adjacent lines (fp32 build) and
// the lines do not come in whole groups of NL: for the wave-local kernel up to 512 points, the group-parallel one at 1024.
// The lengths of those hand-overs (empty in the fp64 build: nothing is instantiated for them):
constexpr bool kXcHandsOn = XcCfg<1024>::NL > 1;
constexpr auto kXcToWaveLens = std::conditional_t<kXcHandsOn, decltype(within<0, 512>(kXcrossLens)), Lens<>>{};
constexpr auto kXcToGroupLens = std::conditional_t<kXcHandsOn, decltype(within<513, 1024>(kXcrossLens)), Lens<>>{};

// The family that takes the pass over `nin` input and `nout` output spectra found through `lay`.  A mix that integrates an energy
// has no group-parallel kernel: XKind::None says that nothing serves the pass (xfused_energy_serves).
inline XKind xpass_choice(const ofdft_ctx* c, const XfLayout& lay, int nin, int nout, bool energy) {
    const int n = c->n0g, nspec = nin + nout;
    if (xcross_wanted(c, nspec)) {
        const int NL = for_len(kXcrossLens, n, [](auto L) { return XcCfg<decltype(L)::value>::NL; }, [] { return 1; });
        if (NL > 1) {          // lanes own groups of memory-adjacent lines: whole groups only
            LineMap main, rem;
            SpecGeom gk = c->gx;
            xpass_maps(c, lay, main, rem, gk);
            if (main.sl != 1 || rem.sl != 1 || main.d % NL || rem.d % NL || main.nlines % NL || rem.nlines % NL)
                return has_len(kXwaveLens, n) ? XKind::Wave : energy ? XKind::None : XKind::Group;
        }
        return XKind::Cross;
    }
    if (xwave_wanted(c, nspec) && has_len(kXwaveLens, n)) return XKind::Wave;
    return !energy && has_len(kLineLens, n) ? XKind::Group : XKind::None;
}

// ---- one frame for the three families: twiddle table, line maps, block counts, the bookkeeping of OFDFT_Q_XPASS_KINDS
template <XKind K, int LEN, int NIN, int NOUT> struct XpCfg;
template <int LEN, int NIN, int NOUT> struct XpCfg<XKind::Group, LEN, NIN, NOUT> {      // spectra traded through LDS
    using Cfg = XfCfg<LEN, (NIN > NOUT ? NIN : NOUT), NOUT>;
    static constexpr int LPB = Cfg::LPW, TPB = Cfg::TPB;
    static constexpr size_t LDS = Cfg::LDS;
    static constexpr unsigned kind = OFDFT_XPASS_GROUP;
};
template <int LEN, int NIN, int NOUT> struct XpCfg<XKind::Wave, LEN, NIN, NOUT> {       // a line of every spectrum in the lanes of one wave
    static constexpr int LPB = XwCfg<LEN>::LPB, TPB = XwCfg<LEN>::TPB;
    static constexpr size_t LDS = XwCfg<LEN>::LDS;
    static constexpr unsigned kind = OFDFT_XPASS_WAVE;
};
template <int LEN, int NIN, int NOUT> struct XpCfg<XKind::Cross, LEN, NIN, NOUT> {      // whole runs of memory-adjacent lines per access
    static constexpr int LPB = XcCfg<LEN>::LPB, TPB = XcCfg<LEN>::TPB;
    static constexpr size_t LDS = XcCfg<LEN>::lds_bytes(xc_one_buffer<LEN, NIN, NOUT>());
    static constexpr unsigned kind = XcCfg<LEN>::NL == 2 ? OFDFT_XPASS_CROSS2 : OFDFT_XPASS_CROSS1;
};

template <XKind K, int LEN, int NIN, int NOUT, class Mix>
int launch_xpass_t(ofdft_ctx* c, const XfIo& io, const Mix& mix, const XfLayout& lay, hipStream_t st, const char* nm) {
    using Cfg = XpCfg<K, LEN, NIN, NOUT>;
    cplx* tw;
    if (int rc = get_twiddle(c, LEN, &tw)) return rc;
    LineMap main, rem;
    SpecGeom gk = c->gx;
    xpass_maps(c, lay, main, rem, gk);
    main.lf = rem.lf = Cfg::LPB;
    const int mb = (main.nlines + Cfg::LPB - 1) / Cfg::LPB, rb = (rem.nlines + Cfg::LPB - 1) / Cfg::LPB;
    const XfStride xs{lay.se_out, lay.tse};
    if constexpr (K == XKind::Cross && Cfg::LDS > 64 * 1024) {          // more dynamic LDS than the default limit: declared once per kernel and device
        static bool declared[64] = {};
        const int dv = c->device & 63;
        if (!declared[dv]) {
            HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&xc_kernel<LEN, NIN, NOUT, Mix>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)Cfg::LDS));
            declared[dv] = true;
        }
    }
    c->xpass_kinds |= Cfg::kind;
    c->xpass_blocks = mb + rb;
    if constexpr (K == XKind::Group)
        OFDFT_LAUNCH(c, st, nm, (xfused_kernel<LEN, NIN, NOUT, Mix>), dim3(mb + rb), dim3(Cfg::TPB), Cfg::LDS, io, main, rem, mb, gk,
                     (const cplx*)tw, mix, xs);
    else if constexpr (K == XKind::Wave)
        OFDFT_LAUNCH(c, st, nm, (xw_kernel<LEN, NIN, NOUT, Mix>), dim3(mb + rb), dim3(Cfg::TPB), Cfg::LDS, io, main, rem, mb, gk,
                     (const cplx*)tw, mix, xs);
    else
        OFDFT_LAUNCH(c, st, nm, (xc_kernel<LEN, NIN, NOUT, Mix>), dim3(mb + rb), dim3(Cfg::TPB), Cfg::LDS, io, main, rem, mb, gk,
                     (const cplx*)tw, mix, xs);
    return 0;
}

// the pass in the family xpass_choice names, at the length of the x lines.  wave_lens / group_lens: the lengths this mix is
// instantiated for in those two families (a mix with an energy never in the group-parallel one)
template <int NIN, int NOUT, class Mix, class WaveLens, class GroupLens>
int xpass_run(ofdft_ctx* c, const XfIo& io, const Mix& mix, const XfLayout& lay, hipStream_t st, const char* nm, WaveLens wave_lens,
              GroupLens group_lens) {
    constexpr bool energy = mix_has_energy<Mix>::value;
    auto miss = [&] {
        return energy ? fail(c, OFDFT_EINVAL, "%s: no energy-integrating x pass for %d-point lines", nm, c->n0g)
                      : fail(c, OFDFT_EINVAL, "unsupported fast FFT length %d", c->n0g);
    };
    auto run = [&](auto family, auto lens) {
        return for_len(lens, c->n0g, [&](auto L) {
            return launch_xpass_t<decltype(family)::value, decltype(L)::value, NIN, NOUT, Mix>(c, io, mix, lay, st, nm);
        }, miss);
    };
    const XKind k = xpass_choice(c, lay, NIN, NOUT, energy);
    if (k == XKind::Cross) return run(std::integral_constant<XKind, XKind::Cross>{}, kXcrossLens);
    if (k == XKind::Wave) return run(std::integral_constant<XKind, XKind::Wave>{}, wave_lens);
    if constexpr (!energy)
        if (k == XKind::Group) return run(std::integral_constant<XKind, XKind::Group>{}, group_lens);
    return miss();
}

// forward-x, k-space mix, inverse-x in one pass over NIN input / NOUT output spectra
template <int NIN, int NOUT, class Mix>
int xfused(ofdft_ctx* c, const XfIo& io, const Mix& mix, hipStream_t st, const char* nm, const XfLayout& lay) {
    return xpass_run<NIN, NOUT>(c, io, mix, lay, st, nm, kXwaveLens, kLineLens);
}

// a pass whose mix integrates an energy (mix_has_energy): the cross-wave or wave-local kernel only
template <int NIN, class Mix>
int xfused_energy(ofdft_ctx* c, const XfIo& io, const Mix& mix, hipStream_t st, const char* nm) {
    static_assert(mix_has_energy<Mix>::value, "xfused_energy: a mix with an energy");
    return xpass_run<NIN, 1>(c, io, mix, XfLayout{}, st, nm, kXwaveLens, Lens<>{});
}

}  // namespace eng
