// Fused x passes, part B: density / gradient / Laplacian mixes.  gfx950 only.
#include "xpass_impl.h"

namespace eng {
template int xfused<1, 1, MixDensity<true, false>>(ofdft_ctx*, const XfIo&, const MixDensity<true, false>&, hipStream_t, const char*, const XfLayout&);
template int xfused<1, 3, MixDensity<false, true>>(ofdft_ctx*, const XfIo&, const MixDensity<false, true>&, hipStream_t, const char*, const XfLayout&);
template int xfused<1, 4, MixDensity<true, true>>(ofdft_ctx*, const XfIo&, const MixDensity<true, true>&, hipStream_t, const char*, const XfLayout&);
template int xfused<1, 1, MixDensityA<false, false>>(ofdft_ctx*, const XfIo&, const MixDensityA<false, false>&, hipStream_t, const char*, const XfLayout&);
template int xfused<1, 2, MixDensityA<true, false>>(ofdft_ctx*, const XfIo&, const MixDensityA<true, false>&, hipStream_t, const char*, const XfLayout&);
template int xfused<1, 2, MixDensityA<false, true>>(ofdft_ctx*, const XfIo&, const MixDensityA<false, true>&, hipStream_t, const char*, const XfLayout&);
template int xfused<1, 3, MixDensityA<true, true>>(ofdft_ctx*, const XfIo&, const MixDensityA<true, true>&, hipStream_t, const char*, const XfLayout&);
// OFDFT_OPT_AXIS_PASSES: D_a n from the z spectrum; what is left of the density pass beside a Laplacian-dependent GGA member
template int xfused<1, 1, MixDerivAS>(ofdft_ctx*, const XfIo&, const MixDerivAS&, hipStream_t, const char*, const XfLayout&);
template int xfused<1, 2, MixDensityA<true, true, false>>(ofdft_ctx*, const XfIo&, const MixDensityA<true, true, false>&, hipStream_t, const char*, const XfLayout&);

extern template int xfused<3, 3, MixWgc>(ofdft_ctx*, const XfIo&, const MixWgc&, hipStream_t, const char*, const XfLayout&);      // xpass_a.hip
int xfused_wgc(ofdft_ctx* c, const XfIo& io, const MixWgc& mix, hipStream_t st, const char* nm, const XfLayout& lay) {
    if (cell_axes_orthogonal(c) && c->wgc_fold && xcross_wanted(c, 3 + 3)) {
        // (the folded mix exists in the other two families only where the cross-wave kernel hands the pass on to them)
        MixWgcFold f;
        static_cast<MixWgc&>(f) = mix;
        f.fold_n0 = c->n0g;
        return xpass_run<3, 3>(c, io, f, lay, st, nm, kXcToWaveLens, kXcToGroupLens);
    }
    return xfused<3, 3, MixWgc>(c, io, mix, st, nm, lay);
}
}  // namespace eng
