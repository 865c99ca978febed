// Fused x passes, part A: table-driven (WGC99) and single-spectrum mixes, and the divergence passes (with the Hartree potential
// and E_H folded in: xfused_energy).  gfx950 only.
#include "xpass_impl.h"

namespace eng {
template int xfused<3, 3, MixWgc>(ofdft_ctx*, const XfIo&, const MixWgc&, hipStream_t, const char*, const XfLayout&);
template int xfused<1, 1, MixScale<SPEC_LAPLACE>>(ofdft_ctx*, const XfIo&, const MixScale<SPEC_LAPLACE>&, hipStream_t, const char*, const XfLayout&);
template int xfused<1, 1, MixScale<SPEC_LAPLACE_AC>>(ofdft_ctx*, const XfIo&, const MixScale<SPEC_LAPLACE_AC>&, hipStream_t, const char*, const XfLayout&);
#ifndef OFDFT_REAL_F32      // ofdft_precondition: fp64 library only
template int xfused<1, 1, MixScale<SPEC_SCREENED>>(ofdft_ctx*, const XfIo&, const MixScale<SPEC_SCREENED>&, hipStream_t, const char*, const XfLayout&);
#endif
template int xfused<1, 1, MixScale<SPEC_LINDHARD>>(ofdft_ctx*, const XfIo&, const MixScale<SPEC_LINDHARD>&, hipStream_t, const char*, const XfLayout&);
template int xfused<1, 1, MixNlk<1>>(ofdft_ctx*, const XfIo&, const MixNlk<1>&, hipStream_t, const char*, const XfLayout&);
template int xfused<2, 2, MixNlk<2>>(ofdft_ctx*, const XfIo&, const MixNlk<2>&, hipStream_t, const char*, const XfLayout&);
template int xfused<1, 1, MixDerivA>(ofdft_ctx*, const XfIo&, const MixDerivA&, hipStream_t, const char*, const XfLayout&);
template int xfused<2, 1, MixDerivAL>(ofdft_ctx*, const XfIo&, const MixDerivAL&, hipStream_t, const char*, const XfLayout&);
template int xfused_energy<2, MixDerivAH<false>>(ofdft_ctx*, const XfIo&, const MixDerivAH<false>&, hipStream_t, const char*);
template int xfused_energy<3, MixDerivAH<true>>(ofdft_ctx*, const XfIo&, const MixDerivAH<true>&, hipStream_t, const char*);
template int xfused<3, 1, MixDiv>(ofdft_ctx*, const XfIo&, const MixDiv&, hipStream_t, const char*, const XfLayout&);
bool xfused_energy_serves(const ofdft_ctx* c, int nin) { return xpass_choice(c, XfLayout{}, nin, 1, true) != XKind::None; }
}  // namespace eng
