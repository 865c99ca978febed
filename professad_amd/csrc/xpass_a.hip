// Fused x passes, part A: table-driven (WGC99) and single-spectrum mixes, and the divergence passes (with the Hartree potential
// and E_H folded in: xfused_energy).  gfx950 only.
#include "xpass_impl.h"

namespace eng {
template int xfused<3, 3, MixWgc>(ofdft_ctx*, const XfIo&, const MixWgc&, hipStream_t, const char*, const XfLayout&);
template int xfused<1, 1, MixScale<SPEC_LAPLACE>>(ofdft_ctx*, const XfIo&, const MixScale<SPEC_LAPLACE>&, hipStream_t, const char*, const XfLayout&);
template int xfused<1, 1, MixScale<SPEC_LAPLACE_AC>>(ofdft_ctx*, const XfIo&, const MixScale<SPEC_LAPLACE_AC>&, hipStream_t, const char*, const XfLayout&);
template int xfused<1, 1, MixScale<SPEC_LINDHARD>>(ofdft_ctx*, const XfIo&, const MixScale<SPEC_LINDHARD>&, hipStream_t, const char*, const XfLayout&);
template int xfused<1, 1, MixNlk<1>>(ofdft_ctx*, const XfIo&, const MixNlk<1>&, hipStream_t, const char*, const XfLayout&);
template int xfused<2, 2, MixNlk<2>>(ofdft_ctx*, const XfIo&, const MixNlk<2>&, hipStream_t, const char*, const XfLayout&);
template int xfused<1, 1, MixDerivA>(ofdft_ctx*, const XfIo&, const MixDerivA&, hipStream_t, const char*, const XfLayout&);
template int xfused<2, 1, MixDerivAL>(ofdft_ctx*, const XfIo&, const MixDerivAL&, hipStream_t, const char*, const XfLayout&);
template int xfused_energy<2, MixDerivAH<false>>(ofdft_ctx*, const XfIo&, const MixDerivAH<false>&, hipStream_t, const char*);
template int xfused_energy<3, MixDerivAH<true>>(ofdft_ctx*, const XfIo&, const MixDerivAH<true>&, hipStream_t, const char*);
template int xfused<3, 1, MixDiv>(ofdft_ctx*, const XfIo&, const MixDiv&, hipStream_t, const char*, const XfLayout&);
// exactly where xfused<nin, 1> itself would take the cross-wave or the wave-local kernel (OFDFT_OPT_XWAVE is honoured; the NL = 2
// fallback of launch_xc_t of the fp32 build leads to the wave-local kernel up to 512 points, to the group-parallel one at 1024)
bool xfused_energy_serves(const ofdft_ctx* c, int nin) {
    const bool xc = nin == 2 ? xc_serves<2, 1>(c) : xc_serves<3, 1>(c);
    const bool xc_len = c->n0g == 128 || c->n0g == 256 || c->n0g == 512 || c->n0g == 1024;
    const bool xw = c->use_xwave == 2 || c->use_xwave == 1 || c->use_xwave >= 5 || (c->use_xwave == 4 && c->n0g < 512);   // (nin + 1 >= 3)
    if (xc && xc_len && XcCfg<1024>::NL > 1 && c->n0g == 1024) {     // the fallback of launch_xc_t at 1024 points is the group-parallel kernel
        LineMap m, r;
        pass_maps(c, 0, m, r);
        constexpr int NL = XcCfg<1024>::NL;
        if (m.sl != 1 || r.sl != 1 || m.d % NL || r.d % NL || m.nlines % NL || r.nlines % NL) return false;
    }
    return (xc && xc_len) || (xw && is_pow2(c->n0g) && c->n0g >= 8 && c->n0g <= 512);
}
}  // namespace eng
