// The transform lengths the hand-written line kernels are instantiated for, stated once per kernel family.
//
// Every line transform is a template on its length.  A family's list here is BOTH its predicate (has_len: is this extent served?)
// and its dispatch (for_len: call the instantiation for this length), so the two cannot disagree.  To serve another length: add
// it to the family's list below and give the kernel its plan for it (fft_radix.h: Plan, ZPick; zpass.h: ZW; xwave.h: XwPlan, XwSwz;
// xcross.h: XcWaves); no other host text names lengths.
#pragma once
#include <type_traits>

namespace eng {

template <int... L> struct Lens {};
template <int... A, int... B> constexpr Lens<A..., B...> operator+(Lens<A...>, Lens<B...>) { return {}; }
template <int... A> constexpr Lens<(A / 2)...> halved(Lens<A...>) { return {}; }
// the members in [LO, HI]
template <int LO, int HI> constexpr Lens<> within(Lens<>) { return {}; }
template <int LO, int HI, int A, int... R> constexpr auto within(Lens<A, R...>) {
    if constexpr (LO <= A && A <= HI) return Lens<A>{} + within<LO, HI>(Lens<R...>{});
    else return within<LO, HI>(Lens<R...>{});
}
template <int MAX, int... A> constexpr auto upto(Lens<A...> l) { return within<0, MAX>(l); }

// is n in the list?
template <int... L> constexpr bool has_len(Lens<L...>, int n) { return ((n == L) || ...); }
// f(std::integral_constant<int, n>) for the member equal to n -- f instantiates and launches the kernel for that length and returns
// its status; no such member: miss() (the site's fail())
template <int... L, class F, class Miss> int for_len(Lens<L...>, int n, F&& f, Miss&& miss) {
    int rc = 0;
    const bool hit = ((n == L && ((rc = f(std::integral_constant<int, L>{})), true)) || ...);
    return hit ? rc : miss();
}

constexpr Lens<8, 16, 32, 64, 128, 256, 512, 1024> kPow2Lens;
// the 2^a 3^b 5^c x / y extents with a plan (fft_radix.h).  Both precisions since round 3; OFDFT_NO_MIXED_F32 restores the round-2
// fp32 build, whose other extents took the chirp-z path
#if !defined(OFDFT_REAL_F32) || !defined(OFDFT_NO_MIXED_F32)
constexpr Lens<48, 96, 120, 144, 160, 192, 240, 250, 270, 288, 320, 384, 480> kMixedLens;
#else
constexpr Lens<> kMixedLens;
#endif

// register / LDS line plans: cpass, ypass_xchg, yderiv / ylap and the group-parallel fused x pass
constexpr auto kLineLens = kPow2Lens + kMixedLens;
// fused x pass, wave-local (xwave.h) and cross-wave (xcross.h) kernels
constexpr auto kXwaveLens = upto<512>(kPow2Lens);
constexpr Lens<128, 256, 512, 1024> kXcrossLens;
// z rows (zfwd, zinv), by their HALF length n2 / 2: the same extents along z
constexpr auto kZRowLens = kPow2Lens + halved(kMixedLens);
// wave-local z kernels with fused real-space physics (zfused.hip), by half length
constexpr auto kZFusedLens = upto<512>(kZRowLens);
// chirp-z transforms, by PADDED length (bluestein_pad): the generic pass, the fused x pass, the fused z / y pass of small grids
constexpr auto kChirpLens = kPow2Lens;
constexpr auto kChirpXmixLens = upto<512>(kPow2Lens);
constexpr auto kChirpZyLens = upto<128>(kPow2Lens);
// persistent small-grid kernel (resident.hip): cubic grids of these extents
constexpr Lens<16, 32, 64> kResidentLens;

// extents the fused pipelines take (any other: chirp-z line transforms + the unfused pipeline)
inline bool line_extent_ok(int n) { return has_len(kLineLens, n); }
inline bool row_extent_ok(int n2) { return n2 % 2 == 0 && has_len(kZRowLens, n2 / 2); }

}  // namespace eng
