// Where an evaluation's scalar results live: the one definition of the four small blocks of doubles that every pipeline ends in.
// Kernels and host code name these slots; include/ofdft_hip.h publishes the part the ABI shows (OFDFT_NSUMS, OFDFT_NSCALARS,
// OFDFT_SCALAR_SUMSQ, OFDFT_Q_RES_CLOCK*), _native.py mirrors that.  A new term's energy slot is added HERE and in kTermSumSlot (engine.hip).
#pragma once
#include "../../include/ofdft_hip.h"

namespace ofdft {
// ---- 1. the sums of an evaluation (c->d_reduced, the head of the pinned mirror c->h_partial, every host `sums[kNSums]`): what one
// combine kernel accumulates per workgroup, then the three of the GGA mid stage
constexpr int kSumIonElectron = 0, kSumHartree = 1, kSumTf = 2, kSumVw = 3;
constexpr int kSumNl = 4;          // the two-power nonlocal term: Wang-Teter family or OFDFT_NLK (never both: they share the chain)
constexpr int kSumWgc = 5, kSumLdaX = 6;
constexpr int kSumLocalC = 7;      // whichever local correlation flavours are set, together
constexpr int kSumVn = 8;          // sum(v n): mu = kSumVn dV / N_e
constexpr int kSumVwgtf = 9, kCombineScalars = 10;
// energy sums of a GGA pass, in the order its kernels accumulate them, and where they sit among the sums of an evaluation
constexpr int kGgaX = 0, kGgaC = 1, kGgaK = 2, kPbeScalars = 3, kSumGga = kCombineScalars;
constexpr int kSumGgaX = kSumGga + kGgaX, kSumGgaC = kSumGga + kGgaC, kSumGgaK = kSumGga + kGgaK;
constexpr int kNSums = kCombineScalars + kPbeScalars;      // 13

// Term bits as the combine kernels test them.  Their mask is combine_mask(c) (engine_ctx.h), not c->mask: OFDFT_NLK is folded onto OFDFT_WT_NL there.
constexpr unsigned kLocalXcAny = OFDFT_LDA_X | OFDFT_PZ_C | OFDFT_PW_C | OFDFT_CHACHIYO_C;
constexpr unsigned kGgaAny = OFDFT_PBE_X | OFDFT_PBE_C | OFDFT_GGA_K;   // terms served by the gradient / divergence machinery

// ---- 2. beyond the sums in c->d_reduced: sum chi^2 of the closure form, and the length of the block ofdft_dist_scalars publishes
constexpr int kSumsqSlot = 15, kReducedLen = 16;

// ---- 3. beyond the sums in the pinned mirror c->h_partial
constexpr int kMirrorWgcSplit = kNSums;           // energy sum of the split WGC99 kernel (zi_wgc_kernel) ...
constexpr int kMirrorWgcSplitVn = kNSums + 1;     // ... and its share of sum(v n); zfused_collect adds both to their sums
constexpr int kMirrorResTimeout = kNSums;         // persistent kernel: 1.0 if one of its grid barriers ran out of patience
constexpr int kMirrorResClock = 16;               // persistent kernel built with OFDFT_RES_CLOCK: phase clock of workgroup 0,
constexpr int kResClockCount = 12;                //   kResClockCount values in hundredths of a microsecond (100 MHz ticks)
// kMirrorWgcSplit and kMirrorResTimeout are ONE slot.  No evaluation writes both: only the z-fused staged pipeline launches the
// split kernel (zstep_mid), only the persistent kernel writes the flag, and an evaluation it serves runs no staged stage.  Each
// writes the slot before the host reads it: workgroup 0 stores the flag in phase D of every launch, ahead of the count-out the
// host waits for, and the host reads it only straight after such a launch; a staged evaluation reads the slot only with
// kCollectWgcSplit set, i.e. after its own split kernel's reduction.  (The ipc closure's copy also lands there; it reads neither.)

// ---- 4. c->d_scal: device-resident scalars that are no sums
constexpr int kScalClosure = 0;         // closure scale c of n = c chi^2
constexpr int kScalWgcSplit = 2;        // split WGC99 kernel: energy sum ...
constexpr int kScalWgcSplitVn = 3;      // ... and its share of sum(v n) (chi_grad adds it to kSumVn on the device)
constexpr int kScalWts = 4, kScalWtsCount = 3;      // stabilised WT-style functional: f - f' X, f', f (wts_weights_kernel)
constexpr int kScalLen = 8;

static_assert(kNSums == OFDFT_NSUMS && kReducedLen == OFDFT_NSCALARS && kSumsqSlot == OFDFT_SCALAR_SUMSQ, "published layout");
static_assert(kMirrorResClock == OFDFT_Q_RES_CLOCK && kResClockCount == OFDFT_Q_RES_CLOCK_COUNT, "the clock is queried by its mirror slot");
static_assert(kMirrorWgcSplit >= kNSums && kMirrorResTimeout >= kNSums, "the mirror's extras start behind the sums");
static_assert(kMirrorWgcSplitVn == kMirrorWgcSplit + 1 && kScalWgcSplitVn == kScalWgcSplit + 1, "one two-value reduction writes the pair");
static_assert(kMirrorWgcSplitVn < kSumsqSlot && kSumsqSlot < kReducedLen && kMirrorWgcSplitVn < kMirrorResClock, "sum chi^2 and the clock lie beyond the other extras");
static_assert(kScalWgcSplit > kScalClosure && kScalWts > kScalWgcSplitVn && kScalWts + kScalWtsCount <= kScalLen, "d_scal");

}  // namespace ofdft
