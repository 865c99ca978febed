// The z-fused pipeline of the engine (five stages, two chains; single- and multi-GPU) and the launchers of the z
// kernels.  Included once by engine.hip inside its anonymous namespace (one translation unit).
// ---------------------------------------------------------------------------------- z-fused pipeline (zpass.h)
// Pipeline with every real-space intermediate kept on chip: z kernels compute their inputs from chi|n on the
// fly and consume the convolution results straight out of the inverse transform.  It is written as five
// stages separated by the four points where the spectra change between the x-slab geometry (z, y passes) and
// the x-pass geometry: on one GPU the two coincide and the stages simply run back to back; on several GPUs
// each boundary is one all-to-all over the listed arrays (the host does the collective, see ofdft_dist_*).
//   stage 1  z-forward (+pointwise pre-ops) and y-forward of every input spectrum          -> exchange
//   stage 2  fused x passes (Hartree, gradient, Laplacian, Lindhard / WGC99 mixing)         -> exchange
//   stage 3  y-inverse of the results; PBE mid stage on chip; y-forward of the flux          -> exchange
//   stage 4  fused x pass of the divergence                                                  -> exchange
//   stage 5  y-inverse of the divergence; combine kernel (potential + energy integrands)
// Every driver sequences the same six steps per chain, each on one kz chunk of the exchange layout (zstep; one GPU: chunk 0),
// then zcombine.  A step that sends leaves its chunk in the chain's send buffer; a y-inverse step reads the receive buffer and
// is a no-op on one GPU, where the mid stage and the combine y-invert in place instead:
//   kStepYFwd     [chunk 0: z kernels]  y-forward of the chunk                              (stage 1)  sends
//   kStepX        fused x passes of the chunk                                               (stage 2)  sends
//   kStepYInv     y-inverse of the chunk                                                    (stage 3)
//   kStepMid      [chunk 0: whole-row kernels: PBE mid stage, split WGC99 combine]  y-forward of the flux chunk  (stage 3)  sends
//   kStepDivX     fused x pass of the divergence chunk                                      (stage 4)  sends
//   kStepDivYInv  y-inverse of the divergence chunk                                         (stage 5)
// Potential-spectrum form (one GPU, split-derivative GGA with Hartree; OFDFT_OPT_POT_SPECTRUM): stage 2 forms i f_a n^ only, stage 4
// reads n^ beside G_a^ and returns i f_a G_a^ - v_H^ / 2 (+ E_H by Parseval), stage 5 adds D_b G_b inside the y-inverse of that
// spectrum -- the combine kernel reads one spectrum for Hartree + divergence where it read three (v_H, D_a part, D_b part).
// One-axis operators as one-axis passes (one GPU; OFDFT_OPT_AXIS_PASSES): i f_a n^ depends on x only, so stage 1 forms D_a n by an x pass
// on the z spectrum BEFORE its y-forward (no y round trip: stage 2 does not produce it, stage 3 does not y-invert it); on cells with
// orthogonal axes -k^2 = -(k_a^2 + k_c^2) - k_b^2, so the von Weizsaecker Laplacian is an x pass on the z spectrum plus one y pass that
// multiplies by -k_b^2 between its two transforms and adds the x pass' result (stage 2; two passes where there were three).
struct ZRun {
    DenSrc ds{};
    double nel = 0.0;
    const real* vext = nullptr;
    real* v_out = nullptr;
    ZCombineArgs za{};
    bool has_h = false, has_g = false, has_vw = false, has_wt = false, has_wgc = false;
    cplx *s_n = nullptr, *s_s = nullptr, *s_vh = nullptr, *s_g[3] = {nullptr, nullptr, nullptr};
    cplx *s_b = nullptr, *s_a = nullptr, *sw[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    real* dfdn = nullptr;
    TermScalars ts{};              // host scalars of the evaluation's terms (zrun_begin; the nonlocal chain's step 1 adds the tables)
    // The evaluation is two independent chains that meet only in the combine kernel:
    //   chain 0: density spectrum -> Hartree, grad n -> PBE -> divergence;  sqrt(n) -> Laplacian (vW)
    //   chain 1: the nonlocal KEDF (Wang-Teter powers or the six WGC99 spectra)
    // xlist[k] = spectra of chain k that cross the next geometry boundary (= one all-to-all on several GPUs)
    std::vector<cplx*> xlist[2];
    bool gsplit = false;           // split-derivative form of the GGA chain (only D_a visits the x pass)
    bool lapl = false;             // Laplacian-dependent Pauli-Gaussian member: lap n in, lap(df/dL) out ride the same chain
    // potential-spectrum form (OFDFT_OPT_POT_SPECTRUM; one GPU, split GGA + Hartree): v_H^ rides in the divergence x pass (which reads
    // n^ again and forms E_H by Parseval), D_b G_b + the y-inverse of that spectrum are one y pass, the combine reads one spectrum
    bool pspec = false;
    bool da_early = false;         // OFDFT_OPT_AXIS_PASSES bit 1: stage 1 formed D_a n from the z spectrum (s_g[0] is final, not an x-pass result)
    bool lap_split = false;        // ... bit 2: the Laplacian of sqrt(n) is x pass + ylap in stage 2 (s_s is never y-forwarded)
    cplx* s_sx = nullptr;          // ... the x pass' result, added by ylap
    cplx* s_l = nullptr;
    real* dzn = nullptr;
    bool wgc_split = false;        // the WGC99 potential was formed by zi_wgc_kernel (za.v_part)
    bool closure = false;          // single-GPU closure evaluation: only chi.grad leaves the call, so v may stay in two parts
    bool late_join = false;        // host-bound sums of a closure evaluation: the share of sum(v n) of the deferred part is added by chi_grad / the host
    bool vpart_deferred = false;   // ... and does: zi_combine does not wait for zi_wgc, chi_grad adds v_part (zcombine)
    // progress of the slab drivers (zstep): last (step, chunk) of each chain; what step 1 sent (read again by every chunk of step 2)
    int step[2] = {0, 0}, step_chunk[2] = {0, 0};
    bool yinv_owed[2] = {false, false};      // ofdft_dist_stage(4) ran step 5: ofdft_dist_finish runs the chain's step 6
    std::vector<cplx*> in_list[2];
    int combine_blocks = 0, pbe_blocks = 0;
    hipStream_t sb = nullptr;      // stream of the nonlocal-KEDF chain (== the main stream unless forked)
    hipStream_t sc = nullptr;      // second side stream: vW chain and the second half of the WGC99 chain
    bool forked = false;
};

}  // namespace
struct ofdft_zrun_holder { ZRun r; };
namespace {

ZRun& zrun(ofdft_ctx* c);

// ---- all-to-all buffers of the slab-decomposed path, one pair per chain (both directions reuse the pair):
// chain 0 carries at most 5 spectra (Hartree, grad n, vW leaving stage 2), chain 1 at most 8 (2 Wang-Teter + 6 WGC99)

enum { kStepYFwd = 1, kStepX, kStepYInv, kStepMid, kStepDivX, kStepDivYInv, kStepDone };

#ifndef OFDFT_YDERIV_FWD
#define OFDFT_YDERIV_FWD 1
#endif
// One begin for every z-fused evaluation (ofdft_dist_begin, ofdft_dist_closure, zfused_enqueue): what the pipeline refuses, the
// complete reset of the run -- a failed earlier call must not leave its state behind -- and the host-side state both chains
// read (term flags, the combine kernel's arguments).
int zrun_begin(ofdft_ctx* c, const DenSrc& ds, double nel, const real* vext, real* v_out) {
    if (!ds.src) return fail(c, OFDFT_EINVAL, "null argument");
    if (!c->mask) return fail(c, OFDFT_ESTATE, "ofdft_set_terms has not been called");
    if (int rc = hc_refuse_staged(c)) return rc;       // (the single-GPU entries hand those kinds to hc_evaluate before they get here)
    if ((c->mask & OFDFT_ION_ELECTRON) && !vext) return fail(c, OFDFT_EINVAL, "IonElectron term needs vext");
    if (!(c->fast && c->n2 / 2 <= 512)) return fail(c, OFDFT_EINVAL, "staged path needs the power-of-two fast path");
    if (gga_needs_laplacian(c) && !c->gga_split)
        return fail(c, OFDFT_EINVAL, "Laplacian-dependent Pauli-Gaussian members need the split-derivative GGA chain (OFDFT_OPT_GGA_SPLIT = 1)");
    if (wts_active(c) && c->nranks > 1)
        return fail(c, OFDFT_EINVAL, "the stabilised Wang-Teter style functional (OFDFT_P_WTS_KIND) is served by single-GPU contexts");
    ZRun& r = zrun(c);
    r.ds = ds;
    r.nel = nel;
    r.vext = vext;
    r.v_out = v_out;
    for (int chain = 0; chain < 2; ++chain) {
        r.step[chain] = r.step_chunk[chain] = 0;
        r.yinv_owed[chain] = false;
        r.xlist[chain].clear();
        r.in_list[chain].clear();
        c->recv_parity[chain] = 0;
    }
    r.forked = false;
    r.closure = false;
    r.vpart_deferred = false;
    const unsigned mask = c->mask;
    r.has_h = mask & OFDFT_HARTREE;
    r.has_g = mask & kGgaAny;
    r.has_vw = mask & OFDFT_VW;
    r.has_wt = mask & (OFDFT_WT_NL | OFDFT_NLK);       // (OFDFT_NLK rides the Wang-Teter stages: nl_pow, engine_ctx.h)
    r.has_wgc = mask & OFDFT_WGC99_NL;
    r.za = ZCombineArgs{};
    r.za.ds = r.ds;
    r.za.vext = r.vext;
    r.za.v_out = r.v_out;
    r.za.mask = combine_mask(c);
    r.za.inv_n = 1.0 / (double)c->npts_g;
    r.ts = term_scalars(c, r.nel);
    r.za.tc = r.ts.tc;
    r.s_g[0] = r.s_g[1] = r.s_g[2] = nullptr;
    r.s_n = r.s_s = r.s_vh = r.s_b = r.s_a = nullptr;
    r.pspec = false;
    r.da_early = r.lap_split = false;
    r.s_sx = nullptr;
    return 0;
}

// Step 1: [chunk 0: z-forward (with the pointwise pre-ops) of the chain's input spectra]  y-forward of the chunk -- in place on one
// GPU, into the send buffer on slabs.
int zstep_yfwd(ofdft_ctx* c, hipStream_t st, int chain, int chunk) {
    ZRun& r = zrun(c);
    int rc;
    hipStream_t sb = r.forked ? r.sb : st, sc = r.forked ? r.sc : st;
    const bool dx = c->nranks > 1;
    std::vector<cplx*>& xl = r.xlist[chain];
    if (chunk == 0) {
    xl.clear();
    if (chain == 0) {
        if (r.has_h || r.has_g)
            if ((rc = spec_ws(c, "zn", &r.s_n))) return rc;
        if (r.has_vw)
            if ((rc = spec_ws(c, "zs", &r.s_s))) return rc;
        if (r.s_n || r.s_s) {
            r.gsplit = r.has_g && c->gga_split;
            r.lapl = r.gsplit && gga_needs_laplacian(c);
            r.s_l = nullptr;
            // (n^ stays in s_n, y-forwarded, until the divergence x pass of stage 4: stage 2 writes its results elsewhere)
            r.pspec = r.gsplit && r.has_h && !dx && c->pot_spectrum && xfused_energy_serves(c, r.lapl ? 3 : 2);
            if (r.gsplit) {
                if ((rc = real_ws(c, "dzn", &r.dzn))) return rc;
                if ((rc = spec_ws(c, "zgx", &r.s_g[0]))) return rc;
                if ((rc = spec_ws(c, "zgy", &r.s_g[1]))) return rc;
                if (r.lapl && (rc = spec_ws(c, "zgl", &r.s_l))) return rc;
            }
            r.da_early = r.gsplit && !dx && (c->axis_passes & 1);
            // fp64 build only: in the fp32 build the two-pass Laplacian measured 1.0 % SLOWER per evaluation than the three-pass one in
            // every alternation (256^3, profiles/r07_ab_axis_passes.jsonl) -- bit 2 is accepted there and changes nothing
            r.lap_split = sizeof(real) == 8 && r.s_s && !dx && (c->axis_passes & 2) && cell_axes_orthogonal(c);
            if (r.lap_split && (rc = spec_ws(c, "zsx", &r.s_sx))) return rc;
            if ((rc = launch_zf_density(c, r.ds, r.s_n, r.s_s, st, r.gsplit ? r.dzn : nullptr))) return rc;
            // D_a n from the same spectrum: the multiply by i f_a commutes with the y transforms, so the x pass runs before the y-forward
            // and its result needs no y-inverse (same stream, before yderiv overwrites s_n: no event)
            if (r.da_early) {
                XfIo io{};
                io.in[0] = r.s_n;
                io.out[0] = r.s_g[0];
                if ((rc = xfused<1, 1>(c, io, MixDerivAS{c->n0g, (real)c->n1}, st, "xfused_n"))) return rc;
            }
            // D_b n from the (kz; y, x) spectrum before its in-place y-forward; scaled so that the consumer's 1/N fits
            // (one GPU: the y-forward of n^ rides in the same pass -- both read the same array; OFDFT_YDERIV_FWD=0: two passes)
            const bool yfwd = OFDFT_YDERIV_FWD && r.gsplit && !dx;
            if (r.gsplit && (rc = yderiv(c, r.s_n, r.s_g[1], (double)c->n0g, st, yfwd ? r.s_n : nullptr))) return rc;
            if (r.forked && r.s_s) {          // the vW chain continues on the second side stream
                HIP_TRY(c, hipEventRecord(c->ev_a, st));
                HIP_TRY(c, hipStreamWaitEvent(sc, c->ev_a, 0));
            }
            if (!dx && r.s_n && !yfwd && (rc = fast_axis_pass<false>(c, 1, r.s_n, st))) return rc;
            if (!dx && r.s_s && !r.lap_split && (rc = fast_axis_pass<false>(c, 1, r.s_s, sc))) return rc;
            if (r.s_n) xl.push_back(r.s_n);
            if (r.s_s) xl.push_back(r.s_s);
        }
    } else {
        if ((rc = ensure_term_tables(c, r.ts, sb))) return rc;
        r.za.tc.nref = r.ts.tc.nref;
        if (r.has_wt) {
            const NlPow& nlp = r.ts.nlp;
            if ((rc = spec_ws(c, "zwb", &r.s_b))) return rc;
            if (nlp.two && (rc = spec_ws(c, "zwa", &r.s_a))) return rc;
            PowersArgs pa{};
            pa.out[0] = r.s_b;
            pa.out[3] = r.s_a;
            pa.e0 = nlp.e_b;
            pa.e1 = nlp.e_a;
            if ((rc = launch_zf_powers(c, r.ds, pa, sb))) return rc;
            for (cplx* sp : {r.s_b, r.s_a}) {
                if (!sp) continue;
                if (!dx && (rc = fast_axis_pass<false>(c, 1, sp, sb))) return rc;
                xl.push_back(sp);
            }
        }
        if (r.has_wgc) {
            const double al = c->params[OFDFT_P_WGC_ALPHA], be = c->params[OFDFT_P_WGC_BETA];
            const char* wn[6] = {"zw0", "zw1", "zw2", "zw3", "zw4", "zw5"};
            PowersArgs pa{};
            for (int i = 0; i < 6; ++i) {
                if ((rc = spec_ws(c, wn[i], &r.sw[i]))) return rc;
                pa.out[i] = r.sw[i];
            }
            pa.e0 = be;
            pa.e1 = al;
            pa.nref = r.ts.tc.nref;
            pa.sum53 = r.ts.tc.wgc_sum_53;
            if ((rc = launch_zf_powers(c, r.ds, pa, sb))) return rc;
            if (r.forked) {                    // second half (P, Q, S) continues on the second side stream
                HIP_TRY(c, hipEventRecord(c->ev_b, sb));
                HIP_TRY(c, hipStreamWaitEvent(sc, c->ev_b, 0));
            }
            if (!dx && c->ybatch) {       // a half's three y passes as ONE launch (grid.y = 3): more workgroups than the
                                          // chip holds at once, so loads, transforms and stores of different tiles overlap
                if ((rc = fast_axis_pass_multi<false>(c, 1, r.sw, 3, sb))) return rc;
                if ((rc = fast_axis_pass_multi<false>(c, 1, r.sw + 3, 3, sc))) return rc;
            }
            for (int i = 0; i < 6; ++i) {
                if (!dx && !c->ybatch && (rc = fast_axis_pass<false>(c, 1, r.sw[i], i < 3 ? sb : sc))) return rc;
                xl.push_back(r.sw[i]);
            }
        }
    }
    }   // chunk == 0
    if (dx && !xl.empty()) {        // the chain's y-forwards in one launch (per chunk), written in the exchange layout
        cplx *send, *recv;
        if ((rc = dist_buffers(c, chain, &send, &recv))) return rc;
        if ((rc = ypass_xchg<false>(c, xl, send, st, chunk))) return rc;
    }
    return 0;
}

// Step 2: the fused x passes (forward x, k-space mixing, inverse x) of the chunk.
int zstep_x(ofdft_ctx* c, hipStream_t st, int chain, int chunk) {
    ZRun& r = zrun(c);
    int rc;
    hipStream_t sb = r.forked ? r.sb : st, sc = r.forked ? r.sc : st;
    // several ranks: the inputs sit in the chain's receive buffer (slot = position in step 1's list) and the
    // outputs are written to its send buffer in the order they are listed here -- per kz chunk of the exchange layout
    const bool dx = c->nranks > 1;
    std::vector<cplx*>& xl = r.xlist[chain];
    if (chunk == 0) r.in_list[chain] = xl;        // what step 1 sent: every chunk's pass reads the same slots
    const std::vector<cplx*>& in_list = r.in_list[chain];
    xl.clear();
    cplx *send = nullptr, *recv = nullptr;
    XfLayout lay{};
    const XcView xv = xc_view(c, chunk);
    int nout = 0;
    if (dx) {
        if ((rc = dist_buffers(c, chain, &send, &recv))) return rc;
        nout = chain == 0 ? (r.has_h ? 1 : 0) + (r.has_g ? (r.gsplit ? (r.lapl ? 2 : 1) : 3) : 0) + (r.s_s ? 1 : 0)
                          : (r.s_b ? 1 : 0) + (r.s_a ? 1 : 0) + (r.has_wgc ? 6 : 0);
        lay = XfLayout{(long long)in_list.size() * xv.arr_sz, nout * xv.arr_sz, xv.arr_sz, xv.nb, xv.nrem, xv.kb0 * 8};
        recv += (long long)in_list.size() * xv.base1;         // this chunk's region of either buffer
        send += (long long)nout * xv.base1;
    }
    auto in_of = [&](cplx* arr) -> cplx* {
        if (!dx) return arr;
        for (size_t i = 0; i < in_list.size(); ++i)
            if (in_list[i] == arr) return recv + (long long)i * xv.arr_sz;
        return nullptr;
    };
    auto out_of = [&](cplx* arr) -> cplx* {       // also records the array as crossing the next boundary
        xl.push_back(arr);
        return dx ? send + (long long)(xl.size() - 1) * xv.arr_sz : arr;
    };
    if (chain == 0) {
        if (r.s_n) {
            XfIo io{};
            io.in[0] = in_of(r.s_n);
            int no = 0;
            const bool vh = r.has_h && !r.pspec;      // (potential-spectrum form: v_H^ comes out of the divergence pass instead)
            if (vh) {
                if ((rc = spec_ws(c, "zvh", &r.s_vh))) return rc;
                io.out[no++] = out_of(r.s_vh);
            }
            if (r.has_g && r.gsplit) {
                if (!r.da_early) io.out[no++] = out_of(r.s_g[0]);     // (D_a n)^ only
                if (r.lapl) io.out[no++] = out_of(r.s_l); // -k^2 n^
            } else if (r.has_g) {
                const char* gn[3] = {"zgx", "zgy", "zgz"};
                for (int k = 0; k < 3; ++k) {
                    if ((rc = spec_ws(c, gn[k], &r.s_g[k]))) return rc;
                    io.out[no++] = out_of(r.s_g[k]);
                }
            }
            if (r.da_early) {         // what is left beside D_a n: [v_H^] [, -k^2 n^] -- nothing in the potential-spectrum form without the latter
                if (r.lapl && vh) rc = xfused<1, 2>(c, io, MixDensityA<true, true, false>{c->kg}, st, "xfused_n", lay);
                else if (r.lapl) rc = xfused<1, 1>(c, io, MixScale<SPEC_LAPLACE>{c->kg, 0.0, 0.0}, st, "xfused_n", lay);
                else if (vh) rc = xfused<1, 1>(c, io, MixDensity<true, false>{c->kg}, st, "xfused_n", lay);
                else rc = 0;
            }
            else if (r.lapl && vh) rc = xfused<1, 3>(c, io, MixDensityA<true, true>{c->kg}, st, "xfused_n", lay);
            else if (r.lapl) rc = xfused<1, 2>(c, io, MixDensityA<false, true>{c->kg}, st, "xfused_n", lay);
            else if (r.gsplit && vh) rc = xfused<1, 2>(c, io, MixDensityA<true>{c->kg}, st, "xfused_n", lay);
            else if (r.gsplit) rc = xfused<1, 1>(c, io, MixDensityA<false>{c->kg}, st, "xfused_n", lay);
            else if (r.has_h && r.has_g) rc = xfused<1, 4>(c, io, MixDensity<true, true>{c->kg}, st, "xfused_n", lay);
            else if (r.has_h) rc = xfused<1, 1>(c, io, MixDensity<true, false>{c->kg}, st, "xfused_n", lay);
            else rc = xfused<1, 3>(c, io, MixDensity<false, true>{c->kg}, st, "xfused_n", lay);
            if (rc) return rc;
        }
        if (r.s_s && r.lap_split) {
            // -(k_a^2 + k_c^2) s^ by an x pass on the z spectrum, then inv_y(-k_b^2 fwd_y(s^)) + that in one y pass: s_s is final
            // (each pass carries the other axis' transform length, as the unnormalised round trips of the three-pass route do)
            XfIo io{};
            io.in[0] = r.s_s;
            io.out[0] = r.s_sx;
            const real* bb = c->kg.b;
            const double kb2 = (double)bb[3] * bb[3] + (double)bb[4] * bb[4] + (double)bb[5] * bb[5];
            if ((rc = xfused<1, 1>(c, io, MixScale<SPEC_LAPLACE_AC>{c->kg, (real)c->n1, 0.0}, sc, "xfused_lap"))) return rc;
            if ((rc = ylap(c, r.s_s, r.s_sx, r.s_s, -kb2 * (double)c->n0g, sc))) return rc;
            c->fft_count++;
        } else if (r.s_s) {
            XfIo io{};
            io.in[0] = in_of(r.s_s);
            io.out[0] = out_of(r.s_s);
            if ((rc = xfused<1, 1>(c, io, MixScale<SPEC_LAPLACE>{c->kg, 0.0, 0.0}, sc, "xfused_lap", lay))) return rc;
        }
    } else {
        if (r.has_wt && (c->mask & OFDFT_NLK)) {
            // the same stage with the kernel from "t:nlk": XWM mixes its two spectra in one 2 -> 2 pass, the others scale each
            // spectrum by the one column
            if (r.ts.nlp.sym) {
                XfIo io{};
                io.in[0] = in_of(r.s_b);
                io.in[1] = in_of(r.s_a);
                io.out[0] = out_of(r.s_b);
                io.out[1] = out_of(r.s_a);
                if ((rc = xfused<2, 2>(c, io, MixNlk<2>{nlk_col(c, 0), nlk_col(c, 1)}, sb, "xfused_nlk", lay))) return rc;
            } else {
                for (cplx* sp : {r.s_b, r.s_a}) {
                    if (!sp) continue;
                    XfIo io{};
                    io.in[0] = in_of(sp);
                    io.out[0] = out_of(sp);
                    if ((rc = xfused<1, 1>(c, io, MixNlk<1>{nlk_col(c, 0), nullptr}, sb, "xfused_nlk", lay))) return rc;
                }
            }
        } else if (r.has_wt) {
            const MixScale<SPEC_LINDHARD> lind{c->kg, (real)r.ts.wt_pref, (real)r.ts.wt_inv2kf};
            for (cplx* sp : {r.s_b, r.s_a}) {
                if (!sp) continue;
                XfIo io{};
                io.in[0] = in_of(sp);
                io.out[0] = out_of(sp);
                if ((rc = xfused<1, 1>(c, io, lind, sb, "xfused_lind", lay))) return rc;
            }
        }
        if (r.has_wgc) {
            const MixWgc mix = wgc_tab(c, dx ? xv.base1 : 0);    // (the table is chunk-major like the buffers)
            for (int half = 0; half < 2; ++half) {
                XfIo io{};
                for (int i = 0; i < 3; ++i) {
                    io.in[i] = in_of(r.sw[3 * half + i]);
                    io.out[i] = out_of(r.sw[3 * half + i]);
                }
                if ((rc = xfused_wgc(c, io, mix, half == 0 ? sb : sc, "xfused_wgc", lay))) return rc;
            }
        }
    }
    return 0;
}

// Steps 3 and 6, slabs only: y-inverse of the chunk of what the preceding x passes sent back (the results of step 2; the
// divergence spectrum of step 5, chain 0), read from the exchange layout in one launch.  One GPU: nothing -- the mid stage and
// the combine y-invert in place.
int zstep_yinv(ofdft_ctx* c, hipStream_t st, int chain, int chunk) {
    const std::vector<cplx*>& xl = zrun(c).xlist[chain];
    if (c->nranks == 1 || xl.empty()) return 0;
    cplx *send, *recv;
    if (int rc = dist_buffers(c, chain, &send, &recv)) return rc;
    return ypass_xchg<true>(c, xl, recv, st, chunk);
}

// Step 4: [chunk 0: the whole-row kernels -- one GPU: y-inverse of what came back from the x passes (each completes one c2r except
// grad n); chain 0: the PBE mid stage on chip; chain 1: the split WGC99 combine]  y-forward of the chunk of the flux.
int zstep_mid(ofdft_ctx* c, hipStream_t st, int chain, int chunk) {
    ZRun& r = zrun(c);
    int rc;
    hipStream_t sb = r.forked ? r.sb : st, sc = r.forked ? r.sc : st;
    const bool dx = c->nranks > 1;
    std::vector<cplx*>& xl = r.xlist[chain];
    auto send_flux = [&]() -> int {              // slabs: the chunk's y-forwards in one launch, written in the exchange layout
        if (!dx || xl.empty()) return 0;
        cplx *send, *recv;
        if (int e = dist_buffers(c, chain, &send, &recv)) return e;
        return ypass_xchg<false>(c, xl, send, st, chunk);
    };
    if (chunk > 0) return send_flux();           // (the row kernels ran with chunk 0, which left the flux in the list)
    const bool wbatch = !dx && c->ybatch && chain == 1 && r.has_wgc && xl.size() >= 6;
    if (wbatch) {           // the six WGC99 results: one batched y-inverse per half (see stage 1)
        if ((rc = fast_axis_pass_multi<true>(c, 1, r.sw, 3, sb))) return rc;
        if ((rc = fast_axis_pass_multi<true>(c, 1, r.sw + 3, 3, sc))) return rc;
    }
    for (cplx* sp : xl) {
        const bool on_b = sp == r.s_b || sp == r.s_a || sp == r.sw[0] || sp == r.sw[1] || sp == r.sw[2];
        const bool on_c = sp == r.s_s || sp == r.sw[3] || sp == r.sw[4] || sp == r.sw[5];
        const bool is_g = sp == r.s_g[0] || sp == r.s_g[1] || sp == r.s_g[2] || (r.s_l && sp == r.s_l);
        const bool is_w = sp == r.sw[0] || sp == r.sw[1] || sp == r.sw[2] || sp == r.sw[3] || sp == r.sw[4] || sp == r.sw[5];
        // (the six WGC99 results were y-inverted by the batched launches above)
        if (!(is_w && wbatch) && !dx && (rc = fast_axis_pass<true>(c, 1, sp, on_b ? sb : (on_c ? sc : st)))) return rc;
        if (!is_g) c->fft_count++;
    }
    xl.clear();
    if (chain == 1) {
        if (r.has_wt) {
            r.za.conv_b = r.s_b;
            r.za.conv_a = r.s_a;
        }
        if (r.has_wgc)
            for (int i = 0; i < 3; ++i) {
                r.za.u[i] = r.sw[i];
                r.za.gw[i] = r.sw[3 + i];
            }
        r.wgc_split = false;
        if (r.has_wgc && c->split_combine && !graph_eligible(c)) {
            // both halves of the chain are done -> its part of the combine runs here, beside the other chain's PBE tail
            real* vp;
            acc_t* part2;
            int blocks = 0;
            if ((rc = real_ws(c, "vpart", &vp))) return rc;
            if ((rc = get_ws(c, "zwgc:part", sizeof(double) * 2 * (size_t)(c->partial_rows + kRedMidRows), (void**)&part2))) return rc;
            if (r.forked) {
                // (its own event: one event recorded on two different streams inside a stream capture crashes the runtime)
                HIP_TRY(c, hipEventRecord(c->ev_c, sc));
                HIP_TRY(c, hipStreamWaitEvent(sb, c->ev_c, 0));
            }
            if ((rc = launch_zi_wgc(c, r.za, vp, part2, &blocks, sb))) return rc;
            OFDFT_REDUCE(c, sb, (const acc_t*)part2, blocks, 2, c->d_scal + kScalWgcSplit, c->h_partial + kMirrorWgcSplit);      // energy sum, this part's sum(v n); host mirror
            r.za.v_part = vp;
            r.wgc_split = true;
            // closure evaluations leave v in two parts: the combine kernel then has nothing to wait for on this stream
            r.vpart_deferred = r.closure && r.forked && c->defer_vpart;
            r.za.v_part_deferred = r.vpart_deferred ? 1 : 0;
        }
        return 0;
    }
    if (r.has_h && !r.pspec) r.za.vh = r.s_vh;
    if (r.s_s) r.za.lap = r.s_s;
    if (r.has_g && r.gsplit) {
        // split-derivative form: A = (D_a n) came back from the x pass and was y-inverted above (or was formed in stage 1), B = (D_b n) is local
        if ((rc = real_ws(c, "dfdn", &r.dfdn))) return rc;
        if ((rc = launch_zpbe2(c, r.ds, r.s_g[0], r.s_g[1], r.dzn, r.dfdn, r.za.inv_n, &r.pbe_blocks, st, r.lapl ? r.s_l : nullptr)))
            return rc;
        OFDFT_REDUCE(c, st, c->d_partial, r.pbe_blocks, kPbeScalars, c->d_reduced + kSumGga, c->h_partial + kSumGga);
        // D_b G_b in one y pass, in place (scaled like B); only G_a goes on to the x pass
        // (potential-spectrum form: G_b waits for stage 5, where its D_b joins the y-inverse of the divergence spectrum)
        if (!r.pspec && (rc = yderiv(c, r.s_g[1], r.s_g[1], (double)c->n0g, st))) return rc;
        if (!dx && (rc = fast_axis_pass<false>(c, 1, r.s_g[0], st))) return rc;
        xl.push_back(r.s_g[0]);
        if (r.lapl) {             // (df/dL)^ goes on to the x pass beside G_a
            if (!dx && (rc = fast_axis_pass<false>(c, 1, r.s_l, st))) return rc;
            xl.push_back(r.s_l);
        }
    } else if (r.has_g) {
        if ((rc = real_ws(c, "dfdn", &r.dfdn))) return rc;
        if ((rc = launch_zpbe(c, r.ds, r.s_g[0], r.s_g[1], r.s_g[2], r.dfdn, r.za.inv_n, &r.pbe_blocks, st))) return rc;
        // no host round trip in the middle of the evaluation: reduce on the device, read with the final sums
        OFDFT_REDUCE(c, st, c->d_partial, r.pbe_blocks, kPbeScalars, c->d_reduced + kSumGga, c->h_partial + kSumGga);
        for (int k = 0; k < 3; ++k) {
            if (!dx && (rc = fast_axis_pass<false>(c, 1, r.s_g[k], st))) return rc;
            xl.push_back(r.s_g[k]);
        }
    }
    return send_flux();
}

// Step 5: fused x pass of the chunk of the divergence (chain 0 only).
int zstep_divx(ofdft_ctx* c, hipStream_t st, int chain, int chunk) {
    ZRun& r = zrun(c);
    r.xlist[chain].clear();
    const XcView xv = xc_view(c, chunk);
    if (chain == 0 && r.pspec) {
        // i f_a G_a^ [+ (k^2 / 2) (df/dL)^] - v_H^ / 2 in place of G_a^, and the partial sums of E_H (one per workgroup)
        acc_t* ehp;
        const size_t rows = (size_t)(c->gx.total / c->gx.n0) + 1;        // >= workgroups of the pass (at least one line each)
        if (int rc = get_ws(c, "zh:part", sizeof(acc_t) * rows, (void**)&ehp)) return rc;
        XfIo dio{};
        dio.in[0] = dio.out[0] = r.s_g[0];
        const double ehpref = 2.0 * kPi / (double)c->npts_g;
        if (r.lapl) {
            dio.in[1] = r.s_l;
            dio.in[2] = r.s_n;
            if (int rc = xfused_energy<3>(c, dio, MixDerivAH<true>{c->kg, ehp, ehpref, c->n2 / 2}, st, "xfused_div")) return rc;
        } else {
            dio.in[1] = r.s_n;
            if (int rc = xfused_energy<2>(c, dio, MixDerivAH<false>{c->kg, ehp, ehpref, c->n2 / 2}, st, "xfused_div")) return rc;
        }
        r.za.eh_part = ehp;
        r.za.eh_rows = c->xpass_blocks;
        c->fft_count++;           // (the inverse transform of v_H^ rides in this spectrum: counted as before)
        r.xlist[0].push_back(r.s_g[0]);
    } else if (chain == 0 && r.has_g && r.gsplit) {
        XfIo dio{};
        XfLayout lay{};
        dio.in[0] = dio.out[0] = r.s_g[0];
        const int nin = r.lapl ? 2 : 1;
        if (c->nranks > 1) {     // receive buffer slot 0 -> send buffer slot 0 (of this kz chunk)
            cplx *send, *recv;
            if (int rc = dist_buffers(c, 0, &send, &recv)) return rc;
            dio.in[0] = recv + (long long)nin * xv.base1;
            dio.out[0] = send + xv.base1;
            lay = XfLayout{xv.arr_sz, xv.arr_sz, xv.arr_sz, xv.nb, xv.nrem, xv.kb0 * 8};
        }
        if (r.lapl) {            // i f_a G_a^ + (k^2 / 2) (df/dL)^ -> the spectrum the combine subtracts twice
            dio.in[1] = r.s_l;
            if (c->nranks > 1) {
                dio.in[1] = dio.in[0] + xv.arr_sz;
                lay.se_in = 2 * xv.arr_sz;
            }
            if (int rc = xfused<2, 1>(c, dio, MixDerivAL{c->kg}, st, "xfused_div", lay)) return rc;
        } else if (int rc = xfused<1, 1>(c, dio, MixDerivA{c->kg}, st, "xfused_div", lay)) {
            return rc;
        }
        r.xlist[0].push_back(r.s_g[0]);
    } else if (chain == 0 && r.has_g) {
        XfIo dio{};
        XfLayout lay{};
        for (int k = 0; k < 3; ++k) dio.in[k] = r.s_g[k];
        dio.out[0] = r.s_n;      // n^ is no longer needed
        if (c->nranks > 1) {     // receive buffer slots 0..2 -> send buffer slot 0 (of this kz chunk)
            cplx *send, *recv;
            if (int rc = dist_buffers(c, 0, &send, &recv)) return rc;
            for (int k = 0; k < 3; ++k) dio.in[k] = recv + 3 * xv.base1 + k * xv.arr_sz;
            dio.out[0] = send + xv.base1;
            lay = XfLayout{3 * xv.arr_sz, xv.arr_sz, xv.arr_sz, xv.nb, xv.nrem, xv.kb0 * 8};
        }
        if (int rc = xfused<3, 1>(c, dio, MixDiv{c->kg}, st, "xfused_div", lay)) return rc;
        r.xlist[0].push_back(r.s_n);
    }
    return 0;
}

// the local sums of an evaluation from the pinned host mirror (after the stream that copied them has been drained)
// what the host has to fold when it reads the pinned mirror of an evaluation's sums (the reducing kernels write it directly)
constexpr int kCollectWgcSplit = 1;     // the split WGC99 kernel's energy sum sits in slot kMirrorWgcSplit
constexpr int kCollectVnShare = 2;      // ... and its share of sum(v n) in slot kMirrorWgcSplitVn (closure form: chi_grad added it on the device)
constexpr int kCollectNoGga = 4;        // no GGA term: the three GGA slots are not written
int collect_flags(const ZRun& r, bool late_join) {
    return (r.wgc_split ? kCollectWgcSplit : 0) | (late_join ? kCollectVnShare : 0) | (r.has_g ? 0 : kCollectNoGga);
}
// ... of the unfused / chirp-z pipelines in their host-free form (finish_terms: defer)
int collect_flags_unfused(const ofdft_ctx* c) { return (c->mask & kGgaAny) ? 0 : kCollectNoGga; }
void zfused_collect(const ofdft_ctx* c, int flags, double* sums) {
    for (int i = 0; i < kNSums; ++i) sums[i] = c->h_partial[i];
    if (flags & kCollectNoGga)
        for (int i = kSumGga; i < kNSums; ++i) sums[i] = 0.0;
    if (flags & kCollectWgcSplit) sums[kSumWgc] += c->h_partial[kMirrorWgcSplit];
    if (flags & kCollectVnShare) sums[kSumVn] += c->h_partial[kMirrorWgcSplitVn];
}

// local sums: sums[kNSums] in the layout of eval_layout.h (the combine sums, then the GGA sums)
// `sums` == nullptr: the caller reduces the device-resident sums itself (slab-decomposed path).  `defer`: the sums are
// copied to the pinned host mirror but nothing waits here (zfused_collect reads them after the caller's stream sync --
// the graph-capturable form)
// (after step 6 of both chains: on slabs the divergence has been y-inverted chunk by chunk, one GPU does it here)
int zcombine(ofdft_ctx* c, double* sums, hipStream_t st, bool defer = false) {
    ZRun& r = zrun(c);
    int rc;
    if (r.has_g) {
        cplx* dsp = r.gsplit ? r.s_g[0] : r.s_n;       // the spectrum that carries the (x part of the) divergence
        if (c->nranks == 1) {     // (pspec: D_b G_b + the y-inverse of the divergence spectrum (+ v_H) in one pass, into that spectrum)
            rc = r.pspec ? yderiv_add(c, r.s_g[1], dsp, dsp, (double)c->n0g, st) : fast_axis_pass<true>(c, 1, dsp, st);
            if (rc) return rc;
        }
        c->fft_count++;
        r.za.div = dsp;
        r.za.div2 = (r.gsplit && !r.pspec) ? r.s_g[1] : nullptr;
        r.za.dfdn = r.dfdn;
    }
    r.xlist[0].clear();
    r.xlist[1].clear();
    const bool late_join = r.forked && r.vpart_deferred && r.wgc_split;
    if (r.forked) {       // the combine needs both chains -- unless the nonlocal chain's only product is the deferred v_part
        if (!late_join) {
            HIP_TRY(c, hipEventRecord(c->ev_join, r.sb));
            HIP_TRY(c, hipStreamWaitEvent(st, c->ev_join, 0));
        }
        HIP_TRY(c, hipEventRecord(c->ev_join2, r.sc));
        HIP_TRY(c, hipStreamWaitEvent(st, c->ev_join2, 0));
    }
    const bool wts = wts_active(c);
    r.za.wts_w = nullptr;
    if (wts) {            // energies-only pass -> device-resident weights f - f' X, f' (no host round trip: graph-capturable)
        ZCombineArgs z1 = r.za;
        z1.v_out = nullptr;
        if ((rc = launch_zi_combine(c, z1, &r.combine_blocks, st))) return rc;
        OFDFT_REDUCE(c, st, c->d_partial, r.combine_blocks, kCombineScalars, c->d_reduced);
        OFDFT_LAUNCH(c, st, "reduce", wts_weights_kernel, dim3(1), dim3(64), 0, (const acc_t*)c->d_reduced, c->d_scal + kScalWts);
        r.za.wts_w = c->d_scal + kScalWts;
    }
    if ((rc = launch_zi_combine(c, r.za, &r.combine_blocks, st))) return rc;
    // (host-bound sums: the reduce kernel writes the pinned mirror itself -- no copy command behind it; the stabilised
    // WT-style functional rewrites two of the sums afterwards and keeps the copy)
    OFDFT_REDUCE(c, st, c->d_partial, r.combine_blocks, kCombineScalars, c->d_reduced, (sums && !wts) ? c->h_partial : (acc_t*)nullptr);
    if (wts) OFDFT_LAUNCH(c, st, "reduce", wts_finalize_kernel, dim3(1), dim3(64), 0, c->d_reduced, (const acc_t*)(c->d_scal + kScalWts));
    if (late_join) {      // now the nonlocal chain: its share of sum(v n) joins the combine's (mu is formed from the total)
        HIP_TRY(c, hipEventRecord(c->ev_join, r.sb));
        HIP_TRY(c, hipStreamWaitEvent(st, c->ev_join, 0));
        // host-bound sums: chi_grad and the host each add the share (kScalWgcSplitVn of the device scalars / its pinned mirror) themselves
        if (!sums)
            OFDFT_LAUNCH(c, st, "reduce", (axpy_kernel<acc_t>), dim3(1), dim3(64), 0, (const acc_t*)(c->d_scal + kScalWgcSplitVn), c->d_reduced + kSumVn,
                         (long long)1, 1);
    }
    r.late_join = late_join && sums != nullptr;
    if (!r.has_g) HIP_TRY(c, hipMemsetAsync(c->d_reduced + kSumGga, 0, kPbeScalars * sizeof(double), st));
    r.step[0] = r.step[1] = kStepDone;         // (a step or a second combine without a new begin is out of order)
    if (!sums) {                  // the caller reduces the device-resident sums (c->d_reduced) itself
        if (r.wgc_split)          // fold in the energy sum of the split WGC99 kernel
            OFDFT_LAUNCH(c, st, "reduce", (axpy_kernel<acc_t>), dim3(1), dim3(64), 0, (const acc_t*)(c->d_scal + kScalWgcSplit), c->d_reduced + kSumWgc,
                         (long long)1, 1);
        return 0;
    }
    if (wts) HIP_TRY(c, hipMemcpyAsync(c->h_partial, c->d_reduced, sizeof(double) * kCombineScalars, hipMemcpyDeviceToHost, st));
    if (defer) return 0;
    HIP_TRY(c, hipStreamSynchronize(st));
    zfused_collect(c, collect_flags(r, r.late_join), sums);
    return 0;
}

// The kernels of one step of a chain on one kz chunk: the one statement of what a step is, for every driver.
int zstep_kernels(ofdft_ctx* c, hipStream_t st, int step, int chain, int chunk) {
    switch (step) {
        case kStepYFwd: return zstep_yfwd(c, st, chain, chunk);
        case kStepX: return zstep_x(c, st, chain, chunk);
        case kStepYInv: return zstep_yinv(c, st, chain, chunk);
        case kStepMid: return zstep_mid(c, st, chain, chunk);
        case kStepDivX: return zstep_divx(c, st, chain, chunk);
        case kStepDivYInv: return zstep_yinv(c, st, chain, chunk);          // (the divergence spectrum: chain 0's list after step 5)
    }
    return fail(c, OFDFT_EINVAL, "no step %d", step);
}

// what a step left to be exchanged: the chunk's region of the chain's send buffer, `offset` elements into it (the same region of
// the receive buffer of parity `land` takes the delivery), `bytes` per peer -- 0: nothing crosses
struct SlabMsg {
    cplx* send = nullptr;
    long long offset = 0;
    size_t bytes = 0;
    int land = 0;
};

// One step of a slab driver (ofdft_dist_step / _stage / _closure).  Order per chain: the next chunk of the same step, or chunk 0
// of the next step after the last chunk of the previous one; chain 1 only after chain 0's step 1.  Runs the kernels, records the
// progress, fills *msg, and after the last chunk of a step that sent turns the chain to the receive buffer the delivery lands in.
int zstep(ofdft_ctx* c, hipStream_t st, int step, int chain, int chunk, SlabMsg* msg) {
    ZRun& r = zrun(c);
    const int K = c->xc.n;
    const bool next_chunk = step == r.step[chain] && chunk == r.step_chunk[chain] + 1 && chunk < K;
    const bool next_step = step == r.step[chain] + 1 && chunk == 0 && (r.step[chain] == 0 || r.step_chunk[chain] == K - 1);
    if (step < kStepYFwd || step > kStepDivYInv || !(next_chunk || next_step) || (chain == 1 && r.step[0] < kStepYFwd))
        return fail(c, OFDFT_ESTATE, "step %d chunk %d of chain %d out of order (last: step %d chunk %d of %d)", step, chunk, chain,
                    r.step[chain], r.step_chunk[chain], K);
    if (int rc = zstep_kernels(c, st, step, chain, chunk)) return rc;
    r.step[chain] = step;
    r.step_chunk[chain] = chunk;
    *msg = SlabMsg{};
    const bool sends = step == kStepYFwd || step == kStepX || step == kStepMid || step == kStepDivX;
    if (sends && c->nranks > 1 && !r.xlist[chain].empty()) {
        cplx *send, *recv;
        if (int rc = dist_buffers(c, chain, &send, &recv)) return rc;
        const XcView v = xc_view(c, chunk);
        const long long narr = (long long)r.xlist[chain].size();
        msg->offset = narr * v.base1;
        msg->send = send + msg->offset;
        msg->bytes = sizeof(cplx) * (size_t)c->xg.nxl * (size_t)v.arr_sz * (size_t)narr;
        msg->land = c->recv_parity[chain] ^ 1;
        if (chunk == K - 1) c->recv_parity[chain] ^= 1;          // the next step reads what this exchange delivers
    }
    return 0;
}

// one evaluation on one GPU enqueued on `st` (and the side streams forked from / joined to it): the six steps with chunk 0,
// then the combine; with `defer` nothing touches the host: the sequence can be captured into a hipGraph
int zfused_enqueue(ofdft_ctx* c, const DenSrc& ds, double nel, const real* vext, real* v_out, double* sums, hipStream_t st,
                   bool defer) {
    int rc;
    if ((rc = zrun_begin(c, ds, nel, vext, v_out))) return rc;
    ZRun& r = zrun(c);
    r.closure = defer;            // (only the closure enqueues in deferred form; its consumer is chi_grad)
    // Forking the nonlocal-KEDF chain (and the vW / second WGC99 half) onto their own streams lets their
    // latency-bound fused kernels overlap the other chain's bandwidth-bound passes.
    r.forked = c->use_side_stream && c->side_stream && c->side_stream2 && (c->mask & (OFDFT_WT_NL | OFDFT_WGC99_NL | OFDFT_NLK)) &&
               (c->mask & (OFDFT_HARTREE | OFDFT_VW | kGgaAny));
    if (r.forked) {
        r.sb = c->side_stream;
        r.sc = c->side_stream2;
        HIP_TRY(c, hipEventRecord(c->ev_fork, st));
        HIP_TRY(c, hipStreamWaitEvent(r.sb, c->ev_fork, 0));
        HIP_TRY(c, hipStreamWaitEvent(r.sc, c->ev_fork, 0));
    }
    // one GPU, forked: the nonlocal chain's first kernels go to the device BEFORE the other chain's four launches (its stream
    // sat idle for ~30 us of host enqueue time at the head of every evaluation; profiles/r04_timeline_*.md)
    // (the y-inverse steps are no-ops here, and nothing is exchanged: no zstep, whose chain order is the slab drivers')
    const bool nl_first = r.forked && c->nranks == 1;
    for (int step = kStepYFwd; step <= kStepDivYInv; ++step)
        for (int i = 0; i < 2; ++i)
            if ((rc = zstep_kernels(c, st, step, (nl_first && step == kStepYFwd) ? 1 - i : i, 0))) return rc;
    return zcombine(c, sums, st, defer);
}

int run_terms_zfused(ofdft_ctx* c, const DenSrc& ds, double nel, const real* vext, double* E_terms, real* v_out,
                     double* vn_int, hipStream_t st) {
    double sums[kNSums];
    if (int rc = zfused_enqueue(c, ds, nel, vext, v_out, sums, st, false)) return rc;
    *vn_int = report_energies(c, sums, E_terms);
    return 0;
}

ZRun& zrun(ofdft_ctx* c) {
    if (!c->zr) c->zr = new ofdft_zrun_holder();
    return c->zr->r;
}

// timed = false: no event pair around the call (OFDFT_Q_KERNEL_MS then reads 0): two stream markers are a visible share of
// a 30-microsecond evaluation
int begin_call(ofdft_ctx* c, hipStream_t st, bool timed = true) {
    if (!c) return OFDFT_EINVAL;      // (the ABI function that called this holds the DeviceScope)
    if (!c->cell_set) return fail(c, OFDFT_ESTATE, "ofdft_set_cell has not been called");
    c->hvp_valid = false;      // an evaluation may reuse any workspace: ofdft_hessian_vector starts over (it restores the flag for itself)
    c->fft_count = 0;
    c->launch_count = 0;
    c->xpass_kinds = 0;
    c->ypass_count = 0.0;
    c->yfwd_fused = 0;
    if (timed) HIP_TRY(c, hipEventRecord(c->ev0, st));
    return 0;
}
int end_call(ofdft_ctx* c, hipStream_t st, bool timed = true) {
    if (timed) HIP_TRY(c, hipEventRecord(c->ev1, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (timed) HIP_TRY(c, hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
    else c->last_ms = 0.f;
    c->ms_pending = false;
    HIP_TRY(c, hipGetLastError());
    if (c->profiling) prof_collect(c);
    return 0;
}

}  // namespace

