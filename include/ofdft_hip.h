/*
 * ofdft_hip.h -- C ABI of the MI355X-native orbital-free DFT energy/gradient engine.
 *
 * This is the drop-in boundary of SURVEY.md §8(b).  The reference (profess-ad) has no FFI: its
 * plugin points are Python callables.  Each entry point below names the reference interface it
 * stands behind (paths relative to the reference repo root):
 *
 *   ofdft_energy_potential  <->  one or several `terms` callables f(box_vecs, den) -> E evaluated
 *                                together, plus their functional derivative:
 *                                System.__compute_energy            src/professad/system.py:759-772
 *                                get_functional_derivative          src/professad/functional_tools.py:9-31
 *                                System.functional_derivative       src/professad/system.py:414-447
 *                                the `potentials=` hook             src/professad/system.py:842-854
 *   ofdft_energy_grad_chi   <->  the optimize_density closure chi -> (E, chi.grad)
 *                                                                   src/professad/system.py:830-838
 *   ofdft_set_cell          <->  wavevecs(box_vecs, shape)          src/professad/functional_tools.py:135-162
 *   ofdft_set_terms         <->  the `terms=[...]` list of System   src/professad/system.py:35-36,66
 *   ofdft_rfftn/ofdft_irfftn<->  torch.fft.rfftn / irfftn call sites src/professad/functionals.py:65,71,650,976-981
 *                                                                   src/professad/functional_tools.py:183,227
 *
 * Conventions
 *   - every function returns 0 on success and a negative OFDFT_E* code on failure; nothing throws or
 *     aborts across the ABI; ofdft_last_error() returns a human-readable message.
 *   - all grid pointers are DEVICE pointers to C-contiguous arrays owned by the caller
 *     (real grids [n0][n1][n2]; half spectra [n0][n1][n2/2+1] interleaved re,im); the engine never
 *     retains them past the call.  Plans, twiddles, kernel tables and workspaces live in the ctx.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Work is enqueued on it and
 *     the call returns after the scalar results are on the host (one stream sync).
 *   - a ctx is bound to one device and is not re-entrant.
 *   - precision: the ABI is built once per precision from the same sources -- libofdft_hip.so (OFDFT_F64, the
 *     reference's precision) and libofdft_hip_f32.so (OFDFT_F32, same symbols; grid arrays are float / float2, every
 *     host-visible scalar stays double).  ofdft_create refuses the dtype of the other build.  The fp32 library serves
 *     the evaluation path and ofdft_lbfgs_*; the ion / stress entry points, ofdft_hessian_vector, ofdft_hessian_vector_chi[_multi] and ofdft_precondition[_multi] are fp64-only and return OFDFT_EINVAL there.
 *   - energies are Hartree; lengths bohr; box_vecs rows are the lattice vectors (reference layout).
 */
#ifndef OFDFT_HIP_H
#define OFDFT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ofdft_ctx ofdft_ctx;

/* error codes */
#define OFDFT_OK            0
#define OFDFT_EINVAL       -1   /* bad argument / shape / unsupported option */
#define OFDFT_EHIP         -2   /* a HIP runtime call failed */
#define OFDFT_ESTATE       -3   /* call sequence error (e.g. set_cell not called) */
#define OFDFT_ENOMEM       -4

/* dtype */
#define OFDFT_F64 0
#define OFDFT_F32 1             /* served by libofdft_hip_f32.so: the same sources built with -DOFDFT_REAL_F32 */

/* term bits; index of a term in E_terms[] is its bit position */
#define OFDFT_ION_ELECTRON  (1u << 0)   /* functionals.py:31-46   (needs vext)                    */
#define OFDFT_HARTREE       (1u << 1)   /* functionals.py:49-72                                  */
#define OFDFT_TF            (1u << 2)   /* functionals.py:207-224                                */
#define OFDFT_VW            (1u << 3)   /* functionals.py:227-246                                */
#define OFDFT_WT_NL         (1u << 4)   /* non_local_KEF functionals.py:644-652, params alpha,beta */
#define OFDFT_WGC99_NL      (1u << 5)   /* WGC99 nonlocal part functionals.py:941-983            */
#define OFDFT_LDA_X         (1u << 6)   /* functionals.py:1510-1512                              */
#define OFDFT_PZ_C          (1u << 7)   /* functionals.py:1515-1521                              */
#define OFDFT_PW_C          (1u << 8)   /* functionals.py:1524-1530                              */
#define OFDFT_CHACHIYO_C    (1u << 9)   /* functionals.py:1533-1537                              */
#define OFDFT_PBE_X         (1u << 10)  /* functionals.py:1597-1603                              */
#define OFDFT_PBE_C         (1u << 11)  /* functionals.py:1606-1618                              */
#define OFDFT_GGA_K         (1u << 12)  /* Pauli part of a GGA kinetic functional, int tau_TF F(s): LuoKarasievTrickey
                                           functionals.py:309-333 (F = 1/cosh(1.3 s)) or PauliGaussian :336-403 with
                                           beta = lambda = sigma = 0 (F = exp(-mu s^2)); the vW part is OFDFT_VW */
#define OFDFT_VWGTF         (1u << 13)  /* local Pauli term of vWGTF1 / vWGTF2, int tau_TF G(n/n0), functionals.py:251-306;
                                           n0 = round(N_e)/vol; the vW part is OFDFT_VW */
#define OFDFT_NLK           (1u << 14)  /* Wang-Teter-shaped nonlocal term with a tabulated, density-independent kernel:
                                           sum_{i<=j} int n^(e_i) (K_ij * n^(e_j)), K_ij(|k|) built once per (cell, round(N_e), parameters) into a
                                           per-k-point table; OFDFT_P_NLK_KIND selects KGAP functionals.py:1106-1171, MiGenovaPavanello :1370-1451
                                           or XuWangMa :1456-1498 (the vW and TF parts are OFDFT_VW / OFDFT_TF).  Single-GPU contexts; not together
                                           with OFDFT_WT_NL / OFDFT_WGC99_NL (they share the nonlocal chain's buffers); ofdft_stress serves KGAP and XWM, and
                                           refuses MGP as the reference's get_stress does */
#define OFDFT_NTERMS        15

/* params[] slots for ofdft_set_terms (missing trailing slots keep their defaults) */
#define OFDFT_P_WT_ALPHA    0   /* default 5/6 */
#define OFDFT_P_WT_BETA     1   /* default 5/6 */
#define OFDFT_P_WGC_ALPHA   2   /* default (5+sqrt5)/6 */
#define OFDFT_P_WGC_BETA    3   /* default (5-sqrt5)/6 */
#define OFDFT_P_WGC_GAMMA   4   /* default 2.7 */
#define OFDFT_P_WGC_KAPPA   5   /* default 1.0 */
#define OFDFT_P_GGAK_KIND   6   /* 0 = LKT (default), 1 = Pauli-Gaussian exp(-mu s^2) */
#define OFDFT_P_GGAK_MU     7   /* default 40/27 (PGS); 1.0 = PG1 */
#define OFDFT_P_GGAK_BETA   8   /* Pauli-Gaussian coefficients of q^2, -q s^2, s^4 (functionals.py:336-403); any non-zero one */
#define OFDFT_P_GGAK_LAMBDA 9   /* makes the term depend on the reduced Laplacian q (PGSL0.25 = the reference's default,    */
#define OFDFT_P_GGAK_SIGMA  10  /* PGSLr): one more spectrum each way in the GGA chain; every pipeline, slabs and stress     */
#define OFDFT_P_VWGTF_KIND  11  /* 1 = vWGTF1 (default), 2 = vWGTF2 */
#define OFDFT_P_WTS_KIND    12  /* Pauli-positivity stabilisation of WangTeterStyleFunctional (functionals.py:728-782) for a term
                                   set with OFDFT_TF and OFDFT_WT_NL (or OFDFT_NLK: KGAP's f argument): T = T_TF f(X), X = T_NL / (f'(0) T_TF).  0 (default): f(x) = 1 + x,
                                   i.e. the plain sum T_TF + T_NL; 1: f(x) = exp(x).  Then E_terms[TF] reports T_TF f(X), E_terms[WT_NL]
                                   zero, the potential and the stress carry the weights f - f' X and f'(X) / f'(0).  Single-GPU contexts. */
#define OFDFT_P_NLK_KIND    13  /* kernel of OFDFT_NLK: 1 = KGAP, 2 = Mi-Genova-Pavanello, 3 = Xu-Wang-Ma, 4 = Huang-Carter, 5 = revised
                                   Huang-Carter (0, the default, is refused with the bit set).  Kinds 4 and 5 (functionals.py:1176-1365) have a
                                   density-DEPENDENT kernel w(|r - r'|, xi(r)): they do not ride the Wang-Teter stages but run a chain of their own
                                   after the rest of the term set (csrc/engine_hc.inc.h), need the table of ofdft_set_nlk_table,
                                   0 < beta < 5/3, kappa > 1, lambda, a, b >= 0 and OFDFT_P_WTS_KIND = 0; fp64 library, no stress */
#define OFDFT_P_NLK_P0      14  /* KGAP: E_gap [eV] (0 -> alpha = beta = 1/2 and the Lindhard kernel: Smargiassi-Madden); MGP: a; XWM: kappa; HC: lambda; revHC: a */
#define OFDFT_P_NLK_P1      15  /* MGP: b; HC: beta; revHC: b */
#define OFDFT_P_NLK_P2      16  /* HC: kappa, the ratio of the geometric xi nodes; revHC: beta */
#define OFDFT_P_NLK_P3      17  /* revHC: kappa */
#define OFDFT_NPARAMS       18

/* The scalar block of an evaluation (ofdft_dist_finish / ofdft_dist_scalars / ofdft_dist_energies; csrc/eval_layout.h names every
 * slot): OFDFT_NSCALARS doubles owned by the context, of which the first OFDFT_NSUMS are the local sums of an evaluation (ten of the
 * combine kernel, then the GGA sums: exchange, correlation, kinetic) and slot OFDFT_SCALAR_SUMSQ holds sum chi^2 of the closure form. */
#define OFDFT_NSUMS         13
#define OFDFT_NSCALARS      16
#define OFDFT_SCALAR_SUMSQ  15

/* ofdft_query selectors */
#define OFDFT_Q_FFT_COUNT        0  /* 3-D FFTs executed by the last energy call              */
#define OFDFT_Q_WORKSPACE_BYTES  1  /* device bytes held by the ctx                            */
#define OFDFT_Q_FAST_PATH        2  /* 1 if the LDS radix FFT path is used, 0 = generic DFT    */
#define OFDFT_Q_KERNEL_MS        3  /* HIP-event time of the last energy call's device work    */
#define OFDFT_Q_LAUNCH_COUNT     4  /* kernel launches of the last energy call                 */
#define OFDFT_Q_YPASS_COUNT      5  /* whole-spectrum y line passes of the last energy call    */
#define OFDFT_Q_GRAPH_REPLAYS     6  /* ofdft_energy_grad_chi calls served by a hipGraph replay so far */
#define OFDFT_Q_RESIDENT_EVALS    7  /* ofdft_energy_grad_chi calls served by the persistent small-grid kernel so far */
#define OFDFT_Q_XCHG_CHUNKS      9  /* effective number of kz chunks of the slab exchange (OFDFT_OPT_XCHG_CHUNKS)               */
#define OFDFT_Q_YFWD_FUSED      10  /* y-forward transforms of the last energy call that rode inside a yderiv launch (1C -> 2C in one pass) */
#define OFDFT_Q_RESIDENT_FALLBACKS 8 /* evaluations re-run on the staged path because a grid barrier of the persistent kernel timed out
                                        (the kernel is switched off for the context after the first one) */
#define OFDFT_Q_XPASS_KINDS     11  /* bitmask of the fused x-pass kernel families the last energy call launched (OFDFT_XPASS_*); like
                                        OFDFT_Q_LAUNCH_COUNT it is reset per call and a hipGraph replay reports what its captured call launched */
#define OFDFT_Q_RES_CLOCK       16  /* first of OFDFT_Q_RES_CLOCK_COUNT selectors: phase clock of the last persistent-kernel evaluation in    */
#define OFDFT_Q_RES_CLOCK_COUNT 12  /* microseconds (libraries built with -DOFDFT_RES_CLOCK=1 only; tools/resident_probe.py)                  */
#define OFDFT_XPASS_GROUP    (1u << 0)  /* group-parallel kernel (fft_kernels.h: xfused_kernel)                               */
#define OFDFT_XPASS_WAVE     (1u << 1)  /* wave-local kernel (xwave.h)                                                        */
#define OFDFT_XPASS_CROSS1   (1u << 2)  /* cross-wave kernel (xcross.h), one line per lane                                    */
#define OFDFT_XPASS_CROSS2   (1u << 3)  /* cross-wave kernel, two memory-adjacent lines per lane (fp32 build)                 */
#define OFDFT_XPASS_CHIRPZ   (1u << 4)  /* chirp-z forward-x / mix / inverse-x kernel (bluestein.h: bluestein_xmix_kernel)    */

int  ofdft_create(ofdft_ctx** out, int n0, int n1, int n2, int dtype, int device_id);
void ofdft_destroy(ofdft_ctx* ctx);
const char* ofdft_last_error(const ofdft_ctx* ctx);   /* ctx may be NULL: last create() error */

int  ofdft_set_cell(ofdft_ctx* ctx, const double box_vecs[9]);
int  ofdft_set_terms(ofdft_ctx* ctx, uint32_t term_mask, const double* params, int nparams);
/* The 1-D kernel table w(eta) of the Huang-Carter kinds of OFDFT_NLK (OFDFT_P_NLK_KIND = 4, 5): n >= 4 values on a uniform eta
 * grid that starts at 0 (host arrays; the reference's HuangCarter.kernel, functionals.py:1227-1230).  The call forms the node
 * slopes of functional_tools.interpolate (functional_tools.py:309-310) on the host and uploads both arrays; eta beyond the last
 * node reads the last node (functionals.py:1257).  It replaces an earlier table and clears the validity of the OFDFT_NLK tables.
 * An evaluation of kind 4 / 5 without a table returns OFDFT_ESTATE.  fp64 library only (the fp32 one returns OFDFT_EINVAL). */
int  ofdft_set_nlk_table(ofdft_ctx* ctx, const double* eta_host, const double* w_host, int n);

/* E_terms_host[OFDFT_NTERMS] (entries of unset terms are 0); dEdn_dev may be NULL (energy only).
 * vext_dev is required iff OFDFT_ION_ELECTRON is set. */
int  ofdft_energy_potential(ofdft_ctx* ctx, const void* den_dev, const void* vext_dev,
                            double* E_terms_host, void* dEdn_dev, void* stream);

/* The density-optimisation closure: n = N_e chi^2 / int chi^2; returns per-term energies,
 * the chemical potential mu = int (dE/dn) n / N_e, and grad_dev = dE/dchi * dV, i.e. exactly what
 * the reference leaves in chi.grad (system.py:836-837,853).  grad_dev may be NULL. */
int  ofdft_energy_grad_chi(ofdft_ctx* ctx, const void* chi_dev, const void* vext_dev, double n_electrons,
                           double* E_terms_host, double* mu_host, void* grad_dev, void* stream);

/* Validation / building-block entry points: same semantics as torch.fft.rfftn / irfftn(s=shape). */
int  ofdft_rfftn(ofdft_ctx* ctx, const void* real_dev, void* spec_dev, void* stream);
int  ofdft_irfftn(ofdft_ctx* ctx, const void* spec_dev, void* real_dev, void* stream);
/* Validation of the lean transcendentals the fused kernels use (csrc/fastmath.h): out[i] = f(in[i]) for n elements of
 * the context's precision; kind 0: 1/x, 1: log x, 2: exp x, 3: x^(-1/6), 4: x^(1/3) and 5: 1/x derived from x^(-1/6). */
int  ofdft_debug_math(ofdft_ctx* ctx, int kind, const void* in_dev, void* out_dev, long long n, void* stream);

int  ofdft_query(ofdft_ctx* ctx, int what, double* out);

/* ---- direct peer-store transport of the slab-decomposed hot path ------------------------------------------------------
 * ofdft_dist_closure runs the whole closure evaluation of a slab-decomposed context in ONE call, the library moving the
 * spectra itself: every rank maps every peer's receive buffers and mailbox through hipIpc, copies a stage's spectra device
 * to device into chunk [rank] of each peer's buffer on the chain's stream (one direct xGMI link per peer pair), stamps an
 * epoch behind them and waits (bounded, ~2 s) for the peers' stamps in a one-wave kernel; the two small reductions use
 * the same mailboxes and add the ranks' numbers in rank order.  Set-up, once per (context, term set): every rank exports
 * the handle of its arena -- ONE allocation that holds the two receive buffers of each chain and the mailbox -- with the
 * five objects' byte offsets, the host passes them around (64 + 40 bytes, any transport) and every rank attaches every peer's.  No torch / RCCL call per evaluation; results are
 * those of the staged path (same kernels in the same order).  v_work_local_dev: a slab-sized work array for dE/dn. */
int  ofdft_ipc_export(ofdft_ctx* ctx, void* handle64, unsigned long long* offsets5);
int  ofdft_ipc_attach(ofdft_ctx* ctx, int peer_rank, const void* handle64, const unsigned long long* offsets5);
/* Close every mapping of a peer's arena this rank holds: the first step of tearing a slab job down -- every rank calls it,
 * the host's ranks meet (a barrier), and only then is any context destroyed: ofdft_destroy frees the arena, and device memory
 * must not be freed while a peer process still has it open through hipIpc.  (While a job runs nothing exported is freed and nothing
 * opened is closed: a term set that needs bigger buffers gets a second arena, csrc/ipc_exchange.inc.h.)  No-op on a context that never attached. */
int  ofdft_ipc_detach(ofdft_ctx* ctx);
int  ofdft_dist_closure(ofdft_ctx* ctx, const void* chi_local_dev, const void* vext_local_dev, double n_electrons_global,
                        double* E_terms_host, double* mu_host, void* grad_local_dev, void* v_work_local_dev, void* stream);

/* ---- collectives for the slab-decomposed per-geometry-step routines --------------------------------------------
 * The hot path (ofdft_dist_*) is staged so that the HOST issues its all-to-alls between stages.  The routines that run
 * once per geometry step (ofdft_stress, ofdft_ionic_potential, ofdft_ion_electron_forces, ofdft_ion_electron_stress)
 * need several distributed transforms and reductions in one call; on a slab-decomposed context they call back into the
 * host's communication layer (torch.distributed over RCCL in professad_amd.distributed; anything with these semantics):
 *   all_to_all(user, send_dev, recv_dev, bytes_per_peer, stream): equal-split all-to-all of device buffers (peer p's chunk
 *       at offset p * bytes_per_peer), ordered after the work already enqueued on `stream`; work enqueued on `stream`
 *       after the call returns is ordered after the exchange.
 *   all_reduce(user, host_buf, count): in-place sum over the ranks of `count` doubles in HOST memory.
 * Both return 0 on success.  Every rank must make the same sequence of calls (they are collective). */
typedef int (*ofdft_all_to_all_fn)(void* user, void* send_dev, void* recv_dev, unsigned long long bytes_per_peer, void* stream);
typedef int (*ofdft_all_reduce_fn)(void* user, double* host_buf, int count);
int  ofdft_set_collectives(ofdft_ctx* ctx, ofdft_all_to_all_fn all_to_all, ofdft_all_reduce_fn all_reduce, void* user);

/* ---- slab-decomposed evaluation over several GPUs (one process per GPU) --------------------
 * Rank r of P owns the real-space x-slab [n0/P][n1][n2].  The evaluation is cut at the four points where the
 * spectra change between the x-slab geometry (z, y passes) and the y-slab geometry (x pass); at each one the
 * engine's kernels leave the spectra in sendbuf in the exchange layout, the HOST does one equal-split all-to-all
 * (RCCL through torch.distributed) from sendbuf to recvbuf, and the next step's kernels read recvbuf directly.
 * The work is two independent chains (0: density / Hartree / vW / PBE, 1: nonlocal KEDF) with their own buffers, so
 * one chain's all-to-all can be in flight while the other chain computes.
 * The exchange buffers are chunk-major -- [chunk][peer][xl][array][...] over K = ofdft_query(OFDFT_Q_XCHG_CHUNKS) ranges of kz
 * blocks -- so chunk k of an exchange is one contiguous equal-split all-to-all message, and an exchange also overlaps the kernels
 * of its OWN chain ("overlap by z-chunks"; the reference is single-device, _optimizers/lbfgs/lbfgsnew.py:31-33, so
 * this has no counterpart there).  Per chain, ofdft_dist_step(step, chain, chunk), each step for chunk = 0 .. K-1 in order:
 *     1  [chunk 0: z kernels]  y-forward of the chunk into the send buffer                  -> exchange of the chunk
 *     2  fused x passes of the chunk, receive buffer -> send buffer                          -> exchange of the chunk
 *     3  y-inverse of the chunk out of the receive buffer
 *     4  [chunk 0: whole-row kernels (GGA mid stage, WGC99 combine)]  y-forward of the flux  -> exchange (chain 0 with a GGA term)
 *     5  fused x pass of the divergence                                                      -> exchange of the chunk
 *     6  y-inverse of the divergence chunk
 * then ofdft_dist_finish.  A call out of this order -- or chain 1 before step 1 of chain 0, or ofdft_dist_finish before step 6
 * of both chains -- returns OFDFT_ESTATE and runs nothing; the next ofdft_dist_begin starts from a clean state.  The kernels of
 * (step, chunk k) need only chunk k of the preceding exchange: the host keeps chunk k's all-to-all in flight while it enqueues
 * chunk k + 1.  *bytes_per_peer = 0: nothing to exchange after this call; otherwise sendbuf / recvbuf address the chunk's
 * region.  Results are bitwise those of the unchunked sequence (same kernels per line).
 * ofdft_dist_stage(stage, chain) is the shorthand for K == 1 (with K > 1 it returns OFDFT_ESTATE): stage 1 = step 1,
 * stage 2 = step 2, stage 3 = steps 3 + 4, stage 4 = step 5, returning the message of its last step; ofdft_dist_finish then runs
 * step 6 itself.  Both calls advance the same progress, so they may be mixed within one evaluation.
 * Sequence per evaluation:
 *     ofdft_dist_sumsq (closure form only) -> all-reduce -> c = N_e / (mean chi^2 vol)
 *     ofdft_dist_begin; for step in 1..6, for chain in 0..1, for chunk in 0..K-1: [wait for that chunk of the chain's previous
 *         all-to-all] ofdft_dist_step(step, chain, chunk) + all_to_all(bytes_per_peer)  (asynchronous if the transport allows);
 *     [wait for both] ofdft_dist_finish -> all-reduce of OFDFT_NSUMS local sums -> ofdft_dist_energies; ofdft_dist_chi_grad.
 * Device-resident scalars (no host round trip before the final sums): pass local_sum_host = NULL to
 * ofdft_dist_sumsq, all-reduce scalars[OFDFT_SCALAR_SUMSQ] in place (ofdft_dist_scalars), call ofdft_dist_begin with from_chi = 2
 * (the closure scale is then formed on the device), ofdft_dist_finish with local_sums_host = NULL, all-reduce
 * scalars[0 .. OFDFT_NSUMS - 1] in place and copy them to the host once; ofdft_dist_chi_grad with cscale = 0 uses the device scale.
 * With nranks == 1 the same calls work and every bytes_per_peer is 0.  These stand behind the same reference
 * interfaces as ofdft_energy_potential / ofdft_energy_grad_chi (system.py:830-838, functional_tools.py:9-31). */
int  ofdft_create_dist(ofdft_ctx** out, int n0_global, int n1_global, int n2, int dtype, int device_id, int nranks, int rank);
int  ofdft_dist_sumsq(ofdft_ctx* ctx, const void* x_local_dev, int square, double* local_sum_host, void* stream);
int  ofdft_dist_begin(ofdft_ctx* ctx, const void* src_local_dev, int from_chi, double cscale, double n_electrons_global,
                      const void* vext_local_dev, void* v_out_local_dev, void* stream);
int  ofdft_dist_step(ofdft_ctx* ctx, int step, int chain, int chunk, void* stream, unsigned long long* bytes_per_peer,
                     void** sendbuf_dev, void** recvbuf_dev);
int  ofdft_dist_stage(ofdft_ctx* ctx, int stage, int chain, void* stream, unsigned long long* bytes_per_peer, void** sendbuf_dev,
                      void** recvbuf_dev);
int  ofdft_dist_finish(ofdft_ctx* ctx, double* local_sums_host /*[OFDFT_NSUMS] or NULL*/, void* stream);
int  ofdft_dist_scalars(ofdft_ctx* ctx, void** scalars_dev /* OFDFT_NSCALARS doubles owned by the context */);
int  ofdft_dist_energies(ofdft_ctx* ctx, const double* global_sums /*[OFDFT_NSUMS]*/, double* E_terms_host, double* vn_integral);
int  ofdft_dist_chi_grad(ofdft_ctx* ctx, const void* chi_local_dev, const void* v_local_dev, void* grad_local_dev,
                         double cscale, double mu, void* stream);

/* Ionic (external) potential of one species on the grid: v(r) = irfftn(S(k) v~(|k|), norm='forward') / vol with the
 * exact structure factor (pme_order = 0) or its particle-mesh-Ewald approximation of even order >= 2, and v~ the
 * cubic-Hermite interpolation of a reciprocal-space pseudopotential table (uniform k grid from 0; the Coulomb tail
 * 4 pi z / k^2 already ADDED to the table for k > 0, exactly as the reference prepares it).  Stands behind
 * System.__potential_from_ions (system.py:183-194) = lattice_sum + structure_factor[_spline] + interpolate_recpot
 * (ion_utils.py:49-286).  frac_coords_host: [nions][3] fractional coordinates (host); vext_dev: [n0][n1][n2] device
 * array that receives (accumulate = 0) or is incremented by (accumulate = 1) the potential. */
int  ofdft_ionic_potential(ofdft_ctx* ctx, const double* frac_coords_host, int nions, const double* table_k_host,
                           const double* table_v_host, int ntable, double z_ion, int pme_order, void* vext_dev,
                           int accumulate, void* stream);

/* Ion-electron forces of one species for a given density: F_a = -d/dR_a int n v_ext (Ha/bohr, [nions][3] on the host),
 * with the same structure-factor options as ofdft_ionic_potential.  Stands behind the IonElectron part of
 * System.__compute_forces (system.py:913-923), which the reference obtains by autograd through the potential build. */
int  ofdft_ion_electron_forces(ofdft_ctx* ctx, const void* den_dev, const double* frac_coords_host, int nions,
                               const double* table_k_host, const double* table_v_host, int ntable, double z_ion,
                               int pme_order, double* forces_host, void* stream);

/* ---- stress -----------------------------------------------------------------------------
 * sigma_ij = (1/Omega) dE/d eps_ij at fixed electron number, per term: what get_stress (functional_tools.py:73-101)
 * and System.__compute_stress (system.py:925-935) obtain by autograd through every FFT.  Closed forms of the
 * reference's own analytic tests (tests/tools_for_tests.py:212-307, 367-472) for Hartree, TF, Wang-Teter, LDA, PBE; the
 * exact discrete forms for vW, the density-dependent WGC99 kernel and the ion-electron term are derived in
 * oracle/stress.py.  sigma_terms_host[OFDFT_NTERMS][9]: row-major symmetric 3x3 per term bit, Ha/bohr^3; the
 * ion-electron entry stays zero (it needs the ions: ofdft_ion_electron_stress, same arguments as the forces). */
int  ofdft_stress(ofdft_ctx* ctx, const void* den_dev, double* sigma_terms_host, void* stream);
int  ofdft_ion_electron_stress(ofdft_ctx* ctx, const void* den_dev, const double* frac_coords_host, int nions,
                               const double* table_k_host, const double* table_v_host, int ntable, double z_ion,
                               int pme_order, double* sigma_host /*[9]*/, void* stream);

/* ---- Hessian-vector product: the second functional derivative applied to a direction ---------------------------------
 * hv(r) = d/d eps v[n + eps w](r) at eps = 0, v = dE/dn as ofdft_energy_potential returns it: with H_ij = d^2 E / dn_i dn_j of the
 * grid values, hv = (H w) / dV.  It stands behind what the reference obtains by differentiating a potential a second time through
 * autograd: get_inv_G (functional_tools.py:34-70), get_functional_derivative(..., requires_grad=True) (functional_tools.py:9-31) and the
 * implicit-function solves of System's second-order derivative terms -- bulk modulus, elastic constants, force constants
 * (system.py:1204-1367), each a linear system in this operator.  den_dev > 0, dir_dev any real grid, hv_dev receives hv;
 * quad_terms_host[t] = sum_i w_i hv_t,i dV = int w (H_t w) per term bit (entries of unset terms 0; NULL skips the host read).
 * Served: ion_electron (hv = 0, no vext needed), hartree, tf, vw, wt_nl (any alpha, beta), lda_x, pz_c, pw_c, chachiyo_c.  In wt_nl the
 * n0 of the kernel is mean(den) vol of the den passed in and a CONSTANT of the differentiation (functionals.py:646-647 take it with
 * .item()), so a finite difference of the potential along a w of non-zero mean differs.  Refused with OFDFT_EINVAL, the message
 * naming the term: wgc99_nl (unless OFDFT_OPT_HVP_WGC = 1, below), pbe_x, pbe_c (unless OFDFT_OPT_HVP_GGA = 1, below), gga_k, vwgtf, nlk,
 * OFDFT_P_WTS_KIND = 1;
 * slab-decomposed contexts; the fp32 library.
 * reuse_density: 0 computes everything and leaves the density-only fields (lap sqrt n, K * n^beta, K * n^alpha) in workspaces of their
 * own; 1 = the caller asserts den holds the values of the previous call made with 0 and those transforms are skipped (Hartree 1 + 1
 * transforms either way; vW 2 + 2, with reuse 1 + 1; wt_nl 2 + 2 / 1 + 1 for alpha = beta, else 4 + 4 / 2 + 2) -- bitwise the same
 * hv.  ofdft_set_cell, ofdft_set_terms, ofdft_set_option and every other evaluation (energy, stress, ofdft_dist_*, ofdft_rfftn /
 * ofdft_irfftn) invalidate the retained fields; 1 with nothing valid retained returns OFDFT_ESTATE.  Sets OFDFT_Q_FFT_COUNT,
 * OFDFT_Q_LAUNCH_COUNT and OFDFT_Q_KERNEL_MS as the energy calls do.  No atomics: bitwise reproducible.
 * With OFDFT_OPT_HVP_GGA = 1 this entry and ofdft_hessian_vector_chi also serve pbe_x and pbe_c: for
 * E = dV sum f(n, sigma), sigma = sum_a (D_a n)^2, dsigma = 2 sum_a D_a n D_a w,
 *     hv = f_nn w + f_nsigma dsigma - 2 sum_a D_a [(f_sigma,n w + f_sigma,sigma dsigma) D_a n + f_sigma D_a w]
 * in two transform stages around a pointwise mid kernel: 2 + 6 + 3 + 1 = 12 transforms more, 8 with reuse_density = 1 (grad n joins
 * the retained fields; the second partials are formed again on every call).  quad_terms_host reports pbe_x and pbe_c from
 * sum f_nn w^2 + 2 f_nsigma w dsigma + f_sigma,sigma dsigma^2 + 2 f_sigma |grad w|^2.  Limits: den > 0 everywhere, as for
 * evaluating PBE itself; single GPU; fp64.
 * With OFDFT_OPT_HVP_WGC = 1 the two entries also serve wgc99_nl.  n_ref = kappa round(N) / vol is a CONSTANT of the
 * differentiation (functionals.py:952-954 take round(N) with .item(); N = mean(den) vol of the den passed in, n_electrons in chi
 * space), so with theta = n - n_ref, a = (A, A theta, A theta^2 / 2), A = n^beta, p likewise with n^alpha, and the symmetric block M of
 * the evaluation's kernel tables, E = c dV sum p . (M a), U = M a, G = M p and
 *     hv = c sum_i [ p_i'' w U_i + p_i' (M (a' w))_i + a_i'' w G_i + a_i' (M (p' w))_i ]
 * from a head kernel, four triples of transforms around the evaluation's spectral mix and a tail kernel: 6 + 6 + 6 + 6 = 24 transforms
 * more, 12 with reuse_density = 1 (U and G join the retained fields).  quad_terms_host reports wgc99_nl from sum w hv of that field. */
int  ofdft_hessian_vector(ofdft_ctx* ctx, const void* den_dev, const void* dir_dev, void* hv_dev,
                          double* quad_terms_host /* [OFDFT_NTERMS] or NULL */, int reuse_density, void* stream);

/* The same second derivative in the optimiser's variable.  phi = chi_dev is the caller's chi at any scale,
 * S = sum phi^2, c = N / (S dV), n = c phi^2, and g = 2 c phi (v - mu) dV is what ofdft_energy_grad_chi leaves in grad_dev
 * (phi . g = 0).  For a direction d with a = phi . d the call writes the derivative of g along d,
 *     dn = 2 c phi d - (2 a / S) n        dv = hv(n, dn)        dmu = (sum dv n dV + g . d) / N
 *     (H d)_j = -(2 a / S) g_j + d_j g_j / phi_j + 2 c phi_j (dv_j - dmu) dV
 * to out_dev.  Where phi_j = 0 the quotient d_j g_j / phi_j counts as 0: its exact value there, 2 c d_j (v_j - mu) dV, cannot be
 * formed from g.  g_dev = NULL stands for a stationary point (g = 0; bitwise the result of a zero array).  scalars_host, if
 * given, receives d . H d, phi . H d, a, S and dmu (OFDFT_HVC_*).  reuse_density = 1 asserts that phi holds the values of the
 * previous call made with 0: n, S, c and the density-only fields are kept and the smaller transform count runs; what
 * invalidates the retained fields of ofdft_hessian_vector invalidates these, and the two entries do not reuse each other's
 * fields.  Single GPU and fp64; the same terms are refused, by name.  The chi-space arithmetic runs inside the product's head
 * and combine kernels; the call adds one sweep over (phi, d) in front and one over (phi, out) behind.  No atomics. */
#define OFDFT_HVC_DHD 0
#define OFDFT_HVC_PHIHD 1
#define OFDFT_HVC_A 2
#define OFDFT_HVC_S 3
#define OFDFT_HVC_DMU 4
#define OFDFT_HVC_NSCALARS 5
int  ofdft_hessian_vector_chi(ofdft_ctx* ctx, const void* chi_dev, const void* dir_dev, const void* g_dev /* or NULL */,
                              double n_electrons, void* out_dev, double* scalars_host /* [OFDFT_HVC_NSCALARS] or NULL */,
                              int reuse_density, void* stream);

/* The kinetic preconditioner of the conjugate gradients below:  z = irfftn( rfftn(r) / (k^2 + kappa2) ), k as
 * everywhere in the engine, kappa2 > 0 [1/bohr^2].  In chi the von Weizsaecker Hessian is c dV (-lap), so 1 / (k^2 + kappa2) with
 * kappa2 = (4/3) k_F^2 (the Thomas-Fermi shift) follows the stiff end of H up to a constant factor.  Fused x pass where it serves
 * the grid (five spectrum passes), chirp-z x-mix on chirp-z extents, and forward, multiply, inverse elsewhere and under
 * OFDFT_OPT_PIPELINE = 1.  It leaves the fields retained for reuse_density = 1 valid and touches no workspace of the products
 * but a transient spectrum, so it may run between two products.  Single GPU and fp64: the fp32 library and slab-decomposed
 * contexts return OFDFT_EINVAL, as do kappa2 <= 0 or non-finite and z_dev == r_dev.  Synchronises the stream.  No atomics. */
int  ofdft_precondition(ofdft_ctx* ctx, const void* r_dev, void* z_dev, double kappa2, void* stream);

/* Several right-hand sides per call.  The response drivers solve with the same Hessian for many perturbations;
 * these entries run the stationary-point product (g = 0) and the preconditioner for ncols = 1 .. OFDFT_MULTI_MAX columns at once.
 * Column j of a stack is base + j * stride elements (stride >= the points of a column; any parity).
 *   ofdft_hessian_vector_chi_multi  out_j = H d_j as ofdft_hessian_vector_chi forms it with g_dev = NULL, to rounding (not
 *       bitwise: the density-only factors of a point are formed once and serve every column).  One sweep and one fetch for all
 *       a_j = phi . d_j and S; one head kernel that reads phi once and writes the density-only fields once; the transforms in
 *       batches through the whole-grid transforms (chirp-z extents: up to four fields per launch; the fused radix extents one
 *       field per launch); one spectral kernel over every spectrum; one combine kernel; one reduction; one shift; one
 *       synchronisation.  scalars_host [ncols][OFDFT_HVC_NSCALARS], in the order of the single-column entry.  The retained
 *       density fields are those of ofdft_hessian_vector_chi: with reuse_density = 1 either entry may follow a reuse_density = 0
 *       call of the other on the same phi, cell and term set, and what invalidates them for one invalidates them for both.
 *       OFDFT_Q_FFT_COUNT: 2 (D + ncols W), with reuse 2 ncols W (D density-only, W per-direction transforms of the term set).
 *   ofdft_precondition_multi  z_j = irfftn(rfftn(r_j) / (k^2 + kappa2)), one synchronisation at the end; leaves the retained
 *       fields alone like ofdft_precondition.
 * OFDFT_EINVAL, the message naming the limit or the argument: ncols outside 1 .. OFDFT_MULTI_MAX, a stride below the points of a
 * column, an output stack that overlaps the input stack, and whatever the single-column entries refuse.  fp64, single GPU. */
#define OFDFT_MULTI_MAX 8
int  ofdft_hessian_vector_chi_multi(ofdft_ctx* ctx, const void* chi_dev, const void* dirs_dev, long long dir_stride, int ncols,
                                    double n_electrons, void* out_dev, long long out_stride,
                                    double* scalars_host /* [ncols][OFDFT_HVC_NSCALARS] or NULL */, int reuse_density, void* stream);
int  ofdft_precondition_multi(ofdft_ctx* ctx, const void* r_dev, long long r_stride, void* z_dev, long long z_stride, int ncols,
                              double kappa2, void* stream);

/* Ion-ion interaction: the real-space damped pair sum in a neutralising background of
 * ion_interaction_sum (ion_utils.py:293-333) with System.__ion_ion_interaction's parameters (system.py:733-754);
 * Rc <= 0 selects its default Rd = 2 h_max, Rc = 3 Rd^2 / h_max.  The pair list (torch-nl's neighbour list in the
 * reference) is every (i, j, lattice shift) with 0 < r <= Rc.  forces_host [nions][3] = -dE/dR and stress_host [9] =
 * (1/vol) dE/d eps are what autograd gives the reference (system.py:913-935); either may be NULL. */
int  ofdft_ion_ion(ofdft_ctx* ctx, const double* frac_coords_host, const double* charges_host, int nions, double Rc,
                   double* E_host, double* forces_host, double* stress_host, void* stream);

/* The same sum through a cell list, for supercells (ion_utils.py:293-333, whose pairs come from a cell-list neighbour list,
 * :313-316; parameters system.py:733-754; forces and stress as autograd gives them, system.py:913-935).  Ions are wrapped into
 * the cell, sorted into m0 x m1 x m2 cells along the lattice axes, and each target cell scans the cells that can hold an ion
 * within Rc of it, with the lattice shift of every wrap: the pair set is that of the entry above, at a cost proportional to
 * the pairs instead of nions^2 x shifts.  Rc <= 0: the reference's default (Rd = 2 h_max, Rc = 3 Rd^2 / h_max); Rc > 0 and
 * Rd <= 0: Rd = sqrt(h_max Rc / 3) as above; Rc > 0 and Rd > 0: both as given (what ion_interaction_sum itself accepts).
 * part / nparts: the call does the work of the target cells [part ncells / nparts, (part + 1) ncells / nparts) of the cell
 * order and returns that share: the energy and stress terms of their ions, and force rows for those ions only (zero
 * elsewhere); the sum over parts is the whole result, and 0, 1 is the whole sum.  Only sorted coordinates, charges and cell
 * offsets go to the device; eight numbers and the owned force rows come back.  No atomics: bitwise reproducible. */
int  ofdft_ion_ion_cells(ofdft_ctx* ctx, const double* frac_coords_host, const double* charges_host, int nions, double Rc,
                         double Rd, int part, int nparts, double* E_host, double* forces_host /* [nions][3] or NULL */,
                         double* stress_host /* [9] or NULL */, void* stream);

/* ---- second derivatives with respect to ion positions: the pieces of the interatomic force constants ----
 * System.force_constants (system.py:695-717, 1340-1367) differentiates the forces F = -dE_tot/dR at the relaxed density once
 * more by autograd:  Phi[p,b] = -dF_p/dR_b = Phi_ion-ion[p,b] + delta_pb D[p] - F_ie[dn_(p,i)][b], with dn_(p,i) the
 * ground-state density response (a conjugate-gradient solve with ofdft_hessian_vector_chi) to dv = d v_ext / d R_{p,i} and F_ie
 * the linear map of ofdft_ion_electron_forces.  The three entries below supply dv, D and Phi_ion-ion.  fp64 and single GPU;
 * the fp32 library and slab-decomposed contexts return OFDFT_EINVAL.  Each clears the fields ofdft_hessian_vector[_chi] retain.
 * No atomics: bitwise reproducible.
 *
 * ofdft_ionic_potential_gradient: the three grids d v_ext / d R_{a,x|y|z} of the ion a = ion_index of one species,
 *     d v_ext / d R_{a,j} (r) = irfftn(-i k_j exp(-i k.R_a) v~(|k|), norm='forward') / vol,
 * into dv_dev [3][n0][n1][n2]: the Jacobian autograd takes through lattice_sum + structure_factor (ion_utils.py:88-137), with
 * the c2r semantics of ofdft_ionic_potential (imaginary parts at the self-conjugate k_z dropped).  Table arguments as there.
 * One spectral kernel (phase and table value once per k-point), one batched inverse transform of three spectra.
 * pme_order != 0 returns OFDFT_EINVAL, the message naming PME: the derivative of the B-spline spread is not built. */
int  ofdft_ionic_potential_gradient(ofdft_ctx* ctx, const double* frac_coords_host, int nions, const double* table_k_host,
                                    const double* table_v_host, int ntable, double z_ion, int pme_order, int ion_index,
                                    void* dv_dev /* [3][n0][n1][n2] */, void* stream);

/* D[a] = d^2 (dV sum_r n v_ext) / dR_a dR_a at fixed density for every ion of one species -- the diagonal blocks of the Hessian
 * of U(R) = IonElectron(box, den, v_ext(R)) (functionals.py IonElectron over lattice_sum, ion_utils.py:88-137; the off-diagonal
 * blocks vanish: v_ext is a sum over ions),
 *     D[a]_ij = -(dV / vol) sum_k w_k v~(|k|) k_i k_j Re(exp(-i k.R_a) conj(n^_k)),   w_k = the half-spectrum multiplicities.
 * curv_host [nions][6]: xx, yy, zz, xy, xz, yz (Ha/bohr^2).  One transform of the density, one reduction kernel.  PME refused. */
int  ofdft_ion_electron_curvature(ofdft_ctx* ctx, const void* den_dev, const double* frac_coords_host, int nions,
                                  const double* table_k_host, const double* table_v_host, int ntable, double z_ion,
                                  int pme_order, double* curv_host /* [nions][6] */, void* stream);

/* Second derivative of the ion-ion pair sum for the ions p of rows_host: hess_host [nrows][nions][3][3] = d^2 E / dR_p dR_b
 * (Ha/bohr^2) at a fixed pair list -- a second autograd pass over ion_interaction_sum (ion_utils.py:293-333); the background term
 * depends on the neighbour charge counts only and drops out.  Rd / Rc and the pair set 0 < r <= Rc are those of ofdft_ion_ion.
 * With f(r) = Z_p Z_b erfc(r/Rd)/r and T(d) = (f'' - f'/r) d d^T / r^2 + (f'/r) I: block b != p is -sum over shifts of T, the
 * diagonal block +sum over b != p and shifts (an ion's own images move with it).  A block depends on (p, b) and the geometry
 * only: any subset of rows returns the same bits. */
int  ofdft_ion_ion_hessian(ofdft_ctx* ctx, const double* frac_coords_host, const double* charges_host, int nions, double Rc,
                           const int* rows_host, int nrows, double* hess_host /* [nrows][nions][3][3] */, void* stream);

/* ---- second strain derivative at fixed chi (the fixed-chi part of the elastic constants) --------------------------
 * The cell is strained as h -> h (I + eps) with a general eps at fixed fractional ion coordinates, fixed grid values of chi and
 * fixed N, so the density scales as 1 / det(I + eps).  Each entry returns d^2 E / d eps_mn d eps_pq at eps = 0 as [3][3][3][3]
 * row-major in (m, n, p, q), Ha -- what torch.autograd.functional.hessian gives in eps through the closure of
 * System.__compute_elastic_constants (system.py:1266-1273) with chi held fixed.  fp64, single GPU, exact structure factor;
 * reductions by wavefront shuffles and a fixed-order host sum: bitwise reproducible.  Each clears the retained fields of
 * ofdft_hessian_vector.
 *
 * ofdft_strain_hessian: the reciprocal-space terms of the active set (hartree, vw, wt_nl) at the density den_dev; the other
 * entries of w2_terms_host are zero (tf, lda_x and the LDA correlations depend on det(I + eps) alone: E_J from the trace of
 * ofdft_stress, E_JJ = n.H_t n from ofdft_hessian_vector).  Refuses what ofdft_hessian_vector refuses, by name. */
int  ofdft_strain_hessian(ofdft_ctx* ctx, const void* den_dev, double* w2_terms_host /* [OFDFT_NTERMS][81] */, void* stream);

/* ---- strain gradient of the potential (the coupling of the strain to the density response) ------------------------
 * v_eps,kl(r), kl = xx, yy, zz, yz, xz, xy: the derivative of the potential v = dE/dn of the active terms with respect to
 * eps_kl at FIXED grid values of the density, the mean density of the Wang-Teter kernel following the cell (n0 = N / vol):
 *   hartree  F^-1[8 pi k_k k_l n^ / k^4];   vw  -F^-1[k_k k_l chi^] / chi;
 *   wt_nl    c_TF [alpha n^(alpha-1) K'_kl * n^beta + beta n^(beta-1) K'_kl * n^alpha],
 *            K'_kl = pref [delta_kl ((alpha + beta - 5/3) F + eta F' / 3) - eta F' k_k k_l / k^2];
 * tf, lda_x and the LDA correlations have no explicit part.  The total strain derivative of the potential at fixed chi is
 * V_kl = v_eps,kl - delta_kl hv(n, n) (ofdft_hessian_vector), since n ~ 1 / det(I + eps).  One forward and six inverse
 * transforms per family (OFDFT_Q_FFT_COUNT: 3 + 18 for hartree + vw + wt_nl with alpha = beta).  Refuses what
 * ofdft_hessian_vector refuses. */
int  ofdft_potential_strain_gradient(ofdft_ctx* ctx, const void* den_dev, void* out6_dev /* [6][n0][n1][n2] */, void* stream);

/* The same for v_ext of one species at fixed fractional coordinates (arguments of ofdft_ionic_potential):
 *   -delta_kl v_ext + F^-1[S v~'(|k|) (-k_k k_l / |k|)] / vol,  v~' = 0 past the table end.  PME refused. */
int  ofdft_ionic_potential_strain_gradient(ofdft_ctx* ctx, const double* frac_coords_host, int nions, const double* table_k_host,
                                           const double* table_v_host, int ntable, double z_ion, int pme_order,
                                           void* out6_dev /* [6][n0][n1][n2] */, void* stream);

/* The ion-electron energy of one species, the potential rebuilt from the ions in the strained cell (arguments of
 * ofdft_ion_electron_stress).  PME refused. */
int  ofdft_ion_electron_strain_hessian(ofdft_ctx* ctx, const void* den_dev, const double* frac_coords_host, int nions,
                                       const double* table_k_host, const double* table_v_host, int ntable, double z_ion,
                                       int pme_order, double* w2_host /* [81] */, void* stream);

/* The ion-ion energy over the fixed pair list of ofdft_ion_ion; Rd and Rc are constants of the differentiation (the reference
 * takes h_max from box_vecs.detach()), the background term varies through rho ~ 1/J and R_a ~ J^(1/3). */
int  ofdft_ion_ion_strain_hessian(ofdft_ctx* ctx, const double* frac_coords_host, const double* charges_host, int nions, double Rc,
                                  double* w2_host /* [81] */, void* stream);

/* ---- limited-memory BFGS building blocks (the consumer of the closure) ----------------
 * The reference's fixed-step optimiser (_optimizers/lbfgs/lbfgsnew.py:594-663) forms y = g - g_prev and s = t d, keeps
 * the pair if y.s > 1e-10 |s|^2, and gets the direction from the two-loop recursion: 2m dependent dot / axpy pairs over
 * full-grid vectors.  Here the history lives on the device and each inner iteration is two sweeps:
 *   ofdft_lbfgs_dots    forms the candidate pair from g, the previous gradient and the previous step, and returns every
 *                       inner product the recursion needs: for each stored pair j (oldest first) (s.S_j, y.S_j, g.S_j), then
 *                       (s.Y_j, y.Y_j, g.Y_j) for each j, then s.s, s.y, y.y, g.s, g.y, g.g, |g|_1  ->  6*npairs + 7 numbers
 *                       (LOCAL sums: all-reduce them over ranks when the vectors are slabs);
 *   ofdft_lbfgs_commit  stores (push = 1) or discards the candidate pair (the caller applies the curvature test);
 *   ofdft_lbfgs_update  d = coef_g g + sum_j coef_s[j] S_j + coef_y[j] Y_j over the stored pairs (oldest first, the
 *                       just-committed pair last), x += t d in place, g_prev = g; returns the local sum |t d|_1.
 *   ofdft_lbfgs_direction  the host side between the two sweeps, natively: curvature test + commit, the Gram blocks of the stored
 *                       pairs, the two-loop recursion on the COEFFICIENTS of d in {S_j, Y_j, g} (so the result is the reference's
 *                       direction up to round-off) -> coef_s, coef_y, coef_g for ofdft_lbfgs_update, and g.d.  A host that wants
 *                       its own recursion calls ofdft_lbfgs_commit itself instead (professad_amd/optimize.py keeps that form for
 *                       backends without this entry).
 * ofdft_lbfgs_update with abs_step_sum == NULL does not wait for the stream; ofdft_lbfgs_abs_step returns the sum after the
 * stream's next synchronisation (the closure evaluation that follows an update does one). */
typedef struct ofdft_lbfgs ofdft_lbfgs;
int  ofdft_lbfgs_create(ofdft_lbfgs** out, long long n_local, int history /* 1..8 */, int device_id);
void ofdft_lbfgs_destroy(ofdft_lbfgs* h);
const char* ofdft_lbfgs_last_error(const ofdft_lbfgs* h);
int  ofdft_lbfgs_reset(ofdft_lbfgs* h);
int  ofdft_lbfgs_direction(ofdft_lbfgs* h, const double* dots /* of ofdft_lbfgs_dots, summed over ranks */, int npairs, int first_iteration,
                           double* coef_s /* [history] */, double* coef_y /* [history] */, double* coef_g, double* g_dot_d,
                           int* npairs_out, int* pushed_out);
int  ofdft_lbfgs_abs_step(ofdft_lbfgs* h, double* abs_step_sum);
int  ofdft_lbfgs_dots(ofdft_lbfgs* h, const void* g_dev, double* dots_host /* [6*8+7] */, int* npairs, void* stream);
int  ofdft_lbfgs_commit(ofdft_lbfgs* h, int push);
int  ofdft_lbfgs_update(ofdft_lbfgs* h, const double* coef_s, const double* coef_y, double coef_g, double t, void* x_dev,
                        const void* g_dev, double* abs_step_sum_host, void* stream);

/* ---- conjugate gradients for P H P x = b, P = I - phi phi^T / (phi . phi), b perpendicular to phi ----------------
 * The solve behind truncated Newton and the density response (professad_amd/optimize.py).  x, r, p, q live in the handle; the
 * caller forms q = H p between the steps (ofdft_hessian_vector_chi with dir_dev = p, out_dev = q of ofdft_cg_vectors, whose
 * scalars are the p . q and phi . q that ofdft_cg_step takes).
 *   ofdft_cg_start  x = 0, r = p = b - phi (phi . b) / S; info_host [3] = |r|^2, S, phi . b.  rtol: stop at |r| <= rtol |r_0|.
 *   ofdft_cg_step   p . q <= 0: reason OFDFT_CG_CURVATURE, x stays (before the first update x = p).  Otherwise one update sweep
 *                   (x += alpha p, r -= alpha (q - phi (phi . q) / S); sums r . r, phi . r), the stopping rules, and one
 *                   direction sweep (p = r - phi (phi . r) / S + beta p).  One stream synchronisation.
 *   ofdft_cg_status iterations done, reason, |r| / |r_0|.        ofdft_cg_solution copies x to the caller's array.
 * These entries are the one-column case of ofdft_cgm_* below (a handle with ncols_max = 1, the scalars as one-element arrays, the
 * reason that of column 0): one solver, one set of kernels, the same bits.  No atomics: bitwise reproducible. */
#define OFDFT_CG_RUNNING   0
#define OFDFT_CG_CONVERGED 1
#define OFDFT_CG_MAXITER   2
#define OFDFT_CG_CURVATURE 3
typedef struct ofdft_cg ofdft_cg;
int  ofdft_cg_create(ofdft_cg** out, long long n, int device_id);
void ofdft_cg_destroy(ofdft_cg* h);
const char* ofdft_cg_last_error(const ofdft_cg* h);
int  ofdft_cg_start(ofdft_cg* h, const void* phi_dev, const void* b_dev, double rtol, int maxiter, double* info_host /* [3] or NULL */,
                    void* stream);
int  ofdft_cg_vectors(ofdft_cg* h, void** x_dev, void** r_dev, void** p_dev, void** q_dev);
int  ofdft_cg_step(ofdft_cg* h, const void* phi_dev, double p_dot_q, double phi_dot_q, int* reason, void* stream);
int  ofdft_cg_status(const ofdft_cg* h, int* iterations, int* reason, double* rel_residual);
int  ofdft_cg_solution(ofdft_cg* h, void* x_out_dev, void* stream);

/* Preconditioned mode of the same handle, opt-in: with it off nothing above changes, launch for launch.
 *   ofdft_cg_set_preconditioned  on != 0: the solves begun by the following ofdft_cg_start calls run preconditioned.  Default 0.
 *   ofdft_cg_z         the handle's vector z (allocated on first use).  Before every ofdft_cg_direction the caller writes
 *                      z = M^-1 r there, r being that of ofdft_cg_vectors (ofdft_precondition, or any symmetric positive definite M^-1).
 *   ofdft_cg_direction one sweep for r . z and phi . z, then rho = r . z - (phi . r)(phi . z) / S, beta = rho / rho_old (0 on the
 *                      first call after ofdft_cg_start), and one sweep p = (z - phi (phi . z) / S) + beta p.  phi . r is the sum of
 *                      the last update sweep.  info_host [4] = r . z, phi . z, rho, beta.  rho <= 0 or NaN: reason
 *                      OFDFT_CG_CURVATURE, x and p stay.  One stream synchronisation.
 * In this mode ofdft_cg_start stops after r = P b, and ofdft_cg_step takes alpha = rho / (p . q), runs the update sweep and the
 * stopping rules -- on r . r, as in plain mode, so |r| / |r_0| keeps its meaning -- and no direction sweep.  One iteration is
 * direction, product, step.  OFDFT_ESTATE: ofdft_cg_direction in plain mode, before ofdft_cg_start, after the solve has ended or
 * twice for one step; ofdft_cg_step before the direction of the step is formed.  No atomics: bitwise reproducible. */
int  ofdft_cg_set_preconditioned(ofdft_cg* h, int on);
int  ofdft_cg_z(ofdft_cg* h, void** z_dev);
int  ofdft_cg_direction(ofdft_cg* h, const void* phi_dev, double* info_host /* [4] or NULL */, int* reason, void* stream);

/* ---- the same solver for several right-hand sides in lockstep ------------------------------------
 * A handle for (n, ncols_max <= OFDFT_MULTI_MAX, device) holds x, r, p, q, z as [ncols_max] columns at the stride that
 * ofdft_cgm_vectors reports (n rounded up to even), and per column rho, phi . r, |r|^2, |r_0|^2, the iteration count and the exit
 * reason.  Not block Krylov: the columns share phi and S only, and each runs the recurrence of ofdft_cg_* with its own alpha and
 * beta, so a column's result, reason and count are those of a solo solve (its sums do not depend on the columns beside it).
 * Every sweep is one launch for all columns -- the column is the grid's y index, the per-column coefficients travel by value --
 * and one fetch of all columns' sums.  A column that has ended (converged, curvature, maxiter, NaN) is frozen: no later sweep
 * writes its x or r, and its reason and count stay.  The caller's product (ofdft_hessian_vector_chi_multi on p -> q of all
 * ncols columns) goes on computing a frozen column's q, which nothing reads: the product's cost per column is small beside
 * what the columns share, and the columns of one ground state end within a few iterations of each other.
 *   ofdft_cgm_start      b_j at b_stride, ncols <= ncols_max; info_host [ncols][3] as ofdft_cg_start.  b_j = 0: converged, x_j = 0.
 *   ofdft_cgm_step       p_dot_q [ncols], phi_dot_q [ncols] (those of ended columns are not read); *running = columns still running.
 *   ofdft_cgm_direction  preconditioned mode, with z_j = M^-1 r_j written for the running columns; info_host [ncols][4].
 *   ofdft_cgm_status     of column col.        ofdft_cgm_solution copies the x_j to the caller's stack at its stride.
 * OFDFT_ESTATE as for ofdft_cg_*, "ended" meaning every column; OFDFT_EINVAL names the limit.  No atomics. */
typedef struct ofdft_cgm ofdft_cgm;
int  ofdft_cgm_create(ofdft_cgm** out, long long n, int ncols_max, int device_id);
void ofdft_cgm_destroy(ofdft_cgm* h);
const char* ofdft_cgm_last_error(const ofdft_cgm* h);
int  ofdft_cgm_vectors(ofdft_cgm* h, void** x_dev, void** r_dev, void** p_dev, void** q_dev, long long* stride);
int  ofdft_cgm_z(ofdft_cgm* h, void** z_dev);
int  ofdft_cgm_set_preconditioned(ofdft_cgm* h, int on);
int  ofdft_cgm_start(ofdft_cgm* h, const void* phi_dev, const void* b_dev, long long b_stride, int ncols, double rtol, int maxiter,
                     double* info_host /* [ncols][3] or NULL */, void* stream);
int  ofdft_cgm_step(ofdft_cgm* h, const void* phi_dev, const double* p_dot_q, const double* phi_dot_q, int* running, void* stream);
int  ofdft_cgm_direction(ofdft_cgm* h, const void* phi_dev, double* info_host /* [ncols][4] or NULL */, int* running, void* stream);
int  ofdft_cgm_status(const ofdft_cgm* h, int col, int* iterations, int* reason, double* rel_residual);
int  ofdft_cgm_solution(ofdft_cgm* h, void* x_out_dev, long long stride, void* stream);

/* Tuning / validation switches.  OFDFT_OPT_PIPELINE: 0 = automatic (power-of-two grids: fused x passes and z
 * passes that keep every real-space intermediate on chip), 1 = force the unfused pipeline (separate forward,
 * multiply, inverse and pointwise passes; the only one for other grids), 2 = fused x passes only. */
#define OFDFT_OPT_PIPELINE 0
/* OFDFT_OPT_SIDE_STREAM: 1 (default) = run the nonlocal-KEDF chain of the z-fused pipeline on a second HIP stream so
 * that it overlaps the Hartree/vW/PBE chain (they only meet in the combine kernel); 0 = everything on the caller's stream. */
/* option numbers 2 and 3 (XCHUNKS, XCHUNK_MASK: the x-chunked single-GPU evaluation) are retired and are not to be reused */
#define OFDFT_OPT_SPLIT_COMBINE 4 /* with side streams, the WGC99 part of the combine runs as its own kernel on the nonlocal chain's stream; 2 (default): and in
                                     closure evaluations (ofdft_energy_grad_chi) the combine kernel does not wait for it -- the potential stays in two
                                     arrays that the chi.grad kernel adds, the part's share of sum(v n) joins the combine's; 1: the combine adds it; 0: off */
#define OFDFT_OPT_BLUESTEIN 5     /* 1 (default): extents that are not powers of two (<= 512) use chirp-z line transforms; 0: plain DFT kernels */
#define OFDFT_OPT_GGA_SPLIT 6     /* 1 (default): split-derivative GGA chain -- only the index derivative along x visits the x pass (and the exchange); 0: three Cartesian components */
#define OFDFT_OPT_GRAPH 7         /* 1 (default): ofdft_energy_grad_chi replays a hipGraph captured on the second call with the same
                                     arguments (device pointers, electron number, cell, terms, options): one graph launch instead
                                     of ~25-50 kernel launches, which is what bounds grids up to ~64^3 (used by single-GPU contexts up to 2^19 points, where
                                     OFDFT_OPT_SPLIT_COMBINE is then ignored); 0: always launch kernel by kernel */
#define OFDFT_OPT_SIDE_STREAM 1
#define OFDFT_OPT_MIXED_RADIX 9   /* 1 (default): extents with factors 3 and 5 that have a line-transform plan (48, 96, 120, 144, 160, 192, 240, 250, 270,
                                     288, 320, 384, 480) run the register / LDS transforms and the fused pipelines like the powers of two;
                                     0: they take the chirp-z transforms + the unfused pipeline like any other extent (validation, A/B) */
#define OFDFT_OPT_RESIDENT 10     /* ofdft_energy_grad_chi on cubic 16^3 / 32^3 / 64^3 grids with local, Hartree, von Weizsaecker and Wang-Teter terms (up to
                                     32^3 also PBE / LKT / mu-only Pauli-Gaussian and WGC99)
                                     runs as ONE persistent kernel (four phases, three grid barriers; csrc/resident.hip) instead of the staged
                                     pipeline.  2 (default): the call is not bracketed by the HIP event pair that times it (OFDFT_Q_KERNEL_MS reads
                                     0 for it) and the host watches a pinned word the last workgroup writes instead of waiting for the stream --
                                     together ~8 microseconds of a ~45-microsecond call; 1: events + stream wait as everywhere else; 0: off */
#define OFDFT_OPT_XCHG_CHUNKS 12  /* slab-decomposed contexts: the exchange buffers (and the k-point tables laid out like them) are cut into this many
                                     ranges of kz blocks, chunk-major, so that ofdft_dist_step / ofdft_dist_closure move chunk k across the fabric
                                     while chunk k + 1 is in its y pass and chunk k - 1 in its x pass.  0 (default): automatic -- 4 chunks
                                     from 8 M points per rank, 2 from 1 M, else 1 (and only when the slab extents n0 / P and n1 / P are multiples
                                     of 32, with >= 4 kz blocks per chunk); 1: off.  Every
                                     rank must use the same value; the ipc transport needs a new ofdft_ipc_export / attach round after a change. */
#define OFDFT_OPT_YBATCH 14       /* 1 (default): the y passes of the three spectra of each WGC99 half run as one launch (grid.y = 3); 0: three launches */
#define OFDFT_OPT_IPC_WAIT_MS 13  /* ipc transport: how long a delivery wait of ofdft_dist_closure stays patient before it aborts the evaluation ON ALL
                                     RANKS (default 30 000 ms: a rank may be late by a module load, a page-in, a garbage collection) */
#define OFDFT_OPT_TEST_FAULT 11   /* test hook, never set in production: 1 = the NEXT persistent-kernel launch is one workgroup short (its grid
                                     barriers time out -> the call must still return the right numbers through the staged path and switch the
                                     kernel off); 2 = the co-residency check of the persistent kernel reports "does not fit" */
#define OFDFT_OPT_BS_FUSED 15     /* chirp-z path (extents without a line-transform plan, i.e. what the reference's System.ecut2shape, system.py:74-89, gives):
                                     1 (default) = forward-x, spectral multiply and inverse-x of every convolution in ONE kernel (x extents up to 256);
                                     0 = three passes per transform and separate multiply kernels */
#define OFDFT_OPT_POT_SPECTRUM 16 /* 1 (default): one GPU, split-derivative GGA with Hartree: the Hartree potential rides in the divergence spectrum
                                     (v_H^ / -2 beside i f_a G_a^ in the divergence x pass, which also forms E_H by Parseval), and D_b G_b plus the
                                     y-inverse of that spectrum are one y pass -- the combine kernel reads one spectrum where it read three.
                                     0: the Hartree spectrum and the two divergence parts travel separately (slabs, chirp-z path and the persistent
                                     small-grid kernel always do) */
#define OFDFT_OPT_AXIS_PASSES 17  /* one GPU, z-fused pipeline: operators of one axis run as passes of that axis.  Bits (default 3):
                                     1 = split-derivative GGA: D_a n = i f_a n^ comes from an x pass on the z spectrum BEFORE its y-forward (the
                                         multiply does not depend on y), so it makes no y round trip: one y pass less on every cell;
                                     2 = cells with orthogonal axes, von Weizsaecker term: -k^2 = -(k_a^2 + k_c^2) - k_b^2, so the Laplacian of
                                         sqrt(n) is an x pass on the z spectrum plus ONE y pass that multiplies by -k_b^2 between its transforms
                                         and adds the x pass' result: two y passes and one launch less, one more spectrum of workspace.  fp64 library
                                         only: the fp32 library accepts the bit and keeps the three passes, which measured faster there.
                                     0: the sequence without either (slabs, chirp-z path, the persistent small-grid kernel and the unsplit GGA form
                                     always run that one) */
#define OFDFT_OPT_WGC_FOLD 28    /* 1 (default): on cells with orthogonal axes the cross-wave x pass reads the WGC99 table entry of x > n0 / 2 at
                                     n0 - x (|k| is even along a line there; functionals.py:968-972 depends on |k| only): both uses of an entry
                                     fall into one tile, the second is a cache hit, the pass' table traffic halves.  0: every k-point its own entry */
#define OFDFT_OPT_HVP_GGA 18      /* 0 (default): the second-derivative entries refuse pbe_x and pbe_c by name; 1: ofdft_hessian_vector and
                                     ofdft_hessian_vector_chi serve them (second transform stage, see there).  ofdft_hessian_vector_chi_multi,
                                     ofdft_potential_strain_gradient and ofdft_strain_hessian refuse them under either value.  Any other value:
                                     OFDFT_EINVAL.  Both libraries accept it; it matters in the fp64 one */
#define OFDFT_OPT_HVP_WGC 19      /* 0 (default): the second-derivative entries refuse wgc99_nl by name; 1: ofdft_hessian_vector and
                                     ofdft_hessian_vector_chi serve it (a stage of its own, see there).  ofdft_hessian_vector_chi_multi,
                                     ofdft_potential_strain_gradient and ofdft_strain_hessian refuse it under either value.  Any other value:
                                     OFDFT_EINVAL.  Both libraries accept it; it matters in the fp64 one */
#define OFDFT_OPT_XWAVE 8         /* fused x passes: 1 (default) = the cross-wave kernel (whole runs of memory-adjacent lines per access, the
                                     radix-4 / -8 step of the line transform across the waves of a workgroup) for 256- and 512-point lines
                                     and, for passes over three or more spectra, 1024-point lines; elsewhere the wave-local kernel (a line of
                                     every spectrum in the lanes of one wavefront, mixing in registers; x extents up to 512) for passes over
                                     three or more spectra and the group-parallel kernel (spectra traded through LDS) for the rest.
                                     0 = always the group-parallel kernel, 2 = the wave-local kernel for every pass, 5 = the cross-wave
                                     kernel wherever it exists (128..1024 points), 6 = ... for passes over >= 3 spectra only, 7 = the
                                     round-3 choice (no cross-wave kernel), 4 = that choice with the group-parallel kernel from 512-point
                                     lines on.  fp32 build under 1: 1024-point lines take the cross-wave kernel for every pass, 256-point
                                     lines the group-parallel one for 1 -> 1 passes; its cross-wave kernel owns two memory-adjacent lines
                                     per lane and hands a pass whose lines do not come in whole pairs on to the wave-local kernel (up to
                                     512 points) or the group-parallel one (1024).  A pass that also integrates an energy has no
                                     group-parallel kernel: where neither other family serves it the evaluation takes its plain form */
int  ofdft_set_option(ofdft_ctx* ctx, int option, double value);

/* Measurement support (bench.py): when on, every kernel launch of the energy calls is bracketed by HIP
 * events on the caller's stream and the durations are accumulated per kernel class.  Adds launch overhead:
 * never on inside a timed region. */
int  ofdft_set_profiling(ofdft_ctx* ctx, int on);
int  ofdft_profile_count(ofdft_ctx* ctx);
int  ofdft_profile_get(ofdft_ctx* ctx, int idx, char* name_buf, int buflen, double* total_ms, long long* launches);

#ifdef __cplusplus
}
#endif
#endif /* OFDFT_HIP_H */
