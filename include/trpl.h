/*
 * trpl.h -- C ABI of libtrpl_hip.so: the MI355X (gfx950) drop-in for the batched TRPL
 * drift-diffusion solve + log-likelihood hot path of HagesLab/Bayesian-Inference-TRPL.
 *
 * Every entry point is `extern "C"`, takes plain pointers and sizes, returns an int status
 * (TRPL_OK = 0) and never throws; the message for the last failure on the calling thread is
 * returned by trpl_last_error().  Each declaration cites the reference interface it
 * replaces (file:line in the reference checkout).  The Python-side binding a maintainer of
 * the reference would add is shown in INTEGRATION.md; this repo's own binding is
 * bayesian-inference-trpl_amd/_abi.py.
 *
 * Two families:
 *   host-buffer calls   (trpl_solve_pl, trpl_log10_clamp, trpl_sse_accumulate, trpl_loglik):
 *       borrow caller-owned host memory for the duration of the call, exactly like the
 *       reference's numpy-in / numpy-in-place callables; device memory is allocated, used
 *       and released inside the call (pvSimPCR.py:365-384, probs.py:53-60, :80-83).
 *   device-resident calls (`*_dev`): every pointer is a HIP device pointer on the current
 *       device and `stream` is a hipStream_t (NULL = default stream); nothing is allocated,
 *       copied or synchronised -- the caller owns residency and ordering.
 *
 * Data layout (all row-major, C-contiguous):
 *   matpar  [S][12] fp64, physical units nm / ns / V, column order
 *           N0, P0, DN, DP, rate, sr0, srL, CN, CP, tauN, tauP, Lambda   (pvSimPCR.py:97-108)
 *   X       [S][13] fp64 = matpar columns + mag_offset                  (bayeslib.py:144,:195)
 *   excitation dN [C][L] fp64, nm^-3, node n at x = (n + 1/2) dx        (pvSimPCR.py:355-356)
 *   PL      [rows][ld] fp32 or fp64 (elem_bytes 4 / 8), column t/plT    (pvSimPCR.py:281)
 */
#ifndef TRPL_H
#define TRPL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRPL_ABI_VERSION 5   /* 5 (round 6): trpl_has_experimental(); TRPL_FLAG_MIXED / TRPL_FLAG_HIST32 exist only in a library built with
                                `make EXPERIMENTAL=1` (the default library answers TRPL_ERR_UNSUPPORTED); trpl_kernel_name validates like a
                                launch; roctx ranges around the host-buffer calls when libroctx64.so is loadable; trpl_interp_rows (host);
                                TRPL_FLAG_PREDICT (an additive, opt-in flag: no existing call changes).
                                4 (round 5): TRPL_FLAG_BDF_ORDER, TRPL_FLAG_PAIR_ALWAYS_SEAM / _PAIR_ADJACENT / _MULTI_FORCE_PAD (were
                                process-wide environment switches), trpl_multi_create_ex, TRPL_PL_ENVELOPE_K_L512; floor_col = -2 for
                                flagged systems, T <= 2^30 - 16, up to TRPL_MAX_CURVES curves and TRPL_FLAG_HIST32 (round 4, then
                                still under version 3) */

/* status codes */
#define TRPL_OK 0
#define TRPL_ERR_ARG 1          /* invalid argument (message says which) */
#define TRPL_ERR_HIP 2          /* a HIP runtime call failed */
#define TRPL_ERR_NODEVICE 3     /* no usable gfx950 device */
#define TRPL_ERR_UNSUPPORTED 4  /* valid request this build has no kernel for */

/* flags for the solver entry points */
#define TRPL_FLAG_STRICT 0x1      /* bit-reproducible arithmetic: no FMA contraction, IEEE divides, the
                                     reference's operation order (state is bit-identical to the
                                     sequentially executed reference); 6.4x slower.
                                     WITHOUT it (the default, "FAST": FMA contraction, v_rcp_f64 + refinement, cyclic reduction +
                                     PCR, reordered sums) a system follows the reference's ITERATION PATH -- the same number of
                                     inner iterations at every time step -- up to knife-edge decisions of the convergence test:
                                     measured against STRICT, iteration totals are identical on every system over the bench window
                                     (T = 8000: Power_scan x 64 x 3, Twothick x 32 x 6, L = 512 x 16 x 3 -- in the -m gpu suite
                                     against the oracle, which allows one system one iteration) and differ by ONE iteration on 8 of
                                     196 608 systems (in totals of ~160 000 each) over the reference's full window T = 80 000
                                     (profiles/r4_validate_twothick_32768_T80000.txt); PL then agrees to the envelope stated at
                                     trpl_loglik below */
#define TRPL_FLAG_PL_F32 0x2      /* trpl_loglik*: round PL and log10 PL through fp32 exactly where the
                                     reference's float32 plI buffer does (bayeslib.py:137) */
#define TRPL_FLAG_NORMALIZE 0x4   /* trpl_loglik*: self-normalise each PL curve to its t = 0 value
                                     (bayeslib.py:150-154) */
#define TRPL_FLAG_FP32 0x8        /* solver state, BDF history and PCR in fp32 (node sums, PL, log10 and the
                                     squared error stay fp64); L >= 128, not combinable with STRICT; use
                                     tol_exp 3-4 (fp32's residual floor is ~1e-7).  A SCREENING mode: an fp32
                                     state cannot hold the BDF history differences, and over thousands of time
                                     steps the PL error grows to percents and, on the decayed tail, tens of
                                     percent (measured at L = 512, T = 8000: DESIGN.md section 7); use the
                                     default fp64 path at tol_exp 6 for results.  No
                                     reference exists for this mode (the reference is fp64 only).  A launch that
                                     takes more than TRPL_FP32_MAX_STEPS time steps is refused (TRPL_ERR_UNSUPPORTED)
                                     unless TRPL_FLAG_FP32_LONG is set too */
#define TRPL_FP32_MAX_STEPS 256   /* measured at L = 512 (tests/test_gpu_l512.py): PL error
                                     ~1e-3 after 60 steps, percents after 1000, 0.4 after 8000 */
#define TRPL_FLAG_FP32_LONG 0x1000 /* with TRPL_FLAG_FP32: run a window longer than TRPL_FP32_MAX_STEPS anyway -- the
                                     caller has read the paragraph above and wants the screening pass */

/* The next two flags name EXPERIMENTAL steppers -- measured, not faster, never selected by default.  They
 * are compiled only into a library built with `make EXPERIMENTAL=1` (libtrpl_hip_exp.so; trpl_has_experimental() == 1); the
 * default library refuses them with TRPL_ERR_UNSUPPORTED and a message that says so.  The bits and TRPL_KERNEL_MIXED / _HIST32
 * keep their values in both builds. */
#define TRPL_FLAG_MIXED 0x40      /* fp64 state, history, assembly, residuals, PL and likelihood; each inner iteration
                                     solves its tridiagonal CORRECTION equation A delta = b - A c in fp32 (L >= 128, not
                                     combinable with STRICT / FP32).  Same convergence test as fp64 (the fp64 residual of
                                     the reference's norm2), so the accuracy is that of the fp64 solver at the same tol;
                                     an fp32 solve resolves ~1e-5 of a correction, so tol_exp 5-6 converges in the fp64
                                     iteration count (measured: tol_exp 7 too).  Measured on MI355X it is NOT faster than
                                     the fp64 stepper (a plain fp32 VALU instruction only issues faster than an fp64 one
                                     with two or more wavefronts per SIMD, tools/ubench_f32_f64.hip; the L = 512 stepper
                                     holds one); it exists as the measured point of DESIGN.md section 7.  No reference exists for it */
#define TRPL_FLAG_HIST32 0x2000    /* fp64 state, assembly, solves, residuals, PL and likelihood; the BDF history kept in
                                     difference form with the older differences stored in fp32 (every row of the BDF table,
                                     pvSimPCR.py:241-250, sums to zero: only the newest level is needed in full).  One-system
                                     stepper at L = 256 / 512; no snapshots, resume or bundles; not combinable with STRICT /
                                     FP32 / MIXED.  An experiment of round 4: the oracle's iteration
                                     totals and PL within 1.4e-9 over 8000 steps at L = 512, but no occupancy gain (-5 %;
                                     +1.6 % in the best build variant) -- never selected by default.  No reference exists
                                     for it */
#define TRPL_FLAG_SNAP_RAW 0x80   /* trpl_solve_pl_snap / _resume: snapshots in SOLVER units (no division by dx^3 / dx), the
                                     form trpl_solve_pl_resume reads back bit for bit */
#define TRPL_FLAG_BUNDLE(m) ((uint32_t)(((m) - 1) & 0xF) << 8)
                                  /* the reference's max_sims_per_block = m (pvSimPCR.py:211-216,:258-266;
                                     bayes_validate.connect_to_gpu defaults to 3).  The reference takes what its 48 KB of
                                     shared memory hold (pvSimPCR.py:113-125: 3 systems at L = 128, 6 at L = 64, 13 at
                                     L = 32); here m <= 16 for L <= 64 and m <= 4 from L = 128 on (one wavefront per system,
                                     one workgroup per bundle; a larger m is TRPL_ERR_ARG).
                                     The samples p .. p+m-1 (p a multiple of m, counted inside the call's batch)
                                     iterate in lockstep until the LARGEST residual of the bundle is below tolerance;
                                     iteration counts and status are the bundle's.  With TRPL_FLAG_STRICT bit-identical to
                                     the reference run that way (tests/golden/pvsim_bundle.npz), any L; without it the
                                     one-system fp64 stepper, L <= 128, to rounding (1e-9).  Not with _FP32 / _MIXED /
                                     _KERNEL_PAIR, and not in the trpl_loglik_multi* calls (a sharded batch would depend on
                                     where it is cut).  m = 1 (no bits set): every sample converges on its own */
#define TRPL_FLAG_BDF_ORDER(k) ((uint32_t)((k) & 0x7) << 14)
                                  /* cap the order of the BDF ramp (pvSimPCR.py:241-250: order min(t + 1, 5) at step t) at
                                     k = 1 .. 5: step t takes the coefficient row of step min(t, k - 1).  No bits set (k = 0): the
                                     reference's ramp.  k = 2 is the time discretisation of the reference's older solver
                                     Legacy/pvSim.py:94-97 (Euler at t = 0, BDF2 ever after), which with CN = CP = 0 makes that
                                     file a WHOLE-CURVE parity reference for every stepper here (tests/golden/legacy_full.npz);
                                     k = 1 is implicit Euler.  Every arithmetic mode and kernel; k > 5 is TRPL_ERR_ARG.  A
                                     wave-uniform select of the coefficient row outside the iterations: no cost when off */
#define TRPL_FLAG_PAIR_ALWAYS_SEAM 0x20000  /* test / measurement: the two-systems-per-wavefront stepper clears every value that
                                     crosses the seam between its two systems in EVERY iteration (the form rounds 1-3 shipped)
                                     instead of only when a time step is repeated ("optimistic seam", round 4).  Results are
                                     bit-identical either way -- this is the reference side of the differential tests on hostile
                                     inputs; ~1.6 % slower.  Ignored by the other kernels */
#define TRPL_FLAG_PAIR_ADJACENT 0x40000     /* measurement: the two-systems-per-wavefront stepper pairs adjacent samples of one curve
                                     (the round-2 rule) instead of two curves of one sample (trpl_pair_table); a scheduling
                                     matter only, results are bit-identical either way */
#define TRPL_FLAG_MULTI_FORCE_PAD 0x80000   /* trpl_loglik_multi_dev, tests: take the padded all-gather + unpadding pass even when
                                     the shards are equal */
#define TRPL_FLAG_PREDICT 0x100000  /* opt-in, OFF by default: each time step's Newton/Picard iteration starts from an
                                     extrapolation of the history instead of U^t (pvSimPCR.py:130-132) -- 3 U^t - 3 U^{t-1} + U^{t-2}
                                     from global step 2 on, 2 U^t - U^{t-1} at step 1, U^t at step 0, for N, P and E.  Nothing else
                                     changes: the BDF right-hand sides are formed from U^t, U^t enters the history, assembly, both
                                     residual tests, both solves, the field update, the break rule and the iters >= MAX flagging are
                                     the default path's.  The first test of a step then usually passes: 1.01 - 1.13 inner
                                     iterations per step instead of 2.01 - 2.25, 1.63 - 1.71 x the system-timesteps/s on
                                     every measured configuration, L = 512 included.  A resumed launch
                                     continues the same sequence (t is the global step), snapshots / resume, FAST and STRICT, every
                                     L and both FAST kernels accept it (their own instantiations, trpl::predict::...).
                                     Tolerance: each step is still solved to the caller's tol, by a different route, so results are
                                     NOT the default path's bits.  Above TRPL_PL_FLOOR_EXCESS, PL is within 5e-5 relative of
                                     the default path for windows of up to 8000 steps and within 3e-4 up to 80 000 steps, with
                                     the same flagged systems (medians ~1e-9; maxima measured on 256-sample subsets of the four
                                     configurations of tools/bench_predict.py: 2.8e-6 .. 2.1e-5 at T = 8000, 1.7e-4 at
                                     T = 80 000).  The gap is NOT a floor effect: near the floor (r = PL / (B L n0p0) < 1) the
                                     paths agree within 2e-8 at T = 8000.  It is the default path's own tol-sized drift in
                                     strongly excited, slowly decaying systems (r ~ 1e5 .. 1e6), growing ~2.5e-9 per step at the
                                     worst point: there the default path is 2.4e-6 (T = 8000) / 1.7e-4 (T = 80 000) away from a
                                     tol-11 solution and predict 4.6e-7 / 6.8e-6.  Predict is never farther from the tol-11
                                     solution than the default path (max over a batch; measured 0.16 - 0.21 of its distance).
                                     The extra 60 B of scratch per lane of trpl::predict::pair::stepper_pair_kernel<true, true,
                                     true> (snapshots + optimistic seam; the default counterpart uses 36 B) is the only resource
                                     difference from the default kernels; the timed, snapshot-free kernels use none.
                                     Refused: with TRPL_FLAG_FP32, _MIXED or _HIST32 TRPL_ERR_ARG; with TRPL_FLAG_BUNDLE(m > 1)
                                     TRPL_ERR_UNSUPPORTED.  Python: predict=True, gpu_info["predict"] */
#define TRPL_FLAG_MOMENTS 0x200000  /* the likelihood-mode steppers whose sink emits esum = sum e_i beside sse = sum e_i^2 (their own
                                     instantiations, trpl::moments::[predict::][pair::]stepper...; the existing kernels are the same
                                     machine code as without them).  SET BY trpl_loglik_moments[_dev] THEMSELVES: every other entry
                                     point has nowhere to put esum and answers TRPL_ERR_ARG before it touches a device.
                                     trpl_kernel_name / trpl_kernel_variant accept it and name the instantiation after the usual
                                     launch checks.  FAST and STRICT, every L, both FAST kernels, with and without
                                     TRPL_FLAG_PREDICT; no snapshot / resume forms.  Refused with TRPL_ERR_UNSUPPORTED:
                                     TRPL_FLAG_FP32, _MIXED, _HIST32, TRPL_FLAG_BUNDLE(m > 1) */
#define TRPL_FLAG_WEIGHTED 0x400000 /* the moments steppers whose sink multiplies every term by its observation's weight: sse = sum w_i e_i^2,
                                     esum = sum w_i e_i (their own instantiations, trpl::weighted::[predict::][pair::]stepper...; the
                                     existing kernels are the same machine code as without them).  SET BY trpl_loglik_weighted[_dev]
                                     THEMSELVES: every other entry point takes no weights and answers TRPL_ERR_ARG before it touches
                                     a device.  With TRPL_FLAG_MOMENTS: TRPL_ERR_ARG (the weighted sink already emits both sums).
                                     trpl_kernel_name / trpl_kernel_variant accept it and name the instantiation after the usual
                                     launch checks.  FAST and STRICT, every L, both FAST kernels, with and without
                                     TRPL_FLAG_PREDICT; no snapshot / resume forms.  Refused with TRPL_ERR_UNSUPPORTED:
                                     TRPL_FLAG_FP32, _MIXED, _HIST32, TRPL_FLAG_BUNDLE(m > 1).  Python: loglik(weights=),
                                     gpu_info["weighted"] */
#define TRPL_FLAG_CUT 0x800000      /* the FAST likelihood-mode steppers whose sink stops a system as soon as its running sse is above
                                     the caller's sse_cut (their own instantiations, trpl::cut::[predict::][pair::]stepper...; the
                                     existing kernels are the same machine code as without them).  SET BY trpl_loglik_cut[_levels][_dev]
                                     THEMSELVES: every other entry point has no sse_cut and answers TRPL_ERR_ARG before it touches
                                     a device.  trpl_kernel_name / trpl_kernel_variant accept it and name the instantiation after
                                     the usual launch checks.  FAST only, every L, both FAST kernels, with and without
                                     TRPL_FLAG_PREDICT; no snapshot / resume / multi forms.  With TRPL_FLAG_MOMENTS or _WEIGHTED:
                                     TRPL_ERR_ARG.  Refused with TRPL_ERR_UNSUPPORTED: TRPL_FLAG_STRICT, _FP32, _MIXED, _HIST32,
                                     TRPL_FLAG_BUNDLE(m > 1).  Python: loglik(sse_cut=), gpu_info["cut_margin"] */
#define TRPL_FLAG_KERNEL_PAIR 0x10    /* run the two-systems-per-wavefront stepper whatever the launch size (L = 128,
                                        fp64, not STRICT -- anything else is TRPL_ERR_ARG) */
#define TRPL_FLAG_KERNEL_SINGLE 0x20  /* run the one-system-per-wavefront stepper whatever the launch size */
/* Without either bit the library picks by launch size (below).  The two FAST kernels agree to rounding
 * (~1e-12 relative on a likelihood: their tridiagonal eliminations and node sums are ordered differently),
 * not bit for bit, so a caller that cuts ONE logical batch into several launches -- sample shards over
 * devices or ranks, blocks of a larger run -- and wants every sample's bits to be independent of the cut
 * pins the variant of the whole batch: flags |= the bit trpl_kernel_variant(total systems, ...) names.
 * trpl_loglik_multi and trpl_loglik_multi_dev do this themselves. */

/* which time-stepper kernel a launch of nsys = S * C systems on L nodes taking `steps` time steps (T, or up
 * to the last observation in likelihood mode) with these flags runs on the current device */
#define TRPL_KERNEL_FAST 0        /* one system per wavefront */
#define TRPL_KERNEL_FAST_PAIR 1   /* two systems per wavefront: L = 128, launches that keep the chip full */
#define TRPL_KERNEL_STRICT 2
#define TRPL_KERNEL_FP32 3
#define TRPL_KERNEL_MIXED 4
#define TRPL_KERNEL_HIST32 5
int trpl_kernel_variant(int64_t nsys, int32_t L, int64_t steps, uint32_t flags);
/* The C++ name (namespace, template arguments; no return type, no parameter list) of the time-stepper kernel such a launch runs
 * -- the name rocprofv3's kernel trace lists it under, after "void " -- written to buf as a NUL-terminated string.  snapshots
 * != 0: a launch with state snapshots or a resume (their own instantiation).  bench.py names its `roofline.rocprof_name` with
 * it instead of guessing the instantiation.  Runs the flag / shape checks of a launch first: a combination a launch would
 * refuse (TRPL_FLAG_KERNEL_PAIR with _STRICT, _HIST32 at L = 128 or with snapshots, _FP32 over more than TRPL_FP32_MAX_STEPS
 * steps without _FP32_LONG, a bundle the grid cannot hold, a flag of the experimental build in the default library ...) returns
 * the launch's error code and message and an empty string -- never the name of an instantiation that does not exist. */
int trpl_kernel_name(int64_t nsys, int32_t L, int64_t steps, uint32_t flags, int32_t snapshots, char *buf, int64_t buflen);

/* Who shares a wavefront in the two-systems-per-wavefront stepper of a fused on-grid likelihood launch (a scheduling
 * matter only: a system's bits do not depend on its partner).  Curves with the same thickness and observation count
 * form a group; inside a group consecutive curves -- neighbouring excitation powers in the reference's files -- are
 * paired for each of the two samples of a period (samples 2p, 2p + 1), and the first curve of a group of odd size pairs
 * with itself across the two samples: two curves of ONE sample need similar iteration counts step by step, adjacent
 * samples of one curve do not.  Fills cA/oA/cB/oB [C]: block k of a period runs the systems (curve
 * cA[k], sample 2p + oA[k]) and (cB[k], 2p + oB[k]); returns the number of entries (C; 0 when the table is not used: one
 * curve), or -TRPL_ERR_* on a bad argument.  Host only, no device needed. */
int trpl_pair_table(const double *lengths_nm, const int64_t *n_obs, int32_t C, int32_t L, int64_t T, double time_ns,
                    int32_t *cA, int32_t *oA, int32_t *cB, int32_t *oB);

int trpl_abi_version(void);
/* 1 when this library contains the experimental steppers (TRPL_FLAG_MIXED, TRPL_FLAG_HIST32: `make EXPERIMENTAL=1`), else 0 */
int trpl_has_experimental(void);
const char *trpl_last_error(void);
/* number of visible HIP devices (0 with none); never fails */
int trpl_device_count(void);

/* ---------------------------------------------------------------------------------------
 * trpl_solve_pl -- replaces pvSimPCR.pvSim(plI, plN, plP, plE, matPar, simPar, iniPar, TPB,
 * BPG, max_sims_per_block, init_mode="points")  (pvSimPCR.py:309-401; kernel tEvol :227-306,
 * iterate :93-225, pcreduce :42-81, norm2 :14-40).
 *
 * Time-steps S independent systems (one curve) for t = 0..T with the reference's
 * variable-order BDF / Newton-Picard / PCR scheme and writes PL(t) = B dx sum_i (N_i P_i -
 * n0 p0) for t % plT == 0 into plI[s][t/plT] in the buffer's dtype, re-dimensionalised
 * (pvSimPCR.py:393).
 *   status[s]      0, or 1+t when iterate() reached max_iter at step t (pvSimPCR.py:269);
 *                  that system stops there and its remaining PL entries are NaN (the
 *                  reference leaves them uninitialised and stops the whole launch).
 *   iters_total[s] (nullable) inner iterations summed over the steps taken.
 *   seconds        (nullable) device time of the solve, like pvSim's return value (pvSimPCR.py:378-381); defined once for
 *                  all host-buffer calls at trpl_posterior_weights below.
 * L must be a power of two, 4 <= L <= 512.
 * ------------------------------------------------------------------------------------- */
int trpl_solve_pl(const double *matpar, int64_t S, double length_nm, double time_ns, int32_t L,
                  int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN,
                  void *plI, int32_t pl_elem_bytes, int64_t pl_ld, int32_t *status,
                  int64_t *iters_total, uint32_t flags, int32_t device, double *seconds);

int trpl_solve_pl_dev(const double *matpar, int64_t S, double length_nm, double time_ns,
                      int32_t L, int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter,
                      const double *dN, void *plI, int32_t pl_elem_bytes, int64_t pl_ld,
                      int32_t *status, int64_t *iters_total, uint32_t flags, void *stream);

/* ---------------------------------------------------------------------------------------
 * trpl_solve_pl_snap -- trpl_solve_pl that also fills pvSim's debug outputs plN, plP, plE
 * (pvSimPCR.py:309 arguments 2-4; recording hook :283-288, disabled in that file; the working form is
 * Legacy/pvSim.py:121-126 with the re-dimensionalisation of :169-171; consumer Testing/compare.py:22-31):
 * the carrier densities on the L nodes and the field on the L + 1 edges of the state at the time steps
 * snap_steps[i] -- the state PL(t) is computed from -- in nm^-3 and nm^-1.
 *   snap_steps [n_snap] HOST int64 time-step indices (the reference's pT after bayeslib.py:123),
 *              n_snap <= 16, any order.  Like Legacy's `pT.index(t)`, a step listed twice fills its
 *              first slot only; a step outside [0, T] is never reached.  Slots that are not filled keep
 *              the caller's contents.
 *   plN, plP   [S][n_snap][L] fp64 (each nullable);  plE [S][n_snap][L+1] fp64 (nullable), E_0 = E_L = 0.
 * A system flagged at step t (status = 1 + t) gets NaN in the slots of steps >= t, like its PL.
 * Not available with TRPL_FLAG_FP32 (TRPL_ERR_UNSUPPORTED).
 * ------------------------------------------------------------------------------------- */
int trpl_solve_pl_snap(const double *matpar, int64_t S, double length_nm, double time_ns, int32_t L,
                       int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN,
                       void *plI, int32_t pl_elem_bytes, int64_t pl_ld, int32_t *status,
                       int64_t *iters_total, const int64_t *snap_steps, int32_t n_snap, double *plN,
                       double *plP, double *plE, uint32_t flags, int32_t device, double *seconds);
int trpl_solve_pl_snap_dev(const double *matpar, int64_t S, double length_nm, double time_ns, int32_t L,
                           int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN,
                           void *plI, int32_t pl_elem_bytes, int64_t pl_ld, int32_t *status,
                           int64_t *iters_total, const int64_t *snap_steps /*host*/, int32_t n_snap,
                           double *plN, double *plP, double *plE, uint32_t flags, void *stream);

/* ---------------------------------------------------------------------------------------
 * trpl_solve_pl_resume -- pvSim's init_mode = "continue" (pvSimPCR.py:357-358), which is only a stub in the
 * reference (`pass`: dN is undefined and the call raises; the commented block :294-306 shows the intent: keep the
 * last time levels in plN / plP / plE and start the next call from them).  Here: the time loop starts at step
 * t0 >= 4 (dN is not an argument: the state comes from the checkpoint) from the five newest BDF levels U^{t0-4} .. U^{t0} of every system,
 *   resN, resP [S][5][L], resE [S][5][L+1] fp64 in SOLVER units, level m <-> step t0 - 4 + m,
 * exactly what trpl_solve_pl_snap[_dev] stores for snap_steps = {t0-4, .., t0} under TRPL_FLAG_SNAP_RAW.
 * A run of T steps and a run to t0 followed by a resume to T give the same PL columns, snapshots and status
 * BIT FOR BIT, in every arithmetic mode (tested): a long window can be cut into segments, checkpointed and
 * continued.  That includes a system that was flagged BEFORE t0: the snapshot slots of a flagged system hold a
 * quiet NaN whose low 31 payload bits are its status word (1 + failing step), the resume finds it in the newest
 * level, reports that status, takes no step (iters_total 0 for this call) and fills PL columns >= the failing
 * step and later snapshots with NaN, as the uninterrupted run does.  Iteration totals add up once the step at t0 is counted once: the time loop runs t = 0 .. T
 * inclusive (pvSimPCR.py:237, the step taken at t = T is computed and dropped), so the run to t0 has taken the
 * step that the resume takes again (a resume with T = t0 counts exactly that step).  PL columns before t0 / plT are not written (the caller's buffer keeps
 * them); snapshot steps before t0 are ignored; iters_total counts the steps taken by this call.
 * Not available with TRPL_FLAG_FP32.
 * ------------------------------------------------------------------------------------- */
int trpl_solve_pl_resume(const double *matpar, int64_t S, double length_nm, double time_ns, int32_t L,
                         int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter, int64_t t0,
                         const double *resN, const double *resP, const double *resE, void *plI,
                         int32_t pl_elem_bytes, int64_t pl_ld, int32_t *status, int64_t *iters_total,
                         const int64_t *snap_steps, int32_t n_snap, double *plN, double *plP, double *plE,
                         uint32_t flags, int32_t device, double *seconds);
int trpl_solve_pl_resume_dev(const double *matpar, int64_t S, double length_nm, double time_ns, int32_t L,
                             int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter, int64_t t0,
                             const double *resN, const double *resP, const double *resE, void *plI,
                             int32_t pl_elem_bytes, int64_t pl_ld, int32_t *status, int64_t *iters_total,
                             const int64_t *snap_steps /*host*/, int32_t n_snap, double *plN, double *plP,
                             double *plE, uint32_t flags, void *stream);

/* ---------------------------------------------------------------------------------------
 * trpl_log10_clamp -- replaces probs.fastlog(plI, MIN, TPB, BPG)  (probs.py:64-85):
 * x <- log10(max(x, min)) in place, in the buffer's dtype.
 * ------------------------------------------------------------------------------------- */
int trpl_log10_clamp(void *x, int32_t elem_bytes, int64_t rows, int64_t cols, int64_t ld,
                     double min, int32_t device, double *seconds);
int trpl_log10_clamp_dev(void *x, int32_t elem_bytes, int64_t rows, int64_t cols, int64_t ld,
                         double min, void *stream);

/* ---------------------------------------------------------------------------------------
 * trpl_sse_accumulate -- replaces probs.prob(P, plI, values, uncertainty, mag_grid, TPB, BPG)
 * (probs.py:20-62):  P[j] -= sum_i (plI[j][i] + mag[j] - values[i])^2, fp64 accumulation in
 * index order.  `uncertainty` is not part of THIS call because the reference never reads it
 * (probs.py:40, commented out).
 * trpl_sse_accumulate_w -- the same with that line restored:
 *     P[j] -= sum_i ((plI[j][i] + mag[j] - values[i])^2 * w[i]),     w [n_obs] fp64, w[i] = 1 / (2 uncertainty[i]^2)
 * formed ONCE by the caller (Python: likelihood.weights_from_uncertainty; the uncertainty column in log10 units,
 * bayes_io.py:75-76), fp64, index order, each term ((e * e) * w).  This is a multiplication by the rounded reciprocal,
 * not the reference's division err / (2 u^2): the two differ by <= 1 ulp per term.  The host form checks the weights
 * (finite, >= 0; TRPL_ERR_ARG naming the index); the _dev form cannot look.
 * ------------------------------------------------------------------------------------- */
int trpl_sse_accumulate(double *P, const void *plI, int32_t elem_bytes, int64_t rows,
                        int64_t n_obs, int64_t ld, const double *values, const double *mag,
                        int32_t device, double *seconds);
int trpl_sse_accumulate_dev(double *P, const void *plI, int32_t elem_bytes, int64_t rows,
                            int64_t n_obs, int64_t ld, const double *values, const double *mag,
                            void *stream);
int trpl_sse_accumulate_w(double *P, const void *plI, int32_t elem_bytes, int64_t rows,
                          int64_t n_obs, int64_t ld, const double *values, const double *wts,
                          const double *mag, int32_t device, double *seconds);
int trpl_sse_accumulate_w_dev(double *P, const void *plI, int32_t elem_bytes, int64_t rows,
                              int64_t n_obs, int64_t ld, const double *values, const double *wts,
                              const double *mag, void *stream);

/* ---------------------------------------------------------------------------------------
 * trpl_interp_rows -- the time interpolation of the UNFUSED call sequence, bayeslib.py:184-191 (a Python loop of
 * scipy.interpolate.griddata over the rows of plI): every row of the host matrix pl [rows][ld] (fp32 / fp64, elem_bytes), of which
 * ncol columns are valid, is interpolated linearly onto n_obs observation times given as brackets -- hi[i] in [1, ncol - 1] the
 * column right of time i, dx[i] = t_i - t[hi[i] - 1], h[i] = t[hi[i]] - t[hi[i] - 1] (trpl_loglik_obs's convention) -- into
 * out [rows][out_ld] fp64:  out = ((pl[hi] - pl[hi - 1]) / h) * dx + pl[hi - 1], the difference in pl's own type, the rest in fp64,
 * no fused multiply-add: scipy's interp1d form, bit for bit.  PLAIN HOST CODE (no device, no stream; callable from several threads
 * at once): it exists so that the worker threads of an unfused driver do not serialise on an interpreter lock; the fused entry
 * points interpolate in the kernel.
 * ------------------------------------------------------------------------------------- */
int trpl_interp_rows(const void *pl, int32_t elem_bytes, int64_t rows, int64_t ncol, int64_t ld, const int32_t *hi,
                     const double *dx, const double *h, int64_t n_obs, double *out, int64_t out_ld);

/* ---------------------------------------------------------------------------------------
 * trpl_loglik_from_pl_dev -- log-likelihood of PL rows that are ALREADY in device memory (the output of
 * trpl_solve_pl_dev) against one observation set, in one pass: replaces, for one experiment,
 * bayeslib.simulate's normalise / fastlog / griddata / prob sequence (bayeslib.py:150-157, :173-201) on a
 * resident PL block, so that one solve serves every experiment (the reference's loop order
 * curves -> blocks -> experiments, bayeslib.py:117-171) without the PL matrix crossing PCIe.
 *   plI [rows][ld] fp32/fp64 PL as written by trpl_solve_pl_dev (ncol = T/plT + 1 valid columns)
 *   obs [n_obs] log10 observations; obs_hi/obs_dx/obs_h all NULL: observation i sits on grid column i;
 *   all non-NULL: off-grid times bracketed like trpl_loglik_obs (obs_hi in [1, ncol-1], plT = 1)
 *   mag [rows] log offsets (X[:, 12]);  P [rows] (nullable): P[j] -= sse_j;  sse [rows] (nullable) out
 *   status [rows] (nullable) as written by trpl_solve_pl_dev: a flagged system scores +inf, like trpl_loglik
 *   flags: TRPL_FLAG_PL_F32 (implied by a 4-byte buffer), TRPL_FLAG_NORMALIZE
 * The squared errors are summed by a wave reduction (trpl_log10_clamp + trpl_sse_accumulate stay the pair
 * that is bit-identical to probs.prob's serial sum).  Device pointers only; nothing is allocated.
 * ------------------------------------------------------------------------------------- */
int trpl_loglik_from_pl_dev(const void *plI, int32_t elem_bytes, int64_t rows, int64_t ncol, int64_t ld,
                            const double *obs, const int32_t *obs_hi, const double *obs_dx,
                            const double *obs_h, int64_t n_obs, const double *mag, const int32_t *status,
                            double *P, double *sse, uint32_t flags, void *stream);

/* ---------------------------------------------------------------------------------------
 * trpl_loglik -- the fused path: replaces the body of bayeslib.simulate (bayeslib.py:117-201)
 * for one experiment whose observation times are the first n_obs[c] points of the simulation
 * grid: for every sample s and curve c it time-steps the system, and accumulates
 *     sse[c][s] = sum_{i < n_obs[c]} ( log10(max(PL_{s,c}(t_i), DBL_MIN)) + X[s][12] - obs[c][i] )^2
 * without ever materialising PL in memory; then P[s] -= sse[0][s] + ... + sse[C-1][s] in
 * curve order (probs.py:44,:60).  A system that does not converge gets sse = +inf.
 *   lengths [C] host doubles (per-curve thickness, bayeslib.py:109-119)
 *   dN      [C][L], obs [C][obs_ld] log10 observations, n_obs [C] host int64 (<= T/plT + 1)
 *   sse     [C][S] out;  status [C][S] out (nullable);  iters_total [C][S] out (nullable)
 *   floor_col [C][S] out (nullable): the CANCELLATION FLOOR indicator.  PL = B (sum_i N_i P_i - L n0 p0) is a
 *           difference of nearly equal numbers once the excess carriers have decayed.  With
 *               r(t) = PL(t) / (B L n0 p0)        (mean excess product per node over the equilibrium product)
 *           this library's default arithmetic and the reference's order of operations (TRPL_FLAG_STRICT, the
 *           sequentially executed reference bit for bit) agree to
 *               |dPL / PL|  <=  1e-9 + K / r(t),    K = TRPL_PL_ENVELOPE_K_THICK = 5e-13 on the 2000 nm films at L = 128,
 *                                                   K = TRPL_PL_ENVELOPE_K_THIN  = 1e-11 on the 311 nm films at L = 128,
 *                                                   K = TRPL_PL_ENVELOPE_K_L512  = 2e-12 on the 2000 nm film at L = 512
 *           (K grows with the stencil's stiffness D dt / dx^2 -- the three grids have dx = 15.6, 2.43 and 3.9 nm; measured
 *           2e-13 / 3.7e-12 / < 2e-12 with the r-independent part at 5.5e-12 for L = 512; the -m gpu tests assert exactly
 *           these constants: tests/gpu_common.py, tests/test_gpu_l512.py, and tests/test_abi.py that header, binding and
 *           tests agree).
 *           floor_col[c][s] = first compared PL column (observation index; the grid step with off-grid observations)
 *           with r < TRPL_PL_FLOOR_EXCESS = 1e-4 or a non-positive / NaN PL; -1 if there is none; -2 for a system
 *           flagged as non-converged (status != 0: sse = +inf, nothing to compare).
 *           CONTRACT: a system with floor_col = -1 has sse within 1e-8 (relative) of the reference evaluation's; every
 *           system whose sse differs by more than 1e-6 has floor_col >= 0, and from that column on its PL depends on
 *           the evaluation order at the level above -- compare such systems across implementations on the columns
 *           before floor_col, or not at all (their posterior weight is 0).  Measurements: DESIGN.md section 2.
 * Any number of curves up to TRPL_MAX_CURVES (bayeslib.py:117 loops over them all): more than 16 run as consecutive launches of
 * up to 16 curves on the same stream; a system's bits do not depend on that grouping.
 * ------------------------------------------------------------------------------------- */
#define TRPL_PL_FLOOR_EXCESS 1e-4
#define TRPL_PL_ENVELOPE_K_THICK 5e-13
#define TRPL_PL_ENVELOPE_K_THIN 1e-11
#define TRPL_PL_ENVELOPE_K_L512 2e-12
#define TRPL_MAX_CURVES 1024
int trpl_loglik(const double *X, int64_t S, int32_t C, const double *lengths_nm, double time_ns,
                int32_t L, int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter,
                const double *dN, const double *obs, int64_t obs_ld, const int64_t *n_obs,
                double *P, double *sse, int32_t *status, int64_t *iters_total, int32_t *floor_col,
                uint32_t flags, int32_t device, double *seconds);

int trpl_loglik_dev(const double *X, int64_t S, int32_t C, const double *lengths_nm /*host*/,
                    double time_ns, int32_t L, int64_t T, int32_t plT, int32_t tol_exp,
                    int32_t max_iter, const double *dN, const double *obs, int64_t obs_ld,
                    const int64_t *n_obs /*host*/, double *P, double *sse, int32_t *status,
                    int64_t *iters_total, int32_t *floor_col, uint32_t flags, void *stream);

/* ---------------------------------------------------------------------------------------
 * trpl_loglik_obs -- trpl_loglik for observation times that do NOT lie on the simulation grid:
 * replaces the per-row time interpolation of bayeslib.simulate (scipy griddata, 1-D linear,
 * bayeslib.py:184-191) followed by probs.prob, fused into the time-stepper.  For observation i of
 * curve c (sorted by time, 0 <= t_i <= time_ns) the host passes the bracketing it would hand to
 * interp1d:  obs_hi[c][i] in [1, T] = index of the upper grid point, obs_dx = t_i - t_lo,
 * obs_h = t_hi - t_lo; the kernel forms ((y_hi - y_lo) / h) * dx + y_lo from log10 PL at the two
 * grid points (difference in fp32 under TRPL_FLAG_PL_F32, like interp1d on the reference's
 * float32 buffer) as soon as step hi has been taken.  plT is 1 on this path.
 * ------------------------------------------------------------------------------------- */
int trpl_loglik_obs(const double *X, int64_t S, int32_t C, const double *lengths_nm, double time_ns,
                    int32_t L, int64_t T, int32_t tol_exp, int32_t max_iter, const double *dN,
                    const double *obs, const int32_t *obs_hi, const double *obs_dx, const double *obs_h,
                    int64_t obs_ld, const int64_t *n_obs, double *P, double *sse, int32_t *status,
                    int64_t *iters_total, int32_t *floor_col, uint32_t flags, int32_t device, double *seconds);

int trpl_loglik_obs_dev(const double *X, int64_t S, int32_t C, const double *lengths_nm /*host*/,
                        double time_ns, int32_t L, int64_t T, int32_t tol_exp, int32_t max_iter,
                        const double *dN, const double *obs, const int32_t *obs_hi, const double *obs_dx,
                        const double *obs_h, int64_t obs_ld, const int64_t *n_obs /*host*/, double *P,
                        double *sse, int32_t *status, int64_t *iters_total, int32_t *floor_col, uint32_t flags,
                        void *stream);

/* ---------------------------------------------------------------------------------------
 * trpl_loglik_moments -- trpl_loglik / trpl_loglik_obs that also return the FIRST moment of the log-errors, so that the
 * likelihood at ANY magnitude offset follows from ONE solve.  Restores what the reference's older likelihood did,
 * probs.lnP (probs.py:5-18): its loop over a `mag_grid` fills P[:, m] for every offset from one simulated curve (the
 * argument of probs.prob, probs.py:20, is still called mag_grid), where the live path compares at the one offset of
 * X[:, 12] (probs.py:33, bayeslib.py:195) and every other trial offset costs a full solve.  With
 *     e_i = log10 PL_i + X[s][12] - obs_i,      sum_i (e_i + d)^2 = sum e_i^2 + 2 d sum e_i + n d^2,
 * so beside sse[c][s] = sum e_i^2 the steppers emit
 *     esum[c][s] = sum_i e_i      -- the very values that are squared: after the optional fp32 rounding, normalisation,
 *                                    the clamp at DBL_MIN, the interpolation and + X[s][12]; summed in sse's order and
 *                                    association (serially under TRPL_FLAG_STRICT; FAST: a wave reduction per 64 columns,
 *                                    the batches added in order).
 * Arguments: those of trpl_loglik_obs[_dev] plus plT and esum [C][S]; obs_hi / obs_dx / obs_h all NULL: observations on
 * the grid (as trpl_loglik, n_obs <= T/plT + 1), all non-NULL: off-grid (plT must be 1).  P, sse, status, iters_total
 * and floor_col are EXACTLY trpl_loglik[_obs]'s on the same inputs and flags, bit for bit (P[s] -= sum_c sse[c][s]); a
 * flagged system has esum = NaN (its sse stays +inf).  TRPL_FLAG_MOMENTS is set by the call.
 * trpl_loglik_multi* has no moments form (out of scope: the sharded drivers keep the one-offset likelihood).
 *
 * trpl_mag_grid -- the mag_grid loop of probs.lnP (probs.py:5-18) from the moments:
 *     P[m][s] -= sum_c max(sse[c][s] + 2 d_m esum[c][s] + n_c d_m^2, 0)
 * evaluated as written -- ((sse + (2 d) esum) + n (d d)), curves in order, no fused multiply-add -- for the offsets
 * d_m = offsets[m] ADDED to X[s][12].  A +inf / NaN moment gives P = -inf.
 * trpl_mag_profile -- the offset that maximises the likelihood and the likelihood there (the profile likelihood):
 *     default (one offset shared by a sample's curves): best[s] = -(sum_c esum[c][s]) / (sum_c n_c)
 *     TRPL_MAG_PER_CURVE:                               best[c][s] = -esum[c][s] / n_c
 *     P[s] -= the grid expression at best;  a flagged system: best = NaN, P = -inf.
 * ERROR BOUND (A(d) = sse + 2 |d esum| + n d^2, eps = 2^-52): against a direct evaluation of sum (e_i + d)^2 on the same PL,
 *     |P_grid - P_direct| <= k eps (A(d) + |d| sum|e_i|),   k = 6 + ceil(n / 64) + 4
 * (the depth of a batch's reduction tree, the batches added serially, the polynomial; k = n + 4 under TRPL_FLAG_STRICT).
 * The clamp at 0 only acts where cancellation has taken the sum below its own rounding error.  lnP's bval_cutoff clamp
 * depends on the offset and is not reproduced (the live reference has it commented out); no sigma weighting in
 * these calls -- trpl_loglik_weighted, trpl_mag_grid_w and trpl_mag_profile_w below are the weighted forms.
 *   sse, esum [C][S];  n_obs [C] HOST int64;  offsets [M] HOST fp64;  P [M][S];  best [S] or [C][S];  C <= TRPL_MAG_MAX_CURVES
 * The host forms are PLAIN HOST CODE (no device, like trpl_interp_rows) in the same operation order; the _dev kernels
 * (device pointers sse / esum / P / best, nothing allocated) equal them bit for bit.
 * trpl_loglik_moments_from_pl_dev -- trpl_loglik_from_pl_dev with an esum [rows] output (nullable), for a resident PL block
 * that serves several experiments; sse / P as that call's, a flagged row: esum = NaN.
 * ------------------------------------------------------------------------------------- */
#define TRPL_MAG_PER_CURVE 0x1
#define TRPL_MAG_MAX_CURVES 64
int trpl_loglik_moments(const double *X, int64_t S, int32_t C, const double *lengths_nm, double time_ns,
                        int32_t L, int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN,
                        const double *obs, const int32_t *obs_hi, const double *obs_dx, const double *obs_h,
                        int64_t obs_ld, const int64_t *n_obs, double *P, double *sse, double *esum, int32_t *status,
                        int64_t *iters_total, int32_t *floor_col, uint32_t flags, int32_t device, double *seconds);
int trpl_loglik_moments_dev(const double *X, int64_t S, int32_t C, const double *lengths_nm /*host*/, double time_ns,
                            int32_t L, int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN,
                            const double *obs, const int32_t *obs_hi, const double *obs_dx, const double *obs_h,
                            int64_t obs_ld, const int64_t *n_obs /*host*/, double *P, double *sse, double *esum,
                            int32_t *status, int64_t *iters_total, int32_t *floor_col, uint32_t flags, void *stream);
int trpl_loglik_moments_from_pl_dev(const void *plI, int32_t elem_bytes, int64_t rows, int64_t ncol, int64_t ld,
                                    const double *obs, const int32_t *obs_hi, const double *obs_dx,
                                    const double *obs_h, int64_t n_obs, const double *mag, const int32_t *status,
                                    double *P, double *sse, double *esum, uint32_t flags, void *stream);
int trpl_mag_grid(const double *sse, const double *esum, const int64_t *n_obs, int64_t S, int32_t C,
                  const double *offsets, int64_t M, double *P);
int trpl_mag_grid_dev(const double *sse, const double *esum, const int64_t *n_obs /*host*/, int64_t S, int32_t C,
                      const double *offsets /*host*/, int64_t M, double *P, void *stream);
int trpl_mag_profile(const double *sse, const double *esum, const int64_t *n_obs, int64_t S, int32_t C,
                     uint32_t flags, double *best, double *P);
int trpl_mag_profile_dev(const double *sse, const double *esum, const int64_t *n_obs /*host*/, int64_t S, int32_t C,
                         uint32_t flags, double *best, double *P, void *stream);

/* ---------------------------------------------------------------------------------------
 * trpl_loglik_weighted -- the UNCERTAINTY-WEIGHTED fused likelihood.  Every observation file has a third column; the
 * reference rescales it to log10 units (bayes_io.py:75-76: sigma / PL / 2.3), ships it to the device and never reads it: the
 * weighting line of kernel_lnP is commented out (probs.py:20-62, :40: `#err /= (2 * uncertainty[i] ** 2)`).  This call
 * restores it on the fused path, inside the stepper's sink (PL never leaves the registers):
 *     e_i = log10 PL_i + X[s][12] - obs_ci  (exactly trpl_loglik[_obs]'s errors),
 *     sse[c][s]  = sum_i w_ci e_i^2,     esum[c][s] = sum_i w_ci e_i,     P[s] -= sum_c sse[c][s]   (curves in order)
 * with each term formed as ((e * e) * w) and (e * w), summed in trpl_loglik_moments' order and association.  Hence
 * weights of 1.0 give trpl_loglik_moments' outputs bit for bit, and a power-of-two weight scales them exactly.
 * Arguments: those of trpl_loglik_moments[_dev] plus wts [C][obs_ld] fp64 directly after obs, indexed like obs (the first
 * n_obs[c] entries of row c are read; off-grid: sorted together with the observation times).  w = 1 / (2 sigma^2) is the
 * chi-square weight of the commented line (Python: likelihood.weights_from_uncertainty).
 * status, iters_total and floor_col do NOT depend on the weights: a weight never enters the solve, and the simulated
 * window still ends at the last observation whatever its weight.  A ZERO WEIGHT removes a finite term -- the observation
 * counts as absent from both sums -- but it does not hide a NaN or infinite observation or error (0 * NaN = NaN).  A
 * flagged system: sse = +inf, esum = NaN.  On- and off-grid (obs_hi / obs_dx / obs_h all NULL or all non-NULL, then
 * plT = 1); any number of curves up to TRPL_MAX_CURVES, run as consecutive launches like the other calls.
 * The host form checks the n_obs[c] weights of every curve BEFORE it touches a device: finite and >= 0, otherwise
 * TRPL_ERR_ARG naming curve and index.  The _dev form cannot look (a device pointer, no synchronisation): there the
 * caller owns that -- a negative weight gives a meaningless sum, a NaN weight a NaN likelihood.
 * TRPL_FLAG_WEIGHTED is set by the call.  Refused: TRPL_FLAG_MOMENTS in flags (TRPL_ERR_ARG); TRPL_FLAG_FP32, _MIXED,
 * _HIST32, TRPL_FLAG_BUNDLE(m > 1) (TRPL_ERR_UNSUPPORTED); there are no snapshot / resume forms.
 * trpl_loglik_multi* has no weighted form (out of scope: the sharded drivers keep the unweighted one-offset likelihood).
 *
 * trpl_mag_grid_w / trpl_mag_profile_w -- trpl_mag_grid / trpl_mag_profile from the weighted moments, with
 * wsum [C] HOST fp64, wsum_c = sum_i w_ci (finite, >= 0), in place of n_obs:  sum_i w (e_i + d)^2 = sse + 2 d esum + wsum d^2,
 *     P[m][s] -= sum_c max(sse[c][s] + (2 d_m) esum[c][s] + wsum_c (d_m d_m), 0)
 *     best[s] = -(sum_c esum[c][s]) / (sum_c wsum_c);   TRPL_MAG_PER_CURVE: best[c][s] = -esum[c][s] / wsum_c
 * -- the SAME expression as the unweighted calls (they pass (double)n_obs[c]): with wsum = n_obs the results are equal bit
 * for bit.  wsum_c = 0 (every weight of the curve zero): best = NaN, and the curve contributes 0 to P.
 * ERROR BOUND (A_w(d) = sse + 2 |d esum| + wsum d^2, eps = 2^-52): against a direct evaluation of sum w_i (e_i + d)^2 on the
 * same PL,   |P_grid - P_direct| <= k eps (A_w(d) + |d| sum w_i |e_i|),   k = 6 + ceil(n / 64) + 6
 * (the moments bound with two more roundings, one for each multiplication by the weight; k = n + 6 for serial sums).
 * trpl_loglik_weighted_from_pl_dev -- trpl_loglik_moments_from_pl_dev with wts [n_obs] directly after obs: the weighted
 * sums of a resident PL block (sse [rows], esum [rows], P[j] -= sse_j).
 * ------------------------------------------------------------------------------------- */
int trpl_loglik_weighted(const double *X, int64_t S, int32_t C, const double *lengths_nm, double time_ns,
                         int32_t L, int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN,
                         const double *obs, const double *wts, const int32_t *obs_hi, const double *obs_dx,
                         const double *obs_h, int64_t obs_ld, const int64_t *n_obs, double *P, double *sse, double *esum,
                         int32_t *status, int64_t *iters_total, int32_t *floor_col, uint32_t flags, int32_t device,
                         double *seconds);
int trpl_loglik_weighted_dev(const double *X, int64_t S, int32_t C, const double *lengths_nm /*host*/, double time_ns,
                             int32_t L, int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN,
                             const double *obs, const double *wts, const int32_t *obs_hi, const double *obs_dx,
                             const double *obs_h, int64_t obs_ld, const int64_t *n_obs /*host*/, double *P, double *sse,
                             double *esum, int32_t *status, int64_t *iters_total, int32_t *floor_col, uint32_t flags,
                             void *stream);
int trpl_loglik_weighted_from_pl_dev(const void *plI, int32_t elem_bytes, int64_t rows, int64_t ncol, int64_t ld,
                                     const double *obs, const double *wts, const int32_t *obs_hi, const double *obs_dx,
                                     const double *obs_h, int64_t n_obs, const double *mag, const int32_t *status,
                                     double *P, double *sse, double *esum, uint32_t flags, void *stream);
int trpl_mag_grid_w(const double *sse, const double *esum, const double *wsum, int64_t S, int32_t C,
                    const double *offsets, int64_t M, double *P);
int trpl_mag_grid_w_dev(const double *sse, const double *esum, const double *wsum /*host*/, int64_t S, int32_t C,
                        const double *offsets /*host*/, int64_t M, double *P, void *stream);
int trpl_mag_profile_w(const double *sse, const double *esum, const double *wsum, int64_t S, int32_t C,
                       uint32_t flags, double *best, double *P);
int trpl_mag_profile_w_dev(const double *sse, const double *esum, const double *wsum /*host*/, int64_t S, int32_t C,
                           uint32_t flags, double *best, double *P, void *stream);

/* ---------------------------------------------------------------------------------------
 * trpl_loglik_cut -- the fused likelihood with an EARLY STOP of hopeless systems (opt-in; the exact, work-saving form of the
 * bval_cutoff of the reference's older likelihood, probs.py:5-18, commented out in the live kernel at probs.py:34-35).
 * sse[c][s] is a running sum of non-negative terms e_i^2, so it never decreases: once it is above a level, the system's
 * final likelihood is known to be below minus that level whatever the remaining time steps would add, and a caller that
 * only needs to know THAT (a posterior weight that underflows to 0.0, see Python posterior.exact_cut_margin) need not
 * pay for them.  On the fused path PL never leaves the registers, so the stop happens inside the stepper's sink.
 * Arguments: those of trpl_loglik_moments[_dev] without esum, plus
 *   sse_cut   the level, directly after n_obs: >= 0 or +inf (NaN or negative: TRPL_ERR_ARG);
 *   cut_col   [C][S] int32 out, directly after sse, nullable.
 * obs_hi / obs_dx / obs_h all NULL: observations on the grid (as trpl_loglik); all non-NULL: off-grid (as trpl_loglik_obs,
 * plT must be 1).  TRPL_FLAG_CUT is set by the call.
 * WHEN THE TEST RUNS.  The FAST sinks add the squared errors one batch of 64 PL columns at a time; each system tests
 * `running sse > sse_cut` after every batch its sink adds, the final (partial) batch included.  The first time the test is
 * true the system stops: no further time step, no further observation.
 * WHAT A CUT SYSTEM REPORTS.  sse[c][s]: the running sum at that moment -- what the plain call (trpl_loglik / trpl_loglik_obs,
 * same flags) returns for n_obs[c] = cut_col[c][s], bit for bit.  cut_col[c][s]: the number of leading observations in that
 * sum (on-grid: a multiple of 64, or n_obs[c]).  status: 0.  floor_col: what the plain call truncated there reports.
 * iters_total, on-grid: the truncated plain call's (both run the steps 0 .. (cut_col - 1) plT).  iters_total, off-grid: a cut
 * system runs to the end of its 64-column batch, so only iters_total <= the plain full call's is promised.
 * AN UNCUT SYSTEM: cut_col = -1 and every output is the plain call's, bit for bit.  A NON-CONVERGED SYSTEM: as in the plain
 * call (sse = +inf, floor_col = -2), and cut_col = -2 -- unless its sum passed the level BEFORE the time step that fails: it
 * stopped there and never takes that step, so it is a cut system like any other (status 0, the truncated plain call's
 * outputs).  The plain call's sse of such a system is +inf, above every level: it is never reported uncut.
 * A NaN running sum never compares true: such a system is never cut.
 * EXACT EQUIVALENCE.  Adding a non-negative term in floating point never decreases a sum, so cut_col >= 0 holds exactly when
 * the plain call's final sse > sse_cut.  Hence sse_cut = +inf gives the plain call's outputs with cut_col = -1 everywhere,
 * and sse_cut = 0 stops every converging system with a non-zero error after its first batch.
 * P[s] -= sum_c sse[c][s] over the REPORTED values (curves in order): for a sample with a cut curve the reported P is at or
 * above the true P, and at or below P_in - sse_cut.
 * The test is per system, against the system's own sum -- never the wavefront partner's or the sample's total: a system's
 * outputs do not depend on sharding, wavefront partner, pairing rule (TRPL_FLAG_PAIR_ADJACENT) or seam form
 * (TRPL_FLAG_PAIR_ALWAYS_SEAM).  In the paired kernel a cut system is parked like a non-converged one and its wavefront
 * ends when both halves are done; workgroups are dispatched in order, so a wave that ends early hands its slot to the next.
 * Combines with TRPL_FLAG_PREDICT, _PL_F32, _NORMALIZE, _BDF_ORDER, _KERNEL_PAIR / _SINGLE, _PAIR_ALWAYS_SEAM, _PAIR_ADJACENT;
 * any number of curves up to TRPL_MAX_CURVES, run as consecutive launches like the other calls.
 * Refused with TRPL_ERR_UNSUPPORTED, before a device is touched: TRPL_FLAG_STRICT (its sink emits column by column: another
 * granularity), _FP32, _MIXED, _HIST32, TRPL_FLAG_BUNDLE(m > 1).  Refused with TRPL_ERR_ARG: TRPL_FLAG_MOMENTS, _WEIGHTED
 * (the profile minimum sse - esum^2 / wsum is non-decreasing too: a later change can compose them).  There are no snapshot,
 * resume or trpl_loglik_multi* forms.
 * ------------------------------------------------------------------------------------- */
int trpl_loglik_cut(const double *X, int64_t S, int32_t C, const double *lengths_nm, double time_ns,
                    int32_t L, int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN,
                    const double *obs, const int32_t *obs_hi, const double *obs_dx, const double *obs_h,
                    int64_t obs_ld, const int64_t *n_obs, double sse_cut, double *P, double *sse, int32_t *cut_col,
                    int32_t *status, int64_t *iters_total, int32_t *floor_col, uint32_t flags, int32_t device,
                    double *seconds);
int trpl_loglik_cut_dev(const double *X, int64_t S, int32_t C, const double *lengths_nm /*host*/, double time_ns,
                        int32_t L, int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN,
                        const double *obs, const int32_t *obs_hi, const double *obs_dx, const double *obs_h,
                        int64_t obs_ld, const int64_t *n_obs /*host*/, double sse_cut, double *P, double *sse,
                        int32_t *cut_col, int32_t *status, int64_t *iters_total, int32_t *floor_col, uint32_t flags,
                        void *stream);

/* ---------------------------------------------------------------------------------------
 * trpl_loglik_cut_levels -- trpl_loglik_cut with A LEVEL PER SYSTEM: the arguments of trpl_loglik_cut[_dev] with
 *   cut_level   [C][S] f64, indexed like cut_col,
 * in the place of sse_cut.  TRPL_FLAG_CUT is set by the call; the kernels (the same 20 trpl::cut:: instantiations), flags,
 * combinations and refusals are trpl_loglik_cut's.  Its consumer is a Metropolis sampler, whose rejection threshold differs from
 * chain to chain and is known before the solve (trpl_mcmc_levels below).
 * System (c, s) tests `running sse > cut_level[c][s]` after every batch its sink adds.  Every output of a system is what
 * trpl_loglik_cut returns for it at sse_cut = cut_level[c][s], bit for bit: a cut system reports the truncated plain call, an
 * uncut system the full plain call, and the paragraphs above on status, floor_col, iters_total and non-converged systems hold
 * with the system's own level.  The proof is trpl_loglik_cut's, system by system: the sum never decreases.
 * A system's outputs do not depend on the levels of other systems, on its wavefront partner, on the pairing rule, on the seam
 * form or on sharding: the level is read by the system's own sink through its own output row (the two sinks of a paired
 * wavefront each read theirs), once per batch, as a wave-uniform scalar load.
 * P[s] -= sum_c sse[c][s] over the reported values, as in trpl_loglik_cut.
 * The host form checks every level (>= 0 or +inf) before it touches a device: a NaN or negative level is TRPL_ERR_ARG and the
 * message names the curve and the sample ("cut_level[c=..][s=..]").  The _dev form cannot look at the levels: there a NaN level
 * never cuts, and a negative level cuts after the first batch.  A NULL cut_level is TRPL_ERR_ARG.  The host form stages
 * cut_level like cut_col.  There is no trpl_loglik_multi* form.
 * ------------------------------------------------------------------------------------- */
int trpl_loglik_cut_levels(const double *X, int64_t S, int32_t C, const double *lengths_nm, double time_ns,
                           int32_t L, int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN,
                           const double *obs, const int32_t *obs_hi, const double *obs_dx, const double *obs_h,
                           int64_t obs_ld, const int64_t *n_obs, const double *cut_level /* [C][S] */, double *P, double *sse,
                           int32_t *cut_col, int32_t *status, int64_t *iters_total, int32_t *floor_col, uint32_t flags,
                           int32_t device, double *seconds);
int trpl_loglik_cut_levels_dev(const double *X, int64_t S, int32_t C, const double *lengths_nm /*host*/, double time_ns,
                               int32_t L, int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN,
                               const double *obs, const int32_t *obs_hi, const double *obs_dx, const double *obs_h,
                               int64_t obs_ld, const int64_t *n_obs /*host*/, const double *cut_level /* [C][S] */, double *P,
                               double *sse, int32_t *cut_col, int32_t *status, int64_t *iters_total, int32_t *floor_col,
                               uint32_t flags, void *stream);

/* ---------------------------------------------------------------------------------------
 * trpl_loglik_cut_budget -- the early stop on a SAMPLE'S TOTAL: a budget carried across the curves.  trpl_loglik_cut[_levels] test
 * each (curve, sample) system on its own, although the levels their callers have (a Metropolis step's, margin + best total) are
 * levels for the sample's SUMMED squared error: a sample whose error is spread evenly over C curves runs to about C times the level
 * before one system stops.  This call spends one level per sample across its curves.  The arguments of trpl_loglik_cut_levels[_dev]
 * with
 *   budget             [S] f64, the level for sum_c sse[c][s], where cut_level is;
 *   curves_per_launch  g, 1 <= g <= TRPL_MAX_CURVES, directly after it;
 *   cut_level          [C][S] f64 OUT, directly before P: the level every system ran at.
 * TRPL_FLAG_CUT is set by the call; the steppers (the same 20 trpl::cut:: instantiations), flags, combinations and refusals are
 * trpl_loglik_cut's.  No stepper and no sink is changed: the only new kernel is trpl::budget::level_kernel (csrc/cut_budget.hip).
 * THE RULE.  The C curves run as consecutive launches of g curves each (the last one possibly ragged), on the same stream, in curve
 * order; the stepper variant is pinned once from the whole batch (as for C > TRPL_MAX_CURVES), so a system's bits do not depend on
 * g.  Before launch j, whose first curve is c0 = j g, one thread per sample forms the level that all curves of that launch run at,
 * from B = budget[s] and the REPORTED sse of the curves 0 .. c0 - 1, and writes it into the rows c0 .. c0 + g - 1 of cut_level:
 *   R = the sum of sse[c][s], c = 0 .. c0 - 1 in ascending order from +0.0, one rounding per addition (the unit is built with
 *       -ffp-contract=off): minus what the reduction over the curves makes of a P that starts at zero;
 *   launch 0:    level = B itself (nothing is carried yet; B = 0 cuts every system with a non-zero error after its first batch);
 *   B or R NaN:  level = +inf, in launch 0 too (the sample is never cut; the host form refuses a NaN budget, the _dev form cannot look);
 *   B = +inf:    level = +inf, whatever R;
 *   R >= B:      level = -1.0 -- the sample is already past its budget, and the sink cuts its later systems after their first
 *                64-column batch, as trpl_loglik_cut_levels_dev says a negative level does;
 *   otherwise the candidates are l0 = max(fl(B - R), 0), nextafter(l0, +inf) and nextafter of that: the first l with
 *                fl(R + l) >= B is the level; if none verifies, +inf.
 * For B > 0 launch 0's level is also what the rule gives at R = +0.0; with g >= C the call is trpl_loglik_cut_levels with budget[s] as the level
 * of every curve of sample s, and budget = +inf everywhere gives the plain call with cut_col = -1.
 * WHAT IS REPORTED.  Every output of system (c, s) is, bit for bit, what trpl_loglik_cut_levels_dev reports for it at the returned
 * cut_level[c][s]; P[s] -= sum_c sse[c][s] over the reported values, as in trpl_loglik_cut.  The results do not depend on
 * sharding, pairing rule or seam form (a sample's levels are formed from its own rows only).
 * WHY THAT IS SAFE.  Floating-point addition of non-negative terms is monotone: a <= a' and b <= b' give fl(a + b) <= fl(a' + b').
 * A system cut at a level l >= 0 reports sse_c > l, and its plain sse_c (the sum never decreases) is above l too.  R is the
 * reported total of the curves before it, at or below their plain total.  So for a sample with a cut system both the reported total
 * and the plain call's total are  fl(.. fl(R + sse_c) ..) >= fl(R + l) >= B,  the last step being the test the rule made before it
 * took l.  A level of -1.0 is only given when R >= B already, and every later term keeps the total there.  Hence: a sample with any
 * cut_col >= 0 has a plain total >= budget[s], and its reported P is at or below P_in - budget[s] when P_in is +0.0.
 * With budget = a level of trpl_mcmc_levels*, LLp = -total <= -level = q is rejected by trpl_mcmc_accept's own expression (the
 * property stated there holds for every LLp <= q).  With budget = margin + best total, the posterior weight of a sample whose total
 * is at or above it is exactly 0.0 (posterior.exact_cut_margin's argument uses <=).
 * HOW TIGHT.  l is l0 or one of its two successors, so a sample stops once a later curve's running sse is above about B - R: with
 * g = 1 the whole of what the earlier curves reported is spent.  WHAT IT COSTS.  g < C serialises the curves: C / g launches, each
 * as long as its slowest uncut system, and each filling the device only from S g systems.  It pays where S is large or most
 * samples die in their first curves, and loses on small batches (DESIGN.md has the measurements).
 * Refused with TRPL_ERR_ARG: budget or cut_level NULL with S > 0 ("budget must not be NULL", "cut_level must not be NULL");
 * curves_per_launch outside [1, TRPL_MAX_CURVES]; host form only, before a device is touched: a NaN or negative budget[s], the
 * message names the sample ("budget[s=..]").  The _dev form allocates nothing and never synchronises; a negative budget there cuts
 * every system of the sample after its first batch.  The host form stages budget in and cut_level out.  There is no
 * trpl_loglik_multi* form.  Python: trpl_amd.driver.loglik(cut_budget=, curves_per_launch=), trpl_amd.mcmc.run(early_reject="sample"),
 * gpu_info["cut_budget"], trpl_amd.device.loglik_cut_budget_device.
 * ------------------------------------------------------------------------------------- */
int trpl_loglik_cut_budget(const double *X, int64_t S, int32_t C, const double *lengths_nm, double time_ns,
                           int32_t L, int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN,
                           const double *obs, const int32_t *obs_hi, const double *obs_dx, const double *obs_h,
                           int64_t obs_ld, const int64_t *n_obs, const double *budget /* [S] */, int32_t curves_per_launch,
                           double *cut_level /* [C][S] out */, double *P, double *sse, int32_t *cut_col, int32_t *status,
                           int64_t *iters_total, int32_t *floor_col, uint32_t flags, int32_t device, double *seconds);
int trpl_loglik_cut_budget_dev(const double *X, int64_t S, int32_t C, const double *lengths_nm /*host*/, double time_ns,
                               int32_t L, int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter, const double *dN,
                               const double *obs, const int32_t *obs_hi, const double *obs_dx, const double *obs_h,
                               int64_t obs_ld, const int64_t *n_obs /*host*/, const double *budget /* [S] */,
                               int32_t curves_per_launch, double *cut_level /* [C][S] out */, double *P, double *sse,
                               int32_t *cut_col, int32_t *status, int64_t *iters_total, int32_t *floor_col, uint32_t flags,
                               void *stream);

/* ---------------------------------------------------------------------------------------
 * trpl_loglik_multi --trpl_loglik / trpl_loglik_obs over several devices from ONE host thread:
 * replaces the reference's distribution of 1024-sample blocks over GPUs (bayeslib.py:131 and the
 * commented-out threaded driver :235-246; one SLURM array task per GPU, :231).  The samples are cut
 * into n_devices contiguous shards (trpl_shard_bounds); every shard is staged, solved and copied back
 * on its own device and stream, all devices run concurrently, and the call returns when the host
 * arrays P[S], sse[C][S], status[C][S], iters_total[C][S] (the last three nullable) are complete.  There is
 * no device-to-device exchange: the systems are independent and the result lives on the host.
 *   devices   [n_devices] HIP device ordinals (an ordinal may repeat: each entry gets its own stream),
 *             or NULL for 0..n_devices-1;  n_devices <= 0 with devices == NULL means every visible device.
 *   obs_hi / obs_dx / obs_h  all NULL: observations on the simulation grid (as trpl_loglik);
 *             all non-NULL: off-grid observations (as trpl_loglik_obs, plT must be 1).
 * The stepper variant is chosen once, from the size of the WHOLE batch (S * C systems), and pinned for every
 * shard, and a system's result does not depend on which other systems share its launch or its wavefront:
 * the results are bit-identical to a single-device call on the same batch, however it is cut.
 * ------------------------------------------------------------------------------------- */
int trpl_loglik_multi(const double *X, int64_t S, int32_t C, const double *lengths_nm, double time_ns,
                      int32_t L, int64_t T, int32_t plT, int32_t tol_exp, int32_t max_iter,
                      const double *dN, const double *obs, const int32_t *obs_hi, const double *obs_dx,
                      const double *obs_h, int64_t obs_ld, const int64_t *n_obs, double *P, double *sse,
                      int32_t *status, int64_t *iters_total, int32_t *floor_col /*[C][S], nullable*/,
                      uint32_t flags, const int32_t *devices, int32_t n_devices, double *seconds);

/* ---------------------------------------------------------------------------------------
 * trpl_multi_* / trpl_loglik_multi_dev -- the device-resident multi-GPU form: ONE process drives
 * n_devices HIP devices; the samples are cut into contiguous shards (trpl_shard_bounds), every device solves
 * its shard, and ONE collective -- an RCCL ncclAllGather over xGMI of ceil(S / n_devices) fp64 per rank --
 * leaves the complete likelihood vector P[S] in the memory of EVERY device, where the posterior core
 * (trpl_posterior_*_dev) consumes it.  Replaces what the reference's commented-out threaded driver
 * (bayeslib.py:235-246) and its one-SLURM-task-per-GPU distribution (:131,:231) leave to separate .npy files.
 *
 * trpl_multi_create: ncclCommInitAll over `devices` (NULL: 0..n_devices-1; n_devices <= 0: every visible
 *   device; ordinals must be distinct), one non-blocking stream per device.  RCCL (librccl.so.1) is bound at
 *   this call, not at library load.  The handle is reusable and not thread-safe.
 * trpl_loglik_multi_dev: per-device pointer tables (host arrays of n_devices device pointers, entry r valid
 *   on devices[r]):
 *     X[r]      [n_r][13]   that shard's samples, n_r = hi_r - lo_r of trpl_shard_bounds(S, n_devices, r)
 *     dN[r]     [C][L]      replicated;  obs[r] [C][obs_ld] replicated (obs_hi / obs_dx / obs_h: tables of
 *               replicated bracket arrays, or all three NULL for on-grid observations)
 *     P_full[r] [S]         OUT on every device: P[s] = - sum_c sse[c][s], the all-gathered likelihoods
 *     sse[r], status[r], iters_total[r], floor_col[r]  [C][n_r] per-shard outputs (tables nullable, as are entries)
 *   Everything is enqueued on the handle's streams (solve, all-gather, unpadding) and the call returns
 *   without waiting; trpl_multi_synchronize waits for all devices.  The kernel variant is pinned from the
 *   whole batch, as in trpl_loglik_multi.
 * ------------------------------------------------------------------------------------- */
typedef struct trpl_multi trpl_multi_t;
int trpl_multi_create(const int32_t *devices, int32_t n_devices, trpl_multi_t **handle);
/* trpl_multi_create with options.  TRPL_MULTI_ALLOW_DUPLICATE_DEVICES: a device ordinal may be listed more than once (one
 * "rank" and stream each) -- for tests that run several ranks on one GPU against a stand-in collective library named by
 * TRPL_RCCL_LIBRARY (tests/mock_rccl); real RCCL refuses duplicate devices. */
#define TRPL_MULTI_ALLOW_DUPLICATE_DEVICES 0x1
int trpl_multi_create_ex(const int32_t *devices, int32_t n_devices, uint32_t create_flags, trpl_multi_t **handle);
int trpl_multi_destroy(trpl_multi_t *handle);
int trpl_multi_device_count(const trpl_multi_t *handle);
int trpl_multi_synchronize(trpl_multi_t *handle);
int trpl_loglik_multi_dev(trpl_multi_t *handle, const double *const *X, int64_t S, int32_t C,
                          const double *lengths_nm /*host*/, double time_ns, int32_t L, int64_t T, int32_t plT,
                          int32_t tol_exp, int32_t max_iter, const double *const *dN, const double *const *obs,
                          const int32_t *const *obs_hi, const double *const *obs_dx, const double *const *obs_h,
                          int64_t obs_ld, const int64_t *n_obs /*host*/, double *const *P_full,
                          double *const *sse, int32_t *const *status, int64_t *const *iters_total,
                          int32_t *const *floor_col, uint32_t flags);
/* The handle's streams are its own (non-blocking): nothing orders them against the streams on which the caller
 * produced X / dN / obs or will consume P_full.  Either wait on the host (trpl_multi_synchronize on both sides), or
 * add the order on the device:
 *   trpl_multi_wait_stream(h, r, s):    what the handle enqueues on rank r from now on runs after what stream s (a
 *                                       hipStream_t of devices[r]; NULL = its default stream) holds now -- call it for
 *                                       every rank BEFORE trpl_loglik_multi_dev when the inputs were just written on s;
 *   trpl_multi_release_stream(h, r, s): what s is given from now on runs after what the handle has enqueued on rank r
 *                                       -- call it AFTER trpl_loglik_multi_dev before reading P_full[r] on s.
 * (trpl_amd.device.MultiDevice.loglik does both with torch's current stream of each device.) */
int trpl_multi_wait_stream(trpl_multi_t *handle, int32_t rank, void *stream);
int trpl_multi_release_stream(trpl_multi_t *handle, int32_t rank, void *stream);

/* [lo, hi) of shard `shard` of S samples cut into n_shards contiguous ranges; the first S % n_shards
 * shards hold one more.  The same rule shards the samples over ranks in the one-process-per-GPU
 * driver (bench.py, trpl_amd.dist.shard_bounds). */
int trpl_shard_bounds(int64_t S, int32_t n_shards, int32_t shard, int64_t *lo, int64_t *hi);
/* the shard whose range contains sample s (the inverse of trpl_shard_bounds; the unpadding pass after the
 * all-gather of trpl_loglik_multi_dev indexes with it); -1 for arguments out of range */
int64_t trpl_shard_of(int64_t S, int32_t n_shards, int64_t s);

/* ---------------------------------------------------------------------------------------
 * trpl_sample_box -- replaces bayeslib.random_grid(minX, maxX, do_log, num_points) after
 * numpy.random.seed(seed) (bayeslib.py:18-32, parallel_bayes_gpu.py:35) and the make_grid overrides
 * (bayeslib.py:67-75), generating X[S][ncol] in device memory: the same MT19937 stream, the same draw
 * order (column after column, fixed columns draw nothing), the same 53-bit doubles.  Linear columns are
 * bit-identical to the reference's; log-uniform columns go through the device's pow() (<= 1 ulp from
 * the host's).  lo / hi / do_log are HOST arrays [ncol] (bounds already unit-converted, as the reference
 * passes them).  flags: 1 = equal mobilities (X[:,2] = X[:,3]), 2 = equal surface velocities
 * (X[:,6] = X[:,5]), 4 = equal Auger coefficients (X[:,8] = X[:,7]).
 * ------------------------------------------------------------------------------------- */
#define TRPL_BOX_EQUAL_MU 0x1
#define TRPL_BOX_EQUAL_S 0x2
#define TRPL_BOX_EQUAL_AUGER 0x4
int trpl_sample_box(uint32_t seed, int64_t S, int32_t ncol, const double *lo, const double *hi,
                    const int32_t *do_log, uint32_t flags, double *X, int32_t device, double *seconds);
int trpl_sample_box_dev(uint32_t seed, int64_t S, int32_t ncol, const double *lo /*host*/,
                        const double *hi /*host*/, const int32_t *do_log /*host*/, uint32_t flags,
                        double *X /*device*/, void *stream);

/* ---------------------------------------------------------------------------------------
 * Posterior core -- the consumer of the likelihood vector: replaces the numpy reductions
 * of Visualization/utils.py on *_BAYRAN_{P,X}.npy.  Streaming, HBM-bound (8 B of likelihood + 8 B per
 * parameter column per sample); results are small arrays a multi-GPU caller can all-reduce.
 *
 * trpl_posterior_weights: normalize(LL / tf)  (utils.py:157-166, marginalization_visual.py:589-591):
 *     W[i] = exp(LL[i]/tf - nanmax(LL/tf) + 1000 ln 2 - ln S) / nansum(same);  NaN stays NaN, -inf gives 0.
 * trpl_posterior_moments: V is [D][S] (one contiguous column per parameter, D <= 16), W the weights;
 *     sums[2+D]      = { sum w, sum w^2, sum w v_d }
 *     central[D][D+2] = { sum w (v_d - m_d)(v_e - m_e) for e < D,  sum w (v_d - m_d)^3,  sum w (v_d - m_d)^4 }
 *     with m = sum w v / sum w: w_mean :197-199, w_variance :202-204, covariance :222-227, w_skew :207-210,
 *     w_kurtosis :212-215 and the weighted sample deviation :168-170 are quotients of these.
 * trpl_posterior_hist: weighted counts (W == NULL: plain counts) of x (and y, for 2-D) in `bins` equal
 *     bins whose edges are lo + (hi - lo) * k / bins exactly as marginalize_1D :243-244 / marginalize_2D
 *     :270-277 build them, with numpy.histogram's rules (left-closed, last bin closed, outside and NaN
 *     dropped); out[xbins] or out[xbins][ybins]; density normalisation is the caller's one-liner.
 * For callers that hold a shard of the samples (one process per GPU): `stats` = { nanmax(LL/tf), nansum of
 * the unnormalised weights } lets the shards' weights be renormalised to the global sum; `mean_in` [D]
 * centres the second call about the all-reduced means; histograms and sums add across shards.
 * The _dev forms take device pointers (out must be zeroed by the caller for hist) and a workspace of
 * trpl_posterior_workspace_bytes(D) bytes (D = 1 for the weights); nothing is allocated.
 * seconds (nullable), here, in trpl_solve_pl[_snap|_resume], trpl_loglik[_obs|_moments|_weighted|_cut] and in every other
 * analysis-side host-buffer call of this header (trpl_sample_box, temperature scan, predictive band, quantiles, corner, refinement,
 * MCMC, trpl_pcr_solve_batched): the device time of the _dev form, from the inputs having landed on the device to its last kernel
 * having finished; the copies in and out are not in it.  Three calls keep the reference's clock instead, which starts before the
 * copies in (probs.py:79, :51): trpl_log10_clamp and trpl_sse_accumulate[_w] time the uploads plus the kernel, not the copy back.
 * ------------------------------------------------------------------------------------- */
int64_t trpl_posterior_workspace_bytes(int32_t D);
int trpl_posterior_weights(const double *LL, int64_t S, double tf, double *W, double *stats /*nullable [2]*/,
                           int32_t device, double *seconds);
int trpl_posterior_weights_dev(const double *LL, int64_t S, double tf, double *W, double *stats, void *workspace,
                               int64_t workspace_bytes, void *stream);
int trpl_posterior_moments(const double *V, int64_t S, int32_t D, const double *W, const double *mean_in /*nullable*/,
                           double *sums, double *central, int32_t device, double *seconds);
int trpl_posterior_moments_dev(const double *V, int64_t S, int32_t D, const double *W, const double *mean_in,
                               double *sums, double *central, void *workspace, int64_t workspace_bytes,
                               void *stream);
int trpl_posterior_hist(const double *x, const double *y /*nullable: 1-D*/, const double *W /*nullable*/,
                        int64_t S, double xlo, double xhi, int32_t xbins, double ylo, double yhi,
                        int32_t ybins, double *out, int32_t device, double *seconds);
int trpl_posterior_hist_dev(const double *x, const double *y, const double *W, int64_t S, double xlo,
                            double xhi, int32_t xbins, double ylo, double yhi, int32_t ybins, double *out,
                            void *stream);

/* ---------------------------------------------------------------------------------------
 * trpl_posterior_tf_scan -- the posterior at K temperatures from one scan of the samples: what choosing the temperature
 * factor needs (LikelihoodData.calc_max_uncertainty -> find_best_tf -> tf_driver, Visualization/utils.py:128-133, 168-183:
 * the tf that maximises Q(tf) = sqrt(sum W^2 * weighted variance), W = normalize(LL / tf)).  For every k < K, with
 * W_k = trpl_posterior_weights(LL, S, tfs[k]) and {sums, central} = trpl_posterior_moments(V, S, D, W_k):
 *     stats[K][4] = { nanmax(LL / tfs[k]), nansum of the unnormalised weights, sum W_k^2 (= sums[1]),
 *                     count of non-NaN entries of LL (the same for every k) }
 *     mean[K][D]  = sums[2 + d] / sums[0]                       w_mean      :197-199
 *     var[K][D]   = central[d][d] / sums[0]                     w_variance  :202-204
 *     Q[K][D]     = sqrt(sums[1] * var[k][d])                   w_sample_var :168-170
 * BIT FOR BIT what those two calls give (the same weight expression, the same per-block partials combined in the same
 * fixed order: csrc/posterior_common.hpp), so a temperature found with the scan is the temperature of the calls that then
 * use it.  No weight vector is written: each phase recomputes the K exponentials of LL[s] in registers.  No atomics; the
 * result does not depend on scheduling.  NaN and -inf follow the two calls: a NaN likelihood is skipped by the maximum and
 * the normalising sum, its weight is NaN and so are the sums over the weights; -inf has weight 0.
 * V is [D][S] as in trpl_posterior_moments; D == 0 (V, mean, var, Q may then be NULL) returns stats alone.
 * Refused with TRPL_ERR_ARG before a device is touched, the message naming the argument (and the index in tfs):
 * S < 1; D outside [0, 16]; K < 1 or K > TRPL_TF_SCAN_MAX; a NULL LL, tfs, stats, or (D > 0) V, mean, var, Q; a tfs[k] that
 * is not finite and > 0 (host form; in the _dev form tfs is device memory and cannot be looked at).
 * The _dev form takes device pointers for everything and a workspace of trpl_posterior_tf_scan_workspace(S, D, K) bytes
 * (0 for arguments the scan refuses); it allocates nothing, never synchronises and can be captured in a HIP graph.
 * ------------------------------------------------------------------------------------- */
#define TRPL_TF_SCAN_MAX 64
int64_t trpl_posterior_tf_scan_workspace(int64_t S, int32_t D, int32_t K);
int trpl_posterior_tf_scan(const double *LL, int64_t S, const double *V /*nullable: D == 0*/, int32_t D, const double *tfs,
                           int32_t K, double *stats, double *mean, double *var, double *Q, int32_t device, double *seconds);
int trpl_posterior_tf_scan_dev(const double *LL, int64_t S, const double *V, int32_t D, const double *tfs, int32_t K,
                               double *stats, double *mean, double *var, double *Q, void *workspace,
                               int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * trpl_posterior_weights_lr, trpl_posterior_tf_scan_lr -- the two calls above with a per-sample proposal log-ratio kept BESIDE
 * the log-likelihood instead of folded into it: the temperature-dependent front end for a refined set (trpl_refine_*, below),
 * whose sample s carries the weight exp(LL[s] / tf) / r(u_s).  With lnr[s] = ln r(u_s) (natural log, fp64):
 *     e_k[s] = LL[s] / tf_k - lnr[s]
 *     m_k    = nanmax_s e_k[s]
 *     w_k[s] = exp(((e_k[s] - m_k) + 1000 ln 2) - ln S)            (the order of utils.py:164)
 *     W_k    = w_k / nansum w_k
 * The weight is trpl_posterior_weights' compensated form: the remainder of the division, the rounding of the subtraction of lnr
 * and the roundings of the three sums are exact in fp64 and are put back.  m_k is NOT nanmax(LL) / tf_k: the sample that leads at
 * one temperature need not lead at another, so the maximum is taken per temperature.
 * NaN: a NaN in LL[s] or in lnr[s] gives a NaN weight; that sample is left out of m_k and of the normalising sum and is not
 * counted, and the sums over the weights (sum W, sum W^2, the moments, ess) are then NaN, as in trpl_posterior_moments.  LL = -inf
 * or lnr = +inf give a weight of exactly 0.  lnr = -inf is the caller's error (r >= S1 / S_total > 0 by construction) and is not
 * looked for.
 * trpl_posterior_weights_lr: one temperature; writes W[S] and stats (nullable) = { m, nansum of the unnormalised weights }.
 * trpl_posterior_tf_scan_lr: K <= TRPL_TF_SCAN_MAX temperatures, D <= 16 columns V[D][S]; mean, var, Q [K][D] as
 * trpl_posterior_tf_scan, and
 *     stats[K][6] = { m_k, nansum of the unnormalised weights, sum W_k, sum W_k^2, count of samples with neither LL nor lnr
 *                     NaN (the same for every k), ess_k = (sum W_k)^2 / sum W_k^2 }
 * BIT FOR BIT: row k of the scan is trpl_posterior_weights_lr(LL, lnr, S, tfs[k]) followed by trpl_posterior_moments(V, S, D, W);
 * trpl_posterior_weights_lr with lnr[s] = +0.0 for every s is trpl_posterior_weights; hence the scan with lnr = +0.0 is
 * trpl_posterior_tf_scan in every output the two share.  No atomics; the result does not depend on scheduling.
 * Refused with TRPL_ERR_ARG before a device is touched, the message naming the argument: what trpl_posterior_tf_scan refuses
 * (S < 1; D outside [0, 16]; K < 1 or K > TRPL_TF_SCAN_MAX; a NULL LL, tfs, stats, or (D > 0) V, mean, var, Q; in the host form a
 * tfs[k] that is not finite and > 0) and a NULL lnr; the weights call: S < 1, a NULL LL, lnr or W, a tf that is not finite and > 0.
 * The _dev forms take device pointers for everything and a workspace -- trpl_posterior_workspace_bytes(1) bytes for the
 * weights, trpl_posterior_tf_scan_lr_workspace(S, D, K) bytes (0 for arguments the scan refuses) for the scan; they allocate
 * nothing, never synchronise and can be captured in a HIP graph.
 * ------------------------------------------------------------------------------------- */
int trpl_posterior_weights_lr(const double *LL, const double *lnr, int64_t S, double tf, double *W, double *stats /*nullable [2]*/,
                              int32_t device, double *seconds);
int trpl_posterior_weights_lr_dev(const double *LL, const double *lnr, int64_t S, double tf, double *W, double *stats,
                                  void *workspace, int64_t workspace_bytes, void *stream);
int64_t trpl_posterior_tf_scan_lr_workspace(int64_t S, int32_t D, int32_t K);
int trpl_posterior_tf_scan_lr(const double *LL, const double *lnr, int64_t S, const double *V /*nullable: D == 0*/, int32_t D,
                              const double *tfs, int32_t K, double *stats, double *mean, double *var, double *Q, int32_t device,
                              double *seconds);
int trpl_posterior_tf_scan_lr_dev(const double *LL, const double *lnr, int64_t S, const double *V, int32_t D, const double *tfs,
                                  int32_t K, double *stats, double *mean, double *var, double *Q, void *workspace,
                                  int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * trpl_predictive* -- the posterior-predictive PL band: the posterior taken back to the DATA.  Which PL(t) does the posterior
 * predict, and how wide is that prediction next to the measured curve (the check a user of the reference does by hand in NumPy
 * on a PL matrix copied to the host).  A streaming reduction over the samples, per time column, of a PL block resident in HBM
 * (the output of trpl_solve_pl_dev) under the weights of trpl_posterior_weights_dev.
 *
 * Definition.  For row j (one sample of one curve) and column i < ncol the model value is
 *     y[j][i] = log10 PL[j][i] + mag[j]                                     (mag == NULL: 0)
 * formed EXACTLY as the on-grid path of trpl_loglik_from_pl_dev forms the value it subtracts the observation from: the same
 * optional fp32 rounding (TRPL_FLAG_PL_F32, implied by a 4-byte buffer), the same optional self-normalisation to column 0
 * (TRPL_FLAG_NORMALIZE), the same clamp at DBL_MIN, the same device function (csrc/log_pl.hpp).
 * A row is USED iff W[j] is finite and > 0 and (status == NULL or status[j] == 0).  Over the used rows, per column,
 *     sw = sum W_j,   mean = sum W_j y_ji / sw,   var = sum W_j (y_ji - mean)^2 / sw,   lo = min y_ji,   hi = max y_ji.
 * An unused row's PL is never read.  A column no used row reached finishes as sw = 0, mean = var = NaN, lo = +inf, hi = -inf.
 * NaN rule: a NaN PL element in a used row makes that column's mean and var NaN; lo and hi ignore it (fmin / fmax).  The same
 * holds for a y that is infinite -- PL <= 0 in a 4-byte buffer, whose clamp (float)DBL_MIN is 0 exactly as in
 * trpl_log10_clamp, gives y = -inf: mean and var of that column are NaN, and lo is -inf.
 *
 * State and passes.  state [5][ncol] fp64 = running (sw, mean, M2 = sum W (y - mean)^2, lo, hi) per column
 * (trpl_predictive_state_bytes = 40 ncol).  trpl_predictive_init_dev sets sw = 0, lo = +inf, hi = -inf;
 * trpl_predictive_accumulate_dev adds the used rows of one block -- any number of calls, e.g. one per solved block;
 * trpl_predictive_finish_dev writes out [5][ncol] = mean, var, lo, hi, sw and leaves the state as it is.  One accumulation:
 * the rows are cut into trpl_predictive_chunks(rows, ncol, elem_bytes) chunks of ceil(rows / chunks) consecutive rows; every
 * chunk accumulates its columns in row order with the weighted one-pass update (West 1979) and writes its partials to the
 * workspace (chunks * ncol * 40 B = trpl_predictive_workspace_bytes; 0 for refused arguments); a second kernel merges the
 * chunks IN CHUNK ORDER with the pairwise formula of Chan, Golub and LeVeque, then the call's result into the state.
 * Determinism: no atomics; the chunking is a pure function of (rows, ncol, elem_bytes) and never of the device, so the same
 * sequence of calls gives the same bits on any device, and the host form equals init + one accumulate + finish bit for bit.
 * A different cut of the rows into calls is a different (equally accurate) summation order.  Against a two-pass
 * extended-precision evaluation on the same y: mean within 1e-12 sum W |y| / sw, var within 1e-10 var; one used row, or a
 * constant column, gives mean = y and var = 0 exactly; lo and hi are the exact minimum and maximum.
 * Any ld >= ncol: rows need only element alignment (trpl_solve_pl_dev's ld = T/plT + 1 is usually odd).
 *
 * Refused with TRPL_ERR_ARG before a device is touched, the message naming the argument: rows < 1; ncol < 1 (or > 2^36);
 * ld < ncol; elem_bytes other than 4 or 8; a NULL plI, W, state, workspace or out; a workspace smaller than
 * trpl_predictive_workspace_bytes returns; flags other than TRPL_FLAG_PL_F32 / TRPL_FLAG_NORMALIZE.
 * The _dev calls take device pointers only (mag and status nullable), allocate nothing and never synchronise.
 * trpl_predictive is the host-buffer form: init, one accumulate, finish; seconds (nullable) the time of the three on the device.
 * Python: trpl_amd.predictive.band / merge / posterior_predictive, trpl_amd.device.predictive_*.
 * ------------------------------------------------------------------------------------- */
int64_t trpl_predictive_state_bytes(int64_t ncol);
int64_t trpl_predictive_workspace_bytes(int64_t rows, int64_t ncol, int32_t elem_bytes);
int32_t trpl_predictive_chunks(int64_t rows, int64_t ncol, int32_t elem_bytes);
int trpl_predictive_init_dev(void *state, int64_t ncol, void *stream);
int trpl_predictive_accumulate_dev(const void *plI, int32_t elem_bytes, int64_t rows, int64_t ncol, int64_t ld,
                                   const double *mag, const double *W, const int32_t *status, uint32_t flags,
                                   void *state, void *workspace, int64_t workspace_bytes, void *stream);
int trpl_predictive_finish_dev(const void *state, int64_t ncol, double *out /* [5][ncol]: mean, var, lo, hi, sw */,
                               void *stream);
int trpl_predictive(const void *plI, int32_t elem_bytes, int64_t rows, int64_t ncol, int64_t ld, const double *mag,
                    const double *W, const int32_t *status, uint32_t flags, double *out, int32_t device, double *seconds);

/* ---------------------------------------------------------------------------------------
 * trpl_weighted_quantiles* -- weighted quantiles of many columns that share one weight vector: the credible interval of
 * every parameter in one call (utils.py:185-196 is one column per call on the host), and, after trpl_predictive_gather_dev,
 * the median and the 2.5 % / 97.5 % band of the posterior-predictive PL -- under weights that span 20 decades mean +- sd is
 * no interval and the envelope is set by samples of weight 1e-300.  (csrc/quantiles.hip)
 *
 * Inputs.  Keys Y[ncols][ldy] fp64, the n keys of column c contiguous at Y + c * ldy (ldy >= n); weights Wq[n], shared by
 * all columns; K <= TRPL_Q_MAX requests (q[k], rule[k]), HOST arrays in both forms.  Output out[K][ncols].
 * Used rows.  Row j is used iff Wq[j] is finite and > 0.  An unused row's key is never looked at, NaN included.
 * Cumulative sum.  S_c(v) = the sum of Wq[j] over the used rows of column c with key <= v, formed in ONE fixed order that
 * is a pure function of n: thread t of a workgroup of TRPL_Q_BLOCK threads adds rows t, t + B, t + 2B, ... in that order;
 * then a fixed tree over the 64 lanes of a wave (lane l += lane l + 32, + 16, ... + 1); then the waves in wave order.
 * sw = S_c(+inf).  Floating-point addition is monotone in each operand, so this sum is non-decreasing in v and the selection
 * below is well defined.  Keys equal as numbers form one point carrying their total weight; -0.0 and +0.0 are equal as
 * numbers (either may be returned: == on a returned key is the test).
 * Rules.  TRPL_Q_FIRST_ABOVE: the smallest key with S_c(v) > q * sw.  TRPL_Q_LAST_BELOW: the largest key with
 * S_c(v) < q * sw; if there is none the result is NaN (the reference raises IndexError there).  On tie-free keys with
 * weights that sum to 1 these are credible_interval's X_high and X_low, up to the rounding of the sum.  q * sw is one fp64
 * product.  (FIRST_ABOVE is NaN as well in the one case where no key qualifies: a subnormal sw with q * sw rounding to sw.)
 * NaN rule.  A NaN key in a used row makes every quantile of that column NaN, as trpl_predictive* does for mean and variance.
 * +-inf keys order like numbers.  sw = 0 (no used row) gives NaN everywhere, and so does a sw that overflowed.
 * Determinism.  No atomics; nothing depends on scheduling or on the device: the same call gives the same bits.  Columns of
 * n <= trpl_quantiles_stage_rows() rows are held in LDS (two workgroups per compute unit fit), longer ones are streamed from
 * memory in every pass; TRPL_Q_FORCE_STREAM (tests) takes the streamed form at any n.  Both give the same bits.
 * Method.  Bisection on the order-preserving 64-bit image of the key, all K requests per pass, starting from the column's
 * smallest and largest used key: at most 64 passes over the column, plus one for a LAST_BELOW request.
 *
 * trpl_predictive_gather_dev fills the store from a resident PL block, beside trpl_predictive_accumulate_dev and with its
 * arguments: Y[i][row0 + j] = y[j][i] of trpl_predictive* (the same device function, TRPL_FLAG_NORMALIZE / TRPL_FLAG_PL_F32)
 * for i < ncol, j < rows, and Wq[row0 + j] = W[j] if W[j] is finite and > 0 and (status == NULL or status[j] == 0), else 0.
 * Every row is written (an unused row's y may be anything; its weight 0 keeps it out).  Any ld >= ncol, rows need only
 * element alignment.  mag and status are nullable.
 *
 * Refused with TRPL_ERR_ARG before a device is touched, the message naming the argument: a NULL Y, Wq, q, rule, out, plI or
 * W; ncols < 1, n < 1, ldy < n; K outside 1 .. TRPL_Q_MAX; a q outside (0, 1) or NaN; an unknown rule or flag; elem_bytes
 * other than 4 or 8; rows < 1, ncol < 1, ld < ncol; row0 < 0 or row0 + rows > ldy.
 * The _dev calls take device pointers (q and rule excepted), allocate nothing and never synchronise.
 * trpl_weighted_quantiles is the host-buffer form; seconds (nullable) is the time of the selection on the device.
 * Python: trpl_amd.posterior.quantiles / credible_intervals, trpl_amd.predictive.band_quantiles /
 * posterior_predictive(quantiles=...), trpl_amd.device.weighted_quantiles_device / predictive_gather_device.
 * ------------------------------------------------------------------------------------- */
#define TRPL_Q_MAX 8
#define TRPL_Q_BLOCK 256
#define TRPL_Q_FIRST_ABOVE 1
#define TRPL_Q_LAST_BELOW 2
#define TRPL_Q_FORCE_STREAM 0x1
int64_t trpl_quantiles_stage_rows(void);
int trpl_weighted_quantiles_dev(const double *Y, int64_t ncols, int64_t n, int64_t ldy, const double *Wq, const double *q,
                                const int32_t *rule, int32_t K, uint32_t flags, double *out /* [K][ncols] */, void *stream);
int trpl_weighted_quantiles(const double *Y, int64_t ncols, int64_t n, int64_t ldy, const double *Wq, const double *q,
                            const int32_t *rule, int32_t K, uint32_t flags, double *out, int32_t device, double *seconds);
int trpl_predictive_gather_dev(const void *plI, int32_t elem_bytes, int64_t rows, int64_t ncol, int64_t ld, const double *mag,
                               const double *W, const int32_t *status, uint32_t flags, double *Y, int64_t ldy, int64_t row0,
                               double *Wq, void *stream);

/* ---------------------------------------------------------------------------------------
 * trpl_convolve_irf* -- the instrument response in the model: a measured TRPL decay is PL(t) convolved with the response
 * function (IRF) of the detection chain.  The reference compares the bare PL(t) and sidesteps the IRF by cutting the data after
 * its peak; this call maps a PL block resident in HBM (the output of trpl_solve_pl_dev) to the block the detector saw, which
 * every consumer of a resident PL block -- trpl_loglik[_moments|_weighted]_from_pl_dev, trpl_predictive_*,
 * trpl_predictive_gather_dev -- then takes unchanged.  (csrc/irf.hip)
 *
 * Definition.  pl [rows][ld] fp32 / fp64 (elem_bytes) as trpl_solve_pl_dev wrote it, ncol valid columns on a uniform time grid;
 * h[0 .. K-1] the IRF samples at that grid's spacing; k0 the index of the tap that sits at time zero, normally the peak.  The
 * output has ncol_out = ncol - k0 valid columns, in the input's element type:
 *     out[r][j] = sum over k = 0 .. K-1, ascending, of  h[k] * (double)pl[r][j + k0 - k]          0 <= j < ncol_out
 *   - a term whose column j + k0 - k is negative is skipped, not added as zero: there is no PL before the excitation;
 *   - no column index exceeds ncol - 1: the last k0 columns are not produced, their sums would need PL past the solved window;
 *   - the accumulator is fp64 and starts at +0.0; each term is one rounded product followed by one rounded addition, never a
 *     fused multiply-add; a 4-byte output is the fp64 sum rounded once.
 * The result is therefore, bit for bit, the NumPy loop  for k: acc[:, lo:hi] += h[k] * pl64[:, lo + k0 - k : hi + k0 - k]
 * (lo = max(0, k - k0), hi = ncol_out), the same on every run and every device: no atomics, every output is one thread's own sum.
 * NaN and inf follow IEEE through that expression: a NaN element poisons exactly the output columns whose window covers it,
 * and 0 * NaN is NaN.  Bytes of out beyond ncol_out in a row are not written.  Any ld >= ncol and out_ld >= ncol_out: rows need
 * only element alignment.
 * Work.  A workgroup convolves a tile of TRPL_IRF_TILE_ROWS rows x TRPL_IRF_TILE_COLS output columns from one staged copy of
 * the TRPL_IRF_TILE_COLS + K - 1 input columns it reads; the grid holds at most TRPL_IRF_GRID_CAP workgroups, which walk the
 * tiles.  None of this enters the result.
 *
 * Refused with TRPL_ERR_ARG before a device is touched, the message naming the argument: elem_bytes other than 4 or 8;
 * rows < 0; ncol < 1; ld < ncol; K < 1 or K > TRPL_IRF_MAX_TAPS (at the reference's 0.25 ns steps a 256 ns response); k0 outside
 * [0, K - 1]; ncol - k0 < 1; out_ld < ncol - k0; with rows > 0 a NULL pl, h or out, and out == pl; in the host-buffer form
 * also a tap that is not finite (its index is named).  rows == 0 is TRPL_OK without a launch.
 * The _dev call takes device pointers only, allocates nothing and never synchronises.  trpl_convolve_irf is the host-buffer
 * form (pl, h and out on the host); seconds (nullable) is the time of the kernel on the device.  The count of the cap:
 * trpl_irf_max_taps.
 * Python: trpl_amd.irf.gaussian / from_samples / convolve / loglik, trpl_amd.device.convolve_irf_device,
 * gpu_info["irf"] of simulate / bayes, posterior_predictive(irf=...).
 * ------------------------------------------------------------------------------------- */
#define TRPL_IRF_MAX_TAPS 1024
#define TRPL_IRF_TILE_COLS 512
#define TRPL_IRF_TILE_ROWS 4
#define TRPL_IRF_GRID_CAP 65536
int trpl_irf_max_taps(void);
int trpl_convolve_irf_dev(const void *pl, int32_t elem_bytes, int64_t rows, int64_t ncol, int64_t ld,
                          const double *h /*device [K]*/, int32_t K, int32_t k0, void *out, int64_t out_ld, void *stream);
int trpl_convolve_irf(const void *pl, int32_t elem_bytes, int64_t rows, int64_t ncol, int64_t ld, const double *h, int32_t K,
                      int32_t k0, void *out, int64_t out_ld, int32_t device, double *seconds);

/* ---------------------------------------------------------------------------------------
 * trpl_loglik_irf_bank* -- the likelihood of a resident PL block against a BANK of J candidate instrument responses, from one
 * solve and one call.  The arrival time of the excitation is not known to a fraction of a grid step and the width of the
 * response only to some tens of per cent: both are nuisance parameters that do not enter the solve, like the magnitude offset
 * of trpl_mag_grid.  A bank is H [J][K] fp64: J responses of ONE length K and ONE index k0 of the tap at time zero -- a shift
 * lives in the taps of a row, zero-padded to the common length, so that all J responses read the same window of PL.
 * (csrc/irf_bank.hip)
 *
 * Definition.  For every j < J and every row, sse[j][row] and esum[j][row] (both [J][rows]; esum nullable) are, bit for bit,
 * what these two calls produce for that row:
 *     trpl_convolve_irf_dev(pl, elem_bytes, rows, ncol, ld, H + j K, K, k0, cv, ncol - k0, stream)
 *     trpl_loglik_moments_from_pl_dev(cv, elem_bytes, rows, ncol - k0, ncol - k0, obs, obs_hi, obs_dx, obs_h, n_obs, mag, status,
 *                                     NULL, sse + j rows, esum + j rows, flags, stream)
 * (trpl_loglik_weighted_from_pl_dev with wts [n_obs] when wts is given).  That fixes the convolved value (fp64 accumulator from
 * +0.0, ascending k, one rounded product and one rounded addition per term, a term left of column 0 skipped, a 4-byte block
 * rounds the sum to float before the logarithm), the error (y + mag - obs with y = log10 max(cv, DBL_MIN), through fp32 under
 * TRPL_FLAG_PL_F32 or a 4-byte block; off the grid ((y_hi - y_lo) / obs_h) * obs_dx + y_lo on the convolved columns obs_hi - 1
 * and obs_hi), the association of the sums (a 256-thread workgroup per row: thread t adds observations t, t + 256, ... in
 * ascending order, an xor butterfly inside each 64-lane wave, then ((p0 + p1) + p2) + p3) and the flagged-row rule (status != 0
 * or a NaN sum: sse = +inf, esum = NaN).  obs_hi [n_obs] in [1, ncol - k0 - 1], in ANY order.  The convolved block is never
 * written: the kernel convolves at the observed columns only, TRPL_IRF_BANK_BLOCK responses per pass over the taps.  None of
 * the blocking enters the result.
 *
 * Refused with TRPL_ERR_ARG before a device is touched, the message naming the argument, in this order: elem_bytes other than
 * 4 or 8; rows < 0 or > 2^31 - 1; ncol < 1 or > 2^31 - 1; ld < ncol; K < 1 or K > TRPL_IRF_MAX_TAPS; k0 outside [0, K - 1];
 * ncol - k0 < 1; J < 1 or J > TRPL_IRF_BANK_MAX_RESPONSES; n_obs < 1; obs_hi, obs_dx and obs_h not all NULL or all non-NULL;
 * on the grid n_obs > ncol - k0; off the grid ncol - k0 < 2; TRPL_FLAG_NORMALIZE (the convolved curve's first column is a
 * fraction of the response's area, not PL(0)); any other flag than TRPL_FLAG_PL_F32; with rows > 0 a NULL pl, H, obs, mag or
 * sse.  rows == 0 is TRPL_OK without a launch.  The host-buffer form (every array on the host; seconds, nullable, the kernel's
 * time) then also refuses a tap that is not finite, a weight that is not finite and >= 0, and an obs_hi outside
 * [1, ncol - k0 - 1], each with its index.  The _dev call takes device pointers only, allocates nothing and never synchronises;
 * there the caller owns those three.
 *
 * trpl_irf_bank_profile* -- the profile over the bank: Pbank [J][S] -> P[s] = the greatest Pbank[j][s], best[s] (int32) = the
 * first j that attains it; a NaN is never the greatest, and where every value is -inf or NaN best = -1 and P = -inf.  The host
 * form is PLAIN HOST CODE (no device, like trpl_mag_profile); the _dev kernel (one thread per sample) equals it bit for bit.
 * Refused: J outside [1, TRPL_IRF_BANK_MAX_RESPONSES]; S < 0; with S > 0 a NULL Pbank, best or P.  S == 0 is TRPL_OK.
 *
 * What follows the moments -- the marginal (log-sum-exp) over the bank, the composition with the magnitude offset, and
 * gpu_info["irf_bank"] inside simulate / bayes -- is trpl_nuisance_reduce*, below.
 * Out of scope: multi-device forms; a bank inside the fused steppers; a response chosen per curve.
 * Python: trpl_amd.irf.gaussian_bank / shift_bank / loglik_bank / loglik_profile, trpl_amd.device.loglik_irf_bank_device /
 * irf_bank_profile_device.
 * ------------------------------------------------------------------------------------- */
#define TRPL_IRF_BANK_MAX_RESPONSES 256
#define TRPL_IRF_BANK_BLOCK 8
int trpl_irf_bank_max_responses(void);
int trpl_irf_bank_block(void);
int trpl_loglik_irf_bank_dev(const void *pl, int32_t elem_bytes, int64_t rows, int64_t ncol, int64_t ld,
                             const double *H /*device [J][K]*/, int32_t J, int32_t K, int32_t k0, const double *obs,
                             const int32_t *obs_hi, const double *obs_dx, const double *obs_h, int64_t n_obs,
                             const double *wts /*nullable*/, const double *mag, const int32_t *status /*nullable*/,
                             double *sse /*[J][rows]*/, double *esum /*[J][rows], nullable*/, uint32_t flags, void *stream);
int trpl_loglik_irf_bank(const void *pl, int32_t elem_bytes, int64_t rows, int64_t ncol, int64_t ld, const double *H, int32_t J,
                         int32_t K, int32_t k0, const double *obs, const int32_t *obs_hi, const double *obs_dx,
                         const double *obs_h, int64_t n_obs, const double *wts, const double *mag, const int32_t *status,
                         double *sse, double *esum, uint32_t flags, int32_t device, double *seconds);
int trpl_irf_bank_profile_dev(const double *Pbank /*[J][S]*/, int32_t J, int64_t S, int32_t *best /*[S]*/, double *P /*[S]*/,
                              void *stream);
int trpl_irf_bank_profile(const double *Pbank, int32_t J, int64_t S, int32_t *best, double *P);

/* ---------------------------------------------------------------------------------------
 * trpl_nuisance_reduce* -- one reduction over the nuisance grid of an experiment: the J responses of a bank x M magnitude
 * offsets, from the moments trpl_loglik_irf_bank* left in HBM.  sse, esum [C][J][S] fp64 (curve-major: curve c holds the [J][S]
 * block one trpl_loglik_irf_bank_dev wrote for it); wsum [C] HOST fp64, the quadratic coefficient of curve c: (double)n_obs[c], or
 * the sum of the curve's weights, as trpl_mag_*_w take it; offsets [M] HOST fp64; P [S] fp64, WRITTEN, not accumulated; best [S]
 * int32 (nullable), the first cell i = j M + m that attains the maximum; best_mag [S] fp64 (nullable), the offset at that cell.
 * (csrc/nuisance.hip)
 *
 * The value of a cell, v[j][m].  Curves in ascending c, every operation rounded once, no fused multiply-add.  flags holds one
 * mag mode:
 *   TRPL_NUISANCE_MAG_FIXED    M = 1, no offsets, esum nullable:  v[j] = +0.0 - (((+0.0 + sse_0) + sse_1) + ...).  That is
 *       -(sum) in every bit but the sign of a zero total, which is +0.0: row j of the P (J, S) that P -= sse_c from zeros gives
 *       (irf.loglik_bank), bit for bit.  FIXED with the maximum is trpl_irf_bank_profile on that P, in P and best; best_mag = +0.0.
 *   TRPL_NUISANCE_MAG_GRID     1 <= M <= TRPL_NUISANCE_MAX_OFFSETS:  v[j][m] = +0.0 - sum_c t_c from +0.0, with d = offsets[m] and
 *       t_c = (sse_c + (2.0 d) esum_c) + wsum_c (d d), clamped from below at 0.0; t_c = +inf where sse_c is +inf or NaN, esum_c is
 *       not finite, or the expression is NaN (trpl_mag_grid_w's term and rule: such a cell is -inf).  With J = 1, v[0][m] is row
 *       m of trpl_mag_grid_w on a P started from +0.0, bit for bit.
 *   TRPL_NUISANCE_MAG_PROFILE  M = 1, no offsets:  per response j, E = sum_c esum_c and N = sum_c wsum_c from +0.0, d_j =
 *       (0.0 - E) / N, v[j] = +0.0 - sum_c t_c(d_j) as above; the offset reported is d_j where every sse_c < +inf and E is
 *       finite, else NaN.  Where N == 0 and every sse_c < +inf there is nothing to fit: v[j] = +0.0, d_j = NaN.  That is best and
 *       P of trpl_mag_profile_w (flags 0, P started from +0.0) on the slice sse[:][j][:], esum[:][j][:], bit for bit.
 *       best_mag = d_j of the winning response.
 *
 * The reduction, over the cells in ascending i = j M + m:
 *   the maximum (default)    P[s] = the greatest v, best = the first cell that attains it.  A NaN is never the greatest; where every
 *       cell is -inf or NaN: P = -inf, best = -1, best_mag = NaN (trpl_irf_bank_profile's rules).
 *   TRPL_NUISANCE_MARGINAL   a_i = v_i / tf + logw_i (one division, one addition; logw NULL: + 0.0).  Pass 1: mx = the greatest a
 *       and best, a NaN a counting as -inf.  Pass 2: sum = sum_i exp(a_i - mx) from +0.0 in ascending i, a NaN term skipped.
 *       P = tf * (mx + log(sum)).  Everything -inf or NaN: as above.  exp(P / tf) = sum_i w_i exp(v_i / tf), w_i = exp(logw_i): the
 *       log of the marginal of the tempered joint posterior over the cells, at ONE tf.  logw [J M] fp64: -inf excludes a cell.
 *
 * Host and device.  trpl_nuisance_reduce is PLAIN HOST CODE (no device, like trpl_mag_profile), every pointer a host pointer.
 * trpl_nuisance_reduce_dev takes device pointers for sse, esum, P, best, best_mag and logw, host pointers for wsum and offsets
 * (they travel as kernel arguments), allocates nothing and never synchronises; one thread per sample, no atomics, LDS or
 * scratch.  logw is a device array there because J M doubles (up to 128 KiB) do not fit kernel arguments; its values are the
 * caller's to vouch for, as the taps of trpl_loglik_irf_bank_dev are.  With the maximum the kernel equals the host form bit for bit
 * in P, best and best_mag.  With the marginal best is equal (a_i is IEEE division and addition on both sides) and P obeys a bound,
 * because exp and log are the device library's there and libm's here.
 *
 * The bound of the marginal.  Let A_i = v_i / tf + logw_i and R = tf (MX + ln sum_i exp(A_i - MX)) in exact arithmetic from the fp64
 * cell values, n = J M, u = 2^-53, B = the greatest |v_i| / tf + |logw_i| over the cells with a finite a_i.
 *   a_i carries two roundings: |a_i - A_i| <= u |v_i| / tf + u |a_i| <= (2 + u) u B.  ln-sum-exp moves by at most the greatest
 *       change of an argument, so this costs at most 3 u B in R / tf.
 *   t_i = a_i - mx carries one rounding, u |t_i|, and a term contributes only for |t_i| <= 745; relative to the sum, which is at
 *       least its greatest term 1, the terms exp(t_i) |t_i| <= 1 / e each: at most (n - 1) u / e.
 *   exp and log are 1 ulp each in the ROCm device library's table of double-precision functions: a relative 2 u per term of the
 *       sum, and 2 u ln(sum) <= 2 u ln(n) < 20 u for n <= 16384.
 *   the n - 1 additions of terms in (0, 1]: a relative (n - 1) u of the sum; terms below exp(-745) that vanish: below u in all.
 *   one addition and one product: 2 u |R|.
 * In sum |P - R| <= TRPL_NUISANCE_BOUND: u (tf (3 B + 2 n + 24) + 3 |R|), the constants 1 + 1 / e, 22 and 2 rounded up to cover the
 * second-order terms.  The host form obeys the same bound (libm's exp and log are below 1 ulp).
 *
 * Refused with TRPL_ERR_ARG before a device is touched, the message naming the argument, in this order: S < 0; C outside
 * [1, TRPL_MAG_MAX_CURVES]; J outside [1, TRPL_IRF_BANK_MAX_RESPONSES]; an unknown mag mode or flag bit; M outside
 * [1, TRPL_NUISANCE_MAX_OFFSETS] in grid mode, M != 1 otherwise; offsets NULL in grid mode, non-NULL otherwise; esum NULL unless
 * FIXED; a wsum that is not finite and >= 0; an offset that is not finite; with the marginal, tf not finite or not > 0, and (host
 * form) a logw entry that is NaN or +inf; without the marginal, logw non-NULL; with S > 0 a NULL sse, wsum or P.  S == 0 is
 * TRPL_OK without a launch.
 *
 * Out of scope: multi-device forms; an analytic marginal over the offset; per-cell posterior shares as an output; a marginal
 * across the rungs of a tempered run (the rungs differ in tf).
 * Python: trpl_amd.device.nuisance_reduce_device, trpl_amd.irf.loglik_nuisance, gpu_info["irf_bank"] of driver.simulate / bayes.
 * ------------------------------------------------------------------------------------- */
#define TRPL_NUISANCE_MAX_OFFSETS 64
#define TRPL_NUISANCE_MAG_FIXED 0x0u
#define TRPL_NUISANCE_MAG_GRID 0x1u
#define TRPL_NUISANCE_MAG_PROFILE 0x2u
#define TRPL_NUISANCE_MAG_MASK 0x3u
#define TRPL_NUISANCE_MARGINAL 0x10u
/* the bound above: tf, B = max_i (|v_i| / tf + |logw_i|), n = J M, R the exact value */
#define TRPL_NUISANCE_BOUND(tf, B, n, R) \
    (1.1102230246251565e-16 * ((tf) * (3.0 * (B) + 2.0 * (double)(n) + 24.0) + 3.0 * ((R) < 0 ? -(R) : (R))))
int trpl_nuisance_max_offsets(void);
double trpl_nuisance_bound(double tf, double B, int32_t n, double R);   /* TRPL_NUISANCE_BOUND, for callers that cannot read a macro */
int trpl_nuisance_reduce_dev(const double *sse /*[C][J][S]*/, const double *esum /*[C][J][S]*/, const double *wsum /*HOST [C]*/,
                             int64_t S, int32_t C, int32_t J, const double *offsets /*HOST [M]*/, int32_t M,
                             const double *logw /*device [J M], nullable*/, double tf, uint32_t flags, double *P /*[S]*/,
                             int32_t *best /*[S], nullable*/, double *best_mag /*[S], nullable*/, void *stream);
int trpl_nuisance_reduce(const double *sse, const double *esum, const double *wsum, int64_t S, int32_t C, int32_t J,
                         const double *offsets, int32_t M, const double *logw /*HOST [J M], nullable*/, double tf, uint32_t flags,
                         double *P, int32_t *best, double *best_mag);

/* ---------------------------------------------------------------------------------------
 * trpl_corner* -- the corner: every posterior marginal of a finished run in one device call.  What plot() of
 * Visualization/marginalization_visual.py:500-609 does after loading a run: drop the samples outside the axis limits
 * (utils.py:48-52, :145-155), add the secondary parameters (utils.py:54-79, secondary_parameters.py), take log10 of the
 * log-scaled columns, temper and normalise, fill one 1-D histogram per enabled parameter and one 2-D histogram per pair
 * (utils.py:91-117, :239-285 -- the reference's only process pool).  (csrc/corner.hip)
 *
 * Column codes.  0 .. 12 are the 13 columns of the exported X (*_BAYRAN_X.npy, the user's units) in the reference's PARAM_ORDER
 * (marginalization_visual.py:67-70); 13 .. 18 the six secondary parameters in that list's order.
 *
 * trpl_corner_columns_dev: one pass over the samples, each X row (S rows of ldx >= 13 doubles) read once.  V[d][s] (V is [D][S],
 * the layout trpl_posterior_moments and trpl_weighted_quantiles take) is the value of cols[d], its log10 where dolog[d] != 0.
 * cols and dolog are HOST arrays.  Secondary columns follow secondary_parameters.py:9-57, evaluated left to right in IEEE fp64
 * with x**-1 = 1.0 / x and p0**2 = p0 * p0 (what NumPy does for those exponents):
 *     tau_rad = 1 / (B p0) * 1e9;  t_aug = 1 / (Cp p0^2) * 1e9;  mu' = 2 / (1 / mu_n + 1 / mu_p);
 *     Dif = mu' * 0.0257 / 1 * 1e14 / 1e9;  tau_surf = thickness / ((Sf + Sb) * 0.01) + thickness^2 / (pi^2 Dif);
 *     tau_eff = 1 / (1 / tau_rad + 1 / t_aug + 1 / tau_surf + 1 / tau_n);  S_F+S_B, epsilon = 1 / lambda, tau_n + tau_p.
 * The reference's own CALL of LI_tau_eff is broken: utils.py:61-62 passes seven arguments to a function of eight and leaves out
 * CP.  This is the function as DEFINED (secondary_parameters.py:17-30), with CP = X[:, 8].
 * Exclusion (excl_lo, excl_hi: HOST arrays of 13, both or neither).  Sample s is kept iff for every primary column c with a
 * non-NaN excl_lo[c]:  excl_lo[c] <= X[s][c] <= excl_hi[c], on the RAW value -- a NaN value excludes the sample, as in
 * utils.py:149-150; a NaN excl_lo[c] means column c is not tested.  LLk[s] (nullable; needs LL) = LL[s] for a kept sample, else
 * NaN: filter_nan's marker, which trpl_posterior_weights_dev passes through, so trpl_posterior_weights_dev(LLk) normalises over
 * the kept samples only (the reference excludes first, :520-523, and normalises afterwards, :589-591).  V is written for
 * every sample.  kept (nullable, device int64) receives the number of samples that pass the exclusion and whose LL (when
 * given) is not NaN: the reference's "Kept" after filter_nan and exclude.
 *
 * trpl_corner_hist_dev: V [D][ldv >= S], weights W[S], limits lo[D], hi[D] (HOST arrays), `bins` <= TRPL_CORNER_MAX_BINS equal
 * bins per axis (128^2 fp64 bins are 128 KiB of the 160 KiB one workgroup may declare on gfx950; the GUI's default is 96).
 * Outputs: h1[D][bins] weighted sums, c1[D][bins] (nullable) plain counts as doubles, h2[D (D - 1) / 2][bins][bins] (nullable)
 * with pair p in the reference's order (utils.py:103-106): for i = 1 .. D-1, for j = 0 .. i-1: x = column j, y = column i,
 * h2[p][x bin][y bin].  Every element is written (no zeroing by the caller).  Bins follow trpl_posterior_hist's rules: edges
 * lo + (hi - lo) * k / bins exactly as the reference builds them, left-closed, the last closed on the right -- at the COMPUTED
 * last edge, not hi --, outside and NaN dropped.  A sample enters the weighted sums iff its weight is finite and > 0
 * (trpl_weighted_quantiles' rule) and the plain counts iff its weight is not NaN (it survived filter_nan and the exclusion):
 * c1 is what marginalize_1D divides by for secondary parameters and mobilities (:248-257).
 * ORDER, and therefore bits: every weighted bin is the fp64 sum of its samples' weights added ONE AT A TIME IN ASCENDING SAMPLE
 * INDEX, starting from +0.0 -- numpy.add.at(out, key, w) on the host.  A pure function of the inputs: it does not depend on the
 * grid, the device or the run.  No floating-point atomics.  (trpl_posterior_hist's sums are fp64 atomics in no fixed order.)
 * workspace: trpl_corner_workspace_bytes(S, D) bytes of device memory (one key byte per sample and column; 0 for refused S, D).
 *
 * trpl_corner is the host-buffer form: stages X and LL, runs the columns, trpl_posterior_weights_dev on LLk at temperature tf,
 * then the histograms.  Returns V [D][S] (nullable), W [S] (nullable), kept (nullable), h1, c1 (nullable), h2 (nullable);
 * seconds (nullable) is the time of the three steps on the device.
 * W is trpl_posterior_weights_dev of the MARKED full-length vector, bit for bit.  Against dropping the samples first and normalising
 * the kept ones (the reference's order) it is the same number, not the same bits: the weight's exponent is lifted by ln S of the
 * full length instead of ln kept, so exp sees another argument, and the normalising sum groups its terms by another grid; both
 * lie within 16 ulp of an extended-precision evaluation at S <= 2048.
 *
 * Refused with TRPL_ERR_ARG before a device is touched, the message naming the argument: S < 0; D outside
 * [1, TRPL_CORNER_MAX_COLS]; a column code outside [0, 18]; bins outside [1, TRPL_CORNER_MAX_BINS]; a lo or hi that is not finite,
 * or hi <= lo; thickness_nm not finite and > 0 while tau_eff is requested; only one of excl_lo / excl_hi; a NaN excl_hi[c]
 * beside a non-NaN excl_lo[c] (it would exclude every sample; excl_hi[c] of an untested column is ignored); ldx < 13; ldv < S; a
 * NULL h1, cols, dolog, lo, hi, V, or (S > 0) X, W, workspace; LLk without LL; tf that is not > 0.  S == 0 succeeds and writes
 * zeros.  The _dev calls take device pointers (the host arrays named above excepted), allocate nothing and never synchronise.
 * Python: trpl_amd.posterior.columns / corner / CORNER_COLUMNS, trpl_amd.device.corner_columns_device / corner_hist_device /
 * corner_workspace.
 * ------------------------------------------------------------------------------------- */
#define TRPL_CORNER_PRIMARY 13
#define TRPL_CORNER_MAX_COLS 19
#define TRPL_CORNER_MAX_BINS 128
#define TRPL_COL_N0 0
#define TRPL_COL_P0 1
#define TRPL_COL_MU_N 2
#define TRPL_COL_MU_P 3
#define TRPL_COL_B 4
#define TRPL_COL_SF 5
#define TRPL_COL_SB 6
#define TRPL_COL_CN 7
#define TRPL_COL_CP 8
#define TRPL_COL_TAU_N 9
#define TRPL_COL_TAU_P 10
#define TRPL_COL_LAMBDA 11
#define TRPL_COL_MAG 12
#define TRPL_COL_TAU_EFF 13
#define TRPL_COL_TAU_RAD 14
#define TRPL_COL_S_SUM 15
#define TRPL_COL_MU_EFF 16
#define TRPL_COL_EPSILON 17
#define TRPL_COL_TAU_SUM 18
int64_t trpl_corner_workspace_bytes(int64_t S, int32_t D);
int trpl_corner_columns_dev(const double *X, int64_t S, int64_t ldx, const int32_t *cols /*host [D]*/, const int32_t *dolog /*host [D]*/,
                            int32_t D, double thickness_nm, const double *excl_lo /*host [13], nullable*/,
                            const double *excl_hi /*host [13], nullable*/, const double *LL /*nullable*/, double *V /* [D][S] */,
                            double *LLk /*nullable*/, int64_t *kept /*nullable, device*/, void *stream);
int trpl_corner_hist_dev(const double *V, int64_t S, int64_t ldv, int32_t D, const double *W, const double *lo /*host [D]*/,
                         const double *hi /*host [D]*/, int32_t bins, double *h1 /* [D][bins] */, double *c1 /*nullable*/,
                         double *h2 /*nullable: [D (D - 1) / 2][bins][bins]*/, void *workspace, void *stream);
int trpl_corner(const double *X, int64_t S, int64_t ldx, const double *LL, double tf, const int32_t *cols, const int32_t *dolog,
                int32_t D, double thickness_nm, const double *excl_lo, const double *excl_hi, const double *lo, const double *hi,
                int32_t bins, double *V, double *W, int64_t *kept, double *h1, double *c1, double *h2, int32_t device,
                double *seconds);

/* ---------------------------------------------------------------------------------------
 * trpl_refine_* -- refinement generations: a further generation of samples drawn around the posterior of the ones at hand, and
 * the exact weights of the union.  (The reference's ancestor refined the cells above minP, Legacy/legacy.py:refineGrid; the
 * random sampler that replaced it has no refinement.)  (csrc/refine.hip)
 *
 * Unit coordinates.  A column of the box (lo, hi, do_log, ncol, flags as trpl_sample_box takes them, HOST arrays) is ACTIVE when
 * lo != hi and it is not the target of a TRPL_BOX_EQUAL_* override that is set (columns 2, 6, 8); the A <= TRPL_REFINE_MAX_DIMS
 * active columns, in column order, are the dimensions.  u = (x - lo) / (hi - lo) for a linear column and
 * (log10 x - log10 lo) / (log10 hi - log10 lo) for a log column; the prior is uniform on [0, 1]^A.  log10 of the bounds is the host's.
 * A call whose A is not the box's number of active columns is refused.
 *
 * Proposal of a generation: K parents with boxes [a_kd, b_kd] (a, b are [K][A]), inv_vol[k] = 1 / prod_d (b_kd - a_kd); the
 * generation has n_uniform + K * m children, the first n_uniform uniform in the cube, child n_uniform + j uniform in the box of
 * parent j mod K: the counts are deterministic, so the mixture proportions are exact.  With generation 1 the uniform draw of S1
 * samples, the deterministic-mixture density of ANY sample u of any generation is
 *     r(u) = (S1 + sum_g [n_uniform_g + m_g * B_g(u)]) / S_total,    B_g(u) = sum_k inv_vol_k * 1[a_k <= u <= b_k]  (closed, every d),
 * its weight at temperature tf is exp(LL / tf) / r(u), and LLc = LL - tf * ln r(u) handed to trpl_posterior_weights, _moments,
 * trpl_weighted_quantiles, trpl_corner and the predictive band makes them work unchanged on the concatenated samples.  LLc is
 * valid at the tf it was formed for only; a temperature scan over a refined set keeps ln r(u) beside LL instead
 * (trpl_posterior_weights_lr, trpl_posterior_tf_scan_lr above).
 *
 * trpl_refine_resample: systematic resampling.  W[S] weights (NaN or <= 0 counts as 0; +inf is refused by the host form and
 * undefined in the _dev form), K draws, offset in [0, 1).  idx[k] (int64, non-decreasing) is the smallest i whose inclusive
 * cumulative weight exceeds (k + offset) / K * sw, evaluated left to right in fp64 (a threshold that rounds up to sw is taken as the
 * largest double below sw); stats[3] (nullable) = { sw, sum w^2, sw^2 / sum w^2 }; the squares are summed after scaling by
 * the power of two of the largest weight, so the ratio (the effective sample size) is right where sum w^2 itself leaves fp64's
 * range (weights near 1e-200: sum w^2 is then 0 or subnormal, the ratio is not).  The cumulative weight is formed in ONE order,
 * a pure function of S: chunks of trpl_refine_chunk_rows() rows; in a chunk, thread t of 256 adds its 16 consecutive rows one
 * after the other, the 256 thread totals are added one after the other, and so are the chunk totals; cum[i] = chunk prefix +
 * (thread base + running sum).  Adding non-negative terms in a fixed order is monotone, so cum never decreases and every i is
 * drawn floor(K p_i) or ceil(K p_i) times up to the rounding of cum.  sw == 0 (or S == 0): idx = -1 everywhere, stats = 0.
 * workspace: trpl_refine_workspace_bytes(S) bytes of device memory.
 *
 * trpl_refine_draw: U2 [n_uniform + K m][A] and X2 [..][ncol].  Child n takes Philox4x32-10 (Salmon et al. 2011) with key
 * (seed low word, seed high word) and counter (n low word, n high word, j, generation); call j gives the uniforms of dimensions 2j
 * and 2j + 1: words (x0, x1) -> ((x0 >> 5) * 2^26 + (x1 >> 6)) / 2^53 and (x2, x3) the same way (genrand_res53, the sampler's
 * form).  u = min(b, a + (b - a) * xi) with separate multiply and add (a = 0, b = 1 for the uniform children).  X2 follows
 * trpl_sample_box's expressions: lo + (hi - lo) * u; pow(10, l + (lh - l) * u) with l, lh the log10 of the bounds; fixed columns
 * copied; the overrides applied last.  U2 and the linear columns are pure functions of the arguments; log columns go through the
 * device's pow.  a > b cannot be seen from the host in the _dev form: the children of such a box are all at b.
 *
 * trpl_refine_density: B[s] = B_g(u_s) for U [S][ldu >= A]; the sum over k is taken in ascending k, one fp64 add per member box
 * starting from +0.0: the plain sequential loop, bit for bit, on any device.  A NaN coordinate lies in no box.  Parents are
 * staged through LDS in tiles of trpl_refine_tile_parents().
 *
 * trpl_refine_unit: U [S][A] of existing samples X [S][ldx >= ncol].  It uses the device's log10, so it is not bit-pinned: the
 * membership of a prior-generation sample at a box face may differ from a host computation by a last bit of u (an event of
 * measure zero under the proposal).
 *
 * Refused with TRPL_ERR_ARG before a device is touched, the message naming the argument: a NULL W, idx, a, b, inv_vol, U, B, U2,
 * X2, X, lo, hi, do_log (or workspace); S < 0; K < 1 or K > TRPL_REFINE_MAX_PARENTS; A outside [1, TRPL_REFINE_MAX_DIMS] or not the
 * box's count; m < 0; n_uniform < 0; more than 2^31 - 2 children; offset outside [0, 1) or NaN; ldu < A; ldx < ncol; a +inf weight
 * (host form).  The _dev calls take device pointers (the box arrays excepted), allocate nothing and never synchronise.
 * Python: trpl_amd.refine, trpl_amd.device.refine_*_device.
 * ------------------------------------------------------------------------------------- */
#define TRPL_REFINE_MAX_DIMS 16
#define TRPL_REFINE_MAX_PARENTS 1048576
int64_t trpl_refine_chunk_rows(void);
int64_t trpl_refine_tile_parents(void);
int64_t trpl_refine_workspace_bytes(int64_t S);
int trpl_refine_resample_dev(const double *W, int64_t S, int64_t K, double offset, int64_t *idx, double *stats /*nullable [3]*/,
                             void *workspace, int64_t workspace_bytes, void *stream);
int trpl_refine_resample(const double *W, int64_t S, int64_t K, double offset, int64_t *idx, double *stats /*nullable [3]*/,
                         int32_t device, double *seconds);
int trpl_refine_draw_dev(const double *a, const double *b, int64_t K, int32_t A, int64_t m, int64_t n_uniform, uint64_t seed,
                         uint32_t generation, int32_t ncol, const double *lo /*host*/, const double *hi /*host*/,
                         const int32_t *do_log /*host*/, uint32_t flags, double *U2, double *X2, void *stream);
int trpl_refine_draw(const double *a, const double *b, int64_t K, int32_t A, int64_t m, int64_t n_uniform, uint64_t seed,
                     uint32_t generation, int32_t ncol, const double *lo, const double *hi, const int32_t *do_log, uint32_t flags,
                     double *U2, double *X2, int32_t device, double *seconds);
int trpl_refine_density_dev(const double *U, int64_t S, int64_t ldu, int32_t A, const double *a, const double *b,
                            const double *inv_vol, int64_t K, double *B, void *stream);
int trpl_refine_density(const double *U, int64_t S, int64_t ldu, int32_t A, const double *a, const double *b, const double *inv_vol,
                        int64_t K, double *B, int32_t device, double *seconds);
int trpl_refine_unit_dev(const double *X, int64_t S, int64_t ldx, int32_t ncol, const double *lo /*host*/, const double *hi /*host*/,
                         const int32_t *do_log /*host*/, uint32_t flags, int32_t A, double *U, void *stream);
int trpl_refine_unit(const double *X, int64_t S, int64_t ldx, int32_t ncol, const double *lo, const double *hi, const int32_t *do_log,
                     uint32_t flags, int32_t A, double *U, int32_t device, double *seconds);

/* ---------------------------------------------------------------------------------------
 * trpl_refine_affine, trpl_refine_draw_oriented -- oriented proposals: the boxes of a generation are axis-parallel in WHITENED
 * coordinates z = M (u - c) instead of in u, so that they follow a posterior ridge that lies across the axes (B * p0 = const is a
 * straight line at 45 degrees in the log10 unit coordinates).  (csrc/refine_oriented.hip)
 *
 * Orientation of a generation with A active columns (formed on the host from the device's weighted moments, A <= 16): c the
 * weighted mean of U and Sigma its weighted covariance under the weights the proposal is built from; diagonal floor
 * Sigma_dd >= (S1^(-1/A) / 2)^2 / 3 (the variance of the axis-parallel scheme's floor half-width); shrinkage Sigma_s = (1 - lam)
 * Sigma + lam diag(Sigma), lam = clip((A + 1) / ESS, 0, 1) unless given; L = chol(Sigma_s) lower, M = L^-1 lower, logdet = sum ln
 * L_dd.  Half-widths in z: h_d = sqrt(3) ESS^(-1 / (A + 4)) for every d (a whitened column has deviation 1).  Parent k is
 * z_k = M (u_k - c) with the box [z_k - h, z_k + h], NOT clipped; inv_vol = 1 / (prod_d 2 h_d * exp(logdet)), the same for every
 * parent, is the density in u.
 *
 * Arithmetic, bit-pinned: z_i = sum_{j <= i} M_ij * (u_j - c_j) and u_i = c_i + sum_{j <= i} L_ij * z_j, j ascending from +0.0:
 * subtract, multiply, add, no contraction.  Only the lower triangles (j <= i) of the host matrices M and L ([A][A] row-major) are
 * read.
 *
 * trpl_refine_affine: Z [S][ldz >= A] <- M (U [S][ldu >= A] - c), one thread per sample.
 *
 * trpl_refine_draw_oriented: zc [K][A] the parents in z (device memory in the _dev form), h [A], L, c HOST arrays.  The
 * n_uniform + K m children are counted and keyed as in trpl_refine_draw (Philox4x32-10, counter (n low, n high, j, generation),
 * call j -> dimensions 2j, 2j + 1, genrand_res53).  Child n_uniform + j of parent k = j mod K: z_d = zc_kd + h_d * (2 xi_d - 1),
 * u = c + L z.  A uniform child: u_d = xi_d, and its row of Z2 is NaN (no z was drawn).  X2 by trpl_refine_draw's expressions from
 * u.  inside[n] (int32) = 1 when every u_d lies in [0, 1], else 0: a child OUTSIDE the cube keeps its u and a finite X slightly
 * beyond the prior box, is never solved, and enters the population with LL = -inf; it counts in S_total, which keeps the mixture
 * proportions and therefore r(u) exact (rejection and redraw would not).  Uniform children are always inside.
 *
 * Density: B_g(u) = sum_k inv_vol * 1[z_k - h <= M_g (u - c_g) <= z_k + h] is trpl_refine_density on Z_g = trpl_refine_affine(U)
 * with a = zc - h, b = zc + h, unchanged: k ascending, one fp64 add per member box from +0.0.  r(u) keeps its form; every
 * generation carries its own (M_g, c_g), and a generation built without orientation contributes its term as before.
 *
 * Refused with TRPL_ERR_ARG before a device is touched: a NULL U, M, c, Z, zc, h, L, Z2, U2, X2, inside, lo, hi, do_log; A outside
 * [1, 16] or not the box's count; ldu < A; ldz < A; S < 1; K < 1 or K > TRPL_REFINE_MAX_PARENTS; m < 0; n_uniform < 0; more than
 * 2^31 - 2 children; a non-finite entry of M, L (lower triangle), c or h; a diagonal of M or L that is not > 0; h_d <= 0.  The _dev
 * calls take device pointers for U, Z, zc, Z2, U2, X2, inside, allocate nothing and never synchronise.
 * Python: trpl_amd.refine.orientation / affine / make_proposal(oriented=True), trpl_amd.device.refine_affine_device,
 * refine_draw_oriented_device.
 * ------------------------------------------------------------------------------------- */
int trpl_refine_affine_dev(const double *U, int64_t S, int64_t ldu, int32_t A, const double *M /*host [A][A] row-major, lower*/,
                           const double *c /*host [A]*/, double *Z, int64_t ldz, void *stream);
int trpl_refine_affine(const double *U, int64_t S, int64_t ldu, int32_t A, const double *M, const double *c, double *Z, int64_t ldz,
                       int32_t device, double *seconds);
int trpl_refine_draw_oriented_dev(const double *zc, const double *h /*host [A]*/, const double *L /*host [A][A] row-major, lower*/,
                                  const double *c /*host [A]*/, int64_t K, int32_t A, int64_t m, int64_t n_uniform, uint64_t seed,
                                  uint32_t generation, int32_t ncol, const double *lo /*host*/, const double *hi /*host*/,
                                  const int32_t *do_log /*host*/, uint32_t flags, double *Z2, double *U2, double *X2, int32_t *inside,
                                  void *stream);
int trpl_refine_draw_oriented(const double *zc, const double *h, const double *L, const double *c, int64_t K, int32_t A, int64_t m,
                              int64_t n_uniform, uint64_t seed, uint32_t generation, int32_t ncol, const double *lo, const double *hi,
                              const int32_t *do_log, uint32_t flags, double *Z2, double *U2, double *X2, int32_t *inside,
                              int32_t device, double *seconds);

/* ---------------------------------------------------------------------------------------
 * trpl_mcmc_propose, trpl_mcmc_accept, trpl_mcmc_chain_stats -- ensemble Metropolis sampling: `count` chains advance in lock-step,
 * every chain's proposal is one row of one launch of the fused likelihood, and these calls are the rest of a sweep: a symmetric
 * proposal drawn on the device, the accept/reject step, and the per-sequence sums of a convergence diagnostic.  Chains live in the
 * unit coordinates of trpl_refine_* (the A active columns of the box, uniform prior on [0, 1]^A).  (csrc/mcmc.hip; DESIGN.md
 * section 23)
 *
 * Randomness.  Chain i of a call is chain n = chain0 + i of the ensemble.  Philox4x32-10 with key (seed low word, seed high word)
 * and counter (n low word, n high word, 0x100 + j, step); genrand_res53 as in trpl_refine_draw.  The 0x100 keeps the stream apart
 * from the refinement draws (third word j < 8) under the same seed.  Call j = 0 .. 7: xi[2j] from words (x0, x1), xi[2j + 1] from
 * (x2, x3).  Call j = 8: xi_a from (x0, x1), xi_b from (x2, x3), the partner choice.  Call j = 9: xi from (x0, x1), the acceptance.
 *
 * trpl_mcmc_propose: U [count][A] the chains, partners [P][A] (NULL with P = 0), gamma, scale [A] HOST array, the box as
 * trpl_refine_draw takes it.  One thread per chain.  With P >= 2 (differential evolution: ter Braak 2006, with the partners taken
 * from the complementary half of the ensemble as in ter Braak & Vrugt 2008 and Foreman-Mackey et al. 2013):
 *     a = min((int64)(xi_a * P), P - 1),   b = min((int64)(xi_b * (P - 1)), P - 2),   b += (b >= a)      so that b != a,
 *     u'_d = (u_d + gamma * (pa_d - pb_d)) + scale_d * (2 xi_d - 1)
 * in exactly this order; with P = 0 (random walk) u'_d = u_d + scale_d * (2 xi_d - 1).  Both are symmetric in (u, u') as long as
 * the partners do not depend on u.  The jitter is uniform, so every bit can be restated without a device log or cos.  Up
 * [count][A] <- u'; inside[i] (int32) = 1 when every u'_d lies in [0, 1] (a NaN is outside), else 0; Xp [count][ncol] by
 * trpl_refine_draw's expressions from u' whether inside or not (a proposal outside keeps a finite X slightly beyond the prior box
 * and is not to be solved: its likelihood is -inf).  Up, inside and the linear columns of Xp are pure functions of the arguments.
 *
 * trpl_mcmc_accept: one thread per chain; U [count][A], X [count][ncol], LL [count] are updated in place from Up, Xp, LLp, inside,
 * and accepted [count] (int32) is written.  With d = (LLp - LL) / tf, a chain takes its proposal exactly when
 *     inside != 0,   LLp is not NaN,   LLp > -inf,   and one of   !(LL > -inf),   d >= 0,   log(xi) < d   (the device's log).
 * !(LL > -inf) lets a chain that stands on a NaN or -inf likelihood always move to a finite one.  An accepted row of U, X, LL is
 * the proposal's bits; a rejected row is not written.
 *
 * trpl_mcmc_chain_stats: H [n][ldh >= Q] a history that stays where it is, the steps [t0, t1).  One thread per column q < Q,
 * adjacent threads reading adjacent addresses:
 *     mean[q] = (sum of H[t][q], t ascending from +0.0) / (t1 - t0),    m2[q] = sum of (H[t][q] - mean[q])^2, t ascending from +0.0,
 * subtract, multiply, add, no contraction: the plain loop, bit for bit.  A NaN propagates.  With the 2 C sequences of a split
 * history as columns these are what split-R-hat is formed from (trpl_amd.mcmc.Chains.rhat).  The host-buffer form copies the steps
 * of the range only.
 *
 * Refused with TRPL_ERR_ARG before a device is touched, the message naming the argument: a NULL U, scale, Up, Xp, inside, X, LL,
 * LLp, accepted, H, mean, m2, lo, hi, do_log; count < 1 or more than 2^31 - 1 blocks of 256 chains; A outside [1, 16] or (propose)
 * not the box's count; P == 1, P < 0, P > 0 with partners NULL; gamma not finite; a scale_d that is not finite or < 0; chain0 < 0;
 * what trpl_refine_draw refuses of a box; (accept) ncol outside [1, 16], tf not finite or <= 0; (chain_stats) n < 1, Q < 1,
 * ldh < Q, a range that does not satisfy 0 <= t0 < t1 <= n.  The _dev calls take device pointers (scale and the box arrays
 * excepted), allocate nothing and never synchronise.
 *
 * TRPL_MCMC_FOLD, a bit of the `flags` of trpl_mcmc_propose / trpl_mcmc_propose_dev only: a proposal that leaves the unit cube is
 * reflected back at its faces, as often as needed, and no longer thrown away.  Each active coordinate goes through fold after the
 * last addition of the expression above, u'_d = ... + scale_d * (2 xi_d - 1); in fp64, one rounding per operation, in this order:
 *     v in [0, 1] (v >= 0.0 && v <= 1.0): unchanged, the same bits (-0.0 included)
 *     otherwise: r = fmod(v, 2.0); if (r < 0.0) r = r + 2.0; if (r > 1.0) r = 2.0 - r; v = r
 * fmod is exact, so any correct implementation gives numpy.fmod's bits; a NaN or +-inf gives NaN.  fold is applied per dimension.
 * Up holds the folded coordinate and Xp is formed from it by the same expressions; a fixed column and the TRPL_BOX_EQUAL_*
 * overrides are unaffected.  inside[i] becomes a code: 0 some coordinate is not finite, 1 no coordinate needed folding, 2 at
 * least one was folded; trpl_mcmc_accept tests inside != 0 and is unchanged.  Without the bit inside stays 0 / 1 and every output
 * bit is as before.  Why no Hastings term is needed: for fixed partners the unfolded increment gamma (pa - pb) + scale (2 xi - 1)
 * has a density p symmetric about 0 (the ordered pair (a, b) is uniform, so (b, a) is as likely), and the reflections at the faces
 * are isometries.  So q(y | x) = sum over the reflection group g of p(g(y) - x) is symmetric in (x, y), and the Metropolis rule of
 * trpl_mcmc_accept leaves the posterior invariant as it stands.
 * Refused (TRPL_ERR_ARG, "flags=0x.."): in trpl_mcmc_propose* any bit other than TRPL_BOX_EQUAL_* and TRPL_MCMC_FOLD;
 * TRPL_MCMC_FOLD in trpl_refine_draw*, trpl_refine_unit* and trpl_refine_draw_oriented*, where folding would change the proposal
 * density r(u).
 * Python: trpl_amd.mcmc, trpl_amd.device.mcmc_*_device.
 * ------------------------------------------------------------------------------------- */
#define TRPL_MCMC_FOLD 0x10
int trpl_mcmc_propose_dev(const double *U, const double *partners /*nullable*/, int64_t count, int64_t P, int32_t A, double gamma,
                          const double *scale /*host [A]*/, int64_t chain0, uint64_t seed, uint32_t step, int32_t ncol,
                          const double *lo /*host*/, const double *hi /*host*/, const int32_t *do_log /*host*/, uint32_t flags,
                          double *Up, double *Xp, int32_t *inside, void *stream);
int trpl_mcmc_propose(const double *U, const double *partners /*nullable*/, int64_t count, int64_t P, int32_t A, double gamma,
                      const double *scale, int64_t chain0, uint64_t seed, uint32_t step, int32_t ncol, const double *lo,
                      const double *hi, const int32_t *do_log, uint32_t flags, double *Up, double *Xp, int32_t *inside, int32_t device,
                      double *seconds);
int trpl_mcmc_accept_dev(double *U, double *X, double *LL, const double *Up, const double *Xp, const double *LLp, const int32_t *inside,
                         int64_t count, int32_t A, int32_t ncol, double tf, int64_t chain0, uint64_t seed, uint32_t step,
                         int32_t *accepted, void *stream);
int trpl_mcmc_accept(double *U, double *X, double *LL, const double *Up, const double *Xp, const double *LLp, const int32_t *inside,
                     int64_t count, int32_t A, int32_t ncol, double tf, int64_t chain0, uint64_t seed, uint32_t step, int32_t *accepted,
                     int32_t device, double *seconds);
int trpl_mcmc_chain_stats_dev(const double *H, int64_t n, int64_t ldh, int64_t Q, int64_t t0, int64_t t1, double *mean, double *m2,
                              void *stream);
int trpl_mcmc_chain_stats(const double *H, int64_t n, int64_t ldh, int64_t Q, int64_t t0, int64_t t1, double *mean, double *m2,
                          int32_t device, double *seconds);

/* ---------------------------------------------------------------------------------------
 * trpl_mcmc_levels -- EARLY REJECTION (Solonen et al. 2012): for each of `count` chains the level of trpl_loglik_cut_levels above
 * which a proposal's running sse makes its rejection by trpl_mcmc_accept certain.  The accept step's uniform depends on (seed;
 * chain, step) only, so the level is known before the proposal is solved; cutting at it changes no decision of the chain, it only
 * stops paying for proposals whose rejection is already decided.
 * One thread per chain; LL [count] in, level [count] out.  xi is drawn exactly as trpl_mcmc_accept draws it for the same (seed,
 * chain0 + i, step): Philox counter word 0x100 + 9, the same 53-bit uniform, the same log.  level = +inf (never cut) when LL is NaN
 * or not above -inf, when xi == 0, or when neither candidate verifies.  The candidates, in order: l0 = -(LL + tf log(xi)), then
 * l0 + (fabs(LL) + l0) 2^-40.  A candidate l is taken only if, with q = -l, the accept step's own expression dq = (q - LL) / tf
 * satisfies dq < 0 && !(log(xi) < dq).
 * WHY THAT IS SAFE.  Subtraction and division by tf > 0 are monotone under round-to-nearest, so every LLp <= q has d = (LLp - LL) /
 * tf <= dq: d < 0 and log(xi) < d is false, and trpl_mcmc_accept with the same (seed, chain, step) rejects it.  A system cut at
 * `level` reports sse_c > level, and the sample's P = fl(... fl(0 - sse_0) ... - sse_c ...) <= -sse_c < q because every term is
 * non-negative and rounding is monotone.  Hence a cut proposal is always one the uncut run would have rejected, and its reported
 * LLp is never stored: the chain's U, X, LL and accept flags are those of the run without levels, bit for bit.
 * PRECONDITION: the likelihood starts P from +0.0, so that LL = -sum sse; the level of a chain is given to each of its C curves (a
 * curve alone above the level is enough, since the others only lower P further).
 * Refused (TRPL_ERR_ARG): count < 1 or more chains than the grid holds; tf not finite or not > 0; chain0 < 0; "LL is NULL", "level is
 * NULL".  Python: trpl_amd.mcmc.reject_levels, trpl_amd.mcmc.run(early_reject=True), trpl_amd.device.mcmc_levels_device.
 * ------------------------------------------------------------------------------------- */
int trpl_mcmc_levels_dev(const double *LL, int64_t count, double tf, int64_t chain0, uint64_t seed, uint32_t step, double *level,
                         void *stream);
int trpl_mcmc_levels(const double *LL, int64_t count, double tf, int64_t chain0, uint64_t seed, uint32_t step, double *level,
                     int32_t device, double *seconds);

/* ---------------------------------------------------------------------------------------
 * trpl_mcmc_propose_rungs, trpl_mcmc_accept_rungs, trpl_mcmc_levels_rungs, trpl_mcmc_swap -- PARALLEL TEMPERING (replica exchange:
 * Swendsen & Wang 1986, Geyer 1991): K copies ("rungs") of the ensemble run at temperatures tf[0 .. K), every rung by the rules of
 * trpl_mcmc_propose / _levels / _accept at its own temperature, and states of adjacent rungs are exchanged by a Metropolis rule.  The
 * hot rungs cross between separated regions of the posterior; the exchange carries that down to the rung the caller wants.  All K
 * rungs advance in ONE call each, so a half-sweep stays one launch of the likelihood.  (csrc/mcmc.hip)
 *
 * Layout.  A block is K rungs of `group` chains: row k * group + c is chain c of rung k, count == K * group.  tf is a HOST array of K
 * values, copied into the kernel argument like scale; it need not be sorted.  Chain i of a call is chain chain0 + i of the ensemble,
 * as above: the row index keys Philox, so with K = 1 every stream is that of the calls above.
 *
 * trpl_mcmc_propose_rungs: trpl_mcmc_propose with `group`: chain i draws its two distinct partners from the rows [(i / group) *
 * group, + group) of partners [P][A], by the index expressions of trpl_mcmc_propose with P replaced by group.  group >= 2, P a
 * multiple of group, count <= P.  TRPL_MCMC_FOLD applies unchanged.  The rows [k group, (k + 1) group) of Up, Xp and inside are, bit
 * for bit, trpl_mcmc_propose on those rows of U with those rows of partners and chain0 + k group.
 * trpl_mcmc_accept_rungs, trpl_mcmc_levels_rungs: trpl_mcmc_accept and trpl_mcmc_levels with (K, group, tf[K]) where the scalar tf
 * is: chain i uses tf[i / group].  Rung k's rows are bit for bit the scalar call on them with tf[k] and chain0 + k group.  The safety
 * argument of trpl_mcmc_levels never compares two chains, so it holds per chain as it stands.
 *
 * trpl_mcmc_swap: U [K group][A], X [K group][ncol], LL [K group] in place, swapped [K group] (int32) out.  The pairs are the rungs
 * (k, k + 1) for k = parity, parity + 2, .. with k + 1 < K, and every c < group: rows a = k group + c and b = a + group.  One thread
 * decides a pair.  xi is the 53-bit uniform of Philox counter (n low, n high, 0x100 + 10, step), n = chain0 + a, from (x0, x1);
 *     d = (LL[b] - LL[a]) * (1.0 / tf[k] - 1.0 / tf[k + 1])        (fp64, one rounding per operation)
 * and the pair is exchanged exactly when neither LL[a] nor LL[b] is NaN and (d >= 0 || log(xi) < d) (the device's log).  A NaN d
 * (both -inf, or 0 * inf at equal temperatures) exchanges nothing.  An exchange swaps the rows a and b of U, X and LL; swapped is 1
 * on both rows of an exchanged pair and 0 on every other row of the block.  A row of no pair (rung k < parity, or the last rung when
 * it has no upper neighbour of this parity) is not touched apart from swapped = 0.  K = 1 has no pair and writes zeros.
 * WHY THE PRODUCT OF THE TEMPERED POSTERIORS STAYS INVARIANT.  The joint state is (x_0 .. x_{K-1}) with density prod_k p(x_k)
 * L(x_k)^(1 / tf[k]) on the cube.  Exchanging x_k and x_{k+1} is its own inverse, so as a proposal it is symmetric (it is proposed
 * with probability 1 from either side, whatever the states are), and its Metropolis ratio is
 *     L(x_{k+1})^(1/tf[k]) L(x_k)^(1/tf[k+1]) / (L(x_k)^(1/tf[k]) L(x_{k+1})^(1/tf[k+1])) = exp(d)
 * -- the uniform prior cancels.  Accepting with min(1, exp(d)) is therefore the exact Metropolis rule on the joint state.  Pairs of
 * one parity are disjoint, so deciding them at once is a product of such kernels; alternating parities is a deterministic cycle
 * of invariant kernels.  The marginal of rung k stays p L^(1 / tf[k]); that of tf[0] is the posterior the caller asked for.
 *
 * Refused (TRPL_ERR_ARG, before a device is touched, the message naming the argument): what trpl_mcmc_propose / _accept / _levels
 * refuse of the arguments they share; K outside [1, TRPL_MCMC_MAX_RUNGS]; group < 1 (propose: < 2); "tf is NULL"; a tf[k] that is
 * not finite and > 0 ("tf[k]="); count != K * group; (propose) P not a positive multiple of group, count > P; (swap) parity other
 * than 0 or 1, "swapped is NULL".
 * Python: trpl_amd.mcmc.propose_rungs / accept_rungs / reject_levels_rungs / swap / run_tempered, trpl_amd.device.mcmc_*_rungs_device,
 * trpl_amd.device.mcmc_swap_device.
 * ------------------------------------------------------------------------------------- */
#define TRPL_MCMC_MAX_RUNGS 64
int trpl_mcmc_propose_rungs_dev(const double *U, const double *partners, int64_t count, int64_t P, int64_t group, int32_t A, double gamma,
                                const double *scale /*host [A]*/, int64_t chain0, uint64_t seed, uint32_t step, int32_t ncol,
                                const double *lo /*host*/, const double *hi /*host*/, const int32_t *do_log /*host*/, uint32_t flags,
                                double *Up, double *Xp, int32_t *inside, void *stream);
int trpl_mcmc_propose_rungs(const double *U, const double *partners, int64_t count, int64_t P, int64_t group, int32_t A, double gamma,
                            const double *scale, int64_t chain0, uint64_t seed, uint32_t step, int32_t ncol, const double *lo,
                            const double *hi, const int32_t *do_log, uint32_t flags, double *Up, double *Xp, int32_t *inside,
                            int32_t device, double *seconds);
int trpl_mcmc_accept_rungs_dev(double *U, double *X, double *LL, const double *Up, const double *Xp, const double *LLp,
                               const int32_t *inside, int64_t count, int32_t A, int32_t ncol, int32_t K, int64_t group,
                               const double *tf /*host [K]*/, int64_t chain0, uint64_t seed, uint32_t step, int32_t *accepted,
                               void *stream);
int trpl_mcmc_accept_rungs(double *U, double *X, double *LL, const double *Up, const double *Xp, const double *LLp, const int32_t *inside,
                           int64_t count, int32_t A, int32_t ncol, int32_t K, int64_t group, const double *tf, int64_t chain0,
                           uint64_t seed, uint32_t step, int32_t *accepted, int32_t device, double *seconds);
int trpl_mcmc_levels_rungs_dev(const double *LL, int64_t count, int32_t K, int64_t group, const double *tf /*host [K]*/, int64_t chain0,
                               uint64_t seed, uint32_t step, double *level, void *stream);
int trpl_mcmc_levels_rungs(const double *LL, int64_t count, int32_t K, int64_t group, const double *tf, int64_t chain0, uint64_t seed,
                           uint32_t step, double *level, int32_t device, double *seconds);
int trpl_mcmc_swap_dev(double *U, double *X, double *LL, int32_t K, int64_t group, int32_t A, int32_t ncol, const double *tf /*host [K]*/,
                       int32_t parity, int64_t chain0, uint64_t seed, uint32_t step, int32_t *swapped /*[K group]*/, void *stream);
int trpl_mcmc_swap(double *U, double *X, double *LL, int32_t K, int64_t group, int32_t A, int32_t ncol, const double *tf, int32_t parity,
                   int64_t chain0, uint64_t seed, uint32_t step, int32_t *swapped, int32_t device, double *seconds);

/* ---------------------------------------------------------------------------------------
 * trpl_mcmc_autocov, trpl_mcmc_autocov_pool, trpl_mcmc_autocov_chains -- the sums of the chains' AUTOCOVARIANCE, from which the
 * effective sample size of a run and the Monte-Carlo error of its posterior means are formed (Geyer 1992; Vehtari, Gelman, Simpson,
 * Carpenter & Buerkner 2021).  The kept states of a chain are not independent draws; these calls say how many independent draws they
 * amount to.  (csrc/mcmc.hip)
 *
 * trpl_mcmc_autocov: H [n][ldh >= Q] a history that stays where it is, the steps [t0, t1), m = t1 - t0, and L lags, 1 <= L <= m.
 * mean [Q] and s [L][lds >= Q] out:
 *     mean[q] = (sum of H[t][q], t ascending from +0.0) / m                       trpl_mcmc_chain_stats' expression and bits
 *     e[t]    = H[t][q] - mean[q]
 *     s[l][q] = sum over t = t0 .. t1 - 1 - l, ascending, from +0.0, of e[t] * e[t + l]
 * subtract, multiply, add, no contraction: the plain loop, bit for bit.  Every (l, q) sum is sequential in t, so the bits do not
 * depend on how (l, q) is spread over threads; s[0][q] is trpl_mcmc_chain_stats' m2[q] bit for bit.  A NaN propagates through its
 * column only.  A thread owns one column and a tile of trpl_mcmc_autocov_tile() consecutive lags, adjacent threads adjacent
 * columns; no element of H outside the rows [t0, t1) and the columns [0, Q) is read, no element of s outside [0, L) x [0, Q) is
 * written.  The host-buffer form copies the steps of the range only and returns s compact, [L][Q].
 *
 * trpl_mcmc_autocov_pool: s [L][lds >= M A] in, pooled [L][A] out, the columns read as M sequences of A columns each:
 *     pooled[l][a] = sum over c = 0 .. M - 1, ascending, from +0.0, of s[l][c * A + a]
 * one thread per (l, a), fixed order, no atomics.
 *
 * trpl_mcmc_autocov_chains: the host-buffer fused form: H [n][ldh >= M A] is staged (the steps of the range only), both kernels
 * run with s in device scratch (8 L M A bytes), and only mean [M A], m2 [M A] = s[0] and pooled [L][A] come back: the bits of the
 * two calls above.
 *
 * THE ESTIMATOR (trpl_amd.mcmc.ess_from_sums; numpy, one rule).  Per column a, over M sequences of m steps:
 *     W = mean over c of m2 / (m - 1),   B / m = var(mean_c, ddof 1),   var+ = (m - 1) / m W + B / m,
 *     acov[l] = pooled[l] / (M m),   rho[l] = 1 - (W - acov[l]) / var+,   rho[0] = 1,
 *     P_k = rho[2k] + rho[2k + 1] (Geyer's pairs),   K = the first k where P_k > 0 fails, or L / 2 if it never fails (the sum is then
 *     truncated by L and the ESS an upper bound),   P made non-increasing by a running minimum,
 *     tau = max(-1 + 2 sum_{k < K} P_k, 1 / log10(M m)),   ess = M m / tau.
 * trpl_amd.mcmc.Chains.ess applies it to the 2 C sequences of a history split in halves, as split-R-hat splits it: one
 * trpl_mcmc_autocov_chains call per half, the pooled sums added, half 0 + half 1.
 *
 * Refused with TRPL_ERR_ARG before a device is touched, the message naming the argument: a NULL H, mean, s, m2, pooled; n < 1,
 * Q < 1, ldh < Q, lds < Q (pool: lds < M * A); a range that does not satisfy 0 <= t0 < t1 <= n; L < 1 or L > t1 - t0; M < 1; A
 * outside [1, TRPL_REFINE_MAX_DIMS]; more than 2^31 - 1 blocks: of 256 columns, of 256 sequences, of 256 columns times the lag tiles,
 * or of 64 sums of the pool.  The _dev calls take device pointers, allocate nothing and never synchronise.
 * Python: trpl_amd.mcmc.autocov / autocov_pool / ess_from_sums, Chains.ess / autocorr / mcse, trpl_amd.device.mcmc_autocov_device /
 * mcmc_autocov_pool_device.
 * ------------------------------------------------------------------------------------- */
int trpl_mcmc_autocov_tile(void);
int trpl_mcmc_autocov_dev(const double *H, int64_t n, int64_t ldh, int64_t Q, int64_t t0, int64_t t1, int64_t L, double *mean, double *s,
                          int64_t lds, void *stream);
int trpl_mcmc_autocov(const double *H, int64_t n, int64_t ldh, int64_t Q, int64_t t0, int64_t t1, int64_t L, double *mean, double *s,
                      int32_t device, double *seconds);
int trpl_mcmc_autocov_pool_dev(const double *s, int64_t L, int64_t lds, int64_t M, int32_t A, double *pooled, void *stream);
int trpl_mcmc_autocov_pool(const double *s, int64_t L, int64_t lds, int64_t M, int32_t A, double *pooled, int32_t device, double *seconds);
int trpl_mcmc_autocov_chains(const double *H, int64_t n, int64_t ldh, int64_t M, int32_t A, int64_t t0, int64_t t1, int64_t L, double *mean,
                             double *m2, double *pooled, int32_t device, double *seconds);

/* ---------------------------------------------------------------------------------------
 * trpl_mcmc_accept_h, trpl_mcmc_levels_h, trpl_mcmc_propose_stretch, trpl_mcmc_prior_term -- METROPOLIS-HASTINGS: an untempered
 * additive log term h [count] per chain in the accept rule and in the early-rejection level, and the two users of it: an asymmetric
 * proposal (the affine-invariant stretch move of Goodman & Weare 2010, h = ln z^(A - 1)) and an informative prior (independent
 * Gaussians in unit coordinates, h = ln p(u') - ln p(u)).  The term is NOT divided by the temperature: tempering tempers the
 * likelihood, not the prior and not the proposal's ratio.  LL stays the likelihood alone, so LL = -sse and early rejection keep
 * working.  All four calls take a block of K rungs of `group` chains (trpl_mcmc_*_rungs above); K = 1 is the single temperature.
 * (accept and levels: csrc/mcmc.hip, beside the calls above, whose argument record they share; the stretch and the prior term:
 * csrc/mcmc_hastings.hip; DESIGN.md sections 30 and 32)
 *
 * trpl_mcmc_accept_h: trpl_mcmc_accept_rungs with h [count] behind inside.  The same xi (Philox counter word 0x100 + 9, key (seed;
 * chain0 + i, step)), the same copy of the rows, the same `accepted`;
 *     d = (LLp - LL) / tf[i / group] + h[i]                       (fp64, one rounding per operation)
 * and the proposal is taken exactly when inside != 0, LLp is neither NaN nor -inf, h is neither NaN nor -inf, and LL is not above
 * -inf, or d >= 0, or log(xi) < d.  h = +inf accepts whatever the likelihoods are (d = +inf), unless they make d a NaN.  With
 * h[i] = +0.0 (or -0.0) everywhere every output is trpl_mcmc_accept_rungs', bit for bit: x + 0.0 is x but for x = -0.0, which no
 * comparison tells from +0.0.
 * WHY THE POSTERIOR STAYS INVARIANT.  With the proposal density q(u -> u') and the prior p, accepting with min(1, exp(d)),
 * d = (ln L(u') - ln L(u)) / tf + ln(p(u') q(u' -> u) / (p(u) q(u -> u'))), is the Metropolis-Hastings rule for the density p L^(1/tf).
 *
 * trpl_mcmc_levels_h: trpl_mcmc_levels_rungs with h [count] behind LL.  level = +inf where trpl_mcmc_levels gives +inf, and where
 * h[i] is NaN or infinite.  Otherwise the candidates, in order: l0 = -(LL + tf (log(xi) - h)), then l0 + (fabs(LL) + l0) 2^-40; a
 * candidate l is taken only if the accept step's own dq = (-l - LL) / tf + h satisfies dq < 0 && !(log(xi) < dq); +inf if neither
 * does.  WHY THAT IS SAFE: as for trpl_mcmc_levels, every LLp <= -l has (LLp - LL) / tf <= (-l - LL) / tf, and adding the same h to
 * both is monotone under round-to-nearest, so d <= dq, d < 0 and log(xi) < d is false: trpl_mcmc_accept_h with the same (seed,
 * chain, step, h) rejects.  A level may be negative (h far below zero): then every LLp = -sse <= 0 is rejected; the caller passes
 * max(level, 0) to trpl_loglik_cut_levels, which is no less safe.  With h = +0.0 the bits are trpl_mcmc_levels_rungs'.
 *
 * trpl_mcmc_propose_stretch: one stretch proposal per chain of U [count][A] with a partner from the chain's rung of partners [P][A]:
 * row (i / group) group + a, a = min((int64)(xa group), group - 1), xa the first uniform of the partner call (counter word 0x100 +
 * 8); xi the first uniform of counter word 0x100 + 11;
 *     s = (a - 1) xi + 1,   z = s s / a,   u'_d = p_d + z (u_d - p_d)      (one rounding per operation, in this order)
 * so that z has the density proportional to 1 / sqrt(z) on [1 / a, a], for which g(1 / z) = z g(z).  Out: Up [count][A], Xp
 * [count][ncol] by the sampler's expressions, formed either way, inside [count] (0 where a coordinate is outside [0, 1] or NaN,
 * else 1), z [count] and lnq [count] = (double)(A - 1) log(z), the h of the move: with partners taken from the OTHER half of the
 * ensemble the move u -> p + z (u - p) has the ratio z^(A - 1) p(u') / p(u) (Goodman & Weare 2010, eq. 7).  There is no jitter and
 * no fold.  TRPL_MCMC_FOLD is refused: a stretch reflected at a face of the cube is not reversible through the same partner -- the
 * line from p through the folded point does not pass through u -- so z^(A - 1) would not be its ratio.
 *
 * trpl_mcmc_prior_term: h_out[i] = h_in[i] + (lnp(Up_i) - lnp(U_i)), lnp(u) = the sum over d ascending, from +0.0, of (-0.5 t) t
 * with t = (u_d - mean_d) / sd_d.  A column with sd_d = +inf contributes exactly +0.0.  h_in NULL means +0.0; h_in may be h_out.
 * mean [A] and sd [A] are HOST arrays, copied into the kernel argument like scale.  The prior is common to the rungs, so it cancels
 * in trpl_mcmc_swap, which stays as it is.
 *
 * Refused (TRPL_ERR_ARG, before a device is touched, the message naming the argument): every refusal of the *_rungs counterpart
 * of the arguments they share; "h is NULL", "z is NULL", "lnq is NULL", "h_out is NULL", "mean is NULL", "sd is NULL"; (stretch) a
 * not finite or <= 1, P < 1, group < 1, P no multiple of group, count > P, "partners is NULL", TRPL_MCMC_FOLD in flags; (prior)
 * sd[d] NaN or <= 0, mean[d] not finite.  The _dev calls take device pointers, allocate nothing and never synchronise.
 * Python: trpl_amd.mcmc.propose_stretch / accept_h / reject_levels_h / prior_term / gaussian_prior, run and run_tempered with
 * kind="stretch" or prior=, trpl_amd.device.mcmc_propose_stretch_device / mcmc_accept_h_device / mcmc_levels_h_device /
 * mcmc_prior_term_device.
 * ------------------------------------------------------------------------------------- */
int trpl_mcmc_propose_stretch_dev(const double *U, const double *partners, int64_t count, int64_t P, int64_t group, int32_t A, double a,
                                  int64_t chain0, uint64_t seed, uint32_t step, int32_t ncol, const double *lo /*host*/,
                                  const double *hi /*host*/, const int32_t *do_log /*host*/, uint32_t flags, double *Up, double *Xp,
                                  int32_t *inside, double *z, double *lnq, void *stream);
int trpl_mcmc_propose_stretch(const double *U, const double *partners, int64_t count, int64_t P, int64_t group, int32_t A, double a,
                              int64_t chain0, uint64_t seed, uint32_t step, int32_t ncol, const double *lo, const double *hi,
                              const int32_t *do_log, uint32_t flags, double *Up, double *Xp, int32_t *inside, double *z, double *lnq,
                              int32_t device, double *seconds);
int trpl_mcmc_accept_h_dev(double *U, double *X, double *LL, const double *Up, const double *Xp, const double *LLp, const int32_t *inside,
                           const double *h, int64_t count, int32_t A, int32_t ncol, int32_t K, int64_t group,
                           const double *tf /*host [K]*/, int64_t chain0, uint64_t seed, uint32_t step, int32_t *accepted, void *stream);
int trpl_mcmc_accept_h(double *U, double *X, double *LL, const double *Up, const double *Xp, const double *LLp, const int32_t *inside,
                       const double *h, int64_t count, int32_t A, int32_t ncol, int32_t K, int64_t group, const double *tf, int64_t chain0,
                       uint64_t seed, uint32_t step, int32_t *accepted, int32_t device, double *seconds);
int trpl_mcmc_levels_h_dev(const double *LL, const double *h, int64_t count, int32_t K, int64_t group, const double *tf /*host [K]*/,
                           int64_t chain0, uint64_t seed, uint32_t step, double *level, void *stream);
int trpl_mcmc_levels_h(const double *LL, const double *h, int64_t count, int32_t K, int64_t group, const double *tf, int64_t chain0,
                       uint64_t seed, uint32_t step, double *level, int32_t device, double *seconds);
int trpl_mcmc_prior_term_dev(const double *U, const double *Up, int64_t count, int32_t A, const double *mean /*host [A]*/,
                             const double *sd /*host [A]*/, const double *h_in /*nullable*/, double *h_out, void *stream);
int trpl_mcmc_prior_term(const double *U, const double *Up, int64_t count, int32_t A, const double *mean, const double *sd,
                         const double *h_in /*nullable*/, double *h_out, int32_t device, double *seconds);

/* ---------------------------------------------------------------------------------------
 * trpl_mcmc_propose_subspace -- SUBSPACE DIFFERENTIAL EVOLUTION (DREAM: Vrugt, ter Braak, Diks, Robinson, Hyman & Higdon 2009): the
 * proposal of trpl_mcmc_propose_rungs on a random subset of the coordinates, along the sum of several difference vectors, with a gamma
 * chosen for the subset's size and the number of pairs and a small multiplicative jitter on the jump.  A full-dimensional DE move
 * pushes all A coordinates along one difference vector with one gamma = 2.38 / sqrt(2 A), the known weak point of DE-MC from about ten
 * dimensions on (ter Braak 2006).  The move is symmetric, so trpl_mcmc_accept*, trpl_mcmc_levels*, trpl_mcmc_prior_term and
 * trpl_mcmc_swap take it as they stand.  For a block of rungs of `group` chains each; K = 1 (group = the half ensemble) is the single
 * temperature.  (csrc/mcmc_subspace.hip)
 *
 * Arguments: those of trpl_mcmc_propose_rungs in its order, then pairs in [1, TRPL_MCMC_MAX_PAIRS], ncr in [1, TRPL_MCMC_MAX_CR], pcr
 * [ncr] (HOST, nullable: equal shares), gamma_tab [pairs][A] (HOST), e_width in [0, 1), mask [count] and sel [count] (int32, out).
 * `gamma` is checked as trpl_mcmc_propose_rungs checks it and is otherwise not read: the move's gamma is the table's.  The host turns
 * pcr into cumulative shares, cdf[m] = (pcr[0] + .. + pcr[m], ascending from +0.0) / (their sum in the same order), or (m + 1) / ncr
 * without pcr; the shares and the table travel in the kernel argument, so the device takes no square root.
 *
 * Randomness.  The stream of the calls above, key (seed) and counter (n low, n high, 0x100 + j, step), n = chain0 + i; every uniform
 * is genrand_res53 of (x0, x1) or (x2, x3).  The calls of this move:
 *     j = 0 .. 7      xi[2j], xi[2j + 1]   the additive jitter, the calls of trpl_mcmc_propose
 *     j = 8           xi_a, xi_b           the partners of pair 0, the call of trpl_mcmc_propose
 *     j = 12 .. 19    c[2(j - 12)], c[2(j - 12) + 1]    the crossover uniforms
 *     j = 20 .. 27    v[2(j - 20)], v[2(j - 20) + 1]    the jump-jitter uniforms
 *     j = 28          xi_m from (x0, x1), the crossover class; xi_s from (x2, x3), the number of pairs and the fallback coordinate
 *     j = 28 + p      xi_a, xi_b           the partners of pair p = 1 .. TRPL_MCMC_MAX_PAIRS - 1 (j = 29, 30, 31)
 * (9, 10 and 11 are the acceptance, the swap and the stretch.)
 *
 * The rule, one thread per chain, fp64 with one rounding per operation, in this order:
 *     m     = the first index with xi_m < cdf[m], or ncr - 1 if there is none;      CR = (double)(m + 1) / (double)ncr
 *     t     = xi_s * (double)pairs;   delta = min((int)t, pairs - 1) + 1;   xi_f = t - (double)(delta - 1)
 *             (delta is uniform in 1 .. pairs; the fraction of t is independent of its integer part, so xi_f is uniform too)
 *     coordinate d is selected when c_d < CR; if none is, coordinate min((int)(xi_f * A), A - 1) alone;   dsel = the number selected
 *     pair p < delta: a_p = min((int64)(xi_a * group), group - 1), b_p = min((int64)(xi_b * (group - 1)), group - 2), b_p += (b_p >=
 *             a_p), rows of the chain's rung [(i / group) * group, + group) of partners, as trpl_mcmc_propose_rungs draws its pair
 *     D_d   = (pa_0[d] - pb_0[d]), then + (pa_p[d] - pb_p[d]) for p = 1 .. delta - 1 in turn
 *     g     = gamma_tab[delta - 1][dsel - 1]
 *     selected d:    u'_d = (u_d + (g * (1.0 + e_width * (2.0 * v_d - 1.0))) * D_d) + scale_d * (2.0 * xi_d - 1.0)
 *     unselected d:  u'_d = u_d, the same bits; no jitter
 * then, for the selected coordinates only, the range test of trpl_mcmc_propose or with TRPL_MCMC_FOLD its fold: inside is 0 / 1, or
 * with the fold the code 0 / 1 / 2.  An unselected coordinate takes no part in `inside`.  Xp is formed from u' for every column by
 * the expressions of trpl_mcmc_propose.  mask[i] has bit d set where coordinate d was selected (never 0); sel[i] = delta | m << 8.
 * a_p != b_p inside a pair; the pairs are drawn independently of each other, so two pairs may share a chain or be the same pair --
 * DREAM draws them without replacement, which needs a rejection loop or a partial shuffle per thread and changes nothing below.
 *
 * WHY THE MOVE IS SYMMETRIC.  The mask, delta, the class and the factor e_d = 1 + e_width (2 v_d - 1) are drawn from the counter
 * alone: they do not depend on the chain's state.  The partners are the other half of the ensemble, which is fixed while this half
 * is updated.  Given (mask, delta, e), the increment of the selected coordinates is g e_d sum_p (pa_p - pb_p)_d + scale_d (2 xi_d - 1).
 * Exchanging a_p and b_p in every pair is as likely as the draw itself (the ordered pair (a, b) is uniform over a != b, so (b, a) has
 * the same probability) and negates the sum; 2 xi_d - 1 is symmetric about 0.  So the increment's density is symmetric about 0 on the
 * selected subspace and the unselected coordinates stay: q(u -> u') = q(u' -> u), conditionally on (mask, delta, e) and therefore
 * after averaging over them, whatever their distribution -- pcr may be anything that does not look at the state.  With
 * TRPL_MCMC_FOLD the reflections at the faces are isometries of the selected subspace, and the argument of trpl_mcmc_propose's fold
 * carries over word for word.  No Hastings term arises.
 *
 * THE ANCHOR.  With ncr = 1, pairs = 1, e_width = 0 and gamma_tab filled with gamma, every output (Up, Xp, inside) is
 * trpl_mcmc_propose_rungs' with that gamma, bit for bit, folded or not: CR = 1 selects every coordinate (c_d < 1 always), pair 0 and
 * the additive jitter use the calls of trpl_mcmc_propose, 1.0 + (+-0.0) = 1.0 and g * 1.0 = g.  mask is then 2^A - 1 and sel is 1.
 *
 * Refused (TRPL_ERR_ARG, before a device is touched, the message naming the argument): what trpl_mcmc_propose_rungs refuses, in its
 * order (group < 2 among them), then pairs outside [1, TRPL_MCMC_MAX_PAIRS]; ncr outside [1, TRPL_MCMC_MAX_CR]; a pcr[m] that is
 * negative or not finite; a pcr whose sum is not positive; a gamma_tab entry that is not finite; e_width outside [0, 1); "gamma_tab is
 * NULL", "mask is NULL", "sel is NULL"; then what trpl_refine_draw refuses of a box.  TRPL_MCMC_FOLD is honoured; any bit other than
 * it and TRPL_BOX_EQUAL_* is refused.  The _dev call takes device pointers (scale, pcr, gamma_tab and the box arrays excepted),
 * allocates nothing and never synchronises.
 * Python: trpl_amd.mcmc.propose_subspace / subspace_gamma_table, run and run_tempered with kind="subspace",
 * trpl_amd.device.mcmc_propose_subspace_device.
 * ------------------------------------------------------------------------------------- */
#define TRPL_MCMC_MAX_PAIRS 4
#define TRPL_MCMC_MAX_CR 8
int trpl_mcmc_propose_subspace_dev(const double *U, const double *partners, int64_t count, int64_t P, int64_t group, int32_t A, double gamma,
                                   const double *scale /*host [A]*/, int64_t chain0, uint64_t seed, uint32_t step, int32_t ncol,
                                   const double *lo /*host*/, const double *hi /*host*/, const int32_t *do_log /*host*/, uint32_t flags,
                                   double *Up, double *Xp, int32_t *inside, int32_t pairs, int32_t ncr, const double *pcr /*host [ncr], nullable*/,
                                   const double *gamma_tab /*host [pairs][A]*/, double e_width, int32_t *mask, int32_t *sel, void *stream);
int trpl_mcmc_propose_subspace(const double *U, const double *partners, int64_t count, int64_t P, int64_t group, int32_t A, double gamma,
                               const double *scale, int64_t chain0, uint64_t seed, uint32_t step, int32_t ncol, const double *lo,
                               const double *hi, const int32_t *do_log, uint32_t flags, double *Up, double *Xp, int32_t *inside,
                               int32_t pairs, int32_t ncr, const double *pcr /*nullable*/, const double *gamma_tab, double e_width,
                               int32_t *mask, int32_t *sel, int32_t device, double *seconds);

/* ---------------------------------------------------------------------------------------
 * trpl_mcmc_evidence_sums -- the sums of the LOG-EVIDENCE estimates of a tempered run: what stepping-stone sampling (Xie, Lewis, Fan,
 * Kuo & Chen 2011) and thermodynamic integration (Lartillot & Philippe 2006) need of the kept likelihoods of the K rungs, so that the
 * hot rungs of trpl_mcmc_swap's ladder also give every ratio Z(tf_k) / Z(tf_k+1) of the marginal likelihood
 *     Z(tf) = integral over the cube of exp(LL(u) / tf) p(u) du
 * without another solve.  (csrc/mcmc_evidence.hip)
 *
 * LL [K][n][C] in, contiguous and rung-major (the kept history of trpl_amd.mcmc.run_tempered), the steps [t0, t1) cut into B blocks
 * of w = (t1 - t0) / B consecutive steps; tf [K] on the host, copied into the kernel argument like trpl_mcmc_swap's.  With
 *     delta_k = 1.0 / tf[k] - 1.0 / tf[k + 1]                                      trpl_mcmc_swap's expression
 * ext [K][2] out: the maximum and the minimum of the rung's LL over the range, a zero as +0.0; both NaN when a value of the rung in
 * the range is NaN.  sums [K][B][TRPL_MCMC_EVIDENCE_SUMS] out, for block b of rung k over its w C values x:
 *     0  sum of x
 *     1  up    = sum of e,   e = exp(delta_(k-1) * (x - a)),  a the rung's maximum if delta_(k-1) >= 0, else its minimum; +0.0 for k = 0
 *     2  up2   = sum of e * e
 *     3  down  = sum of e',  e' = exp((-delta_k) * (x - a')), a' the rung's minimum if delta_k >= 0, else its maximum; +0.0 for k = K - 1
 *     4  down2 = sum of e' * e'
 *     5  the number of x above -inf, as a double
 * up is the rung's stepping-stone sum towards rung k - 1, down the reverse estimate towards rung k + 1; the centring keeps every
 * exponent <= 0.  The exponent is a subtraction and a product in fp64, one rounding each, no contraction.  THE RULE OF -inf AND
 * ZERO: an x = -inf is not put through the expression; it gives +0.0 to a sum whose coefficient (delta_(k-1) for up, -delta_k for
 * down) is >= 0 and +inf to one whose coefficient is < 0, and -inf to the sum of x.  A coefficient of +-0.0 (two equal
 * temperatures) gives 1.0 for every x above -inf, so up = down = slot 5 exactly.  A NaN makes the extrema and every sum of every
 * block of its own rung NaN and touches no other rung.
 * Every sum has one association, a function of (w, C) alone: one workgroup of 256 threads per (k, b); thread j adds the elements j,
 * j + 256, .. of the block in (t, c) row-major order, ascending from +0.0; the 256 partials are added by the halving tree
 * p[j] = p[j] + p[j + s], s = 128 .. 1.  No atomics: the same call gives the same bits on every run and every device.  Two
 * passes: the extrema (per block into the block's own row of sums, then per rung into ext), then the sums, which overwrite those
 * rows; nothing but ext and sums is written, nothing outside the rows [t0, t1) is read.  The host-buffer form copies the steps of
 * the range only.
 *
 * THE ESTIMATOR (trpl_amd.mcmc.log_evidence_ratios; numpy, one rule).  N_k = slot 5 summed over the blocks, the sums below over the
 * blocks in ascending b, mean_k = (sum of slot 0) / N_k.  For every adjacent pair k, k + 1 three estimates of
 * ln Z(tf_k) - ln Z(tf_k+1):
 *     forward = delta_k * a  + ln(up_(k+1) / N_(k+1))      from the hotter rung, a its centre
 *     reverse = delta_k * a' - ln(down_k / N_k)            from the colder rung, a' its centre
 *     ti      = delta_k * (mean_k + mean_(k+1)) / 2        the trapezoid of thermodynamic integration
 * (delta_k = 0: the product with the centre is taken as 0).  Each has a leave-one-block-out jackknife standard error over the B
 * blocks, sqrt((B - 1) / B * sum over b of (theta_(-b) - mean of theta_(-b))^2), NaN for B = 1, and each exponential sum its
 * term_ess = (sum e)^2 / (N sum e^2), the share of the states that carry it.  The totals over the ladder add the pairs in
 * ascending k from 0.0 and their errors in quadrature.  A prior common to the rungs cancels in every ratio.
 *
 * Refused with TRPL_ERR_ARG before a device is touched, the message naming the argument: a NULL LL, tf, ext or sums; K outside
 * [1, TRPL_MCMC_MAX_RUNGS]; n < 1; C < 1 (or K n C above 2^60 - 1); a range that does not satisfy 0 <= t0 < t1 <= n; B < 1 or B not
 * dividing t1 - t0; a tf[k] that is not finite and > 0; K B above 2^31 - 1 workgroups.  The _dev call takes device pointers (tf
 * excepted), allocates nothing and never synchronises.
 * Python: trpl_amd.mcmc.evidence_sums / log_evidence_ratios, Tempered.log_evidence, trpl_amd.posterior.log_evidence (the base of an
 * absolute ln Z), trpl_amd.device.mcmc_evidence_sums_device.
 * ------------------------------------------------------------------------------------- */
#define TRPL_MCMC_EVIDENCE_SUMS 6
int trpl_mcmc_evidence_sums_dev(const double *LL, int32_t K, int64_t n, int64_t C, int64_t t0, int64_t t1, int64_t B,
                                const double *tf /*host [K]*/, double *ext, double *sums, void *stream);
int trpl_mcmc_evidence_sums(const double *LL, int32_t K, int64_t n, int64_t C, int64_t t0, int64_t t1, int64_t B, const double *tf,
                            double *ext, double *sums, int32_t device, double *seconds);

/* ---------------------------------------------------------------------------------------
 * trpl_pcr_solve_batched_dev -- the stand-alone batched tridiagonal solve (unit U1 of the
 * measurement plan): S independent systems  ld[i] x[i-1] + d[i] x[i] + ud[i] x[i+1] = b[i],
 * i < L, the problem pcreduce solves (pvSimPCR.py:42-81), operands and result in HBM, arrays
 * [S][L], elem_bytes 8 (fp64) or 4 (fp32).  Inputs are not modified.  With TRPL_FLAG_STRICT:
 * parallel cyclic reduction in pcreduce's elimination order with IEEE divides, bit-identical to
 * it.  Default (FAST): in-lane cyclic-reduction levels, then PCR on one row per lane with
 * Newton-refined reciprocals, then back-substitution -- the same solution to rounding
 * (both are exact eliminations), not the same operation order.
 * Algorithmic traffic 5 * L * elem_bytes per system.  Placement: five arrays that sit at the same offset
 * modulo a large power of two (separate 64 MiB allocations) send a wavefront's four loads to the same HBM
 * channel; offsetting each array by a further 4 KiB is worth ~6 % (5.26 -> 5.57 TB/s on MI355X).
 * ------------------------------------------------------------------------------------- */
int trpl_pcr_solve_batched_dev(const void *ld, const void *d, const void *ud, const void *b,
                               void *x, int64_t S, int32_t L, int32_t elem_bytes, uint32_t flags,
                               void *stream);
int trpl_pcr_solve_batched(const void *ld, const void *d, const void *ud, const void *b, void *x,
                           int64_t S, int32_t L, int32_t elem_bytes, uint32_t flags,
                           int32_t device, double *seconds);

#ifdef __cplusplus
}
#endif
#endif /* TRPL_H */
