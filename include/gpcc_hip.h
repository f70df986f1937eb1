/*
 * gpcc_hip.h -- C ABI of libgpcc_hip.so: the MI355X (gfx950) implementation of GPCC.jl's
 * marginal-log-likelihood hot path.
 *
 * The reference (pure Julia, /root/reference) has no FFI / plugin interface of its own
 * (SURVEY.md section 8(b)); this header IS the boundary a maintainer binds with `ccall`
 * (INTEGRATION.md shows the Julia shim) and the build's own host layer binds with ctypes
 * (gpcc.jl_amd/_capi.py).  Each entry point cites the reference code whose body it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; host pointers unless the name ends in _device.
 *   - every function returns int: 0 ok, <0 error (message via gpcc_last_error); never throws.
 *   - per-item status in info[] follows LAPACK potrf: 0 ok; >0 = order of the first
 *     non-positive pivot (the reference's PosDefException, swallowed by safewrapper at
 *     src/gpccfixdelay_marginaliseb.jl:153), loglik = NaN; -1 = some alpha <= 0 (the @assert at
 *     src/delayedCovariance.jl:3); -2 = rho <= 0 (error() at src/delayedCovariance.jl:5-7).
 *   - ragged light curves are passed flattened in band order, user order inside a band
 *     (Y = reduce(vcat, yarray), src/gpccfixdelay_marginaliseb.jl:85).
 *   - per-evaluation parameter blocks are ROW-major M x L (Julia passes an L x M Matrix).
 *   - no callbacks on the likelihood path (only gpcc_neldermead_batch and gpcc_newton_batch, the optimisers on their own, take one), no
 *     retained caller pointers, all device memory owned by the handle;
 *     one handle per thread/process; several handles (and processes) may share a GPU.
 *   - there is NO CPU fallback: without a HIP device every compute entry returns an error.
 */
#ifndef GPCC_HIP_H
#define GPCC_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpcc_handle_s *gpcc_handle_t;

/* kernel ids: src/util.jl:15-23 (OU), :28 (rbf), :32-40 (matern32), :44-52 (matern52).
 * Any other Julia callable stays on the pure-Julia path. */
enum { GPCC_KERNEL_OU = 0, GPCC_KERNEL_RBF = 1, GPCC_KERNEL_MATERN32 = 2, GPCC_KERNEL_MATERN52 = 3 };
enum { GPCC_PRECISION_FP64 = 0, GPCC_PRECISION_FP32 = 1 };
enum { GPCC_MAX_BANDS = 8 };

enum {
    GPCC_OK = 0,
    GPCC_ERR_ARGUMENT = -1,      /* bad sizes / ids / NULL pointers */
    GPCC_ERR_HIP = -2,           /* a HIP runtime call failed (no device, OOM, launch failure) */
    GPCC_ERR_UNSUPPORTED = -3,   /* valid request this build does not implement yet */
    GPCC_ERR_STATE = -4
};

int gpcc_version(void);

/* What this library was built from: "src=<first 16 hex digits of the SHA-256 of its sources> defines=[<extra compiler defines>]".
 * The product library is always built without extra defines (gpcc.jl_amd/build.py refuses them for the default output path); A/B
 * libraries of tools/ carry theirs here.  bench.py prints it and quotes committed counter summaries only when it matches. */
const char *gpcc_build_info(void);

/* Last error text of a handle; handle == NULL gives the calling thread's last
 * handle-less error (gpcc_create / gpcc_covariance / gpcc_probabilities). */
const char *gpcc_last_error(gpcc_handle_t handle);

/* Replaces the per-call precompute of gpccfixdelay (src/gpccfixdelay_marginaliseb.jl:85-98;
 * src/gpccfixdelay.jl:85-96 when marginalise_b == 0): uploads t, sigma^2, Y - bbar once and keeps
 * mu_b[l] = mean(y_l), Sigma_b[l] = 100 var(y_l) (n-1).  Nl[l] >= 1 (>= 2 when marginalise_b). */
int gpcc_create(gpcc_handle_t *handle, int L, const int *Nl, const double *t, const double *y,
                const double *sigma, int kernel_id, int marginalise_b, int precision, int device_id);
int gpcc_destroy(gpcc_handle_t handle);

/* The same for a list of devices of ONE process: the reference parallelises the delay-grid map
 * with pmap workers (README.md:181-211, :258-287); here one handle owns a replica of the light curves on every listed
 * device.  gpcc_loglik_batch and gpcc_grid_loglik then cut every batch into contiguous blocks, one host thread and
 * one device per block, and collect [loglik | info] with ONE all-gather (RCCL over xGMI, ncclCommInitAll +
 * ncclAllGather; no torch, no MPI), after which every device holds the whole vector (gpcc_multi_gathered).
 * RCCL refuses a communicator with a repeated device: lists with duplicates (the one-GPU rehearsal {0, 0}) and
 * single-entry lists gather through host memory instead; gpcc_get_option(h, "gather_mode") says which.
 * A multi-device handle is accepted by every entry point that takes a handle, except gpcc_loglik_batch_device
 * (device pointers belong to one device): the single-matrix utilities (gpcc_predict, gpcc_posterior_offsets,
 * gpcc_model_matrix, gpcc_factor_dense, profiling) run on device_ids[0]; options apply to all devices. */
enum { GPCC_GATHER_NONE = 0, GPCC_GATHER_RCCL = 1, GPCC_GATHER_HOST = 2 };
int gpcc_create_multi(gpcc_handle_t *handle, int L, const int *Nl, const double *t, const double *y,
                      const double *sigma, int kernel_id, int marginalise_b, int precision,
                      const int *device_ids, int n_devices);

/* The gathered vector of the last gpcc_loglik_batch as it sits on device `which` of a multi-device handle:
 * n_devices blocks of [loglik(blk) | info-as-double(blk)], blk = ceil(M / n_devices) written to *blk_out
 * (out == NULL only queries blk).  After gpcc_grid_loglik on a multi-device handle (round 4: the fit is sharded BY DELAY, device i
 * fits the delays i, i + n, i + 2n, ... with its own lock-step optimiser, and the results are collected by ONE all-gather):
 * n_devices blocks of blk = ceil(G / n_devices) rows [loglik, info, iterations, rho, alpha(L)], i.e. gpcc_get_option("gather_width")
 * = L + 4 doubles per row instead of 2 x blk. */
int gpcc_multi_gathered(gpcc_handle_t handle, int which, long *blk_out, double *out, long capacity);

/* Timing of the last gpcc_loglik_batch on a multi-device handle: compute_ms[n_devices] = each device's share on its own
 * stream (HIP events), *gather_ms = the gather phase (RCCL all-gather + final copy; host wall clock), *total_ms = the whole
 * call.  Any pointer may be NULL.  (One persistent host thread per device runs the shares; none is created per batch.) */
int gpcc_multi_stats(gpcc_handle_t handle, double *compute_ms, double *gather_ms, double *total_ms);

/* Options (gpcc_set_option / gpcc_get_option).  Defaults are the measured best; none changes WHAT is computed, several select the
 * factorisation path by group size (results of different paths agree to ~1e-13 relative in fp64).  History of every option, and of the
 * variants that were measured and removed, is in LOG.md.
 *
 *   key                      default  meaning
 *   -----------------------  -------  ---------------------------------------------------------------------------------------------
 *   streams                  2        groups of a batch alternate between this many HIP streams
 *   slots_per_stream         256      evaluations resident per group (fewer where 256 slots exceed 55 % of the device's memory)
 *   chain_max                32       groups of at most this many evaluations at N >= 384 -- a single objective(alpha, rho),
 *                                     marginaliseb.jl:133-141 called from Optim's loop, :209-211 -- run as ONE persistent launch
 *                                     (gpcc_chain: two chain workgroups per evaluation carry diagonal step -> column solve -> next
 *                                     diagonal tile without leaving their CUs, all other CUs pull trailing-update jobs; fp64 handles);
 *                                     0 = the two-launches-per-step path below
 *   chain_work_max           4096     ... up to 12 evaluations: and evaluations x (N/128)^2 at most this (12 evaluations up to N = 2048, 4 at
 *                                     N = 4096: above, the path below is faster)
 *   chain_wide_work_max      1024     ... 13 .. chain_max evaluations: and evaluations x (N/128)^2 at most this (32 at N <= 512, 28 at N = 768, 16 at
 *                                     N = 1024: there the alternative,
 *                                     two halves on two streams, is slower even when the halves do overlap -- and they only do when the
 *                                     runtime maps the two streams onto different hardware queues)
 *   chain_workers_max        0        ... at most this many worker workgroups per launch (0 = as many as the widest step has jobs, up to the
 *                                     chip).  For P caller processes sharing a GPU at N >= 2048, where every launch would ask for all CUs and
 *                                     the launches queue: about n_cus / P - 6 (4 processes at N = 4096: 1210 instead of 800 evaluations/s in
 *                                     total; a single caller is 2.4x slower with it).  Changes no result.
 *   chain_batch              8        ... bulk tile updates take aligned blocks of up to this many columns (1, 2, 4, 8) per job where a tile has
 *                                     the slack -- far from the diagonal 8, towards it 4, 2, 1 (8 w chunks of K instead of 8: one fixed cost of
 *                                     ~6 us per w x 13.7 us of MFMAs; the same sums in the same order -- the same bits); 1 = one column per job
 *   chain_batch_min          40000    ... for groups of evaluations x (N/128)^3 >= this (the worker-bound ones: from 3 evaluations at N = 3072, 2 at
 *                                     N = 4096; -3 ... -12 % there, nothing or slightly worse where the chain is the bound)
 *   chain_helpers_max        6        ... with four more dedicated workgroups per evaluation (the solves of the tile below the diagonal run
 *                                     beside every diagonal step) for groups of at most this many evaluations
 *   chain_quarters_max       2        ... and the tile updates the next step needs at once as four quarter-tile jobs each, for groups of
 *                                     at most this many evaluations (latency for CU time: 4 x 7.4 us instead of 22 us per tile)
 *   fused_small_max          12       ... otherwise such groups run the kernels gpcc_panel_trsm_rows and gpcc_small_step: 2 launches per step
 *   right_looking_max        12       groups of at most this many evaluations factorise right-looking
 *   fused_solve              1        larger groups: panel solve inside the update kernel (gpcc_syrk_diag + gpcc_update_solve);
 *                                     0 = the three-kernel path (gpcc_panel_update, gpcc_diag_factor, gpcc_panel_trsm) everywhere
 *   fused_solve_min          112      ... from this group size on (smaller left-looking groups keep the three-kernel path)
 *   fused_solve_min_split    64       ... the same threshold for each half of a split group (follows fused_solve_min when that is
 *                                     set below 64 or above 112)
 *   fold_assembly            1        groups of more than fused_small_max evaluations do not write the off-diagonal tiles of
 *                                     delayedCovariance: the job that reads a tile first evaluates its elements (same bits)
 *   hybrid_tail              1        three-kernel groups finish right-looking once their trailing matrices fit hybrid_mall_mb
 *   hybrid_mall_mb           400      ... that budget (MB; the Infinity Cache is 256 MiB)
 *   hybrid_occ               384      ... and only steps with fewer left-looking jobs than this become right-looking
 *   split_min                24       a group of split_min .. split_max evaluations runs as two halves on two streams (0 = never)
 *   split_max                240      (see split_min)
 *   split_nt_min             12       ... at N > 128 (split_nt_min - 1)
 *   split_small              1        ... and the smaller groups for which that was measured to pay
 *   shared_prefix            1        0 off; 1: gpcc_loglik_batch detects a fixed-hyper-parameter delay sweep (README.md:172-174) and
 *                                     factorises the tile rows inside band 1 once per group (bitwise the same); 2: the caller asserts it
 *   small_n                  1        N <= 383 runs the small-N family (one launch per batch, the matrix in registers, always fp64:
 *                                     an fp32 handle's precision is ignored there); 0 = the tile kernels; env GPCC_SMALL_N = default
 *   small_wide_max           512      small-N batches of at most this many evaluations run four waves per evaluation
 *   fit_device_unpack        1        gpcc_grid_loglik, small-N path: the kernel unpacks the optimiser's vectors itself
 *   fit_speculate            1        ... latency-bound rounds evaluate all four candidate points of an iteration at once
 *   fit_threads              0        ... host threads (slices) of a large fit; 0 = by size
 *   fit_markov               0        gpcc_grid_loglik: 1 = every optimiser round is one gpcc_loglik_markov_batch (OU, Matern kernels; the
 *                                     same likelihood evaluated in linear time, so the fit's trajectory agrees to rounding, not bitwise)
 *   markov_chunk_rows        0        gpcc_predict_markov_batch: rows per chunk of its tap scratch; 0 = what fits 128 MiB (results do not
 *                                     depend on it)
 *   markov_sample_chunk_draws 0       gpcc_sample_markov_batch: draws per chunk of its scratch; 0 = what fits 128 MiB in whole waves
 *                                     (results do not depend on it)
 *   markov_multi_chunk       0        gpcc_loglik_markov_multi_batch: realisations per chunk of its scratch, rounded down to whole blocks;
 *                                     0 = what fits 128 MiB (results do not depend on it)
 *   markov_resample_bytes_max 512 MiB gpcc_loglik_markov_resampled_batch: the most the packed data of one call (16 N R bytes) may take;
 *                                     a larger call is refused with GPCC_ERR_UNSUPPORTED (the callers split R; >= 0)
 *   fp32_refine              1        fp32 handles: fp64 refinement of the quadratic forms
 *   fp32_guard               1        fp32 handles: evaluations whose pivot ratios exceed the limits are repeated in fp64
 *   fp32_assemble            1        fp32 handles: tiles inside one band pair are evaluated in fp32
 *   fp32_chain               1        fp32 handles: a call that chain_max / chain_work_max would give to the persistent launch on an fp64
 *                                     handle (one objective(alpha, rho) at N >= 384: bound by latency, not by the matrix pipe) is
 *                                     evaluated in fp64 by it, on the handle's internal fp64 twin: the fp64 handle's bits, conditioning
 *                                     estimates 0; 0 = fp32 tiles on the launch-per-step path ("fp32_chain_count": evaluations so far)
 *
 * Read-only keys of gpcc_get_option: "N", "Np", "precision", "bytes_per_slot", "hess_bytes_per_slot" / "hess_slots" (the Hessian's
 * memory per slot and the slots it holds, 0 before its first call: gpcc_loglik_hess_batch), "heldout_slots" (the slots of the held-out
 * workspace, 0 before the first gpcc_heldout_loglik_batch), "share_tiles", "n_devices", "gather_mode",
 * "gather_width", "small_n_max" (383), "small_n_active", "small_n_count", "chain_count" (evaluations that took the persistent
 * launch so far), "chain_last_grid" (workgroups of the last one), "fp32_guard_count", "fp32_chain_count", "workspace_streams" / "workspace_slots" (what the workspace really holds: smaller than "streams" /
 * "slots_per_stream" only if the device's memory was short when it was allocated -- then gpcc_last_error carries a note; the
 * options themselves are never rewritten); "markov_tap_bytes" (the tap scratch of gpcc_predict_markov_batch, 0 before its first call);
 * "markov_multi_bytes" (the scratch of gpcc_loglik_markov_multi_batch, 0 before its first call) and "markov_multi_block" (the
 * realisations a lane of that entry carries for this handle's kernel and b-mode; 0 where the entry refuses the handle);
 * "markov_resample_bytes" (the packed per-realisation data of gpcc_loglik_markov_resampled_batch, 16 N R bytes after one call, 0
 * before the first) and "markov_resample_upload_bytes" (what its pack kernel reads: the fluxes, multiplicities, means, prior
 * variances, the rows' realisations and the sort permutation as uploaded) -- both of the handle that computes. */
int gpcc_set_option(gpcc_handle_t handle, const char *key, long value);
long gpcc_get_option(gpcc_handle_t handle, const char *key);

/* mu_b[L], Sigma_b[L], resid[N] as precomputed at create (any pointer may be NULL). */
int gpcc_get_constants(gpcc_handle_t handle, double *mean_b, double *Sigma_b, double *resid);

/* fp32 handles (N >= 384; smaller problems are evaluated in fp64 by the small-N kernels and report zeros here):
 * [sum_i K_ii / d_i, max_i K_ii / d_i] over the Cholesky pivots d_i of each of the first M evaluations
 * of the last gpcc_loglik_batch / gpcc_loglik_batch_device call (2 M doubles) -- the conditioning measure behind the
 * fp32 accuracy guard.  An fp32 handle (a) refines the quadratic forms r'K^-1 r, Q'K^-1 Q, Q'K^-1 r in fp64 after the
 * fp32 factorisation (one backward solve + one pass over the fp64 elements of K regenerated on the fly: second-order
 * accurate, N^2 work; option "fp32_refine", default 1) and (b) repeats in fp64 -- internally, on a small fp64 workspace
 * it creates on first use -- every evaluation whose mean pivot ratio sum / N exceeds 300 (30 without refinement), whose LARGEST
 * ratio exceeds 5e3 (round 3: an adversarial search found evaluations below the mean limit with errors up to 0.6) or whose
 * fp32 factorisation met a non-positive pivot, so that results stay within the 1e-3 bar of fp32 also for
 * ill-conditioned hyper-parameters (calibration: DESIGN.md 4.7).  Options: "fp32_guard" (1 default, 0 = never repeat),
 * "fp32_guard_count" (read-only: evaluations repeated so far).  The guard reads the estimates back, so an fp32
 * handle synchronises the caller's stream once per call (also in the _device form).  An evaluation whose fp32 factorisation
 * broke down, or whose arguments were refused, reports +inf for both numbers.  Option "fp32_assemble" (1 default): the elements of
 * fp32 tiles that lie inside one band pair are evaluated in fp32 too (distance in fp64, rounded once; v_exp_f32) instead of in fp64
 * and rounded once -- the quadratic forms are refined from the exact fp64 elements either way. */
int gpcc_get_conditioning(gpcc_handle_t handle, int M, double *out);

/* THE HOT PATH.  objective(alpha, rho) of src/gpccfixdelay_marginaliseb.jl:133-141
 * (src/gpccfixdelay.jl:131-139 when marginalise_b == 0) for M independent (tau, alpha, rho):
 *   K = delayedCovariance(kernel, alpha, tau, rho, tarray) + Sobs + B ; logpdf(MvNormal(bbar, K), Y).
 * M = 1 serves the closure call site (:145-153, :209, :211); large M serves the delay-grid sweep
 * (README.md:172-174, :202-206, :231).  Blocking; caller-allocated outputs. */
int gpcc_loglik_batch(gpcc_handle_t handle, int M, const double *delays, const double *alpha,
                      const double *rho, double *loglik, int *info);

/* The same objective(alpha, rho) for M independent (tau, alpha, rho) in LINEAR time, for the kernels that are covariances of a Markov
 * process: OU, Matern-3/2 and Matern-5/2 (state dimension p = 1, 2, 3).  With all observations merged in the order of their shifted
 * times t - tau_band, K = delayedCovariance + Sobs (+ B) is the covariance of a linear-Gaussian state-space model, and
 * logpdf(MvNormal(bbar, K), Y) is exactly the sum of the Kalman filter's one-step predictive log-densities: O(N p^2) work and O(1)
 * memory per evaluation instead of N^3 / 3 and N^2; nothing is approximated, only the order of the arithmetic differs (agreement with
 * gpcc_loglik_batch: DESIGN.md 4.15).  The marginalised offsets b are L more (constant) states.
 *   Layout, argument checks and info codes of gpcc_loglik_batch (-1: some alpha <= 0, -2: rho <= 0; a refused row never touches the
 *   others); info[m] = j > 0: the predictive variance of the j-th observation IN MERGED ORDER was not positive and finite (the
 *   PosDefException of the dense path; possible only with sigma = 0 points or non-finite parameters), loglik[m] = NaN.
 *   GPCC_ERR_UNSUPPORTED: an rbf handle (not Markov), or marginalise_b with more than 4 bands (the offset states a lane keeps in
 *   registers; without marginalise_b any L <= GPCC_MAX_BANDS) -- use gpcc_loglik_batch there.
 * Path: one launch of the kernel gpcc_markov_eval, csrc/gpcc_markov.hip.h: one lane per evaluation, the light curves staged in LDS when they fit
 * (N <= ~6500).  Always fp64 (an fp32 handle on its fp64 twin); a multi-device handle computes on device_ids[0].  A row's result
 * depends on that row only: bitwise the same for any M, row order and option.  Memory: the light curves with every band sorted by time
 * (3 N doubles, built on the first call) and 8 M (2L + 2) bytes of staging; NONE of the N^2 workspace -- a handle that only ever calls
 * this entry never allocates it.  Option "fit_markov" (default 0): 1 makes every optimiser round of gpcc_grid_loglik one call of this
 * entry instead of a gpcc_loglik_batch (GPCC_ERR_UNSUPPORTED where this entry is); read-only "markov_count": evaluations so far.
 * Predictions, held-out scores and the offsets' posterior in linear time: the three entries below; the gradient in linear time:
 * gpcc_loglik_grad_markov_batch after them; the (alpha, rho) block of the Hessian is gpcc_loglik_hess_hyper_markov_batch, the full
 * Hessian (the rows of tau) gpcc_loglik_hess_markov_batch; the Fisher information gpcc_loglik_fisher_markov_batch; many flux
 * realisations per row in one pass (a second data axis) gpcc_loglik_markov_multi_batch; rows with their own resampled data set
 * (FR/RSS with refits) gpcc_loglik_markov_resampled_batch, with their gradient gpcc_loglik_grad_markov_resampled_batch.
 * Blocking. */
int gpcc_loglik_markov_batch(gpcc_handle_t handle, int M, const double *delays, const double *alpha, const double *rho,
                             double *loglik, int *info);

/* The three post-fit products of the Markov kernels in linear time, O(N + T) per row, from the same state-space model as
 * gpcc_loglik_markov_batch (kernels: csrc/gpcc_markov_pred.hip.h); nothing is approximated, only the order of the
 * arithmetic differs from the dense entries.  Argument lists, NULL rules, weight checks (GPCC_ERR_ARGUMENT before any device work),
 * 1 <= T <= 32768 with Ntest[l] = 0 allowed and the mixtures' semantics are those of gpcc_predict_batch and
 * gpcc_heldout_loglik_batch; the refusals are gpcc_loglik_markov_batch's (GPCC_ERR_UNSUPPORTED: rbf; marginalise_b with L > 4).  The
 * test times need not be sorted (each band is sorted on the host, results come back in the caller's order).  loglik[m], and info[m]
 * where the training filter fails (-1, -2, 1 .. N), are bitwise gpcc_loglik_markov_batch's for that row.  A row's bits do not depend on
 * M, the chunking, the row order or the launch shape.  Always fp64 (an fp32 handle on its fp64 twin); a multi-device handle computes on
 * device_ids[0].  Blocking.
 *
 * gpcc_predict_markov_batch: gpcc_predict_batch's mu_out / var_out (M x T; predictTest's per-band mean and variance, JITTER = 1e-8
 *   included) by two filters and a combine: one lane per (row, direction) walks the training points merged with the test points in
 *   ascending / descending shifted time and stores, for every test point, a copy of its state propagated to that point (the backward
 *   state mapped by D = diag(1, -1, 1), the time reversal of a stationary process); one lane per (row, test point) then forms
 *   P_s = (P_f^-1 + P_b^-1 - P0^-1)^-1, m_s = P_s (P_f^-1 m_f + P_b^-1 m_b), mu* = h'm_s + mean(y_band), var* = h'P_s h + JITTER.  A
 *   training point that ties with a test point in shifted time counts on the forward side only.  info[m] = N + j (1 <= j <= T, the
 *   caller's flattened order): the combine of test point j met a pivot that is not positive and finite -- row m of mu_out and var_out
 *   is NaN, loglik[m] valid, no other row touched.
 *   Memory, allocated on the first call and grown on demand: gpcc_loglik_markov_batch's, plus 16 T bytes of test points, the tap
 *   scratch 16 T (n + n (n + 1) / 2) bytes per row of a chunk (n = p + L offsets <= 7: at most 560 T), the chunk being the rows that
 *   fit 128 MiB (whole waves of 64 when it holds one; at least one row, whatever it needs; option "markov_chunk_rows" > 0 sets it;
 *   read-only "markov_tap_bytes": its size), 16 T bytes per row of the chunk for mu and var, and with weights 48 T + 8 M bytes.
 * gpcc_heldout_loglik_markov_batch: heldout[m] = loglik(training U test) - loglik(training), two lanes per row of one launch, the test
 *   points entering the first as observations with variance sigmatest^2 + JITTER and residual ytest - mean(y_band of the training
 *   data); equal to gpcc_heldout_loglik_batch's logpdf.  info[m] = N + j: the predictive variance of test point j (the caller's
 *   order) in the union filter was not positive and finite (or that of a training point after it) -- heldout[m] NaN, loglik[m] valid.
 *   There is no nearestposdef retry here (there is no test block to repair).  Memory: 28 T bytes of test points and 28 M + 32 bytes.
 * gpcc_posterior_offsets_markov_batch: mu_b_out (M x L) and Sigma_b_out (M x L x L, symmetric) of gpcc_posterior_offsets at every row:
 *   the offset block of the forward filter's final state, mu = m[p:] + mean(y_band), Sigma = P[p:, p:]; NaN where info[m] != 0.
 *   marginalise_b == 0: GPCC_ERR_ARGUMENT, as gpcc_posterior_offsets.  Memory: 8 M (L + L (L + 1) / 2) bytes.
 * A handle that never calls these allocates none of it, and none of them allocates the N^2 workspace. */
int gpcc_predict_markov_batch(gpcc_handle_t h, int M, const double *delays, const double *alpha, const double *rho, const int *Ntest,
                              const double *ttest, const double *weights, double *mu_out, double *var_out, double *mix_mu,
                              double *mix_var, double *loglik, int *info);
int gpcc_heldout_loglik_markov_batch(gpcc_handle_t h, int M, const double *delays, const double *alpha, const double *rho,
                                     const int *Ntest, const double *ttest, const double *ytest, const double *sigmatest,
                                     const double *weights, double *heldout, double *mix_heldout, double *loglik, int *info);
int gpcc_posterior_offsets_markov_batch(gpcc_handle_t h, int M, const double *delays, const double *alpha, const double *rho,
                                        double *mu_b_out, double *Sigma_b_out, double *loglik, int *info);

/* objective(alpha, rho) and its gradient in LINEAR time for the Markov kernels (OU, Matern-3/2, Matern-5/2), exact: the forward
 * sensitivities of the Kalman filter of gpcc_loglik_markov_batch -- the recursion carried for (d mean / d theta, d covariance / d theta)
 * beside (mean, covariance), O(N p^2) work and O(1) memory per parameter (kernel: csrc/gpcc_markov_grad.hip.h).
 *   Layout of gpcc_loglik_grad_batch: grad is M rows of 2L+1 doubles [d/d alpha_1..alpha_L, d/d rho, d/d tau_1..tau_L] in the
 *   reference's (constrained) parameters; a row is NaN where info != 0.  The conventions are the dense entry's: at an exact tie of two
 *   bands in shifted time the OU kernel's d/d tau is the mean of the one-sided derivatives (dk/ds at 0 taken as 0), computed as the
 *   mean of two filters that place the band first and last among the tied points; the Matern kernels are differentiable there.
 *   Refusals, argument checks, info codes and memory behaviour of gpcc_loglik_markov_batch: GPCC_ERR_UNSUPPORTED for rbf and for
 *   marginalise_b with more than 4 bands -- use gpcc_loglik_grad_batch there; -1 / -2 rows never touch the others; info[m] = j > 0 is
 *   the merged position of the first predictive variance that is not positive and finite.  loglik[m] and info[m] are bitwise
 *   gpcc_loglik_markov_batch's for that row (they come from a launch of its kernel inside the same call).
 * Path: one lane per (row, parameter slot) -- L alpha slots, one rho slot, L tau slots (OU: 2L) -- in one launch, then a small kernel
 * that writes the rows.  A row's bits depend on that row alone: no atomics, the same bits for any M, row order, option and handle
 * flavour.  Always fp64 (an fp32 handle on its fp64 twin); a multi-device handle computes on device_ids[0].  Memory: what
 * gpcc_loglik_markov_batch needs, plus 8 M bytes per slot and 8 M (2L + 1) bytes for the rows, grown on demand; NONE of the N^2
 * workspace.  Blocking. */
int gpcc_loglik_grad_markov_batch(gpcc_handle_t handle, int M, const double *delays, const double *alpha, const double *rho,
                                  double *loglik, double *grad, int *info);

/* objective(alpha, rho) and its gradient for M independent (tau, alpha, rho): loglik[M], info[M] as gpcc_loglik_batch;
 * grad: M rows of 2L+1 doubles [d/d alpha_1..alpha_L, d/d rho, d/d tau_1..tau_L] in the reference's (constrained)
 * parameters; NaN row where info != 0.  Always fp64 (an fp32 handle evaluates it on its fp64 twin).
 * The value is that of src/gpccfixdelay_marginaliseb.jl:133-141 (src/gpccfixdelay.jl:131-139 when marginalise_b == 0); the
 * reference itself has no gradient.  With r = Y - bbar, w = K^-1 r and G = w w' - K^-1, d loglik / d theta = 1/2 sum_ij G_ij
 * d Kd_ij / d theta (Sobs and B do not depend on alpha, rho, tau).  OU is not differentiable at s = 0 (coinciding shifted
 * times); there it takes dk/ds = 0, the mean of the one-sided derivatives.  Argument checks and info codes are gpcc_loglik_batch's;
 * a failed item never touches the others.  Every group runs the launch-per-step tile factorisation (N <= 383 padded to tiles: the
 * small-N family is not used), then a blocked triangular inverse and one fused pass over the lower tiles of K^-1: about three times
 * the value's fp64 work.  Results are bitwise repeatable, also across batch sizes.  A multi-device handle computes on
 * device_ids[0].  Memory: allocated on the first call, on top of bytes_per_slot, for each of workspace_streams x workspace_slots
 * slots: 2 nt tiles (every inv(L_kk) and a scratch column: 2 x nt x 131072 bytes, nt = Np / 128), Np doubles and
 * 3 L^2 nt (nt + 1) / 2 doubles; a handle that never asks for a gradient allocates none of it.  Blocking. */
int gpcc_loglik_grad_batch(gpcc_handle_t h, int M, const double *delays, const double *alpha, const double *rho,
                           double *loglik, double *grad, int *info);

/* objective(alpha, rho), its gradient, its Hessian and the expected (Fisher) information for M independent (tau, alpha, rho), with
 * theta = [alpha_1..alpha_L, rho, tau_1..tau_L], P = 2L+1 (a gradient row's order): loglik[M], info[M] and grad (M rows of P) are
 * bitwise what gpcc_loglik_grad_batch returns; hess and fisher: M row-major P x P blocks, bitwise symmetric; fisher may be NULL.
 * NaN rows / blocks where info != 0 (info as gpcc_loglik_batch; a failed item never touches the others).  With C = K^-1, w = C r,
 * G = w w' - C and D_theta = d Kd / d theta:
 *     H = 1/2 tr(G d2Kd/dtheta dphi) - (D_theta w)' C (D_phi w) + 1/2 tr(C D_theta C D_phi),   F = E[-H] = 1/2 tr(C D_theta C D_phi).
 * The first term needs k and its derivatives k_r, k_s, k_rr, k_rs, k_ss (by rho and by the shifted-time difference s); OU is not
 * differentiable at s = 0 (coinciding shifted times of two bands): there, as the gradient takes k_s = 0, the Hessian takes k_rs = 0 and
 * k_ss = 1/rho^2 (the one-sided limit, the kink's delta left out).  rbf, Matern-3/2 and Matern-5/2 are twice differentiable at 0
 * (Matern-3/2: k_ss(0) = -3/rho^2).  Always fp64 (an fp32 handle on its fp64 twin); a multi-device handle computes on device_ids[0].
 * Each group runs the gradient's path unchanged, then forms K^-1 densely, M_theta = K^-1 D_theta for every theta (fp64 MFMA, the tiles of
 * D_theta generated on the fly: 2 Np^3 flops per parameter) and the pairwise traces.  Results are bitwise repeatable, also across batch
 * sizes.  Memory: the gradient's, plus "hess_bytes_per_slot" = 8 ((P+1) Np^2 + 2 P Np + nt(nt+1)/2 (6 L^2 + P^2)) bytes for each of
 * "hess_slots" slots, allocated on the first call: as many as fit a quarter of the device's memory, at most the workspace's slots (with
 * fewer, the Hessian runs smaller groups with the same arithmetic, and gpcc_last_error carries a note); a handle that never asks for a
 * Hessian allocates none of it.  Blocking. */
int gpcc_loglik_hess_batch(gpcc_handle_t h, int M, const double *delays, const double *alpha, const double *rho,
                           double *loglik, double *grad, double *hess, double *fisher, int *info);

/* The hyper-parameter block of gpcc_loglik_hess_batch: loglik[M], info[M] and grad (M rows of P = 2L+1) as there (bitwise
 * gpcc_loglik_grad_batch's); hess and fisher (may be NULL): M row-major (L+1) x (L+1) blocks over [alpha_1..alpha_L, rho], bitwise
 * the leading block of gpcc_loglik_hess_batch's and bitwise symmetric, NaN where info != 0.  The kernels form K^-1 D_theta and the
 * traces for the L+1 hyper-parameters only (their block mode; the buffers and "hess_bytes_per_slot" are the full Hessian's).  The
 * same rules: fp64 only (an fp32 handle on its fp64 twin), a multi-device handle on device_ids[0].  Blocking. */
int gpcc_loglik_hess_hyper_batch(gpcc_handle_t h, int M, const double *delays, const double *alpha, const double *rho,
                                 double *loglik, double *grad, double *hess, double *fisher, int *info);

/* The same block in LINEAR TIME for the Markov kernels (OU, Matern-3/2, Matern-5/2), exactly: the Kalman filter of
 * gpcc_loglik_markov_batch carrying its second-order forward sensitivities.  loglik[M], info[M] and grad (M rows of
 * P = 2L+1) come from gpcc_loglik_grad_markov_batch's launches inside the same call and are bitwise that entry's; hess (may be NULL:
 * then the call is that entry): M row-major (L+1) x (L+1) blocks over [alpha_1..alpha_L, rho], every pair computed once and written to
 * both halves (bitwise symmetric), NaN where info != 0.  One lane per (row, pair), no atomics: a row's bits depend on the row alone (any
 * M, any row order).  Refusals, argument checks and info codes are gpcc_loglik_markov_batch's (rbf, and marginalise_b with L > 4:
 * GPCC_ERR_UNSUPPORTED before any device work).  An instantiation <states of the process, offset states> that the compiler cannot keep
 * out of scratch memory does not ship and is refused the same way, the message naming gpcc_loglik_hess_hyper_batch: at present <3, 4>
 * alone, Matern-5/2 with marginalise_b and L = 4 (it takes all 512 registers of a lane and 28 bytes more); everything else that
 * gpcc_loglik_markov_batch takes ships (DESIGN.md 4.18 has the table).
 * The Fisher information in linear time has a recursion and an entry of its own, gpcc_loglik_fisher_markov_batch below.  The rows of
 * tau -- the full Hessian -- are gpcc_loglik_hess_markov_batch below.
 * Memory: gpcc_loglik_grad_markov_batch's, plus 8 M bytes per pair ((L+1)(L+2)/2 of them) and 8 M (L+1)^2 bytes; none of the N^2
 * workspace.  Always fp64 (an fp32 handle on its fp64 twin); a multi-device handle computes on device_ids[0].  Blocking.
 * Option "laplace_markov" (default 0; refused where "fit_markov" is): gpcc_laplace_evidence's Newton rounds call this entry instead of
 * gpcc_loglik_hess_hyper_batch. */
int gpcc_loglik_hess_hyper_markov_batch(gpcc_handle_t h, int M, const double *delays, const double *alpha, const double *rho,
                                        double *loglik, double *grad, double *hess, int *info);

/* The FULL Hessian in LINEAR TIME for the Markov kernels, over theta = [alpha_1..alpha_L, rho, tau_1..tau_L], P = 2L+1
 * (gpcc_loglik_hess_batch's order): the same second-order forward sensitivities with the tangents of the transition by the lags
 * (kernel: csrc/gpcc_markov_hess_tau.hip.h).  loglik[M], info[M] and grad are bitwise gpcc_loglik_grad_markov_batch's
 * and the leading (L+1) x (L+1) block of every hess block is bitwise gpcc_loglik_hess_hyper_markov_batch's: both come from that
 * entry's launches inside the same call.  hess (may be NULL: then the call is gpcc_loglik_grad_markov_batch): M row-major P x P
 * blocks, every pair computed once and written to both halves (bitwise symmetric), NaN where info != 0.  There is no Fisher argument:
 * the Fisher information is gpcc_loglik_fisher_markov_batch's.
 *   TIES.  Matern-3/2 and Matern-5/2 are twice differentiable at zero lag: the rows of tau are exact whether or not two bands' shifted
 *   times coincide.  OU is not.  On a row in which two points of DIFFERENT bands have exactly equal shifted times (a delay equal to a
 *   difference of two observation times) no second derivative by tau exists, and gpcc_loglik_hess_batch's convention there
 *   (k_ss = 1/rho^2, k_rs = 0) is bilinear in the one-sided derivatives of K, so no order of the filter returns it: for such a row
 *   EVERY ENTRY WITH A tau INDEX IS NaN, info[m] stays 0, and loglik, grad and the leading (alpha, rho) block are untouched.  Use
 *   gpcc_loglik_hess_batch for OU on a grid of delays that collides with the cadence.  OU rows without such a tie are exact.  With
 *   L = 1 the tau entries are exact zeros.
 * Refusals, argument checks, info codes and memory rules are gpcc_loglik_markov_batch's (rbf, and marginalise_b with L > 4:
 * GPCC_ERR_UNSUPPORTED before any device work; -1 / -2 rows never touch the others).  An instantiation that needs scratch memory does
 * not ship and is refused the same way, the message naming gpcc_loglik_hess_batch (DESIGN.md 4.21 has the table; <3, 4>, Matern-5/2
 * with marginalise_b and L = 4, is refused as it is by gpcc_loglik_hess_hyper_markov_batch).
 * Path: one lane per (row, pair slot) with a tau in the pair -- L^2 (alpha, tau), L (rho, tau), L (tau_l, tau_l) and L (L - 1) / 2
 * (tau_l, tau_m) slots -- in one launch, then a kernel that writes the blocks.  No atomics: a row's bits depend on the row alone.
 * Memory: gpcc_loglik_hess_hyper_markov_batch's, plus 8 M bytes per new slot and 8 M P^2 bytes, grown on demand; none of the N^2
 * workspace.  Always fp64 (an fp32 handle on its fp64 twin); a multi-device handle computes on device_ids[0].  Blocking. */
int gpcc_loglik_hess_markov_batch(gpcc_handle_t h, int M, const double *delays, const double *alpha, const double *rho,
                                  double *loglik, double *grad, double *hess, int *info);

/* The expected (FISHER) INFORMATION in LINEAR TIME for the Markov kernels, over theta = [alpha_1..alpha_L, rho, tau_1..tau_L], P = 2L+1
 * (gpcc_loglik_hess_batch's order and, up to rounding, its `fisher`): I_ab = sum_k [ S_a S_b / (2 S^2) + E[eps_a eps_b] / S ] over the
 * filter's steps, the expectation taken by carrying the second moments of the filter's means and of their tangents beside the
 * covariance and its tangents (kernel: csrc/gpcc_markov_fisher.hip.h).  It is positive semi-definite at any point and
 * reads no flux (with marginalise_b the fluxes enter through the offsets' prior variances only): it answers how well a cadence
 * constrains the delay before any data exist.  loglik[M], info[M] and grad come from gpcc_loglik_grad_markov_batch's launches inside
 * the same call and are bitwise that entry's.  fisher (may be NULL: then the call is gpcc_loglik_grad_markov_batch): M row-major P x P
 * blocks, every pair computed once and written to both halves (bitwise symmetric), NaN where info != 0.
 *   TIES.  Matern-3/2 and Matern-5/2 are exact whether or not two bands' shifted times coincide.  OU has a kink at zero lag: on a row
 *   in which two points of DIFFERENT bands have exactly equal shifted times gpcc_loglik_hess_batch's convention (k_s(0) = 0) is the
 *   mean of the one-sided derivatives of K, the Fisher information is bilinear in them, and no order of the filter returns it: for such
 *   a row EVERY ENTRY WITH A tau INDEX IS NaN, info[m] stays 0 and the (alpha, rho) block is exact (gpcc_loglik_hess_markov_batch's
 *   contract).  With L = 1 the tau entries are exact zeros.
 * Refusals, argument checks, info codes and memory rules are gpcc_loglik_markov_batch's (rbf, and marginalise_b with L > 4:
 * GPCC_ERR_UNSUPPORTED before any device work; -1 / -2 rows never touch the others).  An instantiation <states of the process, offset
 * states> that the compiler cannot keep out of scratch memory does not ship and is refused the same way when fisher is not NULL, the
 * message naming gpcc_loglik_hess_batch: at present <3, 4> alone, Matern-5/2 with marginalise_b and L = 4; <3, 3> keeps one of its
 * moment matrices in LDS (DESIGN.md 4.22 has the table and the layouts tried).
 * Path: one lane per (row, pair slot), P (P + 1) / 2 slots, in one launch, then a kernel that writes the blocks.  No atomics: a row's
 * bits depend on the row alone (any M, any row order).
 * Memory: gpcc_loglik_grad_markov_batch's, plus 8 M bytes per slot and 8 M P^2 bytes, grown on demand; none of the N^2 workspace.
 * Always fp64 (an fp32 handle on its fp64 twin); a multi-device handle computes on device_ids[0].  Blocking. */
int gpcc_loglik_fisher_markov_batch(gpcc_handle_t h, int M, const double *delays, const double *alpha, const double *rho,
                                    double *loglik, double *grad, double *fisher, int *info);

/* The log-likelihood of MANY FLUX REALISATIONS per parameter row in LINEAR TIME for the Markov kernels: the second data axis of
 * gpcc_loglik_markov_batch (kernel: csrc/gpcc_markov_multi.hip.h) -- flux randomisation, parametric-bootstrap draws
 * and null light curves on the handle's cadence.  Y: R x N row-major, each row in the order gpcc_create took y.  mean: R x L, the
 * offset subtracted per realisation and band; NULL: the handle's band means (of the y it was created with) for every realisation.
 * loglik: M x R row-major.  info: M entries.
 *   THE MODEL IS THE HANDLE'S: its times, its sigma, its kernel, its b-mode and, with marginalise_b, ITS prior variances Sigma_b =
 *   100 var(y_l) of the y it was created with.  loglik[m][r] = logpdf(MvNormal(Q mean_r, K_m), Y_r), Q the replication matrix that
 *   repeats each band's offset once per point of that band, K_m = delayedCovariance + Sobs (+ B) built from the handle's constants:
 *   nothing of K depends on r.  With marginalise_b a fresh handle made from Y_r would use 100 var(Y_r) where this entry uses the
 *   handle's Sigma_b; without marginalise_b and with mean_r = the band means of Y_r the value is that fresh handle's (another order of
 *   rounding, the same bar).
 * info[m]: gpcc_loglik_markov_batch's codes (-1, -2, or the merged position j of the first predictive variance that is not positive
 * and finite); they depend on the parameter row only, and a row with info != 0 is NaN in all its R entries.  A flux that is not
 * finite makes its own column NaN and no other.
 * Refusals: gpcc_loglik_markov_batch's (rbf, and marginalise_b with L > 4: GPCC_ERR_UNSUPPORTED before any device work);
 * GPCC_ERR_ARGUMENT for R < 1 or a NULL Y.  M = 0 returns 0.
 * Path: a pack kernel gathers Y through the handle's sort permutation, subtracts the means and writes the residuals point-major in
 * blocks of RB realisations (read-only option "markov_multi_block": 8); then one lane per (row, block) carries the row's covariance
 * recursion once and RB means through it.  No atomics: cell (m, r) is bitwise the same for any M, R, row order, order of the
 * realisations and chunk.  It is not bitwise gpcc_loglik_markov_batch's value of the same data (another statement order); for a
 * single data set that entry stays the route.
 * Memory: handle-owned scratch for one chunk of realisations -- fluxes, packed residuals, results: 16 N + 8 M bytes a realisation --
 * grown on demand, chunked to 128 MiB (option "markov_multi_chunk": realisations per chunk, rounded down to whole blocks, 0 = by the
 * budget; read-only "markov_multi_bytes" reports the scratch); none of the N^2 workspace.  "markov_count" advances by M R.
 * Always fp64 (an fp32 handle on its fp64 twin); a multi-device handle computes on device_ids[0].  Blocking. */
int gpcc_loglik_markov_multi_batch(gpcc_handle_t h, int M, const double *delays, const double *alpha, const double *rho,
                                   int R, const double *Y, const double *mean, double *loglik, int *info);

/* The log-likelihood of M rows that each carry their own (tau, alpha, rho) AND THEIR OWN RESAMPLED DATA SET on the handle's cadence,
 * in LINEAR TIME for the Markov kernels (kernel: csrc/gpcc_markov_resample.hip.h): flux randomisation with a refit
 * per realisation, random subset selection (FR/RSS) and, with marginalise_b, each realisation's own Sigma_b.
 *   real: M entries, the realisation of row m, 0 <= real[m] < R.  Y: R x N row-major, each row in the order gpcc_create took y.
 *   count: R x N multiplicities >= 0 in the same order, or NULL: all 1.  mean: R x L, or NULL: the handle's band means.
 *   sigma_b: R x L, the offsets' prior variances, or NULL: the handle's; read only with marginalise_b.  loglik, info: M entries.
 * SEMANTICS.  Let sel be the points of realisation r = real[m] with count >= 1.  loglik[m] = logpdf(MvNormal(Q mean_r, K), Y_r[sel]):
 * K built from (tau, alpha, rho)_m on the handle's times t[sel] with the variances sigma^2[sel] / count and, with marginalise_b, B
 * from sigma_b[r].  This is the value of a fresh handle created from the distinct selected points with error bars sigma / sqrt(n),
 * when mean_r and sigma_b_r are that data set's band means and 100 var (n - 1); only the order of rounding differs.  A dropped point
 * contributes nothing, not even its 1/2 log 2 pi; a realisation with no selected point gives 0.0 with info 0.
 * info[m]: gpcc_loglik_markov_batch's codes; a positive j counts positions among the KEPT points in merged order, so it equals the
 * fresh handle's code.  A flux that is not finite at a kept point makes the rows that reference that realisation NaN, and no other.
 * With real[m] pointing to the handle's own y, count, mean and sigma_b NULL, the row is bitwise gpcc_loglik_markov_batch's.
 * Refusals: gpcc_loglik_markov_batch's (rbf, and marginalise_b with L > 4: GPCC_ERR_UNSUPPORTED); GPCC_ERR_ARGUMENT for R < 1, a
 * NULL Y or real, a real[m] outside [0, R), a negative count; GPCC_ERR_UNSUPPORTED, the message naming the limit, for a call whose
 * packed data (16 N R bytes) exceeds option "markov_resample_bytes_max" (512 MiB) -- the entry does not chunk, since a row may
 * reference any realisation: split R across calls.  All of them on the host, before any device work.  M = 0 returns 0.
 * Path: a pack kernel gathers Y through the handle's sort permutation, subtracts the means and writes per (r, i) one 16-byte pair
 * {residual, sigma^2_i / count}, a dropped point marked by a negative variance; then one lane per row walks the handle's shared merge
 * and reads its realisation's pair at each step, skipping dropped points and forming the lag from the last kept point.  No atomics:
 * a row's value is bitwise the same for any M, R, row order, position of its realisation in Y and split across calls.
 * Memory: handle-owned scratch grown on demand -- the packed data ("markov_resample_bytes") and what the pack kernel reads
 * ("markov_resample_upload_bytes": 12 N + 16 L bytes a realisation, 4 M for the rows); none of the N^2 workspace.  "markov_count"
 * advances by M.  Always fp64 (an fp32 handle on its fp64 twin); a multi-device handle computes on device_ids[0].  Blocking. */
int gpcc_loglik_markov_resampled_batch(gpcc_handle_t h, int M, const double *delays, const double *alpha, const double *rho,
                                       const int *real, int R, const double *Y, const int *count, const double *mean,
                                       const double *sigma_b, double *loglik, int *info);

/* That log-likelihood AND ITS GRADIENT, exact and in LINEAR TIME (kernel: csrc/gpcc_markov_resample_grad.hip.h): the
 * filter's forward sensitivities of gpcc_loglik_grad_markov_batch over each row's own resampled data set.
 *   grad: M rows of 2L+1 doubles [d/d alpha_1..L, d/d rho, d/d tau_1..L], gpcc_loglik_grad_markov_batch's order.  real, R, Y, count,
 *   mean, sigma_b, loglik, info and every refusal: gpcc_loglik_markov_resampled_batch's, word for word (the limit
 *   "markov_resample_bytes_max", M = 0, all checks on the host before any device work), and GPCC_ERR_ARGUMENT for a NULL grad.
 * SEMANTICS.  grad[m] is the gradient of the log-likelihood of a fresh handle on the reduced data set of realisation real[m] at
 * (tau, alpha, rho)_m: the band means mean_r and Sigma_b are constants of the data, not functions of the parameters.  loglik and info
 * are BITWISE gpcc_loglik_markov_resampled_batch's on the same rows (the same value kernel runs inside the call).  With real[m]
 * pointing to the handle's own y and count, mean and sigma_b NULL, grad[m] is bitwise gpcc_loglik_grad_markov_batch's.
 * A row with info != 0 has a NaN gradient; a realisation with no kept point gives 0.0, a zero gradient and info 0; a flux that is not
 * finite at a kept point makes the rows of that realisation NaN, and no other.  At an exact tie in shifted time between two KEPT
 * points of different bands OU returns the mean of the one-sided derivatives, as gpcc_loglik_grad_batch does; a tie with a dropped
 * point is no tie.
 * Path: the pack kernel and the value kernel of gpcc_loglik_markov_resampled_batch, then one lane per (row, slot) -- L alpha, one rho,
 * L tau slots (OU: 2L, the first / last pair) -- through the one first-order walk of gpcc_loglik_grad_markov_batch, reading the
 * realisation's pair at each step: a dropped point takes no step, the lag and the lag's tangent by tau come from the last KEPT point.
 * Then gpcc_loglik_grad_markov_batch's small kernel writes the rows.  No atomics: a row's bits depend on that row and its realisation
 * alone, whatever M, R, the row order, the position of the realisation in Y and the launch shape.
 * Memory: gpcc_loglik_markov_resampled_batch's plus gpcc_loglik_grad_markov_batch's slots and rows (8 M bytes per slot, 8 M (2L + 1)
 * bytes), grown on demand; none of the N^2 workspace.  "markov_count" advances by M.  Always fp64 (an fp32 handle on its fp64 twin); a
 * multi-device handle computes on device_ids[0].  Blocking. */
int gpcc_loglik_grad_markov_resampled_batch(gpcc_handle_t h, int M, const double *delays, const double *alpha, const double *rho,
                                            const int *real, int R, const double *Y, const int *count, const double *mean,
                                            const double *sigma_b, double *loglik, double *grad, int *info);

/* The log-likelihood, and its gradient, of M rows that each carry their own (tau, alpha, rho) AND THEIR OWN NOISE MODEL, in LINEAR
 * TIME for the Markov kernels (kernels: csrc/gpcc_markov_noise.hip.h).  Point i of band l of row m is observed with
 * the variance
 *     v_i = kappa[m][l]^2 sigma_i^2 + nu[m][l]     kappa >= 0: the scale of the reported error bars; nu >= 0: an excess variance, flux^2
 * kappa = 1, nu = 0 is the model of every other entry; kappa = 0 and one nu for all bands is K + sigma^2 I + B of the reference's
 * src/UNUSED/gpccfixdelay_globalnoiseterm.jl:137-147, which fits that sigma^2 as one more Nelder-Mead parameter.  The band means and
 * Sigma_b depend on y only and stay the handle's.
 *   kappa, nu: M x L row-major each; NULL: all 1 (kappa), all 0 (nu).  loglik, info: M entries.
 *   grad: M rows of 4L+1 doubles [d/d alpha_1..L, d/d rho, d/d tau_1..L, d/d kappa_1..L, d/d nu_1..L]; the first 2L+1 follow
 *   gpcc_loglik_grad_markov_batch's conventions (OU at a tie: the mean of the one-sided derivatives); a row is NaN where info != 0.
 * SEMANTICS.  loglik[m] is the value gpcc_loglik_markov_batch returns on a fresh handle created with the error bars
 * sqrt(kappa_l^2 sigma_i^2 + nu_l); only the order of rounding differs.  With kappa = 1, nu = 0 (or both NULL) loglik and info are
 * BITWISE gpcc_loglik_markov_batch's: kappa^2 sigma^2 + nu is one fma, which returns sigma^2 exactly.
 * info[m]: gpcc_loglik_markov_batch's codes and, after them in precedence (-1: some alpha <= 0, -2: rho <= 0), -3: some kappa or nu of
 * the row is negative or not finite -- loglik NaN, the gradient row NaN, no other row touched.  A positive j keeps its meaning (with
 * kappa = 0, nu = 0 a band has no noise at all, and two points that tie in shifted time give the position of the second).
 * Refusals: gpcc_loglik_markov_batch's (GPCC_ERR_UNSUPPORTED: rbf; marginalise_b with L > 4).  M = 0 returns 0.
 * Path: one lane per row (value), one lane per (row, slot) (gradient: L alpha, one rho, L tau (OU: 2L), L kappa, L nu slots, then a
 * small kernel that writes the rows); a lane's kappa^2 and nu sit in LDS beside its cursors, 44 L bytes a lane instead of 28 L, and
 * the light curves are staged in LDS while they fit beside that.  The gradient's value and info come from the value kernel inside
 * the same call.  No atomics: a row's bits depend on that row alone, whatever M, the row order, the launch shape and the options.
 * Memory: gpcc_loglik_markov_batch's, plus 16 M L bytes for kappa and nu and, for the gradient, 8 M bytes per slot and 8 M (4L + 1)
 * bytes, grown on demand; none of the N^2 workspace.  "markov_count" advances by M.  Always fp64 (an fp32 handle on its fp64 twin);
 * a multi-device handle computes on device_ids[0].  Predictions, held-out scores, the offsets' posterior and leave-one-out scores under
 * a noise model: gpcc_predict_noise_markov_batch and its siblings below; draws: gpcc_sample_noise_markov_batch.  Blocking. */
int gpcc_loglik_noise_markov_batch(gpcc_handle_t h, int M, const double *delays, const double *alpha, const double *rho,
                                   const double *kappa, const double *nu, double *loglik, int *info);
int gpcc_loglik_grad_noise_markov_batch(gpcc_handle_t h, int M, const double *delays, const double *alpha, const double *rho,
                                        const double *kappa, const double *nu, double *loglik, double *grad, int *info);

/* The Hessian of that log-likelihood over the fitted parameters of a row,
 *     theta = [alpha_1..alpha_L, rho, kappa_1..kappa_L, nu_1..nu_L],   n = 3L + 1,
 * in LINEAR TIME (kernel: csrc/gpcc_markov_noise_hess.hip.h): the filter's second-order forward sensitivities with the
 * variance's tangents (d v_i / d kappa_l = 2 kappa_l sigma_i^2, d v_i / d nu_l = 1 on band l, d2 v_i / d kappa_l^2 = 2 sigma_i^2), exact.
 *   grad: M rows of 4L+1 doubles, gpcc_loglik_grad_noise_markov_batch's layout.  loglik, grad and info are BITWISE that entry's: they
 *   come from its launches inside the same call.
 *   hess: M row-major n x n blocks in the order of theta (the delays have no rows in it), bitwise symmetric; NULL: the call IS the
 *   gradient entry.  kappa = nu = NULL: kappa = 1, nu = 0.  A row's leading (L+1) x (L+1) block is the block
 *   gpcc_loglik_hess_hyper_markov_batch returns on a fresh handle created with the error bars sqrt(kappa_l^2 sigma_i^2 + nu_l); only the
 *   order of rounding differs.
 * info, precedence (-1, -2, -3, j > 0), refusals and M = 0: gpcc_loglik_grad_noise_markov_batch's; a row with info != 0 has a NaN block
 * and touches no other row.  Besides: GPCC_ERR_UNSUPPORTED before any device work for an instantiation that the compiler cannot keep
 * out of scratch memory (Matern-5/2 with four bands and marginalised offsets, as gpcc_loglik_hess_hyper_markov_batch); the way round is
 * gpcc_loglik_hess_hyper_batch on a handle created with the effective error bars, which gives the (alpha, rho) block at a fixed noise
 * model.
 * Path: one lane per (row, pair slot a <= b), n (n + 1) / 2 slots, then a small kernel that writes both halves of the blocks.  No
 * atomics: a row's bits depend on that row alone, whatever M, the row order, the launch shape and the options.
 * Memory: the gradient entry's, plus 8 M bytes per slot and 8 M n^2 bytes, grown on demand; none of the N^2 workspace.  "markov_count"
 * advances by M.  Always fp64 (an fp32 handle on its fp64 twin); a multi-device handle computes on device_ids[0].  The rows of tau
 * under a noise model: gpcc_loglik_hess_full_noise_markov_batch below.  Not here: the Fisher information in kappa, nu.  Blocking. */
int gpcc_loglik_hess_noise_markov_batch(gpcc_handle_t h, int M, const double *delays, const double *alpha, const double *rho,
                                        const double *kappa, const double *nu, double *loglik, double *grad, double *hess, int *info);

/* The FULL Hessian of that log-likelihood, the delays included, over the gradient row's order
 *     theta = [alpha_1..alpha_L, rho, tau_1..tau_L, kappa_1..kappa_L, nu_1..nu_L],   n = 4L + 1,
 * in LINEAR TIME (kernel: csrc/gpcc_markov_noise_hess_tau.hip.h): the rows of tau by the same second-order forward
 * sensitivities -- the (alpha, tau), (rho, tau) and (tau, tau) pairs are gpcc_loglik_hess_markov_batch's recursion on the variances
 * kappa_l^2 sigma_i^2 + nu_l, the (tau, kappa) and (tau, nu) pairs carry a noise tangent and a tau tangent.  Exact.
 *   hess: M row-major n x n blocks in the order of theta, bitwise symmetric; NULL: the call IS the gradient entry
 *   (gpcc_loglik_grad_noise_markov_batch).  kappa / nu NULL: 1 / 0.
 *   loglik, grad and info are BITWISE gpcc_loglik_grad_noise_markov_batch's, and the sub-block on the indices {0..L, 2L+1..4L} is BITWISE
 *   gpcc_loglik_hess_noise_markov_batch's: both come from those entries' launches inside the same call.  The leading (2L+1) x (2L+1)
 *   block is what gpcc_loglik_hess_markov_batch returns on a fresh handle created with the error bars sqrt(kappa_l^2 sigma_i^2 + nu_l);
 *   only the order of rounding differs.
 * TIES: gpcc_loglik_hess_markov_batch's contract.  On an OU row where two points of different bands have exactly equal shifted times
 * every entry with a tau index is NaN, the (tau, kappa) and (tau, nu) entries included; info stays 0; value, gradient and the
 * [alpha, rho, kappa, nu] sub-block are untouched.  Matern-3/2 and -5/2 are exact at ties.  With L = 1 the tau entries are exact zeros.
 * info, precedence (-1, -2, -3, j > 0), refusals (GPCC_ERR_UNSUPPORTED before any device work for Matern-5/2 with four bands and
 * marginalised offsets) and M = 0: gpcc_loglik_hess_noise_markov_batch's; a row with info != 0 has a NaN block and touches no other row.
 * Path: that entry's launches, then one lane per (row, pair slot with a tau), 3 L^2 + L + L (L + 1) / 2 slots, then a small kernel
 * that writes the blocks.  No atomics: a row's bits depend on that row alone, whatever M, the row order, the launch shape and the
 * options.
 * Memory: that entry's, plus 8 M bytes per new slot and 8 M n^2 bytes, grown on demand; none of the N^2 workspace.  "markov_count"
 * advances by M.  Always fp64 (an fp32 handle on its fp64 twin); a multi-device handle computes on device_ids[0].  Not here: the Fisher
 * information in kappa, nu.  Blocking. */
int gpcc_loglik_hess_full_noise_markov_batch(gpcc_handle_t h, int M, const double *delays, const double *alpha, const double *rho,
                                             const double *kappa, const double *nu, double *loglik, double *grad, double *hess, int *info);

/* The post-fit products of rows that each carry their own noise model, in LINEAR TIME (kernels: csrc/gpcc_markov_noise_pred.hip.h,
 * DESIGN.md 4.29): gpcc_predict_markov_batch, gpcc_heldout_loglik_markov_batch, gpcc_posterior_offsets_markov_batch and
 * gpcc_loo_markov_batch with kappa, nu (M x L row-major each; NULL: all 1 / all 0, as gpcc_loglik_noise_markov_batch) behind rho.  Point
 * i of band l of row m is observed with v_i = kappa[m][l]^2 sigma_i^2 + nu[m][l]; the band means and Sigma_b stay the handle's.
 * CONTRACT.  A row's outputs are those of the plain entry on a fresh handle created with the error bars sqrt(v_i) and given the same
 * row (for the held-out score: with the test error bars mapped by the same band's kappa, nu); only the order of rounding differs.  With
 * kappa = 1, nu = 0 (arrays or NULL) EVERY output is BITWISE the plain entry's: the mapped variance is one fma, which returns sigma^2.
 *   gpcc_predict_noise_markov_batch: mu* = h'm_s + mean(y_band), var* = h'P_s h + JITTER -- the latent curve, as
 *     gpcc_predict_markov_batch: the noise model enters through the training updates only.  The mixture is that entry's arithmetic in
 *     row order.
 *   gpcc_heldout_loglik_noise_markov_batch: a test point of band l enters the union filter with the variance
 *     fma(kappa_l^2, sigmatest^2, nu_l) + JITTER (sigmatest^2 staged as the rounded product, the variance formed on the lane).
 *   gpcc_posterior_offsets_noise_markov_batch: the offset block of the final state of the filter on the variances v_i.
 *   gpcc_loo_noise_markov_batch: var_i = h'P_s h + fma(kappa_b^2, sigma_i^2, nu_b), the expression the filter's lane uses; lp_i, loo,
 *     mix_lp and mix_loo as gpcc_loo_markov_batch, so (y_i - mu_i) / sqrt(var_i) is standardised by the FITTED error bars.
 * info[m]: -1, -2, then -3 (some kappa or nu of the row is negative or not finite), the precedence of gpcc_loglik_noise_markov_batch;
 * positive codes keep their meaning (1 .. N: the training filter; N + j: test point or point j).  A row with info = -3 is NaN in every
 * per-row output and touches no other row; with a positive weight it makes the mixture NaN as any failed row does, with weight 0 it is
 * skipped.  Refusals, weight checks, NULL-output rules, 1 <= T <= 32768, the chunking (option "markov_chunk_rows", the 128 MiB tap
 * scratch), "markov_count" and the independence of a row's bits from M, the chunking, the row order and the launch shape: the plain
 * entries'.  Every <p, offsets> ships (no scratch memory).  Always fp64 (an fp32 handle on its fp64 twin); a multi-device handle
 * computes on device_ids[0].
 * Path: gpcc_markov_noise_taps / gpcc_markov_noise_loo_taps, the plain tap kernels with the mapped variance handed to the same filter
 * step; a lane's kappa^2 and nu sit in LDS behind the plain kernel's region, 56 L bytes a lane (predictions, held-out, offsets) or 44 L
 * (leave-one-out) instead of 40 L / 28 L, and the light curves are staged in LDS while they fit beside that.  The prediction's combine
 * is gpcc_markov_combine; the leave-one-out combine reads kappa, nu of its row and band.
 * Memory: the plain entry's, plus 16 M L bytes for kappa | nu in the buffer gpcc_loglik_noise_markov_batch stages them in (shared, grown
 * on demand); none of the N^2 workspace.  Draws under a noise model: gpcc_sample_noise_markov_batch.  Not here: the dense path.
 * Blocking. */
int gpcc_predict_noise_markov_batch(gpcc_handle_t h, int M, const double *delays, const double *alpha, const double *rho,
                                    const double *kappa, const double *nu, const int *Ntest, const double *ttest, const double *weights,
                                    double *mu_out, double *var_out, double *mix_mu, double *mix_var, double *loglik, int *info);
int gpcc_heldout_loglik_noise_markov_batch(gpcc_handle_t h, int M, const double *delays, const double *alpha, const double *rho,
                                           const double *kappa, const double *nu, const int *Ntest, const double *ttest, const double *ytest,
                                           const double *sigmatest, const double *weights, double *heldout, double *mix_heldout,
                                           double *loglik, int *info);
int gpcc_posterior_offsets_noise_markov_batch(gpcc_handle_t h, int M, const double *delays, const double *alpha, const double *rho,
                                              const double *kappa, const double *nu, double *mu_b_out, double *Sigma_b_out, double *loglik,
                                              int *info);
int gpcc_loo_noise_markov_batch(gpcc_handle_t h, int M, const double *delays, const double *alpha, const double *rho, const double *kappa,
                                const double *nu, const double *weights, double *mu_out, double *var_out, double *lp_out, double *loo,
                                double *mix_lp, double *mix_loo, double *loglik, int *info);

/* Same with DEVICE pointers, enqueued behind `stream` (a hipStream_t, NULL = default stream) and
 * joined back into it: asynchronous, outputs valid once `stream` has drained. */
int gpcc_loglik_batch_device(gpcc_handle_t handle, int M, const double *d_delays,
                             const double *d_alpha, const double *d_rho, double *d_loglik,
                             int *d_info, void *stream);

/* Dense K = delayedCovariance + Sobs + B of one (tau, alpha, rho), column-major N x N
 * (src/gpccfixdelay_marginaliseb.jl:135, :237-241) -- for prediction and tests. */
int gpcc_model_matrix(gpcc_handle_t handle, const double *delays, const double *alpha, double rho,
                      double *K_out);

/* Lower Cholesky factor of that K (PDMat's cholesky at marginaliseb.jl:139), column-major N x N,
 * strict upper triangle zero; *info as above. */
int gpcc_factor_dense(gpcc_handle_t handle, const double *delays, const double *alpha, double rho,
                      double *L_out, int *info);

/* predictTest(ttest::Vector{Vector}) of src/gpccfixdelay_marginaliseb.jl:259-289 at given (tau, alpha, rho):
 * joint predictive mean mu_out[sum Ntest] and covariance Sigma_out (column-major, + JITTER*I, :279) for
 * Ntest[l] test times per band (flattened in band order); also the training log-likelihood / info.
 * One augmented factorisation on the device: Sigma = cB - V'V, mu = V'w + Q* mu_b with V = L^-1 kB*. */
int gpcc_predict(gpcc_handle_t handle, const double *delays, const double *alpha, double rho,
                 const int *Ntest, const double *ttest, double *mu_out, double *Sigma_out,
                 double *loglik, int *info);

/* The posterior predictive at M rows (tau, alpha, rho) -- row-major M x L delays and alpha, rho[M], gpcc_loglik_batch's layout -- on one
 * set of test times shared by every row (Ntest[l] per band, flattened in band order in ttest, 1 <= T = sum Ntest <= 32768, as
 * gpcc_predict), and its average over the rows.  Per row m: mu_out[m, :] is gpcc_predict's mu_out, kB*' K^-1 (Y - bbar) + Q* mu_b, and
 * var_out[m, :] the diagonal of its Sigma_out, diag(cB) - diag(kB*' K^-1 kB*) + JITTER (1e-8; src/gpccfixdelay_marginaliseb.jl:275-285;
 * with marginalise_b == 0 no B term and the fixed-b offsets, src/gpccfixdelay.jl:244-266).  loglik[m] and info[m] are bitwise what
 * gpcc_loglik_grad_batch returns; where info[m] != 0 row m of mu_out and var_out is NaN and no other row is touched.
 * Mixture (weights != NULL, M entries): p_m = w_m / sum w, mix_mu = sum p_m mu_m, mix_var = sum p_m (var_m + (mu_m - mix_mu)^2), over
 * the rows in row order (a running weighted mean and sum of squared deviations); rows with p_m = 0 are skipped, failed or not; a failed
 * row with p_m > 0 makes mix_mu and mix_var NaN (the call still returns 0).  A negative or non-finite weight, or sum w = 0, returns
 * GPCC_ERR_ARGUMENT before any device work.  mix_mu and mix_var (T each) are required exactly when weights are given; mu_out and
 * var_out (M x T each, row-major) may then both be NULL (mixture only: the rows are never copied back); loglik and info are required.
 * Path: each group runs the gradient's assembly, factorisation, X = L^-1 and w = K^-1 r unchanged, then V = X kB* with fp64 MFMA over
 * the tiles of kB* generated on the fly (about N^3/3 + N^2 T flops per row on top of the factorisation), reduced to column sums of
 * squares, and kB*' w.  Always fp64 (an fp32 handle on its fp64 twin); a multi-device handle computes on device_ids[0].  Results are
 * bitwise repeatable and do not depend on the batch, its grouping or the stream / slot options.  Memory: the gradient's buffers, plus,
 * allocated on the first call with Tp = 128 ceil(T / 128): 12 Tp bytes of test points, 48 Tp bytes of mixture state, 8 M bytes of
 * weights, and for each of workspace_streams x workspace_slots slots 8 (nt + 2) Tp bytes (nt = Np / 128: the partial sums of squares,
 * one row of mu and var); they grow with T; a handle that never predicts allocates none of it.  Blocking. */
int gpcc_predict_batch(gpcc_handle_t h, int M, const double *delays, const double *alpha, const double *rho, const int *Ntest,
                       const double *ttest, const double *weights, double *mu_out, double *var_out, double *mix_mu,
                       double *mix_var, double *loglik, int *info);

/* The held-out (test) log-likelihood at M rows (tau, alpha, rho) -- gpcc_predict_batch's row layout -- on one test set shared by every
 * row (Ntest[l] points per band, flattened in band order in ttest, ytest and sigmatest; 1 <= T = sum Ntest <= 32768; Ntest[l] = 0
 * allowed), and its average over the rows.  Per row m: heldout[m] is predictTest(ttest, ytest, sigmatest) of
 * src/gpccfixdelay_marginaliseb.jl:311-325, logpdf(MvNormal(mu_pred, Sigma_pred + JITTER I + diag(sigmatest^2)), ytest) with
 * JITTER = 1e-8 and gpcc_predict's mu_pred and Sigma_pred (with marginalise_b == 0 the fixed-b model, src/gpccfixdelay.jl).  loglik[m]
 * and info[m]: the training log-likelihood, bitwise what gpcc_loglik_grad_batch returns, and
 *   info 0: success;  1 .. N (or < 0): the training matrix failed, as gpcc_loglik_batch reports it -- heldout[m] NaN;
 *   N + j (1 <= j <= T): the j-th pivot of the test block Sigma_pred + JITTER I + diag(sigmatest^2) is not positive (the case the
 *   reference catches with PosDefException at :327-341; its nearestposdef retry is host work, left to the caller) -- heldout[m] NaN,
 *   loglik[m] valid.  A failed row changes no other row.
 * Mixture (weights != NULL, M entries): p_m = w_m / sum w, mix_heldout = log sum_m p_m exp(heldout_m), a running max-shifted
 * log-sum-exp over the rows in row order (one row of weight 1 returns its own bits); rows with p_m = 0 are skipped, failed or not; a
 * failed row with p_m > 0 makes mix_heldout NaN (the call still returns 0).  A negative or non-finite weight, or sum w = 0, returns
 * GPCC_ERR_ARGUMENT before any device work.  mix_heldout is required exactly when weights are given; heldout may then be NULL
 * (mixture only: no row is copied back); loglik and info are required.
 * Path: each row factorises the augmented system [training | test] (the test points from the next tile boundary on,
 * with sigma*^2 + JITTER on their diagonal and y* - bbar* as their right-hand side) completely, with the launch-per-step tile kernels
 * of the gradient's factorisation; the trailing diagonal and the whitened test residual give the held-out value.
 * Always fp64 (an fp32 handle on its fp64 twin); a multi-device handle computes on device_ids[0].  Results are bitwise repeatable and
 * do not depend on the batch, its grouping or the stream / slot options.  Memory: allocated on the first call and grown with T, an
 * augmented workspace of nta (nta + 1) / 2 tiles per slot (nta = Np / 128 + ceil(T / 128); about 74 MB at N = 3277, T = 819) for as
 * many slots as fit a quarter of the device's memory (at most workspace_streams x workspace_slots; fewer: smaller groups, same
 * results, a note in gpcc_last_error), 28 (Np + 128 ceil(T / 128)) bytes of points and 28 M bytes of per-row state; a handle that
 * never calls this allocates none of it.  A size whose single slot does not fit returns GPCC_ERR_HIP with a message.  Blocking. */
int gpcc_heldout_loglik_batch(gpcc_handle_t h, int M, const double *delays, const double *alpha, const double *rho, const int *Ntest,
                              const double *ttest, const double *ytest, const double *sigmatest, const double *weights,
                              double *heldout, double *mix_heldout, double *loglik, int *info);

/* Exact leave-one-out (LOO) predictive scores at M rows (tau, alpha, rho) -- gpcc_predict_batch's row layout.  K, bbar and Y are
 * exactly objective(alpha, rho)'s (B included when b is marginalised); no JITTER is added: this is p(y_i | y_-i) of the model the
 * likelihood uses.  With G = K^-1 and w = G (Y - bbar), for every training point i, numbered in the CALLER'S order (band 1 as handed
 * to gpcc_create, then band 2, ...):
 *   var_i = 1 / G_ii,  mu_i = y_i - w_i / G_ii,  lp_i = -(log 2 pi + log var_i + (y_i - mu_i)^2 / var_i) / 2,  loo = sum_i lp_i.
 * mu_out, var_out and lp_out are M x N, row-major; loo is M; mix_lp is N; mix_loo is 1.  Every output may be NULL (loglik and info
 * too).  loglik[m] and info[m] are bitwise gpcc_loglik_grad_batch's (the same factorisation path), and
 *   info 0: success;  1 .. N (or < 0): the training matrix failed, as gpcc_loglik_batch reports it -- the row's outputs NaN;
 *   N + i (1 <= i <= N): point i is the first whose LOO variance is not positive and finite -- the row's mu, var, lp and loo NaN,
 *   loglik[m] valid.  A failed row changes no other row.
 * Mixture (weights != NULL, M entries): p_m = w_m / sum w.  With alpha and rho fixed per delay, the exact LOO density of the mixture
 * is the weighted HARMONIC mean of the rows' densities (p(y_i | y_-i) = p(y) / p(y_-i)):
 *   mix_lp_i = -log sum_m p_m exp(-lp_mi),  mix_loo = sum_i mix_lp_i,
 * one running max-shifted log-sum-exp per point over the rows in row order (one row of weight 1 returns its own bits); rows with
 * p_m = 0 are skipped, failed or not; a failed row with p_m > 0 makes mix_lp and mix_loo NaN (the call still returns 0).  A negative
 * or non-finite weight, or sum w = 0, returns GPCC_ERR_ARGUMENT before any device work, as does mix_lp or mix_loo without weights.
 * Path: the gradient's factorisation, X = L^-1 and w (gpcc_loglik_grad_batch without its tile products), then G_ii = sum_k X_ki^2 from
 * one read of the N^2 / 2 doubles of X (kernels: csrc/gpcc_loo.hip.h).  Always fp64 (an fp32 handle on its fp64 twin);
 * a multi-device handle computes on device_ids[0].  No atomics: bitwise repeatable, and a row's bits do not depend on M, the group,
 * the stream / slot options or the row order.  Memory: the gradient's buffers, 8 Np bytes per workspace slot, 8 M N bytes for each of
 * mu, var, lp that is asked for (lp also for the mixture), 8 M bytes, and with a mixture 32 N + 8 M bytes.  Blocking. */
int gpcc_loo_batch(gpcc_handle_t h, int M, const double *delays, const double *alpha, const double *rho, const double *weights,
                   double *mu_out, double *var_out, double *lp_out, double *loo, double *mix_lp, double *mix_loo, double *loglik,
                   int *info);

/* gpcc_loo_batch in LINEAR time for the Markov kernels (OU, Matern-3/2, Matern-5/2), exact: the same arguments, outputs, NULL rules,
 * weight checks and mixture.  The posterior of the process at training point i given every other observation is the two-filter combine
 * of gpcc_predict_markov_batch taken at the point itself -- the forward filter's state propagated to s_i = t_i - tau_band before its
 * update with point i, and the backward filter's likewise, the backward walk being the exact reverse of the forward merged order (ties
 * included), so that every other point is on exactly one side of i -- and with h of the point's band
 *   mu_i = h'm_s + mean(y_band),  var_i = h'P_s h + sigma_i^2.
 * Outputs are in the caller's order.  loglik[m] and info[m] (-1, -2, 1 .. N) are bitwise gpcc_loglik_markov_batch's; info[m] = N + i:
 * point i (1-based, the caller's order) is the first whose combine met a pivot, or whose variance is, not positive and finite -- the
 * row's mu, var, lp and loo NaN, loglik[m] valid.  Refusals: gpcc_loglik_markov_batch's (GPCC_ERR_UNSUPPORTED: rbf; marginalise_b with
 * L > 4).  Kernels: csrc/gpcc_markov_loo.hip.h (one lane per (row, direction), then one lane per (row, point)), DESIGN.md 4.20.  A row's
 * bits do not depend on M, the chunking, the row order or the launch shape.  Always fp64 (an fp32 handle on its fp64 twin); a
 * multi-device handle computes on device_ids[0].  Memory, grown on demand: gpcc_loglik_markov_batch's, 8 N bytes of point indices, the
 * tap scratch 16 N (n + n (n + 1) / 2) bytes per row of a chunk (n = p + L offsets <= 7; shared with gpcc_predict_markov_batch), the
 * chunk being the rows that fit 128 MiB (whole waves of 64 when it holds one; at least one row; option "markov_chunk_rows" > 0 sets
 * it), 24 N bytes per row of the chunk, 8 M bytes, and with a mixture 32 N + 8 M bytes; none of the N^2 workspace.  Blocking. */
int gpcc_loo_markov_batch(gpcc_handle_t h, int M, const double *delays, const double *alpha, const double *rho, const double *weights,
                          double *mu_out, double *var_out, double *lp_out, double *loo, double *mix_lp, double *mix_loo, double *loglik,
                          int *info);

/* Joint posterior draws of the light curves at M rows (tau, alpha, rho) -- gpcc_predict_batch's row layout -- on one test set shared by
 * every row (Ntest[l] points per band, flattened in band order in ttest; 1 <= T = sum Ntest <= 32768; Ntest[l] = 0 allowed).  One draw
 * of row m is f* = mu_pred + chol(Sigma_pred + JITTER I + diag(sigmatest^2)) zeta, zeta ~ N(0, I_T), with gpcc_predict's mu_pred and
 * Sigma_pred (src/gpccfixdelay_marginaliseb.jl:259-289) and JITTER = 1e-8: sigmatest == NULL draws the latent curve, sigmatest (T
 * entries) a replicated observation.  S >= 1.
 *   Per-row mode (weights == NULL): draws holds M S rows of T values, draw s of row m at row m S + s; draw_row (NULL or M S entries)
 *   receives m for each of them.
 *   Mixture mode (weights != NULL, M entries, rejected as gpcc_predict_batch rejects them): draws holds S rows; draw s uses the row
 *   draw_row[s] (required) = the first m with u_s c_{M-1} < c_m and w_m > 0, c_m = sum_{k <= m} w_k in row order.
 * Random numbers (csrc/gpcc_rng.h): Philox4x64-10, key (seed, 0).  Element j of draw s of row m is a Box-Muller normal of counter
 * (j / 4, s, m, 0) (m = 2^64 - 1 in mixture mode: the noise of a mixture draw does not depend on its row); u_s is word 0 of counter
 * (s, 0, 2^64 - 1, 1).  zeta (NULL, or the layout of draws) receives the normals each draw used.
 * Only rows with at least one draw are factorised (every row in per-row mode); the others get loglik NaN and info
 * GPCC_SAMPLE_NOT_DRAWN.  loglik and info of a factorised row are bitwise gpcc_heldout_loglik_batch's for the same row and test set
 * (info = N + j: the j-th pivot of the test block failed); a failed row's draws are NaN and change nothing else; the call returns 0.
 * Path: the held-out path's augmented factorisation with a test residual of 0, then gfx950 kernels: the mean
 * bbar* + L21 w1 once per row and test tile, and L22 zeta in fp64 MFMA with zeta generated in LDS.  Always fp64 (an fp32 handle on
 * its fp64 twin); a multi-device handle computes on device_ids[0].  Bitwise repeatable, and independent of the grouping, the stream /
 * slot options, fp32 vs fp64 handles and S (the first S' draws of a call with S > S' are the draws of a call with S').  Memory: the
 * held-out workspace (gpcc_heldout_loglik_batch, shared with it), plus 8 T' bytes per held-out slot (T' = 128 ceil(T / 128)), 8 D T
 * bytes for the draws (D = M S, or S) and as much again for zeta when asked for, 4 D + 4 M bytes of draw lists; a handle that never
 * samples allocates none of it, and bytes_per_slot is unchanged.  Blocking. */
int gpcc_sample_batch(gpcc_handle_t h, int M, const double *delays, const double *alpha, const double *rho, const int *Ntest,
                      const double *ttest, const double *sigmatest, const double *weights, int S, unsigned long long seed,
                      double *draws, int *draw_row, double *zeta, double *loglik, int *info);

/* gpcc_sample_batch's draws in LINEAR time for the Markov kernels (OU, Matern-3/2, Matern-5/2): the same arguments, modes and layouts
 * (no zeta: a draw takes 4 (N + T + 1) normals), the same distribution N(mu_pred, Sigma_pred + JITTER I + diag(sigmatest^2)) exactly,
 * other draws -- another linear map of other normals.  By Matheron's rule (kernels: csrc/gpcc_markov_sample.hip.h)
 *   f*_j = mu_j + g~_j - c_j + sqrt(JITTER + sigmatest_j^2) xi,
 * mu the mean of gpcc_predict_markov_batch, (r~, g~) a draw of the prior at the training and test points -- the state-space model of
 * gpcc_loglik_markov_batch simulated along the points merged by shifted time (x~ <- A(d) x~ + C xi with C C' = Pinf - A Pinf A', C the
 * triangular factor of that matrix scaled by diag(Pinf)^-1/2, eliminated from the last component; for lambda d <= 1 the matrix is
 * evaluated without cancellation, by incomplete-gamma series; tied points share one state), r~ with the observation noise, the offsets drawn from their prior when they are marginalised -- and c the smoother of gpcc_predict_markov_batch applied to r~ in place of Y - bbar.
 * O(N + T) work per draw; no T x T factor and nothing of the N^2 workspace.
 * Random numbers (csrc/gpcc_rng.h): Philox4x64-10, key (seed, 0), counter (e, s, m, 2) -- word 3 = 2 keeps the stream apart from
 * gpcc_sample_batch's normals (0) and the row picks (1) -- for draw s of row m (m = 2^64 - 1 in mixture mode).  e names a POINT, not
 * its place in the merge: e < N is training point e in gpcc_create's flattened order, N <= e < N + T test point e - N in the caller's
 * order, e = N + T the offsets.  Of the block's four Box-Muller normals the first p (the state dimension, 1 / 2 / 3) drive the
 * simulated state into that point and the fourth is its observation (training) or JITTER / sigmatest (test) noise; the block N + T
 * holds the L <= 4 offsets.  The mixture's rows are gpcc_sample_batch's: draw_row is identical for the same seed and weights.
 * Rows without a draw get loglik NaN and info GPCC_SAMPLE_NOT_DRAWN.  loglik and info of a drawn row are bitwise
 * gpcc_predict_markov_batch's for the same row and test set; a failed row's draws are NaN and change nothing else; the call returns 0.
 * Refusals (rbf; marginalise_b with L > 4) and the fp64 / multi-device rules are gpcc_predict_markov_batch's.  A draw's bits depend on
 * the seed, the row's parameters, s and m alone: not on M, S (the first S' draws of a call with S > S' are those of a call with S'),
 * the chunking, the row order in mixture mode, fp32 vs fp64 handles.
 * Memory, grown on demand (a handle that never calls this allocates none of it): gpcc_predict_markov_batch's buffers for a chunk of
 * rows (its rule, option "markov_chunk_rows") with 16 T n more bytes per row for the combine's weights (n = p + offset states); the
 * scratch of a chunk of draws, 8 (N + T) bytes per draw in flight, as many draws as fit 128 MiB in whole waves of 64 (at least one
 * wave; option "markov_sample_chunk_draws" > 0 sets the number), rounded up to 256; 8 D T bytes for the draws (D = M S, or S; shared
 * with gpcc_sample_batch); 4 (N + 3 D + M) bytes of lists.  Option "markov_sample_bytes" (read only) reports the weights, the scratch
 * and the lists.  Blocking. */
int gpcc_sample_markov_batch(gpcc_handle_t h, int M, const double *delays, const double *alpha, const double *rho, const int *Ntest,
                             const double *ttest, const double *sigmatest, const double *weights, int S, unsigned long long seed,
                             double *draws, int *draw_row, double *loglik, int *info);

/* gpcc_sample_markov_batch of rows that each carry their own noise model (kernel: csrc/gpcc_markov_noise_sample.hip.h, DESIGN.md
 * 4.30): kappa, nu (M x L row-major each; NULL: all 1 / all 0, as gpcc_loglik_noise_markov_batch) behind rho, every other argument,
 * mode and layout gpcc_sample_markov_batch's.  Point i of band l of row m is observed with v_i = kappa[m][l]^2 sigma_i^2 + nu[m][l];
 * the band means and Sigma_b stay the handle's.  The four steps of that entry change in one place each:
 *   prior draw   r~_i = alpha_b x~_1(s_i) + b~_b + sqrt(v_i) xi, v_i = fma(kappa_b^2, sigma_i^2, nu_b) formed on the lane, the expression
 *                of the other noise entries;
 *   correction   the filter of the draw walk updates with v_i; mu and the smoother's weights come from the taps of
 *                gpcc_predict_noise_markov_batch's kernel;
 *   result       sigmatest given: a test point of band b is a REPLICATED OBSERVATION under the fitted model, its noise
 *                sqrt(JITTER + fma(kappa_b^2, sigmatest^2, nu_b)) xi (sigmatest^2 staged as the rounded product).  sigmatest NULL: the
 *                LATENT curve, its noise sqrt(JITTER) xi -- nu is NOT added.  sigmatest of zeros asks for the latent curve plus the
 *                excess variance alone;
 *   normals      unchanged: the same Philox stream, the same counters (e, s, m, 2) naming points, the same row picks -- draw_row is
 *                gpcc_sample_markov_batch's for the same seed and weights.
 * CONSEQUENCES.  (1) A row's draws equal, to rounding, gpcc_sample_markov_batch's on a fresh handle created with the error bars
 * sqrt(v_i), sigmatest mapped the same way, with the SAME SEED: the counters name points, so the normals are the same.  (2) With
 * kappa = 1, nu = 0 (arrays or NULL) EVERY output -- draws, draw_row, loglik, info, in both modes -- is BITWISE
 * gpcc_sample_markov_batch's: fma(1, s2, 0) = s2, and the lane's correctly rounded sqrt(JITTER + sigmatest^2) is the number that
 * entry's host stages.  (3) loglik and info of a drawn row are bitwise gpcc_predict_noise_markov_batch's (the same tap launch);
 * info = -3 marks a kappa or nu that is negative or not finite, after -1 and -2: such a row's draws are NaN and no other row is
 * touched.  A row that receives no draw of the mixture is GPCC_SAMPLE_NOT_DRAWN and is never evaluated, whatever its kappa, nu.
 * (4) A draw's bits depend on the seed, the row's tau, alpha, rho, kappa, nu, s and (per-row mode) m alone: not on M, the row order,
 * "markov_chunk_rows", "markov_sample_chunk_draws" or the launch shape (points staged in LDS or not).
 * Refusals, argument and weight checks, 1 <= T <= 32768, the fp64 twin, the multi-device rule and "markov_count" are
 * gpcc_sample_markov_batch's.  Every <p, offsets> ships (no scratch memory).
 * Path: gpcc_markov_noise_draw, one lane per (row, draw) as gpcc_markov_draw; a lane's kappa^2 and nu sit in LDS behind that kernel's
 * region, 56 L bytes a lane instead of 40 L, so the points are staged in LDS up to a 16 L bytes per lane smaller N + T.
 * Memory: gpcc_sample_markov_batch's, plus 16 Mc L bytes for kappa | nu of the Mc drawn rows in the buffer
 * gpcc_loglik_noise_markov_batch stages them in (shared, grown on demand); none of the N^2 workspace.  Not here: noise in the dense
 * draws.  Blocking. */
int gpcc_sample_noise_markov_batch(gpcc_handle_t h, int M, const double *delays, const double *alpha, const double *rho,
                                   const double *kappa, const double *nu, const int *Ntest, const double *ttest,
                                   const double *sigmatest, const double *weights, int S, unsigned long long seed,
                                   double *draws, int *draw_row, double *loglik, int *info);

/* Posterior of the offsets b (src/gpccfixdelay_marginaliseb.jl:248-252): mu_postb[L], Sigma_postb[L x L]
 * (column-major, symmetrised).  The N x N solves (Sobs + K) \ [Q Y] run on the device as an augmented
 * factorisation; only the final L x L inverse is host arithmetic. */
int gpcc_posterior_offsets(gpcc_handle_t handle, const double *delays, const double *alpha, double rho,
                           double *mu_postb, double *Sigma_postb, int *info);

/* logpdf(MvNormal(mu, Sigma), x) for an explicit dense Sigma (column-major n x n; mu may be NULL = 0):
 * the test log-likelihood of predictTest(ttest, ytest, sigmatest), src/gpccfixdelay_marginaliseb.jl:311-343
 * (:325).  info > 0 is the PosDefException the reference catches at :327-341. */
int gpcc_mvnormal_logpdf(int n, const double *Sigma, const double *mu, const double *x, double *loglik,
                         int *info, int device_id);

/* delayedCovariance(kernel, scale, delays, rho, x, y) of src/delayedCovariance.jl:1-35 (pass
 * y == x, Ny == Nx for the 5-argument form, :38).  out is column-major (sum Nx) x (sum Ny).
 * Returns GPCC_ERR_ARGUMENT with the reference's message for scale <= 0 / rho <= 0. */
int gpcc_covariance(int kernel_id, int L, const double *scale, const double *delays, double rho,
                    const int *Nx, const double *x, const int *Ny, const double *y, double *out,
                    int device_id);

/* The per-delay model FIT for a whole grid of candidate delays -- what README.md:172-174 maps over
 * (`gpcc(...; delays = [0; d])[1]` for each d) -- as one call.  For each row of delays (G x L) and each
 * restart: the best of `initialrandom` random candidates (marginaliseb.jl:209) starts Nelder-Mead with
 * Optim's defaults and Options(iterations, g_tol = 1e-6) (:205-211) over the unconstrained parameters of
 * `unpack` (:112-126); the best restart wins (:222-226).  All G x numberofrestarts minimisations advance in
 * lock-step, every optimiser round being one gpcc_loglik_batch; each keeps its own trajectory.
 *   loglik_out[g] = -result.minimum (:351), alpha_out (G x L), rho_out[g] = the optimised hyper-parameters,
 *   info_out[g]   = 0, or 1 when no evaluated point was valid (loglik_out[g] = -Inf),
 *   iterations_out[g] (may be NULL) = Nelder-Mead iterations of the winning restart,
 *   stats_out (may be NULL) = {objective evaluations, batched rounds}.
 * init_params: numberofrestarts x initialrandom x (L+1) candidates in the optimiser's unconstrained
 * coordinates (the same for every delay: each reference gpcc call seeds its own generator with `seed`).  A
 * Julia caller draws them exactly as the reference does (MersenneTwister(seed), :160-196) and passes them;
 * NULL = drawn here with the same recipe from xoshiro256++(seed) (gpcc_initial_params shows them). */
int gpcc_grid_loglik(gpcc_handle_t h, int G, const double *delays, int iterations, int numberofrestarts,
                     int initialrandom, double rhomin, double rhomax, unsigned long long seed,
                     const double *init_params, double *loglik_out, double *alpha_out, double *rho_out,
                     int *info_out, int *iterations_out, long long *stats_out);

/* The candidates gpcc_grid_loglik uses when init_params == NULL (out: restarts x initialrandom x (L+1)). */
int gpcc_initial_params(gpcc_handle_t h, int numberofrestarts, int initialrandom, double rhomin, double rhomax,
                        unsigned long long seed, double *out);

/* The optimiser inside gpcc_grid_loglik on its own: P independent Nelder-Mead minimisations of dimension n in
 * lock-step (Optim.jl's NelderMead defaults as the reference uses them, marginaliseb.jl:205-211) over a batched
 * objective.  f(ctx, K, pidx, X, out) must write out[i] = objective of problem pidx[i] at row i of X (K x n);
 * NaN / +Inf = rejected point; non-zero return aborts with that code.  x0, xmin: P x n; fmin: P;
 * iterations_out (P) and stats_out ({evaluations, rounds}) may be NULL.  Host only; the tests pin this against the
 * numpy and the scalar restatements of the same algorithm. */
typedef int (*gpcc_batch_objective_t)(void *ctx, long K, const long *pidx, const double *X, double *out);
int gpcc_neldermead_batch(long P, int n, int iterations, double g_tol, const double *x0, gpcc_batch_objective_t f,
                          void *ctx, double *xmin, double *fmin, int *iterations_out, long long *stats_out);

/* Per-delay codes of gpcc_laplace_evidence / gpcc_newton_batch (negative: they cannot clash with a factorisation's pivot index). */
enum {
    GPCC_LAPLACE_NOT_CONVERGED = -10,   /* the polish did not converge within max_rounds evaluations (or its step collapsed) */
    GPCC_LAPLACE_NOT_MAXIMUM = -11,     /* -Hessian not positive definite at the last point */
    GPCC_LAPLACE_ON_BOUND = -12,        /* the mode lies on the box (gpcc_laplace_evidence: rho = rhomin or rhomax) */
    GPCC_LAPLACE_BAD_START = -13,       /* gpcc_newton_batch: the start was rejected (non-finite value) */
    GPCC_SAMPLE_NOT_DRAWN = -14         /* gpcc_sample_batch, gpcc_sample_markov_batch, gpcc_sample_noise_markov_batch: the row received no draw of the mixture and was not factorised */
};

/* The Newton polish of gpcc_laplace_evidence on its own (host only): P independent maximisations of l(u), u in R^n, in lock-step.
 * f(ctx, K, pidx, U, val, grad, hess) must write, for row i of U (K x n) of problem pidx[i], val[i] = l, grad[i] (n) and hess[i] (n x n,
 * row-major); a non-finite val = rejected point; non-zero return aborts with that code.  From u0 (P x n, clipped to the box lo..hi:
 * n entries each, NULL = unbounded), damped Newton: the step solves (-H + lambda I) d = g (lambda = 0, or Levenberg damping while -H
 * is not positive definite; coordinates on a bound with g pointing out stay fixed), is clipped to the box, accepted if l does not
 * decrease (beyond 1e-12 max(1, |l|), the rounding of an evaluated l) and halved otherwise.  Converged when the projected gradient's |.|_inf <= g_tol.  Outputs (P rows): umax, fmax = l(umax),
 * info (0 or GPCC_LAPLACE_*), and, each may be NULL: log_evidence = l + n/2 log(2 pi) - 1/2 log det(-H) (NaN where info != 0),
 * cov = (-H)^-1 (n x n; NaN unless -H is positive definite), rounds_out = evaluations per problem (the start included; at most
 * max_rounds), stats_out = {evaluations, batches}.  The (n x n) systems use an explicit scalar Cholesky without FMA contraction:
 * gpcc.jl_amd/laplace.py reproduces every step bitwise. */
typedef int (*gpcc_batch_hessian_t)(void *ctx, long K, const long *pidx, const double *U, double *val, double *grad, double *hess);
int gpcc_newton_batch(long P, int n, int max_rounds, double g_tol, const double *lo, const double *hi, const double *u0,
                      gpcc_batch_hessian_t f, void *ctx, double *umax, double *fmax, double *log_evidence, double *cov,
                      int *info, int *rounds_out, long long *stats_out);

/* The Laplace-marginalised evidence over alpha and rho at each of G delays (rows of delays, G x L), for the delay posterior
 * getprobabilities(log_evidence_out).  Prior: log-uniform in every alpha_l on (0, inf) and in rho on [rhomin, rhomax],
 * i.e. flat in u = (log alpha_1 .. log alpha_L, log rho), the same measure at every delay.  Its normalising constant (improper in alpha)
 * is common to all delays and cancels in getprobabilities: log_evidence_out is log Z(tau) UP TO ONE ADDITIVE CONSTANT SHARED BY ALL
 * DELAYS -- only differences and normalised probabilities mean anything.  tau is not marginalised.
 *   From (alpha0, rho0) per delay (usually gpcc_grid_loglik's output), gpcc_newton_batch's polish over u with log rho boxed to
 *   [log rhomin, log rhomax], every round one gpcc_loglik_hess_hyper_batch over the delays still active; gradient and Hessian in u:
 *   g_u = theta g_theta, H_u = diag(theta) H_theta diag(theta) + diag(theta g_theta), theta = (alpha, rho).  At the mode u^:
 *     log_evidence = l(u^) + (L+1)/2 log(2 pi) - 1/2 log det(-H_u(u^)).
 * Outputs (G rows): loglik_out = l(u^), alpha_out (G x L), rho_out = exp(u^), log_evidence_out, cov_out (may be NULL: G x (L+1)^2, the
 * posterior covariance (-H_u)^-1 of u), info_out: 0, GPCC_LAPLACE_NOT_CONVERGED / _NOT_MAXIMUM / _ON_BOUND (NaN log_evidence), or the
 * device's code (pivot index, -1, -2) where the start itself could not be evaluated (NaN loglik and log_evidence); rounds_out (may be
 * NULL) = Newton rounds per delay (the start's evaluation included), stats_out (may be NULL) = {evaluations, batches}.  fp64 on any
 * handle (as the Hessian).  Blocking. */
int gpcc_laplace_evidence(gpcc_handle_t h, int G, const double *delays, const double *alpha0, const double *rho0, double rhomin,
                          double rhomax, int max_rounds, double g_tol, double *loglik_out, double *alpha_out, double *rho_out,
                          double *log_evidence_out, double *cov_out, int *info_out, int *rounds_out, long long *stats_out);

/* `unpack` of marginaliseb.jl:112-126 for M parameter vectors X (M x (L+1)): alpha = makepositive(x[1:L]) + 1e-8,
 * rho = transformbetween(x[L+1], rhomin, rhomax).  MiscUtil.jl's source is not part of the reference tree:
 * makepositive is taken to be softplus, transformbetween(x, a, b) = a + (b - a) / (1 + exp(-x)).  Host only. */
int gpcc_unpack_params(int M, int L, const double *X, double rhomin, double rhomax, double *alpha, double *rho);

/* getprobabilities(loglikel[, logpriorpdfvalues]) of src/getprobabilities.jl:1-20;
 * logprior == NULL is the 1-argument form (log-prior of ones, :3). */
int gpcc_probabilities(int G, const double *loglik, const double *logprior, double *out,
                       int device_id);
int gpcc_probabilities_device(int G, const double *d_loglik, const double *d_logprior,
                              double *d_out, void *stream);

/* Per-kernel HIP-event timing (bench.py's roofline leg).  While enabled every launch is
 * bracketed by events on its own stream and groups run on ONE stream. */
enum {
    GPCC_PROF_ASSEMBLE = 0,     /* gpcc_assemble_tiles     -- HBM-bound */
    GPCC_PROF_PANEL_UPDATE = 1, /* gpcc_panel_update       -- fp64 MFMA, dominant */
    GPCC_PROF_DIAG = 2,         /* gpcc_diag_factor */
    GPCC_PROF_TRSM = 3,         /* gpcc_panel_trsm         -- fp64 MFMA */
    GPCC_PROF_REFINE = 4,       /* fp32 mode: backward solve + X' K0 X + final arithmetic */
    GPCC_PROF_SMALL_STEP = 5,   /* gpcc_small_step: trailing update + next diagonal step in one launch (a few evaluations) */
    GPCC_PROF_SMALL_EVAL = 6,   /* gpcc_small_eval / gpcc_smallw_eval: a whole evaluation (assembly + Cholesky + solve) of N <= 383 points in one or four waves */
    GPCC_PROF_COUNT = 7
};
int gpcc_profile_enable(gpcc_handle_t handle, int on);
int gpcc_profile_reset(gpcc_handle_t handle);
int gpcc_profile_get(gpcc_handle_t handle, int which, long *launches, double *total_ms);

/* On-device self-test of the f64 MFMA fragment maps and a timing probe of the fp64 MFMA rate:
 * returns 0 when the maps are as the kernels assume; *tflops (may be NULL) = measured rate. */
/* Measurement plumbing of the persistent few-evaluation launch (option "chain_max"): with option "chain_trace" = 1 its chain
 * workgroups stamp the device's wall clock per diagonal step k, 80 stamps each; out_us[80 k + 0 / 1 / 2] = microseconds (from the
 * first stamp of the evaluation) at which the workgroup of step k began to build tile (k,k), had it complete (first pivot next), had
 * published the whole step; [80 k + 8 + 8 jb + 0 .. 7] = block step jb of the diagonal step: begins, wave 0 done, behind its first
 * barrier, behind its second; wave 0: fold done, block loaded, factored, stored; -1 where nothing was stamped.  `evaluation` = index in the last group of at most
 * chain_max evaluations; capacity >= 80 nt doubles (nt = Np / 128).  tools/chain_trace.py prints the critical chain from it. */
int gpcc_chain_trace(gpcc_handle_t handle, int evaluation, double *out_us, int capacity);
/* ... and the workers' jobs of the same launch: rows of 6 doubles [kind (1 quarter-tile solve, 2 tile update), step k, index in the step,
 * fetched, dependencies met, done] (microseconds from the first fetch), at most capacity_rows (32768 are kept per launch). */
int gpcc_chain_jobs_trace(gpcc_handle_t handle, double *out, long capacity_rows, long *rows_out);

int gpcc_selftest(int device_id, double *mfma_f64_tflops);

#ifdef __cplusplus
}
#endif
#endif
