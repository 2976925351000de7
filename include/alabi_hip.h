/*
 * alabi_hip.h -- C ABI of libalabi_hip.so, the MI355X (gfx950) implementation of the
 * GP-surrogate + ensemble-MCMC hot path of jbirky/alabi.
 *
 * The reference has no FFI: it reaches this arithmetic through the Python object
 * protocols of two third-party packages (george.GP, emcee.EnsembleSampler).  Each entry
 * point below names the reference call site (path:line under /root/reference) whose work
 * it replaces; INTEGRATION.md shows the ctypes binding a maintainer adds on the alabi side.
 *
 * Conventions
 *   - All array arguments are DEVICE pointers to float64 / int32 / int64 unless marked
 *     "host".  They are owned by the caller (PyTorch-ROCm tensors' data_ptr()).
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Work is
 *     enqueued on it; only the calls documented as synchronising wait for it.
 *   - Every call returns an int status; no exception crosses the boundary.
 *   - A handle is not thread-safe; distinct handles are independent.
 *   - Everything computes in IEEE fp64.
 */
#ifndef ALABI_HIP_H
#define ALABI_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define ALABI_OK 0
#define ALABI_NOT_POSITIVE_DEFINITE 1 /* Cholesky met a pivot <= 0 or NaN (see alabi_gp_last_pivot) */
#define ALABI_BAD_ARGUMENT 2
#define ALABI_HIP_ERROR 3
#define ALABI_NOT_COMPUTED 4          /* predict / set_y before a successful compute */
#define ALABI_TIMEOUT 5               /* persistent ensemble kernel: a bounded spin ran out (state is invalid; re-run
                                         with ALABI_ENS_STREAM=0) */

#define ALABI_UTILITY_BAPE 0
#define ALABI_UTILITY_AGP 1
#define ALABI_UTILITY_JONES 2

#define ALABI_MAX_DIM 64

typedef struct alabi_gp alabi_gp;
typedef struct alabi_ens alabi_ens;
typedef struct alabi_ns alabi_ns;
typedef struct alabi_kde alabi_kde;

/* Library / device --------------------------------------------------------------------- */
int alabi_abi_version(void);
const char* alabi_status_string(int status);
const char* alabi_last_error(void);            /* text of the last HIP error on this thread */
int alabi_device_info(int* n_cu, int* lds_bytes, char* arch /* >=64 bytes, host */);

/* GP object: replaces george.GP(kernel=var(y)*ExpSquaredKernel(metric, ndim), mean=,
 * white_noise=)  -- alabi/core.py:1000, :1141; alabi/gp_utils.py:230-233. ---------------- */
int alabi_gp_create(int n_cap, int d, alabi_gp** out);
int alabi_gp_destroy(alabi_gp* gp);

/* gp.set_parameter_vector(p) -- alabi/core.py:705-733, :1157.  log_M is a host array[d];
 * all three log_* values are natural logs (george convention). */
int alabi_gp_set_hyper(alabi_gp* gp, double mean, double log_white_noise, double log_amp,
                       const double* log_M);
/* Kernel family: 0 ExpSquaredKernel (default), 1 Matern32Kernel, 2 Matern52Kernel, 3 RationalQuadraticKernel
 * (log_alpha used by 3 only) -- the four choices of init_gp(kernel=), alabi/core.py:1000-1014. */
int alabi_gp_set_kernel(alabi_gp* gp, int kernel_type, double log_alpha);

/* gp.compute(X) -- alabi/core.py:1158, :1430, :1577; gp_utils.py:243.  Assembles
 * K = k(X,X) + exp(log_white_noise) I and factorises it (lower Cholesky).  X is [N,d]
 * row-major on the device.  SYNCHRONISES the stream (it returns the factorisation status).
 * Returns ALABI_NOT_POSITIVE_DEFINITE where LAPACK's potrf would report info > 0. */
int alabi_gp_compute(alabi_gp* gp, const double* X, int N, void* stream);
int alabi_gp_last_pivot(alabi_gp* gp, int* pivot /* host, 1-based like LAPACK info */);

/* Batched fit + held-out mean: the k-fold cross-validation search of init_gp / _opt_gp -- alabi/gp_utils.py:511-637
 * (_evaluate_candidate_worker: per fold deepcopy(gp), set_parameter_vector, compute(train), log_likelihood, predict(val)) mapped
 * over the candidates by a process pool at gp_utils.py:640-700; alabi/core.py:1287-1305.  ONE call evaluates `njobs`
 * (hyper-parameter vector, training rows, validation rows) triples that share the resident inputs X [n,d] and y [n] (device):
 * every kernel matrix is assembled, all are factorised in one launch of the task queue (the chains of different matrices run side
 * by side), alpha / log-likelihood / held-out mean follow in two launches, one read-back.
 *   hyper      host [njobs][4 + d]: mean, log white noise, log amplitude, log alpha (RationalQuadratic only), log M_1..d
 *   train_idx  device int32, the training rows of job b are train_idx[train_off[b] .. train_off[b+1]) (offsets: host int64)
 *   val_idx    the same for the validation rows (may be empty); mu_val [val_off[njobs]] receives the held-out means
 *   nll        host [njobs]: -log-likelihood of the training rows (+inf where K is not positive definite)
 *   status     host [njobs]: 0, or LAPACK's 1-based pivot index where the factorisation broke down (mu_val is then NaN)
 * Jobs are processed in chunks whose matrices fit `workspace_bytes` (0: ALABI_BATCH_BYTES or 16 GiB, at most half of the free memory).  Factors are bit-identical
 * to alabi_gp_compute on the same rows.  Synchronises with `stream`.  N <= 12288 per job. */
typedef struct alabi_gp_batch alabi_gp_batch;
int alabi_gp_batch_create(int d, int kernel_type, long long workspace_bytes, alabi_gp_batch** out);
int alabi_gp_batch_destroy(alabi_gp_batch* batch);
int alabi_gp_batch_fit_predict(alabi_gp_batch* batch, const double* X, const double* y, int n, int njobs,
                               const double* hyper /* host */, const int* train_idx, const long long* train_off /* host */,
                               const int* val_idx, const long long* val_off /* host */, double* mu_val,
                               double* nll /* host */, int* status /* host */, void* stream);
/* The row lists of a k-fold split for `ncand` candidates at once (alabi/gp_utils.py:538: sklearn KFold(shuffle=True).split yields
 * ascending train and validation rows): fold_of [ncand, n] int8 = the fold of every row under each candidate's shuffle (-1: unused
 * row); job c k + f gets fold f's rows in val_idx[val_off[job] ..) and the other used rows in train_idx[train_off[job] ..).  All
 * arrays on the device (offsets int64 [ncand k + 1], computed by the caller from the fold sizes). */
int alabi_cv_fold_lists(const signed char* fold_of, int ncand, int n, int k, const long long* train_off,
                        const long long* val_off, int* train_idx, int* val_idx, void* stream);
/* Factor [N,N] (zeros above the diagonal) / alpha [N] of a job of the LAST chunk processed (tests: bit-identity with the
 * single-matrix path); ALABI_BAD_ARGUMENT for a job of an earlier chunk. */
int alabi_gp_batch_get_factor(alabi_gp_batch* batch, int job, double* L_out, void* stream);
int alabi_gp_batch_get_alpha(alabi_gp_batch* batch, int job, double* alpha_out, void* stream);
/* Chunks whose queue launch ran into a bounded wait and were redone on the launch-per-step path (expected: 0). */
int alabi_gp_batch_timeouts(alabi_gp_batch* batch, int* count /* host */);

/* Extend the factorisation by ONE training point x_new[d] (device) with the hyper-parameters unchanged: the refit after every
 * active-learning iteration (alabi/core.py:1780 -> _fit_gp -> gp.compute at :1158) in O(N^2) through the cached L^-1 instead
 * of O(N^3).  Needs a free padding row (N not a multiple of 64 and N < n_cap): ALABI_BAD_ARGUMENT otherwise -- call
 * alabi_gp_compute then.  ALABI_NOT_POSITIVE_DEFINITE (alabi_gp_last_pivot: N + 1) leaves the factor, the training set and alpha
 * as they were: every prediction of the old factor is bit for bit what it was.  Success invalidates alpha (call alabi_gp_set_y).
 * SYNCHRONISES the stream. */
int alabi_gp_append(alabi_gp* gp, const double* x_new, void* stream);

/* Change the constant mean only (it does not enter K): keeps the factorisation, invalidates alpha. */
int alabi_gp_set_mean(alabi_gp* gp, double mean);

/* alpha = K^-1 (y - mean): george _compute_alpha inside gp.predict -- alabi/core.py:85. */
int alabi_gp_set_y(alabi_gp* gp, const double* y, void* stream);

/* gp.predict(y, Xs, return_var=) -- alabi/core.py:85, :95, :1441, :1486, :1601, :1812.
 * Xs is [M,d] row-major; mu[M]; var[M] or NULL (mean only).  White noise is not added
 * to var.  var may come out slightly negative from cancellation, as in the reference.
 * The first variance request after a factorisation builds and caches L^-1 (Npad^2 doubles,
 * about 0.25 ms at N = 2000); var = amp - |L^-1 k*|^2 is then a product on the matrix cores.
 * Without room for the cache the blocked forward substitution is used (same values to ~1e-14 amp). */
int alabi_gp_predict(alabi_gp* gp, const double* Xs, long long M, double* mu, double* var,
                     void* stream);

/* One held-out evaluation of a hyper-parameter vector: gp.compute(X) + gp.log_likelihood(y) + gp.predict(y, Xs) as the k-fold
 * cross-validation of the reference does per fold (alabi/gp_utils.py:568-600) -- the three calls in one, so that a search of
 * 875 folds does not pay the binding's per-call overhead three times.  nll_out is a host double (-log likelihood); mu[M] on
 * the device; M may be 0.  Same status codes as the three calls (NOT_POSITIVE_DEFINITE leaves the handle uncomputed). */
int alabi_gp_fit_predict(alabi_gp* gp, const double* X, int N, const double* y, const double* Xs, long long M,
                         double* mu, double* nll_out, void* stream);

/* Prediction with gradients with respect to the query point, for the acquisition optimiser:
 * grad_gp_mean_prediction / grad_gp_var_prediction -- alabi/utility.py:558-623, which difference the kernel numerically
 * (utility.py:511-555, step 1e-6) and form K^-1 explicitly (solver.get_inverse(), utility.py:610).  Here
 * dmu[M,d] = (dk / dx)^T alpha and dvar[M,d] = -2 (dk / dx)^T K^-1 k with the closed-form kernel derivative and
 * K^-1 k = W^T (W k), W = cached L^-1; queries are processed 16 at a time.  mu[M] / var[M] may be NULL.
 * All pointers are device pointers.  ALABI_HIP_ERROR when there is no room for the L^-1 cache. */
int alabi_gp_predict_grad(alabi_gp* gp, const double* Xs, long long M, double* mu, double* var,
                          double* dmu, double* dvar, void* stream);
/* The same for ONE point with host buffers on both sides -- the evaluation the polish step of find_next_point makes ~30 times per
 * active-learning iteration (alabi/utility.py:1030-1163 calls the objective and its gradient point by point): x [d] in, out [2 + 2 d] =
 * mu, var, dmu[d], dvar[d]; pinned staging buffers of the handle, one synchronisation. */
int alabi_gp_predict_grad_point(alabi_gp* gp, const double* x /* host [d] */, double* out /* host [2 + 2 d] */, void* stream);

/* solver.log_determinant and -gp.log_likelihood(y) -- alabi/core.py:1248; gp_utils.py:139.
 * Both SYNCHRONISE the stream and write one host double. */
int alabi_gp_logdet(alabi_gp* gp, double* out, void* stream);
int alabi_gp_nll(alabi_gp* gp, double* out, void* stream);

/* d logL / d p of the log marginal likelihood at the current hyper-parameters, analytic:
 * 0.5 tr((alpha alpha^T - K^-1) dK/dp) and sum(alpha) for the mean.  Replaces george's
 * gp.grad_log_likelihood(y) (reference call sites alabi/core.py:1261, alabi/gp_utils.py:165).
 * grad_out (HOST, d + 4 doubles): [mean, log white noise, log amplitude, log alpha (0 unless the kernel is the
 * rational quadratic), log_M_0 .. log_M_{d-1}].  Needs alabi_gp_compute and alabi_gp_set_y.  Synchronises. */
int alabi_gp_grad_log_likelihood(alabi_gp* gp, double* grad_out, void* stream);

/* Inspection (tests, GP-protocol adapter: gp._alpha, utility.py:577; solver factor). */
int alabi_gp_get_alpha(alabi_gp* gp, double* alpha_out /* [N] */, void* stream);
int alabi_gp_get_factor(alabi_gp* gp, double* L_out /* [N,N] row-major, upper part zero */,
                        void* stream);
/* gp.solver.get_inverse() -- alabi/utility.py:610 (the finite-difference acquisition gradient): K^-1 [N,N] row-major, both
 * triangles, = W^T W on the matrix cores from the cached W = L^-1 of the current factor (built on demand). */
int alabi_gp_get_inverse(alabi_gp* gp, double* Kinv_out, void* stream);
int alabi_gp_n(alabi_gp* gp, int* n /* host */);
/* How the last alabi_gp_compute factorised (tests, soak runs): 0 = not computed, 1 = launch per step, 2 = the one-launch task queue,
 * 3 = the queue's wait ran out and the matrix was assembled and factorised again step by step. */
int alabi_gp_last_factor_path(alabi_gp* gp, int* path /* host */);
/* Which kernels produced the handle's current alpha (the last alabi_gp_set_y): 0 = none yet, 1 = the one-launch dataflow solve,
 * 2 = launch per block step (ALABI_TRSV_STREAM=0, more than 200 block rows, or within 256 solves of a time-out), 3 = the dataflow
 * solve's wait ran out and the launch-per-step kernels solved again. */
int alabi_gp_last_solve_path(alabi_gp* gp, int* path /* host */);

/* kernel.get_value(x1, x2) -- alabi/utility.py:549, :607.  K_out is [n1,n2] row-major,
 * no white noise. */
int alabi_kernel_matrix(const double* X1, int n1, const double* X2, int n2, int d,
                        int kernel_type, double log_alpha, double log_amp,
                        const double* log_M /* host [d] */, double* K_out, void* stream);

/* Acquisition scan: utility.bape_utility / agp_utility / jones_utility evaluated on M
 * candidates + the arg-min that utility.minimize_objective takes over restarts --
 * alabi/utility.py:729-810, :629-701, :853-946, :1149-1163; alabi/core.py:1601-1621.
 * Xs [M,d]; bounds host [d,2]; u [M] or NULL; best_val / best_idx are HOST outputs
 * (SYNCHRONISES).  Candidates outside the open box get +inf. */
int alabi_utility_scan(alabi_gp* gp, int algo, const double* Xs, long long M,
                       const double* bounds, double y_best, double* u, double* mu_out,
                       double* var_out, double* best_val, long long* best_idx, void* stream);
/* Continuous polish of an acquisition optimum: projected limited-memory BFGS from x0 inside the (open) box, value and gradient of the
 * acquisition function from ONE alabi_gp_predict_grad_point per evaluation, the optimiser itself on the host beside it.  Stands for the
 * local optimisation of alabi/utility.py:1030-1163 (scipy L-BFGS-B around one prediction per objective call) on top of the batched
 * scan; never worse than x0.  bounds [d][2], x0 / x_out [d], all host; *nevals = evaluations made. */
int alabi_utility_polish(alabi_gp* gp, int algo, const double* x0, const double* bounds, double y_best, int maxiter,
                         double* x_out, double* u_out, int* nevals, void* stream);
/* The epilogue alone on caller-supplied (mu, var): used by the parity tests. */
int alabi_utility_eval(int algo, const double* Xs, long long M, int d, const double* bounds,
                       double y_best, const double* mu, const double* var, double* u,
                       void* stream);

/* Ensemble sampler: replaces emcee.EnsembleSampler(W, d, sm.lnprob).run_mcmc(p0, nsteps)
 * with the StretchMove -- alabi/core.py:2319-2325, lnprob = surrogate mean + box prior
 * (alabi/core.py:2073-2100, utility.py:218-275).  n_ensembles >= 1 independent ensembles of
 * W walkers each ("independent chains") share every launch; walker ids are global
 * (ensemble e owns rows [e*W, (e+1)*W) of coords / logp / chain) and walkers only interact
 * inside their ensemble.  bounds is a host array [d,2] in the GP's (scaled) coordinates. */
int alabi_ens_create(alabi_gp* gp, int W, int d, int n_ensembles, const double* bounds,
                     unsigned long long seed, alabi_ens** out);
/* alabi_ens_create for Metropolis sets, which need no complementary half: W >= 1.  On a handle with W == 1 alabi_ens_set_moves,
 * alabi_ens_run and alabi_ens_draw are ALABI_BAD_ARGUMENT unless every move of the table is a Gaussian move (kind 5). */
int alabi_ens_create_metropolis(alabi_gp* gp, int n_walkers, int d, int n_ensembles, const double* bounds,
                                unsigned long long seed, alabi_ens** out);
int alabi_ens_destroy(alabi_ens* ens);
/* Independent normal priors on selected coordinates on top of the uniform box: the reference's lnprior_normal
 * (alabi/utility.py:370-378; passed to run_emcee as prior_fn, alabi/core.py:2108).  mean[d], std[d] on the HOST in the
 * sampler's coordinates; a non-finite mean or std <= 0 means "no normal prior on this coordinate".  Adds
 * sum_k norm.logpdf(x_k, mean_k, std_k) to the log-probability.  Takes effect from the next call on. */
int alabi_ens_set_normal_prior(alabi_ens* ens, const double* mean, const double* std);

/* Log-probability inside the box = scale * (GP mean) + shift.  Default (1, 0) is the reference's lnprob with identity
 * scalers; an affine y_scaler (alabi/core.py:1483-1502: y = y_scaler.inverse_transform(gp.predict(...))) sets its slope and
 * offset here, an affine theta_scaler is absorbed by running the ensemble in scaled coordinates (the stretch move is
 * affine-invariant).  scale > 0.  Affects alabi_ens_lnprob / run / half_step from the next call on. */
int alabi_ens_set_logp_affine(alabi_ens* ens, double scale, double shift);

/* Non-affine y scalers the reference ships (alabi/utility.py:62-71; un-scaling per prediction at alabi/core.py:1483-1502):
 * the log-probability becomes map(scale * GP mean + shift) with kind 0 identity (default), 1 nlog_scaler's inverse -10^x,
 * 2 log_scaler's inverse 10^x.  Applied inside every ensemble kernel, once per proposal. */
int alabi_ens_set_logp_map(alabi_ens* ens, int kind);

/* Proposal moves, emcee's EnsembleSampler(moves=...) (documented by the reference as sampler_kwargs['moves'], "Custom proposal
 * moves", alabi/core.py:2144, and handed to emcee.EnsembleSampler at alabi/core.py:2319).  A table of n <= 8 moves, all HOST
 * arrays: kind 0 = StretchMove with p0 = a (> 1); kind 1 = DEMove (emcee 3 moves/de.py) with p0 = gamma0 and p1 = sigma,
 * proposal q = s + gamma0 (1 + sigma n) (C[j2] - C[j1]), n standard normal, j1 != j2 drawn from the complementary set, log
 * factor 0; kind 2 = SnookerMove, the snooker update of ter Braak & Vrugt (2008, eq. 4) on the sampler's two-way split, with
 * p0 = gammas (finite) and p1 = 0: three distinct walkers z = C[j1], z1 = C[j2], z2 = C[j3] of the complementary set, e the unit
 * vector from z to s, q = s + gammas (e.z1 - e.z2) e, log factor (d - 1) (ln|q - z| - ln|s - z|) formed by the kernel that forms
 * q (j3 from Philox stream 5, word 0, at the walker).  This is the published rule, not emcee 3's DESnookerMove, whose factor is
 * half of it.  cum = np.cumsum(w / w.sum()) in fp64: ONE move is chosen per step and ensemble, index = #{k: cum[k] <= u}
 * (clipped to n - 1) with u from Philox stream 3 at the ensemble's walker 0.  n = 0 restores the default (one stretch move with
 * the `a` of each call); with n > 0 the `a` arguments of run / draw / export_draws are not used.  Streams 0-2 (labels, u_z and
 * partner, u') do not depend on the moves, streams 3-4 not on a snooker move.  A set holding a DE move needs W >= 4, one holding a
 * snooker move W >= 6; either runs alabi_ens_run with one launch per half step (a snooker set: one proposal per workgroup) and
 * is refused by the sharded run.  Takes effect from the next call on.
 * kind 3 = WalkMove (Goodman & Weare 2010; emcee 3 moves/walk.py) with p0 = s0, the size of the subset J of the complementary half
 * (0: the whole half) and p1 = 0: q = s + sum_{j in J} z_j (C[j] - mean_J) / sqrt(s0 - 1), z_j standard normal, log factor 0 -- a
 * draw from the Gaussian with the sample covariance of the subset.  Needs 2 <= s0 <= W / 2 (the smaller half; integral) and
 * (W + 1) / 2 <= 2048.  kind 4 = KDEMove (emcee 3 moves/kde.py) with p0 / p1 = the bandwidth factor f (> 0) of split 0 / split 1
 * (the halves of an odd W differ in size; scipy.stats.gaussian_kde's scotts_factor / silverman_factor / scalar, resolved by the
 * caller): once per half step the mean, the unbiased covariance and the Cholesky factor L of f^2 cov of the complementary half,
 * q = C[r] + L z, log factor kde.logpdf(s) - kde.logpdf(q).  Needs W / 2 >= d + 1.  A factorisation with a pivot that is not
 * positive and finite (emcee would raise LinAlgError) rejects every proposal of that half step and ensemble and is counted
 * (alabi_ens_kde_singular).  The subset, r and the normals come from Philox streams 6-8 where the proposal is formed (layout in
 * ensemble.hip); streams 0-5 do not depend on these moves.  Both run like a snooker set: one launch per half step, one proposal
 * per workgroup, in front of every half step of a set with a KDE move one pre-pass launch; refused by the sharded run.  A
 * violated bound is ALABI_BAD_ARGUMENT.
 * kind 5 GaussianMove (emcee 3 moves/gaussian.py: a Metropolis proposal q = x + f C z around the walker, log factor 0): p0 = ln
 * factor >= 0 (0: no scale factor, f = 1; otherwise f = exp(v), v ~ U(-ln factor, ln factor), ONE draw per step and ensemble), p1 =
 * mode: 0 moves every coordinate, 1 one coordinate drawn per walker and step, 2 coordinate (step mod d).  The lower-triangular
 * scale factor C travels apart from the table and AHEAD of it: alabi_ens_set_move_scale(ens, k, ...) for every Gaussian move k,
 * then alabi_ens_set_moves, which is ALABI_BAD_ARGUMENT for a kind-5 move whose slot has been given no factor since the last
 * table was set (or, in modes 1 and 2, a factor that is not diagonal): a table never holds a Gaussian move it cannot run.  Draws: Philox counter (step, global walker id, stream word S + 16 b) --
 * S = 9, b = 0: v = (2 u53(r0, r1) - 1) ln factor at the ensemble's walker 0; S = 9, b = 1: the coordinate of mode 1,
 * (r0 d) >> 32, at the walker; S = 10, b = k: the normal z_k (Box-Muller as stream 4); accept uniform and move choice are streams
 * 2 and 3 as for every move; streams 0-8 do not depend on a Gaussian move.  Arithmetic: s_k = sum_{i <= k} C[k][i] z_i, i
 * ascending, by fma from 0 (a diagonal C: the single term), q_k = fma(f, s_k, x_k); in modes 1 and 2 every other coordinate is
 * copied.  A proposal reads nothing of the other half, so in the launch-per-half-step kernels (mixtures with red-blue moves, host
 * callables, alabi_ens_set_stream(ens, 0)) a full Metropolis step is the rule applied to split 0 and then to split 1.  A table of
 * Gaussian moves alone runs on ens_mh_kernel (path 4 of alabi_ens_last_path): one workgroup per walker, every step of a chunk in
 * one launch, the same bits as path 0; it accepts W == 1.  Such a table runs on path 0 instead -- alabi_ens_last_path says so, the
 * results are the same -- after alabi_ens_set_stream(ens, 0), with ALABI_ENS_MH=0 in the environment, with workgroups of more
 * than 512 lanes (ALABI_ENS_THREADS=1024) or where its factors need more than 128 KB of LDS (more than four moves at d = 64).
 * ALABI_ENS_MH_CHUNK=k caps the steps of one launch at k; both variables are read at every alabi_ens_run.  Refused by the
 * sharded run.
 * kind 6 HMCMove (Hamiltonian Monte Carlo on the closed-form gradient of the ensemble's log-probability; n_leapfrog = 1 is MALA):
 * p0 = step size > 0, resolved by the caller; p1 = n_leapfrog + q / 512 with n_leapfrog in 1 ... 64 and q = ln jitter rounded to a
 * multiple of 2^-36 (0: none; ln jitter < 512), so both parts come apart exactly.  The scale factor C (C C^T = cov, an estimate of
 * the posterior covariance: the mass matrix is cov^-1) travels by alabi_ens_set_move_scale ahead of the table, as for kind 5, and
 * alabi_ens_set_moves is ALABI_BAD_ARGUMENT for a kind-6 move whose slot has no factor, for a step size that is not positive and
 * finite, for n_leapfrog outside 1 ... 64 and for a table that mixes kind 6 with another kind.  One step of walker x with
 * lp = lnp(x), g = grad lnp(x), in whitened momentum: z0 ~ N(0, I); e = p0 f, f = 1 or exp(v), v ~ U(-ln jitter, ln jitter), ONE
 * draw per step and ensemble; z = z0 + (e / 2) C^T g; n_leapfrog times q = q + e C z (from q = x), (lp_q, g_q) = lnp and its
 * gradient at q, z = z + e C^T g_q (e / 2 the last time); accept iff lp_q - |z|^2 / 2 - lp + |z0|^2 / 2 > ln u' and q lies in the
 * open box; NaN anywhere rejects.  Only the end point is tested against the box; in between the trajectory follows the GP mean's
 * smooth extension (lnp there: GP mean through the folded scalers, the y map, the normal priors, no box gate).  Draws: Philox
 * counter (step, global walker id, stream word S + 16 b) -- S = 11, b = k: the momentum normal z0_k at the walker (Box-Muller as
 * stream 4); S = 12, b = 0: v = (2 u53(r0, r1) - 1) ln jitter at the ensemble's walker 0, not drawn without jitter; accept uniform
 * and move choice are streams 2 and 3 as for every move; streams 0-10 keep their meaning.  (S = 11 at b >= 64 -- word
 * 11 + 16 (64 (i + 1) + k) -- is the momentum normal of iteration i, coordinate k of alabi_ens_find_step_size, which consumes no
 * step: kinds 6 and 7 read b = k < 64 only.)  Such a table runs on ens_hmc_kernel
 * (path 5 of alabi_ens_last_path) and on nothing else: one workgroup per walker, every step of a chunk in one launch, any W >= 1
 * and any n_ensembles; alabi_ens_set_stream does not move it, and alabi_ens_run is ALABI_BAD_ARGUMENT where the kernel cannot run
 * (the factors [n][d, d | 1] and the gradient weights [Npad] exceed 128 KB of LDS together).  ALABI_ENS_HMC_CHUNK=k caps the steps
 * of one launch at k, read at every alabi_ens_run; the chunk length changes no bit of the result.  The walker's logp is the
 * caller's and is never recomputed.  alabi_ens_draw and the sharded run refuse such a table.
 * kind 7 NUTSMove (multinomial No-U-Turn sampler, Betancourt 2017 as in Stan, on the same gradient and in the same whitened
 * momentum): p0 = step size > 0; p1 = max_depth + q / 512 with max_depth in 1 ... 10 and q as for kind 6.  The factor travels by
 * alabi_ens_set_move_scale ahead of the table; alabi_ens_set_moves is ALABI_BAD_ARGUMENT for a kind-7 move whose slot has no
 * factor, for a step size that is not positive and finite, for max_depth outside 1 ... 10 and for a table that mixes kind 7 with
 * another kind.  One transition of walker x with lp = the caller's logp, g = grad lnp(x), e = p0 f as kind 6: z0 ~ N(0, I), H0 =
 * -lp + |z0|^2 / 2, both ends of the tree (x, z0, g), rho = z0, proposal x, ln W = 0.  Doubling j = 0 ... max_depth - 1: direction
 * bit v_j set extends forward from the right end (s = e), otherwise backward from the left end (s = -e), by 2^j leaves; a leaf is
 * z += (s / 2) C^T g, q += s C z, (lp_q, g) = lnp and its gradient at q, z += (s / 2) C^T g.  Per leaf delta = H0 - (-lp_q +
 * |z|^2 / 2); divergent iff not (delta > -1000), NaN included: the subtree is dropped and the transition ends; ln w = delta where q
 * lies in the open box, -inf elsewhere (lnp itself has no box gate); the acceptance statistic a = min(1, exp(delta)) in the box, 0
 * elsewhere and for a divergent leaf.  With ln w > -inf: ln W' = logaddexp(ln W', ln w) and the leaf becomes the subtree's candidate
 * iff ln u_leaf < ln w - ln W'.  With the subtree's leaves numbered n = 0, 1, ... as made, the last leaf of every aligned block of
 * 2^k leaves (k >= 1) tests the block: it turns iff rho_block . z_first <= 0 or rho_block . z_last <= 0 (rho_block the sum of the
 * block's z), which drops the subtree and ends the transition.  A complete subtree: the proposal becomes its candidate iff ln W' >
 * -inf and ln u_tree,j < ln W' - ln W; then ln W = logaddexp(ln W, ln W'), rho += rho', the extended end moves, and the tree stops
 * iff rho . z_left <= 0 or rho . z_right <= 0.  The walker becomes the proposal with the lp and gradient of its leaf; n_accept
 * grows by 1 when a leaf was taken.  Stan's further U-turn checks across subtree joints are not built.  Draws: Philox counter
 * (step, global walker id, stream word S + 16 b) -- S = 3, 11 and 12 as kind 6; S = 13, b = 0: bit j of r0 is v_j; S = 14, b = the
 * leaf's ordinal within the transition (0 ... 2^max_depth - 2): u_leaf = u53(r0, r1); S = 15, b = j: u_tree,j = u53(r0, r1); stream
 * 2 is not read; streams 0-12 keep their meaning.  Such a table runs on ens_nuts_kernel (path 6 of alabi_ens_last_path) and on
 * nothing else: one workgroup per walker, every transition of a chunk in one launch, any W >= 1 and any n_ensembles;
 * alabi_ens_set_stream does not move it, and alabi_ens_run is ALABI_BAD_ARGUMENT where the factors [n][d, d | 1], the gradient
 * weights [Npad] and the 10 KB of U-turn checkpoints exceed 128 KB of LDS together.  ALABI_ENS_NUTS_CHUNK=k caps the transitions of
 * one launch at k, read at every alabi_ens_run; the chunk length and call splitting change no bit.  alabi_ens_draw, the sharded
 * run and alabi_ens_hmc_adapt refuse such a table. */
int alabi_ens_set_moves(alabi_ens* ens, int n, const int* kind, const double* cum, const double* p0, const double* p1);

/* The scale factor of slot k (0 <= k < 8) of the move table, for the Gaussian move that the NEXT alabi_ens_set_moves puts there
 * (see kind 5 above): C host [d, d] row-major, lower triangular with a positive diagonal and zeros above it; diagonal != 0 says
 * that it is diagonal (required for modes 1 and 2).  Where slot k of the current table holds a Gaussian move, that move runs
 * with the new factor from the next call on (ALABI_BAD_ARGUMENT if it moves one coordinate and the factor is not diagonal).  At
 * most 8 x 64 x 64 doubles are held on the device.  Synchronises the device. */
int alabi_ens_set_move_scale(alabi_ens* ens, int k, const double* C /* host */, int diagonal);
/* ens_mh_kernel's last launch: out[4] = workgroup size, steps per launch, LDS bytes, 1 if the training set is streamed in tiles
 * (Npad / 2 exceeds the workgroup). */
int alabi_ens_mh_plan(alabi_ens* ens, int* out /* host [4] */);
/* ens_hmc_kernel's last launch: out[4] = workgroup size, steps per launch, LDS bytes, 1 if a lane takes more than one training
 * point per pass (Npad exceeds the workgroup). */
int alabi_ens_hmc_plan(alabi_ens* ens, int* out /* host [4] */);
/* ens_nuts_kernel's last launch: out[4] = workgroup size, transitions per launch, LDS bytes, 1 if a lane takes more than one
 * training point per pass (Npad exceeds the workgroup). */
int alabi_ens_nuts_plan(alabi_ens* ens, int* out /* host [4] */);
/* Per-walker sums of the handle's NUTS transitions since the last reset (they belong to the handle and start at zero with its
 * first kind-7 table): counts_host [E*W, 3] = leaves made, depths reached (completed doublings), divergent transitions;
 * accept_host [E*W] = the sum of the acceptance statistic a over all leaves -- over the leaves it is what a warm-up averages.
 * reset != 0 zeroes them after the copy.  Synchronises the device.  Transitions of alabi_ens_step_with_randoms_nuts count too. */
int alabi_ens_nuts_stats(alabi_ens* ens, long long* counts_host /* host [E*W, 3] */, double* accept_host /* host [E*W] */, int reset);
/* HMC warm-up: nsteps steps of a table of exactly ONE kind-6 move on ens_hmc_adapt_kernel -- ens_hmc_kernel's launch shape,
 * arithmetic, draws and accept rule -- with a step size per walker adapted by dual averaging (Hoffman & Gelman 2014, algorithm 5;
 * tests/hmc_adapt_numpy.py states it).  da_state device [E*W, 5] doubles in/out: m (steps since the last restart), H-bar, ln e,
 * ln e-bar, mu.  A step of walker w runs with e = exp(ln e_w) f, f the step's jitter factor as alabi_ens_run draws it (1 without
 * jitter; the table's p0 is not read).  With dh the left-hand side of the accept test, a = min(1, exp(dh)), 0 where the end point
 * is outside the open box or dh is NaN; then m <- m + 1, H-bar <- (1 - 1 / (m + t0)) H-bar + (delta - a) / (m + t0),
 * ln e <- mu - (sqrt(m) / gamma) H-bar, ln e-bar <- m^-kappa ln e + (1 - m^-kappa) ln e-bar.  da_par host [4]: delta in (0, 1),
 * gamma > 0 (+inf allowed: ln e stays at mu), t0 >= 0, kappa in (0.5, 1]; Stan's defaults are 0.8, 0.05, 10, 0.75.  The call
 * consumes the global steps step0 ... step0 + nsteps - 1 exactly as alabi_ens_run does (a run after warm-up continues at
 * step0 + nsteps), with coords, logp, thin_by, chain, chain_logp and n_accept as there; accept_stat device [E*W] or null: the
 * sum of a over the call's steps is added.  The state is read when a launch starts and written when it ends, so chunking
 * (ALABI_ENS_HMC_CHUNK) and splitting the call change no bit.  Reports through alabi_ens_hmc_plan.  ALABI_BAD_ARGUMENT: the table
 * is not exactly one kind-6 move, a parameter is out of range, or the factor and the gradient weights exceed 128 KB of LDS. */
int alabi_ens_hmc_adapt(alabi_ens* ens, double* coords, double* logp, long long step0, long long nsteps, int thin_by,
                        double* da_state /* device [E*W, 5] in/out */, const double* da_par /* host [4]: delta, gamma, t0, kappa */,
                        double* chain, double* chain_logp, long long* n_accept, double* accept_stat /* or null */, void* stream);
/* NUTS warm-up: nsteps transitions of a table of exactly ONE kind-7 move on ens_nuts_adapt_kernel -- ens_nuts_kernel's launch
 * shape, arithmetic, draws, tree and stop rules (kind 7 above) -- with a step size per walker adapted by dual averaging on NUTS's
 * own statistic (tests/nuts_adapt_numpy.py states it).  da_state device [E*W, 5] doubles in/out as for alabi_ens_hmc_adapt: m,
 * H-bar, ln e, ln e-bar, mu.  A transition of walker w runs with e = exp(ln e_w) f, f the step's jitter factor as alabi_ens_run
 * draws it (the table's p0 is not read).  With leaves_t >= 1 the leaves the transition made, a_t = (the sum of the leaf statistic a
 * of kind 7 over exactly these leaves) / leaves_t: a = min(1, exp(delta)) in the open box, 0 outside it and 0 for a divergent
 * leaf, which counts as a leaf.  Then m <- m + 1, H-bar <- (1 - 1 / (m + t0)) H-bar + (delta - a_t) / (m + t0), ln e <- mu -
 * (sqrt(m) / gamma) H-bar, ln e-bar <- m^-kappa ln e + (1 - m^-kappa) ln e-bar.  da_par host [4] with alabi_ens_hmc_adapt's
 * ranges: delta in (0, 1), gamma > 0 (+inf allowed: ln e stays at mu), t0 >= 0, kappa in (0.5, 1].  The call consumes the global
 * steps step0 ... step0 + nsteps - 1 exactly as alabi_ens_run does, with coords, logp, thin_by, chain, chain_logp and n_accept
 * as there.  counts device [E*W, 3] int64 and accept_sum device [E*W] (either may be null) are the CALLER's and take what
 * alabi_ens_nuts_stats sums for a run -- leaves, depths, divergent transitions; the sum of a over all leaves -- in/out: warm-up
 * transitions are no part of the handle's sums.  accept_stat device [E*W] or null: the sum of a_t over the call's transitions is
 * added.  The state is read when a launch starts and written when it ends, so chunking (ens_nuts_chunk, ALABI_ENS_NUTS_CHUNK) and
 * splitting the call change no bit.  Reports through alabi_ens_nuts_plan.  ALABI_BAD_ARGUMENT: the table is not exactly one kind-7
 * move, a parameter is out of range, or the factor, the gradient weights and the checkpoints exceed 128 KB of LDS. */
int alabi_ens_nuts_adapt(alabi_ens* ens, double* coords, double* logp, long long step0, long long nsteps, int thin_by,
                         double* da_state /* device [E*W, 5] in/out */, const double* da_par /* host [4]: delta, gamma, t0, kappa */,
                         double* chain, double* chain_logp, long long* n_accept, long long* counts /* device [E*W, 3] in/out or null */,
                         double* accept_sum /* device [E*W] in/out or null */, double* accept_stat /* or null */, void* stream);
/* Initial step-size search (Stan's find_reasonable heuristic) for move k_move of a table that is all kind 6 or all kind 7 (both
 * use the same whitened leapfrog), on ens_step_search_kernel: one workgroup per walker, which does not move -- coords and logp are
 * read only.  Per walker from ln e = ln_e[w], with lp = the caller's logp and g = grad lnp(x), iteration i = 0, 1, ...: z ~ N(0, I)
 * fresh; H0 = -lp + |z|^2 / 2; one leapfrog step as a NUTS leaf with e = exp(ln e): z += (e / 2) C^T g, q = x + e C z, (lp_q, g_q)
 * at q, z += (e / 2) C^T g_q; dH = H0 - (-lp_q + |z|^2 / 2), with NaN and a q outside the open box counting as -inf.  Iteration 0
 * fixes dir = +1 if dH > ln 0.8, else -1.  The loop ends at the first iteration where dir = +1 and not dH > ln 0.8, or dir = -1
 * and not dH < ln 0.8; otherwise ln e += dir ln 2 and the next iteration follows, 40 such steps at the most.  iters device [E*W]
 * int32 or null: the number of ln 2 steps taken = the index of the iteration that ended the loop; 40 says that the cap ended it,
 * the walker keeps its last ln e.  Draws: Philox counter (step, global walker id, stream word 11 + 16 (64 (i + 1) + k)) for the
 * momentum normal of iteration i, coordinate k -- stream 11 at b >= 64, where kinds 6 and 7 read b = k < 64 only, so no draw of a
 * move at the same step is read twice.  The search consumes no global step.  ALABI_BAD_ARGUMENT: a table of other kinds, k_move
 * outside the table, no factor, or the factor and the gradient weights exceed 128 KB of LDS. */
int alabi_ens_find_step_size(alabi_ens* ens, const double* coords, const double* logp, long long step, int k_move,
                             double* ln_e /* device [E*W] in/out */, int* iters /* device [E*W] int32 or null */, void* stream);
/* The ensemble's log-probability and its gradient at M arbitrary points, by the evaluation ens_hmc_kernel runs: coords [M, d],
 * logp [M], grad [M, d] on the device.  lnp = GP mean through the folded affine scalers and the y map, plus the normal priors;
 * grad = a T^T dmu (no map), ln10 lnp a T^T dmu (either map), minus (x_k - m_k) / s_k^2 per normal-prior coordinate.  Outside the
 * open box logp is -inf and the gradient zero.  Works with any move table; ALABI_BAD_ARGUMENT where Npad doubles exceed 128 KB. */
int alabi_ens_log_prob_grad(alabi_ens* ens, const double* coords, int M, double* logp, double* grad, void* stream);
/* The maximum of the same log-probability inside the box, by a projected BFGS ascent from S starts at once (ens_map_kernel: one
 * workgroup per start, every iteration in one launch; tests/map_numpy.py states the rule).  starts [S, d], x_out [S, d], lp_out [S],
 * iters_out [S, 2] (iterations, evaluations; int), status_out [S] (int), gnorm_out [S] on the device.  status: 0 = the projected
 * gradient's largest component is at most gtol, 1 = maxiter iterations taken, 2 = no ascent at the smallest step (the best point is
 * kept), 3 = the start lies outside the open box or the log-probability is not finite there (x, lp and gnorm are NaN).  The result
 * is never worse than the start.  The search runs on the box shrunk by 1e-9 of its width, so a coordinate held on a bound sits at
 * lo + 1e-9 (hi - lo) or hi - 1e-9 (hi - lo).  trace (or null with ntrace = 0): device [S, ntrace, 4] doubles, per accepted
 * iteration the new lp, the step length t, the held set (the bits of a 64-bit integer, bit k = coordinate k) and 1 where the BFGS
 * update was applied; rows beyond the last iteration are left as they were.  The bits of a start's result do not depend on S or
 * on its place in the batch.  Works with any move table; ALABI_BAD_ARGUMENT where B [d][d | 1] and the gradient weights [Npad]
 * exceed 128 KB of LDS together. */
int alabi_ens_maximize(alabi_ens* ens, const double* starts, int S, int maxiter, double gtol, double* x_out, double* lp_out,
                       int* iters_out /* [S, 2] */, int* status_out, double* gnorm_out, double* trace /* or null */, int ntrace,
                       void* stream);
/* The Hessian of the same log-probability with respect to the coordinates at M arbitrary points: coords [M, d], hess_out [M, d, d]
 * on the device, symmetric to the bit.  No map: a T^T (d2 mu) T; either y map L = -+10^Mu: ln10 L d2 Mu + ln10^2 L dMu dMu^T; minus
 * 1 / s_k^2 on the diagonal per normal-prior coordinate.  Outside the open box every entry is NaN.  ALABI_BAD_ARGUMENT where
 * 2 Npad doubles exceed 128 KB. */
int alabi_ens_log_prob_hessian(alabi_ens* ens, const double* coords, int M, double* hess_out, void* stream);
/* How alabi_ens_maximize launches on this handle: out[4] = workgroup size, LDS bytes, 1 if a lane takes more than one training
 * point per pass (Npad exceeds the workgroup), dimension bucket. */
int alabi_ens_map_plan(alabi_ens* ens, int* out /* host [4] */);

/* Enable / disable the persistent dataflow kernel for alabi_ens_run on this handle (default: enabled when the
 * ensemble fits one workgroup per CU).  Returns ALABI_BAD_ARGUMENT when enabling is impossible.
 * The same switch turns ens_mh_kernel (path 4, a table of Gaussian moves alone) on and off; it is a setting of the handle and
 * holds for whichever move table a later alabi_ens_run finds, not only for the one set when it is called.  ens_mh_kernel needs
 * no version history, so enabling succeeds on a handle without one while its table is all Gaussian; a red-blue table set later
 * on such a handle runs with one launch per half step, as before. */
int alabi_ens_set_stream(alabi_ens* ens, int enabled);
/* Which path the last alabi_ens_run took: 1 = persistent dataflow kernel with the training set in one workgroup's
 * registers (ens_stream_kernel: N <= 2048, small d), 3 = persistent group kernel (ens_group_kernel: training set
 * partitioned over groups of workgroups, kernel sums on the matrix cores; d <= 30), 4 = ens_mh_kernel (a table of Gaussian moves
 * alone: one workgroup per walker; alabi_ens_set_stream(ens, 0) sends such a table to path 0), 5 = ens_hmc_kernel (a table of HMC
 * moves: one workgroup per walker; it has no other path), 6 = ens_nuts_kernel (a table of NUTS moves: likewise), 0 = one launch per
 * half step. */
int alabi_ens_last_path(alabi_ens* ens, int* path /* host */);
/* Which persistent kernel the last alabi_ens_run of path 1 launched: 0 = ens_stream_kernel (one workgroup per list position),
 * 1 = ens_pair_kernel (two per list position, which evaluate both outcomes of a pending update; chosen where 2 ceil(W/2) E
 * workgroups fit one per CU and the moves are stretch moves; ALABI_ENS_PAIR=0 disables it; a time-out of it is retried inside
 * the call on ens_stream_kernel and turns it off for the handle).  Both produce the same bits. */
int alabi_ens_stream_variant(alabi_ens* ens, int* variant /* host */);
/* Debug counters of ens_pair_kernel, by class (number of input rows of a proposal that the immediately preceding half step
 * produced: 0, 1, 2): out[3 c] items, out[3 c + 1] rows stored by the workgroup that assumes "rejected", out[3 c + 2] by the one
 * that assumes "accepted".  The first call switches counting on (from the next run on); reset != 0 zeroes the counters after
 * reading.  Synchronises the device. */
int alabi_ens_pair_stats(alabi_ens* ens, long long* out /* host [9] */, int reset);
/* Fetch-ahead counters of ens_pair_kernel (its hand-off wave loads the next item's input words in the idle window of the current
 * item and skips the poll when none of them is the sentinel): out[0] items of the workgroups that assume "rejected", out[1] those
 * of them whose inputs the fetch-ahead had complete, out[2], out[3] the same for the workgroups that assume "accepted" (both
 * step through every item; a skipped item reads row 0 and counts as complete); out[4], out[5] are kept for the class-1 items
 * whose fresh input row the "accepted" workgroup takes from slot R and from slot A of a two-slot proposal array, and are 0
 * while the proposal array has one slot.  enable != 0 switches counting on if it is not
 * (from the next run on); the counters are zeroed after reading.  Synchronises the device. */
int alabi_ens_pair_stats2(alabi_ens* ens, long long* out /* host [6] */, int enable);
/* Look counters of ens_pair_kernel's two polls, per role (r = 0: the workgroups that assume "rejected", r = 1: "accepted"):
 * out[10 r + 0] class-1 items that polled the verdict, [10 r + 1] the looks (tests of a loaded verdict word) of those polls,
 * [10 r + 2], [10 r + 3], [10 r + 4] the polls decided at look 1, at look 2, at look 3 or later (a poll that timed out counts by
 * its last look); [10 r + 5 .. 10 r + 9] the same for the input poll at the top of an item, over the items whose inputs the
 * fetch-ahead did not have complete (a look is a reload).  enable != 0 switches counting on if it is not (from the next run
 * on); the counters are zeroed after reading.  Synchronises the device. */
int alabi_ens_pair_stats3(alabi_ens* ens, long long* out /* host [20] */, int enable);
/* Placement of ens_pair_kernel's items by XCD class (ens_place_kernel; on where W is even, W / 2 a multiple of 8 and at most 128,
 * and ALABI_ENS_PLACE is not 0; decided at the first run): out[0] 1 if placement is on for this handle, out[1] items that had a
 * preferred class, out[2] items placed on it -- over the records of the calls made so far (records placed ahead for a call that
 * has not come yet are not counted).  reset != 0 zeroes the counters after reading.  Synchronises the device. */
int alabi_ens_place_stats(alabi_ens* ens, long long* out /* host [3] */, int reset);
/* Draws steps step0 .. step0 + nsteps - 1 (nsteps <= the chunk capacity) as ONE chunk into the handle's buffers, runs the
 * placement pre-pass on them and copies out, by list position: place [nsteps*E*W] the pair every item was handed to and, where
 * not NULL, the packed records as drawn and as permuted ([nsteps*E*W][4] words each; device pointers).  ALABI_NOT_COMPUTED while
 * placement is not on.  Leaves nothing drawn for alabi_ens_half_step. */
int alabi_ens_export_placement(alabi_ens* ens, long long step0, int nsteps, double a, int* place, unsigned long long* packed,
                               unsigned long long* packed_x, void* stream);
/* Blocking of the last group-kernel launch of alabi_ens_run (zeros before the first one), so a parity test can pin WHICH
 * instantiation of ens_group_kernel it compared with the oracle: out[0] Q (16-proposal tiles per group), [1] G (members per
 * group), [2] NG (groups per ensemble), [3] RT (point tiles per wave held in registers), [4] tpm (point tiles per member),
 * [5] ltw (point tiles per wave staged in LDS), [6] KS (MFMA k-steps = ceil((d + 2) / 4)), [7] LDS bytes per workgroup. */
int alabi_ens_group_plan(alabi_ens* ens, int* out /* host [8] */);

/* log-probability of every walker (surrogate mean + box prior): coords [E*W,d] -> logp [E*W]. */
int alabi_ens_lnprob(alabi_ens* ens, const double* coords, double* logp, void* stream);

/* The surrogate part alone, y_scaler^-1(GP mean), at M arbitrary points [M,d] in the sampler's coordinates -- no box
 * gate, no prior (alabi/core.py:1446-1508 surrogate_log_likelihood as lnprob's like_fn, :2073-2100). */
int alabi_ens_surrogate(alabi_ens* ens, const double* points, int M, double* like, void* stream);

/* Run nsteps full stretch-move steps on one GPU.  coords [E*W,d] and logp [E*W] are updated in
 * place; chain [nsteps/thin_by, E*W, d] and chain_logp [nsteps/thin_by, E*W] receive every
 * thin_by-th state (either may be NULL); n_accept [E*W] int64 is ADDED to.  step0 is the
 * global index of the first step (counter-based RNG: draws depend on (seed, step, global
 * walker id) only).  Enqueues on `stream`; does not synchronise with the kernels. */
int alabi_ens_run(alabi_ens* ens, double* coords, double* logp, long long step0,
                  long long nsteps, int thin_by, double a, double* chain, double* chain_logp,
                  long long* n_accept, void* stream);
/* The walkers the last alabi_ens_run left, from the host block that call read back with its time-out flag: coords_out
 * [E*W,d] and logp_out [E*W] are HOST arrays; no device work, no synchronisation.  ALABI_NOT_COMPUTED unless the last
 * alabi_ens_run on this handle ended without a time-out on path 1 (ens_stream_kernel / ens_pair_kernel). */
int alabi_ens_last_state(alabi_ens* ens, double* coords_out /* host */, double* logp_out /* host */);
/* After ALABI_TIMEOUT: copy back what the call saved at its start -- coords [E*W,d], logp [E*W] and, if the call was given
 * counters, n_accept [E*W] (device pointers; n_accept may be NULL) -- so that the caller can repeat the call on another path
 * (alabi_ens_set_stream(ens, 0)).  Enqueues on `stream`.  ALABI_NOT_COMPUTED if no persistent call has run on this handle. */
int alabi_ens_restore(alabi_ens* ens, double* coords, double* logp, long long* n_accept, void* stream);
/* Host-side counters of what alabi_ens_run's path 1 did around its persistent kernels since the handle was created:
 * out[0] calls whose first chunk found its proposal records drawn ahead by the previous call, out[1] calls that had to
 * draw them first, out[2] fill launches on the published-proposal buffer, out[3] fill launches on the version history
 * (both are needed on first use and after a time-out only). */
int alabi_ens_boundary_stats(alabi_ens* ens, long long* out /* host [4] */);

/* sampler.get_autocorr_time(tol=0) -- alabi/mcmc_utils.py:45, alabi/core.py:2387 (emcee.autocorr.integrated_time): the FFT part.
 * chain [n_t, n_w, n_d] (device, as alabi_ens_run stores it) -> acf_mean [n_d, n_t] (device): for every dimension the mean over
 * the walkers of acf = IFFT(|FFT(x - mean(x), 2 n)|^2)[:n_t] / acf[0], n = the next power of two >= n_t.  Hand-written four-step
 * transforms in LDS (alabi_amd/csrc/chain_acf.hip): no run-time kernel compilation per transform length.  n_t <= 2^21.  The Sokal
 * window and tau = 2 cumsum(acf) - 1 follow on the host (alabi_amd/mcmc_utils.py).  Synchronises the stream. */
int alabi_chain_autocorr(const double* chain, long long n_t, int n_w, int n_d, double* acf_mean, void* stream);
/* The device half of the chain diagnostics of Vehtari et al. (2021) (alabi_amd/diagnostics.py: split R-hat, bulk / tail ESS, MCSE):
 * per-chain moments and the chain-averaged, UN-normalised autocovariance of the (split) chains of a run.
 * Element (t, w, k) lies at chain[t * t_stride + w * n_d + k] (t_stride >= n_w * n_d: a discard / thin view is read in place).
 * n = n_t / n_split; split chain c = half * n_w + w holds the steps [0, n) (half 0) or [n_t - n, n_t) (half 1) of walker w.
 * transform is applied on load: 0 y = x, 1 y = 1[x <= par[k]], 2 y = |x - par[k]| (par [n_d] device; may be NULL for 0).
 *   chain_mean, chain_var [n_split * n_w, n_d]   mean and variance (ddof 1) of every split chain: direct two-pass sums
 *   acov_mean [n_d, n]                           mean over the chains c of gamma_c(lag) = (1/n) sum_{t < n - lag} (y[t] - mean)(y[t + lag] - mean),
 *                                                by the transforms of alabi_chain_autocorr; NULL: moments only, no transform runs
 * ALABI_BAD_ARGUMENT: n_split not 1 or 2, n < 2, n > 2^21, t_stride < n_w * n_d, transform not 0..2, transform != 0 without par.
 * Synchronises the stream. */
int alabi_chain_split_stats(const double* chain, long long n_t, long long t_stride, int n_w, int n_d, int n_split, int transform,
                            const double* par, double* chain_mean, double* chain_var, double* acov_mean, void* stream);

/* Multi-GPU building blocks for ONE sharded ensemble (n_ensembles == 1; alabi_amd/dist.py
 * drives them around an RCCL all-gather): draw the proposal records of steps
 * [step0, step0+nsteps) into the handle, then apply one HALF step (split 0 or 1 of local
 * step `t`) to the walkers whose position in that half's list lies in [part_begin, part_end). */
int alabi_ens_draw(alabi_ens* ens, long long step0, int nsteps, double a, void* stream);
int alabi_ens_half_step(alabi_ens* ens, double* coords, double* logp, int t, int split,
                        int part_begin, int part_end, long long* n_accept, void* stream);
/* Generic log-probability (n_ensembles == 1): the reference's lnprob = like_fn(theta) + prior_fn(theta) accepts ANY
 * Python callables (alabi/core.py:2073-2100, :2253-2280; docstring example :2236-2239).  A half step of drawn local step
 * `t` is split around the host call: alabi_ens_propose writes the proposals of that half in LIST order to q [nS,d]
 * (nS = ceil(W/2) for split 0, floor(W/2) for split 1) and, if `like` is not NULL, the surrogate part
 * y_scaler^-1(GP mean) at each proposal (-inf outside the box when gate_box != 0); the caller forms
 * lp_new [nS] = like (or its own like_fn) + prior_fn(q); alabi_ens_accept applies emcee's accept test
 * (d-1) ln z + lp_new - logp > ln u' with the step's draws and updates coords / logp / n_accept in place.
 * A NaN lp_new rejects. */
int alabi_ens_propose(alabi_ens* ens, const double* coords, int t, int split, int gate_box,
                      double* q, double* like, void* stream);
int alabi_ens_accept(alabi_ens* ens, double* coords, double* logp, int t, int split,
                     const double* q, const double* lp_new, long long* n_accept, void* stream);
/* ONE ensemble sharded over the GPUs of a node with the whole step loop in the library (n_ensembles == 1): each rank
 * applies every half step to its slice of the active list and the updated (coords, logp) rows are exchanged with one
 * all-gather per half step, enqueued on `stream` (RCCL ncclAllGather over xGMI; librccl.so is loaded with dlopen on first
 * use).  Replaces the reference's process pool under emcee (alabi/core.py:2300, :2322).  Every rank passes the same
 * initial coords / logp / step0 and ends with the same coords / logp / chain; n_accept [W] is ADDED to (summed over ranks).
 * alabi_dist_unique_id: rank 0 obtains 128 bytes and distributes them (e.g. torch.distributed broadcast), then every rank
 * calls alabi_dist_comm_create with them (nranks == 1 needs no id).  The *_callback form carries a host function instead
 * of RCCL: the test rig for several ranks on one GPU (it must complete the exchange before returning). */
typedef struct alabi_comm alabi_comm;
typedef int (*alabi_allgather_fn)(const double* send_dev, double* recv_dev, long long count_per_rank, void* user, void* stream);
int alabi_dist_unique_id(void* id_out /* host, 128 bytes */);
int alabi_dist_comm_create(const void* id /* host, 128 bytes */, int rank, int nranks, alabi_comm** out);
int alabi_dist_comm_create_callback(alabi_allgather_fn fn, void* user, int rank, int nranks, alabi_comm** out);
int alabi_dist_comm_destroy(alabi_comm* comm);
/* Counters of alabi_ens_run_sharded on this communicator (host int64[4]): [0] full chunks replayed from the captured hipGraph,
 * [1] chunks enqueued launch by launch, [2] graph captures, [3] 1 once a run failed on this rank with peers possibly inside the
 * collective (the communicator is then dead: every later run returns ALABI_HIP_ERROR; end the process). */
int alabi_dist_comm_stats(alabi_comm* comm, long long* out /* host [4] */);
int alabi_ens_run_sharded(alabi_ens* ens, alabi_comm* comm, double* coords, double* logp, long long step0,
                          long long nsteps, int thin_by, double a, double* chain, double* chain_logp,
                          long long* n_accept, void* stream);
/* copy of the walker lists of drawn local step t: order_out[W] int32 (device), n0 (host). */
int alabi_ens_step_lists(alabi_ens* ens, int t, int* order_out, int* n0, void* stream);

/* Test entry (n_ensembles == 1): one full step from caller-supplied draws keyed by WALKER id
 * (bit-exact index-arithmetic fixtures).  order[W] int32 lists set 0 then set 1; partner[W]
 * int32 indexes the complementary list.  Out-of-range indices make that proposal a no-op. */
int alabi_ens_step_with_randoms(alabi_ens* ens, double* coords, double* logp,
                                const int* order, int n0, const double* u_z,
                                const int* partner, const double* u_acc, double a,
                                long long* n_accept, void* stream);
/* Test entry: the device's counter-based draws for one step, copied out in LIST order
 * (position p of ensemble e at [e*W + p]): order = global walker id, partner = index drawn
 * into the complementary list, u_z / u_acc raw uniforms, cw (nullable) = partner's global
 * walker id, zz (nullable) = stretch factor.  n0 is a host int. */
int alabi_ens_export_draws(alabi_ens* ens, long long step, double a, int* order, int* n0,
                           double* u_z, int* partner, double* u_acc, int* cw, double* zz,
                           void* stream);

/* Test entries of the moves (alabi_ens_set_moves; reference call site alabi/core.py:2144, :2319).
 * alabi_ens_export_move_draws: for the step last drawn by alabi_ens_export_draws on a handle with a move set -- move [E] the
 * index of each ensemble's move, and in LIST order j2 [E*W] the second partner's index into the complementary list (-1 at a
 * stretch step) and gamma [E*W] the DE step size (at a stretch step: the stretch factor).  j1 is export_draws' `partner`.
 * alabi_ens_step_with_randoms_de (n_ensembles == 1): one full DE step from caller-supplied draws keyed by WALKER id, the
 * sibling of alabi_ens_step_with_randoms: j1[W] / j2[W] int32 index the complementary list (j1 != j2), gamma[W] is the
 * step size, u_acc[W] the accept uniform.  Out-of-range indices make that proposal a no-op.  All arrays on the device. */
int alabi_ens_export_move_draws(alabi_ens* ens, int* move, int* j2, double* gamma, void* stream);
int alabi_ens_step_with_randoms_de(alabi_ens* ens, double* coords, double* logp, const int* order, int n0,
                                   const int* j1, const int* j2, const double* gamma, const double* u_acc,
                                   long long* n_accept, void* stream);

/* Test entries of the snooker move (kind 2 of alabi_ens_set_moves), siblings of the two above.
 * alabi_ens_export_snooker_draws: for the step last drawn by alabi_ens_export_draws on a handle whose move set holds a snooker
 * move -- in LIST order j3 [E*W], the third partner's index into the complementary list (-1 at a stretch or DE step); j1 is
 * export_draws' `partner`, j2 comes from alabi_ens_export_move_draws.
 * alabi_ens_export_partner_ids: for the same step, in LIST order, the global walker ids of the second (cw2 [E*W]) and the third
 * partner (cw3 [E*W]); -1 where the record has none; either pointer may be NULL.
 * alabi_ens_step_with_randoms_snooker (n_ensembles == 1): one full snooker step from caller-supplied draws keyed by WALKER id:
 * j1[W] / j2[W] / j3[W] int32 index the complementary list (pairwise distinct), gamma is gammas, u_acc[W] the accept uniform.
 * Out-of-range or non-distinct indices make that proposal a no-op.  All arrays on the device. */
int alabi_ens_export_snooker_draws(alabi_ens* ens, int* j3, void* stream);
int alabi_ens_export_partner_ids(alabi_ens* ens, int* cw2, int* cw3, void* stream);
int alabi_ens_step_with_randoms_snooker(alabi_ens* ens, double* coords, double* logp, const int* order, int n0,
                                        const int* j1, const int* j2, const int* j3, double gamma, const double* u_acc,
                                        long long* n_accept, void* stream);

/* Test entries of the walk and KDE moves (kinds 3 and 4 of alabi_ens_set_moves; emcee's moves= as documented at
 * alabi/core.py:2144 and handed over at alabi/core.py:2319), siblings of alabi_ens_step_with_randoms_de / _snooker
 * (n_ensembles == 1, all arrays on the device, draws keyed by WALKER id).
 * alabi_ens_step_with_randoms_walk: one full walk step; subset[W, s0] int32 indexes the complementary list (s0 distinct rows per
 * walker), z[W, s0] holds the rows' normals, the sums run over m = 0 .. s0-1 in that order.  Out-of-range or repeated subset
 * indices make that proposal a no-op.  2 <= s0 <= min(n0, W - n0), both halves <= 2048, else ALABI_BAD_ARGUMENT.
 * alabi_ens_step_with_randoms_kde: one full KDE step with the bandwidth factor `factor` for both splits; r[W] int32 is the row of
 * the complementary list, z[W, d] the normals, lnfac_out[W] (nullable) receives the proposals' log factor.  An out-of-range r
 * makes that proposal a no-op.  Both halves need between d + 1 and (W + 1) / 2 rows, else ALABI_BAD_ARGUMENT.
 * alabi_ens_kde_singular: the number of (half step, ensemble) pairs of this handle whose KDE had no Cholesky factor (host value;
 * synchronises the device). */
int alabi_ens_step_with_randoms_walk(alabi_ens* ens, double* coords, double* logp, const int* order, int n0, int s0,
                                     const int* subset, const double* z, const double* u_acc, long long* n_accept, void* stream);
int alabi_ens_step_with_randoms_kde(alabi_ens* ens, double* coords, double* logp, const int* order, int n0, double factor,
                                    const int* r, const double* z, const double* u_acc, double* lnfac_out, long long* n_accept,
                                    void* stream);
int alabi_ens_kde_singular(alabi_ens* ens, long long* count /* host */);

/* Test entries of the Gaussian move (kind 5 of alabi_ens_set_moves), siblings of alabi_ens_step_with_randoms_de (n_ensembles == 1,
 * all arrays on the device, draws keyed by WALKER id).
 * alabi_ens_step_with_randoms_gauss: one full step of move k_move of the table (its scale factor set) with the step's scale
 * factor f, coord[W] int32 the coordinate that moves (-1: all of them; out of range: that proposal is a no-op), z[W, d] the
 * normals and u_acc[W] the accept uniform.
 * alabi_ens_export_gauss_draws: for the step last drawn by alabi_ens_export_draws -- f [E] the scale factor of each ensemble's
 * step, coord [E*W] and z [E*W, d] by walker id (f = 1 and coord = -1 where the step's move is not a Gaussian move). */
int alabi_ens_step_with_randoms_gauss(alabi_ens* ens, double* coords, double* logp, const int* order, int n0, int k_move, double f,
                                      const int* coord, const double* z, const double* u_acc, long long* n_accept, void* stream);
int alabi_ens_export_gauss_draws(alabi_ens* ens, double* f, int* coord, double* z, void* stream);

/* Test entries of the HMC move (kind 6 of alabi_ens_set_moves; the table must be all HMC; all arrays on the device, keyed by
 * WALKER id).
 * alabi_ens_step_with_randoms_hmc (n_ensembles == 1): one step of move k_move of the table from injected draws -- e the step size
 * actually used (jitter included), z [W, d] the momentum normals z0, u_acc [W] the accept uniform.
 * alabi_ens_export_hmc_draws: the production draws of global step `step` -- move [E] int32 and e [E] per ensemble, z [E*W, d] and
 * u_acc [E*W] (nullable) per walker. */
int alabi_ens_step_with_randoms_hmc(alabi_ens* ens, double* coords, double* logp, int k_move, double e, const double* z,
                                    const double* u_acc, long long* n_accept, void* stream);
int alabi_ens_export_hmc_draws(alabi_ens* ens, long long step, int* move, double* e, double* z, double* u_acc, void* stream);
/* Test entries of the NUTS move (kind 7 of alabi_ens_set_moves; the table must be all NUTS; all arrays on the device, keyed by
 * walker id).
 * alabi_ens_step_with_randoms_nuts (n_ensembles == 1): one transition of move k_move of the table, max_depth its own, from injected
 * draws -- e the step size with the jitter applied, z0 [W, d], dir [W] uint32 direction words (bit j: doubling j goes forward),
 * u_leaf [W, 2^max_depth - 1] by the leaf's ordinal within the transition, u_tree [W, max_depth].  trace [W, 4] int32 or null:
 * depth reached (completed doublings), leaves made, stop reason (0 max_depth, 1 U-turn of the tree, 2 U-turn inside a subtree,
 * 3 divergent) and 1 if a leaf was taken.
 * alabi_ens_export_nuts_draws: the production draws of global step `step` -- move [E] int32 and e [E] per ensemble, z0 [E*W, d],
 * dir [E*W] uint32, u_leaf [E*W, 2^max_depth - 1] and u_tree [E*W, max_depth] for the max_depth (1 ... 10) the caller names. */
int alabi_ens_step_with_randoms_nuts(alabi_ens* ens, double* coords, double* logp, int k_move, double e, const double* z0,
                                     const unsigned* dir, const double* u_leaf, const double* u_tree, int* trace /* or null */,
                                     long long* n_accept, void* stream);
int alabi_ens_export_nuts_draws(alabi_ens* ens, long long step, int max_depth, int* move, double* e, double* z0, unsigned* dir,
                                double* u_leaf, double* u_tree, void* stream);

/* Nested sampling (dynesty's NestedSampler / DynamicNestedSampler with sample="rwalk" as driven by
 * SurrogateModel.run_dynesty, alabi/core.py:2417-2787, likelihood = surrogate_log_likelihood core.py:1446-1508, prior =
 * ut.prior_transform_uniform core.py:2578-2585).  The host keeps the nested-sampling loop (alabi_amd/nested.py); the
 * library runs the constrained random walks.  Points live in the unit cube; bounds is a host array [d,2] in the GP's
 * scaled coordinates, x = lo + u (hi - lo) (hi < lo is allowed: a decreasing affine theta scaler).
 * logL(u) = map(scale * GP mean(x) + shift) as alabi_ens_set_logp_affine / _map (default 1, 0, identity).
 * Draws are keyed by (seed, call, global walk id = walk_id0 + b, step) (Philox4x32-10, layout in nested.hip), so a call
 * split into several launches by walk_id0 gives the same bits.  call, walk_id0 + K < 2^32. */
int alabi_ns_create(alabi_gp* gp, int d, const double* bounds /* host [d,2], scaled */, unsigned long long seed,
                    alabi_ns** out);
int alabi_ns_destroy(alabi_ns* ns);
int alabi_ns_set_logp(alabi_ns* ns, double scale, double shift, int map_kind /* 0 identity, 1 nlog, 2 log */);
/* Independent normal priors on selected cube coordinates: the reference's prior_transform_normal
 * (alabi/utility.py:381-482).  mean[d], std[d] on the HOST in the GP's scaled coordinates; non-finite mean = that
 * coordinate keeps the uniform map over its box; std may be negative, std == 0 (or non-finite) is an error.
 * x_k = mean_k + std_k * ndtri(u_k), not truncated to the box; u_k = 0 is evaluated at 2^-54.  Takes effect from the next call on. */
int alabi_ns_set_normal_prior(alabi_ns* ns, const double* mean, const double* std);
/* x_out [K,d]: the scaled coordinates (before the length scales and the centring) of cube points u [K,d], by the
 * same device function the walks use. */
int alabi_ns_transform(alabi_ns* ns, const double* u, int K, double* x_out, void* stream);
/* n uniform points u_out [n,d] (dynesty's initial live points) and, if logl_out is not NULL, their logL [n]. */
int alabi_ns_prior_draw(alabi_ns* ns, long long call, int walk_id0, int n, double* u_out, double* logl_out, void* stream);
/* K independent walks of `walks` Metropolis steps from u0 [K,d] (logL logl0 [K]; NULL: evaluated first):
 * u' = u + scale * chol z, z ~ N(0, I_d), chol [d,d] row-major lower triangle; accept iff 0 < u' < 1 and logL(u') > logl_star.
 * Writes u_out [K,d] (may alias u0), logl_out [K] and, if n_accept is not NULL, int32 [2K]: accepted steps per walk, then
 * likelihood evaluations (in-cube proposals) per walk.  A walk that accepts nothing returns its start bit for bit. */
int alabi_ns_walk(alabi_ns* ns, long long call, int walk_id0, const double* u0, const double* logl0, int K, double logl_star,
                  const double* chol, double scale, int walks, double* u_out, double* logl_out, int* n_accept, void* stream);
/* The same walk split around a host likelihood (like_fn callables, custom prior_transform, core.py:2533-2601):
 * alabi_ns_propose writes step `step` of every walk, u_prop [K,d], with the draws and arithmetic of alabi_ns_walk;
 * the caller evaluates logl_prop [K] (-inf outside the cube); alabi_ns_accept applies the accept test and updates
 * u_cur / logl_cur in place, ADDING to n_accept [2K] as alabi_ns_walk counts. */
int alabi_ns_propose(alabi_ns* ns, long long call, int walk_id0, const double* u_cur, int K, int step, const double* chol,
                     double scale, double* u_prop, void* stream);
int alabi_ns_accept(alabi_ns* ns, int K, const double* u_prop, const double* logl_prop, double logl_star, double* u_cur,
                    double* logl_cur, int* n_accept, void* stream);
/* Random-direction slice sampling (dynesty's sample="rslice"): K independent walks of `slices` slice updates from u0 [K,d] with
 * logL logl0 [K] (required).  Slice s: axis a = scale * chol z / |z|; interval [t_l, t_r] = [-r, 1 - r], r ~ U(0,1), along
 * u + t a; stepping out by 1 on either side while the end lies strictly inside the cube with logL > logl_star (an expansion
 * each; a point outside the cube ends the stepping without an evaluation); then t ~ U(t_l, t_r) until the point lies inside the
 * cube with logL > logl_star, every failure moving the end on its side to t (a contraction).  After 64 contractions the slice
 * ends where it started (a capped slice).  Writes u_out [K,d] (may alias u0), logl_out [K] and, if counts is not NULL, int32
 * [4K]: likelihood evaluations (in-cube points), expansions, contractions, capped slices per walk.  slices < 2^31 - 1;
 * slices = 0 returns the start bit for bit.  Draw keys: nested.hip. */
int alabi_ns_slice(alabi_ns* ns, long long call, int walk_id0, const double* u0, const double* logl0, int K, double logl_star,
                   const double* chol, double scale, int slices, double* u_out, double* logl_out, int* counts, void* stream);
/* The same move split around a host likelihood, with the draws and arithmetic of alabi_ns_slice.  `state` is a device buffer of
 * alabi_ns_slice_state_bytes(K) bytes (8-byte aligned) that alabi_ns_slice_begin fills from u0 / logl0.  alabi_ns_slice_step
 * consumes logl_query [K] (read for the walks whose previous query is pending), advances every walk to its next query strictly
 * inside the cube, writes it to u_query [K,d] and sets active [K] to 1, or to 0 for a walk that has ended; the caller
 * evaluates the active walks' queries and calls again until no walk is active.  alabi_ns_slice_end writes the outputs of
 * alabi_ns_slice. */
int alabi_ns_slice_state_bytes(alabi_ns* ns, int K, long long* bytes /* host */);
int alabi_ns_slice_begin(alabi_ns* ns, const double* u0, const double* logl0, int K, void* state, void* stream);
int alabi_ns_slice_step(alabi_ns* ns, long long call, int walk_id0, int K, double logl_star, const double* chol, double scale,
                        int slices, void* state, const double* logl_query, double* u_query, int* active, void* stream);
int alabi_ns_slice_end(alabi_ns* ns, int K, const void* state, double* u_out, double* logl_out, int* counts, void* stream);
/* Uniform draws inside bounding ellipsoids (MultiNest's move, the replacement step of SurrogateModel.run_pymultinest,
 * alabi/core.py:2790-3238; dynesty's sample="unif").  The table, device arrays: E ellipsoids {c_e + A_e z : |z| <= 1}, centres [E,d],
 * axes [E,d,d] (A, row-major, lower triangle read), inv_axes [E,d,d] (A^-1 likewise), cum [E] cumulative volume fractions with
 * cum[E-1] = 1.  Candidate i of the launch has the global id cand_id0 + i; its draws are keyed by (seed, call, id) alone (layout in
 * nested_unif.hip), so a call split into several launches by cand_id0 gives the same bits.  A candidate is drawn uniformly in the
 * ellipsoid chosen by volume and gets cand_status 0 (outside the cube), 1 (thinned: inside q ellipsoids it survives with probability
 * 1 / q, which makes the draw uniform over the union) or 2 (evaluated: cand_logl = logL); cand_logl = -inf below 2; cand_u [M,d]
 * holds every candidate's point.  evaluate = 0 stops after the thinning test (status 2, cand_logl = -inf, for a host likelihood to
 * fill) and needs no training set.  E outside [1, ALABI_NS_MAX_ELLIPSOIDS], M < 0 or a NULL table: ALABI_BAD_ARGUMENT. */
#define ALABI_NS_MAX_ELLIPSOIDS 32
int alabi_ns_unif_draw(alabi_ns* ns, long long call, int cand_id0, int M, int evaluate, int E, const double* centres,
                       const double* axes, const double* inv_axes, const double* cum, double* cand_u, double* cand_logl,
                       int* cand_status, void* stream);
/* The first `need` candidates, in candidate order, with status 2 and cand_logl > logl_star: rows to u_out [need,d] / logl_out
 * [need]; counts, device int32 [5]: taken, consumed (the index after the last taken candidate when `need` were found, else M; 0 for
 * need = 0), and the evaluated / outside / thinned candidates among the consumed. */
int alabi_ns_unif_select(alabi_ns* ns, int M, const double* cand_u, const double* cand_logl, const int* cand_status,
                         double logl_star, int need, double* u_out, double* logl_out, int* counts, void* stream);
/* The MLFriends region (UltraNest's bound, the replacement step of SurrogateModel.run_ultranest, alabi/core.py:3241-3690) over the
 * ellipsoids above: a candidate counts only if it lies within r of one of n live points in a whitened metric.  w, device [n,d]: the
 * whitened live points L^-1 p_i; metric_inv, device [d,d]: L^-1, row-major, lower triangle read (layout and draws in nested_mlf.hip).
 * alabi_ns_mlf_radius runs B bootstrap rounds: round b draws n indices with replacement, keyed by (seed, call, b), and writes
 * r2_out[b] = the largest squared distance from a point left out to the nearest point drawn (0 when none is left out); the caller
 * takes the maximum.  n outside [1, ALABI_NS_MLF_MAX_POINTS], B < 1 or a NULL array: ALABI_BAD_ARGUMENT, nothing launched. */
#define ALABI_NS_MLF_MAX_POINTS 16384
int alabi_ns_mlf_radius(alabi_ns* ns, long long call, int n, const double* w /* device [n,d] */, int B,
                        double* r2_out /* device [B] */, void* stream);
/* alabi_ns_unif_draw with one more test: a candidate that would get status 2 keeps it iff some j < n has
 * |metric_inv u - w_j|^2 <= r2, and gets status 1 otherwise, so that status 1 means "thinned, or no live point within r".
 * r2 = +inf gives the bits of alabi_ns_unif_draw, r2 = 0 keeps exact hits only.  Every check of alabi_ns_unif_draw, and n outside
 * [1, ALABI_NS_MLF_MAX_POINTS], a NaN or negative r2 or a NULL w / metric_inv: ALABI_BAD_ARGUMENT, nothing launched. */
int alabi_ns_mlf_draw(alabi_ns* ns, long long call, int cand_id0, int M, int evaluate, int E, const double* centres,
                      const double* axes, const double* inv_axes, const double* cum, int n, const double* w,
                      const double* metric_inv /* device [d,d], lower triangle read */, double r2,
                      double* cand_u, double* cand_logl, int* cand_status, void* stream);
/* Path of the last alabi_ns_walk / alabi_ns_slice / alabi_ns_unif_draw / alabi_ns_mlf_draw (evaluate = 1): 1 training set resident in registers, 2
 * tiled (point pairs beyond the block re-read from L2 every step). */
int alabi_ns_last_path(alabi_ns* ns, int* path /* host */);

/* Gaussian kernel density estimate: scipy.stats.gaussian_kde(dataset, bw_method, weights) as built and evaluated by the
 * reference's metrics, kl_divergence_kde (alabi/metrics.py:210-336: gaussian_kde(...) at :292-296, kde.pdf at :314-315).
 * The host computes the bandwidth (scipy's _compute_covariance; alabi_amd/kde.py); the library holds the whitened samples.
 * p(q) = det(2 pi S)^(-1/2) sum_i w_i exp(-|L^-1 (q - x_i)|^2 / 2), S = L L^T.  Results do not depend on the device:
 * the split of the sample axis is a function of (N, M, d) only, and repeated calls are bit-identical. */
int alabi_kde_create(int d, alabi_kde** out);
int alabi_kde_destroy(alabi_kde* kde);
/* Prepares the samples X [N,d] (row-major) once: centring, whitening by L, augmented rows.  logw [N] holds log w_i of
 * weights normalised to sum 1 (-inf for a zero weight); NULL = uniform 1/N.  cho_cov: host [d,d] row-major, lower
 * triangle read (scipy's kde.cho_cov).  Synchronises `stream`. */
int alabi_kde_set_data(alabi_kde* kde, const double* X, const double* logw, long long N, const double* cho_cov,
                       void* stream);
/* kde.logpdf(Q.T) -- scipy.stats.gaussian_kde.logpdf: out [M] = log p(Q [M,d]); finite where p underflows. */
int alabi_kde_logpdf(alabi_kde* kde, const double* Q, long long M, double* out, void* stream);
/* kde.pdf(Q.T) / kde.evaluate -- alabi/metrics.py:314-315: out [M] = p(Q [M,d]) (0 where it underflows, as scipy's). */
int alabi_kde_pdf(alabi_kde* kde, const double* Q, long long M, double* out, void* stream);
/* The split of the sample axis a call with M queries uses: `parts` ranges of `pts` samples (host ints). */
int alabi_kde_plan(alabi_kde* kde, long long M, int* parts, int* pts);

#ifdef __cplusplus
}
#endif
#endif /* ALABI_HIP_H */
