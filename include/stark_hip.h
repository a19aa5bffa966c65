/*
 * stark_hip.h -- C ABI of libstark_hip.so, the MI355X (gfx950) implementation of
 * stark's data-parallel hot path: subposterior NUTS sampling per data shard and the
 * consensus weighted-average combine.
 *
 * Each entry point replaces one reference interface (all paths under randommm/stark):
 *
 *   stk_model_create            stark/stark.py:37-39  Stark.setStanModel -> StanModel(**kw)
 *                               + stark/stark.py:46   data = callback(rows) (per partition)
 *   stk_model_create_synthetic  SURVEY.md 8d synthetic shards (bench; no host rows)
 *   stk_log_density_grad        Stan log_prob<propto=true,jacobian=true> + gradient, the
 *                               unit of work inside stark/stark.py:48 `sm.sampling`
 *   stk_log_density_grad_shards the same for every shard at once, one sweep launch per group
 *                               (parity hook; C must be a single batch size)
 *   stk_log_density_grad_chains the same at any C >= 1, through the chain batches and grouped
 *                               launches of a sampling run (parity hook)
 *   stk_chain_batches           the batches a regression shard's `chains` run as (host only)
 *   stk_sweep_launch_info       the kernel and launch shape one batch's sweep has at (rows, d, C) (host only)
 *   stk_model_create_sparse /   the same six regression families on CSR shards, kept as padded (index, value) rows:
 *   stk_model_sparse_info /     density hooks, sampler, fingerprints and checkpoints as on a dense model; the
 *   stk_chain_batches_sparse /  sparse batch table and launch shape (host only); the host twin of the sparse
 *   stk_sweep_launch_info_sparse / shard's fingerprint (no reference counterpart: the reference's rows are dense)
 *   stk_shard_fingerprint_sparse_host
 *   stk_fingerprint_words /     a 64-bit fingerprint of a shard's rows, on the device or the host;
 *   stk_shard_fingerprint_host / saved sampler states are bound to it (no reference counterpart)
 *   stk_model_fingerprint
 *   stk_sample / stk_sampler_*  stark/stark.py:48-56  `sm.sampling(data, **kw)` +
 *                               `fit.extract()` -> P x S matrix, for every local partition
 *                               (stark/stark.py:65 mapPartitions(_mcmc(...)))
 *   stk_transition              one Stan NUTS transition (parity hook, no adaptation)
 *   stk_transition_dense        the same under a full D x D inverse metric (Stan's dense_e);
 *                               stk_config.metric selects diag_e / dense_e / unit_e for a run
 *   stk_consensus_products      stark/stark.py:7-21   consensus_avg(J) reducer body
 *   stk_consensus_solve         stark/stark.py:66-70  inv(sum W) . sum W theta
 *   stk_consensus               stark/stark.py:66-70  reduce + solve over all shards
 *   stk_consensus_blocked       the same with block-diagonal weights (lp__ in its own block)
 *   stk_log_density_hessian /   the analytic Hessian of a regression shard's log density at one point, and the
 *   stk_hessian_launch_info /   combine with the caller's weights -- e.g. every shard's Laplace precision
 *   stk_consensus_weighted      W_s = -H_s, the exact consensus weights.  No reference counterpart: on the
 *                               product path they supersede tools/laplace.py's central difference of the
 *                               gradient (2 D gradient points per Hessian)
 *   stk_log_predictive /        per-row statistics over S draws (lppd, WAIC penalty, fitted mean) and their
 *   stk_predictive_launch_info  per-shard totals.  No reference counterpart
 *   stk_log_density_draws /     the log density of a shard at each of S draws in one pass over its rows, and the
 *   stk_logdens_launch_info /   Gaussian proposal draws of a Laplace fit: together the importance ratios of
 *   stk_laplace_draws           Laplace sampling (stark_amd.engine.laplace_sample).  No reference counterpart
 *   stk_log_density_grad_boot / log density + gradient of bootstrap replicates of a shard, 16 per pass over its rows,
 *   stk_boot_weights_host /     every row weighted by a Philox draw made in the kernel (Exp(1): the weighted-
 *   stk_boot_poisson_thresholds / likelihood bootstrap; Poisson(1): the classical one), the weights' host twin and
 *   stk_boot_launch_info        the launch shape (stark_amd.engine.bootstrap).  The reference's README names the
 *                               mode ("akin to a distributed bootstrap") without building it
 *   stk_posterior_predict /     posterior predictive replicates y_rep of every (row, draw), drawn in the kernel by a
 *   stk_yrep_host /             Philox generator, with their per-draw statistics and Pearson discrepancies, per-row
 *   stk_ppc_launch_info         counts and sums, the generator's host twin and the launch shape
 *                               (stark_amd.engine.ppc).  The reference extracts a Stan model's generated quantities
 *                               (stark/stark.py:49-56); the fixed families have no such block, so this supplies it
 *
 * Conventions
 *   - Return 0 on success, a negative STK_E_* code on failure; stk_last_error() gives a
 *     thread-local message.  No entry point ever falls back to a CPU computation.
 *   - Pointer arguments may be host or device memory (HIP unified addressing); the caller
 *     keeps ownership.  The library copies shard data to the device at model creation.
 *   - A context is bound to one device and one stream and is not thread-safe.  Multi-GPU
 *     runs use one process per GPU; the host side (stark_amd) exchanges draws with
 *     torch.distributed over RCCL.
 *   - Matrices are row-major fp64.  Draw matrices are "variables by samples" (P x S), the
 *     layout stark/stark.py:56 returns.
 */
#ifndef STARK_HIP_H
#define STARK_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STK_API __attribute__((visibility("default")))

typedef struct stk_ctx stk_ctx;
typedef struct stk_model stk_model;
typedef struct stk_sampler stk_sampler;

enum {
  STK_OK = 0,
  STK_E_ARG = -1,      /* invalid argument                                   */
  STK_E_HIP = -2,      /* HIP runtime error (no device, launch failure, ...)  */
  STK_E_NOMEM = -3,    /* device allocation failed                            */
  STK_E_STATE = -4,    /* call out of order                                   */
  STK_E_NUMERIC = -5,  /* step size left (0, 1e7] (Stan's init_stepsize error) */
  STK_E_NAN = -6,      /* every shard holds NaN draws (combine)               */
  STK_E_LINALG = -7    /* singular matrix in the combine (LinAlgError)        */
};

/* Model families. */
enum { STK_SCHOOLS = 1, STK_LINREG = 2, STK_LOGREG = 3, STK_POISSON = 4, STK_NEGBIN = 5, STK_STUDENT = 6, STK_GAMMA = 7,
       STK_CATEGORICAL = 8 };
/* STK_POISSON: y ~ poisson_log(alpha + x * beta), the unconstrained parameters (alpha, beta[1..d]) in
 * the logistic layout (D = d + 1, P = d + 2: alpha, beta, lp__).  With eta_i = alpha + x_i . beta and
 * mu_i = exp(eta_i), lp = sum_i (y_i eta_i - mu_i) (+ the normal(0, s) prior terms of
 * stk_model_set_prior), d lp / d alpha = sum_i (y_i - mu_i), d lp / d beta = sum_i x_i (y_i - mu_i):
 * Stan 2.19's poisson_log_lpmf<propto = true>, which drops lgamma(y + 1) (parity unpinned at Stan).
 * eta enters y_i eta_i as it is; mu overflows to +inf and underflows to 0 on its own, so where a
 * row's exp overflows lp is -inf (NaN when y_i eta_i overflowed too), never a finite number, and a
 * NaN eta stays NaN: the NUTS machine takes such a leaf as divergent, as Stan does.
 * Everything a logistic model can do works for the family (every entry point below, the three
 * metrics, both U-turn criteria, saved states), with two refusals, each STK_E_ARG with a message that
 * names the family: stk_model_create_synthetic (the generator has no Poisson form) and
 * stk_sampler_set_allreduce (full-data mode stays logistic-only). */
/* STK_NEGBIN: y ~ neg_binomial_2_log(alpha + x * beta, phi), the unconstrained parameters (alpha,
 * beta[1..d], v = log phi) in the linear layout with phi where sigma is (D = d + 2, P = d + 3: alpha,
 * beta, phi = e^v, lp__).  With eta_i = alpha + x_i . beta, t_i = eta_i - v, sp(t) = log(1 + e^t) and
 * sigma(t) = 1 / (1 + e^-t), Stan's neg_binomial_2_log_lpmf<propto = true> (it drops lgamma(y + 1);
 * logsumexp(eta, log phi) = v + sp(t); parity unpinned at Stan, as for Poisson) is
 *   ll_i       = sum_{j < y_i} log1p(j / phi) + y_i eta_i - (y_i + phi) sp(t_i)
 *   d ll_i / d eta = y_i - (y_i + phi) sigma(t_i)          -> d alpha = sum_i, d beta = X^T (.)
 *   d lp / d v = phi sum_i [psi(y_i + phi) - psi(phi)] - d alpha_lik - phi sum_i sp(t_i) + (prior) + 1
 *   lp         = sum_i ll_i + priors + v                   (the Jacobian of phi = e^v)
 * a form without cancelling y v terms.  The phi-only sums depend on the shard's count histogram alone:
 * with T_j = #{i : y_i > j}, sum_i sum_{j < y_i} log1p(j / phi) = sum_j T_j log1p(j / phi) and sum_i
 * [psi(y_i + phi) - psi(phi)] = sum_j T_j / (phi + j).  stk_model_create builds each shard's table once
 * (T_j for j < 1024; the distinct counts past that with their multiplicities, whose remaining terms come
 * from the asymptotic series of lgamma and digamma); it lives on the device next to the shard, is
 * released with the model and is no part of the fingerprint.  The sweep evaluates neither lgamma nor
 * digamma: the table terms are added once per (shard, chain) in the reduce.
 * Priors: stk_model_set_prior (normal on alpha and beta) and stk_model_set_prior_phi (gamma on phi; flat by
 * default, as Stan runs the flat program: the posterior is then improper in phi).
 * There is no switch to Poisson at large phi.  Where e^v overflows or underflows to 0, or a row's exp
 * overflows, lp is NaN or -inf: never a finite number and never +inf.
 * The sampler (any chains, the three metrics, both U-turn criteria, saved states), the gradient hooks,
 * data copy-out and the fingerprints work for the family.  Refused by name with STK_E_ARG, before any
 * work: stk_model_create_synthetic, stk_sampler_set_allreduce and the analysis sweeps
 * (stk_log_density_hessian, stk_log_predictive, stk_loo, stk_log_density_draws,
 * stk_log_density_grad_boot, stk_posterior_predict). */
/* STK_STUDENT: y ~ student_t(nu, alpha + x * beta, sigma) with nu > 0 a constant of the model
 * (stk_model_set_student_nu; never a parameter), the unconstrained parameters (alpha, beta[1..d],
 * s = log sigma) in the linear layout (D = d + 2, P = d + 3: alpha, beta, sigma = e^s, lp__) and the
 * shard's double y, as linear.  With eta_i = alpha + x_i . beta, z_i = (y_i - eta_i) / sigma and
 * w_i = z_i^2 / nu, the `~` statement's density on the unconstrained scale is
 *   lp             = -(nu + 1)/2 sum_i log1p(w_i) - n s + s    (+ the normal(0, scale) priors of stk_model_set_prior)
 *   d lp / d eta_i = (nu + 1) z_i / (sigma (nu + z_i^2))       -> d alpha = sum_i, d beta = X^T (.)
 *   d lp / d s     = (nu + 1) sum_i z_i^2 / (nu + z_i^2) - n + 1
 * (the last s and + 1: the Jacobian of sigma = e^s).  lgamma((nu + 1)/2) - lgamma(nu/2) - log(nu pi)/2 per row
 * is a constant under `~` with nu as data: Stan drops it and so does the library.  The row term needs a log1p
 * over the whole half-line (an outlier's w is large, a large nu's tiny): st_log1p of csrc/student_math.h, a few
 * ulp from 0 to +inf, so that at nu = 1e6 the density tends to the linear family's without losing digits.
 * The posterior is not log-concave.  Where z_i^2 overflows a double lp is -inf or NaN: never a finite wrong
 * number and never +inf.
 * There is no default nu: until stk_model_set_student_nu has been called every density, transition and sampler
 * entry point refuses the model (STK_E_ARG) with a message that says so.  nu is part of what
 * stk_sampler_load_state compares: a state saved at nu = 4 is refused by a model at nu = 5.
 * The sampler (any chains, the three metrics, both U-turn criteria, saved states), the gradient hooks,
 * stk_model_set_prior, data copy-out and the fingerprints treat the family as they treat STK_LINREG.  Refused by
 * name with STK_E_ARG, before any work: stk_model_create_synthetic, stk_sampler_set_allreduce and the analysis
 * sweeps (stk_log_density_hessian, stk_log_predictive, stk_loo, stk_log_density_draws,
 * stk_log_density_grad_boot, stk_posterior_predict). */
/* STK_GAMMA: y ~ gamma(shape, shape ./ exp(alpha + x * beta)), the gamma GLM with the log link (mean exp(eta),
 * variance mean^2 / shape), the unconstrained parameters (alpha, beta[1..d], u = log shape) in the linear layout
 * with shape where sigma is (D = d + 2, P = d + 3: alpha, beta, shape = e^u, lp__) and the shard's double y, every
 * value finite and > 0 (stk_model_create returns STK_E_ARG and names the first row that is not).  With a = e^u,
 * n rows, eta_i = alpha + x_i . beta, ly_i = log y_i, L = sum_i ly_i and t_i = ly_i - eta_i, the `~` statement's
 * density on the unconstrained scale is
 *   lp             = n kappa(a) - L - a H + u       (+ the priors of stk_model_set_prior / stk_model_set_prior_shape)
 *   kappa(a)       = a log a - a - lgamma(a)
 *   H              = sum_i h(t_i),   h(t) = e^t - 1 - t >= 0
 *   d lp / d eta_i = a (e^{t_i} - 1)                -> d alpha = sum_i, d beta = X^T (.)
 *   d lp / d u     = a [n kappa'(a) - H] + 1,       kappa'(a) = log a - psi(a)
 * (the last u and + 1: the Jacobian of shape = e^u).  This is Stan's gamma_lpdf(y | a, a e^-eta) term for term:
 * shape is a parameter, so nothing is dropped, (a - 1) log y with its -log y part included.  It is written as a
 * deviance because the textbook form n (a log a - lgamma a) + (a - 1) L - a sum_i (eta_i + y_i e^-eta_i) cancels
 * a n against a L and loses lp's last digits on precise data (shape 1e4 and up).  The library therefore keeps, next
 * to y as given (what stk_model_copy_data returns and the fingerprints cover), ly = log y as the array its sweeps
 * read, and L summed once in a fixed order.  kappa and kappa' are never formed from lgamma(a) or digamma(a) (at
 * a = 1e8 kappa is 8, left over from terms of 1.8e9): csrc/gamma_math.h sums their Stirling remainders, by a
 * recurrence below a = 16; stk_gamma_shape_terms_host runs the same code on the host.
 * Where e^t overflows a double lp is -inf or NaN, never +inf and never a finite number; a NaN eta or u stays NaN;
 * a = 0 or inf (exp(u) under- or overflowed) gives NaN.
 * The sampler (any chains, the three metrics, both U-turn criteria, saved states: the family and the shape prior
 * are part of a saved state's geometry), the gradient hooks, stk_model_set_prior, data copy-out and the
 * fingerprints treat the family as they treat STK_LINREG.  Refused by name with STK_E_ARG, before any work:
 * stk_model_create_synthetic, stk_sampler_set_allreduce and the analysis sweeps (stk_log_density_hessian,
 * stk_log_predictive, stk_loo, stk_log_density_draws, stk_log_density_grad_boot, stk_posterior_predict). */
/* STK_CATEGORICAL: y[n] ~ categorical_logit(append_row(alpha + x[n] * beta, 0)), softmax regression with K = ncat >= 2
 * classes (stk_model_set_categories; never a default), G = K - 1 free classes and class K the reference (eta = 0).
 * The unconstrained point is Stan's own order with nothing constrained: q = [alpha_1 .. alpha_G, beta_1[0 .. d), ...,
 * beta_G[0 .. d)] -- class g's coefficients are the g-th block of d, the column-major vector of models/categorical.stan
 * -- so D = G (d + 1) and P = D + 1 (alpha[1..G], beta[1..G d], lp__).  The shard is x and y_int in [1, K] as given.
 * With eta_ig = alpha_g + x_i . beta_g, m_i = max(0, max_g eta_ig) and s_i = e^{-m_i} + sum_g e^{eta_ig - m_i},
 *   lp               = sum_i (eta_{i, y_i} - m_i - log s_i)        eta_{i, K} = 0   (+ the priors of stk_model_set_prior)
 *   d lp / d eta_ig  = 1[y_i = g] - e^{eta_ig - m_i} / s_i          -> d alpha_g = sum_i, d beta_g = X^T (.)
 * (`~`: nothing to drop).  stk_model_set_prior's normal(0, s) priors apply to every alpha_g and to every beta entry.
 * The maximum is subtracted so that coefficients of any size that keep eta finite give a finite lp; a NaN eta stays
 * NaN in lp and the gradient; where an eta is +-inf lp is -inf or NaN, never +inf and never a finite number.
 * Envelope: G <= 16 and G ceil(d / 16) <= 16 (K = 2 to d = 256, K = 3 to d = 128, K = 5 to d = 64, K = 9 to d = 32,
 * K = 17 to d = 16), the accumulator tiles of k_sweep_cat (csrc/sweep_cat.hip).  Outside it stk_model_set_categories
 * returns STK_E_ARG with a message that names K and d, before anything is launched; so do the hooks and
 * stk_sampler_create for a model that never had its categories set.
 * Chains run in launches of up to 16: C chains are C / 16 launches of 16 and one of C mod 16
 * (stk_chain_batches_categorical); a chain's lp and gradient are the same bits in whichever batch and column.
 * The sampler (any chains, the three metrics, both U-turn criteria, saved states: K is part of a saved state's
 * geometry), the gradient hooks, stk_model_set_prior, data copy-out and the fingerprints (y as given) work for the
 * family.  Refused by name with STK_E_ARG, before any work: stk_model_create_sparse, stk_model_create_synthetic,
 * stk_sampler_set_allreduce, the analysis sweeps (stk_log_density_hessian, stk_log_predictive, stk_loo,
 * stk_log_density_draws, stk_log_density_grad_boot, stk_posterior_predict) and stk_yrep_host. */

/* One data shard (= one Spark partition, stark/stark.py:35).
 *   schools: n_rows = J, y[J], sigma[J]                   (example/stark_ex.py:8-11)
 *   linreg : x[n_rows * n_cols] row-major, y[n_rows]
 *   logreg : x[n_rows * n_cols] row-major, y_int[n_rows] in {0, 1}
 *   poisson: x[n_rows * n_cols] row-major, y_int[n_rows] >= 0 (checked on the device copy: the
 *            first negative row is named in the error); y and sigma must be NULL -- counts
 *            handed over as doubles as well as ints are refused (STK_E_ARG), here and by
 *            stk_shard_fingerprint_host, instead of one of the two being ignored
 *   negbin : as poisson (x, y_int >= 0, y and sigma NULL)
 *   student: as linreg (x, y)
 *   gamma  : as linreg (x, y), every y finite and > 0
 *   categorical: x, y_int[n_rows] in [1, K] (checked on the device copy by stk_model_set_categories, which
 *            names the first row outside); y and sigma must be NULL                  */
typedef struct {
  int64_t n_rows;
  int32_t n_cols;
  const double* x;
  const double* y;
  const int32_t* y_int;
  const double* sigma;
} stk_shard;

/* Sampler configuration: pystan 2 `sampling()` keywords (stark/stark.py:48, defaults
 * stark/stark.py:60-64) and the Stan control block.  stk_config_default() fills Stan's
 * defaults (iter 2000 -> 1000 warmup + 1000 draws, chains 1 as stark forces, max_depth 10,
 * adapt_delta 0.8, gamma 0.05, kappa 0.75, t0 10, stepsize 1, init U(-2,2), buffers 75/50/25). */
typedef struct {
  int32_t num_warmup;
  int32_t num_samples;
  int32_t chains;            /* chains per shard: any count >= 1; regressions run it as the batches of
                                stk_chain_batches (stark/stark.py:48 forwards `chains` untouched) */
  int32_t max_depth;         /* 1..30.  8 schools: the fused kernel holds a chain's 17 vectors and
                                max_depth x 4 (stan2.19) or x 7 (stan2.23) stack vectors of
                                Dp = roundup8(J + 2) doubles in LDS; a config whose image exceeds the
                                CU's 160 KiB (only J >= 79 can: e.g. J = 126, stan2.23, max_depth >= 20)
                                is refused with STK_E_ARG by stk_sampler_create */
  double adapt_delta, adapt_gamma, adapt_kappa, adapt_t0;
  double stepsize;           /* initial nominal step size */
  double init_radius;        /* inits ~ U(-R, R) on the unconstrained scale */
  int32_t adapt_init_buffer, adapt_term_buffer, adapt_window;
  int32_t adapt_engaged;
  uint64_t seed;
  const double* init;        /* NULL, or nshards * chains * D unconstrained inits (shard-major,
                                every chain of a shard at that shard's own D, no padding) */
  const double* inv_metric;  /* NULL (unit), or D initial diagonal inverse metric */
  int32_t skip_init_stepsize;/* test hook: do not run base_hmc::init_stepsize */
  int32_t iter_offset;       /* test hook: RNG iteration index of the first transition */
  int32_t save_warmup;       /* also keep unconstrained warmup draws (pystan inc_warmup):
                                stk_sampler_draws_unconstrained then returns all iterations */
  const int32_t* shard_ids;  /* NULL, or the GLOBAL index of every local shard: chain c of shard s
                                draws from RNG stream shard_ids[s] * chains + c, so a shard samples
                                identically whichever GPU (and with whichever other shards) it runs */
  double stepsize_jitter;    /* Stan control stepsize_jitter in [0, 1]: every transition uses
                                stepsize * (1 + jitter * U(-1, 1)) (base_hmc::sample_stepsize) */
  int32_t nuts_criterion;    /* 0 (default): Stan 2.19.1's U-turn test across each merged subtree, as
                                the reference's pystan 2 runs it; 1: also the two tests across the
                                junction of the merged halves that Stan >= 2.23 adds (base_nuts
                                build_tree / transition), which stop the trajectories that the single
                                test lets run on near-isotropic Gaussian posteriors */
  int32_t chains_per_wave;   /* 8-schools fused kernel: chains packed per 64-lane wave, 0 (default) =
                                the most that fit (4 for D <= 16, 2 for D <= 32, else 1); 1 or 2 cap
                                it (test hook: the packing changes no bit of the draws) */
  int32_t metric;            /* Stan's metric: 0 (default) diag_e, 1 dense_e, 2 unit_e.
                                dense_e: every chain adapts a full D x D inverse metric in the diag_e
                                windows (covar_adaptation: Welford covariance, regularised as
                                (n/(n+5)) cov + 1e-3 (5/(n+5)) I) and draws p = L^-T u, M^-1 = L L^T;
                                regression families only (D <= 1024), refused for 8 schools.  A chain
                                whose new metric is not positive definite stops like a step-size error
                                (counted in stk_run_info.errors).
                                unit_e: the metric stays I (inv_metric is ignored), only the step size
                                adapts; every family */
  const double* inv_metric_dense; /* dense_e: NULL (identity), or the D x D row-major symmetric
                                positive definite initial inverse metric (else STK_E_ARG) */
} stk_config;

typedef struct {
  int64_t grad_evals;   /* chain-gradient evaluations issued (all local chains)          */
  int64_t leapfrogs;    /* leapfrog steps inside NUTS trajectories                        */
  int64_t steps;        /* state-machine steps launched                                   */
  int64_t sweeps;       /* steps whose data sweeps ran (regression families)              */
  double sweep_ms;      /* summed HIP-event time of those steps' sweep kernels (profiling on only);
                           one step's event pair spans the sweeps of all its chain batches  */
  int32_t divergent;    /* divergent transitions after warmup                             */
  int32_t errors;       /* chains stopped by a step-size error                            */
  int32_t min_iter;     /* fewest transitions completed by any chain                      */
  int32_t done;         /* chains that completed num_warmup + num_samples                 */
  int64_t shard_sweeps; /* shard passes inside those sweeps, one per shard per chain-batch launch
                           (bytes = shard_sweeps * n*(8d+4))                               */
} stk_run_info;

STK_API const char* stk_last_error(void);
STK_API int stk_version(void);
STK_API void stk_config_default(stk_config* cfg);

/* ---- context: one device, one stream ---- */
STK_API int stk_ctx_create(int device, stk_ctx** out);
STK_API int stk_ctx_destroy(stk_ctx* ctx);
STK_API int stk_ctx_sync(stk_ctx* ctx);
/* A context on the caller's HIP stream (e.g. torch.cuda.current_stream().cuda_stream), so library
 * kernels and the caller's collectives on that stream are ordered without host syncs (NULL: the
 * null stream, which is torch's default current stream).  The stream is not destroyed with the
 * context. */
STK_API int stk_ctx_create_on_stream(int device, void* stream, stk_ctx** out);
/* HIP events around the data sweeps of every on-th split-mode step (0: off; 1: every step).
   Each event pair is a barrier on the stream: sample (e.g. 8) to keep the timing cheap. */
STK_API int stk_ctx_set_profiling(stk_ctx* ctx, int on);
STK_API void* stk_ctx_stream(stk_ctx* ctx);                /* hipStream_t of the context */

/* ---- models: stark/stark.py:37-39 + :46 ---- */
STK_API int stk_model_create(stk_ctx* ctx, int family, const stk_shard* shards, int nshards, stk_model** out);
/* Synthetic shards generated on the device: global rows
 * [row_offset + s*rows_per_shard, row_offset + (s+1)*rows_per_shard) for shard s.  STK_LINREG and
 * STK_LOGREG only: STK_POISSON is refused (STK_E_ARG), the generator draws no counts. */
STK_API int stk_model_create_synthetic(stk_ctx* ctx, int family, int nshards, int64_t rows_per_shard,
                                       int64_t row_offset, int32_t n_cols, uint64_t data_seed,
                                       double alpha, const double* beta, double noise_sigma,
                                       stk_model** out);
STK_API int stk_gen_beta(uint64_t data_seed, int32_t n_cols, double* beta);   /* host, beta ~ N(0, 1/d) */
/* Regressions (linear, logistic, poisson): alpha ~ normal(0, alpha_scale), beta ~ normal(0, beta_scale) (each 0 or inf = flat,
 * the default) -- the priors of a `model` block the front end recognises (stark/stark.py:37-39
 * setStanModel of such a program).  Applies to every shard, before sampling. */
STK_API int stk_model_set_prior(stk_model* m, double alpha_scale, double beta_scale);
/* STK_NEGBIN only: phi ~ gamma(shape, rate), which adds (shape - 1) v - rate e^v to lp (exponential(r)
 * is gamma(1, r)).  shape > 0, rate >= 0; (1, 0) is flat, the default.  Every shard, before sampling. */
STK_API int stk_model_set_prior_phi(stk_model* m, double shape, double rate);
/* STK_GAMMA only: shape ~ gamma(shape, rate), which adds (shape - 1) u - rate e^u to lp (exponential(r) is
 * gamma(1, r)).  shape > 0, rate >= 0; (1, 0) is flat, the default.  Any other family is refused by name.
 * Every shard, before sampling. */
STK_API int stk_model_set_prior_shape(stk_model* m, double shape, double rate);
/* The shape-only terms of STK_GAMMA at shape a, by the code the device runs: out2[0] = kappa(a) =
 * a log a - a - lgamma(a), out2[1] = kappa'(a) = log a - psi(a) > 0.  a = 0, inf or NaN gives NaN for both.
 * No device is touched. */
STK_API int stk_gamma_shape_terms_host(double a, double* out2);
/* STK_STUDENT only: the degrees of freedom nu of y ~ student_t(nu, ., sigma), finite and > 0 (else STK_E_ARG
 * with the value in the message; any other family is refused by name).  Required before any density,
 * transition or sampler call: there is no default.  Every shard, before sampling. */
STK_API int stk_model_set_student_nu(stk_model* m, double nu);
/* STK_CATEGORICAL only: the classes K = ncat >= 2 of y ~ categorical_logit (any other family is refused by name).
 * Called once, before any density, transition or sampler call: there is no default, and a second call is refused.
 * It sets D = (K - 1)(d + 1) and P = D + 1 of every shard, refuses a (K, d) outside the envelope
 * ((K - 1) <= 16, (K - 1) ceil(d / 16) <= 16, (K - 1)(d + 1) <= 1024) with a message that names K and d, and checks
 * every shard's y_int on the device: the first value outside [1, K] is refused with its shard and row named, and the
 * model stays without categories. */
STK_API int stk_model_set_categories(stk_model* m, int32_t ncat);
/* Whether k_sweep_cat covers K = ncat classes at d covariates (1 / 0), and the launches C chains of such a shard
 * run as: C / 16 of 16 chains, then one of C mod 16 (the contract of stk_chain_batches).  Host only: no device. */
STK_API int stk_categorical_supported(int32_t ncat, int32_t d);
STK_API int stk_chain_batches_categorical(int32_t C, int32_t d, int32_t ncat, int32_t* sizes, int32_t cap);
/* The two phi-only sums of STK_NEGBIN over n counts y_int >= 0 at phi > 0, computed on the host by the
 * code the device runs (its table builder and term functions): out[0] = sum_i sum_{j < y_i} log1p(j / phi),
 * out[1] = sum_i [psi(y_i + phi) - psi(phi)].  No device is touched. */
STK_API int stk_negbin_phi_terms_host(const int32_t* y_int, int64_t n, double phi, double* out);
STK_API int stk_model_destroy(stk_model* m);
STK_API int stk_model_info(const stk_model* m, int shard, int32_t* D, int32_t* P, int64_t* n_rows);
STK_API int stk_model_copy_data(stk_model* m, int shard, double* x, double* y, int32_t* y_int);
STK_API int stk_model_device_bytes(const stk_model* m, int64_t* bytes);

/* ---- data fingerprint: a cheap, position-sensitive 64-bit fingerprint of a shard's rows, computed
 * where they lie (one HBM-speed read), with a host twin that gives the same bits -- to check rows
 * before an upload or on another rank, and what a saved sampler state is bound to (below).  It is
 * not cryptographic: it detects accidents (other rows, swapped rows, one flipped bit, a shifted
 * slice), not an adversary.  No reference counterpart.  All arithmetic is on unsigned 64-bit
 * integers, modulo 2^64:
 *
 *   K = 0x9E3779B97F4A7C15        M = 0xD6E8FEB86659FD93
 *   fmix(a):  a ^= a >> 32;  a *= M;  a ^= a >> 29;  return a
 *   T[0..4] = 0x243F6A8885A308D3, 0x13198A2E03707344, 0xA4093822299F31D0,
 *             0x082EFA98EC4E6C89, 0x452821E638D01377
 *   words(w[0..m), tag, index0) = sum over i < m of  fmix( w[i] + (index0 + i + 1) * K + T[tag] )
 *
 * A stream of doubles contributes the doubles' bit patterns (-0.0 differs from 0.0, NaN payloads
 * count); a stream of int32 contributes every element's 32-bit pattern zero-extended to 64 bits,
 * and its index counts elements.  words is additive over index ranges,
 * words(a ++ b, t, i0) = words(a, t, i0) + words(b, t, i0 + len(a)), and an integer sum, so every
 * reduction order gives the same bits.
 *
 *   shard fingerprint = fmix( words([family, n_rows, n_cols], 0, 0)     n_cols = 0 for schools; family is
 *                                                                        the STK_* value (poisson: 4, negbin: 5, student: 6, gamma: 7)
 *                           + words(x: n_rows * n_cols doubles, row-major, 1, 0)   regressions
 *                           + words(y doubles, 2, 0)                    linreg, student, gamma, schools
 *                           + words(y_int int32, 3, 0)                  logreg, poisson, negbin
 *                           + words(sigma doubles, 4, 0) )              schools
 *
 * Priors are not part of it (the saved state's geometry check covers them).
 *
 * stk_fingerprint_words: *sum = words(buf[0..count), tag, index0), word_bytes 8 or 4 (buf aligned
 * to it).  With a context it runs on the context's device and stream; buf may be device memory
 * (read in place) or host memory (staged).  ctx == NULL asks for the host twin: buf must be host
 * memory and no device is needed.  STK_E_ARG: word_bytes not 4 or 8, tag outside 0..4, count < 0,
 * buf NULL with count > 0; count == 0 gives 0.
 * stk_shard_fingerprint_host: the fingerprint of one shard of host pointers (the struct
 * stk_model_create takes, the same pointers required per family); pure host code.
 * stk_model_fingerprint: the same value from the shard's device arrays; computed at the first
 * call for that shard and cached (the data never changes after creation), so model creation and
 * runs that never ask pay nothing. */
STK_API int stk_fingerprint_words(stk_ctx* ctx, const void* buf, int64_t count, int32_t word_bytes, int32_t tag,
                                  uint64_t index0, uint64_t* sum);
STK_API int stk_shard_fingerprint_host(int family, const stk_shard* shard, uint64_t* out);
STK_API int stk_model_fingerprint(stk_model* m, int shard, uint64_t* out);
/* The shard's arrays where the model keeps them: *out is filled with n_rows, n_cols and the DEVICE
 * addresses of x / y / y_int / sigma (NULL for the arrays the family has not), read-only and valid
 * while the model lives -- e.g. to fingerprint a row range with stk_fingerprint_words. */
STK_API int stk_model_shard_arrays(const stk_model* m, int shard, stk_shard* out);

/* ---- log density + gradient at C points of one shard (parity hook) ---- */
STK_API int stk_log_density_grad(stk_model* m, int shard, const double* q, int32_t C, double* lp, double* grad);
/* lp and gradient of EVERY shard at C points each (parity hook): one sweep launch per group; C
 * must be a single batch size.  q: [nshards][C][D], lp: [nshards][C], grad: [nshards][C][D]
 * (grad may be NULL).  Regressions only. */
STK_API int stk_log_density_grad_shards(stk_model* m, const double* q, int32_t C, double* lp, double* grad);
/* The same arrays at ANY C >= 1, run through exactly the chain batches (stk_chain_batches) and
 * grouped launches of a sampling run at chains = C (parity hook).  Regressions only. */
STK_API int stk_log_density_grad_chains(stk_model* m, const double* q, int32_t C, double* lp, double* grad);
/* The contiguous chain batches that the C chains of a regression shard with d covariates run as:
 * greedy, largest first, over the single-launch sizes {64, 16, 8, 4, 2, 1} that a sweep covers at
 * d (1, 2, 4, 8, 16: d <= 1024; 64: any d), no padding -- e.g. d = 100: 3 = 2 + 1, 17 = 16 + 1, 70 = 64 + 4 + 2.  A pure host
 * function of (C, d): needs no device and is the same on every rank.  Writes the first `cap` sizes
 * (sizes may be NULL when cap is 0) and returns the number of batches, or STK_E_ARG (C < 1, or no
 * sweep covers d).  Chain c of shard s keeps RNG stream shard_ids[s] * chains + c, and every
 * layout (draws, stats, the full-data block, the saved state) is that of a single batch. */
STK_API int stk_chain_batches(int32_t C, int32_t d, int32_t* sizes, int32_t cap);
/* The sweep that one batch of C chains (a size stk_chain_batches returns) runs over a shard of
 * n_rows rows and d covariates, as the sampler and the parity hooks launch it.  out[0] kind: 1 k_sweep,
 * 2 k_sweep2, 3 k_sweep3, 4 k_sweep16, 5 the 64-chain GEMM passes, 6 k_sweep16w; out[1] rows per tile;
 * out[2] the kernel's LD argument (kinds 1, 2: LDS row stride in doubles; 3: ring slots per wave; 4: 1;
 * 5: 0; 6: waves per block); out[3] chunks per shard; out[4] dynamic LDS bytes per block; out[5] bytes
 * of 64-chain workspace per shard (0 unless kind 5).  A pure host function of (n_rows, d, C): needs no
 * device.  STK_E_ARG when C is not a batch size at d, or when no sweep covers the shape (a shard so
 * long that one of its chunks does not fit a buffer descriptor) -- the shapes stk_sampler_create and
 * the stk_log_density_grad* hooks refuse with the same code before they launch anything. */
STK_API int stk_sweep_launch_info(int64_t n_rows, int32_t d, int32_t C, int64_t out[6]);

/* ---- sparse design matrices: a second storage for the six regression families ----
 * One shard of a sparse model, in CSR: row r's entries are indices / values [indptr[r], indptr[r + 1]).
 * y / y_int are those of stk_shard for the family (logreg, poisson, negbin: y_int; linreg, student, gamma: y).
 * Checked before anything is launched (STK_E_ARG names the shard and the row): indptr[0] = 0 and indptr
 * non-decreasing; every index in [0, n_cols); indices strictly increasing within a row (duplicates are the
 * caller's to sum); every value finite.  An index outside [0, n_cols) would be an out-of-bounds access on the
 * device, so the check is never skipped.  The arrays may be host or device memory (device arrays are copied
 * back for the check).  The y checks are those of stk_model_create. */
typedef struct {
  int64_t n_rows;
  int32_t n_cols;
  const int64_t* indptr;    /* [n_rows + 1] */
  const int32_t* indices;   /* [indptr[n_rows]] */
  const double* values;     /* [indptr[n_rows]] */
  const double* y;
  const int32_t* y_int;
} stk_shard_sparse;
/* A model whose every shard is sparse (a model is all sparse or all dense).  On the device a shard is kept as
 * padded rows (ELL): K = the shard's longest row, idx[n_rows][K] int32 and val[n_rows][K] double, a short row
 * padded with (0, 0.0) -- 12 K bytes per row instead of 8 n_cols; K may be 0 and may reach n_cols; one long row
 * inflates K for its whole shard.  The priors, stk_model_set_student_nu, the density hooks (stk_log_density_grad,
 * _shards, _chains), the sampler (every chain count, the three metrics, both U-turn criteria, stk_transition*,
 * stk_sample), fingerprints and checkpoints work as on a dense model; the sweeps are k_sweep_sp (kind 7).  The
 * analysis sweeps (Hessian, log-predictive, PSIS-LOO, per-draw log density, bootstrap, posterior predictive) and
 * full-data mode (stk_sampler_set_allreduce) refuse a sparse model with STK_E_ARG and a message that says so. */
STK_API int stk_model_create_sparse(stk_ctx* ctx, int family, const stk_shard_sparse* shards, int nshards, stk_model** out);
/* out[0] = K, out[1] = nnz (the entries handed over, explicit zeros among them), out[2] = device bytes of
 * the padded rows, 12 K n_rows.  STK_E_ARG for a dense model.  stk_model_shard_arrays reports x = NULL. */
STK_API int stk_model_sparse_info(const stk_model* m, int shard, int64_t out[3]);
/* The chain batches of a SPARSE shard's C chains at d covariates: greedy, largest first, over {16, 8, 4, 2, 1}
 * for d <= 512 and {8, 4, 2, 1} for 512 < d <= 1024 (beta and the gradient of 16 chains no longer fit a CU's
 * LDS); there is no 64-chain sparse pass.  A pure host function of (C, d), the contract of stk_chain_batches. */
STK_API int stk_chain_batches_sparse(int32_t C, int32_t d, int32_t* sizes, int32_t cap);
/* The sparse sweep of one batch of C chains over n_rows x d with longest row K (host only).  out[0] kind (7);
 * out[1] rows per tile; out[2] bytes of the entry stage in LDS; out[3] chunks per shard (a function of n_rows
 * alone); out[4] dynamic LDS bytes per block; out[5] private gradient copies per block (4, 2 or 1); out[6] 1 when
 * a tile's entries (12 K bytes per row) are staged in LDS, 0 when the kernel reads them from global memory --
 * the same bits either way; out[7] bytes of the shard's padded rows, 12 K n_rows. */
STK_API int stk_sweep_launch_info_sparse(int64_t n_rows, int32_t d, int32_t K, int32_t C, int64_t out[8]);
/* The fingerprint of a sparse shard.  With the padded rows idx / val as the device keeps them,
 *   fmix( words([family, n_rows, n_cols, K], 0, 0) + words(idx: n_rows K int32, 5, 0) + words(val: n_rows K
 *         doubles, 6, 0) + words(y, 2, 0) or words(y_int, 3, 0) )
 * with two tags of its own, T[5] = 0xBE5466CF34E90C6C and T[6] = 0xC0AC29B7C97C50DD, and a four-word header, so
 * that a sparse shard and the dense shard of the same matrix never share one.  stk_model_fingerprint gives the
 * same bits from the device arrays; a state saved against the dense model of the same matrix is refused as
 * saved against other data.  Host only; validates the shard as stk_model_create_sparse does. */
STK_API int stk_shard_fingerprint_sparse_host(int family, const stk_shard_sparse* shard, uint64_t* out);

/* ---- analytic Hessian (regression families, 1 <= d <= 128): one weighted Gram matrix
 * X~^T diag(w) X~, X~ = [1 | X], accumulated on the fp64 MFMA in a single pass over the shard ----
 * Hessian of the log density of shard `shard` at q[D] -> hess[D][D] (row-major, symmetric to the bit),
 * with respect to the unconstrained parameters in the gradient's layout ((alpha, beta) for logistic and
 * poisson, (alpha, beta, u = log sigma) for linear); the normal(0, s) priors of stk_model_set_prior add
 * -1/s^2 on the diagonal entries they cover.
 * shard == -1: every shard at its own point, q [nshards][D], hess [nshards][D][D], lp [nshards],
 * grad [nshards][D], the Hessians in one grouped launch.  lp / grad may be NULL; when given they are what
 * stk_log_density_grad returns at q, bit for bit (they ARE its C = 1 sweep, one per shard).  The result is bitwise independent of how many shards
 * share the call and of the device.  A NaN eta or an overflowing poisson mu gives non-finite entries and
 * still STK_OK: the caller decides.  Regressions with d <= 128; STK_E_ARG (the message names the family
 * or the limit) for 8 schools and for d > 128. */
STK_API int stk_log_density_hessian(stk_model* m, int shard, const double* q, double* lp, double* grad, double* hess);
/* host only, like stk_sweep_launch_info: out[0] rows per tile, out[1] chunks per shard, out[2] waves per
 * block, out[3] dynamic LDS bytes, out[4] bytes of chunk-partial workspace per shard.  The three families
 * share one geometry (d + 2 live columns: x, the ones column, linear's residual column). */
STK_API int stk_hessian_launch_info(int64_t n_rows, int32_t d, int64_t out[5]);

/* ---- pointwise log-predictive sweep (regression families, 1 <= d <= 128): for every ROW, statistics
 * over S draws -- the reduction the log-density hooks do not form (they reduce over rows for each draw) ----
 * A draw is an unconstrained point q_s[D] in the layout of stk_log_density_grad: (alpha, beta[1..d]) for
 * logistic and poisson, with u = log sigma appended for linear.  With eta_is = alpha_s + x_i . beta_s the
 * pointwise log likelihood is the NORMALISED one (nothing dropped; no prior and no Jacobian enter):
 *   logistic  z = (2 y_i - 1) eta, ll = min(z, 0) - log1p(exp(-|z|)),              g = 1 / (1 + exp(-eta))
 *   poisson   ll = y_i eta - exp(eta) - lgamma(y_i + 1),                           g = exp(eta)
 *   linear    r = y_i - eta, ll = -log(2 pi)/2 - u_s - r^2 e^{-2 u_s} / 2,         g = eta
 * Per row i, over the S draws (S >= 1):
 *   lppd_i = logsumexp_s(ll_is) - log S          mean_i = (1/S) sum_s ll_is
 *   var_i  = the sample variance of ll_is with denominator S - 1, and 0 at S = 1
 *   mu_i   = (1/S) sum_s g_is                    elpd_i = lppd_i - var_i
 * Per shard, eight doubles of totals: [0] n, [1] sum lppd_i, [2] sum var_i (p_waic), [3] sum elpd_i,
 * [4] sum elpd_i^2, [5] the number of rows with var_i > 0.4 (the usual WAIC reliability flag), [6] the
 * number of rows where any of the four statistics is non-finite, [7] 0.  The totals are plain sums: a
 * non-finite row makes its sums non-finite, and slot 6 says how many there were.
 * Non-finite values propagate as IEEE arithmetic on the definitions gives them, never as a finite wrong
 * number: a NaN eta makes the row's statistics NaN; a poisson exp(eta) that overflows gives ll = -inf for
 * that draw, which adds 0 to the lppd sum (every draw -inf: lppd_i = -inf, not NaN), and mean_i is then
 * -inf and var_i NaN.
 * q [S][D]: the same draws for every shard.  shard == -1: every shard in one grouped launch; totals is
 * then [nshards][8] and rows NULL or [sum n_rows][4], shard-major, (lppd, mean, var, mu) per row.  Either
 * output may be NULL, not both.  Row i's statistics depend only on (x_i, y_i) and the draws: they carry
 * the same bits whatever the shard's length, its position in the model and the number of shards in the
 * call; the totals are bitwise independent of how many shards share the call and of the device.
 * rows may be host or device memory.  Memory of the context's own device is written in place by the
 * sweep; anything else -- host memory, or memory of ANOTHER device, which a kernel here must not
 * dereference -- is filled through a staging buffer of the context and one copy.
 * STK_E_ARG (the message names the family or the offending d) for 8 schools, d > 128, S < 1, a NULL q
 * and both outputs NULL. */
STK_API int stk_log_predictive(stk_model* m, int shard, const double* q, int32_t S, double* rows, double* totals);
/* host only, like stk_sweep_launch_info: out[0] rows per tile, out[1] chunks per shard, out[2] waves per
 * block, out[3] dynamic LDS bytes, out[4] bytes of the draw image (16-draw tiles of ceil(d / 4) k-steps x
 * 64 lanes plus 64 per-draw scalars), out[5] bytes of chunk-partial workspace per shard. */
STK_API int stk_predictive_launch_info(int64_t n_rows, int32_t d, int32_t S, int64_t out[6]);

/* ---- PSIS-LOO sweep (regression families, 1 <= d <= 128, 1 <= S <= 1024): for every ROW, Pareto-smoothed
 * importance-sampling leave-one-out over S draws, with the Pareto shape khat of the row's importance
 * ratios as its diagnostic ----
 * ll_is is stk_log_predictive's normalised pointwise log likelihood of row i at draw s.  For one row:
 *   1. lr_s = -ll_s, shifted: lr <- lr - max_s lr.
 *   2. Tail length M = ceil(min(0.2 S, 3 sqrt S)).
 *   3. M < 5 (S <= 20): no smoothing, khat = +inf.
 *   4. Else sort lr ascending; the tail is the M largest, t_1 <= ... <= t_M; cut is the (S - M)-th
 *      smallest, the largest value outside the tail; unless t_M - t_1 > 0: no smoothing, khat = +inf.
 *   5. Exceedances x_j = exp(t_j) - exp(cut).
 *   6. The Zhang-Stephens fit of the generalised Pareto distribution with the loo package's prior:
 *      N = M, Mg = 30 + floor(sqrt N), xstar = x[floor(N / 4 + 0.5)] (1-based); for j = 1 .. Mg
 *        theta_j = 1 / x_N + (1 - sqrt(Mg / (j - 0.5))) / 3 / xstar,   k_j = mean_i log1p(-theta_j x_i),
 *        l_j = N (log(-theta_j / k_j) - k_j - 1),   w_j = 1 / sum_i exp(l_i - l_j) (an overflow gives 0);
 *      theta = sum_j theta_j w_j, k = mean_i log1p(-theta x_i), sigma = -k / theta,
 *      khat = (k N + 5) / (N + 10).
 *   7. If khat is finite: t_j <- log(sigma expm1(-khat log1p(-p_j)) / khat + exp(cut)), p_j = (j - 0.5) / M.
 *   8. Truncate: lw = min(lr, 0).            9. Normalise: lw <- lw - logsumexp(lw).
 *  10. elpd_loo_i = logsumexp_s(ll_s + lw_s), ll paired with lw through the sort.
 *  11. lppd_i = logsumexp_s ll_s - log S,   p_loo_i = lppd_i - elpd_loo_i.
 * (r_eff = 1: no relative-efficiency correction of the tail length; no moment matching.)
 * If any ll_is of a row is not finite, the row's elpd_loo, p_loo and khat are NaN; lppd_i stays what IEEE
 * arithmetic gives (a -inf draw adds 0, a NaN draw gives NaN).  Never a finite wrong number.
 * rows: (elpd_loo, khat, lppd, p_loo) per row.  Per shard, eight doubles of totals: [0] n, [1] sum lppd,
 * [2] sum p_loo, [3] sum elpd_loo, [4] sum elpd_loo^2, [5] the number of rows with khat > 0.5, [6] with
 * khat > 0.7 (+inf counts in both, NaN in neither), [7] the number of rows whose elpd_loo, lppd or p_loo is
 * not finite or whose khat is NaN.  The totals are plain sums: a non-finite row makes its sums non-finite.
 * q, shard, rows and totals follow stk_log_predictive's contract, word for word: shard == -1 is one grouped
 * launch, rows may be host or device memory, either output may be NULL but not both, a row's bits depend
 * only on (x_i, y_i) and the draws, the totals not on how many shards share the call nor on the device.
 * S <= 1024: a 16-row tile's log ratios are kept in LDS (16 x 1024 doubles = 128 KB), never in HBM.
 * STK_E_ARG (the message names the family, or the offending value as d = ... / S = ...) for 8 schools,
 * d > 128, S < 1, S > 1024, a NULL q and both outputs NULL. */
STK_API int stk_loo(stk_model* m, int shard, const double* q, int32_t S, double* rows, double* totals);
/* host only: out[0] rows per tile, out[1] chunks per shard, out[2] waves per block, out[3] dynamic LDS
 * bytes (a function of d and S), out[4] bytes of the draw image (stk_predictive_launch_info's), out[5]
 * bytes of chunk-partial workspace per shard. */
STK_API int stk_loo_launch_info(int64_t n_rows, int32_t d, int32_t S, int64_t out[6]);

/* ---- per-draw log density and the Laplace proposal (regression families, d <= 128) ----
 * stk_log_density_draws: lp[s] is, by definition, the lp stk_log_density_grad returns at q[s] -- Stan's
 * log_prob (propto, with the Jacobian of sigma = e^u and the stk_model_set_prior terms) -- for S draws in ONE
 * pass over the shard's rows, forward only (no gradient).  q is [S][D] unconstrained, the layout of
 * stk_log_predictive; any S >= 1; host or device memory for q and lp.  shard == -1 runs every shard in one
 * grouped launch against the same draws and fills lp[nshards][S]; else lp[S].
 * The launch geometry is a function of n (and d) only, never of S, and every sum runs in an order fixed by
 * them: lp of a draw depends on that draw and the shard alone, bit for bit -- the same at any position in
 * q, with any companions, at any S, and in the grouped launch as in a single-shard one.  A non-finite draw
 * (or one whose Poisson mean overflows) has a non-finite lp; the other draws of the call are untouched.
 * The likelihood is the sweeps' propto one (no lgamma(y + 1) for poisson_log, no log(2 pi) / 2 for normal).
 * STK_E_ARG (the message names the family, or the offending value as d = ... / S = ...) for 8 schools,
 * d > 128, S < 1 and a NULL q or lp. */
STK_API int stk_log_density_draws(stk_model* m, int shard, const double* q, int32_t S, double* lp);
/* host only: out[0] rows per tile, out[1] chunks per shard, out[2] waves per block, out[3] dynamic LDS
 * bytes, out[4] bytes of the draw image (stk_predictive_launch_info's), out[5] bytes of chunk-partial
 * workspace per shard.  out[0..3] do not depend on S. */
STK_API int stk_logdens_launch_info(int64_t n_rows, int32_t d, int32_t S, int64_t out[6]);
/* S draws of N(mode, F F^T): q_out[s] = mode + F xi_s, F any D x D row-major matrix (the Python layer passes
 * L^-T of the Cholesky factorisation -H = L L^T of a Laplace fit), xi_{s,j} = the Box-Muller normal of the
 * Philox counter {stream, s, j / 2, TAG_LAPLACE} under `seed` (csrc/philox.h), and log_q_out[s] =
 * -sum_j xi_{s,j}^2 / 2 in index order: the log proposal density without its constant.  stream is the
 * shard's GLOBAL index, so a shard draws the same proposal on any rank and next to any other shards; draw s
 * does not depend on S.  1 <= D <= 130, S >= 1; host or device memory for every pointer.  STK_E_ARG
 * (naming D = ... / S = ...) otherwise. */
STK_API int stk_laplace_draws(stk_ctx* ctx, const double* mode, const double* factor, int32_t D, int32_t S,
                              uint64_t seed, uint32_t stream, double* q_out, double* log_q_out);

/* ---- weighted-likelihood bootstrap sweep (regression families, d <= 128) ----
 * The bootstrap weight of row i (its index in the shard) in replicate b, a pure function of (seed, stream, i,
 * b, kind) (csrc/boot_math.h): the Philox counter {(uint32)(i >> 4), ((uint32)(i >> 36) << 2) | (i & 3),
 * stream << 12 | b, TAG_BOOT} gives four 32-bit words (first output low, high, second output low, high) and the
 * row takes word (i >> 2) & 3.  kind 0 ("poisson"): w = the number of thresholds T_k <= word, T_k = floor(2^32
 * sum_{j <= k} e^-1 / j!), k = 0 .. 12 -- integers 0 .. 13 of mean 1.  kind 1 ("exponential"): w = -log((word +
 * 1/2) 2^-32), mean 1, at most 22.9.  b < 4096; stream < 2^20 is the shard's GLOBAL index, so a shard draws the
 * same weights on any rank and next to any other shards.
 *
 * stk_log_density_grad_boot: q is [R][D] (unconstrained, the layout of stk_log_density_grad) and holds
 * replicates rep0 .. rep0 + R - 1; rep0 is a multiple of 16 and rep0 + R <= 4096.  For every replicate
 *   lp_b = sum_i w_ib ll_i(q_b) + prior(q_b) + Jacobian,   grad_b = its gradient [D],   wsum_b = sum_i w_ib
 * with ll_i, the prior and the Jacobian exactly those of stk_log_density_grad (propto, the stk_model_set_prior
 * terms unweighted, + u for linear, whose - n u becomes - wsum_b u).  The replicates run as tiles of 16, one
 * pass over the shard's rows per tile.  shard == -1 runs every shard at the same q in grouped launches and
 * fills lp[nshards][R], grad[nshards][R][D], wsum[nshards][R]; else lp[R], grad[R][D], wsum[R].  streams holds
 * one value per shard of the call; NULL: the local shard index.  grad and wsum may be NULL; host or device
 * memory for q, lp, grad, wsum (streams: host).
 * A replicate's three outputs depend on (the shard's rows, seed, stream, b, q_b) alone, bit for bit: not on its
 * companions in the call, on R, on how many shards share the launch or on the device.  A non-finite q_b gives a
 * non-finite lp_b and touches no other replicate.
 * STK_E_ARG (the message names the family or the offending value) for 8 schools, d > 128, a kind other than
 * 0 / 1, R < 1, a rep0 that is no multiple of 16, rep0 + R > 4096, a stream >= 2^20 and a shard whose chunks of
 * rows exceed 2^31 bytes (split the shard). */
STK_API int stk_log_density_grad_boot(stk_model* m, int shard, const double* q, int32_t R, int32_t rep0, uint64_t seed,
                                      const int32_t* streams, int32_t kind, double* lp, double* grad, double* wsum);
/* host only, no context: out[r - row0][b - rep0] = the weight of row r in replicate b for nrows rows from row0
 * and R replicates from rep0 (any rep0 here; rep0 + R <= 4096) -- compiled from the header the kernel uses. */
STK_API int stk_boot_weights_host(uint64_t seed, uint32_t stream, int64_t row0, int64_t nrows, int32_t rep0, int32_t R,
                                  int32_t kind, double* out);
/* host only: the 13 thresholds T_k of kind 0. */
STK_API int stk_boot_poisson_thresholds(uint32_t out[13]);
/* host only: out[0] rows per sub-tile, out[1] chunks per shard (a function of n_rows alone), out[2] waves per
 * block, out[3] dynamic LDS bytes, out[4] bytes of chunk-partial workspace per shard and tile of 16 replicates. */
STK_API int stk_boot_launch_info(int64_t n_rows, int32_t d, int64_t out[5]);

/* ---- posterior predictive replicates and checks (regression families, d <= 128) ----
 * The replicate y_rep of (row i, draw s) is a pure function of (seed, stream, i, s, eta_is, u_s) (csrc/yrep_math.h).
 * Philox call j of the element has the counter {(uint32) i, (uint32)(i >> 32) | s << 8, stream << 12 | j, TAG_YREP}:
 * i < 2^40 is the row's index in its shard, s < 2^24 the draw's GLOBAL index (draw0 + its position in q), stream <
 * 2^20 the shard's GLOBAL index, j < 4096; U and V are the 53-bit uniforms of its two 64-bit outputs.  One call per
 * element, never shared between rows.
 *   logistic  g = 1 / (1 + e^-eta);  y_rep = 1 if U < g else 0                                          (call 0)
 *   linear    z = sqrt(-2 log U) cos(2 pi V);  y_rep = eta + e^u z                                      (call 0)
 *   poisson   mu = e^eta.  mu < 10: inversion of U by upward search (k = 0, p = e^-mu, c = p; while U > c: k += 1,
 *             p *= mu / k, c += p), stopped at k = 128.  10 <= mu < 2^30: Hormann's transformed rejection (PTRS,
 *             numpy's constants), attempt j on call j, floor(mu + 1/2) after 64 rejected attempts.  2^30 <= mu < inf:
 *             max(0, floor(mu + sqrt(mu) z + 1/2)), the normal approximation (distribution function within 2.1e-6).
 *   A non-finite eta or e^u, or mu = +inf, gives y_rep = NaN.
 *
 * stk_posterior_predict: q is [S][D] unconstrained, the layout of stk_log_predictive, and holds draws draw0 ..
 * draw0 + S - 1; X is read once for all of them.  Outputs, with (m, V) = (g, g (1 - g)) logistic, (mu, mu) poisson,
 * (eta, e^{2u}) linear and D(z, theta_s) = sum_i (z_i - m_is)^2 / V_is (a term with V = 0 is 0 where z = m and +inf
 * otherwise, the limit of a point mass):
 *   stats[s][0..7]  sum_i y_rep, sum_i y_rep^2, max_i y_rep, min_i y_rep, #{i : y_rep = 0}, D(y_rep_s, theta_s),
 *                   D(y, theta_s), the number of NaN replicates of the draw (which makes [0..3] and [5] NaN)
 *   obs[0..7]       the same [0..4] of the observed y, [5] = n, the rest 0                           (may be NULL)
 *   rows[i][0..3]   #{s : y_rep_is < y_i}, #{s : y_rep_is = y_i}, sum_s y_rep, sum_s y_rep^2         (may be NULL)
 *                   a NaN replicate counts in neither and makes the sums NaN
 *   yrep[i][s]      the replicates, [n_rows][S]                                                      (may be NULL)
 * shard == -1 is one grouped launch of every shard against the same draws: stats[nshards][S][8], obs[nshards][8],
 * rows[sum n][4] and yrep[sum n][S] shard-major.  streams holds one value per shard of the call (host memory);
 * NULL: the local shard index.  Host or device memory for q and every output, as stk_log_predictive has it: rows
 * and yrep are written in place when they are memory of the context's device.
 * An element's y_rep, a row's four numbers and a draw's eight depend on (the shard's rows, seed, stream, the
 * draw's global index, the draw) alone, bit for bit: not on how many shards share the launch, on the shard's
 * position, on the device, on S or on the draw's position in q or its companions -- a call on q[a .. b) with draw0
 * = a returns columns a .. b - 1 of the call on all of q.
 * STK_E_ARG (the message names the family, or the offending value as d = ... / S = ...) for 8 schools, d > 128,
 * S < 1, draw0 < 0 or draw0 + S > 2^24, a stream >= 2^20 and a NULL q or stats. */
STK_API int stk_posterior_predict(stk_model* m, int shard, const double* q, int32_t S, int32_t draw0, uint64_t seed,
                                  const int32_t* streams, double* stats, double* obs, double* rows, double* yrep);
/* host only, no context: out[r][c] = y_rep of row row0 + r at draw draw0 + c for the caller's eta[nrows][S] (and
 * u[S] = log sigma, linear) -- compiled from the header the kernel uses.  family: 2 linear, 3 logistic, 4 poisson.
 * margin, unless NULL, receives per element the smallest relative gap of any comparison that decided the value
 * (+inf where none did): |a - b| / max(|a|, |b|) for a < b, the distance of a floor's argument to the nearest integer
 * over max(1, mu), |lhs - rhs| over the largest term for the PTRS acceptance test.  An element below 1e-10 may come
 * out differently from an eta that differs in its last bits. */
STK_API int stk_yrep_host(int32_t family, uint64_t seed, uint32_t stream, int64_t row0, int64_t nrows, int32_t draw0,
                          int32_t S, const double* eta, const double* u, double* out, double* margin);
/* host only: out[0] rows per tile, out[1] chunks per shard, out[2] waves per block, out[3] dynamic LDS bytes,
 * out[4] bytes of the draw image (stk_predictive_launch_info's), out[5] bytes of chunk-partial workspace per
 * shard.  out[0..3] do not depend on S. */
STK_API int stk_ppc_launch_info(int64_t n_rows, int32_t d, int32_t S, int64_t out[6]);

/* ---- sampling: stark/stark.py:43-56 for every shard of the model ---- */
STK_API int stk_sampler_create(stk_model* m, const stk_config* cfg, stk_sampler** out);
/* Advance every chain until it has completed `target_iter` transitions (warmup counted),
 * or finished.  max_steps bounds the state-machine steps of this call (0 = no bound). */
STK_API int stk_sampler_run(stk_sampler* s, int32_t target_iter, int64_t max_steps);
STK_API int stk_sampler_info(stk_sampler* s, stk_run_info* info);
/* Draws of one shard: out[P][chains * num_samples] (chain-major columns), stats
 * [chains * num_samples][6] = accept_stat, stepsize, treedepth, n_leapfrog, divergent, energy.
 * Either pointer may be NULL. */
STK_API int stk_sampler_draws(stk_sampler* s, int shard, double* out, double* stats);
/* Unconstrained draws of one shard: out[chains][num_samples][D], or
 * out[chains][num_warmup + num_samples][D] when cfg.save_warmup is set. */
STK_API int stk_sampler_draws_unconstrained(stk_sampler* s, int shard, double* out);
/* Every chain's nominal step size (nshards * chains) and diagonal inverse metric
 * ([nshards * chains][Dmax]; all ones under unit_e).  Either pointer may be NULL. */
STK_API int stk_sampler_adaptation(stk_sampler* s, double* stepsize, double* inv_metric);
/* The same for a dense_e sampler: inv_metric is [nshards * chains][D][D] row-major, every matrix
 * symmetric to the bit.  STK_E_ARG for another metric. */
STK_API int stk_sampler_adaptation_dense(stk_sampler* s, double* stepsize, double* inv_metric);
/* A dense_e sampler's Cholesky factors, M^-1 = L L^T: chol is [nshards * chains][D][D] row-major, every
 * L lower triangular (the upper triangle is zero).  Read-only: the factor the momenta are drawn with.
 * STK_E_ARG for another metric. */
STK_API int stk_sampler_metric_factor_dense(stk_sampler* s, double* chol);
/* Transitions completed so far by every chain (nshards * chains, shard-major). */
STK_API int stk_sampler_iterations(stk_sampler* s, int32_t* iters);
STK_API int stk_sampler_destroy(stk_sampler* s);

/* ---- checkpoint / resume of a run between stk_sampler_run calls.  The state is every chain's
 * device state (position, momentum, gradient, tree stack, adaptation windows and dual-averaging
 * scalars, Philox counters, mode and iteration), the draws and stats so far and the pending
 * evaluation requests, plus the step counters: a run saved after any stk_sampler_run call and
 * loaded into a sampler created from the same model geometry and config -- in another process,
 * on another device -- continues bit for bit as the unsplit run would (the reference has no
 * counterpart: a pystan fit cannot be resumed; SURVEY.md 8 aux "checkpoint/resume").
 * stk_sampler_state_bytes gives the size of the blob; stk_sampler_load_state refuses a blob
 * of another geometry / config (STK_E_ARG) before writing anything.  The blob (version 2) is also
 * bound to the data: after its header it carries the fingerprint of every shard
 * (stk_model_fingerprint, computed on the device the first time a state is saved or loaded and
 * cached in the model), and a model of the same geometry built from other rows -- another
 * data_seed, another file, another rank's slice, one flipped bit -- is refused with STK_E_ARG
 * "the state was saved against other data (shard s)", again before anything is written.  A
 * version-1 blob (no fingerprints) is refused with a message that names its version.  A dense_e
 * sampler's state also carries every chain's M^-1, its Cholesky factor and the window's Welford
 * M2, and the config check includes the metric: a diag_e blob is refused by a dense_e sampler and
 * the reverse.  Full-data mode is part of the config check too: a blob saved by a sampler with an
 * all-reduce callback and a plain sampler refuse each other.  A full-data resume is, in this order,
 * stk_sampler_create -> stk_sampler_set_allreduce -> stk_sampler_load_state: set_allreduce needs a
 * sampler that has not run (and moves the [grad | lp] block, which load_state then fills). */
STK_API int stk_sampler_state_bytes(stk_sampler* s, int64_t* bytes);
STK_API int stk_sampler_save_state(stk_sampler* s, void* buf, int64_t bytes);
STK_API int stk_sampler_load_state(stk_sampler* s, const void* buf, int64_t bytes);

/* ---- full-data mode (BASELINE configs[4]): ONE posterior whose rows are split over ranks.
 * Every rank builds a one-shard model of its rows and a sampler with the same config and the
 * same shard_ids (so the chains' RNG streams agree); after each step's local sweep + reduce,
 * `fn` must replace the [nchains][Dp] gradient block followed by the [nchains] log densities
 * (count = nchains * (Dp + 1) doubles, stk_sampler_grad_block) by their sum over ranks, ordered
 * on `stream` (the context's stream), and return 0.  Every rank then runs the NUTS step on
 * identical inputs, so chain states stay identical without any other exchange.  dev_block:
 * NULL (the library's block), or caller-allocated device memory of `count` doubles used in
 * its place -- e.g. a torch tensor that torch.distributed.all_reduce sums over RCCL.  Logistic
 * family with flat priors only (its log density is a pure sum over rows; the Poisson family's is
 * too, but it is refused here by name: full-data mode is logistic-only); call before the first run.
 * No reference counterpart (SURVEY.md 8e "full-data extension"). */
typedef int (*stk_allreduce_fn)(void* user, double* block, int64_t count, void* stream);
STK_API int stk_sampler_grad_block(stk_sampler* s, int64_t* count);
STK_API int stk_sampler_set_allreduce(stk_sampler* s, stk_allreduce_fn fn, void* user, double* dev_block);
STK_API int stk_sample(stk_model* m, const stk_config* cfg, double* draws, double* stats, stk_run_info* info);

/* One fixed-step-size NUTS transition per chain from q (C x D, updated in place), no
 * adaptation, RNG iteration index `iteration`: the unit of the GPU/CPU twin check. */
STK_API int stk_transition(stk_model* m, int shard, double* q, int32_t C, uint64_t seed, int32_t iteration,
                           double eps, const double* inv_metric, int32_t max_depth, double* lp, double* stats);

/* stk_transition under a dense metric: inv_metric is D x D row-major, symmetric positive definite
 * (STK_E_ARG otherwise); momenta are p = L^-T u with M^-1 = L L^T and u the normals stk_transition
 * draws for the same (seed, chain, iteration).  Regression families. */
STK_API int stk_transition_dense(stk_model* m, int shard, double* q, int32_t C, uint64_t seed, int32_t iteration,
                                 double eps, const double* inv_metric, int32_t max_depth, double* lp, double* stats);

/* ---- consensus combine: stark/stark.py:7-21, 66-70 ---- */
/* draws: nshards x P x S, out: P x S (host or device memory; device buffers are read and
 * written in place, host buffers staged through the context).  shard_used[s] = 0 for shards
 * left out because of NaN draws.  Singular matrices (STK_E_LINALG, numpy's LinAlgError):
 *   - stk_consensus / _blocked / _products invert each sample covariance and sum W, which are
 *     symmetric positive (semi)definite by construction, by diagonal-pivot block Gauss-Jordan on
 *     the unit-diagonal matrix and report a pivot <= P eps or NaN as singular.  S <= p draws
 *     (p = P, or the largest row_block block) give a rank-deficient covariance (rank <= S - 1)
 *     and raise before any arithmetic; np.linalg.inv's LU usually returns a huge finite
 *     "inverse" built from rounding noise there, and raises only on an exactly zero pivot (a
 *     constant row: both raise) -- DESIGN.md section 9.  An exactly duplicated parameter row
 *     with S >> P draws is singular too: its unit-diagonal pivot is within 4.4e-16 of zero,
 *     below P eps, so it raises; numpy raises or returns ~1e34 entries depending on the
 *     rounding (tests/test_gpu_kernels.py::test_combine_duplicated_parameter_row_is_singular);
 *   - stk_consensus_solve takes the caller's sum W as ANY square matrix (symmetric or not) and
 *     inverts it as np.linalg.inv does, by partial pivoting, singular only on an exactly zero
 *     pivot. */
STK_API int stk_consensus_products(stk_ctx* ctx, const double* draws, int32_t nshards, int32_t P, int32_t S,
                                   double* sum_w, double* sum_wtheta, int32_t* shard_used);
STK_API int stk_consensus_solve(stk_ctx* ctx, const double* sum_w, const double* sum_wtheta, int32_t P,
                                int32_t S, double* out);
STK_API int stk_consensus(stk_ctx* ctx, const double* draws, int32_t nshards, int32_t P, int32_t S, double* out,
                          int32_t* shard_used);
/* stk_consensus with block-diagonal weights: row_block[a] names the weight block of row a
 * (e.g. 0 for the parameters, 1 for lp__); covariances between rows of different blocks are
 * taken as 0, so each block is combined from its own covariance. */
STK_API int stk_consensus_blocked(stk_ctx* ctx, const double* draws, int32_t nshards, int32_t P, int32_t S,
                                  const int32_t* row_block, double* out, int32_t* shard_used);
/* (sum_s W_s)^-1 sum_s W_s theta_s with the CALLER's weights: weights [nshards][P][P], symmetric positive
 * definite (host or device memory); draws / out / shard_used as stk_consensus, any S >= 1.  Shards with
 * NaN draws are left out (weights too).  A non-finite weight of a used shard: STK_E_ARG naming the shard.
 * A singular sum: STK_E_LINALG.  The NaN mask, sum W, sum W theta and the final SPD solve are
 * stk_consensus's stages; the covariance and the per-shard inverse are skipped. */
STK_API int stk_consensus_weighted(stk_ctx* ctx, const double* draws, const double* weights, int32_t nshards,
                                   int32_t P, int32_t S, double* out, int32_t* shard_used);

/* ---- semiparametric density-product combiner (semiparamDPE of "Asymptotically exact, embarrassingly
 * parallel MCMC"), a second combiner next to stk_consensus.  No reference counterpart.
 * With M usable shards of S draws theta^m_s in R^p (p = P, or P - 1 when lp_row: the last row is lp__),
 * mu_m / Sigma_m each shard's sample mean and covariance (stk_consensus_products' stages),
 *   Sigma_M = inv(sum_m inv(Sigma_m)) = L L^T,   mu_M = Sigma_M sum_m inv(Sigma_m) mu_m,
 * every shard density is estimated as
 *   p_m(theta) = N(theta | mu_m, Sigma_m) (1/S) sum_s N(theta | theta^m_s, h^2 M Sigma_M) / N(theta^m_s | mu_m, Sigma_m)
 * (kernel covariance h^2 M Sigma_M instead of the paper's h^2 I: affine invariant).  With
 *   y^m_s = inv(L) (theta^m_s - mu_M) / sqrt(M),  n^m_s = |y^m_s|^2,  g^m_s = (theta^m_s - mu_m)^T inv(Sigma_m) (theta^m_s - mu_m) / 2
 * the product of the p_m is a mixture over index tuples t = (t_1 .. t_M); with s_t, N_t, G_t the sums of
 * y, n, g at the chosen indices,
 *   log W_t(h) = -(N_t - |s_t|^2 / M) / (2 h^2) - |s_t|^2 / (2 M (1 + h^2)) + G_t
 *   component:   y ~ N(s_t / (M (1 + h^2)), h^2 / (M (1 + h^2)) I),   theta = mu_M + sqrt(M) L y.
 * The sampler is independent Metropolis within Gibbs on t, K independent chains: chain k starts from uniform
 * indices; sweep r (counted from 0, burn-in and thinning included) uses h = h[r] and proposes, for m = 0 .. M - 1
 * in order, c uniform on {0 .. S - 1}, accepted iff log u < log W_t' - log W_t; after `burn` sweeps every
 * `thin`-th sweep emits a draw, chain k's j-th being output column j K + k (columns >= T are not produced).
 * h has burn + thin ceil(T / K) entries, every one positive and finite.  The lp__ row of a draw is
 * sum_m lp_w[m] lp^m_{t_m}, lp_w[m] ~ 1 / var(lp^m) (the 1 x 1 block of stk_consensus_blocked).
 * Philox counters and the bit-level contract: csrc/dpe_math.h, DESIGN.md section 3.
 *
 * stk_dpe_launch_info: out = {p, ldp (row stride of the image: p rounded up to 8), coordinates per lane,
 *   draws per chain, LDS bytes per chain, prepare workspace bytes, sample workspace bytes, blocks (= K)}.
 * stk_dpe_prepare: draws [nshards][P][S] (host or device) -> shard_used [nshards] and n_used = M (host), and,
 *   host or device: mu [p], L [p][p] (lower), lp_w [nshards] (first M; lp_row), Y [nshards][S][ldp] (first M
 *   shards; one draw per row, pads zero), nrm / g / lpv [nshards][S] (first M; lpv: lp_row).  Shards with NaN
 *   draws are left out; S <= p is STK_E_LINALG before any arithmetic.  Every sum is in an order fixed by
 *   (M, P, S).
 * stk_dpe_sample: prepared arrays of M shards (host or device; lp_w and lpv both NULL: no lp__ row) -> out
 *   [p (+ 1)][T] (host or device), accept [M] accepted proposals per shard (host, or NULL), and optionally the
 *   trace: trace_idx [K][sweeps][M] the index of coordinate m after its proposal, trace_logw [K][sweeps]
 *   log W of the state at the end of the sweep.
 * stk_dpe_sample_host: the same on host arrays with no device: the arithmetic of dpe_math.h in the kernel's
 *   order, so indices and accept counts are the kernel's (the normals' sin / cos / log may differ in the last bit).
 * stk_consensus_dpe: prepare + sample in one call; accept [nshards] (first M).
 * STK_E_ARG, naming the value: T < 1, K < 1, thin < 1, burn < 0, a bandwidth <= 0 or not finite, p > 1024
 * (16 coordinates per lane), more than 4096 shards, stream >= 2^24. */
STK_API int stk_dpe_launch_info(int32_t nshards, int32_t P, int32_t S, int32_t T, int32_t K, int32_t lp_row,
                                int64_t out[8]);
STK_API int stk_dpe_prepare(stk_ctx* ctx, const double* draws, int32_t nshards, int32_t P, int32_t S, int32_t lp_row,
                            int32_t* shard_used, int32_t* n_used, double* mu, double* L, double* lp_w, double* Y,
                            double* nrm, double* g, double* lpv);
STK_API int stk_dpe_sample(stk_ctx* ctx, int32_t M, int32_t p, int32_t S, const double* mu, const double* L,
                           const double* lp_w, const double* Y, const double* nrm, const double* g, const double* lpv,
                           uint64_t seed, uint32_t stream, int32_t T, int32_t K, int32_t burn, int32_t thin,
                           const double* h, double* out, int64_t* accept, int32_t* trace_idx, double* trace_logw);
STK_API int stk_dpe_sample_host(int32_t M, int32_t p, int32_t S, const double* mu, const double* L, const double* lp_w,
                                const double* Y, const double* nrm, const double* g, const double* lpv, uint64_t seed,
                                uint32_t stream, int32_t T, int32_t K, int32_t burn, int32_t thin, const double* h,
                                double* out, int64_t* accept, int32_t* trace_idx, double* trace_logw);
STK_API int stk_consensus_dpe(stk_ctx* ctx, const double* draws, int32_t nshards, int32_t P, int32_t S, int32_t lp_row,
                              uint64_t seed, uint32_t stream, int32_t T, int32_t K, int32_t burn, int32_t thin,
                              const double* h, double* out, int32_t* shard_used, int64_t* accept);

#ifdef __cplusplus
}
#endif
#endif /* STARK_HIP_H */
