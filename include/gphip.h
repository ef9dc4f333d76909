/* gphip.h -- plain C ABI of the MI355X-native Gaussian-process likelihood / prediction path.
 *
 * Drop-in boundary for the GP hot path of ssmit1986/BayesianInference.  Every
 * entry point replaces a Wolfram-Language call site of the reference
 * (BayesianInference/Kernel/BayesianGaussianProcess.wl, cited as BGP:line):
 *
 *   gphip_create        data capture of defineGaussianProcess              BGP:228-238
 *   gphip_loglik        the "LogLikelihoodFunction" closure theta -> R     BGP:295-306 (+181-199)
 *   gphip_loglik_batch  the same closure mapped over a theta matrix        BS:276-298, BS:902-916
 *   gphip_fit           matrixInverseAndDet[covarianceFunction[theta]]     BGP:308 (invCovFun)
 *   gphip_cross_covariance  compiledKandKappa[points1, kernel, nugget][X*]     BGP:63-124
 *   gphip_predict       predictFromGaussianProcessInternal                 BGP:396-422
 *   gphip_predict_samples  predictFromGaussianProcess over all samples     BGP:343-376
 *   gphip_predict_cov / _draws / _logpdf  the joint N(mu, Sigma) of the test points (no reference counterpart)
 *   gphip_loo / gphip_loo_grad  leave-one-out cross-validation of the training set (no reference counterpart)
 *   gphip_*_pw          the same with point-dependent nugget[x] / mean[x]  BGP:37, 113, 171, 300, 408
 *   gphip_covariance    "CovarianceFunction" = compiledCovarianceMatrix    BGP:45-61
 *   gphip_solve         "InverseCovarianceFunction"[theta]["Inverse"][b]   BGP:130-141
 *   gphip_logdet        "InverseCovarianceFunction"[theta]["LogDet"]       BGP:126-128,139
 *
 * Conventions: every function returns an int status (0 = GPHIP_OK).  "K is not positive
 * definite / hopelessly ill-conditioned" is NOT an error status: it is reported through *info
 * (the WL shim / Python host then substitutes $MachineLogZero exactly like Catch["MatInv"],
 * BGP:298-304).  theta and results are fp64 at the ABI.  Host buffers stay owned by the caller;
 * X and y are copied to the device once and stay resident.  One in-flight call per handle
 * (internally serialised); different handles may be used concurrently.
 */
#ifndef GPHIP_H
#define GPHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gphip_ctx* gphip_handle;

/* status codes */
#define GPHIP_OK 0
#define GPHIP_ERR_ARG 1        /* bad argument value / unknown id            (LIBRARY_TYPE_ERROR)      */
#define GPHIP_ERR_DIM 2        /* shape mismatch (p, N, d, M)                (LIBRARY_DIMENSION_ERROR) */
#define GPHIP_ERR_HIP 3        /* HIP runtime failure, see gphip_last_error  (LIBRARY_FUNCTION_ERROR)  */
#define GPHIP_ERR_STATE 4      /* predict/solve/logdet before a successful gphip_fit                    */
#define GPHIP_ERR_NODEVICE 5   /* no gfx950 device visible                                              */
#define GPHIP_ERR_UNSUPPORTED 6

/* *info values */
#define GPHIP_INFO_OK 0
#define GPHIP_INFO_NOT_SPD 1   /* pivot <= tol: singular or ill-conditioned K (LinearSolve::sing1/luc) */
#define GPHIP_INFO_NAN 2       /* non-finite theta or result                                           */

/* kernel_id: named covariance functions (exact forms in SURVEY.md §8d / DESIGN.md).
 * theta layout: (l_1..l_nl, sigma_f, sigma_n [, mu]);  nl = 1 (isotropic) or d (ARD). */
#define GPHIP_KERNEL_SE 0            /* sf^2 exp(-|p-q|^2 / (2 l^2))                                  */
#define GPHIP_KERNEL_SE_ARD 1        /* sf^2 exp(-1/2 sum ((p_j-q_j)/l_j)^2)                          */
#define GPHIP_KERNEL_MATERN52 2      /* sf^2 (1+sqrt5 s+5 s^2/3) exp(-sqrt5 s), s=|p-q|/l             */
#define GPHIP_KERNEL_MATERN52_ARD 3  /* same with s = sqrt(sum ((p_j-q_j)/l_j)^2)                     */
#define GPHIP_KERNEL_NULL 4          /* Function[0]: K = diag(sn^2) (BGP:25-27,156-159); theta=(sn[,mu]) */
#define GPHIP_KERNEL_MATERN32 5      /* sf^2 (1 + sqrt3 s) exp(-sqrt3 s), s = |p-q|/l                  */
#define GPHIP_KERNEL_MATERN32_ARD 6
#define GPHIP_KERNEL_RQ 7            /* rational quadratic sf^2 (1 + r2/(2 alpha))^-alpha, r2 = |p-q|^2/l^2; theta = (l, alpha, sf, ..) */
#define GPHIP_KERNEL_RQ_ARD 8        /* same with r2 = sum ((p_j-q_j)/l_j)^2;                  theta = (l_1..l_d, alpha, sf, ..)  */
/* The reference takes ANY kernel[p, q] (BGP:32); its own worked example is a constant plus a squared exponential,
 * `#2 + Exp[-(pt1 - pt2)^2/#1^2]` (BGP:16).  Composed forms of the named kernels cover that family:
 *     k = [c +] k1   |   [c +] k1 + k2   |   [c +] k1 * k2
 * each term with its own length scales / alpha / sf.  theta layout:
 *     [term 1: l.., (alpha), sf] [term 2: l.., (alpha), sf] [c] sn [mu]
 * (c = the constant offset, present when offset = 1).  Anything else stays on the reference's own path (the WL package
 * falls back to the reference's defineGaussianProcess).  */
#define GPHIP_OP_NONE 0
#define GPHIP_OP_SUM 1
#define GPHIP_OP_PRODUCT 2
#define GPHIP_KERNEL_COMPOSE(term1, op, term2, offset) \
    ((term1) | ((term2) << 8) | ((op) << 16) | ((offset) << 20) | (1 << 24))
/* ANY other covariance function: source text compiled at run time (hiprtc) into the library's own kernel build.
 * `body` = the statements of
 *     template <typename T> T k(X, Y, P, D) { <body> }
 * where X(k) / Y(k) are coordinate k (0-based) of the two points, P(k) the function's k-th hyper-parameter, D the input
 * dimension and T the handle's arithmetic type (double / float); it must `return` the covariance WITHOUT the nugget.  Device
 * math (exp, sqrt, pow, fabs, sin, ..) and the names Mathematica's CForm emits (Power, Sqrt, Exp, Log, Abs, Sin, Cos, Tan, ArcTan, Sinh, Cosh, Tanh, Erf, Erfc, Min, Max, Pi, E)
 * are available.  Example, SE-ARD:  "T s = 0; for (int k = 0; k < D; ++k) { T u = (X(k) - Y(k)) / P(k); s += u * u; }
 * return P(D) * P(D) * exp((T)-0.5 * s);"  with nparams = d + 1.
 * theta layout of such a handle:  [p_0 .. p_{nparams-1}] sn [mu].  The function may be non-stationary: the prior variance
 * k(x, x) is evaluated per point on the device (prediction variance, pivot tolerance of the factorisation).
 * Likelihoods, batches, fits, predictions, posterior-sample mixtures, covariance exports and the native sampler work as for the
 * named kernels.  gphip_loglik_grad costs ONE factorisation, like the named kernels: the body is instantiated a second time
 * with T = a forward-mode dual number (csrc/gp_dual.h: + - * / comparisons, exp log log1p expm1 sqrt pow fabs sin cos tan
 * sinh cosh tanh atan erf erfc fmin fmax and the CForm names) inside the reduction 1/2 tr((alpha alpha^T - K^-1) dK/dp_m);
 * intermediates that depend on a P(k) must therefore be of type T (not double / float).  A body that does not compile
 * that way, more than 64 hyper-parameters, or option "custom_grad" = 0 fall back to central differences of the likelihood
 * (2 p + 1 points in one batched evaluation; step eps^(1/3) max(|theta_k|, 1e-2) in the handle's arithmetic: ~1e-6 relative
 * in fp64, ~1e-2 in fp32).  Option "grad_analytic" reads 1 after a call that took the one-factorisation route.  Replaces the reference's
 * `kernel @@ points[[{i,j}]]` for an arbitrary pure function (BGP:29-33, cross form BGP:100-109).
 * Errors: GPHIP_ERR_ARG = the body does not compile (gphip_create_error() returns the compiler's log),
 * GPHIP_ERR_UNSUPPORTED = no hiprtc (see csrc/rtc_dyn.h; $GPHIP_HIPRTC_PATH names the library explicitly). */
#define GPHIP_KERNEL_CUSTOM 100
int gphip_create_custom(const void* X, const void* y, int64_t N, int64_t d, const char* body, int nparams, int mean_id,
                        int dtype, int device /* < 0: current */, gphip_handle* out);
/* the same with a device list (several ordinals = ONE multi-device handle, see gphip_create) / as one rank of a multi-process
 * job (see gphip_create_rank): every local context compiles the function for itself */
int gphip_create_custom_devices(const void* X, const void* y, int64_t N, int64_t d, const char* body, int nparams, int mean_id,
                                int dtype, const int* devices, int ndev, gphip_handle* out);
int gphip_create_custom_rank(const void* X, const void* y, int64_t N, int64_t d, const char* body, int nparams, int mean_id,
                             int dtype, int device, int rank, int world, const void* id128, gphip_handle* out);
const char* gphip_create_error(void);
/* gphip_custom_compile_d: compile `body` exactly as gphip_create_custom of a d-dimensional problem would (the program is
 * specialised on the input dimension for 1 <= d <= 32; d = 0 or d > 32: the dimension-generic program) -- no handle, no device
 * needed (hiprtc cross-compiles for `arch`, null = "gfx950").  Validates user input early; proves that a deployed libgphip.so finds hiprtc and carries its own kernel text (the
 * text of csrc/gp_kernels.h is embedded in the library at build time; $GPHIP_SRC_DIR overrides it for development); and warms
 * the per-process code-object cache (key: body, dtype, arch, d) that later gphip_create_custom* calls OF THE SAME d hit.  *cache_hit = 1 when
 * the code object was already there.  grad_nparams < 0: the value program (kernel build + prior variance kernels);
 * 1 .. 64: the GRADIENT program instead -- the same text instantiated with forward-mode dual numbers in its grad_nparams
 * hyper-parameters (csrc/gp_dual.h), what the first gphip_loglik_grad of such a handle compiles.
 * Errors as gphip_create_custom (gphip_create_error() = the compiler's log). */
int gphip_custom_compile_d(const char* body, int dtype, const char* arch, int grad_nparams, int d, int* cache_hit);
/* the same with d = 0: validates the function and warms the cache of handles with d > 32 only */
int gphip_custom_compile(const char* body, int dtype, const char* arch, int grad_nparams, int* cache_hit);

/* ---- host logic shared by the two hosts (pure C++, no device; csrc/gphip_hostlogic.inc) ------------------------------------
 * gphip_kernel_parse: the kernel-name grammar (spaces, underscores, case ignored)
 *     term [(+|*) term] [+ const]    term: se, se_ard, matern52, matern52_ard, matern32, matern32_ard, rq, rq_ard;   null | none
 * -> spec[8] = {kernel_id for gphip_create, term 1, op, term 2 (-1 none), offset, parameters of term 1, of term 2, 0-based
 * position of sigma_n in theta}.  GPHIP_ERR_ARG: not a kernel of the library.
 * gphip_cform_to_body: the text Mathematica's CForm prints for a covariance function whose coordinates / hyper-parameters
 * were replaced by the stand-in symbols ..gphipXc<k> / ..gphipYc<k> / ..gphipPc<k>  ->  "return <C expression in X(k), Y(k),
 * P(k)>;", the body gphip_create_custom takes (BGP:29-33: any pure function of two points).
 * gphip_tab_prior_sample: `pool` draws from a separable prior given as log-density tables (p x m, uniform nodes over
 * box[2j] .. box[2j+1]; <= -1e299 = log 0): the starting pool of the sampler (generateStartingPoints, BS:1046-1068). */
int gphip_kernel_parse(const char* name, int64_t d, int* spec);
int gphip_cform_to_body(const char* cform, char* out, int64_t cap);
int gphip_tab_prior_sample(const double* box, const double* tab, int p, int64_t m, int pool, uint64_t seed, double* out);
#define GPHIP_MEAN_ZERO 0            /* Function[0]  (BGP:168,255)                                    */
#define GPHIP_MEAN_CONST 1           /* Function[mu], mu = last entry of theta                        */

/* X: row-major N x d, y: length N, always fp64 host arrays.  dtype selects the DEVICE arithmetic:
 * 64 = fp64 (v_mfma_f64_16x16x4_f64, the 1e-8 parity path) or 32 = fp32 (v_mfma_f32_16x16x4_f32,
 * BASELINE.json config 5; ~1e-3 relative vs the fp64 oracle).  theta and every result stay fp64.
 * devices/ndev: HIP device ordinals this handle may use.  NULL/0 = the current device; one ordinal = that
 * device; SEVERAL ordinals = a multi-device handle living in this one process (one context per listed
 * device, communicator = RCCL ncclCommInitAll, bound at run time; a repeated ordinal makes several virtual
 * ranks share a GPU -- device copies instead of RCCL -- which is how the sharded schedule is tested on a
 * 1-GPU box).  Every entry point below works unchanged on a multi-device handle:
 *   gphip_loglik / _parts / gphip_fit   N >= option "shard_min_n" (default 16384): ONE factorisation sharded
 *                                       over the devices, 1-D block-cyclic over outer panels, one broadcast of
 *                                       the factored panel per step; smaller N: first device
 *   gphip_loglik_batch, gphip_predict_samples   thetas / posterior samples dealt to the devices, no collective
 *   gphip_predict                       after a sharded fit every device holds the whole factor (each received
 *                                       panel is unpacked on arrival): test points shard, no collective
 *   everything else                     first device
 * The reference-side caller this serves: ONE WL kernel process (nestedSampling, BS:1099-1136). */
int gphip_create(const void* X, const void* y, int64_t N, int64_t d, int kernel_id, int mean_id,
                 int dtype, const int* devices, int ndev, gphip_handle* out);
int gphip_destroy(gphip_handle h);

/* One process PER device (WL sub-kernels of parallelNestedSampling, BS:1349-1357; torchrun ranks): rank 0 calls
 * gphip_comm_unique_id, the host hands the GPHIP_COMM_ID_BYTES bytes to every process by its own means, and each
 * process creates its handle with gphip_create_rank (collective: ncclCommInitRank).  Afterwards gphip_loglik /
 * gphip_fit on these handles are COLLECTIVE calls (every rank, same theta, same order) whenever
 * N >= "shard_min_n"; results are identical on every rank.  GPHIP_ERR_UNSUPPORTED if no RCCL can be bound. */
#define GPHIP_COMM_ID_BYTES 128
int gphip_comm_unique_id(void* id128);
int gphip_create_rank(const void* X, const void* y, int64_t N, int64_t d, int kernel_id, int mean_id, int dtype,
                      int device, int rank, int world, const void* id128, gphip_handle* out);
/* world = ranks of the job (1 for a plain handle), nlocal = ranks in this process, *comm = "none" /
 * "device copies" / "rccl (..)" (string owned by the library); any pointer may be NULL */
int gphip_comm_info(gphip_handle h, int* world, int* nlocal, const char** comm);

/* number of hyper-parameters p expected for this handle */
int gphip_num_params(gphip_handle h, int* p);

/* log p(y | X, theta) = -1/2 (N log 2pi + log det K + r^T K^-1 r).  *out undefined if *info != 0. */
int gphip_loglik(gphip_handle h, const double* theta, int p, double* out, int* info);
/* Theta: row-major B x p; out, info: length B. */
int gphip_loglik_batch(gphip_handle h, const double* Theta, int B, int p, double* out, int* info);
/* loglik plus its parts: parts[0]=log det K, parts[1]=r^T K^-1 r (for parity tests). */
int gphip_loglik_parts(gphip_handle h, const double* theta, int p, double* out, double* parts,
                       int* info);

/* loglik and d loglik / d theta (grad: length p, same order as theta):
 * 1/2 tr((alpha alpha^T - K^-1) dK/dtheta_p).  No reference counterpart (the
 * reference maximises without gradients, LaplaceApproximation.wl:177-238).  grad = NaN if *info != 0. */
int gphip_loglik_grad(gphip_handle h, const double* theta, int p, double* out, double* grad, int* info);
/* gphip_loglik_grad_batch: value and gradient for the B rows of the row-major B x p array Theta in one call.  Theta: row-major
 * B x p; out, info: length B; grad: row-major B x p (layout of gphip_loglik_grad per row).  Row s has the semantics of
 * gphip_loglik_grad(h, Theta + s p, p, out + s, grad + s p, info + s).  A row that fails -- non-finite theta, a K that does not
 * factor -- sets only its own info[s] (GPHIP_INFO_NAN / GPHIP_INFO_NOT_SPD), its grad row is NaN and out[s] undefined, as in the
 * one-theta call; the other rows of the call are not disturbed.  NULL h / Theta / out / grad / info are GPHIP_ERR_ARG, a wrong p
 * GPHIP_ERR_DIM, B <= 0 returns GPHIP_OK and touches nothing: all decided before any device work.
 * The rows are evaluated in groups, one theta per workspace slot: a group's K are built and factored together, U_s = L_s^-T of
 * all slots comes from one multi-kernel forward pass over the identity (the route of "grad_potri" = 2), alpha_s = U_s z_s,
 * K_s^-1 = U_s U_s^T and the gradient reductions are launches that carry the slot as a grid dimension, and the accumulators of
 * the group come back in one download.  A group holds as many rows as the context gives workspace slots,
 * as keep what is missing of the 2 (Npad + 16) Npad es bytes of scratch per slot within a quarter of the free device memory, and
 * as option "grad_batch_slots" allows (0, the default: no limit of its own).  "last_grad_batch_slots" (read-only) gives the rows
 * in the last group of the last call, "last_grad_batch_route" (read-only) 1 when that route ran.  It reads 0 when the rows went
 * one by one through gphip_loglik_grad instead, with results bit-identical to the caller's own loop: not even two slots fit,
 * "grad_potri" = 0, the handle has more training points than option "grad_batch_max_n" (default 7168, 0 = no limit: beyond it
 * one theta fills the device and the batch measured no faster than the loop), a point-dependent nugget / mean is set, or the
 * handle's run-time compiled covariance function has no
 * gradient program (it does not compile with dual numbers, more than 64 parameters, "custom_grad" = 0: central differences).
 * With a gradient program, custom_grad_kernel is launched once per slot behind the shared chain.  The null kernel is answered
 * by the host; a multi-device handle runs the batch on its first device, as the one-theta gradient does.
 * The call drops any resident fit, as gphip_loglik_batch does: a following gphip_predict is GPHIP_ERR_STATE.  Every row's sums
 * run in a fixed order without atomics: two calls with the same arguments and options return the same bytes, and permuting the
 * rows of Theta permutes out, grad and info bit for bit while the group sizes stay the same.  Against gphip_loglik_grad of the
 * same theta a row differs by rounding (the factorisations of several slots take another schedule). */
int gphip_loglik_grad_batch(gphip_handle h, const double* Theta, int B, int p, double* out, double* grad, int* info);

/* Factor K(theta) and keep L and L^-1 r resident for predict / solve / logdet. */
int gphip_fit(gphip_handle h, const double* theta, int p, int* info);
/* Xs: row-major M x d fp64.  mean[j] = m(x*_j) + k*_j^T K^-1 r ; var[j] = k(x*,x*) + sn^2 -
 * k*_j^T K^-1 k*_j  (variance of a noisy observation, BGP:113,414-417; sd = sqrt(var)). */
int gphip_predict(gphip_handle h, const void* Xs, int64_t M, double* mean, double* var);
/* predictFromGaussianProcess over posterior samples (BGP:343-376): Thetas row-major S x p; mean, var
 * row-major S x M; info[S] (a sample with info != 0 has undefined mean/var).  All samples of a chunk
 * are factored and solved in one batched pass (one workspace slot per sample). */
int gphip_predict_samples(gphip_handle h, const double* Thetas, int S, int p, const void* Xs, int64_t M,
                          double* mean, double* var, int* info);
/* ---- Joint predictive distribution of the current fit (no reference counterpart: the reference stops at the marginals of
 * gphip_predict).  Sigma = k(X*,X*) + [latent ? 0 : diag(sn^2)] - k*^T K^-1 k*, the full M x M covariance:
 *   latent = 0: of noisy observations (diag(cov) == gphip_predict's var, up to the order of summation);
 *   latent = 1: of the latent function f.
 * On the device: V = L^-1 k* (the forward substitution of gphip_predict, all M rows at once), then C -= [V; z^T] V^T on a
 * tile-major M x M workspace (z = L^-1 r: the same launch turns y* - m(X*) into y* - mu), then -- draws / log density -- the
 * library's own Cholesky of Sigma.  Work on the fitted handle like gphip_predict and never invalidate its fit.
 * Supported: every kernel of the library (named, composed, run-time compiled; the null kernel on the host: Sigma =
 * diag(sn^2), or 0 when latent), fp64 and fp32 handles, and a multi-device handle whose first device holds the whole factor
 * (it computes there).  GPHIP_ERR_STATE: no successful fit.  GPHIP_ERR_UNSUPPORTED: a sharded fit with replicate_factor = 0,
 * and a fit made by gphip_fit_pw with a non-NULL array.  GPHIP_ERR_DIM: M < 1 or M > GPHIP_JOINT_MAX_M (every row of V,
 * M x Npad elements, is resident at once).  Xs: row-major M x d fp64. */
#define GPHIP_JOINT_MAX_M 16384
/* mean[M] (= gphip_predict's mean); cov row-major M x M, both triangles, exactly symmetric. */
int gphip_predict_cov(gphip_handle h, const void* Xs, int64_t M, int latent, double* mean, double* cov);
/* S draws from N(mean, Sigma), row-major S x M: out[s] = mean + chol(Sigma + jitter I) z_s.
 * z == NULL: z_s(j) standard normals made on the device by a counter-based generator (Philox4x32-10, Box-Muller) keyed by
 *            (seed, s, j) only -- the first S rows of a call with S' > S are bit-identical to a call with S.
 * z != NULL: the caller's normals, row-major S x M.
 * jitter < 0: the default, 1e-10 (fp64) / 1e-4 (fp32) x (mean of k(x*,x*) over the test points + sn^2) -- above the
 *            factorisation's pivot tolerance of 64 eps; 0 = none.
 * *info = GPHIP_INFO_NOT_SPD if Sigma + jitter I does not factor (out = NaN), GPHIP_INFO_NAN on non-finite results. */
int gphip_predict_draws(gphip_handle h, const void* Xs, int64_t M, int latent, int S, uint64_t seed, const double* z,
                        double jitter, double* out, int* info);
/* log N(ystar | mean, Sigma) with the noisy-observation Sigma (latent = 0): the joint predictive log density of held-out
 * data.  *info as gphip_loglik's (*out undefined if *info != 0). */
int gphip_predict_logpdf(gphip_handle h, const void* Xs, int64_t M, const double* ystar, double* out, int* info);
/* ---- New observations into a resident fit without refactoring it (no reference counterpart): the observe step of a sequential
 * design loop (fit, maximise an acquisition with gphip_predict_grad, observe, repeat).  After the joint log density of the new
 * points everything the factor of the N + M points consists of is resident:
 *     L' = [ L    0   ]     z' = [ z ; z_new ]     log det K' = log det K + log det Sigma
 *          [ V^T  L_S ]     V = L^-1 k(X, X_new),  L_S = chol(Sigma),  Sigma = k(X_new, X_new) + sn^2 I - V^T V,
 *                           z_new = L_S^-1 (y_new - mu)
 * so conditioning on M more points costs the forward substitution of M rows, an M x M downdate, its factorisation and one
 * streaming pass over the factor: O(N^2 M) instead of the N^3 / 3 of a new handle and gphip_fit.
 *
 * A NEW handle on the N + M points [X; X_new], [y; y_new] whose fit at the parent's fitted theta is resident, made from the
 * parent's factor without refactoring it.  *logp = log p(y_new | X_new, X, y, theta) -- the same bytes
 * gphip_predict_logpdf(h, X_new, M, y_new, ..) returns -- so loglik(extended) = loglik(parent) + *logp.
 * The parent is untouched (its fit stays; gphip_predict returns the same bytes before and after).
 * The new handle is an ordinary single-device handle of the parent's kernel (named, composed or run-time compiled), mean and
 * dtype on the device that holds the parent's whole factor, with default options plus GPHIP_OPTIONS like a fresh handle; the
 * caller destroys it with gphip_destroy, before or after the parent.  Every entry point works on it as on a handle created from
 * the concatenated data after gphip_fit(theta), gphip_extend included: extensions chain.  Calls that rebuild K (gphip_loglik,
 * _batch, gphip_fit, gphip_loglik_grad, gphip_loo, gphip_covariance) return the SAME BYTES as on a handle created from the
 * concatenated host arrays: every handle keeps the fp64 host copy of the X and y it was created with (N (d + 1) 8 bytes) and
 * the new one is created from those.  Calls that use the carried-over factor (gphip_predict*, gphip_solve, gphip_logdet,
 * gphip_predict_cov / _draws / _logpdf, gphip_predict_grad) agree with a fresh fit to rounding: the operation order differs.
 * Two calls with the same arguments give handles whose every result is the same bytes.
 * *info as gphip_predict_logpdf's: GPHIP_INFO_NOT_SPD when Sigma (noisy, no jitter added) does not pass the factorisation's own
 * pivot rule, GPHIP_INFO_NAN for a non-finite y_new entry or result; in both cases *out = NULL, *logp = NaN, the status is
 * GPHIP_OK and the parent keeps its fit.
 * Statuses, all decided before any device work: NULL h / X_new / y_new / out / info GPHIP_ERR_ARG; M < 1 or
 * M > GPHIP_JOINT_MAX_M GPHIP_ERR_DIM; no resident fit GPHIP_ERR_STATE; a sharded fit with replicate_factor = 0 and a fit made by
 * gphip_fit_pw with a non-NULL array GPHIP_ERR_UNSUPPORTED.  The null kernel is answered on the host.
 * Read-only options on the PARENT after a call, microseconds: "last_extend_logpdf_us" (V, Sigma, its factorisation),
 * "last_extend_create_us" (the new context and its buffers), "last_extend_assemble_us" (the copy kernel, csrc/gp_extend.h),
 * "last_extend_derive_us" (the 128-block inverses of the new factor).
 * Not offered: the sparse object (its refit is cheap and its update would need the unfactored B), an in-place form with reserved
 * capacity, removing points, another theta, point-dependent fits, a multi-device result. */
int gphip_extend(gphip_handle h, const void* X_new /* row-major M x d fp64 */, const double* y_new /* M */, int64_t M,
                 gphip_handle* out, double* logp /* may be NULL */, int* info);
/* ---- Gradients of the predictive mean and variance in the TEST inputs (no reference counterpart): how the prediction of the
 * current fit changes when x* moves -- what maximising an acquisition function, finding the optimum of the fitted surface and
 * sensitivity analysis need.  With alpha = K^-1 (y - m), k*_i = k(x*, x_i) and w = K^-1 k* (an N-vector per test point):
 *     dmean[t][c] = dmu /dx*_c  =     sum_i alpha_i dk(x*_t, x_i)/dx*_c
 *     dvar [t][c] = dvar/dx*_c  = -2  sum_i w_i     dk(x*_t, x_i)/dx*_c        (dk(x*, x*)/dx* = 0: every family is stationary)
 *     dk(a, b)/da_c = -sf^2 m2dg(r^2) (a_c - b_c) / l_c^2 per term, m2dg = -2 dg/dr^2; sums and products by the product rule.
 * The constant mean and the noise sn^2 contribute nothing, so the gradient of the latent variance is the same: there is no
 * `latent` argument.  Xs: row-major M x d fp64; dmean, dvar: row-major M x d.  mean, var (length M, each may be NULL) are
 * gphip_predict's, to rounding.  dvar == NULL skips the backward substitution and the matrix-weighted sums: the call then costs
 * what gphip_predict costs; dmean is the same bytes either way.
 * On the device, per chunk of test points: V = L^-1 k(X, X*) as gphip_predict, mean / var from it when asked for, then V L^-1 in
 * place by the route of gphip_solve (dvar only), then ONE reduction kernel evaluates every (test point, training point) pair
 * once and accumulates both gradients in fp64 (csrc/gp_xgrad.h); alpha comes once per call from a single-vector backward
 * substitution.  The strips over the training points are added in a fixed order, no atomics: two calls return the same bytes.
 * The call never invalidates the fit (gphip_predict returns the same bytes before and after it) and works after anything that
 * leaves a fit resident (gphip_fit, gphip_loglik_grad, gphip_loo).  fp64 and fp32 handles; the null kernel is answered on the
 * host with zeros; a multi-device handle whose first device holds the whole factor computes there.
 * Options: "predict_grad_split" n (0 = by the strip rule: at least two workgroups per compute unit while there are slabs of 64
 * training points) forces n strips; "last_predict_grad_nsplit" (read-only) the strips the last reduction used;
 * "predict_grad_chunk" n (0 = gphip_predict's chunk rule, halved beyond 2048 rows) = n test points per chunk, rounded up to
 * 128; "last_predict_grad_chunk" (read-only).
 * Statuses, all decided before any device work: NULL h / Xs / dmean GPHIP_ERR_ARG; M < 1 GPHIP_ERR_DIM; no successful fit
 * GPHIP_ERR_STATE; GPHIP_ERR_UNSUPPORTED for a run-time compiled covariance function (it would need its dual-number program
 * seeded in the coordinates, as gphip_sparse_bound_grad_inducing says), for a fit made by gphip_fit_pw with a non-NULL array
 * (dm/dx of a host function is unknown) and for a sharded fit with replicate_factor = 0. */
int gphip_predict_grad(gphip_handle h, const void* Xs, int64_t M, double* mean, double* var, double* dmean, double* dvar);
/* ---- Pathwise posterior function draws (Matheron's rule; Wilson et al. 2020; no reference counterpart): S draws of the LATENT
 * posterior function of the current fit that can be evaluated anywhere, and differentiated, after they have been drawn -- what
 * Thompson sampling, optimum-location sampling and entropy-search estimators walk.  gphip_predict_draws fixes its M test points
 * before the draw, pays N^2 M + M^3 / 3 per call, stops at GPHIP_JOINT_MAX_M and has no gradient.  With K = k(X, X) + sn^2 I and
 * the constant mean m, draw s = 0 .. S - 1 is
 *     f_s(x)  = m + f~_s(x) + k(x, X) v_s,      v_s = K^-1 (y - m - f~_s(X) - eps_s),   eps_s ~ N(0, sn^2 I)
 *     f~_s(x) = sum_j a_j w_sj cos(Omega_j . x + b_j),   w_sj ~ N(0, 1),   b_j ~ U[0, 2 pi)        (random Fourier features)
 * A noisy observation of f_s is the caller's business (add sn z).  Omega is in raw input units (length scales divided in).
 * f~ approximates the PRIOR with error O(1 / sqrt(F)); given (Omega, b), f_s is exactly linear-Gaussian in (w, eps)
 * (DESIGN.md section 8m has the frequency laws and measured errors).  After the one-off O(N^2 S) solve on the resident factor one
 * evaluation costs O(N + Ftot) per point and draw; the draws of one object are coherent across calls.
 *
 * gphip_rff_table: host only, no device: the feature table of a named kernel at theta (p = its length, with or without the
 * constant mean's entry).  omega: Ftot x d row-major; phase, amp: Ftot.  omega == NULL: the size query (*Ftot_out only).
 * Ftot = F (one term, product), 2 F (sum), + 1 with the constant offset (Omega = 0, b = 0, a = sqrt(c)).  Deterministic in
 * (kernel_id, d, theta, F, seed): Philox counters under documented keys (csrc/gphip_hostlogic.inc); the rows of F features are
 * NOT a prefix of those of F' > F.  GPHIP_KERNEL_CUSTOM and GPHIP_KERNEL_NULL: GPHIP_ERR_UNSUPPORTED; a wrong p, F < 1, d < 1:
 * GPHIP_ERR_DIM; an unknown id, a zero length scale, alpha <= 0, a negative offset, a missing array: GPHIP_ERR_ARG.
 *
 * gphip_paths_create works on a resident fit like gphip_predict_cov; it never invalidates the fit and gphip_predict returns the
 * same bytes before and after it.  w_sj = philox_normal(seed, s, j), eps_si = sn philox_normal(seed ^ 0x2E2AC13EF8E8D8D2, s, i)
 * (both evaluated on the device; the key of eps is 10 x 0x9E3779B97F4A7C15 mod 2^64, which no stream of the table uses: those
 * are 1, 2, 5, 6 and 9 times that constant, so eps is independent of (Omega, b)), the table is gphip_rff_table(fitted theta, F, seed) byte for byte.  Prefix property: the first S
 * rows of w and eps and the whole table equal those of a call with S' > S bit for bit; v and the outputs agree to rounding.
 * The object owns device copies of everything that depends on theta or the draw (raw X, 1 / l, the slot scalars, Omega, b, a w,
 * w, eps, v): it stays valid when the parent is fitted again at another theta.  It borrows the parent's device, stream and mutex
 * (one call in flight) and must be destroyed before the parent: gphip_destroy of a parent with live paths objects returns
 * GPHIP_ERR_STATE and destroys nothing.  Statuses, all decided before any device work: NULL h / out / info GPHIP_ERR_ARG; S < 1,
 * F < 1, S > 2048, Ftot S > 2^26 GPHIP_ERR_DIM; no fit GPHIP_ERR_STATE; a run-time compiled covariance function, a fit made by
 * gphip_fit_pw with a non-NULL array and a sharded fit with replicate_factor = 0 GPHIP_ERR_UNSUPPORTED.  *info = GPHIP_INFO_NAN
 * on a non-finite v: *out = NULL, status GPHIP_OK.  The null kernel is answered on the host (f = m, gradients 0, Ftot = 0).  A
 * multi-device handle whose first device holds the whole factor computes there.  fp64 and fp32 handles (the coordinates, phases
 * and kernel values are fp64 in both; weights, matrix products and the solve are the handle's type).
 *
 * gphip_paths_eval: Xs row-major M x d fp64, any M >= 1 (chunks; no GPHIP_JOINT_MAX_M); out S x M; dout S x M x d
 * (dout[s][t][c] = df_s/dx*_tc) or NULL.  out is the same bytes whether dout is asked for or not, and two calls return the same
 * bytes (fixed-order sums, no atomics).  gphip_paths_get: every pointer may be NULL: omega Ftot x d, phase Ftot, w S x Ftot (the
 * unit normals), eps S x N, v S x N.
 * gphip_paths_eval_own: every draw at ITS OWN M points: Xs row-major S x M x d fp64, any M >= 1; out[s][t] = f_s(x_st), S x M;
 * dout[s][t][c] = df_s/dx_c at x_st, S x M x d, or NULL.  f_s is the f_s of gphip_paths_eval (the object's table, draw and v);
 * what Thompson sampling needs when every draw is refined from its own starting points, at 1 / S of the work and the download
 * of gphip_paths_eval on the S M stacked points.  Against gphip_paths_eval at the same points the result agrees to rounding,
 * NOT byte for byte: a thread sums one (draw, point) pair in fp64 in the order of the contraction index, gphip_paths_eval sums
 * through the matrix pipe.  out is the same bytes whether dout is asked for or not, and two calls with the same arguments and
 * options return the same bytes (fixed-order sums, no atomics).  The call chunks over t so that the staged points, partial sums
 * and outputs of a chunk stay within 1 GiB ("paths_chunk" n = n points per draw and chunk, halved while above that budget;
 * "paths_split" n forces n strips as for gphip_paths_eval); read-only "last_paths_own_nsplit" = the strips of the last call's
 * contraction over the training points, "last_paths_own_us" = host microseconds of the last call.  Statuses, all decided before
 * any device work: NULL q GPHIP_ERR_ARG; NULL Xs / out GPHIP_ERR_ARG; M < 1 GPHIP_ERR_DIM.  The null kernel is answered on the
 * host (out = m, dout = 0).  fp64 and fp32 handles: coordinates, phases and kernel values are fp64 in both, the weights are read
 * in the handle's type, and the accumulation is fp64 in both.  It borrows the parent's device, stream and mutex like
 * gphip_paths_eval and never touches the fit or the bytes gphip_paths_eval returns.
 * Options on the PARENT handle: "paths_split" n (0 = by the strip rule) forces n strips of both contractions;
 * "last_paths_nsplit" (read-only) the strips of the last evaluation's contraction over the training points; "paths_chunk" n
 * (0 = up to 16384) = n points per chunk, rounded up to 64; "last_paths_create_us" / "last_paths_feature_us" /
 * "last_paths_subst_us" / "last_paths_eval_us" (read-only): host microseconds of the last create (whole call, its feature pass,
 * its substitutions) and evaluation.
 * The sparse object's draws are made by gphip_sparse_paths_create (below) and evaluated by the calls here.
 * Not offered: run-time compiled covariance functions, point-dependent fits, sharding over devices, conditioning a paths object
 * on new data, device-resident inputs and outputs. */
typedef struct gphip_paths* gphip_paths_handle;
int gphip_rff_table(int kernel_id, int64_t d, const double* theta, int p, int F, uint64_t seed, int64_t* Ftot_out, double* omega,
                    double* phase, double* amp);
int gphip_paths_create(gphip_handle h, int S, int F, uint64_t seed, gphip_paths_handle* out, int* info);
int gphip_paths_eval(gphip_paths_handle q, const void* Xs /* M x d fp64 */, int64_t M, double* out /* S x M */,
                     double* dout /* S x M x d, or NULL */);
/* out[s][t] = f_s(x_{s,t}), dout[s][t][c] = df_s/dx_c at x_{s,t}: every draw at ITS OWN M points. */
int gphip_paths_eval_own(gphip_paths_handle q, const void* Xs /* row-major S x M x d fp64 */, int64_t M,
                         double* out /* S x M */, double* dout /* S x M x d, or NULL */);
int gphip_paths_shape(gphip_paths_handle q, int* S, int64_t* Ftot, int64_t* N, int64_t* d);
int gphip_paths_get(gphip_paths_handle q, double* omega, double* phase, double* w, double* eps, double* v);
int gphip_paths_destroy(gphip_paths_handle q);
/* ---- Pathwise draws over all posterior samples in one object: a MIXTURE paths object is an ordinary
 * gphip_paths_handle whose S draws each belong to one of R hyper-parameter rows, created in ONE call from the R x p array Thetas.
 * S = sum counts; the draws are ordered by row (row 0's counts[0] draws first, then row 1's, ..).  Draw number q of row r is BY
 * DEFINITION draw q of gphip_paths_create(h fitted at Thetas[r], counts[r], F, seeds[r]): the same table gphip_rff_table(theta_r,
 * F, seeds[r]) byte for byte, the same w and eps bytes (Philox keyed by (seeds[r], q, j) and by the eps key of seeds[r]); v and
 * every evaluated value agree with that object to rounding (several slots are factored by another schedule).  The rows with
 * draws are factored together in groups that fit the workspace slots (as gphip_predict_samples; one factorisation per row, never
 * one per draw), both substitutions run for all slots of a group at once.
 * Rows: a row with counts[r] = 0 is not factored, info[r] = 0.  A row that fails (a non-finite theta, a K that does not factor:
 * info[r] as gphip_loglik_batch's, or GPHIP_INFO_NAN for a non-finite v) sets only its own info[r]; its draws evaluate to NaN,
 * values and gradients; the other rows' bytes are those of the call with a valid theta in its place.  *out is NULL (status
 * GPHIP_OK) only when every row with draws failed.
 * Statuses, all decided before any device work: GPHIP_ERR_ARG any NULL pointer; GPHIP_ERR_DIM a wrong p, R < 1, a negative
 * count, S < 1, S > 2048, F < 1, Ftot S > 2^26, R Ftot d > 2^27 (1 GiB of per-row tables), S N >= 2^31; GPHIP_ERR_UNSUPPORTED a
 * run-time compiled covariance function, a point-dependent nugget or mean array set on the handle.  The null kernel is answered
 * on the host (f = m_r, gradients 0).  A multi-device handle computes on its first device.
 * The call drops any resident fit, as gphip_predict_samples does (gphip_predict then returns GPHIP_ERR_STATE).  The object owns
 * all it needs, so later fits do not touch it; it borrows the parent's device, stream and mutex and blocks gphip_destroy of the
 * parent exactly as ordinary paths objects do.
 * On a mixture object gphip_paths_eval (all draws at the same M points), gphip_paths_eval_own (S x M x d points), _shape (Ftot
 * is the same for every row: it depends on the kernel's structure and F only) and _destroy work as on any paths object.  Both
 * evaluations go through ONE kernel (paths_mix_kernel: a thread owns one (draw, point) pair, fp64 sums in the order of the
 * contraction index, strips added in a fixed order, no atomics): out is the same bytes with and without dout, two calls return
 * the same bytes, and gphip_paths_eval(P) returns the bytes of gphip_paths_eval_own on P broadcast to every draw.
 * gphip_paths_get returns w, eps and v; asked for omega or phase it returns GPHIP_ERR_ARG: they are per row.
 * gphip_paths_get_table(q, r, ..): row r's table, omega Ftot x d, phase Ftot, amp Ftot, each may be NULL; r outside [0, R)
 * GPHIP_ERR_DIM.  gphip_paths_rows: R and, when row_of_draw is not NULL, the row of each of the S draws.  Both work on an
 * ordinary (and a sparse-made) object too: R = 1, every draw in row 0.
 * Options on the PARENT handle: "paths_mix_slots" n = at most n rows per group (0 = by the slot rule of gphip_predict_samples);
 * "paths_mix_stage" n = at most n rows of a workgroup staged in LDS (-1 = by the staging rule of gp_paths_mix.h, 0 = every
 * workgroup reads its rows from global memory; the same arithmetic on the same numbers); read-only "last_paths_mix_slots",
 * "last_paths_mix_groups", "last_paths_mix_create_us" (rows per group, groups, host microseconds of the last creation);
 * "paths_split" and "paths_chunk" act as for gphip_paths_eval_own, in both evaluations.
 * Not offered: the sparse object, run-time compiled covariance functions, point-dependent fits, dealing rows to several devices,
 * device-resident inputs and outputs, a device-resident ascent loop. */
int gphip_paths_create_samples(gphip_handle h, const double* Thetas /* row-major R x p */, int R, int p,
                               const int* counts /* R, each >= 0 */, const uint64_t* seeds /* R */, int F,
                               gphip_paths_handle* out, int* info /* R */);
int gphip_paths_rows(gphip_paths_handle q, int* R, int* row_of_draw /* S, or NULL */);
int gphip_paths_get_table(gphip_paths_handle q, int r, double* omega /* Ftot x d */, double* phase, double* amp /* Ftot; each may be NULL */);
/* ---- Leave-one-out cross-validation (Rasmussen & Williams, GPML section 5.4.2; no reference counterpart): how well the model
 * at theta predicts every training point from the other N - 1, from ONE factorisation.  With alpha = K^-1 (y - m) and
 * k_i = [K^-1]_ii:
 *     mean[i] = y_i - alpha_i / k_i        var[i] = 1 / k_i   (variance of a noisy observation: includes sn^2, as gphip_predict's)
 *     logp[i] = 1/2 log k_i - 1/2 alpha_i^2 / k_i - 1/2 log 2 pi  = log p(y_i | X, y_-i, theta)
 *     *out    = L_LOO = sum_i logp[i], the log pseudo-likelihood
 * mean, var, logp: length N, each may be NULL (it is then not downloaded).  *out is summed on the device in a fixed order:
 * partial sum t (t = 0 .. 1023) adds logp[t], logp[t + 1024], .. in that order, then p[t] += p[t + off] for off = 512, 256, .. 1;
 * *out = p[0].  Two calls give the same bytes.
 * On the device: the factorisation of gphip_loglik_grad, U = L^-T (upper triangular), then ONE pass over U gives alpha = U z
 * (z = L^-1 (y - m)) and the squared row norms k_i = sum_{j >= i} U_ij^2 -- K^-1 itself is not formed.  Cost: a factorisation
 * plus N^3 / 3 for U; one N x N scratch buffer.
 * gphip_loo_grad: L_LOO and its gradient (grad: length p, layout and chain rule of gphip_loglik_grad).  With g = alpha / k,
 * beta = K^-1 g, c_i = 1 / k_i + g_i^2 and M = K^-1 diag(c) K^-1:
 *     dL_LOO/dtheta_j = 1/2 sum_ab (alpha_a beta_b + beta_a alpha_b - M_ab) dK_ab/dtheta_j,      dL_LOO/dmu = sum_i beta_i
 * the contraction of gphip_loglik_grad with other weights.  K^-1 = U U^T as there, then M = B B^T with B = K^-1 diag(sqrt c)
 * on the matrix pipe (N^3 flop, written over U): about twice the cost of gphip_loglik_grad; two N x N scratch buffers.
 * Both calls evaluate at theta and leave that fit resident, like gphip_loglik_grad: gphip_predict / gphip_solve /
 * gphip_predict_cov work afterwards without a gphip_fit.  *info as gphip_loglik's; outputs are NaN when *info != 0.
 * Supported: every kernel (the null kernel on the host: mean = m, var = sn^2), fp64 and fp32 handles.  A run-time compiled
 * function whose dual-number gradient program does not compile (see GPHIP_KERNEL_CUSTOM) gets central differences of gphip_loo
 * (2 p + 1 factorisations, the step of gphip_loglik_grad).  A multi-device handle factors on its first device.
 * GPHIP_ERR_UNSUPPORTED: a handle with a point-dependent nugget / mean array set, and scratch buffers that do not fit in a
 * quarter of the free device memory (there is no row-block route).  GPHIP_ERR_ARG: NULL h, theta, out, (grad,) info;
 * GPHIP_ERR_DIM: wrong p -- both before any device work. */
int gphip_loo(gphip_handle h, const double* theta, int p, double* mean, double* var, double* logp, double* out, int* info);
int gphip_loo_grad(gphip_handle h, const double* theta, int p, double* out, double* grad, int* info);
/* ---- Point-dependent nugget and mean functions.  The reference evaluates nugget[points[[i]]] (BGP:37), meanFunction /@
 * inputData (BGP:171, 300), kernel[p, p] + nugget[p] at the test points (BGP:113) and meanFunction /@ inputs (BGP:408) for
 * ANY functions of the point (heteroscedastic noise, any m(x)).  Those functions live on the host (WL / Python); the host
 * evaluates them for the theta(s) of the call and hands the VALUES over:
 *   mean_train, nugget_train   row-major B x N (S x N for the samples form): m_theta_b(x_i), nu_theta_b(x_i) at the training
 *                              points; nugget values are VARIANCES (they take the place of sn^2 on the diagonal)
 *   mean_test,  nugget_test    length M (gphip_predict_pw) / row-major S x M (samples form): the same at the test points
 * A NULL pointer keeps the constant form read from theta (sn^2 resp. mu / 0).  theta keeps its layout; the entries a vector
 * replaces are not used (sn^2 still scales nothing: the pivot tolerance uses sf^2 + max|nugget|).  Arrays are read during
 * the call only.  Gradients (gphip_loglik_grad) are defined for the constant forms only. */
int gphip_loglik_batch_pw(gphip_handle h, const double* Theta, int B, int p, const double* mean_train,
                          const double* nugget_train, double* out, int* info);
int gphip_fit_pw(gphip_handle h, const double* theta, int p, const double* mean_train, const double* nugget_train, int* info);
int gphip_predict_pw(gphip_handle h, const void* Xs, int64_t M, const double* mean_test, const double* nugget_test,
                     double* mean, double* var);
int gphip_predict_samples_pw(gphip_handle h, const double* Thetas, int S, int p, const double* mean_train,
                             const double* nugget_train, const void* Xs, int64_t M, const double* mean_test,
                             const double* nugget_test, double* mean, double* var, int* info);
/* K: row-major N x N fp64 (full, both triangles), for parity tests at small N. */
int gphip_covariance(gphip_handle h, const double* theta, int p, double* K);
/* Listable form (BGP:59): Theta row-major B x p -> K row-major B x N x N. */
int gphip_covariance_batch(gphip_handle h, const double* Theta, int B, int p, double* K);
/* compiledKandKappa (BGP:91-124, null kernel BGP:63-89): k row-major N x M (rows = training points, columns =
 * test points, the layout of BGP:103-107), kappa[M] = k(x*,x*) + nugget.  No fit needed; un-fits the handle. */
int gphip_cross_covariance(gphip_handle h, const double* theta, int p, const void* Xs, int64_t M, double* k,
                           double* kappa);
/* rhs, out: column-major N x nrhs (each right-hand side contiguous); out = K^-1 rhs. */
int gphip_solve(gphip_handle h, const double* rhs, int64_t nrhs, double* out);
int gphip_logdet(gphip_handle h, double* out);

/* ---- Nested sampling over the hyper-parameters, driven natively.  Restates the reference's
 * nestedSamplingInternal (BayesianStatistics.wl:859-1040): same live-point bookkeeping, X values (:790-802), trapezoid
 * weights (:757-771), stop rule (:967-978) and constrained-prior Metropolis move (:707-745) -- but `walkers` chains advance in
 * lock step so that every Metropolis step is ONE batched likelihood call instead of "MonteCarloSteps" sequential ones.
 *   box          p x 2 row-major {min, max} per parameter (paramSpecPattern, BS:19)
 *   prior_kind   per parameter 0 = uniform, 1 = log-uniform over its range (NULL = all uniform); or
 *   logprior     a "LogPriorPDFFunction" callback (BS:256-274) overriding prior_kind; the box still bounds the walk
 *   start        pool x p starting points (generateStartingPoints, BS:1046-1068) or NULL = drawn from the built-in prior
 * Output, in generation order (the pool first, then one sample per iteration), up to `cap` samples: points (cap x p),
 * loglik, logprior_out, accept_rate (NaN for the pool: Missing["InitialSample"]); *n_samples; *log_evidence = the crude
 * estimate logSumExp of the crude posterior weights (BS:1019); *n_evals = likelihood evaluations spent.  The statistical
 * post-processing (evidenceSampling, BS:1158-1291; combineRuns) stays with the host: the WL package hands the samples to
 * the reference's OWN evidenceSampling. */
typedef double (*gphip_logprior_fn)(const double* theta, int p, void* user);
typedef struct {
    int pool;                      /* "SamplePoolSize", default 100 (BS:833-855) */
    int max_iterations;            /* "MaxIterations" 10000 */
    int min_iterations;            /* "MinIterations" 100 */
    int mc_steps;                  /* "MonteCarloSteps" 200 */
    int walkers;                   /* chains advanced in lock step, default 32 (1 = the reference's sequential chain) */
    double termination_fraction;   /* "TerminationFraction" 0.01 */
    double min_accept, max_accept; /* "MinMaxAcceptanceRate" {0, 1} */
    uint64_t seed;
} gphip_ns_options;
int gphip_ns_default_options(gphip_ns_options* opts);
int gphip_nested_sampling(gphip_handle h, const double* box, const int* prior_kind, gphip_logprior_fn logprior, void* user,
                          const gphip_ns_options* opts, const double* start, int64_t cap, double* points, double* loglik,
                          double* logprior_out, double* accept_rate, int64_t* n_samples, double* log_evidence,
                          int64_t* n_evals);
/* calculateWeightsCrude (BS:818-835) for m samples of which `pool` are live: order (sorted by (LogLikelihood, Point)), log X
 * and crude log posterior weights in that order, and their logSumExp (exported for tests and hosts without the reference). */
int gphip_ns_crude_weights(const double* points, const double* loglik, int64_t m, int p, int pool, int64_t* order,
                           double* logx, double* logw, double* log_evidence);

/* Options (tuning knobs; results do not depend on them beyond rounding order):
 *   "panel"        outer panel width in 128-tiles (default 4)
 *   "panel_wide"   0/1 (default 1): single-device schedule uses 2x / 1.5x that width while >= 192 / >= 128 tile columns
 *                  remain (the long trailing update hides the wider panel and is read-modify-written less often)
 *   "profile"      0 off, 1 kernel build + trailing SYRK + whole evaluation + prediction epilogue, 2 every kernel class
 *   "xcd_swizzle"  0/1 XCD-aware tile order of the GEMM launches (default 1)
 *   "supertile"    tile order of the trailing SYRK: 0 column-major list, one contiguous chunk per XCD; 1 whole 8x8 super-tiles
 *                  dealt statically to the XCDs (measured slower: unequal loads); 2 (default) the tile LIST itself in 8x8
 *                  super-tile order, equal contiguous chunks per XCD (16 operand panels per 64 resident tiles instead of 65:
 *                  less cache-to-L2 traffic, SYRK alone 0.849 -> 0.861 of peak); 3 = 2, for batches of thetas too (measured: no
 *                  difference there)
 *   "lookahead"    0/1 factor panel k+1 on a second stream under the trailing update of panel k (default 1)
 *   "latency_gemm" 0/1 4x4-wave GEMM shape for launches of <= 256 tiles of problems up to "latency_max_nt" tile columns
 *   "dataflow"     0/1 single-launch dataflow Cholesky (one workgroup per tile, flags instead of launches)
 *                  for problems of <= "dataflow_max_nt" 128-tiles (default 96, N <= 12288), with 64x64 tiles up to
 *                  "dataflow_fine_nt" 128-tiles (default 96, fp64).  How many thetas of a call share ONE such launch:
 *                  "dataflow_max_slots" -1 (default) = fp64: as many as keep the launch within "dataflow_max_tasks" 64-tile
 *                  tasks (default 34 000, the measured crossover with the multi-kernel batch at every N = 512 .. 12288: 750
 *                  thetas at N = 512, 128 at 1024, 16 at 4096, 4 at 8192), fp32 (128-tiles): 2 / 5 of that many 128-tile tasks; n >= 1 = at most n thetas (and up to 4 n
 *                  of a problem with <= 2 500 tasks in all: the rule before round 6).  Larger problems hand their last
 *                  "dataflow_tail" tile columns (default 64, 0 = off) to the same kernel
 *   "panel_left"   -1 auto / 0 / 1: left-looking in-panel updates (one K = 128 s update per column instead of
 *                  K = 128 updates after every column); auto = for batches of more than 8 thetas ("dataflow_max_slots" if set)
 *                  and for panels of >= 8 tiles (the wide early panels of a large factorisation)
 *   "dataflow_lds_kib" -1 auto (default) / 0 / KiB: LDS request of the 64-tile dataflow kernel; > 80 puts ONE workgroup on a
 *                  CU, which keeps the chain's latency-bound waves off SIMDs busy with another workgroup's MFMAs: auto
 *                  asks for 84 KiB while the launch has <= 2 700 tile tasks (one theta up to N ~ 4 600: -2..-7 %)
 *   "bcast_chunks" 0/1 (default 1): sharded evaluation -- a factored panel is broadcast one tile column at a time, each as soon as
 *                  it is final, instead of as one message after the whole panel (must agree on all ranks: checked)
 *   "fuse_potrf"   0/1 (default 1): calls of <= 8 thetas -- the panel-stream update that completes a diagonal tile also factors
 *                  it (no separate potrf128 launch, which waits 100-250 us for a CU slot under the trailing update): N = 16384 -3 %
 *   "dataflow_occ3" -1 auto (default) / 0 / 1: the 64-tile dataflow kernel in its three-workgroups-per-CU build (166 registers);
 *                  auto = launches of >= 6 000 tile tasks, which are throughput bound (N = 12288: -6.5 %)
 *   "fused_eval"   0/1 (default 1): a pure likelihood call of <= 8 thetas that qualifies for 64-tile dataflow
 *                  runs as ONE kernel launch (K(theta) tiles built inside the kernel, results written to
 *                  pinned host memory by its last task)
 *   "grad_potri"   0/1 gradient: form K^-1 = U U^T in one go when 2 N^2 of scratch fits (default 1), else
 *                  stream it in row blocks through forward + backward substitution
 *                  (1: where the factorisation is ONE dataflow launch -- N <= 12288 in fp64 -- U = L^-T for that contraction
 *                  comes from a second launch of the same kernel whose tasks are the tiles of U, and alpha = U z from one pass
 *                  over U, instead of ~5 dependent launches per tile column; 2: U always from the multi-kernel forward pass)
 *   "predict_df"   (default 2048; 0 = off): gphip_predict after a fit that was ONE dataflow launch runs the forward substitution
 *                  L^-1 k* of up to this many test points (twice that up to N = 8192) as one launch of the same kernel
 *                  (tasks = 64 x 64 tiles of the right-hand-side rows) instead of two launches per tile column; also after a
 *                  look-ahead-schedule fit up to "predict_df_max_nt" tile columns, and for gphip_predict_samples (all posterior
 *                  samples of a pass in ONE such launch, slot = sample, while the launch has <= 12 000 tasks)
 *   "thin_tiles"   0/1 (default 1): the GEMM kernel skips work whose result is known or never read -- all but the first
 *                  of the 128 bordered right-hand-side rows (zero), and the strictly-upper quadrant of diagonal tiles
 *   "max_slots"    cap on concurrently resident batch matrices
 *   "shard_min_n"  multi-device handles: shard ONE factorisation over the devices from this N on (default 16384;
 *                  0 = always, even for a world of one)
 *   "replicate_factor"  multi-device handles, sharded evaluations: 0 (default) every rank keeps ONLY its own outer panels
 *                  (compact storage + three receive buffers: ~1 / world of the workspace per rank); a fit leaves the factor
 *                  distributed and gphip_predict streams its panels through the ranks once more (a COLLECTIVE call for
 *                  rank handles in separate processes); 1: every rank keeps the dense workspace and receives panels in
 *                  place, so that after a fit all ranks hold all of L and prediction needs no further traffic
 *   "share_local_panels"  0/1 (default 1): ranks that share the owner's GPU (virtual ranks of a 1-GPU box, device-copy
 *                  communicator) read a factored panel where the owner keeps it instead of copying it; 0 forces the copies
 *                  through the rotating receive buffers (what distinct GPUs do)
 *   "bcast_two_hop"  -1 by size (default: on from 4 ranks when the loaded RCCL has send / recv / group calls) / 0 / 1: sharded
 *                  evaluation over RCCL with more than two ranks -- every panel message goes out as
 *                  scatter (the owner sends piece r to rank r: grouped ncclSend / ncclRecv) + in-place ncclAllGather instead of one
 *                  ncclBroadcast, so that all links of the xGMI mesh carry 1 / world of the message at once (never measured on
 *                  real multi-GPU hardware; results are bit-identical; must agree on all ranks: checked)
 *   "panel_df"     -1 by size (default) / 0 / 1: one theta, fp64, look-ahead schedule -- every outer panel (the look-ahead update by
 *                  the panel before it + its own factorisation) is ONE 64-tile dataflow launch whose tasks read the finished panel as
 *                  extra slabs; by size = 92 <= Nt <= 120 (N = 11k-15k: -2..-8 %, with an 80-column dataflow tail behind the panels)
 *   "dist_panel_df" -1 (default: 3 from 2 ranks on; where the device has no stream-ordered wait on memory, 2 at world 2, else 0)
 *                  / 0 / 1 / 2 / 3: sharded evaluation, fp64 -- the owner factors its outer panel as ONE 64-tile dataflow launch
 *                  (1), which also applies the look-ahead update, reading the previous panel from the receive buffer (2): the owner's
 *                  chain of kernels 31.8 -> 22.6 ms per N = 32768 evaluation with the chip to itself, but a panel is then final only
 *                  when its launch ends, so "bcast_chunks" cannot overlap its columns with the factorisation any more; (3) = (2)
 *                  with a counter per 128-wide tile column that the launch's tasks bump when they finish a tile of it: the
 *                  communication stream waits on the counter (hipStreamWaitValue32, value = the column's tile count) and sends
 *                  the column while the launch still works on the later ones.  Same arithmetic as 2 (bit-identical results).
 *                  bench.py --gpus N times every form.  Rank-local: need not agree across ranks.  "last_dist_panel_df"
 *                  (read-only): the form the last sharded evaluation used.
 *   "dist_owner_yield" -1 (default: on from 4 ranks) / 0 / 1: sharded evaluation -- on the rank that factors outer panel k + 1 the
 *                  remainder of its trailing update REST(k - 1) and its REST(k) are queued behind the END event of that panel
 *                  launch instead of sharing the GPU with it (only the piece of REST(k - 1) on panel k + 1 itself runs before):
 *                  a CU hands a freed slot to the next workgroup of the launch it is already dispatching whatever the stream
 *                  priorities, so a panel launch that becomes ready under a trailing GEMM of the same GPU otherwise runs at
 *                  that GEMM's pace (scripts/gpu_cu_partition.py: 8-10 ms instead of 1.2).  Results are bit-identical either way.
 *                  Rank-local.
 *   "last_issue_us" (read-only): host microseconds the last sharded evaluation spent issuing its schedule (all members of a
 *                  one-process group together).
 *   "trsv"         0 / 1 (default): gphip_solve of up to 4 right-hand sides (up to 16 from Nt >= 96, in batches of 4) and the
 *                  alpha = K^-1 (y - m) of gphip_loglik_grad run each triangle as ONE persistent launch that streams the factor once
 *                  (csrc/gp_trsv.h: tiles in registers, a band-2 chain of workgroup pairs, sentinel hand-offs); 0 = the
 *                  GEMM-shaped substitution for every count.  fp64 and fp32.
 *   "predict_df_max_nt" (default 256): gphip_predict / gphip_solve after a look-ahead fit (Nt above "dataflow_max_nt") still run
 *                  their forward / backward substitutions as single dataflow launches up to this many 128-tiles.
 *   "kbuild_mfma"  0 / 1 (default) / 2: the kernel-matrix build of the SE / Matern-5/2 kernels with the cross term of the squared
 *                  distances on the matrix pipe (kbuild_mfma_kernel): never / for every theta whose accuracy bound
 *                  B = sum_k (halfrange_k / l_k)^2 <= "kbuild_mfma_bound" (default 512; fp32: / 8) holds AND whose
 *                  conditioning keeps that entry error out of the likelihood: eps max(B, 64) (1 + k(x,x) / min nugget) <=
 *                  10^-"kbuild_mfma_digits" (default 9; fp32: 6 digits up) / always (tests).  Every other theta is built by the
 *                  direct-difference kernel, per theta of a batch.
 *   "custom_grad"  0/1 (default 1): gphip_loglik_grad of a run-time compiled covariance function through forward-mode dual
 *                  numbers (one factorisation); 0 = central differences.  "grad_analytic" (read-only) = 1 after a gradient call
 *                  that took the one-factorisation route.
 *   "grad_batch_slots" n: gphip_loglik_grad_batch evaluates at most n rows per group; 0 (default): its group rule alone.
 *                  "grad_batch_max_n" (default 7168; 0 = no limit): handles with more training points send the rows one by one
 *                  through gphip_loglik_grad.  "last_grad_batch_slots" / "last_grad_batch_route" (read-only): the rows in the
 *                  last group of the last call / 1 when the batched route ran, 0 for the per-row loop.
 *   "debug_fail_alloc" / "debug_fail_hip" n: tests only -- the n-th device allocation of the next slot allocation / the n-th checked
 *                  HIP call of the next collective sequence fails (fault injection of the multi-process tests).  The names exist
 *                  only in a process started with GPHIP_TEST_HOOKS=1 in its environment ("unknown option" otherwise) and are
 *                  never taken from GPHIP_OPTIONS.
 *   "debug_abort_word" 1 / 2 / 3: tests only, gated like the two above -- sets the abort word of the persistent kernels in front
 *                  of the next dataflow Cholesky (1) / dataflow substitution or inverse (2) / single-vector substitution (3)
 *                  launch, as a dependency wait that hit its spin limit would, then resets itself to 0.  The call fails with
 *                  GPHIP_ERR_HIP; where it substitutes with a factor, the fit is dropped.
 *   "panel", "shard_min_n", "replicate_factor", "bcast_chunks", "bcast_two_hop" must have the same value on every rank of a
 *   multi-process job (checked by one small all-reduce at the start of every sharded evaluation: a mismatch fails the call on ALL
 *   ranks). */
int gphip_set_option(gphip_handle h, const char* name, double value);
int gphip_get_option(gphip_handle h, const char* name, double* value);
/* The environment variable GPHIP_OPTIONS="name=value,name=value" presets options for every handle the process
 * creates (for hosts that bind only the evaluation entry points, e.g. the LibraryLink shim). */

/* Per-kernel-class timing, measured with HIP events on the handle's stream while "profile"=1.
 * class: 0 kbuild, 1 potrf, 2 trsm, 3 gemm (in-panel), 4 gemm/syrk (trailing), 5 total eval, 6 prediction epilogue (the
 * reductions of gphip_predict and the gradient reduction of gphip_predict_grad).
 * Returns accumulated milliseconds, launches, algorithmic flops and bytes since the last reset (class 4: flops =
 * m (m+1) nb per launch, SURVEY.md §8d -- not the tile-granular count the MFMA pipe executes). */
#define GPHIP_NCLASS 7
int gphip_get_profile(gphip_handle h, int cls, double* ms, double* launches, double* flops,
                      double* bytes);
int gphip_reset_profile(gphip_handle h);

/* ---- the per-rank compute STEPS of the multi-GPU 1-D block-cyclic Cholesky; no reference
 * equivalent (the reference never shards one factorisation).  A multi-device / per-rank handle (gphip_create
 * with ndev > 1, gphip_create_rank) drives these itself; they stay exported so that a host may run the schedule
 * with its own collective instead -- dist_cholesky.py does (torch.distributed: RCCL on GPUs, gloo in the CPU
 * schedule tests).  Outer panel j ("panel" option tile columns) belongs to rank j % world. ---- */
int gphip_set_streams(gphip_handle h, void* main_stream, void* panel_stream); /* adopt hipStream_t's */
int gphip_dist_num_panels(gphip_handle h, int* nouter);
int gphip_dist_panel_shape(gphip_handle h, int k, int64_t* rows, int64_t* cols);
int gphip_dist_begin(gphip_handle h, const double* theta, int p, int rank, int world);
/* packed_dev: device buffer of rows*cols elements of the handle's dtype (see gphip_dist_panel_shape) */
int gphip_dist_factor_panel(gphip_handle h, int k, void* packed_dev);
int gphip_dist_update(gphip_handle h, int k, const void* packed_dev, int j_first, int j_last,
                      int on_panel_stream);
int gphip_dist_end(gphip_handle h, double* logdet_partial, double* quad, int* info);

/* Device memory (bytes) local rank `member` of the handle holds for factor storage right now: dense workspace slots +
 * compact own-panel storage + receive buffers (diagnostics: a sharded evaluation keeps ~1 / world of the workspace). */
int gphip_factor_bytes(gphip_handle h, int member, double* bytes);
/* The resident factor itself (diagnostics and tests, off every hot path: one download of slot 0 of the workspace, untiled on the
 * host as gphip_covariance does; fp32 handles are widened).  After a successful fit -- gphip_fit[_pw], or a call that leaves the
 * factor of its theta resident: gphip_loglik_grad, gphip_loo[_grad], gphip_extend's new handle --
 *   L    row-major N x N: the Cholesky factor, L L^T = K(theta_fit); the strict upper triangle is written as zeros.
 *   z    N values or NULL: the bordered row (tile row Nt of the workspace, row N_pad) as the factorisation left it,
 *        z = L^-1 (y - mean).
 *   Winv Nt x 128 x 128 values (Nt = ceil(N / 128)) or NULL: the inverses W_b = L_bb^-1 of the 128 x 128 diagonal blocks that the
 *        substitutions multiply by, block b at Winv + b * 128 * 128, COLUMN-major inside the block as the device keeps them
 *        (element (i, j) of W_b at j * 128 + i), the upper triangle zero.  The last block is that of the padded matrix: rows and
 *        columns beyond N carry the identity.  Every route a local fit can take leaves these blocks resident (the 64-tile
 *        launches rebuild them from L), so a non-NULL Winv is answered wherever L is.
 * GPHIP_ERR_STATE: no successful fit is resident; the null kernel (no factor: K is diagonal); a fit whose factor is not whole in
 * this context's dense workspace -- one sharded over a multi-device handle's ranks, whatever replicate_factor says, and anything
 * between gphip_dist_begin and gphip_dist_end.  Takes the handle's mutex, uses the main stream only, leaves the fit valid. */
int gphip_factor_get(gphip_handle h, double* L, double* z, double* Winv);

/* ---- Sparse inducing-point GP: the collapsed variational bound of Titsias (2009), "SGPR"; no reference equivalent.
 * For data sizes the exact path cannot hold: m << N inducing points Z, a lower bound F(theta) <= log p(y | X, theta) that costs
 * O(N m^2), predictions from two m x m factors.  theta has the layout of the same kernel in gphip_create (.., sf, sn [, mu]);
 * r = y - m(X); j = jitter >= 0 is PART OF THE MODEL: K_uu always means k(Z, Z) + j I.
 *
 *     L_u L_u^T = K_uu                         (m x m)
 *     V   = L_u^-1 k(Z, X)                     (m x N, never resident as a whole: streamed in chunks of data points)
 *     B   = sn^2 I + V V^T                     (m x m)           L_B L_B^T = B
 *     c   = L_B^-1 (V r)
 *     F   = -1/2 [ N log 2 pi + (N - m) log sn^2 + log det B + (r^T r - c^T c) / sn^2 ] - (sum_i k(x_i, x_i) - tr(V V^T)) / (2 sn^2)
 *
 * prediction at x* with v1 = L_u^-1 k(Z, x*), v2 = L_B^-1 v1:
 *     mean = m(x*) + v2^T c            var = k(x*, x*) [+ sn^2 unless latent] - |v1|^2 + sn^2 |v2|^2
 * gphip_sparse_predict runs the prediction pass of gphip_sparse_predict_samples (below) on the one slot of
 * the resident fit: per chunk of test points one kernel hands V1 to the context of B and takes |v1|^2 on the way, B's stream waits
 * for an event, not the host, and one download is scattered into mean and var.
 *
 * A separate opaque type: no other entry point of this header takes a sparse object.  Every named and composed kernel and the
 * run-time compiled ones (gphip_sparse_create_custom: arguments as gphip_create_custom), zero and constant mean (a mean and a
 * noise that depend on the point: the _pw calls below), fp64 and fp32;
 * one device.  m > N is allowed.  Statuses, all decided before any device work: NULL arguments GPHIP_ERR_ARG; N < 1, d < 1,
 * m < 1, m > GPHIP_SPARSE_MAX_M, wrong p GPHIP_ERR_DIM; the null kernel GPHIP_ERR_UNSUPPORTED, unknown ids GPHIP_ERR_ARG;
 * gphip_sparse_predict before a successful fit GPHIP_ERR_STATE; non-finite jitter GPHIP_ERR_ARG.  Non-finite theta is
 * *info = GPHIP_INFO_NAN and a failed factorisation of K_uu or of B *info = GPHIP_INFO_NOT_SPD, not error statuses.
 *
 * gphip_sparse_bound: *out = F; parts (NULL or 5 doubles) = {log det B, c^T c, r^T r, tr(V V^T), sum_i k(x_i, x_i)}.  It leaves
 * the fit resident; gphip_sparse_fit is the same work without the scalar.  gphip_sparse_set_inducing replaces Z (any m) and
 * drops the fit.
 * jitter < 0: the default, 1e-10 (fp64) / 1e-4 (fp32) x k(x, x) (run-time compiled kernels: x the mean of k(z, z) over Z);
 * option "last_jitter" returns the absolute value the last call used -- a reference has to use the same one.  The error of F
 * grows with cond(K_uu) ~ k(x, x) / j; fp64 held 1e-8 against the reference in every measured case up to cond(K_uu) = 4.8e12
 * (DESIGN.md section 8c).
 * Two calls with the same options return the same bytes (fixed-order reductions, no atomics).
 *
 * gphip_sparse_bound_grad: the bound and its analytic gradient from one evaluation plus one more pass over the data.  grad has
 * length p, theta's layout (the chain rule of gphip_loglik_grad); *out is the same bytes gphip_sparse_bound returns for the same
 * arguments and options, parts as there (may be NULL), the fit stays resident, *info as there and grad is NaN when *info != 0;
 * grad == NULL is GPHIP_ERR_ARG.  With a = L_B^-T c, w = (r - V^T a) / sn^2 and D = I / sn^2 - B^-1:
 *
 *     G = L_u^-T (D V + a w^T)                                            (m x N, streamed in the same chunks as V)
 *     H = L_u^-T [ I - sn^2 B^-1 / 2 - a a^T / 2 - B / (2 sn^2) ] L_u^-1    (m x m)
 *     dF/dtheta_q = sum_ki G_ki dk(z_k, x_i)/dtheta_q + sum_kl H_kl dk(z_k, z_l)/dtheta_q - sum_i dk(x_i, x_i)/dtheta_q / (2 sn^2)
 *     dF/dsn = 2 sn [ -(N - m + sn^2 tr B^-1) / (2 sn^2) + (r^T r - c^T c - sn^2 a^T a) / (2 sn^4) + (sum_i k(x_i, x_i) - tr V V^T) / (2 sn^4) ]
 *     dF/dmu = sum_i w_i
 *
 * THE JITTER IS HELD FIXED in the derivative: the gradient is that of F(theta; j) at the value the call used ("last_jitter"),
 * also when j came from the default rule, which scales with k(x, x).  L_u^-1 and L_u^-T are applied as substitutions, never as
 * products with an inverse of K_uu.  Two calls with the same options return the same bytes.  A run-time compiled kernel whose
 * dual-number program does not compile, one with more than 64 parameters, and option "custom_grad" = 0 take central differences of
 * the bound instead (2 p + 1 evaluations with gphip_loglik_grad's step, one more when the jitter is the default: it is found
 * first and then held); *out is the unperturbed bound's bytes all the same.  Read-only option "grad_analytic": 1 / 0 = which route
 * the last call took.  (When device memory is so short that the second m x chunk buffer forces a smaller chunk than
 * gphip_sparse_bound would take, the two F differ by rounding.)
 *
 * gphip_sparse_bound_grad_inducing: the bound, its gradient in theta and its gradient in the inducing LOCATIONS from the same pass.
 * gradZ is row-major m x d, in the unscaled coordinates of Z as they were given:
 *
 *     dF/dz_k = sum_i G_ki dk(z_k, x_i)/dz_k + 2 sum_l H_kl dk(z_k, z_l)/dz_k                (a d-vector per inducing point)
 *
 * with G and H as above and, for one term k = sf^2 g(r^2), r^2 = sum_c ((a_c - b_c) / l_c)^2 of a named family,
 * dk(a, b)/da_c = -sf^2 (-2 dg/dr^2) (a_c - b_c) / l_c^2 (finite at r = 0 for every family; the l = k term of the second sum is
 * zero); sums and products of two terms by the product rule, each term with its own length scales.  sum_i k(x_i, x_i), the noise
 * and the jitter do not depend on Z: the jitter is held fixed here as well.  *out is the same bytes gphip_sparse_bound returns;
 * grad, when not NULL, the same bytes gphip_sparse_bound_grad returns (the new reduction only reads the weights G and H);
 * grad == NULL skips the reductions in theta.  gradZ is all NaN when *info != 0; the fit stays resident.  Sums run in a fixed
 * order without atomics: two calls with the same options return the same bytes.  NULL h / theta / out / gradZ / info and a
 * non-finite jitter are GPHIP_ERR_ARG, a wrong p GPHIP_ERR_DIM, and a run-time compiled covariance function is
 * GPHIP_ERR_UNSUPPORTED: it would need its dual-number program seeded in the coordinates, which is not built.
 * gphip_sparse_set_inducing with an unchanged m replaces the points in place (same buffers, options and compiled programs, fit
 * dropped); every later result is the same bytes as that of a fresh object created with the new Z.  A changed m recreates the
 * two contexts.
 *
 * gphip_sparse_bound_batch: the bound for the B rows of the row-major B x p array Theta in one call; row s has the semantics of
 * gphip_sparse_bound(h, Theta + s p, p, jitter, ..): out[s] = F, parts (NULL or B x 5) as there, info[s] as there.  jitter < 0 is
 * the default rule applied PER ROW (it scales with that row's k(x, x); run-time compiled kernels: that row's mean of k(z, z));
 * "last_jitter" reads the last usable row's value.  A row that fails -- non-finite theta, a K_uu or a B that does not factor --
 * sets only its own info[s] and gets out[s] (and its parts) NaN; the other rows of the call are not disturbed.  NULL h / Theta /
 * out / info and a non-finite jitter are GPHIP_ERR_ARG, a wrong p GPHIP_ERR_DIM, B <= 0 returns GPHIP_OK and touches nothing.
 * The rows are evaluated in groups, one theta per workspace slot: a group's K_uu are built and factored together, every chunk of
 * data points is loaded once and crossed, substituted and accumulated for all slots of the group by launches that carry the slot
 * as a grid dimension, and the group's B are factored together.  A group holds as many rows as the two
 * contexts give slots, as keep 2048 data points of V per slot within the ~8 GiB of a chunk, and as option "sparse_batch_slots"
 * allows.  The call drops any resident fit, as gphip_loglik_batch does: a following gphip_sparse_predict is GPHIP_ERR_STATE.
 * Every row's sums run in a fixed order without atomics: two calls with the same arguments and options return the same bytes, and
 * a row's bytes do not depend on its position in Theta while the group sizes stay the same.  Against gphip_sparse_bound of the
 * same theta the result differs by rounding (the factorisations of several slots take another schedule).
 *
 * gphip_sparse_nested_sampling: gphip_nested_sampling (above) on a sparse object -- the same driver, arguments, outputs and seed
 * behaviour, with F(theta; jitter) in the place of the log-likelihood: every Metropolis step is ONE gphip_sparse_bound_batch call
 * of up to `walkers` rows at the given jitter (< 0: the default rule per row).  Errors go to gphip_sparse_last_error.
 *
 * gphip_sparse_predict_cov / _draws / _logpdf: the JOINT predictive distribution of M test points from the resident fit, with the
 * semantics of gphip_predict_cov / _draws / _logpdf (above), point for point.  With V1 = L_u^-1 k(Z, X*) (m x M) and V2 = L_B^-1 V1
 *
 *     mu = m(X*) + V2^T c        Sigma = k(X*, X*) [+ sn^2 I unless latent] - V1^T V1 + sn^2 V2^T V2
 *
 * whose diagonal is gphip_sparse_predict's variance.  The jitter j of the model belongs to K_uu only; it is not added to k(X*, X*).
 * cov is row-major M x M with both triangles, exactly symmetric.  draws: out is S x M; z == NULL uses the device's Philox normals
 * keyed by (seed, s, j), so the first S' draws of a call are those of a call with S = S'; z != NULL is S x M standard normals of the
 * caller; latent selects the draws of f* (1) or of y* (0); jitter (absolute, >= 0) is added to Sigma's diagonal before its
 * factorisation, jitter < 0 is the default 1e-10 (fp64) / 1e-4 (fp32) x (k(x*, x*) + sn^2) (run-time compiled kernels: k(x*, x*) is its
 * mean over the test points) -- a latent Sigma is singular to rounding and needs it.  *info is GPHIP_INFO_NOT_SPD when Sigma (+ jitter)
 * does not factor and GPHIP_INFO_NAN for non-finite results; the outputs are NaN then.  logpdf: the log density of ystar under
 * N(mu, Sigma) with the noisy Sigma; a non-finite ystar entry gives *info = GPHIP_INFO_NAN.
 * Statuses, all decided before any device work: NULL pointers and a non-finite jitter GPHIP_ERR_ARG; M < 1, M > GPHIP_JOINT_MAX_M
 * and S < 1 GPHIP_ERR_DIM; no successful fit (also after gphip_sparse_bound_batch or gphip_sparse_set_inducing) GPHIP_ERR_STATE.
 * The calls never invalidate the fit: gphip_sparse_predict and gphip_sparse_bound return the same bytes before and after them.
 * All M rows of V1 and V2 are resident at once (2 M m elements); Sigma is assembled in a context whose training points are X*
 * (kept while M stays the same, dies with the object) by one launch of the two-segment downdate kernel over the stacked index
 * [V1 | V2]; cov, draws and the log density then run the exact path's code on it.  Two calls with the same
 * options return the same bytes.
 *
 * gphip_sparse_predict_samples: mean and variance at the M test points Xs for the S rows of the row-major S x p array Thetas --
 * one Normal per posterior sample -- in one call; mean and var are row-major S x M.  Row s has the semantics of
 * gphip_sparse_fit(h, Thetas + s p, p, jitter, ..) followed by gphip_sparse_predict(h, Xs, M, latent, ..): mean = m(x*) + v2^T c,
 * var = k(x*, x*) [+ sn^2 unless latent] - |v1|^2 + sn^2 |v2|^2 with v1 = L_u^-1 k(Z, x*), v2 = L_B^-1 v1, all of that row's theta
 * (k(x*, x*) of a run-time compiled kernel is a function of the point AND the row).  bound (NULL or S): bound[s] = F(theta_s; jitter)
 * as gphip_sparse_bound_batch defines it.  jitter < 0 is the default rule applied PER ROW as there; "last_jitter" reads the last
 * usable row's value.  A row that fails -- non-finite theta, an unusable jitter, a K_uu or a B that does not factor -- sets only its
 * own info[s] (GPHIP_INFO_NAN / GPHIP_INFO_NOT_SPD; a failure of K_uu takes precedence) and gets its rows of mean and var and its
 * bound[s] NaN; the other rows of the call are not disturbed.  Statuses, all decided before any device work: NULL h / Thetas / Xs /
 * mean / var / info and a non-finite jitter GPHIP_ERR_ARG; a wrong p, S < 1 and M < 1 GPHIP_ERR_DIM.
 * The rows are evaluated in the groups of gphip_sparse_bound_batch (the same rule, "sparse_batch_slots" included) by the same
 * group evaluator, which here leaves the factors of every slot of u and b in place; the test points then go through in chunks:
 * k(X*, Z) and u's forward substitution for all slots of the group at once, one pass that hands V1 to the context of B and takes
 * |v1|^2 on the way, B's forward substitution and the reductions for all slots at once, one download per chunk (DESIGN.md section
 * 8h).  The call drops any resident fit: a following gphip_sparse_predict is GPHIP_ERR_STATE.  Every sum runs in a fixed order
 * without atomics: two calls with the same arguments and options return the same bytes, and permuting the rows of Thetas permutes
 * the rows of every output bit for bit while the group sizes stay the same.  Against fit + predict of the same theta a row differs
 * by rounding (the factorisations of several slots take another schedule).  One device.
 *
 * gphip_sparse_bound_pw / _bound_batch_pw / _fit_pw / _predict_pw / _predict_samples_pw: the calls above for a noise variance and a
 * mean that are functions of the point (the reference's nugget[x] and meanFunction[x]; the conventions of gphip_loglik_batch_pw).
 * mean_train / nugget_train: fp64 host arrays of the values at the N training points (the batched calls: row-major B x N / S x N,
 * row s for row s of Theta), read during the call only; nugget values are VARIANCES nu_i.  theta keeps its layout; the entries an
 * array replaces are not used.  A NULL array keeps the constant read from theta (sn^2; mu or 0), broadcast.  The jitter rule is
 * unchanged.  With Lambda = diag(nu), r = y - m:
 *     B = I + V Lambda^-1 V^T = L_B L_B^T,   c = L_B^-1 V Lambda^-1 r
 *     F = -1/2 [N log 2 pi + sum_i log nu_i + log det B + r^T Lambda^-1 r - c^T c] - 1/2 sum_i (k(x_i, x_i) - |v_i|^2) / nu_i
 * -- the model above with sn^2 = 1 on data whitened by 1 / nu_i; with nu_i = sn^2 it is that model (B there = sn^2 B here).
 * parts (NULL or 6 doubles; batch: B x 6) = {log det B, c^T c, r^T Lambda^-1 r, tr(V Lambda^-1 V^T), sum_i k(x_i, x_i) / nu_i,
 * sum_i log nu_i} with this B.  With both training arrays NULL the call IS the constant one: out and info are the same bytes, and
 * the six parts are its five converted on the host.  A row whose mean array holds a non-finite value, or whose noise array a value
 * that is non-finite or <= 0, gets info GPHIP_INFO_NAN and NaN outputs like a non-finite theta; it disturbs no other row of a batch.
 * The weights 1 / nu_i enter the accumulation either inside its kernel (a weight per contraction index ahead of the MFMA) or
 * through a scaling pass ahead of it (option "sparse_pw_fused"); every sum runs in
 * a fixed order without atomics: two calls return the same bytes, and permuting rows and arrays of a batch permutes the outputs
 * bit for bit while the group sizes stay the same.
 * gphip_sparse_predict_pw: mean_test / nugget_test (NULL or M values) are m(x*) and nu(x*) at the test points: mean = m(x*) + v2^T c,
 * var = k(x*, x*) [+ nu(x*) unless latent] - |v1|^2 + s |v2|^2, s = 1 after a _pw fit with an array and sn^2 otherwise.  It works
 * after any successful fit; nugget_test is not read when latent = 1.  gphip_sparse_predict after a _pw fit uses theta's sn^2 and mu
 * at the test points, as gphip_predict does after gphip_fit_pw.  gphip_sparse_predict_samples_pw: training arrays S x N, test
 * arrays S x M, any of them NULL.  gphip_sparse_predict_cov / _draws / _logpdf after a fit made with a non-NULL training array
 * return GPHIP_ERR_UNSUPPORTED, as the exact joint calls do.  Statuses before any device work are those of the calls they extend.
 * There is no _pw form of the gradients or of the native sampler: the library cannot differentiate or call a host function of the
 * point.
 *
 * gphip_sparse_predict_grad: the gradients of gphip_sparse_predict's mean and variance in the test inputs, the sparse form of
 * gphip_predict_grad (same arguments, outputs and NULLs; var is that of a noisy observation, whose gradient is the latent one's).
 * With v1 = L_u^-1 k(Z, x*), v2 = L_B^-1 v1 and s = sn^2:
 *     a_mu = L_u^-T L_B^-T c   (an m-vector, once per call)        W = L_u^-T (V1 - s L_B^-T V2)   (m x M)
 *     dmean[t][c] = sum_k (a_mu)_k dk(x*_t, z_k)/dx*_c             dvar[t][c] = -2 sum_k W_kt dk(x*_t, z_k)/dx*_c
 * On the device it is the prediction pass of gphip_sparse_predict with one more step per chunk: B's stream substitutes V2
 * backward and forms V1 - s (that) in place, hands the block to K_uu's stream through an event (not the host), which substitutes
 * backward with L_u -- every diagonal solve refined once, as the substitutions of gphip_sparse_bound_grad_inducing are, because
 * the difference cancels as cond(K_uu) grows (option "sparse_pgrad_refine" = 0: unrefined, for measurement) -- and runs the
 * reduction kernel of gphip_predict_grad with the scaled Z as its contraction points.  a_mu comes from two single-vector
 * backward substitutions.  dvar == NULL skips everything but a_mu and the mean-weighted sums.  Fixed summation order, no
 * atomics: two calls return the same bytes; the fit stays (gphip_sparse_predict and gphip_sparse_bound return the same bytes
 * before and after).  Options "predict_grad_split" / "predict_grad_chunk" and their read-only results are gphip_predict_grad's
 * (they are handed on to the context of K_uu).  Statuses, before any device work: NULL h / Xs / dmean GPHIP_ERR_ARG; M < 1
 * GPHIP_ERR_DIM; no successful fit (also after gphip_sparse_bound_batch or gphip_sparse_set_inducing) GPHIP_ERR_STATE; a run-time
 * compiled covariance function and a fit made with a non-NULL training array GPHIP_ERR_UNSUPPORTED.
 *
 * Options (gphip_sparse_set_option / gphip_sparse_get_option):
 *   "sparse_chunk"  data points per pass over V (rounded up to 128); 0 (default) = as many as keep the chunk of V within ~8 GiB,
 *                   at least 2048, halved while it does not fit.  "last_sparse_chunk" (read-only): what the last call used.
 *   "sparse_split"  strips the accumulation kernel cuts a chunk into; 0 (default) = by the split rule (output tiles x strips
 *                   >= two per CU; gphip_sparse_bound_batch: output tiles x slots x strips).  "last_sparse_nsplit" (read-only):
 *                   strips of the last chunk of the last call (of its last group).
 *   "sparse_batch_slots"  most rows gphip_sparse_bound_batch / gphip_sparse_predict_samples evaluate together in one group; 0
 *                   (default) = by the group rule above.  "last_sparse_slots" (read-only): rows in the last group of the last call.
 *   "sparse_samples_chunk"  test points per chunk of the prediction pass, which gphip_sparse_predict[_pw] (the one slot of the
 *                   resident fit) and gphip_sparse_predict_samples[_pw] (the slots of a group) both run; 0 (default) = by the
 *                   caller's rule.  predict_samples: at most 2048, the group's slots x points x m_pad elements within ~8 GiB in
 *                   both contexts, halved while the buffers do not fit.  predict: at most 32768, points x m_pad elements within
 *                   ~8 GiB, at least 2048, halved while they do not fit.  n = n points rounded up to 128, within the same caps.
 *                   "last_sparse_samples_chunk" (read-only): what the last of these calls used.
 *   "sparse_samples_handover"  for both calls.  1 (default): V1 reaches the context of B through sparse_handover_kernel (one
 *                   read, one write, the norms on the way); 0: through a device-to-device copy and a separate norm launch, the
 *                   form it replaced (kept for measurement, scripts/gpu_sparse_samples_time.py).  The two return the same bytes.
 *                   Either way B's stream waits for an event of K_uu's stream, not the host.
 *   "sparse_pw_fused"  how the _pw calls apply the weights 1 / nu_i.  1: inside the accumulation kernel, a weight per contraction
 *                   index ahead of the MFMA; 0 (default): a plain kernel scales the chunk of V and the residual row by
 *                   sqrt(1 / nu_i) in place and the unweighted accumulation follows.  The fused form is the faster one at four of the
 *                   five measured sizes and the slower one at (N, m) = (262144, 2048), which decides the default (DESIGN.md section
 *                   8i, scripts/gpu_sparse_pw_time.py); the two agree to rounding.
 *   "sparse_pgrad_refine"  gphip_sparse_predict_grad's backward substitution with L_u.  1 (default): every diagonal 128-block solve
 *                   refined once (the form gphip_sparse_bound_grad_inducing uses); 0: the bare product with the block inverses, kept
 *                   for measurement (equal errors on the pinned one-tile case, 17 - 26 % of the call).
 *   "profile"       0 / 1: time the phases of gphip_sparse_bound / _fit with HIP events; read-only milliseconds of the last call:
 *                   "ms_kuu_factor", "ms_cross", "ms_forward", "ms_accumulate", "ms_b_factor"; of gphip_sparse_bound_grad also
 *                   "ms_grad_small" (the m x m work and the vector w), "ms_grad_weights" (sparse_weight_kernel alone),
 *                   "ms_grad_backward", "ms_grad_reduce" (its second pass over the data adds to "ms_cross" and "ms_forward").
 *                   of gphip_sparse_bound_grad_inducing also "ms_grad_inducing" (the column-wise reductions for dF/dZ).
 *                   of the joint prediction calls "ms_joint_v" (V1 and V2), "ms_joint_build" (K(X*, X*)), "ms_joint_downdate" (the
 *                   two-segment downdate and its strip reduction) and "ms_joint_factor" (Sigma's factorisation; draws / logpdf).
 *                   of gphip_sparse_predict[_pw] and gphip_sparse_predict_samples[_pw] (there next to the bound's five)
 *                   "ms_samples_v1" (k(X*, Z) and u's substitution), "ms_samples_handover" (V1 to b and |v1|^2), "ms_samples_v2"
 *                   (b's substitution) and "ms_samples_reduce" (the dots and norms of v2 and the finishing kernel), summed over
 *                   groups and chunks; each of these calls resets the four, no other call touches them.
 *                   of gphip_sparse_predict_grad next to those four "ms_pgrad_backward" (the backward substitutions with L_B and
 *                   L_u and the kernel between them) and "ms_pgrad_reduce" (the reduction kernel and its finish).
 *   "sparse_joint_split"  strips the joint prediction's downdate cuts the stacked index of 2 m_pad columns into; 0 (default) = by
 *                   gphip_predict_cov's split rule (output tiles x strips >= 2 per CU, strips of whole 128-columns; a strip may
 *                   span the V1 / V2 boundary), n = n strips.  "last_sparse_joint_nsplit" (read-only): strips of the last call.
 *   every other name is handed on to the two contexts that factor K_uu and B (see gphip_set_option; e.g. "dataflow"). ---- */
#define GPHIP_SPARSE_MAX_M 16384
typedef struct gphip_sparse_ctx* gphip_sparse_handle;
int gphip_sparse_create(const void* X, const void* y, int64_t N, int64_t d, const void* Z, int64_t m, int kernel_id, int mean_id,
                        int dtype, int device, gphip_sparse_handle* out);
int gphip_sparse_create_custom(const void* X, const void* y, int64_t N, int64_t d, const void* Z, int64_t m, const char* body,
                               int nparams, int mean_id, int dtype, int device, gphip_sparse_handle* out);
int gphip_sparse_destroy(gphip_sparse_handle h);
int gphip_sparse_set_inducing(gphip_sparse_handle h, const void* Z, int64_t m);
int gphip_sparse_num_params(gphip_sparse_handle h, int* p);
int gphip_sparse_bound(gphip_sparse_handle h, const double* theta, int p, double jitter, double* out, double* parts, int* info);
int gphip_sparse_bound_batch(gphip_sparse_handle h, const double* Theta, int B, int p, double jitter, double* out /* B */,
                             double* parts /* NULL or B x 5 */, int* info /* B */);
int gphip_sparse_nested_sampling(gphip_sparse_handle h, double jitter, const double* box, const int* prior_kind,
                                 gphip_logprior_fn logprior, void* user, const gphip_ns_options* opts, const double* start, int64_t cap,
                                 double* points, double* loglik, double* logprior_out, double* accept_rate, int64_t* n_samples,
                                 double* log_evidence, int64_t* n_evals);
int gphip_sparse_bound_grad(gphip_sparse_handle h, const double* theta, int p, double jitter, double* out, double* grad, double* parts,
                            int* info);
int gphip_sparse_bound_grad_inducing(gphip_sparse_handle h, const double* theta, int p, double jitter, double* out,
                                     double* grad /* p, may be NULL */, double* gradZ /* row-major m x d */, double* parts, int* info);
int gphip_sparse_fit(gphip_sparse_handle h, const double* theta, int p, double jitter, int* info);
int gphip_sparse_predict(gphip_sparse_handle h, const void* Xs, int64_t M, int latent, double* mean, double* var);
int gphip_sparse_predict_grad(gphip_sparse_handle h, const void* Xs, int64_t M, double* mean /* M or NULL */, double* var /* M or NULL */,
                              double* dmean /* row-major M x d */, double* dvar /* row-major M x d or NULL */);
int gphip_sparse_predict_samples(gphip_sparse_handle h, const double* Thetas, int S, int p, double jitter, const void* Xs, int64_t M,
                                 int latent, double* mean /* S x M */, double* var /* S x M */, double* bound /* NULL or S */,
                                 int* info /* S */);
int gphip_sparse_bound_pw(gphip_sparse_handle h, const double* theta, int p, double jitter, const double* mean_train /* N or NULL */,
                          const double* nugget_train /* N or NULL */, double* out, double* parts /* NULL or 6 */, int* info);
int gphip_sparse_bound_batch_pw(gphip_sparse_handle h, const double* Theta, int B, int p, double jitter,
                                const double* mean_train /* B x N or NULL */, const double* nugget_train /* B x N or NULL */,
                                double* out /* B */, double* parts /* NULL or B x 6 */, int* info /* B */);
int gphip_sparse_fit_pw(gphip_sparse_handle h, const double* theta, int p, double jitter, const double* mean_train,
                        const double* nugget_train, int* info);
int gphip_sparse_predict_pw(gphip_sparse_handle h, const void* Xs, int64_t M, int latent, const double* mean_test /* M or NULL */,
                            const double* nugget_test /* M or NULL */, double* mean, double* var);
int gphip_sparse_predict_samples_pw(gphip_sparse_handle h, const double* Thetas, int S, int p, double jitter,
                                    const double* mean_train /* S x N or NULL */, const double* nugget_train /* S x N or NULL */,
                                    const void* Xs, int64_t M, int latent, const double* mean_test /* S x M or NULL */,
                                    const double* nugget_test /* S x M or NULL */, double* mean /* S x M */, double* var /* S x M */,
                                    double* bound /* NULL or S */, int* info /* S */);
int gphip_sparse_predict_cov(gphip_sparse_handle h, const void* Xs, int64_t M, int latent, double* mean /* M */, double* cov /* M x M */);
int gphip_sparse_predict_draws(gphip_sparse_handle h, const void* Xs, int64_t M, int latent, int S, uint64_t seed,
                               const double* z /* NULL or S x M */, double jitter, double* out /* S x M */, int* info);
int gphip_sparse_predict_logpdf(gphip_sparse_handle h, const void* Xs, int64_t M, const double* ystar, double* out, int* info);
int gphip_sparse_set_option(gphip_sparse_handle h, const char* name, double value);
int gphip_sparse_get_option(gphip_sparse_handle h, const char* name, double* value);
const char* gphip_sparse_last_error(gphip_sparse_handle h);   /* owned by the library */

/* ---- Pathwise posterior function draws of the sparse object: gphip_paths_create's draws for a resident
 * gphip_sparse_fit / gphip_sparse_bound, so that Thompson sampling runs at the N the sparse object is for.  With
 * K_uu = k(Z, Z) + j I = L_u L_u^T, B = sn^2 I + V V^T = L_B L_B^T and c = L_B^-1 V r as above, the collapsed bound's optimal q(u)
 * has, for u' = L_u^-1 u, the mean L_B^-T c and the covariance sn^2 L_B^-T L_B^-1, and draw s = 0 .. S - 1 of the latent function is
 *     f_s(x)  = m + f~_s(x) + k(x, Z) v_s
 *     v_s     = L_u^-T [ L_B^-T (c + sn xi_s) - L_u^-1 (f~_s(Z) + sqrt(j) zeta_s) ],     xi_s, zeta_s ~ N(0, I_m)
 * with f~ the random-Fourier-feature prior of gphip_paths_create.  sqrt(j) zeta is part of the model: K_uu holds the jitter, so
 * the prior value that is conditioned on has covariance K_uu; without it the covariance is off by j |K_uu^-1 k(Z, x)|^2.  With an
 * exact prior in the place of f~ the draws have the mean of gphip_sparse_predict and the latent covariance of
 * gphip_sparse_predict_cov.  Neither N nor V appears: creation costs O(m^2 S + m Ftot S), an evaluation O(m + Ftot) per point and
 * draw.
 * The result is an ordinary gphip_paths_handle: gphip_paths_eval, _eval_own, _shape (N reads m), _get and _destroy serve it with
 * the kernels of the exact object.  Its contraction points are Z; in gphip_paths_get eps (S x m) is sqrt(j) zeta and v (S x m) is
 * v.  gphip_sparse_paths_get returns the unit normals xi and zeta (S x m each, either may be NULL); on a handle that
 * gphip_paths_create made it returns GPHIP_ERR_ARG.  Streams: the table is gphip_rff_table(fitted theta, F, seed) byte for byte,
 * w_sj = philox_normal(seed, s, j), xi_si = philox_normal(seed ^ 11 x 0x9E3779B97F4A7C15, s, i), zeta_si = philox_normal(seed ^
 * 12 x 0x9E3779B97F4A7C15, s, i) (tags 10 and 11 of csrc/gphip_hostlogic.inc; products mod 2^64); the prefix property in S holds
 * as for gphip_paths_create.  Fixed summation order, no atomics: two calls return the same bytes.  The fit is only read:
 * gphip_sparse_predict and gphip_sparse_bound return the same bytes before and after.
 * The object owns copies of everything that depends on theta, Z or the draw, so it survives a refit at another theta and a
 * gphip_sparse_set_inducing with the same m.  It borrows the device and stream of the context of K_uu; every call on it takes the
 * sparse object's mutex first.  While such objects live, gphip_sparse_destroy and a gphip_sparse_set_inducing that changes m
 * return GPHIP_ERR_STATE and destroy nothing.  Errors of calls on it are readable through gphip_sparse_last_error.
 * Statuses, all decided before any device work: NULL h / out / info GPHIP_ERR_ARG; S < 1, F < 1, S > 2048, Ftot S > 2^26
 * GPHIP_ERR_DIM; no resident fit (also after gphip_sparse_bound_batch, gphip_sparse_predict_samples, gphip_sparse_set_inducing)
 * GPHIP_ERR_STATE; a run-time compiled covariance function and a fit made by a _pw call with a non-NULL array
 * GPHIP_ERR_UNSUPPORTED.  *info = GPHIP_INFO_NAN on a non-finite v: *out = NULL, status GPHIP_OK.  fp64 and fp32 objects, typed as
 * gphip_paths_create's are; every named and composed kernel.  Options "paths_split", "paths_chunk" and the read-only
 * "last_paths_*" names go through gphip_sparse_set_option / gphip_sparse_get_option to the context of K_uu.
 * Not offered: run-time compiled covariance functions, point-dependent fits, draws over all posterior samples in one call,
 * device-resident inputs and outputs. */
int gphip_sparse_paths_create(gphip_sparse_handle h, int S, int F, uint64_t seed, gphip_paths_handle* out, int* info);
int gphip_sparse_paths_get(gphip_paths_handle q, double* xi /* S x m or NULL */, double* zeta /* S x m or NULL */);

/* Block until all work queued on the handle's stream is complete. */
int gphip_sync(gphip_handle h);

const char* gphip_last_error(gphip_handle h);   /* owned by the library */
const char* gphip_version(void);
int gphip_device_count(int* n);

#ifdef __cplusplus
}
#endif
#endif /* GPHIP_H */
