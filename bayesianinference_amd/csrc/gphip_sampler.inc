// gphip_sampler.inc -- native nested-sampling driver over the GP hyper-parameters (part of gphip.hip's translation unit).
//
// SURVEY.md §8f rank 1: the caller that generates all the load.  The reference's nestedSamplingInternal
// (BayesianStatistics.wl:859-1040, BS below) advances ONE constrained-prior Metropolis chain by "MonteCarloSteps" strictly
// sequential likelihood calls per iteration (BS:990-1012) -- 200 dependent GPU round trips, the regime in which the device
// is latency bound.  Here `walkers` chains start from random live points and advance in LOCK STEP, so every Metropolis step
// is ONE batched call theta[W x p] -> l[W] (gphip_loglik_batch).  A walker's end point is a draw from the prior restricted
// to {L > L*_i}; it is consumed at a later iteration i + j only if it still satisfies L > L*_{i+j} (an exact rejection
// step), so the shrinkage law log X_i = -i/n of the reference (calculateXValues, BS:790-802) is preserved.  The Python
// module bayesianinference_amd/nested_sampling.py is the same algorithm and stays as this code's test oracle (the
// deterministic pieces are compared value for value, the sampler through unbiasedness of log Z over many seeds).
//
//   calculateXValues["Log"]   BS:790-802     log X_i = -i/n (deleted), log(i/(n+1)) - nDel/n (live, i = n..1)
//   trapezoidWeigths["Log"]   BS:757-771     w_i = (X_{i-1} - X_{i+1})/2, X_0 = 2 - X_1, last = (X_{m-1} + X_m)/2
//   calculateWeightsCrude     BS:818-835     sort by (LogLikelihood, Point); weights + LogLikelihood
//   stop rule                 BS:967-978     min X * L_max / Z <= "TerminationFraction"
//   nsMCMC / nsDensity        BS:707-745, 602-628   Metropolis on the prior restricted to {L > L*, theta in box}
// The chain kernel of the reference (Statistics`MCMC`, closed source) cannot be reproduced bit for bit: only log Z +- its
// own standard error is comparable.  evidenceSampling / combineRuns (BS:1158-1315) stay with the host: the WL wrapper hands
// the samples to the reference's OWN evidenceSampling, the Python host to nested_sampling.evidence_sampling.

#include <numeric>

namespace {

constexpr double NS_LOG_ZERO = -1.7976931348623157e308;      // stands for $MachineLogZero (BU:47) inside the sampler

struct NsRng {                                               // xoshiro256** seeded by splitmix64
    uint64_t s[4];
    explicit NsRng(uint64_t seed) {
        uint64_t z = seed + 0x9E3779B97F4A7C15ull;
        for (auto& v : s) {
            z += 0x9E3779B97F4A7C15ull;
            uint64_t t = z;
            t = (t ^ (t >> 30)) * 0xBF58476D1CE4E5B9ull;
            t = (t ^ (t >> 27)) * 0x94D049BB133111EBull;
            v = t ^ (t >> 31);
        }
    }
    static uint64_t rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
    uint64_t next() {
        const uint64_t r = rotl(s[1] * 5, 7) * 9, t = s[1] << 17;
        s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]; s[2] ^= t; s[3] = rotl(s[3], 45);
        return r;
    }
    double uniform() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }     // [0, 1)
    double normal() {                                        // Box-Muller
        const double u1 = 1.0 - uniform(), u2 = uniform();
        return std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2);
    }
    int below(int n) { return (int)(uniform() * n) % n; }
};

double ns_log_subtract(double logy, double logx) { return logy + std::log1p(-std::exp(logx - logy)); }     // BU:337-343
double ns_log_add(double a, double b) {                                                                    // BU:345-356
    const double hi = std::max(a, b), lo = std::min(a, b);
    return hi + std::log1p(std::exp(lo - hi));
}
double ns_log_sum_exp(const std::vector<double>& v) {                                                      // BU:318-335
    double m = -INFINITY;
    for (double x : v) if (x > m) m = x;
    if (!(m > -INFINITY)) return -INFINITY;
    double s = 0.0;
    for (double x : v) if (x > -INFINITY) s += std::exp(x - m);
    return m + std::log(s);
}

// calculateWeightsCrude (BS:818-835): order = samples sorted by (LogLikelihood, Point), logx of that order, crude log
// posterior weights (trapezoid weights + log-likelihood)
void ns_crude_weights(const double* pts, const double* ll, int64_t m, int p, int pool, std::vector<int64_t>& order,
                      std::vector<double>& logx, std::vector<double>& logw) {
    order.resize((size_t)m);
    std::iota(order.begin(), order.end(), (int64_t)0);
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
        if (ll[a] != ll[b]) return ll[a] < ll[b];
        for (int j = 0; j < p; ++j)
            if (pts[a * p + j] != pts[b * p + j]) return pts[a * p + j] < pts[b * p + j];
        return false;
    });
    const int64_t ndel = m - pool;
    logx.resize((size_t)m);
    for (int64_t k = 0; k < ndel; ++k) logx[(size_t)k] = -(double)(k + 1) / pool;                         // BS:790-802
    for (int i = 0; i < pool; ++i) logx[(size_t)(ndel + i)] = std::log((double)(pool - i) / (pool + 1.0)) - (double)ndel / pool;
    logw.resize((size_t)m);
    for (int64_t i = 0; i + 1 < m; ++i) {                                                                 // BS:757-771
        const double left = i == 0 ? ns_log_subtract(std::log(2.0), logx[0]) : logx[(size_t)i - 1];
        logw[(size_t)i] = std::log(0.5) + ns_log_subtract(left, logx[(size_t)i + 1]) + ll[order[(size_t)i]];
    }
    logw[(size_t)m - 1] = std::log(0.5) + ns_log_add(logx[(size_t)m - 2], logx[(size_t)m - 1]) + ll[order[(size_t)m - 1]];
}

// unbiased sample covariance of the rows idx[0..k) of pts (np.cov / Covariance[]), d x d row-major
void ns_covariance(const double* pts, const std::vector<int64_t>& idx, int p, std::vector<double>& cov) {
    const size_t k = idx.size();
    std::vector<double> mean((size_t)p, 0.0);
    for (int64_t i : idx)
        for (int j = 0; j < p; ++j) mean[(size_t)j] += pts[i * p + j];
    for (double& v : mean) v /= (double)k;
    cov.assign((size_t)p * p, 0.0);
    for (int64_t i : idx)
        for (int a = 0; a < p; ++a)
            for (int b = 0; b <= a; ++b) cov[(size_t)a * p + b] += (pts[i * p + a] - mean[(size_t)a]) * (pts[i * p + b] - mean[(size_t)b]);
    for (int a = 0; a < p; ++a)
        for (int b = 0; b <= a; ++b) {
            cov[(size_t)a * p + b] /= (double)(k > 1 ? k - 1 : 1);
            cov[(size_t)b * p + a] = cov[(size_t)a * p + b];
        }
}

// lower Cholesky factor of (2.38^2 / d) cov + jitter (Haario et al. adaptive-Metropolis scaling); false if not SPD
bool ns_proposal_factor(const std::vector<double>& cov, int p, std::vector<double>& L) {
    L.assign((size_t)p * p, 0.0);
    const double sc = 2.38 * 2.38 / p;
    for (int j = 0; j < p; ++j) {
        for (int i = j; i < p; ++i) {
            double s = sc * cov[(size_t)i * p + j] + (i == j ? 1e-12 * (cov[(size_t)i * p + i] + 1e-300) : 0.0);
            for (int k = 0; k < j; ++k) s -= L[(size_t)i * p + k] * L[(size_t)j * p + k];
            if (i == j) {
                if (!(s > 0.0)) return false;
                L[(size_t)j * p + j] = std::sqrt(s);
            } else {
                L[(size_t)i * p + j] = s / L[(size_t)j * p + j];
            }
        }
    }
    return true;
}

struct NsPrior {
    const double* box;           // p x 2
    const int* kind;             // per parameter: 0 uniform, 1 log-uniform (density 1 / (theta log(hi/lo))); null = all uniform
    gphip_logprior_fn fn;        // optional user prior (overrides `kind`); still restricted to the box
    void* user;
    int p;
    bool in_box(const double* th) const {
        for (int j = 0; j < p; ++j)
            if (!(th[j] >= box[2 * j] && th[j] <= box[2 * j + 1])) return false;
        return true;
    }
    double logpdf(const double* th) const {                  // "LogPriorPDFFunction" (BS:256-274); NS_LOG_ZERO outside the box
        if (!in_box(th)) return NS_LOG_ZERO;
        if (fn) {
            const double v = fn(th, p, user);
            return std::isfinite(v) ? v : NS_LOG_ZERO;
        }
        double s = 0.0;
        for (int j = 0; j < p; ++j) {
            const double lo = box[2 * j], hi = box[2 * j + 1];
            if (kind && kind[j] == 1) s -= std::log(th[j]) + std::log(std::log(hi / lo));
            else s -= std::log(hi - lo);
        }
        return s;
    }
    void draw(NsRng& rng, double* th) const {                // RandomVariate[prior] for the built-in product priors
        for (int j = 0; j < p; ++j) {
            const double lo = box[2 * j], hi = box[2 * j + 1], u = rng.uniform();
            th[j] = (kind && kind[j] == 1) ? lo * std::exp(u * std::log(hi / lo)) : lo + u * (hi - lo);
        }
    }
};

// likelihood of a batch with the reference's failure convention: info != 0 / non-finite -> the sentinel.  eval: the batched
// evaluator (Theta, B, p, out, info) -> status -- gphip_loglik_batch of an exact GP, gphip_sparse_bound_batch of a sparse one
template <typename Eval>
int ns_loglik(Eval& eval, const double* Theta, int B, int p, std::vector<double>& out, std::vector<int>& info, int64_t* n_evals) {
    out.resize((size_t)B);
    info.resize((size_t)B);
    if (B == 0) return GPHIP_OK;
    const int rc = eval(Theta, B, p, out.data(), info.data());
    if (rc) return rc;
    for (int i = 0; i < B; ++i)
        if (info[(size_t)i] != 0 || !std::isfinite(out[(size_t)i])) out[(size_t)i] = NS_LOG_ZERO;
        else out[(size_t)i] = std::min(std::max(out[(size_t)i], NS_LOG_ZERO), -NS_LOG_ZERO);      // Clip, BGP:183
    *n_evals += B;
    return GPHIP_OK;
}

// The driver itself, shared by the exact GP (gphip_nested_sampling) and the sparse one (gphip_sparse_nested_sampling): eval is the
// batched evaluator of ns_loglik over p hyper-parameters, failf(code, message) records an error with the caller's handle and
// returns the code.  The caller holds its handle's lock.
template <typename Eval, typename Fail>
int ns_run(int p, Eval&& eval, Fail&& failf, const double* box, const int* prior_kind, gphip_logprior_fn logprior, void* user,
           const gphip_ns_options* opts, const double* start, int64_t cap, double* points, double* loglik, double* logprior_out,
           double* accept_rate, int64_t* n_samples, double* log_evidence, int64_t* n_evals) {
    if (!box || !opts || !points || !loglik || !n_samples) return failf(GPHIP_ERR_ARG, "null argument");
    const int n = opts->pool, W = std::max(1, opts->walkers);
    if (n < 2 || cap < n + 1 || opts->mc_steps < 1) return failf(GPHIP_ERR_ARG, "pool < 2, cap <= pool or mc_steps < 1");
    for (int j = 0; j < p; ++j)
        if (!(box[2 * j] < box[2 * j + 1]) || (prior_kind && prior_kind[j] == 1 && !(box[2 * j] > 0.0)))
            return failf(GPHIP_ERR_ARG, "parameter box must have lo < hi (and lo > 0 for a log-uniform prior)");
    NsPrior prior{box, prior_kind, logprior, user, p};
    NsRng rng(opts->seed);
    int64_t evals = 0;
    std::vector<double> pts((size_t)n * p), ll, lpr((size_t)n), acc((size_t)n, std::nan(""));
    std::vector<int> info;
    if (start) std::copy(start, start + (size_t)n * p, pts.begin());          // generateStartingPoints is host business (BS:1046-1068)
    else for (int i = 0; i < n; ++i) prior.draw(rng, &pts[(size_t)i * p]);
    int rc = ns_loglik(eval, pts.data(), n, p, ll, info, &evals);                // initial sweep, BS:902-916: ONE batched call
    if (rc) return rc;
    for (int i = 0; i < n; ++i) lpr[(size_t)i] = prior.logpdf(&pts[(size_t)i * p]);
    std::vector<int64_t> idx((size_t)n);
    std::iota(idx.begin(), idx.end(), (int64_t)0);
    std::vector<double> cov, covb, L;
    ns_covariance(pts.data(), idx, p, cov);                                   // BS:923
    const int max_it = std::max(opts->max_iterations, opts->min_iterations), min_it = std::min(opts->max_iterations, opts->min_iterations);
    double logz = NS_LOG_ZERO;
    std::vector<double> cand_pts, cand_ll, cand_rate;                         // walker end points not consumed yet (+ their batch's acceptance rate)
    std::vector<int64_t> order;
    std::vector<double> logx, logw;
    int iteration = 1;
    while (iteration <= max_it && (int64_t)ll.size() < cap) {
        const int64_t m = (int64_t)ll.size();
        if (iteration > 1 && iteration > min_it) {                            // stop rule BS:967-978
            ns_crude_weights(pts.data(), ll.data(), m, p, n, order, logx, logw);
            const double lmax = *std::max_element(ll.begin(), ll.end());
            const double missing = std::exp(*std::min_element(logx.begin(), logx.end())) * std::exp(std::min(lmax - logz, 700.0));
            if (missing <= opts->termination_fraction) break;
        }
        // bestPoints (BS:980): the n samples of highest likelihood = the live set; threshold = its minimum
        std::vector<int64_t> byl((size_t)m);
        std::iota(byl.begin(), byl.end(), (int64_t)0);
        std::stable_sort(byl.begin(), byl.end(), [&](int64_t a, int64_t b) { return ll[(size_t)a] < ll[(size_t)b]; });
        std::vector<int64_t> best(byl.end() - n, byl.end());
        const double threshold = ll[(size_t)best[0]];
        ns_covariance(pts.data(), best, p, covb);
        for (size_t i = 0; i < cov.size(); ++i) cov[i] = 0.5 * (cov[i] + covb[i]);         // BS:988
        {   // exact rejection of stale candidates
            std::vector<double> kp, kl, kr;
            for (size_t c = 0; c < cand_ll.size(); ++c)
                if (cand_ll[c] > threshold) {
                    kl.push_back(cand_ll[c]);
                    kr.push_back(cand_rate[c]);
                    kp.insert(kp.end(), cand_pts.begin() + c * p, cand_pts.begin() + (c + 1) * p);
                }
            cand_pts.swap(kp); cand_ll.swap(kl); cand_rate.swap(kr);
        }
        double factor = 1.0;
        while (cand_ll.empty()) {
            const int steps = (int)std::ceil(factor * opts->mc_steps);
            if (!ns_proposal_factor(cov, p, L)) return failf(GPHIP_ERR_ARG, "nested sampling: the live points are degenerate (singular covariance)");
            // W walkers in lock step: random live points, Metropolis on the prior restricted to {L > threshold, box}
            std::vector<double> x((size_t)W * p), lx((size_t)W, std::nan("")), lp((size_t)W), prop((size_t)W * p), lpp((size_t)W);
            for (int w = 0; w < W; ++w) {
                const int64_t src = best[(size_t)rng.below(n)];                            // RandomChoice[bestPoints], BS:992
                std::copy(&pts[(size_t)src * p], &pts[(size_t)src * p] + p, &x[(size_t)w * p]);
                lp[(size_t)w] = prior.logpdf(&x[(size_t)w * p]);
            }
            int64_t accepted = 0;
            std::vector<double> zv((size_t)p), batch, bl;
            std::vector<int> which;
            for (int s = 0; s < steps; ++s) {
                batch.clear(); which.clear();
                for (int w = 0; w < W; ++w) {
                    for (int j = 0; j < p; ++j) zv[(size_t)j] = rng.normal();
                    for (int i = 0; i < p; ++i) {
                        double v = x[(size_t)w * p + i];
                        for (int j = 0; j <= i; ++j) v += L[(size_t)i * p + j] * zv[(size_t)j];
                        prop[(size_t)w * p + i] = v;
                    }
                    lpp[(size_t)w] = prior.logpdf(&prop[(size_t)w * p]);
                    if (lpp[(size_t)w] > NS_LOG_ZERO) {
                        which.push_back(w);
                        batch.insert(batch.end(), &prop[(size_t)w * p], &prop[(size_t)w * p] + p);
                    }
                }
                rc = ns_loglik(eval, batch.data(), (int)which.size(), p, bl, info, &evals);   // ONE batched likelihood call per step
                if (rc) return rc;
                std::vector<double> lnew((size_t)W, NS_LOG_ZERO);
                for (size_t c = 0; c < which.size(); ++c) lnew[(size_t)which[c]] = bl[c];
                for (int w = 0; w < W; ++w) {
                    const double u = std::log(rng.uniform());                              // (drawn for every walker: reproducible streams)
                    if (lpp[(size_t)w] > NS_LOG_ZERO && lnew[(size_t)w] > threshold && u < lpp[(size_t)w] - lp[(size_t)w]) {
                        std::copy(&prop[(size_t)w * p], &prop[(size_t)w * p] + p, &x[(size_t)w * p]);
                        lx[(size_t)w] = lnew[(size_t)w];
                        lp[(size_t)w] = lpp[(size_t)w];
                        ++accepted;
                    }
                }
            }
            const double rate = (double)accepted / ((double)W * steps);
            // BS:990-1004: re-run with 1.25x the steps until the acceptance rate lies inside "MinMaxAcceptanceRate"
            if (rate >= opts->min_accept && rate <= opts->max_accept)
                for (int w = 0; w < W; ++w)
                    if (!std::isnan(lx[(size_t)w])) {                                      // walkers that never moved duplicate a live point
                        cand_ll.push_back(lx[(size_t)w]);
                        cand_rate.push_back(rate);
                        cand_pts.insert(cand_pts.end(), &x[(size_t)w * p], &x[(size_t)w * p] + p);
                    }
            factor *= 1.25;                                                                // BS:1003
            if (factor > 50) return failf(GPHIP_ERR_ARG, "nested sampling: no walker could move (\"Bad likelihood function\", BS:917-921)");
        }
        pts.insert(pts.end(), cand_pts.begin(), cand_pts.begin() + p);                     // BS:1012 (value carried from the chain)
        ll.push_back(cand_ll[0]);
        lpr.push_back(prior.logpdf(cand_pts.data()));
        acc.push_back(cand_rate[0]);                                                       // of the walker batch the point came from
        cand_pts.erase(cand_pts.begin(), cand_pts.begin() + p);
        cand_ll.erase(cand_ll.begin());
        cand_rate.erase(cand_rate.begin());
        ns_crude_weights(pts.data(), ll.data(), (int64_t)ll.size(), p, n, order, logx, logw);
        logz = ns_log_sum_exp(logw);                                                       // BS:1019
        ++iteration;
    }
    const int64_t m = (int64_t)ll.size();
    std::copy(pts.begin(), pts.end(), points);
    std::copy(ll.begin(), ll.end(), loglik);
    if (logprior_out) std::copy(lpr.begin(), lpr.end(), logprior_out);
    if (accept_rate) std::copy(acc.begin(), acc.end(), accept_rate);
    *n_samples = m;
    if (log_evidence) {
        ns_crude_weights(pts.data(), ll.data(), m, p, n, order, logx, logw);
        *log_evidence = ns_log_sum_exp(logw);
    }
    if (n_evals) *n_evals = evals;
    return GPHIP_OK;
}

}  // namespace

extern "C" {

int gphip_ns_default_options(gphip_ns_options* o) {          // BS:833-855
    if (!o) return GPHIP_ERR_ARG;
    o->pool = 100; o->max_iterations = 10000; o->min_iterations = 100; o->mc_steps = 200; o->walkers = 32;
    o->termination_fraction = 0.01; o->min_accept = 0.0; o->max_accept = 1.0; o->seed = 0;
    return GPHIP_OK;
}

// deterministic pieces, exported for the tests (compared value for value with nested_sampling.calculate_weights_crude)
int gphip_ns_crude_weights(const double* points, const double* loglik, int64_t m, int p, int pool, int64_t* order, double* logx,
                           double* logw, double* log_evidence) {
    if (!points || !loglik || !order || !logx || !logw || m < 2 || p < 1 || pool < 1 || pool > m) return GPHIP_ERR_ARG;
    std::vector<int64_t> o;
    std::vector<double> x, w;
    ns_crude_weights(points, loglik, m, p, pool, o, x, w);
    for (int64_t i = 0; i < m; ++i) { order[i] = o[(size_t)i]; logx[i] = x[(size_t)i]; logw[i] = w[(size_t)i]; }
    if (log_evidence) *log_evidence = ns_log_sum_exp(w);
    return GPHIP_OK;
}

int gphip_nested_sampling(gphip_handle h, const double* box, const int* prior_kind, gphip_logprior_fn logprior, void* user,
                          const gphip_ns_options* opts, const double* start, int64_t cap, double* points, double* loglik,
                          double* logprior_out, double* accept_rate, int64_t* n_samples, double* log_evidence, int64_t* n_evals) {
    if (!h) return GPHIP_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    return ns_run(h->p, [h](const double* Theta, int B, int p, double* out, int* info) { return gphip_loglik_batch(h, Theta, B, p, out, info); },
                  [h](int code, const char* msg) { return fail(h, code, msg); }, box, prior_kind, logprior, user, opts, start, cap, points,
                  loglik, logprior_out, accept_rate, n_samples, log_evidence, n_evals);
}

}  // extern "C"
