// gphip_hostlogic.inc -- host-side logic that the Wolfram-Language package used to carry (kernel-name grammar, CForm text ->
// function body, the starting pool of the tabulated-prior sampler).  It lives behind the C ABI so that it runs under test
// (tests/test_host_logic.py on the CPU, tests/test_gpu_wl_shim.py through the LibraryLink shim): the WL file cannot be executed
// in the build containers and keeps only what needs a Wolfram kernel (SURVEY.md section 7: "all logic in the C ABI").
// Included by gphip.hip.  No device code (gp_joint.h: the Philox counters of gphip_rff_table, which are host functions too).
#include "gp_joint.h"

namespace {
std::string hl_squash(const char* s) {             // lower case, without spaces and underscores: "SE ARD" = "se_ard" = "SEARD"
    std::string o;
    for (; s && *s; ++s)
        if (!isspace((unsigned char)*s) && *s != '_') o.push_back((char)tolower((unsigned char)*s));
    return o;
}
int hl_term_id(const std::string& t) {
    static const struct { const char* name; int id; } T[] = {
        {"se", GPHIP_KERNEL_SE}, {"seard", GPHIP_KERNEL_SE_ARD}, {"matern52", GPHIP_KERNEL_MATERN52}, {"matern52ard", GPHIP_KERNEL_MATERN52_ARD},
        {"matern32", GPHIP_KERNEL_MATERN32}, {"matern32ard", GPHIP_KERNEL_MATERN32_ARD}, {"rq", GPHIP_KERNEL_RQ}, {"rqard", GPHIP_KERNEL_RQ_ARD}};
    for (const auto& e : T)
        if (t == e.name) return e.id;
    return -1;
}
int hl_term_params(int id, int64_t d) {            // l.., (alpha), sf
    const bool ard = id == GPHIP_KERNEL_SE_ARD || id == GPHIP_KERNEL_MATERN52_ARD || id == GPHIP_KERNEL_MATERN32_ARD || id == GPHIP_KERNEL_RQ_ARD;
    const bool rq = id == GPHIP_KERNEL_RQ || id == GPHIP_KERNEL_RQ_ARD;
    return (int)(ard ? d : 1) + (rq ? 1 : 0) + 1;
}
}  // namespace

extern "C" {

/* Kernel grammar of the two hosts in ONE place (spaces, underscores and case ignored):
 *     term [(+|*) term] [+ const]      term: se, se_ard, matern52, matern52_ard, matern32, matern32_ard, rq, rq_ard;    null | none
 * spec[8] = {kernel_id (the integer gphip_create takes), term 1 id, op (0 none, 1 sum, 2 product), term 2 id (-1: none),
 *            offset (0 | 1), parameters of term 1, of term 2, 0-based position of sigma_n in theta}.
 * theta layout: [term 1: l.., (alpha), sf] [term 2: ..] [c] sn [mu].  GPHIP_ERR_ARG: not a kernel of the library (the WL
 * package then treats the argument as an arbitrary function, BGP:29-33). */
int gphip_kernel_parse(const char* name, int64_t d, int* spec) {
    if (!name || !spec || d < 1) return GPHIP_ERR_ARG;
    std::string key = hl_squash(name);
    for (int i = 0; i < 8; ++i) spec[i] = 0;
    spec[3] = -1;
    if (key == "null" || key == "none") {
        spec[0] = GPHIP_KERNEL_NULL; spec[1] = GPHIP_KERNEL_NULL; spec[7] = 0;
        return GPHIP_OK;
    }
    int offset = 0;
    if (key.size() > 6 && key.compare(key.size() - 6, 6, "+const") == 0) { key.resize(key.size() - 6); offset = 1; }
    int op = 0;
    std::string a = key, b;
    size_t pos = key.find('+');
    if (pos != std::string::npos) op = 1;
    else if ((pos = key.find('*')) != std::string::npos) op = 2;
    if (op) { a = key.substr(0, pos); b = key.substr(pos + 1); }
    const int ia = hl_term_id(a), ib = op ? hl_term_id(b) : -1;
    if (ia < 0 || (op && ib < 0)) return GPHIP_ERR_ARG;
    spec[1] = ia; spec[2] = op; spec[3] = ib; spec[4] = offset;
    spec[5] = hl_term_params(ia, d);
    spec[6] = op ? hl_term_params(ib, d) : 0;
    spec[7] = spec[5] + spec[6] + offset;
    spec[0] = (op == 0 && offset == 0) ? ia : GPHIP_KERNEL_COMPOSE(ia, op, op ? ib : 0, offset);
    return GPHIP_OK;
}

/* The text Mathematica's CForm prints for a covariance function applied to two symbolic points -> the function body
 * gphip_create_custom takes.  The WL package substitutes stand-in symbols for the coordinates and the hyper-parameters before
 * printing: <anything>gphipXc<k>, <anything>gphipYc<k>, <anything>gphipPc<k> (a symbol of a context that is not on $ContextPath
 * prints with its context, "GPHIP_Private_gphipXc0"); they become X(k), Y(k), P(k).  out = "return <text>;".
 * GPHIP_ERR_ARG: empty text, or text with characters no C expression of CForm contains (a quote, a brace, a semicolon, '#',
 * '`' left over outside a stand-in, a backslash); GPHIP_ERR_DIM: out is too small (cap). */
int gphip_cform_to_body(const char* cform, char* out, int64_t cap) {
    if (!cform || !out || cap < 16) return GPHIP_ERR_ARG;
    const std::string s(cform);
    std::string o = "return ";
    auto ident = [](char c) { return isalnum((unsigned char)c) || c == '_' || c == '`'; };
    size_t i = 0;
    bool any = false;
    while (i < s.size()) {
        if (ident(s[i]) && !(i > 0 && ident(s[i - 1]))) {
            size_t j = i;
            while (j < s.size() && ident(s[j])) ++j;
            const std::string tok = s.substr(i, j - i);
            size_t at = std::string::npos;
            char which = 0;
            for (const char* w : {"gphipXc", "gphipYc", "gphipPc"}) {
                const size_t f = tok.rfind(w);
                if (f != std::string::npos && f + 7 < tok.size() &&
                    tok.find_first_not_of("0123456789", f + 7) == std::string::npos) { at = f; which = w[5]; }
            }
            if (at != std::string::npos) {
                o += which; o += '('; o += tok.substr(at + 7); o += ')';
            } else {
                if (tok.find('`') != std::string::npos) return GPHIP_ERR_ARG;
                o += tok;
            }
            any = true;
            i = j;
            continue;
        }
        const char c = s[i];
        if (c == '"' || c == '\'' || c == '{' || c == '}' || c == ';' || c == '#' || c == '\\' || c == '`') return GPHIP_ERR_ARG;
        o += c;
        ++i;
    }
    if (!any) return GPHIP_ERR_ARG;
    o += ';';
    if ((int64_t)o.size() + 1 > cap) return GPHIP_ERR_DIM;
    memcpy(out, o.c_str(), o.size() + 1);
    return GPHIP_OK;
}

/* Starting pool of the sampler for a SEPARABLE prior given as tables (generateStartingPoints draws from the prior,
 * BS:1046-1068): `pool` independent draws per parameter from the density exp(tab[j][.]) on the m uniform grid nodes of
 * [box[2j], box[2j+1]] -- inverse CDF of the piecewise-linear density (trapezoid rule), splitmix64 stream `seed`.
 * tab values <= -1e299 read as log 0.  out: pool x p, row-major.  GPHIP_ERR_ARG: a factor with no mass inside its range. */
int gphip_tab_prior_sample(const double* box, const double* tab, int p, int64_t m, int pool, uint64_t seed, double* out) {
    if (!box || !tab || !out || p < 1 || m < 2 || pool < 1) return GPHIP_ERR_ARG;
    uint64_t st = seed * 0x9e3779b97f4a7c15ull + 0x632be59bd9b4e019ull;
    auto next = [&]() {
        uint64_t z = (st += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        z ^= z >> 31;
        return (double)(z >> 11) * (1.0 / 9007199254740992.0);
    };
    std::vector<double> dens((size_t)m), cdf((size_t)m);
    for (int j = 0; j < p; ++j) {
        const double lo = box[2 * j], hi = box[2 * j + 1], hstep = (hi - lo) / (double)(m - 1);
        if (!(hi > lo)) return GPHIP_ERR_ARG;
        double top = -1e300;
        for (int64_t i = 0; i < m; ++i) top = std::max(top, tab[(size_t)j * m + i]);
        if (!(top > -1e299)) return GPHIP_ERR_ARG;
        for (int64_t i = 0; i < m; ++i) {
            const double v = tab[(size_t)j * m + i];
            dens[(size_t)i] = (v <= -1e299 || !(v == v)) ? 0.0 : std::exp(v - top);
        }
        cdf[0] = 0.0;
        for (int64_t i = 1; i < m; ++i) cdf[(size_t)i] = cdf[(size_t)i - 1] + 0.5 * (dens[(size_t)i - 1] + dens[(size_t)i]);
        const double total = cdf[(size_t)m - 1];
        if (!(total > 0.0)) return GPHIP_ERR_ARG;
        for (int s = 0; s < pool; ++s) {
            const double u = next() * total;
            int64_t i = (int64_t)(std::upper_bound(cdf.begin(), cdf.end(), u) - cdf.begin());
            i = std::min<int64_t>(std::max<int64_t>(i, 1), m - 1);
            // within cell [i-1, i]: density linear from a to b; solve  a t + (b - a) t^2 / 2 = (u - cdf[i-1])  for t in [0, 1]
            const double a = dens[(size_t)i - 1], b = dens[(size_t)i], r = u - cdf[(size_t)i - 1];
            double t;
            if (std::fabs(b - a) < 1e-14 * (a + b)) t = (a + b) > 0.0 ? r / (0.5 * (a + b)) : 0.5;
            else t = (-a + std::sqrt(std::max(a * a + 2.0 * (b - a) * r, 0.0))) / (b - a);
            t = std::min(std::max(t, 0.0), 1.0);
            out[(size_t)s * p + j] = lo + ((double)(i - 1) + t) * hstep;
        }
    }
    return GPHIP_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// Random-Fourier-feature table of a named kernel at theta (gphip_rff_table; DESIGN.md section 8m): k(x, x') ~ sum_j a_j^2
// cos(Omega_j . (x - x')) with Omega_j drawn from the kernel's spectral law.  Pure host code, deterministic in its arguments.
// Random numbers: Philox counters (gp_joint.h) under the keys  seed ^ RFF_KEY * (tag + 1):
//     tag 4 t + 0   z_jc  = philox_normal(key, j, c)                    the Gaussian direction of feature j of term t (t = 0, 1)
//     tag 4 t + 1   the radial mixing variable of feature j: normals philox_normal(key, j, i), uniforms philox_uniform(key, j, i)
//     tag 8         b_j   = 2 pi philox_uniform(key, j, 0)              the phase
//     tag 9         eps_si = sn philox_normal(key, s, i)                the observation noise of gphip_paths_create (RFF_TAG_EPS):
//                   a tag the table never uses, so eps is independent of (Omega, b).  key = seed ^ 0x2E2AC13EF8E8D8D2.
//     tag 10        xi_si   = philox_normal(key, s, i)                  gphip_sparse_paths_create: the draw of the whitened inducing values
//     tag 11        zeta_si = philox_normal(key, s, i)                  gphip_sparse_paths_create: the jitter's share of the prior at Z
//                   (RFF_TAG_XI, RFF_TAG_ZETA in gphip_sparse_paths.inc: 11 and 12 times RFF_KEY, which no other stream uses)
// gphip_paths_create draws w under the seed itself.  RFF_KEY is odd, so the keys of the tags 0 .. 11 and the seed are all distinct.
//     SE          omega = z                          Matern-nu   omega = z sqrt(2 nu / u), u = the sum of 2 nu squared normals
//     RQ(alpha)   omega = z sqrt(tau), tau ~ Gamma(shape alpha, scale 1 / alpha)  (Marsaglia-Tsang; alpha < 1: the U^(1/alpha) boost)
// Omega_jc = omega_c / l_c.  Sum: the two terms' features side by side, a = sf_t sqrt(2 / F).  Product: Omega = Omega1 + Omega2 of
// independent draws, a = sf_1 sf_2 sqrt(2 / F).  Offset c (k = .. + c): one more feature with Omega = 0, b = 0, a = sqrt(c).
// The rows of a table of F features are NOT a prefix of the rows of a larger table (a depends on F; a sum's second term starts at F).
// ---------------------------------------------------------------------------------------------
namespace {
constexpr uint64_t RFF_KEY = 0x9E3779B97F4A7C15ull;
constexpr int RFF_TAG_EPS = 9;
inline uint64_t rff_key(uint64_t seed, int tag) { return seed ^ (RFF_KEY * (uint64_t)(tag + 1)); }

// Gamma(shape, 1) for feature j from the counters of `key` (Marsaglia & Tsang 2000)
double rff_gamma(uint64_t key, uint32_t j, double shape) {
    const double boost = shape < 1.0 ? std::pow(1.0 - gphip::philox_uniform(key, j, 0xFFFFFFFFu), 1.0 / shape) : 1.0;   // (1 - u in (0, 1])
    const double a = shape < 1.0 ? shape + 1.0 : shape;
    const double dd = a - 1.0 / 3.0, cc = 1.0 / std::sqrt(9.0 * dd);
    for (uint32_t it = 0; it < 0x7FFFFFFFu; ++it) {
        const double x = gphip::philox_normal(key, j, 2 * it), v0 = 1.0 + cc * x;
        if (v0 <= 0.0) continue;
        const double v = v0 * v0 * v0, u = 1.0 - gphip::philox_uniform(key, j, 2 * it + 1);
        if (std::log(u) < 0.5 * x * x + dd - dd * v + dd * std::log(v)) return boost * dd * v;
    }
    return boost * dd;
}

struct RffTerm { int fam; bool ard; const double* ell; double alpha, sf; };

// the decoded kernel: terms, operation, offset and the number of parameters in front of sn
int rff_decode(int kernel_id, int64_t d, const double* theta, RffTerm* t, int* op, int* offs, int* nparam) {
    if (kernel_id == GPHIP_KERNEL_CUSTOM || kernel_id == GPHIP_KERNEL_NULL) return GPHIP_ERR_UNSUPPORTED;
    auto base = [](int id, RffTerm& b) {
        switch (id) {
            case GPHIP_KERNEL_SE: b.fam = 0; b.ard = false; return true;
            case GPHIP_KERNEL_SE_ARD: b.fam = 0; b.ard = true; return true;
            case GPHIP_KERNEL_MATERN52: b.fam = 1; b.ard = false; return true;
            case GPHIP_KERNEL_MATERN52_ARD: b.fam = 1; b.ard = true; return true;
            case GPHIP_KERNEL_MATERN32: b.fam = 2; b.ard = false; return true;
            case GPHIP_KERNEL_MATERN32_ARD: b.fam = 2; b.ard = true; return true;
            case GPHIP_KERNEL_RQ: b.fam = 3; b.ard = false; return true;
            case GPHIP_KERNEL_RQ_ARD: b.fam = 3; b.ard = true; return true;
            default: return false;
        }
    };
    const bool composed = kernel_id >= (1 << 24);
    const int id1 = composed ? (kernel_id & 0xff) : kernel_id, id2 = composed ? ((kernel_id >> 8) & 0xff) : 0;
    *op = composed ? ((kernel_id >> 16) & 0xf) : 0;
    *offs = composed ? ((kernel_id >> 20) & 0xf) : 0;
    if (kernel_id < 0 || !base(id1, t[0]) || *op > 2 || *offs > 1 || (*op != 0 && !base(id2, t[1]))) return GPHIP_ERR_ARG;
    int o = 0;
    for (int k = 0; k < (*op != 0 ? 2 : 1); ++k) {
        if (theta) t[k].ell = theta + o;
        o += t[k].ard ? (int)d : 1;
        t[k].alpha = 1.0;
        if (t[k].fam == 3) { if (theta) t[k].alpha = theta[o]; ++o; }
        if (theta) t[k].sf = theta[o];
        ++o;
    }
    *nparam = o + *offs;
    return GPHIP_OK;
}
}  // namespace

extern "C" {

int gphip_rff_table(int kernel_id, int64_t d, const double* theta, int p, int F, uint64_t seed, int64_t* Ftot_out, double* omega,
                    double* phase, double* amp) {
    if (d < 1 || F < 1) return GPHIP_ERR_DIM;
    RffTerm t[2] = {};
    int op = 0, offs = 0, np = 0;
    if (const int rc = rff_decode(kernel_id, d, theta, t, &op, &offs, &np)) return rc;
    if (p != np + 1 && p != np + 2) return GPHIP_ERR_DIM;                  // .. sn [mu]
    const int64_t Ftot = (op == 1 ? 2 : 1) * (int64_t)F + offs;
    if (Ftot_out) *Ftot_out = Ftot;
    if (!omega) return Ftot_out ? GPHIP_OK : GPHIP_ERR_ARG;                // the size query
    if (!theta || !phase || !amp) return GPHIP_ERR_ARG;
    const int nterm = op != 0 ? 2 : 1;
    for (int k = 0; k < nterm; ++k) {
        for (int c = 0; c < (t[k].ard ? (int)d : 1); ++c)
            if (!(std::fabs(t[k].ell[c]) > 0.0) || !std::isfinite(1.0 / t[k].ell[c])) return GPHIP_ERR_ARG;
        if (!std::isfinite(t[k].sf) || (t[k].fam == 3 && !(t[k].alpha > 0.0 && std::isfinite(t[k].alpha)))) return GPHIP_ERR_ARG;
    }
    const double cst = offs ? theta[np - 1] : 0.0;
    if (offs && !(cst >= 0.0 && std::isfinite(cst))) return GPHIP_ERR_ARG;   // a negative constant is not a variance
    const double two_pi = 6.283185307179586476925286766559;
    // omega of feature j of term k -> row (+=: the product adds its second term's draw)
    auto direction = [&](int k, uint32_t j, double* row, bool add) {
        const uint64_t kz = rff_key(seed, 4 * k), ku = rff_key(seed, 4 * k + 1);
        double scale = 1.0;
        if (t[k].fam == 1 || t[k].fam == 2) {
            const int dof = t[k].fam == 1 ? 5 : 3;
            double u = 0.0;
            for (int i = 0; i < dof; ++i) { const double n = gphip::philox_normal(ku, j, (uint32_t)i); u += n * n; }
            scale = std::sqrt((double)dof / u);
        } else if (t[k].fam == 3) {
            scale = std::sqrt(rff_gamma(ku, j, t[k].alpha) / t[k].alpha);
        }
        for (int64_t c = 0; c < d; ++c) {
            const double w = gphip::philox_normal(kz, j, (uint32_t)c) * scale / std::fabs(t[k].ell[t[k].ard ? c : 0]);
            row[c] = add ? row[c] + w : w;
        }
    };
    const uint64_t kp = rff_key(seed, 8);
    const double rt = std::sqrt(2.0 / (double)F);
    for (int64_t j = 0; j < Ftot - offs; ++j) {
        const int k = (op == 1 && j >= F) ? 1 : 0;
        const uint32_t jj = (uint32_t)(k ? j - F : j);
        direction(k, jj, omega + j * d, false);
        if (op == 2) direction(1, jj, omega + j * d, true);
        phase[j] = two_pi * gphip::philox_uniform(kp, (uint32_t)j, 0u);
        amp[j] = (op == 2 ? std::fabs(t[0].sf * t[1].sf) : std::fabs(t[k].sf)) * rt;
    }
    if (offs) {
        for (int64_t c = 0; c < d; ++c) omega[(Ftot - 1) * d + c] = 0.0;
        phase[Ftot - 1] = 0.0;
        amp[Ftot - 1] = std::sqrt(cst);
    }
    return GPHIP_OK;
}

}  // extern "C"
