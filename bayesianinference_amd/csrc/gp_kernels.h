// gp_kernels.h -- hand-written gfx950 (CDNA4, wave64) kernels of the GP likelihood path.
//
//   k_scale        xs = x / l                       (prologue of K1)
//   kbuild_kernel  K1/K7: pairwise kernel matrix tiles, lower triangle, straight into the
//                  Cholesky workspace (BGP:29-43 covarianceMatrix; BGP:100-109 cross form)
//   potrf128       K2a + K3: 128x128 diagonal-block Cholesky + triangular inverse in LDS (MFMA),
//                  log-det partial, SPD test
//   gemm_nt        K2b/K2c on MFMA: mode 1 = panel solve X <- X W^T (also carries r -> z = L^-1 r,
//                  K4), mode 0 = C -= A B^T SYRK/GEMM trailing update
//   finalize       log det = 2 sum log L_ii, quad = |z|^2, info
//   predict_partial / predict_finish   K9/K10 epilogue: mu* and var* from V = k*^T L^-T and z (V streamed once)
//
// Every kernel is templated on the arithmetic type T: double (v_mfma_f64_16x16x4_f64, the headline
// path) or float (v_mfma_f32_16x16x4_f32, BASELINE.json config 5).  The two MFMA forms share the A/B
// operand layout (lane -> row l&15, k = l>>4) but NOT the C/D layout -- f64: row = (l>>4) + 4 reg,
// f32: row = 4 (l>>4) + reg -- which is what Num<T>::drow encodes.
//
// Storage: one workspace per batch slot in TILE-MAJOR PACKED LOWER-TRIANGULAR form.  The bordered matrix has
// R = Nt + 1 tile rows (Nt = Npad / 128, Npad = N rounded up to the 128 tile); only the tiles (ti, tj) with
// ti >= tj exist, each one a contiguous 128 KiB (fp64) block, column-major inside (leading dimension 128), stored
// tile column by tile column from the diagonal down: tile (ti, tj) sits at tile_index(ti, tj, R) * 128 * 128
// elements.  So a workgroup's C tile, every LDS-DMA stage of an operand tile and every tile the kernel build
// writes is ONE contiguous chunk, an outer panel (consecutive tile columns) is one contiguous range (the
// multi-GPU exchange needs no pack), and a slot costs R (R + 1) / 2 tiles instead of (R * 128)^2 elements.
// Tile row Nt carries right-hand sides as extra ROWS (row Npad = r^T): the panel solve and the trailing update
// then produce z^T = (L^-1 r)^T in that row and -|z|^2 in element (Npad, Npad) with no extra kernels
// ("bordered" Cholesky).  Scratch blocks that are not the factor (V of the substitutions, W_b, K^-1) stay plain
// column-major with a leading dimension; GEMM operands are described as either form.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

// [rtc-begin]  From here to [rtc-end] the text is ALSO compiled at run time (hiprtc, csrc/rtc_dyn.h) for handles created with
// gphip_create_custom: the same kernel build, instantiated with KT = 3 around a covariance function the caller supplied as
// source text (GP_CUSTOM_KERNEL).  Keep the region self-contained: no std:: headers, nothing declared outside it.
namespace gphip {

// Bumped whenever a struct or constant the run-time compiled copy of this region shares with the offline library changes
// (KBuildArgs, SLOTP, the tile layout): rtc_dyn.h refuses a source tree whose value differs from the library's own.
#define GP_RTC_ABI 7
// A run-time compiled program is built for ONE handle, whose input dimension is known: the generated source defines GP_D and the
// dimension loops of the caller's function unroll (their per-dimension reciprocals then leave the column loop).  Offline: the argument.
#ifdef GP_D
#define GP_DIM(x) (GP_D)
#else
#define GP_DIM(x) (x)
#endif
constexpr int TB = 128;         // tile edge
// elements between consecutive tiles of the packed workspace (a pad behind every tile was measured in round 3: no gain)
constexpr long TS = (long)TB * TB;

// index (in tiles) of tile (ti, tj), ti >= tj, in the packed lower-triangular tile-major workspace of R tile rows
__host__ __device__ __forceinline__ long tile_index(int ti, int tj, int R) {
    return (long)tj * R - ((long)tj * (tj - 1)) / 2 + (ti - tj);
}
// Multi-GPU 1-D block-cyclic layout: slot of tile column tj in the per-panel tables -- outer panel tj / panel for the nt
// matrix columns, and one extra slot (the number of outer panels) for the rhs column tj == nt, whose only tile is the corner
__host__ __device__ __forceinline__ int panel_slot(int tj, int nt, int panel) {
    return tj >= nt ? (nt + panel - 1) / panel : tj / panel;
}
constexpr int SLOTP = 16;       // doubles of per-slot scalars: [0] sf2 (term 1), [1] sn2, [2] mu, [3] pivot_tol, [4] bad_theta,
                                // [5] sf2 of term 2, [6] alpha of term 1, [7] alpha of term 2 (rational quadratic), [8] constant
                                // offset c, [9] k(x, x) (prior variance without the nugget), [10] != 0: the slot's kernel matrix is
                                // built by kbuild_mfma_kernel (distance cross term on the matrix pipe), not by kbuild_kernel

typedef double d4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void glb_void;

// ---------------------------------------------------------------------------------------------
// exp(x) for x <= 0, fp64, no hardware transcendental on gfx950: Cody-Waite reduction by ln2,
// degree-13 Taylor/Horner on |r| <= ln2/2 (truncation 4e-18), v_ldexp_f64 scaling. ~20 VALU ops.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double exp_nonpos(double x) {
    x = fmax(x, -800.0);
    const double k = __builtin_rint(x * 1.4426950408889634074);
    double r = __builtin_fma(-k, 6.93147180369123816490e-01, x);
    r = __builtin_fma(-k, 1.90821492927058770002e-10, r);
    double p = 1.6059043836821613e-10;              // 1/13!
    p = __builtin_fma(p, r, 2.0876756987868099e-09);   // 1/12!
    p = __builtin_fma(p, r, 2.5052108385441719e-08);   // 1/11!
    p = __builtin_fma(p, r, 2.7557319223985891e-07);   // 1/10!
    p = __builtin_fma(p, r, 2.7557319223985893e-06);   // 1/9!
    p = __builtin_fma(p, r, 2.4801587301587302e-05);   // 1/8!
    p = __builtin_fma(p, r, 1.9841269841269841e-04);   // 1/7!
    p = __builtin_fma(p, r, 1.3888888888888889e-03);   // 1/6!
    p = __builtin_fma(p, r, 8.3333333333333332e-03);   // 1/5!
    p = __builtin_fma(p, r, 4.1666666666666664e-02);   // 1/4!
    p = __builtin_fma(p, r, 1.6666666666666666e-01);   // 1/3!
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    p = __builtin_fma(p, r, 1.0);
    return __builtin_ldexp(p, (int)k);
}
// fp32: v_exp_f32 (2^x) exists in hardware
__device__ __forceinline__ float exp_nonpos(float x) { return __expf(fmaxf(x, -100.0f)); }

// Table-driven variant for the HBM-bound kernel build, where the exp above is what the VALU spends its time on
// (23 of the 82 instructions per pair of entries; the kernel runs at the post-idle shader clock and every VALU
// instruction shows):   sf2 exp(-a w),  w >= 0,  a = 1/2 (squared exponential of r^2) or 1 (Matern's exp(-s5)).
//   k = rint(-a w 512/ln2)                (round-to-integer by adding 1.5 2^52: k sits in the low mantissa bits)
//   r = -a w - k ln2/512                  (|r| <= ln2/1024 = 6.8e-4; Cody-Waite split, k hi exact)
//   sf2 exp = 2^(k >> 9) * TAB[k & 511] * (1 + r + r^2/2 + r^3/6 + r^4/24)      truncation r^5/120 < 1.3e-18
// TAB[j] = sf2 2^(j/512) lives in LDS (4 KiB, filled per workgroup from a 512-entry device table of 2^(j/512)).
// 15 VALU instructions instead of 23; <= 2.5 ulp.
constexpr int KB_LDS_MAXD = 32;     // generic-d kernel build / gradient reduction: point tiles are staged in LDS up to this many dimensions
constexpr int EXP_TAB = 512;
template <bool HALF>
__device__ __forceinline__ double exp_tab(double w, const double* __restrict__ tab) {
    constexpr double A = HALF ? 0.5 : 1.0;
    constexpr double S = 738.6598609351493;                  // 512 / ln 2
    constexpr double C_HI = 0.0013538030862036976;           // ln2 / 512, upper 31 bits (0x1.62e42fecp-10)
    constexpr double C_LO = 8.274455792596258e-13;
    constexpr double MAGIC = 6755399441055744.0;             // 1.5 * 2^52
    w = fmin(w, 1600.0 / A);                                 // exp(-800) = 0 in fp64: keeps k inside the int range
    const double t = __builtin_fma(w, -A * S, MAGIC);
    const double kd = t - MAGIC;
    double r = __builtin_fma(w, -A, kd * -C_HI);
    r = __builtin_fma(kd, -C_LO, r);
    double p = __builtin_fma(4.1666666666666664e-02, r, 1.6666666666666666e-01);
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    p = __builtin_fma(p, r, 1.0);
    const int ki = __double2loint(t);
    return __builtin_ldexp(tab[ki & (EXP_TAB - 1)] * p, ki >> 9);
}
// table units: sf2 exp(-w ln2/512) = sf2 2^(-w/512); kbuild_mfma_kernel scales the coordinates so that its accumulator IS w
constexpr double EXP_U_PER_ARG = 738.6598609351493;          // 512 / ln 2: w = EXP_U_PER_ARG * (the exponent's magnitude)
constexpr double EXP_COORD_SCALE_SE = 19.217958540583197;    // sqrt(512 / (2 ln 2)): coordinates -> sum of squares = w of exp(-r2/2)

// Per-type numerics and MFMA shape
template <typename T> struct Num;
template <> struct Num<double> {
    typedef d4 acc_t;
    typedef double2 pair_t;
    static constexpr int GK = 16;            // K per LDS stage of gemm_nt (16 KiB per operand tile)
    static __device__ __forceinline__ acc_t mfma(double a, double b, acc_t c) {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ int drow(int l4, int r) { return l4 + 4 * r; }
    // k index a lane group supplies in MFMA k-step kk such that accumulator register kk of a D-layout
    // tile can be fed straight back as the B operand (row drow(l4, kk) of that tile)
    static __device__ __forceinline__ int kidx(int kk, int l4) { return 4 * kk + l4; }
    static __device__ __forceinline__ double readlane(double v, int src) {
        int lo = __double2loint(v), hi = __double2hiint(v);
        lo = __builtin_amdgcn_readlane(lo, src);
        hi = __builtin_amdgcn_readlane(hi, src);
        return __hiloint2double(hi, lo);
    }
    static __device__ __forceinline__ double sqrt_(double x) { return __builtin_sqrt(x); }
    static __device__ __forceinline__ double rsqrt_(double x) { return rsqrt(x); }
    static __device__ __forceinline__ double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }
};
template <> struct Num<float> {
    typedef f4 acc_t;
    typedef float2 pair_t;
    static constexpr int GK = 32;
    static __device__ __forceinline__ acc_t mfma(float a, float b, acc_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ int drow(int l4, int r) { return 4 * l4 + r; }
    static __device__ __forceinline__ int kidx(int kk, int l4) { return 4 * l4 + kk; }
    static __device__ __forceinline__ float readlane(float v, int src) {
        return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
    }
    static __device__ __forceinline__ float sqrt_(float x) { return __builtin_sqrtf(x); }
    static __device__ __forceinline__ float rsqrt_(float x) { return rsqrtf(x); }
    // (__builtin_fma on floats silently promotes to fp64: three conversions per term)
    static __device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
};

// KT = 0: squared exponential  sf2 * exp(-r2/2)
// KT = 1: Matern-5/2           sf2 * (1 + s5 + 5 r2/3) exp(-s5),  s5 = sqrt(5 r2)
template <int KT, typename T>
__device__ __forceinline__ T kfun(T r2, T sf2) {
    if (KT == 0) {
        return sf2 * exp_nonpos((T)-0.5 * r2);
    } else {
        const T s5 = Num<T>::sqrt_((T)5.0 * r2);
        return sf2 * ((T)1.0 + s5 + (T)(5.0 / 3.0) * r2) * exp_nonpos(-s5);
    }
}

// ---------------------------------------------------------------------------------------------
// The general covariance form (KT = 2 instantiations; the reference takes ANY kernel[p, q], BGP:32 -- its own example is a
// constant plus a squared exponential, BGP:16):
//     k(p, q) = c + k1(p, q)  [ + or * k2(p, q) ],     k_t = sf_t^2 g_fam(r_t^2 [, alpha_t]),  r_t^2 = sum ((p_j - q_j) / l_tj)^2
// families: 0 squared exponential exp(-r2/2), 1 Matern-5/2, 2 Matern-3/2 (1 + s3) exp(-s3), s3 = sqrt(3 r2),
// 3 rational quadratic (1 + r2 / (2 alpha))^-alpha.  Each term has its own length scales (its own scaled copy of the
// inputs).  The two-family fast paths above (KT = 0 / 1, one term, no offset) stay as they are.
// ---------------------------------------------------------------------------------------------
struct KSpec {
    int fam1, fam2;     // family of term 1 / term 2
    int op;             // 0: one term, 1: k1 + k2, 2: k1 * k2
    int offset;         // 1: + c
};
constexpr int SP_SF2B = 5, SP_ALPHA1 = 6, SP_ALPHA2 = 7, SP_OFFSET = 8, SP_KXX = 9, SP_MFMA = 10;

// g_fam(r2) and  -2 dg/dr2  (the factor the length-scale derivative needs: dk/dl_j = sf2 (-2 dg/dr2) u_j^2 / l_j) and dg/dalpha
template <typename T>
__device__ __forceinline__ void kfamily(int fam, T r2, T alpha, T& g, T& m2dg, T& dga) {
    dga = (T)0;
    if (fam == 0) {
        g = exp_nonpos((T)-0.5 * r2);
        m2dg = g;
    } else if (fam == 1) {
        const T s5 = Num<T>::sqrt_((T)5.0 * r2), e = exp_nonpos(-s5);
        g = ((T)1.0 + s5 + (T)(5.0 / 3.0) * r2) * e;
        m2dg = (T)(5.0 / 3.0) * ((T)1.0 + s5) * e;
    } else if (fam == 2) {
        const T s3 = Num<T>::sqrt_((T)3.0 * r2), e = exp_nonpos(-s3);
        g = ((T)1.0 + s3) * e;
        m2dg = (T)3.0 * e;
    } else {
        const double q = (double)r2 / (2.0 * (double)alpha), l1p = log1p(q);
        const double gd = exp(-(double)alpha * l1p);
        g = (T)gd;
        m2dg = (T)(gd / (1.0 + q));
        dga = (T)(gd * (q / (1.0 + q) - l1p));
    }
}

// g_fam(r2) alone, for the kernel BUILD of the general form (round 6): what kfamily computes, minus what only the gradient needs and
// minus the slow library routes -- square roots by v_rsq + one Newton step (5 instructions instead of the IEEE expansion's 15;
// relative error ~4e-15), the rational quadratic's logarithm from a v_log_f32 seed corrected to second order on exp_nonpos
// (two exp_nonpos + ~10 instructions instead of the library's log1p + exp: ~150).  Direct-form rational quadratic d = 8 0.16 ->
// see profiles/r06_kbuild_family_table.txt.
__device__ __forceinline__ double kvalue(int fam, double r2, double alpha, double inv_alpha) {
    if (fam == 0) return exp_nonpos(-0.5 * r2);
    if (fam == 3) {
        const double q = r2 * (0.5 * inv_alpha), yq = 1.0 + q;
        const double x0 = (double)(__builtin_amdgcn_logf((float)yq) * 0.69314718f);
        const double dl = __builtin_fma(yq, exp_nonpos(-x0), -1.0);
        const double x1 = x0 + __builtin_fma(-0.5 * dl, dl, dl);
        return exp_nonpos(-alpha * x1);
    }
    const double u = fmax((fam == 1 ? 5.0 : 3.0) * r2, 1.0e-280);
    const double y = __builtin_amdgcn_rsq(u);
    const double e = __builtin_fma(-u * y, y, 1.0);
    const double s = u * __builtin_fma(0.5 * y, e, y);            // sqrt(u)
    const double ex = exp_nonpos(-s);
    return fam == 1 ? (1.0 + s + (1.0 / 3.0) * u) * ex : (1.0 + s) * ex;
}
__device__ __forceinline__ float kvalue(int fam, float r2, float alpha, float inv_alpha) {
    if (fam == 0) return __builtin_amdgcn_exp2f(-0.72134752f * r2);
    if (fam == 3) return __builtin_amdgcn_exp2f(-alpha * __builtin_amdgcn_logf(1.0f + r2 * (0.5f * inv_alpha)));
    const float u = fmaxf((fam == 1 ? 5.0f : 3.0f) * r2, 1e-30f);
    const float s = u * __builtin_amdgcn_rsqf(u);
    const float ex = __builtin_amdgcn_exp2f(s * -1.4426950408889634f);
    return fam == 1 ? (1.0f + s + (1.0f / 3.0f) * u) * ex : (1.0f + s) * ex;
}

// k(p, q) of the general form from the two squared scaled distances; sp = the slot's scalars
template <typename T>
__device__ __forceinline__ T kgeneral(const KSpec& ks, T r2a, T r2b, const double* __restrict__ sp, T inv_a1, T inv_a2) {
    T k = (T)sp[0] * kvalue(ks.fam1, r2a, (T)sp[SP_ALPHA1], inv_a1);
    if (ks.op != 0) {
        const T k2 = (T)sp[SP_SF2B] * kvalue(ks.fam2, r2b, (T)sp[SP_ALPHA2], inv_a2);
        k = (ks.op == 1) ? k + k2 : k * k2;
    }
    return ks.offset ? k + (T)sp[SP_OFFSET] : k;
}

// xs[slot][dd][i] = X[dd][i] * inv_ell[slot][dd]      (Xt is the transposed copy [d][npad])
template <typename T>
__global__ void k_scale(const T* __restrict__ Xt, T* __restrict__ xs, const double* __restrict__ inv_ell,
                        int d, int npad) {
    const int slot = blockIdx.y;
    const long total = (long)d * npad;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long)gridDim.x * blockDim.x) {
        const int dd = (int)(idx / npad);
        xs[(long)slot * total + idx] = (T)((double)Xt[idx] * inv_ell[slot * d + dd]);
    }
}

// Same scaling with the hyper-parameters of the call passed BY VALUE (kernel arguments): for the
// latency path (a few thetas per call) this replaces two host-to-device copies and a memset -- block
// (0,0) also leaves inv_ell / the per-slot scalars in device memory for the kernels that follow and
// clears the info words.  v = [nslots*d inverse length scales][nslots*SLOTP slot scalars].
constexpr int THETA_PACK = 320;
struct ThetaPack { double v[THETA_PACK]; };
template <typename T>
__global__ void k_scale_theta(const T* __restrict__ Xt, T* __restrict__ xs, ThetaPack tp, double* __restrict__ inv_ell_out,
                              double* __restrict__ slotp_out, int* __restrict__ info_out, int d, int npad, int nslots) {
    const int slot = blockIdx.y;
    const long total = (long)d * npad;
    if (blockIdx.x == 0 && slot == 0) {
        for (int k = threadIdx.x; k < nslots * d; k += blockDim.x) inv_ell_out[k] = tp.v[k];
        for (int k = threadIdx.x; k < nslots * SLOTP; k += blockDim.x) slotp_out[k] = tp.v[nslots * d + k];
        for (int k = threadIdx.x; k < nslots; k += blockDim.x) info_out[k] = 0;
    }
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long)gridDim.x * blockDim.x) {
        const int dd = (int)(idx / npad);
        xs[(long)slot * total + idx] = (T)((double)Xt[idx] * tp.v[slot * d + dd]);
    }
}

// Decode linear index t of the lower triangle (incl. diagonal) of an n x n tile grid, enumerated
// column by column: column c holds rows c..n-1.
__device__ __forceinline__ void tri_decode(int t, int n, int& ti, int& tj) {
    const double b = 2.0 * n + 1.0;
    int c = (int)((b - __builtin_sqrt(b * b - 8.0 * (double)t)) * 0.5);
    if (c < 0) c = 0;
    if (c > n - 1) c = n - 1;
    // offset(c) = c*n - c(c-1)/2
    while (c > 0 && (long)c * n - (long)c * (c - 1) / 2 > t) --c;
    while ((long)(c + 1) * n - (long)(c + 1) * c / 2 <= t) ++c;
    tj = c;
    ti = c + (t - (int)((long)c * n - (long)c * (c - 1) / 2));
}

template <typename T>
struct KBuildArgs {
    T* out;                 // mode 0: tiled workspace base (slot 0); mode 1: column-major block
    long ld;                // mode 1: leading dimension (elements)
    long bstride;           // elements between slots
    const T* xi;            // scaled I-operand points [slot][D][npad_i]  (rows of the output)
    const T* xj;            // scaled J-operand points [slot][D][npad_j]  (columns of the output)
    long xi_bstride, xj_bstride;
    int npad_i, npad_j;     // padded point counts (multiples of 128)
    int n_i, n_j;           // true point counts
    const T* y;             // [npad_j] outputs (mode 0 only)
    const double* slotp;    // [slot][SLOTP]
    int d;                  // runtime dimension (used when D == 0)
    int mode;               // 0: train x train (lower-tri tiles, nugget, identity padding, rhs rows)
                            // 1: cross  (rectangular tiles, zero padding)
    int nt_i, nt_j;         // tile counts; mode 0: nt_i = nt_j + 1 (extra rhs block-row)
    const double* exp2tab;  // [EXP_TAB] 2^(j/512) (fp64 build only)
    // Point-dependent nugget / mean (BGP:37 nugget[points[[i]]], BGP:300 meanFunction /@ inputData): values the host
    // evaluated for this call's theta, [slot][pw_bstride]; null = the constant forms sn^2 / mu of the slot scalars
    const T* pw_nug; const T* pw_mean; long pw_bstride;
    // general form (KT = 2): the inputs scaled by the SECOND term's length scales (null for one term) and the spec
    const T* xi2; const T* xj2;
    KSpec ks;
    int own_panel, own_world, own_rank;   // own_world > 0 (multi-GPU 1-D block-cyclic layout): build
                            // only tile columns whose outer panel (tj / own_panel) belongs to own_rank;
                            // the rhs x rhs corner tile belongs to rank 0
    int t0;                 // mode 0: first tile (column-major packed index) of this launch -- the build of a look-ahead
                            // factorisation is split into "tile columns of panel 0" and "the rest" (panel 0 is factored
                            // under the rest of the build)
    const long* adj;        // own_world > 0 and the rank keeps ONLY its own panels (compact storage): adj[q] = tiles to add
                            // to the dense tile index of any tile of outer panel q (index nt_j / .. see panel_slot);
                            // null: the dense packed layout
    const double* cp; int ncp;   // KT = 3 (run-time compiled covariance function): its hyper-parameters, [slot][ncp]
    int mfma_skip;          // 1: slots whose scalar [SP_MFMA] is set belong to kbuild_mfma_kernel's launch -- leave them alone
};

// KT = 3: the covariance function is source text the caller handed to gphip_create_custom (the reference takes ANY
// `kernel @@ points[[{i,j}]]`, BGP:29-33), compiled at run time into this header's kernel build.  X / Y are accessors of the
// two points' coordinates (LDS tiles or, beyond KB_LDS_MAXD dimensions, global memory), Pp the function's hyper-parameters.
template <typename T>
struct PointRef {
    const T* base; long stride;
    __device__ __forceinline__ T operator()(int k) const { return base[(long)k * stride]; }
};
// T: the arithmetic type the body computes in -- S itself for the kernel build, Dual<S, NP> (gp_dual.h) for the gradient
#ifdef GP_CUSTOM_KERNEL
template <typename T, typename S>
__device__ T gphip_custom_k(PointRef<S> X, PointRef<S> Y, const double* __restrict__ Pp, int D);      // defined by the generated source
#else
template <typename T, typename S>
__device__ __forceinline__ T gphip_custom_k(PointRef<S>, PointRef<S>, const double*, int) { return (T)0; }   // never instantiated offline
#endif

// One 128x128 tile per workgroup (4 waves).  Wave w owns 32 output columns; lane owns 2 adjacent
// rows (fp64: every store is a 16-byte dwordx4 and a wave writes one full 1 KiB column segment).
// The J-side points come from LDS as wave-uniform broadcasts; the I-side points live in registers.
template <typename T, int D, int KT>
__global__ __launch_bounds__(256) void kbuild_kernel(KBuildArgs<T> a) {
    extern __shared__ double lds_raw[];
    T* lds = reinterpret_cast<T*>(lds_raw);   // xj tile [d][128] (+ xi tile [d][128] when D == 0)
    typedef typename Num<T>::pair_t pair_t;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slot = blockIdx.y;
    int ti, tj;
    if (a.mode == 0) {
        tri_decode(blockIdx.x + a.t0, a.nt_i, ti, tj);
    } else {
        ti = blockIdx.x % a.nt_i;
        tj = blockIdx.x / a.nt_i;
    }
    if (a.own_world > 0) {
        const int owner = (tj == a.nt_j) ? 0 : (tj / a.own_panel) % a.own_world;
        if (owner != a.own_rank) return;
    }
    const double* sp = a.slotp + (long)slot * SLOTP;
    if (a.mfma_skip && sp[SP_MFMA] != 0.0) return;
    const T sf2 = (T)sp[0], sn2 = (T)sp[1], mu = (T)sp[2];
    const T inv_a1 = (T)(1.0 / sp[SP_ALPHA1]), inv_a2 = (T)(1.0 / sp[SP_ALPHA2]);      // (general form, rational quadratic terms)
    // mode 0 writes one whole tile of the packed workspace (128 KiB contiguous in fp64); mode 1 a tile of a
    // column-major block
    const long ldo = (a.mode == 0) ? (long)TB : a.ld;
    T* out = a.out + (long)slot * a.bstride +
             ((a.mode == 0) ? (tile_index(ti, tj, a.nt_i) + (a.adj ? a.adj[panel_slot(tj, a.nt_j, a.own_panel)] : 0l)) * TS
                            : (long)tj * TB * a.ld + (long)ti * TB);
    const int r0 = 2 * lane;

    if (a.mode == 0 && ti == a.nt_i - 1) {      // right-hand-side block-row: row 0 = r^T, rest 0
        for (int jj = wave * 32; jj < wave * 32 + 32; ++jj) {
            const int gj = tj * TB + jj;
            pair_t v;
            v.x = (T)0;
            v.y = (T)0;
            if (lane == 0 && tj < a.nt_j && gj < a.n_j)
                v.x = a.y[gj] - (a.pw_mean ? a.pw_mean[(long)slot * a.pw_bstride + gj] : mu);
            *reinterpret_cast<pair_t*>(out + (long)jj * ldo + r0) = v;
        }
        return;
    }

    const int d = (D > 0) ? D : GP_DIM(a.d);
    const T* xjg = a.xj + (long)slot * a.xj_bstride + (long)tj * TB;
    const T* xig = a.xi + (long)slot * a.xi_bstride + (long)ti * TB;
    T* xjs = lds;
    T* xis = lds + d * TB;
    // general form (KT = 2, D = 0): the second term's scaled points behind the first term's
    T* xjs2 = lds + 2 * d * TB;
    T* xis2 = lds + 3 * d * TB;
    const bool two = KT == 2 && a.ks.op != 0;
    // Input dimensions beyond KB_LDS_MAXD (generic-d instantiations only): the point tiles no longer fit in LDS next to a
    // second workgroup, so the inner loop reads the scaled coordinates straight from global memory (the J-side value is one
    // wave-uniform 8-byte load per dimension and column, the I-side pair a coalesced 16-byte load; both tiles stay L1 / L2
    // resident).  Slower per entry, but the reference takes points of ANY dimension (BGP:29-43) and for such d the
    // factorisation dominates anyway.
    const bool glb = D == 0 && d > KB_LDS_MAXD;
    // fp64: sf2 2^(j/512) table behind the point tiles (see exp_tab)
    double* etab = lds_raw + (glb ? 0 : ((D > 0) ? D : 2 * d) * TB);
    if (sizeof(T) == 8 && KT < 2)
        for (int idx = tid; idx < EXP_TAB; idx += 256) etab[idx] = sp[0] * a.exp2tab[idx];
    // KT = 3: the function's hyper-parameters behind the point tiles.  Read from LDS (never written inside the column loop, and
    // not aliased by the tile stores) their loads -- and what the function computes from them alone, e.g. 1 / l_k -- are
    // loop invariant for the compiler; read through the global pointer every column would fetch and divide again.
    double* cpl = lds_raw + (glb ? 0 : (size_t)2 * d * TB * sizeof(T) / sizeof(double));
    if constexpr (KT == 3)
        for (int idx = tid; idx < a.ncp; idx += 256) cpl[idx] = a.cp[(long)slot * a.ncp + idx];
    // fp32 fast path below: sum of squares = r2 log2(e) / 2 (SE) or 5 r2 (Matern-5/2)
    constexpr bool F32FAST = sizeof(T) == 4 && D > 0 && KT < 2;
    constexpr float CS32 = KT == 0 ? 0.84932180028801904f /* sqrt(log2(e) / 2) */ : 2.2360679774997896f /* sqrt 5 */;
    const T cscale = F32FAST ? (T)CS32 : (T)1;
    for (int idx = tid; idx < (glb ? 0 : d * TB); idx += 256) {
        const int dd = idx >> 7, c = idx & 127;
        xjs[idx] = F32FAST ? xjg[(long)dd * a.npad_j + c] * cscale : xjg[(long)dd * a.npad_j + c];
        if (D == 0) xis[idx] = xig[(long)dd * a.npad_i + c];
        if (KT == 2 && two) {
            xjs2[idx] = a.xj2[(long)slot * a.xj_bstride + (long)tj * TB + (long)dd * a.npad_j + c];
            xis2[idx] = a.xi2[(long)slot * a.xi_bstride + (long)ti * TB + (long)dd * a.npad_i + c];
        }
    }
    T xa[D > 0 ? D : 1], xb[D > 0 ? D : 1];
    if (D > 0) {
#pragma unroll
        for (int dd = 0; dd < D; ++dd) {
            const pair_t v = *reinterpret_cast<const pair_t*>(xig + (long)dd * a.npad_i + r0);
            xa[dd] = v.x;
            xb[dd] = v.y;
        }
    }
    __syncthreads();

    const bool edge = (a.mode == 0) ? (ti == tj || (ti + 1) * TB > a.n_i)
                                    : ((ti + 1) * TB > a.n_i || (tj + 1) * TB > a.n_j);
    if constexpr (F32FAST) {
        // fp32 (round 4; the build is VALU bound -- 16 dimensions, a square root and an exponential per 4-byte entry): a lane
        // owns FOUR adjacent rows of one column, a half-wave one column, so every store is a 16-byte dwordx4, every J-side LDS
        // broadcast serves four entries and the whole distance loop is v_pk_add_f32 / v_pk_fma_f32 on row pairs.  The
        // coordinates are rescaled once per tile so that the accumulated sum of squares is directly what the kernel function
        // needs: SE  sf2 2^(-acc) (one v_exp_f32, its negation is an input modifier);  Matern-5/2  acc = 5 r2,
        // s5 = acc * rsq(acc) (v_rsq_f32, 1 ulp; the IEEE sqrtf expansion was 14 instructions per entry),
        // sf2 (1 + s5 + acc / 3) 2^(-s5 log2 e).
        constexpr float CS = CS32;
        const int half = lane >> 5, r4 = 4 * (lane & 31);
        typedef float v2f __attribute__((ext_vector_type(2)));     // row pairs: v_pk_add_f32 / v_pk_fma_f32
        v2f xr[D][2];
#pragma unroll
        for (int dd = 0; dd < D; ++dd) {
            const f4 v = *reinterpret_cast<const f4*>(xig + (long)dd * a.npad_i + r4);
            xr[dd][0] = (v2f){v[0] * CS, v[1] * CS};
            xr[dd][1] = (v2f){v[2] * CS, v[3] * CS};
        }
        const int gi4 = ti * TB + r4;
        for (int jj = 2 * wave + half; jj < TB; jj += 8) {
            v2f acc2[2] = {(v2f){0.f, 0.f}, (v2f){0.f, 0.f}};
#pragma unroll
            for (int dd = 0; dd < D; ++dd) {
                const float xj1 = xjs[dd * TB + jj];
                const v2f xjv = (v2f){xj1, xj1};
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const v2f dl = xr[dd][r] - xjv;
                    acc2[r] = __builtin_elementwise_fma(dl, dl, acc2[r]);
                }
            }
            const float acc[4] = {acc2[0][0], acc2[0][1], acc2[1][0], acc2[1][1]};
            f4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (KT == 0) {
                    v[r] = sf2 * __builtin_amdgcn_exp2f(-acc[r]);
                } else {
                    const float q = fmaxf(acc[r], 1e-30f);
                    const float s5 = q * __builtin_amdgcn_rsqf(q);
                    v[r] = sf2 * (1.0f + s5 + q * (1.0f / 3.0f)) * __builtin_amdgcn_exp2f(s5 * -1.4426950408889634f);
                }
            }
            if (edge) {
                const int gj = tj * TB + jj;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int gi = gi4 + r;
                    if (a.mode == 0) {
                        if (gi == gj) v[r] += a.pw_nug ? a.pw_nug[(long)slot * a.pw_bstride + gj] : sn2;
                        if (gj >= a.n_j || gi >= a.n_i) v[r] = (gi == gj) ? 1.f : 0.f;          // identity pad
                    } else if (gj >= a.n_j || gi >= a.n_i) {
                        v[r] = 0.f;
                    }
                }
            }
            *reinterpret_cast<f4*>(out + (long)jj * ldo + r4) = v;
        }
        return;
    }
    const int gi = ti * TB + r0;
    // columns of the tile dealt round-robin to the four waves: at any moment the workgroup writes four ADJACENT 1 KiB
    // column segments (one contiguous 4 KiB of the tile)
    // everything after the first term's squared distances of column jj: the kernel function, nugget / padding, the store
    auto finish = [&](int jj, T ra, T rb) {
        T va, vb;
        if constexpr (KT == 3) {
            const double* cp = cpl;
            const PointRef<T> Yj{glb ? xjg + jj : xjs + jj, glb ? (long)a.npad_j : (long)TB};
            const PointRef<T> Xa{glb ? xig + r0 : xis + r0, glb ? (long)a.npad_i : (long)TB};
            const PointRef<T> Xb{Xa.base + 1, Xa.stride};
            va = gphip_custom_k<T, T>(Xa, Yj, cp, d);
            vb = gphip_custom_k<T, T>(Xb, Yj, cp, d);
        } else if constexpr (KT == 2) {
            T ra2 = (T)0, rb2 = (T)0;
            if (two && !glb)
                for (int dd = 0; dd < d; ++dd) {
                    const T xjv = xjs2[dd * TB + jj];
                    const T da = xis2[dd * TB + r0] - xjv, db = xis2[dd * TB + r0 + 1] - xjv;
                    ra2 = Num<T>::fma_(da, da, ra2);
                    rb2 = Num<T>::fma_(db, db, rb2);
                }
            if (two && glb) {
                const T* xj2g = a.xj2 + (long)slot * a.xj_bstride + (long)tj * TB;
                const T* xi2g = a.xi2 + (long)slot * a.xi_bstride + (long)ti * TB;
                for (int dd = 0; dd < d; ++dd) {
                    const T xjv = xj2g[(long)dd * a.npad_j + jj];
                    const pair_t xi = *reinterpret_cast<const pair_t*>(xi2g + (long)dd * a.npad_i + r0);
                    const T da = xi.x - xjv, db = xi.y - xjv;
                    ra2 = Num<T>::fma_(da, da, ra2);
                    rb2 = Num<T>::fma_(db, db, rb2);
                }
            }
            va = kgeneral<T>(a.ks, ra, ra2, sp, inv_a1, inv_a2);
            vb = kgeneral<T>(a.ks, rb, rb2, sp, inv_a1, inv_a2);
        } else if constexpr (sizeof(T) == 8) {
            if (KT == 0) {
                va = exp_tab<true>(ra, etab);
                vb = exp_tab<true>(rb, etab);
            } else {
                const double sa = __builtin_sqrt(5.0 * ra), sb = __builtin_sqrt(5.0 * rb);
                va = (1.0 + sa + (5.0 / 3.0) * ra) * exp_tab<false>(sa, etab);
                vb = (1.0 + sb + (5.0 / 3.0) * rb) * exp_tab<false>(sb, etab);
            }
        } else {
            va = kfun<KT, T>(ra, sf2);
            vb = kfun<KT, T>(rb, sf2);
        }
        if (edge) {
            const int gj = tj * TB + jj;
            if (a.mode == 0) {
                if (gi == gj || gi + 1 == gj) {
                    const T nug = a.pw_nug ? a.pw_nug[(long)slot * a.pw_bstride + gj] : sn2;
                    if (gi == gj) va += nug;
                    else vb += nug;
                }
                if (gj >= a.n_j || gi >= a.n_i) va = (gi == gj) ? (T)1 : (T)0;       // identity pad
                if (gj >= a.n_j || gi + 1 >= a.n_i) vb = (gi + 1 == gj) ? (T)1 : (T)0;
            } else {
                if (gj >= a.n_j || gi >= a.n_i) va = (T)0;
                if (gj >= a.n_j || gi + 1 >= a.n_i) vb = (T)0;
            }
        }
        pair_t v;
        v.x = va;
        v.y = vb;
        *reinterpret_cast<pair_t*>(out + (long)jj * ldo + r0) = v;
    };
    if constexpr (D == 0 && KT != 3) {
        if (!glb) {
            // generic d, points in LDS (round 6): FOUR columns per pass, so that the I-side pair of a dimension is read from LDS
            // once per four columns instead of once per column -- 1.25 LDS reads per dimension and column instead of 2 (the
            // loop is LDS-issue bound from d ~ 12 on: SE-ARD d = 24 ran at 0.15 of the HBM rate)
            for (int j0 = wave; j0 < TB; j0 += 16) {
                T ra4[4] = {(T)0, (T)0, (T)0, (T)0}, rb4[4] = {(T)0, (T)0, (T)0, (T)0};
                for (int dd = 0; dd < d; ++dd) {
                    const pair_t xi = *reinterpret_cast<const pair_t*>(xis + dd * TB + r0);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const T xjv = xjs[dd * TB + j0 + 4 * c];
                        const T da = xi.x - xjv, db = xi.y - xjv;
                        ra4[c] = Num<T>::fma_(da, da, ra4[c]);
                        rb4[c] = Num<T>::fma_(db, db, rb4[c]);
                    }
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) finish(j0 + 4 * c, ra4[c], rb4[c]);
            }
            return;
        }
    }
    for (int jj = wave; jj < TB; jj += 4) {
        T ra = (T)0, rb = (T)0;
        if constexpr (KT == 3) {
            // (the caller's function sees the points themselves, not a distance)
        } else if (D > 0) {
#pragma unroll
            for (int dd = 0; dd < D; ++dd) {
                const T xjv = xjs[dd * TB + jj];
                const T da = xa[dd] - xjv, db = xb[dd] - xjv;
                ra = Num<T>::fma_(da, da, ra);
                rb = Num<T>::fma_(db, db, rb);
            }
        } else if (!glb) {
            for (int dd = 0; dd < d; ++dd) {
                const T xjv = xjs[dd * TB + jj];
                const T da = xis[dd * TB + r0] - xjv, db = xis[dd * TB + r0 + 1] - xjv;
                ra = Num<T>::fma_(da, da, ra);
                rb = Num<T>::fma_(db, db, rb);
            }
        } else {
            for (int dd = 0; dd < d; ++dd) {
                const T xjv = xjg[(long)dd * a.npad_j + jj];
                const pair_t xi = *reinterpret_cast<const pair_t*>(xig + (long)dd * a.npad_i + r0);
                const T da = xi.x - xjv, db = xi.y - xjv;
                ra = Num<T>::fma_(da, da, ra);
                rb = Num<T>::fma_(db, db, rb);
            }
        }
        finish(jj, ra, rb);
    }
}

#ifdef GP_CUSTOM_KERNEL
// k(x_i, x_i) of the points [d][npad] under the slot's hyper-parameters -> out[slot][ostride] (fp64): the prior variance at
// the test points (BGP:110-115 kappa; a function of the point for a non-stationary covariance function)
template <typename T>
__global__ void custom_diag_kernel(const T* __restrict__ x, long x_bstride, int npad, int n, int d, const double* __restrict__ cp,
                                   int ncp, double* __restrict__ out, long ostride) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, slot = blockIdx.y;
    if (i >= n) return;
    const PointRef<T> X{x + (long)slot * x_bstride + i, (long)npad};
    out[(long)slot * ostride + i] = (double)gphip_custom_k<T, T>(X, X, cp + (long)slot * ncp, GP_DIM(d));
}
// Per slot: the largest prior variance over the training points scales the pivot tolerance of the factorisation (the
// named kernels know k(x, x) = sf^2 on the host; here only the device can evaluate the function).  The host left the
// relative tolerance in sp[3] and the nugget's scale in sp[SP_SF2B]; one workgroup per slot.
template <typename T>
__global__ __launch_bounds__(256) void custom_prep_kernel(const T* __restrict__ x, int npad, int n, int d, const double* __restrict__ cp,
                                                          int ncp, double* __restrict__ slotp) {
    __shared__ double red[256];
    const int slot = blockIdx.x;
    double m = 0.0;
    bool bad = false;
    for (int i = threadIdx.x; i < n; i += 256) {
        const PointRef<T> X{x + i, (long)npad};
        const double v = (double)gphip_custom_k<T, T>(X, X, cp + (long)slot * ncp, GP_DIM(d));
        if (!(fabs(v) <= 1.0e300)) bad = true;
        m = fmax(m, fabs(v));
    }
    red[threadIdx.x] = bad ? __builtin_nan("") : m;
    __syncthreads();
    for (int s2 = 128; s2 > 0; s2 >>= 1) {
        if (threadIdx.x < s2) {
            const double o = red[threadIdx.x + s2], mine = red[threadIdx.x];
            red[threadIdx.x] = (o != o || mine != mine) ? __builtin_nan("") : fmax(o, mine);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double* sp = slotp + (long)slot * SLOTP;
        double kmax = red[0];
        if (kmax != kmax) { kmax = 1.0; sp[4] = 1.0; }         // (NaN / inf prior variance: the evaluation's verdict will be NaN)
        sp[0] = kmax; sp[SP_KXX] = kmax;
        sp[3] = sp[3] * (kmax + sp[SP_SF2B]);
    }
}
#endif

// arguments of the gradient reductions (grad_reduce_*_kernel below the region; custom_grad_kernel here)
template <typename T>
struct GradArgs {
    const T* Kinv; long ldv;        // row block: Kinv(t, j) at Kinv[j*ldv + t], t = row c0+t of K^-1
    const T* alpha;                 // [npad]
    const T* xs;                    // scaled inputs [d][npad]
    int npad, n, c0, mc, d;
    int tri;                        // 1: Kinv holds the lower triangle only (tile rows >= tile columns): skip the
                                    //    upper tiles and count the strictly lower ones twice (everything is symmetric)
    const double* slotp;
    double* gacc;                   // [d + 2]; general form: [2 d + 6], see grad_reduce_general_kernel
    const T* xs2;                   // general form: inputs scaled by the second term's length scales (or null)
    KSpec ks;
    int d0;                         // general form, more than KB_LDS_MAXD dimensions: this launch accumulates the length-scale
                                    // derivatives of dimensions [d0, d0 + 32) only (and the scalar ones when d0 == 0)
    double* gpart;                  // [workgroups][np] per-workgroup sums (grad_finish_kernel adds them into gacc), or null: atomics on gacc
    int np, ws_off;                 // accumulator slots per workgroup; where the [4 waves][np] staging area starts in LDS (doubles)
    const T* beta;                  // [npad] or null.  Null: w = alpha_g alpha_j - Kinv_gj (the log-likelihood).  Set: the leave-one-out
                                    // pseudo-likelihood, w = alpha_g beta_j + beta_g alpha_j - Kinv_gj with Kinv holding M (gp_loo.h)
    const T* xr; const T* xr2;      // null: the rows are training points as the columns are (square).  Set: a RECTANGLE -- the rows are
    int npad_r;                     // the mc points [d][npad_r] of xr (xr2: scaled by term 2), the columns the training points; the weight
                                    // is w = -Kinv(t, j) alone (no alpha term), no entry counts as a diagonal one and tri does not apply
    int diag; double wdiag;         // run-time compiled function only: 1 = no matrix at all, sum_t wdiag dk(x_t, x_t)/dp over the rows
};

// the row points of a gradient reduction and their leading dimension (GradArgs::xr)
template <typename T> __device__ __forceinline__ const T* grad_row_points(const GradArgs<T>& a) { return a.xr ? a.xr : a.xs; }
template <typename T> __device__ __forceinline__ const T* grad_row_points2(const GradArgs<T>& a) { return a.xr ? a.xr2 : a.xs2; }
template <typename T> __device__ __forceinline__ int grad_row_ld(const GradArgs<T>& a) { return a.xr ? a.npad_r : a.npad; }

// the weight of entry (g, j) in a gradient reduction: see GradArgs::beta (bg / beta[j] are read only when beta is set)
template <typename T>
__device__ __forceinline__ double grad_weight(const GradArgs<T>& a, double wt, T ag, T aj, double bg, int j, double kinv) {
    if (a.beta) return wt * ((double)ag * (double)a.beta[j] + bg * (double)aj - kinv);
    return wt * ((double)ag * (double)aj - kinv);
}

// How gradient accumulators leave a workgroup (round 6).  Every wave used to add its wave-reduced sums to gacc with atomics:
// thousands of waves queued on a dozen addresses (N = 8192: 1 ms of a 12.5 ms gradient call) and the sums were not bit-repeatable.
// Now every wave parks its sums in LDS, the workgroup adds the four in a fixed order and stores row `wg` of gpart; grad_finish_kernel
// adds the rows in a fixed order.  gpart == null (more slots than the staging area takes): the atomics.
struct GradEmit {
    double* ws; double* row; double* gacc; int np, tid;
    template <typename A>
    __device__ GradEmit(const A& a, double* lds_raw, int tid_) : ws(a.gpart ? lds_raw + a.ws_off : nullptr),
        row(a.gpart ? a.gpart + ((long)blockIdx.y * gridDim.x + blockIdx.x) * a.np : nullptr), gacc(a.gacc), np(a.np), tid(tid_) {
        if (ws) for (int p = tid; p < 4 * np; p += 256) ws[p] = 0.0;           // (the kernel's own barrier after its LDS loads covers this)
    }
    __device__ void skip() const { if (row) for (int p = tid; p < np; p += 256) row[p] = 0.0; }      // a workgroup with no tile
    __device__ void put(double v, int p) const {                                                      // all lanes of all waves
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if ((tid & 63) == 0) { if (ws) ws[(tid >> 6) * np + p] = v; else atomicAdd(gacc + p, v); }
    }
    __device__ void finish() const {
        if (!ws) return;
        __syncthreads();
        for (int p = tid; p < np; p += 256) row[p] = (ws[p] + ws[np + p]) + (ws[2 * np + p] + ws[3 * np + p]);
    }
};

#if defined(GP_CUSTOM_KERNEL) && defined(GP_CUSTOM_GRAD)
// Gradient reduction for a run-time compiled covariance function: the caller's text instantiated with the forward-mode type
// Dual<T, GP_NCP> (gp_dual.h), so that every entry comes with its derivatives in the function's GP_NCP hyper-parameters:
//   gacc[m]      += w (dk/dp_m)(x_g, x_j),  m < ncp        -> dl/dp_m = 1/2 gacc[m]
//   gacc[ncp]    += w_gg                                    -> dl/dsn  = gacc[ncp] sn
// with w = wt (alpha_g alpha_j - Kinv_gj) exactly as grad_reduce_kernel.  One 128 x 128 tile per workgroup, thread = one
// row x 64 columns; the column points sit in LDS up to KB_LDS_MAXD dimensions, beyond that both points come from global memory.
template <typename T>
__global__ __launch_bounds__(256) void custom_grad_kernel(GradArgs<T> a, const double* __restrict__ cp, int ncp) {
    extern __shared__ double lds_raw[];
    typedef Dual<T, GP_NCP> dual_t;
    const int d = GP_DIM(a.d);
    const bool glb = d > KB_LDS_MAXD;
    T* xjs = reinterpret_cast<T*>(lds_raw);      // [d][128] column points (when they fit), then alpha_j [128]
    T* aj = xjs + (glb ? 0 : d * TB);
    const int tid = threadIdx.x, row = tid & 127, half = tid >> 7;
    const int ti = blockIdx.x, tj = blockIdx.y;
    const GradEmit out(a, lds_raw, tid);
    if (a.tri && tj > ti) { out.skip(); return; }
    const double wt = (a.tri && tj < ti) ? 2.0 : 1.0;
    const int t = ti * TB + row, g = a.c0 + t;
    for (int idx = tid; idx < (glb ? 0 : d * TB); idx += 256) xjs[idx] = a.xs[(long)(idx >> 7) * a.npad + tj * TB + (idx & 127)];
    if (tid < TB) aj[tid] = a.alpha[tj * TB + tid];
    double acc[GP_NCP];
#pragma unroll
    for (int m = 0; m < GP_NCP; ++m) acc[m] = 0.0;
    double acc_dg = 0.0;
    const bool rect = a.xr != nullptr;
    const T ag = (t < a.mc && !rect) ? a.alpha[g] : (T)0;
    const double bg = (a.beta && t < a.mc) ? (double)a.beta[g] : 0.0;
    __syncthreads();
    if (t < a.mc && (rect || g < a.n)) {
        const PointRef<T> Xg{grad_row_points(a) + g, (long)grad_row_ld(a)};
        if (a.diag && half == 0) {                 // the rows' own k(x_t, x_t) only: one thread of the two that share a row
            const dual_t k = gphip_custom_k<dual_t, T>(Xg, Xg, cp, d);
#pragma unroll
            for (int m = 0; m < GP_NCP; ++m) acc[m] = a.wdiag * (double)k.g[m];
        }
        for (int jj = half * 64; jj < (a.diag ? 0 : half * 64 + 64); ++jj) {
            const int j = tj * TB + jj;
            if (j >= a.n) break;
            const PointRef<T> Yj{glb ? a.xs + j : xjs + jj, glb ? (long)a.npad : (long)TB};
            const dual_t k = gphip_custom_k<dual_t, T>(Xg, Yj, cp, d);
            const double w = grad_weight(a, wt, ag, aj[jj], bg, j, (double)a.Kinv[(long)j * a.ldv + t]);
#pragma unroll
            for (int m = 0; m < GP_NCP; ++m) acc[m] = __builtin_fma(w, (double)k.g[m], acc[m]);
            if (j == g && !rect) acc_dg += w;
        }
    }
#pragma unroll
    for (int m = 0; m < GP_NCP; ++m)
        if (m < ncp) out.put(acc[m], m);
    out.put(acc_dg, ncp);
    out.finish();
}
#endif
}  // namespace gphip
// [rtc-end]
namespace gphip {

// ---------------------------------------------------------------------------------------------
// kbuild_mfma_kernel: the tiles of kbuild_kernel (K1 / K7, BGP:29-43 and BGP:100-109) for the four named stationary
// families (KT = 0 SE, 1 Matern-5/2, 2 Matern-3/2, 3 rational quadratic; one term, no offset), with the distance loop moved
// from the vector ALU to the matrix pipe.
//
// kbuild_kernel spends 2 fp64 VALU instructions per input dimension and entry on sum ((p_k - q_k) / l_k)^2 and ~12 more
// on the exponential: at d = 8 the kernel is fp64-VALU bound (0.73 - 0.84 busy, MFMA pipe idle) and its time follows the
// shader clock instead of the HBM store rate.  Here
//     u(i, j) = |a_i|^2 + |b_j|^2 - 2 a_i . b_j,        a = s (x - c) / l  (points centred on c and scaled)
// is ONE accumulator initialisation (a VALU add) plus ceil(d / 4) v_mfma_*_16x16x4 per 16 x 16 entries: the J-side
// operand carries -2 b, the I-side operand a, the norms come from the same rounded coordinates.  s is chosen per
// kernel family so that u is directly the argument the epilogue needs (fp64 SE: the exponent in units of ln2 / 512,
// see exp_tab_u; Matern-5/2: 5 r^2; fp32 SE: r^2 log2(e) / 2).  Cost per entry is then independent of d.
//
// Accuracy: the rounding error of u is ~eps (|a|^2 + |b|^2) instead of ~eps r^2.  The host therefore (1) centres the
// points on the mid-range of the training inputs, (2) bounds sum_k (halfrange_k / l_k)^2 for every theta and hands a
// slot to this kernel only below a threshold (gphip.hip kbuild_mfma_ok; above it kbuild_kernel builds the slot as
// before -- slot scalar SP_MFMA says which).  At the headline configuration (x in [-1, 1)^8, l = 1) the bound is 8 and
// the two forms are equally accurate.  Rows / columns of duplicated points stay bit-identical (same inputs, same
// operation sequence), so an exactly singular K stays exactly singular.
//
// One 128 x 128 tile per workgroup (4 waves).  MFMA m <-> tile column j, n <-> tile row i: a lane (c = l & 15,
// g = l >> 4) ends up with NQ = 16 / sizeof(T) ADJACENT rows i0 + NQ c .. (one MFMA per row offset q) of the columns
// j0 + drow(g, r), r = 0..3 -- every store is 16 bytes and 16 lanes cover 256 contiguous bytes of a column.  A wave
// owns 32 columns (two 16-column blocks) and walks the tile's rows in blocks of 16 NQ.
// ---------------------------------------------------------------------------------------------
template <typename T>
struct KBuildMArgs {
    KBuildArgs<T> b;          // tile bookkeeping exactly as kbuild_kernel's (xi / xj / xi2 / xj2 / cp unused)
    const T* xri;             // RAW (unscaled) row points [d][npad_i]
    const T* xrj;             // RAW column points [d][npad_j]
    const double* inv_ell;    // [slot][d]
    const double* centre;     // [d]
};
constexpr int KM_LDP = 144;   // LDS row stride (elements) of the operand tiles: the four k rows a wave reads at once fall
                              // on disjoint banks (144 * 8 B = 288 dwords = 32 mod 64; 144 * 4 B = 16 mod 32)
template <typename T, int KS> __host__ __device__ constexpr size_t kbuild_mfma_lds(int d) {
    const int kr = KS > 0 ? 4 * KS : 4 * ((d + 3) / 4);
    // (fp64: the I-side tile only, the J-side operand lives in registers -- see the kernel)
    return ((size_t)(sizeof(T) == 8 ? 1 : 2) * kr * KM_LDP + 2 * TB) * sizeof(T) + (sizeof(T) == 8 ? (size_t)EXP_TAB * 8 : 0);
}
template <typename T, int KT> struct KmScale;
template <> struct KmScale<double, 0> { static constexpr double v = EXP_COORD_SCALE_SE; };       // u = table units of exp(-r2 / 2)
template <> struct KmScale<double, 1> { static constexpr double v = 2.2360679774997896 * EXP_U_PER_ARG; };   // u = (sqrt(5) r 512 / ln2)^2: sqrt(u) in table units
template <> struct KmScale<double, 2> { static constexpr double v = 1.7320508075688772 * EXP_U_PER_ARG; };   // Matern-3/2: u = (sqrt(3) r 512 / ln2)^2
template <> struct KmScale<double, 3> { static constexpr double v = 0.70710678118654752; };      // rational quadratic: u = r2 / 2 (q = u / alpha)
template <> struct KmScale<float, 0> { static constexpr double v = 0.84932180028801904; };        // u = r2 log2(e) / 2
template <> struct KmScale<float, 1> { static constexpr double v = 2.2360679774997896; };
template <> struct KmScale<float, 2> { static constexpr double v = 1.7320508075688772; };         // u = 3 r2
template <> struct KmScale<float, 3> { static constexpr double v = 0.70710678118654752; };

// the entry from its accumulator u >= 0 (cancellation may leave u a few ulp of the norms below zero: clamped)
// sf2 2^(-w / 512) for w >= 0 in table units (exp_tab_u without its upper clamp: the host's bound on the norms keeps w far
// inside the int range; w = -1e-10 gives t = MAGIC, k = 0, r = -w and the factor 1 + 1e-13 -- harmless)
__device__ __forceinline__ double km_exp_u(double w, const double* __restrict__ tab) {
    constexpr double MAGIC = 6755399441055744.0;             // 1.5 * 2^52
    constexpr double C1 = 1.3538030870311431e-03;            // ln2 / 512
    constexpr double C2 = 9.163913992275265e-07;             // C1^2 / 2
    constexpr double C3 = 4.1353783506767136e-10;            // C1^3 / 6
    constexpr double C4 = 1.399621994296973e-13;             // C1^4 / 24
    const double t = MAGIC - w;
    const double kd = t - MAGIC;
    const double r = -kd - w;
    double p = __builtin_fma(C4, r, C3);
    p = __builtin_fma(p, r, C2);
    p = __builtin_fma(p, r, C1);
    p = __builtin_fma(p, r, 1.0);
    const int ki = __double2loint(t);
    return __builtin_ldexp(tab[ki & (EXP_TAB - 1)] * p, ki >> 9);
}
// alpha, inv_sf2: the rational quadratic's shape parameter and 1 / sf2 (the LDS table carries sf2)
template <int KT>
__device__ __forceinline__ double km_value(double u, double, const double* __restrict__ tab, double alpha = 1.0, double inv_sf2 = 1.0, double inv_alpha = 1.0) {
    if (KT == 0) {
        return km_exp_u(u, tab);                                  // (no clamp of u: two fp64 instructions per entry saved)
    } else if (KT == 2) {
        // Matern-3/2, (1 + s3) exp(-s3) with s3 = sqrt(3) r = (ln2 / 512) w, w = sqrt(u): the Matern-5/2 recipe without the square term
        asm("v_max_f64 %0, %1, %2" : "=v"(u) : "v"(u), "v"(1.0e-200));
        const double y = __builtin_amdgcn_rsq(u);
        const double e = __builtin_fma(-u * y, y, 1.0);
        const double w = u * __builtin_fma(0.5 * y, e, y);
        constexpr double A1 = 1.3538030870311431e-03;
        return __builtin_fma(A1, w, 1.0) * km_exp_u(w, tab);
    } else if (KT == 3) {
        // rational quadratic (1 + q)^-alpha = exp(-alpha log1p(q)), q = r2 / (2 alpha) = u / alpha >= 0.  No fp64 logarithm in
        // hardware: x0 = ln(1 + q) from v_log_f32 (relative error ~1e-7), one Newton step on exp(x) = 1 + q with the table
        // exponential, x1 = x0 + ln(1 + dl), dl = (1 + q) exp(-x0) - 1.  Tiny q: the seed is 0 and x1 = q - q^2 / 2.
        const double q = fmax(u, 0.0) * inv_alpha, yq = 1.0 + q;              // (a product: an fp64 division is ~20 instructions per entry)
        const double x0 = (double)(__builtin_amdgcn_logf((float)yq) * 0.69314718f);
        const double ex = km_exp_u(x0 * EXP_U_PER_ARG, tab) * inv_sf2;           // exp(-x0)
        const double dl = __builtin_fma(yq, ex, -1.0);                          // (1 + q) exp(-x0) - 1, |dl| ~ 1e-7 x0
        const double x1 = x0 + __builtin_fma(-0.5 * dl, dl, dl);                // ln(1 + dl) to second order: error ~ dl^3 / 3
        return km_exp_u(alpha * x1 * EXP_U_PER_ARG, tab);
    } else {
        // Matern-5/2 with s5 = sqrt(5) r in table units: w = sqrt(u) by the hardware's reciprocal square root seed and one
        // Newton step (relative error ~4e-15; the IEEE sqrt expansion was 15 instructions), s5 = w ln2 / 512
        asm("v_max_f64 %0, %1, %2" : "=v"(u) : "v"(u), "v"(1.0e-200));   // (fmax() costs a canonicalising second v_max_f64)
        const double y = __builtin_amdgcn_rsq(u);
        const double e = __builtin_fma(-u * y, y, 1.0);
        const double w = u * __builtin_fma(0.5 * y, e, y);
        constexpr double A1 = 1.3538030870311431e-03;            // s5 = A1 w
        constexpr double A2 = 6.109275994850177e-07;             // s5^2 / 3 = A2 u
        return __builtin_fma(A2, u, __builtin_fma(A1, w, 1.0)) * km_exp_u(w, tab);
    }
}
template <int KT>
__device__ __forceinline__ float km_value(float u, float sf2, const double*, float alpha = 1.f, float = 1.f, float inv_alpha = 1.f) {
    if (KT == 0) {
        return sf2 * __builtin_amdgcn_exp2f(-fmaxf(u, 0.f));
    } else if (KT == 2) {
        const float q = fmaxf(u, 1e-30f);
        const float s3 = q * __builtin_amdgcn_rsqf(q);
        return sf2 * (1.0f + s3) * __builtin_amdgcn_exp2f(s3 * -1.4426950408889634f);
    } else if (KT == 3) {
        // (1 + q)^-alpha = 2^(-alpha log2(1 + q)) on v_log_f32 / v_exp_f32 (the library's log1pf made this entry 5x slower than the
        // other families'; rounding 1 + q costs 6e-8 alpha of relative error in the entry, below the fp32 build's own 1e-6)
        const float q = fmaxf(u, 0.f) * inv_alpha;
        return sf2 * __builtin_amdgcn_exp2f(-alpha * __builtin_amdgcn_logf(1.0f + q));
    } else {
        const float q = fmaxf(u, 1e-30f);
        const float s5 = q * __builtin_amdgcn_rsqf(q);
        return sf2 * (1.0f + s5 + q * (1.0f / 3.0f)) * __builtin_amdgcn_exp2f(s5 * -1.4426950408889634f);
    }
}

template <typename T, int KS, int KT>
__global__ __launch_bounds__(256, 2) void kbuild_mfma_kernel(KBuildMArgs<T> m) {
    const KBuildArgs<T>& a = m.b;
    constexpr int NQ = 16 / (int)sizeof(T);         // adjacent rows per lane (one 16-byte store)
    constexpr int IBR = 16 * NQ;                    // rows per row block
    constexpr int NIB = TB / IBR;
    typedef T vec_t __attribute__((ext_vector_type(NQ)));
    typedef typename Num<T>::acc_t acc_t;
    typedef typename Num<T>::pair_t pair_t;
    extern __shared__ double lds_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slot = blockIdx.y;
    int ti, tj;
    if (a.mode == 0) {
        tri_decode(blockIdx.x + a.t0, a.nt_i, ti, tj);
    } else {
        ti = blockIdx.x % a.nt_i;
        tj = blockIdx.x / a.nt_i;
    }
    if (a.own_world > 0) {
        const int owner = (tj == a.nt_j) ? 0 : (tj / a.own_panel) % a.own_world;
        if (owner != a.own_rank) return;
    }
    const double* sp = a.slotp + (long)slot * SLOTP;
    if (sp[SP_MFMA] == 0.0) return;                 // (kbuild_kernel's slot)
    const T sf2 = (T)sp[0], sn2 = (T)sp[1], mu = (T)sp[2];
    const T alpha = (T)sp[SP_ALPHA1], inv_sf2 = (T)(1.0 / sp[0]), inv_alpha = (T)(1.0 / sp[SP_ALPHA1]);   // (rational quadratic only)
    const T coff = (T)sp[SP_OFFSET];                // constant offset of c + k1 (0 without one)
    const long ldo = (a.mode == 0) ? (long)TB : a.ld;
    T* out = a.out + (long)slot * a.bstride +
             ((a.mode == 0) ? (tile_index(ti, tj, a.nt_i) + (a.adj ? a.adj[panel_slot(tj, a.nt_j, a.own_panel)] : 0l)) * TS
                            : (long)tj * TB * a.ld + (long)ti * TB);
    if (a.mode == 0 && ti == a.nt_i - 1) {          // right-hand-side block-row: row 0 = r^T, rest 0 (as kbuild_kernel)
        const int r0 = 2 * lane;
        for (int jj = wave * 32; jj < wave * 32 + 32; ++jj) {
            const int gj = tj * TB + jj;
            pair_t v;
            v.x = (T)0;
            v.y = (T)0;
            if (lane == 0 && tj < a.nt_j && gj < a.n_j)
                v.x = a.y[gj] - (a.pw_mean ? a.pw_mean[(long)slot * a.pw_bstride + gj] : mu);
            *reinterpret_cast<pair_t*>(out + (long)jj * ldo + r0) = v;
        }
        return;
    }
    const int d = a.d;
    const int ks = KS > 0 ? KS : (d + 3) / 4, kr = 4 * ks;
    constexpr int KSR = KS > 0 ? KS : KB_LDS_MAXD / 4;    // k-steps a lane keeps J-side operands for (generic build: d <= 32)
    constexpr bool JREG = sizeof(T) == 8;           // J-side operand in registers (fp64) or in LDS (fp32), see below
    T* xjs = reinterpret_cast<T*>(lds_raw);         // [kr][KM_LDP]  -2 b  (fp32 only)
    T* xis = xjs + (JREG ? 0 : kr * KM_LDP);        // [kr][KM_LDP]  a
    T* nrm = xis + kr * KM_LDP;                     // [2][TB]  |b|^2, |a|^2
    const double* etab = reinterpret_cast<const double*>(nrm + 2 * TB);
    if (sizeof(T) == 8) {
        double* et = const_cast<double*>(etab);
        for (int idx = tid; idx < EXP_TAB; idx += 256) et[idx] = sp[0] * a.exp2tab[idx];
    }
    const double* ie = m.inv_ell + (long)slot * d;
    const double cs = KmScale<T, KT>::v;
    {   // one thread per point of the two tiles: centre, scale, round to T, norm of the ROUNDED coordinates
        const int side = tid >> 7, p = tid & 127;
        const T* src = side ? m.xri + (long)ti * TB + p : m.xrj + (long)tj * TB + p;
        const long np = side ? a.npad_i : a.npad_j;
        T* dst = (side ? xis : xjs) + p;
        double n2 = 0.0;
        for (int dd = 0; dd < d; ++dd) {
            const T v = (T)(((double)src[(long)dd * np] - m.centre[dd]) * (ie[dd] * cs));
            n2 = __builtin_fma((double)v, (double)v, n2);
            if (side) dst[dd * KM_LDP] = v;
            else if (!JREG) dst[dd * KM_LDP] = (T)-2 * v;
        }
        if (side || !JREG)
            for (int dd = d; dd < kr; ++dd) dst[dd * KM_LDP] = (T)0;
        nrm[side * TB + p] = (T)n2;
    }
    const int c = lane & 15, g = lane >> 4;
    // fp64 (round 6): the J-side operand -2 b of this wave's two 16-column blocks lives in REGISTERS: lane (c, g) feeds MFMA step s
    // with the coordinate k = 4 s + g of column j0 + c -- 2 ks values, the same rounded numbers the norms were formed from.  LDS
    // then holds the I-side tile only: half the footprint, i.e. more workgroups per CU where it set the occupancy (d = 32: 80 ->
    // 43 KiB, one -> three workgroups per CU; d = 16: 43 -> 25 KiB): d = 16 0.61 -> 0.67, d = 24 0.45 -> 0.53 of 8 TB/s.  Not fp32:
    // its tiles are half the size already and the extra registers cost more than the LDS gave (d = 16 0.66 -> 0.60).
    T avr[2][JREG ? KSR : 1];
    if constexpr (JREG) {
#pragma unroll
        for (int jbi = 0; jbi < 2; ++jbi)
#pragma unroll
            for (int s = 0; s < KSR; ++s) {
                const int k = 4 * s + g;
                T v = (T)0;
                if (k < d)
                    v = (T)-2 * (T)(((double)m.xrj[(long)k * a.npad_j + (long)tj * TB + (wave + 4 * jbi) * 16 + c] - m.centre[k]) * (ie[k] * cs));
                avr[jbi][s] = v;
            }
    }
    __syncthreads();

    const bool edge = (a.mode == 0) ? (ti == tj || (ti + 1) * TB > a.n_i)
                                    : ((ti + 1) * TB > a.n_i || (tj + 1) * TB > a.n_j);
    // 2 column blocks x NIB row blocks per wave; the I-side operands of a step are re-read from LDS (a handful of ds_read per
    // ~100 VALU instructions), which keeps the kernel small in registers -- several workgroups per CU, whose MFMA and VALU
    // phases overlap -- and the code small
#pragma unroll
    for (int jbi = 0; jbi < 2; ++jbi)
#pragma unroll 1
    for (int ib = 0; ib < NIB; ++ib) {
        // the four waves take ADJACENT 16-column blocks (w, w + 4): the workgroup's stores of a moment fall into one contiguous
        // 64 KiB of its tile (measured against a wave owning 32 columns: 0.69 -> 0.72 of 8 TB/s; profiles/r05_kbuild_store_order.txt)
        const int jb = wave + 4 * jbi;
        const int j0 = jb * 16, i0 = ib * IBR + NQ * c;
        const vec_t nai = *reinterpret_cast<const vec_t*>(nrm + TB + i0);
        acc_t acc[NQ];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const T nbj = nrm[j0 + Num<T>::drow(g, r)];
#pragma unroll
            for (int q = 0; q < NQ; ++q) acc[q][r] = nai[q] + nbj;
        }
#pragma unroll
        for (int s = 0; s < KSR; ++s) {
            if (KS > 0 || s < ks) {
                const T av = JREG ? avr[jbi][JREG ? s : 0] : xjs[(4 * s + g) * KM_LDP + j0 + c];
                const vec_t bv = *reinterpret_cast<const vec_t*>(xis + (4 * s + g) * KM_LDP + i0);
#pragma unroll
                for (int q = 0; q < NQ; ++q) acc[q] = Num<T>::mfma(av, bv[q], acc[q]);
            }
        }
        const int gi0 = ti * TB + i0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int jc = j0 + Num<T>::drow(g, r);
            vec_t v;
#pragma unroll
            for (int q = 0; q < NQ; ++q) v[q] = km_value<KT>(acc[q][r], sf2, etab, alpha, inv_sf2, inv_alpha) + coff;
            if (edge) {
                const int gj = tj * TB + jc;
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const int gi = gi0 + q;
                    if (a.mode == 0) {
                        if (gi == gj) v[q] += a.pw_nug ? a.pw_nug[(long)slot * a.pw_bstride + gj] : sn2;
                        if (gj >= a.n_j || gi >= a.n_i) v[q] = (gi == gj) ? (T)1 : (T)0;      // identity pad
                    } else if (gj >= a.n_j || gi >= a.n_i) {
                        v[q] = (T)0;
                    }
                }
            }
            *reinterpret_cast<vec_t*>(out + (long)jc * ldo + i0) = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// potrf128: Cholesky of one 128x128 diagonal block AND its triangular inverse, in LDS.
//
// Factor phase, 8 panels of 16 columns:
//   (a) wave 0 factors the 16x16 diagonal block in registers (lane = row, v_readlane broadcasts),
//   (b) one thread per row below solves its 16 panel entries against L_pp,
//   (c) all 4 waves apply the rank-16 trailing update on the 16x16x4 MFMA.
// Then L goes back to HBM, and W = L^-1 is formed in place (LAPACK dtrtri order, 16x16 blocks,
// MFMA products) and stored to the Winv workspace: the panel solve below the block is then a
// plain MFMA GEMM  X <- A W^T  (gemm_nt mode 1).
// SPD verdict: pivot <= tol (tol = 64 eps (sf2+sn2)) or NaN -> info = NOT_SPD (stands for
// LinearSolve::sing1/::luc -> Throw "MatInv", BGP:131-135).
//
// LDS image: the 36 lower-triangle 16x16 tiles, tile (bi,bj) at ((bi(bi+1)/2 + bj) * 256) elements,
// column-major inside the tile.  72 KiB in fp64: the kernel fits on a CU next to one gemm_nt
// workgroup (look-ahead runs it concurrently with the trailing SYRK), and MFMA fragment reads
// (lane -> row l&15, k = l>>4) are bank-conflict free.
// ---------------------------------------------------------------------------------------------
// developer instrumentation (scripts/micro/df_phases.hip): phase stamps of thread 0 of every workgroup
#ifdef GPHIP_TIMING
__device__ long long* g_stamp_buf;               // [workgroups of the launch][64] wall-clock (100 MHz) phase stamps; entry 63 of a
                                                 // dataflow workgroup = its task number
#define GP_STAMP(i) do { if (threadIdx.x == 0 && g_stamp_buf) g_stamp_buf[(long)blockIdx.x * 64 + (i)] = wall_clock64(); } while (0)
#else
#define GP_STAMP(i) do { } while (0)
#endif

// 1/sqrt(x) for the pivot chain: hardware seed (v_rsq_f64, relative error ~5e-8) + one Newton step
// y + (y/2)(1 - x y^2)  ->  ~4e-15, far below the N eps backward error of the factorisation; three
// dependent operations after the seed instead of the library rsqrt's ~dozen.
__device__ __forceinline__ double fast_rsqrt(double x) {
    const double y = __builtin_amdgcn_rsq(x);
    const double hy = 0.5 * y;
    const double e = __builtin_fma(-x * y, y, 1.0);
    return __builtin_fma(hy, e, y);
}

constexpr int PT_LDS_ELEMS = 36 * 256 + TB;     // tiles + dinv[128]  (+ 2 doubles of reduction scratch)

// global store of the potrf core: plain, or write-through at agent scope (WT: the dataflow kernel's diagonal task, whose
// results are then published without an L2 write-back fence)
template <bool WT, typename T>
__device__ __forceinline__ void gst(T* p, T v) {
    if constexpr (WT) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}
__device__ __forceinline__ int ptile(int bi, int bj) { return ((bi * (bi + 1) / 2) + bj) << 8; }

// Block column PB of W = L^-1 (rows q = PB+1..7), computed by ONE wave with no barriers:
//   W[q][PB] = -W_qq * sum_{r=PB}^{q-1} L[q][r] W[r][PB]
// L tiles and the diagonal inverses W_rr are read from LDS; the W[r][PB] this wave has already
// produced stay in registers in the MFMA D layout, which is exactly the B-operand layout of the
// next product (Num<T>::kidx), and go straight to the Winv workspace.
// Wd: the diagonal inverses W_bb as separate 16x16 tiles [b][col * 16 + row] (the 64-block path, whose factor phase produces
// them on the side and keeps the L image whole), or null: they sit in the diagonal tiles of the image itself.
template <typename T, int PB, int NB = 8, bool WT = false, bool SEPW = false>
__device__ __forceinline__ void inv_block_column(const T* __restrict__ Ls, T* __restrict__ Wg, int l15, int l4,
                                                 const T* __restrict__ Wd = nullptr) {
    typedef typename Num<T>::acc_t acc_t;
    constexpr int NQ = NB - 1 - PB;
    acc_t w[NQ > 0 ? NQ : 1];
    const T* Wpp = SEPW ? Wd + PB * 256 : Ls + ptile(PB, PB);
#pragma unroll
    for (int qq = 0; qq < NQ; ++qq) {
        const int q = PB + 1 + qq;
        acc_t sacc = (acc_t){0, 0, 0, 0};
        {
            const T* Lq = Ls + ptile(q, PB);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int k = Num<T>::kidx(kk, l4);
                const T fb = (k >= l15) ? Wpp[SEPW ? k * 16 + l15 : l15 * 16 + k] : (T)0;   // W_pp(k, j = l15), lower (Wd tiles: [row][col])
                sacc = Num<T>::mfma(Lq[k * 16 + l15], fb, sacc);
            }
        }
#pragma unroll
        for (int rr = 0; rr < qq; ++rr) {
            const T* Lqr = Ls + ptile(q, PB + 1 + rr);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
                sacc = Num<T>::mfma(Lqr[Num<T>::kidx(kk, l4) * 16 + l15], w[rr][kk], sacc);
        }
        const T* Wqq = SEPW ? Wd + q * 256 : Ls + ptile(q, q);
        acc_t out = (acc_t){0, 0, 0, 0};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int k = Num<T>::kidx(kk, l4);
            const T fa = (l15 >= k) ? Wqq[SEPW ? l15 * 16 + k : k * 16 + l15] : (T)0;   // W_qq(i = l15, k), lower
            out = Num<T>::mfma(-fa, sacc[kk], out);
        }
        w[qq] = out;
#pragma unroll
        for (int r = 0; r < 4; ++r) gst<WT>(Wg + (PB * 16 + l15) * (16 * NB) + q * 16 + Num<T>::drow(l4, r), (T)out[r]);
    }
}

// Trailing update of panel p inside the 128x128 block: C(u,v) -= X_u X_v^T over the 16x16 tiles below
// and right of the panel.  A wave owns tiles first, first+stride, ..; NR of them at a time are
// independent MFMA chains issued interleaved (accumulators start AT C, operand negated), so the
// wave runs at MFMA throughput instead of one tile's latency at a time.  Past the last tile it
// recomputes that tile and skips the store.
template <typename T, int NR>
__device__ __forceinline__ void potrf_update(T* __restrict__ Ls, int p, int t, int first, int stride, int l15, int l4) {
    typedef typename Num<T>::acc_t acc_t;
    const int ntile = t * (t + 1) / 2;      // t = block rows below the panel; this wave: tiles first, first+stride, ..
    acc_t acc[NR];
    T fa[NR][4], fb[NR][4];
    T* Ct[NR];
#pragma unroll
    for (int m = 0; m < NR; ++m) {
        int tt = first + stride * m;
        if (tt >= ntile) tt = ntile - 1;
        // tt -> (u, v), v <= u, tt = u(u+1)/2 + v < 28: branch-free (a taken scalar branch costs ~32 cycles)
        const int u = (tt >= 1) + (tt >= 3) + (tt >= 6) + (tt >= 10) + (tt >= 15) + (tt >= 21);
        const int v = tt - u * (u + 1) / 2;
        const T* Xc = Ls + ptile(p + 1 + v, p) + l4 * 16 + l15;
        const T* Xrw = Ls + ptile(p + 1 + u, p) + l4 * 16 + l15;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            fa[m][kk] = -Xc[kk * 64];
            fb[m][kk] = Xrw[kk * 64];
        }
        Ct[m] = Ls + ptile(p + 1 + u, p + 1 + v) + l15;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[m][r] = Ct[m][Num<T>::drow(l4, r) * 16];
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int m = 0; m < NR; ++m) acc[m] = Num<T>::mfma(fa[m][kk], fb[m][kk], acc[m]);
#pragma unroll
    for (int m = 0; m < NR; ++m)
        if (first + stride * m < ntile) {
#pragma unroll
            for (int r = 0; r < 4; ++r) Ct[m][Num<T>::drow(l4, r) * 16] = acc[m][r];
        }
}

// W = L^-1 of a factored block in the tile-packed LDS image (destroys the diagonal tiles of the
// image): (i) the NB 16x16 diagonal inverses, (ii) the off-diagonal blocks column by column on the
// MFMA, (iii) W (with an explicit zero upper triangle) to Wg, leading dimension 16 NB.
// dinv[c] = 1 / L_cc.  All 256 threads; ends without a barrier.
// SEPW: step (i) has been done by the factor phase, the diagonal inverses are the tiles at Wd and the L image stays whole.
template <typename T, int NB, bool WT = false, bool SEPW = false>
__device__ __forceinline__ void tri_inverse_lds(T* __restrict__ Ls, const T* __restrict__ dinv, T* __restrict__ Wg,
                                                const T* __restrict__ Wd = nullptr) {
    constexpr int NE = 16 * NB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int er = tid & 15, ec = tid >> 4;
    // ------------------------------ inverse phase ------------------------------
    if constexpr (!SEPW) {   // (i) the eight 16x16 diagonal inverses: thread = (block, column)
        T w[16];
        const int blk = tid >> 4, c = tid & 15;
        T* Dbb = Ls + ptile(blk & (NB - 1), blk & (NB - 1));
        if (tid < NE) {
            // column c of L_bb^-1 by forward substitution on e_c, right-looking (short dependent chain)
#pragma unroll
            for (int i = 0; i < 16; ++i) w[i] = (i == c) ? (T)1 : (T)0;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                w[k] *= dinv[16 * blk + k];
#pragma unroll
                for (int i = k + 1; i < 16; ++i) w[i] = __builtin_fma(-w[k], Dbb[k * 16 + i], w[i]);
            }
        }
        __syncthreads();
        if (tid < NE) {
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (i >= c) Dbb[c * 16 + i] = w[i];
        }
        __syncthreads();
    }
    GP_STAMP(32);
    // (ii) the off-diagonal blocks: block columns are independent, wave w owns columns w and NB-1-w
    {
        const int uw = __builtin_amdgcn_readfirstlane(wave);
        if constexpr (NB == 8) {
            if (uw == 0) {
                inv_block_column<T, 0, 8, WT>(Ls, Wg, l15, l4);
            } else if (uw == 1) {
                inv_block_column<T, 1, 8, WT>(Ls, Wg, l15, l4);
                inv_block_column<T, 6, 8, WT>(Ls, Wg, l15, l4);
            } else if (uw == 2) {
                inv_block_column<T, 2, 8, WT>(Ls, Wg, l15, l4);
                inv_block_column<T, 5, 8, WT>(Ls, Wg, l15, l4);
            } else {
                inv_block_column<T, 3, 8, WT>(Ls, Wg, l15, l4);
                inv_block_column<T, 4, 8, WT>(Ls, Wg, l15, l4);
            }
        } else {
            if (uw == 0) inv_block_column<T, 0, 4, WT, SEPW>(Ls, Wg, l15, l4, Wd);
            else if (uw == 1) inv_block_column<T, 1, 4, WT, SEPW>(Ls, Wg, l15, l4, Wd);
            else if (uw == 2) inv_block_column<T, 2, 4, WT, SEPW>(Ls, Wg, l15, l4, Wd);
        }
    }
    GP_STAMP(33);
    // diagonal blocks of W and an explicit zero upper triangle (the blocks below went out above)
    for (int bi = 0; bi < NB; ++bi)
        for (int bj = bi; bj < NB; ++bj) {
            T v = (T)0;
            if (bi == bj && er >= ec) v = SEPW ? Wd[bi * 256 + er * 16 + ec] : Ls[ptile(bi, bj) + tid];
            gst<WT>(Wg + (bj * 16 + ec) * NE + bi * 16 + er, v);
        }
}

// X (the chain's freshly solved 64 x 64 sub-diagonal tile) as the dataflow kernel keeps it in LDS: four 16-column images
// [k][row] in the 64-tile stage layout (chol_dataflow_kernel, diagx).  x64_off = df_lds_off<double, 64>.
constexpr int X64_LD = 144, X64_IMG = 8 * X64_LD;
__device__ __forceinline__ int x64_off(int k, int row) { return ((k >> 2) * 2 + (k & 1)) * X64_LD + ((k >> 1) & 1) * 64 + row; }
// 16x16 block (bi, bj) of the potrf image -= X(16 bi.., :) X(16 bj.., :)^T, by ONE wave: the last slab of the diagonal tile's
// update, block by block, so that the factorisation of block column 0 can start while other waves still apply it to the rest.
template <typename T>
__device__ __forceinline__ void xx_block_rmw(T* __restrict__ Ls, const T* __restrict__ Ximg, int bi, int bj, int l15, int l4, T* __restrict__ copy = nullptr) {
    typedef typename Num<T>::acc_t acc_t;
    T* Cb = Ls + ptile(bi, bj) + l15;
    acc_t a;
#pragma unroll
    for (int r = 0; r < 4; ++r) a[r] = Cb[Num<T>::drow(l4, r) * 16];
#pragma unroll
    for (int st = 0; st < 4; ++st)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const T* Im = Ximg + st * X64_IMG + l15;
            const int kq = 4 * kk + l4;
            a = Num<T>::mfma(-Im[x64_off(kq, 16 * bj)], Im[x64_off(kq, 16 * bi)], a);
        }
#pragma unroll
    for (int r = 0; r < 4; ++r) Cb[Num<T>::drow(l4, r) * 16] = a[r];
    if (copy) {
#pragma unroll
        for (int r = 0; r < 4; ++r) copy[Num<T>::drow(l4, r) * 16 + l15] = a[r];
    }
}

// Out-of-line for the use INSIDE the potrf body (idle waves of panels 0 and 1): inlined six times there it changed the register
// allocation of every panel of the factorisation (+0.3 us per panel on the chain); the call itself runs off the chain.
template <typename T>
__device__ __noinline__ void xx_blocks_call(T* Ls, const T* Ximg, int b0i, int b0j, int b1i, int b1j, int l15, int l4) {
    xx_block_rmw<T>(Ls, Ximg, b0i, b0j, l15, l4);
    if (b1i >= 0) xx_block_rmw<T>(Ls, Ximg, b1i, b1j, l15, l4);
}

// 64-block path (fp64): behind the 10 tiles + dinv[64] of the image sit four tiles Wd that start as the identity and end as the
// diagonal inverses, and a copy S of tile (0,0).  The caller fills them with the image, before its barrier: potrf64_aux_init by
// all 256 threads, S by whoever writes tile (0,0) (same [col * 16 + row] order).
constexpr int PT64_WD = 10 * 256 + 64, PT64_S = PT64_WD + 4 * 256;      // element offsets from Ls
template <typename T>
__device__ __forceinline__ void potrf64_aux_init(T* __restrict__ Ls) {
    const int tid = threadIdx.x;
    const T v = ((tid >> 4) == (tid & 15)) ? (T)1 : (T)0;
#pragma unroll
    for (int b = 0; b < 4; ++b) Ls[PT64_WD + b * 256 + tid] = v;
}

// Core of potrf128 on a tile-packed LDS image that is already in place (all 256 threads; the caller
// has synchronised after filling Ls).  NB = 16-blocks per side: 8 (128x128, the tile of the
// multi-kernel schedule) or 4 (64x64, the fine-grained dataflow schedule).  Writes L to Ad (global,
// leading dimension ld), W = L^-1 to Wg (leading dimension 16 NB, explicit zero upper triangle),
// sum log L_jj to *logdet_out and 1 to *info_out on a bad pivot.
template <typename T, int NB = 8, bool WT = false>
__device__ __forceinline__ void potrf128_core(double* __restrict__ lds_raw, T* __restrict__ Ad, long ld,
                                              T* __restrict__ Wg, double* __restrict__ logdet_out,
                                              int* __restrict__ info_out, T tol, int* pub_flag = nullptr, int pub_epoch = 0,
                                              int* chain_flag = nullptr, T* __restrict__ Dg = nullptr, const T* __restrict__ Ximg = nullptr) {
    double* red = lds_raw;                      // 2 doubles
    constexpr int NE = 16 * NB;                 // block edge
    T* Ls = reinterpret_cast<T*>(lds_raw + 2);  // NB(NB+1)/2 tiles + dinv[NE] (+ 64-block path: NB diagonal-inverse tiles)
    T* dinv = Ls + (NB * (NB + 1) / 2) * 256;
    constexpr bool SEPW = NB == 4 && sizeof(T) == 8;
    T* Wd = dinv + NE;                          // SEPW only: = Ls + PT64_WD; the copy S of tile (0,0) behind the four tiles
    typedef typename Num<T>::acc_t acc_t;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int er = tid & 15, ec = tid >> 4;   // element (row, col) of a 16x16 tile owned in copies
    bool bad = false;
    GP_STAMP(1);

    // ------------------------------ factor phase ------------------------------
    // Panel p:  wave 0 brings the diagonal tile (p,p) up to date with panel p-1 and factors it (a) WHILE
    // waves 1-3 apply panel p-1 to every other trailing tile (c); then all rows below solve against L_pp (b).
    const int uwv = __builtin_amdgcn_readfirstlane(wave);
    if constexpr (NB == 4 && sizeof(T) == 8) {
        // 64x64 block: a whole 16-column panel (<= 64 rows) fits ONE wave with lane = row, so the
        // diagonal factor (a) and the row solves (b) are the same elimination: x[c] *= rs_c, then
        // x[c2] -= x[c] L[c2][c] with the pivot row's values broadcast by v_readlane.  No D-layout
        // gather, no separate row-solve pass, one barrier per panel.  Wave 0 first applies panel p-1 to
        // its own block column (<= 3 tiles) while waves 1-3 take the other trailing tiles.
        // (unrolled: with p a constant the roles below fold and the update's tile loops unroll -- 22.6 -> 20.9 us per hop)
#pragma unroll
        for (int p = 0; p < NB; ++p) {
            GP_STAMP(2 + 3 * p);
            if (p > 0) {
                const int t = NB - p;
                if (uwv == 0) {
                    for (int u = 0; u < t; ++u) potrf_update<T, 1>(Ls, p - 1, t, u * (u + 1) / 2, 1 << 20, l15, l4);
                } else {
                    const int tt = (t == 3) ? (uwv == 1 ? 2 : (uwv == 2 ? 4 : 5)) : ((t == 2 && uwv == 1) ? 2 : -1);
                    // (p = 1 with X images: this wave's tile -- (2,2), (3,2) or (3,3) -- first receives its share of -X X^T)
                    if (p == 1 && Ximg) xx_blocks_call<T>(Ls, Ximg, uwv == 1 ? 2 : 3, uwv == 3 ? 3 : 2, -1, -1, l15, l4);
                    if (tt >= 0) potrf_update<T, 1>(Ls, p - 1, t, tt, 1 << 20, l15, l4);
                }
            }
            // The diagonal inverse W_pp rides along: sixteen lanes start from the rows of the identity and go through the same
            // elimination, [I] L_pp^-T = W_pp^T -- the free lanes 48-63 of wave 0 for p > 0; for p = 0 (all 64 lanes are rows)
            // wave 1, idle in that panel, repeats the elimination of the diagonal tile (from the copy S, which wave 0 never
            // writes) with the identity in its lanes 16-31.  The identity rows are LDS tiles like any other (potrf64_aux_init),
            // so those lanes run the very same load / eliminate / store code through their own pointer: tile p of Wd receives
            // W_pp in [row * 16 + col] order.  Same operations in the same order as the substitution it replaces
            // (tri_inverse_lds step (i)), off the chain.
            const bool w1 = p == 0 && uwv == 1;
            if (uwv == 0 || w1) {
                const int nrows = NE - 16 * p;
                const int idl = w1 ? 16 : 48;
                const bool isid = (w1 || p > 0) && lane >= idl && lane < idl + 16;
                const bool rowl = !w1 && lane < nrows;
                const bool live = rowl || isid;
                T* Xr = isid ? Wd + p * 256 + (lane - idl)
                             : (rowl ? Ls + ptile(p + (lane >> 4), p) : (w1 ? Wd + NB * 256 : Ls + ptile(p, p))) + (lane & 15);
                double x[16], dv = 0.0;
#pragma unroll
                for (int c = 0; c < 16; ++c) x[c] = (double)Xr[c * 16];
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const double dj = Num<double>::readlane(x[c], c);
                    bad = bad || !(dj > (double)tol);
                    const double rs = fast_rsqrt(dj);
                    dv = (lane == c) ? rs : dv;
                    x[c] *= rs;
#pragma unroll
                    for (int c2 = c + 1; c2 < 16; ++c2) {
                        const double lc = Num<double>::readlane(x[c], c2);          // L[c2][c]
                        x[c2] = __builtin_fma(-x[c], lc, x[c2]);
                    }
                }
                if (live) {
#pragma unroll
                    for (int c = 0; c < 16; ++c) Xr[c * 16] = (T)x[c];
                }
                if (uwv == 0 && lane < 16) dinv[16 * p + lane] = (T)dv;
            }
            // Ximg given: the image's block column 0 is final, the other lower blocks still lack the last slab -X X^T of the
            // diagonal tile's update.  Block column 1 (needed by panel 1): waves 2 and 3, idle in this panel, under the
            // elimination of panel 0; blocks (2,2), (3,2), (3,3): in panel 1, by the waves that own them there (above).
            if (p == 0 && Ximg) {
                if (uwv == 2) xx_blocks_call<T>(Ls, Ximg, 1, 1, 2, 1, l15, l4);
                if (uwv == 3) xx_blocks_call<T>(Ls, Ximg, 3, 1, -1, -1, l15, l4);
            }
            __syncthreads();
            GP_STAMP(3 + 3 * p);
        }
    } else
    for (int p = 0; p < NB; ++p) {
        T* Dpp = Ls + ptile(p, p);
        GP_STAMP(2 + 3 * p);
        if (p > 0) {                           // (c) trailing update C -= X X^T of panel p-1 on MFMA
            const int t = NB - p;              // block rows below panel p-1
            if (uwv == 0) {
                potrf_update<T, 1>(Ls, p - 1, t, 0, 1 << 20, l15, l4);        // tile (p,p) only
            } else {
                const int cnt = (t * (t + 1) / 2 - 1 + 2) / 3;                // tiles 1.. dealt to waves 1-3
                for (int m0 = 0; m0 < cnt; m0 += 5) potrf_update<T, 5>(Ls, p - 1, t, uwv + 3 * m0, 3, l15, l4);
            }
        }
        if (wave == 0 && sizeof(T) == 8) {
            // (a) fp64: the 16x16 diagonal block lives in the MFMA D layout -- lane (l15, l4) holds
            // A[i = l15][j = l4 + 4r], r = 0..3.  Columns are eliminated four at a time: the 16x4 slab
            // is gathered into row-per-lane form (one ds_bpermute round per slab), factored with
            // v_readlane broadcasts only (pivot chain = readlane, rsq, mul, readlane, fma), and the
            // rank-4 update of the remaining columns is one MFMA in the D layout.
            double a[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r] = (double)Dpp[(l4 + 4 * r) * 16 + l15];
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                // slab = columns 4 s4 .. 4 s4 + 3 in row-per-lane form: s[q] = A[l15][4 s4 + q], gathered
                // from the lanes (l15, q); all four 16-lane groups hold the same copy
                double sl[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) sl[q] = __shfl(a[s4], 16 * q + l15);
                double rsv[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c = 4 * s4 + q;
                    // Pivot chain: readlane, rsq + one Newton step, mul, readlane, fma -- nothing else.
                    // A bad pivot (<= tol, NaN) only raises the flag; its NaN/Inf flows on and the
                    // caller discards the values (info != 0), so no select sits on the chain.  Lane c
                    // already holds d = A[c][c], so scaling every lane by rs leaves sqrt(d) there.
                    const double dj = Num<double>::readlane(sl[q], c);
                    bad = bad || !(dj > (double)tol);
                    const double rs = fast_rsqrt(dj);
                    rsv[q] = rs;
                    sl[q] *= rs;
#pragma unroll
                    for (int q2 = q + 1; q2 < 4; ++q2) {
                        const double lc = Num<double>::readlane(sl[q], 4 * s4 + q2);   // L[4 s4 + q2][c]
                        sl[q2] = __builtin_fma(-sl[q], lc, sl[q2]);
                    }
                }
                if (lane < 4)
                    dinv[16 * p + 4 * s4 + lane] = (T)((lane == 0) ? rsv[0] : (lane == 1) ? rsv[1] : (lane == 2) ? rsv[2] : rsv[3]);
                // back to the D layout; then the rank-4 update of the later column groups is ONE MFMA
                // whose A and B operands are the lane's own column value (L is zero above its diagonal)
                const double mine = (l4 == 0) ? sl[0] : (l4 == 1) ? sl[1] : (l4 == 2) ? sl[2] : sl[3];
                a[s4] = mine;
                if (s4 < 3) {
                    const double xop = (l15 >= 4 * s4 + l4) ? mine : 0.0;
                    d4 cacc = (d4){a[0], a[1], a[2], a[3]};
                    cacc = __builtin_amdgcn_mfma_f64_16x16x4f64(-xop, xop, cacc, 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (r > s4) a[r] = cacc[r];
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (l15 >= l4 + 4 * r) Dpp[(l4 + 4 * r) * 16 + l15] = (T)a[r];
        } else if (wave == 0) {               // (a) fp32: lane l15 owns row l15, v_readlane broadcasts
            T a[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) a[c] = Dpp[c * 16 + l15];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                T dj = Num<T>::readlane(a[j], j);
                if (!(dj > tol)) { bad = true; dj = (T)1; }
                const T rs = Num<T>::rsqrt_(dj);       // one dependent transcendental per pivot, not sqrt + rcp
                const T l = dj * rs;
                a[j] = (l15 == j) ? l : a[j] * rs;
#pragma unroll
                for (int c = j + 1; c < 16; ++c) {
                    const T sc = Num<T>::readlane(a[j], c);
                    a[c] = __builtin_fma(-a[j], sc, a[c]);
                }
                if (lane == 0) dinv[16 * p + j] = rs;
            }
            if (lane < 16) {
#pragma unroll
                for (int c = 0; c < 16; ++c)
                    if (c <= l15) Dpp[c * 16 + l15] = a[c];
            }
        }
        __syncthreads();
        GP_STAMP(3 + 3 * p);
        if (p == NB - 1) break;
        if (tid < NE - 16 * p - 16) {         // (b) rows below: x L_pp^T = a, one row per thread
            T* Xr = Ls + ptile(p + 1 + (tid >> 4), p) + (tid & 15);
            T x[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) x[c] = Xr[c * 16];
            // right-looking order: the dependent chain is one mul + one fma per column (16 x 2), the
            // other 15-c fmas of a step are independent
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                x[c] *= dinv[16 * p + c];
#pragma unroll
                for (int k = c + 1; k < 16; ++k) x[k] = __builtin_fma(-x[c], Dpp[c * 16 + k], x[k]);
            }
#pragma unroll
            for (int c = 0; c < 16; ++c) Xr[c * 16] = x[c];
        }
        __syncthreads();
        GP_STAMP(4 + 3 * p);
    }

    GP_STAMP(30);
    if constexpr (SEPW) {
        // 64-block path (the dataflow kernel's chain): nobody inside the launch reads L_jj -- its consumers (solves, prediction,
        // the broadcast of a sharded panel) come after the kernel -- so the order is W first, then the hand-over to the next hop
        // (flag), and the L tile goes out behind it.  The log-det partial and the info word precede the flag: the corner task
        // of the one-launch evaluation reads them.
        if (uwv == 3) {                                                  // (idle in the inverse phase; NE = 64 = one wave)
            double lg = -log((double)dinv[lane]);
            for (int off = 32; off > 0; off >>= 1) lg += __shfl_down(lg, off);
            if (lane == 0) gst<WT>(logdet_out, lg);
        }
        if (tid == 0 && bad) gst<WT>(info_out, 1);
        GP_STAMP(31);
        if (Dg) {
            // Chain hand-over (Dg given): the next hop's sub-diagonal solve substitutes with L_jj and the four diagonal
            // inverses only, so THOSE go out first, under their own flag; the off-diagonal blocks of W_j -- for the panel
            // solves below, which have slack -- are computed and published behind it.
            // (the substitution reads the six OFF-diagonal 16x16 blocks of L and the inverses of the diagonal ones: those first;
            //  the diagonal blocks of L, which nobody inside the launch reads, behind the flag)
#pragma unroll
            for (int b = 0; b < NB; ++b) gst<WT>(Dg + b * 256 + tid, Wd[b * 256 + er * 16 + ec]);    // [col * 16 + row] out of [row][col]
            for (int bi = 1; bi < NB; ++bi)
                for (int bj = 0; bj < bi; ++bj)
                    gst<WT>(Ad + (long)(bj * 16 + ec) * ld + bi * 16 + er, Ls[ptile(bi, bj) + tid]);
            if (chain_flag) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                if (tid == 0) __hip_atomic_store(chain_flag, pub_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            for (int bi = 0; bi < NB; ++bi) gst<WT>(Ad + (long)(bi * 16 + ec) * ld + bi * 16 + er, Ls[ptile(bi, bi) + tid]);
        }
        GP_STAMP(32);
        tri_inverse_lds<T, NB, WT, true>(Ls, dinv, Wg, Wd);
        GP_STAMP(34);
        if (pub_flag) {                                                  // (WT stores: at the coherent level once vmcnt drains)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) __hip_atomic_store(pub_flag, pub_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        GP_STAMP(35);
        if (!Dg) {
            for (int bi = 0; bi < NB; ++bi)
                for (int bj = 0; bj <= bi; ++bj)
                    gst<WT>(Ad + (long)(bj * 16 + ec) * ld + bi * 16 + er, Ls[ptile(bi, bj) + tid]);
        }
        GP_STAMP(36);
        return;
    }
    // L back to HBM (lower-triangle tiles; diagonal tiles whole, their upper part is never read)
    for (int bi = 0; bi < NB; ++bi)
        for (int bj = 0; bj <= bi; ++bj)
            gst<WT>(Ad + (long)(bj * 16 + ec) * ld + bi * 16 + er, Ls[ptile(bi, bj) + tid]);
    {   // sum log L_jj = -sum log dinv_j  (always accumulated in fp64)
        double lg = 0.0;
        if (tid < NE) lg = -log((double)dinv[tid]);
        for (int off = 32; off > 0; off >>= 1) lg += __shfl_down(lg, off);
        if (wave < 2 && lane == 0) red[wave] = lg;
    }

    GP_STAMP(31);
    tri_inverse_lds<T, NB, WT>(Ls, dinv, Wg);
    GP_STAMP(34);
    if (tid == 0) {
        gst<WT>(logdet_out, red[0] + red[1]);
        if (bad) gst<WT>(info_out, 1);
    }
}

// Out-of-line copy for chol_dataflow_kernel: keeps the factorisation's register allocation apart from
// the accumulator-heavy MFMA loops of that kernel (inlined, the allocator spills accumulators there).
// The image's place in the dynamic LDS is a TEMPLATE argument (doubles from its start; XOFF likewise for the X images): handed
// over as a run-time pointer -- or as a constant that differs between the call sites of one instantiation -- the body addresses
// it with flat instructions (measured: +0.3 us per panel, +1.2 us per hop).
template <typename T, int NB, bool WT = false, int LDSOFF = 0, bool XIMG0 = false>
__device__ __noinline__ void potrf128_core_call(T* Ad, long ld, T* Wg, double* logdet_out,
                                                int* info_out, T tol, int* pub_flag, int pub_epoch, int* chain_flag, T* Dg, bool xx) {
    extern __shared__ double potrf_lds_dyn[];
    potrf128_core<T, NB, WT>(potrf_lds_dyn + LDSOFF, Ad, ld, Wg, logdet_out, info_out, tol, pub_flag, pub_epoch, chain_flag, Dg,
                             (XIMG0 && xx) ? reinterpret_cast<const T*>(potrf_lds_dyn) : nullptr);
}
template <typename T>
__global__ __launch_bounds__(256) void potrf128_kernel(T* __restrict__ Abase, long bstride, int b,
                                                       T* __restrict__ Winv, double* __restrict__ partial,
                                                       int nt, int* __restrict__ info,
                                                       const double* __restrict__ slotp) {
    extern __shared__ double lds_raw[];
    T* Ls = reinterpret_cast<T*>(lds_raw + 2);
    const int tid = threadIdx.x;
    const int er = tid & 15, ec = tid >> 4;
    const int slot = blockIdx.x;
    constexpr long ld = TB;
    T* Ad = Abase + (long)slot * bstride + tile_index(b, b, nt + 1) * TS;       // diagonal tile b of the packed workspace
    for (int bi = 0; bi < 8; ++bi)
        for (int bj = 0; bj <= bi; ++bj)
            Ls[ptile(bi, bj) + tid] = Ad[(long)(bj * 16 + ec) * ld + bi * 16 + er];
    GP_STAMP(0);
    __syncthreads();
    potrf128_core<T>(lds_raw, Ad, ld, Winv + ((long)slot * nt + b) * TB * TB, partial + (long)slot * nt + b,
                     info + slot, (T)slotp[(long)slot * SLOTP + 3]);
}

// W_b = L_bb^-1 of every 128x128 diagonal block of an already factored matrix (grid = (Nt, slots)).
// The fine-grained (64x64) dataflow schedule only produces inverses of 64-blocks; the solve /
// prediction / gradient paths substitute with 128-blocks, so gphip_fit re-inverts once here.
template <typename T>
__global__ __launch_bounds__(256) void trtri128_kernel(const T* __restrict__ Abase, long bstride,
                                                       T* __restrict__ Winv, int nt, int b0 = 0) {
    extern __shared__ double lds_raw[];
    T* Ls = reinterpret_cast<T*>(lds_raw + 2);
    T* dinv = Ls + 36 * 256;
    const int tid = threadIdx.x;
    const int er = tid & 15, ec = tid >> 4;
    const int b = b0 + blockIdx.x, slot = blockIdx.y;           // diagonal blocks b0, b0 + 1, ..
    constexpr long ld = TB;
    const T* Ad = Abase + (long)slot * bstride + tile_index(b, b, nt + 1) * TS;
    for (int bi = 0; bi < 8; ++bi)
        for (int bj = 0; bj <= bi; ++bj)
            Ls[ptile(bi, bj) + tid] = Ad[(long)(bj * 16 + ec) * ld + bi * 16 + er];
    if (tid < TB) dinv[tid] = (T)1 / Ad[(long)tid * ld + tid];
    __syncthreads();
    tri_inverse_lds<T, 8>(Ls, dinv, Winv + ((long)slot * nt + b) * TB * TB);
}

// ---------------------------------------------------------------------------------------------
// gemm_nt: C(i,j) -= sum_k A(i,k) B(j,k) for 128x128 tiles on the 16x16x4 MFMA
// (v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32).
//
// 256 threads = 4 waves in a 2(i) x 2(j) arrangement, 64x64 per wave = 4x4 MFMA tiles, 64
// accumulators per lane.  K is consumed in stages of GK (16 fp64 / 32 fp32 = 16 KiB per operand
// tile) through double-buffered LDS filled by LDS-DMA (global_load_lds_dwordx4) a stage ahead.
// fp64 image: [k][row] with a padded leading dimension of 144 doubles; fp32 image: k-columns
// stored in pairs {4q, 4q+2} / {4q+1, 4q+3} with 16 floats of padding after each pair -- both make
// the MFMA fragment read (lane -> row = lane&15, k = lane>>4) bank-conflict free.
//
// MFMA operand roles: the C-row (memory-contiguous) index i feeds the MFMA *B* operand so that
// D's column index (= lane&15) runs along contiguous memory of column-major C; the C-column index
// j feeds the *A* operand (D row = Num<T>::drow(lane>>4, reg)).
// ---------------------------------------------------------------------------------------------
constexpr int LDT = 144;          // fp64: padded LDS leading dimension (doubles)
constexpr int LDP = 272;          // fp32: one pair of k-columns + 16 floats of padding
constexpr int STAGE_BYTES = 2 * 16 * LDT * 8;      // one stage = I tile + J tile (36,864 B, both types)

template <typename T>
struct GemmArgs {
    T* C; long ldc; long c_bstride;
    const T* A; long lda; long a_bstride;        // I operand: A(i,k) at A[i + k*lda]
    const T* B; long ldb; long b_bstride;        // J operand: B(j,k) at B[j + k*ldb]
    // Each of C / A / B is either a column-major block (x_R = 0: pointer + leading dimension, as above) or lives in
    // the packed tile-major workspace (x_R = R > 0 tile rows: pointer = slot base, ld ignored):
    //   C tile (ti, tj)                          -> tile_index(ti, tj, c_R)
    //   A(i,k), i in tile row ti                 -> tile (ti, a_k0 + k/128), element (i % 128, k % 128)
    //   B(j,k), j in tile row tj                 -> tile (tj, b_k0 + k/128)
    //   ROLE 3 (B read transposed), B(j,k) = L(b_k0*128 + k, tj*128 + j) -> tile (b_k0 + k/128, tj), element (k % 128, j)
    // a_k0 / b_k0 = tile column where the operand panel starts.  The base pointer may be shifted so that a panel kept
    // OUTSIDE the workspace (a received panel of the multi-GPU schedule) is addressed with its global tile indices.
    int c_R, a_R, b_R, a_k0, b_k0;
    int b_lower;                                 // ROLE 2: the J operand is a LOWER-TRIANGULAR 128 x 128 block with explicit zeros above
                                                 //    the diagonal (W_b = L_bb^-1): B(j, k) = 0 for k > j, so the MFMAs of a 16-column
                                                 //    group whose columns all lie left of the current k-group are skipped (they add 0)
    const long* c_adj; int c_adj_panel;          // C in a rank's COMPACT own-panel storage (multi-GPU): tiles to add to the dense index
                                                 // of a tile of outer panel panel_slot(tj, c_R - 1, c_adj_panel); null: dense
    int K;                                       // multiple of GK
    int r0, r1, c0, c1;                          // tile ranges: rows [r0,r1), cols [c0,c1)
    int tri;                                     // 1: keep only tiles with ti >= tj (needs r0 >= c0)
    int nrect;                                   // tiles in the full-height rectangle part
    int ntiles;
    int swizzle;                                 // XCD-aware block remap
    int super;                                   // 2: pure-triangle launch whose tile list is enumerated in 8x8 super-tiles
    int mode;                                    // ROLE 3 only: 0: C -= A B ; 1: C = A B
    int ktri;                                    // 1: tile (ti,tj) contracts k >= ti*128 only (operands upper
                                                 //    triangular in (row, k): the U U^T product of the gradient)
    int grp_stride, grp_width, grp_count;        // grp_stride > 0: GROUPED triangular launch (multi-GPU block-cyclic layout):
                                                 //    group q = tile columns [c0 + q stride, + grp_width) clipped to c1, rows
                                                 //    from the group's own diagonal to r1; one dense 1-D grid over all groups
    int thin_row;                                // tile row whose rows beyond the first are zero and stay zero (the bordered
                                                 //    right-hand-side block-row of the factorisation: only r^T is real); -1: none
    // ROLE 4 (= ROLE 1 for the panel-stream updates of the look-ahead schedule; its own symbol because the potrf body costs
    // registers: 272 -> one such wave per SIMD), fuse_b >= 0: the workgroup that updates diagonal tile
    // (fuse_b, fuse_b) goes on to FACTOR it (the potrf128 body, same LDS) -- a separate potrf128 launch waits 100-250 us for a
    // CU slot under the trailing update, this workgroup already has one.  Outputs as potrf128_kernel's.
    int fuse_b;
    T* fuse_W; double* fuse_partial; int* fuse_info; const double* fuse_slotp; int fuse_nt;
    int skip_upper;                              // 1: diagonal tiles of a triangular update leave their strictly-upper 64x64
                                                 //    quadrant alone (nothing reads it: potrf128 and the dataflow tail take the
                                                 //    lower sub-tiles only)
};

// Position p of the lower triangle of an H x H tile grid enumerated SUPER-TILE by super-tile (8 x 8 tiles; super-tile
// columns left to right, inside a column the diagonal super-tile first, then downwards; inside a super-tile rows fastest).
// Column J < H / 8 holds T(J) = 36 + 8 (H - 8 J - 8) tiles, so the prefix P(J) = J (8 H - 28) - 32 J (J - 1) is inverted in
// closed form; a last column of H % 8 tile columns holds a small triangle.
__device__ __forceinline__ void blocked_tri_decode(int p, int H, int& u, int& v) {
    const int Sf = H >> 3;                                   // full 8-wide super-tile columns
    auto prefix = [&](int J) { return (long)J * (8 * H - 28) - 32l * J * (J - 1); };
    const double b = 8.0 * H + 4.0;
    const double disc = b * b - 128.0 * (double)p;
    int J = (int)((b - __builtin_sqrt(disc > 0.0 ? disc : 0.0)) * (1.0 / 64.0));
    if (J < 0) J = 0;
    if (J > Sf) J = Sf;
    while (J > 0 && prefix(J) > p) --J;
    while (J < Sf && prefix(J + 1) <= p) ++J;
    const int q = p - (int)prefix(J);
    if (J == Sf) {                                           // the ragged last column: a triangle of H % 8 tile columns
        int uu, vv;
        tri_decode(q, H & 7, uu, vv);
        u = 8 * J + uu;
        v = 8 * J + vv;
        return;
    }
    if (q < 36) {                                            // diagonal super-tile: the lower triangle of 8 x 8
        int uu, vv;
        tri_decode(q, 8, uu, vv);
        u = 8 * J + uu;
        v = 8 * J + vv;
        return;
    }
    const int below = H - 8 * J - 8, nfull = below >> 3, q2 = q - 36;
    int grp = q2 >> 6;
    if (grp < nfull) {
        const int w = q2 & 63;
        u = 8 * J + 8 + 8 * grp + (w & 7);
        v = 8 * J + (w >> 3);
    } else {                                                 // the last, shorter group of rows
        const int rl = below & 7, w = q2 - 64 * nfull;
        u = 8 * J + 8 + 8 * nfull + w % rl;
        v = 8 * J + w / rl;
    }
}

template <typename T>
__device__ __forceinline__ void gemm_tile_decode(const GemmArgs<T>& g, int t, int r0, int c0, int nrect, int& ti, int& tj) {
    const int H = g.r1 - r0;
    if (!g.tri || t < nrect) {
        tj = c0 + t / H;
        ti = r0 + t % H;
    } else {
        int u, v;
        tri_decode(t - nrect, H, u, v);        // u >= v in an H x H triangle anchored at (r0, r0)
        ti = r0 + u;
        tj = r0 + v;
    }
}

// element offset of (k, row) inside one staged operand tile
template <typename T> __device__ __forceinline__ int lds_off(int k, int row);
template <> __device__ __forceinline__ int lds_off<double>(int k, int row) { return k * LDT + row; }
template <> __device__ __forceinline__ int lds_off<float>(int k, int row) {
    return ((k >> 2) * 2 + (k & 1)) * LDP + ((k >> 1) & 1) * TB + row;
}

// ROLE only gives each use its own kernel symbol (separate rows in rocprof summaries):
// 0 = trailing SYRK (K = panel*128, the dominant kernel), 1 = in-panel GEMM (K = 128),
// 2 = panel solve X <- X W^T (C = A B^T, A aliases C, one column tile),
// 4 = ROLE 1 + the workgroup of one diagonal tile goes on to factor it (GemmArgs::fuse_b),
// 3 = "NN" form for the backward solve: the J operand is read transposed, B(j,k) at
//     B[k + j*ldb] (k contiguous), through an XOR-swizzled [j][GK] LDS image; g.mode picks
//     C -= A B (0) or C = A B (1).
// NWI x NWJ = wave grid of the workgroup over the 128x128 tile: 2x2 (256 threads, 64x64 per wave, the
// throughput shape) or 4x4 (1024 threads, 32x32 per wave: a quarter of the MFMA chain per wave, for
// the latency-bound launches of the panel stream where tiles <= CUs).
// NBUF = LDS stages: 2 = one stage ahead, vmcnt(0) + barrier per stage (2 workgroups per CU, the
// throughput configuration); 4 = three stages ahead with COUNTED vmcnt waits and a raw s_barrier
// (one workgroup per CU): for launches with <= 1 tile per CU, where a tile pass is bound by the
// DMA round trip of every stage rather than by the MFMA pipe.
#ifndef GP_DIAG
#define GP_DIAG 0          // developer timing experiments only (scripts/micro/syrk_time.hip): 1 = no DMA after the
#endif                     // first two stages, 2 = no C load/store, 4 = no barrier in the main loop (results wrong)
template <typename T, int ROLE, int NWI, int NWJ, int NBUF>
__global__ __launch_bounds__(64 * NWI * NWJ, (NWI * NWJ == 4) ? 2 : 4) void gemm_nt_kernel(GemmArgs<T> g) {
    constexpr int NW = NWI * NWJ, FI = 8 / NWI, FJ = 8 / NWJ;      // MFMA tiles per wave along i / j
    const bool c_tiled = g.c_R > 0, a_tiled = g.a_R > 0, b_tiled = g.b_R > 0;
    extern __shared__ double smem_raw[];       // [2 stages][I tile | J tile]
    T* smem = reinterpret_cast<T*>(smem_raw);
    typedef typename Num<T>::acc_t acc_t;
    constexpr int GK = Num<T>::GK;
    constexpr int STAGE = STAGE_BYTES / (int)sizeof(T);     // elements per stage
    constexpr int JOFF = STAGE / 2;
    constexpr bool F64 = sizeof(T) == 8;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave % NWI, wj = wave / NWI;
    int slot = blockIdx.y;
    int bid = blockIdx.x;
    int ti, tj;
    int r0 = g.r0, c0 = g.c0, nrect = g.nrect, ntiles = g.ntiles;
    if (g.grp_stride > 0) {
        // grouped launch, ONE dense 1-D grid over all groups: group q holds the tile columns [c0 + q stride, + width)
        // (clipped to c1) from its own diagonal down to r1, i.e. T(q) = w H_q - w(w-1)/2 tiles with H_q = H_0 - q stride.
        // The prefix P(q) = q (B + a) - a q^2  (B = w H_0 - w(w-1)/2, a = w stride / 2) is inverted in closed form.
        slot = 0;
        const int w = g.grp_width, st = g.grp_stride, H0 = g.r1 - g.c0;
        const double a = 0.5 * w * st, B = (double)w * H0 - 0.5 * w * (w - 1);
        auto prefix = [&](int q) { return (long)q * (long)(w * H0 - w * (w - 1) / 2) - (long)w * st * ((long)q * (q - 1) / 2); };
        const double disc = (B + a) * (B + a) - 4.0 * a * (double)bid;
        int q = (int)(((B + a) - __builtin_sqrt(disc > 0.0 ? disc : 0.0)) / (2.0 * a));
        if (q < 0) q = 0;
        if (q > g.grp_count - 1) q = g.grp_count - 1;
        while (q > 0 && prefix(q) > bid) --q;
        while (q + 1 < g.grp_count && prefix(q + 1) <= bid) ++q;
        bid -= (int)prefix(q);
        c0 = g.c0 + q * st;
        const int c1 = (c0 + w < g.c1) ? c0 + w : g.c1;
        r0 = c0;
        const int H = g.r1 - r0, ntc = c1 - c0;
        nrect = 0;
        ntiles = ntc * H - ntc * (ntc - 1) / 2;
        if (bid >= ntiles) return;             // (only the clipped last group can come up short)
    }
    if (g.super == 2) {
        // BALANCED blocked order: the tile list itself is enumerated super-tile by super-tile (8 x 8 tiles: 8 row panels + 8
        // column panels = 16 operand panels for 64 tiles, instead of 65 for 64 tiles down a column), and every XCD takes a
        // contiguous, equally long chunk of that list as with the plain swizzle -- whole super-tiles pass through an XCD's
        // private L2 without the static super-tile-per-XCD split whose unequal loads cost more than the traffic saved.
        const int H = g.r1 - g.r0;
        {
            const int nx = 8, n = ntiles;
            const int q = n / nx, rem = n % nx, x = bid % nx, o = bid / nx;
            bid = (x < rem ? x * (q + 1) : rem * (q + 1) + (x - rem) * q) + o;
        }
        int u, v;
        blocked_tri_decode(bid, H, u, v);
        ti = g.r0 + u;
        tj = g.r0 + v;
    } else {
        if (g.swizzle) {                       // give each XCD a contiguous chunk of the tile list
            const int nx = 8, n = ntiles;
            const int q = n / nx, rem = n % nx, x = bid % nx, o = bid / nx;
            bid = (x < rem ? x * (q + 1) : rem * (q + 1) + (x - rem) * q) + o;
        }
        gemm_tile_decode(g, bid, r0, c0, nrect, ti, tj);
    }
    // the decode goes through a floating-point square root, i.e. the vector ALU: hand the (wave-uniform) tile indices back
    // to the scalar unit, or every tile address below -- one per operand and LDS stage -- is 64-bit VECTOR arithmetic
    // issued between the MFMAs (measured: -1.8 % on the trailing SYRK)
    ti = __builtin_amdgcn_readfirstlane(ti);
    tj = __builtin_amdgcn_readfirstlane(tj);
    slot = __builtin_amdgcn_readfirstlane(slot);

    const long koff = g.ktri ? (long)ti * TB : 0;          // first k of this tile's contraction
    const T* Abase = g.A + (long)slot * g.a_bstride;
    const T* Bbase = g.B + (long)slot * g.b_bstride;
    const long lda = a_tiled ? (long)TB : g.lda, ldb = b_tiled ? (long)TB : g.ldb;
    // address of A(ti*128, k) / B(tj*128, k) (ROLE 3: of B(j = tj*128, k) = L(.. + k, tj*128)) for a stage start k; a stage
    // (GK columns) never straddles a k-tile
    auto a_at = [&](long k) -> const T* {
        if (a_tiled) return Abase + tile_index(ti, g.a_k0 + (int)(k >> 7), g.a_R) * TS + (k & 127) * TB;
        return Abase + (long)ti * TB + k * g.lda;
    };
    auto b_at = [&](long k) -> const T* {
        if (ROLE == 3) {
            if (b_tiled) return Bbase + tile_index(g.b_k0 + (int)(k >> 7), tj, g.b_R) * TS + (k & 127);
            return Bbase + (long)tj * TB * g.ldb + k;
        }
        if (b_tiled) return Bbase + tile_index(tj, g.b_k0 + (int)(k >> 7), g.b_R) * TS + (k & 127) * TB;
        return Bbase + (long)tj * TB + k * g.ldb;
    };
    // Staging: LDS-DMA (global_load_lds_dwordx4), no staging registers and no ds_write pass.  One
    // wave-instruction moves 1 KiB landing lane-linear at a wave-uniform LDS base: fp64 = one
    // k-column of 128 rows; fp32 = the two k-columns of one pair (lanes 0-31 / 32-63).  Wave w
    // issues instructions w, w+4, w+8, w+12 of both tiles.
    const int uw = __builtin_amdgcn_readfirstlane(wave);
    // Stages are issued strictly in order kb = 0, 1, 2, ..: the operand addresses are RUNNING scalar pointers (one add per
    // stage; at a k-tile boundary of a tiled operand one jump to the next tile of the row: tile (ti, kt + 1) follows tile
    // (ti, kt) by R - kt - 1 tiles, and for ROLE 3's transposed J operand tile (kt + 1, tj) follows (kt, tj) directly)
    const T* a_run = a_at(koff);
    const T* b_run = b_at(koff);
    int a_left = a_tiled ? g.a_R - (g.a_k0 + (int)(koff >> 7)) - 1 : 0;       // tiles from (ti, kt) to (ti, kt + 1)
    int b_left = b_tiled ? g.b_R - (g.b_k0 + (int)(koff >> 7)) - 1 : 0;
    int kin = 0;                                                               // columns of the current k-tile already staged
    auto stage = [&](int kb, int st) {
        (void)kb;
        T* Is = smem + st * STAGE;
        T* Js = Is + JOFF;
        const T* Ag = a_run;                       // column kb*GK of this tile's contraction, row 0 of the tile
        const T* Bg = b_run;
        a_run += (long)GK * lda;
        b_run += (ROLE == 3) ? (long)GK : (long)GK * ldb;
        kin += GK;
        if (kin == TB) {
            kin = 0;
            if (a_tiled) { a_run += (long)a_left * TS - (long)TB * TB; --a_left; }
            if (b_tiled) {
                if (ROLE == 3) b_run += TS - TB;
                else { b_run += (long)b_left * TS - (long)TB * TB; --b_left; }
            }
        }
#pragma unroll
        for (int s = 0; s < (NW >= 16 ? 1 : 16 / NW); ++s) {
            const int q = uw + NW * s;          // instruction index 0..15 within the stage
            if (F64) {
                const long kcol = q;
                __builtin_amdgcn_global_load_lds((glb_void*)(Ag + kcol * lda + 2 * lane),
                                                 (lds_void*)(Is + q * LDT), 16, 0, 0);
                if (ROLE != 3)
                    __builtin_amdgcn_global_load_lds((glb_void*)(Bg + kcol * ldb + 2 * lane),
                                                     (lds_void*)(Js + q * LDT), 16, 0, 0);
            } else {
                // pair q holds columns k0 = 4(q>>1) + (q&1) (lanes 0-31) and k0 + 2 (lanes 32-63)
                const long kcol = 4 * (q >> 1) + (q & 1) + 2 * (lane >> 5);
                const int row = 4 * (lane & 31);
                __builtin_amdgcn_global_load_lds((glb_void*)(Ag + kcol * lda + row),
                                                 (lds_void*)(Is + q * LDP), 16, 0, 0);
                if (ROLE != 3)
                    __builtin_amdgcn_global_load_lds((glb_void*)(Bg + kcol * ldb + row),
                                                     (lds_void*)(Js + q * LDP), 16, 0, 0);
            }
            if (ROLE == 3) {
                // transposed source: instruction q covers j = 8q..8q+7; lane -> (j, 16-byte k-group);
                // image Js[j*GK + G*((k/G) ^ (j&7)) + k%G], G = elements per 16 B (swizzle on the source)
                constexpr int G = 16 / (int)sizeof(T);
                const int j = 8 * q + (lane >> 3), kg = (lane & 7) ^ (j & 7);
                __builtin_amdgcn_global_load_lds((glb_void*)(Bg + G * kg + (long)j * ldb),
                                                 (lds_void*)(Js + q * 8 * GK), 16, 0, 0);
            }
        }
    };

    // C tile: lane holds i = i0 + y*16 + (lane&15), j = j0 + x*16 + drow(lane>>4, r)
    const long ldc = c_tiled ? (long)TB : g.ldc;
    T* Cg = g.C + (long)slot * g.c_bstride +
            (c_tiled ? (tile_index(ti, tj, g.c_R) + (g.c_adj ? g.c_adj[panel_slot(tj, g.c_R - 1, g.c_adj_panel)] : 0l)) * TS
                     : (long)tj * TB * g.ldc + (long)ti * TB) +
            (long)(wj * (16 * FJ)) * ldc + wi * (16 * FI) + (lane & 15);
    const int l4 = lane >> 4;
    const int nk = (g.K - (int)koff) / GK;
    // Update roles start the accumulators AT C and feed the MFMA the negated J fragment, so acc ends
    // as C - A B^T and the epilogue is stores only.
    const bool from_zero = (ROLE == 2) || (ROLE == 3 && g.mode == 1);
    acc_t acc[FJ][FI];
    // MFMA row-tiles (of FI) this wave really has to compute -- wave-uniform, decided once:
    //   thin row tile: only row 0 of the 128 bordered rows is non-zero -> wave column wi = 0 computes its first
    //     16-row MFMA tile (FJ MFMAs per k-group instead of FJ*FI), wave column wi = 1 none; the skipped rows are
    //     zero in memory and are neither loaded nor stored;
    //   diagonal tile of a triangular update: the wave that owns the strictly-upper quadrant computes nothing.
    // A skipping wave still stages its share of the LDS-DMA and meets every barrier.
    int ny = FI;
    if (NW == 4) {
        const int uwi = uw % NWI, uwj = uw / NWI;
        if (g.thin_row == ti) ny = (uwi == 0) ? 1 : 0;
        else if (g.skip_upper && g.tri && ti == tj && uwi == 0 && uwj == 1) ny = 0;
    }
    auto load_c = [&](auto nyc) {
        constexpr int NY = decltype(nyc)::value;
#pragma unroll
        for (int x = 0; x < FJ; ++x)
#pragma unroll
            for (int y = 0; y < FI; ++y) {
                if (from_zero || (GP_DIAG & 2) || y >= NY) {
                    acc[x][y] = (acc_t){0, 0, 0, 0};
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        acc[x][y][r] = Cg[(long)(x * 16 + Num<T>::drow(l4, r)) * ldc + y * 16];
                }
            }
    };
    // Fragments of one k-group of 4: lane (l15, l4) holds I[i = .. + l15][k = 4 kk + l4] and the
    // same of J.  load_frags only ISSUES the LDS reads; the J fragment is negated where it is used
    // so that nothing has to wait for the reads at issue time.
    auto load_frags = [&](int buf, int kk, T* fi, T* fj) {
        const T* Is = smem + buf * STAGE + wi * (16 * FI) + (lane & 15);
        const T* Js = smem + buf * STAGE + JOFF;
        const int k = 4 * kk + l4;
#pragma unroll
        for (int f = 0; f < FI; ++f) fi[f] = Is[lds_off<T>(k, f * 16)];
#pragma unroll
        for (int f = 0; f < FJ; ++f) {
            const int jrow = wj * (16 * FJ) + f * 16 + (lane & 15);
            if (ROLE == 3) {
                constexpr int G = 16 / (int)sizeof(T);
                fj[f] = Js[jrow * GK + G * ((k / G) ^ (jrow & 7)) + (k % G)];
            } else {
                fj[f] = Js[lds_off<T>(k, jrow)];
            }
        }
    };
    // While an LDS-DMA is in flight hipcc only ever waits with lgkmcnt(0), i.e. for ALL outstanding
    // LDS reads.  An empty asm that "uses" a fragment set makes that wait happen at a chosen point:
    // before the next set's reads are issued instead of after.
    auto pin_frags = [&](T* fi, T* fj) {
#pragma unroll
        for (int f = 0; f < FI; ++f) asm volatile("" : "+v"(fi[f]));
#pragma unroll
        for (int f = 0; f < FJ; ++f) asm volatile("" : "+v"(fj[f]));
    };
    // kfirst = first k of this k-group (ROLE 2 with a lower-triangular J operand only: see GemmArgs::b_lower)
    const int jbase = (uw / NWI) * (16 * FJ) + 15;           // last column of this wave's first 16-column group
    auto mfma_block = [&](const T* fi, const T* fj, auto nyc, int kfirst) {
        constexpr int NY = decltype(nyc)::value;
        T nj[FJ];
#pragma unroll
        for (int f = 0; f < FJ; ++f) nj[f] = from_zero ? fj[f] : -fj[f];
        if constexpr (ROLE == 2) {
            // column group x holds j <= jbase + 16 x: all of its B(j, k) are zero once k > that
            const int d = g.b_lower ? kfirst - jbase : 0;
            const int xskip = d > 0 ? (d + 15) >> 4 : 0;
#pragma unroll
            for (int x = 0; x < FJ; ++x)
                if (x >= xskip) {
#pragma unroll
                    for (int y = 0; y < NY; ++y) acc[x][y] = Num<T>::mfma(nj[x], fi[y], acc[x][y]);
                }
        } else {
#pragma unroll
            for (int x = 0; x < FJ; ++x)
#pragma unroll
                for (int y = 0; y < NY; ++y) acc[x][y] = Num<T>::mfma(nj[x], fi[y], acc[x][y]);
        }
    };
    auto compute = [&](int buf, int kb) {
        T fi[FI], fj[FJ];
#pragma unroll
        for (int kk = 0; kk < GK / 4; ++kk) {
            load_frags(buf, kk, fi, fj);
            mfma_block(fi, fj, std::integral_constant<int, FI>{}, kb * GK + 4 * kk);
        }
    };
    if constexpr (NBUF == 2) {
        // Software pipeline over k-groups: the LDS reads of group kk+1 are issued BEFORE the 16 MFMAs
        // of group kk (two fragment register sets), and the first group of the next stage is read
        // right after the barrier, under the last group's MFMAs -- no LDS latency is exposed.
        constexpr int NKK = GK / 4;
        static_assert(NKK % 2 == 0, "fragment set parity must repeat every stage");
        auto pipeline = [&](auto nyc) {
            constexpr int NY = decltype(nyc)::value;
            T fa[2][FI], fb[2][FJ];
#ifdef GP_STAGGER
            if (ROLE == 0 && (blockIdx.x & 256) && blockIdx.x < 512)
                for (int i = 0; i < GP_STAGGER; ++i) __builtin_amdgcn_s_sleep(127);
#endif
            stage(0, 0);
            load_c(nyc);                                       // C loads fly with the first DMA stage
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (NY > 0) load_frags(0, 0, fa[0], fb[0]);
            for (int kb = 0; kb < nk; ++kb) {
                const int cur = kb & 1;
                if (kb + 1 < nk && !((GP_DIAG & 1) && kb >= 1)) stage(kb + 1, cur ^ 1);   // DMA of the next stage flies under the MFMAs
                if (NY > 0) {
#pragma unroll
                    for (int kk = 0; kk + 1 < NKK; ++kk) {
                        pin_frags(fa[kk & 1], fb[kk & 1]);     // the compiler's LDS wait lands HERE ...
                        __builtin_amdgcn_sched_barrier(0);
                        load_frags(cur, kk + 1, fa[(kk + 1) & 1], fb[(kk + 1) & 1]);   // ... before these reads
                        __builtin_amdgcn_sched_barrier(0);
                        mfma_block(fa[kk & 1], fb[kk & 1], nyc, kb * GK + 4 * kk);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    // every read of this stage has landed: once this wave's DMA has too, the barrier both
                    // publishes the next stage and frees this buffer for the DMA after next
                    pin_frags(fa[(NKK - 1) & 1], fb[(NKK - 1) & 1]);
                }
                if (!(GP_DIAG & 8)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (!(GP_DIAG & 4)) __builtin_amdgcn_s_barrier();
                if (NY > 0) {
                    if (kb + 1 < nk) load_frags(cur ^ 1, 0, fa[0], fb[0]);
                    __builtin_amdgcn_sched_barrier(0);
                    mfma_block(fa[(NKK - 1) & 1], fb[(NKK - 1) & 1], nyc, kb * GK + 4 * (NKK - 1));
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            // epilogue: stores only
            if ((GP_DIAG & 2) && acc[0][0][0] != (typename Num<T>::acc_t){1, 2, 3, 4}[0]) return;
#pragma unroll
            for (int x = 0; x < FJ; ++x)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    T* cp = Cg + (long)(x * 16 + Num<T>::drow(l4, r)) * ldc;
#pragma unroll
                    for (int y = 0; y < NY; ++y) cp[y * 16] = acc[x][y][r];
                }
        };
        if (ny == FI) pipeline(std::integral_constant<int, FI>{});
        else if (ny == 1) pipeline(std::integral_constant<int, 1>{});
        else pipeline(std::integral_constant<int, 0>{});
        if constexpr (ROLE == 4 && NW == 4) {
            if (g.fuse_b >= 0 && ti == g.fuse_b && tj == g.fuse_b) {
                // accumulators (= the fully updated diagonal tile) -> tile-packed LDS image of the lower triangle, then the
                // potrf128 body: L over the tile just stored, W_b, log-det partial, SPD verdict
                __syncthreads();                               // every wave is done with the stage buffers
                T* Ls = reinterpret_cast<T*>(smem_raw + 2);
                if (ny == FI) {
#pragma unroll
                    for (int x = 0; x < FJ; ++x)
#pragma unroll
                        for (int y = 0; y < FI; ++y) {
                            const int bi = wi * FI + y, bj = wj * FJ + x;
                            if (bi >= bj) {
#pragma unroll
                                for (int r = 0; r < 4; ++r) Ls[ptile(bi, bj) + Num<T>::drow(l4, r) * 16 + (lane & 15)] = acc[x][y][r];
                            }
                        }
                }
                __syncthreads();
                T* Ct = Cg - ((long)(wj * (16 * FJ)) * ldc + wi * (16 * FI) + (lane & 15));        // tile base
                potrf128_core_call<T, 8>(Ct, ldc, g.fuse_W + ((long)slot * g.fuse_nt + g.fuse_b) * TB * TB,
                                         g.fuse_partial + (long)slot * g.fuse_nt + g.fuse_b, g.fuse_info + slot,
                                         (T)g.fuse_slotp[(long)slot * SLOTP + 3], nullptr, 0, nullptr, nullptr, false);
            }
        }
        return;
    } else {
        // deep pipeline: NBUF-1 stages in flight; every wave issues IPS DMA instructions per stage
        constexpr int AHEAD = NBUF - 1;
        constexpr int IPS = 2 * ((16 + NW - 1) / NW);      // I + J instructions per wave per stage
        static_assert(NBUF == 4 && IPS == 2, "counted waits below are written for 4 buffers, 16 waves");
        load_c(std::integral_constant<int, FI>{});
        for (int st = 0; st < AHEAD && st < nk; ++st) stage(st, st);
        for (int kb = 0; kb < nk; ++kb) {
            const int rem = nk - 1 - kb;                   // stages issued beyond kb (capped at AHEAD-1)
            if (rem >= 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else if (rem == 1) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                  // stage kb landed for every wave; buffer (kb-1)%4 is free
            if (kb + AHEAD < nk) stage(kb + AHEAD, (kb + AHEAD) % NBUF);
            compute(kb % NBUF, kb);
        }
    }

    // epilogue: stores only
    if ((GP_DIAG & 2) && acc[0][0][0] != (typename Num<T>::acc_t){1, 2, 3, 4}[0]) return;
#pragma unroll
    for (int x = 0; x < FJ; ++x)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            T* cp = Cg + (long)(x * 16 + Num<T>::drow(l4, r)) * ldc;
#pragma unroll
            for (int y = 0; y < FI; ++y) cp[y * 16] = acc[x][y][r];
        }
}

// ---------------------------------------------------------------------------------------------
// chol_dataflow: the whole bordered Cholesky of small / mid problems in ONE launch.
//
// The multi-kernel schedule above is bound, below N ~ 8k, by the serial chain of dependent launches
// (potrf -> panel solve -> in-panel update, ~115 us per 128 columns).  Here every TBX x TBX tile (i,j),
// i >= j, of the bordered matrix (tile row nd = the rhs rows) is ONE workgroup that owns the tile for
// its whole life (left-looking):
//     acc  = K(i,j)
//     for b < j:  wait X(i,b), X(j,b);  acc -= X(i,b) X(j,b)^T          (K = TBX slab on the MFMA)
//     i == j:     L_jj, W_j = potrf128(acc);                 publish ready(j,j)
//     i >  j:     wait ready(j,j);  X(i,j) = acc W_j^T;      publish ready(i,j)
// With 64x64 tiles (fp64) the critical chain is fused: the diagonal task (j,j) also solves its own
// sub-diagonal tile (j,j-1) -- whose owner only accumulates it, stores the pre-solve tile and raises a
// "pre" flag kept in the unused upper slot (j-1,j) -- and applies that last slab from LDS images of
// the freshly solved tile: one flag hop per column on the chain instead of two.
// Dependencies are flags in global memory (value = epoch of this evaluation; write-through tile
// stores + an agent-scope fence before the flag store, acquire after the poll).  One wave per
// workgroup polls; a task first peeks at all its column flags in parallel and consumes the leading
// run of finished columns without further polls.  Tasks are numbered in column-major order, a topological order of the DAG, and a
// workgroup takes its task number from an atomic ticket when it STARTS: every dependency of a task
// therefore belongs to a workgroup that started earlier and is resident, so the schedule cannot
// deadlock whatever order the hardware dispatches workgroups in.  A spin limit turns any violation of
// that argument into an error code (abort flag) instead of a hung GPU.
// ---------------------------------------------------------------------------------------------
template <typename T>
struct DfArgs {
    T* A; long bstride;                       // packed tile-major workspace (slot 0 base), elements between slots
    int R128, c0;                             // R128 = Nt + 1 tile rows of the workspace (128-tiles); c0 = first tile column
                                              // (in TBX units) of the trailing submatrix this launch factors
    T* W; long w_bstride;                     // W_b = L_bb^-1 blocks, [slot][nd][TBX*TBX]
    double* partial; long p_bstride;          // sum log L_jj per diagonal block, [slot * p_bstride + j]
    int* info;                                // [slot]
    const double* slotp;
    int* flags; long f_bstride;               // [slot][(nd+1)^2]: ready(i,j) at i*(nd+1)+j
    unsigned long long* ticket;
    unsigned long long ticket_base;           // value of *ticket before this launch
    int* abort_flag;
    int nd, nslots, epoch;                    // nd = diagonal blocks = Npad / TBX; tile row nd = the rhs rows
    int ncols;                                // tile columns this launch factors (0 = all): a launch restricted to the columns of ONE outer
                                              // panel of the sharded schedule contains no diagonal task for the column behind its last one
    int nprev; long task0; const T* Aprev;    // sharded schedule, fused look-ahead: the first nprev tile columns of the submatrix are a
                                              // FINISHED outer panel (operands only, read through Aprev -- the owner's receive buffer,
                                              // addressed with the same global tile indices); task numbering starts at task0 = the
                                              // first task of column nprev.  The launch applies that panel to its own columns itself.
    unsigned int* colsig;                     // sharded schedule, panel launch (ncols > 0), or null: per 128-tile column of the panel a counter of
                                              // FINISHED 64 x 64 tiles -- every task adds one for each tile it has made final (its own; the
                                              // diagonal task also the sub-diagonal tile it solves) AFTER that tile's write-through stores
                                              // have drained.  The owner's communication stream waits for the column's tile count
                                              // (hipStreamWaitValue32) and sends the column while the launch is still factoring the next ones.
    int* park;                                // 64-tiles, two workgroups per CU: [DF_PARK_SLOTS] counters "a chain task is in its critical
                                              // section on this CU" (index = XCC / SE / SH / CU id); the neighbour sleeps meanwhile; or null
    T* D; long d_bstride;                     // 64-tiles: the 16x16 diagonal inverses of every 64-block, [slot][nd][4][col * 16 + row] -- with L_jj what the
                                              // NEXT hop of the chain needs (its sub-diagonal solve is a blocked substitution), handed over under
                                              // the chain flag (j, j+2) BEFORE the off-diagonal blocks of W_j are even computed; null: the chain
                                              // waits for W_j like everybody else
    T* U; long ldu;                           // INVERSE launch (gradient, K^-1 = U U^T): the factor is final, every task is a tile of
                                              // U = L^-T (column-major, leading dimension ldu, pre-zeroed):  U(rb,cb), rb <= cb, =
                                              // (E - sum_{k=rb}^{cb-1} U(rb,k) L(cb,k)^T) W_cb^T.  Tasks in column order (cb, then
                                              // rb), nd (nd + 1) / 2 of them, one slot; the flag matrix serves U's own hand-overs
                                              // (ready(rb,cb) at rb * (nd + 1) + cb, a fresh epoch).  null: the factorisation
    int u_rows;                               // > 0: FORWARD launch -- U is a dense block of u_rows row blocks x nd column blocks that holds
                                              // right-hand sides as ROWS (test-point covariances k*^T); every task turns one tile into
                                              // the same tile of U L^-T: U(rb,cb) = (U(rb,cb) - sum_{k<cb} U(rb,k) L(cb,k)^T) W_cb^T,
                                              // in place.  Tasks in column order, u_rows * nd of them; needs u_rows <= nd + 1
    long u_bstride;                           // forward launch over several slots (gphip_predict_samples): elements between the slots' U blocks
    const T* LT; int u_back;                  // BACKWARD launch (u_rows > 0, u_back = 1): the rows of U become U L^-1 -- the second half of a solve with K.
                                              // LT = a copy of the factor whose 64x64 blocks are stored TRANSPOSED in place (tile (k, cb) holds L(k,cb)^T),
                                              // W = the transposed 64-block inverses: with them U(rb,cb) = (U(rb,cb) - sum_{k>cb} U(rb,k) L(k,cb)) W_cb is
                                              // the forward task's recurrence read from the other end (columns nd-1 .. 0)
    long long* trace;                         // developer timing (scripts/micro/df_trace.hip): 8 stamps per task, or null
    // BUILD variant only (one launch per evaluation: tiles built in-kernel, results exported by the corner task)
    const T* xt; const T* yv;                 // unscaled inputs [d][npad], outputs [npad]
    int n, npad, d, kt;                       // true N, padded N, input dimension, kernel family (0 SE, 1 Matern-5/2)
    double* hres; int* hinfo;                 // pinned host: {logdet, quad} per slot; info per slot + abort flag
};

#ifndef GP_DF_DMA_AUX
#define GP_DF_DMA_AUX 16           // cache-policy bits of the dataflow kernel's LDS-DMA operand loads: 16 = sc1 (served by L2 / fabric,
#endif                             // never by the CU's L1), 0 = default policy (then GP_DF_ACQUIRE must be 1)
#ifndef GP_DF_ACQUIRE
#define GP_DF_ACQUIRE 0            // 1 = agent-scope acquire (buffer_inv sc1) after every dependency wait
#endif
static_assert(GP_DF_ACQUIRE || GP_DF_DMA_AUX == 16, "plain operand loads need the acquire after a dependency wait");
constexpr int DF_PARK_SLOTS = 4096;           // 16 XCC ids x 256 (SE, SH, CU) ids
constexpr int DF_SPIN_LIMIT = 1 << 22;        // x ~1 us per poll: seconds, never reached by a live schedule

__device__ __forceinline__ void df_wait(const int* f, int epoch, int* abort_flag) {
    int spins = 0;
    // "unlikely": keeps the register allocator from treating this poll loop as hotter than the MFMA
    // loop it sits in (it would spill accumulators around it)
    while (__builtin_expect(__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != epoch, 0)) {
#ifndef GP_DF_POLL_SLEEP
#define GP_DF_POLL_SLEEP 8
#endif
        __builtin_amdgcn_s_sleep(GP_DF_POLL_SLEEP);         // (a longer back-off for long waits was measured: no gain)
        if ((++spins & 63) == 0) {
            if (__hip_atomic_load(abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) break;
            if (spins > DF_SPIN_LIMIT) {
                __hip_atomic_store(abort_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;                          // carry on with whatever is there: no divergent exits
            }
        }
    }
    // No agent-scope acquire (L1 invalidate) here since round 4: every tile another workgroup produced inside this launch is
    // stored write-through (sc1) and read back by LDS-DMA loads that carry the sc1 policy bit themselves (GP_DF_DMA_AUX: they
    // are served by the L2 / fabric, never by this CU's L1) -- MI355X_MICROARCH.md: "sc1 loads may replace the acquire only
    // when the producer stored sc1".  With PLAIN operand loads the acquire is indispensable (measured: -DGP_DF_DMA_AUX=0
    // -DGP_DF_ACQUIRE=0 gives wrong likelihoods within seconds of scripts/gpu_df_soak.py).  -2 % at N = 2048-8192.
    if (GP_DF_ACQUIRE) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

// LDS image of one staged operand tile of the dataflow kernel.  TBX = 128: the gemm_nt image.
// TBX = 64 (fp64 only): one LDS-DMA instruction carries the 64 rows of k-columns {k0, k0+2}
// (lanes 0-31 / 32-63), instruction q = 2 (k>>2) + (k&1) lands at q * 144 doubles -- the same pair
// trick as the fp32 image, so MFMA fragment reads stay bank-conflict free.
constexpr int LD64 = 144;
template <typename T, int TBX> __device__ __forceinline__ int df_lds_off(int k, int row) {
    if constexpr (TBX == 128) return lds_off<T>(k, row);
    else return ((k >> 2) * 2 + (k & 1)) * LD64 + ((k >> 1) & 1) * 64 + row;
}
// k-columns per LDS stage of the 64-tile kernel (GP_DF_GK64: 16 = one quarter of a slab, the gemm_nt stage depth; 32 = half a
// slab: half as many DMA-wait + barrier points per MFMA, 72 KiB of LDS per workgroup -- still two per CU)
#ifndef GP_DF_GK64
#define GP_DF_GK64 16
#endif
template <typename T, int TBX> constexpr int df_stage_k() { return TBX == 128 ? Num<T>::GK : GP_DF_GK64; }
template <typename T, int TBX> constexpr int df_stage_elems() {
    return TBX == 128 ? STAGE_BYTES / (int)sizeof(T) : 2 * (GP_DF_GK64 / 2) * LD64;
}
// NST = LDS stages of the slab pipeline: 2 (double buffer), or 4 with counted DMA waits for a workgroup that
// has the CU to itself (fp64 128-tiles) while the schedule is chain bound: its on-chain products have no
// co-resident workgroup to hide the DMA latency behind (N=4096 -6 %; at N=8192, throughput bound, +4 %).
// 64-tiles, builds with at most two workgroups per CU (DF_XXF): the potrf image lives BEHIND the stage area, so that it can be
// filled before the chain's solve and updated block by block while the X images are still in place (diagx)
constexpr int DF_XXF_POTRF_AT = 32 * LD64 + 1024;            // doubles from the start of the dynamic LDS: [stage / L image / X images | inverses | potrf image]
constexpr size_t DF_XXF_LDS = (size_t)(DF_XXF_POTRF_AT + 2 + PT64_S + 256) * 8;
template <typename T, int TBX, int NST = 2> constexpr size_t df_lds_bytes() {
    constexpr size_t gemm = NST * (size_t)df_stage_elems<T, TBX>() * sizeof(T);
    constexpr size_t nb = TBX / 16;
    constexpr size_t potrf = 16 + (nb * (nb + 1) / 2 * 256 + TBX + (TBX == 64 ? (nb + 1) * 256 : 0)) * sizeof(T);
    constexpr size_t chain = TBX == 64 ? (size_t)(32 * LD64 + 1024) * sizeof(T) : 0;   // L tile image + diagonal inverses (diagx)
    return (gemm > potrf ? gemm : potrf) > chain ? (gemm > potrf ? gemm : potrf) : chain;
}

// OCC = workgroups per CU the register budget is sized for: 2 (256 registers: 64-tiles, fp32 128-tiles) or
// 1 (512 registers: fp64 128-tiles -- 128 accumulator registers plus the out-of-line potrf body do not fit
// in 256 without spilling accumulators around every slab).
// BUILD: the evaluation is this ONE launch -- every task builds its own tile of K(theta) from the resident
// inputs (same arithmetic as kbuild_kernel, hyper-parameters passed by value), and the corner task, which
// depends on everything, reduces log det / quadratic form and writes them to pinned host memory.
template <typename T, int TBX, int OCC = 2, int NST = 2, bool BUILD = false>
__global__ __launch_bounds__(256, OCC) void chol_dataflow_kernel(DfArgs<T> g, ThetaPack tp) {
    static_assert(TBX == 128 || (TBX == 64 && sizeof(T) == 8), "64-tiles are implemented for fp64 only");
    constexpr int FI = TBX / 32, FJ = TBX / 32, WT = TBX / 2;   // MFMA tiles per wave, wave tile edge
    extern __shared__ double smem_raw[];
    __shared__ int s_task;
    __shared__ int s_known;                                // (NOT s_task again: wave 0 could write the peek's result there before a slow wave
                                                           //  has read its ticket -- waves of one workgroup on different tasks = mismatched barriers = a hung launch)
    __shared__ int s_park;
    T* smem = reinterpret_cast<T*>(smem_raw);
    typedef typename Num<T>::acc_t acc_t;
    constexpr int GK = df_stage_k<T, TBX>();
    constexpr int STAGE = df_stage_elems<T, TBX>();
    constexpr int JOFF = STAGE / 2;
    constexpr bool F64 = sizeof(T) == 8;
    constexpr int SPB = TBX / GK;                           // LDS stages per TBX-wide slab
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave & 1, wj = wave >> 1;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int uw = __builtin_amdgcn_readfirstlane(wave);

    if (tid == 0) s_task = (int)(atomicAdd(g.ticket, 1ull) - g.ticket_base);
    __syncthreads();
    const int task = __builtin_amdgcn_readfirstlane(s_task);
    const int R = g.nd + 1;
    const int slot = task % g.nslots, q = task / g.nslots + (int)g.task0;
    // q -> (j, i): column-major over the lower triangle, column j starts at off(j) = jR - j(j-1)/2.
    int j = (int)(((double)(2 * R + 1) - sqrt((double)(2 * R + 1) * (2 * R + 1) - 8.0 * q)) * 0.5);
    if (j < 0) j = 0;
    if (j > R - 1) j = R - 1;
    while (j + 1 < R && (j + 1) * R - (j + 1) * j / 2 <= q) ++j;
    while (j > 0 && j * R - j * (j - 1) / 2 > q) --j;
    int i = j + (q - (j * R - j * (j - 1) / 2));
    j = __builtin_amdgcn_readfirstlane(j);                 // (through the vector sqrt: back to the scalar unit)
    i = __builtin_amdgcn_readfirstlane(i);

#ifdef GPHIP_TIMING
    if (threadIdx.x == 0 && g_stamp_buf) g_stamp_buf[(long)blockIdx.x * 64 + 63] = task;
#endif
    long long* tr = g.trace ? g.trace + (long)task * 8 : nullptr;
    auto stamp = [&](int k) { if (tr && tid == 0) tr[k] = wall_clock64(); };
    stamp(0);
    // The diagonal task IS the critical chain (and with 64-tiles the sub-diagonal one feeds it): let the SIMD arbiter
    // prefer their waves over the co-resident workgroup's accumulation waves (N=8192: 5.2 -> 4.9 ms)
#ifndef GP_DF_PRIO
#define GP_DF_PRIO 3
#endif
    const bool inverse = g.U != nullptr;
    if (inverse && g.u_rows > 0) {                          // forward launch: q = cb * u_rows + rb; backward: columns from the last one
        const int cq = q / g.u_rows;
        i = __builtin_amdgcn_readfirstlane(g.u_back ? g.nd - 1 - cq : cq);
        j = __builtin_amdgcn_readfirstlane(q % g.u_rows);
    } else if (inverse) {                                   // task q -> (rb, cb), rb <= cb, column cb first: q = cb (cb + 1) / 2 + rb
        int cb = (int)((sqrt(8.0 * (double)q + 1.0) - 1.0) * 0.5);
        while ((long)(cb + 1) * (cb + 2) / 2 <= q) ++cb;
        while (cb > 0 && (long)cb * (cb + 1) / 2 > q) --cb;
        i = __builtin_amdgcn_readfirstlane(cb);             // i = column block cb, j = row block rb: tile (i, j) of L exists
        j = __builtin_amdgcn_readfirstlane((int)(q - (long)cb * (cb + 1) / 2));
    }
    if (GP_DF_PRIO > 0 && !inverse && (i == j || (TBX == 64 && i == j + 1))) __builtin_amdgcn_s_setprio(GP_DF_PRIO);
    // Per-phase stamps (scripts/micro/df_phases.hip) show every phase of a diagonal task's potrf / solve running 1.6-1.8x slower
    // next to a co-resident workgroup's back-to-back MFMAs (and at its stand-alone pace with the CU to itself).  So while a
    // diagonal task is in its critical section -- dependencies met, nothing but its own work between it and ready(j,j) -- it
    // raises a counter keyed by its CU, and the neighbour workgroup checks that counter once per slab and sleeps while it is
    // up.  A task in its own critical section never sleeps, and a critical section needs nobody else: no deadlock.
    int* parkp = nullptr;
    bool critical = false;
    if constexpr (TBX == 64) {
        if (g.park) {
            const unsigned hw = __builtin_amdgcn_s_getreg((7 << 11) | (8 << 6) | 4);       // HW_ID[15:8] = SE, SH, CU ids
            const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20);     // XCC_ID[3:0]
            parkp = g.park + (((xcc & 15) << 8) | (hw & 255));
        }
    }
    auto enter_critical = [&]() {
        if (parkp && !critical) {
            critical = true;
            if (tid == 0) __hip_atomic_fetch_add(parkp, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    auto leave_critical = [&]() {
        if (parkp && critical) {
            critical = false;
            if (tid == 0) __hip_atomic_fetch_add(parkp, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    T* As = g.A + (long)slot * g.bstride;
    int* F = g.flags + (long)slot * g.f_bstride;
    T* Wj = g.W + (long)slot * g.w_bstride + (long)j * TBX * TBX;
    // TBX-tile (ti, tj) of this launch's submatrix inside the packed tile-major workspace; leading dimension 128
    // either way (a 64-tile is a quadrant of its 128-tile)
    auto tptr = [&](int ti_, int tj_) -> T* {
        const int gi = ti_ + g.c0, gj = tj_ + g.c0;
        T* base = tj_ < g.nprev ? const_cast<T*>(g.Aprev) : As;        // (nprev = 0 outside the sharded schedule)
        if constexpr (TBX == 128) return base + tile_index(gi, gj, g.R128) * TS;
        else return base + tile_index(gi >> 1, gj >> 1, g.R128) * TS + (long)(gj & 1) * 64 * TB + (gi & 1) * 64;
    };
    auto tptrT = [&](int ti_, int tj_) -> const T* {        // block (ti, tj) of the transposed-blocks copy (backward launch; 64-tiles)
        return g.LT + tile_index(ti_ >> 1, tj_ >> 1, g.R128) * TS + (long)(tj_ & 1) * 64 * TB + (ti_ & 1) * 64;
    };
    constexpr long LDA = TB;
    T* Ct = tptr(i, (inverse && j > i) ? i : j);           // tile (i,j)  (a forward launch's row block index is not a tile column)
    // per-slot scalars {sf2, sn2, mu, pivot tol, ..}: from the argument pack (BUILD) or from device memory
    const double* sp = BUILD ? tp.v + g.nslots * g.d + slot * SLOTP : g.slotp + (long)slot * SLOTP;
    // task (0,0) of the slot precedes every potrf of the slot.  WRITE-THROUGH: no publish of this kernel flushes plain stores any
    // more (round 4), and the corner task reads the word from another XCD (found by scripts/gpu_api_fuzz.py: garbage info words)
    if (BUILD && i == 0 && j == 0 && tid == 0) __hip_atomic_store(g.info + slot, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

    acc_t acc[FJ][FI];
    // D-layout address of this lane's accumulators inside a TBX x TBX tile with leading dimension ldc
    auto c_ptr = [&](T* base, long ldc) { return base + (long)(wj * WT) * ldc + wi * WT + l15; };
    auto load_c = [&](acc_t (&A)[FJ][FI], const T* base, long ldc) {
        const T* cp = c_ptr(const_cast<T*>(base), ldc);
#pragma unroll
        for (int x = 0; x < FJ; ++x)
#pragma unroll
            for (int y = 0; y < FI; ++y)
#pragma unroll
                for (int r = 0; r < 4; ++r) A[x][y][r] = cp[(long)(x * 16 + Num<T>::drow(l4, r)) * ldc + y * 16];
    };
    // Tile stores are write-through at agent scope (sc1): the release fence of publish() writes back every
    // dirty line of the XCD's L2 -- with plain stores that is the tiles of every workgroup on the XCD, again
    // and again (5 us per publish under load); with write-through stores there is nothing left to flush.
    // K(theta) tile (i,j) straight into the accumulators: element for element the arithmetic of kbuild_kernel
    // (inputs scaled as (T)((double)x * 1/l), squared distance accumulated over the dimensions in order,
    // nugget on the diagonal, identity padding, rhs rows = {r^T, 0, ..})
    auto build_tile = [&](acc_t (&A)[FJ][FI]) {
        const int d = g.d;
        const double* ie = tp.v + slot * d;
        const T sf2 = (T)sp[0], sn2 = (T)sp[1], mu = (T)sp[2];
        const long gi0 = (long)i * TBX + wi * WT + l15, gj0 = (long)j * TBX + wj * WT;
        if (i == g.nd) {
#pragma unroll
            for (int x = 0; x < FJ; ++x)
#pragma unroll
                for (int y = 0; y < FI; ++y)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const long gj = gj0 + x * 16 + Num<T>::drow(l4, r);
                        const bool first = (wi * WT + y * 16 + l15) == 0;
                        A[x][y][r] = (first && j < g.nd && gj < g.n) ? g.yv[gj] - mu : (T)0;
                    }
            return;
        }
        T r2[FJ][FI][4];
#pragma unroll
        for (int x = 0; x < FJ; ++x)
#pragma unroll
            for (int y = 0; y < FI; ++y)
#pragma unroll
                for (int r = 0; r < 4; ++r) r2[x][y][r] = (T)0;
        for (int dd = 0; dd < d; ++dd) {
            const double sc = ie[dd];
            const T* xr = g.xt + (long)dd * g.npad;
            T xi[FI], xj[FJ][4];
#pragma unroll
            for (int y = 0; y < FI; ++y) xi[y] = (T)__dmul_rn((double)xr[gi0 + y * 16], sc);   // rounded product, as k_scale stores it
#pragma unroll
            for (int x = 0; x < FJ; ++x)
#pragma unroll
                for (int r = 0; r < 4; ++r) xj[x][r] = (T)__dmul_rn((double)xr[gj0 + x * 16 + Num<T>::drow(l4, r)], sc);
#pragma unroll
            for (int x = 0; x < FJ; ++x)
#pragma unroll
                for (int y = 0; y < FI; ++y)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const T dl = xi[y] - xj[x][r];
                        r2[x][y][r] = __builtin_fma(dl, dl, r2[x][y][r]);
                    }
        }
#pragma unroll
        for (int x = 0; x < FJ; ++x)
#pragma unroll
            for (int y = 0; y < FI; ++y)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long gi = gi0 + y * 16, gj = gj0 + x * 16 + Num<T>::drow(l4, r);
                    T v = (g.kt == 0) ? kfun<0, T>(r2[x][y][r], sf2) : kfun<1, T>(r2[x][y][r], sf2);
                    if (gi == gj) v += sn2;
                    if (gj >= g.n || gi >= g.n) v = (gi == gj) ? (T)1 : (T)0;
                    A[x][y][r] = v;
                }
    };
    // (Round 4, measured and removed: 16-byte write-through stores -- lane pairs swapping one value each by DPP so that every
    //  store is a dwordx4 sc1 through inline asm -- are bit-identical and change nothing: N=4096 1.352 vs 1.339 ms, N=8192 4.32 vs
    //  4.30.  The tile stores are not what a hop waits for.  Lesson kept: a VMEM store of more than 8 bytes issued from inline asm
    //  needs its own s_nop before the data registers are rewritten, the compiler's hazard recogniser cannot see it.)
    auto store_c = [&](acc_t (&A)[FJ][FI], T* base, long ldc) {
        T* cp0 = c_ptr(base, ldc);
#pragma unroll
        for (int x = 0; x < FJ; ++x)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                T* cp = cp0 + (long)(x * 16 + Num<T>::drow(l4, r)) * ldc;
#pragma unroll
                for (int y = 0; y < FI; ++y)
                    __hip_atomic_store(cp + y * 16, A[x][y][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
    };
    auto zero_c = [&](acc_t (&A)[FJ][FI]) {
#pragma unroll
        for (int x = 0; x < FJ; ++x)
#pragma unroll
            for (int y = 0; y < FI; ++y) A[x][y] = (acc_t){0, 0, 0, 0};
    };

    // acc (+/-)= I J^T over nk LDS stages; I(i,k) at Ig[i + k*ldi], J(j,k) at Jg[j + k*ldj].  Same
    // LDS-DMA double buffer as gemm_nt (see there).  No dependency waits in here: a poll loop nested in
    // this loop makes the register allocator spill accumulators around it.
    // mi >= 0: both operands walk the finished tile columns 0, 1, .. of tile rows mi / mj (one TBX-wide slab = SPB
    // stages per column; the columns are separate tiles of the packed workspace); otherwise Ig / Jg are contiguous in k.
    // multi_c = 2 (inverse / forward launch): I contiguous in k (a row block of U), J walks the tiles (mj, mi), (mj, mi + 1), ..;
    // multi_c = 3 (backward launch): J walks the transposed blocks (mi, mj), (mi + 1, mj), .. of DfArgs::LT
    auto run_k_impl = [&](auto multi_c, acc_t (&A)[FJ][FI], const T* Ig0, long ldi, const T* Jg0, long ldj, int nk, bool negate,
                          int mi, int mj) {
        constexpr int MULTI = (int)decltype(multi_c)::value;
        auto stage = [&](int kb, int st) {
            T* Is = smem + st * STAGE;
            T* Js = Is + JOFF;
            const T *Ig, *Jg;                               // column 0 of stage kb
            if constexpr (MULTI == 1) {
                const int bcol = kb / SPB;
                const long o = (long)(kb % SPB) * GK * LDA;
                Ig = tptr(mi, bcol) + o;
                Jg = tptr(mj, bcol) + o;
            } else if constexpr (MULTI == 2) {
                Ig = Ig0 + (long)kb * GK * ldi;
                Jg = tptr(mj, mi + kb / SPB) + (long)(kb % SPB) * GK * LDA;
            } else if constexpr (MULTI == 3) {               // backward launch: J walks the transposed blocks (mi, mj), (mi + 1, mj), ..
                Ig = Ig0 + (long)kb * GK * ldi;
                Jg = tptrT(mi + kb / SPB, mj) + (long)(kb % SPB) * GK * LDA;
            } else {
                Ig = Ig0 + (long)kb * GK * ldi;
                Jg = Jg0 + (long)kb * GK * ldj;
            }
            if constexpr (TBX == 128) {
#pragma unroll
                for (int s2 = 0; s2 < 4; ++s2) {
                    const int qq = uw + 4 * s2;
                    if (F64) {
                        const long kcol = qq;
                        __builtin_amdgcn_global_load_lds((glb_void*)(Ig + kcol * ldi + 2 * lane),
                                                         (lds_void*)(Is + qq * LDT), 16, 0, GP_DF_DMA_AUX);
                        __builtin_amdgcn_global_load_lds((glb_void*)(Jg + kcol * ldj + 2 * lane),
                                                         (lds_void*)(Js + qq * LDT), 16, 0, GP_DF_DMA_AUX);
                    } else {
                        const long kcol = 4 * (qq >> 1) + (qq & 1) + 2 * (lane >> 5);
                        const int row = 4 * (lane & 31);
                        __builtin_amdgcn_global_load_lds((glb_void*)(Ig + kcol * ldi + row),
                                                         (lds_void*)(Is + qq * LDP), 16, 0, GP_DF_DMA_AUX);
                        __builtin_amdgcn_global_load_lds((glb_void*)(Jg + kcol * ldj + row),
                                                         (lds_void*)(Js + qq * LDP), 16, 0, GP_DF_DMA_AUX);
                    }
                }
            } else {
#pragma unroll
                for (int s2 = 0; s2 < GK / 8; ++s2) {
                    const int qq = uw + 4 * s2;           // GK / 2 instructions per operand tile
                    const long kcol = 4 * (qq >> 1) + (qq & 1) + 2 * (lane >> 5);
                    const int row = 2 * (lane & 31);
                    __builtin_amdgcn_global_load_lds((glb_void*)(Ig + kcol * ldi + row),
                                                     (lds_void*)(Is + qq * LD64), 16, 0, GP_DF_DMA_AUX);
                    __builtin_amdgcn_global_load_lds((glb_void*)(Jg + kcol * ldj + row),
                                                     (lds_void*)(Js + qq * LD64), 16, 0, GP_DF_DMA_AUX);
                }
            }
        };
        auto load_frags = [&](int buf, int kk, T* fi, T* fj) {
            const T* Is = smem + buf * STAGE + wi * WT + l15;
            const T* Js = smem + buf * STAGE + JOFF + wj * WT + l15;
            const int k = 4 * kk + l4;
#pragma unroll
            for (int f = 0; f < FI; ++f) fi[f] = Is[df_lds_off<T, TBX>(k, f * 16)];
#pragma unroll
            for (int f = 0; f < FJ; ++f) fj[f] = Js[df_lds_off<T, TBX>(k, f * 16)];
        };
        auto mfma_block = [&](const T* fi, const T* fj) {
            T nj[FJ];
#pragma unroll
            for (int f = 0; f < FJ; ++f) nj[f] = negate ? -fj[f] : fj[f];
#pragma unroll
            for (int x = 0; x < FJ; ++x)
#pragma unroll
                for (int y = 0; y < FI; ++y) A[x][y] = Num<T>::mfma(nj[x], fi[y], A[x][y]);
        };
        constexpr int NKK = GK / 4;
        auto compute = [&](int buf) {
#pragma unroll
            for (int kk = 0; kk < NKK; ++kk) {
                T fi[FI], fj[FJ];
                load_frags(buf, kk, fi, fj);
                mfma_block(fi, fj);
            }
        };
        if constexpr (NST == 4) {
            // deep pipeline: 3 stages of DMA in flight, counted vmcnt waits, one raw barrier per stage
            constexpr int AHEAD = NST - 1;
            static_assert(TBX == 128, "8 DMA instructions per wave and stage");
            for (int st = 0; st < AHEAD && st < nk; ++st) stage(st, st);
            for (int kb = 0; kb < nk; ++kb) {
                const int rem = nk - 1 - kb;               // stages issued beyond kb (capped at AHEAD - 1)
                if (rem >= 2) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
                else if (rem == 1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();              // stage kb landed for every wave; buffer (kb-1)%4 is free
                if (kb + AHEAD < nk) stage(kb + AHEAD, (kb + AHEAD) % NST);
                compute(kb % NST);       // (two fragment register sets were measured here too: no change)
            }
            __syncthreads();                               // LDS is free again
        } else {
            // one fragment register set (the two-set pipeline of gemm_nt does not fit next to the flag /
            // potrf state of this kernel without spilling, and buys ~0 there)
            stage(0, 0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            for (int kb = 0; kb < nk; ++kb) {
                const int cur = kb & 1;
                // once per slab: does a chain task want this CU to itself?  (the load flies under the slab's first stage)
                const bool chk = TBX == 64 && parkp != nullptr && !critical && (kb % SPB) == 0;
                int pk = 0;
                if (chk && tid == 0) pk = __hip_atomic_load(parkp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (kb + 1 < nk) stage(kb + 1, cur ^ 1);
                compute(cur);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (chk && tid == 0) s_park = pk;
                __syncthreads();
                if (chk && __builtin_expect(s_park != 0, 0)) {
                    for (int it = 0; it < 2048; ++it) {             // bounded (~ms): a missed wake-up costs time, never a hang
                        __builtin_amdgcn_s_sleep(48);
                        __syncthreads();
                        if (tid == 0) s_park = __hip_atomic_load(parkp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __syncthreads();
                        if (s_park == 0) break;
                    }
                    __syncthreads();
                }
            }
        }
    };
    auto run_k = [&](acc_t (&A)[FJ][FI], const T* Ig0, long ldi, const T* Jg0, long ldj, int nk, bool negate) {
        run_k_impl(std::integral_constant<int, 0>{}, A, Ig0, ldi, Jg0, ldj, nk, negate, 0, 0);
    };
    // Publishing a tile whose ONLY payload is store_c's write-through (sc1) stores needs no L2 write-back at all: the stores
    // are at the device-coherent level once this wave's vmcnt has drained, the barrier collects all waves, then the flag goes
    // out (MI355X_MICROARCH.md, "sc1 payload -> vmcnt(0) -> sc1 flag").  Saves the buffer_wbl2 / buffer_inv pair that every
    // thread of the workgroup issued per publish (microseconds under load, twice per column on the chain).  GP_DF_LIGHT_PUBLISH=0
    // restores the full fence everywhere.  The diagonal task's publish keeps it: potrf's L, W, log-det and info stores are plain.
#ifndef GP_DF_LIGHT_PUBLISH
#define GP_DF_LIGHT_PUBLISH 1
#endif
    // (GP_DF_WT_POTRF: potrf's L, W, log-det and info stores write-through too, so that its publishes need no fence either)
#ifndef GP_DF_WT_POTRF
#define GP_DF_WT_POTRF 1
#endif
    auto publish_wt = [&](int fi_, int fj_) {
        if (GP_DF_LIGHT_PUBLISH) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else __threadfence();
        __syncthreads();
        if (tid == 0) __hip_atomic_store(F + fi_ * R + fj_, g.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    auto publish = [&](int fi_, int fj_) {                  // everything this workgroup stored is visible first
        __threadfence();
        __syncthreads();
        // relaxed: every thread's own agent-scope fence above has already pushed its stores out, and the barrier
        // orders them before this store -- a second release here would only repeat the L2 write-back
        if (tid == 0) __hip_atomic_store(F + fi_ * R + fj_, g.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };

    // "one more tile of 64-column jc is final" (call with this workgroup's stores of that tile drained and a barrier behind them)
    auto col_done = [&](int jc) {
        if (TBX == 64 && g.colsig && tid == 0 && jc >= g.nprev && jc < g.ncols)
            __hip_atomic_fetch_add(g.colsig + ((jc - g.nprev) >> 1), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    constexpr bool XXF = TBX == 64 && OCC <= 2;           // builds whose LDS holds the stage area AND a second 36 KiB region (DF_XXF_LDS)
    if (inverse) {
        // ---- a tile of U = L^-T.  Row block rb of U advances one column block per task: the k-th slab needs U(rb,k), i.e. the
        // task before this one in the row -- a chain of nd - rb hops per row, nd rows side by side.
        // Forward launch (u_rows > 0): the same recurrence on a dense block of right-hand-side rows, from column 0, starting
        // from the tile's own content instead of the identity.
        // Backward launch (u_back): the recurrence read from the other end -- slabs k = nd-1 .. cb+1, blocks of the transposed copy.
        const bool fwd = g.u_rows > 0, back = fwd && g.u_back != 0;
        const int cb = i, rb = j, kf = fwd ? 0 : rb, nsl = back ? g.nd - 1 - cb : cb - kf;      // slabs k = kf .. cb - 1 (back: nd-1 .. cb+1)
        auto kblk = [&](int b) { return back ? g.nd - 1 - b : kf + b; };                        // block column of slab b, in the order they finish
        T* Ut = g.U + (long)slot * g.u_bstride + (long)cb * TBX * g.ldu + (long)rb * TBX;
        const T* Urow = g.U + (long)slot * g.u_bstride + (long)rb * TBX;      // U(rb rows, column c) at Urow[r + c * ldu]
        // two-per-CU builds (76 KiB of LDS): W_cb is prefetched behind the stage area now -- the factor is final -- and the
        // tile's solve at the end takes both operands from LDS (the accumulators written out as the I image) instead of
        // storing the pre-solve tile, draining the store and loading it back: ~2 of the ~8 us of a hop on the row's chain
        const T* Wcb = g.W + (long)slot * g.w_bstride + (long)cb * TBX * TBX;
        constexpr int IMG16 = (TBX / 2) * LD64 / 4;        // doubles per 16 k-columns of one operand image (= X64_IMG for 64-tiles)
        if constexpr (XXF) {
#pragma unroll
            for (int kb = 0; kb < SPB; ++kb)
#pragma unroll
                for (int s2 = 0; s2 < GK / 8; ++s2) {
                    const int qq = uw + 4 * s2;
                    const long kcol = (long)kb * GK + 4 * (qq >> 1) + (qq & 1) + 2 * (lane >> 5);
                    __builtin_amdgcn_global_load_lds((glb_void*)(Wcb + kcol * TBX + 2 * (lane & 31)),
                                                     (lds_void*)(smem + SPB * IMG16 + kb * IMG16 + qq * LD64), 16, 0, GP_DF_DMA_AUX);
                }
        }
        if (fwd) load_c(acc, Ut, g.ldu);
        else zero_c(acc);
        if (!fwd && nsl == 0) {
#pragma unroll
            for (int x = 0; x < FJ; ++x)
#pragma unroll
                for (int y = 0; y < FI; ++y)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (wi * WT + y * 16 + l15 == wj * WT + x * 16 + Num<T>::drow(l4, r)) acc[x][y][r] = (T)1;
        }
        int known = 0;
        if (nsl > 1) {                                      // the leading run of finished columns: one parallel peek
            if (wave == 0) {
                int run = 0;
                for (int c0 = 0; c0 < nsl; c0 += 64) {
                    const int c = c0 + lane;
                    const bool ready = c < nsl &&
                        __hip_atomic_load(F + rb * R + kblk(c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == g.epoch;
                    const unsigned long long miss = ~__ballot(ready);
                    const int lead = miss ? __builtin_ctzll(miss) : 64;
                    run += lead;
                    if (lead < 64) break;
                }
                if (lane == 0) s_known = run < nsl ? run : nsl;
            }
            __syncthreads();
            known = __builtin_amdgcn_readfirstlane(s_known);
            if (known > 0 && GP_DF_ACQUIRE) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
        int b0 = 0;
        if constexpr (TBX == 64) {
            if (known > 0) {
                if (back)               // the finished run = the LAST `known` block columns: one ascending pass over [nd - known, nd)
                    run_k_impl(std::integral_constant<int, 3>{}, acc, Urow + (long)(g.nd - known) * TBX * g.ldu, g.ldu, nullptr, LDA, known * SPB,
                               true, g.nd - known, cb);
                else
                    run_k_impl(std::integral_constant<int, 2>{}, acc, Urow + (long)kf * TBX * g.ldu, g.ldu, nullptr, LDA, known * SPB, true, kf, cb);
                b0 = known;
            }
        }
        for (int b = b0; b < nsl; ++b) {
            if (b >= known) {
                if (wave == 0) df_wait(F + rb * R + kblk(b), g.epoch, g.abort_flag);
                __syncthreads();
            }
            run_k(acc, Urow + (long)kblk(b) * TBX * g.ldu, g.ldu, back ? tptrT(kblk(b), cb) : tptr(cb, kblk(b)), LDA, SPB, true);
        }
        if constexpr (XXF) {
            static_assert(IMG16 == X64_IMG, "operand image of 16 k-columns");
            acc_t res[FJ][FI];
#pragma unroll
            for (int x = 0; x < FJ; ++x)
#pragma unroll
                for (int y = 0; y < FI; ++y)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int c = wj * WT + x * 16 + Num<T>::drow(l4, r), irow = wi * WT + y * 16 + l15;
                        smem[(c >> 4) * IMG16 + df_lds_off<T, TBX>(c & 15, irow)] = acc[x][y][r];
                    }
            zero_c(res);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (this wave's share of the W image: landed long ago)
            __syncthreads();
#pragma unroll
            for (int kb = 0; kb < SPB; ++kb)
#pragma unroll
                for (int kk = 0; kk < GK / 4; ++kk) {
                    const T* Is = smem + kb * IMG16 + wi * WT + l15;
                    const T* Js = smem + SPB * IMG16 + kb * IMG16 + wj * WT + l15;
                    const int k = 4 * kk + l4;
                    T fi[FI], fj[FJ];
#pragma unroll
                    for (int f = 0; f < FI; ++f) fi[f] = Is[df_lds_off<T, TBX>(k, f * 16)];
#pragma unroll
                    for (int f = 0; f < FJ; ++f) fj[f] = Js[df_lds_off<T, TBX>(k, f * 16)];
#pragma unroll
                    for (int x = 0; x < FJ; ++x)
#pragma unroll
                        for (int y = 0; y < FI; ++y) res[x][y] = Num<T>::mfma(fj[x], fi[y], res[x][y]);
                }
            store_c(res, Ut, g.ldu);
            publish_wt(rb, cb);
            return;
        }
        store_c(acc, Ut, g.ldu);                            // the pre-solve tile becomes an MFMA operand through memory
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        zero_c(acc);
        run_k(acc, Ut, g.ldu, Wcb, TBX, SPB, false);
        store_c(acc, Ut, g.ldu);
        publish_wt(rb, cb);
        return;
    }

    // accumulators -> tile-packed potrf image of the lower triangle (+ the copy of tile (0,0) and the identity tiles of the
    // 64-block path); the caller synchronises
    bool image_done = false;
    const T* ximg = nullptr;
    auto fill_image = [&](T* Ls) {
#pragma unroll
        for (int x = 0; x < FJ; ++x)
#pragma unroll
            for (int y = 0; y < FI; ++y) {
                const int bi = wi * FI + y, bj = wj * FJ + x;
                if (bi >= bj) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) Ls[ptile(bi, bj) + Num<T>::drow(l4, r) * 16 + l15] = acc[x][y][r];
                    if (TBX == 64 && bi == 0 && bj == 0) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) Ls[PT64_S + Num<T>::drow(l4, r) * 16 + l15] = acc[x][y][r];
                    }
                }
            }
        if constexpr (TBX == 64) potrf64_aux_init<T>(Ls);
    };

    // 64-tiles fuse the critical chain: the diagonal task (j,j) ALSO solves its own sub-diagonal tile (j,j-1)
    // (whose owner only accumulates it and hands the pre-solve tile over through memory) and applies that
    // last slab straight from LDS -- one flag hop per column on the chain instead of two.
    constexpr bool FUSE = TBX == 64;
    const bool diagx = FUSE && i == j && j > g.nprev && j < g.nd;   // solves (j,j-1) itself (not a finished panel's tile)
    const bool accp = FUSE && i == j + 1 && i < g.nd && (g.ncols <= 0 || i < g.ncols);   // tile (j+1,j): accumulate only (its solver, diagonal task j+1, must be part of this launch)
    const int jacc = diagx ? j - 1 : j;                          // slabs taken from memory

    // ---- accumulate the updates of all earlier columns
    if constexpr (BUILD) build_tile(acc);
    else if (j > 0 || i == j) load_c(acc, Ct, LDA);
    // A task that starts late finds most of its columns finished already.  Polling them one by one costs a
    // dependent ~1 us flag load (and an L2 invalidate) per slab -- more than a 64-wide slab's MFMA work --
    // so wave 0 peeks at all of them in parallel ONCE, and the leading run of finished columns is taken
    // without further polls (one acquire for the lot).
    int known = g.nprev;                                   // (a finished outer panel's columns need no flags)
    if (jacc > 1) {
        if (wave == 0) {
            int run = 0;
            for (int c0 = 0; c0 < jacc; c0 += 64) {
                const int c = c0 + lane;
                bool ready = false;
                if (c < g.nprev) ready = true;
                else if (c < jacc)
                    ready = __hip_atomic_load(F + i * R + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == g.epoch &&
                            __hip_atomic_load(F + j * R + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == g.epoch;
                const unsigned long long miss = ~__ballot(ready);
                const int lead = miss ? __builtin_ctzll(miss) : 64;
                run += lead;
                if (lead < 64) break;
            }
            if (lane == 0) s_known = run < jacc ? run : jacc;
        }
        __syncthreads();
        known = __builtin_amdgcn_readfirstlane(s_known);
        if (known > 0 && GP_DF_ACQUIRE) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    int b0 = 0;
    if constexpr (TBX == 64) {
        // 64-tiles: the finished run is ONE pipelined pass (a K = 64 slab is only 4 stages, its pipeline fill
        // would cost as much as its MFMAs).  Not for 128-tiles: with 128 accumulator registers a variable
        // trip count makes the allocator spill inside the stage loop.
        if (known > 0) {
            run_k_impl(std::integral_constant<int, 1>{}, acc, nullptr, LDA, nullptr, LDA, known * SPB, true, i, j);
            b0 = known;
        }
    }
    for (int b = b0; b < jacc; ++b) {                      // one TBX-wide slab per finished column b
        if (b >= known) {                                  // ONE wave polls (hundreds of waiting workgroups hammer
            if (wave == 0) {                               // the same few flag lines: 4x fewer pollers), the rest
                df_wait(F + i * R + b, g.epoch, g.abort_flag);             // wait at the barrier
                if (i != j) df_wait(F + j * R + b, g.epoch, g.abort_flag);
            }
            __syncthreads();
        }
        if (b == j - 1) stamp(6);
        run_k(acc, tptr(i, b), LDA, tptr(j, b), LDA, SPB, true);
    }
    stamp(1);

    if constexpr (FUSE) {
        if (accp) {                                         // hand the pre-solve tile (j+1,j) to the diagonal task
            if (BUILD || j > 0) store_c(acc, Ct, LDA);
            publish_wt(j, i);                               // "pre" flag lives in the unused upper slot (j, j+1)
            stamp(4);
            return;
        }
        if (diagx) {
            const int jm = j - 1;
            T* Xt = tptr(j, jm);                                           // tile (j, j-1)
            constexpr int XIMG = 8 * LD64;
            static_assert(XIMG == X64_IMG && LD64 == X64_LD, "xx_block_rmw reads the X images of this kernel");
            if (XXF && g.D && GP_DF_WT_POTRF) {
                // (1) the diagonal tile as accumulated so far goes to the potrf image NOW (it sits behind the stage area in
                // this build), which frees its 64 accumulator registers for the substitution
                fill_image(reinterpret_cast<T*>(smem_raw + DF_XXF_POTRF_AT + 2));
                image_done = true;
            }
            if (g.D && GP_DF_WT_POTRF) {
                // X = pre L^-T by BLOCKED SUBSTITUTION with L_{j-1,j-1} and its four 16x16 diagonal inverses -- available under
                // the chain flag (j-1, j+1), several microseconds before W_{j-1} (potrf128_core).  Wave w owns rows 16 w .. of the
                // tile and holds the TRANSPOSED 16x16 blocks X^T(b) in the MFMA D layout (register r of lane (l15, l4) = row
                // 16 w + l15, column 16 b + drow(l4, r)), so that
                //     X^T(k) = W_kk S_k ;   S_b -= L(b,k) X^T(k)  (b > k)        [S_b starts as pre^T(b)]
                // are LEFT multiplications whose right-hand operand is the previous result's registers as they are (kidx):
                // 40 dependent-free-of-memory MFMAs per wave instead of a 64-MFMA product after the 36-MFMA block inverse.
                const T* Lg = tptr(jm, jm);
                const T* Dg = g.D + (long)slot * g.d_bstride + (long)jm * 1024;
                if (wave == 0) df_wait(F + jm * R + j, g.epoch, g.abort_flag);           // pre-solve tile stored by its owner
                __syncthreads();
                acc_t sb[4], xb[4];
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        sb[b][r] = __hip_atomic_load(Xt + (long)(16 * b + Num<T>::drow(l4, r)) * LDA + 16 * uw + l15, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT);
                if (wave == 0) df_wait(F + jm * R + j + 1, g.epoch, g.abort_flag);       // chain flag of column j-1: L, diagonal inverses
                __syncthreads();
                enter_critical();                          // from here to ready(j,j) nothing but this workgroup's own work
                stamp(5);
                T* Limg = smem;                            // the 64 x 64 tile as ONE 64-column stage image; behind it the inverses
                T* Dimg = smem + 32 * LD64;
#pragma unroll
                for (int s2 = 0; s2 < 8; ++s2) {
                    const int qq = uw + 4 * s2;
                    const long kcol = 4 * (qq >> 1) + (qq & 1) + 2 * (lane >> 5);
                    __builtin_amdgcn_global_load_lds((glb_void*)(Lg + kcol * LDA + 2 * (lane & 31)), (lds_void*)(Limg + qq * LD64), 16, 0,
                                                     GP_DF_DMA_AUX);
                }
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    const int q2 = uw + 4 * s2;
                    __builtin_amdgcn_global_load_lds((glb_void*)(Dg + q2 * 128 + 2 * lane), (lds_void*)(Dimg + q2 * 128), 16, 0, GP_DF_DMA_AUX);
                }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    xb[k] = (acc_t){0, 0, 0, 0};
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk)
                        xb[k] = Num<T>::mfma(Dimg[k * 256 + Num<T>::kidx(kk, l4) * 16 + l15], sb[k][kk], xb[k]);
#pragma unroll
                    for (int b = k + 1; b < 4; ++b)
#pragma unroll
                        for (int kk = 0; kk < 4; ++kk)
                            sb[b] = Num<T>::mfma(-Limg[df_lds_off<T, TBX>(16 * k + Num<T>::kidx(kk, l4), 16 * b + l15)], xb[k][kk], sb[b]);
                }
                __syncthreads();                           // every wave is done with the L image: the X images take its place
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int c = 16 * b + Num<T>::drow(l4, r), irow = 16 * uw + l15;
                        __hip_atomic_store(Xt + (long)c * LDA + irow, (T)xb[b][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        smem[(c >> 4) * XIMG + df_lds_off<T, TBX>(c & 15, irow)] = (T)xb[b][r];
                    }
            } else {
                if (wave == 0) {
                    df_wait(F + jm * R + j, g.epoch, g.abort_flag);           // pre-solve tile stored by its owner
                    df_wait(F + jm * R + jm, g.epoch, g.abort_flag);          // W_{j-1}
                }
                __syncthreads();
                enter_critical();                              // from here to ready(j,j) nothing but this workgroup's own work
                stamp(5);
                acc_t accx[FJ][FI];
                zero_c(accx);
                run_k(accx, Xt, LDA, g.W + (long)slot * g.w_bstride + (long)jm * TBX * TBX, TBX, SPB, false);
                store_c(accx, Xt, LDA);                        // X(j,j-1): the column below waits for it
                // X -> four 16-column LDS images [k][row] (both MFMA operands of X X^T read the same image)
#pragma unroll
                for (int x = 0; x < FJ; ++x)
#pragma unroll
                    for (int y = 0; y < FI; ++y)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int c = wj * WT + x * 16 + Num<T>::drow(l4, r), irow = wi * WT + y * 16 + l15;
                            smem[(c >> 4) * XIMG + df_lds_off<T, TBX>(c & 15, irow)] = accx[x][y][r];
                        }
            }
            // ready(j,j-1) waits until the product below is done: draining the write-through stores of X here (vmcnt(0)) would sit
            // on the chain, and the tasks that read X(j,j-1) are not on it.  Only the LDS images must be complete now (a raw
            // barrier: __syncthreads() would drain the stores as well).
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            stamp(7);
            if (image_done) {
                // (2) only block column 0 of the image before the factorisation starts: one 16x16 block per wave (16 MFMAs
                // instead of 64); the other six lower blocks are applied by waves 2 and 3 under the elimination of panel 0
                T* Lsx = reinterpret_cast<T*>(smem_raw + DF_XXF_POTRF_AT + 2);
                xx_block_rmw<T>(Lsx, smem, uw, 0, l15, l4, uw == 0 ? Lsx + PT64_S : nullptr);
                ximg = smem;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // X(j,j-1) is at the coherent level (sc1 stores) ..
                __syncthreads();                                // .. for every wave; block column 0 of the image is complete
                if (tid == 0) __hip_atomic_store(F + j * R + jm, g.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                col_done(jm);                                   // tile (j, j-1) is final
                stamp(6);
            } else {
#pragma unroll
                for (int st = 0; st < TBX / 16; ++st)
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) {
                        const T* Im = smem + st * XIMG + l15;
                        const int kq = 4 * kk + l4;
                        T fi[FI], fj[FJ];
#pragma unroll
                        for (int f = 0; f < FI; ++f) fi[f] = Im[df_lds_off<T, TBX>(kq, wi * WT + f * 16)];
#pragma unroll
                        for (int f = 0; f < FJ; ++f) fj[f] = -Im[df_lds_off<T, TBX>(kq, wj * WT + f * 16)];
#pragma unroll
                        for (int x = 0; x < FJ; ++x)
#pragma unroll
                            for (int y = 0; y < FI; ++y) acc[x][y] = Num<T>::mfma(fj[x], fi[y], acc[x][y]);
                    }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // X(j,j-1) is at the coherent level (sc1 stores) ..
                __syncthreads();                                // .. for every wave; and the images make way for the potrf image
                if (tid == 0) __hip_atomic_store(F + j * R + jm, g.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                col_done(jm);                                   // tile (j, j-1) is final
                stamp(6);
            }
        }
    }

    if (i == j) {
        if (j == g.nd) {                                    // corner of the border: -|z|^2 accumulates here
            store_c(acc, Ct, LDA);
            if constexpr (BUILD) {
                // this task depends (transitively) on every other task of the slot: everything is final
                if (wave == 0) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");        // (plain loads of other workgroups' partials below)
                    double sum = 0.0;
                    for (int b2 = lane; b2 < g.nd; b2 += 64) sum += g.partial[(long)slot * g.p_bstride + b2];
                    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
                    if (lane == 0) {
                        g.hres[2 * slot + 0] = 2.0 * sum;
                        g.hres[2 * slot + 1] = -(double)acc[0][0][0];          // lane 0 of wave 0 holds entry [0][0]
                        g.hinfo[slot] = __hip_atomic_load(g.info + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (__hip_atomic_load(g.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)
                            g.hinfo[g.nslots] = 1;
                    }
                }
            }
            return;
        }
        enter_critical();                                   // (column 0 has no sub-diagonal solve before it)
        // accumulators -> tile-packed LDS image of the lower triangle, then factor + invert in place
        // (XXF builds keep the image behind the stage area ALWAYS: a compile-time LDS address at the one call site lets the
        //  out-of-line potrf body address it as LDS; a run-time choice of pointer turned every access in there into a flat one)
        double* praw = XXF ? smem_raw + DF_XXF_POTRF_AT : smem_raw;
        if (!image_done) {
            fill_image(reinterpret_cast<T*>(praw + 2));
            __syncthreads();
        }
        stamp(2);
        // 64-tiles: the core publishes ready(j,j) itself, as soon as W_j is out and before the L tile
        int* pubf = (TBX == 64 && GP_DF_WT_POTRF) ? F + j * R + j : nullptr;
        T* Dj = (pubf && g.D) ? g.D + (long)slot * g.d_bstride + (long)j * 1024 : nullptr;
        int* chainf = (Dj && j + 2 <= g.nd) ? F + j * R + j + 2 : nullptr;        // (the last column has no successor on the chain)
        potrf128_core_call<T, TBX / 16, GP_DF_WT_POTRF != 0, XXF ? DF_XXF_POTRF_AT : 0, XXF>(
            Ct, LDA, Wj, g.partial + (long)slot * g.p_bstride + j, g.info + slot, (T)sp[3], pubf, g.epoch, chainf, Dj, ximg != nullptr);
        stamp(3);
        if (pubf) { }
        else if (GP_DF_WT_POTRF) publish_wt(j, j);
        else publish(j, j);
        leave_critical();
        if (TBX == 64 && g.colsig) {                        // the L tile went out AFTER ready(j,j): drain it before the column count
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            col_done(j);
        }
        stamp(4);
        return;
    }

    // ---- panel solve X(i,j) = acc W_j^T: the pre-solve tile goes through memory to become an MFMA operand
    if (BUILD || j > 0) {
        store_c(acc, Ct, LDA);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    zero_c(acc);
    stamp(2);
    if (wave == 0) df_wait(F + j * R + j, g.epoch, g.abort_flag);
    __syncthreads();
    stamp(5);
    run_k(acc, Ct, LDA, Wj, TBX, SPB, false);
    stamp(3);
    store_c(acc, Ct, LDA);
    publish_wt(i, j);
    col_done(j);
    stamp(4);
}

// log det = 2 sum partial ; quad = -E(0,0) ; res[slot] = {logdet, quad}.  When hres is given the results,
// the info words and the dataflow abort flag are ALSO written straight into pinned host memory
// (hres[2*slots], hinfo[slots + 1]): the caller only synchronises the stream, no device-to-host copies.
template <typename T>
__global__ void finalize_kernel(const T* __restrict__ Abase, long bstride, long corner,
                                const double* __restrict__ partial, int nt, double* __restrict__ res,
                                const int* __restrict__ info = nullptr, const int* __restrict__ abort_flag = nullptr,
                                double* __restrict__ hres = nullptr, int* __restrict__ hinfo = nullptr,
                                int pstride = 0, const double* __restrict__ partial2 = nullptr, int n2 = 0) {
    // partial: nt entries per slot at stride pstride (0 = nt); partial2 (optional): n2 more entries per slot,
    // stride n2 -- the 64-blocks of a dataflow tail that followed a multi-kernel bulk
    const int slot = blockIdx.x;
    double s = 0.0;
    for (int b = threadIdx.x; b < nt; b += 64) s += partial[(long)slot * (pstride ? pstride : nt) + b];
    for (int b = threadIdx.x; b < n2; b += 64) s += partial2[(long)slot * n2 + b];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    if (threadIdx.x == 0) {
        // corner = element offset of (Npad, Npad): the first element of the workspace's last tile (Nt, Nt)
        const double logdet = 2.0 * s, quad = -(double)Abase[(long)slot * bstride + corner];
        res[slot * 2 + 0] = logdet;
        res[slot * 2 + 1] = quad;
        if (hres) {
            hres[slot * 2 + 0] = logdet;
            hres[slot * 2 + 1] = quad;
            hinfo[slot] = info[slot];
            if (slot == 0) hinfo[(int)gridDim.x] = *abort_flag;
        }
    }
}

// Prediction epilogue (K9/K10 of SURVEY.md §2.1; BGP:407-417).  V: column-major [mpad x npad] (ld = mpad)
// per slot, V(t, j) = (L^-1 k*_t)_j;  z = L^-1 r sits in row npad of the slot's factor (stride ldz).
//     mean[t] = mu + sum_j V(t,j) z_j ;   var[t] = kappa - sum_j V(t,j)^2      (fp64 accumulation)
// HBM bound: V is streamed exactly once (mpad * npad elements).  Stage 1: one workgroup per
// 128 test points x strip of `js` columns -- the strip's z values are staged once in LDS, wave w takes
// columns w, w+4, .. of the strip, a lane loads 2 adjacent test points per column (fp64: one 16-byte
// dwordx4, a wave covers a full 1 KiB column segment), four columns in flight per wave; the four waves'
// partial sums meet in LDS in a fixed order.  Stage 2 adds the strips in order (deterministic: no atomics).
// grid = (mpad/128, nstrips, nslots); part: [slot][strip][2][mpad].
template <typename T>
__global__ __launch_bounds__(256) void predict_partial_kernel(const T* __restrict__ V, long ldv, long v_bstride, int ncols,
                                                              const T* __restrict__ zbase, int zR, long z_bstride,
                                                              int js, double* __restrict__ part, int nstrips) {
    extern __shared__ double pr_lds[];            // z strip [js] + reduction scratch [4][2][128]
    typedef typename Num<T>::pair_t pair_t;
    double* zs = pr_lds;
    double* red = pr_lds + js;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tb = blockIdx.x, strip = blockIdx.y, slot = blockIdx.z;
    const int j0 = strip * js;
    const int jn = (ncols - j0 < js) ? (ncols - j0) : js;       // columns of this strip (<= 0: nothing to add)
    V += (long)slot * v_bstride + (long)tb * TB + 2 * lane;
    // z_j = element (Npad, j) of the slot's factor: row 0 of tile (Nt, j / 128) of the packed workspace (zR = Nt + 1);
    // zR = 0: a plain vector (the factor is spread over several devices and z was gathered while its panels streamed by)
    zbase += (long)slot * z_bstride;
    for (int j = tid; j < jn; j += 256) {
        const int gj = j0 + j;
        zs[j] = zR > 0 ? (double)zbase[tile_index(zR - 1, gj >> 7, zR) * TS + (long)(gj & 127) * TB] : (double)zbase[gj];
    }
    __syncthreads();
    double d0 = 0.0, d1 = 0.0, n0 = 0.0, n1 = 0.0;
    int j = wave;
    for (; j + 12 < jn; j += 16) {                // four independent 16-byte loads in flight per lane
        pair_t v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const pair_t*>(V + (long)(j0 + j + 4 * u) * ldv);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double z = zs[j + 4 * u], a = (double)v[u].x, b = (double)v[u].y;
            d0 = __builtin_fma(a, z, d0); d1 = __builtin_fma(b, z, d1);
            n0 = __builtin_fma(a, a, n0); n1 = __builtin_fma(b, b, n1);
        }
    }
    for (; j < jn; j += 4) {
        const pair_t v = *reinterpret_cast<const pair_t*>(V + (long)(j0 + j) * ldv);
        const double z = zs[j], a = (double)v.x, b = (double)v.y;
        d0 = __builtin_fma(a, z, d0); d1 = __builtin_fma(b, z, d1);
        n0 = __builtin_fma(a, a, n0); n1 = __builtin_fma(b, b, n1);
    }
    red[(wave * 2 + 0) * TB + 2 * lane] = d0; red[(wave * 2 + 0) * TB + 2 * lane + 1] = d1;
    red[(wave * 2 + 1) * TB + 2 * lane] = n0; red[(wave * 2 + 1) * TB + 2 * lane + 1] = n1;
    __syncthreads();
    {
        const int which = tid >> 7, t = tid & 127;            // threads 0-127: dot, 128-255: norm
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < 4; ++w) s += red[(w * 2 + which) * TB + t];
        part[(((long)slot * nstrips + strip) * 2 + which) * ldv + (long)tb * TB + t] = s;
    }
}

// Stage 2: mean / var per test point from the strip partials, mu and kappa = sf^2 + sn^2 of the slot's theta.
// pw_mean / pw_nug (optional, [slot][out_bstride]): m(x*_t) and nugget(x*_t) evaluated by the host (BGP:113, 408).
__global__ void predict_finish_kernel(const double* __restrict__ part, int nstrips, long mpad, const double* __restrict__ slotp,
                                      int m, long out_bstride, double* __restrict__ mean, double* __restrict__ var,
                                      const double* __restrict__ pw_mean = nullptr, const double* __restrict__ pw_nug = nullptr,
                                      const double* __restrict__ pw_kxx = nullptr) {
    // pw_kxx (optional, [slot][out_bstride]): k(x*_t, x*_t) per test point (run-time compiled covariance functions need not be stationary)
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int slot = blockIdx.y;
    if (t >= m) return;
    const double* sp = slotp + (long)slot * SLOTP;
    double dot = 0.0, nrm = 0.0;
    for (int s = 0; s < nstrips; ++s) {
        dot += part[(((long)slot * nstrips + s) * 2 + 0) * mpad + t];
        nrm += part[(((long)slot * nstrips + s) * 2 + 1) * mpad + t];
    }
    const long o = (long)slot * out_bstride + t;
    mean[o] = (pw_mean ? pw_mean[o] : sp[2]) + dot;
    var[o] = (pw_kxx ? pw_kxx[o] : sp[SP_KXX]) + (pw_nug ? pw_nug[o] : sp[1]) - nrm;            // kappa = k(x*, x*) + nugget (BGP:110-115)
}

// ---------------------------------------------------------------------------------------------
// Hyper-parameter gradient (no reference counterpart):
//   d loglik / d theta_p = 1/2 sum_{g,j} (alpha_g alpha_j - Kinv_gj) dK_gj/dtheta_p
// identity_rows seeds a row block of V with rows of the identity (forward + backward substitution
// then leave rows of K^-1 there); grad_reduce streams that row block once, rebuilds dK/dtheta on
// the fly from the scaled inputs and accumulates   gacc[dd] += w fac u_dd^2  (length scales),
// gacc[d] += w k  (sigma_f),  gacc[d+1] += w_gg  (sigma_n)   with fp64 atomics.
// ---------------------------------------------------------------------------------------------
// row `row` (0..127) of tile row Nt of the packed workspace (z = L^-1 r sits in row 0) -> out[j * ldo], j < npad
template <typename T>
__global__ void gather_rhs_row_kernel(const T* __restrict__ Abase, int R, int row, int npad, T* __restrict__ out, long ldo,
                                      int j_first = 0, long a_bstride = 0, long out_bstride = 0) {
    const int j = j_first + blockIdx.x * blockDim.x + threadIdx.x;        // columns [j_first, npad)
    Abase += (long)blockIdx.z * a_bstride;                                // (slot = blockIdx.z: gphip_loglik_grad_batch)
    out += (long)blockIdx.z * out_bstride;
    if (j < npad) out[(long)j * ldo] = Abase[tile_index(R - 1, j >> 7, R) * TS + (long)(j & 127) * TB + row];
}

// alpha = U z for the explicit upper-triangular U = L^-T (column-major, leading dimension ld; zeros below the diagonal): the
// gradient's alpha = K^-1 r = L^-T (L^-1 r) once U exists, as one pass over U instead of a backward substitution of ~2 launches
// per tile column.  Fixed summation order: a partial sum per (row, chunk of `chunk` columns), then the chunks in order.
// Several slots at once (blockIdx.z, gphip_loglik_grad_batch): u_ / z_ / part_ / out_bstride are the elements between their U, z, partial sums and results.
template <typename T>
__global__ __launch_bounds__(128) void utri_gemv_partial_kernel(const T* __restrict__ U, long ld, const T* __restrict__ z, int npad,
                                                                int chunk, double* __restrict__ part, long u_bstride = 0,
                                                                long z_bstride = 0, long part_bstride = 0) {
    U += (long)blockIdx.z * u_bstride;
    z += (long)blockIdx.z * z_bstride;
    part += (long)blockIdx.z * part_bstride;
    const int r = blockIdx.x * TB + threadIdx.x;                                // one tile row of U per workgroup (128 threads)
    const int c1 = min((int)(blockIdx.y + 1) * chunk, npad);
    const int c0 = max((int)blockIdx.y * chunk, (int)(blockIdx.x * TB));        // (row r has nothing left of column r)
    // four accumulators, eight loads in flight: one dependent load-then-fma per column ran at the load LATENCY (N = 2048:
    // 128 us for a 17 MB read, a tenth of a gradient call); the order of the additions stays fixed
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int c = c0;
#pragma unroll 2
    for (; c + 4 <= c1; c += 4) {
        const T u0 = U[(long)c * ld + r], u1 = U[(long)(c + 1) * ld + r], u2 = U[(long)(c + 2) * ld + r], u3 = U[(long)(c + 3) * ld + r];
        s0 = __builtin_fma((double)u0, (double)z[c], s0);
        s1 = __builtin_fma((double)u1, (double)z[c + 1], s1);
        s2 = __builtin_fma((double)u2, (double)z[c + 2], s2);
        s3 = __builtin_fma((double)u3, (double)z[c + 3], s3);
    }
    for (; c < c1; ++c) s0 = __builtin_fma((double)U[(long)c * ld + r], (double)z[c], s0);
    part[(long)blockIdx.y * npad + r] = (s0 + s1) + (s2 + s3);
}
template <typename T>
__global__ void utri_gemv_finish_kernel(const double* __restrict__ part, int nchunks, int npad, T* __restrict__ out,
                                        long part_bstride = 0, long out_bstride = 0) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= npad) return;
    part += (long)blockIdx.z * part_bstride;
    out += (long)blockIdx.z * out_bstride;
    double s = 0.0;
    for (int y = 0; y < nchunks; ++y) s += part[(long)y * npad + r];
    out[r] = (T)s;
}

// out = in with every 64 x 64 block transposed IN PLACE POSITION (block (a, b) of a tile stays block (a, b), its content turns):
// the copy of the factor (grid.x = lower tiles of the packed workspace, 4 blocks each) or of the 64-block inverses
// (tile_elems = 64 * 64, ld = 64, one block per workgroup) that the backward launch of chol_dataflow_kernel reads.
template <typename T>
__global__ __launch_bounds__(256) void transpose_blocks64_kernel(const T* __restrict__ in, T* __restrict__ out, long tile_elems, int ld, int nblk) {
    __shared__ T t[64][65];
    const long base = (long)blockIdx.x * tile_elems;
    for (int q = 0; q < nblk; ++q) {
        const int a = q & 1, b = q >> 1;
        const long o = base + (long)b * 64 * ld + a * 64;
        for (int e = threadIdx.x; e < 4096; e += 256) t[e >> 6][e & 63] = in[o + (long)(e >> 6) * ld + (e & 63)];       // t[col][row]
        __syncthreads();
        for (int e = threadIdx.x; e < 4096; e += 256) out[o + (long)(e >> 6) * ld + (e & 63)] = t[e & 63][e >> 6];      // (row, col) <- (col, row)
        __syncthreads();
    }
}

template <typename T>
__global__ void identity_rows_kernel(T* __restrict__ V, long ldv, int npad, int c0, int mc, long v_bstride = 0) {
    const long total = ldv * (long)npad;
    V += (long)blockIdx.y * v_bstride;                                    // (slot = blockIdx.y: one slab per slot)
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int t = (int)(idx % ldv), j = (int)(idx / ldv);
        V[idx] = (t < mc && j == c0 + t) ? (T)1 : (T)0;
    }
}

// The diagonal tiles L_bb of the factor in the tile-major workspace (R tile rows), one per workgroup, as [Nt][128 x 128]
// column-major blocks with an explicit zero upper triangle -- the layout of the W_b; the workspace itself promises nothing
// above a diagonal tile's diagonal.  (The refined diagonal solves of queue_backward_rows multiply by them.)
template <typename T>
__global__ __launch_bounds__(256) void diag_tiles_lower_kernel(const T* __restrict__ ws, int R, T* __restrict__ out) {
    const int b = blockIdx.x;
    const T* in = ws + tile_index(b, b, R) * TS;
    T* o = out + (long)b * TS;
    for (int e = threadIdx.x; e < (int)TS; e += 256) o[e] = ((e & (TB - 1)) >= (e >> 7)) ? in[e] : (T)0;     // row >= column
}

// x += r, elementwise over n elements
template <typename T>
__global__ void add_rows_kernel(T* __restrict__ x, const T* __restrict__ r, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) x[i] += r[i];
}


// A group of gradient reductions, one per workspace slot (gphip_loglik_grad_batch): the arguments of slot 0 and the elements
// between the slots' K^-1 slabs, alpha vectors, scaled inputs (both terms), slot scalars, accumulators and per-workgroup rows.
// Square reductions only (beta / xr / diag unset).  The one-theta kernels below take GradArgs as they always did; the *_slots
// kernels run the same tile body on at(blockIdx.z).
struct GradStride {
    long kinv, alpha, xs, slotp, gacc, gpart;
};
template <typename T>
struct GradSlots {
    GradArgs<T> a;
    GradStride s;
    __host__ __device__ GradArgs<T> at(int slot) const {
        GradArgs<T> r = a;
        r.Kinv += slot * s.kinv; r.alpha += slot * s.alpha; r.xs += slot * s.xs; r.slotp += slot * s.slotp; r.gacc += slot * s.gacc;
        if (r.xs2) r.xs2 += slot * s.xs;
        if (r.gpart) r.gpart += slot * s.gpart;
        return r;
    }
};

// One 128 (rows of the block) x 128 (columns) tile per workgroup; thread = one row, 64 columns.
template <typename T, int D, int KT>
__device__ __forceinline__ void grad_reduce_tile(const GradArgs<T>& a) {
    extern __shared__ double lds_raw[];
    T* xjs = reinterpret_cast<T*>(lds_raw);      // [d][128] column points, then alpha_j [128]
    const int d = (D > 0) ? D : a.d;
    T* aj = xjs + d * TB;
    const int tid = threadIdx.x, row = tid & 127, half = tid >> 7;
    const int ti = blockIdx.x, tj = blockIdx.y;
    const GradEmit out(a, lds_raw, tid);
    if (a.tri && tj > ti) { out.skip(); return; }
    const double wt = (a.tri && tj < ti) ? 2.0 : 1.0;
    const int t = ti * TB + row, g = a.c0 + t;
    for (int idx = tid; idx < d * TB; idx += 256) xjs[idx] = a.xs[(long)(idx >> 7) * a.npad + tj * TB + (idx & 127)];
    if (tid < TB) aj[tid] = a.alpha[tj * TB + tid];
    constexpr int DM = (D > 0) ? D : 32;
    const bool rect = a.xr != nullptr;
    const T* xrow = grad_row_points(a);
    const int ldr = grad_row_ld(a);
    T xg[DM];
    double acc[DM];
#pragma unroll
    for (int dd = 0; dd < DM; ++dd) {
        acc[dd] = 0.0;
        xg[dd] = (dd < d && t < a.mc) ? xrow[(long)dd * ldr + g] : (T)0;
    }
    double acc_sf = 0.0, acc_dg = 0.0;
    const T ag = (t < a.mc && !rect) ? a.alpha[g] : (T)0;
    const double bg = (a.beta && t < a.mc) ? (double)a.beta[g] : 0.0;
    const T sf2 = (T)a.slotp[0];
    __syncthreads();
    if (t < a.mc && (rect || g < a.n)) {
        for (int jj = half * 64; jj < half * 64 + 64; ++jj) {
            const int j = tj * TB + jj;
            if (j >= a.n) break;
            T u2[DM];
            T r2 = (T)0;
#pragma unroll
            for (int dd = 0; dd < DM; ++dd) {
                if (dd < d) {
                    const T u = xg[dd] - xjs[dd * TB + jj];
                    u2[dd] = u * u;
                    r2 += u2[dd];
                }
            }
            T kpart, fac;
            if (KT == 0) {
                kpart = sf2 * exp_nonpos((T)-0.5 * r2);
                fac = kpart;
            } else {
                const T s5 = Num<T>::sqrt_((T)5.0 * r2);
                const T e = exp_nonpos(-s5);
                kpart = sf2 * ((T)1.0 + s5 + (T)(5.0 / 3.0) * r2) * e;
                fac = sf2 * (T)(5.0 / 3.0) * ((T)1.0 + s5) * e;
            }
            const double w = grad_weight(a, wt, ag, aj[jj], bg, j, (double)a.Kinv[(long)j * a.ldv + t]);
            const double wf = w * (double)fac;
#pragma unroll
            for (int dd = 0; dd < DM; ++dd)
                if (dd < d) acc[dd] = __builtin_fma(wf, (double)u2[dd], acc[dd]);
            acc_sf = __builtin_fma(w, (double)kpart, acc_sf);
            if (j == g && !rect) acc_dg += w;
        }
    }
    // out of the workgroup: wave sums -> LDS -> one row of per-workgroup sums (GradEmit)
#pragma unroll
    for (int dd = 0; dd < DM; ++dd)
        if (dd < d) out.put(acc[dd], dd);
    out.put(acc_sf, d);
    out.put(acc_dg, d + 1);
    out.finish();
}
template <typename T, int D, int KT>
__global__ __launch_bounds__(256) void grad_reduce_kernel(GradArgs<T> a) { grad_reduce_tile<T, D, KT>(a); }
template <typename T, int D, int KT>
__global__ __launch_bounds__(256) void grad_reduce_slots_kernel(GradSlots<T> b) { grad_reduce_tile<T, D, KT>(b.at((int)blockIdx.z)); }

// The same reduction for the general covariance form (KSpec): w = wt (alpha_g alpha_j - Kinv_gj) contracted with every
// dk/dtheta.  Accumulators (the host applies the chain-rule factors of its theta layout):
//   gacc[dd]           sum w (dk/dk1) sf1^2 (-2 dg1/dr2) u1_dd^2          -> d/dl_1dd = 1/2 gacc / l
//   gacc[d]            sum w (dk/dk1) k1                                  -> d/dsf1  = gacc / sf1
//   gacc[d + 1]        sum_g w_gg                                         -> d/dsn   = gacc sn
//   gacc[d + 2 + dd]   the same for term 2's length scales,  gacc[2 d + 2] for sf2
//   gacc[2 d + 3], gacc[2 d + 4]   sum w (dk/dk_t) sf_t^2 dg_t/dalpha_t   -> d/dalpha_t = 1/2 gacc
//   gacc[2 d + 5]      sum w                                              -> d/dc = 1/2 gacc
// One 128 x 128 tile per workgroup, thread = one row x 64 columns; row and column points of both terms sit in LDS.
template <typename T>
__device__ __forceinline__ void grad_reduce_general_tile(const GradArgs<T>& a) {
    extern __shared__ double lds_raw[];
    const int d = a.d;
    // Beyond KB_LDS_MAXD dimensions the point tiles do not fit in LDS and 32 accumulators per term are all the registers
    // hold: the points are then read from global memory (L1 / L2 resident: 2 x 128 points per workgroup) and the launch
    // covers the length-scale derivatives of the dimension window [d0, d0 + 32) only -- the host launches ceil(d / 32) times.
    const bool glb = d > KB_LDS_MAXD;
    const int d0 = glb ? a.d0 : 0;
    T* xjs = reinterpret_cast<T*>(lds_raw);      // [d][128] column points (term 1), then rows, then the same for term 2
    T* xis = xjs + (glb ? 0 : d * TB);
    T* xjs2 = xis + (glb ? 0 : d * TB);
    T* xis2 = xjs2 + (glb ? 0 : d * TB);
    T* aj = xis2 + (glb ? 0 : d * TB);
    const bool two = a.ks.op != 0;
    const int tid = threadIdx.x, row = tid & 127, half = tid >> 7;
    const int ti = blockIdx.x, tj = blockIdx.y;
    const GradEmit out(a, lds_raw, tid);
    if (a.tri && tj > ti) { out.skip(); return; }
    const double wt = (a.tri && tj < ti) ? 2.0 : 1.0;
    const int t = ti * TB + row, g = a.c0 + t;
    const int g0 = a.c0 + ti * TB;               // first row point of this tile
    const bool rect = a.xr != nullptr;
    const T* xrow = grad_row_points(a);
    const T* xrow2 = grad_row_points2(a);
    const int ldr = grad_row_ld(a);
    for (int idx = tid; idx < (glb ? 0 : d * TB); idx += 256) {
        const int dd = idx >> 7, c = idx & 127;
        xjs[idx] = a.xs[(long)dd * a.npad + tj * TB + c];
        xis[idx] = (g0 + c < ldr) ? xrow[(long)dd * ldr + g0 + c] : (T)0;
        if (two) {
            xjs2[idx] = a.xs2[(long)dd * a.npad + tj * TB + c];
            xis2[idx] = (g0 + c < ldr) ? xrow2[(long)dd * ldr + g0 + c] : (T)0;
        }
    }
    if (tid < TB) aj[tid] = a.alpha[tj * TB + tid];
    // coordinate dd of this thread's row point / of column point jj, term 1 and term 2
    auto xi1 = [&](int dd) -> T { return glb ? xrow[(long)dd * ldr + g] : xis[dd * TB + row]; };
    auto xj1 = [&](int dd, int jj) -> T { return glb ? a.xs[(long)dd * a.npad + tj * TB + jj] : xjs[dd * TB + jj]; };
    auto xi2 = [&](int dd) -> T { return glb ? xrow2[(long)dd * ldr + g] : xis2[dd * TB + row]; };
    auto xj2 = [&](int dd, int jj) -> T { return glb ? a.xs2[(long)dd * a.npad + tj * TB + jj] : xjs2[dd * TB + jj]; };
    double acc1[32], acc2[32];
#pragma unroll
    for (int dd = 0; dd < 32; ++dd) acc1[dd] = acc2[dd] = 0.0;
    double acc_sf1 = 0.0, acc_sf2 = 0.0, acc_dg = 0.0, acc_a1 = 0.0, acc_a2 = 0.0, acc_c = 0.0;
    const T ag = (t < a.mc && !rect) ? a.alpha[g] : (T)0;
    const double bg = (a.beta && t < a.mc) ? (double)a.beta[g] : 0.0;
    const double* sp = a.slotp;
    const T sf2a = (T)sp[0], sf2b = (T)sp[SP_SF2B];
    __syncthreads();
    if (t < a.mc && (rect || g < a.n)) {
        for (int jj = half * 64; jj < half * 64 + 64; ++jj) {
            const int j = tj * TB + jj;
            if (j >= a.n) break;
            T r2a = (T)0, r2b = (T)0;
            for (int dd = 0; dd < d; ++dd) {
                const T u = xi1(dd) - xj1(dd, jj);
                r2a += u * u;
            }
            if (two)
                for (int dd = 0; dd < d; ++dd) {
                    const T u = xi2(dd) - xj2(dd, jj);
                    r2b += u * u;
                }
            T g1, m1, da1, g2 = (T)0, m2 = (T)0, da2 = (T)0;
            kfamily<T>(a.ks.fam1, r2a, (T)sp[SP_ALPHA1], g1, m1, da1);
            if (two) kfamily<T>(a.ks.fam2, r2b, (T)sp[SP_ALPHA2], g2, m2, da2);
            const double k1 = (double)sf2a * (double)g1, k2 = (double)sf2b * (double)g2;
            const double dk1 = (a.ks.op == 2) ? k2 : 1.0, dk2 = (a.ks.op == 2) ? k1 : 1.0;       // dk/dk1, dk/dk2
            const double w = grad_weight(a, wt, ag, aj[jj], bg, j, (double)a.Kinv[(long)j * a.ldv + t]);
            const double f1 = w * dk1 * (double)sf2a * (double)m1, f2 = w * dk2 * (double)sf2b * (double)m2;
#pragma unroll
            for (int q = 0; q < 32; ++q)               // (static indices: the accumulators stay in registers)
                if (d0 + q < d) {
                    const double u = (double)(xi1(d0 + q) - xj1(d0 + q, jj));
                    acc1[q] = __builtin_fma(f1, u * u, acc1[q]);
                }
            if (two) {
#pragma unroll
                for (int q = 0; q < 32; ++q)
                    if (d0 + q < d) {
                        const double u = (double)(xi2(d0 + q) - xj2(d0 + q, jj));
                        acc2[q] = __builtin_fma(f2, u * u, acc2[q]);
                    }
            }
            acc_sf1 = __builtin_fma(w * dk1, k1, acc_sf1);
            acc_sf2 = __builtin_fma(w * dk2, k2, acc_sf2);
            acc_a1 = __builtin_fma(w * dk1, (double)sf2a * (double)da1, acc_a1);
            acc_a2 = __builtin_fma(w * dk2, (double)sf2b * (double)da2, acc_a2);
            acc_c += w;
            if (j == g && !rect) acc_dg += w;
        }
    }
#pragma unroll
    for (int q = 0; q < 32; ++q)
        if (d0 + q < d) {
            out.put(acc1[q], d0 + q);
            if (two) out.put(acc2[q], d + 2 + d0 + q);
        }
    if (d0 == 0) {                                 // the scalar derivatives once, whatever the number of windows
        out.put(acc_sf1, d);
        out.put(acc_dg, d + 1);
        if (two) out.put(acc_sf2, 2 * d + 2);
        out.put(acc_a1, 2 * d + 3);
        if (two) out.put(acc_a2, 2 * d + 4);
        out.put(acc_c, 2 * d + 5);
    }
    out.finish();
}
template <typename T>
__global__ __launch_bounds__(256) void grad_reduce_general_kernel(GradArgs<T> a) { grad_reduce_general_tile<T>(a); }
template <typename T>
__global__ __launch_bounds__(256) void grad_reduce_general_slots_kernel(GradSlots<T> b) { grad_reduce_general_tile<T>(b.at((int)blockIdx.z)); }

// adds the per-workgroup rows of a gradient reduction into gacc: block p = accumulator slot p, fixed summation order
// (blockIdx.y = workspace slot of a group, part_ / gacc_bstride the doubles between the slots' rows and accumulators)
__global__ __launch_bounds__(256) void grad_finish_kernel(const double* __restrict__ part, long nwg, int np, double* __restrict__ gacc,
                                                          long part_bstride = 0, long gacc_bstride = 0) {
    __shared__ double s[256];
    const int p = blockIdx.x, tid = threadIdx.x;
    part += (long)blockIdx.y * part_bstride;
    gacc += (long)blockIdx.y * gacc_bstride;
    double v = 0.0;
    for (long w = tid; w < nwg; w += 256) v += part[w * np + p];
    s[tid] = v;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) s[tid] += s[tid + off];
        __syncthreads();
    }
    if (tid == 0) gacc[p] += s[0];
}

// Null kernel Function[0] (BGP:25-27, 156-159): K = diag(sn^2), so the quadratic form is
// sum (y_i - mu)^2 / sn^2.  One workgroup per theta, fixed-order reduction (deterministic):
// out[b] = { sum (y_i - mu_b), sum (y_i - mu_b)^2 }.
template <typename T>
__global__ __launch_bounds__(1024) void null_reduce_kernel(const T* __restrict__ y, int n, const double* __restrict__ mu,
                                                           double* __restrict__ out) {
    __shared__ double s1[16], s2[16];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double m = mu[b];
    double a1 = 0.0, a2 = 0.0;
    for (int i = tid; i < n; i += 1024) {
        const double r = (double)y[i] - m;
        a1 += r;
        a2 = __builtin_fma(r, r, a2);
    }
    for (int off = 32; off > 0; off >>= 1) {
        a1 += __shfl_down(a1, off);
        a2 += __shfl_down(a2, off);
    }
    if (lane == 0) { s1[wave] = a1; s2[wave] = a2; }
    __syncthreads();
    if (tid == 0) {
        double t1 = 0.0, t2 = 0.0;
        for (int w = 0; w < 16; ++w) { t1 += s1[w]; t2 += s2[w]; }
        out[2 * b] = t1;
        out[2 * b + 1] = t2;
    }
}

// Null kernel with point-dependent nugget / mean: K = diag(nu_i) (BGP:25-27, 156-159):
// out[b] = { sum log |nu_i|, sum (y_i - m_i)^2 / nu_i, #(nu_i not > 0) }; nug / mean: [b][n] (null = constant c_nug[b] / mu[b]).
template <typename T>
__global__ __launch_bounds__(1024) void null_reduce_pw_kernel(const T* __restrict__ y, int n, const double* __restrict__ mu,
                                                              const double* __restrict__ c_nug, const double* __restrict__ nug,
                                                              const double* __restrict__ mean, double* __restrict__ out) {
    __shared__ double s1[16], s2[16], s3[16];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int i = tid; i < n; i += 1024) {
        const double v = nug ? nug[(long)b * n + i] : c_nug[b];
        const double r = (double)y[i] - (mean ? mean[(long)b * n + i] : mu[b]);
        a1 += log(fabs(v));
        a2 += r * r / v;
        a3 += (v > 0.0) ? 0.0 : 1.0;
    }
    for (int off = 32; off > 0; off >>= 1) {
        a1 += __shfl_down(a1, off);
        a2 += __shfl_down(a2, off);
        a3 += __shfl_down(a3, off);
    }
    if (lane == 0) { s1[wave] = a1; s2[wave] = a2; s3[wave] = a3; }
    __syncthreads();
    if (tid == 0) {
        double t1 = 0.0, t2 = 0.0, t3 = 0.0;
        for (int w = 0; w < 16; ++w) { t1 += s1[w]; t2 += s2[w]; t3 += s3[w]; }
        out[3 * b] = t1;
        out[3 * b + 1] = t2;
        out[3 * b + 2] = t3;
    }
}

}  // namespace gphip
