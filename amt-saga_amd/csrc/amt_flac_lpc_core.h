// Linear-prediction analysis of the FLAC encoder: plain C++ behind one macro, so the same functions compile into the frame
// kernel of amt_flac.hip and into a stand-alone CPU program (tests/flac_lpc_host_main.cpp, built with the address and
// undefined-behaviour sanitizers).  tests/flac_lpc_reference.py restates every step in numpy; DESIGN.md 20 has the rule.
//
//   window           w_i = ((4 (i + 1)(bs - i)) << 14) / (bs + 1)^2,  x_i = (q_i w_i) >> 14        (int64, floor)
//   autocorrelation  R_l = sum_i x_i x_(i-l), l = 0 .. 12: exact in int64 (|R| < 2^59), any summation order
//   recurrence       float64 on r_l = (double)R_l, ONE operation order (fll_analyse), IEEE add / subtract / multiply /
//                    divide only, no fused multiply-add: err = r_0; at order m
//                        acc = r_m;  for j < m - 1: acc = acc - a_j r_(m-1-j)
//                        k = acc / err;  a'_j = a_j - k a_(m-2-j) (j < m - 1), a'_(m-1) = k
//                        (order m's coefficients are quantised here)
//                        err = err (1 - k k);  no higher order unless err > 0
//   quantiser        P = 14 (24 bit) or 12 (16 bit); max |a_j| = f 2^e, f in [0.5, 1) (exponent field of the bit pattern);
//                    shift = clamp(P - 1 - e, 0, 15); fe = 0; per j: fe = fe + a_j 2^shift,
//                    c_j = clamp(rint(fe), -2^(P-1), 2^(P-1) - 1), fe = fe - c_j.  An order whose largest coefficient is 0
//                    or that holds a value that is not finite has no candidate.
//   residual         r_i = q_i - ((sum_j c_j q_(i-1-j)) >> shift), int64 sum, arithmetic shift; a candidate with any
//                    |r_i| >= 2^27 is disqualified, so u < 2^28 as for the fixed predictors.
#ifndef AMT_FLAC_LPC_CORE_H
#define AMT_FLAC_LPC_CORE_H

#ifdef __HIP__
#define AMT_FLL_HD __host__ __device__ inline
#else
#define AMT_FLL_HD inline
#endif

#define FLL_MAX_ORDER 12
#define FLL_LAGS (FLL_MAX_ORDER + 1)
#define FLL_WORK (FLL_LAGS + 2 * FLL_MAX_ORDER)      /* doubles fll_analyse works in */
#define FLL_RESID_LIMIT (1LL << 27)

typedef long long fll_i64;
typedef unsigned long long fll_u64;

AMT_FLL_HD int fll_precision(int bps) { return bps == 16 ? 12 : 14; }

AMT_FLL_HD fll_i64 fll_window(int i, int bs) {
    const fll_i64 d = (fll_i64)(bs + 1) * (bs + 1);
    return (((fll_i64)4 * (i + 1) * (bs - i)) << 14) / d;        // both positive: the floor
}

AMT_FLL_HD int fll_windowed(int q, int i, int bs) { return (int)(((fll_i64)q * fll_window(i, bs)) >> 14); }

AMT_FLL_HD fll_u64 fll_double_bits(double v) { fll_u64 u; __builtin_memcpy(&u, &v, 8); return u; }
AMT_FLL_HD double fll_bits_double(fll_u64 u) { double v; __builtin_memcpy(&v, &u, 8); return v; }
AMT_FLL_HD int fll_exp_field(double v) { return (int)((fll_double_bits(v) >> 52) & 0x7ffu); }

// Coefficients a[0 .. m) -> c[0 .. m) of P bits; returns the shift, or -1 where the order has no candidate.
AMT_FLL_HD int fll_quantise(const double *a, int m, int P, int *c) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double cmax = 0.0;
    for (int j = 0; j < m; ++j) {
        if (fll_exp_field(a[j]) == 0x7ff) return -1;              // infinity or NaN
        const double v = fll_bits_double(fll_double_bits(a[j]) & ~(1ULL << 63));
        if (v > cmax) cmax = v;
    }
    if (!(cmax > 0.0)) return -1;
    const int e = fll_exp_field(cmax) - 1022;                     // cmax = f 2^e, f in [0.5, 1); a subnormal counts as 2^-1022
    int shift = P - 1 - e;
    shift = shift < 0 ? 0 : (shift > 15 ? 15 : shift);
    const double scale = fll_bits_double((fll_u64)(1023 + shift) << 52);
    const double hi = (double)((1 << (P - 1)) - 1), lo = -(double)(1 << (P - 1));
    double fe = 0.0;
    for (int j = 0; j < m; ++j) {
        fe = fe + a[j] * scale;
        double v = __builtin_rint(fe);
        v = v > hi ? hi : (v < lo ? lo : v);
        c[j] = (int)v;
        fe = fe - v;
    }
    return shift;
}

// Autocorrelation R[0 .. max_order] -> for every order m = 1 .. max_order (<= FLL_MAX_ORDER) its shift[m - 1] (-1: no
// candidate) and its coefficients coef[(m - 1) FLL_MAX_ORDER + j], j < m.  work: FLL_WORK doubles.
AMT_FLL_HD void fll_analyse(const fll_i64 *R, int max_order, int P, double *work, int *coef, int *shift) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double *r = work, *a = work + FLL_LAGS, *t = a + FLL_MAX_ORDER;
    for (int m = 0; m < FLL_MAX_ORDER; ++m) shift[m] = -1;
    if (R[0] <= 0) return;
    for (int l = 0; l <= max_order; ++l) r[l] = (double)R[l];
    double err = r[0];
    for (int m = 1; m <= max_order; ++m) {
        double acc = r[m];
        for (int j = 0; j < m - 1; ++j) acc = acc - a[j] * r[m - 1 - j];
        const double k = acc / err;
        for (int j = 0; j < m - 1; ++j) t[j] = a[j] - k * a[m - 2 - j];
        for (int j = 0; j < m - 1; ++j) a[j] = t[j];
        a[m - 1] = k;
        shift[m - 1] = fll_quantise(a, m, P, coef + (m - 1) * FLL_MAX_ORDER);
        const double kk = k * k;
        err = err * (1.0 - kk);
        if (!(err > 0.0)) break;
    }
}

// the residual of sample i >= m
AMT_FLL_HD fll_i64 fll_resid(const int *q, int i, const int *c, int m, int shift) {
    fll_i64 s = 0;
    for (int j = 0; j < m; ++j) s += (fll_i64)c[j] * q[i - 1 - j];
    return (fll_i64)q[i] - (s >> shift);
}

AMT_FLL_HD bool fll_resid_ok(fll_i64 r) { return r > -FLL_RESID_LIMIT && r < FLL_RESID_LIMIT; }

#endif
