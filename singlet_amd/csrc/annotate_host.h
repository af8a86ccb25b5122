// Host logic of sgl_annotate (include/singlet_hip.h, "Factor annotation") that makes no HIP call: the argument rules and the
// naming of a defective label, the means-model fit from the three families of group moments, the prior of Smyth (2004,
// section 6.2), the moderated t with its p-values, the log-odds and Benjamini-Hochberg -- and the special functions under
// them (digamma, trigamma and its inverse, Student's t in both tails, a t quantile), which depend on libm alone.  Plain C++
// over plain pointers, so tests/annotate_host_main.cpp compiles it alone under -fsanitize=address,undefined and runs it on
// the CPU.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "gsea_host.h"   // gsea_bh: Benjamini-Hochberg over the values that are not NaN

#define ANNOTATE_MAX_GROUPS 1024
#define ANNOTATE_MAX_K 1024
#define ANNOTATE_SEG 8192   // stored entries per segment of the gene side's residual pass: part of the stated summation order

enum AnnotateArgError {
    ANNOTATE_ARGS_OK = 0,
    ANNOTATE_ARGS_NULL,     // labels == NULL
    ANNOTATE_ARGS_GROUPS,   // n_groups outside [1, 1024]
    ANNOTATE_ARGS_K,        // k outside [1, 1024]
    ANNOTATE_ARGS_LABEL,    // labels[*pos] = *val is outside [-1, n_groups)
};

// The refusals that need no device, in this order; the whole list is read before anything is launched.
inline AnnotateArgError annotate_check_args(const int32_t* labels, int64_t n, int32_t n_groups, int32_t k, int64_t* pos, int32_t* val) {
    *pos = -1;
    *val = 0;
    if (!labels) return ANNOTATE_ARGS_NULL;
    if (n_groups < 1 || n_groups > ANNOTATE_MAX_GROUPS) return ANNOTATE_ARGS_GROUPS;
    if (k < 1 || k > ANNOTATE_MAX_K) return ANNOTATE_ARGS_K;
    for (int64_t j = 0; j < n; ++j)
        if (labels[j] < -1 || labels[j] >= n_groups) { *pos = j; *val = labels[j]; return ANNOTATE_ARGS_LABEL; }
    return ANNOTATE_ARGS_OK;
}

// ---- special functions ------------------------------------------------------------------------------------------------------
// psi(x), x > 0: the recurrence psi(x) = psi(x + 1) - 1 / x up to x >= 12, then the asymptotic series
inline double annotate_digamma(double x) {
    if (!(x > 0.0)) return NAN;
    if (x == INFINITY) return INFINITY;
    double r = 0.0;
    while (x < 12.0) { r -= 1.0 / x; x += 1.0; }
    const double i = 1.0 / x, i2 = i * i;
    const double tail = i2 * (1.0 / 12 - i2 * (1.0 / 120 - i2 * (1.0 / 252 - i2 * (1.0 / 240 - i2 * (1.0 / 132 - i2 * (691.0 / 32760 - i2 / 12))))));
    return r + (log(x) - 0.5 * i - tail);
}
// psi'(x), x > 0
inline double annotate_trigamma(double x) {
    if (!(x > 0.0)) return NAN;
    if (x == INFINITY) return 0.0;
    double r = 0.0;
    while (x < 12.0) { r += 1.0 / (x * x); x += 1.0; }
    const double i = 1.0 / x, i2 = i * i;
    const double tail = i * i2 * (1.0 / 6 - i2 * (1.0 / 30 - i2 * (1.0 / 42 - i2 * (1.0 / 30 - i2 * (5.0 / 66 - i2 * (691.0 / 2730 - i2 * 7.0 / 6))))));
    return r + (i + 0.5 * i2 + tail);
}
// psi''(x), x > 0 (steers the Newton steps of the inverse trigamma; its accuracy does not bound the result's)
inline double annotate_tetragamma(double x) {
    double r = 0.0;
    while (x < 12.0) { r -= 2.0 / (x * x * x); x += 1.0; }
    const double i = 1.0 / x, i2 = i * i;
    return r - i2 * (1.0 + i + i2 * (0.5 - i2 * (1.0 / 6 - i2 * (1.0 / 6 - i2 * (3.0 / 10 - i2 * (5.0 / 6 - i2 * 691.0 / 210))))));
}
// the y > 0 with psi'(y) = x, x > 0: Newton on 1 / psi', which is convex and nearly linear, from y = 0.5 + 1 / x (below the root)
inline double annotate_trigamma_inverse(double x) {
    if (!(x > 0.0)) return NAN;
    if (x == INFINITY) return 0.0;
    if (x > 1e30) return 1.0 / sqrt(x);   // psi'(y) = 1 / y^2 + pi^2 / 6 + ...: the correction is below one unit in the last place
    if (x < 1e-30) return 1.0 / x;
    double y = 0.5 + 1.0 / x;
    for (int it = 0; it < 200; ++it) {
        const double tri = annotate_trigamma(y);
        const double dif = tri * (1.0 - tri / x) / annotate_tetragamma(y);
        y += dif;
        if (fabs(dif) <= 4e-16 * y) break;
    }
    return y;
}

// log(Gamma(a + 1/2) / Gamma(a)), a > 0: lgamma's difference loses digits as a grows; from a = 40 on the Stirling series
inline double annotate_lgamma_ratio_half(double a) {
    if (a < 40.0) return lgamma(a + 0.5) - lgamma(a);
    const double i = 1.0 / a, i2 = i * i;
    return 0.5 * log(a) - i * (1.0 / 8 - i2 * (1.0 / 192 - i2 * (1.0 / 640 - i2 * 17.0 / 14336)));
}
// the continued fraction of the incomplete beta function (modified Lentz); xc = 1 - x, given by the caller without a
// subtraction: the first denominator 1 - (a + b) x / (a + 1) cancels when a is large and x near 1, and is formed from xc there
inline double annotate_betacf(double a, double b, double x, double xc) {
    const double tiny = 1e-300, qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = x < 0.5 ? 1.0 - qab * x / qap : ((1.0 - b) + qab * xc) / qap;
    if (fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= 1000000; ++m) {
        const double m2 = 2.0 * m;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) <= 2.3e-16) break;
    }
    return h;
}
// P(T > t), t > 0, for df >= 1e5, where the continued fraction below loses digits (its denominators cancel like 1 / (t^2 / df)).
// With b = (df + 1) / 2 and y^2 = b log1p(s^2 / df) the tail is  C sqrt(df / b) * integral over y >= y_t of exp(-y^2) G(y^2 / b),
// ln G(w) = 3 w / 4 - w^2 / 48 + w^4 / 5760 - w^6 / 362880 (from ln((e^w - 1) / w); w <= 0.02 here).  Around w_t, ln G is
// linear in q = y^2 - y_t^2 up to q^2 / (48 b^2): the linear part makes the integral a Gaussian one, erfc exactly; the
// quadratic part is a factor 1 - M2 / (48 b^2), M2 the mean of q^2 under that weight.  What is left out is below 1e-15.
inline double annotate_t_upper_large(double t, double df) {
    const double v = 0.5 * df, b = v + 0.5, L = log1p((t / df) * t), a = b * L;   // a = y_t^2
    const double L2 = L * L, lnG = L * (0.75 - L / 48 + L * L2 / 5760 - L * L2 * L2 / 362880);
    const double kappa = (0.75 - L / 24 + L * L2 / 1440) / b, lam = 1.0 - kappa;
    const double yt = sqrt(a);
    double R;   // exp(-a) / integral of exp(-y^2) over y >= y_t
    if (yt < 6.0) {
        R = exp(-a) / (0.5 * sqrt(M_PI) * erfc(yt));
    } else {
        const double ia = 1.0 / a;
        R = 2.0 * yt / (1.0 - ia * (0.5 - ia * (0.75 - ia * (15.0 / 8 - ia * 105.0 / 16))));
    }
    const double M2 = ((a * a - a) + 0.75) - yt * R * (0.5 * a - 0.75);
    const double front = exp(annotate_lgamma_ratio_half(v) + lnG - kappa * a) / (2.0 * sqrt(b * lam));
    return front * erfc(sqrt(a * lam)) * (1.0 - M2 / (48.0 * b * b));
}
// P(T > t) for t >= 0 and T Student's t with df > 0 degrees of freedom (real-valued; +Inf: the normal distribution):
// 0.5 I_x(df / 2, 1 / 2) at x = df / (df + t^2), with x and 1 - x both formed without a subtraction, so that a tiny tail
// keeps its relative accuracy
inline double annotate_t_upper(double t, double df) {
    if (t != t || !(df > 0.0)) return NAN;
    if (t == INFINITY) return 0.0;
    if (df == INFINITY) return 0.5 * erfc(t * M_SQRT1_2);
    if (t == 0.0) return 0.5;
    if (df >= 1e5) return annotate_t_upper_large(t, df);
    const double v = 0.5 * df, u = (t / df) * t;   // t^2 / df
    // x = 1 / (1 + u) and log x; a t whose square overflows goes through logarithms
    const bool huge = !(u < 1e300);
    const double lx = huge ? -(2.0 * log(t) - log(df)) : -log1p(u);
    const double x = huge ? exp(lx) : 1.0 / (1.0 + u), xc = huge ? 1.0 : u / (1.0 + u);
    const double lbeta = 0.5 * log(M_PI) - annotate_lgamma_ratio_half(v);   // log B(df / 2, 1 / 2)
    const double front = exp(v * lx + 0.5 * log(xc) - lbeta);
    if (x < (v + 1.0) / (v + 2.5)) return 0.5 * (front * annotate_betacf(v, 0.5, x, xc) / v);
    return 0.5 * (1.0 - front * annotate_betacf(0.5, v, xc, x) / 0.5);
}
// P(T > t) for any t
inline double annotate_t_sf(double t, double df) { return t >= 0.0 ? annotate_t_upper(t, df) : 1.0 - annotate_t_upper(-t, df); }
// the q with P(T > q) = p, 0 < p < 1: bisection on the bracket found by doubling
inline double annotate_t_isf(double p, double df) {
    if (!(p > 0.0 && p < 1.0) || !(df > 0.0)) return p == 0.0 ? INFINITY : (p == 1.0 ? -INFINITY : NAN);
    if (p > 0.5) return -annotate_t_isf(1.0 - p, df);
    if (p == 0.5) return 0.0;
    double lo = 0.0, hi = 1.0;
    while (hi < 1e300 && annotate_t_upper(hi, df) > p) { lo = hi; hi *= 2.0; }
    for (int it = 0; it < 200; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (!(mid > lo && mid < hi)) break;
        if (annotate_t_upper(mid, df) > p) lo = mid; else hi = mid;
    }
    return 0.5 * (lo + hi);
}

// ---- the fit and the moderated statistics --------------------------------------------------------------------------------------
// group_n[G]; sum, and every per-(row, group) output: rows x G column-major (row fastest); rss and every per-row output: rows.
// stdev_unscaled and var_prior: G.  scalars: df_residual, s2_prior, df_prior, df_total.  Any output may be NULL.  The rules are
// those of include/singlet_hip.h ("Factor annotation"), operation by operation.
inline void annotate_stats(int64_t rows, int32_t G, const int64_t* group_n, const double* sum, const double* rss, int center, int scale,
                           double proportion, int tail, double* coef, double* stdev_unscaled, double* amean, double* sigma, double* s2_post,
                           double* scalars, double* var_prior, double* t_out, double* p_raw, double* p_adj, double* lods) {
    const size_t R = (size_t)rows, RG = R * (size_t)G;
    int64_t N = 0;
    int32_t Gp = 0;
    for (int32_t g = 0; g < G; ++g) { N += group_n[g]; Gp += group_n[g] > 0 ? 1 : 0; }
    const int64_t dfi = N - Gp;
    const double df = (double)dfi, dN = (double)N;
    std::vector<double> vcoef(RG, NAN), vt(RG, NAN), vp(RG, NAN), vl(RG, NAN), vs2(R, NAN), vpost(R, NAN), vam(R, NAN), su((size_t)G, NAN),
        vprior((size_t)G, NAN);
    double s2_prior = NAN, df_prior = NAN, df_total = NAN;
    if (dfi > 0) {
        for (int32_t g = 0; g < G; ++g)
            if (group_n[g] > 0) su[g] = 1.0 / sqrt((double)group_n[g]);
        // the fit
        for (size_t r = 0; r < R; ++r) {
            double grand = 0.0;
            for (int32_t g = 0; g < G; ++g) grand += sum[r + R * g];
            const double am = grand / dN;
            vam[r] = am;
            double s2 = rss[r] / df, sd = 1.0;
            if (scale) {
                double tss = rss[r];
                for (int32_t g = 0; g < G; ++g)
                    if (group_n[g] > 0) {
                        const double d = sum[r + R * g] / (double)group_n[g] - am;
                        tss += (double)group_n[g] * (d * d);
                    }
                sd = sqrt(tss / (dN - 1.0));
                s2 = s2 / (sd * sd);
            }
            vs2[r] = s2;
            for (int32_t g = 0; g < G; ++g)
                if (group_n[g] > 0) {
                    double cf = sum[r + R * g] / (double)group_n[g] - (center ? am : 0.0);
                    if (scale) cf = cf / sd;
                    vcoef[r + R * g] = cf;
                }
        }
        // the prior
        std::vector<double> x;
        x.reserve(R);
        for (size_t r = 0; r < R; ++r)
            if (vs2[r] >= 0.0 && vs2[r] < INFINITY) x.push_back(vs2[r]);
        const size_t nu = x.size();
        if (nu >= 2) {
            std::vector<double> srt(x);
            std::sort(srt.begin(), srt.end());
            double med = nu % 2 ? srt[nu / 2] : (srt[nu / 2 - 1] + srt[nu / 2]) / 2.0;
            if (med == 0.0) med = 1.0;
            const double floor_x = 1e-5 * med, shift = log(df / 2.0) - annotate_digamma(df / 2.0);
            double emean = 0.0;
            for (size_t i = 0; i < nu; ++i) {
                x[i] = log(x[i] > floor_x ? x[i] : floor_x) + shift;
                emean += x[i];
            }
            emean /= (double)nu;
            double ss = 0.0;
            for (size_t i = 0; i < nu; ++i) ss += (x[i] - emean) * (x[i] - emean);
            const double evar = ss / (double)(nu - 1) - annotate_trigamma(df / 2.0);
            if (evar > 0.0) {
                df_prior = 2.0 * annotate_trigamma_inverse(evar);
                s2_prior = exp(emean + annotate_digamma(df_prior / 2.0) - log(df_prior / 2.0));
            } else {
                df_prior = INFINITY;
                s2_prior = exp(emean);
            }
        } else {
            df_prior = 0.0;   // no shrinkage: s2_post = s2 (s2_prior stays NaN)
        }
        df_total = df + df_prior;
        if ((double)nu * df < df_total) df_total = (double)nu * df;
        if (nu == 0) df_total = NAN;
        for (size_t r = 0; r < R; ++r) {
            if (!(vs2[r] >= 0.0 && vs2[r] < INFINITY)) continue;
            vpost[r] = df_prior == 0.0 ? vs2[r] : df_prior == INFINITY ? s2_prior : (df * vs2[r] + df_prior * s2_prior) / (df + df_prior);
        }
        // moderated t, p and log-odds
        std::vector<double> at;
        std::vector<int64_t> order;
        const double lprop = log(proportion / (1.0 - proportion));
        for (int32_t g = 0; g < G; ++g) {
            if (!(group_n[g] > 0)) continue;
            at.assign(R, NAN);
            order.clear();
            for (size_t r = 0; r < R; ++r) {
                const double tv = vcoef[r + R * g] / (su[g] * sqrt(vpost[r]));
                vt[r + R * g] = tv;
                if (tv == tv) {
                    at[r] = fabs(tv);
                    order.push_back((int64_t)r);
                    vp[r + R * g] = tail == 0 ? annotate_t_sf(tv, df_total) : tail == 1 ? annotate_t_sf(-tv, df_total) : 2.0 * annotate_t_upper(at[r], df_total);
                }
            }
            // var_prior: the rows that count are those whose t is a number
            const int64_t nr = (int64_t)order.size();
            if (nr == 0) continue;
            const int64_t ntarget = (int64_t)ceil(proportion / 2.0 * (double)nr);
            std::sort(order.begin(), order.end(), [&at](int64_t a, int64_t b) { return at[a] > at[b] || (at[a] == at[b] && a < b); });
            const double pp = std::max((double)ntarget / (double)nr, proportion), su2 = su[g] * su[g];
            double vsum = 0.0;
            for (int64_t i = 1; i <= ntarget && i <= nr; ++i) {
                const double ta = at[order[(size_t)i - 1]];
                const double p0 = 2.0 * annotate_t_upper(ta, df_total);
                const double ptarget = (((double)i - 0.5) / (double)nr - (1.0 - pp) * p0) / pp;
                double v0 = 0.0;
                if (ptarget > p0) {
                    const double q = annotate_t_isf(ptarget / 2.0, df_total), ratio = ta / q;
                    v0 = su2 * (ratio * ratio - 1.0);
                }
                v0 = v0 < 0.01 ? 0.01 : (v0 > 16.0 ? 16.0 : v0);   // (a NaN is raised to 0.01 by neither comparison: it stays)
                vsum += v0;
            }
            const double vpg = vsum / (double)std::min(ntarget, nr);
            vprior[g] = vpg;
            const double rr = (su2 + vpg) / su2;
            for (size_t r = 0; r < R; ++r) {
                const double tv = vt[r + R * g];
                if (tv != tv) continue;
                const double t2 = tv * tv;
                double kernel;
                if (df_prior > 1e6) kernel = t2 * (1.0 - 1.0 / rr) / 2.0;
                else kernel = (1.0 + df_total) / 2.0 * log((t2 + df_total) / (t2 / rr + df_total));
                vl[r + R * g] = lprop - log(rr) / 2.0 + kernel;
            }
        }
    }
    if (scalars) { scalars[0] = df; scalars[1] = s2_prior; scalars[2] = df_prior; scalars[3] = df_total; }
    if (coef) std::copy(vcoef.begin(), vcoef.end(), coef);
    if (stdev_unscaled) std::copy(su.begin(), su.end(), stdev_unscaled);
    if (amean) std::copy(vam.begin(), vam.end(), amean);
    if (sigma)
        for (size_t r = 0; r < R; ++r) sigma[r] = sqrt(vs2[r]);
    if (s2_post) std::copy(vpost.begin(), vpost.end(), s2_post);
    if (var_prior) std::copy(vprior.begin(), vprior.end(), var_prior);
    if (t_out) std::copy(vt.begin(), vt.end(), t_out);
    if (p_raw) std::copy(vp.begin(), vp.end(), p_raw);
    if (lods) std::copy(vl.begin(), vl.end(), lods);
    if (p_adj && RG > 0) gsea_bh(vp.data(), (int64_t)RG, p_adj);
}
