// The host logic of the factor annotation (singlet_amd/csrc/annotate_host.h) as a program of its own: compiled by
// tests/test_annotate_restatement.py with a host compiler under -fsanitize=address,undefined and run on the CPU.
//   annotate_host_main            the special functions over a fixed grid, one line per value: name, arguments, result
//   annotate_host_main <file>     the statistics of the cases in <file>, one line per value: case, output name, index, result
// A case in <file>: rows G center scale proportion tail, then G counts, rows * G sums (column-major, row fastest), rows rss.
// The test compares every printed number with the scipy restatement (tests/annotate_restatement.py).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../singlet_amd/csrc/annotate_host.h"

static void grid() {
    const double xs[] = {1e-3, 0.05, 0.5, 1.0, 1.46, 1.5, 2.0, 3.7, 7.5, 11.99, 12.0, 50.0, 500.5, 5e3, 5e5, 1e9};
    for (double x : xs) {
        printf("digamma %.17g %.17g\n", x, annotate_digamma(x));
        printf("trigamma %.17g %.17g\n", x, annotate_trigamma(x));
    }
    const double ys[] = {1e-8, 1e-6, 2e-6, 1e-3, 0.01, 0.3, 1.0, 1.6449340668482264, 5.0, 100.0, 1e4, 9.9e6, 1e7, 2e7, 1e12};
    for (double y : ys) printf("trigamma_inverse %.17g %.17g\n", y, annotate_trigamma_inverse(y));
    // (5e4 and 99999: the continued fraction just below the large-df form, which serves 1e5 and above; 37.04 at +Inf: a tail
    // between 1e-300 and 1e-299)
    const double dfs[] = {1.0, 2.0, 2.5, 7.0, 30.0, 99.5, 1e3, 12345.6, 5e4, 99999.0, 1e5, 1e6, 1.5e6, 1e7, 1e9, INFINITY};
    const double ts[] = {0.0, 1e-8, 0.01, 0.5, 1.0, 2.0, 3.5, 6.0, 10.0, 17.0, 25.0, 37.0, 37.04, 40.0};
    for (double df : dfs)
        for (double t : ts)
            for (int sgn = 0; sgn < 2; ++sgn) {
                const double tv = sgn ? -t : t;
                printf("t_sf %.17g %.17g %.17g\n", tv, df, annotate_t_sf(tv, df));
            }
    const double ps[] = {0.4999, 0.3, 0.05, 1e-3, 1e-8, 1e-20, 1e-80, 1e-200, 1e-300};
    for (double df : dfs)
        for (double p : ps) {
            if (p < 1e-100 && df < 30.0) continue;   // quantiles beyond 1e100, where the yardstick's own tail underflows
            printf("t_isf %.17g %.17g %.17g\n", p, df, annotate_t_isf(p, df));
        }
}

static bool read_double(FILE* f, double* v) { return fscanf(f, "%lf", v) == 1; }

static int cases(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
    long long rows, G;
    int center, scale, tail, n_case = 0;
    double proportion;
    while (fscanf(f, "%lld %lld %d %d %lf %d", &rows, &G, &center, &scale, &proportion, &tail) == 6) {
        std::vector<int64_t> gn((size_t)G);
        std::vector<double> sum((size_t)(rows * G)), rss((size_t)rows);
        for (auto& v : gn) {
            long long t;
            if (fscanf(f, "%lld", &t) != 1) { fclose(f); return 3; }
            v = t;
        }
        for (auto& v : sum)
            if (!read_double(f, &v)) { fclose(f); return 3; }
        for (auto& v : rss)
            if (!read_double(f, &v)) { fclose(f); return 3; }
        const size_t R = (size_t)rows, RG = R * (size_t)G;
        std::vector<double> coef(RG), su((size_t)G), am(R), sg(R), post(R), sc(4), vp((size_t)G), t(RG), p(RG), pa(RG), lo(RG);
        annotate_stats(rows, (int32_t)G, gn.data(), sum.data(), rss.data(), center, scale, proportion, tail, coef.data(), su.data(), am.data(),
                       sg.data(), post.data(), sc.data(), vp.data(), t.data(), p.data(), pa.data(), lo.data());
        struct Out { const char* name; const std::vector<double>* v; };
        const Out outs[] = {{"coefficients", &coef}, {"stdev_unscaled", &su}, {"Amean", &am}, {"sigma", &sg}, {"s2_post", &post}, {"scalars", &sc},
                            {"var_prior", &vp}, {"t", &t}, {"p_raw", &p}, {"p_adj", &pa}, {"lods", &lo}};
        for (const Out& o : outs)
            for (size_t i = 0; i < o.v->size(); ++i) printf("%d %s %zu %.17g\n", n_case, o.name, i, (*o.v)[i]);
        // the same call with every output NULL touches nothing
        annotate_stats(rows, (int32_t)G, gn.data(), sum.data(), rss.data(), center, scale, proportion, tail, nullptr, nullptr, nullptr, nullptr,
                       nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        ++n_case;
    }
    fclose(f);
    printf("cases %d\n", n_case);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1) {
        const int rc = cases(argv[1]);
        if (rc) return rc;
    } else {
        grid();
        // the refusals of the arguments, and the naming of a defective label
        int64_t pos = 0;
        int32_t val = 0;
        const int32_t lab[5] = {0, -1, 2, 3, -2};
        if (annotate_check_args(nullptr, 5, 3, 1, &pos, &val) != ANNOTATE_ARGS_NULL) return 10;
        if (annotate_check_args(lab, 5, 0, 1, &pos, &val) != ANNOTATE_ARGS_GROUPS || annotate_check_args(lab, 5, 1025, 1, &pos, &val) != ANNOTATE_ARGS_GROUPS) return 11;
        if (annotate_check_args(lab, 5, 3, 0, &pos, &val) != ANNOTATE_ARGS_K || annotate_check_args(lab, 5, 3, 1025, &pos, &val) != ANNOTATE_ARGS_K) return 12;
        if (annotate_check_args(lab, 5, 3, 1, &pos, &val) != ANNOTATE_ARGS_LABEL || pos != 3 || val != 3) return 13;
        if (annotate_check_args(lab, 5, 4, 1024, &pos, &val) != ANNOTATE_ARGS_LABEL || pos != 4 || val != -2) return 14;
        if (annotate_check_args(lab, 4, 4, 1, &pos, &val) != ANNOTATE_ARGS_OK) return 15;
    }
    printf("annotate_host: ok\n");
    return 0;
}
