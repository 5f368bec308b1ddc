// The per-matrix arithmetic of the residual check of a tridiagonal factorisation (specification: include/basd_hip.h) as
// host + device functions: the layout of the probe buffer, one term of the probe's sums, one component of
// Q^T (A x) - T (Q^T x), the three ratios with their 0 / 0 rule, and the verdict bits.  csrc/tridiag_check.hip calls them
// from its two kernels (which add the parallel reductions, in a fixed order); tools/tridiag_check_host_check.cpp compiles
// the same text for the host under the sanitizers and runs the serial drivers at the end of this file.  Nothing here
// allocates, and nothing touches memory other than the arrays it is handed.
#pragma once
#include "../../include/basd_hip.h"

#include <math.h>

#ifndef BASD_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define BASD_HD __host__ __device__ __forceinline__
#else
#define BASD_HD inline
#endif
#endif

namespace basd {

constexpr double kTridiagCheckEps = 5.9604644775390625e-08;          // 2^-24
constexpr int kTridiagCtlWords = 8;                                  // done, failed, first, mask, worst[3], spare
constexpr unsigned kTridiagNoFirst = 0x7FFFFFFFu;

struct TridiagProbeLayout {            // byte offsets into the probe buffer; every one a multiple of 16
    long parts, sums, ctl, bytes;
    int n_parts;
};

BASD_HD TridiagProbeLayout tridiag_probe_layout(int n, int batch) {
    TridiagProbeLayout l;
    l.n_parts = (n + BASD_TRIDIAG_PROBE_ROWS - 1) / BASD_TRIDIAG_PROBE_ROWS;
    l.parts = (((long)batch * 2 * n * (long)sizeof(float)) + 15) & ~15L;
    l.sums = l.parts + (long)batch * l.n_parts * 2 * (long)sizeof(double);
    l.ctl = l.sums + (long)batch * 2 * (long)sizeof(double);
    l.bytes = l.ctl + kTridiagCtlWords * (long)sizeof(unsigned);
    return l;
}

// What the probe launch leaves in control word w, and what the last workgroup of a check puts back.
BASD_HD unsigned tridiag_ctl_initial(int w) { return w == 2 ? kTridiagNoFirst : 0u; }

// One element a = A(i, j) of a row: its share of y_i = sum_j A(i, j) x_j and of |A|_F^2.  x_j is +-1 (0 past the end), so
// both products are exact in fp64 and only the additions round.
BASD_HD void tridiag_probe_term(float a, float xj, double& y, double& f) {
    y += (double)a * (double)xj;
    f += (double)a * (double)a;
}

// Component i of Q^T (A x) - T (Q^T x):  v = Q^T y, u = Q^T x, T = tridiag(d, e) with e[0 .. n - 2].
BASD_HD double tridiag_residual_term(const float* d, const float* e, const float* u, const float* v, int n, int i) {
    double t = (double)d[i] * (double)u[i];
    if (i + 1 < n) t += (double)e[i] * (double)u[i + 1];
    if (i > 0) t += (double)e[i - 1] * (double)u[i - 1];
    return (double)v[i] - t;
}

// num / den with the zero matrix's 0 / 0 taken as 0; anything else (x / 0, NaN) is left for the comparison to reject.
BASD_HD double tridiag_check_ratio(double num, double den) { return (num == 0.0 && den == 0.0) ? 0.0 : num / den; }

// rho[0 .. 2] = rho_trace, rho_fro, rho_res from the fp64 sums.
BASD_HD void tridiag_check_ratios(double sum_d, double sum_d2, double sum_e2, double res2, double tr, double fro2, int n,
                                  double* rho) {
    const double fro = sqrt(fro2);
    rho[0] = tridiag_check_ratio(fabs(sum_d - tr), kTridiagCheckEps * fro);
    rho[1] = tridiag_check_ratio(fabs(sum_d2 + 2.0 * sum_e2 - fro2), kTridiagCheckEps * fro2);
    rho[2] = tridiag_check_ratio(sqrt(res2), kTridiagCheckEps * fro * sqrt((double)n));
}

// BASD_TRIDIAG_CHECK_BIT_* of the ratios that are not <= their thresholds (so every NaN fails).
BASD_HD int tridiag_check_mask(const double* rho, const float* thr) {
    int mask = 0;
    for (int k = 0; k < 3; ++k)
        if (!(rho[k] <= (double)thr[k])) mask |= 1 << k;
    return mask;
}

BASD_HD void tridiag_check_default_thresholds(int n, float* thr) {
    const double r = sqrt((double)n);
    thr[0] = (float)(BASD_TRIDIAG_CHECK_TRACE_PER_SQRT_N * r);
    thr[1] = (float)(BASD_TRIDIAG_CHECK_FRO_PER_SQRT_N * r);
    thr[2] = (float)BASD_TRIDIAG_CHECK_RES;
}

// ---- serial drivers (the host check; the kernels run the same terms under their own reductions) -----------------
// xy: (2, n) -- x and y = A x of matrix index m; sums[0] = tr A, sums[1] = |A|_F^2.
BASD_HD void tridiag_probe_serial(const float* a, int n, unsigned m, float* xy, double* sums) {
    double tr = 0.0, fro2 = 0.0;
    for (int i = 0; i < n; ++i) {
        double y = 0.0;
        for (int j = 0; j < n; ++j) tridiag_probe_term(a[(long)i * n + j], basd_tridiag_probe_sign(m, (uint32_t)j), y, fro2);
        tr += (double)a[(long)i * n + i];
        xy[i] = basd_tridiag_probe_sign(m, (uint32_t)i);
        xy[n + i] = (float)y;
    }
    sums[0] = tr;
    sums[1] = fro2;
}

// uv: (2, n) = Q^T of the two probe rows.  Returns the verdict bits; rho[0 .. 2] receive the ratios.
BASD_HD int tridiag_check_serial(const float* d, const float* e, const float* uv, const double* sums, int n,
                                 const float* thr, double* rho) {
    double sd = 0.0, sd2 = 0.0, se2 = 0.0, r2 = 0.0;
    for (int i = 0; i < n; ++i) {
        sd += (double)d[i];
        sd2 += (double)d[i] * (double)d[i];
        if (i + 1 < n) se2 += (double)e[i] * (double)e[i];
        const double r = tridiag_residual_term(d, e, uv, uv + n, n, i);
        r2 += r * r;
    }
    tridiag_check_ratios(sd, sd2, se2, r2, sums[0], sums[1], n, rho);
    return tridiag_check_mask(rho, thr);
}

}  // namespace basd
