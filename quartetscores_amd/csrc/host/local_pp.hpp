// local_pp.hpp -- a branch's local posterior probability, its two alternatives, its length in coalescent units and the polytomy test
// from the four words qs_branch_frequencies sums per branch: en = the trees that resolve a 4-set around the branch and
// Z_i = the sums of their normalised frequencies in 2^-40 units. Plain C++ (no HIP): QuartetScores --local-pp writes it, host_abi.cpp
// exports it as qsh_local_pp, engine.local_pp is the same arithmetic in Python.
//
// With z_i = Z_i / 2^40, prior rate lambda, a(x) = x + 1 and b(x) = en - x + 2 lambda (Sayyari & Mirarab 2016; the test is theirs of 2018):
//   h(x)   = B(a, b) (1 - I_{1/3}(a, b))                           B = beta function, I = regularised incomplete beta
//   pp_i   = 2^{z_i} h(z_i) / sum_j 2^{z_j} h(z_j)
//   theta  = z_1 / (en + 2 lambda - 1)
//   length = 0 where theta <= 1/3 (or negative, or not finite), inf where theta >= 1, else -ln(3/2 (1 - theta))
//   chi2   = sum_i (z_i - en/3)^2 / (en/3),   polytomy_p = exp(-chi2 / 2)   (2 degrees of freedom)
// Everything in log space: B(8001, 2001) underflows a double. 1 - I_{1/3}(a, b) = I_{2/3}(b, a), and the continued fraction of I_x(p, q)
// (modified Lentz) converges quickly where x < (p + 1) / (p + q + 2), which holds for exactly one of the two:
//   there for I_{2/3}(b, a):  ln h = b ln(2/3) + a ln(1/3) - ln b + ln cf(b, a, 2/3)           (B cancels: the small upper tail, directly)
//   else for  I_{1/3}(a, b):  ln h = ln B + log1p(-exp(a ln(1/3) + b ln(2/3) - ln B - ln a + ln cf(a, b, 1/3)))
// In the second case 1/3 lies below the mode side of the distribution, I_{1/3} is at most about a half and the subtraction loses nothing.
#pragma once

#include <cmath>
#include <cstdint>
#include <limits>

namespace qsh {

// the continued fraction of I_x(p, q) without its front factor x^p (1-x)^q / (p B(p, q)), for x < (p + 1) / (p + q + 2)
inline double beta_continued_fraction(double p, double q, double x) {
    const double tiny = 1e-300, eps = 1e-16;
    const double qab = p + q, qap = p + 1.0, qam = p - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (std::fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    // about sqrt(max(p, q)) steps are needed; below 2^23 trees that is under 3000
    for (int m = 1; m <= 100000; ++m) {
        const double m2 = 2.0 * m;
        double aa = m * (q - m) * x / ((qam + m2) * (p + m2));
        d = 1.0 + aa * d; if (std::fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(p + m) * (qab + m) * x / ((p + m2) * (qap + m2));
        d = 1.0 + aa * d; if (std::fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (std::fabs(del - 1.0) < eps) break;
    }
    return h;
}

// ln(B(a, b) (1 - I_{1/3}(a, b)))
inline double log_beta_upper_third(double a, double b) {
    const double l13 = std::log(1.0 / 3.0), l23 = std::log(2.0 / 3.0);
    if (2.0 / 3.0 < (b + 1.0) / (a + b + 2.0)) return b * l23 + a * l13 - std::log(b) + std::log(beta_continued_fraction(b, a, 2.0 / 3.0));
    const double log_beta = std::lgamma(a) + std::lgamma(b) - std::lgamma(a + b);
    const double log_lower = a * l13 + b * l23 - log_beta - std::log(a) + std::log(beta_continued_fraction(a, b, 1.0 / 3.0));
    return log_beta + std::log1p(-std::exp(log_lower));
}

// out = (pp1, pp2, pp3, length, polytomy_p); all nan where en <= 0
inline void local_pp(int64_t en, const int64_t Z[3], double lambda, double out[5]) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (en <= 0) { for (int i = 0; i < 5; ++i) out[i] = nan; return; }
    const double n = (double)en, one = 1099511627776.0;   // 2^40
    double z[3], w[3], top = -std::numeric_limits<double>::infinity();
    for (int i = 0; i < 3; ++i) {
        z[i] = (double)Z[i] / one;
        w[i] = z[i] * std::log(2.0) + log_beta_upper_third(z[i] + 1.0, n - z[i] + 2.0 * lambda);
        if (w[i] > top) top = w[i];
    }
    const double total = std::exp(w[0] - top) + std::exp(w[1] - top) + std::exp(w[2] - top);
    for (int i = 0; i < 3; ++i) out[i] = std::exp(w[i] - top) / total;
    const double theta = z[0] / (n + 2.0 * lambda - 1.0);
    if (!std::isfinite(theta) || theta <= 1.0 / 3.0) out[3] = 0.0;
    else if (theta >= 1.0) out[3] = std::numeric_limits<double>::infinity();
    else out[3] = -std::log(1.5 * (1.0 - theta));
    double chi2 = 0.0;
    for (int i = 0; i < 3; ++i) chi2 += (z[i] - n / 3.0) * (z[i] - n / 3.0) / (n / 3.0);
    out[4] = std::exp(-chi2 / 2.0);
}

} // namespace qsh
