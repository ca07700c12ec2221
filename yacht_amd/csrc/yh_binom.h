// yh_binom.h — the binomial distribution function of `yacht run`'s presence test, once, for the host and the device.
//
// Loader's saddle-point point probabilities (C. Loader, "Fast and accurate computation of binomial probabilities", 2000:
// log pmf from Stirling-series errors and the deviance terms) and P[Bin(n, p) <= k] as the SHORTER tail summed outward
// from k by the exact term ratio.  Templated on the floating type T of the point probability and the tail sum:
// yh_hyp.cpp instantiates it with long double (host), yh_presence.hip with double (device).  `small` is the table
// stirlerr(0..15), which the caller computes once (yh_binom_stirlerr_table); `cut` ends a tail sum once a term falls
// below cut times the sum.
#pragma once

#include <math.h>

#include <cmath>

#if defined(__HIP__)
#define YH_BINOM_HD __host__ __device__
#else
#define YH_BINOM_HD
#endif

namespace yh_binom {

// log(n!) - log(sqrt(2 pi n) (n/e)^n) for n = 0..15, evaluated in T (the host's exact factorials up to 15!)
template <typename T>
inline void stirlerr_table(T* t) {
    t[0] = 0;
    T fact = 1;
    for (int i = 1; i <= 15; ++i) {
        fact *= (T)i;
        t[i] = std::log(fact) - ((T)i + (T)0.5L) * std::log((T)i) + (T)i - (T)0.918938533204672741780329736406L;
    }
}

// log(n!) - log(sqrt(2 pi n) (n/e)^n) for integer n >= 1 (0 for n = 0: never used as a factor)
template <typename T>
YH_BINOM_HD inline T stirlerr(T n, const T* small) {
    if (n <= (T)15) return small[(int)n];
    const T S0 = (T)1 / (T)12, S1 = (T)1 / (T)360, S2 = (T)1 / (T)1260, S3 = (T)1 / (T)1680, S4 = (T)1 / (T)1188,
            S5 = (T)691 / (T)360360;
    const T nn = n * n;
    if (n > 500) return (S0 - (S1 - S2 / nn) / nn) / n;
    if (n > 80) return (S0 - (S1 - (S2 - S3 / nn) / nn) / nn) / n;
    return (S0 - (S1 - (S2 - (S3 - (S4 - S5 / nn) / nn) / nn) / nn) / nn) / n;
}

// x log(x / np) + np - x without cancellation near x = np
template <typename T>
YH_BINOM_HD inline T bd0(T x, T np) {
    if (std::fabs(x - np) < (T)0.1L * (x + np)) {
        T v = (x - np) / (x + np);
        T s = (x - np) * v;
        T ej = 2 * x * v;
        v = v * v;
        for (int j = 1; j < 1000; ++j) {
            ej *= v;
            const T s1 = s + ej / ((j << 1) + 1);
            if (s1 == s) return s1;
            s = s1;
        }
        return s;
    }
    return x * std::log(x / np) + np - x;
}

// log P[Bin(n, p) = x], 0 <= x <= n, q = 1 - p
template <typename T>
YH_BINOM_HD inline T log_pmf(double xd, double nd, double pd, double qd, const T* small) {
    const T x = xd, n = nd, p = pd, q = qd;
    if (p <= (T)0) return x == 0 ? (T)0 : (T)-INFINITY;
    if (q <= (T)0) return x == n ? (T)0 : (T)-INFINITY;
    if (x == 0) return n * (p < (T)0.5L ? std::log1p(-p) : std::log(q));  // (whichever of p, q is the small, exactly known one)
    if (x == n) return n * (q < (T)0.5L ? std::log1p(-q) : std::log(p));
    const T lc = stirlerr(n, small) - stirlerr(x, small) - stirlerr(n - x, small) - bd0(x, n * p) - bd0(n - x, n * q);
    const T lf = (T)1.837877066409345483560659472811L + std::log(x) + std::log1p(-x / n);
    return lc - (T)0.5L * lf;
}

// P[Bin(n, p) <= k]; q = 1 - p is passed in: the caller knows which of the two is exact
template <typename T>
YH_BINOM_HD inline double binom_cdf(double k, double n, double p, double q, const T* small, T cut) {
    if (k < 0) return 0.0;
    if (k >= n) return 1.0;
    if (p <= 0.0) return 1.0;
    if (q <= 0.0) return 0.0;  // (k < n)
    if ((k + 1.0) <= (n + 1.0) * p) {  // k below the mode: the lower tail, terms falling from i = k down
        const T l0 = log_pmf<T>(k, n, p, q, small);
        T t = 1, s = 1;
        for (double i = k; i > 0; i -= 1.0) {
            t *= ((T)i * q) / ((T)(n - i + 1.0) * p);
            s += t;
            if (t < s * cut) break;
        }
        return (double)std::exp(l0 + std::log(s));
    }
    // k + 1 at or above the mode: the upper tail, terms falling from i = k + 1 up
    const T l0 = log_pmf<T>(k + 1.0, n, p, q, small);
    T t = 1, s = 1;
    for (double i = k + 1.0; i < n; i += 1.0) {
        t *= ((T)(n - i) * p) / ((T)(i + 1.0) * q);
        s += t;
        if (t < s * cut) break;
    }
    return (double)((T)1 - std::exp(l0 + std::log(s)));
}

}  // namespace yh_binom
