// yh_binom.h — the binomial distribution function of `yacht run`'s presence test, once, for the host and the device.
//
// Loader's saddle-point point probabilities (C. Loader, "Fast and accurate computation of binomial probabilities", 2000:
// log pmf from Stirling-series errors and the deviance terms) and P[Bin(n, p) <= k] as the SHORTER tail summed outward
// from k by the exact term ratio.  Templated on the floating type T of the point probability and the tail sum:
// yh_hyp.cpp instantiates it with long double (host), yh_presence.hip with double (device).  `small` is the table
// stirlerr(0..15), which the caller computes once (yh_binom_stirlerr_table); `cut` ends a tail sum once a term falls
// below cut times the sum.
//
// 1 - p comes in as a double q and its rounding error q_lo (one_minus): a relative error d in n q moves log P by about
// |x - n p| d, which grows like sqrt(n) (2e-11 at n = 3e7 with q rounded to double).  In long double q + q_lo is 1 - p
// exactly (for p >= 2^-11).  In double, x - n p and n - x - n q come from the exact products (fma, so that no contraction
// of the compiler can count a rounding twice), the direct form of bd0 corrects for the roundings of n p and n q, and the
// tail sum for that of q.  Against exact values (n <= 3e7): 2.2e-16 relative in long double (tests/test_binom_exact.py),
// 2.5e-13 in double on the MI355X, 3.2e-14 where P >= 1e-15 (tests/test_gpu_presence_exact.py).
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

// x log(x / M) + M - x for M = m + m_lo (m_lo the rounding error of m), given d = x - M, without cancellation near x = M:
// the series in v = d / (x + M) for |v| < 0.5 (at most ~30 terms), the direct form beyond.  (Loader's 0.1 leaves the
// direct form a cancellation of up to ~20x at |v| = 0.1 .. 0.5, 1e-12 of log P in double at n = 1e6.)
template <typename T>
YH_BINOM_HD inline T bd0(T x, T m, T m_lo, T d) {
    if (std::fabs(d) < (T)0.5L * (x + m)) {
        T v = d / (x + m);
        T s = d * v;
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
    return x * (std::log(x / m) - m_lo / m) - d;
}

// q = 1 - p rounded to double; returns its rounding error q_lo, so that q + q_lo = 1 - p exactly (Fast2Sum of 1 and -p)
YH_BINOM_HD inline double one_minus(double p, double* q_lo) {
    const double q = 1.0 - p;
    *q_lo = -p - (q - 1.0);
    return q;
}

// qd + q_lo in T: exact in long double (for p >= 2^-11), qd in double; *r = the part of it that the result misses
template <typename T>
YH_BINOM_HD inline T q_in(double qd, double q_lo, T* r) {
    const T q = (T)qd + (T)q_lo;
    *r = (T)q_lo - (q - (T)qd);
    return q;
}

// log P[Bin(n, p) = x], 0 <= x <= n, qd + q_lo = 1 - p (q_lo = 0 when qd is the exact one, p only rounded)
template <typename T>
YH_BINOM_HD inline T log_pmf(double xd, double nd, double pd, double qd, double q_lo, const T* small) {
    const T x = xd, n = nd, p = pd;
    T q_r;
    const T q = q_in(qd, q_lo, &q_r);
    if (p <= (T)0) return x == 0 ? (T)0 : (T)-INFINITY;
    if (q <= (T)0) return x == n ? (T)0 : (T)-INFINITY;
    if (x == 0) return n * (p < (T)0.5L ? std::log1p(-p) : std::log(q) + q_r / q);  // (whichever of p, q is the small one)
    if (x == n) return n * (q < (T)0.5L ? std::log1p(-q) - q_r / p : std::log(p));
    // n p and n (q + q_r) as value + rounding error, and x - n p, n - x - n (q + q_r) from the exact products
    const T np = n * p, nq = n * q;
    const T np_lo = std::fma(n, p, -np), nq_lo = std::fma(n, q, -nq) + n * q_r;
    const T dp = std::fma(-n, p, x), dq = std::fma(-n, q, n - x) - n * q_r;
    const T lc = stirlerr(n, small) - stirlerr(x, small) - stirlerr(n - x, small) - bd0(x, np, np_lo, dp) - bd0(n - x, nq, nq_lo, dq);
    const T lf = (T)1.837877066409345483560659472811L + std::log(x) + std::log1p(-x / n);
    return lc - (T)0.5L * lf;
}

// P[Bin(n, p) <= k]; q + q_lo = 1 - p is passed in (one_minus when p is exact; q exact and q_lo = 0 when it is q)
template <typename T>
YH_BINOM_HD inline double binom_cdf(double k, double n, double p, double q, double q_lo, const T* small, T cut) {
    if (k < 0) return 0.0;
    if (k >= n) return 1.0;
    if (p <= 0.0) return 1.0;
    if (q <= 0.0) return 0.0;  // (k < n)
    // Term j of a tail holds j factors of qt or 1 / qt in place of 1 - p = qt (1 + c): the sum adds c sum(j t_j) (lower
    // tail) or subtracts it (upper), the first-order correction (0 in long double, up to ~2e-13 of P at n = 3e7 in double).
    T q_r;
    const T qt = q_in(q, q_lo, &q_r), c = q_r / qt;
    if ((k + 1.0) <= (n + 1.0) * p) {  // k below the mode: the lower tail, terms falling from i = k down
        const T l0 = log_pmf<T>(k, n, p, q, q_lo, small);
        T t = 1, s = 1, sj = 0;
        for (double i = k; i > 0; i -= 1.0) {
            t *= ((T)i * qt) / ((T)(n - i + 1.0) * p);
            s += t;
            sj += (T)(k - i + 1.0) * t;
            if (t < s * cut) break;
        }
        return (double)std::exp(l0 + std::log(s + c * sj));
    }
    // k + 1 at or above the mode: the upper tail, terms falling from i = k + 1 up
    const T l0 = log_pmf<T>(k + 1.0, n, p, q, q_lo, small);
    T t = 1, s = 1, sj = 0;
    for (double i = k + 1.0; i < n; i += 1.0) {
        t *= ((T)(n - i) * p) / ((T)(i + 1.0) * qt);
        s += t;
        sj += (T)(i - k) * t;
        if (t < s * cut) break;
    }
    return (double)((T)1 - std::exp(l0 + std::log(s - c * sj)));
}

}  // namespace yh_binom
