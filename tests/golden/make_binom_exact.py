#!/usr/bin/env python3
"""Generate tests/golden/binom_exact.npz: exact binomial distribution functions P[Bin(n, p) <= k], rounded to float64.

    python tests/golden/make_binom_exact.py        (mpmath only; about a minute on 8 cores)

The reference of `yacht run`'s p-values (yh_hyp_test on the host, yh_presence_rows_device on the GPU) at sizes where
scipy is itself too inexact to serve (its binom.cdf is ~1e-10 off at n = 4e6).  Every value is the SHORTER tail summed
term by term from the exact log point probability (log-gamma in mpmath at DPS digits), P = tail or 1 - tail; the sum
stops once a bound on what is left falls below 1e-35 of it.  p is the double `ani ** ksize` (the libm pow of yh_hyp.cpp
and the presence launcher), taken exactly; q = 1 - p exactly.

The grid is the cross product of
    (ani, ksize)  (0.8, 51) (0.9, 51) (0.95, 31) (0.95, 21) (0.9995, 21), and (0.75, 2): p = 0.5625, 1 - p exact in double
    n             1 2 15 16 17 (end of the stirlerr table) 80 81 500 501 (series switches) 1000 13791 5e4 1e6 4e6 3e7
    k             0, 1, n - 1, the three integers around (n + 1) p - 1 (the lower / upper tail switch of yh_binom.h), and
                  round(n p + z sqrt(n p q)) for z in Z,
clamped to [0, n] and without repeats.  Arrays: ani, ksize, p, n, k, P (float64; 0 where the exact value underflows),
log10P (log10 of the exact value, finite also where P underflows).
"""
from __future__ import annotations

import math
import os
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "binom_exact.npz")
DPS = 45
PAIRS = ((0.8, 51), (0.9, 51), (0.95, 31), (0.95, 21), (0.9995, 21), (0.75, 2))
NS = (1, 2, 15, 16, 17, 80, 81, 500, 501, 1000, 13_791, 50_000, 1_000_000, 4_000_000, 30_000_000)
Z = (-38, -30, -20, -8, -3, -1, -0.3, 0.3, 1, 3, 8)


def ks_for(n: int, p: float) -> list:
    q = 1.0 - p
    b = math.floor((n + 1.0) * p - 1.0)  # (k + 1 <= (n + 1) p: the lower tail)
    ks = [0, 1, n - 1, b - 1, b, b + 1]
    sd = math.sqrt(n * p * q)
    ks += [math.floor(n * p + z * sd + 0.5) for z in Z]
    return sorted({min(max(int(k), 0), n) for k in ks})


def grid() -> list:
    """(ani, ksize, p, n, k) of every case."""
    out = []
    for ani, ksize in PAIRS:
        p = ani ** ksize
        for n in NS:
            out += [(ani, ksize, p, n, k) for k in ks_for(n, p)]
    return out


def exact_cdf(k: int, n: int, p: float):
    """P[Bin(n, p) <= k] as an mpmath number of DPS digits (p the double, exactly)."""
    import mpmath as mp

    with mp.workdps(DPS):
        if k < 0:
            return mp.mpf(0)
        if k >= n:
            return mp.mpf(1)
        P, Q = mp.mpf(p), 1 - mp.mpf(p)
        lp, lq, lgn = mp.log(P), mp.log(Q), mp.loggamma(n + 1)

        def log_pmf(x):
            return lgn - mp.loggamma(x + 1) - mp.loggamma(n - x + 1) + x * lp + (n - x) * lq

        eps = mp.mpf(10) ** -35
        lower = k < n * p  # the shorter tail: below k when k is below the mean, above it otherwise
        i = k if lower else k + 1
        t = s = mp.mpf(1)  # terms relative to the first one
        while True:
            if lower:
                if i == 0:
                    break
                r = (i * Q) / ((n - i + 1) * P)  # pmf(i - 1) / pmf(i)
                i -= 1
            else:
                if i == n:
                    break
                r = ((n - i) * P) / ((i + 1) * Q)  # pmf(i + 1) / pmf(i)
                i += 1
            t *= r
            s += t
            # further ratios are smaller (the pmf is log-concave): what is left is below t r / (1 - r)
            if r < 1 and t * r / (1 - r) < eps * s:
                break
        tail = mp.exp(log_pmf(k if lower else k + 1)) * s
        return tail if lower else 1 - tail


def _case(c):
    import mpmath as mp

    ani, ksize, p, n, k = c
    v = exact_cdf(k, n, p)
    with mp.workdps(DPS):
        return float(v), float(mp.log10(v)) if v > 0 else -math.inf


def main() -> None:
    import mpmath

    cases = grid()
    big_first = sorted(cases, key=lambda c: -c[3])
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        got = dict(zip(big_first, pool.map(_case, big_first, chunksize=1)))
    arrays = dict(ani=np.array([c[0] for c in cases]), ksize=np.array([c[1] for c in cases], np.int64),
                  p=np.array([c[2] for c in cases]), n=np.array([c[3] for c in cases], np.int64),
                  k=np.array([c[4] for c in cases], np.int64), P=np.array([got[c][0] for c in cases]),
                  log10P=np.array([got[c][1] for c in cases]), dps=np.int64(DPS), mpmath=np.array(mpmath.__version__))
    np.savez_compressed(OUT, **arrays)
    print(f"{OUT}: {len(cases)} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
