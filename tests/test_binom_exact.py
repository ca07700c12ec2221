"""yh_hyp_test (host C++) against exact values: its p-value against P[Bin(n, p) <= k] from mpmath (tests/golden/binom_exact.npz,
made by tests/golden/make_binom_exact.py) at n up to 3e7, where scipy is itself ~1e-9 off, and its per-n table -- what a cohort
run reads its thresholds from -- at every n up to 200 000 against scipy's binom.ppf.  Needs no GPU."""
import importlib.util
import os

import numpy as np
import pytest

from yacht_amd.hypothesis_recovery_src import hyp_test_batch, hyp_test_native

GOLD = os.path.join(os.path.dirname(__file__), "golden")
REL = 1e-15      # p_val against the exact value, wherever that is >= TINY (worst 2.2e-16: one rounding)
TINY = 1e-300    # below: the exact value is (nearly) out of double's range, and p_val must be in [0, 1e-290]
TABLE_REL = 1e-12  # confidence and alt. mutation rate of the table against scipy (tests/test_hyp_native.py)
TABLE_N = 200_000
TABLE_SETS = ((31, 0.99, 0.95), (31, 0.95, 0.95), (51, 0.95, 0.95), (21, 0.9, 0.9995), (51, 0.9, 0.9), (31, 0.999, 0.95))


def exact():
    z = np.load(os.path.join(GOLD, "binom_exact.npz"))
    return {k: z[k] for k in z.files}


def maker():
    spec = importlib.util.spec_from_file_location("make_binom_exact", os.path.join(GOLD, "make_binom_exact.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def pairs(z):
    return sorted(set(zip(z["ani"].tolist(), z["ksize"].tolist())))


def test_fixture_is_the_grid_and_exact():
    """The fixture holds the generator's grid, p is the libm `ani ** ksize`, and a handful of its rows come out of mpmath
    again: one per (ani, ksize) at n = 3e7 next to the tail switch, one that underflows, and random ones."""
    z, m = exact(), maker()
    rows = list(zip(z["ani"].tolist(), z["ksize"].tolist(), z["p"].tolist(), z["n"].tolist(), z["k"].tolist()))
    assert rows == m.grid()
    assert all(ani ** ks == p for ani, ks, p, _, _ in rows)
    assert np.all((z["P"] >= 0) & (z["P"] <= 1))
    big = z["n"] == max(m.NS)
    assert {(a, k) for a, k in zip(z["ani"][big].tolist(), z["ksize"][big].tolist())} == set(m.PAIRS)
    pick = []
    for ani, ks in m.PAIRS:
        sel = np.flatnonzero(big & (z["ani"] == ani) & (z["ksize"] == ks))
        switch = np.floor((z["n"][sel] + 1.0) * z["p"][sel] - 1.0)
        pick.append(int(sel[np.argmin(np.abs(z["k"][sel] - switch))]))
    pick.append(int(np.flatnonzero(z["P"] < TINY)[0]))
    pick += np.random.default_rng(3).choice(z["P"].size, 12, replace=False).tolist()
    for i in pick:
        v = m.exact_cdf(int(z["k"][i]), int(z["n"][i]), float(z["p"][i]))
        assert float(v) == z["P"][i], (i, z["n"][i], z["k"][i])


def test_grid_reaches_the_large_sizes_and_both_tails():
    z = exact()
    big = z["n"] >= 1_000_000
    lower = z["k"] + 1.0 <= (z["n"] + 1.0) * z["p"]
    normal = z["P"] >= TINY
    assert (big & lower & normal).sum() >= 40 and (big & ~lower & normal).sum() >= 40
    assert (z["P"] < TINY).sum() >= 20 and (z["P"] == 0).any()
    assert set(z["n"].tolist()) >= {1, 2, 15, 16, 17, 80, 81, 500, 501, 30_000_000}


def test_host_p_value_against_exact():
    z = exact()
    worst = 0.0
    for ani, ks in pairs(z):
        w = (z["ani"] == ani) & (z["ksize"] == ks)
        n, k, P = z["n"][w], z["k"][w], z["P"][w]
        got = hyp_test_native(n, k, ks, 0.99, ani, 1.0)
        assert np.array_equal(got[3], n)  # (n_cov = n at coverage 1)
        pv = got[1]
        assert np.isfinite(pv).all(), (ani, ks, n[~np.isfinite(pv)], k[~np.isfinite(pv)])
        normal = P >= TINY
        rel = np.abs(pv[normal] - P[normal]) / P[normal]
        bad = rel > REL
        assert not bad.any(), (ani, ks, n[normal][bad][:4], k[normal][bad][:4], rel[bad][:4])
        assert np.all((pv[~normal] >= 0) & (pv[~normal] <= 1e-290)), (ani, ks, n[~normal], k[~normal], pv[~normal])
        worst = max(worst, float(rel.max()))
    print(f"yh_hyp_test p_val: worst relative error {worst:.3g} where P >= {TINY:g}")


@pytest.mark.parametrize("ksize,sig,ani", TABLE_SETS)
def test_threshold_table_equals_scipy(ksize, sig, ani):
    """The cohort's table (yh_hyp_test over n = 0..max reference size, n_match = 0) at every n up to 200 000: thresholds
    equal to scipy's binom.ppf (the single-sample path's), confidence and alt. mutation rate within 1e-12 of scipy's."""
    n = np.arange(TABLE_N + 1)
    zero = np.zeros(n.size, np.int64)
    got = hyp_test_native(n, zero, ksize, sig, ani, 1.0)
    want = hyp_test_batch(n, zero, ksize, sig, ani, 1.0)
    diff = np.flatnonzero(got[5] != want[5])
    assert diff.size == 0, (diff[:5], got[5][diff[:5]], want[5][diff[:5]])
    for col, name in ((6, "confidence"), (7, "alt. mutation rate")):
        g, w = got[col], want[col]
        ok = (np.abs(g - w) <= TABLE_REL * np.abs(w)) | ((np.abs(g) < 1e-250) & (np.abs(w) < 1e-250))
        assert ok.all(), (name, n[~ok][:5], g[~ok][:5], w[~ok][:5])
