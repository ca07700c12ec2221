"""The presence kernel (yh_presence_rows_device, yh_presence.hip) on the GPU: its p-values against exact values
(tests/golden/binom_exact.npz: P[Bin(n, p) <= k] from mpmath, n up to 3e7), and its edges row by row against yh_hyp_test
(host): rows past one grid-stride, a row count above and below the capacity, 16 and 17 coverages, the last table entry and
the one past it, n_match at and past n_cov, coverage 0 and truncated coverages."""
import os

import numpy as np
import pytest

from yacht_amd import _lib, cohort, synth
from yacht_amd.engine import RefDB
from yacht_amd.hypothesis_recovery_src import hyp_test_native

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TINY = 1e-300     # exact values below: p_val in [0, 1e-290]
REL = 5e-13       # p_val against the exact value where it is >= TINY (MI355X: worst 2.5e-13)
MID = 1e-15
REL_MID = 6e-14   # ... and where it is >= MID (MI355X: worst 3.2e-14)
HOST_REL, HOST_TINY = 1e-12, 1e-250  # p_val against yh_hyp_test (tests/test_hyp_native.py)
SENT_P, SENT_PRES, SENT_NCOV = -7.0, 7, -559038737  # (0xdeadbeef)
SIG = 0.99


@pytest.fixture(scope="module")
def db(hip_lib):
    values, offsets = synth.pack([np.arange(1, 5, dtype=np.uint64)])  # (the kernel reads no handle state)
    with RefDB(values, offsets) as h:
        yield h


def table(n_max, ksize, ani):
    """The cohort's threshold table over n = 0..n_max."""
    return hyp_test_native(np.arange(n_max + 1), np.zeros(n_max + 1, np.int64), ksize, SIG, ani, 1.0)[5]


def launch(db, e, m, covs, ksize, ani, thr, cap=None, n_rows=None, pad=0):
    """cohort._Device.presence on rows (sample 0, ref i, -, e_i, m_i), *d_n_rows = n_rows, cap_rows = cap.  The outputs are
    [n_covs][cap] views of buffers with `pad` more entries, all filled with sentinels first; rows past e (up to max(cap,
    n_rows)) are valid ones, so that a kernel reading them would write.  Returns p_val, present, n_cov and the pads."""
    import torch

    e, m = np.asarray(e, np.int64), np.asarray(m, np.int64)
    cap = e.size if cap is None else cap
    n_rows = e.size if n_rows is None else n_rows
    dev = cohort._Device(db, covs, ksize, ani, thr)
    nc = dev.covs.size
    nbuf = max(e.size, cap, n_rows)
    rows = np.zeros((nbuf, 5), np.uint32)
    rows[:, 1] = np.arange(nbuf)
    rows[:, 3], rows[:, 4] = 7, 1
    rows[:e.size, 3], rows[:e.size, 4] = e, m
    d_rows = torch.from_numpy(rows.view(np.int32)).to(dev.dev)
    d_n = torch.tensor([n_rows], dtype=torch.int32, device=dev.dev)
    size = nc * cap + pad
    flat = (torch.full((size,), SENT_P, dtype=torch.float64, device=dev.dev),
            torch.full((size,), SENT_PRES, dtype=torch.uint8, device=dev.dev),
            torch.full((size,), SENT_NCOV, dtype=torch.int32, device=dev.dev))
    dev.presence(d_rows, d_n.data_ptr(), cap, tuple(f[:nc * cap].view(nc, cap) for f in flat))
    db.synchronize()
    torch.cuda.synchronize()
    p, pres, ncov = (f.cpu().numpy() for f in flat)
    body = [a[:nc * cap].reshape(nc, cap) for a in (p, pres, ncov)]
    return body[0], body[1], body[2], (p[nc * cap:], pres[nc * cap:], ncov[nc * cap:])


def untouched(p, pres, ncov):
    return bool(np.all(p == SENT_P) and np.all(pres == SENT_PRES) and np.all(ncov == SENT_NCOV))


def close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    tiny = (np.abs(got) < HOST_TINY) & (np.abs(want) < HOST_TINY)
    return tiny | (np.abs(got - want) <= HOST_REL * np.abs(want))


def check_host(out, e, m, covs, ksize, ani, what):
    """Rows 0..len(e) of every coverage against yh_hyp_test: n_cov and present exactly, p_val to 1e-12."""
    pv, pres, ncov = out[:3]
    e, m = np.asarray(e, np.int64), np.asarray(m, np.int64)
    for c, cov in enumerate(covs):
        w = hyp_test_native(e, m, ksize, SIG, ani, cov)
        assert np.array_equal(ncov[c, :e.size].view(np.uint32), w[3]), (what, cov)
        assert np.array_equal(pres[c, :e.size].astype(bool), w[0]), (what, cov)
        ok = close(pv[c, :e.size], w[1])
        assert ok.all(), (what, cov, e[~ok][:3], m[~ok][:3], pv[c, :e.size][~ok][:3], w[1][~ok][:3])


def test_kernel_p_value_against_exact(db):
    z = np.load(os.path.join(GOLD, "binom_exact.npz"))
    worst, worst_mid = 0.0, 0.0
    for ani, ks in sorted(set(zip(z["ani"].tolist(), z["ksize"].tolist()))):
        w = (z["ani"] == ani) & (z["ksize"] == ks)
        n, k, P = z["n"][w], z["k"][w], z["P"][w]
        # the table at the n the rows read, NaN elsewhere (the full table up to 3e7 would take hours on the host)
        thr = np.full(int(n.max()) + 1, np.nan)
        un = np.unique(n)
        thr[un] = hyp_test_native(un, np.zeros(un.size, np.int64), ks, SIG, ani, 1.0)[5]
        pv, pres, ncov, _ = launch(db, n, k, [1.0], ks, ani, thr)
        pv, pres, ncov = pv[0], pres[0], ncov[0].view(np.uint32)
        want = hyp_test_native(n, k, ks, SIG, ani, 1.0)
        assert np.array_equal(ncov, n) and np.array_equal(pres.astype(bool), want[0]), (ani, ks)
        assert np.isfinite(pv).all(), (ani, ks, n[~np.isfinite(pv)], k[~np.isfinite(pv)])
        normal, mid = P >= TINY, P >= MID
        rel = np.zeros(P.size)
        rel[normal] = np.abs(pv[normal] - P[normal]) / P[normal]
        for sel, bound in ((normal, REL), (mid, REL_MID)):
            bad = sel & (rel > bound)
            assert not bad.any(), (ani, ks, bound, n[bad][:4], k[bad][:4], pv[bad][:4], P[bad][:4], rel[bad][:4])
        assert np.all((pv[~normal] >= 0) & (pv[~normal] <= 1e-290)), (ani, ks, n[~normal], k[~normal], pv[~normal])
        worst, worst_mid = max(worst, float(rel[normal].max())), max(worst_mid, float(rel[mid].max()))
    print(f"k_presence_rows p_val: worst relative error {worst:.3g} where P >= {TINY:g}, {worst_mid:.3g} where P >= {MID:g}")


def test_rows_past_one_grid_stride(db):
    """1 300 000 rows: the grid (4096 blocks of 256) covers 1 048 576, the rest takes a second pass of the loop."""
    rng = np.random.default_rng(5)
    n = 1_300_000
    assert n > 4096 * 256
    e = rng.integers(0, 3001, n)
    m = np.minimum(rng.binomial(e, 0.95 ** 31 * 1.02), e)
    m[::97] = rng.integers(0, 3001, m[::97].size)  # (some n_match past n_cov)
    covs = [1.0, 0.3]
    out = launch(db, e, m, covs, 31, 0.95, table(3000, 31, 0.95))
    check_host(out, e, m, covs, 31, 0.95, "1.3e6 rows")


@pytest.mark.parametrize("n_rows", [1500, 600])
def test_row_count_against_capacity(db, n_rows):
    """*d_n_rows above cap_rows: rows 0..cap, nothing past the [n_covs][cap] outputs; below: rows n_rows..cap of every
    coverage stay as they were."""
    rng = np.random.default_rng(n_rows)
    cap, covs = 1000, [1.0, 0.5, 0.05]
    e = rng.integers(0, 2001, max(cap, n_rows))
    m = np.minimum(rng.integers(0, 500, e.size), e)
    out = launch(db, e, m, covs, 31, 0.95, table(2000, 31, 0.95), cap=cap, n_rows=n_rows, pad=1024)
    lim = min(cap, n_rows)
    check_host(out, e[:lim], m[:lim], covs, 31, 0.95, f"n_rows {n_rows}")
    assert untouched(*out[3]), "written past the outputs"
    assert untouched(*(a[:, lim:] for a in out[:3])), "rows past *d_n_rows written"


@pytest.mark.parametrize("n_covs", [16, 17])
def test_many_coverages(db, n_covs):
    """16 coverages in one launch, 17 in two (cohort._Device.presence); 17 in one call is refused."""
    import ctypes as C

    covs = [1.0, 0.0, 0.7, 0.3, 0.1, 0.05, 0.01, 0.001, 0.999, 0.5, 0.25, 0.125, 0.9, 0.6, 0.4, 0.2, 0.15][:n_covs]
    rng = np.random.default_rng(n_covs)
    e = rng.integers(0, 4001, 3000)
    m = np.minimum(rng.integers(0, 900, e.size), e)
    out = launch(db, e, m, covs, 31, 0.95, table(4000, 31, 0.95), pad=64)
    check_host(out, e, m, covs, 31, 0.95, f"{n_covs} coverages")
    assert untouched(*out[3])
    if n_covs == 17:  # (real buffers of 17 coverages: the call is refused before it uses them)
        import torch

        lib = _lib.load()
        cv = np.asarray(covs, np.float64)
        d = torch.zeros(64, dtype=torch.float64, device="cuda")
        ptr = C.c_void_p(d.data_ptr())
        with pytest.raises(_lib.YachtHipError):
            _lib.check(lib.yh_presence_rows_device(db._h, ptr, ptr, 1, 31, 0.95, cv.ctypes.data_as(C.c_void_p), 17, ptr, 10, ptr, ptr, ptr))


def test_table_end_and_n_match_edges(db):
    """n_cov = n_max (the table's last entry) and n_max + 1 (p_val NaN, present 0); n_match 0, at n_cov and past it."""
    n_max = 1000
    thr = table(n_max, 31, 0.95)
    t = int(thr[n_max])
    e = np.array([n_max] * 6 + [n_max + 1] * 3 + [0, 0, 1, 1, 2, 37, 37, 37, 999])
    m = np.array([0, 1, t - 1, t, n_max, n_max + 1] + [0, t, n_max + 2] + [0, 5, 0, 1, 3, 0, 37, 38, 999])
    ok = e <= n_max
    pv, pres, ncov, pads = launch(db, e, m, [1.0], 31, 0.95, thr, pad=16)
    check_host((pv[:, ok], pres[:, ok], ncov[:, ok]), e[ok], m[ok], [1.0], 31, 0.95, "edges")
    assert np.all(np.isnan(pv[0, ~ok])) and np.all(pres[0, ~ok] == 0) and np.array_equal(ncov[0, ~ok], e[~ok])
    assert np.all(pv[0, ok & (m > e)] == 1.0) and np.all(pv[0, ok & (m == e)] == 1.0)
    assert pres[0, 2] == 0 and pres[0, 3] == 1 and untouched(*pads)
    # a row far past the table: n_excl 2^32 - 1
    pv, pres, ncov, _ = launch(db, np.array([2**32 - 1]), np.array([5]), [1.0], 31, 0.95, thr)
    assert np.isnan(pv[0, 0]) and pres[0, 0] == 0 and ncov[0, 0].view(np.uint32) == 2**32 - 1


def test_coverage_zero(db):
    e = np.array([0, 1, 10, 5000, 5000, 123])
    m = np.array([0, 0, 3, 0, 7, 123])
    pv, pres, ncov, _ = launch(db, e, m, [0.0], 31, 0.95, table(5000, 31, 0.95))
    assert np.all(ncov == 0) and np.all(pv == 1.0) and np.array_equal(pres[0].astype(bool), m != 0)
    check_host((pv, pres, ncov), e, m, [0.0], 31, 0.95, "coverage 0")


def test_truncated_coverages(db):
    """n_cov = int(n_excl * cov) at multiples of 10: the double product is an integer for 0.1 and 0.3, and for 0.7 falls
    just below one at 289 of these n_excl (90, 170, 180, ...), which truncation takes to the integer below."""
    e = np.arange(10, 20_001, 10)
    covs = [0.1, 0.3, 0.7]
    below = [sum(int(x * c) < round(x * c) for x in e.tolist()) for c in covs]
    assert below == [0, 0, 289], below
    m = e // 7
    pv, pres, ncov, _ = launch(db, e, m, covs, 31, 0.95, table(20_000, 31, 0.95))
    for c, cov in enumerate(covs):
        assert ncov[c].tolist() == [int(x * cov) for x in e.tolist()], cov
    check_host((pv, pres, ncov), e, m, covs, 31, 0.95, "truncation")
