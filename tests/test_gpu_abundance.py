"""RefDB.abundance / yh_abund_device on the GPU: the kernel set against a brute-force numpy oracle (tests/abund_oracle.py),
exact equality of all three outputs, over the lookup forms the library has (compact buckets behind the presence filter,
compact buckets alone, the five-entry buckets of small databases, one reference), the edge cases, the statement the pass
rests on (all abundances 1: the sums are run_counts' overlap and n_match), and the entry's place among the other calls."""
import numpy as np
import pytest
from abund_oracle import abundance_oracle

from yacht_amd import _lib, synth
from yacht_amd.engine import RefDB, YH_DB_NO_DIRECTORY, YH_DB_NO_INDEX, YachtHipError

pytestmark = pytest.mark.gpu

NARROW = 2 ** 22  # "scaled" whose hash range (2^42) lets a database of ~10^4 distinct hashes take the COMPACT buckets


def _check(db, values, offsets, sample, abund, what):
    w_ov, w_m, med = db.abundance(sample, abund)
    want = abundance_oracle(values, offsets, sample, abund)
    assert w_ov.dtype == np.uint64 and w_m.dtype == np.uint64 and med.dtype == np.float64
    assert np.array_equal(w_ov, want[0]), (what, "w_overlap")
    assert np.array_equal(w_m, want[1]), (what, "w_match")
    assert np.array_equal(med, want[2]), (what, "med_match")
    return w_ov, w_m, med


@pytest.fixture(scope="module")
def independent():
    """config2-style independent references in a narrow hash range: > 2^20 distinct hashes, so compact buckets + filter."""
    rng = np.random.default_rng(501)
    refs = synth.independent_refs(rng, 400, 5000, 0.35, 500, 20000, scaled=NARROW)
    values, offsets = synth.pack(refs)
    return rng, refs, values, offsets


@pytest.mark.parametrize("n_sample", [120_000, 300_000, 600_000])  # the three tile shapes of the lookup
def test_independent_references_against_the_oracle(hip_lib, independent, n_sample):
    rng, refs, values, offsets = independent
    present = rng.choice(len(refs), size=50, replace=False)
    sample = synth.sample_from_refs(rng, refs, present, 0.3, n_sample, scaled=NARROW)
    abund = rng.integers(1, 1001, sample.size)
    assert sample.size >= 100_000
    with RefDB(values, offsets) as db:
        assert db.info()["filter_bytes"] > 0  # (the presence filter exists only in front of compact buckets)
        w_ov, w_m, med = _check(db, values, offsets, sample, abund, f"independent {n_sample}")
        assert int((w_m > 0).sum()) >= 50 and np.all(med[w_m > 0] >= 1.0)


@pytest.mark.parametrize("size,n_sample", [(20_000, 150_000), (20_000, 700_000)])
def test_clustered_references_against_the_oracle(hip_lib, size, n_sample):
    """Cluster members share most hashes (the posting walk); the sample is one cluster member whole plus a little of the
    others, so one reference takes most of the hits (the LDS table's contended slot)."""
    rng = np.random.default_rng(502)
    refs = synth.clustered_refs(rng, 30, (1, 0.9, 0.5, 0.25, 0.1), size, scaled=NARROW)
    values, offsets = synth.pack(refs)
    cov = np.full(len(refs), 0.02)
    cov[4] = 1.0  # the member with the most private hashes: shared AND single-holder hits on one reference
    sample = synth.sample_from_refs(rng, refs, list(range(len(refs))), cov, n_sample, scaled=NARROW)
    abund = rng.integers(1, 1001, sample.size)
    with RefDB(values, offsets) as db:
        assert db.info()["n_shared_distinct"] > 10_000
        w_ov, w_m, med = _check(db, values, offsets, sample, abund, "clustered")
        assert int(np.argmax(w_ov)) == 4 and w_ov[4] > 10 * np.median(w_ov) and w_m[4] > 0 and w_ov[0] > w_m[0]


def test_small_database_with_the_five_entry_buckets(hip_lib):
    """At scaled = 1000 the hash range is 2^54: below ~10^7 distinct hashes a bucket would span more than 2^32 values, so
    the database keeps the full-hash buckets and their directory (YhDirView::find, find_slow for the overflowing ones)."""
    values, offsets, sample = synth.config2(seed=503, n_refs=150, n_sample=200_000)
    rng = np.random.default_rng(503)
    abund = rng.integers(1, 1001, sample.size)
    with RefDB(values, offsets) as db:
        assert db.info()["filter_bytes"] == 0
        _check(db, values, offsets, sample, abund, "five-entry buckets")
        # ... and a tiny one
        few = [np.array([5, 9, 11], np.uint64), np.array([9, 20], np.uint64), np.array([1, 2, 3], np.uint64)]
    v, o = synth.pack(few)
    with RefDB(v, o) as db:
        w_ov, w_m, med = _check(db, v, o, np.array([2, 5, 9, 20, 77], np.uint64), np.array([7, 3, 10, 4, 1]), "tiny")
        assert w_ov.tolist() == [13, 14, 7] and w_m.tolist() == [3, 4, 7] and med.tolist() == [3.0, 4.0, 7.0]


def test_one_reference(hip_lib):
    rng = np.random.default_rng(504)
    ref = synth.random_sketch(rng, 4000, synth.max_hash_for_scaled(1000))
    values, offsets = synth.pack([ref])
    sample = np.union1d(ref[::3], synth.random_sketch(rng, 5000, synth.max_hash_for_scaled(1000)))
    abund = rng.integers(1, 1001, sample.size)
    with RefDB(values, offsets) as db:
        w_ov, w_m, med = _check(db, values, offsets, sample, abund, "one reference")
        assert w_ov[0] == w_m[0] > 0


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(505)
    refs = synth.clustered_refs(rng, 8, (1, 0.6, 0.2), 3000, scaled=NARROW) + synth.independent_refs(rng, 40, 3000, 0.3, 500, 8000, scaled=NARROW)
    values, offsets = synth.pack(refs)
    return rng, refs, values, offsets


def test_edge_cases(hip_lib, small):
    rng, refs, values, offsets = small
    n = len(refs)
    mh = synth.max_hash_for_scaled(NARROW)
    with RefDB(values, offsets) as db:
        # an empty sample
        w_ov, w_m, med = db.abundance(np.zeros(0, np.uint64), np.zeros(0, np.int64))
        assert not w_ov.any() and not w_m.any() and not med.any() and w_ov.size == n
        # a sample with no hit (also: hashes above the database's largest)
        miss = np.setdiff1d(np.unique(rng.integers(0, 2 * mh, 50_000, dtype=np.uint64)), values)
        w_ov, w_m, med = _check(db, values, offsets, miss, rng.integers(1, 1001, miss.size), "no hit")
        assert not w_ov.any() and not med.any()
        # abundances all 2**32 - 1: the sums leave the 32-bit range
        sample = synth.sample_from_refs(rng, refs, [0, 1, 30, 31], 0.9, 20_000, scaled=NARROW)
        w_ov, w_m, med = _check(db, values, offsets, sample, np.full(sample.size, 2 ** 32 - 1, dtype=np.uint64), "all ones bits")
        assert int(w_ov.max()) > 2 ** 40 and np.all(med[w_m > 0] == float(2 ** 32 - 1))
        # exactly one and exactly two exclusive hits: both median cases
        _, single = np.unique(values, return_counts=True)
        only = np.unique(values)[single == 1]
        r40 = only[np.isin(only, refs[40])][:1]
        r41 = only[np.isin(only, refs[41])][:2]
        assert r40.size == 1 and r41.size == 2
        sample = np.union1d(np.concatenate([r40, r41]), miss[:1000])
        abund = np.ones(sample.size, dtype=np.int64)
        abund[sample == r40[0]] = 9
        abund[sample == r41[0]] = 4
        abund[sample == r41[1]] = 7
        w_ov, w_m, med = _check(db, values, offsets, sample, abund, "one and two hits")
        assert (w_m[40], med[40]) == (9, 9.0) and (w_m[41], med[41]) == (11, 5.5) and int((w_m > 0).sum()) == 2


def test_all_ones_give_the_run_counts(hip_lib, small, independent):
    """What the pass rests on: a sample hash is exclusive to a reference of the run subset exactly when that reference is
    its only holder in the database -- with every abundance 1 the two sums are run_counts' overlap and n_match."""
    for rng, refs, values, offsets in (small, independent):
        present = rng.choice(len(refs), size=20, replace=False)
        sample = synth.sample_from_refs(rng, refs, present, 0.5, 60_000, scaled=NARROW)
        with RefDB(values, offsets) as db:
            overlap, _n_excl, n_match = db.run_counts(sample)
            w_ov, w_m, med = db.abundance(sample, np.ones(sample.size, dtype=np.int64))
            assert np.array_equal(w_ov, overlap.astype(np.uint64)) and np.array_equal(w_m, n_match.astype(np.uint64))
            assert n_match.any() and np.array_equal(med, (n_match > 0).astype(np.float64))


def test_device_form_scratch_reuse_and_pipelined_neighbours(hip_lib, independent):
    import torch

    rng, refs, values, offsets = independent
    dev = torch.device("cuda:0")
    n = len(refs)

    def up(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).to(dev)

    samples = [synth.sample_from_refs(rng, refs, rng.choice(n, size=30, replace=False), 0.4, k, scaled=NARROW)
               for k in (600_000, 40_000, 580_000, 610_000)]
    abunds = [rng.integers(1, 1001, s.size).astype(np.uint32) for s in samples]
    with RefDB(values, offsets) as db:
        want = [db.abundance(s, a) for s, a in zip(samples, abunds)]  # (the host form: against the oracle above)
        assert np.array_equal(want[1][0], abundance_oracle(values, offsets, samples[1], abunds[1])[0])
        d_s = [up(s, np.int64) for s in samples]
        d_a = [up(a, np.int32) for a in abunds]
        out = [(torch.full((n,), -1, dtype=torch.int64, device=dev), torch.full((n,), -1, dtype=torch.int64, device=dev),
                torch.full((n,), -1.0, dtype=torch.float64, device=dev)) for _ in samples]
        torch.cuda.synchronize()
        # device form == host form; a second call with another sample size (scratch reuse); d_med_match = NULL
        for k in (0, 1):
            db.abundance_device(d_s[k].data_ptr(), d_a[k].data_ptr(), samples[k].size, out[k][0].data_ptr(), out[k][1].data_ptr(),
                                out[k][2].data_ptr())
        db.abundance_device(d_s[2].data_ptr(), d_a[2].data_ptr(), samples[2].size, out[2][0].data_ptr(), out[2][1].data_ptr(), 0)
        db.synchronize()
        for k in (0, 1, 2):
            assert np.array_equal(out[k][0].cpu().numpy().view(np.uint64), want[k][0]), k
            assert np.array_equal(out[k][1].cpu().numpy().view(np.uint64), want[k][1]), k
        assert np.array_equal(out[0][2].cpu().numpy(), want[0][2]) and np.array_equal(out[1][2].cpu().numpy(), want[1][2])
        assert bool((out[2][2] == -1.0).all())  # no median asked for: the array is not touched
        # between pipelined steps: their results stay what run_counts gives, and the abundance call is right too
        big = [0, 2, 3]
        counts = [[torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3)] for _ in big]
        for i, k in enumerate(big):
            db.run_device_pipelined(d_s[k].data_ptr(), samples[k].size, *(c.data_ptr() for c in counts[i]))
            if i == 1:
                db.abundance_device(d_s[3].data_ptr(), d_a[3].data_ptr(), samples[3].size, out[3][0].data_ptr(), out[3][1].data_ptr(),
                                    out[3][2].data_ptr())
        db.run_device_join()
        db.synchronize()
        got = [[c.cpu().numpy().view(np.uint32) for c in cs] for cs in counts]
        for i, k in enumerate(big):
            for g, w in zip(got[i], db.run_counts(samples[k])):
                assert np.array_equal(g, w), ("pipelined step", i)
        for j in range(3):
            w = want[3][j]
            g = out[3][j].cpu().numpy()
            assert np.array_equal(g.view(np.uint64) if j < 2 else g, w), ("between pipelined steps", j)


def test_unsupported_handles_and_unsorted_samples(hip_lib, small):
    _rng, _refs, values, offsets = small
    sample = np.array([3, 5, 8], np.uint64)
    for flags in (YH_DB_NO_DIRECTORY, YH_DB_NO_INDEX):
        with RefDB(values, offsets, flags=flags) as db:
            with pytest.raises(YachtHipError) as ei:
                db.abundance(sample, [1, 1, 1])
            assert ei.value.code == _lib.YH_ERR_UNSUPPORTED
    with RefDB(values, offsets) as db:
        with pytest.raises(YachtHipError) as ei:
            db.abundance(np.array([3, 8, 5], np.uint64), [1, 1, 1])
        assert ei.value.code == _lib.YH_ERR_UNSORTED
