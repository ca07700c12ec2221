"""RefDB.explain / yh_explain_device on the GPU: the kernel against a brute-force numpy oracle (tests/explain_oracle.py),
exact equality of every flag and all 16 totals, over the lookup forms the library has (compact buckets behind the presence
filter in the three tile shapes, the posting walk, the five-entry buckets of small databases, one reference), a
hand-written database whose flags are spelled out, a hash that 300 references hold, the edge cases, the cross-checks with
the existing entries, and the entry's place among the other calls.

Every database is asked with seven call sets at once: the empty set, all references, and five mixed ones of different
sizes.  For each MIXED set the oracle's own result must show at least 100 sample hashes (1 in the hand-written database)
in each class a kernel can get wrong -- not in the database, single holder inside the set, single holder outside it,
shared with holders on both sides -- so no class passes unseen.  The empty set and the set of all references cannot have
holders on both sides, and a database of ONE reference has no shared hash and no mixed set: there the classes that exist
are asserted (not in the database; single holder inside "all"; single holder outside "empty")."""
import ctypes as C

import numpy as np
import pytest
from explain_oracle import classes, explain_oracle, totals_from_flags

from yacht_amd import _lib, synth
from yacht_amd.engine import RefDB, YH_DB_NO_DIRECTORY, YH_DB_NO_INDEX, YachtHipError

pytestmark = pytest.mark.gpu

NARROW = 2 ** 22  # "scaled" whose hash range (2^42) lets a database of ~10^6 distinct hashes take the COMPACT buckets
MIXED = (2, 3, 4, 5, 6)  # the bits of the mixed call sets of seven_sets


def seven_sets(rng, n):
    """The member table of seven call sets over n references: bit 0 the empty set, bit 1 all references, bits 2..6 mixed:
    every other reference, and random subsets of a half, a quarter, three quarters and a tenth."""
    member = np.zeros(n, dtype=np.uint8)
    member |= np.uint8(1 << 1)
    member[::2] |= np.uint8(1 << 2)
    for bit, share in ((3, 0.5), (4, 0.25), (5, 0.75), (6, 0.1)):
        member[rng.choice(n, size=max(1, int(round(share * n))), replace=False)] |= np.uint8(1 << bit)
    return member


def _assert_classes(values, offsets, sample, member, at_least=100, bits=MIXED):
    for bit, got in classes(values, offsets, sample, member, bits).items():
        print("classes (not in db, single inside, single outside, shared on both sides) of bit", bit, got)
        assert min(got) >= at_least, (bit, got)


def _check(db, values, offsets, sample, member, abund, what, want_flags=None):
    """explain with and without abundances and totals-only, all against the oracle; returns (flags, totals with abund)."""
    if want_flags is None:
        want_flags = explain_oracle(values, offsets, sample, member)[0]
    for ab in (abund, None):
        flags, totals = db.explain(sample, member, ab)
        assert flags.dtype == np.uint8 and flags.shape == (len(sample),) and totals.dtype == np.uint64 and totals.shape == (8, 2)
        assert np.array_equal(flags, want_flags), (what, "flags", ab is None, np.flatnonzero(flags != want_flags)[:10])
        assert np.array_equal(totals, totals_from_flags(want_flags, ab)), (what, "totals", ab is None)
        none, only = db.explain(sample, member, ab, want_flags=False)  # d_flags = NULL
        assert none is None and np.array_equal(only, totals), (what, "totals only", ab is None)
    return db.explain(sample, member, abund)


@pytest.fixture(scope="module")
def big():
    """Independent references plus clusters in a narrow hash range: > 2^20 distinct hashes, so compact buckets + filter,
    single-holder hits (the independent ones) and shared ones (the clusters), interleaved so that the mixed sets cut
    through every cluster."""
    rng = np.random.default_rng(601)
    refs = synth.independent_refs(rng, 300, 5000, 0.35, 500, 20000, scaled=NARROW) + \
        synth.clustered_refs(rng, 12, (1, 0.9, 0.5, 0.25, 0.1), 5000, scaled=NARROW)
    order = rng.permutation(len(refs))
    refs = [refs[i] for i in order]
    values, offsets = synth.pack(refs)
    return rng, refs, values, offsets, seven_sets(rng, len(refs)), np.flatnonzero(order >= 300)


def _big_sample(rng, refs, clustered, n_sample):
    """Every cluster member and twenty other references at coverage 0.3, and noise up to n_sample hashes."""
    present = np.union1d(clustered, rng.choice(len(refs), size=20, replace=False))
    return synth.sample_from_refs(rng, refs, present, 0.3, n_sample, scaled=NARROW)


@pytest.mark.parametrize("n_sample", [120_000, 300_000, 600_000])  # the three tile shapes of the lookup
def test_compact_buckets_and_filter_against_the_oracle(hip_lib, big, n_sample):
    rng, refs, values, offsets, member, clustered = big
    sample = _big_sample(rng, refs, clustered, n_sample)
    lo = {120_000: 100_000, 300_000: 262_144, 600_000: 524_288}[n_sample]
    hi = {120_000: 262_144, 300_000: 524_288, 600_000: 1 << 40}[n_sample]
    assert lo <= sample.size < hi  # (the shape this case is for)
    abund = rng.integers(1, 1001, sample.size)
    _assert_classes(values, offsets, sample, member)
    with RefDB(values, offsets) as db:
        assert db.info()["filter_bytes"] > 0 and db.info()["n_shared_distinct"] > 1000
        flags, totals = _check(db, values, offsets, sample, member, abund, f"big {n_sample}")
        assert totals[0].tolist() == [0, 0] and np.array_equal(totals[1], totals[7])  # the empty set, all references


def test_sizes_around_the_tile_shape_switches(hip_lib, big):
    """n_sample one below, at and one above 262 144 and 524 288: prefixes of one sample (a hash's flag does not depend on
    the other hashes of the sample, so the oracle's flags of the whole sample hold for every prefix)."""
    rng, refs, values, offsets, member, clustered = big
    sample = _big_sample(rng, refs, clustered, 620_000)
    assert sample.size > 524_289
    abund = rng.integers(1, 1001, sample.size)
    want = explain_oracle(values, offsets, sample, member)[0]
    with RefDB(values, offsets) as db:
        for n in (262_143, 262_144, 262_145, 524_287, 524_288, 524_289):
            flags, totals = db.explain(sample[:n], member, abund[:n])
            assert np.array_equal(flags, want[:n]), n
            assert np.array_equal(totals, totals_from_flags(want[:n], abund[:n])), n
            assert np.array_equal(db.explain(sample[:n], member, want_flags=False)[1], totals_from_flags(want[:n])), n


def test_clustered_references_walk_the_posting_lists(hip_lib):
    rng = np.random.default_rng(602)
    refs = synth.clustered_refs(rng, 30, (1, 0.9, 0.5, 0.25, 0.1), 20_000, scaled=NARROW)
    values, offsets = synth.pack(refs)
    member = seven_sets(rng, len(refs))
    cov = np.full(len(refs), 0.02)
    cov[4] = 1.0
    sample = synth.sample_from_refs(rng, refs, list(range(len(refs))), cov, 150_000, scaled=NARROW)
    abund = rng.integers(1, 1001, sample.size)
    _assert_classes(values, offsets, sample, member)
    with RefDB(values, offsets) as db:
        assert db.info()["n_shared_distinct"] > 10_000
        _check(db, values, offsets, sample, member, abund, "clustered")


def test_small_database_with_the_five_entry_buckets(hip_lib):
    """synth.config2 at scaled = 1000 keeps the full-hash buckets and their directory (YhDirView::find, find_slow for the
    overflowing ones).  Its references are independent -- no two share a hash -- so clusters at the same scale are appended
    for the shared class."""
    values, offsets, sample = synth.config2(seed=603, n_refs=150, n_sample=200_000)
    rng = np.random.default_rng(603)
    refs = [values[int(offsets[i]):int(offsets[i + 1])] for i in range(len(offsets) - 1)]
    clusters = synth.clustered_refs(rng, 6, (1, 0.9, 0.5, 0.25, 0.1), 4000)
    refs = refs + clusters
    values, offsets = synth.pack(refs)
    extra = synth.sample_from_refs(rng, clusters, list(range(len(clusters))), 0.5, 1000)
    sample = np.union1d(sample, extra)
    member = seven_sets(rng, len(refs))
    abund = rng.integers(1, 1001, sample.size)
    _assert_classes(values, offsets, sample, member)
    with RefDB(values, offsets) as db:
        assert db.info()["filter_bytes"] == 0
        _check(db, values, offsets, sample, member, abund, "five-entry buckets")


def test_one_reference(hip_lib):
    rng = np.random.default_rng(604)
    ref = synth.random_sketch(rng, 4000, synth.max_hash_for_scaled(1000))
    values, offsets = synth.pack([ref])
    sample = np.union1d(ref[::3], synth.random_sketch(rng, 5000, synth.max_hash_for_scaled(1000)))
    abund = rng.integers(1, 1001, sample.size)
    for member, bit in ((np.array([0b0000010], np.uint8), 1), (np.array([0], np.uint8), 0)):
        not_in, inside, outside, shared = classes(values, offsets, sample, member, (bit,))[bit]
        assert not_in >= 100 and shared == 0 and (inside if bit else outside) >= 100 and (outside if bit else inside) == 0
        with RefDB(values, offsets) as db:
            flags, totals = _check(db, values, offsets, sample, member, abund, "one reference")
            assert set(flags.tolist()) == {0, 0x80 | int(member[0])} and totals[7, 0] == -(-ref.size // 3)


def test_hand_written_database(hip_lib):
    #        reference 0      1          2           3
    few = [np.array([5, 9, 11], np.uint64), np.array([9, 20, 30], np.uint64), np.array([1, 2, 3, 20], np.uint64), np.array([40], np.uint64)]
    v, o = synth.pack(few)
    member = np.array([0b001, 0b010, 0b100, 0b000], np.uint8)  # call set k = {reference k}; reference 3 is in none
    sample = np.array([2, 5, 7, 9, 20, 30, 40, 77], np.uint64)
    abund = np.array([7, 3, 100, 10, 4, 8, 6, 1])
    #        2: ref 2   5: ref 0   7: -   9: refs 0, 1   20: refs 1, 2   30: ref 1   40: ref 3   77: -
    expect = [0x84, 0x81, 0x00, 0x83, 0x86, 0x82, 0x80, 0x00]
    _assert_classes(v, o, sample, member, at_least=1, bits=(0, 1, 2))
    with RefDB(v, o) as db:
        flags, totals = _check(db, v, o, sample, member, abund, "hand written", want_flags=np.array(expect, np.uint8))
        assert flags.tolist() == expect
        assert totals.tolist() == [[2, 13], [3, 22], [2, 11], [0, 0], [0, 0], [0, 0], [0, 0], [6, 38]]
        plain = db.explain(sample, member)[1]
        assert plain[:, 0].tolist() == plain[:, 1].tolist() == [2, 3, 2, 0, 0, 0, 0, 6]


def test_a_hash_every_reference_holds(hip_lib):
    """300 references, each with private hashes, a block of hashes ALL of them hold (posting lists of 300 holders: 75
    rounds of the four-at-a-time walk), and hashes held by 2, 3, 5, 6 and 7 consecutive references (lists whose last round
    is partial)."""
    rng = np.random.default_rng(605)
    mh = synth.max_hash_for_scaled(NARROW)
    pool = synth.random_sketch(rng, 400_000, mh)
    rng.shuffle(pool)
    n = 300
    common, pool = pool[:300], pool[300:]
    refs = [[common] for _ in range(n)]
    for k in (2, 3, 5, 6, 7):
        for j in range(0, n - k, 3):
            block, pool = pool[:4], pool[4:]
            for i in range(k):
                refs[j + i].append(block)
    for j in range(n):
        private, pool = pool[:600], pool[600:]
        refs[j].append(private)
    refs = [np.unique(np.concatenate(r)) for r in refs]
    values, offsets = synth.pack(refs)
    member = seven_sets(rng, n)
    member[7] &= np.uint8(0b0000011)  # one reference that is in no mixed set ...
    member[8] |= np.uint8(0b1111100)  # ... and one that is in all of them
    sample = synth.sample_from_refs(rng, refs, list(range(n)), 0.5, 150_000, scaled=NARROW)
    sample = np.union1d(sample, common)
    abund = rng.integers(1, 1001, sample.size)
    _assert_classes(values, offsets, sample, member)
    with RefDB(values, offsets) as db:
        flags, totals = _check(db, values, offsets, sample, member, abund, "held by all")
        held_by_all = np.isin(sample, common)
        assert int(held_by_all.sum()) == 300 and (flags[held_by_all] == 0xFE).all()  # every set but the empty one


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(606)
    refs = synth.clustered_refs(rng, 8, (1, 0.6, 0.2), 3000, scaled=NARROW) + synth.independent_refs(rng, 104, 3000, 0.3, 500, 8000, scaled=NARROW)
    values, offsets = synth.pack(refs)
    return rng, refs, values, offsets, seven_sets(rng, len(refs))


def test_edge_cases(hip_lib, small):
    rng, refs, values, offsets, member = small
    mh = synth.max_hash_for_scaled(NARROW)
    with RefDB(values, offsets) as db:
        # an empty sample: zero totals, no flags
        flags, totals = db.explain(np.zeros(0, np.uint64), member, np.zeros(0, np.int64))
        assert flags.size == 0 and not totals.any()
        assert not db.explain(np.zeros(0, np.uint64), member)[1].any()
        # one hash: in the database, and not
        one = refs[0][:1]
        flags, totals = _check(db, values, offsets, one, member, np.array([9]), "one hash, held")
        assert flags[0] & 0x80 and totals[7].tolist() == [1, 9]
        gone = np.setdiff1d(np.arange(1, 50, dtype=np.uint64), values)[:1]
        flags, totals = _check(db, values, offsets, gone, member, np.array([9]), "one hash, not held")
        assert flags.tolist() == [0] and not totals.any()
        # no hit at all, half of the hashes above the database's largest hash
        miss = np.setdiff1d(np.unique(rng.integers(0, 2 * mh, 50_000, dtype=np.uint64)), values)
        assert int((miss > values.max()).sum()) > 10_000
        flags, totals = _check(db, values, offsets, miss, member, rng.integers(1, 1001, miss.size), "no hit")
        assert not flags.any() and not totals.any()
        # hashes above the largest hash of the database next to hits
        sample = np.union1d(synth.sample_from_refs(rng, refs, [0, 1, 30, 31], 0.9, 20_000, scaled=NARROW), miss[miss > values.max()][:5000])
        flags, totals = _check(db, values, offsets, sample, member, np.full(sample.size, 2 ** 32 - 1, dtype=np.uint64), "all ones bits")
        assert not flags[sample > values.max()].any() and int(totals[7, 1]) == int(totals[7, 0]) * (2 ** 32 - 1) > 2 ** 40
    # an empty database: zero totals, flags untouched
    with RefDB(np.zeros(0, np.uint64), np.zeros(3, np.uint64)) as db:
        flags, totals = db.explain(np.array([3, 5], np.uint64), np.zeros(2, np.uint8), [4, 4])
        assert flags.tolist() == [0, 0] and not totals.any()


def test_cross_checks_with_the_existing_entries(hip_lib, small):
    rng, refs, values, offsets, member = small
    sample = synth.sample_from_refs(rng, refs, rng.choice(len(refs), size=20, replace=False), 0.5, 60_000, scaled=NARROW)
    with RefDB(values, offsets) as db:
        overlap = db.run_counts(sample)[0]
        flags, totals = db.explain(sample, member)
        assert int(totals[7, 0]) == int(((flags & 0x80) != 0).sum()) > 0
        # call set 0 = the references that overlap the sample: every known hash is explained by it
        flags, totals = db.explain(sample, (overlap > 0).astype(np.uint8))
        assert np.array_equal((flags & 1) != 0, (flags & 0x80) != 0) and np.array_equal(totals[0], totals[7])
    # without shared hashes every known sample hash has one holder: their number is the sum of the overlaps
    indep = refs[24:]
    v, o = synth.pack(indep)
    sample = synth.sample_from_refs(rng, indep, rng.choice(len(indep), size=20, replace=False), 0.5, 60_000, scaled=NARROW)
    with RefDB(v, o) as db:
        assert db.info()["n_shared_distinct"] == 0
        flags, totals = db.explain(sample, np.zeros(len(indep), np.uint8))
        assert int(totals[7, 0]) == int(db.run_counts(sample)[0].sum()) == int((flags == 0x80).sum()) > 1000


def test_device_form_and_its_place_among_the_other_calls(hip_lib, big):
    import torch

    rng, refs, values, offsets, member, clustered = big
    dev = torch.device("cuda:0")
    n = len(refs)

    def up(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).to(dev)

    samples = [_big_sample(rng, refs, clustered, k) for k in (600_000, 40_000, 580_000, 610_000)]
    abunds = [rng.integers(1, 1001, s.size).astype(np.uint32) for s in samples]
    with RefDB(values, offsets) as db:
        want = [db.explain(s, member, a) for s, a in zip(samples, abunds)]  # (the host form: against the oracle above)
        assert np.array_equal(want[1][0], explain_oracle(values, offsets, samples[1], member)[0])
        d_s = [up(s, np.int64) for s in samples]
        d_a = [up(a, np.int32) for a in abunds]
        d_member = up(member | np.uint8(0x80), np.uint8)  # bit 7 set: the device form masks it off
        d_flags = [torch.full((s.size,), 0x55, dtype=torch.uint8, device=dev) for s in samples]
        d_tot = [torch.full((16,), -1, dtype=torch.int64, device=dev) for _ in samples]
        torch.cuda.synchronize()

        def explain(k, flags=True, abund=True):
            db.explain_device(d_s[k].data_ptr(), d_a[k].data_ptr() if abund else 0, samples[k].size, d_member.data_ptr(),
                              d_flags[k].data_ptr() if flags else 0, d_tot[k].data_ptr())

        def same(k, flags=True):
            assert np.array_equal(d_tot[k].cpu().numpy().view(np.uint64).reshape(8, 2), want[k][1]), k
            if flags:
                assert np.array_equal(d_flags[k].cpu().numpy(), want[k][0]), k

        # device form == host form; a second call with another sample size; d_flags = NULL leaves the array alone
        explain(0)
        explain(1)
        explain(2, flags=False)
        db.synchronize()
        same(0)
        same(1)
        same(2, flags=False)
        assert bool((d_flags[2] == 0x55).all())
        explain(1, abund=False)  # d_abund = NULL: every abundance is 1
        db.synchronize()
        got = d_tot[1].cpu().numpy().view(np.uint64).reshape(8, 2)
        assert np.array_equal(got[:, 0], want[1][1][:, 0]) and np.array_equal(got[:, 1], got[:, 0])
        # between pipelined steps: their results stay what run_counts gives, and the explain call is right too
        bigs = [0, 2, 3]
        counts = [[torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3)] for _ in bigs]
        for i, k in enumerate(bigs):
            db.run_device_pipelined(d_s[k].data_ptr(), samples[k].size, *(c.data_ptr() for c in counts[i]))
            if i == 1:
                explain(3)
        db.run_device_join()
        db.synchronize()
        for i, k in enumerate(bigs):
            for g, w in zip(counts[i], db.run_counts(samples[k])):
                assert np.array_equal(g.cpu().numpy().view(np.uint32), w), ("pipelined step", i)
        same(3)
        # inside an open batch slot: between the batch's counts and the compact rows made from the slot's state
        small = [s[:50_000] for s in samples[:3]]
        offs = np.zeros(4, dtype=np.int64)
        offs[1:] = np.cumsum([s.size for s in small])
        d_cat, d_offs = up(np.concatenate(small), np.int64), up(offs, np.int64)
        cap = 3 * n
        rows = []
        for with_explain in (False, True):
            c = torch.zeros((3, 3, n), dtype=torch.int32, device=dev)
            vals = torch.zeros((cap, 3), dtype=torch.int32, device=dev)
            out = torch.zeros((cap, 5), dtype=torch.int32, device=dev)
            n_rows = torch.zeros(2, dtype=torch.int32, device=dev)
            db.run_batch_device(d_cat.data_ptr(), d_offs.data_ptr(), 3, int(offs[-1]), c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr())
            if with_explain:
                d_flags[0].fill_(0x55)
                explain(0)
            db.run_batch_rows_pack_device(c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr(), vals.data_ptr(), cap, n_rows[0].data_ptr())
            db.run_batch_rows_unpack_device(vals.data_ptr(), cap, out.data_ptr(), n_rows[1].data_ptr())
            db.synchronize()
            torch.cuda.synchronize()
            k = int(n_rows[1])
            rows.append((k, out[:k].cpu().numpy(), c.cpu().numpy()))
        assert rows[0][0] == rows[1][0] > 0 and np.array_equal(rows[0][1], rows[1][1]) and np.array_equal(rows[0][2], rows[1][2])
        for s in range(3):
            assert np.array_equal(rows[1][2][0, s].view(np.uint32), db.run_counts(small[s])[0]), s
        same(0)


def test_unsupported_handles_and_bad_arguments(hip_lib, small):
    import torch

    _rng, refs, values, offsets, member = small
    sample = np.array([3, 5, 8], np.uint64)
    for flags in (YH_DB_NO_DIRECTORY, YH_DB_NO_INDEX):
        with RefDB(values, offsets, flags=flags) as db:
            with pytest.raises(YachtHipError) as ei:
                db.explain(sample, member)
            assert ei.value.code == _lib.YH_ERR_UNSUPPORTED
    with RefDB(values, offsets) as db:
        with pytest.raises(YachtHipError) as ei:
            db.explain(np.array([3, 8, 5], np.uint64), member)
        assert ei.value.code == _lib.YH_ERR_UNSORTED
        # a member byte with bit 7 set, past the binding's own check: the host form refuses it
        bad = member.copy()
        bad[5] |= np.uint8(0x80)
        flags, totals = np.zeros(3, np.uint8), np.zeros(16, np.uint64)
        p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        assert db._lib.yh_explain(db._h, p(sample), None, 3, p(bad), p(flags), p(totals)) == _lib.YH_ERR_INVALID_ARG
        assert b"bit 7" in db._lib.yh_last_error()
        assert len(refs) >= 128
        ghost_src = torch.zeros(4, dtype=torch.int32, device="cuda:0")
        db.set_ghosts(64, 4, ghost_src.data_ptr())
        with pytest.raises(YachtHipError) as ei:
            db.explain(sample, member)
        assert ei.value.code == _lib.YH_ERR_UNSUPPORTED
        d = torch.zeros(64, dtype=torch.int64, device="cuda:0")
        with pytest.raises(YachtHipError) as ei:
            db.explain_device(d.data_ptr(), 0, 3, d.data_ptr(), 0, d.data_ptr())
        assert ei.value.code == _lib.YH_ERR_UNSUPPORTED
