"""RefDB.explain_batch / yh_explain_batch_device / yh_explain_members_rows_device on the GPU: exact equality of every flag
and every one of the B x 16 totals with the brute-force oracle (tests/explain_oracle.py) run PER SAMPLE with that sample's
own member row.

A block's samples are random subsets of one pool of hashes of its database (many hits, some noise), of sizes chosen
around the kernel's tile T = YH_EXPLAIN_BATCH_TILE: 0, 1, T - 1, T, T + 1, 2 T + 1, a few thousand, empty samples first, in
the middle and last, two samples with the same hashes.  Every sample has its own seven_sets member row (seeded per
sample), so a kernel that reads another sample's row or adds into another sample's totals fails.  On the `big` database
the oracle's own classes must show, summed over each block, at least 100 hashes per mixed bit in each class a kernel can get
wrong.  The oracles are computed once per module."""
import ctypes as C

import numpy as np
import pytest
from explain_oracle import classes, explain_oracle, totals_from_flags
from test_gpu_explain import MIXED, NARROW, seven_sets

from yacht_amd import _lib, synth
from yacht_amd.engine import RefDB, YH_DB_NO_DIRECTORY, YH_DB_NO_INDEX, YachtHipError

pytestmark = pytest.mark.gpu

T = _lib.YH_EXPLAIN_BATCH_TILE
EDGE_SIZES = [0, 1, T - 1, T, T + 1, 2 * T + 1, 3000]


def _sizes(rng, n_samples):
    """Sample sizes of a block: the edge sizes first (an empty sample FIRST), an empty one in the middle and last (from three
    samples up), small random sizes for the rest."""
    sizes = (EDGE_SIZES + [int(x) for x in rng.integers(40, 700, max(0, n_samples - len(EDGE_SIZES)))])[:n_samples]
    if n_samples == 1:
        sizes = [2 * T + 1]
    elif n_samples == 2:
        sizes = [T + 1, 3000]
    else:
        sizes[n_samples // 2] = 0
        sizes[-1] = 0
    return sizes


def _block(seed, pool, n_refs, sizes, twin=None):
    """(samples, members [B, n_refs], abunds) of a block: subsets of the pool, a member row per sample seeded per sample;
    twin = (i, j): sample j takes sample i's hashes (and keeps its own member row)."""
    rng = np.random.default_rng(seed)
    samples = [np.sort(rng.choice(pool, size=k, replace=False)) for k in sizes]
    if twin is not None:
        samples[twin[1]] = samples[twin[0]].copy()
    members = np.stack([seven_sets(np.random.default_rng(1000 * seed + s), n_refs) for s in range(len(sizes))])
    abunds = [rng.integers(1, 1001, s.size).astype(np.uint32) for s in samples]
    return samples, members, abunds


def _oracle_block(values, offsets, samples, members):
    return [explain_oracle(values, offsets, s, m)[0] for s, m in zip(samples, members)]


def _assert_block_classes(values, offsets, samples, members):
    """Summed over the block's samples, every mixed bit has >= 100 hashes in each of the four classes (the oracle alone).
    The sums only grow with every sample: the walk over the block stops where all of them have reached 100."""
    total = {b: np.zeros(4, dtype=np.int64) for b in MIXED}
    for s, m in zip(samples, members):
        if s.size:
            for b, got in classes(values, offsets, s, m, MIXED).items():
                total[b] += got
        if min(int(total[b].min()) for b in MIXED) >= 100:
            return
    raise AssertionError({b: total[b].tolist() for b in MIXED})


def _check(db, samples, members, abunds, want, what):
    """The host form with abundances, without, with a mix, and totals only, all against the oracle's flags."""
    mixed = [a if s % 2 else None for s, a in enumerate(abunds)]
    for ab in (abunds, None, mixed):
        flags, totals = db.explain_batch(samples, members, ab)
        assert totals.dtype == np.uint64 and totals.shape == (len(samples), 8, 2) and len(flags) == len(samples)
        for s in range(len(samples)):
            assert flags[s].dtype == np.uint8 and np.array_equal(flags[s], want[s]), (what, "flags", s, np.flatnonzero(flags[s] != want[s])[:10])
            assert np.array_equal(totals[s], totals_from_flags(want[s], None if ab is None else ab[s])), (what, "totals", s)
        none, only = db.explain_batch(samples, members, ab, want_flags=False)  # d_flags = NULL
        assert none is None and np.array_equal(only, totals), (what, "totals only")


# ---- the databases, their pools, the blocks and the oracle's answers: made once, on the CPU ------------------------------------
@pytest.fixture(scope="module")
def big():
    """test_gpu_explain.py's `big` recipe (compact buckets behind the filter, > 2^20 distinct hashes, clusters), a pool in
    which every reference is present at coverage 0.04 and the cluster members at 0.3, and its blocks."""
    rng = np.random.default_rng(601)
    refs = synth.independent_refs(rng, 300, 5000, 0.35, 500, 20000, scaled=NARROW) + \
        synth.clustered_refs(rng, 12, (1, 0.9, 0.5, 0.25, 0.1), 5000, scaled=NARROW)
    order = rng.permutation(len(refs))
    refs = [refs[i] for i in order]
    values, offsets = synth.pack(refs)
    cov = np.full(len(refs), 0.04)
    cov[order >= 300] = 0.3
    pool = synth.sample_from_refs(rng, refs, list(range(len(refs))), cov, 200_000, scaled=NARROW)
    blocks = {}
    for n in (1, 2, 65):
        samples, members, abunds = _block(700 + n, pool, len(refs), _sizes(rng, n), twin=(6, 9) if n > 9 else None)
        _assert_block_classes(values, offsets, samples, members)
        blocks[n] = (samples, members, abunds, _oracle_block(values, offsets, samples, members))
    return values, offsets, len(refs), pool, blocks


@pytest.fixture(scope="module")
def clustered():
    rng = np.random.default_rng(602)
    refs = synth.clustered_refs(rng, 16, (1, 0.9, 0.5, 0.25, 0.1), 4000, scaled=NARROW)
    values, offsets = synth.pack(refs)
    pool = synth.sample_from_refs(rng, refs, list(range(len(refs))), 0.1, 45_000, scaled=NARROW)
    blocks = {}
    for n in (63, 64):
        samples, members, abunds = _block(800 + n, pool, len(refs), _sizes(rng, n), twin=(3, 8))
        blocks[n] = (samples, members, abunds, _oracle_block(values, offsets, samples, members))
    return values, offsets, len(refs), pool, blocks


@pytest.fixture(scope="module")
def five_entry():
    """synth.config2 at scaled = 1000 keeps the full-hash (five-entry) buckets; clusters appended for shared hashes."""
    values, offsets, sample = synth.config2(seed=603, n_refs=60, n_sample=40_000)
    rng = np.random.default_rng(603)
    refs = [values[int(offsets[i]):int(offsets[i + 1])] for i in range(len(offsets) - 1)] + \
        synth.clustered_refs(rng, 6, (1, 0.9, 0.5, 0.25, 0.1), 4000)
    values, offsets = synth.pack(refs)
    pool = np.union1d(sample, synth.sample_from_refs(rng, refs, list(range(len(refs))), 0.05, 1000))
    pool = np.union1d(pool, synth.random_sketch(rng, 30_000, synth.max_hash_for_scaled(1000)))  # hashes nobody holds
    blocks = {}
    for n in (1, 2, 63, 65):
        samples, members, abunds = _block(900 + n, pool, len(refs), _sizes(rng, n), twin=(3, 8) if n > 9 else None)
        blocks[n] = (samples, members, abunds, _oracle_block(values, offsets, samples, members))
    return values, offsets, len(refs), pool, blocks


@pytest.mark.parametrize("n_samples", [1, 2, 65])
def test_compact_buckets_and_filter_against_the_oracle(hip_lib, big, n_samples):
    values, offsets, n_refs, _pool, blocks = big
    samples, members, abunds, want = blocks[n_samples]
    with RefDB(values, offsets) as db:
        assert db.info()["filter_bytes"] > 0 and db.info()["n_shared_distinct"] > 1000
        _check(db, samples, members, abunds, want, f"big {n_samples}")
    if n_samples == 65:  # the twins: the same hashes, another member row, other flags
        assert np.array_equal(samples[6], samples[9]) and not np.array_equal(want[6], want[9])


@pytest.mark.parametrize("n_samples", [63, 64])
def test_clustered_references_walk_the_posting_lists(hip_lib, clustered, n_samples):
    values, offsets, n_refs, _pool, blocks = clustered
    samples, members, abunds, want = blocks[n_samples]
    known = sum(int(((w & 0x80) != 0).sum()) for w in want)
    assert 5000 < known < sum(s.size for s in samples) - 1000  # hits and misses
    with RefDB(values, offsets) as db:
        assert db.info()["n_shared_distinct"] > 10_000
        _check(db, samples, members, abunds, want, f"clustered {n_samples}")


@pytest.mark.parametrize("n_samples", [1, 2, 63, 65])
def test_small_database_with_the_five_entry_buckets(hip_lib, five_entry, n_samples):
    values, offsets, n_refs, _pool, blocks = five_entry
    samples, members, abunds, want = blocks[n_samples]
    with RefDB(values, offsets) as db:
        assert db.info()["filter_bytes"] == 0
        _check(db, samples, members, abunds, want, f"five-entry {n_samples}")


def test_one_reference(hip_lib):
    rng = np.random.default_rng(604)
    ref = synth.random_sketch(rng, 4000, synth.max_hash_for_scaled(1000))
    values, offsets = synth.pack([ref])
    pool = np.union1d(ref[::2], synth.random_sketch(rng, 3000, synth.max_hash_for_scaled(1000)))
    sizes = [0, T + 1, 1, 700, 0]
    samples = [np.sort(rng.choice(pool, size=k, replace=False)) for k in sizes]
    members = np.array([[2], [0], [0x7F], [2], [5]], np.uint8)
    abunds = [rng.integers(1, 1001, s.size).astype(np.uint32) for s in samples]
    want = _oracle_block(values, offsets, samples, members)
    assert set(want[1].tolist()) == {0, 0x80} and set(want[3].tolist()) == {0, 0x82}
    with RefDB(values, offsets) as db:
        _check(db, samples, members, abunds, want, "one reference")


def test_full_block_of_256_samples(hip_lib, big):
    """256 samples: RefDB.explain per sample (test_gpu_explain.py pins it to the oracle), and the oracle itself on eight."""
    values, offsets, n_refs, pool, _blocks = big
    rng = np.random.default_rng(611)
    sizes = _sizes(rng, 256)
    samples, members, abunds = _block(611, pool, n_refs, sizes, twin=(6, 200))
    picked = [1, 2, 5, 6, 100, 200, 254, 255]
    _assert_block_classes(values, offsets, [samples[s] for s in picked], members[picked])
    with RefDB(values, offsets) as db:
        flags, totals = db.explain_batch(samples, members, abunds)
        for s in range(256):
            f, t = db.explain(samples[s], members[s], abunds[s])
            assert np.array_equal(flags[s], f) and np.array_equal(totals[s], t), s
        for s in picked:
            want = explain_oracle(values, offsets, samples[s], members[s])[0]
            assert np.array_equal(flags[s], want) and np.array_equal(totals[s], totals_from_flags(want, abunds[s])), s
        assert not np.array_equal(flags[6], flags[200])  # the twins
        plain = db.explain_batch(samples, members, want_flags=False)[1]
        assert np.array_equal(plain[:, :, 0], totals[:, :, 0]) and np.array_equal(plain[:, :, 1], plain[:, :, 0])


def test_only_empty_samples_and_an_empty_database(hip_lib, five_entry):
    values, offsets, n_refs, _pool, _blocks = five_entry
    empty = [np.zeros(0, np.uint64)] * 5
    members = np.full((5, n_refs), 0x7F, np.uint8)
    with RefDB(values, offsets) as db:
        for ab in (None, [np.zeros(0, np.uint32)] * 5):
            flags, totals = db.explain_batch(empty, members, ab)
            assert all(f.size == 0 for f in flags) and totals.shape == (5, 8, 2) and not totals.any()
    with RefDB(np.zeros(0, np.uint64), np.zeros(3, np.uint64)) as db:  # two references without a hash
        flags, totals = db.explain_batch([np.array([3, 5], np.uint64), np.array([4], np.uint64)], np.zeros((2, 2), np.uint8), [[4, 4], [9]])
        assert [f.tolist() for f in flags] == [[0, 0], [0]] and not totals.any()


def test_abundances_whose_sums_pass_32_bits(hip_lib, big):
    values, offsets, n_refs, _pool, blocks = big
    samples, members, abunds, want = blocks[65]
    abunds = list(abunds)
    abunds[5] = np.full(samples[5].size, 2 ** 32 - 1, dtype=np.uint64)  # the sample of 2 T + 1 hashes
    abunds[3] = np.where(np.arange(samples[3].size) % 2 == 0, 2 ** 32 - 1, 2 ** 32 - 2).astype(np.uint64)
    with RefDB(values, offsets) as db:
        _flags, totals = db.explain_batch(samples, members, abunds)
    for s in range(65):
        assert np.array_equal(totals[s], totals_from_flags(want[s], abunds[s])), s
    assert int(totals[5, 7, 1]) == int(totals[5, 7, 0]) * (2 ** 32 - 1) > 2 ** 40 and int(totals[3, 7, 1]) > 2 ** 40


def _up(torch, a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).to("cuda:0")


def _device_block(torch, samples, members, abunds):
    offs = np.zeros(len(samples) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([s.size for s in samples])
    return (_up(torch, np.concatenate(samples), np.int64), _up(torch, offs, np.int64), _up(torch, np.concatenate(abunds), np.int32),
            _up(torch, members, np.uint8), offs)


def test_device_form_leaves_nothing_stale_and_masks_bit_7(hip_lib, big):
    """Two calls in a row on the same output buffers, the second block smaller; member bytes with bit 7 set; d_flags = NULL."""
    import torch

    values, offsets, n_refs, _pool, blocks = big
    first, second = blocks[65], blocks[2]
    with RefDB(values, offsets) as db:
        d_flags = torch.full((int(sum(s.size for s in first[0])) + 64,), 0x55, dtype=torch.uint8, device="cuda:0")
        d_tot = torch.full((65 + 1, 16), -1, dtype=torch.int64, device="cuda:0")
        for samples, members, abunds, want in (first, second):
            d_s, d_o, d_a, d_m, offs = _device_block(torch, samples, members | np.uint8(0x80), abunds)
            total = int(offs[-1])
            db.explain_batch_device(d_s.data_ptr(), d_o.data_ptr(), d_a.data_ptr(), len(samples), total, d_m.data_ptr(),
                                    d_flags.data_ptr(), d_tot.data_ptr())
            db.synchronize()
            flags, tot = d_flags.cpu().numpy(), d_tot.cpu().numpy().view(np.uint64).reshape(-1, 8, 2)
            for s in range(len(samples)):
                assert np.array_equal(flags[offs[s]:offs[s + 1]], want[s]), s
                assert np.array_equal(tot[s], totals_from_flags(want[s], abunds[s])), s
            assert (flags[-64:] == 0x55).all() and (d_tot[65].cpu().numpy() == -1).all()  # nothing behind the outputs
        # d_flags = NULL and d_abund = NULL: the totals alone, the flags array untouched
        d_flags.fill_(0x55)
        db.explain_batch_device(d_s.data_ptr(), d_o.data_ptr(), 0, 2, total, d_m.data_ptr(), 0, d_tot.data_ptr())
        db.synchronize()
        tot = d_tot.cpu().numpy().view(np.uint64).reshape(-1, 8, 2)
        assert all(np.array_equal(tot[s], totals_from_flags(second[3][s])) for s in range(2)) and bool((d_flags == 0x55).all())
        # a block of only empty samples on buffers that hold the last block's totals
        db.explain_batch_device(d_s.data_ptr(), torch.zeros(4, dtype=torch.int64, device="cuda:0").data_ptr(), 0, 3, 0, d_m.data_ptr(),
                                d_flags.data_ptr(), d_tot.data_ptr())
        db.synchronize()
        assert not d_tot[:3].cpu().numpy().any() and bool((d_flags == 0x55).all())


def test_errors(hip_lib, five_entry):
    import torch

    values, offsets, n_refs, _pool, blocks = five_entry
    samples, members, abunds, _want = blocks[2]
    for flags in (YH_DB_NO_DIRECTORY, YH_DB_NO_INDEX):
        with RefDB(values, offsets, flags=flags) as db:
            with pytest.raises(YachtHipError) as ei:
                db.explain_batch(samples, members)
            assert ei.value.code == _lib.YH_ERR_UNSUPPORTED
    with RefDB(values, offsets) as db:
        with pytest.raises(YachtHipError) as ei:
            db.explain_batch([samples[0], np.array([3, 8, 5], np.uint64)], members)
        assert ei.value.code == _lib.YH_ERR_UNSORTED
        # 257 samples and a member byte with bit 7 set, past the binding's own checks
        p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        offs = np.zeros(258, dtype=np.uint64)
        many = np.zeros((257, n_refs), np.uint8)
        totals = np.zeros((257, 16), np.uint64)
        assert db._lib.yh_explain_batch(db._h, None, p(offs), None, 257, p(many), None, p(totals)) == _lib.YH_ERR_INVALID_ARG
        assert db._lib.yh_explain_batch(db._h, None, p(offs), None, 0, p(many), None, p(totals)) == _lib.YH_ERR_INVALID_ARG
        bad = members.copy()
        bad[1, 5] |= np.uint8(0x80)
        cat, offs2 = np.concatenate(samples), np.array([0, samples[0].size, samples[0].size + samples[1].size], np.uint64)
        assert db._lib.yh_explain_batch(db._h, p(cat), p(offs2), None, 2, p(bad), None, p(totals)) == _lib.YH_ERR_INVALID_ARG
        assert b"bit 7" in db._lib.yh_last_error()
        d = torch.zeros(4096, dtype=torch.int64, device="cuda:0")
        for n in (0, 257):
            with pytest.raises(YachtHipError) as ei:
                db.explain_batch_device(d.data_ptr(), d.data_ptr(), 0, n, 0, d.data_ptr(), 0, d.data_ptr())
            assert ei.value.code == _lib.YH_ERR_INVALID_ARG
        for n_sets, n_smp in ((0, 1), (8, 1), (7, 0), (7, 257)):
            with pytest.raises(YachtHipError) as ei:
                db.explain_members_rows_device(d.data_ptr(), d.data_ptr(), 4, d.data_ptr(), n_sets, n_smp, d.data_ptr())
            assert ei.value.code == _lib.YH_ERR_INVALID_ARG


def test_between_the_batch_counts_and_their_compact_rows(hip_lib, big):
    """explain_batch_device queued between yh_run_batch_device and yh_run_batch_rows_pack_device: the rows equal those of a run
    without it, and the explain results are right."""
    import torch

    values, offsets, n_refs, _pool, blocks = big
    samples, members, abunds, want = blocks[65]
    d_s, d_o, d_a, d_m, offs = _device_block(torch, samples, members, abunds)
    total, b, cap = int(offs[-1]), len(samples), 65 * n_refs
    with RefDB(values, offsets) as db:
        d_flags = torch.full((total,), 0x55, dtype=torch.uint8, device="cuda:0")
        d_tot = torch.full((b, 16), -1, dtype=torch.int64, device="cuda:0")
        rows = []
        for with_explain in (False, True):
            c = torch.zeros((3, b, n_refs), dtype=torch.int32, device="cuda:0")
            vals = torch.zeros((cap, 3), dtype=torch.int32, device="cuda:0")
            out = torch.zeros((cap, 5), dtype=torch.int32, device="cuda:0")
            n_rows = torch.zeros(2, dtype=torch.int32, device="cuda:0")
            db.run_batch_device(d_s.data_ptr(), d_o.data_ptr(), b, total, c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr())
            if with_explain:
                db.explain_batch_device(d_s.data_ptr(), d_o.data_ptr(), d_a.data_ptr(), b, total, d_m.data_ptr(), d_flags.data_ptr(),
                                        d_tot.data_ptr())
            db.run_batch_rows_pack_device(c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr(), vals.data_ptr(), cap, n_rows[0].data_ptr())
            db.run_batch_rows_unpack_device(vals.data_ptr(), cap, out.data_ptr(), n_rows[1].data_ptr())
            db.synchronize()
            torch.cuda.synchronize()
            k = int(n_rows[1])
            rows.append((k, out[:k].cpu().numpy(), c.cpu().numpy()))
        assert rows[0][0] == rows[1][0] > 0 and np.array_equal(rows[0][1], rows[1][1]) and np.array_equal(rows[0][2], rows[1][2])
        assert np.array_equal(rows[1][2][0, 5].view(np.uint32), db.run_counts(samples[5])[0])
        flags, tot = d_flags.cpu().numpy(), d_tot.cpu().numpy().view(np.uint64).reshape(b, 8, 2)
        for s in range(b):
            assert np.array_equal(flags[offs[s]:offs[s + 1]], want[s]) and np.array_equal(tot[s], totals_from_flags(want[s], abunds[s])), s


# ---- the member rows from compact rows --------------------------------------------------------------------------------------------
def _members_numpy(rows, n_rows, cap, present, n_sets, n_samples, n_refs):
    want = np.zeros((n_samples, n_refs), np.uint8)
    for k in range(min(n_rows, cap)):
        s, r = int(rows[k, 0]), int(rows[k, 1])
        if s < n_samples and r < n_refs:
            want[s, r] = sum(int(present[c, k] != 0) << c for c in range(n_sets))
    return want


def test_member_rows_against_a_numpy_scatter(hip_lib, five_entry):
    import torch

    values, offsets, n_refs, _pool, _blocks = five_entry
    rng = np.random.default_rng(620)
    cap, guard = 600, 64
    # hand-written corners first, then random distinct (sample, reference) pairs; row 7 is out of range and skipped
    pairs = [(0, 0), (0, n_refs - 1), (255, 0), (255, n_refs - 1), (1, 1), (254, n_refs - 2), (128, n_refs // 2), (256, 3), (3, n_refs)]
    seen = set(pairs)
    while len(pairs) < cap + 50:
        pr = (int(rng.integers(0, 256)), int(rng.integers(0, n_refs)))
        if pr not in seen:
            seen.add(pr)
            pairs.append(pr)
    rows = np.zeros((cap + 50, 5), np.uint32)
    rows[:, :2] = pairs
    rows[:, 2:] = rng.integers(1, 1000, (cap + 50, 3))
    present = rng.integers(0, 2, (9, cap)).astype(np.uint8) * rng.integers(1, 256, (9, cap)).astype(np.uint8)  # any non-zero byte counts
    present[:, 0] = 1
    d_rows = _up(torch, rows[:cap], np.int32)
    d_present = _up(torch, present, np.uint8)
    d_n = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    with RefDB(values, offsets) as db:
        def run(n_rows, c0, n_sets, n_samples):
            d_members = torch.full((n_samples * n_refs + guard,), 0xEE, dtype=torch.uint8, device="cuda:0")
            d_n.fill_(n_rows)
            db.explain_members_rows_device(d_rows.data_ptr(), d_n.data_ptr(), cap, d_present[c0].data_ptr(), n_sets, n_samples,
                                           d_members.data_ptr())
            db.synchronize()
            got = d_members.cpu().numpy()
            assert (got[n_samples * n_refs:] == 0xEE).all(), "guard bytes"
            want = _members_numpy(rows, n_rows, cap, present[c0:c0 + n_sets], n_sets, n_samples, n_refs)
            assert np.array_equal(got[:n_samples * n_refs].reshape(n_samples, n_refs), want), (n_rows, c0, n_sets, n_samples)
            return want

        full = run(cap, 0, 7, 256)  # seven planes, samples 0 and 255, references 0 and N - 1
        assert full[0, 0] == 0x7F and full[255, n_refs - 1] == _members_numpy(rows, cap, cap, present[:7], 7, 256, n_refs)[255, n_refs - 1]
        assert int((full != 0).sum()) > 400 and full.max() <= 0x7F
        run(cap, 7, 2, 256)        # the second pass of nine coverages: planes 7 and 8
        run(cap, 2, 1, 256)
        assert not run(0, 0, 7, 256).any()           # *d_n_rows = 0: the dirty table comes back all zero
        run(cap + 50, 0, 7, 256)                     # *d_n_rows > cap_rows: only the first cap_rows count
        run(300, 0, 7, 256)
        part = run(cap, 0, 7, 100)                   # rows of samples >= n_samples are skipped
        assert int((part != 0).sum()) < int((full != 0).sum())
