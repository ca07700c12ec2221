"""RefDB.gather / yh_gather_device on the GPU: exact equality of the rows, `more` and the owners against the oracles of
tests/gather_oracle.py, over the cases of tests/gather_cases.py (a hand-written database whose rows are spelled out, posting
lists either side of the four-at-a-time walk, the three tile shapes of the lookup, answers either side of a chunk of rounds),
one database per directory format, the stops and the edge cases, abundances that need the 64-bit sum, the cross-checks with
the existing entries, and the entry's place among the other calls.  Every check runs with and without abundances and with
and without the owner array."""
import ctypes as C

import numpy as np
import pytest
from gather_cases import BIG_SIZES, LIST_LENGTHS, NARROW, ROUNDS, assert_big_classes, big, big_sample, descending, hand_written, posting_lists
from gather_oracle import NOBODY, gather_oracle, gather_sets

import lookup_cases
from yacht_amd import _lib, engine, synth
from yacht_amd.engine import RefDB, YH_DB_NO_DIRECTORY, YH_DB_NO_INDEX, YachtHipError

pytestmark = pytest.mark.gpu


def _check(db, values, offsets, sample, cand, abund, what, oracle=gather_oracle, **stops):
    """gather with / without abundances and with / without owner, all four against the oracle; returns the rows with
    abundances."""
    out = None
    for ab in (abund, None):
        want_rows, want_more, want_owner = oracle(values, offsets, sample, cand, ab, **stops)
        for want_own in (True, False):
            rows, more, owner = db.gather(sample, cand, ab, want_owner=want_own, **stops)
            tag = (what, "abund" if ab is not None else "flat", "owner" if want_own else "no owner", stops)
            assert rows.dtype == engine.GATHER_ROW_DTYPE and rows.shape == want_rows.shape, (tag, len(rows), len(want_rows))
            assert np.array_equal(rows, want_rows), (tag, rows[:5], want_rows[:5])
            assert more is want_more, tag
            if want_own:
                assert owner.dtype == np.uint32 and owner.shape == (len(sample),)
                assert np.array_equal(owner, want_owner), (tag, np.flatnonzero(owner != want_owner)[:10])
            else:
                assert owner is None
        out = rows if out is None else out
    return out


def test_hand_written_database(hip_lib):
    values, offsets, sample, cand, abund, want_rows, want_owner = hand_written()
    with RefDB(values, offsets) as db:
        rows = _check(db, values, offsets, sample, cand, abund, "hand written", oracle=gather_sets)
        assert [(int(r["ref"]), int(r["n_overlap"]), int(r["n_unique"]), int(r["w_unique"])) for r in rows] == want_rows
        rows, more, owner = db.gather(sample, cand, abund, want_owner=True)
        assert owner.tolist() == want_owner and more is False
        flat = db.gather(sample, cand)[0]
        assert flat["w_unique"].tolist() == flat["n_unique"].tolist() == [5, 3, 3, 1]


@pytest.mark.parametrize("length", LIST_LENGTHS)
def test_posting_list_lengths(hip_lib, length):
    values, offsets, sample, cand, abund, groups = posting_lists(length)
    with RefDB(values, offsets) as db:
        _check(db, values, offsets, sample, cand, abund, f"lists of {length}")
        _check(db, values, offsets, sample, np.ones_like(cand), abund, f"lists of {length}, all candidates")
        _check(db, values, offsets, sample, cand, abund, f"lists of {length}, capped", cap_rows=2)


@pytest.mark.parametrize("n_sample", BIG_SIZES)  # the three tile shapes of the lookup
def test_the_three_tile_shapes(hip_lib, n_sample):
    refs, values, offsets, cand, present = big()
    sample, abund = big_sample(n_sample)
    stats = {}
    want = gather_oracle(values, offsets, sample, cand, abund, stats=stats)
    assert_big_classes(stats, want[0])
    with RefDB(values, offsets) as db:
        assert db.info()["filter_bytes"] > 0 and db.info()["n_shared_distinct"] > 1000
        rows = _check(db, values, offsets, sample, cand, abund, f"big {n_sample}")
        assert len(rows) > ROUNDS  # (more than one chunk of rounds)


def test_directory_formats_and_one_reference(hip_lib):
    # the compact bucket with exactly 8 entries, its overflow table, and the wide form of the same hashes
    for name in ("compact_edge", "wide_edge", "overflow_505"):
        case = lookup_cases.database(name)
        values, offsets = case.csr()
        sample = lookup_cases.samples(name)["base"]
        rng = np.random.default_rng(7300)
        cand = (rng.random(case.n_refs) < 0.6).astype(np.uint8)
        with RefDB(values, offsets) as db:
            rows = _check(db, values, offsets, sample, cand, rng.integers(1, 1001, sample.size), name)
            assert len(rows) >= 5
    rng = np.random.default_rng(7301)
    ref = synth.random_sketch(rng, 4000, synth.max_hash_for_scaled(1000))
    values, offsets = synth.pack([ref])
    sample = np.union1d(ref[::3], synth.random_sketch(rng, 5000, synth.max_hash_for_scaled(1000)))
    abund = rng.integers(1, 1001, sample.size)
    with RefDB(values, offsets) as db:
        rows = _check(db, values, offsets, sample, np.array([1], np.uint8), abund, "one reference")
        assert rows["ref"].tolist() == [0] and rows["n_unique"].tolist() == rows["n_overlap"].tolist() == [-(-ref.size // 3)]
        assert len(_check(db, values, offsets, sample, np.array([0], np.uint8), abund, "one reference, no candidate")) == 0


@pytest.mark.parametrize("n_rows", [ROUNDS - 1, ROUNDS, ROUNDS + 1, 2 * ROUNDS])
def test_answers_either_side_of_a_chunk_of_rounds(hip_lib, n_rows):
    assert ROUNDS == _lib.YH_GATHER_ROUNDS_PER_SYNC
    values, offsets, sample, cand, abund = descending(n_rows)
    with RefDB(values, offsets) as db:
        rows = _check(db, values, offsets, sample, cand, abund, f"{n_rows} rows")
        assert len(rows) == n_rows and rows["ref"].tolist() == list(range(n_rows))
        _check(db, values, offsets, sample, cand, abund, f"{n_rows} rows, capped at a chunk", cap_rows=ROUNDS)


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(7400)
    refs = synth.clustered_refs(rng, 8, (1, 0.6, 0.2), 3000, scaled=NARROW) + synth.independent_refs(rng, 104, 3000, 0.3, 500, 8000, scaled=NARROW)
    values, offsets = synth.pack(refs)
    present = np.concatenate([np.arange(24), rng.choice(np.arange(24, len(refs)), size=12, replace=False)])
    sample = synth.sample_from_refs(rng, refs, present, 0.4, 60_000, scaled=NARROW)
    cand = np.zeros(len(refs), np.uint8)
    cand[present[::2]] = 1
    cand[100:110] = 1
    return rng, refs, values, offsets, sample, cand, rng.integers(1, 1001, sample.size)


def test_stops(hip_lib, small):
    rng, refs, values, offsets, sample, cand, abund = small
    full = gather_oracle(values, offsets, sample, cand, abund)[0]
    assert len(full) >= 12
    mid = int(full["n_unique"][len(full) // 2])
    assert full["n_unique"][0] > mid > full["n_unique"][-1]  # (a min_hits whose stop falls mid-way)
    with RefDB(values, offsets) as db:
        rows = _check(db, values, offsets, sample, cand, abund, "min_hits", min_hits=mid + 1)
        assert 0 < len(rows) < len(full)
        assert len(_check(db, values, offsets, sample, cand, abund, "min_hits above all", min_hits=int(full["n_unique"][0]) + 1)) == 0
        for cap, more in ((len(full) - 3, True), (1, True), (len(full), False), (len(full) + 5, False), (0, True)):
            rows = _check(db, values, offsets, sample, cand, abund, "cap", cap_rows=cap)
            assert db.gather(sample, cand, abund, cap_rows=cap)[1] is more and len(rows) == min(cap, len(full))
        _check(db, values, offsets, sample, cand, abund, "cap and min_hits", cap_rows=len(full) - 3, min_hits=mid + 1)
        # cap_rows = 0 without an eligible candidate: more stays 0
        assert db.gather(sample, cand, abund, cap_rows=0, min_hits=int(full["n_unique"][0]) + 1)[1] is False


def test_edge_cases(hip_lib, small):
    rng, refs, values, offsets, sample, cand, abund = small
    empty = np.zeros(0, np.uint64)
    with RefDB(values, offsets) as db:
        rows, more, owner = db.gather(empty, cand, np.zeros(0, np.int64), want_owner=True)
        assert len(rows) == 0 and more is False and owner.size == 0
        assert len(db.gather(empty, cand)[0]) == 0
        assert len(_check(db, values, offsets, sample, np.zeros_like(cand), abund, "no candidate")) == 0
        one = refs[0][:1]
        only = np.zeros_like(cand)
        only[0] = 1
        rows = _check(db, values, offsets, one, only, np.array([9]), "one hash, held by a candidate")
        assert rows.tolist() == [(0, 1, 1, 0, 9)]
        # no hit at all, half of the hashes above the database's largest hash
        mh = synth.max_hash_for_scaled(NARROW)
        miss = np.setdiff1d(np.unique(rng.integers(0, 2 * mh, 50_000, dtype=np.uint64)), values)
        assert len(_check(db, values, offsets, miss, cand, rng.integers(1, 1001, miss.size), "no hit")) == 0
    # an empty database: no rows, nobody owns anything
    with RefDB(np.zeros(0, np.uint64), np.zeros(3, np.uint64)) as db:
        rows, more, owner = db.gather(np.array([3, 5], np.uint64), np.ones(2, np.uint8), [4, 4], want_owner=True)
        assert len(rows) == 0 and more is False and owner.tolist() == [NOBODY, NOBODY]
    with RefDB(np.zeros(0, np.uint64), np.zeros(1, np.uint64)) as db:
        assert len(db.gather(np.array([3, 5], np.uint64), np.zeros(0, np.uint8))[0]) == 0


def test_large_abundances_need_the_64_bit_sum(hip_lib, small):
    rng, refs, values, offsets, sample, cand, abund = small
    # 3 000 hashes of the first cluster's parent, shared ones among them, and a second cluster for another row
    assert refs[0].size >= 2990
    take = np.union1d(refs[0], refs[3][:500])
    ab = np.full(take.size, 2 ** 32 - 1, dtype=np.uint64)
    only = np.zeros_like(cand)
    only[[0, 1, 3]] = 1
    with RefDB(values, offsets) as db:
        rows = _check(db, values, offsets, take, only, ab, "all ones bits")
        assert int(rows["ref"][0]) == 0 and int(rows["n_unique"][0]) == refs[0].size
        assert int(rows["w_unique"][0]) == refs[0].size * (2 ** 32 - 1) > 2 ** 43
        assert int(rows["w_unique"].sum()) == take.size * (2 ** 32 - 1)


def test_bad_arguments_and_unsupported_handles(hip_lib, small):
    import torch

    _rng, refs, values, offsets, _sample, cand, _abund = small
    sample = np.array([3, 5, 8], np.uint64)
    for flags in (YH_DB_NO_DIRECTORY, YH_DB_NO_INDEX):
        with RefDB(values, offsets, flags=flags) as db:
            with pytest.raises(YachtHipError) as ei:
                db.gather(sample, cand)
            assert ei.value.code == _lib.YH_ERR_UNSUPPORTED
    with RefDB(values, offsets) as db:
        with pytest.raises(YachtHipError) as ei:
            db.gather(np.array([3, 8, 5], np.uint64), cand)
        assert ei.value.code == _lib.YH_ERR_UNSORTED
        with pytest.raises(ValueError, match="min_hits"):
            db.gather(sample, cand, min_hits=0)
        # min_hits = 0 past the binding's own check: both forms of the library refuse it
        rows, owner = np.zeros(4, engine.GATHER_ROW_DTYPE), np.zeros(3, np.uint32)
        n_rows, more = C.c_uint64(0), C.c_int(0)
        p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        assert db._lib.yh_gather(db._h, p(sample), None, 3, p(cand), 0, p(rows), 4, p(owner), C.byref(n_rows),
                                 C.byref(more)) == _lib.YH_ERR_INVALID_ARG
        assert b"min_hits" in db._lib.yh_last_error()
        d = torch.zeros(256, dtype=torch.int64, device="cuda:0")
        with pytest.raises(YachtHipError) as ei:
            db.gather_device(d.data_ptr(), 0, 3, d.data_ptr(), 0, d.data_ptr(), 4)
        assert ei.value.code == _lib.YH_ERR_INVALID_ARG
        assert len(refs) >= 128
        ghost_src = torch.zeros(4, dtype=torch.int32, device="cuda:0")
        db.set_ghosts(64, 4, ghost_src.data_ptr())
        with pytest.raises(YachtHipError) as ei:
            db.gather(sample, cand)
        assert ei.value.code == _lib.YH_ERR_UNSUPPORTED


def test_cross_checks_with_the_existing_entries(hip_lib, small):
    rng, refs, values, offsets, sample, cand, abund = small
    with RefDB(values, offsets) as db:
        before = db.run_counts(sample)
        rows, more, owner = db.gather(sample, cand, abund, want_owner=True)
        after = db.run_counts(sample)
        for b, a in zip(before, after):
            assert np.array_equal(b, a)
        overlap = before[0]
        assert len(rows) >= 12 and more is False
        assert np.array_equal(rows["n_overlap"], overlap[rows["ref"]])
        assert int(rows["n_unique"][0]) == int(overlap[cand != 0].max())
        assert (np.diff(rows["n_unique"].astype(np.int64)) <= 0).all()
        flags, totals = db.explain(sample, (cand != 0).astype(np.uint8) << 4, abund)
        assert int(rows["n_unique"].sum()) == int(totals[4, 0]) and int(rows["w_unique"].sum()) == int(totals[4, 1])
        assert np.array_equal(owner != NOBODY, (flags & 16) != 0)
        # the candidates = the references that overlap the sample: every known hash gets an owner
        rows, more, owner = db.gather(sample, overlap > 0, want_owner=True)
        flags, totals = db.explain(sample, (overlap > 0).astype(np.uint8))
        assert np.array_equal(owner != NOBODY, (flags & 0x80) != 0) and int(rows["n_unique"].sum()) == int(totals[7, 0])


def test_repeat_and_a_smaller_call_after_a_larger_one(hip_lib, small):
    rng, refs, values, offsets, sample, cand, abund = small
    with RefDB(values, offsets) as db:
        first = db.gather(sample, cand, abund, want_owner=True)
        second = db.gather(sample, cand, abund, want_owner=True)
        assert np.array_equal(first[0], second[0]) and first[1] == second[1] and np.array_equal(first[2], second[2])
        # a smaller sample, fewer candidates, another min_hits: nothing of the larger call survives
        few = cand.copy()
        few[np.flatnonzero(cand)[::2]] = 0
        _check(db, values, offsets, sample[::7], few, abund[::7], "smaller after larger", min_hits=2)
        _check(db, values, offsets, sample, cand, abund, "larger again")


def test_device_form_and_its_place_among_the_other_calls(hip_lib):
    import torch

    refs, values, offsets, cand, present = big()
    dev = torch.device("cuda:0")
    n = len(refs)

    def up(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).to(dev)

    sizes = (600_000, 120_000, 300_000)
    samples = [big_sample(k)[0] for k in sizes]
    abunds = [big_sample(k)[1].astype(np.uint32) for k in sizes]
    with RefDB(values, offsets) as db:
        want = [gather_oracle(values, offsets, s, cand, a) for s, a in zip(samples, abunds)]
        d_s = [up(s, np.int64) for s in samples]
        d_a = [up(a, np.int32) for a in abunds]
        d_cand = up(cand * np.uint8(0x81), np.uint8)  # (any non-zero byte is a candidate)
        d_rows = [torch.full((n, 3), -1, dtype=torch.int64, device=dev) for _ in samples]
        d_owner = [torch.full((s.size,), 0x55, dtype=torch.int32, device=dev) for s in samples]
        torch.cuda.synchronize()

        def run(k, owner=True, abund=True, cap=n):
            return db.gather_device(d_s[k].data_ptr(), d_a[k].data_ptr() if abund else 0, samples[k].size, d_cand.data_ptr(), 1,
                                    d_rows[k].data_ptr(), cap, d_owner[k].data_ptr() if owner else 0)

        def same(k, got, owner=True):
            n_rows, more = got
            db.synchronize()
            rows = d_rows[k].cpu().numpy().view(engine.GATHER_ROW_DTYPE).reshape(-1)
            assert n_rows == len(want[k][0]) and more is False and np.array_equal(rows[:n_rows], want[k][0]), k
            assert (d_rows[k][n_rows:] == -1).all()  # rows behind n_rows are not written
            if owner:
                assert np.array_equal(d_owner[k].cpu().numpy().view(np.uint32), want[k][2]), k

        same(0, run(0))
        same(1, run(1))
        got = run(2, owner=False)
        same(2, got, owner=False)
        assert bool((d_owner[2] == 0x55).all())  # d_owner = NULL leaves the array alone
        n_rows, more = run(1, abund=False, cap=10)  # d_abund = NULL: every abundance is 1; a cap on the device form
        db.synchronize()
        rows = d_rows[1].cpu().numpy().view(engine.GATHER_ROW_DTYPE).reshape(-1)[:n_rows]
        assert n_rows == 10 and more is True and np.array_equal(rows["n_unique"], want[1][0]["n_unique"][:10])
        assert np.array_equal(rows["w_unique"], rows["n_unique"])
        # between pipelined steps: their results stay what run_counts gives, and the gather call is right too
        counts = [[torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3)] for _ in samples]
        got = None
        for i in range(3):
            db.run_device_pipelined(d_s[i].data_ptr(), samples[i].size, *(c.data_ptr() for c in counts[i]))
            if i == 1:
                d_rows[0].fill_(-1)
                got = run(0)
        db.run_device_join()
        db.synchronize()
        for i in range(3):
            for g, w in zip(counts[i], db.run_counts(samples[i])):
                assert np.array_equal(g.cpu().numpy().view(np.uint32), w), ("pipelined step", i)
        same(0, got)
