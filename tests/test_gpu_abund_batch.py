"""RefDB.abundance_batch / yh_abund_batch_device on the GPU: exact equality of all three arrays, row by row, with the
brute-force oracle (tests/abund_oracle.py) run PER SAMPLE and with RefDB.abundance (test_gpu_abundance.py pins it to the
same oracle).  The blocks come from abund_batch_cases.py (test_abund_batch_cases_cpu.py shows what they hold): sizes around
the kernel's tile, empty samples first, in the middle and last, twins that share hashes but not abundances.  The oracles
are computed once per module."""
import ctypes as C

import numpy as np
import pytest
from abund_batch_cases import EDGE_SIZES, I_2T1, T, abundances, big_db, block, edge_block, oracle_block, sizes
from abund_oracle import abundance_oracle

from yacht_amd import _lib, synth
from yacht_amd.engine import RefDB, YH_DB_NO_DIRECTORY, YH_DB_NO_INDEX, YachtHipError

pytestmark = pytest.mark.gpu

PICKED_65 = [0, 1, 2, 3, 4, 5, 6, 7, 9, 32, 40, 64]  # the oracle's samples of the block of 65: the edge sizes, the twin, empties


def _eq(got, want, what):
    assert got[0].dtype == np.uint64 and got[1].dtype == np.uint64
    assert np.array_equal(got[0], want[0]), (what, "w_overlap")
    assert np.array_equal(got[1], want[1]), (what, "w_match")
    if got[2] is not None:
        assert got[2].dtype == np.float64 and np.array_equal(got[2], want[2]), (what, "med_match", np.flatnonzero(got[2] != want[2])[:10])


def _check(db, samples, abunds, want, what):
    """The host form with the medians and sums-only; want = {s: the three arrays} for the samples that have an answer."""
    got = db.abundance_batch(samples, abunds)
    assert all(g.shape == (len(samples), db.n_refs) for g in got)
    sums = db.abundance_batch(samples, abunds, want_median=False)
    assert sums[2] is None and np.array_equal(sums[0], got[0]) and np.array_equal(sums[1], got[1]), (what, "sums only")
    for s, w in want.items():
        _eq([g[s] for g in got], w, (what, s))
    return got


@pytest.fixture(scope="module")
def big():
    values, offsets, n_refs, pool = big_db()
    rng = np.random.default_rng(602)
    blocks = {}
    for n in (1, 2, 9, 65):
        samples, abunds = block(700 + n, pool, sizes(rng, n), twin=(6, 9) if n > 9 else None)
        blocks[n] = (samples, abunds, oracle_block(values, offsets, samples, abunds, PICKED_65 if n == 65 else None))
    return values, offsets, n_refs, pool, blocks


@pytest.fixture(scope="module")
def five_entry():
    """synth.config2 at scaled = 1000 keeps the full-hash (five-entry) buckets and has no filter; clusters appended."""
    values, offsets, sample = synth.config2(seed=603, n_refs=60, n_sample=40_000)
    rng = np.random.default_rng(603)
    refs = [values[int(offsets[i]):int(offsets[i + 1])] for i in range(len(offsets) - 1)] + \
        synth.clustered_refs(rng, 6, (1, 0.9, 0.5, 0.25, 0.1), 4000)
    values, offsets = synth.pack(refs)
    pool = np.union1d(sample, synth.sample_from_refs(rng, refs, list(range(len(refs))), 0.05, 1000))
    pool = np.union1d(pool, synth.random_sketch(rng, 30_000, synth.max_hash_for_scaled(1000)))  # hashes nobody holds
    samples, abunds = block(900, pool, sizes(rng, 9))
    return values, offsets, len(refs), samples, abunds, oracle_block(values, offsets, samples, abunds)


def test_the_edge_block_against_the_oracle(hip_lib):
    values, offsets, _n_refs, _pool = big_db()
    samples, abunds, want, _counts = edge_block()
    with RefDB(values, offsets) as db:
        assert db.info()["filter_bytes"] > 0 and db.info()["n_shared_distinct"] > 1000
        _check(db, samples, abunds, want, "edge block")


@pytest.mark.parametrize("n_samples", [1, 2, 9, 65])  # 9: the first where the order of 8 quantile steps x samples wraps
def test_blocks_against_the_oracle_per_sample(hip_lib, big, n_samples):
    values, offsets, _n_refs, _pool, blocks = big
    samples, abunds, want = blocks[n_samples]
    with RefDB(values, offsets) as db:
        got = _check(db, samples, abunds, want, f"big {n_samples}")
        for s in range(n_samples):
            if s not in want:
                _eq([g[s] for g in got], db.abundance(samples[s], abunds[s]), ("big 65 against abundance", s))
    if n_samples == 65:  # the twins: the same hashes, other abundances, other sums
        assert np.array_equal(samples[6], samples[9]) and not np.array_equal(got[0][6], got[0][9])
        assert [samples[s].size for s in (0, 32, 64)] == [0, 0, 0] and not got[0][[0, 32, 64]].any() and not got[2][[0, 32, 64]].any()


def test_small_database_with_the_five_entry_buckets(hip_lib, five_entry):
    values, offsets, _n_refs, samples, abunds, want = five_entry
    with RefDB(values, offsets) as db:
        assert db.info()["filter_bytes"] == 0
        got = _check(db, samples, abunds, want, "five-entry")
        assert int((got[1] > 0).sum()) > 50


def test_one_reference(hip_lib):
    rng = np.random.default_rng(604)
    ref = synth.random_sketch(rng, 4000, synth.max_hash_for_scaled(1000))
    values, offsets = synth.pack([ref])
    pool = np.union1d(ref[::2], synth.random_sketch(rng, 3000, synth.max_hash_for_scaled(1000)))
    samples, abunds = block(604, pool, [0, T + 1, 1, 700, 0])
    with RefDB(values, offsets) as db:
        got = _check(db, samples, abunds, oracle_block(values, offsets, samples, abunds), "one reference")
        assert got[0].shape == (5, 1) and got[0][1, 0] == got[1][1, 0] > 0


def test_full_block_of_256_samples(hip_lib, big):
    """256 samples: RefDB.abundance per sample, and the oracle itself on eight."""
    values, offsets, _n_refs, pool, _blocks = big
    rng = np.random.default_rng(611)
    samples, abunds = block(611, pool, sizes(rng, 256), twin=(6, 200))
    picked = [1, 2, 5, 6, 100, 200, 254, 255]
    with RefDB(values, offsets) as db:
        got = _check(db, samples, abunds, oracle_block(values, offsets, samples, abunds, picked), "full block")
        for s in range(256):
            _eq([g[s] for g in got], db.abundance(samples[s], abunds[s]), ("full block against abundance", s))
        assert not np.array_equal(got[0][6], got[0][200])  # the twins


def test_all_ones_give_the_batched_run_counts(hip_lib, big):
    values, offsets, _n_refs, _pool, blocks = big
    samples, _abunds, _want = blocks[65]
    with RefDB(values, offsets) as db:
        overlap, _n_excl, n_match = db.run_batch(samples)
        w_ov, w_m, med = db.abundance_batch(samples, [np.ones(s.size, np.uint32) for s in samples])
        assert np.array_equal(w_ov, overlap.astype(np.uint64)) and np.array_equal(w_m, n_match.astype(np.uint64))
        assert n_match.any() and np.array_equal(med, (n_match > 0).astype(np.float64))


def test_a_tile_that_touches_more_references_than_the_hit_table_has_slots(hip_lib):
    """6000 references of 4 hashes each and a sample that holds every hash: a tile of T consecutive hashes touches ~T
    references, more than the 512 slots of the LDS table, so most sums leave by the direct atomics."""
    rng = np.random.default_rng(605)
    hashes = synth.random_sketch(rng, 24_000, synth.max_hash_for_scaled(1000))
    owner = rng.permutation(24_000) % 6000
    refs = [np.sort(hashes[owner == j]) for j in range(6000)]
    values, offsets = synth.pack(refs)
    samples = [hashes, hashes[::3].copy()]
    abunds = [abundances(rng, s, smp.size) for s, smp in enumerate(samples)]
    want = {}
    for s in range(2):  # every hash has one holder: the oracle's answer by a group-by (abund_oracle.py would take minutes here)
        own = owner[::3] if s else owner
        w = np.zeros(6000, np.uint64)
        np.add.at(w, own, abunds[s].astype(np.uint64))
        med = np.array([np.median(abunds[s][own == j].astype(np.float64)) if (own == j).any() else 0.0 for j in range(6000)])
        want[s] = (w, w, med)
    small = np.arange(0, 24_000, 400)
    tiny = abundance_oracle(values, offsets, hashes[small], abunds[0][small])  # ... and abund_oracle.py on a sample of 60
    with RefDB(values, offsets) as db:
        _check(db, samples, abunds, want, "crowded table")
        _check(db, [hashes[small]], [abunds[0][small]], {0: tiny}, "crowded table, the oracle")


def test_abundances_whose_sums_pass_32_bits(hip_lib, big):
    values, offsets, _n_refs, _pool, blocks = big
    samples, abunds, _want = blocks[9]
    samples, abunds = list(samples), list(abunds)
    j = int(np.argmax(np.diff(offsets.astype(np.int64))))  # 2 T + 1 hashes of the largest reference: > 256 hits on one row
    samples[I_2T1] = np.asarray(values[int(offsets[j]):int(offsets[j]) + 2 * T + 1], dtype=np.uint64)
    assert samples[I_2T1].size == 2 * T + 1
    abunds[I_2T1] = np.full(samples[I_2T1].size, 2 ** 32 - 1, dtype=np.uint64)
    abunds[3] = np.where(np.arange(samples[3].size) % 2 == 0, 2 ** 32 - 1, 2 ** 32 - 2).astype(np.uint64)
    want = oracle_block(values, offsets, samples, abunds, [3, I_2T1])
    with RefDB(values, offsets) as db:
        w_ov, w_m, med = _check(db, samples, abunds, want, "all ones bits")
    assert int(w_ov[I_2T1].max()) > 2 ** 40 and bool((med[I_2T1][w_m[I_2T1] > 0] == float(2 ** 32 - 1)).all())
    assert int((med[3] == 2 ** 32 - 1.5).sum()) > 0  # an even count of alternating values: x.5


def _up(torch, a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).to("cuda:0")


def _device_block(torch, samples, abunds):
    offs = np.zeros(len(samples) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([s.size for s in samples])
    cat = np.concatenate(samples) if offs[-1] else np.zeros(1, np.uint64)
    cat_ab = np.concatenate(abunds).astype(np.uint32) if offs[-1] else np.zeros(1, np.uint32)
    return _up(torch, cat, np.int64), _up(torch, offs, np.int64), _up(torch, cat_ab, np.int32), offs


GUARD = 64


def _outputs(torch, rows, n_refs):
    """Three poisoned [rows][N] arrays with GUARD poisoned words behind each."""
    return (torch.full((rows * n_refs + GUARD,), -1, dtype=torch.int64, device="cuda:0"),
            torch.full((rows * n_refs + GUARD,), -1, dtype=torch.int64, device="cuda:0"),
            torch.full((rows * n_refs + GUARD,), -7.25, dtype=torch.float64, device="cuda:0"))


def _rows(out, rows, n_refs):
    return (out[0][:rows * n_refs].cpu().numpy().view(np.uint64).reshape(rows, n_refs),
            out[1][:rows * n_refs].cpu().numpy().view(np.uint64).reshape(rows, n_refs),
            out[2][:rows * n_refs].cpu().numpy().reshape(rows, n_refs))


def _untouched_behind(out, rows, n_refs):
    """Row `rows` onwards and the guard words still hold the poison."""
    return bool((out[0][rows * n_refs:] == -1).all()) and bool((out[1][rows * n_refs:] == -1).all()) and \
        bool((out[2][rows * n_refs:] == -7.25).all())


def test_device_form_leaves_nothing_stale_and_writes_nothing_else(hip_lib, big):
    """A large block, then a small one, then a block of only empty samples, into the same poisoned buffers; medians off."""
    import torch

    values, offsets, n_refs, _pool, blocks = big
    with RefDB(values, offsets) as db:
        host = {n: db.abundance_batch(blocks[n][0], blocks[n][1]) for n in (9, 2)}  # (against the oracle above)
        out = _outputs(torch, 10, n_refs)
        for n in (9, 2):
            samples, abunds, _want = blocks[n]
            d_s, d_o, d_a, offs = _device_block(torch, samples, abunds)
            db.abundance_batch_device(d_s.data_ptr(), d_o.data_ptr(), d_a.data_ptr(), n, int(offs[-1]), *(o.data_ptr() for o in out))
            db.synchronize()
            got = _rows(out, n, n_refs)
            assert all(np.array_equal(g, h) for g, h in zip(got, host[n])), n
            assert _untouched_behind(out, 9, n_refs), "row 9 and the guard words"
        # the rows of the large block behind the small one are the large block's still: rows 2.. are not this call's
        assert np.array_equal(_rows(out, 9, n_refs)[0][2:], host[9][0][2:])
        # medians off (d_med_match = NULL): the same sums, the median array untouched
        out[2].fill_(-7.25)
        out[0].fill_(-1)
        db.abundance_batch_device(d_s.data_ptr(), d_o.data_ptr(), d_a.data_ptr(), 2, int(offs[-1]), out[0].data_ptr(), out[1].data_ptr(), 0)
        db.synchronize()
        got = _rows(out, 2, n_refs)
        assert np.array_equal(got[0], host[2][0]) and np.array_equal(got[1], host[2][1]) and bool((out[2] == -7.25).all())
        assert bool((out[0][2 * n_refs:] == -1).all())
        # a block of only empty samples over the dirty buffers comes back zero, with and without a total of its own
        zero_offs = torch.zeros(4, dtype=torch.int64, device="cuda:0")
        for total in (0, 5):
            for o in out:
                o.fill_(3)
            db.abundance_batch_device(d_s.data_ptr(), zero_offs.data_ptr(), d_a.data_ptr(), 3, total, *(o.data_ptr() for o in out))
            db.synchronize()
            assert not any(g.any() for g in _rows(out, 3, n_refs)) and bool((out[0][3 * n_refs:] == 3).all()) and bool((out[2][3 * n_refs:] == 3).all())


@pytest.mark.parametrize("delta", ["larger", "smaller", "one short", "tiny"])
def test_a_total_that_is_not_the_offsets_own(hip_lib, big, delta):
    """total_hashes sizes the launch and the key buffer; the kernels go by the device offsets.  A larger value costs idle
    workgroups; with a smaller one the samples that end behind it find their medians without a key buffer."""
    import torch

    values, offsets, n_refs, _pool, blocks = big
    samples, abunds, _want = blocks[9]
    d_s, d_o, d_a, offs = _device_block(torch, samples, abunds)
    true = int(offs[-1])
    total = {"larger": true + 5 * T + 3, "smaller": int(offs[6]) + 11, "one short": true - 1, "tiny": 1}[delta]
    with RefDB(values, offsets) as db:
        host = db.abundance_batch(samples, abunds)
        out = _outputs(torch, 9, n_refs)
        db.abundance_batch_device(d_s.data_ptr(), d_o.data_ptr(), d_a.data_ptr(), 9, total, *(o.data_ptr() for o in out))
        db.synchronize()
        got = _rows(out, 9, n_refs)
        assert all(np.array_equal(g, h) for g, h in zip(got, host)), delta
        assert _untouched_behind(out, 9, n_refs)


def test_an_empty_database_gives_zero_rows(hip_lib):
    with RefDB(np.zeros(0, np.uint64), np.zeros(3, np.uint64)) as db:  # two references without a hash
        got = db.abundance_batch([np.array([3, 5], np.uint64), np.array([4], np.uint64)], [[4, 4], [9]])
        assert all(g.shape == (2, 2) and not g.any() for g in got)


def test_between_the_batch_counts_and_their_compact_rows(hip_lib, big):
    """abundance_batch_device queued between yh_run_batch_device and yh_run_batch_rows_pack_device: the rows equal those of a
    run without it, and the abundance rows are right."""
    import torch

    values, offsets, n_refs, _pool, blocks = big
    samples, abunds, _want = blocks[65]
    d_s, d_o, d_a, offs = _device_block(torch, samples, abunds)
    total, b, cap = int(offs[-1]), len(samples), 65 * n_refs
    with RefDB(values, offsets) as db:
        host = db.abundance_batch(samples, abunds)
        out = _outputs(torch, b, n_refs)
        rows = []
        for with_abund in (False, True):
            c = torch.zeros((3, b, n_refs), dtype=torch.int32, device="cuda:0")
            vals = torch.zeros((cap, 3), dtype=torch.int32, device="cuda:0")
            packed = torch.zeros((cap, 5), dtype=torch.int32, device="cuda:0")
            n_rows = torch.zeros(2, dtype=torch.int32, device="cuda:0")
            db.run_batch_device(d_s.data_ptr(), d_o.data_ptr(), b, total, c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr())
            if with_abund:
                db.abundance_batch_device(d_s.data_ptr(), d_o.data_ptr(), d_a.data_ptr(), b, total, *(o.data_ptr() for o in out))
            db.run_batch_rows_pack_device(c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr(), vals.data_ptr(), cap, n_rows[0].data_ptr())
            db.run_batch_rows_unpack_device(vals.data_ptr(), cap, packed.data_ptr(), n_rows[1].data_ptr())
            db.synchronize()
            torch.cuda.synchronize()
            k = int(n_rows[1])
            rows.append((k, packed[:k].cpu().numpy(), c.cpu().numpy()))
        assert rows[0][0] == rows[1][0] > 0 and np.array_equal(rows[0][1], rows[1][1]) and np.array_equal(rows[0][2], rows[1][2])
        assert all(np.array_equal(g, h) for g, h in zip(_rows(out, b, n_refs), host))


def test_errors(hip_lib, five_entry):
    import torch

    values, offsets, n_refs, samples, abunds, _want = five_entry
    for flags in (YH_DB_NO_DIRECTORY, YH_DB_NO_INDEX):
        with RefDB(values, offsets, flags=flags) as db:
            with pytest.raises(YachtHipError) as ei:
                db.abundance_batch(samples[:2], abunds[:2])
            assert ei.value.code == _lib.YH_ERR_UNSUPPORTED
    with RefDB(values, offsets) as db:
        with pytest.raises(YachtHipError) as ei:
            db.abundance_batch([samples[1], np.array([3, 8, 5], np.uint64)], [abunds[1], [1, 1, 1]])
        assert ei.value.code == _lib.YH_ERR_UNSORTED
        p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731  (0 and 257 samples, past the binding's own check)
        offs = np.zeros(258, dtype=np.uint64)
        rows = np.zeros((257, n_refs), np.uint64)
        for n in (0, 257):
            assert db._lib.yh_abund_batch(db._h, None, p(offs), None, n, p(rows), p(rows), None) == _lib.YH_ERR_INVALID_ARG
        d = torch.zeros(4096, dtype=torch.int64, device="cuda:0")
        for n in (0, 257):
            with pytest.raises(YachtHipError) as ei:
                db.abundance_batch_device(d.data_ptr(), d.data_ptr(), d.data_ptr(), n, 0, d.data_ptr(), d.data_ptr(), 0)
            assert ei.value.code == _lib.YH_ERR_INVALID_ARG
