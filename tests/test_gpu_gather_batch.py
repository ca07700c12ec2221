"""RefDB.gather_batch / yh_gather_batch_device on the GPU: for every sample of a block, exact equality of the rows, `more`
and the owners against the oracles of tests/gather_oracle.py applied to that sample alone, over the blocks of
tests/gather_batch_cases.py, and against RefDB.gather on the same handle.  Every check runs with and without abundances and
with and without the owner array.  Then the device form: rows behind a sample's count stay untouched, nothing of a larger
block survives, empty inputs, the errors, its place between a batched run and its compact rows, and the cross-check with
explain_batch."""
import ctypes as C

import numpy as np
import pytest
from gather_batch_cases import (MAX_ROWS, NOBODY, SET_A, SET_B, big_block, candidates, descending_block, hand_block, posting_block, want,
                                wide_block)

from yacht_amd import _lib, engine
from yacht_amd.engine import RefDB, YH_DB_NO_DIRECTORY, YH_DB_NO_INDEX, YachtHipError

pytestmark = pytest.mark.gpu


def _same(tag, got, wanted, with_owner):
    rows, more, owners = got
    assert len(rows) == len(more) == len(wanted)
    for s, (w_rows, w_more, w_owner) in enumerate(wanted):
        assert rows[s].dtype == engine.GATHER_ROW_DTYPE and rows[s].shape == w_rows.shape, (tag, s, len(rows[s]), len(w_rows))
        assert np.array_equal(rows[s], w_rows), (tag, s, rows[s][:5], w_rows[:5])
        assert more[s] is w_more, (tag, s)
        if with_owner:
            assert owners[s].dtype == np.uint32 and np.array_equal(owners[s], w_owner), (tag, s, np.flatnonzero(owners[s] != w_owner)[:10])
    if not with_owner:
        assert owners is None


def _check(db, block, mask, what, **stops):
    """gather_batch with / without abundances and with / without owners, all four against the oracle per sample."""
    for flat in (False, True):
        wanted = want(block, mask, flat, **stops)
        for with_owner in (True, False):
            got = db.gather_batch(block["samples"], block["members"], mask, None if flat else block["abunds"], want_owner=with_owner, **stops)
            _same((what, mask, "flat" if flat else "abund", "owner" if with_owner else "no owner", stops), got, wanted, with_owner)


def _against_single(db, block, mask, picks, **stops):
    """The same handle's RefDB.gather for the samples `picks`, one at a time, against gather_batch for the block."""
    rows, more, owners = db.gather_batch(block["samples"], block["members"], mask, block["abunds"], want_owner=True, **stops)
    for s in picks:
        one = db.gather(block["samples"][s], candidates(block, s, mask), block["abunds"][s], want_owner=True, **stops)
        assert np.array_equal(rows[s], one[0]) and more[s] is one[1] and np.array_equal(owners[s], one[2]), s


def test_hand_written_block_of_four(hip_lib):
    block = hand_block()
    with RefDB(block["values"], block["offsets"]) as db:
        _check(db, block, SET_A, "hand written")
        _against_single(db, block, SET_A, range(4))
        _check(db, block, SET_A, "hand written, capped", cap_rows=2)


@pytest.mark.parametrize("length", [4, 5, 300])
def test_posting_list_lengths(hip_lib, length):
    block = posting_block(length)
    with RefDB(block["values"], block["offsets"]) as db:
        _check(db, block, SET_A, f"lists of {length}")
        _check(db, block, SET_A, f"lists of {length}, capped", cap_rows=2)
        _against_single(db, block, SET_A, range(3))


@pytest.fixture(scope="module")
def big_db(hip_lib):
    block = big_block(1)
    with RefDB(block["values"], block["offsets"]) as db:
        assert db.info()["filter_bytes"] > 0 and db.info()["n_shared_distinct"] > 1000
        yield db


@pytest.mark.parametrize("n_samples", [1, 2, 65, 256])
def test_blocks_over_the_big_database(big_db, n_samples):
    block = big_block(n_samples)
    for mask in (SET_A, SET_B):  # bit 0 in one call and bit 6 in another, over member bytes that hold both sets
        _check(big_db, block, mask, f"big {n_samples}")
    _against_single(big_db, block, SET_B, sorted({0, n_samples // 2, n_samples - 1}))
    _check(big_db, block, SET_A, f"big {n_samples}, capped", cap_rows=8)


def test_samples_that_finish_in_different_rounds_and_the_stops(hip_lib):
    block = descending_block(40)
    with RefDB(block["values"], block["offsets"]) as db:
        _check(db, block, SET_A, "descending")
        _against_single(db, block, SET_A, (0, 1, 17, 39))
        for cap in (_lib.YH_GATHER_ROUNDS_PER_SYNC - 1, _lib.YH_GATHER_ROUNDS_PER_SYNC, _lib.YH_GATHER_ROUNDS_PER_SYNC + 1):
            _check(db, block, SET_A, "descending, capped", cap_rows=cap)
        # cap_rows = the rows sample 20 has: that sample is not cut short
        rows, more, _ = db.gather_batch(block["samples"], block["members"], SET_A, block["abunds"], cap_rows=20)
        assert len(rows[20]) == 20 and more[20] is False and more[21] is True and len(rows[21]) == 20
        _check(db, block, SET_A, "descending, cap 20", cap_rows=20)
        _check(db, block, SET_A, "descending, min_hits", min_hits=30)
        _check(db, block, SET_A, "descending, min_hits and cap", min_hits=12, cap_rows=5)
        _check(db, block, SET_A, "descending, no row allowed", cap_rows=0)


def test_abundances_whose_sums_pass_32_bits(big_db):
    block = wide_block()
    _check(big_db, block, SET_A, "wide sums")
    rows, _more, _ = big_db.gather_batch(block["samples"], block["members"], SET_A, block["abunds"])
    assert int(rows[0]["ref"][0]) == 300 and int(rows[0]["w_unique"][0]) == int(rows[0]["n_unique"][0]) * (2 ** 32 - 1) > 2 ** 43
    assert int(rows[0]["w_unique"].sum()) == block["samples"][0].size * (2 ** 32 - 1)


# ---- the device form ----------------------------------------------------------------------------------------------------------
class _Device:
    """A block on the device, and output buffers pre-filled with sentinels (one spare sample behind the block's)."""

    def __init__(self, torch, block, cap, spare=1):
        dev = torch.device("cuda:0")

        def up(a, dtype):
            return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).to(dev)

        self.torch, self.block, self.cap = torch, block, cap
        self.b = len(block["samples"])
        self.offs = np.concatenate([[0], np.cumsum([s.size for s in block["samples"]])]).astype(np.uint64)
        self.total = int(self.offs[-1])
        cat = np.concatenate(block["samples"]) if self.total else np.zeros(0, np.uint64)
        cat_a = np.concatenate(block["abunds"]).astype(np.uint32) if self.total else np.zeros(0, np.uint32)
        self.d_s = up(np.concatenate([cat, np.zeros(2, np.uint64)]), np.int64)
        self.d_a = up(np.concatenate([cat_a, np.zeros(4, np.uint32)]), np.int32)
        self.d_o = up(self.offs, np.int64)
        self.d_m = up(block["members"], np.uint8)
        self.new_outputs(self.b + spare)

    def new_outputs(self, n):
        torch, dev = self.torch, self.torch.device("cuda:0")
        self.d_rows = torch.full((n, max(self.cap, 1), 3), -1, dtype=torch.int64, device=dev)
        self.d_owner = torch.full((self.total + 64,), 0x55555555, dtype=torch.int32, device=dev)
        self.d_n = torch.full((n,), 0x7777, dtype=torch.int32, device=dev)
        self.d_more = torch.full((n,), 0x77, dtype=torch.uint8, device=dev)

    def run(self, db, mask, abund=True, owner=True, min_hits=1, total=None, outputs=None):
        o = outputs or self
        db.gather_batch_device(self.d_s.data_ptr(), self.d_o.data_ptr(), self.d_a.data_ptr() if abund else 0, self.b,
                               self.total if total is None else total, self.d_m.data_ptr(), mask, min_hits, o.d_rows.data_ptr(), self.cap,
                               o.d_owner.data_ptr() if owner else 0, o.d_n.data_ptr(), o.d_more.data_ptr())

    def same(self, db, wanted, owner=True, outputs=None):
        o = outputs or self
        db.synchronize()
        n_rows = o.d_n.cpu().numpy().view(np.uint32)
        more = o.d_more.cpu().numpy()
        rows = o.d_rows.cpu().numpy().reshape(o.d_rows.shape[0], -1)
        owners = o.d_owner.cpu().numpy().view(np.uint32)
        for s, (w_rows, w_more, w_owner) in enumerate(wanted):
            assert n_rows[s] == len(w_rows) and more[s] == int(w_more), (s, n_rows[s], len(w_rows), more[s], w_more)
            got = rows[s].view(engine.GATHER_ROW_DTYPE)
            assert np.array_equal(got[:len(w_rows)], w_rows), s
            assert (rows[s][3 * len(w_rows):] == -1).all(), s  # rows behind n_rows[s] are not written
            if owner:
                assert np.array_equal(owners[int(self.offs[s]):int(self.offs[s + 1])], w_owner), s
        if owner:
            assert (owners[self.total:] == 0x55555555).all()
        else:
            assert (owners == 0x55555555).all()  # d_owner = NULL leaves the array alone
        # nothing behind the block's samples
        assert (n_rows[len(wanted):] == 0x7777).all() and (more[len(wanted):] == 0x77).all() and (rows[len(wanted):] == -1).all()


def test_device_form_leaves_rows_behind_the_count_untouched(hip_lib):
    import torch

    block = descending_block(40)
    with RefDB(block["values"], block["offsets"]) as db:
        for cap in (33, 40):
            d = _Device(torch, block, cap)
            d.run(db, SET_A)
            d.same(db, want(block, SET_A, cap_rows=cap))
            d.new_outputs(41)
            d.run(db, SET_A, abund=False, owner=False)
            d.same(db, want(block, SET_A, flat=True, cap_rows=cap), owner=False)
        d = _Device(torch, block, 40)
        d.run(db, SET_A, min_hits=30)
        d.same(db, want(block, SET_A, min_hits=30))


def test_a_block_of_two_after_a_block_of_256_on_the_same_buffers(big_db):
    import torch

    first, second = big_block(256), big_block(2)
    cap = 64
    d1, d2 = _Device(torch, first, cap), _Device(torch, second, cap)
    d1.run(big_db, SET_A)
    d1.same(big_db, want(first, SET_A, cap_rows=cap))
    # the second block writes into the first one's outputs: its two samples' counts and flags are its own, the rows behind its
    # counts keep what the larger block left, and sample 2 onwards is not touched
    before = d1.d_rows.clone()
    n_before = d1.d_n.clone()
    big_db.gather_batch_device(d2.d_s.data_ptr(), d2.d_o.data_ptr(), d2.d_a.data_ptr(), 2, d2.total, d2.d_m.data_ptr(), SET_A, 1,
                               d1.d_rows.data_ptr(), cap, 0, d1.d_n.data_ptr(), d1.d_more.data_ptr())
    big_db.synchronize()
    wanted = want(second, SET_A, cap_rows=cap)
    n_rows, more = d1.d_n.cpu().numpy().view(np.uint32), d1.d_more.cpu().numpy()
    rows = d1.d_rows.cpu().numpy().reshape(257, -1)
    for s in range(2):
        k = len(wanted[s][0])
        assert n_rows[s] == k and more[s] == int(wanted[s][1])
        assert np.array_equal(rows[s].view(engine.GATHER_ROW_DTYPE)[:k], wanted[s][0])
        assert np.array_equal(rows[s][3 * k:], before[s].cpu().numpy().reshape(-1)[3 * k:])
    assert len(wanted[1][0]) < int(n_before[1]) or len(wanted[0][0]) != int(n_before[0])  # (the counts did change)
    assert torch.equal(d1.d_rows[2:], before[2:]) and torch.equal(d1.d_n[2:], n_before[2:])
    # and the larger block again, on fresh outputs: no state of the small call survives
    d1.new_outputs(257)
    d1.run(big_db, SET_B, abund=False)
    d1.same(big_db, want(first, SET_B, flat=True, cap_rows=cap))


def test_empty_inputs(hip_lib, big_db):
    import torch

    block = big_block(2)
    # an empty database: no rows, nobody owns anything
    with RefDB(np.zeros(0, np.uint64), np.zeros(3, np.uint64)) as db:
        samples = [np.array([3, 5], np.uint64), np.array([9], np.uint64)]
        rows, more, owners = db.gather_batch(samples, np.ones((2, 2), np.uint8), 1, [np.array([4, 4]), None], want_owner=True)
        assert [len(r) for r in rows] == [0, 0] and more == [False, False]
        assert owners[0].tolist() == [NOBODY, NOBODY] and owners[1].tolist() == [NOBODY]
    with RefDB(np.zeros(0, np.uint64), np.zeros(1, np.uint64)) as db:
        rows, more, _ = db.gather_batch([np.array([3, 5], np.uint64)], np.zeros((1, 0), np.uint8))
        assert len(rows[0]) == 0 and more == [False]
    # only empty samples
    empty = np.zeros(0, np.uint64)
    rows, more, owners = big_db.gather_batch([empty, empty, empty], block["members"][[0, 1, 0]], SET_A, want_owner=True)
    assert [len(r) for r in rows] == [0, 0, 0] and more == [False] * 3 and all(o.size == 0 for o in owners)
    # total_hashes == 0 with non-empty device offsets, on outputs that hold an earlier block's results: zero rows, more 0,
    # and (all zero of the) owners "nobody" -- the owner array is not touched
    d = _Device(torch, block, 16)
    d.run(big_db, SET_A)
    d.same(big_db, want(block, SET_A, cap_rows=16))
    assert int(d.d_n[0]) == 16 and int(d.d_more[0]) == 1
    d.d_owner.fill_(0x55555555)
    rows_before = d.d_rows.clone()
    d.run(big_db, SET_A, total=0)
    big_db.synchronize()
    assert d.d_n.tolist() == [0, 0, 0x7777] and d.d_more.tolist() == [0, 0, 0x77]
    assert bool((d.d_owner == 0x55555555).all()) and torch.equal(d.d_rows, rows_before)


def test_errors(hip_lib):
    import torch

    block = posting_block(4)
    samples, members, n_refs = block["samples"], block["members"], block["members"].shape[1]
    for flags in (YH_DB_NO_DIRECTORY, YH_DB_NO_INDEX):
        with RefDB(block["values"], block["offsets"], flags=flags) as db:
            with pytest.raises(YachtHipError) as ei:
                db.gather_batch(samples, members)
            assert ei.value.code == _lib.YH_ERR_UNSUPPORTED
    with RefDB(block["values"], block["offsets"]) as db:
        with pytest.raises(YachtHipError) as ei:
            db.gather_batch([samples[0], np.array([3, 8, 5], np.uint64), samples[2]], members)
        assert ei.value.code == _lib.YH_ERR_UNSORTED
        # the binding's own checks
        for kwargs, word in ((dict(min_hits=0), "min_hits"), (dict(cand_mask=0), "cand_mask"), (dict(cand_mask=256), "cand_mask"),
                             (dict(cap_rows=MAX_ROWS + 1), "cap_rows"), (dict(cap_rows=-1), "cap_rows")):
            with pytest.raises(ValueError, match=word):
                db.gather_batch(samples, members, **kwargs)
        with pytest.raises(ValueError, match="1..256 samples"):
            db.gather_batch([], np.zeros((0, n_refs), np.uint8))
        with pytest.raises(ValueError, match="members must be"):
            db.gather_batch(samples, members[:2])
        # ... and past them: both forms of the library refuse each
        p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        cat = np.concatenate(samples)
        offs = np.concatenate([[0], np.cumsum([s.size for s in samples])]).astype(np.uint64)
        offs257, many = np.zeros(258, np.uint64), np.zeros((257, n_refs), np.uint8)
        rows, n_rows, more = np.zeros((257, 4), engine.GATHER_ROW_DTYPE), np.zeros(257, np.uint32), np.zeros(257, np.uint8)

        def host(n=3, mask=1, min_hits=1, cap=4, o=offs, m=members):
            return db._lib.yh_gather_batch(db._h, p(cat), p(o), None, n, p(m), mask, min_hits, p(rows), cap, None, p(n_rows), p(more))

        assert host() == _lib.YH_OK
        for kwargs, word in ((dict(n=0, o=offs257, m=many), b"samples"), (dict(n=257, o=offs257, m=many), b"samples"),
                             (dict(min_hits=0), b"min_hits"), (dict(mask=0), b"cand_mask"), (dict(cap=MAX_ROWS + 1), b"cap_rows")):
            assert host(**kwargs) == _lib.YH_ERR_INVALID_ARG, kwargs
            assert word in db._lib.yh_last_error(), (kwargs, db._lib.yh_last_error())
        big_offs = np.array([0, 2 ** 32], np.uint64)  # (refused before a hash is read)
        assert host(n=1, o=big_offs) == _lib.YH_ERR_INVALID_ARG and b"2^32" in db._lib.yh_last_error()
        d = torch.zeros(4096, dtype=torch.int64, device="cuda:0")

        def device(n=3, total=8, mask=1, min_hits=1, cap=4):
            return db._lib.yh_gather_batch_device(db._h, C.c_void_p(d.data_ptr()), C.c_void_p(d.data_ptr()), None, n, total,
                                                  C.c_void_p(d.data_ptr()), mask, min_hits, C.c_void_p(d.data_ptr()), cap, None,
                                                  C.c_void_p(d.data_ptr()), C.c_void_p(d.data_ptr()))

        for kwargs in (dict(n=0), dict(n=257), dict(min_hits=0), dict(mask=0), dict(cap=MAX_ROWS + 1), dict(total=2 ** 32)):
            assert device(**kwargs) == _lib.YH_ERR_INVALID_ARG, kwargs
        with pytest.raises(YachtHipError) as ei:
            db.gather_batch_device(d.data_ptr(), d.data_ptr(), 0, 3, 8, d.data_ptr(), 1, 0, d.data_ptr(), 4, 0, d.data_ptr(), d.data_ptr())
        assert ei.value.code == _lib.YH_ERR_INVALID_ARG


def test_ghosts_make_the_handle_unsupported(big_db):
    import torch

    block = big_block(2)
    with RefDB(block["values"], block["offsets"]) as db:
        ghost_src = torch.zeros(4, dtype=torch.int32, device="cuda:0")
        db.set_ghosts(64, 4, ghost_src.data_ptr())
        for call in (lambda: db.gather(block["samples"][1], candidates(block, 1, SET_A)),
                     lambda: db.gather_batch(block["samples"], block["members"])):
            with pytest.raises(YachtHipError) as ei:
                call()
            assert ei.value.code == _lib.YH_ERR_UNSUPPORTED  # exactly where the single call is


def test_between_the_batch_counts_and_their_compact_rows(big_db):
    """gather_batch_device queued between yh_run_batch_device and yh_run_batch_rows_pack_device: the rows of the run equal those
    of a run without it, and the ranking is right."""
    import torch

    db, block = big_db, big_block(65)
    n_refs = block["members"].shape[1]
    d = _Device(torch, block, 64)
    b, total, cap = d.b, d.total, 65 * n_refs
    runs = []
    for with_gather in (False, True):
        c = torch.zeros((3, b, n_refs), dtype=torch.int32, device="cuda:0")
        vals = torch.zeros((cap, 3), dtype=torch.int32, device="cuda:0")
        out = torch.zeros((cap, 5), dtype=torch.int32, device="cuda:0")
        n_rows = torch.zeros(2, dtype=torch.int32, device="cuda:0")
        db.run_batch_device(d.d_s.data_ptr(), d.d_o.data_ptr(), b, total, c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr())
        if with_gather:
            d.run(db, SET_A)
        db.run_batch_rows_pack_device(c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr(), vals.data_ptr(), cap, n_rows[0].data_ptr())
        db.run_batch_rows_unpack_device(vals.data_ptr(), cap, out.data_ptr(), n_rows[1].data_ptr())
        db.synchronize()
        torch.cuda.synchronize()
        k = int(n_rows[1])
        runs.append((k, out[:k].cpu().numpy(), c.cpu().numpy()))
    assert runs[0][0] == runs[1][0] > 0 and np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])
    assert np.array_equal(runs[1][2][0, 64].view(np.uint32), db.run_counts(block["samples"][64])[0])
    d.same(db, want(block, SET_A, cap_rows=64))


def test_cross_check_with_explain_batch(big_db):
    """min_hits = 1 and cap_rows >= N: a sample's n_unique and w_unique add up to explain_batch's totals for the same member rows."""
    block = big_block(65)
    _flags, totals = big_db.explain_batch(block["samples"], block["members"], block["abunds"], want_flags=False)
    for mask, bit in ((SET_A, 0), (SET_B, 6)):
        rows, more, owners = big_db.gather_batch(block["samples"], block["members"], mask, block["abunds"], want_owner=True)
        assert not any(more)
        for s in range(65):
            assert int(rows[s]["n_unique"].sum()) == int(totals[s, bit, 0]) == int((owners[s] != NOBODY).sum()), (mask, s)
            assert int(rows[s]["w_unique"].sum()) == int(totals[s, bit, 1]), (mask, s)
        assert int(totals[:, bit, 0].sum()) > 1000
