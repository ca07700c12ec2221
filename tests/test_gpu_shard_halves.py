"""GPU: the two halves of the sharded `yacht run` step, called directly, in ONE process -- R handles stand in for R ranks and
torch.stack / slice assignment for the all-gather -- so that every rank's share is checked on its own (a sum over the ranks
lets errors of two ranks cancel) and at 3, 5 and 8 ranks:
  yh_run_local_range_device / yh_run_finish_range_device            hash-range shards, one sample per step context
  yh_run_local_device / yh_run_finish_device + yh_db_set_ghosts     reference shards with ghosts
  yh_run_batch_local_range_device / _finish_range_device            a block of samples per batch slot, words dense or packed
Cases and expectations: tests/shard_cases.py (oracle.overlap / oracle.exclusive per rank; guarded by
tests/test_shard_cases_cpu.py).  Every comparison is exact; every output buffer holds 0xFFFFFFFF before the call that must
overwrite it; the host synchronizes between the halves (the kernels are under test here, not the stream ordering)."""
import contextlib

import numpy as np
import pytest

import shard_cases as sc
from yacht_amd import _lib
from yacht_amd.engine import RefDB

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON = 0xFFFFFFFF
POISON64 = 0xFFFFFFFFFFFFFFFF
LOOKUPS = (_lib.YH_LOOKUP_STREAM, _lib.YH_LOOKUP_INDEXED)


def dev(a):
    """A numpy array on the device, bit for bit (torch has no unsigned 32 / 64-bit types: signed views)."""
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize]).copy()).to(DEV)


def poison(*shape, wide=False):
    import torch

    return torch.full(shape, -1, dtype=torch.int64 if wide else torch.int32, device=DEV)


def u32(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32)


def u64(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def ready():
    """What torch queued (fills, copies into the gathered layouts) is complete before a handle's stream reads or overwrites it."""
    import torch

    torch.cuda.synchronize()


def sync(dbs):
    import torch

    torch.cuda.synchronize()
    for db in dbs:
        db.synchronize()


@contextlib.contextmanager
def refused(code):
    with pytest.raises(_lib.YachtHipError) as e:
        yield
    assert e.value.code == code, str(e.value)


class Shards:
    """One handle per rank over the ranks' CSR pieces (RefDB.from_device); at most 8 at a time."""

    def __init__(self, csrs):
        import torch

        assert len(csrs) <= 8
        self.keep = [(dev(v), dev(o)) for v, o in csrs]
        torch.cuda.synchronize()
        self.dbs = []
        for v, o in self.keep:
            self.dbs.append(RefDB.from_device(v.data_ptr(), o.data_ptr(), o.numel() - 1))

    def lookup(self, mode):
        for db in self.dbs:
            db.set_lookup(mode)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for db in self.dbs:
            db.close()


# ---- hash-range shards, one sample per step context ---------------------------------------------------------------------------------
def range_local(c, sh, s, ctx=0, smp_t=None):
    """First halves of sample s on every rank: per rank (overlap, n_match, bits) -- each equal to the builder's."""
    smp_t = dev(c.samples[s]) if smp_t is None else smp_t
    outs = []
    for g, db in enumerate(sh.dbs):
        a, b = c.spans[s][g]
        ov, m, bits = poison(c.n), poison(c.n), poison(c.W + 5)
        ready()
        db.run_local_range_device(smp_t.data_ptr() + 8 * a, b - a, ov.data_ptr(), m.data_ptr(), bits.data_ptr(), ctx)
        outs.append((ov, m, bits))
    sync(sh.dbs)
    for g, (ov, m, bits) in enumerate(outs):
        what = f"sample {s} rank {g} of {c.n_ranks} (N = {c.n}, slice of {c.spans[s][g][1] - c.spans[s][g][0]} hashes, ctx {ctx})"
        assert np.array_equal(u32(ov), c.share[s][g][0]), f"overlap share, {what}"
        assert np.array_equal(u32(m), c.share[s][g][2]), f"n_match share, {what}"
        got = u32(bits)
        assert np.array_equal(got[: c.W], c.bits[s][g]), f"bit row over its {c.W} words, {what}"
        assert (got[c.W:] == POISON).all(), f"words behind the bit row's extent were written, {what}"
    return outs


def gather_bits(c, outs, stride):
    """The ranks' rows `stride` words apart; what lies between them holds poison."""
    gathered = poison(c.n_ranks * stride + 2)
    for g, (_, _, bits) in enumerate(outs):
        gathered[g * stride: g * stride + c.W] = bits[: c.W]
    ready()
    return gathered


def range_finish(c, sh, s, outs, stride, ctx=0):
    gathered = gather_bits(c, outs, stride)
    ex = [poison(c.n) for _ in sh.dbs]
    ready()
    for g, db in enumerate(sh.dbs):
        db.run_finish_range_device(gathered.data_ptr(), c.n_ranks, stride, ex[g].data_ptr(), ctx)
    sync(sh.dbs)
    for g in range(c.n_ranks):
        assert np.array_equal(u32(ex[g]), c.share[s][g][1]), \
            f"n_excl share of sample {s}, rank {g} of {c.n_ranks} (N = {c.n}, stride {stride}, ctx {ctx}, its slice of the sample: {c.spans[s][g]})"
    for k, row in enumerate(([o[0] for o in outs], ex, [o[1] for o in outs])):
        assert np.array_equal(sum(u32(t).astype(np.int64) for t in row), c.whole[s][k]), f"row {k} summed over the ranks, sample {s}"


def range_steps(c, sh):
    for mode in LOOKUPS:
        sh.lookup(mode)
        for s in range(len(c.samples)):
            smp_t = dev(c.samples[s])
            for stride in (c.W, c.W + 3):
                range_finish(c, sh, s, range_local(c, sh, s, smp_t=smp_t), stride)


@pytest.mark.parametrize("n", sc.N_VALUES)
@pytest.mark.parametrize("n_ranks", sc.RANKS)
def test_range_halves_per_rank(hip_lib, n, n_ranks):
    """Both lookups, every sample of the case (a mixture, the empty one, one inside a single range -- every other rank's slice
    of it is empty --, one on the bounds), the natural stride and a larger one."""
    c = sc.range_case(n, n_ranks)
    with Shards(c.slices) as sh:
        range_steps(c, sh)


def test_range_halves_hand_made_bounds(hip_lib):
    """Three ranks, the middle one with six hashes in a few references: nearly all its cells are 'global subset, nothing here'."""
    c = sc.range_case(257, 3, hand=True)
    with Shards(c.slices) as sh:
        range_steps(c, sh)


def test_range_all_sixteen_contexts(hip_lib):
    """Sixteen first halves in contexts 0..15 on both ranks, one exchange, the second halves in reverse order."""
    c = sc.context_case()
    with Shards(c.slices) as sh:
        for mode in LOOKUPS:
            sh.lookup(mode)
            outs = [range_local(c, sh, k, ctx=k) for k in range(16)]
            for k in reversed(range(16)):
                range_finish(c, sh, k, outs[k], c.W, ctx=k)
        smp_t = dev(c.samples[0])
        ov, m, bits, ex = poison(c.n), poison(c.n), poison(c.W), poison(c.n)
        for ctx in (16, -1):
            with refused(_lib.YH_ERR_INVALID_ARG):
                sh.dbs[0].run_local_range_device(smp_t.data_ptr(), smp_t.numel(), ov.data_ptr(), m.data_ptr(), bits.data_ptr(), ctx)
            with refused(_lib.YH_ERR_INVALID_ARG):
                sh.dbs[0].run_finish_range_device(bits.data_ptr(), 1, c.W, ex.data_ptr(), ctx)
        sync(sh.dbs)
        assert (u32(ov) == POISON).all() and (u32(ex) == POISON).all()


def _finish_one(c, db, g, s, outs, ctx):
    """The second half of ONE rank; returns its n_excl."""
    gathered = gather_bits(c, outs, c.W)
    ex = poison(c.n)
    ready()
    db.run_finish_range_device(gathered.data_ptr(), c.n_ranks, c.W, ex.data_ptr(), ctx)
    sync([db])
    return u32(ex)


def _slice_counts(c, g, smp):
    """What a whole run step of a sample gives on rank g's handle alone (its own subset)."""
    v, o = c.slices[g]
    return sc.whole_counts(v, o, smp)[:3]


def test_range_clobber_detection(hip_lib):
    """The interleaving table of include/yacht_hip.h for an open step context."""
    c = sc.range_case(257, 2)
    with Shards(c.slices) as sh:
        db = sh.dbs[0]
        other_h = np.union1d(c.samples[0][::2], c.samples[3][1::2])
        other = dev(other_h)
        cnt = poison(3, c.n)

        def run_other(pipelined):
            if pipelined:
                db.run_device_pipelined(other.data_ptr(), other.numel(), cnt[0].data_ptr(), cnt[1].data_ptr(), cnt[2].data_ptr())
                db.run_device_join()
            else:
                db.run_device(other.data_ptr(), other.numel(), cnt[0].data_ptr(), cnt[1].data_ptr(), cnt[2].data_ptr())
            sync(sh.dbs)
            want = _slice_counts(c, 0, other_h)
            assert all(np.array_equal(u32(cnt[k]), want[k]) for k in range(3)), "the query in between"
            cnt.fill_(-1)
            ready()

        for mode in LOOKUPS:
            sh.lookup(mode)
            # another query in between: it re-uses the CURRENT context (1); context 0 is intact
            o0, o1 = range_local(c, sh, 0, ctx=0), range_local(c, sh, 3, ctx=1)
            run_other(pipelined=False)
            with refused(_lib.YH_ERR_INVALID_ARG):
                _finish_one(c, db, 0, 3, o1, 1)
            assert np.array_equal(_finish_one(c, db, 0, 0, o0, 0), c.share[0][0][1])
            assert np.array_equal(_finish_one(c, sh.dbs[1], 1, 3, o1, 1), c.share[3][1][1]), "the other rank's handle saw no other query"
            # after a refusal: a fresh pair of halves in the same context
            range_finish(c, sh, 3, range_local(c, sh, 3, ctx=1), c.W, ctx=1)
            # a pipelined call in between rotates through contexts 0..2 (or, where the split does not apply, runs as
            # yh_run_device in the current one, which is 1): context 5 is intact, context 1 is not
            o5, o1 = range_local(c, sh, 0, ctx=5), range_local(c, sh, 3, ctx=1)
            run_other(pipelined=True)
            assert np.array_equal(_finish_one(c, db, 0, 0, o5, 5), c.share[0][0][1])
            with refused(_lib.YH_ERR_INVALID_ARG):
                _finish_one(c, db, 0, 3, o1, 1)
            range_finish(c, sh, 3, range_local(c, sh, 3, ctx=1), c.W, ctx=1)


def test_range_context_survives_the_yes_rows(hip_lib):
    """abundance, explain and pairwise between the halves read and write no step state."""
    c = sc.range_case(257, 2)
    with Shards(c.slices) as sh:
        smp = c.samples[3]
        smp_t, ab_t = dev(smp), dev(np.ones(smp.size, dtype=np.uint32))
        member_t = dev(np.ones(c.n, dtype=np.uint8))
        for mode in LOOKUPS:
            sh.lookup(mode)
            outs = range_local(c, sh, 0, ctx=3)
            for g, db in enumerate(sh.dbs):
                w_ov, w_m, totals = poison(c.n, wide=True), poison(c.n, wide=True), poison(16, wide=True)
                ready()
                db.abundance_device(smp_t.data_ptr(), ab_t.data_ptr(), smp.size, w_ov.data_ptr(), w_m.data_ptr())
                db.explain_device(smp_t.data_ptr(), 0, smp.size, member_t.data_ptr(), 0, totals.data_ptr())
                db.pairwise(0.1)
                sync([db])
                want = _slice_counts(c, g, smp)
                assert np.array_equal(u64(w_ov), want[0]) and np.array_equal(u64(w_m), want[2])
                assert int(u64(totals)[0]) == int(np.isin(smp, c.slices[g][0]).sum())
            range_finish(c, sh, 0, outs, c.W, ctx=3)


# ---- reference shards with ghosts -----------------------------------------------------------------------------------------------------
class GhostShards(Shards):
    def __init__(self, c):
        super().__init__([(r.values, r.offsets) for r in c.ranks])
        self.src = [dev(r.ghost_src) for r in c.ranks]
        sync(self.dbs)
        for db, r, src in zip(self.dbs, c.ranks, self.src):
            db.set_ghosts(r.ghost_begin, r.n_ghost, src.data_ptr())


def ghost_step(c, sh, s, ctx=0):
    smp_t = dev(c.samples[s])
    w_ov, w_e, w_m = c.whole[s]
    outs = []
    for db, r in zip(sh.dbs, c.ranks):
        ov, ex, m, bits = poison(r.n_rows), poison(r.n_rows), poison(r.n_rows), poison(r.out_words + 5)
        ready()
        db.run_local_device(smp_t.data_ptr(), smp_t.numel(), ov.data_ptr(), ex.data_ptr(), m.data_ptr(), bits.data_ptr(), ctx)
        outs.append((ov, ex, m, bits))
    sync(sh.dbs)
    # the layout this test gathers: W words per rank, rank q's local reference i at bit q * W * 32 + i; what a row holds
    # behind its local references is not valid by contract -- ones here, so that a ghost reading there shows
    flags = np.ones((c.n_ranks, c.W * 32), dtype=np.uint8)
    for q, (r, (ov, ex, m, bits)) in enumerate(zip(c.ranks, outs)):
        what = f"sample {s} rank {q} of {c.n_ranks} ({r.n_local} local references, {r.n_ghost} ghosts from row {r.ghost_begin})"
        assert np.array_equal(u32(ov)[: r.n_local], w_ov[r.begin: r.end]), f"overlap, {what}"
        assert np.array_equal(u32(m)[: r.n_local], w_m[r.begin: r.end]), f"n_match, {what}"
        got = u32(bits)
        assert (got[r.out_words:] == POISON).all(), f"words behind the bit row's extent were written, {what}"
        row = np.unpackbits(got[: r.out_words].view(np.uint8), bitorder="little")
        assert np.array_equal(row[: r.n_local] != 0, w_ov[r.begin: r.end] > 0), f"subset bits of the local references, {what}"
        assert not row[r.n_rows:].any(), f"bits behind the handle's references, {what}"
        flags[q, : r.n_local] = row[: r.n_local]
    gathered = dev(np.packbits(flags, axis=1, bitorder="little").view("<u4").astype(np.uint32))
    for db, (ov, ex, m, bits) in zip(sh.dbs, outs):
        db.run_finish_device(gathered.data_ptr(), ex.data_ptr(), ctx)
    sync(sh.dbs)
    for q, (r, (ov, ex, m, bits)) in enumerate(zip(c.ranks, outs)):
        assert np.array_equal(u32(ex)[: r.n_local], w_e[r.begin: r.end]), \
            f"n_excl, sample {s} rank {q} of {c.n_ranks} ({r.n_local} local references, {r.n_ghost} ghosts from row {r.ghost_begin})"


def ghost_steps(c):
    with GhostShards(c) as sh:
        for mode in LOOKUPS:
            sh.lookup(mode)
            for s in range(len(c.samples)):
                ghost_step(c, sh, s, ctx=(5 * s + mode) % 16)


@pytest.mark.parametrize("n_ranks", sc.GHOST_RANKS)
def test_ghost_halves_cuts_through_clusters(hip_lib, n_ranks):
    """Every rank has ghosts; the first and the last rank also hold one reference each of a pair that shares three hashes no
    sample holds (samples 3 and 4: the pair's other member outside and inside the subset)."""
    ghost_steps(sc.ghost_clustered_case(n_ranks))


@pytest.mark.parametrize("n_local0,n_ghost0", sc.GHOST_EDGES)
def test_ghost_halves_at_the_edges_of_the_ghost_range(hip_lib, n_local0, n_ghost0):
    """No padding in front of the ghosts / 63 padding rows; 1, 64 and 65 ghosts (a partial last pair of words); samples 0 and 1:
    the owner of ghost 0 outside and inside the subset -- ghost bits that are ignored fail the one, always set the other."""
    ghost_steps(sc.ghost_edge_case(n_local0, n_ghost0))


def test_ghost_argument_checks(hip_lib):
    c = sc.ghost_edge_case(64, 1)
    r = c.ranks[0]
    with GhostShards(c) as sh:
        db = sh.dbs[0]
        for begin, count in ((r.ghost_begin + 1, 0), (r.ghost_begin - 32, r.n_ghost), (r.ghost_begin, r.n_ghost + 1), (r.ghost_begin + 64, 1)):
            with refused(_lib.YH_ERR_INVALID_ARG):
                db.set_ghosts(begin, count, sh.src[0].data_ptr())
        smp = c.samples[1]
        smp_t = dev(smp)
        ov, m, bits = poison(r.n_rows), poison(r.n_rows), poison(r.out_words)
        with refused(_lib.YH_ERR_INVALID_ARG):
            db.run_local_range_device(smp_t.data_ptr(), smp.size, ov.data_ptr(), m.data_ptr(), bits.data_ptr(), 0)
        with refused(_lib.YH_ERR_UNSUPPORTED):
            db.abundance(smp, np.ones(smp.size, dtype=np.uint32))
        with refused(_lib.YH_ERR_UNSUPPORTED):
            db.explain(smp, np.ones(r.n_rows, dtype=np.uint8))
        for s in (0, 1):  # the refused registrations changed nothing
            ghost_step(c, sh, s)


# ---- a block of samples per batch slot ------------------------------------------------------------------------------------------------------
def batch_local(c, sh, slot=0):
    outs = []
    pn = c.P * c.n
    for g, db in enumerate(sh.dbs):
        cat, soff = dev(c.cat[g]), dev(c.soff[g])
        ov, words = poison(c.B, c.n), poison(pn + 3, wide=True)
        ready()
        db.run_batch_local_range_device(cat.data_ptr(), soff.data_ptr(), c.B, int(c.cat[g].size), ov.data_ptr(), words.data_ptr(), slot)
        outs.append((ov, words, cat, soff))
    sync(sh.dbs)
    for g, (ov, words, _, _) in enumerate(outs):
        what = f"rank {g} of {c.n_ranks}, {c.B} samples ({int(c.cat[g].size)} hashes in its range), slot {slot}"
        assert np.array_equal(u32(ov), c.rows[g][0]), f"overlap shares, {what}"
        got = u64(words)
        assert np.array_equal(got[:pn].reshape(c.P, c.n), c.words[g]), f"subset words [P][N], {what}"
        assert (got[pn:] == POISON64).all(), f"words behind [P][N] were written, {what}"
    return outs


def batch_finish(c, sh, outs, slot=0, gathered=None):
    """gathered: one tensor per rank that is ALREADY the OR (the packed route: n_ranks = 1); default: the dense [R][P][N]."""
    import torch

    pn = c.P * c.n
    dense = torch.stack([w[:pn] for _, w, _, _ in outs]).contiguous()
    res = []
    for g, db in enumerate(sh.dbs):
        e, m = poison(c.B, c.n), poison(c.B, c.n)
        src, n_ranks = (dense, c.n_ranks) if gathered is None else (gathered[g], 1)
        ready()
        db.run_batch_finish_range_device(c.B, src.data_ptr(), n_ranks, outs[g][0].data_ptr(), e.data_ptr(), m.data_ptr(), slot)
        res.append((outs[g][0], e, m))
    sync(sh.dbs)
    for g, (ov, e, m) in enumerate(res):
        what = f"rank {g} of {c.n_ranks}, {c.B} samples, slot {slot}"
        assert np.array_equal(u32(e), c.rows[g][1]), f"n_excl shares, {what}"
        assert np.array_equal(u32(m), c.rows[g][2]), f"n_match shares, {what}"
        assert np.array_equal(u32(ov), c.rows[g][0]), f"overlap shares after the second half, {what}"
    for k in range(3):
        assert np.array_equal(sum(u32(r[k]).astype(np.int64) for r in res), c.whole_rows[k]), f"row {k} summed over the ranks"
    return res


@pytest.mark.parametrize("n_ranks,n_samples", sc.BATCH_SHAPES)
def test_batch_halves_per_rank(hip_lib, n_ranks, n_samples):
    c = sc.batch_case(n_ranks, n_samples)
    with Shards(c.slices) as sh:
        batch_finish(c, sh, batch_local(c, sh))
        batch_finish(c, sh, batch_local(c, sh, slot=2), slot=2)  # (again: what the first pass left in the handle is clean)


def test_batch_rank_without_a_hit(hip_lib):
    """Every sample lies in rank 0's range: rank 1 gets total_hashes = 0 and all offsets equal, and owes n_excl for every cell."""
    c = sc.batch_case(*sc.BATCH_NO_HITS)
    with Shards(c.slices) as sh:
        batch_finish(c, sh, batch_local(c, sh, slot=1), slot=1)


def _nonzero_words(c):
    return [int((c.words[g] != 0).sum()) for g in range(c.n_ranks)]


def test_batch_packed_words_route(hip_lib):
    """Three planes from three ranks through yh_run_batch_words_pack_device / _unpack_device, then the second half with n_ranks = 1."""
    c = sc.batch_case(*sc.BATCH_PACKED)
    assert c.P == 3 and c.n_ranks == 3
    counts = _nonzero_words(c)
    pn = c.P * c.n
    want_or = c.global_words.ravel()
    with Shards(c.slices) as sh:
        outs = batch_local(c, sh)
        for cap, overflow in ((max(counts), 0), (max(counts) - 1, 1)):
            length = int(hip_lib.yh_run_batch_words_packed_len(cap))
            assert length == 1 + cap + (cap + 1) // 2
            packed = poison(c.n_ranks, length, wide=True)
            ready()
            for g, db in enumerate(sh.dbs):
                db.run_batch_words_pack_device(outs[g][1].data_ptr(), packed[g].data_ptr(), cap, n_planes=c.P)
            sync(sh.dbs)
            assert [int(x) for x in u64(packed[:, 0])] == counts, "word [0] of every rank's buffer is its true count"
            ored, flag = [], []
            for db in sh.dbs:
                ored.append(poison(pn, wide=True))
                flag.append(poison(1))
                ready()
                db.run_batch_words_unpack_device(packed.data_ptr(), c.n_ranks, cap, ored[-1].data_ptr(), flag[-1].data_ptr(), n_planes=c.P)
            sync(sh.dbs)
            assert [int(u32(f)[0]) for f in flag] == [overflow] * c.n_ranks, f"overflow flag at capacity {cap} (largest rank {max(counts)})"
            if not overflow:
                for g in range(c.n_ranks):
                    assert np.array_equal(u64(ored[g]), want_or), f"OR of the packed words on rank {g}"
                batch_finish(c, sh, outs, gathered=ored)
            else:
                assert all(((u64(o) | want_or) == want_or).all() for o in ored), "an incomplete OR holds no bit of its own"


def test_batch_slots(hip_lib):
    """All three slots open at once, finished out of order; what a second half is refused for; an abandoned first half."""
    cases = [sc.batch_case(*k) for k in sc.BATCH_SLOTS]
    big, small = (sc.batch_case(*k) for k in sc.BATCH_ABANDONED)
    with Shards(cases[0].slices) as sh:
        outs = [batch_local(c, sh, slot=k) for k, c in enumerate(cases)]
        for k in (2, 0, 1):
            batch_finish(cases[k], sh, outs[k], slot=k)
        a, b = cases[0], cases[1]

        def second_half(c, out, g, slot, n_samples=None):
            e, m = poison(c.B, c.n), poison(c.B, c.n)
            ready()
            sh.dbs[g].run_batch_finish_range_device(c.B if n_samples is None else n_samples, out[g][1].data_ptr(), 1, out[g][0].data_ptr(),
                                                    e.data_ptr(), m.data_ptr(), slot)

        # a different number of samples; the same second half twice; no such slot
        out = batch_local(a, sh, slot=0)
        with refused(_lib.YH_ERR_INVALID_ARG):
            second_half(a, out, 0, 0, n_samples=a.B - 1)
        out = batch_local(a, sh, slot=0)
        batch_finish(a, sh, out, slot=0)
        with refused(_lib.YH_ERR_INVALID_ARG):
            second_half(a, out, 0, 0)
        with refused(_lib.YH_ERR_INVALID_ARG):
            second_half(a, out, 0, 3)
        with refused(_lib.YH_ERR_INVALID_ARG):
            sh.dbs[0].run_batch_local_range_device(out[0][2].data_ptr(), out[0][3].data_ptr(), a.B, int(a.cat[0].size), out[0][0].data_ptr(),
                                                   out[0][1].data_ptr(), 3)
        # yh_run_batch_device runs in slot 0: a first half there is gone, the one in slot 1 is not
        out_a, out_b = batch_local(a, sh, slot=0), batch_local(b, sh, slot=1)
        for g, db in enumerate(sh.dbs):
            cnt = poison(3, small.B, small.n)
            cat, soff = dev(small.cat[g]), dev(small.soff[g])
            ready()
            db.run_batch_device(cat.data_ptr(), soff.data_ptr(), small.B, int(small.cat[g].size), cnt[0].data_ptr(), cnt[1].data_ptr(), cnt[2].data_ptr())
            sync([db])
            v, o = small.slices[g]
            for s in range(small.B):
                want = sc.whole_counts(v, o, small.samples[s])[:3]
                assert all(np.array_equal(u32(cnt[k][s]), want[k]) for k in range(3)), f"yh_run_batch_device on rank {g}'s handle, sample {s}"
            with refused(_lib.YH_ERR_INVALID_ARG):
                second_half(a, out_a, g, 0)
        batch_finish(b, sh, out_b, slot=1)
        # 200 samples that never get their second half, then 3 samples in the same slot
        batch_local(big, sh, slot=2)
        batch_finish(small, sh, batch_local(small, sh, slot=2), slot=2)


def test_batch_compact_rows_over_ranks(hip_lib):
    """rows pack on every rank, the value arrays summed as they are, rows unpack on rank 0."""
    c = sc.batch_case(3, 130)
    want = sc.compact_rows(c)
    k = want.shape[0]
    cap = k + 7
    with Shards(c.slices) as sh:
        res = batch_finish(c, sh, batch_local(c, sh, slot=1), slot=1)
        vals, n_rows = [], []
        for db, (ov, e, m) in zip(sh.dbs, res):
            vals.append(poison(cap, 3))
            n_rows.append(poison(1))
            ready()
            db.run_batch_rows_pack_device(ov.data_ptr(), e.data_ptr(), m.data_ptr(), vals[-1].data_ptr(), cap, n_rows[-1].data_ptr(), slot=1)
        sync(sh.dbs)
        assert [int(u32(x)[0]) for x in n_rows] == [k] * c.n_ranks, "every rank reports the global subset's entries"
        assert all((u32(v)[k:] == POISON).all() for v in vals)
        total = sum(v[:k] for v in vals)
        padded = poison(cap, 3)
        padded[:k] = total
        rows, n2 = poison(cap, 5), poison(1)
        ready()
        sh.dbs[0].run_batch_rows_unpack_device(padded.data_ptr(), cap, rows.data_ptr(), n2.data_ptr(), slot=1)
        sync(sh.dbs)
        assert int(u32(n2)[0]) == k
        assert np.array_equal(u32(rows)[:k], want), "the rows: the non-zero cells of the oracle's dense rows in (reference, sample) order"
        assert (u32(rows)[k:] == POISON).all()


def test_batch_halves_with_a_finish_stream(hip_lib):
    """The multi-rank, multi-plane case again with the second halves on a second stream (the host still waits between them)."""
    import torch

    c = sc.batch_case(*sc.BATCH_PACKED)
    second = torch.cuda.Stream()
    with Shards(c.slices) as sh:
        try:
            for db in sh.dbs:
                db.set_batch_finish_stream(second.cuda_stream)
            for slot in (0, 1):
                batch_finish(c, sh, batch_local(c, sh, slot=slot), slot=slot)
        finally:
            for db in sh.dbs:
                db.set_batch_finish_stream(None)
        batch_finish(c, sh, batch_local(c, sh))


# ---- a handle over N references without a single hash ---------------------------------------------------------------------------------------
def test_all_empty_handle_in_the_range_entry_points(hip_lib):
    """What include/yacht_hip.h says about an all-empty hash-range shard: the single-sample first half is YH_ERR_UNSUPPORTED, the
    other three entries succeed with all-zero shares -- whatever the other ranks put into the subset."""
    n, n_samples = 65, 70
    w = sc.bit_words(n)
    planes = (n_samples + 63) // 64
    with Shards([(sc.EMPTY, np.zeros(n + 1, dtype=np.uint64))]) as sh:
        db = sh.dbs[0]
        assert db.info()["n_hashes"] == 0 and db.info()["n_refs"] == n
        smp_t = dev(np.arange(1, 40, dtype=np.uint64))
        ov, m, bits, ex = poison(n), poison(n), poison(w), poison(n)
        with refused(_lib.YH_ERR_UNSUPPORTED):
            db.run_local_range_device(smp_t.data_ptr(), smp_t.numel(), ov.data_ptr(), m.data_ptr(), bits.data_ptr(), 2)
        sync(sh.dbs)
        assert (u32(ov) == POISON).all() and (u32(m) == POISON).all() and (u32(bits) == POISON).all(), "the refused half wrote"
        others = dev(np.full(2 * w, 0x5A5A5A5A, dtype=np.uint32))  # two other ranks' rows
        db.run_finish_range_device(others.data_ptr(), 2, w, ex.data_ptr(), 2)
        sync(sh.dbs)
        assert not u32(ex).any()
        soff = dev(np.minimum(np.arange(n_samples + 1, dtype=np.uint64), 39))
        b_ov, words = poison(n_samples, n), poison(planes * n, wide=True)
        db.run_batch_local_range_device(smp_t.data_ptr(), soff.data_ptr(), n_samples, 39, b_ov.data_ptr(), words.data_ptr(), 1)
        sync(sh.dbs)
        assert not u32(b_ov).any() and not u64(words).any()
        gathered = dev(np.full(2 * planes * n, 0x00FF00FF00FF00FF, dtype=np.uint64))
        b_e, b_m = poison(n_samples, n), poison(n_samples, n)
        db.run_batch_finish_range_device(n_samples, gathered.data_ptr(), 2, b_ov.data_ptr(), b_e.data_ptr(), b_m.data_ptr(), 1)
        sync(sh.dbs)
        assert not u32(b_e).any() and not u32(b_m).any() and not u32(b_ov).any()
