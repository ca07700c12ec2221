"""Guards tests/shard_cases.py, the reference of tests/test_gpu_shard_halves.py, without a GPU: for every case the device
tests use, the per-rank shares the builder expects add up to the whole-database oracle, the OR of the ranks' bit rows is the
global subset, the ghosts hold only hashes their rank holds, and the cases still contain the edges they are named for."""
import numpy as np
import pytest

import shard_cases as sc
from oracle import oracle


def _check_shares(c):
    for s, smp in enumerate(c.samples):
        ov, e, m = c.whole[s]
        if c.n <= 65:
            assert np.array_equal(ov, oracle.overlap_py(c.values, c.offsets, smp))
        for k, name in enumerate(("overlap", "n_excl", "n_match")):
            tot = sum(c.share[s][g][k].astype(np.int64) for g in range(c.n_ranks))
            assert np.array_equal(tot, c.whole[s][k]), f"sample {s}: the ranks' shares of {name} do not sum to the oracle"
        acc = np.bitwise_or.reduce(np.stack(c.bits[s]), axis=0)
        assert acc.size == ((c.n + 255) // 256) * 8
        assert np.array_equal(acc, sc.bit_row(ov > 0, c.W)), f"sample {s}: OR of the bit rows is not the global subset"
        for g, (a, b) in enumerate(c.spans[s]):
            part = smp[a:b]
            assert np.array_equal(part, sc.in_range(smp, c.bounds[g], c.bounds[g + 1]))
        assert sum(b - a for a, b in c.spans[s]) == smp.size and all(c.spans[s][g][1] == c.spans[s][g + 1][0] for g in range(c.n_ranks - 1))


@pytest.mark.parametrize("n", sc.N_VALUES)
@pytest.mark.parametrize("n_ranks", sc.RANKS)
def test_range_shares_sum_to_the_oracle(n, n_ranks):
    c = sc.range_case(n, n_ranks)
    assert c.n == n and len(c.slices) == n_ranks
    _check_shares(c)
    sizes = np.diff(c.offsets)
    if n >= 8:
        assert (sizes == 0).sum() >= 1 and (sizes == 1).sum() >= 1 and sizes.min() == 0 and 40 <= np.median(sizes) <= 310
        assert np.array_equal(c.refs[2], c.refs[n // 3]), "two references that share every hash"
    # the samples: a mixture, the empty one, one inside a single range, one on the bounds (which the database holds too)
    assert c.samples[1].size == 0
    spans = c.spans[2]
    assert sum(1 for a, b in spans if b > a) == 1 and c.samples[2].size > 0
    everything = set(int(x) for x in c.values)
    for lo in c.bounds[1:-1]:
        assert lo in everything and lo - 1 in everything
        assert lo in set(int(x) for x in c.samples[3]) and lo - 1 in set(int(x) for x in c.samples[3])
    if n_ranks > 1 and n > 1:  # some cell is in the global subset with no hit of this rank -- what a sum over one rank never has
        assert any(((c.whole[s][0] > 0) & (c.share[s][g][0] == 0)).any() for s in range(len(c.samples)) for g in range(n_ranks))
    if n_ranks > 1:  # a rank whose slice of a non-empty sample is empty
        assert any(b == a for a, b in c.spans[2])


def test_hand_made_bounds_leave_one_rank_a_few_references():
    c = sc.range_case(257, 3, hand=True)
    _check_shares(c)
    v, o = c.slices[1]
    assert 1 <= (np.diff(o) > 0).sum() <= 24 and np.unique(v).size <= 8


def test_context_case():
    c = sc.context_case()
    assert len(c.samples) == 16 and c.n_ranks == 2
    _check_shares(c)
    assert len({s.tobytes() for s in c.samples}) == 16


def _check_batch(c):
    _check_shares(c)
    assert np.array_equal(np.bitwise_or.reduce(np.stack(c.words), axis=0), c.global_words)
    for g in range(c.n_ranks):
        assert c.words[g].shape == (c.P, c.n) and c.soff[g].size == c.B + 1 and int(c.soff[g][-1]) == c.cat[g].size
        for s in (0, c.B - 1):
            got = (c.words[g][s >> 6] >> np.uint64(s & 63)) & np.uint64(1)
            assert np.array_equal(got.astype(bool), c.rows[g][0][s] > 0)
    for k in range(3):
        assert np.array_equal(sum(c.rows[g][k].astype(np.int64) for g in range(c.n_ranks)), c.whole_rows[k])


@pytest.mark.parametrize("n_ranks,n_samples", sc.BATCH_SHAPES)
def test_batch_shares_sum_to_the_oracle(n_ranks, n_samples):
    c = sc.batch_case(n_ranks, n_samples)
    _check_batch(c)
    if n_samples > 5:
        assert c.samples[3].size == 0 and np.array_equal(c.samples[4], c.samples[5]) and c.samples[4].size
        assert all(b == a for a, b in c.spans[1][1:]) and c.samples[1].size
    rows = sc.compact_rows(c)
    assert rows.shape[0] == int((c.whole_rows[0] > 0).sum())
    assert np.array_equal(np.lexsort((rows[:, 0], rows[:, 1])), np.arange(rows.shape[0])), "(reference, sample) order"


@pytest.mark.parametrize("key", (sc.BATCH_NO_HITS, sc.BATCH_PACKED) + sc.BATCH_SLOTS + sc.BATCH_ABANDONED)
def test_batch_cases_of_the_slot_and_route_tests(key):
    c = sc.batch_case(*key)
    _check_batch(c)
    if key == sc.BATCH_NO_HITS:  # every sample inside rank 0's range: rank 1 looks nothing up, over a database that has hashes there
        assert c.cat[1].size == 0 and not c.soff[1].any() and c.slices[1][0].size > 0
        assert not c.rows[1][0].any() and c.rows[1][1].any(), "rank 1: global subset, zero local hits, yet a share of n_excl"


@pytest.mark.parametrize("n_ranks", sc.GHOST_RANKS)
def test_ghost_clustered_case(n_ranks):
    c = sc.ghost_clustered_case(n_ranks)
    _check_ghosts(c)
    assert all(r.n_ghost > 0 for r in c.ranks), "every cut goes through a cluster"
    if n_ranks == 2:  # a ghost whose owner's bit sits in the last word of the owner's row
        assert any(int(s) % (c.W * 32) >= (c.W - 1) * 32 for s in c.ranks[0].ghost_src)
    # the pair made by hand: the last reference is a ghost of the first rank and the other way round; it overlaps sample 4
    # only, and in neither sample through the hashes it shares -- so its own overlap as a ghost is zero in both
    last = c.n - 1
    assert c.ranks[0].ghost_ids[-1] == last and c.ranks[-1].ghost_ids[0] == 0 and c.common.size == 3
    assert not np.intersect1d(c.samples[3], c.common).size and not np.intersect1d(c.samples[4], c.common).size
    assert c.whole[3][0][0] > 0 and c.whole[3][0][last] == 0 and c.whole[4][0][last] > 0
    assert int(c.whole[3][1][0]) - int(c.whole[4][1][0]) == 3, "the shared hashes: exclusive to reference 0 in sample 3 only"


def _check_ghosts(c):
    assert c.W == max((r.n_local + 31) // 32 for r in c.ranks)
    for q, r in enumerate(c.ranks):
        assert r.ghost_begin % 64 == 0 and r.ghost_begin - r.n_local < 64 and r.n_rows == r.ghost_begin + r.n_ghost
        rows = [r.values[int(r.offsets[j]):int(r.offsets[j + 1])] for j in range(r.n_rows)]
        local = set(int(x) for j in range(r.n_local) for x in rows[j])
        assert all(rows[j].size == 0 for j in range(r.n_local, r.ghost_begin)), "padding: empty references"
        assert r.ghost_ids == sorted(r.ghost_ids) and not any(r.begin <= f < r.end for f in r.ghost_ids)
        for k, f in enumerate(r.ghost_ids):
            h = rows[r.ghost_begin + k]
            assert h.size and np.all(h[1:] > h[:-1]) and all(int(x) in local for x in h), "a ghost holds only hashes its rank holds"
            assert np.array_equal(h, np.intersect1d(c.refs[f], np.array(sorted(local), dtype=np.uint64)))
            own = next(p for p in range(c.n_ranks) if c.cuts[p] <= f < c.cuts[p + 1])
            assert int(r.ghost_src[k]) == own * c.W * 32 + (f - c.cuts[own]) and own != q
        # a foreign reference that is no ghost shares nothing with this rank
        for f in range(c.n):
            if not r.begin <= f < r.end and f not in r.ghost_ids:
                assert not local.intersection(int(x) for x in c.refs[f])
    for s, smp in enumerate(c.samples):
        ov, e, m = c.whole[s]
        w_ov, w_e, w_m, _ = sc.whole_counts(c.values, c.offsets, smp)
        assert np.array_equal(ov, w_ov) and np.array_equal(e, w_e) and np.array_equal(m, w_m)


@pytest.mark.parametrize("n_local0,n_ghost0", sc.GHOST_EDGES)
def test_ghost_edge_case(n_local0, n_ghost0):
    c = sc.ghost_edge_case(n_local0, n_ghost0)
    _check_ghosts(c)
    r0 = c.ranks[0]
    assert r0.n_local == n_local0 and r0.n_ghost == n_ghost0 and r0.ghost_begin == ((n_local0 + 63) // 64) * 64
    # the two directions of ghost 0's bit: its owner (the first reference of rank 1) overlaps sample 1 only; the hashes
    # reference 0 shares with it are exclusive to reference 0 in sample 0 and to nobody in sample 1
    owner = c.cuts[1]
    assert r0.ghost_ids[0] == owner and c.shared0.size == 2
    assert c.whole[0][0][0] > 0 and c.whole[0][0][owner] == 0 and c.whole[1][0][owner] > 0
    assert int(c.whole[0][1][0]) - int(c.whole[1][1][0]) == c.shared0.size
    assert not np.intersect1d(c.samples[1], c.shared0).size


def test_builder_agrees_with_the_set_backend():
    """The per-rank expectations against the set-based restatement of the two calls that tests/test_dist_range_cpu.py drives
    dist.HashRangeRefDB with: first half, OR of the gathered rows at a stride, second half -- for every rank of one case."""
    import torch

    from test_dist_range_cpu import SetRangeBackend

    c = sc.range_case(65, 3)
    stride = c.W + 3
    locs = [SetRangeBackend().make_range_db(torch.from_numpy(v.view(np.int64).copy()), torch.from_numpy(o.astype(np.int64)))
            for v, o in c.slices]
    for s, smp in enumerate(c.samples):
        st = torch.from_numpy(smp.view(np.int64).copy())
        counts, gathered = [], torch.zeros(c.n_ranks * stride, dtype=torch.int32)
        for g, loc in enumerate(locs):
            cnt = torch.zeros((3, c.n), dtype=torch.int32)
            bits = torch.zeros(c.W, dtype=torch.int32)
            loc.run_local(st, c.spans[s][g][0], c.spans[s][g][1], cnt, bits)
            assert np.array_equal(bits.numpy().view(np.uint32), c.bits[s][g])
            gathered[g * stride: g * stride + c.W] = bits
            counts.append(cnt)
        for g, loc in enumerate(locs):
            loc.run_finish(gathered, c.n_ranks, stride, counts[g])
            got = counts[g].numpy().view(np.uint32)
            for k in range(3):
                assert np.array_equal(got[k], c.share[s][g][k]), f"sample {s} rank {g} row {k}"
