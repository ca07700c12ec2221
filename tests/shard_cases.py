"""Case builder for the two halves of the sharded `yacht run` step (include/yacht_hip.h: yh_run_local*_device /
yh_run_finish*_device, yh_run_batch_local_range_device / _finish_range_device), numpy only: small clustered databases at the
reference counts where the 64-lane ballots and 256-reference blocks of the subset bits end, the samples that ask them, the
per-rank pieces a sharded run works on -- hash-range slices, or reference shards with their ghosts -- and, for EVERY RANK ON ITS
OWN, what the two halves must leave.  Shared by tests/test_shard_cases_cpu.py (which guards that the shares add up to the
whole-database oracle) and tests/test_gpu_shard_halves.py (which runs them on the device, R handles in one process).

Every expected count comes from oracle.overlap / oracle.exclusive: on the whole database for the totals, on a rank's slice
with the GLOBAL subset for its shares (all holders of a hash sit on one rank, so exclusivity is rank-local once the subset
is the global one).  Nothing here calls the library.
"""
import functools
from types import SimpleNamespace

import numpy as np

from oracle import oracle
from yacht_amd import dist as ydist
from yacht_amd import synth

N_VALUES = (1, 63, 64, 65, 255, 256, 257, 700)   # around the 64-lane ballots and the 256-reference blocks of the bit rows
RANKS = (1, 2, 3, 5, 8)
GHOST_RANKS = (2, 3, 5)
GHOST_EDGES = ((64, 1), (65, 64), (128, 65))     # (local references of rank 0, its ghosts): no padding / n_local % 64 == 1
BATCH_SHAPES = tuple((r, b) for r in (2, 3) for b in (1, 64, 65, 130, 256))
BATCH_N = 257
# batch_case keys of the tests that are no shape sweep: (ranks, samples, rank that holds ALL samples or None, seed)
BATCH_NO_HITS = (2, 130, 0)            # every sample inside rank 0's range: rank 1 has no hash to look up in the whole block
BATCH_PACKED = (3, 130, None, 1)       # three word planes from three ranks
BATCH_SLOTS = ((2, 65, None, 2), (2, 3, None, 3), (2, 130, None, 4))   # one block per batch slot, open at the same time
BATCH_ABANDONED = ((2, 200, None, 5), (2, 3, None, 6))                 # a first half that is never finished, then a smaller block
RETENTIONS = (1.0, 0.9, 0.5, 0.25, 0.1)
U64 = np.uint64
EMPTY = np.zeros(0, dtype=U64)


def bit_words(n_refs: int) -> int:
    """32-bit words of one row of subset bits: whole 256-reference blocks."""
    return ((n_refs + 255) // 256) * 8


def bit_row(flags, n_words: int) -> np.ndarray:
    """flags[j] != 0 as bit j & 31 of word j >> 5 (little-endian within the 32-bit words), zero behind the flags."""
    b = np.zeros(n_words * 32, dtype=np.uint8)
    b[: len(flags)] = np.asarray(flags) != 0
    return np.packbits(b, bitorder="little").view("<u4").astype(np.uint32)


def subset_words(overlaps) -> np.ndarray:
    """[P][N] uint64 of a block's overlap rows [B][N]: plane s >> 6, bit s & 63 = sample s overlaps the reference."""
    overlaps = np.asarray(overlaps)
    n_samples, n = overlaps.shape
    words = np.zeros(((n_samples + 63) // 64, n), dtype=U64)
    for s in range(n_samples):
        words[s >> 6] |= (overlaps[s] > 0).astype(U64) << U64(s & 63)
    return words


def whole_counts(values, offsets, sample):
    """(overlap, n_excl, n_match, subset) of the whole database, subset = overlap > 0."""
    ov = oracle.overlap(values, offsets, sample)
    mask = ov > 0
    e, m = oracle.exclusive(values, offsets, mask, sample)
    return ov, e, m, mask


# ---- databases --------------------------------------------------------------------------------------------------------------
def clustered(rng, n: int):
    """n references in clusters of five (sketches of 40..300 hashes, many shared inside a cluster)."""
    refs = []
    while len(refs) < n:
        refs += synth.clustered_refs(rng, 1, RETENTIONS, int(rng.integers(40, 301)))
    return refs[:n]


def make_refs(n: int, seed: int = 0):
    """n references: clusters, plus -- from 8 references on -- a copy of reference 2 (two references that share every hash), an
    empty reference and a one-hash reference (the first hash of reference 0)."""
    rng = np.random.default_rng(9000 + 13 * n + seed)
    if n < 8:
        return [r.copy() for r in synth.clustered_refs(rng, 1, (1.0,) + RETENTIONS[1:n], 300)]
    refs = clustered(rng, n - 3)
    refs.insert(n // 3, refs[2].copy())
    refs.insert(n // 2, EMPTY.copy())
    refs.insert((2 * n) // 3, refs[0][:1].copy())
    assert len(refs) == n
    return refs


def slice_of(sample: np.ndarray, lo: int, hi: int):
    """[a, b): the positions of the sorted sample's hashes in [lo, hi) (hi = 2**64: no upper end)."""
    a = int(np.searchsorted(sample, U64(lo), side="left"))
    b = int(np.searchsorted(sample, U64(hi), side="left")) if hi < 2 ** 64 else int(sample.size)
    return a, b


def in_range(a: np.ndarray, lo: int, hi: int) -> np.ndarray:
    keep = a >= U64(lo)
    if hi < 2 ** 64:
        keep &= a < U64(hi)
    return a[keep]


# ---- hash-range shards --------------------------------------------------------------------------------------------------------
def range_shares(values, offsets, bounds, samples):
    """The per-rank pieces and expectations of hash-range shards for a list of samples."""
    n = offsets.size - 1
    n_ranks = len(bounds) - 1
    w = bit_words(n)
    slices = [ydist.slice_csr_to_hash_range(values, offsets, bounds[g], bounds[g + 1]) for g in range(n_ranks)]
    c = SimpleNamespace(n=n, n_ranks=n_ranks, W=w, values=values, offsets=offsets, bounds=list(bounds), slices=slices,
                        samples=samples, spans=[], whole=[], share=[], bits=[])
    for smp in samples:
        ov, e, m, mask = whole_counts(values, offsets, smp)
        c.whole.append((ov, e, m))
        c.spans.append([slice_of(smp, bounds[g], bounds[g + 1]) for g in range(n_ranks)])
        sh = []
        for v_g, o_g in slices:
            ov_g = oracle.overlap(v_g, o_g, smp)
            e_g, m_g = oracle.exclusive(v_g, o_g, mask, smp)
            sh.append((ov_g, e_g, m_g))
        c.share.append(sh)
        c.bits.append([bit_row(x[0] > 0, w) for x in sh])
    return c


def _samples_for(rng, refs, bounds, n_noise=150):
    """A mixture, the empty sample, a sample wholly inside one rank's range, and one that sits on the bounds."""
    n = len(refs)
    n_ranks = len(bounds) - 1
    present = sorted(set(int(x) for x in rng.choice(n, size=min(n, 9), replace=False)) | {0, min(2, n - 1), n // 3, (2 * n) // 3})
    mix = synth.sample_from_refs(rng, refs, present, 0.6, 0)
    mix = np.union1d(mix, rng.integers(0, synth.max_hash_for_scaled(1000), size=n_noise, dtype=U64))
    g_in = min(1, n_ranks - 1)
    everything = np.unique(np.concatenate(refs))
    inside = in_range(everything[::2], bounds[g_in], bounds[g_in + 1])
    edges = [b - d for b in bounds[1:-1] for d in (0, 1)]
    on_bounds = np.union1d(np.array(edges, dtype=U64), mix[::3]) if edges else mix[1::3]
    return [mix, EMPTY.copy(), inside, on_bounds]


@functools.lru_cache(maxsize=None)
def range_case(n: int, n_ranks: int, hand: bool = False):
    """N references over n_ranks equal-width hash ranges (dist.hash_range_bounds); every inner bound lo_g and lo_g - 1 are
    hashes of the database (of two references each), so a slice or a sample cut one hash off shows.  hand=True: the second of
    three ranges is cut by hand around six neighbouring hashes, so that rank's slice has hashes in a few references only."""
    rng = np.random.default_rng(77 * n + n_ranks)
    refs = make_refs(n)
    max_hash = int(max(int(r[-1]) for r in refs if r.size))
    if hand:
        assert n_ranks == 3
        distinct = np.unique(np.concatenate(refs))
        k = distinct.size // 2
        bounds = [0, int(distinct[k]), int(distinct[k + 6]), 2 ** 64]
    else:
        bounds = ydist.hash_range_bounds(max_hash, n_ranks)
    for k, b in enumerate(bounds[1:-1]):  # the bound and the hash below it, each in two references (where there are two)
        for d, j in ((0, 5 * k + 1), (0, 5 * k + 4), (1, 5 * k + 1), (1, 5 * k + 7)):
            j %= n
            while n >= 8 and (j in (2, n // 3) or refs[j].size <= 1):  # (the twins stay twins, the small ones small)
                j = (j + 1) % n
            refs[j] = np.union1d(refs[j], np.array([b - d], dtype=U64))
    assert int(max(int(r[-1]) for r in refs if r.size)) == max_hash, "the bound hashes must not move the bounds"
    values, offsets = synth.pack(refs)
    c = range_shares(values, offsets, bounds, _samples_for(rng, refs, bounds))
    c.refs = refs
    c.hand = hand
    assert all(v.size for v, _ in c.slices), "every rank needs a non-empty slice: an all-empty handle takes no run step"
    return c


@functools.lru_cache(maxsize=None)
def context_case():
    """Two ranks, 16 different samples: one per step context."""
    rng = np.random.default_rng(4242)
    refs = make_refs(257, seed=1)
    values, offsets = synth.pack(refs)
    bounds = ydist.hash_range_bounds(int(values.max()), 2)
    samples = []
    for k in range(16):
        present = [int(x) for x in rng.choice(len(refs), size=2 + k % 5, replace=False)]
        samples.append(np.union1d(synth.sample_from_refs(rng, refs, present, 0.5, 0),
                                  rng.integers(0, synth.max_hash_for_scaled(1000), size=40, dtype=U64)))
    c = range_shares(values, offsets, bounds, samples)
    c.refs = refs
    return c


# ---- batched hash-range halves ---------------------------------------------------------------------------------------------------
def batch_samples(rng, refs, bounds, n_samples: int, only_rank=None):
    """n_samples samples: sample 3 empty, samples 4 and 5 the same, sample 1 wholly inside the first range; only_rank: ALL of
    them inside that rank's range (every other rank then has no hash to look up in the whole block)."""
    n = len(refs)
    out = []
    for s in range(n_samples):
        present = [int(x) for x in rng.choice(n, size=1 + s % 6, replace=False)]
        smp = np.union1d(synth.sample_from_refs(rng, refs, present, float(rng.uniform(0.1, 0.9)), 0),
                         rng.integers(0, synth.max_hash_for_scaled(1000), size=30, dtype=U64))
        if s == 1:
            smp = in_range(smp, bounds[0], bounds[1])
        if only_rank is not None:
            smp = in_range(smp, bounds[only_rank], bounds[only_rank + 1])
        out.append(smp)
    if n_samples > 3:
        out[3] = EMPTY.copy()
    if n_samples > 5:
        out[5] = out[4].copy()
    return out


def batch_expect(c):
    """Adds the block forms to a range_shares case: per rank the concatenated slices, the subset words and the [B][N] shares."""
    n_samples = len(c.samples)
    c.B, c.P = n_samples, (n_samples + 63) // 64
    c.cat, c.soff, c.words, c.rows = [], [], [], []
    for g in range(c.n_ranks):
        parts = [c.samples[s][c.spans[s][g][0]: c.spans[s][g][1]] for s in range(n_samples)]
        c.cat.append(np.concatenate(parts).astype(U64))
        c.soff.append(np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(U64))
        c.rows.append(tuple(np.stack([c.share[s][g][k] for s in range(n_samples)]) for k in range(3)))
        c.words.append(subset_words(c.rows[g][0]))
    c.whole_rows = tuple(np.stack([c.whole[s][k] for s in range(n_samples)]) for k in range(3))
    c.global_words = subset_words(c.whole_rows[0])
    return c


@functools.lru_cache(maxsize=None)
def batch_db():
    refs = make_refs(BATCH_N, seed=2)
    values, offsets = synth.pack(refs)
    return refs, values, offsets


@functools.lru_cache(maxsize=None)
def batch_case(n_ranks: int, n_samples: int, only_rank=None, seed: int = 0):
    refs, values, offsets = batch_db()
    bounds = ydist.hash_range_bounds(int(values.max()), n_ranks)
    rng = np.random.default_rng(31 * n_samples + n_ranks + 1000 * seed)
    c = range_shares(values, offsets, bounds, batch_samples(rng, refs, bounds, n_samples, only_rank))
    c.refs = refs
    return batch_expect(c)


def compact_rows(c) -> np.ndarray:
    """[k][5] (sample, ref, overlap, n_excl, n_match): the cells of the block's global subset in (reference, sample) order."""
    ov, e, m = c.whole_rows
    ref, smp = np.nonzero(ov.T > 0)
    return np.stack([smp, ref, ov[smp, ref], e[smp, ref], m[smp, ref]], axis=1).astype(np.uint32)


# ---- reference shards with ghosts --------------------------------------------------------------------------------------------------
def ghost_shards(refs, cuts, samples):
    """Reference shards [cuts[r], cuts[r + 1]) with their ghosts.  The gathered layout of the test: one row of W 32-bit words
    per rank, W = what the largest rank's LOCAL references take, rank q's reference i at bit q * W * 32 + i."""
    n_ranks = len(cuts) - 1
    values, offsets = synth.pack(refs)
    w = max((cuts[r + 1] - cuts[r] + 31) // 32 for r in range(n_ranks))
    owner = np.repeat(np.arange(n_ranks), np.diff(cuts))
    c = SimpleNamespace(n=len(refs), n_ranks=n_ranks, W=w, refs=refs, cuts=list(cuts), values=values, offsets=offsets,
                        samples=samples, ranks=[], whole=[whole_counts(values, offsets, s)[:3] for s in samples])
    for r in range(n_ranks):
        b, e = cuts[r], cuts[r + 1]
        local = refs[b:e]
        mine = np.unique(np.concatenate(local)) if sum(x.size for x in local) else EMPTY
        ghosts = [(f, np.intersect1d(refs[f], mine)) for f in range(len(refs)) if not b <= f < e]
        ghosts = [(f, h) for f, h in ghosts if h.size]
        n_pad = ((e - b + 63) // 64) * 64
        rows = list(local) + [EMPTY] * (n_pad - (e - b)) + [h for _, h in ghosts]
        v, o = synth.pack(rows)
        src = np.array([int(owner[f]) * w * 32 + (f - cuts[owner[f]]) for f, _ in ghosts], dtype=np.uint32)
        c.ranks.append(SimpleNamespace(begin=b, end=e, n_local=e - b, ghost_begin=n_pad, n_ghost=len(ghosts), n_rows=len(rows),
                                       values=v, offsets=o, ghost_ids=[f for f, _ in ghosts], ghost_src=src,
                                       out_words=bit_words(len(rows))))
    return c


@functools.lru_cache(maxsize=None)
def ghost_clustered_case(n_ranks: int):
    """Clusters of five cut in their middle, so every rank has ghosts; behind them a copy of a reference of the first rank (all
    its hashes are another rank's too), an empty and a one-hash reference.  The first and the last reference are a pair made by
    hand that shares three hashes and nothing else; samples 3 and 4 hold half of the first one's other hashes -- sample 4 also
    half of the last one's -- so the three hashes are exclusive to the first reference in sample 3 and to nobody in sample 4,
    and on neither rank does the ghost's own overlap say which (the shared hashes are in no sample)."""
    rng = np.random.default_rng(500 + n_ranks)
    mh = synth.max_hash_for_scaled(1000)
    n_cl = 12 * n_ranks + 1
    body = clustered(rng, 5 * n_cl)
    first, last = synth.random_sketch(rng, 80, mh), synth.random_sketch(rng, 60, mh)
    common = synth.random_sketch(rng, 3, mh)
    refs = [np.union1d(first, common)] + body + [body[2].copy(), EMPTY.copy(), body[0][:1].copy(), np.union1d(last, common)]
    cuts = [0] + [1 + 5 * ((n_cl * r) // n_ranks) + 2 for r in range(1, n_ranks)] + [len(refs)]
    half_first = np.setdiff1d(first, common)[::2]
    samples = [np.union1d(synth.sample_from_refs(rng, refs, [c_ - 1 for c_ in cuts[1:-1]] + [1, 3, 8, len(refs) - 4], 0.6, 0),
                          rng.integers(0, mh, size=100, dtype=U64)),
               EMPTY.copy(),
               synth.sample_from_refs(rng, refs, [cuts[1], 12], 0.8, 0),
               half_first,
               np.union1d(half_first, np.setdiff1d(last, common)[::2])]
    c = ghost_shards(refs, cuts, samples)
    c.common = common
    return c


@functools.lru_cache(maxsize=None)
def ghost_edge_case(n_local0: int, n_ghost0: int):
    """Two ranks, built by hand: rank 0 holds n_local0 private references; rank 1 holds n_ghost0 references that each share two
    hashes with reference i % n_local0 of rank 0 -- rank 0's ghosts, exactly n_ghost0 of them -- and 40 that share nothing.
    Samples 0 and 1 are the two directions of ghost 0's bit: both hold half of local reference 0 but NOT the two hashes it
    shares with its ghost's owner; sample 1 also holds private hashes of that owner.  The shared hashes are exclusive to
    reference 0 in sample 0 and not in sample 1."""
    rng = np.random.default_rng(100 * n_local0 + n_ghost0)
    mh = synth.max_hash_for_scaled(1000)
    local = [synth.random_sketch(rng, int(rng.integers(40, 90)), mh) for _ in range(n_local0)]
    sharing = []
    for i in range(n_ghost0):
        sharing.append(np.union1d(synth.random_sketch(rng, int(rng.integers(40, 90)), mh), local[i % n_local0][[1, -2]]))
    rest = [synth.random_sketch(rng, 50, mh) for _ in range(40)]
    refs = local + sharing + rest
    shared0 = np.intersect1d(local[0], np.unique(np.concatenate(sharing)))
    private0 = np.setdiff1d(local[0], shared0)
    owner_private = np.setdiff1d(sharing[0], local[0])
    last = n_ghost0 - 1  # the last ghost: the partial last pair of words of the ghosts' bits
    samples = [private0[::2].copy(),
               np.union1d(private0[::2], owner_private[::3]),
               np.union1d(np.union1d(sharing[last][::2], local[last % n_local0][::2]), rest[5][::4]),
               EMPTY.copy()]
    c = ghost_shards(refs, [0, n_local0, len(refs)], samples)
    c.shared0 = shared0
    return c
