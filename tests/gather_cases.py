"""Case generators for the gather tests, numpy only: the databases, samples and candidate tables that reach the states the
ranking can get wrong by construction.  Shared by tests/test_gather_cases_cpu.py (which guards, with the oracles alone, that
the cases still hold what they are named for) and tests/test_gpu_gather.py (which runs them on the device)."""
import numpy as np

from yacht_amd import synth

NARROW = 2 ** 22  # the "scaled" of tests/test_gpu_explain.py's big database: compact buckets behind the presence filter
ROUNDS = 32       # YH_GATHER_ROUNDS_PER_SYNC
LIST_LENGTHS = (2, 3, 4, 5, 8, 9, 300)  # holders of a shared hash, either side of the four-at-a-time walk
BIG_SIZES = (120_000, 300_000, 600_000)  # one per tile shape of the lookup


def hand_written():
    """Six references, reference 0 no candidate.  (values, offsets, sample, cand, abund, rows, owner), the last two spelled
    out: rows as (ref, n_overlap, n_unique, w_unique).
      round 0: references 1 and 2 both hold five sample hashes: 1 wins (the lower index); it takes 10, which reference 0 --
               no candidate, and in front of it in the hash's holder list -- holds too
      round 1: 2 fell from 5 to 3 and now ties with 3 and 4, which a round ago it did not: 2 wins
      round 2: 4 takes 11 (again shared with reference 0), 21 and 22: reference 5, which held two live hashes, falls to 0
               and never wins
      round 3: 3 is left with 20
    12 has reference 0 as its only holder and 30 has none: nobody's."""
    refs = [[10, 11, 12, 50], [1, 2, 3, 4, 10], [3, 4, 5, 6, 7], [5, 6, 20], [11, 21, 22], [21, 22]]
    values, offsets = synth.pack([np.array(r, np.uint64) for r in refs])
    sample = np.array([1, 2, 3, 4, 5, 6, 7, 10, 11, 12, 20, 21, 22, 30], np.uint64)
    abund = np.arange(1, 15)
    cand = np.array([0, 1, 1, 1, 1, 1], np.uint8)
    rows = [(1, 5, 5, 1 + 2 + 3 + 4 + 8), (2, 5, 3, 5 + 6 + 7), (4, 3, 3, 9 + 12 + 13), (3, 3, 1, 11)]
    none = 0xFFFFFFFF
    owner = [1, 1, 1, 1, 2, 2, 2, 1, 4, none, 3, 4, 4, none]
    return values, offsets, sample, cand, abund, rows, owner


def posting_lists(length: int):
    """A database whose shared hashes all have `length` holders.  Reference 0 (A), the last one (Z) and reference 2 (M) hold
    40, 30 and 20 private hashes and win the first three rounds; the length + 1 references between them hold one to three.
    Three groups of five shared hashes: F is held by A and the first length - 1 of the others (the winner of round 0 is the
    FIRST holder), L by Z and the last length - 1 of them (the winner of round 1 is the LAST holder), X by the first
    `length` of them and by neither A, Z nor M (the winners of rounds 0 to 2 are ABSENT from its lists; M is absent from
    every list).  Every second of the references in between is no candidate, so candidate and other holders alternate in
    every list.  Returns (values, offsets, sample, cand, abund, groups)."""
    rng = np.random.default_rng(7100 + length)
    n_refs = length + 4
    a, z, m = 0, n_refs - 1, 2
    others = [j for j in range(1, n_refs - 1) if j != m]
    assert len(others) == length + 1
    pool = rng.permutation(np.arange(1000, 1000 + 20 * n_refs + 200, dtype=np.uint64))
    take = lambda k: (pool[:k].copy(), pool[k:])  # noqa: E731
    refs = [[] for _ in range(n_refs)]
    groups = {}
    for name, holders in (("F", [a] + others[:length - 1]), ("L", others[-(length - 1):] + [z]), ("X", others[:length])):
        assert len(holders) == length
        block, pool = take(5)
        groups[name] = (np.sort(block), holders)
        for j in holders:
            refs[j].append(block)
    for j, k in ((a, 40), (z, 30), (m, 20)):
        block, pool = take(k)
        refs[j].append(block)
    for i, j in enumerate(others):
        block, pool = take(1 + i % 3)
        refs[j].append(block)
    refs = [np.unique(np.concatenate(r)) for r in refs]
    values, offsets = synth.pack(refs)
    cand = np.ones(n_refs, np.uint8)
    cand[others[1::2]] = 0
    absent, pool = take(30)
    sample = np.union1d(values, absent)
    return values, offsets, sample, cand, rng.integers(1, 1001, sample.size), groups


_BIG = {}


def big():
    """tests/test_gpu_explain.py's big database (300 independent plus 60 clustered references in a narrow hash range: compact
    buckets and the presence filter), with two cluster members duplicated at the end: a copy of the first cluster's parent,
    which is a candidate like the parent itself -- two identical candidates, so the round that cluster's parent wins is
    decided by the tie rule -- and a copy of the second cluster's parent that is NO candidate, so that cluster's hashes have
    holders on both sides.  Returns (refs, values, offsets, cand, clustered): the candidates are the 60 cluster members,
    the first copy, nine independent references that are in the samples and ten that are not."""
    if not _BIG:
        rng = np.random.default_rng(7200)
        refs = synth.independent_refs(rng, 300, 5000, 0.35, 500, 20000, scaled=NARROW) + \
            synth.clustered_refs(rng, 12, (1, 0.9, 0.5, 0.25, 0.1), 5000, scaled=NARROW)
        refs += [refs[300].copy(), refs[305].copy()]
        clustered = np.arange(300, 360)
        present = np.concatenate([clustered, np.arange(0, 40, 2)])  # twenty independent references beside the clusters
        cand = np.zeros(len(refs), np.uint8)
        cand[clustered] = 1
        cand[360] = 1
        cand[np.arange(0, 18, 2)] = 1    # in the samples
        cand[np.arange(101, 121, 2)] = 1  # not in the samples
        values, offsets = synth.pack(refs)
        _BIG.update(refs=refs, values=values, offsets=offsets, cand=cand, present=present)
    return _BIG["refs"], _BIG["values"], _BIG["offsets"], _BIG["cand"], _BIG["present"]


def big_sample(n_sample: int):
    """(sample, abund): the cluster members and twenty independent references at coverage 0.3, noise up to n_sample."""
    key = ("sample", n_sample)
    if key not in _BIG:
        refs, _values, _offsets, _cand, present = big()
        rng = np.random.default_rng(7200 + n_sample)
        sample = synth.sample_from_refs(rng, refs, present, 0.3, n_sample, scaled=NARROW)
        _BIG[key] = (sample, rng.integers(1, 1001, sample.size))
    return _BIG[key]


def descending(n_rows: int):
    """n_rows disjoint references of n_rows + 2, n_rows + 1, ..., 3 hashes, all candidates, and the sample of all their hashes:
    exactly n_rows rows, reference k in round k."""
    sizes = np.arange(n_rows + 2, 2, -1)
    pool = np.arange(500, 500 + int(sizes.sum()), dtype=np.uint64) * np.uint64(3)
    cuts = np.cumsum(sizes)[:-1]
    refs = np.split(pool, cuts)
    values, offsets = synth.pack(refs)
    sample = np.union1d(pool, np.array([1, 2, 3], np.uint64))
    return values, offsets, sample, np.ones(n_rows, np.uint8), np.arange(sample.size) % 7 + 1


def assert_big_classes(stats, rows):
    """What a big case must show, from the oracle's own result: at least 30 rows, 100 hashes that change hands through a
    shared hit, 100 single-holder hits on a candidate and 100 on another reference, 100 shared hits with holders on both
    sides, and a round the tie rule decides."""
    print("rows", len(rows), stats)
    assert len(rows) >= 30
    assert stats["n_owned_shared"] >= 100 and stats["n_solo_candidate"] >= 100 and stats["n_solo_other"] >= 100
    assert stats["n_shared_both_sides"] >= 100 and stats["n_tie_rounds"] >= 1
