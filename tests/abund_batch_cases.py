"""The blocks of the batched abundance tests (yh_abund_batch_device), built on the CPU and shared by
test_abund_batch_cases_cpu.py (the oracle alone shows that the blocks sit on the edges that matter) and
test_gpu_abund_batch.py (the kernels against the oracle).

The database is test_gpu_explain.py's `big` recipe: 360 references in a narrow hash range, compact buckets behind the
presence filter, 12 clusters of five for shared hashes.  Samples are random subsets of one pool of its hashes, of sizes
around the lookup kernel's tile T = YH_ABUND_BATCH_TILE.  Even-numbered samples take abundances uniform in 1..1000
(medians that differ from sample to sample), odd-numbered ones min(geometric(0.5), 50) (many equal values: ties in the
sort, medians that end in .5 only when the two middle values differ)."""
import functools

import numpy as np
from abund_oracle import abundance_oracle

from yacht_amd import _lib, synth

NARROW = 2 ** 22  # test_gpu_explain.py: the "scaled" whose hash range lets ~10^6 distinct hashes take the compact buckets
T = _lib.YH_ABUND_BATCH_TILE
EDGE_SIZES = [0, 1, T - 1, T, T + 1, 2 * T + 1, 3000, 5 * T + 7]
I_2T1, I_5T7 = 5, 7  # the places of the 2 T + 1 and the 5 T + 7 sample in EDGE_SIZES


@functools.lru_cache(maxsize=None)
def big_db():
    """(values, offsets, n_refs, pool): the database, and a pool of its hashes in which every reference is present at
    coverage 0.04 and the cluster members at 0.3, with noise up to 200 000 hashes."""
    rng = np.random.default_rng(601)
    refs = synth.independent_refs(rng, 300, 5000, 0.35, 500, 20000, scaled=NARROW) + \
        synth.clustered_refs(rng, 12, (1, 0.9, 0.5, 0.25, 0.1), 5000, scaled=NARROW)
    order = rng.permutation(len(refs))
    refs = [refs[i] for i in order]
    values, offsets = synth.pack(refs)
    cov = np.full(len(refs), 0.04)
    cov[order >= 300] = 0.3
    pool = synth.sample_from_refs(rng, refs, list(range(len(refs))), cov, 200_000, scaled=NARROW)
    return values, offsets, len(refs), pool


def abundances(rng, s: int, size: int) -> np.ndarray:
    """Sample s's abundances: even s uniform in 1..1000, odd s min(geometric(0.5), 50)."""
    if s % 2 == 0:
        return rng.integers(1, 1001, size).astype(np.uint32)
    return np.minimum(rng.geometric(0.5, size), 50).astype(np.uint32)


def sizes(rng, n_samples: int):
    """Sample sizes of a block: the edge sizes first (an empty sample FIRST), an empty one in the middle and last (from
    three samples up), small random sizes for the rest."""
    if n_samples == 1:
        return [2 * T + 1]
    if n_samples == 2:
        return [T + 1, 3000]
    out = (EDGE_SIZES + [int(x) for x in rng.integers(40, 700, max(0, n_samples - len(EDGE_SIZES)))])[:n_samples]
    out[n_samples // 2] = 0
    out[-1] = 0
    return out


def block(seed: int, pool, block_sizes, twin=None):
    """(samples, abunds) of a block: subsets of the pool; twin = (i, j): sample j takes sample i's HASHES and keeps
    abundances of its own."""
    rng = np.random.default_rng(seed)
    samples = [np.sort(rng.choice(pool, size=k, replace=False)) for k in block_sizes]
    if twin is not None:
        samples[twin[1]] = samples[twin[0]].copy()
    abunds = [abundances(rng, s, smp.size) for s, smp in enumerate(samples)]
    return samples, abunds


def oracle_block(values, offsets, samples, abunds, picked=None):
    """{s: (w_overlap, w_match, med_match)} by the oracle, per sample, for the picked samples (all of them by default)."""
    return {s: abundance_oracle(values, offsets, samples[s], abunds[s]) for s in (range(len(samples)) if picked is None else picked)}


@functools.lru_cache(maxsize=None)
def edge_block():
    """The block of the eight edge sizes on `big`, with the oracle's answers and, per (sample, reference), the number of
    single-holder hits (the oracle again, with every abundance 1: w_match is then a count)."""
    values, offsets, _n_refs, pool = big_db()
    samples, abunds = block(771, pool, EDGE_SIZES)
    want = oracle_block(values, offsets, samples, abunds)
    counts = [abundance_oracle(values, offsets, s, np.ones(s.size, np.uint32))[1].astype(np.int64) for s in samples]
    return samples, abunds, want, counts


def edge_classes():
    """What the edge block holds, summed over its samples, of the (sample, reference) pairs a median kernel can get wrong,
    and the references whose medians differ between the 2 T + 1 and the 5 T + 7 sample."""
    _samples, _abunds, want, counts = edge_block()
    got = dict(one_hit=0, two_hits=0, odd_from_3=0, half=0, partly_exclusive=0)
    for s, cnt in enumerate(counts):
        w_ov, w_m, med = want[s]
        got["one_hit"] += int((cnt == 1).sum())
        got["two_hits"] += int((cnt == 2).sum())
        got["odd_from_3"] += int(((cnt >= 3) & (cnt % 2 == 1)).sum())
        got["half"] += int((med % 1.0 == 0.5).sum())
        got["partly_exclusive"] += int(((w_m > 0) & (w_m < w_ov)).sum())
    both = (counts[I_2T1] > 0) & (counts[I_5T7] > 0)
    got["medians_differ"] = int((both & (want[I_2T1][2] != want[I_5T7][2])).sum())
    return got
