"""Block generators for the batched gather tests, numpy only: blocks of samples over the databases of tests/gather_cases.py,
each sample with its own candidate table inside a member byte that also carries other call sets' bits.  Shared by
tests/test_gather_batch_cases_cpu.py (which guards, with the oracle alone, that the blocks still hold what they are named for)
and tests/test_gpu_gather_batch.py (which runs them on the device).

A block is a dict: values, offsets (the database), samples, abunds (lists, one per sample), members (uint8 [n_samples,
n_refs]) and masks (the cand_mask values worth a call).  want(block, mask, ...) is the oracle's answer per sample, cached:
it is computed once and shared by the tests that need it."""
import numpy as np
from gather_cases import big, big_sample, descending, hand_written, posting_lists
from gather_oracle import NOBODY, gather_oracle, gather_sets

TILE = 1024      # YH_GATHER_BATCH_TILE: consecutive hashes of one sample a lookup workgroup takes
MAX_ROWS = 4096  # YH_GATHER_BATCH_MAX_ROWS
EDGE_SIZES = (0, 1, TILE - 1, TILE, TILE + 1)
SET_A, SET_B = 0x01, 0x40  # bit 0 and bit 6 of a member byte
OTHER_BITS = 0x3E          # bits 1..5: call sets no test ranks


def candidates(block, s: int, mask: int) -> np.ndarray:
    return ((block["members"][s] & np.uint8(mask)) != 0).astype(np.uint8)


def _noise(rng, shape, keep_clear: int) -> np.ndarray:
    """Random bits outside `keep_clear` for every byte: what other call sets leave in a member row."""
    return (rng.integers(0, 256, shape, dtype=np.uint8) & np.uint8(0x7F & ~keep_clear)).astype(np.uint8)


def _block(values, offsets, samples, abunds, members, masks, sets=False, fast=False):
    return dict(values=values, offsets=offsets, samples=[np.asarray(s, np.uint64) for s in samples],
                abunds=[np.asarray(a, np.uint32) for a in abunds], members=np.ascontiguousarray(members, np.uint8), masks=tuple(masks),
                oracle=gather_sets if sets else oracle_on_candidates if fast else gather_oracle, cache={})


def want(block, mask: int, flat: bool = False, **stops):
    """[(rows, more, owner)] per sample from the block's oracle, with the abundances or (flat) without."""
    key = (mask, flat, tuple(sorted(stops.items())))
    if key not in block["cache"]:
        block["cache"][key] = [
            block["oracle"](block["values"], block["offsets"], smp, candidates(block, s, mask), None if flat else block["abunds"][s], **stops)
            for s, smp in enumerate(block["samples"])]
    return block["cache"][key]


def oracle_on_candidates(values, offsets, sample, cand, abund=None, **stops):
    """gather_oracle on the candidate references alone, the rows and owners renamed back: holders that are no candidates
    never count, never win and never block, so the answer is the same, and the oracle's one binary search per reference
    hash covers a few dozen references, not the whole database.  (The guards compare it with the oracle on everything.)"""
    idx = np.flatnonzero(np.asarray(cand) != 0)
    offsets = np.asarray(offsets, dtype=np.int64)
    parts = [values[offsets[j]:offsets[j + 1]] for j in idx]
    sub_offsets = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)
    sub_values = np.concatenate(parts) if parts else np.zeros(0, np.uint64)
    rows, more, owner = gather_oracle(sub_values, sub_offsets, sample, np.ones(idx.size, np.uint8), abund, **stops)
    rows = rows.copy()
    rows["ref"] = idx[rows["ref"]] if rows.size else rows["ref"]
    took = owner != NOBODY
    owner = owner.copy()
    owner[took] = idx[owner[took]]
    return rows, more, owner


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def hand_block():
    """hand_written() four times: its own candidates, all candidates, no candidate, and an empty sample.  The candidates are
    bit 0; every byte carries bit 2 or bit 5 as well, so the non-candidates are not zero bytes."""
    def make():
        values, offsets, sample, cand, abund, _rows, _owner = hand_written()
        n = cand.size
        members = np.stack([cand, np.ones(n, np.uint8), np.zeros(n, np.uint8), cand])
        members = members | np.where(np.arange(n) % 2 == 0, 0x04, 0x20).astype(np.uint8)[None, :]
        empty = np.zeros(0, np.uint64)
        return _block(values, offsets, [sample, sample, sample, empty], [abund, abund, abund, empty], members, (SET_A,), sets=True)
    return _cached("hand", make)


def posting_block(length: int):
    """posting_lists(length) three times with candidate tables that differ: its own (every second of the references in between
    is no candidate), all of them, and the complement of its own plus the three large references; the second and third
    samples lack every seventh / every third hash."""
    def make():
        values, offsets, sample, cand, abund, _groups = posting_lists(length)
        n = cand.size
        third = (1 - cand).astype(np.uint8)
        third[[0, 2, n - 1]] = 1
        rng = np.random.default_rng(8100 + length)
        members = np.stack([cand, np.ones(n, np.uint8), third]) | _noise(rng, (3, n), SET_A)
        keep2, keep3 = np.arange(sample.size) % 7 != 0, np.arange(sample.size) % 3 != 0
        return _block(values, offsets, [sample, sample[keep2], sample[keep3]], [abund, abund[keep2], abund[keep3]], members, (SET_A,))
    return _cached(("posting", length), make)


def _big_members(rng, n_samples: int, few_of):
    """Per-sample member rows over big()'s references.  Set A (bit 0) is big()'s candidate table with a few cluster members
    dropped per sample -- the first cluster's parent (300) and its copy (360) always stay, so their round is a tie -- and set
    B (bit 6) a different table: the second cluster's parent side and other independent references.  few_of(s): about twenty
    candidates per set for sample s (the small samples of the larger blocks keep the oracle's work small).  Bits 1..5 are noise on every byte."""
    _refs, _values, _offsets, cand, _present = big()
    n = cand.size
    members = _noise(rng, (n_samples, n), SET_A | SET_B)
    for s in range(n_samples):
        few = few_of(s)
        a = cand.copy()
        drop = rng.choice(np.arange(301, 360), size=40 if few else 6, replace=False)
        a[drop] = 0
        a[[300, 360]] = 1
        b = np.zeros(n, np.uint8)
        b[rng.choice(np.arange(300, 362), size=12 if few else 30, replace=False)] = 1
        b[np.arange(0, 40, 4)] = 1
        b[361] = 1
        members[s] |= a * np.uint8(SET_A) | b * np.uint8(SET_B)
    return members


def _small_samples(n_samples: int, sizes):
    """Samples cut from big_sample(120_000): sample k is every 16th hash from k on, cut to sizes[k % len(sizes)]."""
    sample, abund = big_sample(120_000)
    out_s, out_a = [], []
    for k in range(n_samples):
        size = sizes[k % len(sizes)]
        out_s.append(sample[k % 16::16][:size])
        out_a.append(abund[k % 16::16][:size])
    return out_s, out_a


def big_block(n_samples: int):
    """Blocks over big(): 1 = one big_sample(120_000); 2 = that and a sample of one hash; 65 = the sizes 0, 1, a tile minus
    one, a tile, a tile plus one and 3000 in turn, with the big sample last; 256 = small samples only (700 to 1100 hashes)."""
    def make():
        _refs, values, offsets, _cand, _present = big()
        large = big_sample(120_000)
        rng = np.random.default_rng(8200 + n_samples)
        if n_samples == 1:
            samples, abunds = [large[0]], [large[1]]
        elif n_samples == 2:
            samples, abunds = [large[0], large[0][500:501]], [large[1], large[1][500:501]]
        elif n_samples == 65:
            samples, abunds = _small_samples(64, EDGE_SIZES + (3000,))
            samples, abunds = samples + [large[0]], abunds + [large[1]]
        else:
            assert n_samples == 256
            samples, abunds = _small_samples(256, (700, TILE, 900, 1100))
        return _block(values, offsets, samples, abunds, _big_members(rng, n_samples, lambda s: samples[s].size < 10_000), (SET_A, SET_B), fast=True)
    return _cached(("big", n_samples), make)


def descending_block(n_rows: int):
    """descending(n_rows) as a block of n_rows samples: sample s is the union of the first s references (and three hashes
    nobody holds), so it has exactly s rows, reference k in round k, and the samples finish after 0 .. n_rows - 1 rounds."""
    def make():
        values, offsets, _sample, cand, _abund = descending(n_rows)
        extra = np.array([1, 2, 3], np.uint64)
        samples = [np.union1d(values[:int(offsets[s])], extra) for s in range(n_rows)]
        abunds = [np.arange(s.size) % 7 + 1 for s in samples]
        rng = np.random.default_rng(8300 + n_rows)
        members = np.ones((n_rows, n_rows), np.uint8) | _noise(rng, (n_rows, n_rows), SET_A)
        return _block(values, offsets, samples, abunds, members, (SET_A,))
    return _cached(("descending", n_rows), make)


def wide_block():
    """Two samples of the first cluster's parent (with shared hashes among its 5000) at abundance 2^32 - 1 and 2^31."""
    def make():
        refs, values, offsets, _cand, _present = big()
        members = np.zeros((2, len(refs)), np.uint8)
        members[:, [300, 301, 305]] = 1
        members |= np.uint8(0x10)
        take = np.union1d(refs[300], refs[305][:500])
        return _block(values, offsets, [take, take[::2]],
                      [np.full(take.size, 2 ** 32 - 1, np.uint64), np.full(take[::2].size, 2 ** 31, np.uint64)], members, (SET_A,), fast=True)
    return _cached("wide", make)


__all__ = ["NOBODY", "TILE", "MAX_ROWS", "EDGE_SIZES", "SET_A", "SET_B", "OTHER_BITS", "candidates", "want", "oracle_on_candidates", "hand_block",
           "posting_block", "big_block", "descending_block", "wide_block"]
