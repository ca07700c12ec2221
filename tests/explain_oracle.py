"""Brute-force restatement of RefDB.explain in numpy, for the residual tests.  No trick from the library: membership of
the sample's hashes by np.isin per reference, the OR of the member bytes over the holders, the totals from the flags."""
import numpy as np


def totals_from_flags(flags, abund=None):
    """totals uint64 [8, 2]: per bit the number of flags that have it set and the sum of the abundances there (None: all 1)."""
    flags = np.asarray(flags, dtype=np.uint8)
    abund = np.ones(flags.size, dtype=np.uint64) if abund is None else np.asarray(abund, dtype=np.uint64)
    assert abund.size == flags.size
    totals = np.zeros((8, 2), dtype=np.uint64)
    for b in range(8):
        has = ((flags >> b) & 1) == 1
        totals[b, 0] = int(has.sum())
        totals[b, 1] = abund[has].sum(dtype=np.uint64)
    return totals


def _held(values, offsets, sample):
    """Per reference j, the boolean array "sample hash is in R_j" (np.isin against the reference's slice)."""
    for j in range(offsets.size - 1):
        yield j, np.isin(sample, values[offsets[j]:offsets[j + 1]])


def explain_oracle(values, offsets, sample, member, abund=None):
    """(flags uint8 [n], totals uint64 [8, 2]) for CSR references, an ascending uint64 sample, one member byte per reference
    and optionally one abundance per sample hash (None: all 1)."""
    values = np.asarray(values, dtype=np.uint64)
    offsets = np.asarray(offsets, dtype=np.int64)
    sample = np.asarray(sample, dtype=np.uint64)
    member = np.asarray(member, dtype=np.uint8)
    assert member.size == offsets.size - 1 and not (member & 0x80).any()
    # only sample hashes that some reference holds can get a flag: the per-reference passes run over those
    known = np.isin(sample, values)
    part = np.zeros(int(known.sum()), dtype=np.uint8)
    for j, held in _held(values, offsets, sample[known]):
        part[held] |= np.uint8(0x80) | member[j]
    flags = np.zeros(sample.size, dtype=np.uint8)
    flags[known] = part
    return flags, totals_from_flags(flags, abund)


def classes(values, offsets, sample, member, bits):
    """For each call set of `bits`, the number of sample hashes in each of the four classes a kernel can get wrong: not in
    the database, single holder inside the set, single holder outside it, shared with holders on both sides of it."""
    values = np.asarray(values, dtype=np.uint64)
    offsets = np.asarray(offsets, dtype=np.int64)
    sample = np.asarray(sample, dtype=np.uint64)
    member = np.asarray(member, dtype=np.uint8)
    known = np.isin(sample, values)
    s = sample[known]
    holders = np.zeros(s.size, dtype=np.int64)
    n_in = {b: np.zeros(s.size, dtype=np.int64) for b in bits}
    for j, held in _held(values, offsets, s):
        holders += held
        for b in bits:
            if (member[j] >> b) & 1:
                n_in[b] += held
    assert (holders >= 1).all()
    out = {}
    for b in bits:
        n_out = holders - n_in[b]
        out[b] = (int(sample.size - s.size), int(((n_in[b] == 1) & (n_out == 0)).sum()), int(((n_in[b] == 0) & (n_out == 1)).sum()),
                  int(((n_in[b] >= 1) & (n_out >= 1)).sum()))
    return out
