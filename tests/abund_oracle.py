"""Brute-force restatement of RefDB.abundance in numpy, for the abundance tests.  No trick from the library: membership
of the sample's hashes by np.isin per reference, a holder count per sample hash, np.median for the median."""
import numpy as np


def abundance_oracle(values, offsets, sample, abund):
    """(w_overlap uint64 [N], w_match uint64 [N], med_match float64 [N]) for CSR references, an ascending uint64 sample
    and one abundance per sample hash."""
    values = np.asarray(values, dtype=np.uint64)
    offsets = np.asarray(offsets, dtype=np.int64)
    sample = np.asarray(sample, dtype=np.uint64)
    abund = np.asarray(abund, dtype=np.uint64)
    assert sample.size == abund.size
    n = offsets.size - 1
    # only sample hashes that some reference holds can count: the per-reference passes run over those
    known = np.isin(sample, values)
    s, a = sample[known], abund[known]
    member = [np.isin(s, values[offsets[j]:offsets[j + 1]]) for j in range(n)]
    holders = np.zeros(s.size, dtype=np.int64)
    for m in member:
        holders += m
    w_overlap = np.zeros(n, dtype=np.uint64)
    w_match = np.zeros(n, dtype=np.uint64)
    med = np.zeros(n, dtype=np.float64)
    for j, m in enumerate(member):
        w_overlap[j] = a[m].sum(dtype=np.uint64)
        only = m & (holders == 1)
        w_match[j] = a[only].sum(dtype=np.uint64)
        if only.any():
            med[j] = float(np.median(a[only].astype(np.float64)))
    return w_overlap, w_match, med
