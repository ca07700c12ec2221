"""Two restatements of RefDB.gather for the gather tests.  gather_sets states the contract with Python sets and recounts
every candidate from scratch in every round; gather_oracle is the same ranking in numpy, counts kept incrementally, for the
large cases.  Neither uses a trick of the library: no directory probe, no single-holder shortcut, no live list -- a reference's
sample hashes are found by binary search and every hash, shared or not, is handled the same way."""
import numpy as np

NOBODY = 0xFFFFFFFF
ROW_DTYPE = np.dtype([("ref", np.uint32), ("n_overlap", np.uint32), ("n_unique", np.uint32), ("reserved_", np.uint32),
                      ("w_unique", np.uint64)])


def _rows(rows):
    out = np.zeros(len(rows), dtype=ROW_DTYPE)
    for k, (ref, n_ov, n_un, w_un) in enumerate(rows):
        out[k] = (ref, n_ov, n_un, 0, w_un)
    return out


def gather_sets(values, offsets, sample, cand, abund=None, min_hits=1, cap_rows=None):
    """(rows, more, owner) by the letter of the contract: Python sets per reference, every count recomputed every round."""
    assert min_hits >= 1
    offsets = [int(o) for o in offsets]
    sample = [int(h) for h in sample]
    ab = {h: 1 if abund is None else int(abund[i]) for i, h in enumerate(sample)}
    refs = [set(int(v) for v in values[offsets[j]:offsets[j + 1]]) for j in range(len(offsets) - 1)]
    candidates = [j for j in range(len(refs)) if cand[j]]
    live = set(sample)
    owner = {}
    in_sample = set(sample)
    rows = []
    more = False
    while True:
        best, best_c = None, -1
        for j in candidates:  # (ascending: the first of equal counts stays)
            c = len(refs[j] & live)
            if c > best_c:
                best, best_c = j, c
        if best is None or best_c < min_hits:
            break
        if cap_rows is not None and len(rows) == cap_rows:
            more = True
            break
        taken = refs[best] & live
        rows.append((best, len(refs[best] & in_sample), best_c, sum(ab[h] for h in taken)))
        for h in taken:
            owner[h] = best
        live -= taken
    return _rows(rows), more, np.array([owner.get(h, NOBODY) for h in sample], dtype=np.uint32)




def _pairs(values, offsets, sample):
    """(reference, sample index) of every reference hash that is in the sample, in reference order: one binary search of
    the sample per reference hash."""
    ref_of = np.repeat(np.arange(offsets.size - 1, dtype=np.int64), np.diff(offsets))
    if sample.size == 0 or values.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    pos = np.minimum(np.searchsorted(sample, values), sample.size - 1)
    hit = sample[pos] == values
    return ref_of[hit], pos[hit].astype(np.int64)


def _ranges(starts, lens):
    """The indices of the ranges [starts[i], starts[i] + lens[i]) back to back."""
    total = int(lens.sum())
    if total == 0:
        return np.zeros(0, np.int64)
    first = np.cumsum(lens) - lens
    return np.repeat(starts - first, lens) + np.arange(total, dtype=np.int64)


def gather_oracle(values, offsets, sample, cand, abund=None, min_hits=1, cap_rows=None, stats=None):
    """The same in numpy, for the large cases: the (candidate, sample hash) pairs once, grouped by reference and by sample
    hash; the counts are kept and lowered by what each winner takes.  stats (a dict) receives what the run was made of:
    n_solo_candidate / n_solo_other (sample hashes with one holder in the database, a candidate / not), n_shared_live
    (several holders, a candidate among them), n_shared_both_sides (of those: with a holder that is no candidate),
    n_owned_shared (hashes with several holders that ended with an owner) and n_tie_rounds (rounds the tie rule decided)."""
    assert min_hits >= 1
    values = np.asarray(values, dtype=np.uint64)
    offsets = np.asarray(offsets, dtype=np.int64)
    sample = np.asarray(sample, dtype=np.uint64)
    cand = np.asarray(cand) != 0
    n_refs, n = offsets.size - 1, sample.size
    abund = np.ones(n, dtype=np.uint64) if abund is None else np.asarray(abund, dtype=np.uint64)
    r_all, s_all = _pairs(values, offsets, sample)
    is_c = cand[r_all] if r_all.size else np.zeros(0, bool)
    r, s = r_all[is_c], s_all[is_c]  # (still grouped by reference)
    ref_start = np.searchsorted(r, np.arange(n_refs + 1))
    by_hash = np.argsort(s, kind="stable")
    holders = r[by_hash]  # the candidate holders, grouped by sample hash
    hash_start = np.searchsorted(s[by_hash], np.arange(n + 1))
    counts = np.where(cand, np.diff(ref_start), -1).astype(np.int64)
    n_overlap = counts.copy()
    live = np.ones(n, dtype=bool)
    owner = np.full(n, NOBODY, dtype=np.uint32)
    rows = []
    more = False
    n_ties = 0
    while n_refs:
        k = int(np.argmax(counts))  # (the first of equal counts: the smallest reference index)
        c = int(counts[k])
        if c < min_hits:
            break
        if cap_rows is not None and len(rows) == cap_rows:
            more = True
            break
        n_ties += int((counts == c).sum()) > 1
        mine = s[ref_start[k]:ref_start[k + 1]]
        taken = mine[live[mine]]
        assert taken.size == c
        rows.append((k, int(n_overlap[k]), c, int(abund[taken].sum(dtype=np.uint64))))
        owner[taken] = k
        live[taken] = False
        np.subtract.at(counts, holders[_ranges(hash_start[taken], hash_start[taken + 1] - hash_start[taken])], 1)
    if stats is not None:
        n_holders = np.bincount(s_all, minlength=n)
        n_cand_holders = np.bincount(s, minlength=n)
        stats.update(n_solo_candidate=int(((n_holders == 1) & (n_cand_holders == 1)).sum()),
                     n_solo_other=int(((n_holders == 1) & (n_cand_holders == 0)).sum()),
                     n_shared_live=int(((n_holders >= 2) & (n_cand_holders >= 1)).sum()),
                     n_shared_both_sides=int(((n_holders >= 2) & (n_cand_holders >= 1) & (n_cand_holders < n_holders)).sum()),
                     n_owned_shared=int(((n_holders >= 2) & (owner != NOBODY)).sum()), n_tie_rounds=n_ties)
    return _rows(rows), more, owner
