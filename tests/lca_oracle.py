"""Brute-force restatement of RefDB.lca in numpy and Python sets, for the lineage tests.  It shares nothing with the device
code: the holders of every sample hash come from the CSR itself (all (hash, reference) pairs sorted by hash), and the lowest
common ancestor is the deepest node in the INTERSECTION OF ANCESTOR SETS -- no depth array is taken and nothing is lifted."""
import numpy as np

NONE = 0xFFFFFFFF


def ancestor_sets(parent):
    """Per node the frozenset of its ancestors, itself included, and its depth counted along the way to the root."""
    parent = [int(p) for p in parent]
    sets, depth = [], []
    for v in range(len(parent)):
        chain = [v]
        while chain[-1] != 0:
            assert parent[chain[-1]] < chain[-1] and len(chain) <= len(parent)
            chain.append(parent[chain[-1]])
        sets.append(frozenset(chain))
        depth.append(len(chain) - 1)
    return sets, depth


def lca_of_nodes(sets, depth, nodes):
    """The deepest node every one of `nodes` has among its ancestors."""
    common = frozenset.intersection(*(sets[int(v)] for v in nodes))
    return max(common, key=lambda v: depth[v])


def holders_of(values, offsets, sample):
    """(refs, lo, hi): sample hash i is held by refs[lo[i]:hi[i]] (ascending reference ids; empty: no reference holds it)."""
    values = np.asarray(values, dtype=np.uint64)
    offsets = np.asarray(offsets, dtype=np.int64)
    sample = np.asarray(sample, dtype=np.uint64)
    ref_of = np.repeat(np.arange(offsets.size - 1, dtype=np.int64), np.diff(offsets))
    order = np.argsort(values, kind="stable")
    sv, sr = values[order], ref_of[order]
    return sr, np.searchsorted(sv, sample, "left"), np.searchsorted(sv, sample, "right")


def lca_oracle(values, offsets, parent, leaf, sample, abund=None):
    """(nodes uint32 [n], counts uint64 [n_nodes, 2]) for CSR references, a taxonomy (parent, leaf) and an ascending uint64
    sample with optionally one abundance per hash (None: all 1)."""
    leaf = np.asarray(leaf, dtype=np.int64)
    sample = np.asarray(sample, dtype=np.uint64)
    n_nodes = len(parent)
    sets, depth = ancestor_sets(parent)
    refs, lo, hi = holders_of(values, offsets, sample)
    n_holders = hi - lo
    nodes = np.full(sample.size, NONE, dtype=np.uint32)
    single = n_holders == 1
    nodes[single] = leaf[refs[lo[single]]]
    memo = {}
    for i in np.flatnonzero(n_holders >= 2):
        key = tuple(sorted(set(leaf[refs[lo[i]:hi[i]]].tolist())))
        if key not in memo:
            memo[key] = lca_of_nodes(sets, depth, key)
        nodes[i] = memo[key]
    return nodes, counts_from_nodes(nodes, n_nodes, abund)


def counts_from_nodes(nodes, n_nodes, abund=None):
    """counts uint64 [n_nodes, 2]: per node the number of hashes assigned to it and the sum of their abundances (None: all 1)."""
    nodes = np.asarray(nodes, dtype=np.uint32)
    known = nodes != NONE
    weights = np.ones(nodes.size, dtype=np.uint64) if abund is None else np.asarray(abund, dtype=np.uint64)
    assert weights.size == nodes.size
    counts = np.zeros((n_nodes, 2), dtype=np.uint64)
    counts[:, 0] = np.bincount(nodes[known].astype(np.int64), minlength=n_nodes)
    sums = np.zeros(n_nodes, dtype=np.uint64)
    np.add.at(sums, nodes[known].astype(np.int64), weights[known])  # (exact 64-bit sums: bincount's weights are floats)
    counts[:, 1] = sums
    return counts


def census(values, offsets, parent, leaf, sample):
    """The classes of sample hashes a kernel can get wrong, from the oracle alone: {"absent", "single", "shared_below_root",
    "shared_root"} -> number of sample hashes, and "shared_depths" -> the set of depths the shared hashes resolve at."""
    nodes, _ = lca_oracle(values, offsets, parent, leaf, sample)
    _, depth = ancestor_sets(parent)
    _, lo, hi = holders_of(values, offsets, sample)
    shared = (hi - lo) >= 2
    return {"absent": int((hi == lo).sum()), "single": int(((hi - lo) == 1).sum()),
            "shared_below_root": int((shared & (nodes != 0)).sum()), "shared_root": int((shared & (nodes == 0)).sum()),
            "shared_depths": {depth[int(v)] for v in np.unique(nodes[shared])}}
