"""Brute-force restatement of RefDB.classify_sets for the classify tests.  The node of every entry is tests/lca_oracle's (the
holders from the CSR, the LCA by intersecting ancestor sets); a set's row is a Python loop over its entries and one more
intersection of ancestor sets over the distinct nodes of its informative hits.  Nothing is tiled, scanned or joined here."""
import numpy as np
from lca_oracle import NONE, ancestor_sets, lca_of_nodes, lca_oracle

ROW_DTYPE = np.dtype([("node", np.uint32), ("n_kept", np.uint32), ("n_hit", np.uint32), ("n_root", np.uint32)])
CLASSES = ("empty", "no_hit", "root_only", "one_informative", "several_agreeing", "fold_above_every_hit", "root_with_informative",
           "crosses_tile_border", "spans_three_tiles")


def rows_from_nodes(parent, nodes, off):
    """rows [n_sets] from the per-entry nodes and the set offsets."""
    sets, depth = ancestor_sets(parent)
    off = np.asarray(off, dtype=np.int64)
    rows = np.zeros(off.size - 1, dtype=ROW_DTYPE)
    memo = {}
    for s in range(off.size - 1):
        mine = nodes[off[s]:off[s + 1]]
        hit = mine[mine != NONE]
        inf = tuple(sorted(set(hit[hit != 0].tolist())))
        if inf:
            if inf not in memo:
                memo[inf] = lca_of_nodes(sets, depth, inf)
            node = memo[inf]
        else:
            node = 0 if hit.size else NONE
        rows[s] = (node, mine.size, hit.size, int((hit == 0).sum()))
    return rows


def classify_oracle(values, offsets, parent, leaf, mins, off):
    """(rows, nodes) for CSR references, a taxonomy (parent, leaf) and the sets (mins, off)."""
    mins = np.asarray(mins, dtype=np.uint64)
    nodes = lca_oracle(values, offsets, parent, leaf, mins)[0] if mins.size else np.zeros(0, dtype=np.uint32)
    return rows_from_nodes(parent, nodes, off), nodes


def census(parent, nodes, off, rows, tile):
    """{class: number of sets} over CLASSES, from the oracle's rows and nodes alone."""
    sets, depth = ancestor_sets(parent)
    off = np.asarray(off, dtype=np.int64)
    got = dict.fromkeys(CLASSES, 0)
    for s in range(off.size - 1):
        a, b = int(off[s]), int(off[s + 1])
        r = rows[s]
        if a == b:
            got["empty"] += 1
            continue
        mine = nodes[a:b]
        inf = mine[(mine != NONE) & (mine != 0)]
        distinct = set(inf.tolist())
        if r["n_hit"] == 0:
            got["no_hit"] += 1
        elif inf.size == 0:
            got["root_only"] += 1
        elif inf.size == 1:
            got["one_informative"] += 1
        elif len(distinct) == 1:
            got["several_agreeing"] += 1
        if inf.size and int(r["node"]) not in distinct:  # (the root among them, when no hit sits there)
            got["fold_above_every_hit"] += 1
        if inf.size and r["node"] == 0:
            got["root_with_informative"] += 1
        tiles = (b - 1) // tile - a // tile + 1
        if tiles >= 2:
            got["crosses_tile_border"] += 1
        if tiles >= 3:
            got["spans_three_tiles"] += 1
    return got
