"""The lineage cases without a GPU: the hand-written database against the oracle with every node spelled out, the census the
GPU tests ask of their samples, the cases' own construction, and the library's four new symbols as header, binding and
shared object agree on them."""
import ctypes as C
import os

import lca_cases as cases
import numpy as np
from lca_oracle import NONE, ancestor_sets, census, counts_from_nodes, holders_of, lca_of_nodes, lca_oracle

from yacht_amd import _lib

ENTRIES = ("yh_db_set_taxonomy", "yh_db_get_taxonomy", "yh_lca_device", "yh_lca")


def test_hand_written_case_passes_the_oracle():
    values, offsets = cases.pack(cases.HAND_REFS)
    nodes, counts = lca_oracle(values, offsets, cases.HAND_PARENT, cases.HAND_LEAF, cases.HAND_SAMPLE, cases.HAND_ABUND)
    assert nodes.tolist() == cases.HAND_NODES.tolist()
    assert counts.tolist() == cases.HAND_COUNTS.tolist()
    plain = lca_oracle(values, offsets, cases.HAND_PARENT, cases.HAND_LEAF, cases.HAND_SAMPLE)[1]
    assert plain[:, 0].tolist() == plain[:, 1].tolist() == cases.HAND_COUNTS[:, 0].tolist()
    # the tree is the one the comments draw, and the depths the library is given are the oracle's own
    assert ancestor_sets(cases.HAND_PARENT)[1] == cases.HAND_DEPTH.tolist()
    assert int(values.max()) < int(cases.HAND_SAMPLE[-1])  # (the last sample hash lies above the database's largest)


def test_oracle_pieces():
    sets, depth = ancestor_sets(cases.HAND_PARENT)
    assert sets[6] == {6, 3, 1, 0} and sets[0] == {0} and depth == [0, 1, 1, 2, 2, 2, 3, 3, 3]
    assert lca_of_nodes(sets, depth, [6, 6]) == 6 and lca_of_nodes(sets, depth, [6, 3]) == 3
    assert lca_of_nodes(sets, depth, [6, 7]) == 1 and lca_of_nodes(sets, depth, [6, 7, 8]) == 0 and lca_of_nodes(sets, depth, [7, 0]) == 0
    values, offsets = cases.pack(cases.HAND_REFS)
    refs, lo, hi = holders_of(values, offsets, np.array([25, 26, 30], np.uint64))
    assert [refs[a:b].tolist() for a, b in zip(lo, hi)] == [[0, 1, 2, 3], [], [4]]
    counts = counts_from_nodes(np.array([2, NONE, 2, 0], np.uint32), 3, np.array([2 ** 40, 9, 2 ** 40, 5], np.uint64))
    assert counts.tolist() == [[1, 5], [0, 0], [2, 2 ** 41]]


def test_census_helper():
    values, offsets = cases.pack(cases.HAND_REFS)
    got = census(values, offsets, cases.HAND_PARENT, cases.HAND_LEAF, cases.HAND_SAMPLE)
    assert got == {"absent": 3, "single": 4, "shared_below_root": 4, "shared_root": 2, "shared_depths": {0, 1, 2, 3}}


def test_tree_builders():
    parent, depth, leaf = cases.tree_from_paths(cases.cluster_paths([-1, 0, 0, 0, 0, 0, 1, 1, 2, 2, 2], [0, 0, 1, 2, 3, 4, 0, 1, 1, 3, 4]))
    assert parent[0] == 0 and all(parent[v] < v for v in range(1, parent.size))
    assert all(depth[v] == depth[parent[v]] + 1 for v in range(1, parent.size)) and int(depth.max()) == 3
    assert leaf[1] == leaf[2] and depth[leaf[7]] == 2 and leaf[9] == 0 and depth[leaf[10]] == 1
    parent, depth, leaf = cases.chain_tree(40)
    assert int(depth.max()) == cases.MAX_DEPTH == _lib.YH_LCA_MAX_DEPTH and parent.tolist() == [0] + list(range(16))
    assert ancestor_sets(parent)[1] == depth.tolist() and int(leaf.max()) == 16


def test_edge_database_holds_lists_of_every_length():
    rng = np.random.default_rng(5)
    refs, parent, depth, leaf, cs = cases.edge_database(rng, 2 ** 42)
    values, offsets = cases.pack(refs)
    hashes = np.array(sorted(h for h, _, _ in cs), dtype=np.uint64)
    by_hash = {h: (L, want) for h, L, want in cs}
    _, lo, hi = holders_of(values, offsets, hashes)
    nodes, _ = lca_oracle(values, offsets, parent, leaf, hashes)
    assert [int(b - a) for a, b in zip(lo, hi)] == [by_hash[int(h)][0] for h in hashes]
    assert nodes.tolist() == [by_hash[int(h)][1] for h in hashes]
    assert sorted({L for _, L, _ in cs}) == list(cases.EDGE_LENGTHS) and {depth[w] for _, _, w in cs} == {0, 1, 3}


def test_header_binding_and_library_agree_on_the_four_entries():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "yacht_hip.h")) as f:
        text = f.read()
    for name in ENTRIES:
        assert f"int {name}(yh_db* db, " in text, name
    assert "#define YH_ABI_VERSION 8" in text and "#define YH_LCA_MAX_DEPTH 16" in text and "#define YH_LCA_NONE 0xffffffffu" in text
    assert "yh_lca / yh_lca_device" in text  # its row of the interleaving table
    assert [len(_lib.SIGNATURES[name][1]) for name in ENTRIES] == [5, 3, 6, 6]
    assert _lib.YH_LCA_NONE == NONE == cases.NONE
    lib = _lib.load()
    assert lib.yh_abi_version() == 8 and all(hasattr(lib, name) for name in ENTRIES)
    buf = np.zeros(16, dtype=np.uint64)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.yh_db_set_taxonomy(None, p, p, 1, p) == _lib.YH_ERR_INVALID_ARG
    assert lib.yh_db_get_taxonomy(None, None, None) == _lib.YH_ERR_INVALID_ARG
    assert lib.yh_lca(None, p, None, 0, p, p) == _lib.YH_ERR_INVALID_ARG
    assert lib.yh_lca_device(None, p, None, 0, None, p) == _lib.YH_ERR_INVALID_ARG
    assert b"null" in lib.yh_last_error()
