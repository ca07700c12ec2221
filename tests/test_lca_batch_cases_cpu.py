"""The blocks of the batched lineage pass without a GPU: every case of tests/lca_batch_cases.py still holds what it is named
for, judged by the oracle alone, and the three new symbols as header, binding and shared object agree on them."""
import ctypes as C
import os

import lca_batch_cases as batch
import lca_cases as cases
import numpy as np
import pytest
from lca_oracle import NONE, holders_of, lca_oracle

from yacht_amd import _lib
from yacht_amd.engine import LCA_ROW_DTYPE

ENTRIES = ("yh_lca_batch_device", "yh_lca_batch", "yh_lca_rows_pack_device")
T = batch.T


@pytest.fixture(scope="module")
def by_name():
    return {c.name: c for c in batch.build_cases()}


def _oracle(case, s):
    parent, _depth, leaf = case.tree
    return lca_oracle(case.values, case.offsets, parent, leaf, case.samples[s], None if case.abunds is None else case.abunds[s])


def test_every_block_is_well_formed(by_name):
    assert len(by_name) == 10
    for case in by_name.values():
        parent, depth, leaf = case.tree
        assert 1 <= len(case.samples) <= _lib.YH_BATCH_MAX_SAMPLES and leaf.size == case.offsets.size - 1, case.name
        assert parent[0] == 0 and all(parent[v] < v for v in range(1, parent.size)) and int(depth.max()) <= cases.MAX_DEPTH
        for s, smp in enumerate(case.samples):
            assert smp.dtype == np.uint64 and (np.diff(smp.astype(object)) > 0).all(), (case.name, s)
            if case.abunds is not None and case.abunds[s] is not None:
                assert case.abunds[s].dtype == np.uint32 and case.abunds[s].size == smp.size, (case.name, s)


def test_tile_edges_and_block_sizes(by_name):
    assert T == 1024
    edges = by_name["tile_edges"]
    assert [s.size for s in edges.samples] == [0, 1, T - 1, T, 0, T + 1, 2 * T + 1, 0]
    assert edges.abunds[3] is None and edges.abunds[2] is not None  # a sample without abundances beside ones with
    assert [len(by_name[n].samples) for n in ("one_sample", "two_samples", "full_block")] == [1, 2, 256]
    assert by_name["one_sample"].samples[0].size > 3 * T and by_name["two_samples_without_abundances"].abunds is None
    full = by_name["full_block"]
    assert all(20 <= s.size <= 60 for s in full.samples) and sum(a is None for a in full.abunds) == 86
    # every class of hash is met in the blocks that are long enough to meet them
    for name in ("tile_edges", "one_sample"):
        case = by_name[name]
        parent, _, leaf = case.tree
        big = max(range(len(case.samples)), key=lambda s: case.samples[s].size)
        nodes, _ = _oracle(case, big)
        _, lo, hi = holders_of(case.values, case.offsets, case.samples[big])
        shared = (hi - lo) >= 2
        assert (nodes == NONE).sum() >= 100 and ((hi - lo) == 1).sum() >= 100, name
        assert (shared & (nodes != 0)).sum() >= 100 and (shared & (nodes == 0)).sum() >= 20, name


def test_above_and_missing(by_name):
    case = by_name["above_and_missing"]
    above, hit, miss = case.samples
    assert int(above.min()) > int(case.values.max()) and int(miss.max()) < int(case.values.max()) and miss.size > 1000
    assert (_oracle(case, 0)[0] == NONE).all() and (_oracle(case, 2)[0] == NONE).all() and not _oracle(case, 2)[1].any()
    assert (_oracle(case, 1)[0] != NONE).sum() >= 400


def test_crowded_tile_meets_more_nodes_than_the_table_has_slots(by_name):
    case = by_name["crowded_table"]
    nodes, _ = _oracle(case, 0)
    assert case.samples[0].size > T and (nodes != NONE).all()
    assert len(set(nodes[:T].tolist())) > batch.TABLE_SLOTS  # the first tile alone


def test_sums_pass_32_bits(by_name):
    case = by_name["sums_pass_32_bits"]
    nodes, counts = _oracle(case, 0)
    assert nodes.tolist() == cases.HAND_NODES.tolist()
    assert int(counts[0, 1]) == 3 * batch.U32_MAX > 2 ** 32 and int(counts[6, 1]) == 2 * batch.U32_MAX > 2 ** 32
    hand = by_name["hand_written"]
    assert _oracle(hand, 0)[1].tolist() == cases.HAND_COUNTS.tolist() and hand.samples[2].size == 0


def test_posting_list_edges(by_name):
    case = by_name["posting_list_edges"]
    _, lo, hi = holders_of(case.values, case.offsets, case.samples[0])
    assert set(cases.EDGE_LENGTHS) <= set((hi - lo).tolist())
    parent, depth, _ = case.tree
    nodes = _oracle(case, 1)[0]
    assert {int(depth[v]) for v in nodes.tolist()} == {0, 1, 3}


def test_header_binding_and_library_agree_on_the_three_entries():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "yacht_hip.h")) as f:
        text = f.read()
    for name in ENTRIES:
        assert f"int {name}(yh_db* db, " in text, name
    assert "#define YH_ABI_VERSION 8" in text and f"#define YH_LCA_BATCH_TILE {T}" in text and "typedef struct yh_lca_row" in text
    assert "yh_lca_batch / yh_lca_batch_device" in text  # its row of the interleaving table
    assert [len(_lib.SIGNATURES[name][1]) for name in ENTRIES] == [8, 7, 6]
    assert LCA_ROW_DTYPE.itemsize == 24 and LCA_ROW_DTYPE.names == ("sample", "node", "n_hashes", "w_hashes")
    lib = _lib.load()
    assert lib.yh_abi_version() == 8 and all(hasattr(lib, name) for name in ENTRIES)
    buf = np.zeros(16, dtype=np.uint64)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.yh_lca_batch_device(None, p, p, None, 1, 0, None, p) == _lib.YH_ERR_INVALID_ARG
    assert lib.yh_lca_batch(None, p, p, None, 1, None, p) == _lib.YH_ERR_INVALID_ARG
    assert lib.yh_lca_rows_pack_device(None, p, 1, p, 1, p) == _lib.YH_ERR_INVALID_ARG
    assert b"null" in lib.yh_last_error()
