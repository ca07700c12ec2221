"""RefDB.lca_batch / lca_batch_device / lca_rows_pack_device (yh_lca_batch, yh_lca_batch_device, yh_lca_rows_pack_device) on
the GPU.  On every block of tests/lca_batch_cases.py the nodes and the dense counts equal, word for word, the per-sample
RefDB.lca calls and the brute-force oracle (tests/lca_oracle.py); the rows equal np.nonzero of the dense counts in (sample,
node) order.  Exact equality everywhere."""
import lca_batch_cases as batch
import lca_cases as cases
import numpy as np
import pytest
from lca_oracle import NONE, lca_oracle

from yacht_amd import _lib
from yacht_amd.engine import LCA_ROW_DTYPE, RefDB, YachtHipError, pack_csr

pytestmark = pytest.mark.gpu

CASES = batch.build_cases()
FILL = 0x55555555


@pytest.fixture(scope="module")
def wanted():
    """Per case the oracle's (nodes, counts) of every sample, computed once."""
    out = {}
    for case in CASES:
        parent, _depth, leaf = case.tree
        out[case.name] = [lca_oracle(case.values, case.offsets, parent, leaf, smp, None if case.abunds is None else case.abunds[s])
                          for s, smp in enumerate(case.samples)]
    return out


def _up(a, view):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(view) if a.size else np.zeros(1, view)).to("cuda:0")


def _cat_abund(samples, abunds):
    if abunds is None or all(a is None for a in abunds):
        return None
    return np.concatenate([np.ones(s.size, np.uint32) if a is None else a for s, a in zip(samples, abunds)]).astype(np.uint32)


class _Block:
    """A block resident on the device, as the cohort command holds it."""

    def __init__(self, samples, abunds):
        self.values, self.offsets = pack_csr(samples)
        self.b, self.total = len(samples), int(self.values.size)
        self.d_s, self.d_o = _up(self.values, np.int64), _up(self.offsets, np.int64)
        cat = _cat_abund(samples, abunds)
        self.d_a = None if cat is None else _up(cat, np.int32)

    def run(self, db, d_counts, d_node=None, abund=True):
        db.lca_batch_device(self.d_s.data_ptr(), self.d_o.data_ptr(), self.d_a.data_ptr() if abund and self.d_a is not None else 0,
                            self.b, self.total, 0 if d_node is None else d_node.data_ptr(), d_counts.data_ptr())


def _counts_of(d_counts, b, n_nodes):
    return d_counts.cpu().numpy().view(np.uint64)[:2 * b * n_nodes].reshape(b, n_nodes, 2)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_every_block_equals_the_single_calls_and_the_oracle(hip_lib, wanted, case):
    import torch

    parent, depth, leaf = case.tree
    n_nodes, b = parent.size, len(case.samples)
    want = wanted[case.name]
    want_nodes, want_counts = [w[0] for w in want], np.stack([w[1] for w in want])
    with RefDB(case.values, case.offsets) as db:
        db.set_taxonomy(parent, depth, leaf)
        # the single call, sample by sample, is the oracle's
        for s in range(0, b, max(1, b // 8)):
            one = db.lca(case.samples[s], None if case.abunds is None else case.abunds[s])
            assert np.array_equal(one[0], want_nodes[s]) and np.array_equal(one[1], want_counts[s]), (case.name, "single", s)
        # the host form
        nodes, counts = db.lca_batch(case.samples, case.abunds)
        assert counts.dtype == np.uint64 and counts.shape == (b, n_nodes, 2) and len(nodes) == b
        for s in range(b):
            assert nodes[s].dtype == np.uint32 and np.array_equal(nodes[s], want_nodes[s]), (case.name, "nodes", s)
        assert np.array_equal(counts, want_counts), (case.name, "counts", np.argwhere(counts != want_counts)[:5])
        none, only = db.lca_batch(case.samples, case.abunds, want_nodes=False)
        assert none is None and np.array_equal(only, want_counts), (case.name, "counts only")
        plain = db.lca_batch(case.samples)[1]  # no abundances: the second column is the first
        assert np.array_equal(plain[:, :, 0], want_counts[:, :, 0]) and np.array_equal(plain[:, :, 1], plain[:, :, 0]), (case.name, "plain")
        # the device form: the same words; d_node = NULL and d_abund = NULL
        blk = _Block(case.samples, case.abunds)
        d_counts = torch.full((2 * b * n_nodes + 8,), -1, dtype=torch.int64, device="cuda:0")
        d_node = torch.full((blk.total + 8,), FILL, dtype=torch.int32, device="cuda:0")
        blk.run(db, d_counts, d_node)
        db.synchronize()
        assert np.array_equal(_counts_of(d_counts, b, n_nodes), want_counts), (case.name, "device counts")
        got = d_node.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:blk.total], np.concatenate(want_nodes)) and (got[blk.total:] == FILL).all(), (case.name, "device nodes")
        assert (d_counts[2 * b * n_nodes:] == -1).all()  # nothing behind the block's cells is touched
        d_node.fill_(FILL)
        d_counts.fill_(-1)
        blk.run(db, d_counts, None, abund=False)
        db.synchronize()
        got = _counts_of(d_counts, b, n_nodes)
        assert np.array_equal(got, plain) and bool((d_node == FILL).all()), (case.name, "NULL node and abund")


def test_a_smaller_block_after_a_larger_one_and_a_replaced_taxonomy(hip_lib, wanted):
    import torch

    case = next(c for c in CASES if c.name == "tile_edges")
    parent, depth, leaf = case.tree
    n_nodes = parent.size
    five, three = [1, 2, 3, 5, 6], [6, 0, 2]  # (samples of the case by index)
    with RefDB(case.values, case.offsets) as db:
        db.set_taxonomy(parent, depth, leaf)
        d_counts = torch.full((2 * 5 * n_nodes,), -1, dtype=torch.int64, device="cuda:0")
        for pick in (five, three):
            blk = _Block([case.samples[i] for i in pick], [case.abunds[i] for i in pick])
            blk.run(db, d_counts)
            db.synchronize()
            want = np.stack([wanted[case.name][i][1] for i in pick])
            assert np.array_equal(_counts_of(d_counts, len(pick), n_nodes), want), pick
        # (the cells of samples 3 and 4 of the larger block are outside the smaller call: they keep what they held)
        tail = d_counts.cpu().numpy().view(np.uint64).reshape(5, n_nodes, 2)[3:]
        assert np.array_equal(tail, np.stack([wanted[case.name][i][1] for i in five[3:]]))
        # another taxonomy between two calls: the chain, where the answer is the shallowest holder's node
        chain = cases.chain_tree(leaf.size)
        db.set_taxonomy(*chain)
        samples, abunds = [case.samples[i] for i in three], [case.abunds[i] for i in three]
        nodes, counts = db.lca_batch(samples, abunds)
        assert counts.shape == (3, 17, 2)
        for s in range(3):
            again = lca_oracle(case.values, case.offsets, chain[0], chain[2], samples[s], abunds[s])
            assert np.array_equal(nodes[s], again[0]) and np.array_equal(counts[s], again[1]), s
        assert not np.array_equal(nodes[0], wanted[case.name][6][0])


@pytest.mark.parametrize("name", ["tile_edges", "full_block", "hand_written"])
def test_rows_pack(hip_lib, wanted, name):
    import torch

    case = next(c for c in CASES if c.name == name)
    parent, depth, leaf = case.tree
    n_nodes, b = parent.size, len(case.samples)
    dense = np.stack([w[1] for w in wanted[name]])
    smp, node = np.nonzero(dense[:, :, 0])  # row-major: ascending (sample, node)
    want = np.zeros(smp.size, dtype=LCA_ROW_DTYPE)
    want["sample"], want["node"], want["n_hashes"], want["w_hashes"] = smp, node, dense[smp, node, 0], dense[smp, node, 1]
    k = int(want.size)
    assert k >= 5
    with RefDB(case.values, case.offsets) as db:
        db.set_taxonomy(parent, depth, leaf)
        blk = _Block(case.samples, case.abunds)
        d_counts = torch.zeros(2 * b * n_nodes, dtype=torch.int64, device="cuda:0")
        blk.run(db, d_counts)
        for cap in (k, k + 3, k - 1, 1, 0):
            d_rows = torch.full((3 * (k + 4),), -1, dtype=torch.int64, device="cuda:0")
            d_n = torch.full((2,), -1, dtype=torch.int64, device="cuda:0")
            db.lca_rows_pack_device(d_counts.data_ptr(), b, d_rows.data_ptr() if cap else 0, cap, d_n.data_ptr())
            db.synchronize()
            assert d_n.tolist() == [k, -1], (name, cap)  # the true count, whatever the capacity
            rows = d_rows.cpu().numpy()
            written = min(cap, k)
            assert np.array_equal(rows[:3 * written].view(LCA_ROW_DTYPE), want[:written]), (name, cap)
            assert (rows[3 * written:] == -1).all(), (name, cap)  # rows behind the count or the capacity are not written
        # a block without a single hit: no row
        d_counts.zero_()
        d_n = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
        db.lca_rows_pack_device(d_counts.data_ptr(), b, 0, 0, d_n.data_ptr())
        db.synchronize()
        assert d_n.tolist() == [0]


def test_errors_and_the_empty_database(hip_lib):
    import torch

    case = next(c for c in CASES if c.name == "hand_written")
    parent, depth, leaf = case.tree
    d = torch.zeros(4096, dtype=torch.int64, device="cuda:0")
    p = d.data_ptr()

    def code(call):
        with pytest.raises(YachtHipError) as ei:
            call()
        return ei.value.code

    with RefDB(case.values, case.offsets) as db:
        # no taxonomy set
        assert code(lambda: db.lca_batch(case.samples)) == _lib.YH_ERR_UNSUPPORTED
        assert code(lambda: db.lca_batch_device(p, p, 0, 1, 0, 0, p)) == _lib.YH_ERR_UNSUPPORTED
        assert code(lambda: db.lca_rows_pack_device(p, 1, p, 4, p)) == _lib.YH_ERR_UNSUPPORTED
        db.set_taxonomy(parent, depth, leaf)
        for n in (0, _lib.YH_BATCH_MAX_SAMPLES + 1):
            assert code(lambda: db.lca_batch_device(p, p, 0, n, 0, 0, p)) == _lib.YH_ERR_INVALID_ARG
            assert code(lambda: db.lca_rows_pack_device(p, n, p, 4, p)) == _lib.YH_ERR_INVALID_ARG
        assert code(lambda: db.lca_batch_device(p, p, 0, 1, 2 ** 32, 0, p)) == _lib.YH_ERR_INVALID_ARG
        assert code(lambda: db.lca_batch_device(p, p, 0, 1, 0, 0, 0)) == _lib.YH_ERR_INVALID_ARG  # no counts
        with pytest.raises(ValueError, match="1..256"):
            db.lca_batch([])
        with pytest.raises(ValueError, match="1..256"):
            db.lca_batch([case.samples[0]] * 257)
        with pytest.raises(ValueError, match="abundance arrays"):
            db.lca_batch(case.samples, [None])
        assert code(lambda: db.lca_batch([case.samples[0], np.array([3, 8, 5], np.uint64)])) == _lib.YH_ERR_UNSORTED
        # total_hashes == 0: zero counts whatever the device offsets say, and no node written
        d.fill_(-1)
        offs = _up(np.array([0, 3, 5], np.uint64), np.int64)
        db.lca_batch_device(p, offs.data_ptr(), 0, 2, 0, p + 8 * 2048, p)
        db.synchronize()
        n_cells = 2 * 2 * parent.size
        assert not d[:n_cells].any() and bool((d[n_cells:] == -1).all())
    # an empty database: zero counts, nodes untouched
    with RefDB(np.zeros(0, np.uint64), np.zeros(3, np.uint64)) as db:
        db.set_taxonomy([0, 0], [0, 1], [1, 0])
        nodes, counts = db.lca_batch([np.array([3, 5], np.uint64), np.array([4], np.uint64)], [np.array([4, 4]), None])
        assert [n.tolist() for n in nodes] == [[NONE, NONE], [NONE]] and counts.shape == (2, 2, 2) and not counts.any()
