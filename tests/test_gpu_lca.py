"""RefDB.set_taxonomy / RefDB.lca (yh_db_set_taxonomy, yh_lca, yh_lca_device) on the GPU against a brute-force oracle
(tests/lca_oracle.py: holders from the CSR, LCA by intersecting ancestor sets).  Exact equality everywhere: every node word
and both columns of the counts, with abundances, without them, and counts-only.

Before the device is asked, the oracle's own answer for a sample must show at least 100 sample hashes in each class a kernel
can get wrong -- absent, single holder, shared resolving below the root, shared resolving to the root -- and shared answers
at three depths or more, so that no class passes unseen (1 of each in the hand-written database, whose nodes are spelled out
in tests/lca_cases.py)."""
import ctypes as C

import lca_cases as cases
import numpy as np
import pytest
from lca_oracle import NONE, census, counts_from_nodes, lca_oracle

from yacht_amd import _lib, synth
from yacht_amd.engine import RefDB, YH_DB_NO_DIRECTORY, YH_DB_NO_INDEX, YachtHipError

pytestmark = pytest.mark.gpu

NARROW = 2 ** 22  # "scaled" whose hash range (2^42) lets a database of ~10^6 distinct hashes take the COMPACT buckets
RETENTIONS = (1, 0.9, 0.5, 0.25, 0.1)


def _assert_census(values, offsets, parent, leaf, sample, at_least=100, depths=3):
    got = census(values, offsets, parent, leaf, sample)
    print("census", got)
    assert min(got["absent"], got["single"], got["shared_below_root"], got["shared_root"]) >= at_least, got
    assert len(got["shared_depths"]) >= depths, got
    return got


def _check(db, values, offsets, parent, leaf, sample, abund, what, want_nodes=None):
    """lca with and without abundances and counts-only, all against the oracle; returns (nodes, counts with abund)."""
    if want_nodes is None:
        want_nodes = lca_oracle(values, offsets, parent, leaf, sample)[0]
    n_nodes = len(parent)
    for ab in (abund, None):
        nodes, counts = db.lca(sample, ab)
        assert nodes.dtype == np.uint32 and nodes.shape == (len(sample),) and counts.dtype == np.uint64 and counts.shape == (n_nodes, 2)
        assert np.array_equal(nodes, want_nodes), (what, "nodes", ab is None, np.flatnonzero(nodes != want_nodes)[:10])
        want_counts = counts_from_nodes(want_nodes, n_nodes, ab)
        assert np.array_equal(counts, want_counts), (what, "counts", ab is None, np.flatnonzero((counts != want_counts).any(axis=1))[:10])
        none, only = db.lca(sample, ab, want_nodes=False)  # d_node = NULL
        assert none is None and np.array_equal(only, counts), (what, "counts only", ab is None)
    return db.lca(sample, abund)


def _cluster_tree(order, n_independent, per_cluster=len(RETENTIONS)):
    """The taxonomy of lca_cases.cluster_paths over references shuffled by `order` (position i holds original reference
    order[i]; the originals behind n_independent are clusters of per_cluster consecutive members)."""
    order = np.asarray(order)
    clustered = order >= n_independent
    cluster_of = np.where(clustered, (order - n_independent) // per_cluster, -1)
    member_of = np.where(clustered, (order - n_independent) % per_cluster, 0)
    return cases.tree_from_paths(cases.cluster_paths(cluster_of, member_of))


@pytest.fixture(scope="module")
def big():
    """test_gpu_explain.py's narrow-range database: 300 independent references plus 12 clusters, shuffled, > 2^20 distinct
    hashes, so compact buckets + filter.  The cluster members are spread over species, genera and families."""
    rng = np.random.default_rng(601)
    refs = synth.independent_refs(rng, 300, 5000, 0.35, 500, 20000, scaled=NARROW) + \
        synth.clustered_refs(rng, 12, RETENTIONS, 5000, scaled=NARROW)
    order = rng.permutation(len(refs))
    refs = [refs[i] for i in order]
    values, offsets = synth.pack(refs)
    parent, depth, leaf = _cluster_tree(order, 300)
    return rng, refs, values, offsets, parent, depth, leaf, np.flatnonzero(order >= 300)


def _big_sample(rng, refs, clustered, n_sample):
    """Every cluster member and twenty other references at coverage 0.3, and noise up to n_sample hashes."""
    present = np.union1d(clustered, rng.choice(len(refs), size=20, replace=False))
    return synth.sample_from_refs(rng, refs, present, 0.3, n_sample, scaled=NARROW)


@pytest.mark.parametrize("n_sample", [120_000, 300_000, 600_000])  # the three tile shapes of the lookup
def test_compact_buckets_and_filter_against_the_oracle(hip_lib, big, n_sample):
    rng, refs, values, offsets, parent, depth, leaf, clustered = big
    sample = _big_sample(rng, refs, clustered, n_sample)
    lo = {120_000: 100_000, 300_000: 262_144, 600_000: 524_288}[n_sample]
    hi = {120_000: 262_144, 300_000: 524_288, 600_000: 1 << 40}[n_sample]
    assert lo <= sample.size < hi  # (the shape this case is for)
    abund = rng.integers(1, 1001, sample.size)
    _assert_census(values, offsets, parent, leaf, sample)
    with RefDB(values, offsets) as db:
        assert db.info()["filter_bytes"] > 0 and db.info()["n_shared_distinct"] > 1000
        before = db.info()
        db.set_taxonomy(parent, depth, leaf)
        assert db.info() == before  # (yh_db_info is unchanged)
        tax = db.taxonomy_info()
        assert tax["n_nodes"] == parent.size and tax["device_bytes"] >= 5 * parent.size + 4 * len(refs) + 4 * before["n_shared_distinct"]
        nodes, counts = _check(db, values, offsets, parent, leaf, sample, abund, f"big {n_sample}")
        assert int(counts[:, 0].sum()) == int((nodes != NONE).sum())


def test_hand_written_database(hip_lib):
    v, o = cases.pack(cases.HAND_REFS)
    got = _assert_census(v, o, cases.HAND_PARENT, cases.HAND_LEAF, cases.HAND_SAMPLE, at_least=1, depths=4)
    assert got["absent"] == 3 and int((cases.HAND_SAMPLE > v.max()).sum()) == 1  # one of them above the largest hash
    with RefDB(v, o) as db:
        db.set_taxonomy(cases.HAND_PARENT, cases.HAND_DEPTH, cases.HAND_LEAF)
        nodes, counts = _check(db, v, o, cases.HAND_PARENT, cases.HAND_LEAF, cases.HAND_SAMPLE, cases.HAND_ABUND, "hand written",
                               want_nodes=cases.HAND_NODES)
        assert nodes.tolist() == cases.HAND_NODES.tolist() and counts.tolist() == cases.HAND_COUNTS.tolist()
        plain = db.lca(cases.HAND_SAMPLE)[1]
        assert plain[:, 0].tolist() == plain[:, 1].tolist() == cases.HAND_COUNTS[:, 0].tolist()


def test_small_database_with_the_five_entry_buckets(hip_lib):
    """synth.config2 at scaled = 1000 keeps the full-hash buckets and their directory; clusters at the same scale are appended
    for the shared classes."""
    values, offsets, sample = synth.config2(seed=603, n_refs=150, n_sample=200_000)
    rng = np.random.default_rng(6031)  # (another stream than config2's: the same seed would repeat its hashes)
    refs = [values[int(offsets[i]):int(offsets[i + 1])] for i in range(len(offsets) - 1)]
    clusters = synth.clustered_refs(rng, 6, RETENTIONS, 4000)
    refs = refs + clusters
    values, offsets = synth.pack(refs)
    parent, depth, leaf = _cluster_tree(np.arange(len(refs)), 150)
    sample = np.union1d(sample, synth.sample_from_refs(rng, clusters, list(range(len(clusters))), 0.5, 1000))
    abund = rng.integers(1, 1001, sample.size)
    _assert_census(values, offsets, parent, leaf, sample)
    with RefDB(values, offsets) as db:
        assert db.info()["filter_bytes"] == 0
        db.set_taxonomy(parent, depth, leaf)
        _check(db, values, offsets, parent, leaf, sample, abund, "five-entry buckets")


def test_clustered_references_walk_the_posting_lists(hip_lib):
    rng = np.random.default_rng(602)
    refs = synth.clustered_refs(rng, 30, RETENTIONS, 20_000, scaled=NARROW)
    values, offsets = synth.pack(refs)
    parent, depth, leaf = _cluster_tree(np.arange(len(refs)), 0)
    cov = np.full(len(refs), 0.02)
    cov[4] = 1.0
    sample = synth.sample_from_refs(rng, refs, list(range(len(refs))), cov, 150_000, scaled=NARROW)
    abund = rng.integers(1, 1001, sample.size)
    _assert_census(values, offsets, parent, leaf, sample)
    with RefDB(values, offsets) as db:
        assert db.info()["n_shared_distinct"] > 10_000
        db.set_taxonomy(parent, depth, leaf)
        _check(db, values, offsets, parent, leaf, sample, abund, "clustered")


def test_one_reference(hip_lib):
    """n_shared == 0: yh_db_set_taxonomy launches nothing, and every known hash is the reference's own node."""
    rng = np.random.default_rng(604)
    ref = synth.random_sketch(rng, 4000, synth.max_hash_for_scaled(1000))
    values, offsets = synth.pack([ref])
    sample = np.union1d(ref[::3], synth.random_sketch(rng, 5000, synth.max_hash_for_scaled(1000)))
    abund = rng.integers(1, 1001, sample.size)
    parent, depth, leaf = cases.tree_from_paths([("K", "P", "S")])
    got = census(values, offsets, parent, leaf, sample)
    assert got["absent"] >= 100 and got["single"] >= 100 and got["shared_below_root"] == got["shared_root"] == 0
    with RefDB(values, offsets) as db:
        assert db.info()["n_shared_distinct"] == 0
        db.set_taxonomy(parent, depth, leaf)
        nodes, counts = _check(db, values, offsets, parent, leaf, sample, abund, "one reference")
        assert set(nodes.tolist()) == {3, NONE} and counts[:3].tolist() == [[0, 0]] * 3 and counts[3, 0] == -(-ref.size // 3)


def test_posting_list_edges(hip_lib):
    """Lists of 2, 3, 4, 5, 63, 64, 65 and 300 holders (the four-at-a-time clamp in every phase), the holder that lifts the
    fold placed LAST in the list: the answer is a species, a family and the root in turn."""
    rng = np.random.default_rng(607)
    mh = synth.max_hash_for_scaled(NARROW)
    refs, parent, depth, leaf, cs = cases.edge_database(rng, mh)
    values, offsets = synth.pack(refs)
    wanted = np.array(sorted(h for h, _, _ in cs), dtype=np.uint64)
    sample = np.union1d(np.union1d(wanted, np.concatenate([r[::2] for r in refs])), synth.random_sketch(rng, 20_000, mh))
    abund = rng.integers(1, 1001, sample.size)
    got = census(values, offsets, parent, leaf, sample)
    assert got["shared_below_root"] >= 32 and got["shared_root"] >= 16 and got["shared_depths"] >= {0, 1, 3}, got
    with RefDB(values, offsets) as db:
        db.set_taxonomy(parent, depth, leaf)
        nodes, _ = _check(db, values, offsets, parent, leaf, sample, abund, "posting-list edges")
        at = {int(h): i for i, h in enumerate(sample.tolist())}
        for h, L, want in cs:
            assert nodes[at[h]] == want, (h, L, want, int(nodes[at[h]]))


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(606)
    refs = synth.clustered_refs(rng, 8, RETENTIONS, 3000, scaled=NARROW) + synth.independent_refs(rng, 104, 3000, 0.3, 500, 8000, scaled=NARROW)
    values, offsets = synth.pack(refs)
    order = np.concatenate([np.arange(104, 144), np.arange(104)])  # (the clusters come first here)
    parent, depth, leaf = _cluster_tree(order, 104)
    sample = synth.sample_from_refs(rng, refs, list(range(60)), 0.5, 60_000, scaled=NARROW)
    return rng, refs, values, offsets, parent, depth, leaf, sample


def test_tree_edges(hip_lib, small):
    rng, refs, values, offsets, parent, depth, leaf, sample = small
    abund = rng.integers(1, 1001, sample.size)
    with RefDB(values, offsets) as db:
        # one node: every known hash goes to node 0
        one = (np.zeros(1, np.uint32), np.zeros(1, np.uint8), np.zeros(len(refs), np.uint32))
        db.set_taxonomy(*one)
        nodes, counts = _check(db, values, offsets, one[0], one[2], sample, abund, "one node")
        known = np.isin(sample, values)
        assert np.array_equal(nodes == 0, known) and counts.tolist() == [[int(known.sum()), int(abund[known].sum())]]
        # a chain of depth exactly YH_LCA_MAX_DEPTH: the deepest pairs are lifted sixteen times
        chain = cases.chain_tree(len(refs))
        assert int(chain[1].max()) == _lib.YH_LCA_MAX_DEPTH
        got = census(values, offsets, chain[0], chain[2], sample)
        assert got["shared_below_root"] >= 100 and got["shared_root"] >= 100 and len(got["shared_depths"]) >= 3, got
        db.set_taxonomy(*chain)
        _check(db, values, offsets, chain[0], chain[2], sample, abund, "chain")


def test_crowded_table_takes_the_global_atomics(hip_lib):
    """2 048 references, each a species of its own, and a sample that is the whole database: a tile of 2 048 hashes (1 024
    table slots) or of 256 (256 slots, two probes each) meets more nodes than its table holds."""
    rng = np.random.default_rng(608)
    mh = synth.max_hash_for_scaled(NARROW)
    pool = synth.random_sketch(rng, 2048 * 300, mh)
    rng.shuffle(pool)
    refs = [np.sort(pool[j::2048]) for j in range(2048)]
    values, offsets = synth.pack(refs)
    parent, depth, leaf = cases.tree_from_paths([(f"F{j % 5}", f"G{j % 64}", f"S{j}") for j in range(2048)])
    assert len(set(leaf.tolist())) == 2048
    sample = np.sort(pool)
    assert sample.size >= 524_288
    abund = rng.integers(1, 1001, sample.size)
    want = lca_oracle(values, offsets, parent, leaf, sample)[0]
    assert (want != NONE).all()
    with RefDB(values, offsets) as db:
        db.set_taxonomy(parent, depth, leaf)
        for n in (sample.size, 100_000):
            per_tile = 2048 if n >= 524_288 else 256
            distinct = [len(set(want[t:t + per_tile].tolist())) for t in range(0, n - per_tile, per_tile)]
            assert min(distinct) > per_tile // 2, min(distinct)  # (every tile meets more nodes than half of its hashes)
            _check(db, values, offsets, parent, leaf, sample[:n], abund[:n], f"crowded {n}", want_nodes=want[:n])


def test_cross_checks_with_the_existing_entries(hip_lib, small):
    rng, refs, values, offsets, parent, depth, leaf, sample = small
    abund = rng.integers(1, 1001, sample.size)
    with RefDB(values, offsets) as db:
        db.set_taxonomy(parent, depth, leaf)
        _, counts = db.lca(sample, abund)
        totals = db.explain(sample, np.zeros(len(refs), np.uint8), abund)[1]
        assert int(counts[:, 0].sum()) == int(totals[7, 0]) > 1000 and int(counts[:, 1].sum()) == int(totals[7, 1])
        # a star tree, every reference a child of the root: a node's counts are abund's w_match, the root holds the shared hashes
        n = len(refs)
        star = (np.zeros(n + 1, np.uint32), np.array([0] + [1] * n, np.uint8), np.arange(1, n + 1, dtype=np.uint32))
        db.set_taxonomy(*star)
        nodes, counts = db.lca(sample, abund)
        w_match = db.abundance(sample, abund)[1]
        assert np.array_equal(counts[1:, 1], w_match) and np.array_equal(counts[1:, 0], db.run_counts(sample)[2])
        flags = db.explain(sample, np.ones(n, np.uint8))[0]
        assert int(counts[0, 0]) == int((nodes == 0).sum()) > 100 and np.array_equal(nodes != NONE, flags != 0)


def test_edges_and_errors(hip_lib, small):
    import torch

    rng, refs, values, offsets, parent, depth, leaf, sample = small
    mh = synth.max_hash_for_scaled(NARROW)
    n = len(refs)
    with RefDB(values, offsets) as db:
        # no taxonomy set
        assert db.taxonomy_info() == {"n_nodes": 0, "device_bytes": 0}
        with pytest.raises(YachtHipError) as ei:
            db.lca(sample)
        assert ei.value.code == _lib.YH_ERR_UNSUPPORTED
        db.set_taxonomy(parent, depth, leaf)
        want = lca_oracle(values, offsets, parent, leaf, sample)
        # an empty sample: zero counts, no node
        nodes, counts = db.lca(np.zeros(0, np.uint64), np.zeros(0, np.int64))
        assert nodes.size == 0 and counts.shape == (parent.size, 2) and not counts.any()
        # a sample wholly above the largest hash of the database
        above = np.unique(rng.integers(int(values.max()) + 1, 2 * mh, 5000, dtype=np.uint64))
        nodes, counts = db.lca(above, np.full(above.size, 7))
        assert (nodes == NONE).all() and not counts.any()
        # an unsorted sample in the host form
        with pytest.raises(YachtHipError) as ei:
            db.lca(np.array([3, 8, 5], np.uint64))
        assert ei.value.code == _lib.YH_ERR_UNSORTED
        # every violation is refused, and the earlier taxonomy still answers
        p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731

        def refused(par, dep, lf):
            par, dep, lf = np.ascontiguousarray(par, np.uint32), np.ascontiguousarray(dep, np.uint8), np.ascontiguousarray(lf, np.uint32)
            assert db._lib.yh_db_set_taxonomy(db._h, p(par), p(dep), par.size, p(lf)) == _lib.YH_ERR_INVALID_ARG
            assert db.taxonomy_info()["n_nodes"] == parent.size
            got = db.lca(sample)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])

        for v, bad in ((0, 1), (1, 1), (5, 5), (5, 9)):  # the root's parent; a node its own parent; a later node as parent
            par = parent.copy()
            par[v] = bad
            refused(par, depth, leaf)
        for v, bad in ((0, 1), (1, 2), (int(np.flatnonzero(depth == 3)[0]), 2)):  # the root's depth; a depth that skips; one too shallow
            dep = depth.copy()
            dep[v] = bad
            refused(parent, dep, leaf)
        deep = cases.chain_tree(n)  # one level deeper than YH_LCA_MAX_DEPTH
        refused(np.append(deep[0], 16), np.append(deep[1], 17), deep[2])
        lf = leaf.copy()
        lf[n - 1] = parent.size
        refused(parent, depth, lf)
        assert db._lib.yh_db_set_taxonomy(db._h, None, p(depth), parent.size, p(leaf)) == _lib.YH_ERR_INVALID_ARG
        with pytest.raises(ValueError, match="one node per reference"):
            db.set_taxonomy(parent, depth, leaf[:-1])
        # replacing the taxonomy changes the answers
        chain = cases.chain_tree(n)
        db.set_taxonomy(*chain)
        got = db.lca(sample)
        again = lca_oracle(values, offsets, chain[0], chain[2], sample)
        assert got[1].shape == (17, 2) and np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1])
        assert not np.array_equal(got[0], want[0])
        # n_nodes == 0 removes it
        db.set_taxonomy(None, None, None)
        assert db.taxonomy_info() == {"n_nodes": 0, "device_bytes": 0}
        with pytest.raises(YachtHipError) as ei:
            db.lca(sample)
        assert ei.value.code == _lib.YH_ERR_UNSUPPORTED
        # ghosts registered
        db.set_taxonomy(parent, depth, leaf)
        ghost_src = torch.zeros(4, dtype=torch.int32, device="cuda:0")
        db.set_ghosts(64, 4, ghost_src.data_ptr())
        d = torch.zeros(2 * parent.size + 64, dtype=torch.int64, device="cuda:0")
        for call in (lambda: db.lca(sample), lambda: db.lca_device(d.data_ptr(), 0, 3, 0, d.data_ptr())):
            with pytest.raises(YachtHipError) as ei:
                call()
            assert ei.value.code == _lib.YH_ERR_UNSUPPORTED
    for flags in (YH_DB_NO_DIRECTORY, YH_DB_NO_INDEX):
        with RefDB(values, offsets, flags=flags) as db:
            for call in (lambda: db.set_taxonomy(parent, depth, leaf), lambda: db.lca(sample)):
                with pytest.raises(YachtHipError) as ei:
                    call()
                assert ei.value.code == _lib.YH_ERR_UNSUPPORTED
    # an empty database: zero counts, nodes untouched
    with RefDB(np.zeros(0, np.uint64), np.zeros(3, np.uint64)) as db:
        db.set_taxonomy([0, 0], [0, 1], [1, 0])
        nodes, counts = db.lca(np.array([3, 5], np.uint64), [4, 4])
        assert nodes.tolist() == [NONE, NONE] and counts.tolist() == [[0, 0], [0, 0]]


def test_device_form_and_its_place_among_the_other_calls(hip_lib, big):
    """The device form equals the host form; run, abund, explain and gather give the same results before and after
    set_taxonomy plus lca on one handle; lca between pipelined steps leaves them alone."""
    import torch

    rng, refs, values, offsets, parent, depth, leaf, clustered = big
    dev = torch.device("cuda:0")
    n = len(refs)

    def up(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).to(dev)

    samples = [_big_sample(rng, refs, clustered, k) for k in (600_000, 40_000, 580_000)]
    abunds = [rng.integers(1, 1001, s.size).astype(np.uint32) for s in samples]
    member = (np.arange(n) % 3 == 0).astype(np.uint8)

    def others(db):
        s, a = samples[1], abunds[1]
        rows, more, owner = db.gather(s, member, a, want_owner=True)
        return [*db.run_counts(s), *db.abundance(s, a), *db.explain(s, member, a), rows, np.array([more]), owner]

    with RefDB(values, offsets) as db:
        before = others(db)
        db.set_taxonomy(parent, depth, leaf)
        want = [db.lca(s, a) for s, a in zip(samples, abunds)]  # (the host form: against the oracle above)
        assert np.array_equal(want[1][0], lca_oracle(values, offsets, parent, leaf, samples[1])[0])
        after = others(db)
        assert len(before) == len(after) and all(np.array_equal(b, a) for b, a in zip(before, after))
        d_s = [up(s, np.int64) for s in samples]
        d_a = [up(a, np.int32) for a in abunds]
        d_node = [torch.full((s.size,), 0x55, dtype=torch.int32, device=dev) for s in samples]
        d_cnt = [torch.full((2 * parent.size,), -1, dtype=torch.int64, device=dev) for _ in samples]
        torch.cuda.synchronize()

        def lca(k, nodes=True, abund=True):
            db.lca_device(d_s[k].data_ptr(), d_a[k].data_ptr() if abund else 0, samples[k].size, d_node[k].data_ptr() if nodes else 0,
                          d_cnt[k].data_ptr())

        def same(k, nodes=True):
            assert np.array_equal(d_cnt[k].cpu().numpy().view(np.uint64).reshape(-1, 2), want[k][1]), k
            if nodes:
                assert np.array_equal(d_node[k].cpu().numpy().view(np.uint32), want[k][0]), k

        lca(0)
        lca(1)
        lca(2, nodes=False)
        db.synchronize()
        same(0)
        same(1)
        same(2, nodes=False)
        assert bool((d_node[2] == 0x55).all())  # d_node = NULL leaves the array alone
        lca(1, abund=False)  # d_abund = NULL: every abundance is 1
        db.synchronize()
        got = d_cnt[1].cpu().numpy().view(np.uint64).reshape(-1, 2)
        assert np.array_equal(got[:, 0], want[1][1][:, 0]) and np.array_equal(got[:, 1], got[:, 0])
        # between pipelined steps: their results stay what run_counts gives, and the lca call is right too
        bigs = [0, 2, 0]
        counts = [[torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3)] for _ in bigs]
        d_node[2].fill_(0x55)
        for i, k in enumerate(bigs):
            db.run_device_pipelined(d_s[k].data_ptr(), samples[k].size, *(c.data_ptr() for c in counts[i]))
            if i == 1:
                lca(2)
        db.run_device_join()
        db.synchronize()
        for i, k in enumerate(bigs):
            for g, w in zip(counts[i], db.run_counts(samples[k])):
                assert np.array_equal(g.cpu().numpy().view(np.uint32), w), ("pipelined step", i)
        same(2)
