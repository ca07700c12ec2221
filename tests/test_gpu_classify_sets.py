"""RefDB.classify_sets / classify_sets_device (yh_classify_sets, yh_classify_sets_device) on the GPU against a brute-force
oracle (tests/classify_oracle.py: the per-entry node of tests/lca_oracle.py, a set's fold by intersecting ancestor sets).
Exact equality of every row and of every node word; the node words also equal RefDB.lca of a set alone (every set of the
hand-written case; the laid-out sets and a draw of the small ones in the synthetic case, to keep the test quick).

Before the device is asked, the oracle's census must show every class of set a kernel can get wrong: empty, no hit, root hits
only, one informative hit, several agreeing, a fold above every hit node, the root with informative hits, a set that crosses a
tile border, one that spans three tiles or more.  T restates YH_CLASSIFY_TILE; a row is 64 entries."""
import lca_cases as cases
import numpy as np
import pytest
from classify_oracle import CLASSES, ROW_DTYPE, census, classify_oracle

from yacht_amd import _lib, synth
from yacht_amd.engine import CLASSIFY_ROW_DTYPE, RefDB, YH_DB_NO_DIRECTORY, YH_DB_NO_INDEX, YachtHipError

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
T = 1024
NARROW = 2 ** 22
RETENTIONS = (1, 0.9, 0.5, 0.25, 0.1)


def _csr(sets):
    off = np.zeros(len(sets) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in sets], dtype=np.uint64)
    mins = np.concatenate([np.asarray(s, dtype=np.uint64) for s in sets]) if sets else np.zeros(0, np.uint64)
    return mins.astype(np.uint64), off


def _same(got, want, what):
    assert got.dtype == CLASSIFY_ROW_DTYPE and got.shape == want.shape, what
    for f in ("node", "n_kept", "n_hit", "n_root"):
        bad = np.flatnonzero(got[f] != want[f])
        assert bad.size == 0, (what, f, bad[:10], got[bad[:10]], want[bad[:10]])


# ---- (a) the hand-written database, every set and its row spelled out -------------------------------------------------------------
# nodes of the hashes (lca_cases.HAND_NODES): 5 -, 10 6, 11 3, 12 0, 20 6, 21 1, 22 0, 23 3, 24 0, 25 1, 27 -, 30 8, 1000 -
HAND_SETS = [
    ([], (NONE, 0, 0, 0)),                       # empty, first
    ([5, 27], (NONE, 2, 0, 0)),                  # no hit
    ([12, 22, 24], (0, 3, 3, 3)),                # root hits only
    ([5, 10, 12], (6, 3, 2, 1)),                 # one informative hit beside an absent hash and a root hit
    ([10, 20], (6, 2, 2, 0)),                    # several, agreeing
    ([10, 11], (3, 2, 2, 0)),                    # a species and its genus: the genus
    ([10, 30], (0, 2, 2, 0)),                    # two kingdoms: the root, above every hit node, with informative hits
    ([], (NONE, 0, 0, 0)), ([], (NONE, 0, 0, 0)), ([], (NONE, 0, 0, 0)),  # three empty sets in a row
    ([1000], (NONE, 1, 0, 0)),                   # one entry above the database's largest hash
    ([5, 10, 11, 12, 20, 21, 22, 23, 24, 25, 27, 30, 1000], (0, 13, 10, 3)),
    ([21, 25], (1, 2, 2, 0)),                    # family A twice
    ([11, 12, 22, 23, 24], (3, 5, 5, 3)),        # three root hits do not lift the genus
    ([], (NONE, 0, 0, 0)),                       # empty, last
]


def test_hand_written_sets(hip_lib):
    v, o = cases.pack(cases.HAND_REFS)
    sets = [s for s, _ in HAND_SETS]
    mins, off = _csr(sets)
    want = np.array([r for _, r in HAND_SETS], dtype=ROW_DTYPE)
    rows, nodes = classify_oracle(v, o, cases.HAND_PARENT, cases.HAND_LEAF, mins, off)
    assert rows.tolist() == want.tolist()  # the oracle agrees with what is written down
    got = census(cases.HAND_PARENT, nodes, off, rows, T)
    print("census", got)
    assert all(got[c] >= 1 for c in CLASSES[:7]), got
    with RefDB(v, o) as db:
        db.set_taxonomy(cases.HAND_PARENT, cases.HAND_DEPTH, cases.HAND_LEAF)
        r, n = db.classify_sets(mins, off, want_nodes=True)
        _same(r, want, "hand")
        assert np.array_equal(n, nodes)
        for s, hashes in enumerate(sets):
            alone = db.lca(np.array(hashes, dtype=np.uint64))[0]
            assert np.array_equal(n[int(off[s]):int(off[s + 1])], alone), s
        assert db.classify_sets(mins, off).tobytes() == r.tobytes()  # (without nodes)
        # n_sets = 1 with total = 0; no set at all
        one = db.classify_sets(np.zeros(0, np.uint64), np.zeros(2, np.uint64))
        assert one.tolist() == [(NONE, 0, 0, 0)]
        assert db.classify_sets(np.zeros(0, np.uint64), np.zeros(1, np.uint64)).size == 0
        for k, (hashes, row) in enumerate(HAND_SETS):  # every set as a call of its own
            assert db.classify_sets(np.array(hashes, np.uint64), np.array([0, len(hashes)], np.uint64)).tolist() == [row], k


# ---- (b) the narrow-range synthetic database, sets laid out against the tile and the 64-entry row ---------------------------------
def _cluster_tree(order, n_independent, per_cluster=len(RETENTIONS)):
    order = np.asarray(order)
    clustered = order >= n_independent
    cluster_of = np.where(clustered, (order - n_independent) // per_cluster, -1)
    member_of = np.where(clustered, (order - n_independent) % per_cluster, 0)
    return cases.tree_from_paths(cases.cluster_paths(cluster_of, member_of))


@pytest.fixture(scope="module")
def big():
    """test_gpu_lca.py's narrow-range database (compact buckets and filter) under the cluster tree, the sets laid out, and the
    oracle's answer for them: computed once, shared, left unchanged."""
    rng = np.random.default_rng(601)
    refs = synth.independent_refs(rng, 300, 5000, 0.35, 500, 20000, scaled=NARROW) + \
        synth.clustered_refs(rng, 12, RETENTIONS, 5000, scaled=NARROW)
    order = rng.permutation(len(refs))
    refs = [refs[i] for i in order]
    values, offsets = synth.pack(refs)
    parent, depth, leaf = _cluster_tree(order, 300)
    clustered = np.flatnonzero(order >= 300)
    present = np.union1d(clustered, rng.choice(len(refs), size=20, replace=False))
    pool = synth.sample_from_refs(rng, refs, present, 0.3, 120_000, scaled=NARROW)  # hits of every class, and noise
    member = np.unique(np.concatenate([refs[j] for j in clustered]))  # hashes of cluster members: many of them shared

    def draw(n, src=pool):
        return np.sort(rng.choice(src, size=n, replace=False))

    sets, laid = [], []

    def put(s, mark=True):
        if mark:
            laid.append(len(sets))
        sets.append(np.asarray(s, dtype=np.uint64))

    def at():
        return sum(len(s) for s in sets)

    put(draw(T))                   # exactly one tile, aligned: ends at entry T - 1 ...
    put(draw(T + 1))               # ... and the next starts at T and straddles the border at 2 T
    put(draw(3 * T + 5))           # spans tiles: a chain of carries
    put([], False), put([], False), put([], False)
    put(draw(64 - at() % 64))      # up to the end of a row: the run ends at lane 63
    assert at() % 64 == 0
    put(draw(64))                  # a whole row: starts at lane 0, ends at lane 63
    for _ in range(64):            # 64 sets of one entry fill a row
        put(draw(1))
    put(draw(10)), put(draw(54))   # ends at lane 63 again
    put(draw(64 * 3))              # three whole rows
    put(draw(2 * T + 700, member))  # cluster hashes only, across three tiles
    same = draw(37)
    for _ in range(50):            # a block where every set is the same hash list
        put(same)
    sizes = rng.integers(0, 4, size=100_000)  # 10^5 sets of 0 to 3 entries
    small0 = len(sets)
    flat = rng.choice(pool, size=int(sizes.sum()))
    cut = np.concatenate([[0], np.cumsum(sizes)])
    for s in range(sizes.size):
        put(np.unique(flat[cut[s]:cut[s + 1]]), False)
    put([], False)
    tail = (1 - at()) % T          # the last tile holds a single entry
    put(draw(tail + T if tail < 2 else tail))
    put([], False)                 # an empty set last
    mins, off = _csr(sets)
    assert mins.size % T == 1
    rows, nodes = classify_oracle(values, offsets, parent, leaf, mins, off)
    return dict(values=values, offsets=offsets, parent=parent, depth=depth, leaf=leaf, sets=sets, laid=laid, small0=small0,
                mins=mins, off=off, rows=rows, nodes=nodes, rng=rng)


def test_census_of_the_laid_out_sets(big):
    got = census(big["parent"], big["nodes"], big["off"], big["rows"], T)
    print("census", got)
    assert all(got[c] >= 1 for c in CLASSES), got
    assert got["empty"] >= 1000 and got["no_hit"] >= 100 and got["one_informative"] >= 100 and got["root_only"] >= 10, got
    # a fold strictly above every hit node AND below the root
    rows, nodes, off = big["rows"], big["nodes"], big["off"].astype(np.int64)
    above = 0
    for s in np.flatnonzero((rows["node"] != 0) & (rows["node"] != NONE)):
        above += int(rows["node"][s]) not in set(nodes[off[s]:off[s + 1]].tolist())
    assert above >= 5, above


def test_laid_out_sets_against_the_oracle(hip_lib, big):
    with RefDB(big["values"], big["offsets"]) as db:
        assert db.info()["filter_bytes"] > 0 and db.info()["n_shared_distinct"] > 1000
        db.set_taxonomy(big["parent"], big["depth"], big["leaf"])
        rows, nodes = db.classify_sets(big["mins"], big["off"], want_nodes=True)
        assert np.array_equal(nodes, big["nodes"]), np.flatnonzero(nodes != big["nodes"])[:10]
        _same(rows, big["rows"], "laid out")
        again, nodes2 = db.classify_sets(big["mins"], big["off"], want_nodes=True)  # (e) two calls, the same bytes
        assert again.tobytes() == rows.tobytes() and nodes2.tobytes() == nodes.tobytes()
        assert db.classify_sets(big["mins"], big["off"]).tobytes() == rows.tobytes()  # d_node = NULL
        off = big["off"].astype(np.int64)
        some = big["laid"][:12] + big["laid"][-3:] + (big["small0"] + big["rng"].choice(100_000, size=25, replace=False)).tolist()
        for s in some:
            if off[s] == off[s + 1]:
                continue
            alone = db.lca(big["sets"][s])[0]
            assert np.array_equal(nodes[off[s]:off[s + 1]], alone), s
        # a prefix of the sets is a call of its own: tiles end elsewhere, rows stay
        for k in (1, 2, 3, 8, len(big["laid"]) + 20):
            part = db.classify_sets(big["mins"][:off[k]], big["off"][:k + 1])
            _same(part, big["rows"][:k], f"prefix {k}")


def test_device_form_leaves_no_stale_row(hip_lib, big):
    """(d) a second call with fewer sets into the same row buffer: every row of its range is its own, the rows behind are the
    first call's; the device form equals the host form."""
    import torch

    dev = torch.device("cuda:0")
    off = big["off"].astype(np.int64)
    n1 = len(big["sets"])
    n2 = big["small0"] + 5000
    sets2 = big["sets"][:n2][::-1]  # the same sets in another order: other rows at the same indices
    mins2, off2 = _csr(sets2)
    want2 = big["rows"][:n2][::-1]
    with RefDB(big["values"], big["offsets"]) as db:
        db.set_taxonomy(big["parent"], big["depth"], big["leaf"])
        d_m = torch.from_numpy(big["mins"].view(np.int64)).to(dev)
        d_o = torch.from_numpy(big["off"].view(np.int64)).to(dev)
        d_m2 = torch.from_numpy(mins2.view(np.int64)).to(dev)
        d_o2 = torch.from_numpy(off2.view(np.int64)).to(dev)
        d_rows = torch.full((4 * n1,), 0x55555555, dtype=torch.int32, device=dev)
        d_node = torch.full((big["mins"].size,), 0x55, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        db.classify_sets_device(d_m.data_ptr(), d_o.data_ptr(), n1, big["mins"].size, d_rows.data_ptr(), d_node.data_ptr())
        db.synchronize()
        first = d_rows.cpu().numpy().view(CLASSIFY_ROW_DTYPE)
        _same(first, big["rows"], "device form")
        assert np.array_equal(d_node.cpu().numpy().view(np.uint32), big["nodes"])
        db.classify_sets_device(d_m2.data_ptr(), d_o2.data_ptr(), n2, mins2.size, d_rows.data_ptr(), 0)
        db.synchronize()
        second = d_rows.cpu().numpy().view(CLASSIFY_ROW_DTYPE)
        _same(second[:n2], want2, "second call")
        assert second[n2:].tobytes() == first[n2:].tobytes()
        assert off[n2] > 0


# ---- (c) the calls refused ---------------------------------------------------------------------------------------------------------
def test_refused_calls(hip_lib):
    v, o = cases.pack(cases.HAND_REFS)
    mins, off = _csr([[10, 20], [5]])

    def refused(db, code, m=mins, f=off):
        with pytest.raises(YachtHipError) as e:
            db.classify_sets(m, f)
        assert e.value.code == code, e.value

    with RefDB(v, o) as db:
        refused(db, _lib.YH_ERR_UNSUPPORTED)  # no taxonomy
        assert db.classify_sets(np.zeros(0, np.uint64), np.zeros(1, np.uint64)).size == 0  # (no set: YH_OK even so)
        db.set_taxonomy(cases.HAND_PARENT, cases.HAND_DEPTH, cases.HAND_LEAF)
        assert db.classify_sets(mins, off).tolist() == [(6, 2, 2, 0), (NONE, 1, 0, 0)]
        refused(db, _lib.YH_ERR_UNSORTED, *_csr([[20, 10], [5]]))   # an unsorted set
        refused(db, _lib.YH_ERR_UNSORTED, *_csr([[10, 10]]))        # not strictly ascending
        refused(db, _lib.YH_ERR_INVALID_ARG, np.array([10, 20, 5], np.uint64), np.array([0, 3, 2, 3], np.uint64))  # descending offsets
        refused(db, _lib.YH_ERR_INVALID_ARG, np.array([10, 20, 5], np.uint64), np.array([1, 2, 3], np.uint64))     # not from 0
        with pytest.raises(ValueError):
            db.classify_sets(mins, np.array([0, 2, 4], np.uint64))  # off does not end at len(mins)
        assert db.classify_sets(*_csr([[5], [10, 20]])).tolist() == [(NONE, 1, 0, 0), (6, 2, 2, 0)]  # (no order ACROSS sets)
        db.set_taxonomy(None, None, None)
        refused(db, _lib.YH_ERR_UNSUPPORTED)
    for flags in (YH_DB_NO_DIRECTORY, YH_DB_NO_INDEX):
        with RefDB(v, o, flags=flags) as db:
            refused(db, _lib.YH_ERR_UNSUPPORTED)
    with RefDB(np.zeros(0, np.uint64), np.zeros(3, np.uint64)) as db:  # an empty database: every row {NONE, n_kept, 0, 0}
        db.set_taxonomy(np.zeros(1, np.uint32), np.zeros(1, np.uint8), np.zeros(2, np.uint32))
        rows, nodes = db.classify_sets(mins, off, want_nodes=True)
        assert rows.tolist() == [(NONE, 2, 0, 0), (NONE, 1, 0, 0)] and nodes.tolist() == [NONE] * 3
