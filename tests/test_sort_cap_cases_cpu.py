"""No GPU: every case of tests/sort_cap_cases.py is what it is named for.

With the numpy model of the sort's one linear function: the geometry each path takes is the one stated, the target bucket
and the target slot hold EXACTLY the named number of pairs, nothing that is not a named target comes near a capacity -- so the
set of buckets the side list must take is exactly the named one --, the sketches are valid, the sizes stay small, and the
side-list lengths, sketch-count residues, walk positions and run lengths at the ends of the side list that the GPU tests
(tests/test_gpu_sort_caps.py) rely on are there.  These are the conditions under which those tests cannot pass vacuously.
Run with -s for the table of cases.
"""
import numpy as np
import pytest

import order_cases as oc
import sort_cap_cases as sc


def _holders(c, h):
    """Sketches that hold hash h."""
    pos = np.flatnonzero(c.values == np.uint64(h))
    return (np.searchsorted(c.offsets, pos.astype(np.uint64), side="right") - 1).tolist()


# ---- the model ----------------------------------------------------------------------------------------------------------------
def test_fine_of_is_region_of_and_the_array_form_agrees():
    """fine_of is written as order_cases.region_of is (the same shift, multiplier and high word); fine_all is fine_of."""
    rng = np.random.default_rng(1)
    for mh in (sc.MAX_HASH, 7999, (1 << 64) - 1, (1 << 63) + 12345, 1 << 40):
        hs = np.concatenate([rng.integers(0, mh, size=400, dtype=np.uint64, endpoint=True), np.array([0, 1, mh - 1, mh], np.uint64)])
        for H in (2_000, 22_000, 96_000):
            p1, p2 = oc.two_level_geometry(H)
            NB = p1 * p2
            got = sc.fine_all(hs, NB, mh)
            for h, f in zip(hs.tolist(), got.tolist()):
                assert f == sc.fine_of(h, NB, mh)
                assert f < NB * oc.BKT_SLOTS                               # (no hash up to max_hash needs the clamp to NB - 1)
                assert min((f >> oc.BKT_SLOT_BITS) // p2, p1 - 1) == oc.region_of(h, H, mh)
            assert np.all(np.diff(sc.fine_all(np.sort(hs), NB, mh).astype(np.int64)) >= 0)


def test_bucket_ranges_tile_the_key_space():
    for NB in (9, 12, 42, 48):
        edges = [sc.bucket_range(b, NB, sc.MAX_HASH) for b in range(NB)]
        assert edges[0][0] == 0 and edges[-1][1] == sc.MAX_HASH + 1
        for b, (lo, hi) in enumerate(edges):
            assert lo < hi and (b == 0 or edges[b - 1][1] == lo)
            assert sc.bucket_of(lo, NB, sc.MAX_HASH) == b == sc.bucket_of(hi - 1, NB, sc.MAX_HASH)
            assert hi - lo >= oc.BKT_SLOTS


def test_cap1_is_out_of_reach_with_two_regions():
    """Why the region case has three regions: with P1 = 2 the capacity exceeds every H that gives P1 = 2."""
    for H in range(oc.BKT_FILL + 1, 40 * oc.BKT_FILL, 97):
        p1, _ = oc.two_level_geometry(H)
        if p1 == 2:
            assert sc.cap1_of(H, p1) > H
    assert sc.cap1_of(sc.REGION_H, 3) < sc.REGION_H - 1


# ---- every case ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.NAMES)
def test_case_is_what_it_is_named_for(name):
    c = sc.case(name)
    assert oc.csr_is_valid(c.values, c.offsets)
    assert c.H <= sc.MAX_H and c.n_refs <= sc.MAX_REFS and c.max_hash == sc.MAX_HASH
    assert int(c.values.max()) == c.max_hash                                # (no interior element above the largest last one)
    # the geometry taken: pieces where no switch forbids them, P1 and P2 as stated
    assert oc.psort_applicable(c.H, c.max_hash)
    assert oc.pieces_geometry(c.H, c.max_hash, c.n_refs) == c.stated["pieces"]
    assert oc.two_level_geometry(c.H) == c.stated["two_level"]
    assert c.stated["pieces"][0] * c.stated["pieces"][1] != c.stated["two_level"][0] * c.stated["two_level"][1]
    own = c.geometry
    cnt = sc.bucket_counts(c.values, c.offsets, own)
    top = sc.max_slot_counts(c.values, c.offsets, own)
    assert int(cnt.sum()) == c.H
    named = set()
    for t in c.targets:
        b = t["bucket"]
        named.add(b)
        assert int(cnt[b]) == t["count"], (name, b, int(cnt[b]))
        slots = sc.slot_counts(c.values, c.offsets, own, b)
        assert int(slots.sum()) == t["count"] and int(slots.max()) == int(top[b])
        if t["slot_count"] is not None:
            assert int(slots[t["slot"]]) == t["slot_count"] == int(slots.max())
            assert t["count"] < 3 * sc.BKT_CAP // 4                         # (a bucket well below its capacity)
        # hashes with 1, 2, 3, 4, 5 and 9 holders, the bucket's smallest and largest key among what it holds
        for k, h in t["extras"].items():
            assert t["lo"] <= h < t["hi"] and len(_holders(c, h)) == k
        inside = c.values[(c.values >= np.uint64(t["lo"])) & (c.values < np.uint64(t["hi"]))]
        assert int(inside.min()) == t["lo"] or (b == 0 and int(inside.min()) == int(c.values.min()))
        assert int(inside.max()) == t["hi"] - 1
    # nothing else near a capacity, on its own geometry ...
    for b in range(cnt.size):
        if b not in named and name != sc.REGION_CASE:   # (the region case crowds a third of the key space: its own test below)
            assert cnt[b] < sc.BKT_CAP and top[b] <= sc.SLOT_MAX, (name, b)
    if c.targets:
        for handle in sc.HANDLES:
            want = {t["bucket"] for t in c.targets if t["count"] > sc.BKT_CAP or (handle == "sort" and int(top[t["bucket"]]) > sc.SLOT_MAX)}
            buckets, pairs = sc.expected_spill(c.values, c.offsets, handle, own) if own == "pieces" else (want, 0)
            assert buckets == want
            if own == "pieces":
                assert pairs == sum(t["count"] for t in c.targets if t["bucket"] in want)
    # ... and on the other one: only a bucket that holds a hot hash may be over a capacity there
    for path in sc.PATHS:
        NB = c.stated[path][0] * c.stated[path][1]
        hot_buckets = {sc.bucket_of(h, NB, c.max_hash) for h, _ in c.hot}
        cnt_p, top_p = sc.bucket_counts(c.values, c.offsets, path), sc.max_slot_counts(c.values, c.offsets, path)
        for b in range(NB):
            if b not in hot_buckets and name != sc.REGION_CASE:
                assert cnt_p[b] < sc.BKT_CAP and top_p[b] <= sc.SLOT_MAX, (name, path, b)
    # holders: sketches of 3 to 6 hashes and two bare ones per hot hash; rows to compare one by one
    for h, js in c.hot:
        assert js == sorted(_holders(c, h)) and len(js) >= 800
        sizes = np.diff(c.offsets.astype(np.int64))[js]
        assert int((sizes == 1).sum()) == 2 and set(sizes.tolist()) <= {1, 3, 4, 5, 6, 513, 1025}
        assert js[0] in c.rows and js[-1] in c.rows
    for x in c.absent:
        assert not np.any(c.values == np.uint64(x))
    assert len(c.rows) >= 3 and all(0 <= r < c.n_refs for r in c.rows)
    s = c.sample()
    assert np.all(np.isin(np.array([h for h, _ in c.hot] + c.absent, np.uint64), s))


def test_the_named_decisions():
    """The table the issue asks for, read off the model: which handle spills or refuses what on which path."""
    e = lambda name, handle, path: sc.case(name).expected(handle, path)
    spilled = lambda name, handle: e(name, handle, "pieces")["n_spilled_buckets"]
    for stem in ("fill1", "fill5"):
        assert [spilled(f"{stem}_{n}", "train") for n in (4095, 4096, 4097)] == [0, 0, 1]
    assert [spilled(f"fill5_{n}", "sort") for n in (4095, 4096, 4097)] == [0, 0, 1]          # the count alone decides
    assert [spilled(f"fill1_{n}", "sort") for n in (4095, 4096, 4097)] == [1, 1, 1]          # the hot slot marks it
    for stem in ("slot_alone", "slot_mixed"):
        assert [spilled(f"{stem}_{n}", "sort") for n in (1023, 1024, 1025)] == [0, 0, 1]
        assert [spilled(f"{stem}_{n}", "train") for n in (1023, 1024, 1025)] == [0, 0, 0]     # the train handle: count alone
        assert e(f"{stem}_1025", "sort", "pieces")["n_spilled_pairs"] == 2600
    for name in ("bucket0", "bucket_last", "twin"):
        assert e(name, "train", "pieces")["n_spilled_buckets"] == 1 == e(name, "sort", "pieces")["n_spilled_buckets"]
    for name in ("word_edge_31_32", "adjacent_walk"):
        assert e(name, "train", "pieces")["n_spilled_buckets"] == 2 == e(name, "sort", "pieces")["n_spilled_buckets"]
    # two-level: taken at the capacity, REFUSED one above it, with the bit that names the capacity
    for handle in sc.HANDLES:
        assert e("tl_bucket_4096", handle, "two_level") == {"sort_path": 2, "verdict": "taken", "bit": 0, "n_spilled_buckets": 0, "n_spilled_pairs": 0}
        assert (e("tl_bucket_4097", handle, "two_level")["verdict"], e("tl_bucket_4097", handle, "two_level")["bit"]) == ("REFUSED", 2)
        assert e("tl_slot_1024", handle, "two_level")["verdict"] == "taken"
        assert (e(sc.REGION_CASE, handle, "two_level")["verdict"], e(sc.REGION_CASE, handle, "two_level")["bit"]) == ("REFUSED", 1)
        assert e(sc.REGION_CASE, handle, "two_level")["sort_path"] == sc.SORT_RADIX
    assert (e("tl_slot_1025", "sort", "two_level")["verdict"], e("tl_slot_1025", "sort", "two_level")["bit"]) == ("REFUSED", 4)
    assert e("tl_slot_1025", "train", "two_level")["verdict"] == "taken"                     # k_bucket_group ranks nothing
    # the neighbours of the "nothing left behind" test
    a, b = sc.NEIGHBOURS
    assert spilled(a, "train") == 1 == spilled(a, "sort") and spilled(b, "train") == 0 == spilled(b, "sort")


def test_where_the_spilled_buckets_sit():
    c = sc.case("bucket0")
    assert c.targets[0]["bucket"] == 0 and c.hot[0][0] == int(c.values.min())                # the database's smallest hash
    c = sc.case("bucket_last")
    NB = c.stated["pieces"][0] * c.stated["pieces"][1]
    assert c.targets[0]["bucket"] == NB - 1 and c.hot[0][0] == c.max_hash
    assert all(int(c.sketch(j)[-1]) == c.max_hash for j in c.hot[0][1])                      # ... held as last element
    c = sc.case("word_edge_31_32")
    assert [t["bucket"] for t in c.targets] == [31, 32] and c.stated["pieces"][0] * c.stated["pieces"][1] > 33
    c = sc.case("adjacent_walk")
    assert c.targets[1]["bucket"] == c.targets[0]["bucket"] + 1
    c = sc.case("twin")
    (h0, j0), (h1, j1) = c.hot
    assert h1 == h0 + 1 and sc.fine_of(h0, 12, c.max_hash) == sc.fine_of(h1, 12, c.max_hash) and len(set(j0) & set(j1)) == 10
    for name in ("word_edge_31_32", "adjacent_walk"):                                        # a sketch with pairs of two marked buckets
        c = sc.case(name)
        assert len(set(c.hot[0][1]) & set(c.hot[1][1])) >= 5


def test_what_the_side_list_kernels_walk():
    spilled = [n for n in sc.NAMES if sc.case(n).geometry == "pieces" and sc.case(n).expected("train", "pieces")["n_spilled_pairs"]]
    # side-list lengths: n mod 256 in {0, 1, 255} (the grids of k_spill_keys, k_spill_group, k_spill_place)
    res = {n: sc.case(n).expected("train", "pieces")["n_spilled_pairs"] % 256 for n in spilled}
    assert res["len_mod256_0"] == 0 and res["fill1_4097"] == 1 and res["len_mod256_255"] == 255
    assert {sc.case(n).expected("sort", "pieces")["n_spilled_pairs"] % 256 for n in spilled} >= {0, 1, 255}
    # four sketches per workgroup of k_spill_collect: every residue of n_refs, the database ending in holders of marked pairs
    assert {sc.case(n).n_refs % 4 for n in spilled if sc.case(n).nrefs_mod is not None} == {0, 1, 2, 3}
    for n in spilled:
        c = sc.case(n)
        assert c.nrefs_mod is None or c.n_refs % 4 == c.nrefs_mod
        t_ranges = [(t["lo"], t["hi"]) for t in c.targets]
        in_marked = lambda x: any(lo <= int(x) < hi for lo, hi in t_ranges)
        assert all(any(in_marked(x) for x in c.sketch(j)) for j in range(c.n_refs - 3, c.n_refs))
        sizes = np.diff(c.offsets.astype(np.int64))
        # a holder with an empty sketch directly before and after it; one-hash holders
        js = [j for j in range(1, c.n_refs - 1) if sizes[j - 1] == 0 and sizes[j + 1] == 0 and sizes[j] > 0 and any(in_marked(x) for x in c.sketch(j))]
        assert len(js) >= 3
        assert sum(1 for j in np.flatnonzero(sizes == 1) if in_marked(c.sketch(j)[0])) >= 2
        # runs at the two ends of the sorted side list: the smallest and the largest key of the marked buckets
        lo_t, hi_t = min(c.targets, key=lambda t: t["bucket"]), max(c.targets, key=lambda t: t["bucket"])
        inside_lo = c.values[(c.values >= np.uint64(lo_t["lo"])) & (c.values < np.uint64(lo_t["hi"]))]
        inside_hi = c.values[(c.values >= np.uint64(hi_t["lo"])) & (c.values < np.uint64(hi_t["hi"]))]
        res[n] = (int((inside_lo == inside_lo.min()).sum()), int((inside_hi == inside_hi.max()).sum()))
    firsts, lasts = {res[n][0] for n in spilled}, {res[n][1] for n in spilled}
    assert 1 in firsts and any(k >= 2 for k in firsts) and 1 in lasts and any(k >= 2 for k in lasts), res
    # sketches of 513 and 1 025 hashes with marked-bucket hashes at positions 0, 511, 512 and last
    c = sc.case("adjacent_walk")
    sizes = np.diff(c.offsets.astype(np.int64))
    (a_lo, a_hi), (b_lo, b_hi) = [(t["lo"], t["hi"]) for t in c.targets]
    for size in (513, 1025):
        found = False
        for j in np.flatnonzero(sizes == size):
            s = c.sketch(j)
            found |= all(a_lo <= int(s[p]) < a_hi for p in (0, 511)) and all(b_lo <= int(s[p]) < b_hi for p in (512, size - 1))
        assert found, size


def test_the_region_case_overflows_the_lower_region_only():
    c = sc.case(sc.REGION_CASE)
    p1, p2 = c.stated["two_level"]
    assert (p1, p2) == (3, 3) and abs(c.H - 20_000) <= 500
    reg = sc.region_counts(c.values, c.offsets)
    cap1 = sc.cap1_of(c.H, p1)
    assert cap1 == ((c.H // 3 + c.H // 3 // 32 + 2 * 4096 + 255) // 256) * 256
    assert reg.tolist() == [c.H - 1, 0, 1] and reg[0] > cap1 and all(r <= cap1 for r in reg[1:])
    ends = c.values[c.offsets[1:][c.offsets[1:] > c.offsets[:-1]].astype(np.int64) - 1]
    assert int((ends == np.uint64(c.max_hash)).sum()) == 1 and int((c.values == np.uint64(c.max_hash)).sum()) == 1


def test_table(capsys):
    with capsys.disabled():
        for name in sc.NAMES:
            c = sc.case(name)
            cells = [f"{p[:2]}/{h[:2]} path {e['sort_path']} {e['verdict']:7s} bit {e['bit']} side list {e['n_spilled_buckets']}/{e['n_spilled_pairs']}"
                     for p in sc.PATHS for h in sc.HANDLES for e in [c.expected(h, p)]]
            print(f"{name:17s} H {c.H:6d} N {c.n_refs:5d}  " + " | ".join(cells))
