"""No GPU: the cases of tests/lookup_cases.py still hold what they are named for -- asserted from the plain-int mirror of the
geometry decision and from numpy, so that a change to a generator cannot quietly turn the device tests of the directory
(tests/test_gpu_lookup_edges.py) into tests of ordinary buckets."""
import numpy as np
import pytest

import lookup_cases as lc

TWO32 = lc.TWO32


def _occ(db, **kw):
    g = db.geometry(**kw)
    return g, lc.occupancy(db.distinct, g)


def test_forms_and_geometry_are_the_stated_ones():
    want = {  # name: (form, bits, nb, mul, span)
        "compact_edge": ("compact", 44, 4096, 4096, TWO32),
        "wide_edge": ("wide", 44, 5119, 5119, None),
        "compact_odd": ("compact", 44, 5000, 5000, 3_518_437_209),
        "small_0": ("compact", 1, 1, 2, None),
        "small_01": ("compact", 1, 1, 1, None),
        "small_012": ("compact", 2, 2, 2, None),
        "small_5_bits32": ("compact", 32, 2, 2, None),
        "small_5_bits33": ("compact", 33, 2, 3, None),
        "small_dense": ("compact", 13, 3277, 3277, None),
        "small_run300": ("compact", 20, 720, 720, None),
        "overflow_504": ("compact", 44, 4096, 4096, TWO32),
        "overflow_505": ("compact", 44, 4096, 4096, TWO32),
        "wide_full": ("wide", 64, 2048, 2048, 1 << 53),
        "wide_four": ("wide", 64, 2048, 2048, 1 << 53),
        "crowd": ("compact", 44, None, None, None),
    }
    assert [d.name for d in lc.databases()] == list(want)
    for db in lc.databases():
        g = db.geometry()
        form, bits, nb, mul, span = want[db.name]
        assert (g.form, g.bits) == (form, bits) and db.form == form, db.name
        assert nb is None or (g.nb, g.mul) == (nb, mul), (db.name, g.nb, g.mul)
        assert span is None or g.span == span, (db.name, g.span)
        if g.form == "compact":
            assert g.bits <= 32 or g.span <= TWO32, db.name
            assert g.bucket(db.max_hash) == g.nb - 1, db.name        # the hashes up to max_hash reach the last bucket
        assert db.distinct[0] == 0 or db.name in ("crowd", "wide_four"), db.name
    # the tiny ones, spelled out
    assert lc.database("small_0").distinct == [0] and lc.database("small_01").distinct == [0, 1]
    assert lc.database("small_012").distinct == [0, 1, 2]
    assert lc.database("small_5_bits32").max_hash == TWO32 - 1 and lc.database("small_5_bits33").max_hash == TWO32
    assert lc.database("small_dense").distinct == list(range(8192))
    assert lc.database("compact_edge").max_hash == lc.database("compact_odd").max_hash == (1 << 44) - 1
    assert lc.database("wide_full").max_hash == lc.M64
    crowd = lc.database("crowd").geometry()
    assert crowd.nb == crowd.mul == (2 * crowd.n_distinct + 4) // 5 and crowd.n_distinct >= 10_238


def test_the_compact_wide_threshold_flips_between_10238_and_10237():
    edge, wide = lc.database("compact_edge"), lc.database("wide_edge")
    assert len(edge.distinct) == 10_238 and len(wide.distinct) == 10_237
    assert set(wide.distinct) < set(edge.distinct)
    ge, gw = edge.geometry(), wide.geometry()
    assert (ge.nb_c, ge.mul_c, ge.span_c) == (4096, 4096, TWO32) and ge.form == "compact"
    assert (gw.nb_c, gw.mul_c, gw.span_c) == (4095, 4095, 4_296_016_129) and gw.span_c > TWO32 and gw.form == "wide"
    assert all(ge.bucket(h) == h >> 32 for h in edge.distinct)
    # the forms the switches force
    assert edge.geometry(wide_buckets=True).form == "wide" and edge.geometry(wide_buckets=True).nb == 5119
    assert wide.geometry(no_buckets=True).form == "directory" and edge.geometry(no_buckets=True).form == "compact"
    assert np.array_equal(lc.samples("compact_edge")["base"], lc.samples("wide_edge")["base"])            # the same sample
    # (4095 compact buckets WOULD hold a present h together with its absent h + 2^32, which the sample asks)
    asked = set(int(x) for x in lc.samples("wide_edge")["base"])
    both = [h for h in wide.distinct if h + TWO32 in asked and (h * 4095) >> 44 == ((h + TWO32) * 4095) >> 44]
    assert len(both) >= 1 and not set(h + TWO32 for h in both) & set(wide.distinct)


@pytest.mark.parametrize("name", ["compact_edge", "wide_edge"])
def test_edge_occupancies_and_2_pow_32_probes(name):
    db = lc.database(name)
    chosen = db.meta["chosen"]
    ge = lc.Geometry((1 << 44) - 1, 10_238)           # the compact geometry the occupancies are stated in: bucket = h >> 32
    occ = lc.occupancy(db.distinct, ge)
    got = [len(occ.get(lc.EDGE_FIRST + i, [])) for i in range(len(lc.EDGE_OCC))]
    assert got == list(lc.EDGE_OCC) and sorted(got) == [0, 1, 6, 7, 8, 9, 15, 63, 64, 65, 66, 200]
    assert {7, 8, lc.RANK_STOP, lc.RANK_STOP + 1}.issubset(got) and max(got) > lc.RANK_STOP + 1
    lows = {h & 0xFFFFFFFF for run in chosen.values() for h in run}
    assert 0 in lows and 0xFFFFFFFF in lows
    for n in (7, 8):     # the first entry's low word is 0, the last one's 0xffffffff: the seventh entry, and the first of the overflow table
        run = occ[lc.EDGE_FIRST + lc.EDGE_OCC.index(n)]
        assert run[0] & 0xFFFFFFFF == 0 and run[-1] & 0xFFFFFFFF == 0xFFFFFFFF
    present, sample = set(db.distinct), set(int(x) for x in lc.samples(name)["base"])
    n_probes = 0
    for b, run in chosen.items():
        stored = {h & 0xFFFFFFFF for h in run}
        for h in run:
            for p in (h - TWO32, h + TWO32):
                assert p not in present and p in sample
                # the false hit guarded against: p sits in the bucket next to one that stores p's own low word
                assert abs(ge.bucket(p) - b) == 1 and (p & 0xFFFFFFFF) in stored
                assert (p & 0xFFFFFFFF) not in {x & 0xFFFFFFFF for x in occ.get(ge.bucket(p), [])}
                n_probes += 1
    assert n_probes == 2 * sum(lc.EDGE_OCC)
    if name == "wide_edge":      # five against six entries of a wide bucket, and buckets that hold h next to an absent h + 2^32
        g, wocc = _occ(db)
        sizes = {len(r) for r in wocc.values()}
        assert {lc.WIDE_ENTRIES, lc.WIDE_ENTRIES + 1}.issubset(sizes), sorted(sizes)
        assert g.dir_shift == 32 and g.dir_nb == 4096
    else:
        over = lc.overflow_entries(db.distinct, ge)
        assert len(over) >= sum(max(n - 7, 0) for n in lc.EDGE_OCC) and lc.ovf_capacity(len(over)) == 1024


def test_compact_odd_pairs_straddle_their_boundaries():
    db = lc.database("compact_odd")
    g = db.geometry()
    present, sample = set(db.distinct), set(int(x) for x in lc.samples("compact_odd")["base"])
    pairs = db.meta["pairs"]
    assert len(pairs) >= 200 and len(db.distinct) == 12_500
    kinds = {"both": 0, "below": 0, "above": 0}
    for k, e, kind in pairs:
        assert g.bucket(e - 1) == k - 1 and g.bucket(e) == k and g.first_of(k) == e
        assert e & (e - 1) != 0                                           # (no power of two)
        assert ((e - 1) in present, e in present) == {"both": (True, True), "below": (True, False), "above": (False, True)}[kind]
        assert e - 1 in sample and e in sample
        kinds[kind] += 1
    assert min(kinds.values()) >= len(pairs) // 3


def test_small_databases():
    db = lc.database("small_run300")
    g, occ = _occ(db)
    assert len(occ[db.meta["run_bucket"]]) == 300 and max(len(r) for r in occ.values()) == 300
    run = occ[db.meta["run_bucket"]]
    assert run == list(range(run[0], run[0] + 300))
    assert len(lc.overflow_entries(db.distinct, g)) >= 293
    g5 = lc.database("small_5_bits33").geometry()
    assert [g5.bucket(h) for h in lc.database("small_5_bits33").distinct] == [0, 0, 0, 1, 1]
    gd, od = _occ(lc.database("small_dense"))
    assert {len(r) for r in od.values()} == {2, 3}


def test_overflow_tables_504_and_505():
    for name, n_over, cap in (("overflow_504", 504, 1024), ("overflow_505", 505, 2048)):
        db = lc.database(name)
        g, occ = _occ(db)
        over = lc.overflow_entries(db.distinct, g)
        assert len(over) == n_over and lc.ovf_capacity(len(over)) == cap, name
        assert lc.ovf_capacity(n_over - 1) == 1024
        assert sorted(b for b, r in occ.items() if len(r) > 7) == list(lc.OVF_HEAVY)
        where = lc.ovf_place(over, cap)
        occupied = set(where.values())
        assert len(occupied) == n_over <= cap // 2                           # at most half full: every chain ends
        if cap == 1024:
            homes = [lc.ovf_slot(h) & 1023 for h in over]
            assert sum(1 for s in homes if s >= 1000) >= 40
            assert any(where[h] < (lc.ovf_slot(h) & 1023) for h in over)     # an entry placed past the table's end
            assert {1023, 0}.issubset(occupied)
        probes = db.meta["probes"]
        flagged = set(lc.OVF_HEAVY)
        assert len(probes) >= 40 and not set(probes) & set(db.distinct)
        sample = set(int(x) for x in lc.samples(name)["base"])
        wrapped = 0
        for p in probes:
            assert p in sample and g.bucket(p) in flagged
            assert (p & 0xFFFFFFFF) not in {h & 0xFFFFFFFF for h in occ[g.bucket(p)][:7]}     # not answered by the bucket itself
            home = lc.ovf_slot(p) & (cap - 1)
            steps = lc.ovf_probe_steps(p, occupied, cap)
            assert home in occupied and 1 <= steps < cap
            wrapped += home + steps >= cap
        assert wrapped >= (5 if cap == 1024 else 0)


def test_wide_full_occupancies_and_pairs():
    db = lc.database("wide_full")
    g, occ = _occ(db)
    got = [len(occ.get(lc.FULL_FIRST + i, [])) for i in range(len(lc.FULL_OCC))]
    assert got == [0, 1, 4, 5, 6, 7, 30] and all(g.bucket(h) == h >> 53 for h in db.distinct)
    assert 0 in db.distinct and lc.M64 in db.distinct and len(db.distinct) == 4096
    assert g.dir_shift == 54 and g.dir_nb == 1024
    present, sample = set(db.distinct), set(int(x) for x in lc.samples("wide_full")["base"])
    assert len(db.meta["both"]) >= 10 and len(db.meta["one"]) >= 10
    for h in db.meta["both"]:
        assert h in present and h + TWO32 in present and g.bucket(h) == g.bucket(h + TWO32)
    for h in db.meta["one"]:
        for p in (h - TWO32, h + TWO32):
            assert p not in present and p in sample and g.bucket(p) == g.bucket(h)
    sizes = {len(occ[g.bucket(h)]) for h in db.meta["both"] + db.meta["one"]}
    assert {5, 6}.issubset(sizes)


def test_wide_four_asks_an_absent_zero_in_a_bucket_of_four():
    """The fifth entry of a wide bucket that holds four hashes is all zero bits: hash 0, absent, is asked in such a bucket."""
    db = lc.database("wide_four")
    g, occ = _occ(db)
    assert g.form == "wide" and len(db.distinct) == 4096 and 0 not in db.distinct and lc.M64 in db.distinct
    assert len(occ[0]) == lc.WIDE_ENTRIES - 1 and g.bucket(0) == 0
    assert lc.samples("wide_four")["base"][0] == 0
    got = [len(occ.get(lc.FULL_FIRST + i, [])) for i in range(len(lc.FULL_OCC))]
    assert got == [0, 1, 4, 5, 6, 7, 30]


def test_crowd_groups_share_a_slot_inside_one_tile():
    db = lc.database("crowd")
    assert db.n_refs >= 6000 and all(1 <= r.size for r in db.refs)
    held = db.holders()
    private = [sum(1 for h in r if held[int(h)] == 1) for r in db.refs]
    assert min(private) >= 1 and max(private) <= 3
    groups = db.meta["groups"]
    assert sum(1 for t, *_ in groups if t == 10) >= 20 and sum(1 for t, *_ in groups if t == 8) >= 20
    seen = set()
    forms = {k: s for k, s in lc.samples("crowd").items() if k == "base" or k.startswith("padded")}
    for tbits, ids, base, shared in groups:
        assert len(ids) >= 3 and not seen & set(ids)
        seen |= set(ids)
        assert len({lc.hit_slot(r, 8) for r in ids}) == 1
        assert (len({lc.hit_slot(r, 10) for r in ids}) == 1) == (tbits == 10)
        if tbits == 8:
            assert len({lc.hit_slot(r, 10) for r in ids}) == len(ids)
        assert held[shared] == len(ids) and all(np.isin(shared, db.refs[r]) for r in ids)
        mine = [base + 4 * i for i in range(len(ids) + 1)]
        assert shared in mine and all(held[h] == 1 for h in mine if h != shared)
        for label, s in forms.items():
            pos = np.searchsorted(s, np.array(mine, dtype=np.uint64))
            assert np.array_equal(s[pos], np.array(mine, dtype=np.uint64))
            assert pos[-1] - pos[0] == 3 * len(ids), label                  # next to each other: only their own h - 1 / h + 1 between
            assert pos[0] // lc.TILE == pos[-1] // lc.TILE, (label, base)    # one 256-hash tile (and so one tile of every geometry)
    lengths = sorted(set(held.values()))
    assert set(lc.CROWD_HOLDERS).issubset(lengths) and 1 in lengths, lengths
    assert all(held[h] == k for h, k in db.meta["lists"].items())


def test_samples_are_ascending_and_of_the_stated_sizes():
    for db in lc.databases():
        forms = lc.samples(db.name)
        base = forms["base"]
        present = np.array(db.distinct, dtype=np.uint64)
        assert np.isin(present, base).all(), db.name                        # every database hash is asked
        for v in (0, db.max_hash, min(db.max_hash + 1, lc.M64), lc.M64):
            assert np.uint64(v) in base
        for label, s in forms.items():
            assert s.dtype == np.uint64 and s.size and (s[1:] > s[:-1]).all(), (db.name, label)
            kind, _, n = label.partition("_")
            if kind == "prefix":
                assert s.size == int(n) < base.size and np.array_equal(s, base[: s.size])
            if kind == "padded":
                assert s.size == int(n) and int(n) * 8 < 4.2e6 and np.isin(base, s).all()
                pad = s[~np.isin(s, base)]
                assert pad.size == s.size - base.size and not np.isin(pad, present).any() and (pad >= np.uint64(db.pad_lo)).all()
        assert {f"padded_{n}" for n in lc.PADDED}.issubset(forms)
        assert base.size <= lc.PREFIXES[0] or {f"prefix_{n}" for n in lc.PREFIXES if n < base.size}.issubset(forms)
        if base.size > 10_000:
            assert len(forms) == 1 + len(lc.PREFIXES) + len(lc.PADDED) and base.size >= 20_000 or db.name == "small_dense"
    # h - 1, h + 1, h - 2^32, h + 2^32 of every hash, where that is a 64-bit value and absent
    for name in ("compact_odd", "wide_full", "small_5_bits33"):
        db = lc.database(name)
        present, base = set(db.distinct), set(int(x) for x in lc.samples(name)["base"])
        for h in db.distinct[:: max(len(db.distinct) // 500, 1)]:
            for p in (h - 1, h + 1, h - TWO32, h + TWO32):
                assert not 0 <= p <= lc.M64 or p in base


def test_every_class_of_sample_hash_has_members():
    for db in lc.databases():
        got = lc.classes(db, lc.samples(db.name)["base"])
        if db.name in lc.SMALL_WITHOUT_CLASSES:      # too small (or, small_dense, too dense) to have twenty of every class
            assert got["present_single"] + got["present_shared"] == len(db.distinct) and got["absent_above_max"] >= 1, (db.name, got)
            continue
        if db.name in lc.NOTHING_ABOVE_MAX:
            assert got.pop("absent_above_max") == 0
        assert min(got.values()) >= 20, (db.name, got)
        # the padded forms add absent hashes of both kinds where the range has room for them
        if db.max_hash - db.pad_lo > 1 << 40:
            forms = lc.samples(db.name)
            pad = forms["padded_262143"][~np.isin(forms["padded_262143"], forms["base"])]
            inside = int((pad <= np.uint64(db.max_hash)).sum())
            assert inside > 50_000 and (pad.size - inside > 50_000 or db.max_hash == lc.M64), db.name
