"""CPU: every case of tests/fused_cases.py reaches the state of the fused step's hit rows it is named for, by the module's
plain-int mirror alone; the mirror's hits per reference are tied to oracle.overlap on one sample per database.  No case is
skipped or filtered: one that misses its state fails here, before tests/test_gpu_fused_edges.py runs it on the device."""
import numpy as np
import pytest

import fused_cases as fc


def steps_of(db, samples):
    return {label: fc.Step(db, s) for label, s in samples.items()}


@pytest.fixture(scope="module")
def fill():
    db = fc.fill_database()
    return db, fc.fill_samples(db), steps_of(db, fc.fill_samples(db))


@pytest.fixture(scope="module")
def crowded():
    db = fc.crowded_database()
    return db, fc.crowded_samples(db), steps_of(db, fc.crowded_samples(db))


@pytest.fixture(scope="module", params=[131_072, 131_073])
def bins(request):
    db = fc.bins_database(request.param)
    smp = fc.bins_samples(db)
    return db, smp, steps_of(db, smp)


@pytest.fixture(scope="module")
def growth():
    return fc.fill_database(), fc.growth_samples(), steps_of(fc.fill_database(), fc.growth_samples())


def well_formed(samples):
    for label, s in samples.items():
        assert s.dtype == np.uint64 and s.size == int(label.split("@")[1]), label
        assert bool((s[1:] > s[:-1]).all()), f"{label} is not ascending and distinct"


def against_oracle(db, sample, step):
    from oracle import oracle

    values, offsets = db.packed()
    assert np.array_equal(step.hits, oracle.overlap(values, offsets, sample, threads=4))


# ---- the rules themselves ---------------------------------------------------------------------------------------------
def test_geometry_and_capacity_rules():
    assert [fc.geometry(n) for n in (1, 262_143, 262_144, 524_287, 524_288, 4_194_305)] == \
        [(256, 256), (256, 256), (1024, 1024), (1024, 1024), (1024, 2048), (1024, 2048)]
    assert [fc.n_tiles(n) for n in fc.GROWTH_SIZES] == [256, 512, 513, 2048, 2049]
    assert [fc.n_tiles(n) for n in (262_144, 262_145, 524_287, 30_000)] == [256, 257, 512, 118]
    assert [fc.capacity_for(t) for t in (1, 256, 512, 513, 768, 769, 1793, 2048)] == [512, 512, 512, 768, 768, 1024, 2048, 2048]
    assert fc.uses_rows(131_072, 524_288) and not fc.uses_rows(131_073, 524_288)
    assert fc.uses_rows(8200, 4_194_304) and not fc.uses_rows(8200, 4_194_305) and not fc.uses_rows(8200, 262_143)
    # 2654435761 >> 22, (2 x 2654435761 mod 2^32) >> 22, 2654435761 mod 1024
    assert [fc.home_slot(j) for j in (0, 1, 2, 1 << 22)] == [0, 632, 241, 433]
    assert fc.apart([0, 2]) and fc.apart([5]) and not fc.apart([j for j in range(20_000) if fc.home_slot(j) == 632][:2])
    wrap = [j for j in range(5000) if fc.home_slot(j) == 1023][0], [j for j in range(5000) if fc.home_slot(j) == 0][1]
    assert not fc.apart(wrap)       # (home + 1 of the table's last slot is its first)


def test_trace_line_round_trip():
    line = fc.HandleMirror(8200).step(1_048_577)
    assert fc.parse(line) == {"sample": 1_048_577, "lanes": 1024, "tiles": 513, "refs": 8200, "capacity": 768, "grew": 1,
                              "drained": 0, "path": "rows"}


# ---- bins32 / bins33 --------------------------------------------------------------------------------------------------
def test_bins_cover_every_bin_and_quarter(bins):
    db, smp, steps = bins
    well_formed(smp)
    assert fc.n_bins(db.n) == (32 if db.n == 131_072 else 33)
    corners, quarters = fc.bins_ids(db)
    assert {j // fc.HR_BIN for j in corners} >= {0, 1, 2, 3, 15, 16, 30, 31}
    for b in (3, 31):
        assert {(j % fc.HR_BIN) // 1024 for j in corners if j // fc.HR_BIN == b} == {0, 1, 2, 3}
    assert 131_071 in corners and 131_071 in quarters and db.n - 1 in corners and db.n - 1 in quarters
    assert {(j // fc.HR_BIN, (j % fc.HR_BIN) // 1024) for j in quarters if j < 131_072} == {(b, q) for b in range(32) for q in range(4)}
    assert len({j % 1024 for j in quarters}) > 100      # (the reducer's lanes differ from quarter to quarter)
    for size in (262_144, 524_288):
        st = steps[f"quarters@{size}"]
        # ONE tile hits a reference in each of the 32 bins -- one in each quarter -- with every reference in its home slot
        assert sorted(st.tile_refs) == [0] and st.exact[0] and sorted(st.tile_refs[0]) == quarters
        assert bool((st.claimed[0, :32] >= 4).all()) and not st.overflowing()
        assert bool((st.hits[quarters] == fc.PER_REF).all())
        st = steps[f"corners@{size}"]
        assert len(st.tile_refs) > 20 and max(st.tile_refs) > st.tiles * 0.9      # hits in many tiles, up to the last ones
        assert bool((st.hits[corners] == fc.PER_REF).all()) and not st.overflowing()
        hit_bins = {b for t, b in zip(*np.nonzero(st.claimed))}
        assert hit_bins >= {0, 1, 2, 3, 15, 16, 30, 31}
        assert st.rows == (db.n == 131_072)
    # a clustered reference is hit on shared hashes: two entries
    st = steps["corners@524288"]
    assert st.claimed[:, 0].sum() > sum(1 for ids in st.tile_refs.values() for j in ids if j < fc.HR_BIN)
    assert steps["corners@30000"].lanes == 256 and not steps["corners@30000"].rows
    assert set(fc.BINS_SEQ) == set(smp)
    # every 1024-lane step is followed by, and follows, a 256-lane one somewhere in the sequence
    lanes = [steps[label].lanes for label in fc.BINS_SEQ]
    assert (1024, 256) in zip(lanes, lanes[1:]) and (256, 1024) in zip(lanes, lanes[1:]) and (1024, 1024) in zip(lanes, lanes[1:])
    assert any(a == "quarters@524288" and steps[b].lanes == 256 for a, b in zip(fc.BINS_SEQ, fc.BINS_SEQ[1:]))
    assert any(a == "quarters@262144" and steps[b].lanes == 256 for a, b in zip(fc.BINS_SEQ, fc.BINS_SEQ[1:]))


def test_bins_limit_from_both_sides(bins):
    db, smp, steps = bins
    lines = [fc.parse(ln) for ln in fc.predict([("handle", db.n)] + [("step", smp[label].size) for label in fc.BINS_SEQ])]
    want = "rows" if db.n == 131_072 else "dense"
    assert [ln["path"] for ln in lines] == [want if smp[label].size >= 262_144 else "dense" for label in fc.BINS_SEQ]
    assert {ln["capacity"] for ln in lines} == ({512} if db.n == 131_072 else {0})
    assert [ln["grew"] for ln in lines] == [int(db.n == 131_072)] + [0] * (len(lines) - 1)


def test_bins_mirror_against_oracle(bins):
    db, smp, steps = bins
    against_oracle(db, smp["corners@524288"], steps["corners@524288"])
    against_oracle(db, smp["quarters@262144"], steps["quarters@262144"])


# ---- fill -------------------------------------------------------------------------------------------------------------
def test_fill_rows_hold_exactly_k(fill):
    db, smp, steps = fill
    well_formed(smp)
    assert db.n == 8200 and fc.n_bins(db.n) == 3
    assert fc.apart(db.singles) and len(db.singles) == 64 and all(j // fc.HR_BIN == 1 for j in db.singles)
    assert not set(db.singles) & set(db.clustered())
    want_sectors = {15: 1, 16: 2, 31: 2, 32: 3, 47: 3, 48: 4, 63: 4, 64: 4}
    for k in fc.FILL_KS:
        for size in (524_288,) + ((262_144,) if f"single{k}@262144" in smp else ()):
            st = steps[f"single{k}@{size}"]
            assert st.rows and st.exact[0] and st.exact[1] and sorted(st.tile_refs) == [0, 1]
            assert st.claimed[0].tolist() == [0, k, 0], (k, size)
            assert st.sectors_read(0, 1) == want_sectors[k]
            assert st.overflowing() == ([(0, 1)] if k == 64 else []), (k, size)
            # the second tile: a few ordinary hits in the other bins, none in bin 1
            assert st.claimed[1].tolist() == [5, 0, 3]
            assert bool((st.hits[db.singles[:k]] == fc.PER_REF).all()) and int(st.hits.sum()) == fc.PER_REF * (k + 8)
    for size in (524_288, 262_144):
        st = steps[f"pairs64@{size}"]
        assert st.exact[0] and st.exact[1] and len([j for j in st.tile_refs[0] if j // fc.HR_BIN == 1]) == 32
        assert st.claimed[0].tolist() == [4, 64, 0] and st.overflowing() == [(0, 1)]
        assert st.claimed[1].tolist() == [5, 0, 0]
    st = steps["pairs63@524288"]
    in_bin1 = [j for j in st.tile_refs[0] if j // fc.HR_BIN == 1]
    assert st.exact[0] and len(in_bin1) == 32 and len(set(in_bin1) & set(db.clustered())) == 31 and db.lone in in_bin1
    assert st.claimed[0].tolist() == [2, 63, 0] and not st.overflowing() and st.claimed[1].tolist() == [0, 0, 3]
    assert set(fc.FILL_SEQ) == set(smp)


def test_fill_sequence_neighbours_differ(fill):
    db, smp, steps = fill
    k = [int(steps[label].claimed[0, 1]) for label in fc.FILL_SEQ]
    assert all(x != y for (x, y) in zip(fc.FILL_SEQ, fc.FILL_SEQ[1:]))
    same_set = list(zip(k, k[2:]))      # (the step two calls earlier wrote the same counter set's rows)
    assert sum(a > b for a, b in same_set) >= 8 and sum(a < b for a, b in same_set) >= 8
    over = [bool(steps[label].overflowing()) for label in fc.FILL_SEQ]
    pairs = list(zip(over, over[2:]))
    assert (True, False) in pairs and (False, True) in pairs      # a stamped overflow word, then an unstamped step; and back
    assert steps[fc.FILL_SEQ[-1]].overflowing() and steps[fc.FILL_SEQ[20]].overflowing()      # at_rest follows an overflow
    for want in fc.FILL_KS:
        assert want in k


def test_fill_mirror_against_oracle(fill):
    db, smp, steps = fill
    against_oracle(db, smp["pairs63@524288"], steps["pairs63@524288"])
    against_oracle(db, smp["single64@262144"], steps["single64@262144"])


# ---- crowded ----------------------------------------------------------------------------------------------------------
def test_crowded_references_share_a_home_slot(crowded):
    db, smp, steps = crowded
    well_formed(smp)
    assert db.n == 8200
    homes = [fc.home_slot(j) for j in db.crowd]
    assert len(set(homes[:4])) == 1 and len(set(homes[4:])) == 1 and homes[4] == homes[0] + 2
    assert all(j // fc.HR_BIN == 1 for j in db.crowd) and db.crowd[4:6] in db.clusters and len(db.crowd) == 8
    for label in ("crowd3", "crowd8", "crowd_full"):
        st = steps[f"{label}@524288"]
        assert not st.exact[0] and st.exact[1] and st.rows
        by_home = np.bincount([fc.home_slot(j) for j in st.tile_refs[0]], minlength=fc.TSLOTS)
        assert by_home.max() >= 3
    # the lower bounds: crowd_full needs only the single hits of ONE displaced reference to overflow its row
    assert steps["crowd3@524288"].claimed[0].tolist() == [0, 3, 0]
    assert steps["crowd8@524288"].claimed[0].tolist() == [0, 10, 0]
    assert steps["crowd_full@524288"].claimed[0].tolist() == [0, 70, 0] and steps["crowd_full@262144"].claimed[0].tolist() == [0, 70, 0]
    assert steps["single16@524288"].exact[0] and steps["single16@524288"].claimed[0].tolist() == [0, 16, 0]
    assert set(fc.CROWDED_SEQ) == set(smp) and all(a != b for a, b in zip(fc.CROWDED_SEQ, fc.CROWDED_SEQ[1:]))


def test_crowded_mirror_against_oracle(crowded):
    db, smp, steps = crowded
    against_oracle(db, smp["crowd_full@524288"], steps["crowd_full@524288"])


# ---- growth and the tile cap ------------------------------------------------------------------------------------------
def test_growth_samples_and_capacities(growth):
    db, smp, steps = growth
    well_formed(smp)
    assert [steps[f"spread@{s}"].tiles for s in fc.GROWTH_SIZES] == [256, 512, 513, 2048, 2049]
    for s in fc.GROWTH_SIZES:
        st = steps[f"spread@{s}"]
        assert sorted(st.tile_refs) == list(range(st.tiles)), f"a tile of spread@{s} without a hit"
        assert st.rows == (s != 4_194_305)
        assert not st.overflowing()
    # the last tile of 1 048 577 and of 4 194 305 hashes is ONE hash, and it is a hit
    assert smp["spread@1048577"].size - 512 * 2048 == 1 and steps["spread@1048577"].claimed[512].sum() == 1
    assert steps["spread@4194305"].claimed[2048].sum() == 1
    lines = [fc.parse(ln) for ln in fc.predict([("handle", db.n)] + [("step", s) for s in fc.GROWTH_SEQ])]
    assert [ln["capacity"] for ln in lines] == [512, 512, 768, 768, 2048, 2048, 2048]
    assert [ln["grew"] for ln in lines] == [1, 0, 1, 0, 1, 0, 0] and [ln["drained"] for ln in lines] == [0, 0, 2, 0, 2, 0, 0]
    assert [lines[i]["capacity"] for i in (0, 1, 2, 4)] == [512, 512, 768, 2048]      # 256, 512, 513 and 2048 tiles
    assert all(ln["path"] == "rows" for ln in lines)
    # a handle whose first 1024-lane step follows two pending 256-lane steps: an allocation with steps pending and nothing to drain for
    lines = [fc.parse(ln) for ln in fc.predict([("handle", db.n)] + [("step", s) for s in (30_000, 30_000, 524_288, 1_048_577, 30_000)])]
    assert [(ln["path"], ln["capacity"], ln["grew"], ln["drained"]) for ln in lines] == \
        [("dense", 0, 0, 0), ("dense", 0, 0, 0), ("rows", 512, 1, 0), ("rows", 768, 1, 2), ("dense", 768, 0, 0)]


def test_tile_cap_alternation(growth):
    db, smp, steps = growth
    lines = [fc.parse(ln) for ln in fc.predict([("handle", db.n)] + [("step", s) for s in fc.TILECAP_SEQ])]
    assert [(ln["tiles"], ln["path"]) for ln in lines] == [(2048, "rows"), (2049, "dense"), (2048, "rows"), (2049, "dense"), (513, "rows")]
    assert all(ln["lanes"] == 1024 and ln["capacity"] == 2048 for ln in lines) and [ln["grew"] for ln in lines] == [1, 0, 0, 0, 0]


def test_growth_mirror_against_oracle(growth):
    db, smp, steps = growth
    against_oracle(db, smp["spread@1048577"], steps["spread@1048577"])
