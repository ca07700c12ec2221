"""No GPU: every case of tests/stream_cases.py reaches the state it is named for according to the mirror of the stream layout
and of the launch geometry, and the oracle's counts for every (database, sample) agree with a set-based count from the case's
own hash -> holders table.

The states are those of k_stream_lookup (yh_query.hip): which byte, lane, block, group, super-block and workgroup a run of
equal keys starts on and continues into, per environment of tests/test_gpu_stream_edges.py; rounds with more than STREAM_WQ
candidates; more holders than the hit table takes; the padding behind the last pair; fillers and the headers they write; the
tiles a workgroup makes of its sample range and the blocks each covers; the staged 32-bit offset next to its sentinel; the
sample ranges of wave_bound.  A constant that changes in the kernel and not here makes the GPU file's layout check fail; one
that changes here makes a case below miss its state and fail.
"""
import numpy as np
import pytest

import stream_cases as sc
from oracle import oracle

B = sc.STREAM_BLOCK


def _ids(cases):
    return [c.name for c in cases]


# ---- the mirror against the pairs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.all_cases(), ids=_ids(sc.all_cases()))
def test_layout_holds_every_pair_once_in_key_order(case):
    lay = case.layout()
    assert lay.H == case.hashes.size and lay.max_hash == int(case.hashes.max())
    assert lay.sshift == 32 or (lay.max_hash >> (lay.sshift + 1)) // lay.H < 32
    assert lay.sshift == 0 or (lay.max_hash >> lay.sshift) // lay.H >= 32
    assert lay.L == lay.H + lay.n_fillers and lay.slen % B == 0 and 0 <= lay.slen - lay.L < B
    assert lay.stream_bytes == lay.slen + 8 * (lay.nblk + 1)
    assert np.all(np.diff(lay.pos) >= 1)
    values, offsets = case.csr()
    assert int(offsets[-1]) == lay.H
    for j in range(min(case.n_refs, 100)):
        s = values[int(offsets[j]):int(offsets[j + 1])]
        assert np.all(s[1:] > s[:-1])
    # every delta fits its byte; a filler's is 255; the padding's is 0 (positions around every pair of a small database)
    if lay.slen <= 4 * B:
        keys = [lay.key_at(p) for p in range(lay.slen)]
        assert all(0 <= b - a <= 255 for a, b in zip(keys, keys[1:]))
        for p in range(lay.slen):
            kind = lay.kind_at(p)
            assert kind != "filler" or lay.delta_at(p) == 255
            assert kind != "pad" or (lay.delta_at(p) == 0 and keys[p] == lay.max_key)
        assert [k for k, p in zip(keys, range(lay.slen)) if lay.kind_at(p) == "real"] == [int(x) for x in lay.t]


def test_ladders_have_no_fillers_so_positions_are_indices():
    want = {"ladder272": 0, "ladder255": 0, "ladder256": 0, "ladder257": 0, "end0": 0, "end1": 0, "end1023": 0, "above": 0,
            "tiles": 20, "trunc1": 1, "trunc20": 20, "trunc32": 32}
    for case in sc.all_cases():
        if case.name in want:
            lay = case.layout()
            assert lay.sshift == want[case.name] and lay.n_fillers == 0, case.name
            assert np.array_equal(lay.pos, np.arange(lay.H))
    assert [c.layout().nblk for c in [sc.case_ladder272()] + sc.cases_ranges()] == [272, 255, 256, 257]
    assert [c.layout().n_padding for c in sc.cases_end()] == [0, 1023, 1]


# ---- runs of equal keys -------------------------------------------------------------------------------------------------------
def test_run_lengths_and_samples():
    c = sc.case_ladder272()
    assert sorted({m for _, m in sc.RUNS_272}) == [2, 16, 17, 30, 64, 65, 200, 1024, 1025, 2100]
    table = c.table()
    for start, m in sc.RUNS_272:
        h = c.hash_at(start)
        assert sorted(table[h]) == list(range(m))
        assert [c.hash_at(p) for p in (start, start + m - 1)] == [h, h] and c.hash_at(start - 1) == h - 1
        assert c.samples[f"run{start}x{m}:alone"].tolist() == [h]
        assert c.samples[f"run{start}x{m}:nbrs"].tolist() == [h - 1, h, h + 1]
        assert len(table[h - 1]) == 1 and (start + m == c.layout().L or len(table[h + 1]) == 1)


# (environment, run start) -> states the run must reach there
RUN_STATES = {
    ("wgs1", 5 * B + 127): {"starts_last_byte_of_lane", "next_lane", "blocks_1"},
    ("wgs1", B - 1): {"starts_last_byte_of_block", "next_block"},
    ("wgs1", 4 * B - 1): {"starts_last_of_group", "next_group"},
    ("wgs1", 16 * B - 1): {"starts_last_of_superblock", "next_superblock", "next_lane"},
    ("wgs1", 21 * B): {"starts_block", "queue_full", "blocks_1"},
    ("wgs1", 32 * B): {"starts_superblock", "queue_full", "table_crowded", "blocks_1"},
    ("wgs1", 64 * B): {"starts_superblock", "next_block", "blocks_2"},
    ("wgs1", 100 * B + 500): {"blocks_3", "next_block", "queue_full", "table_crowded"},
    ("wgs1", 150 * B - 1): {"starts_last_byte_of_block", "next_block"},
    ("wgs2", 4 * B - 1): {"starts_last_of_group", "starts_last_of_superblock", "next_superblock"},
    ("wgs2", 136 * B - 1): {"starts_last_of_workgroup", "next_workgroup", "queue_full"},
    ("wgs8", 100 * B + 500): {"next_workgroup", "next_block", "blocks_3"},
    ("wgs9", 64 * B): {"next_superblock"},
    ("wgs17", 16 * B - 1): {"starts_last_of_workgroup", "next_workgroup"},
    ("wgs19", 150 * B - 1): {"starts_last_of_workgroup", "next_workgroup"},
    ("wgs34", 136 * B - 1): {"starts_last_of_workgroup", "next_workgroup"},
    ("wgs39", 100 * B + 500): {"next_superblock", "blocks_3"},
    ("default", 4 * B - 1): {"starts_last_of_workgroup", "next_workgroup"},
    ("default", 100 * B + 500): {"next_superblock", "next_workgroup", "table_crowded"},
    ("default", 64 * B): {"starts_superblock", "next_superblock"},
}


def test_runs_reach_their_boundaries():
    c = sc.case_ladder272()
    runs = dict(sc.RUNS_272)
    for (env, start), want in RUN_STATES.items():
        got = sc.run_states(c.geometry(sc.wgs_of(env)), start, runs[start])
        assert want <= got, (env, start, sorted(want - got))
    # the run up to the last element of the stream, and the one in front of a last super-block of a single block
    lay = c.layout()
    start, m = sc.RUNS_272[-1]
    assert start + m == lay.L == lay.slen
    c257 = sc.cases_ranges()[2]
    g = c257.geometry(1)
    start, m = sc.RUN_257
    assert {"starts_last_of_superblock", "next_superblock"} <= sc.run_states(g, start, m)
    assert g.where(start + 1)["nvalid"] == 1 and g.where(start + 1)["super"] == 16 and g.where(start + 1)["wave"] == 0


def test_table_mirror():
    assert sc.table_must_overflow(range(2100)) and sc.table_must_overflow(range(1024))
    assert not sc.table_must_overflow(range(2))
    assert all(0 <= sc.table_home(r) < sc.TSLOTS for r in range(3000))


# ---- block ranges per workgroup -----------------------------------------------------------------------------------------------
def test_block_ranges_reach_the_table():
    by_name = {c.name: c for c in sc.all_cases()}
    assert sorted(per for per, _ in sc.RANGES.values()) == [2, 3, 7, 8, 15, 16, 31, 32, 34, 136, 255, 256, 257, 272]
    for (name, env), (per, nb) in sc.RANGES.items():
        c = by_name[name]
        assert env in c.envs
        g = c.geometry(sc.wgs_of(env))
        assert (g.per, g.nb(0)) == (per, nb), (name, env, g.per, g.nb(0))
        assert g.wg_key[0] == c.layout().hdr(0) and g.wg_key[-1] == c.layout().max_key
        assert all(a <= b for a, b in zip(g.wg_key, g.wg_key[1:]))
    g = by_name["ladder272"].geometry()
    assert g.wgs == 136 and sc.supers_per_wave(2) == [1, 1, 0, 0, 0, 0, 0, 0]            # waves with 0 and 1 super-blocks
    assert sc.supers_per_wave(257) == [3, 2, 2, 2, 2, 2, 2, 2] == sc.supers_per_wave(272)    # ... and 3; the preloaded first group
    assert sc.supers_per_wave(256) == [2] * 8 and sc.nb_for(255) == 4
    g = by_name["ladder272"].geometry(8)          # 34 = 8 x 4 + 2: a last group of two valid blocks
    assert g.where(33 * B)["nvalid"] == 2 and g.where(33 * B)["nb"] == 4
    g = by_name["ladder272"].geometry(39)         # a shorter last range
    assert g.blocks(38) == (266, 272) and g.n_ranges() == 39
    g = by_name["ladder257"].geometry()           # the default geometry, an odd number of blocks: empty workgroups behind
    assert (g.wgs, g.per, g.n_ranges()) == (128, 3, 86) and g.blocks(85) == (255, 257)
    # the bounds sample holds the last, first and second element of every block
    for name in ("ladder272", "ladder255", "ladder256", "ladder257"):
        c = by_name[name]
        s = set(c.samples["bounds"].tolist())
        assert all(c.hash_at(p) in s for b in range(1, c.layout().nblk) for p in (b * B - 1, b * B, b * B + 1))


# ---- the end of the stream ----------------------------------------------------------------------------------------------------
def test_end_of_stream_cases():
    for c, rem in zip(sc.cases_end(), (0, 1, B - 1)):
        lay = c.layout()
        assert lay.L % B == rem and lay.nblk == 3
        assert c.samples["largest"].tolist() == [lay.max_hash] and lay.kind_at(lay.L - 1) == "real"
        if rem == 1:
            assert [lay.kind_at(p) for p in (2 * B, 2 * B + 1, 3 * B - 1)] == ["real", "pad", "pad"]
            assert lay.key_at(3 * B - 1) == lay.max_key and lay.hdr(2) == lay.max_key
    for c in sc.cases_trunc():
        lay = c.layout()
        mx = lay.max_hash
        assert lay.n_padding == 1023 and c.samples["largest"].tolist() == [mx]
        other = int(c.samples["largest_other_low"][0])
        assert other != mx and other >> lay.sshift == lay.max_key and other not in c.table()
    assert sc.cases_trunc()[2].layout().max_hash & 0xffffffff == 0xffffffff       # the low word of a record nobody wrote


# ---- truncated keys -----------------------------------------------------------------------------------------------------------
def test_truncated_key_cases():
    assert [c.layout().sshift for c in sc.cases_trunc()] == list(sc.TRUNC_SHIFTS)
    for c in sc.cases_trunc():
        lay = c.layout()
        s = lay.sshift
        group, p0, k = c.notes["group"], c.notes["p0"], c.notes["k"]
        assert k == min(4, 1 << s) and p0 < B <= p0 + k - 1                      # the key straddles blocks 0 | 1
        assert len({h >> s for h in group}) == 1 and len({h & 0xffffffff for h in group}) == k
        assert [c.hash_at(p0 + j) for j in range(k)] == list(group)
        assert len({c.table()[h][0] for h in group}) == k and lay.hdr(1) == group[0] >> s
        assert c.samples["last_of_group"].tolist() == [group[-1]]
        table = c.table()
        strangers = [h for h in c.samples["other_low"].tolist() if h not in table]
        assert len(strangers) == 2 and all(any(x >> s == h >> s for x in (h - 1, h - (1 << s) + 1) if x in table) for h in strangers)
        # the tile cut: slots 6077 | 6078 of the one workgroup hold two hashes of one key, both in the database
        smp = c.samples["tile_cut"]
        g = c.geometry(1)
        assert g.wgs == 1 == c.geometry().wgs
        tiles = g.tiles(0, smp)
        assert [(t.sub, t.n) for t in tiles] == [(0, sc.ST_CAP), (sc.ST_CAP, smp.size - sc.ST_CAP)]
        a, b = int(smp[sc.ST_CAP - 1]), int(smp[sc.ST_CAP])
        assert (a, b) == (group[0], group[1]) and a >> s == b >> s
        assert tiles[1].klo == lay.hdr(1) and tiles[1].bl0 == 0       # hdr[mid + 1] < Klo is false at block 0: it is read again
        assert lay.key_at(B - 1) == tiles[1].klo
        # ... and the pair the second tile's first hash is looked up for lies in block 0, behind a header of the same key
        smp = c.samples["tile_from_header_key"]
        tiles = g.tiles(0, smp)
        assert [(t.sub, t.n) for t in tiles] == [(0, sc.ST_CAP), (sc.ST_CAP, smp.size - sc.ST_CAP)] and int(smp[sc.ST_CAP]) == group[0]
        assert tiles[1].klo == lay.hdr(1) == group[0] >> s and tiles[1].bl0 == 0 and c.hash_at(p0) == group[0] and p0 < B
        if k == 4:
            assert c.hash_at(p0 + 1) == group[1] and p0 + 1 < B      # (the same holds for the cut between equal keys)


# ---- fillers ------------------------------------------------------------------------------------------------------------------
def test_filler_case():
    c = sc.case_fillers()
    lay = c.layout()
    assert lay.sshift == 0
    gaps = {int(lay.t[i + 1] - lay.t[i]): int(lay.nfill[i + 1]) for i in range(lay.H - 1) if lay.t[i + 1] - lay.t[i] > 1}
    assert gaps == {255: 0, 256: 1, 510: 1, 511: 2}
    assert lay.filler_positions() == [B, B + 3, B + 5, B + 6, 2 * B - 1, 2 * B]
    assert lay.kind_at(B) == "filler" and lay.hdr(1) == lay.key_at(B - 1) + 255               # first filler of its gap
    assert lay.kind_at(2 * B) == "filler" and lay.hdr(2) == lay.key_at(2 * B - 2) + 510       # second filler of its gap
    table = c.table()
    assert all(k not in table for k in c.notes["filler_keys"]) and all(h in table for h in c.notes["behind"])
    assert all(h not in table for h in c.samples["between"].tolist())
    assert len(c.notes["behind"]) == 4 and c.hash_at(B + 1) in c.notes["behind"] and c.hash_at(2 * B + 1) in c.notes["behind"]


# ---- tiles --------------------------------------------------------------------------------------------------------------------
def test_tile_cases():
    c = sc.case_tiles()
    lay = c.layout()
    g = c.geometry(1)
    assert g.wgs == 1 and lay.nblk == 3

    def tiles(label):
        t = g.tiles(0, c.samples[label])
        assert all(x.bl0 < x.bl1 for x in t)      # (a tile always covers a block: its keys lie between wg_key[w] and wg_key[w + 1])
        return t

    for n, shape in ((sc.ST_CAP, [sc.ST_CAP]), (sc.ST_CAP + 1, [sc.ST_CAP, 1]), (2 * sc.ST_CAP + 1, [sc.ST_CAP, sc.ST_CAP, 1])):
        smp = c.samples[f"n{n}"]
        assert smp.size == n and int(smp[-1]) <= lay.max_hash and int(smp[0]) == 0
        t = tiles(f"n{n}")
        assert [x.n for x in t] == shape and t[0].single == (len(shape) == 1)
        assert sum(1 for h in smp.tolist() if h in c.table()) >= 1000
    start, m = sc.TILE_RUN
    run_h = c.hash_at(start)
    smp = c.samples["run_last_slot"]
    t = tiles("run_last_slot")
    assert int(smp[sc.ST_CAP - 1]) == run_h and t[0].n == sc.ST_CAP and t[0].khi == run_h >> lay.sshift and len(c.table()[run_h]) == m
    assert len(t) == 2 and t[1].klo > t[0].khi
    t = tiles("one_block_tile")
    assert len(t) == 2 and (t[1].bl0, t[1].bl1) == (2, 3) and (t[0].bl0, t[0].bl1) == (0, 2)
    t = tiles("gap_tile")          # keys between the last key of block 0 and the header of block 1: block 0 is read, nothing found
    assert len(t) == 2 and (t[1].bl0, t[1].bl1) == (0, 1)
    assert lay.key_at(B - 1) < t[1].klo <= t[1].khi < lay.hdr(1)
    assert not any(h in c.table() for h in c.samples["gap_tile"][sc.ST_CAP:].tolist())


# ---- the 32-bit offset and its sentinel ---------------------------------------------------------------------------------------
def test_wide_case_stages_the_largest_offset_and_cuts_at_the_sentinel():
    c = sc.case_wide()
    lay = c.layout()
    assert (lay.sshift, lay.nblk, lay.H) == (32, 16449, 4)
    assert lay.t.tolist() == [0, 0, 0xfffffffe, 0xffffffff]
    g = c.geometry(1)
    t = g.tiles(0, c.samples["all4"])
    assert [(x.sub, x.n) for x in t] == [(0, 3), (3, 1)]
    assert t[0].khi - t[0].klo == sc.OFFSET_MAX and t[1].klo - t[0].klo == 0xffffffff
    assert (t[1].bl0, t[1].bl1) == (lay.nblk - 1, lay.nblk) and lay.kind_at(lay.L - 1) == "real"
    assert lay.hdr(lay.nblk - 1) < 0xfffffffe and lay.kind_at((lay.nblk - 1) * B) == "filler"
    assert c.geometry().wgs == 512


# ---- sample ranges ------------------------------------------------------------------------------------------------------------
def test_sample_range_cases():
    c = sc.case_ladder272()
    lay = c.layout()
    assert [c.samples[f"n{n}"].size for n in (1, 64, 65, 4096, 4097)] == [1, 64, 65, 4096, 4097]
    assert int(c.samples["below"].max()) < int(c.hashes[0]) and int(c.samples["above"].min()) > lay.max_hash
    for env in sc.ALL_ENVS:
        g = c.geometry(sc.wgs_of(env))
        last = g.n_ranges() - 1

        def sizes(label):
            keys = g.keys_of(c.samples[label])
            return [b - a for a, b in (g.sample_range(w, keys) for w in range(g.wgs))]
        assert not any(sizes("below")) and not any(sizes("above")) and not any(sizes("below_above"))
        fl = sizes("first_last")
        assert sum(fl) == 2 and (fl[0], fl[last]) == ((1, 1) if last else (2, 2))
        ob = sizes("one_block")
        assert sum(1 for x in ob if x) == 1 and max(ob) == c.samples["one_block"].size
        assert sum(sizes("n4097")) >= 4097          # (a key on a range boundary is staged on both sides)


def test_hashes_above_the_largest_key_make_no_tiles():
    c = sc.case_above()
    smp = c.samples["far_above"]
    lay = c.layout()
    far = smp[smp > np.uint64(lay.max_hash)]
    assert far.size == sc.N_FAR == 4096 and np.all(np.diff(far) >> np.uint64(lay.sshift) > 2 ** 32)
    assert int(far[0]) - lay.max_hash > 2 ** 32 and len(c.notes["hits"]) == smp.size - far.size
    before = c.geometry(1, last="ones").tiles(0, smp)
    assert len(before) == 1 + sc.N_FAR and all(t.n == 1 and (t.bl0, t.bl1) == (2, 3) for t in before[1:])
    now = c.geometry(1).tiles(0, smp)
    assert len(now) == 1 and now[0].n == len(c.notes["hits"]) and now[0].single
    assert c.geometry(1).tiles(0, c.samples["only_far_above"]) == []


# ---- the counts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.all_cases(), ids=_ids(sc.all_cases()))
def test_oracle_agrees_with_a_set_based_count(case):
    values, offsets = case.csr()
    for label, smp in case.samples.items():
        ov = oracle.overlap(values, offsets, smp)
        e, m = oracle.exclusive(values, offsets, ov > 0, smp)
        w_ov, w_e, w_m = sc.set_counts(case, smp)
        assert np.array_equal(ov, w_ov), label
        assert np.array_equal(np.where(ov > 0, e, 0), w_e) and np.array_equal(np.where(ov > 0, m, 0), w_m), label


def test_samples_hit_what_they_are_named_for():
    c = sc.case_ladder272()
    values, offsets = c.csr()
    for start, m in sc.RUNS_272:
        ov = oracle.overlap(values, offsets, c.samples[f"run{start}x{m}:alone"])
        assert ov[:m].tolist() == [1] * m and int(ov.sum()) == m
    for c in sc.cases_trunc():
        values, offsets = c.csr()
        assert int(oracle.overlap(values, offsets, c.samples["last_of_group"]).sum()) == 1
        assert int(oracle.overlap(values, offsets, c.samples["other_low"]).sum()) == 2
        assert int(oracle.overlap(values, offsets, c.samples["largest_other_low"]).sum()) == 0
    c = sc.case_fillers()
    values, offsets = c.csr()
    assert int(oracle.overlap(values, offsets, c.samples["filler_keys"]).sum()) == 0
    assert int(oracle.overlap(values, offsets, c.samples["behind"]).sum()) == 4
    c = sc.case_wide()
    assert oracle.overlap(*c.csr(), c.samples["all4"]).tolist() == [2, 2]
    c = sc.case_above()
    assert int(oracle.overlap(*c.csr(), c.samples["far_above"]).sum()) == len(c.notes["hits"])
