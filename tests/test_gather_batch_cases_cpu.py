"""Guards for tests/gather_batch_cases.py, with the oracles alone (no device, no library call): the blocks still hold what
they are named for -- samples that finish in different rounds, a cap that cuts some samples and not others, a round the tie
rule decides, member bytes whose other bits sit on non-candidates -- and the oracle on the candidates alone agrees with the
oracle on the whole database."""
import numpy as np
import pytest
from gather_batch_cases import (EDGE_SIZES, OTHER_BITS, SET_A, SET_B, TILE, big_block, candidates, descending_block, hand_block,
                                oracle_on_candidates, posting_block, want, wide_block)
from gather_cases import hand_written
from gather_oracle import gather_oracle

from yacht_amd import _lib


def _other_bits_on_non_candidates(block):
    for mask in block["masks"]:
        for s in range(len(block["samples"])):
            non = candidates(block, s, mask) == 0
            if non.any():
                assert (block["members"][s][non] & np.uint8(0xFF & ~mask)).any(), (mask, s)


def test_constants_match_the_library():
    from gather_batch_cases import MAX_ROWS
    assert TILE == _lib.YH_GATHER_BATCH_TILE and MAX_ROWS == _lib.YH_GATHER_BATCH_MAX_ROWS


def test_hand_block():
    block = hand_block()
    _values, _offsets, _sample, _cand, _abund, rows, owner = hand_written()
    got = want(block, SET_A)
    assert [(int(r["ref"]), int(r["n_overlap"]), int(r["n_unique"]), int(r["w_unique"])) for r in got[0][0]] == rows
    assert got[0][2].tolist() == owner
    assert len(got[1][0]) > len(got[0][0]) and 0 in got[1][0]["ref"].tolist()  # all candidates: reference 0 joins, and wins a round
    assert len(got[2][0]) == 0 and len(got[3][0]) == 0 and got[3][2].size == 0
    assert len({len(g[0]) for g in got}) >= 3  # the samples finish in different rounds
    _other_bits_on_non_candidates(block)


@pytest.mark.parametrize("length", [4, 5, 300])
def test_posting_block(length):
    block = posting_block(length)
    got = want(block, SET_A)
    tables = [candidates(block, s, SET_A) for s in range(3)]
    assert not np.array_equal(tables[0], tables[1]) and not np.array_equal(tables[0], tables[2]) and not np.array_equal(tables[1], tables[2])
    assert all(len(g[0]) >= 3 for g in got) and len({len(g[0]) for g in got}) >= 2
    capped = want(block, SET_A, cap_rows=2)
    assert all(g[1] for g in capped)
    _other_bits_on_non_candidates(block)


def test_big_blocks():
    for n in (1, 2, 65, 256):
        block = big_block(n)
        assert len(block["samples"]) == n and block["members"].shape[0] == n
        _other_bits_on_non_candidates(block)
        assert (block["members"] & np.uint8(OTHER_BITS)).any()
    sizes = {s.size for s in big_block(65)["samples"]}
    assert set(EDGE_SIZES) <= sizes and max(sizes) > 100_000  # (big_sample(120_000))
    assert max(s.size for s in big_block(256)["samples"]) <= 1100
    block = big_block(65)
    for mask in (SET_A, SET_B):
        got = want(block, mask)
        assert len({len(g[0]) for g in got}) >= 5  # the samples finish in different rounds
        assert max(len(g[0]) for g in got) >= 30
    a, b = want(block, SET_A), want(block, SET_B)
    assert any(not np.array_equal(x[0], y[0]) for x, y in zip(a, b))  # the two sets rank differently
    # at a cap of 8 rows some samples are cut short and some are not
    capped = want(block, SET_A, cap_rows=8)
    assert any(g[1] for g in capped) and any(not g[1] for g in capped)
    # a round the tie rule decides (references 300 and 360 are identical candidates), from the oracle on everything, which
    # must agree with the oracle on the candidates alone
    for s in (5, 64):
        stats = {}
        full = gather_oracle(block["values"], block["offsets"], block["samples"][s], candidates(block, s, SET_A), block["abunds"][s], stats=stats)
        assert stats["n_tie_rounds"] >= 1 and stats["n_owned_shared"] >= 10 and stats["n_shared_both_sides"] >= 10, (s, stats)
        assert np.array_equal(full[0], a[s][0]) and full[1] == a[s][1] and np.array_equal(full[2], a[s][2]), s
    # the full block: every sample has rows, not all the same number
    got = want(big_block(256), SET_A)
    assert all(len(g[0]) >= 1 for g in got) and len({len(g[0]) for g in got}) >= 4


def test_oracle_on_candidates_agrees_on_the_hand_written_database():
    values, offsets, sample, cand, abund, _rows, _owner = hand_written()
    for table in (cand, np.ones_like(cand), np.zeros_like(cand)):
        for stops in ({}, {"cap_rows": 2}, {"min_hits": 3}):
            a = gather_oracle(values, offsets, sample, table, abund, **stops)
            b = oracle_on_candidates(values, offsets, sample, table, abund, **stops)
            assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])


def test_descending_block():
    block = descending_block(40)
    got = want(block, SET_A)
    assert [len(g[0]) for g in got] == list(range(40))  # sample s finishes after s rounds
    assert all(g[0]["ref"].tolist() == list(range(s)) for s, g in enumerate(got))
    for cap in (31, 32, 33):
        capped = want(block, SET_A, cap_rows=cap)
        assert [g[1] for g in capped] == [s > cap for s in range(40)]  # more = 1 exactly behind the cap; n_rows == cap gives 0
    stopped = want(block, SET_A, min_hits=30)
    assert 0 < max(len(g[0]) for g in stopped) < 39 and any(len(g[0]) < s for s, g in enumerate(stopped))
    _other_bits_on_non_candidates(big_block(2))


def test_wide_block():
    got = want(wide_block(), SET_A)
    assert int(got[0][0]["w_unique"][0]) > 2 ** 43 and int(got[1][0]["w_unique"][0]) > 2 ** 42
    assert len(got[0][0]) >= 2
