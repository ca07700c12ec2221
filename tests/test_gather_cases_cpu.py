"""The cases of tests/gather_cases.py still hold what they are named for: checked with the oracles alone, no GPU."""
import numpy as np
import pytest
from gather_cases import BIG_SIZES, LIST_LENGTHS, ROUNDS, assert_big_classes, big, big_sample, descending, hand_written, posting_lists
from gather_oracle import NOBODY, gather_oracle, gather_sets

from yacht_amd import _lib


def test_hand_written_rows_are_what_the_contract_gives():
    values, offsets, sample, cand, abund, rows, owner = hand_written()
    for oracle in (gather_sets, gather_oracle):
        got, more, own = oracle(values, offsets, sample, cand, abund)
        assert [(int(r["ref"]), int(r["n_overlap"]), int(r["n_unique"]), int(r["w_unique"])) for r in got] == rows and not more
        assert own.tolist() == owner
    # the round-0 tie, the tie that a decrement makes, and the reference that falls to 0 without winning
    held = lambda j: set(values[int(offsets[j]):int(offsets[j + 1])].tolist()) & set(sample.tolist())  # noqa: E731
    assert len(held(1)) == len(held(2)) == 5 and rows[0][0] == 1
    assert len(held(2) - held(1)) == len(held(3)) == len(held(4)) == 3 and rows[1][0] == 2
    assert len(held(5)) == 2 and held(5) <= held(4) and 5 not in [r[0] for r in rows]
    assert 10 in held(0) and 10 in held(1) and cand[0] == 0 and owner[list(sample).index(10)] == 1


@pytest.mark.parametrize("length", LIST_LENGTHS)
def test_posting_list_cases(length):
    values, offsets, sample, cand, abund, groups = posting_lists(length)
    n_refs = offsets.size - 1
    u, k = np.unique(values, return_counts=True)
    assert set(k.tolist()) == {1, length} and int((k == length).sum()) == 15  # every shared hash has `length` holders
    rows, more, owner = gather_oracle(values, offsets, sample, cand, abund)
    if length <= 9:
        sets = gather_sets(values, offsets, sample, cand, abund)
        assert np.array_equal(rows, sets[0]) and np.array_equal(owner, sets[2])
    assert rows["ref"][:3].tolist() == [0, n_refs - 1, 2]  # A, Z, M
    f, l, x = groups["F"], groups["L"], groups["X"]
    assert f[1][0] == 0 == min(f[1]) and l[1][-1] == n_refs - 1 == max(l[1])  # the winner first, the winner last
    assert not ({0, n_refs - 1, 2} & set(x[1])) and all(2 not in g[1] for g in groups.values())  # the winners absent
    for g in groups.values():  # candidates and others mixed in every list
        assert 0 < int(cand[g[1]].sum()) < length or length == 2
    at = lambda block: np.searchsorted(sample, block)  # noqa: E731
    assert (owner[at(f[0])] == 0).all() and (owner[at(l[0])] == n_refs - 1).all()
    x_owner = set(owner[at(x[0])].tolist())
    assert len(x_owner) == 1 and x_owner <= set(x[1]) and cand[list(x_owner)[0]] == 1  # one candidate of X's holders took X


@pytest.mark.parametrize("n_sample", BIG_SIZES)
def test_big_cases_have_every_class(n_sample):
    refs, values, offsets, cand, present = big()
    assert int(cand.sum()) == 60 + 1 + 9 + 10 and np.array_equal(refs[360], refs[300]) and cand[361] == 0
    sample, abund = big_sample(n_sample)
    lo = {120_000: 100_000, 300_000: 262_144, 600_000: 524_288}[n_sample]
    hi = {120_000: 262_144, 300_000: 524_288, 600_000: 1 << 40}[n_sample]
    assert lo <= sample.size < hi  # (the tile shape this case is for)
    stats = {}
    rows, more, owner = gather_oracle(values, offsets, sample, cand, abund, stats=stats)
    assert_big_classes(stats, rows)
    # the copy of the first cluster's parent never wins anything: the parent (the lower index) took it all
    assert 300 in rows["ref"].tolist() and 360 not in rows["ref"].tolist()


@pytest.mark.parametrize("n_rows", [ROUNDS - 1, ROUNDS, ROUNDS + 1, 2 * ROUNDS])
def test_chunk_edge_cases_have_exactly_their_rows(n_rows):
    assert ROUNDS == _lib.YH_GATHER_ROUNDS_PER_SYNC
    values, offsets, sample, cand, abund = descending(n_rows)
    rows, more, owner = gather_oracle(values, offsets, sample, cand, abund)
    assert len(rows) == n_rows and rows["ref"].tolist() == list(range(n_rows)) and not more
    assert rows["n_unique"].tolist() == list(range(n_rows + 2, 2, -1)) and int((owner == NOBODY).sum()) == 3
