"""The case generators of tests/packed_cases.py against the host packer (no GPU): every case round-trips, the packer chose the
width every block was built for, and the case list as a whole still reaches what tests/test_gpu_packed_edges.py is there to
reach -- every width 0..64, gaps that straddle a 64-bit word and gaps that end exactly on one, the block tails, the sketch
sizes around the block size.  A change to a generator that silently empties the GPU tests fails here."""
import numpy as np
import pytest

import packed_cases as pc
from yacht_amd import _lib
from yacht_amd.engine import csr_pack, csr_unpack, pack_sample, unpack_sample


@pytest.fixture(scope="module")
def cases():
    return pc.sample_cases()


def test_sample_cases_roundtrip_at_the_intended_widths(cases):
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    for c in cases:
        a = c.hashes
        assert a.size <= pc.MAX_SAMPLE and np.all(a[1:] > a[:-1]), c.name
        p = pack_sample(a)
        assert np.array_equal(unpack_sample(p), a), c.name
        assert pc.sample_block_widths(p) == c.widths, c.name


def test_every_width_occurs(cases):
    seen = {w for c in cases for w in c.widths}
    assert seen == set(range(65))
    # the wide gap of every width 57..64 at every one of the lanes around the wave boundaries, in a full block
    for w in range(57, 65):
        lanes = set()
        for c in cases:
            a = c.h
            for b, bw in enumerate(c.widths):
                blk = a[b * pc.BLOCK: (b + 1) * pc.BLOCK]
                if bw == w and len(blk) == pc.BLOCK:
                    lanes |= {i for i in range(1, pc.BLOCK) if (blk[i] - blk[i - 1] - 1) >> (w - 1)}
        assert lanes >= set(pc.WIDE_LANES), (w, sorted(lanes))


def test_gaps_straddle_words_and_end_on_words(cases):
    """A gap straddles a word when sh + w > 64 and ends on one when sh + w == 64 (sh = its first bit mod 64).  Widths that
    divide 64 (1, 2, 4, 8, 16, 32) can never straddle: every gap of theirs lies inside a word; 64 always fills one."""
    straddle, exact = set(), set()
    for c in cases:
        for b, w in enumerate(c.widths):
            cnt = min(pc.BLOCK, len(c.h) - b * pc.BLOCK)
            s, e = pc.gap_fits(w, cnt)
            if s:
                straddle.add(w)
            if e:
                exact.add(w)
    assert exact >= set(range(1, 65))
    assert straddle == {w for w in range(1, 64) if 64 % w}


def test_block_tails_and_sizes(cases):
    by_size = {}
    for c in cases:
        by_size.setdefault(len(c.h), set()).add(c.widths[-1])
    for n in pc.TAIL_SIZES:
        cnt = (n - 1) % pc.BLOCK + 1
        want = {w for w in pc.TAIL_WIDTHS if cnt >= 2 or w == 0}
        assert by_size.get(n, set()) >= want, (n, by_size.get(n))
    tails = {(len(c.h) - 1) % pc.BLOCK + 1 for c in cases}
    assert tails >= {1, 2, 63, 64, 65, 255, 256}
    top = [c for c in cases if c.h[-1] == pc.TOP - 1 and c.widths[-1] == 0 and len(c.h) % pc.BLOCK == 0]
    assert top and all(c.h[-pc.BLOCK:] == list(range(pc.TOP - pc.BLOCK, pc.TOP)) for c in top)
    assert any(c.h == [0, pc.TOP - 1] for c in cases)
    assert any(c.widths[-2:] == [0, 0] and len(c.h) == pc.BLOCK + 2 for c in cases)   # a run and a tail of 2, both width 0


def test_forged_samples_are_ordering_errors_only():
    """The two forgeries keep every size, width and payload offset of the packer (so yh_pack_validate passes them and the
    device reads what a good sample reads); the host decoder refuses both as unsorted."""
    for forge in (pc.forge_last_lane_wraps, pc.forge_block_meets_next_base):
        good, forged = forge(pack_sample)
        p = pack_sample(good)
        assert forged.size == p.size and np.flatnonzero(forged != p).size <= 8
        diff = np.flatnonzero(forged != p)
        b = (int(diff[0]) - 32) // 16
        assert all(32 + 16 * b <= int(d) < 32 + 16 * b + 8 for d in diff), "only a block's base may differ"
        with pytest.raises(_lib.YachtHipError) as e:
            unpack_sample(forged)
        assert e.value.code == _lib.YH_ERR_UNSORTED


@pytest.mark.parametrize("kind", pc.CSR_KINDS)
def test_csr_databases_roundtrip_at_the_intended_widths(kind):
    values, offsets, widths = pc.csr_database(kind)
    blob = csr_pack(values, offsets)
    v2, o2 = csr_unpack(blob)
    assert np.array_equal(v2, values) and np.array_equal(o2, offsets)
    assert pc.csr_block_widths(blob) == widths
    sizes = np.diff(offsets.astype(np.int64))
    assert offsets.size - 1 >= 4                                   # (the device expansion wants at least four references)
    if kind in ("sizes", "top"):
        assert tuple(sizes[: len(pc.CSR_SIZES)]) == pc.CSR_SIZES
        assert {0, 1, 37, 56, 63} <= set(widths)
        assert sizes[len(pc.CSR_SIZES):].min() == 0                 # an empty sketch inside the cluster too
        # gaps that straddle a word and gaps that end on one, at every width that can
        fits = {}
        b = 0
        for size in sizes:
            for first in range(0, int(size), pc.BLOCK):
                s, e = pc.gap_fits(widths[b], min(pc.BLOCK, int(size) - first))
                got = fits.setdefault(widths[b], [False, False])
                got[0] |= s
                got[1] |= e
                b += 1
        assert b == len(widths)
        assert fits[37] == [True, True] and fits[56] == [True, True] and fits[63] == [True, True] and fits[1][1]
    if kind == "sizes":
        assert int(values.max()) < 1 << 63
    if kind == "top":
        assert 64 in widths and int(values.max()) == pc.TOP - 1
        refs = [values[int(offsets[j]): int(offsets[j + 1])] for j in range(offsets.size - 1)]
        assert any(r.size > pc.BLOCK and int(r[-1]) == pc.TOP - 1 for r in refs)
        # full blocks of width 64 whose wide gap is followed by words that are not zero (other gaps, the next block)
        lanes = set()
        for r in refs:
            if r.size >= pc.BLOCK:
                g = [int(q) - int(p) - 1 for p, q in zip(r[: pc.BLOCK - 1], r[1: pc.BLOCK])]
                lanes |= {i + 1 for i, x in enumerate(g) if x >> 63 and (i + 1 < len(g) and g[i + 1] or r.size > pc.BLOCK + 1)}
        assert lanes >= {64, 255}, lanes
    if kind == "tiny":
        assert offsets.size - 1 == 300 and set(sizes) == {0, 1, 2, 3}
        runs = "".join("e" if s == 0 else "x" for s in sizes)
        assert "eee" in runs                                       # a run of empty sketches for the block lookup to pass over


@pytest.mark.parametrize("n", pc.ROWS_N)
def test_rows_patterns_select_what_they_name(n):
    values, offsets = pc.rows_database(n)
    refs = [set(int(x) for x in values[int(offsets[j]): int(offsets[j + 1])]) for j in range(n)]
    pats = pc.rows_patterns(n)
    assert set(pats) >= {"none", "all", "first", "last", "bit0", "bit31", "p01", "p50"} and (("only2048" in pats) == (n > 2048))
    assert pats["all"].size == n and pats["none"].size == 0 and list(pats["last"]) == [n - 1]
    for name, hit in pats.items():
        s = set(int(x) for x in pc.rows_sample(n, hit))
        got = [j for j in range(n) if refs[j] & s]
        assert got == [int(j) for j in hit], name
    if n >= 10:                                                     # the shared hashes make the three counts differ
        s = set(int(x) for x in pc.rows_sample(n, pats["all"]))
        assert any(len(refs[j] & s) == 2 for j in range(n))
