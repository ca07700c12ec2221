"""The expectations of the segmented-sketch cases (tests/sketch_seg_cases.py), checked without a GPU: what the vectorised
oracle says per segment against a statement over the WHOLE buffer (every window's hash, kept when the window lies inside
its segment), and against the scalar restatement tests/sketch_scalar.py on the small cases.  Also what the cases must
cover, so that a change to a builder cannot quietly empty a case."""
import numpy as np

import sketch_scalar as sc
import sketch_seg_cases as sg
import test_gpu_sketch_edges as edges
from oracle import sketch_oracle as so


def _by_window_rule(case):
    """the issue's rule stated on the whole buffer: window i belongs to the segment s with off[s] <= i < off[s + 1] and
    counts when it is valid and i + k <= off[s + 1]"""
    buf, off, k = case["buf"], case["seg_off"].astype(np.int64), case["k"]
    mh = np.uint64(so.max_hash_for_scaled(case["scaled"]))
    n_seg = off.size - 1
    if buf.size < k:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros(n_seg + 1, np.uint64)
    valid = edges.valid_windows(buf, k)
    h = np.zeros(valid.size, dtype=np.uint64)
    h[valid] = so.kmer_hashes(buf.tobytes(), k)
    i = np.arange(valid.size)
    s = np.searchsorted(off, i, side="right") - 1
    inside = i + k <= off[np.minimum(s + 1, n_seg)]
    keep = valid & inside & (h <= mh)
    pairs = np.stack([s[keep].astype(np.uint64), h[keep]], axis=1)
    uniq, counts = np.unique(pairs, axis=0, return_counts=True) if pairs.size else (np.zeros((0, 2), np.uint64), np.zeros(0, np.int64))
    o = np.searchsorted(uniq[:, 0], np.arange(n_seg + 1, dtype=np.uint64), side="left")
    return uniq[:, 1].astype(np.uint64), counts.astype(np.uint32), o.astype(np.uint64)


def test_expectations_agree_with_the_window_rule():
    for case in sg.all_cases():
        mins, abund, off = sg.expected(case["name"])
        m2, a2, o2 = _by_window_rule(case)
        assert np.array_equal(mins, m2) and np.array_equal(abund, a2) and np.array_equal(off, o2), case["name"]
        assert off.size == case["seg_off"].size and int(off[-1]) == mins.size == abund.size
        for s in range(off.size - 1):
            m = mins[int(off[s]):int(off[s + 1])]
            assert bool(np.all(m[1:] > m[:-1])), (case["name"], s)


def test_expectations_agree_with_the_scalar_restatement():
    small = [c for c in sg.all_cases() if c["small"]]
    assert len(small) >= 5
    for case in small:
        mh = so.max_hash_for_scaled(case["scaled"])
        mins, abund, off = [], [], [0]
        for seg in sg.segments(case):
            kept = sorted(h for h in sc.kmer_hashes(seg, case["k"]) if h <= mh)
            u = sorted(set(kept))
            mins += u
            abund += [kept.count(x) for x in u]
            off.append(len(mins))
        want = sg.expected(case["name"])
        assert want[0].tolist() == mins and want[1].tolist() == abund and want[2].tolist() == off, case["name"]


def test_cases_cover_what_they_are_for():
    names = [c["name"] for c in sg.all_cases()]
    # 1: all three kernels, boundaries on both sides of a workgroup edge, every window kept (the LDS list overflows)
    kernels = {}
    for c in sg.boundary_cases():
        kernels.setdefault(sg.kernel_of(c), []).append(c)
        grid = sg.SK_WIN if sg.kernel_of(c) == "bytes" else sg.RL_WIN
        cuts = set(int(x) for x in c["seg_off"][1:-1])
        assert cuts & {grid - 1, grid, grid + 1} and cuts & {2 * grid - 1, 2 * grid, 2 * grid + 1}
        # (the byte-wise kernel's workgroup has no more windows than the list has slots: only the 2-bit kernels overflow)
        assert c["scaled"] == 1 and (grid == sg.SK_WIN or sg.kept_total(c["name"]) > 2 * sg.SK_LCAP)
        # windows are lost at every boundary: fewer than the buffer as one sequence has
        assert sg.kept_total(c["name"]) == c["buf"].size - c["k"] + 1 - sum(
            min(c["k"] - 1, int(c["seg_off"][s + 1] - c["seg_off"][s])) for s in range(c["seg_off"].size - 2))
    assert sorted(kernels) == ["128", "64", "bytes"] and {c["k"] for c in kernels["bytes"]} == {31, 70}
    assert {c["k"] for c in kernels["64"]} == {21, 32} and {c["k"] for c in kernels["128"]} == {33, 51, 64}
    # 2: about 3 000 segments, most of them empty sketches, zero-length runs at both ends
    for c in sg.tiny_cases():
        off = sg.expected(c["name"])[2]
        lens = np.diff(c["seg_off"].astype(np.int64))
        assert lens.size == 3010 and not lens[:5].any() and not lens[-5:].any() and sg.RL_WIN * lens.size // c["buf"].size > 300  # (per workgroup)
        assert int((np.diff(off.astype(np.int64)) == 0).sum()) > lens.size // 2 and int(off[-1]) > 500
    # 3: abundance 3 everywhere in the first segment, 1 in the second, the same hashes in both
    mins, abund, off = sg.expected("strands-k31")
    a, b = int(off[1]), int(off[2])
    assert a == b - a == 3001 - 31 + 1 and bool(np.all(abund[:a] == 3)) and bool(np.all(abund[a:] == 1))
    assert np.array_equal(mins[:a], mins[a:])
    mins, abund, off = sg.expected("palindromes-k32")
    assert 0 < int(off[1]) < int(off[2]) and int(abund.sum()) < 3 * 32 + 1   # (the cut costs the family member it falls in)
    # 4: some workgroups keep more than the LDS list holds, some fewer
    for c in sg.overflow_cases():
        assert c["seg_off"].size == 6 and c["buf"].size == 3 * sg.RL_WIN
    assert all(x > sg.SK_LCAP for x in per_wg_of("overflow-s2")) and any(x > sg.SK_LCAP for x in per_wg_of("overflow-s4")) and \
        any(x <= sg.SK_LCAP for x in per_wg_of("overflow-s4"))
    c = sg.low_complexity_case()    # more kept hashes than 1.25 x what a random sequence keeps, + 4 096
    assert sg.kept_total(c["name"]) > (c["buf"].size - c["k"] + 1) * 0.5 * 1.25 + 4096
    # 5: real records, one segment each
    for c in sg.real_cases():
        assert 150_000 < c["buf"].size <= 200_000 and c["seg_off"].size > 3 and int(sg.expected(c["name"])[2][-1]) > 100
    assert len(names) == len(set(names))


def per_wg_of(name):
    """hashes under the threshold per workgroup of 8 192 windows (what fills the LDS list: windows that leave their segment too)"""
    c = sg.case_named(name)
    k, buf = c["k"], c["buf"]
    valid = edges.valid_windows(buf, k)
    h = np.full(valid.size, 2 ** 64 - 1, dtype=np.uint64)
    h[valid] = so.kmer_hashes(buf.tobytes(), k)
    assert c["scaled"] > 1
    return [int((h[w * sg.RL_WIN:(w + 1) * sg.RL_WIN] <= np.uint64(so.max_hash_for_scaled(c["scaled"]))).sum()) for w in range(3)]
