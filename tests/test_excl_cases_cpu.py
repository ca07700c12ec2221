"""No GPU: every case of tests/excl_cases.py reaches the state it is named for, and the oracle's exclusive counts for every
(case, subset) agree with a second, independent computation.

The state comes from the plain-Python mirror in excl_cases.py: records and pieces per reference, the one record with more than
three other holders and where the build's order puts it, list lengths, multiplicities, the subset words on either side of
EXCL_LDS_WORDS, and -- from oracle.overlap -- that every private-only sample makes exactly its subset.  The counts that
tests/test_gpu_excl_edges.py expects from the kernels are oracle.exclusive's; here they are pinned against a set-based count
from the mirror everywhere (n_excl[r] = |R_r| - nshared_r + the multiplicities of r's records with no other holder in the
subset) and against oracle.exclusive_py where that is fast enough.
"""
import numpy as np
import pytest

import excl_cases as ec
from oracle import oracle


def _ids(cases):
    return [c.name for c in cases]


# ---- the mirror itself ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ec.all_cases(), ids=_ids(ec.all_cases()))
def test_mirror_counts_what_the_csr_holds(case):
    """n_holder_sets as test_holder_sets_are_the_distinct_ones counts it (Python sets over the CSR), the shared postings and the
    sizes: the mirror is derived from the table, this from the packed database."""
    values, offsets = case.csr()
    mir = case.mirror()
    assert np.array_equal(np.diff(offsets.astype(np.int64)), mir.sizes)
    refs = np.repeat(np.arange(case.n_refs), mir.sizes)
    order = np.argsort(values, kind="stable")
    v, r = values[order], refs[order]
    starts = np.flatnonzero(np.r_[True, v[1:] != v[:-1]])
    ends = np.r_[starts[1:], v.size]
    sets, postings = set(), 0
    for a, b in zip(starts[ends - starts > 1], ends[ends - starts > 1]):
        holders = tuple(r[a:b].tolist())
        postings += len(holders)
        for j in holders:
            sets.add((j, tuple(o for o in holders if o != j)) if len(holders) <= ec.INLINE_MAX else (j, "long", int(v[a])))
    assert len(sets) == mir.n_holder_sets()
    assert postings == mir.n_shared_postings
    for j in range(case.n_refs if case.n_refs < 5000 else 0):
        s = values[int(offsets[j]):int(offsets[j + 1])]
        assert np.all(s[1:] > s[:-1])


def test_hashes_stay_below_the_scaled_bound_and_fit_compact_buckets():
    for case in ec.all_cases():
        values, _ = case.csr()
        distinct = np.unique(values).size
        assert int(values.max()) < ec.MAX_HASH_SCALED_1000
        assert int(values.max()) // ((distinct * 2 + 4) // 5) < 2 ** 32       # a compact bucket spans < 2^32 hash values
        assert int(case.noise.min()) > int(values.max())


# ---- case 1 ------------------------------------------------------------------------------------------------------------------
def test_forms_reach_every_record_form():
    c = ec.case_forms()
    mir = c.mirror()
    table = c.notes["table"]
    assert sorted({k for k, *_ in table}) == sorted(ec.FORM_K) and len(table) == 3 * len(ec.FORM_K)
    for i, (k, place, t, h) in enumerate(table):
        assert len(h) == k and t in h
        assert {"low": h[0], "mid": h[(k - 1) // 2] if k > 2 else t, "high": h[-1]}[place] == t
        if place == "mid" and k > 2:
            assert h[0] < t < h[-1]
        others = tuple(o for o in h if o != t)
        if k <= ec.INLINE_MAX:
            rec = dict(mir.inline_records[t])
            assert rec[others] == 1 + i % 3
            assert (len(others) > ec.REC_OTHERS) == (k >= 5)         # k = 5..8 needs recx; k = 8 fills the seven slots
        else:
            assert sum(1 for hh, _ in mir.list_records[t] if hh == h) == 1 + i % 3      # one record per hash
    for t in ec.FORM_UNDER_TEST.values():
        assert mir.list_lengths(t) == [9, 10, 16, 17, 64, 65]
        assert max(len(o) for o, _ in mir.inline_records[t]) == 7
    # the subsets: nobody else / one other at inline slots 0, 2, 3, 6 / at list positions 0, 7, 8, len - 1 / two in the first step
    for k, place, t, h in table:
        subs = ec.form_subsets(k, t, h)
        others = [o for o in h if o != t]
        assert subs["alone"] == (t,)
        if k <= ec.INLINE_MAX:
            assert sorted(subs) == sorted(["alone"] + [f"slot{s}" for s in ec.INLINE_SLOTS if s < k - 1])
            for s in ec.INLINE_SLOTS:
                if s < k - 1:
                    assert set(subs[f"slot{s}"]) == {t, others[s]}
            if k == 8:
                assert "slot6" in subs
        else:
            for p in (0, 7, 8, k - 1):
                assert (f"pos{p}" in subs) == (h[p] != t)
                if h[p] != t:
                    assert set(subs[f"pos{p}"]) == {t, h[p]}
            two = set(subs["two_in_step0"]) - {t}
            assert len(two) == 2 and two <= set(h[:8])
    # walks of the list form, eight holders a step: 9 -> two steps with a clamped tail, 16 -> two exact, 17 -> three
    assert [-(-k // 8) for k in (9, 16, 17)] == [2, 2, 3] and 9 % 8 and not 16 % 8


# ---- case 2 ------------------------------------------------------------------------------------------------------------------
def test_recx_read_is_decided_by_one_record():
    last, first, none = ec.cases_recx()
    for c, want in ((last, [255]), (first, [0]), (none, [])):
        mir = c.mirror()
        assert mir.n_records(ec.RECX_T) == 256 and mir.set_pieces(ec.RECX_T) == 1
        assert mir.wide_records(ec.RECX_T) == want                     # lane 63 of the last sweep / lane 0 of the first / none
        keys = [ec.record_key(o) for o, _ in mir.inline_records[ec.RECX_T]]
        assert keys == sorted(keys) and len(set(keys)) == 256
        for r in mir.refs_with_records():
            if r != ec.RECX_T:
                assert mir.wide_records(r) == [] or c.notes["wide"] and r in c.notes["wide"]
        if want:
            wide = c.notes["wide"]
            assert len(wide) == 4 and 0 not in wide and mir.inline_records[ec.RECX_T][want[0]] == (wide, 1)
            assert set(c.subsets["wide_slot3"]) == {ec.RECX_T, wide[3]}
        assert all(0 not in h for h, _ in c.entries)                  # reference 0 shares nothing


# ---- case 3 ------------------------------------------------------------------------------------------------------------------
def test_sweeps_have_exactly_d_records_and_end_at_the_arrays_end():
    assert [c.n_refs - 2 for c in ec.cases_sweep()] == list(ec.SWEEP_D)
    for c, d in zip(ec.cases_sweep(), ec.SWEEP_D):
        mir = c.mirror()
        for t in (0, d + 1):
            assert mir.n_records(t) == d and mir.set_pieces(t) == -(-d // 256) == mir.posting_pieces(t)
            assert all(len(o) == 1 and m == 1 for o, m in mir.inline_records[t])
            assert sorted(o[0] for o, _ in mir.inline_records[t]) == list(range(1, d + 1))
        # the last reference's records are the last of the database: its last piece ends at n_sets and at n_postings
        assert max(mir.refs_with_records()) == d + 1
        assert mir.n_holder_sets() == 4 * d == mir.n_shared_postings
        assert c.subsets["both_alone"] == (0, d + 1)
        for at in ec.SWEEP_AT + (d - 1,):
            if at < d:
                p = c.subsets[f"record{at}"]
                assert mir.inline_records[0][at][0][0] in p and mir.inline_records[d + 1][at][0][0] in p and len(p) <= 4


# ---- case 4 ------------------------------------------------------------------------------------------------------------------
def test_multiplicities_and_near_equal_sets():
    c = ec.case_mult()
    mir = c.mirror()
    for i, m in enumerate(ec.MULT_M):
        assert mir.inline_records[2 * i] == [((2 * i + 1,), m)] and mir.inline_records[2 * i + 1] == [((2 * i,), m)]
        assert mir.nshared[2 * i] == m
    assert 65_535 in ec.MULT_M and 65_536 in ec.MULT_M and max(ec.MULT_M) == 70_000
    a, b, cc, d, e = ec.MULT_A, ec.MULT_B, ec.MULT_C, ec.MULT_D, ec.MULT_E
    assert dict(mir.inline_records[ec.MULT_T]) == {(a, b, cc): 3, (a, b, cc, d): 5, (a, b, cc, e): 7}
    assert dict(mir.inline_records[ec.MULT_T2]) == {(a, b, cc): 2}          # the same set on another reference
    assert mir.wide_records(ec.MULT_T) and len(mir.wide_records(ec.MULT_T)) == 2
    for r in ec.MULT_DUP:                                                   # whole duplicates: nothing of their own
        assert mir.sizes[r] == 50 == mir.nshared[r]
    values, offsets = c.csr()
    lo, hi = (values[int(offsets[r]):int(offsets[r + 1])] for r in ec.MULT_DUP)
    assert np.array_equal(lo, hi)
    subs = [set(c.subsets[k]) for k in ("t_no_d_no_e", "t_with_d", "t_with_e", "t_with_d_e")]
    assert [(d in s, e in s) for s in subs] == [(False, False), (True, False), (False, True), (True, True)]


# ---- case 5 ------------------------------------------------------------------------------------------------------------------
def test_work_list_blocks():
    assert [c.n_refs for c in ec.cases_work()] == [256, 257, 1024, 1025, 4096, 4097]
    for c in ec.cases_work():
        n = c.n_refs
        mir = c.mirror()
        pieces = {r: mir.set_pieces(r) for r in range(n)}
        assert all(mir.set_pieces(r) == mir.posting_pieces(r) for r in range(n))
        for b in ec.WORK_BLOCKS:
            if 256 * b + 255 < n:
                assert [pieces[256 * b + lane] for lane in (0, 63, 64, 255)] == [0, 1, 2, 3]
        for r in ec.WORK_FIRSTS:
            if r < n:
                assert pieces[r] == 2
        if n > 1024:
            assert (pieces[1023], pieces[1024]) == (3, 2)
        if n > 4096:
            assert (pieces[4095], pieces[4096]) == (3, 2)
        assert pieces[n - 1] in (2, 3)
        tiny = [r for r in range(n) if pieces[r] == 0]
        assert len(tiny) >= n - 60 and set(pieces.values()) == {0, 1, 2, 3}
        # subsets: a block whose total is 0, only a block's last reference, only reference N - 1, everyone
        assert c.subsets["last_of_block0"] == (255,) and c.subsets["only_last"] == (n - 1,)
        assert c.subsets["everyone"] == tuple(range(n))
        assert sum(pieces[r] for r in c.subsets.get("block3", c.subsets.get("no_heavy_of_block0")) if r < 256) == 0


# ---- case 6 ------------------------------------------------------------------------------------------------------------------
def test_subset_words_on_both_sides_of_the_staging_limit():
    small, big = ec.cases_big()
    assert (small.n_refs, big.n_refs) == (393_216, 393_217)
    assert ec.mask_words(small.n_refs) == 12_288 == ec.LDS_WORDS and ec.mask_words(big.n_refs) == 12_296
    for c in (small, big):
        n = c.n_refs
        mir = c.mirror()
        used = mir.refs_with_records()
        assert 250 <= np.count_nonzero(mir.sizes) <= 320
        assert min(used) == 0 and max(used) == n - 1
        assert sum(1 for r in used if r >= n - 32) == 32                  # the last words of the bit row
        assert any(1000 <= r < n - 1000 for r in used)
        assert mir.list_lengths(n - 3) == [9, 10, 16, 17, 64, 65]          # the form table's highest reference under test
        holders_of_last = [h for h, _ in c.entries if n - 1 in h]
        assert any(h[0] < 24 for h in holders_of_last)                     # a hash held on both sides of the last word
        assert any(min(p) < 32 and max(p) >= n - 32 for p in c.subsets.values())
    assert 393_216 in big.subsets["last_alone"] and 393_216 >> 5 == 12_288  # the first word that is not staged


# ---- case 7 ------------------------------------------------------------------------------------------------------------------
def test_batch_blocks_put_the_planes_on_their_edges():
    for c in ec.batch_cases():
        pairs = ec.batch_pairs(c)
        mir = c.mirror()
        smp = ec.batch_samples(c)
        values, offsets = c.csr()
        ov = {k: oracle.overlap(values, offsets, s) for k, s in smp.items()}
        for r, o in pairs:
            shares = [oth for oth, _ in mir.inline_records.get(r, ())] + [tuple(x for x in h if x != r) for h, _ in mir.list_records.get(r, ())]
            assert any(o in s for s in shares)
            assert ov["r_only"][r] and not ov["r_only"][o] and ov["o_only"][o] and not ov["o_only"][r]
            assert ov["r_and_o"][r] and ov["r_and_o"][o] and ov["shared"][r] and ov["shared"][o]
        assert not ov["noise"].any() and not ov["empty"].any() and smp["noise"].size
        for b in ec.BATCH_B:
            labels = ec.batch_block(c, b)
            assert len(labels) == b
            want = {0: "shared", 63: "r_only", 64: "r_and_o", 127: "r_only", 128: "o_only", b - 1: "r_and_o"} if b > 1 else {0: "shared"}
            for pos, label in want.items():
                if pos < b:
                    assert labels[pos] == label
            assert all(x in ("empty", "noise") for i, x in enumerate(labels) if i not in want)
    assert ec.batch_pairs(ec.case_forms())[1][0] == 40 and 9 in ec.case_forms().mirror().list_lengths(40)      # the list form


# ---- the subsets and the two references ---------------------------------------------------------------------------------------
def _py_is_fast(case):
    return case.csr()[0].size <= 5000


@pytest.mark.parametrize("case", ec.all_cases(), ids=_ids(ec.all_cases()))
def test_samples_make_their_subsets_and_the_two_references_agree(case):
    values, offsets = case.csr()
    mir = case.mirror()
    smp = case.samples()
    threads = 8 if case.n_refs > 100_000 else 1
    n_py = 0
    for label, p in case.subsets.items():
        s = smp[f"P:{label}"]
        ov = oracle.overlap(values, offsets, s, threads=threads)
        assert ec.subset_of_mask(ov > 0) == p, label                           # the private-only sample makes exactly P
        assert np.array_equal(ov[list(p)], np.minimum(mir.sizes[list(p)], ec.N_PRIVATE))
        e, m = oracle.exclusive(values, offsets, ov > 0, s)
        assert np.array_equal(e, mir.n_excl(p)), label
        assert np.array_equal(m, ec.n_match_by_sets(case, p, s)), label
        if _py_is_fast(case) and n_py < 12:
            n_py += 1
            e2, m2 = oracle.exclusive_py(values, offsets, ov > 0, s)
            assert np.array_equal(e, e2) and np.array_equal(m, m2), label
    for label in ("shared", "noise"):
        ov = oracle.overlap(values, offsets, smp[label], threads=threads)
        p = ec.subset_of_mask(ov > 0)
        assert p == (tuple(mir.refs_with_records()) if label == "shared" else ())
        e, m = oracle.exclusive(values, offsets, ov > 0, smp[label])
        assert np.array_equal(e, mir.n_excl(p)) and np.array_equal(m, ec.n_match_by_sets(case, p, smp[label])), label
    n_py = 0
    for label, mask, sample_label in case.masks():
        p = ec.subset_of_mask(mask)
        e, m = oracle.exclusive(values, offsets, mask, smp[sample_label])
        assert np.array_equal(e, mir.n_excl(p)), label
        assert np.array_equal(m, ec.n_match_by_sets(case, p, smp[sample_label])), label
        if _py_is_fast(case) and n_py < 6:
            n_py += 1
            e2, m2 = oracle.exclusive_py(values, offsets, mask, smp[sample_label])
            assert np.array_equal(e, e2) and np.array_equal(m, m2), label
    assert any(len(ec.subset_of_mask(mask)) > len(case.subsets[label.split("+")[0]]) for label, mask, _ in case.masks() if "+" in label)
