"""No GPU: tests/order_cases.py alone satisfies the coverage its name promises.

For every case: the clean database is valid, the bad one is not, the two differ in at most two positions, the violation sits
where the site says, and what must stay equal between them does.  For every base: the geometry the kernels' constants imply
(which sort takes it, how many regions and tiles), the target sketches sit on the edges they are named for, and every site class
x kind the base's sizes allow is produced.  Run with -s to see the table of site classes x kinds per base.
"""
import collections

import numpy as np
import pytest

import order_cases as oc


def _last_elements(values, offsets):
    o = offsets.astype(np.int64)
    keep = o[1:] > o[:-1]
    return keep, values[o[1:][keep] - 1]


# ---- the reference ------------------------------------------------------------------------------------------------------------
def test_csr_is_valid_on_hand_made_arrays():
    u = lambda *x: np.array(x, np.uint64)
    assert oc.csr_is_valid(u(), u(0))
    assert oc.csr_is_valid(u(), u(0, 0, 0))
    assert oc.csr_is_valid(u(1, 2, 3), u(0, 3))
    assert oc.csr_is_valid(u(5, 1, 2, 9, 0), u(0, 1, 1, 4, 5))          # a descent across a boundary is none
    assert oc.csr_is_valid(u(0, 2 ** 64 - 1), u(0, 2))
    assert not oc.csr_is_valid(u(5, 4, 9), u(0, 3))
    assert not oc.csr_is_valid(u(4, 4), u(0, 2))                          # strictly
    assert not oc.csr_is_valid(u(1, 2, 3), u(0, 2))                       # does not end at len(values)
    assert not oc.csr_is_valid(u(1, 2, 3), u(1, 3))                       # does not start at 0
    assert not oc.csr_is_valid(u(1, 2, 3, 4), u(0, 3, 2, 4))              # not monotone
    assert not oc.csr_is_valid(u(1, 2, 3, 1), u(0, 2, 2, 4))              # the last sketch, behind an empty one
    assert oc.csr_is_valid(u(1, 2, 3, 1), u(0, 3, 3, 4))


def test_region_of_is_monotone_and_covers_every_region():
    for name in ("A", "C"):
        b = oc.base(name)
        p1, _ = oc.two_level_geometry(b.H)
        hs = np.sort(b.values)[::37]
        regs = [oc.region_of(int(h), b.H, b.max_hash) for h in hs]
        assert regs == sorted(regs) and set(regs) == set(range(p1))


# ---- the bases ----------------------------------------------------------------------------------------------------------------
def test_constants_are_the_kernels():
    """The numbers the layout is built on, as yh_sort.hip defines them (a changed constant moves the edges: re-lay the bases)."""
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "yacht_amd", "csrc", "yh_sort.hip")).read()
    for macro, want in (("YH_PART_TILE", oc.PART_TILE), ("YH_PART_THREADS", oc.PART_THREADS), ("YH_BKT_BITS", oc.BKT_SLOT_BITS),
                        ("YH_BKT_FILL8", oc.BKT_FILL * 8 // oc.BKT_SLOTS), ("YH_PC_BOUND_U", oc.PC_BOUND_U)):
        m = re.search(r"#define\s+%s\s+(\d+)" % macro, src)
        assert m and int(m.group(1)) == want, macro
    assert re.search(r"constexpr u32 SLOT_MAX = %d;" % oc.SLOT_MAX, src)
    assert re.search(r"constexpr u32 PART_MAX_BINS = %d;" % oc.PART_MAX_BINS, src)


def test_every_base_takes_the_path_it_is_built_for():
    a, b, c, d, r = (oc.base(n) for n in oc.BASES)
    # A: a little above three buckets' worth, below 10^4; the piece geometry takes it; two tiles and two regions without the pieces
    assert 3 * oc.BKT_FILL < a.H < 10 ** 4 and 100 <= a.n_refs <= 130
    assert a.max_hash < oc.MAX_HASH_SCALED_1000
    assert oc.pieces_geometry(a.H, a.max_hash, a.n_refs) == (1, 4)
    assert oc.two_level_geometry(a.H) == (2, 2) and oc.PART_TILE < a.H <= 3 * oc.PART_TILE
    # B: one bucket -- the distribution sort takes it, the pieces do not
    assert b.H <= oc.BKT_FILL and 35 <= b.n_refs <= 50
    assert oc.psort_applicable(b.H, b.max_hash) and oc.pieces_geometry(b.H, b.max_hash, b.n_refs) is None
    assert oc.two_level_geometry(b.H) == (1, 1)
    # C: A's shape, the largest hash 2^64 - 1: no pieces (and no fused records: both are switched on max_hash in the code)
    assert np.array_equal(c.offsets, a.offsets) and c.max_hash == oc.M64 and c.H > oc.PART_TILE
    assert oc.psort_applicable(c.H, c.max_hash) and oc.pieces_geometry(c.H, c.max_hash, c.n_refs) is None
    assert int(np.sort(c.values)[c.H // 2]) > 2 ** 62                      # (uniform over the 64 bits)
    # D: a key range too narrow for the fine slots
    assert 5500 < d.H < 6500 and d.max_hash < 8000 and not oc.psort_applicable(d.H, d.max_hash)
    # R: A's sketches and sites, and one slot with more pairs than the two-level sort ranks
    assert np.array_equal(r.values[:a.H], a.values) and np.array_equal(r.offsets[:a.n_refs + 1], a.offsets)
    assert r.H < 10 ** 4 and oc.psort_applicable(r.H, r.max_hash)
    vals, counts = np.unique(r.values, return_counts=True)
    assert int(counts.max()) == oc.N_REFUSED_HOLDERS > oc.SLOT_MAX and int(vals[counts.argmax()]) < r.max_hash
    for x in (a, b, c, d, r):
        assert oc.csr_is_valid(x.values, x.offsets)
        assert set(np.diff(x.offsets.astype(np.int64)).tolist()) <= set(oc.SIZES)
        assert np.unique(x.values).size < x.H                                # some hashes are shared: the oracle checks say something


@pytest.mark.parametrize("name", oc.BASES)
def test_targets_sit_on_the_edges_they_are_named_for(name):
    b = oc.base(name)
    o = b.offsets.astype(np.int64)
    size = np.diff(o)
    t = b.targets
    want = {"start0", "start63", "cross1024", "chunk_last", "chunk_first"} | ({"cross4096"} if b.H > 4096 + 64 else set())
    assert set(t) == want
    assert o[t["start0"]] % 64 == 0 and o[t["start63"]] % 64 == 63
    assert o[t["cross1024"]] < 1024 - 1 and o[t["cross1024"] + 1] > 1024 + 1
    if "cross4096" in t:
        assert o[t["cross4096"]] < 4096 - 1 and o[t["cross4096"] + 1] > 4096 + 1
        assert size[t["cross4096"]] == 1025                                # (q = 513 and a second 512-element round of loads)
    if name != "R":                                                        # (R keeps A's sketches; it is never uploaded in chunks)
        rb = oc.upload_chunks(b.offsets)
        assert len(rb) >= 3 and t["chunk_first"] in rb[1:-1] and t["chunk_last"] == t["chunk_first"] - 1
    for j in t.values():
        assert size[j] >= 63
        assert int(b.sketch(j)[-1]) < b.max_hash                           # the largest hash stays in another sketch
    # an empty and a one-hash sketch directly in front of a target and directly behind one
    assert {0, 1} <= {int(size[j - 1]) for j in t.values()} and {0, 1} <= {int(size[j + 1]) for j in t.values()}


# ---- the cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", oc.BASES)
def test_every_case_is_one_violation_at_its_site(name):
    b = oc.base(name)
    o = b.offsets.astype(np.int64)
    seen = set()
    for cname, cv, co, bv, bo, site in oc.all_cases(name):
        assert cname not in seen
        seen.add(cname)
        assert cv is b.values and co is b.offsets
        assert oc.csr_is_valid(cv, co), cname
        assert not oc.csr_is_valid(bv, bo), cname
        assert bv.size == cv.size and bo.size == co.size, cname                                   # H, N
        dv, do = np.flatnonzero(bv != cv), np.flatnonzero(bo != co)
        assert 1 <= dv.size + do.size <= 2, cname
        assert int(bo.max()) <= b.H, cname                                                          # every offset <= H
        tclass, qcl, kind, crosses = oc.site_info(site)
        if tclass == "offsets":
            assert dv.size == 0 and do.size == 1, cname
            if qcl == ["first"]:
                assert int(bo[0]) == 1 and oc.expected_error(cname) == "invalid_arg"
            else:
                j = int(do[0])
                assert 0 < j < b.n_refs and bo[j] > bo[j + 1] and np.all(np.diff(np.delete(bo.astype(np.int64), j)) >= 0), cname
                assert oc.expected_error(cname) == "unsorted"
            continue
        assert oc.expected_error(cname) == "unsorted"
        assert do.size == 0, cname                                                                  # every sketch size
        j = b.targets[tclass]
        start, size = int(o[j]), int(o[j + 1] - o[j])
        assert np.all((dv >= start) & (dv < start + size)), cname
        # exactly one descent (or tie) inside a sketch, and where it is
        tie = np.flatnonzero(~(bv[1:] > bv[:-1])) + 1
        first = np.zeros(b.H + 1, dtype=bool)
        first[o[:-1]] = True
        viol = [int(p) for p in tie if not first[p]]
        assert len(viol) == 1, (cname, viol)
        keep, clean_last = _last_elements(cv, co)
        _, bad_last = _last_elements(bv, bo)
        assert int(bad_last.max()) == int(clean_last.max()) == b.max_hash, cname                    # what k_ref_extents reports
        if qcl == ["above_max"]:
            assert kind is None and dv.size == 1 and int(bv[dv[0]]) == oc.M64 - 1 > b.max_hash and viol[0] == int(dv[0]) + 1, cname
            assert np.array_equal(bad_last, clean_last), cname
            continue
        q = viol[0] - start
        assert q in oc.q_classes(start, size) and oc.q_classes(start, size)[q] == qcl, (cname, q)
        gp = start + q
        for cl in qcl:
            if cl == "last":
                assert q == size - 1
            elif cl[0] == "q":
                assert q == int(cl[1:])
            else:
                assert gp % int(cl[1:]) == 0
        other = np.ones(clean_last.size, dtype=bool)
        other[int(np.count_nonzero(keep[:j]))] = "last" not in qcl          # every other sketch's last element; the target's own
        assert np.array_equal(bad_last[other], clean_last[other]), cname     # too, unless the violation is at it
        assert int(bv.max()) == int(cv.max()), cname                        # no hash above the largest one
        lo, hi = int(bv[gp - 1]), int(bv[gp])
        if kind == "swap":
            assert dv.tolist() == [gp - 1, gp] and (lo, hi) == (int(cv[gp]), int(cv[gp - 1])) and hi < lo
        elif kind == "equal":
            assert dv.tolist() == [gp] and lo == hi == int(cv[gp - 1])
        elif kind == "near":
            assert dv.tolist() == [gp] and hi == lo - 1
        else:
            assert kind == "far" and dv.tolist() == [gp] and hi == int(cv[start]) - 1 and lo - hi > 1
        if kind != "equal":
            assert crosses == (oc.region_of(lo, b.H, b.max_hash) != oc.region_of(hi, b.H, b.max_hash)), cname


@pytest.mark.parametrize("name", oc.BASES)
def test_every_site_class_and_kind_is_produced(name):
    """Per base: target class x q class x kind, for every q class the target's size and position allow; and descending steps that
    stay inside a first-level region as well as steps that cross one, wherever the two-level sort of the base has two regions."""
    b = oc.base(name)
    table = collections.defaultdict(set)
    crossing = collections.Counter()
    names = set()
    for cname, _, _, _, _, site in oc.all_cases(name):
        names.add(cname.split("/", 1)[1])
        tclass, qcl, kind, crosses = oc.site_info(site)
        if kind is None:
            continue
        for cl in qcl:
            table[(tclass, cl)].add(kind)
        if crosses is not None:
            crossing[(kind, crosses)] += 1
    o = b.offsets.astype(np.int64)
    for tclass, j in b.targets.items():
        start, size = int(o[j]), int(o[j + 1] - o[j])
        want = collections.defaultdict(set)      # q class -> kinds (`far` at q = 1 would be `near` again)
        for q, classes in oc.q_classes(start, size).items():
            for cl in classes:
                want[cl] |= set(oc.KINDS) - ({"far"} if q == 1 else set())
        assert {"q1", "last"} <= set(want) and {f"q{q}" for q in oc.Q_FIXED if q < size} <= set(want)
        got = {cl: kinds for (t, cl), kinds in table.items() if t == tclass}
        assert got == dict(want), (tclass, got, dict(want))
    all_q = {cl for (_, cl) in table}
    big = b.H > 4096 + 64
    assert all_q == {"q1", "q63", "q64", "q65", "q511", "q512", "last", "g64", "g1024"} | ({"q513", "g4096"} if big else set())
    assert {"offsets_nonmonotone", "offsets_first"} <= names
    assert ("above_max" in names) == (b.max_hash < oc.M64 - 1)
    p1, _ = oc.two_level_geometry(b.H)
    if p1 > 1:
        assert crossing[("near", False)] > 0 and crossing[("far", True)] > 0 and crossing[("swap", False)] > 0
        assert sum(n for (k, c), n in crossing.items() if c) >= 5
    else:
        assert not any(c for (_, c) in crossing)
    print(f"\nbase {name}: {len(oc.all_cases(name))} cases, H {b.H}, N {b.n_refs}, crossing steps {dict(crossing)}")
    for (tclass, cl), kinds in sorted(table.items()):
        print(f"  {tclass:<11} {cl:<6} {' '.join(sorted(kinds))}")
