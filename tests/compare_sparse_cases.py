"""Seeded cases for the sparse route of the compare pass (yh_compare_sparse_device, yh_compare_routed) and a plain
numpy / Python-int oracle for the figures it reports (tests/test_compare_sparse_cases_cpu.py checks that the cases hold what
they are named for; tests/test_gpu_compare_sparse.py runs them on the device).  The cells' oracle is compare_cases.oracle.

A case is a dict as in compare_cases.py, with two more keys: "ld_extra" (columns behind n_b of the cells buffer, which must
stay untouched) and "closed_form" (the expected cell when every cell is the same and the general oracle would take minutes).
R is the longest run the flattened kernel takes, K the chunk of sorted records a workgroup of the runs kernel takes, T8 the
dense tile.  These are the smallest shapes at which the pass can go wrong: runs at R - 1, R, R + 1, runs on and across the
chunk edges, hashes at the ends of the range, dropped entries inside runs, and the carry of the product sum.
"""
import functools

import numpy as np
from compare_cases import A_MAX, NARROW_BITS, U64_MAX, _abund, _case, _draw, _keep, _pool
from compare_cases import oracle as cells_oracle

from yacht_amd import _lib

R = _lib.YH_COMPARE_RUN_SMALL
K = _lib.YH_COMPARE_SPARSE_CHUNK
T8 = _lib.YH_COMPARE_TILE
LOG2 = _lib.YH_COMPARE_SAMPLE_LOG2


def _sets(n, shared, private):
    """n samples: shared = [(hash, holders)], private = per sample an array; returns the sorted samples."""
    out = []
    for s in range(n):
        mine = [h for h, holders in shared if s in holders]
        out.append(np.unique(np.concatenate([np.asarray(private[s], dtype=np.uint64), np.asarray(mine, dtype=np.uint64)])))
    return out


def _privates(rng, n, lo=5, hi=20):
    """Disjoint private hashes per sample: multiples of n plus the sample's number, so no two samples share one."""
    return [(np.unique(rng.integers(0, 1 << 40, size=int(rng.integers(lo, hi)))).astype(np.uint64) * np.uint64(n + 1) + np.uint64(s)) << np.uint64(8)
            for s in range(n)]


def _shared_hash(rng):
    return (int(rng.integers(1, 1 << 40)) << 8) | 0x55  # (private hashes end in 0x00: never equal to one of them)


def _chunk_case(mults, n=6):
    """A symmetric case whose sorted records have the given run lengths in order: hash number r (ascending) is held by
    mults[r] samples.  Singletons go round the samples in turn, a run of c to the c samples after the turn."""
    samples = [[] for _ in range(n)]
    turn = 0
    for r, c in enumerate(mults):
        h = (r + 1) * 1000
        for d in range(c):
            samples[(turn + d) % n].append(h)
        turn += 1
    return _case([np.array(s, dtype=np.uint64) for s in samples], None)


def build():
    cases = {}
    # ---- no pairs
    rng = np.random.default_rng(201)
    priv = _privates(rng, 5)
    a = _sets(5, [], priv)
    cases["no_shared"] = _case(a, None, a_ab=_abund(rng, a))
    cases["all_empty_sym"] = _case([np.zeros(0, np.uint64)] * 3, None)
    cases["n_a_zero"] = _case([], [a[0], a[1]])
    h = _shared_hash(rng)
    b = _sets(5, [(h, {0, 1, 3, 4})], priv)
    b[2] = np.zeros(0, np.uint64)
    cases["one_empty_among_full"] = _case(b, None, a_ab=_abund(rng, b))
    # ---- run lengths, symmetric: one hash with exactly c holders among private hashes and a few two-holder runs
    rng = np.random.default_rng(202)
    n = R + 2
    for c in (2, R - 1, R, R + 1):
        priv = _privates(rng, n)
        holders = set(int(x) for x in rng.choice(n, size=c, replace=False))
        shared = [(_shared_hash(rng), holders)] + [(_shared_hash(rng), {int(x) for x in rng.choice(n, size=2, replace=False)}) for _ in range(4)]
        a = _sets(n, shared, priv)
        cases[f"run_sym_{c}"] = _case(a, None, a_ab=_abund(rng, a))
    n = 2 * T8 + 1
    a = _sets(n, [(_shared_hash(rng), set(range(n)))], _privates(rng, n))
    cases["run_sym_all"] = _case(a, None, a_ab=_abund(rng, a))
    # n_a = n_b = 2 048 distinct sides, each sample {one common hash, one private}: one run of 4 096, every cell (1, 1, 1, 0)
    m = _lib.YH_COMPARE_MAX_SAMPLES
    common = 1 << 50
    a = [np.array(sorted((common, 2 * s + 1)), dtype=np.uint64) for s in range(m)]
    b = [np.array(sorted((common, (1 << 51) + 2 * s)), dtype=np.uint64) for s in range(m)]
    cases["run_4096"] = dict(_case(a, b), closed_form=((1, 1, 1, 0), (2, 2, 2, 0)))
    # ---- rectangular
    rng = np.random.default_rng(203)
    na, nb = 3, R + 3
    pa, pb = _privates(rng, na + nb)[:na], _privates(rng, na + nb)[na:]
    h1, h2 = _shared_hash(rng), _shared_hash(rng)
    a = _sets(na, [(h1, {1})], pa)
    b = _sets(nb, [(h1, set(range(R + 1))), (h2, set(range(1, R + 3)))], pb)  # h2: c_a = 0, c_b = R + 2: a long run, no pair
    cases["rect_1_by_R1_and_ca0"] = _case(a, b, a_ab=_abund(rng, a), b_ab=_abund(rng, b))
    pool = _pool(rng, 200)
    a = [_draw(rng, pool, int(rng.integers(20, 80))) for _ in range(T8 + 2)]
    ab = _abund(rng, a)
    cases["rect_same_as_sym"] = _case(a, [x.copy() for x in a], a_ab=ab, b_ab=[x.copy() for x in ab])
    cases["rect_same_as_sym_ref"] = _case(a, None, a_ab=ab)
    a = [_draw(rng, pool, int(rng.integers(20, 80))) for _ in range(T8 + 1)]
    b = [_draw(rng, pool, int(rng.integers(20, 80))) for _ in range(T8 - 1)]
    cases["rect_ld"] = dict(_case(a, b, a_ab=_abund(rng, a), b_ab=_abund(rng, b)), ld_extra=3)
    # ---- chunk edges: more than 2 K records; the run lengths are given in sorted order
    ones = lambda k: [1] * k  # noqa: E731
    cases["chunk_first_is_last_of_0"] = _chunk_case(ones(K - 1) + [3] + ones(K + 10))           # run at records K-1 .. K+1
    cases["chunk_last_is_first_of_1"] = _chunk_case(ones(K - 2) + [3] + ones(K + 10))           # run at records K-2 .. K
    cases["chunk_straddles_1_2"] = _chunk_case(ones(2 * K - 2) + [5] + ones(10))                # run at records 2K-2 .. 2K+2
    cases["chunk_twos_both_sides"] = _chunk_case(ones(K - 2) + [2, 2] + ones(K - 4) + [2, 2] + ones(10))  # K-2..K-1, K..K+1, 2K-2.., 2K..
    # ---- hash range
    rng = np.random.default_rng(204)
    pool = _pool(rng, 300)
    ext = np.array([0, U64_MAX], dtype=np.uint64)
    a = [np.union1d(_draw(rng, pool, 60), e) for e in (ext, ext[:1], ext[1:], ext)]
    cases["extremes_64"] = _case(a, None, a_ab=_abund(rng, a))
    narrow = _pool(rng, 400, NARROW_BITS)
    top = np.array([(1 << NARROW_BITS) - 1], dtype=np.uint64)
    a = [np.union1d(_draw(rng, narrow, 150), top) for _ in range(3)] + [_draw(rng, narrow, 150)]
    b = [np.union1d(_draw(rng, narrow, 150), top) for _ in range(2)]
    cases["narrow_42"] = dict(_case(a, b, a_ab=_abund(rng, a), b_ab=_abund(rng, b)), bits=NARROW_BITS)
    tiny = np.arange(1 << LOG2, dtype=np.uint64)
    a = [np.sort(rng.choice(tiny, size=int(rng.integers(5, 40)), replace=False)) for _ in range(5)]
    cases["tiny_bits"] = _case(a, None, a_ab=_abund(rng, a))
    # ---- keep bytes
    rng = np.random.default_rng(205)
    pool = _pool(rng, 250)
    a = [_draw(rng, pool, int(rng.integers(40, 120))) for _ in range(7)]
    b = [_draw(rng, pool, int(rng.integers(40, 120))) for _ in range(4)]
    ab_a, ab_b, ka, kb = _abund(rng, a), _abund(rng, b), _keep(rng, a), _keep(rng, b)
    x = _draw(rng, pool, 100)
    alt = (np.arange(x.size) % 2).astype(np.uint8)
    cases["keep_kept_in_a_dropped_in_b"] = _case([x], [x.copy()], a_keep=[alt], b_keep=[1 - alt], keep_and=1, keep_eq=0)
    n = 6
    h = _shared_hash(rng)
    s6 = _sets(n, [(h, set(range(n)))], _privates(rng, n))
    k6 = [np.zeros(s.size, np.uint8) for s in s6]
    for s in (1, 3):
        k6[s][s6[s] == np.uint64(h)] = 1  # dropped entries between kept ones inside the run of h
    cases["keep_dropped_inside_run"] = _case(s6, None, a_ab=_abund(rng, s6), a_keep=k6, keep_and=1, keep_eq=0)
    cases["keep_none_kept"] = _case(a, b, a_ab=ab_a, b_ab=ab_b, a_keep=ka, b_keep=kb, keep_and=0, keep_eq=1)
    cases["keep_mask_known"] = _case(a, b, a_ab=ab_a, b_ab=ab_b, a_keep=ka, b_keep=kb, keep_and=0x80, keep_eq=0x80)
    cases["keep_mask_set0"] = _case(a, b, a_ab=ab_a, b_ab=ab_b, a_keep=ka, b_keep=kb, keep_and=1, keep_eq=0)
    cases["keep_mask_set0_sym"] = _case(a, None, a_ab=ab_a, a_keep=ka, keep_and=1, keep_eq=0)
    cases["keep_on_b_only"] = _case(a, b, a_ab=ab_a, b_ab=ab_b, b_keep=kb, keep_and=1, keep_eq=0)
    # ---- sums
    rng = np.random.default_rng(206)
    a = [_draw(rng, pool, 120) for _ in range(3)]
    big = _abund(rng, a, 1000)
    three = np.intersect1d(a[0], a[2])[:3]
    assert three.size == 3
    big[0][np.isin(a[0], three)] = A_MAX
    big[2][np.isin(a[2], three)] = A_MAX
    cases["dot_carry_sym"] = _case(a, None, a_ab=big)
    cases["dot_carry_rect"] = _case(a[:1], a[1:], a_ab=big[:1], b_ab=big[1:])
    cases["abund_on_a_only"] = _case(a, b, a_ab=_abund(rng, a))
    cases["abund_none_rect"] = _case(a, b)
    cases["abund_none_sym"] = _case(a, None)
    return cases


CASES = build()


def hash_bits(case) -> int:
    """What the host form derives: the bits of the call's largest hash, at least 1 (a case may promise its own: "bits")."""
    sides = case["a"] if case["b"] is None else list(case["a"]) + list(case["b"])
    top = max((int(x[-1]) for x in sides if x.size), default=0)
    return max(1, top.bit_length())


def _kept_hashes(xs, keeps, k_and, k_eq):
    out = []
    for s, x in enumerate(xs):
        k = None if keeps is None else keeps[s]
        out.append(x if k is None else x[(np.asarray(k, dtype=np.uint8) & np.uint8(k_and)) == np.uint8(k_eq)])
    return out


def figures(case, bits=None):
    """dict(n_entries, n_shared_hashes, n_pair_updates, longest_run, pairs_sampled, dense_steps) as Python ints, by counting
    holders per hash: a hash held by c kept entries gives c (c - 1) / 2 pairs in the symmetric call, c_a * c_b in the
    rectangular one; pairs_sampled counts the hashes below 2^(bits - LOG2) only (all of them when bits <= LOG2)."""
    bits = hash_bits(case) if bits is None else bits
    sym = case["b"] is None
    ka = _kept_hashes(case["a"], case["a_keep"], case["keep_and"], case["keep_eq"])
    kb = [] if sym else _kept_hashes(case["b"], case["b_keep"], case["keep_and"], case["keep_eq"])
    count = {}
    for side, xs in enumerate((ka, kb)):
        for x in xs:
            for h in x.tolist():
                c = count.setdefault(h, [0, 0])
                c[side] += 1
    window = None if bits <= LOG2 else 1 << (bits - LOG2)
    n_a, n_b = len(case["a"]), len(case["a"] if sym else case["b"])
    out = dict(n_entries=sum(x.size for x in ka) + sum(x.size for x in kb), n_shared_hashes=0, n_pair_updates=0, longest_run=0, pairs_sampled=0)
    if n_a == 0 or n_b == 0:
        out["n_entries"] = 0  # (no cells: nothing is grouped)
        count = {}
    for h, (ca, cb) in count.items():
        pairs = ca * (ca - 1) // 2 if sym else ca * cb
        if pairs:
            out["n_shared_hashes"] += 1
            out["n_pair_updates"] += pairs
            out["longest_run"] = max(out["longest_run"], ca + cb)
            if window is None or h < window:
                out["pairs_sampled"] += pairs
    total_a = sum(x.size for x in case["a"])
    total_b = total_a if sym else sum(x.size for x in case["b"])
    out["dense_steps"] = (n_a + 1) * total_a if sym else n_b * total_a + n_a * total_b
    return out


def sorted_records(case):
    """The hashes of a symmetric case without keep bytes as the sort leaves them: what the chunk cases are laid out in."""
    assert case["b"] is None and case["a_keep"] is None
    return np.sort(np.concatenate(case["a"]))


@functools.lru_cache(maxsize=None)
def expected(name):
    """As compare_cases.expected, for these cases; a closed-form case is built from its one cell and one self row."""
    from yacht_amd import compare

    case = CASES[name]
    if case.get("closed_form"):
        cell, row = case["closed_form"]
        c = np.zeros((len(case["a"]), len(case["b"])), dtype=compare.CELL_DTYPE)
        c[...] = cell
        s = [np.zeros(len(side), dtype=compare.SELF_DTYPE) for side in (case["a"], case["b"])]
        for x in s:
            x[...] = row
    else:
        cells, self_a, self_b = cells_oracle(case)
        mask = (1 << 64) - 1
        c = np.zeros((len(self_a), len(self_b)), dtype=compare.CELL_DTYPE)
        for i, row in enumerate(cells):
            for j, (n, mn, dot) in enumerate(row):
                c[i, j] = (n, mn, dot & mask, dot >> 64)
        s = [np.array([(n, sm, sq & mask, sq >> 64) for n, sm, sq in side], dtype=compare.SELF_DTYPE).reshape(len(side)) for side in (self_a, self_b)]
    for arr in (c, *s):
        arr.setflags(write=False)
    return c, s[0], s[1]
