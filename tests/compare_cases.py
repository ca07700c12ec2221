"""Seeded cases for yh_compare / yh_compare_device and their numpy oracle (tests/test_compare_cases_cpu.py checks that the
cases hold what they are named for; tests/test_gpu_compare.py runs them on the device).

A case is a dict: a / b lists of strictly ascending uint64 arrays (b None: the symmetric call), a_ab / b_ab None or lists of
uint32 arrays or None per sample, a_keep / b_keep likewise uint8, keep_and / keep_eq.  T is the sample tile and E the slice
capacity of the kernel; W the most windows the host cuts [0, the call's largest hash] into (window w of n starts at
w * ((largest >> log2 n) + 1): multiples of 2^64 / n when a sample holds 2^64 - 1).  The
host cuts one more window in two while the tiles are fewer than 1024 and an average cell (a sample of A plus one of B)
still has 4 E entries per window: that rule is restated in `windows_of` so that the cases can say which path they take.
"""
import functools

import numpy as np

from yacht_amd import _lib

T = _lib.YH_COMPARE_TILE
E = _lib.YH_COMPARE_SLICE
W = _lib.YH_COMPARE_MAX_WINDOWS
NARROW_BITS = 42  # lca_batch_cases.NARROW = 2^22: a hash range of 2^42, every top bit equal
U64_MAX = 2 ** 64 - 1
A_MAX = 2 ** 32 - 1


def windows_of(case) -> int:
    """How many windows the host cuts this call into (yh_compare.hip: compare_plan)."""
    a, b = case["a"], case["a"] if case["b"] is None else case["b"]
    if not a or not b:
        return 1
    ta, tb = (len(a) + T - 1) // T, (len(b) + T - 1) // T
    active = ta * (ta + 1) // 2 if case["b"] is None else ta * tb
    avg = sum(x.size for x in a) // len(a) + sum(x.size for x in b) // len(b)
    lg = 0
    while (1 << lg) < W and (active << lg) < 1024 and (avg >> (lg + 1)) >= 4 * E:
        lg += 1
    return 1 << lg


def _case(a, b=None, a_ab=None, b_ab=None, a_keep=None, b_keep=None, keep_and=0, keep_eq=0):
    u = lambda xs: None if xs is None else [np.ascontiguousarray(x, dtype=np.uint64) for x in xs]  # noqa: E731
    return dict(a=u(a), b=u(b), a_ab=a_ab, b_ab=b_ab, a_keep=a_keep, b_keep=b_keep, keep_and=keep_and, keep_eq=keep_eq)


def _pool(rng, n, bits=64):
    hi = U64_MAX if bits == 64 else (1 << bits) - 1
    return np.unique(rng.integers(0, hi, n, dtype=np.uint64, endpoint=True))


def _draw(rng, pool, n):
    return np.sort(rng.choice(pool, size=min(n, pool.size), replace=False))


def _abund(rng, xs, hi=50):
    return [rng.integers(1, hi, x.size).astype(np.uint32) for x in xs]


def _keep(rng, xs):
    return [rng.integers(0, 256, x.size).astype(np.uint8) for x in xs]


def build():
    cases = {}
    # ---- tile edges: n_a, n_b in {1, T-1, T, T+1, 2T+1}, rectangular and symmetric; small samples from one pool
    rng = np.random.default_rng(101)
    pool = _pool(rng, 120)
    sizes = (1, T - 1, T, T + 1, 2 * T + 1)
    for na in sizes:
        a = [_draw(rng, pool, int(rng.integers(10, 50))) for _ in range(na)]
        cases[f"tile_sym_{na}"] = _case(a, None, a_ab=_abund(rng, a))
        for nb in sizes:
            b = [_draw(rng, pool, int(rng.integers(10, 50))) for _ in range(nb)]
            cases[f"tile_rect_{na}x{nb}"] = _case(a, b, a_ab=_abund(rng, a), b_ab=_abund(rng, b))
    # ---- lengths 0, 1, E-1, E, E+1, several slices; an empty sample first, in the middle and last
    rng = np.random.default_rng(102)
    pool = _pool(rng, 4000)
    lens = (0, 1, E - 1, 0, E, E + 1, 3 * E + 5, 0)
    a = [_draw(rng, pool, n) for n in lens]
    b = [_draw(rng, pool, n) for n in lens[::-1]]
    cases["lengths_rect"] = _case(a, b, a_ab=_abund(rng, a), b_ab=_abund(rng, b))
    cases["lengths_sym"] = _case(a, None, a_ab=_abund(rng, a))
    cases["all_empty"] = _case([np.zeros(0, np.uint64)] * 3, [np.zeros(0, np.uint64)] * 2)
    # ---- several windows: the host cuts the hash space (4 windows for 2 x 2 samples of 3 000, 8 for one pair of 5 000,
    # W = 64 for one pair of 33 000: the one case that is larger than a few thousand hashes, because no smaller one takes
    # the top six bits)
    rng = np.random.default_rng(103)
    pool = _pool(rng, 6000)
    a, b = [_draw(rng, pool, 3000) for _ in range(2)], [_draw(rng, pool, 3000) for _ in range(2)]
    cases["windows_4_rect"] = _case(a, b, a_ab=_abund(rng, a), b_ab=_abund(rng, b))
    cases["windows_4_sym"] = _case(a, None, a_ab=_abund(rng, a))
    a, b = [_draw(rng, pool, 5000)], [_draw(rng, pool, 5000)]
    cases["windows_8"] = _case(a, b, a_ab=_abund(rng, a), b_ab=_abund(rng, b))
    big = _pool(rng, 50000)
    a, b = [_draw(rng, big, 33000)], [_draw(rng, big, 33000)]
    cases["windows_64"] = _case(a, b, a_ab=_abund(rng, a), b_ab=_abund(rng, b))
    # ---- set relations
    rng = np.random.default_rng(104)
    pool = _pool(rng, 3000)
    x = _draw(rng, pool, 700)
    sub = x[rng.random(x.size) < 0.4]
    dis = np.setdiff1d(_draw(rng, pool, 900), x)
    inner = np.setdiff1d(pool, x)
    inner = inner[(inner > x[0]) & (inner < x[-1])]
    ends = np.concatenate([[x[0]], _draw(rng, inner, 400), [x[-1]]])  # shares exactly x's first and last hash with x
    a, b = [x, sub, dis, ends], [x, sub, dis, ends]
    cases["relations"] = _case(a, [s.copy() for s in b], a_ab=_abund(rng, a), b_ab=_abund(rng, b))
    # ---- window edges
    rng = np.random.default_rng(105)
    lo_run = np.arange(0, 1000, dtype=np.uint64)
    hi_run = np.uint64(U64_MAX - 999) + np.arange(1000, dtype=np.uint64)  # ends at 2^64 - 1
    a = [lo_run, hi_run, np.array([0, 5, U64_MAX], dtype=np.uint64)]
    b = [np.arange(500, 1500, dtype=np.uint64), hi_run[300:], np.array([0, U64_MAX], dtype=np.uint64), np.array([5], dtype=np.uint64)]
    cases["consecutive_and_extremes"] = _case(a, b, a_ab=_abund(rng, a), b_ab=_abund(rng, b))
    edges = np.array(sorted({(k << 58) - d for k in range(1, W) for d in (0, 1)} | {0, U64_MAX}), dtype=np.uint64)
    pool = _pool(rng, 7000)
    a = [np.union1d(_draw(rng, pool, 3000), e) for e in (edges, edges[rng.random(edges.size) < 0.6])]
    b = [np.union1d(_draw(rng, pool, 3000), e) for e in (edges, edges[rng.random(edges.size) < 0.6])]
    cases["window_boundaries_4"] = _case(a, b, a_ab=_abund(rng, a), b_ab=_abund(rng, b))
    a, b = [np.union1d(_draw(rng, pool, 5000), edges)], [np.union1d(_draw(rng, pool, 5000), np.append(edges[::2], edges[-1]))]
    cases["window_boundaries_8"] = _case(a, b, a_ab=_abund(rng, a), b_ab=_abund(rng, b))
    narrow = _pool(rng, 6000, NARROW_BITS)
    n_edges = np.array(sorted({(k << 40) - d for k in range(1, 4) for d in (0, 1)} | {(1 << NARROW_BITS) - 1}), dtype=np.uint64)
    a = [np.union1d(_draw(rng, narrow, 3000), n_edges) for _ in range(2)]
    b = [np.union1d(_draw(rng, narrow, 3000), n_edges) for _ in range(2)]
    cases["narrow_range"] = _case(a, b, a_ab=_abund(rng, a), b_ab=_abund(rng, b))
    # one long clustered sample beside short uniform ones in the same tile: the rounds are bounded by the long one
    a = [np.arange(1 << 40, (1 << 40) + 2000, dtype=np.uint64), _draw(rng, pool, 300), _draw(rng, pool, 10)]
    b = [np.arange((1 << 40) + 1000, (1 << 40) + 2500, 3, dtype=np.uint64), _draw(rng, pool, 600)]
    cases["clustered_beside_uniform"] = _case(a, b, a_ab=_abund(rng, a), b_ab=_abund(rng, b))
    # ---- abundances: none on A, on B, on both; 2^32 - 1 on three shared hashes; ones everywhere
    rng = np.random.default_rng(106)
    pool = _pool(rng, 1500)
    a, b = [_draw(rng, pool, 600) for _ in range(3)], [_draw(rng, pool, 500) for _ in range(2)]
    ab_a, ab_b = _abund(rng, a, 1000), _abund(rng, b, 1000)
    cases["abund_both"] = _case(a, b, a_ab=ab_a, b_ab=ab_b)
    cases["abund_a_only"] = _case(a, b, a_ab=ab_a)
    cases["abund_b_only"] = _case(a, b, b_ab=ab_b)
    cases["abund_none"] = _case(a, b)
    cases["abund_ones"] = _case(a, b, a_ab=[np.ones(x.size, np.uint32) for x in a], b_ab=[np.ones(x.size, np.uint32) for x in b])
    cases["abund_mixed_per_sample"] = _case(a, b, a_ab=[ab_a[0], None, ab_a[2]], b_ab=[None, ab_b[1]])
    shared = np.intersect1d(a[0], b[0])[:3]
    big_a, big_b = [x.copy() for x in ab_a], [x.copy() for x in ab_b]
    big_a[0][np.isin(a[0], shared)] = A_MAX
    big_b[0][np.isin(b[0], shared)] = A_MAX
    cases["abund_max_on_three"] = _case(a, b, a_ab=big_a, b_ab=big_b)
    cases["abund_max_sym"] = _case(a, None, a_ab=[np.full(x.size, A_MAX, np.uint32) for x in a])
    # ---- keep bytes
    rng = np.random.default_rng(107)
    ka, kb = _keep(rng, a), _keep(rng, b)
    for name, (k_and, k_eq) in {"set0": (1, 0), "set3": (8, 0), "known": (0x80, 0x80), "known_not_set0": (0x81, 0x80)}.items():
        cases[f"keep_{name}"] = _case(a, b, a_ab=ab_a, b_ab=ab_b, a_keep=ka, b_keep=kb, keep_and=k_and, keep_eq=k_eq)
    cases["keep_nothing"] = _case(a, b, a_ab=ab_a, b_ab=ab_b, a_keep=ka, b_keep=kb, keep_and=0, keep_eq=1)
    cases["keep_a_only"] = _case(a, b, a_ab=ab_a, b_ab=ab_b, a_keep=ka, keep_and=1, keep_eq=0)
    cases["keep_b_only"] = _case(a, b, a_ab=ab_a, b_ab=ab_b, b_keep=kb, keep_and=0x80, keep_eq=0x80)
    cases["keep_sym"] = _case(a, None, a_ab=ab_a, a_keep=ka, keep_and=2, keep_eq=0)
    # the same hashes on both sides, kept on A and dropped on B, hash by hash in turn: nothing is shared
    x = _draw(rng, pool, 400)
    alt = (np.arange(x.size) % 2).astype(np.uint8)
    cases["keep_a_kept_b_dropped"] = _case([x], [x.copy()], a_keep=[alt], b_keep=[1 - alt], keep_and=1, keep_eq=0)
    # ---- a full panel at small size: 2T + 3 samples of 20 to 60 hashes from a common pool
    rng = np.random.default_rng(108)
    pool = _pool(rng, 150)
    a = [_draw(rng, pool, int(rng.integers(20, 61))) for _ in range(2 * T + 3)]
    cases["panel_sym"] = _case(a, None, a_ab=_abund(rng, a))
    return cases


CASES = build()


def _kept(x, ab, keep, k_and, k_eq):
    ab = np.ones(x.size, dtype=np.uint64) if ab is None else np.asarray(ab, dtype=np.uint64)
    if keep is None:
        return x, ab
    m = (np.asarray(keep, dtype=np.uint8) & np.uint8(k_and)) == np.uint8(k_eq)
    return x[m], ab[m]


def _side(xs, abs_, keeps, k_and, k_eq):
    return [_kept(x, None if abs_ is None else abs_[s], None if keeps is None else keeps[s], k_and, k_eq) for s, x in enumerate(xs)]


def oracle(case):
    """(cells [n_a][n_b] of (n_shared, sum_min, dot), self_a, self_b of (n_kept, sum, sq)) as Python ints:
    np.intersect1d(..., return_indices=True) for the shared hashes, Python ints for the sums."""
    k_and, k_eq = case["keep_and"], case["keep_eq"]
    sa = _side(case["a"], case["a_ab"], case["a_keep"], k_and, k_eq)
    sb = sa if case["b"] is None else _side(case["b"], case["b_ab"], case["b_keep"], k_and, k_eq)
    cells = []
    for xa, aa in sa:
        row = []
        for xb, bb in sb:
            _, ia, ib = np.intersect1d(xa, xb, assume_unique=True, return_indices=True)
            u, v = [int(t) for t in aa[ia]], [int(t) for t in bb[ib]]
            row.append((len(u), sum(min(p, q) for p, q in zip(u, v)), sum(p * q for p, q in zip(u, v))))
        cells.append(row)
    selves = [[(int(x.size), sum(int(t) for t in ab), sum(int(t) * int(t) for t in ab)) for x, ab in side] for side in (sa, sb)]
    return cells, selves[0], selves[1]


@functools.lru_cache(maxsize=None)
def expected(name):
    """The oracle's answer as the arrays yh_compare writes (compare.CELL_DTYPE / SELF_DTYPE), computed once per case."""
    from yacht_amd import compare

    cells, self_a, self_b = oracle(CASES[name])
    mask = (1 << 64) - 1
    c = np.zeros((len(self_a), len(self_b)), dtype=compare.CELL_DTYPE)
    for i, row in enumerate(cells):
        for j, (n, mn, dot) in enumerate(row):
            c[i, j] = (n, mn, dot & mask, dot >> 64)
    s = [np.array([(n, sm, sq & mask, sq >> 64) for n, sm, sq in side], dtype=compare.SELF_DTYPE).reshape(len(side)) for side in (self_a, self_b)]
    for arr in (c, *s):
        arr.setflags(write=False)
    return c, s[0], s[1]
