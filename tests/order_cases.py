"""Reference databases that break "every sketch strictly ascending" in exactly one place, numpy only.

Never calls the library.  Every query kernel assumes ascending sketches, and the build checks that assumption in whichever pass
reads the pairs anyway ("Where the sketch order is checked"): the bounds pass of the piece distribution, the first
level of the two-level sort, or a pass of its own.  Each of those carries the element in front of a lane across some edge -- a
wave of 64, a 512-element round of loads, an item of 1 024 pairs, a tile of 4 096 -- and a check that loses the carry at one
of them misses exactly the violations that sit there.  So the bases below are laid out so that sketches START and CONTINUE
across those edges, and every bad database differs from its clean base by one violation at a named site.

Kernel constants this layout relies on (tests/test_order_cases_cpu.py asserts the geometry that follows from them):
    WAVE 64            lanes; k_part's first lane of a wave reads its predecessor with a scalar load, k_piece_bounds hands
                       carry_h / have from load to load
    PC_BOUND_U 8       64-element loads a wave of k_piece_bounds has in flight: a round is 512 elements of ONE sketch
    PART_THREADS 1024  an item of k_part: element i of a tile belongs to item i / 1 024
    PART_TILE 4096     pairs per workgroup of k_part
    BKT_FILL 2560      pairs per bucket the sorts aim at: ceil(H / 2 560) buckets decide which distribution takes a database
    BKT_SLOTS 4096     fine slots per bucket: a key range narrower than 4 096 values per bucket is not the distribution sort's
    SLOT_MAX 1024      pairs of one slot the two-level sort ranks: one hash in more sketches than that and it REFUSES the keys

Bases (sizes drawn from {0, 1, 2, 63, 64, 65, 512, 513, 1025}):
    A   ~120 sketches, H a little above 3 x 2 560, hashes uniform below max_hash_for_scaled(1000): four buckets, the piece
        geometry (P1 1 x P2 4); two-level when the pieces are switched off (P1 2 x P2 2, two tiles).
    B   ~45 sketches, H <= 2 560: one bucket -- two-level without a switch, one tile.
    C   A's shape over the full 64 bits, one sketch ending in 2^64 - 1: pieces and fused records are off in the code.
    D   H ~6 300, every hash below 8 000: not the distribution sort's keys (radix sort, the ordering check as its own pass).
    R   A followed by 1 100 one-hash sketches that all hold the same hash: 1 100 pairs in one slot, more than SLOT_MAX, so the
        two-level sort refuses the keys on the device (A's own ~120 sketches could never crowd a slot).

Targets (sketches of at least 63 hashes, an empty and a one-hash sketch directly before and after most of them):
    start0      starts at a global position p with p % 64 == 0
    start63     starts at p % 64 == 63
    cross1024   holds global position 1 024 in its interior
    cross4096   holds global position 4 096 in its interior (A, C, D, R)
    chunk_last / chunk_first   the sketches on either side of a boundary of the chunked upload (shares 0.4, 0.3, 0.2, 0.1)

A violation sits between elements q - 1 and q of the target.  q classes: q1, q63, q64, q65, q511, q512, q513, last (q = size -
1), and g64 / g1024 / g4096: the q that puts element q at a global position that is a multiple of 64 / 1 024 / 4 096.  Kinds:
    swap        the neighbours exchanged
    equal       element q := element q - 1            ("strictly"; at q = last this is the issue's kind (d))
    near        element q := element q - 1 minus 1    (a step of one: stays in its first-level region)
    far         element q := element 0 minus 1        (a step across most of the sketch: crosses regions where there are any)
Whether a descending step crosses a first-level region is COMPUTED, with the build's own multiply-shift (region_of), and
reported as `crosses`; the CPU test asserts that both occur on every base that has more than one region.

Kept equal between clean and bad: H, N, every sketch's size, the largest last element (what k_ref_extents reports as the
largest hash), and every sketch's last element except the target's own at q = last.  The one named exception is `above_max`:
an interior element := 2^64 - 2, above the largest last element, every last element untouched -- the extents pass then
reports a largest hash that the data exceeds.  Offsets cases: one offset raised above its successor (`offsets_nonmonotone`,
every offset <= H) and offsets[0] = 1 (`offsets_first`: YH_ERR_INVALID_ARG, everything else YH_ERR_UNSORTED).
"""
import functools
import math

import numpy as np

WAVE = 64
PC_BOUND_U = 8
PART_THREADS = 1024
PART_TILE = 4096
BKT_FILL = 2560
BKT_SLOTS = 4096
BKT_SLOT_BITS = 12
PART_MAX_BINS = 1024
SLOT_MAX = 1024
UPLOAD_SHARES = (0.4, 0.3, 0.2, 0.1)
M64 = (1 << 64) - 1
MAX_HASH_SCALED_1000 = (2 ** 64 + 500) // 1000
SIZES = (0, 1, 2, 63, 64, 65, 512, 513, 1025)
Q_FIXED = (1, 63, 64, 65, 511, 512, 513)
G_EDGES = (64, 1024, 4096)
KINDS = ("swap", "equal", "near", "far")
BASES = ("A", "B", "C", "D", "R")
N_REFUSED_HOLDERS = 1100

# (size, role): role "" = filler, "crown" = the sketch that keeps the database's largest hash, anything else = a target class
_TAIL = [(2, ""), (1, ""), (0, "")] * 25
_LAYOUT_A = (
    [(63, ""), (1, ""), (0, ""), (513, "start0"), (0, ""), (1, ""),                      # 64 .. 577 | 578
     (65, ""), (64, ""), (63, ""), (2, ""), (513, "cross1024"), (0, "")]                 # 772 .. 1285
    + [(63, "")] * 7 + [(1, ""), (65, "start63"), (1, ""), (0, ""),                       # 1727 .. 1792 | 1793
       (1025, ""), (512, ""), (513, ""), (64, ""), (65, ""), (2, ""), (0, ""), (1, ""),   # 3975
       (1025, "cross4096"), (1, ""), (0, "")]                                             # 3975 .. 5000 | 5001
)
_LAYOUT = {
    "A": _LAYOUT_A + [(1025, ""), (513, ""), (512, ""), (512, "crown"), (65, ""), (64, ""), (63, "")] + _TAIL,
    "D": _LAYOUT_A + [(513, ""), (512, "crown"), (65, ""), (64, ""), (63, "")] + _TAIL,
    "B": [(63, ""), (1, ""), (0, ""), (513, "start0"), (0, ""), (1, ""), (65, ""), (64, "crown"), (63, ""), (2, ""),
          (513, "cross1024"), (0, "")] + [(63, "")] * 7 + [(1, ""), (65, "start63"), (1, ""), (0, "")] + _TAIL[:24],
}
_LAYOUT["C"] = _LAYOUT["A"]


def csr_is_valid(values, offsets):
    """offsets start at 0, never decrease and end at len(values); every slice is strictly ascending."""
    values = np.asarray(values, dtype=np.uint64)
    offsets = np.asarray(offsets, dtype=np.uint64)
    if offsets.ndim != 1 or offsets.size < 1 or int(offsets[0]) != 0 or int(offsets[-1]) != values.size:
        return False
    o = offsets.astype(np.int64)
    if np.any(o[1:] < o[:-1]):
        return False
    if values.size < 2:
        return True
    rising = values[1:] > values[:-1]
    first = np.zeros(values.size, dtype=bool)   # first[p]: position p opens a sketch (no neighbour in front to compare with)
    first[o[:-1][o[:-1] < values.size]] = True
    return bool(np.all(rising | first[1:]))


# ---- the build's geometry (yh_sort.hip: yh_psort_applicable, yh_psort_begin, pc_geometry) ----------------------------------
def n_buckets(H):
    return max((H + BKT_FILL - 1) // BKT_FILL, 1)


def psort_applicable(H, max_hash):
    nb = (H + BKT_FILL - 1) // BKT_FILL
    return H > 0 and (max_hash // nb >= BKT_SLOTS or nb == 1)


def two_level_geometry(H):
    """(P1, P2) of yh_psort_begin."""
    nb = n_buckets(H)
    p2 = 1
    while p2 * p2 < nb:
        p2 += 1
    return (nb + p2 - 1) // p2, p2


def pieces_geometry(H, max_hash, n_refs):
    """(P1, P2) of pc_geometry, or None where the piece distribution does not take the database."""
    if not psort_applicable(H, max_hash) or n_refs == 0 or max_hash == M64:
        return None
    nb = n_buckets(H)
    p2 = min(max(int(2.0 * math.sqrt(nb) + 0.5), 1), PART_MAX_BINS, nb)
    if p2 == 1:
        return None
    return (nb + p2 - 1) // p2, p2


def region_of(h, H, max_hash):
    """First-level region of hash h in the two-level sort of a database of H hashes: fine = umulhi(h << lsh, mul_fine),
    bucket = fine >> 12, region = bucket / P2 (k_part's bin_of, clamped as there)."""
    p1, p2 = two_level_geometry(H)
    bits = max(int(max_hash).bit_length(), 1)
    mul = min(((p1 * p2 * BKT_SLOTS) << bits) // (max_hash + 1), M64)
    fine = ((((int(h) << (64 - bits)) & M64) * mul) >> 64) & 0xffffffff
    return min((fine >> BKT_SLOT_BITS) // p2, p1 - 1)


def upload_chunks(offsets):
    """Reference boundaries of the chunked upload (upload_sorted_impl: shares of the hashes moved to reference boundaries)."""
    n = offsets.size - 1
    H = int(offsets[-1])
    rb, acc = [0], 0.0
    for s in UPLOAD_SHARES[:-1]:
        acc += s
        r = int(np.searchsorted(offsets, np.uint64(int(float(H) * acc)), side="left"))
        if rb[-1] < r < n:
            rb.append(r)
    return rb + [n]


# ---- the bases ----------------------------------------------------------------------------------------------------------------
class Base:
    def __init__(self, name, values, offsets, targets):
        self.name = name
        self.values = values
        self.offsets = offsets
        self.targets = targets   # class -> sketch index
        self.values.setflags(write=False)
        self.offsets.setflags(write=False)

    @property
    def n_refs(self):
        return self.offsets.size - 1

    @property
    def H(self):
        return int(self.values.size)

    @property
    def max_hash(self):
        """What k_ref_extents reports: the largest LAST element."""
        o = self.offsets.astype(np.int64)
        ends = o[1:][o[1:] > o[:-1]]
        return int(self.values[ends - 1].max())

    def sketch(self, j):
        return self.values[int(self.offsets[j]):int(self.offsets[j + 1])]


def _exact(rng, n, lo, hi, pool):
    """n distinct hashes of [lo, hi), a third of them from `pool` (hashes that other sketches hold too), ascending."""
    got = set()
    if pool is not None and n >= 3:
        got.update(int(x) for x in rng.choice(pool, size=min(n // 3, pool.size), replace=False))
    while len(got) < n:
        got.update(int(x) for x in rng.integers(lo, hi, size=n - len(got), dtype=np.uint64))
    return np.array(sorted(got), dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def base(name):
    if name == "R":
        a = base("A")
        common = np.uint64(MAX_HASH_SCALED_1000 // 3)   # (not the largest hash; 1 100 holders in one slot)
        values = np.concatenate([a.values, np.full(N_REFUSED_HOLDERS, common, np.uint64)])
        offsets = np.concatenate([a.offsets, a.offsets[-1] + np.arange(1, N_REFUSED_HOLDERS + 1, dtype=np.uint64)])
        return Base("R", values, offsets, dict(a.targets))
    layout = _LAYOUT[name]
    rng = np.random.default_rng({"A": 20260, "B": 20261, "C": 20262, "D": 20263}[name])
    lo, hi = {"A": (1, MAX_HASH_SCALED_1000 - 1), "B": (1, MAX_HASH_SCALED_1000 - 1), "C": (1, M64 - 2), "D": (1, 7999)}[name]
    pool = np.unique(rng.integers(lo, hi, size=400, dtype=np.uint64))
    sketches, targets = [], {}
    for j, (size, role) in enumerate(layout):
        s = _exact(rng, size, lo, hi, pool)
        if role == "crown":      # the database's largest hash lives here, in no target
            s[-1] = np.uint64({"A": MAX_HASH_SCALED_1000 - 1, "B": MAX_HASH_SCALED_1000 - 1, "C": M64, "D": 7999}[name])
        elif role:
            targets[role] = j
        sketches.append(s)
    offsets = np.zeros(len(sketches) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([s.size for s in sketches], dtype=np.uint64)
    values = np.concatenate(sketches)
    # the sketches on either side of a chunk boundary of the upload: the first boundary with two sketches long enough
    rb = upload_chunks(offsets)
    for r in rb[1:-1]:
        if layout[r - 1][0] >= 63 and layout[r][0] >= 63 and not layout[r - 1][1] and not layout[r][1]:
            targets["chunk_last"], targets["chunk_first"] = r - 1, r
            break
    return Base(name, values, offsets, targets)


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def q_classes(start, size):
    """q -> the classes it belongs to, for a target of `size` hashes at global position `start`."""
    out = {}
    for q in Q_FIXED:
        if q < size:
            out.setdefault(q, []).append(f"q{q}")
    out.setdefault(size - 1, []).append("last")
    for g in G_EDGES:
        q = (-start) % g or g
        if 1 <= q < size:
            out.setdefault(q, []).append(f"g{g}")
    return out


def site_info(site):
    """(target class, [q classes], kind, crosses) of a site string "target:q+q:kind[:cross|:stay]"."""
    parts = site.split(":")
    return parts[0], parts[1].split("+"), parts[2] if len(parts) > 2 else None, (parts[3] == "cross") if len(parts) > 3 else None


def expected_error(name):
    return "invalid_arg" if name.endswith("/offsets_first") else "unsorted"


def cases(base_name):
    """(name, clean_values, clean_offsets, bad_values, bad_offsets, site) for every case of a base."""
    b = base(base_name)
    H, mh = b.H, b.max_hash
    for tclass, j in sorted(b.targets.items(), key=lambda kv: kv[1]):
        start, size = int(b.offsets[j]), int(b.offsets[j + 1] - b.offsets[j])
        v = [int(x) for x in b.sketch(j)]
        for q, classes in sorted(q_classes(start, size).items()):
            for kind in KINDS:
                bad = b.values.copy()
                crosses = None
                if kind == "swap":
                    bad[start + q - 1], bad[start + q] = v[q], v[q - 1]
                    crosses = region_of(v[q], H, mh) != region_of(v[q - 1], H, mh)
                elif kind == "equal":
                    bad[start + q] = v[q - 1]
                else:
                    new = v[q - 1] - 1 if kind == "near" else v[0] - 1
                    if kind == "far" and q == 1:
                        continue      # (the same value as `near`)
                    bad[start + q] = new
                    crosses = region_of(new, H, mh) != region_of(v[q - 1], H, mh)
                site = f"{tclass}:{'+'.join(classes)}:{kind}" + ("" if crosses is None else (":cross" if crosses else ":stay"))
                yield f"{base_name}/{tclass}/{'+'.join(classes)}/{kind}", b.values, b.offsets, bad, b.offsets, site
    # offsets: one offset above its successor (every offset <= H); offsets[0] = 1
    j = b.targets["cross1024"]
    off = b.offsets.copy()
    off[j] = b.offsets[j + 1] + np.uint64(3)
    assert int(off[j]) <= H
    yield f"{base_name}/offsets_nonmonotone", b.values, b.offsets, b.values, off, "offsets:nonmonotone"
    off = b.offsets.copy()
    off[0] = 1
    yield f"{base_name}/offsets_first", b.values, b.offsets, b.values, off, "offsets:first"
    # the named exception: an interior element above the largest last element (not where 2^64 - 1 is the largest hash)
    if mh < M64 - 1:
        j = b.targets["start0"]
        bad = b.values.copy()
        bad[int(b.offsets[j]) + 100] = np.uint64(M64 - 1)
        yield f"{base_name}/above_max", b.values, b.offsets, bad, b.offsets, "start0:above_max"


@functools.lru_cache(maxsize=None)
def all_cases(base_name):
    return tuple(cases(base_name))
