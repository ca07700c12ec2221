"""Case generators for the directory over the database's distinct hashes (YhDirView, yh_common.h; built in yh_build.hip),
numpy and plain Python ints only: databases that reach the states of the three bucket forms by construction -- exactly 7 and
8 entries of a compact bucket, more than 64, a wrapped probe chain of the overflow table, hashes 2^32 apart on both sides of
the compact form's span rule, bucket boundaries that are no powers of two, 5 against 6 entries of a wide bucket, references
that crowd one slot of the LDS hit table, holder lists of every length the walk and the record builder distinguish -- and
the samples that ask them.  Shared by tests/test_lookup_cases_cpu.py (which guards that the cases still hold what they are
named for) and tests/test_gpu_lookup_edges.py (which runs them on the device).

The first part is a MIRROR of the geometry decision in plain ints.  It is used to construct the cases and to prove that they
reach their state; expected counts never come from it (they come from the oracles).
"""
import functools

import numpy as np

M64 = (1 << 64) - 1
TWO32 = 1 << 32
CBKT_ENTRIES = 7        # hashes a compact bucket holds; the rest go to the overflow table
WIDE_ENTRIES = 5        # hashes a wide bucket holds; a fuller one sends the lookup to the two-level directory
RANK_STOP = 64          # where the build's rank count stops
OVF_MIN_CAP = 1024


# ---- the mirror ---------------------------------------------------------------------------------------------------------
def bits_of(max_hash: int) -> int:
    bits = 1
    while bits < 64 and (max_hash >> bits) != 0:
        bits += 1
    return bits


def mul_for(nb: int, bits: int, max_hash: int) -> int:
    """floor(nb * 2^bits / (max_hash + 1)), saturated to 64 bits."""
    return min((nb << bits) // (max_hash + 1), M64)


class Geometry:
    """What the build decides from (max_hash, number of distinct hashes) and the two form switches."""

    def __init__(self, max_hash: int, n_distinct: int, wide_buckets: bool = False, no_buckets: bool = False):
        self.max_hash, self.n_distinct = max_hash, n_distinct
        self.bits = bits_of(max_hash)
        self.nb_c = max((2 * n_distinct + 4) // 5, 1)
        self.mul_c = mul_for(self.nb_c, self.bits, max_hash)
        self.span_c = -(-(1 << self.bits) // self.mul_c) if self.mul_c else None
        compact = (not wide_buckets and self.nb_c <= 0xFFFFFFF0 and self.mul_c > 0
                   and (self.bits <= 32 or self.span_c <= TWO32))
        lg = 4
        while lg < 30 and (4 << lg) < n_distinct:
            lg += 1
        self.dir_shift = self.bits - lg if self.bits > lg else 0
        self.dir_nb = (max_hash >> self.dir_shift) + 1
        if compact:
            self.form, self.nb, self.mul = "compact", self.nb_c, self.mul_c
        elif no_buckets:
            self.form, self.nb, self.mul = "directory", 0, 0
        else:
            self.form = "wide"
            self.nb = (n_distinct + 1) // 2
            self.mul = max(mul_for(self.nb, self.bits, max_hash), 1)
        self.span = -(-(1 << self.bits) // self.mul) if self.mul else None
        self.entries = CBKT_ENTRIES if compact else WIDE_ENTRIES

    def bucket(self, h: int) -> int:
        """(h * mul) >> bits, for h <= max_hash."""
        assert 0 <= h <= self.max_hash and self.mul
        return (h * self.mul) >> self.bits

    def first_of(self, b: int) -> int:
        """The smallest hash of bucket b: ceil(b * 2^bits / mul)."""
        return -(-(b << self.bits) // self.mul)


def ovf_slot(h: int) -> int:
    h ^= h >> 33
    h = (h * 0xFF51AFD7ED558CCD) & M64
    h ^= h >> 33
    return h


def occupancy(hashes, g: Geometry) -> dict:
    """bucket -> the distinct hashes in it, ascending."""
    out = {}
    for h in sorted(int(x) for x in hashes):
        out.setdefault(g.bucket(h), []).append(h)
    return out


def overflow_entries(hashes, g: Geometry) -> list:
    """The hashes beyond the seventh of their compact bucket."""
    return [h for run in occupancy(hashes, g).values() for h in run[CBKT_ENTRIES:]]


def ovf_capacity(n_over: int) -> int:
    cap = OVF_MIN_CAP
    while cap < 2 * n_over + 16:
        cap <<= 1
    return cap


def ovf_place(entries, cap: int) -> dict:
    """hash -> slot after linear probing from ovf_slot(h) & (cap - 1), inserted in the given order.  The SET of occupied slots
    does not depend on the order (the build inserts concurrently); which hash sits where does."""
    taken, where = set(), {}
    for h in entries:
        s = ovf_slot(h) & (cap - 1)
        while s in taken:
            s = (s + 1) & (cap - 1)
        taken.add(s)
        where[h] = s
    return where


def ovf_probe_steps(h: int, occupied: set, cap: int) -> int:
    """Occupied slots an absent hash passes before it ends at an empty one."""
    s, steps = ovf_slot(h) & (cap - 1), 0
    while s in occupied:
        s = (s + 1) & (cap - 1)
        steps += 1
        assert steps < cap
    return steps


def filter_geometry(g: Geometry, bph: int):
    """(bits of the presence filter, its multiplier)."""
    fbits = ((g.n_distinct * bph + 511) // 512) * 512
    return fbits, mul_for(fbits, g.bits, g.max_hash)


def filter_word_mask(h: int, g: Geometry, fmul: int):
    """(index of the 32-bit filter word of h, the two bits it owns there)."""
    bit = (h * fmul) >> g.bits
    m = ((h * 0x9E3779B97F4A7C15) & M64) >> 49
    return bit >> 5, (1 << (m & 31)) | (1 << ((m >> 5) & 31))


def hit_slot(ref: int, tbits: int) -> int:
    """First slot of a reference in a workgroup's hit table of 2^tbits slots."""
    return ((ref * 2654435761) & 0xFFFFFFFF) >> (32 - tbits)


# ---- databases ----------------------------------------------------------------------------------------------------------
class Database:
    """A list of sketches, the form its directory must take, and what its sample gets beyond the general rule."""

    def __init__(self, name, refs, form, extra=(), pad_lo=0, meta=None, sample_of=None):
        self.name, self.form = name, form
        self.sample_of = sample_of                      # the database whose sample this one is asked with (None: its own)
        self.refs = [np.array(sorted(int(x) for x in r), dtype=np.uint64) for r in refs]
        self.extra = sorted(int(x) for x in extra)      # absent hashes the sample asks in addition
        self.pad_lo = pad_lo                            # the fill of the padded samples stays at or above this
        self.meta = meta or {}
        self.distinct = sorted({int(x) for r in self.refs for x in r})
        self.max_hash = self.distinct[-1]
        assert not set(self.extra) & set(self.distinct)

    @property
    def n_refs(self):
        return len(self.refs)

    def geometry(self, **kw) -> Geometry:
        return Geometry(self.max_hash, len(self.distinct), **kw)

    def csr(self):
        offsets = np.zeros(len(self.refs) + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum([r.size for r in self.refs], dtype=np.uint64)
        values = np.concatenate(self.refs) if int(offsets[-1]) else np.zeros(0, np.uint64)
        return np.ascontiguousarray(values, dtype=np.uint64), offsets

    def holders(self) -> dict:
        """hash -> number of references that hold it."""
        u, c = np.unique(self.csr()[0], return_counts=True)
        return {int(h): int(k) for h, k in zip(u, c)}


def _spread(rng, hashes, n_refs=24):
    """Sketches that together hold exactly `hashes`: six in ten with one holder, the others with 2..12."""
    hashes = np.array(sorted(hashes), dtype=np.uint64)
    k = np.where(rng.random(hashes.size) < 0.6, 1, rng.integers(2, max(min(n_refs, 12), 2) + 1, size=hashes.size))
    k = np.minimum(k, n_refs)
    rank = rng.random((hashes.size, n_refs)).argsort(axis=1).argsort(axis=1)
    member = rank < k[:, None]
    return [hashes[member[:, j]] for j in range(n_refs)]


def _even_counts(total: int, n: int) -> list:
    """total spread over n buckets as evenly as it goes."""
    return [total // n + (1 if i < total % n else 0) for i in range(n)]


def _lows(rng, n: int, avoid=()) -> list:
    """n distinct 32-bit words from [1, 2^32 - 2] outside `avoid`."""
    out, avoid = set(), set(avoid)
    while len(out) < n:
        for x in rng.integers(1, TWO32 - 1, size=n - len(out)):
            if int(x) not in avoid:
                out.add(int(x))
    return sorted(out)


# compact_edge / wide_edge: bits 44, 4096 buckets of exactly 2^32 values -- or one bucket fewer
EDGE_MAX = (1 << 44) - 1
EDGE_FIRST = 100
EDGE_OCC = (7, 0, 8, 1, 64, 6, 65, 9, 66, 15, 200, 63)     # occupancies of buckets 100, 101, ...: 7 and 8 next to an empty one
EDGE_D = 10_238


@functools.lru_cache(maxsize=None)
def _edge_hashes():
    """(chosen bucket -> its hashes, the fillers) of compact_edge.  The low words of the chosen buckets differ from bucket to
    bucket, except 0 and 0xffffffff, which the buckets of 7 and of 8 entries both hold as their first and last."""
    rng = np.random.default_rng(4401)
    lows = _lows(rng, sum(EDGE_OCC))
    rng.shuffle(lows)
    chosen, at = {}, 0
    for i, n in enumerate(EDGE_OCC):
        b = EDGE_FIRST + i
        mine = sorted(lows[at: at + n])
        at += n
        if n in (7, 8):
            mine[0], mine[-1] = 0, TWO32 - 1
        chosen[b] = [(b << 32) | lo for lo in mine]
    taken = {h for run in chosen.values() for h in run} | {0, EDGE_MAX}
    fill = set()
    while len(taken) + len(fill) < EDGE_D:
        b = int(rng.integers(0, 4096))
        if EDGE_FIRST - 1 <= b <= EDGE_FIRST + len(EDGE_OCC):
            continue
        h = (b << 32) | int(rng.integers(0, TWO32))
        if h not in taken:
            fill.add(h)
    return chosen, sorted(fill)


def compact_edge():
    chosen, fill = _edge_hashes()
    hashes = [h for run in chosen.values() for h in run] + fill + [0, EDGE_MAX]
    return Database("compact_edge", _spread(np.random.default_rng(4402), hashes), "compact", meta={"chosen": chosen})


def wide_edge():
    """compact_edge without one filler: 4095 buckets would span more than 2^32 values, so the form must be the wide one."""
    chosen, fill = _edge_hashes()
    hashes = [h for run in chosen.values() for h in run] + fill[1:] + [0, EDGE_MAX]
    return Database("wide_edge", _spread(np.random.default_rng(4402), hashes), "wide", meta={"chosen": chosen}, sample_of="compact_edge")


# compact_odd: 5000 buckets over 2^44, boundaries that are no powers of two
ODD_D = 12_500
ODD_K = tuple(7 + 20 * j for j in range(240))


def compact_odd():
    rng = np.random.default_rng(4403)
    nb = 5000
    present, absent, pairs = {0, EDGE_MAX}, set(), []
    for j, k in enumerate(ODD_K):
        e = -(-(k << 44) // nb)
        kind = ("both", "below", "above")[j % 3]     # which of e - 1 (last of bucket k - 1) and e (first of bucket k) the database holds
        pairs.append((k, e, kind))
        (present if kind != "above" else absent).add(e - 1)
        (present if kind != "below" else absent).add(e)
    while len(present) < ODD_D:
        h = int(rng.integers(0, 1 << 44))
        if h not in absent:
            present.add(h)
    return Database("compact_odd", _spread(rng, present), "compact", meta={"pairs": pairs})


# compact_small: at most 32 bits (33 in one case); always compact
def compact_small():
    rng = np.random.default_rng(4404)
    out = []

    def db(name, hashes, n_refs):
        out.append(Database(name, _spread(rng, hashes, n_refs), "compact"))

    db("small_0", [0], 1)
    db("small_01", [0, 1], 2)
    db("small_012", [0, 1, 2], 3)
    db("small_5_bits32", [0, 5, 1 << 31, TWO32 - 2, TWO32 - 1], 3)
    db("small_5_bits33", [0, 1, (1 << 31) + 7, TWO32 - 1, TWO32], 3)
    db("small_dense", range(8192), 24)
    # 300 consecutive values from the first hash of bucket 400, 1500 hashes elsewhere below 2^20: D = 1800, 720 buckets
    g = Geometry((1 << 20) - 1, 1800)
    lo, hi = g.first_of(400), g.first_of(401)
    assert hi - lo >= 300
    hashes = set(range(lo, lo + 300)) | {0, (1 << 20) - 1}
    while len(hashes) < 1800:
        h = int(rng.integers(0, 1 << 20))
        if not lo <= h < hi:
            hashes.add(h)
    out.append(Database("small_run300", _spread(rng, hashes), "compact", meta={"run_bucket": 400}))
    return out


# databases too small to have twenty sample hashes of every class (small_dense: no absent hash up to max_hash at all)
SMALL_WITHOUT_CLASSES = ("small_0", "small_01", "small_012", "small_5_bits32", "small_5_bits33", "small_dense")
NOTHING_ABOVE_MAX = ("wide_full", "wide_four")                  # max_hash = 2^64 - 1


# overflow_chain: an overflow table of the minimum capacity, as full as that capacity gets, its chain wrapped
OVF_HEAVY = tuple(300 + 511 * t for t in range(8))          # eight buckets of 7 + 63 hashes: 504 overflow entries
OVF_WRAP_HOMES = 48                                          # of them with home slots 1000..1023 (24 slots: the chain must wrap)


def _overflow_db(name, n_over):
    rng = np.random.default_rng(4405)
    heavy, nxt = {}, 1_000_000
    for t, b in enumerate(OVF_HEAVY):
        base = b << 32
        run = [base | (1000 * (i + 1)) for i in range(CBKT_ENTRIES)]
        want_wrap = OVF_WRAP_HOMES if t == 0 else 0
        n_here = 63 + (1 if t == 1 and n_over == 505 else 0)
        over = []
        while len(over) < n_here:
            h = base | nxt
            nxt += 1
            if want_wrap and (ovf_slot(h) & (OVF_MIN_CAP - 1)) < 1000:
                continue
            want_wrap = max(want_wrap - 1, 0)
            over.append(h)
        heavy[b] = run + over
    n_heavy = sum(len(r) for r in heavy.values())
    assert n_heavy == 8 * CBKT_ENTRIES + n_over
    light = [b for b in range(4096) if b not in heavy]
    hashes = {h for r in heavy.values() for h in r}
    for b, cnt in zip(light, _even_counts(EDGE_D - 8 * (CBKT_ENTRIES + 63), len(light))):
        assert cnt <= CBKT_ENTRIES
        lows = _lows(rng, cnt)
        if b == 0:
            lows[0] = 0
        if b == 4095:
            lows[-1] = TWO32 - 1
        hashes |= {(b << 32) | lo for lo in lows}
    assert len(hashes) == EDGE_D + (n_over - 504)
    # absent hashes of the flagged buckets whose home slot is occupied: they walk an occupied run, end at an empty slot, miss
    cap = ovf_capacity(n_over)
    occupied = set(ovf_place([h for r in heavy.values() for h in r[CBKT_ENTRIES:]], cap).values())
    probes, c = [], 500_000_000
    need_wrap = 8 if cap == OVF_MIN_CAP else 0
    while len(probes) < 60:
        h = (OVF_HEAVY[c % 8] << 32) | c
        c += 1
        home = ovf_slot(h) & (cap - 1)
        if home not in occupied or (need_wrap and home < 1000):
            continue
        need_wrap = max(need_wrap - 1, 0)
        probes.append(h)
    return Database(name, _spread(rng, hashes), "compact", extra=probes, meta={"heavy": heavy, "n_over": n_over, "probes": probes})


def overflow_chain():
    return [_overflow_db("overflow_504", 504), _overflow_db("overflow_505", 505)]


# wide_full: the whole 64-bit range, 2048 wide buckets of 2^53 values
FULL_FIRST = 500
FULL_OCC = (0, 1, 4, 5, 6, 7, 30)
FULL_D = 4096


def wide_full(name="wide_full", seed=4406, zero=True):
    """zero=False ("wide_four"): hash 0 is absent and bucket 0 holds exactly four hashes -- a lookup of 0 there must not be
    answered by the all-zero fifth entry of the bucket."""
    rng = np.random.default_rng(seed)
    chosen, both, one = {}, [], []
    for i, n in enumerate(FULL_OCC):
        b = FULL_FIRST + i
        run, off = [], TWO32 + int(rng.integers(0, 1 << 40))
        for _ in range(n // 3):                      # pairs h, h + 2^32, both in the database
            h = (b << 53) + off
            run += [h, h + TWO32]
            both.append(h)
            off += 3 * TWO32 + int(rng.integers(0, 1 << 40))
        while len(run) < n:                          # h alone: h - 2^32 and h + 2^32 are absent, in the same bucket
            h = (b << 53) + off
            run.append(h)
            one.append(h)
            off += 3 * TWO32 + int(rng.integers(0, 1 << 40))
        assert off < (1 << 53) - 2 * TWO32
        chosen[b] = sorted(run)
    hashes = {h for r in chosen.values() for h in r}
    light = [b for b in range(2048) if b not in chosen]
    for b, cnt in zip(light, _even_counts(FULL_D - len(hashes), len(light))):
        mine = {(b << 53) + int(x) for x in rng.integers(1, (1 << 53) - 1, size=cnt)}
        if b == 0 and zero:
            mine = set(sorted(mine)[1:]) | {0}
        if b == 0 and not zero:
            mine = {(1 << 40) + 977 * i for i in range(4)}
        if b == 2047:
            mine = set(sorted(mine)[:-1]) | {M64}
        assert len(mine) == cnt or (b == 0 and not zero)
        hashes |= mine
    if not zero:        # (bucket 0 took 4 hashes instead of its share: D back to FULL_D through another light bucket)
        spare = sorted(h for h in hashes if h >> 53 == 1000)
        while len(hashes) > FULL_D:
            hashes.discard(spare.pop())
        while len(hashes) < FULL_D:
            hashes.add((1000 << 53) + int(rng.integers(1, 1 << 52)))
    assert len(hashes) == FULL_D
    return Database(name, _spread(rng, hashes), "wide", meta={"chosen": chosen, "both": both, "one": one})


# crowd: 6000 references, groups of them on one slot of the hit table, holder lists of every length that matters
CROWD_REFS = 6000
CROWD_GROUPS = 24                                   # per table size
CROWD_GROUP = 4
CROWD_HOLDERS = (2, 3, 4, 5, 7, 8, 9, 10, 33)
CROWD_LOW = 1 << 43                                 # the groups sit below, everything else (and every pad) above
TILE = 256


def _crowd_groups():
    """Groups of CROWD_GROUP reference ids: the first CROWD_GROUPS share the first slot of the 2^10 table (and so of the 2^8
    one), the others share the first slot of the 2^8 table only."""
    by10 = {}
    for r in range(CROWD_REFS):
        by10.setdefault(hit_slot(r, 10), []).append(r)
    groups, used = [], set()
    for s in sorted(by10):
        if len(by10[s]) >= CROWD_GROUP and len(groups) < CROWD_GROUPS:
            groups.append((10, by10[s][:CROWD_GROUP]))
            used |= set(by10[s][:CROWD_GROUP])
    for s8 in range(TILE):
        if len(groups) == 2 * CROWD_GROUPS:
            break
        ids = [by10[s][-1] for s in range(4 * s8, 4 * s8 + 4) if s in by10 and by10[s][-1] not in used]
        if len(ids) >= 3:
            groups.append((8, ids))
            used |= set(ids)
    assert len(groups) == 2 * CROWD_GROUPS
    return groups


def crowd():
    rng = np.random.default_rng(4407)
    refs = [[] for _ in range(CROWD_REFS)]
    groups, spans = _crowd_groups(), []
    for g, (tbits, ids) in enumerate(groups):
        base = ((g + 1) << 33) + 8                  # the group's hashes 4 apart: with their h - 1 / h + 1 they are adjacent in the sample
        hs = [base + 4 * i for i in range(len(ids) + 1)]
        shared = hs.pop(len(ids) // 2)
        for r, h in zip(ids, hs):
            refs[r].append(h)
        for r in ids:
            refs[r].append(shared)
        spans.append((tbits, list(ids), base, shared))
    taken = set()

    def fresh():
        while True:
            h = int(rng.integers(CROWD_LOW + (1 << 33), (1 << 44) - (1 << 33)))
            if h not in taken:
                taken.add(h)
                return h

    member = {r for _, ids in groups for r in ids}
    for r in range(CROWD_REFS):
        for _ in range(1 + r % 3 - (1 if r in member else 0)):
            refs[r].append(fresh())
    refs[CROWD_REFS - 1][-1] = EDGE_MAX           # (its last private hash: the largest of the database)
    lists = {}
    for k in CROWD_HOLDERS:
        for _ in range(3):
            h = fresh()
            lists[h] = k
            for r in rng.choice(CROWD_REFS, size=k, replace=False):
                refs[int(r)].append(h)
    db = Database("crowd", refs, "compact", pad_lo=CROWD_LOW, meta={"groups": spans, "lists": lists})
    # absent hashes in front of a group that would straddle a 256-hash tile of the sample, until it does not
    s = _rule_sample(db)
    nudges = []
    for tbits, ids, base, shared in spans:
        width = 3 * (len(ids) + 1)                  # h - 1, h, h + 1 of every hash of the group
        pos = int(np.searchsorted(s, np.uint64(base - 1))) + len(nudges)
        if pos % TILE + width > TILE:
            nudges += [base - 100 - j for j in range(TILE - pos % TILE)]
    db.extra = sorted(nudges)
    return db


@functools.lru_cache(maxsize=None)
def databases() -> tuple:
    return tuple([compact_edge(), wide_edge(), compact_odd()] + compact_small() + overflow_chain() + [wide_full(), wide_full("wide_four", 4409, zero=False), crowd()])


def database(name: str) -> Database:
    return {d.name: d for d in databases()}[name]


# ---- samples ------------------------------------------------------------------------------------------------------------
PREFIXES = (1, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097)
PADDED = (262_143, 262_144, 524_288, 524_289)
ABOVE = 24                                          # hashes between max_hash + 2 and 2^64 - 2 that every base sample asks


def _rule_sample(db: Database) -> np.ndarray:
    """Every distinct hash; h - 1, h + 1, h - 2^32, h + 2^32 where that is a 64-bit value and absent; 0, max_hash,
    max_hash + 1, 2^64 - 1; ABOVE hashes spread over the range above max_hash; the database's own extra hashes."""
    if db.sample_of:
        return _rule_sample(database(db.sample_of))
    d = np.array(db.distinct, dtype=np.uint64)
    parts = [d, np.array([0, db.max_hash, min(db.max_hash + 1, M64), M64], dtype=np.uint64), np.array(db.extra, dtype=np.uint64)]
    room = M64 - db.max_hash - 2
    if room >= 4 * ABOVE:                               # (the rule alone leaves only a handful above max_hash)
        parts.append(np.array([db.max_hash + 2 + j * (room // ABOVE) for j in range(ABOVE)], dtype=np.uint64))
    for step in (1, TWO32):
        parts.append(d[d >= np.uint64(step)] - np.uint64(step))
        parts.append(d[d <= np.uint64(M64 - step)] + np.uint64(step))
    return np.unique(np.concatenate(parts))


@functools.lru_cache(maxsize=None)
def _pads(name: str) -> np.ndarray:
    """Absent hashes in a fixed random order, enough to fill the largest padded sample: half of them inside
    [pad_lo, max_hash] where that range has the room, the others above max_hash (all inside where max_hash is 2^64 - 1)."""
    db = database(name)
    base = _rule_sample(db)
    rng = np.random.default_rng(4408)
    need = PADDED[-1]
    inside = need // 2 if db.max_hash - db.pad_lo > 16 * need else 0
    if db.max_hash >= M64 - 16 * need:
        inside = need
    parts = []
    if inside:
        parts.append(rng.integers(db.pad_lo, db.max_hash, size=inside + inside // 8, dtype=np.uint64, endpoint=True))
    if need - inside:
        k = need - inside
        parts.append(rng.integers(max(db.max_hash + 2, db.pad_lo), M64 - 1, size=k + k // 8, dtype=np.uint64))
    p = np.unique(np.concatenate(parts))
    p = p[~np.isin(p, base)]
    assert p.size >= need
    return rng.permutation(p)[:need]


@functools.lru_cache(maxsize=None)
def samples(name: str) -> dict:
    """label -> strictly ascending uint64 sample: "base" (the rule above), "prefix_n" (its first n hashes, where it has more),
    "padded_n" (base filled with absent hashes to n)."""
    db = database(name)
    base = _rule_sample(db)
    out = {"base": base}
    for n in PREFIXES:
        if n < base.size:
            out[f"prefix_{n}"] = base[:n].copy()
    pads = _pads(name)
    for n in PADDED:
        out[f"padded_{n}"] = np.sort(np.concatenate([base, pads[: n - base.size]]))
    for s in out.values():
        s.setflags(write=False)
    return out


def classes(db: Database, sample: np.ndarray, g: Geometry = None) -> dict:
    """How many sample hashes are: held by one reference, held by several, absent but in a bucket that holds hashes, above
    max_hash."""
    g = g or db.geometry()
    held = db.holders()
    occupied = set(occupancy(db.distinct, g)) if g.mul else set()
    out = {"present_single": 0, "present_shared": 0, "absent_same_bucket": 0, "absent_above_max": 0}
    for h in (int(x) for x in sample):
        if h in held:
            out["present_single" if held[h] == 1 else "present_shared"] += 1
        elif h > db.max_hash:
            out["absent_above_max"] += 1
        elif g.mul and g.bucket(h) in occupied:
            out["absent_same_bucket"] += 1
    return out
