"""Reference databases that sit ON the capacities the build's distribution sort decides by, numpy only.

Never calls the library.  yacht_amd/csrc/yh_sort.hip cuts everything from ONE linear function of the hash -- the fine slot,
fine = umulhi(h << lsh, mul), bucket = fine >> 12, slot = fine & 4095 -- and decides by three capacities which way a database
goes: a final bucket holds BKT_CAP = 4 096 pairs, a slot of k_bucket_sort ranks at most SLOT_MAX = 1 024 pairs, a first-level
region of the two-level sort holds cap1 pairs.  Behind the piece distribution a bucket over a capacity goes to the side list
(k_spill_collect, k_spill_keys, k_spill_gather, k_spill_group, k_spill_place) and the rest of the database never notices;
the two-level sort has no side list and REFUSES the keys (flag bits 1 region, 2 bucket, 4 slot), after which rocPRIM sorts.

The model below restates that function (fine_of, exactly as order_cases.region_of does it) and the rules:
    pieces, `yacht train`'s handle ("train")     a bucket is marked when it holds more than 4 096 pairs
    pieces, a sorting handle ("sort")            ... or when one of its slots holds more than 1 024 pairs
    two-level                                    nothing is marked: a region over cap1, a bucket over 4 096 or -- sorting
                                                 handles -- a slot over 1 024 refuses the whole attempt
The number of buckets NB = P1 x P2 differs between the two geometries (pc_geometry against yh_psort_begin), so the same
database has other buckets on either path: every case is built to be exact for ONE geometry (`case.geometry`) and the model
says what the other one makes of it.  max_hash is the largest LAST element of any sketch, which is what k_ref_extents reports.

Every case names its target bucket(s).  The background (uniform hashes below max_hash_for_scaled(1000)) and the padding of
the holder sketches keep out of the targets' key ranges, so a target holds what the case puts there: hot hashes (holders are
sketches of 3 to 6 hashes, two bare one-hash holders each), hashes with 1, 2, 3, 4, 5 and 9 holders, the bucket's smallest and
largest key, and one-holder fillers that bring the count to the named number.  tests/test_sort_cap_cases_cpu.py asserts,
with the model, that every case is what its name says.

Families (the geometry is stated per case and asserted):
    S   H = 22 000: nine buckets' worth -- pieces P1 2 x P2 6 = 12 buckets, two-level P1 3 x P2 3 = 9
    D   H = 96 000: pieces P1 4 x P2 12 = 48 buckets (buckets 31 and 32 sit on either side of a word of the marked-bucket
        bit map), two-level P1 6 x P2 7 = 42
    R   H = 20 000, every hash but ONE sketch's last element in the lowest first-level region of the two-level sort (P1 3 x
        P2 3: with P1 = 2 a region's capacity H/2 + H/64 + 8 192 exceeds any H that has P1 = 2, so no database can overflow it)
"""
import functools

import numpy as np

import order_cases as oc
from order_cases import (BKT_SLOT_BITS, BKT_SLOTS, M64, MAX_HASH_SCALED_1000, PART_TILE, SLOT_MAX, csr_is_valid,  # noqa: F401
                         n_buckets, pieces_geometry, psort_applicable, two_level_geometry)

BKT_CAP = 4096
PATHS = ("pieces", "two_level")
HANDLES = ("train", "sort")
MAX_HASH = MAX_HASH_SCALED_1000 - 1
EXTRA_HOLDERS = (1, 2, 3, 4, 5, 9)
SORT_RADIX, SORT_TWO_LEVEL, SORT_PIECES = 1, 2, 3
MAX_H, MAX_REFS = 100_000, 10_000


# ---- the model ----------------------------------------------------------------------------------------------------------------
def geometry(H, max_hash, n_refs, path):
    """(P1, P2) of a path, None where the piece distribution does not take the database."""
    return pieces_geometry(H, max_hash, n_refs) if path == "pieces" else two_level_geometry(H)


def _mul(NB, max_hash):
    bits = max(int(max_hash).bit_length(), 1)
    return bits, min(((NB * BKT_SLOTS) << bits) // (int(max_hash) + 1), M64)


def fine_of(h, NB, max_hash):
    """The fine slot of hash h among NB buckets: umulhi(h << lsh, mul_fine), as the device computes it."""
    bits, mul = _mul(NB, max_hash)
    return ((((int(h) << (64 - bits)) & M64) * mul) >> 64) & 0xffffffff


def bucket_of(h, NB, max_hash):
    return min(fine_of(h, NB, max_hash) >> BKT_SLOT_BITS, NB - 1)


def slot_of(h, NB, max_hash):
    return fine_of(h, NB, max_hash) & (BKT_SLOTS - 1)


def fine_all(values, NB, max_hash):
    """fine_of for an array: the high word of a 64 x 64 bit product from 32-bit limbs (no intermediate leaves 64 bits)."""
    bits, mul = _mul(NB, max_hash)
    x = np.asarray(values, dtype=np.uint64) << np.uint64(64 - bits)
    lo32 = np.uint64(0xffffffff)
    s32 = np.uint64(32)
    x_lo, x_hi = x & lo32, x >> s32
    m_lo, m_hi = np.uint64(mul & 0xffffffff), np.uint64(mul >> 32)
    t = x_lo * m_lo
    c1 = x_hi * m_lo + (t >> s32)
    c2 = x_lo * m_hi + (c1 & lo32)
    return (x_hi * m_hi + (c1 >> s32) + (c2 >> s32)) & lo32


def fine_lo(f, NB, max_hash):
    """The smallest hash whose fine slot is >= f (max_hash + 1 where there is none): the function is monotone."""
    lo, hi = 0, int(max_hash) + 1
    while lo < hi:
        mid = (lo + hi) // 2
        if fine_of(mid, NB, max_hash) >= f:
            hi = mid
        else:
            lo = mid + 1
    return lo


def bucket_range(b, NB, max_hash):
    """[lo, hi) of the hashes of bucket b."""
    return fine_lo(b << BKT_SLOT_BITS, NB, max_hash), fine_lo((b + 1) << BKT_SLOT_BITS, NB, max_hash)


def db_max_hash(values, offsets):
    o = np.asarray(offsets).astype(np.int64)
    ends = o[1:][o[1:] > o[:-1]]
    return int(np.asarray(values)[ends - 1].max())


def _nb(values, offsets, path):
    H, n = int(np.asarray(values).size), int(np.asarray(offsets).size) - 1
    mh = db_max_hash(values, offsets)
    g = geometry(H, mh, n, path)
    return (None, mh) if g is None else (g[0] * g[1], mh)


def _fine(values, offsets, path):
    NB, mh = _nb(values, offsets, path)
    assert NB is not None, "the path does not take this database"
    return fine_all(values, NB, mh), NB


def bucket_counts(values, offsets, path):
    f, NB = _fine(values, offsets, path)
    return np.bincount(np.minimum(f >> np.uint64(BKT_SLOT_BITS), np.uint64(NB - 1)).astype(np.int64), minlength=NB)


def slot_counts(values, offsets, path, bucket):
    f, NB = _fine(values, offsets, path)
    b = np.minimum(f >> np.uint64(BKT_SLOT_BITS), np.uint64(NB - 1))
    return np.bincount((f[b == np.uint64(bucket)] & np.uint64(BKT_SLOTS - 1)).astype(np.int64), minlength=BKT_SLOTS)


def max_slot_counts(values, offsets, path):
    """The fullest slot of every bucket."""
    f, NB = _fine(values, offsets, path)
    uniq, cnt = np.unique(f, return_counts=True)
    out = np.zeros(NB, dtype=np.int64)
    np.maximum.at(out, np.minimum(uniq >> np.uint64(BKT_SLOT_BITS), np.uint64(NB - 1)).astype(np.int64), cnt)
    return out


def expected_spill(values, offsets, handle, path):
    """(the set of buckets the side list takes, the pairs they hold)."""
    if path != "pieces":
        return set(), 0
    cnt = bucket_counts(values, offsets, path)
    marked = cnt > BKT_CAP
    if handle == "sort":
        marked |= max_slot_counts(values, offsets, path) > SLOT_MAX
    return set(int(b) for b in np.flatnonzero(marked)), int(cnt[marked].sum())


def cap1_of(H, P1):
    """A first-level region's capacity (yh_psort_begin)."""
    return ((H // P1 + H // P1 // 32 + 2 * PART_TILE + 255) // 256) * 256


def region_counts(values, offsets):
    """Pairs per first-level region of the two-level sort."""
    H = int(np.asarray(values).size)
    p1, p2 = two_level_geometry(H)
    f, NB = _fine(values, offsets, "two_level")
    reg = np.minimum((f >> np.uint64(BKT_SLOT_BITS)) // np.uint64(p2), np.uint64(p1 - 1))
    return np.bincount(reg.astype(np.int64), minlength=p1)


def two_level_verdict(values, offsets, handle):
    """(refused, the flag bit that names the reason: 1 region, 2 bucket, 4 slot; 0 when taken).  A region that overflows
    loses pairs before the buckets are counted and a bucket that overflows before its slots are, so only the FIRST capacity
    exceeded is named; the flags printed may hold later bits as well (an overflowed bucket also raises bit 1: its run does
    not fit the bucket's room in the second level)."""
    H = int(np.asarray(values).size)
    p1, _ = two_level_geometry(H)
    if p1 > 1 and int(region_counts(values, offsets).max()) > cap1_of(H, p1):
        return True, 1
    if int(bucket_counts(values, offsets, "two_level").max()) > BKT_CAP:
        return True, 2
    if handle == "sort" and int(max_slot_counts(values, offsets, "two_level").max()) > SLOT_MAX:
        return True, 4
    return False, 0


def expected_outcome(values, offsets, handle, path):
    """What yh_db_info and the verdict line must say of a build that goes down `path` with a `handle`."""
    if path == "pieces":
        buckets, pairs = expected_spill(values, offsets, handle, path)
        return {"sort_path": SORT_PIECES, "verdict": "taken", "bit": 0, "n_spilled_buckets": len(buckets), "n_spilled_pairs": pairs}
    refused, bit = two_level_verdict(values, offsets, handle)
    return {"sort_path": SORT_RADIX if refused else SORT_TWO_LEVEL, "verdict": "REFUSED" if refused else "taken", "bit": bit,
            "n_spilled_buckets": 0, "n_spilled_pairs": 0}


# ---- the cases ----------------------------------------------------------------------------------------------------------------
_S = {"H": 22_000, "pieces": (2, 6), "two_level": (3, 3)}
_D = {"H": 96_000, "pieces": (4, 12), "two_level": (6, 7)}
_BG_SIZES = (1025, 513, 512, 65, 64, 63, 2, 1, 0, 300, 200, 130)


def _t(bucket, count, hot, slot_count=None, others=(), edges=(1, 2), walk=False):
    """A target bucket: its exact pair count; hot hashes as (slot, holders) -- slot an index, "first" (the database's smallest
    hash), "max" (max_hash itself) or "twin" (the hash in front + 1); slot_count: the exact count of the first hot hash's slot,
    reached with `others` = holder counts of further hashes in that slot; edges: holders of the bucket's smallest and largest key."""
    return {"bucket": bucket, "count": count, "hot": list(hot), "slot_count": slot_count, "others": tuple(others), "edges": edges, "walk": walk}


def _spec(name, fam, geometry_, targets, seed, nrefs_mod=None, cross=0):
    d = dict(fam)
    d.update({"name": name, "geometry": geometry_, "targets": targets, "seed": seed, "nrefs_mod": nrefs_mod, "cross": cross})
    return d


_FIVE = [(300, 805), (1100, 810), (2000, 820), (2900, 800), (3700, 815)]
SPECS = {s["name"]: s for s in [
    # bucket fill: one hot hash + filler (the count alone decides on `yacht train`'s handle; the hot slot marks it on the others)
    _spec("fill1_4095", _S, "pieces", [_t(5, 4095, [(700, 3000)])], 101),
    _spec("fill1_4096", _S, "pieces", [_t(5, 4096, [(700, 3000)], edges=(2, 1))], 102),
    _spec("fill1_4097", _S, "pieces", [_t(5, 4097, [(700, 3000)])], 103, nrefs_mod=0),
    # ... five hashes in five slots: no slot crowded, the count decides on every handle
    _spec("fill5_4095", _S, "pieces", [_t(7, 4095, _FIVE)], 111),
    _spec("fill5_4096", _S, "pieces", [_t(7, 4096, _FIVE, edges=(9, 1))], 112),
    _spec("fill5_4097", _S, "pieces", [_t(7, 4097, _FIVE, edges=(2, 1))], 113, nrefs_mod=1),
    # slot fill, in a bucket well below its capacity: the slot holds one hash alone
    _spec("slot_alone_1023", _S, "pieces", [_t(4, 2600, [(1500, 1023)], slot_count=1023)], 121),
    _spec("slot_alone_1024", _S, "pieces", [_t(4, 2600, [(1500, 1024)], slot_count=1024)], 122),
    _spec("slot_alone_1025", _S, "pieces", [_t(4, 2600, [(1500, 1025)], slot_count=1025, edges=(2, 1))], 123),
    # ... 1 020 holders of one hash + other hashes of the same slot
    _spec("slot_mixed_1023", _S, "pieces", [_t(8, 2600, [(2222, 1020)], slot_count=1023, others=(2, 1))], 131),
    _spec("slot_mixed_1024", _S, "pieces", [_t(8, 2600, [(2222, 1020)], slot_count=1024, others=(2, 1, 1))], 132),
    _spec("slot_mixed_1025", _S, "pieces", [_t(8, 2600, [(2222, 1020)], slot_count=1025, others=(2, 1, 1, 1))], 133),
    # where the spilled bucket sits
    _spec("bucket0", _S, "pieces", [_t(0, 4097, [("first", 3000)], edges=(0, 2))], 141),
    _spec("bucket_last", _S, "pieces", [_t("last", 4097, [("max", 3000)], edges=(1, 0))], 142),
    _spec("word_edge_31_32", _D, "pieces", [_t(31, 4097, [(900, 2600)], edges=(2, 1)), _t(32, 4101, [(3100, 2600)], edges=(1, 9))], 143, cross=5),
    _spec("adjacent_walk", _D, "pieces", [_t(20, 4100, [(4000, 2600)], edges=(1, 1), walk=True), _t(21, 4099, [(50, 2600)], edges=(1, 1), walk=True)], 144, cross=5),
    _spec("twin", _S, "pieces", [_t(9, 4097, [(1234, 2000), ("twin", 2000)], edges=(3, 1))], 145),
    # the side list's length: n mod 256 = 0 and 255 (4 097 = 1)
    _spec("len_mod256_0", _S, "pieces", [_t(6, 4352, [(64, 3000)], edges=(1, 3))], 151, nrefs_mod=2),
    _spec("len_mod256_255", _S, "pieces", [_t(6, 4351, [(64, 3000)])], 152, nrefs_mod=3),
    # exact for the two-level geometry: no side list there, a capacity exceeded refuses the keys
    _spec("tl_bucket_4096", _S, "two_level", [_t(4, 4096, _FIVE)], 161),
    _spec("tl_bucket_4097", _S, "two_level", [_t(4, 4097, _FIVE)], 162),
    _spec("tl_slot_1024", _S, "two_level", [_t(6, 3000, [(777, 1024)], slot_count=1024)], 163),
    _spec("tl_slot_1025", _S, "two_level", [_t(6, 3000, [(777, 1025)], slot_count=1025)], 164),
]}
REGION_CASE = "tl_region"
REGION_H, REGION_GEOMETRY = 20_000, {"pieces": (2, 6), "two_level": (3, 3)}
NAMES = tuple(SPECS) + (REGION_CASE,)
# the neighbours of the "nothing left behind" test: (spilled, not spilled)
NEIGHBOURS = ("fill5_4097", "fill5_4096")


class Case:
    def __init__(self, name, geometry_, stated, values, offsets, targets, hot, rows, absent, nrefs_mod):
        self.name, self.geometry, self.stated = name, geometry_, stated
        self.values, self.offsets = values, offsets
        self.targets = targets      # [{bucket, count, slot, slot_count, lo, hi, extras {holders: hash}, first, last}]
        self.hot = hot              # [(hash, [holder sketches])]
        self.rows = rows            # sketches whose pairwise rows are compared one by one
        self.absent = absent        # hashes no sketch holds, in a hot hash's bucket or slot
        self.nrefs_mod = nrefs_mod
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
        return db_max_hash(self.values, self.offsets)

    def sketch(self, j):
        return self.values[int(self.offsets[j]):int(self.offsets[j + 1])]

    def expected(self, handle, path):
        return expected_outcome(self.values, self.offsets, handle, path)

    def sample(self):
        """The sample the sorting handles answer: every hot hash; the smallest and largest key of each target and its 1-, 2-,
        5- and 9-holder hashes; the last hash in front of a target and the first behind it; hashes of a hot hash's bucket or
        slot that no sketch holds; a few hundred hashes of the database and as many of none."""
        rng = np.random.default_rng(len(self.name) + self.H)
        sv = np.unique(self.values)
        parts = [np.array([h for h, _ in self.hot], np.uint64), np.array(self.absent, np.uint64)]
        for t in self.targets:
            inside = sv[(sv >= np.uint64(t["lo"])) & (sv < np.uint64(t["hi"]))]
            parts.append(np.array([int(inside[0]), int(inside[-1])] + [t["extras"][k] for k in (1, 2, 5, 9)], np.uint64))
            below, above = sv[sv < np.uint64(t["lo"])], sv[sv >= np.uint64(t["hi"])]
            parts.append(np.array(([int(below[-1])] if below.size else []) + ([int(above[0])] if above.size else []), np.uint64))
        parts.append(self.values[rng.integers(0, self.H, 300)])
        parts.append(rng.integers(1, MAX_HASH, size=300, dtype=np.uint64))
        return np.unique(np.concatenate(parts))


def _sizes(total):
    """Background sketch sizes that add up to `total`."""
    out, i = [], 0
    while total > 0:
        s = min(_BG_SIZES[i % len(_BG_SIZES)], total)
        out.append(s)
        total -= s
        i += 1
    return out


class _Pool:
    """Fresh hashes: uniform below max_hash, outside the targets' key ranges, never twice."""
    def __init__(self, rng, excl, hi=MAX_HASH):
        self.rng, self.excl, self.used, self.hi = rng, excl, set(), hi

    def take(self, n, lo=1000, hi=None, ok=None):
        got = []
        hi = self.hi if hi is None else hi
        while len(got) < n:
            for x in self.rng.integers(lo, hi, size=max(2 * (n - len(got)), 16), dtype=np.uint64):
                x = int(x)
                if x in self.used or (ok is None and any(a <= x < b for a, b in self.excl)) or (ok is not None and not ok(x)):
                    continue
                self.used.add(x)
                got.append(x)
                if len(got) == n:
                    break
        return got


def _background(rng, pool, sizes, crown):
    """Sketches of the given sizes; every fourth of ten hashes or more shares most of its hashes with the one in front (pairs
    that pass a containment threshold of 0.5); the first of the largest ends in max_hash when `crown`."""
    out, prev = [], None
    for i, s in enumerate(sizes):
        if prev is not None and s >= 10 and i % 4 == 3 and len(prev) >= s:
            keep = [prev[k] for k in sorted(rng.choice(len(prev), size=(3 * s) // 4, replace=False))]
            sk = sorted(keep + pool.take(s - len(keep)))
        else:
            sk = sorted(pool.take(s))
        if s >= 10:
            prev = sk
        out.append(sk)
    if crown:
        j = int(np.argmax([len(s) for s in out]))
        out[j][-1] = MAX_HASH
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    if name == REGION_CASE:
        return _region_case()
    spec = SPECS[name]
    rng = np.random.default_rng(spec["seed"])
    own = spec["geometry"]
    NB = spec[own][0] * spec[own][1]
    mh = MAX_HASH
    targets = []
    for t in spec["targets"]:
        b = NB - 1 if t["bucket"] == "last" else t["bucket"]
        lo, hi = bucket_range(b, NB, mh)
        targets.append(dict(t, bucket=b, lo=lo, hi=hi, extras={}, placed=0, reserved=set(), slot=None))
    pool = _Pool(rng, [(t["lo"], t["hi"]) for t in targets])
    in_target = lambda t, avoid: (lambda x: t["lo"] <= x < t["hi"] and slot_of(x, NB, mh) not in avoid)
    # ---- what every holder sketch must hold: reqs[k] = (tag, [target hashes]) ---------------------------------------------------
    reqs, hot, absent = [], [], []
    has_max = False
    for ti, t in enumerate(targets):
        first_hot = None
        for slot, m in t["hot"]:
            if slot == "first":
                h = 7
            elif slot == "max":
                h, has_max = mh, True
            elif slot == "twin":
                h = hot[-1][0] + 1
            else:
                a, b = fine_lo((t["bucket"] << BKT_SLOT_BITS) + slot, NB, mh), fine_lo((t["bucket"] << BKT_SLOT_BITS) + slot + 1, NB, mh)
                h = a + (b - a) // 2
            assert t["lo"] <= h < t["hi"] and h not in pool.used
            pool.used.add(h)
            s = slot_of(h, NB, mh)
            t["reserved"].add(s)
            if first_hot is None:
                first_hot, t["slot"] = h, s
            tag = f"hot{len(hot)}"
            hot.append((h, tag))
            for k in range(m):
                reqs.append([tag + ("bare" if k < 2 else ""), [h]])
            t["placed"] += m
            # hashes nobody holds: the hot hash's neighbour in its slot, and one of its bucket
            a, b = fine_lo((t["bucket"] << BKT_SLOT_BITS) + s, NB, mh), min(fine_lo((t["bucket"] << BKT_SLOT_BITS) + s + 1, NB, mh), mh + 1)
            for x in (h + 2, h - 2):
                if a <= x < b and x not in pool.used:
                    pool.used.add(x)
                    absent.append(x)
                    break
        absent += pool.take(1, t["lo"], t["hi"], ok=in_target(t, t["reserved"]))
        if t["slot_count"] is not None:   # further hashes of the hot slot, up to its exact count
            a, b = fine_lo((t["bucket"] << BKT_SLOT_BITS) + t["slot"], NB, mh), fine_lo((t["bucket"] << BKT_SLOT_BITS) + t["slot"] + 1, NB, mh)
            assert t["hot"][0][1] + sum(t["others"]) == t["slot_count"]
            for q, k in enumerate(t["others"]):
                x = pool.take(1, a, b, ok=lambda v: True)[0]
                reqs += [[f"t{ti}o{q}", [x]] for _ in range(k)]
                t["placed"] += k
        # the bucket's smallest and largest key (unless a hot hash is that key) and hashes with 1, 2, 3, 4, 5 and 9 holders
        extras = [(f"t{ti}x{k}", k, None) for k in EXTRA_HOLDERS]
        if t["edges"][0]:
            extras.append((f"t{ti}first", t["edges"][0], t["lo"]))
        if t["edges"][1]:
            extras.append((f"t{ti}last", t["edges"][1], min(t["hi"], mh + 1) - 1))
        for tag, k, x in extras:
            if x is None:
                x = pool.take(1, t["lo"], t["hi"], ok=in_target(t, t["reserved"]))[0]
                t["extras"][k] = x
            else:
                assert x not in pool.used and slot_of(x, NB, mh) not in t["reserved"]
                pool.used.add(x)
            reqs += [[tag, [x]] for _ in range(k)]
            t["placed"] += k
    # sketches that hold hot hashes of two targets / both twins: merged holders (the pair counts stay)
    def merge(tag_a, tag_b, n):
        a = [r for r in reqs if r[0] == tag_a][-n:]
        b = [r for r in reqs if r[0] == tag_b][-n:]
        for ra, rb in zip(a, b):
            ra[1] = sorted(ra[1] + rb[1])
            ra[0] = tag_a + "+" + tag_b
            reqs.remove(rb)
    if spec["cross"]:
        merge("hot0", "hot1", spec["cross"])
    if any(s == "twin" for t in targets for s, _ in t["hot"]):
        merge("hot0", "hot1", 10)
    # ---- the walk of k_spill_collect: sketches of 513 and 1 025 hashes across two adjacent targets, marked-bucket hashes at
    # positions 0, 511, 512 and last (a round of loads is 64 x 8 elements)
    walks = []
    if any(t["walk"] for t in targets):
        ta, tb = targets
        assert ta["walk"] and tb["walk"] and tb["bucket"] == ta["bucket"] + 1
        for size in (513, 1025):
            lo_part = sorted(pool.take(512, ta["lo"], ta["hi"], ok=in_target(ta, ta["reserved"])))
            hi_part = sorted(pool.take(size - 512, tb["lo"], tb["hi"], ok=in_target(tb, tb["reserved"])))
            ta["placed"] += 512
            tb["placed"] += size - 512
            walks.append((f"walk{size}", lo_part + hi_part))
    # ---- fillers: one-holder hashes that bring every target to its exact count, a few per carrier sketch
    fillers = []
    for ti, t in enumerate(targets):
        need = t["count"] - t["placed"]
        assert need >= 0, (name, ti, need)
        xs = pool.take(need, t["lo"], t["hi"], ok=in_target(t, t["reserved"]))
        k = 0
        while k < need:
            n = 1 + (k % 5)
            fillers.append((f"t{ti}fill", sorted(xs[k:k + n] + pool.take(k % 3))))
            k += n
    # ---- holder sketches: the required hashes + padding from outside the targets, 3 to 6 hashes; "bare": the hash alone
    order = rng.permutation(len(reqs))
    holders = []
    for q, k in enumerate(order):
        tag, need = reqs[k]
        pad = 0 if tag.endswith("bare") else max(3 + q % 4 - len(need), 0)
        holders.append((tag, sorted(need + pool.take(pad))))
    special = sum(len(s) for _, s in holders) + sum(len(s) for _, s in fillers) + sum(len(s) for _, s in walks)
    bg = [("bg", s) for s in _background(rng, pool, _sizes(spec["H"] - special), crown=not has_max)]
    seq = bg[:6]
    for q, hs in enumerate(holders[:-3]):
        seq += [("empty", []), hs, ("empty", [])] if q in (0, 1, 7) else [hs]   # (holders with an empty sketch on either side)
    seq += walks + fillers + bg[6:] + holders[-3:]                             # (the database ends in holders)
    if spec["nrefs_mod"] is not None:
        seq[6:6] = [("empty", [])] * ((spec["nrefs_mod"] - len(seq)) % 4)
    values = np.array([x for _, s in seq for x in s], dtype=np.uint64)
    offsets = np.zeros(len(seq) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) for _, s in seq], dtype=np.uint64)
    tags = [tag for tag, _ in seq]
    where = lambda part: [j for j, tag in enumerate(tags) if part in tag.replace("bare", "").split("+")]
    hot_out = [(h, where(tag)) for h, tag in hot]
    rows = []
    for _, js in hot_out:
        rows += [js[0], js[-1]]
    rows += [where("t0x2")[0], where("t0x9")[0], next(j for j, tag in enumerate(tags) if tag == "bg" and len(seq[j][1]) >= 63)]
    keep = ("bucket", "count", "slot", "slot_count", "lo", "hi", "extras")
    return Case(name, own, {p: spec[p] for p in PATHS}, values, offsets, [{k: t[k] for k in keep} for t in targets], hot_out,
                sorted(set(rows)), absent, spec["nrefs_mod"])


def _region_case():
    """Every hash but one sketch's last element in the lowest first-level region of the two-level sort: the region's count
    exceeds cap1 (flag bit 1), the upper regions hold one pair between them."""
    rng = np.random.default_rng(171)
    p1, p2 = REGION_GEOMETRY["two_level"]
    hi = fine_lo(p2 << BKT_SLOT_BITS, p1 * p2, MAX_HASH)   # the first hash of region 1
    pool = _Pool(rng, [], hi=hi)
    sk = _background(rng, pool, _sizes(REGION_H), crown=True)
    values = np.array([x for s in sk for x in s], dtype=np.uint64)
    offsets = np.zeros(len(sk) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in sk], dtype=np.uint64)
    rows = [j for j, s in enumerate(sk) if len(s) >= 63][:3]
    return Case(REGION_CASE, "two_level", dict(REGION_GEOMETRY), values, offsets, [], [], rows, [], None)
