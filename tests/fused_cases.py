"""Seeded databases and samples for the hit rows of the fused run step (k_step_fused behind run_device_pipelined) at the
edges of their bins, their fill, the tile cap and the growth of their allocation -- and a plain-int mirror of the rules
that decide which of those a sample reaches.  numpy only: nothing here loads the library or the oracle.

The rules, restated from yacht_amd/csrc/yh_query.hip (HR_*, lookup_tile_body, sum_hit_rows, yh_q_step_fused) and
yh_lookup.h (yh_tile_shape_for, yh_hit_slot):

    geometry      below 262 144 hashes 256 lanes x 1 hash (never rows); 262 144 .. 524 287: 1024 lanes x 1 hash; from 524 288:
                  1024 lanes x 2 consecutive stretches of 1024 -- a tile is 256 / 1024 / 2048 CONSECUTIVE sample hashes
    bins          4096 references each; rows only while the references fit 32 bins (N <= 131 072) and the tiles 2048 rows
    row           a count word and up to 63 entries in four sectors of 16 words; the 64th claim takes the dense rows and
                  stamps the set's overflow word
    entries       per (tile, bin): one per distinct reference hit, one more if it was hit on a shared hash -- while every
                  reference the tile hits finds a slot in the tile's hit table of 1024 slots: home slot
                  (ref * 2654435761 mod 2^32) >> 22, two probes (home, home + 1).  Home slots pairwise two or more apart:
                  nobody is displaced (`apart`).  A hit that finds no slot is an entry of its own: with three references
                  on one home slot the count depends on who arrives first, and the mirror only gives its lower bound
    capacity      rows per bin; on first use and whenever a step has more tiles: min(max(round_up_256(tiles), 512), 2048),
                  after draining the pending steps if there was an allocation

Databases (six hashes per reference, below 2^40 like test_gpu_fused_hitrows.edge_database, some references clustered so
that the handle has shared hashes):

    bins32, bins33    131 072 and 131 073 references: exactly 32 bins, and one reference too many
    fill              8200 references (three bins): samples whose tile 0 claims exactly k entries in bin 1
    crowded           the same shape, other seed: samples whose tile 0 hits three and more references on one home slot
"""
import functools

import numpy as np

HR_BIN = 4096
HR_MAX_BINS = 32
HR_SECTOR = 16
HR_ROW = 64
HR_ENTS = HR_ROW - 1
HR_MAX_WGS = 2048
TSLOTS = 1024
PER_REF = 6

FILL_KS = (15, 16, 31, 32, 47, 48, 63, 64)
GROWTH_SIZES = (524_288, 1_048_576, 1_048_577, 4_194_304, 4_194_305)
GROWTH_SEQ = (524_288, 1_048_576, 1_048_577, 1_048_577, 4_194_304, 524_288, 4_194_304)
TILECAP_SEQ = (4_194_304, 4_194_305, 4_194_304, 4_194_305, 1_048_577)

# the value bands of a database's hashes: nearly everything in the low band, nothing in the gap, the `late` references above it
LOW_TOP = (1 << 40) - (1 << 34)
HIGH_LO = (1 << 40) - (1 << 33)


# ---- the rules ---------------------------------------------------------------------------------------------------------
def geometry(n_hashes):
    """(lanes, sample hashes per tile) of the fused launch that looks a sample of n_hashes up"""
    if n_hashes < 262_144:
        return 256, 256
    if n_hashes < 524_288:
        return 1024, 1024
    return 1024, 2048


def n_tiles(n_hashes):
    per = geometry(n_hashes)[1]
    return (n_hashes + per - 1) // per


def n_bins(n_refs):
    return (n_refs + HR_BIN - 1) // HR_BIN


def uses_rows(n_refs, n_hashes):
    return geometry(n_hashes)[0] == 1024 and n_refs <= HR_MAX_BINS * HR_BIN and n_tiles(n_hashes) <= HR_MAX_WGS


def capacity_for(tiles):
    return min(max((tiles + 255) // 256 * 256, 512), HR_MAX_WGS)


def home_slot(ref):
    return ((int(ref) * 2654435761) & 0xFFFFFFFF) >> 22


def apart(ids):
    """every home slot two or more from every other (around the table's end too): each reference gets its home slot"""
    homes = sorted(home_slot(j) for j in ids)
    if len(homes) < 2:
        return True
    gaps = [b - a for a, b in zip(homes, homes[1:])] + [homes[0] + TSLOTS - homes[-1]]
    return min(gaps) >= 2


def pick_apart(candidates, count, taken=()):
    """the first `count` of `candidates` whose home slots are two or more apart from each other's and from those of `taken`"""
    used = set()
    for j in taken:
        used.update(((home_slot(j) + d) % TSLOTS for d in (-1, 0, 1)))
    out = []
    for j in candidates:
        h = home_slot(j)
        if h in used:
            continue
        out.append(int(j))
        used.update(((h + d) % TSLOTS for d in (-1, 0, 1)))
        if len(out) == count:
            return out
    raise AssertionError(f"only {len(out)} of {count} references with home slots apart")


class HandleMirror:
    """The host state of one handle's hit rows: capacity, whether anything is allocated, whether steps are pending."""

    def __init__(self, n_refs):
        self.n_refs, self.cap, self.allocated, self.pending = n_refs, 0, False, False

    def step(self, n_hashes):
        """one run_device_pipelined call: the trace line of its launch (YH_TRACE_HITROWS)"""
        lanes, _per = geometry(n_hashes)
        tiles = n_tiles(n_hashes)
        rows = uses_rows(self.n_refs, n_hashes)
        grew = drained = 0
        if rows and tiles > self.cap:
            grew = 1
            if self.allocated and self.pending:
                drained = 2      # (the reducer and the exclusive pass of the last step, the exclusive pass of the one before)
            self.cap, self.allocated = capacity_for(tiles), True
        self.pending = True
        return (f"[yh hitrows] sample {n_hashes}  lanes {lanes}  tiles {tiles}  refs {self.n_refs}  "
                f"capacity {self.cap}  grew {grew}  drained {drained} -> {'rows' if rows else 'dense'}")

    def join(self):
        self.pending = False


def predict(log):
    """log: ("handle", n_refs) | ("step", n_hashes) | ("join",) in call order -> the trace lines of the lookups' launches"""
    lines, h = [], None
    for entry in log:
        if entry[0] == "handle":
            h = HandleMirror(entry[1])
        elif entry[0] == "step":
            lines.append(h.step(entry[1]))
        else:
            h.join()
    return lines


def parse(line):
    """a trace line -> dict(sample, lanes, tiles, refs, capacity, grew, drained, path)"""
    w = line.split()
    assert w[:2] == ["[yh", "hitrows]"] and w[-2] == "->", line
    return {"sample": int(w[3]), "lanes": int(w[5]), "tiles": int(w[7]), "refs": int(w[9]), "capacity": int(w[11]), "grew": int(w[13]),
            "drained": int(w[15]), "path": w[-1]}


# ---- databases ---------------------------------------------------------------------------------------------------------
class Database:
    """refs: (n, 6) ascending rows.  clusters: lists of ids; the members of one hold the first member's first three hashes."""

    def __init__(self, name, refs, clusters, late=()):
        self.name, self.refs2d, self.clusters, self.late = name, refs, clusters, tuple(late)
        self.n = refs.shape[0]
        flat = refs.ravel()
        order = np.argsort(flat, kind="stable")
        self.hashes = flat[order]                                   # every (hash, holder), by hash
        self.holder = (np.arange(flat.size) // PER_REF)[order]
        self.held = np.unique(flat)
        self.top = int(self.held[-1])

    @property
    def refs(self):
        return list(self.refs2d)

    def packed(self):
        return self.refs2d.ravel().copy(), np.arange(self.n + 1, dtype=np.uint64) * np.uint64(PER_REF)

    def core(self, ids):
        return np.unique(self.refs2d[np.asarray(sorted(ids), dtype=np.int64)].ravel())

    def clustered(self):
        return sorted(j for c in self.clusters for j in c)


def _database(name, n, seed, clusters, late=()):
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(1, LOW_TOP, size=PER_REF * n + 8192, dtype=np.uint64))
    assert pool.size >= PER_REF * n
    refs = rng.permutation(pool)[:PER_REF * n].reshape(n, PER_REF)      # (over the whole band)
    if late:
        hi = np.unique(rng.integers(HIGH_LO, 1 << 40, size=PER_REF * len(late) + 64, dtype=np.uint64))
        refs[np.asarray(late)] = rng.permutation(hi[:PER_REF * len(late)]).reshape(len(late), PER_REF)
    for c in clusters:
        for j in c[1:]:
            refs[j, :3] = refs[c[0], :3]
    refs = np.sort(refs, axis=1)
    assert all(np.unique(r).size == PER_REF for r in refs[np.asarray(sorted({j for c in clusters for j in c}), dtype=np.int64)])
    return Database(name, refs, [list(c) for c in clusters], late)


@functools.lru_cache(maxsize=None)
def bins_database(n):
    """131 072 or 131 073 references.  Clusters: 4092 .. 4099 (bins 0 | 1), 131 060 .. 131 067 (the last quarter of bin 31), and pairs
    across the edges 15 | 16 and 30 | 31."""
    assert n in (HR_MAX_BINS * HR_BIN, HR_MAX_BINS * HR_BIN + 1)
    clusters = [list(range(4092, 4100)), list(range(131_060, 131_068)), [16 * HR_BIN - 1, 16 * HR_BIN], [31 * HR_BIN - 2, 31 * HR_BIN + 1]]
    return _database(f"bins{n_bins(n)}", n, 3200 + n, clusters)


def bins_ids(db):
    """corners: first and last reference of bins 0, 1, 2, 3, 15, 16, 30, 31, one in every quarter of bins 3 and 31, the clusters,
    the database's last reference.  quarters: one reference in each 1024-reference quarter of every bin, home slots apart, the
    last reference of bin 31 among them (and the database's last where that is another)."""
    corners = set()
    for b in (0, 1, 2, 3, 15, 16, 30, 31):
        corners.update((b * HR_BIN, b * HR_BIN + HR_BIN - 1))
    for b in (3, 31):
        corners.update(b * HR_BIN + q * 1024 + 511 for q in range(4))
    corners.update(db.clustered())
    corners.add(db.n - 1)
    quarters = [HR_MAX_BINS * HR_BIN - 1] + ([db.n - 1] if db.n > HR_MAX_BINS * HR_BIN else [])
    assert apart(quarters)
    for b in range(HR_MAX_BINS):
        for q in range(4):
            if (b, q) == (HR_MAX_BINS - 1, 3):
                continue
            lo = b * HR_BIN + q * 1024
            # (the candidates walk the quarter from a different place in each, so the reducer's lanes differ too)
            cand = [lo + (37 * (4 * b + q) + i) % 1024 for i in range(1024)]
            quarters += pick_apart([j for j in cand if j not in corners], 1, taken=quarters)
    return sorted(corners), sorted(quarters)


def small_database(name):
    """8200 references: three bins, the last of eight references.  Bin 1 holds everything the fill samples hit in tile 0:

        singles     64 references nobody shares a hash with, home slots apart
        pairs       15 clusters of two inside bin 1, two clusters of a bin-1 reference and a bin-0 partner, and one more
                    single reference: home slots apart among all of them
        late        five references of bin 0 and three of bin 2 whose hashes lie above everybody else's: in a sample they
                    come behind everything else, so a sample can put them into its SECOND tile
        crowd       references of bin 1 on one home slot: four on one, four on the next slot but one, two of those a cluster
    """
    n = 8200
    edge = list(range(4092, 4100))
    late = pick_apart(range(100, 4000, 37), 5)
    late += pick_apart(range(8192, n), 3, taken=late)      # (all eight apart from each other: they share tile 1)
    by_home = {}
    for j in range(4100, 8192):
        by_home.setdefault(home_slot(j), []).append(j)
    h0 = min(h for h in by_home if len(by_home[h]) >= 4 and len(by_home.get(h + 2, ())) >= 4)
    crowd = by_home[h0][:4] + by_home[h0 + 2][:4]
    inner = pick_apart([j for j in range(5000, 6000) if j not in crowd], 33)
    partners = pick_apart(range(1000, 2000), 2, taken=inner)
    pairs = [[inner[2 * i], inner[2 * i + 1]] for i in range(15)] + [[inner[30], partners[0]], [inner[31], partners[1]]]
    lone = inner[32]
    used = set(edge) | set(late) | set(inner) | set(partners) | set(crowd)
    singles = pick_apart([j for j in range(6000, 8192) if j not in used], 64)
    clusters = [edge] + pairs + [crowd[4:6]]
    db = _database(name, n, {"fill": 4100, "crowded": 4200}[name], clusters, late)
    db.singles, db.pairs, db.lone, db.crowd = singles, pairs, lone, crowd
    return db


@functools.lru_cache(maxsize=None)
def fill_database():
    return small_database("fill")


@functools.lru_cache(maxsize=None)
def crowded_database():
    return small_database("crowded")


# ---- samples -----------------------------------------------------------------------------------------------------------
def above(db, count, start=1):
    """`count` hashes above everything the database holds (nobody holds them, the lookup drops them unread)"""
    return np.uint64(db.top) + np.arange(start, start + count, dtype=np.uint64) * np.uint64(977)


def exact(db, ids, size):
    """the references `ids` whole, then hashes above the database's: every hit in the first tile(s)"""
    core = db.core(ids)
    assert core.size <= size
    return np.concatenate([core, above(db, size - core.size)])


def two_tiles(db, first, second, size):
    """tile 0: `first` whole and hashes of the gap nobody holds; tile 1 begins with the `late` references `second`"""
    per = geometry(size)[1]
    a, b = db.core(first), db.core(second)
    assert a.size <= per and int(a[-1]) < LOW_TOP and int(b[0]) >= HIGH_LO and set(second) <= set(db.late)
    gap = np.uint64(LOW_TOP) + np.arange(per - a.size, dtype=np.uint64) * np.uint64(1009)
    assert gap.size == 0 or int(gap[-1]) < HIGH_LO
    out = np.concatenate([a, gap, b, above(db, size - per - b.size)])
    assert out.size == size and bool((np.diff(out.astype(np.int64)) > 0).all())
    return out


def spread(db, ids, size):
    """the references `ids` whole among hashes nobody holds, evenly over the database's low band: exactly `size` ascending
    distinct hashes, and tiles beyond the first have hits"""
    core = db.core(ids)
    grid = np.arange(size, dtype=np.uint64) * np.uint64(LOW_TOP // size) + np.uint64(1)
    pos = np.searchsorted(db.held, grid)
    grid = grid[db.held[np.minimum(pos, db.held.size - 1)] != grid]
    assert grid.size >= size - core.size
    pad = grid[np.linspace(0, grid.size - 1, size - core.size).astype(np.int64)]
    out = np.sort(np.concatenate([core, pad]))
    assert out.size == size and bool((out[1:] > out[:-1]).all())
    return out


def bins_samples(db):
    corners, quarters = bins_ids(db)
    return {"quarters@262144": exact(db, quarters, 262_144), "quarters@524288": exact(db, quarters, 524_288),
            "corners@262144": spread(db, corners, 262_144), "corners@524288": spread(db, corners, 524_288),
            "corners@30000": exact(db, corners, 30_000), "quarters@30000": exact(db, quarters, 30_000)}


BINS_SEQ = ("quarters@524288", "corners@30000", "quarters@262144", "quarters@30000", "corners@524288", "corners@30000",
            "corners@262144", "quarters@524288", "quarters@262144", "corners@524288")


def fill_ids(db):
    """label -> (references of tile 0, references of tile 1)"""
    whole = [j for p in db.pairs[:15] for j in p]
    out = {f"single{k}": (db.singles[:k], list(db.late)) for k in FILL_KS}
    out["pairs64"] = (whole + [db.pairs[15][0], db.pairs[16][0]], list(db.late[:5]))
    out["pairs63"] = (whole + [db.pairs[15][0], db.lone], list(db.late[5:]))
    return out


def fill_samples(db):
    out = {f"{label}@524288": two_tiles(db, a, b, 524_288) for label, (a, b) in fill_ids(db).items()}
    for label in ("single16", "single48", "single64", "pairs64"):      # the tiles of one hash per lane too
        a, b = fill_ids(db)[label]
        out[f"{label}@262144"] = two_tiles(db, a, b, 262_144)
    return out


# step i writes the counter set i & 1: what a row holds beyond its count is the step's two calls earlier.  First half: that
# step had MORE entries (stale entries behind the count), second half: fewer.  single64 and pairs64 stamp the overflow
# word of their set; the step two calls later does not, and the other way round.
FILL_SEQ = tuple(f"{s}@524288" for s in ("single64", "pairs64", "single63", "pairs63", "single48", "single47", "single32", "single31",
                                         "single16", "single15", "single64", "single15", "pairs64", "single16", "pairs63", "single31",
                                         "single32", "single47", "single48", "single63", "single64")) + \
    ("single64@262144", "single48@262144", "pairs64@262144", "single16@262144", "single64@262144", "pairs64@524288")


def crowded_ids(db):
    """crowd3: three references on one home slot.  crowd8: four on one slot and four on the next but one, two of them a cluster (a
    hit on a shared hash without a slot is two entries).  crowd_full: 60 single references and the eight -- the row fills
    through entries of single hits."""
    return {"crowd3": (db.crowd[:3], list(db.late)), "crowd8": (db.crowd, list(db.late[:5])),
            "crowd_full": (db.singles[:60] + db.crowd, list(db.late[5:])), "single16": (db.singles[:16], list(db.late))}


def crowded_samples(db):
    out = {f"{label}@524288": two_tiles(db, a, b, 524_288) for label, (a, b) in crowded_ids(db).items()}
    for label in ("crowd8", "crowd_full"):
        a, b = crowded_ids(db)[label]
        out[f"{label}@262144"] = two_tiles(db, a, b, 262_144)
    return out


CROWDED_SEQ = ("crowd_full@524288", "crowd8@524288", "crowd3@524288", "single16@524288", "crowd_full@524288", "crowd3@524288",
               "crowd8@262144", "crowd_full@262144", "single16@524288", "crowd8@524288", "crowd_full@262144", "crowd_full@524288")


def growth_ids(db, size):
    """about sixteen hits per tile, evenly over the references, and the holder of the database's largest hash: the last tile -- of
    ONE hash at 1 048 577 and 4 194 305 -- has a hit"""
    n_ids = min(db.n, n_tiles(size) * 16 // PER_REF)
    ids = set(np.linspace(0, db.n - 1, n_ids).astype(np.int64).tolist())
    ids.add(int(db.holder[-1]))
    return sorted(ids)


@functools.lru_cache(maxsize=None)
def growth_samples():
    """on `fill`: label -> sample of exactly 524 288, 1 048 576, 1 048 577, 4 194 304, 4 194 305 hashes, and one of 30 000"""
    db = fill_database()
    out = {f"spread@{s}": spread(db, growth_ids(db, s), s) for s in GROWTH_SIZES}
    out["small@30000"] = exact(db, db.clustered() + list(db.late), 30_000)
    return out


# ---- the mirror of one step -------------------------------------------------------------------------------------------
class Step:
    """What the lookup of one sample leaves: per (tile, bin) the entries claimed, per reference its hits.

    claimed[t, b] is exact where exact[t] -- the home slots of the references tile t hits are apart -- and a lower bound elsewhere
    (a hit without a slot is an entry of its own).  A (tile, bin) overflows when it claims more than 63."""

    def __init__(self, db, sample):
        sample = np.asarray(sample, dtype=np.uint64)
        self.lanes, self.per = geometry(sample.size)
        self.tiles = n_tiles(sample.size)
        self.rows = uses_rows(db.n, sample.size)
        lo, hi = np.searchsorted(db.hashes, sample, "left"), np.searchsorted(db.hashes, sample, "right")
        at = np.flatnonzero(hi > lo)
        cnt = (hi - lo)[at]
        pos = np.repeat(at, cnt)                                             # one row per (sample hash, holder)
        ref = db.holder[np.repeat(lo[at], cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))]
        shared = np.repeat(cnt > 1, cnt)
        tile = pos // self.per
        self.hits = np.bincount(ref, minlength=db.n).astype(np.uint32)
        first = np.unique(tile * db.n + ref)                                 # (tile, reference) hit at all
        second = np.unique((tile * db.n + ref)[shared])                      # ... and hit on a shared hash
        self.claimed = np.zeros((self.tiles, n_bins(db.n)), dtype=np.int64)
        for keys in (first, second):
            np.add.at(self.claimed, (keys // db.n, (keys % db.n) // HR_BIN), 1)
        self.tile_refs = {}
        for key in first.tolist():
            self.tile_refs.setdefault(key // db.n, []).append(key % db.n)
        self.exact = {t: apart(ids) for t, ids in self.tile_refs.items()}

    def overflowing(self):
        return [(int(t), int(b)) for t, b in zip(*np.nonzero(self.claimed > HR_ENTS))]

    def sectors_read(self, t, b):
        """sectors of row (t, b) the reducer reads: the first always, the others by the count the lookup stored"""
        c = min(int(self.claimed[t, b]), HR_ENTS)
        return 1 + (c >= HR_SECTOR) * (1 + (c >= 2 * HR_SECTOR) + (c >= 3 * HR_SECTOR))
