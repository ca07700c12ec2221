"""Databases and samples on the edges of the streaming lookup (k_stream_lookup, yh_query.hip), numpy and plain ints only.

Never calls the library.  A database is a list of (hash, reference) pairs in hash order; next to it stands a mirror of what
build_stream / k_stream_scatter (yh_build.hip) make of it -- the shift, the fillers, every pair's position, the block headers,
the padding -- and of the launch geometry of yh_q_overlap_stream and the kernel: workgroups, blocks per workgroup, blocks per
super-block, wg_key, every workgroup's sample range (wave_bound) and its tiles.  For any stream position the mirror says which
byte, lane, block, group, super-block, wave and workgroup it falls in, so a case can say -- and tests/test_stream_cases_cpu.py
can assert -- which boundary it sits on.  tests/test_gpu_stream_edges.py runs the kernel on the cases.

Most cases are LADDERS: consecutive distinct hashes `gap` apart, which gives truncated gaps of 1 (gap = 1, shift 0) or 40
(gap = 40 << s, shift s) and no fillers, so that a pair's position is its index.  A RUN is one hash held by m references: m
consecutive elements of equal key.
"""
import functools

import numpy as np

M64 = (1 << 64) - 1
STREAM_BLOCK = 1024         # elements per block (yh_common.h)
LANE = 16                   # elements (delta bytes) per lane
PF = 4                      # YH_STREAM_PF: blocks per group
NB = 16                     # STREAM_NB: blocks per full super-block
WAVES = 8                   # STREAM_THREADS / 64
ST_SLOTS = 6144             # YH_ST_SLOTS
ST_PAD = 66
ST_CAP = ST_SLOTS - ST_PAD  # sample keys per tile
STREAM_WQ = 64              # candidates a wave queues per round
TBITS = 9                   # YH_STREAM_TBITS: the workgroup's hit table
TSLOTS = 1 << TBITS
TPROBES = 2                 # YH_STREAM_TPROBES
WGS_DEFAULT = 512
OFFSET_MAX = 0xfffffffe     # largest staged 32-bit key offset; 0xffffffff is the sentinel

assert ST_CAP == 6078


# ---- the layout ---------------------------------------------------------------------------------------------------------------
class Layout:
    """What build_stream makes of the sorted pairs (only the hashes matter)."""

    def __init__(self, hashes):
        h = np.asarray(hashes, dtype=np.uint64)
        assert h.size and np.all(h[1:] >= h[:-1])
        self.H = int(h.size)
        self.max_hash = int(h[-1])
        s = 0
        while s < 32 and ((self.max_hash >> (s + 1)) // self.H) >= 32:
            s += 1
        self.sshift = s
        self.t = h >> np.uint64(s)
        d = np.diff(self.t)
        self.nfill = np.concatenate([[0], (np.maximum(d, 1) - 1) // 255]).astype(np.int64)    # fillers in front of element i
        self.pos = np.arange(self.H, dtype=np.int64) + np.cumsum(self.nfill)
        self.L = int(self.pos[-1]) + 1
        self.slen = (self.L + STREAM_BLOCK - 1) // STREAM_BLOCK * STREAM_BLOCK
        self.nblk = self.slen // STREAM_BLOCK
        self.n_fillers = int(self.nfill.sum())
        self.n_padding = self.slen - self.L
        self.max_key = self.max_hash >> s
        self.stream_bytes = self.slen + (self.nblk + 1) * 8          # yh_db_get_info

    def _at(self, p):
        assert 0 <= p < self.slen
        i = int(np.searchsorted(self.pos, p, side="right")) - 1
        return i, p - int(self.pos[i])

    def kind_at(self, p):
        """'real', 'filler' or 'pad' (the padding elements behind the last pair: delta 0, no reference)."""
        i, f = self._at(p)
        return "real" if f == 0 else ("pad" if i == self.H - 1 else "filler")

    def key_at(self, p):
        i, f = self._at(p)
        if f == 0 or i == self.H - 1:
            return int(self.t[i])
        return int(self.t[i]) + 255 * f          # filler f of the gap behind element i

    def delta_at(self, p):
        """The byte k_stream_scatter writes (a block's first byte is written too, and not read)."""
        return 0 if p == 0 else self.key_at(p) - self.key_at(p - 1)

    def hdr(self, b):
        """Key of block b's first element; all ones from nblk on."""
        return self.key_at(b * STREAM_BLOCK) if b < self.nblk else M64

    def filler_positions(self):
        out = []
        for i in np.flatnonzero(self.nfill):
            out += list(range(int(self.pos[i]) - int(self.nfill[i]), int(self.pos[i])))
        return out


def nb_for(n_blocks):
    """Blocks per super-block of a tile that covers n_blocks."""
    return NB if n_blocks >= 2 * WAVES * NB else min(PF, max(n_blocks // WAVES, 1))


def supers_per_wave(n_blocks):
    nb = nb_for(n_blocks)
    n_super = (n_blocks + nb - 1) // nb
    return [len(range(w, n_super, WAVES)) for w in range(WAVES)]


class Tile:
    def __init__(self, sub, n, klo, khi, bl0, bl1, single):
        self.sub, self.n, self.klo, self.khi, self.bl0, self.bl1, self.single = sub, n, klo, khi, bl0, bl1, single
        self.nb = nb_for(bl1 - bl0)

    def __repr__(self):
        return f"Tile(sub={self.sub}, n={self.n}, keys={self.klo}..{self.khi}, blocks={self.bl0}..{self.bl1}, nb={self.nb})"


class Geometry:
    """The launch of yh_q_overlap_stream for a layout under YH_STREAM_WGS = wgs_env.  last = "max": the last wg_key is the
    stream's largest key (what k_wg_key writes); "ones": all ones, as it was before."""

    def __init__(self, layout, wgs_env=WGS_DEFAULT, last="max"):
        self.lay = layout
        nblk = layout.nblk
        self.wgs = min(wgs_env, max(nblk // 2, 1))
        self.per = (nblk + self.wgs - 1) // self.wgs
        end = layout.max_key if last == "max" else M64
        self.wg_key = [layout.hdr(w * self.per) if w * self.per < nblk else end for w in range(self.wgs + 1)]

    def blocks(self, w):
        b0 = min(w * self.per, self.lay.nblk)
        return b0, min(self.lay.nblk, b0 + self.per)

    def n_ranges(self):
        return sum(1 for w in range(self.wgs) if self.blocks(w)[0] < self.blocks(w)[1])

    def nb(self, w):
        b0, b1 = self.blocks(w)
        return nb_for(b1 - b0)

    def where(self, p):
        """Where position p falls when its workgroup's sample range is one tile."""
        block = p // STREAM_BLOCK
        w = block // self.per
        b0, b1 = self.blocks(w)
        nb = nb_for(b1 - b0)
        local = block - b0
        sup = local // nb
        return {"byte": p % LANE, "lane": p % STREAM_BLOCK // LANE, "elem": p % STREAM_BLOCK, "block": block, "wg": w,
                "local": local, "nb": nb, "super": sup, "in_super": local % nb, "group": local % nb // PF,
                "nvalid": min(nb, b1 - b0 - sup * nb), "wave": sup % WAVES, "last_of_wg": block == b1 - 1}

    # -- the sample side
    def sample_range(self, w, keys):
        """[s0, s1) of wave_bound: wg_key[w] <= key <= wg_key[w + 1]; keys = the sample's truncated keys, ascending."""
        keys = np.asarray(keys, dtype=np.uint64)
        return (int(np.searchsorted(keys, np.uint64(self.wg_key[w]), side="left")),
                int(np.searchsorted(keys, np.uint64(self.wg_key[w + 1]), side="right")))

    def keys_of(self, sample):
        return np.asarray(sample, dtype=np.uint64) >> np.uint64(self.lay.sshift)

    def tiles(self, w, sample):
        """The tiles workgroup w makes of the sample, as the kernel's loop over `sub` does."""
        keys = self.keys_of(sample)
        s0, s1 = self.sample_range(w, keys)
        b0, b1 = self.blocks(w)
        out = []
        if b0 >= b1:
            return out
        sub = s0
        while sub < s1:
            n = min(ST_CAP, s1 - sub)
            klo = int(keys[sub])
            far = np.flatnonzero(keys[sub: sub + n] - np.uint64(klo) > np.uint64(OFFSET_MAX))
            if far.size:
                n = int(far[0])
            khi = int(keys[sub + n - 1])
            single = sub == s0 and n == s1 - s0
            bl0, bl1 = b0, b1
            if not single:
                lo, hi = b0, b1
                while lo < hi:
                    mid = (lo + hi) >> 1
                    if self.lay.hdr(mid + 1) < klo:
                        lo = mid + 1
                    else:
                        hi = mid
                bl0 = lo
                hi = b1
                while lo < hi:
                    mid = (lo + hi) >> 1
                    if self.lay.hdr(mid) <= khi:
                        lo = mid + 1
                    else:
                        hi = mid
                bl1 = lo
            out.append(Tile(sub, n, klo, khi, bl0, bl1, single))
            sub += n
        return out

    def all_tiles(self, sample):
        return [t for w in range(self.wgs) for t in self.tiles(w, sample)]


def table_home(ref):
    return ((ref * 2654435761) & 0xffffffff) >> (32 - TBITS)


def table_must_overflow(refs):
    """table_add: a reference sits in its home slot or the next one.  True when no order of arrival fits all of them: more
    references than slots, or more than two with one home (sufficient, not necessary)."""
    refs = sorted(set(int(r) for r in refs))
    if len(refs) > TSLOTS:
        return True
    homes = np.bincount([table_home(r) for r in refs], minlength=TSLOTS)
    return bool(homes.max() > TPROBES)


def run_states(geom, start, m):
    """What a run of m equal keys from position `start` on reaches in stream_blocks under this geometry (one tile)."""
    a = geom.where(start)
    st = set()
    if a["byte"] == LANE - 1:
        st.add("starts_last_byte_of_lane")
        if a["lane"] == 63:
            st.add("starts_last_byte_of_block")
            if a["in_super"] % PF == PF - 1 and a["nb"] >= PF:
                st.add("starts_last_of_group")
            if a["in_super"] == a["nvalid"] - 1:
                st.add("starts_last_of_superblock")
            if a["last_of_wg"]:
                st.add("starts_last_of_workgroup")
    if a["elem"] == 0:
        st.add("starts_block")
        if a["in_super"] == 0:
            st.add("starts_superblock")
    per_super = {}
    for p0 in range(start - start % LANE, start + m, LANE):       # every lane the run touches
        q = max(p0, start)
        x = geom.where(q)
        per_super[(x["wg"], x["super"])] = per_super.get((x["wg"], x["super"]), 0) + min(p0 + LANE, start + m) - q
        if q == start:
            continue
        y = geom.where(q - 1)
        if y["block"] == x["block"]:
            st.add("next_lane")                 # t < 63 -> ++t
        elif y["wg"] != x["wg"]:
            st.add("next_workgroup")            # t <= wg_key[w + 1] there, t >= wg_key[w] here
        elif y["super"] != x["super"]:
            st.add("next_superblock")           # "the next super-block finds it itself"
        else:
            st.add("next_block")                # ++f < NB -> locate()
            if y["group"] != x["group"]:
                st.add("next_group")
    if max(per_super.values()) > STREAM_WQ:
        st.add("queue_full")                    # one lane pushes more than STREAM_WQ candidates in a round
    if table_must_overflow(range(m)):
        st.add("table_crowded")
    st.add(f"blocks_{(start + m - 1) // STREAM_BLOCK - start // STREAM_BLOCK + 1}")
    return st


# ---- a case -------------------------------------------------------------------------------------------------------------------
class Case:
    """One database -- the pairs in hash order -- and its samples (label -> ascending distinct hashes)."""

    def __init__(self, name, hashes, refs, n_refs, envs):
        self.name = name
        self.hashes = np.ascontiguousarray(hashes, dtype=np.uint64)
        self.refs = np.ascontiguousarray(refs, dtype=np.int64)
        self.n_refs = int(n_refs)
        self.envs = tuple(envs)             # the environments of test_gpu_stream_edges.py that run it
        self.samples = {}
        self.notes = {}
        assert self.hashes.size == self.refs.size and self.refs.max() < self.n_refs
        for a in (self.hashes, self.refs):
            a.setflags(write=False)

    def add(self, label, sample):
        s = np.unique(np.asarray(sample, dtype=np.uint64))
        s.setflags(write=False)
        assert label not in self.samples and s.size
        self.samples[label] = s

    @functools.lru_cache(maxsize=None)
    def layout(self):
        return Layout(self.hashes)

    def geometry(self, wgs_env=WGS_DEFAULT, last="max"):
        return Geometry(self.layout(), wgs_env, last)

    @functools.lru_cache(maxsize=None)
    def csr(self):
        order = np.lexsort((self.hashes, self.refs))
        values = np.ascontiguousarray(self.hashes[order])
        offsets = np.zeros(self.n_refs + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum(np.bincount(self.refs, minlength=self.n_refs)).astype(np.uint64)
        values.setflags(write=False)
        offsets.setflags(write=False)
        return values, offsets

    @functools.lru_cache(maxsize=None)
    def table(self):
        """hash -> holders, from the pairs."""
        out = {}
        for h, r in zip(self.hashes.tolist(), self.refs.tolist()):
            out.setdefault(h, []).append(r)
        return out

    def hash_at(self, p):
        """The hash of the pair at stream position p (a real element)."""
        lay = self.layout()
        i, f = lay._at(p)
        assert f == 0
        return int(self.hashes[i])


def ladder(name, length, envs, runs=(), n_refs=8, base=1000, gap=1):
    """`length` pairs: distinct hashes base, base + gap, ... one holder each (reference = its number mod n_refs), except that
    the element at position `start` of every (start, m) in runs is a hash held by references 0 .. m - 1.  Without fillers
    (the mirror is asked) positions are indices."""
    mult, p = [], 0
    for start, m in sorted(runs):
        assert start >= p + 2 or start == p == 0, "runs need a neighbour between them"
        mult.append(np.ones(start - p, dtype=np.int64))
        mult.append(np.array([m], dtype=np.int64))
        p = start + m
    assert p <= length
    mult.append(np.ones(length - p, dtype=np.int64))
    mult = np.concatenate(mult)
    d = np.repeat(np.arange(mult.size, dtype=np.int64), mult)          # which distinct hash each pair holds
    first = np.repeat(np.cumsum(mult) - mult, mult)
    within = np.arange(length, dtype=np.int64) - first
    refs = np.where(np.repeat(mult, mult) == 1, d % n_refs, within)
    hashes = (np.uint64(base) + d.astype(np.uint64) * np.uint64(gap))
    c = Case(name, hashes, refs, max(n_refs, int(mult.max())), envs)
    c.notes["runs"] = tuple(sorted(runs))
    return c


def _bounds_sample(case):
    """The hashes at the last, first and second element of every block, and every 509th."""
    lay = case.layout()
    ps = set(range(0, lay.L, 509))
    for b in range(lay.nblk + 1):
        ps.update(p for p in (b * STREAM_BLOCK - 1, b * STREAM_BLOCK, b * STREAM_BLOCK + 1) if 0 <= p < lay.L)
    return [case.hash_at(p) for p in sorted(ps) if lay.kind_at(p) == "real"]


def _spread(lo, hi, n):
    """n distinct integers in [lo, hi), evenly spread."""
    assert hi - lo >= n
    return [lo + (hi - lo) * i // n for i in range(n)]


# ---- the environments of the GPU file ----------------------------------------------------------------------------------------
# name -> YH_STREAM_WGS (None: the default 512), YH_NO_FUSED_RUN
ENVS = {"default": (None, False), "wgs1": (1, False), "wgs2": (2, False), "wgs8": (8, False), "wgs9": (9, False),
        "wgs17": (17, False), "wgs19": (19, False), "wgs34": (34, False), "wgs39": (39, False), "no_fused": (None, True)}
ALL_ENVS = tuple(ENVS)
SMALL_ENVS = ("default", "wgs1", "no_fused")     # (a database of three blocks is one workgroup whatever YH_STREAM_WGS says)


def wgs_of(env_name):
    return ENVS[env_name][0] or WGS_DEFAULT


# (database, environment) -> blocks per workgroup, blocks per super-block: the table of block ranges
RANGES = {("ladder272", "default"): (2, 1), ("ladder257", "default"): (3, 1), ("ladder272", "wgs39"): (7, 1),
          ("ladder272", "wgs34"): (8, 1), ("ladder272", "wgs19"): (15, 1), ("ladder272", "wgs17"): (16, 2),
          ("ladder272", "wgs9"): (31, 3), ("ladder256", "wgs8"): (32, 4), ("ladder272", "wgs8"): (34, 4),
          ("ladder272", "wgs2"): (136, 4), ("ladder255", "wgs1"): (255, 4), ("ladder256", "wgs1"): (256, 16),
          ("ladder257", "wgs1"): (257, 16), ("ladder272", "wgs1"): (272, 16)}

# ---- case: 272 blocks with the runs -------------------------------------------------------------------------------------------
B = STREAM_BLOCK
RUNS_272 = (            # (start, m); what each reaches under which environment is asserted in test_stream_cases_cpu.py
    (5 * B + 7 * LANE + 15, 2),     # the last byte of a lane
    (B - 1, 16),                    # the last byte of lane 63 of a block
    (4 * B - 1, 17),                # the last element of a group of 4 blocks
    (16 * B - 1, 64),               # the last element of a super-block of 16
    (21 * B, 65),                   # element 0 of a block; more than STREAM_WQ candidates in a round
    (32 * B, 1024),                 # element 0 of a super-block; a whole block
    (64 * B, 1025),                 # element 0 of a super-block; one element into the next block
    (100 * B + 500, 2100),          # three blocks; more holders than the hit table has slots
    (136 * B - 1, 200),             # the last element of the first of two workgroups' ranges
    (150 * B - 1, 2),               # the last byte of a block again, shortest run
    (272 * B - 30, 30),             # up to the last element of the stream
)


@functools.lru_cache(maxsize=None)
def case_ladder272():
    c = ladder("ladder272", 272 * B, ALL_ENVS, RUNS_272, n_refs=64)
    lay = c.layout()
    for start, m in RUNS_272:
        h = c.hash_at(start)
        c.add(f"run{start}x{m}:alone", [h])
        c.add(f"run{start}x{m}:nbrs", [h - 1, h, h + 1])
    c.add("runs", [c.hash_at(s) for s, _ in RUNS_272])
    c.add("bounds", _bounds_sample(c))
    first, last = int(c.hashes[0]), lay.max_hash
    mid = c.hash_at(77 * B + 123)
    c.add("n1", [mid])
    for n in (64, 65, 4096, 4097):                  # wave_bound's 64-ary rounds: none, one, two, three
        c.add(f"n{n}", _spread(first, last + 1, n))
    c.add("below", _spread(1, first, 100))
    c.add("above", range(last + 1, last + 101))
    c.add("below_above", _spread(1, first, 70) + list(range(last + 1, last + 71)))
    c.add("first_last", [c.hash_at(5), c.hash_at(lay.L - 5)])
    c.add("one_block", [c.hash_at(p) for p in range(150 * B + 100, 150 * B + 900, 16)])
    return c


RUN_257 = (256 * B - 1, 17)        # the last element of the last full super-block; the next one has a single block


def _plain_ladder(nblk, envs, runs=()):
    c = ladder(f"ladder{nblk}", nblk * B, envs, runs)
    for start, m in runs:
        h = c.hash_at(start)
        c.add(f"run{start}x{m}:alone", [h])
        c.add(f"run{start}x{m}:nbrs", [h - 1, h, h + 1])
    c.add("bounds", _bounds_sample(c))
    c.add("n4097", _spread(int(c.hashes[0]) - 3, c.layout().max_hash + 4, 4097))
    return c


@functools.lru_cache(maxsize=None)
def cases_ranges():
    return [_plain_ladder(255, ("wgs1",)), _plain_ladder(256, ("wgs1", "wgs8")), _plain_ladder(257, ("default", "wgs1"), (RUN_257,))]


# ---- cases: the end of the stream ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases_end():
    out = []
    for length in (3 * B, 2 * B + 1, 3 * B - 1):        # L % 1024 = 0, 1 (1023 padding elements with the last key), 1023
        c = ladder(f"end{length % B}", length, SMALL_ENVS)
        mx = c.layout().max_hash
        c.add("largest", [mx])
        c.add("largest_nbrs", [mx - 1, mx, mx + 1])
        c.add("bounds", _bounds_sample(c))
        out.append(c)
    return out


# ---- cases: truncated keys ----------------------------------------------------------------------------------------------------
TRUNC_SHIFTS = (1, 20, 32)
TRUNC_UNITS = 40            # truncated gap of these ladders: in [32, 64), and four of them need no filler


def _trunc(s):
    """2049 elements (1023 padding elements), hashes 40 << s apart: shift s.  min(4, 2^s) hashes share the key of the block
    boundary 1023 | 1024, holders all different; for s = 32 the largest hash's low word is all ones, like an unwritten record's."""
    length = 2 * B + 1
    gap = TRUNC_UNITS << s
    h = [i * gap for i in range(length)]
    k = min(4, 1 << s)
    p0 = B - k // 2
    for j in range(k):
        h[p0 + j] = h[p0] + j
    if s == 32:
        h[-1] |= 0xffffffff
    c = Case(f"trunc{s}", h, np.arange(length) % 8, 8, SMALL_ENVS)
    group = h[p0: p0 + k]
    c.notes.update(group=tuple(group), p0=p0, k=k)
    c.add("last_of_group", [group[-1]])
    c.add("group", group)
    c.add("other_low", [h[100] + 1, h[101], h[2000] + (1 << s) - 1, group[-1]])      # two share a key with a pair and must not count
    c.add("largest", [h[-1]])
    c.add("largest_other_low", [h[-1] ^ 1])
    c.add("largest_both", [h[-1] ^ 1, h[-1]])
    c.add("bounds", _bounds_sample(c))
    # a tile cut between two sample hashes of one key, slots 6077 | 6078 of the one workgroup; and a second tile whose first
    # key is block 1's header while the pair that holds it is the last but one (s = 1: the last) of block 0
    c.add("tile_cut", _spread(0, group[0], ST_CAP - 1) + [group[0], group[1]] + [h[p0 + k + 3], h[-1]])
    c.add("tile_from_header_key", _spread(0, group[0], ST_CAP) + [group[0]] + [h[p0 + k + 3], h[-1]])
    return c


@functools.lru_cache(maxsize=None)
def cases_trunc():
    return [_trunc(s) for s in TRUNC_SHIFTS]


# ---- case: fillers ------------------------------------------------------------------------------------------------------------
FILLER_GAPS = ((B - 1, 256), (B + 1, 255), (B + 2, 510), (B + 4, 511), (2 * B - 2, 511))    # (position of the pair in front, gap)


@functools.lru_cache(maxsize=None)
def case_fillers():
    """Shift 0.  Gaps of 256, 255, 510, 511 behind positions 1023, 1025, 1026, 1028: fillers at 1024 (element 0 of block 1),
    1027, 1029, 1030; a gap of 511 behind 2046: fillers at 2047 and 2048 (element 0 of block 2, the second of its gap)."""
    length, h, p, v = 2500, [], 0, 1000
    gaps = dict(FILLER_GAPS)
    while p < length:
        h.append(v)
        g = gaps.get(p, 1)
        v += g
        p += 1 + (g - 1) // 255
    c = Case("fillers", h, np.arange(len(h)) % 8, 8, SMALL_ENVS)
    lay = c.layout()
    fk = [lay.key_at(q) for q in lay.filler_positions()]
    behind = [c.hash_at(q + 1) for q in lay.filler_positions() if lay.kind_at(q + 1) == "real"]
    front = [c.hash_at(q) for q, _ in FILLER_GAPS]
    c.notes.update(filler_keys=tuple(fk), behind=tuple(behind), front=tuple(front))
    c.add("filler_keys", fk)
    c.add("between", [k + d for k in fk for d in (-1, 1, 100) if k + d not in set(h)])
    c.add("behind", behind)
    c.add("front_and_behind", front + behind + [c.hash_at(B + 2)])
    c.add("all", fk + behind + front + [k + 1 for k in fk])
    c.add("bounds", _bounds_sample(c))
    return c


# ---- case: tiles --------------------------------------------------------------------------------------------------------------
TILE_RUN = (2000, 70)


@functools.lru_cache(maxsize=None)
def case_tiles():
    """Three blocks at shift 20 (room for thousands of sample hashes between the keys), one workgroup; a run of 70."""
    c = ladder("tiles", 3 * B, SMALL_ENVS, runs=(TILE_RUN,), n_refs=8, base=0, gap=TRUNC_UNITS << 20)
    lay = c.layout()
    mx = lay.max_hash
    run_h = c.hash_at(TILE_RUN[0])
    every3 = [int(x) for x in c.hashes[::3]]
    for n in (ST_CAP, ST_CAP + 1, 2 * ST_CAP + 1):     # one, two and three tiles: every third pair and hashes nobody holds
        s = set(every3)
        for x in _spread(12345, mx, 2 * n):
            if len(s) == n:
                break
            s.add(x)
        c.add(f"n{n}", sorted(s))
    c.add("run_last_slot", _spread(1, run_h, ST_CAP - 1) + [run_h] + [c.hash_at(p) for p in range(2100, 3000, 7)])
    c.add("one_block_tile", _spread(1, c.hash_at(1500), ST_CAP) + [c.hash_at(p) for p in range(2100, 3000, 9)])
    lo, hi = c.hash_at(B - 1), c.hash_at(B)
    c.add("gap_tile", _spread(1, c.hash_at(900), ST_CAP) + _spread(lo + (1 << 20), hi, 30))
    return c


# ---- case: the 32-bit offset and its sentinel ---------------------------------------------------------------------------------
WIDE_HASHES = (0, 5, 0xfffffffe << 32, (0xffffffff << 32) + 7)


@functools.lru_cache(maxsize=None)
def case_wide():
    """Four hashes, shift 32, 16 449 blocks of fillers: with one workgroup the third hash is staged at offset 0xfffffffe and
    the fourth, at the sentinel's offset, must end the tile and be found by the next."""
    c = Case("wide", WIDE_HASHES, [0, 1, 0, 1], 2, SMALL_ENVS)
    c.add("all4", WIDE_HASHES)
    c.add("ends", [WIDE_HASHES[0], WIDE_HASHES[3]])
    c.add("last_two", WIDE_HASHES[2:])
    c.add("other_low", [1, 5, WIDE_HASHES[2] + 1, WIDE_HASHES[3] - 7])
    return c


# ---- case: hashes above the largest key ---------------------------------------------------------------------------------------
N_FAR = 4096


@functools.lru_cache(maxsize=None)
def case_above():
    """Three blocks, shift 0, and a sample of 4 096 hashes above max_hash, 2^33 apart, plus a few hits: with the last sample
    range ending at all ones each of them was a tile of one key; ending at the largest key none is staged."""
    c = ladder("above", 3 * B, SMALL_ENVS)
    mx = c.layout().max_hash
    hits = [c.hash_at(p) for p in (0, 1, B - 1, B, 2 * B + 77, 3 * B - 1)]
    c.notes["hits"] = tuple(hits)
    c.add("far_above", hits + [mx + (k << 33) for k in range(1, N_FAR + 1)])
    c.add("only_far_above", [mx + (k << 33) for k in range(1, 65)])
    return c


@functools.lru_cache(maxsize=None)
def all_cases():
    return ([case_ladder272()] + cases_ranges() + cases_end() + cases_trunc() +
            [case_fillers(), case_tiles(), case_wide(), case_above()])


def cases_of(env_name):
    return [c for c in all_cases() if env_name in c.envs]


# ---- a set-based count from the table -----------------------------------------------------------------------------------------
def set_counts(case, sample):
    """overlap, n_excl and n_match of the run step (subset = overlap > 0) from the hash -> holders table."""
    table = case.table()
    n = case.n_refs
    ov = np.zeros(n, dtype=np.int64)
    for h in sample.tolist():
        for r in table.get(h, ()):
            ov[r] += 1
    sub = ov > 0
    singles = np.zeros(n, dtype=np.int64)       # hashes with one holder: exclusive to it whatever the subset
    shared = []
    for h, holders in table.items():
        if len(holders) == 1:
            singles[holders[0]] += 1
        else:
            shared.append(holders)
    e = np.where(sub, singles, 0)
    for holders in shared:
        inside = [r for r in holders if sub[r]]
        if len(inside) == 1:
            e[inside[0]] += 1
    m = np.zeros(n, dtype=np.int64)
    for h in sample.tolist():
        inside = [r for r in table.get(h, ()) if sub[r]]
        if len(inside) == 1:
            m[inside[0]] += 1
    return ov.astype(np.uint32), e.astype(np.uint32), m.astype(np.uint32)
