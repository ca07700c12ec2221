"""Case generators for the packed formats (yh_pack.hip), numpy only: strictly ascending uint64 arrays built block by block so
that the packer is forced to a chosen width per 256-hash block, the CSR databases of the device expansion, and the
references / hit patterns of the compact rows.  Shared by tests/test_packed_cases_cpu.py (which guards that the cases still
hold what they are meant to hold) and tests/test_gpu_packed_edges.py (which runs them on the device).

A block of cnt hashes stores cnt - 1 gaps g[i] = h[i] - h[i-1] - 1 at the width of the widest one: width = bit length of the OR
of the gaps.  Gap i - 1 (of lane i) occupies bits [(i-1) w, i w) of the block's payload words.
"""
import numpy as np

BLOCK = 256
TOP = 1 << 64
WIDE_LANES = (1, 63, 64, 65, 127, 128, 255)     # the lane that holds the wide gap of a block of width 57..64
TAIL_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1024 + 1)
TAIL_WIDTHS = (0, 1, 37, 64)
MAX_SAMPLE = 20_000


def bits_of(v: int) -> int:
    return int(v).bit_length()


def block_widths(a: np.ndarray) -> list:
    """The width of every 256-hash block of an ascending array, restated from the format's definition."""
    a = [int(x) for x in a]
    out = []
    for first in range(0, len(a), BLOCK):
        blk = a[first: first + BLOCK]
        widest = 0
        for p, q in zip(blk, blk[1:]):
            assert q > p
            widest |= q - p - 1
        out.append(bits_of(widest))
    return out


def gaps_for(rng, w: int, cnt: int, lanes=(), fill=None) -> list:
    """The cnt - 1 stored gaps of a block whose width comes out as exactly w.
    w = 0: all zero.  w <= 56 (fill = w): every gap random in [0, 2^w), the gaps of `lanes` (one random lane if none is given)
    with bit w - 1 set.  w >= 57 (fill = 40): the gaps of `lanes` in [2^(w-1), 2^(w-1) + 2^(w-3)), the rest random below 2^40.
    `fill` < w keeps the other gaps below 2^fill where the sum has to stay small."""
    k = cnt - 1
    if w == 0 or k == 0:
        assert w == 0, "a block of one hash has no gap to be wide"
        return [0] * k
    if fill is None:
        fill = w if w <= 56 else 40
    fill = min(fill, w)
    g = [int(x) for x in rng.integers(0, 1 << fill, size=k, dtype=np.uint64)]
    lanes = [ln for ln in lanes if 1 <= ln < cnt] or [int(rng.integers(1, cnt))]
    for ln in lanes:
        if w <= 56 and fill == w:
            g[ln - 1] |= 1 << (w - 1)
        else:
            g[ln - 1] = (1 << (w - 1)) + int(rng.integers(0, 1 << max(w - 3, 0), dtype=np.uint64))
    assert bits_of(np.bitwise_or.reduce(np.array(g, dtype=np.uint64))) == w
    return g


def span_of(gaps) -> int:
    return sum(gaps) + len(gaps)            # last hash - first hash


def hashes_from(start: int, gaps) -> list:
    h = [start]
    for g in gaps:
        h.append(h[-1] + g + 1)
    assert h[-1] < TOP
    return h


class Case:
    """One packed sample: its hashes, the width every block was built for, what it is about."""

    def __init__(self, name):
        self.name = name
        self.h = []         # python ints
        self.widths = []
        self.closed = False

    def room(self) -> int:
        return TOP - 1 - (self.h[-1] if self.h else -1)

    def add(self, w, gaps, lead=0, start=None) -> bool:
        """Append a block (`lead` values skipped in front of it); False if it does not fit below 2^64."""
        assert not self.closed and len(self.h) % BLOCK == 0
        if start is None:
            start = (self.h[-1] + 1 + lead) if self.h else lead
        assert not self.h or start > self.h[-1]
        if start + span_of(gaps) > TOP - 1:
            return False
        self.h += hashes_from(start, gaps)
        self.widths.append(w)
        if len(gaps) + 1 < BLOCK:
            self.closed = True
        return True

    @property
    def hashes(self) -> np.ndarray:
        return np.array(self.h, dtype=np.uint64)


def wide_lanes_of(w: int, lane: int) -> tuple:
    """One wide gap, or two for w <= 62 (the second 100 lanes further on, wrapped into 1..255)."""
    return (lane,) if w > 62 else (lane, (lane + 99) % 255 + 1)


def sample_cases(seed: int = 20260) -> list:
    """Every packed-sample case.  The large ones are filled first-fit with full blocks, widest first (a block of width 64
    takes more than half of the range, so each of those seeds a sample of its own); the small ones have the sizes of
    TAIL_SIZES with the widths of TAIL_WIDTHS in their last block."""
    rng = np.random.default_rng(seed)
    specs = []                                                  # (w, lanes) of full blocks
    for w in range(64, 56, -1):
        for lane in WIDE_LANES:
            specs.append((w, wide_lanes_of(w, lane)))
    for w in range(56, -1, -1):
        specs.append((w, ()))
    big = []
    for w, lanes in specs:
        gaps = gaps_for(rng, w, BLOCK, lanes)
        lead = int(rng.integers(0, 1 << 20))
        for c in big:
            if len(c.h) + BLOCK <= MAX_SAMPLE and c.add(w, gaps, lead):
                break
        else:
            c = Case(f"full{len(big)}")
            assert c.add(w, gaps, lead), (w, lanes)
            big.append(c)
    cases = big
    # block tails: sizes n, the last block of 1, 2, 63, 64, 65, 255 or 256 hashes at widths 0, 1, 37, 64; full blocks of width 37 in front
    for n in TAIL_SIZES:
        cnt = (n - 1) % BLOCK + 1
        for w in TAIL_WIDTHS:
            if w and cnt < 2:
                continue
            c = Case(f"n{n}_w{w}")
            for _ in range((n - 1) // BLOCK):
                assert c.add(37, gaps_for(rng, 37, BLOCK), int(rng.integers(0, 1 << 30)))
            lane = (int(rng.integers(1, cnt)),) if cnt > 1 else ()
            assert c.add(w, gaps_for(rng, w, cnt, lane), int(rng.integers(0, 1 << 30)))
            assert len(c.h) == n
            cases.append(c)
    # the two-hash sample with the widest gap there is
    c = Case("zero_and_all_ones")
    assert c.add(64, [TOP - 2])
    cases.append(c)
    # width 0 at the top of the range: a block of 2^64 - 256 + i behind a block of 37-bit gaps; on its own; with a tail of 2 in front
    c = Case("top_run_behind_w37")
    assert c.add(37, gaps_for(rng, 37, BLOCK), 12345)
    assert c.add(0, [0] * (BLOCK - 1), start=TOP - BLOCK)
    cases.append(c)
    c = Case("top_run_alone")
    assert c.add(0, [0] * (BLOCK - 1), start=TOP - BLOCK)
    cases.append(c)
    c = Case("run_and_tail_of_2")
    assert c.add(0, [0] * (BLOCK - 1), 7)
    assert c.add(0, [0], 1 << 50)
    cases.append(c)
    for c in cases:
        assert block_widths(c.h) == c.widths, c.name
        assert len(c.h) <= MAX_SAMPLE
    return cases


def gap_fits(w: int, cnt: int):
    """(a gap of the block straddles a 64-bit word, a gap ends exactly on one) for a block of cnt hashes at width w."""
    straddle = exact = False
    for k in range(cnt - 1):
        sh = (k * w) & 63
        straddle |= sh + w > 64
        exact |= sh + w == 64
    return straddle, exact


def sample_block_widths(packed: np.ndarray) -> list:
    """The widths a packed sample's block table holds: uint32 at byte 32 + 16 b + 12."""
    raw = np.ascontiguousarray(packed, dtype=np.uint8).tobytes()
    n = int(np.frombuffer(raw[8:16], dtype=np.uint64)[0])
    nb = (n + BLOCK - 1) // BLOCK
    return [int(np.frombuffer(raw[32 + 16 * b + 12: 32 + 16 * b + 16], dtype=np.uint32)[0]) for b in range(nb)]


def csr_block_widths(blob: np.ndarray) -> list:
    """The widths of a packed CSR's block table: 64-byte header, offsets [n_refs + 1], 24-byte entries with the width at byte 16."""
    n_refs, n_blocks = int(blob[1]), int(blob[3])
    first = 8 + n_refs + 1
    return [int(blob[first + 3 * b + 2]) & 0xFFFFFFFF for b in range(n_blocks)]


# ---- forged packed samples: ordering errors only (every size, width and payload offset stays as the packer wrote it) ----------
def _set_base(packed: np.ndarray, b: int, base: int) -> np.ndarray:
    out = packed.copy()
    out[32 + 16 * b: 32 + 16 * b + 8] = np.frombuffer(np.uint64(base).tobytes(), dtype=np.uint8)
    return out


def forge_last_lane_wraps(pack_sample, seed: int = 5):
    """One full block whose base is moved up until hash 255 -- and no other -- passes 2^64."""
    rng = np.random.default_rng(seed)
    gaps = gaps_for(rng, 37, BLOCK)
    good = np.array(hashes_from(1000, gaps), dtype=np.uint64)
    base = TOP - span_of(gaps)                 # base + span = 2^64: the last hash wraps to 0, hash 254 stays below 2^64
    assert base + span_of(gaps[:-1]) < TOP
    return good, _set_base(pack_sample(good), 0, base)


def forge_block_meets_next_base(pack_sample, seed: int = 6):
    """Two full blocks; the second one's base is set to the first one's last hash."""
    rng = np.random.default_rng(seed)
    g0, g1 = gaps_for(rng, 37, BLOCK), gaps_for(rng, 37, BLOCK)
    h0 = hashes_from(1000, g0)
    good = np.array(h0 + hashes_from(h0[-1] + 99, g1), dtype=np.uint64)
    return good, _set_base(pack_sample(good), 1, h0[-1])


# ---- CSR databases for the device expansion (k_unpack_csr) -----------------------------------------------------------
def _sketch(rng, blocks, start=None, fill=52):
    """A sketch from (width, count) per block; everything below 2^63 unless a width of 64 asks for more."""
    h, widths = [], []
    for w, cnt in blocks:
        gaps = gaps_for(rng, w, cnt, fill=min(w, fill) if w <= 56 else None)
        s = (h[-1] + 1 + int(rng.integers(0, 1 << 16))) if h else (int(rng.integers(0, 1 << 30)) if start is None else start)
        h += hashes_from(s, gaps)
        widths.append(w)
    return h, widths


CSR_SIZES = (0, 0, 1, 2, 255, 256, 257, 0, 511, 512, 513, 1000, 0, 0, 3, 0)
_CSR_BLOCKS = {1: [(0, 1)], 2: [(63, 2)], 255: [(0, 255)], 256: [(1, 256)], 257: [(37, 256), (0, 1)],
               511: [(56, 256), (1, 255)], 512: [(37, 256), (63, 256)], 513: [(0, 256), (56, 256), (0, 1)],
               1000: [(1, 256), (37, 256), (56, 256), (63, 232)], 3: [(37, 3)]}


def csr_database(kind: str, seed: int = 404):
    """(values, offsets, intended width per block) of the databases the device expansion is run on:
    "sizes"  sketches of CSR_SIZES hashes -- empty ones first, last and in runs -- at widths 0, 1, 37, 56 and 63, all below 2^63,
             followed by a cluster of sketches that share half of their hashes;
    "top"    the same plus [0, 2^64 - 1] (width 64) and a sketch that ends in 2^64 - 1;
    "tiny"   300 sketches of 0..3 hashes drawn from a small pool."""
    rng = np.random.default_rng(seed)
    refs, widths = [], []
    if kind in ("sizes", "top"):
        for size in CSR_SIZES:
            h, w = _sketch(rng, _CSR_BLOCKS[size]) if size else ([], [])
            assert len(h) == size and (not h or h[-1] < 1 << 63)
            refs.append(h)
            widths += w
        # a cluster: five sketches made of halves of two parents (pairs and shared-hash statistics are not trivial), and an
        # empty one in between
        pa, _ = _sketch(rng, [(37, 256), (37, 256), (37, 88)])
        pb, _ = _sketch(rng, [(37, 256), (37, 144)])
        for k, members in enumerate((pa[::2] + pb[::2], pa[1::2] + pb[::2], pa[::2] + pb[1::2], pa, pb[::2])):
            if k == 3:
                refs.append([])
            refs.append(sorted(set(members)))
            widths += block_widths(refs[-1])
        if kind == "top":
            refs.append([0, TOP - 1])
            widths.append(64)
            tail, w = _sketch(rng, [(37, 256)])
            refs.append(tail + list(range(TOP - 44, TOP)))            # 300 hashes, the last one 2^64 - 1
            widths += block_widths(refs[-1])
            # blocks of width 64 whose wide gap has other gaps (and, at lane 255, the next block's words) behind it: what a
            # two-word read that should not happen at sh + w == 64 would pull in
            refs.append(hashes_from(int(rng.integers(0, 1 << 30)), gaps_for(rng, 64, BLOCK, (64,))))
            widths.append(64)
            wide = hashes_from(int(rng.integers(0, 1 << 30)), gaps_for(rng, 64, BLOCK, (255,)))
            more, _ = _sketch(rng, [(37, 44)], start=wide[-1] + 5)
            refs.append(wide + more)
            widths += [64, 37]
    elif kind == "tiny":
        pool = [int(x) for x in np.unique(rng.integers(1, 1 << 62, size=150, dtype=np.uint64))]
        for _ in range(300):
            k = int(rng.integers(0, 4))
            refs.append(sorted(pool[int(i)] for i in rng.choice(len(pool), size=k, replace=False)))
            widths += block_widths(refs[-1])
    else:
        raise ValueError(kind)
    offsets = np.zeros(len(refs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in refs], dtype=np.uint64)
    values = np.array([x for r in refs for x in r], dtype=np.uint64)
    return values, offsets, widths


CSR_KINDS = ("sizes", "top", "tiny")


# ---- compact rows: N references, hit patterns -------------------------------------------------------------------------
ROWS_N = (1, 31, 32, 33, 64, 65, 2047, 2048, 2049, 4096, 4097)


def rows_database(n: int):
    """N references with one private hash each (1000 (j + 1)); every fifth one also holds a hash it shares with its right
    neighbour (1000 (j + 1) + 500), so that n_excl and n_match differ from the overlap."""
    refs = [[1000 * (j + 1)] for j in range(n)]
    for j in range(0, n - 1, 5):
        refs[j].append(1000 * (j + 1) + 500)
        refs[j + 1].insert(0, 1000 * (j + 1) + 500)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in refs], dtype=np.uint64)
    values = np.array([x for r in refs for x in r], dtype=np.uint64)
    return values, offsets


def rows_patterns(n: int, seed: int = 9) -> dict:
    """name -> the references (ascending) that get a row."""
    rng = np.random.default_rng(seed + n)
    every = np.arange(n)
    pats = {"none": every[:0], "all": every, "first": every[:1], "last": every[-1:], "bit0": every[every % 32 == 0],
            "bit31": every[every % 32 == 31], "p01": every[rng.random(n) < 0.01], "p50": every[rng.random(n) < 0.5]}
    if n > 2048:
        pats["only2048"] = every[2048:2049]
    return pats


def rows_sample(n: int, hit: np.ndarray) -> np.ndarray:
    """The sample that overlaps exactly the references of `hit`: their private hashes, the shared hash of a pair where both
    are hit, and one hash no reference holds."""
    hit = set(int(j) for j in hit)
    s = [1000 * (j + 1) for j in hit]
    s += [1000 * (j + 1) + 500 for j in range(0, n - 1, 5) if j in hit and j + 1 in hit]
    s.append(7)
    return np.array(sorted(s), dtype=np.uint64)
