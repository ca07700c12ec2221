"""Databases on the edges of the exclusive pass (holder-set records, pieces, work-list blocks, subset words), numpy only.

Never calls the library.  A database is built from a table of (holders, multiplicity) entries -- `multiplicity` hashes held by
exactly these references -- plus a few PRIVATE hashes per reference that nobody else holds.  Samples steer the subset of the run
step (overlap > 0): a sample made only of the private hashes of a set P of references makes the subset exactly P without
touching a shared hash; the "shared" sample holds every shared hash and pulls in all their holders; the "noise" sample is not
empty and overlaps nothing.

Next to each database stands a plain-Python mirror of the layout the library builds from it (yh_build.hip
k_fill_rg / k_set_*): per reference its holder-set records as (sorted tuple of the OTHER holders, multiplicity), in the order
the build leaves them in (ascending 64-bit mix of the 32-byte record).  A hash with nine or more holders is one record per
hash.  From the records: n_holder_sets, the shared postings, records and pieces per reference, records with more than three
other holders.  tests/test_excl_cases_cpu.py pins that every case reaches its state; tests/test_gpu_excl_edges.py runs the
kernels on them.
"""
import functools

import numpy as np

PIECE = 256                 # YH_EXCL_PIECE: records per work record
INLINE_MAX = 8              # holders of a hash whose OTHER holders (<= 7) sit inline in rec / recx
REC_OTHERS = 3              # other holders in rec; others 3..6 are in recx
LDS_WORDS = 12288           # EXCL_LDS_WORDS: subset words staged in LDS
N_LDS_LAST = 393_216        # the last database whose subset words are staged
MAX_HASH_SCALED_1000 = (2 ** 64 + 500) // 1000
N_PRIVATE = 3
FUSED_1024_SAMPLE = 262_144  # yh_tile_shape_for: from this sample size on k_step_fused runs 1024 lanes (reducer blocks of 4096)
M64 = (1 << 64) - 1


def mask_words(n_refs):
    """Words of the subset bits of a database of n_refs references: whole 256-reference blocks."""
    return (n_refs + 255) // 256 * 8


# ---- the build's record order ---------------------------------------------------------------------------------------------
def _mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def record_key(others):
    """The 64-bit key the build sorts a reference's inline records by (k_set_keys over rec = {o0, o1, o2, count},
    recx = {o3, o4, o5, o6})."""
    o = list(others) + [0] * (7 - len(others))
    h = _mix((o[0] << 32) | o[1])
    h = _mix(h ^ ((o[2] << 32) | len(others)))
    h = _mix(h ^ ((o[3] << 32) | o[4]))
    return _mix(h ^ ((o[5] << 32) | o[6]))


# ---- a case ---------------------------------------------------------------------------------------------------------------
class Case:
    """One database: n_refs, entries [(holders (ascending tuple), multiplicity)], which references get private hashes."""

    def __init__(self, name, n_refs, entries, private_refs=None, seed=0):
        self.name = name
        self.n_refs = int(n_refs)
        self.entries = [(tuple(int(x) for x in sorted(h)), int(m)) for h, m in entries]
        for h, m in self.entries:
            assert len(h) >= 2 and len(set(h)) == len(h) and m >= 1 and h[-1] < self.n_refs
        assert len({h for h, _ in self.entries}) == len(self.entries), "two entries with the same holders would merge"
        self.private_refs = np.arange(self.n_refs) if private_refs is None else np.asarray(sorted(private_refs), dtype=np.int64)
        self.subsets = {}        # label -> ascending tuple of references: a private-only sample makes exactly this subset
        self.extra_masks = {}    # label -> references added to the subset's mask that its private-only sample does not hit
        self.notes = {}
        n_sh = sum(m for _, m in self.entries)
        n_pr = N_PRIVATE * self.private_refs.size
        total = n_sh + n_pr
        # distinct hash values, small enough for the directory's compact form (a bucket must span < 2^32 values) and above
        # 2^32 wherever the database has a few distinct hashes
        bound = min(MAX_HASH_SCALED_1000, max(total, 4) << 30)
        rng = np.random.default_rng([seed, sum(ord(c) for c in name)])
        pool = np.unique(rng.integers(1, bound, size=total + total // 8 + 64, dtype=np.uint64))
        assert pool.size >= total
        pool = rng.permutation(pool)[:total]
        self.entry_hashes = []
        at = 0
        for _, m in self.entries:
            self.entry_hashes.append(np.sort(pool[at: at + m]))
            at += m
        self.private = pool[at:].reshape(self.private_refs.size, N_PRIVATE)
        self._priv_row = {int(r): i for i, r in enumerate(self.private_refs)} if self.private_refs.size <= 100_000 else None
        self.noise = np.sort(np.unique(rng.integers(bound + 1, bound * 2, size=40, dtype=np.uint64)))

    # -- the CSR
    @functools.lru_cache(maxsize=None)
    def csr(self):
        refs = [np.repeat(self.private_refs, N_PRIVATE)]
        vals = [self.private.reshape(-1)]
        for (h, m), hs in zip(self.entries, self.entry_hashes):
            refs.append(np.repeat(np.asarray(h, dtype=np.int64), m))
            vals.append(np.tile(hs, len(h)))
        refs = np.concatenate(refs)
        vals = np.concatenate(vals)
        order = np.lexsort((vals, refs))
        values = np.ascontiguousarray(vals[order], dtype=np.uint64)
        offsets = np.zeros(self.n_refs + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum(np.bincount(refs, minlength=self.n_refs)).astype(np.uint64)
        values.setflags(write=False)
        offsets.setflags(write=False)
        return values, offsets

    def private_of(self, refs):
        refs = list(refs)
        if not refs:
            return np.zeros(0, dtype=np.uint64)
        if self._priv_row is not None:
            rows = [self._priv_row[int(r)] for r in refs]
        else:
            rows = np.searchsorted(self.private_refs, refs)
            assert np.array_equal(self.private_refs[rows], refs)
        return np.sort(self.private[rows].reshape(-1))

    # -- samples
    def shared_sample(self):
        return np.sort(np.concatenate(self.entry_hashes)) if self.entries else np.zeros(0, dtype=np.uint64)

    @functools.lru_cache(maxsize=None)
    def samples(self):
        """label -> sample: "P:<label>" the private-only sample of every subset, "shared" (every shared hash: all holders),
        "noise" (not empty, overlaps nothing)."""
        out = {f"P:{label}": self.private_of(p) for label, p in self.subsets.items()}
        out["shared"] = self.shared_sample()
        out["noise"] = self.noise
        for s in out.values():
            s.setflags(write=False)
        return out

    def masks(self):
        """(label, mask, sample label) for RefDB.exclusive: every subset as the mask with the shared sample (the sample hits
        shared hashes of references inside and outside the mask), the subset widened by references its private-only sample does
        not hit, and every reference with the shared sample."""
        out = []
        for label, p in self.subsets.items():
            m = np.zeros(self.n_refs, dtype=np.uint8)
            m[list(p)] = 1
            out.append((f"{label}|shared", m, "shared"))
            extra = self.extra_masks.get(label)
            if extra is not None:
                m2 = m.copy()
                m2[list(extra)] = 1
                out.append((f"{label}+{len(extra)}|P", m2, f"P:{label}"))
        out.append(("everyone|shared", np.ones(self.n_refs, dtype=np.uint8), "shared"))
        return out

    # -- the mirror
    @functools.lru_cache(maxsize=None)
    def mirror(self):
        return Mirror(self)


class Mirror:
    """What the build makes of a case, from its table alone."""

    def __init__(self, case):
        self.n_refs = case.n_refs
        inline = {}          # reference -> {others: multiplicity}
        lists = {}           # reference -> [(holders, entry index)] one per HASH of a list-form entry
        self.nshared = {}
        self.n_shared_postings = 0
        self.n_shared_distinct = 0
        for e, (h, m) in enumerate(case.entries):
            self.n_shared_postings += m * len(h)
            self.n_shared_distinct += m
            for r in h:
                self.nshared[r] = self.nshared.get(r, 0) + m
                if len(h) <= INLINE_MAX:
                    d = inline.setdefault(r, {})
                    others = tuple(o for o in h if o != r)
                    d[others] = d.get(others, 0) + m
                else:
                    lists.setdefault(r, []).extend([(h, e)] * m)
        self.inline_records = {r: sorted(d.items(), key=lambda kv: record_key(kv[0])) for r, d in inline.items()}   # (build order)
        self.list_records = lists
        self.sizes = np.zeros(case.n_refs, dtype=np.int64)
        self.sizes[case.private_refs] = N_PRIVATE
        for r, c in self.nshared.items():
            self.sizes[r] += c

    def refs_with_records(self):
        return sorted(set(self.inline_records) | set(self.list_records))

    def n_records(self, r):
        return len(self.inline_records.get(r, ())) + len(self.list_records.get(r, ()))

    def n_holder_sets(self):
        return sum(self.n_records(r) for r in self.refs_with_records())

    def set_pieces(self, r):
        """Work records of r in the run step (pieces of its holder-set records)."""
        return (self.n_records(r) + PIECE - 1) // PIECE

    def posting_pieces(self, r):
        """Work records of r in the general pass (pieces of its shared postings)."""
        return (self.nshared.get(r, 0) + PIECE - 1) // PIECE

    def wide_records(self, r):
        """Positions, among r's INLINE records in build order, of those with more than three other holders (the recx read)."""
        return [i for i, (o, _) in enumerate(self.inline_records.get(r, ())) if len(o) > REC_OTHERS]

    def list_lengths(self, r):
        return sorted({len(h) for h, _ in self.list_records.get(r, ())})

    def n_excl(self, subset):
        """n_excl of every reference for a subset, by sets: |R_r| - nshared_r + the multiplicities of r's records with no other
        holder in the subset; zero outside the subset."""
        inside = set(int(x) for x in subset)
        out = np.zeros(self.n_refs, dtype=np.int64)
        for r in inside:
            e = int(self.sizes[r]) - self.nshared.get(r, 0)
            for others, m in self.inline_records.get(r, ()):
                if not inside.intersection(others):
                    e += m
            for h, _ in self.list_records.get(r, ()):
                if len(inside.intersection(h)) == 1:
                    e += 1
            out[r] = e
        return out


def n_match_by_sets(case, subset, sample):
    """n_match for a subset and a sample, from the table: a sample hash counts for reference r of the subset when no other
    holder of it is in the subset."""
    inside = set(int(x) for x in subset)
    out = np.zeros(case.n_refs, dtype=np.int64)
    sample = np.asarray(sample, dtype=np.uint64)
    if case.entries:
        flat = np.concatenate(case.entry_hashes)
        entry_of = np.repeat(np.arange(len(case.entries)), [m for _, m in case.entries])
        hits = np.bincount(entry_of[np.isin(flat, sample)], minlength=len(case.entries))
        for e in np.flatnonzero(hits):
            mine = inside.intersection(case.entries[e][0])
            if len(mine) == 1:
                out[mine.pop()] += int(hits[e])
    hit = np.isin(case.private, sample).sum(axis=1)
    for i in np.flatnonzero(hit):
        r = int(case.private_refs[i])
        if r in inside:
            out[r] += int(hit[i])
    return out


def subset_of_mask(mask):
    return tuple(int(x) for x in np.flatnonzero(np.asarray(mask)))


# ---- case 1: record forms -------------------------------------------------------------------------------------------------
FORM_K = (2, 3, 4, 5, 8, 9, 10, 16, 17, 64, 65)
FORM_N = 80
FORM_UNDER_TEST = {"low": 2, "mid": 40, "high": 77}
INLINE_SLOTS = (0, 2, 3, 6)


def form_entries(rng, n_refs=FORM_N, ids=None):
    """For every k of FORM_K and the reference under test as the lowest, a middle and the highest holder: (k, place, t, holders)."""
    out = []
    for k in FORM_K:
        for place, t in FORM_UNDER_TEST.items():
            below, above = np.arange(0, t), np.arange(t + 1, n_refs)
            n_below = {"low": 0, "mid": (k - 1) // 2, "high": k - 1}[place]
            n_below = min(n_below, below.size)
            n_above = k - 1 - n_below
            if n_above > above.size:
                n_below += n_above - above.size
                n_above = above.size
            h = sorted([t] + rng.choice(below, n_below, replace=False).tolist() + rng.choice(above, n_above, replace=False).tolist())
            assert len(h) == k
            out.append((k, place, t, tuple(h)))
    return out


def form_subsets(k, t, holders):
    """The subsets of one entry: {label: P}."""
    others = [o for o in holders if o != t]
    out = {"alone": (t,)}
    if k <= INLINE_MAX:
        for s in INLINE_SLOTS:
            if s < len(others):
                out[f"slot{s}"] = tuple(sorted((t, others[s])))
    else:
        for p in (0, 7, 8, len(holders) - 1):
            if holders[p] != t:
                out[f"pos{p}"] = tuple(sorted((t, holders[p])))
        two = [o for o in holders[:8] if o != t][:2]           # both inside the walk's first step: the early exit
        out["two_in_step0"] = tuple(sorted([t] + two))
    return out


@functools.lru_cache(maxsize=None)
def case_forms():
    rng = np.random.default_rng(7101)
    table = form_entries(rng)
    c = Case("forms", FORM_N, [(h, 1 + i % 3) for i, (_, _, _, h) in enumerate(table)], seed=1)
    c.notes["table"] = table
    for k, place, t, h in table:
        for label, p in form_subsets(k, t, h).items():
            c.subsets[f"k{k}_{place}_{label}"] = p
            c.extra_masks[f"k{k}_{place}_{label}"] = tuple(x for x in (0, 79) if x not in h)
    return c


# ---- case 2: one lane decides the recx read --------------------------------------------------------------------------------
RECX_T = 130
RECX_N = 258


def _case_recx(where):
    """Reference RECX_T with 256 distinct sets: 255 (or 256) single partners and one set of FOUR others, which the build's
    order puts last / first among t's records; "none": 256 single partners."""
    partners = [r for r in range(1, RECX_N) if r != RECX_T]           # (reference 0 shares nothing: recx left unread reads as id 0)
    singles = partners[:256 if where == "none" else 255]
    entries = [((RECX_T, p), 1) for p in singles]
    wide = None
    if where != "none":
        keys = [record_key((p,)) for p in singles]
        lo, hi = min(keys), max(keys)
        rng = np.random.default_rng(7202)
        for _ in range(200_000):
            cand = tuple(sorted(rng.choice(partners, 4, replace=False).tolist()))
            k = record_key(cand)
            if (where == "last" and k > hi) or (where == "first" and k < lo):
                wide = cand
                break
        assert wide is not None
        entries.append(((RECX_T,) + wide, 1))
    c = Case(f"recx_{where}", RECX_N, entries, seed=2)
    c.notes["wide"] = wide
    c.subsets["alone"] = (RECX_T,)
    c.subsets["a_single"] = tuple(sorted((RECX_T, singles[17])))
    c.subsets["everyone"] = tuple(range(RECX_N))
    if wide:
        for s in range(4):
            c.subsets[f"wide_slot{s}"] = tuple(sorted((RECX_T, wide[s])))
        c.extra_masks["wide_slot3"] = (0,)
    c.extra_masks["alone"] = (0,)
    return c


@functools.lru_cache(maxsize=None)
def cases_recx():
    return tuple(_case_recx(w) for w in ("last", "first", "none"))


# ---- case 3: sweeps and pieces ---------------------------------------------------------------------------------------------
SWEEP_D = (1, 64, 65, 128, 129, 255, 256, 257, 512, 513)
SWEEP_AT = (0, 63, 64, 127, 128, 255, 256)


def _case_sweep(d):
    """References 0 and d + 1 (the last) each share one hash with each of the partners 1..d and with nobody else: d distinct
    single-partner sets, d shared postings.  The last reference's records end at n_sets, its postings at n_postings."""
    first, last = 0, d + 1
    entries = [((first, p), 1) for p in range(1, d + 1)] + [((p, last), 1) for p in range(1, d + 1)]
    c = Case(f"sweep_{d}", d + 2, entries, seed=3)
    c.subsets["both_alone"] = (first, last)
    mir = c.mirror()
    for at in sorted(set(a for a in SWEEP_AT + (d - 1,) if a < d)):
        # the partner whose record sits at position `at` of the reference's records, for each of the two
        pf = mir.inline_records[first][at][0][0]
        pl = mir.inline_records[last][at][0][0]
        c.subsets[f"record{at}"] = tuple(sorted({first, last, pf, pl}))
    c.subsets["everyone"] = tuple(range(d + 2))
    c.extra_masks["both_alone"] = (1,)
    return c


@functools.lru_cache(maxsize=None)
def cases_sweep():
    return tuple(_case_sweep(d) for d in SWEEP_D)


# ---- case 4: multiplicities and near-equal sets ----------------------------------------------------------------------------
MULT_M = (1, 2, 65_535, 65_536, 70_000)
MULT_T, MULT_T2, MULT_A, MULT_B, MULT_C, MULT_D, MULT_E = 10, 11, 12, 13, 14, 15, 16
MULT_DUP = (17, 18)
MULT_N = 20


@functools.lru_cache(maxsize=None)
def case_mult():
    """Pairs (2 i, 2 i + 1) sharing MULT_M[i] hashes; T holds {a,b,c} x 3, {a,b,c,d} x 5, {a,b,c,e} x 7 (records that differ
    in rec.w or in recx only); T2 holds {a,b,c} x 2 (the same set on another reference); 17 and 18 are whole duplicates."""
    entries = [((2 * i, 2 * i + 1), m) for i, m in enumerate(MULT_M)]
    entries += [((MULT_T, MULT_A, MULT_B, MULT_C), 3), ((MULT_T, MULT_A, MULT_B, MULT_C, MULT_D), 5),
                ((MULT_T, MULT_A, MULT_B, MULT_C, MULT_E), 7), ((MULT_T2, MULT_A, MULT_B, MULT_C), 2), (MULT_DUP, 50)]
    c = Case("mult", MULT_N, entries, private_refs=[r for r in range(MULT_N) if r not in MULT_DUP], seed=4)
    c.subsets["evens"] = tuple(range(0, 10, 2))
    c.subsets["pairs"] = tuple(range(0, 10))
    c.subsets["t_no_d_no_e"] = (MULT_T, MULT_T2)
    c.subsets["t_with_d"] = (MULT_T, MULT_T2, MULT_D)
    c.subsets["t_with_e"] = (MULT_T, MULT_T2, MULT_E)
    c.subsets["t_with_d_e"] = (MULT_T, MULT_T2, MULT_D, MULT_E)
    c.subsets["t_with_a"] = (MULT_T, MULT_T2, MULT_A)
    c.subsets["everyone_private"] = tuple(r for r in range(MULT_N) if r not in MULT_DUP)
    c.extra_masks["t_no_d_no_e"] = (MULT_DUP[0],)
    c.extra_masks["t_with_d"] = MULT_DUP
    return c


# ---- case 5: work-list blocks ----------------------------------------------------------------------------------------------
WORK_N = (256, 257, 1024, 1025, 4096, 4097)
WORK_POOL = tuple(range(100, 140))          # the partners every heavy reference draws its sets from
WORK_LANES = {0: 0, 63: 200, 64: 300, 255: 600}     # lane of a 256-block -> records: 0, 1, 2, 3 pieces
WORK_BLOCKS = (0, 3, 15)                     # the pattern's blocks: the first, the ones that end at 1023 and at 4095
WORK_FIRSTS = (256, 1024, 4096)              # the first reference behind a block of 256 / 1024 / 4096: two pieces


def work_heavy(n_refs):
    """reference -> records, for the references of a work-list database that need pieces."""
    out = {}
    for b in WORK_BLOCKS:
        for lane, recs in WORK_LANES.items():
            r = 256 * b + lane
            if recs and r < n_refs:
                out[r] = recs
    for r in WORK_FIRSTS:
        if r < n_refs:
            out[r] = 300
    return out


def _case_work(n_refs):
    pool = list(WORK_POOL)
    sets = [(p,) for p in pool] + [(p, q) for i, p in enumerate(pool) for q in pool[i + 1:]]      # 40 + 780 distinct sets
    heavy = work_heavy(n_refs)
    entries = []
    for r, recs in sorted(heavy.items()):
        entries += [(tuple(sorted((r,) + s)), 1) for s in sets[:recs]]
    c = Case(f"work_{n_refs}", n_refs, entries, seed=5)
    c.notes["heavy"] = heavy
    last_block = (n_refs - 1) // 256
    c.subsets["last_of_block0"] = (255,)
    c.subsets["only_last"] = (n_refs - 1,)
    c.subsets["lanes_63_64"] = (63, 64)
    if n_refs > 1023:
        c.subsets["block3"] = tuple(range(768, 1024))           # block 0 (and every other) totals 0
        c.subsets["around_1024"] = tuple(r for r in (1023, 1024) if r < n_refs)
    else:
        c.subsets["no_heavy_of_block0"] = tuple(r for r in range(140, min(n_refs, 255)))
    if n_refs > 4095:
        c.subsets["around_4096"] = tuple(r for r in (4095, 4096) if r < n_refs)
    c.subsets["last_block"] = tuple(range(256 * last_block, n_refs))
    c.subsets["everyone"] = tuple(range(n_refs))
    c.extra_masks["only_last"] = (0, 100)
    return c


@functools.lru_cache(maxsize=None)
def cases_work():
    return tuple(_case_work(n) for n in WORK_N)


# ---- case 6: subset bits beyond LDS ----------------------------------------------------------------------------------------
BIG_N = (N_LDS_LAST, N_LDS_LAST + 1)


def _case_big(n_refs):
    """Everything empty except ~200 clustered references and the record-form table once, at ids 0.., across the last words of
    the bit row (n_refs - 32 .. n_refs - 1) and scattered."""
    rng = np.random.default_rng(7606)
    scattered = np.sort(rng.choice(np.arange(1000, n_refs - 1000), 24 + 70, replace=False))
    # the 80 local ids of the form table: 0..23 stay, 24..47 scattered, 48..79 the last 32 references
    form_ids = np.concatenate([np.arange(24), scattered[:24], np.arange(n_refs - 32, n_refs)])
    table = form_entries(np.random.default_rng(7101))
    entries = {}
    for i, (_, _, _, h) in enumerate(table):
        entries[tuple(int(form_ids[x]) for x in h)] = 1 + i % 3
    # 200 clustered references, five to a cluster: 65 behind the low form ids, 70 scattered, 65 in front of the last words
    cl_ids = np.concatenate([np.arange(24, 89), scattered[24:], np.arange(n_refs - 32 - 65, n_refs - 32)])
    clusters = cl_ids.reshape(-1, 5)
    clusters[13] = (88, int(scattered[40]), n_refs - 96, n_refs - 64, n_refs - 33)      # one cluster spans all three regions
    for g in clusters.tolist():
        for h, m in ((g, 4), (g[:2], 3), (g[1:4], 2), (g[3:], 1)):
            entries[tuple(sorted(h))] = entries.get(tuple(sorted(h)), 0) + m
    used = sorted(set(form_ids.tolist()) | set(cl_ids.tolist()) | set(clusters.reshape(-1).tolist()))
    c = Case(f"big_{n_refs}", n_refs, list(entries.items()), private_refs=used, seed=6)
    c.notes["form_ids"] = form_ids
    last = n_refs - 1
    k9 = [tuple(int(form_ids[x]) for x in h) for k, place, _, h in table if k == 9 and place == "high"][0]
    c.subsets["last_alone"] = (last,)
    c.subsets["last_words"] = tuple(range(n_refs - 40, n_refs))
    c.subsets["both_sides"] = tuple(sorted(set(range(0, 24)) | set(range(n_refs - 34, n_refs)) | set(clusters[13].tolist())))
    c.subsets["k9_high_alone"] = (k9[-1],)
    c.extra_masks["last_alone"] = (0, n_refs - 2)
    return c


@functools.lru_cache(maxsize=None)
def cases_big():
    return tuple(_case_big(n) for n in BIG_N)


# ---- case 7: batch planes --------------------------------------------------------------------------------------------------
BATCH_B = (1, 64, 65, 256)
BATCH_AT = (0, 63, 64, 127, 128)


def batch_pairs(case):
    """(r, o) of a batch database: r shares a hash with o; one pair in the inline form, one in the list form where the
    database has one."""
    if case.name == "forms":
        out = []
        for k, place in ((2, "low"), (9, "mid")):
            _, _, t, h = [e for e in case.notes["table"] if e[0] == k and e[1] == place][0]
            out.append((t, [o for o in h if o != t][-1]))
        return out
    if case.name == "mult":
        return [(8, 9), (MULT_T, MULT_D)]
    raise KeyError(case.name)


def batch_block(case, b):
    """A block of b samples, as labels into batch_samples(case): position 63 hits every r only, 64 hits r and o, 127 hits r
    only again, 128 (the next plane) hits o only -- r's word there is zero -- position 0 is the shared sample and position
    b - 1 hits both; everything else is empty or noise."""
    at = {0: "shared", 63: "r_only", 64: "r_and_o", 127: "r_only", 128: "o_only"}
    labels = ["empty" if i % 2 else "noise" for i in range(b)]
    for pos, label in at.items():
        if pos < b:
            labels[pos] = label
    if b > 1:
        labels[b - 1] = "r_and_o"
    return labels


def batch_samples(case):
    pairs = batch_pairs(case)
    rs, os_ = [r for r, _ in pairs], [o for _, o in pairs]
    assert len(set(rs + os_)) == len(rs + os_)
    return {"shared": case.shared_sample(), "r_only": case.private_of(sorted(rs)), "o_only": case.private_of(sorted(os_)),
            "r_and_o": case.private_of(sorted(rs + os_)), "noise": case.noise, "empty": np.zeros(0, dtype=np.uint64)}


def batch_cases():
    return (case_forms(), case_mult())


# ---- all of them -----------------------------------------------------------------------------------------------------------
def small_cases():
    return (case_forms(),) + cases_recx() + cases_sweep() + (case_mult(),) + cases_work()


def all_cases():
    return small_cases() + cases_big()


def padded(case, sample, n=FUSED_1024_SAMPLE):
    """The sample widened to n hashes by hashes above everything the database holds: the size at which the fused step takes its
    1024-lane geometry, the overlaps unchanged."""
    top = int(case.noise[-1]) + 1
    pad = top + np.arange(1, n - sample.size + 1, dtype=np.uint64) * np.uint64(977)
    return np.concatenate([sample, pad])
