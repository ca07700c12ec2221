"""Cases for the organism x sample passes (yh_matrix_cells_device, yh_matrix_prevalence_device, yh_matrix_fill_device) as plain
data, and an oracle written with Python loops and dicts, independent of yacht_amd/matrix.py's numpy route.

Shape limits every case keeps (tests/test_matrix_cases_cpu.py checks them): N is 5 or 300 references, at most 3 * CHUNK rows or
cells, at most 320 samples, n_sets in 1..32, depth2 below 2^34.

A cells case:      dict(name, n_refs, rows uint32 [cap][5], n_rows, present uint8 [n_sets][cap], med float64 [cap] or None, base)
A prevalence case: dict(name, n_refs, cells, n_sets, n_samples, skip uint8 [n_samples] or None)
A fill case:       dict(name, n_refs, cells, n_sets, bit, n_samples, skip, kept bool [N], want_rel)
"""
import numpy as np

CHUNK = 1024  # YH_MATRIX_CHUNK
TILE = 2048  # YH_MATRIX_TILE
MAX_ROWS = 3 * CHUNK
MAX_SAMPLES = 320
CELL = np.dtype([("sample", np.uint32), ("ref", np.uint32), ("n_match", np.uint32), ("mask", np.uint32), ("depth2", np.uint64)])
assert CELL.itemsize == 24


# ---- the oracle -----------------------------------------------------------------------------------------------------------
def cells_oracle(rows, n_rows, present, med, base, n_refs):
    out = []
    cap = len(rows)
    for k in range(min(int(n_rows), cap)):
        smp, ref, _ov, _e, m = (int(x) for x in rows[k])
        if ref >= n_refs:
            continue
        mask = 0
        for c in range(len(present)):
            if present[c][k] != 0:
                mask |= 1 << c
        if mask:
            out.append((smp + int(base), ref, m, mask, 0 if med is None else int(2 * float(med[k]))))
    return np.array(out, dtype=CELL) if out else np.zeros(0, dtype=CELL)


def prevalence_oracle(cells, n_sets, n_samples, skip, n_refs):
    prev, denom = {}, {}
    for smp, ref, _m, mask, d2 in cells.tolist():
        if smp >= n_samples or ref >= n_refs or (skip is not None and skip[smp]):
            continue
        for c in range(n_sets):
            if (mask >> c) & 1:
                prev[(c, ref)] = prev.get((c, ref), 0) + 1
                denom[(c, smp)] = denom.get((c, smp), 0) + d2
    p = np.zeros((n_sets, n_refs), dtype=np.uint32)
    d = np.zeros((n_sets, n_samples), dtype=np.uint64)
    for (c, ref), v in prev.items():
        p[c, ref] = v
    for (c, smp), v in denom.items():
        assert v < 1 << 64
        d[c, smp] = v
    return p, d


def fill_oracle(cells, bit, n_samples, skip, row_of_ref, n_kept, denom_bit, want_rel):
    presence = np.zeros((n_kept, n_samples), dtype=np.uint8)
    n_match = np.zeros((n_kept, n_samples), dtype=np.uint32)
    rel = np.zeros((n_kept, n_samples), dtype=np.float64) if want_rel else None
    for smp, ref, m, mask, d2 in cells.tolist():
        if not (mask >> bit) & 1 or smp >= n_samples or ref >= len(row_of_ref) or (skip is not None and skip[smp]):
            continue
        r = int(row_of_ref[ref])
        if r < 0 or r >= n_kept:
            continue
        presence[r, smp], n_match[r, smp] = 1, m
        if want_rel:
            den = int(denom_bit[smp])
            rel[r, smp] = float(d2) / float(den) if den else 0.0
    return presence, n_match, rel


def row_of_ref(kept):
    out, r = [], 0
    for k in kept:
        out.append(r if k else -1)
        r += bool(k)
    return np.array(out, dtype=np.int32)


# ---- cells cases ------------------------------------------------------------------------------------------------------------
def _rows(rng, cap, n_refs, n_samples=7):
    rows = np.zeros((cap, 5), dtype=np.uint32)
    rows[:, 0] = rng.integers(0, n_samples, cap)
    rows[:, 1] = rng.integers(0, n_refs, cap)
    rows[:, 2:] = rng.integers(1, 1 << 20, (cap, 3))
    return rows


def _cells_case(name, rng, n_refs, cap, n_rows=None, n_sets=3, fill=0.4, med="half", base=0):
    rows = _rows(rng, cap, n_refs)
    present = (rng.random((n_sets, cap)) < fill).astype(np.uint8) * rng.integers(1, 256, (n_sets, cap)).astype(np.uint8)  # (any non-zero byte)
    m = None
    if med == "half":  # x.0 and x.5
        m = rng.integers(0, 4000, cap).astype(np.float64) / 2.0
    elif med == "large":
        m = np.full(cap, float(2 ** 32) - 0.5)
        m[::3] = 0.5
    return dict(name=name, n_refs=n_refs, rows=rows, n_rows=cap if n_rows is None else n_rows, present=present, med=m, base=base)


def cells_cases():
    rng = np.random.default_rng(20261021)
    out = [
        _cells_case("n_rows_0", rng, 5, 9, n_rows=0),
        _cells_case("n_rows_1", rng, 5, 9, n_rows=1, fill=1.0),
        _cells_case("n_rows_is_cap", rng, 5, 9),
        _cells_case("n_rows_above_cap", rng, 300, 70, n_rows=1000),
        _cells_case("cap_1", rng, 5, 1, fill=1.0),
    ]
    for n in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1):
        out.append(_cells_case(f"rows_{n}", rng, 300, n))
        out.append(_cells_case(f"rows_{n}_in_cap_{n + 5}", rng, 300, n + 5, n_rows=n, fill=0.9))
    out.append(_cells_case("none_present", rng, 300, CHUNK + 9, fill=0.0))
    out.append(_cells_case("all_present", rng, 300, CHUNK + 9, fill=1.0))
    ends = _cells_case("first_and_last_only", rng, 300, 2 * CHUNK + 7, fill=0.0)
    ends["present"][1, 0] = ends["present"][2, -1] = 1
    out.append(ends)
    for n_sets in (1, 7, 8, 32):
        out.append(_cells_case(f"n_sets_{n_sets}", rng, 300, 700, n_sets=n_sets, fill=0.2))
    top = _cells_case("bit_31_alone", rng, 5, 130, n_sets=32, fill=0.0)
    top["present"][31, 5::7] = 255
    out.append(top)
    bad = _cells_case("ref_out_of_range", rng, 5, 200, fill=1.0)
    bad["rows"][3::11, 1] = 5
    bad["rows"][7, 1] = 0xFFFFFFFF
    out.append(bad)
    out.append(_cells_case("no_medians", rng, 300, 300, med=None))
    out.append(_cells_case("large_medians", rng, 300, 300, med="large", fill=0.8))
    out.append(_cells_case("sample_base_256", rng, 300, CHUNK + 3, base=256))
    return out


# ---- prevalence cases -------------------------------------------------------------------------------------------------------
def _cells(entries):
    return np.array(entries, dtype=CELL) if len(entries) else np.zeros(0, dtype=CELL)


def _block_cells(rng, refs_samples, n_sets, depth=lambda rng: int(rng.integers(0, 1 << 12))):
    """Cells in (reference, sample) order, as a block leaves them: refs_samples = [(ref, [samples])]."""
    out = []
    for ref, samples in sorted(refs_samples):
        for smp in sorted(samples):
            out.append((smp, ref, int(rng.integers(1, 1000)), int(rng.integers(1, 1 << n_sets)), depth(rng)))
    return out


def prevalence_cases():
    rng = np.random.default_rng(77)
    out = []
    for S in (1, 63, 64, 65, 300):  # one reference present in S samples; beside it two others; 300: two blocks of cells
        blocks = [range(0, min(S, 256))] + ([range(256, S)] if S > 256 else [])
        cells = []
        for b in blocks:
            cells += _block_cells(rng, [(1, [s for s in b if s % 5 == 0]), (3, list(b)), (4, [s for s in b if s % 2])], 3)
        out.append(dict(name=f"one_ref_in_{S}_samples", n_refs=5, cells=_cells(cells), n_sets=3, n_samples=S, skip=None))
    # runs that cross a wave (64 cells) and a workgroup's tile: seven references of 290 samples, then one of 300 over cell TILE
    cells = _cells(_block_cells(rng, [(r, range(290)) for r in range(7)] + [(7, range(300)), (200, range(0, 300, 3))], 5))
    assert cells.size > TILE + 64 and cells["ref"][TILE - 1] == cells["ref"][TILE] == 7
    out.append(dict(name="run_over_wave_and_tile", n_refs=300, cells=cells, n_sets=5, n_samples=300, skip=None))
    out.append(dict(name="300_refs_one_cell_each", n_refs=300, n_sets=2, n_samples=40, skip=None,
                    cells=_cells(_block_cells(rng, [(r, [int(rng.integers(0, 40))]) for r in range(300)], 2))))
    big = _cells(_block_cells(rng, [(r, [0, 1]) for r in range(300)], 1, depth=lambda rng: (1 << 33) - 1))
    big["depth2"][big["sample"] == 1] = (1 << 31) + 1  # sample 1 crosses 2^32 at its second cell, sample 0 crosses 2^40
    out.append(dict(name="sums_over_2^32_and_2^40", n_refs=300, cells=big, n_sets=1, n_samples=2, skip=None))
    base = _block_cells(rng, [(r, [s for s in range(40) if (s + r) % 3]) for r in range(0, 300, 7)], 4)
    for name, skip in (("skip_first", [0]), ("skip_last", [39]), ("skip_all", list(range(40)))):
        sk = np.zeros(40, dtype=np.uint8)
        sk[skip] = 1 + (len(skip) % 200)  # (any non-zero byte)
        out.append(dict(name=name, n_refs=300, cells=_cells(base), n_sets=4, n_samples=40, skip=sk))
    out.append(dict(name="no_cells", n_refs=5, cells=_cells([]), n_sets=3, n_samples=4, skip=None))
    wide = _block_cells(rng, [(r, [s for s in range(320) if (s * 7 + r) % 4 == 0]) for r in range(0, 300, 9)], 32)
    out.append(dict(name="32_sets_320_samples", n_refs=300, cells=_cells(wide), n_sets=32, n_samples=320, skip=None))
    stray = _cells(base)
    stray["sample"][5], stray["ref"][9] = 40, 300  # out of range: ignored
    out.append(dict(name="out_of_range_cells", n_refs=300, cells=stray, n_sets=4, n_samples=40, skip=None))
    shuffled = _cells(base)
    rng.shuffle(shuffled)  # (host-made cells arrive in any order)
    out.append(dict(name="any_order", n_refs=300, cells=shuffled, n_sets=4, n_samples=40, skip=None))
    return out


# ---- fill cases -------------------------------------------------------------------------------------------------------------
def fill_cases():
    rng = np.random.default_rng(5)
    out = []
    small = _cells(_block_cells(rng, [(0, [0, 2, 3]), (2, [1, 2]), (4, [0, 1, 2, 3])], 3))
    small["mask"] |= 2  # (bit 1 everywhere)
    for name, kept in (("n_kept_0", [0] * 5), ("n_kept_1", [0, 0, 1, 0, 0]), ("n_kept_N", [1] * 5), ("dropped_refs", [1, 0, 0, 0, 1])):
        out.append(dict(name=name, n_refs=5, cells=small, n_sets=3, bit=1, n_samples=4, skip=None, kept=np.array(kept, bool), want_rel=True))
    one = _cells(_block_cells(rng, [(r, [0]) for r in (0, 1, 3)], 2))
    one["mask"] |= 1
    out.append(dict(name="one_sample", n_refs=5, cells=one, n_sets=2, bit=0, n_samples=1, skip=None, kept=np.ones(5, bool), want_rel=True))
    mid = _cells(_block_cells(rng, [(r, [s for s in range(300) if (s + r) % 5 < 2]) for r in range(0, 300, 12)], 6))
    sk = np.zeros(300, dtype=np.uint8)
    sk[[0, 17, 299]] = 1
    kept = np.zeros(300, bool)
    kept[::6] = True
    out.append(dict(name="skipped_samples", n_refs=300, cells=mid, n_sets=6, bit=2, n_samples=300, skip=sk, kept=kept, want_rel=True))
    out.append(dict(name="no_rel", n_refs=300, cells=mid, n_sets=6, bit=5, n_samples=300, skip=None, kept=kept, want_rel=False))
    off = mid.copy()
    off["mask"] &= ~np.uint32(8)
    out.append(dict(name="bit_in_no_cell", n_refs=300, cells=off, n_sets=6, bit=3, n_samples=300, skip=None, kept=kept, want_rel=True))
    zero = mid.copy()
    zero["depth2"][zero["sample"] == 4] = 0  # a sample present in references whose depths are all 0: its denominator is 0
    out.append(dict(name="zero_denominator", n_refs=300, cells=zero, n_sets=6, bit=0, n_samples=300, skip=None, kept=np.ones(300, bool), want_rel=True))
    out.append(dict(name="no_cells", n_refs=5, cells=_cells([]), n_sets=1, bit=0, n_samples=3, skip=None, kept=np.ones(5, bool), want_rel=True))
    return out
