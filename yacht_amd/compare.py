"""`yacht compare` and `yacht run --compare`: how the samples of a cohort resemble one another.

The device answers exact integers for every pair of samples (yh_compare, include/yacht_hip.h): the shared hashes, the sum
of the smaller abundances, the 128-bit sum of the abundance products, and per sample its size, abundance sum and 128-bit
sum of squares.  Everything else here is numpy on those integers, in float64: the metrics, the long table
results/cohort_compare.tsv and one results/cohort_compare_<metric>.csv per matrix metric in `sourmash compare --csv` layout.
A sketch without abundances counts every hash once, as in the other passes.

A cohort that does not fit the device at once is compared in panels of consecutive samples: YACHT_COMPARE_PANEL_BYTES
(default 1 GiB of hashes, abundances and keep bytes, 13 bytes a hash) bounds a panel, which holds at least two samples and
at most YH_COMPARE_MAX_SAMPLES; each panel pair p <= q is one call.  The integers of a pair do not depend on the panel it
fell into, so neither do the files.

Two routes fill the same matrix (yh_compare_routed): the dense tiles, which merge every pair in full, and the sparse route
through the hashes that are shared.  YACHT_COMPARE_ROUTE = auto (default: chosen per call from a sample of the hash space),
dense or sparse; the files are byte for byte the same under all three.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import time
import zipfile
from pathlib import Path
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import YH_COMPARE_MAX_SAMPLES

# one cell / one self row of yh_compare (include/yacht_hip.h: yh_compare_cell, yh_compare_self)
CELL_DTYPE = np.dtype([("n_shared", np.uint64), ("sum_min", np.uint64), ("dot_lo", np.uint64), ("dot_hi", np.uint64)])
SELF_DTYPE = np.dtype([("n_kept", np.uint64), ("sum", np.uint64), ("sq_lo", np.uint64), ("sq_hi", np.uint64)])

METRICS = ("jaccard", "containment_a_in_b", "containment_b_in_a", "max_containment", "ani_max_containment", "bray_curtis",
           "cosine", "angular_similarity")
MATRIX_METRICS = ("jaccard", "containment", "bray_curtis", "angular_similarity")  # one cohort_compare_<metric>.csv each
TABLE_COLUMNS = ["sample_a", "sample_b", "n_hashes_a", "n_hashes_b", "n_shared", *METRICS, "abund_sum_min"]
TABLE_NAME = "cohort_compare.tsv"
RESIDUAL_TABLE_NAME = "cohort_compare_residual.tsv"
MATRIX_NAME = "cohort_compare_{0}.csv"
PANEL_BYTES_ENV = "YACHT_COMPARE_PANEL_BYTES"
PANEL_BYTES_DEFAULT = 1 << 30
BYTES_PER_HASH = 13  # hash, abundance, keep byte
ROUTE_ENV = "YACHT_COMPARE_ROUTE"
ROUTES = {"dense": _lib.YH_COMPARE_ROUTE_DENSE, "sparse": _lib.YH_COMPARE_ROUTE_SPARSE, "auto": _lib.YH_COMPARE_ROUTE_AUTO}
ROUTE_NAMES = {v: k for k, v in ROUTES.items()}
MSG_NEEDS_TWO = "Comparing samples needs two or more --sample_file, not {0}."
MSG_COMPARE_NEEDS_COHORT = "--compare compares the samples of a cohort with one another: it needs two or more --sample_file, not {0}."
MSG_SCALED_DIFFER = "The samples' scale factors differ ({0} has {1}, {2} has {3}): sketches of different `scaled` are not compared."


def _ptr(a: Optional[np.ndarray]) -> C.c_void_p:
    return C.c_void_p(0 if a is None else a.ctypes.data)


def pack(samples: Sequence[np.ndarray], abunds=None, keeps=None):
    """(values, offsets, abundances or None, keep bytes or None) of a set of samples as yh_compare takes them.  abunds /
    keeps: None, or one entry per sample, each an array parallel to the hashes or None (abundance 1 / keep byte 0
    everywhere).  The abundances are None when no sample has any; the keep bytes likewise."""
    from .engine import check_abundances, pack_csr

    samples = [np.ascontiguousarray(s, dtype=np.uint64) for s in samples]
    values, offsets = pack_csr(samples)
    cat_ab = cat_keep = None
    if abunds is not None:
        if len(abunds) != len(samples):
            raise ValueError(f"{len(abunds)} abundance arrays for {len(samples)} samples")
        if any(a is not None for a in abunds):
            parts = [np.ones(s.size, dtype=np.uint32) if a is None else check_abundances(s, a)[1] for s, a in zip(samples, abunds)]
            cat_ab = np.ascontiguousarray(np.concatenate(parts), dtype=np.uint32)
    if keeps is not None:
        if len(keeps) != len(samples):
            raise ValueError(f"{len(keeps)} keep arrays for {len(samples)} samples")
        if any(k is not None for k in keeps):
            parts = [np.zeros(s.size, dtype=np.uint8) if k is None else np.ascontiguousarray(k, dtype=np.uint8) for s, k in zip(samples, keeps)]
            for s, k in zip(samples, parts):
                if k.size != s.size:
                    raise ValueError(f"{k.size} keep bytes for {s.size} sample hashes")
            cat_keep = np.ascontiguousarray(np.concatenate(parts), dtype=np.uint8)
    return values, offsets, cat_ab, cat_keep


def route_code(route=None) -> int:
    """The route as yh_compare_routed takes it: "auto", "dense" or "sparse"; None reads YACHT_COMPARE_ROUTE (default auto).
    Any other word raises ValueError."""
    word = os.environ.get(ROUTE_ENV, "auto") if route is None else route
    if isinstance(word, str):
        word = word.strip().lower() or "auto"
    if word not in ROUTES:
        raise ValueError(f"{ROUTE_ENV if route is None else 'route'} must be one of auto, dense, sparse, not {word!r}")
    return ROUTES[word]


class Result(tuple):
    """What compare_packed / compare / compare_cohort return: the tuple their callers unpack, with the routes' figures on
    the side.  compare_packed: .info, the fields of yh_compare_sparse_info as a dict (route as its name).  compare_cohort:
    .routes, one (p, q, route name, n_pair_updates) per panel pair."""
    info: Optional[dict] = None
    routes: Optional[list] = None


def compare_packed(a, b=None, keep_and: int = 0, keep_eq: int = 0, device: int = 0, ld_cells: Optional[int] = None, cells=None,
                   route=None):
    """yh_compare_routed on packed sets (what pack returns); b None: the symmetric call, A against itself.  Returns (cells
    [n_a, ld_cells] of CELL_DTYPE, self_a [n_a], self_b [n_b] of SELF_DTYPE), a Result whose .info holds the route taken and
    its figures.  cells: a buffer to write into (its columns behind n_b stay as they are).  route: see route_code."""
    code = route_code(route)
    lib = _lib.load()
    sym = b is None
    if sym:
        b = a
    n_a, n_b = a[1].size - 1, b[1].size - 1
    ld = n_b if ld_cells is None else int(ld_cells)
    if cells is None:
        cells = np.zeros((n_a, ld), dtype=CELL_DTYPE)
    self_a = np.zeros(n_a, dtype=SELF_DTYPE)
    self_b = self_a if sym else np.zeros(n_b, dtype=SELF_DTYPE)
    info = _lib.CompareSparseInfo()
    _lib.check(lib.yh_compare_routed(_ptr(a[0]), _ptr(a[1]), _ptr(a[2]), _ptr(a[3]), n_a, _ptr(b[0]), _ptr(b[1]), _ptr(b[2]),
                                     _ptr(b[3]), n_b, int(keep_and), int(keep_eq), int(device), _ptr(cells), ld, _ptr(self_a),
                                     _ptr(self_b), code, C.byref(info)))
    out = Result((cells, self_a, self_b))
    out.info = {f: int(getattr(info, f)) for f, _ in info._fields_}
    out.info["route"] = ROUTE_NAMES[out.info["route"]]
    return out


def compare(samples_a, samples_b=None, abunds_a=None, abunds_b=None, keeps_a=None, keeps_b=None, keep_and: int = 0,
            keep_eq: int = 0, device: int = 0, route=None):
    """Every sample of A against every sample of B (samples_b None: of A itself, the symmetric call) in one call of
    yh_compare_routed.  A hash takes part iff its side has no keep bytes or (keep & keep_and) == keep_eq.  Returns (cells,
    self_a, self_b) as compare_packed does."""
    a = pack(samples_a, abunds_a, keeps_a)
    b = None if samples_b is None else pack(samples_b, abunds_b, keeps_b)
    return compare_packed(a, b, keep_and, keep_eq, device, route=route)


def work_bytes(n_a: int, n_b: int, total_a: int, total_b: int) -> int:
    return int(_lib.load().yh_compare_work_bytes(int(n_a), int(n_b), int(total_a), int(total_b)))


def compare_device(d_a: int, d_a_off: int, d_a_abund: int, d_a_keep: int, n_a: int, total_a: int, d_b: int, d_b_off: int,
                   d_b_abund: int, d_b_keep: int, n_b: int, total_b: int, keep_and: int, keep_eq: int, d_cells: int, ld_cells: int,
                   d_self_a: int, d_self_b: int, d_work: int, n_work_bytes: int, stream: int = 0) -> None:
    """yh_compare_device: everything on device buffers (addresses; 0 = NULL), enqueued on `stream` without a host sync."""
    v = C.c_void_p
    _lib.check(_lib.load().yh_compare_device(v(d_a), v(d_a_off), v(d_a_abund), v(d_a_keep), int(n_a), int(total_a), v(d_b), v(d_b_off),
                                             v(d_b_abund), v(d_b_keep), int(n_b), int(total_b), int(keep_and), int(keep_eq), v(d_cells),
                                             int(ld_cells), v(d_self_a), v(d_self_b), v(d_work), int(n_work_bytes), v(stream)))


def sparse_work_bytes(n_a: int, n_b: int, total_a: int, total_b: int) -> int:
    return int(_lib.load().yh_compare_sparse_work_bytes(int(n_a), int(n_b), int(total_a), int(total_b)))


def compare_sparse_device(d_a: int, d_a_off: int, d_a_abund: int, d_a_keep: int, n_a: int, total_a: int, d_b: int, d_b_off: int,
                          d_b_abund: int, d_b_keep: int, n_b: int, total_b: int, keep_and: int, keep_eq: int, d_cells: int,
                          ld_cells: int, d_self_a: int, d_self_b: int, d_work: int, n_work_bytes: int, stream: int = 0,
                          hash_bits: int = 64, d_info: int = 0) -> None:
    """yh_compare_sparse_device: the sparse route on device buffers (addresses; 0 = NULL), enqueued on `stream` without a
    host sync.  hash_bits: every hash is below 2**hash_bits.  d_info: room for one yh_compare_sparse_info, or 0."""
    v = C.c_void_p
    _lib.check(_lib.load().yh_compare_sparse_device(v(d_a), v(d_a_off), v(d_a_abund), v(d_a_keep), int(n_a), int(total_a), v(d_b),
                                                    v(d_b_off), v(d_b_abund), v(d_b_keep), int(n_b), int(total_b), int(keep_and),
                                                    int(keep_eq), v(d_cells), int(ld_cells), v(d_self_a), v(d_self_b), v(d_work),
                                                    int(n_work_bytes), v(stream), int(hash_bits), v(d_info)))


def sparse_count_device(d_a: int, d_a_off: int, d_a_keep: int, n_a: int, total_a: int, d_b: int, d_b_off: int, d_b_keep: int, n_b: int,
                        total_b: int, keep_and: int, keep_eq: int, d_work: int, n_work_bytes: int, stream: int, hash_bits: int,
                        d_info: int) -> None:
    """yh_compare_sparse_count_device: the sparse route's grouping alone (records, sort, runs), its figures left in d_info."""
    v = C.c_void_p
    _lib.check(_lib.load().yh_compare_sparse_count_device(v(d_a), v(d_a_off), v(d_a_keep), int(n_a), int(total_a), v(d_b), v(d_b_off),
                                                          v(d_b_keep), int(n_b), int(total_b), int(keep_and), int(keep_eq), v(d_work),
                                                          int(n_work_bytes), v(stream), int(hash_bits), v(d_info)))


# ---- metrics -------------------------------------------------------------------------------------------------------------------
def wide(lo, hi) -> np.ndarray:
    """A 128-bit sum as float64: the SPLIT INTO TWO DOUBLES, hi * 2**64 + lo (each half converts exactly or rounds once; the
    sum rounds once more: a relative error of a few 2**-53)."""
    return np.asarray(hi, dtype=np.float64) * 18446744073709551616.0 + np.asarray(lo, dtype=np.float64)


def _ratio(num, den) -> np.ndarray:
    num, den = np.broadcast_arrays(np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64))
    out = np.zeros(num.shape, dtype=np.float64)
    np.divide(num, den, out=out, where=den > 0)
    return out


def metrics(cells: np.ndarray, self_a: np.ndarray, self_b: np.ndarray, ksize: int) -> Dict[str, np.ndarray]:
    """The metrics of every cell, float64 [n_a, n_b], from the exact integers (the 128-bit sums through `wide`):
      jaccard              n_shared / (n_a + n_b - n_shared)
      containment_a_in_b   n_shared / n_a            containment_b_in_a   n_shared / n_b
      max_containment      n_shared / min(n_a, n_b)
      ani_max_containment  max_containment ** (1 / ksize), 0.0 at containment 0: the plain point estimate, no confidence interval
      bray_curtis          1 - 2 * sum_min / (sum_a + sum_b)     (a dissimilarity)
      cosine               dot / (sqrt(sq_a) * sqrt(sq_b))
      angular_similarity   1 - 2 * acos(cosine) / pi
    n, sum and sq are the self rows' kept hashes, abundance sum and sum of squares.  A pair in which a denominator is 0
    (an empty sample, a mask that keeps nothing) gives 0.0 for every similarity and 1.0 for bray_curtis."""
    n_sh = cells["n_shared"].astype(np.float64)
    n_a = self_a["n_kept"].astype(np.float64)[:, None]
    n_b = self_b["n_kept"].astype(np.float64)[None, :]
    out = {"jaccard": _ratio(n_sh, n_a + n_b - n_sh), "containment_a_in_b": _ratio(n_sh, n_a), "containment_b_in_a": _ratio(n_sh, n_b)}
    out["max_containment"] = _ratio(n_sh, np.minimum(n_a, n_b))
    out["ani_max_containment"] = np.where(out["max_containment"] > 0, np.power(out["max_containment"], 1.0 / float(ksize)), 0.0)
    s_ab = self_a["sum"].astype(np.float64)[:, None] + self_b["sum"].astype(np.float64)[None, :]
    out["bray_curtis"] = np.where(s_ab > 0, 1.0 - _ratio(2.0 * cells["sum_min"].astype(np.float64), s_ab), 1.0)
    norm = np.sqrt(wide(self_a["sq_lo"], self_a["sq_hi"]))[:, None] * np.sqrt(wide(self_b["sq_lo"], self_b["sq_hi"]))[None, :]
    out["cosine"] = np.minimum(_ratio(wide(cells["dot_lo"], cells["dot_hi"]), norm), 1.0)
    out["angular_similarity"] = np.where(norm > 0, 1.0 - 2.0 * np.arccos(out["cosine"]) / math.pi, 0.0)
    return out


def diagonal_from_self(cells: np.ndarray, self_rows: np.ndarray) -> np.ndarray:
    """The square matrix with cell (i, i) taken from self row i: a sample shares all its kept hashes with itself."""
    cells = cells.copy()
    i = np.arange(self_rows.size)
    cells["n_shared"][i, i], cells["sum_min"][i, i] = self_rows["n_kept"], self_rows["sum"]
    cells["dot_lo"][i, i], cells["dot_hi"][i, i] = self_rows["sq_lo"], self_rows["sq_hi"]
    return cells


# ---- the files -----------------------------------------------------------------------------------------------------------------
def table_frame(stems: Sequence[str], cells: np.ndarray, self_rows: np.ndarray, ksize: int):
    """results/cohort_compare.tsv: one row per unordered pair i < j, in input order (TABLE_COLUMNS)."""
    import pandas as pd

    n = len(stems)
    m = metrics(cells, self_rows, self_rows, ksize)
    i, j = np.triu_indices(n, 1)
    stems = np.asarray(list(stems), dtype=object)
    data = {"sample_a": stems[i], "sample_b": stems[j], "n_hashes_a": self_rows["n_kept"][i], "n_hashes_b": self_rows["n_kept"][j],
            "n_shared": cells["n_shared"][i, j]}
    for k in METRICS:
        data[k] = m[k][i, j]
    data["abund_sum_min"] = cells["sum_min"][i, j]
    return pd.DataFrame(data, columns=TABLE_COLUMNS)


def matrices(cells: np.ndarray, self_rows: np.ndarray, ksize: int) -> Dict[str, np.ndarray]:
    """The matrix metrics, n x n, the diagonal from the self rows.  `containment` is asymmetric: row in column."""
    m = metrics(diagonal_from_self(cells, self_rows), self_rows, self_rows, ksize)
    return {"jaccard": m["jaccard"], "containment": m["containment_a_in_b"], "bray_curtis": m["bray_curtis"],
            "angular_similarity": m["angular_similarity"]}


def write_matrix_csv(path: str, stems: Sequence[str], matrix: np.ndarray) -> None:
    """The layout of `sourmash compare --csv`: a header row of sample names, then n rows of n values."""
    import csv

    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(list(stems))
        for row in np.asarray(matrix, dtype=np.float64):
            w.writerow([repr(float(x)) for x in row])


def write_outputs(results_folder: str, stems: Sequence[str], cells: np.ndarray, self_rows: np.ndarray, ksize: int) -> None:
    table_frame(stems, cells, self_rows, ksize).to_csv(os.path.join(results_folder, TABLE_NAME), sep="\t", index=False)
    for name, mat in matrices(cells, self_rows, ksize).items():
        write_matrix_csv(os.path.join(results_folder, MATRIX_NAME.format(name)), stems, mat)


# ---- panels --------------------------------------------------------------------------------------------------------------------
def panel_bytes() -> int:
    return max(1, int(os.environ.get(PANEL_BYTES_ENV, PANEL_BYTES_DEFAULT)))


def plan_panels(n_hashes: Sequence[int], budget: int) -> List[range]:
    """Consecutive samples cut into panels: a panel takes samples while it stays within the budget (BYTES_PER_HASH a hash)
    and YH_COMPARE_MAX_SAMPLES, and always at least two (the last panel may be left with one)."""
    panels, start, used = [], 0, 0
    for i, n in enumerate(n_hashes):
        size = int(n) * BYTES_PER_HASH
        count = i - start
        if count >= 2 and (used + size > budget or count >= YH_COMPARE_MAX_SAMPLES):
            panels.append(range(start, i))
            start, used = i, 0
        used += size
    if start < len(n_hashes):
        panels.append(range(start, len(n_hashes)))
    return panels


def compare_cohort(n_hashes: Sequence[int], load: Callable[[range], Tuple[list, list, list]], keep_and: int = 0, keep_eq: int = 0,
                   device: int = 0, budget: Optional[int] = None, route=None):
    """All samples against all, in panels.  load(panel) returns the panel's (samples, abunds, keeps) for `pack`.  Each panel
    pair p <= q is one call (p == q: the symmetric call), on the route `route` names or chooses; the block (q, p) is
    (p, q)'s transpose.  Returns (cells [n, n], self rows [n], seconds inside the calls), a Result whose .routes lists per
    panel pair the route taken and its cell updates."""
    code = route_code(route)
    route = ROUTE_NAMES[code]
    routes = []
    n = len(n_hashes)
    panels = plan_panels(n_hashes, panel_bytes() if budget is None else int(budget))
    cells = np.zeros((n, n), dtype=CELL_DTYPE)
    self_rows = np.zeros(n, dtype=SELF_DTYPE)
    seconds = 0.0
    for p, pp in enumerate(panels):
        a = pack(*load(pp))
        for q in range(p, len(panels)):
            pq = panels[q]
            b = None if q == p else pack(*load(pq))
            t0 = time.perf_counter()
            res = compare_packed(a, b, keep_and, keep_eq, device, route=route)
            seconds += time.perf_counter() - t0
            got, s_a, s_b = res
            routes.append((p, q, res.info["route"], res.info["n_pair_updates"]))
            cells[pp.start:pp.stop, pq.start:pq.stop] = got
            self_rows[pp.start:pp.stop] = s_a
            if q != p:
                cells[pq.start:pq.stop, pp.start:pp.stop] = got.T
                self_rows[pq.start:pq.stop] = s_b
    out = Result((cells, self_rows, seconds))
    out.routes = routes
    return out


# ---- `yacht compare` -----------------------------------------------------------------------------------------------------------
def add_arguments(parser) -> None:
    parser.add_argument("--sample_file", required=True, nargs="+", help="Two or more samples in .sig.zip format.")
    parser.add_argument("--ksize", type=int, required=True, help="The k-mer size of the sketches to compare.")
    parser.add_argument("--num_threads", type=int, default=16, help="Host threads for file handling.")
    parser.add_argument("--outdir", type=str, default=os.getcwd(), help="Where the 'results' folder is created.")


def check_inputs(files: Sequence[str], ksize: int, outdir: str, num_threads: int = 16) -> dict:
    """The checks the cohort run makes on its sample files, before any device work and before anything is written: two or
    more files, distinct stems, per file the archive's manifest and exactly one sketch of the k-mer size, and one `scaled`
    for all.  Returns paths, stems and meta[i] = (n_hashes, mean_abundance, scaled)."""
    from concurrent.futures import ThreadPoolExecutor

    from . import cohort, run_YACHT as ry, utils

    if len(files) < 2:
        raise ValueError(MSG_NEEDS_TWO.format(len(files)))
    paths = [str(Path(f).absolute()) for f in files]
    outdir = str(Path(outdir).absolute())
    for p in paths:
        utils.check_file_existence(p, f"Sample file {p} does not exist.")
    if not os.access(outdir, os.W_OK):
        raise PermissionError(f"Cannot write to the location: {outdir}.")
    seen: Dict[str, str] = {}
    for p in paths:
        stem = cohort.sample_stem(p)
        if stem in seen:
            raise ValueError(f"Two sample files share the name {stem!r}: {seen[stem]} and {p}")
        seen[stem] = p
    for p in paths:
        with zipfile.ZipFile(p, "r") as z:
            if "SOURMASH-MANIFEST.csv" not in z.namelist():
                raise FileNotFoundError(ry.MSG_ZIP_WITHOUT_MANIFEST.format(p))
    with ThreadPoolExecutor(max(1, min(int(num_threads), len(paths)))) as ex:
        parsed = list(ex.map(lambda p: cohort._check_one(p, ksize), paths))
    meta = []
    for p, (m, err) in zip(paths, parsed):
        if err is not None:
            raise err
        if m[2] != parsed[0][0][2]:
            raise ValueError(MSG_SCALED_DIFFER.format(paths[0], parsed[0][0][2], p, m[2]))
        meta.append(m)
    return dict(paths=paths, outdir=outdir, stems=[cohort.sample_stem(p) for p in paths], meta=meta)


def file_loader(paths: Sequence[str], ksize: int, num_threads: int = 16, keeps: Optional[Sequence] = None):
    """load(panel) for compare_cohort over sample files: the hashes and, where a sketch tracks them, its abundances;
    keeps[i] (or None) are sample i's keep bytes."""
    from concurrent.futures import ThreadPoolExecutor

    from . import cohort

    def load(panel):
        with ThreadPoolExecutor(max(1, min(int(num_threads), len(panel)))) as ex:
            got = list(ex.map(lambda i: cohort._load_for_residual(paths[i], ksize, False), panel))
        return [g[0] for g in got], [g[1] for g in got], None if keeps is None else [keeps[i] for i in panel]

    return load


def run_files(paths: Sequence[str], stems: Sequence[str], meta: Sequence, ksize: int, results_folder: str, num_threads: int = 16,
              residual_keeps: Optional[Sequence] = None) -> float:
    """Compare the sample files and write cohort_compare.tsv and the matrices into results_folder; with residual_keeps
    (per sample uint8 [n_hashes], 1 = explained, or None = nothing explained) also cohort_compare_residual.tsv over the
    hashes whose byte is 0.  Returns the seconds inside the device calls."""
    from .utils import logger

    n_hashes = [m[0] for m in meta]
    route = ROUTE_NAMES[route_code(None)]  # (a bad YACHT_COMPARE_ROUTE stops here, before any device work)
    first = compare_cohort(n_hashes, file_loader(paths, ksize, num_threads), route=route)
    cells, self_rows, seconds = first
    routes = list(first.routes)
    write_outputs(results_folder, stems, cells, self_rows, ksize)
    if residual_keeps is not None:
        second = compare_cohort(n_hashes, file_loader(paths, ksize, num_threads, residual_keeps), keep_and=1, keep_eq=0, route=route)
        r_cells, r_self, more = second
        routes += second.routes
        table_frame(stems, r_cells, r_self, ksize).to_csv(os.path.join(results_folder, RESIDUAL_TABLE_NAME), sep="\t", index=False)
        seconds += more
    n_sparse = sum(1 for r in routes if r[2] == "sparse")
    logger.info(f"{len(routes)} panel pairs: {n_sparse} sparse, {len(routes) - n_sparse} dense "
                f"({sum(r[3] for r in routes)} cell updates on the sparse route; {ROUTE_ENV}={route})")
    return seconds


def main(args) -> None:
    from .utils import logger

    files = [args.sample_file] if isinstance(args.sample_file, str) else list(args.sample_file)
    plan = check_inputs(files, int(args.ksize), args.outdir, args.num_threads)
    results_folder = os.path.join(plan["outdir"], "results")
    os.makedirs(results_folder, exist_ok=True)
    run_files(plan["paths"], plan["stems"], plan["meta"], int(args.ksize), results_folder, args.num_threads)
    logger.info(f"Saved the comparison of {len(files)} samples to {results_folder}.")
