"""`yacht run --matrix` of a cohort: the organism x sample tables.

Every block of a cohort run leaves, on the device, its compact rows, the present bytes of the presence test and (with
--abundance) the median depth at those rows.  yh_matrix_cells_device turns the rows some coverage calls present into cells
(engine.MATRIX_CELL_DTYPE: sample, ref, n_match, a mask with one bit per user coverage, twice the median depth) that stay on
the device, block behind block.  After the last block yh_matrix_prevalence_device counts, per coverage, the samples every
reference is present in and sums every sample's depths; the references to keep are chosen here from those counts, and
yh_matrix_fill_device stores the kept cells into the wide matrices of --matrix_coverage.  Files, under results/:

  cohort_prevalence.tsv                   per user coverage (descending) and organism present in >= 1 sample (database order):
                                          n_samples_present, f_samples_present; with --abundance mean_ and max_relative_abundance
  cohort_matrix_presence.tsv              organism_name, then one column per sample stem in input order: 0 / 1
  cohort_matrix_num_matches.tsv           the same shape: num_matches where present, 0 elsewhere
  cohort_matrix_relative_abundance.tsv    (--abundance) the same shape: the relative_abundance of the sample's own table

Rows are references in DATABASE order: a manifest with a repeated organism_name keeps one row per reference, so the name
repeats.  A sample whose tables the host recomputed (such a manifest) is skipped on the device (skip byte 1) and its cells are
made here from its tables; they enter the passes under an alias column behind the cohort's own, folded back after the fill.
YACHT_COHORT_MATRIX=host makes every sample's cells here and builds the tables with numpy: the same files, byte for byte.
"""
from __future__ import annotations

import os
import time
from typing import List, Optional, Sequence

import numpy as np
import pandas as pd

from . import _lib
from .engine import MATRIX_CELL_DTYPE

MAX_SETS = _lib.YH_MATRIX_MAX_SETS
MAX_BYTES = 4 << 30  # the wide matrices of --matrix_coverage together
SLAB_BYTES = 1 << 28  # a slab of rows of the per-coverage abundance statistics
PREVALENCE_NAME = "cohort_prevalence.tsv"
PRESENCE_NAME = "cohort_matrix_presence.tsv"
NUM_MATCHES_NAME = "cohort_matrix_num_matches.tsv"
ABUNDANCE_NAME = "cohort_matrix_relative_abundance.tsv"
PREVALENCE_COLUMNS = ["min_coverage", "organism_name", "n_samples_present", "f_samples_present"]
PREVALENCE_ABUNDANCE_COLUMNS = ["mean_relative_abundance", "max_relative_abundance"]  # behind them with --abundance
ENV = "YACHT_COHORT_MATRIX"

MSG_MATRIX_NEEDS_COHORT = "--matrix builds the organism x sample tables of a cohort: it needs two or more --sample_file, not {0}."
MSG_COVERAGE_WITHOUT_MATRIX = "--matrix_coverage needs --matrix."
MSG_COVERAGE_NOT_LISTED = "--matrix_coverage {0} is not one of the --min_coverage_list values {1}."
MSG_MIN_SAMPLES_WITHOUT_MATRIX = "--matrix_min_samples needs --matrix."
MSG_BAD_MIN_SAMPLES = "--matrix_min_samples must be at least 1, not {0}."
MSG_TOO_MANY_COVERAGES = "--matrix takes at most 32 --min_coverage_list values, not {0}: a cell carries one bit per coverage."
MSG_BAD_ROUTE = "YACHT_COHORT_MATRIX={0!r} is not understood: unset it, or set it to 'host'."
MSG_TOO_LARGE = ("The matrices of {0} organisms x {1} samples would take {2} bytes, more than {3}: "
                 "raise --matrix_min_samples to keep fewer organisms.")


def matrix_options(args, n_files: int):
    """None without --matrix, else (the coverage whose wide tables are written, the fewest samples an organism must be present
    in, whether the host makes every cell).  ValueError for every combination the command refuses.  Host only."""
    want = bool(getattr(args, "matrix", False))
    cov, m = getattr(args, "matrix_coverage", None), getattr(args, "matrix_min_samples", None)
    if not want:
        if cov is not None:
            raise ValueError(MSG_COVERAGE_WITHOUT_MATRIX)
        if m is not None:
            raise ValueError(MSG_MIN_SAMPLES_WITHOUT_MATRIX)
        return None
    if n_files < 2:
        raise ValueError(MSG_MATRIX_NEEDS_COHORT.format(n_files))
    word = os.environ.get(ENV)
    if word not in (None, "", "host"):
        raise ValueError(MSG_BAD_ROUTE.format(word))
    listed = sorted(set(float(c) for c in args.min_coverage_list), reverse=True)
    if len(listed) > MAX_SETS:
        raise ValueError(MSG_TOO_MANY_COVERAGES.format(len(listed)))
    if m is not None and int(m) < 1:
        raise ValueError(MSG_BAD_MIN_SAMPLES.format(m))
    if cov is None:
        cov = listed[-1]
    elif float(cov) not in listed:
        raise ValueError(MSG_COVERAGE_NOT_LISTED.format(cov, listed))
    return float(cov), 1 if m is None else int(m), word == "host"


# ---- the numpy route -----------------------------------------------------------------------------------------------------
def cells_from_rows(rows, n_rows: int, present, med, base: int, n_refs: int) -> np.ndarray:
    """What yh_matrix_cells_device writes: rows uint32 [cap][5] (sample, ref, overlap, n_excl, n_match), present uint8
    [n_sets][cap], med float64 [cap] or None."""
    rows = np.asarray(rows, dtype=np.uint32).reshape(-1, 5)
    present = np.asarray(present, dtype=np.uint8).reshape(-1, rows.shape[0])
    n = min(int(n_rows), rows.shape[0])
    mask = np.zeros(n, dtype=np.uint32)
    for c in range(present.shape[0]):
        mask |= (present[c, :n] != 0).astype(np.uint32) << np.uint32(c)
    mask[rows[:n, 1] >= n_refs] = 0
    at = np.flatnonzero(mask)
    cells = np.zeros(at.size, dtype=MATRIX_CELL_DTYPE)
    cells["sample"] = rows[at, 0] + np.uint32(base)
    cells["ref"], cells["n_match"], cells["mask"] = rows[at, 1], rows[at, 4], mask[at]
    if med is not None:
        cells["depth2"] = depth2_of(np.asarray(med, dtype=np.float64)[at])
    return cells


def depth2_of(med: np.ndarray) -> np.ndarray:
    """Twice a median depth (x.0 or x.5, NaN where nothing matched) as uint64; NaN and negatives give 0."""
    twice = 2.0 * np.asarray(med, dtype=np.float64)
    return np.where(twice > 0, twice, 0.0).astype(np.uint64)


def cells_from_frames(sample: int, refs, frames: Sequence[pd.DataFrame], want_abundance: bool) -> np.ndarray:
    """The cells of one sample from its own tables (one per user coverage, all over the references `refs`)."""
    refs = np.asarray(refs, dtype=np.int64)
    mask = np.zeros(refs.size, dtype=np.uint32)
    for c, df in enumerate(frames):
        mask |= df["in_sample_est"].to_numpy().astype(bool).astype(np.uint32) << np.uint32(c)
    at = np.flatnonzero(mask)
    cells = np.zeros(at.size, dtype=MATRIX_CELL_DTYPE)
    cells["sample"], cells["ref"], cells["mask"] = sample, refs[at], mask[at]
    cells["n_match"] = frames[0]["num_matches"].to_numpy()[at]
    if want_abundance:
        cells["depth2"] = depth2_of(frames[0]["abund_median_exclusive"].to_numpy(dtype=np.float64)[at])
    return cells


def _valid(cells, n_samples: int, skip, n_refs: int) -> np.ndarray:
    """The cells the passes take: sample and reference in range, the sample not skipped."""
    ok = (cells["sample"] < n_samples) & (cells["ref"] < n_refs)
    if skip is not None and n_samples:
        ok &= np.asarray(skip, dtype=np.uint8)[np.minimum(cells["sample"], n_samples - 1)] == 0
    return ok


def prevalence_numpy(cells, n_sets: int, n_samples: int, skip, n_refs: int):
    """What yh_matrix_prevalence_device writes: (prev uint32 [n_sets][N], denom uint64 [n_sets][n_samples])."""
    prev = np.zeros((n_sets, n_refs), dtype=np.uint32)
    denom = np.zeros((n_sets, n_samples), dtype=np.uint64)
    cells = cells[_valid(cells, n_samples, skip, n_refs)]
    for c in range(n_sets):
        sel = cells[((cells["mask"] >> np.uint32(c)) & np.uint32(1)).astype(bool)]
        prev[c] = np.bincount(sel["ref"], minlength=n_refs).astype(np.uint32)
        # depth2 < 2^34 in two halves of 17 bits: each half's float64 sum over up to 2^32 cells of a sample is exact
        lo = np.bincount(sel["sample"], weights=(sel["depth2"] & np.uint64(0x1FFFF)).astype(np.float64), minlength=n_samples)
        hi = np.bincount(sel["sample"], weights=(sel["depth2"] >> np.uint64(17)).astype(np.float64), minlength=n_samples)
        denom[c] = (hi.astype(np.uint64) << np.uint64(17)) + lo.astype(np.uint64)
    return prev, denom


def fill_numpy(cells, bit: int, n_samples: int, skip, row_of_ref, n_kept: int, denom_bit, want_rel: bool):
    """What yh_matrix_fill_device writes: (presence uint8, n_match uint32, rel float64 or None), each [n_kept][n_samples]."""
    row_of_ref = np.asarray(row_of_ref, dtype=np.int32)
    presence = np.zeros((n_kept, n_samples), dtype=np.uint8)
    n_match = np.zeros((n_kept, n_samples), dtype=np.uint32)
    rel = np.zeros((n_kept, n_samples), dtype=np.float64) if want_rel else None
    sel = cells[_valid(cells, n_samples, skip, row_of_ref.size)]
    sel = sel[((sel["mask"] >> np.uint32(bit)) & np.uint32(1)).astype(bool)]
    row = row_of_ref[sel["ref"]]
    sel, row = sel[(row >= 0) & (row < n_kept)], row[(row >= 0) & (row < n_kept)]
    presence[row, sel["sample"]] = 1
    n_match[row, sel["sample"]] = sel["n_match"]
    if want_rel:
        den = np.asarray(denom_bit, dtype=np.uint64)[sel["sample"]]
        with np.errstate(divide="ignore", invalid="ignore"):
            rel[row, sel["sample"]] = np.where(den != 0, sel["depth2"].astype(np.float64) / den.astype(np.float64), 0.0)
    return presence, n_match, rel


def row_of_ref_for(kept: np.ndarray) -> np.ndarray:
    """int32 [N]: the matrix row of every kept reference (database order), -1 for the others."""
    kept = np.asarray(kept, dtype=bool)
    out = np.full(kept.size, -1, dtype=np.int32)
    out[kept] = np.arange(int(kept.sum()), dtype=np.int32)
    return out


def reduce_rel(rel: np.ndarray, n_samples: int):
    """(mean over all samples, max) of every row of a C-contiguous [rows][n_samples] matrix: each row by itself, in numpy's
    fixed order, so a row's figures do not depend on which other rows came with it."""
    rel = np.ascontiguousarray(rel, dtype=np.float64)
    if rel.shape[0] == 0 or n_samples == 0:
        return np.zeros(rel.shape[0]), np.zeros(rel.shape[0])
    return rel.sum(axis=1) / float(n_samples), rel.max(axis=1)


# ---- the tables ----------------------------------------------------------------------------------------------------------
def prevalence_frame(names, user_covs, prev, n_samples: int, stats=None) -> pd.DataFrame:
    """cohort_prevalence.tsv: user_covs descending as the run holds them, prev [n_sets][N]; stats: per coverage (mean, max) over
    the references with prev >= 1, or None."""
    names = np.asarray(names, dtype=object)
    parts = []
    for c, cov in enumerate(user_covs):
        at = np.flatnonzero(prev[c])
        part = {"min_coverage": cov, "organism_name": names[at], "n_samples_present": prev[c][at].astype(np.int64),
                "f_samples_present": prev[c][at].astype(np.float64) / float(n_samples)}
        if stats is not None:
            part["mean_relative_abundance"], part["max_relative_abundance"] = stats[c]
        parts.append(pd.DataFrame(part))
    columns = PREVALENCE_COLUMNS + (PREVALENCE_ABUNDANCE_COLUMNS if stats is not None else [])
    return pd.concat(parts, ignore_index=True)[columns] if parts else pd.DataFrame(columns=columns)


def wide_frame(names, stems, values) -> pd.DataFrame:
    df = pd.DataFrame(values, columns=list(stems))
    df.insert(0, "organism_name", np.asarray(names, dtype=object), allow_duplicates=True)
    return df


def write_tables(folder: str, names, stems, user_covs, prev, kept, presence, n_match, rel, stats) -> None:
    names = np.asarray(names, dtype=object)
    prevalence_frame(names, user_covs, prev, len(stems), stats).to_csv(os.path.join(folder, PREVALENCE_NAME), sep="\t", index=False)
    rows = names[np.asarray(kept, dtype=bool)]
    wide_frame(rows, stems, presence).to_csv(os.path.join(folder, PRESENCE_NAME), sep="\t", index=False)
    wide_frame(rows, stems, n_match).to_csv(os.path.join(folder, NUM_MATCHES_NAME), sep="\t", index=False)
    if rel is not None:
        wide_frame(rows, stems, rel).to_csv(os.path.join(folder, ABUNDANCE_NAME), sep="\t", index=False)


def check_size(n_kept: int, n_samples: int, want_abundance: bool) -> None:
    need = int(n_kept) * int(n_samples) * (13 if want_abundance else 5)
    if need > MAX_BYTES:
        raise ValueError(MSG_TOO_LARGE.format(n_kept, n_samples, need, MAX_BYTES))


def _slabs(kept_at: np.ndarray, n_columns: int):
    step = max(1, SLAB_BYTES // (13 * max(n_columns, 1)))
    for lo in range(0, kept_at.size, step):
        yield kept_at[lo:lo + step]


def tables_numpy(cells: np.ndarray, n_refs: int, n_samples: int, n_sets: int, bit: int, min_samples: int, want_abundance: bool):
    """The numpy route over the whole cohort's cells: (prev, kept, presence, n_match, rel or None, stats or None)."""
    prev, denom = prevalence_numpy(cells, n_sets, n_samples, None, n_refs)
    kept = prev[bit] >= min_samples
    check_size(int(kept.sum()), n_samples, want_abundance)
    presence, n_match, rel = fill_numpy(cells, bit, n_samples, None, row_of_ref_for(kept), int(kept.sum()), denom[bit], want_abundance)
    stats = None
    if want_abundance:
        stats = []
        for c in range(n_sets):
            if c == bit and min_samples == 1:
                stats.append(reduce_rel(rel, n_samples))
                continue
            mean, mx = [], []
            for slab in _slabs(np.flatnonzero(prev[c]), n_samples):
                on = np.zeros(n_refs, dtype=bool)
                on[slab] = True
                m, x = reduce_rel(fill_numpy(cells, c, n_samples, None, row_of_ref_for(on), slab.size, denom[c], True)[2], n_samples)
                mean.append(m)
                mx.append(x)
            stats.append((np.concatenate(mean) if mean else np.zeros(0), np.concatenate(mx) if mx else np.zeros(0)))
    return prev, kept, presence, n_match, rel, stats


class Collector:
    """The cells of a cohort run: the device's, block behind block (device tensors int64 [n][3] = 24 bytes a cell), and the
    host-made ones (samples whose tables the host recomputed; every sample under YACHT_COHORT_MATRIX=host)."""

    def __init__(self, n_refs: int, n_samples: int, n_sets: int, want_abundance: bool, host_route: bool):
        self.n_refs, self.n_samples, self.n_sets = int(n_refs), int(n_samples), int(n_sets)
        self.want_abundance, self.host_route = bool(want_abundance), bool(host_route)
        self.device_cells: list = []
        self.host_cells: List[np.ndarray] = []
        self.alias: List[int] = []  # device route: the sample behind alias column n_samples + r

    def add_device(self, cells) -> None:
        self.device_cells.append(cells)

    def add_host(self, sample: int, refs, frames) -> None:
        cells = cells_from_frames(sample, refs, frames, self.want_abundance)
        if not self.host_route:  # the device made cells of this sample from rows the host did not use: skipped there
            cells["sample"] = self.n_samples + len(self.alias)
            self.alias.append(int(sample))
        self.host_cells.append(cells)

    def _host_all(self) -> np.ndarray:
        return np.concatenate(self.host_cells) if self.host_cells else np.zeros(0, dtype=MATRIX_CELL_DTYPE)

    def _fold(self, mat: Optional[np.ndarray]) -> Optional[np.ndarray]:
        """The alias columns back onto their samples' own."""
        if mat is None or not self.alias:
            return mat
        mat[:, self.alias] = mat[:, self.n_samples:]
        return np.ascontiguousarray(mat[:, :self.n_samples])

    def tables(self, bit: int, min_samples: int, db=None, torch=None, dev=None, timer=None):
        """(prev, kept, presence, n_match, rel or None, stats or None) of the cohort."""
        if self.host_route:
            return tables_numpy(self._host_all(), self.n_refs, self.n_samples, self.n_sets, bit, min_samples, self.want_abundance)
        t = torch
        S, N, n_sets = self.n_samples + len(self.alias), self.n_refs, self.n_sets
        host = self._host_all()
        parts = list(self.device_cells)
        if host.size:
            parts.append(t.from_numpy(host.view(np.int64).reshape(-1, 3)).to(dev))
        cells = t.cat(parts) if parts else t.zeros((0, 3), dtype=t.int64, device=dev)
        n_cells = int(cells.shape[0])
        skip_h = np.zeros(max(S, 1), dtype=np.uint8)
        skip_h[self.alias] = 1
        skip = t.from_numpy(skip_h).to(dev)
        prev_d = t.zeros((n_sets, max(N, 1)), dtype=t.int32, device=dev)
        denom_d = t.zeros((n_sets, max(S, 1)), dtype=t.int64, device=dev)
        ev = [t.cuda.Event(enable_timing=True) for _ in range(2)]
        ms = 0.0

        def timed(call):
            nonlocal ms
            ev[0].record()
            call()
            ev[1].record()
            db.synchronize()
            t.cuda.synchronize(dev)
            ms += ev[0].elapsed_time(ev[1])

        timed(lambda: db.matrix_prevalence_device(cells.data_ptr(), n_cells, n_sets, S, skip.data_ptr(), prev_d.data_ptr(), denom_d.data_ptr()))
        prev = prev_d[:, :N].cpu().numpy().view(np.uint32)

        def fill(c: int, on: np.ndarray, want_rel: bool):
            n_kept = int(on.sum())
            row_of = t.from_numpy(row_of_ref_for(on)).to(dev) if N else t.zeros(1, dtype=t.int32, device=dev)
            shape = (max(n_kept, 1), max(S, 1))
            p_d, m_d = t.empty(shape, dtype=t.uint8, device=dev), t.empty(shape, dtype=t.int32, device=dev)
            r_d = t.empty(shape, dtype=t.float64, device=dev) if want_rel else None
            timed(lambda: db.matrix_fill_device(cells.data_ptr(), n_cells, c, S, skip.data_ptr(), row_of.data_ptr(), n_kept,
                                                denom_d[c].data_ptr(), p_d.data_ptr(), m_d.data_ptr(), r_d.data_ptr() if want_rel else 0))
            return (self._fold(p_d[:n_kept, :S].cpu().numpy()), self._fold(m_d[:n_kept, :S].cpu().numpy().view(np.uint32)),
                    self._fold(r_d[:n_kept, :S].cpu().numpy()) if want_rel else None)

        kept = prev[bit] >= min_samples
        check_size(int(kept.sum()), self.n_samples, self.want_abundance)
        presence, n_match, rel = fill(bit, kept, self.want_abundance)
        stats = None
        if self.want_abundance:
            stats = []
            for c in range(n_sets):
                if c == bit and min_samples == 1:
                    stats.append(reduce_rel(rel, self.n_samples))
                    continue
                mean, mx = [], []
                for slab in _slabs(np.flatnonzero(prev[c]), S):
                    on = np.zeros(N, dtype=bool)
                    on[slab] = True
                    m, x = reduce_rel(fill(c, on, True)[2], self.n_samples)
                    mean.append(m)
                    mx.append(x)
                stats.append((np.concatenate(mean) if mean else np.zeros(0), np.concatenate(mx) if mx else np.zeros(0)))
        if timer is not None:
            timer["gpu_matrix"] += ms / 1e3
        return prev, kept, presence, n_match, rel, stats

    def finish(self, folder: str, names, stems, user_covs, coverage: float, min_samples: int, db=None, torch=None, dev=None,
               timer=None) -> None:
        """The cohort's tables into `folder`; timer["gpu_matrix"] gains the passes' device time, timer["matrix_files"] the writes."""
        bit = [float(c) for c in user_covs].index(float(coverage))
        prev, kept, presence, n_match, rel, stats = self.tables(bit, min_samples, db, torch, dev, timer)
        t0 = time.perf_counter()
        write_tables(folder, names, stems, user_covs, prev, kept, presence, n_match, rel, stats)
        if timer is not None:
            timer["matrix_files"] += time.perf_counter() - t0
