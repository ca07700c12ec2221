"""`yacht run --abundance`: per-organism depth columns from the sample's per-hash abundances.

The device answers three numbers per reference (RefDB.abundance / yh_abund): the abundance-weighted overlap, the
abundance-weighted exclusive matches and the median abundance of the exclusive matches.  The set behind the last two is the
one `yacht run` already counts as num_matches: a sample hash that two references hold gives both of them overlap, so both
are in the run's subset, and a sample hash is exclusive to a reference exactly when that reference is its only holder in
the database.  Everything here is numpy / pandas on those numbers: no device, no library call.
"""
from __future__ import annotations

import os
from typing import List, Sequence

import numpy as np
import pandas as pd

ABUNDANCE_COLUMNS = [
    "abund_sum_overlap",
    "abund_mean_overlap",
    "abund_sum_exclusive",
    "abund_mean_exclusive",
    "abund_median_exclusive",
    "f_weighted_overlap",
    "relative_abundance",
]
PROFILE_COLUMNS = ["min_coverage", "organism_name", "num_matches", "abund_sum_exclusive", "abund_mean_exclusive",
                   "abund_median_exclusive", "relative_abundance"]
PROFILE_NAME = "abundance_profile.tsv"
MSG_NO_ABUNDANCE = ("--abundance needs per-hash abundances, and the sketch in {0} has none. "
                    "Sketch the sample with abundance tracking (`yacht sketch sample` does).")


def sample_abundances(sample_sig, path: str) -> np.ndarray:
    """The per-hash abundances of a sample's sketch, in the order of its hashes; ValueError naming the file when the
    sketch has none or they do not match the hashes."""
    mh = sample_sig.minhash
    ab = mh.abundances if mh.mean_abundance is not None else None
    if ab is None:
        raise ValueError(MSG_NO_ABUNDANCE.format(path))
    ab = np.asarray(ab)
    if ab.size != len(mh):
        raise ValueError(f"{path}: {ab.size} abundances for {len(mh)} hashes")
    return ab


def abundance_columns(w_overlap, w_match, med_match, intersect_hashes, num_matches, in_sample_est, total_abundance) -> pd.DataFrame:
    """The seven abundance columns of one coverage table, one row per organism of the table (ABUNDANCE_COLUMNS order).
    w_overlap / w_match / med_match: the device's numbers for those rows; intersect_hashes / num_matches: the overlap and
    exclusive-match COUNTS of the same step; in_sample_est: this coverage's presence calls; total_abundance: the sum of
    the abundances of the whole sample.  Means and the median are NaN where their count is 0; relative_abundance is the
    median over the sum of the medians of the rows present in this table, 0 for rows not present."""
    w_ov = np.asarray(w_overlap, dtype=np.uint64)
    w_m = np.asarray(w_match, dtype=np.uint64)
    med = np.asarray(med_match, dtype=np.float64)
    n_ov = np.asarray(intersect_hashes, dtype=np.float64)
    n_m = np.asarray(num_matches, dtype=np.float64)
    present = np.asarray(in_sample_est, dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean_ov = np.where(n_ov > 0, w_ov.astype(np.float64) / n_ov, np.nan)
        mean_m = np.where(n_m > 0, w_m.astype(np.float64) / n_m, np.nan)
        f_w = w_ov.astype(np.float64) / float(total_abundance) if total_abundance else np.zeros(w_ov.size)
    med = np.where(n_m > 0, med, np.nan)
    depth = np.where(present & (n_m > 0), med, 0.0)
    total = float(depth.sum())
    rel = depth / total if total > 0 else np.zeros(depth.size)
    return pd.DataFrame({"abund_sum_overlap": w_ov, "abund_mean_overlap": mean_ov, "abund_sum_exclusive": w_m,
                         "abund_mean_exclusive": mean_m, "abund_median_exclusive": med, "f_weighted_overlap": f_w,
                         "relative_abundance": rel}, columns=ABUNDANCE_COLUMNS)


def append_columns(frame: pd.DataFrame, w_overlap, w_match, med_match, intersect_hashes, total_abundance) -> pd.DataFrame:
    """A coverage table (hypothesis_recovery_src.coverage_frame) with the abundance columns behind its hypothesis columns."""
    cols = abundance_columns(w_overlap, w_match, med_match, intersect_hashes, frame["num_matches"].to_numpy(),
                             frame["in_sample_est"].to_numpy(), total_abundance)
    return pd.concat([frame, cols], axis=1)


def profile_frame(results: Sequence[pd.DataFrame], covs: Sequence[float]) -> pd.DataFrame:
    """One row per (coverage, present organism) from the coverage tables: coverage descending, then relative_abundance
    descending (ties keep the table's order)."""
    parts: List[pd.DataFrame] = []
    for cov, df in sorted(zip(covs, results), key=lambda t: -float(t[0])):
        hit = df[df["in_sample_est"] == True]  # noqa: E712
        part = hit[[c for c in PROFILE_COLUMNS if c != "min_coverage"]].copy()
        part.insert(0, "min_coverage", cov)
        parts.append(part.sort_values("relative_abundance", ascending=False, kind="stable"))
    if not parts:
        return pd.DataFrame(columns=PROFILE_COLUMNS)
    return pd.concat(parts, ignore_index=True)[PROFILE_COLUMNS]


def write_profile(results: Sequence[pd.DataFrame], covs: Sequence[float], results_folder: str) -> None:
    profile_frame(results, covs).to_csv(os.path.join(results_folder, PROFILE_NAME), sep="\t", index=False)
